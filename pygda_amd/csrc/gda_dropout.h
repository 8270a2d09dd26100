// The dropout keep-bit stream of the fused activation kernels, stated once (gfx950).
//
// Every kernel that draws a mask, fuses the activation into an epilogue or regenerates a mask in its backward pass
// promises "same masks, same values as k_relu_dropout_fwd (gda_act.hip)".  The format behind that promise:
//   key        Philox-4x32-10 (gda_philox.h) keyed on the caller's seed, counter = ((step << 20) ^ site, quad): `step` is the
//              trainer's device step counter, `site` numbers the masking calls inside one step.
//   quad       row-major element index >> 2.  The row kernels of the two discriminators (gda_critic.hip,
//              gda_disc_mlp.hip) use row_in_domain * a + unit as the element index.
//   threshold  floor(min(p * 2^32, 2^32 - 1)).
//   rule       element e of a quad is kept when word e & 3 of the draw is >= threshold; a kept value is v * 1 / (1 - p).
// tests/test_gpu_parity.py::test_dropout_keep_bits_are_the_documented_philox_stream pins it against a numpy Philox.
// What a kernel does at p <= 0 (draw anyway, skip the draw, keep a NaN) is its own business and stays in the kernel.
// Not here: gda_asn.hip's reparameterisation noise and dropout -- another key layout (site << 32 ^ step * constant) and a
// float comparison; they call GdaPhilox::gen themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gda_philox.h"

__device__ __forceinline__ uint32_t dropout_thresh(float p) {
    const double t = (double)p * 4294967296.0;
    return (uint32_t)(t > 4294967295.0 ? 4294967295.0 : t);
}

// the four words of quad `quad` at call site `site` of step `step`: the only place that lays out the key
__device__ __forceinline__ void dropout_draw(uint64_t seed, uint64_t step, uint32_t site, uint64_t quad, uint32_t (&r)[4]) {
    GdaPhilox::gen(seed, (step << 20) ^ site, quad, r);
}

// the keep rule: the word of an element against the threshold
__device__ __forceinline__ bool dropout_kept(uint32_t r, uint32_t thresh) { return r >= thresh; }

// forward: (v > 0 && kept) ? v * scale : 0 -- drop(relu(v)) of one value against its word, of a quad against its draw.
// v > 0 is false for a NaN: it reads as 0.  The scalar form is two selects over dropout_kept, the quad form one && per
// element with the comparison written out: the same function of the same inputs.  Writing both the same way, or the quad
// form over dropout_kept, changes the code length (and the SGPR count) of k_relu_dropout_fwd, k_relu_dropout_fwd_T,
// k_il_finish_act or k_tall_fwd_h against the code they replaced (profiles/dropout_header_ab.txt) and nothing else: no
// value, no mask.  Unifying them is a matter of that table, not of behaviour.
__device__ __forceinline__ float relu_keep(float v, uint32_t r, uint32_t thresh, float scale) {
    return v > 0.f ? (dropout_kept(r, thresh) ? v * scale : 0.f) : 0.f;
}

__device__ __forceinline__ float4 relu_keep(float4 v, const uint32_t (&r)[4], uint32_t thresh, float scale) {
    float4 o;
    o.x = (v.x > 0.f && r[0] >= thresh) ? v.x * scale : 0.f;
    o.y = (v.y > 0.f && r[1] >= thresh) ? v.y * scale : 0.f;
    o.z = (v.z > 0.f && r[2] >= thresh) ? v.z * scale : 0.f;
    o.w = (v.w > 0.f && r[3] >= thresh) ? v.w * scale : 0.f;
    return o;
}

// backward: y > 0 <=> the input was positive and kept, so the output is its own mask
__device__ __forceinline__ float4 relu_keep_bwd(float4 y, float4 g, float scale) {
    return make_float4(y.x > 0.f ? g.x * scale : 0.f, y.y > 0.f ? g.y * scale : 0.f,
                       y.z > 0.f ? g.z * scale : 0.f, y.w > 0.f ? g.w * scale : 0.f);
}

// generator arguments of a discriminator row kernel: its masks use the sites site, site + 1, ...
struct GdaDrop {
    float p; uint64_t seed; const int64_t* step; uint32_t site;
};

// keep-factor of hidden unit k of row `row` (numbered inside its domain) of an [., a] hidden layer: 0 or 1 / (1 - p)
__device__ __forceinline__ float keep_factor(const GdaDrop& dr, uint64_t st, uint32_t site, int64_t row, int a, int k) {
    if (dr.p <= 0.f) return 1.f;
    const uint64_t e = (uint64_t)row * (uint64_t)a + (uint64_t)k;
    uint32_t r[4];
    dropout_draw(dr.seed, st, site, e >> 2, r);
    return dropout_kept(r[e & 3], dropout_thresh(dr.p)) ? 1.f / (1.f - dr.p) : 0.f;
}

// activation arguments of a producer's epilogue: y0 = drop_site0(relu(v)) and, where the kernel has a second output,
// y1 = drop_site1(relu(v)), an independent draw of the same pre-activation.  p = 0: relu only.
struct GdaAct {
    float p, scale;
    uint64_t seed;
    const int64_t* step;
    uint32_t site0, site1;
};

__host__ inline GdaAct gda_act(float p, uint64_t seed, const int64_t* step, uint32_t site0, uint32_t site1) {
    return GdaAct{p > 0.f ? p : 0.f, p > 0.f ? 1.f / (1.f - p) : 1.f, seed, step, site0, site1};
}
