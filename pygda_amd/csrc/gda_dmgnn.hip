// DMGNN for gfx950 (pygda/models/dmgnn.py on pygda/nn/acdne_base.py): the per-step losses and predict's propagation.
// process_graph, the batch indices and the network are ACDNE's (gda_acdne.hip); the layout conventions are the same:
// dense fp32 PPMI of leading dimension ld = round_up(N, 4), pidx per domain, an index outside the domain reads zero.
//
// Per step (b = 2 h rows: h source rows, then h target rows):
//   k_dm_prox   one workgroup per domain, three phases behind workgroup barriers: the h x h block of A_ppmi at the
//               batch's PPMI indices (ppmi_block_entry; row sum in double by one lane, rows in order, scale rounded to
//               fp32, as gda_acdne.hip's k_prox_rows) written NORMALISED to a_blocks; D = E - A E with E = relu(z) and
//               |D|_F^2 in double (lane partials, fixed tree); gz = pair_weight (D - A^T D) / (h |D|_F), zero where the
//               norm is zero.  One lane per output element, its sum over j in increasing order.
//   The heads (gda_dmgnn_heads_f32) are gda_acdne.hip's k_heads with the source half's block as a_s.
// predict:
//   P = softmax(relu(z) Wc^T + bc) into the workspace by gda_acdne_predict_f32, then
//   k_dm_prop   out = P + M P, one streaming pass over M: a wave owns PROP_R rows, a lane four contiguous columns per
//               256-column slice (16-byte loads), P goes through LDS in tiles of PROP_JT columns as [class][column].
//               A lane adds its columns in increasing order, then the xor butterfly over the wave: a fixed order.
//               Columns >= n (the padding of ld) are never used.  c <= 8; wider heads take k_dm_prop_wide (a wave per
//               row, a pass over the row per class).
// Every reduction has a fixed order that depends on the shapes only: two runs are bit-identical.  No atomics.
#include "gda_common.h"
#include "gda_ppmi_block.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int PROX_TB = 1024;               // k_dm_prox: one workgroup per domain
constexpr int PROP_TB = 512;                // k_dm_prop: 8 waves
constexpr int PROP_R = 4;                   // rows per wave
constexpr int PROP_JT = 1024;               // columns of P per LDS tile
constexpr int PROP_CMAX = 8;                // classes held in registers

// workspace of the proximity loss: D [2, h, e]
__global__ void __launch_bounds__(PROX_TB) k_dm_prox(const float* __restrict__ ppmi_s, int64_t ld_s, int ns,
                                                     const float* __restrict__ ppmi_t, int64_t ld_t, int nt,
                                                     const int64_t* __restrict__ pidx, const float* __restrict__ z,
                                                     int h, int e, float pair_weight, float* __restrict__ a_blocks,
                                                     float* __restrict__ dws, double* __restrict__ loss,
                                                     float* __restrict__ gz) {
    __shared__ double red[PROX_TB];
    const int dom = blockIdx.x, t = threadIdx.x;
    const float* P = dom ? ppmi_t : ppmi_s;
    const int64_t ld = dom ? ld_t : ld_s;
    const int np = dom ? nt : ns;
    const int64_t* idx = pidx + (int64_t)dom * h;
    float* A = a_blocks + (int64_t)dom * h * h;
    const float* Z = z + (int64_t)dom * h * e;
    float* D = dws + (int64_t)dom * h * e;
    float* G = gz + (int64_t)dom * h * e;
    // the gathered block
    for (int p = t; p < h * h; p += PROX_TB) A[p] = ppmi_block_entry(P, ld, np, idx, p / h, p % h);
    __syncthreads();
    // its rows scaled by 1 / (fp32(double row sum) + 1e-12): a lane per row, the entries in order
    float rinv = 0.f;
    if (t < h) {
        double s = 0.0;
        for (int j = 0; j < h; ++j) s += (double)A[t * h + j];
        rinv = 1.f / ((float)s + 1e-12f);
    }
    __syncthreads();
    if (t < h)
        for (int j = 0; j < h; ++j) A[t * h + j] = rinv * A[t * h + j];
    __syncthreads();
    // D = E - A E and the square of its norm
    double sq = 0.0;
    for (int p = t; p < h * e; p += PROX_TB) {
        const int i = p / e, c = p % e;
        float s = 0.f;
        for (int j = 0; j < h; ++j) s += A[i * h + j] * fmaxf(Z[(int64_t)j * e + c], 0.f);
        const float d = fmaxf(Z[p], 0.f) - s;
        D[p] = d;
        sq += (double)d * (double)d;
    }
    const double nrm = sqrt(block_sum_d(sq, red));           // (the barriers inside publish D to the workgroup)
    if (t == 0) loss[dom] = nrm / (double)h;
    const float scale = nrm > 0.0 ? (float)((double)pair_weight / ((double)h * nrm)) : 0.f;
    for (int p = t; p < h * e; p += PROX_TB) {
        const int k = p / e, c = p % e;
        float s = 0.f;
        for (int i = 0; i < h; ++i) s += A[i * h + k] * D[(int64_t)i * e + c];
        G[p] = nrm > 0.0 ? scale * (D[p] - s) : 0.f;
    }
}

template <int CT>
__global__ void __launch_bounds__(PROP_TB) k_dm_prop(const float* __restrict__ M, int64_t ld, int n,
                                                     const float* __restrict__ P, int C, float* __restrict__ out) {
    __shared__ float tile[CT * PROP_JT];               // [class][column of the tile]
    const int t = threadIdx.x, lane = t & (GDA_WAVE - 1), wave = t / GDA_WAVE;
    const int r0 = (blockIdx.x * (PROP_TB / GDA_WAVE) + wave) * PROP_R;
    float acc[PROP_R][CT];
#pragma unroll
    for (int r = 0; r < PROP_R; ++r)
#pragma unroll
        for (int o = 0; o < CT; ++o) acc[r][o] = 0.f;
    for (int j0 = 0; j0 < n; j0 += PROP_JT) {
        __syncthreads();
        for (int q = t; q < PROP_JT * C; q += PROP_TB) {
            const int j = q / C, o = q % C;
            tile[o * PROP_JT + j] = j0 + j < n ? P[(int64_t)(j0 + j) * C + o] : 0.f;
        }
        __syncthreads();
        if (r0 >= n) continue;                         // (a wave without rows still takes the barriers)
        for (int s = 0; s < PROP_JT; s += 4 * GDA_WAVE) {
            const int jl = s + 4 * lane, j = j0 + jl;
            if (j >= n) continue;
            float4 p[CT];
#pragma unroll
            for (int o = 0; o < CT; ++o)
                p[o] = o < C ? *reinterpret_cast<const float4*>(tile + o * PROP_JT + jl) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int r = 0; r < PROP_R; ++r) {
                if (r0 + r >= n) continue;
                float4 mv = *reinterpret_cast<const float4*>(M + (int64_t)(r0 + r) * ld + j);   // j + 3 < ld
                if (j + 1 >= n) mv.y = 0.f;            // the padding columns hold anything
                if (j + 2 >= n) mv.z = 0.f;
                if (j + 3 >= n) mv.w = 0.f;
#pragma unroll
                for (int o = 0; o < CT; ++o) {
                    acc[r][o] += mv.x * p[o].x;
                    acc[r][o] += mv.y * p[o].y;
                    acc[r][o] += mv.z * p[o].z;
                    acc[r][o] += mv.w * p[o].w;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PROP_R; ++r) {
        if (r0 + r >= n) continue;
#pragma unroll
        for (int o = 0; o < CT; ++o) {
            const float s = wave_sum(acc[r][o]);
            if (lane == 0 && o < C) out[(int64_t)(r0 + r) * C + o] = P[(int64_t)(r0 + r) * C + o] + s;
        }
    }
}

__global__ void __launch_bounds__(TB) k_dm_prop_wide(const float* __restrict__ M, int64_t ld, int n,
                                                     const float* __restrict__ P, int C, float* __restrict__ out) {
    const int lane = threadIdx.x & (GDA_WAVE - 1);
    const int i = blockIdx.x * (TB / GDA_WAVE) + threadIdx.x / GDA_WAVE;
    if (i >= n) return;
    const float* row = M + (int64_t)i * ld;
    for (int o = 0; o < C; ++o) {
        float s = 0.f;
        for (int j = lane; j < n; j += GDA_WAVE) s += row[j] * P[(int64_t)j * C + o];
        s = wave_sum(s);
        if (lane == 0) out[(int64_t)i * C + o] = P[(int64_t)i * C + o] + s;
    }
}

}  // namespace

extern "C" size_t gda_dmgnn_prox_workspace_bytes(int64_t h, int64_t e) {
    if (h < 1 || e < 1) return 256;
    return (size_t)(2 * h * e) * sizeof(float);
}

extern "C" int gda_dmgnn_prox_f32(const float* ppmi_s, int64_t ld_s, int64_t ns, const float* ppmi_t, int64_t ld_t,
                                  int64_t nt, const int64_t* pidx, const float* z, int64_t h, int64_t e,
                                  float pair_weight, double* loss, float* gz, float* a_blocks, void* workspace,
                                  size_t workspace_bytes, gda_stream_t stream) {
    if (h < 1 || h > GDA_ACDNE_MAX_HALF || e < 1 || e > 4096 || ns < 1 || nt < 1 || ns >= INT32_MAX ||
        nt >= INT32_MAX || ld_s < ns || ld_t < nt)
        return GDA_E_SIZE;
    if (!ppmi_s || !ppmi_t || !pidx || !z || !loss || !gz || !a_blocks || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_dmgnn_prox_workspace_bytes(h, e)) return GDA_E_WORKSPACE;
    k_dm_prox<<<2, PROX_TB, 0, (hipStream_t)stream>>>(ppmi_s, ld_s, (int)ns, ppmi_t, ld_t, (int)nt, pidx, z, (int)h,
                                                      (int)e, pair_weight, a_blocks, static_cast<float*>(workspace),
                                                      loss, gz);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_dmgnn_predict_workspace_bytes(int64_t n, int64_t c) {
    if (n < 1 || c < 1) return 256;
    return (size_t)(n * c) * sizeof(float);
}

extern "C" int gda_dmgnn_predict_f32(const float* z, int64_t n, int64_t e, const float* wc, const float* bc, int64_t c,
                                     const float* ppmi, int64_t ld, float* out, void* workspace,
                                     size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX / 2 || e < 1 || c < 1 || c > 4096 || e > 4096 || ld < n) return GDA_E_SIZE;
    if (!z || !wc || !bc || !ppmi || !out || !workspace) return GDA_E_NULL;
    if (ld % 4 != 0 || reinterpret_cast<uintptr_t>(ppmi) % 16 != 0) return GDA_E_UNSUPPORTED;   // 16-byte loads
    if (workspace_bytes < gda_dmgnn_predict_workspace_bytes(n, c)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* prob = static_cast<float*>(workspace);
    const int st = gda_acdne_predict_f32(z, n, e, wc, bc, c, prob, stream);     // the softmax rows P
    if (st != GDA_OK) return st;
    if (c <= 4) {
        const unsigned blocks = (unsigned)gda_cdiv(n, (PROP_TB / GDA_WAVE) * PROP_R);
        k_dm_prop<4><<<blocks, PROP_TB, 0, s>>>(ppmi, ld, (int)n, prob, (int)c, out);
    } else if (c <= PROP_CMAX) {
        const unsigned blocks = (unsigned)gda_cdiv(n, (PROP_TB / GDA_WAVE) * PROP_R);
        k_dm_prop<PROP_CMAX><<<blocks, PROP_TB, 0, s>>>(ppmi, ld, (int)n, prob, (int)c, out);
    } else {
        k_dm_prop_wide<<<(unsigned)gda_cdiv(n, TB / GDA_WAVE), TB, 0, s>>>(ppmi, ld, (int)n, prob, (int)c, out);
    }
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
