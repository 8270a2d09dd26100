// DMGNN for gfx950 (pygda/models/dmgnn.py on pygda/nn/acdne_base.py): the per-step losses and predict's propagation.
// process_graph, the batch indices and the network are ACDNE's (gda_acdne.hip); the layout conventions are the same:
// dense fp32 PPMI of leading dimension ld = round_up(N, 4), pidx per domain, an index outside the domain reads zero.
//
// Per step (b = 2 h rows: h source rows, then h target rows):
//   k_dm_prox   one workgroup per domain, three phases behind workgroup barriers: the h x h block of A_ppmi at the
//               batch's PPMI indices (zero diagonal, row sum in double by one lane, rows in order, scale rounded to
//               fp32 -- gda_acdne.hip's k_prox_rows) written NORMALISED to a_blocks; D = E - A E with E = relu(z) and
//               |D|_F^2 in double (lane partials, fixed tree); gz = pair_weight (D - A^T D) / (h |D|_F), zero where the
//               norm is zero.  One lane per output element, its sum over j in increasing order.
//   k_dm_heads  gda_acdne.hip's k_heads with the propagation: six launches of one kernel, one phase each.  The
//               classifier logits L of the source half (phase 0), L' = L + A_s L and its CE per row (phase 2),
//               dL = dL' + A_s^T dL' (phase 3), then gWc, gbc (phase 4) and dz (phase 5) from dL.  The target half's
//               propagated logits enter no loss and are not formed.
// predict:
//   k_dm_prob   one lane per row: P = softmax(relu(z) Wc^T + bc) (k_predict of gda_acdne.hip) into the workspace.
//   k_dm_prop   out = P + M P, one streaming pass over M: a wave owns PROP_R rows, a lane four contiguous columns per
//               256-column slice (16-byte loads), P goes through LDS in tiles of PROP_JT columns as [class][column].
//               A lane adds its columns in increasing order, then the xor butterfly over the wave: a fixed order.
//               Columns >= n (the padding of ld) are never used.  c <= 8; wider heads take k_dm_prop_wide (a wave per
//               row, a pass over the row per class).
// Every reduction has a fixed order that depends on the shapes only: two runs are bit-identical.  No atomics.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int PROX_TB = 1024;               // k_dm_prox: one workgroup per domain
constexpr int HEAD_MAX_BLOCKS = 1024;       // k_dm_heads: grid cap (the grid strides over the work items)
constexpr int DH = 128;                     // discriminator width (DomainDiscriminator)
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
    for (int p = t; p < h * h; p += PROX_TB) {
        const int i = p / h, j = p % h;
        const int64_t gi = idx[i], gj = idx[j];
        const bool ok = j != i && gi >= 0 && gi < np && gj >= 0 && gj < np;   // (an index out of range reads 0)
        A[p] = ok ? P[gi * ld + gj] : 0.f;
    }
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

struct HeadArgs {
    const float* z;            // [m, e] pre-activation of emb
    const float* gprox;        // [m, e] proximity gradient w.r.t. emb
    const float* a_s;          // [h, h] the source half's normalised block
    const float *wc, *bc, *w1, *b1, *w2, *b2, *w3, *b3;
    const int64_t* y;          // [ny] source labels
    const int64_t* rows;       // [m] batch rows: the first h index y
    int64_t ny;
    const float* alpha;        // device scalar
    const double* prox;        // [2] proximity losses of the two domains
    float pair_weight;
    int h, e, c;
    float* ws;                 // emb [m e] | h1 [m DH] | h2 [m DH] | L [h c] | dLp [h c] | dL [h c] | dd [m 2] | dh2 | dh1
    double* terms;             // [h + m]: per-row CE terms (classifier, then domain)
    float* dz;                 // [m, e]
    float *gwc, *gbc, *gw1, *gb1, *gw2, *gb2, *gw3, *gb3;
    double* loss;              // [1]
    double* loss_acc;          // [1] or null: += loss
};

__host__ __device__ inline int64_t heads_ws_floats(int64_t h, int64_t e, int64_t c) {
    const int64_t m = 2 * h;
    return m * e + 4 * m * DH + 3 * h * c + 2 * m;
}

// One phase of the heads per launch; a phase is a list of independent work items (one output element each, its sum in
// a fixed order) spread over the whole grid.  Phase k reads only what phases < k wrote.
__global__ void __launch_bounds__(TB) k_dm_heads(HeadArgs A, int phase) {
    const int m = 2 * A.h, e = A.e, C = A.c, h = A.h;
    float* emb = A.ws;
    float* h1 = emb + (int64_t)m * e;
    float* h2 = h1 + (int64_t)m * DH;
    float* L = h2 + (int64_t)m * DH;
    float* dlp = L + (int64_t)h * C;
    float* dl = dlp + (int64_t)h * C;
    float* dd = dl + (int64_t)h * C;
    float* dh2 = dd + (int64_t)m * 2;
    float* dh1 = dh2 + (int64_t)m * DH;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (phase == 0) {                                  // emb = relu(z); h1 = relu(emb W1^T + b1); L = emb Wc^T + bc
        const int64_t n0 = (int64_t)m * e, n1 = n0 + (int64_t)m * DH, n2 = n1 + (int64_t)h * C;
        for (int64_t p = t0; p < n2; p += stride) {
            if (p < n0) {
                emb[p] = fmaxf(A.z[p], 0.f);
            } else if (p < n1) {
                const int64_t q = p - n0;
                const int i = (int)(q / DH), o = (int)(q % DH);
                float s = 0.f;
                for (int k = 0; k < e; ++k) s += fmaxf(A.z[(int64_t)i * e + k], 0.f) * A.w1[(int64_t)o * e + k];
                h1[q] = fmaxf(s + A.b1[o], 0.f);
            } else {
                const int64_t q = p - n1;
                const int i = (int)(q / C), o = (int)(q % C);
                float s = 0.f;
                for (int k = 0; k < e; ++k) s += fmaxf(A.z[(int64_t)i * e + k], 0.f) * A.wc[(int64_t)o * e + k];
                L[q] = s + A.bc[o];
            }
        }
    } else if (phase == 1) {                           // h2 = relu(h1 W2^T + b2)
        for (int64_t p = t0; p < (int64_t)m * DH; p += stride) {
            const int i = (int)(p / DH), o = (int)(p % DH);
            float s = 0.f;
            for (int k = 0; k < DH; ++k) s += h1[i * DH + k] * A.w2[o * DH + k];
            h2[p] = fmaxf(s + A.b2[o], 0.f);
        }
    } else if (phase == 2) {                           // per row: the domain CE (rows < h: class 0); L' and its CE
        for (int64_t p = t0; p < m; p += stride) {
            const int i = (int)p;
            float d[2];
            for (int o = 0; o < 2; ++o) {
                float s = 0.f;
                for (int k = 0; k < DH; ++k) s += h2[i * DH + k] * A.w3[o * DH + k];
                d[o] = s + A.b3[o];
            }
            const float mx = fmaxf(d[0], d[1]);
            const float lse = mx + logf(expf(d[0] - mx) + expf(d[1] - mx));
            const int lab = i < h ? 0 : 1;
            A.terms[h + i] = (double)(lse - d[lab]);
            for (int o = 0; o < 2; ++o) dd[i * 2 + o] = (expf(d[o] - lse) - (o == lab ? 1.f : 0.f)) / (float)m;
            if (i < h) {
                const int64_t r = A.rows[i];
                const int64_t y = (r >= 0 && r < A.ny) ? A.y[r] : -1;
                float cm = -INFINITY;
                for (int o = 0; o < C; ++o) {
                    float s = 0.f;
                    for (int j = 0; j < h; ++j) s += A.a_s[i * h + j] * L[j * C + o];
                    s = L[i * C + o] + s;
                    dlp[i * C + o] = s;
                    cm = fmaxf(cm, s);
                }
                float cs = 0.f;
                for (int o = 0; o < C; ++o) cs += expf(dlp[i * C + o] - cm);
                const float clse = cm + logf(cs);
                float ty = 0.f;
                for (int o = 0; o < C; ++o) {
                    const float lo = dlp[i * C + o];
                    if (o == y) ty = lo;
                    dlp[i * C + o] = (expf(lo - clse) - (o == y ? 1.f : 0.f)) / (float)h;
                }
                A.terms[i] = (double)(clse - ty);
            }
        }
    } else if (phase == 3) {                           // dh2, gW3, gb3; dL = dL' + A_s^T dL'; the loss
        const int64_t n0 = (int64_t)m * DH, n1 = n0 + 2 * DH, n2 = n1 + 2, n3 = n2 + (int64_t)h * C;
        for (int64_t p = t0; p <= n3; p += stride) {
            if (p < n0) {
                const int i = (int)(p / DH), k = (int)(p % DH);
                const float g = dd[i * 2] * A.w3[k] + dd[i * 2 + 1] * A.w3[DH + k];
                dh2[p] = h2[p] > 0.f ? g : 0.f;
            } else if (p < n1) {
                const int q = (int)(p - n0), o = q / DH, k = q % DH;
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dd[i * 2 + o] * h2[i * DH + k];
                A.gw3[q] = s;
            } else if (p < n2) {
                const int o = (int)(p - n1);
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dd[i * 2 + o];
                A.gb3[o] = s;
            } else if (p < n3) {
                const int q = (int)(p - n2), i = q / C, o = q % C;
                float s = 0.f;
                for (int k = 0; k < h; ++k) s += A.a_s[k * h + i] * dlp[k * C + o];
                dl[q] = dlp[q] + s;
            } else {
                double clf = 0.0, dom = 0.0;
                for (int i = 0; i < h; ++i) clf += A.terms[i];
                for (int i = 0; i < m; ++i) dom += A.terms[h + i];
                const double dom32 = (double)(float)(dom / (double)m);
                const double total = clf / (double)h + dom32 + (double)A.pair_weight * (A.prox[0] + A.prox[1]);
                A.loss[0] = total;
                if (A.loss_acc) A.loss_acc[0] += total;
            }
        }
    } else if (phase == 4) {                           // dh1 = (dh2 W2) * (h1 > 0); gW2; gb2; gWc; gbc
        const int64_t n0 = (int64_t)m * DH, n1 = n0 + DH * DH, n2 = n1 + DH, n3 = n2 + (int64_t)C * e, n4 = n3 + C;
        for (int64_t p = t0; p < n4; p += stride) {
            if (p < n0) {
                const int i = (int)(p / DH), k = (int)(p % DH);
                float g = 0.f;
                for (int o = 0; o < DH; ++o) g += dh2[i * DH + o] * A.w2[o * DH + k];
                dh1[p] = h1[p] > 0.f ? g : 0.f;
            } else if (p < n1) {
                const int q = (int)(p - n0), o = q / DH, k = q % DH;
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dh2[i * DH + o] * h1[i * DH + k];
                A.gw2[q] = s;
            } else if (p < n2) {
                const int o = (int)(p - n1);
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dh2[i * DH + o];
                A.gb2[o] = s;
            } else if (p < n3) {
                const int64_t q = p - n2;
                const int o = (int)(q / e), k = (int)(q % e);
                float s = 0.f;
                for (int i = 0; i < h; ++i) s += dl[i * C + o] * emb[(int64_t)i * e + k];
                A.gwc[q] = s;
            } else {
                const int o = (int)(p - n3);
                float s = 0.f;
                for (int i = 0; i < h; ++i) s += dl[i * C + o];
                A.gbc[o] = s;
            }
        }
    } else {                                           // gW1; gb1; dz = (dL Wc - alpha dh1 W1 + gprox) * (z > 0)
        const int64_t n0 = (int64_t)DH * e, n1 = n0 + DH, n2 = n1 + (int64_t)m * e;
        const float alpha = A.alpha[0];
        for (int64_t p = t0; p < n2; p += stride) {
            if (p < n0) {
                const int o = (int)(p / e), k = (int)(p % e);
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dh1[i * DH + o] * emb[(int64_t)i * e + k];
                A.gw1[p] = s;
            } else if (p < n1) {
                const int o = (int)(p - n0);
                float s = 0.f;
                for (int i = 0; i < m; ++i) s += dh1[i * DH + o];
                A.gb1[o] = s;
            } else {
                const int64_t q = p - n1;
                const int i = (int)(q / e), k = (int)(q % e);
                float gc = 0.f;
                if (i < h)
                    for (int o = 0; o < C; ++o) gc += dl[i * C + o] * A.wc[(int64_t)o * e + k];
                float gd = 0.f;
                for (int o = 0; o < DH; ++o) gd += dh1[i * DH + o] * A.w1[(int64_t)o * e + k];
                const float g = (gc + (-gd) * alpha) + A.gprox[q];
                A.dz[q] = A.z[q] > 0.f ? g : 0.f;
            }
        }
    }
}

__global__ void __launch_bounds__(TB) k_dm_prob(const float* __restrict__ z, int64_t n, int e,
                                                const float* __restrict__ wc, const float* __restrict__ bc, int C,
                                                float* __restrict__ prob) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const float* zi = z + i * e;
    float* pi = prob + i * C;
    float mx = -INFINITY;
    for (int o = 0; o < C; ++o) {
        float s = 0.f;
        for (int k = 0; k < e; ++k) s += fmaxf(zi[k], 0.f) * wc[(int64_t)o * e + k];
        s += bc[o];
        pi[o] = s;
        mx = fmaxf(mx, s);
    }
    float se = 0.f;
    for (int o = 0; o < C; ++o) se += expf(pi[o] - mx);
    for (int o = 0; o < C; ++o) pi[o] = expf(pi[o] - mx) / se;
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

extern "C" size_t gda_dmgnn_heads_workspace_bytes(int64_t h, int64_t e, int64_t c) {
    if (h < 1 || e < 1 || c < 1) return 256;
    return gda_align_up((size_t)heads_ws_floats(h, e, c) * sizeof(float), 8) + (size_t)3 * h * sizeof(double);
}

extern "C" int gda_dmgnn_heads_f32(const float* z, const float* gprox, const float* a_blocks, int64_t h, int64_t e,
                                   int64_t c, const float* const* w, const int64_t* y, int64_t ny, const int64_t* rows,
                                   const float* alpha, const double* prox, float pair_weight, float* dz,
                                   float* const* g, double* loss, double* loss_acc, void* workspace,
                                   size_t workspace_bytes, gda_stream_t stream) {
    if (h < 1 || h > GDA_ACDNE_MAX_HALF || e < 1 || e > 4096 || c < 1 || c > 4096 || ny < 1) return GDA_E_SIZE;
    if (!z || !gprox || !a_blocks || !w || !y || !rows || !alpha || !prox || !dz || !g || !loss || !workspace)
        return GDA_E_NULL;
    for (int k = 0; k < 8; ++k)
        if (!w[k] || !g[k]) return GDA_E_NULL;
    if (workspace_bytes < gda_dmgnn_heads_workspace_bytes(h, e, c)) return GDA_E_WORKSPACE;
    HeadArgs A;
    A.z = z;
    A.gprox = gprox;
    A.a_s = a_blocks;
    A.wc = w[0]; A.bc = w[1]; A.w1 = w[2]; A.b1 = w[3]; A.w2 = w[4]; A.b2 = w[5]; A.w3 = w[6]; A.b3 = w[7];
    A.y = y;
    A.rows = rows;
    A.ny = ny;
    A.alpha = alpha;
    A.prox = prox;
    A.pair_weight = pair_weight;
    A.h = (int)h;
    A.e = (int)e;
    A.c = (int)c;
    const int64_t m = 2 * h;
    const size_t fbytes = gda_align_up((size_t)heads_ws_floats(h, e, c) * sizeof(float), 8);
    A.ws = static_cast<float*>(workspace);
    A.terms = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + fbytes);
    A.dz = dz;
    A.gwc = g[0]; A.gbc = g[1]; A.gw1 = g[2]; A.gb1 = g[3]; A.gw2 = g[4]; A.gb2 = g[5]; A.gw3 = g[6]; A.gb3 = g[7];
    A.loss = loss;
    A.loss_acc = loss_acc;
    const int64_t work[6] = {m * e + m * DH + h * c, m * DH, m, m * DH + 2 * DH + 3 + h * c,
                             m * DH + DH * DH + DH + c * e + c, DH * e + DH + m * e};
    for (int phase = 0; phase < 6; ++phase) {
        const int64_t blocks = gda_cdiv(work[phase], TB);
        k_dm_heads<<<(unsigned)(blocks < HEAD_MAX_BLOCKS ? blocks : HEAD_MAX_BLOCKS), TB, 0, (hipStream_t)stream>>>(A, phase);
        GDA_LAUNCH_CHECK();
    }
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
    k_dm_prob<<<(unsigned)gda_cdiv(n, TB), TB, 0, s>>>(z, n, (int)e, wc, bc, (int)c, prob);
    GDA_LAUNCH_CHECK();
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
