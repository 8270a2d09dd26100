// SEPA (pygda/models/sepa.py): the prototype machinery of its loss as row kernels, ordered class-grouped reductions
// and one single-workgroup kernel for the C x C InfoNCE terms.  fp32, no atomics: every reduction over the rows is
// per-workgroup partials in LDS (each thread owns its columns, rows taken in order), written out and folded in block
// order, so two runs give the same bits.  See include/gda_hip.h for the contract of each entry point.
#include "gda_common.h"
#include "gda_reduce.h"

#include <math.h>

namespace {

constexpr int TB = 256;        // threads per workgroup (4 waves)
constexpr int ROWS = 64;       // rows per workgroup of the grouped reductions
constexpr int MAXC = GDA_SEPA_MAX_CLASSES;
constexpr float NEPS = 1e-12f; // F.normalize's clamp, and the reference's count / log offsets

template <int W> struct Vec { float v[W]; };

template <int W> __device__ __forceinline__ Vec<W> vload(const float* p) {
    Vec<W> r;
    if constexpr (W == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
        r.v[0] = p[0];
    }
    return r;
}

template <int W> __device__ __forceinline__ void vstore(float* p, const Vec<W>& r) {
    if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else p[0] = r.v[0];
}

// how TB threads share the column units of a [rows, d] matrix: `groups` row groups of `units` threads each
struct Split {
    int units, groups;
};
__host__ __device__ inline Split split_of(int d, int W) {
    Split s;
    s.units = d / W;
    s.groups = s.units >= TB ? 1 : TB / s.units;
    if (s.groups > ROWS) s.groups = ROWS;
    return s;
}
inline size_t part_lds_bytes(int C, int d, int W) { return (size_t)split_of(d, W).groups * C * d * sizeof(float); }

// ---- rows of the logits: P = softmax(Z), pred = argmax (lowest index on a tie), e = -sum P log(P + 1e-12) ----------
__global__ void __launch_bounds__(TB)
k_sepa_stats(const float* __restrict__ Z, int n, int C, float* __restrict__ P, int32_t* __restrict__ pred,
             float* __restrict__ ent) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const float* z = Z + (int64_t)i * C;
    float* p = P + (int64_t)i * C;
    float mx = z[0];
    for (int k = 1; k < C; ++k) mx = fmaxf(mx, z[k]);
    float sum = 0.f;
    for (int k = 0; k < C; ++k) sum += expf(z[k] - mx);
    float best = -1.f, e = 0.f;
    int arg = 0;
    for (int k = 0; k < C; ++k) {
        const float v = expf(z[k] - mx) / sum;
        p[k] = v;
        if (v > best) { best = v; arg = k; }
        e -= v * logf(v + NEPS);
    }
    pred[i] = arg;
    ent[i] = e;
}

// ---- class-grouped sums: part[blk][c][j] = sum over the block's rows with idx == c of w_i X[i][j]; cntp[blk][c] ------
template <int W>
__global__ void __launch_bounds__(TB)
k_sepa_group_sum(const float* __restrict__ X, int64_t ldx, const int32_t* __restrict__ idx,
                 const float* __restrict__ w, int n, int d, int C, float* __restrict__ part,
                 float* __restrict__ cntp) {
    extern __shared__ float lds[];
    __shared__ int sidx[ROWS];
    __shared__ float sw[ROWS];
    const Split sp = split_of(d, W);
    const int r0 = blockIdx.x * ROWS;
    const int rows = min(ROWS, n - r0);
    const int total = sp.groups * C * d;
    for (int q = threadIdx.x; q < total; q += TB) lds[q] = 0.f;
    if (threadIdx.x < rows) {
        const int c = idx[r0 + threadIdx.x];
        sidx[threadIdx.x] = (c >= 0 && c < C) ? c : -1;                   // a row outside [0, C) joins no class
        sw[threadIdx.x] = w != nullptr ? w[r0 + threadIdx.x] : 1.f;
    }
    __syncthreads();
    const int g = sp.units >= TB ? 0 : threadIdx.x / sp.units;
    if (g < sp.groups) {
        float* mine = lds + (size_t)g * C * d;
        const int u0 = sp.units >= TB ? threadIdx.x : threadIdx.x % sp.units;
        for (int r = g; r < rows; r += sp.groups) {                       // this group's rows, in order
            const int c = sidx[r];
            if (c < 0) continue;
            const float wr = sw[r];
            const float* x = X + (int64_t)(r0 + r) * ldx;
            for (int u = u0; u < sp.units; u += TB) {
                const Vec<W> v = vload<W>(x + u * W);
                float* dst = mine + c * d + u * W;
#pragma unroll
                for (int t = 0; t < W; ++t) dst[t] += wr * v.v[t];
            }
        }
    }
    __syncthreads();
    float* out = part + (size_t)blockIdx.x * C * d;
    for (int q = threadIdx.x; q < C * d; q += TB) {
        float a = 0.f;
        for (int gg = 0; gg < sp.groups; ++gg) a += lds[(size_t)gg * C * d + q];
        out[q] = a;
    }
    if (threadIdx.x < C) {
        int k = 0;
        for (int r = 0; r < rows; ++r) k += sidx[r] == (int)threadIdx.x;
        cntp[(size_t)blockIdx.x * C + threadIdx.x] = (float)k;
    }
}

// out[c][j] = fold over the blocks in order; mode 1 divides: (sum + cnt_c add[c][j]) / (cnt_c + eps)
__global__ void __launch_bounds__(TB)
k_sepa_fold(const float* __restrict__ part, const float* __restrict__ cntp, int nblk, int C, int d, int divide,
            float eps, const float* __restrict__ add, float* __restrict__ out, float* __restrict__ cnt,
            const float* __restrict__ cnt_in) {
    const int q = blockIdx.x * TB + threadIdx.x;
    if (q >= C * d) return;
    const int c = q / d;
    float a = 0.f;
    for (int b = 0; b < nblk; ++b) a += part[(size_t)b * C * d + q];
    float k = 0.f;
    if (cntp != nullptr) {
        for (int b = 0; b < nblk; ++b) k += cntp[(size_t)b * C + c];
        if (cnt != nullptr && q % d == 0) cnt[c] = k;
    } else if (cnt_in != nullptr) {
        k = cnt_in[c];
    }
    if (divide) {
        if (add != nullptr) a += k * add[q];
        a = a / (k + eps);
    }
    out[q] = a;
}

// dX[i] = g0 G[idx_i] / (cnt[idx_i] + eps): the gather backward of a class-grouped mean
template <int W>
__global__ void __launch_bounds__(TB)
k_sepa_class_mean_bwd(const float* __restrict__ G, const float* __restrict__ cnt, const int32_t* __restrict__ idx,
                      const float* __restrict__ g0, int n, int d, int C, float eps, float* __restrict__ dX) {
    const int units = d / W;
    const int64_t total = (int64_t)n * units;
    const float gs = g0 != nullptr ? g0[0] : 1.f;
    for (int64_t q = (int64_t)blockIdx.x * TB + threadIdx.x; q < total; q += (int64_t)gridDim.x * TB) {
        const int i = (int)(q / units), u = (int)(q % units);
        const int c = idx[i];
        Vec<W> r;
        if (c >= 0 && c < C) {
            const Vec<W> v = vload<W>(G + (int64_t)c * d + u * W);
            const float den = cnt[c] + eps;
#pragma unroll
            for (int t = 0; t < W; ++t) r.v[t] = gs * v.v[t] / den;
        } else {
#pragma unroll
            for (int t = 0; t < W; ++t) r.v[t] = 0.f;
        }
        vstore<W>(dX + (int64_t)i * d + u * W, r);
    }
}

// ---- the C x C stage between the row kernels (one workgroup) -------------------------------------------------------
// B = SF / (cnt + 1e-12); M = normalize(offdiag(SP_c / cnt_c)) (a zero row where cnt_c == 0);
// loss_im = sum_k m_k log(m_k + 1e-12) + mean(e), m = colsum(SP) / n
__global__ void __launch_bounds__(TB)
k_sepa_mid(const float* __restrict__ SP, const float* __restrict__ cnt, const float* __restrict__ SF,
           const float* __restrict__ ent, int n, int C, int h, float* __restrict__ B, float* __restrict__ M,
           float* __restrict__ loss_im) {
    __shared__ double red[TB];
    for (int q = threadIdx.x; q < C * h; q += TB) B[q] = SF[q] / (cnt[q / h] + NEPS);
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        const float k = cnt[c];
        float ss = 0.f;
        for (int j = 0; j < C; ++j) {
            const float v = (k > 0.f && j != c) ? SP[c * C + j] / k : 0.f;
            ss += v * v;
        }
        const float den = fmaxf(sqrtf(ss), NEPS);
        for (int j = 0; j < C; ++j) M[c * C + j] = ((k > 0.f && j != c) ? SP[c * C + j] / k : 0.f) / den;
    }
    const double esum = fold_d<TB>(ent, n, red);
    if (threadIdx.x == 0) {
        float div = 0.f;
        for (int j = 0; j < C; ++j) {
            float m = 0.f;
            for (int c = 0; c < C; ++c) m += SP[c * C + j];
            m = m / (float)n;
            div += m * logf(m + NEPS);
        }
        loss_im[0] = div + (float)(esum / (double)n);
    }
}

// the weights of one row against its class's row of M: W_k = P_k M[c][k] / max(||.||, 1e-12); s = sum_k (W_k + 1e-12)
__device__ __forceinline__ void row_weights(const float* __restrict__ p, const float* __restrict__ m, int C,
                                            float& rinv, float& s) {
    float ss = 0.f;
    for (int k = 0; k < C; ++k) { const float q = p[k] * m[k]; ss += q * q; }
    rinv = 1.f / fmaxf(sqrtf(ss), NEPS);
    s = 0.f;
    for (int k = 0; k < C; ++k) s += p[k] * m[k] * rinv + NEPS;
}

// U_i = (W_i B) / s_i - B[pred_i]; M and B in LDS, each row of U written once, W floats per lane
template <int W>
__global__ void __launch_bounds__(TB)
k_sepa_unbias_rows(const float* __restrict__ P, const int32_t* __restrict__ pred, const float* __restrict__ M,
                   const float* __restrict__ B, int n, int C, int h, int rows_per_block, float* __restrict__ U) {
    extern __shared__ float lds[];
    float* sB = lds;                 // [C][h]
    float* sM = lds + C * h;         // [C][C]
    for (int q = threadIdx.x; q < C * h; q += TB) sB[q] = B[q];
    for (int q = threadIdx.x; q < C * C; q += TB) sM[q] = M[q];
    __syncthreads();
    const Split sp = split_of(h, W);
    const int g = sp.units >= TB ? 0 : threadIdx.x / sp.units;
    if (g >= sp.groups) return;
    const int u0 = sp.units >= TB ? threadIdx.x : threadIdx.x % sp.units;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(n, r0 + rows_per_block);
    for (int i = r0 + g; i < r1; i += sp.groups) {
        const int c = pred[i];
        const float* p = P + (int64_t)i * C;
        const float* m = sM + c * C;
        float rinv, s;
        row_weights(p, m, C, rinv, s);
        for (int u = u0; u < sp.units; u += TB) {
            Vec<W> acc;
#pragma unroll
            for (int t = 0; t < W; ++t) acc.v[t] = 0.f;
            for (int k = 0; k < C; ++k) {
                const float wk = p[k] * m[k] * rinv;
#pragma unroll
                for (int t = 0; t < W; ++t) acc.v[t] += wk * sB[k * h + u * W + t];
            }
#pragma unroll
            for (int t = 0; t < W; ++t) acc.v[t] = acc.v[t] / s - sB[c * h + u * W + t];
            vstore<W>(U + (int64_t)i * h + u * W, acc);
        }
    }
}

// w_i = e_i / max(||R_i||, 1e-12): T_i = B[pred_i] + w_i R_i (one wave per row)
__global__ void __launch_bounds__(TB)
k_sepa_row_weight(const float* __restrict__ R, const float* __restrict__ ent, int n, int h, float* __restrict__ w) {
    const int row = blockIdx.x * (TB / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (row >= n) return;
    const float* r = R + (int64_t)row * h;
    float ss = 0.f;
    for (int j = lane; j < h; j += 64) ss += r[j] * r[j];
    ss = wave_sum(ss);
    if (lane == 0) w[row] = ent[row] / fmaxf(sqrtf(ss), NEPS);
}

// dR_i = g0 e_i (g - y <g, y>) / d (the clamp's branch: g / d where ||R_i|| < 1e-12), de_i = g0 <g, y>,
// g = dcenter[pred_i] / (cnt + 1e-12), y = R_i / d, d = max(||R_i||, 1e-12)
__global__ void __launch_bounds__(TB)
k_sepa_center_rows_bwd(const float* __restrict__ R, const float* __restrict__ ent, const int32_t* __restrict__ pred,
                       const float* __restrict__ dcenter, const float* __restrict__ cnt, const float* __restrict__ g0,
                       int n, int h, float* __restrict__ dR, float* __restrict__ de) {
    const int row = blockIdx.x * (TB / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (row >= n) return;
    const int c = pred[row];
    const float scale = (g0 != nullptr ? g0[0] : 1.f) / (cnt[c] + NEPS);
    const float* r = R + (int64_t)row * h;
    const float* gc = dcenter + (int64_t)c * h;
    float ss = 0.f, gr = 0.f;
    for (int j = lane; j < h; j += 64) {
        ss += r[j] * r[j];
        gr += gc[j] * scale * r[j];
    }
    ss = wave_sum(ss);
    gr = wave_sum(gr);
    const float nrm = sqrtf(ss);
    const float d = fmaxf(nrm, NEPS);
    const float gy = gr / d;                                    // <g, y>
    const float e = ent[row];
    const float proj = nrm >= NEPS ? gy : 0.f;
    float* out = dR + (int64_t)row * h;
    for (int j = lane; j < h; j += 64) out[j] = e * (gc[j] * scale - (r[j] / d) * proj) / d;
    if (lane == 0) de[row] = gy;
}

// ---- the backward of k_sepa_unbias_rows ---------------------------------------------------------------------------
// per row: t_k = <dU_i, B_k>; dW_k = t_k / s - <dU_i, V_i> / s^2 with <dU_i, V_i> = sum_k W_k t_k; the normalisation's
// backward gives dQ; dPu[i][k] = dQ_k M[c][k]; X[i][k] = dQ_k P[i][k] (its class-grouped sum is dM).
// per workgroup: part[k][j] = sum_i (W_ik / s_i) dU[i][j] - [k == pred_i] dU[i][j]  (dB's partial)
template <int W>
__global__ void __launch_bounds__(TB)
k_sepa_unbias_rows_bwd(const float* __restrict__ dU, const float* __restrict__ P, const int32_t* __restrict__ pred,
                       const float* __restrict__ M, const float* __restrict__ B, int n, int C, int h,
                       float* __restrict__ dPu, float* __restrict__ X, float* __restrict__ part) {
    extern __shared__ float lds[];
    __shared__ float sa[ROWS][MAXC];          // W_ik / s_i of the block's rows
    __shared__ float st[TB / 64][MAXC];       // t_k of the row a wave is on
    __shared__ int sidx[ROWS];
    const Split sp = split_of(h, W);
    const int r0 = blockIdx.x * ROWS;
    const int rows = min(ROWS, n - r0);
    const int total = sp.groups * C * h;
    for (int q = threadIdx.x; q < total; q += TB) lds[q] = 0.f;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int r = wave; r < rows; r += TB / 64) {
        const int i = r0 + r;
        const int c = pred[i];
        const float* g = dU + (int64_t)i * h;
        for (int k = 0; k < C; ++k) {
            const float* b = B + (int64_t)k * h;
            float a = 0.f;
            for (int j = lane; j < h; j += 64) a += g[j] * b[j];
            a = wave_sum(a);
            if (lane == 0) st[wave][k] = a;
        }
        if (lane == 0) {                                        // lane 0 wrote st[wave][.] itself
            const float* p = P + (int64_t)i * C;
            const float* m = M + c * C;
            float ss = 0.f;
            for (int k = 0; k < C; ++k) { const float q = p[k] * m[k]; ss += q * q; }
            const float nrm = sqrtf(ss);
            const float d = fmaxf(nrm, NEPS);
            float s = 0.f, uv = 0.f;
            for (int k = 0; k < C; ++k) {
                const float wk = p[k] * m[k] / d;
                s += wk + NEPS;
                uv += wk * st[wave][k];
            }
            const float ds = -uv / (s * s);
            float dot = 0.f;                                    // <dW, W>
            for (int k = 0; k < C; ++k) dot += (st[wave][k] / s + ds) * (p[k] * m[k] / d);
            if (nrm < NEPS) dot = 0.f;
            for (int k = 0; k < C; ++k) {
                const float wk = p[k] * m[k] / d;
                const float dq = ((st[wave][k] / s + ds) - wk * dot) / d;
                dPu[(int64_t)i * C + k] = dq * m[k];
                X[(int64_t)i * C + k] = dq * p[k];
                sa[r][k] = wk / s;
            }
            sidx[r] = c;
        }
    }
    __syncthreads();
    const int g = sp.units >= TB ? 0 : threadIdx.x / sp.units;
    if (g < sp.groups) {
        float* mine = lds + (size_t)g * C * h;
        const int u0 = sp.units >= TB ? threadIdx.x : threadIdx.x % sp.units;
        for (int r = g; r < rows; r += sp.groups) {
            const int c = sidx[r];
            const float* x = dU + (int64_t)(r0 + r) * h;
            for (int u = u0; u < sp.units; u += TB) {
                const Vec<W> v = vload<W>(x + u * W);
                for (int k = 0; k < C; ++k) {
                    const float a = sa[r][k] - (k == c ? 1.f : 0.f);
                    float* dst = mine + k * h + u * W;
#pragma unroll
                    for (int t = 0; t < W; ++t) dst[t] += a * v.v[t];
                }
            }
        }
    }
    __syncthreads();
    float* out = part + (size_t)blockIdx.x * C * h;
    for (int q = threadIdx.x; q < C * h; q += TB) {
        float a = 0.f;
        for (int gg = 0; gg < sp.groups; ++gg) a += lds[(size_t)gg * C * h + q];
        out[q] = a;
    }
}

// the backward of k_sepa_mid (one workgroup):
//   dBt = dBf + g0 cnt dcenter / (cnt + 1e-12)        (the gather table of dF: dF_i = dBt[pred_i] / (cnt + 1e-12))
//   GP[c][k] = d loss / d SP[c][k] through M          (added to dP_i by pred_i)
//   gim[k] = g0 lam_im (log(m_k + 1e-12) + m_k / (m_k + 1e-12)) / n,  gim[C] = g0 lam_im / n   (the entropy's mean)
__global__ void __launch_bounds__(TB)
k_sepa_mid_bwd(const float* __restrict__ dMn, const float* __restrict__ SP, const float* __restrict__ cnt,
               const float* __restrict__ dBf, const float* __restrict__ dcenter, const float* __restrict__ g0,
               float lam_im, int n, int C, int h, float* __restrict__ dBt, float* __restrict__ GP,
               float* __restrict__ gim) {
    const float gs = g0 != nullptr ? g0[0] : 1.f;
    for (int q = threadIdx.x; q < C * h; q += TB) {
        const float k = cnt[q / h];
        dBt[q] = dBf[q] + gs * k * dcenter[q] / (k + NEPS);
    }
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        const float k = cnt[c];
        float ss = 0.f, dot = 0.f;
        for (int j = 0; j < C; ++j) {
            const float v = (k > 0.f && j != c) ? SP[c * C + j] / k : 0.f;
            ss += v * v;
        }
        const float nrm = sqrtf(ss);
        const float d = fmaxf(nrm, NEPS);
        for (int j = 0; j < C; ++j) {
            const float v = (k > 0.f && j != c) ? SP[c * C + j] / k : 0.f;
            dot += dMn[c * C + j] * (v / d);
        }
        if (nrm < NEPS) dot = 0.f;
        for (int j = 0; j < C; ++j) {
            const float v = (k > 0.f && j != c) ? SP[c * C + j] / k : 0.f;
            const float dv = (dMn[c * C + j] - (v / d) * dot) / d;
            GP[c * C + j] = (k > 0.f && j != c) ? dv / k : 0.f;
        }
        float m = 0.f;
        for (int cc = 0; cc < C; ++cc) m += SP[cc * C + c];
        m = m / (float)n;
        gim[c] = gs * lam_im * (logf(m + NEPS) + m / (m + NEPS)) / (float)n;
    }
    if (threadIdx.x == 0) gim[C] = gs * lam_im / (float)n;
}

// dZ_i = P_i (dP_i - <dP_i, P_i>), dP_ik = dPu_ik + GP[pred_i][k] + gim[k] - de_i (log(P_ik + eps) + P_ik / (P_ik + eps)),
// de_i = de[i] + gim[C]
__global__ void __launch_bounds__(TB)
k_sepa_dz_rows(const float* __restrict__ P, const int32_t* __restrict__ pred, const float* __restrict__ dPu,
               const float* __restrict__ GP, const float* __restrict__ gim, const float* __restrict__ de, int n, int C,
               float* __restrict__ dZ) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const float* p = P + (int64_t)i * C;
    const float* gp = GP + pred[i] * C;
    const float* du = dPu + (int64_t)i * C;
    const float dei = de[i] + gim[C];
    float dot = 0.f;
    for (int k = 0; k < C; ++k) {
        const float v = p[k];
        const float g = du[k] + gp[k] + gim[k] - dei * (logf(v + NEPS) + v / (v + NEPS));
        dot += g * v;
    }
    float* out = dZ + (int64_t)i * C;
    for (int k = 0; k < C; ++k) {
        const float v = p[k];
        const float g = du[k] + gp[k] + gim[k] - dei * (logf(v + NEPS) + v / (v + NEPS));
        out[k] = v * (g - dot);
    }
}

// ---- prototypes: loss_pp (proto_alignment), loss_sep (seperate_center) and both gradients, one workgroup ----------
// T, S [C, h] are read from memory (they are small and cached); the C x C similarity and gradient matrices live in LDS.
__global__ void __launch_bounds__(TB)
k_sepa_proto(const float* __restrict__ T, const float* __restrict__ S, int C, int h, float tau, float wpp, float wsep,
             float* __restrict__ losses, float* __restrict__ dT, float* __restrict__ dS) {
    __shared__ float sim[4][MAXC][MAXC];      // ts, tt, ss (prototypes + 1e-6, normalised), pp (S normalised): exp(cos / tau)
    __shared__ float gsim[4][MAXC][MAXC];     // d loss / d cos
    __shared__ float nrm[3][MAXC];            // ||T + 1e-6||, ||S + 1e-6||, ||S||
    const float off = 1e-6f;
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    for (int a = wave; a < C; a += TB / 64) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int j = lane; j < h; j += 64) {
            const float t = T[a * h + j] + off, s = S[a * h + j] + off, p = S[a * h + j];
            s0 += t * t; s1 += s * s; s2 += p * p;
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { nrm[0][a] = sqrtf(s0); nrm[1][a] = sqrtf(s1); nrm[2][a] = sqrtf(s2); }
    }
    __syncthreads();
    for (int q = wave; q < C * C; q += TB / 64) {
        const int a = q / C, b = q % C;
        float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
        for (int j = lane; j < h; j += 64) {
            const float ta = T[a * h + j] + off, tb = T[b * h + j] + off;
            const float sa = S[a * h + j], sb = S[b * h + j];
            d0 += ta * (sb + off); d1 += ta * tb; d2 += (sa + off) * (sb + off); d3 += sa * sb;
        }
        d0 = wave_sum(d0); d1 = wave_sum(d1); d2 = wave_sum(d2); d3 = wave_sum(d3);
        if (lane == 0) {
            const float ta = fmaxf(nrm[0][a], NEPS), tb = fmaxf(nrm[0][b], NEPS);
            const float sa = fmaxf(nrm[1][a], NEPS), sb = fmaxf(nrm[1][b], NEPS);
            const float pa = fmaxf(nrm[2][a], NEPS), pb = fmaxf(nrm[2][b], NEPS);
            sim[0][a][b] = expf(d0 / (ta * sb) / tau);
            sim[1][a][b] = expf(d1 / (ta * tb) / tau);
            sim[2][a][b] = expf(d2 / (sa * sb) / tau);
            sim[3][a][b] = expf(d3 / (pa * pb) / tau);
        }
    }
    __syncthreads();
    __shared__ float lrow[2][MAXC];
    if (threadIdx.x < C) {
        const int a = threadIdx.x;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int b = 0; b < C; ++b) { s0 += sim[0][a][b]; s1 += sim[1][a][b]; s2 += sim[2][a][b]; s3 += sim[3][a][b]; }
        const float pos = sim[0][a][a];
        const float den = s0 - pos + s1 - sim[1][a][a] + s2 - sim[2][a][a];
        const float denc = fmaxf(den, 1e-6f);
        const float logit = pos / denc;
        const float lc = fmaxf(logit, 1e-6f);
        lrow[0][a] = -logf(lc);
        const float glogit = logit >= 1e-6f ? -wpp / ((float)C * lc) : 0.f;
        const float gpos = glogit / denc;
        const float gden = den >= 1e-6f ? -glogit * pos / (denc * denc) : 0.f;
        const float l = (s3 - sim[3][a][a]) / (float)(C - 1);
        lrow[1][a] = logf(l + 1e-8f);
        const float gl = wsep / ((float)C * (l + 1e-8f)) / (float)(C - 1);
        for (int b = 0; b < C; ++b) {
            const bool diag = b == a;
            gsim[0][a][b] = (diag ? gpos : gden) * sim[0][a][b] / tau;
            gsim[1][a][b] = (diag ? 0.f : gden) * sim[1][a][b] / tau;
            gsim[2][a][b] = (diag ? 0.f : gden) * sim[2][a][b] / tau;
            gsim[3][a][b] = (diag ? 0.f : gl) * sim[3][a][b] / tau;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float a0 = 0.f, a1 = 0.f;
        for (int a = 0; a < C; ++a) { a0 += lrow[0][a]; a1 += lrow[1][a]; }
        losses[0] = a0 / (float)C;
        losses[1] = a1 / (float)C;
    }
    if (dT == nullptr && dS == nullptr) return;
    // the gradient of a normalised row y = x / d from the gradient gy of y: (gy - y <gy, y>) / d (gy / d under the clamp)
    for (int a = wave; a < C; a += TB / 64) {
        const float dt = fmaxf(nrm[0][a], NEPS), ds = fmaxf(nrm[1][a], NEPS), dp = fmaxf(nrm[2][a], NEPS);
        float dot_t = 0.f, dot_s = 0.f, dot_p = 0.f;
        for (int j = lane; j < h; j += 64) {
            float gt = 0.f, gs = 0.f, gp = 0.f;
            for (int b = 0; b < C; ++b) {
                const float tb = (T[b * h + j] + off) / fmaxf(nrm[0][b], NEPS);
                const float sb = (S[b * h + j] + off) / fmaxf(nrm[1][b], NEPS);
                const float pb = S[b * h + j] / fmaxf(nrm[2][b], NEPS);
                gt += gsim[0][a][b] * sb + (gsim[1][a][b] + gsim[1][b][a]) * tb;
                gs += gsim[0][b][a] * tb + (gsim[2][a][b] + gsim[2][b][a]) * sb;
                gp += (gsim[3][a][b] + gsim[3][b][a]) * pb;
            }
            dT[a * h + j] = gt;
            dS[a * h + j] = gs;
            dot_t += gt * ((T[a * h + j] + off) / dt);
            dot_s += gs * ((S[a * h + j] + off) / ds);
            dot_p += gp * (S[a * h + j] / dp);
        }
        dot_t = wave_sum(dot_t); dot_s = wave_sum(dot_s); dot_p = wave_sum(dot_p);
        if (nrm[0][a] < NEPS) dot_t = 0.f;
        if (nrm[1][a] < NEPS) dot_s = 0.f;
        if (nrm[2][a] < NEPS) dot_p = 0.f;
        for (int j = lane; j < h; j += 64) {
            float gp = 0.f;
            for (int b = 0; b < C; ++b)
                gp += (gsim[3][a][b] + gsim[3][b][a]) * (S[b * h + j] / fmaxf(nrm[2][b], NEPS));
            const float gt = dT[a * h + j], gs = dS[a * h + j];               // this lane's own stores
            dT[a * h + j] = (gt - ((T[a * h + j] + off) / dt) * dot_t) / dt;
            dS[a * h + j] = (gs - ((S[a * h + j] + off) / ds) * dot_s) / ds + (gp - (S[a * h + j] / dp) * dot_p) / dp;
        }
    }
}

bool vec_ok(const void* p, int64_t ld, int64_t d) { return d % 4 == 0 && ld % 4 == 0 && ((uintptr_t)p % 16) == 0; }

int64_t nblocks(int64_t n) { return gda_cdiv(n, ROWS); }

bool dims_bad(int64_t n, int64_t C, int64_t d) { return n < 1 || n >= (1 << 24) || C < 1 || d < 1; }

}  // namespace

extern "C" size_t gda_sepa_workspace_bytes(int64_t n, int64_t C, int64_t d) {
    if (n < 1 || C < 1 || d < 1) return 256;
    return gda_align_up((size_t)nblocks(n) * C * (d + 1) * sizeof(float), 256);
}

extern "C" int gda_sepa_stats_f32(const float* Z, int64_t n, int64_t C, float* P, int32_t* pred, float* ent,
                                  gda_stream_t stream) {
    if (dims_bad(n, C, 1)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES) return GDA_E_UNSUPPORTED;
    if (!Z || !P || !pred || !ent) return GDA_E_NULL;
    k_sepa_stats<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(Z, (int)n, (int)C, P, pred, ent);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_group_sum_f32(const float* X, int64_t ldx, const int32_t* idx, const float* w, int64_t n,
                                      int64_t d, int64_t C, int divide, float eps, const float* add, float* out,
                                      float* cnt, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (dims_bad(n, C, d) || ldx < d) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || d > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!X || !idx || !out || !cnt || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_sepa_workspace_bytes(n, C, d)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = nblocks(n);
    float* part = static_cast<float*>(workspace);
    float* cntp = part + nb * C * d;
    if (vec_ok(X, ldx, d)) {
        const size_t lds = part_lds_bytes((int)C, (int)d, 4);
        GDA_LDS_ATTR_ONCE(k_sepa_group_sum<4>, 160 * 1024 - 1024);
        k_sepa_group_sum<4><<<(unsigned)nb, TB, lds, s>>>(X, ldx, idx, w, (int)n, (int)d, (int)C, part, cntp);
    } else {
        const size_t lds = part_lds_bytes((int)C, (int)d, 1);
        GDA_LDS_ATTR_ONCE(k_sepa_group_sum<1>, 160 * 1024 - 1024);
        k_sepa_group_sum<1><<<(unsigned)nb, TB, lds, s>>>(X, ldx, idx, w, (int)n, (int)d, (int)C, part, cntp);
    }
    GDA_LAUNCH_CHECK();
    k_sepa_fold<<<(unsigned)gda_cdiv(C * d, TB), TB, 0, s>>>(part, cntp, (int)nb, (int)C, (int)d, divide, eps, add, out,
                                                              cnt, nullptr);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_class_mean_bwd_f32(const float* G, const float* cnt, const int32_t* idx, const float* g0,
                                           int64_t n, int64_t d, int64_t C, float eps, float* dX,
                                           gda_stream_t stream) {
    if (dims_bad(n, C, d)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || d > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!G || !cnt || !idx || !dX) return GDA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    if (vec_ok(G, d, d) && vec_ok(dX, d, d)) {
        const int64_t blocks = gda_cdiv(n * (d / 4), TB);
        k_sepa_class_mean_bwd<4><<<(unsigned)(blocks < 4096 ? blocks : 4096), TB, 0, s>>>(G, cnt, idx, g0, (int)n,
                                                                                         (int)d, (int)C, eps, dX);
    } else {
        const int64_t blocks = gda_cdiv(n * d, TB);
        k_sepa_class_mean_bwd<1><<<(unsigned)(blocks < 4096 ? blocks : 4096), TB, 0, s>>>(G, cnt, idx, g0, (int)n,
                                                                                         (int)d, (int)C, eps, dX);
    }
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_mid_f32(const float* SP, const float* cnt, const float* SF, const float* ent, int64_t n,
                                int64_t C, int64_t h, float* B, float* M, float* loss_im, gda_stream_t stream) {
    if (dims_bad(n, C, h)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!SP || !cnt || !SF || !ent || !B || !M || !loss_im) return GDA_E_NULL;
    k_sepa_mid<<<1, TB, 0, (hipStream_t)stream>>>(SP, cnt, SF, ent, (int)n, (int)C, (int)h, B, M, loss_im);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_unbias_rows_f32(const float* P, const int32_t* pred, const float* M, const float* B, int64_t n,
                                        int64_t C, int64_t h, float* U, gda_stream_t stream) {
    if (dims_bad(n, C, h)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!P || !pred || !M || !B || !U) return GDA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = (size_t)(C * h + C * C) * sizeof(float);
    // enough rows per workgroup to pay for staging B, enough workgroups to fill the chip
    int64_t rpb = gda_cdiv(n, 512);
    if (rpb < 16) rpb = 16;
    const unsigned grid = (unsigned)gda_cdiv(n, rpb);
    if (vec_ok(U, h, h)) {
        GDA_LDS_ATTR_ONCE(k_sepa_unbias_rows<4>, 160 * 1024 - 1024);
        k_sepa_unbias_rows<4><<<grid, TB, lds, s>>>(P, pred, M, B, (int)n, (int)C, (int)h, (int)rpb, U);
    } else {
        GDA_LDS_ATTR_ONCE(k_sepa_unbias_rows<1>, 160 * 1024 - 1024);
        k_sepa_unbias_rows<1><<<grid, TB, lds, s>>>(P, pred, M, B, (int)n, (int)C, (int)h, (int)rpb, U);
    }
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_row_weight_f32(const float* R, const float* ent, int64_t n, int64_t h, float* w,
                                       gda_stream_t stream) {
    if (dims_bad(n, 1, h)) return GDA_E_SIZE;
    if (h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!R || !ent || !w) return GDA_E_NULL;
    k_sepa_row_weight<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, (hipStream_t)stream>>>(R, ent, (int)n, (int)h, w);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_center_rows_bwd_f32(const float* R, const float* ent, const int32_t* pred,
                                            const float* dcenter, const float* cnt, const float* g0, int64_t n,
                                            int64_t C, int64_t h, float* dR, float* de, gda_stream_t stream) {
    if (dims_bad(n, C, h)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!R || !ent || !pred || !dcenter || !cnt || !dR || !de) return GDA_E_NULL;
    if (dR == R) return GDA_E_ALIAS;
    k_sepa_center_rows_bwd<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, (hipStream_t)stream>>>(R, ent, pred, dcenter, cnt,
                                                                                           g0, (int)n, (int)h, dR, de);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_unbias_rows_bwd_f32(const float* dU, const float* P, const int32_t* pred, const float* M,
                                            const float* B, int64_t n, int64_t C, int64_t h, float* dPu, float* X,
                                            float* dB, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (dims_bad(n, C, h)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!dU || !P || !pred || !M || !B || !dPu || !X || !dB || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_sepa_workspace_bytes(n, C, h)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = nblocks(n);
    float* part = static_cast<float*>(workspace);
    if (vec_ok(dU, h, h)) {
        GDA_LDS_ATTR_ONCE(k_sepa_unbias_rows_bwd<4>, 160 * 1024 - 16 * 1024);
        k_sepa_unbias_rows_bwd<4><<<(unsigned)nb, TB, part_lds_bytes((int)C, (int)h, 4), s>>>(
            dU, P, pred, M, B, (int)n, (int)C, (int)h, dPu, X, part);
    } else {
        GDA_LDS_ATTR_ONCE(k_sepa_unbias_rows_bwd<1>, 160 * 1024 - 16 * 1024);
        k_sepa_unbias_rows_bwd<1><<<(unsigned)nb, TB, part_lds_bytes((int)C, (int)h, 1), s>>>(
            dU, P, pred, M, B, (int)n, (int)C, (int)h, dPu, X, part);
    }
    GDA_LAUNCH_CHECK();
    k_sepa_fold<<<(unsigned)gda_cdiv(C * h, TB), TB, 0, s>>>(part, nullptr, (int)nb, (int)C, (int)h, 0, 0.f, nullptr, dB,
                                                              nullptr, nullptr);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_mid_bwd_f32(const float* dMn, const float* SP, const float* cnt, const float* dBf,
                                    const float* dcenter, const float* g0, float lam_im, int64_t n, int64_t C,
                                    int64_t h, float* dBt, float* GP, float* gim, gda_stream_t stream) {
    if (dims_bad(n, C, h)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!dMn || !SP || !cnt || !dBf || !dcenter || !dBt || !GP || !gim) return GDA_E_NULL;
    k_sepa_mid_bwd<<<1, TB, 0, (hipStream_t)stream>>>(dMn, SP, cnt, dBf, dcenter, g0, lam_im, (int)n, (int)C, (int)h,
                                                      dBt, GP, gim);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_dz_rows_f32(const float* P, const int32_t* pred, const float* dPu, const float* GP,
                                    const float* gim, const float* de, int64_t n, int64_t C, float* dZ,
                                    gda_stream_t stream) {
    if (dims_bad(n, C, 1)) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES) return GDA_E_UNSUPPORTED;
    if (!P || !pred || !dPu || !GP || !gim || !de || !dZ) return GDA_E_NULL;
    k_sepa_dz_rows<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(P, pred, dPu, GP, gim, de, (int)n, (int)C,
                                                                             dZ);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_sepa_proto_f32(const float* T, const float* S, int64_t C, int64_t h, float tau, float wpp,
                                  float wsep, float* losses, float* dT, float* dS, gda_stream_t stream) {
    if (C < 1 || h < 1) return GDA_E_SIZE;
    if (C > GDA_SEPA_MAX_CLASSES || h > GDA_SEPA_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!T || !S || !losses || (dT == nullptr) != (dS == nullptr)) return GDA_E_NULL;
    if (!(tau > 0.f)) return GDA_E_SIZE;
    if (dT != nullptr && (dT == T || dS == S || dT == dS)) return GDA_E_ALIAS;
    k_sepa_proto<<<1, TB, 0, (hipStream_t)stream>>>(T, S, (int)C, (int)h, tau, wpp, wsep, losses, dT, dS);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
