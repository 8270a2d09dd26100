// GraphCTA (pygda/models/graphcta.py): the model loss (instance_proto_alignment with the weighted cross-entropy), the
// per-row top-(K+1) by inner product and the rest of test_time_loss, none of which stores an [N, N] array.
// fp32, no atomics, gfx950.  The all-pairs products are 64x64 tiles on v_mfma_f32_32x32x2_f32 (four waves, a 32x32
// quarter each), staged through LDS in chunks of DK features as in gda_mmd.hip's k_pairdist.  A workgroup owns 64 rows
// and one contiguous share of the column tiles ("split"); what the splits leave -- row sums, [N, d] gradient partials,
// candidate lists -- is folded in split order by the row kernel that follows, so two runs give the same bits.
// See include/gda_hip.h for the contract of each entry point.
#include "gda_common.h"
#include "gda_pair_tile.h"
#include "gda_reduce.h"

#include <math.h>

namespace {

using namespace gda_pair_tile;              // TB, TILE, DK, LDT, TileLds, load4, tile_product
constexpr int ROWS = TB / GDA_WAVE;           // a wavefront per row in the row kernels
constexpr int MAXC = GDA_CTA_MAX_CLASSES;
constexpr int MAXK1 = GDA_CTA_MAX_K1;
constexpr int MAXS = 8;                       // column splits
constexpr int STB = 1024;                     // the one-workgroup statistics kernel
constexpr float NORM_EPS = 1e-12f;            // F.normalize's eps
const int64_t LIM = (int64_t)1 << 31;

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

__device__ __forceinline__ bool in_range(int idx, int64_t n) { return (unsigned)idx < (unsigned)n; }

// a row's class as a wave-uniform value (every lane read the same word), 0 when it is out of range
__device__ __forceinline__ int uniform_class(int c, int C) { return __builtin_amdgcn_readfirstlane(in_range(c, C) ? c : 0); }

// how the column tiles are shared out: tiles per split and the number of splits that leaves none empty
struct Split { int tps, s; };
Split make_split(int64_t rows, int64_t cols) {
    const int64_t rt = gda_cdiv(rows, TILE), ct = gda_cdiv(cols, TILE);
    int64_t s = gda_cdiv(256, rt);                         // 256 CUs
    s = s < 1 ? 1 : s > MAXS ? MAXS : s;
    s = s > ct ? ct : s;
    const int64_t tps = gda_cdiv(ct, s);
    return {(int)tps, (int)gda_cdiv(ct, tps)};
}

// ---- x / max(|x|, 1e-12) per row, a wavefront per row; nrm keeps |x| -------------------------------------------------
__global__ void __launch_bounds__(TB)
k_cta_normalize(const float* __restrict__ X, int64_t n, int d, float* __restrict__ Xh, float* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* x = X + i * d;
    float a = 0.f;
    for (int k = lane; k < d; k += GDA_WAVE) a = fmaf(x[k], x[k], a);
    a = sqrtf(wave_sum(a));
    const float den = fmaxf(a, NORM_EPS);
    for (int k = lane; k < d; k += GDA_WAVE) Xh[i * d + k] = x[k] / den;
    if (lane == 0) nrm[i] = a;
}

// ---- the all-pairs pass over F^ F^^T.  Forward: R_i = sum_{j != i} exp(f^_i . f^_j / tau) over the split's columns.
//      Backward: the tile's E'_ij = e_ij (c_i + c_j) goes to LDS and E' F^_j is accumulated on the matrix cores: wave w
//      owns rows 32 (w & 1).. and the 32-wide feature blocks (w >> 1), (w >> 1) + 2, .. -----------------------------------
template <bool BWD>
__global__ void __launch_bounds__(TB)
k_cta_pairs(const float* __restrict__ Fh, int64_t n, int d, float inv_tau, int tps, const float* __restrict__ cvec,
            float* __restrict__ Rpart, float* __restrict__ Gpart, bool vec) {
    __shared__ TileLds L;
    __shared__ float Es[TILE][LDT];
    __shared__ float ci[TILE], cj[TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, la = lane & 31, ka = lane >> 5;
    const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
    const int64_t i0 = (int64_t)blockIdx.x * TILE;
    const int64_t ntiles = (n + TILE - 1) / TILE;
    const int64_t jt0 = (int64_t)blockIdx.y * tps, jt1 = jt0 + tps < ntiles ? jt0 + tps : ntiles;
    float rs[16];
    f32x16 og[4];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rs[r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) og[q][r] = 0.f;
    }
    if (BWD && tid < TILE) ci[tid] = i0 + tid < n ? cvec[i0 + tid] : 0.f;
    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = jt * TILE;
        const f32x16 acc = tile_product(Fh, n, i0, Fh, n, j0, d, vec, L);
        if (BWD) {
            __syncthreads();                               // the tile before: its second product has read Es
            if (tid < TILE) cj[tid] = j0 + tid < n ? cvec[j0 + tid] : 0.f;
            __syncthreads();
        }
        const int lj = wj + la;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int li = wi + (r & 3) + 8 * (r >> 2) + 4 * ka;
            const int64_t i = i0 + li, j = j0 + lj;
            const float e = (i < n && j < n && i != j) ? expf(acc[r] * inv_tau) : 0.f;
            if (BWD) Es[lj][li] = e * (ci[li] + cj[lj]);
            else rs[r] += e;
        }
        if (BWD) {
            __syncthreads();
            const int fb0 = wave >> 1;
            for (int k = 0; k < TILE; k += 2) {
                const float a = Es[k + ka][wi + la];
                const int64_t jj = j0 + k + ka;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = (fb0 + 2 * q) * 32 + la;
                    if ((fb0 + 2 * q) * 32 < d) {              // wave-uniform
                        const float b = (jj < n && col < d) ? Fh[jj * d + col] : 0.f;
                        og[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, og[q], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (BWD) {
        const int fb0 = wave >> 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = (fb0 + 2 * q) * 32 + la;
            if (col >= d) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t i = i0 + wi + (r & 3) + 8 * (r >> 2) + 4 * ka;
                if (i < n) Gpart[((int64_t)blockIdx.y * n + i) * d + col] = og[q][r];
            }
        }
    } else {
        __syncthreads();                                   // Es is free: no second product in the forward pass
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = rs[r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);      // over the 32 columns of the quarter
            if (la == 0) Es[wave >> 1][wi + (r & 3) + 8 * (r >> 2) + 4 * ka] = v;
        }
        __syncthreads();
        if (tid < TILE && i0 + tid < n) Rpart[(int64_t)blockIdx.y * n + i0 + tid] = Es[0][tid] + Es[1][tid];
    }
}

// ---- what a row knows about the prototypes: lane c holds class c ------------------------------------------------------
struct ProtoRow { float sim, ex, S, pos, w, D, q; };

__device__ __forceinline__ ProtoRow proto_row(const float* __restrict__ fh, const float* __restrict__ Ch, int lane, int C,
                                              int d, int pred, float inv_tau, float R) {
    ProtoRow p;
    float a = 0.f;
    if (lane < C)
        for (int k = 0; k < d; ++k) a = fmaf(fh[k], Ch[(int64_t)lane * d + k], a);
    p.sim = a;
    p.ex = lane < C ? expf(a * inv_tau) : 0.f;
    p.S = wave_sum(p.ex);
    p.w = bcast(p.sim, pred);
    p.pos = bcast(p.ex, pred);
    p.D = p.S - p.pos + R + 1e-8f;
    p.q = p.pos / p.D;
    return p;
}

__device__ __forceinline__ float fold_splits(const float* __restrict__ part, int64_t stride, int64_t at, int s) {
    float a = 0.f;
    for (int q = 0; q < s; ++q) a += part[(int64_t)q * stride + at];
    return a;
}

// ---- model loss, middle: per row w_i, ce_i, cl_i and lamb * dcl/dD_i ---------------------------------------------------
__global__ void __launch_bounds__(TB)
k_cta_rows_mid(const float* __restrict__ Fh, const float* __restrict__ Ch, const float* __restrict__ logits,
               const int32_t* __restrict__ predv, const float* __restrict__ Rpart, int s, int64_t n, int d, int C,
               float inv_tau, float lamb, float* __restrict__ rw, float* __restrict__ rce, float* __restrict__ rcl,
               float* __restrict__ cvec) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (i >= n) return;
    const int pred = uniform_class(predv[i], C);
    const float R = fold_splits(Rpart, n, i, s);
    const ProtoRow p = proto_row(Fh + i * d, Ch, lane, C, d, pred, inv_tau, R);
    const float lg = lane < C ? logits[i * C + lane] : -INFINITY;
    const float mx = wave_max(lg);
    const float se = wave_sum(lane < C ? expf(lg - mx) : 0.f);
    const float ce = (mx + logf(se)) - bcast(lg, pred);
    if (lane == 0) {
        rw[i] = p.w;
        rce[i] = ce;
        rcl[i] = -logf(p.q + 1e-8f);
        cvec[i] = lamb * ((p.pos / (p.D * p.D)) / (p.q + 1e-8f)) / (float)n;
    }
}

// ---- model loss, the three sums: out = {(1 - lamb) local + lamb cl, local, cl}, scal[0] = W --------------------------
__global__ void __launch_bounds__(TB)
k_cta_loss_finalise(const float* __restrict__ rw, const float* __restrict__ rce, const float* __restrict__ rcl, int64_t n,
                    float lamb, float* __restrict__ out, float* __restrict__ scal) {
    __shared__ double red[TB];
    double w = 0.0, num = 0.0, cl = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += TB) {
        w += (double)rw[i];
        num += (double)rw[i] * (double)rce[i];
        cl += (double)rcl[i];
    }
    w = block_sum_d(w, red);
    num = block_sum_d(num, red);
    cl = block_sum_d(cl, red);
    if (threadIdx.x == 0) {
        const float W = (float)w;                          // the reference's .item(): a constant of the backward pass
        const float local = (float)(num / (double)W), c = (float)(cl / (double)n);
        out[0] = local * (1.f - lamb) + c * lamb;
        out[1] = local;
        out[2] = c;
        scal[0] = W;
    }
}

// ---- model loss, gradients: the prototype part, the folded all-pairs part, the chain through F.normalize -------------
__global__ void __launch_bounds__(TB)
k_cta_rows_bwd(const float* __restrict__ Fh, const float* __restrict__ fnrm, const float* __restrict__ Ch,
               const float* __restrict__ logits, const int32_t* __restrict__ predv, const float* __restrict__ Rpart,
               const float* __restrict__ Gpart, int s, int64_t n, int d, int C, float inv_tau, float lamb,
               const float* __restrict__ rce, const float* __restrict__ cvec, const float* __restrict__ scal,
               float* __restrict__ dfeat, float* __restrict__ dlogits) {
    __shared__ float gsl[ROWS][GDA_WAVE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * ROWS + wv;
    const bool live = row < n;
    const int64_t i = live ? row : n - 1;                  // a wavefront past the end recomputes the last row, stores nothing
    const int pred = uniform_class(predv[i], C);
    const float R = fold_splits(Rpart, n, i, s);
    const float* fh = Fh + i * d;
    const ProtoRow p = proto_row(fh, Ch, lane, C, d, pred, inv_tau, R);
    const float W = scal[0], ce = rce[i], cD = cvec[i];
    const float lg = lane < C ? logits[i * C + lane] : -INFINITY;
    const float mx = wave_max(lg);
    const float lse = mx + logf(wave_sum(lane < C ? expf(lg - mx) : 0.f));
    if (live && lane < C) dlogits[i * C + lane] = (1.f - lamb) * (p.w / W) * (expf(lg - lse) - (lane == pred ? 1.f : 0.f));
    float gs = 0.f;
    if (lane == pred) gs = -lamb * ((p.pos * inv_tau) / p.D) / (p.q + 1e-8f) / (float)n + (1.f - lamb) * ce / W;
    else if (lane < C) gs = cD * p.ex * inv_tau;
    gsl[wv][lane] = gs;
    __syncthreads();
    float g[GDA_WGCN_MAX_WIDTH / GDA_WAVE];
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < GDA_WGCN_MAX_WIDTH / GDA_WAVE; ++t) {
        const int k = lane + GDA_WAVE * t;
        g[t] = 0.f;
        if (k < d) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = fmaf(gsl[wv][c], Ch[(int64_t)c * d + k], a);
            g[t] = a + inv_tau * fold_splits(Gpart, n * d, i * d + k, s);
            dot = fmaf(g[t], fh[k], dot);
        }
    }
    dot = wave_sum(dot);
    const float nr = fnrm[i];
#pragma unroll
    for (int t = 0; t < GDA_WGCN_MAX_WIDTH / GDA_WAVE; ++t) {
        const int k = lane + GDA_WAVE * t;
        if (live && k < d) dfeat[i * d + k] = nr >= NORM_EPS ? (g[t] - fh[k] * dot) / nr : g[t] / NORM_EPS;
    }
}

// ---- top-K1: (value descending, index ascending) is the order everywhere; NaN counts as +inf, as torch.topk has it,
//      and val holds that +inf ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool better(float v, int j, float ev, int ej) { return v > ev || (v == ev && j < ej); }

__global__ void __launch_bounds__(TB)
k_cta_knn(const float* __restrict__ F, int64_t n, const float* __restrict__ M, int64_t nm, int d, int K1, int tps,
          float* __restrict__ pval, int32_t* __restrict__ pidx, bool vec) {
    __shared__ TileLds L;
    __shared__ float Ts[TILE][LDT];
    __shared__ float lv[MAXK1][TB];
    __shared__ int li[MAXK1][TB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, la = lane & 31, ka = lane >> 5;
    const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
    const int r = tid & 63, q = tid >> 6;                  // the scan: row r, columns 16 q .. 16 q + 15 of every tile
    const int64_t i0 = (int64_t)blockIdx.x * TILE;
    const int64_t ntiles = (nm + TILE - 1) / TILE;
    const int64_t jt0 = (int64_t)blockIdx.y * tps, jt1 = jt0 + tps < ntiles ? jt0 + tps : ntiles;
    for (int k = 0; k < K1; ++k) {
        lv[k][tid] = -INFINITY;
        li[k][tid] = 0x7fffffff;
    }
    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = jt * TILE;
        const f32x16 acc = tile_product(F, n, i0, M, nm, j0, d, vec, L);   // its barriers also fence the scan before
#pragma unroll
        for (int e = 0; e < 16; ++e) Ts[wi + (e & 3) + 8 * (e >> 2) + 4 * ka][wj + la] = acc[e];
        __syncthreads();
        for (int c = 0; c < 16; ++c) {
            const int64_t j = j0 + 16 * q + c;
            if (j >= nm) break;
            float v = Ts[r][16 * q + c];
            if (v != v) v = INFINITY;
            if (!better(v, (int)j, lv[K1 - 1][tid], li[K1 - 1][tid])) continue;
            int p = K1 - 1;
            while (p > 0 && better(v, (int)j, lv[p - 1][tid], li[p - 1][tid])) {
                lv[p][tid] = lv[p - 1][tid];
                li[p][tid] = li[p - 1][tid];
                --p;
            }
            lv[p][tid] = v;
            li[p][tid] = (int)j;
        }
    }
    __syncthreads();
    if (q == 0 && i0 + r < n) {                            // the row's four lists into one
        int h[4] = {0, 0, 0, 0};
        const int64_t o = ((int64_t)blockIdx.y * n + i0 + r) * K1;
        for (int k = 0; k < K1; ++k) {
            int b = -1;
            float bv = 0.f;
            int bj = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (h[t] >= K1) continue;
                const float v = lv[h[t]][r + TILE * t];
                const int j = li[h[t]][r + TILE * t];
                if (b < 0 || better(v, j, bv, bj)) { b = t; bv = v; bj = j; }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) h[t] += t == b;
            pval[o + k] = bv;
            pidx[o + k] = bj;
        }
    }
}

__global__ void __launch_bounds__(TB)
k_cta_knn_merge(const float* __restrict__ pval, const int32_t* __restrict__ pidx, int64_t n, int64_t nm, int K1, int s,
                float* __restrict__ val, int32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    int h[MAXS];
#pragma unroll
    for (int t = 0; t < MAXS; ++t) h[t] = 0;
    for (int k = 0; k < K1; ++k) {
        int b = -1, bj = 0;
        float bv = 0.f;
#pragma unroll
        for (int t = 0; t < MAXS; ++t) {
            if (t >= s || h[t] >= K1) continue;
            const int64_t o = ((int64_t)t * n + i) * K1 + h[t];
            const float v = pval[o];
            const int j = pidx[o];
            if (b < 0 || better(v, j, bv, bj)) { b = t; bv = v; bj = j; }
        }
#pragma unroll
        for (int t = 0; t < MAXS; ++t) h[t] += t == b;
        val[i * K1 + k] = bv;
        idx[i * K1 + k] = in_range(bj, nm) ? bj : 0;
    }
}

// ---- test_time_loss, first: softmax, its arg-max (first of equals), the entropy and the log-sum-exp per row ------------
__global__ void __launch_bounds__(TB)
k_tt_rows(const float* __restrict__ logits, int64_t n, int C, float* __restrict__ ent, int32_t* __restrict__ pred,
          float* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (i >= n) return;
    const float lg = lane < C ? logits[i * C + lane] : -INFINITY;
    const float mx = wave_max(lg);
    const float ex = lane < C ? expf(lg - mx) : 0.f;
    const float se = wave_sum(ex);
    const float p = ex / se;
    const float pm = wave_max(lane < C ? p : -INFINITY);
    const unsigned long long top = __ballot(lane < C && p == pm);
    const float e = wave_sum(lane < C ? -p * logf(p + 1e-8f) : 0.f);
    if (lane == 0) {
        ent[i] = e;
        pred[i] = top ? __ffsll((long long)top) - 1 : 0;
        lse[i] = mx + logf(se);
    }
}

// ---- the selection's numbers in one workgroup: mean entropy, est_p, per class int(c_num * est_p / 5) ------------------
struct TtStats { int quota[MAXC]; int nsel; };

__global__ void __launch_bounds__(STB)
k_tt_stats(const float* __restrict__ ent, const int32_t* __restrict__ pred, int64_t n, int C, TtStats* __restrict__ st) {
    __shared__ double red[STB];
    __shared__ int cnum[MAXC];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += STB) a += (double)ent[i];
    a = block_sum_d(a, red);
    const float mean = (float)(a / (double)n);
    double lt = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += STB) lt += ent[i] < mean ? 1.0 : 0.0;
    lt = block_sum_d(lt, red);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = wv; c < C; c += STB / GDA_WAVE) {
        double k = 0.0;
        for (int64_t i = lane; i < n; i += GDA_WAVE) k += pred[i] == c ? 1.0 : 0.0;
        k = wave_sum(k);
        if (lane == 0) cnum[c] = (int)k;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double est_p = lt / (double)n;
        int total = 0;
        for (int c = 0; c < MAXC; ++c) {
            const int qc = c < C ? (int)((double)cnum[c] * est_p / 5.0) : 0;
            st->quota[c] = qc;
            total += qc;
        }
        st->nsel = total;
    }
}

// ---- rank of a row among its predicted class by (entropy, index): a counting rank, no sort ----------------------------
__global__ void __launch_bounds__(TB)
k_tt_rank(const float* __restrict__ ent, const int32_t* __restrict__ pred, int64_t n, int C,
          const TtStats* __restrict__ st, int32_t* __restrict__ sel) {
    __shared__ float es[TB];
    __shared__ int ps[TB];
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    const float ei = i < n ? ent[i] : 0.f;
    const int pi = i < n ? pred[i] : -1;
    int rank = 0;
    for (int64_t j0 = 0; j0 < n; j0 += TB) {
        __syncthreads();
        const int64_t j = j0 + threadIdx.x;
        es[threadIdx.x] = j < n ? ent[j] : 0.f;
        ps[threadIdx.x] = j < n ? pred[j] : -2;
        __syncthreads();
        const int m = n - j0 < TB ? (int)(n - j0) : TB;
        for (int t = 0; t < m; ++t)
            rank += ps[t] == pi && (es[t] < ei || (es[t] == ei && j0 + t < i));
    }
    if (i < n) sel[i] = in_range(pi, C) && rank < st->quota[pi] ? 1 : 0;
}

// ---- other[c] = sum over c' != c of the class sums, in class order ------------------------------------------------------
__global__ void __launch_bounds__(TB)
k_tt_other(const float* __restrict__ csum, int C, int d, float* __restrict__ other) {
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= (int64_t)C * d) return;
    const int c = (int)(e / d), k = (int)(e % d);
    float a = 0.f;
    for (int o = 0; o < C; ++o)
        if (o != c) a += csum[(int64_t)o * d + k];
    other[e] = a;
}

// ---- test_time_loss per row: the selected rows' cross-entropy, the neighbour and the negative term, both gradients -----
__global__ void __launch_bounds__(TB)
k_tt_loss_rows(const float* __restrict__ logits, const float* __restrict__ feat, const float* __restrict__ mem,
               const int32_t* __restrict__ nn, const float* __restrict__ other, const float* __restrict__ ccnt,
               const int32_t* __restrict__ predv, const float* __restrict__ lsev, const int32_t* __restrict__ sel,
               const TtStats* __restrict__ st, int64_t n, int64_t nm, int d, int C, int K1, float* __restrict__ rce,
               float* __restrict__ rnb, float* __restrict__ rng, float* __restrict__ dlogits, float* __restrict__ dfeat) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (i >= n) return;
    const int pred = uniform_class(predv[i], C);
    const bool chosen = sel[i] != 0;
    const float nsel = (float)st->nsel, lse = lsev[i];
    const float lg = lane < C ? logits[i * C + lane] : 0.f;
    if (lane < C) dlogits[i * C + lane] = chosen ? (expf(lg - lse) - (lane == pred ? 1.f : 0.f)) / nsel : 0.f;
    const float ce = chosen ? lse - bcast(lg, pred) : 0.f;
    const int K = K1 - 1;
    const float neg = (float)nm - ccnt[pred];
    const float cnb = -0.1f / ((float)n * (float)K), cng = 0.1f / (float)n;
    float a = 0.f, b = 0.f;
    for (int k = lane; k < d; k += GDA_WAVE) {
        float nb = 0.f;
        for (int t = 1; t < K1; ++t) {                     // rank 1 is dropped, whichever row it is
            const int j = nn[i * K1 + t];
            if (in_range(j, nm)) nb += mem[(int64_t)j * d + k];
        }
        const float ok = other[(int64_t)pred * d + k], fk = feat[i * d + k];
        a = fmaf(fk, nb, a);
        b = fmaf(fk, ok, b);
        dfeat[i * d + k] = cnb * nb + cng * (ok / neg);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        rce[i] = ce;
        rnb[i] = a / (float)K;
        rng[i] = b / neg;
    }
}

__global__ void __launch_bounds__(TB)
k_tt_finalise(const float* __restrict__ rce, const float* __restrict__ rnb, const float* __restrict__ rng, int64_t n,
              const TtStats* __restrict__ st, float* __restrict__ out) {
    __shared__ double red[TB];
    double ce = 0.0, nb = 0.0, ng = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += TB) {
        ce += (double)rce[i];
        nb += (double)rnb[i];
        ng += (double)rng[i];
    }
    ce = block_sum_d(ce, red);
    nb = block_sum_d(nb, red);
    ng = block_sum_d(ng, red);
    if (threadIdx.x == 0) {
        const float c = (float)(ce / (double)st->nsel);    // no selected row: 0 / 0, torch's mean over no rows
        const float b = (float)(nb / (double)n), g = (float)(ng / (double)n);
        out[0] = (c - b * 0.1f) + g * 0.1f;
        out[1] = c;
        out[2] = b;
        out[3] = g;
    }
}

// workspace layouts, in floats
struct LossWs { float *Fh, *Ch, *fnrm, *cnrm, *Rpart, *cvec, *rw, *rce, *rcl, *scal, *Gpart; size_t floats; };
LossWs loss_ws(void* base, int64_t n, int64_t d, int64_t c) {
    const Split sp = make_split(n, n);
    LossWs w;
    float* p = static_cast<float*>(base);
    auto take = [&](size_t k) { float* q = p; p += (k + 3) / 4 * 4; return q; };
    w.Fh = take((size_t)n * d);
    w.Ch = take((size_t)c * d);
    w.fnrm = take(n);
    w.cnrm = take(c);
    w.Rpart = take((size_t)sp.s * n);
    w.cvec = take(n);
    w.rw = take(n);
    w.rce = take(n);
    w.rcl = take(n);
    w.scal = take(4);
    w.Gpart = take((size_t)sp.s * n * d);
    w.floats = (size_t)(p - static_cast<float*>(base));
    return w;
}

struct TtWs { float *ent, *lse, *other, *rce, *rnb, *rng; TtStats* st; size_t floats; };
TtWs tt_ws(void* base, int64_t n, int64_t d, int64_t c) {
    TtWs w;
    float* p = static_cast<float*>(base);
    auto take = [&](size_t k) { float* q = p; p += (k + 3) / 4 * 4; return q; };
    w.ent = take(n);
    w.lse = take(n);
    w.other = take((size_t)c * d);
    w.rce = take(n);
    w.rnb = take(n);
    w.rng = take(n);
    w.st = reinterpret_cast<TtStats*>(take(sizeof(TtStats) / sizeof(float)));
    w.floats = (size_t)(p - static_cast<float*>(base));
    return w;
}

bool cta_dims_ok(int64_t n, int64_t d, int64_t c) { return n >= 1 && d >= 1 && c >= 1 && n < LIM / 64 * 32 && n * d < LIM * 16; }

}  // namespace

extern "C" size_t gda_cta_loss_workspace_bytes(int64_t n, int64_t d, int64_t c) {
    if (!cta_dims_ok(n, d, c) || d > GDA_WGCN_MAX_WIDTH || c > MAXC) return 256;
    return gda_align_up(loss_ws(nullptr, n, d, c).floats * sizeof(float), 256);
}

extern "C" int gda_cta_model_loss_f32(const float* feat, const float* logits, const float* proto, const int32_t* pred,
                                      int64_t n, int64_t d, int64_t c, float tau, float lamb, float* out, float* dfeat,
                                      float* dlogits, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (!cta_dims_ok(n, d, c) || !(tau > 0.f)) return GDA_E_SIZE;
    if (d > GDA_WGCN_MAX_WIDTH || c > MAXC) return GDA_E_UNSUPPORTED;
    if (!feat || !logits || !proto || !pred || !out || !dfeat || !dlogits || !workspace) return GDA_E_NULL;
    if (!aligned(feat, 4) || !aligned(logits, 4) || !aligned(proto, 4) || !aligned(pred, 4) || !aligned(out, 4)
        || !aligned(dfeat, 4) || !aligned(dlogits, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (dfeat == feat || dlogits == logits) return GDA_E_ALIAS;
    if (workspace_bytes < gda_cta_loss_workspace_bytes(n, d, c)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const LossWs w = loss_ws(workspace, n, d, c);
    const Split sp = make_split(n, n);
    const float inv_tau = 1.f / tau;
    const bool vec = d % 4 == 0;                           // Fh is 16-byte aligned in the workspace
    const unsigned rows = (unsigned)gda_cdiv(n, ROWS);
    const dim3 grid((unsigned)gda_cdiv(n, TILE), (unsigned)sp.s);
    k_cta_normalize<<<rows, TB, 0, st>>>(feat, n, (int)d, w.Fh, w.fnrm);
    GDA_LAUNCH_CHECK();
    k_cta_normalize<<<(unsigned)gda_cdiv(c, ROWS), TB, 0, st>>>(proto, c, (int)d, w.Ch, w.cnrm);
    GDA_LAUNCH_CHECK();
    k_cta_pairs<false><<<grid, TB, 0, st>>>(w.Fh, n, (int)d, inv_tau, sp.tps, nullptr, w.Rpart, nullptr, vec);
    GDA_LAUNCH_CHECK();
    k_cta_rows_mid<<<rows, TB, 0, st>>>(w.Fh, w.Ch, logits, pred, w.Rpart, sp.s, n, (int)d, (int)c, inv_tau, lamb, w.rw,
                                        w.rce, w.rcl, w.cvec);
    GDA_LAUNCH_CHECK();
    k_cta_loss_finalise<<<1, TB, 0, st>>>(w.rw, w.rce, w.rcl, n, lamb, out, w.scal);
    GDA_LAUNCH_CHECK();
    k_cta_pairs<true><<<grid, TB, 0, st>>>(w.Fh, n, (int)d, inv_tau, sp.tps, w.cvec, nullptr, w.Gpart, vec);
    GDA_LAUNCH_CHECK();
    k_cta_rows_bwd<<<rows, TB, 0, st>>>(w.Fh, w.fnrm, w.Ch, logits, pred, w.Rpart, w.Gpart, sp.s, n, (int)d, (int)c,
                                        inv_tau, lamb, w.rce, w.cvec, w.scal, dfeat, dlogits);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_cta_knn_workspace_bytes(int64_t n, int64_t nm, int64_t k1) {
    if (n < 1 || nm < 1 || k1 < 1 || k1 > MAXK1 || n >= LIM / 2 || nm >= LIM / 2) return 256;
    const Split sp = make_split(n, nm);
    return gda_align_up((size_t)2 * sp.s * n * k1 * sizeof(float), 256);
}

extern "C" int gda_cta_knn_f32(const float* F, const float* M, int64_t n, int64_t nm, int64_t d, int64_t k1, int32_t* idx,
                               float* val, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || nm < 1 || d < 1 || k1 < 1 || n >= LIM / 2 || nm >= LIM / 2 || nm < k1) return GDA_E_SIZE;
    if (d > GDA_WGCN_MAX_WIDTH || k1 > MAXK1) return GDA_E_UNSUPPORTED;
    if (!F || !M || !idx || !val || !workspace) return GDA_E_NULL;
    if (!aligned(F, 4) || !aligned(M, 4) || !aligned(idx, 4) || !aligned(val, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_cta_knn_workspace_bytes(n, nm, k1)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Split sp = make_split(n, nm);
    float* pval = static_cast<float*>(workspace);
    int32_t* pidx = reinterpret_cast<int32_t*>(pval + (size_t)sp.s * n * k1);
    const bool vec = d % 4 == 0 && aligned(F, 16) && aligned(M, 16);
    k_cta_knn<<<dim3((unsigned)gda_cdiv(n, TILE), (unsigned)sp.s), TB, 0, st>>>(F, n, M, nm, (int)d, (int)k1, sp.tps, pval,
                                                                                pidx, vec);
    GDA_LAUNCH_CHECK();
    k_cta_knn_merge<<<(unsigned)gda_cdiv(n, TB), TB, 0, st>>>(pval, pidx, n, nm, (int)k1, sp.s, val, idx);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_cta_tt_workspace_bytes(int64_t n, int64_t d, int64_t c) {
    if (!cta_dims_ok(n, d, c) || d > GDA_WGCN_MAX_WIDTH || c > MAXC) return 256;
    return gda_align_up(tt_ws(nullptr, n, d, c).floats * sizeof(float), 256);
}

extern "C" int gda_cta_test_time_f32(const float* logits, const float* feat, const float* mem, const int32_t* nn_idx,
                                     const float* csum, const float* ccnt, int64_t n, int64_t nm, int64_t d, int64_t c,
                                     int64_t k1, float* out, float* dlogits, float* dfeat, int32_t* pred, int32_t* sel,
                                     void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (!cta_dims_ok(n, d, c) || nm < 1 || nm >= LIM / 2 || k1 < 2 || nm < k1) return GDA_E_SIZE;
    if (d > GDA_WGCN_MAX_WIDTH || c > MAXC || k1 > MAXK1) return GDA_E_UNSUPPORTED;
    if (!logits || !feat || !mem || !nn_idx || !csum || !ccnt || !out || !dlogits || !dfeat || !pred || !sel || !workspace)
        return GDA_E_NULL;
    if (!aligned(logits, 4) || !aligned(feat, 4) || !aligned(mem, 4) || !aligned(nn_idx, 4) || !aligned(csum, 4)
        || !aligned(ccnt, 4) || !aligned(out, 4) || !aligned(dlogits, 4) || !aligned(dfeat, 4) || !aligned(pred, 4)
        || !aligned(sel, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (dlogits == logits || dfeat == feat) return GDA_E_ALIAS;
    if (workspace_bytes < gda_cta_tt_workspace_bytes(n, d, c)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const TtWs w = tt_ws(workspace, n, d, c);
    const unsigned rows = (unsigned)gda_cdiv(n, ROWS);
    k_tt_rows<<<rows, TB, 0, st>>>(logits, n, (int)c, w.ent, pred, w.lse);
    GDA_LAUNCH_CHECK();
    k_tt_stats<<<1, STB, 0, st>>>(w.ent, pred, n, (int)c, w.st);
    GDA_LAUNCH_CHECK();
    k_tt_rank<<<(unsigned)gda_cdiv(n, TB), TB, 0, st>>>(w.ent, pred, n, (int)c, w.st, sel);
    GDA_LAUNCH_CHECK();
    k_tt_other<<<(unsigned)gda_cdiv(c * d, TB), TB, 0, st>>>(csum, (int)c, (int)d, w.other);
    GDA_LAUNCH_CHECK();
    k_tt_loss_rows<<<rows, TB, 0, st>>>(logits, feat, mem, nn_idx, w.other, ccnt, pred, w.lse, sel, w.st, n, nm, (int)d,
                                        (int)c, (int)k1, w.rce, w.rnb, w.rng, dlogits, dfeat);
    GDA_LAUNCH_CHECK();
    k_tt_finalise<<<1, TB, 0, st>>>(w.rce, w.rnb, w.rng, n, w.st, out);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
