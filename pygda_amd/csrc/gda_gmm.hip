// The device side of pygda/nn/gmm_clustering.py: the EM steps of a full-covariance Gaussian mixture (what the reference
// runs through sklearn on the host) for R restarts at once, and the assignment step of a k-means.
//
//   gda_gmm_mstep_f32    weights, means and CENTRED covariances from the responsibilities.  Thin R^T X partials over
//                        row slabs, folded in slab order; then (X - mu_k)^T diag(r_k) (X - mu_k) on
//                        v_mfma_f32_32x32x2_f32 with centring and weight applied while the operand is staged, 64 x 64
//                        tiles on and below the diagonal only, slab partials added in slab order and mirrored.
//   gda_gmm_factor_f32   one workgroup per (run, component): Cholesky in float64 in LDS, the triangular inverse in the
//                        free upper triangle, stored transposed in fp32 (sklearn's precisions_cholesky_), sum log diag.
//   gda_gmm_estep_f32    (x - mu_k) P_k on the matrix cores, squared row norm in the epilogue (the product is never
//                        stored), row log-sum-exp, responsibilities; the sum of the row lse in float64 in a fixed order
//                        and the close of the iteration (lower bound, change, flags).
//   gda_kmeans_step_f32  nearest-centre labels (lowest index on a tie), optional distances, per-centre sums and counts.
//   gda_gmm_label_sums_f32, gda_lsa_cos_f32 / gda_lsa_cost_f64, gda_gmm_relabel_f32
//                        the tail of GMMClustering.forward without a host read (JHGDA's pseudo='gmm'): per-label sums of
//                        the embeddings, the linear assignment of the cosine cost between the two sets of centres (scipy's
//                        shortest augmenting paths in float64, one wave), then cluster -> label, the re-arranged
//                        probabilities and the one-hot rows.  A run whose `failed` is set keeps the labels handed in.
//
// The freeze rule: every run owns a gda_gmm_state.  A kernel leaves a run whose `failed` flag is set untouched; E-step
// kernels also leave a run with `converged` >= 1 untouched, M-step and factor kernels one with `converged` >= 2 (the
// iteration that converges still owns its M-step; the next E-step call moves 1 -> 2).  Launching more iterations than a
// run needs therefore changes none of its bits.  No float atomics anywhere: every sum is formed in a fixed order.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int MAX_DIM = 128, MAX_K = 32, MAX_RUNS = 8;

using State = gda_gmm_state;   // 32 bytes per run
static_assert(sizeof(State) == 32, "gda_gmm_state is 32 bytes");

__device__ __forceinline__ bool frozen_m(const State* st, int run) {
    return st && (st[run].failed != 0 || st[run].converged >= 2);
}

// ---- M-step ----------------------------------------------------------------------------------------------------------
constexpr int GT = 64, GDK = 32, GLD = GT + 4;
constexpr int MSTEP_BLOCKS = 2048;         // tiles x slabs aimed at for a full batch of runs

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct MPlan {
    int64_t tiles_1d, ntiles, slabs, slab_rows;
    size_t sum_off, nk_off, cov_off, bytes;
};

MPlan mstep_plan(int64_t n, int64_t d, int64_t k, int64_t r) {
    MPlan p{};
    p.tiles_1d = gda_cdiv(d, GT);
    p.ntiles = p.tiles_1d * (p.tiles_1d + 1) / 2;
    int64_t cap = MSTEP_BLOCKS / (p.ntiles * k * MAX_RUNS);    // not a function of r: a run sums the same slabs alone
    if (cap < 1) cap = 1;
    int64_t s = gda_cdiv(n, 256);
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    p.slab_rows = gda_cdiv(gda_cdiv(n, s), GDK) * GDK;
    p.slabs = gda_cdiv(n, p.slab_rows);
    p.sum_off = 0;
    p.nk_off = gda_align_up((size_t)(r * p.slabs * k * (d + 1)) * sizeof(float), 16);
    p.cov_off = p.nk_off + gda_align_up((size_t)(r * k) * sizeof(float), 16);
    p.bytes = p.cov_off + (size_t)(r * k * p.slabs * p.ntiles) * GT * GT * sizeof(float);
    return p;
}

// part[run][slab][k][c] = sum over the slab's rows, in row order, of resp[row, k] * (c < d ? x[row, c] : 1)
__global__ void __launch_bounds__(TB)
k_mstep_sums(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int K, const float* __restrict__ resp,
             int64_t slab_rows, const State* __restrict__ st, float* __restrict__ part) {
    const int run = blockIdx.y;
    if (frozen_m(st, run)) return;
    const int64_t kbeg = (int64_t)blockIdx.x * slab_rows, kend = min(n, kbeg + slab_rows);
    const float* rr = resp + (int64_t)run * n * K;
    float* out = part + ((int64_t)run * gridDim.x + blockIdx.x) * K * (d + 1);
    for (int p = threadIdx.x; p < K * (d + 1); p += TB) {
        const int k = p / (d + 1), c = p % (d + 1);
        float a = 0.f;
        if (c < d) {
            for (int64_t row = kbeg; row < kend; ++row) a += rr[row * K + k] * x[row * ldx + c];
        } else {
            for (int64_t row = kbeg; row < kend; ++row) a += rr[row * K + k];
        }
        out[p] = a;
    }
}

// one workgroup per (component, run): nk = sum + 10 eps, means = sums / nk, weights = nk / sum_k nk
__global__ void __launch_bounds__(TB)
k_mstep_means(int d, int K, int slabs, const State* __restrict__ st, const float* __restrict__ part,
              float* __restrict__ nk_ws, float* __restrict__ weights, float* __restrict__ means) {
    __shared__ float nk_s[MAX_K];
    __shared__ float tot_s;
    const int k = blockIdx.x, run = blockIdx.y, t = threadIdx.x;
    if (frozen_m(st, run)) return;
    const float* base = part + (int64_t)run * slabs * K * (d + 1);
    if (t < K) {
        float a = 0.f;
        for (int z = 0; z < slabs; ++z) a += base[((int64_t)z * K + t) * (d + 1) + d];
        nk_s[t] = a + 10.f * 1.1920928955078125e-7f;
    }
    __syncthreads();
    if (t == 0) {
        float a = 0.f;
        for (int q = 0; q < K; ++q) a += nk_s[q];
        tot_s = a;
    }
    __syncthreads();
    const float nk = nk_s[k];
    if (t < d) {
        float a = 0.f;
        for (int z = 0; z < slabs; ++z) a += base[((int64_t)z * K + k) * (d + 1) + t];
        means[((int64_t)run * K + k) * d + t] = a / nk;
    }
    if (t == 0) {
        nk_ws[run * K + k] = nk;
        weights[run * K + k] = nk / tot_s;
    }
}

// x[r, c] - mu[c] inside [0, rows) x [0, d), zero outside (the columns d .. ldx of a panel are never read)
__device__ __forceinline__ float ld_centred(const float* __restrict__ x, int64_t ldx, const float* __restrict__ mu,
                                            int64_t r, int c, int64_t rows, int d) {
    return (r < rows && c < d) ? x[r * ldx + c] - mu[c] : 0.f;
}

// blockIdx.x = k * ntiles + t, tile t = ti (ti + 1) / 2 + tj (tj <= ti); blockIdx.y = slab; blockIdx.z = run
__global__ void __launch_bounds__(TB)
k_mstep_cov(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int K, const float* __restrict__ resp,
            const float* __restrict__ means, int64_t slab_rows, int ntiles, const State* __restrict__ st,
            float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[GDK][GLD];
    __shared__ __attribute__((aligned(16))) float Bs[GDK][GLD];
    const int run = blockIdx.z;
    if (frozen_m(st, run)) return;
    const int k = blockIdx.x / ntiles, t = blockIdx.x % ntiles;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int i0 = ti * GT, j0 = tj * GT;
    const int64_t kbeg = (int64_t)blockIdx.y * slab_rows, kend = min(n, kbeg + slab_rows);
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int ka = lane >> 5, la = lane & 31;
    const int kk = tid / 16, c4 = (tid % 16) * 4;
    const float* rr = resp + (int64_t)run * n * K + k;
    const float* mu = means + ((int64_t)run * K + k) * d;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int64_t k0 = kbeg; k0 < kend; k0 += GDK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t row = k0 + kk + 16 * q;
            const float w = row < kend ? rr[row * K] : 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                As[kk + 16 * q][c4 + e] = w * ld_centred(x, ldx, mu, row, i0 + c4 + e, kend, d);
                Bs[kk + 16 * q][c4 + e] = ld_centred(x, ldx, mu, row, j0 + c4 + e, kend, d);
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < GDK; q += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[q + ka][wi + la], Bs[q + ka][wj + la], acc, 0, 0, 0);
    }
    float* out = part + ((((int64_t)run * K + k) * gridDim.y + blockIdx.y) * ntiles + t) * (GT * GT);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = wi + (r & 3) + 8 * (r >> 2) + 4 * ka;     // C/D layout of the 32x32 MFMA
        out[il * GT + wj + la] = acc[r] + 0.f;
    }
}

// cov[i][j] = cov[j][i] = (sum over the slabs, in slab order, of the lower-triangle entry) / nk + reg on the diagonal
__global__ void __launch_bounds__(TB)
k_mstep_cov_fold(const float* __restrict__ part, int slabs, int ntiles, int d, int K, int R, float reg,
                 const float* __restrict__ nk_ws, const State* __restrict__ st, float* __restrict__ cov) {
    const int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int64_t per = (int64_t)ntiles * GT * GT;
    if (idx >= (int64_t)R * K * per) return;
    const int rk = (int)(idx / per), run = rk / K;
    if (frozen_m(st, run)) return;
    const int64_t rem = idx % per;
    const int t = (int)(rem / (GT * GT)), il = (int)(rem % (GT * GT)) / GT, jl = (int)(rem % GT);
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int i = ti * GT + il, j = tj * GT + jl;
    if (i >= d || j >= d || j > i) return;
    const float* src = part + (int64_t)rk * slabs * per + rem;
    float a = 0.f;
    for (int z = 0; z < slabs; ++z) a += src[z * per];
    a = a / nk_ws[rk];
    if (i == j) a += reg;
    float* c = cov + (int64_t)rk * d * d;
    c[(int64_t)i * d + j] = a;
    c[(int64_t)j * d + i] = a;
}

// ---- factor ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int factor_ld(int d) { return d | 1; }      // odd: a column walk touches every LDS bank

// one workgroup per (component, run).  A [d][ld] float64: the lower triangle becomes L (cov = L L^T); the strict upper
// triangle then receives the inverse, row c = column c of L^-1, each row owned by one thread.
__global__ void __launch_bounds__(TB)
k_factor(const float* __restrict__ cov, int d, int K, State* __restrict__ st, float* __restrict__ prec,
         double* __restrict__ logdet) {
    extern __shared__ double A[];
    __shared__ double red[TB];
    __shared__ int skip;
    const int k = blockIdx.x, run = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) skip = frozen_m(st, run);                    // another component of the run may fail meanwhile: read once
    __syncthreads();
    if (skip) return;
    const int ld = factor_ld(d);
    const float* c = cov + ((int64_t)run * K + k) * d * d;
    for (int e = tid; e < d * d; e += TB) {
        const int i = e / d, j = e % d;
        A[i * ld + j] = j <= i ? (double)c[e] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < d; ++j) {
        const double p = A[j * ld + j];
        if (!(p > 0.0) || !isfinite(p)) {                      // the same value in every thread: a uniform exit
            if (tid == 0) st[run].failed = 1;
            return;
        }
        const double s = sqrt(p);
        __syncthreads();
        for (int i = j + 1 + tid; i < d; i += TB) A[i * ld + j] /= s;
        if (tid == 0) A[j * ld + j] = s;
        __syncthreads();
        const int m = d - j - 1;
        for (int e = tid; e < m * m; e += TB) {
            const int i = j + 1 + e / m, q = j + 1 + e % m;
            if (q <= i) A[i * ld + q] -= A[i * ld + j] * A[q * ld + j];
        }
        __syncthreads();
    }
    // y = column c of L^-1: y[c] = 1 / L[c][c], y[i] = -(sum_{m = c}^{i-1} L[i][m] y[m]) / L[i][i], m descending
    if (tid < d) {
        const int cc = tid;
        const double ycc = 1.0 / A[cc * ld + cc];
        for (int i = cc + 1; i < d; ++i) {
            double s = 0.0;
            for (int m = i - 1; m > cc; --m) s += A[i * ld + m] * A[cc * ld + m];
            s += A[i * ld + cc] * ycc;
            A[cc * ld + i] = -s / A[i * ld + i];
        }
    }
    __syncthreads();
    const double lg = block_sum_d(tid < d ? log(1.0 / A[tid * ld + tid]) : 0.0, red);
    float* P = prec + ((int64_t)run * K + k) * d * d;
    for (int e = tid; e < d * d; e += TB) {
        const int a = e / d, b = e % d;
        const double v = a == b ? 1.0 / A[a * ld + a] : (a < b ? A[a * ld + b] : 0.0);
        P[e] = (float)v;
    }
    if (tid == 0) logdet[run * K + k] = lg;
}

// ---- E-step ----------------------------------------------------------------------------------------------------------
constexpr int ER = 64;                       // rows per workgroup
constexpr int ELD = ER + 4;
constexpr int BLD = MAX_DIM + 4;

__global__ void __launch_bounds__(TB)
k_estep(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int K, const float* __restrict__ weights,
        const float* __restrict__ means, const float* __restrict__ prec, const double* __restrict__ logdet,
        float* __restrict__ resp, const State* __restrict__ st, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Xt[MAX_DIM][ELD];     // the row tile, transposed: Xt[j][row]
    __shared__ __attribute__((aligned(16))) float Bs[GDK][BLD];         // 32 rows of P_k
    __shared__ float mu_s[MAX_DIM];
    __shared__ float red[2][ER];
    __shared__ float sq[ER][MAX_K + 1];                                 // squared norms; the constants stay in float64
    __shared__ double cst_s[MAX_K];
    const int run = blockIdx.y;
    if (st && (st[run].failed != 0 || st[run].converged >= 1)) return;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int rh = wave & 1, cb0 = wave >> 1;
    const int ka = lane >> 5, la = lane & 31;
    const int dpad = (d + 31) / 32 * 32, nj = dpad / 32;
    const int64_t r0 = (int64_t)blockIdx.x * ER;
    for (int e = tid; e < ER * dpad; e += TB) {
        const int row = e / dpad, j = e % dpad;
        Xt[j][row] = (r0 + row < n && j < d) ? x[(r0 + row) * ldx + j] : 0.f;
    }
    for (int k = 0; k < K; ++k) {
        const float* mu = means + ((int64_t)run * K + k) * d;
        const float* P = prec + ((int64_t)run * K + k) * d * d;
        __syncthreads();
        if (tid < MAX_DIM) mu_s[tid] = tid < d ? mu[tid] : 0.f;
        if (tid == TB - 1)                                          // -(d log 2 pi) / 2 + log det + log weight
            cst_s[k] = -0.5 * (double)d * 1.8378770664093453 + logdet[run * K + k] + log((double)weights[run * K + k]);
        f32x16 acc[2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
        for (int jc = 0; jc < nj; ++jc) {
            __syncthreads();
            for (int e = tid; e < GDK * dpad; e += TB) {
                const int jj = e / dpad, c = e % dpad, j = jc * GDK + jj;
                Bs[jj][c] = (j < d && c < d) ? P[(int64_t)j * d + c] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int cb = cb0 + 2 * q;
                if (cb < nj && jc <= cb) {                          // P_k is upper triangular: rows below the block are 0
#pragma unroll
                    for (int kk = 0; kk < GDK; kk += 2) {
                        const int j = jc * GDK + kk + ka;
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(Xt[j][rh * 32 + la] - mu_s[j],
                                                                       Bs[kk + ka][cb * 32 + la], acc[q], 0, 0, 0);
                    }
                }
            }
        }
        // squared norm of the product's rows: this wave's columns, the 32 lanes of a half, then the two column waves
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float s = acc[0][r] * acc[0][r] + acc[1][r] * acc[1][r];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (la == 0) red[cb0][rh * 32 + (r & 3) + 8 * (r >> 2) + 4 * ka] = s;
        }
        __syncthreads();
        if (tid < ER) sq[tid][k] = red[0][tid] + red[1][tid];
    }
    __syncthreads();
    double* lse_s = reinterpret_cast<double*>(&Xt[0][0]);          // the tile is no longer needed
    if (tid < ER) {
        double mine = 0.0;
        if (r0 + tid < n) {
            // the row's log-sum-exp in float64: K values, so that the lower bound carries no float32 rounding of its own
            double m = cst_s[0] - 0.5 * (double)sq[tid][0];
            for (int k = 1; k < K; ++k) m = fmax(m, cst_s[k] - 0.5 * (double)sq[tid][k]);
            double s = 0.0;
            for (int k = 0; k < K; ++k) s += exp(cst_s[k] - 0.5 * (double)sq[tid][k] - m);
            const double lse = m + log(s);
            float* o = resp + ((int64_t)run * n + r0 + tid) * K;
            for (int k = 0; k < K; ++k) o[k] = (float)exp(cst_s[k] - 0.5 * (double)sq[tid][k] - lse);
            mine = lse;
        }
        lse_s[tid] = mine;
    }
    __syncthreads();
    if (tid == 0 && part) {
        double a = 0.0;
        for (int r = 0; r < ER; ++r) a += lse_s[r];
        part[(int64_t)run * gridDim.x + blockIdx.x] = a;
    }
}

// one workgroup per run: lower bound = (sum of the block partials, a fixed strided order) / n, change, flags
__global__ void __launch_bounds__(TB)
k_estep_close(const double* __restrict__ part, int nblk, int64_t n, double tol, State* __restrict__ st) {
    __shared__ double red[TB];
    const int run = blockIdx.x;
    if (st[run].failed != 0 || st[run].converged >= 2) return;
    if (st[run].converged == 1) {                                   // the converging iteration's M-step has run by now
        if (threadIdx.x == 0) st[run].converged = 2;
        return;
    }
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += TB) a += part[(int64_t)run * nblk + b];
    a = block_sum_d(a, red);
    if (threadIdx.x == 0) {
        const double lb = a / (double)n, prev = st[run].lower_bound;
        st[run].prev_lower_bound = prev;
        st[run].lower_bound = lb;
        st[run].n_iter += 1;
        if (fabs(lb - prev) < tol) st[run].converged = 1;
    }
}

// ---- k-means step ----------------------------------------------------------------------------------------------------
constexpr int KR = 64;                        // rows per workgroup
constexpr int KLD = MAX_DIM + 1;

__global__ void __launch_bounds__(TB)
k_kmeans_assign(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int K, const float* __restrict__ centers,
                int metric, int64_t* __restrict__ labels, float* __restrict__ dist, float* __restrict__ part) {
    __shared__ float Xs[KR][KLD];
    __shared__ float Cs[MAX_K][KLD];
    __shared__ float ds[KR][MAX_K + 1];
    __shared__ float xn[KR], cn[MAX_K];
    __shared__ int lab[KR];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * KR;
    for (int e = tid; e < KR * d; e += TB) {
        const int row = e / d, c = e % d;
        Xs[row][c] = r0 + row < n ? x[(r0 + row) * ldx + c] : 0.f;
    }
    for (int e = tid; e < K * d; e += TB) Cs[e / d][e % d] = centers[e];
    __syncthreads();
    if (tid < KR) {
        float a = 0.f;
        if (metric != 1)
            for (int c = 0; c < d; ++c) a += Xs[tid][c] * Xs[tid][c];
        xn[tid] = metric != 1 ? fmaxf(sqrtf(a), 1e-12f) : 1.f;           // F.normalize's eps
    } else if (tid < KR + K) {
        const int k = tid - KR;
        float a = 0.f;
        if (metric != 1)
            for (int c = 0; c < d; ++c) a += Cs[k][c] * Cs[k][c];
        cn[k] = metric != 1 ? fmaxf(sqrtf(a), 1e-12f) : 1.f;
    }
    __syncthreads();
    {
        const int row = tid % KR;
        const float nx = xn[row];
        for (int k = tid / KR; k < K; k += TB / KR) {
            const float nc = cn[k];
            float a = 0.f;
            if (metric == 0) {
                for (int c = 0; c < d; ++c) a += (Xs[row][c] / nx) * (Cs[k][c] / nc);
                a = 0.5f * (1.0f - a);
            } else if (metric == 1) {
                for (int c = 0; c < d; ++c) {
                    const float t = Xs[row][c] - Cs[k][c];
                    a += t * t;
                }
            } else {
                for (int c = 0; c < d; ++c) {
                    const float t = Xs[row][c] / nx - Cs[k][c] / nc;
                    a += t * t;
                }
                a = sqrtf(a);
            }
            ds[row][k] = a;
        }
    }
    __syncthreads();
    if (tid < KR) {
        int best = -1;
        if (r0 + tid < n) {
            best = 0;
            float bv = ds[tid][0];
            for (int k = 1; k < K; ++k)
                if (ds[tid][k] < bv) { bv = ds[tid][k]; best = k; }
            labels[r0 + tid] = best;
            if (dist)
                for (int k = 0; k < K; ++k) dist[(r0 + tid) * K + k] = ds[tid][k];
        }
        lab[tid] = best;
    }
    __syncthreads();
    float* out = part + (int64_t)blockIdx.x * K * (d + 1);
    for (int p = tid; p < K * (d + 1); p += TB) {
        const int k = p / (d + 1), c = p % (d + 1);
        float a = 0.f;
        for (int row = 0; row < KR; ++row)
            if (lab[row] == k) a += c < d ? Xs[row][c] : 1.f;
        out[p] = a;
    }
}

// sums[k][c] / counts[k] = the block partials added in block order
__global__ void __launch_bounds__(TB)
k_kmeans_fold(const float* __restrict__ part, int64_t nblk, int d, int K, float* __restrict__ sums,
              float* __restrict__ counts) {
    const int p = blockIdx.x * TB + threadIdx.x;
    if (p >= K * (d + 1)) return;
    const int k = p / (d + 1), c = p % (d + 1);
    float a = 0.f;
    for (int64_t b = 0; b < nblk; ++b) a += part[b * K * (d + 1) + p];
    if (c < d) sums[k * d + c] = a;
    else counts[k] = a;
}

// ---- per-label sums --------------------------------------------------------------------------------------------------
// part[block][k][c] = the sum over the block's rows with label k, in row order, of (c < d ? x[row, c] : 1); a label
// outside [0, K) belongs to no class.  Folded by k_kmeans_fold in block order.
__global__ void __launch_bounds__(TB)
k_label_part(const float* __restrict__ x, int64_t ldx, int64_t n, int d, int K, const int64_t* __restrict__ labels,
             float* __restrict__ part) {
    __shared__ float Xs[KR][KLD];
    __shared__ int lab[KR];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * KR;
    for (int e = tid; e < KR * d; e += TB) {
        const int row = e / d, c = e % d;
        Xs[row][c] = r0 + row < n ? x[(r0 + row) * ldx + c] : 0.f;
    }
    if (tid < KR) {
        const int64_t l = r0 + tid < n ? labels[r0 + tid] : -1;
        lab[tid] = (l >= 0 && l < K) ? (int)l : -1;
    }
    __syncthreads();
    float* out = part + (int64_t)blockIdx.x * K * (d + 1);
    for (int p = tid; p < K * (d + 1); p += TB) {
        const int k = p / (d + 1), c = p % (d + 1);
        float a = 0.f;
        for (int row = 0; row < KR; ++row)
            if (lab[row] == k) a += c < d ? Xs[row][c] : 1.f;
        out[p] = a;
    }
}

// ---- relabel ---------------------------------------------------------------------------------------------------------
// one thread per row: argmax (lowest index on a tie), cluster -> label, the re-arranged row, the one-hot row.  With the
// run's `failed` set the label is the fallback's.  c2l == NULL: the identity (the argmax of given probabilities alone).
__global__ void __launch_bounds__(TB)
k_relabel(const float* __restrict__ resp, int64_t n, int K, const int* __restrict__ c2l, const int* __restrict__ shuf,
          const int64_t* __restrict__ fallback, const State* __restrict__ st, float* __restrict__ prob,
          int64_t* __restrict__ labels, float* __restrict__ hot) {
    const int64_t row = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (row >= n) return;
    const float* p = resp + row * K;
    int best = 0;
    float bv = p[0];
    for (int k = 1; k < K; ++k)
        if (p[k] > bv) { bv = p[k]; best = k; }
    int lab = c2l ? c2l[best] : best;
    if (st && st[0].failed != 0 && fallback) lab = (int)fallback[row];
    if (lab < 0 || lab >= K) lab = 0;                           // never an index outside the row
    labels[row] = lab;
    if (prob)
        for (int j = 0; j < K; ++j) {
            int s = shuf ? shuf[j] : j;
            if (s < 0 || s >= K) s = j;
            prob[row * K + j] = p[s];
        }
    if (hot)
        for (int j = 0; j < K; ++j) hot[row * K + j] = j == lab ? 1.f : 0.f;
}

// ---- linear assignment -----------------------------------------------------------------------------------------------
constexpr int LSA_LD = MAX_DIM + 1;

// (value, index) minimum over the wave, the lowest index on an exact tie; every lane receives it
__device__ __forceinline__ void wave_argmin(double& v, int& idx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        if (ov < v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
}

// One wave.  The cost [K][K] in float64 in LDS: given, or 0.5 (1 - cos) of the rows of tgt and src normalised as
// F.normalize does.  Then the shortest-augmenting-path solver of scipy.optimize.linear_sum_assignment (rows = clusters in
// order, duals u / v): lane j owns column j (v, the shortest path cost, its predecessor row, its row) and row j (u, its
// column, whether the tree holds it).  c2l[i] = the column of row i, shuf = its inverse.  A non-finite cost, or a run
// that has failed already: the identity, and `failed` set.
__global__ void __launch_bounds__(64)
k_lsa(const float* __restrict__ tgt, const float* __restrict__ src, const double* __restrict__ cost_in, int K, int d,
      int* __restrict__ c2l, int* __restrict__ shuf, State* __restrict__ st) {
    __shared__ double C[MAX_K][MAX_K];
    __shared__ float Ts[MAX_K][LSA_LD];
    __shared__ float Ss[MAX_K][LSA_LD];
    __shared__ double nrm[2 * MAX_K];
    const int lane = threadIdx.x;
    const double INF = __builtin_huge_val();
    bool bad = st && st[0].failed != 0;
    if (!bad) {
        if (cost_in) {
            for (int e = lane; e < K * K; e += 64) C[e / K][e % K] = cost_in[e];
        } else {
            for (int e = lane; e < K * d; e += 64) {
                Ts[e / d][e % d] = tgt[e];
                Ss[e / d][e % d] = src[e];
            }
            __syncthreads();
            {
                const int r = lane & 31;
                if (r < K) {
                    const float* row = lane < 32 ? Ts[r] : Ss[r];
                    double a = 0.0;
                    for (int c = 0; c < d; ++c) a += (double)row[c] * (double)row[c];
                    nrm[lane] = fmax(sqrt(a), 1e-12);
                }
            }
            __syncthreads();
            for (int e = lane; e < K * K; e += 64) {
                const int i = e / K, j = e % K;
                const double ni = nrm[i], nj = nrm[32 + j];
                double a = 0.0;
                for (int c = 0; c < d; ++c) a += ((double)Ts[i][c] / ni) * ((double)Ss[j][c] / nj);
                C[i][j] = 0.5 * (1.0 - a);
            }
        }
        __syncthreads();
        bool mine = false;
        for (int e = lane; e < K * K; e += 64) mine |= !isfinite(C[e / K][e % K]);
        bad = __any(mine);
    }
    double u = 0.0, v = 0.0;
    int col4row = -1, row4col = -1;
    for (int cur = 0; cur < K && !bad; ++cur) {
        double spc = INF, minval = 0.0;
        int path = -1, i = cur, sink = -1;
        bool SC = lane >= K, SR = false;
        for (int it = 0; it < K && sink < 0; ++it) {
            if (lane == i) SR = true;
            const double ui = __shfl(u, i, 64);
            if (!SC) {
                const double r = minval + C[i][lane] - ui - v;
                if (r < spc) { spc = r; path = i; }
            }
            double lowest = SC ? INF : spc;
            int j = lane;
            wave_argmin(lowest, j);
            if (!(lowest < INF)) break;                          // no column left to reach: not with finite costs
            minval = lowest;
            if (lane == j) SC = true;
            const int r4c = __shfl(row4col, j, 64);
            if (r4c < 0) sink = j;
            else i = r4c;
        }
        if (sink < 0) { bad = true; break; }
        const double spc_mine = __shfl(spc, col4row < 0 ? 0 : col4row, 64);
        if (lane == cur) u += minval;
        else if (SR) u += minval - spc_mine;
        if (SC && lane < K) v -= minval - spc;
        int j = sink;
        for (int s = 0; s < K; ++s) {
            const int pi = __shfl(path, j, 64);
            if (lane == j) row4col = pi;
            const int old = __shfl(col4row, pi, 64);
            if (lane == pi) col4row = j;
            j = old;
            if (pi == cur) break;
        }
    }
    if (lane < K) {
        c2l[lane] = bad ? lane : col4row;
        shuf[lane] = bad ? lane : row4col;
    }
    if (bad && st && lane == 0) st[0].failed = 1;
}

int check_dims(int64_t n, int64_t d, int64_t k, int64_t r, int64_t ldx) {
    if (n < 1 || d < 1 || k < 1 || r < 1 || ldx < d || n >= INT32_MAX) return GDA_E_SIZE;
    if (d > MAX_DIM || k > MAX_K || r > MAX_RUNS) return GDA_E_UNSUPPORTED;
    return GDA_OK;
}

}  // namespace

extern "C" size_t gda_gmm_mstep_workspace_bytes(int64_t n, int64_t d, int64_t k, int64_t r) {
    if (check_dims(n, d, k, r, d) != GDA_OK) return 0;
    return mstep_plan(n, d, k, r).bytes;
}

extern "C" int gda_gmm_mstep_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, int64_t r,
                                 const float* resp, float reg_covar, float* weights, float* means, float* covariances,
                                 const void* state, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    const int st = check_dims(n, d, k, r, ldx);
    if (st != GDA_OK) return st;
    if (!x || !resp || !weights || !means || !covariances) return GDA_E_NULL;
    const MPlan p = mstep_plan(n, d, k, r);
    if (!workspace || workspace_bytes < p.bytes) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const State* sp = (const State*)state;
    float* sums = (float*)((char*)workspace + p.sum_off);
    float* nk = (float*)((char*)workspace + p.nk_off);
    float* cpart = (float*)((char*)workspace + p.cov_off);
    k_mstep_sums<<<dim3((unsigned)p.slabs, (unsigned)r), TB, 0, s>>>(x, ldx, n, (int)d, (int)k, resp, p.slab_rows, sp, sums);
    GDA_LAUNCH_CHECK();
    k_mstep_means<<<dim3((unsigned)k, (unsigned)r), TB, 0, s>>>((int)d, (int)k, (int)p.slabs, sp, sums, nk, weights, means);
    GDA_LAUNCH_CHECK();
    k_mstep_cov<<<dim3((unsigned)(k * p.ntiles), (unsigned)p.slabs, (unsigned)r), TB, 0, s>>>(
        x, ldx, n, (int)d, (int)k, resp, means, p.slab_rows, (int)p.ntiles, sp, cpart);
    GDA_LAUNCH_CHECK();
    k_mstep_cov_fold<<<(unsigned)gda_cdiv(r * k * p.ntiles * GT * GT, TB), TB, 0, s>>>(
        cpart, (int)p.slabs, (int)p.ntiles, (int)d, (int)k, (int)r, reg_covar, nk, sp, covariances);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_gmm_factor_f32(const float* covariances, int64_t d, int64_t k, int64_t r, float* precisions_chol,
                                  double* log_det, void* state, gda_stream_t stream) {
    const int st = check_dims(1, d, k, r, d);
    if (st != GDA_OK) return st;
    if (!covariances || !precisions_chol || !log_det || !state) return GDA_E_NULL;
    if ((const float*)precisions_chol == covariances) return GDA_E_ALIAS;
    const size_t lds = (size_t)d * (size_t)((int)d | 1) * sizeof(double);
    GDA_LDS_ATTR_ONCE(k_factor, (size_t)MAX_DIM * (MAX_DIM | 1) * sizeof(double));
    k_factor<<<dim3((unsigned)k, (unsigned)r), TB, lds, (hipStream_t)stream>>>(covariances, (int)d, (int)k, (State*)state,
                                                                             precisions_chol, log_det);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_gmm_estep_workspace_bytes(int64_t n, int64_t r) {
    if (n < 1 || r < 1 || r > MAX_RUNS) return 0;
    return gda_align_up((size_t)(r * gda_cdiv(n, ER)) * sizeof(double), 16);
}

extern "C" int gda_gmm_estep_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, int64_t r,
                                 const float* weights, const float* means, const float* precisions_chol,
                                 const double* log_det, float* resp, double tol, void* state, void* workspace,
                                 size_t workspace_bytes, gda_stream_t stream) {
    const int st = check_dims(n, d, k, r, ldx);
    if (st != GDA_OK) return st;
    if (!x || !weights || !means || !precisions_chol || !log_det || !resp) return GDA_E_NULL;
    const size_t need = gda_gmm_estep_workspace_bytes(n, r);
    if (!workspace || workspace_bytes < need) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nblk = gda_cdiv(n, ER);
    k_estep<<<dim3((unsigned)nblk, (unsigned)r), TB, 0, s>>>(x, ldx, n, (int)d, (int)k, weights, means, precisions_chol,
                                                             log_det, resp, (const State*)state, (double*)workspace);
    GDA_LAUNCH_CHECK();
    if (state) {
        k_estep_close<<<(unsigned)r, TB, 0, s>>>((const double*)workspace, (int)nblk, n, tol, (State*)state);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

extern "C" size_t gda_kmeans_step_workspace_bytes(int64_t n, int64_t d, int64_t k) {
    if (check_dims(n, d, k, 1, d) != GDA_OK) return 0;
    return gda_align_up((size_t)(gda_cdiv(n, KR) * k * (d + 1)) * sizeof(float), 16);
}

extern "C" int gda_kmeans_step_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, const float* centers,
                                   int metric, int64_t* labels, float* dist, float* sums, float* counts,
                                   void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    const int st = check_dims(n, d, k, 1, ldx);
    if (st != GDA_OK) return st;
    if (metric < 0 || metric > 2) return GDA_E_UNSUPPORTED;
    if (!x || !centers || !labels || !sums || !counts) return GDA_E_NULL;
    const size_t need = gda_kmeans_step_workspace_bytes(n, d, k);
    if (!workspace || workspace_bytes < need) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nblk = gda_cdiv(n, KR);
    k_kmeans_assign<<<(unsigned)nblk, TB, 0, s>>>(x, ldx, n, (int)d, (int)k, centers, metric, labels, dist,
                                                  (float*)workspace);
    GDA_LAUNCH_CHECK();
    k_kmeans_fold<<<(unsigned)gda_cdiv(k * (d + 1), TB), TB, 0, s>>>((const float*)workspace, nblk, (int)d, (int)k, sums,
                                                                     counts);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_gmm_label_sums_workspace_bytes(int64_t n, int64_t d, int64_t k) {
    return gda_kmeans_step_workspace_bytes(n, d, k);
}

extern "C" int gda_gmm_label_sums_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, const int64_t* labels,
                                      float* sums, float* counts, void* workspace, size_t workspace_bytes,
                                      gda_stream_t stream) {
    const int st = check_dims(n, d, k, 1, ldx);
    if (st != GDA_OK) return st;
    if (!x || !labels || !sums || !counts) return GDA_E_NULL;
    const size_t need = gda_gmm_label_sums_workspace_bytes(n, d, k);
    if (!workspace || workspace_bytes < need) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int64_t nblk = gda_cdiv(n, KR);
    k_label_part<<<(unsigned)nblk, TB, 0, s>>>(x, ldx, n, (int)d, (int)k, labels, (float*)workspace);
    GDA_LAUNCH_CHECK();
    k_kmeans_fold<<<(unsigned)gda_cdiv(k * (d + 1), TB), TB, 0, s>>>((const float*)workspace, nblk, (int)d, (int)k, sums,
                                                                     counts);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_gmm_relabel_f32(const float* resp, int64_t n, int64_t k, const int32_t* cluster2label,
                                   const int32_t* shuffle_idx, const int64_t* fallback, const void* state, float* prob,
                                   int64_t* labels, float* onehot, gda_stream_t stream) {
    const int st = check_dims(n, 1, k, 1, 1);
    if (st != GDA_OK) return st;
    if (!resp || !labels || (cluster2label == nullptr) != (shuffle_idx == nullptr)) return GDA_E_NULL;
    if (prob == resp) return GDA_E_ALIAS;
    k_relabel<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(resp, n, (int)k, cluster2label, shuffle_idx,
                                                                         fallback, (const State*)state, prob, labels,
                                                                         onehot);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_lsa_cos_f32(const float* tgt_centers, const float* src_centers, int64_t k, int64_t d,
                               int32_t* cluster2label, int32_t* shuffle_idx, void* state, gda_stream_t stream) {
    const int st = check_dims(1, d, k, 1, d);
    if (st != GDA_OK) return st;
    if (!tgt_centers || !src_centers || !cluster2label || !shuffle_idx) return GDA_E_NULL;
    k_lsa<<<1, 64, 0, (hipStream_t)stream>>>(tgt_centers, src_centers, nullptr, (int)k, (int)d, cluster2label, shuffle_idx,
                                             (State*)state);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_lsa_cost_f64(const double* cost, int64_t k, int32_t* cluster2label, int32_t* shuffle_idx, void* state,
                                gda_stream_t stream) {
    const int st = check_dims(1, 1, k, 1, 1);
    if (st != GDA_OK) return st;
    if (!cost || !cluster2label || !shuffle_idx) return GDA_E_NULL;
    k_lsa<<<1, 64, 0, (hipStream_t)stream>>>(nullptr, nullptr, cost, (int)k, 1, cluster2label, shuffle_idx, (State*)state);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
