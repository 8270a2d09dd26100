// PairAlign (pygda/models/pa.py): the statistics of its two re-weighting fits, its class-weighted loss and the
// refresh of the re-weighted CSR values.  Contracts in include/gda_hip.h.
//
// (a) k_pa_edge: S[a][p][b][q] = sum over edges (i, j), cls_i = a, cls_j = b, of z_i[p] z_j[q].  The reference fills
//     [E, C, C] and [E, C^2] host arrays (pa.py:566-590, :776-795); here a workgroup takes row SEGMENTS of one class a
//     (a segment: at most GDA_PA_SEGMENT neighbours of one row, so a hub row is many segments spread over workgroups),
//     eight at a time: a group of 32 lanes walks a segment's neighbours in CSR order and adds z_j[q] into T[b][q]
//     (lane q owns column q: no two lanes meet), then every thread adds z_i[p] T[b][q] of the eight segments, in
//     segment order, into the accumulator entries it owns.  Accumulator [C][K][C] and the eight T [K][C] in float64
//     in LDS: 8 C^2 K + 64 C K + 32 C bytes, 144.75 KiB at C = K = 24 (GDA_PA_MAX_CLASSES; C = 25 would need 161.9) of
//     the 160 KiB of a CU, 88.1 KiB at 20, 1.8 KiB at the citation graphs' 5.  One partial per
//     workgroup, folded per class in item order by k_pa_fold: no floating-point atomics, bit-identical call to call.
// (b) k_pa_soft: P[a][p] = sum of softmax(z_i)[p] over the rows of class a, both domains in one launch; a thread owns
//     rows, per-thread float64 sums, an xor butterfly per wavefront, the wavefronts in order, k_pa_fold.
// (c) k_pa_ce_*: (1/n) sum over the selected rows of coef[y_i] ce_i with coef read from the device.
// (d) k_pa_refresh: val[e] = base[e] ((1 - lmda) + lmda rw[cls_row][cls_col]), the row by bisection of rowptr.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int MAXC = GDA_PA_MAX_CLASSES;
constexpr int GROUP = 32;              // lanes per segment in (a): one per class column, MAXC <= GROUP
constexpr int ROWS = TB / GROUP;       // segments per tile
constexpr int CE_BLOCKS = 256;
static_assert(MAXC <= GROUP, "a lane per class column");

__host__ __device__ inline size_t pa_edge_lds(int64_t C, int64_t K) {
    return (size_t)(C * K * C + ROWS * K * C) * sizeof(double) + (size_t)ROWS * C * sizeof(float);
}

__global__ void __launch_bounds__(TB)
k_pa_edge(const int32_t* __restrict__ colidx, const float* __restrict__ z, const int64_t* __restrict__ cls, int64_t N, int C,
          int K, const int32_t* __restrict__ seg, const int32_t* __restrict__ items, double* __restrict__ partial) {
    extern __shared__ double pa_smem[];
    const int KC = K * C, CKC = C * KC, t = threadIdx.x;
    double* acc = pa_smem;
    double* T = acc + CKC;
    float* zi = reinterpret_cast<float*>(T + ROWS * KC);
    const int lo = items[3 * blockIdx.x + 1], hi = items[3 * blockIdx.x + 2];
    for (int e = t; e < CKC; e += TB) acc[e] = 0.0;
    const int r = t / GROUP, q = t % GROUP;
    for (int s0 = lo; s0 < hi; s0 += ROWS) {
        const int nr = min(ROWS, hi - s0);
        for (int e = t; e < ROWS * KC; e += TB) T[e] = 0.0;
        __syncthreads();
        if (r < nr && q < C) {
            const int32_t* sg = seg + 3 * (int64_t)(s0 + r);
            const int64_t row = sg[0];
            zi[r * C + q] = (row >= 0 && row < N) ? z[row * C + q] : 0.f;
            double* Tr = T + r * KC + q;
            for (int e = sg[1]; e < sg[2]; ++e) {
                const int64_t j = colidx[e];
                if (j < 0 || j >= N) continue;
                const int64_t b = cls ? cls[j] : 0;
                if (b < 0 || b >= K) continue;
                Tr[b * C] += (double)z[j * C + q];
            }
        }
        __syncthreads();
        for (int e = t; e < CKC; e += TB) {
            const int p = e / KC, bq = e - p * KC;
            double s = acc[e];
            for (int k = 0; k < nr; ++k) s += (double)zi[k * C + p] * T[k * KC + bq];
            acc[e] = s;
        }
        __syncthreads();
    }
    double* out = partial + (size_t)blockIdx.x * CKC;
    for (int e = t; e < CKC; e += TB) out[e] = acc[e];
}

// out[slot][e] = the partials of the slot's items, in item order (a slot without items: 0)
__global__ void __launch_bounds__(TB)
k_pa_fold(const double* __restrict__ partial, const int32_t* __restrict__ slot_ptr, int64_t slots, int64_t width,
          double* __restrict__ out) {
    for (int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x; idx < slots * width; idx += (int64_t)gridDim.x * TB) {
        const int64_t slot = idx / width, e = idx - slot * width;
        double s = 0.0;
        for (int it = slot_ptr[slot]; it < slot_ptr[slot + 1]; ++it) s += partial[(size_t)it * width + e];
        out[idx] = s;
    }
}

__global__ void __launch_bounds__(TB)
k_pa_soft(const float* __restrict__ z0, const float* __restrict__ z1, const int32_t* __restrict__ order0,
          const int32_t* __restrict__ order1, int64_t n0, int64_t n1, int C, const int32_t* __restrict__ items,
          double* __restrict__ partial) {
    __shared__ double red[TB / GDA_WAVE][MAXC];
    const int32_t* it = items + 4 * (int64_t)blockIdx.x;
    const int dom = it[0];
    const float* z = dom ? z1 : z0;
    const int32_t* order = dom ? order1 : order0;
    const int64_t n = dom ? n1 : n0;
    double acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.0;
    for (int k = it[2] + (int)threadIdx.x; k < it[3]; k += TB) {
        const int64_t i = order ? order[k] : k;
        if (i < 0 || i >= n) continue;
        const float* x = z + i * C;
        float v[MAXC], mx = -INFINITY, s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) if (c < C) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) if (c < C) { v[c] = expf(v[c] - mx); s += v[c]; }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) if (c < C) acc[c] += (double)(v[c] / s);
    }
    const int w = threadIdx.x / GDA_WAVE;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        if (c < C) {
            const double a = wave_sum(acc[c]);
            if (threadIdx.x % GDA_WAVE == 0) red[w][c] = a;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        double s = 0.0;
        for (int k = 0; k < TB / GDA_WAVE; ++k) s += red[k][threadIdx.x];
        partial[(size_t)blockIdx.x * C + threadIdx.x] = s;
    }
}

__device__ __forceinline__ float pa_row_lse(const float* __restrict__ x, int C, float (&v)[MAXC]) {
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) if (c < C) { v[c] = x[c]; mx = fmaxf(mx, v[c]); }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) if (c < C) s += expf(v[c] - mx);
    return mx + logf(s);
}

// first index attaining the row maximum, NaN counting as the largest value (torch.argmax)
__device__ __forceinline__ int pa_row_argmax(const float (&v)[MAXC], int C) {
    float best = v[0];
    int bi = 0;
#pragma unroll
    for (int c = 1; c < MAXC; ++c)
        if (c < C && (v[c] > best || (v[c] != v[c] && best == best))) { best = v[c]; bi = c; }
    return bi;
}

// partial[b] = weighted loss sum of block b over the selection, partial[CE_BLOCKS + b] = its rows (ALL rows) whose argmax
// is the label
__global__ void __launch_bounds__(TB)
k_pa_ce_fwd(const float* __restrict__ x, const int64_t* __restrict__ y, int64_t N, int C, const int64_t* __restrict__ sel,
            int64_t n_sel, const float* __restrict__ coef, double* __restrict__ partial) {
    __shared__ double sh[TB];
    double acc = 0.0, hit = 0.0;
    float v[MAXC];
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < N; i += (int64_t)gridDim.x * TB) {
        const float lse = pa_row_lse(x + i * C, C, v);
        const int64_t yi = y[i];
        hit += pa_row_argmax(v, C) == (int)yi ? 1.0 : 0.0;
        if (!sel && yi >= 0 && yi < C) acc += (double)(coef[yi] * (lse - x[i * C + yi]));
    }
    if (sel)
        for (int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x; k < n_sel; k += (int64_t)gridDim.x * TB) {
            const int64_t i = sel[k];
            if (i < 0 || i >= N) continue;
            const int64_t yi = y[i];
            if (yi < 0 || yi >= C) continue;
            const float lse = pa_row_lse(x + i * C, C, v);
            acc += (double)(coef[yi] * (lse - x[i * C + yi]));
        }
    const double a = block_sum_d(acc, sh);
    const double h = block_sum_d(hit, sh);
    if (threadIdx.x == 0) { partial[blockIdx.x] = a; partial[CE_BLOCKS + blockIdx.x] = h; }
}

__global__ void __launch_bounds__(TB)
k_pa_ce_final(const double* __restrict__ partial, int n, int64_t rows, float* __restrict__ loss, double* __restrict__ stats) {
    __shared__ double sh[TB];
    double a = 0.0, h = 0.0;
    for (int k = threadIdx.x; k < n; k += TB) { a += partial[k]; h += partial[CE_BLOCKS + k]; }
    a = block_sum_d(a, sh);
    h = block_sum_d(h, sh);
    if (threadIdx.x == 0) {
        *loss = (float)(a / (double)rows);
        if (stats) { stats[0] = (double)*loss; stats[1] = h; }
    }
}

__global__ void __launch_bounds__(TB)
k_pa_ce_bwd(const float* __restrict__ x, const int64_t* __restrict__ y, int64_t N, int C, const int64_t* __restrict__ sel,
            int64_t n_sel, const float* __restrict__ coef, const float* __restrict__ grad_loss, float* __restrict__ gx) {
    const int64_t rows = sel ? n_sel : N;
    const float scale = *grad_loss / (float)rows;
    float v[MAXC];
    for (int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x; k < rows; k += (int64_t)gridDim.x * TB) {
        const int64_t i = sel ? sel[k] : k;
        if (i < 0 || i >= N) continue;
        const int64_t yi = y[i];
        const bool ok = yi >= 0 && yi < C;
        const float lse = pa_row_lse(x + i * C, C, v);
        const float w = ok ? coef[yi] * scale : 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
            if (c < C) gx[i * C + c] = (expf(v[c] - lse) - (c == yi ? 1.f : 0.f)) * w;
    }
}

__global__ void __launch_bounds__(TB)
k_pa_refresh(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ base,
             float* __restrict__ val, int64_t N, const int64_t* __restrict__ cls, const float* __restrict__ rw, int C,
             float keep, float lmda, int swap) {
    const int64_t nnz = rowptr[N];
    for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * TB) {
        int64_t lo = 0, hi = N;                       // the row r with rowptr[r] <= e < rowptr[r + 1]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) / 2;
            if (rowptr[mid] <= e) lo = mid; else hi = mid;
        }
        const int64_t j = colidx[e];
        if (j < 0 || j >= N) continue;
        int64_t a = cls[lo], b = cls[j];
        if (a < 0 || a >= C || b < 0 || b >= C) continue;
        if (swap) { const int64_t s = a; a = b; b = s; }
        val[e] = base[e] * (keep + lmda * rw[a * C + b]);
    }
}

}  // namespace

extern "C" size_t gda_pa_edge_stats_workspace_bytes(int64_t n_items, int64_t C, int64_t K) {
    if (n_items < 0 || C < 1 || K < 1) return 0;
    return gda_align_up((size_t)(n_items > 0 ? n_items : 1) * C * K * C * sizeof(double), 256);
}

extern "C" int gda_pa_edge_stats_f64(const int32_t* colidx, const float* z, const int64_t* cls, int64_t N, int64_t C, int64_t K,
                                     const int32_t* seg, int64_t n_seg, const int32_t* items, int64_t n_items,
                                     const int32_t* slot_ptr, double* out, void* workspace, size_t workspace_bytes,
                                     gda_stream_t stream_) {
    if (N < 0 || C < 1 || K < 1 || n_seg < 0 || n_items < 0 || n_items > GDA_PA_MAX_ITEMS) return GDA_E_SIZE;
    if (C > MAXC || K > MAXC) return GDA_E_UNSUPPORTED;
    if (!slot_ptr || !out || !workspace || (n_items > 0 && (!colidx || !z || !seg || !items))) return GDA_E_NULL;
    if (K > 1 && !cls) return GDA_E_NULL;
    if (workspace_bytes < gda_pa_edge_stats_workspace_bytes(n_items, C, K)) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t width = C * K * C;
    if (n_items > 0) {
        GDA_LDS_ATTR_ONCE(k_pa_edge, pa_edge_lds(MAXC, MAXC));
        k_pa_edge<<<(unsigned)n_items, TB, pa_edge_lds(C, K), stream>>>(colidx, z, cls, N, (int)C, (int)K, seg, items,
                                                                       (double*)workspace);
        GDA_LAUNCH_CHECK();
    }
    k_pa_fold<<<(unsigned)gda_cdiv(K * width, TB), TB, 0, stream>>>((const double*)workspace, slot_ptr, K, width, out);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_pa_softmax_sums_workspace_bytes(int64_t n_items, int64_t C) {
    if (n_items < 0 || C < 1) return 0;
    return gda_align_up((size_t)(n_items > 0 ? n_items : 1) * C * sizeof(double), 256);
}

extern "C" int gda_pa_softmax_sums_f64(const float* z0, const float* z1, const int32_t* order0, const int32_t* order1,
                                       int64_t n0, int64_t n1, int64_t C, const int32_t* items, int64_t n_items,
                                       const int32_t* slot_ptr, int64_t slots, double* out, void* workspace,
                                       size_t workspace_bytes, gda_stream_t stream_) {
    if (n0 < 0 || n1 < 0 || C < 1 || n_items < 0 || n_items > GDA_PA_MAX_ITEMS || slots < 1) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (!slot_ptr || !out || !workspace || (n_items > 0 && !items) || (n0 > 0 && !z0) || (n1 > 0 && !z1)) return GDA_E_NULL;
    if (workspace_bytes < gda_pa_softmax_sums_workspace_bytes(n_items, C)) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_items > 0) {
        k_pa_soft<<<(unsigned)n_items, TB, 0, stream>>>(z0, z1, order0, order1, n0, n1, (int)C, items, (double*)workspace);
        GDA_LAUNCH_CHECK();
    }
    k_pa_fold<<<(unsigned)gda_cdiv(slots * C, TB), TB, 0, stream>>>((const double*)workspace, slot_ptr, slots, C, out);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_pa_ce_workspace_bytes(void) { return 2 * CE_BLOCKS * sizeof(double); }

extern "C" int gda_pa_ce_fwd_f32(const float* logits, const int64_t* labels, int64_t N, int64_t C, const int64_t* sel,
                                 int64_t n_sel, const float* coef, float* loss, double* stats, void* workspace,
                                 size_t workspace_bytes, gda_stream_t stream_) {
    if (N < 1 || C < 1 || n_sel < 0 || (sel && n_sel < 1)) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (!logits || !labels || !coef || !loss || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_pa_ce_workspace_bytes()) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int blocks = (int)(gda_cdiv(N, TB) < CE_BLOCKS ? gda_cdiv(N, TB) : CE_BLOCKS);
    k_pa_ce_fwd<<<blocks, TB, 0, stream>>>(logits, labels, N, (int)C, sel, n_sel, coef, (double*)workspace);
    GDA_LAUNCH_CHECK();
    k_pa_ce_final<<<1, TB, 0, stream>>>((const double*)workspace, blocks, sel ? n_sel : N, loss, stats);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_pa_ce_bwd_f32(const float* logits, const int64_t* labels, int64_t N, int64_t C, const int64_t* sel,
                                 int64_t n_sel, const float* coef, const float* grad_loss, float* grad_logits,
                                 gda_stream_t stream_) {
    if (N < 1 || C < 1 || n_sel < 0 || (sel && n_sel < 1)) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (!logits || !labels || !coef || !grad_loss || !grad_logits) return GDA_E_NULL;
    if (grad_logits == logits) return GDA_E_ALIAS;
    hipStream_t stream = (hipStream_t)stream_;
    if (sel) GDA_HIP_TRY(hipMemsetAsync(grad_logits, 0, (size_t)N * C * sizeof(float), stream));
    const int64_t rows = sel ? n_sel : N;
    const int64_t blocks = gda_cdiv(rows, TB) < 4096 ? gda_cdiv(rows, TB) : 4096;
    k_pa_ce_bwd<<<(unsigned)blocks, TB, 0, stream>>>(logits, labels, N, (int)C, sel, n_sel, coef, grad_loss, grad_logits);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_pa_refresh_values_f32(const int32_t* rowptr, const int32_t* colidx, const float* base, float* val,
                                         int64_t N, int64_t nnz_cap, const int64_t* cls, const float* rw, int64_t C,
                                         float keep, float lmda, int swap, gda_stream_t stream_) {
    if (N < 0 || nnz_cap < 0 || C < 1) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (N == 0 || nnz_cap == 0) return GDA_OK;
    if (!rowptr || !colidx || !base || !val || !cls || !rw) return GDA_E_NULL;
    const int64_t blocks = gda_cdiv(nnz_cap, TB) < 4096 ? gda_cdiv(nnz_cap, TB) : 4096;
    k_pa_refresh<<<(unsigned)blocks, TB, 0, (hipStream_t)stream_>>>(rowptr, colidx, base, val, N, cls, rw, (int)C, keep, lmda,
                                                                   swap);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
