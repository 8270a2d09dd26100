// JHGDA for gfx950 (pygda/models/jhgda.py, pygda/nn/jhgda_base.py): the pooled proximity loss and the pooling rows.
//
// Proximity (jhgda_base.py:337-377): P = S S^T (S [N, K] the soft assignment), Pc = min(P, 1),
//   loss = 1 / N^2 sum_ij ( -a_ij log(Pc + eps) - (1 - a_ij) log(1 - Pc + eps) ),  eps = 1e-7,
// where a_ij is the dense pooled adjacency (levels >= 1) or the number of times (i, j) occurs in the edge list
// (level 0: -(sum_e log(P_e) + sum_all log(1 - P) - sum_e log(1 - P_e)) / N^2 is exactly this with a = the counts).
// The gradient: dL/dS = (G + G^T) S with G_ij = m_ij / N^2 (-a_ij / (Pc + eps) + (1 - a_ij) / (1 - Pc + eps)) and
// m_ij = 1 where P < 1, 1/2 where P == 1, 0 above (torch's rule for min against a tensor).  P is symmetric, so
// (G + G^T)_ij = H_ij needs only P_ij, a_ij and a_ji.  Dense A also gets dA_ij = (log(1 - Pc + eps) - log(Pc + eps)) / N^2.
//   k_prox_tile   a block = one 64 x 64 tile of P on v_mfma_f32_32x32x2_f32 (exact fp32 operands, the k-ordered fma
//                 chain of gda_gemm.hip's tiles; K streamed in 32-deep chunks through 17 KB of LDS with the next chunk
//                 held in registers), then in registers: the loss terms (one partial per block), H (into the row strip
//                 of the workspace) and dA.  Edge counts come from binary searches in the edge CSR and its transpose
//                 (columns sorted inside a row, duplicates kept).
//   dS            rows are done in batches of B = round_up(K, 64) (at most N): H's [B, N] strip is the workspace and
//                 dS[batch] = H_strip S runs on the project's own GEMM (gda_gemm_ex_f32, NN).  The workspace is
//                 B N floats + the partials (< N + N / B): O(N K), never N x N.  Every P entry is formed once per ordered
//                 pair (2 N^2 K flops) and H S costs another 2 N^2 K: 4 N^2 K in all.  Visiting only the upper
//                 triangle would save a quarter of that but needs either float atomics or [N/64, N, K] partials to
//                 sum G^T S_i into other rows' dS; neither is taken.
//   k_fold_scalar gda_reduce.h's, one block per row batch: the batch's tile partials in index order (double) into one
//                 float; then one block over the batch sums, times 1 / N^2.  Partials: (B / 64) ceil(N / 64) +
//                 ceil(N / B) floats.
// dS = NULL computes the loss (and dA) alone: no strip, no GEMM -- S takes no gradient (the one-hot assignments of
// sparse=True).
// Pooling rows (GCNPooling.forward, jhgda_base.py:87, and JHGDABase.entropy): S = softmax(relu(X)) row by row, the row
// entropies -sum S log(S + eps) folded into mean_i; the backward takes the upstream dS and the entropy's scalar
// gradient and writes dX = [X > 0] S (g - <S, g>) with g = dS + gce / N (-log(S + eps) - S / (S + eps)).
//   k_pool_rows_fwd / k_pool_rows_bwd   one wave per row, the row's columns strided over the lanes, butterfly sums.
// Fixed-order reductions everywhere: two runs are bit-identical.  No atomics.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int TILE = 64;
constexpr int DK = 32;
constexpr int LDT = TILE + 4;
constexpr float PEPS = 1e-7f;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// 64 rows x 32 columns (k0 ..) of S into regs: thread t holds row t / 4, columns (t % 4) * 8 .. + 7
__device__ __forceinline__ void prox_load(float (&v)[8], const float* __restrict__ S, int64_t lds, int64_t r0,
                                          int64_t k0, int64_t n, int64_t k, bool vec) {
    const int t = threadIdx.x;
    const int64_t r = r0 + t / 4, c = k0 + (t % 4) * 8;
    if (r >= n) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = 0.f;
        return;
    }
    const float* p = S + r * lds + c;
    if (vec && c + 8 <= k) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        return;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = c + q < k ? p[q] : 0.f;
}

__device__ __forceinline__ void prox_store(float (&T)[DK][LDT], const float (&v)[8]) {
    const int t = threadIdx.x;
    const int r = t / 4, kq = (t % 4) * 8;
#pragma unroll
    for (int q = 0; q < 8; ++q) T[kq + q][r] = v[q];
}

// number of entries equal to j in col[beg, end) (sorted ascending)
__device__ __forceinline__ float csr_count(const int32_t* __restrict__ col, int32_t beg, int32_t end, int32_t j) {
    int32_t lo = beg, hi = end;
    while (lo < hi) {
        const int32_t m = (lo + hi) >> 1;
        if (col[m] < j) lo = m + 1; else hi = m;
    }
    int32_t e = lo;
    while (e < end && col[e] == j) ++e;
    return (float)(e - lo);
}

__device__ __forceinline__ float prox_g(float a, float lp_inv, float ln_inv) { return -a * lp_inv + (1.f - a) * ln_inv; }

// one 64 x 64 tile of P: rows row0 + blockIdx.x * 64 .., columns blockIdx.y * 64 ..; rows are global indices, the strip
// row is (i - row0).  rows_end bounds the batch.
__global__ void __launch_bounds__(TB)
k_prox_tile(const float* __restrict__ S, int64_t lds, int n, int k, int row0, int rows_end, bool vec,
            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ t_rowptr,
            const int32_t* __restrict__ t_col, const float* __restrict__ A, int64_t lda, float inv_n2,
            float* __restrict__ strip, float* __restrict__ dA, int64_t ldda, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[DK][LDT];
    __shared__ __attribute__((aligned(16))) float Bs[DK][LDT];
    __shared__ float red[TB];
    const int i0 = row0 + blockIdx.x * TILE, j0 = blockIdx.y * TILE;
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int ka = lane >> 5, la = lane & 31;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float va[8], vb[8];
    prox_load(va, S, lds, i0, 0, rows_end, k, vec);
    prox_load(vb, S, lds, j0, 0, n, k, vec);
    for (int k0 = 0; k0 < k; k0 += DK) {
        __syncthreads();
        prox_store(As, va);
        prox_store(Bs, vb);
        __syncthreads();
        if (k0 + DK < k) {                                       // the next chunk's loads in flight under the MFMAs
            prox_load(va, S, lds, i0, k0 + DK, rows_end, k, vec);
            prox_load(vb, S, lds, j0, k0 + DK, n, k, vec);
        }
#pragma unroll
        for (int kk = 0; kk < DK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + ka][wi + la], Bs[kk + ka][wj + la], acc, 0, 0, 0);
    }
    const int j = j0 + wj + la;
    float lsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + wi + (r & 3) + 8 * (r >> 2) + 4 * ka;   // C/D layout of the 32x32 MFMA
        if (i < rows_end && j < n) {
            const float p = acc[r];
            const float pc = fminf(p, 1.f);
            float aij, aji;
            if (A != nullptr) {
                aij = A[(int64_t)i * lda + j];
                aji = A[(int64_t)j * lda + i];
            } else {
                aij = csr_count(col, rowptr[i], rowptr[i + 1], j);
                aji = csr_count(t_col, t_rowptr[i], t_rowptr[i + 1], j);   // edges j -> i
            }
            const float lp = logf(pc + PEPS), ln = logf(1.f - pc + PEPS);
            lsum += -aij * lp - (1.f - aij) * ln;
            if (strip != nullptr) {                              // NULL: the loss alone (S takes no gradient)
                const float m = p < 1.f ? 1.f : (p == 1.f ? 0.5f : 0.f);
                const float lpi = 1.f / (pc + PEPS), lni = 1.f / (1.f - pc + PEPS);
                strip[(int64_t)(i - row0) * n + j] = inv_n2 * m * (prox_g(aij, lpi, lni) + prox_g(aji, lpi, lni));
            }
            if (dA != nullptr) dA[(int64_t)i * ldda + j] = inv_n2 * (ln - lp);
        }
    }
    const float bs = block_sum_f(lsum, red);
    if (tid == 0) part[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = bs;          // the batch's tiles, row-major
}

// S = softmax(relu(X)) per row (one wave per row); ent[row] = -sum S log(S + eps)
__global__ void __launch_bounds__(TB)
k_pool_rows_fwd(const float* __restrict__ X, int64_t ldx, int n, int k, float* __restrict__ S, int64_t lds,
                float* __restrict__ ent) {
    const int row = blockIdx.x * (TB / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (row >= n) return;
    const float* x = X + (int64_t)row * ldx;
    float* s = S + (int64_t)row * lds;
    float mx = 0.f;                                              // relu(x) >= 0 and every row has k >= 1 entries
    for (int c = lane; c < k; c += 64) mx = fmaxf(mx, fmaxf(x[c], 0.f));
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < k; c += 64) sum += expf(fmaxf(x[c], 0.f) - mx);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    float e = 0.f;
    for (int c = lane; c < k; c += 64) {
        const float v = expf(fmaxf(x[c], 0.f) - mx) * inv;
        s[c] = v;
        e -= v * logf(v + PEPS);
    }
    e = wave_sum(e);
    if (lane == 0) ent[row] = e;
}

// dX = [X > 0] S (g - <S, g>),  g = dS + went (-log(S + eps) - S / (S + eps)),  went = gce[0] / n
__global__ void __launch_bounds__(TB)
k_pool_rows_bwd(const float* __restrict__ X, int64_t ldx, const float* __restrict__ S, int64_t lds,
                const float* __restrict__ dS, int64_t ldg, const float* __restrict__ gce, int n, int k,
                float* __restrict__ dX, int64_t lddx) {
    const int row = blockIdx.x * (TB / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (row >= n) return;
    const float went = gce != nullptr ? gce[0] / (float)n : 0.f;
    const float* x = X + (int64_t)row * ldx;
    const float* s = S + (int64_t)row * lds;
    const float* gs = dS != nullptr ? dS + (int64_t)row * ldg : nullptr;
    float dot = 0.f;
    for (int c = lane; c < k; c += 64) {
        const float v = s[c];
        const float g = (gs != nullptr ? gs[c] : 0.f) + went * (-logf(v + PEPS) - v / (v + PEPS));
        dot += v * g;
    }
    dot = wave_sum(dot);
    float* dx = dX + (int64_t)row * lddx;
    for (int c = lane; c < k; c += 64) {
        const float v = s[c];
        const float g = (gs != nullptr ? gs[c] : 0.f) + went * (-logf(v + PEPS) - v / (v + PEPS));
        dx[c] = x[c] > 0.f ? v * (g - dot) : 0.f;
    }
}

int64_t prox_batch(int64_t n, int64_t k) {
    const int64_t nr = gda_cdiv(n, TILE) * TILE;
    const int64_t b = gda_cdiv(k, TILE) * TILE;
    return b < nr ? b : nr;
}

}  // namespace

extern "C" size_t gda_jhgda_prox_workspace_bytes(int64_t n, int64_t k) {
    if (n < 1 || k < 1) return 256;
    const int64_t b = prox_batch(n, k);
    const int64_t nparts = (b / TILE) * gda_cdiv(n, TILE) + gda_cdiv(n, b);     // one batch's tiles + one per batch
    const int64_t last = n - (gda_cdiv(n, b) - 1) * b;
    size_t g = gda_gemm_workspace_bytes(GDA_GEMM_NN, b < n ? b : n, k, n);
    const size_t g2 = gda_gemm_workspace_bytes(GDA_GEMM_NN, last, k, n);
    if (g2 > g) g = g2;
    return gda_align_up((size_t)(b * n + nparts) * sizeof(float), 256) + g;
}

extern "C" int gda_jhgda_prox_f32(const float* S, int64_t lds, int64_t n, int64_t k, const int32_t* rowptr,
                                  const int32_t* col, const int32_t* t_rowptr, const int32_t* t_col, const float* A,
                                  int64_t lda, float* loss, float* dS, int64_t ldds, float* dA, int64_t ldda,
                                  void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || k < 1 || lds < k || ldds < k) return GDA_E_SIZE;
    if (n > GDA_JHGDA_PROX_MAX_N || k > GDA_JHGDA_PROX_MAX_K) return GDA_E_UNSUPPORTED;
    if (!S || !loss || !workspace) return GDA_E_NULL;
    const bool dense = A != nullptr;
    if (!dense && (!rowptr || !col || !t_rowptr || !t_col)) return GDA_E_NULL;
    if (dense && (lda < n || (dA != nullptr && ldda < n))) return GDA_E_SIZE;
    if (!dense && dA != nullptr) return GDA_E_SIZE;
    if (workspace_bytes < gda_jhgda_prox_workspace_bytes(n, k)) return GDA_E_WORKSPACE;
    if (dS == S || (dense && dA == A)) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    const int64_t b = prox_batch(n, k);
    const int64_t ntj = gda_cdiv(n, TILE);
    const int64_t nb = gda_cdiv(n, b);
    const int64_t nparts = (b / TILE) * ntj + nb;
    float* strip = static_cast<float*>(workspace);
    float* part = strip + b * n;
    float* bsum = part + (b / TILE) * ntj;
    char* gws = static_cast<char*>(workspace) + gda_align_up((size_t)(b * n + nparts) * sizeof(float), 256);
    const size_t gws_bytes = workspace_bytes - gda_align_up((size_t)(b * n + nparts) * sizeof(float), 256);
    const bool vec = k % 4 == 0 && lds % 4 == 0 && ((uintptr_t)S % 16) == 0;
    const float inv_n2 = (float)(1.0 / ((double)n * (double)n));
    for (int64_t r0 = 0, bi = 0; r0 < n; r0 += b, ++bi) {
        const int64_t rows = n - r0 < b ? n - r0 : b;
        const dim3 grid((unsigned)gda_cdiv(rows, TILE), (unsigned)ntj);
        k_prox_tile<<<grid, TB, 0, s>>>(S, lds, (int)n, (int)k, (int)r0, (int)(r0 + rows), vec, rowptr, col, t_rowptr,
                                        t_col, A, lda, inv_n2, dS != nullptr ? strip : nullptr, dA, ldda, part);
        GDA_LAUNCH_CHECK();
        k_fold_scalar<TB><<<1, TB, 0, s>>>(part, (int)(grid.x * grid.y), 1.0, bsum + bi);   // the batch's tiles in order
        GDA_LAUNCH_CHECK();
        if (dS != nullptr) {
            const int rc = gda_gemm_ex_f32(GDA_GEMM_NN, rows, k, n, strip, n, S, lds, dS + r0 * ldds, ldds, nullptr,
                                           nullptr, gws, gws_bytes, stream);
            if (rc != GDA_OK) return rc;
        }
    }
    k_fold_scalar<TB><<<1, TB, 0, s>>>(bsum, (int)nb, (double)inv_n2, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_jhgda_pool_rows_fwd_f32(const float* X, int64_t ldx, int64_t n, int64_t k, float* S, int64_t lds,
                                           float* ent, float* ce, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || k < 1 || ldx < k || lds < k) return GDA_E_SIZE;
    if (!X || !S || !ent || !ce) return GDA_E_NULL;
    if (S == X) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    k_pool_rows_fwd<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, s>>>(X, ldx, (int)n, (int)k, S, lds, ent);
    GDA_LAUNCH_CHECK();
    k_fold_scalar<TB><<<1, TB, 0, s>>>(ent, (int)n, 1.0 / (double)n, ce);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_jhgda_pool_rows_bwd_f32(const float* X, int64_t ldx, const float* S, int64_t lds, const float* dS,
                                           int64_t ldg, const float* gce, int64_t n, int64_t k, float* dX,
                                           int64_t lddx, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || k < 1 || ldx < k || lds < k || lddx < k || (dS != nullptr && ldg < k))
        return GDA_E_SIZE;
    if (!X || !S || !dX) return GDA_E_NULL;
    k_pool_rows_bwd<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, (hipStream_t)stream>>>(X, ldx, S, lds, dS, ldg, gce,
                                                                                     (int)n, (int)k, dX, lddx);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
