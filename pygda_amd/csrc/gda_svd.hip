// The device side of svd_transform (pygda/utils/svd_transform.py:8-75): a randomized range finder on the combinatorial
// Laplacian L = D - A that never forms the dense [N, N] matrix.  Everything of extent N is one of
//
//   gda_svd_lap_apply_f32    Y = L X  (or L^T X on the transposed CSR): y[i] = diag[i] x[i] - sum_{j in row i} x[j].  The
//                            off-diagonal values are all -1, so NO value array is read.  A lane group owns a row and
//                            CPL columns per lane; the neighbour list is walked once per 64 CPL columns, in CSR order.
//                            Rows beyond the split threshold are cut into chunks of `threshold` entries (the layout of
//                            gda_row_split_build); their partials are added in chunk order by k_lap_long: the sums do
//                            not depend on scheduling.
//   gda_svd_lap_moments_f32  the same walk, nothing stored: per-column sum and sum of squares of L X in float64
//                            (explained_variance_ of the reference without writing the last [N, k] product).  Every lane
//                            group keeps its columns' two sums in registers over a fixed, strided set of rows; the
//                            per-group partials are folded in a fixed order (gda_reduce.h).
//   gda_svd_gram_f32         G = Y^T Y on v_mfma_f32_32x32x2_f32 (exact fp32 fma chains): 64 x 64 tiles on and below the
//                            diagonal only, the reduction over N split into row slabs whose partial tiles are added in
//                            slab order and mirrored, so G == G^T bit for bit and two runs agree bit for bit.
//
// and a tall-times-small product, which is gda_gemm_ex_f32 (NN).  No float atomics anywhere.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int LAP_MOMENT_BLOCKS = 512;     // row blocks of the moments walk: bounds the partials, not the rows
constexpr int LAP_LONG_BLOCKS = 64;
constexpr int MAX_WIDTH = 4096;            // GDA_SVD_MAX_WIDTH

struct Split {
    int32_t threshold, n_long, n_chunks;
    const int32_t* long_rows;
    const int32_t* long_chunk_ptr;
    const int32_t* chunk_long;
};

// ---- the operator ----------------------------------------------------------------------------------------------------
// item < n: row `item` (skipped when the split owns it); item >= n: chunk `item - n` of a long row -> chunk_part.
template <int G, int CPL, bool MOMENTS>
__global__ void __launch_bounds__(TB)
k_lap_rows(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ diag,
           int64_t n, int w, const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, Split sp,
           float* __restrict__ chunk_part, double* __restrict__ part) {
    constexpr int GPB = TB / G;
    const int gl = threadIdx.x % G;
    const int64_t g = (int64_t)blockIdx.x * GPB + threadIdx.x / G, stride = (int64_t)gridDim.x * GPB;
    const int c0 = blockIdx.y * (G * CPL) + gl;
    const int64_t items = n + sp.n_chunks;
    double msum[CPL], msq[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) msum[q] = msq[q] = 0.0;
    for (int64_t item = g; item < items; item += stride) {
        int32_t start, end;
        int64_t row = item;
        const bool chunk = item >= n;
        if (!chunk) {
            start = rowptr[row];
            end = rowptr[row + 1];
            if (sp.n_long > 0 && end - start > sp.threshold) continue;           // done by chunks
        } else {
            const int32_t cq = (int32_t)(item - n), li = sp.chunk_long[cq];
            row = sp.long_rows[li];
            start = rowptr[row] + (cq - sp.long_chunk_ptr[li]) * sp.threshold;
            end = min(start + sp.threshold, rowptr[row + 1]);
        }
        float s[CPL];
#pragma unroll
        for (int q = 0; q < CPL; ++q) s[q] = 0.f;
        int32_t e = start;
        for (; e + 4 <= end; e += 4) {                                           // four gathers in flight, added in order
            const int64_t j0 = colidx[e], j1 = colidx[e + 1], j2 = colidx[e + 2], j3 = colidx[e + 3];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int c = c0 + G * q;
                if (c < w) {
                    const float v0 = x[j0 * ldx + c], v1 = x[j1 * ldx + c], v2 = x[j2 * ldx + c], v3 = x[j3 * ldx + c];
                    s[q] += v0; s[q] += v1; s[q] += v2; s[q] += v3;
                }
            }
        }
        for (; e < end; ++e) {
            const int64_t j = colidx[e];
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int c = c0 + G * q;
                if (c < w) s[q] += x[j * ldx + c];
            }
        }
        if (chunk) {
#pragma unroll
            for (int q = 0; q < CPL; ++q) {
                const int c = c0 + G * q;
                if (c < w) chunk_part[(item - n) * w + c] = s[q];
            }
            continue;
        }
        const float dg = diag[row];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = c0 + G * q;
            if (c < w) {
                const float v = dg * x[row * ldx + c] - s[q];
                if constexpr (MOMENTS) {
                    msum[q] += (double)v;
                    msq[q] += (double)v * (double)v;
                } else {
                    y[row * ldy + c] = v;
                }
            }
        }
    }
    if constexpr (MOMENTS) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = c0 + G * q;
            if (c < w) {
                part[(g * 2 + 0) * w + c] = msum[q];
                part[(g * 2 + 1) * w + c] = msq[q];
            }
        }
    }
}

// the long rows: a wave per row, 4 columns per lane; the row's chunk partials in chunk order
template <bool MOMENTS>
__global__ void __launch_bounds__(TB)
k_lap_long(const float* __restrict__ diag, int w, const float* __restrict__ x, int64_t ldx, float* __restrict__ y,
           int64_t ldy, Split sp, const float* __restrict__ chunk_part, double* __restrict__ part) {
    constexpr int CPL = 4, GPB = TB / 64;
    const int gl = threadIdx.x % 64;
    const int64_t g = (int64_t)blockIdx.x * GPB + threadIdx.x / 64, stride = (int64_t)gridDim.x * GPB;
    const int c0 = blockIdx.y * (64 * CPL) + gl;
    double msum[CPL], msq[CPL];
#pragma unroll
    for (int q = 0; q < CPL; ++q) msum[q] = msq[q] = 0.0;
    for (int64_t li = g; li < sp.n_long; li += stride) {
        const int64_t row = sp.long_rows[li];
        const int32_t qb = sp.long_chunk_ptr[li], qe = sp.long_chunk_ptr[li + 1];
        const float dg = diag[row];
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = c0 + 64 * q;
            if (c >= w) continue;
            float s = 0.f;
            for (int32_t k = qb; k < qe; ++k) s += chunk_part[(int64_t)k * w + c];
            const float v = dg * x[row * ldx + c] - s;
            if constexpr (MOMENTS) {
                msum[q] += (double)v;
                msq[q] += (double)v * (double)v;
            } else {
                y[row * ldy + c] = v;
            }
        }
    }
    if constexpr (MOMENTS) {
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
            const int c = c0 + 64 * q;
            if (c < w) {
                part[(g * 2 + 0) * w + c] = msum[q];
                part[(g * 2 + 1) * w + c] = msq[q];
            }
        }
    }
}

// out[c] = sum_p part[p][0][c], out[w + c] = sum_p part[p][1][c]: one workgroup per column, a fixed strided order
__global__ void __launch_bounds__(TB)
k_fold_moments(const double* __restrict__ part, int64_t nparts, int w, double* __restrict__ out) {
    __shared__ double red[TB];
    const int c = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t p = threadIdx.x; p < nparts; p += TB) {
        a += part[(p * 2 + 0) * w + c];
        b += part[(p * 2 + 1) * w + c];
    }
    a = block_sum_d(a, red);
    b = block_sum_d(b, red);
    if (threadIdx.x == 0) {
        out[c] = a;
        out[w + c] = b;
    }
}

struct LapPlan {
    int g, cpl;                 // lanes per row, columns per lane
    int64_t row_blocks, long_blocks, col_blocks, long_col_blocks;
    int64_t nparts_rows, nparts;
    size_t chunk_bytes, total_bytes;
};

LapPlan lap_plan(int64_t n, int64_t w, int64_t n_long, int64_t n_chunks, bool moments) {
    LapPlan p{};
    if (w <= 16) { p.g = 8; p.cpl = 2; }
    else if (w <= 64) { p.g = 64; p.cpl = 1; }
    else if (w <= 128) { p.g = 64; p.cpl = 2; }
    else { p.g = 64; p.cpl = 4; }
    const int gpb = TB / p.g;
    p.row_blocks = gda_cdiv(n + n_chunks, gpb);
    p.long_blocks = n_long > 0 ? gda_cdiv(n_long, TB / 64) : 0;
    if (moments) {
        if (p.row_blocks > LAP_MOMENT_BLOCKS) p.row_blocks = LAP_MOMENT_BLOCKS;
        if (p.long_blocks > LAP_LONG_BLOCKS) p.long_blocks = LAP_LONG_BLOCKS;
    }
    p.col_blocks = gda_cdiv(w, p.g * p.cpl);
    p.long_col_blocks = gda_cdiv(w, 256);
    p.nparts_rows = p.row_blocks * gpb;
    p.nparts = p.nparts_rows + p.long_blocks * (TB / 64);
    p.chunk_bytes = gda_align_up((size_t)(n_long > 0 ? n_chunks : 0) * (size_t)w * sizeof(float), 16);
    p.total_bytes = p.chunk_bytes + (moments ? (size_t)p.nparts * 2 * (size_t)w * sizeof(double) : 0);
    return p;
}

int lap_check(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n, int64_t w, const float* x,
              int64_t ldx, const gda_row_split* sp) {
    if (n < 0 || w < 0 || n >= INT32_MAX || ldx < w) return GDA_E_SIZE;
    if (w > MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (n == 0 || w == 0) return GDA_OK;
    if (!rowptr || !diag || !x) return GDA_E_NULL;
    (void)colidx;               // may be NULL only when nnz == 0, which the host cannot see here
    if (sp && sp->n_long > 0) {
        if (sp->threshold <= 0 || sp->n_chunks < sp->n_long) return GDA_E_SIZE;
        if (!sp->long_rows || !sp->long_chunk_ptr || !sp->chunk_long) return GDA_E_NULL;
        if (sp->counts_dev) return GDA_E_UNSUPPORTED;      // deferred counts: graphs that live one step, not this one
    }
    return GDA_OK;
}

Split make_split(const gda_row_split* h) {
    Split sp{};
    if (h && h->threshold > 0 && h->n_long > 0) {
        sp.threshold = h->threshold; sp.n_long = h->n_long; sp.n_chunks = h->n_chunks;
        sp.long_rows = h->long_rows; sp.long_chunk_ptr = h->long_chunk_ptr; sp.chunk_long = h->chunk_long;
    }
    return sp;
}

template <bool MOMENTS>
int lap_launch(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n, int w, const float* x,
               int64_t ldx, float* y, int64_t ldy, const Split& sp, const LapPlan& p, float* chunk_part, double* part,
               hipStream_t s) {
    if (p.row_blocks > INT32_MAX) return GDA_E_SIZE;
    const dim3 grid((unsigned)p.row_blocks, (unsigned)p.col_blocks);
#define GO(G, C) k_lap_rows<G, C, MOMENTS><<<grid, TB, 0, s>>>(rowptr, colidx, diag, n, w, x, ldx, y, ldy, sp, chunk_part, part)
    if (p.g == 8) GO(8, 2);
    else if (p.cpl == 1) GO(64, 1);
    else if (p.cpl == 2) GO(64, 2);
    else GO(64, 4);
#undef GO
    GDA_LAUNCH_CHECK();
    if (sp.n_long > 0) {
        k_lap_long<MOMENTS><<<dim3((unsigned)p.long_blocks, (unsigned)p.long_col_blocks), TB, 0, s>>>(
            diag, w, x, ldx, y, ldy, sp, chunk_part, part ? part + p.nparts_rows * 2 * w : nullptr);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

// ---- the Gram matrix -------------------------------------------------------------------------------------------------
constexpr int GT = 64, GDK = 32, GLD = GT + 4;
constexpr int GRAM_BLOCKS = 2048;          // tiles x slabs aimed at: eight workgroups per CU

using f32x16 = __attribute__((ext_vector_type(16))) float;

// rows r, columns c .. c + 3 of Y with zeros outside [0, rows) x [0, w); a 16-byte load where the row allows it (the
// columns w .. ld of a padded panel may hold anything: they are read, never used)
__device__ __forceinline__ float4 gram_ld4(const float* __restrict__ Y, int64_t ld, int64_t r, int64_t c, int64_t rows,
                                           int64_t w, bool vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= rows || c >= w) return v;
    const float* q = Y + r * ld + c;
    if (vec && c + 3 < ld) {
        v = *reinterpret_cast<const float4*>(q);
        if (c + 1 >= w) v.y = 0.f;
        if (c + 2 >= w) v.z = 0.f;
        if (c + 3 >= w) v.w = 0.f;
        return v;
    }
    v.x = q[0];
    if (c + 1 < w) v.y = q[1];
    if (c + 2 < w) v.z = q[2];
    if (c + 3 < w) v.w = q[3];
    return v;
}

struct GramPlan {
    int64_t tiles_1d, ntiles, slabs, slab_rows;
    size_t bytes;
};

GramPlan gram_plan(int64_t n, int64_t w) {
    GramPlan p{};
    p.tiles_1d = gda_cdiv(w, GT);
    p.ntiles = p.tiles_1d * (p.tiles_1d + 1) / 2;
    int64_t cap = GRAM_BLOCKS / (p.ntiles > 0 ? p.ntiles : 1);
    if (cap < 1) cap = 1;
    int64_t s = gda_cdiv(n, 256);
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    p.slab_rows = gda_cdiv(gda_cdiv(n, s), GDK) * GDK;
    if (p.slab_rows < GDK) p.slab_rows = GDK;
    p.slabs = n > 0 ? gda_cdiv(n, p.slab_rows) : 1;
    p.bytes = (size_t)p.slabs * (size_t)p.ntiles * GT * GT * sizeof(float);
    return p;
}

// tile t = ti (ti + 1) / 2 + tj (tj <= ti) of slab blockIdx.y: part[slab][t] = Y[rows of the slab, i-columns]^T Y[.., j-columns]
__global__ void __launch_bounds__(TB)
k_gram(const float* __restrict__ Y, int64_t ld, int64_t n, int64_t w, int64_t slab_rows, int ntiles,
       float* __restrict__ part, bool vec) {
    __shared__ __attribute__((aligned(16))) float As[GDK][GLD];
    __shared__ __attribute__((aligned(16))) float Bs[GDK][GLD];
    const int t = blockIdx.x;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int64_t i0 = (int64_t)ti * GT, j0 = (int64_t)tj * GT;
    const int64_t kbeg = (int64_t)blockIdx.y * slab_rows, kend = min(n, kbeg + slab_rows);
    const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    const int ka = lane >> 5, la = lane & 31;
    const int kk = tid / 16, c4 = (tid % 16) * 4;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float4 va[2], vb[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        va[q] = gram_ld4(Y, ld, kbeg + kk + 16 * q, i0 + c4, kend, w, vec);
        vb[q] = gram_ld4(Y, ld, kbeg + kk + 16 * q, j0 + c4, kend, w, vec);
    }
    for (int64_t k0 = kbeg; k0 < kend; k0 += GDK) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *reinterpret_cast<float4*>(&As[kk + 16 * q][c4]) = va[q];
            *reinterpret_cast<float4*>(&Bs[kk + 16 * q][c4]) = vb[q];
        }
        if (k0 + GDK < kend) {                                   // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                va[q] = gram_ld4(Y, ld, k0 + GDK + kk + 16 * q, i0 + c4, kend, w, vec);
                vb[q] = gram_ld4(Y, ld, k0 + GDK + kk + 16 * q, j0 + c4, kend, w, vec);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GDK; k += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k + ka][wi + la], Bs[k + ka][wj + la], acc, 0, 0, 0);
    }
    float* out = part + ((int64_t)blockIdx.y * ntiles + t) * (GT * GT);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int il = wi + (r & 3) + 8 * (r >> 2) + 4 * ka;     // C/D layout of the 32x32 MFMA
        out[il * GT + wj + la] = acc[r] + 0.f;
    }
}

// G[i][j] = G[j][i] = sum over the slabs, in slab order, of the lower-triangle tile entry (i >= j)
__global__ void __launch_bounds__(TB)
k_gram_fold(const float* __restrict__ part, int slabs, int ntiles, int64_t w, float* __restrict__ G, int64_t ldg) {
    const int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (idx >= (int64_t)ntiles * GT * GT) return;
    const int t = (int)(idx / (GT * GT)), il = (int)(idx % (GT * GT)) / GT, jl = (int)(idx % GT);
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const int64_t i = (int64_t)ti * GT + il, j = (int64_t)tj * GT + jl;
    if (i >= w || j >= w || j > i) return;
    const float* src = part + idx;
    const int64_t step = (int64_t)ntiles * GT * GT;
    float a = 0.f;
    int z = 0;
    for (; z + 4 <= slabs; z += 4) {
        const float v0 = src[z * step], v1 = src[(z + 1) * step], v2 = src[(z + 2) * step], v3 = src[(z + 3) * step];
        a += v0; a += v1; a += v2; a += v3;
    }
    for (; z < slabs; ++z) a += src[z * step];
    G[i * ldg + j] = a;
    G[j * ldg + i] = a;
}

}  // namespace

extern "C" size_t gda_svd_lap_workspace_bytes(int64_t n, int64_t w, int64_t n_long, int64_t n_chunks, int moments) {
    if (n <= 0 || w <= 0 || n_long < 0 || n_chunks < 0) return 0;
    return lap_plan(n, w, n_long, n_chunks, moments != 0).total_bytes;
}

extern "C" int gda_svd_lap_apply_f32(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n,
                                     int64_t w, const float* x, int64_t ldx, float* y, int64_t ldy,
                                     const gda_row_split* split, void* workspace, size_t workspace_bytes,
                                     gda_stream_t stream) {
    if (ldy < w) return GDA_E_SIZE;
    int st = lap_check(rowptr, colidx, diag, n, w, x, ldx, split);
    if (st != GDA_OK || n == 0 || w == 0) return st;
    if (!y) return GDA_E_NULL;
    if ((const float*)y == x) return GDA_E_ALIAS;
    const Split sp = make_split(split);
    const LapPlan p = lap_plan(n, w, sp.n_long, sp.n_chunks, false);
    if (p.total_bytes > 0 && (!workspace || workspace_bytes < p.total_bytes)) return GDA_E_WORKSPACE;
    if (p.total_bytes > 0 && ((uintptr_t)workspace & 15)) return GDA_E_UNSUPPORTED;
    return lap_launch<false>(rowptr, colidx, diag, n, (int)w, x, ldx, y, ldy, sp, p, (float*)workspace, nullptr,
                             (hipStream_t)stream);
}

extern "C" int gda_svd_lap_moments_f32(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n,
                                       int64_t w, const float* x, int64_t ldx, double* moments,
                                       const gda_row_split* split, void* workspace, size_t workspace_bytes,
                                       gda_stream_t stream) {
    int st = lap_check(rowptr, colidx, diag, n, w, x, ldx, split);
    if (st != GDA_OK || w == 0) return st;
    if (!moments) return GDA_E_NULL;
    if ((const void*)moments == (const void*)x) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        GDA_HIP_TRY(hipMemsetAsync(moments, 0, sizeof(double) * 2 * (size_t)w, s));
        return GDA_OK;
    }
    const Split sp = make_split(split);
    const LapPlan p = lap_plan(n, w, sp.n_long, sp.n_chunks, true);
    if (!workspace || workspace_bytes < p.total_bytes) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    double* part = (double*)((char*)workspace + p.chunk_bytes);
    st = lap_launch<true>(rowptr, colidx, diag, n, (int)w, x, ldx, nullptr, 0, sp, p, (float*)workspace, part, s);
    if (st != GDA_OK) return st;
    k_fold_moments<<<(unsigned)w, TB, 0, s>>>(part, p.nparts, (int)w, moments);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_svd_gram_workspace_bytes(int64_t n, int64_t w) {
    if (n <= 0 || w <= 0 || w > MAX_WIDTH) return 0;
    return gram_plan(n, w).bytes;
}

extern "C" int gda_svd_gram_f32(const float* Y, int64_t ldy, int64_t n, int64_t w, float* G, int64_t ldg,
                                void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 0 || w < 0 || ldy < w || ldg < w) return GDA_E_SIZE;
    if (w > MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (w == 0) return GDA_OK;
    if (!G || (n > 0 && !Y)) return GDA_E_NULL;
    if ((const float*)G == Y) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        GDA_HIP_TRY(hipMemset2DAsync(G, sizeof(float) * ldg, 0, sizeof(float) * w, (size_t)w, s));
        return GDA_OK;
    }
    const GramPlan p = gram_plan(n, w);
    if (!workspace || workspace_bytes < p.bytes) return GDA_E_WORKSPACE;
    if ((uintptr_t)workspace & 15) return GDA_E_UNSUPPORTED;
    const bool vec = ldy % 4 == 0 && ((uintptr_t)Y & 15) == 0;
    k_gram<<<dim3((unsigned)p.ntiles, (unsigned)p.slabs), TB, 0, s>>>(Y, ldy, n, w, p.slab_rows, (int)p.ntiles,
                                                                     (float*)workspace, vec);
    GDA_LAUNCH_CHECK();
    k_gram_fold<<<(unsigned)gda_cdiv(p.ntiles * GT * GT, TB), TB, 0, s>>>((const float*)workspace, (int)p.slabs,
                                                                         (int)p.ntiles, w, G, ldg);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
