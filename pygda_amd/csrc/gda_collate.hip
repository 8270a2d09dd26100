// Device-side collation of graph-mode batches out of a device-resident dataset (pygda_amd.data.GraphStore), gfx950.
//
// The dataset is one block-diagonal graph in dataset order: node rows, edges and the entries of its normalised CSR are
// stored graph after graph.  A batch is a list of graph ids; everything PyG's Batch.from_data_list would build for it is
// a SEGMENTED GATHER WITH INDEX SHIFT: the b-th chosen graph's block is copied behind the blocks of the b graphs before
// it, node ids moved by (its first row in the batch) - (its first row in the store).  gcn_norm never looks across a
// block and gda_graph.hip keeps each row's entries in edge order, so the gathered CSR is the CSR a fresh build of the
// collated edge list would give, bit for bit.
//
//   offsets : exclusive scans of the chosen graphs' node / edge / entry counts (one workgroup per scan, chunked with a
//             carry: any batch size)
//   gathers : lanes map to FLAT OUTPUT positions -- a graph here has 1 to ~100 nodes, one workgroup per graph would idle
//             the chip -- and find the owning graph in the batch's offset array (feature rows: in the `batch` vector the
//             node pass has just written, one load instead of a search per 16 bytes).  Feature rows move as 16-byte
//             accesses when F % 4 == 0 (row starts are then 16-byte aligned), as scalars otherwise.
//
//   ppmi    : a store in "per_graph" mode keeps every graph's random-walk PPMI pairs (graph-local ids, p / colsum in
//             double: walks never leave a block); a batch's pair list is the same gather, and the one thing that depends
//             on the batch -- its number of visited nodes, a host sum -- enters each weight through the clipped log
//   ppmi csr: the NORMALISED graph of that pair list without running the ingestion per batch: its structure is the
//             store's own (gathered like any variant's), its values are the weights above pushed through k_degree's
//             and k_normalize's arithmetic -- three launches (gather + weight, degree per row, scale per row) behind the
//             pair gather, bound: the copies plus one double log per pair
//
// These are copies: their bound is HBM bandwidth (read + write of every byte once).  An id outside [0, G) counts as an
// empty graph; every gather stops at the capacity the caller passed, whatever the device offsets say.
#include "gda_common.h"

namespace {

constexpr int TB = 256;
constexpr int SCAN_TB = 1024;
constexpr int MAX_BLOCKS = 8192;          // grid-stride beyond it: 32 workgroups per CU

struct ScanJob {
    const int64_t* ptr;        // [G + 1] dataset pointers
    const int32_t* rowptr;     // NULL: count = ptr[g+1] - ptr[g]; else count = rowptr[ptr[g+1]] - rowptr[ptr[g]]
    int64_t* out;              // [B + 1]
};

__device__ __forceinline__ int64_t count_of(const ScanJob& j, int64_t g, int64_t G) {
    if (g < 0 || g >= G) return 0;
    const int64_t a = j.ptr[g], b = j.ptr[g + 1];
    return j.rowptr ? (int64_t)j.rowptr[b] - (int64_t)j.rowptr[a] : b - a;
}

// one workgroup per job; chunks of SCAN_TB ids, the running total carried from chunk to chunk
__global__ void __launch_bounds__(SCAN_TB)
k_collate_scan(const int64_t* __restrict__ ids, int64_t B, int64_t G, ScanJob j0, ScanJob j1) {
    __shared__ int64_t wave_sum[SCAN_TB / GDA_WAVE];
    __shared__ int64_t carry_s;
    const ScanJob j = blockIdx.x == 0 ? j0 : j1;
    const int lane = threadIdx.x & (GDA_WAVE - 1), wave = threadIdx.x / GDA_WAVE;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < B; base += SCAN_TB) {
        const int64_t b = base + threadIdx.x;
        const int64_t c = b < B ? count_of(j, ids[b], G) : 0;
        int64_t incl = c;
#pragma unroll
        for (int o = 1; o < GDA_WAVE; o <<= 1) {
            const int64_t up = __shfl_up(incl, o, GDA_WAVE);
            if (lane >= o) incl += up;
        }
        if (lane == GDA_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_sum[w];
        if (b < B) j.out[b] = before + incl - c;
        __syncthreads();                                  // everyone has read carry_s and wave_sum
        if (threadIdx.x == SCAN_TB - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) j.out[B] = carry_s;
}

// largest b in [0, B) with off[b] <= p, for 0 <= p < off[B]: the (non-empty) segment that holds position p
__device__ __forceinline__ int64_t owner_of(const int64_t* __restrict__ off, int64_t B, int64_t p) {
    int64_t lo = 0, hi = B;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// per node: batch[r] = its graph's position in the batch; per chosen graph: y_out[b] = y[ids[b]]
__global__ void __launch_bounds__(TB)
k_collate_nodes(const int64_t* __restrict__ ids, int64_t B, int64_t G, const int64_t* __restrict__ seg_ptr,
                const int64_t* __restrict__ y, int64_t n_cap, int64_t* __restrict__ batch_out,
                int64_t* __restrict__ y_out) {
    const int64_t n = min64(n_cap, seg_ptr[B]);
    const int64_t work = n > B ? n : B;
    for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < work; r += (int64_t)gridDim.x * TB) {
        if (r < n) batch_out[r] = owner_of(seg_ptr, B, r);
        if (r < B) {
            const int64_t g = ids[r];
            y_out[r] = (g >= 0 && g < G) ? y[g] : -1;
        }
    }
}

// out[r, :] = x[node_ptr[ids[b]] + r - seg_ptr[b], :], b = batch[r]; one lane per UNIT of V floats
template <typename V>
__global__ void __launch_bounds__(TB)
k_collate_rows(const V* __restrict__ x, int64_t upr, const int64_t* __restrict__ ids, int64_t B,
               const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ seg_ptr,
               const int64_t* __restrict__ batch, int64_t n_cap, V* __restrict__ out) {
    const int64_t units = min64(n_cap, seg_ptr[B]) * upr;
    for (int64_t u = (int64_t)blockIdx.x * TB + threadIdx.x; u < units; u += (int64_t)gridDim.x * TB) {
        const int64_t r = u / upr;
        const int64_t b = batch[r];
        const int64_t shift = node_ptr[ids[b]] - seg_ptr[b];          // store row - batch row
        out[u] = x[u + shift * upr];
    }
}

// out[k, e] = edges[k, edge_ptr[ids[b]] + e - edge_off[b]] + seg_ptr[b], k = 0, 1 (graph-local ids in the store)
__global__ void __launch_bounds__(TB)
k_collate_edges(const int64_t* __restrict__ ids, int64_t B, const int64_t* __restrict__ edge_ptr,
                const int64_t* __restrict__ edge_off, const int64_t* __restrict__ seg_ptr,
                const int64_t* __restrict__ edges, int64_t E_total, int64_t e_cap, int64_t* __restrict__ out) {
    const int64_t E = min64(e_cap, edge_off[B]);
    for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < E; e += (int64_t)gridDim.x * TB) {
        const int64_t b = owner_of(edge_off, B, e);
        const int64_t s = edge_ptr[ids[b]] + e - edge_off[b];
        const int64_t first = seg_ptr[b];
        out[e] = edges[s] + first;
        out[e_cap + e] = edges[E_total + s] + first;
    }
}

// PPMI pair k of the batch = pair (k - pair_off[b]) of graph ids[b]'s block (stored once per graph: graph-local ids and
// ratio = p / colsum in double); its weight is k_weights' expression (gda_ppmi_dev.hip) -- same association, same double
// log -- with the BATCH's target count, so the bits are those of a fresh build of the collated edge list
__global__ void __launch_bounds__(TB)
k_collate_ppmi(const int64_t* __restrict__ ids, int64_t B, const int64_t* __restrict__ pair_ptr,
               const int64_t* __restrict__ pair_off, const int64_t* __restrict__ seg_ptr,
               const int32_t* __restrict__ local_src, const int32_t* __restrict__ local_dst,
               const double* __restrict__ ratio, int64_t P_total, int64_t n_targets, int path_len, int64_t m_cap,
               int64_t* __restrict__ out, float* __restrict__ w_out) {
    const int64_t M = min64(m_cap, pair_off[B]);
    for (int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x; k < M; k += (int64_t)gridDim.x * TB) {
        const int64_t b = owner_of(pair_off, B, k);
        const int64_t s = pair_ptr[ids[b]] + k - pair_off[b];
        if (s < 0 || s >= P_total) continue;              // (a pair pointer that is not the store's own)
        const int64_t first = seg_ptr[b];
        out[k] = (int64_t)local_src[s] + first;
        out[m_cap + k] = (int64_t)local_dst[s] + first;
        const double v = log(ratio[s] * (double)n_targets / (double)path_len);
        w_out[k] = (float)(v > 0.0 ? v : 0.0);
    }
}

struct CsrSide {
    const int32_t* rowptr; const int32_t* colidx; const float* val;
    int32_t* rowptr_out; int32_t* colidx_out; float* val_out;
};

// rowptr_out[r] = rowptr[store row of r] - (first entry of its graph in the store) + (first entry of it in the batch)
__global__ void __launch_bounds__(TB)
k_collate_rowptr(const int64_t* __restrict__ ids, int64_t B, const int64_t* __restrict__ node_ptr,
                 const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ batch,
                 const int64_t* __restrict__ nnz_off, int64_t n_cap, CsrSide fwd, CsrSide bwd) {
    const CsrSide s = blockIdx.y == 0 ? fwd : bwd;
    const int64_t n = min64(n_cap, seg_ptr[B]);
    for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r <= n_cap; r += (int64_t)gridDim.x * TB) {
        if (r >= n) {                                     // the closing entry (and rows a short device total leaves)
            s.rowptr_out[r] = (int32_t)nnz_off[B];
            continue;
        }
        const int64_t b = batch[r];
        const int64_t first = node_ptr[ids[b]];
        s.rowptr_out[r] = (int32_t)((int64_t)s.rowptr[first + r - seg_ptr[b]] - (int64_t)s.rowptr[first] + nnz_off[b]);
    }
}

// entry k of the batch = entry (k - nnz_off[b]) of graph ids[b]'s block; its column moves with the graph's rows
__global__ void __launch_bounds__(TB)
k_collate_entries(const int64_t* __restrict__ ids, int64_t B, const int64_t* __restrict__ node_ptr,
                  const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ nnz_off, int64_t nnz_cap,
                  CsrSide fwd, CsrSide bwd) {
    const CsrSide s = blockIdx.y == 0 ? fwd : bwd;
    const int64_t nnz = min64(nnz_cap, nnz_off[B]);
    for (int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * TB) {
        const int64_t b = owner_of(nnz_off, B, k);
        const int64_t first = node_ptr[ids[b]];
        const int64_t src = (int64_t)s.rowptr[first] + k - nnz_off[b];
        s.colidx_out[k] = (int32_t)((int64_t)s.colidx[src] + seg_ptr[b] - first);
        s.val_out[k] = s.val[src];
    }
}

// ---- the normalised PPMI graph of a batch, without a sort (gda_collate_ppmi_csr_f32) ----
// What gda_build_csr_norm makes of a batch's PPMI pair list has a structure that is fixed per graph (gda_graph.hip keeps
// every edge whatever its weight, sorts stably, closes each row with the node's loop; a walk never leaves its graph):
// the store keeps both CSRs of the dataset-order graph and, per stored entry, the pair whose ratio weighs it (-1: a
// loop filled with the constant).  Only the values depend on the batch, through its target count.
struct PpmiSide {
    const int32_t* rowptr; const int32_t* colidx; const int32_t* pair_of;
    int32_t* rowptr_out; int32_t* colidx_out; float* val_out;
};

// rowptr as k_collate_rowptr, colidx as k_collate_entries; val_out = the entry's raw weight: its pair's, as k_collate_ppmi
// has just written it into the batch's pair list (one double log per PAIR, shared by the pair's entry on either side)
__global__ void __launch_bounds__(TB)
k_ppmi_csr_gather(const int64_t* __restrict__ ids, int64_t B, int64_t G, const int64_t* __restrict__ node_ptr,
                  const int64_t* __restrict__ seg_ptr, const int64_t* __restrict__ batch,
                  const int64_t* __restrict__ ent_off, int64_t n_cap, int64_t nnz_cap, int64_t nnz_total,
                  const int64_t* __restrict__ pair_ptr, const int64_t* __restrict__ pair_off,
                  const float* __restrict__ w_pairs, int64_t m_cap, float fill_value, PpmiSide fwd, PpmiSide bwd) {
    const PpmiSide s = blockIdx.y == 0 ? fwd : bwd;
    const int64_t n = min64(n_cap, seg_ptr[B]);
    const int64_t nnz = min64(nnz_cap, ent_off[B]);
    const int64_t work = nnz > n_cap + 1 ? nnz : n_cap + 1;
    for (int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x; i < work; i += (int64_t)gridDim.x * TB) {
        if (i <= n_cap) {
            int64_t v = nnz;                              // the closing entry (and rows a short device total leaves)
            if (i < n) {
                const int64_t b = batch[i];
                const int64_t g = (b >= 0 && b < B) ? ids[b] : -1;
                if (g >= 0 && g < G) {
                    const int64_t first = node_ptr[g];
                    v = min64((int64_t)s.rowptr[first + i - seg_ptr[b]] - (int64_t)s.rowptr[first] + ent_off[b], nnz);
                }
            }
            s.rowptr_out[i] = (int32_t)v;
        }
        if (i < nnz) {
            const int64_t b = owner_of(ent_off, B, i);
            const int64_t g = ids[b];
            int32_t col = 0;
            float w = 0.0f;
            if (g >= 0 && g < G) {
                const int64_t first = node_ptr[g];
                const int64_t src = (int64_t)s.rowptr[first] + i - ent_off[b];
                if (src >= 0 && src < nnz_total) {
                    col = (int32_t)((int64_t)s.colidx[src] + seg_ptr[b] - first);
                    // the pair's place in the batch's pair list: (its place in its graph's block) + (the block's)
                    const int64_t p = s.pair_of[src];
                    const int64_t k = p >= 0 && m_cap > 0 ? p - pair_ptr[g] + pair_off[b] : -1;
                    w = (k >= 0 && k < m_cap) ? w_pairs[k] : fill_value;
                }
            }
            s.colidx_out[i] = col;
            s.val_out[i] = w;
        }
    }
}

// k_degree of gda_graph.hip over the by-source rows (degree_side = "row"): sequential in entry order
__global__ void __launch_bounds__(TB)
k_ppmi_csr_degree(const int32_t* __restrict__ t_rowptr_out, const float* __restrict__ t_val_out, int64_t n_cap,
                  int64_t nnz_cap, float* __restrict__ dis) {
    for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < n_cap; r += (int64_t)gridDim.x * TB) {
        const int64_t lo = t_rowptr_out[r], hi = min64(t_rowptr_out[r + 1], nnz_cap);
        float s = 0.0f;
        for (int64_t k = lo < 0 ? 0 : lo; k < hi; ++k) s = __fadd_rn(s, t_val_out[k]);
        float d = 1.0f / sqrtf(s);
        if (isinf(d)) d = 0.0f;
        dis[r] = d;
    }
}

// k_normalize of gda_graph.hip, one lane per row of either side: dis[source] * w * dis[target]
__global__ void __launch_bounds__(TB)
k_ppmi_csr_scale(int64_t n_cap, int64_t nnz_cap, const float* __restrict__ dis, PpmiSide fwd, PpmiSide bwd) {
    const bool by_dst = blockIdx.y == 0;
    const PpmiSide s = by_dst ? fwd : bwd;
    for (int64_t r = (int64_t)blockIdx.x * TB + threadIdx.x; r < n_cap; r += (int64_t)gridDim.x * TB) {
        const int64_t lo = s.rowptr_out[r], hi = min64(s.rowptr_out[r + 1], nnz_cap);
        const float dr = dis[r];
        // four entries per trip, their loads issued together: a row's entries depend on nothing but their own column
        for (int64_t k = lo < 0 ? 0 : lo; k < hi; k += 4) {
            int64_t c[4];
            float w[4], dc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = k + j < hi ? (int64_t)s.colidx_out[k + j] : -1;
                w[j] = k + j < hi ? s.val_out[k + j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) dc[j] = (c[j] >= 0 && c[j] < n_cap) ? dis[c[j]] : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k + j < hi)
                    s.val_out[k + j] = by_dst ? __fmul_rn(__fmul_rn(dc[j], w[j]), dr) : __fmul_rn(__fmul_rn(dr, w[j]), dc[j]);
        }
    }
}

inline int blocks_for(int64_t work) { return (int)(gda_cdiv(work, TB) < MAX_BLOCKS ? gda_cdiv(work, TB) : MAX_BLOCKS); }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int gda_collate_offsets(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* edge_ptr,
                        int64_t* seg_ptr_out, int64_t* edge_off_out, gda_stream_t stream) {
    if (B < 0 || G < 0) return GDA_E_SIZE;
    if (B == 0) return 0;
    if (!ids || !node_ptr || !edge_ptr || !seg_ptr_out || !edge_off_out) return GDA_E_NULL;
    if (seg_ptr_out == edge_off_out || seg_ptr_out == ids || edge_off_out == ids || seg_ptr_out == node_ptr
        || seg_ptr_out == edge_ptr || edge_off_out == node_ptr || edge_off_out == edge_ptr) return GDA_E_ALIAS;
    const ScanJob j0{node_ptr, nullptr, seg_ptr_out}, j1{edge_ptr, nullptr, edge_off_out};
    hipLaunchKernelGGL(k_collate_scan, dim3(2), dim3(SCAN_TB), 0, (hipStream_t)stream, ids, B, G, j0, j1);
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_nodes_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                          const float* x, int64_t F, const int64_t* y, int64_t n_out, float* x_out,
                          int64_t* batch_out, int64_t* y_out, gda_stream_t stream) {
    if (B < 0 || G < 0 || F < 0 || n_out < 0) return GDA_E_SIZE;
    if (B == 0) return 0;
    if (!ids || !node_ptr || !seg_ptr || !y || !y_out) return GDA_E_NULL;
    if (n_out > 0 && !batch_out) return GDA_E_NULL;
    if (n_out > 0 && F > 0 && (!x || !x_out)) return GDA_E_NULL;
    if ((x_out && x_out == x) || y_out == y || y_out == ids || batch_out == ids || batch_out == seg_ptr
        || y_out == seg_ptr || (batch_out && batch_out == y_out)) return GDA_E_ALIAS;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_collate_nodes, dim3(blocks_for(n_out > B ? n_out : B)), dim3(TB), 0, st, ids, B, G, seg_ptr, y,
                       n_out, batch_out, y_out);
    GDA_LAUNCH_CHECK();
    if (n_out == 0 || F == 0) return 0;
    if (F % 4 == 0 && aligned16(x) && aligned16(x_out)) {
        const int64_t upr = F / 4;
        hipLaunchKernelGGL(k_collate_rows<float4>, dim3(blocks_for(n_out * upr)), dim3(TB), 0, st,
                           reinterpret_cast<const float4*>(x), upr, ids, B, node_ptr, seg_ptr, batch_out, n_out,
                           reinterpret_cast<float4*>(x_out));
    } else {
        hipLaunchKernelGGL(k_collate_rows<float>, dim3(blocks_for(n_out * F)), dim3(TB), 0, st, x, F, ids, B, node_ptr,
                           seg_ptr, batch_out, n_out, x_out);
    }
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_edges(const int64_t* ids, int64_t B, int64_t G, const int64_t* edge_ptr, const int64_t* edge_off,
                      const int64_t* seg_ptr, const int64_t* edges, int64_t E_total, int64_t e_out,
                      int64_t* edge_index_out, gda_stream_t stream) {
    if (B < 0 || G < 0 || E_total < 0 || e_out < 0 || (E_total == 0 && e_out > 0)) return GDA_E_SIZE;
    if (B == 0 || e_out == 0) return 0;
    if (!ids || !edge_ptr || !edge_off || !seg_ptr || !edges || !edge_index_out) return GDA_E_NULL;
    if (edge_index_out == edges || edge_index_out == ids || edge_index_out == edge_off || edge_index_out == seg_ptr)
        return GDA_E_ALIAS;
    hipLaunchKernelGGL(k_collate_edges, dim3(blocks_for(e_out)), dim3(TB), 0, (hipStream_t)stream, ids, B, edge_ptr,
                       edge_off, seg_ptr, edges, E_total, e_out, edge_index_out);
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_ppmi_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* pair_ptr, const int64_t* pair_off,
                         const int64_t* seg_ptr, const int32_t* local_src, const int32_t* local_dst, const double* ratio,
                         int64_t P_total, int64_t n_targets, int path_len, int64_t m_out, int64_t* pairs_out,
                         float* w_out, gda_stream_t stream) {
    if (B < 0 || G < 0 || P_total < 0 || m_out < 0 || n_targets < 0 || path_len < 1 || (P_total == 0 && m_out > 0))
        return GDA_E_SIZE;
    if (B == 0 || m_out == 0) return 0;
    if (!ids || !pair_ptr || !pair_off || !seg_ptr || !local_src || !local_dst || !ratio || !pairs_out || !w_out)
        return GDA_E_NULL;
    if (pairs_out == ids || pairs_out == pair_ptr || pairs_out == pair_off || pairs_out == seg_ptr
        || (const void*)pairs_out == (const void*)ratio || (const void*)pairs_out == (const void*)local_src
        || (const void*)pairs_out == (const void*)local_dst || (const void*)w_out == (const void*)pairs_out
        || (const void*)w_out == (const void*)ratio || (const void*)w_out == (const void*)local_src
        || (const void*)w_out == (const void*)local_dst)
        return GDA_E_ALIAS;
    hipLaunchKernelGGL(k_collate_ppmi, dim3(blocks_for(m_out)), dim3(TB), 0, (hipStream_t)stream, ids, B, pair_ptr,
                       pair_off, seg_ptr, local_src, local_dst, ratio, P_total, n_targets, path_len, m_out, pairs_out,
                       w_out);
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_ppmi_csr_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                             const int64_t* batch, int64_t n_out, const int64_t* ent_off, int64_t nnz_out,
                             const int32_t* rowptr, const int32_t* colidx, const int32_t* pair_of,
                             const int32_t* t_rowptr, const int32_t* t_colidx, const int32_t* t_pair_of,
                             int64_t nnz_total, const int64_t* pair_ptr, const int64_t* pair_off, const float* w_pairs,
                             int64_t m_pairs, float fill_value, int32_t* rowptr_out, int32_t* colidx_out, float* val_out,
                             int32_t* t_rowptr_out, int32_t* t_colidx_out, float* t_val_out, float* dis_ws,
                             gda_stream_t stream) {
    if (B < 0 || G < 0 || n_out < 0 || nnz_out < 0 || nnz_total < 0 || m_pairs < 0 || n_out >= INT32_MAX
        || nnz_out > INT32_MAX)
        return GDA_E_SIZE;
    if (B == 0) return 0;
    // every row holds at least its loop: rows without room for an entry, or entries out of an empty store, are no batch
    if (nnz_out < n_out || (nnz_total == 0 && nnz_out > 0)) return GDA_E_SIZE;
    if (!ids || !node_ptr || !seg_ptr || !ent_off || !rowptr || !t_rowptr || !rowptr_out || !t_rowptr_out)
        return GDA_E_NULL;
    if (n_out > 0 && (!batch || !dis_ws)) return GDA_E_NULL;
    if (nnz_out > 0 && (!colidx || !pair_of || !t_colidx || !t_pair_of || !colidx_out || !val_out || !t_colidx_out || !t_val_out))
        return GDA_E_NULL;
    if (m_pairs > 0 && (!pair_ptr || !pair_off || !w_pairs)) return GDA_E_NULL;
    if (rowptr_out == rowptr || rowptr_out == t_rowptr || t_rowptr_out == rowptr || t_rowptr_out == t_rowptr
        || rowptr_out == t_rowptr_out)
        return GDA_E_ALIAS;
    if (nnz_out > 0 && (colidx_out == colidx || colidx_out == t_colidx || t_colidx_out == colidx || t_colidx_out == t_colidx
                        || colidx_out == t_colidx_out || colidx_out == pair_of || colidx_out == t_pair_of
                        || t_colidx_out == pair_of || t_colidx_out == t_pair_of || val_out == t_val_out
                        || dis_ws == val_out || dis_ws == t_val_out
                        || val_out == w_pairs || t_val_out == w_pairs || dis_ws == w_pairs))
        return GDA_E_ALIAS;
    hipStream_t st = (hipStream_t)stream;
    const PpmiSide fwd{rowptr, colidx, pair_of, rowptr_out, colidx_out, val_out};
    const PpmiSide bwd{t_rowptr, t_colidx, t_pair_of, t_rowptr_out, t_colidx_out, t_val_out};
    const int64_t work = nnz_out > n_out + 1 ? nnz_out : n_out + 1;
    hipLaunchKernelGGL(k_ppmi_csr_gather, dim3(blocks_for(work), 2), dim3(TB), 0, st, ids, B, G, node_ptr, seg_ptr, batch,
                       ent_off, n_out, nnz_out, nnz_total, pair_ptr, pair_off, w_pairs, m_pairs, fill_value, fwd, bwd);
    GDA_LAUNCH_CHECK();
    if (n_out == 0) return 0;
    hipLaunchKernelGGL(k_ppmi_csr_degree, dim3(blocks_for(n_out)), dim3(TB), 0, st, t_rowptr_out, t_val_out, n_out,
                       nnz_out, dis_ws);
    GDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ppmi_csr_scale, dim3(blocks_for(n_out), 2), dim3(TB), 0, st, n_out, nnz_out, dis_ws, fwd, bwd);
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_csr_offsets(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int32_t* rowptr,
                            int64_t* nnz_off_out, gda_stream_t stream) {
    if (B < 0 || G < 0) return GDA_E_SIZE;
    if (B == 0) return 0;
    if (!ids || !node_ptr || !rowptr || !nnz_off_out) return GDA_E_NULL;
    if (nnz_off_out == ids || nnz_off_out == node_ptr || (const void*)nnz_off_out == (const void*)rowptr)
        return GDA_E_ALIAS;
    const ScanJob j0{node_ptr, rowptr, nnz_off_out};
    hipLaunchKernelGGL(k_collate_scan, dim3(1), dim3(SCAN_TB), 0, (hipStream_t)stream, ids, B, G, j0, j0);
    GDA_LAUNCH_CHECK();
    return 0;
}

int gda_collate_csr_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                        const int64_t* batch, int64_t n_out, const int64_t* nnz_off, int64_t nnz_out,
                        const int32_t* rowptr, const int32_t* colidx, const float* val, const int32_t* t_rowptr,
                        const int32_t* t_colidx, const float* t_val, int32_t* rowptr_out, int32_t* colidx_out,
                        float* val_out, int32_t* t_rowptr_out, int32_t* t_colidx_out, float* t_val_out,
                        gda_stream_t stream) {
    if (B < 0 || G < 0 || n_out < 0 || nnz_out < 0 || n_out >= INT32_MAX || nnz_out > INT32_MAX) return GDA_E_SIZE;
    if (B == 0) return 0;
    if (!ids || !node_ptr || !seg_ptr || !nnz_off || !rowptr || !t_rowptr || !rowptr_out || !t_rowptr_out)
        return GDA_E_NULL;
    if (n_out > 0 && !batch) return GDA_E_NULL;
    if (nnz_out > 0 && (!colidx || !val || !t_colidx || !t_val || !colidx_out || !val_out || !t_colidx_out || !t_val_out))
        return GDA_E_NULL;
    if (rowptr_out == rowptr || rowptr_out == t_rowptr || t_rowptr_out == rowptr || t_rowptr_out == t_rowptr
        || rowptr_out == t_rowptr_out)
        return GDA_E_ALIAS;
    if (nnz_out > 0 && (colidx_out == colidx || colidx_out == t_colidx || t_colidx_out == colidx || t_colidx_out == t_colidx
                        || colidx_out == t_colidx_out || val_out == val || val_out == t_val || t_val_out == val
                        || t_val_out == t_val || val_out == t_val_out))
        return GDA_E_ALIAS;
    hipStream_t st = (hipStream_t)stream;
    const CsrSide fwd{rowptr, colidx, val, rowptr_out, colidx_out, val_out};
    const CsrSide bwd{t_rowptr, t_colidx, t_val, t_rowptr_out, t_colidx_out, t_val_out};
    hipLaunchKernelGGL(k_collate_rowptr, dim3(blocks_for(n_out + 1), 2), dim3(TB), 0, st, ids, B, node_ptr, seg_ptr, batch,
                       nnz_off, n_out, fwd, bwd);
    GDA_LAUNCH_CHECK();
    if (nnz_out == 0) return 0;
    hipLaunchKernelGGL(k_collate_entries, dim3(blocks_for(nnz_out), 2), dim3(TB), 0, st, ids, B, node_ptr, seg_ptr, nnz_off,
                       nnz_out, fwd, bwd);
    GDA_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
