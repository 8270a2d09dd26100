/*
 * gda_hip.h -- C ABI of libgda_hip.so: the MI355X (gfx950) kernels behind pygda's
 * message-passing / domain-adaptation-loss hot path.
 *
 * The reference (pygda-team/pygda v1.2.1) is pure Python and has no FFI of its own;
 * the arithmetic on this path lives in third-party wheels it calls (PyG
 * MessagePassing.propagate, torch_scatter.scatter_add, add_remaining_self_loops) and
 * in torch elementwise chains (pygda/utils/mmd.py).  Each entry point below names the
 * reference call site(s) whose work it replaces.  pygda_amd/ binds these with ctypes
 * (INTEGRATION.md shows the stub a pygda maintainer would add).
 *
 * Conventions
 *   - every function returns int: 0 = ok, <0 = invalid argument (GDA_E_*),
 *     >0 = hipError_t of the failing runtime call.  Nothing throws across the ABI.
 *   - all pointers are caller-owned DEVICE pointers unless the name ends in _host;
 *     kernels never allocate: scratch is passed in (size from gda_*_workspace_bytes).
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); all
 *     work is enqueued asynchronously on it; the library keeps no mutable state, so
 *     calls are re-entrant and hipGraph-capturable.
 *   - indices inside the library are int32 (N, nnz < 2^31); features are fp32,
 *     row-major with an explicit leading dimension in elements.
 */
#ifndef GDA_HIP_H
#define GDA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDA_OK 0
#define GDA_E_NULL (-1)      /* required pointer is NULL */
#define GDA_E_SIZE (-2)      /* negative / overflowing / inconsistent size */
#define GDA_E_WORKSPACE (-3) /* workspace too small */
#define GDA_E_UNSUPPORTED (-4)
#define GDA_E_ALIAS (-5)     /* output aliases an input that must stay intact */
#define GDA_E_RCCL (-100)    /* RCCL failure: status = GDA_E_RCCL - ncclResult_t */

typedef void* gda_stream_t;

int gda_abi_version(void);
/* Human-readable text for a status returned by any function here. */
const char* gda_status_string(int status);

/* ------------------------------------------------------------------------------
 * Graph ingestion: COO edge list -> self-loop merge -> symmetric normalisation ->
 * CSR by destination (forward) + CSR by source (transpose, for the backward pass).
 *
 * Replaces gcn_norm (pygda/nn/prop_gcn_conv.py:64-81: add_remaining_self_loops :72,
 * scatter_add degree over col :78, deg^-1/2 with inf->0 :79-80, w' = dis[row]*w*dis[col]
 * :81) and CachedGCNConv.norm (pygda/nn/cached_gcn_conv.py:88-103, degree over row),
 * plus the edge ordering PyG's propagate scatter relies on.  Both CSRs keep the
 * edges of a row in their original edge order (stable sort), so a sequential row
 * sum reproduces the CPU scatter-add order.
 *
 *   src,dst   [E] int64  edge_index[0], edge_index[1]  (message flows src -> dst)
 *   w         [E] fp32 or NULL (all ones)
 *   fill_value     self-loop weight for nodes without one (1, or 2 for improved)
 *   add_self_loops 0 = edges as given; 1 = PyG add_remaining_self_loops; 2 = existing loops dropped,
 *                  none appended (get_laplacian's remove_self_loops, pygda/nn/dgsda_base.py:128)
 *   normalize 0/1 (0: values are the raw weights)
 *   degree_side    0 = over dst/col (PropGCNConv, GCNConv), 1 = over src/row (CachedGCNConv)
 *   rowptr  [N+1], colidx/val [E+N]  : by-destination CSR, colidx = source node
 *   t_rowptr[N+1], t_colidx/t_val [E+N] : by-source CSR, t_colidx = destination node
 * nnz (= kept edges + N) is rowptr[N].
 * ---------------------------------------------------------------------------- */
size_t gda_graph_workspace_bytes(int64_t E, int64_t N);
int gda_build_csr_norm(const int64_t* src, const int64_t* dst, const float* w,
                       int64_t E, int64_t N, float fill_value, int add_self_loops,
                       int normalize, int degree_side,
                       int32_t* rowptr, int32_t* colidx, float* val,
                       int32_t* t_rowptr, int32_t* t_colidx, float* t_val,
                       void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* Same, and additionally t_to_fwd [E+N]: for entry k' of the by-source CSR, the position of the
 * same edge in the by-destination CSR -- lets a backward pass that walks the transpose read
 * per-edge quantities (attention coefficients) stored in forward order. */
int gda_build_csr_norm_map(const int64_t* src, const int64_t* dst, const float* w,
                           int64_t E, int64_t N, float fill_value, int add_self_loops,
                           int normalize, int degree_side,
                           int32_t* rowptr, int32_t* colidx, float* val,
                           int32_t* t_rowptr, int32_t* t_colidx, float* t_val, int32_t* t_to_fwd,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* Expand a CSR back to the COO edge_index the reference returns from gcn_norm, in
 * CSR order; nnz_cap >= rowptr[N] bounds the launch (entries past rowptr[N] untouched). */
int gda_csr_to_coo(const int32_t* rowptr, const int32_t* colidx, int64_t N, int64_t nnz_cap,
                   int64_t* src_out, int64_t* dst_out, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Neighbour aggregation  y = A_hat * x  (CSR SpMM, fp32).
 *
 * Replaces MessagePassing.propagate + message + scatter-add aggregate
 * (pygda/nn/prop_gcn_conv.py:208-210,238; pygda/nn/cached_gcn_conv.py:138,156):
 *   y[i,:] = sum_{k in rowptr[i]..rowptr[i+1]} val[k] * x[colidx[k],:]   (+ bias)
 * accumulated in CSR (= edge) order with separately rounded multiply and add, i.e.
 * the CPU result bit for bit for rows processed by one lane group.
 * `bias` ([d], may be NULL) is added once to the final output (prop_gcn_conv.py:212-213,
 * cached_gcn_conv.py:172-174).  y must not alias x.
 *
 * gda_spmm_csr_kstep_f32 applies the operator K>=1 times (the prop_nums loop
 * prop_gcn_conv.py:208-210) ping-ponging between y and tmp ([n_rows, ldy], needed
 * when K>1); x is left intact.  The backward of K steps is the same call on the
 * by-source CSR with the incoming gradient.
 * ---------------------------------------------------------------------------- */
/* Optional load balancing for power-law graphs: rows with more than `threshold` entries are
 * processed as chunks of `threshold` entries (partials in `scratch [n_chunks, d]`, then an
 * ordered per-row reduce).  Built once per graph by gda_row_split_build; all pointers device. */
typedef struct gda_row_split {
    int32_t threshold;
    int32_t n_long, n_chunks;
    const int32_t* long_rows;       /* [n_long]     */
    const int32_t* long_chunk_ptr;  /* [n_long + 1] */
    const int32_t* chunk_long;      /* [n_chunks]   */
    float* scratch;                 /* [n_chunks, d] caller-owned, reused across calls */
    const int32_t* counts_dev;      /* NULL, or the device {n_long, n_chunks} written by gda_row_split_build:
                                       n_long / n_chunks above then hold the CAPACITIES (grid bounds) and
                                       the kernels read the live counts themselves -- no host read-back,
                                       for graphs that live one step (sampled mini-batches) */
} gda_row_split;

/* Find the long rows of a CSR and lay out their chunks.  Outputs must hold the upper bounds
 * cap_long = nnz_cap/threshold + 1 and cap_chunks = 2*nnz_cap/threshold + 2 entries;
 * counts_out [2] (device) receives {n_long, n_chunks}: the one data-dependent pair the host
 * reads back, once per graph. */
size_t gda_row_split_workspace_bytes(int64_t n_rows);
int gda_row_split_build(const int32_t* rowptr, int64_t n_rows, int32_t threshold,
                        int32_t* long_rows, int32_t* long_chunk_ptr, int32_t* chunk_long,
                        int32_t* counts_out, void* workspace, size_t workspace_bytes,
                        gda_stream_t stream);

/* K-step aggregation with optional row splitting (split may be NULL). */
int gda_spmm_csr_split_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                           int64_t n_rows, int64_t d, int K, const float* x, int64_t ldx,
                           float* y, int64_t ldy, float* tmp, const float* bias,
                           const gda_row_split* split, gda_stream_t stream);

int gda_spmm_csr_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                     int64_t n_rows, int64_t d, const float* x, int64_t ldx,
                     float* y, int64_t ldy, const float* bias, gda_stream_t stream);
int gda_spmm_csr_kstep_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                           int64_t n_rows, int64_t d, int K, const float* x, int64_t ldx,
                           float* y, int64_t ldy, float* tmp, const float* bias,
                           gda_stream_t stream);
/* One step with the result written TRANSPOSED: yT[c * ldyT + i] = (A x)[i][c] (+ bias[c]), ldyT >= n_rows -- the same
 * row walk and sums as gda_spmm_csr_f32 (no hub-row split: callers with rows beyond the split threshold use
 * gda_spmm_csr_split_f32 + gda_transpose_f32).  The projection of sparse input features (pygda/nn/prop_gcn_conv.py:205
 * on a bag-of-words matrix) hands its result to gda_kstep_lds_colmajor_f32 in that kernel's own layout. */
int gda_spmm_csr_tout_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                          int64_t n_rows, int64_t d, const float* x, int64_t ldx,
                          float* yT, int64_t ldyT, const float* bias, gda_stream_t stream);

/* K aggregation steps on a sampled sub-graph (a NeighborLoader batch, pygda/models/a2gnn.py:260-277, numbered seeds
 * first then in discovery order): the nodes found in the last hop are never expanded, so rows [n_int, n_rows) of the
 * normalised adjacency hold their unit self loop only and K steps leave them unchanged.  Only rows [0, n_int) are
 * recomputed per step (transposed = 0: leaf columns are read from x; same values as gda_spmm_csr_kstep_f32, signed
 * zeros aside); the transposed operator (backward) runs its K steps on the interior rows, sums their inputs in `sacc`
 * and finishes the leaves in one pass, y_L = x_L + A_IL^T (h_0 + ... + h_{K-1}) -- K full steps up to fp32 summation
 * order.  Rows must be short (<= 128 entries: no hub splitting here; sampled batches hold fan-out + 1 per row).
 * x, y: [n_rows, d] contiguous; tmp [n_int, d] (K > 1), sacc [n_int, d] (transposed). */
int gda_spmm_csr_interior_kstep_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                    int64_t n_rows, int64_t n_int, int64_t d, int K, int transposed,
                                    const float* x, float* y, float* tmp, float* sacc, const float* bias,
                                    gda_stream_t stream);

/* The same K steps with ONE launch for the step loop (round 5; csrc/gda_interior.inc): per feature column the interior
 * block (<= gda_interior_max_rows() = 16,384 rows: 1024 seeds at fan-out 15) is a 64 KB vector that stays in the LDS of one workgroup for all K
 * steps,  y_I <- A_II y_I + c  with the leaf columns' contribution c = A_IL x_L formed once; a call is 3 launches forward
 * (c + transposition | step loop | rows back + leaf copy) and 4 transposed, whatever K is, against K + 2 above.
 *   gda_interior_plan_build: compiles ONE direction of the batch's CSR (rowptr / colidx / val = the by-destination arrays
 *     for the forward operator, the by-source arrays for the transposed one) into the step loop's per-lane register
 *     program ON THE DEVICE -- three small capacity-sized launches, typically on the sampler's stream right after
 *     gda_dsampler_sample; n_int_dev = device int64 (the sampler's counts + 4); plan = gda_interior_plan_bytes() device
 *     bytes, 16-byte aligned; status_dev = device int64[2]: [0] <- > 0: the plan is valid (entries per lane), 0: the batch
 *     does not fit (too many interior rows, more than 1024 x 26 off-diagonal interior entries): keep the call above;
 *     [1] <- the number of off-diagonal interior entries.
 *   gda_interior_kstep_lds_f32: x, y [n_rows, d] contiguous, 16-byte aligned; d % 4 == 0, d <= gda_interior_max_width();
 *     workspace = gda_interior_kstep_lds_workspace_bytes(n_int, d) device bytes.  Same sums as the call above with `sacc`
 *     given (bit for bit when the diagonal entry is the last of its row, as in every CSR this library builds). */
int gda_interior_max_rows(void);
int gda_interior_max_width(void);
size_t gda_interior_plan_bytes(void);
size_t gda_interior_kstep_lds_workspace_bytes(int64_t n_int, int64_t d);
int gda_interior_plan_build(const int32_t* rowptr, const int32_t* colidx, const float* val,
                            const int64_t* n_int_dev, void* plan, size_t plan_bytes, int64_t* status_dev,
                            gda_stream_t stream);
int gda_interior_kstep_lds_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                               int64_t n_rows, int64_t n_int, int64_t d, int K, int transposed,
                               const void* plan, const float* x, float* y, const float* bias,
                               void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The forward call with the conv layer's activation (pygda/nn/a2gnn_base.py:135-138: relu, then inverted dropout) in its
 * epilogue: y0 = dropout_{site0}(relu(A^K x + bias)); y1 (may be NULL) = dropout_{site1}(relu(the same values)) -- a second,
 * independent draw for the trainer's second pass over a shared layer-0 output.  The values gda_relu_dropout_fwd_f32 would
 * produce from gda_interior_kstep_lds_f32's result with the same (seed, step, site); the pre-activation is not stored
 * (gda_relu_dropout_bwd_f32 needs y > 0 only).  p <= 0: relu only. */
int gda_interior_kstep_lds_act_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                   int64_t n_rows, int64_t n_int, int64_t d, int K, const void* plan,
                                   const float* x, float* y0, float* y1, const float* bias,
                                   float p, uint64_t seed, const int64_t* step_dev, uint32_t site0, uint32_t site1,
                                   void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * K-step aggregation in ONE launch for graphs whose feature columns fit a CU's LDS
 * (n_rows <= gda_kstep_max_rows() = 16320; the citation-graph regime), csrc/gda_kstep.hip.
 *
 * Replaces the same prop_nums loop (pygda/nn/prop_gcn_conv.py:208-210) as gda_spmm_csr_kstep_f32,
 * with the same results bit for bit (per-row sums in CSR order, separately rounded multiply and
 * add): A_hat^K x is independent per feature column, so a workgroup keeps one column of all rows in
 * LDS across the K steps and the graph is compiled once into a per-lane register program.
 * On a graph with a row of more than 48 entries (power-law hubs) the rows longer than 4*S entries are cut into
 * segments of 4*S entries whose sequential
 * sums are added as a fixed balanced tree by a second phase of each step: deterministic, within fp32
 * summation tolerance of the sequential order (the rows of up to 4*S entries stay bit-exact).
 *
 * gda_kstep_plan_host compiles a CSR given as HOST arrays into `plan_host` (caller-owned host
 * memory of gda_kstep_plan_bytes(12) bytes; the first gda_kstep_plan_bytes(slots) are meaningful) and
 * returns `slots` = S | hub_waves << 8 (S = 6, 8, 10 or 12 slots per thread; hub_waves = 0 for a graph
 * without long rows) -- the value the launch entry points take --, 0 when the graph is not eligible (too
 * many rows / a row longer than 64 segments / more slots than one workgroup holds / nodes + segments beyond
 * the 16320 words of an LDS buffer) -- callers then use gda_spmm_csr_kstep_f32 --, or a negative status.
 * The plan is copied to the device by the caller.
 * gda_kstep_plan_host_ex takes flags: bit 0 = bank-aware placement -- WHERE a node's word lives in LDS is
 * chosen such that the 32 words a lane group gathers (or stores) in one instruction fall on different LDS
 * banks as far as possible (the step loop is bound by exactly those gathers); the sums and their order do
 * not change.  gda_kstep_plan_host = flags 1.
 *
 * gda_kstep_lds_f32: K >= 1 steps; x is row-major [n_rows, ldx] (x_colmajor = 0) or column-major
 * [d, ldx] (x_colmajor = 1: ldx >= round_up(n_rows, 4), 16-byte aligned columns), y likewise; bias ([d] or
 * NULL) is added once at the end; colsum ([d] or NULL) receives the column sums of the INPUT over the
 * real rows in a fixed order (the bias gradient when the call is the backward pass of the layer);
 * scratchT holds 2 * d * round_up(n_rows, 4) floats for the transposes of row-major operands.
 * gda_kstep_lds_colmajor_f32: the kernel alone on column-major operands, K >= 0.
 * gda_transpose_f32: out [cols, ldo] = in [rows, ldi]^T.
 * ---------------------------------------------------------------------------- */
int gda_kstep_max_rows(void);
size_t gda_kstep_plan_bytes(int slots);
int gda_kstep_plan_host(const int32_t* rowptr_host, const int32_t* colidx_host, const float* val_host,
                        int64_t n_rows, void* plan_host, size_t plan_bytes);
int gda_kstep_plan_host_ex(const int32_t* rowptr_host, const int32_t* colidx_host, const float* val_host,
                           int64_t n_rows, int flags, void* plan_host, size_t plan_bytes);
int gda_kstep_lds_f32(const void* plan, int slots, int64_t n_rows, int64_t d, int K,
                      const float* x, int64_t ldx, int x_colmajor, float* y, int64_t ldy, int y_colmajor,
                      const float* bias, float* colsum, float* scratchT, gda_stream_t stream);
int gda_kstep_lds_colmajor_f32(const void* plan, int slots, int64_t n_rows, int64_t d, int K,
                               const float* xT, int64_t ldx, float* yT, int64_t ldy,
                               const float* bias, float* colsum, gda_stream_t stream);
int gda_transpose_f32(const float* in, int64_t ldi, float* out, int64_t ldo, int64_t rows, int64_t cols,
                      gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * GAT aggregation (single head): edge-softmax attention + weighted neighbour sum, fused.
 *
 * Replaces PyG GATConv(heads=1, concat=False) as GNNBase(gnn='gat') uses it
 * (pygda/nn/gnn_base.py:80-87): for destination i over its incoming edges k (self loop
 * included by the ingestion),  e_k = LeakyReLU_slope(a_src[col_k] + a_dst[i]),
 * alpha = softmax_k(e),  out[i,:] = sum_k alpha_k h[col_k,:].   h = x W^T and the two
 * attention logits a_src = h.att_src, a_dst = h.att_dst are formed by the caller (dense).
 *   forward : out [N,d]; alpha [nnz] (by-destination order, kept for backward)
 *   backward: given gout [N,d] ->  gh [N,d] (the aggregation path only), ga_src [N], ga_dst [N];
 *             the caller adds the dense chain  gh += ga_src att_src + ga_dst att_dst.
 *             needs the by-source CSR and t_to_fwd from gda_build_csr_norm_map;
 *             dpre [nnz] is caller-owned scratch.
 * ---------------------------------------------------------------------------- */
int gda_gat_fwd_f32(const int32_t* rowptr, const int32_t* colidx, int64_t n_rows, int64_t d,
                    const float* h, const float* a_src, const float* a_dst, float slope,
                    float* out, float* alpha, gda_stream_t stream);
int gda_gat_bwd_f32(const int32_t* rowptr, const int32_t* colidx,
                    const int32_t* t_rowptr, const int32_t* t_colidx, const int32_t* t_to_fwd,
                    int64_t n_rows, int64_t d, const float* h, const float* a_src, const float* a_dst,
                    float slope, const float* alpha, const float* gout,
                    float* gh, float* ga_src, float* ga_dst, float* dpre, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * FAConv aggregation: tanh-gated, GCN-normalised neighbour sum, fused.
 *
 * Replaces PyG FAConv(channels, eps=0.1) as SAGDA's SAGNN layer calls it, conv(x, x, edge_index) then
 * torch.mm(., W) + b (pygda/nn/sagda_base.py:50,87-88).  PyG semantics (tests/golden/_faconv_semantics.py):
 * gcn_norm with remaining self loops (fill 1) and the degree over the destination, recomputed per call;
 * message x_j * (tanh(att_l.x_j + att_r.x_i) * w_ij), summed in edge order; then out += eps * x_0.
 * The layer is linear in x, so it runs reassociated on the caller's projection [h | s | r] = x [W | att_l^T |
 * att_r^T]: for destination i over its CSR entries k (by-destination CSR of gda_build_csr_norm_map, degree
 * side "col"),
 *   t_k = tanh(s[col_k] + r[i]),  c_k = t_k * w_k,  out[i,:] = sum_k c_k h[col_k,:] + eps h[i,:] + bias
 *   forward : out [N, ldo]; t [nnz] (by-destination order, kept for backward); bias [d] may be NULL.
 *   backward: given gout [N, ldgo] -> gh [N, ldgh] = A_att^T gout + eps gout,  gs [N], gr [N] (the gradients
 *             of the two logits); dc_k = gout_i . h[col_k], dpre_k = dc_k w_k (1 - t_k^2),
 *             gr[i] = sum_k dpre_k, gs[j] = sum over entries with source j of dpre.  Needs the by-source CSR
 *             and t_to_fwd; dpre [nnz] is caller-owned scratch.  The bias gradient is the caller's.
 * Any d >= 1.  Row strides: h and the gradient gh take ldh / ldgh >= d; s, r and gs, gr take ldsr / ldgsr >= 1,
 * so that h, s, r (and gh, gs, gr) may be column views of one [N, d + 2] matrix.  Multiply and add are rounded
 * separately, sums are sequential in CSR order (deterministic, no atomics).  out must not alias h; gh must not
 * alias h or gout (GDA_E_ALIAS).
 * ---------------------------------------------------------------------------- */
int gda_faconv_fwd_f32(const int32_t* rowptr, const int32_t* colidx, const float* val, int64_t n_rows, int64_t d,
                       const float* h, int64_t ldh, const float* s, const float* r, int64_t ldsr, float eps,
                       const float* bias, float* out, int64_t ldo, float* t, gda_stream_t stream);
int gda_faconv_bwd_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                       const int32_t* t_rowptr, const int32_t* t_colidx, const int32_t* t_to_fwd,
                       int64_t n_rows, int64_t d, const float* h, int64_t ldh, const float* t,
                       const float* gout, int64_t ldgo, float eps, float* gh, int64_t ldgh, float* gs,
                       float* gr, int64_t ldgsr, float* dpre, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * CWGCN's losses (pygda/nn/cwgcn_base.py:193-219, pygda/models/cwgcn.py:306-350,423-458), fused.
 *
 * Correntropy-induced loss over logits z [n, c] (row stride ldz >= c) and int64 labels y [n]:
 *   d_i = sum_k (z_ik - onehot(y_i)_k)^2,  loss = mean_i (1 - exp(-d_i / 100)),  weight_i = exp(-d_i / 10),
 *   factor_i = exp(-d_i / 100) (kept for the backward).  loss is a device scalar; the mean is a two-stage sum in a
 *   fixed order (one launch when one workgroup covers the rows).  A label outside [0, c) matches no column.
 *   backward: gz [n, ldgz] = g (2 / (100 n)) factor_i (z - onehot), g = *gloss read on the device.
 * Weighted column moments of x [n, d] (ldx >= d) under w [n] (get_src_mean_std):
 *   w' = w / sum w;  mean = sum w' x;  std = sqrt(sum w' (x - mean)^2 / (1 - sum w'^2)).
 * Column mean / std matching against given mean_s [d], std_s [d] (torch.std_mean, unbiased):
 *   loss = sum_j (mean_s - mean_t)^2 + sum_j (std_s - std_t)^2;  mean_t, std_t [d] are written, and coef [2 d]
 *   for the backward:  gx [n, ldgx] = g (coef[j] + coef[d + j] (x - mean_t)),  coef[j] = -2 (mean_s - mean_t) / n,
 *   coef[d + j] = -2 (std_s - std_t) / ((n - 1) std_t), 0 where std_t == 0 (torch masks that gradient); n = 1 gives
 *   NaN as torch does.
 * The column statistics are slab partials (weight, mean, M2 per slab and column, merged pairwise in a fixed order).
 * 1 <= n < 2^31, 1 <= d <= 2^22; workspace from gda_closs_workspace_bytes / gda_colstats_workspace_bytes (both
 * statistics entries take the same size).  Deterministic, no atomics, no allocation or synchronisation.
 * ---------------------------------------------------------------------------- */
size_t gda_closs_workspace_bytes(int64_t n, int64_t c);
int gda_closs_fwd_f32(const float* z, int64_t ldz, const int64_t* y, int64_t n, int64_t c, float* loss, float* weight,
                      float* factor, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_closs_bwd_f32(const float* z, int64_t ldz, const int64_t* y, const float* factor, const float* gloss,
                      int64_t n, int64_t c, float* gz, int64_t ldgz, gda_stream_t stream);
size_t gda_colstats_workspace_bytes(int64_t n, int64_t d);
int gda_weighted_moments_f32(const float* x, int64_t ldx, const float* w, int64_t n, int64_t d, float* mean,
                             float* std, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_std_mean_match_fwd_f32(const float* x, int64_t ldx, int64_t n, int64_t d, const float* mean_s,
                               const float* std_s, float* loss, float* mean_t, float* std_t, float* coef,
                               void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_std_mean_match_bwd_f32(const float* x, int64_t ldx, int64_t n, int64_t d, const float* mean_t,
                               const float* coef, const float* gloss, float* gx, int64_t ldgx, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * ACDNE (pygda/models/acdne.py, pygda/nn/acdne_base.py).
 *
 * process_graph's PPMI on dense fp32 N x N buffers of leading dimension ld = round_up(N, 4) (the padding columns are
 * scratch).  The adjacency is a coalesced CSR by source row: rowptr [N + 1], col [nnz] (no duplicates), cnt [nnz] the
 * edge multiplicities.  gda_acdne_ppmi_f32 forms P = D^-1 A (1 / (deg + 1e-12)) into pval [nnz], a = sum_{k<=step}
 * P^k / k into buf_a, then A_ppmi (diagonal zeroed, rows normalised, max(log(N a / colsum + 1e-12), 0), colsum 0 -> 1)
 * in buf_a and its row-normalised copy in buf_b.  buf_c is needed for step >= 3 only.  Workspace from
 * gda_acdne_ppmi_workspace_bytes.
 * gda_acdne_xnei_f32: out [N, f] (ldo) = na [N, N] (ld) @ X, X as a row-major CSR (xrowptr [N + 1], xcol, xval),
 * f <= 40960.
 * Per step (2h rows: h source rows, then h target rows; 1 <= h <= GDA_ACDNE_MAX_HALF):
 * gda_acdne_prox_f32: for each domain the h x h block of its A_ppmi at pidx (source: pidx[0..h), target:
 *   pidx[h..2h)), zero diagonal, rows scaled by 1 / (fp32(double row sum) + 1e-12) in double; loss[dom] =
 *   mean_i sum_j a_ij (r_i + r_j - 2 e_i.e_j) with e = relu(z); gz [2h, e] = pair_weight * its gradient in e.
 *   An index outside the domain reads zero.  Workspace from gda_acdne_prox_workspace_bytes.
 * gda_acdne_heads_f32: w = {Wc [c, e], bc, W1 [128, e], b1, W2 [128, 128], b2, W3 [2, 128], b3}, g the same shapes
 *   (overwritten).  emb = relu(z); clf = CE(emb Wc^T + bc, y[rows[i]]) over the first h rows; dom = CE(disc(emb),
 *   0 for the first h rows, 1 for the rest); loss = clf + fp32(dom) + pair_weight (prox[0] + prox[1]) in double,
 *   loss_acc (optional) += loss.  dz = (dlogits Wc - alpha ddisc W1 + gprox) * (z > 0); alpha is a device scalar.
 *   A label outside [0, c) matches no column.  One kernel and one workspace layout with gda_dmgnn_heads_f32 (below):
 *   this entry point runs it without a block, L' = L; gda_acdne_heads_workspace_bytes equals
 *   gda_dmgnn_heads_workspace_bytes.
 * gda_acdne_predict_f32: prob [n, c] = softmax(relu(z) Wc^T + bc).
 * Deterministic, no atomics, no allocation or synchronisation.
 * ---------------------------------------------------------------------------- */
#define GDA_ACDNE_MAX_HALF 128
size_t gda_acdne_ppmi_workspace_bytes(int64_t n);
int gda_acdne_ppmi_f32(const int32_t* rowptr, const int32_t* col, const float* cnt, int64_t n, int step, float* pval,
                       float* buf_a, float* buf_b, float* buf_c, void* workspace, size_t workspace_bytes,
                       gda_stream_t stream);
int gda_acdne_xnei_f32(const float* na, int64_t n, int64_t ld, const int32_t* xrowptr, const int32_t* xcol,
                       const float* xval, int64_t f, float* out, int64_t ldo, gda_stream_t stream);
size_t gda_acdne_prox_workspace_bytes(int64_t h);
int gda_acdne_prox_f32(const float* ppmi_s, int64_t ld_s, int64_t ns, const float* ppmi_t, int64_t ld_t, int64_t nt,
                       const int64_t* pidx, const float* z, int64_t h, int64_t e, float pair_weight, double* loss,
                       float* gz, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_acdne_heads_workspace_bytes(int64_t h, int64_t e, int64_t c);
int gda_acdne_heads_f32(const float* z, const float* gprox, int64_t h, int64_t e, int64_t c, const float* const* w,
                        const int64_t* y, int64_t ny, const int64_t* rows, const float* alpha, const double* prox,
                        float pair_weight, float* dz, float* const* g, double* loss, double* loss_acc,
                        void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_acdne_predict_f32(const float* z, int64_t n, int64_t e, const float* wc, const float* bc, int64_t c,
                          float* prob, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * DMGNN (pygda/models/dmgnn.py on pygda/nn/acdne_base.py).  process_graph and the network are ACDNE's; the layout is
 * the same: dense fp32 PPMI of leading dimension ld, pidx per domain, an index outside the domain reads zero,
 * 1 <= h <= GDA_ACDNE_MAX_HALF, e and c up to 4096.
 * gda_dmgnn_prox_f32: for each domain the h x h block of its A_ppmi at pidx, zero diagonal, rows scaled by
 *   1 / (fp32(double row sum) + 1e-12) (the block of gda_acdne_prox_f32, rounded to fp32), written to a_blocks
 *   [2, h, h].  With E = relu(z) and D = E - A E: loss[dom] = |D|_F / h (nei_prox_loss, the square sum in double),
 *   gz [2h, e] = pair_weight (D - A^T D) / (h |D|_F), zero where |D|_F = 0.  One launch.  Workspace from
 *   gda_dmgnn_prox_workspace_bytes.
 * gda_dmgnn_heads_f32: gda_acdne_heads_f32's kernel with the classifier logits propagated: L = emb Wc^T + bc,
 *   L' = L + A_s L over the first h rows (A_s = a_blocks[0]), clf = CE(L', y[rows[i]]); backward dL = dL' + A_s^T dL'.
 *   The domain branch, alpha, loss and loss_acc as in gda_acdne_heads_f32.  The target half's propagated logits enter
 *   no loss and are not formed.  Workspace from gda_dmgnn_heads_workspace_bytes.
 * gda_dmgnn_predict_f32: out [n, c] = P + M P with P = softmax(relu(z) Wc^T + bc) and M = ppmi [n, n] (ld): P into
 *   the workspace (gda_dmgnn_predict_workspace_bytes) by gda_acdne_predict_f32, then one pass over M with 16-byte
 *   loads -- ld % 4 == 0 and a 16-byte aligned ppmi, else GDA_E_UNSUPPORTED; the columns n..ld of M are never used.
 * Deterministic, no atomics, no allocation or synchronisation.
 * ---------------------------------------------------------------------------- */
size_t gda_dmgnn_prox_workspace_bytes(int64_t h, int64_t e);
int gda_dmgnn_prox_f32(const float* ppmi_s, int64_t ld_s, int64_t ns, const float* ppmi_t, int64_t ld_t, int64_t nt,
                       const int64_t* pidx, const float* z, int64_t h, int64_t e, float pair_weight, double* loss,
                       float* gz, float* a_blocks, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_dmgnn_heads_workspace_bytes(int64_t h, int64_t e, int64_t c);
int gda_dmgnn_heads_f32(const float* z, const float* gprox, const float* a_blocks, int64_t h, int64_t e, int64_t c,
                        const float* const* w, const int64_t* y, int64_t ny, const int64_t* rows, const float* alpha,
                        const double* prox, float pair_weight, float* dz, float* const* g, double* loss,
                        double* loss_acc, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_dmgnn_predict_workspace_bytes(int64_t n, int64_t c);
int gda_dmgnn_predict_f32(const float* z, int64_t n, int64_t e, const float* wc, const float* bc, int64_t c,
                          const float* ppmi, int64_t ld, float* out, void* workspace, size_t workspace_bytes,
                          gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Multi-kernel Gaussian MMD over sampled rows, forward and backward, with no
 * [n,n,d] temporary.
 *
 * Replaces MMD / get_MMD / guassian_kernel (pygda/utils/mmd.py:4-159) as called from
 * A2GNN.forward_model (pygda/models/a2gnn.py:208) and GRADE (pygda/models/grade.py:182).
 * For each of `times` resamples t: rows r<n of `total` are src[src_idx[t,r]], rows
 * n<=r<2n are tgt[tgt_idx[t,r-n]] (idx NULL = the rows as given, stacked [times, n, d] per
 * domain; times = 1 is get_MMD).  L2[i,j] = sum_k (total[j,k]-total[i,k])^2 (direct
 * difference form, mmd.py:43-46); bandwidth = (sum L2 + 1e-6)/(m^2-m) / kernel_mul^(kernel_num/2),
 * m = 2n (mmd.py:50-51; fix_sigma>0 overrides the data-dependent value); K = sum_q
 * exp(-L2/(bandwidth*kernel_mul^q)) (mmd.py:52-55); loss_t = mean(XX+YY-XY-YX) over the
 * n x n blocks (mmd.py:100-106); loss = (sum_t loss_t)/times (mmd.py:152-157).
 * The reference's block arithmetic needs equally many source and target rows; so does this.
 *
 *   loss        [1] fp32 (device)
 *   bandwidth   [times] fp32 (device, saved for backward; gradient does not flow
 *               through it -- mmd.py:50 uses .data)
 *   l2_saved    [times, 2n, 2n] fp32 (device; produced by fwd, consumed by bwd -- on return it
 *               holds d K / d L2 with the block signs applied, not the distances themselves;
 *               opaque to the caller)
 * Backward: grad_rows [times, 2n, d] = d loss / d total rows, scaled by *grad_loss.
 * The caller scatters them onto feature rows (a CSR SpMM with the selection matrix).
 * ---------------------------------------------------------------------------- */
size_t gda_mmd_workspace_bytes(int times, int64_t n, int64_t d);
int gda_mmd_fwd_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                    int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                    int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                    float* loss, float* bandwidth, float* l2_saved,
                    void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mmd_bwd_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                    int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                    int times, int64_t n, float kernel_mul, int kernel_num,
                    const float* bandwidth, const float* l2_saved, const float* grad_loss,
                    float* grad_rows, void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The same two calls with the glue of the trainer's loss line folded in (`loss = CE + MMD(...) * weight`,
 * pygda/models/a2gnn.py:207-209): forward returns add[0] + scale * mmd (add may be NULL); backward scales the
 * incoming gradient by `scale`, and -- given the 0/1 selection CSRs of the sampled rows (rows = feature rows of a
 * domain, columns = positions t*2n + i of the [times, 2n, d] row-gradient array: gda_selection_csr_host) -- sums the
 * row gradients straight onto the feature rows: gsrc [n_src_rows, d], gtgt [n_tgt_rows, d] (grad_rows unused then;
 * the same values as grad_rows followed by the selection-matrix SpMM, bit for bit). */
int gda_mmd_fwd_ex_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                       int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                       int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                       float scale, const float* add, float* loss, float* bandwidth, float* l2_saved,
                       void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* _gather: with row indices, rows_src / rows_tgt ([times*n, d] each, both or neither) receive the sampled rows
 * (`source_feat[source_samples]` mmd.py:153-154) as a by-product of the statistics pass, and the later kernels --
 * and the backward call, which is then handed these buffers without indices -- read them instead of chasing the
 * index again: no separate gather launches. */
int gda_mmd_fwd_gather_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                           int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                           int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                           float scale, const float* add, float* rows_src, float* rows_tgt,
                           float* loss, float* bandwidth, float* l2_saved,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mmd_bwd_ex_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                       int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                       int times, int64_t n, float kernel_mul, int kernel_num,
                       const float* bandwidth, const float* l2_saved, const float* grad_loss, float scale,
                       float* grad_rows,
                       const int32_t* sel_s_rowptr, const int32_t* sel_s_col, int64_t n_src_rows, float* gsrc,
                       const int32_t* sel_t_rowptr, const int32_t* sel_t_col, int64_t n_tgt_rows, float* gtgt,
                       void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* The same loss and gradients in ONE pass over the row pairs (round 4): the kernel weights d K / d L2 are consumed where
 * they are produced -- multiplied into the rows on the 16-bit matrix cores -- instead of travelling through a
 * [times, 2n, 2n] matrix.  Both products run on fp16 MFMAs with SPLIT operands (a = hi + lo, three products per pair,
 * fp32 accumulation: 22 significant bits per operand, an error of the order of an fp32 sum in another order; the rows
 * are scaled by one power of two per resample first, so fp16's exponent range never matters).  Covered:
 * kernel_num = 5 with kernel_mul = 2 (every pygda call: mmd.py:57-63 defaults), d in {32, 64, 96, 128}, rows on
 * 16-byte boundaries; gda_mmd_fused_nseg() returns 0 for anything else (use gda_mmd_fwd_gather_f32 / gda_mmd_bwd_ex_f32).
 *   grad_part   [times, nseg, 2n, d] fp32 (device; nseg = gda_mmd_fused_nseg(...)): UNSCALED row-gradient partials,
 *               produced by fwd, consumed by bwd (which multiplies by 4 * grad_loss * scale / (n^2 times), folds the
 *               segments in order and, given the selection CSRs, scatters onto the feature rows).  Opaque.
 *   workspace   gda_mmd_workspace_bytes(times, n, d) bytes, as for the two-pass calls
 * src_idx / tgt_idx need rows_src / rows_tgt (the gathered copy) here. */
int gda_mmd_fused_nseg(int times, int64_t n, int64_t d, float kernel_mul, int kernel_num);
/* Host arithmetic only (no device): what the fused pass lays out for (times, n, d), for tests and debuggers.
 *   out[16] = { nb, ntiles, njb, nseg, workgroups, image bytes,
 *               image offsets: rows lo, columns hi, columns lo, norms; float index of the tile scale in the norm block,
 *               floats reserved for that block (32 norms + scale);
 *               workspace offsets: images, part_max, kpartial; workspace bytes }
 * GDA_E_UNSUPPORTED when gda_mmd_fused_nseg() would return 0. */
int gda_mmd_fused_layout(int times, int64_t n, int64_t d, int64_t* out, int n_out);
int gda_mmd_fused_fwd_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                          int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                          int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                          float scale, const float* add, float* rows_src, float* rows_tgt,
                          float* loss, float* bandwidth, float* grad_part, int nseg,
                          void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mmd_fused_bwd_f32(const float* grad_part, int nseg, int times, int64_t n, int64_t d,
                          const float* grad_loss, float scale, float* grad_rows,
                          const int32_t* sel_s_rowptr, const int32_t* sel_s_col, int64_t n_src_rows, float* gsrc,
                          const int32_t* sel_t_rowptr, const int32_t* sel_t_col, int64_t n_tgt_rows, float* gtgt,
                          gda_stream_t stream);
/* _mask: mask_src / mask_tgt (either may be NULL) = the OUTPUT y [n_*_rows, d] of the activation dropout(relu(.), p_*) that
 * produced that domain's feature rows: the scattered row gradient is stored as y > 0 ? g / (1 - p) : 0, i.e. already
 * through that activation's backward (gda_relu_dropout_bwd_f32's values) -- its launch and one [rows, d] round trip
 * disappear.  Scatter form only (selection CSRs given). */
int gda_mmd_fused_bwd_mask_f32(const float* grad_part, int nseg, int times, int64_t n, int64_t d,
                               const float* grad_loss, float scale, float* grad_rows,
                               const int32_t* sel_s_rowptr, const int32_t* sel_s_col, int64_t n_src_rows, float* gsrc,
                               const int32_t* sel_t_rowptr, const int32_t* sel_t_col, int64_t n_tgt_rows, float* gtgt,
                               const float* mask_src, float p_src, const float* mask_tgt, float p_tgt,
                               gda_stream_t stream);
/* The same pass for target features that are dropout(relu(.)) of a COLUMN-MAJOR pre-activation tgtT [d, ldT] (the K-step
 * kernel's layout; n_tgt_rows feature rows, ldT >= n_tgt_rows, ldT % 4 == 0) which nothing but this loss reads: the pass
 * applies the activation while it gathers the sampled rows -- the values and the kept set of gda_relu_dropout_fwd_cm_f32
 * called with the same (p, seed, step, site); `step` is read on the device -- and the backward call writes the gradient of
 * the PRE-ACTIVATION, column-major gxT [d, ldT], from the same single scatter launch: sign from tgtT, keep-bit drawn again,
 * rows nobody sampled and the columns n_tgt_rows..ldT exact zeros (tgtT's own padding columns are never read).  The
 * row-major activation and the two launches that wrote and unwound it do not exist.  Same bits as the composition.
 * Envelope: gda_mmd_fused_nseg() != 0, no fix_sigma, src_idx / tgt_idx and rows_src / rows_tgt given, the selection CSRs
 * given (bwd), nseg 1..8, every array 16-byte aligned, ld_src % 4 == 0; GDA_E_UNSUPPORTED outside it.  mask_src / p_src as
 * in gda_mmd_fused_bwd_mask_f32 (may be NULL). */
int gda_mmd_fused_fwd_act_cm_f32(const float* src, int64_t ld_src, const float* tgtT, int64_t ldT, int64_t n_tgt_rows,
                                 int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                                 int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                                 float scale, const float* add, float* rows_src, float* rows_tgt,
                                 float* loss, float* bandwidth, float* grad_part, int nseg,
                                 float p, uint64_t seed, const int64_t* step, uint32_t site,
                                 void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mmd_fused_bwd_act_cm_f32(const float* grad_part, int nseg, int times, int64_t n, int64_t d,
                                 const float* grad_loss, float scale,
                                 const int32_t* sel_s_rowptr, const int32_t* sel_s_col, int64_t n_src_rows, float* gsrc,
                                 const int32_t* sel_t_rowptr, const int32_t* sel_t_col, int64_t n_tgt_rows,
                                 const float* tgtT, float* gxT, int64_t ldT,
                                 float p, uint64_t seed, const int64_t* step, uint32_t site,
                                 const float* mask_src, float p_src, gda_stream_t stream);

/* The one-pass MMD for ANY feature width d <= 1024 (round 6; pygda/models/grade.py:177-182 calls MMD() on 645-wide rows):
 * the feature dimension is cut into chunks of 32 | 64 | 96 | 128 columns -- the chunk width that pads d least --, a
 * workgroup keeps the 32 x 32 distance blocks of up to eight row tiles in accumulators over all chunks, takes the
 * exponentials once, and forms the gradient chunk by chunk (csrc/gda_mmd_chunked.inc).  Rows of any alignment; same
 * split-fp16 arithmetic and the same error class as gda_mmd_fused_fwd_f32.  kernel_num = 5, kernel_mul = 2, n <= 1024.
 *   gda_mmd_chunked_plan   host arithmetic only: out[8] = { nseg, padded width dp, nb (32-column blocks per chunk), nc
 *                          (chunks), ntiles, njb, workgroups, image bytes }; GDA_E_UNSUPPORTED outside the envelope
 *   rows_src / rows_tgt    [times * n, ld_rows] fp32 scratch, ld_rows = dp, 16-byte aligned: the gathered (src_idx given)
 *                          or copied (NULL: rows stacked [times, n, d]) rows, zero padded -- REQUIRED
 *   grad_part              [times, nseg, 2n, ld_part] fp32, ld_part = dp: unscaled row-gradient partials for
 *                          gda_mmd_fused_bwd_ld_f32 (= gda_mmd_fused_bwd_mask_f32 with the partials' row stride)
 *   workspace              gda_mmd_chunked_workspace_bytes(times, n, d) */
int gda_mmd_chunked_plan(int times, int64_t n, int64_t d, float kernel_mul, int kernel_num, int64_t* out, int n_out);
size_t gda_mmd_chunked_workspace_bytes(int times, int64_t n, int64_t d);
int gda_mmd_chunked_fwd_f32(const float* src, int64_t ld_src, const float* tgt, int64_t ld_tgt,
                            int64_t d, const int64_t* src_idx, const int64_t* tgt_idx,
                            int times, int64_t n, float kernel_mul, int kernel_num, float fix_sigma,
                            float scale, const float* add, float* rows_src, float* rows_tgt, int64_t ld_rows,
                            float* loss, float* bandwidth, float* grad_part, int64_t ld_part, int nseg,
                            void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mmd_fused_bwd_ld_f32(const float* grad_part, int64_t ld_part, int nseg, int times, int64_t n, int64_t d,
                             const float* grad_loss, float scale, float* grad_rows,
                             const int32_t* sel_s_rowptr, const int32_t* sel_s_col, int64_t n_src_rows, float* gsrc,
                             const int32_t* sel_t_rowptr, const int32_t* sel_t_col, int64_t n_tgt_rows, float* gtgt,
                             const float* mask_src, float p_src, const float* mask_tgt, float p_tgt,
                             gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Gradient-reversal + linear domain discriminator + softmax cross-entropy, fused.
 *
 * Replaces GradReverse.apply (pygda/nn/reverse_layer.py:39,65-66) -> Linear(h, C) ->
 * F.cross_entropy over cat(source, target) rows (pygda/models/a2gnn.py:197-205,
 * pygda/models/grade.py:170-176).  Rows [0, n_src) of `feat_src` carry label 0,
 * rows of `feat_tgt` label 1 (C = 2 in the reference; labels may instead be given
 * per row with `labels` != NULL over the concatenation).  Shapes: 2 <= C <= 4,
 * h <= 1024 and C * h <= 3072 (the backward keeps W and four partials of gW in
 * 60 KB of LDS); anything else is GDA_E_UNSUPPORTED in BOTH directions, so a
 * forward call that succeeds has a backward that runs.
 *   forward : loss[0] = mean_r ( logsumexp(z_r) - z_r[label_r] ),  z = f W^T + b
 *             also writes probs [n_src+n_tgt, C] (softmax, saved for backward)
 *   backward: dz = (probs - onehot)/n * grad_loss ; gW [C,h] = dz^T f ; gb [C] = sum dz ;
 *             gfeat = -alpha * dz W   (the reversal), written for both domains.
 * ---------------------------------------------------------------------------- */
int gda_grl_disc_ce_fwd_f32(const float* feat_src, int64_t ld_src, int64_t n_src,
                            const float* feat_tgt, int64_t ld_tgt, int64_t n_tgt,
                            int64_t h, int C, const float* W, const float* b,
                            const int64_t* labels, float* probs, float* loss,
                            void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_grl_disc_ce_bwd_f32(const float* feat_src, int64_t ld_src, int64_t n_src,
                            const float* feat_tgt, int64_t ld_tgt, int64_t n_tgt,
                            int64_t h, int C, const float* W, const int64_t* labels,
                            const float* probs, const float* grad_loss, float alpha,
                            float* gfeat_src, float* gfeat_tgt, float* gW, float* gb,
                            void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_grl_disc_workspace_bytes(int64_t n_rows, int64_t h, int C);

/* ------------------------------------------------------------------------------
 * Gradient-reversal + TWO-LAYER domain discriminator + per-domain softmax cross-entropy, fused
 * (csrc/gda_disc_mlp.hip).  Replaces UDAGCN's domain branch, pygda/models/udagcn.py:176-190 with the
 * discriminator built at pygda/nn/udagcn_base.py:157-162:
 *     D(x) = W2 dropout_p(relu(W1 GradReverse(x) + b1)) + b2,   W1 [a, h], b1 [a], W2 [2, a], b2 [2] (row-major)
 *     losses[0] = mean over the n_s source rows of CE(D(x), 0),  losses[1] = mean over the n_t target rows of CE(D(x), 1),
 *     losses[2] = their sum (what the reference adds to its loss; the two means also come back separately so that a
 *     data-parallel caller can weight them by node counts).  h <= 128, a <= 64.  Dropout keep-bits: Philox keyed on (seed, *step, site + domain, row, unit) --
 * forward and backward regenerate them, nothing of size [rows, a] is stored.
 *   backward: grad_losses = upstream gradients (device): of the two means at [0] and [grad_stride] (grad_stride 1), or
 *             of their sum (grad_stride 0); g_es / g_et (may be NULL) receive
 *             -alpha * dD/dx (the reversal; alpha_dev != NULL: alpha read from the device), gW1 [a, h], gb1 [a],
 *             gW2 [2, a], gb2 [2] the parameter gradients (fixed-order sums: deterministic).
 * ---------------------------------------------------------------------------- */
size_t gda_grl_mlp_ce_workspace_bytes(int64_t h, int64_t a);
int gda_grl_mlp_ce_fwd_f32(const float* es, int64_t ld_s, int64_t n_s, const float* et, int64_t ld_t, int64_t n_t,
                           int64_t h, int64_t a, const float* W1, const float* b1, const float* W2, const float* b2,
                           float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                           float* losses, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_grl_mlp_ce_bwd_f32(const float* es, int64_t ld_s, int64_t n_s, const float* et, int64_t ld_t, int64_t n_t,
                           int64_t h, int64_t a, const float* W1, const float* b1, const float* W2, const float* b2,
                           float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                           const float* grad_losses, int grad_stride, float alpha, const float* alpha_dev,
                           float* g_es, float* g_et, float* gW1, float* gb1, float* gW2, float* gb2,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The same row kernels with the head given: head = 0 is gda_grl_mlp_ce_*; head = 1 -- ONE logit per row through a sigmoid, the
 * loss term of a domain the MEAN of its rows' sigmoids: losses[0] = mean_s D(x), losses[1] = mean_t D(x), D = Linear(h, a) -
 * ReLU - Dropout(p) - Linear(a, 1) - Sigmoid, i.e. the critic of pygda/models/adagcn.py:264-270 inside the encoder's loss
 * (:190-193, `torch.mean(D(source)) - torch.mean(D(target))`), W2 [1, a], b2 [1], gW2 [1, a], gb2 [1]; no reversal: pass
 * alpha = -1 (the input gradient is multiplied by -alpha). */
int gda_mlp_head_fwd_f32(int head, const float* es, int64_t ld_s, int64_t n_s, const float* et, int64_t ld_t, int64_t n_t,
                         int64_t h, int64_t a, const float* W1, const float* b1, const float* W2, const float* b2,
                         float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                         float* losses, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_mlp_head_bwd_f32(int head, const float* es, int64_t ld_s, int64_t n_s, const float* et, int64_t ld_t, int64_t n_t,
                         int64_t h, int64_t a, const float* W1, const float* b1, const float* W2, const float* b2,
                         float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                         const float* grad_losses, int grad_stride, float alpha, const float* alpha_dev,
                         float* g_es, float* g_et, float* gW1, float* gb1, float* gW2, float* gb2,
                         void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * DANE's LSGAN discriminator head (csrc/gda_disc_mlp.hip).  Replaces what follows the first layer of
 * domain_discriminator = Linear(h, h) - ReLU - Linear(h, 1) (pygda/models/dane.py:241-247) in the LSGAN terms
 * `(pre ** 2).mean()` / `((pre - 1) ** 2).mean()` (dane.py:339-350, 468-470) and their autograd graph, on
 * Z = x W1^T + b1 ([rows, a] fp32, the first layer: a GEMM, gda_gemm_ex_f32):
 *   forward : pre[r] = sum_k relu(Z[r,k]) w2[k] + b2,  loss[0] = mean_r (pre[r] - target)^2
 *   backward: gZ[r,k] = 2 (pre[r] - target) / rows * grad_loss[0] * w2[k] * [Z[r,k] > 0],  gw2 [a], gb2 [1]
 * (gW1, gb1 and the input gradient follow from gZ by gda_gemm_ex_f32).  a <= 256; fixed-order sums.
 * ---------------------------------------------------------------------------- */
size_t gda_lsgan_head_workspace_bytes(int64_t a);
int gda_lsgan_head_fwd_f32(const float* Z, int64_t ldz, int64_t rows, int64_t a, const float* w2, const float* b2,
                           float target, float* pre, float* loss, void* workspace, size_t workspace_bytes,
                           gda_stream_t stream);
int gda_lsgan_head_bwd_f32(const float* Z, int64_t ldz, int64_t rows, int64_t a, const float* w2, const float* pre,
                           float target, const float* grad_loss, float* gZ, int64_t ldg, float* gw2, float* gb2,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Wasserstein critic update with gradient penalty (WGAN-GP), loss and parameter gradients in closed form
 * (csrc/gda_critic.hip).  Replaces the body of AdaGCN's critic loop, pygda/models/adagcn.py:169-183 with
 * gradient_penalty (:387-454), for the critic built at :264-270:
 *     D(x) = sigmoid(w2 . dropout_p(relu(W1 x + b1)) + b2),   W1 [a, h] row-major, b1 [a], w2 [a], b2 [1]
 *     loss = -| mean D(es) - mean D(et) | + gp_weight * mean_i (|| grad_x D(x_i) ||_2 - 1)^2,
 *     x_i over cat(es, et, interpolates),  interpolates_i = et[idx_t[i]] + alpha[i] * (es[idx_s[i]] - et[idx_t[i]])
 * es [n_s, h], et [n_t, h] contiguous; idx_s / idx_t int32 [n_i], alpha [n_i] (the reference draws it from the
 * host generator).  The three critic evaluations (on es, on et, on the penalty rows) draw independent dropout
 * masks from Philox keyed on (seed, step[0], site + {0, 1, 2}); dropout_p = 0 needs no step.  Outputs: loss [1]
 * and the gradients gW1 [a, h], gb1 [a], gw2 [a], gb2 [1] of that loss (deterministic reductions).
 * h <= 256, h % 4 == 0, a <= 64.
 * ---------------------------------------------------------------------------- */
size_t gda_wgan_critic_workspace_bytes(int64_t n_s, int64_t n_t, int64_t n_i, int h, int a);
int gda_wgan_critic_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                        const int32_t* idx_s, const int32_t* idx_t, const float* alpha, int64_t n_i,
                        const float* W1, const float* b1, const float* w2, const float* b2, int a,
                        float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                        float gp_weight, float* loss, float* gW1, float* gb1, float* gw2, float* gb2,
                        void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * ReLU + inverted dropout, fused (the activation after every conv layer:
 * pygda/nn/a2gnn_base.py:135-138, grade_base.py:146-148, gnn_base.py:166-168).
 *   forward : y = (x > 0 && keep) ? x/(1-p) : 0, keep-bits from Philox-4x32-10 keyed on `seed`
 *             with counter (step[0], site, element/4): `step` is a device int64 the trainer
 *             increments once per training step (so hipGraph replays draw fresh masks), `site`
 *             numbers the call sites inside a step.
 *   backward: gx = (y > 0) ? gy/(1-p) : 0   -- needs only the saved output.
 * x, y, gy, gx: n contiguous fp32 values, 16-byte aligned.
 * ---------------------------------------------------------------------------- */
int gda_relu_dropout_fwd_f32(const float* x, float* y, int64_t n, float p, uint64_t seed,
                             const int64_t* step, uint32_t site, gda_stream_t stream);
int gda_relu_dropout_bwd_f32(const float* gy, const float* y, float* gx, int64_t n, float p,
                             gda_stream_t stream);
/* gda_relu_dropout_fwd_f32 of `copies` stacked copies of x [period] (period % 4 == 0) without materialising them:
 * y [copies * period], element i = the activation of x[i % period] with element i's keep-bit -- what
 * `F.dropout(F.relu(x.repeat(copies, 1)), p)` draws.  AdaGCN's critic loop re-encodes both domains `critic_steps` times
 * with an encoder that does not change inside the loop (pygda/models/adagcn.py:169-171): the passes differ by their
 * dropout draws only and run as one stacked pass.  Forward only (the loop runs under no_grad). */
int gda_relu_dropout_tiled_fwd_f32(const float* x, int64_t period, int64_t copies, float* y, float p, uint64_t seed,
                                   const int64_t* step, uint32_t site, gda_stream_t stream);
/* The same activation across a layout change, next to the LDS-resident K-step kernel (which works on
 * column-major activations): forward reads xT [d, ldT] column-major and writes y [n, d] row-major, backward
 * reads gy, y [n, d] row-major and writes gxT [d, ldT] column-major (rows n..ldT-1 of a column untouched) --
 * the transposition rides through LDS tiles, no separate pass.  Same keep-bits as the plain kernels (keyed on
 * the row-major element index); d % 4 == 0. */
int gda_relu_dropout_fwd_cm_f32(const float* xT, int64_t ldT, float* y, int64_t n, int64_t d, float p,
                               uint64_t seed, const int64_t* step, uint32_t site, gda_stream_t stream);
int gda_relu_dropout_bwd_cm_f32(const float* gy, const float* y, float* gxT, int64_t ldT, int64_t n, int64_t d,
                               float p, gda_stream_t stream);

/* Two independent dropout draws of one activation, stacked: y [2n, d], y[i] = drop_a(relu(x[i])),
 * y[n + i] = drop_b(relu(x[i])) -- A2GNN's source feature pass and source logits pass (pygda/models/a2gnn.py:181,192:
 * the same layers on the same input, separate dropout draws) continue as ONE pass over 2n rows.  Backward sums the
 * halves: gx[i] = ((y[i] > 0) gy[i] + (y[n+i] > 0) gy[n+i]) / (1 - p).  d % 4 == 0.
 * gda_stack2_f32: out = [a ; b] of half_elems floats each (a NULL half reads as zeros) -- the gradient of such a
 * pair whose halves went to different consumers (MMD rows / classifier). */
int gda_relu_dropout_pair_fwd_f32(const float* x, float* y, int64_t n, int64_t d, float p, uint64_t seed,
                                  const int64_t* step, uint32_t site_a, uint32_t site_b, gda_stream_t stream);
/* colsum (may be NULL) [d]: column sums of gx as a by-product (the bias gradient of the layer that produced x);
 * needs workspace of gda_relu_dropout_pair_workspace_bytes(d) and d <= 1024. */
size_t gda_relu_dropout_pair_workspace_bytes(int64_t d);
int gda_relu_dropout_pair_bwd_f32(const float* gy, const float* y, float* gx, int64_t n, int64_t d, float p,
                                  float* colsum, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_stack2_f32(const float* a, const float* b, float* out, int64_t half_elems, gda_stream_t stream);
/* The backward of `relu_dropout` followed by a split into halves, in one pass: gx [2 * half_elems] = mask(y) * [ga ; gb]
 * / (1 - p) with mask = (y > 0) -- gda_stack2_f32 and gda_relu_dropout_bwd_f32 without the unmasked stack in between
 * (a NULL half reads as zeros). */
int gda_relu_dropout_bwd2_f32(const float* ga, const float* gb, const float* y, float* gx, int64_t half_elems,
                              float p, gda_stream_t stream);

/* Column sums of a row-major [n, d] matrix (ld = ldx): the bias gradient `gy.sum(0)` of a conv layer
 * (out += self.bias, pygda/nn/prop_gcn_conv.py:212-213) as a deterministic two-stage sum; d <= 1024. */
size_t gda_colsum_workspace_bytes(int64_t n, int64_t d);
int gda_colsum_f32(const float* x, int64_t ldx, int64_t n, int64_t d, float* out, void* workspace,
                   size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Layer epilogue of StruRW's mixup backbone -- replaces the elementwise tail of the three
 * MixUpGCNConv calls per layer in pygda/nn/mixup_base.py:146-196 (out = Agg(lin(x)) + lin_cen(x_cen)
 * + bias, pygda/nn/mixup_gcnconv.py:231-236).  With P = Agg(lin(x)) [n, h] (one aggregation: the
 * shuffled graph of pygda/models/strurw.py:735-758 is a renumbering, so its aggregate is P[perm]):
 *     XX[i]     = drop(relu(P[i] + C[i]  + bias))                                       (x')
 *     XX[n + i] = drop(lam relu(P[i] + Cm[i] + bias) + (1-lam) relu(Pb[i] + Cm[i] + bias))   (x_mix')
 * Pb = P[perm[i]] when the pointer is NULL, else an explicit [n, h] aggregate (foreign edge_index_b).
 *   first != 0: CC = C = lin_cen(x) is [n, h] and Cm[i] = lam C[i] + (1-lam) C[perm[i]]  (x_mix of the
 *               input features is never formed);   first == 0: CC = [C ; Cm] is [2n, h] = lin_cen(XX_prev).
 * mask [n, h] bytes (relu bits of the two mixed terms + keep bit) is written for the backward pass.
 * Keep-bits as in gda_relu_dropout_fwd_f32, two call sites (plain row, mixed row).  h % 4 == 0, h <= 1024.
 * Backward: gXX [2n, h] -> gP [n, h] (incl. the P[perm] route, gathered through inv_perm), gPb [n, h] iff the
 * forward had an explicit Pb (else NULL), gCC ([n, h] if first else [2n, h]), gbias [h] (deterministic
 * two-stage column sum; workspace from gda_mixup_combine_workspace_bytes).
 * ---------------------------------------------------------------------------- */
size_t gda_mixup_combine_workspace_bytes(int64_t n, int64_t h);
int gda_mixup_combine_fwd_f32(const float* P, const float* Pb, const float* CC, int first, const float* bias,
                              const int64_t* perm, int64_t n, int64_t h, float lam, float p, uint64_t seed,
                              const int64_t* step, uint32_t site_x, uint32_t site_m, float* XX, uint8_t* mask,
                              gda_stream_t stream);
int gda_mixup_combine_bwd_f32(const float* gXX, const float* XX, const uint8_t* mask, const int64_t* inv_perm,
                              int first, int64_t n, int64_t h, float lam, float p, float* gP, float* gPb,
                              float* gCC, float* gbias, void* workspace, size_t workspace_bytes,
                              gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Feature-row gather  out[r,:] = x[idx[r],:]  (mini-batch assembly: the x[n_id]
 * slice PyG's NeighborLoader performs, pygda/models/a2gnn.py:260-277).
 * ---------------------------------------------------------------------------- */
int gda_gather_rows_f32(const float* x, int64_t ldx, int64_t d, const int64_t* idx,
                        int64_t n_out, float* out, int64_t ldo, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Graph-level readout (mode='graph'): PyG's global_mean_pool(x, batch) as pygda/nn/a2gnn_base.py:140-141 calls
 * it on the collated batch of a DataLoader -- `batch` sorted, graph g = rows seg_ptr[g] .. seg_ptr[g+1].
 * out[g] = (rows added in node order) / max(count, 1); backward gx[i] = gout[batch[i]] / max(count, 1).
 * seg_ptr int64 [G+1], batch int64 [n] (device).
 * ---------------------------------------------------------------------------- */
int gda_segment_mean_fwd_f32(const float* x, int64_t ldx, const int64_t* seg_ptr, int64_t G, int64_t d,
                             float* out, int64_t ldo, gda_stream_t stream);
int gda_segment_mean_bwd_f32(const float* gout, int64_t ldg, const int64_t* seg_ptr, const int64_t* batch,
                             int64_t n, int64_t d, float* gx, int64_t ldx, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Host neighbour sampler (mini-batch assembly; HOST pointers throughout).
 *
 * Replaces the C++ sampler behind PyG's NeighborLoader as pygda's trainers construct it
 * (pygda/models/a2gnn.py:260-277; grade.py, udagcn.py, adagcn.py likewise): L-hop in-neighbour
 * sampling without replacement from seed nodes, fan-out list `fanouts` (-1 = all), seeds first
 * then newly reached nodes in discovery order, sampled edges relabelled to local ids.
 * A handle is not thread-safe; one per loader.  gda_sampler_sample keeps the batch inside the
 * handle and reports its sizes; gda_sampler_fetch copies it out into caller buffers of those
 * sizes (nodes: global ids [n_nodes]; esrc/edst: local ids [n_edges], message esrc -> edst).
 * ---------------------------------------------------------------------------- */
typedef struct gda_sampler gda_sampler;
int gda_sampler_create(const int64_t* src_host, const int64_t* dst_host, int64_t E, int64_t N,
                       gda_sampler** out);
void gda_sampler_destroy(gda_sampler* s);
/* Worker threads for the neighbour picks of a hop (default 1).  The batch does not depend on it. */
int gda_sampler_set_threads(gda_sampler* s, int workers);
int gda_sampler_sample(gda_sampler* s, const int64_t* seeds_host, int64_t n_seeds,
                       const int32_t* fanouts, int L, uint64_t rng_seed,
                       int64_t* n_nodes_out, int64_t* n_edges_out);
int gda_sampler_fetch(const gda_sampler* s, int64_t* nodes_out, int64_t* esrc_out,
                      int64_t* edst_out);
/* The GCN-normalised adjacency of the last sampled batch as the two CSRs of the aggregation kernels, built on
 * the host where the structure is known: exactly the arrays gda_build_csr_norm(esrc, edst, NULL, n_edges,
 * n_nodes, 1.0, add_self_loops = 1, normalize = 1, degree_side = 0) writes (gcn_norm with unit weights,
 * pygda/nn/prop_gcn_conv.py:64-81), without the device sorts.  rowptr / t_rowptr: n_nodes + 1 entries;
 * colidx / val / t_colidx / t_val: n_edges + n_nodes entries (HOST pointers). */
int gda_sampler_csr_norm(const gda_sampler* s, int32_t* rowptr, int32_t* colidx, float* val,
                         int32_t* t_rowptr, int32_t* t_colidx, float* t_val);

/* ------------------------------------------------------------------------------
 * Device neighbour sampler (csrc/gda_dsampler.hip; DEVICE pointers, fan-outs on the host).
 *
 * The same NeighborLoader call sites (pygda/models/a2gnn.py:260-277) with the graph resident in HBM: the same
 * contract as the host sampler above and, bit for bit, the same batches (same counter-based generator keyed on
 * (seed, hop, node), same discovery order) -- plus the batch's GCN-normalised CSR pair exactly as
 * gda_build_csr_norm(esrc, edst, NULL, n_edges, n_nodes, 1.0, 1, 1, 0) would write it, without its two sorts.
 * Stateless: the caller owns every array.
 *
 * gda_dsampler_build_graph: in-neighbour lists (in_ptr int64 [N+1], in_src int32 [E], edge order kept inside a
 *   list) from a COO edge list; status = device int32[2] {edges with an endpoint outside [0, N), largest in-degree}.
 * gda_dsampler_caps: node_cap / edge_cap of a batch of n_seeds seeds (every output array is sized by them);
 *   GDA_E_UNSUPPORTED for a fan-out of 0 or above 64, or a batch beyond the int32 range (use the host sampler).
 * gda_dsampler_sample: nodes int64 [node_cap] (global ids, seeds first), esrc / edst int64 [edge_cap] (local ids),
 *   rowptr / t_rowptr int32 [node_cap + 1], colidx / val / t_colidx / t_val [edge_cap + node_cap] (all six NULL:
 *   no CSR), counts = device int64[5] {n_nodes, n_edges, nnz, status: 0 ok / 1 capacity exceeded / 2 seed out of
 *   range, n_interior: nodes before the last hop's discoveries -- the rows from there on are never expanded and hold
 *   their self loop only (gda_spmm_csr_interior_kstep_f32)}; rowptr[i] == nnz for i >= n_nodes.  All launches are capacity sized; nothing returns to the host.
 * ---------------------------------------------------------------------------- */
size_t gda_dsampler_graph_workspace_bytes(int64_t E, int64_t N);
int gda_dsampler_build_graph(const int64_t* src, const int64_t* dst, int64_t E, int64_t N,
                             int64_t* in_ptr, int32_t* in_src, int32_t* status,
                             void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_dsampler_caps(int64_t n_seeds, const int32_t* fanouts_host, int L, int64_t max_in_degree, int64_t E,
                      int64_t N, int64_t* node_cap, int64_t* edge_cap);
size_t gda_dsampler_workspace_bytes(int64_t n_seeds, const int32_t* fanouts_host, int L, int64_t max_in_degree,
                                    int64_t E, int64_t N);
int gda_dsampler_sample(const int64_t* in_ptr, const int32_t* in_src, int64_t N, int64_t E, int64_t max_in_degree,
                        const int64_t* seeds, int64_t n_seeds, const int32_t* fanouts_host, int L, uint64_t rng_seed,
                        int64_t* nodes, int64_t* esrc, int64_t* edst,
                        int32_t* rowptr, int32_t* colidx, float* val,
                        int32_t* t_rowptr, int32_t* t_colidx, float* t_val,
                        int64_t* counts, void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* Host-to-device copy of a PINNED host block (hipHostMalloc / hipHostRegister, 16-byte aligned both sides) as a kernel on
 * `stream` that reads the host memory over the bus: for the 0.1 - 1 MB blocks a captured step is fed with per replay (MMD row
 * samples, interpolation weights), where a DMA-engine copy queued behind a running graph idles the device for the engine
 * hand-over.  GDA_E_UNSUPPORTED when the block is not device-mapped or misaligned (callers fall back to hipMemcpyAsync). */
int gda_copy_from_pinned(void* dst, const void* src_host, size_t bytes, gda_stream_t stream);

/* One foreign call per batch for a loader that RECYCLES its batch blocks (round 5; pygda_amd/sampler.py, the producer
 * thread of pygda_amd/data.py's NeighborLoader -- the reference's NeighborLoader workers, pygda/models/a2gnn.py:260-277):
 *   [stream waits for wait_event] -> seeds (host OR device, int64 [n_seeds]) copied to seeds_dev -> gda_dsampler_sample
 *   -> gda_interior_plan_build for both directions when plan_fwd / plan_bwd are given (both or neither; their {q, T} land
 *   in counts[5:7] / counts[7:9]) -> counts (device int64[12], zeroed first) copied to counts_host (PINNED int64[12]) ->
 *   [done_event recorded].  Every array may be a block an earlier batch used: wait_event (recorded by the consumer on its
 *   stream once it has moved on) orders the overwrite.
 * gda_event_*: plain HIP events without timing, owned by the library, so that neither side of that hand-over builds
 *   framework objects per batch.  gda_event_synchronize blocks the calling host thread. */
int gda_event_create(void** event_out);
int gda_event_destroy(void* event);
int gda_event_record(void* event, gda_stream_t stream);
int gda_event_synchronize(void* event);
int gda_stream_wait_event(gda_stream_t stream, void* event);
int gda_dsampler_batch(const int64_t* in_ptr, const int32_t* in_src, int64_t N, int64_t E, int64_t max_in_degree,
                       const int64_t* seeds, int64_t n_seeds, int64_t* seeds_dev,
                       const int32_t* fanouts_host, int L, uint64_t rng_seed,
                       int64_t* nodes, int64_t* esrc, int64_t* edst,
                       int32_t* rowptr, int32_t* colidx, float* val,
                       int32_t* t_rowptr, int32_t* t_colidx, float* t_val,
                       int64_t* counts, void* plan_fwd, void* plan_bwd, size_t plan_bytes,
                       int64_t* counts_host, void* wait_event, void* done_event,
                       void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* _ex: interior_rows > 0 declares the batch's first min(interior_rows, n_nodes) rows "interior" (counts[4] is raised to it
 * before the plans are built): for a consumer that runs every batch at ONE static shape (the captured sampled step).  The
 * rows between the sampled n_interior and interior_rows hold their unit self loop only, so the interior-rows kernels
 * leave them as the leaf copy would. */
int gda_dsampler_batch_ex(const int64_t* in_ptr, const int32_t* in_src, int64_t N, int64_t E, int64_t max_in_degree,
                          const int64_t* seeds, int64_t n_seeds, int64_t* seeds_dev,
                          const int32_t* fanouts_host, int L, uint64_t rng_seed,
                          int64_t* nodes, int64_t* esrc, int64_t* edst,
                          int32_t* rowptr, int32_t* colidx, float* val,
                          int32_t* t_rowptr, int32_t* t_colidx, float* t_val,
                          int64_t* counts, void* plan_fwd, void* plan_bwd, size_t plan_bytes,
                          int64_t* counts_host, void* wait_event, void* done_event, int64_t interior_rows,
                          void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Host construction of the PPMI graph (HOST pointers).
 *
 * Replaces the Python random-walk loop of PPMIConv.norm (pygda/nn/ppmi_conv.py:98-172):
 * `passes` walks (40 in the reference) of length ~U{1..path_len} from every node over the
 * symmetrised neighbour sets, row-normalised visit counts, PPMI weights
 * max(log(p / colsum * |targets| / path_len), 0).  Own counter-based generator (`seed`):
 * statistical, not bit-wise, parity with the reference's np.random stream.  The weighted edge
 * list (sorted by (src, dst), zero weights kept, no self loops added) is held by the returned
 * handle; fetch it into buffers of gda_edge_list_size() entries, then feed it to
 * gda_build_csr_norm(add_self_loops=1, normalize=1, degree_side=1) (ppmi_conv.py:174-184).
 * ---------------------------------------------------------------------------- */
/* Host helper for the MMD backward: CSR (rowptr [num_rows+1], colidx [times*n], int32) of the
 * 0/1 selection matrix that sums the per-sample row gradients back onto the sampled feature
 * rows; idx_host [times, n] are the row samples torch.randint drew on the host
 * (pygda/utils/mmd.py:148-149); column ids are t*m + offset + r into the [times, m, d] buffer. */
int gda_selection_csr_host(const int64_t* idx_host, int times, int64_t n, int64_t num_rows,
                           int64_t offset, int64_t m, int32_t* rowptr_out, int32_t* colidx_out);

typedef struct gda_edge_list gda_edge_list;
int gda_ppmi_build_host(const int64_t* src_host, const int64_t* dst_host, int64_t E, int64_t N,
                        int path_len, int passes, uint64_t seed, gda_edge_list** out);
int64_t gda_edge_list_size(const gda_edge_list* l);
int gda_edge_list_fetch(const gda_edge_list* l, int64_t* src_out, int64_t* dst_out, float* w_out);
void gda_edge_list_destroy(gda_edge_list* l);

/* Aggregation with an affine epilogue, for polynomial graph filters:
 *     y[i] = alpha * x[i] + beta * sum_j A[i,j] x[j] + gamma * z[i]
 * gamma = gamma_imm * (gamma_dev ? *gamma_dev : 1); z may be NULL (then gamma is ignored).
 * Replaces the propagate calls of BernProp.forward (pygda/nn/dgsda_base.py:128-148), where
 * the operators are L = I - A_sym (get_laplacian 'sym', :128) and 2I - L = I + A_sym
 * (add_self_loops(-norm, fill 2), :130): one launch per operator application, the Horner
 * accumulation of the filter terms riding in the same pass.  gamma_dev lets a learnable filter
 * coefficient stay on the device (hipGraph-capturable, no host sync). */
int gda_spmm_csr_axpby_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                           int64_t n_rows, int64_t d, const float* x, int64_t ldx,
                           float* y, int64_t ldy, float alpha, float beta,
                           const float* z, int64_t ldz, float gamma_imm, const float* gamma_dev,
                           const gda_row_split* split, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * TDSS smoothness term (rank 1 of the "next" rows): Laplacian loss over a smoothing graph.
 *
 * gda_laplacian_fwd_f32 / _bwd_f32 replace TDSS.compute_laplacian_loss
 * (pygda/models/tdss.py:435-454) and its autograd graph:
 *     loss = 1/2 sum_e || f[row_e] dinv[row_e] - f[col_e] dinv[col_e] ||^2,
 *     dinv[i] = (#edges with row == i)^-1/2 (inf -> 0).
 *   rowptr_r/colidx_r : CSR whose rows are the `row` (= edge_index[0]) nodes, entries the `col` nodes
 *                       (the by-source CSR of gda_build_csr_norm(add_self_loops=0, normalize=0))
 *   rowptr_c/colidx_c : CSR whose rows are the `col` nodes, entries the `row` nodes (by-destination)
 *   f [N, d] fp32 (ld = ldf); loss [1]; dinv [N] is written by fwd and read by bwd;
 *   grad_loss [1] DEVICE scalar (upstream gradient); grad_f [N, d] overwritten.
 * ---------------------------------------------------------------------------- */
size_t gda_laplacian_workspace_bytes(int64_t N);
int gda_laplacian_fwd_f32(const int32_t* rowptr_r, const int32_t* colidx_r, int64_t N, int d,
                          const float* f, int64_t ldf, float* loss, float* dinv,
                          void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_laplacian_bwd_f32(const int32_t* rowptr_r, const int32_t* colidx_r,
                          const int32_t* rowptr_c, const int32_t* colidx_c, int64_t N, int d,
                          const float* f, int64_t ldf, const float* dinv, const float* grad_loss,
                          float* grad_f, int64_t ldg, gda_stream_t stream);

/* Host builders of the TDSS smoothing graphs (pygda/models/tdss.py:314-388); results come back as a
 * gda_edge_list sorted by (row, col) without duplicates (w is empty: pass NULL to _fetch).
 *   gda_two_hop_host   : `rounds` applications of TwoHopNeighbor (tdss.py:67-87):
 *                        E <- coalesce(E U pattern(A.A) without self loops)
 *   gda_walk_smooth_host: one uniform random walk of walk_len steps from every node along
 *                        row -> col (torch_cluster.random_walk semantics); edge (visited, start)
 *                        for every visited node (tdss.py:367-373).  Own generator (`seed`):
 *                        statistical parity. */
int gda_two_hop_host(const int64_t* src_host, const int64_t* dst_host, int64_t E, int64_t N,
                     int rounds, int threads, gda_edge_list** out);
int gda_walk_smooth_host(const int64_t* src_host, const int64_t* dst_host, int64_t E, int64_t N,
                         int walk_len, uint64_t seed, int threads, gda_edge_list** out);

/* ------------------------------------------------------------------------------
 * Data-parallel exchange steps over RCCL (xGMI inside a node), on a communicator owned by this
 * library and on the caller's stream.  The reference is single-GPU; these are the
 * collectives SURVEY 8e assigns to the path: ONE flat gradient all-reduce per step and the
 * all-gather of the MMD sample rows.
 *   gda_rccl_load       bind librccl at run time (dlopen `path`; NULL/"" = "librccl.so"); pass the
 *                       copy the host framework already loaded so one RCCL lives in the process.
 *                       Without it every function below returns GDA_E_UNSUPPORTED.
 *   gda_comm_unique_id  rank 0 fills 128 bytes (ncclUniqueId) and ships them to the other ranks
 *                       out of band (the host uses its rendezvous store / a broadcast)
 *   gda_comm_init_rank  collective over all ranks; returns the communicator handle
 *   gda_allreduce_f32   in-place sum of buf[count] over the ranks
 *   gda_allgather_f32   recv[rank * count_per_rank ...] = send of that rank
 * ---------------------------------------------------------------------------- */
typedef void* gda_comm_t;
int gda_rccl_load(const char* path);
int gda_comm_unique_id(void* id_out, size_t bytes);
int gda_comm_init_rank(const void* id, size_t bytes, int nranks, int rank, gda_comm_t* comm_out);
int gda_comm_destroy(gda_comm_t comm);
int gda_allreduce_f32(float* buf, int64_t count, gda_comm_t comm, gda_stream_t stream);
int gda_allgather_f32(const float* send, float* recv, int64_t count_per_rank, gda_comm_t comm,
                      gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * View attention of UDAGCN's dual-view encoder (pygda/nn/attention.py:51-54):
 *   stacked = stack(inputs, dim=1); weights = softmax(dense_weight(stacked), dim=1); out = sum(stacked * weights, dim=1)
 * fused: s_k = x_k . w + b, a = softmax_k(s), out = sum_k a_k x_k, one pass each way, no [N, K, h] temporary.
 *   x     HOST array of n_views (2..4) device pointers, view k = [n, h] rows with leading dimension ld[k]
 *   w [h], b [1]   dense_weight.weight / .bias (device);  att [n, n_views] receives the weights (kept for backward)
 * Backward: gx[k] ([n, h] contiguous, or NULL for a view that needs no gradient), gw [h], gb [1]; fixed-order sums
 * (scratch from gda_attention_workspace_bytes).  h % 4 == 0, h <= 512, 16-byte aligned rows, else GDA_E_UNSUPPORTED.
 * ---------------------------------------------------------------------------- */
size_t gda_attention_workspace_bytes(int64_t n, int64_t h);
int gda_attention_fuse_fwd_f32(int n_views, const float* const* x /* HOST array */, const int64_t* ld /* HOST array */,
                               int64_t n, int64_t h, const float* w, const float* b, float* out, int64_t ldo,
                               float* att, gda_stream_t stream);
int gda_attention_fuse_bwd_f32(int n_views, const float* const* x /* HOST array */, const int64_t* ld /* HOST array */,
                               int64_t n, int64_t h, const float* w, const float* att, const float* gout, int64_t ldg,
                               float* const* gx /* HOST array */, float* gw, float* gb,
                               void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Step epilogue: the Adam update.
 *
 * gda_adam_multi_f32: one torch.optim.Adam step (amsgrad off, maximize off) over up to
 *   GDA_ADAM_MAX_TENSORS fp32 tensors in one launch -- the optimiser of every trainer
 *   (pygda/models/a2gnn.py:290-294).  grad += weight_decay * param; m = lerp(m, grad, 1-beta1);
 *   v = beta2 v + (1-beta2) grad^2; param -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps).
 *   `step` of every tensor is a device float holding t-1 (torch keeps one per parameter); it is
 *   incremented first (capturable: no host state).  Tensors with numel 0 are skipped.
 * ---------------------------------------------------------------------------- */
#define GDA_ADAM_MAX_TENSORS 48
typedef struct gda_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    int64_t numel;
} gda_adam_tensor;
int gda_adam_multi_f32(const gda_adam_tensor* tensors /* HOST array */, int n_tensors, float lr, float beta1,
                       float beta2, float eps, float weight_decay, gda_stream_t stream);
/* The same update in TWO calls, so that the counter bump leaves the tail of the step (it sat between the last
 * gradient kernel and the update, 8 us + a launch gap on the critical path of a replayed step):
 *   gda_step_bump          at the START of a training step: `*counter += 1` (the device step counter the fused
 *                          dropout kernels key their Philox streams on; may be NULL) and `*steps[k] += 1` for the
 *                          n_steps Adam step counters (device floats; HOST array of device pointers, n_steps <=
 *                          GDA_ADAM_MAX_TENSORS) -- one launch;
 *   gda_adam_multi_ex_f32  flags & GDA_ADAM_STEPS_BUMPED: the step counters already hold t (no increment launch). */
#define GDA_ADAM_STEPS_BUMPED 1
int gda_step_bump(int64_t* counter, float* const* steps /* HOST array */, int n_steps, gda_stream_t stream);
int gda_adam_multi_ex_f32(const gda_adam_tensor* tensors /* HOST array */, int n_tensors, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int flags, gda_stream_t stream);
/* ... with a gradient that arrives as TWO contributions: grad2[k] (HOST array of device pointers, entries or the array
 * itself may be NULL) is added to tensors[k].grad inside the update -- `g = grad + grad2`, one rounding, the value
 * autograd's accumulation of the two would have stored.  A parameter used by two branches of a step (A2GNN's source
 * and target passes share every layer, pygda/models/a2gnn.py:181-193) otherwise costs one elementwise launch per
 * tensor between the last gradient kernel and the update. */
int gda_adam_multi_sum_f32(const gda_adam_tensor* tensors /* HOST array */, const float* const* grad2 /* HOST array */,
                           int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay, int flags,
                           gda_stream_t stream);
/* gda_wgan_critic_f32 (above) AND the critic optimiser's step in the same two launches: the body of one iteration of
 * AdaGCN's critic loop, pygda/models/adagcn.py:169-183 (`loss.backward(); self.c_optimizer.step()`, the optimiser built
 * at :271-275).  params[0..3] (HOST array) = W1 [a, h], b1 [a], w2 [a], b2 [1] with their torch.optim.Adam state; the
 * gradients are written to params[k].grad (as gda_wgan_critic_f32 writes gW1 ...), every step counter is incremented
 * and the parameters are updated by the thread that formed the gradient -- same arithmetic as gda_adam_multi_f32, same
 * bits.  Only where gda_wgan_critic_f32 takes its two-launch matrix-core path (h in {64, 96, 128}, a % 4 == 0, 16-byte
 * aligned es / et / W1): GDA_E_UNSUPPORTED otherwise, nothing launched. */
int gda_wgan_critic_adam_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                             const int32_t* idx_s, const int32_t* idx_t, const float* alpha, int64_t n_i,
                             int a, float dropout_p, uint64_t seed, const int64_t* step, uint32_t site,
                             float gp_weight, float* loss, const gda_adam_tensor* params /* HOST array of 4 */,
                             float lr, float beta1, float beta2, float eps, float weight_decay,
                             void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * SpecReg's three-layer Wasserstein critic (csrc/gda_critic3.hip), built at pygda/models/specreg.py:281-287:
 *     D(x) = w3 . relu(W2 relu(W1 x + b1) + b2) + b3,   W1, W2 [h, h] row-major, b1, b2, w3 [h], b3 [1]
 * es [n_s, h], et [n_t, h] contiguous fp32 (4-byte alignment suffices).  Envelope: h % 4 == 0, 4 <= h <= 128,
 * n_s, n_t >= 1; GDA_E_UNSUPPORTED outside it, nothing launched.  Every reduction is in a fixed order; no host
 * synchronisation.  Workspace from gda_critic3_workspace_bytes, 16-byte aligned.
 *
 * gda_critic3_update_f32: loss and the six parameter gradients of one critic update -- the body of the critic loop,
 *   specreg.py:194-200 (`loss_1`, `loss_2 = calculate_gradient_penalty` (:380-419, autograd.grad with create_graph),
 *   `(-loss_1 + 10 * loss_2).backward()`), in closed form:
 *     loss = -(mean D(es) - mean D(et)) + 10 * mean_i (|| grad_x D(x_i) ||_2 - 1)^2,   x = cat(es, et)
 *   A row whose input gradient is exactly zero adds 1 to the penalty sum and nothing to the gradients (torch's norm
 *   backward).  One row launch, two deterministic TN products, one fold launch.
 * gda_critic3_update_adam_f32: the same AND `self.optimizer_critic.step()` (specreg.py:200, the optimiser of :288):
 *   params[0..5] (HOST array) = W1, b1, W2, b2, w3, b3 with their torch.optim.Adam state; the gradients are written to
 *   params[k].grad, every step counter is incremented and the parameters are updated in the fold launch -- the
 *   arithmetic of gda_adam_multi_f32, the same bits as gda_critic3_update_f32 followed by it.  The counters are
 *   incremented by the FIRST launch (the fold reads them): every argument is validated before anything is launched, but
 *   should a later launch of the call fail (a HIP launch error, returned as the status), the counters have advanced
 *   and the parameters have not -- the caller then holds an optimiser state one step ahead.
 * gda_critic3_gap_f32: the encoder-side term `loss_grl` (specreg.py:202): means[0] = mean D(es), means[1] = mean D(et)
 *   and, where non-NULL, ges [n_s, h] = d (means[0] - means[1]) / d es = grad_x D / n_s and get [n_t, h] = -grad_x D / n_t.
 * ---------------------------------------------------------------------------- */
int gda_critic3_rows_per_trip(void);    /* rows one trip of the row kernel's capped grid covers (tests size a case by it) */
size_t gda_critic3_workspace_bytes(int64_t n_s, int64_t n_t, int h);
int gda_critic3_update_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                           const float* W1, const float* b1, const float* W2, const float* b2, const float* w3,
                           const float* b3, float* loss, float* gW1, float* gb1, float* gW2, float* gb2,
                           float* gw3, float* gb3, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_critic3_update_adam_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h, float* loss,
                                const gda_adam_tensor* params /* HOST array of 6 */, float lr, float beta1,
                                float beta2, float eps, float weight_decay,
                                void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_critic3_gap_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                        const float* W1, const float* b1, const float* W2, const float* b2, const float* w3,
                        const float* b3, float* means, float* ges, float* get,
                        void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * SpecReg's spectral hinges (csrc/gda_critic3.hip) on X = eivec @ encoded [k, h] contiguous fp32 -- the smoothness
 * and maximum-frequency-response terms of one domain, pygda/models/specreg.py:209-215, with their gradient:
 *     value[0] = gamma_smooth * mean relu(|X[i] - X[i+1]| - thr_smooth)   (over (k - 1) h elements; if thr_smooth > 0)
 *              + gamma_mfr * mean relu(|X| - thr_mfr)                     (over k h elements; if thr_mfr > 0)
 *     G [k, h] = d value / d X, with torch's subgradients relu'(0) = 0, abs'(0) = 0.
 * One launch (k = 100 | 1000 rows of the Laplacian basis in the reference): every workgroup leaves its double sums in
 * the workspace and the one that finishes last adds them in block order, a fixed order.  thr_smooth > 0 needs k >= 2
 * (GDA_E_SIZE).  Workspace from gda_spectral_hinge_workspace_bytes, 16-byte aligned (its ticket word is cleared by a
 * memset node on the stream).
 * ---------------------------------------------------------------------------- */
size_t gda_spectral_hinge_workspace_bytes(int64_t k, int64_t h);
int gda_spectral_hinge_f32(const float* X, int64_t k, int64_t h, float thr_smooth, float gamma_smooth,
                           float thr_mfr, float gamma_mfr, float* value, float* G,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Tall-skinny fp32 GEMMs on the matrix cores: the dense projection of the hidden / classifier
 * layers and its two gradient products (`self.lin(x)`, pygda/nn/prop_gcn_conv.py:204,
 * cached_gcn_conv.py:129, and autograd's dgrad / wgrad).  One operand is tall (rows = nodes).
 *   GDA_GEMM_NT  C[M,N] = A[M,K] * B[N,K]^T      forward  y  = x W^T
 *   GDA_GEMM_NN  C[M,N] = A[M,K] * B[K,N]        dgrad    gx = gy W
 *   GDA_GEMM_TN  C[M,N] = A[K,M]^T * B[K,N]      wgrad    gW = gy^T x  (K = nodes; deterministic split
 *                                                over row slabs, scratch from gda_gemm_workspace_bytes)
 * Row-major with leading dimensions in elements; C must not alias A or B.
 * The same three modes serve activations kept COLUMN-MAJOR (hT [out, ld] next to the LDS-resident K-step
 * kernel): forward hT = W x^T is NT with A = W, B = x; dgrad gx = gT^T W is TN with A = gT; wgrad
 * gW = gT x is NN whose K is the node count -- NN with K >= 1024 and M, N <= 512 takes the deterministic
 * row-slab split as well (gda_gemm_workspace_bytes says how much scratch that needs).
 * ---------------------------------------------------------------------------- */
#define GDA_GEMM_NT 0
#define GDA_GEMM_NN 1
#define GDA_GEMM_TN 2
size_t gda_gemm_workspace_bytes(int mode, int64_t M, int64_t N, int64_t K);
int gda_gemm_f32(int mode, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                 const float* B, int64_t ldb, float* C, int64_t ldc,
                 void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The same with the two by-products of a biased layer `y = x W^T + b` (prop_gcn_conv.py:204,212-213 with
 * prop_nums = 0): `bias` [N] (NT only) is added in the forward epilogue; `colsum` [M] (TN only) receives
 * sum_k A[k, m] -- with A = gy that is the bias gradient, formed beside the weight gradient gy^T x from the tiles
 * the kernel stages anyway (deterministic row-slab partials like the product itself).  Either may be NULL. */
int gda_gemm_ex_f32(int mode, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                    const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, float* colsum,
                    void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The same products for the shapes of sampled sub-graphs (10^5 .. 10^7 rows against a weight whose extents are 128 or
 * 256; pygda/nn/prop_gcn_conv.py:205 on a NeighborLoader batch): the weight lives in registers as ready MFMA operands,
 * only the tall operand streams through LDS (NT / NN), and the weight gradient (TN) reads both operands along their
 * rows with the whole output of a row slab in accumulators (csrc/gda_gemm.hip, "tall products").
 *   NT / NN: N in {128, 256}, K in {128, 256}, A 16-byte aligned with lda % 4 == 0;
 *   TN: M == 128 (the output rows = columns of A), N in {128, 256}, K = the node count; colsum as in gda_gemm_ex_f32.
 * GDA_E_UNSUPPORTED outside that envelope -- callers then use gda_gemm_ex_f32, which takes any shape. */
size_t gda_gemm_tall_workspace_bytes(int mode, int64_t M, int64_t N, int64_t K);
/* ... and for the classifier projection h -> C (C <= 8 classes, `self.cls` of a2gnn_base.py:62 / grade_base.py:66) at
 * 10^5 rows, where a matrix-core tile is 92 % padding: memory-bound vector kernels, fixed-order sums.
 *   NT: N <= 8, K in {32, 64, 128, 256} (+ bias);  NN: K <= 8, N in {32, .., 256};  TN: M <= 8, N in {32, .., 256}
 *   (colsum as in gda_gemm_ex_f32).  GDA_E_UNSUPPORTED outside. */
size_t gda_gemm_skinny_workspace_bytes(int mode, int64_t M, int64_t N, int64_t K);
int gda_gemm_skinny_f32(int mode, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                        const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, float* colsum,
                        void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* Data gradient with the upstream activation's backward in its epilogue: C[M, N] = (y > 0) * (A[M, K] B[K, N]) / (1 - p) with
 * y [M, N] (ld = ldm) the output of dropout(relu(.), p) -- gda_relu_dropout_bwd_f32(A B, y) in one launch, same values.
 * Envelopes: tall (N, K in {128, 256}, the split-fp16 kernel) and skinny (K <= 8, N in {32, 64, 128, 256});
 * GDA_E_UNSUPPORTED elsewhere. */
int gda_gemm_nn_mask_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                         float* C, int64_t ldc, const float* y, int64_t ldm, float p, gda_stream_t stream);
/* Projections that apply the UPSTREAM conv layer's activation while they stage their operand: the input is the pre-activation
 * as the LDS-resident K-step kernel leaves it, column-major xT [K, ldT] (ldT >= n), and no activation launch is left between
 * the aggregation and the next projection.  Dropout arguments as gda_relu_dropout_fwd_cm_f32 (p in [0, 1); p = 0: relu only).
 *   gda_gemm_act_cm_f32:  y [n, K] row-major = drop(relu(x)) -- bit-identical to gda_relu_dropout_fwd_cm_f32; NULL: not stored
 *     (a forward-only pass) -- and hT [M, ldc] = W [M, K] y^T column-major for the next K-step, bit-identical to gda_gemm_f32's NT
 *     product of W with y.  Envelope: K % 4 == 0, M % 4 == 0, ldw % 4 == 0, W and y 16-byte aligned, any n >= 1.
 *   gda_gemm_skinny_act_cm_f32:  Y [n, N] = drop(relu(x)) W [N, K]^T, bit-identical to gda_gemm_skinny_f32's NT form on the
 *     activated rows; forward only.  Envelope: N <= 8, K in {32, 64, 128, 256}, any n >= 1.
 * GDA_E_UNSUPPORTED outside the envelopes: the caller composes the two launches. */
int gda_gemm_act_cm_f32(int64_t n, int64_t M, int64_t K, const float* xT, int64_t ldT, const float* W, int64_t ldw,
                        float* y, float* hT, int64_t ldc, float p, uint64_t seed, const int64_t* step, uint32_t site,
                        gda_stream_t stream);
int gda_gemm_skinny_act_cm_f32(int64_t n, int64_t N, int64_t K, const float* xT, int64_t ldT, const float* W, int64_t ldw,
                               float* Y, int64_t ldy, float p, uint64_t seed, const int64_t* step, uint32_t site,
                               gda_stream_t stream);
/* The backward of gda_gemm_act_cm_f32 from gT [M, ldT], the column-major gradient of hT, with the saved y [n, K], in ONE
 * launch: the data-gradient tiles and the weight gradient's row-slab tiles are two block ranges of one grid on the caller's
 * stream (the weight gradient as a launch of its own sat between the data gradient and its consumer on the backward chain),
 * the activation's backward is the data-gradient tiles' epilogue; the slab partials are summed by the same fixed-order kernel
 * as before.
 *   gxT [K, ldT] = the column-major gradient of the pre-activation = gda_relu_dropout_bwd_cm_f32 of gda_gemm_f32(TN, n, K, M,
 *     gT, W), its padding columns [n, ldT) written as zeros;
 *   gW [M, K] = gda_gemm_f32(NN, M, K, n, gT, y) (workspace: gda_gemm_workspace_bytes of that call).
 * Same values as those calls within the envelope.  gT's padding is never read as a value.  Either output may be NULL: that
 * half's workgroups are not launched.  Envelope: that of gda_gemm_act_cm_f32 with 1 <= M <= 128 (above 128 output rows the
 * composition's data gradient is a sum of two or more slab partials, which this kernel does not reproduce);
 * GDA_E_UNSUPPORTED outside it: the caller composes. */
int gda_gemm_act_cm_bwd_f32(int64_t n, int64_t M, int64_t K, const float* gT, int64_t ldT, const float* W, int64_t ldw,
                            const float* y, float p, float* gxT, float* gW, void* workspace, size_t workspace_bytes,
                            gda_stream_t stream);
/* The sampled batch's first projection without its gather pass, and projections with the conv layer's activation
 * (pygda/nn/a2gnn_base.py:135-138) in the epilogue.  Forward (NT): C = act(A[arow] B^T + bias).
 *   arow (may be NULL): int64 [M] device row ids -- row i of the tall operand is A[arow[i]] (x[n_id] of a sampled batch).
 *   act_mode 0: none; 1: C [M, N] = dropout_site0(relu(.)); 2: C [2M, N], rows i / M + i = two independent draws of the same
 *   pre-activation (gda_relu_dropout_pair_fwd_f32's stacked pair).  Keep-bits as gda_relu_dropout_fwd_f32 / _pair_fwd_f32
 *   would draw them on the [M, N] pre-activation; p <= 0: relu only.
 * Envelope: N, K in {128, 256}, ldc == N, 16-byte aligned operands, the split-fp16 kernel; GDA_E_UNSUPPORTED elsewhere.
 * gda_gemm_tall_wgrad_gather_f32: the TN form of gda_gemm_tall_f32 (C[128, N] = A[Krows, 128]^T X[xrow], colsum[128]) reading
 * x through the batch's node ids; same workspace (gda_gemm_tall_workspace_bytes(TN, 128, N, Krows)). */
int gda_gemm_tall_fwd_ex_f32(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const int64_t* arow,
                             const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                             int act_mode, float p, uint64_t seed, const int64_t* step_dev, uint32_t site0,
                             uint32_t site1, gda_stream_t stream);
int gda_gemm_tall_wgrad_gather_f32(int64_t N, int64_t Krows, const float* A, int64_t lda, const float* X, int64_t ldx,
                                   const int64_t* xrow, float* C, int64_t ldc, float* colsum,
                                   void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_gemm_tall_f32(int mode, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                      const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, float* colsum,
                      void* workspace, size_t workspace_bytes, gda_stream_t stream);


/* ------------------------------------------------------------------------------
 * Source classification loss: mean_i( -log_softmax(logits_i)[labels_i] ), forward and backward.
 * Replaces F.nll_loss(F.log_softmax(source_logits, dim=1), source_data.y)
 * (pygda/models/a2gnn.py:182 and the same line of every trainer).  logits [N, C] fp32 (C <= 64),
 * labels [N] int64 in [0, C); loss [1]; grad_loss [1] DEVICE scalar; grad_logits [N, C].
 * Labels are trusted (no ignore_index): the trainers pass dataset labels.
 * ---------------------------------------------------------------------------- */
size_t gda_softmax_nll_workspace_bytes(void);
/* Mean entropy of the clamped softmax: loss = mean_i sum_c -q_ic log q_ic, q = clamp(softmax(logits_i), clamp_min, 1) --
 * UDAGCN's target term (pygda/models/udagcn.py:193-197: softmax, clamp(min=1e-9, max=1.0), -p log p, sum, mean: seven library
 * launches forward and their autograd twins) as one row kernel + the loss kernels' final fold each way.  The clamp's
 * gradient is the reference's (passes where clamp_min <= p <= 1).  workspace: gda_softmax_nll_workspace_bytes(). */
int gda_softmax_entropy_fwd_f32(const float* logits, int64_t ld, int64_t N, int C, float clamp_min, float* loss,
                                void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_softmax_entropy_bwd_f32(const float* logits, int64_t ld, int64_t N, int C, float clamp_min,
                                const float* grad_loss, float* grad_logits, int64_t ldg, gda_stream_t stream);
int gda_softmax_nll_fwd_f32(const float* logits, int64_t ld, const int64_t* labels, int64_t N, int C,
                            float* loss, void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* _ex: stats (may be NULL) [2] doubles = {loss, number of rows whose argmax (first maximum, as torch.argmax) is the
 * label}: the per-epoch log line of every trainer (loss.item(), source micro-F1 = accuracy of the single-label
 * predictions, pygda/models/a2gnn.py:326-343) as a by-product of the pass that reads the logits anyway. */
int gda_softmax_nll_fwd_ex_f32(const float* logits, int64_t ld, const int64_t* labels, int64_t N, int C,
                               float* loss, double* stats, void* workspace, size_t workspace_bytes,
                               gda_stream_t stream);
int gda_softmax_nll_bwd_f32(const float* logits, int64_t ld, const int64_t* labels, int64_t N, int C,
                            const float* grad_loss, float* grad_logits, int64_t ldg, gda_stream_t stream);
/* _nv: n_valid (DEVICE int64[1], or NULL = all N rows): only rows [0, *n_valid) are real -- the loss is THEIR mean, the
 * count is theirs, the backward pass writes exact zeros into the rows behind them.  For batches padded to a static
 * capacity (the captured sampled step): the row count is read on the device, the launch is the same for every batch. */
int gda_softmax_nll_fwd_nv_f32(const float* logits, int64_t ld, const int64_t* labels, int64_t N, int C,
                               const int64_t* n_valid, float* loss, double* stats, void* workspace,
                               size_t workspace_bytes, gda_stream_t stream);
int gda_softmax_nll_bwd_nv_f32(const float* logits, int64_t ld, const int64_t* labels, int64_t N, int C,
                               const int64_t* n_valid, const float* grad_loss, float* grad_logits, int64_t ldg,
                               gda_stream_t stream);

/* PPMI graph construction on the DEVICE: the estimator and the walks of gda_ppmi_build_host (same
 * counter-based generator, so both builders count the same visits), as sorts + run-length counts.
 *   src/dst [E] int64 device; out_src/out_dst [cap] int64, out_w [cap] fp32 with
 *   cap = N * passes * path_len (upper bound of distinct (start, visited) pairs); out_count [1] int64
 *   DEVICE: the number of pairs written, sorted by (src, dst).
 * Returns GDA_E_UNSUPPORTED when 2E or N*passes*path_len does not fit int32 (use the host builder). */
size_t gda_ppmi_workspace_bytes(int64_t E, int64_t N, int path_len, int passes);
int gda_ppmi_build(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int path_len, int passes,
                   uint64_t seed, int64_t* out_src, int64_t* out_dst, float* out_w, int64_t* out_count,
                   void* workspace, size_t workspace_bytes, gda_stream_t stream);
/* The same walks, counts and column sums, stopped before the weights: out_ratio [cap] double = p / colsum per pair
 * (same workspace, same limits, same order).  Both factors are local to a connected block of the graph, so the pairs
 * of a block-diagonal graph can be kept per block and re-weighted per batch (gda_collate_ppmi_f32). */
int gda_ppmi_build_ratio(const int64_t* src, const int64_t* dst, int64_t E, int64_t N, int path_len, int passes,
                         uint64_t seed, int64_t* out_src, int64_t* out_dst, double* out_ratio, int64_t* out_count,
                         void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * ASN(pygda/models/asn.py, pygda/nn/asn_base.py).
 *
 * gda_asn_recon_f32: recon_loss's cost term without forming the N x N matrix.  z [N, K] (ldz), K <= GDA_ASN_MAX_K;
 *   the labels A + I as a coalesced CSR by row (rowptr [N + 1], col, lab = counts) and the same matrix transposed
 *   (t_rowptr, t_col, t_lab); the labels need not be symmetric.  loss [1] = norm * mean_ij f(x_ij, y_ij) with x = z z^T
 *   and f torch's stable pos_weight-ed BCE-with-logits; dz [N, K] (lddz, must not alias z) = d loss / d z.
 *   Workspace from gda_asn_recon_workspace_bytes(N, K): gda_asn_recon_chunks(N) column chunks of [N, K] partials,
 *   one float per (chunk, 32-row block) and one per row.  N < 2^24.
 * gda_asn_kld_f32: loss [1] = -0.5 / n_nodes * mean_i sum_k (1 + 2 lv - mu^2 - exp(lv)^2) over [N, D] and its gradients
 *   gmu, glv ([N, D], contiguous).  Workspace from gda_asn_rows_workspace_bytes(N, 1, 1).
 * gda_asn_reparam_fwd_f32: z = eps * exp(lv) + mu ([N, D] contiguous z and eps); draw != 0 fills eps with standard
 *   normals from Philox (seed, *step, site), draw == 0 reads it.  gda_asn_reparam_bwd_f32: glv = g * eps * exp(lv).
 * gda_asn_dropout_fwd_f32: y = x * mask, mask in {0, 1 / (1 - p)} from Philox; gda_asn_mask_mul_f32: gx = g * mask.
 * gda_asn_diff_fwd_f32 / _bwd_f32: DiffLoss(a, b) with rows scaled by 1 / (|row| + 1e-6) (the norm is not
 *   differentiated); gram [k1, k2] = An^T Bn, loss [1] = mean(gram^2); the backward writes ga [N, k1], gb [N, k2]
 *   (contiguous) times gl[0].  k1, k2 <= 32.  Workspace from gda_asn_rows_workspace_bytes(N, k1, k2).
 * gda_asn_ppmi_count / _fill: the row-scaled PPMI na [N, N] (ld) as GCNConv's sparse adjacency: cnt [N] = non-zeros
 *   per row plus the diagonal; with rowptr [N + 1] its exclusive scan, row/col/val [nnz] in row-major order,
 *   val = deg^-1/2[j] (na + I)_ij deg^-1/2[i], deg the row sums of na + I (dis [N] = deg^-1/2).
 * Deterministic, no atomics, no allocation or synchronisation.
 * ---------------------------------------------------------------------------- */
#define GDA_ASN_MAX_K 128
#define GDA_ASN_MAX_CHUNKS 64
int gda_asn_recon_chunks(int64_t n);
size_t gda_asn_recon_workspace_bytes(int64_t n, int64_t k);
int gda_asn_recon_f32(const float* z, int64_t ldz, int64_t n, int64_t k, const int32_t* rowptr, const int32_t* col,
                      const float* lab, const int32_t* t_rowptr, const int32_t* t_col, const float* t_lab, float norm,
                      float pos_weight, float* loss, float* dz, int64_t lddz, void* workspace, size_t workspace_bytes,
                      gda_stream_t stream);
size_t gda_asn_rows_workspace_bytes(int64_t n, int64_t k1, int64_t k2);
int gda_asn_kld_f32(const float* mu, int64_t ldm, const float* lv, int64_t ldl, int64_t n, int64_t d, double n_nodes,
                    float* loss, float* gmu, float* glv, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_asn_reparam_fwd_f32(const float* mu, int64_t ldm, const float* lv, int64_t ldl, int64_t n, int64_t d,
                            float* eps, int draw, uint64_t seed, const int64_t* step, uint32_t site, float* z,
                            gda_stream_t stream);
int gda_asn_reparam_bwd_f32(const float* g, const float* eps, const float* lv, int64_t ldl, int64_t n, int64_t d,
                            float* glv, gda_stream_t stream);
int gda_asn_dropout_fwd_f32(const float* x, int64_t n, float p, uint64_t seed, const int64_t* step, uint32_t site,
                            float* mask, float* y, gda_stream_t stream);
int gda_asn_mask_mul_f32(const float* g, const float* mask, int64_t n, float* gx, gda_stream_t stream);
int gda_asn_diff_fwd_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int64_t k1, int64_t k2,
                         float* loss, float* gram, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_asn_diff_bwd_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int64_t k1, int64_t k2,
                         const float* gram, const float* gl, float* ga, float* gb, gda_stream_t stream);
int gda_asn_ppmi_count(const float* na, int64_t n, int64_t ld, int64_t* cnt, gda_stream_t stream);
int gda_asn_ppmi_fill(const float* na, int64_t n, int64_t ld, const int64_t* rowptr, int64_t nnz, int64_t* row,
                      int64_t* col, float* val, float* dis, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * DGDA (pygda/models/dgda.py, pygda/nn/dgda_base.py, pygda/nn/deepwalk_pretrain.py): the manipulated pass on a
 * bit-packed dense adjacency.  bits [N, W = ceil(N / 32)] uint32: bit b of word w of row i is the pair (i, 32 w + b);
 * the matrix is symmetric, its diagonal is set and the bits past column N - 1 are zero.
 *
 * gda_dgda_manip_bits: drop_edges of one domain.  Input: the label CSR of A + I (rowptr [N + 1], col, cnt = counts,
 *   coalesced, by row).  For i > j: bit = add(i, j) OR (cnt(i, j) - drop(i, j) > 0), mirrored to (j, i); only the
 *   lower triangle of the CSR is read.  drop and add are Bernoulli(p_drop) and Bernoulli(p_add) draws per pair from
 *   Philox (seed, *step, site).  Also written: deg [N] = popcount(row) + 1 (the encoder's in-place += I), dis [N] =
 *   deg^-1/2, and scal [4] = {n_lab = sum(bits) + N, pos_weight = (N^2 - n_lab) / n_lab,
 *   norm = N^2 / (2 (N^2 - n_lab)), 0}.  Workspace from gda_dgda_bits_workspace_bytes(N).
 * gda_dgda_pack_bits_f32: the same outputs from a dense matrix adj [N, N] (ld): bit = adj > 0, diagonal set.
 * gda_dgda_bitadj_gemm_f32: out [N, C] (ldo) = dis * (B~ (dis * H)) + bias, B~ the bit matrix with diagonal weight 2,
 *   H [N, C] (ldh), bias [C] or NULL, out must not alias H.  The matrix is symmetric: the backward is the same call
 *   on the incoming gradient without bias.  H enters as three bf16 terms (24 bits), the accumulation is fp32.
 * gda_dgda_recon_bits_f32: gda_asn_recon_f32 with the labels y = bit (+ 1 on the diagonal) and norm, pos_weight
 *   read from scal.  Workspace from gda_dgda_recon_bits_workspace_bytes(N, K).  K <= GDA_ASN_MAX_K.
 * gda_dgda_walks: out [nwalks, length + 1] int64: walk w starts at start[w] and takes `length` uniform steps over
 *   the CSR (rowptr [N + 1], col; int64); a node without out-edges stays put.
 * N <= GDA_DGDA_MAX_N, C <= GDA_DGDA_MAX_C.  Deterministic (integer atomic OR only), no allocation or
 * synchronisation.
 * ---------------------------------------------------------------------------- */
#define GDA_DGDA_MAX_N (1 << 20)
#define GDA_DGDA_MAX_C (1 << 16)
size_t gda_dgda_bits_workspace_bytes(int64_t n);
int gda_dgda_manip_bits(const int32_t* rowptr, const int32_t* col, const float* cnt, int64_t n, float p_drop,
                        float p_add, uint64_t seed, const int64_t* step, uint32_t site, uint32_t* bits, float* deg,
                        float* dis, float* scal, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_dgda_pack_bits_f32(const float* adj, int64_t ld, int64_t n, uint32_t* bits, float* deg, float* dis,
                           float* scal, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_dgda_bitadj_gemm_f32(const uint32_t* bits, int64_t n, const float* dis, const float* h, int64_t ldh, int64_t c,
                             const float* bias, float* out, int64_t ldo, gda_stream_t stream);
size_t gda_dgda_recon_bits_workspace_bytes(int64_t n, int64_t k);
int gda_dgda_recon_bits_f32(const float* z, int64_t ldz, int64_t n, int64_t k, const uint32_t* bits, const float* scal,
                            float* loss, float* dz, int64_t lddz, void* workspace, size_t workspace_bytes,
                            gda_stream_t stream);
int gda_dgda_walks(const int64_t* rowptr, const int64_t* col, int64_t n, const int64_t* start, int64_t nwalks,
                   int64_t length, uint64_t seed, const int64_t* step, uint32_t site, int64_t* out,
                   gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * JHGDA (pygda/models/jhgda.py, pygda/nn/jhgda_base.py).
 *
 * gda_jhgda_prox_f32: proximity_loss(A, S) and its gradients without forming an N x N buffer.  S [N, K] (lds);
 *   loss [1] = 1 / N^2 sum_ij (-a_ij log(Pc + eps) - (1 - a_ij) log(1 - Pc + eps)), P = S S^T, Pc = min(P, 1),
 *   eps = 1e-7.  Level 0: a_ij = the count of (i, j) in the edge list, given as a CSR by source row (rowptr [N + 1],
 *   col, columns ascending inside a row, duplicates kept) and its transpose (t_rowptr, t_col); A = NULL, dA = NULL.
 *   Levels >= 1: the dense A [N, N] (lda), the CSR pointers unused; dA [N, N] (ldda, may be NULL, must not alias A)
 *   receives d loss / d A.  dS [N, K] (ldds, must not alias S) receives d loss / d S (min passes no gradient where
 *   P > 1, half where P == 1); dS = NULL computes the loss (and dA) alone.  Rows in batches of round_up(K, 64): the batch's [B, N] strip of (G + G^T) lives in the
 *   workspace and dS = strip S runs on gda_gemm_ex_f32.  Workspace from gda_jhgda_prox_workspace_bytes(N, K): O(N K).
 *   N <= GDA_JHGDA_PROX_MAX_N, K <= GDA_JHGDA_PROX_MAX_K (GDA_E_UNSUPPORTED beyond).
 * gda_jhgda_pool_rows_fwd_f32: S = softmax(relu(X)) by rows ([N, K]), ent [N] the row entropies -sum S log(S + eps),
 *   ce [1] = mean_i ent_i.  gda_jhgda_pool_rows_bwd_f32: dX = [X > 0] S (g - <S, g>) with
 *   g = dS + gce[0] / N (-log(S + eps) - S / (S + eps)); dS and gce may be NULL (zero).
 * Deterministic, no atomics, no allocation or synchronisation.
 * ---------------------------------------------------------------------------- */
#define GDA_JHGDA_PROX_MAX_N (1 << 20)
#define GDA_JHGDA_PROX_MAX_K 4096
size_t gda_jhgda_prox_workspace_bytes(int64_t n, int64_t k);
int gda_jhgda_prox_f32(const float* S, int64_t lds, int64_t n, int64_t k, const int32_t* rowptr, const int32_t* col,
                       const int32_t* t_rowptr, const int32_t* t_col, const float* A, int64_t lda, float* loss,
                       float* dS, int64_t ldds, float* dA, int64_t ldda, void* workspace, size_t workspace_bytes,
                       gda_stream_t stream);
int gda_jhgda_pool_rows_fwd_f32(const float* X, int64_t ldx, int64_t n, int64_t k, float* S, int64_t lds, float* ent,
                                float* ce, gda_stream_t stream);
int gda_jhgda_pool_rows_bwd_f32(const float* X, int64_t ldx, const float* S, int64_t lds, const float* dS, int64_t ldg,
                                const float* gce, int64_t n, int64_t k, float* dX, int64_t lddx, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * SEPA (pygda/models/sepa.py): the prototype machinery of its loss.  Z [N, C] target logits, F [N, h] target
 * bottleneck features; P = softmax(Z), pred = argmax (lowest index on a tie), e_i = -sum_c P_ic log(P_ic + 1e-12).
 * All matrices contiguous fp32 unless a leading dimension is given; pred / idx are int32.  C <= GDA_SEPA_MAX_CLASSES,
 * widths <= GDA_SEPA_MAX_WIDTH (GDA_E_UNSUPPORTED beyond), 1 <= N < 2^24 (counts are exact in fp32).  Deterministic,
 * no atomics, no allocation or synchronisation; 16-byte accesses where the width and the pointers allow it.
 *
 * gda_sepa_stats_f32: P, pred, e from Z (one pass over the rows).
 * gda_sepa_group_sum_f32: out[c] = sum over {i: idx_i == c} of w_i X_i ([C, d]; w may be NULL = 1; a row whose idx is
 *   outside [0, C) joins no class), cnt[c] = |{i: idx_i == c}|.  divide != 0: out[c] = (sum + cnt_c add[c]) /
 *   (cnt_c + eps) (add [C, d] may be NULL): the class-grouped mean.  Per-workgroup partials (64 rows each, every
 *   thread owns its columns, rows in order) in the workspace, folded in block order.
 *   Workspace from gda_sepa_workspace_bytes(N, C, d): ceil(N / 64) * C * (d + 1) floats.
 * gda_sepa_class_mean_bwd_f32: dX_i = g0[0] G[idx_i] / (cnt[idx_i] + eps), the gather backward of the grouped mean
 *   (g0 may be NULL = 1).
 * gda_sepa_mid_f32 (one workgroup): B = SF / (cnt + 1e-12) [C, h]; M = normalize(offdiag(SP_c / cnt_c)) [C, C], a zero
 *   row where cnt_c == 0; loss_im[0] = sum_k m_k log(m_k + 1e-12) + mean_i e_i with m = colsum(SP) / N.
 * gda_sepa_unbias_rows_f32: U_i = (W_i B) / sum_k (W_ik + 1e-12) - B[pred_i], W_i = normalize(P_i * M[pred_i]);
 *   M and B staged in LDS, each row of U written once.
 * gda_sepa_row_weight_f32: w_i = e_i / max(||R_i||, 1e-12), so that T_i = B[pred_i] + w_i R_i and the class-grouped
 *   sum of T is gda_sepa_group_sum_f32(R, pred, w, divide, eps = 1e-12, add = B) without T being written.
 * gda_sepa_center_rows_bwd_f32: from dcenter [C, h]: dR [N, h] (F.normalize's backward, following its clamp, times
 *   e_i) and de [N], both scaled by g0[0] (NULL = 1).
 * gda_sepa_unbias_rows_bwd_f32: from dU: dPu [N, C] (the gradient of P through W), X [N, C] with X_i = dQ_i * P_i
 *   (its class-grouped sum by pred is dM), and dB [C, h] = sum_i (W_i / s_i)^T dU_i - onehot^T dU, per-workgroup
 *   partials in the workspace (gda_sepa_workspace_bytes(N, C, h)) folded in block order.
 * gda_sepa_mid_bwd_f32 (one workgroup): dBt = dBf + g0 cnt dcenter / (cnt + 1e-12); GP [C, C] = the gradient of SP
 *   through M; gim [C + 1]: gim[k] = g0 lam_im d div / d P_ik, gim[C] = g0 lam_im / N (the mean entropy's share).
 * gda_sepa_dz_rows_f32: dZ from dPu, GP[pred_i], gim and de (entropy, diversity and softmax backward in one row pass).
 * gda_sepa_proto_f32 (one workgroup): T, S [C, h] target / source prototypes; losses[0] = proto_alignment(T, S),
 *   losses[1] = seperate_center(S); dT, dS (both or neither, must not alias the inputs) receive
 *   d (wpp losses[0] + wsep losses[1]) / d (T, S).  The C x C similarity matrices stay in LDS.
 * ---------------------------------------------------------------------------- */
#define GDA_SEPA_MAX_CLASSES 32
#define GDA_SEPA_MAX_WIDTH 1024
size_t gda_sepa_workspace_bytes(int64_t n, int64_t C, int64_t d);
int gda_sepa_stats_f32(const float* Z, int64_t n, int64_t C, float* P, int32_t* pred, float* ent, gda_stream_t stream);
int gda_sepa_group_sum_f32(const float* X, int64_t ldx, const int32_t* idx, const float* w, int64_t n, int64_t d,
                           int64_t C, int divide, float eps, const float* add, float* out, float* cnt, void* workspace,
                           size_t workspace_bytes, gda_stream_t stream);
int gda_sepa_class_mean_bwd_f32(const float* G, const float* cnt, const int32_t* idx, const float* g0, int64_t n,
                                int64_t d, int64_t C, float eps, float* dX, gda_stream_t stream);
int gda_sepa_mid_f32(const float* SP, const float* cnt, const float* SF, const float* ent, int64_t n, int64_t C,
                     int64_t h, float* B, float* M, float* loss_im, gda_stream_t stream);
int gda_sepa_unbias_rows_f32(const float* P, const int32_t* pred, const float* M, const float* B, int64_t n, int64_t C,
                             int64_t h, float* U, gda_stream_t stream);
int gda_sepa_row_weight_f32(const float* R, const float* ent, int64_t n, int64_t h, float* w, gda_stream_t stream);
int gda_sepa_center_rows_bwd_f32(const float* R, const float* ent, const int32_t* pred, const float* dcenter,
                                 const float* cnt, const float* g0, int64_t n, int64_t C, int64_t h, float* dR,
                                 float* de, gda_stream_t stream);
int gda_sepa_unbias_rows_bwd_f32(const float* dU, const float* P, const int32_t* pred, const float* M, const float* B,
                                 int64_t n, int64_t C, int64_t h, float* dPu, float* X, float* dB, void* workspace,
                                 size_t workspace_bytes, gda_stream_t stream);
int gda_sepa_mid_bwd_f32(const float* dMn, const float* SP, const float* cnt, const float* dBf, const float* dcenter,
                         const float* g0, float lam_im, int64_t n, int64_t C, int64_t h, float* dBt, float* GP,
                         float* gim, gda_stream_t stream);
int gda_sepa_dz_rows_f32(const float* P, const int32_t* pred, const float* dPu, const float* GP, const float* gim,
                         const float* de, int64_t n, int64_t C, float* dZ, gda_stream_t stream);
int gda_sepa_proto_f32(const float* T, const float* S, int64_t C, int64_t h, float tau, float wpp, float wsep,
                       float* losses, float* dT, float* dS, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * SOGA (pygda/models/soga.py): the source phase's label-smoothed cross-entropy and the target phase's adaptation term
 * with its gradient.  logits / dlogits [N, C] contiguous fp32, C <= GDA_SOGA_MAX_CLASSES (GDA_E_UNSUPPORTED beyond); a
 * row is owned by next_pow2(C) lanes.  Deterministic, no atomics, no allocation or synchronisation.  Buffers must be
 * aligned to their element size and the workspace to 16 bytes (GDA_E_UNSUPPORTED otherwise).
 *
 * gda_soga_smooth_ce_f32: loss[0] = mean_i -sum_c t_ic log_softmax(logits_i)_c with t = (1 - epsilon) onehot(labels_i)
 *   + epsilon / C (labels int64); dlogits = d loss / d logits (the 1 / N applied); stats (may be NULL) = { loss, number
 *   of rows whose arg-max (lowest index on a tie) equals the label }.  One row launch and a one-workgroup finalise.
 *   Workspace from gda_soga_ce_workspace_bytes(N, C).
 * gda_soga_adapt_f32: with P = softmax(logits), m = mean_i P_i,
 *     IM    = mean_i -sum_c P_ic log(P_ic + 1e-5) - sum_c -m_c log(m_c + 1e-8)
 *     NCE_v = mean_r [ log sum_k exp(P[center_vr] . P[negative_vrk]) - P[center_vr] . P[positive_vr] ]
 *   out = { IM + lambda_struct NCE_0 + lambda_neigh NCE_1, IM, NCE_0, NCE_1 } (NCE_1 = 0 when V == 1) and dlogits =
 *   d out[0] / d logits.  The tables are int32 and hold node ids in [0, N): center, positive [V, M], negative
 *   [V, M, K], V in {1, 2}; an id outside the range reads node 0 (callers validate on the host).  Five launches: rows
 *   (P, entropy and column-sum partials), pairs (sigma [V, M, K], the centre gradients, loss partials), finalise,
 *   segments, nodes.  The scatter of the InfoNCE gradient is a gather over the REVERSE INDEX: the V M (K + 2) table
 *   entries (view, row, role, k), role centre < positive < negative, grouped by the node they name and sorted by that
 *   tuple inside a node, given as
 *     rev_src [nrev]: the row of P the entry gathers (center_vr), or for a centre entry the table row v M + r;
 *     rev_sig [nrev]: for a negative the index (v M + r) K + k of its sigma; -1 / -2 for a positive of view 0 / 1;
 *                     -3 / -4 for a centre of view 0 / 1;
 *     seg_off [nseg + 1]: the entries cut into segments, none across two nodes, each of a node's segments but its
 *                     last at least GDA_SOGA_MIN_SEGMENT long (so nseg <= N + nrev / GDA_SOGA_MIN_SEGMENT);
 *     node_seg [N + 1]: the segments of each node.
 *   One lane group sums one segment in stored order, the node's group adds its segments in order.  nrev must be
 *   V M (K + 2) (GDA_E_SIZE: an index built for another K).  Workspace from gda_soga_workspace_bytes(N, C, M, K, V).
 * ---------------------------------------------------------------------------- */
#define GDA_SOGA_MAX_CLASSES 64
#define GDA_SOGA_MIN_SEGMENT 16
size_t gda_soga_ce_workspace_bytes(int64_t n, int64_t C);
int gda_soga_smooth_ce_f32(const float* logits, const int64_t* labels, int64_t n, int64_t C, float epsilon, float* loss,
                           float* dlogits, double* stats, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_soga_workspace_bytes(int64_t n, int64_t C, int64_t M, int64_t K, int64_t V);
int gda_soga_adapt_f32(const float* logits, int64_t n, int64_t C, const int32_t* center, const int32_t* positive,
                       const int32_t* negative, int64_t V, int64_t M, int64_t K, float lambda_struct,
                       float lambda_neigh, const int32_t* node_seg, const int32_t* seg_off, int64_t nseg,
                       const int32_t* rev_src, const int32_t* rev_sig, int64_t nrev, float* out, float* dlogits,
                       void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * GTrans (pygda/models/gtrans.py, pygda/utils/perturb.py): a GCN aggregation whose normalised values are a differentiable
 * function of one flip weight p_k per undirected edge, the three-view cosine loss and the budget projection.  fp32,
 * deterministic, no atomics, no allocation or synchronisation: every call may be captured.  Buffers must be aligned to
 * their element size and a workspace to 16 bytes (GDA_E_UNSUPPORTED otherwise).
 *
 * gda_wgcn_plan: the structure of a fit, fixed after get_modified_adj's first coalesce.  The by-destination and
 *   by-source CSR of gda_build_csr_norm_map (add_self_loops = 1: exactly one self-loop slot per row, nnz = edges + N)
 *   with t_to_fwd, and per by-destination entry e
 *     erow [nnz]  its destination (the row it is stored in),
 *     epos [nnz]  its position in the coalesced edge list of ec <= nnz edges, sorted by (source, destination), that
 *                 dropout_adj sees (keep holds ec factors; a position outside [0, ec) reads as a slot without a listed edge); -1
 *                 for the self-loop slot of a node without a listed self loop,
 *     kidx [nnz]  the parameter GROUP that feeds it, -1 for none (self loops, edges outside the parameter list);
 *   the m parameters form mu <= m groups, one per distinct node pair (a duplicate target edge lists its pair twice):
 *   gptr [mu + 1] / gidx [m] the parameters of each group in listed order, pgrp [m] the group of each parameter; a
 *   group contributes the sum of its parameters, or with mean != 0 their mean (to_symmetric's op = 'mean');
 *   pent [mu, 2]  per group the at most two entries it feeds (-1: none);
 *   seg_off [nseg + 1], row_seg [N + 1] (and t_ for the by-source CSR): the entries cut into segments of at most
 *   GDA_WGCN_SEGMENT, none across two rows, and the segments of each row.  A lane group sums a segment in stored order,
 *   the row's thread adds its segments in order.  All pointers device; an index outside its range is skipped (callers
 *   validate on the host).
 * gda_wgcn_norm_f32: per entry w = fold(w_prev + P[kidx]) with P the group's sum or mean and fold(x) = x <= 1 ? x :
 *   2 - x (w = w_prev where kidx < 0, and everywhere when p == NULL: the weights as they stand), dsign = keep * (+1 | -1
 *   by fold branch) = d (keep w) / d P, kw = keep * w; per node deg_i = sum over the entries into i of kw (the self loop
 *   with its own weight), s_i = deg_i^-1/2, 0 where deg_i <= 0; val_e = (s_src kw_e) s_dst in by-destination order and,
 *   through t_to_fwd, t_val in by-source order.  keep: one factor per listed edge, indexed by epos -- 0 or 1, or the
 *   kept share of the weight of an edge that coalesces several listed copies with keep bits of their own --, or NULL;
 *   with keep == NULL and p_drop > 0 the keep bits come from the stream of csrc/gda_dropout.h -- key (seed, (step[0] << 20) ^ site),
 *   element index epos, kept when the element's word >= floor(p_drop 2^32), NO rescaling: a dropped edge is an edge of
 *   weight 0 in the degree, in the message and in its gradient.  A self-loop slot without a listed edge is never
 *   dropped; a listed self loop that is dropped leaves kw = 1 behind, the unit loop gcn_norm then adds.  w, dsign, kw
 *   must not alias w_prev (GDA_E_ALIAS).  Three launches.  Workspace from
 *   gda_wgcn_workspace_bytes(N, nnz).
 * gda_wgcn_edge_grad_f32: gv_e = <G[dst_e], H[src_e]> for every stored entry, self loops included: the gradient of
 *   Y = A H with respect to the values of A given G = dL/dY; G, H [N, d] contiguous, d <= GDA_WGCN_MAX_WIDTH
 *   (GDA_E_UNSUPPORTED beyond).  A lane group per entry, so hub rows need no further cut.  One launch.
 * gda_wgcn_norm_bwd_f32: chains gv = dL/dval to p with the arrays gda_wgcn_norm_f32 left:
 *     dL/ds_i   = sum_{e into i} gv_e kw_e s_src + sum_{e out of i} gv_e kw_e s_dst   (a self loop is in both sums)
 *     dL/ddeg_i = -1/2 s_i^3 dL/ds_i
 *     dL/dkw_e  = s_src s_dst gv_e + dL/ddeg_dst(e)
 *     dp_k      = sum over the entries e that k's group feeds of dsign_e dL/dkw_e, over the group's size for a mean
 *                 (a gather, not a scatter)
 *   Three launches.  Workspace from gda_wgcn_workspace_bytes(N, nnz).
 * gda_gtrans_loss_f32: with c(a, b)_i = <a_i, b_i> / ((|a_i| + 1e-15)(|b_i| + 1e-15)),
 *     out = { part1 - part2, part1 = mean_i 1 - c(o1, o2)_i, part2 = mean_i 1 - c(o2, o3)_i } for margin == -1 and
 *     part2 = mean_i relu(1 - c(o2, o3)_i - margin) otherwise; g1, g2, g3 = d out[0] / d o1, o2, o3 ([N, d] contiguous).
 *   The norm's own gradient is 0 at a zero row, as torch's is.  A row launch and a one-workgroup finalise.  Workspace
 *   from gda_gtrans_loss_workspace_bytes(N).
 * gda_gtrans_project_f32: perturb.project in place, the clamp p >= lo that follows the Adam step folded in: p = max(p,
 *   lo); if sum clamp(p, 0, 1) > budget, bisect miu over [min p - 1, max p] as the reference does (midpoint, f(miu) == 0
 *   or a bracket <= 1e-5 ends it) and p = clamp(p - miu, lo, 1 - lo); else p = clamp(p, lo, 1 - lo).  No host read: the
 *   bisection is GDA_GTRANS_PROJECT_HALVINGS predicated halvings -- a bracket of width W needs ceil(log2(W / 1e-5));
 *   p lies in [lo, 1 - lo] before the Adam step and the step moves an entry by about lr, so W <= 2 + lr and 18 would do
 *   for lr -> 0; 20 cover W <= 10.  One workgroup for m <= GDA_GTRANS_PROJECT_ONE_WG, a chain of HALVINGS + 3 launches
 *   beyond, every workgroup folding the partial sums of the launch before in the same order.  Workspace from
 *   gda_gtrans_project_workspace_bytes(m).
 * ---------------------------------------------------------------------------- */
#define GDA_WGCN_SEGMENT 128
#define GDA_WGCN_MAX_WIDTH 256
#define GDA_GTRANS_PROJECT_ONE_WG 8192
#define GDA_GTRANS_PROJECT_HALVINGS 20
typedef struct gda_wgcn_plan {
    int64_t n, nnz, m, mu, nseg, t_nseg, mean, ec;
    const int32_t *rowptr, *colidx, *t_rowptr, *t_colidx, *t_to_fwd;
    const int32_t *erow, *epos, *kidx, *pent, *gptr, *gidx, *pgrp;
    const int32_t *seg_off, *row_seg, *t_seg_off, *t_row_seg;
} gda_wgcn_plan;
size_t gda_wgcn_workspace_bytes(int64_t n, int64_t nnz);
int gda_wgcn_norm_f32(const gda_wgcn_plan* plan, const float* w_prev, const float* p, const float* keep, float p_drop,
                      uint64_t seed, const int64_t* step, uint32_t site, float* w, float* dsign, float* kw, float* deg,
                      float* s, float* val, float* t_val, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_wgcn_edge_grad_f32(const gda_wgcn_plan* plan, const float* G, const float* H, int64_t d, float* gv,
                           gda_stream_t stream);
int gda_wgcn_norm_bwd_f32(const gda_wgcn_plan* plan, const float* gv, const float* kw, const float* s, const float* dsign,
                          float* dp, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_gtrans_loss_workspace_bytes(int64_t n);
int gda_gtrans_loss_f32(const float* o1, const float* o2, const float* o3, int64_t n, int64_t d, float margin, float* out,
                        float* g1, float* g2, float* g3, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_gtrans_project_workspace_bytes(int64_t m);
int gda_gtrans_project_f32(float* p, int64_t m, float budget, float lo, void* workspace, size_t workspace_bytes,
                           gda_stream_t stream);

/* ----------------------------------------------------------------------------
 * GraphCTA (pygda/models/graphcta.py): the model loss, the per-row top-(K+1) and the rest of test_time_loss without an
 * [N, N] array.  fp32, deterministic (no atomics, fixed summation order), no allocation and no synchronisation.  All
 * matrices contiguous and row-major, every pointer aligned to its element size and a workspace to 16 bytes
 * (GDA_E_UNSUPPORTED otherwise); widths d <= GDA_WGCN_MAX_WIDTH, classes C <= GDA_CTA_MAX_CLASSES, K1 <=
 * GDA_CTA_MAX_K1 (GDA_E_UNSUPPORTED beyond).  The all-pairs products are 64x64 tiles on v_mfma_f32_32x32x2_f32; a
 * workgroup owns 64 rows and a contiguous share of the column tiles, and the shares are folded in order.
 *
 * gda_cta_model_loss_f32: instance_proto_alignment and the weighted cross-entropy.  feat [N, d], logits [N, C],
 *   proto [C, d] (a constant), pred [N] int32 in [0, C).  With f^ = feat / max(|feat|, 1e-12) per row, c^ likewise,
 *   w_i = <f^_i, c^_pred_i>, S_i = sum_c exp(<f^_i, c^_c> / tau), pos_i = exp(w_i / tau), R_i = sum_{j != i}
 *   exp(<f^_i, f^_j> / tau):
 *     cl    = -mean_i log(pos_i / (S_i - pos_i + R_i + 1e-8) + 1e-8)
 *     local = sum_i w_i CE(logits_i, pred_i) / W, W = sum_i w_i a constant of the backward pass (not guarded: it may be
 *             negative or tiny, as in the reference)
 *     out   = {(1 - lamb) local + lamb cl, local, cl};  dfeat = d out[0] / d feat, dlogits = d out[0] / d logits.
 *   The diagonal is left out of R instead of summed and subtracted (the same function and gradient).  Seven launches: two
 *   normalisations, the streamed F^ F^^T with an exp-and-row-sum epilogue, the rows' terms, a one-workgroup sum, the
 *   second streamed pass -- the tile's e_ij (c_i + c_j), c_i = d out[0] / d R_i, times F^_j on the matrix cores --, the
 *   rows' gradients with the chain through the normalisation.  Workspace from gda_cta_loss_workspace_bytes(N, d, C):
 *   O(splits N d), splits <= 8.
 * gda_cta_knn_f32: idx, val [N, K1] = the K1 largest of <F_i, M_j> over j < Nm, values descending, TIES TO THE LOWER
 *   INDEX (the order is (value descending, index ascending) at every step, so it does not depend on the tiling); NaN
 *   counts as +inf, as torch.topk has it, and is RETURNED as +inf in val (torch.topk returns the NaN).  Nm < K1: GDA_E_SIZE.  A tile launch (every row keeps its running list in
 *   LDS) and the merge of the column shares.  Workspace from gda_cta_knn_workspace_bytes(N, Nm, K1).
 * gda_cta_test_time_f32: the rest of test_time_loss.  logits [N, C], feat [N, d] (the bottleneck's output), mem
 *   [Nm, d], nn_idx [N, K1] (gda_cta_knn_f32's; rank 1 is dropped whichever row it is, indices outside [0, Nm) add
 *   nothing), csum [C, d] / ccnt [C] the sums and counts of the memory rows per arg-max class of mem_cls.
 *   p = softmax(logits), pred = its first arg-max, ent = -sum p log(p + 1e-8), est_p = #{ent < mean ent} / N; per class
 *   the int(c_num * est_p / 5) (float64, that operation order) rows of lowest (ent, index) are selected (a counting
 *   rank: no sort, no host read) and
 *     out = {ce - 0.1 nb + 0.1 ng, ce, nb, ng}, ce = mean over the selected rows of CE(logits_i, pred_i) (NaN when none
 *     is), nb = mean_i <f_i, sum_{k = 2..K1} m_nn_ik> / (K1 - 1), ng = mean_i <f_i, sum_{c' != pred_i} csum_c'> /
 *     (Nm - ccnt_pred_i) (0 / 0 = NaN when the memory holds one class only);
 *   dlogits, dfeat the gradients of out[0]; pred, sel [N] int32 the arg-max and the selected mask.  Six launches.
 *   Workspace from gda_cta_tt_workspace_bytes(N, d, C).
 * ---------------------------------------------------------------------------- */
#define GDA_CTA_MAX_CLASSES 64
#define GDA_CTA_MAX_K1 16
size_t gda_cta_loss_workspace_bytes(int64_t n, int64_t d, int64_t c);
int gda_cta_model_loss_f32(const float* feat, const float* logits, const float* proto, const int32_t* pred, int64_t n,
                           int64_t d, int64_t c, float tau, float lamb, float* out, float* dfeat, float* dlogits,
                           void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_cta_knn_workspace_bytes(int64_t n, int64_t nm, int64_t k1);
int gda_cta_knn_f32(const float* F, const float* M, int64_t n, int64_t nm, int64_t d, int64_t k1, int32_t* idx, float* val,
                    void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_cta_tt_workspace_bytes(int64_t n, int64_t d, int64_t c);
int gda_cta_test_time_f32(const float* logits, const float* feat, const float* mem, const int32_t* nn_idx,
                          const float* csum, const float* ccnt, int64_t n, int64_t nm, int64_t d, int64_t c, int64_t k1,
                          float* out, float* dlogits, float* dfeat, int32_t* pred, int32_t* sel, void* workspace,
                          size_t workspace_bytes, gda_stream_t stream);

/* ----------------------------------------------------------------------------
 * KBL (pygda/models/kbl.py, pygda/nn/kbl_base.py): the pair-similarity loss of the bridge model and the global top-k
 * of the cross-domain cosine, without the [ma mb, d] gathers and the [na, nb] array the reference forms.  fp32,
 * deterministic (no atomics, fixed summation order), no allocation, no synchronisation and no host read: both can be
 * captured in a hipGraph.  All matrices contiguous and row-major, every pointer aligned to its element size and a
 * workspace to 16 bytes (GDA_E_UNSUPPORTED otherwise).  The cosine is torch's cosine_similarity: every row is
 * normalised once as x / max(|x|, 1e-8) and the products are 64x64 tiles on v_mfma_f32_32x32x2_f32.
 *
 * gda_kbl_pair_bce_f32: U [n, d], index lists ia [ma], ib [mb] (int32, entries may repeat; an entry outside [0, n)
 *   reads as a zero row that matches no label and receives no gradient), labels y [n] int32.
 *     out[0] = mean over the ma mb pairs (p, q) of BCE(sigmoid(cos(U[ia[p]], U[ib[q]])), [y[ia[p]] == y[ib[q]]]),
 *   each logarithm clamped at -100 as binary_cross_entropy clamps it; dU [n, d] = d out[0] / d U, every row written
 *   (zeros for a node no list names).  Six launches: the two gathered normalisations ([ma, d] and [mb, d]), the tiled
 *   product twice -- g_pq = (sigmoid - target) / (ma mb) goes to LDS and G B^ (then G^T A^) is accumulated on the matrix
 *   cores, per share of the column tiles --, the loss sum, and a wavefront per node that folds the partials of every
 *   list position naming it -- ia in order, then ib in order, the shares in order inside each -- and applies the chain
 *   through the normalisation.  n >= 1, 1 <= d <= GDA_KBL_MAX_WIDTH, 1 <= ma, mb <= GDA_KBL_MAX_PAIR_ROWS: GDA_E_SIZE
 *   beyond.  Workspace from gda_kbl_pair_bce_workspace_bytes(d, ma, mb): O(shares (ma + mb) d), shares <= 8.
 * gda_kbl_bridge_topk_f32: A [na, d], B [nb, d]; row, col [k] int32 and val [k] = the k pairs (i, j) of largest
 *   cos(A_i, B_j) over all na nb pairs, val = sigmoid(cos), in the order (cosine descending, flat index i nb + j
 *   ascending).  That order holds at every step -- in a workgroup's running list in LDS and in the merge of the lists --
 *   so the result does not depend on the tiling.  NaN counts as +inf, as in gda_cta_knn_f32 (val = 1).  THE ORDER IS
 *   BY THE COSINE, NOT BY ITS ROUNDED SIGMOID, on purpose: the reference ranks sigmoid(cos), which is monotone, so the
 *   two differ only among entries the fp32 sigmoid rounds together, where the reference's choice is an artefact of
 *   rounding.  Four launches: two normalisations, the streamed tiles (a workgroup strides over row tiles against its
 *   share of the column tiles; a tile without an element that beats the list's last entry costs one barrier, any
 *   other is offered in four quarters whose candidates are packed by a scan and ranked by counting), the one-workgroup
 *   merge.  1 <= k <= na nb: GDA_E_SIZE otherwise;
 *   k > GDA_KBL_MAX_K: GDA_E_UNSUPPORTED.  Workspace from gda_kbl_bridge_topk_workspace_bytes(na, nb, d, k):
 *   (na + nb) d floats and at most 1024 lists of k entries.
 * ---------------------------------------------------------------------------- */
#define GDA_KBL_MAX_WIDTH 256
#define GDA_KBL_MAX_PAIR_ROWS 1024
#define GDA_KBL_MAX_K 256
size_t gda_kbl_pair_bce_workspace_bytes(int64_t d, int64_t ma, int64_t mb);
int gda_kbl_pair_bce_f32(const float* U, const int32_t* ia, const int32_t* ib, const int32_t* y, int64_t n, int64_t d,
                         int64_t ma, int64_t mb, float* out, float* dU, void* workspace, size_t workspace_bytes,
                         gda_stream_t stream);
size_t gda_kbl_bridge_topk_workspace_bytes(int64_t na, int64_t nb, int64_t d, int64_t k);
int gda_kbl_bridge_topk_f32(const float* A, const float* B, int64_t na, int64_t nb, int64_t d, int64_t k, int32_t* row,
                            int32_t* col, float* val, void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ----------------------------------------------------------------------------
 * GraphATA (pygda/models/graphata.py, pygda/nn/node_centric_conv.py): the row kernels of the node-centric layer and of
 * the multi-source adaptation step.  fp32, deterministic (no atomics, fixed summation order), no allocation, no
 * synchronisation and no host read: an epoch can be captured in a hipGraph.  All matrices contiguous and row-major,
 * every pointer aligned to its element size and a workspace to 16 bytes (GDA_E_UNSUPPORTED otherwise); sources S <=
 * GDA_ATA_MAX_SOURCES, classes C <= GDA_ATA_MAX_CLASSES, widths h, d <= GDA_WGCN_MAX_WIDTH, K1 <= GDA_CTA_MAX_K1
 * (GDA_E_UNSUPPORTED beyond); rows N < 2^25, every size at least 1 (GDA_E_SIZE otherwise).  Nothing is launched when a
 * status other than GDA_OK is returned.
 *
 * SPARSEMAX is the reference's SparsemaxFunction over the S scores of a row, in its operation order: z = a - max a, z
 * sorted descending, support = #{k : k z_(k) > cumsum_k - 1}, tau = (cumsum_support - 1) / support, w = max(z - tau,
 * 0); S = 1 gives w = 1.  Its backward takes the mean of dw over the entries with w != 0 off those entries and gives 0
 * to the others (an entry of the support whose w rounds to exactly 0 counts as outside: the reference divides by the
 * support size there, a difference of measure zero).
 *
 * gda_ata_gate_f32: g = sigmoid(nr) nr, elementwise over numel entries -- what the reference's second, gated
 *   aggregation propagate(x, gamma = sigmoid(nr)) with aggr = 'mean' equals row by row.
 * gda_ata_gate_bwd_f32: dnr = dg (sig + nr sig (1 - sig)) + dnr_in (dnr_in may be NULL; dnr may alias dg or dnr_in).
 * gda_ata_sparsemax_f32 / _bwd_f32: w [N, S] from a [N, S]; da [N, S] from w and dw.  A thread per row.
 * gda_ata_mix_f32: P [N, S h] (block s = g W_s^T), Q [N, h] (= nr W), a [N, S] (the scores nr (W_s^T att)):
 *     w = sparsemax(a_i), y_i = sum_s w_is P_is + lamb Q_i, the sum in the order of s.
 *   A group of min(64, max(8, next_pow2(h))) lanes per row; every lane computes the row's sparsemax in registers.
 * gda_ata_mix_bwd_f32: from gy [N, h], P and w: dP_is = w_is gy_i, dQ = lamb gy, dw_is = <gy_i, P_is> (a fixed
 *   butterfly over the group), da = the sparsemax backward of dw.
 * gda_ata_head_f32: the head of an adaptation step.  Z holds the S classifier outputs, element (s, i, c) at
 *   s src_stride + i row_stride + c: either an [S, N, C] array (src_stride = N C, row_stride = C) or the S column blocks
 *   of an [N, S C] array (src_stride = C, row_stride = S C); any other pair of strides is GDA_E_SIZE.  att [C], pred
 *   [N] int32 (a label outside [0, C) adds no cross-entropy term).
 *     w = sparsemax_s(<Z_si, att>), logits_i = sum_s w_is Z_si, p = softmax(logits),
 *     ent = mean_i -sum_c p log(p + 1e-8), div = sum_c m_c log(m_c + 1e-5) with m = mean_i p, ce = mean_i CE(logits_i,
 *     pred_i); out = {ent + div + ce, ent, div, ce}; dZ (Z's layout) and datt [C] the gradients of out[0].
 *   (The two offsets are the other way round from SOGA's.)  With pred == NULL the call is forward only: logits alone
 *   is written, in one launch, and out / dZ / datt / workspace may be NULL.  Otherwise four launches: the rows with
 *   per-workgroup partials of ent, ce and the column sums of p; a one-workgroup finalise (m, the diversity gradient, the
 *   four figures, in double); the rows' gradients with per-workgroup partials of datt; their ordered fold.  A group of
 *   next_pow2(C) lanes per row, one class per lane.  Workspace from gda_ata_head_workspace_bytes(N, C).
 * gda_ata_vote_f32: pred_i = the FIRST arg-max over c of sum_{k = 2 .. K1} mem_cls[nn_idx[i, k], c] / (K1 - 1), the sum
 *   in rank order; rank 1 is dropped whichever row it is, an index outside [0, Nm) adds nothing.  K1 >= 2.
 * gda_ata_memory_f32: p = softmax(logits [N, C]), q = p^2 / sum_i p^2 (the column sums in two phases: per-workgroup
 *   partials in row order, then their ordered fold in double), and in place
 *     mem_cls = keep mem_cls + momentum q,  mem_fea = keep mem_fea + momentum feat    (feat, mem_fea [N, d]).
 *   keep is passed beside momentum because the reference rounds 1 - momentum in double before the product.  Four
 *   launches.  Workspace from gda_ata_memory_workspace_bytes(N, C).
 * ---------------------------------------------------------------------------- */
#define GDA_ATA_MAX_SOURCES 8
#define GDA_ATA_MAX_CLASSES 64
int gda_ata_gate_f32(const float* nr, float* g, int64_t numel, gda_stream_t stream);
int gda_ata_gate_bwd_f32(const float* nr, const float* dg, const float* dnr_in, float* dnr, int64_t numel,
                         gda_stream_t stream);
int gda_ata_sparsemax_f32(const float* a, int64_t n, int64_t S, float* w, gda_stream_t stream);
int gda_ata_sparsemax_bwd_f32(const float* w, const float* dw, int64_t n, int64_t S, float* da, gda_stream_t stream);
int gda_ata_mix_f32(const float* P, const float* Q, const float* a, int64_t n, int64_t h, int64_t S, float lamb, float* y,
                    float* w, gda_stream_t stream);
int gda_ata_mix_bwd_f32(const float* gy, const float* P, const float* w, int64_t n, int64_t h, int64_t S, float lamb,
                        float* dP, float* dQ, float* da, gda_stream_t stream);
size_t gda_ata_head_workspace_bytes(int64_t n, int64_t C);
int gda_ata_head_f32(const float* Z, int64_t src_stride, int64_t row_stride, const float* att, const int32_t* pred,
                     int64_t n, int64_t C, int64_t S, float* logits, float* out, float* dZ, float* datt, void* workspace,
                     size_t workspace_bytes, gda_stream_t stream);
int gda_ata_vote_f32(const int32_t* nn_idx, const float* mem_cls, int64_t n, int64_t nm, int64_t C, int64_t K1,
                     int32_t* pred, gda_stream_t stream);
size_t gda_ata_memory_workspace_bytes(int64_t n, int64_t C);
int gda_ata_memory_f32(const float* logits, const float* feat, int64_t n, int64_t C, int64_t d, float keep, float momentum,
                       float* mem_cls, float* mem_fea, void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ----------------------------------------------------------------------------
 * PairAlign (pygda/models/pa.py): the statistics behind its edge-weight and label-weight fits, its class-weighted
 * cross-entropy and the refresh of the re-weighted CSR values (csrc/gda_pairalign.hip).  Deterministic (no
 * floating-point atomics: fixed partials folded in a fixed order, so two calls give the same bits), no allocation, no
 * synchronisation and no host read: every call can be captured in a hipGraph.  Matrices contiguous and row-major;
 * classes C, K <= GDA_PA_MAX_CLASSES (GDA_E_UNSUPPORTED beyond), item counts <= GDA_PA_MAX_ITEMS (GDA_E_SIZE).
 * Nothing is launched when a status other than GDA_OK is returned.
 *
 * PLANS.  The statistic kernels take their work as lists the caller builds once per graph (ops.PaPlan):
 *   seg   [n_seg, 3] int32: {row, begin, end} -- the neighbours colidx[begin .. end) of one row, at most
 *         GDA_PA_SEGMENT of them (a hub row is several segments), sorted by the class of the row;
 *   items [n_items, 3] int32: {slot, first segment, end segment} -- one workgroup each, every segment of an item has a
 *         row of class `slot`; sorted by slot, slot_ptr [K + 1] the items of each slot.
 *   For the softmax sums items are [n_items, 4] int32 {domain, slot, first, end} over positions of order0 / order1 (the
 *   rows sorted by class; NULL = the identity), slot_ptr [slots + 1].
 *
 * edge stats: out[a][p][b][q] (float64, [K, C, K, C]) = sum over the stored entries (i, j) of the CSR with cls_i = a,
 *   cls_j = b of z_i[p] z_j[q]; z [N, C] fp32, cls [N] int64 in [0, K) (NULL with K = 1: every node is class 0).  An
 *   entry whose column or class is out of range adds nothing.  Products and sums in float64.  Two launches.
 * softmax sums: out[slot][p] (float64, [slots, C]) = sum of softmax(z_i)[p] over the rows of the slot's items, z0 / z1
 *   the two domains' [n, C] rows.  Two launches for both domains together.
 * ce fwd: loss = (1/n) sum over the rows sel[0 .. n_sel) (sel == NULL: all N rows, n = N; the entries of sel distinct
 *   and in [0, N)) of coef[y_i] (lse(x_i) - x_i[y_i]); coef [C] fp32 is read on the device.  stats (may be NULL) =
 *   {loss, number of rows AMONG ALL N whose first arg-max is their label} as gda_softmax_nll_fwd_ex_f32.  Workspace
 *   from gda_pa_ce_workspace_bytes().  Two launches.
 * ce bwd: grad_logits [N, C] = coef[y_i] (softmax(x_i) - onehot(y_i)) grad_loss / n on the selected rows, exact zeros
 *   elsewhere.  grad_logits must not alias logits (GDA_E_ALIAS).
 * refresh: val[e] = base[e] (keep + lmda rw[cls_row, cls_col]) for every stored entry e of the CSR (swap != 0:
 *   rw[cls_col, cls_row], for the by-source CSR); rw [C, C] fp32 and cls [N] int64 on the device, nnz_cap an upper
 *   bound of rowptr[N] that sizes the launch.  One launch.
 * ---------------------------------------------------------------------------- */
#define GDA_PA_MAX_CLASSES 24
#define GDA_PA_SEGMENT 64
#define GDA_PA_MAX_ITEMS 4096
size_t gda_pa_edge_stats_workspace_bytes(int64_t n_items, int64_t C, int64_t K);
int gda_pa_edge_stats_f64(const int32_t* colidx, const float* z, const int64_t* cls, int64_t N, int64_t C, int64_t K,
                          const int32_t* seg, int64_t n_seg, const int32_t* items, int64_t n_items,
                          const int32_t* slot_ptr, double* out, void* workspace, size_t workspace_bytes,
                          gda_stream_t stream);
size_t gda_pa_softmax_sums_workspace_bytes(int64_t n_items, int64_t C);
int gda_pa_softmax_sums_f64(const float* z0, const float* z1, const int32_t* order0, const int32_t* order1, int64_t n0,
                            int64_t n1, int64_t C, const int32_t* items, int64_t n_items, const int32_t* slot_ptr,
                            int64_t slots, double* out, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_pa_ce_workspace_bytes(void);
int gda_pa_ce_fwd_f32(const float* logits, const int64_t* labels, int64_t N, int64_t C, const int64_t* sel, int64_t n_sel,
                      const float* coef, float* loss, double* stats, void* workspace, size_t workspace_bytes,
                      gda_stream_t stream);
int gda_pa_ce_bwd_f32(const float* logits, const int64_t* labels, int64_t N, int64_t C, const int64_t* sel, int64_t n_sel,
                      const float* coef, const float* grad_loss, float* grad_logits, gda_stream_t stream);
int gda_pa_refresh_values_f32(const int32_t* rowptr, const int32_t* colidx, const float* base, float* val, int64_t N,
                              int64_t nnz_cap, const int64_t* cls, const float* rw, int64_t C, float keep, float lmda,
                              int swap, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * Graph-mode collation on the device (csrc/gda_collate.hip; pygda_amd.data.GraphStore): a batch of a DataLoader over a
 * list of graphs, built from a device-resident copy of the whole list and the batch's graph ids alone.
 * Store: G graphs in dataset order; x [N_total, F] fp32 row-major; node_ptr / edge_ptr int64 [G+1]; edges int64
 * [2, E_total] with GRAPH-LOCAL node ids; y int64 [G]; per normalisation variant the two CSRs (gda_build_csr_norm) of the
 * dataset-order block-diagonal graph.  Batch: ids int64 [B] (device), in batch order; an id outside [0, G) counts as an
 * empty graph.  B == 0 launches nothing.  No entry point allocates or synchronises; outputs must not alias inputs
 * (GDA_E_ALIAS).
 * offsets: seg_ptr_out / edge_off_out int64 [B+1] = exclusive scans of the chosen graphs' node / edge counts, the totals
 *   last.  One launch.
 * nodes: batch_out int64 [n_out] = position in the batch of each node's graph; y_out [B] = y[ids]; x_out [n_out, F] =
 *   the chosen graphs' feature rows, 16-byte accesses when F % 4 == 0 and both arrays are 16-byte aligned.  n_out is the
 *   CAPACITY of the outputs (the host's seg_ptr[B]); nothing is written beyond it.  Two launches.
 * edges: edge_index_out int64 [2, e_out] = the chosen graphs' edges, ids moved by the graph's first row.  One launch.
 * csr offsets: nnz_off_out int64 [B+1] = exclusive scan of the chosen graphs' stored-entry counts
 *   rowptr[node_ptr[g+1]] - rowptr[node_ptr[g]] (the same in both orientations).  One launch.
 * csr: both orientations of the batch's CSR: rowptr rebased, colidx moved by (first row in the batch - first row in
 *   the store), val copied; rowptr_out [n_out+1], colidx_out / val_out [nnz_out].  n_out < 2^31 - 1, nnz_out <= 2^31 - 1
 *   (GDA_E_SIZE).  Two launches.
 * ---------------------------------------------------------------------------- */
int gda_collate_offsets(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* edge_ptr,
                        int64_t* seg_ptr_out, int64_t* edge_off_out, gda_stream_t stream);
/* ppmi: the batch's random-walk PPMI pair list out of pairs kept once per graph (gda_ppmi_build_ratio over the
 *   dataset-order graph, cut per graph): pair_ptr int64 [G+1]; local_src / local_dst int32 [P_total] graph-local ids,
 *   ratio double [P_total] = p / colsum, graph after graph, each sorted by (src, dst).  pair_off int64 [B+1] = the
 *   offsets scan with pair_ptr in the edge-pointer slot.  pairs_out int64 [2, m_out], node ids moved to the batch;
 *   w_out fp32 [m_out] = max(log(ratio * n_targets / path_len), 0), the expression of gda_ppmi_build with the BATCH's
 *   number of visited nodes n_targets (a host sum of per-graph counts, like m_out).  m_out == 0 launches nothing. */
int gda_collate_ppmi_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* pair_ptr, const int64_t* pair_off,
                         const int64_t* seg_ptr, const int32_t* local_src, const int32_t* local_dst, const double* ratio,
                         int64_t P_total, int64_t n_targets, int path_len, int64_t m_out, int64_t* pairs_out,
                         float* w_out, gda_stream_t stream);
/* ppmi csr: the batch's NORMALISED PPMI graph -- what gda_build_csr_norm(pairs_out, w_out, add_self_loops = 1,
 *   normalize = 1, degree_side = 1) gives for the pair list of gda_collate_ppmi_f32, bit for bit -- without a sort.  The
 *   store keeps, once, both CSRs of the ingested dataset-order pair list (rowptr / t_rowptr int32 [N_total+1], colidx /
 *   t_colidx int32 [nnz_total]) and per stored entry the pair that weighs it (pair_of / t_pair_of int32 [nnz_total]:
 *   a store-global pair index, or -1 for a loop that carries fill_value, 1 or 2 when `improved`).  ent_off int64 [B+1] =
 *   gda_collate_csr_offsets over rowptr; batch int64 [n_out] as written by gda_collate_nodes_f32; pair_ptr / pair_off and
 *   w_pairs fp32 [m_pairs] = the inputs and the w_out of gda_collate_ppmi_f32 for this batch (m_pairs == 0: a batch
 *   without a pair, the three may be NULL and every loop is filled).  Outputs: rowptr_out /
 *   t_rowptr_out [n_out+1], colidx_out / val_out / t_colidx_out / t_val_out [nnz_out]; dis_ws fp32 [n_out] is scratch
 *   (deg^-1/2 per row).  An entry's weight is its pair's w_pairs value (the log is evaluated once per pair, there);
 *   degrees are summed over the by-source row in entry order; val = (dis[src] * w) * dis[dst].  n_out / nnz_out are CAPACITIES from host counts
 *   (nnz_out >= n_out: every row holds its loop; n_out < 2^31 - 1, nnz_out <= 2^31 - 1, else GDA_E_SIZE); nothing is
 *   written beyond them.  Three launches; no atomics. */
int gda_collate_ppmi_csr_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                             const int64_t* batch, int64_t n_out, const int64_t* ent_off, int64_t nnz_out,
                             const int32_t* rowptr, const int32_t* colidx, const int32_t* pair_of,
                             const int32_t* t_rowptr, const int32_t* t_colidx, const int32_t* t_pair_of,
                             int64_t nnz_total, const int64_t* pair_ptr, const int64_t* pair_off, const float* w_pairs,
                             int64_t m_pairs, float fill_value, int32_t* rowptr_out, int32_t* colidx_out, float* val_out,
                             int32_t* t_rowptr_out, int32_t* t_colidx_out, float* t_val_out, float* dis_ws,
                             gda_stream_t stream);
int gda_collate_nodes_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                          const float* x, int64_t F, const int64_t* y, int64_t n_out, float* x_out,
                          int64_t* batch_out, int64_t* y_out, gda_stream_t stream);
int gda_collate_edges(const int64_t* ids, int64_t B, int64_t G, const int64_t* edge_ptr, const int64_t* edge_off,
                      const int64_t* seg_ptr, const int64_t* edges, int64_t E_total, int64_t e_out,
                      int64_t* edge_index_out, gda_stream_t stream);
int gda_collate_csr_offsets(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int32_t* rowptr,
                            int64_t* nnz_off_out, gda_stream_t stream);
int gda_collate_csr_f32(const int64_t* ids, int64_t B, int64_t G, const int64_t* node_ptr, const int64_t* seg_ptr,
                        const int64_t* batch, int64_t n_out, const int64_t* nnz_off, int64_t nnz_out,
                        const int32_t* rowptr, const int32_t* colidx, const float* val, const int32_t* t_rowptr,
                        const int32_t* t_colidx, const float* t_val, int32_t* rowptr_out, int32_t* colidx_out,
                        float* val_out, int32_t* t_rowptr_out, int32_t* t_colidx_out, float* t_val_out,
                        gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * svd_transform on the device (pygda/utils/svd_transform.py:8-75): the three operations of extent N of a randomized
 * range finder on the combinatorial Laplacian L = D - A, which is never formed (csrc/gda_svd.hip).  The fourth, a tall
 * panel times a small matrix, is gda_gemm_ex_f32 (NN).  Widths 1 <= w <= GDA_SVD_MAX_WIDTH (GDA_E_UNSUPPORTED beyond);
 * panels are row-major [n, w] fp32 with a leading dimension >= w -- columns w .. ld are never written.  Workspaces are
 * 16-byte aligned (GDA_E_UNSUPPORTED otherwise).  Every sum is formed in a fixed order: two runs agree bit for bit.
 *
 * gda_svd_lap_apply_f32: y[i, :] = diag[i] x[i, :] - sum_{k in rowptr[i] .. rowptr[i+1]} x[colidx[k], :]
 *   rowptr / colidx: a CSR of the DISTINCT, loop-free directed pairs (no value array: every entry is -1); pass the
 *   by-source CSR for L X and the by-destination CSR for L^T X.  diag [n] fp32 is the duplicate-counting out-degree,
 *   the same for both.  `split` (may be NULL) is the long-row layout of THAT CSR from gda_row_split_build with live
 *   counts (counts_dev NULL; its `scratch` member is not used: the chunk partials live in the workspace); rows with
 *   more than `threshold` entries are summed chunk by chunk, the chunks in order.  y must not alias x (GDA_E_ALIAS).
 * gda_svd_lap_moments_f32: the same walk, nothing stored: moments [2, w] float64 = the per-column sum and sum of
 *   squares of L X, accumulated in float64 (explained_variance_ = moments[1] / n - (moments[0] / n)^2).
 * Workspace for both from gda_svd_lap_workspace_bytes(n, w, n_long, n_chunks, moments != 0).
 *
 * gda_svd_gram_f32: G [w, w] (ldg) = Y^T Y, Y [n, w] (ldy), on v_mfma_f32_32x32x2_f32.  Only the 64 x 64 tiles on and
 *   below the diagonal are computed, over row slabs whose partial tiles are added in slab order and mirrored:
 *   G == G^T bit for bit.  G must not alias Y.  n == 0 zero-fills G.  Workspace from gda_svd_gram_workspace_bytes(n, w).
 * ---------------------------------------------------------------------------- */
#define GDA_SVD_MAX_WIDTH 4096
size_t gda_svd_lap_workspace_bytes(int64_t n, int64_t w, int64_t n_long, int64_t n_chunks, int moments);
int gda_svd_lap_apply_f32(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n, int64_t w,
                          const float* x, int64_t ldx, float* y, int64_t ldy, const gda_row_split* split,
                          void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_svd_lap_moments_f32(const int32_t* rowptr, const int32_t* colidx, const float* diag, int64_t n, int64_t w,
                            const float* x, int64_t ldx, double* moments, const gda_row_split* split,
                            void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_svd_gram_workspace_bytes(int64_t n, int64_t w);
int gda_svd_gram_f32(const float* Y, int64_t ldy, int64_t n, int64_t w, float* G, int64_t ldg,
                     void* workspace, size_t workspace_bytes, gda_stream_t stream);

/* ------------------------------------------------------------------------------
 * GMMClustering / Clustering (pygda/nn/gmm_clustering.py) on the device (csrc/gda_gmm.hip): the EM steps of a
 * full-covariance Gaussian mixture as sklearn.mixture.GaussianMixture runs them, for r restarts at once, and the
 * assignment step of a k-means.  Sizes 1 <= n < 2^31, 1 <= d <= GDA_GMM_MAX_DIM, 1 <= k <= GDA_GMM_MAX_COMPONENTS,
 * 1 <= r <= GDA_GMM_MAX_RUNS: GDA_E_SIZE below, GDA_E_UNSUPPORTED beyond.  Nothing synchronises; every sum is formed
 * in a fixed order (no float atomics): two calls agree bit for bit, and a run's results do not depend on the other
 * runs of the batch.  Workspaces are 16-byte aligned (GDA_E_UNSUPPORTED otherwise).
 *
 * Layouts (fp32, contiguous unless a leading dimension is named):
 *   x [n, d] row-major with ldx >= d, shared by the runs; the columns d .. ldx are never read
 *   resp [r, n, k]   weights [r, k]   means [r, k, d]   covariances, precisions_chol [r, k, d, d]
 *   log_det [r, k] float64
 *   state [r] of gda_gmm_state (32 bytes each, 8-byte aligned), zeroed with lower_bound = -inf before a fit
 *
 * The freeze rule.  A kernel leaves every array and the state of a run untouched when the run's `failed` is set;
 * E-step kernels also when `converged` >= 1, M-step and factor kernels when `converged` >= 2.  The E-step call that
 * finds |lower_bound - previous| < tol sets converged = 1 (that iteration's M-step and factor still run, as sklearn's
 * loop does); the next E-step call moves it to 2.  So enqueueing E, M, factor more often than a run needs changes none
 * of its bits, and no host read sits inside the loop.  state == NULL: no freezing (and for the E-step no closing).
 *
 * gda_gmm_mstep_f32: nk = sum_rows resp + 10 eps(fp32); weights = nk / sum_k nk; means = resp^T x / nk; covariances =
 *   (x - mean_k)^T diag(resp_k) (x - mean_k) / nk + reg_covar I on v_mfma_f32_32x32x2_f32, centring and weight applied
 *   while the operand is staged; 64 x 64 tiles on and below the diagonal, row-slab partials added in slab order and
 *   mirrored: every covariance equals its transpose bit for bit.  Workspace from gda_gmm_mstep_workspace_bytes.
 * gda_gmm_factor_f32: per (run, component) the Cholesky factor L of the covariance in float64, precisions_chol =
 *   (L^-1)^T (upper triangular, the rest zero-filled), log_det = sum log diag(precisions_chol).  A non-positive or
 *   non-finite pivot sets the run's `failed` and stores nothing else for that component.  state is required.
 * gda_gmm_estep_f32: log p[i, c] = -(d log 2 pi + |(x_i - mean_c) P_c|^2) / 2 + log_det_c + log weights_c, the product on
 *   the matrix cores and never stored; lse_i = logsumexp_c and resp = exp(log p - lse) per row in float64 from the fp32
 *   squared norms.  With state: sum_i lse_i in float64
 *   in a fixed order, then per run prev = lower_bound, lower_bound = sum / n, n_iter += 1 and the flag as above.
 *   Workspace from gda_gmm_estep_workspace_bytes(n, r).
 * gda_kmeans_step_f32: metric 0 = 0.5 (1 - cos) (F.normalize with eps 1e-12 on both sides), 1 = squared Euclidean,
 *   2 = Euclidean between the normalised rows.  labels [n] int64 = the nearest of centers [k, d], lowest index on an
 *   exact tie; dist [n, k] (may be NULL); sums [k, d] = the sum of the UNnormalised rows per label and counts [k], added
 *   in row-block order.  Workspace from gda_kmeans_step_workspace_bytes(n, d, k).
 * gda_gmm_label_sums_f32: sums [k, d] = the sum of the rows of x per label and counts [k], from labels [n] int64 (a
 *   label outside [0, k) belongs to no class); partials per block of 64 rows, added in block order.  Workspace from
 *   gda_gmm_label_sums_workspace_bytes(n, d, k).
 * gda_lsa_cos_f32 / gda_lsa_cost_f64: the linear assignment of a [k, k] float64 cost -- 0.5 (1 - cos) between the rows
 *   of tgt_centers and src_centers [k, d] (normalised as F.normalize, eps 1e-12, in float64), or the cost given -- by the
 *   shortest-augmenting-path algorithm of scipy.optimize.linear_sum_assignment in float64, one wave, the lowest column on
 *   an exact tie.  cluster2label [k] int32 = the column of each row, shuffle_idx [k] its inverse.  state (one
 *   gda_gmm_state, may be NULL): a non-finite cost, or `failed` set on entry, writes the identity and sets `failed`.
 * gda_gmm_relabel_f32: per row of resp [n, k] the argmax (lowest index on a tie); labels [n] int64 =
 *   cluster2label[argmax], or fallback[row] when state's `failed` is set (state, fallback may be NULL); prob [n, k] (may
 *   be NULL) = the columns re-arranged, prob[:, j] = resp[:, shuffle_idx[j]]; onehot [n, k] (may be NULL) of the label.
 *   cluster2label == shuffle_idx == NULL: the identity (the argmax of given probabilities alone).
 * ---------------------------------------------------------------------------- */
#define GDA_GMM_MAX_DIM 128
#define GDA_GMM_MAX_COMPONENTS 32
#define GDA_GMM_MAX_RUNS 8
typedef struct gda_gmm_state {
    double lower_bound, prev_lower_bound;
    int32_t n_iter, converged, failed, reserved;
} gda_gmm_state;
size_t gda_gmm_mstep_workspace_bytes(int64_t n, int64_t d, int64_t k, int64_t r);
int gda_gmm_mstep_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, int64_t r, const float* resp,
                      float reg_covar, float* weights, float* means, float* covariances, const void* state,
                      void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_gmm_factor_f32(const float* covariances, int64_t d, int64_t k, int64_t r, float* precisions_chol,
                       double* log_det, void* state, gda_stream_t stream);
size_t gda_gmm_estep_workspace_bytes(int64_t n, int64_t r);
int gda_gmm_estep_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, int64_t r, const float* weights,
                      const float* means, const float* precisions_chol, const double* log_det, float* resp, double tol,
                      void* state, void* workspace, size_t workspace_bytes, gda_stream_t stream);
size_t gda_kmeans_step_workspace_bytes(int64_t n, int64_t d, int64_t k);
int gda_kmeans_step_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, const float* centers, int metric,
                        int64_t* labels, float* dist, float* sums, float* counts, void* workspace,
                        size_t workspace_bytes, gda_stream_t stream);
size_t gda_gmm_label_sums_workspace_bytes(int64_t n, int64_t d, int64_t k);
int gda_gmm_label_sums_f32(const float* x, int64_t ldx, int64_t n, int64_t d, int64_t k, const int64_t* labels,
                           float* sums, float* counts, void* workspace, size_t workspace_bytes, gda_stream_t stream);
int gda_gmm_relabel_f32(const float* resp, int64_t n, int64_t k, const int32_t* cluster2label,
                        const int32_t* shuffle_idx, const int64_t* fallback, const void* state, float* prob,
                        int64_t* labels, float* onehot, gda_stream_t stream);
int gda_lsa_cos_f32(const float* tgt_centers, const float* src_centers, int64_t k, int64_t d, int32_t* cluster2label,
                    int32_t* shuffle_idx, void* state, gda_stream_t stream);
int gda_lsa_cost_f64(const double* cost, int64_t k, int32_t* cluster2label, int32_t* shuffle_idx, void* state,
                     gda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GDA_HIP_H */
