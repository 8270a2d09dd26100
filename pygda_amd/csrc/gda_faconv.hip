// FAConv aggregation for gfx950: tanh-gated GCN-normalised neighbour sum, fused, on a projected input.
//
// Replaces PyG FAConv(channels, eps=0.1) as SAGDA's SAGNN layer calls it, conv(x, x, edge_index)
// followed by torch.mm(., W) + b (pygda/nn/sagda_base.py:50,87-88).  The operator is linear in x and
// both attention logits are rank-1 projections of x, so the layer is reassociated onto the projection
// [h | s | r] = x [W | att_l^T | att_r^T]:
//   out_i = sum_k c_k h[col_k] + eps h_i + b,   c_k = tanh(s[col_k] + r_i) * w_k
// (w = gcn_norm's weight with the destination degree).  The gathers run over d = hid columns instead
// of the input width.  Same mapping as the GAT kernels (gda_gat.hip): a lane group of G lanes owns one
// destination row; the per-edge scalars are 4-byte gathers.  The edges of a row are walked in chunks of
// G: each lane computes one coefficient and the chunk is broadcast by lane shuffles, so a tanh is
// evaluated once per edge and column pass.
//   forward   out[i,:] = sum_k c_k h[col_k,:] + eps h[i,:] + bias;  t_k = tanh(.) stored in CSR order
//   backward  k_faconv_bwd_dst (group per destination):  dc_k = gout_i . h[col_k] (group butterfly),
//             dpre_k = dc_k w_k (1 - t_k^2),  gr[i] = sum_k dpre_k
//             k_faconv_bwd_src (group per source, transposed CSR + edge map):
//             gh[j] = sum_k' c[map k'] gout[dst_k'] + eps gout[j],  gs[j] = sum_k' dpre[map k']
// Every product and sum is rounded separately (mul, then add); all sums are sequential in CSR order:
// deterministic, no atomics.  tanhf is the accurate device-library function.
#include "gda_common.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;

// One destination (forward) or source (backward, gh) row: acc[v] = sum over the row's entries of
// coef(k) * src[other(k) * ld + c_v], for the V columns c_v = c0 + lane + v G of this pass.
// Forward: other = colidx, coef = tanh(s[col] + r_i) * w (t stored on the first pass).
// Backward: other = t_colidx, coef = t[map] * w[map], and the dpre sum rides along (gsum).
template <int G, int V, bool FWD>
__device__ __forceinline__ void row_walk(int32_t start, int32_t end, int lane, int c0, int d,
                                         const int32_t* __restrict__ other, const int32_t* __restrict__ map,
                                         const float* __restrict__ w, const float* __restrict__ s, int64_t ldsr,
                                         float ri, float* __restrict__ t_out, const float* __restrict__ t_in,
                                         const float* __restrict__ dpre, const float* __restrict__ src,
                                         int64_t ld, float (&acc)[V], float* gsum) {
    for (int32_t base = start; base < end; base += G) {
        const int32_t k = base + lane;
        int32_t j = 0;
        float cf = 0.f, dp = 0.f;
        if (k < end) {
            j = other[k];
            if (FWD) {
                const float tk = tanhf(__fadd_rn(s[(int64_t)j * ldsr], ri));
                if (c0 == 0) t_out[k] = tk;
                cf = __fmul_rn(tk, w[k]);
            } else {
                const int32_t m = map[k];
                cf = __fmul_rn(t_in[m], w[m]);
                if (c0 == 0) dp = dpre[m];
            }
        }
        const int cnt = min(G, end - base);
        for (int q = 0; q < cnt; ++q) {
            const int32_t jq = __shfl(j, q, G);
            const float cq = __shfl(cf, q, G);
            if (!FWD && c0 == 0) *gsum = __fadd_rn(*gsum, __shfl(dp, q, G));
            const float* row = src + (int64_t)jq * ld;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int c = c0 + lane + v * G;
                if (c < d) acc[v] = __fadd_rn(acc[v], __fmul_rn(cq, row[c]));
            }
        }
    }
}

template <int G, int V>
__global__ void __launch_bounds__(TB)
k_faconv_fwd(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ val,
             int64_t n_rows, int d, const float* __restrict__ h, int64_t ldh, const float* __restrict__ s,
             const float* __restrict__ r, int64_t ldsr, float eps, const float* __restrict__ bias,
             float* __restrict__ out, int64_t ldo, float* __restrict__ t) {
    const int lane = threadIdx.x % G;
    const int64_t row = (int64_t)blockIdx.x * (TB / G) + threadIdx.x / G;
    if (row >= n_rows) return;                 // whole groups leave together (G divides the wavefront)
    const int32_t start = rowptr[row], end = rowptr[row + 1];
    const float ri = r[row * ldsr];
    for (int c0 = 0; c0 < d; c0 += G * V) {
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        row_walk<G, V, true>(start, end, lane, c0, d, colidx, nullptr, val, s, ldsr, ri, t, nullptr, nullptr, h,
                             ldh, acc, nullptr);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = c0 + lane + v * G;
            if (c < d) {
                float o = __fadd_rn(acc[v], __fmul_rn(eps, h[row * ldh + c]));
                if (bias) o = __fadd_rn(o, bias[c]);
                out[row * ldo + c] = o;
            }
        }
    }
}

template <int G>
__global__ void __launch_bounds__(TB)
k_faconv_bwd_dst(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                 const float* __restrict__ val, int64_t n_rows, int d, const float* __restrict__ h, int64_t ldh,
                 const float* __restrict__ t, const float* __restrict__ gout, int64_t ldgo,
                 float* __restrict__ gr, int64_t ldgsr, float* __restrict__ dpre) {
    const int lane = threadIdx.x % G;
    const int64_t row = (int64_t)blockIdx.x * (TB / G) + threadIdx.x / G;
    if (row >= n_rows) return;
    const int32_t start = rowptr[row], end = rowptr[row + 1];
    const float* g = gout + row * ldgo;
    float acc = 0.f;
    for (int32_t k = start; k < end; ++k) {
        const float* hj = h + (int64_t)colidx[k] * ldh;
        float part = 0.f;
        for (int c = lane; c < d; c += G) part = __fadd_rn(part, __fmul_rn(g[c], hj[c]));
        const float dc = __shfl(group_sum<G>(part), 0, G);      // lane 0's order: one value for the whole group
        const float tk = t[k];
        const float dp = __fmul_rn(__fmul_rn(dc, val[k]), __fsub_rn(1.f, __fmul_rn(tk, tk)));
        if (lane == 0) dpre[k] = dp;
        acc = __fadd_rn(acc, dp);
    }
    if (lane == 0) gr[row * ldgsr] = acc;
}

template <int G, int V>
__global__ void __launch_bounds__(TB)
k_faconv_bwd_src(const int32_t* __restrict__ t_rowptr, const int32_t* __restrict__ t_colidx,
                 const int32_t* __restrict__ t_to_fwd, const float* __restrict__ val, int64_t n_rows, int d,
                 const float* __restrict__ t, const float* __restrict__ dpre, const float* __restrict__ gout,
                 int64_t ldgo, float eps, float* __restrict__ gh, int64_t ldgh, float* __restrict__ gs,
                 int64_t ldgsr) {
    const int lane = threadIdx.x % G;
    const int64_t row = (int64_t)blockIdx.x * (TB / G) + threadIdx.x / G;
    if (row >= n_rows) return;
    const int32_t start = t_rowptr[row], end = t_rowptr[row + 1];
    float gsum = 0.f;
    for (int c0 = 0; c0 < d; c0 += G * V) {
        float acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = 0.f;
        row_walk<G, V, false>(start, end, lane, c0, d, t_colidx, t_to_fwd, val, nullptr, 0, 0.f, nullptr, t, dpre,
                              gout, ldgo, acc, &gsum);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = c0 + lane + v * G;
            if (c < d) gh[row * ldgh + c] = __fadd_rn(acc[v], __fmul_rn(eps, gout[row * ldgo + c]));
        }
    }
    if (lane == 0) gs[row * ldgsr] = gsum;
}

int pick_group(int64_t d) { return d > 32 ? 64 : d > 16 ? 32 : d > 8 ? 16 : 8; }
// columns per lane and pass: one pass up to 4 G columns, passes of 4 G beyond
int pick_vec(int64_t d, int G) { return d <= G ? 1 : d <= 2 * G ? 2 : 4; }

int check_sizes(int64_t n_rows, int64_t d, int64_t ld_a, int64_t ld_b, int64_t ld_c, int64_t ld_d) {
    if (n_rows < 0 || d < 0 || n_rows >= INT32_MAX || d >= INT32_MAX) return GDA_E_SIZE;
    if (ld_a < d || ld_c < d || ld_b < 1 || ld_d < 1) return GDA_E_SIZE;
    if (n_rows > 0 && (ld_a > INT64_MAX / n_rows || ld_b > INT64_MAX / n_rows || ld_c > INT64_MAX / n_rows ||
                       ld_d > INT64_MAX / n_rows)) return GDA_E_SIZE;
    return GDA_OK;
}

}  // namespace

#define FACONV_SWITCH(d, CALL)                                      \
    do {                                                            \
        const int G_ = pick_group(d), V_ = pick_vec(d, G_);         \
        switch (G_ * 10 + V_) {                                     \
            case 641: CALL(64, 1); break;                           \
            case 642: CALL(64, 2); break;                           \
            case 644: CALL(64, 4); break;                           \
            case 321: CALL(32, 1); break;                           \
            case 161: CALL(16, 1); break;                           \
            default: CALL(8, 1); break;                             \
        }                                                           \
    } while (0)

extern "C" int gda_faconv_fwd_f32(const int32_t* rowptr, const int32_t* colidx, const float* val, int64_t n_rows,
                                  int64_t d, const float* h, int64_t ldh, const float* s, const float* r,
                                  int64_t ldsr, float eps, const float* bias, float* out, int64_t ldo, float* t,
                                  gda_stream_t stream_) {
    const int st = check_sizes(n_rows, d, ldh, ldsr, ldo, 1);
    if (st != GDA_OK) return st;
    if (!rowptr || !colidx || !val || !h || !s || !r || !out || !t) return GDA_E_NULL;
    if (n_rows == 0 || d == 0) return GDA_OK;
    if (out == h) return GDA_E_ALIAS;
    hipStream_t hs = (hipStream_t)stream_;
#define CALL(G, V) k_faconv_fwd<G, V><<<(unsigned)gda_cdiv(n_rows, TB / G), TB, 0, hs>>>(                 \
        rowptr, colidx, val, n_rows, (int)d, h, ldh, s, r, ldsr, eps, bias, out, ldo, t)
    FACONV_SWITCH(d, CALL);
#undef CALL
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_faconv_bwd_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                  const int32_t* t_rowptr, const int32_t* t_colidx, const int32_t* t_to_fwd,
                                  int64_t n_rows, int64_t d, const float* h, int64_t ldh, const float* t,
                                  const float* gout, int64_t ldgo, float eps, float* gh, int64_t ldgh, float* gs,
                                  float* gr, int64_t ldgsr, float* dpre, gda_stream_t stream_) {
    int st = check_sizes(n_rows, d, ldh, ldgsr, ldgh, 1);
    if (st != GDA_OK) return st;
    if ((st = check_sizes(n_rows, d, ldgo, 1, d, 1)) != GDA_OK) return st;
    if (!rowptr || !colidx || !val || !t_rowptr || !t_colidx || !t_to_fwd || !h || !t || !gout || !gh || !gs ||
        !gr || !dpre) return GDA_E_NULL;
    if (n_rows == 0 || d == 0) return GDA_OK;
    if (gh == gout || gh == h) return GDA_E_ALIAS;
    hipStream_t hs = (hipStream_t)stream_;
    switch (pick_group(d)) {
        case 64: k_faconv_bwd_dst<64><<<(unsigned)gda_cdiv(n_rows, TB / 64), TB, 0, hs>>>(
                     rowptr, colidx, val, n_rows, (int)d, h, ldh, t, gout, ldgo, gr, ldgsr, dpre); break;
        case 32: k_faconv_bwd_dst<32><<<(unsigned)gda_cdiv(n_rows, TB / 32), TB, 0, hs>>>(
                     rowptr, colidx, val, n_rows, (int)d, h, ldh, t, gout, ldgo, gr, ldgsr, dpre); break;
        case 16: k_faconv_bwd_dst<16><<<(unsigned)gda_cdiv(n_rows, TB / 16), TB, 0, hs>>>(
                     rowptr, colidx, val, n_rows, (int)d, h, ldh, t, gout, ldgo, gr, ldgsr, dpre); break;
        default: k_faconv_bwd_dst<8><<<(unsigned)gda_cdiv(n_rows, TB / 8), TB, 0, hs>>>(
                     rowptr, colidx, val, n_rows, (int)d, h, ldh, t, gout, ldgo, gr, ldgsr, dpre); break;
    }
    GDA_LAUNCH_CHECK();
#define CALL(G, V) k_faconv_bwd_src<G, V><<<(unsigned)gda_cdiv(n_rows, TB / G), TB, 0, hs>>>(              \
        t_rowptr, t_colidx, t_to_fwd, val, n_rows, (int)d, t, dpre, gout, ldgo, eps, gh, ldgh, gs, ldgsr)
    FACONV_SWITCH(d, CALL);
#undef CALL
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
