// ACDNE for gfx950 (pygda/models/acdne.py, pygda/nn/acdne_base.py): the PPMI preprocessing of process_graph and the
// per-step losses.  DMGNN (gda_dmgnn.hip) trains the same network: the heads kernel and the softmax rows here serve
// both, and gda_dmgnn_heads_f32 is defined next to gda_acdne_heads_f32.
//
// Preprocessing, on dense N x N fp32 buffers of leading dimension ld = round_up(N, 4):
//   k_tran      one block per row: the out-degree of the coalesced CSR (counts), r_inv = 1 / (deg + 1e-12), the row of
//               P = D^-1 A written to the CSR values and densely into a_1 and a (my_scale_sim_mat on the adjacency).
//   k_power     a_k = P a_{k-1} (CSR SpMM of width N, P^k commutes with P) fused with a += a_k / k; a block is one row
//               and 1024 columns, each lane four contiguous columns; the CSR entries of the row in order.
//   k_rownorm   one block per row: zero the diagonal, row sum (lane partials, fixed tree), scale by 1 / (sum + 1e-12).
//   k_colsum_*  column sums: slab partials (one lane per column, rows in order), then slabs merged in order; 0 -> 1.
//   k_ppmi      one block per row: max(log(N a / col + 1e-12), 0) (NaN -> 0) in place, its row sum, and the row of the
//               row-normalised copy.
//   k_xnei      one wave per row i: X_nei[i] = sum_j nA[i, j] X[j] over the non-zero j of the row in increasing order,
//               X as CSR (row-major non-zeros); the row accumulates in LDS, one lane per non-zero of X[j] (distinct
//               columns), so every sum runs in the same order each time.
// Per step (b = 2 h rows: h source rows, then h target rows):
//   k_prox_*    both domains in each of three launches, a block per (row, domain): the h x h block of A_ppmi at the
//               batch's PPMI indices (zero diagonal), row-normalised (row sum in double, scale rounded to fp32);
//               net_pro_loss = mean_i sum_j a_ij dis_ij with dis = r_i - 2 e_i.e_j + r_j, and its gradient
//               (2 / h)[(sum_j a_kj + sum_i a_ik) e_k - sum_j (a_kj + a_jk) e_j]; then the two means, rows in order.
//   k_heads     ACDNE's and DMGNN's heads: six launches of one kernel over the whole grid, one phase each.  0: emb =
//               relu(z), h1 and the source half's classifier logits L; 1: h2; 2: per row the domain CE behind
//               GRL(alpha) -> 128 -> 128 -> 2 and, over the source half, the classifier CE of L' (DMGNN: L' = L + A_s L
//               with A_s the source half's normalised block; ACDNE: L' = L); 3: dh2, gW3, gb3, dL (DMGNN: dL' +
//               A_s^T dL'; ACDNE: dL') and the loss; 4: dh1, gW2, gb2, gWc, gbc; 5: gW1, gb1 and dz = (d emb) * (z > 0)
//               with the proximity gradient added.  The target half's logits enter no loss and are not formed.
//               One lane per output element; intermediates in a caller-owned workspace.
//   k_predict   one lane per row: softmax(relu(z) Wc^T + bc) (ACDNE's predict; the P of DMGNN's P + M P).
// Every reduction has a fixed order that depends on the shapes only: two runs are bit-identical.  No atomics.
#include "gda_common.h"
#include "gda_ppmi_block.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int PW_COLS = 1024;               // k_power: columns per block (4 per lane)
constexpr int CS_SLAB = 64;                 // k_colsum_partial: rows per slab
constexpr int HEAD_MAX_BLOCKS = 1024;      // k_heads: grid cap (the grid strides over the work items)
constexpr int DH = 128;                     // discriminator width (DomainDiscriminator)

__global__ void __launch_bounds__(TB) k_tran(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                             const float* __restrict__ cnt, int n, int64_t ld, float* __restrict__ pval,
                                             float* __restrict__ a1, float* __restrict__ a) {
    __shared__ float red[TB];
    const int i = blockIdx.x;
    const int b = rowptr[i], e = rowptr[i + 1];
    float s = 0.f;
    for (int k = b + (int)threadIdx.x; k < e; k += TB) s += cnt[k];
    const float deg = block_sum_f(s, red);
    const float r_inv = 1.f / (deg + 1e-12f);
    float* ra1 = a1 ? a1 + (int64_t)i * ld : nullptr;
    float* ra = a + (int64_t)i * ld;
    for (int64_t c = threadIdx.x; c < ld; c += TB) {
        if (ra1) ra1[c] = 0.f;
        ra[c] = 0.f;
    }
    __syncthreads();
    for (int k = b + (int)threadIdx.x; k < e; k += TB) {
        const float v = cnt[k] * r_inv;
        pval[k] = v;
        if (ra1) ra1[col[k]] = v;
        ra[col[k]] = v;
    }
}

__global__ void __launch_bounds__(TB) k_power(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                              const float* __restrict__ pval, int64_t ld,
                                              const float* __restrict__ prev, float* __restrict__ next,
                                              float* __restrict__ a, float kf) {
    const int i = blockIdx.x;
    const int64_t c = (int64_t)blockIdx.y * PW_COLS + 4 * (int64_t)threadIdx.x;
    if (c >= ld) return;
    const int b = rowptr[i], e = rowptr[i + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = b; k < e; ++k) {
        const float w = pval[k];
        const float4 v = *reinterpret_cast<const float4*>(prev + (int64_t)col[k] * ld + c);
        acc.x += w * v.x;
        acc.y += w * v.y;
        acc.z += w * v.z;
        acc.w += w * v.w;
    }
    const int64_t o = (int64_t)i * ld + c;
    if (next) *reinterpret_cast<float4*>(next + o) = acc;
    float4 s = *reinterpret_cast<float4*>(a + o);
    s.x += acc.x / kf;
    s.y += acc.y / kf;
    s.z += acc.z / kf;
    s.w += acc.w / kf;
    *reinterpret_cast<float4*>(a + o) = s;
}

__global__ void __launch_bounds__(TB) k_rownorm(float* __restrict__ a, int n, int64_t ld) {
    __shared__ float red[TB];
    const int i = blockIdx.x;
    float* r = a + (int64_t)i * ld;
    if (threadIdx.x == 0) r[i] = 0.f;
    __syncthreads();
    float s = 0.f;
    for (int c = threadIdx.x; c < n; c += TB) s += r[c];
    const float r_inv = 1.f / (block_sum_f(s, red) + 1e-12f);
    for (int c = threadIdx.x; c < n; c += TB) r[c] = r_inv * r[c];
}

__global__ void __launch_bounds__(TB) k_colsum_partial(const float* __restrict__ a, int n, int64_t ld,
                                                       float* __restrict__ part) {
    const int64_t c = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (c >= n) return;
    const int r0 = blockIdx.y * CS_SLAB, r1 = min(n, r0 + CS_SLAB);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += a[(int64_t)r * ld + c];
    part[(int64_t)blockIdx.y * ld + c] = s;
}

__global__ void __launch_bounds__(TB) k_colsum_final(const float* __restrict__ part, int slabs, int n, int64_t ld,
                                                     float* __restrict__ colsum) {
    const int64_t c = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (c >= n) return;
    float s = 0.f;
    for (int k = 0; k < slabs; ++k) s += part[(int64_t)k * ld + c];
    colsum[c] = s == 0.f ? 1.f : s;
}

__global__ void __launch_bounds__(TB) k_ppmi(float* __restrict__ a, int n, int64_t ld, const float* __restrict__ colsum,
                                             float* __restrict__ na) {
    __shared__ float red[TB];
    const int i = blockIdx.x;
    float* r = a + (int64_t)i * ld;
    const float p = (float)n;
    float s = 0.f;
    for (int c = threadIdx.x; c < n; c += TB) {
        float v = logf((p * r[c]) / colsum[c] + 1e-12f);
        if (!(v > 0.f)) v = 0.f;                      // NaN and negatives
        r[c] = v;
        s += v;
    }
    const float r_inv = 1.f / (block_sum_f(s, red) + 1e-12f);
    float* q = na + (int64_t)i * ld;
    for (int c = threadIdx.x; c < n; c += TB) q[c] = r_inv * r[c];
}

__global__ void __launch_bounds__(GDA_WAVE) k_xnei(const float* __restrict__ na, int n, int64_t ld,
                                                   const int32_t* __restrict__ xrp, const int32_t* __restrict__ xcol,
                                                   const float* __restrict__ xval, int f, float* __restrict__ out,
                                                   int64_t ldo) {
    extern __shared__ float acc[];
    const int i = blockIdx.x, lane = threadIdx.x;
    for (int c = lane; c < f; c += GDA_WAVE) acc[c] = 0.f;
    __syncthreads();
    const float* r = na + (int64_t)i * ld;
    for (int j0 = 0; j0 < n; j0 += GDA_WAVE) {
        const int jl = j0 + lane;
        const float w = jl < n ? r[jl] : 0.f;
        uint64_t live = __ballot(w != 0.f);
        while (live) {
            const int src = __ffsll((unsigned long long)live) - 1;
            live &= live - 1;
            const float wj = __shfl(w, src);
            const int j = j0 + src;
            const int b = xrp[j], e = xrp[j + 1];
            for (int k = b + lane; k < e; k += GDA_WAVE) acc[xcol[k]] += wj * xval[k];
            __syncthreads();
        }
    }
    float* o = out + (int64_t)i * ldo;
    for (int c = lane; c < f; c += GDA_WAVE) o[c] = acc[c];
}

// ---------------------------------------------------------------------------------------------------- per step --
// k_prox_rows: block (row i, domain): the gathered row i of the block (zero diagonal), its scale rinv_i = 1 /
// (fp32(double row sum) + 1e-12) and |e_i|^2.  k_prox_grad: block (row k, domain): the row's loss term
// sum_j a_kj dis_kj, and the row of the gradient.  k_prox_sum: the two means, rows in order.
struct ProxWs {
    float* A;        // [2, h, h]
    float* rinv;     // [2 h]
    float* rr;       // [2 h]
    double* li;      // [2 h]
};

__device__ __forceinline__ ProxWs prox_ws(void* ws, int h) {
    ProxWs w;
    w.li = static_cast<double*>(ws);
    w.A = reinterpret_cast<float*>(w.li + 2 * h);
    w.rinv = w.A + (int64_t)2 * h * h;
    w.rr = w.rinv + 2 * h;
    return w;
}

__global__ void __launch_bounds__(GDA_WAVE) k_prox_rows(const float* __restrict__ ppmi_s, int64_t ld_s, int ns,
                                                        const float* __restrict__ ppmi_t, int64_t ld_t, int nt,
                                                        const int64_t* __restrict__ pidx, const float* __restrict__ z,
                                                        int h, int e, void* ws) {
    const int i = blockIdx.x, dom = blockIdx.y, t = threadIdx.x;
    const float* P = dom ? ppmi_t : ppmi_s;
    const int64_t ld = dom ? ld_t : ld_s;
    const int np = dom ? nt : ns;
    const int64_t* idx = pidx + (int64_t)dom * h;
    ProxWs w = prox_ws(ws, h);
    float* row = w.A + ((int64_t)dom * h + i) * h;
    for (int j = t; j < h; j += GDA_WAVE) row[j] = ppmi_block_entry(P, ld, np, idx, i, j);
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int j = 0; j < h; ++j) s += (double)row[j];
        w.rinv[dom * h + i] = 1.f / ((float)s + 1e-12f);
        const float* ei = z + ((int64_t)dom * h + i) * e;
        float r = 0.f;
        for (int c = 0; c < e; ++c) {
            const float v = fmaxf(ei[c], 0.f);
            r += v * v;
        }
        w.rr[dom * h + i] = r;
    }
}

__global__ void __launch_bounds__(TB) k_prox_grad(const float* __restrict__ z, int h, int e, float pair_weight,
                                                  void* ws, float* __restrict__ gz) {
    __shared__ double wj[GDA_ACDNE_MAX_HALF], term[GDA_ACDNE_MAX_HALF];
    const int k = blockIdx.x, dom = blockIdx.y, t = threadIdx.x;
    ProxWs w = prox_ws(ws, h);
    const float* A = w.A + (int64_t)dom * h * h;
    const float* rinv = w.rinv + dom * h;
    const float* rr = w.rr + dom * h;
    const float* E = z + (int64_t)dom * h * e;
    for (int j = t; j < h; j += TB) {
        const double a_kj = (double)rinv[k] * (double)A[k * h + j];
        const double a_jk = (double)rinv[j] * (double)A[j * h + k];
        float dot = 0.f;
        for (int c = 0; c < e; ++c) dot += fmaxf(E[(int64_t)k * e + c], 0.f) * fmaxf(E[(int64_t)j * e + c], 0.f);
        wj[j] = a_kj + a_jk;
        term[j] = a_kj * (double)((rr[k] - 2.f * dot) + rr[j]);
    }
    __syncthreads();
    __shared__ double rc;
    if (t == 0) {
        double l = 0.0, r = 0.0;
        for (int j = 0; j < h; ++j) {
            l += term[j];
            r += wj[j];                  // sum_j a_kj + sum_j a_jk
        }
        w.li[dom * h + k] = l;
        rc = r;
    }
    __syncthreads();
    const double scale = 2.0 * (double)pair_weight / (double)h;
    for (int c = t; c < e; c += TB) {
        double s = rc * (double)fmaxf(E[(int64_t)k * e + c], 0.f);
        for (int j = 0; j < h; ++j) s -= wj[j] * (double)fmaxf(E[(int64_t)j * e + c], 0.f);
        gz[((int64_t)dom * h + k) * e + c] = (float)(scale * s);
    }
}

__global__ void k_prox_sum(int h, void* ws, double* __restrict__ loss) {
    const int dom = threadIdx.x;
    if (dom >= 2) return;
    ProxWs w = prox_ws(ws, h);
    double l = 0.0;
    for (int i = 0; i < h; ++i) l += w.li[dom * h + i];
    loss[dom] = l / (double)h;
}

struct HeadArgs {
    const float* z;            // [m, e] pre-activation of emb
    const float* gprox;        // [m, e] proximity gradient w.r.t. emb
    const float* a_s;          // [h, h] the source half's normalised block (DMGNN), or null: no propagation (ACDNE)
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

// bytes of HeadArgs::ws, rounded up to 8: the double terms follow
inline size_t heads_ws_float_bytes(int64_t h, int64_t e, int64_t c) {
    return gda_align_up((size_t)(2 * h * e + 8 * h * DH + 3 * h * c + 4 * h) * sizeof(float), 8);
}

// One phase of the heads per launch; a phase is a list of independent work items (one output element each, its sum in
// a fixed order) spread over the whole grid.  Phase k reads only what phases < k wrote.  With A.a_s null L' = L and
// dL = dL' (ACDNE); every other line is common to the two trainers.
__global__ void __launch_bounds__(TB) k_heads(HeadArgs A, int phase) {
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
                    float s = L[i * C + o];
                    if (A.a_s) {
                        float t = 0.f;
                        for (int j = 0; j < h; ++j) t += A.a_s[i * h + j] * L[j * C + o];
                        s = s + t;
                    }
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
    } else if (phase == 3) {                           // dh2, gW3, gb3; dL = dL' (+ A_s^T dL'); the loss
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
                float g = dlp[q];
                if (A.a_s) {
                    float s = 0.f;
                    for (int k = 0; k < h; ++k) s += A.a_s[k * h + i] * dlp[k * C + o];
                    g = g + s;
                }
                dl[q] = g;
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

__global__ void __launch_bounds__(TB) k_predict(const float* __restrict__ z, int64_t n, int e,
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

}  // namespace

extern "C" size_t gda_acdne_ppmi_workspace_bytes(int64_t n) {
    if (n < 1) return 256;
    const int64_t ld = (n + 3) / 4 * 4;
    return (size_t)(gda_cdiv(n, CS_SLAB) * ld + ld) * sizeof(float);
}

extern "C" int gda_acdne_ppmi_f32(const int32_t* rowptr, const int32_t* col, const float* cnt, int64_t n, int step,
                                  float* pval, float* buf_a, float* buf_b, float* buf_c, void* workspace,
                                  size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX / 2 || step < 1) return GDA_E_SIZE;
    if (!rowptr || !col || !cnt || !pval || !buf_a || !buf_b || !workspace) return GDA_E_NULL;
    if (step >= 3 && !buf_c) return GDA_E_NULL;
    if (workspace_bytes < gda_acdne_ppmi_workspace_bytes(n)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ld = (n + 3) / 4 * 4;
    const int ni = (int)n;
    // a (the sum) lives in buf_a; the powers ping-pong between buf_b and buf_c
    k_tran<<<ni, TB, 0, s>>>(rowptr, col, cnt, ni, ld, pval, step >= 2 ? buf_b : nullptr, buf_a);
    GDA_LAUNCH_CHECK();
    float* prev = buf_b;
    float* next = buf_c;
    const dim3 pg((unsigned)ni, (unsigned)gda_cdiv(ld, PW_COLS));
    for (int k = 2; k <= step; ++k) {
        k_power<<<pg, TB, 0, s>>>(rowptr, col, pval, ld, prev, k < step ? next : nullptr, buf_a, (float)k);
        GDA_LAUNCH_CHECK();
        float* tmp = prev;
        prev = next;
        next = tmp;
    }
    k_rownorm<<<ni, TB, 0, s>>>(buf_a, ni, ld);
    GDA_LAUNCH_CHECK();
    float* part = static_cast<float*>(workspace);
    const int slabs = (int)gda_cdiv(n, CS_SLAB);
    float* colsum = part + (int64_t)slabs * ld;
    k_colsum_partial<<<dim3((unsigned)gda_cdiv(n, TB), (unsigned)slabs), TB, 0, s>>>(buf_a, ni, ld, part);
    GDA_LAUNCH_CHECK();
    k_colsum_final<<<(unsigned)gda_cdiv(n, TB), TB, 0, s>>>(part, slabs, ni, ld, colsum);
    GDA_LAUNCH_CHECK();
    k_ppmi<<<ni, TB, 0, s>>>(buf_a, ni, ld, colsum, buf_b);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_acdne_xnei_f32(const float* na, int64_t n, int64_t ld, const int32_t* xrowptr, const int32_t* xcol,
                                  const float* xval, int64_t f, float* out, int64_t ldo, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || ld < n || f < 1 || ldo < f) return GDA_E_SIZE;
    if ((size_t)f * sizeof(float) > 160 * 1024) return GDA_E_UNSUPPORTED;
    if (!na || !xrowptr || !xcol || !xval || !out) return GDA_E_NULL;
    const size_t lds = (size_t)f * sizeof(float);
    if (lds > 64 * 1024) GDA_LDS_ATTR_ONCE(k_xnei, 160 * 1024);
    k_xnei<<<(unsigned)n, GDA_WAVE, lds, (hipStream_t)stream>>>(na, (int)n, ld, xrowptr, xcol, xval, (int)f, out, ldo);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_acdne_prox_workspace_bytes(int64_t h) {
    if (h < 1) return 256;
    return (size_t)2 * h * sizeof(double) + (size_t)(2 * h * h + 4 * h) * sizeof(float);
}

extern "C" int gda_acdne_prox_f32(const float* ppmi_s, int64_t ld_s, int64_t ns, const float* ppmi_t, int64_t ld_t,
                                  int64_t nt, const int64_t* pidx, const float* z, int64_t h, int64_t e,
                                  float pair_weight, double* loss, float* gz, void* workspace, size_t workspace_bytes,
                                  gda_stream_t stream) {
    if (h < 1 || h > GDA_ACDNE_MAX_HALF || e < 1 || e > 4096 || ns < 1 || nt < 1 || ns >= INT32_MAX ||
        nt >= INT32_MAX || ld_s < ns || ld_t < nt)
        return GDA_E_SIZE;
    if (!ppmi_s || !ppmi_t || !pidx || !z || !loss || !gz || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_acdne_prox_workspace_bytes(h)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)h, 2);
    k_prox_rows<<<grid, GDA_WAVE, 0, s>>>(ppmi_s, ld_s, (int)ns, ppmi_t, ld_t, (int)nt, pidx, z, (int)h, (int)e,
                                          workspace);
    GDA_LAUNCH_CHECK();
    k_prox_grad<<<grid, TB, 0, s>>>(z, (int)h, (int)e, pair_weight, workspace, gz);
    GDA_LAUNCH_CHECK();
    k_prox_sum<<<1, GDA_WAVE, 0, s>>>((int)h, workspace, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_acdne_heads_workspace_bytes(int64_t h, int64_t e, int64_t c) {
    if (h < 1 || e < 1 || c < 1) return 256;
    return heads_ws_float_bytes(h, e, c) + (size_t)3 * h * sizeof(double);
}

extern "C" size_t gda_dmgnn_heads_workspace_bytes(int64_t h, int64_t e, int64_t c) {
    return gda_acdne_heads_workspace_bytes(h, e, c);
}

// The two heads entry points: a_s is required with prop (DMGNN) and null without (ACDNE).
static int launch_heads(const float* z, const float* gprox, const float* a_s, bool prop, int64_t h, int64_t e,
                        int64_t c, const float* const* w, const int64_t* y, int64_t ny, const int64_t* rows,
                        const float* alpha, const double* prox, float pair_weight, float* dz, float* const* g,
                        double* loss, double* loss_acc, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (h < 1 || h > GDA_ACDNE_MAX_HALF || e < 1 || e > 4096 || c < 1 || c > 4096 || ny < 1) return GDA_E_SIZE;
    if (!z || !gprox || (prop && !a_s) || !w || !y || !rows || !alpha || !prox || !dz || !g || !loss || !workspace)
        return GDA_E_NULL;
    for (int k = 0; k < 8; ++k)
        if (!w[k] || !g[k]) return GDA_E_NULL;
    if (workspace_bytes < gda_acdne_heads_workspace_bytes(h, e, c)) return GDA_E_WORKSPACE;
    HeadArgs A;
    A.z = z;
    A.gprox = gprox;
    A.a_s = a_s;
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
    A.ws = static_cast<float*>(workspace);
    A.terms = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + heads_ws_float_bytes(h, e, c));
    A.dz = dz;
    A.gwc = g[0]; A.gbc = g[1]; A.gw1 = g[2]; A.gb1 = g[3]; A.gw2 = g[4]; A.gb2 = g[5]; A.gw3 = g[6]; A.gb3 = g[7];
    A.loss = loss;
    A.loss_acc = loss_acc;
    const int64_t work[6] = {m * e + m * DH + h * c, m * DH, m, m * DH + 2 * DH + 3 + h * c,
                             m * DH + DH * DH + DH + c * e + c, DH * e + DH + m * e};
    for (int phase = 0; phase < 6; ++phase) {
        const int64_t blocks = gda_cdiv(work[phase], TB);
        k_heads<<<(unsigned)(blocks < HEAD_MAX_BLOCKS ? blocks : HEAD_MAX_BLOCKS), TB, 0, (hipStream_t)stream>>>(A, phase);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

extern "C" int gda_acdne_heads_f32(const float* z, const float* gprox, int64_t h, int64_t e, int64_t c,
                                   const float* const* w, const int64_t* y, int64_t ny, const int64_t* rows,
                                   const float* alpha, const double* prox, float pair_weight, float* dz,
                                   float* const* g, double* loss, double* loss_acc, void* workspace,
                                   size_t workspace_bytes, gda_stream_t stream) {
    return launch_heads(z, gprox, nullptr, false, h, e, c, w, y, ny, rows, alpha, prox, pair_weight, dz, g, loss,
                        loss_acc, workspace, workspace_bytes, stream);
}

extern "C" int gda_dmgnn_heads_f32(const float* z, const float* gprox, const float* a_blocks, int64_t h, int64_t e,
                                   int64_t c, const float* const* w, const int64_t* y, int64_t ny, const int64_t* rows,
                                   const float* alpha, const double* prox, float pair_weight, float* dz,
                                   float* const* g, double* loss, double* loss_acc, void* workspace,
                                   size_t workspace_bytes, gda_stream_t stream) {
    return launch_heads(z, gprox, a_blocks, true, h, e, c, w, y, ny, rows, alpha, prox, pair_weight, dz, g, loss,
                        loss_acc, workspace, workspace_bytes, stream);
}

extern "C" int gda_acdne_predict_f32(const float* z, int64_t n, int64_t e, const float* wc, const float* bc, int64_t c,
                                     float* prob, gda_stream_t stream) {
    if (n < 1 || e < 1 || c < 1 || c > 4096 || e > 4096) return GDA_E_SIZE;
    if (!z || !wc || !bc || !prob) return GDA_E_NULL;
    k_predict<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(z, n, (int)e, wc, bc, (int)c, prob);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
