// GTrans (pygda/models/gtrans.py, pygda/utils/perturb.py): a GCN aggregation whose normalised values are a
// differentiable function of one flip weight per undirected edge, the three-view cosine loss and the budget projection.
// fp32, no atomics, gfx950.  The CSR pattern (by destination and by source, one self-loop slot per row) is fixed for a
// fit; a gda_wgcn_plan carries it with what the kernels need beside it: the destination of every entry, the parameter
// that feeds it, the entries each parameter feeds and both CSRs cut into segments of at most GDA_WGCN_SEGMENT entries,
// none across two rows.  Every per-node sum is one lane group per segment in stored order and then the row's segments in
// order, so a hub row is as wide as it is long and two runs give the same bits.  The aggregation itself is gda_spmm.hip
// on the value arrays that gda_wgcn_norm_f32 refreshes.  See include/gda_hip.h for the contract of each entry point.
#include "gda_common.h"
#include "gda_dropout.h"
#include "gda_reduce.h"

#include <math.h>

namespace {

constexpr int TB = 256;                       // threads per workgroup (4 waves)
constexpr int SG = 8;                         // lanes per segment
constexpr int EG = 16;                        // lanes per entry of the edge-gradient kernel, per row of the loss kernel
constexpr int PTB = 1024;                     // the one-workgroup projection
constexpr int NH = GDA_GTRANS_PROJECT_HALVINGS;
constexpr float BISECT_EPS = 1e-5f;           // the reference's bisection width

__device__ __forceinline__ bool in_range(int idx, int64_t n) { return (unsigned)idx < (unsigned)n; }

// ---- norm, first launch: a lane group per segment of the by-destination CSR -- the new raw weights, the fold sign times
//      the keep bit, keep * w and the segment's share of the degree -------------------------------------------------------
__global__ void __launch_bounds__(TB)
k_wgcn_seg(gda_wgcn_plan pl, const float* __restrict__ w_prev, const float* __restrict__ p,
           const float* __restrict__ keep, float p_drop, uint64_t seed, const int64_t* __restrict__ step, uint32_t site,
           float* __restrict__ w, float* __restrict__ dsign, float* __restrict__ kw, float* __restrict__ segpart) {
    const int lane = threadIdx.x % SG;
    const int64_t s = (int64_t)blockIdx.x * (TB / SG) + threadIdx.x / SG;
    const bool live = s < pl.nseg;
    float acc = 0.f;
    if (live) {
        const bool draw = keep == nullptr && p_drop > 0.f;
        const uint32_t thresh = dropout_thresh(p_drop);
        const uint64_t st = draw && step != nullptr ? (uint64_t)step[0] : 0;
        const int b = pl.seg_off[s], e = pl.seg_off[s + 1];
        for (int q = b + lane; q < e; q += SG) {
            if (!in_range(q, pl.nnz)) continue;
            const int u = pl.kidx[q], pos = pl.epos[q];
            float x = w_prev[q], sg = 1.f;
            if (p != nullptr && in_range(u, pl.mu)) {
                // the group's parameters in listed order: their sum, or (to_symmetric's op='mean') their mean
                const int gb = pl.gptr[u], ge = pl.gptr[u + 1];
                float pm = 0.f;
                for (int j = gb; j < ge; ++j)
                    if (in_range(j, pl.m) && in_range(pl.gidx[j], pl.m)) pm += p[pl.gidx[j]];
                if (pl.mean && ge - gb > 1) pm = pm / (float)(ge - gb);
                x += pm;
            }
            // the reference's "allow removal of edges": get_modified_adj folds EVERY coalesced weight above 1, also one
            // that no parameter feeds (a duplicate edge with row > col under make_undirected=False, a doubled self loop)
            if (p != nullptr && x > 1.f) {
                x = 2.f - x;
                sg = -1.f;
            }
            float kp = 1.f;                                     // a self-loop slot without a listed edge: pos < 0
            if (in_range(pos, pl.ec)) {
                if (keep != nullptr) kp = keep[pos];
                else if (draw) {
                    uint32_t r[4];
                    dropout_draw(seed, st, site, (uint64_t)pos >> 2, r);
                    kp = dropout_kept(r[pos & 3], thresh) ? 1.f : 0.f;
                }
            }
            w[q] = x;
            dsign[q] = sg * kp;
            // a listed self loop that is dropped leaves gcn_norm's unit loop behind
            const float v = kp == 0.f && pl.erow[q] == pl.colidx[q] ? 1.f : kp * x;
            kw[q] = v;
            acc += v;
        }
    }
    acc = group_sum<SG>(acc);
    if (live && lane == 0) segpart[s] = acc;
}

// ---- norm, second launch: a thread per node adds its segments in order; s = deg^-1/2, 0 where deg <= 0 -----------------
__global__ void __launch_bounds__(TB)
k_wgcn_rows(gda_wgcn_plan pl, const float* __restrict__ segpart, float* __restrict__ deg, float* __restrict__ sn) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= pl.n) return;
    float a = 0.f;
    for (int s = pl.row_seg[i]; s < pl.row_seg[i + 1]; ++s)
        if (in_range(s, pl.nseg)) a += segpart[s];
    deg[i] = a;
    sn[i] = a > 0.f ? 1.f / sqrtf(a) : 0.f;
}

// the normalised value of by-destination entry f: (s_src * keep w) * s_dst, gcn_norm's order of the two products
__device__ __forceinline__ float norm_val(const gda_wgcn_plan& pl, const float* kw, const float* sn, int f) {
    const int dst = pl.erow[f], src = pl.colidx[f];
    if (!in_range(dst, pl.n) || !in_range(src, pl.n)) return 0.f;
    return (sn[src] * kw[f]) * sn[dst];
}

// ---- norm, third launch: a thread per entry of either CSR ---------------------------------------------------------------
__global__ void __launch_bounds__(TB)
k_wgcn_vals(gda_wgcn_plan pl, const float* __restrict__ kw, const float* __restrict__ sn, float* __restrict__ val,
            float* __restrict__ t_val) {
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= pl.nnz) return;
    val[e] = norm_val(pl, kw, sn, (int)e);
    const int f = pl.t_to_fwd[e];
    t_val[e] = in_range(f, pl.nnz) ? norm_val(pl, kw, sn, f) : 0.f;
}

// ---- the SDDMM: gv_e = <G[dst_e], H[src_e]>, a group of EG lanes per stored entry (self loops included).  An entry is
//      the unit of work, so a hub row spreads over as many groups as it has entries. ---------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(TB)
k_wgcn_edge_grad(gda_wgcn_plan pl, const float* __restrict__ G, const float* __restrict__ H, int d,
                 float* __restrict__ gv) {
    const int lane = threadIdx.x % EG;
    const int64_t e = (int64_t)blockIdx.x * (TB / EG) + threadIdx.x / EG;
    const bool live = e < pl.nnz;
    float acc = 0.f;
    if (live) {
        const int dst = pl.erow[e], src = pl.colidx[e];
        if (in_range(dst, pl.n) && in_range(src, pl.n)) {
            const float* g = G + (int64_t)dst * d;
            const float* h = H + (int64_t)src * d;
            if (VEC) {
                for (int c = lane * 4; c < d; c += EG * 4) {
                    const float4 a = *reinterpret_cast<const float4*>(g + c);
                    const float4 b = *reinterpret_cast<const float4*>(h + c);
                    acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
                }
            } else {
                for (int c = lane; c < d; c += EG) acc += g[c] * h[c];
            }
        }
    }
    acc = group_sum<EG>(acc);
    if (live && lane == 0) gv[e] = acc;
}

// ---- chain, first launch: blockIdx.y = 0 the segments of the by-destination CSR (sum of gv kw s_src into a node),
//      1 those of the by-source CSR (sum of gv kw s_dst out of a node); a self loop is in both -----------------------------
__global__ void __launch_bounds__(TB)
k_wgcn_bwd_seg(gda_wgcn_plan pl, const float* __restrict__ gv, const float* __restrict__ kw, const float* __restrict__ sn,
               float* __restrict__ part_in, float* __restrict__ part_out) {
    const int lane = threadIdx.x % SG;
    const int64_t s = (int64_t)blockIdx.x * (TB / SG) + threadIdx.x / SG;
    const bool by_src = blockIdx.y == 1;
    const bool live = s < (by_src ? pl.t_nseg : pl.nseg);
    float acc = 0.f;
    if (live) {
        const int32_t* off = by_src ? pl.t_seg_off : pl.seg_off;
        for (int q = off[s] + lane; q < off[s + 1]; q += SG) {
            if (!in_range(q, pl.nnz)) continue;
            const int f = by_src ? pl.t_to_fwd[q] : q;
            if (!in_range(f, pl.nnz)) continue;
            const int other = by_src ? pl.erow[f] : pl.colidx[f];
            if (in_range(other, pl.n)) acc += (gv[f] * kw[f]) * sn[other];
        }
    }
    acc = group_sum<SG>(acc);
    if (live && lane == 0) (by_src ? part_out : part_in)[s] = acc;
}

// ---- chain, second launch: dL/ds_i and dL/ddeg_i = -1/2 s_i^3 dL/ds_i ---------------------------------------------------
__global__ void __launch_bounds__(TB)
k_wgcn_bwd_rows(gda_wgcn_plan pl, const float* __restrict__ part_in, const float* __restrict__ part_out,
                const float* __restrict__ sn, float* __restrict__ ddeg) {
    const int64_t i = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (i >= pl.n) return;
    float a = 0.f, b = 0.f;
    for (int s = pl.row_seg[i]; s < pl.row_seg[i + 1]; ++s)
        if (in_range(s, pl.nseg)) a += part_in[s];
    for (int s = pl.t_row_seg[i]; s < pl.t_row_seg[i + 1]; ++s)
        if (in_range(s, pl.t_nseg)) b += part_out[s];
    const float si = sn[i];
    ddeg[i] = -0.5f * si * si * si * (a + b);
}

// ---- chain, third launch: a thread per parameter gathers the at most two entries it feeds ------------------------------
__global__ void __launch_bounds__(TB)
k_wgcn_bwd_param(gda_wgcn_plan pl, const float* __restrict__ gv, const float* __restrict__ sn,
                 const float* __restrict__ dsign, const float* __restrict__ ddeg, float* __restrict__ dp) {
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= pl.m) return;
    const int u = pl.pgrp[k];
    if (!in_range(u, pl.mu)) {
        dp[k] = 0.f;
        return;
    }
    const int cnt = pl.gptr[u + 1] - pl.gptr[u];
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int e = pl.pent[2 * u + j];
        if (!in_range(e, pl.nnz)) continue;
        const int dst = pl.erow[e], src = pl.colidx[e];
        if (!in_range(dst, pl.n) || !in_range(src, pl.n)) continue;
        a += dsign[e] * ((sn[src] * sn[dst]) * gv[e] + ddeg[dst]);
    }
    dp[k] = pl.mean && cnt > 1 ? a / (float)cnt : a;
}

// ---- the loss: EG lanes per row; c12 = cos(o1, o2), c23 = cos(o2, o3) with the reference's norm + 1e-15 ------------------
// sum over an aligned group of EG lanes, in double
__device__ __forceinline__ double group_sum_d(double v) {
#pragma unroll
    for (int off = EG / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, EG);
    return v;
}

__global__ void __launch_bounds__(TB)
k_gtrans_loss_rows(const float* __restrict__ o1, const float* __restrict__ o2, const float* __restrict__ o3, int64_t n,
                   int d, float margin, float* __restrict__ g1, float* __restrict__ g2, float* __restrict__ g3,
                   double* __restrict__ part) {
    __shared__ double red[TB];
    const int lane = threadIdx.x % EG;
    const int64_t i = (int64_t)blockIdx.x * (TB / EG) + threadIdx.x / EG;
    const bool row = i < n;
    const int64_t base = (row ? i : 0) * d;
    // three passes over the row's d columns (the second and third hit the cache): the norms, the cosines of the
    // normalised rows -- torch's own order of operations, t1 = o1 / (|o1| + 1e-15) first --, the gradients
    // (the norms and the cosines in double: the loss is the small difference of two means near 1, and float32 sums of
    // its terms would leave an error of the size of the loss's own last digits)
    double q1 = 0.0, q2 = 0.0, q3 = 0.0;
    if (row)
        for (int c = lane; c < d; c += EG) {
            const double a = o1[base + c], b = o2[base + c], e = o3[base + c];
            q1 += a * a;
            q2 += b * b;
            q3 += e * e;
        }
    const double m1 = sqrt(group_sum_d(q1)), m2 = sqrt(group_sum_d(q2)), m3 = sqrt(group_sum_d(q3));
    const double f1 = m1 + 1e-15, f2 = m2 + 1e-15, f3 = m3 + 1e-15;
    double x12 = 0.0, x23 = 0.0;
    if (row)
        for (int c = lane; c < d; c += EG) {
            const double v = (double)o2[base + c] / f2;
            x12 += ((double)o1[base + c] / f1) * v;
            x23 += v * ((double)o3[base + c] / f3);
        }
    x12 = group_sum_d(x12);
    x23 = group_sum_d(x23);
    const float n1 = (float)m1, n2 = (float)m2, n3 = (float)m3;
    const float e1 = n1 + 1e-15f, e2 = n2 + 1e-15f, e3 = n3 + 1e-15f;
    const float c12 = (float)x12, c23 = (float)x23;
    const bool plain = margin == -1.f;
    const double t2 = plain ? 1.0 - x23 : fmax(1.0 - x23 - (double)margin, 0.0);
    const float on = plain || (1.0 - x23 - (double)margin) > 0.0 ? 1.f : 0.f;       // relu'
    if (row) {
        // d c(a, b) / d a = (b / eb - c a / na) / ea: the second term is the norm's, 0 at a zero row
        const float inv = 1.f / (float)n;
        const float k1 = inv / e1, k2 = inv / e2, k3 = on * inv / e3;
        const bool z1 = !(n1 > 0.f), z2 = !(n2 > 0.f), z3 = !(n3 > 0.f);
        for (int c = lane; c < d; c += EG) {
            const float a = o1[base + c], b = o2[base + c], e = o3[base + c];
            const float u = a / e1, v = b / e2, w = e / e3;
            const float ah = z1 ? 0.f : a / n1, bh = z2 ? 0.f : b / n2, eh = z3 ? 0.f : e / n3;   // exactly +-1 at d = 1
            g1[base + c] = -k1 * (v - c12 * ah);
            g2[base + c] = -k2 * (u - c12 * bh) + on * k2 * (w - c23 * bh);
            g3[base + c] = k3 * (v - c23 * eh);
        }
    }
    const bool head = row && lane == 0;
    const double s1 = block_sum_d(head ? 1.0 - x12 : 0.0, red);
    const double s2 = block_sum_d(head ? t2 : 0.0, red);
    if (threadIdx.x == 0) {
        part[2 * (int64_t)blockIdx.x] = s1;
        part[2 * (int64_t)blockIdx.x + 1] = s2;
    }
}

__global__ void __launch_bounds__(TB)
k_gtrans_loss_finalise(const double* __restrict__ part, int64_t nb, int64_t n, float* __restrict__ out) {
    __shared__ double red[TB];
    double a = 0.0, b = 0.0;
    for (int64_t q = threadIdx.x; q < nb; q += TB) {
        a += part[2 * q];
        b += part[2 * q + 1];
    }
    a = block_sum_d(a, red) / (double)n;
    b = block_sum_d(b, red) / (double)n;
    if (threadIdx.x == 0) {
        out[0] = (float)(a - b);
        out[1] = (float)a;
        out[2] = (float)b;
    }
}

// ---- project: the reference's bisection as a fixed sequence of stages, the same on one workgroup and as a chain of
//      launches.  Stage 0 clamps p to >= lo (the clamp that follows the Adam step) and takes sum clamp(p, 0, 1), min and
//      max; stage 1 opens the bracket [min - 1, max] and evaluates f at its left end; stages 2 .. NH + 1 evaluate f at
//      the midpoint of the stage before; the last stage takes the final decision and writes p.  f(x) = sum clamp(p - x,
//      0, 1) - budget.  `done` freezes miu exactly where the reference's loop breaks. ----------------------------------------
struct Bisect {
    float a, b, fa, miu, done, active;
};

// the state after the sum `sum` of stage `stage`'s predecessor has arrived; returns the point the next sum is taken at
__device__ __forceinline__ void bisect_advance(Bisect& st, int stage, double sum, float mn, float mx, float budget) {
    const float F = (float)sum - budget;
    if (stage == 1) {
        st.active = (float)sum > budget ? 1.f : 0.f;
        st.a = mn - 1.f;
        st.b = mx;
        st.fa = 0.f;
        st.miu = st.a;
        st.done = st.active > 0.f ? 0.f : 1.f;
        return;
    }
    if (stage == 2) {
        st.fa = F;                                              // f at the left end
        if (st.done == 0.f) st.miu = (st.a + st.b) / 2;
        return;
    }
    if (st.done != 0.f) return;
    if (F == 0.f) {
        st.done = 1.f;
        return;
    }
    if (F * st.fa < 0.f) st.b = st.miu;
    else {
        st.a = st.miu;
        st.fa = F;
    }
    if (st.b - st.a <= BISECT_EPS) {
        st.done = 1.f;
        return;
    }
    st.miu = (st.a + st.b) / 2;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ float project_value(const Bisect& st, float v, float lo) {
    const float x = st.active > 0.f ? v - st.miu : v;
    return fminf(fmaxf(x, lo), 1.f - lo);
}

__device__ __forceinline__ float block_min_f(float v, float* red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fminf(red[t], red[t + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(PTB)
k_gtrans_project_one(float* __restrict__ p, int64_t m, float budget, float lo) {
    __shared__ double red[PTB];
    float* redf = reinterpret_cast<float*>(red);
    float s0 = 0.f, mn = INFINITY, mx = -INFINITY;
    for (int64_t q = threadIdx.x; q < m; q += PTB) {
        const float v = fmaxf(p[q], lo);
        p[q] = v;
        s0 += clamp01(v);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    double sum = block_sum_d((double)s0, red);
    mn = block_min_f(mn, redf);
    mx = -block_min_f(-mx, redf);
    Bisect st = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    bisect_advance(st, 1, sum, mn, mx, budget);
    for (int stage = 2; stage <= NH + 2; ++stage) {
        float acc = 0.f;
        if (st.done == 0.f || stage == 2)
            for (int64_t q = threadIdx.x; q < m; q += PTB) acc += clamp01(p[q] - st.miu);
        sum = block_sum_d((double)acc, red);
        bisect_advance(st, stage, sum, mn, mx, budget);
    }
    for (int64_t q = threadIdx.x; q < m; q += PTB) p[q] = project_value(st, p[q], lo);
}

// One stage of the chain.  Every workgroup folds the partials of the stage before in the same order and advances the
// state itself; workgroup 0 writes it to this stage's slot, which the next launch reads.
__global__ void __launch_bounds__(TB)
k_gtrans_project_chain(float* __restrict__ p, int64_t m, int stage, float budget, float lo, Bisect* __restrict__ states,
                       const double* __restrict__ prev, double* __restrict__ cur, int nb) {
    __shared__ double red[TB];
    float* redf = reinterpret_cast<float*>(red);
    Bisect st = {0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    if (stage >= 1) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nb; b += TB) a += prev[b];
        const double sum = block_sum_d(a, red);
        float mn = 0.f, mx = 0.f;
        if (stage == 1) {
            float x = INFINITY, y = INFINITY;
            for (int b = threadIdx.x; b < nb; b += TB) {
                x = fminf(x, (float)prev[nb + b]);
                y = fminf(y, -(float)prev[2 * nb + b]);
            }
            mn = block_min_f(x, redf);
            mx = -block_min_f(y, redf);
        } else {
            st = states[stage - 1];
        }
        bisect_advance(st, stage, sum, mn, mx, budget);
        if (blockIdx.x == 0 && threadIdx.x == 0) states[stage] = st;
    }
    const int64_t stride = (int64_t)gridDim.x * TB;
    const int64_t first = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (stage == NH + 2) {
        for (int64_t q = first; q < m; q += stride) p[q] = project_value(st, p[q], lo);
        return;
    }
    float acc = 0.f, mn = INFINITY, mx = -INFINITY;
    if (stage == 0) {
        for (int64_t q = first; q < m; q += stride) {
            const float v = fmaxf(p[q], lo);
            p[q] = v;
            acc += clamp01(v);
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
    } else if (st.done == 0.f || stage == 1) {
        for (int64_t q = first; q < m; q += stride) acc += clamp01(p[q] - st.miu);
    }
    const double sum = block_sum_d((double)acc, red);
    if (stage == 0) {
        mn = block_min_f(mn, redf);
        mx = -block_min_f(-mx, redf);
    }
    if (threadIdx.x == 0) {
        cur[blockIdx.x] = sum;
        if (stage == 0) {
            cur[nb + blockIdx.x] = (double)mn;
            cur[2 * nb + blockIdx.x] = (double)mx;
        }
    }
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

const int64_t LIM = (int64_t)1 << 31;

int plan_status(const gda_wgcn_plan* pl) {
    if (!pl) return GDA_E_NULL;
    if (pl->n < 1 || pl->nnz < pl->n || pl->m < 0 || pl->mu < 0 || pl->mu > pl->m || pl->ec < 0 || pl->ec > pl->nnz || pl->nnz >= LIM || pl->n >= LIM || pl->m >= LIM / 2) return GDA_E_SIZE;
    if (pl->nseg < pl->n || pl->t_nseg < pl->n || pl->nseg > pl->n + pl->nnz / GDA_WGCN_SEGMENT + 1
        || pl->t_nseg > pl->n + pl->nnz / GDA_WGCN_SEGMENT + 1)
        return GDA_E_SIZE;
    if (!pl->rowptr || !pl->colidx || !pl->t_rowptr || !pl->t_colidx || !pl->t_to_fwd || !pl->erow || !pl->epos || !pl->kidx
        || (pl->m > 0 && (!pl->pent || !pl->gptr || !pl->gidx || !pl->pgrp)) || !pl->seg_off || !pl->row_seg || !pl->t_seg_off || !pl->t_row_seg)
        return GDA_E_NULL;
    return GDA_OK;
}

int project_blocks(int64_t m) { return (int)(gda_cdiv(m, (int64_t)TB * 8) < 256 ? gda_cdiv(m, (int64_t)TB * 8) : 256); }

}  // namespace

extern "C" size_t gda_wgcn_workspace_bytes(int64_t n, int64_t nnz) {
    if (n < 1 || nnz < n || nnz >= LIM) return 256;
    const size_t nseg = (size_t)(n + nnz / GDA_WGCN_SEGMENT + 1);
    return gda_align_up((2 * nseg + (size_t)n) * sizeof(float), 256);
}

extern "C" int gda_wgcn_norm_f32(const gda_wgcn_plan* plan, const float* w_prev, const float* p, const float* keep,
                                 float p_drop, uint64_t seed, const int64_t* step, uint32_t site, float* w, float* dsign,
                                 float* kw, float* deg, float* s, float* val, float* t_val, void* workspace,
                                 size_t workspace_bytes, gda_stream_t stream) {
    const int bad = plan_status(plan);
    if (bad) return bad;
    if (!(p_drop >= 0.f && p_drop < 1.f)) return GDA_E_SIZE;
    if (!w_prev || !w || !dsign || !kw || !deg || !s || !val || !t_val || !workspace)
        return GDA_E_NULL;
    if (w == w_prev || kw == w_prev || dsign == w_prev) return GDA_E_ALIAS;
    if (!aligned(w_prev, 4) || !aligned(p, 4) || !aligned(w, 4) || !aligned(dsign, 4) || !aligned(kw, 4) || !aligned(deg, 4)
        || !aligned(s, 4) || !aligned(val, 4) || !aligned(t_val, 4) || !aligned(step, 8) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_wgcn_workspace_bytes(plan->n, plan->nnz)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* segpart = static_cast<float*>(workspace);
    k_wgcn_seg<<<(unsigned)gda_cdiv(plan->nseg, TB / SG), TB, 0, st>>>(*plan, w_prev, p, keep, p_drop, seed, step, site, w,
                                                                       dsign, kw, segpart);
    GDA_LAUNCH_CHECK();
    k_wgcn_rows<<<(unsigned)gda_cdiv(plan->n, TB), TB, 0, st>>>(*plan, segpart, deg, s);
    GDA_LAUNCH_CHECK();
    k_wgcn_vals<<<(unsigned)gda_cdiv(plan->nnz, TB), TB, 0, st>>>(*plan, kw, s, val, t_val);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_wgcn_edge_grad_f32(const gda_wgcn_plan* plan, const float* G, const float* H, int64_t d, float* gv,
                                      gda_stream_t stream) {
    const int bad = plan_status(plan);
    if (bad) return bad;
    if (d < 1) return GDA_E_SIZE;
    if (d > GDA_WGCN_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!G || !H || !gv) return GDA_E_NULL;
    if (!aligned(G, 4) || !aligned(H, 4) || !aligned(gv, 4)) return GDA_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)gda_cdiv(plan->nnz, TB / EG);
    if (d % 4 == 0 && aligned(G, 16) && aligned(H, 16))
        k_wgcn_edge_grad<true><<<grid, TB, 0, st>>>(*plan, G, H, (int)d, gv);
    else
        k_wgcn_edge_grad<false><<<grid, TB, 0, st>>>(*plan, G, H, (int)d, gv);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_wgcn_norm_bwd_f32(const gda_wgcn_plan* plan, const float* gv, const float* kw, const float* s,
                                     const float* dsign, float* dp, void* workspace, size_t workspace_bytes,
                                     gda_stream_t stream) {
    const int bad = plan_status(plan);
    if (bad) return bad;
    if (!gv || !kw || !s || !dsign || (plan->m > 0 && !dp) || !workspace) return GDA_E_NULL;
    if (!aligned(gv, 4) || !aligned(kw, 4) || !aligned(s, 4) || !aligned(dsign, 4) || !aligned(dp, 4)
        || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_wgcn_workspace_bytes(plan->n, plan->nnz)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t cap = (size_t)(plan->n + plan->nnz / GDA_WGCN_SEGMENT + 1);
    float* part_in = static_cast<float*>(workspace);
    float* part_out = part_in + cap;
    float* ddeg = part_out + cap;
    const int64_t most = plan->nseg > plan->t_nseg ? plan->nseg : plan->t_nseg;
    k_wgcn_bwd_seg<<<dim3((unsigned)gda_cdiv(most, TB / SG), 2), TB, 0, st>>>(*plan, gv, kw, s, part_in, part_out);
    GDA_LAUNCH_CHECK();
    k_wgcn_bwd_rows<<<(unsigned)gda_cdiv(plan->n, TB), TB, 0, st>>>(*plan, part_in, part_out, s, ddeg);
    GDA_LAUNCH_CHECK();
    if (plan->m > 0) {
        k_wgcn_bwd_param<<<(unsigned)gda_cdiv(plan->m, TB), TB, 0, st>>>(*plan, gv, s, dsign, ddeg, dp);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

extern "C" size_t gda_gtrans_loss_workspace_bytes(int64_t n) {
    if (n < 1 || n >= LIM) return 256;
    return gda_align_up((size_t)2 * gda_cdiv(n, TB / EG) * sizeof(double), 256);
}

extern "C" int gda_gtrans_loss_f32(const float* o1, const float* o2, const float* o3, int64_t n, int64_t d, float margin,
                                   float* out, float* g1, float* g2, float* g3, void* workspace, size_t workspace_bytes,
                                   gda_stream_t stream) {
    if (n < 1 || d < 1 || n >= LIM || d >= LIM || n * d >= LIM * 64) return GDA_E_SIZE;
    if (!o1 || !o2 || !o3 || !out || !g1 || !g2 || !g3 || !workspace) return GDA_E_NULL;
    if (!aligned(o1, 4) || !aligned(o2, 4) || !aligned(o3, 4) || !aligned(out, 4) || !aligned(g1, 4) || !aligned(g2, 4)
        || !aligned(g3, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_gtrans_loss_workspace_bytes(n)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = gda_cdiv(n, TB / EG);
    double* part = static_cast<double*>(workspace);
    k_gtrans_loss_rows<<<(unsigned)nb, TB, 0, st>>>(o1, o2, o3, n, (int)d, margin, g1, g2, g3, part);
    GDA_LAUNCH_CHECK();
    k_gtrans_loss_finalise<<<1, TB, 0, st>>>(part, nb, n, out);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_gtrans_project_workspace_bytes(int64_t m) {
    if (m < 1 || m >= LIM) return 256;
    if (m <= GDA_GTRANS_PROJECT_ONE_WG) return 256;
    return gda_align_up((size_t)(NH + 3) * sizeof(Bisect) + 64 + (size_t)2 * 3 * project_blocks(m) * sizeof(double), 256);
}

extern "C" int gda_gtrans_project_f32(float* p, int64_t m, float budget, float lo, void* workspace, size_t workspace_bytes,
                                      gda_stream_t stream) {
    if (m < 1 || m >= LIM || !(budget >= 0.f) || !(lo >= 0.f && lo < 0.5f)) return GDA_E_SIZE;
    if (!p || !workspace) return GDA_E_NULL;
    if (!aligned(p, 4) || !aligned(workspace, 16)) return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_gtrans_project_workspace_bytes(m)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (m <= GDA_GTRANS_PROJECT_ONE_WG) {
        k_gtrans_project_one<<<1, PTB, 0, st>>>(p, m, budget, lo);
        GDA_LAUNCH_CHECK();
        return GDA_OK;
    }
    const int nb = project_blocks(m);
    Bisect* states = static_cast<Bisect*>(workspace);
    double* buf = reinterpret_cast<double*>(static_cast<char*>(workspace)
                                            + gda_align_up((size_t)(NH + 3) * sizeof(Bisect), 64));
    for (int stage = 0; stage <= NH + 2; ++stage) {
        double* cur = buf + (size_t)(stage & 1) * 3 * nb;
        const double* prev = buf + (size_t)((stage + 1) & 1) * 3 * nb;
        k_gtrans_project_chain<<<nb, TB, 0, st>>>(p, m, stage, budget, lo, states, prev, cur, nb);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}
