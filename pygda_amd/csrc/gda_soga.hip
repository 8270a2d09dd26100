// SOGA (pygda/models/soga.py): the label-smoothed cross-entropy of its source phase and the whole adaptation term of
// its target phase -- information maximisation plus the InfoNCE terms over fixed index tables -- with the gradient
// with respect to the logits.  fp32, no atomics.  A row of C classes is owned by an aligned group of G = next_pow2(C)
// lanes, one class per lane; the probabilities live in a padded [N, G] buffer (pad classes hold 0), so a group gathers
// a row with one 4 G-byte request.  Every reduction over rows is per-workgroup partials folded in block order by a
// single-workgroup finalise, and the scatter of the InfoNCE gradient is a gather over a precomputed reverse index cut
// into segments, so two runs give the same bits.  See include/gda_hip.h for the contract of each entry point.
#include "gda_common.h"
#include "gda_reduce.h"

#include <math.h>

namespace {

constexpr int TB = 256;                       // threads per workgroup (4 waves)
constexpr int MAXC = GDA_SOGA_MAX_CLASSES;
constexpr float ENT_EPS = 1e-5f;              // the reference's entropy offset
constexpr double DIV_EPS = 1e-8;              // and its diversity offset

// ---- label-smoothed cross-entropy: loss rows, dlogits (1 / N applied) and arg-max hits, TB / G rows per workgroup ----
template <int G>
__global__ void __launch_bounds__(TB)
k_soga_smooth_ce(const float* __restrict__ Z, const int64_t* __restrict__ y, int n, int C, float eps,
                 float* __restrict__ dZ, float* __restrict__ lossp, float* __restrict__ hitp) {
    __shared__ float red[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n, live = row && lane < C;
    const float z = live ? Z[(int64_t)i * C + lane] : (row ? -INFINITY : 0.f);
    const float mx = group_max<G>(z);
    const float e = (live || !row) ? expf(z - mx) : 0.f;
    const float s = group_sum<G>(e);
    const float logp = z - mx - logf(s);
    const int label = row ? (int)y[i] : -1;
    const float t = (lane == label ? 1.f - eps : 0.f) + eps / (float)C;
    const float lrow = group_sum<G>(live ? -t * logp : 0.f);
    if (live) dZ[(int64_t)i * C + lane] = (e / s - t) / (float)n;
    // arg-max: the lowest class that holds the maximum
    int arg = (live && z == mx) ? lane : G;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) arg = min(arg, __shfl_xor(arg, off, G));
    const bool head = row && lane == 0;
    const float lsum = block_sum_f(head ? lrow : 0.f, red);
    const float hsum = block_sum_f(head && arg == label ? 1.f : 0.f, red);
    if (threadIdx.x == 0) {
        lossp[blockIdx.x] = lsum;
        hitp[blockIdx.x] = hsum;
    }
}

__global__ void __launch_bounds__(TB)
k_soga_ce_finalise(const float* __restrict__ lossp, const float* __restrict__ hitp, int nb, int n,
                   float* __restrict__ loss, double* __restrict__ stats) {
    __shared__ double red[TB];
    const double l = fold_d<TB>(lossp, nb, red) / (double)n;
    const double h = fold_d<TB>(hitp, nb, red);
    if (threadIdx.x == 0) {
        loss[0] = (float)l;
        if (stats != nullptr) {
            stats[0] = l;
            stats[1] = h;
        }
    }
}

// ---- row pass: P = softmax(Z) into [N, G], the block's entropy sum and its column sums of P --------------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_soga_rows(const float* __restrict__ Z, int n, int C, float* __restrict__ P, float* __restrict__ entp,
            float* __restrict__ colp) {
    __shared__ float tile[TB];
    __shared__ float red[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n, live = row && lane < C;
    const float z = live ? Z[(int64_t)i * C + lane] : (row ? -INFINITY : 0.f);
    const float mx = group_max<G>(z);
    const float e = (live || !row) ? expf(z - mx) : 0.f;
    const float p = e / group_sum<G>(e);
    if (row) P[(int64_t)i * G + lane] = p;                                   // pad classes: 0
    const float h = group_sum<G>(live ? -p * logf(p + ENT_EPS) : 0.f);
    tile[threadIdx.x] = row ? p : 0.f;
    const float hsum = block_sum_f(row && lane == 0 ? h : 0.f, red);       // (its barriers publish tile too)
    if (threadIdx.x < G) {
        float a = 0.f;
        for (int r = 0; r < TB / G; ++r) a += tile[r * G + threadIdx.x];     // the block's rows, in order
        colp[(int64_t)blockIdx.x * G + threadIdx.x] = a;
    }
    if (threadIdx.x == 0) entp[blockIdx.x] = hsum;
}

__device__ __forceinline__ int in_range(int idx, int n) { return (unsigned)idx < (unsigned)n ? idx : 0; }

// ---- pair pass: per table row of a view the K + 1 scores, sigma [V, M, K], the centre's gradient
//      gc = sum_k sigma_k P[n_k] - P[p] ([V, M, G], unweighted) and the row's loss log sum_k exp(s_k) - s_pos ----------
template <int G>
__global__ void __launch_bounds__(TB)
k_soga_pairs(const float* __restrict__ P, const int32_t* __restrict__ cen, const int32_t* __restrict__ pos,
             const int32_t* __restrict__ neg, int M, int K, int n, float* __restrict__ sigma,
             float* __restrict__ gc, float* __restrict__ lossp) {
    __shared__ float red[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < M;
    const int64_t r = (int64_t)blockIdx.y * M + (row ? i : M - 1);           // rows past the end redo the last one
    const float pc = P[(int64_t)in_range(cen[r], n) * G + lane];
    const float pp = P[(int64_t)in_range(pos[r], n) * G + lane];
    const float spos = group_sum<G>(pc * pp);
    const int32_t* nr = neg + r * K;
    float* sg = sigma + r * K;
    float S = 0.f, acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const float pn = P[(int64_t)in_range(nr[k], n) * G + lane];
        const float e = expf(group_sum<G>(pc * pn));                         // scores lie in [0, 1]: no shift needed
        S += e;
        acc += e * pn;
        if (row && lane == k % G) sg[k] = e;
    }
    if (row) {
        for (int k = lane; k < K; k += G) sg[k] = sg[k] / S;                 // each lane divides what it wrote itself
        gc[r * G + lane] = acc / S - pp;
    }
    const float lsum = block_sum_f(row && lane == 0 ? logf(S) - spos : 0.f, red);
    if (threadIdx.x == 0) lossp[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = lsum;
}

// ---- finalise (one workgroup): m = colsum / N and the diversity gradient into mg [2, G]; the four loss figures -------
__global__ void __launch_bounds__(TB)
k_soga_finalise(const float* __restrict__ entp, const float* __restrict__ colp, int nbr, const float* __restrict__ lossp,
                int nbp, int V, int n, int M, int C, int G, float lam0, float lam1, float* __restrict__ mg,
                float* __restrict__ out) {
    __shared__ double red[TB];
    __shared__ double cols[TB];
    const int t = threadIdx.x, lane = t % G, slices = TB / G;
    double a = 0.0;
    for (int b = t / G; b < nbr; b += slices) a += (double)colp[(int64_t)b * G + lane];
    cols[t] = a;
    __syncthreads();
    double dterm = 0.0;
    if (t < G) {
        double s = 0.0;
        for (int q = 0; q < slices; ++q) s += cols[q * G + t];
        const double m = s / (double)n;
        mg[t] = (float)m;
        mg[G + t] = t < C ? (float)((log(m + DIV_EPS) + m / (m + DIV_EPS)) / (double)n) : 0.f;
        dterm = t < C ? -m * log(m + DIV_EPS) : 0.0;
    }
    const double div = block_sum_d(dterm, red);
    const double ent = fold_d<TB>(entp, nbr, red) / (double)n;
    const double nce0 = fold_d<TB>(lossp, nbp, red) / (double)M;
    const double nce1 = V > 1 ? fold_d<TB>(lossp + nbp, nbp, red) / (double)M : 0.0;
    if (t == 0) {
        const double im = ent - div;
        out[0] = (float)(im + (double)lam0 * nce0 + (double)lam1 * nce1);
        out[1] = (float)im;
        out[2] = (float)nce0;
        out[3] = (float)nce1;
    }
}

// ---- node pass, first half: one group per segment of the reverse index, its entries in stored order -----------------
// rev_sig >= 0: a negative, the index of its sigma; -1 / -2: a positive of view 0 / 1; -3 / -4: a centre of view 0 / 1.
// rev_src: the row of P to gather (the table row's centre), or for a centre entry the row of gc.
template <int G>
__global__ void __launch_bounds__(TB)
k_soga_segments(const float* __restrict__ P, const float* __restrict__ gc, const float* __restrict__ sigma,
                const int32_t* __restrict__ seg_off, int nseg, const int32_t* __restrict__ rev_src,
                const int32_t* __restrict__ rev_sig, int n, int VM, int MK, int nsig, float w0, float w1,
                float* __restrict__ gpart) {
    const int lane = threadIdx.x % G;
    const int s = blockIdx.x * (TB / G) + threadIdx.x / G;
    if (s >= nseg) return;
    const int b = seg_off[s], e = seg_off[s + 1];
    float acc = 0.f;
    for (int q = b; q < e; ++q) {
        const int src = rev_src[q], sig = rev_sig[q];
        float coef;
        int view;
        const float* base = P;
        int limit = n;
        if (sig >= 0) {
            if (sig >= nsig) continue;
            coef = sigma[sig];
            view = sig >= MK;
        } else {
            view = (-sig - 1) & 1;
            coef = sig >= -2 ? -1.f : 1.f;
            if (sig < -2) {
                base = gc;
                limit = VM;
            }
        }
        if ((unsigned)src >= (unsigned)limit) continue;
        acc += (view ? w1 : w0) * coef * base[(int64_t)src * G + lane];
    }
    gpart[(int64_t)s * G + lane] = acc;
}

// ---- node pass, second half: a node's segments in order, the IM gradient, the softmax Jacobian ----------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_soga_nodes(const float* __restrict__ P, const float* __restrict__ gpart, const int32_t* __restrict__ node_seg,
             const float* __restrict__ mg, int n, int C, float* __restrict__ dZ) {
    const int lane = threadIdx.x % G;
    const int j = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = j < n;
    const int jj = row ? j : n - 1;
    const float p = P[(int64_t)jj * G + lane];
    float g = 0.f;
    for (int s = node_seg[jj]; s < node_seg[jj + 1]; ++s) g += gpart[(int64_t)s * G + lane];
    if (lane < C) g += (-logf(p + ENT_EPS) - p / (p + ENT_EPS)) / (float)n + mg[G + lane];
    else g = 0.f;
    const float dot = group_sum<G>(g * p);
    if (row && lane < C) dZ[(int64_t)j * C + lane] = p * (g - dot);
}

int group_of(int64_t C) {
    int g = 1;
    while (g < C) g <<= 1;
    return g;
}

size_t al4(size_t floats) { return gda_align_up(floats, 4); }               // sections start on 16 bytes

struct Layout {
    size_t P, entp, colp, sigma, gc, lossp, mg, gpart, total;
    int64_t nbr, nbp, max_seg;
};

Layout layout_of(int64_t n, int64_t C, int64_t M, int64_t K, int64_t V) {
    const int G = group_of(C);
    const int64_t rpb = TB / G;
    Layout L;
    L.nbr = gda_cdiv(n, rpb);
    L.nbp = gda_cdiv(M, rpb);
    L.max_seg = n + V * M * (K + 2) / GDA_SOGA_MIN_SEGMENT + 1;
    size_t o = 0;
    L.P = o;      o += al4((size_t)n * G);
    L.entp = o;   o += al4((size_t)L.nbr);
    L.colp = o;   o += al4((size_t)L.nbr * G);
    L.sigma = o;  o += al4((size_t)V * M * K);
    L.gc = o;     o += al4((size_t)V * M * G);
    L.lossp = o;  o += al4((size_t)2 * L.nbp);
    L.mg = o;     o += al4((size_t)2 * G);
    L.gpart = o;  o += al4((size_t)L.max_seg * G);
    L.total = o;
    return L;
}

bool adapt_dims_bad(int64_t n, int64_t C, int64_t M, int64_t K, int64_t V) {
    const int64_t lim = (int64_t)1 << 31;
    return n < 1 || C < 1 || M < 1 || K < 1 || V < 1 || V > 2 || n >= lim / 64 || M >= lim || K >= lim
           || V * M * (K + 2) >= lim;
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

#define SOGA_DISPATCH(G, CALL)                       \
    switch (G) {                                     \
        case 1: { constexpr int GG = 1; CALL; } break;   \
        case 2: { constexpr int GG = 2; CALL; } break;   \
        case 4: { constexpr int GG = 4; CALL; } break;   \
        case 8: { constexpr int GG = 8; CALL; } break;   \
        case 16: { constexpr int GG = 16; CALL; } break; \
        case 32: { constexpr int GG = 32; CALL; } break; \
        default: { constexpr int GG = 64; CALL; } break; \
    }

}  // namespace

extern "C" size_t gda_soga_ce_workspace_bytes(int64_t n, int64_t C) {
    if (n < 1 || C < 1 || C > MAXC) return 256;
    return gda_align_up((size_t)2 * gda_cdiv(n, TB / group_of(C)) * sizeof(float), 256);
}

extern "C" int gda_soga_smooth_ce_f32(const float* logits, const int64_t* labels, int64_t n, int64_t C, float epsilon,
                                      float* loss, float* dlogits, double* stats, void* workspace,
                                      size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || C < 1 || n >= ((int64_t)1 << 31) / 64) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (!logits || !labels || !loss || !dlogits || !workspace) return GDA_E_NULL;
    if (!aligned(logits, 4) || !aligned(dlogits, 4) || !aligned(loss, 4) || !aligned(labels, 8) || !aligned(stats, 8)
        || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_soga_ce_workspace_bytes(n, C)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int G = group_of(C);
    const int64_t nb = gda_cdiv(n, TB / G);
    float* lossp = static_cast<float*>(workspace);
    float* hitp = lossp + nb;
    SOGA_DISPATCH(G, (k_soga_smooth_ce<GG><<<(unsigned)nb, TB, 0, s>>>(logits, labels, (int)n, (int)C, epsilon, dlogits,
                                                                       lossp, hitp)));
    GDA_LAUNCH_CHECK();
    k_soga_ce_finalise<<<1, TB, 0, s>>>(lossp, hitp, (int)nb, (int)n, loss, stats);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_soga_workspace_bytes(int64_t n, int64_t C, int64_t M, int64_t K, int64_t V) {
    if (adapt_dims_bad(n, C, M, K, V) || C > MAXC) return 256;
    return gda_align_up(layout_of(n, C, M, K, V).total * sizeof(float), 256);
}

extern "C" int gda_soga_adapt_f32(const float* logits, int64_t n, int64_t C, const int32_t* center,
                                  const int32_t* positive, const int32_t* negative, int64_t V, int64_t M, int64_t K,
                                  float lambda_struct, float lambda_neigh, const int32_t* node_seg,
                                  const int32_t* seg_off, int64_t nseg, const int32_t* rev_src, const int32_t* rev_sig,
                                  int64_t nrev, float* out, float* dlogits, void* workspace, size_t workspace_bytes,
                                  gda_stream_t stream) {
    if (adapt_dims_bad(n, C, M, K, V)) return GDA_E_SIZE;
    if (C > MAXC) return GDA_E_UNSUPPORTED;
    if (nrev != V * M * (K + 2)) return GDA_E_SIZE;                          // a reverse index built for another K / M / V
    const Layout L = layout_of(n, C, M, K, V);
    if (nseg < 1 || nseg > L.max_seg) return GDA_E_SIZE;
    if (!logits || !center || !positive || !negative || !node_seg || !seg_off || !rev_src || !rev_sig || !out || !dlogits
        || !workspace)
        return GDA_E_NULL;
    if (!aligned(logits, 4) || !aligned(dlogits, 4) || !aligned(out, 4) || !aligned(center, 4) || !aligned(positive, 4)
        || !aligned(negative, 4) || !aligned(node_seg, 4) || !aligned(seg_off, 4) || !aligned(rev_src, 4)
        || !aligned(rev_sig, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < L.total * sizeof(float)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int G = group_of(C);
    const int rpb = TB / G;
    float* ws = static_cast<float*>(workspace);
    float *P = ws + L.P, *entp = ws + L.entp, *colp = ws + L.colp, *sigma = ws + L.sigma, *gc = ws + L.gc;
    float *lossp = ws + L.lossp, *mg = ws + L.mg, *gpart = ws + L.gpart;
    const float w0 = lambda_struct / (float)M, w1 = lambda_neigh / (float)M;
    SOGA_DISPATCH(G, (k_soga_rows<GG><<<(unsigned)L.nbr, TB, 0, s>>>(logits, (int)n, (int)C, P, entp, colp)));
    GDA_LAUNCH_CHECK();
    SOGA_DISPATCH(G, (k_soga_pairs<GG><<<dim3((unsigned)L.nbp, (unsigned)V), TB, 0, s>>>(
                         P, center, positive, negative, (int)M, (int)K, (int)n, sigma, gc, lossp)));
    GDA_LAUNCH_CHECK();
    k_soga_finalise<<<1, TB, 0, s>>>(entp, colp, (int)L.nbr, lossp, (int)L.nbp, (int)V, (int)n, (int)M, (int)C, G,
                                     lambda_struct, lambda_neigh, mg, out);
    GDA_LAUNCH_CHECK();
    SOGA_DISPATCH(G, (k_soga_segments<GG><<<(unsigned)gda_cdiv(nseg, rpb), TB, 0, s>>>(
                         P, gc, sigma, seg_off, (int)nseg, rev_src, rev_sig, (int)n, (int)(V * M), (int)(M * K),
                         (int)(V * M * K), w0, w1, gpart)));
    GDA_LAUNCH_CHECK();
    SOGA_DISPATCH(G, (k_soga_nodes<GG><<<(unsigned)L.nbr, TB, 0, s>>>(P, gpart, node_seg, mg, (int)n, (int)C, dlogits)));
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
