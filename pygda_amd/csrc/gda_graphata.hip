// GraphATA (pygda/models/graphata.py, pygda/nn/node_centric_conv.py): the row kernels of the node-centric layer and of
// the adaptation step -- the gate sigmoid(nr) nr, the sparsemax blend of the S source projections with its backward,
// the head (sparsemax blend of the S classifier outputs, information maximisation and the pseudo-label
// cross-entropy, with the gradient), the K-nearest-memory vote and the momentum update of the two memory banks.
// fp32, no atomics.  A row is owned by an aligned group of G lanes (a power of two, at most 64): one class per lane in
// the head / vote / memory kernels, a stride of columns per lane in the mix kernels.  The sparsemax of at most
// GDA_ATA_MAX_SOURCES scores is computed by every lane of the group in registers (a sorting network, the reference's
// operation order).  Reductions over rows are per-workgroup partials folded in block order by one workgroup, so two
// runs give the same bits.  See include/gda_hip.h for the contract of each entry point.
#include "gda_common.h"
#include "gda_reduce.h"

#include <math.h>

namespace {

constexpr int TB = 256;                       // threads per workgroup (4 waves)
constexpr int MAXS = GDA_ATA_MAX_SOURCES;
constexpr int MAXC = GDA_ATA_MAX_CLASSES;
constexpr float ENT_EPS = 1e-8f;              // the reference's entropy offset
constexpr double DIV_EPS = 1e-5;              // and its diversity offset (the other way round from SOGA's)

// ---- sparsemax over a[0 .. S) as node_centric_conv.py:42-71, :102-107 spell it: subtract the maximum, sort descending,
//      support = #{k : k z_(k) > cumsum_k - 1}, tau = (cumsum_support - 1) / support, w = max(z - tau, 0) ----------------
__device__ __forceinline__ void sparsemax_regs(const float (&a)[MAXS], int S, float (&w)[MAXS]) {
    float mx = a[0];
#pragma unroll
    for (int s = 1; s < MAXS; ++s)
        if (s < S) mx = fmaxf(mx, a[s]);
    float z[MAXS], srt[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        z[s] = s < S ? a[s] - mx : -INFINITY;
        srt[s] = z[s];
    }
#pragma unroll
    for (int pass = 0; pass < MAXS; ++pass) {                                // odd-even transposition, descending
#pragma unroll
        for (int j = pass & 1; j + 1 < MAXS; j += 2) {
            const float hi = fmaxf(srt[j], srt[j + 1]), lo = fminf(srt[j], srt[j + 1]);
            srt[j] = hi;
            srt[j + 1] = lo;
        }
    }
    float cs[MAXS];
    float cum = 0.f;
    int supp = 0;
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
        cum += srt[k];
        cs[k] = cum - 1.f;
        if (k < S && (float)(k + 1) * srt[k] > cs[k]) ++supp;
    }
    float t = cs[0];
#pragma unroll
    for (int k = 1; k < MAXS; ++k)
        if (k == supp - 1) t = cs[k];
    const float tau = t / (float)supp;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) w[s] = s < S ? fmaxf(z[s] - tau, 0.f) : 0.f;
}

// its backward (:128-136): the mean of dw over the entries with w != 0 is taken off those entries, the others get 0
__device__ __forceinline__ void sparsemax_bwd_regs(const float (&w)[MAXS], const float (&dw)[MAXS], int S,
                                                   float (&da)[MAXS]) {
    float sum = 0.f;
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S && w[s] != 0.f) {
            sum += dw[s];
            ++cnt;
        }
    const float vhat = sum / (float)cnt;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) da[s] = (s < S && w[s] != 0.f) ? dw[s] - vhat : 0.f;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// ---- gate --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) k_ata_gate(const float* __restrict__ nr, float* __restrict__ g, int64_t numel) {
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= numel) return;
    const float x = nr[e];
    g[e] = sigmoidf(x) * x;
}

__global__ void __launch_bounds__(TB)
k_ata_gate_bwd(const float* __restrict__ nr, const float* __restrict__ dg, const float* __restrict__ dnr_in,
               float* __restrict__ dnr, int64_t numel) {
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= numel) return;
    const float x = nr[e], sg = sigmoidf(x);
    float r = dg[e] * (sg + x * sg * (1.f - sg));
    if (dnr_in != nullptr) r += dnr_in[e];
    dnr[e] = r;
}

// ---- plain sparsemax rows: a thread per row ---------------------------------------------------------------------------
__global__ void __launch_bounds__(TB) k_ata_sparsemax(const float* __restrict__ a, int n, int S, float* __restrict__ w) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    float av[MAXS], wv[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) av[s] = s < S ? a[(int64_t)i * S + s] : 0.f;
    sparsemax_regs(av, S, wv);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S) w[(int64_t)i * S + s] = wv[s];
}

__global__ void __launch_bounds__(TB)
k_ata_sparsemax_bwd(const float* __restrict__ w, const float* __restrict__ dw, int n, int S, float* __restrict__ da) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    float wv[MAXS], dv[MAXS], av[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        wv[s] = s < S ? w[(int64_t)i * S + s] : 0.f;
        dv[s] = s < S ? dw[(int64_t)i * S + s] : 0.f;
    }
    sparsemax_bwd_regs(wv, dv, S, av);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S) da[(int64_t)i * S + s] = av[s];
}

// ---- mix: y = sum_s w_s P_s + lamb Q, w = sparsemax(a); G lanes per row stride over the h columns ---------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_ata_mix(const float* __restrict__ P, const float* __restrict__ Q, const float* __restrict__ a, int n, int h, int S,
          float lamb, float* __restrict__ y, float* __restrict__ w) {
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    if (i >= n) return;
    float av[MAXS], wv[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) av[s] = s < S ? a[(int64_t)i * S + s] : 0.f;
    sparsemax_regs(av, S, wv);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S && lane == s % G) w[(int64_t)i * S + s] = wv[s];
    const float* Pi = P + (int64_t)i * S * h;
    for (int c = lane; c < h; c += G) {
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < S) acc += wv[s] * Pi[(int64_t)s * h + c];
        y[(int64_t)i * h + c] = acc + Q[(int64_t)i * h + c] * lamb;
    }
}

template <int G>
__global__ void __launch_bounds__(TB)
k_ata_mix_bwd(const float* __restrict__ gy, const float* __restrict__ P, const float* __restrict__ w, int n, int h,
              int S, float lamb, float* __restrict__ dP, float* __restrict__ dQ, float* __restrict__ da) {
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n;
    const int ii = row ? i : n - 1;                       // rows past the end redo the last one (the shuffles need all lanes)
    const float* Pi = P + (int64_t)ii * S * h;
    const float* gi = gy + (int64_t)ii * h;
    float wv[MAXS], dw[MAXS], dav[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        wv[s] = s < S ? w[(int64_t)ii * S + s] : 0.f;
        dw[s] = 0.f;
    }
    for (int c = lane; c < h; c += G) {
        const float g = gi[c];
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < S) {
                dw[s] += g * Pi[(int64_t)s * h + c];
                if (row) dP[((int64_t)i * S + s) * h + c] = wv[s] * g;
            }
        if (row) dQ[(int64_t)i * h + c] = lamb * g;
    }
#pragma unroll
    for (int s = 0; s < MAXS; ++s) dw[s] = group_sum<G>(dw[s]);
    sparsemax_bwd_regs(wv, dw, S, dav);
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (row && s < S && lane == s % G) da[(int64_t)i * S + s] = dav[s];
}

// ---- head, rows: scores, sparsemax, logits, softmax; the block's entropy / cross-entropy sums and column sums of p ---
// Z element (s, i, c) sits at s zs + i zr + c (zs = N C, zr = C for [S, N, C]; zs = C, zr = S C for column blocks).
template <int G>
__global__ void __launch_bounds__(TB)
k_ata_head_rows(const float* __restrict__ Z, int64_t zs, int64_t zr, const float* __restrict__ att,
                const int32_t* __restrict__ pred, int n, int C, int S, float* __restrict__ logits,
                float* __restrict__ W, float* __restrict__ Pp, float* __restrict__ entp, float* __restrict__ cep,
                float* __restrict__ colp) {
    __shared__ float tile[TB];
    __shared__ float red[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n, live = row && lane < C;
    const float at = lane < C ? att[lane] : 0.f;
    float zv[MAXS], av[MAXS], wv[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        zv[s] = (live && s < S) ? Z[(int64_t)s * zs + (int64_t)i * zr + lane] : 0.f;
        av[s] = group_sum<G>(zv[s] * at);
    }
    sparsemax_regs(av, S, wv);
    float lg = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S) lg += wv[s] * zv[s];
    if (live) logits[(int64_t)i * C + lane] = lg;
    if (pred == nullptr) return;                                             // forward only (uniform: no barrier skipped)
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (row && s < S && lane == s % G) W[(int64_t)i * MAXS + s] = wv[s];
    const float x = live ? lg : (row ? -INFINITY : 0.f);
    const float mx = group_max<G>(x);
    const float e = (live || !row) ? expf(x - mx) : 0.f;
    const float sum = group_sum<G>(e);
    const float p = e / sum;
    if (row) Pp[(int64_t)i * G + lane] = p;                                  // pad classes: 0
    const float ent = group_sum<G>(live ? -p * logf(p + ENT_EPS) : 0.f);
    const int label = row ? pred[i] : -1;
    const float ce = group_sum<G>((live && lane == label) ? -(x - mx - logf(sum)) : 0.f);
    tile[threadIdx.x] = row ? p : 0.f;
    const bool head = row && lane == 0;
    const float esum = block_sum_f(head ? ent : 0.f, red);                   // (its barriers publish tile too)
    const float csum = block_sum_f(head ? ce : 0.f, red);
    if (threadIdx.x < G) {
        float acc = 0.f;
        for (int r = 0; r < TB / G; ++r) acc += tile[r * G + threadIdx.x];   // the block's rows, in order
        colp[(int64_t)blockIdx.x * G + threadIdx.x] = acc;
    }
    if (threadIdx.x == 0) {
        entp[blockIdx.x] = esum;
        cep[blockIdx.x] = csum;
    }
}

// sum over the blocks b of part[b G + lane] in double, slices of blocks folded in order through cols[TB]; valid for t < G
__device__ __forceinline__ double fold_cols(const float* __restrict__ part, int nb, int G, double* cols) {
    const int t = threadIdx.x, lane = t % G, slices = TB / G;
    double a = 0.0;
    for (int b = t / G; b < nb; b += slices) a += (double)part[(int64_t)b * G + lane];
    cols[t] = a;
    __syncthreads();
    double s = 0.0;
    if (t < G)
        for (int q = 0; q < slices; ++q) s += cols[q * G + t];
    __syncthreads();
    return s;
}

// ---- head, finalise (one workgroup): m = colsum / N, the diversity gradient into mg [G], the four figures -------------
__global__ void __launch_bounds__(TB)
k_ata_head_finalise(const float* __restrict__ entp, const float* __restrict__ cep, const float* __restrict__ colp, int nb,
                    int n, int C, int G, float* __restrict__ mg, float* __restrict__ out) {
    __shared__ double red[TB];
    __shared__ double cols[TB];
    const int t = threadIdx.x;
    const double s = fold_cols(colp, nb, G, cols);
    double dterm = 0.0;
    if (t < G) {
        const double m = s / (double)n;
        mg[t] = t < C ? (float)((log(m + DIV_EPS) + m / (m + DIV_EPS)) / (double)n) : 0.f;
        dterm = t < C ? m * log(m + DIV_EPS) : 0.0;
    }
    const double div = block_sum_d(dterm, red);
    const double ent = fold_d<TB>(entp, nb, red) / (double)n;
    const double ce = fold_d<TB>(cep, nb, red) / (double)n;
    if (t == 0) {
        out[0] = (float)(ent + div + ce);
        out[1] = (float)ent;
        out[2] = (float)div;
        out[3] = (float)ce;
    }
}

// ---- head, gradient rows: dlogits, dZ_s = w_s dlogits + da_s att, the block's partials of datt -------------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_ata_head_grad(const float* __restrict__ Z, int64_t zs, int64_t zr, const float* __restrict__ att,
                const int32_t* __restrict__ pred, const float* __restrict__ W, const float* __restrict__ Pp,
                const float* __restrict__ mg, int n, int C, int S, float* __restrict__ dZ, float* __restrict__ dattp) {
    __shared__ float tile[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n, live = row && lane < C;
    const int ii = row ? i : n - 1;
    const float at = lane < C ? att[lane] : 0.f;
    const float p = Pp[(int64_t)ii * G + lane];
    const int label = pred[ii];
    float g = lane < C ? (-logf(p + ENT_EPS) - p / (p + ENT_EPS)) / (float)n + mg[lane] : 0.f;
    const float dot = group_sum<G>(g * p);
    // (a label outside [0, C) adds no cross-entropy term to the forward's sum, so none to the gradient either)
    const float dce = (unsigned)label < (unsigned)C ? (p - (lane == label ? 1.f : 0.f)) / (float)n : 0.f;
    const float dl = lane < C ? p * (g - dot) + dce : 0.f;
    float zv[MAXS], wv[MAXS], dw[MAXS], dav[MAXS];
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
        zv[s] = (live && s < S) ? Z[(int64_t)s * zs + (int64_t)i * zr + lane] : 0.f;
        wv[s] = s < S ? W[(int64_t)ii * MAXS + s] : 0.f;
        dw[s] = group_sum<G>(dl * zv[s]);
    }
    sparsemax_bwd_regs(wv, dw, S, dav);
    float dat = 0.f;
#pragma unroll
    for (int s = 0; s < MAXS; ++s)
        if (s < S) {
            if (live) dZ[(int64_t)s * zs + (int64_t)i * zr + lane] = wv[s] * dl + dav[s] * at;
            dat += dav[s] * zv[s];
        }
    tile[threadIdx.x] = live ? dat : 0.f;
    __syncthreads();
    if (threadIdx.x < G) {
        float acc = 0.f;
        for (int r = 0; r < TB / G; ++r) acc += tile[r * G + threadIdx.x];
        dattp[(int64_t)blockIdx.x * G + threadIdx.x] = acc;
    }
}

// the ordered fold of [nb, G] partials into out[0 .. C)
__global__ void __launch_bounds__(TB)
k_ata_fold_cols(const float* __restrict__ part, int nb, int C, int G, float* __restrict__ out) {
    __shared__ double cols[TB];
    const double s = fold_cols(part, nb, G, cols);
    if (threadIdx.x < C) out[threadIdx.x] = (float)s;
}

// ---- vote: the mean of the memory's class rows over ranks 2 .. K1, in rank order; the first arg-max --------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_ata_vote(const int32_t* __restrict__ nn_idx, const float* __restrict__ mem_cls, int n, int nm, int C, int K1,
           int32_t* __restrict__ pred) {
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n;
    const int ii = row ? i : n - 1;
    float acc = 0.f;
    for (int k = 1; k < K1; ++k) {
        const int j = nn_idx[(int64_t)ii * K1 + k];
        if ((unsigned)j < (unsigned)nm && lane < C) acc += mem_cls[(int64_t)j * C + lane];
    }
    const float v = lane < C ? acc / (float)(K1 - 1) : -INFINITY;
    const float mx = group_max<G>(v);
    int arg = (lane < C && v == mx) ? lane : G;
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) arg = min(arg, __shfl_xor(arg, off, G));
    if (row && lane == 0) pred[i] = arg < C ? arg : 0;                       // (a row of NaN: class 0)
}

// ---- memory: q = p^2 / colsum(p^2), both banks moved by the momentum ---------------------------------------------------
template <int G>
__global__ void __launch_bounds__(TB)
k_ata_mem_rows(const float* __restrict__ logits, int n, int C, float* __restrict__ SQ, float* __restrict__ colp) {
    __shared__ float tile[TB];
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    const bool row = i < n, live = row && lane < C;
    const float x = live ? logits[(int64_t)i * C + lane] : (row ? -INFINITY : 0.f);
    const float mx = group_max<G>(x);
    const float e = (live || !row) ? expf(x - mx) : 0.f;
    const float p = e / group_sum<G>(e);
    const float sq = row ? p * p : 0.f;
    if (row) SQ[(int64_t)i * G + lane] = sq;
    tile[threadIdx.x] = sq;
    __syncthreads();
    if (threadIdx.x < G) {
        float acc = 0.f;
        for (int r = 0; r < TB / G; ++r) acc += tile[r * G + threadIdx.x];
        colp[(int64_t)blockIdx.x * G + threadIdx.x] = acc;
    }
}

__global__ void __launch_bounds__(TB)
k_ata_mem_fold(const float* __restrict__ colp, int nb, int G, float* __restrict__ cs) {
    __shared__ double cols[TB];
    const double s = fold_cols(colp, nb, G, cols);
    if (threadIdx.x < G) cs[threadIdx.x] = (float)s;
}

template <int G>
__global__ void __launch_bounds__(TB)
k_ata_mem_cls(const float* __restrict__ SQ, const float* __restrict__ cs, int n, int C, float keep, float mu,
              float* __restrict__ mem_cls) {
    const int lane = threadIdx.x % G;
    const int i = blockIdx.x * (TB / G) + threadIdx.x / G;
    if (i >= n || lane >= C) return;
    const float q = SQ[(int64_t)i * G + lane] / cs[lane];
    float* m = mem_cls + (int64_t)i * C + lane;
    *m = keep * *m + mu * q;
}

__global__ void __launch_bounds__(TB)
k_ata_mem_fea(const float* __restrict__ feat, int64_t numel, float keep, float mu, float* __restrict__ mem_fea) {
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= numel) return;
    mem_fea[e] = keep * mem_fea[e] + mu * feat[e];
}

int group_of(int64_t C) {
    int g = 1;
    while (g < C) g <<= 1;
    return g;
}

int mix_group(int64_t h) { return h >= 64 ? 64 : (h > 8 ? group_of(h) : 8); }

size_t al4(size_t floats) { return gda_align_up(floats, 4); }               // sections start on 16 bytes

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

constexpr int64_t ROW_LIMIT = ((int64_t)1 << 31) / 64;                       // rows: n G fits an int

struct HeadLayout {
    size_t W, P, entp, cep, colp, mg, dattp, total;
    int64_t nb;
};

HeadLayout head_layout(int64_t n, int64_t C) {
    const int G = group_of(C);
    HeadLayout L;
    L.nb = gda_cdiv(n, TB / G);
    size_t o = 0;
    L.W = o;      o += al4((size_t)n * MAXS);
    L.P = o;      o += al4((size_t)n * G);
    L.entp = o;   o += al4((size_t)L.nb);
    L.cep = o;    o += al4((size_t)L.nb);
    L.colp = o;   o += al4((size_t)L.nb * G);
    L.mg = o;     o += al4((size_t)G);
    L.dattp = o;  o += al4((size_t)L.nb * G);
    L.total = o;
    return L;
}

#define ATA_DISPATCH(G, CALL)                            \
    switch (G) {                                         \
        case 1: { constexpr int GG = 1; CALL; } break;   \
        case 2: { constexpr int GG = 2; CALL; } break;   \
        case 4: { constexpr int GG = 4; CALL; } break;   \
        case 8: { constexpr int GG = 8; CALL; } break;   \
        case 16: { constexpr int GG = 16; CALL; } break; \
        case 32: { constexpr int GG = 32; CALL; } break; \
        default: { constexpr int GG = 64; CALL; } break; \
    }

#define ATA_MIX_DISPATCH(G, CALL)                        \
    switch (G) {                                         \
        case 8: { constexpr int GG = 8; CALL; } break;   \
        case 16: { constexpr int GG = 16; CALL; } break; \
        case 32: { constexpr int GG = 32; CALL; } break; \
        default: { constexpr int GG = 64; CALL; } break; \
    }

}  // namespace

extern "C" int gda_ata_gate_f32(const float* nr, float* g, int64_t numel, gda_stream_t stream) {
    if (numel < 1 || numel >= ((int64_t)1 << 31) * TB) return GDA_E_SIZE;
    if (!nr || !g) return GDA_E_NULL;
    if (!aligned(nr, 4) || !aligned(g, 4)) return GDA_E_UNSUPPORTED;
    k_ata_gate<<<(unsigned)gda_cdiv(numel, TB), TB, 0, (hipStream_t)stream>>>(nr, g, numel);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_gate_bwd_f32(const float* nr, const float* dg, const float* dnr_in, float* dnr, int64_t numel,
                                    gda_stream_t stream) {
    if (numel < 1 || numel >= ((int64_t)1 << 31) * TB) return GDA_E_SIZE;
    if (!nr || !dg || !dnr) return GDA_E_NULL;
    if (!aligned(nr, 4) || !aligned(dg, 4) || !aligned(dnr_in, 4) || !aligned(dnr, 4)) return GDA_E_UNSUPPORTED;
    k_ata_gate_bwd<<<(unsigned)gda_cdiv(numel, TB), TB, 0, (hipStream_t)stream>>>(nr, dg, dnr_in, dnr, numel);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_sparsemax_f32(const float* a, int64_t n, int64_t S, float* w, gda_stream_t stream) {
    if (n < 1 || S < 1 || n >= ROW_LIMIT) return GDA_E_SIZE;
    if (S > MAXS) return GDA_E_UNSUPPORTED;
    if (!a || !w) return GDA_E_NULL;
    if (!aligned(a, 4) || !aligned(w, 4)) return GDA_E_UNSUPPORTED;
    k_ata_sparsemax<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(a, (int)n, (int)S, w);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_sparsemax_bwd_f32(const float* w, const float* dw, int64_t n, int64_t S, float* da,
                                         gda_stream_t stream) {
    if (n < 1 || S < 1 || n >= ROW_LIMIT) return GDA_E_SIZE;
    if (S > MAXS) return GDA_E_UNSUPPORTED;
    if (!w || !dw || !da) return GDA_E_NULL;
    if (!aligned(w, 4) || !aligned(dw, 4) || !aligned(da, 4)) return GDA_E_UNSUPPORTED;
    k_ata_sparsemax_bwd<<<(unsigned)gda_cdiv(n, TB), TB, 0, (hipStream_t)stream>>>(w, dw, (int)n, (int)S, da);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_mix_f32(const float* P, const float* Q, const float* a, int64_t n, int64_t h, int64_t S,
                               float lamb, float* y, float* w, gda_stream_t stream) {
    if (n < 1 || h < 1 || S < 1 || n >= ROW_LIMIT) return GDA_E_SIZE;
    if (S > MAXS || h > GDA_WGCN_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!P || !Q || !a || !y || !w) return GDA_E_NULL;
    if (!aligned(P, 4) || !aligned(Q, 4) || !aligned(a, 4) || !aligned(y, 4) || !aligned(w, 4)) return GDA_E_UNSUPPORTED;
    const int G = mix_group(h);
    ATA_MIX_DISPATCH(G, (k_ata_mix<GG><<<(unsigned)gda_cdiv(n, TB / G), TB, 0, (hipStream_t)stream>>>(
                            P, Q, a, (int)n, (int)h, (int)S, lamb, y, w)));
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_mix_bwd_f32(const float* gy, const float* P, const float* w, int64_t n, int64_t h, int64_t S,
                                   float lamb, float* dP, float* dQ, float* da, gda_stream_t stream) {
    if (n < 1 || h < 1 || S < 1 || n >= ROW_LIMIT) return GDA_E_SIZE;
    if (S > MAXS || h > GDA_WGCN_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!gy || !P || !w || !dP || !dQ || !da) return GDA_E_NULL;
    if (!aligned(gy, 4) || !aligned(P, 4) || !aligned(w, 4) || !aligned(dP, 4) || !aligned(dQ, 4) || !aligned(da, 4))
        return GDA_E_UNSUPPORTED;
    const int G = mix_group(h);
    ATA_MIX_DISPATCH(G, (k_ata_mix_bwd<GG><<<(unsigned)gda_cdiv(n, TB / G), TB, 0, (hipStream_t)stream>>>(
                            gy, P, w, (int)n, (int)h, (int)S, lamb, dP, dQ, da)));
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_ata_head_workspace_bytes(int64_t n, int64_t C) {
    if (n < 1 || C < 1 || C > MAXC || n >= ROW_LIMIT) return 256;
    return gda_align_up(head_layout(n, C).total * sizeof(float), 256);
}

extern "C" int gda_ata_head_f32(const float* Z, int64_t src_stride, int64_t row_stride, const float* att,
                                const int32_t* pred, int64_t n, int64_t C, int64_t S, float* logits, float* out,
                                float* dZ, float* datt, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || C < 1 || S < 1 || n >= ROW_LIMIT || src_stride < 1 || row_stride < C) return GDA_E_SIZE;
    if (C > MAXC || S > MAXS) return GDA_E_UNSUPPORTED;
    // the two layouts an [S, N, C] array and S column blocks of an [N, S C] array have: nothing else is in bounds by rule
    if (!((src_stride == n * C && row_stride == C) || (src_stride == C && row_stride == S * C))) return GDA_E_SIZE;
    if (!Z || !att || !logits) return GDA_E_NULL;
    if (pred && (!out || !dZ || !datt || !workspace)) return GDA_E_NULL;
    if (!aligned(Z, 4) || !aligned(att, 4) || !aligned(pred, 4) || !aligned(logits, 4) || !aligned(out, 4)
        || !aligned(dZ, 4) || !aligned(datt, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int G = group_of(C);
    const HeadLayout L = head_layout(n, C);
    if (!pred) {
        ATA_DISPATCH(G, (k_ata_head_rows<GG><<<(unsigned)L.nb, TB, 0, s>>>(Z, src_stride, row_stride, att, nullptr, (int)n,
                                                                           (int)C, (int)S, logits, nullptr, nullptr,
                                                                           nullptr, nullptr, nullptr)));
        GDA_LAUNCH_CHECK();
        return GDA_OK;
    }
    if (workspace_bytes < L.total * sizeof(float)) return GDA_E_WORKSPACE;
    float* ws = static_cast<float*>(workspace);
    float *W = ws + L.W, *Pp = ws + L.P, *entp = ws + L.entp, *cep = ws + L.cep, *colp = ws + L.colp, *mg = ws + L.mg;
    float* dattp = ws + L.dattp;
    ATA_DISPATCH(G, (k_ata_head_rows<GG><<<(unsigned)L.nb, TB, 0, s>>>(Z, src_stride, row_stride, att, pred, (int)n, (int)C,
                                                                       (int)S, logits, W, Pp, entp, cep, colp)));
    GDA_LAUNCH_CHECK();
    k_ata_head_finalise<<<1, TB, 0, s>>>(entp, cep, colp, (int)L.nb, (int)n, (int)C, G, mg, out);
    GDA_LAUNCH_CHECK();
    ATA_DISPATCH(G, (k_ata_head_grad<GG><<<(unsigned)L.nb, TB, 0, s>>>(Z, src_stride, row_stride, att, pred, W, Pp, mg,
                                                                       (int)n, (int)C, (int)S, dZ, dattp)));
    GDA_LAUNCH_CHECK();
    k_ata_fold_cols<<<1, TB, 0, s>>>(dattp, (int)L.nb, (int)C, G, datt);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_ata_vote_f32(const int32_t* nn_idx, const float* mem_cls, int64_t n, int64_t nm, int64_t C, int64_t K1,
                                int32_t* pred, gda_stream_t stream) {
    if (n < 1 || nm < 1 || C < 1 || K1 < 2 || n >= ROW_LIMIT || nm >= ROW_LIMIT) return GDA_E_SIZE;
    if (C > MAXC || K1 > GDA_CTA_MAX_K1) return GDA_E_UNSUPPORTED;
    if (!nn_idx || !mem_cls || !pred) return GDA_E_NULL;
    if (!aligned(nn_idx, 4) || !aligned(mem_cls, 4) || !aligned(pred, 4)) return GDA_E_UNSUPPORTED;
    const int G = group_of(C);
    ATA_DISPATCH(G, (k_ata_vote<GG><<<(unsigned)gda_cdiv(n, TB / G), TB, 0, (hipStream_t)stream>>>(
                        nn_idx, mem_cls, (int)n, (int)nm, (int)C, (int)K1, pred)));
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_ata_memory_workspace_bytes(int64_t n, int64_t C) {
    if (n < 1 || C < 1 || C > MAXC || n >= ROW_LIMIT) return 256;
    const int G = group_of(C);
    return gda_align_up((al4((size_t)n * G) + al4((size_t)gda_cdiv(n, TB / G) * G) + al4((size_t)G)) * sizeof(float), 256);
}

extern "C" int gda_ata_memory_f32(const float* logits, const float* feat, int64_t n, int64_t C, int64_t d, float keep,
                                  float momentum, float* mem_cls, float* mem_fea, void* workspace,
                                  size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || C < 1 || d < 1 || n >= ROW_LIMIT) return GDA_E_SIZE;
    if (C > MAXC || d > GDA_WGCN_MAX_WIDTH) return GDA_E_UNSUPPORTED;
    if (!logits || !feat || !mem_cls || !mem_fea || !workspace) return GDA_E_NULL;
    if (!aligned(logits, 4) || !aligned(feat, 4) || !aligned(mem_cls, 4) || !aligned(mem_fea, 4) || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_ata_memory_workspace_bytes(n, C)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int G = group_of(C);
    const int64_t nb = gda_cdiv(n, TB / G);
    float* SQ = static_cast<float*>(workspace);
    float* colp = SQ + al4((size_t)n * G);
    float* cs = colp + al4((size_t)nb * G);
    ATA_DISPATCH(G, (k_ata_mem_rows<GG><<<(unsigned)nb, TB, 0, s>>>(logits, (int)n, (int)C, SQ, colp)));
    GDA_LAUNCH_CHECK();
    k_ata_mem_fold<<<1, TB, 0, s>>>(colp, (int)nb, G, cs);
    GDA_LAUNCH_CHECK();
    ATA_DISPATCH(G, (k_ata_mem_cls<GG><<<(unsigned)nb, TB, 0, s>>>(SQ, cs, (int)n, (int)C, keep, momentum, mem_cls)));
    GDA_LAUNCH_CHECK();
    k_ata_mem_fea<<<(unsigned)gda_cdiv(n * d, TB), TB, 0, s>>>(feat, n * d, keep, momentum, mem_fea);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
