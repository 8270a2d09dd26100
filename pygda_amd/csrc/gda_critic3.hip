// SpecReg's three-layer Wasserstein critic and its spectral hinges, gfx950.
//
// Replaces the critic loop body of pygda/models/specreg.py:194-200 with calculate_gradient_penalty (:380-419), the
// encoder-side gap (:202) and the regulariser (:209-215) for the critic built at :281-287,
//     D(x) = w3 . relu(W2 relu(W1 x + b1) + b2) + b3,      W1, W2 [h, h], w3 [h]   (no dropout, no sigmoid)
//     L = -(mean_s D(e_s) - mean_t D(e_t)) + 10 * mean_i (|| grad_x D(x_i) ||_2 - 1)^2,   x = cat(e_s, e_t)  (M rows)
// The reference differentiates twice through torch autograd.  D is piecewise linear, so per row everything is closed
// form; with the masks r1 = [a1 > 0], r2 = [a2 > 0]:
//     a1 = W1 x + b1, h1 = r1 a1;  a2 = W2 h1 + b2, h2 = r2 a2;  D = w3 . h2 + b3
//     p = r2 w3, q = r1 (W2^T p), g = W1^T q = grad_x D, n = |g|, ghat = g / n (0 where n == 0, as torch's norm backward)
//     c = 10 * 2 (n - 1) / M, sigma = -1 / n_s | +1 / n_t;  t = r1 (W1 ghat), s = r2 (W2 t)
//     gW1 = sum q (sigma x + c ghat)^T, gb1 = sum sigma q, gW2 = sum p (sigma h1 + c t)^T, gb2 = sum sigma p (from exact on-counts),
//     gw3 = sum (sigma h2 + c s), gb3 = sum sigma
// Launches of one update:
//   k_critic3_rows<HT, 0>   32 rows per wavefront, four wavefronts per workgroup; the six [h, h] products of a row as
//                           32-row tile products on v_mfma_f32_32x32x2_f32 with the rows as the MFMA's column index (a
//                           lane pair (l, l + 32) owns one row and holds its units in accumulator registers).  h is zero
//                           filled to HP = 32 HT inside the kernel.  ONE weight matrix sits in LDS at a time ([HP][HP + 1],
//                           conflict free in both orientations), staged from L2 four times per trip: W1 | W2 | W1 | W2 for
//                           the products (1) | (2, 3) | (4, 5) | (6); beside it the four wavefronts' tiles [32][HP + 1].
//                           Q, Y1 = sigma x + c ghat, P, Y2 = sigma h1 + c t go to the workspace through the tile
//                           (coalesced); the per-unit sums (gb1, gb2, gw3) are column sums of the tile, the per-row sums
//                           (gb3, D per domain, penalty) lane sums: all as double block partials part[column][block].
//   gda_gemm_f32 TN x 2     gW1 = Q^T Y1, gW2 = P^T Y2 (deterministic row-slab split)
//   k_critic3_fold          the block partials folded in a fixed order: gb1, gb2, gw3, gb3, loss; with Adam on, the
//                           update of all six tensors (gda_adam_rule.h) by the thread that holds the gradient
// The gap (k_critic3_rows<HT, 1>, k_critic3_gap_fold) is the same row program cut after its fourth product.
// k_spectral_hinge: value and gradient of the two hinges over X = eivec @ encoded in one launch; the workgroups' double
// sums are added in block order by the workgroup that finishes last.
#include "gda_common.h"
#include "gda_adam_rule.h"
#include "gda_reduce.h"

namespace {

constexpr int TB = 256;
constexpr int WAVES = TB / 64;
constexpr int RT = 32;             // rows per wavefront tile
constexpr int HMAX3 = 128;         // widest critic
constexpr int ROW_BLOCKS3 = 256;   // grid cap of the row kernel: ROW_BLOCKS3 * WAVES * RT rows per trip
constexpr int NSC = 4 * HMAX3;        // first scalar column of the block partials
constexpr int NCOL = NSC + 5;         // gb1 | rows with unit on (source) | (target) | gw3 | sum sigma (source, target), sum D_s, sum D_t, penalty
constexpr float GP_WEIGHT3 = 10.f;    // specreg.py:199

using f32x16 = __attribute__((ext_vector_type(16))) float;

struct Critic3 {
    const float* W1; const float* b1; const float* W2; const float* b2; const float* w3; const float* b3;
    int h;
};

struct Rows3 { const float* es; int64_t n_s; const float* et; int64_t n_t; };

// torch.optim.Adam state of W1, b1, W2, b2, w3, b3 (in this order); on = 0: gradients only
struct Adam3 {
    float* p[6]; float* m[6]; float* v[6]; float* step[6];
    float lr, beta1, beta2, eps, weight_decay;
    int on;
};

// A wavefront's tile is written and read by that wavefront alone, so the hand-over between its lanes needs no workgroup
// barrier (the four wavefronts run different phases of their tiles; __syncthreads is kept for the shared weight): the
// wavefront's LDS operations complete in order, and this wait with its memory clobber keeps the compiler from moving
// them across the hand-over.
__device__ __forceinline__ void lds_settle() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// unit (or column) held by accumulator register q of tile t in the lane's half
__device__ __forceinline__ int acc_unit(int t, int q, int half) { return 32 * t + (q & 3) + 8 * (q >> 2) + 4 * half; }

// W [h, h] -> Ws [HP][HP + 1], zero filled past h, by the whole workgroup
template <int HT>
__device__ __forceinline__ void stage_weight(const float* __restrict__ W, int h, float* Ws) {
    constexpr int HP = 32 * HT, ld = HP + 1;
#pragma unroll 8
    for (int e = threadIdx.x; e < HP * HP; e += TB) {
        const int r = e / HP, c = e % HP;
        Ws[r * ld + c] = (r < h && c < h) ? W[(size_t)r * h + c] : 0.f;
    }
}

// row g of cat(e_s, e_t)
__device__ __forceinline__ const float* cat_row(const Rows3& R, int h, int64_t g) {
    return g < R.n_s ? R.es + g * h : R.et + (g - R.n_s) * h;
}

// 32 rows from `base` of cat(e_s, e_t) -> the wavefront's tile, zeros past M and past h: coalesced 4-byte loads (any alignment)
template <int HT>
__device__ __forceinline__ void tile_load_x(const Rows3& R, int h, int64_t base, int64_t M, float* Ts, int lane) {
    constexpr int HP = 32 * HT, ld = HP + 1;
#pragma unroll 8
    for (int k = 0; k < RT * HP / 64; ++k) {
        const int idx = lane + 64 * k, row = idx / HP, col = idx % HP;
        const int64_t g = base + row;
        Ts[row * ld + col] = (g < M && col < h) ? cat_row(R, h, g)[col] : 0.f;
    }
}

// the same from / to a workspace matrix [M, h]; both use ONE lane <-> address mapping, so a lane that loads what an
// earlier tile_store of the same tile wrote reads its own stores
template <int HT>
__device__ __forceinline__ void tile_load_ws(const float* __restrict__ src, int h, int64_t base, int64_t M, float* Ts, int lane) {
    constexpr int HP = 32 * HT, ld = HP + 1;
#pragma unroll 8
    for (int k = 0; k < RT * HP / 64; ++k) {
        const int idx = lane + 64 * k, row = idx / HP, col = idx % HP;
        const int64_t g = base + row;
        Ts[row * ld + col] = (g < M && col < h) ? src[g * h + col] : 0.f;
    }
}

template <int HT>
__device__ __forceinline__ void tile_store_ws(float* __restrict__ dst, int h, int64_t base, int64_t M, const float* Ts, int lane) {
    constexpr int HP = 32 * HT, ld = HP + 1;
#pragma unroll 8
    for (int k = 0; k < RT * HP / 64; ++k) {
        const int idx = lane + 64 * k, row = idx / HP, col = idx % HP;
        const int64_t g = base + row;
        if (g < M && col < h) dst[g * h + col] = Ts[row * ld + col];
    }
}

// acc[it][.] = (W V^T)[unit 32 it + ., row rl]: W as the MFMA's row operand, the tile's rows as its columns
template <int HT>
__device__ __forceinline__ void prod_n(const float* Ws, const float* Ts, int h, int rl, int half, f32x16 (&acc)[HT]) {
    constexpr int ld = 32 * HT + 1;
#pragma unroll
    for (int it = 0; it < HT; ++it)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[it][q] = 0.f;
    const float* w = Ws + rl * ld + half;
    const float* v = Ts + rl * ld + half;
    for (int kk = 0; kk < h; kk += 4) {                                // h % 4 == 0: two k-steps a pass, their operands fetched together
        const float b0 = v[kk], b1 = v[kk + 2];
        float a0[HT], a1[HT];
#pragma unroll
        for (int it = 0; it < HT; ++it) { a0[it] = w[32 * it * ld + kk]; a1[it] = w[32 * it * ld + kk + 2]; }
#pragma unroll
        for (int it = 0; it < HT; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[it], b0, acc[it], 0, 0, 0);
#pragma unroll
        for (int it = 0; it < HT; ++it) acc[it] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[it], b1, acc[it], 0, 0, 0);
    }
}

// acc[jt][.] = (W^T V^T)[column 32 jt + ., row rl]
template <int HT>
__device__ __forceinline__ void prod_t(const float* Ws, const float* Ts, int h, int rl, int half, f32x16 (&acc)[HT]) {
    constexpr int ld = 32 * HT + 1;
#pragma unroll
    for (int jt = 0; jt < HT; ++jt)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[jt][q] = 0.f;
    const float* w = Ws + half * ld + rl;
    const float* v = Ts + rl * ld + half;
    for (int kk = 0; kk < h; kk += 4) {
        const float b0 = v[kk], b1 = v[kk + 2];
        float a0[HT], a1[HT];
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) { a0[jt] = w[kk * ld + 32 * jt]; a1[jt] = w[(kk + 2) * ld + 32 * jt]; }
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[jt], b0, acc[jt], 0, 0, 0);
#pragma unroll
        for (int jt = 0; jt < HT; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[jt], b1, acc[jt], 0, 0, 0);
    }
}

// the lane pair's row of accumulators -> its row of the tile
template <int HT>
__device__ __forceinline__ void acc_to_tile(const f32x16 (&acc)[HT], float* Ts, int rl, int half) {
    constexpr int ld = 32 * HT + 1;
#pragma unroll
    for (int t = 0; t < HT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) Ts[rl * ld + acc_unit(t, q, half)] = acc[t][q];
}

// sum over the tile's 32 rows of column c (plain, or weighted by the row's sigma): fixed order, four chains
__device__ __forceinline__ float tile_colsum(const float* Ts, int ld, int c) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int r = 0; r < RT; r += 4) {
        s0 += Ts[r * ld + c]; s1 += Ts[(r + 1) * ld + c]; s2 += Ts[(r + 2) * ld + c]; s3 += Ts[(r + 3) * ld + c];
    }
    return (s0 + s1) + (s2 + s3);
}

__device__ __forceinline__ float row_sigma(const Rows3& R, int64_t g) {
    return g < R.n_s ? -1.f / (float)R.n_s : (g < R.n_s + R.n_t ? 1.f / (float)R.n_t : 0.f);
}

__device__ __forceinline__ float tile_colsum_sigma(const float* Ts, int ld, int c, const Rows3& R, int64_t base) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int r = 0; r < RT; r += 4) {
        s0 += row_sigma(R, base + r) * Ts[r * ld + c]; s1 += row_sigma(R, base + r + 1) * Ts[(r + 1) * ld + c];
        s2 += row_sigma(R, base + r + 2) * Ts[(r + 2) * ld + c]; s3 += row_sigma(R, base + r + 3) * Ts[(r + 3) * ld + c];
    }
    return (s0 + s1) + (s2 + s3);
}

// rows of the tile's column c that belong to the source (which = 0) or the target (which = 1), weighted by the tile's
// entry (an indicator tile: a count, exact in fp32)
__device__ __forceinline__ float tile_colsum_domain(const float* Ts, int ld, int c, const Rows3& R, int64_t base, int which) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int64_t g = base + r;
        const bool in = which == 0 ? g < R.n_s : (g >= R.n_s && g < R.n_s + R.n_t);
        s += in ? Ts[r * ld + c] : 0.f;
    }
    return s;
}

// MODE 0: the critic update's rows (Q, Y1, P, Y2 and the block partials).  MODE 1: the gap -- products (1) - (4), the input
// gradient g with +1/n_s | -1/n_t applied into ges | get (either may be null), sum D per domain.
template <int HT, int MODE>
__global__ void __launch_bounds__(TB)
k_critic3_rows(Critic3 C, Rows3 R, float* __restrict__ Qw, float* __restrict__ Y1w, float* __restrict__ Pw, float* __restrict__ Y2w,
               float* __restrict__ ges, float* __restrict__ get, double* __restrict__ part, Adam3 ad) {
    constexpr int HP = 32 * HT, ld = HP + 1, NC = (HP + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ float b1s[HMAX3], b2s[HMAX3], w3s[HMAX3];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64, rl = lane & 31, half = lane >> 5;
    const int h = C.h;
    float* Ws = smem;                                                   // the weight of the phase [HP][ld]
    float* Ts = smem + HP * ld + wave * RT * ld;                        // this wavefront's tile [32][ld]
    if (MODE == 0 && ad.on && blockIdx.x == 0) {                        // the step counters: read by the fold launch
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (threadIdx.x == k) *ad.step[k] += 1.0f;
    }
    if (threadIdx.x < HMAX3) {
        const int i = threadIdx.x;
        b1s[i] = i < h ? C.b1[i] : 0.f; b2s[i] = i < h ? C.b2[i] : 0.f; w3s[i] = i < h ? C.w3[i] : 0.f;
    }
    const float b3 = C.b3[0];
    const int64_t M = R.n_s + R.n_t;
    const int64_t nquad = (M + WAVES * RT - 1) / (WAVES * RT);
    double cs_b1[NC], cs_b2s[NC], cs_b2t[NC], cs_w3[NC];                             // lane's columns lane + 64 cc
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) cs_b1[cc] = cs_b2s[cc] = cs_b2t[cc] = cs_w3[cc] = 0.0;
    double acc_sig_s = 0.0, acc_sig_t = 0.0, acc_ds = 0.0, acc_dt = 0.0, acc_pen = 0.0;

    // every wavefront runs every trip (rows past the end are dead: zero contributions): the barriers are uniform
    for (int64_t quad = blockIdx.x; quad < nquad; quad += gridDim.x) {
        const int64_t base = (quad * WAVES + wave) * RT;
        const int64_t r = base + rl;                                    // this lane pair's row
        const bool live = r < M;
        const float sigma = live ? row_sigma(R, r) : 0.f;
        f32x16 acc[HT];
        // ---- (1) a1 = W1 x + b1, h1 = relu
        stage_weight<HT>(C.W1, h, Ws);
        tile_load_x<HT>(R, h, base, M, Ts, lane);
        __syncthreads();
        prod_n<HT>(Ws, Ts, h, rl, half, acc);
        uint64_t r1 = 0, r2 = 0;
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float a = acc[t][q] + b1s[acc_unit(t, q, half)];
                const bool on = live && a > 0.f;
                r1 |= (uint64_t)on << (16 * t + q);
                acc[t][q] = on ? a : 0.f;
            }
        lds_settle();
        acc_to_tile<HT>(acc, Ts, rl, half);                             // H1
        lds_settle();
        if (MODE == 0) tile_store_ws<HT>(Y2w, h, base, M, Ts, lane);    // h1 waits in Y2's rows for t
        __syncthreads();
        // ---- (2) a2 = W2 h1 + b2, h2 = relu, D
        stage_weight<HT>(C.W2, h, Ws);
        __syncthreads();
        prod_n<HT>(Ws, Ts, h, rl, half, acc);
        float dpart = 0.f;
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = acc_unit(t, q, half);
                const float a = acc[t][q] + b2s[i];
                const bool on = live && a > 0.f;
                r2 |= (uint64_t)on << (16 * t + q);
                acc[t][q] = on ? a : 0.f;
                dpart = fmaf(w3s[i], acc[t][q], dpart);
            }
        const float D = dpart + __shfl_xor(dpart, 32, 64) + b3;
        if (live && half == 0) {
            // gb3 = sum sigma, the sum itself: each domain's in double
            if (r < R.n_s) { acc_ds += (double)D; acc_sig_s += -1.0 / (double)R.n_s; }
            else { acc_dt += (double)D; acc_sig_t += 1.0 / (double)R.n_t; }
        }
        lds_settle();
        if (MODE == 0) {
            acc_to_tile<HT>(acc, Ts, rl, half);                         // H2: gw3's gap part sum sigma h2
            lds_settle();
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
                if (lane + 64 * cc < HP) cs_w3[cc] += (double)tile_colsum_sigma(Ts, ld, lane + 64 * cc, R, base);
            lds_settle();
            // gb2 = sum sigma p = w3 (rows on in the target / n_t - rows on in the source / n_s): the counts, exact, so that
            // a unit that is on for every row gets -1 + 1 = 0 and not a rounding residue for Adam to amplify
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = ((r2 >> (16 * t + q)) & 1) ? 1.f : 0.f;
            acc_to_tile<HT>(acc, Ts, rl, half);
            lds_settle();
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
                if (lane + 64 * cc < HP) {
                    cs_b2s[cc] += (double)tile_colsum_domain(Ts, ld, lane + 64 * cc, R, base, 0);
                    cs_b2t[cc] += (double)tile_colsum_domain(Ts, ld, lane + 64 * cc, R, base, 1);
                }
            lds_settle();
        }
        // ---- p = r2 w3; (3) q = r1 (W2^T p)
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = ((r2 >> (16 * t + q)) & 1) ? w3s[acc_unit(t, q, half)] : 0.f;
        acc_to_tile<HT>(acc, Ts, rl, half);                             // P
        lds_settle();
        if (MODE == 0) tile_store_ws<HT>(Pw, h, base, M, Ts, lane);
        prod_t<HT>(Ws, Ts, h, rl, half, acc);
#pragma unroll
        for (int t = 0; t < HT; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = ((r1 >> (16 * t + q)) & 1) ? acc[t][q] : 0.f;
        lds_settle();
        acc_to_tile<HT>(acc, Ts, rl, half);                             // Q
        lds_settle();
        if (MODE == 0) {
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
                if (lane + 64 * cc < HP) cs_b1[cc] += (double)tile_colsum_sigma(Ts, ld, lane + 64 * cc, R, base);
            tile_store_ws<HT>(Qw, h, base, M, Ts, lane);
        }
        __syncthreads();
        // ---- (4) g = W1^T q
        stage_weight<HT>(C.W1, h, Ws);
        __syncthreads();
        prod_t<HT>(Ws, Ts, h, rl, half, acc);
        if (MODE == 1) {
            const float sc = live ? (r < R.n_s ? 1.f / (float)R.n_s : -1.f / (float)R.n_t) : 0.f;
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] *= sc;
            lds_settle();
            acc_to_tile<HT>(acc, Ts, rl, half);
            lds_settle();
            // rows [0, n_s) of the tile go to ges, the others to get
            if (ges || get) {
#pragma unroll 8
                for (int k = 0; k < RT * HP / 64; ++k) {
                    const int idx = lane + 64 * k, row = idx / HP, col = idx % HP;
                    const int64_t g = base + row;
                    if (g < M && col < h) {
                        const float v = Ts[row * ld + col];
                        if (g < R.n_s) { if (ges) ges[g * h + col] = v; }
                        else if (get) get[(g - R.n_s) * h + col] = v;
                    }
                }
            }
        } else {
            float n2 = 0.f;
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) n2 = fmaf(acc[t][q], acc[t][q], n2);
            n2 += __shfl_xor(n2, 32, 64);
            const float n = sqrtf(n2), inv = n > 0.f ? 1.f / n : 0.f;
            const float c = live ? GP_WEIGHT3 * 2.f * (n - 1.f) / (float)M : 0.f;
            if (live && half == 0) acc_pen += (double)((n - 1.f) * (n - 1.f));
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] *= inv;          // ghat
            // ---- Y1 = sigma x + c ghat, in place over the reloaded x (a lane pair owns its row)
            lds_settle();
            tile_load_x<HT>(R, h, base, M, Ts, lane);
            lds_settle();
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    float* y = Ts + rl * ld + acc_unit(t, q, half);
                    *y = sigma * *y + c * acc[t][q];
                }
            lds_settle();
            tile_store_ws<HT>(Y1w, h, base, M, Ts, lane);
            lds_settle();
            acc_to_tile<HT>(acc, Ts, rl, half);                         // Ghat
            lds_settle();
            // ---- (5) t = r1 (W1 ghat)
            prod_n<HT>(Ws, Ts, h, rl, half, acc);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = ((r1 >> (16 * t + q)) & 1) ? acc[t][q] : 0.f;
            // ---- Y2 = sigma h1 + c t over the h1 this wavefront parked in Y2's rows
            lds_settle();
            tile_load_ws<HT>(Y2w, h, base, M, Ts, lane);
            lds_settle();
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    float* y = Ts + rl * ld + acc_unit(t, q, half);
                    *y = sigma * *y + c * acc[t][q];
                }
            lds_settle();
            tile_store_ws<HT>(Y2w, h, base, M, Ts, lane);
            lds_settle();
            acc_to_tile<HT>(acc, Ts, rl, half);                         // T
            __syncthreads();
            // ---- (6) s = r2 (W2 t): gw3's penalty part sum c s
            stage_weight<HT>(C.W2, h, Ws);
            __syncthreads();
            prod_n<HT>(Ws, Ts, h, rl, half, acc);
#pragma unroll
            for (int t = 0; t < HT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[t][q] = ((r2 >> (16 * t + q)) & 1) ? c * acc[t][q] : 0.f;
            lds_settle();
            acc_to_tile<HT>(acc, Ts, rl, half);
            lds_settle();
#pragma unroll
            for (int cc = 0; cc < NC; ++cc)
                if (lane + 64 * cc < HP) cs_w3[cc] += (double)tile_colsum(Ts, ld, lane + 64 * cc);
        }
        __syncthreads();                                                // the weight and the tiles are free for the next trip
    }
    // ---- block partials part[column][block] over the dynamic LDS (free after the last barrier)
    __syncthreads();
    double* red = reinterpret_cast<double*>(smem);                      // [WAVES][NCOL]
#pragma unroll
    for (int cc = 0; cc < HMAX3 / 64; ++cc) {
        const int c = lane + 64 * cc;
        const bool has = cc < NC && c < HP;
        red[wave * NCOL + c] = has ? cs_b1[cc < NC ? cc : 0] : 0.0;
        red[wave * NCOL + HMAX3 + c] = has ? cs_b2s[cc < NC ? cc : 0] : 0.0;
        red[wave * NCOL + 2 * HMAX3 + c] = has ? cs_b2t[cc < NC ? cc : 0] : 0.0;
        red[wave * NCOL + 3 * HMAX3 + c] = has ? cs_w3[cc < NC ? cc : 0] : 0.0;
    }
    const double ss = wave_sum(acc_sig_s), st = wave_sum(acc_sig_t), ds = wave_sum(acc_ds), dt = wave_sum(acc_dt), pn = wave_sum(acc_pen);
    if (lane == 0) {
        red[wave * NCOL + NSC + 0] = ss; red[wave * NCOL + NSC + 1] = st; red[wave * NCOL + NSC + 2] = ds;
        red[wave * NCOL + NSC + 3] = dt; red[wave * NCOL + NSC + 4] = pn;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NCOL; t += TB) {
        double v = 0.0;
        for (int w = 0; w < WAVES; ++w) v += red[w * NCOL + t];
        part[(int64_t)t * gridDim.x + blockIdx.x] = v;
    }
}

// sum of one column of the block partials by ONE wavefront: coalesced loads, fixed order
__device__ __forceinline__ double column_sum3(const double* __restrict__ part, int col, int blocks, int lane) {
    double v = 0.0;
    for (int b = lane; b < blocks; b += 64) v += part[(int64_t)col * blocks + b];
    return wave_sum(v);
}

// gb1, gb2, gw3, gb3 and the loss from the block partials (one wavefront per output); with Adam on, the update of the six
// tensors: the vectors by the lane that formed the gradient, W1 and W2 elementwise from the gradients the GEMMs wrote.
// The step counters were incremented by the row kernel.
__global__ void __launch_bounds__(TB)
k_critic3_fold(int h, int64_t n_s, int64_t n_t, const float* w3, const double* __restrict__ part, int blocks, float* __restrict__ loss,
               const float* __restrict__ gW1, float* __restrict__ gb1, const float* __restrict__ gW2, float* __restrict__ gb2,
               float* __restrict__ gw3, float* __restrict__ gb3, Adam3 ad) {
    const int t = threadIdx.x, lane = t % 64;
    const int gw = blockIdx.x * WAVES + t / 64, nw = gridDim.x * WAVES;
    auto update = [&](int k, int64_t i, float g) {
        if (ad.on)
            gda_adam_element(ad.p[k] + i, g, ad.m[k] + i, ad.v[k] + i, gda_adam_coef(*ad.step[k], ad.lr, ad.beta1, ad.beta2),
                             ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
    };
    for (int k = gw; k < h + 2; k += nw) {
        if (k < h) {                                                    // unit k: gb1, gb2, gw3 (w3 read before its update)
            const int u = k;
            const double s1 = column_sum3(part, u, blocks, lane);
            const double cs = column_sum3(part, HMAX3 + u, blocks, lane), ct = column_sum3(part, 2 * HMAX3 + u, blocks, lane);
            const double s3 = column_sum3(part, 3 * HMAX3 + u, blocks, lane);
            if (lane == 0) {
                const float v1 = (float)s1, v2 = (float)((double)w3[u] * (ct / (double)n_t - cs / (double)n_s)), v3 = (float)s3;
                gb1[u] = v1; update(1, u, v1);
                gb2[u] = v2; update(3, u, v2);
                gw3[u] = v3; update(4, u, v3);
            }
        } else if (k == h) {
            // each domain's sum rounded to the output's precision, then added: -1 + 1 whenever the two round to it
            const double ss = column_sum3(part, NSC, blocks, lane), st = column_sum3(part, NSC + 1, blocks, lane);
            if (lane == 0) { const float v = (float)ss + (float)st; gb3[0] = v; update(5, 0, v); }
        } else {
            const double ds = column_sum3(part, NSC + 2, blocks, lane), dt = column_sum3(part, NSC + 3, blocks, lane);
            const double pn = column_sum3(part, NSC + 4, blocks, lane);
            if (lane == 0)                                              // specreg.py:196-199
                loss[0] = (float)(-(ds / (double)n_s - dt / (double)n_t) + (double)GP_WEIGHT3 * pn / (double)(n_s + n_t));
        }
    }
    if (ad.on) {
        const int64_t hh = (int64_t)h * h;
        const GdaAdamCoef c1 = gda_adam_coef(*ad.step[0], ad.lr, ad.beta1, ad.beta2);
        const GdaAdamCoef c2 = gda_adam_coef(*ad.step[2], ad.lr, ad.beta1, ad.beta2);
        for (int64_t e = (int64_t)blockIdx.x * TB + t; e < 2 * hh; e += (int64_t)gridDim.x * TB) {
            if (e < hh) gda_adam_element(ad.p[0] + e, gW1[e], ad.m[0] + e, ad.v[0] + e, c1, ad.beta1, ad.beta2, ad.eps, ad.weight_decay);
            else gda_adam_element(ad.p[2] + (e - hh), gW2[e - hh], ad.m[2] + (e - hh), ad.v[2] + (e - hh), c2, ad.beta1, ad.beta2, ad.eps,
                                  ad.weight_decay);
        }
    }
}

// means[0] = mean_s D, means[1] = mean_t D
__global__ void __launch_bounds__(64)
k_critic3_gap_fold(int64_t n_s, int64_t n_t, const double* __restrict__ part, int blocks, float* __restrict__ means) {
    const int lane = threadIdx.x;
    const double ds = column_sum3(part, NSC + 2, blocks, lane), dt = column_sum3(part, NSC + 3, blocks, lane);
    if (lane == 0) { means[0] = (float)(ds / (double)n_s); means[1] = (float)(dt / (double)n_t); }
}

struct Ws3 {
    double* part; float* Q; float* Y1; float* P; float* Y2; void* gemm_ws; size_t gemm_bytes;
    size_t total;
};

Ws3 carve3(void* base, int64_t M, int h, bool update) {
    Ws3 w{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        void* p = base ? (void*)((char*)base + off) : nullptr;
        off += gda_align_up(bytes, 256);
        return p;
    };
    w.part = (double*)take(sizeof(double) * ROW_BLOCKS3 * NCOL);
    if (update) {
        w.Q = (float*)take(sizeof(float) * M * h);
        w.Y1 = (float*)take(sizeof(float) * M * h);
        w.P = (float*)take(sizeof(float) * M * h);
        w.Y2 = (float*)take(sizeof(float) * M * h);
        w.gemm_bytes = gda_gemm_workspace_bytes(GDA_GEMM_TN, h, h, M);
        w.gemm_ws = take(w.gemm_bytes);
    }
    w.total = off;
    return w;
}

bool envelope3(int64_t n_s, int64_t n_t, int h) { return h % 4 == 0 && h >= 4 && h <= HMAX3 && n_s >= 1 && n_t >= 1; }

template <int MODE>
int launch_rows3(const Critic3& C, const Rows3& R, const Ws3& ws, float* ges, float* get, const Adam3& ad, int* blocks_out,
                 hipStream_t stream) {
    const int64_t M = R.n_s + R.n_t;
    const int64_t want = gda_cdiv(gda_cdiv(M, RT), WAVES);
    const int blocks = (int)(want < ROW_BLOCKS3 ? want : ROW_BLOCKS3);
    const int HT = (C.h + 31) / 32;
    const size_t lds = sizeof(float) * (size_t)(32 * HT + 1) * (32 * HT + WAVES * RT);
#define GDA_CRITIC3_ROWS(HT_)                                                                                       \
    {                                                                                                               \
        GDA_LDS_ATTR_ONCE((k_critic3_rows<HT_, MODE>), lds);                                                        \
        k_critic3_rows<HT_, MODE><<<blocks, TB, lds, stream>>>(C, R, ws.Q, ws.Y1, ws.P, ws.Y2, ges, get, ws.part, ad); \
    }
    switch (HT) {
        case 1: GDA_CRITIC3_ROWS(1) break;
        case 2: GDA_CRITIC3_ROWS(2) break;
        case 3: GDA_CRITIC3_ROWS(3) break;
        default: GDA_CRITIC3_ROWS(4) break;
    }
#undef GDA_CRITIC3_ROWS
    GDA_LAUNCH_CHECK();
    *blocks_out = blocks;
    return GDA_OK;
}

int critic3_update(const float* es, int64_t n_s, const float* et, int64_t n_t, int h, const Critic3& C, float* loss, float* gW1,
                   float* gb1, float* gW2, float* gb2, float* gw3, float* gb3, const Adam3& ad, void* workspace,
                   size_t workspace_bytes, gda_stream_t stream_) {
    if (n_s <= 0 || n_t <= 0 || h <= 0 || n_s + n_t >= INT32_MAX / 2) return GDA_E_SIZE;
    if (!es || !et || !C.W1 || !C.b1 || !C.W2 || !C.b2 || !C.w3 || !C.b3 || !loss || !gW1 || !gb1 || !gW2 || !gb2 || !gw3 || !gb3
        || !workspace)
        return GDA_E_NULL;
    if (!envelope3(n_s, n_t, h)) return GDA_E_UNSUPPORTED;
    if (((uintptr_t)es | (uintptr_t)et | (uintptr_t)C.W1 | (uintptr_t)C.W2) % 4 != 0 || (uintptr_t)workspace % 16 != 0) return GDA_E_UNSUPPORTED;
    const int64_t M = n_s + n_t;
    const Ws3 ws = carve3(workspace, M, h, true);
    if (workspace_bytes < ws.total) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const Rows3 R{es, n_s, et, n_t};
    int blocks = 0;
    int st = launch_rows3<0>(C, R, ws, nullptr, nullptr, ad, &blocks, stream);
    if (st != GDA_OK) return st;
    st = gda_gemm_f32(GDA_GEMM_TN, h, h, M, ws.Q, h, ws.Y1, h, gW1, h, ws.gemm_ws, ws.gemm_bytes, stream_);
    if (st != GDA_OK) return st;
    st = gda_gemm_f32(GDA_GEMM_TN, h, h, M, ws.P, h, ws.Y2, h, gW2, h, ws.gemm_ws, ws.gemm_bytes, stream_);
    if (st != GDA_OK) return st;
    k_critic3_fold<<<16, TB, 0, stream>>>(h, n_s, n_t, C.w3, ws.part, blocks, loss, gW1, gb1, gW2, gb2, gw3, gb3, ad);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

constexpr int HINGE_TB = 256;
constexpr int HINGE_BLOCKS = 256;                    // grid cap: one double pair of partials per workgroup

// value = gamma_s mean relu(|X[i] - X[i+1]| - thr_s) + gamma_m mean relu(|X| - thr_m), G = d value / d X; a term is present
// only if its threshold is > 0; relu'(0) = 0, abs'(0) = 0 (torch's).  Every workgroup leaves its two double sums in
// part[2 block ..]; the workgroup that draws the last ticket adds them in block order -- a fixed order whichever it is --
// and hands the ticket counter back at 0 (the host zeroes it before the launch).
__global__ void __launch_bounds__(HINGE_TB)
k_spectral_hinge(const float* __restrict__ X, int64_t k, int64_t h, float thr_s, float gam_s, float thr_m, float gam_m,
                 float* __restrict__ value, float* __restrict__ G, double* __restrict__ part, unsigned int* __restrict__ ticket) {
    __shared__ double red[HINGE_TB];
    __shared__ bool last;
    const bool on_s = thr_s > 0.f, on_m = thr_m > 0.f;
    const double cnt_s = (double)(k - 1) * (double)h, cnt_m = (double)k * (double)h;
    const float ws = on_s ? (float)((double)gam_s / cnt_s) : 0.f, wm = on_m ? (float)((double)gam_m / cnt_m) : 0.f;
    double sum_s = 0.0, sum_m = 0.0;
    auto sgn = [](float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); };
    for (int64_t e = (int64_t)blockIdx.x * HINGE_TB + threadIdx.x; e < k * h; e += (int64_t)gridDim.x * HINGE_TB) {
        const int64_t i = e / h;
        const float x = X[e];
        float g = 0.f;
        if (on_m) {
            const float v = fabsf(x) - thr_m;
            if (v > 0.f) { sum_m += (double)v; g += wm * sgn(x); }
        }
        if (on_s) {
            if (i + 1 < k) {
                const float d = x - X[e + h], v = fabsf(d) - thr_s;
                if (v > 0.f) { sum_s += (double)v; g += ws * sgn(d); }
            }
            if (i > 0) {
                const float d = X[e - h] - x, v = fabsf(d) - thr_s;
                if (v > 0.f) g -= ws * sgn(d);
            }
        }
        G[e] = g;
    }
    const double ts = block_sum_d(sum_s, red), tm = block_sum_d(sum_m, red);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = ts; part[2 * blockIdx.x + 1] = tm;
        __threadfence();                                                // the partials before the ticket
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double a = 0.0, b = 0.0;
    if (threadIdx.x < (int)gridDim.x) {                                 // gridDim.x <= HINGE_BLOCKS == HINGE_TB
        a = __hip_atomic_load(part + 2 * threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // past this CU's L1
        b = __hip_atomic_load(part + 2 * threadIdx.x + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const double fs = block_sum_d(a, red), fm = block_sum_d(b, red);
    if (threadIdx.x == 0) {
        value[0] = (float)((on_s ? (double)gam_s * fs / cnt_s : 0.0) + (on_m ? (double)gam_m * fm / cnt_m : 0.0));
        *ticket = 0u;
    }
}

}  // namespace

extern "C" int gda_critic3_rows_per_trip(void) { return ROW_BLOCKS3 * WAVES * RT; }

extern "C" size_t gda_critic3_workspace_bytes(int64_t n_s, int64_t n_t, int h) {
    if (n_s <= 0 || n_t <= 0 || h <= 0) return 0;
    return carve3(nullptr, n_s + n_t, h, true).total;
}

extern "C" int gda_critic3_update_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                                      const float* W1, const float* b1, const float* W2, const float* b2, const float* w3,
                                      const float* b3, float* loss, float* gW1, float* gb1, float* gW2, float* gb2,
                                      float* gw3, float* gb3, void* workspace, size_t workspace_bytes, gda_stream_t stream_) {
    Adam3 ad{};
    const Critic3 C{W1, b1, W2, b2, w3, b3, h};
    return critic3_update(es, n_s, et, n_t, h, C, loss, gW1, gb1, gW2, gb2, gw3, gb3, ad, workspace, workspace_bytes, stream_);
}

extern "C" int gda_critic3_update_adam_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h, float* loss,
                                           const gda_adam_tensor* params, float lr, float beta1, float beta2, float eps,
                                           float weight_decay, void* workspace, size_t workspace_bytes, gda_stream_t stream_) {
    if (!params) return GDA_E_NULL;
    if (h <= 0) return GDA_E_SIZE;
    Adam3 ad{};
    const int64_t want[6] = {(int64_t)h * h, h, (int64_t)h * h, h, h, 1};
    for (int k = 0; k < 6; ++k) {
        const gda_adam_tensor& t = params[k];
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || !t.step) return GDA_E_NULL;
        if (t.numel != want[k]) return GDA_E_SIZE;
        ad.p[k] = t.param; ad.m[k] = t.exp_avg; ad.v[k] = t.exp_avg_sq; ad.step[k] = t.step;
    }
    ad.lr = lr; ad.beta1 = beta1; ad.beta2 = beta2; ad.eps = eps; ad.weight_decay = weight_decay; ad.on = 1;
    const Critic3 C{params[0].param, params[1].param, params[2].param, params[3].param, params[4].param, params[5].param, h};
    auto g = [&](int k) { return const_cast<float*>(params[k].grad); };
    return critic3_update(es, n_s, et, n_t, h, C, loss, g(0), g(1), g(2), g(3), g(4), g(5), ad, workspace, workspace_bytes, stream_);
}

extern "C" int gda_critic3_gap_f32(const float* es, int64_t n_s, const float* et, int64_t n_t, int h,
                                   const float* W1, const float* b1, const float* W2, const float* b2, const float* w3,
                                   const float* b3, float* means, float* ges, float* get, void* workspace,
                                   size_t workspace_bytes, gda_stream_t stream_) {
    if (n_s <= 0 || n_t <= 0 || h <= 0 || n_s + n_t >= INT32_MAX / 2) return GDA_E_SIZE;
    if (!es || !et || !W1 || !b1 || !W2 || !b2 || !w3 || !b3 || !means || !workspace) return GDA_E_NULL;
    if (!envelope3(n_s, n_t, h)) return GDA_E_UNSUPPORTED;
    if (((uintptr_t)es | (uintptr_t)et | (uintptr_t)W1 | (uintptr_t)W2) % 4 != 0 || (uintptr_t)workspace % 16 != 0) return GDA_E_UNSUPPORTED;
    const Ws3 ws = carve3(workspace, n_s + n_t, h, false);
    if (workspace_bytes < ws.total) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const Critic3 C{W1, b1, W2, b2, w3, b3, h};
    const Rows3 R{es, n_s, et, n_t};
    Adam3 ad{};
    int blocks = 0;
    const int st = launch_rows3<1>(C, R, ws, ges, get, ad, &blocks, stream);
    if (st != GDA_OK) return st;
    k_critic3_gap_fold<<<1, 64, 0, stream>>>(n_s, n_t, ws.part, blocks, means);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_spectral_hinge_workspace_bytes(int64_t k, int64_t h) {
    (void)k; (void)h;
    return 256 + sizeof(double) * 2 * HINGE_BLOCKS;      // the ticket counter, the workgroups' partial sums
}

extern "C" int gda_spectral_hinge_f32(const float* X, int64_t k, int64_t h, float thr_smooth, float gamma_smooth,
                                      float thr_mfr, float gamma_mfr, float* value, float* G, void* workspace,
                                      size_t workspace_bytes, gda_stream_t stream_) {
    if (k <= 0 || h <= 0 || k * h >= INT32_MAX) return GDA_E_SIZE;
    if (thr_smooth > 0.f && k < 2) return GDA_E_SIZE;    // the mean over no differences
    if (!X || !value || !G || !workspace) return GDA_E_NULL;
    if ((uintptr_t)workspace % 16 != 0) return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_spectral_hinge_workspace_bytes(k, h)) return GDA_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    unsigned int* ticket = (unsigned int*)workspace;
    double* part = (double*)((char*)workspace + 256);
    GDA_HIP_TRY(hipMemsetAsync(ticket, 0, sizeof(unsigned int), stream));
    const int64_t want = gda_cdiv(k * h, HINGE_TB);
    const int blocks = (int)(want < HINGE_BLOCKS ? want : HINGE_BLOCKS);
    k_spectral_hinge<<<blocks, HINGE_TB, 0, stream>>>(X, k, h, thr_smooth, gamma_smooth, thr_mfr, gamma_mfr, value, G, part, ticket);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
