// Tall products on the 16-bit matrix cores with SPLIT operands (round 5; included by gda_gemm.hip inside its namespace).
//
// The dense hidden x weight contraction of a sampled batch (pygda/nn/prop_gcn_conv.py:136,200 at 10^5 rows: forward
// y = x W^T and data gradient gx = gy W) on k_tall_fwd16 runs at 0.45 - 0.6 of the fp32 matrix-core roof, 80 - 120 us for
// a product that moves 160 MB.  The fp32 MFMA is 1/16 of the 16-bit pipe's rate; fp32 accuracy survives on that pipe with
// split operands (csrc/gda_mmd_fused.inc, round 4): a = hi + lo, hi = fp16(a), lo = fp16(a - hi) carries 22 significant
// bits, a.b = hi.hi + hi.lo + lo.hi (+ lo.lo, 2^-22 relative, dropped) is three v_mfma_f32_16x16x32_f16 accumulating in
// fp32.  fp16's exponent range is kept out of the way by ONE power of two per ROW of the tall operand and per output
// column of the weight (largest entry into [2^13, 2^14); applied exactly, undone exactly in the epilogue) -- a row's scale
// needs the whole row, so the staging is row-complete: a tile is 128 rows x K (64 rows at K = 256), loaded as 16-byte
// pieces by a lane group per row, its largest entry found with a butterfly, split in registers and written as two
// row-major fp16 images (row stride K + 8 halves: the 16-byte operand fetch of 16 rows is conflict-free).
// Workgroup = 8 waves, wave w = 16 output columns with its weight slice hi | lo in registers for the whole kernel
// (K/32 x 8 registers), persistent over the row tiles, double-buffered images, one barrier per tile, the next tile's
// global loads in flight under the current tile's MFMAs.  Matrix time: 3 x 16 cycles per 16 x 16 x 32 block against
// 8 x 32 for the fp32 form -- the kernel is bound by its 160 MB of traffic, not by the matrix pipe.
// Error: 2^-22 of sum |a_k b_k| per output (the class of an fp32 fma chain in another order); tests/test_gpu_parity.py::
// test_tall_gemm_weight_in_registers_vs_fp64 holds its fp32-level bound through it.  PYGDA_AMD_GEMM_SPLIT_F16=0 keeps
// k_tall_fwd16.

using gh8 = __attribute__((ext_vector_type(8))) _Float16;
using gh4 = __attribute__((ext_vector_type(4))) _Float16;

// power of two s with max * s in [2^13, 2^14) (1 for max = 0 or denormal-small), and its inverse
__device__ __forceinline__ void split_scale(float mx, float& s, float& sinv) {
    const int ex = (int)((__float_as_uint(mx) >> 23) & 0xffu);          // biased exponent of the largest |entry|
    const bool ok = ex >= 24 && ex < 255;                                // (finite, not tiny: 267 - ex stays a normal exponent)
    s = ok ? __uint_as_float((uint32_t)(267 - ex) << 23) : 1.0f;         // 2^(13 - (ex - 127))
    sinv = ok ? __uint_as_float((uint32_t)(ex - 13) << 23) : 1.0f;       // 2^((ex - 127) - 13)
}

// Forward activation in the epilogue (ACT = 1: y = dropout_site0(relu(c)); ACT = 2: additionally row M + i of C receives a
// second, independent draw dropout_site1(relu(c)) -- the stacked pair of gda_relu_dropout_pair_fwd_f32).  Keep-bits in the
// format of gda_dropout.h on the row-major index of the [M, N] pre-activation; requires ldc == N.

template <int K, bool BT, int DBG = 0, int ACT = 0>
__global__ void __launch_bounds__(TALL_TB, 1)
k_tall_fwd_h(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb, float* __restrict__ C,
             int64_t ldc, int64_t M, const float* __restrict__ bias,
             const float* __restrict__ mask = nullptr, int64_t ldm = 0, float mscale = 1.f,
             const int64_t* __restrict__ arow = nullptr, GdaAct act = GdaAct{}) {
    // arow (may be NULL): row i of the tall operand is A[arow[i]] -- the feature gather of a sampled batch (x[n_id]) done by
    // the operand fetch instead of a gather pass that writes and re-reads [M, K]
    // mask (may be NULL): the output y [M, N] of the activation dropout(relu(.)) whose INPUT gradient this product is -- the
    // result is stored as y > 0 ? c * mscale : 0 (gda_relu_dropout_bwd_f32's values), the activation's backward launch and
    // one [M, N] round trip through HBM disappear
    constexpr int BM = K == 128 ? 128 : 64;           // rows of a tile
    constexpr int KB = K / 32;                        // 32-deep blocks of the reduction
    constexpr int RSB = (K + 8) * 2;                  // bytes per image row
    constexpr int IMG = BM * RSB;                     // bytes of one image (hi or lo)
    constexpr int LPR = K / 16;                       // lanes per row, four 16-byte pieces each: 8 or 16
    constexpr int RPP = TALL_TB / LPR;                // rows per staging pass: 64 or 32
    constexpr int PR = BM / RPP;                      // rows per thread and tile: 2
    constexpr int MS = BM / 16;                       // 16-row sub-tiles
    extern __shared__ __attribute__((aligned(16))) char th_lds[];
    // [buffer][hi | lo][BM rows][RSB bytes], then the rows' inverse scales [buffer][BM]
    float* rinv = reinterpret_cast<float*>(th_lds + 4 * IMG);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int kk = lane >> 4, lc = lane & 15;         // operand layout of both MFMA inputs: index lc, k = 8 kk .. 8 kk + 7
    const int64_t j0 = (int64_t)blockIdx.y * 128 + 16 * wave;
    // the weight slice: column j0 + lc, its own power of two, hi | lo halves per 32-deep block.  A lane loads exactly the
    // 8 K/32 values it holds (NT: 32 contiguous bytes per block, BT: coalesced across the 16 columns); the column's
    // largest entry is the maximum over the lane's values and its three partner lanes (k groups kk = 0..3: lanes lc + 16 kk).
    // (First versions: every lane walking its whole column twice -- 2 K dependent loads, 17 - 22 us of a 40 us kernel in
    // the NT form --, then the slice staged through LDS -- two barriers and K LDS reads per lane, 8 us.)
    gh8 bh[KB], bl[KB];
    float tinv;
    {
        float wv[KB][8];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
            const int k0 = kb * 32 + 8 * kk;
            if (BT) {
#pragma unroll
                for (int e = 0; e < 8; ++e) wv[kb][e] = B[(int64_t)(k0 + e) * ldb + j0 + lc];
            } else {
                const float4 p0 = *reinterpret_cast<const float4*>(B + (j0 + lc) * ldb + k0);
                const float4 p1 = *reinterpret_cast<const float4*>(B + (j0 + lc) * ldb + k0 + 4);
                wv[kb][0] = p0.x; wv[kb][1] = p0.y; wv[kb][2] = p0.z; wv[kb][3] = p0.w;
                wv[kb][4] = p1.x; wv[kb][5] = p1.y; wv[kb][6] = p1.z; wv[kb][7] = p1.w;
            }
        }
        float mx = 0.f;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(wv[kb][e]));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float t;
        split_scale(mx, t, tinv);
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float w = wv[kb][e] * t;
                const _Float16 h = (_Float16)w;
                bh[kb][e] = h;
                bl[kb][e] = (_Float16)(w - (float)h);
            }
    }
    // The products are formed TRANSPOSED, D[j][i] = sum_k W[j][k] A[i][k] (weight slice as the MFMA's first operand): the
    // accumulator layout then gives a lane FOUR CONSECUTIVE OUTPUT COLUMNS j0 + 4 kk .. + 3 of row 16 ms + lc -- one
    // 16-byte store per sub-tile instead of four 4-byte ones (the stores were 25 of the kernel's 62 us)
    float tq[4], bq[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        tq[r] = __shfl(tinv, 4 * kk + r, 16);
        bq[r] = bias ? bias[j0 + 4 * kk + r] : 0.f;
    }
    uint64_t act_st = 0;
    uint32_t act_thresh = 0;
    if constexpr (ACT != 0) {
        if (act.p > 0.f) {
            act_st = (uint64_t)act.step[0];
            act_thresh = dropout_thresh(act.p);
        }
    }
    const int64_t ntiles = (M + BM - 1) / BM;
    const int sr = tid / LPR, sp = tid % LPR;          // staging role: rows sr + RPP q, pieces sp + LPR j (floats 4 (sp + LPR j) ..)
    float4 v[PR][4];
    int64_t tile = blockIdx.x;
    if (tile >= ntiles) return;
#define TH_FETCH(TILE)                                                                                \
    _Pragma("unroll") for (int q = 0; q < PR; ++q) {                                                 \
        int64_t r = (TILE) * BM + sr + RPP * q;                                                      \
        r = r < M ? r : M - 1;      /* rows past the end: any valid address; their outputs are not stored */ \
        if (arow) r = arow[r];                                                                       \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                \
            v[q][j] = *reinterpret_cast<const float4*>(A + r * lda + 4 * (sp + LPR * j));            \
    }
#define TH_STASH(BUF)                                                                                 \
    _Pragma("unroll") for (int q = 0; q < PR; ++q) {                                                 \
        float mx = 0.f;                                                                              \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                \
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(v[q][j].x), fabsf(v[q][j].y)), fmaxf(fabsf(v[q][j].z), fabsf(v[q][j].w)))); \
        _Pragma("unroll") for (int off = LPR / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, LPR)); \
        float s, sinv;                                                                               \
        split_scale(mx, s, sinv);                                                                    \
        char* d = th_lds + (BUF) * 2 * IMG + (sr + RPP * q) * RSB;                                   \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                              \
            const float x0 = v[q][j].x * s, x1 = v[q][j].y * s, x2 = v[q][j].z * s, x3 = v[q][j].w * s; \
            gh4 h, l;                                                                                \
            h[0] = (_Float16)x0; h[1] = (_Float16)x1; h[2] = (_Float16)x2; h[3] = (_Float16)x3;      \
            l[0] = (_Float16)(x0 - (float)h[0]); l[1] = (_Float16)(x1 - (float)h[1]);                \
            l[2] = (_Float16)(x2 - (float)h[2]); l[3] = (_Float16)(x3 - (float)h[3]);                \
            *reinterpret_cast<gh4*>(d + 8 * (sp + LPR * j)) = h;                                     \
            *reinterpret_cast<gh4*>(d + IMG + 8 * (sp + LPR * j)) = l;                               \
        }                                                                                            \
        if (sp == 0) rinv[(BUF) * BM + sr + RPP * q] = sinv;                                         \
    }
    TH_FETCH(tile)
    TH_STASH(0)
    __syncthreads();
    int buf = 0;
    for (; tile < ntiles; tile += gridDim.x) {
        const bool more = tile + gridDim.x < ntiles;
        if (more) { TH_FETCH(tile + gridDim.x) }
        __builtin_amdgcn_sched_barrier(0);            // the loads go out before the tile's MFMAs, not between them
        // Odd waves split and stash the NEXT tile first, even waves multiply and store the current one first: the eight
        // waves of the workgroup (alone on its CU) otherwise move through the phases in lockstep -- matrix pipe idle
        // while everybody stores, memory idle while everybody multiplies (measured additive: 12 + 22 + 8 us of 51)
        if ((wave & 1) && more && !(DBG & 4)) { TH_STASH(buf ^ 1) }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[MS];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ms][r] = 0.f;
        const char* img = th_lds + buf * 2 * IMG + lc * RSB + 16 * kk;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) {
                if constexpr ((DBG & 2) != 0) continue;
                const gh8 ah = *reinterpret_cast<const gh8*>(img + ms * 16 * RSB + kb * 64);
                const gh8 al = *reinterpret_cast<const gh8*>(img + IMG + ms * 16 * RSB + kb * 64);
                acc[ms] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[kb], al, acc[ms], 0, 0, 0);
                acc[ms] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bl[kb], ah, acc[ms], 0, 0, 0);
                acc[ms] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bh[kb], ah, acc[ms], 0, 0, 0);
            }
        const float* ri = rinv + buf * BM;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms) {             // D layout: column lane % 16 = the tile's row 16 ms + lc, rows 4 kk + r = output columns
            const int lr = 16 * ms + lc;
            const int64_t i = tile * BM + lr;
            const float rs = ri[lr];
            float4 o;
            o.x = acc[ms][0] * (rs * tq[0]) + bq[0]; o.y = acc[ms][1] * (rs * tq[1]) + bq[1];
            o.z = acc[ms][2] * (rs * tq[2]) + bq[2]; o.w = acc[ms][3] * (rs * tq[3]) + bq[3];
            if (mask && i < M) {
                const float4 y = *reinterpret_cast<const float4*>(mask + i * ldm + j0 + 4 * kk);
                o = relu_keep_bwd(y, o, mscale);
            }
            if constexpr (ACT != 0) {
                if (i < M) {
                    const int64_t off = i * ldc + j0 + 4 * kk;
                    float4 o1 = o;
                    if (act.p > 0.f) {
                        const uint32_t thresh = act_thresh;
                        uint32_t rn[4];
                        dropout_draw(act.seed, act_st, act.site0, (uint64_t)(off >> 2), rn);
                        const float4 c = o;
                        o = relu_keep(c, rn, thresh, act.scale);
                        if constexpr (ACT == 2) {
                            dropout_draw(act.seed, act_st, act.site1, (uint64_t)(off >> 2), rn);
                            o1 = relu_keep(c, rn, thresh, act.scale);
                        }
                    } else {
                        o.x = o.x > 0.f ? o.x : (o.x != o.x ? o.x : 0.f); o.y = o.y > 0.f ? o.y : (o.y != o.y ? o.y : 0.f);
                        o.z = o.z > 0.f ? o.z : (o.z != o.z ? o.z : 0.f); o.w = o.w > 0.f ? o.w : (o.w != o.w ? o.w : 0.f);
                        o1 = o;
                    }
                    if constexpr (ACT == 2) *reinterpret_cast<float4*>(C + (M + i) * ldc + j0 + 4 * kk) = o1;
                }
            }
            if (i < M && !(DBG & 1)) *reinterpret_cast<float4*>(C + i * ldc + j0 + 4 * kk) = o;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!(wave & 1) && more && !(DBG & 4)) { TH_STASH(buf ^ 1) }
        __syncthreads();
        buf ^= 1;
    }
#undef TH_FETCH
#undef TH_STASH
}
