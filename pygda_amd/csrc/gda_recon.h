// The all-pairs graph reconstruction pass that gda_asn.hip and gda_dgda.hip share: loss = c * sum_ij f(x_ij, y_ij) with
// x = z z^T and f torch's stable pos_weight-ed BCE-with-logits
//   f = (1 - y) x + (1 + (pw - 1) y) (log1p(exp(-|x|)) + max(-x, 0)),
// and S Z with S_ij = df / dx, per chunk of the columns.  No N x N buffer exists: S lives in LDS for one 32 x 64 tile.
// Where a pair's label y comes from is the kernel's Labels policy, a struct passed by value:
//   NoLabels   (ASN) every pair takes y = 0, f_0 = softplus(x) and f_0' = sigmoid(x); the label term compiles away and
//              the caller corrects its labelled pairs afterwards (gda_asn.hip's k_recon_fold walks the label CSR).
//   BitLabels  (DGDA) y = the pair's bit of the bit adjacency, + 1 on the diagonal; pos_weight from the device scalars.
// A policy has pm1() = pos_weight - 1, tile(i, row_live, j0) = what row i needs of the column tile at j0 (loaded before
// the barrier), and y(tile, i, j0, jj) = the label of pair (i, j0 + jj).
#ifndef GDA_RECON_H
#define GDA_RECON_H

#include "gda_common.h"
#include "gda_reduce.h"

namespace gda_recon {

constexpr int TB = 256;
constexpr int RT_I = 32;                    // k_recon_pairs: rows per block
constexpr int RT_J = 64;                    // k_recon_pairs: columns per tile (two words of a bit row)

struct NoLabels {
    struct Tile {};
    __device__ __forceinline__ float pm1() const { return 0.f; }
    __device__ __forceinline__ Tile tile(int, bool, int) const { return {}; }
    __device__ __forceinline__ float y(const Tile&, int, int, int) const { return 0.f; }
};

struct BitLabels {
    int W;                                  // words per row of bits
    const uint32_t* __restrict__ bits;
    const float* __restrict__ scal;         // scal[1] = pos_weight
    struct Tile { uint32_t wd[2]; };
    __device__ __forceinline__ float pm1() const { return scal[1] - 1.f; }
    __device__ __forceinline__ Tile tile(int i, bool row_live, int j0) const {
        Tile t = {{0u, 0u}};
        if (row_live) {
            const int w0 = j0 >> 5;
            t.wd[0] = bits[(int64_t)i * W + w0];
            if (w0 + 1 < W) t.wd[1] = bits[(int64_t)i * W + w0 + 1];
        }
        return t;
    }
    __device__ __forceinline__ float y(const Tile& t, int i, int j0, int jj) const {
        return (float)((t.wd[jj >> 5] >> (jj & 31)) & 1u) + (j0 + jj == i ? 1.f : 0.f);
    }
};

namespace {

// a block = 32 rows x one chunk of the columns: 64-column tiles of Z staged in LDS, x, f and df / dx of the 32 x 64 tile
// (8 pairs per lane), then the tile's S Z_j into per-lane accumulators; the block's loss sum goes to lpart and its
// [32, K] slab of S Z to part, per chunk.  Three spellings are load-bearing for NoLabels (profiles/recon_shared_ab.txt):
// log1p under `if (live)` (outside it the eight pairs of a lane interleave and the registers double), the loss block
// before the sigmoid (after it the select sinks into the block: +1.8 %), and the policy as the last argument (ASN's
// argument block stays as it was).
template <int KP, class Labels>
__global__ void __launch_bounds__(TB) k_recon_pairs(const float* __restrict__ z, int64_t ldz, int n, int K,
                                                    int tiles_per_chunk, float* __restrict__ part,
                                                    float* __restrict__ lpart, Labels lab) {
    __shared__ float zi[RT_I][KP + 1];
    __shared__ float zj[RT_J][KP + 1];
    __shared__ float S[RT_I][RT_J + 1];
    __shared__ float red[TB];
    const int t = threadIdx.x;
    const int i0 = blockIdx.x * RT_I;
    const int chunk = blockIdx.y;
    const int ntj = (n + RT_J - 1) / RT_J;
    const int jt0 = chunk * tiles_per_chunk;
    const int jt1 = min(jt0 + tiles_per_chunk, ntj);
    const float pm1 = lab.pm1();
    for (int idx = t; idx < RT_I * KP; idx += TB) {
        const int r = idx / KP, k = idx % KP;
        zi[r][k] = (i0 + r < n && k < K) ? z[(int64_t)(i0 + r) * ldz + k] : 0.f;
    }
    constexpr int Q = KP / 8;
    float acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.f;
    float lsum = 0.f;
    const int pi = t >> 3, pj = t & 7;              // pairs (pi, pj + 8m); outputs (pi, pj + 8q)
    const int i = i0 + pi;
    const bool row_live = i < n;
    for (int jt = jt0; jt < jt1; ++jt) {
        const int j0 = jt * RT_J;
        __syncthreads();
        for (int idx = t; idx < RT_J * KP; idx += TB) {
            const int r = idx / KP, k = idx % KP;
            zj[r][k] = (j0 + r < n && k < K) ? z[(int64_t)(j0 + r) * ldz + k] : 0.f;
        }
        const typename Labels::Tile lt = lab.tile(i, row_live, j0);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int jj = pj + 8 * m;
            float x = 0.f;
#pragma unroll 8
            for (int k = 0; k < KP; ++k) x = fmaf(zi[pi][k], zj[jj][k], x);
            const bool live = row_live && j0 + jj < n;
            const float y = lab.y(lt, i, j0, jj);
            const float e = expf(-fabsf(x));
            const float r = 1.f / (1.f + e);
            if (live) {
                const float l = log1pf(e);
                float f = l + fmaxf(x, 0.f);
                if (y != 0.f) f += -y * x + pm1 * y * (l + fmaxf(-x, 0.f));
                lsum += f;
            }
            float d = x >= 0.f ? r : e * r;                                 // sigmoid(x)
            if (y != 0.f) d += -y - pm1 * y * (x >= 0.f ? e * r : r);       // sigmoid(-x)
            S[pi][jj] = live ? d : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < RT_J; ++jj) {
            const float s = S[pi][jj];
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] = fmaf(s, zj[jj][pj + 8 * q], acc[q]);
        }
    }
    if (row_live) {
        float* o = part + ((int64_t)chunk * n + i) * K;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int k = pj + 8 * q;
            if (k < K) o[k] = acc[q];
        }
    }
    const float bs = block_sum_f(lsum, red);
    if (t == 0) lpart[(int64_t)chunk * gridDim.x + blockIdx.x] = bs;
}

// one block: loss = c * (the block partials, then the nrows row corrections, each in strided order, in double);
// c by value, or formed here as norm[0] / n^2 where the norm is a device scalar
__global__ void __launch_bounds__(TB) k_recon_final(const float* __restrict__ lpart, int nparts,
                                                    const float* __restrict__ rowloss, int nrows, float c,
                                                    const float* __restrict__ norm, int n, float* __restrict__ loss) {
    __shared__ double red[TB];
    const double tot = block_sum_d(stride_sum_d<TB>(rowloss, nrows, stride_sum_d<TB>(lpart, nparts)), red);
    if (norm != nullptr) c = (float)((double)norm[0] / ((double)n * (double)n));
    if (threadIdx.x == 0) loss[0] = (float)((double)c * tot);
}

}  // namespace

// column chunks of the pair pass: enough blocks for the chip (~2048 blocks of 32 rows), at least 4 column tiles per chunk
inline int chunks(int64_t n) {
    const int64_t row_blocks = gda_cdiv(n, RT_I);
    const int64_t ntj = gda_cdiv(n, RT_J);
    int64_t ch = gda_cdiv(2048, row_blocks);
    const int64_t cap = gda_cdiv(ntj, 4);
    if (ch > cap) ch = cap;
    if (ch > GDA_ASN_MAX_CHUNKS) ch = GDA_ASN_MAX_CHUNKS;
    return (int)(ch < 1 ? 1 : ch);
}

// the pair pass at the narrowest padded width that holds K (K <= GDA_ASN_MAX_K): part [chunks(n), n, K], lpart
// [chunks(n), ceil(n / 32)]
template <class Labels>
int launch_pairs(const float* z, int64_t ldz, int n, int K, Labels lab, float* part, float* lpart, hipStream_t s) {
    const int ch = chunks(n);
    const int tpc = (int)gda_cdiv(gda_cdiv(n, RT_J), ch);
    const dim3 grid((unsigned)gda_cdiv(n, RT_I), (unsigned)ch);
    if (K <= 8) k_recon_pairs<8><<<grid, TB, 0, s>>>(z, ldz, n, K, tpc, part, lpart, lab);
    else if (K <= 16) k_recon_pairs<16><<<grid, TB, 0, s>>>(z, ldz, n, K, tpc, part, lpart, lab);
    else if (K <= 32) k_recon_pairs<32><<<grid, TB, 0, s>>>(z, ldz, n, K, tpc, part, lpart, lab);
    else if (K <= 64) k_recon_pairs<64><<<grid, TB, 0, s>>>(z, ldz, n, K, tpc, part, lpart, lab);
    else k_recon_pairs<128><<<grid, TB, 0, s>>>(z, ldz, n, K, tpc, part, lpart, lab);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

}  // namespace gda_recon

#endif
