// DGDA for gfx950 (pygda/models/dgda.py, pygda/nn/dgda_base.py, pygda/nn/deepwalk_pretrain.py): the manipulated pass on a
// bit-packed dense adjacency, and DeepWalk's uniform walks.
//
// drop_edges draws its two Bernoulli masks over ALL N^2 pairs (torch.bernoulli(adj, p=...) ignores adj), so the manipulated
// adjacency is ~10 % dense and new every epoch.  It lives here as one bit per pair, bits [N, W = ceil(N / 32)] uint32, bit b
// of word w of row i = pair (i, 32 w + b); bits past column N - 1 are zero.
//   k_manip_add / k_manip_edges / k_pack_dense   the bit matrix: for i > j bit = add(i, j) OR (adj(i, j) - drop(i, j) > 0),
//                      mirrored, diagonal set.  The draws of pair (i, j), i > j, are words 0 (drop) and 1 (add) of the
//                      Philox block at counter i N + j, so both triangles and both kernels read the same draw.  The kept
//                      edges are OR-ed in from the label CSR of A + I (integer atomic OR: the result has no order).
//   k_bits_rows / k_bits_final   deg = popcount(row) + 1 (the encoder's in-place += I makes the diagonal 2), dis = deg^-1/2,
//                      and the device scalars n_lab = sum(bits) + N, pos_weight = (N^2 - n_lab) / n_lab,
//                      norm = N^2 / (2 (N^2 - n_lab)): integer sums, fixed order.
//   k_bitadj_gemm      out = dis * (B~ (dis * H)) + bias with B~ the bit matrix at diagonal weight 2: a GEMM over the nodes
//                      on v_mfma_f32_16x16x32_bf16.  One 32-bit word is the 32 contraction steps of one row, the lane's
//                      byte (lane >> 4) of it its 8 consecutive k: the 0/1 operand is expanded to bf16 in registers and is
//                      exact.  G = dis * H is split into three bf16 terms (hi + mid + lo carries 24 bits, no scaling:
//                      bf16 has fp32's exponent range) and staged transposed through LDS once per 64 nodes; a workgroup =
//                      128 rows x 64 columns, wave w = rows 32 w .. 32 w + 31.  The diagonal's second unit and the row
//                      scale are applied in fp32 in the epilogue.  Every output is one accumulator chain over the nodes in
//                      ascending order: two runs are bit-identical.
//   gda_recon::k_recon_pairs<KP, BitLabels> / k_rb_fold / gda_recon::k_recon_final   the all-pairs reconstruction loss
//                      of gda_recon.h with the label read from the bit tile (y = bit, + 1 on the diagonal); the labels
//                      are symmetric, so dZ = 2 c G Z with no sparse correction.  norm and pos_weight come from the
//                      device scalars.
//   k_walks            one lane per walk, a uniform neighbour per step from Philox; a node without out-edges stays put.
#include "gda_common.h"
#include "gda_philox.h"
#include "gda_recon.h"
#include "gda_reduce.h"

namespace {

using gda_recon::RT_I;
using gda_recon::TB;
constexpr int GM = 128, GN = 64, GK = 64;   // k_bitadj_gemm: rows, columns and nodes per stage of a workgroup
constexpr int GLD = GK + 8;                 // halves per image row: 16-byte aligned operand fetches

using bf8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ void manip_draw(uint64_t seed, uint64_t step, uint32_t site, uint64_t pair, float p_drop,
                                           float p_add, bool& drop, bool& add) {
    uint32_t r[4];
    GdaPhilox::gen(seed, ((uint64_t)site << 32) ^ (step * 0x9E3779B97F4A7C15ull), pair, r);
    drop = (float)(r[0] >> 8) * (1.f / 16777216.f) < p_drop;
    add = (float)(r[1] >> 8) * (1.f / 16777216.f) < p_add;
}

// ------------------------------------------------------------------------------------------------ bit matrix --
__global__ void __launch_bounds__(TB) k_manip_add(int n, int W, float p_drop, float p_add, uint64_t seed,
                                                  const int64_t* __restrict__ step, uint32_t site,
                                                  uint32_t* __restrict__ bits) {
    const int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (idx >= (int64_t)n * W) return;
    const int i = (int)(idx / W), w = (int)(idx % W);
    const uint64_t st = (uint64_t)step[0];
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const int j = 32 * w + b;
        if (j >= n) break;
        bool drop, add = true;
        if (j != i) {
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            manip_draw(seed, st, site, (uint64_t)hi * (uint64_t)n + (uint64_t)lo, p_drop, p_add, drop, add);
        }
        word |= (add ? 1u : 0u) << b;
    }
    bits[idx] = word;
}

// the label CSR's lower triangle: an edge survives when its count minus the drop draw stays positive
__global__ void __launch_bounds__(TB) k_manip_edges(const int32_t* __restrict__ rp, const int32_t* __restrict__ ci,
                                                    const float* __restrict__ cnt, int n, int W, float p_drop,
                                                    float p_add, uint64_t seed, const int64_t* __restrict__ step,
                                                    uint32_t site, uint32_t* __restrict__ bits) {
    const int i = blockIdx.x * TB + threadIdx.x;
    if (i >= n) return;
    const uint64_t st = (uint64_t)step[0];
    for (int e = rp[i]; e < rp[i + 1]; ++e) {
        const int j = ci[e];
        if (j >= i || j < 0) continue;
        bool drop, add;
        manip_draw(seed, st, site, (uint64_t)i * (uint64_t)n + (uint64_t)j, p_drop, p_add, drop, add);
        if (cnt[e] - (drop ? 1.f : 0.f) > 0.f) {
            atomicOr(bits + (int64_t)i * W + (j >> 5), 1u << (j & 31));
            atomicOr(bits + (int64_t)j * W + (i >> 5), 1u << (i & 31));
        }
    }
}

__global__ void __launch_bounds__(TB) k_pack_dense(const float* __restrict__ a, int64_t ld, int n, int W,
                                                   uint32_t* __restrict__ bits) {
    const int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (idx >= (int64_t)n * W) return;
    const int i = (int)(idx / W), w = (int)(idx % W);
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
        const int j = 32 * w + b;
        if (j >= n) break;
        word |= (j == i || a[(int64_t)i * ld + j] > 0.f ? 1u : 0u) << b;
    }
    bits[idx] = word;
}

// one wave per row
__global__ void __launch_bounds__(TB) k_bits_rows(const uint32_t* __restrict__ bits, int n, int W,
                                                  float* __restrict__ deg, float* __restrict__ dis,
                                                  int32_t* __restrict__ rowcnt) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popc(bits[(int64_t)i * W + w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (lane == 0) {
        const float d = (float)(c + 1);
        deg[i] = d;
        dis[i] = 1.f / sqrtf(d);
        rowcnt[i] = c;
    }
}

__global__ void __launch_bounds__(TB) k_bits_final(const int32_t* __restrict__ rowcnt, int n,
                                                   float* __restrict__ scal) {
    __shared__ long long red[TB];
    long long s = 0;
    for (int k = threadIdx.x; k < n; k += TB) s += rowcnt[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = TB / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double lab = (double)(red[0] + n), tot = (double)n * (double)n;
        scal[0] = (float)lab;
        scal[1] = (float)((tot - lab) / lab);
        scal[2] = (float)(tot / (2.0 * (tot - lab)));
        scal[3] = 0.f;
    }
}

// -------------------------------------------------------------------------------------------------- bit GEMM --
__global__ void __launch_bounds__(TB) k_bitadj_gemm(const uint32_t* __restrict__ bits, int n, int W,
                                                    const float* __restrict__ dis, const float* __restrict__ H,
                                                    int64_t ldh, int C, const float* __restrict__ bias,
                                                    float* __restrict__ out, int64_t ldo) {
    __shared__ __attribute__((aligned(16))) __bf16 img[3][GN][GLD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, g = lane >> 4;          // operand maps: index lr, k = 8 g .. 8 g + 7
    const int i0 = blockIdx.x * GM + wave * 32;
    const int c0 = blockIdx.y * GN;
    f32x4 acc[2][4];
#pragma unroll
    for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int cs = 0; cs < 4; ++cs)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[ms][cs][r] = 0.f;
    const int sc = tid & 63, sn = tid >> 6;           // staging role: column sc, nodes sn + 4 q
    const bool col_live = c0 + sc < C;
    for (int j0 = 0; j0 < n; j0 += GK) {
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < GK / 4; ++q) {
            const int node = sn + 4 * q, j = j0 + node;
            float v = 0.f;
            if (col_live && j < n) v = dis[j] * H[(int64_t)j * ldh + c0 + sc];
            const __bf16 hi = (__bf16)v;
            const float r1 = v - (float)hi;
            const __bf16 mid = (__bf16)r1;
            const __bf16 lo = (__bf16)(r1 - (float)mid);
            img[0][sc][node] = hi;
            img[1][sc][node] = mid;
            img[2][sc][node] = lo;
        }
        __syncthreads();
#pragma unroll
        for (int kw = 0; kw < GK / 32; ++kw) {
            const int w = (j0 >> 5) + kw;
            if (w >= W) break;
            bf8 a[2];
#pragma unroll
            for (int ms = 0; ms < 2; ++ms) {
                const int row = i0 + 16 * ms + lr;
                const uint32_t word = row < n ? bits[(int64_t)row * W + w] : 0u;
                const uint32_t byte = (word >> (8 * g)) & 0xffu;
                union { uint32_t u[4]; bf8 v; } x;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    x.u[e] = ((byte >> (2 * e)) & 1u) * 0x3F80u | ((byte >> (2 * e + 1)) & 1u) * 0x3F800000u;
                a[ms] = x.v;
            }
#pragma unroll
            for (int cs = 0; cs < 4; ++cs)
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const bf8 b = *reinterpret_cast<const bf8*>(&img[2 - t][cs * 16 + lr][kw * 32 + 8 * g]);
#pragma unroll
                    for (int ms = 0; ms < 2; ++ms)
                        acc[ms][cs] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ms], b, acc[ms][cs], 0, 0, 0);
                }
        }
    }
    // D layout: column lane & 15 = output column, rows 4 g + r = output rows
#pragma unroll
    for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + 16 * ms + 4 * g + r;
            if (row >= n) continue;
            const float di = dis[row];
#pragma unroll
            for (int cs = 0; cs < 4; ++cs) {
                const int col = c0 + cs * 16 + lr;
                if (col >= C) continue;
                const float self = di * H[(int64_t)row * ldh + col];      // the diagonal's second unit
                out[(int64_t)row * ldo + col] = di * (acc[ms][cs][r] + self) + (bias ? bias[col] : 0.f);
            }
        }
}

// ---------------------------------------------------------------------------------------- reconstruction --
__global__ void __launch_bounds__(TB) k_rb_fold(const float* __restrict__ part, int n, int K, int chunks,
                                                const float* __restrict__ scal, float* __restrict__ dz,
                                                int64_t lddz) {
    const int64_t idx = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (idx >= (int64_t)n * K) return;
    const int64_t i = idx / K;
    const int k = (int)(idx % K);
    float d = 0.f;
    for (int ch = 0; ch < chunks; ++ch) d += part[((int64_t)ch * n + i) * K + k];
    const float c = (float)((double)scal[2] / ((double)n * (double)n));
    dz[i * lddz + k] = 2.f * c * d;
}

// ------------------------------------------------------------------------------------------------- walks --
__global__ void __launch_bounds__(TB) k_walks(const int64_t* __restrict__ rp, const int64_t* __restrict__ ci,
                                              const int64_t* __restrict__ start, int64_t nw, int len, uint64_t seed,
                                              const int64_t* __restrict__ step, uint32_t site,
                                              int64_t* __restrict__ out) {
    const int64_t wk = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (wk >= nw) return;
    const uint64_t st = (uint64_t)step[0];
    int64_t cur = start[wk];
    out[wk * (len + 1)] = cur;
    for (int s = 1; s <= len; ++s) {
        const int64_t b = rp[cur], d = rp[cur + 1] - b;
        if (d > 0) {
            uint32_t r[4];
            GdaPhilox::gen(seed, ((uint64_t)site << 32) ^ (st * 0x9E3779B97F4A7C15ull), (uint64_t)(wk * len + s - 1), r);
            cur = ci[b + (int64_t)(((uint64_t)r[0] * (uint64_t)d) >> 32)];
        }
        out[wk * (len + 1) + s] = cur;
    }
}

unsigned elem_grid(int64_t n) { return (unsigned)gda_cdiv(n < 1 ? 1 : n, TB); }

int finish_bits(const uint32_t* bits, int n, int W, float* deg, float* dis, float* scal, void* workspace,
                hipStream_t s) {
    int32_t* rowcnt = static_cast<int32_t*>(workspace);
    k_bits_rows<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, s>>>(bits, n, W, deg, dis, rowcnt);
    GDA_LAUNCH_CHECK();
    k_bits_final<<<1, TB, 0, s>>>(rowcnt, n, scal);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

}  // namespace

extern "C" size_t gda_dgda_bits_workspace_bytes(int64_t n) { return n < 64 ? 256 : (size_t)n * sizeof(int32_t); }

extern "C" int gda_dgda_manip_bits(const int32_t* rowptr, const int32_t* col, const float* cnt, int64_t n, float p_drop,
                                   float p_add, uint64_t seed, const int64_t* step, uint32_t site, uint32_t* bits,
                                   float* deg, float* dis, float* scal, void* workspace, size_t workspace_bytes,
                                   gda_stream_t stream) {
    if (n < 1 || n > GDA_DGDA_MAX_N || !(p_drop >= 0.f && p_drop <= 1.f) || !(p_add >= 0.f && p_add <= 1.f))
        return GDA_E_SIZE;
    if (!rowptr || !col || !cnt || !step || !bits || !deg || !dis || !scal || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_dgda_bits_workspace_bytes(n)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int ni = (int)n, W = (int)gda_cdiv(n, 32);
    k_manip_add<<<elem_grid(n * W), TB, 0, s>>>(ni, W, p_drop, p_add, seed, step, site, bits);
    GDA_LAUNCH_CHECK();
    k_manip_edges<<<elem_grid(n), TB, 0, s>>>(rowptr, col, cnt, ni, W, p_drop, p_add, seed, step, site, bits);
    GDA_LAUNCH_CHECK();
    return finish_bits(bits, ni, W, deg, dis, scal, workspace, s);
}

extern "C" int gda_dgda_pack_bits_f32(const float* adj, int64_t ld, int64_t n, uint32_t* bits, float* deg, float* dis,
                                      float* scal, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n > GDA_DGDA_MAX_N || ld < n) return GDA_E_SIZE;
    if (!adj || !bits || !deg || !dis || !scal || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_dgda_bits_workspace_bytes(n)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int ni = (int)n, W = (int)gda_cdiv(n, 32);
    k_pack_dense<<<elem_grid(n * W), TB, 0, s>>>(adj, ld, ni, W, bits);
    GDA_LAUNCH_CHECK();
    return finish_bits(bits, ni, W, deg, dis, scal, workspace, s);
}

extern "C" int gda_dgda_bitadj_gemm_f32(const uint32_t* bits, int64_t n, const float* dis, const float* h, int64_t ldh,
                                        int64_t c, const float* bias, float* out, int64_t ldo, gda_stream_t stream) {
    if (n < 1 || n > GDA_DGDA_MAX_N || c < 1 || c > GDA_DGDA_MAX_C || ldh < c || ldo < c) return GDA_E_SIZE;
    if (!bits || !dis || !h || !out) return GDA_E_NULL;
    if (out == h) return GDA_E_ALIAS;
    const dim3 grid((unsigned)gda_cdiv(n, GM), (unsigned)gda_cdiv(c, GN));
    k_bitadj_gemm<<<grid, TB, 0, (hipStream_t)stream>>>(bits, (int)n, (int)gda_cdiv(n, 32), dis, h, ldh, (int)c, bias,
                                                        out, ldo);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_dgda_recon_bits_workspace_bytes(int64_t n, int64_t k) {
    if (n < 1 || k < 1) return 256;
    const int64_t ch = gda_recon::chunks(n);
    return (size_t)(ch * n * k + ch * gda_cdiv(n, RT_I)) * sizeof(float);
}

extern "C" int gda_dgda_recon_bits_f32(const float* z, int64_t ldz, int64_t n, int64_t k, const uint32_t* bits,
                                       const float* scal, float* loss, float* dz, int64_t lddz, void* workspace,
                                       size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n > GDA_DGDA_MAX_N || k < 1 || ldz < k || lddz < k) return GDA_E_SIZE;
    if (k > GDA_ASN_MAX_K) return GDA_E_UNSUPPORTED;
    if (!z || !bits || !scal || !loss || !dz || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_dgda_recon_bits_workspace_bytes(n, k)) return GDA_E_WORKSPACE;
    if (dz == z) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    const int ni = (int)n, ki = (int)k, W = (int)gda_cdiv(n, 32);
    const int ch = gda_recon::chunks(n);
    const int rb = (int)gda_cdiv(n, RT_I);
    float* part = static_cast<float*>(workspace);
    float* lpart = part + (int64_t)ch * n * k;
    const int rc = gda_recon::launch_pairs(z, ldz, ni, ki, gda_recon::BitLabels{W, bits, scal}, part, lpart, s);
    if (rc != GDA_OK) return rc;
    k_rb_fold<<<elem_grid(n * k), TB, 0, s>>>(part, ni, ki, ch, scal, dz, lddz);
    GDA_LAUNCH_CHECK();
    gda_recon::k_recon_final<<<1, TB, 0, s>>>(lpart, ch * rb, nullptr, 0, 0.f, scal + 2, ni, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_dgda_walks(const int64_t* rowptr, const int64_t* col, int64_t n, const int64_t* start, int64_t nwalks,
                              int64_t length, uint64_t seed, const int64_t* step, uint32_t site, int64_t* out,
                              gda_stream_t stream) {
    if (n < 1 || nwalks < 0 || length < 0 || length > (1 << 20)) return GDA_E_SIZE;
    if (nwalks == 0) return GDA_OK;
    if (!rowptr || !col || !start || !step || !out) return GDA_E_NULL;
    k_walks<<<elem_grid(nwalks), TB, 0, (hipStream_t)stream>>>(rowptr, col, start, nwalks, (int)length, seed, step, site,
                                                               out);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
