// ASN for gfx950 (pygda/models/asn.py, pygda/nn/asn_base.py): the all-pairs graph reconstruction loss, the small row
// kernels of the VAE encoders and the normalised PPMI graph of the global encoders.
//
// Reconstruction (recon_loss's cost term): loss = c * sum_ij f(x_ij, y_ij), x = z z^T, c = norm / N^2, f torch's stable
// pos_weight-ed BCE-with-logits  f = (1 - y) x + (1 + (pw - 1) y) (log1p(exp(-|x|)) + max(-x, 0)).
// Every pair takes the y = 0 term f_0(x) = softplus(x) with f_0' = sigmoid(x); the label CSR (A + I, counts) adds
// f_y - f_0 = -y x + (pw - 1) y softplus(-x) and its derivative -y - (pw - 1) y sigmoid(-x).  dZ = c (G + G^T) Z; the
// dense part of G is symmetric, so it contributes 2 c G_0 Z, and the sparse part walks the label CSR and its transpose.
//   gda_recon::k_recon_pairs<KP, NoLabels>  the pair pass of gda_recon.h without labels: per chunk of the columns the
//                      blocks' softplus sums and their [32, K] slabs of sigmoid(x) Z go to the caller's workspace.
//   k_recon_fold       one wave per row: the chunks' slabs summed in chunk order (x 2c), then the label row and the
//                      transposed label row in CSR order (x recomputed by a butterfly dot), dZ written, the row's loss
//                      correction to the workspace.
//   gda_recon::k_recon_final  one block: block sums and row corrections in a fixed strided order (double), times c.
// Row kernels:
//   k_kld              -0.5 / n_nodes * mean_i sum_k (1 + 2 lv - mu^2 - exp(lv)^2) over [N, D]: row-slab partials,
//                      folded by gda_reduce.h's k_fold_scalar; the gradients (mu / (n N), -(1 - exp(2 lv)) / (n N)) in
//                      the same pass.
//   k_reparam_fwd/bwd  z = eps exp(lv) + mu, eps standard normal from Philox (Box-Muller) or given; d lv = g eps exp(lv).
//   k_dropout_fwd      y = x * m, m in {0, 1 / (1 - p)} from Philox, m kept for the backward (k_mask_mul).
//   k_diff_*           DiffLoss: rows scaled by 1 / (|row| + 1e-6) (the norm is a constant for the gradient), the
//                      K1 x K2 Gram An^T Bn as row-slab partials folded in slab order, mean(M^2), then per row
//                      dA = (2 / (K1 K2)) Bn M^T / (|A_i| + 1e-6) and dB = (2 / (K1 K2)) An M / (|B_i| + 1e-6).
// PPMI graph (GCNConv on the row-scaled PPMI as a sparse adjacency, PyG's torch-sparse gcn_norm branch):
//   k_pg_count / k_pg_fill / k_pg_norm  count the non-zeros of each dense row plus the diagonal, fill the COO in
//                      row-major order (block scan, columns ascending) with the self loop summed into the diagonal and
//                      the row sum as the degree, then value = deg^-1/2[j] v deg^-1/2[i].
// Every reduction has a fixed order that depends on the shapes only: two runs are bit-identical.  No atomics.
#include "gda_common.h"
#include "gda_philox.h"
#include "gda_recon.h"
#include "gda_reduce.h"

namespace {

using gda_recon::RT_I;
using gda_recon::TB;
constexpr int SLAB = 256;                   // row kernels: rows per block
constexpr int DIFF_MAXK = 32;               // DiffLoss: widths up to 32 (Gram of at most 1024 entries)

__device__ __forceinline__ float softplus_f(float x) {      // log1p(exp(-|x|)) + max(x, 0)
    return log1pf(expf(-fabsf(x))) + fmaxf(x, 0.f);
}

__device__ __forceinline__ float sigmoid_f(float x) {
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e);
    return x >= 0.f ? r : e * r;
}

// ------------------------------------------------------------------------------------------ reconstruction --
// one wave per row; lanes hold columns k = lane and lane + 64
__global__ void __launch_bounds__(TB) k_recon_fold(const float* __restrict__ z, int64_t ldz, int n, int K, int chunks,
                                                   const float* __restrict__ part, const int32_t* __restrict__ rp,
                                                   const int32_t* __restrict__ ci, const float* __restrict__ lv,
                                                   const int32_t* __restrict__ trp, const int32_t* __restrict__ tci,
                                                   const float* __restrict__ tlv, float c, float pw,
                                                   float* __restrict__ dz, int64_t lddz, float* __restrict__ rowloss) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (TB / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    const int k0 = lane, k1 = lane + 64;
    const float zi0 = k0 < K ? z[(int64_t)i * ldz + k0] : 0.f;
    const float zi1 = k1 < K ? z[(int64_t)i * ldz + k1] : 0.f;
    float d0 = 0.f, d1 = 0.f;
    for (int ch = 0; ch < chunks; ++ch) {
        const float* p = part + ((int64_t)ch * n + i) * K;
        if (k0 < K) d0 += p[k0];
        if (k1 < K) d1 += p[k1];
    }
    d0 *= 2.f * c;
    d1 *= 2.f * c;
    float lcorr = 0.f;
    const float pm1 = pw - 1.f;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t* r = pass ? trp : rp;
        const int32_t* col = pass ? tci : ci;
        const float* val = pass ? tlv : lv;
        for (int e = r[i]; e < r[i + 1]; ++e) {
            const int j = col[e];
            const float y = val[e];
            const float zj0 = k0 < K ? z[(int64_t)j * ldz + k0] : 0.f;
            const float zj1 = k1 < K ? z[(int64_t)j * ldz + k1] : 0.f;
            const float x = wave_sum(fmaf(zi1, zj1, zi0 * zj0));
            const float g1 = -y - pm1 * y * sigmoid_f(-x);
            if (pass == 0) lcorr += -y * x + pm1 * y * softplus_f(-x);
            d0 = fmaf(c * g1, zj0, d0);
            d1 = fmaf(c * g1, zj1, d1);
        }
    }
    if (k0 < K) dz[(int64_t)i * lddz + k0] = d0;
    if (k1 < K) dz[(int64_t)i * lddz + k1] = d1;
    if (lane == 0) rowloss[i] = lcorr;
}

// ------------------------------------------------------------------------------------------ row kernels --
// KLD over [N, D] (mu, lv row-major with their own leading dimensions); the row-slab partial of sum_k (...)
__global__ void __launch_bounds__(TB) k_kld(const float* __restrict__ mu, int64_t ldm, const float* __restrict__ lv,
                                            int64_t ldl, int n, int D, float gscale, float* __restrict__ gmu,
                                            float* __restrict__ glv, float* __restrict__ part) {
    __shared__ float red[TB];
    const int64_t b = (int64_t)blockIdx.x * SLAB;
    float s = 0.f;
    const int64_t cnt = min((int64_t)SLAB, (int64_t)n - b) * D;
    for (int64_t idx = threadIdx.x; idx < cnt; idx += TB) {
        const int64_t i = b + idx / D;
        const int k = (int)(idx % D);
        const float m = mu[i * ldm + k], l = lv[i * ldl + k];
        const float el = expf(l);
        s += 1.f + 2.f * l - m * m - el * el;
        gmu[i * D + k] = gscale * m;
        glv[i * D + k] = -gscale * (1.f - el * el);
    }
    const float bs = block_sum_f(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = bs;
}

__device__ __forceinline__ float philox_normal(uint64_t seed, uint64_t step, uint32_t site, int64_t idx) {
    uint32_t r[4];
    GdaPhilox::gen(seed, ((uint64_t)site << 32) ^ (step * 0x9E3779B97F4A7C15ull), (uint64_t)idx, r);
    const float u1 = ((float)(r[0] >> 8) + 1.f) * (1.f / 16777216.f);      // (0, 1]
    const float u2 = (float)(r[1] >> 8) * (1.f / 16777216.f);
    return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__global__ void k_reparam_fwd(const float* __restrict__ mu, int64_t ldm, const float* __restrict__ lv, int64_t ldl,
                              int n, int D, float* __restrict__ eps, int draw, uint64_t seed,
                              const int64_t* __restrict__ step, uint32_t site, float* __restrict__ z) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n * D) return;
    const int64_t i = idx / D;
    const int k = (int)(idx % D);
    const float e = draw ? philox_normal(seed, (uint64_t)step[0], site, idx) : eps[idx];
    if (draw) eps[idx] = e;
    z[idx] = e * expf(lv[i * ldl + k]) + mu[i * ldm + k];
}

__global__ void k_reparam_bwd(const float* __restrict__ g, const float* __restrict__ eps, const float* __restrict__ lv,
                              int64_t ldl, int n, int D, float* __restrict__ glv) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)n * D) return;
    const int64_t i = idx / D;
    const int k = (int)(idx % D);
    glv[idx] = g[idx] * eps[idx] * expf(lv[i * ldl + k]);
}

__global__ void k_dropout_fwd(const float* __restrict__ x, int64_t n, float p, uint64_t seed,
                              const int64_t* __restrict__ step, uint32_t site, float* __restrict__ m,
                              float* __restrict__ y) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    uint32_t r[4];
    GdaPhilox::gen(seed, ((uint64_t)site << 32) ^ ((uint64_t)step[0] * 0xD1B54A32D192ED03ull), (uint64_t)idx, r);
    const float u = (float)(r[0] >> 8) * (1.f / 16777216.f);
    const float keep = u >= p ? 1.f / (1.f - p) : 0.f;
    m[idx] = keep;
    y[idx] = x[idx] * keep;
}

__global__ void k_mask_mul(const float* __restrict__ g, const float* __restrict__ m, int64_t n, float* __restrict__ gx) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) gx[idx] = g[idx] * m[idx];
}

// DiffLoss: Gram partials of one row slab, entries (a, b) of An^T Bn; the slab's scaled rows staged in LDS
__global__ void __launch_bounds__(TB) k_diff_gram(const float* __restrict__ A, int64_t lda, const float* __restrict__ B,
                                                  int64_t ldb, int n, int K1, int K2, float* __restrict__ part) {
    __shared__ float an[64][DIFF_MAXK + 1];
    __shared__ float bn[64][DIFF_MAXK + 1];
    const int KK = K1 * K2;
    float acc[DIFF_MAXK * DIFF_MAXK / TB];
#pragma unroll
    for (int q = 0; q < DIFF_MAXK * DIFF_MAXK / TB; ++q) acc[q] = 0.f;
    const int64_t b0 = (int64_t)blockIdx.x * SLAB;
    const int64_t b1 = min(b0 + SLAB, (int64_t)n);
    for (int64_t r0 = b0; r0 < b1; r0 += 64) {
        __syncthreads();
        if (threadIdx.x < 64) {                    // one lane per row: the norms in column order
            const int64_t i = r0 + threadIdx.x;
            if (i < b1) {
                float sa = 0.f, sb = 0.f;
                for (int k = 0; k < K1; ++k) sa = fmaf(A[i * lda + k], A[i * lda + k], sa);
                for (int k = 0; k < K2; ++k) sb = fmaf(B[i * ldb + k], B[i * ldb + k], sb);
                const float ia = 1.f / (sqrtf(sa) + 1e-6f), ib = 1.f / (sqrtf(sb) + 1e-6f);
                for (int k = 0; k < K1; ++k) an[threadIdx.x][k] = A[i * lda + k] * ia;
                for (int k = 0; k < K2; ++k) bn[threadIdx.x][k] = B[i * ldb + k] * ib;
            } else {
                for (int k = 0; k < K1; ++k) an[threadIdx.x][k] = 0.f;
                for (int k = 0; k < K2; ++k) bn[threadIdx.x][k] = 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < DIFF_MAXK * DIFF_MAXK / TB; ++q) {
            const int e = threadIdx.x + q * TB;
            if (e < KK) {
                const int a = e / K2, bb = e % K2;
                float s = acc[q];
                for (int r = 0; r < 64; ++r) s = fmaf(an[r][a], bn[r][bb], s);
                acc[q] = s;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < DIFF_MAXK * DIFF_MAXK / TB; ++q) {
        const int e = threadIdx.x + q * TB;
        if (e < KK) part[(int64_t)blockIdx.x * KK + e] = acc[q];
    }
}

// the slabs folded in order into M [K1, K2], and mean(M^2) (one block)
__global__ void __launch_bounds__(TB) k_diff_fold(const float* __restrict__ part, int slabs, int KK,
                                                  float* __restrict__ M, float* __restrict__ loss) {
    __shared__ double red[TB];
    double s = 0.0;
    for (int e = threadIdx.x; e < KK; e += TB) {
        float m = 0.f;
        for (int b = 0; b < slabs; ++b) m += part[(int64_t)b * KK + e];
        M[e] = m;
        s += (double)m * (double)m;
    }
    const double tot = block_sum_d(s, red);
    if (threadIdx.x == 0) loss[0] = (float)(tot / (double)KK);
}

// per row: dA_i = (2 / KK) (Bn_i M^T) / (|A_i| + 1e-6), dB_i = (2 / KK) (An_i M) / (|B_i| + 1e-6)
__global__ void k_diff_bwd(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb, int n,
                           int K1, int K2, const float* __restrict__ M, const float* __restrict__ gl,
                           float* __restrict__ gA, float* __restrict__ gB) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float sa = 0.f, sb = 0.f;
    for (int k = 0; k < K1; ++k) sa = fmaf(A[i * lda + k], A[i * lda + k], sa);
    for (int k = 0; k < K2; ++k) sb = fmaf(B[i * ldb + k], B[i * ldb + k], sb);
    const float ia = 1.f / (sqrtf(sa) + 1e-6f), ib = 1.f / (sqrtf(sb) + 1e-6f);
    const float s = 2.f * gl[0] / (float)(K1 * K2);
    for (int a = 0; a < K1; ++a) {
        float v = 0.f;
        for (int b = 0; b < K2; ++b) v = fmaf(B[i * ldb + b] * ib, M[a * K2 + b], v);
        gA[i * K1 + a] = s * v * ia;
    }
    for (int b = 0; b < K2; ++b) {
        float v = 0.f;
        for (int a = 0; a < K1; ++a) v = fmaf(A[i * lda + a] * ia, M[a * K2 + b], v);
        gB[i * K2 + b] = s * v * ib;
    }
}

// ------------------------------------------------------------------------------------------ PPMI graph --
__device__ __forceinline__ bool pg_entry(const float* row, int i, int j) { return row[j] != 0.f || j == i; }

__global__ void __launch_bounds__(TB) k_pg_count(const float* __restrict__ na, int n, int64_t ld,
                                                 int64_t* __restrict__ cnt) {
    __shared__ float red[TB];
    const int i = blockIdx.x;
    const float* row = na + (int64_t)i * ld;
    float c = 0.f;                                   // exact: at most 2^24 entries per row (n < 2^24)
    for (int j = threadIdx.x; j < n; j += TB) c += pg_entry(row, i, j) ? 1.f : 0.f;
    const float tot = block_sum_f(c, red);
    if (threadIdx.x == 0) cnt[i] = (int64_t)tot;
}

__global__ void __launch_bounds__(TB) k_pg_fill(const float* __restrict__ na, int n, int64_t ld,
                                                const int64_t* __restrict__ rowptr, int64_t* __restrict__ row_out,
                                                int64_t* __restrict__ col_out, float* __restrict__ val,
                                                float* __restrict__ dis) {
    __shared__ int scan[TB];
    __shared__ float red[TB];
    const int i = blockIdx.x;
    const int t = threadIdx.x;
    const float* row = na + (int64_t)i * ld;
    int64_t base = rowptr[i];
    float deg = 0.f;
    for (int j0 = 0; j0 < n; j0 += TB) {
        const int j = j0 + t;
        const bool f = j < n && pg_entry(row, i, j);
        const float v = f ? row[j] + (j == i ? 1.f : 0.f) : 0.f;
        deg += v;
        scan[t] = f ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < TB; o <<= 1) {           // inclusive Hillis-Steele scan
            const int add = t >= o ? scan[t - o] : 0;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        if (f) {
            const int64_t pos = base + scan[t] - 1;
            row_out[pos] = i;
            col_out[pos] = j;
            val[pos] = v;
        }
        base += scan[TB - 1];
        __syncthreads();
    }
    const float d = block_sum_f(deg, red);
    if (t == 0) dis[i] = d > 0.f ? 1.f / sqrtf(d) : 0.f;
}

__global__ void k_pg_norm(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t nnz,
                          const float* __restrict__ dis, float* __restrict__ val) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) val[e] = dis[col[e]] * val[e] * dis[row[e]];
}

unsigned elem_grid(int64_t n) { return (unsigned)gda_cdiv(n < 1 ? 1 : n, TB); }

}  // namespace

extern "C" int gda_asn_recon_chunks(int64_t n) { return n < 1 ? 0 : gda_recon::chunks(n); }

extern "C" size_t gda_asn_recon_workspace_bytes(int64_t n, int64_t k) {
    if (n < 1 || k < 1) return 256;
    const int64_t ch = gda_recon::chunks(n);
    const int64_t floats = ch * n * k + ch * gda_cdiv(n, RT_I) + n;
    return (size_t)floats * sizeof(float);
}

extern "C" int gda_asn_recon_f32(const float* z, int64_t ldz, int64_t n, int64_t k, const int32_t* rowptr,
                                 const int32_t* col, const float* lab, const int32_t* t_rowptr, const int32_t* t_col,
                                 const float* t_lab, float norm, float pos_weight, float* loss, float* dz, int64_t lddz,
                                 void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n >= (1 << 24) || k < 1 || ldz < k || lddz < k) return GDA_E_SIZE;
    if (k > GDA_ASN_MAX_K) return GDA_E_UNSUPPORTED;
    if (!z || !rowptr || !col || !lab || !t_rowptr || !t_col || !t_lab || !loss || !dz || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_asn_recon_workspace_bytes(n, k)) return GDA_E_WORKSPACE;
    if (dz == z) return GDA_E_ALIAS;
    hipStream_t s = (hipStream_t)stream;
    const int ni = (int)n, ki = (int)k;
    const int ch = gda_recon::chunks(n);
    const int rb = (int)gda_cdiv(n, RT_I);
    float* part = static_cast<float*>(workspace);
    float* lpart = part + (int64_t)ch * n * k;
    float* rowloss = lpart + (int64_t)ch * rb;
    const float c = (float)((double)norm / ((double)n * (double)n));
    const int rc = gda_recon::launch_pairs(z, ldz, ni, ki, gda_recon::NoLabels{}, part, lpart, s);
    if (rc != GDA_OK) return rc;
    k_recon_fold<<<(unsigned)gda_cdiv(n, TB / 64), TB, 0, s>>>(z, ldz, ni, ki, ch, part, rowptr, col, lab, t_rowptr,
                                                               t_col, t_lab, c, pos_weight, dz, lddz, rowloss);
    GDA_LAUNCH_CHECK();
    gda_recon::k_recon_final<<<1, TB, 0, s>>>(lpart, ch * rb, rowloss, ni, c, nullptr, ni, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_asn_rows_workspace_bytes(int64_t n, int64_t k1, int64_t k2) {
    const int64_t slabs = gda_cdiv(n < 1 ? 1 : n, SLAB);
    return (size_t)(slabs * (k1 * k2 > 1 ? k1 * k2 : 1) + k1 * k2 + 64) * sizeof(float);
}

extern "C" int gda_asn_kld_f32(const float* mu, int64_t ldm, const float* lv, int64_t ldl, int64_t n, int64_t d,
                               double n_nodes, float* loss, float* gmu, float* glv, void* workspace,
                               size_t workspace_bytes, gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || d < 1 || ldm < d || ldl < d || !(n_nodes > 0.0)) return GDA_E_SIZE;
    if (!mu || !lv || !loss || !gmu || !glv || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_asn_rows_workspace_bytes(n, 1, 1)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int slabs = (int)gda_cdiv(n, SLAB);
    float* part = static_cast<float*>(workspace);
    const double scale = -0.5 / n_nodes / (double)n;
    k_kld<<<(unsigned)slabs, TB, 0, s>>>(mu, ldm, lv, ldl, (int)n, (int)d, (float)(1.0 / (n_nodes * (double)n)), gmu,
                                         glv, part);
    GDA_LAUNCH_CHECK();
    k_fold_scalar<TB><<<1, TB, 0, s>>>(part, slabs, scale, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_reparam_fwd_f32(const float* mu, int64_t ldm, const float* lv, int64_t ldl, int64_t n,
                                       int64_t d, float* eps, int draw, uint64_t seed, const int64_t* step,
                                       uint32_t site, float* z, gda_stream_t stream) {
    if (n < 0 || d < 1 || ldm < d || ldl < d) return GDA_E_SIZE;
    if (n == 0) return GDA_OK;
    if (!mu || !lv || !eps || !z || (draw && !step)) return GDA_E_NULL;
    k_reparam_fwd<<<elem_grid(n * d), TB, 0, (hipStream_t)stream>>>(mu, ldm, lv, ldl, (int)n, (int)d, eps, draw, seed,
                                                                     step, site, z);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_reparam_bwd_f32(const float* g, const float* eps, const float* lv, int64_t ldl, int64_t n,
                                       int64_t d, float* glv, gda_stream_t stream) {
    if (n < 0 || d < 1 || ldl < d) return GDA_E_SIZE;
    if (n == 0) return GDA_OK;
    if (!g || !eps || !lv || !glv) return GDA_E_NULL;
    k_reparam_bwd<<<elem_grid(n * d), TB, 0, (hipStream_t)stream>>>(g, eps, lv, ldl, (int)n, (int)d, glv);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_dropout_fwd_f32(const float* x, int64_t n, float p, uint64_t seed, const int64_t* step,
                                       uint32_t site, float* mask, float* y, gda_stream_t stream) {
    if (n < 0 || !(p >= 0.f && p < 1.f)) return GDA_E_SIZE;
    if (n == 0) return GDA_OK;
    if (!x || !step || !mask || !y) return GDA_E_NULL;
    k_dropout_fwd<<<elem_grid(n), TB, 0, (hipStream_t)stream>>>(x, n, p, seed, step, site, mask, y);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_mask_mul_f32(const float* g, const float* mask, int64_t n, float* gx, gda_stream_t stream) {
    if (n < 0) return GDA_E_SIZE;
    if (n == 0) return GDA_OK;
    if (!g || !mask || !gx) return GDA_E_NULL;
    k_mask_mul<<<elem_grid(n), TB, 0, (hipStream_t)stream>>>(g, mask, n, gx);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_diff_fwd_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int64_t k1,
                                    int64_t k2, float* loss, float* gram, void* workspace, size_t workspace_bytes,
                                    gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || k1 < 1 || k2 < 1 || lda < k1 || ldb < k2) return GDA_E_SIZE;
    if (k1 > DIFF_MAXK || k2 > DIFF_MAXK) return GDA_E_UNSUPPORTED;
    if (!a || !b || !loss || !gram || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_asn_rows_workspace_bytes(n, k1, k2)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int slabs = (int)gda_cdiv(n, SLAB);
    float* part = static_cast<float*>(workspace);
    k_diff_gram<<<(unsigned)slabs, TB, 0, s>>>(a, lda, b, ldb, (int)n, (int)k1, (int)k2, part);
    GDA_LAUNCH_CHECK();
    k_diff_fold<<<1, TB, 0, s>>>(part, slabs, (int)(k1 * k2), gram, loss);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_diff_bwd_f32(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int64_t k1,
                                    int64_t k2, const float* gram, const float* gl, float* ga, float* gb,
                                    gda_stream_t stream) {
    if (n < 1 || n >= INT32_MAX || k1 < 1 || k2 < 1 || lda < k1 || ldb < k2) return GDA_E_SIZE;
    if (k1 > DIFF_MAXK || k2 > DIFF_MAXK) return GDA_E_UNSUPPORTED;
    if (!a || !b || !gram || !gl || !ga || !gb) return GDA_E_NULL;
    k_diff_bwd<<<elem_grid(n), TB, 0, (hipStream_t)stream>>>(a, lda, b, ldb, (int)n, (int)k1, (int)k2, gram, gl, ga, gb);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_ppmi_count(const float* na, int64_t n, int64_t ld, int64_t* cnt, gda_stream_t stream) {
    if (n < 1 || n >= (1 << 24) || ld < n) return GDA_E_SIZE;
    if (!na || !cnt) return GDA_E_NULL;
    k_pg_count<<<(unsigned)n, TB, 0, (hipStream_t)stream>>>(na, (int)n, ld, cnt);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" int gda_asn_ppmi_fill(const float* na, int64_t n, int64_t ld, const int64_t* rowptr, int64_t nnz,
                                 int64_t* row, int64_t* col, float* val, float* dis, gda_stream_t stream) {
    if (n < 1 || n >= (1 << 24) || ld < n || nnz < n) return GDA_E_SIZE;
    if (!na || !rowptr || !row || !col || !val || !dis) return GDA_E_NULL;
    hipStream_t s = (hipStream_t)stream;
    k_pg_fill<<<(unsigned)n, TB, 0, s>>>(na, (int)n, ld, rowptr, row, col, val, dis);
    GDA_LAUNCH_CHECK();
    k_pg_norm<<<elem_grid(nnz), TB, 0, s>>>(row, col, nnz, dis, val);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
