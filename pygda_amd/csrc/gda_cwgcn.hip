// CWGCN's two losses for gfx950: the correntropy-induced loss with its sample weights, the weighted source moments
// and the unbiased column mean / std matching loss (pygda/nn/cwgcn_base.py:193-219; pygda/models/cwgcn.py:306-350,
// 423-458).
//
// All of them are column or row reductions over a few MB: memory / launch-latency bound.  The designs keep every
// lane's loads independent (a few in flight per lane) and the number of dependent launches small:
//   c_loss      k_closs_fwd: a group of G lanes per row (G = next power of two >= C, at most 64), the row distance
//               folded by a butterfly inside the group; per-block sums of the row losses -> k_sum_final (fixed order).
//               One launch when a single block covers the rows.
//   moments     k_colstat_partial: slab s x column tile; per (slab, column) the weight sum W, the weighted mean m and
//               M2 = sum w (x - m)^2 in two passes over the slab (the second pass hits the cache), per slab sum w^2.
//               k_colstat_final: per column, lane g of 32 merges slabs g, g + 32, ... (Chan's pairwise update), then a
//               fixed binary tree over the 32 lanes.
//   matching    the same two kernels with unit weights, k_colstat_final also forms the loss terms and the backward
//               coefficients per column; k_sum_final adds the terms in a fixed order.
// Every reduction order depends on (n, d) only: two runs are bit-identical.  No float atomics.  Labels are read only
// for rows < n and compared against the column index: a label outside [0, C) matches no column and is never used as an
// address.
#include "gda_common.h"

namespace {

constexpr int TB = 256;
constexpr int CL_MAX_BLOCKS = 1024;
constexpr int CS_TILE = 64;                 // columns per partial block (one wave reads 256 contiguous bytes of a row)
constexpr int CS_MAX_BLOCKS = 2048;
constexpr int CF_COLS = 8, CF_LANES = TB / CF_COLS;

int closs_lanes(int64_t c) {
    int g = 1;
    while (g < c && g < GDA_WAVE) g <<= 1;
    return g;
}

int closs_blocks(int64_t n, int64_t c) {
    const int64_t rpb = TB / closs_lanes(c);
    const int64_t b = gda_cdiv(n, rpb);
    return (int)(b > CL_MAX_BLOCKS ? CL_MAX_BLOCKS : (b < 1 ? 1 : b));
}

struct ColPlan {
    int ct, rows, tiles;
    int64_t rs, slabs;
};

ColPlan col_plan(int64_t n, int64_t d) {
    ColPlan p;
    p.ct = (int)(d < CS_TILE ? d : CS_TILE);
    p.rows = TB / p.ct;
    p.tiles = (int)gda_cdiv(d, p.ct);
    const int64_t cap = CS_MAX_BLOCKS / p.tiles > 1 ? CS_MAX_BLOCKS / p.tiles : 1;
    int64_t s = gda_cdiv(n, (int64_t)p.rows * 8);                       // >= 8 rows per lane and pass
    s = s > cap ? cap : (s < 1 ? 1 : s);
    p.rs = gda_cdiv(n, s);
    p.slabs = gda_cdiv(n, p.rs);
    return p;
}

// fixed binary tree over the first `count` entries of red[k * stride + lane] (count need not be a power of two)
__device__ __forceinline__ void tree_fold(float* red, int k, int count, int stride, int lane) {
    int w = 1;
    while (w < count) w <<= 1;
    for (w >>= 1; w > 0; w >>= 1) {
        if (k < w && k + w < count) red[k * stride + lane] += red[(k + w) * stride + lane];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TB)
k_closs_fwd(const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ y, int64_t n, int c, int G,
            float* __restrict__ weight, float* __restrict__ factor, float* __restrict__ partial, float* __restrict__ loss) {
    __shared__ float red[TB];
    const int lane = threadIdx.x % G, slot = threadIdx.x / G, rpb = TB / G;
    float acc = 0.f;
    for (int64_t base = (int64_t)blockIdx.x * rpb; base < n; base += (int64_t)gridDim.x * rpb) {   // block-uniform
        const int64_t row = base + slot;
        float dist = 0.f;
        if (row < n) {
            const int64_t lab = y[row];
            for (int col = lane; col < c; col += G) {
                const float diff = z[row * ldz + col] - (col == lab ? 1.f : 0.f);
                dist += diff * diff;
            }
        }
        for (int off = G / 2; off > 0; off >>= 1) dist += __shfl_xor(dist, off, GDA_WAVE);     // same sum in every lane
        if (row < n && lane == 0) {
            const float e = expf(-dist / 100.f);
            factor[row] = e;
            weight[row] = expf(-dist / 10.f);
            acc += 1.f - e;
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    tree_fold(red, threadIdx.x, TB, 1, 0);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) loss[0] = red[0] / (float)n;
        else partial[blockIdx.x] = red[0];
    }
}

// out[0] = scale_div ? (sum of v[0..count)) / div : sum, and, with count2 > 0, out[0] += sum of v2[0..count2) -- one
// block, lane t adds t, t + TB, ... in order, then a fixed tree
__global__ void __launch_bounds__(TB)
k_sum_final(const float* __restrict__ v, int64_t count, const float* __restrict__ v2, int64_t count2, float div,
            float* __restrict__ out) {
    __shared__ float red[2][TB];
    float a = 0.f, b = 0.f;
    for (int64_t i = threadIdx.x; i < count; i += TB) a += v[i];
    for (int64_t i = threadIdx.x; i < count2; i += TB) b += v2[i];
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int w = TB / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = count2 > 0 ? red[0][0] + red[1][0] : red[0][0] / div;
}

__global__ void __launch_bounds__(TB)
k_closs_bwd(const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ y, const float* __restrict__ factor,
            const float* __restrict__ gloss, int64_t n, int c, float* __restrict__ gz, int64_t ldgz) {
    const float k = gloss[0] / (50.f * (float)n);                      // g * 2 / (100 n)
    const int64_t total = n * c;
    for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < total; e += (int64_t)gridDim.x * TB) {
        const int64_t row = e / c;
        const int col = (int)(e - row * c);
        const float diff = z[row * ldz + col] - (col == y[row] ? 1.f : 0.f);
        gz[row * ldgz + col] = k * factor[row] * diff;
    }
}

// slab partials: pm[(s * d + col) * 2 + {0, 1}] = {m, M2}; ps[s * 2 + {0, 1}] = {W, sum w^2}
__global__ void __launch_bounds__(TB)
k_colstat_partial(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w, int64_t n, int d, int ct,
                  int64_t rs, float* __restrict__ pm, float* __restrict__ ps) {
    __shared__ float red[3][TB];
    __shared__ float mean[CS_TILE];
    const int rows = TB / ct, tc = threadIdx.x % ct, tr = threadIdx.x / ct;
    const int col = blockIdx.y * ct + tc;
    const bool live = tr < rows && col < d;
    const int64_t r0 = (int64_t)blockIdx.x * rs, r1 = r0 + rs < n ? r0 + rs : n;
    float sw = 0.f, swx = 0.f, sww = 0.f;
    if (live) {
        for (int64_t i = r0 + tr; i < r1; i += rows) {
            const float wi = w ? w[i] : 1.f;
            const float v = x[i * ldx + col];
            sw += wi;
            swx += wi * v;
            sww += wi * wi;
        }
    }
    const int slot = tr < rows ? tr : 0;
    if (tr < rows) {
        red[0][threadIdx.x] = sw;
        red[1][threadIdx.x] = swx;
        red[2][threadIdx.x] = sww;
    }
    __syncthreads();
    int wpow = 1;
    while (wpow < rows) wpow <<= 1;
    for (wpow >>= 1; wpow > 0; wpow >>= 1) {
        if (tr < rows && slot < wpow && slot + wpow < rows) {
            red[0][threadIdx.x] += red[0][threadIdx.x + wpow * ct];
            red[1][threadIdx.x] += red[1][threadIdx.x + wpow * ct];
            red[2][threadIdx.x] += red[2][threadIdx.x + wpow * ct];
        }
        __syncthreads();
    }
    const float W = red[0][tc];
    if (tr == 0) mean[tc] = W > 0.f ? red[1][tc] / W : 0.f;
    __syncthreads();
    const float m = mean[tc];
    float m2 = 0.f;
    if (live) {
        for (int64_t i = r0 + tr; i < r1; i += rows) {
            const float wi = w ? w[i] : 1.f;
            const float dv = x[i * ldx + col] - m;
            m2 += dv * dv * wi;
        }
    }
    __syncthreads();                                                      // everyone has read red[0][tc]
    if (tr < rows) red[1][threadIdx.x] = m2;
    __syncthreads();
    wpow = 1;
    while (wpow < rows) wpow <<= 1;
    for (wpow >>= 1; wpow > 0; wpow >>= 1) {
        if (tr < rows && slot < wpow && slot + wpow < rows) red[1][threadIdx.x] += red[1][threadIdx.x + wpow * ct];
        __syncthreads();
    }
    if (tr == 0 && col < d) {
        pm[((int64_t)blockIdx.x * d + col) * 2] = m;
        pm[((int64_t)blockIdx.x * d + col) * 2 + 1] = red[1][tc];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        ps[blockIdx.x * 2] = W;
        ps[blockIdx.x * 2 + 1] = red[2][0];
    }
}

struct Moments {
    float W, m, M, ww;
};

// Chan et al.'s pairwise update of (weight, mean, M2); sum w^2 adds
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
    if (b.W == 0.f) { a.ww += b.ww; return a; }
    if (a.W == 0.f) { b.ww += a.ww; return b; }
    Moments r;
    r.W = a.W + b.W;
    const float delta = b.m - a.m, f = b.W / r.W;
    r.m = a.m + delta * f;
    r.M = (a.M + b.M) + delta * delta * a.W * f;
    r.ww = a.ww + b.ww;
    return r;
}

// per column: the merged moments.  weighted (match == 0): out_a = mean, out_b = std = sqrt((M2 / W) / (1 - ww / W^2))
// (NaN where the denominator is 0).
// match: out_a = mean_t, out_b = std_t = sqrt(M2 / (n - 1)); terms[c] = (ms - mt)^2, terms[d + c] = (ss - st)^2;
// coef[c] = -2 (ms - mt) / n, coef[d + c] = -2 (ss - st) / ((n - 1) st), 0 where st == 0 (torch masks the std
// gradient there)
__global__ void __launch_bounds__(TB)
k_colstat_final(const float* __restrict__ pm, const float* __restrict__ ps, int64_t slabs, int d, int match,
                const float* __restrict__ mean_s, const float* __restrict__ std_s, float* __restrict__ out_a,
                float* __restrict__ out_b, float* __restrict__ terms, float* __restrict__ coef) {
    __shared__ float red[4][CF_LANES][CF_COLS];
    const int cl = threadIdx.x % CF_COLS, g = threadIdx.x / CF_COLS;
    const int col = blockIdx.x * CF_COLS + cl;
    Moments acc{0.f, 0.f, 0.f, 0.f};
    if (col < d) {
        for (int64_t s = g; s < slabs; s += CF_LANES) {
            Moments b{ps[s * 2], pm[(s * d + col) * 2], pm[(s * d + col) * 2 + 1], ps[s * 2 + 1]};
            acc = merge(acc, b);
        }
    }
    red[0][g][cl] = acc.W;
    red[1][g][cl] = acc.m;
    red[2][g][cl] = acc.M;
    red[3][g][cl] = acc.ww;
    __syncthreads();
    for (int w = CF_LANES / 2; w > 0; w >>= 1) {
        Moments r{0.f, 0.f, 0.f, 0.f};
        if (g < w) {
            const Moments a{red[0][g][cl], red[1][g][cl], red[2][g][cl], red[3][g][cl]};
            const Moments b{red[0][g + w][cl], red[1][g + w][cl], red[2][g + w][cl], red[3][g + w][cl]};
            r = merge(a, b);
        }
        __syncthreads();
        if (g < w) {
            red[0][g][cl] = r.W;
            red[1][g][cl] = r.m;
            red[2][g][cl] = r.M;
            red[3][g][cl] = r.ww;
        }
        __syncthreads();
    }
    if (g != 0 || col >= d) return;
    const float W = red[0][0][cl], m = red[1][0][cl], M = red[2][0][cl], ww = red[3][0][cl];
    if (!match) {
        out_a[col] = m;
        // 1 - sum w'^2 == 0: one row carries all the weight and the variance is exactly 0 -- 0 / 0, NaN as in the
        // reference (whose rounding of M2 does not then leave a residue to divide by 0)
        const float den = 1.f - ww / (W * W);
        out_b[col] = den == 0.f ? __builtin_nanf("") : sqrtf((M / W) / den);
        return;
    }
    const float st = sqrtf(M / (W - 1.f));
    const float dm = mean_s[col] - m, ds = std_s[col] - st;
    out_a[col] = m;
    out_b[col] = st;
    terms[col] = dm * dm;
    terms[d + col] = ds * ds;
    coef[col] = -2.f * dm / W;
    coef[d + col] = st == 0.f ? 0.f : -2.f * ds / ((W - 1.f) * st);
}

__global__ void __launch_bounds__(TB)
k_match_bwd(const float* __restrict__ x, int64_t ldx, int64_t n, int d, const float* __restrict__ mean_t,
            const float* __restrict__ coef, const float* __restrict__ gloss, float* __restrict__ gx, int64_t ldgx) {
    const float g = gloss[0];
    const int64_t total = n * d;
    for (int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x; e < total; e += (int64_t)gridDim.x * TB) {
        const int64_t row = e / d;
        const int col = (int)(e - row * d);
        gx[row * ldgx + col] = g * (coef[col] + coef[d + col] * (x[row * ldx + col] - mean_t[col]));
    }
}

unsigned elem_grid(int64_t total) {
    int64_t g = gda_cdiv(total, TB);
    if (g > 2048) g = 2048;
    return (unsigned)(g < 1 ? 1 : g);
}

size_t colstat_bytes(int64_t n, int64_t d) {
    const ColPlan p = col_plan(n, d);
    return (size_t)(p.slabs * d * 2 + p.slabs * 2 + 2 * d) * sizeof(float);
}

bool col_args_ok(int64_t n, int64_t d, int64_t ld) {
    return n >= 1 && d >= 1 && n < INT32_MAX && d <= (1 << 22) && ld >= d;
}

int colstat_launch(const float* x, int64_t ldx, const float* w, int64_t n, int64_t d, int match, const float* mean_s,
                   const float* std_s, float* out_a, float* out_b, float* coef, float* loss, void* ws,
                   hipStream_t s) {
    const ColPlan p = col_plan(n, d);
    float* pm = static_cast<float*>(ws);
    float* ps = pm + p.slabs * d * 2;
    float* terms = ps + p.slabs * 2;
    k_colstat_partial<<<dim3((unsigned)p.slabs, (unsigned)p.tiles), TB, 0, s>>>(x, ldx, w, n, (int)d, p.ct, p.rs, pm, ps);
    GDA_LAUNCH_CHECK();
    k_colstat_final<<<(unsigned)gda_cdiv(d, CF_COLS), TB, 0, s>>>(pm, ps, p.slabs, (int)d, match, mean_s, std_s, out_a,
                                                                  out_b, terms, coef);
    GDA_LAUNCH_CHECK();
    if (match) {
        k_sum_final<<<1, TB, 0, s>>>(terms, d, terms + d, d, 1.f, loss);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

}  // namespace

extern "C" size_t gda_closs_workspace_bytes(int64_t n, int64_t c) {
    if (n < 1 || c < 1) return 256;
    return (size_t)closs_blocks(n, c) * sizeof(float);
}

extern "C" int gda_closs_fwd_f32(const float* z, int64_t ldz, const int64_t* y, int64_t n, int64_t c, float* loss,
                                 float* weight, float* factor, void* workspace, size_t workspace_bytes,
                                 gda_stream_t stream) {
    if (n < 1 || c < 1 || n >= INT32_MAX || c >= INT32_MAX || ldz < c) return GDA_E_SIZE;
    if (!z || !y || !loss || !weight || !factor || !workspace) return GDA_E_NULL;
    if (workspace_bytes < gda_closs_workspace_bytes(n, c)) return GDA_E_WORKSPACE;
    const int G = closs_lanes(c), blocks = closs_blocks(n, c);
    float* partial = static_cast<float*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    k_closs_fwd<<<blocks, TB, 0, s>>>(z, ldz, y, n, (int)c, G, weight, factor, partial, loss);
    GDA_LAUNCH_CHECK();
    if (blocks > 1) {
        k_sum_final<<<1, TB, 0, s>>>(partial, blocks, nullptr, 0, (float)n, loss);
        GDA_LAUNCH_CHECK();
    }
    return GDA_OK;
}

extern "C" int gda_closs_bwd_f32(const float* z, int64_t ldz, const int64_t* y, const float* factor,
                                 const float* gloss, int64_t n, int64_t c, float* gz, int64_t ldgz,
                                 gda_stream_t stream) {
    if (n < 1 || c < 1 || n >= INT32_MAX || c >= INT32_MAX || ldz < c || ldgz < c) return GDA_E_SIZE;
    if (!z || !y || !factor || !gloss || !gz) return GDA_E_NULL;
    if (gz == z) return GDA_E_ALIAS;
    k_closs_bwd<<<elem_grid(n * c), TB, 0, (hipStream_t)stream>>>(z, ldz, y, factor, gloss, n, (int)c, gz, ldgz);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_colstats_workspace_bytes(int64_t n, int64_t d) {
    if (n < 1 || d < 1 || d > (1 << 22)) return 256;
    return colstat_bytes(n, d);
}

extern "C" int gda_weighted_moments_f32(const float* x, int64_t ldx, const float* w, int64_t n, int64_t d, float* mean,
                                        float* std, void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (!col_args_ok(n, d, ldx)) return GDA_E_SIZE;
    if (!x || !w || !mean || !std || !workspace) return GDA_E_NULL;
    if (workspace_bytes < colstat_bytes(n, d)) return GDA_E_WORKSPACE;
    return colstat_launch(x, ldx, w, n, d, 0, nullptr, nullptr, mean, std, nullptr, nullptr, workspace,
                          (hipStream_t)stream);
}

extern "C" int gda_std_mean_match_fwd_f32(const float* x, int64_t ldx, int64_t n, int64_t d, const float* mean_s,
                                          const float* std_s, float* loss, float* mean_t, float* std_t, float* coef,
                                          void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (!col_args_ok(n, d, ldx)) return GDA_E_SIZE;
    if (!x || !mean_s || !std_s || !loss || !mean_t || !std_t || !coef || !workspace) return GDA_E_NULL;
    if (workspace_bytes < colstat_bytes(n, d)) return GDA_E_WORKSPACE;
    return colstat_launch(x, ldx, nullptr, n, d, 1, mean_s, std_s, mean_t, std_t, coef, loss, workspace,
                          (hipStream_t)stream);
}

extern "C" int gda_std_mean_match_bwd_f32(const float* x, int64_t ldx, int64_t n, int64_t d, const float* mean_t,
                                          const float* coef, const float* gloss, float* gx, int64_t ldgx,
                                          gda_stream_t stream) {
    if (!col_args_ok(n, d, ldx) || ldgx < d) return GDA_E_SIZE;
    if (!x || !mean_t || !coef || !gloss || !gx) return GDA_E_NULL;
    if (gx == x) return GDA_E_ALIAS;
    k_match_bwd<<<elem_grid(n * d), TB, 0, (hipStream_t)stream>>>(x, ldx, n, (int)d, mean_t, coef, gloss, gx, ldgx);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
