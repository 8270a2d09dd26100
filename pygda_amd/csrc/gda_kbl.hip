// KBL (pygda/models/kbl.py, pygda/nn/kbl_base.py): the pair-similarity loss of the bridge model over the Cartesian
// product of two index lists, and the global top-k of the cosine between every source and every target row.  Neither
// stores the [ma mb, d] gathers or the [na, nb] array the reference forms.  fp32, no atomics, gfx950.  Rows are
// normalised once (x / max(|x|, 1e-8), torch's cosine_similarity); the products are gda_pair_tile.h's 64x64 tiles on
// v_mfma_f32_32x32x2_f32.  As in gda_graphcta.hip a workgroup owns row tiles and one contiguous share of the column
// tiles; what the shares leave -- loss partials, gradient partials, candidate lists -- is folded in a fixed order by
// the launch that follows, so two runs give the same bits.  See include/gda_hip.h for the contracts.
#include "gda_common.h"
#include "gda_pair_tile.h"
#include "gda_reduce.h"

#include <limits.h>
#include <math.h>

namespace {

using namespace gda_pair_tile;                // TB, TILE, DK, LDT, TileLds, load4, tile_product
constexpr int ROWS = TB / GDA_WAVE;           // a wavefront per row in the row kernels
constexpr int MAXS = 8;                       // column splits
constexpr int MAXD = GDA_KBL_MAX_WIDTH;
constexpr int MAXM = GDA_KBL_MAX_PAIR_ROWS;
constexpr int MAXK = GDA_KBL_MAX_K;
constexpr int MAXG = 128;                     // workgroups along the row tiles of the top-k (each strides over its tiles)
constexpr float COS_EPS = 1e-8f;              // cosine_similarity's clamp of each norm
const int64_t LIM = (int64_t)1 << 31;

static_assert(MAXK <= TB, "a thread per list entry");
static_assert(MAXD <= 8 * 32, "the second product covers eight 32-wide feature blocks");

bool aligned(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

struct Split { int tps, s; };
Split make_split(int64_t row_groups, int64_t cols, int64_t per_cu = 1, bool round_up = true) {
    const int64_t ct = gda_cdiv(cols, TILE);
    int64_t s = round_up ? gda_cdiv(256 * per_cu, row_groups) : 256 * per_cu / row_groups;      // 256 CUs
    s = s < 1 ? 1 : s > MAXS ? MAXS : s;
    s = s > ct ? ct : s;
    const int64_t tps = gda_cdiv(ct, s);
    return {(int)tps, (int)gda_cdiv(ct, tps)};
}

// ---- Xh[p] = X[idx[p]] / max(|X[idx[p]]|, 1e-8) (idx == nullptr: row p itself), a wavefront per row; lab[p] =
//      y[idx[p]].  An index outside [0, n) reads as a zero row with the label -1 - p (equal to no other) -----------------
__global__ void __launch_bounds__(TB)
k_kbl_normalize(const float* __restrict__ X, int64_t n, int d, const int32_t* __restrict__ idx, int64_t m,
                const int32_t* __restrict__ y, float* __restrict__ Xh, int32_t* __restrict__ lab) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (p >= m) return;
    const int64_t src = idx ? (int64_t)idx[p] : p;
    const bool ok = src >= 0 && src < n;
    const float* x = X + (ok ? src : 0) * d;
    float a = 0.f;
    for (int k = lane; k < d; k += GDA_WAVE) a = fmaf(x[k], x[k], a);
    const float den = fmaxf(sqrtf(wave_sum(a)), COS_EPS);
    for (int k = lane; k < d; k += GDA_WAVE) Xh[p * d + k] = ok ? x[k] / den : 0.f;
    if (lab && lane == 0) lab[p] = ok ? y[src] : (int32_t)(-1 - p);
}

// ---- the pair loss over the rows' share of the ma x mb product.  Per tile: c = <a^_p, b^_q>, s = sigmoid(c),
//      t = [la_p == lb_q]; the loss terms are summed (Lpart, when asked for) and g_pq = (s - t) scale goes to LDS, from
//      where G B^ is accumulated on the matrix cores: wave w owns rows 32 (w & 1).. and the 32-wide feature blocks
//      (w >> 1), (w >> 1) + 2, ..  The same kernel with the roles swapped gives G^T A^ ---------------------------------------
__global__ void __launch_bounds__(TB)
k_kbl_pairs(const float* __restrict__ Ah, const int32_t* __restrict__ la, int64_t ma, const float* __restrict__ Bh,
            const int32_t* __restrict__ lb, int64_t mb, int d, int tps, float scale, double* __restrict__ Lpart,
            float* __restrict__ Gpart, bool vec) {
    __shared__ TileLds L;
    __shared__ float Es[TILE][LDT];
    __shared__ int li_s[TILE], lj_s[TILE];
    __shared__ double red[TB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 31, ka = lane >> 5;
    const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
    const int64_t i0 = (int64_t)blockIdx.x * TILE;
    const int64_t ntiles = (mb + TILE - 1) / TILE;
    const int64_t jt0 = (int64_t)blockIdx.y * tps, jt1 = jt0 + tps < ntiles ? jt0 + tps : ntiles;
    f32x16 og[4];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) og[q][r] = 0.f;
    double loss = 0.0;
    if (tid < TILE) li_s[tid] = i0 + tid < ma ? la[i0 + tid] : 0;
    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = jt * TILE;
        const f32x16 acc = tile_product(Ah, ma, i0, Bh, mb, j0, d, vec, L);
        __syncthreads();                                   // the tile before: its second product has read Es
        if (tid < TILE) lj_s[tid] = j0 + tid < mb ? lb[j0 + tid] : 0;
        __syncthreads();
        const int lj = wj + lc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int li = wi + (r & 3) + 8 * (r >> 2) + 4 * ka;
            float g = 0.f;
            if (i0 + li < ma && j0 + lj < mb) {
                const float s = 1.f / (1.f + expf(-acc[r]));
                const bool same = li_s[li] == lj_s[lj];
                // binary_cross_entropy: each logarithm clamped at -100
                loss -= (double)(same ? fmaxf(logf(s), -100.f) : fmaxf(log1pf(-s), -100.f));
                g = (s - (same ? 1.f : 0.f)) * scale;
            }
            Es[lj][li] = g;
        }
        __syncthreads();
        const int fb0 = wave >> 1;
        for (int k = 0; k < TILE; k += 2) {
            const float a = Es[k + ka][wi + lc];
            const int64_t jj = j0 + k + ka;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = (fb0 + 2 * q) * 32 + lc;
                if ((fb0 + 2 * q) * 32 < d) {              // wave-uniform
                    const float b = (jj < mb && col < d) ? Bh[jj * d + col] : 0.f;
                    og[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, og[q], 0, 0, 0);
                }
            }
        }
    }
    const int fb0 = wave >> 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col = (fb0 + 2 * q) * 32 + lc;
        if (col >= d) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = i0 + wi + (r & 3) + 8 * (r >> 2) + 4 * ka;
            if (i < ma) Gpart[((int64_t)blockIdx.y * ma + i) * d + col] = og[q][r];
        }
    }
    if (Lpart) {                                           // kernel-uniform
        loss = block_sum_d(loss, red);
        if (tid == 0) Lpart[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = loss;
    }
}

__global__ void k_kbl_loss_sum(const double* __restrict__ Lpart, int parts, double pairs, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = 0.0;
    for (int p = 0; p < parts; ++p) a += Lpart[p];
    out[0] = (float)(a / pairs);
}

// ---- dU: per node the partials of every list position that names it -- ia in order, then ib in order, the splits in
//      order inside each -- and the chain through x / max(|x|, 1e-8).  A wavefront per node --------------------------------
__device__ __forceinline__ void fold_list(const int32_t* __restrict__ idx, int64_t m, int64_t node,
                                          const float* __restrict__ G, int s, int d, int lane, float* g) {
    for (int64_t p0 = 0; p0 < m; p0 += GDA_WAVE) {
        const int64_t p = p0 + lane;
        unsigned long long hit = __ballot(p < m && (int64_t)idx[p] == node);
        while (hit) {
            const int64_t pp = p0 + __ffsll((long long)hit) - 1;
            hit &= hit - 1;
            for (int q = 0; q < s; ++q)
#pragma unroll
                for (int t = 0; t < MAXD / GDA_WAVE; ++t) {
                    const int k = lane + GDA_WAVE * t;
                    if (k < d) g[t] += G[((int64_t)q * m + pp) * d + k];
                }
        }
    }
}

__global__ void __launch_bounds__(TB)
k_kbl_fold(const float* __restrict__ U, int64_t n, int d, const int32_t* __restrict__ ia, int64_t ma,
           const int32_t* __restrict__ ib, int64_t mb, const float* __restrict__ GA, int sa, const float* __restrict__ GB,
           int sb, float* __restrict__ dU) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * ROWS + (threadIdx.x >> 6);
    if (i >= n) return;
    float g[MAXD / GDA_WAVE];
#pragma unroll
    for (int t = 0; t < MAXD / GDA_WAVE; ++t) g[t] = 0.f;
    fold_list(ia, ma, i, GA, sa, d, lane, g);
    fold_list(ib, mb, i, GB, sb, d, lane, g);
    const float* x = U + i * d;
    float a = 0.f;
    for (int k = lane; k < d; k += GDA_WAVE) a = fmaf(x[k], x[k], a);
    const float nr = sqrtf(wave_sum(a)), den = fmaxf(nr, COS_EPS);
    float dot = 0.f;
#pragma unroll
    for (int t = 0; t < MAXD / GDA_WAVE; ++t) {
        const int k = lane + GDA_WAVE * t;
        if (k < d) dot = fmaf(g[t], x[k] / den, dot);
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int t = 0; t < MAXD / GDA_WAVE; ++t) {
        const int k = lane + GDA_WAVE * t;
        if (k < d) dU[i * d + k] = nr >= COS_EPS ? (g[t] - (x[k] / den) * dot) / nr : g[t] / COS_EPS;
    }
}

// ---- the running list: K entries sorted by (value descending, flat index ascending).  Unused entries are
//      (-inf, LLONG_MAX - slot): behind every pair and distinct from each other, so every key of an offer is distinct and
//      the ranks below are a bijection -----------------------------------------------------------------------------------
constexpr int OFFER = 4;                      // candidates a thread may offer at once
constexpr int CAND = OFFER * TB;

__device__ __forceinline__ bool better(float v, long long f, float ev, long long ef) { return v > ev || (v == ev && f < ef); }

struct TopList {
    float v[2][MAXK];
    long long f[2][MAXK];
    float cv[CAND];
    long long cf[CAND];
    int wsum[2][TB / GDA_WAVE];
};

// cur: the buffer that holds the list; par: which wsum row the next offer uses (two offers apart share a row, and an
// offer's first barrier lies between them)
struct ListState { int cur, par; };

__device__ __forceinline__ ListState list_init(TopList& T, int K) {
    const int tid = threadIdx.x;
    if (tid < K) {
        T.v[0][tid] = -INFINITY;
        T.f[0][tid] = LLONG_MAX - tid;
    }
    return {0, 0};
}

// One offer: every thread hands in up to OFFER candidates (bit j of pass: candidate j beats the list's last entry).  They
// are packed into cv / cf by a scan of the counts (lane order inside a wavefront, then wavefront order); an offer without
// a candidate costs one barrier.  Otherwise every candidate and every list entry finds its rank in the union by
// counting -- the list is sorted, so an entry's rank among the entries is its slot -- and the first K go to the other
// buffer.
__device__ __forceinline__ void list_offer(TopList& T, ListState& S, int K, unsigned pass, const float* v,
                                           const long long* f) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int count = __popc(pass);
    int incl = count;
#pragma unroll
    for (int o = 1; o < GDA_WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o, GDA_WAVE);
        if (lane >= o) incl += up;
    }
    int* wsum = T.wsum[S.par];
    S.par ^= 1;
    if (lane == GDA_WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    int total = 0, at = incl - count;
#pragma unroll
    for (int w = 0; w < TB / GDA_WAVE; ++w) {
        total += wsum[w];
        at += w < wave ? wsum[w] : 0;
    }
    if (total == 0) return;                                // uniform
#pragma unroll
    for (int j = 0; j < OFFER; ++j)
        if (pass >> j & 1) {
            T.cv[at] = v[j];
            T.cf[at] = f[j];
            ++at;
        }
    __syncthreads();
    const int cur = S.cur, nxt = cur ^ 1;
    for (int c = tid; c < total; c += TB) {
        const float xv = T.cv[c];
        const long long xf = T.cf[c];
        int rank = 0;
#pragma unroll 8                                           // (independent LDS reads in flight: four waves hide no latency)
        for (int e = 0; e < K; ++e) rank += better(T.v[cur][e], T.f[cur][e], xv, xf);
#pragma unroll 8
        for (int e = 0; e < total; ++e) rank += better(T.cv[e], T.cf[e], xv, xf);
        if (rank < K) { T.v[nxt][rank] = xv; T.f[nxt][rank] = xf; }
    }
    if (tid < K) {
        const float ev = T.v[cur][tid];
        const long long ef = T.f[cur][tid];
        int rank = tid;
#pragma unroll 8
        for (int e = 0; e < total; ++e) rank += better(T.cv[e], T.cf[e], ev, ef);
        if (rank < K) { T.v[nxt][rank] = ev; T.f[nxt][rank] = ef; }
    }
    __syncthreads();
    S.cur = nxt;
}

// ---- the bridge top-k, first launch: workgroup (x, y) streams the row tiles x, x + gridDim.x, .. against the column
//      tiles of share y.  A tile without an element that beats the list's last entry costs one barrier; any other is
//      offered in four quarters of four elements per thread -- one element at a time while more than a quarter of the
//      threads hold a candidate (the list is filling: a short offer raises the bar for the next) --, the last entry read
//      afresh for each offer.  NaN counts as +inf.  The lists are stored position-major, [K][lists] ----------------------
__global__ void __launch_bounds__(TB)
k_kbl_topk_tiles(const float* __restrict__ Ah, int64_t na, const float* __restrict__ Bh, int64_t nb, int d, int K,
                 int tps, float* __restrict__ pval, long long* __restrict__ pflat, bool vec) {
    __shared__ TileLds L;
    __shared__ float Ts[TILE][LDT];
    __shared__ TopList T;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lc = lane & 31, ka = lane >> 5;
    const int wi = (wave & 1) * 32, wj = (wave >> 1) * 32;
    const int r = tid & 63, q = tid >> 6;                  // the scan: row r, columns 16 q .. 16 q + 15 of every tile
    const int64_t nrt = (na + TILE - 1) / TILE, nct = (nb + TILE - 1) / TILE;
    const int64_t jt0 = (int64_t)blockIdx.y * tps, jt1 = jt0 + tps < nct ? jt0 + tps : nct;
    ListState S = list_init(T, K);
    for (int64_t rt = blockIdx.x; rt < nrt; rt += gridDim.x) {
        const int64_t i0 = rt * TILE;
        for (int64_t jt = jt0; jt < jt1; ++jt) {
            const int64_t j0 = jt * TILE;
            const f32x16 acc = tile_product(Ah, na, i0, Bh, nb, j0, d, vec, L);   // its barriers fence the scan before
#pragma unroll
            for (int e = 0; e < 16; ++e) Ts[wi + (e & 3) + 8 * (e >> 2) + 4 * ka][wj + lc] = acc[e];
            __syncthreads();                               // (and list_init's stores, the first time)
            const int64_t i = i0 + r;
            float tv = T.v[S.cur][K - 1];
            long long tf = T.f[S.cur][K - 1];
            bool any = false;
            for (int c = 0; c < 16; ++c) {
                const int64_t j = j0 + 16 * q + c;
                float v = Ts[r][16 * q + c];
                if (v != v) v = INFINITY;
                any |= i < na && j < nb && better(v, i * nb + j, tv, tf);
            }
            const int holders = __syncthreads_count(any);
            if (!holders) continue;
            const int step = holders > TB / 4 ? 1 : OFFER;
            for (int c0 = 0; c0 < 16; c0 += step) {
                tv = T.v[S.cur][K - 1];
                tf = T.f[S.cur][K - 1];
                float v[OFFER];
                long long f[OFFER];
                unsigned pass = 0;
#pragma unroll
                for (int c = 0; c < OFFER; ++c) {
                    const int64_t j = j0 + 16 * q + c0 + c;
                    v[c] = Ts[r][16 * q + c0 + c];
                    if (v[c] != v[c]) v[c] = INFINITY;
                    f[c] = i * nb + j;
                    pass |= (c < step && i < na && j < nb && better(v[c], f[c], tv, tf) ? 1u : 0u) << c;
                }
                list_offer(T, S, K, pass, v, f);
            }
        }
    }
    __syncthreads();
    const int64_t lists = (int64_t)gridDim.x * gridDim.y, mine = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (tid < K) {
        pval[tid * lists + mine] = T.v[S.cur][tid];
        pflat[tid * lists + mine] = T.f[S.cur][tid];
    }
}

// ---- second launch, one workgroup: the candidate lists through the same offers -- every list's best entry first, which
//      sets a bar that few of the later entries pass --, then (row, col, sigmoid) ------------------------------------------
__global__ void __launch_bounds__(TB)
k_kbl_topk_merge(const float* __restrict__ pval, const long long* __restrict__ pflat, int64_t entries, int64_t na,
                 int64_t nb, int K, int32_t* __restrict__ row, int32_t* __restrict__ col, float* __restrict__ val) {
    __shared__ TopList T;
    const int tid = threadIdx.x;
    const long long total = (long long)na * nb;
    ListState S = list_init(T, K);
    __syncthreads();
    for (int64_t e0 = 0; e0 < entries; e0 += CAND) {
        const float tv = T.v[S.cur][K - 1];
        const long long tf = T.f[S.cur][K - 1];
        float v[OFFER];
        long long f[OFFER];
        unsigned pass = 0;
#pragma unroll
        for (int c = 0; c < OFFER; ++c) {
            const int64_t e = e0 + (int64_t)c * TB + tid;
            v[c] = e < entries ? pval[e] : -INFINITY;
            f[c] = e < entries ? pflat[e] : LLONG_MAX;
            pass |= (f[c] >= 0 && f[c] < total && better(v[c], f[c], tv, tf) ? 1u : 0u) << c;
        }
        const int holders = __syncthreads_count(pass != 0);
        if (!holders) continue;
        if (holders <= TB / 4) {
            list_offer(T, S, K, pass, v, f);
            continue;
        }
#pragma unroll
        for (int c = 0; c < OFFER; ++c) {                  // the list is filling: one element at a time, as in the tiles
            const bool still = (pass >> c & 1) && better(v[c], f[c], T.v[S.cur][K - 1], T.f[S.cur][K - 1]);
            list_offer(T, S, K, still ? 1u << c : 0u, v, f);
        }
    }
    __syncthreads();
    if (tid < K) {
        const long long f = T.f[S.cur][tid];
        const bool ok = f >= 0 && f < total;               // K <= na nb: every entry is a pair
        row[tid] = ok ? (int32_t)(f / nb) : 0;
        col[tid] = ok ? (int32_t)(f % nb) : 0;
        val[tid] = ok ? 1.f / (1.f + expf(-T.v[S.cur][tid])) : 0.f;
    }
}

// workspace layouts, in floats
struct PairWs { float *Ah, *Bh; int32_t *la, *lb; double* Lpart; float *GA, *GB; Split sa, sb; size_t floats; };
PairWs pair_ws(void* base, int64_t d, int64_t ma, int64_t mb) {
    PairWs w;
    w.sa = make_split(gda_cdiv(ma, TILE), mb);
    w.sb = make_split(gda_cdiv(mb, TILE), ma);
    float* p = static_cast<float*>(base);
    auto take = [&](size_t k) { float* q = p; p += (k + 3) / 4 * 4; return q; };
    w.Ah = take((size_t)ma * d);
    w.Bh = take((size_t)mb * d);
    w.la = reinterpret_cast<int32_t*>(take(ma));
    w.lb = reinterpret_cast<int32_t*>(take(mb));
    w.Lpart = reinterpret_cast<double*>(take(2 * (size_t)gda_cdiv(ma, TILE) * w.sa.s));
    w.GA = take((size_t)w.sa.s * ma * d);
    w.GB = take((size_t)w.sb.s * mb * d);
    w.floats = (size_t)(p - static_cast<float*>(base));
    return w;
}

struct TopkGrid { int gx; Split sp; };
TopkGrid topk_grid(int64_t na, int64_t nb) {
    const int64_t rt = gda_cdiv(na, TILE);
    const int gx = (int)(rt < MAXG ? rt : MAXG);
    return {gx, make_split(gx, nb, 3, false)};             // three workgroups' LDS fit a CU: all resident at once
}

struct TopkWs { float *Ah, *Bh, *pval; long long* pflat; size_t floats; };
TopkWs topk_ws(void* base, int64_t na, int64_t nb, int64_t d, int64_t k) {
    const TopkGrid g = topk_grid(na, nb);
    TopkWs w;
    float* p = static_cast<float*>(base);
    auto take = [&](size_t n) { float* q = p; p += (n + 3) / 4 * 4; return q; };
    w.Ah = take((size_t)na * d);
    w.Bh = take((size_t)nb * d);
    w.pval = take((size_t)g.gx * g.sp.s * k);
    w.pflat = reinterpret_cast<long long*>(take(2 * (size_t)g.gx * g.sp.s * k));
    w.floats = (size_t)(p - static_cast<float*>(base));
    return w;
}

bool pair_dims_ok(int64_t n, int64_t d, int64_t ma, int64_t mb) {
    return n >= 1 && n < LIM && d >= 1 && d <= MAXD && ma >= 1 && ma <= MAXM && mb >= 1 && mb <= MAXM;
}

bool topk_dims_ok(int64_t na, int64_t nb, int64_t d) {
    return na >= 1 && nb >= 1 && d >= 1 && na < LIM && nb < LIM && d < LIM / 64 && na * d < LIM * 16 && nb * d < LIM * 16;
}

}  // namespace

extern "C" size_t gda_kbl_pair_bce_workspace_bytes(int64_t d, int64_t ma, int64_t mb) {
    if (!pair_dims_ok(1, d, ma, mb)) return 256;
    return gda_align_up(pair_ws(nullptr, d, ma, mb).floats * sizeof(float), 256);
}

extern "C" int gda_kbl_pair_bce_f32(const float* U, const int32_t* ia, const int32_t* ib, const int32_t* y, int64_t n,
                                    int64_t d, int64_t ma, int64_t mb, float* out, float* dU, void* workspace,
                                    size_t workspace_bytes, gda_stream_t stream) {
    if (!pair_dims_ok(n, d, ma, mb)) return GDA_E_SIZE;
    if (!U || !ia || !ib || !y || !out || !dU || !workspace) return GDA_E_NULL;
    if (!aligned(U, 4) || !aligned(ia, 4) || !aligned(ib, 4) || !aligned(y, 4) || !aligned(out, 4) || !aligned(dU, 4)
        || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (dU == U) return GDA_E_ALIAS;
    if (workspace_bytes < gda_kbl_pair_bce_workspace_bytes(d, ma, mb)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const PairWs w = pair_ws(workspace, d, ma, mb);
    const bool vec = d % 4 == 0;                           // Ah, Bh are 16-byte aligned in the workspace
    const float scale = (float)(1.0 / ((double)ma * (double)mb));
    const unsigned ra = (unsigned)gda_cdiv(ma, TILE), rb = (unsigned)gda_cdiv(mb, TILE);
    k_kbl_normalize<<<(unsigned)gda_cdiv(ma, ROWS), TB, 0, st>>>(U, n, (int)d, ia, ma, y, w.Ah, w.la);
    GDA_LAUNCH_CHECK();
    k_kbl_normalize<<<(unsigned)gda_cdiv(mb, ROWS), TB, 0, st>>>(U, n, (int)d, ib, mb, y, w.Bh, w.lb);
    GDA_LAUNCH_CHECK();
    k_kbl_pairs<<<dim3(ra, (unsigned)w.sa.s), TB, 0, st>>>(w.Ah, w.la, ma, w.Bh, w.lb, mb, (int)d, w.sa.tps, scale,
                                                          w.Lpart, w.GA, vec);
    GDA_LAUNCH_CHECK();
    k_kbl_pairs<<<dim3(rb, (unsigned)w.sb.s), TB, 0, st>>>(w.Bh, w.lb, mb, w.Ah, w.la, ma, (int)d, w.sb.tps, scale,
                                                          nullptr, w.GB, vec);
    GDA_LAUNCH_CHECK();
    k_kbl_loss_sum<<<1, GDA_WAVE, 0, st>>>(w.Lpart, (int)(ra * w.sa.s), (double)ma * (double)mb, out);
    GDA_LAUNCH_CHECK();
    k_kbl_fold<<<(unsigned)gda_cdiv(n, ROWS), TB, 0, st>>>(U, n, (int)d, ia, ma, ib, mb, w.GA, w.sa.s, w.GB, w.sb.s, dU);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

extern "C" size_t gda_kbl_bridge_topk_workspace_bytes(int64_t na, int64_t nb, int64_t d, int64_t k) {
    if (!topk_dims_ok(na, nb, d) || k < 1 || k > MAXK) return 256;
    return gda_align_up(topk_ws(nullptr, na, nb, d, k).floats * sizeof(float), 256);
}

extern "C" int gda_kbl_bridge_topk_f32(const float* A, const float* B, int64_t na, int64_t nb, int64_t d, int64_t k,
                                       int32_t* row, int32_t* col, float* val, void* workspace, size_t workspace_bytes,
                                       gda_stream_t stream) {
    if (!topk_dims_ok(na, nb, d) || k < 1 || k > na * nb) return GDA_E_SIZE;
    if (k > MAXK) return GDA_E_UNSUPPORTED;
    if (!A || !B || !row || !col || !val || !workspace) return GDA_E_NULL;
    if (!aligned(A, 4) || !aligned(B, 4) || !aligned(row, 4) || !aligned(col, 4) || !aligned(val, 4)
        || !aligned(workspace, 16))
        return GDA_E_UNSUPPORTED;
    if (workspace_bytes < gda_kbl_bridge_topk_workspace_bytes(na, nb, d, k)) return GDA_E_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const TopkWs w = topk_ws(workspace, na, nb, d, k);
    const TopkGrid g = topk_grid(na, nb);
    const bool vec = d % 4 == 0;
    k_kbl_normalize<<<(unsigned)gda_cdiv(na, ROWS), TB, 0, st>>>(A, na, (int)d, nullptr, na, nullptr, w.Ah, nullptr);
    GDA_LAUNCH_CHECK();
    k_kbl_normalize<<<(unsigned)gda_cdiv(nb, ROWS), TB, 0, st>>>(B, nb, (int)d, nullptr, nb, nullptr, w.Bh, nullptr);
    GDA_LAUNCH_CHECK();
    k_kbl_topk_tiles<<<dim3((unsigned)g.gx, (unsigned)g.sp.s), TB, 0, st>>>(w.Ah, na, w.Bh, nb, (int)d, (int)k, g.sp.tps,
                                                                          w.pval, w.pflat, vec);
    GDA_LAUNCH_CHECK();
    k_kbl_topk_merge<<<1, TB, 0, st>>>(w.pval, w.pflat, (int64_t)g.gx * g.sp.s * k, na, nb, (int)k, row, col, val);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
