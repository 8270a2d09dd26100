// K aggregation steps on a SAMPLED batch in ONE launch of the step loop (round 5; included by gda_spmm.hip).
//
// Replaces, for a NeighborLoader batch, the K dependent launches gda_spmm_csr_interior_kstep_f32 makes of the
// prop_nums loop of pygda/nn/prop_gcn_conv.py:208-210 (cfg-S: 55 launches of 13.5 us per training step).
//
// What the K steps really iterate on such a batch is small.  Rows [n_int, n) (the last hop's discoveries) hold their
// unit self loop only and never change; the interior rows obey  y_I <- A_II y_I + c  with  c = A_IL x_L  formed once, and
// A_II of a fan-out [15, 10] batch of 1024 seeds is ~16.4 k rows with ONE diagonal entry each plus ~15 k off-diagonal
// entries (the seeds' sampled neighbours; a last-but-one-hop node's own neighbours are leaves).  Per FEATURE COLUMN
// that is a 64 KB vector: the step loop runs with one workgroup per column, the column ping-pong in LDS, workgroup
// barriers only -- the structure of csrc/gda_kstep.hip, with three differences forced by the setting:
//   * the graph changes every step, so the per-lane register program is built ON THE DEVICE (k_il_count / _scan /
//     _entries, on the sampler's stream beside the batch's CSR pair: nothing on the training stream), in a form a parallel
//     builder can emit: the T off-diagonal interior entries in row order, cut into 1024 runs of q = ceil(T / 1024) <=
//     IL_E entries -- balanced to the entry whatever the rows look like; an entry = {LDS word of the neighbour : 16 |
//     LDS word its running sum is stored to : 16, weight}: a row's last entry stores to the row's word, an entry that
//     finishes nothing to a dump word, and a row cut by a run boundary is summed in pieces that the thread holding its
//     last piece adds up in run order after a barrier (a fixed order: deterministic);
//   * the diagonal (every row has one) and the constant c are the ROW OWNER's registers (thread t owns rows t + 1024 s:
//     conflict-free LDS accesses), so a step is: plan entries -> barrier -> cut rows' pieces -> barrier -> owner pass
//     -> barrier;
//   * the interior block (<= 17,408 rows) needs more than the 2 x 64 KB the 16-bit DS offset trick of gda_kstep.hip
//     addresses: buffer bases are run-time values, one v_lshl_add per access.
// Sums: a row is (its off-diagonal interior entries in CSR = edge order, separately rounded multiply and add) + diagonal
// + c -- for the GCN-normalised CSRs of this library (self loop last in its row) the chain of the hoisted k_spmm_range
// steps it replaces, bit for bit for every row that lies inside one run; a row cut by a run boundary adds its pieces'
// sums instead (fp32 summation order, as the hoisted chain itself against the unhoisted one).  The transposed operator
// (backward) likewise, with the running sum of the step inputs (h_0 + ... + h_{K-1}, needed by the leaf rows at the end)
// kept in the owner's registers where the forward pass keeps c.
// Bound: LDS gather rate / VALU issue of one CU per column; HBM sees one read of x (leaf rows gathered once for c),
// one write of y.

namespace {

constexpr int IL_TB = 1024;                     // 16 wavefronts per workgroup, <= 128 VGPRs each
constexpr int IL_E = 26;                        // plan entries per thread: T <= 26,624 off-diagonal interior entries (123 VGPRs; 28 spills)
constexpr int IL_RS = 16;                       // rows per owner thread
constexpr int IL_MAX_ROWS = IL_RS * IL_TB;      // 16,384 interior rows: 1024 seeds at fan-out 15
constexpr int IL_MAX_D = 128;                   // feature width of the LDS path (one workgroup per column)
// words of one LDS buffer: 0 reads as 0 (unused plan entries); [IL_DUMP0, +64) take the stores of entries that finish
// nothing -- one word per LANE: 64 lanes storing to one address cost the step loop ~2 us per step (first version: one
// dump word, k_il_lds 52 us at K = 10); [IL_PW, +1024) the partial sum a run leaves unfinished at its end, [IL_LW, +1024)
// the sum with which a run's first segment finishes a row begun in an earlier run, then the node words
constexpr unsigned IL_ZERO = 0u, IL_DUMP0 = 64u, IL_PW = 128u, IL_LW = IL_PW + IL_TB;
constexpr int IL_HEAD = (int)IL_LW + IL_TB;     // 2176: node i lives at word IL_HEAD + i (16-byte aligned start)
__host__ __device__ constexpr uint32_t il_dump(int thread) { return IL_DUMP0 + (uint32_t)(thread & 63); }
constexpr int IL_TILE = 32;                     // rows of a transposition tile
static_assert(IL_HEAD % 4 == 0 && IL_HEAD + IL_MAX_ROWS < 65536, "word indices travel in 16 bits");
static_assert(2 * (IL_HEAD + IL_MAX_ROWS) * 4 <= 160 * 1024, "both buffers in one CU's LDS");

constexpr size_t IL_OFF_PW = (size_t)IL_TB * IL_E * 4;
constexpr size_t IL_OFF_DIAG = 2 * IL_OFF_PW;
constexpr size_t IL_OFF_ACT = IL_OFF_DIAG + (size_t)IL_MAX_ROWS * 4;
constexpr size_t IL_OFF_LEAD = IL_OFF_ACT + (size_t)IL_TB * 4;
constexpr size_t IL_OFF_WMAX = IL_OFF_LEAD + (size_t)IL_TB * 4;
constexpr size_t IL_OFF_CNT = IL_OFF_WMAX + 256;                      // builder scratch: per-row counts, row prefixes
constexpr size_t IL_OFF_ROWP = IL_OFF_CNT + (size_t)IL_MAX_ROWS * 4;
constexpr size_t IL_PLAN_BYTES = IL_OFF_ROWP + (size_t)IL_MAX_ROWS * 4;

struct IlPlan {
    const uint32_t* pk;      // [16 waves][IL_E][64]: neighbour word | store word << 16
    const float* pw;         // same layout: weights
    const float* diag;       // [IL_MAX_ROWS]: the row's diagonal weight (0 beyond n_int)
    const uint32_t* actm;    // [1024]: bit s = row t + 1024 s has off-diagonal interior entries
    const uint32_t* lead;    // [1024]: 0, or word of the row run t's first segment finishes | runs before it that hold it << 16
    const uint32_t* wmax;    // [16]: entries the longest run of the wave holds
};

inline IlPlan il_plan(const void* plan) {
    const char* p = static_cast<const char*>(plan);
    return IlPlan{reinterpret_cast<const uint32_t*>(p), reinterpret_cast<const float*>(p + IL_OFF_PW),
                  reinterpret_cast<const float*>(p + IL_OFF_DIAG), reinterpret_cast<const uint32_t*>(p + IL_OFF_ACT),
                  reinterpret_cast<const uint32_t*>(p + IL_OFF_LEAD), reinterpret_cast<const uint32_t*>(p + IL_OFF_WMAX)};
}

__device__ __forceinline__ size_t il_slot(int thread, int e) {
    return ((size_t)(thread >> 6) * IL_E + (size_t)e) * 64 + (size_t)(thread & 63);
}

// ---- the plan, built on the device -------------------------------------------------------------------------------------
// The off-diagonal interior entries in row order (T of them) are cut into 1024 runs of q = ceil(T / 1024) entries: entry
// g belongs to thread g / q, slot g % q -- balanced to the entry, whatever the rows look like (a seed row of 15 entries
// forward, fifteen one-entry rows transposed, a hub row of hundreds).  A row that crosses a run boundary is summed in
// pieces: every run but the row's last leaves its piece in its P word, the last run's leading piece goes to its L word,
// and after a barrier the last run's thread adds them up in run order (k_il_lds, phase 1b).
// Three capacity-sized launches that read the live n_int from device memory: per-row counts + diagonal (a thread per
// row) | prefix over the rows, q, the verdict, defaults (one workgroup) | the entries (a thread per row).
// status[0] <- q (>= 1: the plan is valid), or 0 when the batch does not fit (more than IL_MAX_ROWS interior rows, more
// than 1024 * IL_E off-diagonal interior entries): the caller then keeps the launch chain.
__global__ void __launch_bounds__(256)
k_il_count(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ val,
           const int64_t* __restrict__ n_int_dev, float* __restrict__ diag, uint32_t* __restrict__ cnt) {
    const int64_t n_int64 = *n_int_dev;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (n_int64 <= 0 || n_int64 > IL_MAX_ROWS || i >= IL_MAX_ROWS) return;
    const int n_int = (int)n_int64;
    float dsum = 0.f;
    uint32_t c_off = 0;
    if (i < n_int) {
        const int32_t b = rowptr[i], e = rowptr[i + 1];
        for (int32_t k = b; k < e; ++k) {
            const int32_t c = colidx[k];
            if (c == i) dsum = __fadd_rn(dsum, val[k]);
            else if (c < n_int) ++c_off;
        }
    }
    diag[i] = dsum;                                               // 0 beyond n_int
    cnt[i] = c_off;
}

__global__ void __launch_bounds__(IL_TB)
k_il_scan(const int64_t* __restrict__ n_int_dev, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ rowp,
          uint32_t* __restrict__ pk, float* __restrict__ pw, uint32_t* __restrict__ actm, uint32_t* __restrict__ lead,
          uint32_t* __restrict__ wmax, int64_t* __restrict__ status) {
    __shared__ uint32_t s_scan[IL_TB];
    const int t = threadIdx.x;
    const int64_t n_int64 = *n_int_dev;
    if (n_int64 <= 0 || n_int64 > IL_MAX_ROWS) {                  // uniform
        if (t == 0) *status = 0;
        return;
    }
    const int n_int = (int)n_int64;
    const int rpt = (n_int + IL_TB - 1) / IL_TB;
    const int r0 = min(t * rpt, n_int), r1 = min(r0 + rpt, n_int);
    uint32_t total = 0;
    for (int i = r0; i < r1; ++i) total += cnt[i];
    s_scan[t] = total;
    __syncthreads();
    for (int off = 1; off < IL_TB; off <<= 1) {                   // Hillis-Steele over the 1024 chunk totals
        const uint32_t add = t >= off ? s_scan[t - off] : 0u;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    const uint32_t T = s_scan[IL_TB - 1];
    const uint32_t q = T == 0 ? 1u : (T + IL_TB - 1) / IL_TB;
    if (q > (uint32_t)IL_E) {                                     // uniform
        if (t == 0) *status = 0;
        return;
    }
    uint32_t P = s_scan[t] - total;
    for (int i = r0; i < r1; ++i) { rowp[i] = P; P += cnt[i]; }
    // the unused tail of this thread's run, the per-thread words the entry pass fills in
    const uint32_t lo = min((uint32_t)t * q, T), hi = min(lo + q, T);
    for (int e = (int)(hi - lo); e < IL_E; ++e) {
        const size_t at = il_slot(t, e);
        pk[at] = IL_ZERO | (il_dump(t) << 16);
        pw[at] = 0.f;
    }
    actm[t] = 0u;
    lead[t] = 0u;
    if (t < IL_TB / 64) wmax[t] = min(q, T - min((uint32_t)t * 64u * q, T));     // runs of a wave are full from its first on
    if (t == 0) { status[0] = (int64_t)q; status[1] = (int64_t)T; }
}

__global__ void __launch_bounds__(256)
k_il_entries(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ val,
             const int64_t* __restrict__ n_int_dev, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ rowp,
             const int64_t* __restrict__ status, uint32_t* __restrict__ pk, float* __restrict__ pw,
             uint32_t* __restrict__ actm, uint32_t* __restrict__ lead) {
    const int64_t q64 = status[0];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (q64 <= 0 || i >= (int)*n_int_dev) return;
    const uint32_t q = (uint32_t)q64, T = (uint32_t)status[1];
    const int n_int = (int)*n_int_dev;
    const uint32_t n_off = cnt[i];
    if (!n_off) return;
    const uint32_t P = rowp[i];
    const uint32_t first_run = P / q;
    const int32_t b = rowptr[i], e = rowptr[i + 1];
    uint32_t j = 0;
    for (int32_t k = b; k < e; ++k) {
        const int32_t c = colidx[k];
        if (c == i || c >= n_int) continue;
        const uint32_t g = P + j;
        const uint32_t run = g / q, slot = g - run * q;
        const bool row_ends = j + 1 == n_off, run_ends = slot + 1 == q || g + 1 == T;
        uint32_t store = il_dump((int)run);
        if (row_ends) {
            if (run == first_run) store = (uint32_t)(IL_HEAD + i);
            else { store = IL_LW + run; lead[run] = (uint32_t)(IL_HEAD + i) | ((run - first_run) << 16); }
        } else if (run_ends) {
            store = IL_PW + run;
        }
        const size_t at = il_slot((int)run, (int)slot);
        pk[at] = (uint32_t)(IL_HEAD + c) | (store << 16);
        pw[at] = val[k];
        ++j;
    }
    atomicOr(&actm[i & (IL_TB - 1)], 1u << (i >> 10));
}

// ---- the step loop ---------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) float il_lds_float;
__device__ __forceinline__ float il_ld(unsigned a) { return *reinterpret_cast<const il_lds_float*>((uintptr_t)a); }
__device__ __forceinline__ void il_st(unsigned a, float v) { *reinterpret_cast<il_lds_float*>((uintptr_t)a) = v; }

// One workgroup per feature column c.  xT / cT / yT / sT are column-major [d][ldT] (ldT >= RS * 1024).
//   TRANS = false:  K steps  v <- A_II v + c  from v = x_I                                           (cT given)
//   TRANS = true :  h_K = M^K h_0 (M = the plan's operator: A_II^T) and  sT = h_0 + ... + h_{K-1}
// A step: (1a) every thread walks its run of the plan -- gather, multiply, add, store the running sum where the entry
// says (a finished row's word / the dump word / the run's P or L word); barrier; (1b) the threads whose run finishes a
// row begun earlier add the pieces in run order; barrier; (2) every row's owner adds the diagonal term and c;
// barrier.
template <bool TRANS>
__global__ void __launch_bounds__(IL_TB)
k_il_lds(IlPlan P, int n_int, int RS, int K, const float* __restrict__ xT, const float* __restrict__ cT, int64_t ldT,
         float* __restrict__ yT, float* __restrict__ sT) {
    extern __shared__ __attribute__((aligned(16))) char il_lds[];
    const int c = blockIdx.x, t = threadIdx.x;
    const int w = t >> 6, lane = t & 63;
    const unsigned bufw = (unsigned)(IL_HEAD + ((RS + 3) & ~3) * IL_TB);     // words per buffer: rows per thread rounded up to 4
    const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)il_lds;
    unsigned cur = base, nxt = base + bufw * 4u;
    uint32_t pk[IL_E];
    float pw[IL_E];
    {
        const uint32_t* kp = P.pk + ((size_t)w * IL_E) * 64 + lane;
        const float* wp = P.pw + ((size_t)w * IL_E) * 64 + lane;
#pragma unroll
        for (int e = 0; e < IL_E; ++e) { pk[e] = kp[(size_t)e * 64]; pw[e] = wp[(size_t)e * 64]; }
    }
    const int wm = __builtin_amdgcn_readfirstlane((int)P.wmax[w]);
    const uint32_t am = P.actm[t];
    const uint32_t ld = P.lead[t];
    float dg[IL_RS], cc[IL_RS];
    const float* xc = xT + (int64_t)c * ldT;
    const float* ccol = TRANS ? nullptr : cT + (int64_t)c * ldT;
#pragma unroll
    for (int s = 0; s < IL_RS; ++s) {
        dg[s] = 0.f; cc[s] = 0.f;
        if (s < ((RS + 3) & ~3)) {
            const int row = t + IL_TB * s;
            const bool live = row < n_int;
            dg[s] = live ? P.diag[row] : 0.f;
            const float a = live ? xc[row] : 0.f;
            if (!TRANS) cc[s] = live ? ccol[row] : 0.f;
            il_st(cur + (unsigned)(IL_HEAD + row) * 4u, a);
            il_st(nxt + (unsigned)(IL_HEAD + row) * 4u, 0.f);
        }
    }
    if (t == 0) { il_st(cur, 0.f); il_st(nxt, 0.f); }                        // the zero word of each buffer
    __syncthreads();
    const int RS4 = (RS + 3) & ~3;
    for (int step = 0; step < K; ++step) {
        float acc = 0.f;
        // the plan in groups of four entries: ONE wave-uniform test per group, so that a group's four gathers are issued
        // back to back ahead of their dependent chain (an entry beyond the wave's longest run reads the zero word and
        // stores to the lane's dump word: harmless) -- one test per entry left every gather's LDS latency exposed
        // (k_il_lds 48 us at K = 10, ~4 us per step, against ~2 us of LDS and VALU work)
#pragma unroll
        for (int e0 = 0; e0 < IL_E; e0 += 4) {
            if (e0 < wm) {
                float xv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) xv[u] = e0 + u < IL_E ? il_ld(cur + ((pk[e0 + u < IL_E ? e0 + u : 0] & 0xffffu) << 2)) : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (e0 + u < IL_E) {
                        const int e = e0 + u;
                        acc = __fadd_rn(acc, __fmul_rn(pw[e], xv[u]));
                        const unsigned st = pk[e] >> 16;
                        il_st(nxt + (st << 2), acc);                         // a row's word, the run's P / L word, or the lane's dump word
                        acc = st < IL_PW ? acc : 0.f;                        // the row continues / something new starts
                    }
                }
            }
        }
        __syncthreads();
        if (ld) {                                                            // this run finishes a row begun `np` runs earlier
            const unsigned np = ld >> 16;
            float v = 0.f;
            for (unsigned k = np; k >= 1; --k) v = __fadd_rn(v, il_ld(nxt + (IL_PW + (unsigned)t - k) * 4u));
            v = __fadd_rn(v, il_ld(nxt + (IL_LW + (unsigned)t) * 4u));
            il_st(nxt + ((ld & 0xffffu) << 2), v);
        }
        __syncthreads();
        // the owner pass, two rows per wave-uniform test (a row beyond RS inside the last group: zero diagonal, zero c,
        // never gathered -- its word exists, the buffers are sized for RS rounded up to 4 rows per thread); four rows per
        // test cost a spilled register
#pragma unroll
        for (int s0 = 0; s0 < IL_RS; s0 += 2) {
            if (s0 < RS4) {
                float a[2], o[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned ra = (unsigned)(IL_HEAD + t + IL_TB * (s0 + u)) * 4u;
                    a[u] = il_ld(cur + ra);
                    o[u] = il_ld(nxt + ra);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int sidx = s0 + u;
                    const unsigned ra = (unsigned)(IL_HEAD + t + IL_TB * sidx) * 4u;
                    const float ov = ((am >> sidx) & 1u) ? o[u] : 0.f;
                    float v = __fadd_rn(ov, __fmul_rn(dg[sidx], a[u]));
                    if (TRANS) cc[sidx] = __fadd_rn(cc[sidx], a[u]);
                    else v = __fadd_rn(v, cc[sidx]);
                    il_st(nxt + ra, v);
                }
            }
        }
        __syncthreads();
        const unsigned sw = cur; cur = nxt; nxt = sw;
    }
    float* yc = yT + (int64_t)c * ldT;
    float* sc = TRANS ? sT + (int64_t)c * ldT : nullptr;
#pragma unroll
    for (int s = 0; s < IL_RS; ++s) {
        if (s < RS) {
            const int row = t + IL_TB * s;
            yc[row] = il_ld(cur + (unsigned)(IL_HEAD + row) * 4u);
            if (TRANS) sc[row] = cc[s];
        }
    }
}

// ---- row-major <-> column-major around it -----------------------------------------------------------------------------
// Forward prologue: for a tile of 32 interior rows, c = A_IL x_L (the leaf columns' contribution: the plain row walk of
// k_spmm_range restricted to columns >= n_int, same order) and the rows of x themselves, both written column-major.
__global__ void __launch_bounds__(256)
k_il_prep(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, const float* __restrict__ val,
          int n_int, int d, const float* __restrict__ x, float* __restrict__ xT, float* __restrict__ cT, int64_t ldT) {
    __shared__ float tx[IL_TILE][IL_MAX_D + 1];
    __shared__ float tc[IL_TILE][IL_MAX_D + 1];
    const int row0 = blockIdx.x * IL_TILE;
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31;          // 8 lane groups of 32; lane l owns columns 4l .. 4l+3
    const int c4 = l * 4;
    const bool col_ok = c4 < d;
    for (int rr = g; rr < IL_TILE; rr += 8) {
        const int row = row0 + rr;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        float own[4] = {0.f, 0.f, 0.f, 0.f};
        if (row < n_int) {
            const int32_t start = rowptr[row], end = rowptr[row + 1];
            for (int32_t b = start; b < end; b += 32) {
                const int32_t k = b + l;
                const int32_t my_col = k < end ? colidx[k] : 0;
                const float my_val = k < end ? val[k] : 0.f;
                const int cnt = min(32, end - b);
                int e = 0;
                for (; e + 4 <= cnt; e += 4) {
                    float4 xv[4];
                    float wv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int32_t cu = __shfl(my_col, e + u, 32);
                        wv[u] = __shfl(my_val, e + u, 32);
                        xv[u] = (col_ok && cu >= n_int) ? *reinterpret_cast<const float4*>(x + (int64_t)cu * d + c4)
                                                        : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc[0] = __fadd_rn(acc[0], __fmul_rn(wv[u], xv[u].x));
                        acc[1] = __fadd_rn(acc[1], __fmul_rn(wv[u], xv[u].y));
                        acc[2] = __fadd_rn(acc[2], __fmul_rn(wv[u], xv[u].z));
                        acc[3] = __fadd_rn(acc[3], __fmul_rn(wv[u], xv[u].w));
                    }
                }
                for (; e < cnt; ++e) {
                    const int32_t cu = __shfl(my_col, e, 32);
                    const float wv = __shfl(my_val, e, 32);
                    if (col_ok && cu >= n_int) {
                        const float4 xv = *reinterpret_cast<const float4*>(x + (int64_t)cu * d + c4);
                        acc[0] = __fadd_rn(acc[0], __fmul_rn(wv, xv.x));
                        acc[1] = __fadd_rn(acc[1], __fmul_rn(wv, xv.y));
                        acc[2] = __fadd_rn(acc[2], __fmul_rn(wv, xv.z));
                        acc[3] = __fadd_rn(acc[3], __fmul_rn(wv, xv.w));
                    }
                }
            }
            if (col_ok) {
                const float4 v = *reinterpret_cast<const float4*>(x + (int64_t)row * d + c4);
                own[0] = v.x; own[1] = v.y; own[2] = v.z; own[3] = v.w;
            }
        }
        if (col_ok) {
#pragma unroll
            for (int v = 0; v < 4; ++v) { tc[rr][c4 + v] = acc[v]; tx[rr][c4 + v] = own[v]; }
        }
    }
    __syncthreads();
    const int r = threadIdx.x & 31;
    for (int col = threadIdx.x >> 5; col < d; col += 8) {
        xT[(int64_t)col * ldT + row0 + r] = tx[r][col];
        cT[(int64_t)col * ldT + row0 + r] = tc[r][col];
    }
}

// Column-major [d][ldT] tiles back to row-major rows (+ bias); with NSRC = 2 blockIdx.y picks the matrix.
__device__ __forceinline__ void il_tile_out(const float* __restrict__ srcT, int64_t ldT, float* __restrict__ dst, int row0,
                                            int n_rows, int d, const float* __restrict__ bias, float (*tile)[IL_MAX_D + 1]) {
    const int r = threadIdx.x & 31;
    for (int col = threadIdx.x >> 5; col < d; col += 8) tile[r][col] = srcT[(int64_t)col * ldT + row0 + r];
    __syncthreads();
    const int q = d >> 2;
    for (int idx = threadIdx.x; idx < IL_TILE * q; idx += 256) {
        const int rr = idx / q, c4 = (idx - rr * q) * 4;
        if (row0 + rr >= n_rows) continue;
        float4 v = make_float4(tile[rr][c4], tile[rr][c4 + 1], tile[rr][c4 + 2], tile[rr][c4 + 3]);
        if (bias) {
            v.x = __fadd_rn(v.x, bias[c4]); v.y = __fadd_rn(v.y, bias[c4 + 1]);
            v.z = __fadd_rn(v.z, bias[c4 + 2]); v.w = __fadd_rn(v.w, bias[c4 + 3]);
        }
        *reinterpret_cast<float4*>(dst + (int64_t)(row0 + rr) * d + c4) = v;
    }
}

// Forward epilogue in one launch: blocks [0, nb_int) bring the interior rows back (+ bias), the others copy the leaf
// rows  y[row] = x[row] (+ bias).
__global__ void __launch_bounds__(256)
k_il_finish(const float* __restrict__ yT, int64_t ldT, int n_int, int64_t n_rows, int d, const float* __restrict__ x,
            float* __restrict__ y, const float* __restrict__ bias, int nb_int) {
    __shared__ float tile[IL_TILE][IL_MAX_D + 1];
    if ((int)blockIdx.x < nb_int) {
        il_tile_out(yT, ldT, y, blockIdx.x * IL_TILE, n_int, d, bias, tile);
        return;
    }
    const int q = d >> 2;
    const int64_t total = (n_rows - n_int) * q;
    const int64_t stride = (int64_t)(gridDim.x - nb_int) * 256;
    for (int64_t k = (int64_t)(blockIdx.x - nb_int) * 256 + threadIdx.x; k < total; k += stride) {
        const int64_t rr = n_int + k / q;
        const int c4 = (int)(k % q) * 4;
        float4 v = *reinterpret_cast<const float4*>(x + rr * d + c4);
        if (bias) {
            v.x = __fadd_rn(v.x, bias[c4]); v.y = __fadd_rn(v.y, bias[c4 + 1]);
            v.z = __fadd_rn(v.z, bias[c4 + 2]); v.w = __fadd_rn(v.w, bias[c4 + 3]);
        }
        *reinterpret_cast<float4*>(y + rr * d + c4) = v;
    }
}

// The same epilogue with the activation that follows every conv layer (a2gnn_base.py:135-138: relu, then inverted dropout)
// applied on the way out: y0 = drop_site0(relu(v)), and -- when y1 is given -- y1 = drop_site1(relu(v)), a second,
// independent draw of the same pre-activation (the trainer's two passes over one shared layer-0 output).  Keep-bits in the
// format of gda_dropout.h on the row-major index of the [n_rows, d] result -- the values relu_dropout(y) would produce
// from this launch's result.  p <= 0: plain relu.  The pre-activation is never stored: the backward pass needs y > 0
// only (gda_relu_dropout_bwd_f32).

__device__ __forceinline__ void il_act_store(float4 v, int64_t row, int c4, int d, float* __restrict__ y0, float* __restrict__ y1,
                                             const GdaAct& a, uint64_t st, uint32_t thresh) {
    const int64_t off = row * d + c4;
    float4 o0, o1;
    if (a.p > 0.f) {
        uint32_t r[4];
        dropout_draw(a.seed, st, a.site0, (uint64_t)(off >> 2), r);
        o0 = relu_keep(v, r, thresh, a.scale);
        if (y1) {
            dropout_draw(a.seed, st, a.site1, (uint64_t)(off >> 2), r);
            o1 = relu_keep(v, r, thresh, a.scale);
        }
    } else {
        o0 = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        // relu as torch writes it: NaN stays NaN (fmaxf would drop it)
        o0.x = v.x != v.x ? v.x : o0.x; o0.y = v.y != v.y ? v.y : o0.y; o0.z = v.z != v.z ? v.z : o0.z; o0.w = v.w != v.w ? v.w : o0.w;
        o1 = o0;
    }
    *reinterpret_cast<float4*>(y0 + off) = o0;
    if (y1) *reinterpret_cast<float4*>(y1 + off) = o1;
}

__global__ void __launch_bounds__(256)
k_il_finish_act(const float* __restrict__ yT, int64_t ldT, int n_int, int64_t n_rows, int d, const float* __restrict__ x,
                float* __restrict__ y0, float* __restrict__ y1, const float* __restrict__ bias, int nb_int, GdaAct a) {
    __shared__ float tile[IL_TILE][IL_MAX_D + 1];
    const uint64_t st = a.p > 0.f ? (uint64_t)a.step[0] : 0;
    const uint32_t thresh = dropout_thresh(a.p);
    const int q = d >> 2;
    if ((int)blockIdx.x < nb_int) {
        const int row0 = blockIdx.x * IL_TILE;
        const int r = threadIdx.x & 31;
        for (int col = threadIdx.x >> 5; col < d; col += 8) tile[r][col] = yT[(int64_t)col * ldT + row0 + r];
        __syncthreads();
        for (int idx = threadIdx.x; idx < IL_TILE * q; idx += 256) {
            const int rr = idx / q, c4 = (idx - rr * q) * 4;
            if (row0 + rr >= n_int) continue;
            float4 v = make_float4(tile[rr][c4], tile[rr][c4 + 1], tile[rr][c4 + 2], tile[rr][c4 + 3]);
            if (bias) {
                v.x = __fadd_rn(v.x, bias[c4]); v.y = __fadd_rn(v.y, bias[c4 + 1]);
                v.z = __fadd_rn(v.z, bias[c4 + 2]); v.w = __fadd_rn(v.w, bias[c4 + 3]);
            }
            il_act_store(v, row0 + rr, c4, d, y0, y1, a, st, thresh);
        }
        return;
    }
    const int64_t total = (n_rows - n_int) * q;
    const int64_t stride = (int64_t)(gridDim.x - nb_int) * 256;
    for (int64_t k = (int64_t)(blockIdx.x - nb_int) * 256 + threadIdx.x; k < total; k += stride) {
        const int64_t rr = n_int + k / q;
        const int c4 = (int)(k % q) * 4;
        float4 v = *reinterpret_cast<const float4*>(x + rr * d + c4);
        if (bias) {
            v.x = __fadd_rn(v.x, bias[c4]); v.y = __fadd_rn(v.y, bias[c4 + 1]);
            v.z = __fadd_rn(v.z, bias[c4 + 2]); v.w = __fadd_rn(v.w, bias[c4 + 3]);
        }
        il_act_store(v, rr, c4, d, y0, y1, a, st, thresh);
    }
}

// Transposed epilogue: h_K -> the interior rows of the result, the summed step inputs -> a row-major scratch.
__global__ void __launch_bounds__(256)
k_il_untranspose2(const float* __restrict__ aT, float* __restrict__ a, const float* __restrict__ bT, float* __restrict__ b,
                  int64_t ldT, int n_int, int d) {
    __shared__ float tile[IL_TILE][IL_MAX_D + 1];
    il_tile_out(blockIdx.y ? bT : aT, ldT, blockIdx.y ? b : a, blockIdx.x * IL_TILE, n_int, d, nullptr, tile);
}

// Transposed prologue: the interior rows of the incoming gradient, column-major.
__global__ void __launch_bounds__(256)
k_il_transpose_in(const float* __restrict__ x, int n_int, int d, float* __restrict__ xT, int64_t ldT) {
    __shared__ float tile[IL_TILE][IL_MAX_D + 1];
    const int row0 = blockIdx.x * IL_TILE;
    const int q = d >> 2;
    for (int idx = threadIdx.x; idx < IL_TILE * q; idx += 256) {
        const int rr = idx / q, c4 = (idx - rr * q) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row0 + rr < n_int) v = *reinterpret_cast<const float4*>(x + (int64_t)(row0 + rr) * d + c4);
        tile[rr][c4] = v.x; tile[rr][c4 + 1] = v.y; tile[rr][c4 + 2] = v.z; tile[rr][c4 + 3] = v.w;
    }
    __syncthreads();
    const int r = threadIdx.x & 31;
    for (int col = threadIdx.x >> 5; col < d; col += 8) xT[(int64_t)col * ldT + row0 + r] = tile[r][col];
}

inline int64_t il_ldT(int64_t n_int) { return gda_cdiv(n_int, IL_TB) * IL_TB; }

}  // namespace

extern "C" int gda_interior_max_rows(void) { return IL_MAX_ROWS; }
extern "C" int gda_interior_max_width(void) { return IL_MAX_D; }
extern "C" size_t gda_interior_plan_bytes(void) { return IL_PLAN_BYTES; }

extern "C" size_t gda_interior_kstep_lds_workspace_bytes(int64_t n_int, int64_t d) {
    if (n_int <= 0 || d <= 0 || n_int > IL_MAX_ROWS || d > IL_MAX_D) return 0;
    return (size_t)(3 * d * il_ldT(n_int) + n_int * d) * sizeof(float);
}

// Build the register program of one direction of a sampled batch's normalised adjacency (rows [0, *n_int_dev) are the
// interior rows) on the device: three small capacity-sized launches, no host read-back.  status_dev[0] receives the
// plan's verdict (see above; status_dev[1] the number of off-diagonal interior entries): int64[2] on the device; the caller
// reads it whenever it reads the batch's sizes.
extern "C" int gda_interior_plan_build(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                       const int64_t* n_int_dev, void* plan, size_t plan_bytes, int64_t* status_dev,
                                       gda_stream_t stream) {
    if (!rowptr || !colidx || !val || !n_int_dev || !plan || !status_dev) return GDA_E_NULL;
    if (plan_bytes < IL_PLAN_BYTES) return GDA_E_WORKSPACE;
    if ((uintptr_t)plan % 16) return GDA_E_SIZE;
    char* p = static_cast<char*>(plan);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* pk = reinterpret_cast<uint32_t*>(p);
    float* pw = reinterpret_cast<float*>(p + IL_OFF_PW);
    float* diag = reinterpret_cast<float*>(p + IL_OFF_DIAG);
    uint32_t* actm = reinterpret_cast<uint32_t*>(p + IL_OFF_ACT);
    uint32_t* lead = reinterpret_cast<uint32_t*>(p + IL_OFF_LEAD);
    uint32_t* wmax = reinterpret_cast<uint32_t*>(p + IL_OFF_WMAX);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(p + IL_OFF_CNT);
    uint32_t* rowp = reinterpret_cast<uint32_t*>(p + IL_OFF_ROWP);
    constexpr unsigned nb = IL_MAX_ROWS / 256;
    k_il_count<<<nb, 256, 0, s>>>(rowptr, colidx, val, n_int_dev, diag, cnt);
    GDA_LAUNCH_CHECK();
    k_il_scan<<<1, IL_TB, 0, s>>>(n_int_dev, cnt, rowp, pk, pw, actm, lead, wmax, status_dev);
    GDA_LAUNCH_CHECK();
    k_il_entries<<<nb, 256, 0, s>>>(rowptr, colidx, val, n_int_dev, cnt, rowp, status_dev, pk, pw, actm, lead);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}

// The K steps of gda_spmm_csr_interior_kstep_f32 with ONE launch for the step loop (plan = the device plan of THIS
// direction's CSR, built by gda_interior_plan_build with a verdict > 0).  x, y: [n_rows, d] row-major, contiguous;
// d % 4 == 0, d <= gda_interior_max_width(); 0 < n_int <= gda_interior_max_rows().  Launches: forward 3 (leaf
// contribution + transposition | step loop | interior rows back + leaf copy), transposed 4 (transposition | step loop |
// two matrices back | leaf rows).  Same sums as the hoisted launch chain (bit for bit when every row's diagonal entry is
// the last of its row, as in this library's normalised CSRs).
extern "C" int gda_interior_kstep_lds_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                          int64_t n_rows, int64_t n_int, int64_t d, int K, int transposed,
                                          const void* plan, const float* x, float* y, const float* bias,
                                          void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (K < 1 || n_int <= 0 || n_int > n_rows || n_int > IL_MAX_ROWS || d <= 0 || d > IL_MAX_D || d % 4) return GDA_E_SIZE;
    if (n_rows >= INT32_MAX) return GDA_E_SIZE;
    if (!rowptr || !colidx || !val || !plan || !x || !y || !workspace) return GDA_E_NULL;
    if (x == y) return GDA_E_ALIAS;
    if (transposed && bias) return GDA_E_UNSUPPORTED;
    if (((uintptr_t)x % 16) || ((uintptr_t)y % 16) || ((uintptr_t)workspace % 16)) return GDA_E_SIZE;
    if (workspace_bytes < gda_interior_kstep_lds_workspace_bytes(n_int, d)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ldT = il_ldT(n_int);
    const int RS = (int)(ldT / IL_TB);
    float* aT = static_cast<float*>(workspace);          // forward: x^T   | transposed: g^T
    float* bT = aT + d * ldT;                             // forward: c^T   | transposed: (sum of the step inputs)^T
    float* oT = bT + d * ldT;                             // the step loop's result, column-major
    float* sacc = oT + d * ldT;                           // transposed: the summed step inputs, row-major [n_int, d]
    const IlPlan P = il_plan(plan);
    const int ni = (int)n_int, di = (int)d;
    const unsigned nb_int = (unsigned)gda_cdiv(n_int, IL_TILE);
    const size_t lds = (size_t)2 * (IL_HEAD + (size_t)((RS + 3) & ~3) * IL_TB) * sizeof(float);
    if (!transposed) {
        k_il_prep<<<nb_int, 256, 0, s>>>(rowptr, colidx, val, ni, di, x, aT, bT, ldT);
        GDA_LAUNCH_CHECK();
        GDA_LDS_ATTR_ONCE(k_il_lds<false>, 160 * 1024);
        k_il_lds<false><<<(unsigned)d, IL_TB, lds, s>>>(P, ni, RS, K, aT, bT, ldT, oT, nullptr);
        GDA_LAUNCH_CHECK();
        const int64_t leaf4 = (n_rows - n_int) * (d / 4);
        int64_t nb_leaf = gda_cdiv(leaf4, 256);
        if (nb_leaf > 256 * 16) nb_leaf = 256 * 16;
        k_il_finish<<<(unsigned)(nb_int + nb_leaf), 256, 0, s>>>(oT, ldT, ni, n_rows, di, x, y, bias, (int)nb_int);
        GDA_LAUNCH_CHECK();
        return GDA_OK;
    }
    k_il_transpose_in<<<nb_int, 256, 0, s>>>(x, ni, di, aT, ldT);
    GDA_LAUNCH_CHECK();
    GDA_LDS_ATTR_ONCE(k_il_lds<true>, 160 * 1024);
    k_il_lds<true><<<(unsigned)d, IL_TB, lds, s>>>(P, ni, RS, K, aT, nullptr, ldT, oT, bT);
    GDA_LAUNCH_CHECK();
    k_il_untranspose2<<<dim3(nb_int, 2), 256, 0, s>>>(oT, y, bT, sacc, ldT, ni, di);
    GDA_LAUNCH_CHECK();
    const int64_t n_leaf = n_rows - n_int;
    if (n_leaf == 0) return GDA_OK;
    // leaves of the transposed operator: interior columns read the summed step inputs, the self loop reads x
    return dispatch_range(rowptr, colidx, val, n_int, n_leaf, d, sacc, d, x, d, (int32_t)n_int, y, d, nullptr, nullptr, 0, s);
}

// Forward K steps of gda_interior_kstep_lds_f32 with the conv layer's activation in the epilogue (k_il_finish_act):
//   y0 = dropout_{site0}(relu(A^K x + bias)),  y1 (may be NULL) = dropout_{site1}(relu(same)) -- the launch count of the
// plain call (3), one activation launch (two with y1) and one [n_rows, d] round trip through HBM fewer.  seed / step_dev /
// sites as gda_relu_dropout_fwd_f32 takes them; p <= 0: relu only (step_dev is not read).
extern "C" int gda_interior_kstep_lds_act_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                              int64_t n_rows, int64_t n_int, int64_t d, int K, const void* plan,
                                              const float* x, float* y0, float* y1, const float* bias,
                                              float p, uint64_t seed, const int64_t* step_dev, uint32_t site0, uint32_t site1,
                                              void* workspace, size_t workspace_bytes, gda_stream_t stream) {
    if (K < 1 || n_int <= 0 || n_int > n_rows || n_int > IL_MAX_ROWS || d <= 0 || d > IL_MAX_D || d % 4) return GDA_E_SIZE;
    if (n_rows >= INT32_MAX || !(p < 1.f)) return GDA_E_SIZE;
    if (!rowptr || !colidx || !val || !plan || !x || !y0 || !workspace || (p > 0.f && !step_dev)) return GDA_E_NULL;
    if (x == y0 || x == y1 || (y1 && y0 == y1)) return GDA_E_ALIAS;
    if (((uintptr_t)x % 16) || ((uintptr_t)y0 % 16) || ((uintptr_t)y1 % 16) || ((uintptr_t)workspace % 16)) return GDA_E_SIZE;
    if (workspace_bytes < gda_interior_kstep_lds_workspace_bytes(n_int, d)) return GDA_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ldT = il_ldT(n_int);
    const int RS = (int)(ldT / IL_TB);
    float* aT = static_cast<float*>(workspace);
    float* bT = aT + d * ldT;
    float* oT = bT + d * ldT;
    const IlPlan P = il_plan(plan);
    const int ni = (int)n_int, di = (int)d;
    const unsigned nb_int = (unsigned)gda_cdiv(n_int, IL_TILE);
    const size_t lds = (size_t)2 * (IL_HEAD + (size_t)((RS + 3) & ~3) * IL_TB) * sizeof(float);
    k_il_prep<<<nb_int, 256, 0, s>>>(rowptr, colidx, val, ni, di, x, aT, bT, ldT);
    GDA_LAUNCH_CHECK();
    GDA_LDS_ATTR_ONCE(k_il_lds<false>, 160 * 1024);
    k_il_lds<false><<<(unsigned)d, IL_TB, lds, s>>>(P, ni, RS, K, aT, bT, ldT, oT, nullptr);
    GDA_LAUNCH_CHECK();
    const int64_t leaf4 = (n_rows - n_int) * (d / 4);
    int64_t nb_leaf = gda_cdiv(leaf4, 256);
    if (nb_leaf > 256 * 16) nb_leaf = 256 * 16;
    const GdaAct a = gda_act(p, seed, step_dev, site0, site1);
    k_il_finish_act<<<(unsigned)(nb_int + nb_leaf), 256, 0, s>>>(oT, ldT, ni, n_rows, di, x, y0, y1, bias, (int)nb_int, a);
    GDA_LAUNCH_CHECK();
    return GDA_OK;
}
