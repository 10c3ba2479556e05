// kernel_ecdf.hpp -- llda_ecdf_totals / _keys / _walk kernels: every word's ECDF rank within every topic (on kernel_label.hpp's sort), and
//                    llda_frex_select_kernel / llda_frex_merge_kernel: the n best words of every topic by two such ranks, compared exactly
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_ecdf_ranks (include/llda_gibbs.h): rank[l][w] = how many candidate words have a value <= the word's in
// column first + l of a word-major float64 matrix -- the column's ECDF times the number of candidates Vc.  The value is the entry
// (mode 0) or the entry divided by the row's total (mode 1: the exclusivity phi_kw / sum_j phi_jw).
//
// Pass a, llda_ecdf_totals_kernel: one wavefront per word row, four rows per workgroup and round.  tot = sum64 over ALL K columns (the
//   rule of doc_model.hpp: lane j adds x[j], x[j + 64], ... from +0.0, then doc_tree<64>), whatever the batch of columns.  tot[w] keeps
//   the total of a candidate (cand[w] != 0 and 0 < tot < inf) and +0.0 for any other word: one array is the total and the flag.
// Pass b, llda_ecdf_keys_kernel: llda_label_keys_kernel's 64 x 64 tile (words x columns) through LDS; the reads run along a matrix
//   row, the writes along a column's key row.  The tile keeps the VALUE (a -0.0 must reach the value output as one); the key is made
//   on the way out: rank_key(v), payload word << 1.  A candidate's v is never a NaN (its row sums to a finite number, so every
//   entry is finite, and finite / positive finite is no NaN), so its key is below RANK_KEY_PAD.  Any other word gets RANK_KEY_PAD
//   with its own payload, the padding RANK_KEY_PAD with LABEL_PAY_PAD: the candidates sort to the front, value descending, then the
//   other words, then the padding.  Grid (Vp / 64, ceil(n_labels / 64)), Vp = V rounded up to the chunk.
// Pass c: llda_label_sort_kernel and llda_label_merge_kernel (kernel_label.hpp) as they are, on a LabelParams that names these arrays.
// Pass d, llda_ecdf_walk_kernel: one workgroup per column.  Vc is the first position whose key is RANK_KEY_PAD (a binary search; the
//   same number in every column).  The sorted row is read in tiles of LABEL_TILE positions, eight per thread; a position starts a
//   tie group when its key differs from the key before it.  One max-scan over the workgroup gives every thread the last start
//   before its positions; between tiles the workgroup carries the start of the open group, so a group may straddle any tile, run
//   or chunk boundary.  A member of the group that starts at position g (value descending) has Vc - g candidates at or below it:
//   rank[l][word] = Vc - g, one scattered 4-byte store per position; the positions from Vc on store 0.
// Integers throughout, and one IEEE division per element in mode 1: nothing depends on the chunk, the batch or the geometry.
// ---------------------------------------------------------------------------------------------
constexpr int ECDF_WAVES = 4;
constexpr uint64_t ECDF_QNAN = 0x7FF8000000000000ull;

struct EcdfParams {
    const double *mat;
    const uint8_t *cand;
    int64_t V, ld, Vp;
    int32_t K, first, n_labels, mode;
    double *tot;                                          // [V]: a candidate's total, +0.0 for any other word
    uint64_t *key_a;                                      // [n_labels][Vp]: the first of the sort's four arrays
    uint32_t *pay_a;
    const uint64_t *key_sorted;                           // whichever of the sort's arrays the last merge level wrote
    const uint32_t *pay_sorted;
    int32_t *rank;
    double *value;
    int64_t *n_cand;
};

__global__ void __launch_bounds__(ECDF_WAVES * 64) llda_ecdf_totals_kernel(const EcdfParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t w = (int64_t)blockIdx.x * ECDF_WAVES + wave; w < P.V; w += (int64_t)gridDim.x * ECDF_WAVES) {
        const double *row = P.mat + w * P.ld;
        double part = 0.0;
#pragma unroll 4
        for (int k = lane; k < P.K; k += 64) part = part + row[k];
        const double tot = doc_tree<64>(part);            // (every lane holds it)
        const bool is_cand = (!P.cand || P.cand[w] != 0) && tot > 0.0 && tot < __builtin_inf();
        if (lane == 0) P.tot[w] = is_cand ? tot : 0.0;
    }
}

__global__ void __launch_bounds__(256) llda_ecdf_keys_kernel(const EcdfParams P)
{
    __shared__ double t_val[64][65];                      // [word][column], one column of padding against bank conflicts
    const int tid = threadIdx.x, x = tid & 63, y = tid >> 6;
    const int64_t w0 = (int64_t)blockIdx.x * 64;
    const int l0 = (int)blockIdx.y * 64;
    const double qnan = __longlong_as_double((long long)ECDF_QNAN);
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {                        // lanes along a matrix row
        const int r = y + 4 * i;
        const int64_t w = w0 + r;
        const int l = l0 + x;
        double v = qnan;
        if (w < P.V && l < P.n_labels) {
            const double tot = P.tot[w];                  // (one address for the row's lanes)
            if (tot != 0.0) {
                v = P.mat[w * P.ld + P.first + l];
                if (P.mode) v = v / tot;
            }
        }
        t_val[r][x] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {                        // lanes along a column's key row
        const int c = y + 4 * i;
        const int l = l0 + c;
        const int64_t w = w0 + x;
        if (l < P.n_labels) {                             // (w < Vp: Vp is a multiple of 64)
            const int64_t at = (int64_t)l * P.Vp + w;
            const double v = t_val[x][c];
            const bool is_cand = w < P.V && P.tot[w] != 0.0;
            P.key_a[at] = is_cand ? rank_key((uint64_t)__double_as_longlong(v)) : RANK_KEY_PAD;
            P.pay_a[at] = w < P.V ? (uint32_t)w << 1 : LABEL_PAY_PAD;
            if (P.value && w < P.V) P.value[(int64_t)l * P.V + w] = v;
        }
    }
}

__global__ void __launch_bounds__(LABEL_WALK_NT) llda_ecdf_walk_kernel(const EcdfParams P)
{
    constexpr int NT = LABEL_WALK_NT;
    __shared__ int32_t s_b[2][NT];                        // scan: last group start + 1 (within the tile)
    __shared__ int64_t s_vc;
    const int tid = threadIdx.x;
    const int l = blockIdx.x;
    const int64_t V = P.V;
    const uint64_t *key = P.key_sorted + (int64_t)l * P.Vp;
    const uint32_t *pay = P.pay_sorted + (int64_t)l * P.Vp;
    int32_t *rank = P.rank + (int64_t)l * V;
    if (tid == 0) {                                       // Vc: the first position that holds no candidate
        int64_t lo = 0, hi = V;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (key[mid] != RANK_KEY_PAD) lo = mid + 1;
            else hi = mid;
        }
        s_vc = lo;
        if (l == 0 && P.n_cand) *P.n_cand = lo;
    }
    __syncthreads();
    const int64_t Vc = s_vc;
    int64_t carry = 0;                                    // the start of the group that is open at the tile's first position
    for (int64_t t0 = 0; t0 < V; t0 += LABEL_TILE) {
        const int own = tid * 8;
        const int64_t p0 = t0 + own;
        uint64_t k[9];                                    // k[e + 1]: the key of position p0 + e; k[0]: the one before
        k[0] = (p0 > 0 && p0 <= V) ? key[p0 - 1] : RANK_KEY_PAD;
#pragma unroll
        for (int e = 0; e < 8; ++e) k[e + 1] = p0 + e < V ? key[p0 + e] : RANK_KEY_PAD;
        uint32_t starts = 0;
        int last = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t pos = p0 + e;
            if (pos < V && (pos == 0 || k[e + 1] != k[e])) { starts |= 1u << e; last = own + e + 1; }
        }
        int vm = last, buf = 0;
        __syncthreads();                                  // (the previous tile's LDS is no longer read)
        s_b[0][tid] = vm;
        for (int off = 1; off < NT; off <<= 1) {
            __syncthreads();
            if (tid >= off) vm = max(vm, s_b[buf][tid - off]);
            buf ^= 1;
            s_b[buf][tid] = vm;
        }
        __syncthreads();
        const int prev = tid ? s_b[buf][tid - 1] : 0;     // 0: no group of this tile starts before the thread
        const int tile_last = s_b[buf][NT - 1];
        int64_t cur = prev ? t0 + prev - 1 : carry;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t pos = p0 + e;
            if (pos < V) {                                // (the first V positions hold the V words: their payloads are below 2 V)
                if ((starts >> e) & 1u) cur = pos;
                rank[pay[pos] >> 1] = pos < Vc ? (int32_t)(Vc - cur) : 0;
            }
        }
        if (tile_last) carry = t0 + tile_last - 1;        // (the same in every thread)
    }
}

// ---------------------------------------------------------------------------------------------
// llda_frex_select (include/llda_gibbs.h): the n best words of every column by the cost
//   c = s / re + (t - s) / rf = A / B,  A = s rf + (t - s) re,  B = re rf,
// ascending, then word id ascending -- FREX = 1 / (omega / F_e + (1 - omega) / F_f) descending with omega = s / t and F = rank / Vc.
// A <= 64 x 2^30 and B <= 2^60: A B' against A' B are 96-bit products, compared as unsigned __int128 -- integers only, so two words
// whose costs differ by one part in 2^60 are still told apart, which no double does.
//
// The shape of kernel_scored.hpp, turned: the ranks lie [n_labels][V], so the lanes of ONE wavefront run along a column's row of
// FREX_CHUNK words (coalesced 4-byte loads, four rounds in flight) and every lane keeps the best N of its words in a TopList
// (top_list.hpp) of (rf, re, word); the padding has re = 0 and loses against everything.  Then the wavefront pops the best head of
// its 64 lists n times (word ids are unique within a column) and leaves one partial list of n.
// llda_frex_merge_kernel: one wavefront per column, lanes over the partial lists, the same pop; its lanes below m look the probes up.
// ---------------------------------------------------------------------------------------------
constexpr int FREX_CHUNK = 16384;                        // words of a partial list
constexpr int FREX_UNROLL = 4;
constexpr uint32_t FREX_PAD_ID = 0xFFFFFFFFu;

struct FrexParams {
    const int32_t *rank_f, *rank_e, *probe;
    int64_t V, Vc, parts;
    int32_t n_labels, n, m, s, u, reserved;              // u = t - s
    int32_t *part;                                        // [n_labels][parts][3][n]: rf, re, word
    int32_t *top_idx, *top_rank_f, *top_rank_e, *probe_rank_f, *probe_rank_e;
};

// is (rf, re, w) before (rf2, re2, w2)?  re = 0 marks the padding
__device__ __forceinline__ bool frex_better(int s, int u, uint32_t rf, uint32_t re, uint32_t w, uint32_t rf2, uint32_t re2, uint32_t w2)
{
    if (re == 0) return false;
    if (re2 == 0) return true;
    const uint64_t A = (uint64_t)s * rf + (uint64_t)u * re, B = (uint64_t)re * rf;
    const uint64_t A2 = (uint64_t)s * rf2 + (uint64_t)u * re2, B2 = (uint64_t)re2 * rf2;
    const unsigned __int128 lhs = (unsigned __int128)A * B2, rhs = (unsigned __int128)A2 * B;
    return lhs < rhs || (lhs == rhs && w < w2);
}

// both ranks in 1 .. Vc
__device__ __forceinline__ bool frex_ranked(int32_t rf, int32_t re, int64_t Vc)
{
    return rf >= 1 && re >= 1 && rf <= Vc && re <= Vc;
}

// (rf, re, word) as a list entry: w[0 .. 2]; the order carries the two weights
struct FrexOrd {
    static constexpr int Q = 0, W = 3;
    typedef TopEntry<0, 3> E;
    int s, u;
    static __device__ __forceinline__ E entry(uint32_t rf, uint32_t re, uint32_t v) { return E{{0}, {rf, re, v}}; }
    __device__ __forceinline__ E pad() const { return entry(0, 0, FREX_PAD_ID); }
    __device__ __forceinline__ bool before(const E &a, const E &b) const { return frex_better(s, u, a.w[0], a.w[1], a.w[2], b.w[0], b.w[1], b.w[2]); }
    __device__ __forceinline__ bool same(const E &a, const E &b) const { return a.w[2] == b.w[2]; }
};

template <int N>
__global__ void __launch_bounds__(64) llda_frex_select_kernel(const FrexParams P)
{
    const int lane = threadIdx.x, l = blockIdx.y;
    const int64_t w0 = (int64_t)blockIdx.x * FREX_CHUNK;
    const int64_t w1 = w0 + FREX_CHUNK < P.V ? w0 + FREX_CHUNK : P.V;
    const int32_t *rf = P.rank_f + (int64_t)l * P.V, *re = P.rank_e + (int64_t)l * P.V;
    TopList<N, FrexOrd> L(FrexOrd{P.s, P.u});
    for (int64_t w = w0 + lane; w < w1; w += 64 * FREX_UNROLL) {
        int32_t a[FREX_UNROLL], b[FREX_UNROLL];
#pragma unroll
        for (int q = 0; q < FREX_UNROLL; ++q) {
            const int64_t ww = w + 64 * q;
            a[q] = ww < w1 ? rf[ww] : 0;
            b[q] = ww < w1 ? re[ww] : 0;
        }
#pragma unroll
        for (int q = 0; q < FREX_UNROLL; ++q) {
            const FrexOrd::E e = FrexOrd::entry((uint32_t)a[q], (uint32_t)b[q], (uint32_t)(w + 64 * q));
            if (frex_ranked(a[q], b[q], P.Vc) && L.admits(e)) L.insert(e);
        }
    }
    int32_t *out = P.part + ((int64_t)l * P.parts + blockIdx.x) * 3 * P.n;
    for (int i = 0; i < P.n; ++i) {
        const FrexOrd::E m = L.pop_wave();
        if (lane == 0) { out[i] = (int32_t)m.w[0]; out[P.n + i] = (int32_t)m.w[1]; out[2 * P.n + i] = (int32_t)m.w[2]; }
    }
}

template <int N>
__global__ void __launch_bounds__(64) llda_frex_merge_kernel(const FrexParams P)
{
    const int lane = threadIdx.x, l = blockIdx.x, n = P.n;
    TopList<N, FrexOrd> L(FrexOrd{P.s, P.u});
    for (int64_t part = lane; part < P.parts; part += 64) {
        const int32_t *in = P.part + ((int64_t)l * P.parts + part) * 3 * n;
        L.fold_sorted(n, [&](int j) { return FrexOrd::entry((uint32_t)in[j], (uint32_t)in[n + j], (uint32_t)in[2 * n + j]); });
    }
    for (int i = 0; i < n; ++i) {
        const FrexOrd::E m = L.pop_wave();
        if (lane == 0) {
            const bool real = m.w[1] != 0;
            const int64_t at = (int64_t)l * n + i;
            if (P.top_idx) P.top_idx[at] = real ? (int32_t)m.w[2] : -1;
            if (P.top_rank_f) P.top_rank_f[at] = real ? (int32_t)m.w[0] : 0;
            if (P.top_rank_e) P.top_rank_e[at] = real ? (int32_t)m.w[1] : 0;
        }
    }
    if (P.probe && lane < P.m) {
        const int64_t at = (int64_t)l * P.m + lane;
        const int32_t w = P.probe[at];
        int32_t a = 0, b = 0;
        if (w >= 0 && w < P.V) {
            a = P.rank_f[(int64_t)l * P.V + w];
            b = P.rank_e[(int64_t)l * P.V + w];
            if (!frex_ranked(a, b, P.Vc)) a = b = 0;
        }
        if (P.probe_rank_f) P.probe_rank_f[at] = a;
        if (P.probe_rank_e) P.probe_rank_e[at] = b;
    }
}

}  // namespace
