// kernel_scored.hpp -- llda_scored_words_kernel / llda_scored_merge_kernel: the n best words of every topic by a float64 score
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_scored_words (include/llda_gibbs.h): score[w][k] = P_a(x[w][k]) / wdiv[w], the n best words per topic.
// x is phi of the counts, computed in the pass as llda_readout_phi computes it (counts mode), or an entry of a word-major float64
// matrix (matrix mode).  P_a is a - 1 rounded multiplications, left to right; the division is the hardware's IEEE division; nothing
// is contracted (the translation unit is built with -ffp-contract=off).  Every output is therefore the result of the stated IEEE
// operations on ONE element, and the result does not depend on the geometry.
//
// Key.  A float score does not fit llda_top_words' single 64-bit integer: the key is 96 bits, (score, word), a TopList entry
// (top_list.hpp): the double's bits and the id.  a is better than b when a.score > b.score, or the scores compare equal (-0 == +0) and
// a.word < b.word.  NaN scores never enter a list (they are counted), so this is a total order over the entries of a column.  The
// padding is (-inf, all ones): a word id never has bit 31 set, so a real -inf beats it.
//
// Pass 1, the shape of llda_top_words_kernel (its geometry, thread decode and unroll depth) with TWO columns per thread instead of
// four: 2 * N * 3 = 96 list registers at N = 16.  One 8-byte load per row in counts mode, one 16-byte load in matrix mode (two 8-byte
// loads where the matrix is not 16-byte aligned or its leading dimension is odd).  wdiv[row] is the same address for every lane of
// a row phase.  Every (row chunk, phase) leaves its two lists and its two NaN counts in scratch: scores [parts][C][n], ids
// [parts][C][n], NaN counts [parts][C].
//
// Pass 2: one wavefront per column -- a device position in counts mode (the padding returns at once), a topic in matrix mode --
// folds the partial lists as llda_top_words_merge_kernel does and writes reference topic order.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t SCORED_PAD_ID = 0xFFFFFFFFu;
constexpr int SCORED_COUNTS = 0, SCORED_MATRIX = 1, SCORED_MATRIX_VEC = 2;

struct ScoredParams {
    const int2 *n_kw;                                     // counts mode: [V][KP / 2], else NULL
    const int32_t *n_k;
    const double *den;
    const double *mat;                                    // matrix mode: [V][ld]
    const double *wdiv;                                   // [V] or NULL
    int64_t V, ld;
    double beta, vbeta;
    int32_t cpr;                                          // column pairs of a row
    int32_t rpb;                                          // row phases of a workgroup
    int32_t n, a;
    int32_t C;                                            // columns of the scratch lists: 2 * cpr
    int32_t K, G, T;
    int64_t parts;                                        // partial lists per column: row chunks * rpb
    double *part_score;                                   // [parts][C][n]
    uint32_t *part_id;                                    // [parts][C][n]
    int32_t *part_nan;                                    // [parts][C]
    int32_t *top_idx;                                     // [K][n] or NULL
    double *top_score;                                    // [K][n] or NULL
    int32_t *n_nan;                                       // [K] or NULL
    int32_t leaf_start[LLDA_MAX_WIDE_LEAVES], leaf_len[LLDA_MAX_WIDE_LEAVES];
};

__device__ __forceinline__ bool scored_better(double s, uint32_t v, double t, uint32_t w)
{
    return s > t || (s == t && v < w);
}

// (score, word) as a list entry: q[0] the bits of the double, w[0] the word id
struct ScoredOrd {
    static constexpr int Q = 1, W = 1;
    typedef TopEntry<1, 1> E;
    static __device__ __forceinline__ double score(const E &e) { return __longlong_as_double((long long)e.q[0]); }
    static __device__ __forceinline__ E entry(double s, uint32_t v) { return E{{(uint64_t)__double_as_longlong(s)}, {v}}; }
    __device__ __forceinline__ E pad() const { return entry(-__builtin_inf(), SCORED_PAD_ID); }
    __device__ __forceinline__ bool before(const E &a, const E &b) const { return scored_better(score(a), a.w[0], score(b), b.w[0]); }
    __device__ __forceinline__ bool same(const E &a, const E &b) const { return a.w[0] == b.w[0]; }
};

// P_a(x): a - 1 multiplications, left to right, each rounded
__device__ __forceinline__ double scored_power(double x, int a)
{
    double p = x;
    for (int i = 1; i < a; ++i) p = p * x;
    return p;
}

template <int N>
__device__ __forceinline__ void scored_consider(TopList<N, ScoredOrd> &L, int &nan, double s, uint32_t v)
{
    const ScoredOrd::E e = ScoredOrd::entry(s, v);
    if (s != s) ++nan;
    else if (L.admits(e)) L.insert(e);
}

template <int N, int MODE>
__global__ void __launch_bounds__(256) llda_scored_words_kernel(const ScoredParams P)
{
    int lr, c;
    int64_t r0, r1;
    if (!topw_thread(P.rpb, P.cpr, P.V, lr, c, r0, r1)) return;
    TopList<N, ScoredOrd> L[2];
    int nan0 = 0, nan1 = 0;
    const int rpb = P.rpb, cpr = P.cpr, a = P.a;
    const bool divide = P.wdiv != nullptr;
    const bool second = MODE == SCORED_COUNTS || 2 * c + 1 < P.K;     // (matrix mode, odd K: the last thread has one column)
    double den0 = 1.0, den1 = 1.0;
    if (MODE == SCORED_COUNTS) {                           // the denominators of llda_readout_phi_kernel
        den0 = P.den ? P.den[2 * c] : (double)P.n_k[2 * c] + P.vbeta;
        den1 = P.den ? P.den[2 * c + 1] : (double)P.n_k[2 * c + 1] + P.vbeta;
    }
    for (int64_t r = r0 + lr; r < r1; r += (int64_t)rpb * TOPW_UNROLL) {
        double x0[TOPW_UNROLL], x1[TOPW_UNROLL], wd[TOPW_UNROLL];
        int2 cnt[TOPW_UNROLL];
#pragma unroll
        for (int u = 0; u < TOPW_UNROLL; ++u) {
            const int64_t rr = r + (int64_t)u * rpb;
            const bool in = rr < r1;
            x0[u] = x1[u] = 0.0;
            cnt[u] = make_int2(0, 0);
            if (MODE == SCORED_COUNTS) {
                if (in) cnt[u] = P.n_kw[rr * cpr + c];
            } else if (MODE == SCORED_MATRIX_VEC) {
                if (in) {
                    const double2 v = *reinterpret_cast<const double2 *>(P.mat + rr * P.ld + 2 * c);
                    x0[u] = v.x; x1[u] = v.y;
                }
            } else if (in) {
                x0[u] = P.mat[rr * P.ld + 2 * c];
                if (second) x1[u] = P.mat[rr * P.ld + 2 * c + 1];
            }
            wd[u] = !in ? 0.0 : (divide ? P.wdiv[rr] : 1.0);
        }
#pragma unroll
        for (int u = 0; u < TOPW_UNROLL; ++u) {
            const int64_t rr = r + (int64_t)u * rpb;
            if (wd[u] == 0.0) continue;                   // past the chunk, or a word that is not ranked (either sign of zero)
            if (MODE == SCORED_COUNTS) {
                x0[u] = ((double)cnt[u].x + P.beta) / den0;
                x1[u] = ((double)cnt[u].y + P.beta) / den1;
            }
            double s0 = scored_power(x0[u], a), s1 = scored_power(x1[u], a);
            if (divide) { s0 = s0 / wd[u]; s1 = s1 / wd[u]; }
            scored_consider<N>(L[0], nan0, s0, (uint32_t)rr);
            scored_consider<N>(L[1], nan1, s1, (uint32_t)rr);
        }
    }
    const int64_t part = (int64_t)blockIdx.x * rpb + lr;
    const int64_t col = part * P.C + 2 * (int64_t)c;
    double *ds = P.part_score + col * P.n;
    uint32_t *di = P.part_id + col * P.n;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < P.n) { ds[q * P.n + j] = ScoredOrd::score(L[q].at(j)); di[q * P.n + j] = L[q].at(j).w[0]; }
    P.part_nan[col] = nan0;
    P.part_nan[col + 1] = nan1;
}

template <int N>
__global__ void __launch_bounds__(64) llda_scored_merge_kernel(const ScoredParams P)
{
    const int col = (int)blockIdx.x, lane = threadIdx.x;
    const int k = P.n_kw ? wide_topic_of(P.leaf_start, P.leaf_len, P.G, P.T, col) : col;
    if (k < 0) return;                                    // a position of the padding: its lists are never read
    const int n = P.n;
    TopList<N, ScoredOrd> L;
    int nan = 0;
    for (int64_t part = lane; part < P.parts; part += 64) {
        const int64_t at = part * P.C + col;
        nan += P.part_nan[at];
        const double *ss = P.part_score + at * n;
        const uint32_t *si = P.part_id + at * n;
        L.fold_sorted(n, [&](int j) { return ScoredOrd::entry(ss[j], si[j]); });
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) nan += __shfl_xor(nan, off, 64);
    if (lane == 0 && P.n_nan) P.n_nan[k] = nan;
    for (int i = 0; i < n; ++i) {
        const ScoredOrd::E m = L.pop_wave();
        if (lane == 0) {
            const bool real = m.w[0] != SCORED_PAD_ID;
            if (P.top_idx) P.top_idx[(int64_t)k * n + i] = real ? (int32_t)m.w[0] : -1;
            if (P.top_score) P.top_score[(int64_t)k * n + i] = real ? ScoredOrd::score(m) : __longlong_as_double(0x7ff8000000000000ll);
        }
    }
}

}  // namespace
