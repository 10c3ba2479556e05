// kernel_topwords.hpp -- llda_top_words_kernel / llda_top_words_merge_kernel: the n best words of every topic from n_kw
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_top_words (include/llda_gibbs.h): what topwords_per_topic (LabeledLDA.py:241-254) asks of phi, answered from the integer
// counts.  phi[k][v] = (n_kw[v][k] + beta) / den[k] is strictly increasing in the count for a fixed topic, and two different counts
// give numerators a relative 2^-40 or more apart (V*beta < 2^40), so they never round to one double: ranking by phi IS ranking by
// the count, and equal phi means equal counts.
//
// Key.  (count, word) becomes ONE 64-bit integer, (0x7fffffff - count) << 32 | word: it ascends as the count descends (compared as
// signed int32) and, among equal counts, as the word id ascends.  A single unsigned compare is the whole order; every key is unique;
// all ones is the padding (a word id never has bit 31 set).  The lists are TopLists (top_list.hpp) of this one 64-bit word.
//
// Pass 1, a bandwidth pass over V * KP * 4 bytes.  A thread owns one 16-byte chunk of the row -- four columns -- and keeps a list of
// N >= n keys per column.  The vocabulary is cut into chunks of LLDA_TOPW_CHUNK_ROWS rows, one workgroup per chunk and per 256 chunks
// of the row, so the grid fills the chip at KP = 512 too; where a row has fewer than 256 chunks, up to TOPW_MAX_PHASES rows share the
// workgroup (thread = row phase * cpr + chunk: the wavefront's loads stay one contiguous run) and each phase walks every rpb-th row of
// the chunk (topw_thread; kernel_scored.hpp walks the same way).  TOPW_UNROLL loads of a thread are in flight before the first is
// looked at.  After the first rows an insertion is rare, and a zero count never beats the zero of a lower word id.  Every (row chunk,
// phase) leaves its four lists in scratch.
//
// Pass 2 merges the partial lists of a column: one wavefront per POSITION of the row (positions of the padding return at once and
// their lists are never read), each lane folds the lists lane, lane + 64, ... into a list of its own, then n rounds take the
// best head of the 64 lanes.  The outputs are in reference topic order.  Nothing here rounds: the result does not depend on the
// geometry.
// ---------------------------------------------------------------------------------------------
constexpr int TOPW_UNROLL = 4;
constexpr int TOPW_MAX_PHASES = 4;                       // rows that share a workgroup when the row is short

struct TopwParams {
    const int4 *n_kw;
    int64_t V;
    int32_t cpr;                                          // chunks of a row (KP / 4)
    int32_t rpb;                                          // row phases of a workgroup
    int32_t n;
    int32_t KP, G, T, K;
    int64_t parts;                                        // partial lists per column: row chunks * rpb
    uint64_t *scratch;                                    // [parts][KP][n]
    int32_t *top_idx, *top_cnt;                           // [K][n] or NULL
    int32_t leaf_start[LLDA_MAX_WIDE_LEAVES], leaf_len[LLDA_MAX_WIDE_LEAVES];
};

constexpr uint64_t TOPW_PAD = 0xFFFFFFFFFFFFFFFFull;

// the key as a list entry: q[0]
struct TopwOrd {
    static constexpr int Q = 1, W = 0;
    typedef TopEntry<1, 0> E;
    static __device__ __forceinline__ E entry(uint64_t key) { return E{{key}, {0}}; }
    static __device__ __forceinline__ E entry(int32_t cnt, uint32_t v) { return entry(((uint64_t)(0x7FFFFFFFu - (uint32_t)cnt) << 32) | v); }
    __device__ __forceinline__ E pad() const { return entry(TOPW_PAD); }
    __device__ __forceinline__ bool before(const E &a, const E &b) const { return a.q[0] < b.q[0]; }
    __device__ __forceinline__ bool same(const E &a, const E &b) const { return a.q[0] == b.q[0]; }
};

// A thread of a row-chunk pass: its row phase lr, its column chunk c and the rows [r0, r1) of the workgroup's chunk.  False: no work.
__device__ __forceinline__ bool topw_thread(int rpb, int cpr, int64_t V, int &lr, int &c, int64_t &r0, int64_t &r1)
{
    const int tid = threadIdx.x;
    if (rpb > 1) { lr = tid / cpr; c = tid - lr * cpr; }
    else { lr = 0; c = (int)blockIdx.y * 256 + tid; }
    r0 = (int64_t)blockIdx.x * LLDA_TOPW_CHUNK_ROWS;
    r1 = r0 + LLDA_TOPW_CHUNK_ROWS < V ? r0 + LLDA_TOPW_CHUNK_ROWS : V;
    return lr < rpb && c < cpr;
}

template <int N>
__global__ void __launch_bounds__(256) llda_top_words_kernel(const TopwParams P)
{
    int lr, c;
    int64_t r0, r1;
    if (!topw_thread(P.rpb, P.cpr, P.V, lr, c, r0, r1)) return;
    TopList<N, TopwOrd> L[4];
    const int rpb = P.rpb, cpr = P.cpr;
    for (int64_t r = r0 + lr; r < r1; r += (int64_t)rpb * TOPW_UNROLL) {
        int4 v[TOPW_UNROLL];
#pragma unroll
        for (int u = 0; u < TOPW_UNROLL; ++u) {
            const int64_t rr = r + (int64_t)u * rpb;
            v[u] = rr < r1 ? P.n_kw[rr * cpr + c] : make_int4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < TOPW_UNROLL; ++u) {
            const int64_t rr = r + (int64_t)u * rpb;
            if (rr < r1) {
                const int32_t cnt[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const TopwOrd::E e = TopwOrd::entry(cnt[q], (uint32_t)rr);
                    if (L[q].admits(e)) L[q].insert(e);
                }
            }
        }
    }
    const int64_t part = (int64_t)blockIdx.x * rpb + lr;
    uint64_t *dst = P.scratch + ((part * P.KP) + 4 * (int64_t)c) * P.n;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < P.n) dst[q * P.n + j] = L[q].at(j).q[0];
}

template <int N>
__global__ void __launch_bounds__(64) llda_top_words_merge_kernel(const TopwParams P)
{
    const int pos = (int)blockIdx.x, lane = threadIdx.x;
    const int k = wide_topic_of(P.leaf_start, P.leaf_len, P.G, P.T, pos);
    if (k < 0) return;                                    // a position of the padding: its lists are never read
    const int n = P.n;
    TopList<N, TopwOrd> L;
    for (int64_t part = lane; part < P.parts; part += 64) {
        const uint64_t *src = P.scratch + (part * P.KP + pos) * n;
        L.fold_sorted(n, [&](int j) { return TopwOrd::entry(src[j]); });
    }
    for (int i = 0; i < n; ++i) {
        const uint64_t m = L.pop_wave().q[0];
        if (lane == 0) {
            const bool real = m != TOPW_PAD;
            if (P.top_idx) P.top_idx[(int64_t)k * n + i] = real ? (int32_t)(uint32_t)m : -1;
            if (P.top_cnt) P.top_cnt[(int64_t)k * n + i] = real ? (int32_t)(0x7FFFFFFFu - (uint32_t)(m >> 32)) : 0;
        }
    }
}

}  // namespace
