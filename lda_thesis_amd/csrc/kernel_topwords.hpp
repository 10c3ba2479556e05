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
// all ones is the padding (a word id never has bit 31 set).
//
// Pass 1, a bandwidth pass over V * KP * 4 bytes.  A thread owns one 16-byte chunk of the row -- four columns -- and keeps a sorted
// list of N >= n keys per column in registers (N is a template argument: the lists are never indexed dynamically).  The vocabulary
// is cut into chunks of LLDA_TOPW_CHUNK_ROWS rows, one workgroup per chunk and per 256 chunks of the row, so the grid fills the chip
// at KP = 512 too; where a row has fewer than 256 chunks, up to TOPW_MAX_PHASES rows share the workgroup (thread = row phase * cpr +
// chunk: the wavefront's loads stay one contiguous run) and each phase walks every rpb-th row of the chunk.  TOPW_UNROLL loads of a
// thread are in flight before the first is looked at.  A key is inserted only when it beats the list's worst; after the first rows
// that is rare, and a zero count never beats the zero of a lower word id.  Every (row chunk, phase) leaves its four lists in scratch.
//
// Pass 2 merges the partial lists of a column: one wavefront per POSITION of the row (positions of the padding return at once and
// their lists are never read), each lane folds the lists lane, lane + 64, ... into a list of its own, then n rounds take the
// smallest head of the 64 lanes.  The outputs are in reference topic order.  Nothing here rounds: the result does not depend on the
// geometry.
// ---------------------------------------------------------------------------------------------
constexpr int TOPW_UNROLL = 4;
constexpr int TOPW_MAX_PHASES = 4;                       // rows that share a workgroup when the row is short
constexpr uint64_t TOPW_PAD = 0xFFFFFFFFFFFFFFFFull;

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

__device__ __forceinline__ uint64_t topw_key(int32_t cnt, uint32_t v)
{
    return ((uint64_t)(0x7FFFFFFFu - (uint32_t)cnt) << 32) | v;
}

// sorted insertion into registers: every L[j] takes its lower neighbour, the key, or stays
template <int N>
__device__ __forceinline__ void topw_insert(uint64_t (&L)[N], uint64_t key)
{
#pragma unroll
    for (int j = N - 1; j > 0; --j) L[j] = key < L[j - 1] ? L[j - 1] : (key < L[j] ? key : L[j]);
    L[0] = key < L[0] ? key : L[0];
}

template <int N>
__global__ void __launch_bounds__(256) llda_top_words_kernel(const TopwParams P)
{
    const int tid = threadIdx.x;
    int lr, c;
    if (P.rpb > 1) { lr = tid / P.cpr; c = tid - lr * P.cpr; }
    else { lr = 0; c = (int)blockIdx.y * 256 + tid; }
    if (lr >= P.rpb || c >= P.cpr) return;
    const int64_t r0 = (int64_t)blockIdx.x * LLDA_TOPW_CHUNK_ROWS;
    const int64_t r1 = r0 + LLDA_TOPW_CHUNK_ROWS < P.V ? r0 + LLDA_TOPW_CHUNK_ROWS : P.V;
    uint64_t L[4][N];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < N; ++j) L[q][j] = TOPW_PAD;
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
                const uint64_t k0 = topw_key(v[u].x, (uint32_t)rr), k1 = topw_key(v[u].y, (uint32_t)rr);
                const uint64_t k2 = topw_key(v[u].z, (uint32_t)rr), k3 = topw_key(v[u].w, (uint32_t)rr);
                if (k0 < L[0][N - 1]) topw_insert<N>(L[0], k0);
                if (k1 < L[1][N - 1]) topw_insert<N>(L[1], k1);
                if (k2 < L[2][N - 1]) topw_insert<N>(L[2], k2);
                if (k3 < L[3][N - 1]) topw_insert<N>(L[3], k3);
            }
        }
    }
    const int64_t part = (int64_t)blockIdx.x * rpb + lr;
    uint64_t *dst = P.scratch + ((part * P.KP) + 4 * (int64_t)c) * P.n;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < P.n) dst[q * P.n + j] = L[q][j];
}

__device__ __forceinline__ uint64_t topw_wave_min(uint64_t x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off, 64);
        const uint64_t y = ((uint64_t)hi << 32) | lo;
        x = y < x ? y : x;
    }
    return x;
}

template <int N>
__global__ void __launch_bounds__(64) llda_top_words_merge_kernel(const TopwParams P)
{
    const int pos = (int)blockIdx.x, lane = threadIdx.x;
    const int k = wide_topic_of(P.leaf_start, P.leaf_len, P.G, P.T, pos);
    if (k < 0) return;                                    // a position of the padding: its lists are never read
    const int n = P.n;
    uint64_t L[N];
#pragma unroll
    for (int j = 0; j < N; ++j) L[j] = TOPW_PAD;
    for (int64_t part = lane; part < P.parts; part += 64) {
        const uint64_t *src = P.scratch + (part * P.KP + pos) * n;
        for (int j = 0; j < n; ++j) {
            const uint64_t key = src[j];
            if (!(key < L[N - 1])) break;                 // (the partial list ascends: nothing behind it gets in either)
            topw_insert<N>(L, key);
        }
    }
    for (int i = 0; i < n; ++i) {
        const uint64_t m = topw_wave_min(L[0]);
        if (L[0] == m) {                                  // keys are unique: one lane pops (all of them once only padding is left)
#pragma unroll
            for (int j = 0; j + 1 < N; ++j) L[j] = L[j + 1];
            L[N - 1] = TOPW_PAD;
        }
        if (lane == 0) {
            const bool real = m != TOPW_PAD;
            if (P.top_idx) P.top_idx[(int64_t)k * n + i] = real ? (int32_t)(uint32_t)m : -1;
            if (P.top_cnt) P.top_cnt[(int64_t)k * n + i] = real ? (int32_t)(0x7FFFFFFFu - (uint32_t)(m >> 32)) : 0;
        }
    }
}

}  // namespace
