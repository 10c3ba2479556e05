// top_list.hpp -- TopList<N, Ord>: the N best entries under a strict total order, kept sorted in registers
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there); everything but pop_wave is
// plain C++ and is compiled by a host test too (tests/test_top_list_host.py).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define TOP_LIST_FN __device__ __forceinline__
#define TOP_LIST_UNROLL _Pragma("unroll")
#else
#define TOP_LIST_FN inline
#define TOP_LIST_UNROLL
#endif

// ---------------------------------------------------------------------------------------------
// The list behind every "best n of a column" kernel: kernel_topwords.hpp, kernel_scored.hpp, kernel_ecdf.hpp (FREX)
// and the merge kernel of kernel_nearest.hpp.  An entry is Q 64-bit words and W 32-bit words.  The list keeps one array of N
// registers PER WORD, never an array of entries, and every index is a constant once the loops are unrolled: N is a template argument
// and the list never leaves the registers.  Place 0 is the best entry; places that hold nothing hold the padding.
// A part of the key that is compared as 64 bits (an integer key, the bits of a double) is a 64-bit word, never two 32-bit words: the
// compare wants a register pair, and a list of halves is then held twice, as halves and as pairs (profiles/top_list_refactor.md).
//
// Ord is the order and everything a caller has of its own:
//   Q, W           64-bit and 32-bit words of an entry
//   pad()          the padding: before(pad(), x) is false for every x, before(x, pad()) is true for every real x
//   before(a, b)   strict: does a come before b?  A total order over the entries that are offered (a caller keeps out what has no
//                  place in it, such as a NaN score)
//   same(a, b)     the identity that is unique within one selection -- it names the one lane whose head pop_wave takes
// An Ord may carry state (FREX: the two weights); the list holds a copy.
//
// The n best under a total order do not depend on the order of arrival, so the result is the same for every split of the input into
// partial lists: insert whatever admits() lets in, fold_sorted() the sorted partial lists of an earlier pass, and, where the 64 lanes
// of a wavefront each hold a list, take the overall best n by n calls of pop_wave().
// ---------------------------------------------------------------------------------------------
template <int Q, int W>
struct TopEntry {
    uint64_t q[Q ? Q : 1];                                // (an array the order does not use is never read: it costs no register)
    uint32_t w[W ? W : 1];
};

template <int N, class Ord>
struct TopList {
    static constexpr int Q = Ord::Q, W = Ord::W;
    typedef TopEntry<Q, W> Entry;
    uint64_t rq[Q ? Q : 1][N];
    uint32_t rw[W ? W : 1][N];
    Ord ord;

    TOP_LIST_FN explicit TopList(const Ord &o = Ord()) : ord(o)
    {
        const Entry p = ord.pad();
        TOP_LIST_UNROLL
        for (int j = 0; j < N; ++j) {
            TOP_LIST_UNROLL
            for (int k = 0; k < Q; ++k) rq[k][j] = p.q[k];
            TOP_LIST_UNROLL
            for (int k = 0; k < W; ++k) rw[k][j] = p.w[k];
        }
    }
    // (j is a constant wherever this is called: the loops around it are unrolled)
    TOP_LIST_FN Entry at(int j) const
    {
        Entry e = Entry();
        TOP_LIST_UNROLL
        for (int k = 0; k < Q; ++k) e.q[k] = rq[k][j];
        TOP_LIST_UNROLL
        for (int k = 0; k < W; ++k) e.w[k] = rw[k][j];
        return e;
    }
    // does c beat the worst entry?  Nothing else changes the list
    TOP_LIST_FN bool admits(const Entry &c) const { return ord.before(c, at(N - 1)); }
    // sorted insertion: every place takes its better neighbour, the candidate, or stays (one compare per place)
    TOP_LIST_FN void insert(const Entry &c)
    {
        bool b[N];
        TOP_LIST_UNROLL
        for (int j = 0; j < N; ++j) b[j] = ord.before(c, at(j));
        TOP_LIST_UNROLL
        for (int k = 0; k < Q; ++k) shift_in(rq[k], b, c.q[k]);
        TOP_LIST_UNROLL
        for (int k = 0; k < W; ++k) shift_in(rw[k], b, c.w[k]);
    }
    // a sorted partial list of n entries, read(j) its j-th: behind the first entry that is not admitted nothing gets in either
    template <class Read>
    TOP_LIST_FN void fold_sorted(int n, Read &&read)
    {
        for (int j = 0; j < n; ++j) {
            const Entry c = read(j);
            if (!admits(c)) break;
            insert(c);
        }
    }
#ifdef __HIPCC__
    // the best head of the wavefront's 64 lists, removed from the lane that holds it: the same entry in every lane.  Once only the
    // padding is left every lane pops, which changes nothing.
    TOP_LIST_FN Entry pop_wave()
    {
        Entry m = at(0);
        TOP_LIST_UNROLL
        for (int off = 32; off >= 1; off >>= 1) {
            Entry y = Entry();
            TOP_LIST_UNROLL
            for (int k = 0; k < Q; ++k) y.q[k] = __shfl_xor(m.q[k], off, 64);
            TOP_LIST_UNROLL
            for (int k = 0; k < W; ++k) y.w[k] = __shfl_xor(m.w[k], off, 64);
            const bool take = ord.before(y, m);
            TOP_LIST_UNROLL
            for (int k = 0; k < Q; ++k) m.q[k] = take ? y.q[k] : m.q[k];
            TOP_LIST_UNROLL
            for (int k = 0; k < W; ++k) m.w[k] = take ? y.w[k] : m.w[k];
        }
        const bool mine = ord.same(at(0), m);             // (selects, not a branch: some lane always pops)
        const Entry p = ord.pad();
        TOP_LIST_UNROLL
        for (int k = 0; k < Q; ++k) shift_out(rq[k], mine, p.q[k]);
        TOP_LIST_UNROLL
        for (int k = 0; k < W; ++k) shift_out(rw[k], mine, p.w[k]);
        return m;
    }
#endif

private:
    template <class T>
    static TOP_LIST_FN void shift_in(T (&a)[N], const bool (&b)[N], T c)
    {
        TOP_LIST_UNROLL
        for (int j = N - 1; j > 0; --j) a[j] = b[j - 1] ? a[j - 1] : (b[j] ? c : a[j]);
        a[0] = b[0] ? c : a[0];
    }
    template <class T>
    static TOP_LIST_FN void shift_out(T (&a)[N], bool mine, T pad)
    {
        TOP_LIST_UNROLL
        for (int j = 0; j + 1 < N; ++j) a[j] = mine ? a[j + 1] : a[j];
        a[N - 1] = mine ? pad : a[N - 1];
    }
};
