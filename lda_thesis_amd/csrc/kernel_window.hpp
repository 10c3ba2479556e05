// kernel_window.hpp -- llda_window_cooc_kernel<AGG>: in how many sliding windows of the running text the words a topic lists meet
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_window_cooc (include/llda_gibbs.h): the integers C_V, C_UCI and C_NPMI (Roeder, Both and Hinneburg 2015) are made of.  A
// document of L tokens has the windows [w, w + s) for w = 0 .. L - s (one window, the whole document, when s = 0 or L <= s); for
// every window and topic k, R = the ranks r for which a position of the window carries the word listed as (k, r);
// co[k][i][j] += 1 for i >= j in R.
//
// Run lengths.  A document's windows overlap, so a mask per document (kernel_cooc.hpp) does not do; but R changes only where a
// listed word enters or leaves the window.  One wavefront per document, WINDOW_WAVES documents per workgroup.  Per topic of its
// slice a wavefront keeps in LDS: how often every rank occurs inside the current window (16 bits each, two per word: a count is
// at most s <= LLDA_WINDOW_MAX = 65 535), the 16-bit rank mask R, and `since` = the first window index at which that mask has
// held.  The first window is filled by all lanes at once (LDS atomics).  Then the lanes load, 64 windows at a time, the token
// that leaves at window w (position w - 1), the token that enters (position w + s - 1) and their ranges in the membership table;
// a ballot leaves the windows at which a listed word moves, and only those are played, in order, the leaving token before the
// entering one.  The entries of a token go one to a lane.  A count that goes 1 -> 0 or 0 -> 1 is a change of R: the lane swaps
// w into `since` (of two ranks of one topic that list the same word, exactly one receives the old value), reads the old mask,
// and -- behind a wavefront barrier, so that every lane has read -- toggles its bit.  Each topic that changed after holding its
// mask for len = w - since > 0 windows is then FLUSHED: the lanes take the n (n + 1) / 2 <= 136 pairs (i >= j), three to a lane
// at most, and add len where the old mask holds both ranks.  After the last window every topic with a mask is flushed with the
// number of windows, masks and `since` go back to zero, and the counts are cleared by walking the last window once more.  The
// work goes with the listed tokens, not with windows x topics.  A window index is 32 bits: a document holds fewer than 2^32
// tokens.  All adds are integers: the result does not depend on geometry or order and is compared with ==.
//
// Where a flush adds.  AGG = false: 64-bit global atomics on co.  AGG = true (from LLDA_WINDOW_AGG_MIN_DOCS documents on): 64-bit
// LDS counters of the workgroup, [topics of the slice][pairs], added to co once at the end -- the chip's rate of global atomics
// binds the first form where most windows hold several listed words (kernel_cooc.hpp has the figure).
//
// LDS.  State of a wavefront: 2 + (n + 1) / 2 words per topic (28 bytes at n = 10, 40 at n = 16); the counters 8 n (n + 1) / 2
// bytes per topic.  Neither fits for K = LLDA_MAX_K, so the topics are cut into slices (blockIdx.y) that fit WINDOW_LDS_BYTES
// (two workgroups per CU), each slice reading the corpus again and ignoring the entries of other topics: K = 512, n = 10 is one
// slice without counters and four with them; K = 7 688, n = 16 is sixteen without.  With more than WINDOW_AGG_MAX_SLICES slices
// the counters are not worth the re-reads and the first form stays.  Every form and every slicing adds the same integers.
// ---------------------------------------------------------------------------------------------
constexpr int WINDOW_WAVES = 4;
constexpr int WINDOW_LDS_BYTES = 80 * 1024;
constexpr int WINDOW_AGG_MAX_SLICES = 8;
constexpr int WINDOW_AGG_BLOCKS = 1024;                     // workgroups over all slices

struct WindowParams {
    const int64_t *tok_off;
    const int32_t *tok;
    const int32_t *memb_off;
    const int32_t *memb;
    unsigned long long *co;
    int64_t D, V;
    int32_t K, n, window;
    int32_t ks, np, cw;                                   // topics of a slice, n (n + 1) / 2, count words of a topic: (n + 1) / 2
};

// the pairs of a lane: pair t = lane + 64 q is (ri, rj), ri (ri + 1) / 2 + rj = t; bits = both ranks (never met by a mask when
// t >= np), off = the pair's place in the destination
struct WindowPairs {
    uint32_t bits[3];
    int32_t off[3];
};

__device__ inline void window_flush(unsigned long long *base, const WindowPairs &pr, uint32_t m, uint32_t len)
{
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if ((m & pr.bits[q]) == pr.bits[q]) atomicAdd(base + pr.off[q], (unsigned long long)len);
}

inline __device__ void window_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <bool AGG>
__global__ void __launch_bounds__(64 * WINDOW_WAVES) llda_window_cooc_kernel(const WindowParams P)
{
    extern __shared__ unsigned long long s_window[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, np = P.np, cw = P.cw, ks = P.ks;
    const int k0 = (int)blockIdx.y * ks;
    const int kn = min(ks, P.K - k0);                     // topics of this slice
    unsigned long long *acc = s_window;                   // AGG: [ks][np]
    uint32_t *state = reinterpret_cast<uint32_t *>(s_window + (AGG ? ks * np : 0)) + wave * ks * (2 + cw);
    uint32_t *mask = state, *since = state + ks, *cnt = state + 2 * ks;
    if (AGG)
        for (int i = tid; i < ks * np; i += 64 * WINDOW_WAVES) acc[i] = 0;
    for (int i = lane; i < ks * (2 + cw); i += 64) state[i] = 0;
    if (AGG) __syncthreads();
    window_sync();
    WindowPairs pr;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int t = lane + 64 * q;
        int ri = 0;
        while ((ri + 1) * (ri + 2) / 2 <= t) ++ri;
        const int rj = t - ri * (ri + 1) / 2;
        pr.bits[q] = t < np ? (1u << ri) | (1u << rj) : 0xFFFFFFFFu;
        pr.off[q] = t < np ? (AGG ? t : ri * n + rj) : 0;
    }
    auto dest = [&](uint32_t kl) { return AGG ? acc + kl * np : P.co + (int64_t)(k0 + (int)kl) * n * n; };

    for (int64_t d = (int64_t)blockIdx.x * WINDOW_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * WINDOW_WAVES) {
        const int64_t b = P.tok_off[d], L = P.tok_off[d + 1] - b;
        if (L <= 0) continue;
        const bool slide = P.window > 0 && L > P.window;
        const int64_t s = slide ? P.window : L;
        const int64_t W = L - s + 1;                      // windows of the document
        bool hit = false;
        // the first window
        for (int64_t p = b + lane; p < b + s; p += 64) {
            const int32_t w = P.tok[p];
            if ((uint64_t)(int64_t)w >= (uint64_t)P.V) continue;
            const int32_t lo = P.memb_off[w], hi = P.memb_off[w + 1];
            for (int32_t m = lo; m < hi; ++m) {
                const uint32_t en = (uint32_t)P.memb[m], r = en & 15u;
                const uint32_t kl = (en >> 4) - (uint32_t)k0;                 // (wraps to a large value below the slice)
                if (kl < (uint32_t)kn && r < (uint32_t)n) {
                    atomicOr(&mask[kl], 1u << r);
                    if (slide) atomicAdd(&cnt[kl * cw + (r >> 1)], 1u << (16u * (r & 1u)));
                    hit = true;
                }
            }
        }
        window_sync();
        if (slide) {
            for (int64_t w0 = 1; w0 < W; w0 += 64) {
                int32_t lo_l = 0, hi_l = 0, lo_e = 0, hi_e = 0;
                if (w0 + lane < W) {
                    const int32_t tl = P.tok[b + w0 + lane - 1], te = P.tok[b + w0 + lane + s - 1];
                    if ((uint64_t)(int64_t)tl < (uint64_t)P.V) { lo_l = P.memb_off[tl]; hi_l = P.memb_off[tl + 1]; }
                    if ((uint64_t)(int64_t)te < (uint64_t)P.V) { lo_e = P.memb_off[te]; hi_e = P.memb_off[te + 1]; }
                }
                uint64_t moves = __ballot(hi_l > lo_l || hi_e > lo_e);
                while (moves) {
                    const int j = __builtin_ctzll(moves);
                    moves &= moves - 1;
                    const uint32_t wi = (uint32_t)(w0 + j);
#pragma unroll
                    for (int enter = 0; enter < 2; ++enter) {                 // the leaving token first
                        const int32_t lo = __shfl(enter ? lo_e : lo_l, j), hi = __shfl(enter ? hi_e : hi_l, j);
                        for (int32_t m0 = lo; m0 < hi; m0 += 64) {
                            bool change = false;
                            uint32_t kl = 0, r = 0, held = 0, len = 0;
                            if (m0 + lane < hi) {
                                const uint32_t en = (uint32_t)P.memb[m0 + lane];
                                r = en & 15u;
                                kl = (en >> 4) - (uint32_t)k0;
                                if (kl < (uint32_t)kn && r < (uint32_t)n) {
                                    const uint32_t sh = 16u * (r & 1u);
                                    const uint32_t was = (atomicAdd(&cnt[kl * cw + (r >> 1)], enter ? 1u << sh : 0u - (1u << sh)) >> sh) & 0xFFFFu;
                                    change = was == (enter ? 0u : 1u);
                                }
                            }
                            if (change) {
                                len = wi - atomicExch(&since[kl], wi);
                                held = mask[kl];
                            }
                            window_sync();                                    // every lane has read the mask it flushes
                            if (change) atomicXor(&mask[kl], 1u << r);
                            hit |= change;
                            uint64_t todo = __ballot(change && len != 0 && held != 0);
                            while (todo) {
                                const int f = __builtin_ctzll(todo);
                                todo &= todo - 1;
                                window_flush(dest(__shfl(kl, f)), pr, __shfl(held, f), __shfl(len, f));
                            }
                            window_sync();
                        }
                    }
                }
            }
        }
        if (!__any(hit)) continue;
        // after the last window: what every topic still holds, for W - since windows
        for (int i0 = 0; i0 < kn; i0 += 64) {
            uint32_t held = 0, len = 0;
            if (i0 + lane < kn) {
                held = mask[i0 + lane];
                const uint32_t so = since[i0 + lane];
                len = (uint32_t)W - so;
                if (held) mask[i0 + lane] = 0;
                if (so) since[i0 + lane] = 0;
            }
            uint64_t todo = __ballot(held != 0);
            while (todo) {
                const int f = __builtin_ctzll(todo);
                todo &= todo - 1;
                window_flush(dest((uint32_t)(i0 + f)), pr, __shfl(held, f), __shfl(len, f));
            }
        }
        if (slide) {
            for (int64_t p = b + L - s + lane; p < b + L; p += 64) {          // the counts of the last window back to zero
                const int32_t w = P.tok[p];
                if ((uint64_t)(int64_t)w >= (uint64_t)P.V) continue;
                const int32_t lo = P.memb_off[w], hi = P.memb_off[w + 1];
                for (int32_t m = lo; m < hi; ++m) {
                    const uint32_t en = (uint32_t)P.memb[m], r = en & 15u, kl = (en >> 4) - (uint32_t)k0;
                    if (kl < (uint32_t)kn && r < (uint32_t)n) cnt[kl * cw + (r >> 1)] = 0;
                }
            }
        }
        window_sync();
    }
    if (AGG) {
        __syncthreads();
        for (int c = tid; c < kn * np; c += 64 * WINDOW_WAVES) {
            const unsigned long long v = acc[c];
            if (v == 0) continue;
            const int kl = c / np, t = c - kl * np;
            int ri = 0;
            while ((ri + 1) * (ri + 2) / 2 <= t) ++ri;
            const int rj = t - ri * (ri + 1) / 2;
            atomicAdd(P.co + ((int64_t)(k0 + kl) * n + ri) * n + rj, v);
        }
    }
}

}  // namespace
