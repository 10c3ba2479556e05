// kernel_cooc.hpp -- llda_word_cooc_kernel, llda_word_cooc_agg_kernel: document and co-document frequencies of the words a topic lists
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_word_cooc (include/llda_gibbs.h): the integers UMass coherence (Mimno et al. 2011) and NPMI are made of.  For every document
// d and topic k, R(d, k) = the ranks r for which a site of d carries the word listed as (k, r); co[k][i][j] += 1 for i >= j in R.
//
// Geometry.  One wavefront per document, COOC_WAVES documents per workgroup.  Each wavefront owns K 16-bit rank masks in LDS, two
// topics per 32-bit word (1 KB at K = 512, 15 KB at K = 7688).  The lanes walk the document's sites 64 at a time, look the word up
// in the membership table and OR 1 << rank into the topic's mask with an LDS atomic: a word that repeats, or two words of one
// topic, meet in the mask, so a pair is counted once per document.  Most sites carry a word no topic lists and cost two loads.
// Then the lanes take the mask words lane, lane + 64, ...; a non-zero word is cleared on the spot -- the masks are all zero
// again when the wavefront turns to its next document -- and gives one 64-bit global atomic per set bit and per set pair.  A
// document without any listed word skips that pass.  Integer atomics are exact and independent of order: the result can be
// compared with ==.  Only the wavefront itself touches its masks and LDS operations of a wavefront complete in order, so no
// workgroup barrier is needed: a wavefront-scope fence keeps the compiler from reordering across the two phases.
//
// Large calls (llda_word_cooc_agg_kernel, from LLDA_COOC_AGG_MIN_DOCS documents on).  Where most documents hold most listed words
// -- configs[3]: 27 213 of the 28 160 entries of co per document -- the pass above is bound by the chip's rate of global atomics
// (measured: 19.7 G adds / s, 1 381 ms = 43 sweeps).  The same two phases then run per SLICE of topics (blockIdx.y) whose
// n (n + 1) / 2 counters per topic fit into LDS next to the masks (60 KB a workgroup): a set bit or pair is an LDS atomic on a
// 32-bit counter, the lanes on different topics, and every workgroup adds its non-zero counters to co once, at the end (83 ms).
// A slice re-reads the corpus, so the form is taken only up to COOC_AGG_MAX_SLICES slices; beyond that (K in the thousands with
// long lists: sparse label sets, few hits per document) the direct form stays.  Both forms add the same integers.
// ---------------------------------------------------------------------------------------------
constexpr int COOC_WAVES = 4;
constexpr int COOC_AGG_MAX_SLICES = 8;
constexpr int COOC_AGG_LDS_WORDS = 15 * 1024;               // counters + masks of a workgroup: 60 KB, two workgroups per CU
constexpr int COOC_AGG_BLOCKS = 1024;                       // workgroups over all slices

struct CoocParams {
    const int64_t *doc_off;
    const int32_t *word;
    const int32_t *memb_off;
    const int32_t *memb;
    unsigned long long *co;
    int64_t D, V;
    int32_t K, n, words;                                  // words = mask words of a document: (K + 1) / 2
    int32_t ks, np;                                       // agg form: topics of a slice (even), n (n + 1) / 2
};

__global__ void __launch_bounds__(64 * COOC_WAVES) llda_word_cooc_kernel(const CoocParams P)
{
    extern __shared__ uint32_t s_cooc[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *mask = s_cooc + wave * P.words;
    for (int i = lane; i < P.words; i += 64) mask[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int n = P.n;
    for (int64_t d = (int64_t)blockIdx.x * COOC_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * COOC_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        bool hit = false;
        for (int64_t s = b + lane; s < e; s += 64) {
            const int32_t w = P.word[s];
            if ((uint64_t)(int64_t)w >= (uint64_t)P.V) continue;
            const int32_t lo = P.memb_off[w], hi = P.memb_off[w + 1];
            for (int32_t m = lo; m < hi; ++m) {
                const uint32_t en = (uint32_t)P.memb[m], k = en >> 4, r = en & 15u;
                if (k < (uint32_t)P.K && r < (uint32_t)n) {
                    atomicOr(&mask[k >> 1], 1u << ((k & 1u) * 16u + r));
                    hit = true;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (__any(hit)) {
            for (int i = lane; i < P.words; i += 64) {
                const uint32_t both = mask[i];
                if (both == 0) continue;
                mask[i] = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t bits = (both >> (16 * h)) & 0xFFFFu;
                    if (bits == 0) continue;
                    unsigned long long *base = P.co + (int64_t)(2 * i + h) * n * n;
                    uint32_t hiw = bits;
                    while (hiw) {
                        const int ri = __builtin_ctz(hiw);
                        hiw &= hiw - 1;
                        uint32_t low = bits & ((2u << ri) - 1u);          // the set ranks j <= i
                        while (low) {
                            const int rj = __builtin_ctz(low);
                            low &= low - 1;
                            atomicAdd(base + ri * n + rj, 1ull);
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

__global__ void __launch_bounds__(64 * COOC_WAVES) llda_word_cooc_agg_kernel(const CoocParams P)
{
    extern __shared__ uint32_t s_cooc[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, np = P.np;
    const int k0 = (int)blockIdx.y * P.ks;
    const int kn = min(P.ks, P.K - k0);                   // topics of this slice
    const int words = (kn + 1) >> 1;
    uint32_t *cnt = s_cooc;                               // [ks][np]
    uint32_t *mask = s_cooc + P.ks * np + wave * (P.ks >> 1);
    for (int i = tid; i < P.ks * np + COOC_WAVES * (P.ks >> 1); i += 64 * COOC_WAVES) s_cooc[i] = 0;
    __syncthreads();
    for (int64_t d = (int64_t)blockIdx.x * COOC_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * COOC_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        bool hit = false;
        for (int64_t s = b + lane; s < e; s += 64) {
            const int32_t w = P.word[s];
            if ((uint64_t)(int64_t)w >= (uint64_t)P.V) continue;
            const int32_t lo = P.memb_off[w], hi = P.memb_off[w + 1];
            for (int32_t m = lo; m < hi; ++m) {
                const uint32_t en = (uint32_t)P.memb[m], r = en & 15u;
                const uint32_t kl = (en >> 4) - (uint32_t)k0;                 // (wraps to a large value below the slice)
                if (kl < (uint32_t)kn && r < (uint32_t)n) {
                    atomicOr(&mask[kl >> 1], 1u << ((kl & 1u) * 16u + r));
                    hit = true;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (__any(hit)) {
            for (int i = lane; i < words; i += 64) {
                const uint32_t both = mask[i];
                if (both == 0) continue;
                mask[i] = 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t bits = (both >> (16 * h)) & 0xFFFFu;
                    if (bits == 0) continue;
                    uint32_t *base = cnt + (2 * i + h) * np;
                    uint32_t hiw = bits;
                    while (hiw) {
                        const int ri = __builtin_ctz(hiw);
                        hiw &= hiw - 1;
                        uint32_t low = bits & ((2u << ri) - 1u);
                        const int row = ri * (ri + 1) / 2;
                        while (low) {
                            const int rj = __builtin_ctz(low);
                            low &= low - 1;
                            atomicAdd(base + row + rj, 1u);
                        }
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    for (int c = tid; c < kn * np; c += 64 * COOC_WAVES) {
        const uint32_t v = cnt[c];
        if (v == 0) continue;
        const int kl = c / np, t = c - kl * np;
        int ri = 0;
        while ((ri + 1) * (ri + 2) / 2 <= t) ++ri;
        const int rj = t - ri * (ri + 1) / 2;
        atomicAdd(P.co + ((int64_t)(k0 + kl) * n + ri) * n + rj, (unsigned long long)v);
    }
}

}  // namespace
