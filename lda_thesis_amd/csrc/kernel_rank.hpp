// kernel_rank.hpp -- llda_rank_labels_kernel: per-document ranking of label scores, top-n labels and the ingredients of the harness metrics
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_rank_labels (include/llda_gibbs.h): everything the harness does with a held-out document's loads after the fold-in --
// get_preds (LabeledLDA.py:214-229) and one_roc / macro_auc_roc / n_error / get_f1 (evaluate_LabeledLDA.py:8-93) -- from ONE sort of
// the document's L = K - first ranked scores.
//
// Geometry.  NP = L rounded up to a power of two (at least 16).  A TEAM of NP / 8 threads owns a document: eight keys per thread.
// A workgroup has max(256, NP / 8) threads and walks 2048 / NP documents at a time (one for NP >= 2048), so the LDS of a workgroup
// is 20 KB of keys up to NP = 2048, 40 KB at 4096 and 80 KB at 8192, plus 10.5 bytes per thread for the scans.  Several teams share a
// wavefront for NP < 512, one wavefront is a team at 512 (K = 512: four documents per workgroup), several wavefronts beyond.
//
// Sort.  A score becomes a 64-bit key that ASCENDS as the score descends (-0 folded onto +0), its payload is topic << 1 | truth:
// (key, payload) ascending is "score descending, then topic id ascending", a strict total order, so the bitonic network -- not a
// stable sort -- has exactly one result, np.argsort(-row, kind="stable").  Padding carries key = payload = all ones and sorts behind
// every score that is not a NaN.  The stages with a distance below 8 stay inside a thread's eight CONTIGUOUS keys and run in
// registers (one LDS round trip for the three of them); the others exchange through LDS, lanes on consecutive keys.
//
// After the sort every thread walks its eight positions.  A position ends a tie group when its key differs from the next one's:
// those are the thresholds of one_roc, highest first, with tp = truths so far and fp = position + 1 - tp.  One scan over the team
// gives every thread the truths before it and the position of the last threshold before it (whose tp is looked up in LDS); the sums
// (A, T), the best F1 -- compared by cross-multiplication of integers -- and the first true position are reduced over the team.
// All of it is integer arithmetic; auc and f1 are ONE IEEE division each, so the outputs do not depend on the geometry.
// ---------------------------------------------------------------------------------------------
struct RankParams {
    const double *score;
    const uint8_t *truth;
    int64_t D, ld, n_tiles;
    int32_t K, first, L, top_n;
    int32_t *top_idx;
    double *top_val;
    int32_t *n_thr;
    double *auc;
    double *f1;
    int32_t *hit_rank;
    int32_t *flags;
};

constexpr uint64_t RANK_KEY_ZERO = 0x7FFFFFFFFFFFFFFFull;   // the key of +0.0 (and of -0.0)
constexpr uint64_t RANK_KEY_PAD = 0xFFFFFFFFFFFFFFFFull;
constexpr uint32_t RANK_PAY_PAD = 0xFFFFu;

__device__ __forceinline__ uint64_t rank_key(uint64_t bits)
{
    if (bits == 0x8000000000000000ull) bits = 0;                                    // -0.0 == +0.0
    return (bits >> 63) ? bits : (~bits & 0x7FFFFFFFFFFFFFFFull);                   // +inf lowest ... +0 ... -inf highest
}

// compare-exchange of (key, payload) in registers: ascending when asc
__device__ __forceinline__ void rank_ce(uint64_t &ka, uint32_t &pa, uint64_t &kb, uint32_t &pb, bool asc)
{
    const bool gt = ka > kb || (ka == kb && pa > pb);
    const bool sw = gt == asc;
    const uint64_t k0 = sw ? kb : ka, k1 = sw ? ka : kb;
    const uint32_t p0 = sw ? pb : pa, p1 = sw ? pa : pb;
    ka = k0; kb = k1; pa = p0; pb = p1;
}

template <int NP>
__global__ void __launch_bounds__((NP / 8 > 256 ? NP / 8 : 256)) llda_rank_labels_kernel(const RankParams P)
{
    constexpr int TPD = NP / 8;                         // threads of a team
    constexpr int NT = TPD > 256 ? TPD : 256;
    constexpr int DPB = NT / TPD;                       // documents of a tile
    __shared__ uint64_t s_key[NT * 8];
    __shared__ uint16_t s_pay[NT * 8];                  // payloads; after the sort: truths up to every position
    __shared__ int32_t s_a[2][NT];                      // scan: truths; reduction: best F1 as num << 16 | den
    __shared__ int32_t s_b[2][NT];                      // scan: last threshold position + 1; reduction: first true position
    __shared__ uint64_t s_at[NT];                       // reduction: A << 16 | T
    __shared__ uint32_t s_seen[DPB];                    // bit 0 a NaN, bit 1 a score that is not zero

    const int tid = threadIdx.x, dl = tid / TPD, tl = tid % TPD;
    const int base = dl * NP;
    const int L = P.L;

    for (int64_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const int64_t d = tile * DPB + dl;
        const bool active = d < P.D;
        __syncthreads();                                // (the previous tile's LDS is no longer read)
        if (tl == 0) s_seen[dl] = 0;
        __syncthreads();
        // ---- load: lanes on consecutive columns
        {
            const double *srow = P.score + (active ? d * P.ld + P.first : 0);
            const uint8_t *trow = P.truth ? P.truth + (active ? d * (int64_t)P.K + P.first : 0) : nullptr;
            uint32_t seen = 0;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int i = m * TPD + tl;
                uint64_t key = RANK_KEY_PAD;
                uint32_t pay = RANK_PAY_PAD;
                if (active && i < L) {
                    const uint64_t bits = (uint64_t)__double_as_longlong(srow[i]);
                    const uint32_t t = trow ? (trow[i] != 0 ? 1u : 0u) : 0u;
                    key = rank_key(bits);
                    pay = ((uint32_t)(P.first + i) << 1) | t;
                    if ((bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) seen |= 1u;
                    if (key != RANK_KEY_ZERO) seen |= 2u;
                }
                s_key[base + i] = key;
                s_pay[base + i] = (uint16_t)pay;
            }
            if (seen) atomicOr(&s_seen[dl], seen);      // (an LDS atomic)
        }
        __syncthreads();
        // ---- bitonic sort of (key, payload), ascending
        uint64_t k[8];
        uint32_t p[8];
        const int own = base + tl * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) { k[e] = s_key[own + e]; p[e] = s_pay[own + e]; }
#pragma unroll
        for (int kk = 2; kk <= 8; kk <<= 1)
#pragma unroll
            for (int j = kk >> 1; j >= 1; j >>= 1)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if ((e ^ j) > e) rank_ce(k[e], p[e], k[e ^ j], p[e ^ j], kk < 8 ? (e & kk) == 0 : (tl & 1) == 0);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s_key[own + e] = k[e]; s_pay[own + e] = (uint16_t)p[e]; }
        for (int kk = 16; kk <= NP; kk <<= 1) {
            for (int j = kk >> 1; j >= 8; j >>= 1) {
                __syncthreads();
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int q = m * TPD + tl;                                      // pair of the document, lanes consecutive
                    const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i + j;
                    const uint64_t ka = s_key[base + i], kb = s_key[base + l];
                    const uint32_t pa = s_pay[base + i], pb = s_pay[base + l];
                    const bool gt = ka > kb || (ka == kb && pa > pb);
                    if (gt == ((i & kk) == 0)) {
                        s_key[base + i] = kb; s_key[base + l] = ka;
                        s_pay[base + i] = (uint16_t)pb; s_pay[base + l] = (uint16_t)pa;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 8; ++e) { k[e] = s_key[own + e]; p[e] = s_pay[own + e]; }
            const bool asc = ((tl * 8) & kk) == 0;
#pragma unroll
            for (int j = 4; j >= 1; j >>= 1)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if ((e ^ j) > e) rank_ce(k[e], p[e], k[e ^ j], p[e ^ j], asc);
            if (kk < NP) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { s_key[own + e] = k[e]; s_pay[own + e] = (uint16_t)p[e]; }
            } else if (tl > 0) {
                s_key[own] = k[0];                      // (all the neighbour below needs)
            }
        }
        __syncthreads();
        // ---- thresholds and truths of the thread's eight positions
        const uint32_t seen = s_seen[dl];
        const bool has_nan = seen & 1u;
        const int p0 = tl * 8;
        const uint64_t k_next = tl + 1 < TPD ? s_key[own + 8] : RANK_KEY_PAD;
        uint32_t ends = 0, tr = 0;                      // bit e: position p0 + e ends a tie group / carries a true label
        int c = 0, last_end = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int pos = p0 + e;
            const uint64_t nx = e < 7 ? k[e + 1] : k_next;
            if (pos < L) {
                if (pos == L - 1 || k[e] != nx) { ends |= 1u << e; last_end = pos + 1; }
                if (p[e] & 1u) { tr |= 1u << e; ++c; }
            }
        }
        // top-n: the first positions of the order, straight from the registers of the team's first two threads
        if (active && p0 < P.top_n) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int pos = p0 + e;
                if (pos < P.top_n) {
                    const bool real = pos < L && !has_nan;
                    const int topic = (int)(p[e] >> 1);
                    if (P.top_idx) P.top_idx[d * P.top_n + pos] = real ? topic : -1;
                    if (P.top_val) P.top_val[d * P.top_n + pos] = real ? P.score[d * P.ld + topic] : 0.0;
                }
            }
        }
        // ---- scan over the team: truths before the thread, last threshold before the thread
        int vs = c, vm = last_end, buf = 0;
        s_a[0][tid] = vs; s_b[0][tid] = vm;
        for (int off = 1; off < TPD; off <<= 1) {
            __syncthreads();
            if (tl >= off) { vs += s_a[buf][tid - off]; vm = max(vm, s_b[buf][tid - off]); }
            buf ^= 1;
            s_a[buf][tid] = vs; s_b[buf][tid] = vm;
        }
        __syncthreads();
        const int tp_before = tl ? s_a[buf][tid - 1] : 0;
        const int prev_end = tl ? s_b[buf][tid - 1] : 0;                            // position + 1 of the last threshold before p0; 0: none
        const int n_pos = s_a[buf][tid - tl + TPD - 1];                              // P
        {
            int run = tp_before;
#pragma unroll
            for (int e = 0; e < 8; ++e) { run += (tr >> e) & 1u; s_pay[own + e] = (uint16_t)run; }
        }
        __syncthreads();
        // ---- walk
        int run_tp = tp_before, prev_tp = prev_end ? (int)s_pay[base + prev_end - 1] : 0, prev_fp = prev_end - prev_tp;
        bool have_prev = prev_end > 0;
        int n_thr = 0, hit = 0x7FFFFFFF, best_num = 0, best_den = 0;
        int64_t area = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int pos = p0 + e;
            if ((tr >> e) & 1u) { ++run_tp; hit = min(hit, pos + 1); }
            if ((ends >> e) & 1u) {
                const int fp = pos + 1 - run_tp;
                ++n_thr;
                if (have_prev) area += (int64_t)(fp - prev_fp) * (run_tp + prev_tp);
                prev_tp = run_tp; prev_fp = fp; have_prev = true;
                if (run_tp > 0) {
                    const int num = 2 * run_tp, den = run_tp + fp + n_pos;           // 2 tp / (2 tp + fp + fn)
                    if (best_den == 0 || num * best_den > best_num * den) { best_num = num; best_den = den; }
                }
            }
        }
        // ---- reduction over the team (scan arrays reused: their last readers are behind the barrier above)
        uint64_t at = ((uint64_t)area << 16) | (uint32_t)n_thr;                      // A < 2^27, T <= 8192: the fields never carry
        s_at[tid] = at; s_a[0][tid] = (best_num << 16) | best_den; s_b[0][tid] = hit;
        for (int off = TPD >> 1; off >= 1; off >>= 1) {
            __syncthreads();
            if (tl < off) {
                at += s_at[tid + off];
                hit = min(hit, s_b[0][tid + off]);
                const int o = s_a[0][tid + off], o_num = o >> 16, o_den = o & 0xFFFF;
                if (o_den != 0 && (best_den == 0 || o_num * best_den > best_num * o_den)) { best_num = o_num; best_den = o_den; }
                s_at[tid] = at; s_a[0][tid] = (best_num << 16) | best_den; s_b[0][tid] = hit;
            }
        }
        if (active && tl == 0) {
            const double nan = __longlong_as_double(0x7FF8000000000000ll);
            const int T = (int)(at & 0xFFFFu);
            const int64_t A = (int64_t)(at >> 16);
            const int n_neg = L - n_pos;
            int fl = 0;
            if (has_nan) fl = 16;
            else {
                if (T < 2) fl |= 4;
                if (!(seen & 2u)) fl |= 8;
                if (P.truth) fl |= (n_pos == 0 ? 1 : 0) | (n_neg == 0 ? 2 : 0);
            }
            if (P.n_thr) P.n_thr[d] = has_nan ? 0 : T;
            if (P.flags) P.flags[d] = fl;
            if (P.truth) {
                const bool no_auc = has_nan || n_pos == 0 || n_neg == 0 || T < 2;
                if (P.auc) P.auc[d] = no_auc ? nan : (double)A / (double)(2 * (int64_t)n_pos * n_neg);
                if (P.f1) P.f1[d] = (has_nan || best_den == 0) ? nan : (double)best_num / (double)best_den;
                if (P.hit_rank) P.hit_rank[d] = (has_nan || hit == 0x7FFFFFFF) ? 0 : hit;
            }
        }
    }
}

}  // namespace
