// kernel_label.hpp -- llda_label_keys / _sort / _merge / _walk kernels: the documents of every label ranked by that label's score, and
//                     llda_label_sets_kernel: per-label thresholds applied to every document
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_label_metrics (include/llda_gibbs.h): the other sort.  llda_rank_labels sorts the K scores of a document inside
// one workgroup; here every ranked label sorts its D documents -- a segmented sort of D keys for each of n_labels segments, D up to
// 2^30 -- and one pass over the sorted row gives the label's AUC, its best F1 with the threshold that reaches it, and the order.
//
// Keys.  rank_key (kernel_rank.hpp) of the score, payload doc << 1 | truth: (key, payload) ascending is "score descending, then
// document id ascending", a strict total order, so the sort has exactly one result whatever the network or the merge tree.  A row is
// padded to Dp = D rounded up to the chunk with key = payload = all ones.  A real payload is below 2^31, so the padding sorts behind
// every document, even behind a NaN whose bits are all ones.  A NaN's key lies outside [key(+inf), key(-inf)] and therefore sorts to
// one of the two ends of the row: looking at positions 0 and D - 1 finds it.
//
// Pass 1, llda_label_keys_kernel: a 64 x 64 tile (documents x labels) goes through LDS; the reads run along a score row, the writes
//   along a label's key row.  Grid (Dp / 64, ceil(n_labels / 64)).
// Pass 2, llda_label_sort_kernel<CH>: grid (Dp / CH, n_labels); CH / 8 threads sort one chunk of CH pairs in LDS (12 bytes a pair) with
//   the bitonic network of llda_rank_labels_kernel: eight contiguous keys per thread, the stages with a distance below 8 in registers
//   (rank_ce), the others through LDS with lanes on consecutive pairs.  In place.
// Pass 3, llda_label_merge_kernel<TILE>, once per level (runs of R, 2 R, ... until one run is left), ping-pong between the two buffers:
//   grid (Dp / TILE, n_labels).  A tile of TILE outputs finds its split of the two runs by a merge-path search on (key, payload) in
//   global memory (two lanes, one for each end of the tile), stages both pieces in LDS, every thread finds its own split there and
//   merges eight outputs; they leave through LDS so that the stores are coalesced.  A run without a partner is copied.
// Pass 4, llda_label_walk_kernel: one workgroup per label.  It counts the label's positives P (the best F1 needs P from the first
//   threshold on), then reads the sorted row in tiles of 2048 positions, eight per thread.  Per tile one scan over the workgroup gives
//   every thread the truths before it and the last threshold before it (llda_rank_labels_kernel's scan); between tiles the workgroup
//   carries tp and the previous threshold's (tp, fp).  A, T and the best F1 stay per thread until one reduction at the end.  A tie
//   group, and the best threshold, may straddle any tile, run or chunk boundary: nothing but the carries knows about tiles.
// All of it is integer arithmetic; auc and f1 are ONE IEEE division each, so the outputs do not depend on the geometry.
// ---------------------------------------------------------------------------------------------
constexpr int LABEL_CHUNK = 4096;                         // pairs of a sorted chunk (48 KB of LDS: three workgroups per CU)
constexpr int LABEL_TEST_CHUNK = 256;                     // args.chunk = 256: a deep merge tree at a few thousand documents
constexpr int LABEL_TILE = 2048;                          // outputs of a merge tile, positions of a walk tile (256 threads x 8)
constexpr int LABEL_WALK_NT = 256;
constexpr uint32_t LABEL_PAY_PAD = 0xFFFFFFFFu;
constexpr uint64_t LABEL_KEY_POS_INF = 0x000FFFFFFFFFFFFFull;   // rank_key(+inf): a smaller key is a NaN with the sign bit clear
constexpr uint64_t LABEL_KEY_NEG_INF = 0xFFF0000000000000ull;   // rank_key(-inf): a larger key is a NaN with the sign bit set

struct LabelParams {
    const double *score;
    const uint8_t *truth;
    int64_t D, ld, Dp;
    int32_t K, first, n_labels, reserved;
    uint64_t *key_a, *key_b;                              // [n_labels][Dp] each; key_a takes the keys, then the passes ping-pong
    uint32_t *pay_a, *pay_b;
    const uint64_t *key_sorted;                           // whichever of the two the last merge level wrote
    const uint32_t *pay_sorted;
    int64_t run;                                          // merge: length of a sorted run of the source
    int64_t *n_pos, *n_thr;
    uint64_t *auc_num;
    double *auc;
    int64_t *thr_tp, *thr_fp;
    double *f1, *thr;
    int32_t *flags;
    int32_t *order;
};

// (key, payload) of a before or equal to that of b
__device__ __forceinline__ bool label_le(uint64_t ka, uint32_t pa, uint64_t kb, uint32_t pb)
{
    return ka < kb || (ka == kb && pa <= pb);
}

__global__ void __launch_bounds__(256) llda_label_keys_kernel(const LabelParams P)
{
    __shared__ uint64_t t_key[64][65];                    // [document][label], one column of padding against bank conflicts
    __shared__ uint8_t t_tr[64][68];
    const int tid = threadIdx.x, x = tid & 63, y = tid >> 6;
    const int64_t d0 = (int64_t)blockIdx.x * 64;
    const int l0 = (int)blockIdx.y * 64;
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {                        // lanes along a score row
        const int r = y + 4 * i;
        const int64_t d = d0 + r;
        const int l = l0 + x;
        uint64_t key = RANK_KEY_PAD;
        uint8_t t = 0;
        if (d < P.D && l < P.n_labels) {
            key = rank_key((uint64_t)__double_as_longlong(P.score[d * P.ld + P.first + l]));
            t = P.truth[d * (int64_t)P.K + P.first + l] != 0 ? 1 : 0;
        }
        t_key[r][x] = key;
        t_tr[r][x] = t;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {                        // lanes along a label's key row
        const int c = y + 4 * i;
        const int l = l0 + c;
        const int64_t d = d0 + x;
        if (l < P.n_labels) {                             // (d < Dp: Dp is a multiple of 64)
            const int64_t at = (int64_t)l * P.Dp + d;
            P.key_a[at] = t_key[x][c];
            P.pay_a[at] = d < P.D ? ((uint32_t)d << 1) | t_tr[x][c] : LABEL_PAY_PAD;
        }
    }
}

// the three register stages (distances 4, 2, 1) of a thread's eight contiguous keys, all in the direction asc
__device__ __forceinline__ void label_reg_stages(uint64_t (&k)[8], uint32_t (&p)[8], bool asc)
{
#pragma unroll
    for (int j = 4; j >= 1; j >>= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if ((e ^ j) > e) rank_ce(k[e], p[e], k[e ^ j], p[e ^ j], asc);
}

template <int CH>
__global__ void __launch_bounds__(CH / 8) llda_label_sort_kernel(const LabelParams P)
{
    constexpr int NT = CH / 8;
    __shared__ uint64_t s_key[CH];
    __shared__ uint32_t s_pay[CH];
    const int tl = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.y * P.Dp + (int64_t)blockIdx.x * CH;
    uint64_t *gk = P.key_a + row;
    uint32_t *gp = P.pay_a + row;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = m * NT + tl;
        s_key[i] = gk[i];
        s_pay[i] = gp[i];
    }
    __syncthreads();
    uint64_t k[8];
    uint32_t p[8];
    const int own = tl * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) { k[e] = s_key[own + e]; p[e] = s_pay[own + e]; }
    // kk = 2, 4, 8: all inside the thread's keys
#pragma unroll
    for (int kk = 2; kk <= 8; kk <<= 1)
#pragma unroll
        for (int j = kk >> 1; j >= 1; j >>= 1)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if ((e ^ j) > e) rank_ce(k[e], p[e], k[e ^ j], p[e ^ j], kk < 8 ? (e & kk) == 0 : (tl & 1) == 0);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s_key[own + e] = k[e]; s_pay[own + e] = p[e]; }
    for (int kk = 16; kk <= CH; kk <<= 1) {
        for (int j = kk >> 1; j >= 8; j >>= 1) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int q = m * NT + tl;                                           // pair of the chunk, lanes consecutive
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i + j;
                const uint64_t ka = s_key[i], kb = s_key[l];
                const uint32_t pa = s_pay[i], pb = s_pay[l];
                const bool gt = ka > kb || (ka == kb && pa > pb);
                if (gt == ((i & kk) == 0)) {
                    s_key[i] = kb; s_key[l] = ka;
                    s_pay[i] = pb; s_pay[l] = pa;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) { k[e] = s_key[own + e]; p[e] = s_pay[own + e]; }
        label_reg_stages(k, p, (own & kk) == 0);
#pragma unroll
        for (int e = 0; e < 8; ++e) { s_key[own + e] = k[e]; s_pay[own + e] = p[e]; }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = m * NT + tl;
        gk[i] = s_key[i];
        gp[i] = s_pay[i];
    }
}

// how many of the first `diag` outputs of merging a[0 .. na) with b[0 .. nb) come from a (equal pairs: a first)
template <typename I>
__device__ __forceinline__ I label_merge_path(const uint64_t *ak, const uint32_t *ap, I na, const uint64_t *bk, const uint32_t *bp, I nb, I diag)
{
    I lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;                     // mid < na and 0 <= diag - 1 - mid < nb
        if (label_le(ak[mid], ap[mid], bk[diag - 1 - mid], bp[diag - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int TILE>
__global__ void __launch_bounds__(TILE / 8) llda_label_merge_kernel(const LabelParams P, const int flip)
{
    constexpr int NT = TILE / 8;
    __shared__ uint64_t s_key[TILE];
    __shared__ uint32_t s_pay[TILE];
    __shared__ int64_t s_split[2];
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)blockIdx.y * P.Dp;
    const uint64_t *sk = (flip ? P.key_b : P.key_a) + row;
    const uint32_t *sp = (flip ? P.pay_b : P.pay_a) + row;
    uint64_t *dk = (flip ? P.key_a : P.key_b) + row;
    uint32_t *dp = (flip ? P.pay_a : P.pay_b) + row;
    const int64_t o0 = (int64_t)blockIdx.x * TILE, R = P.run;
    const int64_t base = o0 / (2 * R) * (2 * R);
    if (base + R >= P.Dp) {                               // a run without a partner
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int64_t i = o0 + m * NT + tid;
            dk[i] = sk[i];
            dp[i] = sp[i];
        }
        return;
    }
    const int64_t na = R, nb = P.Dp - base - R < R ? P.Dp - base - R : R;            // (both multiples of TILE)
    const uint64_t *ak = sk + base, *bk = ak + R;
    const uint32_t *ap = sp + base, *bp = ap + R;
    if (tid < 2) s_split[tid] = label_merge_path<int64_t>(ak, ap, na, bk, bp, nb, o0 - base + tid * TILE);
    __syncthreads();
    const int64_t a0 = s_split[0], b0 = o0 - base - a0;
    const int ca = (int)(s_split[1] - a0), cb = TILE - ca;                           // pairs of the tile from either run
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = m * NT + tid;
        const int64_t src = i < ca ? a0 + i : R + b0 + (i - ca);
        s_key[i] = ak[src];
        s_pay[i] = ap[src];
    }
    __syncthreads();
    const int dg = tid * 8;
    uint64_t ok[8];
    uint32_t op[8];
    {
        int i = label_merge_path<int>(s_key, s_pay, ca, s_key + ca, s_pay + ca, cb, dg), j = dg - i;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool from_a = j >= cb || (i < ca && label_le(s_key[i], s_pay[i], s_key[ca + j], s_pay[ca + j]));
            const int at = from_a ? i : ca + j;
            ok[e] = s_key[at];
            op[e] = s_pay[at];
            i += from_a ? 1 : 0;
            j += from_a ? 0 : 1;
        }
    }
    __syncthreads();                                      // the outputs leave through the same LDS: coalesced stores
#pragma unroll
    for (int e = 0; e < 8; ++e) { s_key[dg + e] = ok[e]; s_pay[dg + e] = op[e]; }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = m * NT + tid;
        dk[o0 + i] = s_key[i];
        dp[o0 + i] = s_pay[i];
    }
}

// is num / den larger than best_num / best_den (none yet: best_den = 0)?  Factors up to 2^31: the products fit 64 bits
__device__ __forceinline__ bool label_f1_better(int64_t num, int64_t den, int64_t best_num, int64_t best_den)
{
    return best_den == 0 || (uint64_t)num * (uint64_t)best_den > (uint64_t)best_num * (uint64_t)den;
}

__global__ void __launch_bounds__(LABEL_WALK_NT) llda_label_walk_kernel(const LabelParams P)
{
    constexpr int NT = LABEL_WALK_NT;
    __shared__ int32_t s_tp[LABEL_TILE];                  // truths of the tile up to every position
    __shared__ int32_t s_a[2][NT];                        // scan: truths
    __shared__ int32_t s_b[2][NT];                        // scan: last threshold position + 1 (within the tile)
    __shared__ uint64_t s_r[4][NT];                       // final reduction: A, T, best num << 32 | den, best start

    const int tid = threadIdx.x;
    const int l = blockIdx.x;
    const int64_t D = P.D;
    const uint64_t *key = P.key_sorted + (int64_t)l * P.Dp;
    const uint32_t *pay = P.pay_sorted + (int64_t)l * P.Dp;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    int32_t *order = P.order ? P.order + (int64_t)l * D : nullptr;

    const uint64_t k_first = key[0], k_last = key[D - 1];
    if (k_first < LABEL_KEY_POS_INF || k_last > LABEL_KEY_NEG_INF) {                 // a NaN in the column
        if (order)
            for (int64_t i = tid; i < D; i += NT) order[i] = -1;
        if (tid == 0) {
            if (P.n_pos) P.n_pos[l] = 0;
            if (P.n_thr) P.n_thr[l] = 0;
            if (P.auc_num) P.auc_num[l] = 0;
            if (P.auc) P.auc[l] = nan;
            if (P.thr_tp) P.thr_tp[l] = 0;
            if (P.thr_fp) P.thr_fp[l] = 0;
            if (P.f1) P.f1[l] = nan;
            if (P.thr) P.thr[l] = nan;
            if (P.flags) P.flags[l] = 16;
        }
        return;
    }

    // ---- P: the label's positives
    int64_t n_pos;
    {
        int64_t c = 0;
        for (int64_t i = tid; i < D; i += NT) c += pay[i] & 1u;
        s_r[0][tid] = (uint64_t)c;
        for (int off = NT >> 1; off >= 1; off >>= 1) {
            __syncthreads();
            if (tid < off) s_r[0][tid] += s_r[0][tid + off];
        }
        __syncthreads();
        n_pos = (int64_t)s_r[0][0];
    }

    int64_t carry_tp = 0, carry_ptp = 0, carry_pfp = 0;   // truths before the tile; (tp, fp) of the last threshold before the tile
    uint64_t area = 0;
    int64_t n_thr = 0, best_num = 0, best_den = 0, best_start = 0;
    for (int64_t t0 = 0; t0 < D; t0 += LABEL_TILE) {
        const int own = tid * 8;
        const int64_t p0 = t0 + own;
        uint64_t k[9];
        uint32_t tr = 0, ends = 0;
        int c = 0, last_end = 0;
#pragma unroll
        for (int e = 0; e < 9; ++e) k[e] = p0 + e < D ? key[p0 + e] : RANK_KEY_PAD;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t pos = p0 + e;
            if (pos < D) {
                const uint32_t py = pay[pos];
                if (order) order[pos] = (int32_t)(py >> 1);
                if (pos == D - 1 || k[e] != k[e + 1]) { ends |= 1u << e; last_end = own + e + 1; }
                if (py & 1u) { tr |= 1u << e; ++c; }
            }
        }
        // ---- scan over the workgroup: truths before the thread, last threshold of the tile before the thread
        int vs = c, vm = last_end, buf = 0;
        __syncthreads();                                  // (the previous tile's LDS is no longer read)
        s_a[0][tid] = vs; s_b[0][tid] = vm;
        for (int off = 1; off < NT; off <<= 1) {
            __syncthreads();
            if (tid >= off) { vs += s_a[buf][tid - off]; vm = max(vm, s_b[buf][tid - off]); }
            buf ^= 1;
            s_a[buf][tid] = vs; s_b[buf][tid] = vm;
        }
        {
            int run = vs - c;
#pragma unroll
            for (int e = 0; e < 8; ++e) { run += (tr >> e) & 1u; s_tp[own + e] = run; }
        }
        __syncthreads();
        const int tp_before = tid ? s_a[buf][tid - 1] : 0;
        const int prev_end = tid ? s_b[buf][tid - 1] : 0;                            // 0: no threshold of this tile before the thread
        const int tile_tp = s_a[buf][NT - 1], tile_end = s_b[buf][NT - 1];
        // ---- walk
        int64_t run_tp = carry_tp + tp_before;
        int64_t prev_tp = prev_end ? carry_tp + s_tp[prev_end - 1] : carry_ptp;
        int64_t prev_fp = prev_end ? t0 + prev_end - prev_tp : carry_pfp;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t pos = p0 + e;
            if ((tr >> e) & 1u) ++run_tp;
            if ((ends >> e) & 1u) {
                const int64_t fp = pos + 1 - run_tp;
                ++n_thr;
                area += (uint64_t)(fp - prev_fp) * (uint64_t)(run_tp + prev_tp);
                if (run_tp > 0) {
                    const int64_t num = 2 * run_tp, den = pos + 1 + n_pos;           // 2 tp / (tp + fp + P)
                    if (label_f1_better(num, den, best_num, best_den)) { best_num = num; best_den = den; best_start = prev_tp + prev_fp; }
                }
                prev_tp = run_tp; prev_fp = fp;
            }
        }
        // ---- carries (the same in every thread)
        if (tile_end) {
            carry_ptp = carry_tp + s_tp[tile_end - 1];
            carry_pfp = t0 + tile_end - carry_ptp;
        }
        carry_tp += tile_tp;
    }
    // ---- reduction: sums of A and T; the best F1, equal rationals to the earlier position
    __syncthreads();
    s_r[0][tid] = area; s_r[1][tid] = (uint64_t)n_thr; s_r[2][tid] = ((uint64_t)best_num << 32) | (uint64_t)best_den; s_r[3][tid] = (uint64_t)best_start;
    for (int off = NT >> 1; off >= 1; off >>= 1) {
        __syncthreads();
        if (tid < off) {
            s_r[0][tid] += s_r[0][tid + off];
            s_r[1][tid] += s_r[1][tid + off];
            const uint64_t m = s_r[2][tid], o = s_r[2][tid + off];
            const int64_t m_num = (int64_t)(m >> 32), m_den = (int64_t)(m & 0xFFFFFFFFu), o_num = (int64_t)(o >> 32), o_den = (int64_t)(o & 0xFFFFFFFFu);
            if (o_den != 0) {
                const uint64_t lhs = (uint64_t)o_num * (uint64_t)m_den, rhs = (uint64_t)m_num * (uint64_t)o_den;
                if (m_den == 0 || lhs > rhs || (lhs == rhs && s_r[3][tid + off] < s_r[3][tid])) { s_r[2][tid] = o; s_r[3][tid] = s_r[3][tid + off]; }
            }
        }
    }
    if (tid == 0) {
        const uint64_t A = s_r[0][0], b = s_r[2][0];
        const int64_t T = (int64_t)s_r[1][0], n_neg = D - n_pos;
        const int64_t b_num = (int64_t)(b >> 32), b_den = (int64_t)(b & 0xFFFFFFFFu), b_tp = b_num >> 1;
        int fl = 0;
        if (n_pos == 0) fl |= 1;
        if (n_neg == 0) fl |= 2;
        if (T < 2) fl |= 4;
        if (k_first == RANK_KEY_ZERO && k_last == RANK_KEY_ZERO) fl |= 8;
        if (P.n_pos) P.n_pos[l] = n_pos;
        if (P.n_thr) P.n_thr[l] = T;
        if (P.auc_num) P.auc_num[l] = A;
        if (P.auc) P.auc[l] = (n_pos == 0 || n_neg == 0) ? nan : (double)A / (double)(2 * n_pos * n_neg);
        if (P.thr_tp) P.thr_tp[l] = b_den ? b_tp : 0;
        if (P.thr_fp) P.thr_fp[l] = b_den ? b_den - n_pos - b_tp : 0;
        if (P.f1) P.f1[l] = b_den ? (double)b_num / (double)b_den : nan;
        if (P.thr) P.thr[l] = b_den ? P.score[(int64_t)(pay[s_r[3][0]] >> 1) * P.ld + P.first + l] : nan;
        if (P.flags) P.flags[l] = fl;
    }
}

// ---------------------------------------------------------------------------------------------
// llda_label_sets (include/llda_gibbs.h): one wavefront per document, lanes over columns, four documents per workgroup and round.
// Pass A over the columns: the ballot of score >= thr gives 64 bits of the mask at a time (kept in LDS), and the wavefront reduces
// the number of predictions, whether an eligible score is a NaN, and the best eligible label by (rank_key, topic id).  Then the mask
// is settled (cleared for a NaN document; the best label's bit for an empty one with at_least_one) and written; with truth, pass B
// over the columns counts hits and adds tp / fp / fn to the workgroup's LDS counters, which leave with one 64-bit integer atomic per
// label and workgroup at the end: integer sums, the same whatever the order.
// ---------------------------------------------------------------------------------------------
struct SetsParams {
    const double *score, *thr;
    const uint8_t *truth;
    int64_t D, ld;
    int32_t K, first, at_least_one, W;
    uint32_t *mask;
    int32_t *n_pred, *n_hit, *n_true;
    unsigned long long *tp, *fp, *fn;
};

constexpr int SETS_WAVES = 4;
constexpr int SETS_MAX_BLOCKS = 1024;                     // workgroups at most: each takes its rounds of SETS_WAVES documents in turn

__global__ void __launch_bounds__(SETS_WAVES * 64) llda_label_sets_kernel(const SetsParams P)
{
    extern __shared__ uint32_t sets_lds[];
    const int K = P.K, W2 = (K + 63) / 64 * 2;            // mask words of a wavefront in LDS: whole ballots
    uint32_t *s_mask = sets_lds;                          // [SETS_WAVES][W2]
    uint32_t *s_cnt = sets_lds + SETS_WAVES * W2;         // [3][K], with truth only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *my = s_mask + wave * W2;
    if (P.truth)
        for (int i = tid; i < 3 * K; i += SETS_WAVES * 64) s_cnt[i] = 0;
    __syncthreads();
    for (int64_t d = (int64_t)blockIdx.x * SETS_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * SETS_WAVES) {
        const double *srow = P.score + d * P.ld;
        int n_pred = 0;
        bool has_nan = false;
        uint64_t best_key = RANK_KEY_PAD;
        int best_k = 0x7FFFFFFF;
        for (int c0 = 0; c0 < K; c0 += 64) {
            const int k = c0 + lane;
            bool pred = false;
            if (k >= P.first && k < K) {
                const double th = P.thr[k], s = srow[k];
                if (th == th) {                           // an eligible column
                    if (s != s) has_nan = true;
                    else {
                        pred = s >= th;
                        const uint64_t key = rank_key((uint64_t)__double_as_longlong(s));
                        if (key < best_key) { best_key = key; best_k = k; }          // (k ascends: the first of equal keys stays)
                    }
                }
            }
            const uint64_t b = __ballot(pred);
            n_pred += __popcll(b);
            if (lane == 0) { my[c0 / 32] = (uint32_t)b; my[c0 / 32 + 1] = (uint32_t)(b >> 32); }
        }
        has_nan = __any(has_nan);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint64_t ok = __shfl_xor((unsigned long long)best_key, off);
            const int okk = __shfl_xor(best_k, off);
            if (ok < best_key || (ok == best_key && okk < best_k)) { best_key = ok; best_k = okk; }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (has_nan) {
            for (int w = lane; w < W2; w += 64) my[w] = 0;
            n_pred = -1;
        } else if (n_pred == 0 && P.at_least_one && best_k != 0x7FFFFFFF) {
            if (lane == 0) my[best_k >> 5] = 1u << (best_k & 31);
            n_pred = 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (P.mask)
            for (int w = lane; w < P.W; w += 64) P.mask[d * P.W + w] = my[w];
        if (lane == 0 && P.n_pred) P.n_pred[d] = n_pred;
        if (P.truth) {
            const uint8_t *trow = P.truth + d * (int64_t)K;
            int n_hit = 0, n_true = 0;
            for (int c0 = 0; c0 < K; c0 += 64) {
                const int k = c0 + lane;
                if (k >= P.first && k < K) {
                    const bool t = trow[k] != 0, pr = (my[k >> 5] >> (k & 31)) & 1u;
                    if (t) ++n_true;
                    if (t && pr) { ++n_hit; atomicAdd(&s_cnt[k], 1u); }
                    else if (pr) atomicAdd(&s_cnt[K + k], 1u);
                    else if (t) atomicAdd(&s_cnt[2 * K + k], 1u);
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { n_hit += __shfl_xor(n_hit, off); n_true += __shfl_xor(n_true, off); }
            if (lane == 0) {
                if (P.n_hit) P.n_hit[d] = n_hit;
                if (P.n_true) P.n_true[d] = n_true;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();                  // (the mask words are rewritten in the next round)
    }
    if (P.truth) {
        __syncthreads();
        for (int k = tid; k < K; k += SETS_WAVES * 64) {
            const uint32_t a = s_cnt[k], b = s_cnt[K + k], c = s_cnt[2 * K + k];
            if (a && P.tp) atomicAdd(&P.tp[k], (unsigned long long)a);
            if (b && P.fp) atomicAdd(&P.fp[k], (unsigned long long)b);
            if (c && P.fn) atomicAdd(&P.fn[k], (unsigned long long)c);
        }
    }
}

}  // namespace
