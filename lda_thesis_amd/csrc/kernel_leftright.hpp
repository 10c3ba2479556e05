// kernel_leftright.hpp -- llda_leftright_kernel: the left-to-right estimate of p(w_d | phi, alpha), a particle sampler per document
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_left_to_right (include/llda_gibbs.h): Wallach, Murray, Salakhutdinov and Mimno (ICML 2009), Algorithm 3, with R particles
// per document.  The output is llda_heldout_loglik's: the product of the positions' p_n as a pair (mantissa in
// [0.5, 1), 64-bit exponent), the scored tokens and the bad ones.
//
// Arithmetic (fixed by the header, restated in tests/leftrightref.py).  Every operation is one IEEE float64 operation rounded on its
// own.  Topic k belongs to lane k mod 64, slot k / 64 (the plain 64-lane layout -- not a group layout).  For a particle with the
// counts c and a word w:  x[k] = ((double)c[k] + alpha) * phi_t[w][k] where k is allowed, +0.0 elsewhere.
//   draw64(x, u)   q[j][i] the lane's inclusive prefix over its slots; X the Hillis-Steele scan of the lane totals; t = u * X[63];
//                  t_j = t - X[j-1], X[-1] = 0; the first (j, i), lanes first, with x > 0 and q[j][i] > t_j, else the last with
//                  x > 0, else none.  No division: the weights are not normalised.
//   sum64(x)       llda_heldout_loglik's: the lane's partial over its slots from +0.0, then part[j] + part[j ^ s], s = 1 .. 32.
//   position n     every particle r: for m = 0 .. n-1 that hold an assignment: c[z[m]] -= 1; z[m] = draw64(x of w_m, u(n, r, m)) (the
//                  old topic when the draw finds none); c[z[m]] += 1.  Then S = sum64(x of w_n), pred_r = S / (assigned + A * alpha)
//                  and, when 0 < S < inf, z[n] = draw64(x, u(n, r, n)), c[z[n]] += 1 (else, or when the draw finds none, the
//                  position stays without an assignment in this particle).  A word outside [0, V) is never used as an index:
//                  the earlier positions are resampled all the same, pred_r is NaN and the position stays unassigned.
//                  p_n = (pred_0 + ... + pred_{R-1}) / R, added in increasing r from +0.0; 0 < p_n < inf: tok += 1 and the
//                  document's pair *= frexp(p_n); else bad += 1.
//   u(n, r, m)     the keyed uniform of Philox counter (m >> 1, doc id, stream_id + r, n): words (0, 1) for an even m, (2, 3) for an
//                  odd one (oracle/llda_oracle.py keyed_uniform).
//
// Geometry.  One workgroup per document, one wavefront per particle: the particle's counts stay in NI = K / 64 (rounded up to 1, 2,
// 4, 8, 16) registers per lane, its assignments (16 bits each) and the document's words in LDS, sized by max_doc_tokens.  A lane
// whose topic is >= K reads a column < K and drops the value: no column >= K is read.  A wavefront generates the Philox blocks of 128
// positions m at a time, lane l the block (m >> 1) + l.  One barrier per position: the wavefronts leave their pred_r in LDS (two
// buffers, by the parity of n), wavefront 0 adds them in order and multiplies the pair.  Everything that decides a branch is
// uniform over the wavefront (m, n, the old topic, the word); the barrier is reached by every wavefront N times per document.
// A document's outputs depend on its own tokens, its id, its allowed row and the scalars only.
// ---------------------------------------------------------------------------------------------
struct LrParams {
    const int64_t *doc_off;
    const int32_t *word;
    const double *phi_t;
    const uint8_t *allowed;
    const int64_t *doc_ids;
    int64_t D, V, ld_phi, ld_allowed, doc_base;
    int32_t K, R, cap;                                  // cap: max_doc_tokens, the tokens the LDS arrays hold
    double alpha;
    uint32_t key0, key1, stream_id;
    double *mant;
    int64_t *expo;
    int64_t *tok;
    int64_t *bad;
    int32_t *status;
};

constexpr int LR_MAX_PARTICLES = 16;                    // LLDA_LR_MAX_PARTICLES
constexpr uint32_t LR_NONE = 0xFFFFu;                   // no assignment (K <= 1024: never a topic)
constexpr size_t LR_PRED_BYTES = 2 * LR_MAX_PARTICLES * sizeof(double);

// bytes of dynamic LDS: pred[2][16] doubles, word[cap] int32, z[R][cap] uint16
inline size_t lr_lds_bytes(int R, int cap) { return LR_PRED_BYTES + (size_t)cap * 4 + (size_t)R * cap * 2; }

// draw64: the topic, or -1 when no weight is > 0
template <int NI>
__device__ __forceinline__ int lr_draw(const double (&x)[NI], double u, int lane)
{
    // (NI = 16: the prefixes are formed twice, the same additions in the same order, instead of held in 32 registers)
    constexpr bool KEEP = NI < 16;
    double q[KEEP ? NI : 1];
    double run = x[0];
    if constexpr (KEEP) q[0] = run;
#pragma unroll
    for (int i = 1; i < NI; ++i) {
        run = run + x[i];
        if constexpr (KEEP) q[i] = run;
    }
    const double X = group_scan<64>(run, lane);
    const double t = u * readlane_f64(X, 63);
    const double prev = __shfl_up(X, 1, 64);
    const double tg = t - (lane ? prev : 0.0);
    uint32_t fm = 0, pm = 0;
    run = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const bool pos = x[i] > 0.0;
        double qi;
        if constexpr (KEEP) qi = q[i];
        else qi = run = i ? run + x[i] : x[0];
        pm |= (pos ? 1u : 0u) << i;
        fm |= ((pos && qi > tg) ? 1u : 0u) << i;
    }
    const uint64_t gf = __ballot(fm != 0), gp = __ballot(pm != 0);
    if (gp == 0) return -1;
    const bool hit = gf != 0;
    const int sl = hit ? (int)__ffsll((unsigned long long)gf) - 1 : 63 - (int)__clzll((unsigned long long)gp);
    const int my = hit ? (int)__ffs((int)(fm | 0x10000u)) - 1 : 31 - (int)__clz((int)(pm | 1u));
    return sl + 64 * __builtin_amdgcn_readlane(my, sl);
}

// c[topic] += -g  (onehot_add1 adds m * g with m = -1 at the topic's slot of its lane)
template <int NI>
__device__ __forceinline__ void lr_count(int (&c)[NI], int topic, int lane, int g)
{
    const uint32_t oh = lane == (topic & 63) ? 1u << (topic >> 6) : 0u;
    onehot_add1<NI>(c, oh, g);
}

// WAVES: the most particles the launch may have (8 or 16) -- with up to eight wavefronts in a workgroup a wavefront may hold 256
// registers, with sixteen 128
template <int NI, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) llda_leftright_kernel(const LrParams P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lr_lds[];
    const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;            // the block has 64 R threads: r < R
    const int K = P.K, cap = P.cap, R = P.R;
    double *s_pred = (double *)lr_lds;                                  // [2][LR_MAX_PARTICLES]
    int32_t *s_word = (int32_t *)(lr_lds + LR_PRED_BYTES);              // [cap]
    uint16_t *s_z = (uint16_t *)(s_word + cap) + (size_t)r * cap;       // [cap], this particle's
    const int col0 = lane < K ? lane : 0;
    const uint32_t in = lane < K ? (1u << ((K - 1 - lane) / 64 + 1)) - 1u : 0u;        // slot i: the lane has a topic there
    auto col = [&](const int i) { return (in >> i & 1u) ? lane + 64 * i : col0; };     // (a column < K in any case; the value is dropped)
    const double alpha = P.alpha, inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
    const uint32_t stream = P.stream_id + (uint32_t)r;
    for (int64_t d = blockIdx.x; d < P.D; d += gridDim.x) {
        const int64_t b = P.doc_off[d], len = P.doc_off[d + 1] - b;
        const bool over = len > (int64_t)cap;
        const int N = (len < 0 || over) ? 0 : (int)len;
        __syncthreads();                                                // the previous document's words and predictions are done with
        for (int i = threadIdx.x; i < N; i += blockDim.x) s_word[i] = P.word[b + i];
        __syncthreads();
        uint32_t am = 0;                                                // slot i: the lane has a topic there and it is allowed
        int A = 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const bool on = (in >> i & 1u) && (!P.allowed || P.allowed[d * P.ld_allowed + col(i)] != 0);
            am |= (on ? 1u : 0u) << i;
            A += (int)__popcll(__ballot(on));
        }
        const double a_alpha = (double)A * alpha;
        const uint32_t gdoc = P.doc_ids ? (uint32_t)P.doc_ids[d] : (uint32_t)(d + P.doc_base);
        int c[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) c[i] = 0;
        int assigned = 0;
        double dm = 0.5;                                                // the document's pair and counters (N <= 4096: 32 bits do)
        int de = 1, dtok = 0, dbad = 0;
        for (int n = 0; n < N; ++n) {
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            int batch = -1;                                             // the 128 positions m whose Philox blocks the lanes hold
            auto uniform = [&](const int m) {
                if ((m >> 7) != batch) {
                    batch = m >> 7;
                    r0 = (uint32_t)(batch << 6) + (uint32_t)lane; r1 = gdoc; r2 = stream; r3 = (uint32_t)n;
                    philox4x32_10(r0, r1, r2, r3, P.key0, P.key1);
                }
                const int holder = (m >> 1) & 63;
                const uint32_t ra = (uint32_t)__builtin_amdgcn_readlane((int)((m & 1) ? r2 : r0), holder);
                const uint32_t rb = (uint32_t)__builtin_amdgcn_readlane((int)((m & 1) ? r3 : r1), holder);
                return ((double)(ra >> 5) * 67108864.0 + (double)(rb >> 6)) * (1.0 / 9007199254740992.0);
            };
            auto weights = [&](const int w, double (&x)[NI]) {
                const double *row = P.phi_t + (int64_t)w * P.ld_phi;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    double v = 0.0;
                    if ((NI > 1 && i < NI / 2) || (in >> i & 1u)) v = row[lane + 64 * i];     // (K > 32 NI: the lower slots hold a topic in every lane)
                    const double t = ((double)c[i] + alpha) * v;
                    x[i] = (am >> i & 1u) ? t : 0.0;
                }
            };
            // m < n: resampling of the earlier positions that hold an assignment, in order; m == n: prediction and extension
            double pred = nan;
            for (int m = 0; m <= n; ++m) {
                const bool last = m == n;
                const int zo = last ? (int)LR_NONE : __builtin_amdgcn_readfirstlane((int)s_z[m]);
                if (!last && (uint32_t)zo == LR_NONE) continue;
                const int w = __builtin_amdgcn_readfirstlane(s_word[m]);
                const bool ok = word_ok(w, P.V);                       // (m < n: the position was assigned, so it is)
                if (!last) lr_count<NI>(c, zo, lane, 1);
                double x[NI];
                weights(ok ? w : 0, x);
                bool draw = true;
                if (last) {
                    double part = 0.0;
#pragma unroll
                    for (int i = 0; i < NI; ++i) part = part + x[i];
                    const double sum = doc_tree<64>(part);
                    const double S = ok ? sum : nan;
                    pred = S / ((double)assigned + a_alpha);
                    draw = S > 0.0 && S < inf;
                }
                int zn = draw ? lr_draw<NI>(x, uniform(m), lane) : -1;
                zn = zn < 0 ? zo : zn;                                  // (m < n: the old topic; m == n: none)
                if ((uint32_t)zn != LR_NONE) {
                    lr_count<NI>(c, zn, lane, -1);
                    assigned += last ? 1 : 0;
                }
                s_z[m] = (uint16_t)zn;                                  // (every lane the same value)
            }
            double *pr = s_pred + (n & 1) * LR_MAX_PARTICLES;
            pr[r] = pred;                                               // (every lane the same value)
            __syncthreads();
            if (r == 0) {
                double acc = 0.0;
                for (int i = 0; i < R; ++i) acc = acc + pr[i];
                const double p = acc / (double)R;
                const bool good = p > 0.0 && p < inf;
                dtok += good ? 1 : 0;
                dbad += good ? 0 : 1;
                if (good) pair_mul_frexp(dm, de, p);
            }
        }
        if (threadIdx.x == 0) {
            if (over && P.status) atomicOr(P.status, 1);
            P.mant[d] = dm; P.expo[d] = de; P.tok[d] = dtok; P.bad[d] = dbad;
        }
    }
}

}  // namespace
