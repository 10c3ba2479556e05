// kernel_attr.hpp -- llda_attr_wave_kernel, llda_attr_lds_kernel, llda_attr_group_kernel: per-word label shares and the EM fold-in
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_attribute (include/llda_gibbs.h): the E-step of the document model -- every site's posterior share per label against the
// document's loads, r_k = theta_k phi_t[w][k] / p, added up (times f) as the document's credit -- and, iterated with the M-step
// theta_k = (credit_k + alpha) / sum, a fold-in without random numbers.
//
// Arithmetic (fixed by the header, restated in tests/attrref.py): IEEE float64 operations, each rounded on its own (contraction
// is off in this unit; the two divisions are the correctly rounded ones).  p is the sum of kernel_heldout.hpp -- 64 partials, then
// the xor tree (heldout_tree) -- and so is the M-step's denominator.  ONE division per site (inv = 1 / p): f * inv is the site's
// weight and t_k * inv its shares.  A site is good when its word is in [0, V) and 2^-960 <= p < inf; any other adds f to bad.
//
// Geometry, as in kernel_heldout.hpp.  32 < K <= 1024: one wavefront per document, lane j on the topics j + 64 i; theta and the
// credit stay in NI = 1 .. 16 registers per lane each and U sites are in flight.  K > 1024 (llda_attr_lds_kernel): both rows live
// in LDS, 16 K bytes, one wavefront per workgroup; every lane reads and writes its own columns only, so no barrier is needed, and
// a site's row is read twice (the second time from the caches).  K <= 32: a group of G = 8, 16 or 32 lanes per document; the groups
// of a wavefront walk to their longest document.  All iters steps of a document run inside the launch: pass 0 .. iters over its
// sites, the M-step between two passes; the last pass leaves the credit and, when asked for, every site's best labels: at most four
// rounds of "the best key after the one taken last" (r descending, then topic ascending), a wave-wide exchange each.
// The whole row of phi_t is read even where theta is 0.  A document's outputs depend on its own inputs only.
// ---------------------------------------------------------------------------------------------
struct AttrParams {
    const int64_t *doc_off;
    const int32_t *word;
    const int32_t *freq;
    const double *theta;
    const double *phi_t;
    int64_t D, V, ld_theta, ld_phi, ld_out, ld_credit;
    int32_t K, iters, top_m;
    double alpha;
    double *theta_out;
    double *credit;
    int32_t *site_idx;
    double *site_val;
    int64_t *tok;
    int64_t *bad;
};

constexpr int ATTR_WAVES = 4;                           // wavefronts of a workgroup (wave and group kernels)
constexpr int ATTR_MAX_TOP = 4;

__device__ __forceinline__ bool attr_good(double p)
{
    return p >= __longlong_as_double(0x03F0000000000000ll) && p < __longlong_as_double(0x7FF0000000000000ll);     // 2^-960, inf
}

// the order of a site's labels: r descending, then topic ascending
__device__ __forceinline__ bool attr_before(double r, int k, double r2, int k2) { return r > r2 || (r == r2 && k < k2); }

// (r, k) of the lane -> the first key of the G lanes' keys in that order, in every lane
template <int G>
__device__ __forceinline__ void attr_first(double &r, int &k)
{
#pragma unroll
    for (int s = 1; s < G; s <<= 1) {
        const double r2 = __shfl_xor(r, s, 64);
        const int k2 = __shfl_xor(k, s, 64);
        const bool take = attr_before(r2, k2, r, k);
        r = take ? r2 : r;
        k = take ? k2 : k;
    }
}

// a site that is not good: all -1 / 0.0
__device__ __forceinline__ void attr_site_none(const AttrParams &P, int64_t s)
{
    for (int m = 0; m < P.top_m; ++m) {
        P.site_idx[s * P.top_m + m] = -1;
        P.site_val[s * P.top_m + m] = 0.0;
    }
}

__device__ __forceinline__ void attr_site_put(const AttrParams &P, int64_t s, int m, double r, int k)
{
    const bool some = r > 0.0;
    P.site_idx[s * P.top_m + m] = some ? k : -1;
    P.site_val[s * P.top_m + m] = some ? r : 0.0;
}

// one candidate (r, k) of the lane: it becomes the lane's key (br, bk) when it has a share, comes after the key taken last (pr, pk)
// and before the lane's key so far
__device__ __forceinline__ void attr_offer(double r, int k, double pr, int pk, double &br, int &bk)
{
    const bool cand = r > 0.0 && attr_before(pr, pk, r, k);
    if (cand && attr_before(r, k, br, bk)) { br = r; bk = k; }
}

// the best top_m labels of the good site s: rounds of "the first key after the one taken last" over the G lanes; offer(pr, pk, br, bk)
// runs attr_offer over the lane's own labels; the lane with store set writes (every lane of the wavefront takes part in the exchange)
template <int G, typename F>
__device__ __forceinline__ void attr_site_top(const AttrParams &P, int64_t s, bool store, F &&offer)
{
    double pr = __longlong_as_double(0x7FF0000000000000ll);                // before every key
    int pk = -1;
    for (int m = 0; m < P.top_m; ++m) {
        double br = 0.0;                                                    // none: what the padding stores
        int bk = 0x7FFFFFFF;
        offer(pr, pk, br, bk);
        attr_first<G>(br, bk);
        if (store) attr_site_put(P, s, m, br, bk);
        pr = br; pk = bk;
    }
}

// the M-step of one lane's NI values: num, its tree, the division (go: the lane's document has sites)
template <int NI, int G>
__device__ __forceinline__ void attr_mstep(double (&th)[NI], const double (&credit)[NI], uint32_t in, double alpha, bool go)
{
    double num[NI], part = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        num[i] = ((in >> i & 1u) && th[i] > 0.0) ? credit[i] + alpha : 0.0;
        part = (in >> i & 1u) ? part + num[i] : part;
    }
    const double den = heldout_tree<G>(part);
    if (go && den > 0.0 && den < __longlong_as_double(0x7FF0000000000000ll)) {
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = num[i] / den;
    }
}

template <int NI, int U, bool SITES>
__global__ void __launch_bounds__(64 * ATTR_WAVES) llda_attr_wave_kernel(const AttrParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = P.K;
    int kc[NI];                                         // the lane's columns; column 0 where it has none
    uint32_t in = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int k = lane + 64 * i;
        kc[i] = k < K ? k : 0;
        if (k < K) in |= 1u << i;
    }
    for (int64_t d = (int64_t)blockIdx.x * ATTR_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * ATTR_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        const double *trow = P.theta + d * P.ld_theta;
        double th[NI], credit[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = trow[kc[i]];
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters || b == e;     // (a document without sites takes no step)
            tok = 0; bad = 0;
#pragma unroll
            for (int i = 0; i < NI; ++i) credit[i] = 0.0;
            for (int64_t s0 = b; s0 < e; s0 += 64) {
                const int n = (int)(e - s0 < 64 ? e - s0 : 64);
                const int32_t wv = lane < n ? P.word[s0 + lane] : -1;
                const int32_t fv = lane < n ? (P.freq ? P.freq[s0 + lane] : 1) : 0;
                for (int t = 0; t < n; t += U) {
                    int32_t f[U];
                    bool ok[U];
                    double v[U][NI];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int tt = t + u < n ? t + u : n - 1;                    // (a repeat of the last site, not used)
                        const int32_t w = __builtin_amdgcn_readlane(wv, tt);
                        f[u] = __builtin_amdgcn_readlane(fv, tt);
                        ok[u] = heldout_word_ok(w, P.V);
                        const double *row = P.phi_t + (int64_t)(ok[u] ? w : 0) * P.ld_phi;
#pragma unroll
                        for (int i = 0; i < NI; ++i) v[u][i] = row[kc[i]];
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (t + u >= n) break;
                        double part = 0.0;
#pragma unroll
                        for (int i = 0; i < NI; ++i) {
                            v[u][i] = th[i] * v[u][i];                               // t_k
                            part = (in >> i & 1u) ? part + v[u][i] : part;
                        }
                        const double p = heldout_tree<64>(part);
                        const bool good = ok[u] && attr_good(p);
                        tok += good ? f[u] : 0;
                        bad += good ? 0 : f[u];
                        if (!good) {
                            if (SITES && last && lane == 0) attr_site_none(P, s0 + t + u);
                            continue;
                        }
                        const double inv = 1.0 / p;
                        const double g = (double)f[u] * inv;
#pragma unroll
                        for (int i = 0; i < NI; ++i) credit[i] = credit[i] + v[u][i] * g;
                        if (SITES && last)
                            attr_site_top<64>(P, s0 + t + u, lane == 0, [&](double pr, int pk, double &br, int &bk) {
#pragma unroll
                                for (int i = 0; i < NI; ++i)
                                    if (in >> i & 1u) attr_offer(v[u][i] * inv, lane + 64 * i, pr, pk, br, bk);
                            });
                    }
                }
            }
            if (last) break;
            attr_mstep<NI, 64>(th, credit, in, P.alpha, true);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (in >> i & 1u) {
                if (P.theta_out) P.theta_out[d * P.ld_out + kc[i]] = th[i];
                if (P.credit) P.credit[d * P.ld_credit + kc[i]] = credit[i];
            }
        }
        if (lane == 0) {
            if (P.tok) P.tok[d] = tok;
            if (P.bad) P.bad[d] = bad;
        }
    }
}

// K > 1024: theta and the credit of the document in LDS (dynamic: 16 K bytes), one wavefront per workgroup.  Lane j touches the
// entries j + 64 i of both rows and no other: nothing is shared between lanes, so there is no barrier.
template <bool SITES>
__global__ void __launch_bounds__(64) llda_attr_lds_kernel(const AttrParams P)
{
    extern __shared__ double attr_lds[];
    const int lane = threadIdx.x;
    const int K = P.K;
    double *th = attr_lds, *credit = attr_lds + K;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int64_t d = blockIdx.x; d < P.D; d += gridDim.x) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        const double *trow = P.theta + d * P.ld_theta;
        for (int k = lane; k < K; k += 64) th[k] = trow[k];
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters || b == e;     // (a document without sites takes no step)
            tok = 0; bad = 0;
            for (int k = lane; k < K; k += 64) credit[k] = 0.0;
            for (int64_t s0 = b; s0 < e; s0 += 64) {
                const int n = (int)(e - s0 < 64 ? e - s0 : 64);
                const int32_t wv = lane < n ? P.word[s0 + lane] : -1;
                const int32_t fv = lane < n ? (P.freq ? P.freq[s0 + lane] : 1) : 0;
                for (int t = 0; t < n; ++t) {
                    const int32_t w = __builtin_amdgcn_readlane(wv, t), f = __builtin_amdgcn_readlane(fv, t);
                    const bool ok = heldout_word_ok(w, P.V);
                    const double *row = P.phi_t + (int64_t)(ok ? w : 0) * P.ld_phi;
                    double part = 0.0;
#pragma unroll 8
                    for (int k = lane; k < K; k += 64) part = part + th[k] * row[k];
                    const double p = heldout_tree<64>(part);
                    const bool good = ok && attr_good(p);
                    tok += good ? f : 0;
                    bad += good ? 0 : f;
                    if (!good) {
                        if (SITES && last && lane == 0) attr_site_none(P, s0 + t);
                        continue;
                    }
                    const double inv = 1.0 / p;
                    const double g = (double)f * inv;
#pragma unroll 8
                    for (int k = lane; k < K; k += 64) credit[k] = credit[k] + (th[k] * row[k]) * g;
                    if (SITES && last)
                        attr_site_top<64>(P, s0 + t, lane == 0, [&](double pr, int pk, double &br, int &bk) {
                            for (int k = lane; k < K; k += 64) attr_offer((th[k] * row[k]) * inv, k, pr, pk, br, bk);
                        });
                }
            }
            if (last) break;
            double part = 0.0;                          // the M-step; num takes the credit's place
            for (int k = lane; k < K; k += 64) {
                const double num = th[k] > 0.0 ? credit[k] + P.alpha : 0.0;
                credit[k] = num;
                part = part + num;
            }
            const double den = heldout_tree<64>(part);
            if (den > 0.0 && den < inf)
                for (int k = lane; k < K; k += 64) th[k] = credit[k] / den;
        }
        for (int k = lane; k < K; k += 64) {
            if (P.theta_out) P.theta_out[d * P.ld_out + k] = th[k];
            if (P.credit) P.credit[d * P.ld_credit + k] = credit[k];
        }
        if (lane == 0) {
            if (P.tok) P.tok[d] = tok;
            if (P.bad) P.bad[d] = bad;
        }
    }
}

// K <= G <= 32: 64 / G documents per wavefront
template <int G, bool SITES>
__global__ void __launch_bounds__(64 * ATTR_WAVES) llda_attr_group_kernel(const AttrParams P, const int64_t n_tiles)
{
    constexpr int DPB = 64 * ATTR_WAVES / G;            // documents of a workgroup
    constexpr int U = 4;
    const int gl = threadIdx.x % G, dl = threadIdx.x / G;
    const bool mine = gl < P.K;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t d = tile * DPB + dl;
        const bool active = d < P.D;
        const int64_t b = active ? P.doc_off[d] : 0, n = active ? P.doc_off[d + 1] - b : 0;
        int64_t n_max = n;                              // the longest document of the wavefront
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            const int64_t o = __shfl_xor(n_max, s, 64);
            n_max = o > n_max ? o : n_max;
        }
        double th[1] = {(active && mine) ? P.theta[d * P.ld_theta + gl] : 0.0}, credit[1] = {0.0};
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters;
            tok = 0; bad = 0;
            credit[0] = 0.0;
            for (int64_t t = 0; t < n_max; t += U) {
                int32_t f[U];
                bool ok[U];
                double v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const bool live = t + u < n;
                    const int32_t w = live ? P.word[b + t + u] : -1;
                    f[u] = live ? (P.freq ? P.freq[b + t + u] : 1) : 0;
                    ok[u] = heldout_word_ok(w, P.V);
                    v[u] = (ok[u] && mine) ? P.phi_t[(int64_t)w * P.ld_phi + gl] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double tk = th[0] * v[u];
                    double part = 0.0;
                    if (ok[u] && mine) part = part + tk;
                    const double p = heldout_tree<G>(part);
                    const bool live = t + u < n;
                    const bool good = ok[u] && attr_good(p);
                    tok += good ? f[u] : 0;                                          // (a site past the document's end: f = 0)
                    bad += good ? 0 : f[u];
                    const double inv = good ? 1.0 / p : 0.0;
                    if (good && mine) credit[0] = credit[0] + tk * ((double)f[u] * inv);
                    if (SITES && last)                                               // (a site that is not good offers nothing: all -1 / 0.0)
                        attr_site_top<G>(P, b + t + u, live && gl == 0, [&](double pr, int pk, double &br, int &bk) {
                            if (good && mine) attr_offer(tk * inv, gl, pr, pk, br, bk);
                        });
                }
            }
            if (last) break;
            attr_mstep<1, G>(th, credit, mine ? 1u : 0u, P.alpha, n > 0);      // (a document without sites takes no step)
        }
        if (active && mine) {
            if (P.theta_out) P.theta_out[d * P.ld_out + gl] = th[0];
            if (P.credit) P.credit[d * P.ld_credit + gl] = credit[0];
        }
        if (active && gl == 0) {
            if (P.tok) P.tok[d] = tok;
            if (P.bad) P.bad[d] = bad;
        }
    }
}

}  // namespace
