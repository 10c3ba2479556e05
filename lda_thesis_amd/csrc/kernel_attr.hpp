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
// is off in this unit; the two divisions are the correctly rounded ones).  p is the sum of doc_model.hpp -- 64 partials, then
// the xor tree (doc_tree) -- and so is the M-step's denominator.  ONE division per site (inv = 1 / p): f * inv is the site's
// weight and t_k * inv its shares.  A site is good when its word is in [0, V) and 2^-960 <= p < inf; any other adds f to bad.
//
// Geometry: the walks of doc_model.hpp.  32 < K <= 1024: one wavefront per document, lane j on the topics j + 64 i; theta and the
// credit stay in NI = 1 .. 16 registers per lane each and U sites are in flight.  K > 1024 (llda_attr_lds_kernel): both rows live
// in LDS, 16 K bytes, one wavefront per workgroup; every lane reads and writes its own columns only, so no barrier is needed, and
// a site's row is read twice (the second time from the caches).  K <= 32: a group of G = 8, 16 or 32 lanes per document; the groups
// of a wavefront walk to their longest document.  All iters steps of a document run inside the launch: pass 0 .. iters over its
// sites, the M-step between two passes; the last pass leaves the credit and, when asked for, every site's best labels: at most four
// rounds of "the best key after the one taken last" (r descending, then topic ascending), a wave-wide exchange each.
// The whole row of phi_t is read even where theta is 0.  A document's outputs depend on its own inputs only.
// ---------------------------------------------------------------------------------------------
struct AttrParams : DocModel {
    int64_t ld_out, ld_credit;
    int32_t iters, top_m;
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
constexpr int64_t ATTR_LDS_MAX_BLOCKS = 1 << 16;        // workgroups of llda_attr_lds_kernel at most: each takes its documents in turn
constexpr int attr_u(int NI) { return NI <= 2 ? 4 : NI <= 8 ? 2 : 1; }     // sites in flight in the wave kernel: NI = 1, 2 | 4, 8 | 16

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
    const double den = doc_tree<G>(part);
    if (go && den > 0.0 && den < __longlong_as_double(0x7FF0000000000000ll)) {
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = num[i] / den;
    }
}

// the document's counters and outputs
__device__ __forceinline__ void attr_store(const AttrParams &P, int64_t d, int64_t tok, int64_t bad)
{
    if (P.tok) P.tok[d] = tok;
    if (P.bad) P.bad[d] = bad;
}

template <int NI, int U, bool SITES>
__global__ void __launch_bounds__(64 * ATTR_WAVES) llda_attr_wave_kernel(const AttrParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveCols<NI> C(lane, P.K);
    for (int64_t d = (int64_t)blockIdx.x * ATTR_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * ATTR_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        const double *trow = P.theta + d * P.ld_theta;
        double th[NI], credit[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = trow[C.kc[i]];
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters || b == e;     // (a document without sites takes no step)
            tok = 0; bad = 0;
#pragma unroll
            for (int i = 0; i < NI; ++i) credit[i] = 0.0;
            wave_sites<NI, U>(P, C, th, lane, b, e, [&](int64_t s, int32_t f, bool ok, double p, const double (&t)[NI]) {
                const bool good = ok && attr_good(p);
                tok += good ? f : 0;
                bad += good ? 0 : f;
                if (!good) {
                    if (SITES && last && lane == 0) attr_site_none(P, s);
                    return;
                }
                const double inv = 1.0 / p;
                const double g = (double)f * inv;
#pragma unroll
                for (int i = 0; i < NI; ++i) credit[i] = credit[i] + t[i] * g;
                if (SITES && last)
                    attr_site_top<64>(P, s, lane == 0, [&](double pr, int pk, double &br, int &bk) {
#pragma unroll
                        for (int i = 0; i < NI; ++i)
                            if (C.in >> i & 1u) attr_offer(t[i] * inv, lane + 64 * i, pr, pk, br, bk);
                    });
            });
            if (last) break;
            attr_mstep<NI, 64>(th, credit, C.in, P.alpha, true);
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (C.in >> i & 1u) {
                if (P.theta_out) P.theta_out[d * P.ld_out + C.kc[i]] = th[i];
                if (P.credit) P.credit[d * P.ld_credit + C.kc[i]] = credit[i];
            }
        }
        if (lane == 0) attr_store(P, d, tok, bad);
    }
}

// K > 1024: theta and the credit of the document in LDS (dynamic: 16 K bytes), one wavefront per workgroup.  Lane j touches the
// entries j + 64 i of both rows and no other: nothing is shared between lanes, so there is no barrier.  A site's row is read twice
// (the second time from the caches).
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
            stream_sites(P, th, lane, b, e, [&](int64_t s, int32_t f, bool ok, double p, const double *row) {
                const bool good = ok && attr_good(p);
                tok += good ? f : 0;
                bad += good ? 0 : f;
                if (!good) {
                    if (SITES && last && lane == 0) attr_site_none(P, s);
                    return;
                }
                const double inv = 1.0 / p;
                const double g = (double)f * inv;
#pragma unroll 8
                for (int k = lane; k < K; k += 64) credit[k] = credit[k] + (th[k] * row[k]) * g;
                if (SITES && last)
                    attr_site_top<64>(P, s, lane == 0, [&](double pr, int pk, double &br, int &bk) {
                        for (int k = lane; k < K; k += 64) attr_offer((th[k] * row[k]) * inv, k, pr, pk, br, bk);
                    });
            });
            if (last) break;
            double part = 0.0;                          // the M-step; num takes the credit's place
            for (int k = lane; k < K; k += 64) {
                const double num = th[k] > 0.0 ? credit[k] + P.alpha : 0.0;
                credit[k] = num;
                part = part + num;
            }
            const double den = doc_tree<64>(part);
            if (den > 0.0 && den < inf)
                for (int k = lane; k < K; k += 64) th[k] = credit[k] / den;
        }
        for (int k = lane; k < K; k += 64) {
            if (P.theta_out) P.theta_out[d * P.ld_out + k] = th[k];
            if (P.credit) P.credit[d * P.ld_credit + k] = credit[k];
        }
        if (lane == 0) attr_store(P, d, tok, bad);
    }
}

// K <= G <= 32: 64 / G documents per wavefront
template <int G, bool SITES>
__global__ void __launch_bounds__(64 * ATTR_WAVES) llda_attr_group_kernel(const AttrParams P, const int64_t n_tiles)
{
    group_docs<G, ATTR_WAVES>(P, n_tiles, [&](const GroupDoc &g) {
        double th[1] = {g.th}, credit[1] = {0.0};
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters;
            tok = 0; bad = 0;
            credit[0] = 0.0;
            group_sites<G>(P, g, th[0], [&](int64_t s, int32_t f, bool ok, bool live, double p, double tk) {
                const bool good = ok && attr_good(p);
                tok += good ? f : 0;                    // (a site past the document's end: f = 0)
                bad += good ? 0 : f;
                const double inv = good ? 1.0 / p : 0.0;
                if (good && g.mine) credit[0] = credit[0] + tk * ((double)f * inv);
                if (SITES && last)                      // (a site that is not good offers nothing: all -1 / 0.0)
                    attr_site_top<G>(P, s, live && g.gl == 0, [&](double pr, int pk, double &br, int &bk) {
                        if (good && g.mine) attr_offer(tk * inv, g.gl, pr, pk, br, bk);
                    });
            });
            if (last) break;
            attr_mstep<1, G>(th, credit, g.mine ? 1u : 0u, P.alpha, g.n > 0);      // (a document without sites takes no step)
        }
        if (g.active && g.mine) {
            if (P.theta_out) P.theta_out[g.d * P.ld_out + g.gl] = th[0];
            if (P.credit) P.credit[g.d * P.ld_credit + g.gl] = credit[0];
        }
        if (g.active && g.gl == 0) attr_store(P, g.d, tok, bad);
    });
}

}  // namespace
