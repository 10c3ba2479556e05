// kernel_heldout.hpp -- llda_heldout_wave_kernel, llda_heldout_wide_kernel, llda_heldout_group_kernel: the likelihood of held-out sites
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_heldout_loglik (include/llda_gibbs.h): for every document the product over its sites of p^f, p = theta[d] . phi_t[w], as a
// pair (mantissa in [0.5, 1), 64-bit exponent): the scored half of document completion.  The host takes the
// logarithm; nothing here but IEEE multiplications and additions, each rounded on its own (contraction is off in this unit), and
// frexp, which is exact.
//
// The sum p, the pair product and the three walks over a document's sites (wave, streaming, group) are doc_model.hpp's.  p^f by
// right-to-left binary exponentiation on pairs, the document's product site by site in ascending order: the same in every lane,
// so lane 0 (of the group) stores.  A document's outputs depend on its own inputs only; a site whose word is outside [0, V) counts
// as bad.
// ---------------------------------------------------------------------------------------------
struct HeldoutParams : DocModel {
    double *mant;
    int64_t *expo;
    int64_t *tok;
    int64_t *bad;
};

constexpr int HELDOUT_WAVES = 4;                        // wavefronts of a workgroup
constexpr int heldout_u(int NI) { return NI <= 8 ? 4 : 2; }     // sites in flight in the wave kernel: NI = 1, 2, 4, 8 | 16

struct HeldoutDoc {
    double m;
    int64_t e, tok, bad;
};

// one site: the document's product *= p^f
__device__ __forceinline__ void heldout_site(HeldoutDoc &doc, double p, int32_t f)
{
    const bool good = p > 0.0 && p < __longlong_as_double(0x7FF0000000000000ll);
    doc.tok += good ? f : 0;                            // (two selects: a choice between the two counters would put them in scratch)
    doc.bad += good ? 0 : f;
    if (!good) return;
    double bm = __builtin_amdgcn_frexp_mant(p), am = 0.5;                            // frexp: exact, denormals included
    int64_t be = __builtin_amdgcn_frexp_exp(p), ae = 1;
    for (uint32_t r = (uint32_t)f; r != 0;) {
        if (r & 1u) pair_mul(am, ae, bm, be);
        r >>= 1;
        if (r != 0) pair_mul(bm, be, bm, be);           // (squarings past the highest set bit reach nothing)
    }
    pair_mul(doc.m, doc.e, am, ae);
}

__device__ __forceinline__ void heldout_store(const HeldoutParams &P, int64_t d, const HeldoutDoc &doc)
{
    if (P.mant) P.mant[d] = doc.m;
    if (P.expo) P.expo[d] = doc.e;
    if (P.tok) P.tok[d] = doc.tok;
    if (P.bad) P.bad[d] = doc.bad;
}

template <int NI, int U>
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_wave_kernel(const HeldoutParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const WaveCols<NI> C(lane, P.K);
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int64_t d = (int64_t)blockIdx.x * HELDOUT_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * HELDOUT_WAVES) {
        const double *trow = P.theta + d * P.ld_theta;
        double th[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = trow[C.kc[i]];
        HeldoutDoc doc = {0.5, 1, 0, 0};
        wave_sites<NI, U>(P, C, th, lane, P.doc_off[d], P.doc_off[d + 1],
                          [&](int64_t, int32_t f, bool ok, double p, const double (&)[NI]) { heldout_site(doc, ok ? p : nan, f); });
        if (lane == 0) heldout_store(P, d, doc);
    }
}

// K > 1024: theta is read again with every site: the row is the document's own and stays in the caches
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_wide_kernel(const HeldoutParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int64_t d = (int64_t)blockIdx.x * HELDOUT_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * HELDOUT_WAVES) {
        HeldoutDoc doc = {0.5, 1, 0, 0};
        stream_sites(P, P.theta + d * P.ld_theta, lane, P.doc_off[d], P.doc_off[d + 1],
                     [&](int64_t, int32_t f, bool ok, double p, const double *) { heldout_site(doc, ok ? p : nan, f); });
        if (lane == 0) heldout_store(P, d, doc);
    }
}

// K <= G <= 32: 64 / G documents per wavefront
template <int G>
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_group_kernel(const HeldoutParams P, const int64_t n_tiles)
{
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    group_docs<G, HELDOUT_WAVES>(P, n_tiles, [&](const GroupDoc &g) {
        HeldoutDoc doc = {0.5, 1, 0, 0};
        group_sites<G>(P, g, g.th, [&](int64_t, int32_t f, bool ok, bool live, double p, double) {
            if (live) heldout_site(doc, ok ? p : nan, f);
        });
        if (g.active && g.gl == 0) heldout_store(P, g.d, doc);
    });
}

}  // namespace
