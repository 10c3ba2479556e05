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
// Arithmetic (fixed by the header, restated in tests/heldoutref.py).  64 partial sums, partial j over the topics j, j + 64, ... in
// increasing order from +0.0; then part[j] += part[j ^ s] for s = 1, 2, 4, 8, 16, 32, every j at once: IEEE addition commutes, so
// after the step s the lanes of a block of 2 s hold one value, and after the last all 64 hold p.  p^f by right-to-left binary
// exponentiation on pairs, the document's product site by site in ascending order: the same in every lane, so lane 0 stores.
//
// Geometry.  K > 32: one wavefront per document, lane j on the topics j + 64 i -- a row of phi_t arrives as coalesced 512-byte
// runs.  Up to K = 1024 the document's theta row stays in NI = 1, 2, 4, 8 or 16 registers per lane and U sites are in flight at a
// time (all their loads are issued before the first sum); a lane whose topic is >= K loads column 0 instead and drops the value, so
// the loop has no branch and no column >= K is read.  Beyond (llda_heldout_wide_kernel) theta is re-read with every site: the row
// is the document's own and stays in the caches.  The wavefront reads the document's words and frequencies 64 sites at a time and
// hands them round with v_readlane.
// K <= 32: a group of G = 8, 16 or 32 >= K lanes per document, 64 / G documents per wavefront.  The partials of the lanes >= K are
// +0.0 and the steps s >= G of the tree add +0.0 to a sum that is never -0.0 (it starts from +0.0): the same bits as 64 lanes.
// The groups of a wavefront walk to the longest of their documents so that every lane takes part in every exchange.
// A document's outputs depend on its own inputs only.  A word id outside [0, V) is never used as an index: its site counts as bad.
// ---------------------------------------------------------------------------------------------
struct HeldoutParams {
    const int64_t *doc_off;
    const int32_t *word;
    const int32_t *freq;
    const double *theta;
    const double *phi_t;
    int64_t D, V, ld_theta, ld_phi;
    int32_t K;
    double *mant;
    int64_t *expo;
    int64_t *tok;
    int64_t *bad;
};

constexpr int HELDOUT_WAVES = 4;                        // wavefronts of a workgroup

// (m, e) = (m, e) * (bm, be): mantissas in [0.5, 1), so the product is in [0.25, 1) and doubling it is exact
__device__ __forceinline__ void heldout_mul(double &m, int64_t &e, double bm, int64_t be)
{
    double c = m * bm;
    int64_t x = e + be;
    if (c < 0.5) { c = c + c; x -= 1; }
    m = c; e = x;
}

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
        if (r & 1u) heldout_mul(am, ae, bm, be);
        r >>= 1;
        if (r != 0) heldout_mul(bm, be, bm, be);        // (squarings past the highest set bit reach nothing)
    }
    heldout_mul(doc.m, doc.e, am, ae);
}

__device__ __forceinline__ void heldout_store(const HeldoutParams &P, int64_t d, const HeldoutDoc &doc)
{
    if (P.mant) P.mant[d] = doc.m;
    if (P.expo) P.expo[d] = doc.e;
    if (P.tok) P.tok[d] = doc.tok;
    if (P.bad) P.bad[d] = doc.bad;
}

// One step of the tree, part[j] + part[j ^ s], without LDS.  After the steps below s the lanes of a block of s hold one value, so
// ANY lane of the partner block gives part[j ^ s]: the quad permutations are the steps 1 and 2 themselves, the mirror of eight
// lanes pairs the two blocks of four (step 4), the mirror of a row the two blocks of eight (step 8); v_permlane16_swap / 32_swap
// of a value with itself leave the lower block's value in one result and the upper block's in the other, in both blocks.
template <int CTRL>
__device__ __forceinline__ double heldout_dpp(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

template <int S>
__device__ __forceinline__ double heldout_step(double part)
{
    if constexpr (S == 1) return part + heldout_dpp<0xB1>(part);                   // quad_perm [1, 0, 3, 2]
    else if constexpr (S == 2) return part + heldout_dpp<0x4E>(part);              // quad_perm [2, 3, 0, 1]
    else if constexpr (S == 4) return part + heldout_dpp<0x141>(part);             // row_half_mirror
    else if constexpr (S == 8) return part + heldout_dpp<0x140>(part);             // row_mirror
    else {
        const uint32_t lo = (uint32_t)__double2loint(part), hi = (uint32_t)__double2hiint(part);
        if constexpr (S == 16) {
            const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
            return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
        } else {
            const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
            return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
        }
    }
}

// the steps s = 1 .. G / 2 of the tree: G = 64 is all of it
template <int G>
__device__ __forceinline__ double heldout_tree(double part)
{
    part = heldout_step<1>(part);
    part = heldout_step<2>(part);
    part = heldout_step<4>(part);
    if constexpr (G > 8) part = heldout_step<8>(part);
    if constexpr (G > 16) part = heldout_step<16>(part);
    if constexpr (G > 32) part = heldout_step<32>(part);
    return part;
}

__device__ __forceinline__ bool heldout_word_ok(int32_t w, int64_t V) { return (uint64_t)(int64_t)w < (uint64_t)V; }

template <int NI, int U>
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_wave_kernel(const HeldoutParams P)
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
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int64_t d = (int64_t)blockIdx.x * HELDOUT_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * HELDOUT_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        const double *trow = P.theta + d * P.ld_theta;
        double th[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) th[i] = trow[kc[i]];
        HeldoutDoc doc = {0.5, 1, 0, 0};
        for (int64_t s0 = b; s0 < e; s0 += 64) {
            const int n = (int)(e - s0 < 64 ? e - s0 : 64);
            const int32_t wv = lane < n ? P.word[s0 + lane] : -1;
            const int32_t fv = lane < n ? (P.freq ? P.freq[s0 + lane] : 1) : 0;
            for (int t = 0; t < n; t += U) {
                int32_t w[U], f[U];
                bool ok[U];
                double v[U][NI];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int tt = t + u < n ? t + u : n - 1;                        // (a repeat of the last site, not used)
                    w[u] = __builtin_amdgcn_readlane(wv, tt);
                    f[u] = __builtin_amdgcn_readlane(fv, tt);
                    ok[u] = heldout_word_ok(w[u], P.V);
                    const double *row = P.phi_t + (int64_t)(ok[u] ? w[u] : 0) * P.ld_phi;
#pragma unroll
                    for (int i = 0; i < NI; ++i) v[u][i] = row[kc[i]];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (t + u >= n) break;
                    double part = 0.0;
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const double sum = part + th[i] * v[u][i];
                        part = (in >> i & 1u) ? sum : part;
                    }
                    const double p = heldout_tree<64>(part);
                    heldout_site(doc, ok[u] ? p : nan, f[u]);
                }
            }
        }
        if (lane == 0) heldout_store(P, d, doc);
    }
}

// K > 1024: theta is read again with every site
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_wide_kernel(const HeldoutParams P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = P.K;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    for (int64_t d = (int64_t)blockIdx.x * HELDOUT_WAVES + wave; d < P.D; d += (int64_t)gridDim.x * HELDOUT_WAVES) {
        const int64_t b = P.doc_off[d], e = P.doc_off[d + 1];
        const double *trow = P.theta + d * P.ld_theta;
        HeldoutDoc doc = {0.5, 1, 0, 0};
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
                for (int k = lane; k < K; k += 64) part = part + trow[k] * row[k];
                const double p = heldout_tree<64>(part);
                heldout_site(doc, ok ? p : nan, f);
            }
        }
        if (lane == 0) heldout_store(P, d, doc);
    }
}

// K <= G <= 32: 64 / G documents per wavefront
template <int G>
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_group_kernel(const HeldoutParams P, const int64_t n_tiles)
{
    constexpr int DPB = 64 * HELDOUT_WAVES / G;         // documents of a workgroup
    constexpr int U = 4;
    const int gl = threadIdx.x % G, dl = threadIdx.x / G;
    const bool mine = gl < P.K;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
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
        const double th = (active && mine) ? P.theta[d * P.ld_theta + gl] : 0.0;
        HeldoutDoc doc = {0.5, 1, 0, 0};
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
                double part = 0.0;
                if (ok[u] && mine) part = part + th * v[u];
                part = heldout_tree<G>(part);
                if (t + u < n) heldout_site(doc, ok[u] ? part : nan, f[u]);
            }
        }
        if (active && gl == 0) heldout_store(P, d, doc);
    }
}

}  // namespace
