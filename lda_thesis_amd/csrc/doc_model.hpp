// doc_model.hpp -- the document model p(w | d) = theta[d] . phi_t[w]: its sum, the pair product and the three site walks
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// What llda_heldout_loglik, llda_attribute and llda_left_to_right (include/llda_gibbs.h) have in common, each piece once.
//
// The sum (fixed by the header, restated in tests/heldoutref.py).  64 partial sums, partial j over the topics j, j + 64, ... in
// increasing order from +0.0; then part[j] += part[j ^ s] for s = 1, 2, 4, 8, 16, 32, every j at once: IEEE addition commutes, so
// after the step s the lanes of a block of 2 s hold one value, and after the last all 64 hold p.  Nothing here but IEEE
// multiplications and additions, each rounded on its own (contraction is off in this unit).
//
// The walks.  A walk visits the sites of a document in ascending order and hands each to a callable with p and the products
// t_k = theta_k phi_t[w][k] it was added up from; what a site means is the kernel's business (kernel_heldout.hpp, kernel_attr.hpp).
// A word id outside [0, V) is never used as an index: row 0 is read in its place and the site arrives with ok = false.
// Wave (32 < K <= 1024): one wavefront per document, lane j on the topics j + 64 i -- a row of phi_t arrives as coalesced 512-byte
// runs.  The document's theta row stays in NI = 1, 2, 4, 8 or 16 registers per lane and U sites are in flight at a time (all their
// loads are issued before the first sum); a lane whose topic is >= K loads column 0 instead and drops the value, so the loop has
// no branch and no column >= K is read.  The wavefront reads the document's words and frequencies 64 sites at a time and hands
// them round with v_readlane.
// Streaming (K > 1024): the same walk, one site at a time, theta read again with every site through a pointer.
// Group (K <= G <= 32): a group of G = 8, 16 or 32 >= K lanes per document, 64 / G documents per wavefront.  The partials of the
// lanes >= K are +0.0 and the steps s >= G of the tree add +0.0 to a sum that is never -0.0 (it starts from +0.0): the same bits
// as 64 lanes.  The groups of a wavefront walk to the longest of their documents and the callable runs in every lane for every
// site up to there (live = false past the document's own end, where f = 0): every lane takes part in every exchange.
// ---------------------------------------------------------------------------------------------
struct DocModel {
    const int64_t *doc_off;
    const int32_t *word;
    const int32_t *freq;
    const double *theta;
    const double *phi_t;
    int64_t D, V, ld_theta, ld_phi;
    int32_t K;
};

// One step of the tree, part[j] + part[j ^ s], without LDS.  After the steps below s the lanes of a block of s hold one value, so
// ANY lane of the partner block gives part[j ^ s]: the quad permutations are the steps 1 and 2 themselves, the mirror of eight
// lanes pairs the two blocks of four (step 4), the mirror of a row the two blocks of eight (step 8); v_permlane16_swap / 32_swap
// of a value with itself leave the lower block's value in one result and the upper block's in the other, in both blocks.
template <int S>
__device__ __forceinline__ double doc_step(double part)
{
    if constexpr (S == 1) return part + dpp_f64<DPP_XOR1>(part);
    else if constexpr (S == 2) return part + dpp_f64<DPP_XOR2>(part);
    else if constexpr (S == 4) return part + dpp_f64<DPP_HALF_MIRROR>(part);
    else if constexpr (S == 8) return part + dpp_f64<0x140>(part);                 // row_mirror
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
__device__ __forceinline__ double doc_tree(double part)
{
    part = doc_step<1>(part);
    part = doc_step<2>(part);
    part = doc_step<4>(part);
    if constexpr (G > 8) part = doc_step<8>(part);
    if constexpr (G > 16) part = doc_step<16>(part);
    if constexpr (G > 32) part = doc_step<32>(part);
    return part;
}

__device__ __forceinline__ bool word_ok(int32_t w, int64_t V) { return (uint64_t)(int64_t)w < (uint64_t)V; }

// (m, e) = (m, e) * (bm, be): mantissas in [0.5, 1), so the product is in [0.25, 1) and doubling it is exact
template <typename E>
__device__ __forceinline__ void pair_mul(double &m, E &e, double bm, E be)
{
    const double c = m * bm;
    const bool half = c < 0.5;
    m = half ? c + c : c;
    e += be - (half ? 1 : 0);
}

// (m, e) *= p, 0 < p < inf.  frexp: exact, denormals included
template <typename E>
__device__ __forceinline__ void pair_mul_frexp(double &m, E &e, double p)
{
    pair_mul(m, e, __builtin_amdgcn_frexp_mant(p), (E)__builtin_amdgcn_frexp_exp(p));
}

// ---- wave: 32 < K <= 1024 ----
template <int NI>
struct WaveCols {
    int kc[NI];                                         // the lane's columns; column 0 where it has none
    uint32_t in;                                        // bit i: the lane has the topic lane + 64 i
    __device__ __forceinline__ WaveCols(int lane, int K) : in(0)
    {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int k = lane + 64 * i;
            kc[i] = k < K ? k : 0;
            if (k < K) in |= 1u << i;
        }
    }
};

// the sites [b, e) of one document: site(site index, f, ok, p, t[NI]) with t[i] = th[i] * phi_t[w][kc[i]]
template <int NI, int U, typename F>
__device__ __forceinline__ void wave_sites(const DocModel &M, const WaveCols<NI> &C, const double (&th)[NI], int lane, int64_t b,
                                           int64_t e, F &&site)
{
    for (int64_t s0 = b; s0 < e; s0 += 64) {
        const int n = (int)(e - s0 < 64 ? e - s0 : 64);
        const int32_t wv = lane < n ? M.word[s0 + lane] : -1;
        const int32_t fv = lane < n ? (M.freq ? M.freq[s0 + lane] : 1) : 0;
        for (int t = 0; t < n; t += U) {
            int32_t f[U];
            bool ok[U];
            double v[U][NI];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int tt = t + u < n ? t + u : n - 1;                            // (a repeat of the last site, not used)
                const int32_t w = __builtin_amdgcn_readlane(wv, tt);
                f[u] = __builtin_amdgcn_readlane(fv, tt);
                ok[u] = word_ok(w, M.V);
                const double *row = M.phi_t + (int64_t)(ok[u] ? w : 0) * M.ld_phi;
#pragma unroll
                for (int i = 0; i < NI; ++i) v[u][i] = row[C.kc[i]];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (t + u >= n) break;
                double part = 0.0;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    v[u][i] = th[i] * v[u][i];                                       // t_k
                    part = (C.in >> i & 1u) ? part + v[u][i] : part;
                }
                site(s0 + t + u, f[u], ok[u], doc_tree<64>(part), v[u]);
            }
        }
    }
}

// ---- streaming: K > 1024 ----
// the sites [b, e) of one document against the K loads at th (global memory or LDS): site(site index, f, ok, p, row of phi_t)
template <typename F>
__device__ __forceinline__ void stream_sites(const DocModel &M, const double *th, int lane, int64_t b, int64_t e, F &&site)
{
    const int K = M.K;
    for (int64_t s0 = b; s0 < e; s0 += 64) {
        const int n = (int)(e - s0 < 64 ? e - s0 : 64);
        const int32_t wv = lane < n ? M.word[s0 + lane] : -1;
        const int32_t fv = lane < n ? (M.freq ? M.freq[s0 + lane] : 1) : 0;
        for (int t = 0; t < n; ++t) {
            const int32_t w = __builtin_amdgcn_readlane(wv, t), f = __builtin_amdgcn_readlane(fv, t);
            const bool ok = word_ok(w, M.V);
            const double *row = M.phi_t + (int64_t)(ok ? w : 0) * M.ld_phi;
            double part = 0.0;
#pragma unroll 8
            for (int k = lane; k < K; k += 64) part = part + th[k] * row[k];
            site(s0 + t, f, ok, doc_tree<64>(part), row);
        }
    }
}

// ---- group: K <= G <= 32 ----
struct GroupDoc {
    int64_t d, b, n, n_max;                             // the document, its first site, its sites, those of the wavefront's longest
    int gl;                                             // the lane of the group: its topic
    bool active, mine;                                  // d < D; gl < K
    double th;                                          // theta[d][gl], 0.0 where there is none
};

// the tiles of WAVES * 64 / G documents of a workgroup, one after the other: doc(GroupDoc) in every lane
template <int G, int WAVES, typename F>
__device__ __forceinline__ void group_docs(const DocModel &M, int64_t n_tiles, F &&doc)
{
    constexpr int DPB = 64 * WAVES / G;                 // documents of a workgroup
    GroupDoc g;
    g.gl = threadIdx.x % G;
    g.mine = g.gl < M.K;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        g.d = tile * DPB + threadIdx.x / G;
        g.active = g.d < M.D;
        g.b = g.active ? M.doc_off[g.d] : 0;
        g.n = g.active ? M.doc_off[g.d + 1] - g.b : 0;
        g.n_max = g.n;                                  // the longest document of the wavefront
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            const int64_t o = __shfl_xor(g.n_max, s, 64);
            g.n_max = o > g.n_max ? o : g.n_max;
        }
        g.th = (g.active && g.mine) ? M.theta[g.d * M.ld_theta + g.gl] : 0.0;
        doc(g);
    }
}

// the sites 0 .. n_max of the group's document against the load th: site(site index, f, ok, live, p, t_k) in every lane.
// col: the column of phi_t that the lane reads where g.mine -- its own number, or the label it holds (kernel_docsparse.hpp)
template <int G, typename F>
__device__ __forceinline__ void group_sites_at(const DocModel &M, const GroupDoc &g, int col, double th, F &&site)
{
    constexpr int U = 4;
    for (int64_t t = 0; t < g.n_max; t += U) {
        int32_t f[U];
        bool ok[U];
        double v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool live = t + u < g.n;
            const int32_t w = live ? M.word[g.b + t + u] : -1;
            f[u] = live ? (M.freq ? M.freq[g.b + t + u] : 1) : 0;
            ok[u] = word_ok(w, M.V);
            v[u] = (ok[u] && g.mine) ? M.phi_t[(int64_t)w * M.ld_phi + col] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const double tk = th * v[u];
            double part = 0.0;
            if (ok[u] && g.mine) part = part + tk;
            site(g.b + t + u, f[u], ok[u], t + u < g.n, doc_tree<G>(part), tk);
        }
    }
}

template <int G, typename F>
__device__ __forceinline__ void group_sites(const DocModel &M, const GroupDoc &g, double th, F &&site)
{
    group_sites_at<G>(M, g, g.gl, th, site);
}

}  // namespace
