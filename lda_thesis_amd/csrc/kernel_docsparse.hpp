// kernel_docsparse.hpp -- llda_attr_sparse_kernel, llda_heldout_sparse_kernel, llda_wcredit_sparse_kernel: the document model on sparse label sets
// Part of the single translation unit llda_gibbs.hip (included in order; see the contents list there).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// llda_attribute_sparse and llda_credit_words_sparse (include/llda_gibbs.h): llda_attribute and llda_credit_words
// for documents that carry a handful of the K labels.  A document's labels are a CSR next to its sites -- lab_off [D+1], lab [NL]
// strictly ascending -- and its loads, its new loads and its credit live per SLOT of that list.  A site gathers L_d doubles of its
// word's row of phi_t where the dense kernels stream K.
//
// Arithmetic (fixed by the header, restated in tests/sparseref.py): kernel_attr.hpp's, on the one-document problem with K' = L_d
// columns, column j = label lab[j].  A group of G = 8, 16 or 32 >= max_labels lanes holds a document's list, lane gl the slot gl:
// p is doc_tree<G> over the lanes' products (the lanes >= L_d hold +0.0), which is sum64 of the L_d <= 32 products in slot order.
// The list is ascending, so "ties by topic id" and "ties by slot" are one order.
//
// Unfit documents: L_d > max_labels, offsets outside [0, NL], a label id outside [0, K), a list that does not strictly ascend (a
// lane compares its id with its left neighbour's: a duplicate would make two lanes of one site add to one sum).  No lane of an
// unfit document uses a label id as an index.
//
// Document side (llda_attr_sparse_kernel): llda_attr_group_kernel with a column per lane and a K per group -- the same walk
// (group_sites_at), E-step, M-step and top-m rounds.  Word side (llda_wcredit_sparse_kernel): one wavefront per chunk of a word's
// sites, found through llda_credit_words' index pass; the chunk's K sums live in LDS (8 K bytes per wavefront), 64 / G sites are
// worked at a time, one group each, and the groups commit their products to LDS one group after the other in ascending site order:
// two sites that share a label (every document has the root) add in site order, and no site is added twice.
// ---------------------------------------------------------------------------------------------
struct LabelSets {
    const int64_t *lab_off;
    const int32_t *lab;
    const double *theta_s;
    int64_t NL;
    int32_t max_labels;
};

struct AttrSparseParams : AttrParams {                  // theta / ld_theta / ld_out / ld_credit are not used: the slots take their place
    LabelSets sets;
};

struct WCreditSparseParams : WCreditParams {            // DocModel::phi_t / ld_phi are not used (V = D still bounds the document ids)
    LabelSets sets;
};

// the label list of document d in a group of G lanes
struct LabelSlot {
    int64_t lb, L;                                      // the first slot, the slots (as the offsets say)
    int k;                                              // the lane's label; 0 where it has none
    bool inside, fit, mine;                             // the offsets lie in [0, NL]; the document is fit; gl < L of a fit document
    double th;                                          // theta_s of the slot, 0.0 where there is none
};

// every lane of the group calls it (there is a ballot inside); have: d is a document; LOADS: theta_s is given (else th = 0.0)
template <int G, bool LOADS = true>
__device__ __forceinline__ LabelSlot label_slot(const LabelSets &T, int64_t d, bool have, int gl, int K)
{
    LabelSlot s;
    s.lb = have ? T.lab_off[d] : 0;
    s.L = have ? T.lab_off[d + 1] - s.lb : 0;
    s.inside = s.lb >= 0 && s.L >= 0 && s.L <= T.NL && s.lb <= T.NL - s.L;
    const bool range = s.inside && s.L <= T.max_labels;
    const bool slot = range && gl < s.L;
    const int k = slot ? T.lab[s.lb + gl] : -1;
    const int left = __shfl_up(k, 1, 64);               // (gl = 0 does not look at it)
    const bool wrong = slot && ((uint32_t)k >= (uint32_t)K || (gl > 0 && k <= left));
    const uint64_t group = (G == 64 ? ~0ull : (1ull << G) - 1) << (__lane_id() & ~(G - 1));
    s.fit = range && !(__ballot(wrong) & group);
    s.mine = s.fit && slot;
    s.k = s.mine ? k : 0;
    if constexpr (LOADS) s.th = s.mine ? T.theta_s[s.lb + gl] : 0.0;
    else s.th = 0.0;
    return s;
}

// G lanes per document, 64 / G documents per wavefront: the tiles of group_docs, the loads from the slots
template <int G, bool SITES>
__global__ void __launch_bounds__(64 * ATTR_WAVES) llda_attr_sparse_kernel(const AttrSparseParams P, const int64_t n_tiles)
{
    constexpr int DPB = 64 * ATTR_WAVES / G;            // documents of a workgroup
    GroupDoc g;
    g.gl = threadIdx.x % G;
    g.th = 0.0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        g.d = tile * DPB + threadIdx.x / G;
        g.active = g.d < P.D;
        g.b = g.active ? P.doc_off[g.d] : 0;
        g.n = g.active ? P.doc_off[g.d + 1] - g.b : 0;
        g.n_max = g.n;                                  // the longest document of the wavefront
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            const int64_t o = __shfl_xor(g.n_max, s, 64);
            g.n_max = o > g.n_max ? o : g.n_max;
        }
        const LabelSlot ls = label_slot<G>(P.sets, g.d, g.active, g.gl, P.K);
        g.mine = ls.mine;
        double th[1] = {ls.th}, credit[1] = {0.0};
        int64_t tok = 0, bad = 0;
        for (int pass = 0;; ++pass) {
            const bool last = pass == P.iters;
            tok = 0; bad = 0;
            credit[0] = 0.0;
            group_sites_at<G>(P, g, ls.k, th[0], [&](int64_t s, int32_t f, bool ok, bool live, double p, double tk) {
                const bool good = ls.fit && ok && attr_good(p);
                tok += good ? f : 0;                    // (a site past the document's end: f = 0)
                bad += good ? 0 : f;
                const double inv = good ? 1.0 / p : 0.0;
                if (good && g.mine) credit[0] = credit[0] + tk * ((double)f * inv);
                if (SITES && last)                      // (a site that is not good offers nothing: all -1 / 0.0)
                    attr_site_top<G>(P, s, live && g.gl == 0, [&](double pr, int pk, double &br, int &bk) {
                        if (good && g.mine) attr_offer(tk * inv, ls.k, pr, pk, br, bk);
                    });
            });
            if (last) break;
            attr_mstep<1, G>(th, credit, g.mine ? 1u : 0u, P.alpha, g.n > 0);      // (a document without sites takes no step)
        }
        if (g.mine) {
            if (P.theta_out) P.theta_out[ls.lb + g.gl] = th[0];
            if (P.credit) P.credit[ls.lb + g.gl] = credit[0];
        }
        if (g.active && !ls.fit && ls.inside)           // unfit: its slots keep their loads and get no credit
            for (int64_t j = ls.lb + g.gl; j < ls.lb + ls.L; j += G) {
                if (P.theta_out) P.theta_out[j] = P.sets.theta_s[j];
                if (P.credit) P.credit[j] = 0.0;
            }
        if (g.active && g.gl == 0) attr_store(P, g.d, tok, bad);
    }
}

// llda_heldout_loglik_sparse: llda_heldout_group_kernel with a label per lane and a label list per group.  p is
// doc_tree<G> over the slots' products, the lanes >= L_d holding +0.0: sum64 of the compacted problem; heldout_site is unchanged.
// An unfit document's sites arrive as NaN (all bad); L_d = 0 gives p = +0.0 at every site (all bad as well).
struct HeldoutSparseParams : HeldoutParams {            // theta / ld_theta are not used: the slots take their place
    LabelSets sets;
};

template <int G>
__global__ void __launch_bounds__(64 * HELDOUT_WAVES) llda_heldout_sparse_kernel(const HeldoutSparseParams P, const int64_t n_tiles)
{
    constexpr int DPB = 64 * HELDOUT_WAVES / G;         // documents of a workgroup
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    GroupDoc g;
    g.gl = threadIdx.x % G;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        g.d = tile * DPB + threadIdx.x / G;
        g.active = g.d < P.D;
        g.b = g.active ? P.doc_off[g.d] : 0;
        g.n = g.active ? P.doc_off[g.d + 1] - g.b : 0;
        g.n_max = g.n;                                  // the longest document of the wavefront
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            const int64_t o = __shfl_xor(g.n_max, s, 64);
            g.n_max = o > g.n_max ? o : g.n_max;
        }
        const LabelSlot ls = label_slot<G>(P.sets, g.d, g.active, g.gl, P.K);
        g.mine = ls.mine;
        g.th = ls.th;
        HeldoutDoc doc = {0.5, 1, 0, 0};
        group_sites_at<G>(P, g, ls.k, ls.th, [&](int64_t, int32_t f, bool ok, bool live, double p, double) {
            if (live) heldout_site(doc, (ls.fit && ok) ? p : nan, f);
        });
        if (g.active && g.gl == 0) heldout_store(P, g.d, doc);
    }
}

// one wavefront per chunk; blockDim.x / 64 wavefronts per workgroup, each with its own K sums in LDS (dynamic: 8 K bytes each)
template <int G>
__global__ void __launch_bounds__(64 * WCREDIT_WAVES) llda_wcredit_sparse_kernel(const WCreditSparseParams P)
{
    extern __shared__ double wsparse_lds[];
    constexpr int NG = 64 / G;                          // sites worked at a time
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const int gl = lane % G, grp = lane / G;
    const int K = P.K;
    double *acc = wsparse_lds + (int64_t)wave * K;
    const int64_t total = wcredit_total(P);
    for (int64_t c = (int64_t)blockIdx.x * waves + wave; c < total; c += (int64_t)gridDim.x * waves) {
        const WChunk w = wcredit_chunk(P, c);
        const double *prow = P.wphi + w.v * P.ld_wphi;
        for (int k = lane; k < K; k += 64) acc[k] = 0.0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (other lanes add to what this one cleared)
        __builtin_amdgcn_wave_barrier();
        int64_t tok = 0, bad = 0;                       // of the group's own sites
        for (int64_t s0 = w.b; s0 < w.e; s0 += 64) {
            const int n = (int)(w.e - s0 < 64 ? w.e - s0 : 64);
            const int32_t dv = lane < n ? P.word[s0 + lane] : -1;
            const int32_t fv = lane < n ? (P.freq ? P.freq[s0 + lane] : 1) : 0;
            for (int t = 0; t < n; t += NG) {
                const bool live = t + grp < n;
                const int32_t d = __shfl(dv, (t + grp) & 63, 64), ft = __shfl(fv, (t + grp) & 63, 64);      // (every lane: a lane that sits
                const int32_t f = live ? ft : 0;                                                            // out returns 0 to its readers)
                const bool ok = live && word_ok(d, P.V);
                const LabelSlot ls = label_slot<G>(P.sets, d, ok, gl, K);
                const double tk = ls.th * (ls.mine ? prow[ls.k] : 0.0);
                double part = 0.0;
                if (ls.mine) part = part + tk;
                const double p = doc_tree<G>(part);
                const bool good = ok && ls.fit && attr_good(p);
                tok += good ? f : 0;
                bad += good ? 0 : f;
                const double inv = good ? 1.0 / p : 0.0;
                const double add = tk * ((double)f * inv);
#pragma unroll
                for (int i = 0; i < NG; ++i) {          // site t + i: its labels are distinct, the sites before it are in
                    if (grp == i && good && ls.mine) acc[ls.k] = acc[ls.k] + add;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
#pragma unroll
        for (int s = G; s < 64; s <<= 1) {
            tok += __shfl_xor(tok, s, 64);
            bad += __shfl_xor(bad, s, 64);
        }
        const WDest dst(P, w);
        if (dst.row)
            for (int k = lane; k < K; k += 64) dst.row[k] = w.single ? 0.0 + acc[k] : acc[k];
        if (lane == 0 && dst.tok) *dst.tok = tok;
        if (lane == 0 && dst.bad) *dst.bad = bad;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // (the next chunk clears the sums the lanes above read)
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace
