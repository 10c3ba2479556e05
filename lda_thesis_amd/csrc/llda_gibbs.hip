// llda_gibbs.hip -- collapsed-Gibbs sweep for Labeled LDA / CascadeLDA on MI355X (gfx950, wave64).
//
// Hot path replaced: LabeledLDA.training_iteration (/root/reference/LabeledLDA.py:101-125) ==
// SubLDA.training_iteration (/root/reference/CascadeLDA.py:397-421).  C ABI: include/llda_gibbs.h.
//
// Execution model (DESIGN.md sections 3-4):
//   * group layout: one lane GROUP of G = 8..64 lanes per document (64/G documents per wavefront), T topic
//     slots per lane; topic k lives at (lane, slot) chosen so that numpy's pairwise summation order (np.sum at
//     LabeledLDA.py:117) is lane-local: one accumulator chain = one lane walking its slots, the 8 accumulators
//     of a 128-topic leaf = 8 neighbouring lanes;
//   * the n_kw row of the current word is one contiguous KP*4-byte read (word-major layout), prefetched one
//     site ahead.  A changed site stores ONE word (old position | new position << 16) at its word-major place in the
//     commit log, which llda_commit_log folds into n_kw word by word without global atomics (callers without a
//     log: two int32 atomics into n_kw_delta per changed site); n_k_delta is updated through an LDS accumulator per
//     workgroup.  Snapshot semantics + integer sums => bit-deterministic;
//   * the draw is TIERED: an fp32 decision with a proven margin, an fp64 decision, and the
//     reference's fp64 pipeline bit for bit (IEEE division, numpy-ordered sum, keyed Philox4x32-10 draw) for
//     the sites the cheaper tiers cannot decide -- the chosen topic is always the exact pipeline's.
// No MFMA (gather/scan, not a contraction).  FMA contraction is OFF: the reference rounds after every ufunc.
//
// Contents (one translation unit; the headers are included in this order)
//   build_info.hpp      llda_build_info() from the preprocessor alone (host only)
//   sweep_plan.hpp      sweep_plan            what llda_sweep launches -- family, template choices, margins, grid, LDS -- as a
//                                             pure function of its arguments and the layout (host only; the debug_margin table)
//   device_common.hpp   kernel parameters, Philox, row loads, one-hot updates, exact division, DPP / permlane
//                       cross-lane moves, numpy-ordered group sum, keyed categorical draw (exact)
//   draw_tiers.hpp      tier-0 (fp32) decision, cold tiers (fp64 decision, exact pipeline), commit of a site
//   exact_generic.hpp   exact_site_wave           the exact pipeline with the layout known at run time (a whole wave per
//                                                 document): the sparse kernels' answer to a site they cannot decide
//   kernel_sweep.hpp    llda_sweep_exact_kernel   general kernel, every site through the exact pipeline
//                       llda_sweep_kernel         tiered kernel, per-document state in LDS (the hot kernel)
//   quad_doc_map.hpp    quad_tier1_doc's lane-to-position mapping: one document on 64 lanes (constexpr, compiled by a host test too)
//   kernel_quad.hpp     llda_sweep_quad_kernel    K = 512 dense, 16-bit image: FOUR documents per wavefront (the bench's timed kernel)
//   kernel_sparse.hpp   llda_sweep_sparse_kernel  one lane per ALLOWED topic for sparse label sets
//   kernel_batch.hpp    llda_sweep_batch_kernel   one sweep over many independent small problems (CascadeLDA's
//                                                 ensemble) in one launch, sparse-kernel arithmetic
//   kernel_readout.hpp  llda_loglik_kernel, llda_readout_phi / _theta kernels (thinning read-outs)
//   kernel_foldin.hpp   llda_foldin_kernel (test-time sampler)
//   kernel_counts.hpp   llda_commit_log_kernel, llda_apply_delta_kernel, llda_count_init_kernel, self test
//   kernel_hist.hpp     llda_count_hist_kernel    counts of counts of n_dk / n_kw (the estimate of alpha and beta)
//   kernel_rank.hpp     llda_rank_labels_kernel   top-n labels and the harness metrics' ingredients from one sort per document
//   kernel_wide.hpp     the general path for K with more than 8 pairwise leaves (one wavefront per document)
//   top_list.hpp        TopList<N, Ord>   the N best entries under a strict total order, sorted in registers: insertion, the fold of
//                                         sorted partial lists, the pop across a wavefront (the four selections below; a host test too)
//   kernel_topwords.hpp llda_top_words_kernel, llda_top_words_merge_kernel   the n best words of every topic, by count
//   kernel_scored.hpp   llda_scored_words_kernel, llda_scored_merge_kernel   the n best words of every topic by a float64 score: 96-bit (score, word) keys
//   kernel_cooc.hpp     llda_word_cooc_kernel, llda_word_cooc_agg_kernel   document and co-document frequencies of the listed words (topic coherence)
//   kernel_window.hpp   llda_window_cooc_kernel   in how many sliding windows of the running text the listed words meet (C_V, C_UCI, C_NPMI)
//   doc_model.hpp       p(w | d) = theta[d] . phi_t[w] once: the 64-partial xor-tree sum, word_ok, the (mantissa, exponent) product and
//                       the three walks over a document's sites -- wave_sites, stream_sites, group_docs / group_sites
//   kernel_heldout.hpp  llda_heldout_wave_kernel, _wide_kernel, _group_kernel   per-document likelihood of held-out sites as (mantissa, exponent)
//   kernel_attr.hpp     llda_attr_wave_kernel, _lds_kernel, _group_kernel           per-word label shares, credit and the EM fold-in
//   kernel_leftright.hpp llda_leftright_kernel   left-to-right estimate of a document's likelihood: one particle per wavefront
//   kernel_nearest.hpp  llda_nearest_kernel, llda_nearest_merge_kernel   the n best rows of b per row of a: tiled fp64 product, selection in its epilogue
//   kernel_label.hpp    llda_label_keys / _sort / _merge / _walk kernels   the documents of every label ranked: chunk sort in LDS, merge levels, one walk
//                       llda_label_sets_kernel   per-label thresholds applied to every document: masks by ballot, tp / fp / fn
//   kernel_ecdf.hpp     llda_ecdf_totals / _keys / _walk kernels   every word's ECDF rank within every topic, on kernel_label.hpp's sort
//                       llda_frex_select_kernel, llda_frex_merge_kernel   the n best words of every topic by two ranks (FREX): exact 96-bit compares
//   kernel_emfit.hpp    llda_wcredit_index / _wave / _lds / _group / _combine kernels   the E-step's shares added up per word, in chunks of a word's sites
//                       llda_phistep_block / _den / _div kernels   the phi M-step: column sums in a fixed order, one division per entry
//   kernel_docsparse.hpp llda_attr_sparse_kernel, llda_wcredit_sparse_kernel   both on sparse label sets: a lane per label of the document, the word's sums in LDS
//                       llda_heldout_sparse_kernel   the likelihood of held-out sites against the loads per slot
//   kernel_lrsparse.hpp llda_leftright_sparse_kernel   left-to-right on a document's own labels: one particle per lane group, one count per lane
//   kernel_foldinsparse.hpp llda_foldin_sparse_kernel   the test-time sampler on a document's own labels: 8 lanes per document, its list in registers
//   this file           host side: layout (llda_layout_init), dispatch, C entry points
#include <hip/hip_runtime.h>
#include "build_info.hpp"
#include "sweep_plan.hpp"
#include <stdint.h>
#include <math.h>
#include <string.h>
#include <map>
#include <memory>
#include <type_traits>

#include "llda_gibbs.h"

#pragma clang fp contract(off)

#include "device_common.hpp"
#include "draw_tiers.hpp"
#include "exact_generic.hpp"
#include "kernel_sweep.hpp"
#include "quad_doc_map.hpp"
#include "kernel_quad.hpp"
#include "kernel_sparse.hpp"
#include "kernel_batch.hpp"
#include "kernel_readout.hpp"
#include "kernel_foldin.hpp"
#include "kernel_counts.hpp"
#include "kernel_hist.hpp"
#include "kernel_rank.hpp"
#include "kernel_wide.hpp"
#include "top_list.hpp"
#include "kernel_topwords.hpp"
#include "kernel_scored.hpp"
#include "kernel_cooc.hpp"
#include "kernel_window.hpp"
#include "doc_model.hpp"
#include "kernel_heldout.hpp"
#include "kernel_attr.hpp"
#include "kernel_leftright.hpp"
#include "kernel_nearest.hpp"
#include "kernel_label.hpp"
#include "kernel_ecdf.hpp"
#include "kernel_emfit.hpp"
#include "kernel_docsparse.hpp"
#include "kernel_lrsparse.hpp"
#include "kernel_foldinsparse.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static_assert(SWEEP_MAX_LIVE == LLDA_MAX_LIVE && SWEEP_QUAD_THREADS == QNT, "sweep_plan.hpp restates two kernel constants");

void add_leaves(llda_layout *L, int n, int start)
{
    if (n <= 128) {
        if (L->n_leaves < LLDA_MAX_WIDE_LEAVES) {
            L->leaf_start[L->n_leaves] = start;
            L->leaf_len[L->n_leaves] = n;
        }
        L->n_leaves++;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    add_leaves(L, n2, start);
    add_leaves(L, n - n2, start + n2);
}

// numpy's recursion over leaf ranges [first, first+count): returns depth, fills the schedule
int schedule(llda_layout *L, int n, int *next_leaf, int *first_out, int *count_out)
{
    if (n <= 128) {
        *first_out = (*next_leaf)++;
        *count_out = 1;
        return 0;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    int lf, lc, rf, rc;
    const int dl = schedule(L, n2, next_leaf, &lf, &lc);
    const int dr = schedule(L, n - n2, next_leaf, &rf, &rc);
    const int d = (dl > dr ? dl : dr);      // this node combines in round d
    if (d < LLDA_MAX_ROUNDS) {
        for (int a = lf; a < lf + lc; ++a) L->rounds[d][a] = rf;
        for (int b = rf; b < rf + rc; ++b) L->rounds[d][b] = lf;
    }
    if (d + 1 > L->n_rounds) L->n_rounds = d + 1;
    *first_out = lf;
    *count_out = lc + rc;
    return d + 1;
}

// numpy's recursion as in-place adds over the leaf totals, post-order: returns the first leaf of the subtree
int comb_tree(llda_layout *L, int n, int *next_leaf, int *n_comb)
{
    if (n <= 128) return (*next_leaf)++;
    int n2 = n / 2;
    n2 -= n2 % 8;
    const int a = comb_tree(L, n2, next_leaf, n_comb);
    const int b = comb_tree(L, n - n2, next_leaf, n_comb);
    if (*n_comb < LLDA_MAX_WIDE_LEAVES) { L->comb_dst[*n_comb] = a; L->comb_src[*n_comb] = b; }
    ++*n_comb;
    return a;
}

int hip_fail(hipError_t e)
{
    g_last_hip_error = (int)e;
    return LLDA_E_HIP;
}

// the return code of an entry point after its last launch
int launched()
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? LLDA_OK : hip_fail(e);
}

// run-time value -> template argument: f(std::integral_constant<int, V>) for the V that v equals, LLDA_E_BAD_K when none does
template <int... Vs, typename F>
int visit_int(int v, F &&f)
{
    int rc = LLDA_E_BAD_K;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}

// f with the smallest of Ns (ascending) that is >= n, LLDA_E_BAD_K when none is
template <int... Ns, typename F>
int visit_at_least(int n, F &&f)
{
    int b = -1;
    (void)((n <= Ns && ((b = Ns), true)) || ...);
    return visit_int<Ns...>(b, f);
}

template <typename F>
int visit_bool(bool b, F &&f)
{
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// the narrow layouts llda_layout_init makes: 8 lanes with 1, 2, 4, 8, 12 or 16 slots, 16 / 32 / 64 lanes with 12 or 16
template <typename F>
int visit_layout(int G, int T, F &&f)
{
    return visit_int<8, 16, 32, 64>(G, [&](auto g) {
        if constexpr (g.value == 8) return visit_int<1, 2, 4, 8, 12, 16>(T, [&](auto t) { return f(g, t); });
        else return visit_int<12, 16>(T, [&](auto t) { return f(g, t); });
    });
}

// the leaf table of the pairwise sum, into the parameters of a kernel that maps positions to topics
template <typename Params>
void copy_leaves(const llda_layout &L, Params &P)
{
    for (int p = 0; p < LLDA_MAX_WIDE_LEAVES; ++p) { P.leaf_start[p] = L.leaf_start[p]; P.leaf_len[p] = L.leaf_len[p]; }
}

// The layout of K (128 KB of tables): built once per host thread and K, not once per call.
const llda_layout *layout_of(int32_t K, int *rc)
{
    static thread_local std::map<int32_t, std::unique_ptr<llda_layout>> cache;
    auto it = cache.find(K);
    if (it != cache.end()) { *rc = LLDA_OK; return it->second.get(); }
    std::unique_ptr<llda_layout> L(new llda_layout);
    *rc = llda_layout_init(K, L.get());
    if (*rc) return nullptr;
    if (cache.size() >= 256) cache.clear();
    return (cache[K] = std::move(L)).get();
}

// kernels of the wide path take their LDS as a run-time size; above 64 KB a kernel has to be told once
template <typename Kern>
int allow_lds(Kern kern, size_t bytes)
{
    if (bytes > 160 * 1024) return LLDA_E_BAD_K;
    if (bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return hip_fail(e);
    }
    return LLDA_OK;
}

void fill_wide(const llda_layout &L, WideLayout &W)
{
    W.NT = L.tiers; W.T = L.T; W.G = L.G; W.KP = L.KP;
    W.m = L.n_leaves; W.last_leaf = L.n_leaves - 1; W.tail = L.tail; W.tail_row = L.tail_row;
    for (int i = 0; i < LLDA_MAX_WIDE_LEAVES; ++i) {
        W.comb_dst[i] = (uint8_t)L.comb_dst[i];
        W.comb_src[i] = (uint8_t)L.comb_src[i];
    }
}

// a kernel of llda_sweep on the grid, the block and the dynamic LDS of the plan
template <typename Kern, typename... Args>
int launch(Kern kern, const SweepPlan &p, hipStream_t st, const Args &...args)
{
    const int rl = allow_lds(kern, p.lds);
    if (rl) return rl;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(p.block), p.lds, st, args...);
    return launched();
}

// SWEEP_EXACT, SWEEP_TIERED, SWEEP_ROWS16
template <int G, int T>
int launch_sweep(const KParams &P, const SweepPlan &p, hipStream_t st)
{
    if constexpr (G <= 16) {
        if (p.rec) {                                    // 16-byte site records (llda_sweep_args.site_rec)
            if (p.dense) return launch(llda_sweep_kernel<G, T, false, true, true, true>, p, st, P);
            if (p.has_tail) return launch(llda_sweep_kernel<G, T, true, false, true, true>, p, st, P);
            return launch(llda_sweep_kernel<G, T, false, false, true, true>, p, st, P);
        }
    }
    if constexpr (G >= 32 && T == 16) {
        if (p.family == SWEEP_ROWS16) {
            if (p.w4) return launch(llda_sweep_kernel<G, T, false, true, true, false, true, true>, p, st, P);
            return launch(llda_sweep_kernel<G, T, false, true, true, false, true>, p, st, P);
        }
    }
    if (p.family == SWEEP_EXACT) {
        if (p.has_tail) return launch(llda_sweep_exact_kernel<G, T, true>, p, st, P);
        return launch(llda_sweep_exact_kernel<G, T, false>, p, st, P);
    }
    if (p.dense) {
        if (p.logged) return launch(llda_sweep_kernel<G, T, false, true, true>, p, st, P);
        return launch(llda_sweep_kernel<G, T, false, true, false>, p, st, P);
    }
    if (p.has_tail) {
        if (p.logged) return launch(llda_sweep_kernel<G, T, true, false, true>, p, st, P);
        return launch(llda_sweep_kernel<G, T, true, false, false>, p, st, P);
    }
    if (p.logged) return launch(llda_sweep_kernel<G, T, false, false, true>, p, st, P);
    return launch(llda_sweep_kernel<G, T, false, false, false>, p, st, P);
}

// SWEEP_SPARSE (Params = KParams) and SWEEP_WIDE_SPARSE (WSParams)
template <typename Params>
int launch_sparse(const llda_sweep_args *a, const SweepPlan &p, Params &P, hipStream_t st)
{
    P.live_off = a->live_off; P.live_pos = a->live_pos;
    if (p.img) { P.img = a->n_kw_img; P.img_col = a->img_col; }
    return visit_int<8, 16, 32, 64>(p.gs, [&](auto gs) {
        return visit_int<0, 8, 16>(p.img, [&](auto img) {
            return launch(llda_sweep_sparse_kernel<gs.value, Params, img.value>, p, st, P);
        });
    });
}

// SWEEP_WIDE_F32, SWEEP_WIDE_REG, SWEEP_WIDE_LDS
int launch_wide(const llda_sweep_args *a, const SweepPlan &p, const WParams &W, hipStream_t st)
{
    if (p.family == SWEEP_WIDE_F32) {
        double *scr = p.slim ? static_cast<double *>(a->scratch) : nullptr;
        return visit_int<2, 3, 4, 5, 6, 7, 8>(p.nt, [&](auto nt) {
            return visit_int<3, 4>(p.tc, [&](auto tc) {
                return visit_bool(p.slim, [&](auto slim) {
                    if constexpr (wide_f32_pair(nt.value, tc.value))
                        return launch(llda_sweep_wide_f32_kernel<nt.value, tc.value, slim.value>, p, st, W, p.m0, scr);
                    else return (int)LLDA_E_BAD_K;
                });
            });
        });
    }
    if (p.family == SWEEP_WIDE_REG)
        return visit_int<2, 3, 4, 5, 6, 7, 8>(p.nt, [&](auto nt) {
            return visit_bool(p.compact, [&](auto compact) {
                return launch(llda_sweep_wide_reg_kernel<nt.value, compact.value>, p, st, W);
            });
        });
    return visit_bool(p.tiered, [&](auto tiered) { return launch(llda_sweep_wide_kernel<tiered.value>, p, st, W); });
}

// SWEEP_QUAD
int launch_quad(const SweepPlan &p, const KParams &P, hipStream_t st)
{
    return visit_int<2, 3, 4>(p.lb, [&](auto lb) {
        return visit_bool(p.pad, [&](auto pad) {
            return visit_bool(p.hooks, [&](auto hooks) {
                return launch(llda_sweep_quad_kernel<lb.value, (lb.value < 4), pad.value, hooks.value>, p, st, P);
            });
        });
    });
}

template <int G, int T>
int launch_loglik(const LParams &P, hipStream_t st)
{
    const int64_t blocks = (P.D + (256 / G) - 1) / (256 / G);
    hipLaunchKernelGGL((llda_loglik_kernel<G, T>), dim3((unsigned)blocks), dim3(256), 0, st, P);
    return launched();
}

template <int G, int T>
int launch_foldin(const FParams &P, bool has_tail, hipStream_t st)
{
    if (P.n_sites > 0) {                              // initial assignments: one lane group per site
        const int64_t ib = (P.n_sites + (256 / G) - 1) / (256 / G);
        if (ib > 0x7fffffffLL) return LLDA_E_BAD_ARG;
        if (has_tail) hipLaunchKernelGGL((llda_foldin_init_kernel<G, T, true>), dim3((unsigned)ib), dim3(256), 0, st, P);
        else hipLaunchKernelGGL((llda_foldin_init_kernel<G, T, false>), dim3((unsigned)ib), dim3(256), 0, st, P);
    }
    const int64_t blocks = (P.D + (256 / G) - 1) / (256 / G);
    if (has_tail) hipLaunchKernelGGL((llda_foldin_kernel<G, T, true>), dim3((unsigned)blocks), dim3(256), 0, st, P);
    else hipLaunchKernelGGL((llda_foldin_kernel<G, T, false>), dim3((unsigned)blocks), dim3(256), 0, st, P);
    return launched();
}

template <int G, int T>
int launch_theta(const RParams &P, bool has_tail, hipStream_t st)
{
    const int64_t blocks = (P.D + (256 / G) - 1) / (256 / G);
    if (has_tail) hipLaunchKernelGGL((llda_readout_theta_kernel<G, T, true>), dim3((unsigned)blocks), dim3(256), 0, st, P);
    else hipLaunchKernelGGL((llda_readout_theta_kernel<G, T, false>), dim3((unsigned)blocks), dim3(256), 0, st, P);
    return launched();
}

// the summation schedule shared by llda_sweep and llda_foldin
void fill_schedule(const llda_layout &L, int32_t &last_leaf, int32_t &tail, int32_t &tail_row, int32_t &n_rounds,
                   int32_t &xor_tree, uint32_t (&rounds_pk)[LLDA_MAX_ROUNDS])
{
    last_leaf = L.n_leaves - 1; tail = L.tail; tail_row = L.tail_row; n_rounds = L.n_rounds;
    const int P2 = L.G / 8;
    int xt = (L.n_leaves == P2) ? 1 : 0;
    for (int r = 0; (1 << r) < P2 && xt; ++r)
        for (int p = 0; p < P2; ++p)
            if (L.rounds[r][p] != (p ^ (1 << r))) xt = 0;
    xor_tree = xt;
    for (int r = 0; r < LLDA_MAX_ROUNDS; ++r) {
        uint32_t pk = 0;
        for (int p = 0; p < LLDA_MAX_LEAVES; ++p) pk |= (uint32_t)L.rounds[r][p] << (4 * p);
        rounds_pk[r] = pk;
    }
}

// The document-model entry points (doc_model.hpp).  The geometry by K: a group of G lanes per document up to 32 topics, a wavefront
// per document with NI registers per lane up to 1024, streaming beyond (NI = 0).  llda_left_to_right takes NI alone.
struct DocGeom { int G, NI; };
constexpr DocGeom doc_geom(int K)
{
    return {K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 0, K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : K <= 1024 ? 16 : 0};
}
constexpr bool doc_geom_is(int K, int G, int NI) { return doc_geom(K).G == G && doc_geom(K).NI == NI; }
static_assert(doc_geom_is(8, 8, 1) && doc_geom_is(9, 16, 1) && doc_geom_is(16, 16, 1) && doc_geom_is(17, 32, 1) && doc_geom_is(32, 32, 1), "group seams");
static_assert(doc_geom_is(33, 0, 1) && doc_geom_is(64, 0, 1) && doc_geom_is(65, 0, 2) && doc_geom_is(128, 0, 2) && doc_geom_is(129, 0, 4) &&
              doc_geom_is(256, 0, 4) && doc_geom_is(257, 0, 8) && doc_geom_is(512, 0, 8) && doc_geom_is(513, 0, 16) && doc_geom_is(1024, 0, 16) &&
              doc_geom_is(1025, 0, 0), "wave seams");

// what llda_heldout_loglik and llda_attribute check alike, in their order, and the fields they copy alike.  LLDA_OK with D = 0:
// the caller has nothing to do; extra(): the checks of its own that come before that
template <typename Args, typename Extra>
int doc_model_args(const Args *a, DocModel &M, Extra &&extra)
{
    if (!a) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->ld_theta < a->K || a->ld_phi < a->K) return LLDA_E_BAD_ARG;
    if (!extra()) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->theta || !a->phi_t) return LLDA_E_BAD_ARG;
    if (a->D > INT64_MAX / a->ld_theta || a->V > INT64_MAX / a->ld_phi) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->theta, a->phi_t, a->tok, a->bad) || misaligned(3, a->word, a->freq)) return LLDA_E_BAD_ARG;
    M.doc_off = a->doc_off; M.word = a->word; M.freq = a->freq; M.theta = a->theta; M.phi_t = a->phi_t;
    M.D = a->D; M.V = a->V; M.ld_theta = a->ld_theta; M.ld_phi = a->ld_phi; M.K = a->K;
    return LLDA_OK;
}

inline dim3 doc_grid(int64_t blocks, int64_t cap = 1 << 20) { return dim3((unsigned)(blocks < cap ? blocks : cap)); }

// the one ladder: group(G, grid, n_tiles), wave(NI, grid) or stream(grid) launches the family's kernel of that form
template <int WAVES, typename FG, typename FW, typename FS>
int launch_doc_model(const DocModel &M, FG &&group, FW &&wave, FS &&stream)
{
    const DocGeom g = doc_geom(M.K);
    if (g.G) return visit_int<8, 16, 32>(g.G, [&](auto G) {
        constexpr int docs = 64 * WAVES / G.value;
        const int64_t n_tiles = (M.D + docs - 1) / docs;
        group(G, doc_grid(n_tiles), n_tiles);
        return launched();
    });
    const dim3 grid = doc_grid((M.D + WAVES - 1) / WAVES);
    if (g.NI) return visit_int<1, 2, 4, 8, 16>(g.NI, [&](auto NI) {
        wave(NI, grid);
        return launched();
    });
    return stream(grid);
}

// llda_attribute: the kernel form by K (kernel_attr.hpp); SITES: the per-site outputs are wanted
template <bool SITES>
int launch_attr(const AttrParams &P, hipStream_t st)
{
    const dim3 block(64 * ATTR_WAVES);
    return launch_doc_model<ATTR_WAVES>(P,
        [&](auto G, dim3 grid, int64_t n_tiles) { hipLaunchKernelGGL((llda_attr_group_kernel<G.value, SITES>), grid, block, 0, st, P, n_tiles); },
        [&](auto NI, dim3 grid) { hipLaunchKernelGGL((llda_attr_wave_kernel<NI.value, attr_u(NI.value), SITES>), grid, block, 0, st, P); },
        [&](dim3) {
            const size_t lds = (size_t)2 * P.K * sizeof(double);                 // theta and credit: at most 123 008 bytes
            const int rl = allow_lds(llda_attr_lds_kernel<SITES>, lds);
            if (rl) return rl;
            hipLaunchKernelGGL(llda_attr_lds_kernel<SITES>, doc_grid(P.D, ATTR_LDS_MAX_BLOCKS), dim3(64), lds, st, P);
            return launched();
        });
}

// llda_credit_words: the chunk kernel by K (kernel_emfit.hpp), on at most `chunks` chunks
int launch_wcredit(const WCreditParams &P, int64_t chunks, hipStream_t st)
{
    const dim3 block(64 * WCREDIT_WAVES);
    const DocGeom g = doc_geom(P.K);
    if (g.G) return visit_int<8, 16, 32>(g.G, [&](auto G) {
        constexpr int per = 64 * WCREDIT_WAVES / G.value;
        hipLaunchKernelGGL(llda_wcredit_group_kernel<G.value>, doc_grid((chunks + per - 1) / per), block, 0, st, P);
        return launched();
    });
    if (g.NI) return visit_int<1, 2, 4, 8, 16>(g.NI, [&](auto NI) {
        hipLaunchKernelGGL((llda_wcredit_wave_kernel<NI.value, attr_u(NI.value)>), doc_grid((chunks + WCREDIT_WAVES - 1) / WCREDIT_WAVES), block, 0, st, P);
        return launched();
    });
    const size_t lds = (size_t)P.K * sizeof(double);                             // the chunk's sums: at most 61 504 bytes
    const int rl = allow_lds(llda_wcredit_lds_kernel, lds);
    if (rl) return rl;
    hipLaunchKernelGGL(llda_wcredit_lds_kernel, doc_grid(chunks, WCREDIT_LDS_MAX_BLOCKS), dim3(64), lds, st, P);
    return launched();
}

// the lane group of a sparse-label call: the smallest of 8, 16, 32 that holds max_labels
constexpr int sparse_group(int max_labels) { return max_labels <= 8 ? 8 : max_labels <= 16 ? 16 : 32; }
static_assert(sparse_group(1) == 8 && sparse_group(8) == 8 && sparse_group(9) == 16 && sparse_group(16) == 16 && sparse_group(17) == 32 &&
              sparse_group(LLDA_SPARSE_MAX_LABELS) == 32, "sparse group seams");

// wavefronts of a workgroup of llda_wcredit_sparse_kernel: as many of WCREDIT_WAVES as 32 KB of LDS hold, 8 K bytes each (K <= 1024: 4,
// K <= 2048: 2, beyond: 1).  What is left of the CU's 160 KB goes to further workgroups.
constexpr int wsparse_waves(int K) { return K <= 1024 ? WCREDIT_WAVES : K <= 2048 ? 2 : 1; }
static_assert((size_t)wsparse_waves(LLDA_MAX_K) * LLDA_MAX_K * sizeof(double) <= 160 * 1024 && wsparse_waves(1024) * 1024 * 8 <= 32 * 1024 &&
              wsparse_waves(2048) * 2048 * 8 <= 32 * 1024, "the sums of a workgroup fit the LDS of a CU");

// llda_attribute_sparse: the lane group by max_labels (kernel_docsparse.hpp)
template <bool SITES>
int launch_attr_sparse(const AttrSparseParams &P, hipStream_t st)
{
    return visit_int<8, 16, 32>(sparse_group(P.sets.max_labels), [&](auto G) {
        constexpr int docs = 64 * ATTR_WAVES / G.value;
        const int64_t n_tiles = (P.D + docs - 1) / docs;
        hipLaunchKernelGGL((llda_attr_sparse_kernel<G.value, SITES>), doc_grid(n_tiles), dim3(64 * ATTR_WAVES), 0, st, P, n_tiles);
        return launched();
    });
}

// llda_credit_words_sparse: the chunk kernel on at most `chunks` chunks
int launch_wcredit_sparse(const WCreditSparseParams &P, int64_t chunks, hipStream_t st)
{
    const int waves = wsparse_waves(P.K);
    const size_t lds = (size_t)waves * P.K * sizeof(double);
    return visit_int<8, 16, 32>(sparse_group(P.sets.max_labels), [&](auto G) {
        const int rl = allow_lds(llda_wcredit_sparse_kernel<G.value>, lds);
        if (rl) return rl;
        hipLaunchKernelGGL(llda_wcredit_sparse_kernel<G.value>, doc_grid((chunks + waves - 1) / waves), dim3(64 * waves), lds, st, P);
        return launched();
    });
}

// partial rows of llda_credit_words at most: a word with more than one chunk has more than `chunk` sites, so its chunks are fewer
// than twice its share of S / chunk
inline int64_t wcredit_rows(int64_t S, int32_t chunk) { return 2 * (S / chunk); }

// chunks of llda_credit_words at most: a word's last chunk may be short, and there are never more chunks than sites
inline int64_t wcredit_chunks_cap(int64_t V, int64_t S, int32_t chunk) { const int64_t most = S / chunk + V; return most < S ? most : S; }

}  // namespace

extern "C" {

int llda_abi_version(void) { return LLDA_ABI_VERSION; }

int llda_build_info(void) { return LLDA_BUILD_INFO_BITS; }

int llda_last_hip_error(void) { return g_last_hip_error; }

int llda_struct_size(int which)
{
    switch (which) {
    case 0: return (int)sizeof(llda_layout);
    case 1: return (int)sizeof(llda_sweep_args);
    case 2: return (int)sizeof(llda_batch_args);
    case 3: return (int)sizeof(llda_foldin_args);
    case 4: return (int)sizeof(llda_rank_args);
    case 5: return (int)sizeof(llda_heldout_args);
    case 6: return (int)sizeof(llda_attr_args);
    default: return -1;
    }
}

const char *llda_strerror(int code)
{
    switch (code) {
    case LLDA_OK: return "ok";
    case LLDA_E_BAD_K: return "K outside 1..7688, or a wide layout (more than 8 pairwise leaves) handed to an entry point that only takes narrow ones";
    case LLDA_E_BAD_ARG: return "bad argument";
    case LLDA_E_HIP: return "HIP runtime error";
    case LLDA_E_NO_DEVICE: return "no HIP device";
    default: return "unknown error";
    }
}

int llda_layout_init(int32_t K, llda_layout *L)
{
    if (!L) return LLDA_E_BAD_ARG;
    if (K < 1 || K > LLDA_MAX_K) return LLDA_E_BAD_K;
    memset(L, 0, sizeof *L);
    L->K = K;
    add_leaves(L, K, 0);
    if (L->n_leaves > LLDA_MAX_WIDE_LEAVES) return LLDA_E_BAD_K;
    L->wide = L->n_leaves > LLDA_MAX_LEAVES ? 1 : 0;
    int P = 1;
    if (L->wide) P = (L->n_leaves + 7) / 8 * 8;          // 64-lane tiers of one wavefront
    else
        while (P < L->n_leaves) P *= 2;
    L->G = 8 * P;
    L->tiers = L->wide ? P / 8 : 0;
    int t = 0;
    for (int p = 0; p < L->n_leaves; ++p) {
        const int r = (L->leaf_len[p] + 7) / 8;
        if (r > t) t = r;
    }
    if (t > 2) t = (t + 3) / 4 * 4;
    L->T = t;
    L->KP = L->G * t;
    L->tail = L->leaf_len[L->n_leaves - 1] % 8;
    L->tail_row = L->leaf_len[L->n_leaves - 1] / 8;
    for (int i = 0; i < LLDA_MAX_KP; ++i) L->pos_topic[i] = -1;
    // memory position of (lane g, slot s): the 16-byte chunk s >> 2 of all lanes is contiguous (rows with fewer than
    // 4 slots per lane: pos = g*T + s)
    const int w = (t % 4 == 0) ? 4 : t;
    for (int g = 0; g < L->G; ++g)
        for (int s = 0; s < t; ++s) {
            const int pos = ((s / w) * L->G + g) * w + (s % w);
            L->pos_lane[pos] = g;
            L->pos_slot[pos] = s;
        }
    for (int p = 0; p < L->n_leaves; ++p)
        for (int rel = 0; rel < L->leaf_len[p]; ++rel) {
            const int g = 8 * p + (rel & 7), s = rel >> 3;
            const int pos = ((s / w) * L->G + g) * w + (s % w);
            L->topic_pos[L->leaf_start[p] + rel] = pos;
            L->pos_topic[pos] = L->leaf_start[p] + rel;
        }
    {
        int next = 0, n_comb = 0;
        comb_tree(L, K, &next, &n_comb);
    }
    for (int r = 0; r < LLDA_MAX_ROUNDS; ++r)
        for (int p = 0; p < LLDA_MAX_LEAVES; ++p) L->rounds[r][p] = p;
    if (!L->wide) {
        int next = 0, first, count;
        schedule(L, K, &next, &first, &count);
        if (L->n_rounds > LLDA_MAX_ROUNDS) return LLDA_E_BAD_K;
    }
    return LLDA_OK;
}

int64_t llda_sweep_scratch_bytes(int32_t K, int64_t D)
{
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc || !Lp->wide) return 0;
    return (int64_t)wide_blocks(D) * Lp->KP * 8;          // one row of doubles per workgroup of the wide sweep
}

int llda_sweep(const llda_sweep_args *a, void *stream)
{
    if (!a || a->D < 0 || a->V < 1) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(a->K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    SweepPlan p;
    rc = sweep_plan(*a, L, true, &p);                   // (true: the quad kernels compile the margin hooks out of production)
    if (rc || p.family == SWEEP_NONE) return rc;

    KParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.doc_order = a->doc_order; P.word = a->word; P.freq = a->freq; P.z = a->z;
    P.lab_mask = a->lab_mask; P.n_dk = a->n_dk; P.n_kw = a->n_kw; P.n_kw_delta = a->n_kw_delta;
    P.n_k = a->n_k; P.n_k_delta = a->n_k_delta; P.status = a->status;
    P.csc_pos = a->csc_pos; P.commit_log = a->commit_log;
    P.site_rec = p.site_rec ? a->site_rec : nullptr;
    P.D = a->D; P.doc_base = a->doc_base;
    P.alpha = a->alpha; P.beta = a->beta;
    P.vbeta = (double)a->V * a->beta;                       // V * beta evaluated first (LabeledLDA.py:115)
    P.alpha32 = (float)a->alpha; P.beta32 = (float)a->beta; P.vbeta32 = (float)P.vbeta;
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32);
    P.sweep = a->sweep; P.stream_id = a->stream_id;
    fill_schedule(L, P.last_leaf, P.tail, P.tail_row, P.n_rounds, P.xor_tree, P.rounds_pk);
    P.KP = L.KP;
    P.margin_rel = p.margin_rel; P.margin0_rel = p.margin0_rel; P.margin0_data = p.margin0_data;
    P.dpg = p.dpg;
    hipStream_t st = (hipStream_t)stream;

    switch (p.family) {
    case SWEEP_SPARSE:
        return launch_sparse(a, p, P, st);
    case SWEEP_WIDE_SPARSE: {
        WSParams W;
        memset(&W, 0, sizeof W);
        static_cast<KParams &>(W) = P;
        fill_wide(L, W.w);
        return launch_sparse(a, p, W, st);
    }
    case SWEEP_WIDE_F32:
    case SWEEP_WIDE_REG:
    case SWEEP_WIDE_LDS: {
        WParams W;
        memset(&W, 0, sizeof W);
        W.k = P;
        fill_wide(L, W.w);
        return launch_wide(a, p, W, st);
    }
    case SWEEP_QUAD:
        P.n_kw16 = a->n_kw16;
        P.row16 = a->row16;
        P.quad_pad = p.pad;
        return launch_quad(p, P, st);
    case SWEEP_ROWS16:
        P.n_kw16 = a->n_kw16;
        P.site_row = a->site_row;
        P.w4 = p.w4;
        break;
    default:
        break;
    }
    return visit_layout(L.G, L.T, [&](auto g, auto t) { return launch_sweep<g.value, t.value>(P, p, st); });
}


int llda_sweep_batch(const llda_batch_args *a, void *stream)
{
    if (!a || a->n_inst < 0 || a->V < 1) return LLDA_E_BAD_ARG;
    if (a->n_inst == 0) return LLDA_OK;
    if (!a->inst_off || !a->order || !a->word || !a->freq || !a->z || !a->inst_prob || !a->inst_doc || !a->live_off ||
        !a->live_pos || !a->ndk_off || !a->n_dk || !a->kw_off || !a->nk_off || !a->kp || !a->prob_stream || !a->k || !a->counts ||
        !a->delta)
        return LLDA_E_BAD_ARG;
    if (a->lanes != 8 && a->lanes != 16 && a->lanes != 32 && a->lanes != 64) return LLDA_E_BAD_ARG;
    BParams P;
    memset(&P, 0, sizeof P);
    P.inst_off = a->inst_off; P.order = a->order; P.n_inst = a->n_inst; P.word = a->word; P.freq = a->freq; P.z = a->z;
    P.inst_prob = a->inst_prob; P.inst_doc = a->inst_doc; P.live_off = a->live_off; P.live_pos = a->live_pos;
    P.ndk_off = a->ndk_off; P.n_dk = a->n_dk; P.kw_off = a->kw_off; P.nk_off = a->nk_off; P.kp = a->kp;
    P.prob_stream = a->prob_stream; P.k = a->k;
    P.counts = a->counts; P.delta = a->delta; P.status = a->status;
    P.alpha = a->alpha; P.beta = a->beta; P.vbeta = (double)a->V * a->beta;
    // the sparse arithmetic needs strictly positive scores and an in-range reciprocal (as llda_sweep's tiered kernels)
    if (!(a->alpha >= 1e-6 && a->beta >= 1e-6 && P.vbeta < 1099511627776.0)) return LLDA_E_BAD_ARG;
    P.margin_rel = batch_margin_rel(a->debug_margin);
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32); P.sweep = a->sweep;
    const int gpb = 256 / a->lanes;
    const int64_t blocks = (a->n_inst + gpb - 1) / gpb;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (a->lanes) {
    case 8: hipLaunchKernelGGL(llda_sweep_batch_kernel<8>, grid, block, 0, st, P); break;
    case 16: hipLaunchKernelGGL(llda_sweep_batch_kernel<16>, grid, block, 0, st, P); break;
    case 32: hipLaunchKernelGGL(llda_sweep_batch_kernel<32>, grid, block, 0, st, P); break;
    default: hipLaunchKernelGGL(llda_sweep_batch_kernel<64>, grid, block, 0, st, P); break;
    }
    return launched();
}

int llda_commit_log(const int64_t *item_begin, const int32_t *item_len, const int32_t *item_word, int64_t n_items,
                    const uint32_t *commit_log, const int32_t *freq_csc, int32_t K, const int64_t *row_off,
                    int32_t *target, int32_t *n_k, int32_t *n_k_delta, void *stream)
{
    if (n_items < 0 || (n_k != nullptr) != (n_k_delta != nullptr)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (n_items > 0 && (!item_begin || !item_len || !item_word || !commit_log || !freq_csc || !target)) return LLDA_E_BAD_ARG;
    if (n_items == 0 && !n_k) return LLDA_OK;
    CParams P;
    P.item_begin = item_begin; P.item_len = item_len; P.item_word = item_word; P.n_items = n_items;
    P.log = commit_log; P.freq = freq_csc; P.row_off = row_off; P.target = target; P.n_k = n_k; P.n_k_delta = n_k_delta;
    P.KP = L.KP;
    int64_t blocks = (n_items + 3) / 4;
    if (blocks < 1) blocks = 1;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    const int rl = allow_lds(llda_commit_log_kernel, 4 * L.KP * sizeof(int));      // (above 64 KB from KP = 4 096 on)
    if (rl) return rl;
    hipLaunchKernelGGL(llda_commit_log_kernel, dim3((unsigned)blocks), dim3(256), 4 * L.KP * sizeof(int), (hipStream_t)stream, P);
    return launched();
}

int llda_apply_rows(const int64_t *row_off, int32_t *rows, int64_t n_rows, int32_t K, int32_t *counts, void *stream)
{
    if (n_rows < 0) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (n_rows == 0) return LLDA_OK;
    if (!row_off || !rows || !counts) return LLDA_E_BAD_ARG;
    if (misaligned(7, counts, row_off)) return LLDA_E_BAD_ARG;           // (a pair word is decoded into two counts with one 8-byte access)
    const int64_t blocks = (n_rows + 3) / 4;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    hipLaunchKernelGGL(llda_apply_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, row_off, rows,
                       n_rows, L.KP, counts);
    return launched();
}

int llda_rows16_ok(int32_t K)
{
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    return !rc && !Lp->wide && Lp->T == 16 && Lp->G >= 32 && Lp->K == Lp->KP ? 1 : 0;
}

int llda_quad_ok(int32_t K)
{
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    // (every lane group holds a leaf: the branch-free count update rewrites slot 0 of the lanes that own neither topic of a site
    // with the factor of ITS counts, which must then be a position with a topic -- K = 250, three leaves in a four-leaf layout, is out)
    return !rc && !Lp->wide && Lp->T == 16 && (Lp->G == 8 || Lp->G == 16 || Lp->G == 32) && Lp->n_leaves * 8 == Lp->G ? 1 : 0;
}

int llda_pack_rows16(const int32_t *n_kw, const uint8_t *row16, int64_t V, int32_t K, uint16_t *n_kw16, int32_t *status,
                     void *stream)
{
    if (V < 0) return LLDA_E_BAD_ARG;
    if (!llda_rows16_ok(K)) return LLDA_E_BAD_K;
    if (V == 0) return LLDA_OK;
    if (!n_kw || !row16 || !n_kw16) return LLDA_E_BAD_ARG;
    if (misaligned(15, n_kw16, n_kw)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout &L = *layout_of(K, &rc);
    const int64_t blocks = (V * 2 * L.G + 255) / 256;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    hipLaunchKernelGGL(llda_pack_rows16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_kw, row16, n_kw16,
                       V, L.G, status);
    return launched();
}

int llda_pack_image_cols(const int32_t *n_kw, int64_t V, int32_t K, int32_t bits, const int32_t *col_src, void *img, void *stream)
{
    if (V < 0 || (bits != 8 && bits != 16)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    if (V == 0) return LLDA_OK;
    if (!n_kw || !img || !col_src || (Lp->KP & 3)) return LLDA_E_BAD_ARG;
    if (misaligned(15, n_kw) || misaligned(bits == 8 ? 3 : 7, img)) return LLDA_E_BAD_ARG;
    if (misaligned(15, col_src)) return LLDA_E_BAD_ARG;
    int64_t blocks = V < 256 * 32 ? V : 256 * 32;
    const dim3 grid((unsigned)blocks), block(256);
    const size_t lds = (size_t)Lp->KP * sizeof(int);
    if (bits == 8) hipLaunchKernelGGL(llda_pack_image_cols_kernel<8>, grid, block, lds, (hipStream_t)stream, n_kw, col_src, img, V, Lp->KP);
    else hipLaunchKernelGGL(llda_pack_image_cols_kernel<16>, grid, block, lds, (hipStream_t)stream, n_kw, col_src, img, V, Lp->KP);
    return launched();
}

int llda_pack_rows16_all(const int32_t *n_kw, int64_t V, int32_t K, uint16_t *n_kw16, uint8_t *row16, void *stream)
{
    if (V < 0) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    if (!llda_quad_ok(K)) return LLDA_E_BAD_K;
    if (V == 0) return LLDA_OK;
    if (!n_kw || !row16 || !n_kw16) return LLDA_E_BAD_ARG;
    if (misaligned(15, n_kw16, n_kw)) return LLDA_E_BAD_ARG;
    const int64_t blocks = (V * 2 * Lp->G + 255) / 256;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (Lp->G == 32) hipLaunchKernelGGL(llda_pack_rows16_all_kernel<32>, grid, block, 0, st, n_kw, n_kw16, row16, V);
    else if (Lp->G == 16) hipLaunchKernelGGL(llda_pack_rows16_all_kernel<16>, grid, block, 0, st, n_kw, n_kw16, row16, V);
    else hipLaunchKernelGGL(llda_pack_rows16_all_kernel<8>, grid, block, 0, st, n_kw, n_kw16, row16, V);
    return launched();
}

int llda_pack_image(const int32_t *n_kw, int64_t n, int32_t bits, void *img, void *stream)
{
    if (n < 0 || (n & 3) || (bits != 8 && bits != 16)) return LLDA_E_BAD_ARG;
    if (n == 0) return LLDA_OK;
    if (!n_kw || !img) return LLDA_E_BAD_ARG;
    if (misaligned(15, n_kw) || misaligned(bits == 8 ? 3 : 7, img)) return LLDA_E_BAD_ARG;
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    const dim3 grid((unsigned)blocks), block(256);
    if (bits == 8)
        hipLaunchKernelGGL(llda_pack_image_kernel<8>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const int4 *>(n_kw), img, n4);
    else
        hipLaunchKernelGGL(llda_pack_image_kernel<16>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const int4 *>(n_kw), img, n4);
    return launched();
}

int llda_apply_delta(int32_t *counts, int32_t *delta, int64_t n, void *stream)
{
    if (!counts || !delta || n < 0) return LLDA_E_BAD_ARG;
    if (n == 0) return LLDA_OK;
    const bool aligned = !misaligned(15, counts, delta);
    const int64_t n4 = aligned ? n / 4 : 0;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(llda_apply_delta_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       counts, delta, n4, n);
    return launched();
}

int llda_count_init(const int64_t *doc_off, const int32_t *word, const int32_t *freq, const int32_t *z,
                    int64_t D, int32_t K, int32_t *n_dk, int32_t *n_kw, int32_t *n_k, void *stream)
{
    if (D < 0) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (D == 0) return LLDA_OK;
    if (!doc_off || !word || !freq || !z || !n_dk || !n_kw || !n_k) return LLDA_E_BAD_ARG;
    // rows too long for five LDS histograms per workgroup (wide layouts): one wavefront per workgroup, two histograms
    const int waves = (size_t)5 * L.KP * sizeof(int) <= 48 * 1024 ? 4 : 1;
    const size_t lds = (size_t)(1 + waves) * L.KP * sizeof(int);
    const int rl = allow_lds(llda_count_init_kernel, lds);
    if (rl) return rl;
    int64_t blocks = (D + waves - 1) / waves;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(llda_count_init_kernel, dim3((unsigned)blocks), dim3(64 * waves), lds,
                       (hipStream_t)stream, doc_off, word, freq, z, D, L.KP, n_dk, n_kw, n_k);
    return launched();
}

int llda_count_hist(const int32_t *counts, int64_t rows, int32_t K, const uint16_t *lab_mask, int32_t mask_per_row, int32_t n_bins,
                    unsigned long long *hist, int32_t *over_val, int64_t over_cap, unsigned long long *over_n, void *stream)
{
    if (rows < 0 || n_bins < 1 || over_cap < 0 || (mask_per_row != 0 && mask_per_row != 1)) return LLDA_E_BAD_ARG;
    if (rows > 0 && (!counts || !lab_mask || !hist || !over_val || !over_n)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (rows == 0) return LLDA_OK;
    if (misaligned(15, counts) || misaligned(1, lab_mask) || misaligned(7, hist, over_n) || misaligned(3, over_val)) return LLDA_E_BAD_ARG;
    if (rows > INT64_MAX / L.KP) return LLDA_E_BAD_ARG;
    HParams P;
    P.counts = reinterpret_cast<const int4 *>(counts);
    P.cpr = L.KP / 4;                                  // (KP = 8 * leaves * T: a multiple of 8)
    P.n4 = rows * P.cpr;
    P.mask = lab_mask;
    P.mask_stride = mask_per_row ? L.G : 0;
    P.G = L.G;
    P.g_magic = (uint32_t)(((1u << 24) + (uint32_t)L.G - 1u) / (uint32_t)L.G);
    P.n_bins = (uint32_t)n_bins;
    P.hist = hist; P.over_val = over_val; P.over_cap = over_cap; P.over_n = over_n;
    const int64_t tile = 256 * HIST_UNROLL;
    int64_t blocks = (P.n4 + tile - 1) / tile;
    if (blocks > 256 * 8) blocks = 256 * 8;
    P.step256_r = 256 / P.cpr;
    P.step256_c = 256 % P.cpr;
    const int64_t skip = (blocks - 1) * tile;
    P.tile_rows = skip / P.cpr;
    P.tile_c = (int32_t)(skip % P.cpr);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (L.T % 4 == 0) hipLaunchKernelGGL(llda_count_hist_kernel<4>, grid, block, 0, st, P);
    else if (L.T == 2) hipLaunchKernelGGL(llda_count_hist_kernel<2>, grid, block, 0, st, P);
    else hipLaunchKernelGGL(llda_count_hist_kernel<1>, grid, block, 0, st, P);
    return launched();
}

int llda_rank_labels(const llda_rank_args *a, void *stream)
{
    if (!a) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->first < 0 || a->first >= a->K || a->ld < a->K || a->top_n < 0 || a->top_n > 16) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->score || a->D > INT64_MAX / a->ld) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->score, a->top_val, a->auc, a->f1)) return LLDA_E_BAD_ARG;
    if (misaligned(3, a->top_idx, a->n_thr, a->hit_rank, a->flags)) return LLDA_E_BAD_ARG;
    RankParams P;
    P.score = a->score; P.truth = a->truth;
    P.D = a->D; P.ld = a->ld;
    P.K = a->K; P.first = a->first; P.L = a->K - a->first; P.top_n = a->top_n;
    P.top_idx = a->top_idx; P.top_val = a->top_val; P.n_thr = a->n_thr; P.auc = a->auc; P.f1 = a->f1;
    P.hit_rank = a->hit_rank; P.flags = a->flags;
    int np = 16;
    while (np < P.L) np <<= 1;                          // (L <= 7688: np <= 8192)
    const int threads = np / 8 > 256 ? np / 8 : 256, docs = threads / (np / 8);
    P.n_tiles = (a->D + docs - 1) / docs;
    const dim3 grid((unsigned)(P.n_tiles < (1 << 20) ? P.n_tiles : (1 << 20))), block((unsigned)threads);
    hipStream_t st = (hipStream_t)stream;
    switch (np) {
#define LLDA_RANK(NP_) case NP_: hipLaunchKernelGGL(llda_rank_labels_kernel<NP_>, grid, block, 0, st, P); break;
    LLDA_RANK(16) LLDA_RANK(32) LLDA_RANK(64) LLDA_RANK(128) LLDA_RANK(256) LLDA_RANK(512) LLDA_RANK(1024) LLDA_RANK(2048)
    LLDA_RANK(4096) LLDA_RANK(8192)
#undef LLDA_RANK
    default: return LLDA_E_BAD_K;
    }
    return launched();
}

// the geometry of a row-chunk pass (llda_top_words, llda_scored_words) over `cols` columns, `per` of them to a thread: column chunks
// of a row, row phases of a workgroup, workgroups across a row, row chunks.  A column has chunks * rpb partial lists.
struct RowChunkGeometry { int32_t cpr, rpb, col_blocks; int64_t chunks; };

static RowChunkGeometry row_chunk_geometry(int32_t cols, int32_t per, int64_t V)
{
    RowChunkGeometry g;
    g.cpr = (cols + per - 1) / per;
    g.rpb = 256 / g.cpr;
    if (g.rpb < 1) g.rpb = 1;
    if (g.rpb > TOPW_MAX_PHASES) g.rpb = TOPW_MAX_PHASES;
    g.col_blocks = (g.cpr + 255) / 256;
    g.chunks = (V + LLDA_TOPW_CHUNK_ROWS - 1) / LLDA_TOPW_CHUNK_ROWS;
    return g;
}

int64_t llda_top_words_scratch_bytes(int64_t V, int32_t K, int32_t n)
{
    if (V < 1 || V > INT32_MAX || n < 1 || n > 16) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const RowChunkGeometry g = row_chunk_geometry(Lp->KP, 4, V);
    return g.chunks * g.rpb * Lp->KP * n * (int64_t)sizeof(uint64_t);
}

int llda_top_words(const int32_t *n_kw, int64_t V, int32_t K, int32_t n, int32_t *top_idx, int32_t *top_cnt, void *scratch,
                   int64_t scratch_bytes, void *stream)
{
    if (!n_kw || !scratch || V < 1 || V > INT32_MAX || n < 1 || n > 16) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (misaligned(15, n_kw) || misaligned(7, scratch) || misaligned(3, top_idx, top_cnt)) return LLDA_E_BAD_ARG;
    TopwParams P;
    memset(&P, 0, sizeof P);
    const RowChunkGeometry g = row_chunk_geometry(L.KP, 4, V);
    P.rpb = g.rpb;
    P.parts = g.chunks * g.rpb;
    if (scratch_bytes < P.parts * L.KP * n * (int64_t)sizeof(uint64_t)) return LLDA_E_BAD_ARG;
    P.n_kw = reinterpret_cast<const int4 *>(n_kw);
    P.V = V; P.cpr = g.cpr; P.n = n; P.KP = L.KP; P.G = L.G; P.T = L.T; P.K = L.K;
    P.scratch = static_cast<uint64_t *>(scratch);
    P.top_idx = top_idx; P.top_cnt = top_cnt;
    copy_leaves(L, P);
    const dim3 grid((unsigned)g.chunks, (unsigned)g.col_blocks), merge_grid((unsigned)L.KP);
    hipStream_t st = (hipStream_t)stream;
    return visit_at_least<2, 4, 8, 10, 16>(n, [&](auto N) {
        hipLaunchKernelGGL(llda_top_words_kernel<N.value>, grid, dim3(256), 0, st, P);
        hipLaunchKernelGGL(llda_top_words_merge_kernel<N.value>, merge_grid, dim3(64), 0, st, P);
        return launched();
    });
}

int llda_word_cooc(const int64_t *doc_off, const int32_t *word, int64_t D, int64_t V, int32_t K, int32_t n,
                   const int32_t *memb_off, const int32_t *memb, unsigned long long *co, void *stream)
{
    if (D < 0 || V < 1 || V > INT32_MAX || n < 1 || n > 16) return LLDA_E_BAD_ARG;
    if (K < 1 || K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (D == 0) return LLDA_OK;
    if (!doc_off || !word || !memb_off || !memb || !co) return LLDA_E_BAD_ARG;
    if (misaligned(7, doc_off, co)) return LLDA_E_BAD_ARG;
    if (misaligned(3, word, memb_off, memb)) return LLDA_E_BAD_ARG;
    CoocParams P;
    P.doc_off = doc_off; P.word = word; P.memb_off = memb_off; P.memb = memb; P.co = co;
    P.D = D; P.V = V; P.K = K; P.n = n; P.words = (K + 1) / 2;
    P.np = n * (n + 1) / 2; P.ks = 0;
    hipStream_t st = (hipStream_t)stream;
    // a large corpus: counters per slice of topics in LDS, when few slices cover K (kernel_cooc.hpp)
    const int ks_max = (COOC_AGG_LDS_WORDS / (P.np + 2)) & ~1;
    const int slices = (K + ks_max - 1) / ks_max;
    if (D >= LLDA_COOC_AGG_MIN_DOCS && slices <= COOC_AGG_MAX_SLICES) {
        P.ks = ((K + slices - 1) / slices + 1) & ~1;                         // even: two topics share a mask word
        const size_t lds = ((size_t)P.ks * P.np + (size_t)COOC_WAVES * (P.ks / 2)) * sizeof(uint32_t);
        const int rl = allow_lds(llda_word_cooc_agg_kernel, lds);
        if (rl) return rl;
        int64_t bx = (D + COOC_WAVES - 1) / COOC_WAVES;
        const int64_t cap = COOC_AGG_BLOCKS / slices > 1 ? COOC_AGG_BLOCKS / slices : 1;
        if (bx > cap) bx = cap;
        hipLaunchKernelGGL(llda_word_cooc_agg_kernel, dim3((unsigned)bx, (unsigned)slices), dim3(64 * COOC_WAVES), lds, st, P);
        return launched();
    }
    const size_t lds = (size_t)COOC_WAVES * P.words * sizeof(uint32_t);      // at most 61 504 bytes
    const int rl = allow_lds(llda_word_cooc_kernel, lds);
    if (rl) return rl;
    int64_t blocks = (D + COOC_WAVES - 1) / COOC_WAVES;
    if (blocks > LLDA_COOC_MAX_WAVES / COOC_WAVES) blocks = LLDA_COOC_MAX_WAVES / COOC_WAVES;
    hipLaunchKernelGGL(llda_word_cooc_kernel, dim3((unsigned)blocks), dim3(64 * COOC_WAVES), lds, st, P);
    return launched();
}

int llda_window_cooc(const int64_t *tok_off, const int32_t *tok, int64_t D, int64_t V, int32_t K, int32_t n, int32_t window,
                     const int32_t *memb_off, const int32_t *memb, unsigned long long *co, void *stream)
{
    if (D < 0 || V < 1 || V > INT32_MAX || n < 1 || n > 16 || window < 0 || window > LLDA_WINDOW_MAX) return LLDA_E_BAD_ARG;
    if (K < 1 || K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (D == 0) return LLDA_OK;
    if (!tok_off || !tok || !memb_off || !memb || !co) return LLDA_E_BAD_ARG;
    if (misaligned(7, tok_off, co)) return LLDA_E_BAD_ARG;
    if (misaligned(3, tok, memb_off, memb)) return LLDA_E_BAD_ARG;
    WindowParams P;
    P.tok_off = tok_off; P.tok = tok; P.memb_off = memb_off; P.memb = memb; P.co = co;
    P.D = D; P.V = V; P.K = K; P.n = n; P.window = window;
    P.np = n * (n + 1) / 2; P.cw = (n + 1) / 2;
    hipStream_t st = (hipStream_t)stream;
    const int state = WINDOW_WAVES * (2 + P.cw) * (int)sizeof(uint32_t);       // bytes per topic: the wavefronts' masks, `since`, counts
    // a large corpus: flushes go to counters per slice of topics in LDS, when few slices cover K (kernel_window.hpp)
    const int agg = P.np * (int)sizeof(unsigned long long) + state;
    const int agg_slices = (K + WINDOW_LDS_BYTES / agg - 1) / (WINDOW_LDS_BYTES / agg);
    if (D >= LLDA_WINDOW_AGG_MIN_DOCS && agg_slices <= WINDOW_AGG_MAX_SLICES) {
        P.ks = (K + agg_slices - 1) / agg_slices;
        const size_t lds = (size_t)P.ks * agg;
        const int rl = allow_lds(llda_window_cooc_kernel<true>, lds);
        if (rl) return rl;
        int64_t bx = (D + WINDOW_WAVES - 1) / WINDOW_WAVES;
        const int64_t cap = WINDOW_AGG_BLOCKS / agg_slices > 1 ? WINDOW_AGG_BLOCKS / agg_slices : 1;
        if (bx > cap) bx = cap;
        hipLaunchKernelGGL(llda_window_cooc_kernel<true>, dim3((unsigned)bx, (unsigned)agg_slices), dim3(64 * WINDOW_WAVES), lds, st, P);
        return launched();
    }
    const int slices = (K + WINDOW_LDS_BYTES / state - 1) / (WINDOW_LDS_BYTES / state);
    P.ks = (K + slices - 1) / slices;
    const size_t lds = (size_t)P.ks * state;
    const int rl = allow_lds(llda_window_cooc_kernel<false>, lds);
    if (rl) return rl;
    int64_t blocks = (D + WINDOW_WAVES - 1) / WINDOW_WAVES;
    if (blocks > LLDA_WINDOW_MAX_WAVES / WINDOW_WAVES) blocks = LLDA_WINDOW_MAX_WAVES / WINDOW_WAVES;
    hipLaunchKernelGGL(llda_window_cooc_kernel<false>, dim3((unsigned)blocks, (unsigned)slices), dim3(64 * WINDOW_WAVES), lds, st, P);
    return launched();
}

int llda_heldout_loglik(const llda_heldout_args *a, void *stream)
{
    HeldoutParams P;
    const int rc = doc_model_args(a, P, [] { return true; });
    if (rc || a->D == 0) return rc;
    if (misaligned(7, a->mant, a->expo)) return LLDA_E_BAD_ARG;
    P.mant = a->mant; P.expo = a->expo; P.tok = a->tok; P.bad = a->bad;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(64 * HELDOUT_WAVES);
    return launch_doc_model<HELDOUT_WAVES>(P,
        [&](auto G, dim3 grid, int64_t n_tiles) { hipLaunchKernelGGL(llda_heldout_group_kernel<G.value>, grid, block, 0, st, P, n_tiles); },
        [&](auto NI, dim3 grid) { hipLaunchKernelGGL((llda_heldout_wave_kernel<NI.value, heldout_u(NI.value)>), grid, block, 0, st, P); },
        [&](dim3 grid) {
            hipLaunchKernelGGL(llda_heldout_wide_kernel, grid, block, 0, st, P);
            return launched();
        });
}

int llda_attribute(const llda_attr_args *a, void *stream)
{
    AttrParams P;
    const int rc = doc_model_args(a, P, [&] {
        return !((a->theta_out && a->ld_out < a->K) || (a->credit && a->ld_credit < a->K) || a->iters < 0 || !(a->alpha >= 0.0) ||
                 a->top_m < 0 || a->top_m > LLDA_ATTR_MAX_TOP || (a->top_m > 0 && !a->site_idx != !a->site_val));
    });
    if (rc || a->D == 0) return rc;
    if ((a->theta_out && a->D > INT64_MAX / a->ld_out) || (a->credit && a->D > INT64_MAX / a->ld_credit)) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->theta_out, a->credit, a->site_val) || misaligned(3, a->site_idx)) return LLDA_E_BAD_ARG;
    P.ld_out = a->ld_out; P.ld_credit = a->ld_credit; P.iters = a->iters; P.alpha = a->alpha;
    P.theta_out = a->theta_out; P.credit = a->credit; P.tok = a->tok; P.bad = a->bad;
    const bool sites = a->top_m > 0 && a->site_idx;                          // (top_m = 0 or no buffers: nothing in the site loop)
    P.top_m = sites ? a->top_m : 0; P.site_idx = sites ? a->site_idx : nullptr; P.site_val = sites ? a->site_val : nullptr;
    hipStream_t st = (hipStream_t)stream;
    return sites ? launch_attr<true>(P, st) : launch_attr<false>(P, st);
}

int llda_leftright_struct_bytes(void) { return (int)sizeof(llda_leftright_args); }

int llda_left_to_right(const llda_leftright_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_leftright_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_NARROW_KP) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->ld_phi < a->K || (a->allowed && a->ld_allowed < a->K)) return LLDA_E_BAD_ARG;
    if (a->R < 1 || a->R > LLDA_LR_MAX_PARTICLES || !(a->alpha > 0.0) || !(a->alpha < INFINITY)) return LLDA_E_BAD_ARG;
    if (a->max_doc_tokens < 1 || a->max_doc_tokens > LLDA_LR_MAX_TOKENS) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->phi_t || !a->mant || !a->expo || !a->tok || !a->bad) return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi || (a->allowed && a->D > INT64_MAX / a->ld_allowed)) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->phi_t, a->doc_ids, a->mant, a->expo, a->tok, a->bad)) return LLDA_E_BAD_ARG;
    if (misaligned(3, a->word, a->status)) return LLDA_E_BAD_ARG;
    static_assert(LR_MAX_PARTICLES == LLDA_LR_MAX_PARTICLES && LLDA_LR_MAX_TOKENS < 0xFFFF, "kernel_leftright.hpp restates the header");
    LrParams P;
    P.doc_off = a->doc_off; P.word = a->word; P.phi_t = a->phi_t; P.allowed = a->allowed; P.doc_ids = a->doc_ids;
    P.D = a->D; P.V = a->V; P.ld_phi = a->ld_phi; P.ld_allowed = a->ld_allowed; P.doc_base = a->doc_base;
    P.K = a->K; P.R = a->R; P.cap = a->max_doc_tokens; P.alpha = a->alpha;
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32); P.stream_id = a->stream_id;
    P.mant = a->mant; P.expo = a->expo; P.tok = a->tok; P.bad = a->bad; P.status = a->status;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = lr_lds_bytes(P.R, P.cap);                            // at most 147 712 bytes
    const dim3 grid((unsigned)(P.D < (1 << 20) ? P.D : (1 << 20))), block(64 * P.R);
    return visit_int<1, 2, 4, 8, 16>(doc_geom(P.K).NI, [&](auto ni) {
        return visit_int<8, 16>(P.R <= 8 ? 8 : 16, [&](auto waves) {
            const auto kern = llda_leftright_kernel<ni.value, waves.value>;
            const int rl = allow_lds(kern, lds);
            if (rl) return rl;
            hipLaunchKernelGGL(kern, grid, block, lds, st, P);
            return launched();
        });
    });
}

int llda_nearest_struct_bytes(void) { return (int)sizeof(llda_nearest_args); }

// the row ranges llda_nearest_rows walks b in: the caller's count capped at D, or enough workgroups to fill the chip a few times
// while a range keeps eight tiles or more (every range fills its lists anew, and that costs about a tile's product)
static int64_t near_chunks(int64_t Q, int64_t D, int32_t chunks)
{
    if (D == 0) return 0;
    if (chunks > 0) return chunks < D ? chunks : D;
    const int64_t q_tiles = (Q + NEAR_T - 1) / NEAR_T, tiles = (D + NEAR_T - 1) / NEAR_T;
    int64_t want = q_tiles > 0 ? 2048 / q_tiles : 1;
    if (want > tiles / 8) want = tiles / 8;
    return want < 1 ? 1 : want;
}

int64_t llda_nearest_scratch_bytes(int64_t Q, int64_t D, int32_t n, int32_t chunks)
{
    if (Q < 0 || D < 0 || chunks < 0 || n < 1 || n > LLDA_NEAREST_MAX_N) return LLDA_E_BAD_ARG;
    const int64_t C = near_chunks(Q, D, chunks), per = 16 * (int64_t)n + 8;
    if (C > 0 && Q > (INT64_MAX - 16) / per / C) return LLDA_E_BAD_ARG;
    return Q * C * per + 16;                              // (never 0: a caller's allocation always has an address)
}

int llda_nearest_rows(const llda_nearest_args *a, void *stream)
{
    static_assert(NEAR_T == LLDA_NEAREST_TILE && NEAR_KS == LLDA_NEAREST_KSTEP && NEAR_MAX_N == LLDA_NEAREST_MAX_N,
                  "kernel_nearest.hpp restates the header");
    if (!a || a->struct_bytes != sizeof(llda_nearest_args)) return LLDA_E_BAD_ARG;
    if (!a->a || !a->b || !a->scratch || a->n < 1 || a->n > LLDA_NEAREST_MAX_N || a->L < 1) return LLDA_E_BAD_ARG;
    if (a->lda < a->L || a->ldb < a->L || a->Q < 0 || a->D < 0 || a->chunks < 0 || a->row_base < 0) return LLDA_E_BAD_ARG;
    if (a->row_base > INT64_MAX - a->D || a->Q > INT64_MAX / a->lda || a->D > INT64_MAX / a->ldb) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->a, a->b, a->exclude, a->top_idx, a->top_val, a->n_nan) || misaligned(7, a->scratch)) return LLDA_E_BAD_ARG;
    const int64_t need = llda_nearest_scratch_bytes(a->Q, a->D, a->n, a->chunks);
    if (need < 0 || a->scratch_bytes < need) return LLDA_E_BAD_ARG;
    const int64_t C = near_chunks(a->Q, a->D, a->chunks), q_tiles = (a->Q + NEAR_T - 1) / NEAR_T;
    if (C > 0 && q_tiles > INT32_MAX / C) return LLDA_E_BAD_ARG;
    if (a->Q == 0) return LLDA_OK;
    NearParams P;
    memset(&P, 0, sizeof P);
    P.a = a->a; P.b = a->b; P.Q = a->Q; P.D = a->D; P.lda = a->lda; P.ldb = a->ldb; P.row_base = a->row_base;
    P.exclude = a->exclude; P.L = a->L; P.n = a->n; P.chunks = (int32_t)C;
    P.part_val = static_cast<double *>(a->scratch);
    P.part_idx = reinterpret_cast<int64_t *>(P.part_val + a->Q * C * a->n);
    P.part_nan = P.part_idx + a->Q * C * a->n;
    P.top_idx = a->top_idx; P.top_val = a->top_val; P.n_nan = a->n_nan;
    hipStream_t st = (hipStream_t)stream;
    if (C > 0) {
        const dim3 grid((unsigned)(q_tiles * C));
        const bool vec = !misaligned(15, a->a, a->b) && !(a->lda & 1) && !(a->ldb & 1);
        if (vec) hipLaunchKernelGGL(llda_nearest_kernel<true>, grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL(llda_nearest_kernel<false>, grid, dim3(256), 0, st, P);
    }
    hipLaunchKernelGGL(llda_nearest_merge_kernel, dim3((unsigned)((a->Q + 63) / 64)), dim3(64), 0, st, P);
    return launched();
}

int llda_label_struct_bytes(void) { return (int)sizeof(llda_label_args); }
int llda_sets_struct_bytes(void) { return (int)sizeof(llda_sets_args); }

static int64_t label_chunk(int32_t chunk) { return chunk == 0 ? LABEL_CHUNK : chunk == LABEL_TEST_CHUNK ? LABEL_TEST_CHUNK : 0; }

int64_t llda_label_scratch_bytes(int64_t D, int32_t n_labels, int32_t chunk)
{
    const int64_t C = label_chunk(chunk);
    if (D < 0 || D > LLDA_LABEL_MAX_D || n_labels < 0 || n_labels > LLDA_MAX_K || C == 0) return LLDA_E_BAD_ARG;
    const int64_t Dp = (D + C - 1) / C * C;               // (Dp <= 2^30, n_labels < 2^13: the product stays below 2^48)
    return 24 * Dp * n_labels + 16;                       // (never 0: a caller's allocation always has an address)
}

// llda_label_sort_kernel over chunks of C, then the merge levels, on P's four arrays (Dp positions by n_labels).  Returns 0 when
// key_a / pay_a hold the sorted rows, 1 when key_b / pay_b do.
static int label_sort(LabelParams &P, int64_t C, hipStream_t st)
{
    const unsigned L = (unsigned)P.n_labels;
    const bool small = C == LABEL_TEST_CHUNK;
    if (small) hipLaunchKernelGGL(llda_label_sort_kernel<LABEL_TEST_CHUNK>, dim3((unsigned)(P.Dp / C), L), dim3(LABEL_TEST_CHUNK / 8), 0, st, P);
    else hipLaunchKernelGGL(llda_label_sort_kernel<LABEL_CHUNK>, dim3((unsigned)(P.Dp / C), L), dim3(LABEL_CHUNK / 8), 0, st, P);
    int flip = 0;
    for (int64_t R = C; R < P.Dp; R *= 2, flip ^= 1) {
        P.run = R;
        if (small) hipLaunchKernelGGL(llda_label_merge_kernel<LABEL_TEST_CHUNK>, dim3((unsigned)(P.Dp / LABEL_TEST_CHUNK), L), dim3(LABEL_TEST_CHUNK / 8), 0, st, P, flip);
        else hipLaunchKernelGGL(llda_label_merge_kernel<LABEL_TILE>, dim3((unsigned)(P.Dp / LABEL_TILE), L), dim3(LABEL_TILE / 8), 0, st, P, flip);
    }
    return flip;
}

int llda_label_metrics(const llda_label_args *a, void *stream)
{
    static_assert(LABEL_CHUNK == LLDA_LABEL_CHUNK && LABEL_TEST_CHUNK == LLDA_LABEL_TEST_CHUNK, "kernel_label.hpp restates the header");
    static_assert(LABEL_CHUNK % LABEL_TILE == 0 && LABEL_TILE == 8 * LABEL_WALK_NT && LABEL_TEST_CHUNK % 64 == 0, "label tiles");
    if (!a || a->struct_bytes != sizeof(llda_label_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->first < 0 || a->n_labels < 0 || a->first > a->K - a->n_labels || a->ld < a->K) return LLDA_E_BAD_ARG;
    if (a->D < 0 || a->D > LLDA_LABEL_MAX_D || label_chunk(a->chunk) == 0) return LLDA_E_BAD_ARG;
    if (a->D == 0 || a->n_labels == 0) return LLDA_OK;
    if (!a->score || !a->truth || !a->scratch || a->D > INT64_MAX / a->ld) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->score, a->n_pos, a->n_thr, a->auc_num, a->auc, a->thr_tp, a->thr_fp, a->f1, a->thr) || misaligned(7, a->scratch)) return LLDA_E_BAD_ARG;
    if (misaligned(3, a->flags, a->order)) return LLDA_E_BAD_ARG;
    const int64_t need = llda_label_scratch_bytes(a->D, a->n_labels, a->chunk);
    if (need < 0 || a->scratch_bytes < need) return LLDA_E_BAD_ARG;
    const int64_t C = label_chunk(a->chunk), Dp = (a->D + C - 1) / C * C, n = Dp * a->n_labels;
    LabelParams P;
    memset(&P, 0, sizeof P);
    P.score = a->score; P.truth = a->truth; P.D = a->D; P.ld = a->ld; P.Dp = Dp;
    P.K = a->K; P.first = a->first; P.n_labels = a->n_labels;
    P.key_a = static_cast<uint64_t *>(a->scratch);
    P.key_b = P.key_a + n;
    P.pay_a = reinterpret_cast<uint32_t *>(P.key_b + n);
    P.pay_b = P.pay_a + n;
    P.n_pos = a->n_pos; P.n_thr = a->n_thr; P.auc_num = a->auc_num; P.auc = a->auc; P.thr_tp = a->thr_tp; P.thr_fp = a->thr_fp;
    P.f1 = a->f1; P.thr = a->thr; P.flags = a->flags; P.order = a->order;
    hipStream_t st = (hipStream_t)stream;
    const unsigned L = (unsigned)a->n_labels;
    hipLaunchKernelGGL(llda_label_keys_kernel, dim3((unsigned)(Dp / 64), (L + 63) / 64), dim3(256), 0, st, P);
    const int flip = label_sort(P, C, st);
    P.key_sorted = flip ? P.key_b : P.key_a;
    P.pay_sorted = flip ? P.pay_b : P.pay_a;
    hipLaunchKernelGGL(llda_label_walk_kernel, dim3(L), dim3(LABEL_WALK_NT), 0, st, P);
    return launched();
}

int llda_label_sets(const llda_sets_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_sets_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->first < 0 || a->first > a->K || a->ld < a->K || a->D < 0 || a->D > INT64_MAX / a->ld) return LLDA_E_BAD_ARG;
    if (a->at_least_one != 0 && a->at_least_one != 1) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->score || !a->thr) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->score, a->thr, a->tp, a->fp, a->fn) || misaligned(3, a->mask, a->n_pred, a->n_hit, a->n_true)) return LLDA_E_BAD_ARG;
    SetsParams P;
    memset(&P, 0, sizeof P);
    P.score = a->score; P.thr = a->thr; P.truth = a->truth; P.D = a->D; P.ld = a->ld;
    P.K = a->K; P.first = a->first; P.at_least_one = a->at_least_one; P.W = (a->K + 31) / 32;
    P.mask = a->mask; P.n_pred = a->n_pred; P.n_hit = a->n_hit; P.n_true = a->n_true;
    P.tp = reinterpret_cast<unsigned long long *>(a->tp); P.fp = reinterpret_cast<unsigned long long *>(a->fp);
    P.fn = reinterpret_cast<unsigned long long *>(a->fn);
    // LDS: whole ballots of mask words per wavefront, and with truth three counters per label (K <= 7688: at most 100 KB)
    const size_t lds = sizeof(uint32_t) * ((size_t)SETS_WAVES * ((a->K + 63) / 64 * 2) + (a->truth ? 3 * (size_t)a->K : 0));
    const int rl = allow_lds(llda_label_sets_kernel, lds);
    if (rl) return rl;
    const int64_t rounds = (a->D + SETS_WAVES - 1) / SETS_WAVES;
    // every workgroup flushes K counters: a few workgroups per compute unit, each with many documents
    hipLaunchKernelGGL(llda_label_sets_kernel, dim3((unsigned)(rounds < SETS_MAX_BLOCKS ? rounds : SETS_MAX_BLOCKS)), dim3(SETS_WAVES * 64), lds, (hipStream_t)stream, P);
    return launched();
}

int llda_scored_struct_bytes(void) { return (int)sizeof(llda_scored_args); }

// the scratch of llda_scored_words over `cols` columns (KP in counts mode, K in matrix mode), two to a thread.  Per (part, column):
// n scores, n word ids, one NaN count (2 * cpr columns: a multiple of 8 bytes)
static RowChunkGeometry scored_geometry(int32_t cols, int64_t V) { return row_chunk_geometry(cols, 2, V); }

static int64_t scored_bytes(const RowChunkGeometry &g, int32_t n) { return g.chunks * g.rpb * (2 * (int64_t)g.cpr) * (12 * n + 4); }

int64_t llda_scored_words_scratch_bytes(int64_t V, int32_t K, int32_t n)
{
    if (V < 1 || V > INT32_MAX || n < 1 || n > 16) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const int64_t counts = scored_bytes(scored_geometry(Lp->KP, V), n), matrix = scored_bytes(scored_geometry(K, V), n);
    return counts > matrix ? counts : matrix;
}

int llda_scored_words(const llda_scored_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_scored_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    const bool counts = a->n_kw != nullptr;
    if (counts == (a->mat != nullptr)) return LLDA_E_BAD_ARG;
    if (a->n < 1 || a->n > 16 || a->a < 1 || a->a > 8 || a->V < 1 || a->V > INT32_MAX) return LLDA_E_BAD_ARG;
    if (counts ? (!a->n_k && !a->den) : (a->ld < a->K || a->ld > INT64_MAX / 8 / a->V)) return LLDA_E_BAD_ARG;
    if (!a->scratch) return LLDA_E_BAD_ARG;
    if (misaligned(15, a->n_kw) || misaligned(7, a->den, a->mat, a->wdiv, a->top_score) || misaligned(7, a->scratch)) return LLDA_E_BAD_ARG;
    if (misaligned(3, a->n_k, a->top_idx, a->n_nan)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(a->K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    const RowChunkGeometry g = scored_geometry(counts ? L.KP : a->K, a->V);
    if (a->scratch_bytes < scored_bytes(g, a->n)) return LLDA_E_BAD_ARG;
    ScoredParams P;
    memset(&P, 0, sizeof P);
    P.n_kw = reinterpret_cast<const int2 *>(a->n_kw);
    P.n_k = a->n_k; P.den = a->den; P.mat = a->mat; P.wdiv = a->wdiv;
    P.V = a->V; P.ld = a->ld; P.beta = a->beta; P.vbeta = (double)a->V * a->beta;
    P.cpr = g.cpr; P.rpb = g.rpb; P.n = a->n; P.a = a->a; P.C = 2 * g.cpr; P.K = a->K; P.G = L.G; P.T = L.T;
    P.parts = g.chunks * g.rpb;
    const int64_t lists = P.parts * P.C * a->n;
    P.part_score = static_cast<double *>(a->scratch);
    P.part_id = reinterpret_cast<uint32_t *>(P.part_score + lists);
    P.part_nan = reinterpret_cast<int32_t *>(P.part_id + lists);
    P.top_idx = a->top_idx; P.top_score = a->top_score; P.n_nan = a->n_nan;
    copy_leaves(L, P);
    const dim3 grid((unsigned)g.chunks, (unsigned)g.col_blocks), merge_grid((unsigned)(counts ? L.KP : a->K));
    hipStream_t st = (hipStream_t)stream;
    // 16-byte loads of a matrix row pair need the base 16-byte aligned and an even leading dimension
    const int mode = counts ? SCORED_COUNTS : (!misaligned(15, a->mat) && !(a->ld & 1)) ? SCORED_MATRIX_VEC : SCORED_MATRIX;
    return visit_at_least<4, 10, 16>(a->n, [&](auto N) {
        return visit_int<SCORED_COUNTS, SCORED_MATRIX, SCORED_MATRIX_VEC>(mode, [&](auto M) {
            hipLaunchKernelGGL((llda_scored_words_kernel<N.value, M.value>), grid, dim3(256), 0, st, P);
            hipLaunchKernelGGL(llda_scored_merge_kernel<N.value>, merge_grid, dim3(64), 0, st, P);
            return launched();
        });
    });
}

int llda_ecdf_struct_bytes(void) { return (int)sizeof(llda_ecdf_args); }
int llda_frex_struct_bytes(void) { return (int)sizeof(llda_frex_args); }

int64_t llda_ecdf_scratch_bytes(int64_t V, int32_t n_labels, int32_t chunk)
{
    const int64_t C = label_chunk(chunk);
    if (V < 1 || V > LLDA_ECDF_MAX_V || n_labels < 0 || n_labels > LLDA_MAX_K || C == 0) return LLDA_E_BAD_ARG;
    const int64_t Vp = (V + C - 1) / C * C;               // (Vp <= 2^30, n_labels < 2^13: the product stays below 2^48)
    return 24 * Vp * n_labels + 8 * V + 16;
}

int llda_ecdf_ranks(const llda_ecdf_args *a, void *stream)
{
    static_assert(LLDA_ECDF_MAX_V == LLDA_LABEL_MAX_D, "the ECDF sort is the label sort");
    if (!a || a->struct_bytes != sizeof(llda_ecdf_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->first < 0 || a->n_labels < 0 || a->first > a->K - a->n_labels || a->ld < a->K) return LLDA_E_BAD_ARG;
    if (a->V < 1 || a->V > LLDA_ECDF_MAX_V || label_chunk(a->chunk) == 0 || (a->mode != 0 && a->mode != 1)) return LLDA_E_BAD_ARG;
    if (a->n_labels == 0) return LLDA_OK;
    if (!a->mat || !a->rank || !a->scratch || a->V > INT64_MAX / 8 / a->ld) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->mat, a->value, a->n_cand) || misaligned(7, a->scratch) || misaligned(3, a->rank)) return LLDA_E_BAD_ARG;
    const int64_t need = llda_ecdf_scratch_bytes(a->V, a->n_labels, a->chunk);
    if (need < 0 || a->scratch_bytes < need) return LLDA_E_BAD_ARG;
    const int64_t C = label_chunk(a->chunk), Vp = (a->V + C - 1) / C * C, n = Vp * a->n_labels;
    LabelParams S;                                        // the sort and the merge levels of llda_label_metrics, on these arrays
    memset(&S, 0, sizeof S);
    S.D = a->V; S.Dp = Vp; S.n_labels = a->n_labels;
    S.key_a = static_cast<uint64_t *>(a->scratch);
    S.key_b = S.key_a + n;
    S.pay_a = reinterpret_cast<uint32_t *>(S.key_b + n);
    S.pay_b = S.pay_a + n;
    EcdfParams P;
    memset(&P, 0, sizeof P);
    P.mat = a->mat; P.cand = a->cand; P.V = a->V; P.ld = a->ld; P.Vp = Vp;
    P.K = a->K; P.first = a->first; P.n_labels = a->n_labels; P.mode = a->mode;
    P.tot = reinterpret_cast<double *>(S.pay_b + n);      // (24 n bytes in: 8-byte aligned)
    P.key_a = S.key_a; P.pay_a = S.pay_a;
    P.rank = a->rank; P.value = a->value; P.n_cand = a->n_cand;
    hipStream_t st = (hipStream_t)stream;
    const unsigned L = (unsigned)a->n_labels;
    const int64_t rounds = (a->V + ECDF_WAVES - 1) / ECDF_WAVES;
    hipLaunchKernelGGL(llda_ecdf_totals_kernel, dim3((unsigned)(rounds < (1 << 20) ? rounds : (1 << 20))), dim3(ECDF_WAVES * 64), 0, st, P);
    hipLaunchKernelGGL(llda_ecdf_keys_kernel, dim3((unsigned)(Vp / 64), (L + 63) / 64), dim3(256), 0, st, P);
    const int flip = label_sort(S, C, st);
    P.key_sorted = flip ? S.key_b : S.key_a;
    P.pay_sorted = flip ? S.pay_b : S.pay_a;
    hipLaunchKernelGGL(llda_ecdf_walk_kernel, dim3(L), dim3(LABEL_WALK_NT), 0, st, P);
    return launched();
}

int64_t llda_frex_scratch_bytes(int64_t V, int32_t n_labels, int32_t n)
{
    if (V < 1 || V > LLDA_ECDF_MAX_V || n_labels < 0 || n_labels > LLDA_MAX_K || n < 1 || n > LLDA_FREX_MAX_N) return LLDA_E_BAD_ARG;
    return 12 * (int64_t)n * ((V + FREX_CHUNK - 1) / FREX_CHUNK) * n_labels + 16;    // (below 2^37)
}

int llda_frex_select(const llda_frex_args *a, void *stream)
{
    static_assert(FREX_CHUNK == LLDA_FREX_CHUNK && FREX_CHUNK % (64 * FREX_UNROLL) == 0, "kernel_ecdf.hpp restates the header");
    if (!a || a->struct_bytes != sizeof(llda_frex_args)) return LLDA_E_BAD_ARG;
    if (a->n_labels < 0 || a->n_labels > LLDA_MAX_K || a->V < 1 || a->V > LLDA_ECDF_MAX_V || a->Vc < 1 || a->Vc > LLDA_ECDF_MAX_V) return LLDA_E_BAD_ARG;
    if (a->t < 1 || a->t > LLDA_FREX_MAX_T || a->s < 0 || a->s > a->t) return LLDA_E_BAD_ARG;
    if (a->n < 1 || a->n > LLDA_FREX_MAX_N || a->m < 0 || a->m > LLDA_FREX_MAX_N) return LLDA_E_BAD_ARG;
    if (a->n_labels == 0) return LLDA_OK;
    if (!a->rank_f || !a->rank_e || !a->scratch) return LLDA_E_BAD_ARG;
    if (misaligned(3, a->rank_f, a->rank_e, a->probe, a->top_idx, a->top_rank_f, a->top_rank_e, a->probe_rank_f, a->probe_rank_e)
        || misaligned(7, a->scratch)) return LLDA_E_BAD_ARG;
    const int64_t need = llda_frex_scratch_bytes(a->V, a->n_labels, a->n);
    if (need < 0 || a->scratch_bytes < need) return LLDA_E_BAD_ARG;
    FrexParams P;
    memset(&P, 0, sizeof P);
    P.rank_f = a->rank_f; P.rank_e = a->rank_e; P.probe = a->m > 0 ? a->probe : nullptr;
    P.V = a->V; P.Vc = a->Vc; P.parts = (a->V + FREX_CHUNK - 1) / FREX_CHUNK;
    P.n_labels = a->n_labels; P.n = a->n; P.m = a->m; P.s = a->s; P.u = a->t - a->s;
    P.part = static_cast<int32_t *>(a->scratch);
    P.top_idx = a->top_idx; P.top_rank_f = a->top_rank_f; P.top_rank_e = a->top_rank_e;
    P.probe_rank_f = a->probe_rank_f; P.probe_rank_e = a->probe_rank_e;
    const dim3 grid((unsigned)P.parts, (unsigned)a->n_labels), merge_grid((unsigned)a->n_labels);
    hipStream_t st = (hipStream_t)stream;
    return visit_at_least<4, 10, 16>(a->n, [&](auto N) {
        hipLaunchKernelGGL(llda_frex_select_kernel<N.value>, grid, dim3(64), 0, st, P);
        hipLaunchKernelGGL(llda_frex_merge_kernel<N.value>, merge_grid, dim3(64), 0, st, P);
        return launched();
    });
}

int llda_wcredit_struct_bytes(void) { return (int)sizeof(llda_wcredit_args); }
int llda_phistep_struct_bytes(void) { return (int)sizeof(llda_phistep_args); }

int64_t llda_credit_words_scratch_bytes(int64_t V, int64_t S, int32_t K, int32_t chunk)
{
    if (V < 1 || V > INT32_MAX || S < 0 || S > LLDA_WCREDIT_MAX_SITES || K < 1 || K > LLDA_MAX_K || chunk < 1) return LLDA_E_BAD_ARG;
    return 16 * (V + 1) + wcredit_rows(S, chunk) * (8 * (int64_t)K + 16) + (4 * wcredit_chunks_cap(V, S, chunk) + 7) / 8 * 8 + 16;    // (below 2^58)
}

int llda_credit_words(const llda_wcredit_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_wcredit_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->S < 0 || a->S > LLDA_WCREDIT_MAX_SITES || a->chunk < 1) return LLDA_E_BAD_ARG;
    if (a->ld_theta < a->K || a->ld_phi < a->K || a->ld_credit < a->K) return LLDA_E_BAD_ARG;
    if (a->D > INT64_MAX / a->ld_theta || a->V > INT64_MAX / a->ld_phi || a->V > INT64_MAX / a->ld_credit) return LLDA_E_BAD_ARG;
    if (a->S > 0 && (!a->word_off || !a->site_doc || !a->phi_t || !a->scratch || (a->D > 0 && !a->theta))) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->word_off, a->theta, a->phi_t, a->credit_w, a->tok, a->bad) || misaligned(7, a->scratch) || misaligned(3, a->site_doc, a->freq))
        return LLDA_E_BAD_ARG;
    const int64_t need = llda_credit_words_scratch_bytes(a->V, a->S, a->K, a->chunk);
    if (a->S > 0 && (need < 0 || a->scratch_bytes < need)) return LLDA_E_BAD_ARG;
    if (!a->credit_w && !a->tok && !a->bad) return LLDA_OK;
    WCreditParams P;
    memset(&P, 0, sizeof P);
    P.word = a->site_doc; P.freq = a->freq; P.K = a->K;
    // the rows that stream in are theta's.  No document at all: every site is not ok and reads row 0 "in its place", which is phi_t's
    P.phi_t = a->D > 0 ? a->theta : a->phi_t; P.ld_phi = a->D > 0 ? a->ld_theta : a->ld_phi; P.V = a->D;
    P.word_off = a->word_off; P.wphi = a->phi_t; P.n_words = a->V; P.ld_wphi = a->ld_phi; P.ld_credit = a->ld_credit;
    P.S = a->S; P.chunk = a->chunk; P.rows_cap = wcredit_rows(a->S, a->chunk);
    P.credit_w = a->credit_w; P.tok = a->tok; P.bad = a->bad;
    hipStream_t st = (hipStream_t)stream;
    if (a->S > 0) {
        P.cfirst = static_cast<int64_t *>(a->scratch);
        P.pfirst = P.cfirst + (a->V + 1);
        P.ptok = P.pfirst + (a->V + 1);
        P.pbad = P.ptok + P.rows_cap;
        P.part = reinterpret_cast<double *>(P.pbad + P.rows_cap);
        P.cword = reinterpret_cast<int32_t *>(P.part + P.rows_cap * a->K);
        P.chunks_cap = wcredit_chunks_cap(a->V, a->S, a->chunk);
        hipLaunchKernelGGL(llda_wcredit_index_kernel, dim3(1), dim3(WCREDIT_INDEX_NT), 0, st, P);
        const int rc = launch_wcredit(P, P.chunks_cap, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(llda_wcredit_combine_kernel, doc_grid((a->V + WCREDIT_WAVES - 1) / WCREDIT_WAVES), dim3(64 * WCREDIT_WAVES), 0, st, P);
    return launched();
}

int llda_attr_sparse_struct_bytes(void) { return (int)sizeof(llda_attr_sparse_args); }
int llda_wcredit_sparse_struct_bytes(void) { return (int)sizeof(llda_wcredit_sparse_args); }

int llda_attribute_sparse(const llda_attr_sparse_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_attr_sparse_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->NL < 0 || a->ld_phi < a->K) return LLDA_E_BAD_ARG;
    if (a->max_labels < 1 || a->max_labels > LLDA_SPARSE_MAX_LABELS || a->iters < 0 || !(a->alpha >= 0.0) || a->top_m < 0 ||
        a->top_m > LLDA_ATTR_MAX_TOP || (a->top_m > 0 && !a->site_idx != !a->site_val))
        return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->lab_off || !a->phi_t || (a->NL > 0 && (!a->lab || !a->theta_s))) return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->lab_off, a->theta_s, a->phi_t, a->tok, a->bad) || misaligned(7, a->theta_out, a->credit, a->site_val) ||
        misaligned(3, a->word, a->freq, a->lab, a->site_idx))
        return LLDA_E_BAD_ARG;
    AttrSparseParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.word = a->word; P.freq = a->freq; P.phi_t = a->phi_t;
    P.D = a->D; P.V = a->V; P.ld_phi = a->ld_phi; P.K = a->K;
    P.sets.lab_off = a->lab_off; P.sets.lab = a->lab; P.sets.theta_s = a->theta_s; P.sets.NL = a->NL; P.sets.max_labels = a->max_labels;
    P.iters = a->iters; P.alpha = a->alpha;
    P.theta_out = a->theta_out; P.credit = a->credit; P.tok = a->tok; P.bad = a->bad;
    const bool sites = a->top_m > 0 && a->site_idx;                          // (top_m = 0 or no buffers: nothing in the site loop)
    P.top_m = sites ? a->top_m : 0; P.site_idx = sites ? a->site_idx : nullptr; P.site_val = sites ? a->site_val : nullptr;
    hipStream_t st = (hipStream_t)stream;
    return sites ? launch_attr_sparse<true>(P, st) : launch_attr_sparse<false>(P, st);
}

int64_t llda_credit_words_sparse_scratch_bytes(int64_t V, int64_t S, int32_t K, int32_t chunk)
{
    return llda_credit_words_scratch_bytes(V, S, K, chunk);                  // (the same index tables and partial rows)
}

int llda_credit_words_sparse(const llda_wcredit_sparse_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_wcredit_sparse_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->S < 0 || a->S > LLDA_WCREDIT_MAX_SITES || a->NL < 0 || a->chunk < 1) return LLDA_E_BAD_ARG;
    if (a->max_labels < 1 || a->max_labels > LLDA_SPARSE_MAX_LABELS || a->ld_phi < a->K || a->ld_credit < a->K) return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi || a->V > INT64_MAX / a->ld_credit) return LLDA_E_BAD_ARG;
    if (a->S > 0 && (!a->word_off || !a->site_doc || !a->phi_t || !a->scratch || (a->D > 0 && !a->lab_off) || (a->NL > 0 && (!a->lab || !a->theta_s))))
        return LLDA_E_BAD_ARG;
    if (misaligned(7, a->word_off, a->lab_off, a->theta_s, a->phi_t, a->credit_w, a->tok) || misaligned(7, a->bad) || misaligned(7, a->scratch) ||
        misaligned(3, a->site_doc, a->freq, a->lab))
        return LLDA_E_BAD_ARG;
    const int64_t need = llda_credit_words_sparse_scratch_bytes(a->V, a->S, a->K, a->chunk);
    if (a->S > 0 && (need < 0 || a->scratch_bytes < need)) return LLDA_E_BAD_ARG;
    if (!a->credit_w && !a->tok && !a->bad) return LLDA_OK;
    WCreditSparseParams P;
    memset(&P, 0, sizeof P);
    P.word = a->site_doc; P.freq = a->freq; P.K = a->K; P.V = a->D;          // (the "words" of the sites are document ids)
    P.sets.lab_off = a->lab_off; P.sets.lab = a->lab; P.sets.theta_s = a->theta_s; P.sets.NL = a->NL; P.sets.max_labels = a->max_labels;
    P.word_off = a->word_off; P.wphi = a->phi_t; P.n_words = a->V; P.ld_wphi = a->ld_phi; P.ld_credit = a->ld_credit;
    P.S = a->S; P.chunk = a->chunk; P.rows_cap = wcredit_rows(a->S, a->chunk);
    P.credit_w = a->credit_w; P.tok = a->tok; P.bad = a->bad;
    hipStream_t st = (hipStream_t)stream;
    if (a->S > 0) {
        P.cfirst = static_cast<int64_t *>(a->scratch);
        P.pfirst = P.cfirst + (a->V + 1);
        P.ptok = P.pfirst + (a->V + 1);
        P.pbad = P.ptok + P.rows_cap;
        P.part = reinterpret_cast<double *>(P.pbad + P.rows_cap);
        P.cword = reinterpret_cast<int32_t *>(P.part + P.rows_cap * a->K);
        P.chunks_cap = wcredit_chunks_cap(a->V, a->S, a->chunk);
        hipLaunchKernelGGL(llda_wcredit_index_kernel, dim3(1), dim3(WCREDIT_INDEX_NT), 0, st, P);
        const int rc = launch_wcredit_sparse(P, P.chunks_cap, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(llda_wcredit_combine_kernel, doc_grid((a->V + WCREDIT_WAVES - 1) / WCREDIT_WAVES), dim3(64 * WCREDIT_WAVES), 0, st, P);
    return launched();
}

int llda_heldout_sparse_struct_bytes(void) { return (int)sizeof(llda_heldout_sparse_args); }
int llda_leftright_sparse_struct_bytes(void) { return (int)sizeof(llda_leftright_sparse_args); }

int llda_heldout_loglik_sparse(const llda_heldout_sparse_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_heldout_sparse_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->NL < 0 || a->ld_phi < a->K) return LLDA_E_BAD_ARG;
    if (a->max_labels < 1 || a->max_labels > LLDA_SPARSE_MAX_LABELS) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->lab_off || !a->phi_t || (a->NL > 0 && (!a->lab || !a->theta_s))) return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->lab_off, a->theta_s, a->phi_t, a->tok, a->bad) || misaligned(7, a->mant, a->expo) ||
        misaligned(3, a->word, a->freq, a->lab))
        return LLDA_E_BAD_ARG;
    HeldoutSparseParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.word = a->word; P.freq = a->freq; P.phi_t = a->phi_t;
    P.D = a->D; P.V = a->V; P.ld_phi = a->ld_phi; P.K = a->K;
    P.sets.lab_off = a->lab_off; P.sets.lab = a->lab; P.sets.theta_s = a->theta_s; P.sets.NL = a->NL; P.sets.max_labels = a->max_labels;
    P.mant = a->mant; P.expo = a->expo; P.tok = a->tok; P.bad = a->bad;
    hipStream_t st = (hipStream_t)stream;
    return visit_int<8, 16, 32>(sparse_group(a->max_labels), [&](auto G) {
        constexpr int docs = 64 * HELDOUT_WAVES / G.value;
        const int64_t n_tiles = (P.D + docs - 1) / docs;
        hipLaunchKernelGGL(llda_heldout_sparse_kernel<G.value>, doc_grid(n_tiles), dim3(64 * HELDOUT_WAVES), 0, st, P, n_tiles);
        return launched();
    });
}

int llda_left_to_right_sparse(const llda_leftright_sparse_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_leftright_sparse_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->NL < 0 || a->ld_phi < a->K) return LLDA_E_BAD_ARG;
    if (a->max_labels < 1 || a->max_labels > LLDA_SPARSE_MAX_LABELS) return LLDA_E_BAD_ARG;
    if (a->R < 1 || a->R > LLDA_LR_MAX_PARTICLES || !(a->alpha > 0.0) || !(a->alpha < INFINITY)) return LLDA_E_BAD_ARG;
    if (a->max_doc_tokens < 1 || a->max_doc_tokens > LLDA_LR_MAX_TOKENS) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->lab_off || !a->phi_t || !a->mant || !a->expo || !a->tok || !a->bad || (a->NL > 0 && !a->lab))
        return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->lab_off, a->phi_t, a->doc_ids, a->mant, a->expo, a->tok) || misaligned(7, a->bad) ||
        misaligned(3, a->word, a->lab, a->status))
        return LLDA_E_BAD_ARG;
    static_assert(LLDA_SPARSE_MAX_LABELS <= LRS_NONE && LLDA_LR_MAX_PARTICLES * 32 == LRS_MAX_THREADS, "kernel_lrsparse.hpp restates the header");
    LrSparseParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.word = a->word; P.phi_t = a->phi_t; P.doc_ids = a->doc_ids;
    P.D = a->D; P.V = a->V; P.ld_phi = a->ld_phi; P.doc_base = a->doc_base;
    P.K = a->K; P.R = a->R; P.cap = a->max_doc_tokens; P.alpha = a->alpha;
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32); P.stream_id = a->stream_id;
    P.mant = a->mant; P.expo = a->expo; P.tok = a->tok; P.bad = a->bad; P.status = a->status;
    P.sets.lab_off = a->lab_off; P.sets.lab = a->lab; P.sets.NL = a->NL; P.sets.max_labels = a->max_labels;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = lrs_lds_bytes(P.R, P.cap);                           // at most 82 176 bytes
    const dim3 grid((unsigned)(P.D < (1 << 20) ? P.D : (1 << 20)));
    return visit_int<8, 16, 32>(sparse_group(a->max_labels), [&](auto G) {
        const auto kern = llda_leftright_sparse_kernel<G.value>;
        const int rl = allow_lds(kern, lds);
        if (rl) return rl;
        const int waves = (P.R * G.value + 63) / 64;                        // 64 / G particles per wavefront
        hipLaunchKernelGGL(kern, grid, dim3(64 * waves), lds, st, P);
        return launched();
    });
}

int llda_foldin_sparse_struct_bytes(void) { return (int)sizeof(llda_foldin_sparse_args); }

int llda_foldin_sparse(const llda_foldin_sparse_args *a, void *stream)
{
    if (!a || a->struct_bytes != sizeof(llda_foldin_sparse_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->D < 0 || a->V < 1 || a->V > INT32_MAX || a->NL < 0 || a->ld_phi < a->K) return LLDA_E_BAD_ARG;
    if (a->max_labels < 1 || a->max_labels > LLDA_SPARSE_MAX_LABELS || a->iters < 0 || a->thinning < 1) return LLDA_E_BAD_ARG;
    if (!(a->c_init > 1.0) || !(a->c_loop > 1.0) || a->alpha != a->alpha) return LLDA_E_BAD_ARG;
    if (a->D == 0) return LLDA_OK;
    if (!a->doc_off || !a->word || !a->freq || !a->lab_off || !a->phi_t || !a->z || (a->NL > 0 && (!a->lab || !a->n_dk_s || !a->th_s)))
        return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / a->ld_phi) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->doc_off, a->lab_off, a->phi_t, a->doc_ids, a->th_s) || misaligned(3, a->word, a->freq, a->lab, a->z, a->n_dk_s) ||
        misaligned(3, a->status))
        return LLDA_E_BAD_ARG;
    static_assert(LLDA_SPARSE_MAX_LABELS == 32, "kernel_foldinsparse.hpp holds a list in 8 lanes of 4 slots");
    FoldinSparseParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.word = a->word; P.freq = a->freq; P.phi_t = a->phi_t; P.doc_ids = a->doc_ids;
    P.z = a->z; P.n_dk_s = a->n_dk_s; P.th_s = a->th_s; P.status = a->status;
    P.sets.lab_off = a->lab_off; P.sets.lab = a->lab; P.sets.NL = a->NL; P.sets.max_labels = a->max_labels;
    P.D = a->D; P.V = a->V; P.ld_phi = a->ld_phi; P.doc_base = a->doc_base;
    P.alpha = a->alpha; P.c_init = a->c_init; P.c_loop = a->c_loop;
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32); P.stream_id = a->stream_id;
    P.K = a->K; P.iters = a->iters; P.thinning = a->thinning;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_tiles = (P.D + FS_DOCS - 1) / FS_DOCS;
    return visit_int<1, 2, 4>(foldin_sparse_slots(a->max_labels), [&](auto T) {
        hipLaunchKernelGGL(llda_foldin_sparse_kernel<T.value>, doc_grid(n_tiles), dim3(FS_THREADS), 0, st, P, n_tiles);
        return launched();
    });
}

int64_t llda_phi_step_scratch_bytes(int64_t V, int32_t K)
{
    if (V < 1 || V > INT32_MAX || K < 1 || K > LLDA_MAX_K) return LLDA_E_BAD_ARG;
    return ((V + PHISTEP_ROWS - 1) / PHISTEP_ROWS + 1) * 8 * (int64_t)K + 16;
}

int llda_phi_step(const llda_phistep_args *a, void *stream)
{
    static_assert(PHISTEP_ROWS == LLDA_COLSUM_ROWS, "kernel_emfit.hpp restates the header");
    if (!a || a->struct_bytes != sizeof(llda_phistep_args)) return LLDA_E_BAD_ARG;
    if (a->K < 1 || a->K > LLDA_MAX_K) return LLDA_E_BAD_K;
    if (a->V < 1 || a->V > INT32_MAX || a->ld < a->K || a->ld_out < a->K) return LLDA_E_BAD_ARG;
    if (!(a->beta > 0.0) || !(a->beta < INFINITY)) return LLDA_E_BAD_ARG;
    if (!a->cw || !a->phi_t_out || !a->scratch) return LLDA_E_BAD_ARG;
    if (a->V > INT64_MAX / 8 / a->ld || a->V > INT64_MAX / 8 / a->ld_out) return LLDA_E_BAD_ARG;
    if (misaligned(7, a->cw, a->phi_t_out, a->den) || misaligned(7, a->scratch)) return LLDA_E_BAD_ARG;
    const int64_t need = llda_phi_step_scratch_bytes(a->V, a->K);
    if (need < 0 || a->scratch_bytes < need) return LLDA_E_BAD_ARG;
    PhiStepParams P;
    memset(&P, 0, sizeof P);
    P.cw = a->cw; P.out = a->phi_t_out; P.den_out = a->den;
    P.V = a->V; P.ld = a->ld; P.ld_out = a->ld_out; P.K = a->K;
    P.n_blocks = (a->V + PHISTEP_ROWS - 1) / PHISTEP_ROWS;
    P.bsum = static_cast<double *>(a->scratch);
    P.den = P.bsum + P.n_blocks * a->K;
    P.beta = a->beta; P.Vb = (double)a->V * a->beta;
    hipStream_t st = (hipStream_t)stream;
    const unsigned kb = (unsigned)((a->K + PHISTEP_NT - 1) / PHISTEP_NT);
    hipLaunchKernelGGL(llda_phistep_block_kernel, dim3((unsigned)P.n_blocks, kb), dim3(PHISTEP_NT), 0, st, P);
    hipLaunchKernelGGL(llda_phistep_den_kernel, dim3(kb), dim3(PHISTEP_NT), 0, st, P);
    const int64_t blocks = (a->V * a->K + PHISTEP_NT - 1) / PHISTEP_NT;
    hipLaunchKernelGGL(llda_phistep_div_kernel, doc_grid(blocks, 1 << 16), dim3(PHISTEP_NT), 0, st, P);
    return launched();
}

int llda_loglik(const int64_t *doc_off, const int32_t *word, const uint16_t *lab_mask, const int32_t *n_dk,
                const int32_t *n_kw, const int32_t *n_k, int64_t D, int64_t V, int32_t K, double alpha,
                double beta, double *out_doc, void *stream)
{
    if (D < 0 || V < 1) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (D == 0) return LLDA_OK;
    if (!doc_off || !word || !lab_mask || !n_dk || !n_kw || !n_k || !out_doc) return LLDA_E_BAD_ARG;
    LParams P;
    P.doc_off = doc_off; P.word = word; P.lab_mask = lab_mask; P.n_dk = n_dk; P.n_kw = n_kw; P.n_k = n_k;
    P.out_doc = out_doc; P.D = D; P.alpha = alpha; P.beta = beta; P.vbeta = (double)V * beta;
    hipStream_t st = (hipStream_t)stream;
    if (L.wide) {
        WLParams W;
        W.l = P; W.NT = L.tiers; W.T = L.T; W.G = L.G; W.KP = L.KP;
        const size_t lds = (size_t)L.KP * 16;
        const int rl = allow_lds(llda_loglik_wide_kernel, lds);
        if (rl) return rl;
        hipLaunchKernelGGL(llda_loglik_wide_kernel, dim3(wide_blocks(D)), dim3(64), lds, st, W);
        return launched();
    }
    return visit_layout(L.G, L.T, [&](auto g, auto t) { return launch_loglik<g.value, t.value>(P, st); });
}

static void readout_layout(const llda_layout &L, RParams &P)
{
    P.K = L.K; P.KP = L.KP; P.T = L.T;
    copy_leaves(L, P);
    fill_schedule(L, P.last_leaf, P.tail, P.tail_row, P.n_rounds, P.xor_tree, P.rounds_pk);
}

int llda_readout_phi(const int32_t *n_kw, const int32_t *n_k, const double *den, int64_t V, int32_t K, double beta,
                     int32_t mode, double keep, double share, double *out, int32_t *flags, void *stream)
{
    if (V < 1 || (mode != 0 && mode != 1) || !n_kw || (!n_k && !den) || !out) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    RParams P;
    memset(&P, 0, sizeof P);
    readout_layout(L, P);
    P.n_kw = n_kw; P.n_k = n_k; P.den = den; P.out = out; P.flags = flags; P.V = V; P.mode = mode;
    P.beta = beta; P.vbeta = (double)V * beta; P.keep = keep; P.share = share;
    hipLaunchKernelGGL(llda_readout_phi_kernel, dim3((unsigned)((V + 63) / 64)), dim3(256), 0, (hipStream_t)stream, P);
    return launched();
}

int llda_readout_theta(const int32_t *n_dk, const uint16_t *lab_mask, int64_t D, int32_t K, double alpha, int32_t mode,
                       double keep, double share, double *out, void *stream)
{
    if (D < 0 || (mode != 0 && mode != 1)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (D == 0) return LLDA_OK;
    if (!n_dk || !lab_mask || !out) return LLDA_E_BAD_ARG;
    if (L.wide) {
        WRParams W;
        memset(&W, 0, sizeof W);
        W.n_dk = n_dk; W.lab_mask = lab_mask; W.out = out; W.D = D; W.K = L.K; W.mode = mode; W.alpha = alpha;
        W.keep = keep; W.share = share;
        copy_leaves(L, W);
        fill_wide(L, W.w);
        const size_t lds = (size_t)L.KP * 8;
        const int rl = allow_lds(llda_readout_theta_wide_kernel, lds);
        if (rl) return rl;
        hipLaunchKernelGGL(llda_readout_theta_wide_kernel, dim3(wide_blocks(D)), dim3(64), lds, (hipStream_t)stream, W);
        return launched();
    }
    RParams P;
    memset(&P, 0, sizeof P);
    readout_layout(L, P);
    P.n_dk = n_dk; P.lab_mask = lab_mask; P.out = out; P.D = D; P.mode = mode; P.alpha = alpha;
    P.keep = keep; P.share = share;
    hipStream_t st = (hipStream_t)stream;
    const bool has_tail = L.tail != 0;
    return visit_layout(L.G, L.T, [&](auto g, auto t) { return launch_theta<g.value, t.value>(P, has_tail, st); });
}

int llda_foldin(const llda_foldin_args *a, void *stream)
{
    if (!a || !a->doc_off || !a->word || !a->init_idx || !a->freq || !a->ph || !a->init_rows || !a->z || !a->n_dk ||
        !a->th || !a->slot_valid || a->D < 0 || a->iters < 0 || a->thinning < 1)
        return LLDA_E_BAD_ARG;
    // `while prob.sum() > 1: prob /= c` ends only for c > 1 (NaN refused too)
    if (!(a->c_init > 1.0) || !(a->c_loop > 1.0)) return LLDA_E_BAD_ARG;
    int rc;
    const llda_layout *Lp = layout_of(a->K, &rc);
    if (rc) return rc;
    const llda_layout &L = *Lp;
    if (a->D == 0) return LLDA_OK;
    FParams P;
    memset(&P, 0, sizeof P);
    P.doc_off = a->doc_off; P.word = a->word; P.init_idx = a->init_idx; P.freq = a->freq; P.z = a->z;
    P.ph = a->ph; P.phn = a->init_rows; P.n_dk = a->n_dk; P.th = a->th; P.slot_valid = a->slot_valid;
    P.status = a->status; P.D = a->D; P.doc_base = a->doc_base; P.doc_ids = a->doc_ids; P.alpha = a->alpha; P.beta = a->beta;
    P.c_init = a->c_init; P.c_loop = a->c_loop;
    P.key0 = (uint32_t)a->seed; P.key1 = (uint32_t)(a->seed >> 32); P.stream_id = a->stream_id;
    P.iters = a->iters; P.thinning = a->thinning; P.beta_fallback = a->beta_fallback; P.avg_mode = a->avg_mode;
    // the decided tier needs non-negative scores and a divisor c whose distance from 1 dwarfs the rounding of a normalised sum
    P.exact_only = (a->exact_only != 0 || !(a->alpha >= 0.0) || !(a->c_loop - 1.0 >= 1e-9)) ? 1 : 0;
    P.n_sites = a->n_sites > 0 ? a->n_sites : 0;
    P.ph_base = a->ph_base; P.doc_stream = a->doc_stream;
    fill_schedule(L, P.last_leaf, P.tail, P.tail_row, P.n_rounds, P.xor_tree, P.rounds_pk);
    hipStream_t st = (hipStream_t)stream;
    const bool has_tail = L.tail != 0;
    if (L.wide) {
        WFParams W;
        memset(&W, 0, sizeof W);
        W.f = P;
        fill_wide(L, W.w);
        // (n_sites > 0: the initial assignments with one wavefront per site; 0: llda_foldin_wide_kernel draws them itself)
        int rl = allow_lds(llda_foldin_init_wide_kernel, (size_t)L.KP * 8);
        if (rl) return rl;
        if (P.n_sites > 0)
            hipLaunchKernelGGL(llda_foldin_init_wide_kernel, dim3(wide_blocks(P.n_sites)), dim3(64), (size_t)L.KP * 8, st, W);
        rl = allow_lds(llda_foldin_wide_kernel, (size_t)L.KP * 12);
        if (rl) return rl;
        hipLaunchKernelGGL(llda_foldin_wide_kernel, dim3(wide_blocks(P.D)), dim3(64), (size_t)L.KP * 12, st, W);
        return launched();
    }
    return visit_layout(L.G, L.T, [&](auto g, auto t) { return launch_foldin<g.value, t.value>(P, has_tail, st); });
}

int llda_selftest_div(uint64_t seed, int64_t n, unsigned long long *mismatches_dev, void *stream)
{
    if (!mismatches_dev || n < 1) return LLDA_E_BAD_ARG;
    const int iters = 1024;
    int64_t threads = (n + iters - 1) / iters;
    int64_t blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    hipLaunchKernelGGL(llda_selftest_div_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       seed, iters, mismatches_dev);
    return launched();
}

}  // extern "C"
