// sweep_plan.hpp -- what llda_sweep launches, decided ONCE: kernel family, template choices, margins, grid, block, dynamic LDS.
// Host only: no HIP header, no pointer is dereferenced.  llda_gibbs.hip includes it after build_info.hpp (which has to see the margin
// switches before anything defaults them) and launches what the plan names; tests/test_sweep_plan_host.py compiles it with the plain
// host compiler and checks the table below over a grid of arguments.  llda_sweep_args.debug_margin is read HERE and nowhere else.
//
// dm = debug_margin (the DM_* names below), fast = alpha >= 1e-6 && beta >= 1e-6 && V*beta < 2^40,
// dense = fast && dense_mask != 0 && K == KP, logged = csc_pos && commit_log.
//
// Base margins (every family starts from these)
//   margin_rel    2^-40 for dm == 0 and -8 <= dm <= -2;  2^-dm for dm > 0;  2.0 otherwise (dm == -1, dm <= -9)
//   margin0_rel   LLDA_MARGIN0 for dm in {0, -8};  2^-dm for 1 <= dm <= 15;  2.0 otherwise
//   margin0_data  0
// Sparse and wide sparse (fast, live_off, live_pos, 1 <= live_max <= 64, and dense_mask == 0 on wide layouts / !dense on narrow ones)
//   GS = 8 / 16 / 32 / 64 from live_max;  IMG in {0, 8, 16} from img_bits (n_kw_img present and aligned to 4 / 8 bytes, else BAD_ARG)
//   the wide form drops site_rec, its LDS is KP*8 + 16 bytes;  any dm < 0 sets both margins to 2.0
// Wide, dense or general mask (n_kw_img / img_bits: BAD_ARG)
//   compact = 0 < max_doc_tokens < 32768 && dm != -4
//   fp32-tiered <NT, TC, SLIM>  when fast && compact && (dm >= -1 || dm in {-6, -7})
//       m0 = LLDA_MARGIN0_WIDE for dm in {0, -6, -7};  2^-dm for 1 <= dm <= 15;  else 2.0
//       slim = scratch && scratch_bytes >= llda_sweep_scratch_bytes && dm != -6 && (dm == -7 || tiers in {3, 4})
//       LDS = KP*6 when slim, else KP*10;  (NT, TC) outside wide_f32_pair(): BAD_K
//   register <NT, COMPACT>      otherwise, when fast && dm != -3;  NT outside 2 .. 8: BAD_K;  LDS = KP*10 when compact, else KP*16
//   LDS-only <TIERED = fast>    otherwise;  LDS = KP*16
//   margin_rel is the base value in every case
// Quad (row16): BAD_ARG unless n_kw16 && !site_row, fast && dense_mask && logged && llda_quad_ok(K), D < 2^31, 0 < max_doc_tokens < 65536,
//   n_kw16 and n_kw 16-byte aligned, V < 2^22, n_sites < 2^30, site_rec when G <= 16 -- in this order;  n_sites < 1: OK, no launch
//       dm == 0           (margin0_rel, margin0_data) = (0, 1)
//       dm == -9          margin0_rel = LLDA_MARGIN0_QUAD, margin_rel = 2^-40
//       dm == -10         (0, 1 / 1.05f), margin_rel = 2^-40
//       dm == -11 .. -18  (0, 2^(dm + 10)), margin_rel = 2^-40
//       every other dm    base values
//   LB = 4 / 3 / 2 for G = 32 / 16 / 8;  REC = G <= 16;  PAD = K != KP;  HOOKS = dm != 0 || !quad_hooks_out
//   grid = ceil(D / ((2 * 128 / G) * dpg)), 128 threads
// Two-document 16-bit rows (n_kw16 and site_row, BAD_ARG when one comes without the other): BAD_ARG unless fast && dense && logged &&
//   T == 16 && G >= 32 and both images 16-byte aligned;  W4 = 0 < max_doc_tokens < 65536 && dm != -8
// General narrow, in this order
//   record kernels   G <= 16 && fast && logged && site_rec:  tiered <HAS_TAIL, DENSE, LOGGED, REC>
//   16-bit rows      (above)
//   all-exact        !fast:  <HAS_TAIL>
//   tiered           (DENSE | HAS_TAIL | neither) x LOGGED
// Narrow grids: ceil(D / ((256 / G) * dpg)) workgroups of 256 threads (sparse: G = GS), dpg = max(1, docs_per_group); more than
// 2^31 - 1 workgroups: BAD_ARG.  Wide grids: wide_blocks(D) workgroups of one wavefront.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "llda_gibbs.h"

// the tier-0 (fp32) decision margins relative to the total score, in units of 2^-24 next to the worst-case error bounds they cover
#ifndef LLDA_MARGIN0
#define LLDA_MARGIN0 0x1p-17f                      // narrow tiered kernels: 128 (bound 105)
#endif
#ifndef LLDA_MARGIN0_WIDE
#define LLDA_MARGIN0_WIDE (112.0f * 0x1p-24f)      // wide fp32-tiered kernel: 112 (bound 92, kernel_wide.hpp)
#endif
// quad kernel: 104 (bound 99.2, 101.2 with int32 counts >= 2^24) -- what the test hooks scale; production uses the sharper
// data-dependent form (kernel_quad.hpp)
constexpr float LLDA_MARGIN0_QUAD = 0x1.ap-18f;
#ifndef ABL_EXTRA_LDS_BYTES
#define ABL_EXTRA_LDS_BYTES 0      // occupancy ablation: dynamic LDS nobody uses (tools: -DABL_EXTRA_LDS_BYTES=20000 -> 2 workgroups per CU)
#endif

// llda_sweep_args.debug_margin: n > 0 is the margin 2^-n, 0 production, below 0 one of
enum : int32_t {
    DM_EXACT = -1,           // every site through the exact tier
    DM_NO_TIER0 = -2,        // no fp32 tier
    DM_WIDE_LDS_ONLY = -3,   // wide: the kernel that keeps nothing of the row in registers
    DM_WIDE_COPIES = -4,     // wide: LDS copies of the counts whatever max_doc_tokens says
    DM_WIDE_NO_F32 = -5,     // wide: the fp64 register kernel without its fp32 tier
    DM_WIDE_FAT = -6,        // wide: the fp32 tier with fp64 factors in LDS even when scratch is there
    DM_WIDE_SLIM = -7,       // wide: fp32 factors only whenever scratch is there
    DM_ROWS16_W3 = -8,       // two-document 16-bit rows: the three-wave form
    DM_QUAD_CONST = -9,      // quad: the constant tier-0 margin
    DM_QUAD_BOUND = -10,     // quad: the data-dependent margin scaled by 1 / 1.05 (the derived bound itself)
    DM_QUAD_SCALE_LAST = -18 // quad: -11 .. -18 scale it by 1/2 .. 1/256
};

enum SweepFamily {
    SWEEP_NONE,              // nothing to sample: no launch
    SWEEP_EXACT,             // llda_sweep_exact_kernel<G, T, HAS_TAIL>
    SWEEP_TIERED,            // llda_sweep_kernel<G, T, HAS_TAIL, DENSE, LOGGED, REC>
    SWEEP_ROWS16,            // llda_sweep_kernel<G, T, false, true, true, false, true, W4>
    SWEEP_QUAD,              // llda_sweep_quad_kernel<LB, REC, PAD, HOOKS>
    SWEEP_SPARSE,            // llda_sweep_sparse_kernel<GS, KParams, IMG>
    SWEEP_WIDE_SPARSE,       // llda_sweep_sparse_kernel<GS, WSParams, IMG>
    SWEEP_WIDE_F32,          // llda_sweep_wide_f32_kernel<NT, TC, SLIM>
    SWEEP_WIDE_REG,          // llda_sweep_wide_reg_kernel<NT, COMPACT>
    SWEEP_WIDE_LDS           // llda_sweep_wide_kernel<TIERED>
};

struct SweepPlan {
    SweepFamily family;
    bool has_tail, dense, logged, rec, w4;      // narrow general kernels (rec: the quad kernel too)
    int gs, img;                                // sparse: lanes per document, bits of the narrow image (0: none)
    int nt, tc;                                 // wide: tiers, slots per virtual lane / 4
    bool slim, compact, tiered;
    int lb;                                     // quad: log2 of the lanes per document
    bool pad, hooks;
    double margin_rel;                          // KParams.margin_rel
    float margin0_rel, margin0_data;            // KParams.margin0_rel, .margin0_data
    float m0;                                   // SWEEP_WIDE_F32: the kernel's tier-0 margin (it does not read KParams')
    bool site_rec;                              // KParams.site_rec is llda_sweep_args.site_rec (else NULL)
    int32_t dpg;                                // KParams.dpg
    unsigned grid, block;
    size_t lds;                                 // dynamic LDS bytes
};

constexpr int SWEEP_MAX_LIVE = 64;              // (LLDA_MAX_LIVE, device_common.hpp)
constexpr int SWEEP_QUAD_THREADS = 128;         // (QNT, kernel_quad.hpp)

// one wavefront per document (or site): enough workgroups to fill the chip a few times over
inline unsigned wide_blocks(int64_t n)
{
    const int64_t cap = 256 * 16;
    return (unsigned)(n < 1 ? 1 : (n < cap ? n : cap));
}

// the instantiations of llda_sweep_wide_f32_kernel
constexpr bool wide_f32_pair(int nt, int tc)
{
    return (tc == 4 && nt >= 2 && nt <= 8) || (tc == 3 && (nt == 2 || nt == 4 || nt == 8));
}

// true when one of the pointers has a bit of mask set
template <typename... T>
bool misaligned(uintptr_t mask, const T *...p)
{
    return ((reinterpret_cast<uintptr_t>(p) | ...) & mask) != 0;
}

// llda_quad_ok(K), from the layout
inline bool plan_quad_ok(const llda_layout &L)
{
    return !L.wide && L.T == 16 && (L.G == 8 || L.G == 16 || L.G == 32) && L.n_leaves * 8 == L.G;
}

// 2^-dm for 1 <= dm <= 15, else "tier 0 off"
inline float plan_hook_margin0(int32_t dm) { return dm > 0 && dm < 16 ? ldexpf(1.0f, -dm) : 2.0f; }

// llda_sweep_batch's one margin
inline double batch_margin_rel(int32_t dm) { return dm == 0 ? 0x1p-40 : (dm > 0 ? ldexp(1.0, -dm) : 2.0); }

// sparse-label kernels, narrow and wide: lanes per document, the "everything exact" hook, the narrow image, the grid
inline int plan_sparse(const llda_sweep_args &a, SweepPlan &p)
{
    p.gs = a.live_max <= 8 ? 8 : a.live_max <= 16 ? 16 : a.live_max <= 32 ? 32 : 64;
    if (a.debug_margin < 0) {       // every site through the exact pipeline (also with -8, which keeps the fp32 tier only for the 16-bit rows)
        p.margin_rel = 2.0;
        p.margin0_rel = 2.0f;
    }
    const int64_t per_block = (int64_t)(256 / p.gs) * p.dpg;
    const int64_t blocks = (a.D + per_block - 1) / per_block;
    if (blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
    p.grid = (unsigned)blocks;
    if (a.n_kw_img || a.img_bits) {
        if (!a.n_kw_img || (a.img_bits != 8 && a.img_bits != 16)) return LLDA_E_BAD_ARG;
        if (misaligned(a.img_bits == 8 ? 3 : 7, a.n_kw_img)) return LLDA_E_BAD_ARG;     // (as llda_pack_image)
        p.img = a.img_bits;
    }
    return LLDA_OK;
}

// The plan of llda_sweep(&a): LLDA_OK and *out, or the refusal.  a.D >= 0 and a.V >= 1 (llda_sweep checks them before it asks for the
// layout); L is llda_layout_init(a.K); quad_hooks_out: production (debug_margin == 0) runs the quad kernels' instantiation with the
// margin hooks compiled out (llda_sweep passes true).
inline int sweep_plan(const llda_sweep_args &a, const llda_layout &L, bool quad_hooks_out, SweepPlan *out)
{
    SweepPlan p = {};
    p.family = SWEEP_NONE;
    *out = p;
    if (a.D == 0) return LLDA_OK;                       // an empty shard: nothing to do, array pointers may be NULL
    if (a.n_sites < 0 || a.n_sites >= (1LL << 30)) return LLDA_E_BAD_ARG;   // split the shard (llda_gibbs.h)
    const bool logged = a.csc_pos && a.commit_log;
    if ((a.csc_pos != nullptr) != (a.commit_log != nullptr)) return LLDA_E_BAD_ARG;
    if (!a.doc_off || !a.word || !a.freq || !a.z || !a.lab_mask || !a.n_dk || !a.n_kw || (!a.n_kw_delta && !logged) || !a.n_k ||
        !a.n_k_delta)
        return LLDA_E_BAD_ARG;
    p.site_rec = logged && a.site_rec;
    if (p.site_rec && L.G <= 16 && a.n_sites >= (1LL << 28)) return LLDA_E_BAD_ARG;   // 16-byte records: 32-bit offsets
    // with alpha, beta >= 1e-6 and int32 counts no label-allowed score can underflow to zero ...
    // ... and with V*beta < 2^40 the fp32 / fp64 reciprocals of n_k + V*beta stay in range
    const bool fast = a.alpha >= 1e-6 && a.beta >= 1e-6 && (double)a.V * a.beta < 1099511627776.0;
    // all-ones label masks and no padded slots: the mask need not be applied at all
    const bool dense = fast && a.dense_mask != 0 && L.K == L.KP;
    const int32_t dm = a.debug_margin;
    p.margin_rel = dm == 0 || (dm <= DM_NO_TIER0 && dm >= DM_ROWS16_W3) ? 0x1p-40 : (dm > 0 ? ldexp(1.0, -dm) : 2.0);
    p.margin0_rel = dm == 0 || dm == DM_ROWS16_W3 ? (float)LLDA_MARGIN0 : plan_hook_margin0(dm);
    p.dpg = a.docs_per_group < 1 ? 1 : a.docs_per_group;
    p.block = 256;
    const bool live = fast && a.live_off && a.live_pos && a.live_max >= 1 && a.live_max <= SWEEP_MAX_LIVE;

    if (L.wide && live && a.dense_mask == 0) {
        // sparse label sets on a wide layout: one lane per allowed topic, the wide exact tier for undecided sites
        p.family = SWEEP_WIDE_SPARSE;
        p.site_rec = false;
        p.lds = (size_t)L.KP * 8 + 16;
        const int rc = plan_sparse(a, p);
        if (rc) return rc;
    } else if (L.wide) {                                // more than 8 pairwise leaves: the general path, one wavefront per document
        if (a.n_kw_img || a.img_bits) return LLDA_E_BAD_ARG;   // the narrow image belongs to the sparse-label kernels
        p.site_rec = false;
        p.dpg = 0;
        p.grid = wide_blocks(a.D);
        p.block = 64;
        p.nt = L.tiers;
        p.tc = L.T / 4;
        // counts as start values + int16 changes (no document may then hold 2^15 tokens): 10 instead of 16 bytes of LDS per position
        p.compact = a.max_doc_tokens > 0 && a.max_doc_tokens < 32768 && dm != DM_WIDE_COPIES;
        p.lds = (size_t)L.KP * (p.compact ? 10 : 16);   // (16: scores (f64) + n_dk + n_k (int32), per wavefront)
        if (fast && p.compact && (dm >= DM_EXACT || dm == DM_WIDE_FAT || dm == DM_WIDE_SLIM)) {
            // fp32 tier 0 in front of the fp64 decision (needs the int16 count changes): production
            p.family = SWEEP_WIDE_F32;
            p.m0 = dm == 0 || dm == DM_WIDE_FAT || dm == DM_WIDE_SLIM ? LLDA_MARGIN0_WIDE : plan_hook_margin0(dm);
            // fp32 factors only in LDS (6 bytes per position) when the caller brought the scratch rows of the rare tiers
            // (measured faster only for three and four tiers: see the note at the kernel; -7 forces it for tests and ablations)
            p.slim = a.scratch && a.scratch_bytes >= (int64_t)wide_blocks(a.D) * L.KP * 8 && dm != DM_WIDE_FAT &&
                     (dm == DM_WIDE_SLIM || L.tiers == 3 || L.tiers == 4);
            if (p.slim) p.lds = (size_t)L.KP * 6;
            if (L.T != 4 * p.tc || !wide_f32_pair(p.nt, p.tc)) return LLDA_E_BAD_K;
        } else if (fast && dm != DM_WIDE_LDS_ONLY) {    // the tiered kernel with the row in registers
            p.family = SWEEP_WIDE_REG;
            if (p.nt < 2 || p.nt > 8) return LLDA_E_BAD_K;
        } else {                                        // -3: the same decision on the LDS-only kernel; tiny priors: every site exact
            p.family = SWEEP_WIDE_LDS;
            p.tiered = fast;
            p.compact = false;
            p.lds = (size_t)L.KP * 16;
        }
    } else {
        // sparse label sets: one lane per allowed topic (a site the margin cannot decide is resolved inside the kernel by the exact
        // pipeline, exact_site_wave)
        const bool sparse = live && !dense;
        // one pass of documents per workgroup by default.  Workgroups of equal-length documents finish in lock step, so the tail of
        // the launch idles for up to one workgroup's run time: the shorter the workgroup the better (synth2: 3540 M sites/s at 1,
        // 3341 at 4, 3205 at 6 documents per lane group)
        const int64_t per_block = (int64_t)(256 / L.G) * p.dpg;
        const int64_t blocks = (a.D + per_block - 1) / per_block;
        if (!sparse && blocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
        p.grid = (unsigned)blocks;
        if (sparse) {
            p.family = SWEEP_SPARSE;
            const int rc = plan_sparse(a, p);
            if (rc) return rc;
        } else if (a.n_kw_img || a.img_bits) {
            return LLDA_E_BAD_ARG;                      // the narrow image belongs to the sparse-label kernels
        } else if (a.row16) {
            // four / eight / sixteen documents per wavefront (kernel_quad.hpp): K = 512 / 256 / 128 dense with the commit log, every
            // row in the 16-bit image, flags per word from llda_pack_rows16_all, documents below 2^16 tokens
            if (!a.n_kw16 || a.site_row) return LLDA_E_BAD_ARG;
            if (!(fast && a.dense_mask != 0 && logged && plan_quad_ok(L))) return LLDA_E_BAD_ARG;
            if (a.D >= (1LL << 31)) return LLDA_E_BAD_ARG;
            p.pad = L.K != L.KP;
            if (!(a.max_doc_tokens > 0 && a.max_doc_tokens < 65536)) return LLDA_E_BAD_ARG;
            if (misaligned(15, a.n_kw16, a.n_kw)) return LLDA_E_BAD_ARG;
            if (a.V >= (1LL << 22)) return LLDA_E_BAD_ARG;                  // (the image is addressed with 32-bit byte offsets)
            // (the commit log too: log position << 2 in 32 bits.  The general check above refuses such a call for the site arrays'
            // sake; this kernel's own reason stands here, with its other bounds, so that it survives a change of that one)
            if (a.n_sites >= (1LL << 30)) return LLDA_E_BAD_ARG;
            if (L.G <= 16 && !p.site_rec) return LLDA_E_BAD_ARG;            // (8 / 16 documents per wavefront read 16-byte site records)
            if (a.n_sites < 1) return LLDA_OK;                              // (documents without sites: nothing to sample)
            if (dm == 0) {                                                  // this kernel's own, data-dependent bound: kernel_quad.hpp
                p.margin0_rel = 0.0f;
                p.margin0_data = 1.0f;
            } else if (dm == DM_QUAD_CONST) {                               // the constant margin 104 * 2^-24 of the total
                p.margin0_rel = LLDA_MARGIN0_QUAD;
                p.margin_rel = 0x1p-40;
            } else if (dm <= DM_QUAD_BOUND && dm >= DM_QUAD_SCALE_LAST) {   // the data-dependent margin SCALED DOWN: how much of it
                p.margin0_rel = 0.0f;                                       // the worst site needs
                p.margin0_data = dm == DM_QUAD_BOUND ? 1.0f / 1.05f : ldexpf(1.0f, dm + 10);
                p.margin_rel = 0x1p-40;
            }
            const int64_t per_q = (int64_t)(2 * SWEEP_QUAD_THREADS / L.G) * p.dpg;   // (a document is G / 2 lanes)
            const int64_t qblocks = (a.D + per_q - 1) / per_q;
            if (qblocks > 0x7fffffffLL) return LLDA_E_BAD_ARG;
            // (K = 512 with the site records measured SLOWER: 5.19 vs 4.84 ms on 125 000 documents -- four documents per wavefront
            // are not bound by the address pipeline, and the records are 4 more bytes per site)
            p.family = SWEEP_QUAD;
            p.lb = L.G == 32 ? 4 : L.G == 16 ? 3 : 2;
            p.rec = L.G <= 16;
            // every dm != 0 runs the instantiation that reads the margins of both tiers from the arguments; production has them compiled in
            p.hooks = dm != 0 || !quad_hooks_out;
            p.grid = (unsigned)qblocks;
            p.block = SWEEP_QUAD_THREADS;
        } else {
            if ((a.n_kw16 != nullptr) != (a.site_row != nullptr)) return LLDA_E_BAD_ARG;
            p.dense = dense;
            p.has_tail = L.tail != 0 && !dense;
            p.logged = logged;
            if (a.n_kw16) {
                // 16-bit rows (bit 31 of csc_pos): the dense 16-slot kernel with the commit log, nothing else knows the flag
                if (!(fast && dense && logged && L.T == 16 && L.G >= 32)) return LLDA_E_BAD_ARG;
                if (misaligned(15, a.n_kw16, a.n_kw)) return LLDA_E_BAD_ARG;
                p.family = SWEEP_ROWS16;
                // four waves per SIMD: n_dk and its sweep-start value share an LDS word (-8: the three-wave form regardless)
                p.w4 = a.max_doc_tokens > 0 && a.max_doc_tokens < 65536 && dm != DM_ROWS16_W3;
                if (!p.w4) p.lds = ABL_EXTRA_LDS_BYTES;
            } else if (L.G <= 16 && fast && p.site_rec) {
                p.family = SWEEP_TIERED;
                p.rec = true;                           // 16-byte site records (llda_sweep_args.site_rec)
            } else if (!fast) {
                p.family = SWEEP_EXACT;
            } else {
                p.family = SWEEP_TIERED;
            }
        }
    }
    *out = p;
    return LLDA_OK;
}
