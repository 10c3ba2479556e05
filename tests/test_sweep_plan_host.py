"""csrc/sweep_plan.hpp decides what llda_sweep launches: kernel family, template choices, margins, grid, block, dynamic LDS.  The parity
tests select kernel forms through llda_sweep_args.debug_margin and can only see the resulting state, which is the same whichever kernel
ran: a hook value that fell through to the production kernel would leave them green.  Here the header is compiled with the host compiler
around a driver that prints the plan (no HIP call, no pointer dereferenced, nothing launched) over debug_margin -20 .. 20, every kind of
layout and the argument combinations that select each family, and compared with the table of include/llda_gibbs.h / sweep_plan.hpp
written out again below in Python."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import layoutclasses
from conftest import ROOT

OK, BAD_K, BAD_ARG = 0, -1, -2
FAMILIES = ("none", "exact", "tiered", "rows16", "quad", "sparse", "wide_sparse", "wide_f32", "wide_reg", "wide_lds")
NEW_TIER_KS = tuple(layoutclasses.new_tier_ks())                  # the smallest K of five, six and seven tiers
KS = (8, 100, 128, 256, 392, 512, 1024, 1031, 2048, 3000, 7688) + NEW_TIER_KS
DMS = tuple(range(-20, 21))
MARGIN0, MARGIN0_WIDE, MARGIN0_QUAD = 2.0 ** -17, 112 * 2.0 ** -24, 104 * 2.0 ** -24      # the production build's
f32 = lambda x: float(np.float32(x))

DRIVER = r"""
#include "build_info.hpp"
#include "sweep_plan.hpp"
#include <stdio.h>
#include <string.h>
static void *ptr(long long v) { return reinterpret_cast<void *>(static_cast<uintptr_t>(v)); }
int main()
{
    llda_layout *L = new llda_layout;
    llda_sweep_args a;
    long long dm, n_kw, delta, csc, log, rec, kw16, srow, row16, img, live, scr, hooks_out;
    for (;;) {
        memset(L, 0, sizeof *L);
        memset(&a, 0, sizeof a);
        if (scanf("%d %d %d %d %d %d %d %d", &L->K, &L->n_leaves, &L->G, &L->T, &L->KP, &L->tail, &L->wide, &L->tiers) != 8) break;
        if (scanf("%lld %ld %ld %ld %d %d %lf %lf", &dm, &a.D, &a.V, &a.n_sites, &a.docs_per_group, &a.dense_mask, &a.alpha, &a.beta) != 8) return 2;
        if (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %d %lld %d %lld %ld %d %lld", &n_kw, &delta, &csc, &log, &rec, &kw16, &srow, &row16,
                  &img, &a.img_bits, &live, &a.live_max, &scr, &a.scratch_bytes, &a.max_doc_tokens, &hooks_out) != 16) return 2;
        a.K = L->K; a.debug_margin = (int32_t)dm;
        a.doc_off = (const int64_t *)ptr(64); a.word = a.freq = (const int32_t *)ptr(64); a.z = a.n_dk = (int32_t *)ptr(64);
        a.lab_mask = (const uint16_t *)ptr(64); a.n_k = (const int32_t *)ptr(64); a.n_k_delta = (int32_t *)ptr(64);
        a.n_kw = (const int32_t *)ptr(n_kw); a.n_kw_delta = (int32_t *)ptr(delta); a.csc_pos = (const int32_t *)ptr(csc);
        a.commit_log = (uint32_t *)ptr(log); a.site_rec = (const int32_t *)ptr(rec); a.n_kw16 = (const uint16_t *)ptr(kw16);
        a.site_row = (const int32_t *)ptr(srow); a.row16 = (const uint8_t *)ptr(row16); a.n_kw_img = ptr(img);
        a.live_off = (const int64_t *)ptr(live); a.live_pos = (const int32_t *)ptr(live); a.scratch = ptr(scr);
        SweepPlan p;
        const int rc = sweep_plan(a, *L, hooks_out != 0, &p);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %a %a %a %a %d %d %u %u %zu %a\n", rc, (int)p.family, p.has_tail, p.dense,
               p.logged, p.rec, p.w4, p.gs, p.img, p.nt, p.tc, p.slim, p.compact, p.tiered, p.lb, p.pad, p.hooks, p.margin_rel,
               (double)p.margin0_rel, (double)p.margin0_data, (double)p.m0, p.site_rec, p.dpg, p.grid, p.block, p.lds,
               batch_margin_rel(a.debug_margin));
    }
    return 0;
}
"""

FIELDS = ("rc", "family", "has_tail", "dense", "logged", "rec", "w4", "gs", "img", "nt", "tc", "slim", "compact", "tiered", "lb", "pad",
          "hooks", "margin_rel", "margin0_rel", "margin0_data", "m0", "site_rec", "dpg", "grid", "block", "lds", "batch_margin")


def layout(K):
    from lda_thesis_amd.layout import GroupLayout
    g = GroupLayout(K)
    return dict(K=K, n_leaves=g.m, G=g.G, T=g.T, KP=g.KP, tail=g.tail, wide=int(g.wide), tiers=g.NT if g.wide else 0)


def args(**kw):
    """llda_sweep_args of a valid all-exact-capable call: pointers are numbers (0 = NULL), nothing reads through them"""
    a = dict(dm=0, D=1000, V=5000, n_sites=50000, docs_per_group=0, dense_mask=0, alpha=0.1, beta=0.01, n_kw=4096, n_kw_delta=4096,
             csc_pos=0, commit_log=0, site_rec=0, n_kw16=0, site_row=0, row16=0, n_kw_img=0, img_bits=0, live=0, live_max=0, scratch=0,
             scratch_bytes=0, max_doc_tokens=0, hooks_out=1)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return a


@pytest.fixture(scope="module")
def run_plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("sweep_plan")
    src, exe = d / "driver.cpp", str(d / "driver")
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", exe, str(src), "-I", os.path.join(ROOT, "lda_thesis_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include")])

    def run(cases):
        """cases: (layout dict, args dict) -> one dict of FIELDS per case"""
        lines = []
        for L, a in cases:
            lines.append(" ".join(str(x) for x in (
                L["K"], L["n_leaves"], L["G"], L["T"], L["KP"], L["tail"], L["wide"], L["tiers"],
                a["dm"], a["D"], a["V"], a["n_sites"], a["docs_per_group"], a["dense_mask"], repr(a["alpha"]), repr(a["beta"]),
                a["n_kw"], a["n_kw_delta"], a["csc_pos"], a["commit_log"], a["site_rec"], a["n_kw16"], a["site_row"], a["row16"],
                a["n_kw_img"], a["img_bits"], a["live"], a["live_max"], a["scratch"], a["scratch_bytes"], a["max_doc_tokens"],
                a["hooks_out"])))
        out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
        rows = out.splitlines()
        assert len(rows) == len(cases)
        res = []
        for r in rows:
            v = r.split()
            res.append({k: (float.fromhex(x) if k in ("margin_rel", "margin0_rel", "margin0_data", "m0", "batch_margin") else int(x))
                        for k, x in zip(FIELDS, v)})
        return res
    return run


# ---- the table, written out again (llda_gibbs.h: llda_sweep_args.debug_margin; sweep_plan.hpp) ----
def ceil_div(a, b):
    return -(-a // b)


def wide_blocks(n):
    return max(1, min(n, 256 * 16))


def quad_ok(L):
    return not L["wide"] and L["T"] == 16 and L["G"] in (8, 16, 32) and L["n_leaves"] * 8 == L["G"]


def sparse_image(a):
    """IMG of a sparse-label launch, or the refusal"""
    if not a["n_kw_img"] and not a["img_bits"]:
        return 0
    if not a["n_kw_img"] or a["img_bits"] not in (8, 16) or a["n_kw_img"] % (4 if a["img_bits"] == 8 else 8):
        return None
    return a["img_bits"]


def expect(L, a):
    """-> the refusal code, or the fields of the plan that the family defines (FIELDS the family does not use are not compared)"""
    dm, D, KP, G, T = a["dm"], a["D"], L["KP"], L["G"], L["T"]
    if D == 0:
        return dict(family="none")
    if not 0 <= a["n_sites"] < 2 ** 30 or bool(a["csc_pos"]) != bool(a["commit_log"]):
        return BAD_ARG
    logged = bool(a["commit_log"])
    if not a["n_kw"] or not (a["n_kw_delta"] or logged):
        return BAD_ARG
    rec = logged and bool(a["site_rec"])
    if rec and G <= 16 and a["n_sites"] >= 2 ** 28:
        return BAD_ARG
    fast = a["alpha"] >= 1e-6 and a["beta"] >= 1e-6 and a["V"] * a["beta"] < 2.0 ** 40
    dense = fast and a["dense_mask"] != 0 and L["K"] == KP
    live = fast and a["live"] and 1 <= a["live_max"] <= 64
    dpg = max(1, a["docs_per_group"])
    margin_rel = 2.0 ** -40 if dm == 0 or -8 <= dm <= -2 else 2.0 ** -dm if dm > 0 else 2.0
    margin0_rel = MARGIN0 if dm in (0, -8) else 2.0 ** -dm if 1 <= dm <= 15 else 2.0
    e = dict(margin_rel=margin_rel, margin0_rel=margin0_rel, margin0_data=0.0, dpg=dpg, block=256, lds=0, site_rec=int(rec))

    if live and (a["dense_mask"] == 0 if L["wide"] else not dense):               # sparse label sets
        gs = 8 if a["live_max"] <= 8 else 16 if a["live_max"] <= 16 else 32 if a["live_max"] <= 32 else 64
        grid = ceil_div(D, (256 // gs) * dpg)
        img = sparse_image(a)
        if grid > 2 ** 31 - 1 or img is None:
            return BAD_ARG
        e.update(family="wide_sparse" if L["wide"] else "sparse", gs=gs, img=img, grid=grid)
        if dm < 0:
            e.update(margin_rel=2.0, margin0_rel=2.0)
        if L["wide"]:
            e.update(site_rec=0, lds=KP * 8 + 16)
        return e
    if L["wide"]:                                                                  # dense or general mask
        if a["n_kw_img"] or a["img_bits"]:
            return BAD_ARG
        nt, tc = L["tiers"], T // 4
        compact = 0 < a["max_doc_tokens"] < 32768 and dm != -4
        e.update(site_rec=0, dpg=0, grid=wide_blocks(D), block=64, nt=nt)
        if fast and compact and (dm >= -1 or dm in (-6, -7)):
            if T % 4 or (nt, tc) not in ((2, 3), (2, 4), (3, 4), (4, 3), (4, 4), (5, 4), (6, 4), (7, 4), (8, 3), (8, 4)):
                return BAD_K
            slim = bool(a["scratch"]) and a["scratch_bytes"] >= wide_blocks(D) * KP * 8 and dm != -6 and (dm == -7 or nt in (3, 4))
            m0 = MARGIN0_WIDE if dm in (0, -6, -7) else 2.0 ** -dm if 1 <= dm <= 15 else 2.0
            e.update(family="wide_f32", tc=tc, slim=int(slim), m0=m0, lds=KP * (6 if slim else 10))
        elif fast and dm != -3:
            if not 2 <= nt <= 8:
                return BAD_K
            e.update(family="wide_reg", compact=int(compact), lds=KP * (10 if compact else 16))
        else:
            e.update(family="wide_lds", tiered=int(fast), lds=KP * 16)
        return e
    grid = ceil_div(D, (256 // G) * dpg)
    if grid > 2 ** 31 - 1 or a["n_kw_img"] or a["img_bits"]:
        return BAD_ARG
    e.update(grid=grid)
    if a["row16"]:                                                                 # quad
        if not a["n_kw16"] or a["site_row"] or not (fast and a["dense_mask"] != 0 and logged and quad_ok(L)) or D >= 2 ** 31:
            return BAD_ARG
        if not 0 < a["max_doc_tokens"] < 65536 or a["n_kw16"] % 16 or a["n_kw"] % 16 or a["V"] >= 2 ** 22:
            return BAD_ARG
        if G <= 16 and not rec:
            return BAD_ARG
        if a["n_sites"] < 1:
            return dict(family="none")
        if dm == 0:
            e.update(margin0_rel=0.0, margin0_data=1.0)
        elif dm == -9:
            e.update(margin0_rel=MARGIN0_QUAD, margin_rel=2.0 ** -40)
        elif -18 <= dm <= -10:
            e.update(margin0_rel=0.0, margin0_data=float(np.float32(1.0) / np.float32(1.05)) if dm == -10 else 2.0 ** (dm + 10), margin_rel=2.0 ** -40)
        qgrid = ceil_div(D, (2 * 128 // G) * dpg)
        if qgrid > 2 ** 31 - 1:
            return BAD_ARG
        e.update(family="quad", lb={32: 4, 16: 3, 8: 2}[G], rec=int(G <= 16), pad=int(L["K"] != KP), hooks=int(dm != 0 or not a["hooks_out"]),
                 grid=qgrid, block=128)
        return e
    if bool(a["n_kw16"]) != bool(a["site_row"]):
        return BAD_ARG
    if a["n_kw16"]:                                                                # two-document 16-bit rows
        if not (fast and dense and logged and T == 16 and G >= 32) or a["n_kw16"] % 16 or a["n_kw"] % 16:
            return BAD_ARG
        e.update(family="rows16", w4=int(0 < a["max_doc_tokens"] < 65536 and dm != -8))
        return e
    has_tail = L["tail"] != 0
    if G <= 16 and fast and rec:
        e.update(family="tiered", rec=1, logged=1, dense=int(dense), has_tail=int(has_tail and not dense))
    elif not fast:
        e.update(family="exact", has_tail=int(has_tail))
    else:
        e.update(family="tiered", rec=0, logged=int(logged), dense=int(dense), has_tail=int(has_tail and not dense))
    return e


def check(cases, got):
    base = args()
    for (L, a), g in zip(cases, got):
        e = expect(L, a)
        if not isinstance(e, dict):
            e = dict(rc=e)
        else:
            e = dict(e, rc=OK, family=FAMILIES.index(e["family"]))
            for k in ("margin0_rel", "margin0_data", "m0"):
                if k in e:
                    e[k] = f32(e[k])                        # (the plan holds them as float)
        bad = {k: (g[k], v) for k, v in e.items() if g[k] != v}
        assert not bad, "K=%d tiers=%d %r: (plan, table) %r" % (L["K"], L["tiers"], {k: v for k, v in a.items() if v != base[k]}, bad)


def scenarios():
    P = 4096                                             # an aligned, non-NULL pointer
    log_kinds = (dict(), dict(csc_pos=P, commit_log=P), dict(csc_pos=P, commit_log=P, site_rec=P))
    row_kinds = (dict(), dict(n_kw16=P, site_row=P), dict(n_kw16=P, row16=P))
    prior_kinds = (dict(), dict(alpha=1e-7), dict(beta=1e-7))
    tokens = (0, 32767, 32768, 65535, 65536)
    out = []
    # the narrow general families: mask x commit log / site records x 16-bit rows x priors, and the token bounds of the row kernels
    for mask, lg, rows, pri in itertools.product((0, 1), log_kinds, row_kinds, prior_kinds[:2]):
        out.append(dict(dense_mask=mask, max_doc_tokens=65535, **lg, **rows, **pri))
    for rows, mdt in itertools.product(row_kinds[1:], tokens):
        out.append(dict(dense_mask=1, max_doc_tokens=mdt, **log_kinds[2], **rows))
    # sparse label sets: lanes x image x mask x log, and tiny priors (which switch them off)
    for lm, bits, mask, lg in itertools.product((8, 64), (0, 8, 16), (0, 1), log_kinds[::2]):
        out.append(dict(live=P, live_max=lm, img_bits=bits, n_kw_img=P if bits else 0, dense_mask=mask, max_doc_tokens=100, **lg))
    out.append(dict(live=P, live_max=8, beta=1e-7))
    out.append(dict(live=P, live_max=8, beta=1e-7, dense_mask=1))
    # the wide kernels: scratch absent / too small / there x token bound x mask x priors
    # (1000 documents: llda_sweep_scratch_bytes is 1000 * KP * 8, between 8 192 000 and 65 536 000 on the wide layouts)
    for scr, mdt, mask, pri in itertools.product((0, 2), tokens, (0, 1), prior_kinds[:2]):
        out.append(dict(scratch=P if scr else 0, scratch_bytes=(0, 0, 1 << 30)[scr], max_doc_tokens=mdt, dense_mask=mask, **pri))
    out.append(dict(scratch=P, scratch_bytes=8000 * 8 - 1, max_doc_tokens=32767))
    out.append(dict(scratch=0, scratch_bytes=1 << 30, max_doc_tokens=32767))
    out.append(dict(n_kw_img=P, img_bits=8))                                        # the image without the live lists
    out.append(dict(n_kw_img=P, img_bits=8, n_kw16=P, row16=P, dense_mask=1, csc_pos=P, commit_log=P, site_rec=P, max_doc_tokens=100))
    out.append(dict(docs_per_group=3, dense_mask=1, csc_pos=P, commit_log=P, site_rec=P, n_kw16=P, row16=P, max_doc_tokens=100))
    out.append(dict(docs_per_group=3, live=P, live_max=20))
    return out


def test_plan_over_the_grid(run_plans):
    """family, template choices, the three margins, grid, block and LDS for debug_margin -20 .. 20 x every kind of layout x the
    argument combinations that select each family"""
    lay = {K: layout(K) for K in KS}
    assert {L["G"] for L in lay.values() if not L["wide"]} == {8, 16, 32, 64}
    tiers = {L["tiers"] for L in lay.values() if L["wide"]}
    assert {2, 8} <= tiers and tiers & {3, 4} and {5, 6, 7} <= tiers
    cases = [(lay[K], args(dm=dm, **s)) for s in scenarios() for K in KS for dm in DMS]
    got = run_plans(cases)
    check(cases, got)
    assert {FAMILIES[g["family"]] for g in got if g["rc"] == OK} == set(FAMILIES) - {"none"}      # every family was reached
    for (L, a), g in zip(cases, got):                                               # llda_sweep_batch's one margin
        assert g["batch_margin"] == (2.0 ** -40 if a["dm"] == 0 else 2.0 ** -a["dm"] if a["dm"] > 0 else 2.0)


def test_every_kernel_hook_selects_its_own_plan(run_plans):
    """-3 ... -10 each differ from 0 in the plan, on the inputs of the parity tests that use them"""
    P = 4096
    wide = dict(max_doc_tokens=32767, dense_mask=1, scratch=P, scratch_bytes=1 << 30)
    quad = dict(dense_mask=1, csc_pos=P, commit_log=P, site_rec=P, n_kw16=P, row16=P, max_doc_tokens=65535)
    rows = dict(dense_mask=1, csc_pos=P, commit_log=P, n_kw16=P, site_row=P, max_doc_tokens=65535)
    L2, L3, L512 = layout(2048), layout(3000), layout(512)
    assert L2["tiers"] == 2 and L3["tiers"] in (3, 4)
    picks = [(L3, wide, -3), (L3, wide, -4), (L3, wide, -5), (L3, wide, -6), (L2, wide, -7), (L512, rows, -8), (L512, quad, -9),
             (L512, quad, -10)]
    cases = [(L, args(dm=d, **s)) for L, s, dm in picks for d in (0, dm)]
    got = run_plans(cases)
    check(cases, got)
    for i, (L, s, dm) in enumerate(picks):
        prod, hook = got[2 * i], got[2 * i + 1]
        assert prod["rc"] == hook["rc"] == OK
        assert prod != hook, dm
    fam = [FAMILIES[got[2 * i + 1]["family"]] for i in range(len(picks))]
    assert fam == ["wide_lds", "wide_reg", "wide_reg", "wide_f32", "wide_f32", "rows16", "quad", "quad"]
    assert FAMILIES[got[0]["family"]] == "wide_f32" and got[0]["slim"] == 1 and got[7]["slim"] == 0 and got[8]["slim"] == 0 and got[9]["slim"] == 1
    assert (got[3]["compact"], got[5]["compact"]) == (0, 1) and (got[10]["w4"], got[11]["w4"]) == (1, 0)
    # QUAD_HOOKS_OUT: production runs the instantiation without the hooks only when the build compiled them out
    q = run_plans([(L512, args(dm=0, hooks_out=h, **quad)) for h in (1, 0)])
    assert [g["hooks"] for g in q] == [0, 1]


def test_five_six_and_seven_tiers_take_every_wide_form(run_plans):
    """the widths whose dynamic LDS crosses the 64 KB opt-in at new sizes: every debug_margin, with and without scratch, a corpus
    with and without a document of 2^15 tokens, tiny priors; slim only where -7 forces it"""
    P = 4096
    lays = [layout(K) for K in NEW_TIER_KS]
    assert [(L["tiers"], L["T"], L["KP"]) for L in lays] == [(5, 16, 5120), (6, 16, 6144), (7, 16, 7168)]
    kinds = dict(light=dict(max_doc_tokens=32767, scratch=P, scratch_bytes=1 << 30), no_scratch=dict(max_doc_tokens=32767),
                 heavy=dict(max_doc_tokens=32768, scratch=P, scratch_bytes=1 << 30), unknown=dict(scratch=P, scratch_bytes=1 << 30),
                 tiny=dict(max_doc_tokens=32767, scratch=P, scratch_bytes=1 << 30, alpha=1e-9, beta=1e-9))
    cases = [(L, args(dm=dm, dense_mask=mask, **kw)) for L in lays for kw in kinds.values() for mask in (0, 1) for dm in DMS]
    got = run_plans(cases)
    check(cases, got)
    fat, full = {5: 51200, 6: 61440, 7: 71680}, {5: 81920, 6: 98304, 7: 114688}
    seen = set()
    for (L, a), g in zip(cases, got):
        assert g["rc"] == OK and g["nt"] == L["tiers"] and g["block"] == 64, (L["K"], a["dm"])
        fam, dm, nt = FAMILIES[g["family"]], a["dm"], L["tiers"]
        light = a["max_doc_tokens"] == 32767
        if a["alpha"] < 1e-6:
            assert (fam, g["tiered"], g["lds"]) == ("wide_lds", 0, full[nt])
        elif dm == -3:
            assert (fam, g["tiered"], g["lds"]) == ("wide_lds", 1, full[nt])
        elif light and (dm >= -1 or dm in (-6, -7)):
            slim = dm == -7 and bool(a["scratch"])
            assert (fam, g["tc"], g["slim"]) == ("wide_f32", 4, int(slim)) and g["lds"] == (L["KP"] * 6 if slim else fat[nt])
        else:
            compact = light and dm != -4
            assert (fam, g["compact"]) == ("wide_reg", int(compact)) and g["lds"] == (fat[nt] if compact else full[nt])
        seen.add((nt, fam, g["slim"] if fam == "wide_f32" else g["compact"] if fam == "wide_reg" else g["tiered"]))
    assert seen == {(nt, fam, v) for nt in (5, 6, 7) for fam in ("wide_f32", "wide_reg", "wide_lds") for v in (0, 1)}


def test_refusals(run_plans):
    P = 4096
    L8, L256, L512, L1031, L2048 = (layout(K) for K in (8, 256, 512, 1031, 2048))
    log = dict(csc_pos=P, commit_log=P)
    quad = dict(dense_mask=1, site_rec=P, n_kw16=P, row16=P, max_doc_tokens=100, **log)
    rows = dict(dense_mask=1, n_kw16=P, site_row=P, max_doc_tokens=100, **log)
    live = dict(live=P, live_max=8)
    fake = lambda nt, t: dict(L2048, tiers=nt, G=64 * nt, T=t, KP=64 * nt * t)       # a wide layout llda_layout_init never makes
    bad_arg = [
        (L8, args(n_sites=-1)), (L8, args(n_sites=2 ** 30)), (L8, args(csc_pos=P)), (L8, args(commit_log=P)), (L8, args(n_kw=0)),
        (L8, args(n_kw_delta=0)), (L8, args(n_sites=2 ** 28, site_rec=P, **log)), (L256, args(n_sites=2 ** 28, site_rec=P, **log)),
        (L8, args(D=2 ** 40)), (L8, args(D=2 ** 40, **live)), (L2048, args(D=2 ** 40, **live)),
        (L8, args(n_kw_img=P, img_bits=0, **live)), (L8, args(n_kw_img=0, img_bits=8, **live)), (L8, args(n_kw_img=P, img_bits=4, **live)),
        (L8, args(n_kw_img=P + 2, img_bits=8, **live)), (L8, args(n_kw_img=P + 4, img_bits=16, **live)),
        (L2048, args(n_kw_img=P + 4, img_bits=16, **live)), (L2048, args(n_kw_img=P, img_bits=8)), (L512, args(n_kw_img=P, img_bits=8)),
        (L512, args(**dict(quad, n_kw16=0))), (L512, args(**dict(quad, site_row=P))), (L512, args(**dict(quad, alpha=1e-7))),
        (L512, args(**dict(quad, dense_mask=0))), (L512, args(**dict(quad, csc_pos=0, commit_log=0))),
        (layout(250), args(**quad)), (L512, args(D=2 ** 31, **quad)), (L512, args(**dict(quad, max_doc_tokens=0))),
        (L512, args(**dict(quad, max_doc_tokens=65536))), (L512, args(**dict(quad, n_kw16=P + 8))), (L512, args(**dict(quad, n_kw=P + 4))),
        (L512, args(V=2 ** 22, **quad)), (L256, args(**dict(quad, site_rec=0))),
        (L512, args(n_kw16=P)), (L512, args(site_row=P)), (L512, args(**dict(rows, dense_mask=0))), (L512, args(**dict(rows, alpha=1e-7))),
        (L512, args(**dict(rows, csc_pos=0, commit_log=0))), (L256, args(**rows)), (layout(384), args(**rows)),
        (L512, args(**dict(rows, n_kw16=P + 8))), (L512, args(**dict(rows, n_kw=P + 8))),
    ]
    bad_k = [(fake(3, 12), args(max_doc_tokens=100)), (fake(5, 12), args(max_doc_tokens=100)), (fake(2, 8), args(max_doc_tokens=100)),
             (fake(9, 16), args(max_doc_tokens=100)), (fake(9, 16), args()), (fake(1, 16), args()), (fake(9, 16), args(dm=-5))]
    none = [(L8, args(D=0, n_kw=0, n_kw_delta=0)), (L512, args(n_sites=0, **quad))]
    # (a wide layout outside the instantiated kernels that ALSO brings the narrow image: the argument is refused first)
    both = [(fake(9, 16), args(n_kw_img=P, img_bits=8))]
    fine = [(L256, args(n_sites=2 ** 28 - 1, site_rec=P, **log)), (L512, args(n_sites=2 ** 28, site_rec=P, **log)), (L512, args(**quad)),
            (L256, args(**quad)), (L512, args(**rows)), (L512, args(**dict(quad, site_rec=0))), (fake(9, 16), args(dm=-3)),
            (fake(9, 16), args(alpha=1e-7)), (L1031, args(**quad))]          # (a wide layout never looks at row16)
    cases = bad_arg + bad_k + none + both + fine
    got = run_plans(cases)
    check(cases, got)
    want = [BAD_ARG] * len(bad_arg) + [BAD_K] * len(bad_k) + [OK] * len(none) + [BAD_ARG] * len(both) + [OK] * len(fine)
    for (L, a), g, w in zip(cases, got, want):
        assert g["rc"] == w, (L["K"], L["tiers"], {k: v for k, v in a.items() if v != args()[k]})
    assert [FAMILIES[g["family"]] for g in got[len(bad_arg) + len(bad_k):][:2]] == ["none", "none"]


def test_the_hook_is_read_in_the_plan_header_only():
    """nothing else in csrc/ looks at debug_margin: llda_sweep_batch hands its own to sweep_plan.hpp's helper"""
    import re
    csrc = os.path.join(ROOT, "lda_thesis_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        text = open(os.path.join(csrc, name)).read()
        text = re.sub(r"//[^\n]*", "", text)
        uses = re.findall(r"debug_margin[^\n;]*", text)
        if name == "sweep_plan.hpp":
            assert uses
        elif name == "llda_gibbs.hip":
            assert uses == ["debug_margin)"], uses                                  # batch_margin_rel(a->debug_margin)
        else:
            assert not uses, (name, uses)
