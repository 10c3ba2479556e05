"""lda_thesis_amd/sampler_plan.py decides which arrays GibbsSampler hands to the library: commit log or atomics, 16-bit rows in the
two-document or the quad form, narrow image of 8 / 16 / no bits, column order, scratch, site records, call limits, heavy documents.
The parity tests cannot see a wrong choice -- the state is bit-identical whichever kernel ran -- so the rules are written out again
below, as the sampler's documentation states them, and compared with the module over a grid of plain numbers: no device, no torch.
Facts that cost the sampler a device pass are zero-argument callables; the grid also checks that each is called exactly on the
paths that need it."""
import itertools
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from lda_thesis_amd import sampler_plan as P

KS = (8, 100, 128, 256, 392, 512, 1024, 1031, 2048)
MiB = 1 << 20
TRI = (None, True, False)
ENV_VARS = ("LLDA_ROWS16", "LLDA_QUAD", "LLDA_IMAGE")


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)


def layouts():
    """K -> (G, KP, wide, rows16_ok, quad_ok): the library's two answers derived from the layout, as plan_quad_ok in sweep_plan.hpp"""
    from lda_thesis_amd.layout import GroupLayout
    out = {}
    for K in KS:
        g = GroupLayout(K)
        narrow16 = not g.wide and g.T == 16
        out[K] = dict(K=K, G=g.G, KP=g.KP, wide=bool(g.wide), rows16_ok=narrow16 and g.G >= 32 and K == g.KP,
                      quad_ok=narrow16 and g.G in (8, 16, 32) and 8 * g.m == g.G)
    return out


class Lazy(object):
    """a fact the sampler measures on the device: counts how often the plan asked for it"""

    def __init__(self, value):
        self.value, self.calls = value, 0

    def __call__(self):
        self.calls += 1
        return self.value


QUAD_TRUE_TEXT = ("quad=True: needs a K with llda_quad_ok (16 slots per lane in 8, 16 or 32 lanes: K = 100, 128, 200, 256, 400, 512 ...), "
                  "documents of fewer than 65 536 tokens, a vocabulary below 2^22 words and fewer than 2^30 sites")
ROWS_TRUE_TEXT = "rows16=True: n_kw of %d x %d is too large for the 32-bit row offsets of the 16-bit-row kernel"
IMAGE_TEXT = "image must be None (automatic), 0 (off), 8 or 16"


# ---- the rules, written out again ----
def expect_rows(rows16, quad, S, V, KP, dense_mask, logged, r16ok, qok, alpha, beta, mdt, tokens, share, fits):
    """-> ((form, tolerate_oom, max_doc_tokens) or the ValueError text, the lazy facts that are looked at)"""
    keep, used = ("int32", False, mdt), set()
    if rows16 is False or not S or not dense_mask or not logged or alpha < 1e-6 or beta < 1e-6:
        return keep, used
    if not (r16ok or (quad is not False and qok)):
        return keep, used
    auto = rows16 is None
    if (V + 1) * (KP // 4) + V * (KP // 8) >= 2 ** 31:
        return (keep if auto else ROWS_TRUE_TEXT % (V, KP)), used
    used.add("tokens")
    four_waves = 0 < tokens < 65536
    if auto and not four_waves and V * KP * 4 < 64 * MiB:
        return keep, used
    as_quad = quad is not False and four_waves and qok and V < 2 ** 22 and S < 2 ** 30
    if as_quad and quad is None:
        used.add("share")
        as_quad = not share > 0.02 * S
    if quad is True and not as_quad:
        return QUAD_TRUE_TEXT, used
    if as_quad:
        return ("quad16", auto, tokens), used
    if not r16ok:
        return keep, used
    used.add("fits")
    if not fits:
        return keep, used
    return ("two_doc16", auto, mdt if mdt else tokens), used


def got_rows(rows16, quad, S, V, KP, dense_mask, logged, r16ok, qok, alpha, beta, mdt, tokens, share, fits):
    lazy = dict(tokens=Lazy(tokens), share=Lazy(share), fits=Lazy(fits))
    try:
        if not P.rows_possible(rows16, quad, S, dense_mask, logged, r16ok, qok, alpha, beta):
            res = ("int32", False, mdt)
        else:
            res = tuple(P.rows(rows16, quad, S, V, KP, r16ok, qok, mdt, lazy["tokens"], lazy["share"], lazy["fits"]))
    except ValueError as e:
        res = str(e)
    assert all(v.calls <= 1 for v in lazy.values())
    return res, {k for k, v in lazy.items() if v.calls}


def expect_image(image, S, V, KP, sparse, live_max, alpha, beta, r8, r16):
    if image not in (None, 0, 8, 16):
        return IMAGE_TEXT, False
    if image == 0 or not S or not sparse or alpha < 1e-6 or beta < 1e-6 or not V * beta < 2.0 ** 40 or live_max == 0:
        return 0, False
    if image is not None:
        return image, False
    if V * KP * 4 < 32 * MiB or S < 2 ** 20:
        return 0, False
    return (8 if r8 <= 0.5 else 16 if r16 <= 0.5 else 0), True


def test_rows_over_the_grid():
    """rows16 x quad x K x S around 2^20 / 2^30 / 2^31 x V around 2^22, the 64 MiB bar and the 32-bit row offsets x the longest
    document around 2^16 x the wide-row share around 2 % x "some row fits": form, tolerated allocation failure, max_doc_tokens,
    the two refusals, and which device passes were asked for"""
    lay = layouts()
    assert {K for K in KS if lay[K]["rows16_ok"]} == {512, 1024}
    assert {K for K in KS if lay[K]["quad_ok"]} == {100, 128, 256, 392, 512}
    sites = (0, 2 ** 20 - 1, 2 ** 20, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, 2 ** 31)
    seen, used_any, n = set(), set(), 0
    for K in KS:
        L = lay[K]
        bar = 64 * MiB // (4 * L["KP"])                      # V*KP*4 == 64 MiB
        for S, V, rows16, quad, tokens, over, fits, mdt in itertools.product(
                sites, (300, bar - 1, bar, 2 ** 22 - 1, 2 ** 22, 12000000), TRI, TRI, (0, 65535, 65536), (False, True), (True, False),
                (0, 40000)):
            share = 0.02 * S + (1.0 if over else 0.0)
            gates = ((1, 1, 0.1, 0.01),)
            if tokens == 65535 and fits and not over and not mdt:             # (the outer gate: crossed with the options and sizes only)
                gates += ((0, 1, 0.1, 0.01), (1, 0, 0.1, 0.01), (1, 1, 1e-7, 0.01), (1, 1, 0.1, 1e-7))
            for dense_mask, logged, alpha, beta in gates:
                a = (rows16, quad, S, V, L["KP"], dense_mask, logged, L["rows16_ok"], L["quad_ok"], alpha, beta, mdt, tokens, share, fits)
                want, got = expect_rows(*a), got_rows(*a)
                assert got == want, (K, a, got, want)
                seen.add(want[0] if isinstance(want[0], str) else want[0][:2])
                used_any |= want[1]
                n += 1
    assert n > 90000 and used_any == {"tokens", "share", "fits"}
    assert {s for s in seen if isinstance(s, tuple)} == {("int32", False), ("two_doc16", False), ("two_doc16", True), ("quad16", False),
                                                         ("quad16", True)}
    assert QUAD_TRUE_TEXT in seen and ROWS_TRUE_TEXT % (12000000, 512) in seen


def test_rows_of_the_five_policy_corpora():
    """tests/test_gpu_zz_policy.py as plain rows: K = 512, 8 000 x 300 sites, documents of 300 / 70 299 tokens, n_kw above / below 64 MiB
    -> (16-bit rows, quad, site_row, four waves)"""
    S = 8000 * 300
    for V, long_doc, want in ((1000000, False, True), (100000, False, True), (20000, False, True), (20000, True, False),
                              (100000, True, True)):
        assert (V * 512 * 4 >= 64 * MiB) == (V != 20000)
        tokens = 70299 if long_doc else 300
        assert P.rows_possible(None, None, S, True, True, True, True, 0.1, 0.01)
        r = P.rows(None, None, S, V, 512, True, True, 0, Lazy(tokens), Lazy(0.0), Lazy(True))
        assert (r.form != "int32") == want, (V, long_doc)
        assert (r.form == "quad16") == (want and not long_doc)
        assert (r.form == "two_doc16") == (want and long_doc)
        if want:
            assert (0 < r.max_doc_tokens < 65536) == (not long_doc)
            assert r.tolerate_oom


def test_the_three_refusals():
    with pytest.raises(ValueError) as e:
        P.rows(True, True, 1000, 300, 512, True, True, 0, Lazy(65536), Lazy(0.0), Lazy(True))
    assert str(e.value) == QUAD_TRUE_TEXT
    # (rows16=None with a small n_kw and a long document: no image at all, decided before the quad request is looked at)
    assert P.rows(None, True, 1000, 300, 512, True, True, 0, Lazy(65536), Lazy(0.0), Lazy(True)) == ("int32", False, 0)
    with pytest.raises(ValueError) as e:
        P.rows(True, None, 1000, 6000000, 1024, True, False, 0, Lazy(100), Lazy(0.0), Lazy(True))
    assert str(e.value) == ROWS_TRUE_TEXT % (6000000, 1024)
    assert P.rows(None, None, 1000, 6000000, 1024, True, False, 0, Lazy(100), Lazy(0.0), Lazy(True)) == ("int32", False, 0)
    for bad in (4, 32, "8", -1):
        with pytest.raises(ValueError) as e:
            P.image_bits(bad, 1000, 300, 512, True, 7, 0.1, 0.01, Lazy((0.0, 0.0)))
        assert str(e.value) == IMAGE_TEXT


def test_quad_handover():
    for S in (1000, 2 ** 20, 2 ** 30):
        for r16ok in (True, False):
            assert P.quad_handover(0.02 * S, S, r16ok) is None
            assert P.quad_handover(0.02 * S + 1, S, r16ok) == ("two_doc16" if r16ok else "int32")
            assert P.quad_handover(0.5 * S, S, r16ok, max_wide_sites=0.5) is None


def test_image_bits_over_the_grid():
    """image x S around 2^20 x n_kw around 32 MiB x escape rates around 0.5 x the gate: the bits, and the sample only where image=None
    gets as far as the rates"""
    lay = layouts()
    sampled = 0
    for K in KS:
        KP = lay[K]["KP"]
        bar = 32 * MiB // (4 * KP)
        for image, S, V, sparse, live_max, (alpha, beta), r8, r16 in itertools.product(
                (None, 0, 8, 16, 4), (0, 2 ** 20 - 1, 2 ** 20), (bar - 1, bar, 2 ** 22), (True, False), (0, 7, 64),
                ((0.1, 0.01), (1e-7, 0.01), (0.1, 1e-7), (0.1, 2.0 ** 40)), (0.5, 0.5000001), (0.5, 0.5000001)):
            rates = Lazy((r8, r16))
            want, lazy = expect_image(image, S, V, KP, sparse, live_max, alpha, beta, r8, r16)
            try:
                got = P.image_bits(image, S, V, KP, sparse, live_max, alpha, beta, rates)
            except ValueError as e:
                got = str(e)
            assert got == want and rates.calls == int(lazy), (K, image, S, V, sparse, live_max, alpha, beta, r8, r16, got, want)
            sampled += rates.calls
    assert sampled
    # the thresholds are arguments (GibbsSampler passes its class attributes, which tests patch)
    assert P.image_bits(None, 100, 300, 512, True, 7, 0.1, 0.01, Lazy((0.2, 0.0)), min_bytes=0, min_sites=0, max_escapes=0.1) == 16


def test_image_order():
    for K, KP in ((K, L["KP"]) for K, L in layouts().items()):
        for bits, force in itertools.product((8, 16), TRI):
            per_line = 128 if bits == 8 else 64
            assert P.image_cols_per_line(bits) == per_line
            assert P.image_order_possible(force, KP, bits) == (force is not False and KP > per_line)
    for force, (before, after) in itertools.product((None, True), ((10.0, 9.0), (10.0, 9.000001), (10.0, 5.0), (1.0, 1.0), (3.0, 4.0))):
        assert P.image_order_taken(force, before, after) == (force is True or after <= 0.9 * before)
    assert P.image_order_taken(None, 10.0, 9.0) and not P.image_order_taken(None, 10.0, 9.000001)


def test_commit_log_site_records_and_call_limit():
    lay = layouts()
    for K, wanted, S in itertools.product(KS, TRI, (0, 1, 2 ** 20 - 1, 2 ** 20, 2 ** 31 - 1, 2 ** 31)):
        G = lay[K]["G"]
        on = S > 0 and S < 2 ** 31 and (S >= 2 ** 20 if wanted is None else wanted)
        rec = on and G <= 16
        got = P.commit_log(wanted, S, G)
        assert got == (on, rec, 2 ** 28 - 1 if rec else 2 ** 30 - 1), (K, wanted, S)
        assert P.commit_log(wanted, S, G, 150, 1000).call_limit == 150                   # (the smaller bound, whichever it is)
        assert P.commit_log(wanted, S, G, 1000, 150).call_limit == (150 if rec else 1000)
    assert {lay[K]["G"] <= 16 for K in KS} == {True, False}


def test_heavy_documents_lane_classes_and_scratch():
    assert (P.HEAVY_TOPICS, P.HEAVY_K_PARTS) == (64, 4)
    for K, c in itertools.product(KS, (0, 1, 2, 3, 25, 26, 64, 65, 128, 129, 512, 513)):
        assert P.doc_is_heavy(c, K) == (c > 64 or c > K / 4.0), (K, c)
    for D, h in itertools.product((0, 1, 2, 7, 8), range(9)):
        if h <= D:
            assert P.shard_is_dense(h, D) == (h > D / 2.0)
    assert P.LANE_CLASSES == ((8, -1), (16, 8), (32, 16), (64, 32))
    for sparse, live_max, heavy in itertools.product((False, True), (0, 8, 9, 64), (0, 3)):
        assert P.one_launch(sparse, live_max, heavy) == (not sparse or (live_max <= 8 and heavy == 0))
    for wide, D, sparse, heavy in itertools.product((False, True), (0, 5), (False, True), (0, 3)):
        assert P.scratch(wide, D, sparse, heavy) is (wide and D > 0 and (not sparse or heavy > 0))


def test_environment_values_and_precedence(monkeypatch):
    """every value of the three variables, an invalid one for each, and: an explicit argument wins"""
    assert P.options(None, None, None) == (None, None, None)
    values = dict(LLDA_ROWS16=(("on", True), ("off", False)), LLDA_QUAD=(("on", True), ("off", False)),
                  LLDA_IMAGE=(("0", 0), ("8", 8), ("16", 16)))
    for i, var in enumerate(ENV_VARS):
        for text, value in values[var]:
            monkeypatch.setenv(var, text)
            want = [None, None, None]
            want[i] = value
            assert P.options(None, None, None) == tuple(want)
            for explicit in ((True, False) if i < 2 else (0, 8, 16)):
                args = [None, None, None]
                args[i] = explicit
                assert P.options(*args) == tuple(args), (var, text, explicit)
        allowed = ", ".join(t for t, _ in values[var])
        for bad in ("", "ON", "1", "yes", "4"):
            monkeypatch.setenv(var, bad)
            for args in ((None, None, None), (True, True, 8)):                       # (refused even where an argument would win)
                with pytest.raises(ValueError) as e:
                    P.options(*args)
                assert str(e.value) == "%s=%r: expected one of %s" % (var, bad, allowed)
        monkeypatch.delenv(var)
    monkeypatch.setenv("LLDA_ROWS16", "off")
    monkeypatch.setenv("LLDA_QUAD", "off")
    monkeypatch.setenv("LLDA_IMAGE", "16")
    assert P.options(None, None, None) == (False, False, 16)
    assert P.options(True, None, 0) == (True, False, 0)
    # a bad variable is reported in the order ROWS16, QUAD, IMAGE, and before a bad ``image`` argument (image_bits reports that)
    monkeypatch.setenv("LLDA_IMAGE", "3")
    monkeypatch.setenv("LLDA_QUAD", "maybe")
    with pytest.raises(ValueError, match="LLDA_QUAD='maybe'"):
        P.options(None, None, 5)


def test_the_environment_is_read_in_one_function_and_the_sampler_keeps_no_rule():
    import re
    plan_src = open(os.path.join(ROOT, "lda_thesis_amd", "sampler_plan.py")).read()
    assert len(re.findall(r"os\.environ|getenv", plan_src)) == 1
    src = open(os.path.join(ROOT, "lda_thesis_amd", "sampler.py")).read()
    assert not re.search(r"os\.environ|getenv|^import os|^from os", src, re.M)


def test_the_class_attributes_are_the_plan_defaults():
    from lda_thesis_amd.sampler import GibbsSampler as G
    want = dict(ROWS16_MIN_BYTES=64 << 20, QUAD_MAX_WIDE_SITES=0.02, QUAD_CHECK_EVERY=32, IMAGE_MIN_BYTES=32 << 20, IMAGE_MIN_SITES=1 << 20,
                IMAGE_MAX_ESCAPES=0.5, MAX_CALL_SITES=(1 << 30) - 1, MAX_CALL_SITES_REC=(1 << 28) - 1, LOG_ITEM=4096, PAIR_LIMIT=32767,
                MAX_FREQ=1 << 23)
    for name, value in want.items():
        assert getattr(G, name) == value == getattr(P, name), name
    assert P.SamplerPlan._fields == ("commit_log", "site_rec", "call_limit", "sparse", "heavy_docs", "scratch", "rows", "max_doc_tokens",
                                     "image_bits", "image_order")


def test_the_module_imports_neither_torch_nor_numpy():
    code = ("import sys; import lda_thesis_amd.sampler_plan; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('torch', 'numpy') or m.endswith('_native')]; print(bad); sys.exit(bool(bad))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
