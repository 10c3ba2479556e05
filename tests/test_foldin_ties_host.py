"""The planted fold-in inputs of tests/foldinties.py are what they claim to be, and they discriminate (host only).

The builder's own walk is foldinref.fold_in bit for bit; every planted class is present at every boundary kind; at the kernel's margin
of 2^-40 the modelled decided tier hands over every last-bit tie, decides every just-outside site and every random site, and decides
them as the reference does.  The same inputs catch a tier that is not careful enough: with margin 0 the model is wrong or without a
decision on 107 of the 216 last-bit ties of the "llda" cases below (K = 9: 17 of 48, 40: 26 of 48, 130: 13 of 24, 257: 7, 512: 6, 777: 11,
968: 9, 1031: 6, 2100: 12 of 16 each), with scores rounded to fp32 it gets just-outside sites wrong at every K.  With totals in the
subnormal range (the loadings times an exact power of two) the tier WITHOUT a floor on the total is sure and wrong (K = 9: 35 of 2055
sites at totals of 2^-1069 .. 2^-1062, K = 512: 61 of 504): u * total is rounded onto the subnormal grid, whose relative step is wider
than any band.  With the kernel's floor of 2^-960 it is never sure there.
"""
import numpy as np
import pytest

import foldinties as ft
from test_gpu_foldin_direct import reference

KS = [9, 40, 130, 257, 512, 777, 968, 1031, 2100]
SETTINGS = ["flat", "llda"]

pytestmark = []                                   # (host only: the gpu mark of test_gpu_foldin_direct is not inherited)


def _same(ref, walk):
    for k in ("z", "n_dk", "th", "raises"):
        np.testing.assert_array_equal(ref[k], walk[k], err_msg=k)


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("K", KS)
def test_planted_sites_are_what_the_builder_says(K, setting):
    c, w = ft.tie_case(K, setting)
    assert not w["raises"].any()
    _same(reference(c), w)
    assert c["iters"] == 3 and c["thinning"] == 1
    lens = np.diff(c["doc_off"])
    assert lens.min() >= 3 and lens.max() <= 12 and c["freq"].min() == 1 and c["freq"].max() == 4
    f = ft.facts(K, setting)
    n = f["n_planted"]
    assert n == len(c["plan"]) >= 24 and n % 4 == 0
    # a quarter of the planted sites per boundary kind; ties and just-outside sites of both sides at every kind
    for kind in ft.KINDS:
        assert sum(v for (k, _), v in f["count"].items() if k == kind) == n // 4
        for cls in ft.CLASSES:
            assert f["count"].get((kind, cls), 0) >= 1, (kind, cls)
    ties = [p for p in w["planted"] if p["cls"].startswith("tie")]
    assert sum(p["cls"] == "tie_upper" for p in ties) == sum(p["cls"] == "tie_lower" for p in ties)
    assert f["n_equal"] > 0 and f["n_equal_lower"] > 0          # q == t - X[g-1] exactly: the strict `>` alone decides the planted double
    assert f["max_tie_gap"] < 2.0 ** -48                        # (a tie of the reference, seen through <= 16 + 9 + 3 roundings of 2^-53 of the model)
    assert all(ft.OUT_LO <= g <= ft.OUT_HI for g in f["outside_gaps"])
    assert f["min_random_gap"] > 2.0 ** -30
    # the planted word occurs nowhere else; first, last and middle sites are all in use
    words, counts = np.unique(c["word"], return_counts=True)
    assert (counts[words >= ft.V_RANDOM] == 1).all() and (words >= ft.V_RANDOM).sum() == n
    where = {("first" if p["n"] == 0 else "last" if p["n"] == lens[p["doc"]] - 1 else "middle") for p in w["planted"]}
    assert where == {"first", "last", "middle"}


@pytest.mark.parametrize("K", KS)
def test_wavefronts_mix_planted_and_random_documents(K):
    c, _ = ft.tie_case(K, "llda")
    lay = ft.orc.layout(K)
    per_wave = max(64 // lay.G, 1)
    D = len(c["doc_off"]) - 1
    assert D % per_wave == 0 and D * min(lay.G, 64) >= 4 * 256            # several workgroups, every wavefront full
    site_of = {d: n for (d, n) in c["plan"]}
    for wave in range(D // per_wave):
        docs = range(wave * per_wave, (wave + 1) * per_wave)
        planted = [d for d in docs if d in site_of]
        if wave % 2:
            assert len(planted) == per_wave
        elif per_wave > 1:
            assert len(planted) == per_wave // 2 and len({site_of[d] for d in planted}) == 1
    if per_wave == 1:                                                     # (one document per wavefront: every other even one)
        assert [d in site_of for d in range(0, 8, 2)] == [True, False, True, False]


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("K", KS)
def test_model_verdicts(K, setting):
    _, w = ft.tie_case(K, setting)
    sites = w["sites"]
    at = lambda p: sites[p["index"]]
    ties = [at(p) for p in w["planted"] if p["cls"].startswith("tie")]
    outside = [at(p) for p in w["planted"] if not p["cls"].startswith("tie")]
    rand = [s for s in sites if not s["planted"]]
    for p in w["planted"]:
        assert at(p)["ref"] == p["topic"] and at(p)["sweep"] == 0 and at(p)["planted"]
    assert not any(s["sure"] for s in ties)
    assert all(s["sure"] and s["model"] == s["ref"] for s in outside)
    assert all(s["sure"] and s["model"] == s["ref"] for s in rand)
    # discrimination: no margin -> a quarter of the ties at least is not the reference's; fp32 scores -> just-outside sites go wrong
    bad0 = sum(not s["sure0"] or s["model0"] != s["ref"] for s in ties)
    assert 4 * bad0 >= len(ties), (bad0, len(ties))
    assert sum(s["sure32"] and s["model32"] != s["ref"] for s in outside) > 0


@pytest.mark.parametrize("K", [9, 130, 777, 1031])
def test_init_rows_are_planted(K):
    c, w = ft.init_case(K, "llda")
    assert not w["raises"].any()
    _same(reference(c), w)
    pl = w["planted"]
    assert len(pl) == ft.N_INIT_PLANTED
    assert {(p["kind"], p["row_kind"], p["upper"]) for p in pl} == {(k, r, u) for k in ft.KINDS for r in ft.ROW_KINDS for u in (False, True)}
    assert all(p["steps"] == 0 for p in pl if p["row_kind"] == "no_step") and all(p["steps"] == 1 for p in pl if p["row_kind"] == "one_step")
    assert all(p["steps"] > 400 for p in pl if p["row_kind"] == "jump")
    assert sum(p["equal"] for p in pl) > 0
    assert (np.sum(c["rows"], axis=1) > 0).all() and (c["rows"] >= 0).all() and c["rows"].max() <= 1.3


@pytest.mark.parametrize("K", [9, 512])
def test_subnormal_totals_need_the_floor(K):
    c = ft.scaled_case(K, "llda", "sub1066")
    free, kept = ft.scaled_walk(K, "llda", "sub1066", 0.0), ft.scaled_walk(K, "llda", "sub1066", ft.FLOOR)
    _same(reference(c), free)
    tot = np.array([s["total"] for s in free["sites"]])
    assert 0 < tot.max() < 2.0 ** -1056
    assert sum(s["sure"] and s["model"] != s["ref"] for s in free["sites"]) > 0
    assert not any(s["sure"] for s in kept["sites"])


@pytest.mark.parametrize("scale", sorted(ft.SCALES))
def test_scales_land_where_they_say(scale):
    K = 40
    w = ft.scaled_walk(K, "flat", scale, ft.FLOOR)
    tot = np.array([s["total"] for s in w["sites"]])
    e = ft.SCALES[scale]
    assert tot.min() > 0 and np.isfinite(tot).all()
    lg = np.log2(tot)
    if scale == "top":
        assert tot.min() > 1e300 and lg.max() < 1010 and not w["raises"].any()
    else:
        assert e - 6 < lg.min() and lg.max() < e + 8
    assert not any(s["sure"] and s["model"] != s["ref"] for s in w["sites"])
