"""The planted sweep states of tests/sweepties.py are what they claim to be, and they discriminate (host only).

Every planted tie is within 2^-46 of the total of its boundary in exact arithmetic (most within 2^-56), both signs; every just-outside
site is 2^-38 .. 2^-36 away, both signs; every other site at least 2^-14.5; the wavefronts mix planted and random documents as
the module says.  At the margin 2^-40 the modelled tier 1 hands over every tie and decides every other site as the C oracle does.  The
same sites catch a tier that is not careful enough.  Planted sites (of `ties` ties / `outside` just-outside sites) on which the wrong
model disagrees with the C oracle -- measurements; the tests ask for one each:
  (a) tier 1 at margin 0  (b) sequential sum for numpy's pairwise  (c) w * (1 / S) for w / S  (d) `>=` for `>`  (e) fp32 scores, outside

                    ties out     a   b   c   d   e     s                          ties out     a   b   c   d   e     s
  general    9 dense   48  48    13   4  12  11  28   4.7      general    9 masked  48  48     9   2   2  14  20   4.2
  general   40 dense   48  48    14   4   5  11  21   4.0      general   40 masked  48  48    16   8   9  13  26   4.4
  general  130 dense   48  48    16   9   6   5  24   3.3      general  130 masked  48  48    18  10   5   8  22   4.9
  general  257 dense   48  48    24  10   4  12  26   5.3      general  257 masked  48  48    15   6   2   6  20   4.9
  general  777 dense   48  48    21  13   4   3  24   4.3      general  777 masked  48  48    20   8   4   9  25   3.2
  general  968 dense   48  48    22  15   7   4  25   3.5      general  968 masked  48  48    13  16   5   4  26   3.9
  general 1024 dense   48  48    21   9   6   4  25   5.3      general 1024 masked  48  48    19  10   7   6  25   3.0
  general  512 dense   48  48    21  16   9   6  25   4.7      quad     512         49  48    16  11   4   4  27   3.7
  quad     256         49  48    18  15   6  12  25   3.9      quad     128         49  48    19  10   7  11  27   3.1
  quad     100         49  48    17   8   5   9  29   3.7      quad     400         49  48    16  13   5   4  21   4.2
  sparse    40 / 7     48  48    12   3   6  16  21   5.1      sparse   392 / 7     48  48    10   4   4  18  23   5.8
  sparse   512 / 7     48  48     8   5   5   8  17   5.9      sparse   512 / 20    48  48    12   4   2  10  22   3.9
  sparse   777 / 40    48  48    19   7   3   3  23   3.1      sparse  1031 / 7     48  48    15   4   9  15  26   3.5
  sparse  2048 / 7     48  48    17   3   7  13  21   4.5      wide    1031 masked  48  48    21  12   7  11  27   3.1
  wide    2048 dense   48  48    25  11   7   2  28   5.8      wide    3000 masked  48  48    20  16   8   5  24   2.7
  batched    5 (0)     48  48     9   0   4  18  31   4.3      batched   60 (1)     48  48    16   7   7   9  21   3.6
  batched  128 (2)     48  48    10   5   4  11  17   4.0      batched  100 (3)     48  48    14   5   4   9  24   3.2
  wide    4167 masked  48  48    14  14   5   4  21   8.2      wide    4295 masked  48  48    22  11   7   9  25  12.9
Sub-problems that share the wavefronts of one batched launch (sweepties.BATCH_MIXED: 64 documents each, lanes 8 and 16), with
  (f) the exact pipeline evaluated with the NEIGHBOURING group's K -- the sub-problem of the same KP -- at the site's own KP

                    ties out     a   b   c   d   e   f     s                        ties out     a   b   c   d   e   f     s
  mixed  100 (8)       24  24     7   3   3   3   9   1   4.7      mixed  128 (8)       24  24     6   2   3   6  14   2   4.8
  mixed   60 (8)       24  24     8   3   3   5   8   2   6.8      mixed   64 (8)       24  24     8   4   5   5  12   3   5.6
  mixed   96 (8)       24  24     5   2   2   5  15   -   3.6      mixed  100 (16)      24  24     4   5   4   7  13   1   3.8
  mixed  128 (16)      24  24     7   6   3   7  10   2   3.3
(96 has no neighbour of its KP.  (f) is a condition, not a measurement: with 6 .. 8 labels out of 100 few planted documents allow a
topic of the one row the two sums treat differently, and the streams of BATCH_MIXED were chosen so that every paired state has one.
Seconds on a machine on which batched 60 (1) took 8 s.)
(All seconds of this docstring are what the FIRST test that asks for a state pays: sweepties.state is an lru_cache, and only that sharing
keeps the other tests of a process cheap -- test_batched_wavefronts_from_their_order run on its own plants the four batched and the
seven mixed states itself, 36 s on that machine.)
(4167 and 4295: the largest K of five and of seven tiers, tests/layoutclasses.py tier_ks().  Their seconds are from a slower machine,
on which wide 3000 took 7.6 s: 1.1 and 1.7 times that state's.)
(s: seconds to generate the state on one core of the development machine; sweepties.state is cached, so the host and the GPU tests of a
process pay once.  numpy sums fewer than 8 terms sequentially: at K = 5 model (b) IS the pipeline and cannot be caught.  With fewer than
some 48 ties a state missed a model now and then -- see sweepties.N_DOCS.)
"""
import time

import numpy as np
import pytest

import sweepties as st
from neartie import _gap, _site_scores

CASES = [("general", a) for a in st.GENERAL] + [("quad", (K,)) for K in st.QUAD] + [("sparse", a[:2]) for a in st.SPARSE] + \
        [("wide", a) for a in st.WIDE] + [("batch", (i,)) for i in range(len(st.BATCH))] + [("mixed", (i,)) for i in range(len(st.MIXED_SUBS))]
MAKE = dict(general=st.general_state, quad=st.quad_state, sparse=st.sparse_state, wide=st.wide_state, batch=st.batch_state, mixed=st.mixed_state)
ids = ["%s-%s" % (f, "-".join(str(int(v)) for v in a)) for f, a in CASES]


def _lay(s):
    return st.orc.layout(s["n_d_k"].shape[1])


@pytest.mark.parametrize("family,args", CASES, ids=ids)
def test_planted_sites_are_what_the_generator_says(family, args):
    t0 = time.time()
    s = MAKE[family](*args)
    print("generated in %.1f s" % (time.time() - t0))
    lay, D = _lay(s), len(s["doc_off"]) - 1
    a, b, vb = s["alpha"], s["beta"], s["V"] * s["beta"]
    assert s["V"] == int(s["doc_off"][-1]) + s["extra_columns"] and (np.diff(s["doc_off"]) >= 1).all() and (np.diff(s["doc_off"]) <= 4).all()
    n_cls = np.zeros(4, dtype=int)
    for r in s["sites"]:
        d = r["doc"]
        last = r["n"] == s["doc_off"][d + 1] - s["doc_off"][d] - 1
        assert r["planted"] == bool(s["planted"][d] and last)
        if not r["planted"]:
            _, cum = _site_scores(lay, r["lab"], r["nd"], r["nk"], r["x"], a, b, vb)
            assert _gap(cum, r["u"] * cum[-1]) > 2.0 ** -14.5
            continue
        f = s["facts"][d]
        pos = st.positives(lay, r["lab"])
        assert st.kind_holds(lay, pos, f["b"], f["kind"]) and st.KINDS[s["kind"][d]] == f["kind"] and st.CLASSES[s["klass"][d]] == f["cls"]
        e = st.exact_signed_gap(lay, r["lab"], r["nd"], r["nk"], r["x"], r["u"], a, b, vb, f["b"])
        _, cum = _site_scores(lay, r["lab"], r["nd"], r["nk"], r["x"], a, b, vb)
        others = np.abs(cum[pos[:-1][pos[:-1] != f["b"]]] - r["u"] * cum[-1]) / cum[-1]
        assert not len(others) or others.min() > 2.0 ** -31              # the planted boundary is THE near one (doubles see that far)
        if f["cls"].startswith("tie"):
            assert 0 < abs(e) <= st.TIE_MAX and (e > 0) == (f["cls"] == "tie_upper")
        else:
            assert st.OUT_LO <= abs(e) <= st.OUT_HI and (e > 0) == (f["cls"] == "outside_plus")
        n_cls[s["klass"][d]] += 1
    assert n_cls.sum() == s["planted"].sum() == s["n_ties"] + s["n_outside"] and (n_cls >= max(1, D // 16)).all(), n_cls
    # every kind of boundary is there (a dense document has no zero lane; a wanted kind the labels or the uniform do not allow gives
    # way to another one: s["unplaced"])
    placed = np.bincount(s["kind"][s["kind"] >= 0], minlength=4)
    no_zero = bool(s["labs"][s["planted"]].all())                        # (dense, or K = 5: a planted document allows all five topics)
    assert (placed[[0, 1, 3]] >= max(1, D // 16)).all() and (placed[2] == 0 if no_zero else placed[2] >= max(1, D // 16)), placed
    # counts a kernel can hold; the quad states within the 16-bit image
    if family == "quad":
        assert int(s["n_k_v"].max()) <= 65535 and int(s["n_d_k"].sum(axis=1).max()) < 65536
    assert int(s["n_k_v"].min()) >= 0 and int(s["n_d_k"].min()) >= 0


@pytest.mark.parametrize("family,args", [c for c in CASES if c[0] != "batch"], ids=[i for i in ids if not i.startswith("batch")])
def test_wavefronts_mix_planted_and_random_documents(family, args):
    s = MAKE[family](*args)
    lay = _lay(s)
    per_wave = s["per_wave"]
    want = dict(general=max(64 // lay.G, 1), wide=1, quad=64 // (lay.G // 2), sparse=64 // st.sparse_lanes(args[-1]) if family == "sparse" else 0,
                mixed=64 // st.MIXED_SUBS[args[0]][1] if family == "mixed" else 0)[family]
    assert per_wave == want
    D = len(s["doc_off"]) - 1
    lens = np.diff(s["doc_off"])
    for wave in range(D // per_wave):
        docs = np.arange(wave * per_wave, (wave + 1) * per_wave)
        if wave % 2:
            assert s["planted"][docs].all()
        elif per_wave > 1:
            assert s["planted"][docs].sum() == per_wave // 2 and len(set(lens[docs])) == 1         # ONE site index
    if per_wave == 1:
        assert list(s["planted"][:8:2]) == [True, False, True, False]


def _waves(docs, per_wave):
    return [docs[i:i + per_wave] for i in range(0, len(docs), per_wave)]


def test_batched_wavefronts_from_their_order():
    """The wavefronts of the two batched families as their launches compose them -- from ``order``, not from the states' own numbering.
    batch: every sub-problem is its own lane class and Ensemble launches it longest document first (a stable sort), so a wavefront
    holds ONE problem; the sort leaves whole blocks of the states together only where lengths agree, and what remains is asserted:
    in every sub-problem of fewer than 64 lanes some wavefront holds planted and random documents of one length, and some holds
    planted documents only (measured: 11 and 2 of 16 wavefronts at K = 5, 25 and 6 of 32 at K = 60, 31 and 32 of 64 at K = 128).
    mixed (sweepties.mixed_order): EVERY wavefront holds min(P, 64 / lanes) >= 2 problems, no two neighbouring groups share one, it
    holds planted and random documents, and the planted and random documents of its first half have one length (ONE site index)."""
    for i, (K, _, hi) in enumerate(st.BATCH):
        s = st.batch_state(i)
        per_wave = 64 // st.sparse_lanes(hi - 1)
        assert per_wave == s["per_wave"]
        lens = np.diff(s["doc_off"])
        order = np.argsort(-lens, kind="stable")                         # Ensemble.orders: longest first inside a lane class
        both = only = 0
        for docs in _waves(order, per_wave):
            p = s["planted"][docs]
            both += bool(p.any() and not p.all() and len(set(lens[docs])) == 1)
            only += bool(p.all())
        if per_wave == 1:                                                # 64 lanes a document: a wavefront IS one document
            assert both == 0 and only == int(s["planted"].sum())
        else:
            assert both >= 1 and only >= 1, (i, both, only)
    for g, (lanes, D, subs) in enumerate(st.BATCH_MIXED):
        order = st.mixed_order(g)
        per_wave, P = 64 // lanes, len(subs)
        states = {i: st.mixed_state(i) for i in set(i for i, _ in order)}
        assert len(states) == P and len(order) == P * D and len(order) % per_wave == 0
        for wave in _waves(order, per_wave):
            probs = [i for i, _ in wave]
            assert len(set(probs)) == min(P, per_wave) >= 2 and all(a != b for a, b in zip(probs, probs[1:]))
            planted = np.array([states[i]["planted"][d] for i, d in wave])
            lens = np.array([np.diff(states[i]["doc_off"])[d] for i, d in wave])
            half = per_wave // 2
            assert planted[:half].sum() == half // 2 + half % 2 or planted[:half].sum() == half // 2, planted
            assert planted[:half].any() and not planted[:half].all() and len(set(lens[:half])) == 1
            assert planted[half:].all()


@pytest.mark.parametrize("family,args", CASES, ids=ids)
def test_model_verdicts_and_discrimination(c_oracle, family, args):
    s = MAKE[family](*args)
    cs = c_oracle.CState(s["doc_off"], s["word"], s["freq"], s["z"], s["labs"], s["n_d_k"], s["n_k_v"], s["n_zk"], s["V"], s["alpha"], s["beta"])
    cs.sweep(1, s["seed"], 0, stream=s["stream"], doc_base=s["doc_base"], threads=4)
    v = st.verdicts(s, quad=family == "quad")
    assert len(v) == len(cs.z)
    for i, r in enumerate(v):
        assert r["ref"] == cs.z[i], (i, r)                              # the numpy restatement of the exact pipeline IS the C oracle's
        if r["planted"] and r["cls"].startswith("tie"):
            assert not r["sure"]
        else:
            assert r["sure"] and r["model"] == cs.z[i], r
    if family == "quad":                                                 # int32 rows take the standard order out of line: the same verdicts
        for i, r in enumerate(st.verdicts(s, quad=False)):
            assert r["sure"] != bool(r["planted"] and r["cls"].startswith("tie")) and (not r["sure"] or r["model"] == cs.z[i])
    other = st.mixed_neighbour(args[0]) if family == "mixed" else None
    c = st.caught(s, quad=family == "quad", other_k=None if other is None else st.MIXED_SUBS[other][3])
    print(family, args, c)
    if other is not None:
        # (f) the exact pipeline with the NEIGHBOURING group's K at the site's own KP: a condition on the chosen pairings and streams,
        # not a measurement; the same statement with the state's own K is the pipeline on every planted site
        assert c["own"] == 0 and c["f"] >= 1, c
    assert c["ties"] == s["n_ties"] and c["outside"] == s["n_outside"]
    for model in "abcde":
        if model == "b" and _lay(s).K < 8:                               # numpy's sum of fewer than 8 terms is the sequential one
            assert c[model] == 0
            continue
        assert c[model] >= 1, (model, c)
