"""llda_foldin called directly through lda_thesis_amd._native, as a binding written from include/llda_gibbs.h alone would call it, and
held against tests/foldinref.py (numpy, float64, the header's pseudo-code site by site; pinned to the oracle's run_test / cascade_test /
cascade_run_test in tests/test_foldin_ref_host.py).  Every comparison is exact: z, n_dk and th.

What lda_thesis_amd/foldin.py never passes and this file does: n_sites = 0 (the initial assignments drawn inside the per-document
launch, narrow and wide), doc_ids = NULL with a doc_base that wraps, status = NULL, empty documents, iters = 0, a thinning that does
not divide iters or exceeds it, c_loop so close to 1 or alpha so small that the host picks the exact pipeline itself, initial rows that
take both branches of the `while prob.sum() > 1: prob /= c` loop (no jump: sums of 1 + a few ulp and 1.03; the log jump of ~500 steps:
1.3), loadings over 40 orders of magnitude with half of them exact zeros.

One corpus shape per layout: document lengths 0 (first, middle, last), 1, 2, 2G and 2G + 1 (128 and 129 for G >= 64: a Philox block
serves 2G sites of a narrow document and 128 of a wide one, so it is regenerated inside those documents), frequencies 1..4.  The
matrices go to the device lane-major (layout.lm_topic_pos), z comes back as group-layout positions (layout.pos_topic); the outputs
sit between sentinel margins (countref.Guarded) and are pre-filled: th with NaN, z with a valid position, n_dk with zeros where the
contract asks for that (n_sites > 0) and with 0x3C3C3C3C where it is a pure output (n_sites = 0)."""
import functools

import numpy as np
import pytest

import foldinref
import layoutclasses
from countref import Guarded

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15                      # all 64 bits of the key in use
V = 60                                         # word V - 1 loads on no topic
STREAM = 0x80C0FFEE
C_INIT = 1.0005
GRID_KS = [1, 2, 8, 9, 16, 17, 33, 60, 96, 129, 257, 512, 777, 968, 969, 1031, 2100]      # 968: last narrow, 969: first wide
# five tiers with one leaf in the last (the smallest such K) and seven full tiers with a 7-topic tail (the largest): tests/layoutclasses.py
GRID_KS += [layoutclasses.tier_ks()[5][0], layoutclasses.tier_ks()[7][1]]
SINGLE_KS = [40, 512, 1031]
SETTINGS = {       # LabeledLDA.run_test; CascadeLDA's flat run_test with cascade_test's fall-back switched on
    "llda": dict(alpha=0.1, beta=0.0, c_loop=1.0000005, beta_fallback=False, avg_mode=0),
    "flat": dict(alpha=0.2, beta=0.01, c_loop=1.000005, beta_fallback=True, avg_mode=1),
}
FILL = 0x3C3C3C3C


def _layout(K):
    from lda_thesis_amd.layout import group_layout
    return group_layout(K)


def make_loadings(K, variant=0):
    """(K, V): wide dynamic range, half exact zeros, no all-zero topic, every word but V - 1 loads on some topic, V - 1 on none"""
    rng = np.random.default_rng([11, K, variant])
    ph = rng.random((K, V)) ** 12
    ph[rng.random((K, V)) < 0.5] = 0.0
    v = np.arange(V - 1)
    ph[(v + variant) % K, v] += rng.random(V - 1) ** 12 + 1e-30
    k = np.arange(K)
    ph[k, (k + variant) % (V - 1)] += 1e-25
    ph[:, V - 1] = 0.0
    assert (ph[:, :V - 1] > 0).any(axis=0).all() and (ph > 0).any(axis=1).all()
    assert K < 8 or (ph == 0).mean() > 0.4
    return ph


def make_init_rows(K):
    """12 rows: sums of 1 + a few ulp and of 1.03 (single steps), 1.3 (the jump), 0.9 (no step), in turn"""
    rng = np.random.default_rng([12, K])
    rows = rng.random((12, K)) ** 12
    rows[rng.random((12, K)) < 0.5] = 0.0
    rows[np.arange(12), rng.integers(0, K, 12)] += 0.05
    for r in range(12):
        rows[r] /= np.sum(rows[r])
        if r % 4 == 0:
            while not np.sum(rows[r]) > 1:
                rows[r] *= 1 + 2.0 ** -52
            assert 1 < np.sum(rows[r]) < 1 + 1e-13
        else:
            rows[r] *= (1.03, 1.3, 0.9)[r % 4 - 1]
    sums = np.array([np.sum(r) for r in rows])
    assert (sums[1::4] > 1.02).all() and (sums[1::4] < 1 + 128 * (C_INIT - 1)).all() and (sums[2::4] > 1.29).all() and (sums[3::4] < 1).all()
    return rows


def make_corpus(K, zero_word):
    lay = _layout(K)
    B = 2 * min(lay.G, 64)
    lens = [0, 1, 2, B, 0, B + 1, 5, 3, 7, 2, 1, 0]
    rng = np.random.default_rng([13, K])
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(0, V - 1, S).astype(np.int32)
    if zero_word:       # the lone site of document 1, the first site of the 2G document, the last of the 2G + 1 one, one more
        for s in (doc_off[1], doc_off[3], doc_off[6] - 1, doc_off[8] + 3):
            word[s] = V - 1
    freq = rng.integers(1, 5, S).astype(np.int32)
    init_idx = rng.integers(0, 12, S).astype(np.int32)
    init_idx[doc_off[3]:doc_off[3] + 12] = rng.permutation(12)          # every row is used
    return dict(doc_off=doc_off, word=word, freq=freq, init_idx=init_idx)


def make_case(K, setting, **change):
    """everything one call takes, in reference topic order; ``change`` overrides single arguments"""
    p = dict(SETTINGS[setting])
    zero_word = change.pop("zero_word", p["beta_fallback"])
    c = dict(K=K, phs=[make_loadings(K)], ph_sel=None, rows=make_init_rows(K), doc_ids=None, doc_base=1000, doc_stream=None,
             stream_id=STREAM, c_init=C_INIT, iters=4, thinning=2, seed=SEED, **p)
    c.update(make_corpus(K, zero_word))
    c.update(change)
    return c


def reference(c):
    D = len(c["doc_off"]) - 1
    ids = c["doc_ids"] if c["doc_ids"] is not None else c["doc_base"] + np.arange(D)
    streams = c["doc_stream"] if c["doc_stream"] is not None else np.full(D, c["stream_id"])
    return foldinref.fold_in(init_rows=c["rows"], init_idx=c["init_idx"], ph=c["phs"], ph_sel=c["ph_sel"], doc_off=c["doc_off"],
                             word=c["word"], freq=c["freq"], alpha=c["alpha"], beta=c["beta"], c_init=c["c_init"], c_loop=c["c_loop"],
                             beta_fallback=c["beta_fallback"], avg_mode=c["avg_mode"], iters=c["iters"], thinning=c["thinning"],
                             seed=c["seed"], doc_ids=ids, doc_streams=streams)


def device(c, start, exact_only=0, with_status=True):
    """one llda_foldin call -> dict(z topics [S], n_dk (D, K), th (D, K), status); start: "sites" (n_sites = S, the initial
    assignments by a launch of their own) or "inside" (n_sites = 0)"""
    import torch
    from lda_thesis_amd import _native
    K = c["K"]
    lay = _layout(K)
    KP, lm = lay.KP, lay.lm_topic_pos.astype(np.int64)
    D, S = len(c["doc_off"]) - 1, len(c["word"])
    valid = lay.lm_pos_topic >= 0
    assert valid.sum() == K and (lay.lm_pos_topic[lm] == np.arange(K)).all()

    def lane_major(m):                          # (R, K) -> (R, KP), zeros in the padding
        out = np.zeros((m.shape[0], KP), dtype=np.float64)
        out[:, lm] = m
        return out
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ph = dev(np.vstack([lane_major(p.T) for p in c["phs"]]))
    rows = dev(lane_major(c["rows"]))
    z = Guarded(np.full(S, lay.topic_pos[K - 1], dtype=np.int32))
    n_dk = Guarded(np.full(D * KP, 0 if start == "sites" else FILL, dtype=np.int32))
    th = Guarded(np.full(D * KP, np.nan, dtype=np.float64))
    status = torch.zeros((1,), dtype=torch.int32, device="cuda") if with_status else None
    opt = {}
    if c["doc_ids"] is not None:
        opt["doc_ids"] = dev(np.asarray(c["doc_ids"], dtype=np.int64))
    if c["doc_stream"] is not None:
        opt["doc_stream"] = dev(np.asarray(c["doc_stream"], dtype=np.uint32).view(np.int32))
    if c["ph_sel"] is not None:
        opt["ph_base"] = dev(np.asarray(c["ph_sel"], dtype=np.int64) * (V * KP))
    _native.foldin(doc_off=dev(c["doc_off"]), word=dev(c["word"]), init_idx=dev(c["init_idx"]), freq=dev(c["freq"]), ph=ph,
                   init_rows=rows, slot_valid=dev(valid.astype(np.uint8)), z=z.t, n_dk=n_dk.t, th=th.t, status=status, D=D, K=K,
                   iters=c["iters"], thinning=c["thinning"], alpha=c["alpha"], beta=c["beta"], c_init=c["c_init"], c_loop=c["c_loop"],
                   seed=c["seed"], stream_id=c["stream_id"], doc_base=c["doc_base"], beta_fallback=c["beta_fallback"],
                   avg_mode=c["avg_mode"], exact_only=bool(exact_only), n_sites=None if start == "sites" else 0, **opt)
    torch.cuda.synchronize()
    what = "K=%d %s" % (K, start)
    zp = z.host(what + " z")
    assert ((zp >= 0) & (zp < KP)).all() and (lay.pos_topic[zp] >= 0).all(), what + ": z is no position of a topic"
    nd, t = n_dk.host(what + " n_dk").reshape(D, KP), th.host(what + " th").reshape(D, KP)
    assert not nd[:, ~valid].any(), what + ": n_dk in the padding"
    assert (t[:, ~valid] == 0).all(), what + ": th in the padding"
    return dict(z=lay.pos_topic[zp].astype(np.int64), n_dk=nd[:, lm].astype(np.int64), th=t[:, lm],
                status=int(status.item()) if with_status else None)


def same(got, want, doc_off, skip=(), what=""):
    """z, n_dk and th of every document outside ``skip``, bit for bit"""
    for d in range(len(doc_off) - 1):
        if d in skip:
            continue
        sl = slice(int(doc_off[d]), int(doc_off[d + 1]))
        msg = "%s document %d (%d sites)" % (what, d, sl.stop - sl.start)
        np.testing.assert_array_equal(got["z"][sl], want["z"][sl], err_msg=msg + ": z")
        np.testing.assert_array_equal(got["n_dk"][d], want["n_dk"][d], err_msg=msg + ": n_dk")
        np.testing.assert_array_equal(got["th"][d], want["th"][d], err_msg=msg + ": th")


def check(c, want, start, exact_only=0, what=""):
    """the call gives the reference's outputs and status 0; with start = "inside" the other start path gives the same again"""
    assert not want["raises"].any()
    got = device(c, start, exact_only)
    assert got["status"] == 0, what
    same(got, want, c["doc_off"], what=what)
    lens = np.diff(c["doc_off"])
    assert not got["n_dk"][lens == 0].any() and not got["th"][lens == 0].any(), what + ": an empty document"
    np.testing.assert_array_equal(got["n_dk"].sum(axis=1), np.add.reduceat(np.append(c["freq"], 0), c["doc_off"][:-1]) * (lens > 0))
    if start == "inside":
        other = device(c, "sites", exact_only)
        same(got, other, c["doc_off"], what=what + " inside vs sites")
    return got


@functools.lru_cache(maxsize=None)
def grid_case(K, setting):
    c = make_case(K, setting)
    return c, reference(c)


@pytest.mark.parametrize("exact_only", [0, 1])
@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("K", GRID_KS)
def test_every_layout_both_start_paths(K, setting, start, exact_only):
    c, want = grid_case(K, setting)
    got = check(c, want, start, exact_only, "K=%d %s %s exact_only=%d" % (K, setting, start, exact_only))
    assert (got["th"][np.diff(c["doc_off"]) > 0].sum(axis=1) > 0.99).all()           # (thinned twice: rows of a distribution)


# ------------------------------------------------------------------------------------------------
# single options, K = 40 (G = 8, T = 8), 512 (G = 32, T = 16), 1031 (wide)
# ------------------------------------------------------------------------------------------------
def _singles():
    rng = np.random.default_rng(14)
    D = 12
    out = {
        # the id of document d is (uint32)(doc_base + d): it wraps after two documents
        "doc_base_wraps": ("llda", dict(doc_base=2 ** 32 - 2)),
        # any ids, only their low 32 bits count; a stream per document, the top bit in use
        "doc_ids_and_streams": ("flat", dict(doc_ids=rng.permutation(D) * 7919 + np.where(np.arange(D) % 2, 2 ** 40, 2 ** 32 - 5),
                                             doc_stream=rng.integers(0, 2 ** 32, D, dtype=np.uint64))),
        "iters_0": ("llda", dict(iters=0)),
        "thin_5_2": ("llda", dict(iters=5, thinning=2)),
        "thin_2_3": ("flat", dict(iters=2, thinning=3)),
        "thin_6_6": ("flat", dict(iters=6, thinning=6)),
        # c_loop - 1 < 1e-9 / a tiny alpha: legal; for the first the host takes the exact pipeline by itself
        "c_loop_2p-36": ("llda", dict(c_loop=1 + 2.0 ** -36)),
        "alpha_1e-9": ("flat", dict(alpha=1e-9)),
    }
    return out


SINGLES = _singles()


@functools.lru_cache(maxsize=None)
def single_case(K, name):
    setting, change = SINGLES[name]
    c = make_case(K, setting, **change)
    return c, reference(c)


@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("name", sorted(SINGLES))
@pytest.mark.parametrize("K", SINGLE_KS)
def test_single_options(K, name, start):
    c, want = single_case(K, name)
    got = check(c, want, start, 0, "K=%d %s %s" % (K, name, start))
    if c["iters"] < c["thinning"]:
        assert not got["th"].any()                                   # no sweep reaches the thinning: th = 0


def test_single_cases_differ_from_the_grid():
    """(host only, cheap) the options above change the reference's result: a kernel that ignored one could not pass"""
    base = grid_case(40, "llda")[1]
    assert not np.array_equal(single_case(40, "doc_base_wraps")[1]["z"], base["z"])
    assert not np.array_equal(single_case(40, "thin_5_2")[1]["z"], base["z"])        # (th is that of sweep 4: the fifth only moves z)
    np.testing.assert_array_equal(single_case(40, "thin_5_2")[1]["th"], base["th"])
    flat = grid_case(40, "flat")[1]
    assert not np.array_equal(single_case(40, "doc_ids_and_streams")[1]["z"], flat["z"])
    assert not np.array_equal(single_case(40, "alpha_1e-9")[1]["z"], flat["z"])


@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("K", SINGLE_KS)
def test_two_loadings_matrices_in_one_launch(K, start):
    """ph_base: every document samples against its own matrix and equals the reference run against that matrix alone"""
    sel = np.array([0, 1, 1, 0, 1, 1, 0, 0, 1, 0, 1, 0])
    c = make_case(K, "flat", phs=[make_loadings(K), make_loadings(K, variant=1)], ph_sel=sel)
    got = device(c, start)
    assert got["status"] == 0
    for j in (0, 1):
        alone = dict(c, phs=[c["phs"][j]], ph_sel=None)
        want = reference(alone)
        assert not want["raises"].any()
        same(got, want, c["doc_off"], skip=set(np.flatnonzero(sel != j)), what="K=%d %s matrix %d" % (K, start, j))
        if j == 1:      # (the second matrix matters: the documents of the first differ under it)
            assert not np.array_equal(got["z"][c["doc_off"][3]:c["doc_off"][4]], want["z"][c["doc_off"][3]:c["doc_off"][4]])


@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("K", SINGLE_KS)
def test_status_reports_a_site_without_probability(K, start):
    """without the fall-back a document that holds the word no topic loads on sets bit 0 of status (the reference would raise there);
    its own outputs are left open, every other document still equals the reference; status = NULL gives the same outputs"""
    c = make_case(K, "llda")
    bad = 6                                                           # a document of 5 sites
    c["word"] = c["word"].copy()
    c["word"][c["doc_off"][bad] + 2] = V - 1
    want = reference(c)
    np.testing.assert_array_equal(np.flatnonzero(want["raises"]), [bad])
    for exact_only in (0, 1):
        got = device(c, start, exact_only)
        assert got["status"] & 1
        same(got, want, c["doc_off"], skip={bad}, what="K=%d %s" % (K, start))
        quiet = device(c, start, exact_only, with_status=False)
        same(quiet, got, c["doc_off"], what="K=%d %s status = NULL" % (K, start))
