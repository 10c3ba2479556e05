"""llda_sweep_batch driven directly (include/llda_gibbs.h llda_batch_args): wavefronts whose lane groups belong to DIFFERENT problems
-- other K, other KP, other count block, other RNG stream, other dense layout in the exact tier --, ``order`` tensors Ensemble never
builds, and the read-outs on such an ensemble.  Cases and runner: tests/batchdirect.py; what is pinned and the measured times: DESIGN.md
4.4n.  Every comparison is of whole buffers, bit for bit, against the C oracle run problem by problem on CPU copies of the tensors the
launch took (helpers.OracleBackend.sweep_batch); z, n_dk and delta carry guard words before and behind; counts must not change.

The status words are predicted, not measured: margin -1 sends every site of the launch through the exact tier, margin 0 none (random
counts: the closest site is 2^-20 of the total away, the band is 2^-40), and at margin 4 (a band of 2^-4) the sites inside the band are
counted on the oracle's trajectory by batchdirect.predict_exact.

The first test of the file carries no gpu mark and proves NOTHING about the kernel: it runs the runner with the oracle stand-in on both
sides (the same code twice), so what it checks is the construction of the cases, the plumbing of the runner and the predictions of
predict_exact -- a mistake in those then shows where there is no GPU, before the device tests are ever run.
"""
import numpy as np
import pytest

import batchdirect as bd
from helpers import OracleBackend

gpu = pytest.mark.gpu
MARGINS = (0, 4, -1)
MARGIN_REL = {0: 2.0 ** -40, 4: 2.0 ** -4, -1: 2.0}
_RUNS = {}


def _run(lanes, empty=False):
    """the device state of a case, built once per process and reset for every test"""
    import lda_thesis_amd._native as native
    key = (lanes, empty)
    if key not in _RUNS:
        _RUNS[key] = bd.Run(bd.case(lanes, empty), native)
    _RUNS[key].reset()
    return _RUNS[key]


def _want_status(r, before, after, order, margin, empty_sites=0):
    """status words 0 and 2 of one launch from zeroed words"""
    n_exact, edge = bd.predict_exact(before, after, order, MARGIN_REL[margin])
    assert edge > 1e-9, "a site sits on the edge of the band: the prediction would depend on the last bit"
    if margin == -1:
        assert n_exact == r.sites(order)
    if margin == 0:
        assert n_exact == empty_sites
    return [(2 if n_exact else 0) | (1 if empty_sites else 0), n_exact]


def _launch_and_check(r, co, order, lanes, margin, what):
    """one launch, compared with the oracle's; -> (before, after) CPU tensors"""
    backend = OracleBackend(co)
    before = r.host()
    after = {k: v.clone() for k, v in before.items()}
    r.oracle_launch(backend, after, order)
    assert bool((after["z"] != before["z"]).any()), "%s: the oracle moves no site" % what
    r.launch(order, lanes, margin)
    r.check(after, what)
    st = r.status()
    assert [st[0], st[2]] == _want_status(r, before, after, order, margin), (what, st)
    return before, after


# ------------------------------------------------------------------------------------------------
# without a device: the cases and the runner
# ------------------------------------------------------------------------------------------------
def test_cases_and_predictions_without_a_device(c_oracle, monkeypatch):
    """NOT a test of the kernel: the oracle stand-in plays the device, so `r.check` compares the C oracle with itself.  Pinned here: the
    case tables (n_inst, K, KP, exact label-set sizes, the empty instance), that a sweep moves sites, that a K = 1 instance keeps its
    own, and the exact-tier counts the device tests predict (none at margin 0, all at -1, some at 4, none on the edge of the band)."""
    import lda_thesis_amd.ensemble as E
    backend = OracleBackend(c_oracle)
    monkeypatch.setattr(E, "_native", backend)
    for lanes in (8, 16, 32, 64):
        c = bd.case(lanes)
        cl = bd.CLASSES[lanes]
        assert len(c["order_rr"]) == cl["n_inst"] and sorted(c["order_rr"].tolist()) == list(range(cl["n_inst"]))
        assert [pl["K"] for pl in c["plans"]] == list(cl["Ks"])
        r = bd.Run(c, backend, device="cpu")
        kps = sorted(set(int(x) for x in r.ens._kp_h))
        assert kps == ([8, 16, 32, 64, 96, 128] if lanes == 8 else sorted(set(orc_kp(K) for K in cl["Ks"])))
        before = r.host()
        after = {k: v.clone() for k, v in before.items()}
        r.oracle_launch(backend, after, c["order_rr"])
        r.launch(c["order_rr"], lanes, 0)
        r.check(after, "host runner, lanes %d" % lanes)
        moved = int((after["z"] != before["z"]).sum())
        assert moved > r.sites(c["order_rr"]) // 8, "the sweep moves sites"
        # the predictions the device tests rely on
        for margin in MARGINS:
            n_exact, edge = bd.predict_exact(before, after, c["order_rr"], MARGIN_REL[margin])
            assert edge > 1e-9
            if margin != 4:
                assert n_exact == (0 if margin == 0 else r.sites(c["order_rr"]))
            else:
                assert 0 < n_exact < r.sites(c["order_rr"])              # decided and exact sites in one launch
        # a K = 1 instance keeps every site
        if lanes == 8:
            for i in np.flatnonzero(before["inst_prob"].numpy() == 0):
                assert (after["z"][r.z_slice(i)] == before["z"][r.z_slice(i)]).all()
    c = bd.case(8, True)
    assert c["n_allowed"][bd.EMPTY_DOC] == 0 and c["lens"][bd.EMPTY_DOC] == 3


def orc_kp(K):
    return bd.orc.layout(K).KP


# ------------------------------------------------------------------------------------------------
# mixed wavefronts at every lane class
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_mixed_wavefronts(c_oracle, lanes, margin):
    """every instance of the class, round-robin over the problems: neighbouring lane groups never share a problem; the last workgroup
    has idle groups"""
    r = _run(lanes)
    c = r.c
    before, after = _launch_and_check(r, c_oracle, c["order_rr"], lanes, margin, "lanes %d margin %d" % (lanes, margin))
    if lanes == 8:                                                       # a K = 1 instance keeps every site
        z = r.ens.z.cpu().numpy()
        for i in np.flatnonzero(before["inst_prob"].numpy() == 0):
            assert (z[r.z_slice(i)] == before["z"].numpy()[r.z_slice(i)]).all()


# ------------------------------------------------------------------------------------------------
# what `order` means (the lanes-8 ensemble)
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("margin", [4, -1])
def test_order_subset_in_reverse(c_oracle, margin):
    r = _run(8)
    order = r.c["order_rr"][::3][::-1]
    before, after = _launch_and_check(r, c_oracle, order, 8, margin, "every third instance, reversed")
    z, nd = r.ens.z.cpu().numpy(), r.ens.n_dk.cpu().numpy()
    for i in sorted(set(range(r.ens.I)) - set(order.tolist())):         # (implied by the whole-buffer comparison; stated for the reader)
        assert (z[r.z_slice(i)] == before["z"].numpy()[r.z_slice(i)]).all() and (nd[r.ndk_slice(i)] == before["n_dk"].numpy()[r.ndk_slice(i)]).all()
    assert int((after["z"] != before["z"]).sum()) > 0


@gpu
@pytest.mark.parametrize("margin", [4, -1])
def test_disjoint_launches_equal_their_union(c_oracle, margin):
    r = _run(8)
    rr = r.c["order_rr"]
    before, after = _launch_and_check(r, c_oracle, rr, 8, margin, "the union")
    r.reset()
    first, second = rr[0::2], rr[1::2][::-1]
    r.launch(first, 8, margin)
    assert int((r.ens.delta != 0).sum()) > 0                             # the second launch adds to a delta that holds changes
    r.launch(second, 8, margin)
    r.check(after, "two launches over disjoint subsets")
    assert r.status()[2] == bd.predict_exact(before, after, rr, MARGIN_REL[margin])[0]


@gpu
@pytest.mark.parametrize("margin", [4, -1])
def test_permutations_of_one_order(c_oracle, margin):
    """three permutations of one ``order`` -- a proper subset of the instances: a launch that took instances 0 .. n_inst - 1, whatever
    ``order`` says, would leave the same buffers for every permutation of ALL instances -- and of all of them"""
    r = _run(8)
    rr = r.c["order_rr"]
    for base in (rr[1::2], rr):
        perms = [base, base[::-1], np.random.default_rng(5).permutation(base), np.sort(base)]     # (the last: problem by problem, as Ensemble numbers them)
        want = None
        for k, order in enumerate(perms):
            r.reset()
            if want is None:
                want = _launch_and_check(r, c_oracle, order, 8, margin, "permutation 0 of %d instances" % len(base))[1]
            else:
                r.launch(order, 8, margin)
                r.check(want, "permutation %d of %d instances" % (k, len(base)))


@gpu
@pytest.mark.parametrize("margin", [0, -1])
def test_one_instance(c_oracle, margin):
    """n_inst = 1: 31 idle groups, 7 of them in the first wavefront, all reading order[0]"""
    r = _run(8)
    c = r.c
    # five batches of 8 sites and more than one allowed topic, at the largest K that has such a document
    j = max(np.flatnonzero((c["lens"] == 40) & (c["n_allowed"] >= 2)), key=lambda j: c["plans"][c["prob_of_doc"][j]]["K"])
    i = int(c["order_rr"][j])
    assert r.sites([i]) == 40 and c["plans"][c["prob_of_doc"][j]]["K"] == 100 and i != 0             # (KP = 128, a tail of 4)
    _launch_and_check(r, c_oracle, np.array([i]), 8, margin, "one instance")


@gpu
@pytest.mark.parametrize("margin", [4, -1])
def test_more_lanes_than_a_set_needs(c_oracle, margin):
    """the lanes-8 instances with 64 lanes each: one group a wavefront, 56 lanes and more of it idle"""
    r = _run(8)
    _launch_and_check(r, c_oracle, r.c["order_rr"], 64, margin, "lanes 64 for sets of <= 8")


# ------------------------------------------------------------------------------------------------
# an instance without an allowed topic
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("margin", [0, -1])
def test_empty_label_set(c_oracle, margin):
    """total 0 -> the exact tier -> no topic with a positive probability: z stays, bit 0 of status[0] is set, nothing else changes (the
    sentence in the llda_batch_args comment).  Every other instance equals the oracle run of the same launch WITHOUT the instance."""
    r = _run(8, True)
    c = r.c
    e = c["empty_inst"]
    rr = c["order_rr"]
    others = rr[rr != e]
    assert len(others) == len(rr) - 1 and r.sites([e]) == 3
    before = r.host()
    after = {k: v.clone() for k, v in before.items()}
    r.oracle_launch(OracleBackend(c_oracle), after, others)
    r.launch(rr, 8, margin)
    r.check(after, "an empty label set among ordinary instances")       # (z, n_dk of the instance unchanged, delta holds nothing from it)
    st = r.status()
    assert st[0] & 1
    assert [st[0], st[2]] == _want_status(r, before, after, rr, margin, empty_sites=3), st
    with pytest.raises(ValueError):
        r.ens.check_status()


# ------------------------------------------------------------------------------------------------
# the read-outs on the mixed ensemble (K up to 128, a topic nobody uses)
# ------------------------------------------------------------------------------------------------
@gpu
def test_readouts_after_two_sweeps(c_oracle):
    import torch
    r = _run(8)
    c, ens = r.c, r.ens
    backend = OracleBackend(c_oracle)
    host = r.host()
    for sweep in range(2):
        r.oracle_launch(backend, host, c["order_rr"], sweep=sweep)
        backend.apply_delta(host["counts"], host["delta"])
        r.launch(c["order_rr"], 8, 0, sweep=sweep)
        r.fold()
    r.check(host, "two sweeps")
    label_rows, nrow = [], 0
    for i, pl in enumerate(c["plans"]):                                  # every second topic of every problem gets a row of ph, in a scattered order
        rows = np.full(pl["K"], -1, dtype=np.int64)
        rows[i % 2::2] = nrow + np.arange(len(rows[i % 2::2]))[::-1]
        nrow += len(rows[i % 2::2])
        if i == c["unused"][0] and rows[c["unused"][1]] < 0:             # ... and the topic nobody uses
            rows[c["unused"][1]] = nrow
            nrow += 1
        label_rows.append(rows.tolist())
    fill = -123.25
    ph_dev = torch.full((nrow + 3, bd.V), fill, dtype=torch.float64, device=ens.device)
    ens.scatter_ph(ph_dev, label_rows)
    ph_dev = ph_dev.cpu().numpy()
    want_dev = np.full((nrow + 3, bd.V), fill)
    got_rows = ens.ph_rows()
    up, ut = c["unused"]
    for i, pl in enumerate(c["plans"]):
        n_k_v, n_d_k, n_zk, z, ph = bd.numpy_state(ens, c, host, i)
        got = ens.problem_state(i)
        for a, b, name in zip(got, (n_k_v, n_d_k, n_zk, z), ("n_k_v", "n_d_k", "n_zk", "z")):
            assert a.dtype == np.int64 and a.shape == b.shape, (i, name)
            np.testing.assert_array_equal(a, b, err_msg="problem %d %s" % (i, name))
        g = got_rows[i].cpu().numpy()
        assert g.shape == (pl["K"], bd.V) and np.array_equal(bd.canon(g), bd.canon(ph)), "get_ph of problem %d" % i
        if i == up:
            assert np.isnan(ph[ut]).all() and np.isnan(g[ut]).all() and int(n_k_v[ut].sum()) == 0      # 0/0: the topic nobody uses
            assert np.isfinite(np.delete(ph, ut, axis=0)).all()
        else:
            assert np.isfinite(ph).all()
        for t, row in enumerate(label_rows[i]):
            if row >= 0:
                want_dev[row] = ph[t]
    assert np.array_equal(bd.canon(ph_dev), bd.canon(want_dev)), "scatter_ph"
    assert label_rows[up][ut] >= 0                                       # (the 0/0 row is among the scattered ones)
