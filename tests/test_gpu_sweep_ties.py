"""The sweep kernels on the planted states of tests/sweepties.py: last-bit ties of the keyed draw (within 2^-46 of the total of a prefix
boundary in exact arithmetic, most within 2^-56) and sites 2^-38 .. 2^-36 outside tier 1's band, at four kinds of boundary, planted and
random documents side by side in one wavefront (tests/test_sweep_ties_host.py shows what the states hold and that they catch a tier 1
without a margin, a sequential sum, a reciprocal-multiply, a `>=` and fp32 scores at every K used here).

One sweep per case.  z, n_d_k, n_k_v, n_zk equal the C oracle's (/root/reference/LabeledLDA.py:106-125) bit for bit at every margin, and
the status words are what DESIGN.md 4.3's bounds say, not what was measured: at production margins tier 0 hands over exactly the planted
sites (status[1] = ties + outside) and tier 1 exactly the ties (status[2] = ties: an outside site is 4 .. 16 bands away and tier 1's error
is a sixteenth of the band; a tie is 2^6 times closer than the band is wide); without the fp32 tier (debug_margin -2) status[2] = ties;
with -1 every site goes through the exact pipeline.

Failing cases on the MI355X when this file was written: none in any family (general 15 cases, quad 5, sparse-label 7, wide 3, batched 2:
0 of 32 -- the kernels leave the oracle's state and the status words of the table at every margin).  The two wide cases added since
(the largest K of five and of seven tiers: the scan's carry over more than four tiers) pass as well, and so do the two mixed-wave cases
of the batched kernel (test_batched_mixed_waves; with exact_call reading K from lane 0 of the wavefront both fail).
"""
import numpy as np
import pytest

import sweepties as st

pytestmark = pytest.mark.gpu


def _oracle(c_oracle, s):
    cs = c_oracle.CState(s["doc_off"], s["word"], s["freq"], s["z"], s["labs"], s["n_d_k"], s["n_k_v"], s["n_zk"], s["V"], s["alpha"], s["beta"])
    cs.sweep(1, s["seed"], 0, stream=s["stream"], doc_base=s["doc_base"], threads=4)
    return cs


def _run(c_oracle, s, margins, check=None, **kw):
    """one sweep of the planted state per margin -> {margin: status words}; the state is the C oracle's after each"""
    from lda_thesis_amd.sampler import GibbsSampler
    cs = _oracle(c_oracle, s)
    counts = dict(n_d_k=s["n_d_k"], n_k_v=s["n_k_v"], n_zk=s["n_zk"])
    status = {}
    for margin in margins:
        g = GibbsSampler(s["doc_off"], s["word"], s["freq"], s["z"], s["n_d_k"].shape[1], s["V"], s["alpha"], s["beta"], counts=counts,
                         seed=s["seed"], doc_base=s["doc_base"], sort_docs=False, **kw)
        g.debug_margin = margin
        g.sweep()
        g.check_status()
        if check is not None:                              # (after the sweep: the quad kernels' row flags are written by it)
            check(g)
        what = "debug_margin %d" % margin
        np.testing.assert_array_equal(g.z_topics(), cs.z, err_msg=what)
        np.testing.assert_array_equal(g.n_d_k(), cs.n_d_k, err_msg=what)
        np.testing.assert_array_equal(g.n_k_v(), cs.n_k_v, err_msg=what)
        np.testing.assert_array_equal(g.n_zk(), cs.n_zk, err_msg=what)
        status[margin] = g.status.cpu().numpy()
    return status


def _status_words(s, status, tier0=(0,)):
    """the table of the module docstring"""
    n_sites = int(s["doc_off"][-1])
    for m in tier0:
        assert int(status[m][1]) == s["n_ties"] + s["n_outside"], (m, int(status[m][1]), s["n_ties"], s["n_outside"])
        assert int(status[m][2]) == s["n_ties"], (m, int(status[m][2]), s["n_ties"])
    if -2 in status:
        assert int(status[-2][2]) == s["n_ties"], (int(status[-2][2]), s["n_ties"])
    assert int(status[-1][2]) == n_sites


@pytest.mark.parametrize("K,dense", st.GENERAL)
def test_general_kernel(c_oracle, K, dense):
    """llda_sweep_kernel (cold_tiers, exact_site_wave): every group width G = 8 .. 64, with and without a tail and PAD positions"""
    s = st.general_state(K, dense)
    status = _run(c_oracle, s, (0, -2, -1), labs=None if dense else s["labs"], sparse_labels=False, quad=False)
    _status_words(s, status)


@pytest.mark.parametrize("K", st.QUAD)
def test_quad_kernel(c_oracle, K):
    """llda_sweep_quad_kernel: quad_tier1_doc (one unsure document on 64 lanes, another summation order) and the out-of-line exact path;
    4, 8 and 16 documents a wavefront, K = 100 and 400 with PAD positions"""
    s = st.quad_state(K)
    assert int(s["n_k_v"].max()) <= 65535 and int(s["n_d_k"].sum(axis=1).max()) < 65536

    def check(g):
        assert g.quad and g.row16 is not None and int((g.row16 == 0).sum()) == 0

    status = _run(c_oracle, s, (0, -2, -1), check, commit_log=True, rows16=True, quad=True)
    _status_words(s, status)


@pytest.mark.parametrize("K,labels,image", st.SPARSE)
def test_sparse_label_kernel(c_oracle, K, labels, image):
    """llda_sweep_sparse_kernel (sparse_site, its exact_call): 8, 32 and 64 lanes a document, images of 0, 8 and 16 bits, wide layouts"""
    s = st.sparse_state(K, labels)

    def check(g):
        assert g.live_off is not None and (g.n_kw_img is not None) == bool(image)

    status = _run(c_oracle, s, (0, -1), check, labs=s["labs"], image=image)
    _status_words(s, status)


@pytest.mark.parametrize("K,dense", st.WIDE)
def test_wide_layouts(c_oracle, K, dense):
    """kernel_wide.hpp (wide_rare_tiers, wide_draw, wide_exact_site): the fp32-tiered kernel in both of its LDS forms (-6, -7)"""
    s = st.wide_state(K, dense)
    status = _run(c_oracle, s, (0, -1, -6, -7), labs=None if dense else s["labs"], sparse_labels=False)
    _status_words(s, status, tier0=(0, -6, -7))


def _planted_ensemble(subs, streams=None):
    """one Ensemble over the sub-problems ``subs`` (planted states over one vocabulary, each with its own word range).  The Ensemble
    counts its state from the assignments, so the planted counts are written over it."""
    import torch
    from lda_thesis_amd.ensemble import Ensemble
    V, alpha, beta = subs[0]["V"], subs[0]["alpha"], subs[0]["beta"]
    assert all(s["V"] == V for s in subs) and sum(int(s["doc_off"][-1]) for s in subs) == V
    lens = np.concatenate([np.diff(s["doc_off"]) for s in subs])
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    word = np.concatenate([s["word"] for s in subs]).astype(np.int32)
    freq = np.concatenate([s["freq"] for s in subs]).astype(np.int32)
    assert (word == np.arange(V)).all() and int(freq.max()) < V
    plans, d0 = [], 0
    for s in subs:
        D, K = s["labs"].shape
        n_allowed = s["labs"].sum(axis=1).astype(np.int64)
        allowed = np.full((D, int(n_allowed.max())), -1, dtype=np.int64)
        for d in range(D):
            allowed[d, :n_allowed[d]] = np.flatnonzero(s["labs"][d])
        plans.append(dict(K=K, docs=np.arange(d0, d0 + D, dtype=np.int64), allowed=allowed, n_allowed=n_allowed))
        d0 += D
    ens = Ensemble(plans, [s["z"] for s in subs], doc_off, word, freq, V, alpha, beta, st.SEED, streams=streams)
    for i, s in enumerate(subs):                         # the planted counts in the device's position order
        kp, tp = int(ens._kp_h[i]), torch.from_numpy(ens._layouts[plans[i]["K"]].topic_pos.astype(np.int64)).to(ens.device)
        D = s["labs"].shape[0]
        kw0, nk0 = int(ens._kw_off_h[i]), int(ens._nk_off_h[i])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=ens.device, dtype=torch.int32)
        blk = torch.zeros((V, kp), dtype=torch.int32, device=ens.device)
        blk[:, tp] = up(s["n_k_v"].T)
        ens.counts[kw0:kw0 + V * kp] = blk.reshape(-1)
        row = torch.zeros((kp,), dtype=torch.int32, device=ens.device)
        row[tp] = up(s["n_zk"])
        ens.counts[nk0:nk0 + kp] = row
        rows = torch.zeros((D, kp), dtype=torch.int32, device=ens.device)
        rows[:, tp] = up(s["n_d_k"])
        r0 = int(ens._ndk_off_h[int(ens._n_docs_h[:i].sum())])
        ens.n_dk[r0:r0 + D * kp] = rows.reshape(-1)
        got = ens.problem_state(i)
        for a, b in zip(got, (s["n_k_v"], s["n_d_k"], s["n_zk"], s["z"])):
            np.testing.assert_array_equal(a, b)
    return ens


def _equals_the_oracle(c_oracle, ens, subs):
    for i, s in enumerate(subs):
        cs = _oracle(c_oracle, s)
        n_k_v, n_d_k, n_zk, z = ens.problem_state(i)
        what = "sub-problem %d" % i
        np.testing.assert_array_equal(z, cs.z, err_msg=what)
        np.testing.assert_array_equal(n_d_k, cs.n_d_k, err_msg=what)
        np.testing.assert_array_equal(n_k_v, cs.n_k_v, err_msg=what)
        np.testing.assert_array_equal(n_zk, cs.n_zk, err_msg=what)


@pytest.mark.parametrize("margin", [0, -1])
def test_batched_kernel(c_oracle, margin):
    """llda_sweep_batch_kernel: one Ensemble of four sub-problems (K = 5, 60, 128, 100: lane classes 8, 16, 32, 64), each sub-problem's
    documents a planted state of its K under SubLDA's key (stream = index of the sub-problem, documents counted from 0), all over one
    vocabulary."""
    subs = [st.batch_state(i) for i in range(len(st.BATCH))]
    V = subs[0]["V"]
    ens = _planted_ensemble(subs)
    assert [g for g, _ in ens.orders] == [8, 16, 32, 64]
    ens.debug_margin = margin
    ens.sweep()
    ens.check_status()
    _equals_the_oracle(c_oracle, ens, subs)
    if margin == 0:                                      # the kernel's one margin is tier 1's: exactly the ties take the exact pipeline
        assert int(ens.status[2]) == sum(s["n_ties"] for s in subs)
    else:
        assert int(ens.status[2]) == V


@pytest.mark.parametrize("margin", [0, -1])
def test_batched_mixed_waves(c_oracle, margin):
    """llda_sweep_batch_kernel with lane groups of DIFFERENT sub-problems in one wavefront: the sub-problems of sweepties.BATCH_MIXED
    share a lane class but not a layout (K = 100 with 128 and 60 with 64: the same KP, another tail; 96: another KP), and the launches
    are made directly with the interleaved ``order`` of sweepties.mixed_order -- neighbouring groups never share a problem, every
    wavefront holds planted and random documents.  The exact tier reads the dense layout of the group it serves from that group's lanes
    (exact_call); with a neighbour's K the planted ties go wrong (model (f) of tests/test_sweep_ties_host.py)."""
    import batchdirect as bd
    from helpers import OracleBackend
    from lda_thesis_amd import _native
    subs = [st.mixed_state(i) for i in range(len(st.MIXED_SUBS))]
    ens = _planted_ensemble(subs, streams=[m[5] for m in st.MIXED_SUBS])
    assert [g for g, _ in ens.orders] == [lanes for lanes, _, _ in st.BATCH_MIXED]
    # z, n_dk and delta in buffers with guard words before and behind; every launch compared as WHOLE buffers -- the padding positions
    # of the rows and delta before the fold included -- with the C oracle run problem by problem on CPU copies of the same tensors
    r = bd.Run.of(ens, _native)
    backend = OracleBackend(c_oracle)
    start = np.concatenate(([0], np.cumsum(ens._n_docs_h)))
    want = r.host()
    for g, (lanes, D, _) in enumerate(st.BATCH_MIXED):
        order = np.array([start[i] + d for i, d in st.mixed_order(g)], dtype=np.int32)
        assert sorted(order.tolist()) == sorted(ens.orders[g][1].cpu().tolist())          # Ensemble's launch of the class, in another order
        r.oracle_launch(backend, want, order)
        r.launch(order, lanes, margin)
        r.check(want, "mixed waves, lanes %d, margin %d" % (lanes, margin))            # (counts unchanged by the launch, guards intact)
    assert int((want["delta"] != 0).sum()) > 0
    r.fold()
    backend.apply_delta(want["counts"], want["delta"])
    r.check(want, "mixed waves after the fold")
    ens.check_status()
    _equals_the_oracle(c_oracle, ens, subs)              # ... and every sub-problem on its own, a whole sweep of the C oracle
    agg = dict(doc_off=np.array([0, ens.S]), n_ties=sum(s["n_ties"] for s in subs), n_outside=sum(s["n_outside"] for s in subs))
    status = ens.status.cpu().numpy()
    assert int(status[1]) == 0                           # (the batched kernel has no fp32 tier: nothing is handed over by one)
    if margin == 0:
        assert int(status[2]) == agg["n_ties"]           # its one margin is tier 1's: exactly the ties take the exact pipeline
    else:
        _status_words(agg, {-1: status}, tier0=())
