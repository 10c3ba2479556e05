"""Estimating alpha and beta during training: GibbsSampler.count_histograms / set_priors, LabeledLDA.optimize_priors and
run_training(optimize_interval=...), on the device.

The histograms equal numpy's of the sampler's own counts; priors set mid-chain reach every kernel family (the state after further
sweeps equals the C oracle's under the same two doubles, the read-outs the numpy oracle's); the drop-in class estimates exactly what
priors.estimate gives on its host-side state, and fold-in, pickling and several ranks go on with the new values."""
import math
import pickle
import types

import numpy as np
import pytest

from test_gpu_long_docs_and_keys import _assert_equal, ran_general, ran_quad, ran_sparse

pytestmark = pytest.mark.gpu

V = 300
ALPHA0, BETA0 = 0.1, 0.01


def small_corpus(K, labels, D, seed=0):
    """D documents of 5 ... 60 sites over V = 300 words; labels: 'dense', 'heavy' (more than a quarter of K, never all: label masks
    on the general kernel) or 'root7' (root plus 7 labels: the sparse-label kernels)"""
    import longdocs as L
    rng = np.random.default_rng([seed, K, D])
    lens = rng.integers(5, 61, size=D)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, 4, size=int(doc_off[-1])).astype(np.int32)
    if labels == "root7":
        labs = np.zeros((D, K), dtype=np.uint8)
        labs[:, 0] = 1
        for d in range(D):
            labs[d, 1 + rng.choice(K - 1, size=7, replace=False)] = 1
    else:
        labs = L.label_sets(rng, lens, K, labels)
    z = np.concatenate([np.flatnonzero(labs[d])[rng.integers(0, int(labs[d].sum()), size=int(lens[d]))] for d in range(D)])
    tokens = np.bincount(np.repeat(np.arange(D), lens), weights=freq, minlength=D).astype(np.int64)
    return dict(doc_off=doc_off, word=word, freq=freq, labs=labs, z=z.astype(np.int64), V=V, lens=lens, tokens=tokens)


# family: (K, labels, documents, sampler arguments, the kernel it must take)
FAMILIES = {
    "quad128": (128, "dense", 150, dict(commit_log=True, quad=True), ran_quad),
    "general40_masks": (40, "heavy", 300, dict(commit_log=False), ran_general(False, False)),
    "sparse512_image8": (512, "root7", 200, dict(image=8), ran_sparse(8, False)),
    "wide_sparse1031": (1031, "root7", 100, dict(), ran_sparse(0, True)),
}
SEED = 0x5EED0123


def start(co, family, sweeps=2):
    """a sampler of the family and the C oracle beside it, both ``sweeps`` sweeps on"""
    from lda_thesis_amd.sampler import GibbsSampler
    K, labels, D, kw, ran = FAMILIES[family]
    c = small_corpus(K, labels, D)
    s = GibbsSampler(c["doc_off"], c["word"], c["freq"], c["z"], K, V, ALPHA0, BETA0, labs=c["labs"], seed=SEED, **kw)
    ran(s)
    cs = co.CState(c["doc_off"], c["word"], c["freq"], c["z"], c["labs"], s.n_d_k(), s.n_k_v(), s.n_zk(), V, ALPHA0, BETA0)
    for i in range(sweeps):
        s.sweep()
        cs.sweep(1, SEED, i, threads=4)
    _assert_equal(s, cs, "before the priors change")
    return c, s, cs, ran


def host_histograms(n_d_k, n_k_v, labs, n_bins):
    dk, kw = n_d_k[np.asarray(labs) != 0], n_k_v.ravel()
    return (np.bincount(dk[dk < n_bins], minlength=n_bins).astype(np.int64), np.sort(dk[dk >= n_bins]),
            np.bincount(kw[kw < n_bins], minlength=n_bins).astype(np.int64), np.sort(kw[kw >= n_bins]))


def host_estimate(alpha, beta, n_d_k, n_k_v, n_zk, labs, n_bins=65536):
    from lda_thesis_amd import priors
    h = host_histograms(n_d_k, n_k_v, labs, n_bins)
    cls = priors.doc_classes((np.asarray(labs) != 0).sum(axis=1), n_d_k.sum(axis=1))
    return priors.estimate(alpha, beta, hist_dk=h[0], over_dk=h[1], classes=cls, hist_kw=h[2], over_kw=h[3], n_k=n_zk, V=n_k_v.shape[1])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_count_histograms_equal_the_host_histograms_of_the_counts(c_oracle, family):
    c, s, cs, ran = start(c_oracle, family)
    for n_bins in (8, 65536):                 # (8: the larger counts of n_dk and n_kw travel through the overflow lists)
        got = s.count_histograms(n_bins)
        want = host_histograms(s.n_d_k(), s.n_k_v(), c["labs"], n_bins)
        for g, w, name in zip(got, want, ("hist_dk", "over_dk", "hist_kw", "over_kw")):
            assert g.dtype == np.int64
            np.testing.assert_array_equal(g, w, err_msg="%s n_bins=%d" % (name, n_bins))
        assert int(got[0].sum()) + got[1].size == int(c["labs"].sum()) and int(got[2].sum()) + got[3].size == s.K * V
    assert host_histograms(s.n_d_k(), s.n_k_v(), c["labs"], 8)[1].size > 0
    with pytest.raises(ValueError):
        s.count_histograms(0)
    ran(s)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_new_priors_reach_every_kernel_path(c_oracle, family):
    import llda_oracle as orc
    import torch
    c, s, cs, ran = start(c_oracle, family)
    est = host_estimate(ALPHA0, BETA0, s.n_d_k(), s.n_k_v(), s.n_zk(), c["labs"])
    assert est.converged and est.alpha != ALPHA0 and est.beta != BETA0
    for bad in ((9e-7, 0.01), (0.1, 9e-7), (0.1, 2.0 ** 40 / V), (float("nan"), 0.01)):
        with pytest.raises(ValueError):
            s.set_priors(*bad)
    assert (s.alpha, s.beta) == (ALPHA0, BETA0)
    s.set_priors(est.alpha, est.beta)
    cs.alpha, cs.beta = est.alpha, est.beta
    for i in range(2, 4):
        s.sweep()
        cs.sweep(1, SEED, i, threads=4)
        _assert_equal(s, cs, "sweep %d, with the estimated priors" % (i + 1))
    s.check_status()
    ran(s)
    # the same chain under the OLD priors ends elsewhere: the comparison above can tell the two apart
    old = c_oracle.CState(c["doc_off"], c["word"], c["freq"], c["z"], c["labs"], *_initial(c, s.K), V, ALPHA0, BETA0)
    for i in range(4):
        old.sweep(1, SEED, i, threads=4)
    assert not np.array_equal(old.z, cs.z)
    off = c["doc_off"]
    st = types.SimpleNamespace(n_k_v=cs.n_k_v, n_d_k=cs.n_d_k, n_zk=cs.n_zk, labs=c["labs"].astype(np.float64), V=V, alpha=est.alpha,
                               beta=est.beta, docs=[c["word"][off[d]:off[d + 1]].tolist() for d in range(len(c["lens"]))])
    np.testing.assert_array_equal(s.theta().cpu().numpy(), orc.get_theta(st))
    np.testing.assert_array_equal(s.phi().cpu().numpy(), orc.get_phi(st))
    assert abs(s.perplexity() / orc.perplexity(st) - 1) < 1e-9
    torch.cuda.synchronize()


def _initial(c, K):
    import longdocs as L
    return L.initial_counts(c, K)


# ------------------------------------------------------------------------------------------------ the drop-in class
def evidence_alpha(alpha, labs, n_d_k):
    labs = np.asarray(labs) != 0
    return (math.fsum(math.lgamma(a * alpha) - math.lgamma(n + a * alpha) for a, n in zip(labs.sum(axis=1), n_d_k.sum(axis=1)))
            + math.fsum(math.lgamma(n + alpha) - math.lgamma(alpha) for n in n_d_k[labs]))


def evidence_beta(beta, n_k_v):
    W = n_k_v.shape[1]
    return (math.fsum(math.lgamma(W * beta) - math.lgamma(n + W * beta) for n in n_k_v.sum(axis=1))
            + math.fsum(math.lgamma(n + beta) - math.lgamma(beta) for n in n_k_v.ravel()))


def test_labeledlda_optimize_priors_on_a_golden_corpus():
    from fixture_corpora import tiny_corpus
    from lda_thesis_amd.foldin import TEST_STREAM, fold_in
    from test_gpu_dropin import build_model
    m, _, _ = build_model("k40")
    a0, b0 = m.alpha, m.beta
    m.run_training(4, 2)
    n_d_k, n_k_v, n_zk = m.n_d_k, m.n_k_v, m.n_zk
    want = host_estimate(a0, b0, n_d_k, n_k_v, n_zk, m.labs)
    pair = m.optimize_priors()
    assert pair == (want.alpha, want.beta) == (m.alpha, m.beta) == (m._sampler.alpha, m._sampler.beta)
    assert want.converged and pair != (a0, b0)
    assert evidence_alpha(pair[0], m.labs, n_d_k) >= evidence_alpha(a0, m.labs, n_d_k)
    assert evidence_beta(pair[1], n_k_v) >= evidence_beta(b0, n_k_v)
    # one prior at a time
    m1, _, _ = build_model("k40")
    m1.run_training(4, 2)
    assert m1.optimize_priors(beta=False) == (want.alpha, b0) and m1.optimize_priors(alpha=False) == (want.alpha, want.beta)
    # fold-in takes the new alpha
    docs = tiny_corpus("k40")[0][:5]
    th = m.run_test(docs, 6, 2)
    tups = [m.dicti.doc2bow(x) for x in docs]
    np.testing.assert_array_equal(th, fold_in(m.ph_hat, pair[0], tups, 6, 2, m.seed, TEST_STREAM)["th_hat"])
    assert not np.array_equal(th, fold_in(m.ph_hat, a0, tups, 6, 2, m.seed, TEST_STREAM)["th_hat"])
    # a pickle round trip keeps the priors and continues identically
    m2 = pickle.loads(pickle.dumps(m))
    assert (m2.alpha, m2.beta) == pair == (m2._sampler.alpha, m2._sampler.beta)
    for _ in range(2):
        m.training_iteration()
        m2.training_iteration()
    np.testing.assert_array_equal(np.concatenate(m.z_dn), np.concatenate(m2.z_dn))
    np.testing.assert_array_equal(m.n_k_v, m2.n_k_v)
    np.testing.assert_array_equal(m.get_theta(), m2.get_theta())
    assert m.perplexity() == m2.perplexity()


def test_run_training_prior_trace_and_inert_default(capsys):
    from conftest import load_golden
    from test_gpu_dropin import build_model
    m, _, _ = build_model("k12")
    a0, b0 = m.alpha, m.beta
    m.run_training(12, 4, optimize_interval=3, optimize_burn_in=3)
    assert [t[0] for t in m.prior_trace] == [6, 9, 12]
    assert m.prior_trace[-1][1:] == (m.alpha, m.beta) == (m._sampler.alpha, m._sampler.beta) and (m.alpha, m.beta) != (a0, b0)
    assert len(m.cur_perplx) == 3 and all(np.isfinite(m.cur_perplx))
    # the default: no prior ever changes, the chain is the one training_iteration() alone gives
    m2, _, _ = build_model("k12")
    m2.run_training(12, 4)
    m3, _, _ = build_model("k12")
    for _ in range(12):
        m3.training_iteration()
    assert m2.prior_trace == [] and (m2.alpha, m2.beta) == (a0, b0) == (m2._sampler.alpha, m2._sampler.beta)
    np.testing.assert_array_equal(np.concatenate(m2.z_dn), np.concatenate(m3.z_dn))
    np.testing.assert_array_equal(m2.n_k_v, m3.n_k_v)
    assert not np.array_equal(np.concatenate(m.z_dn), np.concatenate(m2.z_dn))
    # ... and the reference's golden run, with the new keywords left at their defaults
    g = load_golden("runtraining_k12")
    m4, _, _ = build_model("k12", seed=int(g["seed"]))
    m4.run_training(int(g["iters"]), int(g["thinning"]))
    np.testing.assert_array_equal(m4.ph_hat, g["ph_hat"])
    np.testing.assert_array_equal(m4.th_hat, g["th_hat"])


# ------------------------------------------------------------------------------------------------ several ranks on the one GPU
N_BINS_RANKS = 8          # (short histograms: overflow values on every rank that holds documents)


def _rank_worker(rank, world, port, empty_last, q):
    """sampler level: shards of tiny_k40, two sweeps, the histograms of all ranks, the estimate, two sweeps with it"""
    import torch.distributed as dist
    from test_distributed_gloo import _setup
    dev = _setup(rank, world, port, True) if world > 1 else "cuda:0"
    out = _sampler_run(rank, world, empty_last, dev)
    q.put((rank,) + out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _sampler_run(rank, world, empty_last, dev):
    from conftest import load_golden
    from lda_thesis_amd import priors
    from lda_thesis_amd.sampler import GibbsSampler, shard_documents
    g = load_golden("tiny_k40")
    off, D, K, W = g["doc_off"], int(g["D"]), int(g["K"]), int(g["V"])
    b = shard_documents(off, world)
    if empty_last:
        b = shard_documents(off, world - 1) + [D]
    lo, hi = b[rank], b[rank + 1]
    s0, s1 = int(off[lo]), int(off[hi])
    s = GibbsSampler(off[lo:hi + 1] - off[lo], g["word"][s0:s1], g["freq"][s0:s1], g["init_z"][s0:s1], K, W, float(g["alpha"]),
                     float(g["beta"]), labs=g["labs"][lo:hi], seed=int(g["seed"]), doc_base=lo, device=dev, commit_log=True)
    for _ in range(2):
        s.sweep()
    h = s.count_histograms(N_BINS_RANKS)
    pre = np.concatenate([[0], np.cumsum(g["freq"].astype(np.int64))])
    cls = priors.doc_classes(g["labs"].sum(axis=1), pre[off[1:]] - pre[off[:-1]])
    est = priors.estimate(s.alpha, s.beta, hist_dk=h[0], over_dk=h[1], classes=cls, hist_kw=h[2], over_kw=h[3], n_k=s.n_zk(), V=W)
    s.set_priors(est.alpha, est.beta)
    for _ in range(2):
        s.sweep()
    s.check_status()
    return (lo, hi), tuple(x.tolist() for x in h), (est.alpha, est.beta), s.z_topics(), s.n_d_k(), s.n_k_v(), s.n_zk()


def test_two_ranks_and_an_empty_one_estimate_what_one_process_estimates():
    from test_gpu_multirank import _spawn
    _, h1, pair1, z1, ndk1, nkv1, nzk1 = _sampler_run(0, 1, False, "cuda:0")
    assert len(h1[1]) > 0 and pair1 != (0.1, 0.01)
    res = sorted(_spawn(3, _rank_worker, (True,)), key=lambda r: r[0])
    assert res[2][1][0] == res[2][1][1]                         # the last rank holds no document
    for rank, (lo, hi), h, pair, z, ndk, nkv, nzk in res:
        assert h == h1, "rank %d: histograms" % rank
        assert pair == pair1, "rank %d: (alpha, beta)" % rank
        np.testing.assert_array_equal(nkv, nkv1)
        np.testing.assert_array_equal(nzk, nzk1)
    np.testing.assert_array_equal(np.concatenate([r[4] for r in res]), z1)
    np.testing.assert_array_equal(np.concatenate([r[5] for r in res]), ndk1)


def _llda_rank_worker(rank, world, port, q):
    """the drop-in class over two ranks: optimize_priors() is collective and every rank ends with rank 0's two doubles"""
    import torch.distributed as dist
    from test_distributed_gloo import _setup
    _setup(rank, world, port, True)
    q.put((rank,) + _llda_run())
    dist.barrier()
    dist.destroy_process_group()


def _llda_run():
    from test_gpu_dropin import build_model
    m, _, _ = build_model("k40")
    for _ in range(2):
        m.training_iteration()
    pair = m.optimize_priors()
    for _ in range(2):
        m.training_iteration()
    return pair, (m._sampler.alpha, m._sampler.beta), m._sampler.D, np.concatenate(m.z_dn), m.n_d_k, m.n_k_v, m.n_zk, m.perplexity()


def test_labeledlda_optimize_priors_over_two_ranks():
    from test_gpu_multirank import _spawn
    pair1, _, D1, z1, ndk1, nkv1, nzk1, perp1 = _llda_run()
    res = _spawn(2, _llda_rank_worker, ())
    assert sum(r[3] for r in res) == D1 and all(0 < r[3] < D1 for r in res)
    for rank, pair, held, _, z, ndk, nkv, nzk, perp in res:
        assert pair == pair1 == held, "rank %d" % rank
        np.testing.assert_array_equal(z, z1)
        np.testing.assert_array_equal(ndk, ndk1)
        np.testing.assert_array_equal(nkv, nkv1)
        np.testing.assert_array_equal(nzk, nzk1)
        assert abs(perp / perp1 - 1) < 1e-12
