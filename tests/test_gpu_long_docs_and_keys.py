"""Every sweep and fold-in kernel family on LONG documents and under FULL-WIDTH draw keys, bit for bit against the oracles.

Long documents (tests/longdocs.py: documents of 0, 1, 2, 7, 64 and 300 sites next to documents of 3 000 ... 60 000 sites, token
totals exactly on 2^15 - 1 / 2^15 / 2^16 - 1 / 2^16 reached by site count): the per-document site loops far past their prologue --
the quad kernel's FULL trio loop and its uniform table refills, the sparse-label kernel's batches of eight, the wide kernels' int16
changes, the fold-in's cyclic pipeline.  Every case asserts which kernel it ran, and that most sites of the long documents moved.

Draw keys: (seed u64; sweep u32, stream u32, doc u32, site).  The long-document cases already run under a wide key
(longdocs.LONG_KEY); the key cases run every family on a small corpus whose documents pass Philox block 256 under each setting of
longdocs.KEYS -- seeds with a high word (and one with ONLY a high word), streams with bit 31 set, sweep numbers across 2^16, 2^31
and up to 2^32 - 1, document ids that cross 2^31 and wrap at 2^32 inside the shard.  tests/test_long_docs_inputs.py shows on the
CPU that a kernel which dropped any of these bits would leave a different z on these inputs.

All comparisons are exact equality of integer state (and of th_hat for the fold-in)."""
import numpy as np
import pytest

import longdocs as L

pytestmark = pytest.mark.gpu


def _assert_equal(s, cs, what):
    np.testing.assert_array_equal(s.z_topics(), cs.z, err_msg="z " + what)
    np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k, err_msg="n_d_k " + what)
    np.testing.assert_array_equal(s.n_zk(), cs.n_zk, err_msg="n_zk " + what)
    np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v, err_msg="n_k_v " + what)


def _sweeps_vs_oracle(co, c, K, key, sweeps, margin, ran, moved=True, **kw):
    """``sweeps`` sweeps of a GibbsSampler on corpus ``c`` under the draw key ``key`` = (seed, stream, first sweep, doc_base)
    against the C oracle given the same words; ``ran(s)`` asserts the kernel the sampler takes, before and after."""
    from lda_thesis_amd.sampler import GibbsSampler
    seed, stream, sweep0, doc_base = key
    s = GibbsSampler(c["doc_off"], c["word"], c["freq"], c["z"], K, c["V"], c["alpha"], c["beta"], labs=c["labs"], seed=seed,
                     stream_id=stream, doc_base=doc_base, **kw)
    s.sweeps_done = sweep0
    s.debug_margin = margin
    ran(s)
    cs = co.CState(c["doc_off"], c["word"], c["freq"], c["z"], c["labs"], s.n_d_k(), s.n_k_v(), s.n_zk(), c["V"], c["alpha"],
                   c["beta"])
    for i in range(sweeps):
        s.sweep()
        cs.sweep(1, seed, sweep0 + i, stream=stream, doc_base=doc_base, threads=8)
        _assert_equal(s, cs, "after sweep %d (sweep word %d)" % (i + 1, sweep0 + i))
        if moved and i == 0:
            # a site redraws among at least 8 allowed topics from a start that is uniform over them: it stays with a probability of
            # about an eighth -- "most moved" is more than half
            assert L.share_moved(c, c["z"], cs.z) > 0.5
    s.check_status()
    assert s.sweeps_done == sweep0 + sweeps
    ran(s)
    return s


# ------------------------------------------------------------------------------------------------
# which kernel a sampler takes (csrc/llda_gibbs.hip: llda_sweep)
# ------------------------------------------------------------------------------------------------
def ran_quad(s):
    assert s.quad and s.dense_mask and s.n_kw16 is not None and s.row16 is not None and s.commit_log is not None
    assert not s.layout.wide and s.live_off is None and 0 < s.max_doc_tokens < 65536


def ran_two_doc(four_waves):
    def ran(s):
        assert not s.quad and s.dense_mask and s.n_kw16 is not None and s.site_row is not None and s.commit_log is not None
        assert not s.layout.wide and s.live_off is None
        assert (s.max_doc_tokens == 65535) if four_waves else (s.max_doc_tokens == 65536)
    return ran


def ran_general(dense, logged):
    def ran(s):
        assert not s.quad and s.n_kw16 is None and s.row16 is None and not s.layout.wide and s.live_off is None
        assert s.dense_mask == dense and (s.commit_log is not None) == logged and s.n_kw_img is None
    return ran


def ran_sparse(image, wide):
    def ran(s):
        import torch
        assert s.live_off is not None and s.live_max == 8 and s._heavy is None and not s.dense_mask and not s.quad
        assert s.layout.wide == wide and s.n_kw16 is None
        assert (s.n_kw_img is None) if image == 0 else (s.n_kw_img.dtype == {8: torch.uint8, 16: torch.int16}[image])
    return ran


def ran_wide_dense(tokens):
    def ran(s):
        assert s.layout.wide and s.live_off is None and s.dense_mask and s.max_doc_tokens == tokens and s._scratch is not None
    return ran


# ------------------------------------------------------------------------------------------------
# 2. long documents
# ------------------------------------------------------------------------------------------------
MARGINS = [0, -1]         # production margins; every site through the exact tier


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("sort_docs", [False, True])
@pytest.mark.parametrize("K", [512, 256, 128, 400])
def test_long_documents_quad_kernel(c_oracle, K, sort_docs, margin):
    """four / eight / sixteen documents per wavefront, the largest document at 65 535 tokens from 60 000 sites; in corpus order a
    document of one site shares its wavefront with it"""
    c = L.thesis_corpus(K, top_tokens=65535)
    assert c["tokens"].max() == 65535
    _sweeps_vs_oracle(c_oracle, c, K, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_quad, commit_log=True, quad=True, sort_docs=sort_docs)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("K", [512, 256])
def test_long_documents_leave_the_quad_kernel_at_65536_tokens(c_oracle, K, margin):
    """one token more in the largest document: the sampler (quad left to it) takes the two-document kernel in its three-wave form at
    K = 512 and the general kernel at K = 256, and the state still equals the oracle's"""
    c = L.thesis_corpus(K, top_tokens=65536)
    assert c["tokens"].max() == 65536 and 65535 in c["tokens"]
    ran = ran_two_doc(four_waves=False) if K == 512 else ran_general(dense=True, logged=True)
    _sweeps_vs_oracle(c_oracle, c, K, L.LONG_KEY, L.LONG_SWEEPS, margin, ran, commit_log=True, quad=None, rows16=True)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("top", [65535, 65536])
@pytest.mark.parametrize("K", [512, 1024])
def test_long_documents_two_document_kernel_on_16_bit_rows(c_oracle, K, top, margin):
    """four waves per SIMD (n_dk packed with its sweep-start value) with every document below 2^16 tokens, three at 2^16"""
    c = L.thesis_corpus(K, top_tokens=top)
    _sweeps_vs_oracle(c_oracle, c, K, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_two_doc(four_waves=top == 65535), commit_log=True,
                      quad=False, rows16=True)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("commit_log", [True, False])
@pytest.mark.parametrize("K,labels", [(392, "dense"), (40, "heavy")])
def test_long_documents_general_kernel(c_oracle, K, labels, commit_log, margin):
    """llda_sweep_kernel with int32 rows: dense at K = 392 and with label masks at K = 40 (label sets too heavy for the sparse-label
    kernel), the largest document beyond 2^16 tokens"""
    c = L.thesis_corpus(K, labels=labels, top_tokens=65536)
    _sweeps_vs_oracle(c_oracle, c, K, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_general(labels == "dense", commit_log),
                      commit_log=commit_log, quad=False, rows16=False)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("image", [0, 8, 16])
@pytest.mark.parametrize("K", [392, 512])
def test_long_documents_sparse_label_kernel(c_oracle, K, image, margin):
    """at most 8 allowed topics per document (8 in the long ones): eight documents per wavefront, batches of eight sites"""
    c = L.thesis_corpus(K, labels="sparse", top_tokens=65536)
    _sweeps_vs_oracle(c_oracle, c, K, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_sparse(image, wide=False), image=image)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("top", [32767, 32768])
def test_long_documents_wide_dense_kernel(c_oracle, top, margin):
    """K = 2 048: int16 count changes in LDS while every document is below 2^15 tokens, full-width counts from 2^15 on"""
    c = L.thesis_corpus(2048, kind="wide", top_tokens=top)
    assert c["tokens"].max() == top
    _sweeps_vs_oracle(c_oracle, c, 2048, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_wide_dense(top))


@pytest.mark.parametrize("margin", MARGINS)
def test_long_documents_wide_sparse_kernel(c_oracle, margin):
    c = L.thesis_corpus(1031, labels="sparse", kind="wide", top_tokens=32768)
    _sweeps_vs_oracle(c_oracle, c, 1031, L.LONG_KEY, L.LONG_SWEEPS, margin, ran_sparse(0, wide=True))


# ------------------------------------------------------------------------------------------------
# llda_sweep_batch: an ensemble of sub-problems over one corpus, batched against one by one
# ------------------------------------------------------------------------------------------------
def _ensemble_plans(c, rng):
    """four sub-problems over the documents of ``c`` that have sites; label sets of 4 .. 5, 9 .. 15, 17 .. 32 and 33 .. 64 topics:
    one launch of llda_sweep_batch per class of lanes (8, 16, 32, 64).  One by one, the second and the third run through the
    sparse-label kernel (16 and 32 lanes) and the others, whose label sets are heavy for their K, through the general kernel."""
    have = np.flatnonzero(c["lens"] > 0)
    plans, z_local = [], []
    for K, lo, hi, docs in ((5, 4, 5, have), (60, 9, 15, have[::2]), (128, 17, 32, have[1::2]), (100, 33, 64, have)):
        allowed = np.full((len(docs), hi), -1, dtype=np.int64)
        n_allowed = rng.integers(lo, hi + 1, size=len(docs))
        zs = []
        for r, d in enumerate(docs):
            a = np.sort(rng.choice(K, size=int(n_allowed[r]), replace=False))
            allowed[r, :len(a)] = a
            zs.append(a[rng.integers(0, len(a), size=int(c["lens"][d]))])
        plans.append(dict(K=K, docs=docs.astype(np.int64), allowed=allowed, n_allowed=n_allowed.astype(np.int64)))
        z_local.append(np.concatenate(zs).astype(np.int64))
    return plans, z_local


def _batched_vs_one_by_one(co, c, seed, sweep0, sweeps, margin, moved):
    """Ensemble.sweep (llda_sweep_batch) against one GibbsSampler per sub-problem (llda_sweep, SubLDA's construction: the stream
    is the index of the sub-problem, the documents count from 0, phantom columns added) -- and that one against the C oracle"""
    from lda_thesis_amd.ensemble import Ensemble
    from lda_thesis_amd.sampler import GibbsSampler
    rng = np.random.default_rng(77)
    plans, z_local = _ensemble_plans(c, rng)
    off, V, alpha, beta = c["doc_off"], c["V"], c["alpha"], c["beta"]
    assert int(c["freq"].max()) < V                       # (the phantom column of a site is its frequency)
    ens = Ensemble(plans, z_local, off, c["word"], c["freq"], V, alpha, beta, seed)
    assert [g for g, _ in ens.orders] == [8, 16, 32, 64]
    ens.sweeps_done = sweep0
    ens.debug_margin = margin
    subs = []
    for i, pl in enumerate(plans):
        sites = np.concatenate([np.arange(off[d], off[d + 1]) for d in pl["docs"]])
        lens = c["lens"][pl["docs"]]
        sub_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        w, f = c["word"][sites], c["freq"][sites]
        labs = np.zeros((len(pl["docs"]), pl["K"]), dtype=np.uint8)
        for r in range(len(pl["docs"])):
            labs[r, pl["allowed"][r, :pl["n_allowed"][r]]] = 1
        s = GibbsSampler(sub_off, w, f, z_local[i], pl["K"], V, alpha, beta, labs=labs, seed=seed, stream_id=i, sharded=False)
        ghost = f != w
        s.add_word_topic_counts(f[ghost], z_local[i][ghost], f[ghost])
        s.sweeps_done = sweep0
        s.debug_margin = margin
        cs = co.CState(sub_off, w, f, z_local[i], labs, s.n_d_k(), s.n_k_v(), s.n_zk(), V, alpha, beta)
        n_k_v, n_d_k, n_zk, z = ens.problem_state(i)       # the same start, phantom columns included
        np.testing.assert_array_equal(n_k_v, cs.n_k_v)
        np.testing.assert_array_equal(z, z_local[i])
        subs.append((s, cs, dict(lens=lens)))
    for j in range(sweeps):
        ens.sweep()
        for i, (s, cs, sub) in enumerate(subs):
            s.sweep()
            cs.sweep(1, seed, sweep0 + j, stream=i, doc_base=0, threads=4)
            what = "sub-problem %d after sweep %d" % (i, j + 1)
            _assert_equal(s, cs, what)
            n_k_v, n_d_k, n_zk, z = ens.problem_state(i)
            np.testing.assert_array_equal(z, cs.z, err_msg="batched z " + what)
            np.testing.assert_array_equal(n_d_k, cs.n_d_k, err_msg="batched n_d_k " + what)
            np.testing.assert_array_equal(n_zk, cs.n_zk, err_msg="batched n_zk " + what)
            np.testing.assert_array_equal(n_k_v, cs.n_k_v, err_msg="batched n_k_v " + what)
            if moved and j == 0:
                assert L.share_moved(sub, z_local[i], z) > 0.5            # (at least 4 allowed topics: a site stays about 1 in 4)
    ens.check_status()
    for s, _, _ in subs:
        s.check_status()
    if margin == -1:
        assert int(ens.status[2]) > 0                       # sites went through the exact pipeline inside the batched kernel
    return ens


@pytest.mark.parametrize("margin", MARGINS)
def test_long_documents_batched_ensemble_equals_one_by_one(c_oracle, margin):
    """sub-problems that hold documents of 3 000 ... 5 000 sites"""
    c = L.thesis_corpus(8, kind="wide", top_tokens=32768)
    seed, _, sweep0, _ = L.LONG_KEY
    ens = _batched_vs_one_by_one(c_oracle, c, seed, sweep0, L.LONG_SWEEPS, margin, moved=True)
    assert int(np.diff(ens._inst_off_h).max()) == 5000


# ------------------------------------------------------------------------------------------------
# fold-in
# ------------------------------------------------------------------------------------------------
def _loadings(rng, K, V, zeros):
    ph = rng.random((K, V)) ** 3
    if zeros:
        ph[rng.random((K, V)) < zeros] = 0.0
    ph[0] += 1e-6                                           # (no word without a loading: LabeledLDA.run_test divides 0 by 0 there)
    return ph / ph.sum(axis=1, keepdims=True)


def _held_out(rng, V, lens):
    tups = []
    for n in lens:
        ids = np.sort(rng.choice(V, size=n, replace=False)).tolist()
        tups.append(list(zip(ids, rng.integers(1, 4, size=n).tolist())))
    return tups


def _same_result(a, b):
    np.testing.assert_array_equal(a["th_hat"], b["th_hat"])
    np.testing.assert_array_equal(a["n_dk"], b["n_dk"])
    for x, y in zip(a["z"], b["z"]):
        np.testing.assert_array_equal(x, y)


def _exact_only(fn):
    import lda_thesis_amd.foldin as F
    F.EXACT_ONLY = True
    try:
        return fn()
    finally:
        F.EXACT_ONLY = False


def _fold_in_case(K, V, lens, seed, stream, doc_base, it=2):
    """LabeledLDA's fold-in (llda_foldin) against oracle/llda_oracle.run_test, and against itself with every site through the
    reference's pipeline"""
    import llda_oracle as orc
    from lda_thesis_amd.foldin import fold_in
    rng = np.random.default_rng(K + V)
    ph = _loadings(rng, K, V, 0.2)
    tups = _held_out(rng, V, lens)
    got = fold_in(ph, 0.3, tups, it, 1, seed, stream_id=stream, doc_base=doc_base)
    want = orc.run_test(ph, 0.3, [[v for v, _ in t] for t in tups], [[f for _, f in t] for t in tups], it, 1,
                        orc.keyed_draw_for(seed, stream, doc_base=doc_base))
    np.testing.assert_array_equal(got["th_hat"], want)
    assert (got["n_dk"].sum(1) == [sum(f for _, f in t) for t in tups]).all()
    _same_result(got, _exact_only(lambda: fold_in(ph, 0.3, tups, it, 1, seed, stream_id=stream, doc_base=doc_base)))
    return got, tups


def _cascade_fold_in_case(K, V, lens, seed, stream, doc_base, it=2, oracle=True):
    """CascadeLDA's fold-in on a label subset against oracle/llda_oracle.cascade_test (``oracle``), and against itself with every
    site through the reference's pipeline"""
    import llda_oracle as orc
    from lda_thesis_amd.foldin import cascade_fold_in
    rng = np.random.default_rng(K + V + 1)
    ph = _loadings(rng, K, V, 0.6)
    tups = _held_out(rng, V, lens)
    ids = np.arange(len(tups), dtype=np.int64) + doc_base
    got = cascade_fold_in(ph, 0.2, 0.01, tups, it, 1, seed, stream, ids)
    if oracle:
        for d, tup in enumerate(tups):
            w, f = zip(*tup)

            def draw_for_sweep(sw, d=d):
                k = orc.KeyedDraw(seed, stream)
                k.sweep, k.doc, k.site = sw, int(ids[d]) & 0xFFFFFFFF, 0
                return k
            want = orc.cascade_test(ph, 0.2, 0.01, list(w), list(f), it, 1, draw_for_sweep)
            np.testing.assert_array_equal(got["th_hat"][d], want, err_msg="doc %d" % d)
    _same_result(got, _exact_only(lambda: cascade_fold_in(ph, 0.2, 0.01, tups, it, 1, seed, stream, ids)))
    return got, tups


HELD_OUT = [1, 3000, 2, 5000]          # sites per held-out document; ids 2^32 - 2, 2^32 - 1, 0, 1
HELD_OUT_WIDE = [1, 2, 3000]           # (the wide kernels run one wavefront per document, every site through the exact pipeline once)


def _most_moved(run, two, lens):
    """most sites of the long documents change their topic from the first sweep of the fold-in to the second: the same key gives
    the same first sweep, so one sweep and two sweeps differ by what the second one moved (a site redraws among the topics that
    load on its word, dozens here, with n_dk spread over all of them: it stays far less often than every second time)"""
    one = run(1)                                           # (``two``: the result of the same call with two sweeps)
    for d, n in enumerate(lens):
        if n >= L.LONG:
            assert float((one["z"][d] != two["z"][d]).mean()) > 0.5


def _cascade_moved(K, tups, got, lens=HELD_OUT):
    from lda_thesis_amd.foldin import cascade_fold_in
    ph = _loadings(np.random.default_rng(K + 5200 + 1), K, 5200, 0.6)
    ids = np.arange(len(tups), dtype=np.int64) + 2 ** 32 - 2
    _most_moved(lambda it: cascade_fold_in(ph, 0.2, 0.01, tups, it, 1, L.SEEDS[0], 0xC0DE0123, ids), got, lens)


def test_long_documents_fold_in():
    from lda_thesis_amd.foldin import fold_in
    got, tups = _fold_in_case(130, 5200, HELD_OUT, L.SEEDS[0], 0xC0DE0123, 2 ** 32 - 2)
    assert max(len(t) for t in tups) == 5000
    ph = _loadings(np.random.default_rng(130 + 5200), 130, 5200, 0.2)
    _most_moved(lambda it: fold_in(ph, 0.3, tups, it, 1, L.SEEDS[0], stream_id=0xC0DE0123, doc_base=2 ** 32 - 2), got, HELD_OUT)


def test_long_documents_cascade_fold_in():
    got, tups = _cascade_fold_in_case(40, 5200, HELD_OUT, L.SEEDS[0], 0xC0DE0123, 2 ** 32 - 2)
    assert max(len(t) for t in tups) == 5000
    _cascade_moved(40, tups, got)


def test_long_documents_wide_fold_in_against_itself():
    """K = 1 031 (the wide fold-in kernels): the decided tier against the reference's pipeline on the device only -- the numpy oracle
    is a Python loop per site that takes about 2 ms a site at 1 031 topics; it pins the same kernels on short documents in
    test_gpu_dropin.py and on 601 sites in test_draw_key_fold_in below"""
    got, tups = _cascade_fold_in_case(1031, 5200, HELD_OUT_WIDE, L.SEEDS[0], 0xC0DE0123, 2 ** 32 - 2, oracle=False)
    _cascade_moved(1031, tups, got, HELD_OUT_WIDE)


# ------------------------------------------------------------------------------------------------
# 3. full-width draw keys, every family, small corpus
# ------------------------------------------------------------------------------------------------
KEY_IDS = ["seed_9E37_sweep_65535_docs_cross_2p31", "seed_all_ones_stream_all_ones_sweep_2p31", "seed_2p32_sweep_to_2p32m1_docs_wrap"]


def ran_two_doc_small(s):
    assert not s.quad and s.n_kw16 is not None and s.site_row is not None and 0 < s.max_doc_tokens < 65536 and s.dense_mask


def ran_wide_small(s):
    assert s.layout.wide and s.live_off is None and s.dense_mask and 0 < s.max_doc_tokens < 32768


# family: (K, label pattern, sampler arguments, the kernel it must take)
FAMILIES = {
    "quad512": (512, "dense", dict(commit_log=True, quad=True, sort_docs=False), ran_quad),
    "quad256": (256, "dense", dict(commit_log=True, quad=True), ran_quad),
    "quad128": (128, "dense", dict(commit_log=True, quad=True, sort_docs=False), ran_quad),
    "quad400": (400, "dense", dict(commit_log=True, quad=True), ran_quad),
    "two_doc512": (512, "dense", dict(commit_log=True, quad=False, rows16=True), ran_two_doc_small),
    "two_doc1024": (1024, "dense", dict(commit_log=True, quad=False, rows16=True), ran_two_doc_small),
    "general392": (392, "dense", dict(commit_log=True, quad=False, rows16=False), ran_general(True, True)),
    "general40_masks": (40, "heavy", dict(commit_log=False), ran_general(False, False)),
    "sparse392": (392, "sparse", dict(image=0), ran_sparse(0, False)),
    "sparse512_image8": (512, "sparse", dict(image=8), ran_sparse(8, False)),
    "wide2048": (2048, "dense", dict(), ran_wide_small),
    "wide_sparse1031": (1031, "sparse", dict(), ran_sparse(0, True)),
}


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("key", range(len(L.KEYS)), ids=KEY_IDS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_draw_key_sweep_kernels(c_oracle, family, key, margin):
    K, labels, kw, ran = FAMILIES[family]
    c = L.thesis_corpus(K, labels=labels, kind="keys")
    assert (c["lens"] >= 600).sum() >= 4
    _sweeps_vs_oracle(c_oracle, c, K, L.KEYS[key], L.KEY_SWEEPS, margin, ran, moved=False, **kw)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("key", range(len(L.KEYS)), ids=KEY_IDS)
def test_draw_key_batched_ensemble(c_oracle, key, margin):
    """llda_sweep_batch takes the seed and the sweep from the settings; its stream (index of the sub-problem) and document words
    (index inside the sub-problem) are small by construction"""
    c = L.thesis_corpus(8, kind="keys")
    seed, _, sweep0, _ = L.KEYS[key]
    _batched_vs_one_by_one(c_oracle, c, seed, sweep0, L.KEY_SWEEPS, margin, moved=False)


@pytest.mark.parametrize("seed", L.SEEDS, ids=["seed_9E37", "seed_all_ones", "seed_2p32"])
@pytest.mark.parametrize("kernel", ["labeled", "cascade", "wide"])
def test_draw_key_fold_in(kernel, seed):
    """the fold-in kernels take the seed: narrow (LabeledLDA's and CascadeLDA's) and wide, documents of 601 to 700 sites, against
    the numpy oracle"""
    lens = [1, 700, 2, 650]
    if kernel == "labeled":
        _fold_in_case(40, 800, lens, seed, 0xFFFFFFFF, 2 ** 31 - 2)
    elif kernel == "cascade":
        _cascade_fold_in_case(12, 800, lens, seed, 0xC0DE0123, 2 ** 32 - 2)
    else:
        _cascade_fold_in_case(1031, 800, [2, 601], seed, 0xC0DE0123, 2 ** 32 - 1)
