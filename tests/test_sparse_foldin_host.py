"""llda_foldin_sparse without a GPU: the CPU restatement (tests/sparsefoldinref.py) against tests/foldinref.py on every document's
compacted problem, the entry point's exports, struct size and refusals, and the Python argument errors of foldin.fold_in_sparse and
of the LabeledLDA keywords that stand on it (with the kernels replaced by the restatements)."""
import ctypes

import numpy as np
import pytest

import foldinref
import sparsefoldinref as sfr
import sparseheldref
import sparseref

BAD_K, BAD_ARG = -1, -2
MAX_K = 7688
SEED, STREAM = 0x5EEDF00DCAFE, 0x7E57


@pytest.fixture(scope="module")
def nat():
    from lda_thesis_amd import _native
    _native.lib()
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the restatement ----
def toy(seed, K=40, V=60, lists=(1, 5, 7, 8, 9, 17, 32, 3), lens=(4, 9, 1, 17, 6, 5, 33, 0)):
    rng = np.random.default_rng(seed)
    phi_t = rng.gamma(0.3, size=(V, K)) ** 3 + 1e-12
    phi_t[rng.random((V, K)) < 0.3] = 0.0
    phi_t[:, 0] = rng.random(V) + 0.01                                   # label 0 loads on every word ...
    phi_t[V - 1] = 0.0                                                   # ... but the last, which loads on nothing
    labs = [[0] + sorted(rng.choice(np.arange(1, K), size=L - 1, replace=False).tolist()) for L in lists]
    lab_off, lab = np.concatenate([[0], np.cumsum(lists)]).astype(np.int64), np.concatenate(labs).astype(np.int32)
    word = np.concatenate([rng.integers(0, V - 1, size=n) for n in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    freq = rng.integers(1, 6, size=word.shape[0]).astype(np.int32)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return dict(phi_t=phi_t, doc_off=doc_off, word=word, freq=freq, lab_off=lab_off, lab=lab, K=K, V=V)


def compacted(c, d, iters, thinning, alpha, doc_id):
    """foldinref.fold_in on document d's compacted problem, its init rows by the port of fold_in's preparation"""
    b, e = int(c["doc_off"][d]), int(c["doc_off"][d + 1])
    ids = c["lab"][int(c["lab_off"][d]):int(c["lab_off"][d + 1])].astype(np.int64)
    sub = np.ascontiguousarray(c["phi_t"][:, ids].T)                     # ph' (L_d, V)
    rows, bad = sfr.prepared_rows(sub)
    w = c["word"][b:e]
    idx = np.full(e - b, c["V"]) if bad[w].any() else w
    return foldinref.fold_in(init_rows=rows, init_idx=idx, ph=sub, doc_off=np.array([0, e - b]), word=w, freq=c["freq"][b:e], alpha=alpha,
                             beta=0.0, c_init=sfr.C_INIT, c_loop=sfr.C_LOOP, beta_fallback=False, avg_mode=0, iters=iters,
                             thinning=thinning, seed=SEED, doc_ids=[doc_id], doc_streams=[STREAM])


@pytest.mark.parametrize("iters,thinning", [(5, 2), (0, 1), (2, 3)])
def test_restatement_is_foldinref_on_every_compacted_problem(iters, thinning):
    c = toy(1)
    c["word"][5] = c["V"] - 1                                            # document 1 holds the word that loads on nothing
    ids = np.array([7, 2 ** 32 + 3, 0, 5, 2 ** 31, 9, 1, 4])
    got = sfr.fold_in_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], 0.1, iters, thinning, SEED, STREAM,
                                 doc_ids=ids)
    D = len(ids)
    # the word that loads on nothing: a uniform start (no raise with no sweep), a raise in the first sweep
    np.testing.assert_array_equal(got["raises"], [d == 1 and iters > 0 for d in range(D)])
    assert got["status"] == (1 if iters > 0 else 0)
    for d in range(D):
        want = compacted(c, d, iters, thinning, 0.1, ids[d])
        assert bool(want["raises"][0]) == bool(got["raises"][d])
        if got["raises"][d]:
            continue
        b, e, lb, le = (int(x) for x in (c["doc_off"][d], c["doc_off"][d + 1], c["lab_off"][d], c["lab_off"][d + 1]))
        np.testing.assert_array_equal(got["z"][b:e], want["z"])
        np.testing.assert_array_equal(got["n_dk_s"][lb:le], want["n_dk"][0])
        np.testing.assert_array_equal(bits(got["th_s"][lb:le]), bits(want["th"][0]))
    assert not got["n_dk_s"][c["lab_off"][7]:].any() and not got["th_s"][c["lab_off"][7]:].any()      # the empty document
    if thinning > iters:
        fit = ~np.isnan(got["th_s"])
        assert not got["th_s"][fit].any()                                # no sweep reached a multiple of thinning


def test_restatement_uniform_start_is_observable():
    """iters = 0 leaves the start state: the document with the unnormalisable column draws from 1 / L_d at EVERY site"""
    c = toy(2)
    plain = sfr.fold_in_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], 0.1, 0, 1, SEED, STREAM)
    c["word"][5] = c["V"] - 1
    got = sfr.fold_in_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], 0.1, 0, 1, SEED, STREAM)
    b, e = int(c["doc_off"][1]), int(c["doc_off"][2])
    assert not np.array_equal(plain["z"][b:e], got["z"][b:e])            # (sites other than the replaced one moved too)
    assert np.array_equal(np.delete(plain["z"], np.arange(b, e)), np.delete(got["z"], np.arange(b, e)))
    import llda_oracle as orc
    L = int(c["lab_off"][2] - c["lab_off"][1])
    for n in range(e - b):
        u = float(orc.keyed_uniform(SEED, orc.SWEEP_INIT, STREAM, 1, n))
        assert got["z"][b + n] == orc.draw_keyed(np.full(L, 1 / L), u, orc.layout(L))


def test_restatement_unfit_documents_and_bad_words():
    c = toy(3)
    lab = c["lab"].copy()
    lo = c["lab_off"]
    lab[lo[1] + 2] = lab[lo[1] + 1]                                      # document 1: a label twice
    lab[lo[3] + 4] = c["K"]                                              # document 3: an id outside [0, K)
    word = c["word"].copy()
    b4 = int(c["doc_off"][4])
    word[b4 + 1], word[b4 + 3] = c["V"], -1                              # document 4: two bad words
    got = sfr.fold_in_sparse_ref(c["phi_t"], c["doc_off"], word, c["freq"], lo, lab, 0.1, 0, 1, SEED, STREAM, max_labels=17)
    assert got["status"] == 4 | 2 and not got["raises"].any()
    for d in (1, 3, 6):                                                  # (6: 32 labels > max_labels)
        assert (got["z"][c["doc_off"][d]:c["doc_off"][d + 1]] == -1).all()
        assert (got["n_dk_s"][lo[d]:lo[d + 1]] == sfr.ND_FILL).all() and np.isnan(got["th_s"][lo[d]:lo[d + 1]]).all()
    # the bad words: z = -1, no count, and the sites around them keep their numbers n -- the start state is a draw per site
    clean = sfr.fold_in_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["freq"], lo, c["lab"], 0.1, 0, 1, SEED, STREAM)
    z4, c4 = got["z"][b4:b4 + 6], clean["z"][b4:b4 + 6]
    assert z4[1] == -1 and z4[3] == -1 and np.array_equal(z4[[0, 2, 4, 5]], c4[[0, 2, 4, 5]])
    assert got["n_dk_s"][lo[4]:lo[5]].sum() == c["freq"][b4:b4 + 6][[0, 2, 4, 5]].sum()
    for d in (0, 2, 5):                                                  # the documents between them are untouched
        assert np.array_equal(got["z"][c["doc_off"][d]:c["doc_off"][d + 1]], clean["z"][c["doc_off"][d]:c["doc_off"][d + 1]])
    # L_d = 0: fit, every site raises
    empty = sfr.fold_in_sparse_ref(c["phi_t"], np.array([0, 2]), np.array([1, 2]), np.array([1, 1]), np.array([0, 0]), np.zeros(0, dtype=np.int32),
                                   0.1, 1, 1, SEED, STREAM, K=c["K"])
    assert empty["status"] == 1 and empty["raises"][0]


# ---- the C ABI ----
def test_symbols_and_struct(nat):
    from test_abi import declared_symbols
    L = nat.lib()
    assert L.llda_abi_version() == 22 == nat.ABI_VERSION                # additive: the ABI number stays
    for s in ("llda_foldin_sparse_struct_bytes", "llda_foldin_sparse"):
        assert s in nat.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_foldin_sparse_struct_bytes() == ctypes.sizeof(nat.LldaFoldinSparseArgs) == 184


def foldin_call(nat, **kw):
    a = nat.LldaFoldinSparseArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.doc_off, a.word, a.freq, a.phi_t, a.lab_off, a.lab, a.doc_ids = (4096 + 1024 * i for i in range(7))
    a.z, a.n_dk_s, a.th_s, a.status = (16384 + 1024 * i for i in range(4))
    a.D, a.V, a.K, a.ld_phi, a.NL, a.max_labels, a.iters, a.thinning = 2, 10, 8, 8, 6, 8, 3, 2
    a.alpha, a.c_init, a.c_loop = 0.1, 1.0000000005, 1.0000005
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_foldin_sparse(ctypes.byref(a), None)


def test_foldin_sparse_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it) or has nothing to do: D = 0"""
    call = lambda **kw: foldin_call(nat, **kw)
    assert call(D=0) == 0 and call(D=0, doc_off=None, word=None, freq=None, phi_t=None, lab_off=None, lab=None, z=None, n_dk_s=None, th_s=None) == 0
    assert nat.lib().llda_foldin_sparse(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaFoldinSparseArgs) + 8, D=0) == BAD_ARG
    assert call(struct_bytes=ctypes.sizeof(nat.LldaLeftrightSparseArgs), D=0) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_phi=MAX_K + 1, D=0) == BAD_K, K
    for K in (1, 9, 1024, 1025, 2048, MAX_K):                           # every K
        assert call(K=K, ld_phi=K, D=0) == 0, K
    assert call(D=-1) == BAD_ARG and call(NL=-1, D=0) == BAD_ARG and call(ld_phi=7, D=0) == BAD_ARG
    for V in (0, -1, 2 ** 31):
        assert call(V=V, D=0) == BAD_ARG, V
    for m in (0, -1, 33, 2 ** 31 - 1):
        assert call(max_labels=m, D=0) == BAD_ARG, m
    for m in (1, 8, 9, 16, 17, 32):
        assert call(max_labels=m, D=0) == 0, m
    assert call(iters=-1, D=0) == BAD_ARG and call(iters=0, D=0) == 0
    for t in (0, -1):
        assert call(thinning=t, D=0) == BAD_ARG, t
    assert call(thinning=2 ** 31 - 1, D=0) == 0
    for c in (1.0, 0.5, 0.0, -2.0, float("nan")):
        assert call(c_init=c, D=0) == BAD_ARG and call(c_loop=c, D=0) == BAD_ARG, c
    assert call(c_init=float("inf"), c_loop=1.0 + 2.0 ** -52, D=0) == 0
    assert call(alpha=float("nan"), D=0) == BAD_ARG and call(alpha=0.0, D=0) == 0
    for name in ("doc_off", "word", "freq", "phi_t", "lab_off", "lab", "z", "n_dk_s", "th_s"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("doc_off", "phi_t", "lab_off", "doc_ids", "th_s"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("word", "freq", "lab", "z", "n_dk_s", "status"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG               # V x ld leaves an int64


# ---- Python ----
def test_fold_in_sparse_argument_errors_come_before_the_device():
    import torch
    from lda_thesis_amd import foldin
    phi_t = torch.zeros((5, 40), dtype=torch.float64)
    doc = [[(0, 1), (3, 2)]]
    with pytest.raises(ValueError, match="33 labels"):
        foldin.fold_in_sparse(phi_t, 0.1, doc, [0, 33], np.arange(33), 2, 1, SEED)
    with pytest.raises(ValueError, match="ascend"):
        foldin.fold_in_sparse(phi_t, 0.1, doc, [0, 2], [3, 3], 2, 1, SEED)
    with pytest.raises(ValueError, match=r"\[0, K\)"):
        foldin.fold_in_sparse(phi_t, 0.1, doc, [0, 2], [3, 40], 2, 1, SEED)
    with pytest.raises(ValueError, match="offsets"):
        foldin.fold_in_sparse(phi_t, 0.1, doc, [0, 1, 2], [3, 4], 2, 1, SEED)
    with pytest.raises(ValueError, match="in-vocabulary"):
        foldin.fold_in_sparse(phi_t, 0.1, [[]], [0, 1], [3], 2, 1, SEED)
    for it, thinning in ((-1, 1), (2, 0)):
        with pytest.raises(ValueError, match="thinning"):
            foldin.fold_in_sparse(phi_t, 0.1, doc, [0, 1], [3], it, thinning, SEED)
    with pytest.raises(ValueError, match="phi_t"):
        foldin.fold_in_sparse(np.zeros((5, 40)), 0.1, doc, [0, 1], [3], 2, 1, SEED)


class Dicti(object):
    def __init__(self, words):
        self.token2id = {w: i for i, w in enumerate(words)}

    def doc2bow(self, doc):
        c = {}
        for w in doc:
            if w in self.token2id:
                c[self.token2id[w]] = c.get(self.token2id[w], 0) + 1
        return sorted(c.items())


@pytest.fixture
def model(monkeypatch):
    """a LabeledLDA that was never trained: six labels after the root, eleven words, phi_t fixed; the kernels behind the new keywords
    are the CPU restatements"""
    import torch
    from lda_thesis_amd import foldin, heldout
    from lda_thesis_amd.LabeledLDA import LabeledLDA
    rng = np.random.default_rng(78)
    K, V = 7, 11
    m = LabeledLDA.__new__(LabeledLDA)
    m.K, m.alpha, m.seed = K, 0.25, SEED
    m.labelmap = dict([("root", 0)] + [("l%d" % k, k) for k in range(1, K)])
    m.dicti = Dicti(["w%d" % v for v in range(V)])
    phi_t = rng.gamma(0.5, size=(V, K)) + 1e-3
    phi_t /= phi_t.sum(axis=0, keepdims=True)
    m._attr_device = lambda: torch.device("cpu")
    m._test_phi_t_device = lambda: torch.from_numpy(phi_t)
    calls = []

    def fold_in_sparse(phi, alpha, tups, lab_off, lab, it, thinning, seed, stream_id=foldin.TEST_STREAM, doc_base=0, keep_device=False):
        from lda_thesis_amd.corpus import csr_from_doc_tups
        calls.append("fold_in_sparse")
        doc_off, word, freq = csr_from_doc_tups(tups)
        r = sfr.fold_in_sparse_ref(phi.numpy(), doc_off, word, freq, lab_off, lab, alpha, it, thinning, seed, stream_id, doc_base=doc_base)
        assert keep_device and r["status"] == 0
        return torch.from_numpy(r["th_s"]), None, None

    def loglik_sparse(theta_s, phi, doc_off, word, freq, lab_off, lab, weighted=True):
        calls.append("loglik_sparse")
        return sparseheldref.loglik_sparse_ref(theta_s.numpy(), phi.numpy(), doc_off, word, freq if weighted else None, lab_off, lab)

    monkeypatch.setattr(foldin, "fold_in_sparse", fold_in_sparse)
    monkeypatch.setattr(heldout, "loglik_sparse", loglik_sparse)
    m.test_phi_t, m.test_calls = phi_t, calls
    return m


DOCS = [["w1", "w2", "w2", "w5", "w9", "nope"], ["w3"], ["w0", "w4", "w4", "w4", "w7", "w8", "w10"]]
CANDS = [["l2", "l5"], [], ["l6", "l1", "l3"]]


def _csr(tups):
    return (np.concatenate([[0], np.cumsum([len(t) for t in tups])]).astype(np.int64), np.array([w for t in tups for w, _ in t], dtype=np.int32),
            np.array([f for t in tups for _, f in t], dtype=np.int32))


def test_candidates_route_through_the_sparse_sampler(model):
    tups = [model.dicti.doc2bow(x) for x in DOCS]
    cols = [[0] + sorted(model.labelmap[x] for x in labs) for labs in CANDS]
    lab_off, lab = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64), np.concatenate(cols).astype(np.int32)
    want = sfr.fold_in_sparse_ref(model.test_phi_t, *_csr(tups), lab_off, lab, model.alpha, 6, 2, SEED, 0x7E57)
    th = model.run_test(DOCS, 6, 2, candidates=CANDS)
    assert th.shape == (3, model.K) and np.array_equal(bits(th), bits(sparseref.scatter(want["th_s"], lab_off, lab, model.K)))
    assert not np.signbit(th).any()
    # predict: the slots ranked by load descending, ties by label index; min(n, list) pairs per document
    pr = model.predict(DOCS, 6, 2, n=3, candidates=CANDS)
    names = list(model.labelmap.keys())
    for d, pairs in enumerate(pr):
        row = want["th_s"][lab_off[d]:lab_off[d + 1]]
        order = np.argsort(-row, kind="stable")[:3]
        assert [p[0] for p in pairs] == [names[cols[d][j]] for j in order] and [p[1] for p in pairs] == [row[j] for j in order]
    assert len(pr[1]) == 1 and len(pr[0]) == 3 and len(pr[2]) == 3
    assert model.test_calls == ["fold_in_sparse"] * 2


def test_heldout_perplexity_labels_route_and_argument_errors(model):
    from lda_thesis_amd import heldout
    docs, labels = DOCS + [["nope"], []], CANDS + [["l1"], ["l2"]]
    r = model.heldout_perplexity(docs, 4, 2, labels=labels)
    tups = [model.dicti.doc2bow(x) for x in DOCS]
    obs, sc = [t[0::2] for t in tups], [t[1::2] for t in tups]
    cols = [[0] + sorted(model.labelmap[x] for x in labs) for labs in CANDS]
    lab_off, lab = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64), np.concatenate(cols).astype(np.int32)
    th_s = sfr.fold_in_sparse_ref(model.test_phi_t, *_csr(obs), lab_off, lab, model.alpha, 4, 2, SEED, 0x7E57)["th_s"]
    theta_s = sparseheldref.smooth_slots_ref(th_s, heldout.observed_tokens(obs), lab_off, model.alpha)
    want = heldout.perplexity_from(*sparseheldref.loglik_sparse_ref(theta_s, model.test_phi_t, *_csr(sc), lab_off, lab))
    assert (r["loglik"], r["tokens"], r["documents"], r["skipped"]) == (want["loglik"], want["tokens"], 3, 2)
    assert model.test_calls == ["fold_in_sparse", "loglik_sparse"]
    with pytest.raises(ValueError):
        model.heldout_perplexity(docs, 4, 2, labels=labels[:-1])
    with pytest.raises(KeyError):
        model.heldout_perplexity(docs, 4, 2, labels=[["unknown"]] * 5)
    for f in (model.predict, lambda *a, **k: model.score_test(a[0], CANDS, *a[1:], **k)):
        with pytest.raises(ValueError, match="exclude"):
            f(DOCS, 4, 2, candidates=CANDS, shortlist=3)
        for m in (0, 17, -1):
            with pytest.raises(ValueError, match="shortlist"):
                f(DOCS, 4, 2, shortlist=m)
    with pytest.raises(ValueError):
        model.run_test(DOCS, 4, 2, candidates=CANDS[:-1])
    with pytest.raises(KeyError):
        model.run_test(DOCS, 4, 2, candidates=[["unknown"]] * 3)


def test_the_harness_takes_the_new_flag():
    from lda_thesis_amd import evaluate_LabeledLDA as E
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])[0].shortlist == 0
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--shortlist", "7"])[0].shortlist == 7
