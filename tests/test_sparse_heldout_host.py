"""llda_heldout_loglik_sparse and llda_left_to_right_sparse without a GPU: the entry points' refusals, the struct sizes, the CPU
restatements (tests/sparseheldref.py) against the dense restatements they are built on, and the split, skip and smoothing rules of
LabeledLDA.heldout_perplexity_em with the kernels replaced by the restatements."""
import ctypes
import math

import numpy as np
import pytest

import attrref
import heldoutref
import leftrightref
import sparseheldref
import sparseref

BAD_K, BAD_ARG = -1, -2
MAX_K = 7688
SEED = 0x5EEDF00DCAFE


@pytest.fixture(scope="module")
def nat():
    from lda_thesis_amd import _native
    _native.lib()
    return _native


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the C ABI ----
def test_symbols_and_structs(nat):
    from test_abi import declared_symbols
    L = nat.lib()
    assert L.llda_abi_version() == 22 == nat.ABI_VERSION                # additive: the ABI number stays
    for s in ("llda_heldout_sparse_struct_bytes", "llda_heldout_loglik_sparse", "llda_leftright_sparse_struct_bytes",
              "llda_left_to_right_sparse"):
        assert s in nat.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_heldout_sparse_struct_bytes() == ctypes.sizeof(nat.LldaHeldoutSparseArgs) == 136
    assert L.llda_leftright_sparse_struct_bytes() == ctypes.sizeof(nat.LldaLeftrightSparseArgs) == 168
    assert nat.LR_MAX_K == 1024                                         # the dense entry point's limit has not moved


def heldout_call(nat, **kw):
    a = nat.LldaHeldoutSparseArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.max_labels = 12, 8
    a.doc_off, a.word, a.freq, a.lab_off, a.lab, a.theta_s, a.phi_t = (4096 + 1024 * i for i in range(7))
    a.mant, a.expo, a.tok, a.bad = (16384 + 1024 * i for i in range(4))
    a.D, a.V, a.NL, a.ld_phi = 5, 9, 20, 12
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_heldout_loglik_sparse(ctypes.byref(a), None)


def test_heldout_sparse_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it) or has nothing to do: D = 0"""
    call = lambda **kw: heldout_call(nat, **kw)
    assert call(D=0) == 0 and call(D=0, doc_off=None, word=None, lab_off=None, lab=None, theta_s=None, phi_t=None) == 0
    assert call(D=0, mant=None, expo=None, tok=None, bad=None) == 0
    assert nat.lib().llda_heldout_loglik_sparse(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaHeldoutSparseArgs) + 8, D=0) == BAD_ARG
    assert call(struct_bytes=ctypes.sizeof(nat.LldaHeldoutArgs), D=0) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_phi=MAX_K + 1, D=0) == BAD_K, K
    assert call(K=MAX_K, ld_phi=MAX_K, D=0) == 0 and call(K=1025, ld_phi=1025, D=0) == 0
    assert call(D=-1) == BAD_ARG and call(NL=-1, D=0) == BAD_ARG and call(ld_phi=11, D=0) == BAD_ARG
    for V in (0, -1, 2 ** 31):
        assert call(V=V, D=0) == BAD_ARG, V
    for m in (0, -1, 33, 2 ** 31 - 1):
        assert call(max_labels=m, D=0) == BAD_ARG, m
    for m in (1, 8, 9, 16, 17, 32):
        assert call(max_labels=m, D=0) == 0, m
    for name in ("doc_off", "word", "lab_off", "lab", "theta_s", "phi_t"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("doc_off", "lab_off", "theta_s", "phi_t", "mant", "expo", "tok", "bad"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("word", "freq", "lab"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG               # V x ld leaves an int64


def leftright_call(nat, **kw):
    a = nat.LldaLeftrightSparseArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.doc_off, a.word, a.phi_t, a.lab_off, a.lab, a.doc_ids = (4096 + 1024 * i for i in range(6))
    a.mant, a.expo, a.tok, a.bad, a.status = (16384 + 1024 * i for i in range(5))
    a.D, a.V, a.K, a.R, a.ld_phi, a.NL, a.max_labels, a.max_doc_tokens, a.alpha = 2, 10, 8, 4, 8, 6, 8, 100, 0.1
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_left_to_right_sparse(ctypes.byref(a), None)


def test_leftright_sparse_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it) or has nothing to do: D = 0"""
    call = lambda **kw: leftright_call(nat, **kw)
    assert call(D=0) == 0 and call(D=0, doc_off=None, word=None, phi_t=None, lab_off=None, lab=None, mant=None) == 0
    assert nat.lib().llda_left_to_right_sparse(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaLeftrightSparseArgs) + 8, D=0) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_phi=MAX_K + 1, D=0) == BAD_K, K
    for K in (1024, 1025, 2048, MAX_K):                                 # beyond the dense entry point's 1024
        assert call(K=K, ld_phi=K, D=0) == 0, K
    assert call(D=-1) == BAD_ARG and call(NL=-1, D=0) == BAD_ARG and call(ld_phi=7, D=0) == BAD_ARG
    for V in (0, -1, 2 ** 31):
        assert call(V=V, D=0) == BAD_ARG, V
    for m in (0, -1, 33):
        assert call(max_labels=m, D=0) == BAD_ARG, m
    for m in (1, 8, 9, 16, 17, 32):
        assert call(max_labels=m, D=0) == 0, m
    for R in (0, -1, 17):
        assert call(R=R, D=0) == BAD_ARG, R
    for R in (1, 16):
        assert call(R=R, D=0) == 0, R
    for alpha in (0.0, -0.5, float("inf"), float("nan")):
        assert call(alpha=alpha, D=0) == BAD_ARG, alpha
    for n in (0, -1, 4097):
        assert call(max_doc_tokens=n, D=0) == BAD_ARG, n
    assert call(max_doc_tokens=4096, D=0) == 0
    for name in ("doc_off", "word", "phi_t", "lab_off", "lab", "mant", "expo", "tok", "bad"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("doc_off", "phi_t", "lab_off", "doc_ids", "mant", "expo", "tok", "bad"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("word", "lab", "status"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG               # V x ld leaves an int64


# ---- the restatements ----
def toy(seed, K, D=12, V=15, prefix=False, max_count=6):
    rng = np.random.default_rng(seed)
    phi_t = rng.gamma(0.4, size=(V, K)) / V + 1e-6
    phi_t[rng.random((V, K)) < 0.2] = 0.0
    lens = rng.integers(0, 9, size=D)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = rng.integers(0, V, size=int(doc_off[-1])).astype(np.int32)
    word[::7] = V                                                       # outside the vocabulary
    freq = rng.integers(0, 5, size=word.shape[0]).astype(np.int32)
    sets = []
    for d in range(D):
        L = 0 if d == 3 else int(rng.integers(1, min(max_count, K) + 1))   # document 3 carries no label
        sets.append(np.arange(L) if prefix else np.sort(rng.choice(K, size=L, replace=False)))
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    lab = np.concatenate(sets).astype(np.int32)
    theta_s = rng.gamma(0.5, size=lab.shape[0]) + 1e-3
    return dict(K=K, V=V, D=D, phi_t=phi_t, doc_off=doc_off, word=word, freq=freq, lab_off=lab_off, lab=lab, theta_s=theta_s)


@pytest.mark.parametrize("K", (9, 70, 200))
def test_loglik_sparse_ref_on_prefix_sets_is_loglik_ref_at_full_k(K):
    c = toy(100 + K, K, prefix=True)
    theta = sparseref.scatter(c["theta_s"], c["lab_off"], c["lab"], K)
    want = heldoutref.loglik_ref(theta, c["phi_t"], c["doc_off"], c["word"], c["freq"])
    got = sparseheldref.loglik_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"])
    assert np.array_equal(bits(got[0]), bits(want[0])) and all(np.array_equal(g, w) for g, w in zip(got[1:], want[1:]))
    assert got[2].sum() > 0 and got[3].sum() > 0 and np.diff(c["lab_off"])[3] == 0 and got[2][3] == 0


@pytest.mark.parametrize("K", (70, 200))
def test_loglik_sparse_ref_on_scattered_sets_differs_only_where_sum64_pairs_differently(K):
    """the same sites are scored (tok / bad bit for bit); the logarithms agree to rounding (this tolerance is no contract)"""
    c = toy(200 + K, K)
    theta = sparseref.scatter(c["theta_s"], c["lab_off"], c["lab"], K)
    want = heldoutref.loglik_ref(theta, c["phi_t"], c["doc_off"], c["word"], c["freq"])
    got = sparseheldref.loglik_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"])
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    ll = lambda r: np.log(r[0]) + r[1].astype(np.float64) * math.log(2.0)
    np.testing.assert_allclose(ll(got), ll(want), rtol=1e-12, atol=1e-12)


def test_loglik_sparse_ref_unfit_documents():
    c = toy(7, 30)
    lab, fsum = c["lab"].copy(), np.add.reduceat(np.append(c["freq"], 0).astype(np.int64), c["doc_off"][:-1]) * (np.diff(c["doc_off"]) > 0)
    d = int(np.flatnonzero((np.diff(c["lab_off"]) >= 2) & (np.diff(c["doc_off"]) > 0))[0])
    lab[c["lab_off"][d] + 1] = lab[c["lab_off"][d]]                     # a label named twice
    full = sparseheldref.loglik_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"])
    got = sparseheldref.loglik_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], lab)
    assert (got[0][d], got[1][d], got[2][d], got[3][d]) == (0.5, 1, 0, fsum[d])
    others = np.arange(c["D"]) != d
    assert all(np.array_equal(bits(g[others]) if g.dtype == np.float64 else g[others], bits(f[others]) if f.dtype == np.float64 else f[others])
               for g, f in zip(got, full))
    few = sparseheldref.loglik_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], max_labels=1)
    long = np.diff(c["lab_off"]) > 1
    assert (few[2][long] == 0).all() and np.array_equal(few[3][long], fsum[long]) and np.array_equal(few[2][~long], full[2][~long])


@pytest.mark.parametrize("K,R", ((9, 3), (70, 2), (200, 4)))
def test_left_to_right_sparse_ref_on_prefix_sets_is_left_to_right_ref_at_full_k(K, R):
    c = toy(300 + K, K, D=8, prefix=True)
    allowed = (sparseref.scatter(np.ones(c["lab"].shape[0]), c["lab_off"], c["lab"], K) != 0).astype(np.uint8)
    ids = [5, 2 ** 32 + 1, 0, 3, 2 ** 35, 9, 1, 2]
    want = leftrightref.left_to_right_ref(c["phi_t"], c["doc_off"], c["word"], 0.3, R, SEED, 9, allowed=allowed, doc_ids=ids)
    got = sparseheldref.left_to_right_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["lab_off"], c["lab"], 0.3, R, SEED, 9, doc_ids=ids)
    assert np.array_equal(bits(got[0]), bits(want[0])) and all(np.array_equal(g, w) for g, w in zip(got[1:4], want[1:4])) and got[4] == want[4] == 0
    assert got[2].sum() > 0 and got[3].sum() > 0
    # the document without a label: A = 0, every pred NaN, every token bad -- in both
    assert got[2][3] == 0 and got[3][3] == np.diff(c["doc_off"])[3] == want[3][3]


def test_left_to_right_sparse_ref_on_scattered_sets_scores_the_same_tokens():
    """scattered sets, one particle: the draws may differ where sum64 pairs differently, the scored and the bad tokens may not
    (a token is bad when its word is outside the vocabulary or loads on none of the document's labels, whatever was drawn)"""
    K = 70
    c = toy(400, K, D=8)
    c["phi_t"] = np.where(c["phi_t"] == 0.0, 1e-7, c["phi_t"])          # (only the words outside the vocabulary are bad)
    allowed = (sparseref.scatter(np.ones(c["lab"].shape[0]), c["lab_off"], c["lab"], K) != 0).astype(np.uint8)
    want = leftrightref.left_to_right_ref(c["phi_t"], c["doc_off"], c["word"], 0.3, 1, SEED, 9, allowed=allowed)
    got = sparseheldref.left_to_right_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["lab_off"], c["lab"], 0.3, 1, SEED, 9)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    # one token, one particle: p = sum64(alpha phi) / (L alpha), the same products paired by slot or by topic id
    one = dict(doc_off=np.array([0, 1]), word=np.array([2]), lab_off=c["lab_off"][:2], lab=c["lab"][:int(c["lab_off"][1])])
    a = sparseheldref.left_to_right_sparse_ref(c["phi_t"], one["doc_off"], one["word"], one["lab_off"], one["lab"], 0.3, 1, SEED, 9)
    b = leftrightref.left_to_right_ref(c["phi_t"], one["doc_off"], one["word"], 0.3, 1, SEED, 9, allowed=allowed[:1])
    ll = lambda r: math.log(r[0][0]) + float(r[1][0]) * math.log(2.0)
    assert a[2][0] == b[2][0] == 1 and abs(ll(a) - ll(b)) < 1e-12


def test_left_to_right_sparse_ref_too_long_and_unfit():
    c = toy(500, 40, D=8)
    lens = np.diff(c["doc_off"])
    cap = int(np.sort(lens)[-2])
    r = sparseheldref.left_to_right_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["lab_off"], c["lab"], 0.3, 2, SEED, 9, max_doc_tokens=cap)
    over = lens > cap
    assert r[4] == 1 and over.sum() >= 1 and (r[0][over] == 0.5).all() and (r[1][over] == 1).all() and not r[2][over].any() and not r[3][over].any()
    few = sparseheldref.left_to_right_sparse_ref(c["phi_t"], c["doc_off"], c["word"], c["lab_off"], c["lab"], 0.3, 2, SEED, 9, max_labels=1)
    long = np.diff(c["lab_off"]) > 1
    assert few[4] == 0 and not few[2][long].any() and np.array_equal(few[3][long], lens[long])


# ---- LabeledLDA.heldout_perplexity_em with the kernels replaced by the restatements ----
class Dicti:
    def __init__(self, vocab):
        self.token2id = {w: i for i, w in enumerate(vocab)}

    def doc2bow(self, doc):
        c = {}
        for w in doc:
            if w in self.token2id:
                c[self.token2id[w]] = c.get(self.token2id[w], 0) + 1
        return sorted(c.items())


@pytest.fixture
def model(monkeypatch):
    """a LabeledLDA that was never trained: six labels after the root, eleven words, phi_t fixed; the four kernels behind
    heldout_perplexity_em are the CPU restatements"""
    import torch
    from lda_thesis_amd import attribution, heldout
    from lda_thesis_amd.LabeledLDA import LabeledLDA
    rng = np.random.default_rng(77)
    K, V = 7, 11
    m = LabeledLDA.__new__(LabeledLDA)
    m.K, m.alpha = K, 0.25
    m.labelmap = dict([("root", 0)] + [("l%d" % k, k) for k in range(1, K)])
    m.dicti = Dicti(["w%d" % v for v in range(V)])
    phi_t = rng.gamma(0.5, size=(V, K)) + 1e-3
    phi_t /= phi_t.sum(axis=0, keepdims=True)
    m._attr_device = lambda: torch.device("cpu")
    m._phi_t_device = lambda: torch.from_numpy(phi_t)
    calls = []

    def attribute(theta, phi, doc_off, word, freq, iters=0, alpha=0.0, top_m=1, want=()):
        calls.append("attribute")
        r = attrref.attribute_ref(theta.numpy(), phi.numpy(), doc_off, word, freq, iters=iters, alpha=alpha, top_m=0)
        return dict(theta=torch.from_numpy(r["theta_out"]))

    def attribute_sparse(theta_s, phi, doc_off, word, freq, lab_off, lab, iters=0, alpha=0.0, top_m=1, want=()):
        calls.append("attribute_sparse")
        r = sparseref.attribute_sparse_ref(theta_s.numpy(), phi.numpy(), doc_off, word, freq, lab_off, lab, iters=iters, alpha=alpha)
        return dict(theta=torch.from_numpy(r["theta_out"]))

    def loglik(theta, phi, doc_off, word, freq, weighted=True):
        calls.append("loglik")
        return heldoutref.loglik_ref(theta.numpy(), phi.numpy(), doc_off, word, freq if weighted else None)

    def loglik_sparse(theta_s, phi, doc_off, word, freq, lab_off, lab, weighted=True):
        calls.append("loglik_sparse")
        return sparseheldref.loglik_sparse_ref(theta_s.numpy(), phi.numpy(), doc_off, word, freq if weighted else None, lab_off, lab)

    monkeypatch.setattr(attribution, "attribute", attribute)
    monkeypatch.setattr(attribution, "attribute_sparse", attribute_sparse)
    monkeypatch.setattr(heldout, "loglik", loglik)
    monkeypatch.setattr(heldout, "loglik_sparse", loglik_sparse)
    m.test_phi_t, m.test_calls = phi_t, calls
    return m


DOCS = [["w1", "w2", "w2", "w5", "w9", "nope"], ["nope"], ["w3"], ["w0", "w4", "w4", "w4", "w7", "w8", "w10"], []]
LABELS = [["l2", "l5"], ["l1"], [], ["l6", "l1", "l3"], ["l2"]]


def test_heldout_perplexity_em_split_skip_and_smoothing(model):
    from lda_thesis_amd import heldout
    tups = [model.dicti.doc2bow(x) for x in DOCS]
    cols = [[0] + sorted(model.labelmap[x] for x in labs) for labs in LABELS]
    for weighted in (True, False):
        r = model.heldout_perplexity_em(DOCS, iters=6, labels=LABELS, sparse=True, weighted=weighted)
        want = sparseheldref.heldout_perplexity_em_ref(model.test_phi_t, tups, cols, model.alpha, 6, weighted=weighted)
        s = heldout.perplexity_from(want["mant"], want["expo"], [want["tokens"]], [want["bad"]])
        assert (r["loglik"], r["tokens"], r["documents"], r["skipped"]) == (s["loglik"], want["tokens"], 3, 2)
        assert r["perplexity"] == math.exp(-r["loglik"] / r["tokens"]) and want["bad"] == 0
    assert model.test_calls == ["attribute_sparse", "loglik_sparse"] * 2             # no dense kernel on the sparse route
    # the split: the sites 0, 2, .. observed, 1, 3, .. scored (unweighted here: two sites of document 0, two of document 3);
    # document 2 has one site -- observed, nothing scored; 1 and 4 have nothing to observe and are skipped
    assert tups[0] == [(1, 1), (2, 2), (5, 1), (9, 1)] and r["tokens"] == 2 + 0 + 2 and want["documents"] == 3 and want["skipped"] == 2
    # the smoothing rule by hand for document 0: (W th + alpha) / (W + L alpha) per slot, W = 2 observed tokens, L = 3
    obs = [t[0::2] for t in tups]
    th = sparseref.attribute_sparse_ref(np.full(3, 1.0 / 3.0), model.test_phi_t, np.array([0, 2]), np.array([w for w, _ in obs[0]]),
                                        np.array([f for _, f in obs[0]]), np.array([0, 3]), np.array(cols[0]), iters=6, alpha=model.alpha)["theta_out"]
    W = float(sum(f for _, f in obs[0]))
    assert W == 2.0
    by_hand = (W * th + model.alpha) / (W + 3.0 * model.alpha)
    assert np.array_equal(bits(sparseheldref.smooth_slots_ref(th, [W], [0, 3], model.alpha)), bits(by_hand))
    assert np.array_equal(bits(heldout.smooth_slots(th, np.array([W]), np.array([0, 3]), model.alpha)), bits(by_hand))
    assert abs(by_hand.sum() - 1.0) < 1e-12
    # scored_docs: newdocs observed whole, these scored
    r2 = model.heldout_perplexity_em(DOCS, iters=3, labels=LABELS, sparse=True, scored_docs=[["w1"], ["w2"], ["w3", "w3"], [], ["w4"]])
    want2 = sparseheldref.heldout_perplexity_em_ref(model.test_phi_t, tups, cols, model.alpha, 3,
                                                    scored_tups=[model.dicti.doc2bow(x) for x in (["w1"], ["w2"], ["w3", "w3"], [], ["w4"])])
    assert (r2["tokens"], r2["documents"], r2["skipped"]) == (want2["tokens"], 3, 2) == (3, 3, 2)
    assert r2["loglik"] == heldout.perplexity_from(want2["mant"], want2["expo"], [3], [0])["loglik"]
    with pytest.raises(ValueError):
        model.heldout_perplexity_em(DOCS, sparse=True)
    with pytest.raises(ValueError):
        model.heldout_perplexity_em(DOCS, labels=LABELS[:-1])
    with pytest.raises(KeyError):
        model.heldout_perplexity_em(DOCS, labels=[["unknown"]] * 5)
    none = model.heldout_perplexity_em([["nope"], []], iters=2)
    assert math.isnan(none["perplexity"]) and (none["tokens"], none["documents"], none["skipped"]) == (0, 0, 2)


def test_heldout_perplexity_em_dense_routes(model):
    """prefix label sets: sparse and dense return identical dicts; without labels the smoothing is smooth_theta's, with K"""
    from lda_thesis_amd import heldout
    prefix = [["l1", "l2"], ["l1"], [], ["l1", "l2", "l3"], ["l1"]]
    a = model.heldout_perplexity_em(DOCS, iters=5, labels=prefix, sparse=True)
    b = model.heldout_perplexity_em(DOCS, iters=5, labels=prefix, sparse=False)
    assert a == b and a["tokens"] == 3 + 4 and model.test_calls == ["attribute_sparse", "loglik_sparse", "attribute", "loglik"]
    # scattered sets: the same tokens, the logarithm to rounding
    c = model.heldout_perplexity_em(DOCS, iters=5, labels=LABELS, sparse=True)
    d = model.heldout_perplexity_em(DOCS, iters=5, labels=LABELS, sparse=False)
    assert c["tokens"] == d["tokens"] and abs(c["loglik"] - d["loglik"]) < 1e-9
    # no labels: every topic, theta = (W th + alpha) / (W + K alpha)
    e = model.heldout_perplexity_em(DOCS, iters=4)
    tups = [model.dicti.doc2bow(x) for x in DOCS]
    keep = [0, 2, 3]
    obs, sc = [tups[i][0::2] for i in keep], [tups[i][1::2] for i in keep]
    csr = lambda ts: (np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int64), np.array([w for t in ts for w, _ in t], dtype=np.int32),
                      np.array([f for t in ts for _, f in t], dtype=np.int32))
    th = attrref.attribute_ref(np.full((3, model.K), 1.0 / model.K), model.test_phi_t, *csr(obs), iters=4, alpha=model.alpha, top_m=0)["theta_out"]
    theta = heldout.smooth_theta(th, heldout.observed_tokens(obs), model.alpha)
    want = heldout.perplexity_from(*heldoutref.loglik_ref(theta, model.test_phi_t, *csr(sc)))
    assert (e["loglik"], e["tokens"], e["documents"], e["skipped"]) == (want["loglik"], want["tokens"], 3, 2)
    # with labels, dense: L_d in place of K on the allowed columns, 0 elsewhere
    on = np.array([[1, 1, 0, 1], [1, 0, 0, 0]], dtype=np.uint8)
    t2 = np.array([[0.5, 0.25, 0.0, 0.25], [1.0, 0.0, 0.0, 0.0]])
    sm = heldout.smooth_theta_labels(t2, np.array([4.0, 2.0]), on, 0.5)
    assert np.array_equal(bits(sm[0]), bits(np.array([(4.0 * 0.5 + 0.5) / (4.0 + 3 * 0.5), (4.0 * 0.25 + 0.5) / 5.5, 0.0, (4.0 * 0.25 + 0.5) / 5.5])))
    assert np.array_equal(bits(sm[1]), bits(np.array([1.0, 0.0, 0.0, 0.0])))
    import torch
    st = heldout.smooth_theta_labels(torch.from_numpy(t2), torch.tensor([4.0, 2.0], dtype=torch.float64), torch.from_numpy(on), 0.5)
    assert np.array_equal(bits(st.numpy()), bits(sm))


def test_the_harness_takes_the_new_flags():
    from lda_thesis_amd import evaluate_LabeledLDA as E
    opt = E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])[0]
    assert opt.lr_sparse is False and opt.heldout_em == 0
    opt = E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--left-to-right", "5", "--lr-sparse", "--heldout-em", "7", "--em-sparse"])[0]
    assert opt.lr_sparse is True and opt.heldout_em == 7 and opt.em_sparse is True and opt.left_to_right == 5
