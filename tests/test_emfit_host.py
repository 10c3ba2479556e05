"""EM training without a GPU: the restatement tests/emref.py against the document side (tests/attrref.py) and against its own
specification, the monotone MAP objective of the iteration, and the C ABI of llda_credit_words / llda_phi_step -- the exported
symbols, the two structs and every refusal of the header, all decided on the host before any HIP call (the pointers below are never
dereferenced there)."""
import ctypes

import numpy as np
import pytest

import attrref
import emref

BAD_K, BAD_ARG = -1, -2
MAX_K = 7688


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def toy(seed, D=40, V=23, K=9, lens=(1, 2, 5, 9, 17), labelled=True):
    """a random corpus with label sets: theta0 (D, K) uniform over root + 1 .. 3 labels, phi_t0 (V, K) positive, the CSR"""
    rng = np.random.default_rng(seed)
    n = rng.choice(lens, size=D)
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = np.minimum((rng.zipf(1.3, size=S) - 1), V - 1).astype(np.int32)     # a few hot words, a tail; word V - 2 may stay unused
    word[word == V - 2] = 0
    freq = rng.integers(1, 5, size=S).astype(np.int32)
    theta = np.zeros((D, K))
    for d in range(D):
        cols = np.concatenate([[0], 1 + rng.choice(K - 1, size=rng.integers(1, 4), replace=False)]) if labelled else np.arange(K)
        theta[d, cols] = 1.0 / len(cols)
    phi_t = rng.gamma(0.3, size=(V, K)) + 1e-6
    phi_t /= phi_t.sum(axis=0, keepdims=True)
    return theta, phi_t, doc_off, word, freq


def test_word_side_and_document_side_add_the_same_terms():
    theta, phi_t, doc_off, word, freq = toy(1)
    S, V = int(doc_off[-1]), phi_t.shape[0]
    assert 200 <= S <= 900
    word_off, site_doc, w_freq, order = emref.word_major(doc_off, word, freq, V)
    assert (np.diff(site_doc[word_off[0]:word_off[1]]) >= 0).all() and (word[order] == np.repeat(np.arange(V), np.diff(word_off))).all()
    doc = attrref.attribute_ref(theta, phi_t, doc_off, word, freq)
    for chunk in (1, 7, 10 ** 6):
        got = emref.credit_words_ref(theta, phi_t, word_off, site_doc, w_freq, chunk)
        a, b = got["credit"].sum(axis=0), doc["credit"].sum(axis=0)
        assert (np.abs(a - b) <= S * 2.0 ** -52 * b).all(), chunk              # the same non-negative terms in another order
        assert int(got["tok"].sum()) == int(doc["tok"].sum()) == int(freq.sum()) and int(got["bad"].sum()) == int(doc["bad"].sum()) == 0
        assert not got["credit"][V - 2].any() and got["tok"][V - 2] == 0       # a word without sites
        assert (got["credit"][:, 1:][:, (theta[:, 1:] == 0).all(axis=0)] == 0).all()
    # sites that do not count: a document id outside [0, D), a row of zeros
    site_doc2 = site_doc.copy()
    site_doc2[[0, 5]] = (-1, theta.shape[0])
    theta2 = theta.copy()
    theta2[3] = 0.0
    got = emref.credit_words_ref(theta2, phi_t, word_off, site_doc2, w_freq, 4)
    want_bad = int(w_freq[[0, 5]].sum()) + int(w_freq[(site_doc2 == 3)].sum())
    assert int(got["bad"].sum()) == want_bad and int(got["tok"].sum()) == int(freq.sum()) - want_bad


def site_terms(theta, phi_t, word_off, site_doc, freq, K):
    """t_k * g of every site, from the specification (every site of this corpus is good)"""
    v_of = np.repeat(np.arange(len(word_off) - 1), np.diff(word_off))
    t = theta[site_doc][:, :K] * phi_t[v_of][:, :K]
    p = attrref.sum64(t)
    g = freq.astype(np.float64) * (np.float64(1.0) / p)
    return t * g[:, None]


def test_the_result_depends_on_chunk_alone():
    theta, phi_t, doc_off, word, freq = toy(2, D=60)
    V, K = phi_t.shape
    word_off, site_doc, w_freq, _ = emref.word_major(doc_off, word, freq, V)
    runs = np.diff(word_off)
    longest = int(runs.max())
    assert longest > 130 and (runs == 0).any() and (runs == 1).any()
    terms = site_terms(theta, phi_t, word_off, site_doc, w_freq, K)
    got = {c: emref.credit_words_ref(theta, phi_t, word_off, site_doc, w_freq, c)["credit"] for c in (1, 3, 64, longest + 5)}
    for chunk, credit in got.items():
        for v in range(V):                                                      # the grouping, written out
            total = np.zeros(K)
            for c in range(int(word_off[v]), int(word_off[v + 1]), chunk):
                acc = np.zeros(K)
                for s in range(c, min(c + chunk, int(word_off[v + 1]))):
                    acc = acc + terms[s]
                total = total + acc
            assert np.array_equal(bits(credit[v]), bits(total)), (chunk, v)
    differ = {c: (bits(got[c]) != bits(got[longest + 5])).any(axis=1) for c in (1, 3, 64)}
    assert differ[3].any() and differ[64].any()                                 # the order does reach the last bits ...
    for c in (3, 64):                                                           # ... of no word whose run fits one chunk
        assert not differ[c][runs <= c].any()
    assert np.array_equal(bits(got[1]), bits(got[longest + 5]))                 # chunks of one site: the same sequential sum


def test_phi_step_ref():
    rng = np.random.default_rng(3)
    cw = rng.gamma(0.5, size=(600, 5)) * 10
    phi, den = emref.phi_step_ref(cw, 0.01)
    blocks = [np.add.reduce(cw[r:r + 256], axis=0) for r in (0, 256, 512)]     # (pairwise in numpy: close, not equal)
    np.testing.assert_allclose(den, blocks[0] + blocks[1] + blocks[2] + 6.0, rtol=1e-13)
    np.testing.assert_allclose(phi.sum(axis=0), 1.0, rtol=1e-12)
    seq = np.zeros(5)
    for r in range(255):
        seq = seq + cw[r]
    assert np.array_equal(bits(emref.phi_step_ref(cw[:255], 0.5)[1]), bits((np.zeros(5) + seq) + 255 * 0.5))


@pytest.mark.parametrize("alpha", (0.001, 0.1))
@pytest.mark.parametrize("beta", (0.001, 0.1))
def test_the_map_objective_never_falls(alpha, beta):
    theta, phi_t, doc_off, word, freq = toy(4, D=30, V=17, K=6, lens=(1, 3, 6, 11))
    zero = theta == 0.0
    trail = [emref.objective(theta, phi_t, doc_off, word, freq, alpha, beta)]

    def each(it, th, ph):
        assert (th[zero] == 0.0).all() and (th[~zero] > 0.0).all() and (ph > 0.0).all()      # a zero of theta stays zero
        np.testing.assert_allclose(th.sum(axis=1), 1.0, rtol=1e-12)
        np.testing.assert_allclose(ph.sum(axis=0), 1.0, rtol=1e-12)
        trail.append(emref.objective(th, ph, doc_off, word, freq, alpha, beta))

    emref.fit_ref(theta, phi_t, doc_off, word, freq, alpha, beta, 15, chunk=5, each=each)
    assert len(trail) == 16 and trail[-1] > trail[0]
    for a, b in zip(trail[:-1], trail[1:]):
        assert b >= a - 1e-9 * abs(a), trail


# ---- the C ABI ----
@pytest.fixture(scope="module")
def nat():
    from lda_thesis_amd import _native
    _native.lib()
    return _native


def test_symbols_structs_and_constants(nat):
    from test_abi import declared_symbols
    L = nat.lib()
    assert L.llda_abi_version() == 22 == nat.ABI_VERSION                # additive: the ABI number stays
    for s in ("llda_wcredit_struct_bytes", "llda_credit_words_scratch_bytes", "llda_credit_words", "llda_phistep_struct_bytes",
              "llda_phi_step_scratch_bytes", "llda_phi_step"):
        assert s in nat.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_wcredit_struct_bytes() == ctypes.sizeof(nat.LldaWcreditArgs)
    assert L.llda_phistep_struct_bytes() == ctypes.sizeof(nat.LldaPhistepArgs)
    assert nat.COLSUM_ROWS == emref.COLSUM_ROWS == 256
    header = open(nat.os.path.join(nat.os.path.dirname(nat._HERE), "include", "llda_gibbs.h")).read()
    assert "#define LLDA_COLSUM_ROWS 256" in header and "#define LLDA_WCREDIT_MAX_SITES (1LL << 40)" in header


def test_scratch_queries(nat):
    L = nat.lib()
    sb = nat.credit_words_scratch_bytes
    assert sb(1, 0, 1, 1) == 16 * 2 + 16 and sb(61, 1000, 7, 4096) == 16 * 62 + 4 * 61 + 4 + 16    # no word can have two chunks
    assert sb(61, 1000, 7, 64) == 16 * 62 + 2 * 15 * (8 * 7 + 16) + 4 * (15 + 61) + 16 and sb(61, 10, 7, 1) == 16 * 62 + 20 * 72 + 40 + 16
    assert sb(2 ** 31 - 1, 2 ** 40, MAX_K, 1) < 2 ** 63
    sizes = [sb(100, S, 512, 64) for S in (0, 63, 64, 65, 10 ** 4, 10 ** 9)]
    assert sizes == sorted(sizes) and sizes[1] - sizes[0] == 4 * 63 + 4 and sizes[2] - sizes[1] == 2 * (8 * 512 + 16)
    for bad in ((0, 5, 8, 4), (2 ** 31, 5, 8, 4), (5, -1, 8, 4), (5, 2 ** 40 + 1, 8, 4), (5, 5, 0, 4), (5, 5, MAX_K + 1, 4), (5, 5, 8, 0), (5, 5, 8, -3)):
        assert L.llda_credit_words_scratch_bytes(*bad) == BAD_ARG, bad
    with pytest.raises(nat.NativeError):
        sb(5, 5, 8, 0)
    pb = nat.phi_step_scratch_bytes
    assert pb(1, 1) == 2 * 8 + 16 and pb(256, 3) == 2 * 24 + 16 and pb(257, 3) == 3 * 24 + 16
    for bad in ((0, 3), (2 ** 31, 3), (5, 0), (5, MAX_K + 1)):
        assert L.llda_phi_step_scratch_bytes(*bad) == BAD_ARG, bad


def wcredit_call(nat, **kw):
    a = nat.LldaWcreditArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.chunk = 12, 64
    a.word_off, a.site_doc, a.freq, a.theta, a.phi_t = (4096 + 1024 * i for i in range(5))
    a.credit_w, a.tok, a.bad, a.scratch = (16384 + 1024 * i for i in range(4))
    a.D, a.V, a.S, a.ld_theta, a.ld_phi, a.ld_credit, a.scratch_bytes = 5, 9, 100, 12, 12, 12, 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_credit_words(ctypes.byref(a), None)


def test_credit_words_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it), or has nothing to launch: every output NULL"""
    call = lambda **kw: wcredit_call(nat, **kw)
    none = dict(credit_w=None, tok=None, bad=None)
    assert call(**none) == 0
    assert nat.lib().llda_credit_words(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaWcreditArgs) + 8) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_theta=MAX_K + 1, ld_phi=MAX_K + 1, ld_credit=MAX_K + 1) == BAD_K, K
    assert call(K=MAX_K, ld_theta=MAX_K, ld_phi=MAX_K, ld_credit=MAX_K, **none) == 0
    assert call(D=-1) == BAD_ARG and call(D=0, theta=None, **none) == 0
    for V in (0, -1, 2 ** 31):
        assert call(V=V) == BAD_ARG, V
    assert call(V=2 ** 31 - 1, **none) == 0
    assert call(S=-1) == BAD_ARG and call(S=2 ** 40 + 1) == BAD_ARG
    for name in ("ld_theta", "ld_phi", "ld_credit"):
        assert call(**{name: 11}) == BAD_ARG, name
    for chunk in (0, -1, -2 ** 31):
        assert call(chunk=chunk) == BAD_ARG, chunk
    assert call(chunk=1, **none) == 0 and call(chunk=2 ** 31 - 1, **none) == 0
    for name in ("word_off", "site_doc", "phi_t", "theta", "scratch"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(freq=None, **none) == 0
    assert call(S=0, word_off=None, site_doc=None, phi_t=None, theta=None, scratch=None, scratch_bytes=0, **none) == 0
    for name in ("word_off", "theta", "phi_t", "credit_w", "tok", "bad", "scratch"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("site_doc", "freq"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    need = nat.credit_words_scratch_bytes(9, 100, 12, 64)
    assert call(scratch_bytes=need - 1) == BAD_ARG and call(scratch_bytes=0) == BAD_ARG and call(scratch_bytes=need, **none) == 0
    assert call(chunk=1, scratch_bytes=need) == BAD_ARG                 # smaller chunks, more partial rows
    assert call(D=2 ** 40, ld_theta=2 ** 40) == BAD_ARG                 # D x ld leaves an int64
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG and call(V=2 ** 31 - 1, ld_credit=2 ** 40) == BAD_ARG


def phistep_call(nat, **kw):
    a = nat.LldaPhistepArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.cw, a.phi_t_out, a.den, a.scratch = 12, 4096, 8192, 12288, 16384
    a.V, a.ld, a.ld_out, a.beta, a.scratch_bytes = 9, 12, 12, 0.01, 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_phi_step(ctypes.byref(a), None)


def test_phi_step_refusals_come_before_the_device(nat):
    """no call below could launch: each has its one flaw"""
    call = lambda **kw: phistep_call(nat, **kw)
    assert nat.lib().llda_phi_step(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaPhistepArgs) + 8) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld=MAX_K + 1, ld_out=MAX_K + 1) == BAD_K, K
    for V in (0, -1, 2 ** 31):
        assert call(V=V) == BAD_ARG, V
    assert call(ld=11) == BAD_ARG and call(ld_out=11) == BAD_ARG
    for beta in (0.0, -0.5, float("inf"), float("nan"), -0.0):
        assert call(beta=beta) == BAD_ARG, beta
    for name in ("cw", "phi_t_out", "scratch"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("cw", "phi_t_out", "den", "scratch"):
        assert call(**{name: 4100}) == BAD_ARG, name
    need = nat.phi_step_scratch_bytes(9, 12)
    assert call(scratch_bytes=need - 1) == BAD_ARG and call(scratch_bytes=0) == BAD_ARG
    assert call(V=2 ** 31 - 1, ld=2 ** 40) == BAD_ARG and call(V=2 ** 31 - 1, ld_out=2 ** 40) == BAD_ARG


def test_the_harness_takes_em_train(monkeypatch):
    """--em-train ITERS reaches train_it, which then calls fit_em in place of run_training"""
    from lda_thesis_amd import LabeledLDA as L, evaluate_LabeledLDA as ev
    opt, _ = ev.build_parser().parse_args(["-f", "x.csv", "-i", "4", "--em-train", "30"])
    assert opt.em_train == 30 and ev.build_parser().parse_args(["-f", "x.csv"])[0].em_train == 0
    calls = []

    class Model(object):
        def __init__(self, *a):
            pass

        def fit_em(self, iters):
            calls.append(("fit_em", iters))

        def run_training(self, it, s):
            calls.append(("run_training", it, s))

    monkeypatch.setattr(L, "LabeledLDA", Model)
    monkeypatch.setattr(L, "prune_dict", lambda a, lower, upper: None)
    L.train_it(([], [], []), it=4, s=2, em=30)
    L.train_it(([], [], []), it=4, s=2)
    assert calls == [("fit_em", 30), ("run_training", 4, 2)]


def test_python_refusals_need_no_device():
    """what emfit checks before it asks for a device"""
    from lda_thesis_amd import emfit
    with pytest.raises(ValueError):
        emfit._check_chunk(0)
    with pytest.raises(ValueError):
        emfit._check_chunk(2 ** 31)
    assert emfit._check_chunk(4096) == emfit.DEFAULT_CHUNK
