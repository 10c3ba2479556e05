"""Host side of the score-ranked top words (``llda_scored_words``, lda_thesis_amd/topics.py): the exported symbols and the struct,
every refusal -- which returns before anything touches HIP, so it runs without a GPU --, ``relevance_powers`` and ``word_divisor``,
and the claims the device pass rests on: the order of phi^a / p^b IS the order of LDAvis relevance (no logarithm needed), the
counts-mode x has the bits of phi, and lam = 1 is the order by count."""
import ctypes

import numpy as np
import pytest

import scoredref
import topicref
from test_abi import declared_symbols

E_BAD_K, E_BAD_ARG = -1, -2


@pytest.fixture(scope="module")
def L():
    from lda_thesis_amd import _native
    return _native.lib()


def test_symbols_struct_and_abi_number(L):
    from lda_thesis_amd import _native
    for s in ("llda_scored_struct_bytes", "llda_scored_words_scratch_bytes", "llda_scored_words"):
        assert s in _native.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_abi_version() == 22 == _native.ABI_VERSION
    assert L.llda_scored_struct_bytes() == ctypes.sizeof(_native.LldaScoredArgs)
    assert L.llda_struct_size(7) == -1


def _args(**kw):
    """a call that would be accepted, counts mode, with never-dereferenced pointers; kw overrides fields"""
    from lda_thesis_amd import _native
    p = 4096
    a = dict(struct_bytes=ctypes.sizeof(_native.LldaScoredArgs), K=12, n=10, a=2, n_kw=p, n_k=p, den=None, mat=None, wdiv=p, V=100, ld=0,
             beta=0.01, top_idx=p, top_score=p, n_nan=p, scratch=p, scratch_bytes=1 << 40)
    a.update(kw)
    return _native.LldaScoredArgs(**a)


def _matrix(**kw):
    base = dict(n_kw=None, n_k=None, mat=4096, ld=12)
    base.update(kw)
    return _args(**base)


def test_every_refusal_returns_before_hip(L):
    from lda_thesis_amd import _native
    call = lambda a: L.llda_scored_words(ctypes.byref(a), None)
    assert L.llda_scored_words(None, None) == E_BAD_ARG
    assert call(_args(struct_bytes=0)) == E_BAD_ARG
    assert call(_args(struct_bytes=ctypes.sizeof(_native.LldaScoredArgs) + 8)) == E_BAD_ARG
    for K in (0, -3, _native.MAX_K + 1):
        assert call(_args(K=K)) == E_BAD_K and call(_matrix(K=K, ld=1 << 20)) == E_BAD_K
    assert call(_args(mat=4096, ld=12)) == E_BAD_ARG                     # both sources
    assert call(_args(n_kw=None)) == E_BAD_ARG                           # neither
    for n in (0, -1, 17):
        assert call(_args(n=n)) == E_BAD_ARG and call(_matrix(n=n)) == E_BAD_ARG
    for a in (0, -1, 9):
        assert call(_args(a=a)) == E_BAD_ARG and call(_matrix(a=a)) == E_BAD_ARG
    for V in (0, -5, 2 ** 31):
        assert call(_args(V=V)) == E_BAD_ARG and call(_matrix(V=V)) == E_BAD_ARG
    assert call(_matrix(ld=11)) == E_BAD_ARG and call(_matrix(ld=0)) == E_BAD_ARG and call(_matrix(ld=-1)) == E_BAD_ARG
    assert call(_matrix(ld=2 ** 62)) == E_BAD_ARG                        # V x ld beyond an int64
    assert call(_args(n_k=None, den=None)) == E_BAD_ARG                  # counts without a denominator
    assert call(_args(scratch=None)) == E_BAD_ARG
    assert call(_args(scratch_bytes=0)) == E_BAD_ARG and call(_matrix(scratch_bytes=0)) == E_BAD_ARG
    for name, align in (("n_kw", 16), ("den", 8), ("wdiv", 8), ("top_score", 8), ("scratch", 8), ("n_k", 4), ("top_idx", 4), ("n_nan", 4)):
        assert call(_args(**{name: 4096 + align // 2})) == E_BAD_ARG, name
    assert call(_matrix(mat=4100)) == E_BAD_ARG
    assert call(_args(n_kw=4104)) == E_BAD_ARG                           # 8-byte aligned is not enough for the counts


def test_scratch_bytes_codes_and_sizes(L):
    from lda_thesis_amd import _native
    sb = L.llda_scored_words_scratch_bytes
    assert sb(0, 12, 10) == E_BAD_ARG and sb(-1, 12, 10) == E_BAD_ARG and sb(2 ** 31, 12, 10) == E_BAD_ARG
    assert sb(100, 12, 0) == E_BAD_ARG and sb(100, 12, 17) == E_BAD_ARG
    assert sb(100, 0, 10) == E_BAD_K and sb(100, _native.MAX_K + 1, 10) == E_BAD_K
    call = lambda a: L.llda_scored_words(ctypes.byref(a), None)
    for K in (1, 5, 12, 511, 512, 1031, _native.MAX_K):
        KP = _native.layout_init(K)["KP"]
        for V in (1, 255, 256, 257, 5000):
            for n in (1, 10, 16):
                b = sb(V, K, n)
                chunks = -(-V // _native.TOPW_CHUNK_ROWS)
                per_part = KP * (12 * n + 4)                          # n scores, n ids and a NaN count per column
                assert b > 0 and b % 8 == 0 and b % (chunks * per_part) == 0 and b // (chunks * per_part) in (1, 2, 3, 4)
                assert call(_args(V=V, K=K, n=n, scratch_bytes=b - 1)) == E_BAD_ARG       # counts need all of it
                assert _native.scored_words_scratch_bytes(V, K, n) == b
    with pytest.raises(_native.NativeError):
        _native.scored_words_scratch_bytes(100, 0, 10)


def test_relevance_powers():
    from lda_thesis_amd import topics
    for lam, want in ((1, (1, 0)), (0, (1, 1)), (0.5, (2, 1)), (0.6, (5, 2)), (0.3, (7, 5)), (0.25, (4, 3)), (2 / 3, (3, 1))):
        assert topics.relevance_powers(lam) == want == scoredref.relevance_powers_ref(lam)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            topics.relevance_powers(bad)


def test_word_divisor():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(3)
    n_w = rng.integers(0, 50, size=400)
    n_w[:20] = 0
    for b in (0, 1, 2, 5, 7):
        for min_count in (0, 1, 3, 10):
            got = topics.word_divisor(n_w, b, min_count)
            assert got.dtype == np.float64
            assert np.array_equal(got == 0, n_w < max(min_count, 1))
            assert np.array_equal(got.view(np.uint64), scoredref.word_divisor_ref(n_w, b, min_count).view(np.uint64))
            if b == 0:
                assert np.array_equal(got[got != 0], np.ones(int((got != 0).sum())))
    with pytest.raises(ValueError):
        topics.word_divisor(n_w, 9)


LAMS = (0, 0.25, 0.3, 0.5, 0.6, 2 / 3, 1)


_INPUTS = {}


def _inputs(K, V, seed):
    """(m, n_w, p, {beta: (x, phi)}) of one generated matrix, built once for all the lam that use it"""
    key = (K, V, seed)
    if key not in _INPUTS:
        m = scoredref.skewed(np.random.default_rng(seed), K, V)
        m[:, m.sum(axis=0) == 0] = 1                                 # a word nobody holds gets count 1 in every topic
        n_w = m.sum(axis=0)
        p = n_w.astype(np.float64) / float(n_w.sum())
        _INPUTS[key] = (m, n_w, p, {beta: (scoredref.x_of_counts(m, beta), topicref.phi_of(m, beta)) for beta in (1e-6, 0.01, 0.5)})
    return _INPUTS[key]


def _against_log_form(K, V, seed, lam, log_lam):
    m, n_w, p, by_beta = _inputs(K, V, seed)
    a, b = scoredref.relevance_powers_ref(lam)
    wdiv = scoredref.word_divisor_ref(n_w, b)
    for beta, (x, phi) in by_beta.items():
        assert np.array_equal(x.T.view(np.uint64), phi.view(np.uint64))          # counts mode: x has the bits of phi
        idx, sc, nn = scoredref.scored_words_ref(x, 10, a, wdiv)
        assert (nn == 0).all() and sc.min() > 1e-78 and sc.max() < 1e9
        rel = log_lam * np.log(phi) + (1 - log_lam) * np.log(phi / p)
        bad = [k for k in range(K) if not np.array_equal(idx[k], np.argsort(-rel[k], kind="stable")[:10])]
        print("K=%d V=%d seed=%d beta=%g lam=%g (a, b)=(%d, %d): %d of %d topics differ" % (K, V, seed, beta, lam, a, b, len(bad), K))
        assert not bad, (beta, lam, bad[:5])


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("K,V", [(12, 5000), (130, 3000)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_power_form_has_the_order_of_the_log_form(K, V, seed, lam):
    """6 inputs x 7 lam, each with 3 beta = 126 cases: the first 10 words of EVERY topic by P_a(phi) / P_b(p) are the first 10 by
    lam * log(phi) + (1 - lam) * log(phi / p).  Every lam of the list goes through ``Fraction(lam).limit_denominator(8)``, as
    ``relevance_powers`` takes it: the lam of the log form is that fraction, which is lam itself for every entry but 0.3 -> 2/7 (the
    order at 2/7 is not the order at 0.3: a lam that is no such fraction is ranked at the nearest one)."""
    from fractions import Fraction
    _against_log_form(K, V, seed, lam, float(Fraction(lam).limit_denominator(8)))


def test_lam_one_is_the_order_by_count_on_hard_matrices():
    """the matrices of test_count_order_is_phi_order_on_hard_matrices (tests/test_topics_host.py), same seed"""
    rng = np.random.default_rng(5)
    V = 700
    small = rng.integers(0, 3, size=(6, V))
    small[3] = 0
    huge = rng.integers(0, topicref.INT32_MAX, size=(4, V), endpoint=True)
    huge[0, :40] = topicref.INT32_MAX - rng.integers(0, 3, size=40)
    huge[1, 5] = huge[1, 600] = topicref.INT32_MAX
    mixed = np.concatenate([small[:2], huge[:2] // 1000, np.zeros((1, V), dtype=np.int64)])
    for m in (small, huge, mixed):
        for beta in (1e-6, 0.01, 0.5, 2.0 ** 20):
            x = scoredref.x_of_counts(m, beta)
            assert np.array_equal(x.T.view(np.uint64), topicref.phi_of(m, beta).view(np.uint64))
            for n in (1, 10, 16):
                idx, _, _ = scoredref.scored_words_ref(x, n, 1, None)
                assert np.array_equal(idx, topicref.top_words_ref(m, n)[0]), (beta, n)
    m = rng.integers(0, 3, size=(3, 7))                                # V < n: padding
    idx, sc, _ = scoredref.scored_words_ref(scoredref.x_of_counts(m, 0.01), 10, 1, None)
    assert np.array_equal(idx, topicref.top_words_ref(m, 10)[0]) and (idx[:, 7:] == -1).all()
    assert (sc[:, 7:].view(np.uint64) == 0x7FF8000000000000).all()


def test_restatement_on_a_hand_made_matrix():
    """skipped words (either sign of zero), NaN counting, -0 == +0 by id, infinities, padding"""
    x = np.array([[1.0, -0.0], [np.nan, 0.0], [np.inf, -np.inf], [2.0, 5.0], [3.0, np.nan], [-1.0, 7.0]])
    idx, sc, nn = scoredref.scored_words_ref(x, 4, 1, None)
    assert idx.tolist() == [[2, 4, 3, 0], [5, 3, 0, 1]] and nn.tolist() == [1, 1]
    assert np.signbit(sc[1, 2]) and not np.signbit(sc[1, 3])
    wdiv = np.array([1.0, 1.0, 0.0, -0.0, 2.0, 1.0])
    idx, sc, nn = scoredref.scored_words_ref(x, 4, 2, wdiv)
    assert idx.tolist() == [[4, 0, 5, -1], [5, 0, 1, -1]] and nn.tolist() == [1, 1]
    assert sc[0, :3].tolist() == [4.5, 1.0, 1.0] and np.isnan(sc[0, 3])
    idx, sc, nn = scoredref.scored_words_ref(x, 3, 1, np.zeros(6))
    assert (idx == -1).all() and (sc.view(np.uint64) == 0x7FF8000000000000).all() and (nn == 0).all()
