"""Host side of the sliding-window coherence (lda_thesis_amd/topics.py, llda_window_cooc): the export, the refusals -- which return
before anything touches HIP, so they run without a GPU --, ``window_count`` and ``token_csr`` on hand cases, and the three measures
on hand-made tables against values written out with math.log."""
import ctypes
import math

import numpy as np
import pytest

import topicref
import windowref
from test_abi import declared_symbols

E_BAD_K, E_BAD_ARG = -1, -2
U = 2.0 ** -52


@pytest.fixture(scope="module")
def L():
    from lda_thesis_amd import _native
    return _native.lib()


def test_symbol_is_exported_and_the_abi_number_stays(L):
    from lda_thesis_amd import _native
    assert "llda_window_cooc" in _native.EXPORTS and "llda_window_cooc" in declared_symbols() and hasattr(L, "llda_window_cooc")
    assert L.llda_abi_version() == 22 == _native.ABI_VERSION
    header = open(_native.os.path.join(_native.os.path.dirname(_native._HERE), "include", "llda_gibbs.h")).read()
    assert "#define LLDA_WINDOW_MAX %d\n" % _native.WINDOW_MAX in header and _native.WINDOW_MAX == 65535
    assert "#define LLDA_WINDOW_MAX_WAVES %d\n" % _native.WINDOW_MAX_WAVES in header
    assert "#define LLDA_WINDOW_AGG_MIN_DOCS %d\n" % _native.WINDOW_AGG_MIN_DOCS in header


def test_refusals_come_before_the_device(L):
    from lda_thesis_amd import _native
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below is turned down on the host
    call = lambda off=p, tok=p, D=3, V=100, K=12, n=10, s=10, mo=p, m=p, out=p: L.llda_window_cooc(off, tok, D, V, K, n, s, mo, m, out, None)
    assert call(s=-1) == E_BAD_ARG and call(s=_native.WINDOW_MAX + 1) == E_BAD_ARG
    assert call(n=0) == E_BAD_ARG and call(n=17) == E_BAD_ARG
    assert call(K=0) == E_BAD_K and call(K=_native.MAX_K + 1) == E_BAD_K
    assert call(V=0) == E_BAD_ARG and call(D=-1) == E_BAD_ARG
    for name in ("off", "tok", "mo", "m", "out"):
        assert call(**{name: None}) == E_BAD_ARG, name
    assert call(off=ctypes.c_void_p(4100)) == E_BAD_ARG and call(tok=ctypes.c_void_p(4098)) == E_BAD_ARG     # misaligned
    assert call(D=0) == 0 and call(D=0, off=None, tok=None, mo=None, m=None, out=None) == 0                 # a no-op
    assert call(D=0, s=-1) == E_BAD_ARG and call(D=0, K=0) == E_BAD_K


def test_window_count_and_token_csr_on_hand_cases():
    import torch
    from lda_thesis_amd import topics
    s = 4
    lens = [0, 1, s - 1, s, s + 1, 9]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert topics.window_count(off, s) == 0 + 1 + 1 + 1 + 2 + 6
    assert topics.window_count(off, 0) == 5                      # the non-empty documents
    assert topics.window_count(off, 1) == sum(lens)
    assert topics.window_count(torch.from_numpy(off), s) == 11
    assert topics.window_count(off[:1], s) == 0 and isinstance(topics.window_count(off, s), int)
    for w in (0, 1, 2, s, 100):
        assert topics.window_count(off, w) == windowref.window_count_ref(off, w)
    with pytest.raises(ValueError):
        topics.window_count(off, -1)
    with pytest.raises(ValueError):
        topics.window_count(off, 65536)
    t2i = {"a": 0, "b": 1, "c": 2}
    tok_off, tok = topics.token_csr([["a", "x", "c"], [], ["b", "b", "a", "?"]], t2i)
    assert tok_off.dtype == np.int64 and tok.dtype == np.int32
    assert tok_off.tolist() == [0, 3, 3, 7] and tok.tolist() == [0, -1, 2, 1, 1, 0, -1]      # the unknown token keeps its place
    tok_off, tok = topics.token_csr([], t2i)
    assert tok_off.tolist() == [0] and tok.shape == (0,)


def test_the_restatement_on_a_count_made_by_hand():
    """windows of 3 over a b - a a: {a, b}, {b, a}, {a}: the unknown token holds its place"""
    top = np.array([[0, 1]])
    off, tok = np.array([0, 5]), np.array([0, 1, -1, 0, 0])
    assert windowref.window_ref(off, tok, top, 3)[0].tolist() == [[3, 0], [2, 2]]
    assert windowref.window_ref(off, tok, top, 1)[0].tolist() == [[3, 0], [0, 1]]            # token frequencies
    assert windowref.window_ref(off, tok, top, 0)[0].tolist() == [[1, 0], [1, 1]]
    assert windowref.window_ref(off, tok, top, 5)[0].tolist() == [[1, 0], [1, 1]]
    rng = np.random.default_rng(4)
    doc_off, word = topicref.mixed_corpus(rng, 40, rng.integers(0, 30, size=50))
    lists = topicref.random_lists(rng, 9, 6, 40, holes=0.1)
    assert np.array_equal(windowref.window_ref(doc_off, word, lists, 0), topicref.cooc_ref(doc_off, word, lists))


def hand_table():
    co = np.zeros((4, 3, 3), dtype=np.int64)
    co[0] = [[4, 0, 0], [2, 5, 0], [0, 1, 2]]          # ordinary; the pair (2, 0) never met
    co[1] = [[4, 0, 0], [2, 0, 0], [0, 0, 2]]          # rank 1 listed but in no window
    co[2] = [[4, 0, 0], [0, 0, 0], [0, 0, 0]]          # one listed word only (with the mask below)
    co[3] = [[3, 0, 0], [0, 0, 0], [1, 0, 5]]          # ranks 0 and 2 listed, rank 1 a hole
    listed = np.array([[5, 6, 7], [5, 6, 7], [5, -1, -1], [9, -1, 2]])
    return co, listed, 8


def test_the_three_measures_on_a_hand_made_table():
    """Tolerance, derived (windowref.pair_mean_ref): numpy and the expressions below feed the same doubles to the logarithm; two
    logarithms differ by at most 2 ulp, a quotient of two by 5, and a sum of three terms and its division by 3 add 3 more: 8 ulp of the
    sum of the terms' magnitudes, divided by 3.  c_v: the first-order bound of windowref.c_v_ref."""
    from lda_thesis_amd import topics
    co, listed, N = hand_table()
    E = topics.EPS
    assert E == 1e-12 and topics.DEFAULT_WINDOW == {"c_v": 110, "c_uci": 10, "c_npmi": 10}
    pmi10 = math.log((2 / 8 + E) / ((5 / 8) * (4 / 8)))
    pmi20 = math.log((0 / 8 + E) / ((2 / 8) * (4 / 8)))
    pmi21 = math.log((1 / 8 + E) / ((2 / 8) * (5 / 8)))
    uci = topics.c_uci(co, N, listed=listed)
    assert uci.dtype == np.float64 and uci.shape == (4,)
    assert abs(uci[0] - (pmi10 + pmi20 + pmi21) / 3) <= 8 * U * (abs(pmi10) + abs(pmi20) + abs(pmi21)) / 3
    nl10, nl20, nl21 = pmi10 / -math.log(2 / 8 + E), pmi20 / -math.log(0 / 8 + E), pmi21 / -math.log(1 / 8 + E)
    npmi = topics.c_npmi(co, N, listed=listed)
    assert abs(npmi[0] - (nl10 + nl20 + nl21) / 3) <= 8 * U * (abs(nl10) + abs(nl20) + abs(nl21)) / 3
    assert -1.0 <= nl20 < -0.9                                   # a pair that never met: close to -1
    pmi3 = math.log((1 / 8 + E) / ((5 / 8) * (3 / 8)))
    assert abs(uci[3] - pmi3) <= 4 * U * abs(pmi3)
    assert abs(npmi[3] - pmi3 / -math.log(1 / 8 + E)) <= 7 * U * abs(pmi3 / -math.log(1 / 8 + E))
    # c_v of topic 0, written out: the 3 x 3 matrix of nlr with p_aa = p_a, the sum of its rows, three cosines
    p = [4 / 8, 5 / 8, 2 / 8]
    M = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        M[a][a] = math.log((p[a] + E) / (p[a] * p[a])) / -math.log(p[a] + E)
    M[1][0] = M[0][1] = nl10
    M[2][0] = M[0][2] = nl20
    M[2][1] = M[1][2] = nl21
    v = [M[0][b] + M[1][b] + M[2][b] for b in range(3)]
    nv = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    cos = [(M[a][0] * v[0] + M[a][1] * v[1] + M[a][2] * v[2]) / (math.sqrt(M[a][0] ** 2 + M[a][1] ** 2 + M[a][2] ** 2) * nv) for a in range(3)]
    want, bound = windowref.c_v_ref(co[0], N, np.ones(3, dtype=bool))
    assert abs(want - (cos[0] + cos[1] + cos[2]) / 3) <= bound and bound < 1e-13
    cv = topics.c_v(co, N, listed=listed)
    print("c_v by hand %.17g, topics %.17g, bound %.3g" % ((cos[0] + cos[1] + cos[2]) / 3, cv[0], bound))
    assert abs(cv[0] - (cos[0] + cos[1] + cos[2]) / 3) <= bound
    assert 0.0 < cv[0] < 1.0
    # the NaN rule: a listed word no window holds, fewer than two listed words; a hole is no word -- unless the mask is missing
    for got in (uci, npmi, cv):
        assert np.isnan(got[1]) and np.isnan(got[2]) and np.isfinite(got[0]) and np.isfinite(got[3])
    assert np.isnan(topics.c_v(co, N)[3]) and np.isnan(topics.c_uci(co, N)[3]) and np.isnan(topics.c_npmi(co, N)[3])
    assert np.isnan(topics.c_v(np.zeros((2, 3, 3), dtype=np.int64), 0)).all()        # no window at all: nothing raises
    for name, got in (("c_v", cv), ("c_uci", uci), ("c_npmi", npmi)):
        assert np.array_equal(topics.window_coherence(co, N, name, listed=listed), got, equal_nan=True)
        ref, bound = windowref.coherence_ref(co, N, name, listed)
        assert np.array_equal(np.isnan(ref), np.isnan(got))
        ok = ~np.isnan(ref)
        assert (np.abs(got[ok] - ref[ok]) <= bound[ok]).all()
    with pytest.raises(ValueError):
        topics.window_coherence(co, N, "umass")
    with pytest.raises(ValueError):
        topics.window_coherence(co, N, "c_p")


def test_a_cosine_with_a_zero_norm_counts_zero():
    """(p_a + EPS) / (p_a p_a) > 1 for every p_a <= 1, so no count table gives a zero vector: the rule is met on the matrix itself"""
    from lda_thesis_amd import topics
    assert topics._cosine_mean(np.zeros((3, 3))) == 0.0
    M = np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.5], [0.0, 0.5, 1.0]])                 # u_0 = 0; u_1 and u_2 mirror each other about v
    want = 2 * (1.5 * 1.5) / (math.sqrt(1.25) * math.sqrt(4.5)) / 3
    assert abs(topics._cosine_mean(M) - want) <= 8 * U * want
    assert abs(windowref.cosine_mean_ref(M.tolist())[0] - want) <= 8 * U * want
    assert topics._cosine_mean(np.array([[1.0, -1.0], [-1.0, 1.0]])) == 0.0          # v = 0


def test_the_measures_against_the_plain_loops_on_random_tables():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(12)
    N = 5000
    for n in (2, 3, 10, 16):
        K = 20
        df = rng.integers(1, N + 1, size=(K, n))
        co = np.zeros((K, n, n), dtype=np.int64)
        for k in range(K):
            for i in range(n):
                co[k, i, i] = df[k, i]
                for j in range(i):
                    co[k, i, j] = rng.integers(0, min(df[k, i], df[k, j]) + 1)
        co[0][np.tril_indices(n)] = N                                  # every window holds every word
        co[1][np.tril_indices(n, -1)] = 0                              # no pair ever met
        listed = np.where(rng.random((K, n)) < 0.15, -1, 1)
        listed[:2] = 1
        for name in ("c_v", "c_uci", "c_npmi"):
            got = topics.window_coherence(co, N, name, listed=listed)
            ref, bound = windowref.coherence_ref(co, N, name, listed)
            assert np.array_equal(np.isnan(ref), np.isnan(got)) and np.isfinite(got).any()
            ok = ~np.isnan(ref)
            print(name, n, "largest |d| / bound:", float(np.max(np.abs(got[ok] - ref[ok]) / bound[ok])))
            assert (np.abs(got[ok] - ref[ok]) <= bound[ok]).all()


def test_coherence_still_knows_umass_and_npmi_only():
    from lda_thesis_amd import topics
    co, listed, N = hand_table()
    with pytest.raises(ValueError):
        topics.coherence(co, N, "c_v")
    with pytest.raises(ValueError):
        topics.coherence(co, N, "c_npmi")
    assert np.isfinite(topics.coherence(co, N, "umass", listed=listed)[0])
