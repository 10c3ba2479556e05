"""Host side of the topic summaries (lda_thesis_amd/topics.py, llda_top_words / llda_word_cooc): argument validation of the
entry points -- which returns before anything touches HIP, so it runs without a GPU --, the claim the device pass rests on (the
order of a topic's words by count IS their order by phi), the host formulas and the membership table."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
import topicref

E_BAD_K, E_BAD_ARG = -1, -2


@pytest.fixture(scope="module")
def L():
    from lda_thesis_amd import _native
    return _native.lib()


def test_symbols_are_exported_and_the_abi_number_stays(L):
    from lda_thesis_amd import _native
    for name in ("llda_top_words", "llda_top_words_scratch_bytes", "llda_word_cooc"):
        assert name in _native.EXPORTS
        assert getattr(L, name) is not None
    assert L.llda_abi_version() == 22 == _native.ABI_VERSION
    with open(os.path.join(ROOT, "include", "llda_gibbs.h")) as f:
        assert "#define LLDA_TOPW_CHUNK_ROWS %d\n" % _native.TOPW_CHUNK_ROWS in f.read()


def test_argument_validation_returns_before_hip(L):
    from lda_thesis_amd import _native
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below is turned down on the host
    big = 1 << 40
    top = lambda n_kw=p, V=100, K=12, n=10, idx=p, cnt=p, scr=p, nbytes=big: L.llda_top_words(n_kw, V, K, n, idx, cnt, scr, nbytes, None)
    assert top(n_kw=None) == E_BAD_ARG and top(scr=None) == E_BAD_ARG
    assert top(n=0) == E_BAD_ARG and top(n=17) == E_BAD_ARG and top(n=-1) == E_BAD_ARG
    assert top(V=0) == E_BAD_ARG and top(V=-5) == E_BAD_ARG and top(V=2 ** 31) == E_BAD_ARG
    assert top(K=0) == E_BAD_K and top(K=_native.MAX_K + 1) == E_BAD_K and top(K=-3) == E_BAD_K
    assert top(nbytes=0) == E_BAD_ARG             # scratch too small
    assert top(n_kw=ctypes.c_void_p(4100)) == E_BAD_ARG     # n_kw not 16-byte aligned
    sb = L.llda_top_words_scratch_bytes
    assert sb(0, 12, 10) == E_BAD_ARG and sb(100, 12, 0) == E_BAD_ARG and sb(100, 12, 17) == E_BAD_ARG
    assert sb(100, 0, 10) == E_BAD_K and sb(100, _native.MAX_K + 1, 10) == E_BAD_K
    for K in (1, 12, 512, 1031, _native.MAX_K):
        KP = _native.layout_init(K)["KP"]
        for V in (1, 255, 256, 257, 5000):
            for n in (1, 10, 16):
                b = sb(V, K, n)
                chunks = -(-V // _native.TOPW_CHUNK_ROWS)
                assert b > 0 and b % (chunks * KP * n * 8) == 0 and b // (chunks * KP * n * 8) in (1, 2, 3, 4)
                assert top(V=V, K=K, n=n, nbytes=b - 1) == E_BAD_ARG
    with pytest.raises(_native.NativeError):
        _native.top_words_scratch_bytes(100, 0, 10)
    co = lambda off=p, word=p, D=3, V=100, K=12, n=10, mo=p, m=p, out=p: L.llda_word_cooc(off, word, D, V, K, n, mo, m, out, None)
    assert co(D=-1) == E_BAD_ARG and co(V=0) == E_BAD_ARG and co(n=0) == E_BAD_ARG and co(n=17) == E_BAD_ARG
    assert co(K=0) == E_BAD_K and co(K=_native.MAX_K + 1) == E_BAD_K
    for name in ("off", "word", "mo", "m", "out"):
        assert co(**{name: None}) == E_BAD_ARG
    assert co(D=0) == 0 and co(D=0, off=None, word=None, mo=None, m=None, out=None) == 0      # a no-op
    assert co(D=0, K=0) == E_BAD_K and co(D=0, n=17) == E_BAD_ARG


def _check_order(n_k_v, beta, n):
    idx, cnt = topicref.top_words_ref(n_k_v, n)
    phi = topicref.phi_of(n_k_v, beta)
    m = min(n, n_k_v.shape[1])
    for k in range(n_k_v.shape[0]):
        want = np.argsort(-phi[k], kind="stable")[:n]
        assert np.array_equal(idx[k, :m], want), (k, beta)
        assert np.array_equal(cnt[k, :m], np.asarray(n_k_v)[k, want])
    assert (idx[:, m:] == -1).all() and (cnt[:, m:] == 0).all()


@pytest.mark.parametrize("name", ["tiny_k12", "tiny_k130", "tiny_k1031"])
def test_count_order_is_phi_order_on_the_goldens(name):
    g = load_golden(name)
    for beta in (1e-6, float(g["beta"]), 0.5, 2.0 ** 20):
        for s in range(1, int(g["sweeps"]) + 1):
            _check_order(g["o3_s%d_n_k_v" % s].astype(np.int64), beta, 10)


def test_count_order_is_phi_order_on_hard_matrices():
    rng = np.random.default_rng(5)
    V = 700
    small = rng.integers(0, 3, size=(6, V))                            # {0, 1, 2}: ties in every list
    small[3] = 0                                                       # an all-zero topic
    huge = rng.integers(0, topicref.INT32_MAX, size=(4, V), endpoint=True)
    huge[0, :40] = topicref.INT32_MAX - rng.integers(0, 3, size=40)    # neighbours at the top of the range, with ties
    huge[1, 5] = huge[1, 600] = topicref.INT32_MAX
    mixed = np.concatenate([small[:2], huge[:2] // 1000, np.zeros((1, V), dtype=np.int64)])
    for m in (small, huge, mixed):
        for beta in (1e-6, 0.01, 0.5, 2.0 ** 20):
            for n in (1, 10, 16):
                _check_order(m, beta, n)
    _check_order(rng.integers(0, 3, size=(3, 7)), 0.01, 10)           # V < n: padding


def test_umass_and_npmi_against_a_per_pair_loop():
    """Bound, derived: a topic's value sums at most 120 terms, each ONE correctly rounded division and ONE logarithm (npmi: the
    quotient of two such), so the vectorised sum and the loop differ by at most (pairs + 4) * 2^-52 * sum|term|."""
    from lda_thesis_amd import topics
    rng = np.random.default_rng(11)
    D = 1000
    for n in (2, 3, 10, 16):
        K = 30
        df = rng.integers(1, D + 1, size=(K, n))
        co = np.zeros((K, n, n), dtype=np.int64)
        for k in range(K):
            for i in range(n):
                co[k, i, i] = df[k, i]
                for j in range(i):
                    co[k, i, j] = rng.integers(0, min(df[k, i], df[k, j]) + 1)
        co[0] = D                                                      # every document holds every word
        co[1][np.tril_indices(n, -1)] = 0                              # no pair ever met
        on = np.ones(n, dtype=bool)
        for eps in (1.0, 1e-12):
            got = topics.umass(co, eps)
            for k in range(K):
                want, mag, pairs = topicref.umass_ref(co[k], eps, on)
                assert pairs == n * (n - 1) // 2
                print("umass n=%d k=%d |d|=%.3g bound=%.3g" % (n, k, abs(got[k] - want), (pairs + 4) * 2.0 ** -52 * mag))
                assert abs(got[k] - want) <= (pairs + 4) * 2.0 ** -52 * mag
        got = topics.npmi(co, D)
        for k in range(K):
            want, mag, pairs = topicref.npmi_ref(co[k], D, on)
            assert abs(got[k] - want) <= (pairs + 4) * 2.0 ** -52 * mag
        assert got[0] == 1.0 and got[1] == -1.0


def test_nan_rule_and_the_minus_one_convention_on_a_hand_made_table():
    from lda_thesis_amd import topics
    D = 8
    co = np.zeros((5, 3, 3), dtype=np.int64)
    co[0] = [[4, 0, 0], [2, 4, 0], [0, 1, 2]]          # ordinary; the pair (2, 0) never met
    co[1] = [[4, 0, 0], [2, 0, 0], [0, 0, 2]]          # rank 1 listed but in no document
    co[2] = [[4, 0, 0], [0, 0, 0], [0, 0, 0]]          # one listed word only (with the mask below)
    co[3] = [[3, 0, 0], [0, 0, 0], [1, 0, 5]]          # ranks 0 and 2 listed, rank 1 a hole
    co[4] = 0                                          # nothing listed
    listed = np.array([[5, 6, 7], [5, 6, 7], [5, -1, -1], [9, -1, 2], [-1, -1, -1]])
    u = topics.umass(co, 1.0, listed=listed)
    want0 = math.log(3 / 4) + math.log(1 / 4) + math.log(2 / 4)
    assert abs(u[0] - want0) <= 7 * 2.0 ** -52 * abs(want0) * 3
    assert np.isnan(u[1]) and np.isnan(u[2]) and np.isnan(u[4])
    assert abs(u[3] - math.log(2 / 3)) <= 5 * 2.0 ** -52
    assert np.isnan(topics.umass(co, 1.0)[3])          # without the mask the hole counts as a word no document holds
    p = topics.npmi(co, D, listed=listed)
    t10 = math.log((2 * 8) / (4 * 4)) / -math.log(2 / 8)
    t21 = math.log((1 * 8) / (2 * 4)) / -math.log(1 / 8)
    assert abs(p[0] - (t10 - 1.0 + t21) / 3) <= 7 * 2.0 ** -52 * 3
    assert np.isnan(p[1]) and np.isnan(p[2]) and np.isnan(p[4])
    assert abs(p[3] - math.log((1 * 8) / (5 * 3)) / -math.log(1 / 8)) <= 5 * 2.0 ** -52
    assert np.array_equal(np.isnan(topics.coherence(co, D, "npmi", listed=listed)), np.isnan(p))
    with pytest.raises(ValueError):
        topics.coherence(co, D, "c_v")


def test_membership_against_a_dict_of_lists():
    import torch
    from lda_thesis_amd import topics
    V = 50
    top = np.array([[7, 3, -1, 49], [3, -1, 7, 0], [49, 7, 3, -1], [-1, -1, -1, -1], [12, 13, 14, 15]])   # 3 and 7: three topics
    memb_off, memb = topics.membership(top, V, device="cpu")
    assert memb_off.dtype == torch.int32 and memb.dtype == torch.int32 and tuple(memb_off.shape) == (V + 1,)
    off, m = memb_off.numpy(), memb.numpy()
    want = topicref.membership_ref(top)
    assert off[0] == 0 and off[-1] == m.shape[0] == int((top >= 0).sum())
    for w in range(V):
        assert sorted(m[off[w]:off[w + 1]].tolist()) == want.get(w, []), w
    assert sorted(m[off[3]:off[4]].tolist()) == [1, 16, 34]
    rng = np.random.default_rng(2)
    top = topicref.random_lists(rng, 40, 16, 200, holes=0.2)
    memb_off, memb = topics.membership(torch.from_numpy(top), 200)
    off, m = memb_off.numpy(), memb.numpy()
    want = topicref.membership_ref(top)
    for w in range(200):
        assert sorted(m[off[w]:off[w + 1]].tolist()) == want.get(w, [])
    with pytest.raises(ValueError):
        topics.membership(np.array([[1, 50]]), 50, device="cpu")
    off, m = topics.membership(np.full((3, 4), -1), 9, device="cpu")
    assert off.numpy().tolist() == [0] * 10 and m.numel() == 0
