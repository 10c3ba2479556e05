"""Host side of FREX and exclusivity (``llda_ecdf_ranks``, ``llda_frex_select``, lda_thesis_amd/topics.py): the restatement
(tests/frexref.py) against a brute-force definition in pure Python, ``frex_weight`` and ``frex_score``, the exported symbols, the two
structs and the scratch sizes, every refusal -- which returns before anything touches HIP, so it runs without a GPU --, and a check of
the generators: the planted inputs of the GPU tests really hold the cases those tests are there for."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import attrref
import frexref
from test_abi import declared_symbols

E_BAD_K, E_BAD_ARG = -1, -2


@pytest.fixture(scope="module")
def L():
    from lda_thesis_amd import _native
    return _native.lib()


# ---------------------------------------------------------------------------------------------- the restatement
def test_sum64_is_the_sum_of_the_other_restatements():
    rng = np.random.default_rng(1)
    for K in (1, 3, 64, 65, 130, 700):
        x = rng.standard_normal((50, K)) * 10.0 ** rng.integers(-5, 6, size=(50, K))
        assert np.array_equal(frexref.sum64(x).view(np.uint64), attrref.sum64(x).view(np.uint64))


def _brute_ranks(mat, K, mode, cand):
    """#{candidates u : v_u <= v_w} by a double loop over Python floats"""
    V = mat.shape[0]
    tot = frexref.sum64(mat[:, :K])
    c = [(cand is None or cand[w] != 0) and 0 < tot[w] < np.inf for w in range(V)]
    rank = np.zeros((K, V), dtype=np.int32)
    for k in range(K):
        v = [float(mat[w, k]) / float(tot[w]) if (mode and c[w]) else float(mat[w, k]) for w in range(V)]
        for w in range(V):
            if c[w]:
                rank[k, w] = sum(1 for u in range(V) if c[u] and v[u] <= v[w])
    return rank, sum(c)


def test_ranks_against_the_brute_force_definition():
    rng = np.random.default_rng(2)
    for V, K in ((1, 1), (2, 3), (65, 3), (120, 5), (90, 70)):
        x = frexref.x_of_counts(rng.integers(0, 3, size=(K, V)), 0.5)                    # many ties
        x[rng.random((V, K)) < 0.1] = 0.0
        if V > 10:
            x[3, 0], x[4, 0] = 0.0, -0.0                                                  # -0 == +0: one tie group
            x[5, :] = 0.0                                                                 # total 0: no candidate
            x[6, 0] = np.inf
            x[7, K - 1] = np.nan
        cand = (rng.random(V) < 0.8).astype(np.uint8)
        for mode in (0, 1):
            for cd in (None, cand):
                rank, Vc, val = frexref.ecdf_ranks_ref(x, K, mode, cd)
                want, want_vc = _brute_ranks(x, K, mode, cd)
                assert Vc == want_vc and np.array_equal(rank, want), (V, K, mode)
                isc = rank[0] > 0
                assert ((rank > 0) == isc[None, :]).all() and (rank <= Vc).all()
                assert (val[:, ~isc].view(np.uint64) == frexref.QNAN_BITS).all()
                if mode == 0:
                    assert np.array_equal(val[:, isc].view(np.uint64), np.ascontiguousarray(x.T[:, isc]).view(np.uint64))
    # the batches give the columns of the whole
    x = frexref.x_of_counts(rng.integers(0, 3, size=(7, 40)), 0.5)
    whole = frexref.ecdf_ranks_ref(x, 7, 1)[0]
    assert np.array_equal(np.concatenate([frexref.ecdf_ranks_ref(x, 7, 1, None, lo, min(3, 7 - lo))[0] for lo in range(0, 7, 3)]), whole)


def test_selection_against_sorted_fractions():
    rng = np.random.default_rng(3)
    V, Vc = 60, 50
    rf = rng.integers(0, Vc + 1, size=(2, V)).astype(np.int32)
    re = rng.integers(0, Vc + 1, size=(2, V)).astype(np.int32)
    for s, t in ((0, 1), (1, 1), (1, 2), (7, 10), (63, 64)):
        probe = np.array([[0, -1, 5, V - 1], [3, 3, -1, 59]], dtype=np.int32)
        idx, trf, tre, prf, pre = frexref.frex_select_ref(rf, re, Vc, s, t, 16, probe)
        for l in range(2):
            ws = [w for w in range(V) if rf[l, w] >= 1 and re[l, w] >= 1]
            want = sorted(ws, key=lambda w: (Fraction(s, int(re[l, w])) + Fraction(t - s, int(rf[l, w])), w))[:16]
            assert idx[l].tolist() == want
            assert trf[l].tolist() == [rf[l, w] for w in want] and tre[l].tolist() == [re[l, w] for w in want]
            for j, w in enumerate(probe[l]):
                on = w >= 0 and w in ws
                assert (prf[l, j], pre[l, j]) == ((rf[l, w], re[l, w]) if on else (0, 0))
    few = frexref.frex_select_ref(np.array([[0, 2, 3]]), np.array([[1, 0, 1]]), 3, 1, 2, 4)
    assert few[0].tolist() == [[2, -1, -1, -1]] and few[1].tolist() == [[3, 0, 0, 0]] and few[2].tolist() == [[1, 0, 0, 0]]


def test_frex_weight_and_score():
    from lda_thesis_amd import topics
    for w, want in ((0.5, (1, 2)), (0.7, (7, 10)), (1, (1, 1)), (0, (0, 1)), (63 / 64, (63, 64)), (1 / 3, (1, 3)), (0.123456, None),
                    (Fraction(7, 10), (7, 10)), ((3, 4), (3, 4))):
        f = topics.frex_weight(w)
        assert isinstance(f, Fraction) and 1 <= f.denominator <= 64 and 0 <= f <= 1
        if not isinstance(w, tuple):
            assert f == Fraction(w).limit_denominator(64) and (f.numerator, f.denominator) == frexref.weight_ref(w)
        if want:
            assert (f.numerator, f.denominator) == want
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            topics.frex_weight(bad)
    rng = np.random.default_rng(4)
    for Vc in (1, 50, 99999, 1 << 30):
        re = rng.integers(0, Vc + 1, size=(5, 40))
        rf = rng.integers(0, Vc + 1, size=(5, 40))
        re[0, :3], rf[0, :3] = Vc, (Vc, max(Vc - 1, 0), max(Vc - 2, 0))
        for s, t in ((0, 1), (1, 1), (1, 2), (7, 10), (63, 64)):
            got = topics.frex_score(re, rf, Vc, s, t)
            want = frexref.report_table(re, rf, Vc, s, t)
            assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
            assert np.array_equal(np.isnan(got), (re < 1) | (rf < 1))
    assert topics.frex_score([[10]], [[10]], 10, 1, 2)[0, 0] == 1.0                         # both ECDFs 1: FREX 1
    assert topics.frex_score([[5]], [[10]], 10, 1, 1)[0, 0] == 0.5                          # weight 1: the exclusivity ECDF


# ---------------------------------------------------------------------------------------------- the ABI
def test_symbols_structs_and_abi_number(L):
    from lda_thesis_amd import _native
    for s in ("llda_ecdf_struct_bytes", "llda_ecdf_scratch_bytes", "llda_ecdf_ranks", "llda_frex_struct_bytes", "llda_frex_scratch_bytes",
              "llda_frex_select"):
        assert s in _native.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_abi_version() == 22 == _native.ABI_VERSION
    assert L.llda_ecdf_struct_bytes() == ctypes.sizeof(_native.LldaEcdfArgs)
    assert L.llda_frex_struct_bytes() == ctypes.sizeof(_native.LldaFrexArgs)


def _ecdf(**kw):
    """a call that would be accepted, with never-dereferenced pointers; kw overrides fields"""
    from lda_thesis_amd import _native
    p = 4096
    a = dict(struct_bytes=ctypes.sizeof(_native.LldaEcdfArgs), K=12, first=0, n_labels=12, chunk=0, mode=1, mat=p, cand=p, V=100, ld=12,
             rank=p, value=p, n_cand=p, scratch=p, scratch_bytes=1 << 40)
    a.update(kw)
    return _native.LldaEcdfArgs(**a)


def _frex(**kw):
    from lda_thesis_amd import _native
    p = 4096
    a = dict(struct_bytes=ctypes.sizeof(_native.LldaFrexArgs), n_labels=12, n=10, m=10, s=1, t=2, rank_f=p, rank_e=p, probe=p, V=100, Vc=90,
             top_idx=p, top_rank_f=p, top_rank_e=p, probe_rank_f=p, probe_rank_e=p, scratch=p, scratch_bytes=1 << 40)
    a.update(kw)
    return _native.LldaFrexArgs(**a)


def test_every_refusal_of_ecdf_ranks_returns_before_hip(L):
    from lda_thesis_amd import _native
    call = lambda a: L.llda_ecdf_ranks(ctypes.byref(a), None)
    assert L.llda_ecdf_ranks(None, None) == E_BAD_ARG
    assert call(_ecdf(struct_bytes=0)) == E_BAD_ARG
    assert call(_ecdf(struct_bytes=ctypes.sizeof(_native.LldaEcdfArgs) + 8)) == E_BAD_ARG
    for K in (0, -3, _native.MAX_K + 1):
        assert call(_ecdf(K=K, ld=1 << 20)) == E_BAD_K
    assert call(_ecdf(first=-1)) == E_BAD_ARG and call(_ecdf(n_labels=-1)) == E_BAD_ARG
    assert call(_ecdf(first=1)) == E_BAD_ARG and call(_ecdf(first=12, n_labels=1)) == E_BAD_ARG and call(_ecdf(n_labels=13)) == E_BAD_ARG
    assert call(_ecdf(first=2 ** 31 - 1, n_labels=2 ** 31 - 1)) == E_BAD_ARG
    assert call(_ecdf(ld=11)) == E_BAD_ARG and call(_ecdf(ld=0)) == E_BAD_ARG and call(_ecdf(ld=-1)) == E_BAD_ARG
    for V in (0, -5, 2 ** 30 + 1):
        assert call(_ecdf(V=V)) == E_BAD_ARG
    for chunk in (1, 64, 255, 512, 4096, -256):
        assert call(_ecdf(chunk=chunk)) == E_BAD_ARG
    for mode in (-1, 2):
        assert call(_ecdf(mode=mode)) == E_BAD_ARG
    assert call(_ecdf(n_labels=0, mat=None, rank=None, scratch=None, scratch_bytes=0)) == 0       # nothing to rank: a no-op
    assert call(_ecdf(V=0, n_labels=0)) == E_BAD_ARG                                               # ... a bad size still is one
    for name in ("mat", "rank", "scratch"):
        assert call(_ecdf(**{name: None})) == E_BAD_ARG, name
    assert call(_ecdf(ld=2 ** 62)) == E_BAD_ARG                                                   # V x ld beyond an int64
    for name, align in (("mat", 8), ("value", 8), ("n_cand", 8), ("scratch", 8), ("rank", 4)):
        assert call(_ecdf(**{name: 4096 + align // 2})) == E_BAD_ARG, name
    for V, nl, chunk in ((100, 12, 0), (5000, 3, 256), (4097, 1, 0)):
        need = L.llda_ecdf_scratch_bytes(V, nl, chunk)
        assert call(_ecdf(V=V, n_labels=nl, chunk=chunk, scratch_bytes=need - 1)) == E_BAD_ARG
    assert call(_ecdf(scratch_bytes=0)) == E_BAD_ARG


def test_every_refusal_of_frex_select_returns_before_hip(L):
    from lda_thesis_amd import _native
    call = lambda a: L.llda_frex_select(ctypes.byref(a), None)
    assert L.llda_frex_select(None, None) == E_BAD_ARG
    assert call(_frex(struct_bytes=0)) == E_BAD_ARG
    assert call(_frex(struct_bytes=ctypes.sizeof(_native.LldaFrexArgs) + 8)) == E_BAD_ARG
    for nl in (-1, _native.MAX_K + 1):
        assert call(_frex(n_labels=nl)) == E_BAD_ARG
    for V in (0, -5, 2 ** 30 + 1):
        assert call(_frex(V=V)) == E_BAD_ARG
    for Vc in (0, -1, 2 ** 30 + 1):
        assert call(_frex(Vc=Vc)) == E_BAD_ARG
    for s, t in ((0, 0), (1, 0), (-1, 2), (3, 2), (1, 65), (65, 65), (0, -1)):
        assert call(_frex(s=s, t=t)) == E_BAD_ARG, (s, t)
    for n in (0, -1, 17):
        assert call(_frex(n=n)) == E_BAD_ARG
    for m in (-1, 17):
        assert call(_frex(m=m)) == E_BAD_ARG
    assert call(_frex(n_labels=0, rank_f=None, rank_e=None, scratch=None, scratch_bytes=0)) == 0  # a no-op
    for name in ("rank_f", "rank_e", "scratch"):
        assert call(_frex(**{name: None})) == E_BAD_ARG, name
    for name in ("rank_f", "rank_e", "probe", "top_idx", "top_rank_f", "top_rank_e", "probe_rank_f", "probe_rank_e"):
        assert call(_frex(**{name: 4098})) == E_BAD_ARG, name
    assert call(_frex(scratch=4100)) == E_BAD_ARG
    for V, nl, n in ((100, 12, 10), (40000, 3, 16), (16385, 1, 1)):
        need = L.llda_frex_scratch_bytes(V, nl, n)
        assert call(_frex(V=V, Vc=V, n_labels=nl, n=n, scratch_bytes=need - 1)) == E_BAD_ARG
    assert call(_frex(scratch_bytes=0)) == E_BAD_ARG


def test_scratch_bytes_codes_and_sizes(L):
    from lda_thesis_amd import _native
    eb, fb = L.llda_ecdf_scratch_bytes, L.llda_frex_scratch_bytes
    assert eb(0, 3, 0) == E_BAD_ARG and eb(-1, 3, 0) == E_BAD_ARG and eb(2 ** 30 + 1, 3, 0) == E_BAD_ARG
    assert eb(100, -1, 0) == E_BAD_ARG and eb(100, _native.MAX_K + 1, 0) == E_BAD_ARG and eb(100, 3, 128) == E_BAD_ARG
    for V in (1, 255, 256, 257, 4096, 4097, 5000, 2 ** 30):
        for nl in (0, 1, 7, 512):
            for chunk in (0, 256):
                C = chunk or _native.LABEL_CHUNK
                Vp = -(-V // C) * C
                assert eb(V, nl, chunk) == 24 * Vp * nl + 8 * V + 16 == _native.ecdf_scratch_bytes(V, nl, chunk)
    assert fb(0, 3, 10) == E_BAD_ARG and fb(2 ** 30 + 1, 3, 10) == E_BAD_ARG and fb(100, -1, 10) == E_BAD_ARG
    assert fb(100, _native.MAX_K + 1, 10) == E_BAD_ARG and fb(100, 3, 0) == E_BAD_ARG and fb(100, 3, 17) == E_BAD_ARG
    assert _native.FREX_CHUNK == 16384
    for V in (1, 16384, 16385, 40000, 2 ** 30):
        for nl in (0, 1, 512):
            for n in (1, 10, 16):
                assert fb(V, nl, n) == 12 * n * -(-V // 16384) * nl + 16 == _native.frex_scratch_bytes(V, nl, n)
    with pytest.raises(_native.NativeError):
        _native.ecdf_scratch_bytes(0, 3)
    with pytest.raises(_native.NativeError):
        _native.frex_scratch_bytes(100, 3, 17)


# ---------------------------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("s,t", [(1, 2), (7, 10)])
def test_planted_equal_costs(s, t):
    """(i) two ranked words with EQUAL cost and different (re, rf), decided by the word id, inside the list"""
    rank_f, rank_e, Vc, planted = frexref.planted_equal(s, t)
    assert len(planted) >= 5
    for a, b in planted:
        ra, rb = (int(rank_e[0, a]), int(rank_f[0, a])), (int(rank_e[0, b]), int(rank_f[0, b]))
        assert ra != rb and min(ra + rb) >= 1 and max(ra + rb) <= Vc
        assert frexref.cost(*ra, s, t) == frexref.cost(*rb, s, t)
    idx = frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, 16)[0][0].tolist()
    both = [(a, b) for a, b in planted if a in idx and b in idx]
    assert both, "no planted pair reaches the first 16"
    for a, b in both:
        assert idx.index(a) < idx.index(b)


@pytest.mark.parametrize("s,t", frexref.PLANTED_WEIGHTS)
def test_planted_near_ties_defeat_a_double_comparator(s, t):
    """(ii) at Vc = 2^30, ranks 2^30 - i with i < 700: words with DIFFERENT exact costs whose reported double has the same bits, at
    the head of the list -- so that the list by (double, id) is not the exact list"""
    rank_f, rank_e, Vc = frexref.planted_near_ties(s, t)
    V = rank_f.shape[1]
    assert Vc == 1 << 30 and 100 <= V <= 1000
    assert rank_f.min() > Vc - 700 and rank_e.min() > Vc - 700 and rank_f.max() <= Vc and rank_e.max() <= Vc
    exact = frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, 16)[0][0].tolist()
    pairs = 0
    for i, a in enumerate(exact):
        for b in exact[i + 1:]:
            ca, cb = (frexref.cost(rank_e[0, w], rank_f[0, w], s, t) for w in (a, b))
            da, db = (frexref.report(rank_e[0, w], rank_f[0, w], Vc, s, t) for w in (a, b))
            pairs += ca != cb and da == db
    print("s/t = %d/%d: V = %d, %d pairs of the first 16 with different costs and one double" % (s, t, V, pairs))
    assert pairs >= 1
    for n in (10, 16):
        assert frexref.double_order(rank_f, rank_e, Vc, s, t, n) != exact[:n], n
    if (s, t) == (1, 2):                                                                # the example of the issue
        a, b = frexref.cost(1 << 30, (1 << 30) - 2, 1, 2), frexref.cost((1 << 30) - 1, (1 << 30) - 1, 1, 2)
        assert a != b and frexref.report(1 << 30, (1 << 30) - 2, Vc, 1, 2) == frexref.report((1 << 30) - 1, (1 << 30) - 1, Vc, 1, 2)


def test_planted_tie_groups_straddle_the_chunk_boundaries():
    """(iii) in the matrix of the chunk = 256 test, a tie group of equal phi and one of equal exclusivity whose members come from
    several 256-pair chunks of the input and lie across a multiple of 256 -- and of 2048, the walk's tile -- in the sorted row"""
    x = frexref.straddle_matrix()
    V, K = x.shape
    c, tot = frexref.candidates(x, K)
    assert c.all()
    for mode in (0, 1):
        v = frexref.values(x, K, mode, c, tot)
        for k in range(K):
            groups = frexref.tie_groups(v[:, k])
            over = lambda step: [g for g in groups if (g[0] // step) != ((g[1] - 1) // step) and len(set(g[2] // 256)) >= 2]
            print("mode %d column %d: %d tie groups, %d across a multiple of 256, %d across one of 2048" % (mode, k, len(groups), len(over(256)), len(over(2048))))
            assert over(256) and over(2048), (mode, k)
