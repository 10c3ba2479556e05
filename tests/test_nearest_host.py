"""llda_nearest_rows without a GPU: the exported symbols and the struct, the entry point's refusals, the CPU restatement
(tests/nearref.py) on the values whose order the header spells out, and the host helpers of lda_thesis_amd.similar."""
import ctypes
import math

import numpy as np
import pytest

import nearref as ref
from lda_thesis_amd import similar

BAD_ARG = -2


def test_symbols_and_struct():
    from lda_thesis_amd import _native
    from test_abi import declared_symbols
    L = _native.lib()
    assert L.llda_abi_version() == 22
    for s in ("llda_nearest_rows", "llda_nearest_scratch_bytes", "llda_nearest_struct_bytes"):
        assert s in _native.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_nearest_struct_bytes() == ctypes.sizeof(_native.LldaNearestArgs)
    assert (_native.NEAREST_MAX_N, _native.NEAREST_TILE, _native.NEAREST_KSTEP) == (16, 128, 16) and similar.MAX_N == 16


def test_refusals_come_before_the_device():
    """every refusal of the header, on a machine without a device (the pointers below are never dereferenced on the host)"""
    from lda_thesis_amd import _native
    L = _native.lib()

    def call(**kw):
        a = _native.LldaNearestArgs()
        a.struct_bytes = ctypes.sizeof(a)
        a.a, a.b, a.exclude, a.top_idx, a.top_val, a.n_nan, a.scratch = 4096, 8192, 12288, 16384, 20480, 24576, 28672
        a.Q, a.D, a.L, a.lda, a.ldb, a.n, a.chunks, a.row_base = 0, 9, 4, 5, 4, 3, 0, 7
        a.scratch_bytes = 1 << 20
        for k, v in kw.items():
            setattr(a, k, v)
        return L.llda_nearest_rows(ctypes.byref(a), None)

    assert call() == 0                                                  # Q == 0: nothing to do, nothing touched
    assert L.llda_nearest_rows(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(_native.LldaNearestArgs) + 8) == BAD_ARG
    for name in ("a", "b", "scratch"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("exclude", "top_idx", "top_val", "n_nan"):
        assert call(**{name: None}) == 0, name
    for n in (0, -1, 17):
        assert call(n=n) == BAD_ARG, n
    assert call(n=1) == 0 and call(n=16) == 0
    assert call(L=0) == BAD_ARG and call(L=-3) == BAD_ARG
    assert call(lda=3) == BAD_ARG and call(ldb=3) == BAD_ARG
    assert call(L=2 ** 31 - 1, lda=2 ** 31 - 1, ldb=2 ** 31) == 0       # L is not bound by LLDA_MAX_K
    assert call(Q=-1) == BAD_ARG and call(D=-1) == BAD_ARG and call(chunks=-1) == BAD_ARG and call(row_base=-1) == BAD_ARG
    assert call(row_base=2 ** 63 - 5) == BAD_ARG                        # row_base + D leaves an int64
    for name in ("a", "b", "exclude", "top_idx", "top_val", "n_nan", "scratch"):
        assert call(**{name: 4100}) == BAD_ARG, name                   # not 8-byte aligned
    assert call(a=4104, b=8200, lda=7, ldb=9) == 0                      # 8-byte aligned rows with odd ld are taken
    # scratch too small: refused for the sizes of a real call too (Q > 0), still before the device
    need = _native.nearest_scratch_bytes(5, 9, 3, 2)
    assert need >= 5 * 2 * (16 * 3 + 8)
    assert call(Q=5, chunks=2, scratch_bytes=need - 1) == BAD_ARG and call(Q=5, scratch_bytes=0) == BAD_ARG


def test_scratch_bytes():
    from lda_thesis_amd import _native
    L = _native.lib()
    sb = _native.nearest_scratch_bytes
    assert sb(0, 0, 1) > 0 and sb(4, 0, 16) > 0                         # an allocation of that size has an address
    assert sb(3, 5, 2, 9) == sb(3, 5, 2, 5)                             # chunks are capped at D
    assert sb(3, 500, 2, 2) < sb(3, 500, 2, 3)
    assert sb(1024, 10 ** 6, 10) < 64 << 20                             # the flagship call: tens of megabytes, not Q x D scores
    for bad in ((-1, 5, 2, 0), (3, -1, 2, 0), (3, 5, 0, 0), (3, 5, 17, 0), (3, 5, 2, -1)):
        assert L.llda_nearest_scratch_bytes(*bad) == BAD_ARG, bad
    assert L.llda_nearest_scratch_bytes(2 ** 60, 2 ** 60, 16, 0) == BAD_ARG


def test_reference_fma_is_one_rounding():
    x, y = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30                          # x * y = 1 - 2^-60: rounds to 1.0, the residual shows fused
    assert x * y == 1.0 and ref.fma(x, y, -1.0) == -2.0 ** -60
    assert ref.fma(3.0, 5.0, 7.0) == 22.0 and ref.fma(2.0 ** -600, 2.0 ** -470, 0.0) == 2.0 ** -1070       # a denormal product
    assert ref.fma(1e200, 1e200, 0.0) == math.inf and ref.fma(-1e200, 1e200, 0.0) == -math.inf
    assert math.isnan(ref.fma(math.inf, 0.0, 1.0)) and math.isnan(ref.fma(math.inf, 1.0, -math.inf))
    assert ref.fma(math.inf, -2.0, 5.0) == -math.inf and ref.fma(1.0, 2.0, math.inf) == math.inf
    assert math.copysign(1.0, ref.fma(-0.0, 3.0, 0.0)) == 1.0 and math.copysign(1.0, ref.fma(-0.0, 3.0, -0.0)) == -1.0
    assert math.copysign(1.0, ref.fma(2.0, 3.0, -6.0)) == 1.0
    rng = np.random.default_rng(3)
    for a, b, c in rng.standard_normal((200, 3)):                       # against exact arithmetic in float128-free form: integers
        ia, ib, ic = int(a * 2 ** 20), int(b * 2 ** 20), int(c * 2 ** 40)
        assert ref.fma(float(ia), float(ib), float(ic)) == float(ia * ib + ic)


def test_reference_order():
    """-0.0 == +0.0 (the id decides), +-inf ordinary, NaN counted and left out, exclude left out, padding -1 / 0.0"""
    sc = np.array([[0.0, -0.0, np.inf, np.nan, -np.inf, 0.0, 1.0, np.nan],
                   [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0]])
    idx, val, nan = ref.select(sc, 8, row_base=100, exclude=[102, 999])
    assert list(idx[0]) == [106, 100, 101, 105, 104, -1, -1, -1] and list(nan) == [2, 0]
    assert list(val[0][:5]) == [1.0, 0.0, 0.0, 0.0, -np.inf] and math.copysign(1.0, val[0][2]) == -1.0      # the stored bits stay
    assert np.all(val[0][5:] == 0.0) and list(idx[1]) == list(range(100, 108))
    idx, val, nan = ref.select(sc, 2, row_base=100)
    assert list(idx[0]) == [102, 106] and list(val[0]) == [np.inf, 1.0]


def test_merge_lists_of_a_split_is_the_whole():
    rng = np.random.default_rng(11)
    sc = rng.integers(0, 4, size=(6, 40)).astype(np.float64)            # few distinct scores: ties everywhere, across every split
    sc[2, 5] = np.nan
    sc[3] = 1.0
    for n in (1, 5, 16):
        want = ref.select(sc, n, row_base=1000)
        for cuts in ((0, 40), (0, 13, 40), (0, 1, 2, 40), (0, 20, 20, 40), (0, 7, 19, 33, 40)):
            parts = [ref.select(sc[:, lo:hi], n, row_base=1000 + lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
            for order in (parts, parts[::-1]):
                idx, val = similar.merge_lists([p[0] for p in order], [p[1] for p in order], n)
                assert np.array_equal(idx, want[0]) and np.array_equal(val, want[1])
    idx, val = similar.merge_lists([np.full((2, 3), -1)], [np.zeros((2, 3))], 4)
    assert np.all(idx == -1) and np.all(val == 0.0) and idx.shape == (2, 4)


def test_knn_votes_equals_a_plain_loop():
    rng = np.random.default_rng(12)
    labs = (rng.random((30, 7)) < 0.3).astype(np.float64)
    idx = rng.integers(0, 30, size=(9, 6))
    val = rng.random((9, 6))
    idx[4, 3:] = -1
    for k in (1, 3, 6, 10):
        want = np.zeros((9, 7))
        for q in range(9):
            for c in range(7):
                v = 0.0
                for j in range(min(k, 6)):
                    if idx[q, j] >= 0:
                        v = v + val[q, j] * labs[idx[q, j], c]
                want[q, c] = v
        assert np.array_equal(similar.knn_votes(idx, val, labs, k), want)


def test_affinity_rows_measures():
    import torch
    x = torch.tensor([[0.25, 0.75, 0.0], [3.0, 4.0, 0.0]], dtype=torch.float64)
    assert torch.equal(similar.affinity_rows(x, "hellinger"), torch.sqrt(x))
    assert torch.equal(similar.affinity_rows(x, "dot"), x) and similar.affinity_rows(x, "dot") is not x
    assert torch.allclose(similar.affinity_rows(x, "cosine")[1], torch.tensor([0.6, 0.8, 0.0], dtype=torch.float64))
    with pytest.raises(ValueError):
        similar.affinity_rows(x, "jensen-shannon")
