"""llda_nearest_rows on the device through the C ABI against its CPU restatement (tests/nearref.py), bit for bit in top_idx, top_val
(compared as uint64) and n_nan.  The kernel's tile is 128 queries x 128 rows and its k-loop steps by 16 columns; a score depends on its
two rows only, so one exact score matrix per case serves every sub-shape, every n and every ``chunks``."""
import functools

import numpy as np
import pytest

import nearref as ref

pytestmark = pytest.mark.gpu

T = 128                                                                 # LLDA_NEAREST_TILE (both tile edges)
S = 16                                                                  # LLDA_NEAREST_KSTEP
GUARD = 5


def device_run(a, b, n, row_base=0, exclude=None, chunks=0, layout="odd", want=("idx", "val", "nan")):
    """llda_nearest_rows through the binding.  layout "odd": odd ld, bases 8 but not 16 bytes aligned, NaN in the columns >= L;
    "vec": even ld, 16-byte aligned bases (the 16-byte loads).  Every output sits between guard words, which are checked."""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda")
    Q, L = a.shape
    D = b.shape[0]

    def place(x):
        rows = x.shape[0]
        ld = L + 1 + (L % 2) if layout == "odd" else L + 2 - (L % 2)
        off = 1 if layout == "odd" else 2
        host = np.full((rows * ld + off + 3,), np.nan)
        view = host[off:off + rows * ld].reshape(rows, ld)
        view[:, :L] = x
        t = torch.from_numpy(host).to(dev)
        inner = t[off:off + max(rows, 1) * ld] if rows else t[off:off + 1]
        assert inner.data_ptr() % 16 == (8 if layout == "odd" else 0) and ld % 2 == (1 if layout == "odd" else 0)
        return t, inner, ld

    ta, va, lda = place(a)
    tb, vb, ldb = place(b)

    def out(shape, dtype, fill):
        size = int(np.prod(shape))
        t = torch.full((size + 2 * GUARD,), fill, dtype=dtype, device=dev)
        return t, t[GUARD:GUARD + max(size, 1)]

    g_idx, v_idx = out((Q, n), torch.int64, -77)
    g_val, v_val = out((Q, n), torch.float64, -77.0)
    g_nan, v_nan = out((Q,), torch.int64, -77)
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, dtype=np.int64)).to(dev)
    nbytes = _native.nearest_scratch_bytes(Q, D, n, chunks)
    scratch = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
    _native.nearest_rows(va, vb, Q, D, L, n, scratch[:nbytes], lda=lda, ldb=ldb, row_base=row_base, exclude=ex, chunks=chunks,
                         top_idx=v_idx if "idx" in want else None, top_val=v_val if "val" in want else None,
                         n_nan=v_nan if "nan" in want else None)
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0xA5).all()), "scratch written beyond llda_nearest_scratch_bytes"
    res = []
    for name, guard, shape in (("idx", g_idx, (Q, n)), ("val", g_val, (Q, n)), ("nan", g_nan, (Q,))):
        h = guard.cpu().numpy()
        size = int(np.prod(shape))
        assert np.all(h[:GUARD] == -77) and np.all(h[GUARD + size:] == -77), "guard words around %s" % name
        if name not in want:
            assert np.all(h == -77), "%s was NULL and is written" % name
        res.append(h[GUARD:GUARD + size].reshape(shape))
    return tuple(res)


def check(got, want, what=""):
    idx, val, nan = got
    w_idx, w_val, w_nan = want
    assert np.array_equal(idx, w_idx), "%s top_idx\n%s\n%s" % (what, idx, w_idx)
    assert np.array_equal(val.view(np.uint64), w_val.view(np.uint64)), "%s top_val" % what
    assert np.array_equal(nan, w_nan), "%s n_nan" % what


def _dists(rng, rows, L):
    """square roots of sparse-ish distributions: what fold-in loads look like"""
    x = rng.gamma(0.3, size=(rows, L)) * (rng.random((rows, L)) < 0.7)
    x[:, 0] += 1e-3
    return np.sqrt(x / x.sum(axis=1, keepdims=True))


# ------------------------------------------------------------------------------------------------ shapes around both tile edges
@functools.lru_cache(maxsize=None)
def _edge_case():
    rng = np.random.default_rng(4100)
    a, b = _dists(rng, T + 1, 5), _dists(rng, T + 1, 5)
    return a, b, ref.scores(a, b)


@pytest.mark.parametrize("Q,D", [(1, 1), (2, 2), (1, T + 1), (T + 1, 1), (T - 1, T + 1), (T, T), (T + 1, T - 1), (2, T), (T, 2),
                                 (T + 1, T + 1)])
def test_shapes_around_the_tile_edges(Q, D):
    a, b, sc = _edge_case()
    for n, layout in ((1, "odd"), (5, "vec"), (16, "odd")):
        check(device_run(a[:Q], b[:D], n, layout=layout), ref.select(sc[:Q, :D], n), "Q=%d D=%d n=%d" % (Q, D, n))


# ------------------------------------------------------------------------------------------------ inner lengths around the k-step
@functools.lru_cache(maxsize=None)
def _length_case(L):
    rng = np.random.default_rng(4200 + L)
    a, b = _dists(rng, 3, L), _dists(rng, 7, L)
    b[5] = b[1]                                                         # equal scores: the order is by id
    return a, b, ref.scores(a, b)


@pytest.mark.parametrize("L", [1, 2, 3, S - 1, S, S + 1, 511, 512, 513, 1031])
def test_inner_lengths(L):
    a, b, sc = _length_case(L)
    for layout in ("odd", "vec"):
        check(device_run(a, b, 5, layout=layout), ref.select(sc, 5), "L=%d %s" % (L, layout))


# ------------------------------------------------------------------------------------------------ planted rows
ROW_BASE = 2 ** 40 - 70                                                 # the ids cross 2^40
PL_D, PL_L = 140, 6


@functools.lru_cache(maxsize=None)
def _planted():
    rng = np.random.default_rng(4300)
    a, b = _dists(rng, 7, PL_L), _dists(rng, PL_D, PL_L)
    b[126:131] = b[3]                                                   # a tie group across the tile edge at 128 ...
    b[68:72] = b[5]                                                     # ... and one across the seam of chunks = 2 (row 70)
    b[10] = 0.0                                                         # all-zero rows, +0.0 and -0.0
    b[11] = -0.0
    b[12, 0] = np.inf                                                   # inf * 0 = NaN for the query with a zero there, +inf for the others
    a[:, 0] = np.maximum(a[:, 0], 0.01)
    a[2, 0] = 0.0
    a[3, :] = np.nan                                                    # a whole NaN query
    a[4] = a[4] * 2.0 ** -1040                                          # denormal products
    a[5] = b[3]                                                         # its six best are one tie group: a tie at the n-th place for n = 5
    b[21] = b[20]
    b[21, 2] = np.nextafter(b[20, 2], 2.0)                              # scores equal up to the last bit
    b[22] = b[20]
    b[22, 2] = np.nextafter(b[20, 2], 0.0)
    a[6] = -a[0]                                                        # negative scores: the zero rows come first, -inf last
    exclude = np.array([ROW_BASE + 3, ROW_BASE - 5, ROW_BASE + PL_D + 7, -1, -1, ROW_BASE + 126, ROW_BASE + 10], dtype=np.int64)
    return a, b, exclude, ref.scores(a, b)


@pytest.mark.parametrize("n", [1, 5, 16])
def test_planted_rows_at_every_chunking(n):
    a, b, exclude, sc = _planted()
    want = ref.select(sc, n, ROW_BASE, exclude)
    assert want[2][3] == PL_D and np.all(want[0][3] == -1) and want[2][2] == 1          # the NaN query; inf * 0 counted
    assert np.isposinf(want[1][0, 0]) and want[0][0, 0] == ROW_BASE + 12
    first = None
    for chunks in (0, 1, 2, 3, PL_D, PL_D + 9):
        got = device_run(a, b, n, ROW_BASE, exclude, chunks, layout="odd" if chunks % 2 else "vec")
        check(got, want, "n=%d chunks=%d" % (n, chunks))
        first = got if first is None else first
        assert all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(got[:2], first[:2]))
    if n == 5:                                                          # query 5: the inf row, then the tie group by id, 126 excluded
        full = ref.select(sc, 6, ROW_BASE, exclude)
        assert list(full[0][5] - ROW_BASE) == [12, 3, 127, 128, 129, 130] and full[1][5, 4] == full[1][5, 5]


def test_fewer_candidates_than_n_and_null_outputs():
    a, b, exclude, sc = _planted()
    for D, n, ex in ((3, 16, None), (5, 5, np.full(7, 2, dtype=np.int64)), (1, 1, np.zeros(7, dtype=np.int64)), (0, 4, None)):
        want = ref.select(sc[:, :D], n, 0, ex)
        check(device_run(a, b[:D], n, 0, ex, layout="odd"), want, "D=%d n=%d" % (D, n))
        if D and ex is not None:
            assert np.all(want[0][:, -1] == -1) and np.all(want[1][:, -1] == 0.0)       # D - 1 < n: padded
    want = ref.select(sc, 4, 0, None)
    for only in ("idx", "val", "nan"):
        got = device_run(a, b, 4, want=(only,))
        k = ("idx", "val", "nan").index(only)
        assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64))
    idx, val, nan = device_run(a[:0], b, 4)                             # Q == 0: a no-op
    assert idx.shape == (0, 4) and nan.shape == (0,)


def test_device_sqrt_is_numpy_sqrt():
    """the rows of the Hellinger affinity are torch.sqrt on the device: correctly rounded, as np.sqrt, on values where a sloppy root
    shows -- exact squares and their neighbours, denormals, zero, the largest doubles"""
    import torch
    rng = np.random.default_rng(4400)
    roots = np.concatenate([rng.integers(1, 2 ** 26, size=200).astype(np.float64), rng.random(200) + 0.5])
    squares = roots * roots
    x = np.concatenate([squares, np.nextafter(squares, np.inf), np.nextafter(squares, 0.0), [0.0, 5e-324, 1e-310, 2.0 ** -1022],
                        [np.finfo(np.float64).max, 2.0 ** 1023, 1.0, 2.0, 0.5], rng.random(500) * 10.0 ** rng.uniform(-300, 300, size=500)])
    got = torch.sqrt(torch.from_numpy(x).to("cuda")).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), np.sqrt(x).view(np.uint64))


def test_wrapper_matches_the_c_call():
    """similar.nearest_rows (validation, scratch, strides from the tensors) returns what the C call returns"""
    import torch
    from lda_thesis_amd import similar
    a, b, exclude, sc = _planted()
    want = ref.select(sc, 5, ROW_BASE, exclude)
    ta, tb = torch.from_numpy(a).to("cuda"), torch.from_numpy(np.hstack([b, b])).to("cuda")[:, :PL_L]      # a strided b
    got = similar.nearest_rows(ta, tb, 5, exclude=exclude, row_base=ROW_BASE, chunks=3)
    check(tuple(x.cpu().numpy() for x in got), want, "wrapper")
    with pytest.raises(ValueError):
        similar.nearest_rows(ta, tb, 17)
    with pytest.raises(ValueError):
        similar.nearest_rows(ta, tb[:, :3], 5)
    with pytest.raises(ValueError):
        similar.nearest_rows(ta.cpu(), tb, 5)
