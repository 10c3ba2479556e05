"""``llda_ecdf_ranks`` (include/llda_gibbs.h) bit for bit against its numpy restatement (tests/frexref.py): every vocabulary size around
the 64-word tile and the chunk, every K around the 64 lanes of the total, ld > K with NaN in the unused columns, both modes, the
column range in one call and in batches, chunk = 256 (a five-level merge tree at V = 5000) with tie groups across the chunk seams,
an all-equal column, signed zeros, a candidate mask, rows whose total is 0, inf or NaN, no candidate at all, the value output, NULL
outputs, a non-default stream.  The output buffers carry guard words behind them and are pre-filled; the scratch is poisoned."""
import numpy as np
import pytest
import torch

import frexref

pytestmark = pytest.mark.gpu

GUARD = 8
FILL_RANK, FILL_VALUE, FILL_NC = -77, -123.25, -55
DEV = "cuda:0"
VS = (1, 2, 63, 64, 65, 257, 5000)


def up(arr):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def run(mat, K, mode, *, cand=None, first=0, n_labels=None, chunk=0, want=(True, True)):
    """the entry point on the (V, ld) device tensor ``mat`` -> (rank (n_labels, V), Vc, value bits (n_labels, V)) numpy"""
    from lda_thesis_amd import _native
    V, ld = int(mat.shape[0]), int(mat.shape[1])
    nl = K - first if n_labels is None else n_labels
    nbytes = _native.ecdf_scratch_bytes(V, nl, chunk)
    scratch = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    rank = torch.full((nl * V + GUARD,), FILL_RANK, dtype=torch.int32, device=DEV)
    val = torch.full((nl * V + GUARD,), FILL_VALUE, dtype=torch.float64, device=DEV)
    nc = torch.full((1 + GUARD,), FILL_NC, dtype=torch.int64, device=DEV)
    _native.ecdf_ranks(mat, V, K, mode, first, nl, rank, scratch[:nbytes], ld=ld, chunk=chunk, cand=cand, value=val if want[0] else None,
                       n_cand=nc if want[1] else None)
    torch.cuda.current_stream(torch.device(DEV)).synchronize()
    rank_h, val_h, nc_h = rank.cpu().numpy(), val.cpu().numpy(), nc.cpu().numpy()
    assert (scratch[nbytes:] == 0x5A).all()
    assert (rank_h[nl * V:] == FILL_RANK).all() and (val_h[nl * V:] == FILL_VALUE).all() and (nc_h[1:] == FILL_NC).all()
    if not want[0]:
        assert (val_h == FILL_VALUE).all()
    if not want[1]:
        assert (nc_h == FILL_NC).all()
    return (rank_h[:nl * V].reshape(nl, V), int(nc_h[0]) if want[1] else None,
            val_h[:nl * V].reshape(nl, V).view(np.uint64) if want[0] else None)


def same(got, ref, what=""):
    rank, Vc, val = got
    bad = np.flatnonzero((rank != ref[0]).any(axis=1))
    assert bad.size == 0, "%s columns %s: got %s want %s" % (what, bad[:5], rank[bad[0]][:12], ref[0][bad[0]][:12])
    if Vc is not None:
        assert Vc == ref[1], what
    if val is not None:
        assert np.array_equal(val, ref[2].view(np.uint64)), what


def check(x, K, *, ld=None, cand=None, chunks=(0,), batches=(), modes=(0, 1), what=""):
    """x (V, K) against the restatement: the whole range for every chunk, then the batches"""
    mat = up(frexref.matrix_rows(x, K if ld is None else ld))
    cd = up(None if cand is None else np.asarray(cand, dtype=np.uint8))
    for mode in modes:
        ref = frexref.ecdf_ranks_ref(x, K, mode, cand)
        for chunk in chunks:
            same(run(mat, K, mode, cand=cd, chunk=chunk), ref, "%s mode=%d chunk=%d" % (what, mode, chunk))
        for b in batches:
            for lo in range(0, K, b):
                nl = min(b, K - lo)
                part = (ref[0][lo:lo + nl], ref[1], np.ascontiguousarray(ref[2][lo:lo + nl]))
                same(run(mat, K, mode, cand=cd, first=lo, n_labels=nl, chunk=chunks[-1]), part, "%s mode=%d batch=%d at %d" % (what, mode, b, lo))
    return mat


@pytest.mark.parametrize("K", [1, 3, 64, 65, 130])
def test_every_shape_both_modes_batches_and_chunks(K):
    """phi of skewed counts (many ties) over every V; ld = K + 3 with NaN behind the columns; a candidate mask at every second V;
    batches of 1 and 7 at V = 65 and 257; chunk = 256 at V = 5000"""
    rng = np.random.default_rng(K)
    for i, V in enumerate(VS):
        x = frexref.x_of_counts(frexref.skewed(rng, K, V), 0.01)
        cand = (rng.random(V) < 0.8) if i % 2 else None
        check(x, K, ld=K + 3, cand=cand, chunks=(0, 256) if V == 5000 else (0,), batches=(1, 7) if V in (65, 257) else (),
              what="V=%d K=%d" % (V, K))
    check(frexref.x_of_counts(frexref.skewed(rng, K, 300), 0.01), K, chunks=(256,), batches=(7,), what="ld=K chunk=256")


def test_tie_groups_across_the_chunk_seams():
    """the planted matrix of tests/test_frex_host.py: tie groups of equal phi and of equal exclusivity whose members come from several
    256-pair chunks and lie across the seams of the merge tiles and of the walk's tile"""
    x = frexref.straddle_matrix()
    check(x, x.shape[1], chunks=(256, 0), batches=(1,), what="straddle")
    check(x, x.shape[1], ld=x.shape[1] + 1, cand=np.arange(x.shape[0]) % 3 != 0, chunks=(256,), what="straddle cand")


@pytest.mark.parametrize("V", [65, 257, 5000])
def test_special_values(V):
    rng = np.random.default_rng(V)
    K = 3
    x = rng.random((V, K))
    x[:, 1] = 0.25                                   # a column of equal values but for the rows planted below
    x[::5, 0] = 0.0                                  # +0.0 and -0.0 in one tie group
    x[2::10, 0] = -0.0
    x[3, :] = 0.0                                    # total 0
    x[4, :] = [-0.0, -0.0, -0.0]                     # total +0.0 (the sum starts from +0.0)
    x[7, :] = [1.0, -1.0, 0.0]                       # total 0 with entries
    x[8, 2] = np.inf                                 # total inf
    x[9, :] = [np.inf, -np.inf, 1.0]                 # total NaN
    x[10, 0] = np.nan
    x[11, :] = [-1.0, -2.0, 0.5]                     # total < 0
    x[12, :] = [-1.0, 3.0, -0.5]                     # a candidate with negative entries
    x[13, :] = [1e308, 1e308, 0.0]                   # the total overflows
    x[14, :] = [5e-324, 0.0, 0.0]                    # a denormal total: the exclusivity is 1
    x[15, :] = [1e300, -1e300 + 1e284, 1e-300]       # mode 1 divides by a small total
    cand = rng.random(V) < 0.7
    cand[12] = cand[14] = cand[15] = True
    chunks = (0, 256) if V == 5000 else (0,)
    check(x, K, ld=K + 1, chunks=chunks, what="special")
    mat = check(x, K, ld=K + 1, cand=cand, chunks=chunks, batches=(1,), what="special cand")
    for mode in (0, 1):
        ref = frexref.ecdf_ranks_ref(x, K, mode)
        assert ref[1] < V and (ref[0][:, [3, 4, 7, 8, 9, 10, 11, 13]] == 0).all() and (ref[0][:, [12, 14, 15]] > 0).all()
    flat = rng.random((V, K))
    flat[:, 1] = 0.25                                # an all-equal column: one tie group, every word has rank V
    check(flat, K, chunks=chunks, what="flat")
    assert (run(up(flat), K, 0, chunk=chunks[-1])[0][1] == V).all()
    # no candidate at all: by the mask, and by the matrix
    for m, cd in ((mat, up(np.zeros(V, dtype=np.uint8))), (up(np.zeros((V, K))), None)):
        for mode in (0, 1):
            rank, Vc, val = run(m, K, mode, cand=cd)
            assert Vc == 0 and (rank == 0).all() and (val == frexref.QNAN_BITS).all()


def test_null_outputs_strides_and_the_python_surface():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(9)
    V, K = 700, 12
    x = frexref.x_of_counts(frexref.skewed(rng, K, V), 0.01)
    cand = rng.random(V) < 0.9
    mat = up(frexref.matrix_rows(x, K + 2))
    for want in ((False, True), (True, False), (False, False)):
        for mode in (0, 1):
            same(run(mat, K, mode, cand=up(cand.astype(np.uint8)), want=want), frexref.ecdf_ranks_ref(x, K, mode, cand))
    ref = frexref.ecdf_ranks_ref(x, K, 1, cand)
    side = torch.cuda.Stream(torch.device(DEV))
    rank, nc, val = topics.ecdf_ranks(mat, K, 1, cand, value=True, stream=side)           # (V, K + 2) rows: ld > K, no copy
    side.synchronize()
    assert rank.dtype == torch.int32 and nc.dtype == torch.int64 and val.dtype == torch.float64 and tuple(rank.shape) == (K, V)
    same((rank.cpu().numpy(), int(nc.item()), val.cpu().numpy().view(np.uint64)), ref)
    rank, nc = topics.ecdf_ranks(mat[:, :K], K, 1, up(cand))                              # a view with stride K + 2
    same((rank.cpu().numpy(), int(nc.item()), None), ref)
    rank, nc = topics.ecdf_ranks(up(x.T.copy()).t(), K, 0, first=5, n_labels=4)           # a transposed view: copied
    r0 = frexref.ecdf_ranks_ref(x, K, 0, None, 5, 4)
    same((rank.cpu().numpy(), int(nc.item()), None), r0)
    assert tuple(topics.ecdf_ranks(mat, K, 0, n_labels=0)[0].shape) == (0, V)
    for bad in (dict(mode=2), dict(K=K + 3), dict(first=10, n_labels=5), dict(cand=np.ones(V + 1))):
        kw = dict(K=K, mode=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            topics.ecdf_ranks(mat, kw.pop("K"), kw.pop("mode"), **kw)
    with pytest.raises(ValueError):
        topics.ecdf_ranks(mat.to(torch.float32), K, 0)
