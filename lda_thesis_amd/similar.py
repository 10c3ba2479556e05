"""Nearest rows on the device (``llda_nearest_rows``, include/llda_gibbs.h): similar documents, similar labels, kNN prediction.

For every row of a matrix ``a`` the n best rows of a matrix ``b`` under a bilinear score: with rows that hold the square roots of
``theta`` (or ``phi``) the score is the Bhattacharyya coefficient sum_k sqrt(a_k b_k), and the Hellinger distance is sqrt(1 - score).
One tiled fp64 product with the selection in its epilogue: the (Q, D) scores are never written to memory, where
``torch.topk(a @ b.T)`` materialises them and leaves ties and the order of summation to the BLAS.

Score of a pair: s = +0.0, then s = fma(a[k], b[k], s) for k ascending.  Order: score descending (IEEE compares), then global row
id ascending; NaN scores and the query's ``exclude`` row are left out.  Both are independent of the geometry, of ``chunks`` and of the
rank that holds a row, so per-shard lists merged with ``merge_lists`` equal the list of the whole.
"""
import numpy as np

from . import _native

MAX_N = _native.NEAREST_MAX_N
MEASURES = ("hellinger", "cosine", "dot")


def _check_n(n):
    n = int(n)
    if not 1 <= n <= MAX_N:
        raise ValueError("n must be in 1 .. %d" % MAX_N)
    return n


def _rows(x, name):
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 2):
        raise ValueError("%s must be a float64 (rows, L) tensor on the device" % name)
    if x.shape[0] > 0 and x.shape[1] > 0 and (x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
        x = x.contiguous()
    return x


def nearest_rows(a, b, n, exclude=None, row_base=0, chunks=0, stream=None):
    """The n <= 16 best rows of ``b`` (D, L) for every row of ``a`` (Q, L), both float64 on the device (any row stride): device tensors
    (top_idx (Q, n) int64 global row ids = row_base + row, top_val (Q, n) float64, n_nan (Q,) int64 NaN scores left out), padded with
    -1 / 0.0 where a query has fewer than n candidates.  ``exclude``: int64 [Q] (tensor or array), the global row id query q must not
    return (-1 = none) -- the self-match.  ``chunks``: into how many row ranges b is cut (0 = the library chooses); no output depends
    on it.  Enqueues on ``stream`` (default: the current one)."""
    import torch
    _native.lib()
    _native.require_device()
    n = _check_n(n)
    a, b = _rows(a, "a"), _rows(b, "b")
    if a.device != b.device:
        raise ValueError("a and b must live on one device")
    Q, D, L = int(a.shape[0]), int(b.shape[0]), int(a.shape[1])
    if int(b.shape[1]) != L or L < 1:
        raise ValueError("a and b must have the same number of columns, at least one")
    if int(chunks) < 0 or int(row_base) < 0:
        raise ValueError("chunks and row_base must not be negative")
    dev = a.device
    ex = None
    if exclude is not None:
        ex = exclude if isinstance(exclude, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(exclude, dtype=np.int64))
        ex = ex.to(device=dev, dtype=torch.int64).contiguous()
        if tuple(ex.shape) != (Q,):
            raise ValueError("exclude must hold one row id per query")
    nbytes = _native.nearest_scratch_bytes(Q, D, n, chunks)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        top_idx = torch.empty((Q, n), dtype=torch.int64, device=dev)
        top_val = torch.empty((Q, n), dtype=torch.float64, device=dev)
        n_nan = torch.empty((Q,), dtype=torch.int64, device=dev)
        _native.nearest_rows(a, b, Q, D, L, n, scratch, lda=int(a.stride(0)) if Q > 1 else L, ldb=int(b.stride(0)) if D > 1 else L,
                             row_base=row_base, exclude=ex, chunks=chunks, top_idx=top_idx, top_val=top_val, n_nan=n_nan)
        for x in (a, b, ex):
            if x is not None:
                x.record_stream(stream)
    return top_idx, top_val, n_nan


def affinity_rows(x, measure="hellinger"):
    """The rows whose bilinear score is the measure, as a new float64 tensor on the device of ``x`` (rows, L):
    "hellinger": ``torch.sqrt(x)`` -- the score is the Bhattacharyya coefficient of two distributions (1 = equal, 0 = disjoint
    support), Hellinger distance = sqrt(1 - score); "cosine": every row divided by its 2-norm (a zero row becomes NaN and is never
    returned); "dot": the rows as they are.  The square roots are materialised once per matrix: another rows * L * 8 bytes next to
    ``x`` -- 4 GB for a million documents of 512 labels."""
    import torch
    if measure not in MEASURES:
        raise ValueError("measure must be one of %s" % (MEASURES,))
    x = x.to(torch.float64)
    if measure == "hellinger":
        return torch.sqrt(x)
    if measure == "cosine":
        return x / torch.sqrt((x * x).sum(dim=1, keepdim=True))
    return x.clone()


# ---------------------------------------------------------------------------------------------- host side, numpy only
def merge_lists(idx_lists, val_lists, n):
    """Merge per-shard results of ``nearest_rows`` -- sequences of (Q, m) int64 ids and (Q, m) float64 scores, padding = id -1 --
    under the same order: (ids (Q, n) int64, scores (Q, n) float64), padded with -1 / 0.0."""
    n = int(n)
    idx = np.concatenate([np.asarray(x, dtype=np.int64) for x in idx_lists], axis=1)
    val = np.concatenate([np.asarray(x, dtype=np.float64) for x in val_lists], axis=1)
    if idx.shape != val.shape or idx.ndim != 2:
        raise ValueError("the lists must be (Q, m) and pair up")
    Q = idx.shape[0]
    out_i = np.full((Q, n), -1, dtype=np.int64)
    out_v = np.zeros((Q, n), dtype=np.float64)
    for q in range(Q):
        real = idx[q] >= 0
        i, v = idx[q][real], val[q][real]
        order = np.lexsort((i, -v))[:n]
        out_i[q, :order.shape[0]] = i[order]
        out_v[q, :order.shape[0]] = v[order]
    return out_i, out_v


def knn_votes(idx, val, labs, k):
    """votes[q][c] = the sum over the first k neighbours of query q, in list order, of val * labs[idx][c] (float64 (Q, C)); idx holds
    rows of ``labs`` (-1 = padding, skipped).  Added one neighbour after the other from +0.0."""
    idx, val, labs = np.asarray(idx, dtype=np.int64), np.asarray(val, dtype=np.float64), np.asarray(labs, dtype=np.float64)
    k = min(int(k), idx.shape[1])
    votes = np.zeros((idx.shape[0], labs.shape[1]), dtype=np.float64)
    for j in range(k):
        real = idx[:, j] >= 0
        votes[real] = votes[real] + val[real, j][:, None] * labs[idx[real, j]]
    return votes
