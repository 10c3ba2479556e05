"""CPU restatement of llda_rank_labels (include/llda_gibbs.h): one stable sort per row, everything else cumulative sums over the
sorted row.  The yardstick of tests/test_gpu_rank_labels.py (bit for bit) and itself checked against lda_thesis_amd.evaluate in
tests/test_rank_host.py.  Also holds the row generators both test files share."""
import numpy as np

NO_POSITIVE, NO_NEGATIVE, ONE_THRESHOLD, ALL_ZERO, HAS_NAN = 1, 2, 4, 8, 16


def rank_rows(score, truth=None, first=1, top_n=5, K=None):
    """score (D, ld) float64, truth (D, K) or None -> dict of the seven outputs (auc, f1, hit_rank None without truth).  Only the
    columns first .. K-1 are looked at."""
    score = np.asarray(score, dtype=np.float64)
    K = score.shape[1] if K is None else K
    D, L = score.shape[0], K - first
    raw = score[:, first:K]
    nanrow = np.isnan(raw).any(axis=1)
    s = np.where(nanrow[:, None], 0.0, raw)
    order = np.argsort(-s, axis=1, kind="stable")                 # score descending, then column ascending (-0.0 == 0.0)
    ss = np.take_along_axis(s, order, axis=1)
    m = min(top_n, L)
    top_idx = np.full((D, top_n), -1, dtype=np.int32)
    top_val = np.zeros((D, top_n), dtype=np.float64)
    top_idx[:, :m] = order[:, :m] + first
    top_val[:, :m] = np.take_along_axis(raw, order[:, :m], axis=1)   # (the row's own bits: a -0.0 stays one)
    top_idx[nanrow] = -1
    top_val[nanrow] = 0.0
    end = np.ones((D, L), dtype=bool)                             # position ends a group of equal scores = a threshold
    end[:, :-1] = ss[:, :-1] != ss[:, 1:]
    n_thr = end.sum(axis=1).astype(np.int32)
    flags = np.where(n_thr < 2, ONE_THRESHOLD, 0) | np.where((s == 0).all(axis=1), ALL_ZERO, 0)
    out = dict(top_idx=top_idx, top_val=top_val, auc=None, f1=None, hit_rank=None)
    if truth is not None:
        t = np.take_along_axis(np.asarray(truth)[:, first:K] != 0, order, axis=1)
        tp = np.cumsum(t, axis=1, dtype=np.int64)
        fp = np.arange(1, L + 1, dtype=np.int64)[None, :] - tp
        P = tp[:, -1]
        N = L - P
        flags = flags | np.where(P == 0, NO_POSITIVE, 0) | np.where(N == 0, NO_NEGATIVE, 0)
        # the threshold before every position (-1: none)
        last = np.maximum.accumulate(np.where(end, np.arange(L)[None, :], -1), axis=1)
        prev = np.concatenate([np.full((D, 1), -1, dtype=last.dtype), last[:, :-1]], axis=1)
        has = end & (prev >= 0)
        pc = np.maximum(prev, 0)
        term = (fp - np.take_along_axis(fp, pc, axis=1)) * (tp + np.take_along_axis(tp, pc, axis=1))
        A = np.where(has, term, 0).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            auc = A.astype(np.float64) / (2 * P * N).astype(np.float64)
            auc[(P == 0) | (N == 0) | (n_thr < 2)] = np.nan
            # best F1: rationals with numerator and denominator below 2^15 that differ do so by more than 2^-30 relative, so the
            # float comparison picks a largest one; equal rationals give the same quotient
            num, den = 2 * tp, tp + fp + P[:, None]
            ok = end & (tp > 0)
            ratio = np.where(ok, num / den, -1.0)
            best = np.argmax(ratio, axis=1)[:, None]
            f1 = (np.take_along_axis(num, best, axis=1)[:, 0].astype(np.float64) /
                  np.take_along_axis(den, best, axis=1)[:, 0].astype(np.float64))
            f1[~ok.any(axis=1)] = np.nan
        hit = np.where(P > 0, np.argmax(t, axis=1) + 1, 0).astype(np.int32)
        auc[nanrow] = np.nan
        f1[nanrow] = np.nan
        hit[nanrow] = 0
        out.update(auc=auc, f1=f1, hit_rank=hit)
    flags = np.where(nanrow, HAS_NAN, flags).astype(np.int32)
    n_thr[nanrow] = 0
    out.update(n_thr=n_thr, flags=flags)
    return out


KINDS = ("foldin", "grid", "distinct", "ulp")


def gen_scores(rng, kind, D, L):
    """(D, L) rows of one of the four score kinds"""
    if kind == "foldin":                                          # a few ratios of small integers, the rest exact zeros
        s = np.zeros((D, L))
        for d in range(D):
            nnz = min(L, int(rng.integers(1, 9)))
            cols = rng.choice(L, size=nnz, replace=False)
            s[d, cols] = rng.integers(1, 30, size=nnz) / rng.integers(30, 60, size=nnz)
        return s
    if kind == "grid":                                            # heavy ties
        return rng.integers(0, 4, size=(D, L)) / 7
    if kind == "distinct":
        return rng.random((D, L))
    if kind == "ulp":                                             # neighbours a few last bits apart
        return 0.25 + np.stack([rng.permutation(L) for _ in range(D)]) * 2.0 ** -52
    raise ValueError(kind)


def gen_truth(rng, D, L, row0=0):
    """(D, L) uint8, density min(0.5, 4 / L); every 9th row (counted from row0) all false, every 11th all true"""
    y = (rng.random((D, L)) < min(0.5, 4 / L)).astype(np.uint8)
    r = np.arange(row0, row0 + D)
    y[r % 9 == 8] = 0
    y[r % 11 == 10] = 1
    return y
