"""CPU restatement of llda_label_metrics and llda_label_sets (include/llda_gibbs.h): one stable argsort per column, cumulative sums,
the header's rules.  The yardstick of tests/test_gpu_label_metrics.py, test_gpu_label_sets.py and test_gpu_label_dropin.py (bit for
bit) and itself checked against definitions that share no code with it in tests/test_label_host.py.  Also holds the column generators
the test files share; the score kinds of tests/rankref.py are reused by import."""
import numpy as np

import rankref
from rankref import ALL_ZERO, HAS_NAN, NO_NEGATIVE, NO_POSITIVE, ONE_THRESHOLD  # noqa: F401

NAN = float("nan")
OUTPUTS = ("n_pos", "n_thr", "auc_num", "auc", "thr_tp", "thr_fp", "f1", "thr", "flags", "order")


def label_column(col, y):
    """the ten outputs of one ranked label: col (D,) float64, y (D,) truth"""
    col = np.asarray(col, dtype=np.float64)
    y = np.asarray(y) != 0
    D = col.shape[0]
    if np.isnan(col).any():
        return dict(n_pos=0, n_thr=0, auc_num=0, auc=NAN, thr_tp=0, thr_fp=0, f1=NAN, thr=NAN, flags=HAS_NAN,
                    order=np.full((D,), -1, dtype=np.int32))
    order = np.argsort(-col, kind="stable")                       # score descending, then document id ascending (-0.0 == 0.0)
    ss, t = col[order], y[order]
    end = np.ones((D,), dtype=bool)                               # position ends a tie group = a threshold
    end[:-1] = ss[:-1] != ss[1:]
    tp_all = np.cumsum(t, dtype=np.int64)
    at = np.flatnonzero(end)
    tp = tp_all[at]
    fp = at + 1 - tp
    start = np.concatenate([[0], at[:-1] + 1])                    # first position of every group
    P, T = int(tp_all[-1]), int(at.shape[0])
    N = D - P
    tp0, fp0 = np.concatenate([[0], tp[:-1]]), np.concatenate([[0], fp[:-1]])
    A = int(((fp - fp0) * (tp + tp0)).sum())                      # < 2^61: exact in int64
    flags = (NO_POSITIVE if P == 0 else 0) | (NO_NEGATIVE if N == 0 else 0) | (ONE_THRESHOLD if T < 2 else 0) | (ALL_ZERO if (col == 0).all() else 0)
    out = dict(n_pos=P, n_thr=T, auc_num=A, auc=np.float64(A) / np.float64(2 * P * N) if P and N else NAN, flags=flags,
               order=order.astype(np.int32), thr_tp=0, thr_fp=0, f1=NAN, thr=NAN)
    best = None
    for g in range(T):                                            # highest threshold first: a later equal rational does not replace
        if tp[g] > 0:
            num, den = 2 * int(tp[g]), int(tp[g]) + int(fp[g]) + P
            if best is None or num * best[1] > best[0] * den:     # python integers: exact
                best = (num, den, g)
    if best is not None:
        g = best[2]
        out.update(thr_tp=int(tp[g]), thr_fp=int(fp[g]), f1=np.float64(best[0]) / np.float64(best[1]), thr=col[order[start[g]]])
    return out


def label_metrics(score, truth, first=1, n_labels=None, K=None):
    """score (D, ld), truth (D, K) -> dict of arrays over the ranked columns first .. first + n_labels - 1 (order: (n_labels, D))"""
    score = np.asarray(score, dtype=np.float64)
    K = score.shape[1] if K is None else K
    n_labels = K - first if n_labels is None else n_labels
    cols = [label_column(score[:, first + l], truth[:, first + l]) for l in range(n_labels)]
    out = {}
    for name in OUTPUTS:
        dt = {"auc": np.float64, "f1": np.float64, "thr": np.float64, "flags": np.int32, "order": np.int32}.get(name, np.int64)
        out[name] = np.array([c[name] for c in cols], dtype=dt).reshape((n_labels,) + ((score.shape[0],) if name == "order" else ()))
    return out


def rank_key(x):
    """the sort key of llda_rank_labels as a python integer: ascends as the score descends, -0.0 folded onto +0.0"""
    bits = int(np.float64(x).view(np.uint64))
    if bits == 1 << 63:
        bits = 0
    return bits if bits >> 63 else (~bits & 0x7FFFFFFFFFFFFFFF)


def label_sets(score, thr, truth=None, first=1, at_least_one=True, K=None):
    """dict(mask (D, K) bool, n_pred, and with truth n_hit, n_true, tp, fp, fn) by the rules of llda_label_sets"""
    score = np.asarray(score, dtype=np.float64)
    K = score.shape[1] if K is None else K
    D = score.shape[0]
    thr = np.asarray(thr, dtype=np.float64)
    elig = ~np.isnan(thr[:K])
    elig[:first] = False
    s = score[:, :K]
    with np.errstate(invalid="ignore"):
        mask = (s >= thr[None, :K]) & elig[None, :]
    n_pred = mask.sum(axis=1).astype(np.int32)
    cols = np.flatnonzero(elig)
    for d in range(D):
        if np.isnan(s[d, cols]).any():
            mask[d] = False
            n_pred[d] = -1
        elif n_pred[d] == 0 and at_least_one and cols.size:
            k = cols[np.argsort(-s[d, cols], kind="stable")[0]]
            mask[d, k] = True
            n_pred[d] = 1
    out = dict(mask=mask, n_pred=n_pred)
    if truth is not None:
        t = np.asarray(truth)[:, :K] != 0
        t[:, :first] = False
        out.update(n_hit=(mask & t).sum(axis=1).astype(np.int32), n_true=t.sum(axis=1).astype(np.int32),
                   tp=(mask & t).sum(axis=0).astype(np.int64), fp=(mask & ~t).sum(axis=0).astype(np.int64),
                   fn=(~mask & t).sum(axis=0).astype(np.int64))
    return out


def pack_mask(mask):
    """(D, K) bool -> (D, (K + 31) // 32) uint32 bit words"""
    D, K = mask.shape
    W = (K + 31) // 32
    m = np.zeros((D, W * 32), dtype=np.uint64)
    m[:, :K] = mask
    return (m.reshape(D, W, 32) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2).astype(np.uint32)


# ---- generators ----
KINDS = rankref.KINDS + ("equal", "zeros", "signed_zero", "extreme")


def gen_column_scores(rng, kind, D, L):
    """(D, L) scores whose COLUMNS are of one kind: rankref's four kinds (generated label-major, so that a column has the kind's
    structure), all-equal, all-zero, a mix of +-0.0, and +-inf / denormals / negative scores"""
    if kind in rankref.KINDS:
        if kind == "foldin":                                      # mostly exact zeros down a column
            s = np.zeros((L, D))
            for l in range(L):
                nnz = max(1, D // 16)
                rows = rng.choice(D, size=min(D, nnz), replace=False)
                s[l, rows] = rng.integers(1, 30, size=rows.shape[0]) / rng.integers(30, 60, size=rows.shape[0])
            return np.ascontiguousarray(s.T)
        return np.ascontiguousarray(rankref.gen_scores(rng, kind, L, D).T)
    if kind == "equal":
        return np.full((D, L), 0.375)
    if kind == "zeros":
        return np.zeros((D, L))
    if kind == "signed_zero":
        return np.where(rng.random((D, L)) < 0.5, -0.0, 0.0)
    if kind == "extreme":
        pool = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, 2.5e-310, -1.5, -0.25, 0.0, -0.0, 1.0, 1e308, -1e308])
        return pool[rng.integers(0, pool.shape[0], size=(D, L))]
    raise ValueError(kind)


def gen_label_truth(rng, D, L):
    """(D, L) uint8 with about one document in five positive"""
    return (rng.random((D, L)) < 0.2).astype(np.uint8)


def plant_columns(rng, score, truth, first):
    """overwrite the first ranked columns (as many as there are) with the cases a walk gets wrong first; returns the column of the NaN
    (or None): no positive, no negative, the only positive ranked first, the only positive ranked last, a NaN"""
    D, K = truth.shape
    nan_col = None
    for i, c in enumerate(range(first, min(K, first + 5))):
        if i == 0:
            truth[:, c] = 0
        elif i == 1:
            truth[:, c] = 1
        elif i in (2, 3):
            col = rng.permutation(D).astype(np.float64) / 8
            truth[:, c] = 0
            truth[np.argmax(col) if i == 2 else np.argmin(col), c] = 1
            score[:, c] = col
        else:
            score[int(rng.integers(0, D)), c] = np.nan
            nan_col = c
    return nan_col
