"""CPU restatement of llda_nearest_rows (include/llda_gibbs.h), exact.

Score of a pair: s = +0.0, then s = fma(a[k], b[k], s) for k ascending.  Python 3.10 has no ``math.fma`` and numpy has none; for finite
operands ``float(Fraction(x) * Fraction(y) + Fraction(s))`` is one: the sum is exact and the conversion rounds once, to nearest even.
Zeros, infinities and NaNs go by IEEE 754's rules for fusedMultiplyAdd, written out below.

Order per query: ``np.lexsort`` on (row id, -score) after NaN scores and the ``exclude`` row are removed -- score descending as IEEE
values (-0.0 == +0.0), then global row id ascending.
"""
import math
from fractions import Fraction

import numpy as np


def fma(x, y, s):
    """one correctly rounded x * y + s"""
    x, y, s = float(x), float(y), float(s)
    if math.isnan(x) or math.isnan(y) or math.isnan(s):
        return math.nan
    if math.isinf(x) or math.isinf(y):
        if x == 0.0 or y == 0.0:
            return math.nan                                  # inf * 0
        p = math.copysign(math.inf, math.copysign(1.0, x) * math.copysign(1.0, y))
        return math.nan if math.isinf(s) and s != p else p   # inf - inf
    if math.isinf(s):
        return s
    if x == 0.0 or y == 0.0:
        p = math.copysign(0.0, math.copysign(1.0, x) * math.copysign(1.0, y))
        return p + s                                         # (+-0) + s is exact; -0 + -0 = -0, -0 + +0 = +0
    exact = Fraction(x) * Fraction(y) + Fraction(s)
    if exact == 0:
        return 0.0                                           # exact cancellation of non-zero terms: +0 under round-to-nearest
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def score(arow, brow):
    s = 0.0
    for x, y in zip(arow, brow):
        s = fma(x, y, s)
    return s


def scores(a, b):
    """(Q, D) float64: the chain of every pair (columns of a and b beyond the shorter are the caller's to cut off)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    al, bl = a.tolist(), b.tolist()
    for q, arow in enumerate(al):
        for j, brow in enumerate(bl):
            out[q, j] = score(arow, brow)
    return out


def select(sc, n, row_base=0, exclude=None):
    """from a (Q, D) score matrix: (top_idx (Q, n) int64, top_val (Q, n) float64, n_nan (Q,) int64), padded with -1 / 0.0"""
    sc = np.asarray(sc, dtype=np.float64)
    Q, D = sc.shape
    ids = np.arange(D, dtype=np.int64) + np.int64(row_base)
    top_idx = np.full((Q, n), -1, dtype=np.int64)
    top_val = np.zeros((Q, n), dtype=np.float64)
    n_nan = np.zeros((Q,), dtype=np.int64)
    for q in range(Q):
        nan = np.isnan(sc[q])
        n_nan[q] = int(nan.sum())
        keep = ~nan
        if exclude is not None:
            keep &= ids != np.int64(exclude[q])
        s, i = sc[q][keep], ids[keep]
        order = np.lexsort((i, -(s + 0.0)))[:n]              # (s + 0.0: -0.0 and +0.0 are one key; lexsort compares values anyway)
        top_idx[q, :order.shape[0]] = i[order]
        top_val[q, :order.shape[0]] = s[order]
    return top_idx, top_val, n_nan


def nearest_rows_ref(a, b, n, row_base=0, exclude=None):
    return select(scores(a, b), n, row_base, exclude)
