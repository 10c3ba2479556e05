"""numpy restatement of ``llda_scored_words`` (include/llda_gibbs.h) and the inputs its tests share (tests/test_scored_words_host.py,
tests/test_gpu_scored_words.py, tests/test_gpu_label_words_dropin.py).

Pure numpy: nothing here needs a GPU.  Every score is a - 1 IEEE multiplications and one IEEE division of ONE element, which numpy's
element-wise ``*`` and ``/`` perform exactly as stated, so the restatement is compared bit for bit.
"""
from fractions import Fraction

import numpy as np

import topicref

QNAN = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]


def power(x, a):
    """P_a(x): a - 1 multiplications, left to right, each rounded"""
    p = x
    for _ in range(int(a) - 1):
        p = p * x
    return p


def x_of_counts(n_k_v, beta, den=None, n_k=None):
    """(V, K) float64, x[w][k] = ((double)n_k_v[k][w] + beta) / den[k]; den = None: (double)n_k[k] + V*beta with n_k = None: the row
    sums (llda_readout_phi)"""
    n_k_v = np.asarray(n_k_v).astype(np.int64)
    V = n_k_v.shape[1]
    with np.errstate(all="ignore"):
        if den is None:
            n_k = n_k_v.sum(axis=1) if n_k is None else np.asarray(n_k)
            den = n_k.astype(np.float64) + float(V) * float(beta)
        return ((n_k_v.astype(np.float64) + float(beta)) / np.asarray(den, dtype=np.float64)[:, np.newaxis]).T.copy()


def scores_of(x, a=1, wdiv=None):
    """(V, K) float64: P_a(x) / wdiv[w], nothing divided without wdiv"""
    with np.errstate(all="ignore"):
        s = power(np.asarray(x, dtype=np.float64), a)
        return s if wdiv is None else s / np.asarray(wdiv, dtype=np.float64)[:, np.newaxis]


def scored_words_ref(x, n, a=1, wdiv=None):
    """-> (top_idx (K, n) int32, top_score (K, n) float64, n_nan (K,) int32) of the (V, K) matrix x: per topic the candidates are the
    words with wdiv != 0 in id order, NaN scores are dropped and counted, and the list is ``np.argsort(-score, kind="stable")[:n]``
    of the rest; missing entries are -1 / the quiet NaN."""
    x = np.asarray(x, dtype=np.float64)
    V, K = x.shape
    cand = np.arange(V) if wdiv is None else np.flatnonzero(np.asarray(wdiv) != 0)
    s = np.ascontiguousarray(scores_of(x, a, wdiv)[cand].T)          # (K, candidates): a topic's scores side by side
    idx = np.full((K, n), -1, dtype=np.int32)
    sc = np.full((K, n), QNAN, dtype=np.float64)
    nn = np.zeros((K,), dtype=np.int32)
    for k in range(K):
        sk = s[k]
        bad = np.isnan(sk)
        nn[k] = int(bad.sum())
        words, sk = cand[~bad], sk[~bad]
        order = np.argsort(-sk, kind="stable")[:n]
        idx[k, :order.shape[0]] = words[order]
        sc[k, :order.shape[0]] = sk[order]
    return idx, sc, nn


def relevance_powers_ref(lam):
    f = Fraction(lam).limit_denominator(8)
    return f.denominator, f.denominator - f.numerator


def word_divisor_ref(n_w, b, min_count=1):
    """a per-element Python loop of multiplications"""
    n_w = np.asarray(n_w)
    total = float(n_w.sum())
    out = np.zeros(n_w.shape[0], dtype=np.float64)
    for w in range(n_w.shape[0]):
        if n_w[w] < max(min_count, 1):
            continue
        p = float(n_w[w]) / total
        v = 1.0 if b == 0 else p
        for _ in range(b - 1):
            v = v * p
        out[w] = v
    return out


def label_words_ref(n_k_v, beta, n, lam, min_count=1):
    """what LabeledLDA.label_words(n, lam, min_count, source="counts") returns, from the (K, V) counts"""
    n_k_v = np.asarray(n_k_v).astype(np.int64)
    a, b = relevance_powers_ref(lam)
    wdiv = None if (b == 0 and min_count < 1) else word_divisor_ref(n_k_v.sum(axis=0), b, min_count)
    idx, sc, _ = scored_words_ref(x_of_counts(n_k_v, beta), n, a, wdiv)
    return idx, sc


def skewed(rng, K, V):
    """counts as a trained n_k_v has them: mostly 0, a few large, many ties (the generator of tests/test_gpu_top_words.py)"""
    m = rng.integers(0, 40, size=(K, V))
    m[rng.random((K, V)) < 0.6] = 0
    heavy = rng.random((K, V)) < 0.02
    m[heavy] = rng.integers(40, 100000, size=int(heavy.sum()))
    return m


def matrix_rows(x, ld, fill=np.nan):
    """the (V, ld) float64 image of a (V, K) matrix, the columns K .. ld-1 holding ``fill``"""
    x = np.asarray(x, dtype=np.float64)
    out = np.full((x.shape[0], ld), fill, dtype=np.float64)
    out[:, :x.shape[1]] = x
    return out


def device_vector(vec, K, pad):
    """a [K] vector in device order ([KP]), the padding ``pad`` (as topicref.device_rows lays out a matrix)"""
    from lda_thesis_amd import _native
    lay = _native.layout_init(K)
    vec = np.asarray(vec)
    out = np.full((lay["KP"],), pad, dtype=vec.dtype)
    out[lay["topic_pos"]] = vec
    return out


device_rows = topicref.device_rows
