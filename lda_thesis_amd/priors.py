"""Estimate of the symmetric Dirichlet priors alpha and beta from count histograms (host side, numpy only).

Minka's fixed point for the precision of a symmetric Dirichlet-multinomial ("Estimating a Dirichlet distribution", 2000, eq. 55),
for Labeled LDA where document d allows the topic set L_d (A_d = |L_d| topics, N_d tokens) and topic k holds n_k tokens over V words:

    alpha <- alpha * [ sum_d sum_{k in L_d} ( psi(n_dk + alpha) - psi(alpha) ) ] / [ sum_d A_d * ( psi(N_d + A_d*alpha) - psi(A_d*alpha) ) ]
    beta  <- beta  * [ sum_k sum_v ( psi(n_kv + beta) - psi(beta) ) ]            / [ V * sum_k ( psi(n_k + V*beta) - psi(V*beta) ) ]

For an integer n,  psi(n + a) - psi(a) = sum_{i<n} 1 / (a + i),  so with H[n] = how many entries hold the value n and
T[i] = #{entries > i} each numerator is  sum_i T[i] / (a + i):  the counts enter only through their histogram, which
``llda_count_hist`` builds on the device (exact, independent of order, summed over ranks as integers) and nothing here ever
reads the count matrices.  Entries at or above the histogram's length arrive as a list (``over``) and take the harmonic sum up
to that length plus the asymptotic series of digamma beyond it; so do the long denominators.

The alpha denominator needs only the static multiset of pairs (A_d, N_d) (``doc_classes``), the beta denominator the K numbers n_k.
Every step maximises a lower bound of the evidence that touches it at the current value, so the evidence never falls.
"""
import collections

import numpy as np

PRIOR_MIN = 1e-6            # the kernels of a constructed sampler were selected for alpha, beta >= 1e-6 ...
VBETA_MAX = 2.0 ** 40       # ... and V*beta < 2^40 (sampler.py, llda_sweep_batch); alpha is held below the same bound
ASYM_MIN = 64               # the asymptotic series of digamma is only used at arguments >= 64 (next term < 1e-23 there)
HARMONIC_CAP = 65536        # longest harmonic sum of a denominator before the series takes over

Estimate = collections.namedtuple("Estimate", "alpha beta iterations converged")


def in_domain(alpha, beta, V):
    """are the priors ones a constructed sampler can go on with?"""
    return bool(np.isfinite(alpha) and np.isfinite(beta) and PRIOR_MIN <= alpha < VBETA_MAX and beta >= PRIOR_MIN
                and V * beta < VBETA_MAX)


def tail_counts(hist):
    """T[i] = number of histogrammed entries with a value above i (same length as hist; the last one is 0), as float64 -- exact
    below 2^53 entries."""
    h = np.asarray(hist).astype(np.int64)
    if h.size and int(h.min()) < 0:
        raise ValueError("a histogram bin is negative")
    return (int(h.sum()) - np.cumsum(h)).astype(np.float64)


def _psi_asym(x):
    """digamma(x) for x >= ASYM_MIN: ln x - 1/2x - sum B_2j / (2j x^2j) through x^-10."""
    y = 1.0 / (x * x)
    return np.log(x) - 0.5 / x - y * (1.0 / 12 - y * (1.0 / 120 - y * (1.0 / 252 - y * (1.0 / 240 - y * (1.0 / 132)))))


def psi_diff(a, n, cap=HARMONIC_CAP):
    """psi(n + a) - psi(a) = sum_{i<n} 1/(a + i) for a > 0 and an array of integers n >= 0: the harmonic sum up to
    max(cap, ASYM_MIN) terms, the asymptotic series of digamma for what lies beyond."""
    n = np.asarray(n, dtype=np.int64)
    if n.size == 0:
        return np.zeros(0)
    if int(n.min()) < 0:
        raise ValueError("a count is negative")
    m = min(int(n.max()), max(int(cap), ASYM_MIN))
    cum = np.zeros(m + 1)
    np.cumsum(1.0 / (a + np.arange(m, dtype=np.float64)), out=cum[1:])
    out = cum[np.minimum(n, m)]
    far = n > m
    if far.any():
        out[far] += _psi_asym(a + n[far].astype(np.float64)) - _psi_asym(a + float(m))
    return out


def _numerator(a, hist, over):
    """sum over the entries of psi(n + a) - psi(a) from their histogram and the list of entries beyond it"""
    filled = np.flatnonzero(np.asarray(hist))
    top = int(filled[-1]) if filled.size else 0                        # the largest value in the histogram: T[i] = 0 from there on
    T = tail_counts(np.asarray(hist)[:top + 1])[:top]
    num = float(np.dot(T, 1.0 / (a + np.arange(top, dtype=np.float64))))
    over = np.asarray(over, dtype=np.int64)
    if over.size:
        if int(over.min()) < len(hist):
            raise ValueError("the overflow list holds a value that belongs to the histogram (or a negative count)")
        num += float(psi_diff(a, over, cap=len(hist)).sum())
    return num


def _clamp(x, hi):
    return float(min(max(x, PRIOR_MIN), hi))


def doc_classes(n_allowed, n_tokens):
    """the unique pairs (A_d, N_d) of the documents with their multiplicities: int64 (C, 3) rows (A, N, documents)."""
    pairs = np.stack([np.asarray(n_allowed, dtype=np.int64).ravel(), np.asarray(n_tokens, dtype=np.int64).ravel()], axis=1)
    if pairs.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.int64)
    uniq, mult = np.unique(pairs, axis=0, return_counts=True)
    return np.concatenate([uniq, mult[:, None].astype(np.int64)], axis=1)


def update_alpha(alpha, hist, over, classes):
    """one step of the fixed point for alpha.  hist / over: histogram and overflow list of the ALLOWED entries of n_dk;
    classes: ``doc_classes``.  A numerator or denominator of 0 (no documents, or every document allows one topic only: the
    evidence does not depend on alpha) leaves alpha as it is."""
    alpha = float(alpha)
    classes = np.asarray(classes, dtype=np.int64).reshape(-1, 3)
    if not (classes[:, 0] > 1).any():
        return alpha                      # (one allowed topic per document: numerator = denominator term by term)
    num = _numerator(alpha, hist, over)
    den = 0.0
    for A in np.unique(classes[:, 0]):
        rows = classes[classes[:, 0] == A]
        den += float(A) * float(np.dot(rows[:, 2].astype(np.float64), psi_diff(float(A) * alpha, rows[:, 1])))
    if not (num > 0.0 and den > 0.0 and np.isfinite(num) and np.isfinite(den)):
        return alpha
    return _clamp(alpha * num / den, np.nextafter(VBETA_MAX, 0.0))


def update_beta(beta, hist, over, n_k, V):
    """one step of the fixed point for beta.  hist / over: histogram and overflow list of the (topic, word) entries of n_kw;
    n_k: tokens of every topic; V: vocabulary size."""
    beta, V = float(beta), int(V)
    num = _numerator(beta, hist, over)
    den = float(V) * float(psi_diff(V * beta, n_k).sum()) if V > 0 else 0.0
    if not (num > 0.0 and den > 0.0 and np.isfinite(num) and np.isfinite(den)):
        return beta
    return _clamp(beta * num / den, np.nextafter(VBETA_MAX / V, 0.0))


def _iterate(x, step, tol, max_iter):
    for it in range(1, max_iter + 1):
        new = step(x)
        done = abs(new - x) <= tol * abs(x)
        x = new
        if done:
            return x, it, True
    return x, max_iter, False


def estimate(alpha=None, beta=None, hist_dk=None, over_dk=(), classes=None, hist_kw=None, over_kw=(), n_k=None, V=None,
             tol=1e-9, max_iter=1000):
    """iterate the fixed points from ``alpha`` / ``beta`` (None = leave that prior alone) until the relative step is at most
    ``tol`` or ``max_iter`` steps were taken.  The two priors do not depend on one another given the counts.  Returns
    Estimate(alpha, beta, iterations, converged): the larger of the two iteration counts, and whether BOTH converged."""
    its, ok = 0, True
    if alpha is not None:
        alpha, n, c = _iterate(float(alpha), lambda a: update_alpha(a, hist_dk, over_dk, classes), tol, max_iter)
        its, ok = max(its, n), ok and c
    if beta is not None:
        beta, n, c = _iterate(float(beta), lambda b: update_beta(b, hist_kw, over_kw, n_k, V), tol, max_iter)
        its, ok = max(its, n), ok and c
    return Estimate(alpha, beta, its, ok)
