"""Host side of the estimate of alpha and beta (lda_thesis_amd/priors.py) and the argument checks of llda_count_hist: no GPU.

The estimator sees the counts only through their histogram (plus the list of values beyond it); the tests build both from small
explicit arrays and compare with the per-entry formulas evaluated directly on the same arrays."""
import ctypes
import math

import numpy as np
import pytest

from lda_thesis_amd import priors

_HARM = {}


BIG = 20_000_000


def harm(a, n):
    """psi(n + a) - psi(a) = sum_{i<n} 1/(a + i) with math.fsum (the first BIG terms of a long sum are summed once per a)"""
    a, n = float(a), int(n)
    if n < BIG:
        return math.fsum((1.0 / (a + np.arange(n, dtype=np.float64))).tolist())
    if a not in _HARM:
        _HARM[a] = math.fsum((1.0 / (a + np.arange(BIG, dtype=np.float64))).tolist())
    return math.fsum([_HARM[a]] + list(1.0 / (a + np.arange(BIG, n, dtype=np.float64))))


def split(values, n_bins):
    values = np.asarray(values, dtype=np.int64).ravel()
    return np.bincount(values[values < n_bins], minlength=n_bins).astype(np.int64), np.sort(values[values >= n_bins])


def alpha_case(n_bins):
    """six documents, K = 5; None = topic not allowed"""
    big = BIG
    rows = [[n_bins - 1, n_bins, 0, 3, None], [n_bins + 1, None, 2, None, None], [big, 1, 0, None, None],
            [4, 4, 1, 0, 7], [2, None, None, None, 0], [9, None, None, None, None]]
    entries = [v for r in rows for v in r if v is not None]
    A = [sum(v is not None for v in r) for r in rows]
    N = [sum(v for v in r if v is not None) for r in rows]
    return entries, A, N


def beta_case(n_bins):
    """K = 3, V = 7"""
    return np.array([[n_bins - 1, n_bins, 0, 3, 0, 1, 2], [n_bins + 1, 0, 0, BIG, 5, 0, 1], [0, 0, 1, 1, 2, 14, 0]], dtype=np.int64)


@pytest.mark.parametrize("n_bins", [16, 65536])
def test_one_update_equals_the_per_entry_formula(n_bins):
    alpha, beta = 0.37, 0.021
    entries, A, N = alpha_case(n_bins)
    hist, over = split(entries, n_bins)
    assert over.size == 3
    got = priors.update_alpha(alpha, hist, over, priors.doc_classes(A, N))
    want = alpha * math.fsum(harm(alpha, n) for n in entries) / math.fsum(a * harm(a * alpha, n) for a, n in zip(A, N))
    assert abs(got / want - 1) < 1e-10, (got, want)

    n_kv = beta_case(n_bins)
    K, V = n_kv.shape
    hist, over = split(n_kv, n_bins)
    assert over.size == 3
    got = priors.update_beta(beta, hist, over, n_kv.sum(axis=1), V)
    want = beta * math.fsum(harm(beta, n) for n in n_kv.ravel()) / (V * math.fsum(harm(V * beta, n) for n in n_kv.sum(axis=1)))
    assert abs(got / want - 1) < 1e-10, (got, want)


def test_tail_counts_and_doc_classes():
    np.testing.assert_array_equal(priors.tail_counts([5, 0, 2, 1]), [3, 3, 1, 0])
    cls = priors.doc_classes([2, 3, 2, 2], [10, 10, 10, 7])
    np.testing.assert_array_equal(cls, [[2, 7, 1], [2, 10, 2], [3, 10, 1]])
    assert priors.doc_classes([], []).shape == (0, 3)


def planted_alpha(rng, D=400, K=40, alpha=0.3):
    labs = np.zeros((D, K), dtype=bool)
    labs[:, 0] = True
    n_dk = np.zeros((D, K), dtype=np.int64)
    for d in range(D):
        labs[d, 1 + rng.choice(K - 1, size=int(rng.integers(1, 8)), replace=False)] = True
        idx = np.flatnonzero(labs[d])
        n_dk[d, idx] = rng.multinomial(int(rng.integers(5, 300)), rng.dirichlet(np.full(idx.size, alpha)))
    return labs, n_dk


def planted_beta(rng, K=40, V=500, beta=0.05):
    n_k = rng.integers(200, 20001, size=K)
    return np.stack([rng.multinomial(int(n), rng.dirichlet(np.full(V, beta))) for n in n_k]).astype(np.int64)


def evidence_alpha(alpha, labs, n_dk):
    A, N = labs.sum(axis=1), n_dk.sum(axis=1)
    return (math.fsum(math.lgamma(a * alpha) - math.lgamma(n + a * alpha) for a, n in zip(A, N))
            + math.fsum(math.lgamma(n + alpha) - math.lgamma(alpha) for n in n_dk[labs]))


def evidence_beta(beta, n_kv):
    V = n_kv.shape[1]
    return (math.fsum(math.lgamma(V * beta) - math.lgamma(n + V * beta) for n in n_kv.sum(axis=1))
            + math.fsum(math.lgamma(n + beta) - math.lgamma(beta) for n in n_kv.ravel()))


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(20240917)
    labs, n_dk = planted_alpha(rng)
    n_kv = planted_beta(rng)
    hist_dk, over_dk = split(n_dk[labs], 64)              # (a short histogram: the longest documents' counts go through the list)
    hist_kw, over_kw = split(n_kv, 65536)
    est = priors.estimate(0.001, 0.001, hist_dk=hist_dk, over_dk=over_dk, classes=priors.doc_classes(labs.sum(axis=1), n_dk.sum(axis=1)),
                          hist_kw=hist_kw, over_kw=over_kw, n_k=n_kv.sum(axis=1), V=n_kv.shape[1])
    return labs, n_dk, n_kv, est


def test_planted_priors_are_recovered(planted):
    labs, n_dk, n_kv, est = planted
    print("alpha %.6f (planted 0.3: %+.2f %%), beta %.6f (planted 0.05: %+.2f %%), %d iterations"
          % (est.alpha, 100 * (est.alpha / 0.3 - 1), est.beta, 100 * (est.beta / 0.05 - 1), est.iterations))
    assert est.converged and 0 < est.iterations < 1000
    assert abs(est.alpha / 0.3 - 1) < 0.10
    assert abs(est.beta / 0.05 - 1) < 0.10


def test_the_evidence_never_falls_and_ends_at_a_maximum(planted):
    labs, n_dk, n_kv, est = planted
    e = evidence_alpha(est.alpha, labs, n_dk)
    assert e >= evidence_alpha(0.001, labs, n_dk)
    assert e >= evidence_alpha(0.95 * est.alpha, labs, n_dk) and e >= evidence_alpha(1.05 * est.alpha, labs, n_dk)
    e = evidence_beta(est.beta, n_kv)
    assert e >= evidence_beta(0.001, n_kv)
    assert e >= evidence_beta(0.95 * est.beta, n_kv) and e >= evidence_beta(1.05 * est.beta, n_kv)
    # ... and step by step from the start
    hist, over = split(n_dk[labs], 64)
    cls = priors.doc_classes(labs.sum(axis=1), n_dk.sum(axis=1))
    a, prev = 0.001, evidence_alpha(0.001, labs, n_dk)
    for _ in range(5):
        a = priors.update_alpha(a, hist, over, cls)
        cur = evidence_alpha(a, labs, n_dk)
        assert cur >= prev
        prev = cur


def test_degenerate_inputs_leave_the_prior_alone():
    # every document allows one topic only: the evidence does not depend on alpha
    n = np.array([5, 17, 1, 40])
    hist, over = split(n, 16)
    cls = priors.doc_classes(np.ones(4), n)
    assert priors.update_alpha(0.25, hist, over, cls) == 0.25
    est = priors.estimate(0.25, None, hist_dk=hist, over_dk=over, classes=cls)
    assert est.alpha == 0.25 and est.beta is None and est.converged
    # nothing at all
    empty = np.zeros(16, dtype=np.int64)
    assert priors.update_alpha(0.25, empty, [], priors.doc_classes([], [])) == 0.25
    assert priors.update_beta(0.125, empty, [], np.zeros(3, dtype=np.int64), 7) == 0.125
    assert priors.update_beta(0.125, empty, [], np.zeros(0, dtype=np.int64), 0) == 0.125
    # documents that allow several topics but hold no token
    zeros = np.zeros(16, dtype=np.int64)
    zeros[0] = 6
    assert priors.update_alpha(0.25, zeros, [], priors.doc_classes([3, 3], [0, 0])) == 0.25
    est = priors.estimate(0.25, 0.125, hist_dk=empty, classes=priors.doc_classes([], []), hist_kw=empty, n_k=np.zeros(3), V=7)
    assert (est.alpha, est.beta, est.converged) == (0.25, 0.125, True) and not any(math.isnan(x) for x in est[:2])


def test_an_estimate_below_the_domain_is_clamped():
    # every topic's tokens on one word of many: every step shrinks beta (towards 0, ever more slowly); a step from the edge of the
    # domain would leave it and is clamped
    n_kv = np.zeros((4, 50), dtype=np.int64)
    n_kv[np.arange(4), [3, 9, 20, 41]] = [1000, 500, 2000, 50]
    hist, over = split(n_kv, 65536)
    assert priors.update_beta(0.01, hist, over, n_kv.sum(axis=1), 50) < 0.01
    assert priors.update_beta(2e-6, hist, over, n_kv.sum(axis=1), 50) < 2e-6
    assert priors.update_beta(1e-6, hist, over, n_kv.sum(axis=1), 50) == 1e-6 == priors.PRIOR_MIN
    est = priors.estimate(None, 1e-6, hist_kw=hist, over_kw=over, n_k=n_kv.sum(axis=1), V=50)
    assert est.beta == 1e-6 and est.alpha is None and est.converged
    # every document's tokens on one of its three topics: the same for alpha
    vals = np.array([30, 0, 0] * 20)
    hist, over = split(vals, 65536)
    cls = priors.doc_classes([3] * 20, [30] * 20)
    assert priors.update_alpha(0.5, hist, over, cls) < 0.5 and priors.update_alpha(2e-6, hist, over, cls) < 2e-6
    assert priors.update_alpha(1e-6, hist, over, cls) == 1e-6
    assert priors.in_domain(1e-6, 1e-6, 50) and not priors.in_domain(9e-7, 0.1, 50) and not priors.in_domain(0.1, 2.0 ** 40 / 50, 50)
    assert not priors.in_domain(float("nan"), 0.1, 50)


def test_negative_counts_are_refused():
    with pytest.raises(ValueError):
        priors.update_beta(0.1, np.array([3, 1]), [-5], np.array([4]), 3)
    with pytest.raises(ValueError):
        priors.psi_diff(0.1, [-1])


def test_count_hist_validates_arguments():
    """llda_count_hist returns before anything touches HIP: NULL pointers, n_bins < 1, over_cap < 0 -> LLDA_E_BAD_ARG (-2); K outside
    1 .. LLDA_MAX_K -> LLDA_E_BAD_K (-1); rows = 0 is a no-op."""
    from lda_thesis_amd import _native
    L = _native.lib()
    assert "llda_count_hist" in _native.EXPORTS and _native.ABI_VERSION == 22 == L.llda_abi_version()
    buf = (ctypes.c_int64 * 64)()                          # host memory standing in for device pointers: never dereferenced here
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.llda_count_hist(None, 1, 8, None, 1, 16, None, None, 4, None, None) == -2
    for which in range(5):
        args = [p, 1, 8, p, 1, 16, p, p, 4, p, None]
        args[(0, 3, 6, 7, 9)[which]] = None
        assert L.llda_count_hist(*args) == -2
    assert L.llda_count_hist(p, 1, 8, p, 1, 0, p, p, 4, p, None) == -2          # n_bins = 0
    assert L.llda_count_hist(p, 1, 8, p, 1, 16, p, p, -1, p, None) == -2        # over_cap < 0
    assert L.llda_count_hist(p, -1, 8, p, 1, 16, p, p, 4, p, None) == -2        # rows < 0
    assert L.llda_count_hist(p, 1, 8, p, 2, 16, p, p, 4, p, None) == -2         # mask_per_row is 0 or 1
    assert L.llda_count_hist(p, 1, 0, p, 1, 16, p, p, 4, p, None) == -1         # K = 0
    assert L.llda_count_hist(p, 1, 7689, p, 1, 16, p, p, 4, p, None) == -1
    assert L.llda_count_hist(p, 0, 8, p, 1, 16, p, p, 4, p, None) == 0          # rows = 0
    assert L.llda_count_hist(None, 0, 1031, None, 0, 16, None, None, 0, None, None) == 0
