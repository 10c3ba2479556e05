"""llda_heldout_loglik without a GPU: its CPU restatement (tests/heldoutref.py) against an extended-precision evaluation of the
same quantity, the host side of lda_thesis_amd.heldout and the argument validation of the entry point itself."""
import ctypes
import math

import numpy as np
import pytest

import heldoutref
from lda_thesis_amd import heldout

EPS = 2.0 ** -53
LN2_LD = np.log(np.longdouble(2))


def _model(rng, D, K, V):
    """theta rows and phi_t columns that sum to one, all entries positive and within a few orders of magnitude of one another:
    every product and partial sum is a normal number, so the relative error bounds of float64 hold term by term"""
    theta = rng.gamma(0.5, size=(D, K)) + 1e-3
    theta /= theta.sum(axis=1, keepdims=True)
    phi = rng.gamma(0.3, size=(K, V)) + 1e-4
    phi /= phi.sum(axis=1, keepdims=True)
    return theta, np.ascontiguousarray(phi.T)


def _docs(rng, D, V, n_lo, n_hi, f_hi):
    lens = rng.integers(n_lo, n_hi + 1, size=D)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = np.concatenate([np.sort(rng.choice(V, size=n, replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, f_hi + 1, size=int(lens.sum())).astype(np.int32)
    return doc_off, word, freq


@pytest.mark.parametrize("K", (1, 7, 33, 64, 130, 512, 1031))
def test_restatement_agrees_with_extended_precision(K):
    """per document |ll_d - sum f log p| <= 2^-53 W_d (K + 6), ll_d = log(mant) + expo ln 2 taken in long double from the
    restatement's pair and the sum on the right in long double throughout, W_d the scored tokens: a dot product of K positive
    terms has a relative error of at most (K + 2) 2^-53 (one rounding per product, at most K + 1 additions on the path of any
    term through the partials and the tree), which is its logarithm's absolute error; the pair products -- a site's
    exponentiation, squarings included, and the document's product -- add at most 2 * 2^-53 per token; the last 2 cover
    the long-double evaluation of both sides."""
    rng = np.random.default_rng(1000 + K)
    D, V = 24, 97
    theta, phi_t = _model(rng, D, K, V)
    doc_off, word, freq = _docs(rng, D, V, 0, 40, 9)
    freq[::7] = 1000                                                    # long exponentiation chains
    mant, expo, tok, bad = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq)
    assert not bad.any()
    worst = 0.0
    for d in range(D):
        b, e = doc_off[d], doc_off[d + 1]
        W = int(freq[b:e].sum())
        assert tok[d] == W and 0.5 <= mant[d] < 1.0
        p = (theta[d].astype(np.longdouble)[None, :] * phi_t[word[b:e]].astype(np.longdouble)).sum(axis=1)
        want = (freq[b:e].astype(np.longdouble) * np.log(p)).sum() if e > b else np.longdouble(0)
        got = np.log(np.longdouble(mant[d])) + np.longdouble(int(expo[d])) * LN2_LD
        err = abs(float(got - want))
        if W:
            worst = max(worst, err / (EPS * W * (K + 6)))
        assert err <= EPS * W * (K + 6) + (0 if W else 1e-18), (K, d, err / EPS, W)
    print("K %d: worst error %.4f of the bound" % (K, worst))
    assert np.finfo(np.longdouble).nmant >= 63                         # the yardstick is wider than what it measures


def test_restatement_edge_cases():
    theta = np.array([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0]])
    phi_t = np.array([[0.5, 0.5], [0.0, 0.0], [np.inf, 1.0], [np.nan, 1.0], [1e-320, 0.0], [1.0, 1.0]])
    doc_off = np.array([0, 0, 6, 8])
    word = np.array([0, 1, 2, 3, 5, 7, 4, 5], dtype=np.int32)
    freq = np.array([3, 2, 4, 5, 2, 6, 1, 0], dtype=np.int32)
    mant, expo, tok, bad = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq)
    assert (mant[0], expo[0], tok[0], bad[0]) == (0.5, 1, 0, 0)                       # no site: 1.0
    # document 1: 0.5^3 * 1^2 scored; the zero row, inf, NaN and the word outside the vocabulary go to bad
    assert (mant[1], expo[1], tok[1], bad[1]) == (0.5, -2, 5, 2 + 4 + 5 + 6)
    # document 2: a denormal p, then f = 0
    m, e = math.frexp(1e-320)
    assert (mant[2], expo[2], tok[2], bad[2]) == (m, e, 1, 0)
    # freq = None: every site once
    mant, expo, tok, bad = heldoutref.loglik_ref(theta, phi_t, doc_off, word, None)
    assert (mant[1], expo[1], tok[1], bad[1]) == (0.5, 0, 2, 4) and tok[2] == 2
    # the partials: K = 65 puts topic 64 behind topic 0 in partial 0, ahead of topic 1 -- in topic order the sum would be
    # (1 + 2^-53 -> 1) + 2^-52 = 1 + 2^-52; here (1 + 2^-52) + 2^-53 is a tie that goes to the even neighbour
    t = np.zeros((1, 65))
    t[0, 0], t[0, 1], t[0, 64] = 1.0, 2.0 ** -53, 2.0 ** -52
    assert heldoutref.dot64(t[0], np.ones((1, 65)), 65)[0] == 1.0 + 2.0 ** -51


def test_completion_split():
    obs, sco = heldout.completion_split([[(3, 1)], [], [(1, 2), (4, 1), (7, 3), (9, 1)], [(0, 1), (2, 5), (5, 1)]])
    assert obs == [[(3, 1)], [], [(1, 2), (7, 3)], [(0, 1), (5, 1)]]
    assert sco == [[], [], [(4, 1), (9, 1)], [(2, 5)]]
    assert heldout.completion_split([]) == ([], [])
    assert heldout.observed_tokens(obs).tolist() == [1.0, 0.0, 5.0, 2.0]


def test_smooth_theta_rounds_every_operation():
    th = np.array([[0.1, 0.9, 0.0], [1 / 3, 1 / 3, 1 / 3]])
    w = np.array([7.0, 12.0])
    got = heldout.smooth_theta(th, w, 0.1)
    for d in range(2):
        for k in range(3):
            assert got[d, k] == (w[d] * th[d, k] + 0.1) / (w[d] + 3 * 0.1)


def test_perplexity_from():
    mant, expo = np.array([0.5, 0.75, 0.5]), np.array([1, -10, -3], dtype=np.int64)
    tok, bad = np.array([0, 4, 2], dtype=np.int64), np.zeros(3, dtype=np.int64)
    r = heldout.perplexity_from(mant, expo, tok, bad)
    ll = [math.log(0.5) + 1 * math.log(2.0), float(np.log(0.75)) + -10.0 * math.log(2.0), float(np.log(0.5)) + -3.0 * math.log(2.0)]
    assert r["loglik"] == (0.0 + ll[0]) + ll[1] + ll[2] and r["tokens"] == 6 and r["bad"] == 0
    assert r["perplexity"] == float(np.exp(-r["loglik"] / 6))
    bad[1] = 3
    r = heldout.perplexity_from(mant, expo, tok, bad)
    assert r["perplexity"] == float("inf") and r["bad"] == 3 and r["tokens"] == 6
    r = heldout.perplexity_from(mant[:1], expo[:1], tok[:1], bad[:1])
    assert math.isnan(r["perplexity"]) and r["tokens"] == 0 and r["loglik"] == 0.0
    assert math.isnan(heldout.perplexity_from(mant[:0], expo[:0], tok[:0], bad[:0])["perplexity"])


def test_heldout_loglik_validates_arguments():
    """the symbol is declared, exported and bound; K = 0 and K = 7 689, NULL required pointers, ld < K, V < 1, a negative D and
    misaligned pointers are refused before anything touches HIP; D = 0 is a no-op; the ABI number has not moved"""
    from lda_thesis_amd import _native
    from test_abi import declared_symbols
    L = _native.lib()
    assert L.llda_abi_version() == 22
    assert "llda_heldout_loglik" in _native.EXPORTS and "llda_heldout_loglik" in declared_symbols()
    assert L.llda_struct_size(5) == ctypes.sizeof(_native.LldaHeldoutArgs)
    assert _native.HELDOUT_MAX_FREQ == 2 ** 23 - 1

    def call(**kw):
        a = _native.LldaHeldoutArgs()
        a.doc_off, a.word, a.freq, a.theta, a.phi_t = 4096, 8192, 12288, 16384, 20480      # (fake pointers: never dereferenced on the host)
        a.D, a.V, a.ld_theta, a.ld_phi, a.K = 2, 10, 8, 8, 8
        a.mant, a.expo, a.tok, a.bad = 24576, 28672, 32768, 36864
        for k, v in kw.items():
            setattr(a, k, v)
        return L.llda_heldout_loglik(ctypes.byref(a), None)

    assert L.llda_heldout_loglik(None, None) == -2
    assert call(K=0, ld_theta=0, ld_phi=0) == -1
    assert call(K=7689, ld_theta=7689, ld_phi=7689) == -1
    for name in ("doc_off", "word", "theta", "phi_t"):
        assert call(**{name: None}) == -2, name
    assert call(ld_theta=7) == -2
    assert call(ld_phi=7) == -2
    assert call(V=0) == -2
    assert call(V=2 ** 31) == -2
    assert call(D=-1) == -2
    for name in ("doc_off", "theta", "phi_t", "mant", "expo", "tok", "bad"):
        assert call(**{name: 4100}) == -2, name                        # not 8-byte aligned
    for name in ("word", "freq"):
        assert call(**{name: 4098}) == -2, name                        # not 4-byte aligned
    assert call(D=0, doc_off=None, word=None, theta=None, phi_t=None) == 0           # nothing to score
    assert call(D=0, K=0) == -1                                        # (K is looked at first)


def test_python_surface_refuses_host_tensors_and_missing_device():
    import torch
    with pytest.raises(Exception) as e:
        heldout.loglik(torch.zeros((1, 2), dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64), [0, 0], [], None)
    assert isinstance(e.value, (ValueError, RuntimeError))             # no device: NativeError; a device: the tensors are not on it


def test_harness_option_is_off_by_default():
    from lda_thesis_amd import evaluate_LabeledLDA as E
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])[0].heldout_perplexity is False
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--heldout-perplexity"])[0].heldout_perplexity is True
