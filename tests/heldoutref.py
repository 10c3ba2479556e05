"""CPU restatement of llda_heldout_loglik (include/llda_gibbs.h), written from its specification: numpy float64 operations, each
rounded on its own, for the dot product; Python floats (IEEE float64) and Python integers for the pair products.

    dot      64 partials, partial j over the topics j, j + 64, ... in increasing order from +0.0; then part[j] + part[j ^ s] for
             s = 1, 2, 4, 8, 16, 32, every j at once; p = part[0]
    pair     (m, e), m in [0.5, 1); mul: c = a * b; c < 0.5: c = 2 c, exponent - 1
    site     (m, e) = frexp(p); p^f by right-to-left binary exponentiation from (0.5, 1)
    document the sites' p^f multiplied in ascending order from (0.5, 1); tok += f; a site whose p is not a finite positive number
             (or whose word is outside [0, V)) adds f to bad instead
"""
import math

import numpy as np

LANES = 64
_XOR = [np.arange(LANES) ^ s for s in (1, 2, 4, 8, 16, 32)]


def dot64(theta_row, phi_rows, K):
    """p of every row of phi_rows (n, >= K) against theta_row (>= K): float64 [n].  Columns >= K are not touched."""
    n = phi_rows.shape[0]
    part = np.zeros((n, LANES), dtype=np.float64)                      # +0.0
    with np.errstate(all="ignore"):
        for i in range(0, K, LANES):                                       # the 64 partials take their next topic, each its own
            w = min(LANES, K - i)
            prod = theta_row[None, i:i + w] * phi_rows[:, i:i + w]         # rounded
            part[:, :w] = part[:, :w] + prod                               # rounded
        for x in _XOR:
            part = part + part[:, x]
    return part[:, 0]


def pair_mul(a, ea, b, eb):
    c = a * b
    e = ea + eb
    if c < 0.5:
        c = c + c
        e -= 1
    return c, e


def pair_pow(p, f):
    """p^f as a pair, p a finite positive float, f >= 0"""
    m, e = math.frexp(p)
    acc, base = (0.5, 1), (m, e)
    while f:
        if f & 1:
            acc = pair_mul(acc[0], acc[1], base[0], base[1])
        base = pair_mul(base[0], base[1], base[0], base[1])
        f >>= 1
    return acc


def loglik_ref(theta, phi_t, doc_off, word, freq, K=None, V=None):
    """theta (D, >= K), phi_t (V, >= K) float64; CSR doc_off / word / freq (None: all 1) -> (mant float64 [D], expo, tok, bad
    int64 [D])"""
    D = len(doc_off) - 1
    K = theta.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    mant, expo = np.empty(D, dtype=np.float64), np.empty(D, dtype=np.int64)
    tok, bad = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    for d in range(D):
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        ws = np.asarray(word[b:e], dtype=np.int64)
        fs = [1] * (e - b) if freq is None else [int(x) for x in freq[b:e]]
        inside = (ws >= 0) & (ws < V)
        p = np.full(e - b, np.nan)
        if inside.any():
            p[inside] = dot64(theta[d], phi_t[ws[inside]], K)
        acc = (0.5, 1)
        for pv, f in zip(p.tolist(), fs):
            if not (pv > 0.0 and pv < math.inf):
                bad[d] += f
                continue
            site = pair_pow(pv, f)
            acc = pair_mul(acc[0], acc[1], site[0], site[1])
            tok[d] += f
        mant[d], expo[d] = acc
    return mant, expo, tok, bad
