"""CPU restatement of llda_attribute (include/llda_gibbs.h), written from its specification: numpy float64 operations, each rounded
on its own.

    sum64    64 partials, partial j over the entries j, j + 64, ... in increasing order from +0.0; then part[j] + part[j ^ s] for
             s = 1, 2, 4, 8, 16, 32, every j at once; the sum is part[0]  (heldoutref.dot64's tree)
    site     t_k = theta_k * phi_t[w][k]; p = sum64(t); good: w in [0, V) and 2^-960 <= p < inf, else bad += f and nothing else;
             good: tok += f; inv = 1 / p; g = f * inv; credit_k = credit_k + t_k * g, sites in ascending order from +0.0
    step     (a document with sites only) num_k = theta_k > 0 ? credit_k + alpha : 0; den = sum64(num); 0 < den < inf:
             theta_k = num_k / den; then the credit again from zero
    last     r_k = t_k * inv; the labels with r_k > 0 by (r_k descending, k ascending), the first top_m, padded with -1 / 0.0
"""
import numpy as np

from heldoutref import LANES, _XOR

MIN_P = 2.0 ** -960


def sum64(x):
    """the 64-partial tree over the rows of x (n, K): float64 [n]"""
    n, K = x.shape
    part = np.zeros((n, LANES), dtype=np.float64)                          # +0.0
    with np.errstate(all="ignore"):
        for i in range(0, K, LANES):
            w = min(LANES, K - i)
            part[:, :w] = part[:, :w] + x[:, i:i + w]
        for perm in _XOR:
            part = part + part[:, perm]
    return part[:, 0]


def estep(th, rows, inside, fs, top_m):
    """one pass over a document's sites: th [K], rows (n, K) the sites' rows of phi_t (anything where not inside), fs [n] ints ->
    credit [K], tok, bad, site_idx (n, top_m), site_val (n, top_m)"""
    n, K = rows.shape
    credit = np.zeros(K, dtype=np.float64)
    idx = np.full((n, top_m), -1, dtype=np.int32)
    val = np.zeros((n, top_m), dtype=np.float64)
    tok = bad = 0
    with np.errstate(all="ignore"):
        t = th[None, :] * rows
        p = sum64(t)
        good = inside & (p >= MIN_P) & (p < np.inf)
        for s in range(n):
            if not good[s]:
                bad += fs[s]
                continue
            tok += fs[s]
            inv = np.float64(1.0) / p[s]
            g = np.float64(fs[s]) * inv
            credit = credit + t[s] * g
            if top_m:
                r = t[s] * inv
                ks = np.flatnonzero(r > 0.0)
                ks = ks[np.lexsort((ks, -r[ks]))][:top_m]                  # r descending, then k ascending
                idx[s, :len(ks)] = ks
                val[s, :len(ks)] = r[ks]
    return credit, tok, bad, idx, val


def attribute_ref(theta, phi_t, doc_off, word, freq, K=None, V=None, iters=0, alpha=0.0, top_m=0):
    """theta (D, >= K), phi_t (V, >= K) float64; CSR doc_off / word / freq (None: all 1) -> dict(theta_out (D, K), credit (D, K),
    site_idx (S, top_m) int32, site_val (S, top_m), tok, bad int64 [D])"""
    D = len(doc_off) - 1
    K = theta.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    S = int(doc_off[-1])
    out = dict(theta_out=np.empty((D, K)), credit=np.empty((D, K)), site_idx=np.full((S, top_m), -1, dtype=np.int32),
               site_val=np.zeros((S, top_m)), tok=np.zeros(D, dtype=np.int64), bad=np.zeros(D, dtype=np.int64))
    for d in range(D):
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        ws = np.asarray(word[b:e], dtype=np.int64)
        fs = [1] * (e - b) if freq is None else [int(x) for x in freq[b:e]]
        inside = (ws >= 0) & (ws < V)
        rows = phi_t[np.where(inside, ws, 0)][:, :K]
        th = np.array(theta[d, :K], dtype=np.float64)
        steps = iters if e > b else 0                                      # (a document without sites keeps its loads)
        for step in range(steps + 1):
            r = estep(th, rows, inside, fs, top_m if step == steps else 0)
            if step == steps:
                break
            with np.errstate(all="ignore"):
                num = np.where(th > 0.0, r[0] + np.float64(alpha), 0.0)
                den = sum64(num[None, :])[0]
                if den > 0.0 and den < np.inf:
                    th = num / den
        out["theta_out"][d], out["credit"][d], out["tok"][d], out["bad"][d] = th, r[0], r[1], r[2]
        out["site_idx"][b:e], out["site_val"][b:e] = r[3], r[4]
    return out


def objective(theta_row, phi_t, ws, fs, alpha, K):
    """sum f log p + alpha * sum_{theta_k > 0} log theta_k over the good sites of one document (plain float64; for the monotonicity
    check only)"""
    th = theta_row[:K]
    p = phi_t[ws][:, :K] @ th
    ok = (p >= MIN_P) & np.isfinite(p)
    return float(np.sum(np.asarray(fs, dtype=np.float64)[ok] * np.log(p[ok])) + alpha * np.sum(np.log(th[th > 0.0])))
