"""CPU restatement of llda_left_to_right (include/llda_gibbs.h), written from its specification: numpy float64 operations, each
rounded on its own, vectorised over the documents of a batch and their particles (which do not influence one another).

    x(c, w)      ((double)c[k] + alpha) * phi_t[w][k] for the allowed k, +0.0 for the others
    draw64       lane j owns x[j + 64 i]; sequential prefix over i; Hillis-Steele scan of the lane totals; t = u * X[63];
                 t_j = t - X[j-1]; first (j, i), lanes first, with x > 0 and q > t_j, else the last with x > 0, else none (-1)
    sum64        heldoutref's: 64 partials from +0.0, then part[j] + part[j ^ s], s = 1 .. 32
    position n   resample the assigned m < n in order with u(n, r, m); S_r = sum64(x(c_r, w_n)); pred_r = S_r / (assigned + A alpha);
                 0 < S_r < inf: z_r[n] = draw64(x, u(n, r, n)); p_n = (pred_0 + ... + pred_{R-1}) / R; pair *= frexp(p_n)
"""
import math

import numpy as np

from heldoutref import LANES, _XOR, pair_mul
from llda_oracle import keyed_uniform

NONE = -1


def slots(K):
    """slots per lane the kernel gives K topics: K / 64 rounded up to 1, 2, 4, 8 or 16"""
    ni = 1
    while 64 * ni < K:
        ni *= 2
    return ni


def _grid(x, NI):
    """(P, K) -> (P, NI, 64) with [p, i, j] = x[p, j + 64 i], +0.0 where there is no topic"""
    P, K = x.shape
    out = np.zeros((P, NI * LANES), dtype=np.float64)
    out[:, :K] = x
    return out.reshape(P, NI, LANES)


def masked(x, m):
    """the weights of the topics that are not allowed are +0.0 (on its own so that a test can take the mask away)"""
    return np.where(m, x, 0.0)


def draw64(x, u, stats=None):
    """x (P, K) weights, u (P,) uniforms -> int64 (P,) topics, -1 where no weight is > 0.  stats: a dict whose 'draws' and 'no_hit'
    are raised by the draws that had a weight > 0 and by those of them that no q > t_j decided (the "last with x > 0" rule)"""
    x = np.asarray(x, dtype=np.float64)
    P, K = x.shape
    NI = slots(K)
    g = _grid(x, NI)
    with np.errstate(all="ignore"):
        q = g.copy()
        for i in range(1, NI):
            q[:, i] = q[:, i - 1] + g[:, i]
        X = q[:, NI - 1].copy()
        d = 1
        while d < LANES:
            Y = X.copy()
            Y[:, d:] = X[:, :-d] + X[:, d:]
            X = Y
            d *= 2
        t = np.asarray(u, dtype=np.float64) * X[:, LANES - 1]
        off = np.concatenate([np.zeros((P, 1)), X[:, :-1]], axis=1)
        tg = t[:, None] - off
        pos = g > 0.0
        flag = pos & (q > tg[:, None, :])
    flag = flag.transpose(0, 2, 1).reshape(P, -1)                       # lane-major: (j, i) at j * NI + i
    pos = pos.transpose(0, 2, 1).reshape(P, -1)
    first = np.argmax(flag, axis=1)
    last = pos.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1)
    at = np.where(flag.any(axis=1), first, last)
    if stats is not None:
        stats["draws"] = stats.get("draws", 0) + int(pos.any(axis=1).sum())
        stats["no_hit"] = stats.get("no_hit", 0) + int((pos.any(axis=1) & ~flag.any(axis=1)).sum())
    topic = at // NI + LANES * (at % NI)
    return np.where(pos.any(axis=1), topic, NONE).astype(np.int64)


def sum64(x):
    """x (P, K) -> (P,)"""
    x = np.asarray(x, dtype=np.float64)
    NI = slots(x.shape[1])
    g = _grid(x, NI)
    with np.errstate(all="ignore"):
        part = np.zeros((x.shape[0], LANES), dtype=np.float64)
        for i in range(NI):
            part = part + g[:, i]
        for xo in _XOR:
            part = part + part[:, xo]
    return part[:, 0]


def left_to_right_ref(phi_t, doc_off, word, alpha, R, seed, stream_id, K=None, V=None, allowed=None, doc_ids=None, max_doc_tokens=None,
                      trace=None, stats=None):
    """phi_t (V, >= K) float64; token CSR; allowed (D, >= K) or None; doc_ids [D] or None (= 0, 1, ...) -> (mant float64 [D], expo, tok,
    bad int64 [D], status).  trace: a dict that receives 'z' (D, R, Nmax) and 'p' (D, Nmax), the final assignments and the p_n;
    stats: a dict for draw64's counts (the resampling draws and the extensions together)."""
    draw = draw64 if stats is None else (lambda x, u: draw64(x, u, stats))
    phi_t = np.asarray(phi_t, dtype=np.float64)
    D = len(doc_off) - 1
    K = phi_t.shape[1] if K is None else int(K)
    V = phi_t.shape[0] if V is None else int(V)
    alpha = float(alpha)
    lens = np.array([int(doc_off[d + 1]) - int(doc_off[d]) for d in range(D)], dtype=np.int64)
    status = 0
    if max_doc_tokens is not None:
        if np.any(lens > max_doc_tokens):
            status = 1
        lens = np.where(lens > max_doc_tokens, 0, lens)
    ids = np.arange(D, dtype=np.int64) if doc_ids is None else np.asarray(doc_ids, dtype=np.int64)
    mask = np.ones((D, K), dtype=bool) if allowed is None else (np.asarray(allowed)[:, :K] != 0)
    a_alpha = mask.sum(axis=1).astype(np.float64) * alpha               # (double)A * alpha
    Nmax = int(lens.max()) if D else 0
    words = np.full((D, max(Nmax, 1)), -1, dtype=np.int64)
    for d in range(D):
        words[d, :lens[d]] = np.asarray(word[int(doc_off[d]):int(doc_off[d]) + int(lens[d])], dtype=np.int64)
    # particle p = d * R + r
    pd = np.repeat(np.arange(D), R)
    pr = np.tile(np.arange(R, dtype=np.int64), D)
    p_doc = (ids[pd] & 0xFFFFFFFF).astype(np.uint64)
    p_stream = ((int(stream_id) + pr) & 0xFFFFFFFF).astype(np.uint64)
    c = np.zeros((D * R, K), dtype=np.float64)                          # exact small integers
    z = np.full((D * R, max(Nmax, 1)), NONE, dtype=np.int64)
    assigned = np.zeros(D * R, dtype=np.float64)
    acc = [(0.5, 1)] * D
    tok, bad = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    p_all = np.full((D, max(Nmax, 1)), np.nan)

    def weights(p, w):
        with np.errstate(all="ignore"):
            x = (c[p] + alpha) * phi_t[w, :K]
        return masked(x, mask[pd[p]])

    for n in range(Nmax):
        live = np.nonzero(lens[pd] > n)[0]                              # the particles of the documents that have a position n
        u = keyed_uniform(seed, n, p_stream[live, None], p_doc[live, None], np.arange(n + 1, dtype=np.uint64)[None, :])
        for m in range(n):
            sel = z[live, m] != NONE
            if not sel.any():
                continue
            p = live[sel]
            zo = z[p, m]
            c[p, zo] -= 1.0
            zn = draw(weights(p, words[pd[p], m]), u[sel, m])
            zn = np.where(zn < 0, zo, zn)
            c[p, zn] += 1.0
            z[p, m] = zn
        w = words[pd[live], n]
        ok = (w >= 0) & (w < V)
        x = weights(live, np.where(ok, w, 0))
        S = np.where(ok, sum64(x), np.nan)
        with np.errstate(all="ignore"):
            pred = S / (assigned[live] + a_alpha[pd[live]])
            go = (S > 0.0) & (S < np.inf)
        if go.any():
            p = live[go]
            zn = draw(x[go], u[go, n])
            hit = zn >= 0
            c[p[hit], zn[hit]] += 1.0
            z[p[hit], n] = zn[hit]
            assigned[p[hit]] += 1.0
        docs = pd[live[::R]]
        pred = pred.reshape(-1, R)
        with np.errstate(all="ignore"):
            tot = np.zeros(len(docs), dtype=np.float64)
            for r in range(R):
                tot = tot + pred[:, r]
            pn = tot / float(R)
        for d, pv in zip(docs.tolist(), pn.tolist()):
            p_all[d, n] = pv
            if pv > 0.0 and pv < math.inf:
                m_, e_ = math.frexp(pv)
                acc[d] = pair_mul(acc[d][0], acc[d][1], m_, e_)
                tok[d] += 1
            else:
                bad[d] += 1
    mant = np.array([a[0] for a in acc], dtype=np.float64).reshape(D)
    expo = np.array([a[1] for a in acc], dtype=np.int64).reshape(D)
    if trace is not None:
        trace["z"] = z.reshape(D, R, -1)
        trace["p"] = p_all
    return mant, expo, tok, bad, status
