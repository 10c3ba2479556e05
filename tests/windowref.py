"""Restatement of ``llda_window_cooc`` (include/llda_gibbs.h) and of the sliding-window coherence measures of
``lda_thesis_amd/topics.py`` (tests/test_window_host.py, tests/test_gpu_window_cooc.py, tests/test_gpu_window_dropin.py).

The count is the brute force: every window of every document gets the set of listed words it holds, then loops over the topics
and ranks of those words.  (Two windows that hold the same set add the same pairs; the pairs of a set are looked up once.)  The
measures are plain loops with ``math.log``, each with the bound by which the numpy form may differ from it.

Pure numpy and python: nothing here needs a GPU.
"""
import math

import numpy as np

EPS = 1e-12
U = 2.0 ** -52


def windows_of(L, s):
    """the (start, stop) of every window of a document of L tokens at window s"""
    if L == 0:
        return []
    if s == 0 or L <= s:
        return [(0, L)]
    return [(w, w + s) for w in range(L - s + 1)]


def window_count_ref(tok_off, s):
    return sum(len(windows_of(int(b) - int(a), s)) for a, b in zip(tok_off[:-1], tok_off[1:]))


def window_ref(tok_off, tok, top_idx, s, lo=0, hi=None):
    """(K, n, n) int64: for every window and topic k, R = the ranks whose word the window holds; co[k][i][j] += 1 for i >= j in R."""
    top_idx = np.asarray(top_idx)
    K, n = top_idx.shape
    lists = {}
    for k in range(K):
        for r in range(n):
            if top_idx[k, r] >= 0:
                lists.setdefault(int(top_idx[k, r]), []).append((k, r))
    words = sorted(lists)
    slot = {w: i + 1 for i, w in enumerate(words)}                    # 0 = a position without a listed word
    tok = np.asarray(tok)
    co = np.zeros((K, n, n), dtype=np.int64)
    adds = {}                                                         # the present words of a window -> the entries it adds to
    hi = len(tok_off) - 1 if hi is None else hi
    for d in range(lo, hi):
        doc = np.array([slot.get(int(w), 0) for w in tok[int(tok_off[d]):int(tok_off[d + 1])]], dtype=np.int64)
        for a, b in windows_of(len(doc), s):
            present = np.flatnonzero(np.bincount(doc[a:b], minlength=len(words) + 1)[1:])
            key = present.tobytes()
            if key not in adds:
                ranks = {}
                for i in present:
                    for k, r in lists[words[i]]:
                        ranks.setdefault(k, set()).add(r)
                e = [(k, i, j) for k, R in ranks.items() for i in R for j in R if i >= j]
                adds[key] = tuple(np.array(x, dtype=np.int64) for x in zip(*e)) if e else None
            if adds[key] is not None:
                co[adds[key]] += 1                                    # (every entry once: a plain indexed add)
    return co


def _topic(co_k, on):
    """the listed ranks of one topic, or None under the NaN rule"""
    ranks = [r for r in range(co_k.shape[0]) if on[r]]
    if len(ranks) < 2 or any(int(co_k[r, r]) == 0 for r in ranks):
        return None
    return ranks


def _pmi_nlr(co_k, N, i, j):
    c_ij = float(co_k[max(i, j), min(i, j)])
    p_i, p_j, p_ij = float(co_k[i, i]) / N, float(co_k[j, j]) / N, c_ij / N
    pmi = math.log((p_ij + EPS) / (p_i * p_j))
    return pmi, pmi / -math.log(p_ij + EPS)


def pair_mean_ref(co_k, N, on, which):
    """c_uci (which = 0) or c_npmi (1) of one topic -> (value or nan, bound).
    Bound, derived: the arguments of every logarithm are the same IEEE operations in the same order here and in numpy, so they are the
    same doubles; two logarithms that are each within one ulp of the truth differ by at most 2 U |log| (U = 2^-52), a quotient of two
    such by 5 U |term|; a pairwise and a sequential sum of P terms by (P - 1) U sum|term|, the division by P by another U."""
    ranks = _topic(co_k, on)
    if ranks is None:
        return float("nan"), 0.0
    N = float(N)
    tot = mag = 0.0
    pairs = 0
    for i in ranks:
        for j in ranks:
            if i > j:
                t = _pmi_nlr(co_k, N, i, j)[which]
                tot += t
                mag += abs(t)
                pairs += 1
    return tot / pairs, (pairs + 5) * U * mag / pairs


def cosine_mean_ref(M):
    """the tail of c_v on a matrix given as lists -> (value, bound); see c_v_ref"""
    m = len(M)
    v = [0.0] * m
    dv = [0.0] * m
    for b in range(m):
        for a in range(m):
            v[b] += M[a][b]
            dv[b] += abs(M[a][b])
        dv[b] *= (m + 5) * U
    nv = math.sqrt(sum(x * x for x in v))
    d_nv = math.sqrt(sum(x * x for x in dv)) + (m / 2 + 2) * U * nv
    tot = mag = err = 0.0
    for a in range(m):
        dot = sum(M[a][b] * v[b] for b in range(m))
        nu = math.sqrt(sum(M[a][b] * M[a][b] for b in range(m)))
        if nu == 0.0 or nv == 0.0:
            continue
        cos = dot / (nu * nv)
        d_dot = sum(abs(M[a][b]) * dv[b] + (5 + m + 1) * U * abs(M[a][b] * v[b]) for b in range(m))
        err += d_dot / (nu * nv) + abs(cos) * ((m + 9) * U + d_nv / nv)
        tot += cos
        mag += abs(cos)
    return tot / m, err / m + (m + 1) * U * mag / m


def c_v_ref(co_k, N, on):
    """c_v of one topic -> (value or nan, bound).
    Bound, first order, U = 2^-52: an entry M[a][b] differs by at most 5 U |M[a][b]| (pair_mean_ref); v[b] = sum_a M[a][b] by
    dv[b] = (m + 5) U sum_a |M[a][b]|; the dot product u_a . v by d_dot = sum_b (|M[a][b]| dv[b] + (5 + m + 1) U |M[a][b] v[b]|) (the
    entries, the products and the sum); |u_a| by (m + 7) U |u_a| and |v| by d_nv = |dv| + (m / 2 + 2) U |v|; the cosine by
    d_dot / (|u_a| |v|) + |cos| ((m + 7) U + d_nv / |v| + 2 U); the mean of m cosines by their mean error + (m + 1) U mean|cos|."""
    ranks = _topic(co_k, on)
    if ranks is None:
        return float("nan"), 0.0
    N = float(N)
    return cosine_mean_ref([[_pmi_nlr(co_k, N, a, b)[1] for b in ranks] for a in ranks])


def coherence_ref(co, N, measure, listed=None):
    """(values [K], bounds [K]) of a (K, n, n) table by name"""
    co = np.asarray(co)
    on = np.ones(co.shape[:2], dtype=bool) if listed is None else np.asarray(listed) >= 0
    one = {"c_uci": lambda c, o: pair_mean_ref(c, N, o, 0), "c_npmi": lambda c, o: pair_mean_ref(c, N, o, 1),
           "c_v": lambda c, o: c_v_ref(c, N, o)}[measure]
    got = [one(co[k], on[k]) for k in range(co.shape[0])]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])
