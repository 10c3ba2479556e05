"""numpy / ``fractions.Fraction`` restatement of ``llda_ecdf_ranks`` and ``llda_frex_select`` (include/llda_gibbs.h), of the drop-in
methods built on them, and the planted inputs their tests share (tests/test_frex_host.py, tests/test_gpu_ecdf_ranks.py,
tests/test_gpu_frex_select.py, tests/test_gpu_frex_dropin.py).

Pure numpy and Python integers: nothing here needs a GPU.

    sum64      64 partials, partial j over the entries j, j + 64, ... in increasing order from +0.0; then part[j] + part[j ^ s] for
               s = 1, 2, 4, 8, 16, 32, every j at once; the sum is part[0]  (tests/attrref.py)
    candidate  cand[w] != 0 and 0 < tot[w] < inf, tot = sum64 over ALL K columns
    value      mode 0: the entry; mode 1: the entry / tot[w], one division
    rank       np.searchsorted(np.sort(v[cand, k]), v[w, k], side="right") for a candidate, 0 for any other word
    order      sorted((Fraction(s rf + (t - s) re, re rf), w)) over the words with both ranks in 1 .. Vc
    report     (float(t) * float(re rf)) / (float(Vc) * float(s rf + (t - s) re)), each step rounded
"""
from fractions import Fraction

import numpy as np

from scoredref import matrix_rows, skewed, x_of_counts  # noqa: F401  (the generators of the scored-words tests)

LANES = 64
_XOR = [np.arange(LANES) ^ s for s in (1, 2, 4, 8, 16, 32)]
QNAN_BITS = 0x7FF8000000000000
QNAN = np.array([QNAN_BITS], dtype=np.uint64).view(np.float64)[0]


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


def candidates(mat, K, cand=None):
    """(is candidate bool [V], tot float64 [V]) of the (V, >= K) matrix; the columns >= K are not touched"""
    tot = sum64(np.asarray(mat, dtype=np.float64)[:, :K])
    with np.errstate(all="ignore"):
        c = (tot > 0) & (tot < np.inf)
    if cand is not None:
        c &= np.asarray(cand) != 0
    return c, tot


def values(mat, K, mode, c, tot):
    """(V, K) float64: the value of every candidate's entries, the quiet NaN in the rows of the other words"""
    v = np.asarray(mat, dtype=np.float64)[:, :K].copy()
    with np.errstate(all="ignore"):
        if mode:
            v = v / tot[:, None]
    v[~c] = QNAN
    return v


def ecdf_ranks_ref(mat, K, mode, cand=None, first=0, n_labels=None):
    """-> (rank (n_labels, V) int32, Vc, value (n_labels, V) float64)"""
    n_labels = K - first if n_labels is None else n_labels
    c, tot = candidates(mat, K, cand)
    v = values(mat, K, mode, c, tot)
    V = v.shape[0]
    rank = np.zeros((n_labels, V), dtype=np.int32)
    for l in range(n_labels):
        vc = v[c, first + l]
        rank[l, c] = np.searchsorted(np.sort(vc), vc, side="right")
    return rank, int(c.sum()), np.ascontiguousarray(v[:, first:first + n_labels].T)


def cost(re, rf, s, t):
    """the exact cost s / re + (t - s) / rf of two ranks >= 1"""
    re, rf = int(re), int(rf)
    return Fraction(s * rf + (t - s) * re, re * rf)


def report(re, rf, Vc, s, t):
    """the float64 that is reported for two ranks >= 1: Python floats, each step rounded"""
    re, rf = int(re), int(rf)
    return (float(t) * float(re * rf)) / (float(int(Vc)) * float(s * rf + (t - s) * re))


def frex_select_ref(rank_f, rank_e, Vc, s, t, n, probe=None):
    """-> (top_idx, top_rank_f, top_rank_e (L, n) int32[, probe_rank_f, probe_rank_e (L, m) int32])"""
    rank_f, rank_e = np.asarray(rank_f), np.asarray(rank_e)
    L, V = rank_f.shape
    idx = np.full((L, n), -1, dtype=np.int32)
    trf = np.zeros((L, n), dtype=np.int32)
    tre = np.zeros((L, n), dtype=np.int32)
    ranked = (rank_f >= 1) & (rank_e >= 1) & (rank_f <= Vc) & (rank_e <= Vc)
    for l in range(L):
        ws = np.flatnonzero(ranked[l])
        best = sorted((cost(rank_e[l, w], rank_f[l, w], s, t), int(w)) for w in ws)[:n]
        for i, (_, w) in enumerate(best):
            idx[l, i], trf[l, i], tre[l, i] = w, rank_f[l, w], rank_e[l, w]
    if probe is None:
        return idx, trf, tre
    probe = np.asarray(probe)
    prf = np.zeros(probe.shape, dtype=np.int32)
    pre = np.zeros(probe.shape, dtype=np.int32)
    for l in range(L):
        for j, w in enumerate(probe[l]):
            if 0 <= w < V and ranked[l, w]:
                prf[l, j], pre[l, j] = rank_f[l, w], rank_e[l, w]
    return idx, trf, tre, prf, pre


def report_table(rank_e, rank_f, Vc, s, t):
    """``report`` of every entry of two int tables; NaN where a rank is below 1"""
    rank_e, rank_f = np.asarray(rank_e), np.asarray(rank_f)
    out = np.full(rank_e.shape, np.nan, dtype=np.float64)
    for at in np.ndindex(*rank_e.shape):
        if rank_e[at] >= 1 and rank_f[at] >= 1:
            out[at] = report(rank_e[at], rank_f[at], Vc, s, t)
    return out


def weight_ref(w):
    f = Fraction(w).limit_denominator(64)
    return f.numerator, f.denominator


def frex_words_ref(phi_t, n, weight, cand):
    """what LabeledLDA.frex_words returns, from the (V, K) float64 phi_t and the candidate mask: ((K, n) int32, (K, n) float64)"""
    s, t = weight_ref(weight)
    phi_t = np.asarray(phi_t, dtype=np.float64)
    K = phi_t.shape[1]
    rank_f, Vc, _ = ecdf_ranks_ref(phi_t, K, 0, cand)
    rank_e, _, _ = ecdf_ranks_ref(phi_t, K, 1, cand)
    idx, trf, tre = frex_select_ref(rank_f, rank_e, max(Vc, 1), s, t, n)
    return idx, report_table(tre, trf, Vc, s, t)


def exclusivity_ref(phi_t, n, weight, cand):
    """what LabeledLDA.exclusivity returns: the reports of every label's n most probable candidate words (phi descending, then word
    id ascending, over cand != 0), added from +0.0 in that order; NaN where none of them is ranked"""
    s, t = weight_ref(weight)
    phi_t = np.asarray(phi_t, dtype=np.float64)
    K = phi_t.shape[1]
    rank_f, Vc, _ = ecdf_ranks_ref(phi_t, K, 0, cand)
    rank_e, _, _ = ecdf_ranks_ref(phi_t, K, 1, cand)
    words = np.flatnonzero(np.asarray(cand) != 0)
    out = np.full((K,), np.nan, dtype=np.float64)
    for k in range(K):
        total, any_ranked = 0.0, False
        for w in words[np.argsort(-phi_t[words, k], kind="stable")[:n]]:
            if rank_f[k, w] >= 1 and rank_e[k, w] >= 1:
                total, any_ranked = total + report(rank_e[k, w], rank_f[k, w], Vc, s, t), True
        if any_ranked:
            out[k] = total
    return out


# ---------------------------------------------------------------------------------------------- planted inputs
PLANTED_WEIGHTS = ((1, 2), (7, 10), (63, 64))
BIG = 1 << 30


def equal_cost_pairs(s, t, limit=40):
    """[((re, rf), (re', rf')), ...]: DIFFERENT rank pairs in 1 .. limit with EQUAL cost at s / t, found by enumeration"""
    seen, out = {}, []
    for re in range(1, limit + 1):
        for rf in range(1, limit + 1):
            c = cost(re, rf, s, t)
            if c in seen:
                out.append((seen[c], (re, rf)))
            else:
                seen[c] = (re, rf)
    return out


def planted_equal(s, t, V=300, seed=0):
    """(rank_f, rank_e (1, V) int32, Vc, [(w, w'), ...]): random ranks in 0 .. 60 with the twenty cheapest of ``equal_cost_pairs``,
    times ten, planted at chosen words: their costs are below every other word's, so they make up the head of the list, and within
    a pair the id decides"""
    rng = np.random.default_rng(1000 * s + t + seed)
    Vc = 400
    rank_f = rng.integers(0, 61, size=(1, V)).astype(np.int32)
    rank_e = rng.integers(0, 61, size=(1, V)).astype(np.int32)
    pairs = sorted(equal_cost_pairs(s, t), key=lambda p: cost(p[0][0], p[0][1], s, t))[:20]
    spots = rng.choice(V, size=2 * len(pairs), replace=False)
    planted = []
    for i, ((re, rf), (re2, rf2)) in enumerate(pairs):
        a, b = sorted(spots[2 * i:2 * i + 2])
        rank_e[0, b], rank_f[0, b] = 10 * re, 10 * rf
        rank_e[0, a], rank_f[0, a] = 10 * re2, 10 * rf2
        planted.append((int(a), int(b)))
    return rank_f, rank_e, Vc, planted


def planted_near_ties(s, t, words=300, span=130, seed=0):
    """(rank_f, rank_e (1, V) int32, Vc = 2^30): ranks 2^30 - i (exclusivity) and 2^30 - j (frequency), i, j < span <= 700.  To first
    order the cost of (i, j) is (t / 2^30) (1 + (s i + (t - s) j) / (t 2^30)): words with equal s i + (t - s) j differ in the cost by
    parts in 2^60 only.  The words are the lone best one, i = j = 0, and the members of the lowest such sums that have at least two
    members, until there are ``words`` of them, in a seeded shuffle of the ids: the head of the exact order is made of near ties."""
    u = t - s
    by_key = {}
    for i in range(span):
        for j in range(span):
            by_key.setdefault(s * i + u * j, []).append((i, j))
    members = [(0, 0)]
    for key in sorted(by_key):
        if len(by_key[key]) >= 2 and len(members) < words:
            members += [m for m in by_key[key] if m != (0, 0)]
    members = sorted(set(members))
    rng = np.random.default_rng(77 * s + t + seed)
    order = rng.permutation(len(members))
    rank_e = np.array([[BIG - members[o][0] for o in order]], dtype=np.int32)
    rank_f = np.array([[BIG - members[o][1] for o in order]], dtype=np.int32)
    return rank_f, rank_e, BIG


def double_order(rank_f, rank_e, Vc, s, t, n):
    """the list a comparator on the reported double would give: (report descending, word id ascending)"""
    ws = [w for w in range(rank_f.shape[1]) if rank_f[0, w] >= 1 and rank_e[0, w] >= 1]
    return sorted(ws, key=lambda w: (-report(rank_e[0, w], rank_f[0, w], Vc, s, t), w))[:n]


def straddle_matrix(V=5000, K=3, seed=11):
    """the (V, K) matrix of the chunk = 256 test: phi of skewed counts with few columns, so that many ROWS are equal as a whole
    (every count 0) -- their exclusivities tie as their phi do"""
    return x_of_counts(skewed(np.random.default_rng(seed), K, V), 0.01)


def tie_groups(v):
    """[(start, end, members), ...] of the runs of equal values in the descending order of the 1-d array v (positions in that
    order, end exclusive; members: the original indices), runs of at least two"""
    order = np.argsort(-v, kind="stable")
    sv = v[order]
    cut = np.flatnonzero(np.concatenate([[True], sv[1:] != sv[:-1], [True]]))
    return [(int(a), int(b), order[a:b]) for a, b in zip(cut[:-1], cut[1:]) if b - a >= 2]
