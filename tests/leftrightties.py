"""Adversarial inputs for llda_left_to_right: last-bit ties of draw64, the "no hit -> last with x > 0" rule, loadings at both ends
of the double range (test infrastructure, host only: numpy + oracle/ + tests/leftrightref.py).

On random data a 53-bit uniform never puts u * X[63] on a prefix, and never behind the last one, so the strict `>` of
`q[j][i] > t_j`, the lane-major order of the positions and the fall-back of a draw that nothing decides are not exercised by anything
random.  This module plants such draws:

  * ``exact_case``: documents of two tokens whose words occur nowhere else.  The extension draw of position 0 cannot be observed
    (position 0 is resampled at n = 1 from zero counts before anything reads it); the draw that shows is that resampling, with
    u(1, r, 0) and x[k] = alpha * phi_t[w0][k].  With alpha = 0.25 and phi_t[w0][k] = a_k * 2^-51, the integers a_k summing to 2^53
    over the allowed topics, every x, prefix, scan value and t_j is an exact multiple of 2^-53 and t = u * 1.0: the draw is the first
    position in lane-major order whose integer cumulative exceeds U = u * 2^53.  ``int_model`` computes that in Python integers; it
    does not come from leftrightref.  The cumulative at a chosen boundary (KINDS) is U (``tie``: the boundary is not taken), U + 1
    (``above``) or U - 1 (``below``).  phi_t[w1][k] = (k + 1) / (2 K), so p_1 -- and with it (mant, expo) -- names z_0 (``decode_z0``).
  * ``tuned_case``: documents of 4 .. 10 tokens whose last-but-one word occurs once; the final z of that position is the outcome of
    the last resampling before the last prediction, with counts in play.  The word's boundary entry is bisected, the restatement
    re-run on the documents as the oracle, down to two adjacent doubles between which that topic flips; the upper double is planted
    in half of the documents, the lower in the other half.
  * ``scaled_case``: every row times an exact power of two, the site totals at the SCALES.  In the subnormal cases u * X[63] is
    rounded onto the subnormal grid and reaches X[63] itself for u near 1: the no-hit rule at work without an overflow.
  * ``overflow_case``: the document B B A A A B X X.  Word B loads 0.9 * 2^1023 on two topics k1, k2, word A is one-hot on k1: from
    n = 3 on the resampling of position 0 sees X[63] = inf, t_j = inf or NaN, no hit -- and returns the lane-major last of (k1, k2).

With R > 1 only particle r_star is planted: its uniforms are those of the stream (STREAM + r_star) mod 2^32, which is all a plant
depends on, so the builders tune with R = 1 on that stream.  Planted and random documents alternate in every case; some document
ids are at or above 2^32 (the device and the restatement key the draw with their low 32 bits).
"""
import functools
import math

import numpy as np

import leftrightref as ref
from heldoutref import pair_mul
from llda_oracle import keyed_uniform

SEED = 0xC0FFEE1234567
STREAM = 0xFFFFFFF8                               # stream_id + r wraps around 2^32 from r = 8 on
KINDS = ("lane0_first", "slot_seam", "lane_end", "zero_lane", "before_last")
#   lane0_first : the first positive position of lane 0 (nothing in front of it: t_j = t itself)
#   slot_seam   : the next positive position is the next slot of the same lane (K > 64)
#   lane_end    : the last slot of a lane, the next positive position in the next lane (prefix = a lane total = a scan value)
#   zero_lane   : exact zeros from the boundary through the whole next lane: the next positive position is two lanes on.  Half by
#                 phi_t == 0, half by allowed == 0 over loadings of 2^40 (a mask applied after the prefix would show)
#   before_last : the boundary in front of the last positive position
CLASSES = ("tie", "above", "below")
V_RANDOM = 30
ALPHA_EXACT = 0.25
ALPHA = 0.3
ONE = 1 << 53
POISON = 2.0 ** 40
N_TUNED = 24
# name -> exponent E: (alpha + 1) * sum(row) in [2^E, 2^(E+1)); "top": alpha * sum(row) there, so every total is above 1e300 = 2^996.6
SCALES = {"sub1066": -1066, "sub1045": -1045, "tiny1000": -1000, "big960": 960, "top": 998}
SCALED_R = 3


def lane_major(K):
    """the topics in draw order: lane k mod 64 first, then slot k / 64"""
    NI = ref.slots(K)
    return [j + 64 * i for j in range(64) for i in range(NI) if j + 64 * i < K]


def kinds_of(K):
    return tuple(k for k in KINDS if not (k == "slot_seam" and K <= 64) and not (k == "zero_lane" and K < 3))


def uniform(n, stream, doc, m):
    return float(keyed_uniform(SEED, n, np.uint64(stream & 0xFFFFFFFF), np.uint64(doc & 0xFFFFFFFF), np.uint64(m)))


def doc_ids(D):
    """1000 + d; every fifth at or above 2^32, one above 2^33"""
    ids = 1000 + np.arange(D, dtype=np.int64)
    ids[::5] += 3 << 32
    if D > 2:
        ids[2] += 1 << 33
    return ids


def int_model(a, U, order=None):
    """a[k] integer weights -> the first topic, in lane-major order (or the given one), whose inclusive cumulative exceeds U"""
    cum = 0
    for k in (lane_major(len(a)) if order is None else order):
        cum += a[k]
        if a[k] > 0 and cum > U:
            return k
    raise AssertionError("U is not below the total")


def _pattern(K, kind, rng, upper_slots=False):
    """-> (ranks of the positive positions in draw order, index of the boundary among them); the next positive position follows.
    upper_slots: one of the other positive positions is in a slot above 0 where the kind leaves room for one"""
    order = lane_major(K)
    lane = [k % 64 for k in order]
    n_lanes = min(K, 64)
    first = [lane.index(j) for j in range(n_lanes)] + [K]              # the rank at which lane j begins
    if kind == "lane0_first":
        b = min(int(rng.integers(0, first[1])), K - 2)                 # (lane 0 holds the ranks 0 .. first[1] - 1)
        nx = int(rng.integers(b + 1, K))
        lo, hi = [], list(range(nx + 1, K))
    elif kind == "slot_seam":
        j = int(rng.integers(0, sum(1 for x in range(n_lanes) if first[x + 1] - first[x] > 1)))
        b = int(rng.integers(first[j], first[j + 1] - 1))
        nx = b + 1
        lo, hi = list(range(b)), list(range(nx + 1, K))
    elif kind == "lane_end":
        j = int(rng.integers(0, n_lanes - 1))
        b = first[j + 1] - 1
        nx = int(rng.integers(first[j + 1], first[j + 2]))
        lo, hi = list(range(b)), list(range(nx + 1, K))
    elif kind == "zero_lane":
        j = int(rng.integers(0, n_lanes - 2))
        b = int(rng.integers(first[j], first[j + 1]))
        nx = first[j + 2]
        lo, hi = list(range(b)), list(range(nx + 1, K))
    else:
        b = int(rng.integers(0, K - 1))
        nx = int(rng.integers(b + 1, K))
        lo, hi = list(range(b)), []
    extra = min(int(rng.integers(0, 7)), len(lo) + len(hi))
    pool = lo + hi
    more = sorted(int(x) for x in rng.choice(len(pool), size=extra, replace=False)) if extra else []
    ranks = set([pool[i] for i in more] + [b, nx])
    upper = [r for r in pool if order[r] >= 64]
    if upper_slots and upper:
        ranks.add(upper[int(rng.integers(0, len(upper)))])
    ranks = sorted(ranks)
    return ranks, ranks.index(b)


def _cuts(rng, lo, hi, n):
    """n distinct integers in [lo, hi), ascending"""
    assert hi - lo >= n
    got = set()
    while len(got) < n:
        got.add(int(rng.integers(lo, hi)))
    return sorted(got)


# ------------------------------------------------------------------------------------------------
# the random documents that go between the planted ones
# ------------------------------------------------------------------------------------------------
def random_loadings(rng, K, V=V_RANDOM):
    """positive loadings across eight orders of magnitude, three topics in ten exact zeros; every word loads on some topic"""
    phi = rng.gamma(0.5, size=(V, K)) * 10.0 ** rng.uniform(-8, 0, size=(V, K)) + 1e-300
    phi[rng.random((V, K)) < 0.3] = 0.0
    phi[np.arange(V), np.arange(V) % K] += 1e-3
    return phi


RANDOM_LENS = (3, 0, 7, 1, 12, 2, 5, 9)


def _assemble(K, planted_docs, planted_allowed, phi_planted, rng):
    """planted and random documents alternate (planted first) -> dict(phi_t, doc_off, word, allowed, doc_ids, docs_of_plants)"""
    phi = np.vstack([random_loadings(rng, K), phi_planted])
    docs, allowed, where = [], [], []
    for j, ws in enumerate(planted_docs):
        where.append(len(docs))
        docs.append(list(ws))
        allowed.append(planted_allowed[j])
        docs.append(rng.integers(0, V_RANDOM, size=RANDOM_LENS[j % len(RANDOM_LENS)]).tolist())
        row = np.ones(K, dtype=np.uint8)
        if j % 3 == 1 and K > 1:
            row[rng.random(K) < 0.5] = 0
            row[int(rng.integers(0, K))] = 1
        allowed.append(row)
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    word = np.array([w for t in docs for w in t], dtype=np.int64)
    return dict(K=K, phi_t=phi, doc_off=doc_off, word=word, allowed=np.array(allowed, dtype=np.uint8), doc_ids=doc_ids(len(docs)),
                where=np.array(where, dtype=np.int64))


def expected(c, R, **kw):
    """the restatement on a case -> (mant, expo, tok, bad, status)"""
    with np.errstate(all="ignore"):
        return ref.left_to_right_ref(c["phi_t"], c["doc_off"], c["word"], c["alpha"], R, SEED, STREAM, K=c["K"], allowed=c["allowed"],
                                     doc_ids=c["doc_ids"], **kw)


# ------------------------------------------------------------------------------------------------
# exact_case
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _exact_plants(K, r_star):
    order = lane_major(K)
    kinds = kinds_of(K)
    n_plant = 6 * len(kinds) * len(CLASSES)                            # kind x class x (zero_lane: masked or not), three times each
    rng = np.random.default_rng([31, K, r_star])
    ids = doc_ids(2 * n_plant)
    phi = np.zeros((2 * n_plant, K))
    allowed = np.ones((n_plant, K), dtype=np.uint8)
    plants = []
    for j in range(n_plant):
        kind, cls = kinds[j % len(kinds)], CLASSES[(j // len(kinds)) % 3]
        use_mask = kind == "zero_lane" and (j // (3 * len(kinds))) % 2 == 1
        u = uniform(1, STREAM + r_star, int(ids[2 * j]), 0)
        U = int(u * ONE)
        assert U * 2.0 ** -53 == u
        target = U + {"tie": 0, "above": 1, "below": -1}[cls]
        for attempt in range(100):
            ranks, ib = _pattern(K, kind, rng, upper_slots=attempt % 2 == 1)
            n_after = len(ranks) - ib - 1
            assert len(ranks) < U < ONE - len(ranks), "the uniform of document %d leaves no room for a plant" % j
            cuts = _cuts(rng, 1, target, ib) + [target] + _cuts(rng, target + 1, ONE, n_after - 1) + [ONE]
            a = [0] * K
            for i, r in enumerate(ranks):
                a[order[r]] = cuts[i] - (cuts[i - 1] if i else 0)
            z = int_model(a, U)
            # (K > 64: a tie that the topic-major order decides differently, wherever the uniform leaves room for one)
            if cls != "tie" or K <= 64 or int_model(a, U, range(K)) != z:
                break
        assert all(a[order[r]] > 0 for r in ranks) and sum(a) == ONE
        assert sum(a[order[r]] for r in ranks[:ib + 1]) == target
        assert z == (order[ranks[ib]] if cls == "above" else order[ranks[ib + 1]])
        row = np.array([float(x) for x in a]) * 2.0 ** -51
        assert all(int(v * 2.0 ** 51) == x for v, x in zip(row.tolist(), a))
        if use_mask:
            for r in range(ranks[ib] + 1, ranks[ib + 1]):
                row[order[r]] = POISON
                allowed[j, order[r]] = 0
            assert (allowed[j] == 0).any()
        phi[2 * j] = row
        phi[2 * j + 1] = (np.arange(K) + 1.0) / (2 * K)
        plants.append(dict(kind=kind, cls=cls, masked=use_mask, z0=z, z0_topic_major=int_model(a, U, range(K)),
                           positives=[order[r] for r in ranks], U=U))
    return phi, allowed, plants


@functools.lru_cache(maxsize=None)
def exact_case(K, R, r_star):
    """-> dict: the case (phi_t, doc_off, word, allowed, doc_ids, alpha), where[j] the document of plant j, plants[j] its facts
    (kind, cls, masked, z0 by the integer model, positives)"""
    assert 0 <= r_star < R
    phi, allowed, plants = _exact_plants(K, r_star)
    # (the planted documents stand at the even places, so their ids are doc_ids(2 n)[2 j] as the plants assumed)
    docs = [[V_RANDOM + 2 * j, V_RANDOM + 2 * j + 1] for j in range(len(plants))]
    c = _assemble(K, docs, allowed, phi, np.random.default_rng([32, K]))
    assert (c["where"] == 2 * np.arange(len(plants))).all()
    count = {}
    for p in plants:
        key = (p["kind"], p["cls"]) + ((p["masked"],) if p["kind"] == "zero_lane" else ())
        count[key] = count.get(key, 0) + 1
    for kind in kinds_of(K):                                           # no requested plant was skipped
        for cls in CLASSES:
            for key in ([(kind, cls, False), (kind, cls, True)] if kind == "zero_lane" else [(kind, cls)]):
                assert count.get(key, 0) >= 3, key
    if K > 64:                                                         # ties that tell the lane-major order from the topic-major one
        for kind in kinds_of(K):
            assert any(p["kind"] == kind and p["cls"] == "tie" and p["z0_topic_major"] != p["z0"] for p in plants), kind
    return dict(c, alpha=ALPHA_EXACT, R=R, r_star=r_star, plants=plants, count=count)


def decode_z0(c, mant, expo, trace_z):
    """the z_0 of particle r_star that the outputs (mant, expo) of the planted documents name, by trying every positive topic of the
    planted row (the other particles' z_0 from trace_z, a restatement's) -> list of lists of topics, one list per plant"""
    K, R, alpha = c["K"], c["R"], c["alpha"]
    phi1 = (np.arange(K) + 1.0) / (2 * K)
    out = []
    for j, p in enumerate(c["plants"]):
        d = int(c["where"][j])
        on = c["allowed"][d] != 0
        A = float(on.sum())
        p0 = 0.0
        for _ in range(R):
            p0 = p0 + 1.0 / (0.0 + A * alpha)
        p0 = p0 / float(R)
        names = []
        for k in p["positives"]:
            z = [int(t) for t in trace_z[d, :, 0]]
            z[c["r_star"]] = k
            tot = 0.0
            for r in range(R):
                cnt = np.zeros(K)
                cnt[z[r]] = 1.0
                x = np.where(on, (cnt + alpha) * phi1, 0.0)
                tot = tot + float(ref.sum64(x[None, :])[0]) / (1.0 + A * alpha)
            acc = pair_mul(0.5, 1, *math.frexp(p0))
            acc = pair_mul(acc[0], acc[1], *math.frexp(tot / float(R)))
            if acc == (float(mant[d]), int(expo[d])):
                names.append(k)
        out.append(names)
    return out


# ------------------------------------------------------------------------------------------------
# tuned_case
# ------------------------------------------------------------------------------------------------
def draw_parts(x, u):
    """draw64's own q (NI, 64) and t_j (64,) for one weight vector"""
    x = np.asarray(x, dtype=np.float64)
    NI = ref.slots(len(x))
    g = ref._grid(x[None, :], NI)[0]
    q = np.cumsum(g, axis=0)
    X = q[-1].copy()
    d = 1
    while d < 64:
        Y = X.copy()
        Y[d:] = X[:-d] + X[d:]
        X = Y
        d *= 2
    return q, u * X[63] - np.concatenate([[0.0], X[:-1]])


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.int64)


def _floats(b):
    return np.asarray(b, dtype=np.int64).view(np.float64)


@functools.lru_cache(maxsize=None)
def _tuned_plants(K, r_star):
    order = lane_major(K)
    rank = np.empty(K, dtype=np.int64)
    rank[order] = np.arange(K)
    kinds = kinds_of(K)
    rng = np.random.default_rng([33, K, r_star])
    phi_r = random_loadings(np.random.default_rng([32, K]), K)          # (the random words of _assemble, same generator)
    n = N_TUNED
    ids = doc_ids(2 * n)[::2]
    lens = rng.integers(4, 11, size=n)
    docs = [rng.integers(0, V_RANDOM, size=int(N)).tolist() for N in lens]
    rows = np.zeros((n, K))
    k_at, k_next, us = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    pats = []
    for j in range(n):
        docs[j][-2] = V_RANDOM + j
        ranks, ib = _pattern(K, kinds[j % len(kinds)], rng)
        pats.append((ranks, ib))
        rows[j, [order[r] for r in ranks]] = rng.random(len(ranks)) ** 3 + 0.01
        k_at[j], k_next[j] = order[ranks[ib]], order[ranks[ib + 1]]
        us[j] = uniform(int(lens[j]) - 1, STREAM + r_star, int(ids[j]), int(lens[j]) - 2)
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = np.array([w for t in docs for w in t], dtype=np.int64)
    at = np.arange(n), 0, lens - 2

    def run(rows_now):
        tr = {}
        ref.left_to_right_ref(np.vstack([phi_r, rows_now]), doc_off, word, ALPHA, 1, SEED, STREAM + r_star, K=K, doc_ids=ids, trace=tr)
        return tr["z"]

    def counts(z, j):
        c = np.zeros(K)
        for t in z[j, 0, :lens[j] - 2]:
            if t >= 0:
                c[t] += 1.0
        return c

    # shape: the weight in front of the boundary u / 2 of the total, the boundary's u / 2 (u if it is the first), the rest 1 - u --
    # under the counts that the restatement reaches (which may move once with the row: two rounds)
    for _ in range(2):
        z = run(rows)
        for j in range(n):
            ranks, ib = pats[j]
            wgt = counts(z, j) + ALPHA
            ks = [order[r] for r in ranks]
            front, back = ks[:ib], ks[ib + 1:]
            u = us[j]
            if front:
                rows[j, front] *= (u / 2) / float(np.sum(rows[j, front] * wgt[front]))
            rows[j, ks[ib]] = (u / 2 if front else u) / wgt[ks[ib]]
            rows[j, back] *= (1 - u) / float(np.sum(rows[j, back] * wgt[back]))
    cols = k_at
    base = rows[np.arange(n), cols].copy()
    lo, hi = _bits(base / 8.0).copy(), _bits(base * 8.0).copy()

    def above(bits):
        r = rows.copy()
        r[np.arange(n), cols] = _floats(bits)
        return rank[np.maximum(run(r)[at], 0)] <= rank[k_at]
    ok = (us > 1e-3) & (us < 1 - 1e-3) & ~above(lo) & above(hi)
    while ((hi - lo)[ok] > 1).any():
        mid = lo + (hi - lo) // 2
        up = above(mid)
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    # the check at the end: adjacent doubles, and the topic flips between them from the next positive position to the boundary
    r_lo, r_hi = rows.copy(), rows.copy()
    r_lo[np.arange(n), cols], r_hi[np.arange(n), cols] = _floats(lo), _floats(hi)
    z_lo, z_hi = run(r_lo), run(r_hi)
    ok &= (hi - lo == 1) & (z_lo[at] == k_next) & (z_hi[at] == k_at)
    upper = np.arange(n) % 2 == 0
    rows[np.arange(n), cols] = np.where(upper, _floats(hi), _floats(lo))
    z = run(rows)
    facts = []
    for j in range(n):
        if not ok[j]:
            rows[j, cols[j]] = base[j]                                  # (not a plant: an ordinary document)
            continue
        # draw64's own arithmetic at the lower double: is q == t_j exactly at the boundary (the strict `>` alone decides)?
        x = (counts(z_lo, j) + ALPHA) * r_lo[j]
        q, tg = draw_parts(x, us[j])
        assert int(ref.draw64(x[None, :], np.array([us[j]]))[0]) == k_next[j]
        facts.append(dict(doc=j, kind=kinds[j % len(kinds)], upper=bool(upper[j]), topic=int(z[j, 0, lens[j] - 2]), k_at=int(k_at[j]),
                          k_next=int(k_next[j]), equal=bool(q[k_at[j] // 64, k_at[j] % 64] == tg[k_at[j] % 64])))
        assert facts[-1]["topic"] == (k_at[j] if upper[j] else k_next[j])
    assert len(facts) >= 16, "only %d of %d tuned plants were made at K = %d" % (len(facts), n, K)
    return docs, rows, facts


@functools.lru_cache(maxsize=None)
def tuned_case(K, R, r_star=0):
    """-> dict: the case, where[j] the document of candidate j, plants = the facts of those that were planted (doc = j, kind, upper,
    topic = the final z of position N - 2 in particle r_star, equal: q == t_j exactly at the lower double)"""
    assert 0 <= r_star < R
    docs, rows, facts = _tuned_plants(K, r_star)
    c = _assemble(K, docs, np.ones((len(docs), K), dtype=np.uint8), rows, np.random.default_rng([32, K]))
    return dict(c, alpha=ALPHA, R=R, r_star=r_star, plants=facts, n_equal=sum(f["equal"] for f in facts))


# ------------------------------------------------------------------------------------------------
# scaled_case
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scaled_case(K, scale):
    """documents of 6 .. 12 tokens over 20 words.  The words load on 12 topics (K = 9: 6) out of a pool of 24 that every document is
    allowed and nothing else (with A = K = 1024 the division by n + A alpha alone would take every subnormal p_n to zero).  The base
    rows hold small integers (sum 200 .. 380, two of them 1) and two entries of 2^-21, times 2^e: at sub1066 one unit of the base is
    one step of the subnormal grid (5e-324), at sub1045 the entries of 2^-21 are.  alpha * 5e-324 rounds to +0.0, (1 + alpha) * 5e-324
    does not."""
    rng = np.random.default_rng([34, K])
    V, D = 20, 24
    pool = np.sort(rng.choice(K, size=min(K, 24), replace=False))
    base = np.zeros((V, K))
    for w in range(V):
        ks = rng.choice(pool, size=min(2 * K // 3, 12), replace=False)
        vals = rng.integers(1, 16, size=len(ks)).astype(np.float64)
        vals[:2] = 1.0
        vals[2:4] = 0.0
        vals[-1] += float(rng.integers(200, 380)) - vals.sum()
        vals[2:4] = 2.0 ** -21
        base[w, ks] = vals
    E = SCALES[scale]
    lead = (ALPHA if scale == "top" else ALPHA + 1.0) * base.sum(axis=1)
    e = E - np.floor(np.log2(lead)).astype(np.int64)
    with np.errstate(under="ignore"):
        phi = np.ldexp(base, e[:, None])
    lens = rng.integers(6, 13, size=D)
    docs = [rng.integers(0, V, size=int(N)).tolist() for N in lens]
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    allowed = np.zeros((D, K), dtype=np.uint8)
    allowed[:, pool] = 1
    c = dict(K=K, phi_t=phi, doc_off=doc_off, word=np.array([w for t in docs for w in t], dtype=np.int64), allowed=allowed,
             doc_ids=doc_ids(D), alpha=ALPHA, R=SCALED_R, scale=scale)
    if scale.startswith("sub"):
        tiny = phi[np.unique(c["word"])]
        with np.errstate(under="ignore"):
            c["n_flushed"] = int(((tiny > 0) & (ALPHA * tiny == 0.0) & ((1.0 + ALPHA) * tiny > 0.0)).sum())
        assert c["n_flushed"] > 0
    return c


# ------------------------------------------------------------------------------------------------
# overflow_case
# ------------------------------------------------------------------------------------------------
def overflow_pairs(K):
    """(k1, k2, what): word A is one-hot on k1.  Neither topic is the last position in lane-major order."""
    NI = ref.slots(K)
    pairs = [(3, 4, "adjacent lanes"), (4, 3, "adjacent lanes, the other order"), (2, 9, "k2 followed by zero lanes only"),
             (9, 2, "k1 followed by zero lanes only")]
    if NI > 1:
        pairs += [(5, 69, "one lane, two slots"), (69, 5, "one lane, two slots, the other order"),
                  (63, 70, "lane 63 against a higher slot of a lower lane"), (70, 63, "the same, the other order")]
    last = lane_major(K)[-1]
    assert all(k1 < K and k2 < K and last not in (k1, k2) for k1, k2, _ in pairs)
    return pairs


@functools.lru_cache(maxsize=None)
def overflow_case(K):
    """one document B B A A A B X X per pair, two particles -> dict: the case, pairs, no_hit[i] = the draws of document i that had a
    positive weight and no hit, last[i] = the lane-major last of (k1, k2)"""
    pairs = overflow_pairs(K)
    rank = np.empty(K, dtype=np.int64)
    rank[lane_major(K)] = np.arange(K)
    phi = np.zeros((3 * len(pairs), K))
    docs = []
    for i, (k1, k2, _) in enumerate(pairs):
        B, A, X = 3 * i, 3 * i + 1, 3 * i + 2
        phi[B, [k1, k2]] = 0.9 * 2.0 ** 1023
        phi[A, k1] = 0.5
        phi[X] = (np.arange(K) + 1.0) / (2 * K)
        docs.append([B, B, A, A, A, B, X, X])
    doc_off = 8 * np.arange(len(pairs) + 1, dtype=np.int64)
    c = dict(K=K, phi_t=phi, doc_off=doc_off, word=np.array(sum(docs, []), dtype=np.int64), allowed=None, doc_ids=doc_ids(len(pairs)),
             alpha=ALPHA, R=2, pairs=pairs, last=[k1 if rank[k1] > rank[k2] else k2 for k1, k2, _ in pairs], no_hit=[])
    for i in range(len(pairs)):
        stats, tr = {}, {}
        with np.errstate(all="ignore"):
            ref.left_to_right_ref(phi, doc_off[i:i + 2] - doc_off[i], docs[i], ALPHA, 2, SEED, STREAM, doc_ids=c["doc_ids"][i:i + 1],
                                  stats=stats, trace=tr)
        assert stats["no_hit"] > 0, pairs[i]
        assert (tr["z"][0, :, 0] == c["last"][i]).all(), pairs[i]
        c["no_hit"].append(stats["no_hit"])
    return c
