"""Adversarial inputs for llda_foldin: last-bit ties of the keyed draw, sites just outside the decided tier's band, and loadings at the
edges of the double range (test infrastructure, host only: numpy + oracle/ + tests/foldinref.py).

The narrow fold-in kernel (csrc/kernel_foldin.hpp) decides almost every site from fp64 prefix sums of the UNNORMALISED scores
(n_dk + alpha) * ph[:, v], the threshold u * total and a band of total * 2^-40; a site with a prefix inside the band takes the reference's
pipeline (numpy-ordered sum, division, `while prob.sum() > 1`, keyed draw).  On random data a 53-bit uniform never comes within 2^-40 of
a prefix, so nothing random exercises the hand-over, the strict `>` of the draw, or a wavefront in which some lane groups are decided
and others are not.  This module plants such sites:

  * a planted document has ONE planted site in sweep 0 (the only sweep whose incoming state does not depend on the word's own row of
    ph); the site's word occurs nowhere else, so its row of ph is free.  The row is shaped so that a chosen prefix boundary (KINDS)
    sits at u * total -- a coarse scale of the entries up to the boundary, then bisection on the boundary's own entry with the
    REFERENCE's pipeline as the oracle, down to two adjacent doubles between which the reference's topic flips ("tie": the upper double
    in half of the sites, the lower in the other half), or moved away again until the modelled gap is 2^-38 .. 2^-36 of the total
    ("outside", both signs: 4 .. 16 times the band, so roundings of 2^-47 cannot carry it across -- the tier must decide it, and right);
  * in even wavefronts of a narrow launch only every second document is planted, all at one site index (decided and handed-over lane
    groups meet in one loop iteration), in odd wavefronts every document; the other sites are random;
  * ``init_case``: the planted site's own row of init_rows instead, tuned on the row the reference draws from after its
    `while prob.sum() > 1: prob /= c_init` (ROW_KINDS: no step, one step, the ~525 steps the narrow kernels jump over);
  * ``scaled_case``: every row of ph times an exact power of two, so that the site totals land at the SCALES.

``tier_model`` is the decided tier restated in numpy in the kernel's association order (per-lane sequential prefix in lane-major
order, Hillis-Steele scan of the lane totals, tg -+ total * margin, the positive mask); ``walk`` follows the reference site by site,
plants where told to, and records the model's verdict for every site of every sweep.  The arguments keep the conventions of
tests/test_gpu_foldin_direct.make_case, so its ``device`` and ``reference`` take these cases unchanged.
"""
import functools

import numpy as np

import llda_oracle as orc
from test_gpu_foldin_direct import C_INIT, SEED, SETTINGS, STREAM, make_init_rows

KINDS = ("lane0_first", "lane_end", "zero_lane", "before_last")
#   lane0_first : the first positive position of lane 0 (nothing in front of it: tg = u * total itself)
#   lane_end    : the last slot of a lane, the next positive score in the next lane (prefix = a lane total = a scan value)
#   zero_lane   : exact zeros from the boundary through the whole next lane: the next positive position is two lanes on
#   before_last : the boundary in front of the last positive position (behind it: one score, the "no hit -> last positive" rule)
CLASSES = ("tie_upper", "tie_lower", "outside_plus", "outside_minus")
ROW_KINDS = ("no_step", "one_step", "jump")       # sum 0.9 / 1 + a few ulp / 1.3 (c_init = 1.0005: 525 steps, jumped by the narrow kernels)
WHERE = ("first", "last", "middle")
V_RANDOM = 40
MARGIN = 2.0 ** -40
FLOOR = 2.0 ** -960                               # the decided tier's floor on the total (csrc/kernel_foldin.hpp)
OUT_LO, OUT_HI = 2.0 ** -38, 2.0 ** -36
ITERS, THINNING = 3, 1
N_INIT_PLANTED = 24                               # KINDS x ROW_KINDS x both sides, once each (a jump row costs the host 525 sums per try)
# name -> exponent the totals are put at ("top": every total above 1e300 = 2^996.6 and every sum finite)
SCALES = {"sub1066": -1066, "sub1045": -1045, "tiny1000": -1000, "tiny960": -960, "big960": 960, "top": 998}


def _sum(prob):
    return np.sum(np.ascontiguousarray(prob, dtype=np.float64))


# ------------------------------------------------------------------------------------------------
# the decided tier, restated
# ------------------------------------------------------------------------------------------------
def _scan(x):
    x = x.copy()
    d = 1
    while d < x.shape[0]:
        y = x.copy()
        y[d:] = x[:-d] + x[d:]
        x = y
        d *= 2
    return x


def tier_model(lay, w, u, margin=MARGIN, floor=0.0, fp32=False):
    """llda_foldin_kernel's decided tier on the scores w (topic order) -> (sure, topic or -1, gap, total): gap = distance of the
    nearest per-lane prefix to its threshold, relative to the total (signed gap of one position: ``signed_gap``).  floor = 0 is the
    tier without a floor on the total; fp32 rounds the scores to float first (a tier that is too coarse)."""
    g = lay.grid(np.asarray(w, dtype=np.float64))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if fp32:
            g = g.astype(np.float32).astype(np.float64)
        q = np.cumsum(g, axis=1)
        X = _scan(q[:, -1])
        tot = X[-1]
        tg = u * tot - np.concatenate(([0.0], X[:-1]))
        m = tot * margin
        cnt_lo = (q <= (tg - m)[:, None]).sum(axis=1)
        cnt_hi = (q <= (tg + m)[:, None]).sum(axis=1)
        gap = float(np.min(np.abs(q - tg[:, None])) / tot) if tot > 0 and np.isfinite(tot) else 0.0
    fm = (g > 0) & (np.arange(lay.T)[None, :] >= cnt_lo[:, None])
    unsure = bool((cnt_lo != cnt_hi).any()) or not tot > 0.0 or not m < tot or not tot < 1.0e300 or not tot >= floor
    if unsure or not fm.any():
        return False, -1, gap, float(tot)
    return True, int(lay.slot_topic[int(np.argmax(fm.ravel()))]), gap, float(tot)


def signed_gap(lay, w, u, topic):
    """(prefix at the topic's position - its lane's threshold) / total, in the tier's arithmetic"""
    q = np.cumsum(lay.grid(np.asarray(w, dtype=np.float64)), axis=1)
    X = _scan(q[:, -1])
    g, s = divmod(int(lay.topic_slot[topic]), lay.T)
    return float((q[g, s] - (u * X[-1] - (X[g - 1] if g else 0.0))) / X[-1])


# ------------------------------------------------------------------------------------------------
# the reference's pipeline for one site
# ------------------------------------------------------------------------------------------------
def ref_site(lay, num_a, b, u, c_loop, beta_fallback, beta):
    """foldinref's statements for one site of a sweep -> (topic, prob the draw saw); raises FloatingPointError as it does"""
    prob = num_a * b
    S = _sum(prob)
    if beta_fallback and S == 0.0:
        prob = num_a * (b + beta)
        S = _sum(prob)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        prob = prob / S
    while _sum(prob) > 1:
        prob /= c_loop
    return orc.draw_keyed(prob, u, lay), prob


def ref_init(lay, row, u, c_init):
    prob = row.copy()
    steps = 0
    while _sum(prob) > 1:
        prob /= c_init
        steps += 1
    return orc.draw_keyed(prob, u, lay), prob, steps


def draw_equal_at(lay, prob, u, topic):
    """draw_keyed's own arithmetic: is q == t - X[g-1] exactly at the topic's position (the strict `>` alone decides)?"""
    q = np.cumsum(lay.grid(prob), axis=1)
    x = _scan(q[:, -1])
    g, s = divmod(int(lay.topic_slot[topic]), lay.T)
    return bool(q[g, s] == u * x[-1] - (x[g - 1] if g else 0.0))


# ------------------------------------------------------------------------------------------------
# planting
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lane_major(K):
    """topics in draw order (lane-major), the lane of each, and every topic's rank in that order"""
    lay = orc.layout(K)
    pos = np.flatnonzero(lay.slot_topic >= 0)
    topics = lay.slot_topic[pos].astype(np.int64)
    rank = np.empty(K, dtype=np.int64)
    rank[topics] = np.arange(K)
    return topics, pos // lay.T, rank


def _pattern(K, kind, rng):
    """-> (positive[K] in draw order, rank of the boundary, rank of the next positive position)"""
    _, lane, _ = _lane_major(K)
    lanes = np.unique(lane)
    pos = rng.random(K) > 0.3
    of = lambda g: np.flatnonzero(lane == lanes[g])
    if kind == "lane0_first":
        r = of(0)
        i = r[1] if len(r) > 1 and rng.random() < 0.5 else r[0]
        pos[r[0]:i] = False
        pos[K - 1] = True
    elif kind == "lane_end":
        g = int(rng.integers(0, len(lanes) - 1))
        i = of(g)[-1]
        pos[of(g + 1)[0]] = True
    elif kind == "zero_lane":
        g = int(rng.integers(0, len(lanes) - 2))
        i = int(rng.choice(of(g)))
        pos[i + 1:of(g + 1)[-1] + 1] = False
        pos[of(g + 2)[0]] = True
    else:
        pos[[0, K - 1]] = True
        i = np.flatnonzero(pos)[-2]
    pos[i] = True
    nxt = i + 1 + int(np.argmax(pos[i + 1:]))
    assert pos[nxt]
    return pos, int(i), nxt


def _bisect(x0, above):
    """adjacent doubles lo < hi around x0 with above(lo) False and above(hi) True"""
    lo = hi = float(x0)
    for _ in range(80):
        if not above(lo):
            break
        lo *= 0.5
    for _ in range(80):
        if above(hi):
            break
        hi *= 2.0
    assert not above(lo) and above(hi)
    a, b = (int(np.float64(v).view(np.int64)) for v in (lo, hi))
    while b - a > 1:
        mid = (a + b) // 2
        if above(float(np.int64(mid).view(np.float64))):
            b = mid
        else:
            a = mid
    return float(np.int64(a).view(np.float64)), float(np.int64(b).view(np.float64))


def _shape(K, kind, rng, weight, u):
    """a row in topic order whose prefix up to the boundary is the fraction u of the weighted total, roughly"""
    topics, _, _ = _lane_major(K)
    pos, i, nxt = _pattern(K, kind, rng)
    v = (rng.random(K) ** 3 + 0.01) * pos
    A, B = float(np.sum(v[:i + 1] * weight[topics[:i + 1]])), float(np.sum(v[i + 1:] * weight[topics[i + 1:]]))
    v[:i + 1] *= u * B / ((1.0 - u) * A)
    row = np.zeros(K)
    row[topics] = v
    return row, int(topics[i]), int(topics[nxt])


def plant_ph(lay, num_a, u, kind, cls, rng, p):
    """the planted word's column of ph -> (column, facts)"""
    K = lay.K
    _, _, rank = _lane_major(K)
    assert 1e-6 < u < 1 - 1e-6
    b, k_at, k_next = _shape(K, kind, rng, num_a, u)

    def topic(x):
        b[k_at] = x
        return ref_site(lay, num_a, b, u, p["c_loop"], p["beta_fallback"], p["beta"])[0]
    lo, hi = _bisect(b[k_at], lambda x: rank[topic(x)] <= rank[k_at])
    assert topic(lo) == k_next and topic(hi) == k_at, "the flip is not between the boundary and the next positive position"
    b[k_at] = lo
    equal = draw_equal_at(lay, ref_site(lay, num_a, b, u, p["c_loop"], p["beta_fallback"], p["beta"])[1], u, k_at)
    if cls.startswith("tie"):
        b[k_at] = hi if cls == "tie_upper" else lo
    else:
        want = 2.0 ** -37 * (1 if cls == "outside_plus" else -1)
        x = hi
        for _ in range(6):
            b[k_at] = x
            w = num_a * b
            g = signed_gap(lay, w, u, k_at)
            if OUT_LO * 1.3 < abs(g) < OUT_HI / 1.3 and g * want > 0:
                break
            x *= 1.0 + (want - g) / (w[k_at] / _sum(w) * (1.0 - u))
        b[k_at] = x
    w = num_a * b
    t = topic(b[k_at])
    assert t == (k_at if cls in ("tie_upper", "outside_plus") else k_next)
    return b.copy(), dict(kind=kind, cls=cls, topic=t, k_at=k_at, k_next=k_next, equal=equal, sgap=signed_gap(lay, w, u, k_at))


def plant_row(lay, u, kind, row_kind, upper, rng, c_init):
    """the planted site's own row of init_rows -> (row, facts)"""
    K = lay.K
    _, _, rank = _lane_major(K)
    assert 1e-6 < u < 1 - 1e-6
    row, k_at, k_next = _shape(K, kind, rng, np.ones(K), u)
    row /= _sum(row)
    if row_kind == "one_step":
        while not _sum(row) >= 1 + 8 * 2.0 ** -52:
            row *= 1 + 2.0 ** -52
    else:
        row *= 0.9 if row_kind == "no_step" else 1.3

    def topic(x):
        row[k_at] = x
        return ref_init(lay, row, u, c_init)[0]
    lo, hi = _bisect(row[k_at], lambda x: rank[topic(x)] <= rank[k_at])
    assert topic(lo) == k_next and topic(hi) == k_at
    row[k_at] = lo
    equal = draw_equal_at(lay, ref_init(lay, row, u, c_init)[1], u, k_at)
    row[k_at] = hi if upper else lo
    t, _, steps = ref_init(lay, row, u, c_init)
    s = float(_sum(row))
    assert (s <= 1 and steps == 0) if row_kind == "no_step" else (1 < s < 1 + 1e-13 and steps == 1) if row_kind == "one_step" else \
        (s > 1 + 128 * (c_init - 1) and steps > 400)
    return row.copy(), dict(kind=kind, row_kind=row_kind, upper=bool(upper), topic=t, equal=equal, steps=steps)


# ------------------------------------------------------------------------------------------------
# the corpus and the walk
# ------------------------------------------------------------------------------------------------
def make_corpus(K):
    """-> dict(doc_off, word, freq, init_idx, plan): plan[(d, n)] = index of the planted site (its word is V_RANDOM + index).
    4 * 256 / G documents (four workgroups of a narrow launch, every wavefront full), 32 at least: every boundary kind needs a tie of
    either side and a just-outside site of either sign; lengths 3 .. 12, frequencies 1 .. 4."""
    lay = orc.layout(K)
    per_wave = max(64 // lay.G, 1)                      # documents of one wavefront (a wide launch: one document each)
    D = max(4 * 256 // lay.G, 32)
    rng = np.random.default_rng([21, K])
    lens = rng.integers(3, 13, D)
    plan = {}
    for d in range(D):
        wave, i = divmod(d, per_wave)
        if wave % 2 == 0:
            lens[d] = 3 + (5 * wave) % 10               # one length per even wavefront: "last" is one site index as well
            if (i + wave // 2) % 2:
                continue
            where = WHERE[(wave // 2) % 3]
        else:
            where = WHERE[len(plan) % 3]
        plan[(d, {"first": 0, "last": int(lens[d]) - 1, "middle": int(lens[d]) // 2}[where])] = len(plan)
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(0, V_RANDOM, S).astype(np.int32)
    for (d, n), j in plan.items():
        word[doc_off[d] + n] = V_RANDOM + j
    return dict(doc_off=doc_off, word=word, freq=rng.integers(1, 5, S).astype(np.int32), init_idx=rng.integers(0, 12, S).astype(np.int32),
                plan=plan)


def make_loadings(K, n_planted):
    """(K, V_RANDOM + n_planted): the random words as in the direct test (wide dynamic range, half exact zeros, every word loads on
    some topic); the planted words' columns are filled in by the walk"""
    rng = np.random.default_rng([22, K])
    ph = rng.random((K, V_RANDOM)) ** 12
    ph[rng.random((K, V_RANDOM)) < 0.5] = 0.0
    v = np.arange(V_RANDOM)
    ph[v % K, v] += rng.random(V_RANDOM) ** 12 + 1e-30
    return np.hstack([ph, np.zeros((K, n_planted))])


def walk(c, plant=None, floor=0.0, models="all"):
    """foldinref.fold_in's statements, document by document, with hooks -> dict(z, n_dk, th, raises, sites): sites = one record per
    site of every sweep >= 0 (doc, n, sweep, ref topic, total, gap and the model's verdicts: sure / model at the 2^-40 margin, sure0 /
    model0 at margin 0, sure32 / model32 with fp32 scores; models = "tier": the first pair only, None: no records), planted = the planted
    sites' facts.

    plant = "ph": the sites of c["plan"] get their word's column of c["phs"][0] when sweep 0 reaches them; "rows": they get a row of
    c["rows"] of their own when prep4test reaches them (c["init_idx"] points at it).  Both write into c."""
    K = c["K"]
    lay = orc.layout(K)
    ph, rows = c["phs"][0], c["rows"]
    doc_off, word, freq, init_idx = c["doc_off"], c["word"], c["freq"], c["init_idx"]
    D = len(doc_off) - 1
    z = np.zeros(int(doc_off[-1]), dtype=np.int64)
    n_dk_all = np.zeros((D, K), dtype=np.int64)
    th = np.zeros((D, K))
    raises = np.zeros(D, dtype=bool)
    sites, planted = [], []
    n_rows0 = rows.shape[0] - N_INIT_PLANTED                         # (plant = "rows": the planted rows follow the random ones)
    for d in range(D):
        s0, s1 = int(doc_off[d]), int(doc_off[d + 1])
        doc = (c["doc_base"] + d) & 0xFFFFFFFF
        n_dk = n_dk_all[d]
        try:
            for n in range(s1 - s0):
                u = float(orc.keyed_uniform(c["seed"], orc.SWEEP_INIT, c["stream_id"], doc, n))
                j = c["plan"].get((d, n))
                if plant == "rows" and j is not None and j < N_INIT_PLANTED:
                    rng = np.random.default_rng([23, K, j])
                    rows[n_rows0 + j], f = plant_row(lay, u, KINDS[j % 4], ROW_KINDS[(j // 4) % 3], j < N_INIT_PLANTED // 2, rng, c["c_init"])
                    init_idx[s0 + n] = n_rows0 + j
                    planted.append(dict(f, doc=d, n=n))
                z[s0 + n] = ref_init(lay, rows[int(init_idx[s0 + n])], u, c["c_init"])[0]
                n_dk[z[s0 + n]] += int(freq[s0 + n])
            avg = np.zeros(K)
            for i in range(c["iters"]):
                for n in range(s1 - s0):
                    v, f = int(word[s0 + n]), int(freq[s0 + n])
                    n_dk[z[s0 + n]] -= f
                    num_a = n_dk + c["alpha"]
                    u = float(orc.keyed_uniform(c["seed"], i, c["stream_id"], doc, n))
                    j = c["plan"].get((d, n)) if i == 0 else None
                    if plant == "ph" and j is not None:
                        rng = np.random.default_rng([24, K, j])
                        ph[:, v], fact = plant_ph(lay, num_a, u, KINDS[j % 4], CLASSES[(j // 4) % 4], rng, c)
                        planted.append(dict(fact, doc=d, n=n, index=len(sites)))
                    try:
                        new_z = ref_site(lay, num_a, ph[:, v], u, c["c_loop"], c["beta_fallback"], c["beta"])[0]
                    except FloatingPointError:
                        n_dk[z[s0 + n]] += f
                        raise
                    if models:
                        w = num_a * ph[:, v]
                        if c["beta_fallback"] and _sum(w) == 0.0:
                            w = num_a * (ph[:, v] + c["beta"])
                        sure, t, gap, tot = tier_model(lay, w, u, floor=floor)
                        rec = dict(doc=d, n=n, sweep=i, ref=new_z, sure=sure, model=t, gap=gap, total=tot, planted=j is not None and plant == "ph")
                        if models == "all":
                            rec["sure0"], rec["model0"] = tier_model(lay, w, u, margin=0.0, floor=floor)[:2]
                            rec["sure32"], rec["model32"] = tier_model(lay, w, u, floor=floor, fp32=True)[:2]
                        sites.append(rec)
                    z[s0 + n] = new_z
                    n_dk[new_z] += f
                if (i + 1) % c["thinning"] == 0:
                    s2 = (i + 1) // c["thinning"]
                    cur = n_dk / n_dk.sum()
                    if s2 == 1:
                        avg = cur
                    elif c["avg_mode"] == 0:
                        old = (s2 - 1) / s2 * avg
                        new = (1 / s2) * cur
                        avg = old + new
                    else:
                        m = (s2 - 1) / s2
                        old = m * avg
                        new = (1 - m) * cur
                        avg = old + new
            th[d] = avg
        except FloatingPointError:
            raises[d] = True
    return dict(z=z, n_dk=n_dk_all, th=th, raises=raises, sites=sites, planted=planted)


def _base(K, setting):
    corpus = make_corpus(K)
    c = dict(K=K, phs=[make_loadings(K, len(corpus["plan"]))], ph_sel=None, rows=make_init_rows(K), doc_ids=None, doc_base=1000,
             doc_stream=None, stream_id=STREAM, c_init=C_INIT, iters=ITERS, thinning=THINNING, seed=SEED, **SETTINGS[setting])
    c.update(corpus)
    return c


@functools.lru_cache(maxsize=None)
def tie_case(K, setting):
    """-> (case, walk): planted columns of ph.  No ties for the fall-back scores (n_dk + alpha) * beta themselves: they hold nothing to tune."""
    c = _base(K, setting)
    return c, walk(c, plant="ph")


@functools.lru_cache(maxsize=None)
def init_case(K, setting):
    """-> (case, walk): random ph (the planted words get random columns), planted rows of init_rows"""
    c = _base(K, setting)
    rng = np.random.default_rng([25, K])
    c["phs"][0][:, V_RANDOM:] = rng.random((K, len(c["plan"]))) ** 6
    c["rows"] = np.vstack([c["rows"], np.zeros((N_INIT_PLANTED, K))])
    return c, walk(c, plant="rows", models=None)


@functools.lru_cache(maxsize=None)
def scaled_case(K, setting, scale):
    """the tie case with every row of ph times an exact power of two.  A site's total is at least alpha * sum(row) and at most
    (alpha + 48) * sum(row); "top" puts the lower end at 2^998 (> 1e300, every sum below 2^1008), the others put (alpha + 1) * sum(row)
    at the scale's exponent."""
    c0, _ = tie_case(K, setting)
    ph = c0["phs"][0]
    base = (c0["alpha"] if scale == "top" else c0["alpha"] + 1.0) * ph.sum(axis=0)
    e = SCALES[scale] - np.floor(np.log2(base)).astype(np.int64)
    # sub1066 at K in the thousands: every product of a site would underflow to zero and the reference raise in EVERY document.  All
    # words but every sixteenth are lifted until their largest product is 8 steps of the subnormal grid at least (totals stay subnormal);
    # the others keep some raising documents in the cases, for bit 0 of status
    lift = -1071 - np.floor(np.log2(c0["alpha"] * ph.max(axis=0))).astype(np.int64)
    e = np.where(np.arange(ph.shape[1]) % 16 != 0, np.maximum(e, lift), e)
    with np.errstate(under="ignore"):
        return dict(c0, phs=[np.ldexp(ph, e[None, :])])


def scaled_walk(K, setting, scale, floor):
    """the reference and the tier's verdicts (with the given floor on the total) on a scaled case"""
    return walk(scaled_case(K, setting, scale), floor=floor, models="tier")


def facts(K, setting):
    """what the tests assert about the tie case"""
    c, w = tie_case(K, setting)
    pl, sites = w["planted"], w["sites"]
    count = {}
    for f in pl:
        count[(f["kind"], f["cls"])] = count.get((f["kind"], f["cls"]), 0) + 1
    ties = [f for f in pl if f["cls"].startswith("tie")]
    return dict(n_planted=len(pl), count=count, n_equal=sum(f["equal"] for f in ties), n_equal_lower=sum(f["equal"] for f in ties if f["cls"] == "tie_lower"),
                max_tie_gap=max(sites[f["index"]]["gap"] for f in ties),
                min_random_gap=min(s["gap"] for s in sites if not s["planted"]),
                outside_gaps=[sites[f["index"]]["gap"] for f in pl if not f["cls"].startswith("tie")])
