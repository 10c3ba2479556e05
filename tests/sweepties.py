"""Adversarial inputs for the sweep kernels' fp64 tier and exact tier: last-bit ties of the keyed draw and sites just outside tier 1's
band (test infrastructure, host only: numpy + oracle/ + tests/neartie.py).

tests/neartie.py pins tier 0: thresholds 2^-24 .. 2^-28 of the total away from a prefix boundary.  That is 2^10 and more away from
where the two tiers behind it can differ from the reference: tier 1 (unnormalised fp64, margin 2^-40, error 254 * 2^-53)
and the exact pipeline (numpy's pairwise sum, the division, per-lane prefix, Hillis-Steele scan, the strict `>`).  A sweep's scores are
lab * (n_dk + alpha) * (n_kw + beta) / (n_k + V beta) with integer counts, so a tie cannot be bisected as the fold-in's real-valued
loadings are (tests/foldinties.py).  Here the LAST site of a planted document gets its own word (V = S), whose column of n_k_v is free:

  * a boundary b of the wanted kind (KINDS, stated for the group layout of oracle/llda_oracle.py) is chosen among the positions the
    document's labels allow, the random heavy-tailed column is scaled so that u * total falls near the prefix at b, and a greedy pass
    over single entries takes the distance down to a few scores;
  * E - g * total (E = prefix at b - u * total, g = 0 for a tie, +-2^-37 for a site just outside the band) is LINEAR in the counts: raising
    x_j by k changes it by k (1 - u - g) c_j for a topic up to the boundary and by -k (u + g) c_j behind it, c_j = (n_dk_j + alpha) /
    (n_k_j + V beta).  Five entries are tuned at once: four run over windows of N whole counts each, two against two (meet in the
    middle: sort one side's N^2 sums modulo |d_1|, look the other side's up), the fifth is solved by rounding.  N^4 = 2^32 .. 2^40
    candidates bring the residual to 2^-50 .. 2^-60 of the total.  The search runs on 64-bit fixed-point fractions of |d_1| made from
    np.longdouble quotients (a build whose longdouble is a double finds fewer ties and says so); the candidates it prefers are then evaluated in integer arithmetic on the double values of alpha, beta and fl(V beta) (every score to 2^-256 of itself:
    ``exact_signed_gap``), and the best one of the wanted sign is kept;
  * tie_upper / tie_lower: 0 < +-E* <= 2^-46 of the total -- below the exact pipeline's own bound of 164 * 2^-53, so the order of its
    roundings decides the topic; outside_plus / outside_minus: +-E* in [2^-38, 2^-36] -- 4 .. 16 times tier 1's band: tier 1 must decide;
  * every other site is at least 2^-14 away from every boundary (neartie's `safe` rule), so tier 0 decides it;
  * in even wavefronts of a launch every second document is planted and all documents of the wavefront have one length (the planted
    site is ONE site index: decided and handed-over lane groups meet in one loop iteration), in odd wavefronts every document is.

``tier1_model`` is tier 1 restated in numpy in the kernels' association orders (cold_tiers_acc's: per-lane sequential prefix in the
group layout, Hillis-Steele scan of the lane totals; quad_tier1_doc's: one document on 64 lanes, KP / 64 consecutive positions a lane);
``exact_model`` is the exact pipeline with switches for the defects the planted sites must catch (tests/test_sweep_ties_host.py).

Generation time on one core of the development machine: 2.7 .. 5.9 s per state of 128 documents (96 planted sites: 30 .. 60 ms each, the
sort and the look-up of 2^16 .. 2^20 sums), K = 5 .. 3000 alike; per state in the docstring of tests/test_sweep_ties_host.py.  ``state``
caches per argument tuple.
"""
import functools
from fractions import Fraction

import numpy as np

import layoutclasses
import llda_oracle as orc
from neartie import _gap, _site_scores

KINDS = ("lane0_first", "lane_end", "zero_lane", "before_last")
#   lane0_first : the first positive position of lane 0 (nothing in front of it: the threshold is u * total itself)
#   lane_end    : the last positive slot of a lane, the next positive score in the next lane (prefix = a lane total = a scan value)
#   zero_lane   : exact zeros (masked topics) from the boundary through the whole next lane: the next positive position is two lanes on
#                 or more.  A dense document has no zero in front of a positive score: its planted sites take the other three kinds
#   before_last : the boundary in front of the last positive position (behind it: one score, the "no hit -> last positive" rule)
CLASSES = ("tie_upper", "tie_lower", "outside_plus", "outside_minus")
MARGIN = 2.0 ** -40
TIE_MAX = 2.0 ** -46
OUT_LO, OUT_HI = 2.0 ** -38, 2.0 ** -36
SAFE = 2.0 ** -14
SEED, DOC_BASE = 4242, 7
LD = np.longdouble


# ------------------------------------------------------------------------------------------------
# exact evaluation
# ------------------------------------------------------------------------------------------------
def _dyadic(v):
    f = Fraction(float(v))
    return f.numerator, f.denominator


def exact_signed_gap(lay, lab, nd, nk, x, u, alpha, beta, vbeta, b):
    """(prefix up to draw-order position b - u * total) / total of the scores lab (nd + alpha) (x + beta) / (nk + vbeta) as a Fraction:
    alpha, beta, vbeta are taken as the doubles they are, every score is cut off 2^-256 below its own size (K of them: nothing a
    comparison against 2^-46 could see)."""
    an, ad = _dyadic(alpha)
    bn, bd = _dyadic(beta)
    vn, vd = _dyadic(vbeta)
    un = int(u * 2.0 ** 53)
    assert un * 2.0 ** -53 == u
    pos = lay.topic_slot
    tot = front = 0
    for j in np.flatnonzero(lab):
        t = (((int(nd[j]) * ad + an) * (int(x[j]) * bd + bn)) << 256) // (int(nk[j]) * vd + vn)
        tot += t
        if pos[j] <= b:
            front += t
    return Fraction((front << 53) - un * tot, tot << 53)


def positives(lay, lab):
    """draw-order positions with a positive score, ascending"""
    return np.sort(lay.topic_slot[np.flatnonzero(lab)])


def kind_holds(lay, pos, b, kind):
    i = int(np.searchsorted(pos, b))
    if kind == "lane0_first":
        return i == 0 and b // lay.T == 0 and len(pos) > 1
    if i >= len(pos) - 1:
        return False
    nxt = int(pos[i + 1])
    if kind == "lane_end":
        return nxt // lay.T == b // lay.T + 1
    if kind == "zero_lane":
        return nxt // lay.T >= b // lay.T + 2
    return i == len(pos) - 2


# ------------------------------------------------------------------------------------------------
# the tiers, restated
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


def scores(lab, nd, nk, x, alpha, beta, vbeta):
    """the unnormalised scores of the reference's statement, topic order"""
    return lab * (nd + alpha) * ((x + beta) / (nk + vbeta))


def tier1_model(lay, w, u, margin=MARGIN, fp32=False, quad=False):
    """tier 1 on the unnormalised scores w (topic order) -> (sure, topic or -1).
    quad=False: cold_tiers_acc's order (draw_tiers.hpp) -- sequential prefix over the slots of each of the G lanes, Hillis-Steele scan of
    the lane totals, tg = u * total - X[g-1], sure when no prefix lies within total * margin of its lane's threshold.
    quad=True : quad_tier1_doc's (kernel_quad.hpp) -- the same positions in the same order on 64 lanes, KP / 64 (at most 8) to a lane:
    at most 7 additions in a lane and 6 scan steps.
    fp32: the scores are rounded to float first (a tier that is too coarse for the band)."""
    g = lay.grid(np.asarray(w, dtype=np.float64))
    if quad:
        assert lay.KP % 64 == 0 and lay.KP // 64 <= 8
        g = g.reshape(64, lay.KP // 64)
    if fp32:
        g = g.astype(np.float32).astype(np.float64)
    q = np.cumsum(g, axis=1)
    X = _scan(q[:, -1])
    tot = X[-1]
    tg = u * tot - np.concatenate(([0.0], X[:-1]))
    m = tot * margin
    cnt_lo = (q <= (tg - m)[:, None]).sum(axis=1)
    cnt_hi = (q <= (tg + m)[:, None]).sum(axis=1)
    fm = (g > 0) & (np.arange(g.shape[1])[None, :] >= cnt_lo[:, None])
    if bool((cnt_lo != cnt_hi).any()) or not tot > 0.0 or not m < tot or not fm.any():
        return False, -1
    return True, int(lay.slot_topic[int(np.argmax(fm.ravel()))])


def exact_model(lay, lab, nd, nk, x, u, alpha, beta, vbeta, seq_sum=False, reciprocal=False, ge=False):
    """the exact pipeline (oracle/llda_oracle.py: _site and draw_keyed) -> topic; the switches are the defects the planted ties must
    catch: a sequential sum for numpy's pairwise one, w * (1 / S) for w / S, `>=` for the strict `>` of the draw."""
    w = scores(lab, nd, nk, x, alpha, beta, vbeta)
    S = np.cumsum(w)[-1] if seq_sum else np.sum(w)
    prob = w * (1.0 / S) if reciprocal else w / S
    if not ge:
        return orc.draw_keyed(prob, u, lay)
    p = lay.grid(prob)
    q = np.cumsum(p, axis=1)
    X = _scan(q[:, -1])
    tg = u * X[-1] - np.concatenate(([0.0], X[:-1]))
    flag = ((p > 0.0) & (q >= tg[:, None])).ravel()
    if flag.any():
        return int(lay.slot_topic[int(np.argmax(flag))])
    pp = (p > 0.0).ravel()
    return int(lay.slot_topic[pp.shape[0] - 1 - int(np.argmax(pp[::-1]))])


def exact_model_other_k(lay, k_other, lab, nd, nk, x, u, alpha, beta, vbeta):
    """the exact pipeline of a one-leaf layout (K <= 128: 8 lanes x T slots) as the batched kernel's exact_call states it -- np.sum's
    order from tail = K & 7 and tail_row = K >> 3 -- but with ANOTHER problem's K at the site's own KP: what a wavefront that mixes
    sub-problems computes when it takes the layout of the wrong lane group.  Row ``tail_row`` of every lane stays out of the eight
    accumulators and only its first ``tail`` lanes are added behind the butterfly: with the wrong K a full row is cut short (K = 128
    read as 100) or a tail is summed inside the accumulators (100 read as 128).  With k_other = lay.K this IS exact_model."""
    assert lay.G == 8
    w = scores(lab, nd, nk, x, alpha, beta, vbeta)
    g = lay.grid(w)
    tail, tail_row = k_other & 7, k_other >> 3
    acc = np.zeros(8)
    for s in range(lay.T):
        if not (tail != 0 and s == tail_row):
            acc = acc + g[:, s]
    S = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))
    for t in range(tail):
        S = S + (g[t, tail_row] if tail_row < lay.T else 0.0)
    return orc.draw_keyed(w / S, u, lay)


# ------------------------------------------------------------------------------------------------
# planting one site
# ------------------------------------------------------------------------------------------------
def _side(vals):
    """all sums of one value per array, index = ((i0) * n1 + i1) * n2 + ..."""
    v = np.zeros(1, dtype=np.uint64)
    for a in vals:
        v = (v[:, None] + a[None, :]).ravel()
    return v


def _frac64(v):
    """the fractional part of a longdouble as a 64-bit fixed-point number"""
    v = LD(v)
    return np.uint64(int((v - np.floor(v)) * LD(2.0) ** 64) % (1 << 64))


def _decode(idx, sizes):
    out = []
    for n in reversed(sizes):
        idx, r = divmod(int(idx), n)
        out.append(r)
    return out[::-1]


def plant(lay, lab, nd, nk, u, kind, cls, rng, alpha, beta, vbeta, xcap, xlog, bits=57):
    """the planted site's column of counts (without the site's own) -> (x, facts) or None: the label set holds no boundary of that
    kind, or the uniform / the counts left no room"""
    K = lay.K
    pos = positives(lay, lab)
    cand = [int(b) for b in pos if kind_holds(lay, pos, int(b), kind)]
    allowed = np.flatnonzero(lab)
    if not cand or len(allowed) < 3 or not 1e-4 < u < 1 - 1e-4:
        return None
    b = int(rng.choice(cand))
    front = (lay.topic_slot <= b) & (lab > 0)
    behind = (lay.topic_slot > b) & (lab > 0)
    g = {"tie_upper": 0.0, "tie_lower": 0.0, "outside_plus": 2.0 ** -37, "outside_minus": -2.0 ** -37}[cls]
    cl = lab.astype(LD) * (nd.astype(LD) + LD(alpha)) / (nk.astype(LD) + LD(vbeta))
    ul, gl, bl = LD(u), LD(g), LD(beta)
    dl = np.where(front, (1 - ul - gl) * cl, -(ul + gl) * cl)         # d (E - g total) / d x_j
    c = cl.astype(np.float64)
    xmax = float(xcap - 8)

    # the five entries the search turns: neighbours in |d|, so that no window dwarfs another
    nt = min(5, len(allowed))
    by_d = allowed[np.argsort(np.abs(dl[allowed]))]
    q0 = int(rng.integers((len(by_d) - nt) // 2, len(by_d) - nt + 1))
    tun = [int(j) for j in by_d[q0:q0 + nt]]
    j1 = tun[0]                                                       # solved by rounding: the finest step
    others = tun[1:]
    mo = len(others)
    ncap = {4: 1024, 3: 1400, 2: 60000}[mo]

    x = np.minimum(np.floor(np.exp(rng.uniform(0.0, xlog, size=K))), xmax)
    x[rng.random(K) < 0.3] = 0.0
    x[j1] = np.floor(rng.uniform(20000.0, 40000.0))
    for side in (front, behind):                                      # a side of one or two scores (lane0_first, before_last): wide ones
        if side.sum() <= 2:
            x[side] = np.floor(rng.uniform(0.5, 0.95, size=int(side.sum())) * min(xmax, 1e5))
    for j in others:
        x[j] = min(x[j], xmax - ncap)
    # coarse: scale the heavier side until (1 - u) A = u B
    for _ in range(8):
        w = c * (x + beta)
        A, B = float(w[front].sum()), float(w[behind].sum())
        heavy, target = (front, u * B / (1 - u)) if (1 - u) * A > u * B else (behind, (1 - u) * A / u)
        m = heavy.copy()
        m[j1] = False
        fixed = float(w[j1]) if heavy[j1] else 0.0
        rest_x, rest_b = float((c[m] * x[m]).sum()), float(c[m].sum() * beta)
        s = (target - fixed - rest_b) / rest_x if rest_x > 0 else -1.0
        if 0.0 < s <= 1.0:
            x[m] = np.floor(x[m] * s)
            break
        if heavy[j1] and x[j1] >= 4000:
            x[j1] = np.floor(x[j1] / 2)
        elif not heavy[j1] and x[j1] * 2 <= min(xmax, 60000.0):      # the light side cannot be reached by scaling: raise its pin
            x[j1] = x[j1] * 2
        else:
            return None
    else:
        return None

    def residual():
        wl = cl * (x.astype(LD) + bl)
        tot = wl.sum()
        return wl[front].sum() - (ul + gl) * tot, tot

    # greedy: whole counts of single entries outside the tuned five, until the rest is a few steps of j1
    free = np.setdiff1d(allowed, tun)
    for _ in range(12):
        R0, T0 = residual()
        if len(free) == 0 or abs(R0) < 500 * abs(dl[j1]):
            break
        k = np.clip(np.rint((-R0 / dl[free]).astype(np.float64)), -x[free], xmax - x[free])
        res = np.abs(R0 + k.astype(LD) * dl[free])
        i = int(np.argmin(res))
        if not res[i] < abs(R0) or k[i] == 0:
            break
        x[free[i]] += k[i]
    R0, T0 = residual()

    # meet in the middle over the four, the fifth by rounding
    m1 = abs(dl[j1])
    N = int(np.clip(np.ceil(float(m1 / T0 * 2.0 ** bits) ** (1.0 / mo)), 16, ncap))
    if not cls.startswith("tie"):
        N = min(N, 64)
    los, vals = [], []
    for j in others:
        lo = -min(int(x[j]), N // 2)
        lo = min(lo, int(xmax - x[j]) - N + 1)
        if lo < -int(x[j]):
            return None
        los.append(lo)
        vals.append((lo + np.arange(N, dtype=np.int64)).astype(np.uint64) * _frac64(dl[j] / m1))
    ha = (mo + 1) // 2
    # everything modulo m1, as 64-bit fractions of it: unsigned addition wraps where the modulus does, and a sum read as int64 is the
    # signed residual in units of m1 * 2^-64 (a step of j1 is a whole number and drops out)
    a = _frac64(R0 / m1) + _side(vals[:ha])
    bv = _side(vals[ha:])
    order = np.argsort(a)
    qo = np.argsort(-bv)                                              # (sorted queries: the look-up walks the array once)
    i0 = np.empty(len(bv), dtype=np.int64)
    i0[qo] = np.searchsorted(a[order], (-bv)[qo])
    found = []
    for off in (-1, 0):
        ia = order[(i0 + off) % len(a)]
        res = (a[ia] + bv).view(np.int64)
        ok = res > 0 if cls == "tie_upper" else res < 0 if cls == "tie_lower" else res != 0
        idx = np.flatnonzero(ok)
        idx = idx[np.argsort(np.abs(res[idx]))[:32]]
        found += [(abs(int(res[i])), int(ia[i]), int(i)) for i in idx]
    found.sort()
    best = None
    tried = 0
    for _, ia, ib in found:
        y = x.copy()
        ks = _decode(ia, [N] * ha) + _decode(ib, [N] * (mo - ha))
        tot = R0
        for j, lo, kk in zip(others, los, ks):
            y[j] += lo + kk
            tot = tot + LD(lo + kk) * dl[j]
        y[j1] += float(np.rint(np.float64(-tot / dl[j1])))
        if y.min() < 0 or y.max() > xmax or y[j1] > x[j1] + 60000.0:
            continue
        tried += 1
        if tried > 4:
            break
        e = exact_signed_gap(lay, lab, nd, nk, y, u, alpha, beta, vbeta, b)
        if best is None or abs(e - Fraction(g)) < abs(best[0] - Fraction(g)):
            best = (e, y)
    if best is None:
        return None
    e, x = best
    want_pos = cls in ("tie_upper", "outside_plus")
    if (e > 0) != want_pos or e == 0:
        return None
    if cls.startswith("tie") and not abs(e) <= Fraction(TIE_MAX) / 2:
        return None
    if not cls.startswith("tie") and not Fraction(OUT_LO) * Fraction(5, 4) <= abs(e) <= Fraction(OUT_HI) * Fraction(4, 5):
        return None
    # every OTHER boundary is far: the next positive slot is wider than tier 0's band is
    _, cum = _site_scores(lay, lab, nd, nk, x, alpha, beta, vbeta)
    t = u * cum[-1]
    far = np.abs(cum[pos[pos != b]] - t) / cum[-1]
    if len(far) and far.min() < 2.0 ** -30:
        return None
    i = int(np.searchsorted(pos, b))
    k_at, k_next = int(lay.slot_topic[b]), int(lay.slot_topic[pos[i + 1]])
    return x, dict(kind=kind, cls=cls, b=b, k_at=k_at, k_next=k_next, gap=float(e), real=k_at if e > 0 else k_next)


# ------------------------------------------------------------------------------------------------
# the state
# ------------------------------------------------------------------------------------------------
def docs_per_wavefront(K, lanes=None):
    """lanes = lanes of a document in the kernel the state is made for (None: the group layout's G, one wavefront at least;
    the quad kernels: G / 2; the sparse-label kernels: 8 .. 64 by the largest label set)"""
    if lanes is None:
        lanes = orc.layout(K).G
    return max(64 // lanes, 1)


def plan(D, per_wave):
    """-> planted[D] (bool), same_len[D] (bool: the document's length is its wavefront's)"""
    planted = np.zeros(D, dtype=bool)
    same = np.zeros(D, dtype=bool)
    for d in range(D):
        wave, i = divmod(d, per_wave)
        if wave % 2 == 0:
            same[d] = True
            planted[d] = (i + wave // 2) % 2 == 0
        else:
            planted[d] = True
    return planted, same


def doc_lengths(K, D, per_wave, max_sites=4):
    """1 .. max_sites sites a document; the documents of an even wavefront share one length"""
    lens = np.random.default_rng([32, K, D, per_wave]).integers(1, max_sites + 1, size=D)
    _, same = plan(D, per_wave)
    for d in range(D):
        if same[d]:
            lens[d] = 1 + (d // per_wave // 2) % max_sites
    return lens


def _force_labels(lay, lab, kind, dense, rng, sparse):
    """a planted document allows 6 topics at least (the search turns five counts), and -- general label masks only -- a document that
    wants a zero lane gets one masked"""
    K = lay.K
    if dense:
        return
    need = min(K, 6) - int(lab.sum())
    if need > 0:
        lab[rng.choice(np.flatnonzero(lab == 0), size=need, replace=False)] = 1
    lane_of = lay.topic_slot // lay.T
    if kind == "lane_end" and sparse:
        # a handful of labels among hundreds of topics seldom has two in neighbouring lanes: one label moves behind another's lane
        pos = positives(lay, lab)
        if any(kind_holds(lay, pos, int(b), kind) for b in pos):
            return
        ends = [int(b) for i, b in enumerate(pos) if (i == len(pos) - 1 or pos[i + 1] // lay.T != b // lay.T) and (lane_of == b // lay.T + 1).any()]
        spare = [int(t) for t in np.flatnonzero(lab) if t != 0]
        if not ends or len(spare) < 2:
            return
        b = int(rng.choice(ends))
        spare.remove(int(lay.slot_topic[b])) if int(lay.slot_topic[b]) in spare else None
        new = int(rng.choice(np.flatnonzero((lane_of == b // lay.T + 1) & (lab == 0))))
        lab[int(rng.choice(spare))] = 0
        lab[new] = 1
        return
    if kind != "zero_lane":
        return
    if sparse:
        # small label sets leave lanes empty by themselves; a large one gets one lane masked where that adds no label
        pos = positives(lay, lab)
        if any(kind_holds(lay, pos, int(b), kind) for b in pos):
            return
        lanes = np.unique(lane_of)
        has = np.array([bool(lab[lane_of == l].any()) for l in lanes])
        cands = [g for g in range(len(lanes) - 2) if has[g] and has[g + 2:].any() and
                 int(lab.sum()) - int(lab[lane_of == lanes[g + 1]].sum()) >= min(K, 6)]
        if cands:
            lab[lane_of == lanes[int(rng.choice(cands)) + 1]] = 0
        return
    lanes = np.unique(lane_of)
    if len(lanes) < 3:
        return
    g = int(rng.integers(0, len(lanes) - 2))
    lab[lane_of == lanes[g + 1]] = 0
    lab[0] = 1
    for gg in (g, g + 2):
        if not lab[lane_of == lanes[gg]].any():
            lab[int(rng.choice(np.flatnonzero(lane_of == lanes[gg])))] = 1


def make_ties_state(K, D, dense, seed=SEED, doc_base=DOC_BASE, stream=0, lanes=None, label_count=None, xcap=2e8, xlog=11.5, nd_big=2000,
                    max_sites=4, alpha=0.1, beta=0.01, extra_columns=0, word_base=0, bits=57):
    """-> the dict of neartie.make_neartie_state (doc_off, word, freq, z, labs, n_d_k, n_k_v, n_zk, V, alpha, beta) plus
    klass[D], kind[D] (indices into CLASSES / KINDS, -1: not planted), unplaced (documents whose wanted kind gave way to another),
    sites (one record per site: doc, n, planted, lab, nd, nk, x, u -- the state the site sees without its own count), facts[D].
    extra_columns, word_base: V = S + extra_columns, the sites' words are word_base .. word_base + S - 1 (a sub-problem of an
    ensemble over one corpus: the other columns are other sub-problems' words and SubLDA's phantom columns; V * beta counts them)."""
    lay = orc.layout(K)
    rng = np.random.default_rng([31, K, D, int(dense), label_count or 0, 0 if lanes is None else lanes, stream, extra_columns])
    per_wave = docs_per_wavefront(K, lanes)
    planted, same = plan(D, per_wave)
    lens = doc_lengths(K, D, per_wave, max_sites)
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    V = S + extra_columns
    vbeta = V * beta
    word = word_base + np.arange(S, dtype=np.int32)
    freq = rng.integers(1, 4, size=S).astype(np.int32)
    n_zk = np.floor(np.exp(rng.uniform(np.log(1e3), np.log(1e6), size=K))).astype(np.int64)
    sparse = label_count is not None
    if dense:
        labs = np.ones((D, K), dtype=np.uint8)
    elif sparse:
        labs = np.zeros((D, K), dtype=np.uint8)
        labs[:, 0] = 1
        for d in range(D):
            n = int(rng.integers(max(1, label_count - 2), label_count + 1))
            labs[d, rng.choice(K - 1, size=min(n, K - 1), replace=False) + 1] = 1
    else:
        labs = (rng.random((D, K)) < 0.4).astype(np.uint8)
        labs[:, 0] = 1
    kinds = [k for k in KINDS if not (dense and k == "zero_lane")]
    z = np.zeros(S, dtype=np.int64)
    n_d_k = np.zeros((D, K), dtype=np.int64)
    n_k_v = np.zeros((K, V), dtype=np.int64)
    klass = np.full(D, -1, dtype=np.int64)
    kind_of = np.full(D, -1, dtype=np.int64)
    facts = [None] * D
    sites = []
    unplaced = 0
    j = 0
    for d in range(D):
        want_kind = want_cls = None
        if planted[d]:
            want_kind, want_cls = kinds[j % len(kinds)], CLASSES[(j // len(kinds)) % 4]
            j += 1
            _force_labels(lay, labs[d], want_kind, dense, rng, sparse)
        allowed = np.flatnonzero(labs[d])
        lab = labs[d].astype(np.float64)
        s0, L = int(doc_off[d]), int(lens[d])
        zo = rng.choice(allowed, size=L)
        z[s0:s0 + L] = zo
        nd = np.where(rng.random(K) < 0.1, rng.integers(0, nd_big, size=K), rng.integers(0, 20, size=K)) * labs[d]
        np.add.at(nd, zo, freq[s0:s0 + L])
        n_d_k[d] = nd
        nd = nd.astype(np.float64)
        nk = n_zk.astype(np.float64)
        us = orc.keyed_uniform(seed, 0, stream, d + doc_base, np.arange(L))
        for n in range(L):
            i, f, u = s0 + n, float(freq[s0 + n]), float(us[n])
            nd[zo[n]] -= f
            nk[zo[n]] -= f
            if planted[d] and n == L - 1:
                got = None
                for kind in [want_kind] + [k for k in kinds if k != want_kind]:
                    for _attempt in range(12):
                        got = plant(lay, lab, nd, nk, u, kind, want_cls, rng, alpha, beta, vbeta, xcap, xlog, bits)
                        if got is not None:
                            break
                    if got is not None:
                        break
                    unplaced += kind == want_kind
                if got is None:
                    raise RuntimeError("could not plant document %d (K = %d)" % (d, K))
                x, facts[d] = got
                klass[d], kind_of[d] = CLASSES.index(want_cls), KINDS.index(facts[d]["kind"])
            else:
                for _attempt in range(400):
                    x = np.minimum(np.floor(np.exp(rng.uniform(0.0, xlog, size=K))), xcap - 8)
                    x[rng.random(K) < 0.3] = 0.0
                    wp, cum = _site_scores(lay, lab, nd, nk, x, alpha, beta, vbeta)
                    if _gap(cum, u * cum[-1]) > SAFE:
                        break
                else:
                    raise RuntimeError("could not place site %d of document %d" % (n, d))
            sites.append(dict(doc=d, n=n, planted=bool(planted[d] and n == L - 1), lab=lab, nd=nd.copy(), nk=nk.copy(), x=x.copy(), u=u))
            col = x.astype(np.int64)
            col[zo[n]] += int(f)
            n_k_v[:, word_base + i] = col
            zn = exact_model(lay, lab, nd, nk, x, u, alpha, beta, vbeta)
            nd[zn] += f
            nk[zn] += f
    return dict(doc_off=doc_off, word=word, freq=freq, z=z, labs=labs, n_d_k=n_d_k, n_k_v=n_k_v, n_zk=n_zk, V=V, alpha=alpha, beta=beta,
                klass=klass, kind=kind_of, facts=facts, sites=sites, unplaced=unplaced, per_wave=per_wave, planted=planted,
                n_ties=int(((klass == 0) | (klass == 1)).sum()), n_outside=int((klass >= 2).sum()), extra_columns=extra_columns, seed=seed, doc_base=doc_base, stream=stream)


@functools.lru_cache(maxsize=None)
def state(K, D, dense, lanes=None, label_count=None, quad=False, stream=0, doc_base=DOC_BASE, extra_columns=0, word_base=0):
    """the cached states of the tests.  quad: every count within the 16-bit image and documents below 2^16 tokens (neartie's xcap / nd_big)"""
    kw = dict(xcap=65000, xlog=11.0, nd_big=600) if quad else {}
    return make_ties_state(K, D, dense, lanes=lanes, label_count=label_count, stream=stream, doc_base=doc_base, extra_columns=extra_columns,
                           word_base=word_base, **kw)


# ------------------------------------------------------------------------------------------------
# the states of the tests (tests/test_sweep_ties_host.py, tests/test_gpu_sweep_ties.py)
# ------------------------------------------------------------------------------------------------
GENERAL = [(K, dense) for K in (9, 40, 130, 257, 777, 968, 1024) for dense in (True, False)] + [(512, True)]
QUAD = [512, 256, 128, 100, 400]
SPARSE = [(40, 7, 0), (392, 7, 0), (512, 7, 8), (512, 20, 16), (777, 40, 0), (1031, 7, 0), (2048, 7, 8)]        # (K, labels, image)
WIDE = [(1031, False), (2048, True), (3000, False)]
# the largest K of five and of seven tiers (tests/layoutclasses.py): the scan's carry runs over more than four tiers, the last tier is full
# (both with general masks: exact_signed_gap walks the allowed topics in Python integers, and a dense state of 4 295 topics takes 26 s)
WIDE += [(layoutclasses.tier_ks()[5][1], False), (layoutclasses.tier_ks()[7][1], False)]
BATCH = [(5, 4, 5), (60, 9, 15), (128, 17, 32), (100, 33, 64)]                                                    # (K, fewest, most allowed topics)


# Documents per state: a wrong model gets 5 .. 30 % of the ties wrong, so a state needs some 48 ties (128 documents) before every model
# of tests/test_sweep_ties_host.py is caught at every K.  With two workgroups' worth of documents (17 .. 65) the quad states held 7 ..
# 25 ties and the reciprocal-multiply and the `>=` models got none wrong at K = 512, 256 and 400; with 64 documents the wide states and
# the batched sub-problems held 24 and the same happened at K = 2048 and K = 5.
N_DOCS = 128


def general_state(K, dense):
    return state(K, N_DOCS, dense)


def quad_state(K):
    """whole workgroups' worth of documents (128 threads, G / 2 lanes a document) plus one"""
    lanes = orc.layout(K).G // 2
    assert N_DOCS % (128 // lanes) == 0
    return state(K, N_DOCS + 1, True, lanes=lanes, quad=True)


def sparse_lanes(labels):
    n = labels + 1                                                    # the root and up to `labels` labels
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def sparse_state(K, labels):
    return state(K, N_DOCS, False, lanes=sparse_lanes(labels), label_count=labels)


def wide_state(K, dense):
    return state(K, N_DOCS, dense)


BATCH_D = N_DOCS


def batch_state(i):
    """sub-problem i of the batched ensemble: SubLDA's key (stream = index of the sub-problem, documents counted from 0), label sets of
    BATCH[i]'s sizes -- lane classes 8, 16, 32, 64 --, its words behind those of the sub-problems before it in ONE vocabulary"""
    sizes = [int(doc_lengths(K, BATCH_D, docs_per_wavefront(K, sparse_lanes(hi - 1))).sum()) for K, _, hi in BATCH]
    K, _, hi = BATCH[i]
    return state(K, BATCH_D, False, lanes=sparse_lanes(hi - 1), label_count=hi - 1, stream=i, doc_base=0,
                 extra_columns=sum(sizes) - sizes[i], word_base=sum(sizes[:i]))


# Sub-problems that SHARE a lane class but not a layout: the lane groups of one wavefront of llda_sweep_batch then belong to different
# problems (tests/test_gpu_sweep_ties.py test_batched_mixed_waves).  (lanes, documents a sub-problem, [(K, labels, RNG stream)]):
# lanes 8 -- K = 100 with 128 (both KP = 128, another tail), 60 with 64 (both KP = 64) and 96 (KP = 96, T = 12); lanes 16 -- 100 with
# 128 at up to 15 allowed topics.  64 documents (24 ties) a sub-problem in both classes, half of N_DOCS, and no K = 5: choices made for
# the time the host tests take, not forced by anything (the note over N_DOCS applies: with 24 ties a wrong model can slip through).
# So the streams are CHOSEN: with them every state can be planted and every wrong model of tests/test_sweep_ties_host.py, (f)
# included, gets a tie wrong -- (f) only 1 .. 3 of 24.  A change to the generator re-rolls the states and may break that condition;
# it then fails in test_model_verdicts_and_discrimination, it does not weaken silently: choose streams again.
BATCH_MIXED = [(8, 64, [(100, 7, 91), (128, 7, 32), (60, 7, 53), (64, 7, 34), (96, 7, 36)]),
               (16, 64, [(100, 14, 67), (128, 14, 38)])]              # (lanes, documents a sub-problem, [(K, labels, RNG stream)])
MIXED_SUBS = [(g, lanes, D, K, labels, stream) for g, (lanes, D, subs) in enumerate(BATCH_MIXED) for K, labels, stream in subs]


def mixed_state(i):
    """sub-problem i of MIXED_SUBS: as batch_state -- its own stream (not its index in the ensemble), documents counted from 0, its
    words behind those of the sub-problems before it in one vocabulary"""
    sizes = [int(doc_lengths(K, D, docs_per_wavefront(K, lanes)).sum()) for _, lanes, D, K, _, _ in MIXED_SUBS]
    _, lanes, D, K, labels, stream = MIXED_SUBS[i]
    assert sparse_lanes(labels) == lanes
    return state(K, D, False, lanes=lanes, label_count=labels, stream=stream, doc_base=0,
                 extra_columns=sum(sizes) - sizes[i], word_base=sum(sizes[:i]))


def mixed_neighbour(i):
    """the sub-problem of i's lane class with the same KP and another K (-> its index in MIXED_SUBS), or None"""
    g, K = MIXED_SUBS[i][0], MIXED_SUBS[i][3]
    for j, (g2, _, _, K2, _, _) in enumerate(MIXED_SUBS):
        if g2 == g and K2 != K and orc.layout(K2).KP == orc.layout(K).KP:
            return j
    return None


def mixed_order(g):
    """the launch of lane class g of BATCH_MIXED -> list of (index in MIXED_SUBS, document) in launch order.
    A state numbers its documents in blocks of per_wave = 64 / lanes: in an even block every second document is planted and all have
    one length -- the same in every state --, in an odd block every document is planted (plan, doc_lengths).  A wavefront of the launch
    takes half a block of each kind -- its first half from an even block, its second half from the odd block behind it -- and slot i of
    wavefront (.., r) belongs to sub-problem (i + r) % P: neighbouring groups never share a problem, every wavefront holds
    min(P, per_wave) problems, planted and random documents, and the planted sites of its first half are ONE site index."""
    subs = [i for i, s in enumerate(MIXED_SUBS) if s[0] == g]
    lanes, D = BATCH_MIXED[g][:2]
    pw, P = 64 // lanes, len(subs)
    half = pw // 2
    out = []
    for c in range(D // (2 * pw)):
        for h in range(2):
            for r in range(P):
                for i in range(pw):
                    block, j = (2 * c, i) if i < half else (2 * c + 1, i - half)
                    out.append((subs[(i + r) % P], block * pw + h * half + j))
    assert sorted(out) == [(i, d) for i in subs for d in range(D)]
    return out


def verdicts(st, quad=False, other_k=None):
    """the models on every site of a state -> list of dict(doc, n, planted, cls, ref (the exact pipeline's topic), sure / model (tier 1
    at 2^-40), sure0 / model0 (margin 0), sure32 / model32 (fp32 scores), seq / recip / ge (the exact pipeline with one defect); the
    defective models on the planted sites only"""
    K = st["n_d_k"].shape[1]
    lay = orc.layout(K)
    a, b, vb = st["alpha"], st["beta"], st["V"] * st["beta"]
    out = []
    for r in st["sites"]:
        args = (lay, r["lab"], r["nd"], r["nk"], r["x"], r["u"], a, b, vb)
        w = scores(r["lab"], r["nd"], r["nk"], r["x"], a, b, vb)
        rec = dict(doc=r["doc"], n=r["n"], planted=r["planted"], cls=CLASSES[st["klass"][r["doc"]]] if r["planted"] else None,
                   ref=exact_model(*args))
        rec["sure"], rec["model"] = tier1_model(lay, w, r["u"], quad=quad)
        if r["planted"]:
            rec["sure0"], rec["model0"] = tier1_model(lay, w, r["u"], margin=0.0, quad=quad)
            rec["sure32"], rec["model32"] = tier1_model(lay, w, r["u"], fp32=True, quad=quad)
            rec["seq"] = exact_model(*args, seq_sum=True)
            rec["recip"] = exact_model(*args, reciprocal=True)
            rec["ge"] = exact_model(*args, ge=True)
            if other_k is not None:
                rec["other_k"] = exact_model_other_k(lay, other_k, *args[1:])
                rec["own_k"] = exact_model_other_k(lay, K, *args[1:])
        out.append(rec)
    return out


def caught(st, quad=False, other_k=None):
    """how many planted sites each deliberately wrong model gets wrong -> dict(a .. e; with other_k: f, and own = sites on which
    exact_model_other_k with the state's own K differs from the pipeline: none) (tests/test_sweep_ties_host.py)"""
    v = [r for r in verdicts(st, quad, other_k) if r["planted"]]
    ties = [r for r in v if r["cls"].startswith("tie")]
    outside = [r for r in v if not r["cls"].startswith("tie")]
    f = {} if other_k is None else dict(f=sum(r["other_k"] != r["ref"] for r in ties), own=sum(r["own_k"] != r["ref"] for r in v))
    return dict(f, a=sum(not r["sure0"] or r["model0"] != r["ref"] for r in ties), b=sum(r["seq"] != r["ref"] for r in ties),
                c=sum(r["recip"] != r["ref"] for r in ties), d=sum(r["ge"] != r["ref"] for r in ties),
                e=sum(r["sure32"] and r["model32"] != r["ref"] for r in outside), ties=len(ties), outside=len(outside))
