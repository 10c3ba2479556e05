"""Every K from 1 to LLDA_MAX_K: the layout restated from numpy's pairwise recursion alone, the classes the layouts fall into, and the
summation schedule of the kernels run on the host from the C library's tables (test infrastructure, host only: numpy; the C tables are
read through lda_thesis_amd._native when ``c_tables`` is called, nothing here imports lda_thesis_amd.layout).

numpy adds a contiguous float64 vector of n elements pairwise: n <= 128 is one leaf (eight interleaved accumulators, combined as
((0+1)+(2+3))+((4+5)+(6+7)), then n % 8 leftovers one after the other); a longer vector is split at n / 2 rounded down to a multiple of
8 and the two halves' sums are added.  include/llda_gibbs.h places topic ``rel`` of leaf ``p`` at lane 8 p + (rel & 7), slot rel >> 3, a
document on G = 8 * (leaves rounded up to a power of two; beyond 8 leaves -- "wide" -- to a multiple of 8) lanes of T slots (the longest
leaf's rows, rounded up to a multiple of 4 beyond 2), and (lane g, slot s) at position ((s / 4) G + g) 4 + s % 4 of a row of KP = G T
entries (g T + s where T is 1 or 2).

``first_principles(K)`` is that paragraph and nothing else.  ``classes()`` walks all K once and keeps, per geometry and per schedule
signature, the smallest and the largest K: the K lists of the device tests come from there, never from typed-in ranges.
``schedule_sum(tables, x)`` adds a K-vector the way group_sum_tail (device_common.hpp) and wide_sum (kernel_wide.hpp) do, from the
tables alone, with switches for the defects that tests/test_layout_every_k_host.py shows the test vectors catch.
"""
import functools

import numpy as np

MAX_K = 7688                # LLDA_MAX_K
LEAF = 128                  # numpy's pairwise-sum block
NARROW_LEAVES = 8           # LLDA_MAX_LEAVES
MAX_ROUNDS = 4              # LLDA_MAX_ROUNDS
ALPHA = 0.1
COUNT_BITS = (8, 14, 20)    # the three rows of every_k_rows: counts below 2^8, 2^14 and 2^20


# ------------------------------------------------------------------------------------------------
# numpy's recursion
# ------------------------------------------------------------------------------------------------
def leaf_lengths(n):
    if n <= LEAF:
        return [n]
    h = n // 2
    h -= h % 8
    return leaf_lengths(h) + leaf_lengths(n - h)


def _tree(n, first):
    """-> (node, leaves below it); a node is a leaf index or a pair of nodes"""
    if n <= LEAF:
        return first, 1
    h = n // 2
    h -= h % 8
    a, na = _tree(h, first)
    b, nb = _tree(n - h, first + na)
    return (a, b), na + nb


def _first(t):
    return t if isinstance(t, int) else _first(t[0])


def _depth(t):
    return 0 if isinstance(t, int) else 1 + max(_depth(t[0]), _depth(t[1]))


def _members(t):
    return [t] if isinstance(t, int) else _members(t[0]) + _members(t[1])


def _nodes(t):
    """the internal nodes in post-order"""
    return [] if isinstance(t, int) else _nodes(t[0]) + _nodes(t[1]) + [t]


def comb_of(K):
    """total[first leaf of the left child] += total[first leaf of the right child] for every internal node, post-order"""
    return [(_first(t[0]), _first(t[1])) for t in _nodes(_tree(K, 0)[0])]


def rounds_of(K):
    """the narrow kernels' partner table: a node of depth d (a leaf has depth 0) is added in round d - 1; every leaf below its left
    child reads the first leaf of the right child and the other way round; a leaf that idles reads itself"""
    nodes = _nodes(_tree(K, 0)[0])
    n_rounds = max([_depth(t) for t in nodes] + [0])
    rounds = np.tile(np.arange(NARROW_LEAVES, dtype=np.int32), (n_rounds, 1))
    for t in nodes:
        left, right = _members(t[0]), _members(t[1])
        rounds[_depth(t) - 1, left] = right[0]
        rounds[_depth(t) - 1, right] = left[0]
    return rounds


def geometry(K):
    """dict(wide, tiers, G, T, KP, n_leaves, tail, tail_row) from the leaf lengths"""
    lens = leaf_lengths(K)
    m = len(lens)
    wide = m > NARROW_LEAVES
    if wide:
        P = (m + 7) // 8 * 8
    else:
        P = 1
        while P < m:
            P *= 2
    T = max((n + 7) // 8 for n in lens)
    if T > 2:
        T = (T + 3) // 4 * 4
    return dict(wide=int(wide), tiers=P // 8 if wide else 0, G=8 * P, T=T, KP=8 * P * T, n_leaves=m, tail=lens[-1] % 8,
                tail_row=lens[-1] // 8)


def first_principles(K):
    """the fields of llda_layout (include/llda_gibbs.h) for K topics"""
    lens = np.asarray(leaf_lengths(K), dtype=np.int64)
    g = geometry(K)
    G, T, KP = g["G"], g["T"], g["KP"]
    start = np.concatenate(([0], np.cumsum(lens)[:-1]))
    leaf = np.repeat(np.arange(len(lens)), lens)
    rel = np.arange(K) - start[leaf]
    lane, slot = 8 * leaf + (rel & 7), rel >> 3
    w = 4 if T % 4 == 0 else T
    position = lambda ln, sl: ((sl // w) * G + ln) * w + sl % w
    topic_pos = position(lane, slot)
    pos_topic = np.full(KP, -1, dtype=np.int64)
    pos_topic[topic_pos] = np.arange(K)
    all_lane, all_slot = np.divmod(np.arange(KP), T)
    pos_lane, pos_slot = np.zeros(KP, dtype=np.int64), np.zeros(KP, dtype=np.int64)
    pos_lane[position(all_lane, all_slot)], pos_slot[position(all_lane, all_slot)] = all_lane, all_slot
    out = dict(g, K=K, leaf_start=start, leaf_len=lens, topic_pos=topic_pos, pos_topic=pos_topic, pos_lane=pos_lane, pos_slot=pos_slot,
               comb=comb_of(K))
    out["rounds"] = rounds_of(K) if not g["wide"] else np.zeros((0, NARROW_LEAVES), dtype=np.int32)
    out["n_rounds"] = len(out["rounds"])
    return out


# ------------------------------------------------------------------------------------------------
# the classes
# ------------------------------------------------------------------------------------------------
def signature(K):
    """what the summation schedule of K depends on: narrow (G, T, leaves, tail, tail_row, rounds), wide (tiers, T, leaves, tail,
    tail_row, comb)"""
    g = geometry(K)
    if g["wide"]:
        return True, (g["tiers"], g["T"], g["n_leaves"], g["tail"], g["tail_row"], tuple(comb_of(K)))
    return False, (g["G"], g["T"], g["n_leaves"], g["tail"], g["tail_row"], tuple(map(tuple, rounds_of(K).tolist())))


def _span(table, key, K):
    lo, hi = table.get(key, (K, K))
    table[key] = (min(lo, K), max(hi, K))


@functools.lru_cache(maxsize=None)
def classes():
    """dict of four tables, each key -> (smallest K, largest K):
    geometry  (wide, G, T);  tiers  number of tiers of a wide layout;  narrow / wide  the schedule signatures"""
    out = dict(geometry={}, tiers={}, narrow={}, wide={})
    for K in range(1, MAX_K + 1):
        g = geometry(K)
        _span(out["geometry"], (bool(g["wide"]), g["G"], g["T"]), K)
        if g["wide"]:
            _span(out["tiers"], g["tiers"], K)
        wide, sig = signature(K)
        _span(out["wide" if wide else "narrow"], sig, K)
    return out


def narrow_classes():
    """(G, T) -> (smallest K, largest K) of the narrow layouts"""
    return {(G, T): span for (wide, G, T), span in classes()["geometry"].items() if not wide}


def wide_classes():
    """(tiers, T) -> (smallest K, largest K) of the wide layouts"""
    return {(G // 64, T): span for (wide, G, T), span in classes()["geometry"].items() if wide}


def tier_ks():
    """number of tiers -> (smallest K, largest K) with that many, for every tier count of a wide layout (2 .. 8)"""
    return dict(classes()["tiers"])


def new_tier_ks(which="smallest"):
    """the K of 5, 6 and 7 tiers the device tests take: the smallest or the largest of each"""
    return [tier_ks()[nt][0 if which == "smallest" else 1] for nt in (5, 6, 7)]


def seam_ks(have=()):
    """the smallest and the largest K of every narrow (G, T) class, ascending, without those in ``have``"""
    ks = sorted({K for span in narrow_classes().values() for K in span})
    return [K for K in ks if K not in set(have)]


# ------------------------------------------------------------------------------------------------
# the C tables
# ------------------------------------------------------------------------------------------------
_ARRAYS = ("leaf_start", "leaf_len", "rounds", "comb_dst", "comb_src", "topic_pos", "pos_topic", "pos_lane", "pos_slot")
_SCALARS = ("K", "n_leaves", "G", "T", "KP", "tail", "tail_row", "n_rounds", "wide", "tiers")


def c_tables(K):
    """llda_layout_init(K) as a dict of ints and int32 arrays cut to their used length (rounds keeps all LLDA_MAX_ROUNDS rows: the
    idle rows are part of what fill_schedule reads).  One buffer view of the struct: no per-element conversion."""
    import ctypes
    from lda_thesis_amd import _native
    out = _native.LldaLayout()
    _native.check(_native.lib().llda_layout_init(int(K), ctypes.byref(out)), "llda_layout_init(K=%d)" % K)
    words = np.frombuffer(out, dtype=np.int32)
    t = {n: int(getattr(out, n)) for n in _SCALARS}
    used = dict(leaf_start=t["n_leaves"], leaf_len=t["n_leaves"], rounds=MAX_ROUNDS * NARROW_LEAVES, comb_dst=t["n_leaves"] - 1,
                comb_src=t["n_leaves"] - 1, topic_pos=t["K"], pos_topic=t["KP"], pos_lane=t["KP"], pos_slot=t["KP"])
    for n in _ARRAYS:
        first = getattr(_native.LldaLayout, n).offset // 4
        t[n] = words[first:first + used[n]].copy()
    t["rounds"] = t["rounds"].reshape(MAX_ROUNDS, NARROW_LEAVES)
    return t


def as_tables(fp):
    """first_principles(K) in the shape of c_tables(K) (for schedule_sum without the library)"""
    t = {n: fp[n] for n in _SCALARS + ("leaf_start", "leaf_len", "topic_pos", "pos_topic", "pos_lane", "pos_slot")}
    rounds = np.tile(np.arange(NARROW_LEAVES, dtype=np.int32), (MAX_ROUNDS, 1))
    rounds[:fp["n_rounds"]] = fp["rounds"]
    t["rounds"] = rounds
    t["comb_dst"] = np.asarray([a for a, _ in fp["comb"]], dtype=np.int32)
    t["comb_src"] = np.asarray([b for _, b in fp["comb"]], dtype=np.int32)
    return t


# ------------------------------------------------------------------------------------------------
# the kernels' summation schedule
# ------------------------------------------------------------------------------------------------
def xor_tree(t):
    """fill_schedule (llda_gibbs.hip): every lane group holds a leaf and round r pairs leaf p with p ^ (1 << r)"""
    P2 = t["G"] // 8
    if t["n_leaves"] != P2:
        return False
    r = 0
    while (1 << r) < P2:
        if any(int(t["rounds"][r][p]) != p ^ (1 << r) for p in range(P2)):
            return False
        r += 1
    return True


def device_row(t, x, dtype=np.float64):
    """the K-vector x in device order: entry topic_pos[k] holds x[k], zeros in the padding"""
    row = np.zeros(np.shape(x)[:-1] + (t["KP"],), dtype=dtype)
    row[..., t["topic_pos"]] = x
    return row


def schedule_sum(t, x, tail_first=False):
    """np.sum(x) as group_sum / group_sum_tail and wide_sum add it, from the tables pos_lane, pos_slot, tail, tail_row, n_leaves, rounds,
    n_rounds, comb_dst, comb_src (and G, T, KP, topic_pos for the device row):
      chains   every (virtual) lane adds its T slots from 0.0 in slot order; the lanes of the last leaf keep slot tail_row aside
      leaf     the eight chains of a leaf: lane ^ 1, lane ^ 2, then the mirror image 7 - lane
      tail     the ``tail`` values kept aside, one after the other, onto the last leaf's total
      leaves   narrow: lane ^ 8, ^ 16, ^ 32 when xor_tree, else ``rounds`` (a leaf adds its partner's total unless it is its own
               partner; the sum is leaf 0's); wide: total[comb_dst[i]] += total[comb_src[i]] in order, the sum is total[0]
    tail_first (a defect): the tail goes onto the last leaf's first chain BEFORE the xor steps."""
    G, T = t["G"], t["T"]
    grid = np.zeros((G, T), dtype=np.float64)
    grid[t["pos_lane"], t["pos_slot"]] = device_row(t, np.asarray(x, dtype=np.float64))
    lane = np.arange(G)
    last = t["n_leaves"] - 1
    last_lanes = (lane >> 3) == last
    acc = np.zeros(G, dtype=np.float64)
    tv = np.zeros(G, dtype=np.float64)
    for s in range(T):
        aside = last_lanes & (t["tail"] != 0 and s == t["tail_row"])
        tv = np.where(aside, grid[:, s], tv)
        acc = np.where(aside, acc, acc + grid[:, s])
    if tail_first:
        for i in range(t["tail"]):
            acc[8 * last] = acc[8 * last] + tv[8 * last + i]
    acc = acc + acc[lane ^ 1]
    acc = acc + acc[lane ^ 2]
    acc = acc + acc[lane ^ 7]
    if not tail_first:
        for i in range(t["tail"]):
            acc = np.where(last_lanes, acc + tv[8 * last + i], acc)
    if t["wide"]:
        total = acc[::8].copy()
        for a, b in zip(t["comb_dst"], t["comb_src"]):
            total[a] = total[a] + total[b]
        return total[0]
    if G > 8 and xor_tree(t):
        for d in (8, 16, 32):
            if d < G:
                acc = acc + acc[lane ^ d]
        return acc[0]
    for r in range(t["n_rounds"]):
        partner = np.asarray(t["rounds"][r])[lane >> 3]
        other = acc[partner * 8 + (lane & 7)]
        acc = np.where(partner != (lane >> 3), acc + other, acc)
    return acc[0]


# ------------------------------------------------------------------------------------------------
# the test vectors
# ------------------------------------------------------------------------------------------------
def binade_vector(K, seed=0):
    """K doubles of either sign whose magnitudes spread over 60 binades, 2^-30 .. 2^30"""
    rng = np.random.default_rng([41, K, seed])
    return np.ldexp(rng.uniform(1.0, 2.0, K), rng.integers(-30, 30, K)) * rng.choice([-1.0, 1.0], K)


def every_k_rows(K):
    """labs (3, K) uint8 -- a general mask, the root always set -- and n (3, K) int64 counts below 2^8, 2^14 and 2^20 on the labelled
    topics.  The rows are there to tell summation orders apart, so of up to eight seeded draws the first is taken whose theta differs
    as bits between numpy's pairwise row sum and a sequential one (no draw can below 8 topics, where numpy adds sequentially, and
    tests/test_layout_every_k_host.py shows which K are left without one: none from 32 on)."""
    for attempt in range(8):
        rng = np.random.default_rng([42, K, attempt])
        labs = (rng.random((3, K)) < 0.7).astype(np.uint8)
        labs[:, 0] = 1
        n = np.stack([rng.integers(0, 1 << b, K) for b in COUNT_BITS]).astype(np.int64) * labs
        if K < 8 or orders_differ(labs, n):
            break
    return labs, n


def pairwise_theta(labs, n, alpha=ALPHA):
    """theta with numpy's own row sums (tests/readoutref.py theta_ref, restated: this file imports nothing of the tests)"""
    num = numerators(labs, n, alpha)
    return num / np.array([np.sum(row) for row in num])[:, None]


def orders_differ(labs, n, alpha=ALPHA):
    return bool((pairwise_theta(labs, n, alpha).view(np.uint64) != sequential_theta(labs, n, alpha).view(np.uint64)).any())


def numerators(labs, n, alpha=ALPHA):
    return np.ascontiguousarray(n.astype(np.int64) + labs.astype(np.float64) * float(alpha))


def sequential_theta(labs, n, alpha=ALPHA):
    """theta with the rows added one element after the other: what a wrong summation order would give"""
    num = numerators(labs, n, alpha)
    return num / np.cumsum(num, axis=1)[:, -1:]


def lane_masks(t, labs):
    """(D, K) labels -> (D, G) uint16 lane masks from the C tables: bit pos_slot of lane pos_lane for every labelled topic"""
    labs = np.asarray(labs) != 0
    out = np.zeros((labs.shape[0], t["G"]), dtype=np.uint32)
    lane, slot = t["pos_lane"][t["topic_pos"]], t["pos_slot"][t["topic_pos"]].astype(np.uint32)
    np.bitwise_or.at(out, (slice(None), lane), labs.astype(np.uint32) << slot)
    return out.astype(np.uint16)
