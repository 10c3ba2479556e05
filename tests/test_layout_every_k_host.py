"""Every K from 1 to 7688 on the host: the C library's layout table against numpy's recursion written out again
(tests/layoutclasses.py), against lda_thesis_amd.layout.GroupLayout, and the kernels' summation schedule, run from the C tables, against
np.sum bit for bit.  The classes the layouts fall into are enumerated here once and asserted; the device tests take their K from them.

The schedule test would pass on vectors that any order sums alike, so the same file shows that its vectors tell orders apart: a
sequential sum, one exchanged pair of partners in the wide leaf combine and a tail added before the xor steps each change the bits of a
sum (how many K each defect shows at is printed; the assertions ask for what the arithmetic promises, not for those figures).

Time on one core, two runs: the three every-K tests 5 .. 7 s, 19 .. 32 s (GroupLayout costs milliseconds at large K) and 12 .. 20 s, the
sequential-sum test 3 .. 5 s, the rest under 1 s: 40 .. 65 s in all, in sixteen ranges of K so that no case takes more than 4 s."""
import numpy as np
import pytest

import layoutclasses as lc

N_RANGES = 16
RANGES = [(1 + i * lc.MAX_K // N_RANGES, (i + 1) * lc.MAX_K // N_RANGES) for i in range(N_RANGES)]
range_ids = ["K%d-%d" % r for r in RANGES]


def test_the_ranges_cover_every_k():
    assert RANGES[0][0] == 1 and RANGES[-1][1] == lc.MAX_K == 7688
    assert all(a[1] + 1 == b[0] for a, b in zip(RANGES, RANGES[1:]))


def ks(r):
    return range(r[0], r[1] + 1)


def bits(x):
    return np.float64(x).view(np.uint64)


# ------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RANGES, ids=range_ids)
def test_c_table_against_first_principles(r):
    for K in ks(r):
        c, f = lc.c_tables(K), lc.first_principles(K)
        for n in ("K", "n_leaves", "G", "T", "KP", "tail", "tail_row", "wide", "tiers", "n_rounds"):
            assert c[n] == f[n], (K, n, c[n], f[n])
        for n in ("leaf_start", "leaf_len", "topic_pos", "pos_topic", "pos_lane", "pos_slot"):
            assert np.array_equal(c[n], f[n]), (K, n)
        assert list(zip(c["comb_dst"].tolist(), c["comb_src"].tolist())) == f["comb"], K
        want = lc.as_tables(f)["rounds"]                          # (idle rows and idle leaves read themselves)
        assert np.array_equal(c["rounds"], want), K
        # what the formulas promise of any K: a permutation onto the topics, nothing lost in the padding
        assert c["KP"] == c["G"] * c["T"] and c["KP"] >= K and int((c["pos_topic"] >= 0).sum()) == K
        assert np.array_equal(c["pos_topic"][c["topic_pos"]], np.arange(K))


@pytest.mark.parametrize("r", RANGES, ids=range_ids)
def test_c_table_against_group_layout(r):
    """what tests/test_abi.py::test_layout_init_matches_python_layout compares at 29 K, at every K"""
    from lda_thesis_amd.layout import GroupLayout
    for K in ks(r):
        a, b = lc.c_tables(K), GroupLayout(K)
        for n in ("G", "T", "KP", "tail", "tail_row", "n_rounds"):
            assert a[n] == getattr(b, n), (K, n)
        assert a["n_leaves"] == b.m and bool(a["wide"]) == b.wide and a["tiers"] == b.NT, K
        assert list(zip(a["comb_dst"].tolist(), a["comb_src"].tolist())) == list(b.comb), K
        for n in ("topic_pos", "pos_topic", "pos_lane", "pos_slot"):
            assert np.array_equal(a[n], getattr(b, n)), (K, n)
        for i in range(a["n_rounds"]):
            assert np.array_equal(a["rounds"][i], b.rounds[i]), (K, i)
        # the lane masks the device test builds from the C tables are GroupLayout's
        if K % 97 == 0 or K in (1, lc.MAX_K):
            labs, _ = lc.every_k_rows(K)
            assert np.array_equal(lc.lane_masks(a, labs), b.lane_masks(labs)), K


# ------------------------------------------------------------------------------------------------
# the schedule
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", RANGES, ids=range_ids)
def test_schedule_of_the_c_table_is_numpys_sum(r):
    """two vectors over 60 binades and the three count rows plus alpha of the device test, every K"""
    for K in ks(r):
        t = lc.c_tables(K)
        labs, n = lc.every_k_rows(K)
        vectors = [lc.binade_vector(K, 0), lc.binade_vector(K, 1)] + list(lc.numerators(labs, n))
        for i, x in enumerate(vectors):
            got, want = lc.schedule_sum(t, x), np.sum(np.ascontiguousarray(x))
            assert bits(got) == bits(want), (K, i, float(got).hex(), float(want).hex())


def test_which_layouts_take_the_xor_shortcut():
    """fill_schedule's shortcut (lane xor 8, 16, 32 in place of the partner table) as the tables decide it: taken by every two-leaf
    layout, and by no layout of 32 or 64 lanes -- there the partner table names the FIRST leaf of the other side in the later rounds
    ([2, 2, 0, 0], not p ^ 2), so those layouts combine through the table.  Both branches are the schedule test's to cover; this pins
    which K run which."""
    taken = {}
    for K in range(1, lc.narrow_classes()[(64, 16)][1] + 1):
        g = lc.geometry(K)
        if g["wide"] or g["G"] == 8:
            continue
        x = lc.xor_tree(lc.as_tables(lc.first_principles(K)))
        assert not x or g["n_leaves"] * 8 == g["G"], K
        taken.setdefault(g["G"], set()).add(x)
    assert taken == {16: {True}, 32: {False}, 64: {False}}
    for span in lc.narrow_classes().values():                      # the C tables say the same
        for K in span:
            if lc.geometry(K)["G"] > 8:                            # (one leaf: the flag is set and nothing reads it)
                assert lc.xor_tree(lc.c_tables(K)) == (lc.geometry(K)["G"] == 16), K


# ------------------------------------------------------------------------------------------------
# the vectors discriminate
# ------------------------------------------------------------------------------------------------
def test_a_sequential_sum_is_caught_at_every_k_from_32():
    """the condition tests/test_gpu_every_k.py relies on: the theta of the three count rows differs as bits between numpy's pairwise
    row sum and a sequential one.  (Below 8 numpy's sum IS sequential.)"""
    import readoutref as rr
    same = []
    for K in range(1, lc.MAX_K + 1):
        labs, n = lc.every_k_rows(K)
        assert labs[:, 0].all() and int(n.max()) < 1 << 20 and (n[labs == 0] == 0).all()
        if not (rr.theta_ref(n, labs, lc.ALPHA).view(np.uint64) != lc.sequential_theta(labs, n).view(np.uint64)).any():
            same.append(K)
    print("K at which a sequential row sum gives the same theta:", same)
    assert all(K < 32 for K in same), same
    assert set(range(1, 8)) <= set(same)


def swap_partners(t):
    """the sources of the first two combine steps exchanged: every leaf is still added once, to another partner"""
    m = dict(t, comb_src=t["comb_src"].copy())
    m["comb_src"][[0, 1]] = t["comb_src"][[1, 0]]
    return m


def test_a_swapped_pair_of_comb_entries_is_caught():
    """on the smallest and the largest K of every wide (tiers, T) class and of the tier counts"""
    ks_ = sorted({K for span in list(lc.wide_classes().values()) + list(lc.tier_ks().values()) for K in span})
    caught = []
    for K in ks_:
        t = lc.c_tables(K)
        x = lc.binade_vector(K, 0)
        assert bits(lc.schedule_sum(t, x)) == bits(np.sum(x))
        labs, n = lc.every_k_rows(K)
        rows = [x, lc.binade_vector(K, 1)] + list(lc.numerators(labs, n))
        if any(bits(lc.schedule_sum(swap_partners(t), v)) != bits(np.sum(v)) for v in rows):
            caught.append(K)
    print("a swapped pair of partners changes a sum at %d of %d K: %s" % (len(caught), len(ks_), caught))
    assert len(caught) >= 1


def test_a_tail_added_before_the_xor_steps_is_caught():
    """at K with a tail: one per narrow class that has one, and the new tier classes' edges"""
    ks_ = sorted({K for (G, T), (lo, hi) in lc.narrow_classes().items() for K in (lo, hi) if lc.geometry(K)["tail"]}
                 | {K for nt in (5, 6, 7) for K in lc.tier_ks()[nt] if lc.geometry(K)["tail"]})
    assert len(ks_) >= 12 and {lc.geometry(K)["tail"] for K in ks_} >= {1, 7}
    caught = []
    for K in ks_:
        t = lc.c_tables(K)
        labs, n = lc.every_k_rows(K)
        rows = [lc.binade_vector(K, 0), lc.binade_vector(K, 1)] + list(lc.numerators(labs, n))
        assert all(bits(lc.schedule_sum(t, v)) == bits(np.sum(v)) for v in rows)
        if any(bits(lc.schedule_sum(t, v, tail_first=True)) != bits(np.sum(v)) for v in rows):
            caught.append(K)
    print("a tail added first changes a sum at %d of %d K: %s" % (len(caught), len(ks_), caught))
    assert len(caught) >= 1


# ------------------------------------------------------------------------------------------------
# the classes
# ------------------------------------------------------------------------------------------------
def test_the_classes_of_all_k():
    c = lc.classes()
    assert set(lc.wide_classes()) == {(2, 12), (2, 16), (3, 16), (4, 12), (4, 16), (5, 16), (6, 16), (7, 16), (8, 12), (8, 16)}
    assert set(lc.narrow_classes()) == {(8, 1), (8, 2), (8, 4), (8, 8), (8, 12), (8, 16), (16, 12), (16, 16), (32, 12), (32, 16),
                                        (64, 12), (64, 16)}
    assert len(c["narrow"]) == 352 and len(c["wide"]) == 616
    # the geometry of K is not monotone: the classes overlap
    assert lc.narrow_classes()[(32, 16)][0] < lc.narrow_classes()[(16, 16)][1]
    assert lc.tier_ks()[4][1] > lc.tier_ks()[5][0]
    assert min(lo for lo, _ in lc.wide_classes().values()) == 969 and max(hi for _, hi in lc.wide_classes().values()) == lc.MAX_K


def test_tier_ks_are_the_edges_of_five_six_and_seven_tiers():
    tk = lc.tier_ks()
    assert sorted(tk) == [2, 3, 4, 5, 6, 7, 8]
    assert (tk[5], tk[6], tk[7]) == ((3849, 4167), (4168, 4231), (4232, 4295))
    for nt, leaves, tails in ((5, (33, 40), (1, 7)), (6, (41, 48), (0, 7)), (7, (49, 56), (0, 7))):
        lo, hi = (lc.geometry(K) for K in tk[nt])
        assert (lo["n_leaves"], hi["n_leaves"]) == leaves and (lo["tail"], hi["tail"]) == tails
        assert lo["tiers"] == hi["tiers"] == nt and lo["T"] == hi["T"] == 16 and lo["G"] == 64 * nt
        assert lc.wide_classes()[(nt, 16)] == tk[nt]
        # the last tier is partly empty at the smallest K and full at the largest
        assert leaves[0] == 8 * (nt - 1) + 1 and leaves[1] == 8 * nt
    # the interval holds 4-tier layouts too: tier counts do not grow with K
    between = [K for K in range(tk[5][0], tk[7][1] + 1) if lc.geometry(K)["tiers"] == 4]
    assert 4000 in between and 4096 in between
    assert sum(lc.geometry(K)["tiers"] in (5, 6, 7) for K in range(1, lc.MAX_K + 1)) == tk[7][1] - tk[5][0] + 1 - len(between) == 416
    assert lc.new_tier_ks() == [3849, 4168, 4232] and lc.new_tier_ks("largest") == [4167, 4231, 4295]
