"""llda_count_hist (the counts of counts behind the estimate of alpha and beta) against numpy.bincount on the host, bit for bit.

Matrices in the group layout of every kind -- one, two, 4 ... 16 slots per lane, padded rows, a tail, the quad geometry, a wide
layout -- with label masks per row (root plus 1 ... 7 labels) or the all-topics row, about 70 % zeros, values in every range the
kernel treats differently (registers below 4, the workgroup's LDS histogram below 4096, global atomics up to n_bins, the overflow
list beyond), n_bins - 1, n_bins, n_bins + 1 and 2^31 - 1 planted at the first and last allowed position of the first and last
row, and nonzero garbage in every position that is padded or masked off."""
import collections

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = [5, 12, 40, 100, 130, 512, 1031]      # T = 1, T = 2, 8 slots (padded), 16 slots with a tail, two leaves, quad geometry, wide
ROWS = [1, 63, 1000]
BINS = [1, 4, 1000, 65536]
GUARD = -7777


def build(K, rows, per_row, n_bins, seed=0):
    """-> (counts (rows, KP) int32, masks uint16 (rows, G) or (G,), allowed (rows, KP) bool)"""
    from lda_thesis_amd.layout import group_layout
    lay = group_layout(K)
    rng = np.random.default_rng([seed, K, rows, int(per_row)])
    labs = np.ones((rows, K), dtype=np.uint8)
    if per_row:
        labs[:, 1:] = 0
        for r in range(rows):
            labs[r, 1 + rng.choice(K - 1, size=int(rng.integers(1, min(7, K - 1) + 1)), replace=False)] = 1
    allowed = np.zeros((rows, lay.KP), dtype=bool)
    allowed[:, lay.topic_pos] = labs.astype(bool)
    masks = lay.lane_masks(labs) if per_row else lay.lane_masks(np.ones((1, K)))[0]
    u = rng.random((rows, lay.KP))
    counts = np.where(u < 0.7, 0, np.where(u < 0.9, rng.integers(1, 4, size=u.shape),
                                           np.where(u < 0.97, rng.integers(4, 4096, size=u.shape), rng.integers(4096, 70000, size=u.shape))))
    garbage = rng.integers(1, 2 ** 31, size=u.shape) * rng.choice([-1, 1], size=u.shape)
    counts = np.where(allowed, counts, garbage).astype(np.int64)
    spots = [(r, p) for r in (0, rows - 1) for p in (np.flatnonzero(allowed[r])[0], np.flatnonzero(allowed[r])[-1])]
    for (r, p), v in zip(spots, (n_bins - 1, n_bins, n_bins + 1, 2 ** 31 - 1)):
        counts[r, p] = v
    return counts.astype(np.int32), masks, allowed


def expected(counts, allowed, n_bins):
    vals = counts[allowed].astype(np.int64)
    inside = (vals >= 0) & (vals < n_bins)
    return np.bincount(vals[inside], minlength=n_bins).astype(np.int64), np.sort(vals[~inside])


def run(counts, masks, K, per_row, n_bins, cap, pieces=1):
    """llda_count_hist over the rows in ``pieces`` calls -> (hist, over_n, over buffer with 8 guard words behind its capacity)"""
    import torch
    from lda_thesis_amd import _native
    c = torch.from_numpy(counts).cuda()
    m = torch.from_numpy(np.ascontiguousarray(masks).view(np.int16)).cuda()
    hist = torch.zeros((n_bins,), dtype=torch.int64, device="cuda")
    over = torch.full((cap + 8,), GUARD, dtype=torch.int32, device="cuda")
    over_n = torch.zeros((1,), dtype=torch.int64, device="cuda")
    rows = counts.shape[0]
    cuts = [rows * i // pieces for i in range(pieces + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        _native.count_hist(c[lo:hi], K, m[lo:hi] if per_row else m, per_row, hist, over, over_n, over_cap=cap)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), int(over_n.item()), over.cpu().numpy()


@pytest.mark.parametrize("per_row", [True, False], ids=["label_masks", "all_topics_row"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("K", KS)
def test_count_hist_equals_bincount(K, rows, per_row):
    for n_bins in BINS:
        counts, masks, allowed = build(K, rows, per_row, n_bins)
        want_hist, want_over = expected(counts, allowed, n_bins)
        assert want_over.size >= 2 and (counts[~allowed] != 0).all()
        what = "K=%d rows=%d n_bins=%d" % (K, rows, n_bins)
        hist, over_n, over = run(counts, masks, K, per_row, n_bins, want_over.size)
        np.testing.assert_array_equal(hist, want_hist, err_msg=what)
        assert over_n == want_over.size, what
        np.testing.assert_array_equal(np.sort(over[:over_n].astype(np.int64)), want_over, err_msg=what)
        assert (over[over_n:] == GUARD).all(), what
        assert int(hist.sum()) + over_n == int(allowed.sum()), what
        # a buffer smaller than the number of values outside: the count is still the true one, nothing is written behind the capacity
        for cap in (want_over.size // 2, 0):
            hist, over_n, over = run(counts, masks, K, per_row, n_bins, cap)
            np.testing.assert_array_equal(hist, want_hist, err_msg=what)
            assert over_n == want_over.size, what
            assert (over[cap:] == GUARD).all(), what
            stored = collections.Counter(over[:cap].tolist())
            assert GUARD not in stored and not stored - collections.Counter(want_over.tolist()), what
        # hist and over_n accumulate: the two halves of the rows in two calls
        if rows > 1:
            hist, over_n, over = run(counts, masks, K, per_row, n_bins, want_over.size, pieces=2)
            np.testing.assert_array_equal(hist, want_hist, err_msg=what)
            np.testing.assert_array_equal(np.sort(over[:over_n].astype(np.int64)), want_over, err_msg=what)


@pytest.mark.parametrize("per_row", [True, False], ids=["label_masks", "all_topics_row"])
def test_count_hist_indexes_past_2_to_the_31(per_row):
    """rows * KP = 2^31 + 1536 entries (8.6 GB of zeros built on the device): values planted in the last rows are found, and with
    per-row masks the rows masked off at the far end are not counted"""
    import torch
    from lda_thesis_amd import _native
    from lda_thesis_amd.layout import group_layout
    K, rows, n_bins = 512, (1 << 22) + 3, 16
    lay = group_layout(K)
    assert lay.KP == 512 and rows * lay.KP > 2 ** 31
    c = torch.zeros((rows, lay.KP), dtype=torch.int32, device="cuda")
    row = torch.from_numpy(lay.lane_masks(np.ones((1, K))).view(np.int16)).cuda()
    c[rows - 1, 511] = 7
    c[rows - 1, 0] = 100
    c[rows - 2, 17] = 7
    c[rows - 3, 5] = 9                       # (masked off with per-row masks)
    c[1 << 21, 3] = 15
    masks = row[0]
    want = {0: rows * 512 - 5, 7: 2, 9: 1, 15: 1}
    if per_row:
        masks = row.repeat(rows, 1)
        masks[rows - 3] = 0
        masks[5] = 0
        want = {0: (rows - 2) * 512 - 4, 7: 2, 15: 1}
    hist = torch.zeros((n_bins,), dtype=torch.int64, device="cuda")
    over = torch.full((4,), GUARD, dtype=torch.int32, device="cuda")
    over_n = torch.zeros((1,), dtype=torch.int64, device="cuda")
    _native.count_hist(c, K, masks, per_row, hist, over, over_n)
    assert {i: int(h) for i, h in enumerate(hist.tolist()) if h} == want
    assert int(over_n.item()) == 1 and over.tolist() == [100, GUARD, GUARD, GUARD]
