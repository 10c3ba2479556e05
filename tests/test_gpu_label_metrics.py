"""llda_label_metrics on the device: bit for bit against its CPU restatement (tests/labelref.py), every output including the order,
around every seam of the geometry -- the padding of a run, the shapes of the merge tree, the default chunk, the edges of the
transposing tile, label batches -- for every score kind and with the special columns planted.  Nothing is masked out."""
import numpy as np
import pytest

import labelref

pytestmark = pytest.mark.gpu

C = 4096                                                  # LLDA_LABEL_CHUNK
GUARD = 8
NAN_BITS = np.uint64(0x7FF8000000000000)
PATTERN = {"int32": np.int32(-0x12345679), "int64": np.int64(-0x123456789ABCDEF), "float64": np.float64(-1234.5)}
SCALARS = ("n_pos", "n_thr", "auc_num", "auc", "thr_tp", "thr_fp", "f1", "thr", "flags")


def mixed(rng, D, L, plant=True, first=0, ld=None):
    """(score (D, ld), truth (D, K)), K = first + L: the ranked columns cycle through every score kind, the first five of them carry
    the planted cases; every column the kernel must not read holds NaN / 0xFF"""
    K = first + L
    s = np.empty((D, L))
    for j, kind in enumerate(labelref.KINDS):
        cols = np.arange(j, L, len(labelref.KINDS))
        if cols.size:
            s[:, cols] = labelref.gen_column_scores(rng, kind, D, cols.size)
    score = np.full((D, K if ld is None else ld), np.nan)
    score[:, first:K] = s
    truth = np.full((D, K), 0xFF, dtype=np.uint8)
    truth[:, first:K] = labelref.gen_label_truth(rng, D, L)
    if plant:
        labelref.plant_columns(rng, score, truth, first)
    return score, truth


def run(score, truth, K, first, n_labels, chunk=0, skip=(), want_order=True):
    """one llda_label_metrics call with guarded, pre-filled output buffers and guarded scratch -> dict of numpy arrays (whole
    buffers, guards included)"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    D = score.shape[0]
    s, t = torch.from_numpy(score).to(dev), torch.from_numpy(truth).to(dev)
    shapes = {n: (n_labels, torch.float64 if n in ("auc", "f1", "thr") else torch.int32 if n == "flags" else torch.int64) for n in SCALARS}
    if want_order:
        shapes["order"] = (n_labels * D, torch.int32)
    bufs = {n: torch.full((m + GUARD,), PATTERN[str(dt).split(".")[1]].item(), dtype=dt, device=dev) for n, (m, dt) in shapes.items()}
    need = _native.label_scratch_bytes(D, n_labels, chunk)
    scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    _native.label_metrics(s, t, D, K, first, n_labels, scratch[:need], ld=score.shape[1], chunk=chunk,
                          **{n: b for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    assert (scratch[need:] == 0xA5).all().item(), "bytes behind the scratch overwritten"
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), NAN_BITS, a.view(np.uint64))
    return a


def check(got, want, D, n_labels, skip=(), what=""):
    for name, g in got.items():
        n = n_labels * D if name == "order" else n_labels
        pat = PATTERN[str(g.dtype)]
        assert (g[n:] == pat).all(), "%s: guard words behind %s overwritten" % (what, name)
        if name in skip:
            assert (g[:n] == pat).all(), "%s: %s was written" % (what, name)
            continue
        w = np.asarray(want[name]).reshape(-1)
        bad = np.flatnonzero(bits(g[:n]) != bits(w))
        assert bad.size == 0, "%s: %s differs at %s: got %s want %s" % (what, name, bad[:5], g[:n][bad[:5]], w[bad[:5]])


def against_ref(score, truth, K, first, n_labels, chunk, what):
    want = labelref.label_metrics(score, truth, first=first, n_labels=n_labels, K=K)
    check(run(score, truth, K, first, n_labels, chunk), want, score.shape[0], n_labels, what=what)
    return want


@pytest.mark.parametrize("D", (1, 2, 7, 8, 9, 255, 256, 257))
def test_one_run_and_its_padding(D):
    rng = np.random.default_rng(100 + D)
    score, truth = mixed(rng, D, 13, first=1)
    against_ref(score, truth, 14, 1, 13, 256, "D=%d chunk=256" % D)


@pytest.mark.parametrize("D", (511, 512, 513, 769, 1283, 2309))
def test_merge_tree_shapes(D):
    """chunk = 256: two full runs, a run of one pair, three runs; 1 283 = 6 runs -> 3 -> 2 -> 1 with a run without a partner at the
    second level; 2 309 = 10 -> 5 -> 3 -> 2 -> 1"""
    rng = np.random.default_rng(200 + D)
    score, truth = mixed(rng, D, 13, first=1)
    against_ref(score, truth, 14, 1, 13, 256, "D=%d chunk=256" % D)


@pytest.mark.parametrize("D", (C - 1, C, C + 1, 2 * C + 3, 3 * C))
def test_default_chunk(D):
    rng = np.random.default_rng(300 + D)
    score = np.full((D, 4), np.nan)
    for j, kind in enumerate(("grid", "ulp", "foldin")):
        score[:, 1 + j] = labelref.gen_column_scores(rng, kind, D, 1)[:, 0]
    truth = np.full((D, 4), 0xFF, dtype=np.uint8)
    truth[:, 1:] = labelref.gen_label_truth(rng, D, 3)
    against_ref(score, truth, 4, 1, 3, 0, "D=%d default chunk" % D)


@pytest.mark.parametrize("first", (0, 1, 5))
@pytest.mark.parametrize("n_labels", (1, 63, 64, 65))
def test_transpose_tile_edges(n_labels, first):
    """K = 130, ld > K, 300 documents (five document tiles, two runs of 256): label tiles with one column, one short of full, full,
    and one over; the columns outside first .. first + n_labels - 1 hold NaN / 0xFF and must not be read"""
    rng = np.random.default_rng(1000 * first + n_labels)
    K, D = 130, 300
    score, truth = mixed(rng, D, n_labels, first=first, ld=K + 3)
    wide_s, wide_t = np.full((D, K + 3), np.nan), np.full((D, K), 0xFF, dtype=np.uint8)
    wide_s[:, :first + n_labels] = score[:, :first + n_labels]
    wide_t[:, :first + n_labels] = truth
    against_ref(wide_s, wide_t, K, first, n_labels, 256, "n_labels=%d first=%d" % (n_labels, first))


def test_label_batches():
    """one call with all 129 labels against two calls that split them at 60: the same bytes, and the reference's"""
    rng = np.random.default_rng(7)
    K, D = 130, 600
    score, truth = mixed(rng, D, K - 1, first=1, ld=K + 1)
    want = against_ref(score, truth, K, 1, K - 1, 256, "whole")
    a, b = run(score, truth, K, 1, 60, 256), run(score, truth, K, 61, 69, 256)
    for name in want:
        w = D if name == "order" else 1
        got = np.concatenate([a[name][:60 * w], b[name][:69 * w]])
        assert np.array_equal(bits(got), bits(np.asarray(want[name]).reshape(-1))), name


@pytest.mark.parametrize("kind", labelref.KINDS)
def test_every_score_kind_across_every_boundary(kind):
    """D = 1 283 with chunk = 256, four columns of one kind: all-equal is one threshold spanning every run and tile, grid has four
    distinct values (tie groups across every boundary), ulp neighbours, mostly exact zeros, +-0.0, +-inf and denormals"""
    rng = np.random.default_rng(sum(map(ord, kind)))
    D = 1283
    score = np.concatenate([np.full((D, 1), np.nan), labelref.gen_column_scores(rng, kind, D, 4)], axis=1)
    truth = np.concatenate([np.full((D, 1), 0xFF, dtype=np.uint8), labelref.gen_label_truth(rng, D, 4)], axis=1)
    want = against_ref(score, truth, 5, 1, 4, 256, kind)
    if kind in ("equal", "zeros", "signed_zero"):
        assert (want["n_thr"] == 1).all() and (want["flags"] & 4).all() and (want["auc"] == 0.5).all()
        assert ((want["flags"] & 8) != 0).all() == (kind != "equal")
    if kind == "grid":
        assert (want["n_thr"] == 4).all()
    if kind == "signed_zero":                             # the threshold is the first document's own zero, sign and all
        assert np.array_equal(np.signbit(want["thr"]), np.signbit(score[0, 1:]))


@pytest.mark.parametrize("chunk,D", ((256, 1283), (0, C + 77)))
def test_planted_columns(chunk, D):
    rng = np.random.default_rng(D)
    score = np.concatenate([np.full((D, 1), np.nan), rng.integers(0, 50, size=(D, 7)) / 64], axis=1)
    truth = np.concatenate([np.full((D, 1), 0xFF, dtype=np.uint8), labelref.gen_label_truth(rng, D, 7)], axis=1)
    nan_col = labelref.plant_columns(rng, score, truth, 1)
    want = against_ref(score, truth, 8, 1, 7, chunk, "planted")
    assert nan_col == 5
    fl = want["flags"]
    assert fl[0] & 1 and np.isnan(want["auc"][0]) and np.isnan(want["f1"][0]) and np.isnan(want["thr"][0])      # no positive
    assert fl[1] & 2 and np.isnan(want["auc"][1]) and want["f1"][1] == 1.0 and want["thr_tp"][1] == D          # no negative
    assert want["auc"][2] == 1.0 and (want["thr_tp"][2], want["thr_fp"][2], want["f1"][2]) == (1, 0, 1.0)       # the only positive first
    assert want["auc"][3] == 0.0 and (want["thr_tp"][3], want["thr_fp"][3]) == (1, D - 1)                       # ... and last
    assert fl[4] == 16 and (want["order"][4] == -1).all() and (fl[[5, 6]] == 0).all()                           # a NaN; the others unaffected
    clean = score.copy()
    clean[:, nan_col] = 0.0
    other = labelref.label_metrics(clean, truth, first=1)
    for name in want:
        assert np.array_equal(bits(np.delete(want[name], 4, axis=0)), bits(np.delete(other[name], 4, axis=0))), name


def test_every_output_pointer_may_be_null():
    rng = np.random.default_rng(11)
    D = 700
    score, truth = mixed(rng, D, 9, first=1)
    want = labelref.label_metrics(score, truth, first=1)
    for name in SCALARS + ("order",):
        check(run(score, truth, 10, 1, 9, 256, skip=(name,)), want, D, 9, skip=(name,), what="%s = NULL" % name)


def test_python_surface():
    import torch
    from lda_thesis_amd import labelwise
    rng = np.random.default_rng(3)
    D, K = 900, 41
    score, truth = mixed(rng, D, K - 1, first=1, plant=False)
    score[:, 0] = 0.5
    truth[:, 0] = 1
    truth[:, 1], truth[:, 2] = 0, 1                      # a label without a positive, one without a negative
    want = labelref.label_metrics(score, truth, first=1)
    wide = torch.from_numpy(np.concatenate([score, np.full((D, 7), np.nan)], axis=1)).to("cuda:0")
    per_label = 24 * 1024                                 # chunk = 256: 900 documents are padded to 1 024
    for arg, kw in ((score, dict(chunk=256)), (wide[:, :K], dict(chunk=256, max_scratch_bytes=7 * per_label + 16)), (score, {})):
        r = labelwise.label_metrics(arg, truth, first=1, order=True, **kw)      # numpy uploaded; a device view keeps its stride; batches of 7
        h = r.host()
        for name in labelref.OUTPUTS:
            assert np.array_equal(bits(h[name]), bits(want[name])), name
    assert labelwise.label_metrics(score, truth, first=1).order is None
    m = labelwise.macro(r)
    keep = (want["flags"] & 3) == 0
    assert m["n_labels"] == int(keep.sum()) == K - 3 and m["skipped"] == 2
    assert m["macro_auc"] == np.mean(want["auc"][keep]) and m["macro_f1"] == np.mean(want["f1"][keep])
    thr = labelwise.thresholds(r)
    assert thr.shape == (K,) and np.isnan(thr[0]) and np.isnan(thr[1]) and np.array_equal(bits(thr[1:]), bits(want["thr"]))
    bad = score.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        labelwise.macro(labelwise.label_metrics(bad, truth, chunk=256))
    with pytest.raises(ValueError):
        labelwise.label_metrics(score[:0], truth[:0])
    with pytest.raises(ValueError):
        labelwise.label_metrics(score, truth[:, :5])
