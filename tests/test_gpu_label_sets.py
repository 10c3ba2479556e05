"""llda_label_sets on the device: masks, counts and the per-label tp / fp / fn against the CPU restatement (tests/labelref.py), all
integers and therefore exact: K around the 32-bit words and the 64-lane ballots, D around the four documents of a workgroup round,
NaN and +-inf thresholds, scores on their threshold and one ulp either side, empty sets with and without at_least_one, a tie for
the best label, a NaN document, with and without truth."""
import numpy as np
import pytest

import labelref

pytestmark = pytest.mark.gpu

GUARD = 8
P32, P64 = np.int32(-0x12345679), np.int64(-0x123456789ABCDEF)
KS = (1, 31, 32, 33, 130, 512)
DS = (1, 63, 64, 65, 1000)


def make(rng, D, K, first, ld):
    """scores around their thresholds -- exactly on it, one ulp below, one ulp above -- mixed with a coarse grid; thresholds with NaN
    and +inf entries and, for odd D and K > 3, -inf in the last column (which every score but a NaN reaches: no set is empty then);
    every fifth document reaches no finite threshold, with a tie for its best label or nothing but +-0.0; document 7 has a NaN in
    the last column, document 8 a NaN under a NaN threshold"""
    thr = rng.integers(1, 6, size=K) / 8
    special = rng.integers(0, 8, size=K)
    thr[special == 0] = np.nan
    thr[special == 1] = np.inf
    if K > 3 and D % 2:
        thr[K - 1] = -np.inf
    base = np.where(np.isfinite(thr), thr, 0.5)
    which = rng.integers(0, 3, size=(D, K))
    s = np.where(which == 0, base, np.where(which == 1, np.nextafter(base, -np.inf), np.nextafter(base, np.inf)))
    s = np.where(rng.random((D, K)) < 0.5, s, rng.integers(0, 8, size=(D, K)) / 16)
    for d in range(0, D, 5):
        s[d] = -1.0
        if d % 10 == 5:
            s[d, K - 1] = -np.inf                                 # (-inf >= -inf: predicted under that threshold)
        elif K - first >= 2:
            s[d, [first, K - 1]] = -0.5                           # a tie for the best label
        if d % 15 == 0:
            s[d] = np.where(np.arange(K) % 2 == 0, -0.0, 0.0)
    if D > 7:
        s[7, K - 1] = np.nan
    if D > 8 and np.isnan(thr).any():
        s[8, int(np.flatnonzero(np.isnan(thr))[0])] = np.nan
    score = np.full((D, ld), np.nan)
    score[:, :K] = s
    score[:, :first] = 9.0                                        # above every finite threshold, and never predicted
    truth = (rng.random((D, K)) < 0.3).astype(np.uint8) * 0xFF
    return score, thr, truth


def run(score, thr, truth, K, first, alo, skip=()):
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    D, W = score.shape[0], (K + 31) // 32
    s, th = torch.from_numpy(score).to(dev), torch.from_numpy(thr).to(dev)
    t = None if truth is None else torch.from_numpy(truth).to(dev)
    full = lambda n, pat, dt: torch.full((n + GUARD,), pat.item(), dtype=dt, device=dev)
    bufs = dict(mask=full(D * W, P32, torch.int32), n_pred=full(D, P32, torch.int32), n_hit=full(D, P32, torch.int32),
                n_true=full(D, P32, torch.int32))
    for n in ("tp", "fp", "fn"):
        bufs[n] = full(K, P64, torch.int64)
        bufs[n][:K] = 0                                           # the caller zeroes what is added to
    _native.label_sets(s, th, t, D, K, first, alo, ld=score.shape[1], **{n: b for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def check(got, want, D, K, with_truth=True, skip=(), what=""):
    W = (K + 31) // 32
    sizes = dict(mask=D * W, n_pred=D, n_hit=D, n_true=D, tp=K, fp=K, fn=K)
    for name, g in got.items():
        n = sizes[name]
        pat = P64 if g.dtype == np.int64 else P32
        assert (g[n:] == pat).all(), "%s: guard words behind %s overwritten" % (what, name)
        if name in skip or (not with_truth and name in ("n_hit", "n_true", "tp", "fp", "fn")):
            untouched = 0 if name in ("tp", "fp", "fn") else pat
            assert (g[:n] == untouched).all(), "%s: %s was written" % (what, name)
            continue
        w = labelref.pack_mask(want["mask"]).view(np.int32).reshape(-1) if name == "mask" else want[name]
        bad = np.flatnonzero(g[:n] != w)
        assert bad.size == 0, "%s: %s differs at %s: got %s want %s" % (what, name, bad[:5], g[:n][bad[:5]], np.asarray(w)[bad[:5]])


@pytest.mark.parametrize("K", KS)
def test_against_labelref(K):
    rng = np.random.default_rng(K)
    for D in DS:
        for first in sorted(set((0, min(1, K), min(5, K)))):
            score, thr, truth = make(rng, D, K, first, K + (3 if D % 2 else 0))
            for alo in (0, 1):
                what = "K=%d D=%d first=%d at_least_one=%d" % (K, D, first, alo)
                want = labelref.label_sets(score, thr, truth, first=first, at_least_one=bool(alo), K=K)
                check(run(score, thr, truth, K, first, alo), want, D, K, what=what)
                check(run(score, thr, None, K, first, alo), want, D, K, with_truth=False, what=what + " truth=NULL")
                elig = np.flatnonzero(~np.isnan(thr[first:])) + first
                if D == 1000 and elig.size:                       # the planted documents did what they are there for
                    assert (want["n_pred"] == 0).any() == (alo == 0), what
                    assert (want["n_pred"][7] == -1) == (K - 1 in elig) and (want["n_pred"] == -1).sum() <= 1, what


def test_planted_documents_by_hand():
    """K = 6, first = 1: what every rule does, spelled out"""
    thr = np.array([0.0, 0.5, np.nan, 0.25, np.inf, -np.inf])
    inf = np.inf
    score = np.array([[9.0, 0.5, 9.0, 0.2, 1e300, -inf],         # on the threshold; under a NaN threshold; below; below +inf; -inf >= -inf
                      [9.0, np.nextafter(0.5, 0), 9.0, np.nextafter(0.25, 1), inf, np.nan],   # NaN in an eligible column
                      [9.0, np.nextafter(0.5, 1), np.nan, 0.25, inf, 0.0]])                   # NaN under the NaN threshold
    truth = np.array([[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 0]], dtype=np.uint8)
    for alo in (0, 1):
        got = run(score, thr, truth, 6, 1, alo)
        assert list(got["mask"][:3].view(np.uint32)) == [0b100010, 0, 0b111010]
        assert list(got["n_pred"][:3]) == [2, -1, 4] and list(got["n_hit"][:3]) == [1, 0, 2] and list(got["n_true"][:3]) == [3, 5, 3]
        assert list(got["tp"][:6]) == [0, 1, 0, 1, 1, 0] and list(got["fp"][:6]) == [0, 1, 0, 0, 0, 2]
        assert list(got["fn"][:6]) == [0, 1, 3, 2, 1, 1]
    thr[5] = 2.0                                                  # now document 0 reaches one label, document 3 none
    score = np.concatenate([score, [[9.0, 0.125, 7.0, -0.0, 0.125, 0.0]]])
    truth = np.concatenate([truth, np.array([[0, 0, 0, 0, 1, 0]], dtype=np.uint8)])
    got0, got1 = run(score, thr, truth, 6, 1, 0), run(score, thr, truth, 6, 1, 1)
    assert list(got0["mask"][:4].view(np.uint32)) == [0b000010, 0, 0b011010, 0] and list(got0["n_pred"][:4]) == [1, -1, 3, 0]
    # the best eligible label of document 3: 0.125 in columns 1 and 4 -> the lower topic id; column 2 (7.0) has no threshold
    assert list(got1["mask"][:4].view(np.uint32)) == [0b000010, 0, 0b011010, 0b000010] and list(got1["n_pred"][:4]) == [1, -1, 3, 1]
    assert got0["fn"][4] == 2 and got1["fn"][4] == 2 and got1["fp"][1] == got0["fp"][1] + 1


def test_every_output_pointer_may_be_null_and_counts_accumulate():
    rng = np.random.default_rng(5)
    D, K = 300, 70
    score, thr, truth = make(rng, D, K, 1, K + 1)
    want = labelref.label_sets(score, thr, truth, first=1, at_least_one=True, K=K)
    for name in ("mask", "n_pred", "n_hit", "n_true", "tp", "fp", "fn"):
        check(run(score, thr, truth, K, 1, 1, skip=(name,)), want, D, K, skip=(name,), what="%s = NULL" % name)
    # two calls over the halves add up in the caller's counters
    import torch
    from lda_thesis_amd import _native
    s, th, t = (torch.from_numpy(x).to("cuda:0") for x in (score, thr, truth))
    cnt = {n: torch.zeros((K,), dtype=torch.int64, device="cuda:0") for n in ("tp", "fp", "fn")}
    for lo, hi in ((0, 140), (140, D)):
        _native.label_sets(s[lo:hi], th, t[lo:hi], hi - lo, K, 1, True, ld=K + 1, **cnt)
    for n in cnt:
        assert np.array_equal(cnt[n].cpu().numpy(), want[n]), n


def test_largest_k():
    rng = np.random.default_rng(9)
    K, D = 7688, 9
    score, thr, truth = make(rng, D, K, 1, K)
    for alo in (0, 1):
        check(run(score, thr, truth, K, 1, alo), labelref.label_sets(score, thr, truth, first=1, at_least_one=bool(alo), K=K), D, K, what="K=7688")


def test_python_surface():
    import torch
    from lda_thesis_amd import labelwise
    rng = np.random.default_rng(3)
    D, K = 200, 45
    score, thr, truth = make(rng, D, K, 1, K)
    score[7, K - 1] = 0.0                                         # no NaN document: the ratios are defined
    want = labelref.label_sets(score, thr, truth, first=1, at_least_one=True)
    wide = torch.from_numpy(np.concatenate([score, np.full((D, 5), np.nan)], axis=1)).to("cuda:0")
    for arg in (score, wide[:, :K]):
        r = labelwise.label_sets(arg, thr, truth, first=1)
        assert np.array_equal(r.sets(), want["mask"])
        h = r.host()
        for n in ("n_pred", "n_hit", "n_true", "tp", "fp", "fn"):
            assert np.array_equal(h[n], want[n]), n
    assert r.scores() == labelwise.set_scores(want["tp"], want["fp"], want["fn"], want["n_pred"], want["n_hit"], want["n_true"], first=1)
    tp, fp, fn = (int(want[n][1:].sum()) for n in ("tp", "fp", "fn"))
    assert r.micro_f1 == 2 * tp / (2 * tp + fp + fn) and 0 < r.macro_f1 < 1 and 0 < r.example_f1 < 1
    bare = labelwise.label_sets(score, thr, None, first=1, at_least_one=False)
    assert bare.tp is None and np.array_equal(bare.sets(), labelref.label_sets(score, thr, None, first=1, at_least_one=False)["mask"])
    with pytest.raises(ValueError):
        bare.scores()
    score[7, K - 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        labelwise.label_sets(score, np.where(np.isnan(thr), 0.5, thr), truth).scores()
    with pytest.raises(ValueError):
        labelwise.label_sets(score, thr[:-1])
