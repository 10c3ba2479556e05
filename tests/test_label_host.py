"""tests/labelref.py -- the yardstick of the label-wise GPU tests -- against definitions that share no code with it (brute force
over pairs, plain loops over thresholds), and the host-side ratios of lda_thesis_amd.labelwise on hand-made counts.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import labelref
from lda_thesis_amd import labelwise

SHAPES = ((1, 1), (2, 3), (7, 4), (16, 5), (33, 6), (60, 8))


def cases():
    rng = np.random.default_rng(20250607)
    for kind in labelref.KINDS:
        for D, L in SHAPES:
            s = labelref.gen_column_scores(rng, kind, D, L)
            y = labelref.gen_label_truth(rng, D, L)
            if D >= 16:
                y[:, 0] = 0
                y[:, 1] = 1
            yield kind, s, y


CASES = list(cases())


def geq(a, b):
    """a >= b as IEEE values, without numpy"""
    return float(a) >= float(b)


@pytest.mark.parametrize("kind,s,y", CASES, ids=["%s-%dx%d" % (k, s.shape[0], s.shape[1]) for k, s, y in CASES])
def test_restatement_against_definitions(kind, s, y):
    D, L = s.shape
    ref = labelref.label_metrics(s, y, first=0)
    for l in range(L):
        col, t = [float(x) for x in s[:, l]], [bool(x) for x in y[:, l]]
        # order: score descending, then document id ascending
        order = sorted(range(D), key=lambda d: (-col[d], d))
        assert list(ref["order"][l]) == order
        pos, neg = [d for d in range(D) if t[d]], [d for d in range(D) if not t[d]]
        assert ref["n_pos"][l] == len(pos)
        assert ref["n_thr"][l] == len(set(0.0 if x == 0 else x for x in col))
        # A: twice the (positive above negative) pairs plus the tied ones
        A = sum(2 * (col[p] > col[n]) + (col[p] == col[n]) for p in pos for n in neg)
        assert ref["auc_num"][l] == A
        if pos and neg:
            assert ref["auc"][l] == A / (2 * len(pos) * len(neg))
        else:
            assert np.isnan(ref["auc"][l])
        # best F1: every distinct score as a threshold with >=
        best = None
        for th in sorted(set(col), reverse=True):
            pred = [geq(col[d], th) for d in range(D)]
            tp = sum(1 for d in range(D) if pred[d] and t[d])
            fp = sum(pred) - tp
            if tp > 0:
                f = Fraction(2 * tp, tp + fp + len(pos))
                if best is None or f > best[0]:                   # (thresholds descend: an equal F1 further down does not replace)
                    best = (f, tp, fp, th)
        if best is None:
            assert np.isnan(ref["f1"][l]) and np.isnan(ref["thr"][l]) and ref["thr_tp"][l] == 0 and ref["thr_fp"][l] == 0
        else:
            assert (ref["thr_tp"][l], ref["thr_fp"][l]) == (best[1], best[2])
            assert ref["f1"][l] == (2 * best[1]) / (best[1] + best[2] + len(pos))
            assert ref["thr"][l] == best[3]                       # as values; the bits below
            first_doc = min(d for d in range(D) if col[d] == best[3])
            assert np.float64(ref["thr"][l]).view(np.uint64) == s[first_doc, l].view(np.uint64)
        fl = (1 if not pos else 0) | (2 if not neg else 0) | (4 if ref["n_thr"][l] < 2 else 0) | (8 if all(x == 0 for x in col) else 0)
        assert ref["flags"][l] == fl


def test_restatement_nan_column():
    rng = np.random.default_rng(3)
    s, y = rng.random((20, 3)), labelref.gen_label_truth(rng, 20, 3)
    s[7, 1] = np.nan
    ref = labelref.label_metrics(s, y, first=0)
    clean = labelref.label_metrics(np.delete(s, 1, axis=1), np.delete(y, 1, axis=1), first=0)
    assert ref["flags"][1] == 16 and (ref["order"][1] == -1).all()
    assert [ref[n][1] for n in ("n_pos", "n_thr", "auc_num", "thr_tp", "thr_fp")] == [0] * 5
    assert np.isnan([ref[n][1] for n in ("auc", "f1", "thr")]).all()
    for n in labelref.OUTPUTS:                                    # the others unaffected
        np.testing.assert_array_equal(np.delete(ref[n], 1, axis=0), clean[n])


def test_first_and_n_labels_select_columns():
    rng = np.random.default_rng(5)
    s, y = rng.random((30, 9)), labelref.gen_label_truth(rng, 30, 9)
    whole = labelref.label_metrics(s, y, first=0)
    part = labelref.label_metrics(s, y, first=2, n_labels=4)
    for n in labelref.OUTPUTS:
        np.testing.assert_array_equal(part[n], whole[n][2:6])


@pytest.mark.parametrize("low", (-np.inf, 2.0), ids=("minus_inf", "no_minus_inf"))      # (a -inf threshold leaves no document empty)
@pytest.mark.parametrize("at_least_one", (False, True))
def test_label_sets_against_a_double_loop(at_least_one, low):
    rng = np.random.default_rng(11)
    D, K, first = 40, 9, 1
    s = rng.integers(0, 6, size=(D, K)) / 4
    s[3] = 0.0                                                    # nothing reaches a threshold; a tie for the best label
    s[4, :] = -1.0
    s[4, [5, 7]] = 0.125
    s[5, 2] = np.nan
    s[6, 4] = np.nan                                              # under a NaN threshold: not a NaN document
    thr = np.array([0.0, 0.5, 0.75, np.inf, np.nan, 0.25, low, 1.0, 1.25])
    s[7, 6] = -np.inf                                             # reaches the -inf threshold
    y = labelref.gen_label_truth(rng, D, K)
    ref = labelref.label_sets(s, thr, y, first=first, at_least_one=at_least_one)
    tp, fp, fn = [0] * K, [0] * K, [0] * K
    for d in range(D):
        elig = [k for k in range(first, K) if thr[k] == thr[k]]
        if any(s[d, k] != s[d, k] for k in elig):
            pred, n_pred = set(), -1
        else:
            pred = set(k for k in elig if geq(s[d, k], thr[k]))
            if not pred and at_least_one:
                pred = {min(elig, key=lambda k: (-float(s[d, k]), k))}
            n_pred = len(pred)
        true = set(k for k in range(first, K) if y[d, k])
        assert set(np.flatnonzero(ref["mask"][d])) == pred and ref["n_pred"][d] == n_pred
        assert ref["n_hit"][d] == len(pred & true) and ref["n_true"][d] == len(true)
        for k in range(first, K):
            tp[k] += k in pred and k in true
            fp[k] += k in pred and k not in true
            fn[k] += k not in pred and k in true
    assert (list(ref["tp"]), list(ref["fp"]), list(ref["fn"])) == (tp, fp, fn)
    assert ref["n_pred"][5] == -1 and ref["n_pred"][6] >= 0 and ref["mask"][7, 6] == (low < 0)
    if low > 0:
        assert ref["n_pred"][3] == ref["n_pred"][4] == int(at_least_one)
        if at_least_one:
            assert list(np.flatnonzero(ref["mask"][3])) == [1]    # all equal: the first eligible label
            assert list(np.flatnonzero(ref["mask"][4])) == [5]    # 5 before 7: equal scores go by topic id
    words = labelref.pack_mask(ref["mask"])
    np.testing.assert_array_equal(labelwise.mask_rows(words, K), ref["mask"])


def test_rank_key_orders_like_the_scores():
    xs = [np.inf, 1e308, 1.0, 5e-324, 0.0, -0.0, -5e-324, -1.0, -np.inf]
    keys = [labelref.rank_key(x) for x in xs]
    assert keys == sorted(keys) and keys[4] == keys[5] and len(set(keys)) == len(xs) - 1


def test_macro_on_hand_made_results():
    h = dict(flags=np.array([0, 1, 0, 2, 4], dtype=np.int32), auc=np.array([0.5, np.nan, 0.75, np.nan, 1.0]),
             f1=np.array([0.25, np.nan, 0.5, 1.0, 0.75]))
    m = labelwise.macro(h)
    assert m == dict(macro_auc=np.mean([0.5, 0.75, 1.0]), macro_f1=np.mean([0.25, 0.5, 0.75]), n_labels=3, skipped=2)
    empty = labelwise.macro(dict(flags=np.array([1, 2], dtype=np.int32), auc=np.array([np.nan] * 2), f1=np.array([np.nan, 1.0])))
    assert np.isnan(empty["macro_auc"]) and np.isnan(empty["macro_f1"]) and empty["n_labels"] == 0 and empty["skipped"] == 2
    with pytest.raises(ValueError, match="NaN"):
        labelwise.macro(dict(flags=np.array([0, 16], dtype=np.int32), auc=np.zeros(2), f1=np.zeros(2)))


def test_thresholds_from_a_host_dict():
    h = dict(flags=np.array([0, 1, 0], dtype=np.int32), thr=np.array([0.5, np.nan, -0.0]))
    thr = labelwise.thresholds(h, K=5, first=2)
    assert np.isnan(thr[[0, 1, 3]]).all() and thr[2] == 0.5 and np.signbit(thr[4]) and thr[4] == 0
    with pytest.raises(ValueError, match="NaN"):
        labelwise.thresholds(dict(flags=np.array([16], dtype=np.int32), thr=np.array([np.nan])), K=2, first=1)


def test_set_scores_on_hand_made_counts():
    #          root  a  b  c (never seen or predicted)
    tp = [9, 3, 0, 0]
    fp = [9, 1, 2, 0]
    fn = [9, 2, 1, 0]
    n_pred, n_hit, n_true = [2, 1, 0, 3], [1, 1, 0, 1], [2, 1, 0, 3]
    r = labelwise.set_scores(tp, fp, fn, n_pred, n_hit, n_true, first=1)
    assert r["micro_f1"] == 6 / 12                                # root's counts are left out
    assert r["macro_f1"] == np.mean([6 / 9, 0 / 3]) and r["labels_scored"] == 2
    assert r["example_f1"] == np.mean([2 / 4, 2 / 2, 2 / 6]) and r["docs_scored"] == 3
    nothing = labelwise.set_scores([0, 0], [0, 0], [0, 0], [0], [0], [0], first=1)
    assert all(np.isnan(nothing[k]) for k in ("micro_f1", "macro_f1", "example_f1"))
    with pytest.raises(ValueError, match="NaN"):
        labelwise.set_scores(tp, fp, fn, [2, -1, 0, 3], n_hit, n_true)
