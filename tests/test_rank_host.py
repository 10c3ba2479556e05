"""llda_rank_labels without a GPU: its CPU restatement (tests/rankref.py) against the host metrics of lda_thesis_amd.evaluate,
which tests/golden/evaluate.npz pins to the reference, and the argument validation of the entry point itself."""
import ctypes
import warnings

import numpy as np

import rankref
from lda_thesis_amd import evaluate

LS = (2, 3, 7, 63, 64, 65, 127, 391, 511, 1023, 2999)
ROWS = 12                                   # per (L, kind): the 9th is all false, the 11th all true
EPS = 2.0 ** -53


def _cases():
    rng = np.random.default_rng(20240611)
    for L in LS:
        for kind in rankref.KINDS:
            s = rankref.gen_scores(rng, kind, ROWS, L)
            y = rankref.gen_truth(rng, ROWS, L)
            yield L, kind, s, y


def _host_row(s, y):
    """(auc or 'raise' , f1) of one row through evaluate.rates / macro_auc_roc / get_f1"""
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        tps, tns, fps, fns, fprs, tprs = evaluate.rates(s[None, :], y[None, :])
        try:
            auc = float(evaluate.macro_auc_roc(fprs, tprs))
        except ValueError as e:
            assert "At least 2 points" in str(e)
            auc = "raise"
        f1 = float(evaluate.get_f1(tps, fps, tns, fns))
    return auc, f1


def test_rankref_agrees_with_the_host_metrics():
    """per row: the same NaN pattern, ValueError on the host exactly where T < 2, |auc - host| <= (4 T + 32) 2^-53 (every fpr / tpr
    carries one rounding of a value <= 1, so a trapezoid term is off by <= 2 * 2^-53 from the difference plus three relative
    roundings, and numpy's pairwise sum of T - 1 non-negative terms adds at most 13) and |f1 - host| <= 8 * 2^-53 f1 (five roundings
    on the host, one here)."""
    total = compared = 0
    worst_auc = worst_f1 = 0.0
    for L, kind, s, y in _cases():
        padded = np.concatenate([np.full((ROWS, 1), np.nan), s], axis=1)             # column 0 is not ranked
        ytrue = np.concatenate([np.full((ROWS, 1), 255, dtype=np.uint8), y], axis=1)
        r = rankref.rank_rows(padded, ytrue, first=1, top_n=0)
        for d in range(ROWS):
            total += 1
            auc, f1 = _host_row(s[d], y[d])
            T = int(r["n_thr"][d])
            assert T == np.unique(s[d]).size
            assert (auc == "raise") == (T < 2) == bool(r["flags"][d] & rankref.ONE_THRESHOLD), (L, kind, d)
            if auc != "raise":
                assert np.isnan(auc) == np.isnan(r["auc"][d]), (L, kind, d)
            assert np.isnan(f1) == np.isnan(r["f1"][d]), (L, kind, d)
            assert bool(r["flags"][d] & rankref.NO_POSITIVE) == (y[d].sum() == 0)
            assert bool(r["flags"][d] & rankref.NO_NEGATIVE) == (y[d].sum() == L)
            if r["flags"][d] != 0:
                continue
            compared += 1
            da, df = abs(r["auc"][d] - auc), abs(r["f1"][d] - f1)
            worst_auc, worst_f1 = max(worst_auc, da / (T * EPS)), max(worst_f1, df / (EPS * f1))
            assert da <= (4 * T + 32) * EPS, (L, kind, d, da / EPS)
            assert df <= 8 * EPS * f1, (L, kind, d, df / EPS)
    print("rows %d compared %d worst auc %.2f T 2^-53, worst f1 %.2f 2^-53 relative" % (total, compared, worst_auc, worst_f1))
    assert compared * 4 >= total * 3


def test_hit_rank_is_n_error():
    rng = np.random.default_rng(7)
    for L in (3, 7, 65, 391):
        # rows whose three highest scores are distinct: the host's unstable argsort has one answer
        s = rankref.gen_scores(rng, "distinct", 40, L)
        y = rankref.gen_truth(rng, 40, L)
        hit = rankref.rank_rows(s, y, first=0, top_n=0)["hit_rank"]
        for n in (1, 2):
            assert evaluate.n_error(s, y, n) == int(((hit > 0) & (hit <= n)).sum()) / 40
        # tied rows: the rule is the stable order
        s = rankref.gen_scores(rng, "grid", 40, L)
        hit = rankref.rank_rows(s, y, first=0, top_n=0)["hit_rank"]
        for d in range(40):
            yo = y[d][np.argsort(-s[d], kind="stable")]
            assert hit[d] == (int(np.argmax(yo)) + 1 if yo.any() else 0)


def test_rank_labels_validates_arguments():
    """NULL score, K = 0, K = 7 689, first = K, ld < K, top_n = 17 and a negative D are refused before anything touches HIP; the
    struct is the size the library was compiled with and the ABI number has not moved."""
    from lda_thesis_amd import _native
    L = _native.lib()
    assert L.llda_abi_version() == 22
    assert L.llda_struct_size(4) == ctypes.sizeof(_native.LldaRankArgs)
    assert "llda_rank_labels" in _native.EXPORTS

    def call(**kw):
        a = _native.LldaRankArgs()
        a.score, a.D, a.ld, a.K, a.first, a.top_n = 4096, 1, 8, 8, 1, 5       # (a fake pointer: never dereferenced on the host)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.llda_rank_labels(ctypes.byref(a), None)

    assert L.llda_rank_labels(None, None) == -2
    assert call(score=None) == -2
    assert call(K=0, first=0) == -1
    assert call(K=7689, ld=7689) == -1
    assert call(first=8) == -2
    assert call(first=-1) == -2
    assert call(ld=7) == -2
    assert call(top_n=17) == -2
    assert call(top_n=-1) == -2
    assert call(D=-1) == -2
    assert call(score=4100) == -2                                              # not 8-byte aligned
    assert call(D=0, score=None) == 0                                          # nothing to rank
