"""Label-wise evaluation and tuned label sets end to end on the smallest trained toy model: LabeledLDA.label_report, tune_thresholds,
predict_sets and score_test_sets equal the CPU restatement (tests/labelref.py) applied to run_test's loads; the pickle of an untuned
model is what it was and a tuned one round-trips its thresholds; both flags of the harness run."""
import pickle

import numpy as np
import pytest

import labelref
from test_gpu_rank_labels import _model, _write_csv

pytestmark = pytest.mark.gpu

IT, THIN, SEED = 6, 2, 77


@pytest.fixture(scope="module")
def toy():
    from lda_thesis_amd.evaluate import binary_yreal
    m, docs, labs = _model("k12")
    keys_before = set(pickle.loads(pickle.dumps(m)).__dict__)      # before any tuning
    th = m.run_test(docs, IT, THIN, seed=SEED)
    return m, docs, labs, th, binary_yreal(labs, m.labelmap), keys_before


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(np.where(np.isnan(a), -7.0, a), np.where(np.isnan(b), -7.0, b))


def test_label_report(toy):
    from lda_thesis_amd import labelwise
    m, docs, labs, th, y, _ = toy
    want = labelref.label_metrics(th, y, first=1)
    r = m.label_report(docs, labs, IT, THIN, seed=SEED)
    names = list(m.labelmap.keys())[1:]
    assert [row[0] for row in r["table"]] == names
    assert [row[1] for row in r["table"]] == list(want["n_pos"])
    for i, key in ((2, "auc"), (3, "f1"), (4, "thr")):
        assert same([row[i] for row in r["table"]], want[key]), key
    ref_macro = labelwise.macro(want)
    for k in ("macro_auc", "macro_f1", "n_labels", "skipped"):
        assert same(r[k], ref_macro[k]), k
    assert r["n_labels"] + r["skipped"] == len(names) and r["n_labels"] > 0


def test_tuned_sets(toy):
    from lda_thesis_amd import labelwise
    m, docs, labs, th, y, keys_before = toy
    with pytest.raises(ValueError, match="tune_thresholds"):
        m.predict_sets(docs, IT, THIN, seed=SEED)
    want = labelref.label_metrics(th, y, first=1)
    thr = m.tune_thresholds(docs, labs, IT, THIN, seed=SEED)
    assert thr is m.label_thresholds and thr.shape == (m.K,) and np.isnan(thr[0])
    assert same(thr[1:], want["thr"]) and np.array_equal(np.isnan(thr[1:]), want["n_pos"] == 0)
    names = np.array(list(m.labelmap.keys()))
    for alo in (True, False):
        ref = labelref.label_sets(th, thr, y, first=1, at_least_one=alo)
        got = m.predict_sets(docs, IT, THIN, at_least_one=alo, seed=SEED)
        assert got == [list(names[row]) for row in ref["mask"]]
        assert all("root" not in s for s in got) and (not alo or all(len(s) >= 1 for s in got))
        sc = m.score_test_sets(docs, labs, IT, THIN, at_least_one=alo, seed=SEED)
        assert sc == labelwise.set_scores(ref["tp"], ref["fp"], ref["fn"], ref["n_pred"], ref["n_hit"], ref["n_true"], first=1)
        assert 0 < sc["micro_f1"] <= 1 and 0 < sc["example_f1"] <= 1
    # thresholds tuned on these very documents reach every label's best F1: the macro F1 of the sets (at_least_one off) is their mean
    ref = labelref.label_sets(th, thr, y, first=1, at_least_one=False)
    scored = ref["tp"][1:] + ref["fp"][1:] + ref["fn"][1:] > 0
    assert np.array_equal((2 * ref["tp"][1:] / (2 * ref["tp"][1:] + ref["fp"][1:] + ref["fn"][1:]))[scored], want["f1"][scored])
    # pickles: an untuned model has the keys it always had, a tuned one carries its thresholds
    back = pickle.loads(pickle.dumps(m))
    assert set(back.__dict__) == keys_before | {"label_thresholds"} and "label_thresholds" not in keys_before
    assert same(back.label_thresholds, thr)
    assert back.predict_sets(docs[:5], IT, THIN, seed=SEED) == m.predict_sets(docs[:5], IT, THIN, seed=SEED)
    assert m.predict_sets([], IT, THIN) == []


def test_cli_flags(tmp_path, capsys, monkeypatch):
    from lda_thesis_amd import evaluate_LabeledLDA as H
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv)
    plain = capsys.readouterr().out
    np.random.seed(0)
    H.main(argv + ["--label-report", "--label-sets"])
    out = capsys.readouterr().out
    tail = lambda text: text[text.index("Model:               Labeled LDA"):].splitlines()
    a, b = tail(plain), tail(out)
    assert len(a) == 9 and b[:9] == a                             # both default off; the existing report's text is unchanged
    extra = "\n".join(b[9:])
    for line in ("Label-wise evaluation over", "AUC ROC (macro over labels):", "best F1 (macro over labels):", "ten best labels by AUC",
                 "ten worst labels by AUC", "Label sets:", "F1 (micro):", "F1 (macro over labels):", "F1 (example-based):"):
        assert line in extra, line
    value = lambda tag: float([x for x in extra.splitlines() if x.startswith(tag)][0][len(tag):])
    assert 0 <= value("AUC ROC (macro over labels):") <= 1 and 0 <= value("F1 (micro):") <= 1
    help_text = "".join(H.build_parser().format_help().split())   # (the formatter may wrap at a hyphen)
    assert "even-indexed" in help_text and "odd-indexed" in help_text and "--label-report" in help_text
