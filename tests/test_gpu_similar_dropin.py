"""Nearest rows through the drop-in class (LabeledLDA.similar_documents / similar_labels / predict_knn / score_test_knn) on the tiny_k12
model after run_training, against the CPU restatement (tests/nearref.py) on the downloaded matrices, and the harness's --knn and
--similar-labels end to end."""
import functools

import numpy as np
import pytest

import nearref as ref
import rankref

pytestmark = pytest.mark.gpu

IT, THIN, SEED = 6, 2, 77


@functools.lru_cache(maxsize=None)
def trained():
    from test_gpu_rank_labels import _model
    m, docs, labs = _model("k12")
    theta = m._th_hat.dev.cpu().numpy()                                 # (the running mean stays on the device: a copy, not the property)
    return m, [list(d) for d in docs[:7]], [list(l) for l in labs[:7]], theta


@functools.lru_cache(maxsize=None)
def corpus_scores_of_training_queries():
    m, _, _, theta = trained()
    ids = np.array([0, 3, m.D - 1, 3], dtype=np.int64)
    root = np.sqrt(theta)
    return ids, ref.scores(root[ids], root)


@functools.lru_cache(maxsize=None)
def heldout_queries():
    m, docs, _, theta = trained()
    loads = m.run_test(docs, IT, THIN, seed=SEED)
    return loads, ref.scores(np.sqrt(loads), np.sqrt(theta))


def _same(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(np.asarray(got[1]).view(np.uint64), want[1].view(np.uint64))


def test_training_documents_never_return_themselves():
    m, _, _, theta = trained()
    ids, sc = corpus_scores_of_training_queries()
    got = m.similar_documents(doc_ids=ids, n=5)
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == (4, 5)
    _same(got, ref.select(sc, 5, 0, ids)[:2])
    assert not np.any(got[0] == ids[:, None])
    assert np.array_equal(got[0][1], got[0][3])                         # the same query twice
    with pytest.raises(ValueError):
        m.similar_documents()
    with pytest.raises(ValueError):
        m.similar_documents(newdocs=[["x"]], doc_ids=[0])
    with pytest.raises(ValueError):
        m.similar_documents(doc_ids=[m.D])
    with pytest.raises(ValueError):
        m.similar_documents(doc_ids=[0], n=17)
    with pytest.raises(ValueError):
        m.similar_documents(doc_ids=[0], measure="jensen-shannon")


def test_heldout_queries_equal_the_restatement_on_run_test_loads():
    m, docs, _, _ = trained()
    _, sc = heldout_queries()
    for n in (1, 10, 16):
        _same(m.similar_documents(newdocs=docs, n=n, it=IT, thinning=THIN, seed=SEED), ref.select(sc, n)[:2])
    idx, val = m.similar_documents(newdocs=[], n=3)
    assert idx.shape == (0, 3) and val.shape == (0, 3)


def test_corpus_in_row_ranges_merged_equals_the_unsplit_call():
    import torch
    from lda_thesis_amd import similar
    m, _, _, theta = trained()
    loads, sc = heldout_queries()
    dev = m._sampler.device
    q = similar.affinity_rows(torch.from_numpy(loads).to(dev))
    b = similar.affinity_rows(torch.from_numpy(theta).to(dev))
    whole = similar.nearest_rows(q, b, 10)
    _same((whole[0].cpu().numpy(), whole[1].cpu().numpy()), ref.select(sc, 10)[:2])
    D = theta.shape[0]
    for cuts in ((0, D // 2, D), (0, 1, D - 2, D)):
        parts = [similar.nearest_rows(q, b[lo:hi], 10, row_base=lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
        merged = similar.merge_lists([p[0].cpu().numpy() for p in parts], [p[1].cpu().numpy() for p in parts], 10)
        _same(merged, (whole[0].cpu().numpy(), whole[1].cpu().numpy()))


def test_similar_labels_equal_the_restatement_on_phi():
    m, _, _, _ = trained()
    ph = np.asarray(m._ph_hat.dev.cpu().numpy())                        # after thinning read-outs the rows are ph_hat
    want = ref.select(ref.scores(np.sqrt(ph), np.sqrt(ph)), 3, 0, np.arange(m.K))
    names = list(m.labelmap.keys())
    got = m.similar_labels(3)
    assert [g[0] for g in got] == names
    for k, (_, near) in enumerate(got):
        assert [x for x, _ in near] == [names[j] for j in want[0][k] if j >= 0] and names[k] not in [x for x, _ in near]
        assert [float(v) for _, v in near] == [float(v) for j, v in zip(want[0][k], want[1][k]) if j >= 0]
    other = m.similar_labels(2, measure="cosine")
    assert len(other) == m.K and all(len(near) == 2 for _, near in other)


def test_predict_knn_and_score_test_knn_equal_votes_and_rankref():
    from lda_thesis_amd import similar
    from lda_thesis_amd.evaluate import binary_yreal
    m, docs, labs, _ = trained()
    _, sc = heldout_queries()
    K = 4
    idx, val, _ = ref.select(sc, K)
    votes = similar.knn_votes(idx, val, m.labs, K)
    names = np.array(list(m.labelmap.keys()))
    want = rankref.rank_rows(votes, None, first=0, top_n=5, K=m.K)
    got = m.predict_knn(docs, IT, THIN, k=K, n=5, seed=SEED)
    assert len(got) == len(docs)
    for d, pairs in enumerate(got):
        assert [str(x) for x, _ in pairs] == [str(x) for x in names[want["top_idx"][d][:5]]]
        assert [float(v) for _, v in pairs] == [float(v) for v in want["top_val"][d][:5]]
    truth = binary_yreal(labs, m.labelmap)
    r = rankref.rank_rows(votes, (truth != 0).astype(np.uint8), first=1, top_n=0, K=m.K)
    keep = (r["flags"] & 8) == 0                                        # ALL_ZERO documents are dropped
    hit = r["hit_rank"][keep]
    s = m.score_test_knn(docs, labs, IT, THIN, k=K, seed=SEED)
    assert s["kept"] == int(keep.sum()) and s["dropped"] == len(docs) - int(keep.sum())
    assert s["auc"] == np.mean(r["auc"][keep]) and s["f1"] == np.mean(r["f1"][keep])
    assert s["one_error"] == int(((hit > 0) & (hit <= 1)).sum()) / s["kept"]
    assert s["two_error"] == int(((hit > 0) & (hit <= 2)).sum()) / s["kept"]
    assert m.predict_knn([], IT, THIN) == []
    with pytest.raises(ValueError):
        m.predict_knn(docs, IT, THIN, k=17)


def test_cli_knn_and_similar_labels(tmp_path, capsys, monkeypatch):
    """--knn 3 --similar-labels 2 print their blocks behind the report and change nothing before them"""
    from lda_thesis_amd import evaluate_LabeledLDA as H
    from test_gpu_rank_labels import _write_csv
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv)
    before = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    H.main(argv + ["--knn", "3", "--similar-labels", "2"])
    out = capsys.readouterr().out.splitlines()
    assert out[:len(before)] == before and before[-1].startswith("F1 score (macro average) ")
    extra = out[len(before):]
    assert extra[0] == "-----------------------------------"
    assert extra[1] == "k nearest training documents (k = 3, Hellinger affinity):"
    for line, label in zip(extra[2:6], ("AUC ROC:", "one error:", "two error:", "F1 score (macro average)")):
        assert line[:25].strip() == label and 0.0 <= float(line[25:]) <= 1.0
    assert extra[6] == "-----------------------------------" and extra[7].startswith("Nearest labels by word distribution")
    rows = extra[8:]
    assert len(rows) == 8 and rows[0].split()[0] == "root"             # root and the seven codes of the toy corpus
    for row in rows:
        cells = row.split()
        assert len(cells) == 5 and cells[0] not in (cells[1], cells[3]) and 0.0 <= float(cells[4]) <= float(cells[2]) <= 1.0 + 1e-12
