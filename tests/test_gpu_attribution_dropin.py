"""Credit attribution through the drop-in class (LabeledLDA.word_credit, fold_in_em, predict_em, explain) on the tiny_k12 model
after run_training, against the CPU restatement (tests/attrref.py), and the harness's --em-foldin / --explain end to end."""
import functools

import numpy as np
import pytest

import attrref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def trained():
    from test_gpu_rank_labels import _model
    m, docs, labs = _model("k12")
    docs = [list(d) for d in docs[:30]]
    return m, docs, [list(l) for l in labs[:30]]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def csr(m, tups):
    from lda_thesis_amd.corpus import csr_from_doc_tups
    return csr_from_doc_tups(tups)


def test_word_credit_equals_attrref_and_stays_inside_the_labels():
    m, _, _ = trained()
    got = m.word_credit(top_m=2)
    th, ph = m.th_hat, m.ph_hat                                           # downloaded after the call: the same bits
    doc_off, word, freq = csr(m, m.doc_tups)
    want = attrref.attribute_ref(th, np.ascontiguousarray(ph.T), doc_off, word, freq, top_m=2)
    assert np.array_equal(bits(got["credit"]), bits(want["credit"]))
    assert len(got["labels"]) == len(got["shares"]) == m.D
    for d in range(m.D):
        a, b = int(doc_off[d]), int(doc_off[d + 1])
        assert got["labels"][d].shape == (b - a, 2) and got["labels"][d].dtype == np.int32
        assert np.array_equal(got["labels"][d], want["site_idx"][a:b]) and np.array_equal(bits(got["shares"][d]), bits(want["site_val"][a:b]))
        allowed = m.labs[d] != 0
        assert (got["credit"][d][~allowed] == 0.0).all()                  # nothing outside the document's labels
        ids = got["labels"][d]
        assert allowed[ids[ids >= 0]].all()
    assert (want["bad"] == 0).all() and np.abs(got["credit"].sum(axis=1) - want["tok"]).max() < 1e-11
    assert np.array_equal(bits(m.word_credit(top_m=2)["credit"]), bits(got["credit"]))       # and again, th_hat / ph_hat on the host
    for top_m in (0, 5):
        with pytest.raises(ValueError):
            m.word_credit(top_m=top_m)


def test_fold_in_em_is_deterministic_and_equals_attrref():
    m, docs, labs = trained()
    th = m.fold_in_em(docs, iters=7)
    assert th.shape == (len(docs), m.K) and th.dtype == np.float64
    assert np.array_equal(bits(m.fold_in_em(docs, iters=7)), bits(th))
    seed = m.seed
    try:
        m.seed = seed + 1                                                # no random numbers: the model's seed reaches nothing
        assert np.array_equal(bits(m.fold_in_em(docs, iters=7)), bits(th))
    finally:
        m.seed = seed
    from lda_thesis_amd import attribution
    tups = [m.dicti.doc2bow(x) for x in docs]
    doc_off, word, freq = csr(m, tups)
    phi_t = np.ascontiguousarray(m.ph_hat.T)
    want = attrref.attribute_ref(attribution.uniform_start(None, len(docs), m.K), phi_t, doc_off, word, freq, iters=7, alpha=m.alpha)
    assert np.array_equal(bits(th), bits(want["theta_out"]))
    assert np.abs(th.sum(axis=1) - 1.0).max() < 1e-13
    # with label sets: loads only on root and the document's labels
    th_l = m.fold_in_em(docs, iters=7, labels=labs)
    cols = [[0] + sorted(m.labelmap[x] for x in set(l)) for l in labs]
    want = attrref.attribute_ref(attribution.uniform_start(cols, len(docs), m.K), phi_t, doc_off, word, freq, iters=7, alpha=m.alpha)
    assert np.array_equal(bits(th_l), bits(want["theta_out"]))
    for d, c in enumerate(cols):
        assert (np.delete(th_l[d], c) == 0.0).all() and (th_l[d][c] > 0.0).all()
    with pytest.raises(ValueError, match="no in-vocabulary word"):
        m.fold_in_em(docs[:2] + [["no-such-token"]], iters=2)


def test_predict_em_has_the_shape_of_predict():
    m, docs, _ = trained()
    a, b = m.predict(docs, 4, 2, n=5, seed=7), m.predict_em(docs, iters=5, n=5)
    assert len(a) == len(b) == len(docs)
    th = m.fold_in_em(docs, iters=5)
    names = list(m.labelmap.keys())
    for d, (x, y) in enumerate(zip(a, b)):
        assert len(x) == len(y) == 5
        assert all(type(p[0]) is type(q[0]) and type(p[1]) is type(q[1]) for p, q in zip(x, y))
        assert [float(v) for _, v in y] == sorted(th[d].tolist(), reverse=True)[:5]
        assert all(th[d][names.index(str(lab))] == v for lab, v in y)


def test_explain_shares_sum_to_one():
    m, docs, labs = trained()
    for kw in (dict(labels=[l[:3] for l in labs]), dict(n=3), dict(n=1)):
        out = m.explain(docs, iters=6, **kw)
        assert len(out) == len(docs)
        for d, (words, credit) in enumerate(out):
            tups = m.dicti.doc2bow(docs[d])
            assert [(t, f) for t, f, _ in words] == [(m.v_to_w[w], f) for w, f in tups]
            assert "root" in credit or not credit
            size = len(set(labs[d][:3])) + 1 if "labels" in kw else kw["n"] + 1
            assert len(credit) <= size <= 4
            for token, f, shares in words:
                assert 1 <= len(shares) <= size and set(lab for lab, _ in shares) <= set(credit)
                assert abs(sum(s for _, s in shares) - 1.0) <= 1e-12      # the whole set fits into four places
                assert [s for _, s in shares] == sorted((s for _, s in shares), reverse=True)
            assert abs(sum(credit.values()) - sum(f for _, f, _ in words)) < 1e-10
    with pytest.raises(ValueError):
        m.explain(docs, n=4)
    assert m.explain([]) == []


def test_cli_em_foldin_and_explain(tmp_path, capsys, monkeypatch):
    """--em-foldin 5 --explain 2 print their lines behind the report and change nothing before them"""
    from lda_thesis_amd import evaluate_LabeledLDA as H
    from test_gpu_rank_labels import _write_csv
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv)
    plain = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    H.main(argv + ["--em-foldin", "5", "--explain", "2"])
    out = capsys.readouterr().out.splitlines()
    assert out[:len(plain)] == plain and plain[-1].startswith("F1 score (macro average) ")
    extra = out[len(plain):]
    assert extra[0] == "-----------------------------------" and extra[1] == "EM fold-in, 5 steps (no random numbers):"
    for line, label in zip(extra[2:6], ("AUC ROC:", "one error:", "two error:", "F1 score (macro average)")):
        assert line[:25].strip() == label and 0.0 <= float(line[25:]) <= 1.0
    assert extra[6] == "-----------------------------------" and extra[7] == "Credit attribution of the first 2 test documents:"
    assert [x for x in extra[8:] if x.startswith("document ")][0].startswith("document 0: ")
    assert len([x for x in extra[8:] if x.startswith("document ")]) == 2
    label_lines = [x for x in extra[8:] if x.startswith("  ")]
    assert label_lines and all(len(x.split()) >= 3 for x in label_lines)  # label, credited tokens, at least one word
