"""The sparse-label estimators through the drop-in class on the tiny_k12 corpus: LabeledLDA.left_to_right(labels=..., sparse=True) and
heldout_perplexity_em(labels=..., sparse=True) against tests/sparseheldref.py, a model of K = 1100 that only the sparse form can
score, prefix label sets where sparse and dense agree to the bit, fit_em's two traces, and the harness's two flags end to end."""
import functools
import math

import numpy as np
import pytest

import emref
import heldoutref
import sparseheldref
import sparseref
from test_gpu_fit_em_sparse_dropin import CHUNK, ITERS, csr, model_with

pytestmark = pytest.mark.gpu

R = 3


@functools.lru_cache(maxsize=None)
def fitted():
    """tiny_k12 after two EM passes; its first documents as held-out text, with scattered label lists of none .. three labels"""
    from test_gpu_dropin import build_model
    m, _, _ = build_model("k12")
    m.fit_em(2, chunk=CHUNK)
    names = sorted(m.labelmap, key=m.labelmap.get)
    assert names[0] == "root" and len(names) == m.K
    docs = [[m.v_to_w[w] for w, f in t for _ in range(f)] for t in m.doc_tups[:12]] + [["no-such-token"], []]
    labels = [[names[1 + (5 * d + 3 * j) % (m.K - 1)] for j in range(d % 4)] for d in range(14)]
    prefix = [names[1:1 + d % 4] for d in range(14)]
    return m, docs, labels, prefix


def cols_of(m, labels):
    return [[0] + sorted(set(int(m.labelmap[x]) for x in labs) - {0}) for labs in labels]


def want_left_to_right(m, docs, labels, particles=R):
    from lda_thesis_amd import docmodel, heldout, leftright
    t2i = m.dicti.token2id
    lists, keep = leftright.prepare_tokens([[t2i[x] for x in doc if x in t2i] for doc in docs], None)
    lab_off, lab = docmodel.label_csr(cols_of(m, [labels[d] for d in keep]), K=m.K)
    doc_off, word = leftright.tokens_csr(lists)
    mant, expo, tok, bad, _ = sparseheldref.left_to_right_sparse_ref(np.ascontiguousarray(m.ph_hat.T), doc_off, word, lab_off, lab, m.alpha,
                                                                     particles, m.seed, leftright.LR_STREAM)
    r = heldout.perplexity_from(mant, expo, tok, bad)
    return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=len(docs) - len(keep),
                bad=r["bad"])


def test_left_to_right_sparse_equals_the_restatement():
    m, docs, labels, prefix = fitted()
    got = m.left_to_right(docs, particles=R, labels=labels, sparse=True)
    assert got == want_left_to_right(m, docs, labels)
    assert got["skipped"] == 2 and got["documents"] == 12 and got["tokens"] > 0 and math.isfinite(got["loglik"])
    assert m.left_to_right(docs, particles=R, labels=labels, sparse=True) == got                    # the same call twice
    dense = m.left_to_right(docs, particles=R, labels=labels)
    assert dense["tokens"] + dense["bad"] == got["tokens"] + got["bad"] and abs(dense["loglik"] / got["loglik"] - 1) < 0.2
    with pytest.raises(ValueError):
        m.left_to_right(docs, particles=R, sparse=True)                  # no label sets given
    with pytest.raises(KeyError):
        m.left_to_right(docs, particles=R, labels=[["no-such-label"]] * len(docs), sparse=True)


def test_prefix_label_sets_score_the_same_bits_sparse_and_dense():
    m, docs, _, prefix = fitted()
    a = m.left_to_right(docs, particles=R, labels=prefix, sparse=True)
    assert a == m.left_to_right(docs, particles=R, labels=prefix) and a["tokens"] > 0
    b = m.heldout_perplexity_em(docs, iters=5, labels=prefix, sparse=True)
    assert b == m.heldout_perplexity_em(docs, iters=5, labels=prefix, sparse=False) and b["tokens"] > 0 and b["documents"] == 12


def test_a_model_of_1100_topics_is_scored_by_the_sparse_form_only():
    from lda_thesis_amd import _native
    pick = lambda d, ls: sorted(set([ls[(7 * d) % len(ls)], ls[(13 * d + 5) % len(ls)], ls[-1 - d % 3]]))
    m = model_with(pick, n_labels=1099)
    assert m.K == 1100 > _native.LR_MAX_K
    m.fit_em(1, sparse=True)
    docs = [[m.v_to_w[w] for w, f in t for _ in range(f)][:20] for t in m.doc_tups[:8]]
    labels = [pick(d, sorted(set(m.labelmap) - {"root"}, key=m.labelmap.get)) for d in range(8)]
    got = m.left_to_right(docs, particles=R, labels=labels, sparse=True)
    assert got["documents"] == 8 and got["bad"] == 0 and got["tokens"] > 0 and math.isfinite(got["perplexity"]) and got["perplexity"] > 1.0
    assert got == want_left_to_right(m, docs, labels)
    with pytest.raises(_native.NativeError):
        m.left_to_right(docs, particles=R, labels=labels)


def test_more_than_32_labels_are_refused():
    m = model_with(lambda d, ls: ls[:2], n_labels=40)
    m.fit_em(1)
    names = sorted(set(m.labelmap) - {"root"}, key=m.labelmap.get)
    docs = [[m.v_to_w[w] for w, _ in t] for t in m.doc_tups[:2]]
    with pytest.raises(ValueError):
        m.left_to_right(docs, particles=R, labels=[names[:32], names[:1]], sparse=True)        # root + 32
    with pytest.raises(ValueError):
        m.heldout_perplexity_em(docs, iters=2, labels=[names[:32], names[:1]], sparse=True)
    assert m.left_to_right(docs, particles=R, labels=[names[:31], names[:1]], sparse=True)["tokens"] > 0


def test_heldout_perplexity_em_sparse_equals_the_restatement():
    from lda_thesis_amd import heldout
    m, docs, labels, _ = fitted()
    tups = [m.dicti.doc2bow(x) for x in docs]
    phi_t = np.ascontiguousarray(m.ph_hat.T)
    for weighted in (True, False):
        got = m.heldout_perplexity_em(docs, iters=6, labels=labels, sparse=True, weighted=weighted)
        want = sparseheldref.heldout_perplexity_em_ref(phi_t, tups, cols_of(m, labels), m.alpha, 6, weighted=weighted)
        s = heldout.perplexity_from(want["mant"], want["expo"], [want["tokens"]], [want["bad"]])
        assert (got["loglik"], got["tokens"], got["documents"], got["skipped"]) == (s["loglik"], want["tokens"], 12, 2)
        assert got["perplexity"] == s["perplexity"] and got["tokens"] > 0 and 1.0 < got["perplexity"] < len(m.dicti)
    assert m.heldout_perplexity_em(docs, iters=6, labels=labels, sparse=True, weighted=False) == got           # no random numbers
    dense = m.heldout_perplexity_em(docs, iters=6, labels=labels, weighted=False)
    assert dense["tokens"] == got["tokens"] and abs(dense["loglik"] - got["loglik"]) < 1e-9 * abs(got["loglik"])
    free = m.heldout_perplexity_em(docs, iters=6)
    assert free["tokens"] >= dense["tokens"] and free["documents"] == 12 and math.isfinite(free["perplexity"])


def test_fit_em_traces():
    """sparse_trace=True: the numbers of loglik_sparse_ref on the slots; the default: those of llda_heldout_loglik on the scattered
    loads, exactly as before"""
    from lda_thesis_amd import docmodel, heldout
    from test_gpu_dropin import build_model
    a, _, _ = build_model("k12")
    b, _, _ = build_model("k12")
    doc_off, word, freq = csr(a)
    th0, phi_t0 = a.get_theta(), np.ascontiguousarray(a.get_phi().T)
    lab_off, lab = docmodel.label_csr(a.labs)
    ra = a.fit_em(ITERS, chunk=CHUNK, trace_every=1, sparse=True, sparse_trace=True)
    rb = b.fit_em(ITERS, chunk=CHUNK, trace_every=1, sparse=True)
    want_sparse, want_dense = [], []

    def each(it, th_s, ph):
        s = heldout.perplexity_from(*sparseheldref.loglik_sparse_ref(th_s, ph, doc_off, word, freq, lab_off, lab))
        d = heldout.perplexity_from(*heldoutref.loglik_ref(sparseref.scatter(th_s, lab_off, lab, a.K), ph, doc_off, word, freq))
        want_sparse.append((it, s["loglik"], s["tokens"], s["bad"]))
        want_dense.append((it, d["loglik"], d["tokens"], d["bad"]))

    sparseref.fit_sparse_ref(sparseref.gather(th0, lab_off, lab), phi_t0, doc_off, word, freq, lab_off, lab, a.alpha, a.beta, ITERS,
                             chunk=CHUNK, each=each)
    assert ra["trace"] == want_sparse and rb["trace"] == want_dense and len(want_sparse) == ITERS
    np.testing.assert_allclose([t[1] for t in ra["trace"]], [t[1] for t in rb["trace"]], rtol=1e-12)
    assert np.array_equal(a.th_hat, b.th_hat) and np.array_equal(a.ph_hat, b.ph_hat)                 # the trace does not touch the fit
    with pytest.raises(ValueError):
        b.fit_em(1, sparse_trace=True)                                   # the dense fit has no slots to score


def test_cli_lr_sparse_and_heldout_em(tmp_path, capsys, monkeypatch):
    """--lr-sparse and --heldout-em print their lines behind the report and change nothing before them"""
    from lda_thesis_amd import evaluate_LabeledLDA as H
    from test_gpu_rank_labels import _write_csv
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5", "--em-train", "3", "--em-sparse"]
    np.random.seed(0)
    H.main(argv)
    before = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    H.main(argv + ["--left-to-right", "4", "--lr-sparse", "--heldout-em", "5"])
    out = capsys.readouterr().out.splitlines()
    assert out[:len(before)] == before and before[-1].startswith("F1 score (macro average) ")
    extra = out[len(before):]
    assert len(extra) == 6 and extra[0] == extra[3] == "-----------------------------------"
    assert extra[1].startswith("Held-out perplexity (left-to-right, own labels, 4 particles): ") and 1.0 < float(extra[1].split()[-1]) < 1e6
    assert extra[2].startswith("  scored tokens ") and extra[5].startswith("  scored tokens ")
    assert extra[4].startswith("Held-out perplexity (document completion, EM fold-in of 5 steps, own labels): ")
    assert 1.0 < float(extra[4].split()[-1]) < 1e6
    np.random.seed(0)
    H.main(argv[:-1] + ["--heldout-em", "5"])                           # without --em-sparse: the dense route, every topic
    dense = capsys.readouterr().out.splitlines()
    assert dense[-2].startswith("Held-out perplexity (document completion, EM fold-in of 5 steps): ") and 1.0 < float(dense[-2].split()[-1]) < 1e6
