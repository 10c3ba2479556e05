"""The left-to-right estimate through the drop-in class (LabeledLDA.left_to_right) on the tiny_k12 model after run_training, against
the CPU restatement (tests/leftrightref.py), and the harness's --left-to-right end to end."""
import functools

import numpy as np
import pytest

import leftrightref as ref

pytestmark = pytest.mark.gpu

R = 3


@functools.lru_cache(maxsize=None)
def trained():
    from test_gpu_rank_labels import _model
    m, docs, labs = _model("k12")
    docs = [list(d)[:24] for d in docs[:12]] + [["no-such-token"], []]
    return m, docs, [list(l) for l in labs[:12]] + [[], []]


@functools.lru_cache(maxsize=None)
def plain():
    m, docs, _ = trained()
    return m.left_to_right(docs, particles=R)


def _want(m, docs, labels=None, max_tokens=None):
    from lda_thesis_amd import heldout, leftright
    t2i = m.dicti.token2id
    lists, keep = leftright.prepare_tokens([[t2i[x] for x in doc if x in t2i] for doc in docs], max_tokens)
    allowed = None if labels is None else leftright.allowed_matrix([labels[d] for d in keep], m.labelmap, m.K)
    doc_off, word = leftright.tokens_csr(lists)
    mant, expo, tok, bad, _ = ref.left_to_right_ref(np.ascontiguousarray(m.ph_hat.T), doc_off, word, m.alpha, R, m.seed,
                                                    leftright.LR_STREAM, allowed=allowed)
    r = heldout.perplexity_from(mant, expo, tok, bad)
    return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=len(docs) - len(keep),
                bad=r["bad"])


def test_left_to_right_equals_the_restatement():
    m, docs, _ = trained()
    got = plain()
    assert got == _want(m, docs)
    assert got["skipped"] == 2 and got["documents"] == 12 and got["bad"] == 0 and got["tokens"] > 0
    assert 1.0 < got["perplexity"] < len(m.dicti)
    assert m.left_to_right(docs, particles=R) == got                    # the same call twice


def test_labels_restrict_the_topics():
    m, docs, labs = trained()
    got = m.left_to_right(docs, particles=R, labels=labs)
    assert got == _want(m, docs, labels=labs) and got != plain()
    with pytest.raises(KeyError):
        m.left_to_right(docs, particles=R, labels=[["no-such-label"]] * len(docs))


def test_seed_and_truncation():
    m, docs, _ = trained()
    other = m.left_to_right(docs, particles=R, seed=m.seed + 1)
    assert other != plain() and other["tokens"] == plain()["tokens"]
    short = m.left_to_right(docs, particles=R, max_tokens=5)
    assert short == _want(m, docs, max_tokens=5) and short["tokens"] <= 5 * 12


def test_cli_left_to_right(tmp_path, capsys, monkeypatch):
    """--left-to-right 4 prints its two lines behind the report and changes nothing before them"""
    from lda_thesis_amd import evaluate_LabeledLDA as H
    from test_gpu_rank_labels import _write_csv
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv)
    before = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    H.main(argv + ["--left-to-right", "4"])
    out = capsys.readouterr().out.splitlines()
    assert out[:len(before)] == before and before[-1].startswith("F1 score (macro average) ")
    extra = out[len(before):]
    assert len(extra) == 3 and extra[0] == "-----------------------------------"
    assert extra[1].startswith("Held-out perplexity (left-to-right, 4 particles): ") and float(extra[1].split()[-1]) > 1.0
    assert extra[2].startswith("  scored tokens ")
