"""Distinctive words on the drop-in class: ``LabeledLDA.label_words`` against the numpy restatement (tests/scoredref.py) on the
model's own counts and running mean, bit for bit; lam = 1 is ``top_words``; ``coherence`` / ``window_coherence`` / ``topwords_per_topic``
with ``lam`` equal the host functions on those id tables and are untouched without it; the harness options."""
import numpy as np
import pytest

from test_gpu_rank_labels import _model, _write_csv
from test_gpu_topics_dropin import corpus_of, trained
from test_gpu_window_dropin import texts_of
import scoredref
import topicref
import windowref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["k12", "k392"])
def model(request):
    return trained(request.param)


@pytest.fixture(scope="module")
def averaged():
    """the k12 model after run_training(4, 2): ph_hat is the mean of two read-outs"""
    return _model("k12")[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("lam,min_count", [(0.6, 1), (0, 1), (0.5, 3), (0.3, 1), (1, 1), (1, 0)])
def test_label_words_equal_the_restatement_on_the_counts(model, lam, min_count):
    m = model
    idx, sc = m.label_words(10, lam, min_count)
    assert idx.shape == sc.shape == (m.K, 10) and idx.dtype == np.int32 and sc.dtype == np.float64
    want_idx, want_sc = scoredref.label_words_ref(m.n_k_v, m.beta, 10, lam, min_count)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(sc), bits(want_sc))
    assert (idx >= 0).any()
    if (lam, min_count) == (0.6, 1):
        assert np.array_equal(m.label_words()[0], idx)                                   # the defaults


def test_lam_one_without_a_minimum_count_is_top_words(model):
    m = model
    for n in (1, 10, 16):
        idx, sc = m.label_words(n, 1, 0)
        top, _ = m.top_words(n)
        assert np.array_equal(idx, top)
        phi = m.get_phi()
        for k in range(m.K):
            assert np.array_equal(bits(sc[k]), bits(phi[k, top[k]]))
    with pytest.raises(ValueError):
        m.label_words(17)
    with pytest.raises(ValueError):
        m.label_words(10, 1.5)
    with pytest.raises(ValueError):
        m.label_words(10, source="theta")


def test_ranking_the_running_mean(model, averaged):
    for m in (model, averaged):                      # before the first read-out ph_hat stands for the current phi
        ph = m.ph_hat if m.cur_perplx else m.get_phi()
        for n in (10, 16):
            idx, sc = m.label_words(n, 1, 0, source="ph_hat")
            for k in range(m.K):
                want = np.argsort(-ph[k], kind="stable")[:n]
                assert np.array_equal(idx[k], want), k
                assert np.array_equal(bits(sc[k]), bits(ph[k, want]))
    m = averaged
    assert m.cur_perplx and not np.array_equal(m.ph_hat, m.get_phi())
    a, b = scoredref.relevance_powers_ref(0.6)
    wdiv = scoredref.word_divisor_ref(m.n_k_v.sum(axis=0), b, 2)
    want = scoredref.scored_words_ref(np.ascontiguousarray(m.ph_hat.T), 10, a, wdiv)
    idx, sc = m.label_words(10, 0.6, 2, source="ph_hat")
    assert np.array_equal(idx, want[0]) and np.array_equal(bits(sc), bits(want[1]))


def test_coherence_of_the_distinctive_lists(model):
    from lda_thesis_amd import topics
    m = model
    before_u, before_v = m.coherence(10, "umass"), m.window_coherence(texts_of(m), 10, "c_v")
    idx, _ = m.label_words(10, 0.5, 2)
    doc_off, word = corpus_of(m)
    co = topicref.cooc_ref(doc_off, word, idx)
    D = len(doc_off) - 1
    assert same(m.coherence(10, "umass", lam=0.5, min_count=2), topics.umass(co, listed=idx))
    assert same(m.coherence(10, "npmi", lam=0.5, min_count=2), topics.npmi(co, D, listed=idx))
    tok_off, tok = topics.token_csr(texts_of(m), m.dicti.token2id)
    for measure, window in (("c_v", None), ("c_npmi", 5)):
        s = topics.DEFAULT_WINDOW[measure] if window is None else window
        wco, N = windowref.window_ref(tok_off, tok, idx, s), windowref.window_count_ref(tok_off, s)
        assert same(m.window_coherence(texts_of(m), 10, measure, window, lam=0.5, min_count=2), getattr(topics, measure)(wco, N, listed=idx))
    # lam = None: what it was
    top, _ = m.top_words(10)
    assert same(m.coherence(10, "umass"), before_u) and same(m.coherence(10, "umass", None, None), before_u)
    assert same(before_u, topics.umass(topicref.cooc_ref(doc_off, word, top), listed=top))
    assert same(m.window_coherence(texts_of(m), 10, "c_v", lam=None), before_v)
    with pytest.raises(ValueError):
        m.coherence(10, "c_v", lam=0.5)
    with pytest.raises(ValueError):
        topics.coherence(co, D, "c_v")
    names = list(m.labelmap.keys())
    assert m.topwords_per_topic(10, lam=0.5) == [[names[k]] + [m.v_to_w[int(v)] for v in m.label_words(10, 0.5)[0][k] if v >= 0]
                                                 for k in range(m.K)]
    assert m.topwords_per_topic(10, device=True, lam=None) == [[names[k]] + [m.v_to_w[int(v)] for v in top[k]] for k in range(m.K)]


def test_harness_options(tmp_path, capsys, monkeypatch):
    from lda_thesis_amd import evaluate_LabeledLDA as H
    opt, _ = H.build_parser().parse_args(["-f", "x.csv", "-i", "2"])
    assert opt.label_words == 0 and opt.relevance == 0.6               # off by default: the report is what it was
    opt, _ = H.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--label-words", "7", "--relevance", "0.5"])
    assert opt.label_words == 7 and opt.relevance == 0.5
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    np.random.seed(0)
    H.main(["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5", "--label-words", "4", "--relevance", "0.5", "--coherence", "4",
            "--window-coherence", "4"])
    out = capsys.readouterr().out.splitlines()
    at = out.index("Label words (top 4): most frequent | most distinctive (relevance 0.5):")
    rows = [line for line in out[at + 1:] if " | " in line]
    assert len(rows) >= 8 and rows[0].split()[0] == "root"
    for line in rows:                                                  # both lists, four words each
        left, right = line.split(" | ")
        assert len(left.split()) == 5 and len(right.split()) == 4
    assert any(line.split(" | ")[0].split()[1:] != line.split(" | ")[1].split() for line in rows)
    assert any(line.startswith("UMass coherence (top 4 words), mean: frequent ") and ", distinctive " in line for line in out[at:])
    assert any(line.startswith("C_V coherence (top 4 words), mean: frequent ") and ", distinctive " in line for line in out[at:])
