"""FREX words and topic exclusivity on the drop-in class: ``LabeledLDA.frex_words`` and ``LabeledLDA.exclusivity`` against the
restatement (tests/frexref.py) on the model's own counts and running mean, bit for bit; weight = 1 is the exclusivity order and
weight = 0 the phi order of ``label_words(lam = 1)``; the harness options end to end; ``label_words``, ``top_words`` and ``coherence``
are what they were."""
import numpy as np
import pytest

from test_gpu_rank_labels import _model, _write_csv
from test_gpu_topics_dropin import trained
import frexref
import scoredref

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


def cand_of(m, min_count):
    return m.n_k_v.sum(axis=0) >= max(min_count, 1)


@pytest.mark.parametrize("weight,min_count", [(0.5, 1), (0.7, 1), (0.5, 3), (63 / 64, 1), (1, 1), (0, 2), (0.3, 0)])
def test_frex_words_equal_the_restatement_on_the_counts(model, weight, min_count):
    m = model
    phi_t = frexref.x_of_counts(m.n_k_v, m.beta)
    assert np.array_equal(bits(phi_t.T), bits(m.get_phi()))
    for n in (10, 16):
        idx, fx = m.frex_words(n, weight, min_count)
        assert idx.shape == fx.shape == (m.K, n) and idx.dtype == np.int32 and fx.dtype == np.float64
        want_idx, want_fx = frexref.frex_words_ref(phi_t, n, weight, cand_of(m, min_count))
        assert np.array_equal(idx, want_idx) and np.array_equal(bits(fx), bits(want_fx))
        assert (idx >= 0).any() and np.array_equal(idx < 0, np.isnan(fx)) and np.nanmax(fx) <= 1.0 and np.nanmin(fx) > 0.0
    if (weight, min_count) == (0.5, 1):
        assert np.array_equal(m.frex_words()[0], m.frex_words(10, 0.5, 1)[0])            # the defaults
        assert np.array_equal(m.frex_words(1)[0], m.frex_words(10)[0][:, :1])


def test_the_ends_of_the_weight(model):
    """weight = 1: the exclusivity order; weight = 0: the phi order, which is ``label_words(n, 1)`` -- equal phi share one ECDF rank,
    so ties go by word id there as here"""
    m = model
    phi_t = frexref.x_of_counts(m.n_k_v, m.beta)
    cand = cand_of(m, 1)
    rank_e = frexref.ecdf_ranks_ref(phi_t, m.K, 1, cand)[0]
    words = np.flatnonzero(cand)
    for n in (10, 16):
        idx, fx = m.frex_words(n, 1)
        for k in range(m.K):
            want = words[np.argsort(-rank_e[k, words].astype(np.int64), kind="stable")[:n]]
            assert np.array_equal(idx[k, :len(want)], want), k
        assert np.array_equal(m.frex_words(n, 0)[0], m.label_words(n, 1)[0])
        assert np.array_equal(m.frex_words(n, 0, 3)[0], m.label_words(n, 1, 3)[0])
    for bad in (dict(n=17), dict(n=0), dict(weight=1.5), dict(weight=-0.1), dict(source="theta")):
        with pytest.raises(ValueError):
            m.frex_words(**bad)
        with pytest.raises(ValueError):
            m.exclusivity(**bad)


@pytest.mark.parametrize("weight,min_count", [(0.7, 1), (0.5, 2), (1, 1), (0, 1)])
def test_exclusivity_equals_the_restatement(model, weight, min_count):
    m = model
    phi_t = frexref.x_of_counts(m.n_k_v, m.beta)
    for n in (1, 10, 16):
        ex = m.exclusivity(n, weight, min_count)
        assert ex.shape == (m.K,) and ex.dtype == np.float64
        assert np.array_equal(bits(ex), bits(frexref.exclusivity_ref(phi_t, n, weight, cand_of(m, min_count))))
        assert (ex[~np.isnan(ex)] > 0).all() and (ex[~np.isnan(ex)] <= n).all()
    if (weight, min_count) == (0.7, 1):
        assert np.array_equal(bits(m.exclusivity()), bits(m.exclusivity(10, 0.7, 1)))     # the defaults
    # a minimum count no word reaches: nothing is ranked
    huge = int(m.n_k_v.sum()) + 1
    assert np.isnan(m.exclusivity(10, weight, huge)).all()
    idx, fx = m.frex_words(10, weight, huge)
    assert (idx == -1).all() and np.isnan(fx).all()


def test_the_running_mean(model, averaged):
    for m in (model, averaged):                      # before the first read-out ph_hat stands for the current phi
        ph = m.ph_hat if m.cur_perplx else m.get_phi()
        phi_t = np.ascontiguousarray(ph.T)
        for weight, min_count in ((0.5, 1), (0.7, 2)):
            idx, fx = m.frex_words(10, weight, min_count, source="ph_hat")
            want_idx, want_fx = frexref.frex_words_ref(phi_t, 10, weight, cand_of(m, min_count))
            assert np.array_equal(idx, want_idx) and np.array_equal(bits(fx), bits(want_fx))
            ex = m.exclusivity(10, weight, min_count, source="ph_hat")
            assert np.array_equal(bits(ex), bits(frexref.exclusivity_ref(phi_t, 10, weight, cand_of(m, min_count))))
    m = averaged
    assert m.cur_perplx and not np.array_equal(m.ph_hat, m.get_phi())


def test_batches_change_nothing(model):
    from lda_thesis_amd import topics
    import torch
    m = model
    phi_t = torch.from_numpy(frexref.x_of_counts(m.n_k_v, m.beta)).to("cuda:0")
    cand = cand_of(m, 1)
    whole = topics.frex_words(phi_t, m.K, 10, 0.7, cand, batch=m.K)
    for batch in (1, 5, None):
        got = topics.frex_words(phi_t, m.K, 10, 0.7, cand, batch=batch)
        assert got[3] == whole[3] == int(cand.sum())
        for a, b in zip(got[:3], whole[:3]):
            assert torch.equal(a, b)
    assert topics._frex_batch(5000, 512, 10 ** 12) == 512 and topics._frex_batch(5000, 512, 0) == 1
    assert topics._frex_batch(100000, 512, 2 * 50 * (24 * 102400 + 800000)) == 50


def test_the_other_read_outs_are_what_they_were(model):
    m = model
    before = (m.top_words(10), m.label_words(10, 0.6, 1), m.coherence(10, "umass"), m.coherence(10, "npmi", lam=0.5))
    m.frex_words(10, 0.5)
    m.exclusivity(10, 0.7)
    m.frex_words(16, 0.7, source="ph_hat")
    after = (m.top_words(10), m.label_words(10, 0.6, 1), m.coherence(10, "umass"), m.coherence(10, "npmi", lam=0.5))
    assert same(before[0][0], after[0][0]) and same(before[0][1], after[0][1])
    assert same(before[1][0], after[1][0]) and np.array_equal(bits(before[1][1]), bits(after[1][1]))
    assert same(before[2], after[2]) and same(before[3], after[3])
    want_idx, want_sc = scoredref.label_words_ref(m.n_k_v, m.beta, 10, 0.6, 1)
    assert np.array_equal(after[1][0], want_idx) and np.array_equal(bits(after[1][1]), bits(want_sc))
    phi = m.get_phi()
    for k in range(m.K):
        assert np.array_equal(after[0][0][k], np.argsort(-phi[k], kind="stable")[:10])


def test_harness_options(tmp_path, capsys, monkeypatch):
    from lda_thesis_amd import evaluate_LabeledLDA as H
    opt, _ = H.build_parser().parse_args(["-f", "x.csv", "-i", "2"])
    assert opt.frex_words == 0 and opt.exclusivity == 0 and opt.frex_weight is None    # off by default: the report is what it was
    opt, _ = H.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--frex-words", "7", "--frex-weight", "0.25", "--exclusivity", "5"])
    assert opt.frex_words == 7 and opt.frex_weight == 0.25 and opt.exclusivity == 5
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv + ["--frex-words", "4", "--exclusivity", "4"])
    out = capsys.readouterr().out.splitlines()
    at = out.index("Label words (top 4): most frequent | FREX (weight 0.5):")
    rows = [line for line in out[at + 1:] if " | " in line]
    assert len(rows) >= 8 and rows[0].split()[0] == "root"
    for line in rows:                                                  # both lists, four words each
        left, right = line.split(" | ")
        assert len(left.split()) == 5 and len(right.split()) == 4
    assert any(line.split(" | ")[0].split()[1:] != line.split(" | ")[1].split() for line in rows)
    ex = [i for i, line in enumerate(out) if line.startswith("Exclusivity (FREX weight 0.7, top 4 words), mean over ")]
    assert len(ex) == 1 and ex[0] > at and out[ex[0] + 1] == "Least exclusive labels:"
    low = [float(line.split()[-1]) for line in out[ex[0] + 2:ex[0] + 7]]
    assert len(low) == 5 and low == sorted(low) and 0 < low[0] <= 4
    np.random.seed(0)
    H.main(argv + ["--frex-words", "4", "--exclusivity", "4", "--frex-weight", "0.25"])
    out = capsys.readouterr().out.splitlines()
    assert "Label words (top 4): most frequent | FREX (weight 0.25):" in out
    assert any(line.startswith("Exclusivity (FREX weight 0.25, top 4 words), mean over ") for line in out)
