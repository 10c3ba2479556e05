"""Sliding-window coherence on the drop-in class: ``LabeledLDA.window_coherence`` against the brute force over windows fed to the
same host functions (bit for bit) and against the plain-loop restatement of the measures (tests/windowref.py, within its derived
bound), on texts with unknown tokens in the middle; and the harness option."""
import numpy as np
import pytest

from test_gpu_topics_dropin import trained
import windowref

pytestmark = pytest.mark.gpu

UNKNOWN = "no-such-token"


@pytest.fixture(scope="module", params=["k12", "k392"])
def model(request):
    return trained(request.param)


def texts_of(m, unknown=True):
    """``m.docs`` mapped back to words; with an unknown token put in at every fifth position of every second text"""
    texts = [[m.v_to_w[w] for w in ws] for ws in m.docs]
    if unknown:
        for d in range(0, len(texts), 2):
            out = []
            for x in texts[d]:
                if len(out) % 5 == 4:
                    out.append(UNKNOWN)
                out.append(x)
            texts[d] = out
    return texts


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def counted(model):
    """the brute-force integers of the model's 10 best words, per window width, with and without the unknown tokens: computed once"""
    from lda_thesis_amd import topics
    idx, _ = model.top_words(10)
    out = {"idx": idx}
    for unknown in (True, False):
        tok_off, tok = topics.token_csr(texts_of(model, unknown), model.dicti.token2id)
        assert (tok == -1).any() == unknown
        for window in (5, 10, 110):
            out[unknown, window] = (windowref.window_ref(tok_off, tok, idx, window), windowref.window_count_ref(tok_off, window))
    return out


@pytest.mark.parametrize("measure", ["c_v", "c_uci", "c_npmi"])
@pytest.mark.parametrize("window", [None, 5])
def test_window_coherence_on_the_class(model, counted, measure, window):
    from lda_thesis_amd import topics
    m, idx = model, counted["idx"]
    s = topics.DEFAULT_WINDOW[measure] if window is None else window
    co, N = counted[True, s]
    got = m.window_coherence(texts_of(m), 10, measure, window)
    assert got.dtype == np.float64 and got.shape == (m.K,)
    assert same(got, getattr(topics, measure)(co, N, listed=idx))              # same function, same integers: bit for bit
    ref, bound = windowref.coherence_ref(co, N, measure, idx)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert ok.any()                                                            # all-NaN output shows nothing
    print(measure, s, "finite labels %d of %d, largest |d| / bound %.3g" % (ok.sum(), m.K, float(np.max(np.abs(got[ok] - ref[ok]) / bound[ok]))))
    assert (np.abs(got[ok] - ref[ok]) <= bound[ok]).all()
    if window is None:
        assert same(got, m.window_coherence(texts_of(m), 10, measure, s)) and same(got, m.window_coherence(texts_of(m), measure=measure))
    # the unknown tokens hold their places: without them the windows, and at least one integer, are different -- wherever a text
    # is longer than the window; at 110 every text of these models is one window, which the unknown tokens cannot change
    longest = max(len(t) for t in texts_of(m, False))
    assert 10 < longest < 110
    assert np.array_equal(co, counted[False, s][0]) == (s > longest)


def test_window_coherence_refuses_other_measures_and_coherence_stays(model):
    m = model
    for name in ("umass", "npmi", "c_p"):
        with pytest.raises(ValueError):
            m.window_coherence(texts_of(m), 10, name)
    with pytest.raises(ValueError):
        m.coherence(10, "c_v")
    with pytest.raises(ValueError):
        m.window_coherence(texts_of(m), 10, "c_v", 65536)
    with pytest.raises(ValueError):
        m.window_coherence(texts_of(m), 17)


def test_harness_option_prints_the_mean_and_the_five_worst_labels(capsys):
    from lda_thesis_amd import evaluate_LabeledLDA as E
    opt, _ = E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])
    assert opt.window_coherence == 0                               # off by default: the report is what it was
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--window-coherence", "7"])[0].window_coherence == 7
    m = trained("k12")
    texts = texts_of(m)
    capsys.readouterr()
    E.report_window_coherence(m, texts, 5)
    out = capsys.readouterr().out.splitlines()
    coh = m.window_coherence(texts, 5, "c_v")
    ok = np.flatnonzero(~np.isnan(coh))
    assert ok.shape[0] > 0
    assert out[0] == "-----------------------------------"
    assert out[1].startswith("C_V coherence (top 5 words), mean over %d of %d labels: " % (ok.shape[0], m.K))
    assert float(out[1].rsplit(" ", 1)[1]) == pytest.approx(float(np.mean(coh[ok])), rel=1e-12)
    assert len(out) == 2 + min(5, ok.shape[0])
    names = list(m.labelmap.keys())
    worst = ok[np.argsort(coh[ok], kind="stable")[:5]]
    idx, _ = m.top_words(5)
    for line, k in zip(out[2:], worst):
        assert line.split()[0] == names[k] and line.split()[2:] == [m.v_to_w[int(v)] for v in idx[k] if v >= 0]
