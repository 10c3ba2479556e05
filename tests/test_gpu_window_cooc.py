"""``llda_window_cooc`` (include/llda_gibbs.h) bit for bit against the brute force over windows (tests/windowref.py): random corpora
with positions that hold no word, words listed by several topics and lists with holes; planted edges of the run-length walk (a word
that leaves on the step another enters, one word under two ranks, counts that fill 16 bits); window 0 against ``llda_word_cooc``;
accumulation over document ranges; both sides of LLDA_WINDOW_AGG_MIN_DOCS and the slicing of the topics.  ``co`` is pre-filled and
carries guard words behind it."""
import numpy as np
import pytest
import torch

import topicref
import windowref

pytestmark = pytest.mark.gpu

GUARD = 8
DEV = "cuda:0"


def prefill(K, n):
    return (np.arange(K * n * n + GUARD, dtype=np.int64) * 7919 + 1000003) % 1000000007


def run(tok_off, tok, V, top_idx, window, ranges=None, base=0, kernel="window"):
    """-> what the calls ADDED to the (K, n, n) counts; checks that entries j > i and the guard words stay what they were.
    ranges: document boundaries [0, a, b, ..., D] -- one call per range into the same buffer (default: one call); base: so many
    tokens of another text in front of ``tok``, the offsets shifted to match.  One token of another text always follows."""
    from lda_thesis_amd import _native, topics
    top_idx = np.asarray(top_idx)
    K, n = top_idx.shape
    D = len(tok_off) - 1
    off_d = torch.from_numpy(np.ascontiguousarray(tok_off, dtype=np.int64) + base).to(DEV)
    other = np.full(base + 1, top_idx.max(), dtype=np.int32)                       # a listed word: counted if an index strays
    tok_d = torch.from_numpy(np.concatenate([other[:base], np.asarray(tok, dtype=np.int32), other[:1]])).to(DEV)
    memb_off, memb = topics.membership(top_idx, V, device=DEV)
    if memb.numel() == 0:
        memb = torch.zeros((1,), dtype=torch.int32, device=DEV)
    before = prefill(K, n)
    co = torch.from_numpy(before.copy()).to(DEV)
    ranges = [0, D] if ranges is None else ranges
    for a, b in zip(ranges[:-1], ranges[1:]):
        if kernel == "window":
            _native.window_cooc(off_d[a:], tok_d, b - a, V, K, n, window, memb_off, memb, co)
        else:
            _native.word_cooc(off_d[a:], tok_d, b - a, V, K, n, memb_off, memb, co)
    torch.cuda.synchronize()
    after = co.cpu().numpy()
    assert np.array_equal(after[K * n * n:], before[K * n * n:]), "guard words"
    delta = (after - before)[:K * n * n].reshape(K, n, n)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    assert (delta[:, upper] == 0).all(), "entries j > i were written"
    return delta


def csr(docs):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return off, np.array([w for d in docs for w in d], dtype=np.int32)


D_RANDOM = 300


@pytest.fixture(scope="module")
def corpora():
    """one corpus per V, shared and left unchanged: 300 documents of 0 .. 200 tokens, one in ten with positions that hold no word"""
    out = {}
    for V in (7, 2000):
        rng = np.random.default_rng(V)
        lens = rng.integers(0, 201, size=D_RANDOM)
        lens[:4] = [0, 200, 1, 111]
        off, tok = topicref.mixed_corpus(rng, V, lens)
        for d in range(1, D_RANDOM, 10):
            part = tok[off[d]:off[d + 1]]
            part[rng.random(part.shape[0]) < 0.3] = -1
        out[V] = (off, tok)
    return out


# a fixed subset of V x K x n x window: every value of every parameter, every window at both vocabularies' densities
@pytest.mark.parametrize("V,K,n,window", [(7, 1, 1, 1), (7, 1, 16, 2), (7, 12, 2, 5), (7, 12, 10, 110), (7, 130, 2, 10), (7, 12, 2, 0),
                                          (2000, 12, 10, 10), (2000, 130, 16, 110), (2000, 1031, 10, 0), (2000, 1031, 2, 2),
                                          (2000, 130, 1, 110), (2000, 1031, 16, 5), (2000, 12, 16, 1), (2000, 1, 10, 10)])
def test_random_corpora_against_the_brute_force(corpora, V, K, n, window):
    off, tok = corpora[V]
    rng = np.random.default_rng([V, K, n, window])
    top = topicref.random_lists(rng, K, n, V, holes=0.1 if n > 1 else 0.0)          # V = 7 < n: the rest of a list is -1
    top[:, 0] = rng.choice(tok[tok >= 0], size=K)                                   # words the corpus holds
    if K >= 3:
        top[1, 0] = top[2, n - 1] = top[0, 0]                                       # one word, three topics
        assert (top == top[0, 0]).sum() >= 3
    if n > 1:
        top[0, n - 1] = -1                                                          # a list with a hole
    want = windowref.window_ref(off, tok, top, window)
    assert want.max() > 0
    got = run(off, tok, V, top, window)
    assert np.array_equal(got, want)


S = 5
EDGE_TOP = np.array([[3, 4, 9, 3],           # word 3 under ranks 0 and 3 of topic 0, and under rank 1 of topic 1
                     [8, 3, -1, 2],
                     [-1, -1, -1, -1]])
EDGE_V = 12


def alternating(period, length):
    """word 3 and word 4 (ranks 0 and 1 of topic 0) in turn, ``period`` positions apart, nothing between them"""
    doc = [-1] * length
    for i, p in enumerate(range(0, length, period)):
        doc[p] = 3 if i % 2 == 0 else 4
    return doc


EDGES = {
    "L=0": [[]], "L=1": [[4]], "L=s-1": [[4, 3, 0, 9][:S - 1]], "L=s": [[4, 0, 3, 9, 4]], "L=s+1": [[4, 0, 3, 9, 4, 8]],
    "L=2s": [[4, 0, 3, 9, 4, 8, 1, 1, 2, 4]],
    "only -1": [[-1] * 13],
    "one word 3s times": [[9] * (3 * S)],
    "first and last": [[8] + [0] * 11 + [8]],
    "period s": [alternating(S, 6 * S + 1)],
    "period s+1": [alternating(S + 1, 6 * S + 3)],
    "one word, two ranks": [[0, 0, 3, 0, 0, 0, 0, 0, 4, 3, 3, 0, 0, 0, 0, 0, 0, 3]],
    "all of them, one wavefront each": [[4, 0, 3, 9, 4, 8], [], [-1] * 13, alternating(S, 31), [9] * 15, [8] + [0] * 11 + [8]],
}


@pytest.mark.parametrize("name", list(EDGES))
def test_planted_edges(name):
    off, tok = csr(EDGES[name])
    want = windowref.window_ref(off, tok, EDGE_TOP, S)
    got = run(off, tok, EDGE_V, EDGE_TOP, S)
    assert np.array_equal(got, want), name
    if name == "period s":              # by hand: 31 positions, 27 windows, each holds exactly one of the two words
        assert got[0, 0, 0] + got[0, 1, 1] == 27 and got[0, 1, 0] == 0
    if name == "period s+1":            # a window of 5 misses both words once in six
        assert got[0, 1, 0] == 0 and got[0, 0, 0] + got[0, 1, 1] < len(tok) - S + 1
    if name == "one word, two ranks":
        assert got[0, 3, 0] == got[0, 0, 0] == got[0, 3, 3] == got[1, 1, 1] > 0


def test_a_document_longer_than_any_stride():
    rng = np.random.default_rng(5000)
    V, K, n = 300, 12, 10
    off, tok = topicref.mixed_corpus(rng, V, [5000])
    tok[rng.random(5000) < 0.05] = -1
    top = topicref.random_lists(rng, K, n, V, holes=0.1)
    want = windowref.window_ref(off, tok, top, 110)
    assert want.max() > 1000
    assert np.array_equal(run(off, tok, V, top, 110), want)


def test_a_count_that_fills_sixteen_bits_does_not_wrap():
    """70 000 tokens at the widest window: word 5 nearly everywhere -- 65 535 times in many windows --, word 6 at a few places"""
    from lda_thesis_amd import _native
    s = _native.WINDOW_MAX
    tok = np.full(70000, 5, dtype=np.int32)
    tok[[0, 3000, 65534, 65535, 69000, 69999]] = 6
    off = np.array([0, 70000], dtype=np.int64)
    top = np.array([[6, 5], [5, -1]])
    want = windowref.window_ref(off, tok, top, s)
    windows = 70000 - s + 1
    assert want[1, 0, 0] == windows and want[0, 1, 0] == windows and np.array_equal(want[0].diagonal(), [windows, windows])
    assert np.array_equal(run(off, tok, 9, top, s), want)
    tok[[0, 3000, 65534, 65535]] = 5                        # now the first windows hold word 5 alone, 65 535 times
    want = windowref.window_ref(off, tok, top, s)
    assert 0 < want[0, 0, 0] < windows
    assert np.array_equal(run(off, tok, 9, top, s), want)


@pytest.mark.parametrize("V,K,n", [(7, 12, 2), (2000, 130, 16), (2000, 1031, 10)])
def test_window_zero_is_llda_word_cooc(corpora, V, K, n):
    off, tok = corpora[V]
    rng = np.random.default_rng([0, V, K, n])
    top = topicref.random_lists(rng, K, n, V, holes=0.1)
    top[:, 0] = rng.choice(tok[tok >= 0], size=K)
    got = run(off, tok, V, top, 0)
    assert got.max() > 0
    assert np.array_equal(got, run(off, tok, V, top, 0, kernel="word"))
    assert np.array_equal(got, run(off, tok, V, top, 201))                         # no document is longer than 200 tokens


def test_accumulation_over_document_ranges_and_an_offset_base(corpora):
    off, tok = corpora[2000]
    rng = np.random.default_rng(78)
    top = topicref.random_lists(rng, 12, 10, 2000, holes=0.1)
    top[:, 0] = rng.integers(0, 30, size=12)
    want = windowref.window_ref(off, tok, top, 10)
    assert np.array_equal(run(off, tok, 2000, top, 10), want)
    assert np.array_equal(run(off, tok, 2000, top, 10, ranges=[0, 100, D_RANDOM]), want)
    assert np.array_equal(run(off, tok, 2000, top, 10, ranges=[0, 1, 2, 40, 41, 130, 299, D_RANDOM]), want)
    assert np.array_equal(run(off, tok, 2000, top, 10, ranges=[0, 100, D_RANDOM], base=777), want)


def test_python_surface_and_out_argument(corpora):
    from lda_thesis_amd import topics
    off, tok = corpora[2000]
    rng = np.random.default_rng(3)
    top = topicref.random_lists(rng, 12, 10, 2000)
    top[:, 0] = rng.integers(0, 30, size=12)
    want = windowref.window_ref(off, tok, top, 10)
    off_d, tok_d = torch.from_numpy(off).to(DEV), torch.from_numpy(tok).to(DEV)
    co = topics.window_cooccurrence(off_d, tok_d, 2000, top, 10)
    assert co.dtype == torch.int64 and tuple(co.shape) == (12, 10, 10) and np.array_equal(co.cpu().numpy(), want)
    again = topics.window_cooccurrence(off_d, tok_d, 2000, torch.from_numpy(top).to(DEV), 10, out=co)
    assert again is co and np.array_equal(co.cpu().numpy(), 2 * want)
    part = topics.window_cooccurrence(off_d[:31], tok_d, 2000, top, 10)
    topics.window_cooccurrence(off_d[30:], tok_d, 2000, top, 10, out=part, table=topics.membership(top, 2000, device=DEV))
    assert np.array_equal(part.cpu().numpy(), want)
    assert topics.window_count(off_d, 10) == windowref.window_count_ref(off, 10)
    with pytest.raises(ValueError):
        topics.window_cooccurrence(off_d, tok_d, 2000, top, 65536)
    assert (topics.window_cooccurrence(off_d, tok_d, 2000, np.full((3, 4), -1), 10).cpu().numpy() == 0).all()     # an empty table


@pytest.mark.parametrize("K,n,window,V", [(12, 10, 3, 40), (512, 16, 6, 4000), (1031, 16, 6, 8000)])
def test_both_sides_of_the_threshold_add_the_same_integers(K, n, window, V):
    """from LLDA_WINDOW_AGG_MIN_DOCS documents on a call adds to LDS counters per slice of topics (one slice, eight slices) -- or,
    at K = 1 031 with 16 ranks, where the slices would be too many, stays with the global atomics.  The same corpus in two halves
    stays below the threshold.  Tiny documents; a wavefront takes several in turn either way."""
    from lda_thesis_amd import _native
    rng = np.random.default_rng([8, K, n])
    D = _native.WINDOW_AGG_MIN_DOCS + 37
    assert D // 2 > _native.WINDOW_MAX_WAVES
    off, tok = topicref.mixed_corpus(rng, V, rng.integers(0, 9, size=D))
    tok[rng.random(tok.shape[0]) < 0.02] = -1
    top = topicref.random_lists(rng, K, n, V, holes=0.3)
    top[:, 0] = rng.choice(tok[tok >= 0], size=K)
    want = windowref.window_ref(off, tok, top, window)
    assert want.max() > 0
    above = run(off, tok, V, top, window)
    below = run(off, tok, V, top, window, ranges=[0, D // 2, D])
    assert np.array_equal(above, below)
    assert np.array_equal(above, want)


def test_the_topics_are_sliced_at_the_largest_k():
    """K = 7 688 with 16 ranks: sixteen slices of per-wavefront state, each walking the corpus"""
    rng = np.random.default_rng(7688)
    K, n, V = 7688, 16, 20000
    lens = rng.integers(0, 201, size=100)
    off, tok = topicref.mixed_corpus(rng, V, lens)
    top = topicref.random_lists(rng, K, n, V, holes=0.1)
    top[:, 0] = rng.choice(tok, size=K)
    top[K - 1, 1] = top[0, 0]                                                       # one word in the first and in the last slice
    want = windowref.window_ref(off, tok, top, 10)
    assert want[0].max() > 0 and want[K - 1].max() > 0
    assert np.array_equal(run(off, tok, V, top, 10), want)
