"""``llda_word_cooc`` (include/llda_gibbs.h) bit for bit against its numpy restatement (tests/topicref.py: a per-document set
loop): documents of 0 .. 3 000 sites with repeated words, every K that changes the LDS footprint, diagonal-only up to all 120
pairs, hand-made membership tables, full contention, isolation between the documents a wavefront takes in turn, untouched
entries and accumulation over document ranges.  ``co`` is pre-filled and carries guard words behind it."""
import numpy as np
import pytest
import torch

import topicref

pytestmark = pytest.mark.gpu

GUARD = 8
DEV = "cuda:0"


def prefill(K, n):
    return (np.arange(K * n * n + GUARD, dtype=np.int64) * 7919 + 1000003) % 1000000007


def run(doc_off, word, V, top_idx, ranges=None):
    """-> what the calls ADDED to the (K, n, n) counts; checks that entries j > i and the guard words stay what they were.
    ranges: document boundaries [0, a, b, ..., D] -- one call per range into the same buffer (default: one call)."""
    from lda_thesis_amd import _native, topics
    top_idx = np.asarray(top_idx)
    K, n = top_idx.shape
    D = len(doc_off) - 1
    off_d = torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(DEV)
    word_d = torch.from_numpy(np.ascontiguousarray(word, dtype=np.int32)).to(DEV)
    memb_off, memb = topics.membership(top_idx, V, device=DEV)
    if memb.numel() == 0:
        memb = torch.zeros((1,), dtype=torch.int32, device=DEV)
    before = prefill(K, n)
    co = torch.from_numpy(before.copy()).to(DEV)
    ranges = [0, D] if ranges is None else ranges
    for a, b in zip(ranges[:-1], ranges[1:]):
        _native.word_cooc(off_d[a:], word_d, b - a, V, K, n, memb_off, memb, co)
    torch.cuda.synchronize()
    after = co.cpu().numpy()
    assert np.array_equal(after[K * n * n:], before[K * n * n:]), "guard words"
    delta = (after - before)[:K * n * n].reshape(K, n, n)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    assert (delta[:, upper] == 0).all(), "entries j > i were written"
    return delta


def lens_for(rng, D):
    special = {1: [300], 3: [64, 0, 65]}.get(D)
    if special is None:
        special = [3000, 0, 1, 63, 64, 65, 300] + rng.integers(0, 40, size=D - 7).tolist()
    assert len(special) == D
    return special


CORPUS_V = 3000


@pytest.fixture(scope="module")
def corpora():
    """one corpus per D, shared and left unchanged: documents of 0, 1, 63, 64, 65, 300 and 3 000 sites, words repeat"""
    out = {}
    for D in (1, 3, 65, 257, 1000):
        rng = np.random.default_rng(D)
        out[D] = topicref.mixed_corpus(rng, CORPUS_V, lens_for(rng, D))
    return out


@pytest.mark.parametrize("K,n,D", [(1, 1, 1), (1, 16, 257), (12, 1, 1000), (12, 2, 3), (12, 10, 1000), (12, 16, 257),
                                   (512, 10, 1000), (512, 16, 65), (512, 2, 257), (1031, 10, 257), (1031, 1, 65),
                                   (7688, 10, 65), (7688, 16, 3), (7688, 2, 1)])
def test_against_the_restatement(corpora, K, n, D):
    doc_off, word = corpora[D]
    if D >= 65:
        assert len(np.unique(word[doc_off[0]:doc_off[1]])) < doc_off[1] - doc_off[0]      # a word repeats inside a document
    rng = np.random.default_rng([K, n, D])
    top = topicref.random_lists(rng, K, n, CORPUS_V, holes=0.1 if n > 1 else 0.0)
    top[:, 0] = rng.choice(word, size=K)                                                 # words the corpus holds: pairs do occur
    want = topicref.cooc_ref(doc_off, word, top)
    assert want.max() > 0
    got = run(doc_off, word, CORPUS_V, top)
    assert np.array_equal(got, want)


def test_no_documents_is_a_no_op():
    got = run(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), 50, np.array([[1, 2], [3, 4]]))
    assert (got == 0).all()


def test_hand_made_tables():
    V = 50
    top = np.array([[7, 3, -1, 49],            # word 7: topic 0 rank 0, topic 1 rank 2, topic 2 rank 1; a hole; the last word id
                    [3, -1, 7, 0],
                    [49, 7, 3, -1],
                    [-1, -1, -1, -1],          # a topic that lists nothing
                    [12, 13, 14, 15]])         # 15 is listed and no document holds it
    docs = [[7, 7, 3], [49], [], [0, 3, 7, 49, 12, 13], [14, 12, 12, 12], [1, 2, 4], [49, 7]]
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    word = np.array([w for d in docs for w in d], dtype=np.int32)
    want = topicref.cooc_ref(doc_off, word, top)
    got = run(doc_off, word, V, top)
    assert np.array_equal(got, want)
    assert got[0, 0, 0] == 3 and got[0, 1, 0] == 2 and got[0, 3, 3] == 3 and got[0, 3, 0] == 2      # by hand
    assert got[1, 2, 0] == 2 and got[2, 1, 0] == 2 and (got[3] == 0).all()
    assert got[4, 3, 3] == 0 and got[4, 2, 0] == 1 and got[4, 1, 0] == 1 and got[4, 0, 0] == 2
    assert (run(doc_off, word, V, np.full((3, 4), -1)) == 0).all()                                    # an empty table


@pytest.mark.parametrize("K,n", [(12, 16), (512, 4)])
def test_contention_every_document_holds_every_listed_word(K, n):
    rng = np.random.default_rng(K)
    V, D = 400, 1000
    top = topicref.random_lists(rng, K, n, V)
    listed = np.unique(top)
    docs = [np.concatenate([rng.permutation(listed), rng.integers(0, V, size=int(rng.integers(0, 5)))]) for _ in range(D)]
    doc_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    got = run(doc_off, np.concatenate(docs).astype(np.int32), V, top)
    assert (got[:, np.tril(np.ones((n, n), dtype=bool))] == D).all()


def test_isolation_between_the_documents_a_wavefront_takes_in_turn():
    """wavefront i takes the documents i, i + COOC_MAX_WAVES, ...: a long document, then an empty one, then one that shares no
    word with it, on ONE wavefront -- and random short documents on all the others.  Masks that are not reset show up at once."""
    from lda_thesis_amd import _native
    W = _native.COOC_MAX_WAVES
    rng = np.random.default_rng(9)
    V, K, n = 3000, 12, 16
    D = 2 * W + 40
    lens = rng.integers(0, 7, size=D)
    lens[5], lens[5 + W], lens[5 + 2 * W] = 3000, 0, 60
    doc_off, word = topicref.mixed_corpus(rng, V, lens)
    word[doc_off[5]:doc_off[6]] = rng.integers(0, 1500, size=3000)                        # the long document: low half of the ids
    word[doc_off[5 + 2 * W]:doc_off[5 + 2 * W + 1]] = rng.integers(1500, V, size=60)      # its second successor: high half
    top = topicref.random_lists(rng, K, n, V)
    top[:, :8] = rng.permuted(np.tile(np.arange(0, 1500, 15)[:96].reshape(K, 8), 1), axis=1)    # words the long document is rich in
    top[:, 8:] = 1500 + rng.choice(1500, size=(K, 8), replace=False)
    want = topicref.cooc_ref(doc_off, word, top)
    got = run(doc_off, word, V, top)
    assert np.array_equal(got, want)
    alone = topicref.cooc_ref(doc_off, word, top, 5 + 2 * W, 5 + 2 * W + 1)
    assert (alone[:, :8, :8] == 0).all()                                                  # it holds none of the long document's words


def test_accumulation_over_document_ranges(corpora):
    doc_off, word = corpora[257]
    D, K, n = 257, 12, 10
    rng = np.random.default_rng(77)
    top = topicref.random_lists(rng, K, n, CORPUS_V, holes=0.1)
    top[:, 0] = rng.integers(0, 30, size=K)
    want = topicref.cooc_ref(doc_off, word, top)
    one = run(doc_off, word, CORPUS_V, top)
    two = run(doc_off, word, CORPUS_V, top, ranges=[0, 100, D])
    seven = run(doc_off, word, CORPUS_V, top, ranges=[0, 1, 2, 40, 41, 130, 256, D])
    each = run(doc_off, word, CORPUS_V, top, ranges=list(range(D + 1)))
    for got in (one, two, seven, each):
        assert np.array_equal(got, want)


def test_python_surface_and_out_argument(corpora):
    from lda_thesis_amd import topics
    doc_off, word = corpora[65]
    rng = np.random.default_rng(3)
    top = topicref.random_lists(rng, 12, 10, CORPUS_V)
    top[:, 0] = rng.integers(0, 30, size=12)
    want = topicref.cooc_ref(doc_off, word, top)
    off_d, word_d = torch.from_numpy(doc_off).to(DEV), torch.from_numpy(word).to(DEV)
    co = topics.cooccurrence(off_d, word_d, CORPUS_V, top)
    assert co.dtype == torch.int64 and tuple(co.shape) == (12, 10, 10) and np.array_equal(co.cpu().numpy(), want)
    again = topics.cooccurrence(off_d, word_d, CORPUS_V, torch.from_numpy(top).to(DEV), out=co)
    assert again is co and np.array_equal(co.cpu().numpy(), 2 * want)
    part = topics.cooccurrence(off_d[:31], word_d, CORPUS_V, top)
    topics.cooccurrence(off_d[30:], word_d, CORPUS_V, top, out=part, table=topics.membership(top, CORPUS_V, device=DEV))
    assert np.array_equal(part.cpu().numpy(), want)


@pytest.mark.parametrize("K,n", [(1, 1), (12, 16), (130, 10), (512, 10), (512, 16), (1031, 2), (7688, 16)])
def test_large_calls_count_in_lds_first_and_add_the_same_integers(K, n):
    """from COOC_AGG_MIN_DOCS documents on a call counts per slice of topics in LDS (one, two, five slices here) -- or, at
    K = 7 688 with 16 ranks, where the slices would be too many, stays with the global atomics.  A wavefront takes many documents
    in turn; a long and an empty document sit among the short ones."""
    from lda_thesis_amd import _native
    rng = np.random.default_rng([7, K, n])
    V = 600 if K <= 1031 else 20000          # (the restatement's time goes with the topics that list a word)
    D = _native.COOC_AGG_MIN_DOCS + 37
    lens = rng.integers(0, 6, size=D)
    lens[11], lens[12], lens[D - 1] = 3000, 0, 300
    doc_off, word = topicref.mixed_corpus(rng, V, lens)
    top = topicref.random_lists(rng, K, n, V, holes=0.1 if n > 1 else 0.0)
    top[:, 0] = rng.choice(word, size=K)
    want = topicref.cooc_ref(doc_off, word, top)
    assert want.max() > 0
    assert np.array_equal(run(doc_off, word, V, top), want)
    if K == 12:          # ranges on either side of the threshold add up to the same
        assert np.array_equal(run(doc_off, word, V, top, ranges=[0, 5, D - 3, D]), want)
