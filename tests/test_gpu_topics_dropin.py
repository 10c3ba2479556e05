"""Top words and coherence on the drop-in class and on sharded samplers: ``LabeledLDA.top_words`` / ``topwords_per_topic`` /
``coherence`` against the model's own ``get_phi()`` and the numpy restatement (tests/topicref.py), a pickle round trip, and two
and three ranks on the one GPU (the last shard empty) against the one-process integers, bit for bit."""
import pickle

import numpy as np
import pytest

from conftest import load_golden
from test_distributed_gloo import _setup
from test_gpu_dropin import build_model
from test_gpu_multirank import _spawn
import topicref

pytestmark = pytest.mark.gpu


def trained(name):
    m, _, sweeps = build_model(name)
    for _ in range(sweeps):
        m.training_iteration()
    return m


def corpus_of(m, docs=None):
    from lda_thesis_amd.corpus import csr_from_doc_tups
    tups = m.doc_tups if docs is None else [m.dicti.doc2bow(x) for x in docs]
    doc_off, word, _ = csr_from_doc_tups(tups)
    return np.asarray(doc_off, dtype=np.int64), np.asarray(word, dtype=np.int32)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module", params=["k12", "k392"])
def model(request):
    return trained(request.param)


def test_top_words_on_the_class(model):
    m = model
    idx, cnt = m.top_words(10)
    assert idx.shape == cnt.shape == (m.K, 10) and idx.dtype == np.int32
    phi, n_k_v = m.get_phi(), m.n_k_v
    for k in range(m.K):
        want = np.argsort(-phi[k], kind="stable")[:10]
        assert np.array_equal(idx[k], want), k
        assert np.array_equal(cnt[k], n_k_v[k, want])
    names = list(m.labelmap.keys())
    on_device = m.topwords_per_topic(10, device=True)
    assert on_device == [[names[k]] + [m.v_to_w[int(v)] for v in idx[k]] for k in range(m.K)]
    as_it_was = [[names[k]] + [m.v_to_w[v] for v in np.argsort(-phi[k, :])[:10]] for k in range(m.K)]
    assert m.topwords_per_topic(10) == as_it_was == m.topwords_per_topic(topwords=10, device=False)
    assert [r[:4] for r in m.topwords_per_topic(3, device=True)] == [r[:4] for r in on_device]
    with pytest.raises(ValueError):
        m.top_words(17)


def test_coherence_on_the_class(model):
    from lda_thesis_amd import topics
    m = model
    idx, _ = m.top_words(10)
    doc_off, word = corpus_of(m)
    co = topicref.cooc_ref(doc_off, word, idx)
    D = len(doc_off) - 1
    u, p = m.coherence(10, "umass"), m.coherence(10, "npmi")
    assert u.dtype == np.float64 and u.shape == (m.K,)
    assert same(u, topics.umass(co, listed=idx)) and same(p, topics.npmi(co, D, listed=idx))
    assert np.isfinite(u).any() and np.isfinite(p).any()
    assert same(m.coherence(), u)
    # a held-out reference corpus: token lists, words outside the dictionary are dropped by doc2bow
    held = [[m.v_to_w[w] for w in reversed(ws)] + ["no-such-token"] for ws in m.docs[:9]]
    held.append(["no-such-token"])                                 # a document without any in-vocabulary word: no sites
    off2, word2 = corpus_of(m, held)
    co2 = topicref.cooc_ref(off2, word2, idx)
    assert same(m.coherence(10, "umass", docs=held), topics.umass(co2, listed=idx))
    assert same(m.coherence(10, "npmi", docs=held), topics.npmi(co2, len(held), listed=idx))
    with pytest.raises(ValueError):
        m.coherence(10, "c_v")


def test_pickle_round_trip_keeps_working():
    m = trained("k12")
    idx, cnt = m.top_words(10)
    u = m.coherence(10, "umass")
    m2 = pickle.loads(pickle.dumps(m))
    idx2, cnt2 = m2.top_words(10)
    assert np.array_equal(idx, idx2) and np.array_equal(cnt, cnt2)
    assert same(m2.coherence(10, "umass"), u)
    assert m2.topwords_per_topic(10, device=True) == m.topwords_per_topic(10, device=True)


def _rank_worker(rank, world, port, name, q):
    dev = _setup(rank, world, port, True)
    import torch.distributed as dist
    from lda_thesis_amd import topics
    from lda_thesis_amd.sampler import GibbsSampler, shard_documents
    g = load_golden(name)
    off = g["doc_off"]
    b = shard_documents(off, world - 1) + [int(g["D"])]          # the last rank holds no document at all
    lo, hi = b[rank], b[rank + 1]
    s0, s1 = int(off[lo]), int(off[hi])
    s = GibbsSampler(off[lo:hi + 1] - off[lo], g["word"][s0:s1], g["freq"][s0:s1], g["init_z"][s0:s1], int(g["K"]), int(g["V"]),
                     float(g["alpha"]), float(g["beta"]), labs=g["labs"][lo:hi], seed=int(g["seed"]), doc_base=lo, device=dev)
    for _ in range(int(g["sweeps"])):
        s.sweep()
    idx, cnt = s.top_words(10)
    co, d_total = s.word_cooccurrence(idx)
    idx = idx.cpu().numpy()
    q.put((rank, hi - lo, idx, cnt.cpu().numpy(), co, d_total, topics.umass(co, listed=idx), topics.npmi(co, d_total, listed=idx)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_returns_the_one_process_integers(world):
    from lda_thesis_amd import topics
    name = "tiny_k40"
    g = load_golden(name)
    n_k_v = g["o3_s%d_n_k_v" % int(g["sweeps"])]
    idx, cnt = topicref.top_words_ref(n_k_v, 10)
    co = topicref.cooc_ref(g["doc_off"], g["word"], idx)
    D = int(g["D"])
    u, p = topics.umass(co, listed=idx), topics.npmi(co, D, listed=idx)
    res = _spawn(world, _rank_worker, (name,))
    assert sorted(r[0] for r in res) == list(range(world))
    assert [r[1] for r in sorted(res, key=lambda r: r[0])][-1] == 0 and sum(r[1] for r in res) == D
    for r in res:
        assert np.array_equal(r[2], idx) and np.array_equal(r[3], cnt), r[0]
        assert np.array_equal(r[4], co) and r[5] == D, r[0]
        assert same(r[6], u) and same(r[7], p), r[0]


def test_harness_option_prints_the_mean_and_the_five_worst_labels(capsys):
    from lda_thesis_amd import evaluate_LabeledLDA as E
    opt, _ = E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])
    assert opt.coherence == 0                                      # off by default: the report is what it was
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--coherence", "7"])[0].coherence == 7
    m = trained("k12")
    capsys.readouterr()
    E.report_coherence(m, 5)
    out = capsys.readouterr().out.splitlines()
    coh = m.coherence(5, "umass")
    ok = np.flatnonzero(~np.isnan(coh))
    assert out[0] == "-----------------------------------"
    assert out[1].startswith("UMass coherence (top 5 words), mean over %d of %d labels: " % (ok.shape[0], m.K))
    assert float(out[1].rsplit(" ", 1)[1]) == pytest.approx(float(np.mean(coh[ok])), rel=1e-12)
    assert len(out) == 2 + min(5, ok.shape[0])
    names = list(m.labelmap.keys())
    worst = ok[np.argsort(coh[ok], kind="stable")[:5]]
    idx, _ = m.top_words(5)
    for line, k in zip(out[2:], worst):
        assert line.split()[0] == names[k] and line.split()[2:] == [m.v_to_w[int(v)] for v in idx[k] if v >= 0]
