"""llda_heldout_loglik on the device: bit for bit against its CPU restatement (tests/heldoutref.py) around every seam of the
geometry, and end to end (LabeledLDA.heldout_perplexity, the harness's --heldout-perplexity) against the host path."""
import pickle

import numpy as np
import pytest

import heldoutref

pytestmark = pytest.mark.gpu

MAX_K = 7688
KS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 392, 512, 513, 1024, 1025, 1031, MAX_K)
DS = (1, 3, 4, 5, 63, 64, 65, 257)
GUARD = 8
MAX_F = 2 ** 23 - 1
PATTERN = {"float64": np.float64(-1234.5), "int64": np.int64(-0x123456789ABCDEF)}
OUTPUTS = (("mant", "float64"), ("expo", "int64"), ("tok", "int64"), ("bad", "int64"))
V = 61
W_ZERO, W_NAN, W_INF, W_TINY = 0, 1, 2, 3                                # words with a planted row of phi_t


def model(rng, K, D, pad_theta=3, pad_phi=5):
    """theta (D, K + pad_theta), phi_t (V, K + pad_phi): NaN in every column >= K; sparse positive loads as a fold-in leaves them,
    smoothed; planted rows: all zero (p = 0), a NaN and an inf in a column that is read, entries whose products with theta
    underflow to denormals and to zero"""
    theta = np.full((D, K + pad_theta), np.nan)
    t = rng.gamma(0.3, size=(D, K)) * (rng.random((D, K)) < max(0.1, min(1.0, 6 / K))) + 1e-4
    if K > 1:
        t[:, rng.integers(0, K)] = 0.0                                   # an exact zero in every row
    theta[:, :K] = t / np.maximum(t.sum(axis=1, keepdims=True), 1e-300)
    phi_t = np.full((V, K + pad_phi), np.nan)
    phi_t[:, :K] = rng.gamma(0.2, size=(V, K)) / V + 1e-9
    phi_t[W_ZERO, :K] = 0.0
    phi_t[W_NAN, rng.integers(0, K)] = np.nan
    phi_t[W_INF, rng.integers(0, K)] = np.inf
    phi_t[W_TINY, :K] = rng.choice([5e-324, 3e-310, 1e-308, 7e-315], size=K)
    return theta, phi_t


def corpus(rng, D, lens, freq_mode="mixed"):
    n = rng.choice(lens, size=D)
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(4, V, size=S).astype(np.int32)
    plant = rng.random(S)
    for w, lo in ((W_ZERO, 0.0), (W_NAN, 0.02), (W_INF, 0.04), (W_TINY, 0.06)):
        word[(plant >= lo) & (plant < lo + (0.06 if w == W_TINY else 0.02))] = w
    if freq_mode == "ones":
        freq = np.ones(S, dtype=np.int32)
    else:
        freq = rng.integers(0, 10, size=S).astype(np.int32)               # f = 0 included
        freq[rng.random(S) < 0.1] = MAX_F
        freq[rng.random(S) < 0.3] = 1
    return doc_off, word, freq


def run(theta, phi_t, doc_off, word, freq, K, skip=(), n_vocab=V):
    """one llda_heldout_loglik call with guard words before and behind every output -> dict of whole buffers"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    D = len(doc_off) - 1
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_theta, d_phi, d_off, d_word, d_freq = up(theta), up(phi_t), up(doc_off), up(word), up(freq)
    if d_word.numel() == 0:
        d_word = torch.zeros((1,), dtype=torch.int32, device=dev)
    bufs = {n: torch.full((D + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    _native.heldout_loglik(d_off, d_word, d_freq, d_theta, d_phi, D, n_vocab, K, ld_theta=theta.shape[1], ld_phi=phi_t.shape[1],
                           **{n: b[GUARD:GUARD + D] for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def check(got, want, D, skip=(), what=""):
    for (name, dt), w in zip(OUTPUTS, want):
        g, pat = got[name], PATTERN[dt]
        assert (g[:GUARD] == pat).all() and (g[GUARD + D:] == pat).all(), "%s: guard words around %s overwritten" % (what, name)
        body = g[GUARD:GUARD + D]
        if name in skip:
            assert (body == pat).all(), "%s: %s was written" % (what, name)
            continue
        a, b = (body.view(np.uint64), np.ascontiguousarray(w).view(np.uint64)) if dt == "float64" else (body, w)
        diff = np.flatnonzero(a != b)
        assert diff.size == 0, "%s: %s differs at documents %s: got %s want %s" % (what, name, diff[:5], body[diff[:5]], w[diff[:5]])


def lens_for(K):
    """site counts: none, one, the seams of the 64-site chunks; a few dozen at most where a row is long"""
    return (0, 1, 2, 3, 5, 63, 64, 65, 130) if K <= 513 else (0, 1, 2, 7, 33, 65)


@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_heldoutref(K):
    rng = np.random.default_rng(5000 + K)
    seen = np.zeros(4, dtype=np.int64)
    for D in DS:
        pad = (0, 0) if D == 4 else (3, 5)                               # D = 4: ld == K
        theta, phi_t = model(rng, K, D, *pad)
        doc_off, word, freq = corpus(rng, D, lens_for(K)[:6] if D == 257 else lens_for(K), "ones" if D == 5 else "mixed")
        want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq, K=K)
        check(run(theta, phi_t, doc_off, word, freq, K), want, D, what="K %d D %d" % (K, D))
        seen += [int(want[2].sum() > 0), int(want[3].sum() > 0), int((want[1] < -1100).any()), int((freq == MAX_F).any())]
        if D == 65:                                                      # freq = NULL: every site once
            want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, None, K=K)
            check(run(theta, phi_t, doc_off, word, None, K), want, D, what="K %d D %d no freq" % (K, D))
    assert (seen > 0).all(), seen                                        # scored and bad sites, a product below the float64 range, f = 2^23 - 1


def test_long_document_and_empty_ones():
    """K = 64: no site, one site, 3 000 sites (47 chunks of 64, the last one short), then one site again"""
    rng = np.random.default_rng(64)
    K, D = 64, 4
    theta, phi_t = model(rng, K, D)
    doc_off = np.array([0, 0, 1, 3001, 3002], dtype=np.int64)
    word = rng.integers(3, V, size=3002).astype(np.int32)
    freq = rng.integers(1, 4, size=3002).astype(np.int32)
    want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq, K=K)
    assert (want[0][0], want[1][0], want[2][0], want[3][0]) == (0.5, 1, 0, 0) and want[2][2] > 3000
    check(run(theta, phi_t, doc_off, word, freq, K), want, D, what="long")


def test_denormal_p_and_words_outside_the_vocabulary():
    """p itself a denormal (frexp must normalise it) at both kernel forms; a word id of -1 or V is never an index: bad"""
    for K in (5, 70):
        theta = np.zeros((2, K))
        theta[:, 0] = 1.0
        phi_t = np.full((V, K), 0.25)
        phi_t[4, :] = 0.0
        phi_t[4, 0] = 5e-324
        phi_t[5, 0] = 3e-310
        doc_off = np.array([0, 3, 8], dtype=np.int64)
        word = np.array([4, 5, 6, -1, 4, V, 5, 2 ** 31 - 1], dtype=np.int32)
        freq = np.array([3, 1, 2, 5, 1, 7, 2, 11], dtype=np.int32)
        want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq, K=K)
        assert want[3].tolist() == [0, 23] and want[1][0] < -4000
        check(run(theta, phi_t, doc_off, word, freq, K), want, 2, what="denormal K %d" % K)


@pytest.mark.parametrize("K", (7, 32, 65, 512, 1031))
def test_geometry_independence(K):
    """the same documents, shuffled and cut into batches of 1, 7 and all of them: identical bits per document"""
    rng = np.random.default_rng(7000 + K)
    D = 23
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 4, 9, 66))
    want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq, K=K)
    order = rng.permutation(D)
    for batch in (1, 7, D):
        got = [np.empty(D, dtype=dt) for _, dt in OUTPUTS]
        for lo in range(0, D, batch):
            ids = order[lo:lo + batch]
            n = np.diff(doc_off)[ids]
            off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
            sites = np.concatenate([np.arange(doc_off[d], doc_off[d + 1]) for d in ids]).astype(np.int64)
            r = run(theta[ids], phi_t, off, word[sites], freq[sites], K)
            for g, (name, _) in zip(got, OUTPUTS):
                g[ids] = r[name][GUARD:GUARD + len(ids)]
        for g, w, (name, _) in zip(got, want, OUTPUTS):
            assert np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)), (K, batch, name)


@pytest.mark.parametrize("K", (8, 129, 2000))
def test_every_output_may_be_null(K):
    rng = np.random.default_rng(8000 + K)
    D = 9
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 5, 20))
    want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq, K=K)
    for name, _ in OUTPUTS:
        check(run(theta, phi_t, doc_off, word, freq, K, skip=(name,)), want, D, skip=(name,), what="K %d without %s" % (K, name))
    import torch
    from lda_thesis_amd import _native
    t = torch.zeros((1, K), dtype=torch.float64, device="cuda:0")
    _native.heldout_loglik(None, None, None, t, t, 0, 1, K)              # D = 0: a no-op, nothing is dereferenced


def test_python_surface():
    """heldout.loglik: numpy CSR, strided device tensors, weighted=False, and its refusals"""
    import torch
    from lda_thesis_amd import heldout
    rng = np.random.default_rng(11)
    K, D = 40, 6
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 5, 20), "ones")
    freq = rng.integers(1, 6, size=freq.shape[0]).astype(np.int32)
    word[word < 4] = 9
    dev = torch.device("cuda", 0)
    d_theta, d_phi = torch.from_numpy(theta).to(dev)[:, :K], torch.from_numpy(phi_t).to(dev)[:, :K]      # row strides K + 3, K + 5
    for weighted in (True, False):
        want = heldoutref.loglik_ref(theta, phi_t, doc_off, word, freq if weighted else None, K=K)
        got = heldout.loglik(d_theta, d_phi, doc_off, word, freq, weighted=weighted)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g.view(np.uint64), w.view(np.uint64))
        assert heldout.perplexity_from(*got) == heldout.perplexity_from(*want)
    ppl = heldout.perplexity_from(*got)
    assert ppl["bad"] == 0 and ppl["tokens"] == len(word) and np.isfinite(ppl["perplexity"])
    with pytest.raises(ValueError):
        heldout.loglik(d_theta, d_phi, doc_off, np.where(word == 9, V, word), freq)
    with pytest.raises(ValueError):
        heldout.loglik(d_theta, d_phi, doc_off, word, np.full_like(freq, 2 ** 23))
    with pytest.raises(ValueError):
        heldout.loglik(d_theta, d_phi, doc_off[:-1], word, freq)
    with pytest.raises(ValueError):
        heldout.loglik(d_theta, d_phi[:, :K - 1], doc_off, word, freq)
    with pytest.raises(ValueError):
        heldout.loglik(theta, d_phi, doc_off, word, freq)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def host_path(m, docs, it, thinning, seed=None, weighted=True, scored_docs=None):
    """the definition on the host: run_test on the observed halves, the theta expression in numpy, heldoutref, perplexity_from"""
    from lda_thesis_amd import heldout
    from lda_thesis_amd.corpus import csr_from_doc_tups
    tups = [m.dicti.doc2bow(x) for x in docs]
    if scored_docs is None:
        obs, sco = heldout.completion_split(tups)
    else:
        obs, sco = tups, [m.dicti.doc2bow(x) for x in scored_docs]
    keep = [d for d, t in enumerate(obs) if t]
    obs, sco = [obs[d] for d in keep], [sco[d] for d in keep]
    inv = {v: k for k, v in m.dicti.token2id.items()}
    th = m.run_test([[inv[w] for w, f in t for _ in range(f)] for t in obs], it, thinning, seed=seed)
    theta = heldout.smooth_theta(th, heldout.observed_tokens(obs), m.alpha)
    doc_off, word, freq = csr_from_doc_tups(sco)
    out = heldoutref.loglik_ref(theta, np.ascontiguousarray(m.ph_hat.T), doc_off, word, freq if weighted else None)
    r = heldout.perplexity_from(*out)
    return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=len(tups) - len(keep))


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.float64(a[k]).view(np.uint64), np.float64(b[k]).view(np.uint64)) for k in a)


@pytest.mark.parametrize("name", ("k12", "k392"))
def test_heldout_perplexity_equals_the_host_path(name, capsys):
    from test_gpu_rank_labels import _model
    m, docs, _ = _model(name)
    docs = [list(d) for d in docs[:40]]
    docs[3] = ["no-such-token"]                                          # no in-vocabulary word: skipped
    docs[5] = docs[5][:1]                                                # one site: observed, nothing scored
    got = m.heldout_perplexity(docs, 6, 2, seed=77)
    want = host_path(m, docs, 6, 2, seed=77)
    print(name, got, want)
    assert same(got, want), (got, want)
    assert got["skipped"] == 1 and got["documents"] == len(docs) - 1 and got["tokens"] > 0 and np.isfinite(got["perplexity"])
    assert same(m.heldout_perplexity(docs, 6, 2, seed=77), got)          # and again, with ph_hat uploaded from the host
    unweighted = m.heldout_perplexity(docs, 6, 2, weighted=False, seed=77)
    assert same(unweighted, host_path(m, docs, 6, 2, seed=77, weighted=False)) and unweighted["tokens"] <= got["tokens"]
    # the caller's own pair: the first half of every token list observed, the second half scored
    a, b = [d[:len(d) // 2 + 1] for d in docs], [d[len(d) // 2 + 1:] for d in docs]
    pair = m.heldout_perplexity(a, 6, 2, seed=77, scored_docs=b)
    assert same(pair, host_path(m, a, 6, 2, seed=77, scored_docs=b)) and pair["skipped"] == 1
    with pytest.raises(ValueError):
        m.heldout_perplexity(a, 6, 2, scored_docs=b[:-1])
    none = m.heldout_perplexity([["no-such-token"]], 6, 2)
    assert none["documents"] == 0 and none["skipped"] == 1 and none["tokens"] == 0 and np.isnan(none["perplexity"])


def test_cli_heldout_perplexity(tmp_path, capsys, monkeypatch):
    """--heldout-perplexity prints the host path's number behind the report and changes nothing else; without it nothing is added"""
    from lda_thesis_amd import evaluate_LabeledLDA as H
    from test_gpu_rank_labels import _write_csv
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv)
    plain = capsys.readouterr().out.splitlines()
    np.random.seed(0)
    H.main(argv + ["-p", "--heldout-perplexity"])
    out = capsys.readouterr().out.splitlines()
    assert out[:len(plain)] == plain and len(out) == len(plain) + 3
    assert plain[-1].startswith("F1 score (macro average) ")
    assert out[-3] == "-----------------------------------"
    label = "Held-out perplexity (document completion):  "
    assert out[-2].startswith(label)
    model, test = (pickle.load(open(tmp_path / f, "rb")) for f in ("LabeledLDA_model.pkl", "LabeledLDA_testset.pkl"))
    known = set(model.vocab)
    want = host_path(model, [[x for x in doc if x in known] for doc in test[0]], 20, 5)
    assert float(out[-2][len(label):]) == want["perplexity"] and np.isfinite(want["perplexity"])
    assert out[-1] == "  scored tokens %d in %d documents (%d skipped), log-likelihood %s" % (
        want["tokens"], want["documents"], want["skipped"], want["loglik"])
