"""llda_credit_words on the device: bit for bit against its CPU restatement (tests/emref.py) at every seam of the geometry -- the
lane groups of K <= 32, the register forms up to K = 1024, the LDS form beyond -- and of the chunking, with guard words before and
behind every output and behind every output row, and NaN in every column >= K of both inputs."""
import numpy as np
import pytest

import emref
from test_gpu_attribute import V, W_ABOVE, W_BELOW, W_INF, W_NAN, W_ZERO, model

pytestmark = pytest.mark.gpu

MAX_K = 7688
KS = (1, 7, 8, 9, 32, 33, 64, 65, 128, 129, 512, 513, 1024, 1025, 1031, MAX_K)
# every K runs chunk = 3 and 64; 1, 65 and 4096 go round the kernel forms (groups of 8, 16, 32 lanes; 1 .. 16 registers; LDS)
MORE_CHUNKS = {1: (1,), 9: (1,), 65: (1,), 513: (1,), 1025: (1, 4096), 7: (65,), 32: (65,), 128: (65,), 1024: (65,), MAX_K: (65,),
               8: (4096,), 64: (4096,)}
FREQ_MODES = (None, "ones", "mixed")
GUARD = 8
MAX_F = 2 ** 23 - 1
D = 200
D_ZERO, D_NAN, D_INF = 0, 1, 2                                             # documents with a planted row of theta
HOT, PLANTED_LEN = 1003, 5
PATTERN = {"float64": np.float64(-1234.5), "int64": np.int64(-0x123456789ABCDEF)}
OUTPUTS = (("credit", "float64"), ("tok", "int64"), ("bad", "int64"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def plant_theta(rng, theta, K):
    theta[D_ZERO, :K] = 0.0                                                # p = 0
    theta[D_NAN, rng.integers(0, K)] = np.nan
    theta[D_INF, rng.integers(0, K)] = np.inf
    return theta


def run_lengths(rng, chunk):
    """sites of every word: the planted rows of phi_t, then 0, 1, chunk - 1, chunk, chunk + 1, 2 chunk and the hot word, then a mix"""
    lens = [PLANTED_LEN] * 5 + [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, HOT]
    small = (0, 1, 2, 5, min(chunk, 70), min(chunk, 70) + 1)
    return np.asarray(lens + list(rng.choice(small, size=V - len(lens))), dtype=np.int64)


def sites(rng, lens, freq_mode):
    """word_off, site_doc with ids -1 and D and the planted rows of theta among them, freq"""
    word_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(word_off[-1])
    site_doc = rng.integers(3, D, size=S).astype(np.int32)
    plant = rng.random(S)
    for d, lo in ((D_ZERO, 0.0), (D_NAN, 0.02), (D_INF, 0.04), (-1, 0.06), (D, 0.08)):
        site_doc[(plant >= lo) & (plant < lo + 0.02)] = d
    if freq_mode is None:
        return word_off, site_doc, None
    if freq_mode == "ones":
        return word_off, site_doc, np.ones(S, dtype=np.int32)
    freq = rng.integers(0, 10, size=S).astype(np.int32)                    # f = 0 included
    freq[rng.random(S) < 0.1] = MAX_F
    freq[rng.random(S) < 0.3] = 1
    return word_off, site_doc, freq


def run(theta, phi_t, word_off, site_doc, freq, K, chunk, skip=(), pad_out=2, n_docs=D):
    """one llda_credit_words call with guard words before and behind every output (and, with pad_out, behind every row of credit)
    -> dict of whole buffers"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    n_words, S = len(word_off) - 1, int(word_off[-1])
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_theta, d_phi, d_off, d_doc, d_freq = up(theta), up(phi_t), up(word_off), up(site_doc), up(freq)
    if d_doc.numel() == 0:
        d_doc = torch.zeros((1,), dtype=torch.int32, device=dev)
    ld = K + pad_out
    sizes = dict(credit=n_words * ld, tok=n_words, bad=n_words)
    bufs = {n: torch.full((sizes[n] + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    need = _native.credit_words_scratch_bytes(n_words, S, K, chunk)
    scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    outs = {n: b[GUARD:GUARD + sizes[n]] for n, b in bufs.items() if n not in skip}
    _native.credit_words(d_off, d_doc, d_freq, d_theta, d_phi, n_docs, n_words, S, K, chunk, scratch[:need], ld_theta=theta.shape[1],
                         ld_phi=phi_t.shape[1], ld_credit=ld, credit_w=outs.get("credit"), tok=outs.get("tok"), bad=outs.get("bad"))
    torch.cuda.synchronize()
    assert (scratch[need:] == 0xA5).all(), "written behind the scratch"
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def check(got, want, n_words, K, skip=(), what="", pad_out=2):
    ld = K + pad_out
    for name, dt in OUTPUTS:
        g, pat = got[name], PATTERN[dt]
        n = g.shape[0] - 2 * GUARD
        assert (g[:GUARD] == pat).all() and (g[GUARD + n:] == pat).all(), "%s: guard words around %s overwritten" % (what, name)
        body = g[GUARD:GUARD + n]
        if name in skip:
            assert (body == pat).all(), "%s: %s was written" % (what, name)
            continue
        w = want[name]
        if name == "credit":
            body = body.reshape(n_words, ld)
            assert (body[:, K:] == pat).all(), "%s: credit written behind column K" % what
            body = body[:, :K]
        diff = np.argwhere(bits(body) != bits(w))
        assert diff.shape[0] == 0, "%s: %s differs at %s: got %s want %s" % (what, name, diff[:5].tolist(), body[tuple(diff[0])], w[tuple(diff[0])])


@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_emref(K):
    rng = np.random.default_rng(31000 + K)
    for i, chunk in enumerate((3, 64) + MORE_CHUNKS.get(K, ())):
        freq_mode = FREQ_MODES[(KS.index(K) + i) % 3]
        theta, phi_t = model(rng, K, D)                                    # NaN in the columns >= K of both
        assert np.isnan(theta[:, K:]).all() and np.isnan(phi_t[:, K:]).all() and theta.shape[1] > K < phi_t.shape[1]
        plant_theta(rng, theta, K)
        lens = run_lengths(rng, chunk)
        word_off, site_doc, freq = sites(rng, lens, freq_mode)
        want = emref.credit_words_ref(theta, phi_t, word_off, site_doc, freq, chunk, K=K, D=D)
        what = "K %d chunk %d freq %s" % (K, chunk, freq_mode)
        # what the case is there for was met: both sides of the bound, every planted row, both ids outside, good and bad sites
        ordinary = theta[3:, :K]
        assert (emref.attrref.sum64(ordinary * phi_t[W_ABOVE, :K]) >= emref.MIN_P).all(), what
        assert (emref.attrref.sum64(ordinary * phi_t[W_BELOW, :K]) < emref.MIN_P).all(), what
        assert all((site_doc == d).any() for d in (D_ZERO, D_NAN, D_INF, -1, D)), what
        assert want["tok"][W_ABOVE] > 0 or freq_mode == "mixed"
        assert want["tok"][[W_ZERO, W_NAN, W_INF, W_BELOW]].sum() == 0 and want["bad"][[W_ZERO, W_NAN, W_INF, W_BELOW]].sum() > 0, what
        assert want["tok"].sum() > 0 and want["bad"][5:].sum() > 0 and not want["credit"][5].any(), what
        check(run(theta, phi_t, word_off, site_doc, freq, K, chunk), want, V, K, what=what)


def gather(ids, word_off, site_doc, freq):
    n = np.diff(word_off)[ids]
    s = np.concatenate([np.arange(word_off[v], word_off[v + 1]) for v in ids] + [np.zeros(0)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64), site_doc[s], None if freq is None else freq[s]


@pytest.mark.parametrize("K", (7, 65, 1031))
def test_batch_independence(K):
    """a word's row has the same bits alone, among the other words, with the words in reverse and with V doubled"""
    rng = np.random.default_rng(32000 + K)
    theta, phi_t = model(rng, K, D)
    plant_theta(rng, theta, K)
    chunk = 64
    lens = run_lengths(rng, chunk)
    lens[11] = 300                                                         # (the hot word: five chunks are enough here)
    word_off, site_doc, freq = sites(rng, lens, "mixed")
    want = emref.credit_words_ref(theta, phi_t, word_off, site_doc, freq, chunk, K=K, D=D)
    everything = run(theta, phi_t, word_off, site_doc, freq, K, chunk, pad_out=0)
    check(everything, want, V, K, what="among the others", pad_out=0)
    for v in (3, 5, 6, 8, 9, 10, 11):                                      # alone: V = 1
        off, docs, f = gather([v], word_off, site_doc, freq)
        got = run(theta, phi_t[v:v + 1], off, docs, f, K, chunk, pad_out=0)
        check(got, {n: want[n][v:v + 1] for n in want}, 1, K, what="word %d alone" % v, pad_out=0)
    back = list(range(V))[::-1]
    off, docs, f = gather(back, word_off, site_doc, freq)
    check(run(theta, phi_t[back], off, docs, f, K, chunk, pad_out=0), {n: want[n][back] for n in want}, V, K, what="reversed", pad_out=0)
    twice = list(range(V)) * 2
    off, docs, f = gather(twice, word_off, site_doc, freq)
    check(run(theta, phi_t[twice], off, docs, f, K, chunk, pad_out=0), {n: want[n][twice] for n in want}, 2 * V, K, what="V doubled", pad_out=0)


@pytest.mark.parametrize("K", (8, 129, 2000))
def test_every_output_may_be_null_and_no_site_at_all(K):
    rng = np.random.default_rng(33000 + K)
    theta, phi_t = model(rng, K, D)
    plant_theta(rng, theta, K)
    chunk = 3
    lens = run_lengths(rng, chunk)
    lens[11] = 40
    word_off, site_doc, freq = sites(rng, lens, "mixed")
    want = emref.credit_words_ref(theta, phi_t, word_off, site_doc, freq, chunk, K=K, D=D)
    for skip in (("credit",), ("tok",), ("bad",), ("credit", "tok"), ("credit", "tok", "bad")):
        check(run(theta, phi_t, word_off, site_doc, freq, K, chunk, skip=skip), want, V, K, skip=skip, what="K %d without %s" % (K, skip))
    # V words with no site at all: the zero rows are still written
    none = np.zeros(V + 1, dtype=np.int64)
    zero = dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=np.zeros(V, dtype=np.int64))
    check(run(theta, phi_t, none, site_doc[:0], None, K, chunk), zero, V, K, what="no site")
    # no document at all: every site is bad, no row of theta is read
    got = run(theta[:0], phi_t, word_off, site_doc, freq, K, chunk, n_docs=0)
    fsum = np.add.reduceat(np.append(freq, 0).astype(np.int64), word_off[:-1]) * (lens > 0)
    check(got, dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=fsum), V, K, what="no document")


def test_python_surface():
    """emfit.word_major and emfit.credit_words: numpy CSR in, device tensors out, strided matrices, and the refusals"""
    import torch
    from lda_thesis_amd import emfit
    from test_gpu_attribute import corpus
    rng = np.random.default_rng(34)
    K, n_docs = 40, 50
    theta, phi_t = model(rng, K, n_docs)
    doc_off, word, freq = corpus(rng, n_docs, (0, 1, 5, 20), "ones")
    freq = rng.integers(1, 6, size=freq.shape[0]).astype(np.int32)
    word[(word < 5) | (word >= V)] = 9
    dev = torch.device("cuda", 0)
    w_off, w_doc, w_freq, order = emref.word_major(doc_off, word, freq, V)
    got = emfit.word_major(doc_off, word, freq, V, dev)
    for g, w in zip(got, (w_off, w_doc, w_freq, order)):
        assert g.is_cuda and np.array_equal(g.cpu().numpy(), w) and g.cpu().numpy().dtype == w.dtype
    assert emfit.word_major(doc_off, word, None, V, dev)[2] is None
    d_theta, d_phi = torch.from_numpy(theta).to(dev)[:, :K], torch.from_numpy(phi_t).to(dev)[:, :K]      # row strides K + 3, K + 5
    for chunk in (2, 64):
        want = emref.credit_words_ref(theta, phi_t, w_off, w_doc, w_freq, chunk, K=K)
        r = emfit.credit_words(d_theta, d_phi, got[0], got[1], got[2], chunk=chunk)
        assert sorted(r) == ["bad", "credit", "tok"]
        for name in r:
            assert np.array_equal(bits(r[name].cpu().numpy()), bits(want[name])), (chunk, name)
    only = emfit.credit_words(d_theta, d_phi, w_off, w_doc, None, want=("tok",))
    assert sorted(only) == ["tok"] and np.array_equal(only["tok"].cpu().numpy(), np.diff(w_off) - emref.credit_words_ref(
        theta, phi_t, w_off, w_doc, None, 4096, K=K)["bad"])
    for bad in (dict(chunk=0), dict(w_off=w_off[:-1]), dict(w_doc=np.where(w_doc == w_doc.max(), n_docs, w_doc)), dict(w_doc=w_doc[:-1]),
                dict(w_freq=np.full_like(w_freq, 2 ** 23)), dict(phi=d_phi[:, :K - 1]), dict(theta=theta), dict(want=("credit", "all"))):
        args = dict(theta=d_theta, phi=d_phi, w_off=w_off, w_doc=w_doc, w_freq=w_freq, chunk=64, want=("credit",))
        args.update(bad)
        with pytest.raises(ValueError):
            emfit.credit_words(args["theta"], args["phi"], args["w_off"], args["w_doc"], args["w_freq"], chunk=args["chunk"], want=args["want"])
    with pytest.raises(ValueError):
        emfit.word_major(doc_off, np.where(word == 9, V, word), freq, V, dev)
