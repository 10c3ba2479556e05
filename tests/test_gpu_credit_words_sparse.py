"""llda_credit_words_sparse on the device: bit for bit against its CPU restatement (tests/sparseref.py) at every lane group, on
both sides of every chunk seam, with sites of one wavefront step that share a label and whose order of addition shows in the last
bit, and -- for prefix label sets -- against the dense llda_credit_words on the device at full K; guard words before and behind
every output and behind every output row."""
import numpy as np
import pytest

import sparseref
from test_gpu_attribute import MAX_F, W_ABOVE, W_BELOW, W_INF, W_NAN, W_ZERO
from test_gpu_attribute_sparse import D, KS, MAX_LABELS, V, label_sets, phi_model
from test_gpu_credit_words import GUARD, OUTPUTS, PATTERN, bits, check
from test_gpu_credit_words import run as run_dense

pytestmark = pytest.mark.gpu

MAX_K = 7688
HOT = 1003                                                                 # (the chunks run are 1, 3, 64 and 4096)
D_ONE, D_SMALL = 4, (5, 6, 7)                                              # the documents of the planted order words
W_UP, W_DOWN, W_SAME = 17, 18, 19                                          # the order words: big share first, last; one document repeated
SMALL = 0.75 * 2.0 ** -53


def plant_order(K, lab_off, lab, theta_s, phi_t):
    """document D_ONE carries the root alone (share 1.0 of the root's column), the documents D_SMALL the root with a load of
    0.75 * 2^-53 beside a label with load 1.0; the order words have one constant row of phi_t.  1.0 and then 0.75 * 2^-53 again and
    again stays 1.0; three of them first and 1.0 after them is 1.0 + 2^-52, and stays there."""
    sets = [lab[lab_off[d]:lab_off[d + 1]] for d in range(len(lab_off) - 1)]
    loads = [theta_s[lab_off[d]:lab_off[d + 1]] for d in range(len(lab_off) - 1)]
    sets[D_ONE], loads[D_ONE] = np.array([0], dtype=np.int32), np.array([1.0])
    for i, d in enumerate(D_SMALL):
        sets[d], loads[d] = np.array([0, K - 2 - i], dtype=np.int32), np.array([SMALL, 1.0])
    for w in (W_UP, W_DOWN, W_SAME):
        phi_t[w, :K] = 2.0 ** -7
    return np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64), np.concatenate(sets), np.concatenate(loads)


def run_lengths(rng, chunk):
    """sites of every word: the planted rows of phi_t, then 0, 1, chunk - 1, chunk, chunk + 1, 2 chunk and a hot word of many chunks,
    the order words, then a mix"""
    lens = [5] * 5 + [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, HOT if chunk <= 64 else 3 * chunk + 7]
    lens += [0] * (W_UP - len(lens)) + [8, 8, 8]
    small = (0, 1, 2, 5, min(chunk, 70), min(chunk, 70) + 1)
    return np.asarray(lens + list(rng.choice(small, size=V - len(lens))), dtype=np.int64)


def sites(rng, lens, freq_mode, n_docs=D):
    """word_off, site_doc with ids -1 and D, unfit documents and the order words among them, freq"""
    word_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    S = int(word_off[-1])
    site_doc = rng.integers(8, n_docs, size=S).astype(np.int32)
    plant = rng.random(S)
    for d, lo in ((0, 0.0), (1, 0.01), (2, 0.02), (3, 0.03), (-1, 0.04), (n_docs, 0.06)):
        site_doc[(plant >= lo) & (plant < lo + (0.02 if d in (-1, n_docs) else 0.01))] = d
    freq = None
    if freq_mode == "mixed":
        freq = rng.integers(0, 10, size=S).astype(np.int32)                # f = 0 included
        freq[rng.random(S) < 0.1] = MAX_F
        freq[rng.random(S) < 0.3] = 1
    one, (a, b, c) = D_ONE, D_SMALL
    for w, docs in ((W_UP, (one, a, b, c, a, b, c, a)), (W_DOWN, (a, b, c, one, a, b, c, a)), (W_SAME, (one, one, a, a, a, one, b, b))):
        site_doc[word_off[w]:word_off[w + 1]] = docs
        if freq is not None:
            freq[word_off[w]:word_off[w + 1]] = 1
    return word_off, site_doc, freq


def run(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, K, max_labels, chunk, skip=(), pad_out=2):
    """one llda_credit_words_sparse call with guard words before and behind every output (and, with pad_out, behind every row of
    credit) -> dict of whole buffers"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    n_words, S, NL, n_docs = len(word_off) - 1, int(word_off[-1]), len(lab), len(lab_off) - 1
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_phi, d_off, d_doc, d_freq, d_loff = up(phi_t), up(word_off), up(site_doc), up(freq), up(lab_off)
    d_lab = up(lab) if NL else torch.zeros((1,), dtype=torch.int32, device=dev)
    d_th = up(theta_s) if NL else torch.zeros((1,), dtype=torch.float64, device=dev)
    if d_doc.numel() == 0:
        d_doc = torch.zeros((1,), dtype=torch.int32, device=dev)
    ld = K + pad_out
    sizes = dict(credit=n_words * ld, tok=n_words, bad=n_words)
    bufs = {n: torch.full((sizes[n] + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    need = _native.credit_words_sparse_scratch_bytes(n_words, S, K, chunk)
    scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    outs = {n: b[GUARD:GUARD + sizes[n]] for n, b in bufs.items() if n not in skip}
    _native.credit_words_sparse(d_off, d_doc, d_freq, d_loff, d_lab, d_th, d_phi, n_docs, n_words, S, K, NL, max_labels, chunk,
                                scratch[:need], ld_phi=phi_t.shape[1], ld_credit=ld, credit_w=outs.get("credit"), tok=outs.get("tok"),
                                bad=outs.get("bad"))
    torch.cuda.synchronize()
    assert (scratch[need:] == 0xA5).all(), "written behind the scratch"
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def case(rng, K, max_labels, chunk, freq_mode, prefix=False):
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, max_labels, prefix=prefix, unfit=not prefix)
    if not prefix:
        lab_off, lab, theta_s = plant_order(K, lab_off, lab, theta_s, phi_t)
    word_off, site_doc, freq = sites(rng, run_lengths(rng, chunk), freq_mode)
    return phi_t, lab_off, lab, theta_s, word_off, site_doc, freq


def one_case(K, max_labels, chunk, freq_mode, seed):
    rng = np.random.default_rng(seed)
    phi_t, lab_off, lab, theta_s, word_off, site_doc, freq = case(rng, K, max_labels, chunk, freq_mode)
    want = sparseref.credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk, K=K, max_labels=max_labels)
    what = "K %d max_labels %d chunk %d freq %s" % (K, max_labels, chunk, freq_mode)
    # what the case is there for was met: unfit documents and ids outside among the sites, the planted rows, the order of addition
    assert all((site_doc == d).any() for d in (0, 1, 2, 3, -1, D)), what
    assert want["tok"][[W_ZERO, W_NAN, W_INF, W_BELOW]].sum() == 0 and want["bad"][[W_ZERO, W_NAN, W_INF, W_BELOW]].sum() > 0, what
    assert want["tok"][W_ABOVE] > 0 or freq_mode == "mixed", what
    assert want["tok"].sum() > 0 and want["bad"][5:].sum() > 0 and not want["credit"][5].any(), what
    if chunk >= 8:                                                         # (smaller chunks cut the planted runs apart)
        up, down = want["credit"][W_UP, 0], want["credit"][W_DOWN, 0]
        assert up == 1.0 and down == 1.0 + 2.0 ** -52, (what, up, down)
    check(run(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, K, max_labels, chunk), want, V, K, what=what)


@pytest.mark.parametrize("max_labels", MAX_LABELS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_sparseref(K, max_labels):
    i = KS.index(K) * len(MAX_LABELS) + MAX_LABELS.index(max_labels)
    for j, chunk in enumerate((3, 64, (1, 4096)[i % 2])):
        one_case(K, max_labels, chunk, (None, "mixed")[(i + j) % 2], 51000 + 100 * K + 10 * max_labels + j)


def test_the_largest_k_sizes_its_lds():
    """K = LLDA_MAX_K: 61 504 bytes of sums, one wavefront per workgroup"""
    one_case(MAX_K, 8, 64, "mixed", 52000)


@pytest.mark.parametrize("K,max_labels,chunk", ((33, 8, 64), (33, 32, 3), (512, 16, 64), (2048, 32, 4096), (2048, 8, 1)))
def test_prefix_label_sets_give_the_bits_of_the_dense_kernel_at_full_k(K, max_labels, chunk):
    rng = np.random.default_rng(53000 + K + max_labels)
    phi_t, lab_off, lab, theta_s, word_off, site_doc, freq = case(rng, K, max_labels, chunk, "mixed", prefix=True)
    theta = sparseref.scatter(theta_s, lab_off, lab, K)
    dense = run_dense(theta, phi_t, word_off, site_doc, freq, K, chunk, n_docs=D)
    got = run(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, K, max_labels, chunk)
    for name, _ in OUTPUTS:
        assert np.array_equal(bits(got[name]), bits(dense[name])), name
    assert got["tok"][GUARD:-GUARD].sum() > 0 and got["bad"][GUARD:-GUARD].sum() > 0


def gather(ids, word_off, site_doc, freq):
    n = np.diff(word_off)[ids]
    s = np.concatenate([np.arange(word_off[v], word_off[v + 1]) for v in ids] + [np.zeros(0)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64), site_doc[s], None if freq is None else freq[s]


@pytest.mark.parametrize("K,max_labels", ((33, 16), (2048, 8)))
def test_batch_independence(K, max_labels):
    """a word's row has the same bits alone, among the other words, with the words in reverse and with V doubled"""
    rng = np.random.default_rng(54000 + K)
    chunk = 64
    phi_t, lab_off, lab, theta_s, word_off, site_doc, freq = case(rng, K, max_labels, chunk, "mixed")
    want = sparseref.credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk, K=K, max_labels=max_labels)
    check(run(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, K, max_labels, chunk, pad_out=0), want, V, K, what="among the others", pad_out=0)
    for v in (3, 6, 8, 9, 11, W_UP, W_DOWN):                               # alone: V = 1
        off, docs, f = gather([v], word_off, site_doc, freq)
        got = run(theta_s, phi_t[v:v + 1], off, docs, f, lab_off, lab, K, max_labels, chunk, pad_out=0)
        check(got, {n: want[n][v:v + 1] for n in want}, 1, K, what="word %d alone" % v, pad_out=0)
    back = list(range(V))[::-1]
    off, docs, f = gather(back, word_off, site_doc, freq)
    check(run(theta_s, phi_t[back], off, docs, f, lab_off, lab, K, max_labels, chunk, pad_out=0), {n: want[n][back] for n in want}, V, K,
          what="reversed", pad_out=0)
    twice = list(range(V)) * 2
    off, docs, f = gather(twice, word_off, site_doc, freq)
    check(run(theta_s, phi_t[twice], off, docs, f, lab_off, lab, K, max_labels, chunk, pad_out=0), {n: want[n][twice] for n in want}, 2 * V, K,
          what="V doubled", pad_out=0)


@pytest.mark.parametrize("K,max_labels", ((33, 8), (2048, 32)))
def test_every_output_may_be_null_and_no_site_at_all(K, max_labels):
    rng = np.random.default_rng(55000 + K)
    chunk = 3
    phi_t, lab_off, lab, theta_s, word_off, site_doc, freq = case(rng, K, max_labels, chunk, "mixed")
    want = sparseref.credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk, K=K, max_labels=max_labels)
    for skip in (("credit",), ("tok",), ("bad",), ("credit", "tok"), ("credit", "tok", "bad")):
        got = run(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, K, max_labels, chunk, skip=skip)
        check(got, want, V, K, skip=skip, what="K %d without %s" % (K, skip))
    # V words with no site at all: the zero rows are still written
    none = np.zeros(V + 1, dtype=np.int64)
    zero = dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=np.zeros(V, dtype=np.int64))
    check(run(theta_s, phi_t, none, site_doc[:0], None, lab_off, lab, K, max_labels, chunk), zero, V, K, what="no site")
    # no document at all: every site is bad, no label set is read
    got = run(np.zeros(0), phi_t, word_off, site_doc, freq, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), K, max_labels, chunk)
    fsum = np.add.reduceat(np.append(freq, 0).astype(np.int64), word_off[:-1]) * (np.diff(word_off) > 0)
    check(got, dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=fsum), V, K, what="no document")


def test_python_surface():
    """emfit.credit_words_sparse: numpy CSRs in, device tensors out, strided phi_t, and the refusals on the host"""
    import torch
    from lda_thesis_amd import emfit
    rng = np.random.default_rng(56)
    K, n_docs = 40, 50
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, 16, n_docs=n_docs, unfit=False)
    word_off, site_doc, freq = sites(rng, run_lengths(rng, 16), "mixed", n_docs=n_docs)
    site_doc = np.clip(site_doc, 0, n_docs - 1)
    dev = torch.device("cuda", 0)
    d_phi, d_th = torch.from_numpy(phi_t).to(dev)[:, :K], torch.from_numpy(theta_s).to(dev)          # row stride K + 5
    for chunk in (2, 64):
        want = sparseref.credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk, K=K)
        r = emfit.credit_words_sparse(d_th, d_phi, word_off, site_doc, freq, lab_off, lab, chunk=chunk)
        assert sorted(r) == ["bad", "credit", "tok"]
        for name in r:
            assert np.array_equal(bits(r[name].cpu().numpy()), bits(want[name])), (chunk, name)
    only = emfit.credit_words_sparse(d_th, d_phi, word_off, site_doc, None, lab_off, lab, want=("tok",))
    assert sorted(only) == ["tok"]
    twice = lab.copy()
    d = int(np.flatnonzero(np.diff(lab_off) >= 2)[0])
    twice[lab_off[d] + 1] = twice[lab_off[d]]
    for bad in (dict(chunk=0), dict(w_off=word_off[:-1]), dict(w_doc=np.where(site_doc == site_doc.max(), n_docs, site_doc)),
                dict(w_doc=site_doc[:-1]), dict(w_freq=np.full_like(freq, 2 ** 23)), dict(theta=theta_s), dict(theta=d_th[:-1]),
                dict(lab=twice), dict(lab=np.where(lab == lab.max(), K, lab)), dict(lab_off=lab_off[1:]), dict(want=("credit", "all"))):
        args = dict(theta=d_th, phi=d_phi, w_off=word_off, w_doc=site_doc, w_freq=freq, lab_off=lab_off, lab=lab, chunk=64, want=("credit",))
        args.update(bad)
        with pytest.raises(ValueError):
            emfit.credit_words_sparse(args["theta"], args["phi"], args["w_off"], args["w_doc"], args["w_freq"], args["lab_off"], args["lab"],
                                      chunk=args["chunk"], want=args["want"])
