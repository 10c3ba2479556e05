"""llda_heldout_loglik_sparse on the device: bit for bit against its CPU restatement (tests/sparseheldref.py) at every lane group and
on both sides of every group seam, with unfit documents of every kind next to fit ones, planted sites whose p is 0, denormal or
inf, word ids outside the vocabulary, guard words around every output -- and, for prefix label sets, against the dense
llda_heldout_loglik on the scattered theta."""
import functools

import numpy as np
import pytest

import sparseheldref
import sparseref
from test_gpu_heldout import GUARD, MAX_F, OUTPUTS, PATTERN, check
from test_gpu_heldout import run as run_dense

pytestmark = pytest.mark.gpu

KS = (5, 40, 392, 1031, 2048)
MAX_LABELS = (1, 8, 9, 16, 17, 32)
D, V = 67, 61                                                             # 67: the last tile of a workgroup is partial for every group
LENS = (0, 1, 2, 63, 64, 65, 130, 5)                                      # document d has LENS[d % 8] sites: all of them in one wavefront of 8
W_ZERO, W_TINY, W_INF, W_BIG = 0, 1, 2, 3                                 # words with a planted row of phi_t
# documents with a planted label list, each between fit documents of its wavefront; the two with offsets outside [0, NL] can only
# stand at the ends of a CSR whose other documents are fit
U_FRONT, U_LONG, U_TWICE, U_DOWN, U_HIGH, U_NEG, U_EMPTY, U_BEYOND = 0, 10, 12, 21, 23, 33, 35, D - 1
UNFIT = (U_FRONT, U_LONG, U_TWICE, U_DOWN, U_HIGH, U_NEG, U_BEYOND)


def phi_model(rng, K, pad=5):
    """phi_t (V, K + pad), NaN in every column >= K (ld_phi > K); the planted rows: all zero (p = 0), denormal entries (p denormal or
    0), an inf in column 0 -- the root, which every document with a label carries -- and entries near the largest double (p
    overflows for the documents whose loads add up to more than 1.2)"""
    phi_t = np.full((V, K + pad), np.nan)
    phi_t[:, :K] = rng.gamma(0.2, size=(V, K)) / V + 1e-9
    phi_t[W_ZERO, :K] = 0.0
    phi_t[W_TINY, :K] = rng.choice([5e-324, 3e-310, 1e-308, 7e-315], size=K)
    phi_t[W_INF, 0] = np.inf
    phi_t[W_BIG, :K] = 1.5e308
    return phi_t


def label_sets(rng, K, max_labels, n_docs=D, prefix=False, planted=True):
    """(lab_off, lab, theta_s, NL): scattered lists that reach K - 1 and do not ascend from document to document, every count the
    group allows, exact zero loads, loads that add up to 2 in every fifth document; planted: the unfit documents and L_d = 0"""
    top = min(max_labels, K)
    counts = sorted(set(c for c in (1, 2, 7, 8, 9, 15, 16, 17, 31, 32) if c <= top) | {top})
    sets, loads = [], []
    for d in range(n_docs):
        L = counts[d % len(counts)]
        if prefix:
            ids = np.arange(L)
        else:
            ids = np.sort(np.concatenate([[0], 1 + rng.choice(K - 1, size=L - 1, replace=False)])) if K > 1 else np.zeros(1, dtype=np.int64)
            if L > 1 and d % 3 == 0:
                ids[-1] = K - 1
        t = rng.gamma(0.5, size=L) + 1e-3
        if L > 2:
            t[1 + np.flatnonzero(rng.random(L - 1) < 0.2)] = 0.0
        t = t / t.sum() * (2.0 if d % 5 == 0 else 1.0)
        sets.append(ids.astype(np.int64))
        loads.append(t)
    if planted:
        some = lambda n: np.sort(rng.choice(K, size=n, replace=False)) if n <= K else np.arange(n)
        sets[U_LONG] = some(max_labels + 1)                               # (K < max_labels + 1: an id >= K as well)
        sets[U_TWICE] = np.array([0, 0])
        sets[U_DOWN] = np.array([min(2, K - 1), 0])
        sets[U_HIGH] = np.array([K])
        sets[U_NEG] = np.array([-1])
        sets[U_EMPTY] = np.zeros(0, dtype=np.int64)
        for d in (U_LONG, U_TWICE, U_DOWN, U_HIGH, U_NEG, U_EMPTY):
            loads[d] = np.full(len(sets[d]), 0.5)
        if max_labels == 1:                                               # (two ids do not fit the call at all: unfit by their count)
            assert len(sets[U_TWICE]) > max_labels and len(sets[U_DOWN]) > max_labels
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    lab, theta_s = np.concatenate(sets).astype(np.int32), np.concatenate(loads)
    NL = int(lab_off[-1])
    if planted:
        lab_off[0] = -1                                                   # document 0 starts before the array
        NL = int(lab_off[-1]) - 1                                         # the last document ends behind what the caller states
    return lab_off, lab, theta_s, NL


def corpus(rng, n_docs, freq_mode):
    n = np.asarray([LENS[d % len(LENS)] for d in range(n_docs)])
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(4, V, size=S).astype(np.int32)
    plant = rng.random(S)
    for w, lo in ((W_ZERO, 0.0), (W_TINY, 0.02), (W_INF, 0.08), (W_BIG, 0.10), (-1, 0.14), (V, 0.16), (2 ** 31 - 1, 0.18)):
        word[(plant >= lo) & (plant < lo + (0.06 if w == W_TINY else 0.04 if w == W_BIG else 0.02))] = w
    if freq_mode is None:
        return doc_off, word, None
    freq = rng.choice(np.array([0, 1, 2, 3, 7, MAX_F], dtype=np.int32), size=S, p=[0.1, 0.4, 0.15, 0.15, 0.1, 0.1])
    return doc_off, word, freq


def run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, NL=None, skip=()):
    """one llda_heldout_loglik_sparse call with guard words before and behind every output -> dict of whole buffers.  lab and theta_s
    are physically longer than NL: nothing beyond NL may be READ, which the poison there shows (an id of 2^30, a NaN load)"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    n_docs = len(doc_off) - 1
    NL = len(lab) if NL is None else NL
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lab_p = np.concatenate([lab[:NL], np.full(40, 2 ** 30)]).astype(np.int32)
    th_p = np.concatenate([theta_s[:NL], np.full(40, np.nan)])
    d_word = up(word) if len(word) else torch.zeros((1,), dtype=torch.int32, device=dev)
    bufs = {n: torch.full((n_docs + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    _native.heldout_loglik_sparse(up(doc_off), d_word, up(freq), up(lab_off), up(lab_p), up(th_p), up(phi_t), n_docs, V, K, NL, max_labels,
                                  ld_phi=phi_t.shape[1], **{n: b[GUARD:GUARD + n_docs] for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


@functools.lru_cache(maxsize=None)
def case(K, max_labels):
    """the inputs of one (K, max_labels) and what the restatement makes of them, computed once"""
    rng = np.random.default_rng(51000 + 100 * K + max_labels)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s, NL = label_sets(rng, K, max_labels)
    doc_off, word, freq = corpus(rng, D, None if (K + max_labels) % 2 else "mixed")
    want = sparseheldref.loglik_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=K, V=V, max_labels=max_labels, NL=NL)
    return phi_t, lab_off, lab, theta_s, NL, doc_off, word, freq, want


@pytest.mark.parametrize("max_labels", MAX_LABELS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_the_restatement(K, max_labels):
    phi_t, lab_off, lab, theta_s, NL, doc_off, word, freq, want = case(K, max_labels)
    what = "K %d max_labels %d freq %s" % (K, max_labels, freq is not None)
    fit = np.asarray([sparseref.doc_fit(lab_off, lab, d, K, max_labels, NL)[0] for d in range(D)])
    assert sorted(np.flatnonzero(~fit)) == sorted(UNFIT), what
    for d in UNFIT[:-1]:                                                # each one next to a fit document of its own wavefront
        assert any(0 <= e < D and fit[e] and e // 2 == d // 2 for e in (d - 1, d + 1)), (what, d)
    mant, expo, tok, bad = want
    fsum = np.add.reduceat(np.append(np.ones(len(word), dtype=np.int64) if freq is None else freq.astype(np.int64), 0), doc_off[:-1]) * (np.diff(doc_off) > 0)
    gone = list(UNFIT) + [U_EMPTY]
    assert (tok[gone] == 0).all() and (bad[gone] == fsum[gone]).all() and (mant[gone] == 0.5).all() and (expo[gone] == 1).all(), what
    assert bad[gone].sum() > 0 and tok[fit].sum() > 0 and bad[fit].sum() > 0, what
    # what the planted rows are there for was met by a fit document: p = 0, p denormal, p = inf by overflow
    seen = set()
    for d in np.flatnonzero(fit & (np.diff(lab_off) > 0)):
        th, cols = theta_s[lab_off[d]:lab_off[d + 1]], lab[lab_off[d]:lab_off[d + 1]].astype(np.int64)
        ws = set(word[doc_off[d]:doc_off[d + 1]].tolist())
        with np.errstate(all="ignore"):
            for w in (W_ZERO, W_TINY, W_BIG):
                if w in ws:
                    p = sparseref.attrref.sum64((th * phi_t[w, cols])[None, :])[0]
                    seen.add("zero" if p == 0.0 else "denormal" if p < 2.3e-308 else "inf" if p == np.inf else "normal")
    assert {"zero", "denormal", "inf"} <= seen, (what, seen)
    assert all((word == w).any() for w in (-1, V, 2 ** 31 - 1)) and lab.max() >= K - 1, what
    assert freq is None or set(freq.tolist()) >= {0, 1, 2, 3, MAX_F}
    check(run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, NL), want, D, what=what)


@pytest.mark.parametrize("K,max_labels", ((5, 8), (392, 17), (2048, 32)))
def test_every_output_may_be_null(K, max_labels):
    phi_t, lab_off, lab, theta_s, NL, doc_off, word, freq, want = case(K, max_labels)
    for skip in (("mant",), ("expo",), ("tok",), ("bad",), ("mant", "expo", "tok", "bad")):
        got = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, NL, skip=skip)
        check(got, want, D, skip=skip, what="K %d without %s" % (K, skip))
    import torch
    from lda_thesis_amd import _native
    t = torch.zeros((1, K), dtype=torch.float64, device="cuda:0")
    _native.heldout_loglik_sparse(None, None, None, None, None, None, t, 0, 1, K, 0, max_labels)      # D = 0: a no-op


@pytest.mark.parametrize("K,max_labels", ((40, 8), (1031, 9), (2048, 32)))
def test_batch_independence(K, max_labels):
    """a fit and an unfit document: alone, and at position 66 of a batch, the bits they have in the middle of the whole batch"""
    phi_t, lab_off, lab, theta_s, NL, doc_off, word, freq, want = case(K, max_labels)
    for d in (38, U_TWICE, U_EMPTY):                                    # (38: 130 sites)
        sites, slots = np.arange(doc_off[d], doc_off[d + 1]), np.arange(lab_off[d], lab_off[d + 1])
        one = [np.asarray([w[d]]) for w in want]
        f1 = None if freq is None else freq[sites]
        alone = run(theta_s[slots], phi_t, np.array([0, len(sites)]), word[sites], f1, np.array([0, len(slots)]), lab[slots], K, max_labels)
        check(alone, one, 1, what="K %d document %d alone" % (K, d))
        # position 66: behind the 66 first documents of the batch, whose label lists are compacted to fit ones
        head = np.arange(doc_off[66])
        off = np.concatenate([doc_off[:67], [doc_off[66] + len(sites)]])
        loff = np.concatenate([[0], np.cumsum([1] * 66), [66 + len(slots)]]).astype(np.int64)
        lab2 = np.concatenate([np.zeros(66, dtype=np.int32), lab[slots]])
        th2 = np.concatenate([np.full(66, 0.25), theta_s[slots]])
        f2 = None if freq is None else np.concatenate([freq[head], freq[sites]])
        last = run(th2, phi_t, off, np.concatenate([word[head], word[sites]]), f2, loff, lab2, K, max_labels)
        for (name, _), w in zip(OUTPUTS, one):
            g = last[name][GUARD + 66]
            assert g.tobytes() == np.asarray(w[0], dtype=g.dtype).tobytes(), "K %d document %d at position 66: %s" % (K, d, name)


@pytest.mark.parametrize("K,max_labels", ((40, 8), (40, 32), (392, 16), (392, 9)))
def test_prefix_label_sets_give_the_bits_of_the_dense_kernel(K, max_labels):
    """labels 0 .. L_d - 1, the dense row +0.0 elsewhere: llda_heldout_loglik at full K gives the same bits"""
    rng = np.random.default_rng(52000 + K + max_labels)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s, NL = label_sets(rng, K, max_labels, prefix=True, planted=False)
    doc_off, word, freq = corpus(rng, D, "mixed")
    theta = sparseref.scatter(theta_s, lab_off, lab, K)
    dense = run_dense(theta, phi_t, doc_off, word, freq, K, n_vocab=V)
    got = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels)
    for name, _ in OUTPUTS:
        assert got[name].tobytes() == dense[name].tobytes(), name
    assert got["tok"][GUARD:GUARD + D].sum() > 0 and got["bad"][GUARD:GUARD + D].sum() > 0


def test_python_surface():
    """heldout.loglik_sparse: numpy CSRs in, numpy results out, weighted=False, and the refusals on the host"""
    import torch
    from lda_thesis_amd import heldout
    rng = np.random.default_rng(53)
    K = 40
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s, _ = label_sets(rng, K, 8, planted=False)
    doc_off, word, freq = corpus(rng, D, "mixed")
    word[(word < 0) | (word >= V)] = 9
    dev = torch.device("cuda", 0)
    d_phi, d_th = torch.from_numpy(phi_t).to(dev)[:, :K], torch.from_numpy(theta_s).to(dev)          # row stride K + 5
    for weighted in (True, False):
        want = sparseheldref.loglik_sparse_ref(theta_s, phi_t, doc_off, word, freq if weighted else None, lab_off, lab, K=K)
        got = heldout.loglik_sparse(d_th, d_phi, doc_off, word, freq, lab_off, lab, weighted=weighted)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    down = lab.copy()
    d = int(np.flatnonzero(np.diff(lab_off) >= 2)[0])
    down[lab_off[d]:lab_off[d] + 2] = down[lab_off[d]:lab_off[d] + 2][::-1]
    for bad in (dict(lab=down), dict(lab=np.where(lab == lab.max(), K, lab)), dict(lab_off=lab_off[:-1]), dict(theta=d_th[:-1]),
                dict(theta=theta_s), dict(word=np.where(word == 9, V, word))):
        args = dict(theta=d_th, lab_off=lab_off, lab=lab, word=word)
        args.update(bad)
        with pytest.raises(ValueError):
            heldout.loglik_sparse(args["theta"], d_phi, doc_off, args["word"], freq, args["lab_off"], args["lab"])
