"""llda_attribute_sparse on the device: bit for bit against its CPU restatement (tests/sparseref.py), against the DENSE llda_attribute
on the device on every document's compacted problem, and -- for prefix label sets -- against the dense llda_attribute at full K; at
every lane group (max_labels 8, 16, 32), with label counts on both sides of every group seam, unfit documents of every kind, and
guard words before and behind every output."""
import numpy as np
import pytest

import attrref
import sparseref
from test_gpu_attribute import GUARD, MAX_F, PATTERN, W_ABOVE, W_BELOW, W_INF, W_NAN, W_ZERO, bits
from test_gpu_attribute import run as run_dense

pytestmark = pytest.mark.gpu

KS = (33, 512, 2048)
MAX_LABELS = (8, 16, 32)
COUNTS = (0, 1, 7, 8, 9, 16, 17, 32)
LENS = (0, 1, 3, 4, 5, 63, 64, 65, 130)
D, V = 200, 101
OUTPUTS = (("theta_out", "float64"), ("credit", "float64"), ("site_idx", "int32"), ("site_val", "float64"), ("tok", "int64"),
           ("bad", "int64"))
# (iters, alpha, top_m, freq mode): iters 0 / 1 / 3 with alpha 0 and > 0, top_m 0 / 1 / 4, with and without frequencies
SETTINGS = ((0, 0.0, 1, "mixed"), (1, 0.1, 4, None), (3, 0.0, 0, "mixed"), (3, 0.1, 4, "mixed"), (1, 0.0, 0, None), (0, 0.1, 4, "mixed"))
UNFIT_LONG, UNFIT_ID, UNFIT_TWICE, UNFIT_DOWN = 0, 1, 2, 3                # documents with a planted label list


def phi_model(rng, K, pad=5):
    """phi_t (V, K + pad), NaN in every column >= K; columns 0 and K - 1 equal (ties); the planted rows of test_gpu_attribute.py with
    their NaN / inf in column 0, the root every document with a label carries"""
    phi_t = np.full((V, K + pad), np.nan)
    phi_t[:, :K] = rng.gamma(0.2, size=(V, K)) / V + 1e-9
    phi_t[:, K - 1] = phi_t[:, 0]
    phi_t[W_ZERO, :K] = 0.0
    phi_t[W_NAN, 0] = np.nan
    phi_t[W_INF, 0] = np.inf
    phi_t[W_ABOVE, :K] = 2.0 ** -960 * (1 + 2.0 ** -20)
    phi_t[W_BELOW, :K] = 2.0 ** -960 * (1 - 2.0 ** -20)
    return phi_t


def label_sets(rng, K, max_labels, n_docs=D, prefix=False, unfit=True):
    """lab_off, lab, theta_s: every count of COUNTS that max_labels allows, the root in every list, K - 1 in every third with the
    root's load (an exact tie, the largest load of the list), an exact zero here and there, the loads of a document summing to 1;
    unfit: the four planted documents"""
    counts = [c for c in COUNTS if c <= max_labels]
    sets, loads = [], []
    for d in range(n_docs):
        L = counts[d % len(counts)] if d >= 4 or not unfit else 3
        if prefix:
            ids = np.arange(L)
        else:
            ids = np.zeros(L, dtype=np.int64)
            if L > 1:
                rest = 1 + rng.choice(K - 2, size=L - 1, replace=False)
                if d % 3 == 0:
                    rest[0] = K - 1
                ids[1:] = rest
            ids = np.sort(ids)
        t = rng.gamma(0.5, size=L) + 1e-3
        if L > 2:
            t[rng.random(L) < 0.15] = 0.0
        if L:
            t[0] = t.max() + 0.25
            if L > 1 and ids[-1] == K - 1:
                t[-1] = t[0]
            t = t / t.sum()
        sets.append(ids)
        loads.append(t)
    if unfit:
        sets[UNFIT_LONG] = np.sort(rng.choice(K, size=max_labels + 1, replace=False))
        loads[UNFIT_LONG] = np.full(max_labels + 1, 1.0 / (max_labels + 1))
        sets[UNFIT_ID] = np.array([0, 5, K])
        sets[UNFIT_TWICE] = np.array([0, 7, 7])
        sets[UNFIT_DOWN] = np.array([0, 9, 8])
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return lab_off, np.concatenate(sets).astype(np.int32), np.concatenate(loads)


def corpus(rng, n_docs, freq_mode):
    """every length of LENS, the planted words and both words outside the vocabulary among the sites"""
    n = np.asarray([LENS[(d // 3 + d) % len(LENS)] for d in range(n_docs)])
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(5, V, size=S).astype(np.int32)
    plant = rng.random(S)
    for w, lo in ((W_ZERO, 0.0), (W_NAN, 0.02), (W_INF, 0.04), (W_ABOVE, 0.06), (W_BELOW, 0.10), (V, 0.14), (-1, 0.16)):
        word[(plant >= lo) & (plant < lo + (0.04 if w in (W_ABOVE, W_BELOW) else 0.02))] = w
    if freq_mode is None:
        return doc_off, word, None
    freq = rng.integers(0, 10, size=S).astype(np.int32)                   # f = 0 included
    freq[rng.random(S) < 0.1] = MAX_F
    freq[rng.random(S) < 0.3] = 1
    return doc_off, word, freq


def run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, iters=0, alpha=0.0, top_m=0, skip=()):
    """one llda_attribute_sparse call with guard words before and behind every output -> dict of whole buffers"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    n_docs, S, NL = len(doc_off) - 1, int(doc_off[-1]), len(lab)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_phi, d_off, d_word, d_freq, d_loff = up(phi_t), up(doc_off), up(word), up(freq), up(lab_off)
    d_lab = up(lab) if NL else torch.zeros((1,), dtype=torch.int32, device=dev)
    d_th = up(theta_s) if NL else torch.zeros((1,), dtype=torch.float64, device=dev)
    if d_word.numel() == 0:
        d_word = torch.zeros((1,), dtype=torch.int32, device=dev)
    sizes = dict(theta_out=NL, credit=NL, site_idx=S * top_m, site_val=S * top_m, tok=n_docs, bad=n_docs)
    bufs = {n: torch.full((sizes[n] + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    _native.attribute_sparse(d_off, d_word, d_freq, d_loff, d_lab, d_th, d_phi, n_docs, V, K, NL, max_labels, iters=iters, alpha=alpha,
                             top_m=top_m, ld_phi=phi_t.shape[1], **{n: b[GUARD:GUARD + sizes[n]] for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def body(got, name, shape=None):
    b = got[name][GUARD:got[name].shape[0] - GUARD]
    return b if shape is None else b.reshape(shape)


def check(got, want, top_m, skip=(), what=""):
    for name, dt in OUTPUTS:
        g, pat = got[name], PATTERN[dt]
        n = g.shape[0] - 2 * GUARD
        assert (g[:GUARD] == pat).all() and (g[GUARD + n:] == pat).all(), "%s: guard words around %s overwritten" % (what, name)
        b = g[GUARD:GUARD + n]
        if name in skip or (name.startswith("site_") and top_m == 0):
            assert (b == pat).all(), "%s: %s was written" % (what, name)
            continue
        w = want[name]
        b = b.reshape(w.shape)
        diff = np.argwhere(bits(b) != bits(w))
        assert diff.shape[0] == 0, "%s: %s differs at %s: got %s want %s" % (what, name, diff[:5].tolist(), b[tuple(diff[0])], w[tuple(diff[0])])


def dense_compacted(theta_s, phi_t, doc_off, word, freq, lab_off, lab, docs, iters, alpha, top_m):
    """the dense llda_attribute on the device on the compacted problems of ``docs`` (fit, L >= 1): the documents of one label count
    share a launch, each with a vocabulary block of its own that holds its columns of phi_t -> {d: dict of its outputs}"""
    out = {}
    counts = np.diff(lab_off)
    for L in sorted(set(int(counts[d]) for d in docs)):
        ids = [d for d in docs if counts[d] == L]
        theta = np.stack([theta_s[lab_off[d]:lab_off[d + 1]] for d in ids])
        phi = np.concatenate([phi_t[:, lab[lab_off[d]:lab_off[d + 1]].astype(np.int64)] for d in ids])      # (n V, L)
        n = np.asarray([doc_off[d + 1] - doc_off[d] for d in ids])
        off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        sites = np.concatenate([np.arange(doc_off[d], doc_off[d + 1]) for d in ids] + [np.zeros(0)]).astype(np.int64)
        w = word[sites].astype(np.int64)
        w = np.where((w >= 0) & (w < V), np.repeat(np.arange(len(ids)), n) * V + w, -1).astype(np.int32)
        r = run_dense(theta, phi, off, w, None if freq is None else freq[sites], L, iters, alpha, top_m, n_vocab=len(ids) * V, pad_out=0)
        m = len(ids)
        th, cr = body(r, "theta_out", (m, L)), body(r, "credit", (m, L))
        idx, val = body(r, "site_idx", (int(off[-1]), top_m)), body(r, "site_val", (int(off[-1]), top_m))
        for i, d in enumerate(ids):
            out[d] = dict(theta_out=th[i], credit=cr[i], tok=body(r, "tok")[i], bad=body(r, "bad")[i], site_idx=idx[off[i]:off[i + 1]],
                          site_val=val[off[i]:off[i + 1]])
    return out


@pytest.mark.parametrize("max_labels", MAX_LABELS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_sparseref_and_the_dense_kernel(K, max_labels):
    case = KS.index(K) * len(MAX_LABELS) + MAX_LABELS.index(max_labels)
    rng = np.random.default_rng(41000 + 100 * K + max_labels)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, max_labels)
    counts = np.diff(lab_off)
    assert set(counts[4:]) == set(c for c in COUNTS if c <= max_labels) and counts[UNFIT_LONG] == max_labels + 1
    fit = np.asarray([sparseref.doc_fit(lab_off, lab, d, K, max_labels)[0] for d in range(D)])
    assert not fit[:4].any() and fit[4:].all()
    for j in range(3):
        iters, alpha, top_m, freq_mode = SETTINGS[(case + 2 * j) % len(SETTINGS)]
        what = "K %d max_labels %d iters %d alpha %g top_m %d freq %s" % (K, max_labels, iters, alpha, top_m, freq_mode)
        doc_off, word, freq = corpus(rng, D, freq_mode)
        lens = np.diff(doc_off)
        assert set(lens) == set(LENS) and all(set(lens[counts == c]) >= {0, 1, 65} for c in set(counts[4:])), what
        want = sparseref.attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=K, V=V, max_labels=max_labels,
                                              iters=iters, alpha=alpha, top_m=top_m)
        # what the case is there for was met: both sides of the bound against the final loads, good and bad sites, a tie by label id
        full = np.flatnonzero(fit & (counts > 0))
        for d in full[:40]:
            th = want["theta_out"][lab_off[d]:lab_off[d + 1]]
            cols = lab[lab_off[d]:lab_off[d + 1]].astype(np.int64)
            assert attrref.sum64((th * phi_t[W_ABOVE, cols])[None, :])[0] >= attrref.MIN_P, what
            assert attrref.sum64((th * phi_t[W_BELOW, cols])[None, :])[0] < attrref.MIN_P, what
        assert all((word == w).any() for w in (W_ZERO, W_NAN, W_INF, W_ABOVE, W_BELOW, V, -1)), what
        assert want["tok"][full].sum() > 0 and want["bad"][full].sum() > 0 and want["tok"][~fit].sum() == 0 and want["bad"][~fit].sum() > 0
        if top_m > 1 and max_labels > 1:
            idx, val = want["site_idx"], want["site_val"]
            assert ((idx[:, 0] == 0) & (idx[:, 1] == K - 1) & (val[:, 0] == val[:, 1]) & (val[:, 0] > 0.0)).any(), what
            assert ((idx[:, 0] >= 0) & (idx[:, -1] < 0)).any(), what       # a good site with a padded list
        got = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, iters, alpha, top_m)
        check(got, want, top_m, what=what)
        if j:
            continue
        # ... and the dense kernel on the device, on every fit document's compacted problem
        dense = dense_compacted(theta_s, phi_t[:, :K], doc_off, word, freq, lab_off, lab, [int(d) for d in full], iters, alpha, top_m)
        th, cr, tok, bad = body(got, "theta_out"), body(got, "credit"), body(got, "tok"), body(got, "bad")
        S = int(doc_off[-1])
        idx, val = (body(got, "site_idx", (S, top_m)), body(got, "site_val", (S, top_m))) if top_m else (None, None)
        for d in full:
            r, lb, le, b, e = dense[int(d)], lab_off[d], lab_off[d + 1], doc_off[d], doc_off[d + 1]
            assert np.array_equal(bits(th[lb:le]), bits(r["theta_out"])) and np.array_equal(bits(cr[lb:le]), bits(r["credit"])), (what, d)
            assert tok[d] == r["tok"] and bad[d] == r["bad"], (what, d)
            if top_m:
                cols = lab[lb:le].astype(np.int64)
                assert np.array_equal(bits(val[b:e]), bits(r["site_val"])), (what, d)
                assert np.array_equal(idx[b:e], np.where(r["site_idx"] >= 0, cols[np.maximum(r["site_idx"], 0)], -1)), (what, d)


@pytest.mark.parametrize("K,max_labels", ((33, 8), (33, 32), (512, 16), (2048, 32), (2048, 8)))
def test_prefix_label_sets_give_the_bits_of_the_dense_kernel_at_full_k(K, max_labels):
    """labels 0 .. L_d - 1, the dense row 0 elsewhere: llda_attribute at full K (wave and LDS forms) gives the same bits"""
    rng = np.random.default_rng(42000 + K + max_labels)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, max_labels, prefix=True, unfit=False)
    iters, alpha, top_m, freq_mode = SETTINGS[3] if K != 512 else SETTINGS[1]
    doc_off, word, freq = corpus(rng, D, freq_mode)
    theta = sparseref.scatter(theta_s, lab_off, lab, K)
    dense = run_dense(theta, phi_t, doc_off, word, freq, K, iters, alpha, top_m, n_vocab=V, pad_out=0)
    got = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, iters, alpha, top_m)
    S = int(doc_off[-1])
    for name in ("theta_out", "credit"):
        full = body(dense, name, (D, K))
        assert np.array_equal(bits(sparseref.gather(full, lab_off, lab)), bits(body(got, name))), name
        assert np.array_equal(bits(sparseref.scatter(body(got, name), lab_off, lab, K)), bits(full)), name      # (+0.0 outside the sets)
    for name in ("site_idx", "site_val", "tok", "bad"):
        assert np.array_equal(bits(body(dense, name)), bits(body(got, name))), name
    assert body(got, "tok").sum() > 0 and body(got, "bad").sum() > 0 and (body(got, "site_idx", (S, top_m))[:, 1] > 0).any()


@pytest.mark.parametrize("K,max_labels", ((33, 8), (512, 16), (2048, 32)))
def test_batch_independence(K, max_labels):
    """a subset of the documents, in another order, alone and with max_labels of the next group: the same bits per document"""
    rng = np.random.default_rng(43000 + K)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, max_labels)
    doc_off, word, freq = corpus(rng, D, "mixed")
    iters, alpha, top_m = 2, 0.1, 4
    S = int(doc_off[-1])
    whole = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, iters, alpha, top_m)
    th, cr, tok, bad = (body(whole, n) for n in ("theta_out", "credit", "tok", "bad"))
    idx, val = body(whole, "site_idx", (S, top_m)), body(whole, "site_val", (S, top_m))
    plans = [("a subset, reversed", list(range(D))[::-3], max_labels), ("alone", [57], max_labels), ("alone, unfit", [UNFIT_TWICE], max_labels)]
    if max_labels < 32:
        plans.append(("a wider group", list(range(4, D, 2)), 2 * max_labels))
    for what, ids, ml in plans:
        sites = np.concatenate([np.arange(doc_off[d], doc_off[d + 1]) for d in ids] + [np.zeros(0)]).astype(np.int64)
        slots = np.concatenate([np.arange(lab_off[d], lab_off[d + 1]) for d in ids] + [np.zeros(0)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(np.diff(doc_off)[ids])]).astype(np.int64)
        loff = np.concatenate([[0], np.cumsum(np.diff(lab_off)[ids])]).astype(np.int64)
        r = run(theta_s[slots], phi_t, off, word[sites], freq[sites], loff, lab[slots], K, ml, iters, alpha, top_m)
        want = dict(theta_out=th[slots], credit=cr[slots], tok=tok[ids], bad=bad[ids], site_idx=idx[sites], site_val=val[sites])
        check(r, want, top_m, what="K %d %s" % (K, what))


@pytest.mark.parametrize("K,max_labels", ((33, 16), (2048, 8)))
def test_every_output_may_be_null_and_no_document(K, max_labels):
    rng = np.random.default_rng(44000 + K)
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, max_labels, n_docs=40)
    doc_off, word, freq = corpus(rng, 40, "mixed")
    want = sparseref.attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=K, V=V, max_labels=max_labels, iters=2,
                                          alpha=0.1, top_m=2)
    for skip in (("theta_out",), ("credit",), ("site_idx", "site_val"), ("tok",), ("bad",), tuple(n for n, _ in OUTPUTS)):
        got = run(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K, max_labels, 2, 0.1, 2, skip=skip)
        check(got, want, 2, skip=skip, what="K %d without %s" % (K, skip))
    import torch
    from lda_thesis_amd import _native
    t = torch.zeros((1, K), dtype=torch.float64, device="cuda:0")
    _native.attribute_sparse(None, None, None, None, None, None, t, 0, 1, K, 0, max_labels)      # D = 0: a no-op, nothing is dereferenced
    with pytest.raises(_native.NativeError):                             # one of the pair alone: refused
        _native.attribute_sparse(t, t, None, t, t, t, t, 1, 1, K, 1, max_labels, top_m=1, site_val=t)
    # documents and no label at all: NL = 0, every site is bad, no slot is written
    none = np.zeros(41, dtype=np.int64)
    got = run(np.zeros(0), phi_t, doc_off, word, freq, none, np.zeros(0, dtype=np.int32), K, max_labels, 1, 0.1, 1)
    fsum = np.add.reduceat(np.append(freq, 0).astype(np.int64), doc_off[:-1]) * (np.diff(doc_off) > 0)
    S = int(doc_off[-1])
    check(got, dict(theta_out=np.zeros(0), credit=np.zeros(0), site_idx=np.full((S, 1), -1, dtype=np.int32), site_val=np.zeros((S, 1)),
                    tok=np.zeros(40, dtype=np.int64), bad=fsum), 1, what="no label")


def test_python_surface():
    """attribution.attribute_sparse and docmodel.label_csr: numpy CSRs in, device tensors out, and the refusals on the host"""
    import torch
    from lda_thesis_amd import attribution, docmodel
    rng = np.random.default_rng(45)
    K, n_docs = 40, 30
    phi_t = phi_model(rng, K)
    lab_off, lab, theta_s = label_sets(rng, K, 8, n_docs=n_docs, unfit=False)
    doc_off, word, freq = corpus(rng, n_docs, "mixed")
    word[(word < 5) | (word >= V)] = 9
    dev = torch.device("cuda", 0)
    d_phi, d_th = torch.from_numpy(phi_t).to(dev)[:, :K], torch.from_numpy(theta_s).to(dev)          # row stride K + 5
    lists = [lab[lab_off[d]:lab_off[d + 1]].tolist()[::-1] for d in range(n_docs)]
    off2, lab2 = docmodel.label_csr(lists, K=K)
    assert np.array_equal(off2, lab_off) and np.array_equal(lab2, lab)
    want = sparseref.attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=K, iters=4, alpha=0.05, top_m=3)
    got = attribution.attribute_sparse(d_th, d_phi, doc_off, word, freq, off2, lab2, iters=4, alpha=0.05, top_m=3)
    assert sorted(got) == ["bad", "credit", "site_idx", "site_val", "theta", "tok"]
    for name, ref in (("theta", "theta_out"), ("credit", "credit"), ("site_idx", "site_idx"), ("site_val", "site_val"), ("tok", "tok"),
                      ("bad", "bad")):
        g = got[name].cpu().numpy()
        assert g.dtype == want[ref].dtype and np.array_equal(bits(g), bits(want[ref])), name
    dense = attribution.scatter_slots(got["theta"], lab_off, lab, K)
    assert np.array_equal(bits(dense.cpu().numpy()), bits(sparseref.scatter(want["theta_out"], lab_off, lab, K)))
    assert np.array_equal(bits(attribution.gather_slots(dense, lab_off, lab).cpu().numpy()), bits(want["theta_out"]))
    only = attribution.attribute_sparse(d_th, d_phi, doc_off, word, None, lab_off, lab, top_m=0, want=("credit", "sites"))
    assert sorted(only) == ["credit"]
    twice, down, far = lab.copy(), lab.copy(), lab.copy()
    d = int(np.flatnonzero(np.diff(lab_off) >= 2)[0])
    twice[lab_off[d] + 1] = twice[lab_off[d]]
    down[lab_off[d]:lab_off[d] + 2] = down[lab_off[d]:lab_off[d] + 2][::-1]
    far[lab_off[d + 1] - 1] = K
    for bad in (dict(lab=twice), dict(lab=down), dict(lab=far), dict(lab_off=lab_off[:-1]), dict(lab=lab[:-1]), dict(theta=d_th[:-1]),
                dict(theta=theta_s), dict(word=np.where(word == 9, V, word)), dict(iters=-1), dict(alpha=-0.5), dict(top_m=5),
                dict(want=("theta", "everything")), dict(lab_off=np.array([0, 33] + [33] * (n_docs - 1)), lab=np.arange(33), theta=d_th[:33])):
        args = dict(theta=d_th, phi=d_phi, doc_off=doc_off, word=word, freq=freq, lab_off=lab_off, lab=lab, iters=1, alpha=0.1, top_m=1,
                    want=("theta",))
        args.update(bad)
        with pytest.raises(ValueError):
            attribution.attribute_sparse(args["theta"], args["phi"], args["doc_off"], args["word"], args["freq"], args["lab_off"], args["lab"],
                                         iters=args["iters"], alpha=args["alpha"], top_m=args["top_m"], want=args["want"])
