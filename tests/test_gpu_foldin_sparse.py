"""llda_foldin_sparse on the device: z / n_dk_s / th_s / status bit for bit against its CPU restatement (tests/sparsefoldinref.py) for
every slot count of a lane and on both sides of every seam, for K up to LLDA_MAX_K, with label lists of every summation schedule
mixed inside one wavefront, unfit documents of every kind between fit ones, words outside the vocabulary, rows of loadings scaled to
the ends of the double range and a word that loads on nothing planted in two designated documents.  For documents that share one
label list also against the unchanged dense llda_foldin on the compacted loadings."""
import functools

import numpy as np
import pytest

import sparsefoldinref as sfr
import sparseref

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567
STREAM = 0x7E57
KS = (9, 64, 392, 2048, 7688)
MAX_LABELS = (1, 8, 9, 16, 17, 32)
V = 50
W_ZERO = 0                                                              # a word that loads on nothing
LS = (1, 7, 8, 9, 15, 16, 17, 24, 31, 32)                               # sequential, tail only, rows only, rows and tail; T_d = 1, 2, 4
SITES = (1, 17, 2, 33, 0)
N_DOCS = 40                                                             # two workgroups of 32 documents
UNFIT_AT = {0: "front", 6: "long", 11: "twice", 17: "down", 22: "high", 27: "neg", N_DOCS - 1: "beyond"}
NO_LIST_AT = 20                                                         # L_d = 0 and no site: fit, nothing to draw
ALPHA = 0.3


def loadings(rng, K):
    """positive loadings across eight orders of magnitude, three in ten exactly zero; label 0 loads on every word but word 0, which
    loads on nothing; the rows 1 .. 4 are scaled by 2^200, 2^-200, 2^500, 2^-500"""
    phi_t = rng.gamma(0.5, size=(V, K)) * 10.0 ** rng.uniform(-8, 0, size=(V, K)) + 1e-300
    phi_t[rng.random((V, K)) < 0.3] = 0.0
    phi_t[:, 0] = rng.uniform(0.01, 1.0, size=V)
    phi_t[W_ZERO] = 0.0
    for row, e in ((1, 200), (2, -200), (3, 500), (4, -500)):
        phi_t[row] *= 2.0 ** e
    return phi_t


def batch(rng, K, max_labels, plain=False):
    """(doc_off, word, freq, lab_off, lab, NL, planted, ids): N_DOCS documents; plain: fit lists and good words only"""
    top = min(max_labels, K)
    ls = sorted(set([L for L in LS if L <= top] + [top]))
    docs, sets = [], []
    for d in range(N_DOCS):
        kind = None if plain else UNFIT_AT.get(d)
        n = SITES[(3 * d + d // 10) % len(SITES)]
        L = ls[d % len(ls)] if kind is None else 1
        if d == NO_LIST_AT:
            n, L = 0, 0
        t = rng.integers(1, V, size=n)
        if n >= 17:
            t[:4] = (1, 2, 3, 4)                                        # the scaled rows
            if not plain:
                t[6], t[n - 1] = V, -1
        docs.append(t)
        ids = np.sort(np.concatenate([[0], 1 + rng.choice(K - 1, size=L - 1, replace=False)])) if L else np.zeros(0, dtype=np.int64)
        if L > 1:
            ids[-1] = K - 1
        if kind == "long":
            ids = np.sort(rng.choice(K, size=max_labels + 1, replace=False)) if max_labels + 1 <= K else np.arange(max_labels + 1)
        ids = {"twice": np.array([0, 0]), "down": np.array([2, 0]), "high": np.array([K]), "neg": np.array([-1])}.get(kind, ids)
        sets.append(ids.astype(np.int64))
    planted = ()
    if not plain:
        fit = [d for d in range(N_DOCS) if d not in UNFIT_AT]
        planted = ([d for d in fit if len(docs[d]) == 33][0], [d for d in fit if len(docs[d]) == 17][-1])
        for d in planted:
            docs[d][4] = W_ZERO
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    NL = int(lab_off[-1])
    if not plain:
        lab_off[0] = -1                                                 # "front": the first document starts before the array
        NL -= 1                                                         # "beyond": the last one ends behind what the caller states
    word = np.concatenate(docs).astype(np.int32)
    freq = rng.integers(1, 6, size=word.shape[0]).astype(np.int32)
    ids = rng.integers(0, 2 ** 20, size=N_DOCS) + np.where(np.arange(N_DOCS) % 3 == 1, 2 ** 32 * (1 + np.arange(N_DOCS)), 0)
    return doc_off, word, freq, lab_off, np.concatenate(sets).astype(np.int32), NL, planted, ids.astype(np.int64)


def run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, iters, thinning, doc_ids=None, doc_base=0, pad=3):
    """llda_foldin_sparse through the binding with ld_phi = K + pad, NaN beyond K, poison behind the NL label ids the caller states and
    outputs that start from the restatement's fill values.  Returns (z, n_dk_s, th_s, status) as numpy values."""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda")
    D, S = len(doc_off) - 1, int(doc_off[-1])
    wide = np.full((phi_t.shape[0], K + pad), np.nan)
    wide[:, :K] = phi_t[:, :K]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    d_word, d_freq = up(np.concatenate([word, np.zeros(1)]), np.int32), up(np.concatenate([freq, np.zeros(1)]), np.int32)
    d_lab = up(np.concatenate([lab[:NL], np.full(40, 2 ** 30)]), np.int32)
    d_ids = None if doc_ids is None else up(doc_ids, np.int64)
    z = torch.full((S + 1,), -9, dtype=torch.int32, device=dev)
    n_dk_s = torch.full((NL + 1,), sfr.ND_FILL, dtype=torch.int32, device=dev)
    th_s = torch.full((NL + 1,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _native.foldin_sparse(up(doc_off, np.int64), d_word, d_freq, up(wide, np.float64), up(lab_off, np.int64), d_lab, D, phi_t.shape[0], K, NL,
                          max_labels, iters=iters, thinning=thinning, alpha=ALPHA, c_init=sfr.C_INIT, c_loop=sfr.C_LOOP, seed=SEED,
                          stream_id=STREAM, z=z, n_dk_s=n_dk_s, th_s=th_s, ld_phi=K + pad, doc_ids=d_ids, doc_base=doc_base, status=status)
    torch.cuda.synchronize()
    out = z.cpu().numpy(), n_dk_s.cpu().numpy(), th_s.cpu().numpy(), int(status.item())
    assert out[0][S] == -9 and out[1][NL] == sfr.ND_FILL and np.isnan(out[2][NL])          # nothing behind the arrays was written
    return out[0][:S].astype(np.int64), out[1][:NL].astype(np.int64), out[2][:NL], out[3]


def check(got, want, doc_off, lab_off, NL, skip=(), what=""):
    """z, n_dk_s, th_s of every document but ``skip``, slot by slot (a slot nobody writes keeps its fill value), and the status"""
    z, n_dk_s, th_s, status = got
    for d in range(len(doc_off) - 1):
        if d in skip:
            continue
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        assert np.array_equal(z[b:e], want["z"][b:e]), "%s: z of document %d: %s != %s" % (what, d, z[b:e], want["z"][b:e])
        lb, le = max(int(lab_off[d]), 0), min(int(lab_off[d + 1]), NL)
        assert np.array_equal(n_dk_s[lb:le], want["n_dk_s"][lb:le]), "%s: n_dk_s of document %d: %s != %s" % (what, d, n_dk_s[lb:le], want["n_dk_s"][lb:le])
        g, w = th_s[lb:le], want["th_s"][lb:le]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)].view(np.uint64), w[~np.isnan(w)].view(np.uint64)), \
            "%s: th_s of document %d: %s != %s" % (what, d, g, w)
    assert status == want["status"], what


@functools.lru_cache(maxsize=None)
def case(K, max_labels, iters=7, thinning=3, plain=False):
    rng = np.random.default_rng(73000 + 100 * K + max_labels)
    phi_t = loadings(rng, K)
    doc_off, word, freq, lab_off, lab, NL, planted, ids = batch(rng, K, max_labels, plain)
    want = sfr.fold_in_sparse_ref(phi_t, doc_off, word, freq, lab_off, lab, ALPHA, iters, thinning, SEED, STREAM, K=K, V=V,
                                  max_labels=max_labels, doc_ids=ids, NL=NL)
    return phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want


def test_the_plan_covers_the_geometries():
    """every schedule of the sum inside one call, the unfit kinds between fit documents, every site count"""
    rng = np.random.default_rng(1)
    doc_off, word, freq, lab_off, lab, NL, planted, ids = batch(rng, 64, 32)
    fit = [d for d in range(N_DOCS) if sparseref.doc_fit(lab_off, lab, d, 64, 32, NL)[0]]
    assert sorted(set(range(N_DOCS)) - set(fit)) == sorted(UNFIT_AT)
    assert set(int(lab_off[d + 1] - lab_off[d]) for d in fit) == set(LS) | {0}
    assert set(np.diff(doc_off)[fit]) == set(SITES) and len(planted) == 2 and planted[0] // 32 != planted[1] // 32 or planted[0] != planted[1]
    first = [int(lab_off[d + 1] - lab_off[d]) for d in fit if d < 8]      # the first wavefront mixes the schedules
    assert len(set(L >> 3 for L in first)) >= 2 and len(set(L & 7 for L in first)) >= 3
    assert (ids > 2 ** 32).any() and (word == V).any() and (word == -1).any()


@pytest.mark.parametrize("max_labels", MAX_LABELS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_the_restatement(K, max_labels):
    phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want = case(K, max_labels)
    what = "K %d max_labels %d" % (K, max_labels)
    # before anything is compared: the restatement raises in exactly the two documents that hold the word without a loading
    assert sorted(np.flatnonzero(want["raises"])) == sorted(planted) and len(set(planted)) == 2, what
    assert want["status"] == 1 | 2 | 4, what
    got = run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, 7, 3, doc_ids=ids)
    check(got, want, doc_off, lab_off, NL, skip=planted, what=what)


def test_start_state_and_the_uniform_start():
    """iters = 0: the start state; the two planted documents start every site from 1 / L_d and nothing raises"""
    K, max_labels = 392, 17
    phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want = case(K, max_labels, 0, 1)
    assert not want["raises"].any() and want["status"] == 2 | 4
    other = sfr.fold_in_sparse_ref(np.where(np.arange(V)[:, None] == W_ZERO, 1.0, phi_t), doc_off, word, freq, lab_off, lab, ALPHA, 0, 1, SEED,
                                   STREAM, K=K, V=V, max_labels=max_labels, doc_ids=ids, NL=NL)
    for d in planted:                                                   # (the uniform start shows: other loadings of that word, other z)
        assert not np.array_equal(other["z"][doc_off[d]:doc_off[d + 1]], want["z"][doc_off[d]:doc_off[d + 1]])
    got = run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, 0, 1, doc_ids=ids)
    check(got, want, doc_off, lab_off, NL, what="start state")
    fit = ~np.isnan(want["th_s"])
    assert not got[2][fit].any()                                        # th_s = 0: no sweep


def test_thinning_beyond_the_sweeps():
    K, max_labels = 64, 9
    phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want = case(K, max_labels, 2, 5)
    assert sorted(np.flatnonzero(want["raises"])) == sorted(planted)
    got = run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, 2, 5, doc_ids=ids)
    check(got, want, doc_off, lab_off, NL, skip=planted, what="thinning 5 > iters 2")
    keep = np.ones(NL, dtype=bool)
    for d in planted:
        keep[lab_off[d]:lab_off[d + 1]] = False
    assert not got[2][keep & ~np.isnan(want["th_s"])].any()


def test_plain_batch_has_status_zero():
    K, max_labels = 2048, 32
    phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want = case(K, max_labels, 7, 3, True)
    assert planted == () and not want["raises"].any() and want["status"] == 0
    got = run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, 7, 3, doc_ids=ids)
    check(got, want, doc_off, lab_off, NL, what="plain")
    assert got[3] == 0
    # doc_base + d in place of doc_ids
    base = 2 ** 32 - 7
    want = sfr.fold_in_sparse_ref(phi_t, doc_off, word, freq, lab_off, lab, ALPHA, 3, 1, SEED, STREAM, K=K, V=V, max_labels=max_labels, doc_base=base)
    check(run(phi_t, K, doc_off, word, freq, lab_off, lab, NL, max_labels, 3, 1, doc_base=base), want, doc_off, lab_off, NL, what="doc_base")


def test_a_document_does_not_depend_on_its_batch():
    """the documents of a batch in reverse order, and one of them alone, with their own ids: the same outputs"""
    K, max_labels = 392, 32
    phi_t, doc_off, word, freq, lab_off, lab, NL, planted, ids, want = case(K, max_labels, 7, 3, True)
    order = np.arange(N_DOCS)[::-1]
    for sub in (order, np.array([13])):
        w = np.concatenate([word[doc_off[d]:doc_off[d + 1]] for d in sub] + [np.zeros(0, dtype=np.int32)])
        f = np.concatenate([freq[doc_off[d]:doc_off[d + 1]] for d in sub] + [np.zeros(0, dtype=np.int32)])
        la = np.concatenate([lab[lab_off[d]:lab_off[d + 1]] for d in sub] + [np.zeros(0, dtype=np.int32)])
        off = np.concatenate([[0], np.cumsum([doc_off[d + 1] - doc_off[d] for d in sub])]).astype(np.int64)
        loff = np.concatenate([[0], np.cumsum([lab_off[d + 1] - lab_off[d] for d in sub])]).astype(np.int64)
        z, n_dk_s, th_s, status = run(phi_t, K, off, w, f, loff, la, int(loff[-1]), max_labels, 7, 3, doc_ids=ids[sub])
        assert status == 0
        for i, d in enumerate(sub):
            assert np.array_equal(z[off[i]:off[i + 1]], want["z"][doc_off[d]:doc_off[d + 1]]), d
            assert np.array_equal(n_dk_s[loff[i]:loff[i + 1]], want["n_dk_s"][lab_off[d]:lab_off[d + 1]]), d
            assert np.array_equal(th_s[loff[i]:loff[i + 1]].view(np.uint64), want["th_s"][lab_off[d]:lab_off[d + 1]].view(np.uint64)), d


@pytest.mark.parametrize("L", (1, 7, 8, 9, 20, 32))
def test_the_compacted_problem_through_the_dense_kernel(L):
    """documents that share one label list of length L: llda_foldin at K = L on the compacted loadings gives the same z, n_dk, th"""
    import torch
    from lda_thesis_amd import foldin
    K = 64
    rng = np.random.default_rng(500 + L)
    phi_t = loadings(rng, K)
    ids = np.sort(np.concatenate([[0], 1 + rng.choice(K - 1, size=L - 1, replace=False)]))
    tups = []
    for n in (1, 2, 17, 33, 5, 9, 17, 3, 33, 1):
        words = rng.choice(np.arange(1, V), size=n, replace=False)
        tups.append([(int(w), int(f)) for w, f in zip(words, rng.integers(1, 6, size=n))])
    D = len(tups)
    lab_off, lab = np.arange(D + 1, dtype=np.int64) * L, np.tile(ids, D).astype(np.int32)
    sparse = foldin.fold_in_sparse(torch.from_numpy(phi_t).cuda(), ALPHA, tups, lab_off, lab, 7, 3, SEED, STREAM, doc_base=2 ** 32 - 3)
    dense = foldin.fold_in(np.ascontiguousarray(phi_t[:, ids].T), ALPHA, tups, 7, 3, SEED, STREAM, doc_base=2 ** 32 - 3)
    for d in range(D):
        assert np.array_equal(sparse["z"][d], dense["z"][d]), d
    assert np.array_equal(sparse["n_dk_s"].reshape(D, L), dense["n_dk"])
    assert np.array_equal(sparse["th_s"].reshape(D, L).view(np.uint64), np.ascontiguousarray(dense["th_hat"]).view(np.uint64))
    assert sparse["n_dk_s"].sum() == sum(f for t in tups for _, f in t)


def test_the_python_entry_raises_where_the_reference_does():
    """foldin.fold_in_sparse: a site without a positive probability is numpy.random.multinomial's ValueError, as in fold_in"""
    import torch
    from lda_thesis_amd import foldin
    phi_t = loadings(np.random.default_rng(9), 16)
    with pytest.raises(ValueError, match="pvals"):
        foldin.fold_in_sparse(torch.from_numpy(phi_t).cuda(), ALPHA, [[(3, 1), (W_ZERO, 2)]], [0, 3], [0, 5, 9], 2, 1, SEED)
    r = foldin.fold_in_sparse(torch.from_numpy(phi_t).cuda(), ALPHA, [[(3, 1), (7, 2)], [(5, 4)]], [0, 3, 4], [0, 5, 9, 0], 2, 1, SEED)
    want = sfr.fold_in_sparse_ref(phi_t, [0, 2, 3], [3, 7, 5], [1, 2, 4], [0, 3, 4], [0, 5, 9, 0], ALPHA, 2, 1, SEED, foldin.TEST_STREAM)
    assert np.array_equal(np.concatenate(r["z"]), want["z"]) and np.array_equal(r["n_dk_s"], want["n_dk_s"])
    assert np.array_equal(r["th_s"].view(np.uint64), want["th_s"].view(np.uint64))
