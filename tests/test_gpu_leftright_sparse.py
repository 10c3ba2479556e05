"""llda_left_to_right_sparse on the device: mant / expo / tok / bad / status bit for bit against its CPU restatement
(tests/sparseheldref.py) at every lane group and on both sides of every group seam, for K up to LLDA_MAX_K, with particles that
fill a wavefront, half a wavefront and eight wavefronts, unfit documents of every kind between fit ones, words outside the
vocabulary, words without a loading -- and one planted divergence between the particles of one wavefront.  For prefix label sets
also against the dense llda_left_to_right with the prefix as the allowed row."""
import functools

import numpy as np
import pytest

import sparseheldref
import sparseref
from test_gpu_leftright import device_run as dense_run

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567
STREAM = 0xFFFFFFF8                                                     # stream_id + r wraps around 2^32 for the later particles
KS = (9, 64, 392, 1024, 2048, 7688)
MAX_LABELS = (1, 8, 9, 16, 17, 32)
RS = (1, 3, 8, 9, 16)
V = 50
W_ZERO = 0                                                              # a word that loads on nothing
# the documents of a batch: (tokens, kind of label list)
PLAN = ((1, "front"), (17, "full"), (5, "long"), (33, "half"), (2, "twice"), (0, "full"), (3, "down"), (1, "one"), (2, "high"), (2, "full"),
        (1, "neg"), (4, "empty"), (9, "full"), (3, "beyond"))
UNFIT_KINDS = ("front", "long", "twice", "down", "high", "neg", "beyond")
IDS = (3, 2 ** 32 + 5, 0, 2 ** 40 + 1, 7, 2 ** 32 + 5, 1, 9, 2 ** 33, 4, 6, 8, 2 ** 32, 11)


def particles(K, max_labels):
    return RS[(KS.index(K) + MAX_LABELS.index(max_labels)) % len(RS)]


def group(max_labels):
    return 8 if max_labels <= 8 else 16 if max_labels <= 16 else 32


def loadings(rng, K):
    """positive loadings across eight orders of magnitude, three in ten exactly zero; word 0 loads on nothing, the rows 1 and 2 are
    scaled by 2^200 and 2^-200"""
    phi_t = rng.gamma(0.5, size=(V, K)) * 10.0 ** rng.uniform(-8, 0, size=(V, K)) + 1e-300
    phi_t[rng.random((V, K)) < 0.3] = 0.0
    phi_t[W_ZERO] = 0.0
    phi_t[1] *= 2.0 ** 200
    phi_t[2] *= 2.0 ** -200
    return phi_t


def batch(rng, K, max_labels, plan=PLAN):
    """(doc_off, word, lab_off, lab, NL): scattered lists that reach K - 1; tokens outside [0, V) and the word without a loading in the
    longer documents"""
    top = min(max_labels, K)
    docs, sets = [], []
    for n, kind in plan:
        t = rng.integers(1, V, size=n)
        if n >= 9:
            t[4], t[6], t[n - 1] = W_ZERO, V, -1
        docs.append(t)
        L = {"full": top, "half": max(1, top // 2), "one": 1, "empty": 0}.get(kind, 1)
        ids = np.sort(np.concatenate([[0], 1 + rng.choice(K - 1, size=L - 1, replace=False)])) if L else np.zeros(0, dtype=np.int64)
        if L > 1:
            ids[-1] = K - 1
        if kind == "long":
            ids = np.sort(rng.choice(K, size=max_labels + 1, replace=False)) if max_labels + 1 <= K else np.arange(max_labels + 1)
        ids = {"twice": np.array([0, 0]), "down": np.array([2, 0]), "high": np.array([K]), "neg": np.array([-1])}.get(kind, ids)
        sets.append(ids.astype(np.int64))
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    NL = int(lab_off[-1])
    if plan[0][1] == "front":
        lab_off[0] = -1                                                 # the first document starts before the array
    if plan[-1][1] == "beyond":
        NL -= 1                                                         # the last one ends behind what the caller states
    return doc_off, np.concatenate(docs).astype(np.int32), lab_off, np.concatenate(sets).astype(np.int32), NL


def run(phi_t, K, doc_off, word, lab_off, lab, NL, max_labels, alpha, R, seed, stream, doc_ids=None, cap=None, pad=3):
    """llda_left_to_right_sparse through the binding with ld_phi = K + pad, NaN beyond K, and poison behind the NL label ids the
    caller states.  Returns (mant, expo, tok, bad, status) as numpy values."""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda")
    D = len(doc_off) - 1
    wide = np.full((phi_t.shape[0], K + pad), np.nan)
    wide[:, :K] = phi_t[:, :K]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)
    d_word = up(np.concatenate([word, np.zeros(1)]), np.int32)
    d_lab = up(np.concatenate([lab[:NL], np.full(40, 2 ** 30)]), np.int32)
    d_ids = None if doc_ids is None else up(doc_ids, np.int64)
    mant = torch.full((max(D, 1),), -7.0, dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.full((max(D, 1),), -7, dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    lens = np.diff(np.asarray(doc_off, dtype=np.int64))
    cap = max(1, int(lens.max()) if D else 1) if cap is None else cap
    _native.left_to_right_sparse(up(doc_off, np.int64), d_word, up(wide, np.float64), up(lab_off, np.int64), d_lab, D, phi_t.shape[0], K, NL,
                                 max_labels, particles=R, alpha=alpha, seed=seed, stream_id=stream, max_doc_tokens=cap, mant=mant, expo=expo,
                                 tok=tok, bad=bad, ld_phi=K + pad, doc_ids=d_ids, status=status)
    torch.cuda.synchronize()
    return mant.cpu().numpy()[:D], expo.cpu().numpy()[:D], tok.cpu().numpy()[:D], bad.cpu().numpy()[:D], int(status.item())


def check(got, want, what=""):
    for name, g, w in zip(("mant", "expo", "tok", "bad"), got[:4], want[:4]):
        g, w = np.asarray(g), np.asarray(w)
        diff = np.flatnonzero(g.view(np.uint64) != w.astype(g.dtype).view(np.uint64))
        assert diff.size == 0, "%s: %s differs at documents %s: %s != %s" % (what, name, diff[:5], g[diff[:5]], w[diff[:5]])
    assert got[4] == want[4], what


@functools.lru_cache(maxsize=None)
def case(K, max_labels):
    rng = np.random.default_rng(61000 + 100 * K + max_labels)
    phi_t = loadings(rng, K)
    doc_off, word, lab_off, lab, NL = batch(rng, K, max_labels)
    R, alpha = particles(K, max_labels), 0.3
    stats, trace = {}, {}
    want = sparseheldref.left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, alpha, R, SEED, STREAM, K=K, V=V, max_labels=max_labels,
                                                  doc_ids=IDS, NL=NL, stats=stats, trace=trace)
    return phi_t, doc_off, word, lab_off, lab, NL, R, alpha, want, stats, trace


def test_the_table_of_cases_covers_the_geometries():
    """R = 8 in one wavefront of 8-lane groups, a half-filled last wavefront, eight wavefronts of 32-lane groups, every R and group"""
    seen = set((group(ml), particles(K, ml)) for K in KS for ml in MAX_LABELS)
    assert {(8, 8), (8, 9), (32, 16), (32, 3), (16, 9)} <= seen and set(r for _, r in seen) == set(RS)


@pytest.mark.parametrize("max_labels", MAX_LABELS)
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_the_restatement(K, max_labels):
    phi_t, doc_off, word, lab_off, lab, NL, R, alpha, want, stats, trace = case(K, max_labels)
    what = "K %d max_labels %d R %d" % (K, max_labels, R)
    fit = np.asarray([sparseref.doc_fit(lab_off, lab, d, K, max_labels, NL)[0] for d in range(len(PLAN))])
    assert [k in UNFIT_KINDS for _, k in PLAN] == (~fit).tolist(), what
    mant, expo, tok, bad, status = want
    lens = np.diff(doc_off)
    gone = np.flatnonzero(~fit | (np.diff(lab_off) == 0))
    assert status == 0 and (tok[gone] == 0).all() and (bad[gone] == lens[gone]).all() and (mant[gone] == 0.5).all(), what
    assert tok[fit].sum() > 0 and bad[fit].sum() >= 3 * 3, what         # (the three planted tokens of the three longer documents)
    assert stats["draws"] > 0, what
    # the word without a loading stays unassigned in every particle, and the later positions skip it
    for d in (1, 3, 12):
        assert (trace["z"][d][:, 4] == -1).all() and (trace["z"][d][:, :4] >= 0).any(), (what, d)
    check(run(phi_t, K, doc_off, word, lab_off, lab, NL, max_labels, alpha, R, SEED, STREAM, doc_ids=IDS), want, what)


@pytest.mark.parametrize("K,max_labels", ((2048, 8), (7688, 16), (1024, 32)))
def test_a_document_of_130_tokens(K, max_labels):
    """130 tokens: more than one Philox batch of every group (16, 32, 64 positions) and more than the dense kernel's 128; R = 3"""
    rng = np.random.default_rng(62000 + K)
    phi_t = loadings(rng, K)
    doc_off, word, lab_off, lab, NL = batch(rng, K, max_labels, plan=((2, "full"), (130, "full"), (1, "one")))
    want = sparseheldref.left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, 0.3, 3, SEED, 5, K=K, V=V, max_labels=max_labels,
                                                  doc_ids=[2, 2 ** 32 + 1, 0])
    assert want[2][1] == 127 and want[3][1] == 3
    check(run(phi_t, K, doc_off, word, lab_off, lab, NL, max_labels, 0.3, 3, SEED, 5, doc_ids=[2, 2 ** 32 + 1, 0]), want, "K %d" % K)


DIVERGENCE_SEED = 0


def divergence_case(seed):
    """alpha = 2^-10; the labels {j, other}; word 1 loads on both, word 2 has 2^-1070 on j and nothing elsewhere: (0 + alpha) * 2^-1070
    is +0.0, (c + alpha) * 2^-1070 > 0 once c >= 1 -- S_r > 0 only in the particles that have assigned j before"""
    K, alpha, R = 40, 2.0 ** -10, 8
    phi_t = np.zeros((V, K))
    j, other = 17, 3
    phi_t[1, j], phi_t[1, other] = 0.4, 0.6
    phi_t[2, j] = 2.0 ** -1070
    docs = [[1, 1], [1, 1, 2, 1, 2, 1, 1], [1]]
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    word = np.concatenate(docs).astype(np.int32)
    lab_off, lab = np.array([0, 2, 4, 6], dtype=np.int64), np.array([other, j] * 3, dtype=np.int32)
    trace = {}
    want = sparseheldref.left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, alpha, R, seed, 0, K=K, V=V, max_labels=8, trace=trace)
    return phi_t, K, doc_off, word, lab_off, lab, alpha, R, want, trace


def test_particles_of_one_wavefront_diverge():
    """R = 8 at G = 8: the eight particles share a wavefront; at the planted position some hold an assignment and some do not, so
    what a wavefront-uniform branch decided in the dense kernel has to be decided per group"""
    assert 0.0 + (0.0 + 2.0 ** -10) * 2.0 ** -1070 == 0.0 and (1.0 + 2.0 ** -10) * 2.0 ** -1070 > 0.0
    phi_t, K, doc_off, word, lab_off, lab, alpha, R, want, trace = divergence_case(DIVERGENCE_SEED)
    z = trace["z"][1]
    assert (z[:, 2] >= 0).any() and (z[:, 2] < 0).any(), "pick another seed: %s" % z[:, 2]
    check(run(phi_t, K, doc_off, word, lab_off, lab, len(lab), 8, alpha, R, DIVERGENCE_SEED, 0), want, "divergence")


def test_a_document_longer_than_the_launch_allows():
    rng = np.random.default_rng(63)
    K, max_labels = 392, 9
    phi_t = loadings(rng, K)
    doc_off, word, lab_off, lab, NL = batch(rng, K, max_labels, plan=((5, "full"), (9, "full"), (4, "half"), (8, "full")))
    want = sparseheldref.left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, 0.3, 9, SEED, 1, K=K, V=V, max_labels=max_labels,
                                                  max_doc_tokens=8)
    assert want[4] == 1 and [x[1] for x in want[:4]] == [0.5, 1, 0, 0] and want[2][0] > 0 and want[2][3] > 0
    check(run(phi_t, K, doc_off, word, lab_off, lab, NL, max_labels, 0.3, 9, SEED, 1, cap=8), want, "too long")
    # ... and with room for it, nothing is flagged and its neighbours have the same bits
    roomy = run(phi_t, K, doc_off, word, lab_off, lab, NL, max_labels, 0.3, 9, SEED, 1)
    assert roomy[4] == 0 and roomy[2][1] > 0
    for i in (0, 2, 3):
        assert all(roomy[k][i] == want[k][i] for k in range(4))


@pytest.mark.parametrize("K,max_labels,R", ((9, 8, 8), (64, 16, 9), (392, 32, 16), (64, 1, 3)))
def test_prefix_label_sets_give_the_bits_of_the_dense_kernel(K, max_labels, R):
    """labels 0 .. L_d - 1: llda_left_to_right at full K with the prefix as the allowed row, same ids, seed and stream"""
    rng = np.random.default_rng(64000 + K)
    phi_t = loadings(rng, K)
    top = min(max_labels, K)
    counts = [top, 1, max(1, top // 2), top, max(1, top - 1), 0]
    lens = [17, 5, 33, 0, 9, 3]
    docs = [rng.integers(0, V, size=n) for n in lens]
    docs[2][7], docs[2][9] = V, -1
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = np.concatenate(docs).astype(np.int32)
    lab_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    lab = np.concatenate([np.arange(c) for c in counts]).astype(np.int32)
    allowed = np.zeros((len(lens), K), dtype=np.uint8)
    for d, c in enumerate(counts):
        allowed[d, :c] = 1
    ids = [5, 2 ** 32 + 1, 0, 3, 2 ** 35, 9]
    dense = dense_run(phi_t, K, doc_off, word, 0.3, R, SEED, STREAM, allowed=allowed, doc_ids=ids)
    got = run(phi_t, K, doc_off, word, lab_off, lab, len(lab), max_labels, 0.3, R, SEED, STREAM, doc_ids=ids)
    check(got, dense, "K %d" % K)
    assert got[2].sum() > 0 and got[3][5] == 3 and got[2][5] == 0       # (the document without a label: all bad, in both)


def test_no_document_is_a_no_op_and_the_python_surface():
    import torch
    from lda_thesis_amd import _native, leftright
    t = torch.zeros((1, 2000), dtype=torch.float64, device="cuda:0")
    _native.left_to_right_sparse(None, None, t, None, None, 0, 1, 2000, 0, 4, particles=2, alpha=0.1, seed=1, stream_id=0, max_doc_tokens=1,
                                 mant=None, expo=None, tok=None, bad=None)
    rng = np.random.default_rng(65)
    K = 1100
    phi_t = loadings(rng, K)
    doc_off, word, lab_off, lab, NL = batch(rng, K, 8, plan=((5, "full"), (9, "full"), (0, "half"), (8, "one")))
    word = np.where((word < 0) | (word >= V), 3, word)
    want = sparseheldref.left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, 0.2, 5, SEED, leftright.LR_STREAM, K=K, doc_ids=[4, 3, 2, 1])
    d_phi = torch.from_numpy(phi_t).to("cuda:0")
    got = leftright.loglik_sparse(d_phi, doc_off, word, lab_off, lab, 0.2, 5, SEED, doc_ids=[4, 3, 2, 1])
    check(got + (0,), want, "python surface")
    with pytest.raises(ValueError):
        leftright.loglik_sparse(d_phi, doc_off, word, lab_off, lab[::-1].copy(), 0.2, 5, SEED)
    with pytest.raises(ValueError):
        leftright.loglik_sparse(d_phi, doc_off, word, lab_off, lab, 0.2, 17, SEED)
    with pytest.raises(ValueError):
        leftright.loglik_sparse(d_phi, doc_off, word, np.array([0, 33, 33, 33, 33]), np.arange(33), 0.2, 5, SEED)
