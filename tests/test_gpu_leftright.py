"""llda_left_to_right on the device against its CPU restatement (tests/leftrightref.py), bit for bit on all four outputs."""
import functools
import math

import numpy as np
import pytest

import leftrightref as ref

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567
STREAM = 0xFFFFFFF8                                                     # stream_id + r wraps around 2^32 for the later particles
V = 50
LENS = (0, 1, 2, 3, 17, 64, 65, 70, 5, 17, 9)                           # 70: longer than max_doc_tokens = 65
CAP = 65
R_OF_K = {1: 1, 2: 2, 31: 3, 32: 16, 33: 1, 63: 2, 64: 3, 65: 16, 127: 1, 128: 2, 129: 3, 392: 16, 512: 2, 1000: 3, 1024: 16}


def device_run(phi_t, K, doc_off, word, alpha, R, seed, stream, allowed=None, doc_ids=None, cap=None, pad=3):
    """llda_left_to_right through the binding with ld_phi = K + pad and ld_allowed = K + pad, NaN / 1 beyond K.  Returns
    (mant, expo, tok, bad, status) as numpy values."""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda")
    D = len(doc_off) - 1
    wide = np.full((phi_t.shape[0], K + pad), np.nan)
    wide[:, :K] = phi_t[:, :K]
    d_phi = torch.from_numpy(wide).to(dev)
    d_allowed = None
    if allowed is not None:
        wa = np.ones((D, K + pad), dtype=np.uint8)
        wa[:, :K] = allowed[:, :K]
        d_allowed = torch.from_numpy(wa).to(dev)
    d_off = torch.from_numpy(np.asarray(doc_off, dtype=np.int64)).to(dev)
    d_word = torch.from_numpy(np.concatenate([np.asarray(word, dtype=np.int32), np.zeros(1, dtype=np.int32)])).to(dev)
    d_ids = None if doc_ids is None else torch.from_numpy(np.asarray(doc_ids, dtype=np.int64)).to(dev)
    mant = torch.full((max(D, 1),), -7.0, dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.full((max(D, 1),), -7, dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    lens = np.diff(np.asarray(doc_off, dtype=np.int64))
    cap = max(1, int(lens.max()) if D else 1) if cap is None else cap
    _native.left_to_right(d_off, d_word, d_phi, D, phi_t.shape[0], K, particles=R, alpha=alpha, seed=seed, stream_id=stream,
                          max_doc_tokens=cap, mant=mant, expo=expo, tok=tok, bad=bad, ld_phi=K + pad, allowed=d_allowed,
                          ld_allowed=K + pad, doc_ids=d_ids, status=status)
    torch.cuda.synchronize()
    return mant.cpu().numpy()[:D], expo.cpu().numpy()[:D], tok.cpu().numpy()[:D], bad.cpu().numpy()[:D], int(status.item())


def _loadings(rng, K):
    """positive loadings across eight orders of magnitude; word 0 loads on nothing, the rows 1 and 2 are scaled by 2^200 and 2^-200"""
    phi_t = rng.gamma(0.5, size=(V, K)) * 10.0 ** rng.uniform(-8, 0, size=(V, K)) + 1e-300
    phi_t[0] = 0.0
    phi_t[1] *= 2.0 ** 200
    phi_t[2] *= 2.0 ** -200
    return phi_t


def _batch(rng, K):
    docs = [rng.integers(1, V, size=n) for n in LENS]
    docs[4][8] = 0                                                      # a zero-probability word in the middle of a document
    docs[9][3] = V                                                      # word ids outside [0, V)
    docs[9][11] = -1
    docs[10] = docs[8][:5].tolist() + [1, 2, 1, 2]                      # the scaled rows next to one another
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])])
    word = np.concatenate([np.asarray(t, dtype=np.int64) for t in docs])
    allowed = np.ones((len(docs), K), dtype=np.uint8)                   # document d: every topic, one topic, the topics at a
    for d in range(len(docs)):                                          # lane seam (or the two ends), only the last topic
        kind = d % 4
        if kind:
            allowed[d] = 0
            allowed[d, {1: [K // 2], 2: [63, 64] if K > 64 else [0, K - 1], 3: [K - 1]}[kind]] = 1
    return doc_off, word, allowed


@functools.lru_cache(maxsize=None)
def _case(K, masked):
    rng = np.random.default_rng(7000 + K)
    phi_t = _loadings(rng, K)
    doc_off, word, allowed = _batch(rng, K)
    allowed = allowed if masked else None
    alpha = 0.3
    want = ref.left_to_right_ref(phi_t, doc_off, word, alpha, R_OF_K[K], SEED, STREAM, allowed=allowed, max_doc_tokens=CAP)
    return phi_t, doc_off, word, allowed, alpha, want


def _check(got, want):
    names = ("mant", "expo", "tok", "bad")
    for name, g, w in zip(names, got[:4], want[:4]):
        diff = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert diff.size == 0, "%s differs at documents %s: %s != %s" % (name, diff[:5], np.asarray(g)[diff[:5]], np.asarray(w)[diff[:5]])
    assert got[4] == want[4]


@pytest.mark.parametrize("K", sorted(R_OF_K))
def test_device_equals_restatement_masked(K):
    """lengths 0 .. 65 mixed in one batch, a mask of every kind, ld > K with poison beyond, loadings across magnitudes, a
    zero-probability word, word ids outside the vocabulary and a document that is too long"""
    phi_t, doc_off, word, allowed, alpha, want = _case(K, True)
    got = device_run(phi_t, K, doc_off, word, alpha, R_OF_K[K], SEED, STREAM, allowed=allowed, cap=CAP)
    _check(got, want)
    over = LENS.index(70)
    assert got[4] == 1 and (got[0][over], got[1][over], got[2][over], got[3][over]) == (0.5, 1, 0, 0)
    assert (got[0][0], got[1][0], got[2][0], got[3][0]) == (0.5, 1, 0, 0)              # the empty document
    assert got[3][4] >= 1 and got[3][9] >= 2 and got[2][5] > 0


@pytest.mark.parametrize("K", (33, 129, 512))
def test_device_equals_restatement_without_a_mask(K):
    phi_t, doc_off, word, allowed, alpha, want = _case(K, False)
    _check(device_run(phi_t, K, doc_off, word, alpha, R_OF_K[K], SEED, STREAM, cap=CAP), want)


def test_a_long_document():
    """N = 200 (the Philox blocks of a wavefront are renewed after 128 positions) next to short ones"""
    rng = np.random.default_rng(200)
    K, R = 65, 2
    phi_t = _loadings(rng, K)
    docs = [rng.integers(1, V, size=n) for n in (3, 200, 1)]
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])])
    word = np.concatenate(docs)
    want = ref.left_to_right_ref(phi_t, doc_off, word, 0.05, R, SEED, 5)
    _check(device_run(phi_t, K, doc_off, word, 0.05, R, SEED, 5), want)


def test_a_document_does_not_depend_on_its_place():
    """the same document at two places of a batch (by doc_ids) and alone: identical outputs; another id: another estimate"""
    rng = np.random.default_rng(12)
    K, R = 129, 3
    phi_t = _loadings(rng, K)
    doc = rng.integers(1, V, size=30)
    others = [rng.integers(1, V, size=n) for n in (7, 41)]
    docs = [others[0], doc, others[1], doc, doc]
    doc_off = np.concatenate([[0], np.cumsum([len(t) for t in docs])])
    ids = [5, 1000, 6, 2 ** 32 + 1000, 1001]
    got = device_run(phi_t, K, doc_off, np.concatenate(docs), 0.2, R, SEED, 5, doc_ids=ids)
    alone = device_run(phi_t, K, [0, 30], doc, 0.2, R, SEED, 5, doc_ids=[1000], cap=300)
    for x, y in zip(got[:4], alone[:4]):
        assert x[1] == x[3] == y[0]
    assert (got[0][4], got[1][4]) != (got[0][1], got[1][1])
    _check(got, ref.left_to_right_ref(phi_t, doc_off, np.concatenate(docs), 0.2, R, SEED, 5, doc_ids=ids))


def test_no_document_is_a_no_op():
    got = device_run(np.ones((V, 4)), 4, [0], [], 0.1, 2, SEED, 5)
    assert got[4] == 0 and all(len(x) == 0 for x in got[:4])


@pytest.mark.parametrize("R", (1, 2, 4, 8))
def test_one_hot_closed_form_on_the_device(R):
    """loadings under which nothing is random (tests/test_leftright_host.py): the device's pair is the direct product"""
    from test_leftright_host import _pair
    rng = np.random.default_rng(11)
    K, alpha = 130, 0.21
    topic_of = rng.integers(0, K, size=V)
    topic_of[:3] = (0, 64, 129)
    phi_t = np.zeros((V, K))
    phi_t[np.arange(V), topic_of] = rng.uniform(0.01, 0.9, size=V)
    phi_t[:, 5] = 0.5                                                   # a topic every word loads on, allowed to no document
    lens = [1, 2, 7, 40, 33]
    docs = [rng.integers(0, V, size=n) for n in lens]
    doc_off = np.concatenate([[0], np.cumsum(lens)])
    allowed = np.ones((len(lens), K), dtype=np.uint8)
    allowed[:, 5] = 0
    got = device_run(phi_t, K, doc_off, np.concatenate(docs), alpha, R, SEED, 3, allowed=allowed)
    for d, ws in enumerate(docs):
        c, ps = np.zeros(K), []
        for n, w in enumerate(ws):
            t = topic_of[w]
            ps.append(((c[t] + alpha) * phi_t[w, t]) / (float(n) + float(K - 1) * alpha))
            c[t] += 1.0
        assert (got[0][d], got[1][d]) == _pair(ps, R) and got[2][d] == len(ws) and got[3][d] == 0
        assert math.isfinite(got[0][d])
