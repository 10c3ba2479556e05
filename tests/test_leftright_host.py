"""llda_left_to_right without a GPU: the entry point's refusals, the CPU restatement (tests/leftrightref.py) against closed forms and
exact enumeration that do not come from it, and the host helpers of lda_thesis_amd.leftright."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import leftrightref as ref
from heldoutref import pair_mul
from lda_thesis_amd import leftright

SEED = 0x5EEDF00DCAFE


def mean_of_equal(pred, R):
    """the mean of R particles that all predict pred, by the header's rule: added in increasing r from +0.0, one division.  It is
    pred itself for R = 1, 2 and 4; from the fifth term on a partial sum may round, so for R = 8 it is taken as specified"""
    tot = 0.0
    for _ in range(R):
        tot = tot + pred
    return tot / float(R)


def _pair(values, R=1):
    acc = (0.5, 1)
    for v in values:
        m, e = math.frexp(mean_of_equal(v, R))
        acc = pair_mul(acc[0], acc[1], m, e)
    return acc


def test_symbols_struct_and_refusals():
    """both symbols are declared, exported and bound; the struct size is the binding's; the ABI has not moved; every refusal the
    header states comes back before anything touches HIP (the pointers below are never dereferenced on the host)"""
    from lda_thesis_amd import _native
    from test_abi import declared_symbols
    L = _native.lib()
    assert L.llda_abi_version() == 22 and L.llda_struct_size(7) == -1
    for s in ("llda_leftright_struct_bytes", "llda_left_to_right"):
        assert s in _native.EXPORTS and s in declared_symbols()
    assert L.llda_leftright_struct_bytes() == ctypes.sizeof(_native.LldaLeftrightArgs)
    assert (_native.LR_MAX_PARTICLES, _native.LR_MAX_TOKENS, _native.LR_MAX_K) == (16, 4096, 1024)
    BAD_K, BAD_ARG = -1, -2

    def call(**kw):
        a = _native.LldaLeftrightArgs()
        a.struct_bytes = ctypes.sizeof(a)
        a.doc_off, a.word, a.phi_t, a.allowed, a.doc_ids = 4096, 8192, 12288, 16384, 20480
        a.mant, a.expo, a.tok, a.bad, a.status = 24576, 28672, 32768, 36864, 40960
        a.D, a.V, a.K, a.R, a.ld_phi, a.ld_allowed, a.max_doc_tokens, a.alpha = 2, 10, 8, 4, 8, 8, 100, 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return L.llda_left_to_right(ctypes.byref(a), None)

    assert L.llda_left_to_right(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(_native.LldaLeftrightArgs) + 8) == BAD_ARG
    for K in (0, -1, 1025, 7688):
        assert call(K=K, ld_phi=8000, ld_allowed=8000) == BAD_K, K
    for name in ("doc_off", "word", "phi_t", "mant", "expo", "tok", "bad"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(D=-1) == BAD_ARG
    assert call(V=0) == BAD_ARG and call(V=2 ** 31) == BAD_ARG
    assert call(ld_phi=7) == BAD_ARG and call(ld_allowed=7) == BAD_ARG
    for R in (0, -1, 17):
        assert call(R=R) == BAD_ARG, R
    for alpha in (0.0, -0.5, float("inf"), float("nan")):
        assert call(alpha=alpha) == BAD_ARG, alpha
    for n in (0, -1, 4097):
        assert call(max_doc_tokens=n) == BAD_ARG, n
    for name in ("doc_off", "phi_t", "doc_ids", "mant", "expo", "tok", "bad"):
        assert call(**{name: 4100}) == BAD_ARG, name                   # not 8-byte aligned
    for name in ("word", "status"):
        assert call(**{name: 4098}) == BAD_ARG, name                   # not 4-byte aligned
    assert call(D=0) == 0                                               # nothing to score
    assert call(D=0, doc_off=None, word=None, phi_t=None, mant=None) == 0
    assert call(D=0, R=0) == BAD_ARG and call(D=0, K=0) == BAD_K       # (the scalars are looked at first)


@pytest.mark.parametrize("R", (1, 3, 16, 64))
def test_one_token_is_the_prior_predictive(R):
    """N = 1: p = sum64(alpha * phi) / (A * alpha), whatever R -- the R equal terms pred added from +0.0 and divided by R are
    recomputed here as such"""
    rng = np.random.default_rng(5)
    K, V, alpha = 70, 9, 0.37
    phi_t = rng.gamma(0.4, size=(V, K)) + 1e-6
    allowed = np.zeros((V, K), dtype=np.uint8)
    allowed[:, [1, 65, 69]] = 1
    allowed[0] = 1
    doc_off, word = np.arange(V + 1), np.arange(V)
    mant, expo, tok, bad, _ = ref.left_to_right_ref(phi_t, doc_off, word, alpha, R, SEED, 7, allowed=allowed)
    for d in range(V):
        x = np.where(allowed[d] != 0, (0.0 + alpha) * phi_t[d], 0.0)
        A = int(allowed[d].sum())
        pred = float(ref.sum64(x[None, :])[0]) / (0.0 + float(A) * alpha)
        assert (mant[d], expo[d]) == math.frexp(mean_of_equal(pred, R)) and tok[d] == 1 and bad[d] == 0
        # ... and sum64 against an independent sum, to rounding
        assert abs(float(ref.sum64(x[None, :])[0]) / math.fsum(x.tolist()) - 1) < 1e-13


@pytest.mark.parametrize("R", (1, 2, 4, 8))
def test_one_hot_loadings_leave_nothing_to_chance(R):
    """every word has exactly one allowed topic with phi > 0: each draw has one candidate, so z_n is that topic in every particle
    and pred_r = ((c + alpha) * phi) / (n + A * alpha) in every particle, p_n their mean (mean_of_equal) -- the pair must be the
    direct product bit for bit, for N up to 40 with repeated words"""
    rng = np.random.default_rng(11)
    K, V, alpha = 130, 12, 0.21
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
    A = K - 1
    trace = {}
    mant, expo, tok, bad, _ = ref.left_to_right_ref(phi_t, doc_off, np.concatenate(docs), alpha, R, SEED, 3, allowed=allowed, trace=trace)
    for d, ws in enumerate(docs):
        c = np.zeros(K)
        ps = []
        for n, w in enumerate(ws):
            t = topic_of[w]
            ps.append(((c[t] + alpha) * phi_t[w, t]) / (float(n) + float(A) * alpha))
            c[t] += 1.0
        assert (mant[d], expo[d]) == _pair(ps, R), (R, d)
        assert R > 4 or _pair(ps, R) == _pair(ps)
        assert tok[d] == len(ws) and bad[d] == 0
        assert (trace["z"][d, :, :len(ws)] == topic_of[ws][None, :]).all()


def test_a_word_without_an_allowed_topic_is_bad_and_stays_unassigned():
    """word 2 is zero on every allowed topic: its position is bad, holds no assignment and does not count in the later
    denominators; a word id outside [0, V) behaves the same"""
    K, V, alpha, R = 3, 4, 0.5, 4
    phi_t = np.array([[0.2, 0.0, 0.0], [0.0, 0.3, 0.0], [0.0, 0.0, 0.7], [0.1, 0.0, 0.0]])
    allowed = np.array([[1, 1, 0]] * 2, dtype=np.uint8)
    docs = [[0, 2, 0, 1], [0, 9, 0, 1]]
    trace = {}
    mant, expo, tok, bad, _ = ref.left_to_right_ref(phi_t, [0, 4, 8], sum(docs, []), alpha, R, SEED, 3, allowed=allowed, trace=trace)
    A = 2
    want = _pair([((0 + alpha) * 0.2) / (0.0 + A * alpha), ((1 + alpha) * 0.2) / (1.0 + A * alpha), ((0 + alpha) * 0.3) / (2.0 + A * alpha)])
    for d in range(2):
        assert (mant[d], expo[d], tok[d], bad[d]) == (want[0], want[1], 3, 1)
        assert (trace["z"][d, :, 1] == ref.NONE).all() and (trace["z"][d, :, [0, 2, 3]] != ref.NONE).all()
    assert trace["p"][0, 1] == 0.0 and math.isnan(trace["p"][1, 1])


def _exact(phi_t, ws, topics, alpha):
    """p(w) by summing over all assignments of the tokens to the allowed topics"""
    A, total = len(topics), 0.0
    for zs in itertools.product(range(A), repeat=len(ws)):
        c, p = [0] * A, 1.0
        for n, (w, zi) in enumerate(zip(ws, zs)):
            p *= (c[zi] + alpha) / (n + A * alpha) * phi_t[w, topics[zi]]
            c[zi] += 1
        total += p
    return total


def _cases():
    rng = np.random.default_rng(2009)
    out = []
    for K, topics, ws, alpha in ((3, [0, 1, 2], [0, 1, 0, 2], 0.3), (2, [0, 1], [1, 1, 0], 1.1), (70, [1, 65, 69], [3, 0, 3, 1], 0.15)):
        phi = rng.gamma(0.5, size=(K, 5)) + 1e-3
        phi /= phi.sum(axis=1, keepdims=True)
        out.append((np.ascontiguousarray(phi.T), topics, ws, alpha))
    return out


@pytest.mark.parametrize("case", range(3))
@pytest.mark.parametrize("R", (64,))
def test_consistent_with_exact_enumeration(case, R):
    """the mean of the estimates under the 40 independent keys of the document ids 0 .. 39 lies within 5 standard errors (from
    their own spread) of the exactly enumerated p(w); the inputs are fixed above, once"""
    phi_t, topics, ws, alpha = _cases()[case]
    K = phi_t.shape[1]
    allowed = np.zeros((40, K), dtype=np.uint8)
    allowed[:, topics] = 1
    doc_off = np.arange(41) * len(ws)
    mant, expo, tok, bad, _ = ref.left_to_right_ref(phi_t, doc_off, ws * 40, alpha, R, SEED, 100, allowed=allowed)
    assert (tok == len(ws)).all() and not bad.any()
    est = mant * np.exp2(expo.astype(np.float64))
    want = _exact(phi_t, ws, topics, alpha)
    se = est.std(ddof=1) / math.sqrt(40)
    print("case %d R %d: exact %.6e mean %.6e, %.2f standard errors" % (case, R, want, est.mean(), (est.mean() - want) / se))
    assert len(set(est.tolist())) > 1 and abs(est.mean() - want) <= 5 * se


def test_documents_do_not_depend_on_their_batch():
    rng = np.random.default_rng(3)
    K, V = 5, 6
    phi_t = rng.gamma(0.5, size=(V, K)) + 1e-3
    docs = [rng.integers(0, V, size=n).tolist() for n in (4, 0, 9, 3)]
    off = np.concatenate([[0], np.cumsum([len(t) for t in docs])])
    full = ref.left_to_right_ref(phi_t, off, sum(docs, []), 0.2, 3, SEED, 9, doc_ids=[7, 8, 2 ** 32 + 7, 11], max_doc_tokens=8)
    assert full[4] == 1 and (full[0][2], full[1][2], full[2][2], full[3][2]) == (0.5, 1, 0, 0)       # the long one is not scored
    assert (full[0][1], full[1][1], full[2][1], full[3][1]) == (0.5, 1, 0, 0)
    alone = ref.left_to_right_ref(phi_t, [0, 4], docs[0], 0.2, 3, SEED, 9, doc_ids=[7])
    assert [x[0] for x in alone[:4]] == [x[0] for x in full[:4]]
    twin = ref.left_to_right_ref(phi_t, [0, 3, 7], docs[3] + docs[0], 0.2, 3, SEED, 9, doc_ids=[11, 2 ** 32 + 7])
    assert [x[1] for x in twin[:4]] == [x[0] for x in full[:4]] and [x[0] for x in twin[:4]] == [x[3] for x in full[:4]]
    other = ref.left_to_right_ref(phi_t, [0, 4], docs[0], 0.2, 3, SEED, 9, doc_ids=[6])
    assert other[0][0] != alone[0][0]


def test_host_helpers():
    off, word = leftright.tokens_csr([[3, 1, 3], [], [2]])
    assert off.tolist() == [0, 3, 3, 4] and off.dtype == np.int64 and word.tolist() == [3, 1, 3, 2] and word.dtype == np.int32
    assert leftright.tokens_csr([])[0].tolist() == [0]
    labelmap = {"root": 0, "a": 1, "b": 2, "c": 3}
    m = leftright.allowed_matrix([["b"], [], ["a", "c"]], labelmap, 4)
    assert m.dtype == np.uint8 and m.tolist() == [[1, 0, 1, 0], [1, 0, 0, 0], [1, 1, 0, 1]]
    with pytest.raises(KeyError):
        leftright.allowed_matrix([["nope"]], labelmap, 4)
    long = list(range(5000))
    kept, index = leftright.prepare_tokens([[1, 2, 3], [], long, [4]], None)
    assert kept == [[1, 2, 3], [4]] and index == [0, 3]                 # nothing left, and more than 4096: skipped
    kept, index = leftright.prepare_tokens([[1, 2, 3], [], long, [4]], 2)
    assert kept == [[1, 2], [0, 1], [4]] and index == [0, 2, 3]         # only the first tokens are scored
    kept, index = leftright.prepare_tokens([long], 4096)
    assert len(kept[0]) == 4096 and index == [0]
    with pytest.raises(ValueError):
        leftright.prepare_tokens([[1]], 0)
    from lda_thesis_amd.foldin import CASCADE_STREAM, TEST_STREAM
    streams = set(range(leftright.LR_STREAM, leftright.LR_STREAM + leftright.MAX_PARTICLES))
    assert TEST_STREAM not in streams and max(streams) < CASCADE_STREAM and min(streams) > TEST_STREAM


def test_python_surface_refuses_host_tensors_and_missing_device():
    import torch
    with pytest.raises(Exception) as e:
        leftright.loglik(torch.zeros((3, 2), dtype=torch.float64), [0, 0], [], 0.1, 2, 1)
    assert isinstance(e.value, (ValueError, RuntimeError))             # no device: NativeError; a device: the tensor is not on it


def test_harness_option_is_off_by_default():
    from lda_thesis_amd import evaluate_LabeledLDA as E
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2"])[0].left_to_right == 0
    assert E.build_parser().parse_args(["-f", "x.csv", "-i", "2", "--left-to-right", "5"])[0].left_to_right == 5
