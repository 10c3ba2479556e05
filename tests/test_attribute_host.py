"""llda_attribute without a device: the properties of its specification on the numpy restatement (tests/attrref.py), the struct
and every refusal through the real library (all decided before anything touches HIP), and the host helpers of attribution.py."""
import ctypes

import numpy as np
import pytest

import attrref

V = 40


def problem(rng, K, D=3, n_sites=25, zero_share=0.3):
    """sparse start loads with exact zeros, a smooth phi_t, documents of n_sites sites with mixed frequencies"""
    theta = rng.random((D, K)) + 0.05
    theta[rng.random((D, K)) < zero_share] = 0.0
    theta[:, 0] = 0.5                                                    # (never an all-zero row)
    theta /= theta.sum(axis=1, keepdims=True)
    phi_t = rng.gamma(0.3, size=(V, K)) / V + 1e-7
    doc_off = np.arange(D + 1, dtype=np.int64) * n_sites
    word = rng.integers(0, V, size=D * n_sites).astype(np.int32)
    freq = rng.integers(1, 5, size=D * n_sites).astype(np.int32)
    return theta, phi_t, doc_off, word, freq


@pytest.mark.parametrize("K", (7, 64, 65, 392))
def test_em_properties(K):
    """over 30 steps the objective sum f log p + alpha sum_{theta_k > 0} log theta_k never falls (relative slack 1e-9); the loads sum
    to 1 within rounding; the credit adds up to the tokens within 3e-14; a label that starts at 0 stays exactly 0"""
    rng = np.random.default_rng(100 + K)
    theta, phi_t, doc_off, word, freq = problem(rng, K)
    alpha = 0.1
    prev = None
    for iters in range(0, 31):
        r = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, iters=iters, alpha=alpha)
        obj = np.array([attrref.objective(r["theta_out"][d], phi_t, word[doc_off[d]:doc_off[d + 1]], freq[doc_off[d]:doc_off[d + 1]],
                                          alpha, K) for d in range(theta.shape[0])])
        if prev is not None:
            assert (obj >= prev - 1e-9 * np.abs(prev)).all(), (iters, obj, prev)
        prev = obj
        assert (r["bad"] == 0).all() and (r["tok"] == np.add.reduceat(freq, doc_off[:-1])).all()
        if iters:
            assert np.abs(r["theta_out"].sum(axis=1) - 1.0).max() < 1e-13
        assert np.abs(r["credit"].sum(axis=1) - r["tok"]).max() < 3e-14
        assert (r["theta_out"][theta == 0.0] == 0.0).all() and (r["credit"][theta == 0.0] == 0.0).all()
        assert not np.signbit(r["theta_out"]).any() and not np.signbit(r["credit"]).any()


def test_iters_zero_returns_the_bits_of_theta():
    rng = np.random.default_rng(1)
    theta, phi_t, doc_off, word, freq = problem(rng, 70)
    r = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, iters=0, alpha=0.3)
    assert np.array_equal(r["theta_out"].view(np.uint64), theta.view(np.uint64))


def test_tie_by_topic_id_and_padding():
    """two labels with equal theta and equal phi_t columns: the smaller id first, the same share; fewer positive labels than top_m:
    -1 / 0.0; a site that is not good (p = 0, p below 2^-960, a word outside the vocabulary): all -1 / 0.0 and f in bad"""
    K = 6
    theta = np.array([[0.25, 0.0, 0.25, 0.0, 0.5, 0.0]])
    phi_t = np.zeros((4, K))
    phi_t[0] = [0.1, 0.9, 0.1, 0.9, 0.05, 0.9]                            # labels 0 and 2 tie; label 4 the same product, a third tie
    phi_t[1] = [0.0, 0.9, 0.2, 0.9, 0.4, 0.9]                             # label 0 has no share
    phi_t[3] = 2.0 ** -961
    doc_off = np.array([0, 5], dtype=np.int64)
    word = np.array([0, 1, 2, 3, 7], dtype=np.int32)
    freq = np.array([2, 3, 5, 7, 11], dtype=np.int32)
    r = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, V=4, top_m=4)
    assert r["site_idx"][0].tolist() == [0, 2, 4, -1]
    assert r["site_val"][0, 0] == r["site_val"][0, 1] and r["site_val"][0, 3] == 0.0
    assert r["site_idx"][1].tolist() == [4, 2, -1, -1] and r["site_val"][1, 2:].tolist() == [0.0, 0.0]
    assert abs(r["site_val"][1, :2].sum() - 1.0) < 1e-15
    for s in (2, 3, 4):
        assert r["site_idx"][s].tolist() == [-1] * 4 and r["site_val"][s].tolist() == [0.0] * 4
    assert r["tok"][0] == 5 and r["bad"][0] == 23
    top1 = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, V=4, top_m=1)
    assert top1["site_idx"][:, 0].tolist() == [0, 4, -1, -1, -1]
    assert np.array_equal(top1["credit"], r["credit"])


def test_the_bound_on_p_is_2_to_the_minus_960():
    """p exactly 2^-960 is good, the double below it is not"""
    theta = np.array([[1.0, 0.0]])
    phi_t = np.array([[2.0 ** -960, 1.0], [np.nextafter(2.0 ** -960, 0.0), 1.0]])
    r = attrref.attribute_ref(theta, phi_t, np.array([0, 2]), np.array([0, 1], dtype=np.int32), None, top_m=1)
    assert r["site_idx"][:, 0].tolist() == [0, -1] and r["tok"][0] == 1 and r["bad"][0] == 1
    assert r["site_val"][0, 0] == 1.0 and r["credit"][0].tolist() == [1.0, 0.0]
    from lda_thesis_amd import _native
    assert _native.ATTR_MIN_P == attrref.MIN_P == float.fromhex("0x1p-960")


def test_empty_document_keeps_its_loads():
    theta = np.array([[0.25, 0.75, 0.0]])
    r = attrref.attribute_ref(theta, np.ones((2, 3)), np.array([0, 0]), np.zeros(0, dtype=np.int32), None, iters=3, alpha=0.1, top_m=2)
    assert np.array_equal(r["theta_out"], theta) and not r["credit"].any() and r["tok"][0] == 0 and r["bad"][0] == 0
    assert r["site_idx"].shape == (0, 2)


# ---- the real library, no device -----------------------------------------------------------------------------------------------
def test_struct_size_and_symbol():
    from lda_thesis_amd import _native
    L = _native.lib()
    assert L.llda_struct_size(6) == ctypes.sizeof(_native.LldaAttrArgs)
    assert L.llda_struct_size(7) == -1
    assert "llda_attribute" in _native.EXPORTS and hasattr(L, "llda_attribute")
    assert L.llda_abi_version() == 22


def test_refusals_one_by_one():
    """every refusal include/llda_gibbs.h states for llda_attribute, each with all the other arguments in order: decided on the host
    before anything touches HIP (no call below could launch: each has its one flaw, or D == 0; the pointers are never read)"""
    from lda_thesis_amd import _native
    L = _native.lib()
    BAD_K, BAD_ARG = -1, -2
    pointers = ("doc_off", "word", "freq", "theta", "phi_t", "theta_out", "credit", "site_idx", "site_val", "tok", "bad")

    def call(**change):
        a = _native.LldaAttrArgs()
        for name in pointers:
            setattr(a, name, 0x1000)
        a.D, a.V, a.K, a.ld_theta, a.ld_phi, a.ld_out, a.ld_credit, a.iters, a.top_m, a.alpha = 3, 10, 8, 8, 9, 8, 10, 2, 2, 0.1
        for k, v in change.items():
            setattr(a, k, v)
        return L.llda_attribute(ctypes.byref(a), None)

    assert L.llda_attribute(None, None) == BAD_ARG
    for name in ("doc_off", "word", "theta", "phi_t"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(D=-1) == BAD_ARG
    for v in (0, -1, 2 ** 31):
        assert call(V=v) == BAD_ARG, v
    for name in ("ld_theta", "ld_phi", "ld_out", "ld_credit"):
        assert call(**{name: 7}) == BAD_ARG, name
    assert call(iters=-1) == BAD_ARG
    for alpha in (-0.1, -1e-300, float("nan"), float("-inf")):
        assert call(alpha=alpha) == BAD_ARG, alpha
    for m in (-1, 5):
        assert call(top_m=m) == BAD_ARG, m
    assert call(site_idx=None) == BAD_ARG and call(site_val=None) == BAD_ARG
    for name in ("doc_off", "theta", "phi_t", "theta_out", "credit", "site_val", "tok", "bad"):
        assert call(**{name: 0x1004}) == BAD_ARG, name                   # 8-byte aligned
    for name in ("word", "freq", "site_idx"):
        assert call(**{name: 0x1002}) == BAD_ARG, name                   # 4-byte aligned
    for K in (0, -1, _native.MAX_K + 1):
        assert call(K=K) == BAD_K, K
    # D == 0: nothing to do, whatever the pointers; the refusals above still hold
    assert call(D=0) == 0
    assert call(D=0, K=_native.MAX_K, ld_theta=_native.MAX_K, ld_phi=_native.MAX_K, ld_out=_native.MAX_K, ld_credit=_native.MAX_K,
                **{name: None for name in pointers}) == 0
    assert call(D=0, top_m=5) == BAD_ARG and call(D=0, iters=-1) == BAD_ARG and call(D=0, K=0) == BAD_K


# ---- attribution.py on the host ------------------------------------------------------------------------------------------------
def test_uniform_start():
    from lda_thesis_amd import attribution
    u = attribution.uniform_start(None, 2, 5)
    assert u.shape == (2, 5) and u.dtype == np.float64 and (u == 1.0 / 5.0).all()
    u = attribution.uniform_start([[0, 3], [0], [4, 0, 4, 2]], 3, 5)
    assert u.tolist() == [[0.5, 0, 0, 0.5, 0], [1.0, 0, 0, 0, 0], [1.0 / 3.0, 0, 1.0 / 3.0, 0, 1.0 / 3.0]]
    for bad in ([[0, 5]], [[-1]], [[]]):
        with pytest.raises(ValueError):
            attribution.uniform_start(bad, 1, 5)
    with pytest.raises(ValueError):
        attribution.uniform_start([[0]], 2, 5)
    assert attribution.uniform_start(None, 0, 5).shape == (0, 5)


def test_explain_label_sets():
    """root plus the given labels, or root plus the n <= 3 best non-root labels of a ranking"""
    from lda_thesis_amd import attribution
    labelmap = {"root": 0, "A10": 1, "B20": 2, "C30": 3, "D40": 4}
    f = attribution.explain_label_cols
    assert f(labelmap, 2, labels=[["C30", "A10", "C30"], []]) == [[0, 1, 3], [0]]
    assert f(labelmap, 1, labels=[["root", "B20"]]) == [[0, 2]]
    with pytest.raises(KeyError):
        f(labelmap, 1, labels=[["Z99"]])
    with pytest.raises(ValueError):
        f(labelmap, 2, labels=[["A10"]])
    ranked = np.array([[4, 2, 1], [3, -1, -1]], dtype=np.int32)
    assert f(labelmap, 2, ranked=ranked, n=3) == [[0, 1, 2, 4], [0, 3]]
    assert f(labelmap, 2, ranked=ranked, n=2) == [[0, 2, 4], [0, 3]]
    for n in (0, 4):
        with pytest.raises(ValueError):
            f(labelmap, 2, ranked=ranked, n=n)
    with pytest.raises(ValueError):
        f(labelmap, 3, ranked=ranked, n=2)


def test_spans_and_explanations():
    from lda_thesis_amd import attribution
    doc_tups = [[(2, 3), (5, 1)], [], [(1, 2)]]
    idx = np.array([[1, 0], [0, -1], [2, 1]], dtype=np.int32)
    val = np.array([[0.75, 0.25], [1.0, 0.0], [0.6, 0.4]])
    a, b = attribution.spans([0, 2, 2, 3], idx, val)
    assert [x.shape for x in a] == [(2, 2), (0, 2), (1, 2)] and b[2].tolist() == [[0.6, 0.4]]
    credit = np.array([[1.75, 2.25, 0.0], [0.0, 0.0, 0.0], [0.0, 0.8, 1.2]])
    names, id2token = ["root", "A", "B"], {1: "one", 2: "two", 5: "five"}
    out = attribution.explanations(doc_tups, idx, val, credit, names, id2token)
    assert out[0] == ([("two", 3, [("A", 0.75), ("root", 0.25)]), ("five", 1, [("root", 1.0)])], {"root": 1.75, "A": 2.25})
    assert out[1] == ([], {}) and out[2] == ([("one", 2, [("B", 0.6), ("A", 0.4)])], {"A": 0.8, "B": 1.2})
