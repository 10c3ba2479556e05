"""The document model on sparse label sets without a GPU: the restatement tests/sparseref.py against the dense restatements
(attrref.py on every document's compacted problem, attrref.py / emref.py at full K for prefix label sets), the unfit-document rules,
docmodel.label_csr, and the C ABI of llda_attribute_sparse / llda_credit_words_sparse -- the exported symbols, the two structs and
every refusal of the header, all decided on the host before any HIP call (the pointers below are never dereferenced there)."""
import ctypes

import numpy as np
import pytest

import attrref
import emref
import sparseref

BAD_K, BAD_ARG = -1, -2
MAX_K = 7688


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def toy(seed, D=40, V=23, K=70, lens=(0, 1, 2, 5, 9, 17), counts=(0, 1, 2, 4, 7, 8, 9), prefix=False):
    """a random corpus with label sets of the given sizes: the CSR of the sites, lab_off / lab, theta_s [NL] (an exact zero here and
    there), phi_t (V, K) positive with an all-zero row, words outside the vocabulary among the sites"""
    rng = np.random.default_rng(seed)
    n = rng.choice(lens, size=D)
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = np.minimum((rng.zipf(1.3, size=S) - 1), V - 1).astype(np.int32)
    word[rng.random(S) < 0.03] = V
    word[rng.random(S) < 0.03] = -1
    freq = rng.integers(0, 5, size=S).astype(np.int32)
    sets = []
    for d in range(D):
        L = int(rng.choice(counts))
        sets.append(np.arange(L) if prefix else np.sort(rng.choice(K, size=L, replace=False)))
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    lab = np.concatenate(sets + [np.zeros(0)]).astype(np.int32)
    theta_s = rng.gamma(0.5, size=lab.shape[0]) + 1e-3
    theta_s[rng.random(lab.shape[0]) < 0.1] = 0.0
    phi_t = rng.gamma(0.3, size=(V, K)) + 1e-6
    phi_t /= phi_t.sum(axis=0, keepdims=True)
    phi_t[1] = 0.0
    return dict(doc_off=doc_off, word=word, freq=freq, lab_off=lab_off, lab=lab, theta_s=theta_s, phi_t=phi_t, D=D, V=V, K=K)


@pytest.mark.parametrize("iters,alpha,top_m", ((0, 0.0, 4), (1, 0.1, 1), (3, 0.0, 0), (2, 0.05, 3)))
def test_document_side_is_attrref_on_every_compacted_problem(iters, alpha, top_m):
    c = toy(1 + iters)
    got = sparseref.attribute_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], iters=iters,
                                         alpha=alpha, top_m=top_m)
    seen = 0
    for d in range(c["D"]):
        b, e, lb, le = int(c["doc_off"][d]), int(c["doc_off"][d + 1]), int(c["lab_off"][d]), int(c["lab_off"][d + 1])
        if le == lb:                                                       # fit, no slot: every site is bad
            assert got["tok"][d] == 0 and got["bad"][d] == int(c["freq"][b:e].sum()) and (got["site_idx"][b:e] == -1).all()
            continue
        ids = c["lab"][lb:le].astype(np.int64)
        one = attrref.attribute_ref(c["theta_s"][None, lb:le], np.ascontiguousarray(c["phi_t"][:, ids]), np.array([0, e - b]), c["word"][b:e],
                                    c["freq"][b:e], iters=iters, alpha=alpha, top_m=top_m)
        for name in ("theta_out", "credit"):
            assert np.array_equal(bits(got[name][lb:le]), bits(one[name][0])), (d, name)
        assert got["tok"][d] == one["tok"][0] and got["bad"][d] == one["bad"][0]
        assert np.array_equal(bits(got["site_val"][b:e]), bits(one["site_val"]))
        assert np.array_equal(got["site_idx"][b:e], np.where(one["site_idx"] >= 0, ids[np.maximum(one["site_idx"], 0)], -1))
        seen += int(one["tok"][0] > 0)
    assert seen > 10 and got["bad"].sum() > 0


@pytest.mark.parametrize("K", (9, 33, 70))
def test_prefix_label_sets_give_the_dense_bits_at_full_k(K):
    """labels 0 .. L_d - 1 and a dense row that is 0 elsewhere: adding +0.0 to a sum that is never -0.0 is the identity"""
    c = toy(10 + K, K=K, counts=(1, 2, 7, 8, 9), prefix=True)
    dense = sparseref.scatter(c["theta_s"], c["lab_off"], c["lab"], K)
    assert np.array_equal(bits(sparseref.gather(dense, c["lab_off"], c["lab"])), bits(c["theta_s"]))
    for iters, alpha, top_m in ((0, 0.0, 2), (2, 0.1, 4)):
        want = attrref.attribute_ref(dense, c["phi_t"], c["doc_off"], c["word"], c["freq"], iters=iters, alpha=alpha, top_m=top_m)
        got = sparseref.attribute_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"],
                                             iters=iters, alpha=alpha, top_m=top_m)
        for name in ("theta_out", "credit"):
            assert np.array_equal(bits(sparseref.scatter(got[name], c["lab_off"], c["lab"], K)), bits(want[name])), name
        for name in ("site_idx", "site_val", "tok", "bad"):
            assert np.array_equal(bits(got[name]), bits(want[name])), name
    ok = (c["word"] >= 0) & (c["word"] < c["V"])
    order = np.argsort(c["word"][ok], kind="stable")                       # the sites inside the vocabulary, word-major
    word_off = np.concatenate([[0], np.cumsum(np.bincount(c["word"][ok], minlength=c["V"]))]).astype(np.int64)
    site_doc = np.repeat(np.arange(c["D"]), np.diff(c["doc_off"]))[ok][order].astype(np.int32)
    w_freq = c["freq"][ok][order]
    site_doc[::17] = c["D"]                                                # a few sites of documents that do not exist
    for chunk in (1, 3, 4096):
        want = emref.credit_words_ref(dense, c["phi_t"], word_off, site_doc, w_freq, chunk)
        got = sparseref.credit_words_sparse_ref(c["theta_s"], c["phi_t"], word_off, site_doc, w_freq, c["lab_off"], c["lab"], chunk)
        for name in want:
            assert np.array_equal(bits(got[name]), bits(want[name])), (chunk, name)
        assert want["tok"].sum() > 0 and want["bad"].sum() > 0


def test_label_csr_round_trips_and_refuses():
    from lda_thesis_amd import docmodel
    rng = np.random.default_rng(3)
    labs = (rng.random((30, 12)) < 0.3).astype(np.int64)
    labs[4] = 0
    off, lab = docmodel.label_csr(labs)
    assert off.dtype == np.int64 and lab.dtype == np.int32 and off.shape == (31,) and off[-1] == labs.sum() == lab.shape[0]
    back = np.zeros_like(labs)
    back[np.repeat(np.arange(30), np.diff(off)), lab] = 1
    assert np.array_equal(back, labs) and off[5] == off[4]
    lists = [list(np.flatnonzero(r))[::-1] for r in labs]                  # any order in, ascending out
    off2, lab2 = docmodel.label_csr(lists, K=12)
    assert np.array_equal(off2, off) and np.array_equal(lab2, lab) and lab2.dtype == np.int32
    assert all((np.diff(lab[off[d]:off[d + 1]]) > 0).all() for d in range(30))
    e_off, e_lab = docmodel.label_csr([])
    assert e_off.tolist() == [0] and e_lab.shape == (0,)
    for bad in ([[0, 3, 3]], [[1], [2, -1]], [[12]]):
        with pytest.raises(ValueError):
            docmodel.label_csr(bad, K=12)
    with pytest.raises(ValueError):
        docmodel.label_csr(labs, K=13)
    # the check before a launch: what the kernel would call unfit is a ValueError on the host
    assert docmodel.label_sets(off, lab, 30, 12)[2:] == (int(off[-1]), int(np.diff(off).max()))
    assert docmodel.label_sets([0, 0], [], 1, 5)[2:] == (0, 1)
    for o, l, D, K in (([0, 2], [1, 1], 1, 5), ([0, 2], [2, 1], 1, 5), ([0, 1], [5], 1, 5), ([0, 1], [-1], 1, 5), ([1, 2], [0, 1], 1, 5),
                       ([0, 2, 1], [0, 1], 2, 5), ([0, 2], [0], 1, 5), ([0, 33], list(range(33)), 1, 40), ([0, 1], [0], 2, 5)):
        with pytest.raises(ValueError):
            docmodel.label_sets(o, l, D, K)
    assert docmodel.label_sets([0, 2, 4], [3, 4, 0, 1], 2, 5)[3] == 2      # the step from one list to the next may descend
    assert docmodel.label_sets([0, 32], list(range(32)), 1, 40)[3] == 32


def test_unfit_documents():
    """too many labels, an id = K, a negative id, a repeated label, a descending pair, offsets outside lab: never indexed, all bad"""
    K, V = 12, 7
    rng = np.random.default_rng(5)
    phi_t = rng.random((V, K)) + 0.1
    sets = [[0, 3, 5], [0, 1, 2, 3], [0, K], [-1, 2], [4, 4], [5, 2], [], [1, 7]]
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    lab = np.concatenate([np.asarray(s, dtype=np.int32) for s in sets])
    theta_s = rng.random(lab.shape[0]) + 0.1
    D = len(sets)
    doc_off = np.arange(0, 3 * D + 1, 3).astype(np.int64)
    word = rng.integers(0, V, size=3 * D).astype(np.int32)
    freq = rng.integers(1, 4, size=3 * D).astype(np.int32)
    got = sparseref.attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=K, max_labels=3, iters=2, alpha=0.1, top_m=2)
    fit = [sparseref.doc_fit(lab_off, lab, d, K, 3)[0] for d in range(D)]
    assert fit == [True, False, False, False, False, False, True, True]
    fsum = np.add.reduceat(freq.astype(np.int64), doc_off[:-1])
    for d in range(D):
        lb, le = int(lab_off[d]), int(lab_off[d + 1])
        if fit[d] and le > lb:
            assert got["tok"][d] == fsum[d] and got["bad"][d] == 0 and (got["site_idx"][3 * d:3 * d + 3, 0] >= 0).all()
            assert abs(got["theta_out"][lb:le].sum() - 1) < 1e-12 and abs(got["credit"][lb:le].sum() - fsum[d]) < 1e-9
        else:
            assert got["tok"][d] == 0 and got["bad"][d] == fsum[d] and (got["site_idx"][3 * d:3 * d + 3] == -1).all()
            assert np.array_equal(bits(got["theta_out"][lb:le]), bits(theta_s[lb:le])) and not got["credit"][lb:le].any()
    assert sparseref.doc_fit(lab_off, lab, 1, K, 4)[0] and not sparseref.doc_fit(np.array([0, 99]), lab, 0, K, 32)[1]
    # the word side: the sites of an unfit document are not ok
    word_off, site_doc, w_freq, _ = emref.word_major(doc_off, word, freq, V)
    cw = sparseref.credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, w_freq, lab_off, lab, 2, K=K, max_labels=3)
    unfit_sites = ~np.asarray(fit)[site_doc] | (np.diff(lab_off)[site_doc] == 0)
    assert cw["bad"].sum() == w_freq[unfit_sites].sum() and cw["tok"].sum() == w_freq[~unfit_sites].sum()
    reached = np.zeros(K, dtype=bool)
    reached[[0, 3, 5, 1, 7]] = True
    assert not cw["credit"][:, ~reached].any() and (np.signbit(cw["credit"]) == False).all()     # noqa: E712  (+0.0, never -0.0)
    np.testing.assert_allclose(cw["credit"].sum(), cw["tok"].sum(), rtol=1e-12)


def test_fit_sparse_ref_is_fit_ref_on_prefix_sets():
    c = toy(21, D=25, V=11, K=9, lens=(1, 3, 6), counts=(1, 2, 3, 8, 9), prefix=True)
    c["word"] = np.clip(c["word"], 0, c["V"] - 1)
    c["theta_s"] = np.where(c["theta_s"] == 0.0, 0.25, c["theta_s"])
    c["phi_t"][1] = 1e-3
    dense = sparseref.scatter(c["theta_s"], c["lab_off"], c["lab"], c["K"])
    want_th, want_phi = emref.fit_ref(dense, c["phi_t"], c["doc_off"], c["word"], c["freq"], 0.1, 0.01, 4, chunk=5)
    got_th, got_phi = sparseref.fit_sparse_ref(c["theta_s"], c["phi_t"], c["doc_off"], c["word"], c["freq"], c["lab_off"], c["lab"], 0.1, 0.01,
                                               4, chunk=5)
    assert np.array_equal(bits(sparseref.scatter(got_th, c["lab_off"], c["lab"], c["K"])), bits(want_th))
    assert np.array_equal(bits(got_phi), bits(want_phi))


# ---- the C ABI ----
@pytest.fixture(scope="module")
def nat():
    from lda_thesis_amd import _native
    _native.lib()
    return _native


def test_symbols_structs_and_constants(nat):
    from test_abi import declared_symbols
    L = nat.lib()
    assert L.llda_abi_version() == 22 == nat.ABI_VERSION                # additive: the ABI number stays
    for s in ("llda_attr_sparse_struct_bytes", "llda_attribute_sparse", "llda_wcredit_sparse_struct_bytes",
              "llda_credit_words_sparse_scratch_bytes", "llda_credit_words_sparse"):
        assert s in nat.EXPORTS and s in declared_symbols() and hasattr(L, s)
    assert L.llda_attr_sparse_struct_bytes() == ctypes.sizeof(nat.LldaAttrSparseArgs) == 168
    assert L.llda_wcredit_sparse_struct_bytes() == ctypes.sizeof(nat.LldaWcreditSparseArgs) == 160
    assert nat.SPARSE_MAX_LABELS == sparseref.MAX_LABELS == 32
    header = open(nat.os.path.join(nat.os.path.dirname(nat._HERE), "include", "llda_gibbs.h")).read()
    assert "#define LLDA_SPARSE_MAX_LABELS 32" in header
    for args in ((61, 1000, 7, 64), (1, 0, 1, 1), (100, 10 ** 6, 2048, 4096)):
        assert nat.credit_words_sparse_scratch_bytes(*args) == nat.credit_words_scratch_bytes(*args)
    for bad in ((0, 5, 8, 4), (5, -1, 8, 4), (5, 5, 0, 4), (5, 5, MAX_K + 1, 4), (5, 5, 8, 0)):
        assert L.llda_credit_words_sparse_scratch_bytes(*bad) == BAD_ARG, bad


def attr_call(nat, **kw):
    a = nat.LldaAttrSparseArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.max_labels, a.iters, a.top_m = 12, 8, 1, 0
    a.doc_off, a.word, a.freq, a.lab_off, a.lab, a.theta_s, a.phi_t = (4096 + 1024 * i for i in range(7))
    a.theta_out, a.credit, a.site_idx, a.site_val, a.tok, a.bad = (16384 + 1024 * i for i in range(6))
    a.D, a.V, a.NL, a.ld_phi, a.alpha = 5, 9, 20, 12, 0.1
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_attribute_sparse(ctypes.byref(a), None)


def test_attribute_sparse_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it) or has nothing to do: D = 0"""
    call = lambda **kw: attr_call(nat, **kw)
    assert call(D=0) == 0 and call(D=0, doc_off=None, word=None, lab_off=None, lab=None, theta_s=None, phi_t=None) == 0
    assert nat.lib().llda_attribute_sparse(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaAttrSparseArgs) + 8, D=0) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_phi=MAX_K + 1, D=0) == BAD_K, K
    assert call(K=MAX_K, ld_phi=MAX_K, D=0) == 0
    assert call(D=-1) == BAD_ARG and call(NL=-1, D=0) == BAD_ARG and call(ld_phi=11, D=0) == BAD_ARG
    for V in (0, -1, 2 ** 31):
        assert call(V=V, D=0) == BAD_ARG, V
    for m in (0, -1, 33, 2 ** 31 - 1):
        assert call(max_labels=m, D=0) == BAD_ARG, m
    for m in (1, 8, 9, 32):
        assert call(max_labels=m, D=0) == 0, m
    assert call(iters=-1, D=0) == BAD_ARG and call(alpha=-0.5, D=0) == BAD_ARG and call(alpha=float("nan"), D=0) == BAD_ARG
    assert call(top_m=-1, D=0) == BAD_ARG and call(top_m=5, D=0) == BAD_ARG and call(top_m=4, D=0) == 0
    assert call(top_m=1, site_idx=None, D=0) == BAD_ARG and call(top_m=1, site_val=None, D=0) == BAD_ARG
    assert call(top_m=1, site_idx=None, site_val=None, D=0) == 0
    for name in ("doc_off", "word", "lab_off", "lab", "theta_s", "phi_t"):
        assert call(**{name: None}) == BAD_ARG, name
    for name in ("doc_off", "lab_off", "theta_s", "phi_t", "theta_out", "credit", "site_val", "tok", "bad"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("word", "freq", "lab", "site_idx"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG               # V x ld leaves an int64


def wcredit_call(nat, **kw):
    a = nat.LldaWcreditSparseArgs()
    a.struct_bytes = ctypes.sizeof(a)
    a.K, a.chunk, a.max_labels = 12, 64, 8
    a.word_off, a.site_doc, a.freq, a.lab_off, a.lab, a.theta_s, a.phi_t = (4096 + 1024 * i for i in range(7))
    a.credit_w, a.tok, a.bad, a.scratch = (16384 + 1024 * i for i in range(4))
    a.D, a.V, a.S, a.NL, a.ld_phi, a.ld_credit, a.scratch_bytes = 5, 9, 100, 20, 12, 12, 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return nat.lib().llda_credit_words_sparse(ctypes.byref(a), None)


def test_credit_words_sparse_refusals_come_before_the_device(nat):
    """every call below is refused (there is no device to take it), or has nothing to launch: every output NULL"""
    call = lambda **kw: wcredit_call(nat, **kw)
    none = dict(credit_w=None, tok=None, bad=None)
    assert call(**none) == 0
    assert nat.lib().llda_credit_words_sparse(None, None) == BAD_ARG
    assert call(struct_bytes=0) == BAD_ARG and call(struct_bytes=ctypes.sizeof(nat.LldaWcreditSparseArgs) + 8) == BAD_ARG
    for K in (0, -1, MAX_K + 1):
        assert call(K=K, ld_phi=MAX_K + 1, ld_credit=MAX_K + 1) == BAD_K, K
    assert call(K=MAX_K, ld_phi=MAX_K, ld_credit=MAX_K, **none) == 0
    assert call(D=-1) == BAD_ARG and call(D=0, lab_off=None, **none) == 0 and call(NL=-1) == BAD_ARG
    for V in (0, -1, 2 ** 31):
        assert call(V=V) == BAD_ARG, V
    assert call(S=-1) == BAD_ARG and call(S=2 ** 40 + 1) == BAD_ARG
    for name in ("ld_phi", "ld_credit"):
        assert call(**{name: 11}) == BAD_ARG, name
    for chunk in (0, -1, -2 ** 31):
        assert call(chunk=chunk) == BAD_ARG, chunk
    for m in (0, -1, 33):
        assert call(max_labels=m) == BAD_ARG, m
    for m in (1, 8, 9, 32):
        assert call(max_labels=m, **none) == 0, m
    for name in ("word_off", "site_doc", "phi_t", "lab_off", "lab", "theta_s", "scratch"):
        assert call(**{name: None}) == BAD_ARG, name
    assert call(freq=None, **none) == 0 and call(NL=0, lab=None, theta_s=None, **none) == 0
    assert call(S=0, word_off=None, site_doc=None, phi_t=None, lab_off=None, lab=None, theta_s=None, scratch=None, scratch_bytes=0, **none) == 0
    for name in ("word_off", "lab_off", "theta_s", "phi_t", "credit_w", "tok", "bad", "scratch"):
        assert call(**{name: 4100}) == BAD_ARG, name                    # not 8-byte aligned
    for name in ("site_doc", "freq", "lab"):
        assert call(**{name: 4098}) == BAD_ARG, name                    # not 4-byte aligned
    need = nat.credit_words_sparse_scratch_bytes(9, 100, 12, 64)
    assert call(scratch_bytes=need - 1) == BAD_ARG and call(scratch_bytes=0) == BAD_ARG and call(scratch_bytes=need, **none) == 0
    assert call(chunk=1, scratch_bytes=need) == BAD_ARG                 # smaller chunks, more partial rows
    assert call(V=2 ** 31 - 1, ld_phi=2 ** 40) == BAD_ARG and call(V=2 ** 31 - 1, ld_credit=2 ** 40) == BAD_ARG
