"""The quad kernels' fp64 tier 1 (quad_tier1_doc, csrc/kernel_quad.hpp) plays ONE unsure document on all 64 lanes of the wavefront, in a
loop over the documents tier 0 was unsure about.  The smallest shapes at which that loop can go wrong, against the C oracle
(LabeledLDA.py:106-125): two workgroups and one document more (the last workgroup's other lane groups walk a copy of the last document
with no sites), documents of 0, 1, 2 and up to 40 sites mixed inside a wavefront, one word in five with a count the 16-bit image cannot
hold (such a site skips tier 1, next to documents that take it), and the margins that send every document of every iteration through
the loop (debug_margin -2), many sites on to the exact tier (6) and almost none anywhere (0)."""
import numpy as np
import pytest

V, ALPHA, BETA, SEED, DOC_BASE = 300, 0.1, 0.01, 21, 3
SWEEPS = 2
_expected = {}                 # K -> what the C oracle leaves after every sweep (computed once per K, shared by the margins, read only)


def corpus(K):
    from lda_thesis_amd.layout import GroupLayout
    L = GroupLayout(K)
    docs_per_workgroup = 2 * 128 // L.G                      # 128 threads, G / 2 lanes per document
    D = 2 * docs_per_workgroup + 1
    rng = np.random.default_rng(500 + K)
    lens = rng.integers(0, 41, size=D)
    lens[:6] = (0, 1, 2, 40, 0, 33)
    lens[-1] = 7                                             # the document of the last workgroup: its copies have no sites
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    word = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, 6, size=int(off[-1])).astype(np.int32)
    z = rng.integers(0, K, size=int(off[-1])).astype(np.int64)
    wide_words = np.arange(0, V, 5)
    return D, off, word, freq, z, wide_words, rng.integers(0, K, size=len(wide_words))


@pytest.mark.gpu
@pytest.mark.parametrize("margin", [-2, 6, 0])
@pytest.mark.parametrize("K", [512, 256, 128, 100, 400])
def test_document_loop_of_tier1_equals_the_c_oracle(c_oracle, K, margin):
    from lda_thesis_amd.sampler import GibbsSampler
    D, off, word, freq, z, wide_words, wide_topics = corpus(K)
    s = GibbsSampler(off, word, freq, z, K, V, ALPHA, BETA, labs=None, seed=SEED, doc_base=DOC_BASE, commit_log=True, rows16=True, quad=True,
                     sort_docs=False)
    s.add_word_topic_counts(wide_words, wide_topics, np.full(len(wide_words), 70000))
    assert s.quad and s.row16 is not None and s.dense_mask
    if K not in _expected:
        cs = c_oracle.CState(off, word, freq, z, np.ones((D, K), dtype=np.uint8), s.n_d_k(), s.n_k_v(), s.n_zk(), V, ALPHA, BETA)
        states = []
        for i in range(SWEEPS):
            cs.sweep(1, SEED, i, doc_base=DOC_BASE, threads=2)
            states.append(tuple(np.array(a, copy=True) for a in (cs.z, cs.n_d_k, cs.n_k_v, cs.n_zk)))
        for st in states:
            for a in st:
                a.setflags(write=False)
        _expected[K] = states
    s.debug_margin = margin
    for i in range(SWEEPS):
        s.sweep()
        assert int((s.row16 == 0).sum()) >= len(wide_words)                      # the words that are read as int32 rows
        ez, endk, enkv, enzk = _expected[K][i]
        np.testing.assert_array_equal(s.z_topics(), ez, err_msg="z after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_d_k(), endk, err_msg="n_d_k after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_k_v(), enkv, err_msg="n_k_v after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_zk(), enzk, err_msg="n_zk after sweep %d" % (i + 1))
    s.check_status()                                                             # no status bit
    assert s.quad
    st = s.status.cpu().numpy()
    if margin == -2:
        assert int(st[1]) == SWEEPS * int(off[-1])                               # every site left tier 0
    # margin 2^-40: the fp64 decision -- tier 1 here, or the one in front of the exact tier for the sites of the wide rows -- settles all
    # but a handful of sites per 10^10; margin 2^-6: a site in thirty or so goes on to the exact tier
    if margin in (-2, 0):
        assert int(st[2]) <= 2
    else:
        assert int(st[2]) > 0


def planted_in_documents_1_and_3(K, D):
    """quad_neartie_state (test_gpu_parity.py) plants a near tie at the LAST site of every document; here the documents 0 and 2 of every
    wavefront (K = 512: four documents each, in order) lose that site.  The counts stay as they were -- the remaining sites of such a
    document see exactly the state they were placed in, with the dropped site's count as a phantom one -- so the planted sites of the
    documents 1 and 3 are the only ones tier 0 must hand over."""
    from test_gpu_parity import quad_neartie_state
    st = quad_neartie_state(K, D)
    lens = np.diff(st["doc_off"])
    keep = np.ones(int(st["doc_off"][-1]), dtype=bool)
    even = np.arange(D) % 2 == 0
    keep[st["doc_off"][1:][even] - 1] = False
    lens = lens - even
    out = dict(st, doc_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), word=st["word"][keep], freq=st["freq"][keep],
               z=st["z"][keep], n_planted=int((~even).sum()))
    return out, lens


@pytest.mark.gpu
def test_ties_in_documents_1_and_3_of_a_wavefront_only(c_oracle):
    """production margins: the document loop runs for the scalar mask 0b1010 (documents 1 and 3 of equal length: both ties in one
    iteration), 0b0010 and 0b1000, never for a document tier 0 decided; status[1] counts exactly the planted sites"""
    from lda_thesis_amd.sampler import GibbsSampler
    K, D = 512, 128
    st, lens = planted_in_documents_1_and_3(K, D)
    assert st["tuned_gap_max"] < 2.0 ** -27.5 and st["safe_gap_min"] > 2.0 ** -14.5
    both = sum(1 for w in range(D // 4) if lens[4 * w + 1] == lens[4 * w + 3])
    assert 0 < both < D // 4                                                     # wavefronts with both ties in ONE iteration, and without
    counts = dict(n_d_k=st["n_d_k"], n_k_v=st["n_k_v"], n_zk=st["n_zk"])
    s = GibbsSampler(st["doc_off"], st["word"], st["freq"], st["z"], K, st["V"], st["alpha"], st["beta"], counts=counts, seed=4242,
                     doc_base=7, commit_log=True, rows16=True, quad=True, sort_docs=False)
    assert s.quad and s.row16 is not None and s.doc_order is None
    s.sweep()
    s.check_status()
    cs = c_oracle.CState(st["doc_off"], st["word"], st["freq"], st["z"], st["labs"], st["n_d_k"], st["n_k_v"], st["n_zk"], st["V"],
                         st["alpha"], st["beta"])
    cs.sweep(1, 4242, 0, doc_base=7, threads=2)
    np.testing.assert_array_equal(s.z_topics(), cs.z)
    np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k)
    np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v)
    np.testing.assert_array_equal(s.n_zk(), cs.n_zk)
    status = s.status.cpu().numpy()
    assert int(status[1]) == st["n_planted"] == D // 2
