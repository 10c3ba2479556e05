"""The quad kernels (llda_sweep_quad_kernel, csrc/kernel_quad.hpp) on wavefronts that MIX document lengths.

The site loop has two forms: the FULL one runs while every document of the wavefront still has the sites n .. n + 3, three sites at a
time, and hands over to the masked one, which runs to the longest document.  The corpus below puts documents of 0, 1, 2, ... 15 and
297 ... 300 sites next to each other, so that the shortest document of a wavefront -- where the hand-over happens -- takes every
residue modulo three, wavefronts hand over at once (a shortest document below six sites, an empty document, a lane group without a
document) or never leave the FULL form before the last three sites (equal lengths), and the number of documents is no multiple of the
eight / sixteen / thirty-two of a workgroup.  Bit-exact against the C oracle after each of three sweeps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# groups of four = the wavefronts of K = 512 / 400 in corpus order (sort_docs=False); K = 256 and 128 take eight and sixteen in a row
LENS = [1, 2, 3, 4,   5, 7, 299, 300,        # (one workgroup of K = 512: hand-over at once / at site 0 with a 300-site tail)
        0, 20, 21, 22,   6, 6, 6, 9,         # an empty document; shortest 6: one FULL trio
        7, 8, 30, 7,   8, 9, 10, 11,         # shortest 7, 8
        9, 9, 9, 9,   10, 40, 10, 10,        # equal lengths; shortest 10
        11, 300, 12, 13,   299, 300, 298, 297,
        300, 300, 300, 300,   12, 13, 14, 15,
        13, 13, 14, 300,   14, 15, 15, 15,
        15, 299, 16, 17,   16, 16, 33, 18,
        17, 18, 19, 20,   298, 298, 298, 18,
        19, 19, 19, 19,   20, 21, 22, 23,
        21, 64, 65, 66,   22, 97, 98, 99,
        23, 24, 25, 26,   24, 24, 24, 24,
        25, 25, 300, 25,   26, 27, 28, 29,
        27, 28, 29, 30,   28, 28, 28, 28,
        300, 299, 1, 0,   29, 30, 31, 32,
        5, 5, 5]                             # 123 documents: the last workgroup of every geometry has lane groups without a document


def corpus(rng, lens, V, K, fmax=3):
    lens = np.asarray(lens, dtype=np.int64)
    D = len(lens)
    doc_off = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(lens, out=doc_off[1:])
    word = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, fmax + 1, size=int(doc_off[-1])).astype(np.int32)
    labs = np.ones((D, K), dtype=np.uint8)
    z = rng.integers(0, K, size=int(doc_off[-1])).astype(np.int64)
    return doc_off, word, freq, labs, z


@pytest.mark.parametrize("sort_docs", [False, True])
@pytest.mark.parametrize("K", [512, 256, 128, 400])
def test_quad_kernels_on_mixed_document_lengths(c_oracle, K, sort_docs):
    from lda_thesis_amd.sampler import GibbsSampler
    assert len(LENS) % 8 != 0 and 0 in LENS
    rng = np.random.default_rng(1000 + K)
    V, alpha, beta, seed = 400, 0.1, 0.01, 11
    doc_off, word, freq, labs, z = corpus(rng, LENS, V, K)
    s = GibbsSampler(doc_off, word, freq, z, K, V, alpha, beta, labs=labs, seed=seed, commit_log=True, sort_docs=sort_docs)
    assert s.quad and s.dense_mask and s.n_kw16 is not None and s.commit_log is not None
    cs = c_oracle.CState(doc_off, word, freq, z, labs, s.n_d_k(), s.n_k_v(), s.n_zk(), V, alpha, beta)
    for i in range(3):
        s.sweep()
        cs.sweep(1, seed, i, threads=2)
        np.testing.assert_array_equal(s.z_topics(), cs.z, err_msg="z after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k, err_msg="n_d_k after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v, err_msg="n_k_v after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_zk(), cs.n_zk, err_msg="n_zk after sweep %d" % (i + 1))
    s.check_status()
