"""How a slot travels through the quad kernels (llda_sweep_quad_kernel, csrc/kernel_quad.hpp): as the slot number rho = 8 i + 2 c + e (key
of the draw: quad lane << 14 | rho << 9 | device position), and the old position of a site is decoded by a table.  (A second encoding,
the slot as the LDS byte offsets rho stands for, was measured, rejected and removed: DESIGN.md 4.1a.)  The CPU part restates the key in
numpy from these formulas and checks, for the three geometries and every position, what the kernel relies on; the GPU part runs the
kernels where the changed paths are taken far more often than on random data, and the argument check that the 32-bit log offsets need."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_BITS = 5                  # width of a slot number in the key
LANE_SHIFT = 9 + SLOT_BITS     # QK_LANE


def quad_rho(pos, LB):
    pos = np.asarray(pos, dtype=np.int64)
    return ((pos >> LB) & 0x18) | ((pos & 3) << 1) | ((pos >> 2) & 1)


def key_none(LB):
    return 0x3F << LANE_SHIFT | 31 << 9 | (32 * (1 << LB) - 1)


def draw_key(pos, LB):
    """the key quad_draw builds for a position: every search outcome ORs its bit of the position and its bit of the slot number"""
    pos = np.asarray(pos, dtype=np.int64)
    IS = 3 + LB
    lq = (pos >> 3) & ((1 << LB) - 1)
    c1, c2 = (pos >> (IS + 1)) & 1, (pos >> IS) & 1                    # slot chunk i = 2 c1 + c2
    c3, c4, c0 = (pos >> 1) & 1, pos & 1, (pos >> 2) & 1               # slot in the chunk c = 2 c3 + c4; chain e = c0
    const = {"c1": (2 << IS) | 16 << 9, "c2": (1 << IS) | 8 << 9, "c3": 2 | 4 << 9, "c4": 1 | 2 << 9, "c0": 4 | 1 << 9}
    return (c1 * const["c1"] | c2 * const["c2"] | c3 * const["c3"] | c4 * const["c4"] | c0 * const["c0"] | lq << 3 | lq << LANE_SHIFT)


@pytest.mark.parametrize("LB", [2, 3, 4], ids=lambda LB: "%d-rho" % LB)          # (the ids these cases have always had)
def test_the_key_of_every_position(LB):
    KP, LPD = 32 << LB, 1 << LB
    pos = np.arange(KP)
    key = draw_key(pos, LB)
    np.testing.assert_array_equal(key & 511, pos)
    np.testing.assert_array_equal((key >> 9) & ((1 << SLOT_BITS) - 1), quad_rho(pos, LB))
    np.testing.assert_array_equal(key >> LANE_SHIFT, (pos >> 3) & (LPD - 1))
    assert sorted(quad_rho(pos[((pos >> 3) & (LPD - 1)) == 0], LB).tolist()) == list(range(32))
    # KEY_NONE is the largest key, names the last slot of the last lane, and fits a positive int32
    none = key_none(LB)
    assert int(key.max()) < none < 1 << 31
    assert none & 511 == KP - 1 and (none >> 9) & ((1 << SLOT_BITS) - 1) == 31 == int(quad_rho(KP - 1, LB))
    # the minimum over a document orders by lane first
    lane = key >> LANE_SHIFT
    for l in range(LPD - 1):
        assert int(key[lane == l].max()) < int(key[lane == l + 1].min())
    # zn = key without the lane field gives the position, the slot and the lane back
    zn = key & ((1 << LANE_SHIFT) - 1)
    np.testing.assert_array_equal(zn & 511, pos)
    np.testing.assert_array_equal(zn >> 9, quad_rho(pos, LB))
    # the table of decode_old (uint16_t s_ent[KP]) holds every slot as it travels
    assert int(quad_rho(pos, LB).max()) < 1 << 16


def test_the_kernel_source_states_the_same_constants():
    text = open(os.path.join(ROOT, "lda_thesis_amd", "csrc", "kernel_quad.hpp")).read()
    m = re.search(r"constexpr int QK_LANE = (\d+);", text)
    assert m and int(m.group(1)) == LANE_SHIFT == 14
    assert "QUAD_KEY_NONE = 0x3Fu << QK_LANE | 31u << 9 | (uint32_t)(QuadGeo<LB>::KP - 1);" in text
    assert "s_ent[i] = (uint16_t)quad_rho<LB>(i);" in text
    assert "return ((pos >> LB) & 0x18) | ((pos & 3) << 1) | ((pos >> 2) & 1);" in text          # quad_rho, as restated above


def one_topic_corpus(rng, D, V, K):
    lens = rng.integers(12, 60, size=D).astype(np.int64)
    lens[:4] = [1, 2, 3, 7]
    doc_off = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(lens, out=doc_off[1:])
    word = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, 4, size=int(doc_off[-1])).astype(np.int32)
    labs = np.ones((D, K), dtype=np.uint8)
    z = np.repeat(rng.integers(0, K, size=D), lens).astype(np.int64)    # every site of a document on ONE topic
    return doc_off, word, freq, labs, z


@pytest.mark.gpu
@pytest.mark.parametrize("K", [512, 256, 128])
def test_documents_that_start_on_one_topic(c_oracle, K):
    """With all of a document on one topic (and a small alpha, which keeps most of it there) the lane that receives a site is, most of the time,
    the lane the next site leaves: the count update's second pass ("one lane owns both"), 1 in 16 / 8 / 4 on random assignments."""
    from lda_thesis_amd.sampler import GibbsSampler
    rng = np.random.default_rng(2000 + K)
    V, alpha, beta, seed = 300, 0.001, 0.01, 5
    doc_off, word, freq, labs, z = one_topic_corpus(rng, 77, V, K)
    s = GibbsSampler(doc_off, word, freq, z, K, V, alpha, beta, labs=labs, seed=seed, commit_log=True, sort_docs=False)
    assert s.quad and s.dense_mask and s.commit_log is not None
    cs = c_oracle.CState(doc_off, word, freq, z, labs, s.n_d_k(), s.n_k_v(), s.n_zk(), V, alpha, beta)
    same_lane = 0
    for i in range(4):
        s.sweep()
        cs.sweep(1, seed, i, threads=2)
        np.testing.assert_array_equal(s.z_topics(), cs.z, err_msg="z after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k, err_msg="n_d_k after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v, err_msg="n_k_v after sweep %d" % (i + 1))
        np.testing.assert_array_equal(s.n_zk(), cs.n_zk, err_msg="n_zk after sweep %d" % (i + 1))
        zt = np.asarray(cs.z)
        same_lane += int(np.sum(zt[1:] == zt[:-1]))
    # the case was exercised: neighbouring sites on one topic, i.e. on one lane (random assignments: 4 S / K pairs over the four sweeps)
    assert same_lane > doc_off[-1] // 2
    s.check_status()


@pytest.mark.gpu
def test_quad_call_spanning_two_to_the_thirty_sites_is_refused(monkeypatch):
    """The quad kernel addresses the commit log as base + (position << 2) in 32 bits: llda_sweep refuses, in front of the launch, a call
    whose n_sites does not keep every position below 2^30.  The call is the sampler's own quad call with n_sites replaced."""
    from lda_thesis_amd import _native
    from lda_thesis_amd.sampler import GibbsSampler
    rng = np.random.default_rng(7)
    K, V = 512, 300
    doc_off, word, freq, labs, z = one_topic_corpus(rng, 9, V, K)
    s = GibbsSampler(doc_off, word, freq, z, K, V, 0.1, 0.01, labs=labs, seed=3, commit_log=True)
    assert s.quad
    real, seen = _native.sweep, []

    def huge(**kw):
        assert kw["row16"] is not None and kw["commit_log"] is not None          # (the quad path)
        seen.append(kw["n_sites"])
        kw["n_sites"] = 2 ** 30
        return real(**kw)

    monkeypatch.setattr(_native, "sweep", huge)
    z_before = s.z_topics().copy()
    with pytest.raises(_native.NativeError, match=r"bad argument \(code -2"):
        s.sweep()
    assert seen == [int(doc_off[-1])]
    np.testing.assert_array_equal(s.z_topics(), z_before)           # nothing ran
