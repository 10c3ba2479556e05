"""How a slot travels through the quad kernels (llda_sweep_quad_kernel, csrc/kernel_quad.hpp).  The production build carries the slot
number rho = 8 i + 2 c + e (key of the draw: quad lane << 14 | rho << 9 | device position) and decodes the old position of a site by a
table; -DLLDA_QUAD_PARTS bit 8 carries the slot as its ENTRY, the LDS byte offsets rho stands for,

    entry(rho) = (rho >> 2) * 2048 + (rho & 3) * 4      offset of QLDS(arr, rho, 0) inside s_ndk / s_pa: bits 2, 3, 11 .. 13
               | rho << 6                                offset of row rho of s_hot:                      bits 6 .. 10

(key: quad lane << 23 | entry << 9 | device position; measured, not faster: profiles/r08_quad_entry_key.md).  The CPU part restates
both encodings in numpy from these formulas and checks, for the three geometries and every position, what the kernel relies on; the GPU
part runs the kernels where the changed paths are taken far more often than on random data, and the argument check that the 32-bit
log offsets need."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QNT = 128                      # threads of a workgroup: the arrays are [rho >> 2][QNT][4] of 4-byte words
MASK_NDK, MASK_HOT = 0x380C, 0x7C0
FORMS = {"rho": (5, lambda rho: np.asarray(rho, dtype=np.int64)), "entry": (14, lambda rho: entry(rho))}     # width of a slot, slot(rho)


def entry(rho):
    rho = np.asarray(rho, dtype=np.int64)
    return ((rho >> 2) * 2048 + (rho & 3) * 4) | (rho << 6)


def quad_rho(pos, LB):
    pos = np.asarray(pos, dtype=np.int64)
    return ((pos >> LB) & 0x18) | ((pos & 3) << 1) | ((pos >> 2) & 1)


def key_none(LB, form):
    bits, slot = FORMS[form]
    return 0x3F << (9 + bits) | int(slot(31)) << 9 | (32 * (1 << LB) - 1)


def draw_key(pos, LB, form):
    """the key quad_draw builds for a position: every search outcome ORs its bit of the position and its bits of the slot"""
    pos = np.asarray(pos, dtype=np.int64)
    IS = 3 + LB
    lq = (pos >> 3) & ((1 << LB) - 1)
    c1, c2 = (pos >> (IS + 1)) & 1, (pos >> IS) & 1                    # slot chunk i = 2 c1 + c2
    c3, c4, c0 = (pos >> 1) & 1, pos & 1, (pos >> 2) & 1               # slot in the chunk c = 2 c3 + c4; chain e = c0
    if form == "entry":
        const = {"c1": (2 << IS) | (8192 | 16 << 6) << 9, "c2": (1 << IS) | (4096 | 8 << 6) << 9, "c3": 2 | (2048 | 4 << 6) << 9,
                 "c4": 1 | (8 | 2 << 6) << 9, "c0": 4 | (4 | 1 << 6) << 9}
    else:
        const = {"c1": (2 << IS) | 16 << 9, "c2": (1 << IS) | 8 << 9, "c3": 2 | 4 << 9, "c4": 1 | 2 << 9, "c0": 4 | 1 << 9}
    return (c1 * const["c1"] | c2 * const["c2"] | c3 * const["c3"] | c4 * const["c4"] | c0 * const["c0"] | lq << 3 | lq << (9 + FORMS[form][0]))


def test_entry_is_injective_and_its_fields_do_not_overlap():
    en = entry(np.arange(32))
    assert len(set(en.tolist())) == 32
    assert MASK_NDK & MASK_HOT == 0
    assert np.all(en & ~(MASK_NDK | MASK_HOT) == 0) and int(np.bitwise_or.reduce(en)) == MASK_NDK | MASK_HOT
    assert int(en.max()) < 1 << 14
    # the entry of an OR of slot bits is the OR of their entries (what lets the search build it bit by bit)
    for rho in range(32):
        bits = [1 << b for b in range(5) if rho >> b & 1]
        assert (int(np.bitwise_or.reduce(entry(bits))) if bits else 0) == int(entry(rho))


def test_the_masks_recover_the_two_offsets():
    rho = np.arange(32)
    en = entry(rho)
    words = np.arange(8 * QNT * 4).reshape(8, QNT, 4)                 # word index inside s_ndk / s_pa
    np.testing.assert_array_equal(en & MASK_NDK, 4 * words[rho >> 2, 0, rho & 3])
    np.testing.assert_array_equal(en & MASK_HOT, rho * 16 * 4)        # row rho of int s_hot[32][16]
    # every thread's own part starts tid * 16 bytes on and stays inside the array
    assert int((en & MASK_NDK).max()) + (QNT - 1) * 16 + 4 <= words.size * 4


@pytest.mark.parametrize("form", ["rho", "entry"])
@pytest.mark.parametrize("LB", [2, 3, 4])
def test_the_key_of_every_position(LB, form):
    KP, LPD = 32 << LB, 1 << LB
    bits, slot = FORMS[form]
    lane_shift = 9 + bits
    pos = np.arange(KP)
    key = draw_key(pos, LB, form)
    np.testing.assert_array_equal(key & 511, pos)
    np.testing.assert_array_equal((key >> 9) & ((1 << bits) - 1), slot(quad_rho(pos, LB)))
    np.testing.assert_array_equal(key >> lane_shift, (pos >> 3) & (LPD - 1))
    assert sorted(quad_rho(pos[((pos >> 3) & (LPD - 1)) == 0], LB).tolist()) == list(range(32))
    # KEY_NONE is the largest key, names the last slot of the last lane, and fits a positive int32
    none = key_none(LB, form)
    assert int(key.max()) < none < 1 << 31
    assert none & 511 == KP - 1 and (none >> 9) & ((1 << bits) - 1) == int(slot(31)) == int(slot(quad_rho(KP - 1, LB)))
    # the minimum over a document orders by lane first
    lane = key >> lane_shift
    for l in range(LPD - 1):
        assert int(key[lane == l].max()) < int(key[lane == l + 1].min())
    # zn = key without the lane field gives the position, the slot and the lane back
    zn = key & ((1 << lane_shift) - 1)
    np.testing.assert_array_equal(zn & 511, pos)
    np.testing.assert_array_equal(zn >> 9, slot(quad_rho(pos, LB)))
    # the table of decode_old (uint16_t s_ent[KP]) holds every slot as it travels
    assert int(slot(quad_rho(pos, LB)).max()) < 1 << 16


def test_the_kernel_source_states_the_same_constants():
    text = open(os.path.join(ROOT, "lda_thesis_amd", "csrc", "kernel_quad.hpp")).read()
    m = re.search(r"QE_NDK = (0x[0-9A-Fa-f]+)u, QE_HOT = (0x[0-9A-Fa-f]+)u", text)
    assert m and int(m.group(1), 16) == MASK_NDK and int(m.group(2), 16) == MASK_HOT
    assert "return ((rho >> 2) * 2048u + (rho & 3u) * 4u) | rho << 6;" in text
    assert re.search(r"QS_BITS = QUAD_ENTRY \? 14 : 5;", text) and "QK_LANE = 9 + QS_BITS" in text
    assert "quad_slot(uint32_t rho) { return QUAD_ENTRY ? quad_entry(rho) : rho; }" in text


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
