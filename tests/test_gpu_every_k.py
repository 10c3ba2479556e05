"""Every K on the device, and the wide layouts of five, six and seven tiers in every form of the wide sweep.

K is the number of labels plus one: any K from 1 to 7688 is a production input, its layout decides which instantiation runs and in what
order the exact tiers add the K scores, and the geometry of K is not monotone.  tests/test_layout_every_k_host.py proves the C table
equal to numpy's recursion and to GroupLayout for every K and the schedule, run from that table, equal to np.sum; here the kernels
that consume the table run on it.

  test_theta_every_k   one llda_readout_theta call (mode 0) per K, K = 1 .. 7688: the narrow llda_readout_theta_kernel<G, T, HAS_TAIL>
                       and wide_sum on every table the library can make.  Three rows of a general mask with the root set, counts below
                       2^8, 2^14 and 2^20, alpha = 0.1 (layoutclasses.every_k_rows), against readoutref.theta_ref as uint64.  Before
                       the device is used the test checks that the rows of every K >= 32 tell numpy's order from a sequential sum.
                       Device rows and lane masks are built from the C tables (GroupLayout costs milliseconds at large K).
  test_wide_sweep_forms_on_five_six_and_seven_tiers
                       llda_sweep_wide_f32_kernel<5|6|7, 4, SLIM>, llda_sweep_wide_reg_kernel<5|6|7, COMPACT> and the run-time-tier
                       llda_sweep_wide_kernel (tiered and all-exact), three sweeps against the C oracle, every integer.  The K come
                       from layoutclasses.tier_ks(); what csrc/sweep_plan.hpp makes of every case is pinned on the host
                       (tests/test_sweep_plan_host.py::test_five_six_and_seven_tiers_take_every_wide_form), the device test asserts
                       what SELECTS the form.

test_theta_every_k on the MI355X: one timing in eight ranges of 961 K took 1.84 s (the first: it loads the library), 0.30, 0.38, 0.45, 0.54,
0.61, 0.68 and 0.75 s -- 5.6 s for all 7 688 calls with their host references, 0.3 .. 0.8 ms a K.  Chosen: FOUR ranges of 1 922 K, which
then took 2.35, 0.84, 1.17 and 1.46 s.  The 36 sweep cases take 0.05 .. 0.13 s each (the first 2.6 s: it builds the C oracle)."""
import numpy as np
import pytest

import layoutclasses as lc
import readoutref as rr
from countref import Guarded

pytestmark = pytest.mark.gpu

N_RANGES = 4
RANGES = [(1 + i * lc.MAX_K // N_RANGES, (i + 1) * lc.MAX_K // N_RANGES) for i in range(N_RANGES)]
PREFILL = 7.0                                    # no theta: an entry is at most 1, or NaN


def test_the_ranges_cover_every_k():
    assert RANGES[0][0] == 1 and RANGES[-1][1] == lc.MAX_K
    assert all(a[1] + 1 == b[0] for a, b in zip(RANGES, RANGES[1:]))


@pytest.mark.parametrize("r", RANGES, ids=["K%d-%d" % r for r in RANGES])
def test_theta_every_k(r):
    import torch
    from lda_thesis_amd import _native as nat
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for K in range(r[0], r[1] + 1):
        t = lc.c_tables(K)
        labs, n = lc.every_k_rows(K)
        want = rr.theta_ref(n, labs, lc.ALPHA)
        # the inputs tell summation orders apart (a K that does not is a failure of the inputs)
        if K >= 32:
            assert (want.view(np.uint64) != lc.sequential_theta(labs, n).view(np.uint64)).any(), K
        n_dk = lc.device_row(t, n, np.int32)
        mask = lc.lane_masks(t, labs)
        assert n_dk.shape == (3, t["KP"]) and mask.shape == (3, t["G"]) and int(n_dk.sum()) == int(n.sum())
        out = Guarded(np.full(3 * K, PREFILL))
        nat.readout_theta(up(n_dk), up(mask.view(np.int16)), 3, K, lc.ALPHA, out.t)
        torch.cuda.synchronize()
        rr.assert_same_bits(out.host("theta K=%d" % K).reshape(3, K), want, "theta K=%d (G=%d T=%d leaves=%d tail=%d wide=%d)"
                            % (K, t["G"], t["T"], t["n_leaves"], t["tail"], t["wide"]))


# ------------------------------------------------------------------------------------------------
# the wide sweeps of five, six and seven tiers
# ------------------------------------------------------------------------------------------------
SEED, DOC_BASE, SWEEPS = 99, 1000, 3
TINY_PRIOR = 1e-9                                # below the tiered kernels' domain: every site through the exact pipeline
HEAVY_FREQ = 40000                               # one site that takes its document beyond 2^15 tokens
# form -> (debug_margin, tiny priors, heavy document): the table of tests/secondtrip.py SWEEP_CASES
FORMS = {
    "f32_fat": (0, False, False),
    "f32_slim_forced": (-7, False, False),
    "f32_fat_forced": (-6, False, False),
    "reg_compact": (-5, False, False),
    "reg_lds_copies": (-4, False, False),
    "lds_only_tiered": (-3, False, False),
    "f32_fat_all_rare": (-1, False, False),
    "lds_only_all_exact": (0, True, False),
    "reg_heavy_document": (0, False, True),
}
LARGEST_FORMS = ("f32_fat", "f32_fat_all_rare", "reg_compact")


def sweep_cases():
    """(tiers, K, form, dense): every form on the smallest K of each tier count, three on the largest; dense and general masks in turn"""
    out = []
    for nt in (5, 6, 7):
        lo, hi = lc.tier_ks()[nt]
        out += [(nt, lo, form) for form in FORMS] + [(nt, hi, form) for form in LARGEST_FORMS]
    return [(nt, K, form, i % 2 == 0) for i, (nt, K, form) in enumerate(out)]


def test_the_sweep_cases_leave_no_gap():
    cases = sweep_cases()
    for nt in (5, 6, 7):
        lo, hi = lc.tier_ks()[nt]
        assert {f for t, K, f, _ in cases if K == lo} == set(FORMS) and {f for t, K, f, _ in cases if K == hi} == set(LARGEST_FORMS)
        assert {d for t, K, f, d in cases if t == nt} == {True, False}
        assert lc.geometry(lo)["tiers"] == lc.geometry(hi)["tiers"] == nt
    assert {dm for dm, _, _ in FORMS.values()} == {0, -1, -3, -4, -5, -6, -7}


def sweep_corpus(K, dense, heavy):
    """D = 16 documents of 1 .. 60 sites over V = 300 words (tests/test_gpu_parity.py synth: a general mask is the root and a
    handful of labels); heavy: the first site of document 3 holds HEAVY_FREQ tokens"""
    from test_gpu_parity import synth
    D, V = 16, 300
    doc_off, word, freq, labs, z = synth(np.random.default_rng([43, K, int(dense)]), D, V, K, 1, 60, dense)
    freq = freq.copy()
    if heavy:
        freq[doc_off[3]] = HEAVY_FREQ
    return D, V, doc_off, word, freq, labs, z


@pytest.mark.parametrize("nt,K,form,dense", sweep_cases(), ids=["%dtiers-K%d-%s-%s" % (c[0], c[1], c[2], "dense" if c[3] else "masked")
                                                                for c in sweep_cases()])
def test_wide_sweep_forms_on_five_six_and_seven_tiers(c_oracle, nt, K, form, dense):
    from lda_thesis_amd.sampler import GibbsSampler
    margin, tiny, heavy = FORMS[form]
    D, V, doc_off, word, freq, labs, z = sweep_corpus(K, dense, heavy)
    alpha, beta = (TINY_PRIOR, TINY_PRIOR) if tiny else (0.1, 0.01)
    S = int(doc_off[-1])
    s = GibbsSampler(doc_off, word, freq, z, K, V, alpha, beta, labs=labs, seed=SEED, doc_base=DOC_BASE, sparse_labels=False)
    # what selects the kernel form (csrc/sweep_plan.hpp)
    g = lc.geometry(K)
    assert s.layout.wide and s.layout.NT == nt == g["tiers"] and s.layout.T == 16 and s.layout.KP == g["KP"] == 1024 * nt
    assert s.live_off is None and s._scratch is not None and s.dense_mask == dense and len(s._calls) == 1
    assert s.max_doc_tokens >= 32768 if heavy else 0 < s.max_doc_tokens < 32768
    s.debug_margin = margin
    n_dk0, n_kv0, n_k0 = s.n_d_k(), s.n_k_v(), s.n_zk()
    cs = c_oracle.CState(doc_off, word, freq, z, labs, n_dk0, n_kv0, n_k0, V, alpha, beta)
    for i in range(SWEEPS):
        s.sweep()
        cs.sweep(1, SEED, i, doc_base=DOC_BASE, threads=4)
        what = "K=%d %s sweep %d" % (K, form, i)
        np.testing.assert_array_equal(s.z_topics(), cs.z, err_msg=what)
        np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k, err_msg=what)
        np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v, err_msg=what)
        np.testing.assert_array_equal(s.n_zk(), cs.n_zk, err_msg=what)
        if margin == -1:                                          # every site through the rare tiers, the exact pipeline included
            assert int(s.status[2]) == (i + 1) * S and int(s.status[1]) == (i + 1) * S
    s.check_status()
    assert not np.array_equal(cs.z, z)                            # (the sweeps moved something)
    assert int(s.n_zk().sum()) == int(freq.astype(np.int64).sum()) and (s.n_d_k()[labs == 0] == 0).all()
