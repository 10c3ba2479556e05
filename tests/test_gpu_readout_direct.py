"""The read-out kernels called directly through lda_thesis_amd._native (readout_theta, readout_phi, loglik) and held against
tests/readoutref.py, the numpy restatement that tests/test_readout_host.py ties to the reference's own outputs.

theta and phi are the same IEEE operations in the same order as numpy's, so they are compared BIT FOR BIT (as uint64 where the
value is no NaN: -0.0 is not 0.0; NaN at the same places) -- there is no tolerance.  Every buffer a kernel writes sits between two
margins of 64 sentinel elements (countref.Guarded) which must come back untouched, and is pre-filled with a value the kernel
cannot produce (7.0: theta and phi of counts are at most 1, or inf / NaN).  The K list walks the geometry: fewer than 8 topics
and K = 1, one leaf with and without a tail, 8 / 16 / 32 / 64 lanes per document, padded layouts, KP = 16, and four wide layouts
(the smallest, one with a 7-topic tail, 12 slots per lane, the largest).  n_dk keeps ZERO padding (theta and llda_loglik add the
padding into the row sum); n_kw, n_k and den carry poison in the padding, which llda_readout_phi must never look at."""
import numpy as np
import pytest

import layoutclasses
import readoutref as rr
from countref import Guarded

pytestmark = pytest.mark.gpu

NARROW_KS = [1, 5, 8, 12, 40, 130, 392, 512, 1000]
WIDE_KS = [969, 1031, 5000, 7688]
KS = NARROW_KS + WIDE_KS
# what the list relies on: K -> (lanes per document G, slots per lane T, topics of the last leaf's tail, wide)
GEOMETRY = {1: (8, 1, 1, False), 5: (8, 1, 5, False), 8: (8, 1, 0, False), 12: (8, 2, 4, False), 40: (8, 8, 0, False),
            130: (16, 12, 2, False), 392: (32, 16, 0, False), 512: (32, 16, 0, False), 1000: (64, 16, 0, False),
            969: (128, 16, 1, True), 1031: (128, 16, 7, True), 5000: (512, 12, 0, True), 7688: (512, 16, 0, True)}
ALPHAS = [0.37, 0.0, 1e-12, 50.3]
PREFILL = 7.0
POISON_I32 = 0x7fffffff


def geometry(K):
    lay = rr.layout(K)
    assert (lay.G, lay.T, lay.tail, bool(lay.wide)) == GEOMETRY[K], K
    return lay


def test_the_k_list_covers_the_geometry():
    lays = {K: geometry(K) for K in KS}
    assert {lays[K].G for K in NARROW_KS} == {8, 16, 32, 64}
    assert lays[12].KP == 16 and lays[1].KP == 8 and lays[5].m == 1 and lays[40].m == 1
    assert all(lays[K].KP > K for K in (1, 5, 12, 40, 130, 392, 1000)) and all(lays[K].KP == K for K in (8, 512))
    assert not rr.layout(968).wide and min(K for K in range(900, 1100) if rr.layout(K).wide) == 969       # the smallest wide layout
    assert [lays[K].NT for K in WIDE_KS] == [2, 2, 8, 8] and 7688 == rr.layout(7688).K and lays[7688].KP == 8192


def _dev(a):
    """device copy of the 1-D array ``a`` (uint16 as int16, the same bits)"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# llda_readout_theta
# ------------------------------------------------------------------------------------------------
def run_theta(lay, n_d_k, labs, alpha, old=None, keep=None, share=None):
    """-> out (D, K) of llda_readout_theta on the device rows of the counts (zero padding) and the lane masks of the labels"""
    from lda_thesis_amd import _native as nat
    D, K = labs.shape
    n_dk = rr.device_dk(lay, n_d_k)
    mask = lay.lane_masks(labs)
    assert mask.shape == (D, lay.G) and (lay.labs_from_masks(mask) == labs).all()
    out = Guarded(np.full(D * K, PREFILL) if old is None else old)
    nat.readout_theta(_dev(n_dk), _dev(mask), D, K, alpha, out.t, keep, share)
    _sync()
    return out.host("theta").reshape(D, K)


def theta_inputs(K, D, masks, seed=3):
    rng = np.random.default_rng([seed, K, D, rr.MASKS.index(masks)])
    labs = rr.label_rows(rng, D, K, masks)
    return labs, rr.theta_counts(rng, labs, masks)


def odd_d(lay):
    """a D that is no multiple of the documents per workgroup and has two label-free documents of each kind in ``mixed``"""
    return 11 if lay.wide else 2 * (256 // lay.G) + 5


@pytest.mark.parametrize("masks", rr.MASKS)
@pytest.mark.parametrize("K", KS)
def test_theta_bit_for_bit_masks_and_alphas(K, masks):
    """every mask kind at alpha = 0.37, 0 (a label-free or count-free row is 0/0 = NaN, as numpy gives), 1e-12 and 50.3 (where the
    order of the pairwise row sum decides the last bit); one document with counts near 2^31 - 1, one with a single count"""
    lay = geometry(K)
    D = odd_d(lay)
    labs, n = theta_inputs(K, D, masks)
    assert n.max() > rr.INT32_MAX - 3 and (n[D - 1] != 0).sum() == 1
    if masks == "mixed":
        free = np.flatnonzero(labs.sum(axis=1) == 0)
        assert len(free) >= 2 and (n[free].sum(axis=1) == 0).any() and (n[free].sum(axis=1) > 0).any()
    if masks in ("root_and_3", "single") and K > 8:
        assert (labs.sum(axis=1) < K).all()                          # partial masks
    for alpha in ALPHAS:
        want = rr.theta_ref(n, labs, alpha)
        if masks == "mixed":
            assert np.isnan(want).all(axis=1).any()
        rr.assert_same_bits(run_theta(lay, n, labs, alpha), want, "theta K=%d %s alpha=%g" % (K, masks, alpha))


@pytest.mark.parametrize("K", KS)
def test_theta_document_counts_around_the_workgroup_seam(K):
    """D = 1 and, for the narrow kernels (256 / G documents per workgroup), one less than, exactly and one more than a workgroup"""
    lay = geometry(K)
    gpb = 256 // lay.G if not lay.wide else 2
    for D in sorted({1, gpb - 1, gpb, gpb + 1} - {0}):
        labs, n = theta_inputs(K, D, "mixed", seed=4)
        rr.assert_same_bits(run_theta(lay, n, labs, 0.37), rr.theta_ref(n, labs, 0.37), "theta K=%d D=%d" % (K, D))


def test_theta_wide_second_trip_of_the_grid_stride_loop():
    """more documents than the 4096 workgroups of a wide launch: workgroup b walks document b and then b + 4096, whose masks and
    counts differ, through the same LDS row"""
    K = min(WIDE_KS)
    lay = geometry(K)
    D = rr.WIDE_GRID + 7
    labs, n = theta_inputs(K, D, "mixed", seed=5)
    for d in range(D - rr.WIDE_GRID):
        assert (labs[d] != labs[d + rr.WIDE_GRID]).any() and (n[d] != n[d + rr.WIDE_GRID]).any()
    assert D * lay.KP * 4 < 40e6
    rr.assert_same_bits(run_theta(lay, n, labs, 0.37), rr.theta_ref(n, labs, 0.37), "theta K=%d D=%d" % (K, D))


def plant_fma_document(lay, labs, n, old, d):
    """document d: no label, counts 1 and 2 -> cur = 1/3 and 2/3 whatever alpha; old of the first = the FMA-revealing value"""
    K = labs.shape[1]
    a, b = K // 3, K - 1
    labs[d] = 0
    n[d] = 0
    n[d, a], n[d, b] = 1, 2
    old[d, a] = rr.FMA_TRIPLE[1]
    return a


@pytest.mark.parametrize("K", [130, 512, 969])
def test_theta_running_mean_is_two_products_and_a_sum(K):
    """mode 1 on a narrow layout with a tail, one without and a wide one: old holds random doubles, NaN, +-inf, -0.0 and a
    denormal; keep / share of 1/2, 6/7 and 1/7, and the zeros and ones that turn 0 * inf into NaN; one entry where a fused
    multiply-add of either product gives another last bit (tests/test_readout_host.py proves that of the triple)"""
    lay = geometry(K)
    assert (lay.tail != 0, bool(lay.wide)) == {130: (True, False), 512: (False, False), 969: (True, True)}[K]
    D = odd_d(lay)
    labs, n = theta_inputs(K, D, "mixed", seed=6)
    rng = np.random.default_rng([6, K])
    old = rr.poisoned_old(rng, (D, K))
    assert np.isnan(old).any() and np.isinf(old).sum() == 2 and np.signbit(old[old == 0]).all() and (old == 5e-324).any()
    a = plant_fma_document(lay, labs, n, old, 5)
    cur = rr.theta_ref(n, labs, 0.37)
    assert cur[5, a] == rr.FMA_TRIPLE[3]
    for keep, share in rr.COEFFS:
        want = rr.running_mean_ref(old, cur, keep, share)
        got = run_theta(lay, n, labs, 0.37, old.copy(), keep, share)
        rr.assert_same_bits(got, want, "theta mean K=%d keep=%g share=%g" % (K, keep, share))
        if (keep, share) == rr.FMA_TRIPLE[::2]:
            assert got[5, a] != rr.fma_exact(keep, old[5, a], share * cur[5, a])
            assert got[5, a] != rr.fma_exact(share, cur[5, a], keep * old[5, a])


@pytest.mark.parametrize("K", [130, 969])
def test_theta_on_a_side_stream(K):
    import torch
    lay = geometry(K)
    labs, n = theta_inputs(K, odd_d(lay), "root_and_3", seed=7)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = run_theta(lay, n, labs, 0.37)
    rr.assert_same_bits(got, rr.theta_ref(n, labs, 0.37), "theta on a side stream")


# ------------------------------------------------------------------------------------------------
# llda_readout_phi
# ------------------------------------------------------------------------------------------------
VS = [1, 63, 64, 65, 129]
KV = [(K, V) for K in KS for V in VS if K < 7688 or V <= 65]


def run_phi(lay, n_k_v, V, beta, n_zk=None, den=None, old=None, keep=None, share=None, flags=0):
    """-> (out (K, V), flags or None) of llda_readout_phi.  The padding of n_kw and n_k holds 0x7fffffff and den's NaN: the kernel
    skips a padding position before it reads anything of it.  flags: the word's start value, None: a NULL pointer."""
    from lda_thesis_amd import _native as nat
    K = lay.K
    n_kw = rr.device_kw(lay, n_k_v, pad=POISON_I32)
    assert n_kw.shape == (V, lay.KP)
    n_k = None if n_zk is None else _dev(rr.device_vec(lay, n_zk, pad=POISON_I32))
    dn = None if den is None else _dev(rr.device_vec(lay, den, pad=np.nan, dtype=np.float64))
    out = Guarded(np.full(K * V, PREFILL) if old is None else old)
    fl = None if flags is None else Guarded(np.array([flags], dtype=np.int32))
    nat.readout_phi(_dev(n_kw), n_k, dn, V, K, beta, out.t, None if fl is None else fl.t, keep, share)
    _sync()
    return out.host("phi").reshape(K, V), None if fl is None else int(fl.host("flags")[0])


def phi_counts(K, V, seed=11, low=0):
    rng = np.random.default_rng([seed, K, V])
    n = rng.integers(low, 6, (K, V)).astype(np.int64)
    if low == 0:
        n[rng.random((K, V)) < 0.5] = 0
    return rng, n


@pytest.mark.parametrize("K,V", KV)
def test_phi_bit_for_bit_with_poisoned_padding(K, V):
    """den == NULL: get_phi.  V = 1, one short of, exactly and one past a 64-word tile, two tiles and a word"""
    lay = geometry(K)
    rng, n = phi_counts(K, V)
    n_zk = n.sum(axis=1) + rng.integers(0, 3, K)
    want = rr.phi_ref(n, n_zk, V, 0.013)
    assert rr.flags_ref(want) == 0
    got, flags = run_phi(lay, n, V, 0.013, n_zk=n_zk)
    rr.assert_same_bits(got, want, "phi K=%d V=%d" % (K, V))
    assert flags == 0


@pytest.mark.parametrize("K,V", KV)
def test_get_ph_bit_for_bit_with_zero_denominators(K, V):
    """den != NULL, beta = 0: SubLDA.get_ph.  One den[k] = 0 under a zero row (NaN), one under a non-zero row (inf); NaN in the
    padding of den"""
    lay = geometry(K)
    rng, n = phi_counts(K, V, seed=12)
    n[:, 0] += 1                                                     # (no empty row but the one made below)
    den = n.sum(axis=1).astype(np.float64) + 0.5 * rng.integers(0, 2, K)
    k_nan = K // 2
    n[k_nan], den[k_nan] = 0, 0.0
    if K > 1:
        k_inf = K - 1 if k_nan != K - 1 else 0
        den[k_inf] = 0.0
    want = rr.ph_rows_ref(n, den)
    assert np.isnan(want[k_nan]).all() and (K == 1 or np.isinf(want[k_inf]).any())
    got, flags = run_phi(lay, n, V, 0.0, den=den)
    rr.assert_same_bits(got, want, "get_ph K=%d V=%d" % (K, V))
    assert flags == rr.flags_ref(want) and flags & rr.NAN


GUARD_KS = [5, 12, 130, 512, 1000, 7688]


def guard_places(lay, V):
    """(topic, word): the first of both; the last of both; a topic in the last 64-column block of the row with the last word"""
    k_hi = int(np.argmax(lay.topic_pos))
    assert lay.topic_pos[k_hi] >= (lay.KP - 1) // 64 * 64
    return [(0, 0), (lay.K - 1, V - 1), (k_hi, V - 1)]


@pytest.mark.parametrize("bit", ["negative", "nan", "no_load"])
@pytest.mark.parametrize("K", GUARD_KS)
def test_phi_guards_one_bit_at_a_time(K, bit):
    """mode 0, every count at least 1 but the planted ones.  negative: one count of -3 (den == NULL); nan: den[k] = 0 and one zero
    count in a row of positive ones (0/0 beside x/0 = inf); no_load: beta = 0 and one word with no count at all.  V = 70: the last
    word is the last of a partial tile, and the 58 lanes past it must stay silent."""
    lay = geometry(K)
    V = 70
    for k, v in guard_places(lay, V):
        _, n = phi_counts(K, V, seed=13, low=1)
        den = n.sum(axis=1).astype(np.float64)
        if bit == "negative":
            n[k, v] = -3
            want = rr.phi_ref(n, den.astype(np.int64), V, 0.013)
            got, flags = run_phi(lay, n, V, 0.013, n_zk=den.astype(np.int64))
            assert (want < 0).sum() == 1
        elif bit == "nan":
            n[k, v], den[k] = 0, 0.0
            want = rr.ph_rows_ref(n, den)
            got, flags = run_phi(lay, n, V, 0.0, den=den)
            assert np.isnan(want).sum() == 1
        else:
            n[:, v] = 0
            want = rr.ph_rows_ref(n, den)
            got, flags = run_phi(lay, n, V, 0.0, den=den)
        rr.assert_same_bits(got, want, "phi guard K=%d %s at (%d, %d)" % (K, bit, k, v))
        assert rr.flags_ref(want) == {"negative": rr.NEGATIVE, "nan": rr.NAN, "no_load": rr.NO_LOAD}[bit]
        assert flags == rr.flags_ref(want), (K, bit, k, v, flags)


@pytest.mark.parametrize("V", [1, 63, 65, 129])
@pytest.mark.parametrize("K", [5, 130, 969])
def test_phi_no_load_sees_the_words_and_only_the_words(K, V):
    """mode 0 through den with beta = 0: an all-zero column at the last word raises LLDA_READOUT_NO_LOAD, no such column gives
    0 -- the lanes past V (which see no value either) do not raise it"""
    lay = geometry(K)
    _, n = phi_counts(K, V, seed=14)
    n[0, :] += 1                                                     # every word has a load
    den = n.sum(axis=1).astype(np.float64) + 1.0
    got, flags = run_phi(lay, n, V, 0.0, den=den)
    rr.assert_same_bits(got, rr.ph_rows_ref(n, den), "get_ph")
    assert flags == 0
    n[:, V - 1] = 0
    want = rr.ph_rows_ref(n, den)
    got, flags = run_phi(lay, n, V, 0.0, den=den)
    rr.assert_same_bits(got, want, "get_ph with an empty word")
    assert flags == rr.NO_LOAD == rr.flags_ref(want)


@pytest.mark.parametrize("K", [12, 130, 1031])
def test_phi_flags_are_ored_optional_and_all_three_at_once(K):
    """all three guards in one call: in mode 0 a NaN needs a zero or NaN denominator, which leaves no zero in its row, so the three
    meet in mode 1 -- a NaN and a negative entry in old, and a word whose old and current columns are both zero.  The flag word
    is OR-ed into (a start value of 8 comes back as 8 | bits) and may be NULL."""
    lay = geometry(K)
    V = 70
    rng, n = phi_counts(K, V, seed=15, low=1)
    den = n.sum(axis=1).astype(np.float64)
    n[:, V - 1] = 0
    old = rng.random((K, V))
    old[:, V - 1] = 0.0
    old[K - 1, 3] = -2.0
    old[0, V - 2] = np.nan
    want = rr.running_mean_ref(old, rr.ph_rows_ref(n, den), 0.5, 0.5)
    assert rr.flags_ref(want) == rr.NEGATIVE | rr.NAN | rr.NO_LOAD == 7
    got, flags = run_phi(lay, n, V, 0.0, den=den, old=old.copy(), keep=0.5, share=0.5)
    rr.assert_same_bits(got, want, "phi mean with all three guards")
    assert flags == 7
    got8, flags8 = run_phi(lay, n, V, 0.0, den=den, old=old.copy(), keep=0.5, share=0.5, flags=8)
    rr.assert_same_bits(got8, want, "flags pre-set")
    assert flags8 == 8 | 7
    # mode 0, one bit raised: OR-ed into a word that holds another bit and a foreign one; nothing is cleared
    want0 = rr.ph_rows_ref(n, den)
    assert rr.flags_ref(want0) == rr.NO_LOAD
    got0, flags0 = run_phi(lay, n, V, 0.0, den=den, flags=8 | rr.NEGATIVE)
    rr.assert_same_bits(got0, want0, "flags pre-set, mode 0")
    assert flags0 == 8 | rr.NEGATIVE | rr.NO_LOAD
    got_null, none = run_phi(lay, n, V, 0.0, den=den, old=old.copy(), keep=0.5, share=0.5, flags=None)
    assert none is None
    rr.assert_same_bits(got_null, want, "flags == NULL")


@pytest.mark.parametrize("K", [130, 512, 969])
def test_phi_running_mean_and_its_guards(K):
    """mode 1 with the poisons and coefficients of the theta test; the guards are those of the finished out"""
    lay = geometry(K)
    V = 70
    rng, n = phi_counts(K, V, seed=16)
    den = n.sum(axis=1).astype(np.float64) + 1.5
    k0, v0 = K // 3, V - 1
    n[k0, v0], den[k0] = 1, 3.0
    cur = rr.ph_rows_ref(n, den)
    old = rr.poisoned_old(rng, (K, V))
    old[k0, v0] = rr.FMA_TRIPLE[1]
    assert cur[k0, v0] == rr.FMA_TRIPLE[3]
    seen = set()
    for keep, share in rr.COEFFS:
        want = rr.running_mean_ref(old, cur, keep, share)
        got, flags = run_phi(lay, n, V, 0.0, den=den, old=old.copy(), keep=keep, share=share)
        rr.assert_same_bits(got, want, "phi mean K=%d keep=%g share=%g" % (K, keep, share))
        assert flags == rr.flags_ref(want), (K, keep, share, flags)
        seen.add(flags)
        if (keep, share) == rr.FMA_TRIPLE[::2]:
            assert got[k0, v0] != rr.fma_exact(keep, old[k0, v0], share * cur[k0, v0])
    assert rr.NEGATIVE | rr.NAN in seen                              # (-inf and NaN in old)
    # all-zero coefficients on a clean old: every column is zero
    clean = rng.random((K, V))
    got, flags = run_phi(lay, n, V, 0.0, den=den, old=clean.copy(), keep=0.0, share=0.0)
    assert (got == 0).all() and flags == rr.NO_LOAD


def test_phi_on_a_side_stream():
    import torch
    K, V = 130, 65
    lay = geometry(K)
    rng, n = phi_counts(K, V, seed=17)
    n_zk = n.sum(axis=1)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, flags = run_phi(lay, n, V, 0.013, n_zk=n_zk)
    rr.assert_same_bits(got, rr.phi_ref(n, n_zk, V, 0.013), "phi on a side stream")
    assert flags == 0


# ------------------------------------------------------------------------------------------------
# llda_loglik, wide layouts, per document
# ------------------------------------------------------------------------------------------------
U = 2.0 ** -53
LOGLIK_WIDE_KS = [969, 5000, 7688] + layoutclasses.new_tier_ks("largest")   # ... and five, six and seven FULL tiers with a 7-topic tail
GEOMETRY.update({K: (64 * nt, 16, 7, True) for nt, K in zip((5, 6, 7), layoutclasses.new_tier_ks("largest"))})


def check_loglik_per_document(K, masks, **case):
    import torch
    from helpers import OracleBackend
    from lda_thesis_amd import _native as nat
    lay, D, V, lens, doc_off, word, labs, (n_dk, n_kw, n_k) = rr.loglik_case(K, masks, wide=True, **case)
    alpha, beta = 0.37, 0.013
    lab_mask = lay.lane_masks(labs)
    ref = torch.zeros(D, dtype=torch.float64)
    cpu = torch.from_numpy
    OracleBackend(None).loglik(cpu(doc_off), cpu(word), cpu(lab_mask.view(np.int16)), cpu(n_dk), cpu(n_kw), cpu(n_k), D, V, K,
                               alpha, beta, ref)
    ref = ref.numpy()
    out = Guarded(np.full(D, PREFILL))
    nat.loglik(_dev(doc_off), _dev(word), _dev(lab_mask), _dev(n_dk), _dev(n_kw), _dev(n_k), D, V, K, alpha, beta, out.t)
    _sync()
    got = out.host("out_doc")
    assert (got[lens == 0] == 0.0).all() and (lens == 0).any() and (got[lens > 0] > 0).all()
    bound = 1.01 * U * (lens * (2 * lay.KP + 5) + 2 * np.abs(ref) + lens * np.abs(ref))
    assert (np.abs(got - ref) <= 2 * bound).all(), (K, masks, np.abs(got - ref).max())
    if np.finfo(np.longdouble).nmant >= 63:
        exact = rr.loglik_high_precision(lay, doc_off, word, labs, n_dk, n_kw, n_k, V, alpha, beta)
        err_dev, err_ref = np.abs(got - exact).astype(np.float64), np.abs(ref - exact).astype(np.float64)
        live = lens > 0
        print("loglik wide K=%d %s D=%d: max |dev - exact| / bound = %.4f, max |ref - exact| / bound = %.4f, max |dev - exact| = %.3g"
              % (K, masks, D, (err_dev[live] / bound[live]).max(), (err_ref[live] / bound[live]).max(), err_dev.max()))
        assert (err_dev <= bound).all(), (K, masks, (err_dev[live] / bound[live]).max())
        assert (err_ref <= bound).all()
    return lens, labs, n_dk


@pytest.mark.parametrize("masks", ["all", "root_and_3", "single"])
@pytest.mark.parametrize("K", LOGLIK_WIDE_KS)
def test_loglik_per_document_on_the_wide_layouts(K, masks):
    """out_doc document by document for llda_loglik_wide_kernel, as test_loglik_per_document_on_the_tuned_layouts
    (tests/test_gpu_count_kernels.py) checks the narrow kernel: the same corpus shape, the same two references, the same bound
    (n (2 KP + 5) + 2 S + n S) u with 1 % on top.

    The bound carries over because the wide kernel rounds no more often than the narrow one.  Per term of a site's dot product:
    theta's numerator n_dk + alpha is 1 rounding; its denominator rs is a sum of KP non-negative terms (the padding adds exact
    zeros), each of which passes through at most KP - 1 additions in ANY order -- a per-lane chain of KP / 64 terms and six
    butterfly steps here -- so its relative error stays below (KP - 1) u; th / rs, formed at the point of use, is the 1 rounding the
    narrow kernel spends when it divides ahead of the loop: theta carries 2 roundings and the denominator's error, as there.  phi is
    the same three operations and V * beta (x + beta, n_k + vbeta, the quotient: the +5 leaves room for the rounding of V * beta),
    the product 1, and the sum of the KP products over 64 lanes is again below (KP - 1) u whatever its order.  That is
    (2 KP + 4) u per dot at the most, within the (2 KP + 5) u of the formula; log, and the accumulator's n additions, are the same
    code.  The test prints the ratio of every case (pytest -s); profiles/readout_loglik_bound.md keeps the largest seen."""
    geometry(K)
    lens, _, _ = check_loglik_per_document(K, masks)
    assert (lens == 0).sum() == 10 and lens.max() == 90


def test_loglik_wide_second_trip_of_the_grid_stride_loop():
    """more documents than the 4096 workgroups of a wide launch, 0 to 3 sites each: document d + 4096 goes through the LDS rows
    that held the theta of document d, with other masks and counts"""
    K = min(LOGLIK_WIDE_KS)
    lay = geometry(K)
    D = rr.WIDE_GRID + 9
    lens = np.random.default_rng(21).integers(0, 4, D)
    lens[-9:] = [3, 0, 1, 2, 3, 3, 0, 2, 1]
    lens[:9] = [2, 3, 3, 1, 0, 0, 3, 1, 2]
    assert D * lay.KP * 4 < 40e6
    lens, labs, n_dk = check_loglik_per_document(K, "root_and_3", D=D, lens=lens)
    live = [d for d in range(D - rr.WIDE_GRID) if lens[d] and lens[d + rr.WIDE_GRID]]
    assert len(live) >= 4
    for d in live:
        assert (labs[d] != labs[d + rr.WIDE_GRID]).any() and (n_dk[d] != n_dk[d + rr.WIDE_GRID]).any()
