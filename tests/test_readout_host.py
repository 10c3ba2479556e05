"""tests/readoutref.py against the reference's own outputs (the golden vectors), its edge cases, and the return codes of
llda_readout_phi / llda_readout_theta -- all without a device.  tests/test_gpu_readout_direct.py holds the kernels against
readoutref bit for bit; this file is what makes that comparison one against the reference project's arithmetic."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import readoutref as rr
from conftest import golden_names, load_golden

TINY = golden_names("tiny_")


def final_counts(g):
    key = "o3_s%d_" % int(g["sweeps"])
    return g[key + "n_d_k"], g[key + "n_k_v"], g[key + "n_zk"]


@pytest.mark.parametrize("name", TINY)
def test_readoutref_reproduces_the_golden_phi_and_theta(name):
    g = load_golden(name)
    n_d_k, n_k_v, n_zk = final_counts(g)
    np.testing.assert_array_equal(rr.phi_ref(n_k_v, n_zk, int(g["V"]), float(g["beta"])), g["o3_phi"])
    theta, num, rs = rr.theta_ref(n_d_k, g["labs"], float(g["alpha"]), with_sums=True)
    np.testing.assert_array_equal(theta, g["o3_theta"])
    np.testing.assert_array_equal(rs, num.sum(axis=1))               # the row-by-row np.sum IS num.sum(axis=1) of the reference
    assert rr.flags_ref(g["o3_phi"]) == 0


def test_ph_rows_ref_has_numpys_nan_and_inf():
    n_k_v = np.array([[0, 0, 0], [2, 0, 6], [1, 3, 0], [0, 0, 0]])
    with np.errstate(divide="ignore", invalid="ignore"):
        want = n_k_v / n_k_v.sum(axis=1, keepdims=True)              # CascadeLDA.py:394-395 as it stands
    got = rr.ph_rows_ref(n_k_v, n_k_v.sum(axis=1))
    rr.assert_same_bits(got, want, "get_ph")
    assert np.isnan(got[0]).all() and got[1, 2] == 0.75
    out = rr.ph_rows_ref(n_k_v, [0.0, 0.0, 4.0, 1.0])
    assert np.isnan(out[0]).all() and np.isnan(out[1, 1]) and out[1, 0] == np.inf and out[2, 1] == 0.75
    assert rr.flags_ref(out) == rr.NAN                              # (column 1: NaN does not compare equal to 0)


def test_theta_ref_edges():
    labs = np.array([[1, 0, 1], [0, 0, 0], [0, 0, 0], [0, 1, 0]])
    n = np.array([[1, 0, 0], [0, 0, 0], [1, 2, 0], [0, 0, 0]])
    th = rr.theta_ref(n, labs, 0.5)
    np.testing.assert_array_equal(th[0], [0.75, 0.0, 0.25])
    assert np.isnan(th[1]).all()                                     # no label, no count: 0/0
    np.testing.assert_array_equal(th[2], [1 / 3.0, 2 / 3.0, 0.0])    # counts outside the labels still count
    np.testing.assert_array_equal(th[3], [0.0, 1.0, 0.0])
    th0 = rr.theta_ref(n, labs, 0.0)
    assert np.isnan(th0[3]).all() and (th0[0] == [1.0, 0.0, 0.0]).all()
    assert rr.FMA_TRIPLE[3] == th[2, 0]                              # the cur of the FMA triple is reachable from counts


def test_flags_ref_each_bit_alone_and_together():
    ok = np.array([[0.25, 0.0], [0.0, 1e-300]])
    assert rr.flags_ref(ok) == 0
    assert rr.flags_ref(np.array([[0.25, -1e-300], [0.5, 0.5]])) == rr.NEGATIVE
    assert rr.flags_ref(np.array([[0.25, -np.inf], [0.5, 0.5]])) == rr.NEGATIVE
    assert rr.flags_ref(np.array([[0.25, np.nan], [0.5, 0.5]])) == rr.NAN
    assert rr.flags_ref(np.array([[0.25, np.nan], [0.5, 0.0]])) == rr.NAN             # a NaN is no zero: the column has a load
    assert rr.flags_ref(np.array([[0.25, 0.0], [0.5, 0.0]])) == rr.NO_LOAD
    assert rr.flags_ref(np.array([[0.25, -0.0], [0.5, 0.0]])) == rr.NO_LOAD           # -0.0 == 0 and is not < 0
    assert rr.flags_ref(np.array([[0.25, 5e-324], [0.5, 0.0]])) == 0                  # a denormal is a load
    assert rr.flags_ref(np.array([[-1.0, 0.0, np.nan], [0.5, 0.0, 1.0]])) == rr.NEGATIVE | rr.NAN | rr.NO_LOAD
    assert rr.flags_ref(np.array([[np.inf, 1.0]])) == 0
    assert (rr.NEGATIVE, rr.NAN, rr.NO_LOAD) == (1, 2, 4)


def test_running_mean_ref_is_two_products_and_a_sum_where_an_fma_differs():
    keep, old, share, cur = rr.FMA_TRIPLE
    assert cur == 1.0 / 3.0 and (keep, share) in rr.COEFFS
    a, b = keep * old, share * cur
    two = float(rr.running_mean_ref(old, cur, keep, share))
    assert two == a + b
    fused_keep, fused_share = rr.fma_exact(keep, old, b), rr.fma_exact(share, cur, a)
    assert fused_keep == float(Fraction(keep) * Fraction(old) + Fraction(b))         # (fma_exact is one rounding of the exact value)
    assert fused_share == float(Fraction(share) * Fraction(cur) + Fraction(a))
    assert two != fused_keep and two != fused_share                                  # either contraction moves the last bit
    # elementwise on arrays, poisons included
    olds = np.array([old, np.nan, np.inf, -np.inf, -0.0, 5e-324])
    got = rr.running_mean_ref(olds, np.full(6, cur), keep, share)
    assert got[0] == two and np.isnan(got[1]) and got[2] == np.inf and got[3] == -np.inf and got[4] == b and got[5] == b
    z = rr.running_mean_ref(olds, np.full(6, cur), 0.0, 0.0)
    assert np.isnan(z[1:4]).all() and z[0] == 0 and z[4] == 0 and not np.signbit(z[4])          # 0 * inf = NaN; -0.0 + 0.0 = +0.0
    assert np.signbit(rr.running_mean_ref(-0.0, -0.0, 1.0, 1.0))


def test_device_row_helpers_place_topics_and_padding():
    for K in (5, 12, 130, 1000):
        lay = rr.layout(K)
        pad = rr.padding_positions(lay)
        assert len(pad) == lay.KP - K
        m = np.arange(3 * K).reshape(3, K) + 1
        rows = rr.device_dk(lay, m, pad=-7)
        assert (rows[:, pad] == -7).all()
        np.testing.assert_array_equal(lay.from_device(rows), m)
        np.testing.assert_array_equal(rr.device_kw(lay, m.T, pad=-7), rows)
        v = rr.device_vec(lay, np.arange(K) + 0.5, pad=np.nan, dtype=np.float64)
        assert np.isnan(v[pad]).all() and (v[lay.topic_pos] == np.arange(K) + 0.5).all()
    assert rr.same_bits(np.array([0.0]), np.array([-0.0])) is not None
    assert rr.same_bits(np.array([np.nan, 1.0]), np.array([np.nan, 1.0])) is None
    assert rr.same_bits(np.array([np.nan]), np.array([1.0])) is not None


# ------------------------------------------------------------------------------------------------
# return codes (the entry points return before they touch HIP)
# ------------------------------------------------------------------------------------------------
OK, BAD_K, BAD_ARG = 0, -1, -2


def test_readout_phi_validates_arguments():
    from lda_thesis_amd import _native
    phi = _native.lib().llda_readout_phi
    p = ctypes.c_void_p(4096)                                        # never dereferenced: every call below is refused on the host

    def call(n_kw=p, n_k=p, den=None, V=10, K=8, mode=0, out=p, flags=None):
        return phi(n_kw, n_k, den, V, K, 0.01, mode, 0.5, 0.5, out, flags, None)

    assert call(V=0) == BAD_ARG and call(V=-5) == BAD_ARG
    assert call(mode=2) == BAD_ARG and call(mode=-1) == BAD_ARG
    assert call(n_kw=None) == BAD_ARG
    assert call(out=None) == BAD_ARG
    assert call(n_k=None, den=None) == BAD_ARG
    for K in (0, -3, _native.MAX_K + 1):
        assert call(K=K) == BAD_K
        assert call(K=K, n_k=None, den=p, flags=p) == BAD_K


def test_readout_theta_validates_arguments():
    from lda_thesis_amd import _native
    theta = _native.lib().llda_readout_theta
    p = ctypes.c_void_p(4096)

    def call(n_dk=p, lab_mask=p, D=3, K=8, mode=0, out=p):
        return theta(n_dk, lab_mask, D, K, 0.1, mode, 0.5, 0.5, out, None)

    assert call(D=-1) == BAD_ARG
    assert call(mode=2) == BAD_ARG and call(mode=-1) == BAD_ARG and call(D=0, mode=2) == BAD_ARG
    for K in (0, -3, _native.MAX_K + 1):
        assert call(K=K) == BAD_K and call(K=K, D=0) == BAD_K
    assert call(n_dk=None) == BAD_ARG and call(lab_mask=None) == BAD_ARG and call(out=None) == BAD_ARG
    for K in (8, 1031, _native.MAX_K):                               # narrow and wide
        assert call(n_dk=None, lab_mask=None, out=None, D=0, K=K) == OK
        assert call(n_dk=None, lab_mask=None, out=None, D=0, K=K, mode=1) == OK
