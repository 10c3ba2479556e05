"""llda_foldin on the planted inputs of tests/foldinties.py: last-bit ties of the keyed draw, sites just outside the decided tier's band,
planted rows of init_rows, and loadings at the edges of the double range -- z, n_dk and th equal tests/foldinref.py bit for bit for every
document, status is 0, the sentinel margins of countref.Guarded are intact, and the n_sites = 0 and n_sites = S paths agree
(test_gpu_foldin_direct.check).  tests/test_foldin_ties_host.py shows what the inputs are and that a tier without the margin, or a
coarser one, or one without the floor on the total, fails them.

K = 9 .. 968 are the narrow layouts G = 8 .. 64, with and without a tail (in an even wavefront every second document hands its planted
site over while its neighbours decide theirs); 1031 and 2100 are wide (exact pipeline only: there the ties pin the strict `>` of
wide_draw and the division).  Both start paths, exact_only 0 and 1, iters = 3 and thinning = 1, so the planted draw reaches th.

SCALES: the same loadings times an exact power of two per word.  The reference divides with numpy's true division, so a total in the
subnormal range or next to the overflow threshold is an ordinary input to it; where it raises (every product of a site underflows to
zero and there is no fall-back) bit 0 of status is compared instead, as test_status_reports_a_site_without_probability does, and the
other documents still have to agree.

What these cases found in the kernels as they were (no floor on the decided tier's total, no rescaling in front of the division): the
ties, the just-outside sites and the planted rows all passed; at sub1045 and sub1066 the exact pipeline set status 1 and missed every
document (y = 1 / S = inf) and the decided tier missed 25 of 128 documents at K = 9, 17 of 128 at K = 40, 7 of 64 at K = 130; at tiny1000
one document of 32 at K = 2100 (a planted tie, div_by's residuals inexact at S = 2^-1000).  142 of the 576 runs in all.

No ties are planted for beta_fallback's own scores (n_dk + alpha) * beta: they hold nothing to tune, and the grid of
test_gpu_foldin_direct covers that branch on random data.
"""
import functools

import numpy as np
import pytest

import foldinties as ft
from test_gpu_foldin_direct import SETTINGS, check, device, reference, same

pytestmark = pytest.mark.gpu

KS = [9, 40, 130, 257, 512, 777, 968, 1031, 2100]


@functools.lru_cache(maxsize=None)
def expected(K, setting, which):
    c = ft.tie_case(K, setting)[0] if which == "ties" else ft.init_case(K, setting)[0] if which == "init" else ft.scaled_case(K, setting, which)
    return c, reference(c)


@pytest.mark.parametrize("exact_only", [0, 1])
@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("K", KS)
def test_planted_ties_and_just_outside_sites(K, setting, start, exact_only):
    c, want = expected(K, setting, "ties")
    check(c, want, start, exact_only, "ties K=%d %s %s exact_only=%d" % (K, setting, start, exact_only))


@pytest.mark.parametrize("exact_only", [0, 1])
@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("K", KS)
def test_planted_initial_rows(K, setting, start, exact_only):
    c, want = expected(K, setting, "init")
    check(c, want, start, exact_only, "init rows K=%d %s %s exact_only=%d" % (K, setting, start, exact_only))


@pytest.mark.parametrize("exact_only", [0, 1])
@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("scale", sorted(ft.SCALES))
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("K", KS)
def test_extreme_scales(K, setting, scale, start, exact_only):
    c, want = expected(K, setting, scale)
    what = "%s K=%d %s %s exact_only=%d" % (scale, K, setting, start, exact_only)
    if not want["raises"].any():
        check(c, want, start, exact_only, what)
        return
    bad = set(np.flatnonzero(want["raises"]))
    assert len(bad) <= len(want["raises"]) // 2, what                     # (half of the documents at least are still compared)
    got = device(c, start, exact_only)
    assert got["status"] & 1, what
    same(got, want, c["doc_off"], skip=bad, what=what)
    if start == "inside":
        same(got, device(c, "sites", exact_only), c["doc_off"], skip=bad, what=what + " inside vs sites")
