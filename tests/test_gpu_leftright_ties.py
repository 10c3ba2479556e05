"""llda_left_to_right on the planted inputs of tests/leftrightties.py: last-bit ties of draw64 (decided by an integer model and tuned
with counts in play), the no-hit rule reached by overflow and by subnormal rounding, loadings at both ends of the double range, and
the largest launch the header allows -- mant, expo, tok, bad and status equal tests/leftrightref.py bit for bit.
tests/test_leftright_ties_host.py shows what the inputs are and which wrong draws fail them.

K = 2 .. 1024 are every NI class (1, 2, 4, 8, 16 slots per lane) and both sides of its edges; R = 1, 3, 16 with the planted particle
r_star at 0, R - 1 and, for R = 16, at 8, the first whose stream id has wrapped around 2^32.  Planted and random documents alternate in
one launch; ld_phi = ld_allowed = K + 3 with NaN / 1 beyond K (test_gpu_leftright.device_run).
"""
import functools

import numpy as np
import pytest

import leftrightref as ref
import leftrightties as lt
from test_gpu_leftright import _check, device_run

pytestmark = pytest.mark.gpu

KS = (2, 9, 64, 65, 128, 130, 257, 512, 1000, 1024)
PARTICLES = ((1, 0), (3, 0), (3, 2), (16, 0), (16, 8), (16, 15))


def device(c, R, cap=None):
    return device_run(c["phi_t"], c["K"], c["doc_off"], c["word"], c["alpha"], R, lt.SEED, lt.STREAM, allowed=c["allowed"],
                      doc_ids=c["doc_ids"], cap=cap)


@pytest.mark.parametrize("R,r_star", PARTICLES)
@pytest.mark.parametrize("K", KS)
def test_exact_ties(K, R, r_star):
    """the integer model's z_0 in every planted document, read from the device's own (mant, expo)"""
    c = lt.exact_case(K, R, r_star)
    trace = {}
    want = lt.expected(c, R, trace=trace)
    got = device(c, R)
    named = lt.decode_z0(c, got[0], got[1], trace["z"])
    wrong = [(j, p["kind"], p["cls"], p["z0"], named[j]) for j, p in enumerate(c["plants"]) if named[j] != [p["z0"]]]
    assert not wrong, "%d of %d plants, the first: %s" % (len(wrong), len(c["plants"]), wrong[:5])
    _check(got, want)


@pytest.mark.parametrize("R,r_star", PARTICLES)
@pytest.mark.parametrize("K", KS)
def test_tuned_ties(K, R, r_star):
    c = lt.tuned_case(K, R, r_star)
    assert len(c["plants"]) >= 16
    _check(device(c, R), lt.expected(c, R))


@pytest.mark.parametrize("scale", sorted(lt.SCALES))
@pytest.mark.parametrize("K", (9, 130, 1024))
def test_extreme_scales(K, scale):
    c = lt.scaled_case(K, scale)
    want = lt.expected(c, c["R"])
    assert want[2].sum() > 0.9 * np.diff(c["doc_off"]).sum()            # (the p_n are finite and positive: they are compared as such)
    _check(device(c, c["R"]), want)


@pytest.mark.parametrize("K", (40, 130, 1000))
def test_no_hit_by_overflow(K):
    c = lt.overflow_case(K)
    assert min(c["no_hit"]) > 0
    _check(device(c, c["R"]), lt.expected(c, c["R"]))


@functools.lru_cache(maxsize=None)
def _largest(K):
    rng = np.random.default_rng([35, K])
    V = 40
    phi = lt.random_loadings(rng, K, V)
    lens = (40, 3, 150, 0, 4097, 17, 1)
    docs = [rng.integers(0, V, size=n) for n in lens]
    doc_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = dict(K=K, phi_t=phi, doc_off=doc_off, word=np.concatenate(docs).astype(np.int64), allowed=np.ones((len(lens), K), dtype=np.uint8),
             doc_ids=lt.doc_ids(len(lens)), alpha=lt.ALPHA)
    return c, lens, lt.expected(c, 16, max_doc_tokens=4096)


@pytest.mark.parametrize("K", (1, 1024))
def test_the_largest_launch(K):
    """max_doc_tokens = 4096 with 16 particles: 147 712 bytes of dynamic LDS, 1024 threads; the last particle's assignments lie at
    the top of it.  One document of 4097 tokens is refused; the same batch with room for the longest kept document only gives the
    same bytes"""
    c, lens, want = _largest(K)
    got = device(c, 16, cap=4096)
    _check(got, want)
    over = lens.index(4097)
    assert got[4] == 1 and (got[0][over], got[1][over], got[2][over], got[3][over]) == (0.5, 1, 0, 0)
    assert got[2][lens.index(150)] + got[3][lens.index(150)] == 150
    small = device(c, 16, cap=150)
    assert small[4] == 1
    for a, b in zip(got[:4], small[:4]):
        assert a.tobytes() == b.tobytes()
