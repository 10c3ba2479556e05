"""llda_phi_step on the device: bit for bit against tests/emref.py around the blocks of 256 words of the column sums and the
blocks of 256 columns of the kernels, with padded strides, in place and out of place, with guard words round every output."""
import numpy as np
import pytest

import emref

pytestmark = pytest.mark.gpu

VS = (1, 255, 256, 257, 1000)
KS = (1, 8, 64, 65, 513)
GUARD = 8
PAT = np.float64(-1234.5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def credit(rng, V, K, pad):
    """a word credit: mostly small, exact zeros, a few large entries; NaN in the columns >= K"""
    cw = np.full((V, K + pad), np.nan)
    body = rng.gamma(0.3, size=(V, K)) * rng.choice((1e-3, 1.0, 1e4), size=(V, K))
    body[rng.random((V, K)) < 0.3] = 0.0
    cw[:, :K] = body
    return cw


def run(cw, K, beta, in_place, pad_out, with_den=True):
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    V, ld = cw.shape
    d_cw = torch.full((V * ld + 2 * GUARD,), PAT.item(), dtype=torch.float64, device=dev)
    d_cw[GUARD:GUARD + V * ld] = torch.from_numpy(cw.reshape(-1)).to(dev)
    src = d_cw[GUARD:GUARD + V * ld]
    ld_out = ld if in_place else K + pad_out
    d_out = d_cw if in_place else torch.full((V * ld_out + 2 * GUARD,), PAT.item(), dtype=torch.float64, device=dev)
    dst = d_out[GUARD:GUARD + V * ld_out]
    d_den = torch.full((K + 2 * GUARD,), PAT.item(), dtype=torch.float64, device=dev)
    need = _native.phi_step_scratch_bytes(V, K)
    scratch = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device=dev)
    _native.phi_step(src, V, K, beta, dst, scratch[:need], ld=ld, ld_out=ld_out, den=d_den[GUARD:GUARD + K] if with_den else None)
    torch.cuda.synchronize()
    assert (scratch[need:] == 0xA5).all(), "written behind the scratch"
    return d_out.cpu().numpy(), d_den.cpu().numpy(), ld_out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
def test_bit_for_bit_against_emref(V, K):
    rng = np.random.default_rng(41000 + 10 * V + K)
    for in_place, pad, pad_out, beta, with_den in ((False, 3, 2, 0.01, True), (True, 3, 0, 0.001, True), (False, 0, 0, 0.5, False),
                                                  (True, 0, 0, 1e-9, False)):
        cw = credit(rng, V, K, pad)
        want_phi, want_den = emref.phi_step_ref(cw, beta, K=K)
        out, den, ld_out = run(cw, K, beta, in_place, pad_out, with_den)
        what = "V %d K %d in place %s ld %d" % (V, K, in_place, ld_out)
        assert (out[:GUARD] == PAT).all() and (out[-GUARD:] == PAT).all(), what
        body = out[GUARD:-GUARD].reshape(V, ld_out)
        behind = body[:, K:]
        assert (np.isnan(behind).all() if in_place else (behind == PAT).all()), what + ": written behind column K"
        assert np.array_equal(bits(body[:, :K]), bits(want_phi)), what
        assert (den[:GUARD] == PAT).all() and (den[-GUARD:] == PAT).all(), what
        if with_den:
            assert np.array_equal(bits(den[GUARD:-GUARD]), bits(want_den)), what
        else:
            assert (den == PAT).all(), what
        assert (want_phi > 0.0).all() and np.abs(want_phi.sum(axis=0) - 1.0).max() < 1e-12


def test_python_surface():
    import torch
    from lda_thesis_amd import emfit
    rng = np.random.default_rng(42)
    V, K = 300, 20
    cw = credit(rng, V, K, 4)
    want_phi, want_den = emref.phi_step_ref(cw, 0.05, K=K)
    d_cw = torch.from_numpy(cw).to("cuda:0")[:, :K]                        # row stride K + 4
    got = emfit.phi_step(d_cw, 0.05)
    assert got.shape == (V, K) and got.is_contiguous() and np.array_equal(bits(got.cpu().numpy()), bits(want_phi))
    phi, den = emfit.phi_step(d_cw, 0.05, want_den=True)
    assert np.array_equal(bits(den.cpu().numpy()), bits(want_den)) and np.array_equal(bits(phi.cpu().numpy()), bits(want_phi))
    assert emfit.phi_step(d_cw, 0.05, out=d_cw) is d_cw and np.array_equal(bits(d_cw.cpu().numpy()), bits(want_phi))
    for bad in (dict(beta=0.0), dict(beta=float("nan")), dict(beta=float("inf")), dict(cw=cw), dict(out=torch.empty((V, K + 1), dtype=torch.float64, device="cuda:0")),
                dict(out=torch.empty((V, K), dtype=torch.float32, device="cuda:0"))):
        args = dict(cw=d_cw, beta=0.1, out=None)
        args.update(bad)
        with pytest.raises(ValueError):
            emfit.phi_step(args["cw"], args["beta"], out=args["out"])
