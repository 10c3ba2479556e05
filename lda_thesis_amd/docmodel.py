"""What ``heldout.loglik``, ``attribution.attribute`` and ``leftright.loglik`` do alike before they call the library: check the
document offsets on the host, check the float64 matrices theta / phi_t, and stage the CSR doc_off / word / freq on the device."""
import numpy as np

from . import _native

MAX_FREQ = _native.HELDOUT_MAX_FREQ


def check_offsets(doc_off, D=None):
    """Host only.  doc_off (sequence, numpy array or tensor) -> (off_h, D, S): the offsets as a numpy array, the documents and the
    sites they span.  D given: exactly D + 1 offsets are wanted; None: D is what doc_off holds.  ValueError unless the offsets
    start at 0 or above and never descend."""
    off_h = doc_off.cpu().numpy() if hasattr(doc_off, "cpu") else np.asarray(doc_off, dtype=np.int64)
    if D is None:
        D = int(off_h.shape[0]) - 1
        wrong, msg = off_h.ndim != 1 or D < 0, "doc_off must hold D + 1 ascending offsets"
    else:
        wrong, msg = off_h.shape != (D + 1,), "doc_off must hold D + 1 = %d ascending offsets" % (D + 1)
    if wrong or (D and (int(off_h[0]) < 0 or np.any(np.diff(off_h) < 0))):
        raise ValueError(msg)
    return off_h, D, int(off_h[-1]) if D else 0


def matrix(x, name):
    """x must be a two-dimensional float64 tensor on the device; returned with unit column stride and a row stride >= its columns
    (a copy where it has not)."""
    import torch
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float64 and x.dim() == 2):
        raise ValueError("%s must be a two-dimensional float64 tensor on the device" % name)
    return x.contiguous() if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]) else x


def matrices(theta, phi_t):
    """theta (D, K) and phi_t (V, K) through ``matrix``, on one device and with one K -> (theta, phi_t, D, V, K)"""
    theta, phi_t = matrix(theta, "theta"), matrix(phi_t, "phi_t")
    if phi_t.device != theta.device:
        raise ValueError("theta and phi_t live on different devices")
    D, K = int(theta.shape[0]), int(theta.shape[1])
    if int(phi_t.shape[1]) != K:
        raise ValueError("theta has %d topics, phi_t %d" % (K, int(phi_t.shape[1])))
    return theta, phi_t, D, int(phi_t.shape[0]), K


def on_dev(a, dt, dev):
    """a (integers: numpy array, sequence or tensor) as a contiguous tensor of dtype dt on dev"""
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dt).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(device=dev, dtype=dt)


def stage(dev, doc_off, word, freq, S, V=None, unit="sites"):
    """(d_off int64, d_word int32, d_freq int32 or None) on dev for the S sites that doc_off spans.  word and freq must hold S
    entries at least; V given: the word ids must be in [0, V); the frequencies in 0 .. MAX_FREQ."""
    import torch
    d_off, d_word = on_dev(doc_off, torch.int64, dev), on_dev(word, torch.int32, dev)
    if int(d_word.numel()) == 0:
        d_word = torch.zeros((1,), dtype=torch.int32, device=dev)      # (nothing at all: the pointer must still be one)
    if int(d_word.numel()) < S:
        raise ValueError("word holds %d %s, doc_off asks for %d" % (int(d_word.numel()), unit, S))
    if V is not None and S and (int(d_word[:S].min()) < 0 or int(d_word[:S].max()) >= V):
        raise ValueError("word ids must be in [0, V)")
    d_freq = None
    if freq is not None:
        d_freq = on_dev(freq, torch.int32, dev)
        if int(d_freq.numel()) < S:
            raise ValueError("freq holds %d %s, doc_off asks for %d" % (int(d_freq.numel()), unit, S))
        if S and (int(d_freq[:S].min()) < 0 or int(d_freq[:S].max()) > MAX_FREQ):
            raise ValueError("frequencies must be in 0 .. 2^23 - 1")
    return d_off, d_word, d_freq
