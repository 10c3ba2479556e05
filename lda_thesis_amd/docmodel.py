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


def label_csr(labs, K=None):
    """Host only.  The label sets of D documents as a CSR: (lab_off int64 [D+1], lab int32 [NL]), every document's ids ascending.
    ``labs`` is a (D, K) array whose non-zero entries are the labels, or one sequence of label ids per document (any order; K
    given: the ids must be in [0, K)).  ValueError for an id out of range or a label named twice."""
    if isinstance(labs, np.ndarray) and labs.ndim == 2:
        if K is not None and labs.shape[1] != int(K):
            raise ValueError("labs has %d columns, K is %d" % (labs.shape[1], int(K)))
        rows, cols = np.nonzero(labs)                                       # (row-major: ascending within a document)
        lab_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=labs.shape[0]))]).astype(np.int64)
        return lab_off, cols.astype(np.int32)
    lists = [np.sort(np.asarray(list(x), dtype=np.int64)) for x in labs]
    for d, c in enumerate(lists):
        if c.size and (c[0] < 0 or c[-1] >= (2 ** 31 if K is None else int(K))):
            raise ValueError("document %d: a label id is outside 0 .. %s" % (d, "2^31 - 1" if K is None else int(K) - 1))
        if np.any(np.diff(c) == 0):
            raise ValueError("document %d: a label is named twice" % d)
    lab_off = np.concatenate([[0], np.cumsum([c.size for c in lists])]).astype(np.int64)
    return lab_off, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)


def label_sets(lab_off, lab, D, K, limit=_native.SPARSE_MAX_LABELS):
    """Host check of a label CSR (sequences, numpy arrays or tensors) before a sparse-label launch -> (off_h, lab_h, NL, max_labels):
    D + 1 ascending offsets from 0, NL ids in [0, K) that ascend strictly inside every document, at most ``limit`` per document.
    max_labels is the longest list, 1 at least."""
    off_h, _, NL = check_offsets(lab_off, D)
    lab_h = lab.cpu().numpy() if hasattr(lab, "cpu") else np.asarray(lab)
    if D and int(off_h[0]) != 0:
        raise ValueError("lab_off must start at 0")
    if lab_h.ndim != 1 or lab_h.shape[0] < NL:
        raise ValueError("lab holds %d label ids, lab_off asks for %d" % (lab_h.shape[0] if lab_h.ndim == 1 else -1, NL))
    lab_h = lab_h[:NL].astype(np.int64)
    if NL and (int(lab_h.min()) < 0 or int(lab_h.max()) >= K):
        raise ValueError("label ids must be in [0, K)")
    inner = np.ones(max(NL - 1, 0), dtype=bool)
    inner[off_h[1:-1][(off_h[1:-1] > 0) & (off_h[1:-1] < NL)] - 1] = False  # (the step from one document's list to the next)
    if NL > 1 and np.any((np.diff(lab_h) <= 0) & inner):
        raise ValueError("the label ids of a document must ascend strictly")
    longest = int(np.diff(off_h).max()) if D else 0
    if longest > limit:
        raise ValueError("a document has %d labels: the sparse-label form takes %d at most" % (longest, limit))
    return off_h, lab_h.astype(np.int32), NL, max(longest, 1)


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
