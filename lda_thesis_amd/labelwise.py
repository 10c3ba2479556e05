"""Label-wise evaluation and tuned label sets on the device (``llda_label_metrics``, ``llda_label_sets``; include/llda_gibbs.h).

``ranking.py`` looks at a document and ranks its K labels.  This module looks at a label and ranks its D documents: per label the
AUC, the best F1 and the threshold that reaches it (SCut), and -- on request -- the order itself.  With one threshold per label a
document's prediction is a SET, the labels whose load reaches their threshold, instead of always n labels; ``label_sets`` applies
the thresholds on the device and counts what micro / macro / example-based F1 need.

Tie rule: documents are ordered by score descending, then document id ascending (``np.argsort(-col, kind="stable")``).  The
label-wise AUC starts its curve at (0, 0) -- the usual definition, the Mann-Whitney statistic -- and is therefore not the
per-document figure of ``ranking``, which keeps the reference's start at the first threshold.
"""
import numpy as np

from . import _native

NO_POSITIVE, NO_NEGATIVE, ONE_THRESHOLD, ALL_ZERO, HAS_NAN = (_native.RANK_NO_POSITIVE, _native.RANK_NO_NEGATIVE, _native.RANK_ONE_THRESHOLD,
                                                              _native.RANK_ALL_ZERO, _native.RANK_NAN)      # LabelResult.flags bits
MAX_D = _native.LABEL_MAX_D


def _device_scores(scores):
    """(tensor (D, K) float64 on the device with unit column stride, ld)"""
    import torch
    if isinstance(scores, torch.Tensor):
        if not scores.is_cuda:
            raise ValueError("scores: a torch tensor must live on the device (pass numpy arrays to have them uploaded)")
        s = scores if scores.dtype == torch.float64 else scores.to(torch.float64)
    else:
        s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64)).to(torch.device("cuda:%d" % torch.cuda.current_device()))
    if s.dim() != 2:
        raise ValueError("scores must be (documents, labels)")
    D, K = int(s.shape[0]), int(s.shape[1])
    if D > 0 and K > 0 and (s.stride(1) != 1 or (D > 1 and s.stride(0) < K)):
        s = s.contiguous()
    return s, (int(s.stride(0)) if D > 1 else K)


def _device_truth(truth, shape, dev):
    import torch
    if isinstance(truth, torch.Tensor):
        t = (truth if truth.dtype == torch.uint8 else (truth != 0).to(torch.uint8)).to(dev).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(truth) != 0).view(np.uint8)).to(dev)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("truth must have the shape of scores")
    return t


class LabelResult(object):
    """Per-label outputs of one ``label_metrics`` call, as device tensors over the labels first .. K-1: n_pos, n_thr, thr_tp, thr_fp
    (L,) int64, auc_num (L,) int64 (the Mann-Whitney count A; below 2^61), auc, f1, thr (L,) float64, flags (L,) int32 and, when
    asked for, order (L, D) int32.  ``host()`` downloads them once as a dict of numpy arrays."""
    FIELDS = ("n_pos", "n_thr", "auc_num", "auc", "thr_tp", "thr_fp", "f1", "thr", "flags", "order")

    def __init__(self, stream, D, K, first, **tensors):
        self.stream, self.D, self.K, self.first = stream, D, K, first
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))
        self._host = None

    def host(self):
        if self._host is None:
            import torch
            with torch.cuda.stream(self.stream):
                self._host = {n: None if getattr(self, n) is None else getattr(self, n).cpu().numpy() for n in self.FIELDS}
        return self._host


def label_metrics(scores, truth, first=1, order=False, stream=None, max_scratch_bytes=None, chunk=0):
    """Rank the documents of every label first .. K-1 of ``scores`` (D, K) float64 -- a torch tensor on the device (any row stride) or
    a numpy array, which is uploaded -- against ``truth`` (D, K), non-zero = the document carries the label.  1 <= D <= 2^30.
    The sort needs 24 bytes of scratch per document and label; when all labels together would take more than ``max_scratch_bytes``
    (default: a quarter of the free device memory) the labels are walked in batches, with the same result.  order=True also returns
    the ranked document ids (L x D x 4 bytes).  ``chunk``: 0, or 256 for tests of the merge tree; no output depends on it.  Enqueues
    on ``stream`` (default: the current one) and returns a LabelResult."""
    import torch
    _native.lib()
    _native.require_device()
    s, ld = _device_scores(scores)
    dev = s.device
    D, K = int(s.shape[0]), int(s.shape[1])
    if not 1 <= D <= MAX_D:
        raise ValueError("label_metrics needs 1 .. 2^30 documents")
    if not 0 <= int(first) <= K:
        raise ValueError("first must be in 0 .. K")
    first = int(first)
    L = K - first
    t = _device_truth(truth, (D, K), dev)
    per_label = _native.label_scratch_bytes(D, 1, chunk) - 16
    if max_scratch_bytes is None:
        max_scratch_bytes = torch.cuda.mem_get_info(dev)[0] // 4
    batch = max(1, min(L, (int(max_scratch_bytes) - 16) // per_label)) if L else 0
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = {n: new((L,), torch.int64) for n in ("n_pos", "n_thr", "auc_num", "thr_tp", "thr_fp")}
        out.update({n: new((L,), torch.float64) for n in ("auc", "f1", "thr")})
        out["flags"] = new((L,), torch.int32)
        if order:
            out["order"] = new((L, D), torch.int32)
        if L:
            scratch = new((_native.label_scratch_bytes(D, batch, chunk),), torch.uint8)
            for l0 in range(0, L, batch):
                l1 = min(L, l0 + batch)
                _native.label_metrics(s, t, D, K, first + l0, l1 - l0, scratch, ld=ld, chunk=chunk, **{n: v[l0:l1] for n, v in out.items()})
            scratch.record_stream(stream)
        for x in (s, t):
            x.record_stream(stream)
    return LabelResult(stream, D, K, first, **out)


def macro(result):
    """dict(macro_auc, macro_f1, n_labels, skipped) of a LabelResult (or of its ``host()`` dict): np.mean of auc and of f1 over the
    labels that have a positive and a negative document; ``skipped`` counts the others (flags 1 or 2), ``n_labels`` the ones
    averaged.  No label left: both means are nan.  A NaN score raises ValueError, as ``ranking.metrics`` does."""
    h = result if isinstance(result, dict) else result.host()
    flags = np.asarray(h["flags"])
    if np.any(flags & HAS_NAN):
        raise ValueError("scores of label row %d hold a NaN" % int(np.flatnonzero(flags & HAS_NAN)[0]))
    keep = (flags & (NO_POSITIVE | NO_NEGATIVE)) == 0
    n = int(keep.sum())
    nan = float("nan")
    return dict(macro_auc=np.mean(np.asarray(h["auc"])[keep]) if n else nan, macro_f1=np.mean(np.asarray(h["f1"])[keep]) if n else nan,
                n_labels=n, skipped=int(flags.shape[0]) - n)


def thresholds(result, K=None, first=None):
    """K doubles for ``label_sets`` from a LabelResult (or its host dict, then with K and first): every label's best-F1 threshold,
    NaN -- never predicted -- below ``first`` and for labels without a positive document.  A NaN score raises ValueError."""
    h = result if isinstance(result, dict) else result.host()
    K = result.K if K is None else K
    first = result.first if first is None else first
    if np.any(np.asarray(h["flags"]) & HAS_NAN):
        raise ValueError("scores hold a NaN")
    thr = np.full((K,), np.nan)
    thr[first:] = h["thr"]
    return thr


def set_scores(tp, fp, fn, n_pred, n_hit, n_true, first=1):
    """dict(micro_f1, macro_f1, example_f1, labels_scored, docs_scored) from the integer counts of ``llda_label_sets``:
    micro_f1 = 2 sum tp / (2 sum tp + sum fp + sum fn); macro_f1 = np.mean over the labels >= first with 2 tp + fp + fn > 0 of
    2 tp / (2 tp + fp + fn); example_f1 = np.mean over the documents with n_pred + n_true > 0 of 2 n_hit / (n_pred + n_true).  Every
    ratio is one division of two exact integers; a mean over nothing is nan.  A document with n_pred = -1 (a NaN score) raises
    ValueError."""
    tp, fp, fn = (np.asarray(x, dtype=np.int64)[first:] for x in (tp, fp, fn))
    n_pred, n_hit, n_true = (np.asarray(x, dtype=np.int64) for x in (n_pred, n_hit, n_true))
    if np.any(n_pred < 0):
        raise ValueError("scores of document %d hold a NaN" % int(np.flatnonzero(n_pred < 0)[0]))
    nan = float("nan")
    den = 2 * tp + fp + fn
    micro_den = int(den.sum())
    lab = den > 0
    doc_den = n_pred + n_true
    doc = doc_den > 0
    return dict(micro_f1=2 * int(tp.sum()) / micro_den if micro_den else nan,
                macro_f1=np.mean((2 * tp[lab]) / den[lab]) if lab.any() else nan,
                example_f1=np.mean((2 * n_hit[doc]) / doc_den[doc]) if doc.any() else nan,
                labels_scored=int(lab.sum()), docs_scored=int(doc.sum()))


def mask_rows(mask, K):
    """(D, K) bool from the (D, W) bit words of ``llda_label_sets``"""
    m = np.ascontiguousarray(mask).view(np.uint32)
    bits = (m[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & np.uint32(1)
    return bits.reshape(m.shape[0], -1)[:, :K].astype(bool)


class SetResult(object):
    """Outputs of one ``label_sets`` call, as device tensors: mask (D, W) int32 bit words (bit k & 31 of word k >> 5), n_pred (D,)
    int32 (-1: a NaN score) and -- with truth -- n_hit, n_true (D,) int32, tp, fp, fn (K,) int64; ``host()`` downloads them once,
    ``sets()`` gives the (D, K) bool matrix, and micro_f1 / macro_f1 / example_f1 are ``set_scores`` of the counts."""
    FIELDS = ("mask", "n_pred", "n_hit", "n_true", "tp", "fp", "fn")

    def __init__(self, stream, D, K, first, **tensors):
        self.stream, self.D, self.K, self.first = stream, D, K, first
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))
        self._host = self._scores = None

    def host(self):
        if self._host is None:
            import torch
            with torch.cuda.stream(self.stream):
                self._host = {n: None if getattr(self, n) is None else getattr(self, n).cpu().numpy() for n in self.FIELDS}
        return self._host

    def sets(self):
        return mask_rows(self.host()["mask"], self.K)

    def scores(self):
        if self.tp is None:
            raise ValueError("set scores need truth: label_sets(scores, thr, truth, ...)")
        if self._scores is None:
            h = self.host()
            self._scores = set_scores(h["tp"], h["fp"], h["fn"], h["n_pred"], h["n_hit"], h["n_true"], first=self.first)
        return self._scores

    micro_f1 = property(lambda self: self.scores()["micro_f1"])
    macro_f1 = property(lambda self: self.scores()["macro_f1"])
    example_f1 = property(lambda self: self.scores()["example_f1"])


def label_sets(scores, thr, truth=None, first=1, at_least_one=True, stream=None):
    """Apply the per-label thresholds ``thr`` (K doubles; NaN = never predicted) to ``scores`` (D, K): label k >= first is predicted
    for a document when its score is >= thr[k]; with at_least_one a document that would predict nothing predicts its best label
    among those with a threshold.  ``truth`` (D, K) adds the counts of the F1 figures.  Enqueues on ``stream`` (default: the
    current one) and returns a SetResult."""
    import torch
    _native.lib()
    _native.require_device()
    s, ld = _device_scores(scores)
    dev = s.device
    D, K = int(s.shape[0]), int(s.shape[1])
    if not 0 <= int(first) <= K:
        raise ValueError("first must be in 0 .. K")
    th = thr if isinstance(thr, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64))
    th = th.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(th.shape) != (K,):
        raise ValueError("thr must hold one threshold per label")
    t = None if truth is None else _device_truth(truth, (D, K), dev)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        out = dict(mask=torch.empty((D, (K + 31) // 32), dtype=torch.int32, device=dev), n_pred=torch.empty((D,), dtype=torch.int32, device=dev))
        if t is not None:
            out.update(n_hit=torch.empty((D,), dtype=torch.int32, device=dev), n_true=torch.empty((D,), dtype=torch.int32, device=dev))
            out.update({n: torch.zeros((K,), dtype=torch.int64, device=dev) for n in ("tp", "fp", "fn")})
        if D and K:
            _native.label_sets(s, th, t, D, K, int(first), at_least_one, ld=ld, **out)
        for x in (s, th, t):
            if x is not None:
                x.record_stream(stream)
    return SetResult(stream, D, K, int(first), **out)
