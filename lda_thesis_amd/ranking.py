"""Label ranking and the harness metrics on the device (``llda_rank_labels``, include/llda_gibbs.h).

What the reference does with a held-out document's loads after the fold-in -- ``get_preds`` (/root/reference/LabeledLDA.py:214-229)
and ``rates`` / ``macro_auc_roc`` / ``n_error`` / ``get_f1`` (/root/reference/evaluate_LabeledLDA.py:8-93) -- costs the host two
sorts and a (thresholds x labels) matrix per document.  Here one kernel sorts every document's scores once and leaves per document
the top-n labels, its AUC, its best F1 and the rank of its best-ranked true label; the host downloads those few numbers, never
the (D, K) scores.

Tie rule: labels are ordered by score descending, then topic id ascending (``np.argsort(-row, kind="stable")``).  numpy's default
``argsort`` in the host's ``n_error`` and ``get_pred`` leaves the order of equal scores open; this rule does not.
"""
import numpy as np
import torch

from . import _native

NO_POSITIVE, NO_NEGATIVE, ONE_THRESHOLD, ALL_ZERO, HAS_NAN = (_native.RANK_NO_POSITIVE, _native.RANK_NO_NEGATIVE, _native.RANK_ONE_THRESHOLD,
                                                              _native.RANK_ALL_ZERO, _native.RANK_NAN)      # RankResult.flags bits
MAX_TOP_N = _native.RANK_MAX_TOP_N


class RankResult(object):
    """Per-document outputs of one ``rank_labels`` call, as device tensors: top_idx (D, top_n) int32 topic ids (-1 = padding),
    top_val (D, top_n) float64, n_thr (D,) int32 distinct scores, flags (D,) int32 and -- with truth -- auc, f1 (D,) float64 and
    hit_rank (D,) int32 (1-based rank of the best-ranked true label, 0 = none); without truth those three are None.
    ``host()`` downloads them once (D x (12 top_n + 28) bytes) as a dict of numpy arrays."""
    FIELDS = ("top_idx", "top_val", "n_thr", "auc", "f1", "hit_rank", "flags")

    def __init__(self, stream, D, K, first, top_n, **tensors):
        self.stream, self.D, self.K, self.first, self.top_n = stream, D, K, first, top_n
        for name in self.FIELDS:
            setattr(self, name, tensors.get(name))
        self._host = None

    def host(self):
        if self._host is None:
            with torch.cuda.stream(self.stream):
                self._host = {n: None if getattr(self, n) is None else getattr(self, n).cpu().numpy() for n in self.FIELDS}
        return self._host


def rank_labels(scores, truth=None, first=1, top_n=5, stream=None):
    """Rank the columns first .. K-1 of ``scores`` (D, K) float64 -- a torch tensor on the device (any row stride) or a numpy array,
    which is uploaded -- in reference topic order.  ``truth`` (D, K), non-zero = the document carries the label, or None: then only
    the top-n labels, n_thr and flags are computed.  first = 1 leaves the root label out, as the harness does.  Enqueues on ``stream``
    (default: the current one) and returns a RankResult."""
    _native.lib()
    _native.require_device()
    if isinstance(scores, torch.Tensor):
        if not scores.is_cuda:
            raise ValueError("scores: a torch tensor must live on the device (pass numpy arrays to have them uploaded)")
        dev = scores.device
        s = scores if scores.dtype == torch.float64 else scores.to(torch.float64)
    else:
        dev = torch.device("cuda:%d" % torch.cuda.current_device())
        s = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float64)).to(dev)
    if s.dim() != 2:
        raise ValueError("scores must be (documents, labels)")
    D, K = int(s.shape[0]), int(s.shape[1])
    if D > 0 and K > 0 and (s.stride(1) != 1 or (D > 1 and s.stride(0) < K)):
        s = s.contiguous()
    ld = int(s.stride(0)) if D > 1 else K
    if not 0 <= int(top_n) <= MAX_TOP_N:
        raise ValueError("top_n must be in 0 .. %d" % MAX_TOP_N)
    t = None
    if truth is not None:
        if isinstance(truth, torch.Tensor):
            t = (truth if truth.dtype == torch.uint8 else (truth != 0).to(torch.uint8)).to(dev).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(truth) != 0).view(np.uint8)).to(dev)
        if tuple(t.shape) != (D, K):
            raise ValueError("truth must have the shape of scores")
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = dict(top_idx=new((D, top_n), torch.int32), top_val=new((D, top_n), torch.float64), n_thr=new((D,), torch.int32),
                   flags=new((D,), torch.int32))
        if t is not None:
            out.update(auc=new((D,), torch.float64), f1=new((D,), torch.float64), hit_rank=new((D,), torch.int32))
        _native.rank_labels(s, t, D, K, first, top_n, ld=ld, **out)
        for x in (s, t):
            if x is not None:
                x.record_stream(stream)
    return RankResult(stream, D, K, int(first), int(top_n), **out)


def metrics(result):
    """dict(auc, one_error, two_error, f1, kept, dropped) of a RankResult with truth, by the rules of the harness's report
    (evaluate_LabeledLDA.py:150-180): documents whose ranked scores are all zero are dropped, the rest are macro-averaged with
    np.mean; one_error / two_error are the share of kept documents with a true label among the first one / two of the order.
    A kept document with fewer than two distinct scores raises the ValueError the host's trapezoid raises; a document without
    a positive or without a negative label gives nan, as on the host.  A NaN score raises ValueError."""
    if result.auc is None:
        raise ValueError("metrics need truth: rank_labels(scores, truth, ...)")
    h = result.host()
    flags = h["flags"]
    if np.any(flags & HAS_NAN):
        raise ValueError("scores of document %d hold a NaN" % int(np.flatnonzero(flags & HAS_NAN)[0]))
    keep = (flags & ALL_ZERO) == 0
    short = np.flatnonzero(keep & ((flags & ONE_THRESHOLD) != 0))
    if short.size:
        raise ValueError("At least 2 points are needed to compute area under curve, but x.shape = %s" % ((int(h["n_thr"][short[0]]),),))
    kept = int(keep.sum())
    hit = h["hit_rank"][keep]
    return dict(auc=np.mean(h["auc"][keep]), one_error=int(((hit > 0) & (hit <= 1)).sum()) / kept,
                two_error=int(((hit > 0) & (hit <= 2)).sum()) / kept, f1=np.mean(h["f1"][keep]), kept=kept,
                dropped=int(flags.shape[0]) - kept)
