"""Held-out perplexity by document completion, scored on the device (``llda_heldout_loglik``, include/llda_gibbs.h).

How well does a trained model predict text it has not seen?  The reference has no such number (its ``perplexity`` scores the
training corpus, /root/reference/LabeledLDA.py:256-265), so the definition is this project's:

  * a held-out document is its ``doc2bow`` list, word ids ascending; the sites 0, 2, 4, ... are OBSERVED, the sites 1, 3, 5, ...
    SCORED (``completion_split``), or the caller brings its own two lists;
  * the observed halves go through the fold-in as they are (``foldin.fold_in``); its thinned average ``th`` is smoothed with the
    observed tokens W_d:  theta[d][k] = (W_d * th[d][k] + alpha) / (W_d + K * alpha)   (``smooth_theta``: IEEE float64, every
    operation rounded on its own);
  * a scored site (w, f) has p = sum_k theta[d][k] * phi[k][w]; perplexity = exp(-sum f log p / sum f).

The kernel leaves per document the product of its p^f as a pair (mantissa in [0.5, 1), 64-bit exponent), the scored tokens and the
tokens of sites whose p was not a finite positive number: 32 bytes come back per document, and the host takes the logarithm.
"""
import math

import numpy as np

from . import _native, docmodel

MAX_FREQ = _native.HELDOUT_MAX_FREQ


def completion_split(doc_tups):
    """doc2bow lists -> (observed, scored): the sites 0, 2, 4, ... and 1, 3, 5, ... of every document.  A document with one site
    has nothing scored, an empty one nothing at all."""
    return [list(t[0::2]) for t in doc_tups], [list(t[1::2]) for t in doc_tups]


def observed_tokens(doc_tups):
    """W_d: the sum of the frequencies of every document, float64 [D] (exact integers)."""
    return np.array([float(sum(int(f) for _, f in t)) for t in doc_tups], dtype=np.float64)


def smooth_theta(th, w_obs, alpha):
    """(W_d * th + alpha) / (W_d + K * alpha) with th (D, K) and W_d [D]: numpy arrays, or torch tensors on one device -- the same
    IEEE operations in the same order either way (a product, a sum, a product and a sum of scalars, a division)."""
    K = th.shape[1]
    return (w_obs[:, None] * th + alpha) / (w_obs + K * alpha)[:, None]


def loglik(theta_dev, phi_t_dev, doc_off, word, freq, weighted=True):
    """Score the sites of the CSR doc_off (int64 [D+1]) / word / freq (numpy arrays or device tensors) against theta_dev (D, K) and
    phi_t_dev (V, K), float64 tensors on the device in reference topic order (any row stride >= K).  weighted=False: every
    frequency counts as 1.  Returns the per-document (mant, expo, tok, bad) as numpy arrays: float64, int64, int64, int64."""
    import torch
    _native.lib()
    _native.require_device()
    theta_dev, phi_t_dev, D, V, K = docmodel.matrices(theta_dev, phi_t_dev)
    dev = theta_dev.device
    _, _, S = docmodel.check_offsets(doc_off, D)
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq if weighted else None, S, V)
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    _native.heldout_loglik(d_off, d_word, d_freq, theta_dev, phi_t_dev, D, V, K,
                           ld_theta=int(theta_dev.stride(0)) if D > 1 else K, ld_phi=int(phi_t_dev.stride(0)) if V > 1 else K,
                           mant=mant, expo=expo, tok=tok, bad=bad)
    return mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy()


def loglik_sparse(theta_s, phi_t_dev, doc_off, word, freq, lab_off, lab, weighted=True):
    """``loglik`` for documents that carry a few of the K labels (``llda_heldout_loglik_sparse``): the label sets are
    the CSR lab_off (int64 [D+1]) / lab (``docmodel.label_csr``), theta_s (float64 [NL], on the device) the loads per slot.  A site
    reads len(labels) entries of its word's row of phi_t_dev (V, K), not K, and no (D, K) matrix exists.  Returns the same
    (mant, expo, tok, bad).  ValueError on the host, before any launch, for label sets the kernel would call unfit."""
    import torch
    from . import attribution
    _native.lib()
    _native.require_device()
    phi_t_dev = docmodel.matrix(phi_t_dev, "phi_t")
    V, K = int(phi_t_dev.shape[0]), int(phi_t_dev.shape[1])
    dev = phi_t_dev.device
    _, D, S = docmodel.check_offsets(doc_off)
    off_h, lab_h, NL, max_labels = docmodel.label_sets(lab_off, lab, D, K)
    theta_s = attribution._slots(theta_s, NL, dev, "theta_s")
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq if weighted else None, S, V)
    d_loff, d_lab = docmodel.on_dev(off_h, torch.int64, dev), docmodel.on_dev(lab_h if NL else np.zeros(1), torch.int32, dev)
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    _native.heldout_loglik_sparse(d_off, d_word, d_freq, d_loff, d_lab, theta_s, phi_t_dev, D, V, K, NL, max_labels,
                                  ld_phi=int(phi_t_dev.stride(0)) if V > 1 else K, mant=mant, expo=expo, tok=tok, bad=bad)
    return mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy()


def smooth_slots(th_s, w_obs, lab_off, alpha):
    """``smooth_theta`` per slot of a label CSR, with a document's label count L_d in place of K:  (W_d * th + alpha) / (W_d + L_d *
    alpha) at every slot of document d.  th_s [NL], w_obs [D] and lab_off [D+1] (host offsets): numpy arrays, or th_s / w_obs torch
    tensors on one device -- the same IEEE operations in the same order either way."""
    off_h = np.asarray(lab_off, dtype=np.int64)
    counts = np.diff(off_h)
    den = w_obs + _like(counts.astype(np.float64), w_obs) * alpha
    rows = _like(np.repeat(np.arange(off_h.shape[0] - 1, dtype=np.int64), counts), w_obs)
    return (w_obs[rows] * th_s[:int(off_h[-1])] + alpha) / den[rows]


def smooth_theta_labels(th, w_obs, allowed, alpha):
    """``smooth_theta`` on label sets: (W_d * th + alpha) / (W_d + L_d * alpha) on the allowed columns (``allowed`` (D, K), non-zero =
    allowed; L_d = how many) and +0.0 elsewhere.  numpy arrays or torch tensors on one device."""
    on = allowed != 0
    tensors = not isinstance(th, np.ndarray)
    L = on.sum(1).to(th.dtype) if tensors else on.sum(1).astype(np.float64)
    full = (w_obs[:, None] * th + alpha) / (w_obs + L * alpha)[:, None]
    if tensors:
        import torch
        return torch.where(on, full, torch.zeros_like(full))
    return np.where(on, full, 0.0)


def _like(a, ref):
    """the numpy array a as ref is: a numpy array, or a tensor on ref's device"""
    if hasattr(ref, "device") and not isinstance(ref, np.ndarray):
        import torch
        return torch.from_numpy(a).to(ref.device)
    return a


_LN2 = math.log(2.0)


def doc_logliks(mant, expo):
    """ll_d = log(mant) + expo * ln 2, float64 [D]"""
    return np.log(np.asarray(mant, dtype=np.float64)) + np.asarray(expo, dtype=np.int64).astype(np.float64) * _LN2


def perplexity_from(mant, expo, tok, bad):
    """dict(perplexity, loglik, tokens, bad) of the per-document outputs: the document log-likelihoods added one after the other
    in document order (a plain float64 sum), perplexity = exp(-loglik / tokens); inf when a site of any document had no finite
    positive probability, nan when nothing was scored."""
    total = 0.0
    for x in doc_logliks(mant, expo).tolist():
        total += x
    tokens, n_bad = int(np.asarray(tok, dtype=np.int64).sum()), int(np.asarray(bad, dtype=np.int64).sum())
    if n_bad > 0:
        ppl = float("inf")
    elif tokens == 0:
        ppl = float("nan")
    else:
        ppl = float(np.exp(-total / tokens))
    return dict(perplexity=ppl, loglik=total, tokens=tokens, bad=n_bad)
