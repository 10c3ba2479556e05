"""Deterministic EM training on the device (``llda_credit_words``, ``llda_phi_step``, include/llda_gibbs.h).

``attribution.attribute`` is the E-step of the document model with the theta M-step: it adds a site's label shares

    r[k] = theta[d][k] * phi_t[w][k] / p,        p = sum_k theta[d][k] * phi_t[w][k]

(times f) to the site's DOCUMENT.  ``credit_words`` adds the same shares to the site's WORD: ``cw[w][k]``, the expected n_kw of the
corpus under the model, and ``phi_step`` is the phi M-step on it, ``phi_t[w][k] = (cw[w][k] + beta) / (sum_w cw[w][k] + V beta)``.
One iteration of ``fit`` is the three of them; each half is an exact M-step on its block, so the MAP objective

    sum f log p + alpha sum_{theta > 0} log theta + beta sum log phi

never falls.  No random numbers and no floating-point atomics: the same start gives the same bits on every call.  A load that
starts at 0 stays 0 -- that is how the label sets enter.

The word side walks the sites WORD-major (``word_major``): within a word in ascending document order.  A word's run is cut into
chunks of ``chunk`` sites, one wavefront each; the order of the sum, and so the last bits of the result, depend on ``chunk`` and on
nothing else.
"""
import numpy as np

from . import _native, docmodel

MAX_FREQ = _native.HELDOUT_MAX_FREQ
DEFAULT_CHUNK = 4096


def word_major(doc_off, word, freq, V, device):
    """The sites of the CSR doc_off (int64 [D+1]) / word / freq (numpy arrays or tensors; freq None: all 1) in word-major order, built
    on ``device`` with a stable sort by word id: (word_off int64 [V+1], site_doc int32 [S], freq int32 [S] or None, order int64 [S]).
    ``order[i]`` is the document-major site that became word-major site i; within a word the sites are in ascending document order,
    then in site order.  The word ids must be in [0, V)."""
    import torch
    _native.require_device()
    V = int(V)
    if V < 1:
        raise ValueError("V must be at least 1")
    off_h, D, S = docmodel.check_offsets(doc_off)
    d_off, d_word, d_freq = docmodel.stage(device, doc_off, word, freq, S, V)
    d_word = d_word[:S].to(torch.int64)
    order = torch.sort(d_word, stable=True).indices
    lens = d_off[1:] - d_off[:-1]
    site_doc = torch.repeat_interleave(torch.arange(D, dtype=torch.int32, device=d_off.device), lens, output_size=S)
    word_off = torch.zeros((V + 1,), dtype=torch.int64, device=d_off.device)
    if S:
        word_off[1:] = torch.cumsum(torch.bincount(d_word, minlength=V), 0)
    return word_off, site_doc[order].contiguous(), None if d_freq is None else d_freq[:S][order].contiguous(), order


def _check_chunk(chunk):
    chunk = int(chunk)
    if not 1 <= chunk <= 2 ** 31 - 1:
        raise ValueError("chunk must be in 1 .. 2^31 - 1")
    return chunk


def credit_words(theta, phi_t, word_off, site_doc, freq, chunk=DEFAULT_CHUNK, want=("credit", "tok", "bad")):
    """The word side of the E-step: theta (D, K) and phi_t (V, K) float64 tensors on the device (reference topic order, any row
    stride >= K) against the word-major sites word_off (int64 [V+1]) / site_doc / freq (``word_major``; numpy arrays or tensors,
    freq None: all 1).  Returns a dict of device tensors, the ones ``want`` names: credit (V, K) float64, tok, bad (int64 [V]).
    ValueError on the host, before any launch, for shapes that do not fit."""
    import torch
    _native.lib()
    _native.require_device()
    theta, phi_t, D, V, K = docmodel.matrices(theta, phi_t)
    dev = phi_t.device
    chunk = _check_chunk(chunk)
    want = tuple(want)
    if set(want) - {"credit", "tok", "bad"}:
        raise ValueError("want: unknown output %s" % sorted(set(want) - {"credit", "tok", "bad"}))
    _, _, S = docmodel.check_offsets(word_off, V)
    d_off, d_doc, d_freq = docmodel.stage(dev, word_off, site_doc, freq, S, unit="sites")
    if S and D and (int(d_doc[:S].min()) < 0 or int(d_doc[:S].max()) >= D):
        raise ValueError("document ids must be in [0, D)")
    if S and not D:
        raise ValueError("there are sites and no document")
    out = {}
    if "credit" in want:
        out["credit"] = torch.empty((V, K), dtype=torch.float64, device=dev)
    for name in ("tok", "bad"):
        if name in want:
            out[name] = torch.empty((V,), dtype=torch.int64, device=dev)
    scratch = torch.empty((_native.credit_words_scratch_bytes(V, S, K, chunk),), dtype=torch.uint8, device=dev) if S else None
    _native.credit_words(d_off, d_doc, d_freq, theta, phi_t, D, V, S, K, chunk, scratch,
                         ld_theta=int(theta.stride(0)) if D > 1 else K, ld_phi=int(phi_t.stride(0)) if V > 1 else K, ld_credit=K,
                         credit_w=out.get("credit"), tok=out.get("tok"), bad=out.get("bad"))
    return out


def credit_words_sparse(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk=DEFAULT_CHUNK, want=("credit", "tok", "bad")):
    """``credit_words`` for documents that carry a few of the K labels (``llda_credit_words_sparse``): the label sets
    are the CSR lab_off (int64 [D+1]) / lab (``docmodel.label_csr``), theta_s (float64 [NL], on the device) the loads per slot.
    Returns the same dict: credit (V, K) float64 dense rows, tok, bad (int64 [V]).  ValueError on the host, before any launch, for
    shapes that do not fit and for label sets the kernel would call unfit."""
    import torch
    from . import attribution
    _native.lib()
    _native.require_device()
    phi_t = docmodel.matrix(phi_t, "phi_t")
    V, K = int(phi_t.shape[0]), int(phi_t.shape[1])
    dev = phi_t.device
    chunk = _check_chunk(chunk)
    want = tuple(want)
    if set(want) - {"credit", "tok", "bad"}:
        raise ValueError("want: unknown output %s" % sorted(set(want) - {"credit", "tok", "bad"}))
    _, D, _ = docmodel.check_offsets(lab_off)
    off_h, lab_h, NL, max_labels = docmodel.label_sets(lab_off, lab, D, K)
    theta_s = attribution._slots(theta_s, NL, dev, "theta_s")
    _, _, S = docmodel.check_offsets(word_off, V)
    d_off, d_doc, d_freq = docmodel.stage(dev, word_off, site_doc, freq, S, unit="sites")
    if S and D and (int(d_doc[:S].min()) < 0 or int(d_doc[:S].max()) >= D):
        raise ValueError("document ids must be in [0, D)")
    if S and not D:
        raise ValueError("there are sites and no document")
    d_loff, d_lab = docmodel.on_dev(off_h, torch.int64, dev), docmodel.on_dev(lab_h if NL else np.zeros(1), torch.int32, dev)
    out = {}
    if "credit" in want:
        out["credit"] = torch.empty((V, K), dtype=torch.float64, device=dev)
    for name in ("tok", "bad"):
        if name in want:
            out[name] = torch.empty((V,), dtype=torch.int64, device=dev)
    scratch = torch.empty((_native.credit_words_sparse_scratch_bytes(V, S, K, chunk),), dtype=torch.uint8, device=dev) if S else None
    _native.credit_words_sparse(d_off, d_doc, d_freq, d_loff, d_lab, theta_s, phi_t, D, V, S, K, NL, max_labels, chunk, scratch,
                                ld_phi=int(phi_t.stride(0)) if V > 1 else K, ld_credit=K, credit_w=out.get("credit"), tok=out.get("tok"),
                                bad=out.get("bad"))
    return out


def phi_step(cw, beta, out=None, want_den=False):
    """The phi M-step: cw (V, K) float64 on the device, the word credit -> phi_t (V, K) = (cw + beta) / (column sums + V beta).
    ``out``: where to (a (V, K) float64 tensor on the same device; it may be cw itself); None: a new tensor.  want_den: return
    (phi_t, den [K]) instead."""
    import torch
    _native.lib()
    _native.require_device()
    cw = docmodel.matrix(cw, "cw")
    V, K = int(cw.shape[0]), int(cw.shape[1])
    beta = float(beta)
    if not (beta > 0.0 and beta < float("inf")):
        raise ValueError("beta must be a finite number above 0")
    if V < 1 or K < 1:
        raise ValueError("cw must have at least one row and one column")
    if out is None:
        out = torch.empty((V, K), dtype=torch.float64, device=cw.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float64 and out.device == cw.device and tuple(out.shape) == (V, K)
              and out.stride(1) == 1 and (V == 1 or out.stride(0) >= K)):
        raise ValueError("out must be a (V, K) float64 tensor on cw's device with unit column stride")
    den = torch.empty((K,), dtype=torch.float64, device=cw.device) if want_den else None
    scratch = torch.empty((_native.phi_step_scratch_bytes(V, K),), dtype=torch.uint8, device=cw.device)
    _native.phi_step(cw, V, K, beta, out, scratch, ld=int(cw.stride(0)) if V > 1 else K, ld_out=int(out.stride(0)) if V > 1 else K, den=den)
    return (out, den) if want_den else out


def fit(theta0, phi_t0, doc_off, word, freq, alpha, beta, iters, theta_steps=1, chunk=DEFAULT_CHUNK, trace_every=0):
    """EM training from the loads theta0 (D, K) and phi_t0 (V, K), float64 tensors on the device, on the CSR doc_off / word / freq
    (numpy arrays or tensors; freq None: all 1).  One iteration: theta = ``attribution.attribute(theta, phi_t, iters=theta_steps,
    alpha)``; cw = ``credit_words(theta, phi_t)``; phi_t = ``phi_step(cw, beta)``.  trace_every = n > 0: after the iterations n,
    2 n, ... the data term sum f log p of the training sites (``heldout.loglik``, the logarithm on the host) is recorded as
    (iteration, loglik, tokens, bad).  Returns dict(theta (D, K), phi_t (V, K) device tensors, iterations, trace)."""
    import torch
    from . import heldout
    _native.lib()
    _native.require_device()
    theta, phi_t, D, V, K = docmodel.matrices(theta0, phi_t0)
    dev = theta.device
    iters, theta_steps, trace_every, chunk = int(iters), int(theta_steps), int(trace_every), _check_chunk(chunk)
    alpha, beta = float(alpha), float(beta)
    if iters < 0 or theta_steps < 1 or trace_every < 0:
        raise ValueError("iters >= 0, theta_steps >= 1 and trace_every >= 0 are wanted")
    if not alpha >= 0.0:
        raise ValueError("alpha must not be negative")
    if not (beta > 0.0 and beta < float("inf")):
        raise ValueError("beta must be a finite number above 0")
    _, _, S = docmodel.check_offsets(doc_off, D)
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq, S, V)
    word_off, site_doc, w_freq, _ = word_major(d_off, d_word, d_freq, V, dev)
    theta, phi_t = theta.contiguous().clone(), phi_t.contiguous().clone()           # (row stride K from here on)
    spare = torch.empty_like(theta)
    cw = torch.empty((V, K), dtype=torch.float64, device=dev)
    scratch = torch.empty((max(_native.credit_words_scratch_bytes(V, S, K, chunk), _native.phi_step_scratch_bytes(V, K)),),
                          dtype=torch.uint8, device=dev)
    trace = []
    for it in range(1, iters + 1):
        if D:
            _native.attribute(d_off, d_word, d_freq, theta, phi_t, D, V, K, iters=theta_steps, alpha=alpha, top_m=0, ld_theta=K,
                              ld_phi=K, ld_out=K, theta_out=spare)
            theta, spare = spare, theta
        _native.credit_words(word_off, site_doc, w_freq, theta, phi_t, D, V, S, K, chunk, scratch if S else None,
                             ld_theta=K, ld_phi=K, ld_credit=K, credit_w=cw)
        _native.phi_step(cw, V, K, beta, phi_t, scratch, ld=K, ld_out=K)
        if trace_every and it % trace_every == 0:
            r = heldout.perplexity_from(*heldout.loglik(theta, phi_t, d_off, d_word, d_freq))
            trace.append((it, r["loglik"], r["tokens"], r["bad"]))
    return dict(theta=theta, phi_t=phi_t, iterations=iters, trace=trace)


def fit_sparse(theta_s0, phi_t0, doc_off, word, freq, lab_off, lab, alpha, beta, iters, theta_steps=1, chunk=DEFAULT_CHUNK, trace_every=0,
               sparse_trace=False):
    """``fit`` for documents that carry a few of the K labels: the same loop on ``llda_attribute_sparse`` and
    ``llda_credit_words_sparse`` plus the unchanged ``phi_step``.  theta_s0 (float64 [NL], on the device) holds the start loads per
    slot of the label CSR lab_off / lab (``docmodel.label_csr``); phi_t0 is (V, K).  A site costs len(labels) gathered entries on
    either side, whatever K is.  The trace is ``heldout.loglik`` on the loads scattered to (D, K); sparse_trace=True:
    ``heldout.loglik_sparse`` on the slots themselves (no (D, K) matrix; its sums pair by slot, so the figures differ from the
    default's in their last bits).  Returns dict(theta_s [NL], phi_t (V, K), theta (D, K): theta_s scattered, +0.0 outside the
    label sets; iterations, trace)."""
    import torch
    from . import attribution, heldout
    _native.lib()
    _native.require_device()
    phi_t = docmodel.matrix(phi_t0, "phi_t")
    V, K = int(phi_t.shape[0]), int(phi_t.shape[1])
    dev = phi_t.device
    iters, theta_steps, trace_every, chunk = int(iters), int(theta_steps), int(trace_every), _check_chunk(chunk)
    alpha, beta = float(alpha), float(beta)
    if iters < 0 or theta_steps < 1 or trace_every < 0:
        raise ValueError("iters >= 0, theta_steps >= 1 and trace_every >= 0 are wanted")
    if not alpha >= 0.0:
        raise ValueError("alpha must not be negative")
    if not (beta > 0.0 and beta < float("inf")):
        raise ValueError("beta must be a finite number above 0")
    _, D, S = docmodel.check_offsets(doc_off)
    off_h, lab_h, NL, max_labels = docmodel.label_sets(lab_off, lab, D, K)
    theta_s = attribution._slots(theta_s0, NL, dev, "theta_s0").clone()
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq, S, V)
    word_off, site_doc, w_freq, _ = word_major(d_off, d_word, d_freq, V, dev)
    d_loff, d_lab = docmodel.on_dev(off_h, torch.int64, dev), docmodel.on_dev(lab_h if NL else np.zeros(1), torch.int32, dev)
    phi_t = phi_t.contiguous().clone()                                              # (row stride K from here on)
    spare = torch.empty_like(theta_s)
    cw = torch.empty((V, K), dtype=torch.float64, device=dev)
    scratch = torch.empty((max(_native.credit_words_sparse_scratch_bytes(V, S, K, chunk), _native.phi_step_scratch_bytes(V, K)),),
                          dtype=torch.uint8, device=dev)
    trace = []
    for it in range(1, iters + 1):
        if D:
            _native.attribute_sparse(d_off, d_word, d_freq, d_loff, d_lab, theta_s, phi_t, D, V, K, NL, max_labels, iters=theta_steps,
                                     alpha=alpha, top_m=0, ld_phi=K, theta_out=spare)
            theta_s, spare = spare, theta_s
        _native.credit_words_sparse(word_off, site_doc, w_freq, d_loff, d_lab, theta_s, phi_t, D, V, S, K, NL, max_labels, chunk,
                                    scratch if S else None, ld_phi=K, ld_credit=K, credit_w=cw)
        _native.phi_step(cw, V, K, beta, phi_t, scratch, ld=K, ld_out=K)
        if trace_every and it % trace_every == 0:
            if sparse_trace:
                r = heldout.perplexity_from(*heldout.loglik_sparse(theta_s, phi_t, d_off, d_word, d_freq, off_h, lab_h))
            else:
                r = heldout.perplexity_from(*heldout.loglik(attribution.scatter_slots(theta_s, off_h, lab_h, K), phi_t, d_off, d_word, d_freq))
            trace.append((it, r["loglik"], r["tokens"], r["bad"]))
    return dict(theta_s=theta_s[:NL], phi_t=phi_t, theta=attribution.scatter_slots(theta_s, off_h, lab_h, K), iterations=iters, trace=trace)
