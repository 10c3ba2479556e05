"""Left-to-right held-out likelihood: a particle sampler on the device (``llda_left_to_right``, include/llda_gibbs.h).

The estimator of Wallach, Murray, Salakhutdinov and Mimno, "Evaluation methods for topic models" (ICML 2009), Algorithm 3: an
estimate of p(w_d | phi, alpha) itself -- the whole document, no split, comparable with what other LDA packages report (DESIGN.md
4.4f).  With the topics restricted to a document's own labels it is p(w_d | labels_d), the document likelihood of Labeled LDA.

A document is its TOKENS, one entry per occurrence in the text's order.  Scoring N tokens with R particles costs R N (N + 1) / 2
categorical draws over K topics; the kernel leaves the pair (mantissa, exponent), the scored and the bad tokens per document, which
``heldout.doc_logliks`` and ``heldout.perplexity_from`` turn into numbers.
"""
import numpy as np

from . import _native, docmodel

MAX_PARTICLES = _native.LR_MAX_PARTICLES
MAX_TOKENS = _native.LR_MAX_TOKENS
MAX_K = _native.LR_MAX_K
# default RNG stream id: particle r draws from LR_STREAM + r.  foldin.TEST_STREAM is 0x7E57 and the CASCADE_STREAM range starts at
# 0xC0DE0000 and grows by K * level + label id (far less than 2^16 * 2^13): the sixteen streams from 0x1E7F0000 meet neither.
LR_STREAM = 0x1E7F0000


def tokens_csr(token_id_lists):
    """token id lists, one per document in the text's order -> (doc_off int64 [D+1], word int32 [S])"""
    lens = [len(t) for t in token_id_lists]
    doc_off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=doc_off[1:])
    word = np.fromiter((int(w) for t in token_id_lists for w in t), dtype=np.int64, count=int(doc_off[-1]))
    if word.size and (word.min() < -2 ** 31 or word.max() >= 2 ** 31):
        raise ValueError("token ids must fit 32 bits")
    return doc_off, word.astype(np.int32)


def allowed_matrix(label_lists, labelmap, K):
    """uint8 (D, K): 1 where document d may use topic k -- the topics of its labels and column 0 ('root'), which the model gives
    every document (``labs[:, 0] = 1``).  A label the labelmap does not know raises KeyError."""
    out = np.zeros((len(label_lists), int(K)), dtype=np.uint8)
    out[:, 0] = 1
    for d, labs in enumerate(label_lists):
        for lab in labs:
            if lab not in labelmap:
                raise KeyError("document %d: unknown label %r" % (d, lab))
            k = int(labelmap[lab])
            if not 0 <= k < K:
                raise ValueError("label %r maps to topic %d, outside [0, %d)" % (lab, k, K))
            out[d, k] = 1
    return out


def prepare_tokens(token_id_lists, max_tokens=None):
    """the truncation and skip rules of ``LabeledLDA.left_to_right``: every list is cut to its first max_tokens entries (None: kept
    whole); a document with no token left, or with more than MAX_TOKENS, is skipped.  Returns (kept lists, their indices)."""
    if max_tokens is not None and int(max_tokens) < 1:
        raise ValueError("max_tokens must be at least 1")
    kept, index = [], []
    for d, t in enumerate(token_id_lists):
        t = list(t) if max_tokens is None else list(t[:int(max_tokens)])
        if 0 < len(t) <= MAX_TOKENS:
            kept.append(t)
            index.append(d)
    return kept, index


def loglik(phi_t_dev, doc_off, word, alpha, particles, seed, stream_id=LR_STREAM, allowed=None, doc_ids=None):
    """Score the token CSR doc_off (int64 [D+1]) / word against phi_t_dev (V, K), a float64 tensor on the device in reference topic
    order (any row stride >= K), with ``particles`` particles per document.  allowed: (D, K) uint8 (array or tensor) or None = every
    topic; doc_ids: int64 [D] or None = 0, 1, ...  Returns the per-document (mant, expo, tok, bad) as numpy arrays; a document
    longer than MAX_TOKENS raises."""
    import torch
    _native.lib()
    _native.require_device()
    x = docmodel.matrix(phi_t_dev, "phi_t")
    dev = x.device
    V, K = int(x.shape[0]), int(x.shape[1])
    if not 1 <= int(particles) <= MAX_PARTICLES:
        raise ValueError("particles must be in 1 .. %d" % MAX_PARTICLES)

    off_h, D, S = docmodel.check_offsets(doc_off)
    longest = int(np.diff(off_h).max()) if D else 0
    if longest > MAX_TOKENS:
        raise ValueError("a document holds %d tokens, more than %d" % (longest, MAX_TOKENS))
    d_off, d_word, _ = docmodel.stage(dev, off_h, word, None, S, unit="tokens")
    d_allowed = None
    if allowed is not None:
        d_allowed = docmodel.on_dev(allowed, torch.uint8, dev)
        if tuple(d_allowed.shape) != (D, K):
            raise ValueError("allowed must be (D, K) = (%d, %d)" % (D, K))
    d_ids = None
    if doc_ids is not None:
        d_ids = docmodel.on_dev(doc_ids, torch.int64, dev)
        if int(d_ids.numel()) != D:
            raise ValueError("doc_ids must hold D = %d ids" % D)
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _native.left_to_right(d_off, d_word, x, D, V, K, particles=int(particles), alpha=float(alpha), seed=seed, stream_id=stream_id,
                          max_doc_tokens=max(1, longest), mant=mant, expo=expo, tok=tok, bad=bad,
                          ld_phi=int(x.stride(0)) if V > 1 else K, allowed=d_allowed, ld_allowed=K, doc_ids=d_ids, status=status)
    out = mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy()
    if int(status.item()) & 1:
        raise _native.NativeError("llda_left_to_right: a document was longer than the launch allowed")
    return out


def loglik_sparse(phi_t_dev, doc_off, word, lab_off, lab, alpha, particles, seed, stream_id=LR_STREAM, doc_ids=None):
    """``loglik`` with every document's topics restricted to its own label list (``llda_left_to_right_sparse``): the
    lists are the CSR lab_off (int64 [D+1]) / lab (``docmodel.label_csr``: ids ascending, at most 32 per document).  A draw touches
    len(labels) entries of the word's row of phi_t_dev (V, K), whatever K is -- K may be anything up to the library's limit, not
    1024.  The result is that of ``loglik`` on the document's own columns of phi_t.  Returns the per-document (mant, expo, tok,
    bad); ValueError on the host, before any launch, for label sets the kernel would call unfit."""
    import torch
    _native.lib()
    _native.require_device()
    x = docmodel.matrix(phi_t_dev, "phi_t")
    dev = x.device
    V, K = int(x.shape[0]), int(x.shape[1])
    if not 1 <= int(particles) <= MAX_PARTICLES:
        raise ValueError("particles must be in 1 .. %d" % MAX_PARTICLES)
    off_h, D, S = docmodel.check_offsets(doc_off)
    loff_h, lab_h, NL, max_labels = docmodel.label_sets(lab_off, lab, D, K)
    longest = int(np.diff(off_h).max()) if D else 0
    if longest > MAX_TOKENS:
        raise ValueError("a document holds %d tokens, more than %d" % (longest, MAX_TOKENS))
    d_off, d_word, _ = docmodel.stage(dev, off_h, word, None, S, unit="tokens")
    d_loff, d_lab = docmodel.on_dev(loff_h, torch.int64, dev), docmodel.on_dev(lab_h if NL else np.zeros(1), torch.int32, dev)
    d_ids = None
    if doc_ids is not None:
        d_ids = docmodel.on_dev(doc_ids, torch.int64, dev)
        if int(d_ids.numel()) != D:
            raise ValueError("doc_ids must hold D = %d ids" % D)
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    _native.left_to_right_sparse(d_off, d_word, x, d_loff, d_lab, D, V, K, NL, max_labels, particles=int(particles), alpha=float(alpha),
                                 seed=seed, stream_id=stream_id, max_doc_tokens=max(1, longest), mant=mant, expo=expo, tok=tok, bad=bad,
                                 ld_phi=int(x.stride(0)) if V > 1 else K, doc_ids=d_ids, status=status)
    out = mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy()
    if int(status.item()) & 1:
        raise _native.NativeError("llda_left_to_right_sparse: a document was longer than the launch allowed")
    return out
