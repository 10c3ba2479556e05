"""Credit attribution and the deterministic EM fold-in on the device (``llda_attribute``, include/llda_gibbs.h).

Labeled LDA was introduced for credit attribution: which words of a document belong to which of its labels.  With the loads
``theta`` of a document fixed, the E-step of the document model answers it: a site (w, f) has

    p = sum_k theta[k] * phi[k][w],        r[k] = theta[k] * phi[k][w] / p        (the word's posterior share per label)

and the document's credit is ``credit[k] = sum_sites f * r[k]``, the tokens each label accounts for.  Iterated with the matching
M-step ``theta[k] = (credit[k] + alpha) / sum`` over the labels whose load is not 0, the same kernel is a fold-in without random
numbers: the same document gets the same loads, always.  A label set is expressed by the start row: 0 outside the set
(``uniform_start``), and a load that is 0 stays 0.

The kernel reads the whole row of ``phi_t`` for every site even where ``theta`` is sparse; ``attribute_sparse`` takes the label sets
as a CSR and reads a document's own columns only.  A site whose p is below 2^-960 or not finite (or whose word is unknown) is
attributed to nobody and counted in ``bad``.
"""
import numpy as np

from . import _native, docmodel

MAX_FREQ = _native.HELDOUT_MAX_FREQ
MAX_TOP = _native.ATTR_MAX_TOP
OUTPUTS = ("theta", "credit", "sites", "tok", "bad")


def uniform_start(label_cols, D, K):
    """The start rows (D, K) float64: 1 / n on the n allowed columns of every document and 0 elsewhere.  ``label_cols`` is None
    (every label allowed: 1 / K everywhere) or one sequence of column indices per document (duplicates count once)."""
    D, K = int(D), int(K)
    if label_cols is None:
        return np.full((D, K), np.float64(1.0) / np.float64(K))
    if len(label_cols) != D:
        raise ValueError("label_cols must hold one list of columns per document")
    out = np.zeros((D, K), dtype=np.float64)
    for d, cols in enumerate(label_cols):
        c = np.unique(np.asarray(list(cols), dtype=np.int64))
        if c.size == 0 or c[0] < 0 or c[-1] >= K:
            raise ValueError("document %d: label columns must be a non-empty subset of 0 .. K-1" % d)
        out[d, c] = np.float64(1.0) / np.float64(c.size)
    return out


def explain_label_cols(labelmap, D, labels=None, ranked=None, n=3):
    """The label set of every document that ``LabeledLDA.explain`` fits: column 0 ('root') plus the given labels (``labels``: one
    list of label strings per document; an unknown label is a KeyError, as in ``set_label``), or plus the first n <= 3 non-root
    columns of ``ranked`` (D, >= n) topic ids, best first, -1 = padding.  Columns ascending, root first."""
    if labels is not None:
        if len(labels) != D:
            raise ValueError("labels must hold one list per document")
        return [[0] + sorted(set(int(labelmap[x]) for x in lab) - {0}) for lab in labels]
    if not 1 <= int(n) <= 3:
        raise ValueError("n must be in 1 .. 3 (at most four labels per site: root and three)")
    if ranked is None or len(ranked) != D:
        raise ValueError("ranked must hold one row of topic ids per document")
    return [[0] + sorted([int(k) for k in row if int(k) >= 1][:int(n)]) for row in ranked]


def attribute(theta_dev, phi_t_dev, doc_off, word, freq, iters=0, alpha=0.0, top_m=1, want=OUTPUTS):
    """Attribute the sites of the CSR doc_off (int64 [D+1]) / word / freq (numpy arrays or device tensors; freq None: all 1) against
    theta_dev (D, K), the start loads, and phi_t_dev (V, K): float64 tensors on the device in reference topic order (any row stride
    >= K).  iters EM steps with alpha come first (0: theta as it is).  Returns a dict of device tensors, the ones ``want`` names:
    theta (D, K) the final loads, credit (D, K), site_idx (S, top_m) int32 / site_val (S, top_m) float64 (for "sites"; -1 / 0.0
    padding), tok, bad (int64 [D])."""
    import torch
    _native.lib()
    _native.require_device()
    theta_dev, phi_t_dev, D, V, K = docmodel.matrices(theta_dev, phi_t_dev)
    dev = theta_dev.device
    iters, top_m, alpha = int(iters), int(top_m), float(alpha)
    if iters < 0:
        raise ValueError("iters must not be negative")
    if not alpha >= 0.0:
        raise ValueError("alpha must not be negative")
    if not 0 <= top_m <= MAX_TOP:
        raise ValueError("top_m must be in 0 .. %d" % MAX_TOP)
    want = tuple(want)
    if set(want) - set(OUTPUTS):
        raise ValueError("want: unknown output %s" % sorted(set(want) - set(OUTPUTS)))

    _, _, S = docmodel.check_offsets(doc_off, D)
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq, S, V)
    out = {}
    if "theta" in want:
        out["theta"] = torch.empty((D, K), dtype=torch.float64, device=dev)
    if "credit" in want:
        out["credit"] = torch.empty((D, K), dtype=torch.float64, device=dev)
    if "sites" in want and top_m > 0:
        out["site_idx"] = torch.empty((S, top_m), dtype=torch.int32, device=dev)
        out["site_val"] = torch.empty((S, top_m), dtype=torch.float64, device=dev)
    for name in ("tok", "bad"):
        if name in want:
            out[name] = torch.empty((D,), dtype=torch.int64, device=dev)
    _native.attribute(d_off, d_word, d_freq, theta_dev, phi_t_dev, D, V, K, iters=iters, alpha=alpha,
                      top_m=top_m if "site_idx" in out else 0,
                      ld_theta=int(theta_dev.stride(0)) if D > 1 else K, ld_phi=int(phi_t_dev.stride(0)) if V > 1 else K,
                      ld_out=K, ld_credit=K, theta_out=out.get("theta"), credit=out.get("credit"), site_idx=out.get("site_idx"),
                      site_val=out.get("site_val"), tok=out.get("tok"), bad=out.get("bad"))
    return out


def _slots(x, NL, dev, name):
    """x must be a float64 tensor of NL loads at least on dev; returned contiguous"""
    import torch
    if not (isinstance(x, torch.Tensor) and x.dtype == torch.float64 and x.dim() == 1 and x.device == dev and int(x.numel()) >= NL):
        raise ValueError("%s must be a float64 tensor of %d loads (one per slot of lab) on phi_t's device" % (name, NL))
    return x.contiguous() if NL else torch.zeros((1,), dtype=torch.float64, device=dev)


def attribute_sparse(theta_s, phi_t_dev, doc_off, word, freq, lab_off, lab, iters=0, alpha=0.0, top_m=1, want=OUTPUTS):
    """``attribute`` for documents that carry a few of the K labels (``llda_attribute_sparse``): the label sets are
    the CSR lab_off (int64 [D+1]) / lab (ids ascending inside a document; ``docmodel.label_csr``), theta_s (float64 [NL], on the
    device) holds the start loads per slot of lab.  A site reads len(labels) entries of its word's row of phi_t, not K.  Returns a dict
    of device tensors, the ones ``want`` names: theta and credit float64 [NL] per slot, site_idx (label ids) / site_val (S, top_m),
    tok, bad (int64 [D]).  ValueError on the host, before any launch, for label sets the kernel would call unfit."""
    import torch
    _native.lib()
    _native.require_device()
    phi_t_dev = docmodel.matrix(phi_t_dev, "phi_t")
    V, K = int(phi_t_dev.shape[0]), int(phi_t_dev.shape[1])
    dev = phi_t_dev.device
    iters, top_m, alpha = int(iters), int(top_m), float(alpha)
    if iters < 0:
        raise ValueError("iters must not be negative")
    if not alpha >= 0.0:
        raise ValueError("alpha must not be negative")
    if not 0 <= top_m <= MAX_TOP:
        raise ValueError("top_m must be in 0 .. %d" % MAX_TOP)
    want = tuple(want)
    if set(want) - set(OUTPUTS):
        raise ValueError("want: unknown output %s" % sorted(set(want) - set(OUTPUTS)))
    _, D, S = docmodel.check_offsets(doc_off)
    off_h, lab_h, NL, max_labels = docmodel.label_sets(lab_off, lab, D, K)
    theta_s = _slots(theta_s, NL, dev, "theta_s")
    d_off, d_word, d_freq = docmodel.stage(dev, doc_off, word, freq, S, V)
    d_loff, d_lab = docmodel.on_dev(off_h, torch.int64, dev), docmodel.on_dev(lab_h if NL else np.zeros(1), torch.int32, dev)
    out = {}
    for name in ("theta", "credit"):
        if name in want:
            out[name] = torch.empty((NL,), dtype=torch.float64, device=dev)
    if "sites" in want and top_m > 0:
        out["site_idx"] = torch.empty((S, top_m), dtype=torch.int32, device=dev)
        out["site_val"] = torch.empty((S, top_m), dtype=torch.float64, device=dev)
    for name in ("tok", "bad"):
        if name in want:
            out[name] = torch.empty((D,), dtype=torch.int64, device=dev)
    _native.attribute_sparse(d_off, d_word, d_freq, d_loff, d_lab, theta_s, phi_t_dev, D, V, K, NL, max_labels, iters=iters, alpha=alpha,
                             top_m=top_m if "site_idx" in out else 0, ld_phi=int(phi_t_dev.stride(0)) if V > 1 else K,
                             theta_out=out.get("theta"), credit=out.get("credit"), site_idx=out.get("site_idx"),
                             site_val=out.get("site_val"), tok=out.get("tok"), bad=out.get("bad"))
    return out


def scatter_slots(values, lab_off, lab, K):
    """per-slot values (float64 [NL], device) -> the dense (D, K) rows, +0.0 outside the label sets; lab_off / lab host arrays"""
    import torch
    off_h = np.asarray(lab_off, dtype=np.int64)
    D, NL = off_h.shape[0] - 1, int(off_h[-1]) if off_h.shape[0] else 0
    out = torch.zeros((D, int(K)), dtype=torch.float64, device=values.device)
    if NL:
        rows = torch.from_numpy(np.repeat(np.arange(D, dtype=np.int64), np.diff(off_h))).to(values.device)
        cols = torch.from_numpy(np.asarray(lab, dtype=np.int64)[:NL]).to(values.device)
        out[rows, cols] = values[:NL]
    return out


def gather_slots(dense, lab_off, lab):
    """the dense (D, K) rows (float64, device) -> their entries at the label sets, float64 [NL]"""
    import torch
    off_h = np.asarray(lab_off, dtype=np.int64)
    D, NL = off_h.shape[0] - 1, int(off_h[-1])
    rows = torch.from_numpy(np.repeat(np.arange(D, dtype=np.int64), np.diff(off_h))).to(dense.device)
    cols = torch.from_numpy(np.asarray(lab, dtype=np.int64)[:NL]).to(dense.device)
    return dense[rows, cols].contiguous()


def spans(doc_off, site_idx, site_val):
    """The host shaping of the per-site outputs: (S, top_m) arrays -> two lists with one (len(doc), top_m) array per document."""
    off = np.asarray(doc_off, dtype=np.int64)
    idx, val = np.asarray(site_idx), np.asarray(site_val)
    pairs = list(zip(off[:-1].tolist(), off[1:].tolist()))
    return [idx[a:b] for a, b in pairs], [val[a:b] for a, b in pairs]


def explanations(doc_tups, site_idx, site_val, credit, names, id2token):
    """Per document ([(token, f, [(label, share), ...])], {label: credited tokens}): the sites of doc_tups (one doc2bow list per
    document) with their best labels (padding left out) and the document's credit over the labels that got any."""
    off = np.concatenate([[0], np.cumsum([len(t) for t in doc_tups])]).astype(np.int64)
    idx, val = spans(off, site_idx, site_val)
    out = []
    for d, tups in enumerate(doc_tups):
        words = [(id2token[int(w)], int(f), [(names[int(k)], float(r)) for k, r in zip(idx[d][s], val[d][s]) if k >= 0])
                 for s, (w, f) in enumerate(tups)]
        out.append((words, {names[int(k)]: float(credit[d, k]) for k in np.flatnonzero(credit[d] > 0.0)}))
    return out
