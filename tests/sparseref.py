"""CPU restatement of llda_attribute_sparse and llda_credit_words_sparse (include/llda_gibbs.h) and of emfit.fit_sparse, written from
the header on the pieces of attrref.py / emref.py: numpy float64 operations, each rounded on its own.

    sets     lab_off [D+1], lab [NL]: the labels of document d are the slots lab_off[d] .. lab_off[d+1]; loads, new loads and credit
             live per slot.  UNFIT: more than max_labels slots, offsets outside [0, NL], an id outside [0, K), ids that do not
             ascend strictly.  The ids of an unfit document are never used.
    site     t_j = theta_s[j] * phi_t[w][lab[j]] over the document's slots; p = sum64(t) in slot order; everything after that is
             attrref.estep on the compacted problem (K' = L_d), with lab[j] in site_idx where that problem has j
    unfit    document side: every site adds f to bad, tok = 0, its slots keep theta_s and get credit +0.0; word side: its sites
             are not ok
    word     acc[lab[j]] = acc[lab[j]] + t_j * g, emref's chunks and their order; columns nobody reaches stay +0.0
"""
import numpy as np

import attrref
import emref

MIN_P = attrref.MIN_P
MAX_LABELS = 32


def doc_fit(lab_off, lab, d, K, max_labels, NL=None):
    """(fit, inside, lb, L) of document d"""
    NL = len(lab) if NL is None else NL
    lb, L = int(lab_off[d]), int(lab_off[d + 1]) - int(lab_off[d])
    inside = lb >= 0 and L >= 0 and lb + L <= NL
    if not inside or L > max_labels:
        return False, inside, lb, L
    ids = np.asarray(lab[lb:lb + L], dtype=np.int64)
    fit = bool(((ids >= 0) & (ids < K)).all() and (np.diff(ids) > 0).all())
    return fit, inside, lb, L


def attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=None, V=None, max_labels=MAX_LABELS, iters=0, alpha=0.0,
                         top_m=0):
    """theta_s [NL], phi_t (V, >= K); the sites doc_off / word / freq (None: all 1); the label sets lab_off / lab -> dict(theta_out
    [NL], credit [NL], site_idx (S, top_m) int32 label ids, site_val (S, top_m), tok, bad int64 [D]).  Slots that no document
    owns keep NaN in theta_out / credit (the kernel does not write them)."""
    D = len(doc_off) - 1
    K = phi_t.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    S, NL = int(doc_off[-1]), len(lab)
    theta_s = np.asarray(theta_s, dtype=np.float64)
    out = dict(theta_out=np.full(NL, np.nan), credit=np.full(NL, np.nan), site_idx=np.full((S, top_m), -1, dtype=np.int32),
               site_val=np.zeros((S, top_m)), tok=np.zeros(D, dtype=np.int64), bad=np.zeros(D, dtype=np.int64))
    for d in range(D):
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        fs = [1] * (e - b) if freq is None else [int(x) for x in freq[b:e]]
        fit, inside, lb, L = doc_fit(lab_off, lab, d, K, max_labels, NL)
        if not fit:
            out["bad"][d] = sum(fs)
            if inside:
                out["theta_out"][lb:lb + L] = theta_s[lb:lb + L]
                out["credit"][lb:lb + L] = 0.0
            continue
        if L == 0:                                                         # fit, p = 0 at every site, no slot
            out["bad"][d] = sum(fs)
            continue
        ids = np.asarray(lab[lb:lb + L], dtype=np.int64)
        sub = np.ascontiguousarray(phi_t[:V][:, ids])                      # phi_t'[w][j] = phi_t[w][lab[j]]
        r = attrref.attribute_ref(theta_s[None, lb:lb + L], sub, np.array([0, e - b], dtype=np.int64), word[b:e],
                                  None if freq is None else freq[b:e], K=L, V=V, iters=iters, alpha=alpha, top_m=top_m)
        out["theta_out"][lb:lb + L], out["credit"][lb:lb + L] = r["theta_out"][0], r["credit"][0]
        out["tok"][d], out["bad"][d] = r["tok"][0], r["bad"][0]
        out["site_idx"][b:e] = np.where(r["site_idx"] >= 0, ids[np.maximum(r["site_idx"], 0)], -1)
        out["site_val"][b:e] = r["site_val"]
    return out


def chunk_sum_sparse(theta_s, prow, docs, fs, sets, K):
    """one chunk: (sum [K], tok, bad); sets = (lab_off, lab, fit [D] bools)"""
    lab_off, lab, fit = sets
    D = len(lab_off) - 1
    acc = np.zeros(K, dtype=np.float64)
    tok = bad = 0
    with np.errstate(all="ignore"):
        for d, f in zip(docs, fs):
            d, f = int(d), int(f)
            if not (0 <= d < D and fit[d]):
                bad += f
                continue
            lb, le = int(lab_off[d]), int(lab_off[d + 1])
            ids = np.asarray(lab[lb:le], dtype=np.int64)
            t = theta_s[lb:le] * prow[ids]
            p = attrref.sum64(t[None, :])[0]
            if not (p >= MIN_P and p < np.inf):
                bad += f
                continue
            tok += f
            inv = np.float64(1.0) / p
            g = np.float64(f) * inv
            acc[ids] = acc[ids] + t * g
    return acc, tok, bad


def credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, freq, lab_off, lab, chunk, K=None, max_labels=MAX_LABELS):
    """theta_s [NL], phi_t (V, >= K); word-major sites word_off / site_doc / freq (None: all 1) -> dict(credit (V, K), tok, bad [V])"""
    V = len(word_off) - 1
    K = phi_t.shape[1] if K is None else K
    D = len(lab_off) - 1
    theta_s = np.asarray(theta_s, dtype=np.float64)
    fit = [doc_fit(lab_off, lab, d, K, max_labels)[0] for d in range(D)]
    out = dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=np.zeros(V, dtype=np.int64))
    for v in range(V):
        b, e = int(word_off[v]), int(word_off[v + 1])
        total = np.zeros(K, dtype=np.float64)                                # +0.0
        for c in range(b, e, chunk):
            ce = min(c + chunk, e)
            fs = [1] * (ce - c) if freq is None else freq[c:ce]
            acc, tok, bad = chunk_sum_sparse(theta_s, phi_t[v], site_doc[c:ce], fs, (lab_off, lab, fit), K)
            with np.errstate(all="ignore"):
                total = total + acc
            out["tok"][v] += tok
            out["bad"][v] += bad
        out["credit"][v] = total
    return out


def scatter(values, lab_off, lab, K):
    """per-slot values -> (D, K), +0.0 outside the label sets"""
    D = len(lab_off) - 1
    out = np.zeros((D, K), dtype=np.float64)
    out[np.repeat(np.arange(D), np.diff(lab_off)), np.asarray(lab, dtype=np.int64)] = values
    return out


def gather(dense, lab_off, lab):
    D = len(lab_off) - 1
    return np.ascontiguousarray(dense[np.repeat(np.arange(D), np.diff(lab_off)), np.asarray(lab, dtype=np.int64)])


def fit_sparse_ref(theta_s0, phi_t0, doc_off, word, freq, lab_off, lab, alpha, beta, iters, theta_steps=1, chunk=4096, each=None):
    """emfit.fit_sparse: (theta_s [NL], phi_t (V, K)) after iters iterations; each(iteration, theta_s, phi_t) after every one"""
    theta_s, phi_t = np.array(theta_s0, dtype=np.float64), np.array(phi_t0, dtype=np.float64)
    V = phi_t.shape[0]
    word_off, site_doc, w_freq, _ = emref.word_major(doc_off, word, freq, V)
    for it in range(1, iters + 1):
        theta_s = attribute_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, iters=theta_steps, alpha=alpha)["theta_out"]
        cw = credit_words_sparse_ref(theta_s, phi_t, word_off, site_doc, w_freq, lab_off, lab, chunk)["credit"]
        phi_t = emref.phi_step_ref(cw, beta)[0]
        if each is not None:
            each(it, theta_s, phi_t)
    return theta_s, phi_t
