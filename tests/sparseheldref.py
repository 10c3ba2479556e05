"""CPU restatement of llda_heldout_loglik_sparse and llda_left_to_right_sparse (include/llda_gibbs.h) and of
LabeledLDA.heldout_perplexity_em, written from the header on the pieces of heldoutref.py, leftrightref.py and sparseref.py, which are
imported unchanged: a fit document is handed to the dense restatement on its compacted problem -- K' = L_d, theta' = its slots,
phi_t'[w][j] = phi_t[w][lab[j]] -- one document at a time.

    unfit    (sparseref.doc_fit) score: every site adds f to bad, tok = 0, pair (0.5, 1); left-to-right: every token is bad
    L_d = 0  fit: p = 0 at every site / A = 0 and pred = NaN at every position: all bad
    too long left-to-right only: more than max_doc_tokens tokens: status bit 0 and (0.5, 1, 0, 0), before anything else
"""
import numpy as np

import heldoutref
import leftrightref
import sparseref

MAX_LABELS = sparseref.MAX_LABELS


def loglik_sparse_ref(theta_s, phi_t, doc_off, word, freq, lab_off, lab, K=None, V=None, max_labels=MAX_LABELS, NL=None):
    """theta_s [NL], phi_t (V, >= K); the sites doc_off / word / freq (None: all 1); the label sets lab_off / lab -> (mant float64
    [D], expo, tok, bad int64 [D])"""
    D = len(doc_off) - 1
    K = phi_t.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    theta_s = np.asarray(theta_s, dtype=np.float64)
    mant, expo = np.full(D, 0.5), np.ones(D, dtype=np.int64)
    tok, bad = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    for d in range(D):
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        fs = [1] * (e - b) if freq is None else [int(x) for x in freq[b:e]]
        fit, _, lb, L = sparseref.doc_fit(lab_off, lab, d, K, max_labels, NL)
        if not fit or L == 0:
            bad[d] = sum(fs)
            continue
        ids = np.asarray(lab[lb:lb + L], dtype=np.int64)
        sub = np.ascontiguousarray(phi_t[:V][:, ids])                      # phi_t'[w][j] = phi_t[w][lab[j]]
        r = heldoutref.loglik_ref(theta_s[None, lb:lb + L], sub, np.array([0, e - b], dtype=np.int64), word[b:e],
                                  None if freq is None else freq[b:e], K=L, V=V)
        mant[d], expo[d], tok[d], bad[d] = r[0][0], r[1][0], r[2][0], r[3][0]
    return mant, expo, tok, bad


def left_to_right_sparse_ref(phi_t, doc_off, word, lab_off, lab, alpha, R, seed, stream_id, K=None, V=None, max_labels=MAX_LABELS,
                             doc_ids=None, max_doc_tokens=None, NL=None, trace=None, stats=None):
    """phi_t (V, >= K); token CSR; the label sets -> (mant, expo, tok, bad, status).  trace: a dict that receives 'z' and 'p', one
    entry per document (the SLOTS assigned, (R, N), and the p_n; None for a document that is not drawn for)"""
    D = len(doc_off) - 1
    K = phi_t.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    ids_all = np.arange(D, dtype=np.int64) if doc_ids is None else np.asarray(doc_ids, dtype=np.int64)
    mant, expo = np.full(D, 0.5), np.ones(D, dtype=np.int64)
    tok, bad = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    status = 0
    zs, ps = [None] * D, [None] * D
    for d in range(D):
        b, e = int(doc_off[d]), int(doc_off[d + 1])
        if max_doc_tokens is not None and e - b > max_doc_tokens:
            status = 1
            continue
        fit, _, lb, L = sparseref.doc_fit(lab_off, lab, d, K, max_labels, NL)
        if not fit or L == 0:
            bad[d] = e - b
            continue
        ids = np.asarray(lab[lb:lb + L], dtype=np.int64)
        sub = np.ascontiguousarray(phi_t[:V][:, ids])
        t = {}
        r = leftrightref.left_to_right_ref(sub, np.array([0, e - b], dtype=np.int64), word[b:e], alpha, R, seed, stream_id, K=L, V=V,
                                           allowed=None, doc_ids=[int(ids_all[d])], trace=t, stats=stats)
        mant[d], expo[d], tok[d], bad[d] = r[0][0], r[1][0], r[2][0], r[3][0]
        zs[d], ps[d] = t["z"][0][:, :e - b], t["p"][0][:e - b]
    if trace is not None:
        trace["z"], trace["p"] = zs, ps
    return mant, expo, tok, bad, status


def smooth_slots_ref(th_s, w_obs, lab_off, alpha):
    """(W_d * th + alpha) / (W_d + L_d * alpha) at every slot of document d"""
    counts = np.diff(np.asarray(lab_off, dtype=np.int64))
    rows = np.repeat(np.arange(len(counts)), counts)
    den = np.asarray(w_obs, dtype=np.float64) + counts.astype(np.float64) * alpha
    return (np.asarray(w_obs, dtype=np.float64)[rows] * np.asarray(th_s, dtype=np.float64) + alpha) / den[rows]


def heldout_perplexity_em_ref(phi_t, doc_tups, label_cols, alpha, iters, weighted=True, scored_tups=None):
    """LabeledLDA.heldout_perplexity_em(labels=..., sparse=True) on doc2bow lists: phi_t (V, K); label_cols one ascending list of
    topic ids per document (root included) -> dict(loglik, tokens, bad, documents, skipped, mant, expo)"""
    if scored_tups is None:
        observed, scored = [list(t[0::2]) for t in doc_tups], [list(t[1::2]) for t in doc_tups]
    else:
        observed, scored = doc_tups, scored_tups
    keep = [d for d, t in enumerate(observed) if t]
    observed, scored, cols = [observed[d] for d in keep], [scored[d] for d in keep], [label_cols[d] for d in keep]

    def csr(tups):
        off = np.concatenate([[0], np.cumsum([len(t) for t in tups])]).astype(np.int64)
        return off, np.array([w for t in tups for w, _ in t], dtype=np.int32), np.array([f for t in tups for _, f in t], dtype=np.int32)

    lab_off = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    lab = np.array([k for c in cols for k in c], dtype=np.int32)
    th0 = np.concatenate([np.full(len(c), np.float64(1.0) / np.float64(len(c))) for c in cols]) if cols else np.zeros(0)
    o_off, o_word, o_freq = csr(observed)
    th = sparseref.attribute_sparse_ref(th0, phi_t, o_off, o_word, o_freq, lab_off, lab, iters=iters, alpha=alpha)["theta_out"]
    w_obs = np.array([float(sum(int(f) for _, f in t)) for t in observed], dtype=np.float64)
    theta_s = smooth_slots_ref(th, w_obs, lab_off, alpha)
    s_off, s_word, s_freq = csr(scored)
    mant, expo, tok, bad = loglik_sparse_ref(theta_s, phi_t, s_off, s_word, s_freq if weighted else None, lab_off, lab)
    total = 0.0
    for m, e in zip(mant.tolist(), expo.tolist()):
        total += float(np.log(np.float64(m)) + np.float64(e) * np.log(2.0))
    return dict(loglik=total, tokens=int(tok.sum()), bad=int(bad.sum()), documents=len(keep), skipped=len(doc_tups) - len(keep),
                mant=mant, expo=expo)
