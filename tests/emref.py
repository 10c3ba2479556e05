"""CPU restatement of llda_credit_words and llda_phi_step (include/llda_gibbs.h) and of the EM iteration built from them
(lda_thesis_amd/emfit.py), written from the header: numpy float64 operations, each rounded on its own.

    site     (d, f) of word v: ok = d in [0, D); t_k = theta[d][k] * phi_t[v][k]; p = sum64(t) (attrref.sum64); good: ok and
             2^-960 <= p < inf, else bad[v] += f and nothing else; good: tok[v] += f; inv = 1 / p; g = f * inv; acc_k = acc_k + t_k * g
    order    the sites of a word in chunks of `chunk`; a chunk in ascending site order from +0.0; the chunk sums in ascending chunk
             order from +0.0
    phi step colsum over blocks of 256 words, a block in ascending word order from +0.0, the blocks in ascending order from +0.0;
             Vb = V * beta; den_k = colsum_k + Vb; phi_t[v][k] = (cw[v][k] + beta) / den_k
"""
import numpy as np

import attrref

MIN_P = attrref.MIN_P
COLSUM_ROWS = 256


def chunk_sum(theta, prow, docs, fs, D, K):
    """one chunk: (sum [K], tok, bad)"""
    acc = np.zeros(K, dtype=np.float64)
    tok = bad = 0
    if len(docs) == 0:
        return acc, tok, bad
    docs = np.asarray(docs, dtype=np.int64)
    ok = (docs >= 0) & (docs < D)
    with np.errstate(all="ignore"):
        rows = theta[np.where(ok, docs, 0)][:, :K] if D > 0 else np.zeros((len(docs), K))
        t = rows * prow[None, :K]
        p = attrref.sum64(t)
        good = ok & (p >= MIN_P) & (p < np.inf)
        for s in range(len(docs)):
            if not good[s]:
                bad += int(fs[s])
                continue
            tok += int(fs[s])
            inv = np.float64(1.0) / p[s]
            g = np.float64(fs[s]) * inv
            acc = acc + t[s] * g
    return acc, tok, bad


def credit_words_ref(theta, phi_t, word_off, site_doc, freq, chunk, K=None, D=None):
    """theta (D, >= K), phi_t (V, >= K); word-major CSR word_off / site_doc / freq (None: all 1) -> dict(credit (V, K), tok, bad [V])"""
    V = len(word_off) - 1
    K = phi_t.shape[1] if K is None else K
    D = theta.shape[0] if D is None else D
    out = dict(credit=np.zeros((V, K)), tok=np.zeros(V, dtype=np.int64), bad=np.zeros(V, dtype=np.int64))
    for v in range(V):
        b, e = int(word_off[v]), int(word_off[v + 1])
        total = np.zeros(K, dtype=np.float64)                                # +0.0
        for c in range(b, e, chunk):
            ce = min(c + chunk, e)
            fs = [1] * (ce - c) if freq is None else freq[c:ce]
            acc, tok, bad = chunk_sum(theta, phi_t[v], site_doc[c:ce], fs, D, K)
            with np.errstate(all="ignore"):
                total = total + acc
            out["tok"][v] += tok
            out["bad"][v] += bad
        out["credit"][v] = total
    return out


def phi_step_ref(cw, beta, K=None):
    """cw (V, >= K) -> (phi_t (V, K), den [K])"""
    V = cw.shape[0]
    K = cw.shape[1] if K is None else K
    colsum = np.zeros(K, dtype=np.float64)
    for r0 in range(0, V, COLSUM_ROWS):
        blk = np.zeros(K, dtype=np.float64)
        for r in range(r0, min(r0 + COLSUM_ROWS, V)):
            blk = blk + cw[r, :K]
        colsum = colsum + blk
    den = colsum + np.float64(V) * np.float64(beta)
    return (cw[:, :K] + np.float64(beta)) / den[None, :], den


def word_major(doc_off, word, freq, V):
    """the stable sort by word id: (word_off, site_doc, freq or None, order)"""
    word = np.asarray(word, dtype=np.int64)
    D = len(doc_off) - 1
    order = np.argsort(word, kind="stable")
    site_doc = np.repeat(np.arange(D, dtype=np.int32), np.diff(doc_off))
    word_off = np.concatenate([[0], np.cumsum(np.bincount(word, minlength=V))]).astype(np.int64)
    return word_off, site_doc[order], None if freq is None else np.asarray(freq)[order], order


def fit_ref(theta0, phi_t0, doc_off, word, freq, alpha, beta, iters, theta_steps=1, chunk=4096, each=None):
    """emfit.fit: (theta (D, K), phi_t (V, K)) after iters iterations; each(iteration, theta, phi_t) is called after every one"""
    theta, phi_t = np.array(theta0, dtype=np.float64), np.array(phi_t0, dtype=np.float64)
    V = phi_t.shape[0]
    word_off, site_doc, w_freq, _ = word_major(doc_off, word, freq, V)
    for it in range(1, iters + 1):
        theta = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, iters=theta_steps, alpha=alpha)["theta_out"]
        cw = credit_words_ref(theta, phi_t, word_off, site_doc, w_freq, chunk)["credit"]
        phi_t = phi_step_ref(cw, beta)[0]
        if each is not None:
            each(it, theta, phi_t)
    return theta, phi_t


def data_term(theta, phi_t, doc_off, word, freq):
    """sum f log p over the good sites (plain float64; for the monotonicity checks only)"""
    D = len(doc_off) - 1
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    p = np.einsum("sk,sk->s", theta[doc], phi_t[np.asarray(word, dtype=np.int64)])
    f = np.ones(len(doc)) if freq is None else np.asarray(freq, dtype=np.float64)
    ok = (p >= MIN_P) & np.isfinite(p)
    return float(np.sum(f[ok] * np.log(p[ok])))


def objective(theta, phi_t, doc_off, word, freq, alpha, beta):
    """the MAP objective of emfit.py: sum f log p + alpha sum_{theta > 0} log theta + beta sum log phi"""
    return data_term(theta, phi_t, doc_off, word, freq) + alpha * float(np.sum(np.log(theta[theta > 0.0]))) + beta * float(np.sum(np.log(phi_t)))
