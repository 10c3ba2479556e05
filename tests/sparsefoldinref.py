"""CPU restatement of llda_foldin_sparse (include/llda_gibbs.h), written site by site from the header in numpy float64 -- test
infrastructure only.  The pieces are oracle/llda_oracle.py's ``layout``, ``draw_keyed`` and ``keyed_uniform``, ``np.sum`` of a
contiguous 1-D vector for numpy's order, and tests/sparseref.py's ``doc_fit``.

    problem   of a fit document: K' = L_d, ph'[j][v] = phi_t[v][lab[j]], in layout(L_d); z holds the SLOT j
    start     a first pass finds a column that cannot be normalised (sum 0, or a quotient that is not finite): then every site
              starts from 1 / L_d, else from column / sum; `while sum > 1: prob /= c_init`; the draw under SWEEP_INIT
    sweep     prob = (n_dk + alpha) * ph'[:, v]; prob /= sum; `while sum > 1: prob /= c_loop`; draw
    average   every `thinning` sweeps, (s-1)/s * avg + (1/s) * cur, each product rounded on its own
    unfit     z = -1 at its sites, its slots keep the fill values, status bit 2
    bad word  z = -1, no count, the site keeps its number n, status bit 1
    raises    a site without a positive probability (every site of L_d = 0): raises[d], status bit 0; the document's outputs are
              then unspecified (left as they were before that site) and are not to be compared

tests/test_sparse_foldin_host.py pins it to tests/foldinref.py on every document's compacted problem; tests/test_gpu_foldin_sparse.py
holds the kernel against it.
"""
import numpy as np

import llda_oracle as orc
import sparseref

C_INIT, C_LOOP = 1.0000000005, 1.0000005            # foldin.fold_in's
MAX_LABELS = sparseref.MAX_LABELS
ND_FILL = -7                                        # n_dk_s of a slot nobody writes (th_s: NaN)


def _sum(prob):
    return np.sum(np.ascontiguousarray(prob, dtype=np.float64))


def _draw(prob, u):
    if prob.shape[0] == 0:
        raise FloatingPointError("no label")
    return orc.draw_keyed(prob, u, orc.layout(prob.shape[0]))


def fold_in_sparse_ref(phi_t, doc_off, word, freq, lab_off, lab, alpha, iters, thinning, seed, stream_id, c_init=C_INIT, c_loop=C_LOOP,
                       K=None, V=None, max_labels=MAX_LABELS, doc_ids=None, doc_base=0, NL=None):
    """phi_t (V, >= K) float64; the sites doc_off / word / freq; the label sets lab_off / lab (NL: how many of lab count)
    -> dict(z int64 [S], n_dk_s int64 [NL], th_s float64 [NL], status, raises bool [D])"""
    assert c_init > 1 and c_loop > 1 and thinning >= 1
    D = len(doc_off) - 1
    K = phi_t.shape[1] if K is None else K
    V = phi_t.shape[0] if V is None else V
    NL = len(lab) if NL is None else NL
    z = np.full(int(doc_off[-1]), -9, dtype=np.int64)
    n_dk_s = np.full(NL, ND_FILL, dtype=np.int64)
    th_s = np.full(NL, np.nan)
    raises = np.zeros(D, dtype=bool)
    status = 0
    stream = int(stream_id) & 0xFFFFFFFF
    for d in range(D):
        s0, s1 = int(doc_off[d]), int(doc_off[d + 1])
        fit, _, lb, L = sparseref.doc_fit(lab_off, lab, d, K, max_labels, NL)
        if not fit:
            z[s0:s1] = -1
            status |= 4
            continue
        ids = np.asarray(lab[lb:lb + L], dtype=np.int64)
        doc = (int(doc_ids[d]) if doc_ids is not None else d + doc_base) & 0xFFFFFFFF
        ws = [int(w) for w in word[s0:s1]]
        fs = [int(f) for f in freq[s0:s1]]
        ok = [0 <= w < V for w in ws]
        if not all(ok):
            status |= 2
        col = lambda w: np.ascontiguousarray(phi_t[w, ids], dtype=np.float64)          # ph'[:, w]
        uniform = False
        with np.errstate(all="ignore"):
            for w, good in zip(ws, ok):
                if good:
                    c = col(w)
                    cs = _sum(c)
                    if cs == 0 or not np.isfinite(c / cs).all():
                        uniform = True
        n_dk = np.zeros(L, dtype=np.int64)
        avg = np.zeros(L, dtype=np.float64)
        n_dk_s[lb:lb + L], th_s[lb:lb + L] = n_dk, avg                                 # (views would not follow `avg = cur`)
        if s1 == s0:
            continue                                                                   # an empty document: n_dk_s = 0, th_s = 0
        try:
            with np.errstate(all="ignore"):
                for n, (w, f, good) in enumerate(zip(ws, fs, ok)):
                    if not good:
                        z[s0 + n] = -1
                        continue
                    if uniform:
                        prob = np.full(L, 1 / L) if L else np.zeros(0)
                    else:
                        c = col(w)
                        prob = c / _sum(c)
                    while _sum(prob) > 1:
                        prob = prob / c_init
                    u = float(orc.keyed_uniform(seed, orc.SWEEP_INIT, stream, doc, n))
                    z[s0 + n] = _draw(prob, u)
                    n_dk[z[s0 + n]] += f
                    n_dk_s[lb:lb + L] = n_dk
                for i in range(iters):
                    for n, (w, f, good) in enumerate(zip(ws, fs, ok)):
                        if not good:
                            continue
                        n_dk[z[s0 + n]] -= f
                        prob = (n_dk + alpha) * col(w)
                        S = _sum(prob)
                        prob = prob / S
                        while _sum(prob) > 1:
                            prob = prob / c_loop
                        u = float(orc.keyed_uniform(seed, i, stream, doc, n))
                        try:
                            new_z = _draw(prob, u)
                        except FloatingPointError:
                            n_dk[z[s0 + n]] += f
                            raise
                        z[s0 + n] = new_z
                        n_dk[new_z] += f
                        n_dk_s[lb:lb + L] = n_dk
                    if (i + 1) % thinning == 0:
                        s2 = (i + 1) // thinning
                        cur = n_dk / n_dk.sum()
                        if s2 == 1:
                            avg = cur
                        else:
                            old = (s2 - 1) / s2 * avg
                            new = (1 / s2) * cur
                            avg = old + new
                        th_s[lb:lb + L] = avg
        except FloatingPointError:
            raises[d] = True
            status |= 1
    return dict(z=z, n_dk_s=n_dk_s, th_s=th_s, status=status, raises=raises)


def prepared_rows(sub):
    """numpy port of foldin.fold_in's preparation for loadings ``sub`` (K', V'): every column divided by its own numpy sum (the
    fancy-indexed matrix is F-contiguous: a contiguous column each), a bad column -> 0 -> (rows (V' + 1, K'), bad bool [V']); row V'
    is the uniform one."""
    Kc, Vc = sub.shape
    colsum = np.array([_sum(sub[:, v]) for v in range(Vc)])
    with np.errstate(all="ignore"):
        phn = sub / colsum
    bad = ~np.isfinite(phn).all(axis=0) | (colsum == 0)
    rows = np.zeros((Vc + 1, Kc))
    rows[:Vc] = np.where(bad[None, :], 0.0, phn).T
    rows[Vc] = 1 / Kc
    return rows, bad
