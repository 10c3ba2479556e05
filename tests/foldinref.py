"""What ``llda_foldin`` promises (include/llda_gibbs.h), restated site by site in numpy and float64 -- test infrastructure only.

Everything is in REFERENCE topic order and built from pieces of oracle/llda_oracle.py alone: ``layout`` and ``draw_keyed`` (the keyed
categorical draw), ``keyed_uniform`` (its uniform), and ``np.sum`` of a contiguous 1-D vector for numpy's pairwise order.  Per site it
reads exactly as the header's pseudo-code: no decided tier, no jump in the `while prob.sum() > 1` loop, every product of the thinned
average rounded on its own.  tests/test_foldin_ref_host.py pins it, bit for bit, to oracle run_test / cascade_test / cascade_run_test
(themselves pinned to the unmodified reference by goldens); tests/test_gpu_foldin_direct.py holds the kernels against it.
"""
import numpy as np

import llda_oracle as orc


def _sum(prob):
    return np.sum(np.ascontiguousarray(prob, dtype=np.float64))


def fold_in(*, init_rows, init_idx, ph, doc_off, word, freq, alpha, beta, c_init, c_loop, beta_fallback, avg_mode, iters, thinning,
            seed, doc_ids, doc_streams, ph_sel=None):
    """init_rows (R, K) float64, init_idx[S] the row of every site; ph (K, V) float64 or a list of such matrices with ph_sel[d] the
    one document d samples against; doc_off / word / freq the CSR; doc_ids[d] / doc_streams[d] the RNG id (its low 32 bits count) and
    stream of document d.  -> dict(z int64[S] topic ids, n_dk int64 (D, K), th float64 (D, K), raises bool[D]).

    raises[d]: a site of document d had no positive probability (numpy.random.multinomial would raise in the reference); the
    outputs of that document are then unspecified here (left at the state before that site) and are not to be compared."""
    assert c_init > 1 and c_loop > 1                                  # (the loops below would not end)
    init_rows = np.asarray(init_rows, dtype=np.float64)
    phs = [np.asarray(p, dtype=np.float64) for p in (ph if isinstance(ph, (list, tuple)) else [ph])]
    K = init_rows.shape[1]
    lay = orc.layout(K)
    D = len(doc_off) - 1
    z = np.zeros(int(doc_off[-1]), dtype=np.int64)
    n_dk_all = np.zeros((D, K), dtype=np.int64)
    th = np.zeros((D, K), dtype=np.float64)
    raises = np.zeros(D, dtype=bool)
    for d in range(D):
        s0, s1 = int(doc_off[d]), int(doc_off[d + 1])
        if s1 == s0:
            continue                                                  # an empty document: n_dk = 0, th = 0
        P = phs[0 if ph_sel is None else int(ph_sel[d])]
        doc, stream = int(doc_ids[d]) & 0xFFFFFFFF, int(doc_streams[d]) & 0xFFFFFFFF
        n_dk = n_dk_all[d]
        try:
            for n in range(s1 - s0):                                  # prep4test
                prob = init_rows[int(init_idx[s0 + n])].copy()
                while _sum(prob) > 1:
                    prob /= c_init
                u = float(orc.keyed_uniform(seed, orc.SWEEP_INIT, stream, doc, n))
                z[s0 + n] = orc.draw_keyed(prob, u, lay)
                n_dk[z[s0 + n]] += int(freq[s0 + n])
            avg = np.zeros(K, dtype=np.float64)
            for i in range(iters):
                for n in range(s1 - s0):
                    v, f = int(word[s0 + n]), int(freq[s0 + n])
                    n_dk[z[s0 + n]] -= f
                    num_a = n_dk + alpha
                    b = P[:, v]
                    prob = num_a * b
                    S = _sum(prob)
                    if beta_fallback and S == 0.0:                    # (0 / 0 raises in the reference)
                        prob = num_a * (b + beta)
                        S = _sum(prob)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        prob /= S
                    while _sum(prob) > 1:
                        prob /= c_loop
                    u = float(orc.keyed_uniform(seed, i, stream, doc, n))
                    try:
                        new_z = orc.draw_keyed(prob, u, lay)
                    except FloatingPointError:
                        n_dk[z[s0 + n]] += f
                        raise
                    z[s0 + n] = new_z
                    n_dk[new_z] += f
                if (i + 1) % thinning == 0:
                    s2 = (i + 1) // thinning
                    cur = n_dk / n_dk.sum()
                    if s2 == 1:
                        avg = cur
                    elif avg_mode == 0:
                        old = (s2 - 1) / s2 * avg
                        new = (1 / s2) * cur
                        avg = old + new
                    else:
                        m = (s2 - 1) / s2
                        old = m * avg
                        new = (1 - m) * cur
                        avg = old + new
            th[d] = avg
        except FloatingPointError:
            raises[d] = True
    return dict(z=z, n_dk=n_dk_all, th=th, raises=raises)
