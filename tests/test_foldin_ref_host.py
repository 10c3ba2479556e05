"""tests/foldinref.py -- the restatement of llda_foldin's contract the direct GPU test compares with -- pinned on the CPU: with inputs
prepared by the numpy expressions of oracle prep4test / cascade_prep4test it gives bit for bit what oracle run_test, cascade_test
and cascade_run_test give (th_hat as they return it; z and n_dk as their draws leave them), for a narrow and for a wide K.  Those
three are pinned to the unmodified reference by goldens (tests/test_oracle_golden.py), so this ties foldinref to the reference.

CascadeLDA's initial rows sum to 1 - p_0 + 1 / len(doc) and its `while prob.sum() > 1: prob /= 1.0000005` takes ln(sum) / 5e-7 steps,
so the loadings of the generic topic are set to put p_0 within 0.004 of 1 / len(doc): both signs occur and a loop stays short."""
import numpy as np
import pytest

import llda_oracle as orc
import foldinref

SEED, STREAM = 77, 0x7E57
KS = [12, 1031]            # narrow (G = 8, T = 2), wide (9 pairwise leaves)


class Recorder(object):
    """draw_for / draw_for_sweep factories whose draws are logged per (document, sweep)"""

    def __init__(self, doc_ids):
        self.doc_ids, self.log = doc_ids, {}

    def draw_for(self, d, sweep):
        k = orc.KeyedDraw(SEED, STREAM)
        k.sweep, k.doc, k.site = sweep, int(self.doc_ids[d]), 0
        log = self.log[(d, sweep)] = []

        def draw(n, prob):
            out = k(n, prob)
            log.append(int(out.argmax()))
            return out
        return draw

    def final(self, docs, freqs, iters, K):
        """(z, n_dk) after the last sweep"""
        last = iters - 1 if iters > 0 else orc.SWEEP_INIT
        z = np.concatenate([np.asarray(self.log[(d, last)], dtype=np.int64) for d in range(len(docs))])
        n_dk = np.zeros((len(docs), K), dtype=np.int64)
        for d, fr in enumerate(freqs):
            np.add.at(n_dk[d], self.log[(d, last)], fr)
        return z, n_dk


def _csr(docs, freqs):
    doc_off = np.concatenate(([0], np.cumsum([len(d) for d in docs]))).astype(np.int64)
    return doc_off, np.concatenate(docs).astype(np.int32), np.concatenate(freqs).astype(np.int32)


def _docs(rng, V, lens, must_hold=None):
    """documents of distinct words, no word in two documents; ``must_hold``: a word put into the last document, and into no other"""
    perm = rng.permutation([v for v in range(V) if v != must_hold])
    assert sum(lens) <= len(perm)
    docs, freqs, at = [], [], 0
    for i, n in enumerate(lens):
        ids = perm[at:at + n].copy()
        at += n
        if must_hold is not None and i == len(lens) - 1:
            ids[n // 2] = must_hold
        docs.append([int(v) for v in ids])
        freqs.append([int(f) for f in rng.integers(1, 5, size=n)])
    return docs, freqs


def _check(got, want_th, rec, docs, freqs, iters, K):
    assert not got["raises"].any()
    np.testing.assert_array_equal(got["th"], want_th)
    z, n_dk = rec.final(docs, freqs, iters, K)
    np.testing.assert_array_equal(got["z"], z)
    np.testing.assert_array_equal(got["n_dk"], n_dk)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("iters,thinning", [(5, 2), (0, 1)])
def test_equals_oracle_run_test(K, iters, thinning):
    """LabeledLDA.prep4test + run_test: column-normalised loadings as initial rows, c = 1.0000000005 / 1.0000005, no fall-back"""
    rng = np.random.default_rng([1, K])
    V = 30
    ph_hat = rng.random((K, V)) ** 12 + 1e-300                        # wide dynamic range, no exact zero
    ph_hat /= ph_hat.sum(axis=1, keepdims=True)
    docs, freqs = _docs(rng, V, [1, 2, 9, 17])
    doc_ids = np.array([5, 2 ** 32 - 1, 0, 123456789])
    rec = Recorder(doc_ids)
    want = orc.run_test(ph_hat, 0.1, docs, freqs, iters, thinning, rec.draw_for)
    rows = []
    for ids in docs:                                                  # prep4test, oracle/llda_oracle.py
        probs = ph_hat[:, list(ids)]
        probs /= probs.sum(axis=0)
        rows.append(probs.T)
    doc_off, word, freq = _csr(docs, freqs)
    got = foldinref.fold_in(init_rows=np.vstack(rows), init_idx=np.arange(len(word)), ph=ph_hat, doc_off=doc_off, word=word, freq=freq,
                            alpha=0.1, beta=0.0, c_init=1.0000000005, c_loop=1.0000005, beta_fallback=False, avg_mode=0, iters=iters,
                            thinning=thinning, seed=SEED, doc_ids=doc_ids, doc_streams=np.full(len(docs), STREAM))
    _check(got, want, rec, docs, freqs, iters, K)


def _cascade_rows(ph, beta, docs):
    rows = []
    for ids in docs:                                                  # cascade_prep4test, oracle/llda_oracle.py
        probs = ph[:, list(ids)]
        probs += beta
        probs /= probs.sum(axis=0)
        probs[0, :] = 1 / len(ids)
        rows.append(probs.T)
    return np.vstack(rows)


def _cascade_case(K):
    """sparse loadings (the all-zero word V - 1 triggers the fall-back), generic row set so that the initial rows sum to 1 +- 0.004"""
    rng = np.random.default_rng([2, K])
    V, beta = 64, 0.01
    # (the all-zero word has p_0 = 1 / K whatever the generic row holds: it sits in the last document, whose 1 / len is nearest to that)
    docs, freqs = _docs(rng, V, [8, 12, 12] if K < 100 else [8, 12, 40], must_hold=V - 1)
    ph = rng.random((K, V)) ** 12
    ph[rng.random((K, V)) < 0.6] = 0.0
    ph[1 + np.arange(V) % (K - 1), np.arange(V)] += 1e-3             # no word but the last is all zero
    ln = np.full(V, 8.0)
    for ids in docs:
        ln[ids] = len(ids)
    target = 1 / ln + rng.uniform(-0.004, 0.004, V)                  # p_0 of every word
    ph[0] = np.maximum(target / (1 - target) * (ph[1:] + beta).sum(axis=0) - beta, 0.0)
    ph[:, V - 1] = 0.0
    return ph, beta, docs, freqs


def _short_loops(rows):
    sums = np.array([np.sum(r) for r in rows])
    assert (sums > 1).any() and (sums < 1).any() and sums.max() < 1.03


@pytest.mark.parametrize("K", KS)
def test_equals_oracle_cascade_test(K):
    """CascadeLDA.prep4test + cascade_test: the beta fall-back on a word that loads on no topic, averaging formula 0"""
    ph, beta, docs, freqs = _cascade_case(K)
    rows = _cascade_rows(ph, beta, docs)
    _short_loops(rows)
    iters, thinning = 5, 2
    doc_ids = np.array([3, 4, 2 ** 31])
    rec = Recorder(doc_ids)
    want = np.array([orc.cascade_test(ph, 0.2, beta, docs[d], freqs[d], iters, thinning, lambda sw, d=d: rec.draw_for(d, sw))
                     for d in range(len(docs))])
    doc_off, word, freq = _csr(docs, freqs)
    kw = dict(init_rows=rows, init_idx=np.arange(len(word)), ph=ph, doc_off=doc_off, word=word, freq=freq, alpha=0.2, beta=beta,
              c_init=1.0000005, c_loop=1.000005, avg_mode=0, iters=iters, thinning=thinning, seed=SEED, doc_ids=doc_ids,
              doc_streams=np.full(len(docs), STREAM))
    got = foldinref.fold_in(beta_fallback=True, **kw)
    _check(got, want, rec, docs, freqs, iters, K)
    # without the fall-back the document that holds the all-zero word would raise, and only that one
    got = foldinref.fold_in(beta_fallback=False, **kw)
    np.testing.assert_array_equal(got["raises"], [False, False, True])
    np.testing.assert_array_equal(got["th"][:2], want[:2])


@pytest.mark.parametrize("K", KS)
def test_equals_oracle_cascade_run_test(K):
    """CascadeLDA.prep4test + run_test (flat): no fall-back, averaging formula 1"""
    ph, beta, docs, freqs = _cascade_case(K)
    zero = ph.shape[1] - 1                                            # (0 / 0 raises here: the all-zero word leaves the corpus)
    freqs = [[f for v, f in zip(ids, fr) if v != zero] for ids, fr in zip(docs, freqs)]
    docs = [[v for v in ids if v != zero] for ids in docs]
    rows = _cascade_rows(ph, beta, docs)
    _short_loops(rows)
    iters, thinning = 6, 2
    doc_ids = np.array([0, 1, 2])
    rec = Recorder(doc_ids)
    want = orc.cascade_run_test(ph, 0.2, beta, docs, freqs, iters, thinning, rec.draw_for)
    doc_off, word, freq = _csr(docs, freqs)
    got = foldinref.fold_in(init_rows=rows, init_idx=np.arange(len(word)), ph=ph, doc_off=doc_off, word=word, freq=freq, alpha=0.2,
                            beta=beta, c_init=1.0000005, c_loop=1.000005, beta_fallback=False, avg_mode=1, iters=iters,
                            thinning=thinning, seed=SEED, doc_ids=doc_ids, doc_streams=np.full(len(docs), STREAM))
    _check(got, want, rec, docs, freqs, iters, K)


def test_rows_indices_streams_and_empty_documents():
    """what the oracle functions never vary: shared init rows through init_idx, a stream and a loadings matrix per document (each
    document equals the run against its own matrix alone), empty documents (n_dk = 0, th = 0)"""
    rng = np.random.default_rng(3)
    K, V = 9, 20
    phs = [rng.random((K, V)) for _ in range(2)]
    rows = rng.random((V, K))
    rows /= rows.sum(axis=1, keepdims=True)
    docs, freqs = _docs(rng, V, [3, 5, 4])
    _, word, freq = _csr(docs, freqs)
    doc_off = np.array([0, 0, 3, 3, 8, 12, 12])                      # documents 0, 2 and 5 are empty
    D = 6
    kw = dict(init_rows=rows, init_idx=word, doc_off=doc_off, word=word, freq=freq, alpha=0.3, beta=0.0, c_init=1.0005, c_loop=1.0000005,
              beta_fallback=False, avg_mode=0, iters=4, thinning=2, seed=SEED, doc_ids=np.arange(D) + 9)
    streams, sel = np.array([1, 2, 3, 1, 2, 3]), np.array([0, 1, 1, 0, 1, 0])
    got = foldinref.fold_in(ph=phs, ph_sel=sel, doc_streams=streams, **kw)
    for d in (0, 2, 5):
        assert not got["n_dk"][d].any() and not got["th"][d].any()
    for j in range(2):
        alone = foldinref.fold_in(ph=phs[j], doc_streams=streams, **kw)
        for d in np.flatnonzero(sel == j):
            np.testing.assert_array_equal(got["th"][d], alone["th"][d])
            np.testing.assert_array_equal(got["z"][doc_off[d]:doc_off[d + 1]], alone["z"][doc_off[d]:doc_off[d + 1]])
    other = foldinref.fold_in(ph=phs, ph_sel=sel, doc_streams=streams + 1, **kw)
    assert not np.array_equal(other["z"], got["z"])
    for d in range(D):
        assert got["n_dk"][d].sum() == freq[doc_off[d]:doc_off[d + 1]].sum()
