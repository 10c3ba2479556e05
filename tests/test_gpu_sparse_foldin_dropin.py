"""The fold-in sampler on label lists through the drop-in class, on the tiny_k12 corpus (K = 12 <= 32): run_test / predict / score_test
with ``candidates`` and ``shortlist``, heldout_perplexity with ``labels``, and the defaults, which stay what they were."""
import functools
import math

import numpy as np
import pytest

import sparsefoldinref as sfr
import sparseheldref
import sparseref

pytestmark = pytest.mark.gpu

IT, THIN = 12, 4


@functools.lru_cache(maxsize=None)
def fitted():
    """tiny_k12 after two EM passes; its first documents as held-out text, with scattered candidate lists of none .. three labels"""
    from test_gpu_dropin import build_model
    from test_gpu_fit_em_sparse_dropin import CHUNK
    m, _, _ = build_model("k12")
    m.fit_em(2, chunk=CHUNK)
    names = sorted(m.labelmap, key=m.labelmap.get)
    assert names[0] == "root" and len(names) == m.K <= 32
    docs = [[m.v_to_w[w] for w, f in t for _ in range(f)] for t in m.doc_tups[:12]]
    cands = [[names[1 + (5 * d + 3 * j) % (m.K - 1)] for j in range(d % 4)] for d in range(12)]
    return m, docs, cands, names


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def csr_of(tups):
    return (np.concatenate([[0], np.cumsum([len(t) for t in tups])]).astype(np.int64), np.array([w for t in tups for w, _ in t], dtype=np.int32),
            np.array([f for t in tups for _, f in t], dtype=np.int32))


def sets_of(m, labels):
    cols = [[0] + sorted(set(int(m.labelmap[x]) for x in labs) - {0}) for labs in labels]
    return np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64), np.concatenate(cols).astype(np.int32)


def test_every_label_as_a_candidate_is_run_test():
    m, docs, _, names = fitted()
    dense = m.run_test(docs, IT, THIN)
    got = m.run_test(docs, IT, THIN, candidates=[names[1:]] * len(docs))
    assert dense.shape == got.shape == (len(docs), m.K) and np.array_equal(bits(got), bits(dense))
    assert np.array_equal(bits(m.run_test(docs, IT, THIN, seed=5, stream_id=9, candidates=[names[1:]] * len(docs))),
                          bits(m.run_test(docs, IT, THIN, seed=5, stream_id=9)))


def test_candidates_equal_the_restatement_and_rank_like_get_preds():
    from lda_thesis_amd.foldin import TEST_STREAM
    m, docs, cands, names = fitted()
    tups = [m.dicti.doc2bow(x) for x in docs]
    lab_off, lab = sets_of(m, cands)
    want = sfr.fold_in_sparse_ref(np.ascontiguousarray(m.ph_hat.T), *csr_of(tups), lab_off, lab, m.alpha, IT, THIN, m.seed, TEST_STREAM)
    assert not want["raises"].any()
    th = m.run_test(docs, IT, THIN, candidates=cands)
    assert np.array_equal(bits(th), bits(sparseref.scatter(want["th_s"], lab_off, lab, m.K))) and not np.signbit(th).any()
    assert np.array_equal(th != 0, sparseref.scatter(want["th_s"], lab_off, lab, m.K) != 0)
    # predict: the pairs of get_preds on that matrix, wherever get_pred's own order is defined: distinct positive loads
    for n in (1, 2):
        got = m.predict(docs, IT, THIN, n=n, candidates=cands)
        host = m.get_preds(th, n)
        seen = 0
        for d in range(len(docs)):
            top = np.sort(th[d])[::-1][:n + 1]
            if top[n - 1] > 0 and len(set(top)) == n + 1 and lab_off[d + 1] - lab_off[d] >= n:
                assert [(a, b) for a, b in got[d]] == [(a, b) for a, b in host[d]], d
                seen += 1
        assert seen >= 4
    # score_test on the lists: ranking.metrics of the scattered loads
    from lda_thesis_amd import ranking
    from lda_thesis_amd.evaluate import binary_yreal
    truth = [[names[1 + (d + j) % (m.K - 1)] for j in range(1 + d % 2)] for d in range(len(docs))]
    assert m.score_test(docs, truth, IT, THIN, candidates=cands) == ranking.metrics(ranking.rank_labels(th, binary_yreal(truth, m.labelmap), first=1, top_n=0))


def test_shortlist_is_its_three_steps():
    """one attribution pass from uniform loads, the m best-credited labels without the root, the sampler on root plus those"""
    import torch
    from lda_thesis_amd import attribution, ranking
    m, docs, _, names = fitted()
    tups = [m.dicti.doc2bow(x) for x in docs]
    doc_off, word, freq = csr_of(tups)
    phi_t = torch.from_numpy(np.ascontiguousarray(m.ph_hat.T)).cuda()
    for short in (1, 3):
        credit = attribution.attribute(torch.full((len(docs), m.K), 1.0 / m.K, dtype=torch.float64).cuda(), phi_t, doc_off, word, freq, iters=0,
                                       top_m=0, want=("credit",))["credit"]
        ranked = ranking.rank_labels(credit, None, first=1, top_n=short).host()["top_idx"]
        by_hand = [[names[k] for k in row if k >= 1] for row in ranked]
        assert all(len(x) == short for x in by_hand)
        assert m.shortlist_cols(tups, short) == [[0] + sorted(m.labelmap[x] for x in labs) for labs in by_hand]
        th = m.run_test(docs, IT, THIN, candidates=by_hand)
        got = m.predict(docs, IT, THIN, n=2, shortlist=short)
        assert got == m.predict(docs, IT, THIN, n=2, candidates=by_hand)
        assert all(len(p) == min(2, short + 1) for p in got)
        truth = [[names[1 + d % (m.K - 1)]] for d in range(len(docs))]
        assert m.score_test(docs, truth, IT, THIN, shortlist=short) == m.score_test(docs, truth, IT, THIN, candidates=by_hand)
        assert ((th != 0).sum(axis=1) <= short + 1).all()
    with pytest.raises(ValueError):
        m.predict(docs, IT, THIN, candidates=by_hand, shortlist=3)
    with pytest.raises(ValueError):
        m.score_test(docs, truth, IT, THIN, shortlist=17)


def test_heldout_perplexity_on_labels_equals_the_restatement():
    from lda_thesis_amd import heldout
    from lda_thesis_amd.foldin import TEST_STREAM
    m, docs, cands, names = fitted()
    docs, labels = docs + [["no-such-token"], []], cands + [[names[1]], []]
    tups = [m.dicti.doc2bow(x) for x in docs]
    keep = [d for d, t in enumerate(tups) if t[0::2]]
    assert keep == list(range(12))
    obs, sc = [tups[d][0::2] for d in keep], [tups[d][1::2] for d in keep]
    lab_off, lab = sets_of(m, [labels[d] for d in keep])
    phi_t = np.ascontiguousarray(m.ph_hat.T)
    th_s = sfr.fold_in_sparse_ref(phi_t, *csr_of(obs), lab_off, lab, m.alpha, IT, THIN, m.seed, TEST_STREAM)["th_s"]
    theta_s = sparseheldref.smooth_slots_ref(th_s, heldout.observed_tokens(obs), lab_off, m.alpha)
    for weighted in (True, False):
        s_off, s_word, s_freq = csr_of(sc)
        want = heldout.perplexity_from(*sparseheldref.loglik_sparse_ref(theta_s, phi_t, s_off, s_word, s_freq if weighted else None, lab_off, lab))
        got = m.heldout_perplexity(docs, IT, THIN, weighted=weighted, labels=labels)
        assert (got["loglik"], got["tokens"], got["documents"], got["skipped"]) == (want["loglik"], want["tokens"], 12, 2)
        assert got["perplexity"] == want["perplexity"] and got["tokens"] > 0 and 1.0 < got["perplexity"] < len(m.dicti)
    free = m.heldout_perplexity(docs, IT, THIN)
    assert free["documents"] == 12 and free["skipped"] == 2 and math.isfinite(free["perplexity"])
    with pytest.raises(ValueError):
        m.heldout_perplexity(docs, IT, THIN, labels=labels[:-1])


def test_defaults_return_what_they_returned():
    """without the new keywords the dense fold-in: the same launch as foldin.fold_in by hand"""
    from lda_thesis_amd import foldin, ranking
    m, docs, _, names = fitted()
    tups = [m.dicti.doc2bow(x) for x in docs]
    by_hand = foldin.fold_in(m.ph_hat, m.alpha, tups, IT, THIN, m.seed, foldin.TEST_STREAM)["th_hat"]
    assert np.array_equal(bits(m.run_test(docs, IT, THIN)), bits(by_hand))
    assert np.array_equal(bits(m.run_test(docs, IT, THIN, candidates=None)), bits(by_hand))
    r = ranking.rank_labels(by_hand, None, first=0, top_n=3).host()
    assert m.predict(docs, IT, THIN, n=3) == m.predict(docs, IT, THIN, n=3, candidates=None, shortlist=None) == \
        [list(zip(np.array(list(m.labelmap.keys()))[i], v)) for i, v in zip(r["top_idx"], r["top_val"])]
