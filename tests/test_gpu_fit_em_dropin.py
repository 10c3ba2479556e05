"""EM training through the drop-in class (LabeledLDA.fit_em) on the tiny_k12 corpus: bit for bit against tests/emref.py from the
same start, without a trace in the chain's state, and with every reader of ph_hat / th_hat on the EM estimates afterwards."""
import numpy as np
import pytest

import attrref
import emref
from test_gpu_dropin import build_model

pytestmark = pytest.mark.gpu

ITERS, CHUNK = 8, 16                                                      # (chunk 16: the frequent words of the corpus have several chunks)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def csr(m):
    from lda_thesis_amd.corpus import csr_from_doc_tups
    return csr_from_doc_tups(m.doc_tups)


def state(m):
    return dict(n_zk=m.n_zk.copy(), n_d_k=m.n_d_k.copy(), n_k_v=m.n_k_v.copy(), z=np.concatenate(m.z_dn))


def test_fit_em_equals_emref_and_leaves_the_chain_alone(capsys):
    m, _, _ = build_model("k12")
    twin, _, _ = build_model("k12")
    doc_off, word, freq = csr(m)
    assert int(np.bincount(word).max()) > 2 * CHUNK
    th0, phi_t0 = m.get_theta(), np.ascontiguousarray(m.get_phi().T)
    before = state(m)
    assert not m.cur_perplx
    r = m.fit_em(ITERS, chunk=CHUNK, trace_every=1)
    assert sorted(r) == ["iterations", "trace"] and r["iterations"] == ITERS and len(m.cur_perplx) == 1
    want_trace = []
    want_th, want_phi = emref.fit_ref(th0, phi_t0, doc_off, word, freq, m.alpha, m.beta, ITERS, chunk=CHUNK,
                                      each=lambda it, th, ph: want_trace.append(emref.data_term(th, ph, doc_off, word, freq)))
    assert np.array_equal(bits(m.th_hat), bits(want_th)) and np.array_equal(bits(m.ph_hat), bits(np.ascontiguousarray(want_phi.T)))
    # theta is 0 outside every document's labels, and a distribution inside
    assert (m.th_hat[m.labs == 0] == 0.0).all() and (m.th_hat[m.labs != 0] > 0.0).all() and np.abs(m.th_hat.sum(axis=1) - 1).max() < 1e-12
    assert np.abs(m.ph_hat.sum(axis=1) - 1).max() < 1e-12
    # the trace: the data term of every iteration, never falling
    tokens = int(np.asarray(freq, dtype=np.int64).sum())
    assert [t[0] for t in r["trace"]] == list(range(1, ITERS + 1)) and all(t[2] == tokens and t[3] == 0 for t in r["trace"])
    got_trace = [t[1] for t in r["trace"]]
    print("trace", got_trace)
    np.testing.assert_allclose(got_trace, want_trace, rtol=1e-12)
    for a, b in zip(got_trace[:-1], got_trace[1:]):
        assert b >= a - 1e-9 * abs(a), got_trace
    assert abs(m.cur_perplx[0] / float(np.exp(-emref.data_term(want_th, want_phi, doc_off, word, None) / len(word))) - 1) < 1e-9
    # the chain's state is where it was ...
    after = state(m)
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    # ... two calls give the same bits, whatever happened in between ...
    th1, ph1 = m.th_hat.copy(), m.ph_hat.copy()
    assert m.fit_em(ITERS, chunk=CHUNK)["trace"] == []
    assert np.array_equal(bits(m.th_hat), bits(th1)) and np.array_equal(bits(m.ph_hat), bits(ph1))
    # ... the default chunk adds in another order: close, and the same zeros
    m.fit_em(ITERS)
    np.testing.assert_allclose(m.ph_hat, ph1, rtol=1e-9)
    assert np.array_equal(m.th_hat == 0.0, th1 == 0.0)
    # ... and run_training goes on as on a model that never called it, its read-outs starting the means afresh
    m.run_training(4, 2)
    twin.run_training(4, 2)
    capsys.readouterr()
    a, b = state(m), state(twin)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(bits(m.ph_hat), bits(twin.ph_hat)) and np.array_equal(bits(m.th_hat), bits(twin.th_hat))
    assert m.cur_perplx[-2:] == twin.cur_perplx


def test_the_readers_of_the_hats_see_the_em_estimates():
    from lda_thesis_amd import attribution
    m, _, _ = build_model("k12")
    m.fit_em(5, chunk=CHUNK)
    th, ph = m.th_hat.copy(), m.ph_hat.copy()
    phi_t = np.ascontiguousarray(ph.T)
    doc_off, word, freq = csr(m)
    got = m.word_credit(top_m=2)
    want = attrref.attribute_ref(th, phi_t, doc_off, word, freq, top_m=2)
    assert np.array_equal(bits(got["credit"]), bits(want["credit"]))
    assert np.array_equal(np.concatenate(got["labels"]), want["site_idx"]) and np.array_equal(bits(np.concatenate(got["shares"])), bits(want["site_val"]))
    docs = [[m.v_to_w[w] for w, _ in t] for t in m.doc_tups[:12]]
    tups = [m.dicti.doc2bow(x) for x in docs]
    from lda_thesis_amd.corpus import csr_from_doc_tups
    off2, word2, freq2 = csr_from_doc_tups(tups)
    fold = m.fold_in_em(docs, iters=6)
    want = attrref.attribute_ref(attribution.uniform_start(None, len(docs), m.K), phi_t, off2, word2, freq2, iters=6, alpha=m.alpha)
    assert np.array_equal(bits(fold), bits(want["theta_out"]))
    # start="ph_hat": from the hats as they are; one more iteration from them is what fit_ref makes of them
    m.fit_em(1, start="ph_hat", chunk=CHUNK)
    want_th, want_phi = emref.fit_ref(th, phi_t, doc_off, word, freq, m.alpha, m.beta, 1, chunk=CHUNK)
    assert np.array_equal(bits(m.th_hat), bits(want_th)) and np.array_equal(bits(m.ph_hat), bits(np.ascontiguousarray(want_phi.T)))
    for bad in (dict(start="z"), dict(iters=-1), dict(theta_steps=0), dict(chunk=0), dict(trace_every=-1)):
        with pytest.raises(ValueError):
            m.fit_em(**bad)
