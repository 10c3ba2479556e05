"""What tests/test_gpu_offset_edges.py relies on, without a device: the sizes of tests/offsetedge.py are the edges they claim to be (the
site at byte 2^31 lies inside a sampled document; the top sizes are the host's limits and one more is refused, by sampler_plan.py and by
csrc/sweep_plan.hpp), the word bands of the vocabulary case straddle row 2^21 of the image, and the C oracle run on the columns of the
used words only equals the run on the whole matrix."""
import numpy as np
import pytest

import offsetedge as oe
import test_sweep_plan_host as sp
from lda_thesis_amd import sampler_plan as P

NO_CROSSING = {"two_calls": [1], "tail_half": [2]}      # calls that end before byte 2^31 of their widest site array
run_plans = sp.run_plans                  # (the fixture: the plan header compiled around a driver, nothing launched)


def test_sizes_are_the_edges():
    assert oe.S_TOP == P.MAX_CALL_SITES == 2 ** 30 - 1 and oe.R_TOP == P.MAX_CALL_SITES_REC == 2 ** 28 - 1
    assert oe.S_HALF == 2 ** 29 + 1_024_000 and oe.R_HALF == 2 ** 27 + 1_024_000 and oe.S_TWO == 2 ** 30 + 8192
    assert oe.V_HALF == 2 ** 21 + 1024 and oe.V_TOP == 2 ** 22 - 1
    # the last site of the *_HALF sizes is past byte 2^31, the first site of the *_TOP sizes' last document too
    assert (oe.S_HALF - 1) * 4 > 2 ** 31 and (oe.R_HALF - 1) * 16 > 2 ** 31 and (oe.V_HALF - 1) * 2 * 512 >= 2 ** 31
    assert (oe.S_TOP - 1) * 4 < 2 ** 32 <= oe.S_TOP * 4 + 4 and (oe.R_TOP - 1) * 16 < 2 ** 32 <= oe.R_TOP * 16 + 16
    assert (oe.V_TOP - 1) * 2 * 512 + 1023 < 2 ** 32 <= oe.V_TOP * 2 * 512 + 1024
    assert oe.SPLIT_LIMIT * 4 <= 2 ** 28 and oe.SPLIT_LIMIT_REC * 16 <= 2 ** 28


def test_layouts_of_the_cases():
    from lda_thesis_amd.layout import GroupLayout
    for K, (KP, G, tail) in oe.GEOMETRY.items():
        g = GroupLayout(K)
        assert (g.KP, g.G, g.tail) == (KP, G, tail), K
    assert {c.K for c in oe.CASES.values()} == set(oe.GEOMETRY)
    assert GroupLayout(2048).wide and not GroupLayout(512).wide


@pytest.mark.parametrize("name", list(oe.CASES))
def test_documents_calls_and_samples(name):
    case = oe.CASES[name]
    off = oe.doc_offsets(case.S)
    D = len(off) - 1
    lens = np.diff(off)
    assert int(off[-1]) == case.S and D == oe.n_docs(case.S) == 1 + -(-(case.S - oe.HEAD) // oe.N)
    assert lens[0] == oe.HEAD and (lens[1:-1] == oe.N).all() and 0 < lens[-1] <= oe.N
    assert case.S <= oe.key_sites(oe.corpus_key(case))
    # 16-byte records exactly where the layout has 8 or 16 lanes per document and the log is on
    G = oe.GEOMETRY[case.K][1]
    log = P.commit_log(case.kw.get("commit_log"), case.S, G)
    assert (case.unit == 16) == log.site_rec and log.call_limit == oe.call_limit(case)
    calls = oe.call_ranges(off, oe.call_limit(case))
    assert len(calls) == case.calls and calls[0][0] == 0 and calls[-1][1] == D
    assert all(a[1] == b[0] for a, b in zip(calls, calls[1:]))
    assert all(off[hi] - off[lo] <= oe.call_limit(case) for lo, hi in calls)
    split = oe.call_ranges(off, oe.call_limit(case, split=True))
    assert len(split) > 7
    assert all((off[hi] - off[lo]) * case.unit <= 2 ** 28 for lo, hi in split)
    # the site at byte 2^31 of a call lies strictly inside a document, and the "around" group holds it
    groups = oe.sample_groups(off, calls, case.unit, np.random.default_rng(1))
    crossed = [oe.crossing(off, lo, hi, case.unit) for lo, hi in calls]
    assert crossed[0] is not None and [i for i, c in enumerate(crossed) if c is None] == NO_CROSSING.get(name, [])
    if name == "two_calls":
        assert calls[0][1] < D and off[calls[1][0]] > 2 ** 30 - 2 * oe.N
    for i, c in enumerate(crossed):
        if c is not None:
            site, d = c
            # (a later call starts at a document boundary, HEAD sites off a multiple of N: its crossing site starts a document)
            assert (off[d] < site if i == 0 else off[d] == site) and site < off[d + 1] - 1 and d in groups["around"]
    assert set(groups) == {"first", "last", "around", "random"}
    assert len(groups["random"]) == oe.GROUP * (1 + sum(c is None for c in crossed))
    for lo, hi in calls:
        assert lo in groups["first"] and hi - 1 in groups["last"]
    for ids in groups.values():
        assert (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < D
    # the split run never has a crossing
    assert all(oe.crossing(off, lo, hi, case.unit) is None for lo, hi in split)


def test_sampler_plan_accepts_the_top_and_refuses_one_more():
    for S, G, rec in ((oe.S_TOP, 32, False), (oe.R_TOP, 8, True), (oe.R_TOP, 16, True)):
        log = P.commit_log(None, S, G)
        assert log.commit_log and log.site_rec == rec and S <= log.call_limit < S + 1
    facts = dict(rows16_ok=True, quad_ok=True, max_doc_tokens=0, tokens_max=lambda: oe.N, wide_share=lambda: 0.0, any_row_fits=lambda: True)
    assert P.rows(None, None, oe.S_TOP, 100_000, 512, **facts).form == "quad16"
    assert P.rows(None, None, oe.S_TOP + 1, 100_000, 512, **facts).form == "two_doc16"      # (log positions: the whole shard)
    assert P.rows(None, None, oe.S_TWO, 100_000, 512, **facts).form == "two_doc16"          # ... the two_calls case
    assert P.rows(None, True, 900_000, oe.V_TOP, 512, **facts).form == "quad16"
    assert P.rows(None, None, 900_000, oe.V_TOP + 1, 512, **facts).form == "two_doc16"
    with pytest.raises(ValueError):
        P.rows(None, True, 900_000, oe.V_TOP + 1, 512, **facts)
    with pytest.raises(ValueError):
        P.rows(None, True, oe.S_TOP + 1, 100_000, 512, **facts)


def test_sweep_plan_accepts_the_top_and_refuses_one_more(run_plans):
    Pn = 4096
    log = dict(csc_pos=Pn, commit_log=Pn)
    quad = dict(dense_mask=1, n_kw16=Pn, row16=Pn, max_doc_tokens=oe.N, **log)
    rows = dict(dense_mask=1, n_kw16=Pn, site_row=Pn, max_doc_tokens=oe.N, **log)
    L100, L128, L256, L512, L2048 = (sp.layout(K) for K in (100, 128, 256, 512, 2048))
    fine = [(L512, sp.args(n_sites=oe.S_TOP, **quad), "quad"), (L512, sp.args(n_sites=oe.S_TOP, **rows), "rows16"),
            (L512, sp.args(n_sites=oe.S_TOP, **log), "tiered"), (L512, sp.args(n_sites=oe.S_TOP), "tiered"),
            (L100, sp.args(n_sites=oe.S_TOP), "tiered"), (L2048, sp.args(n_sites=oe.S_TOP, max_doc_tokens=oe.N, **log), "wide_f32"),
            (L512, sp.args(n_sites=oe.S_TOP, live=Pn, live_max=8, n_kw_img=Pn, img_bits=8, **log), "sparse"),
            (L128, sp.args(n_sites=oe.R_TOP, site_rec=Pn, **quad), "quad"), (L256, sp.args(n_sites=oe.R_TOP, site_rec=Pn, **quad), "quad"),
            (L100, sp.args(n_sites=oe.R_TOP, site_rec=Pn, **quad), "quad"), (L128, sp.args(n_sites=oe.R_TOP, site_rec=Pn, **log), "tiered"),
            (L512, sp.args(V=oe.V_TOP, **quad), "quad")]
    more = [(L, dict(a, n_sites=a["n_sites"] + 1), f) for L, a, f in fine[:-1]] + [(L512, sp.args(V=oe.V_TOP + 1, **quad), "quad")]
    got = run_plans([(L, a) for L, a, _ in fine + more])
    sp.check([(L, a) for L, a, _ in fine + more], got)
    for (L, a, fam), g in zip(fine, got):
        assert g["rc"] == sp.OK and sp.FAMILIES[g["family"]] == fam, (L["K"], fam)
    for g in got[len(fine):]:
        assert g["rc"] == sp.BAD_ARG
    pad = {L["K"]: g["pad"] for (L, a, fam), g in zip(fine, got) if fam == "quad"}
    assert pad == {512: 0, 128: 0, 256: 0, 100: 1}
    tail = [g["has_tail"] for (L, a, fam), g in zip(fine, got) if L["K"] == 100 and fam == "tiered"]
    assert tail == [1]


@pytest.mark.parametrize("V", list(oe.VOCAB_CASES.values()))
def test_vocabulary_bands(V):
    b = oe.bands(V)
    assert b[0] + oe.BAND <= b[1] and b[1] + oe.BAND <= b[2] and b[2] + oe.BAND == V           # disjoint, the last ends the vocabulary
    assert b[1] < 2 ** 21 < b[1] + oe.BAND - 1 and (2 ** 21) * 2 * oe.VOCAB_K == 2 ** 31       # the middle one straddles byte 2^31
    ids = oe.vocab_ids(V)
    doc_off, word, freq, z = oe.vocab_corpus(V)
    assert len(doc_off) - 1 == oe.VOCAB_DOCS and (np.diff(doc_off) == oe.VOCAB_TOKENS).all()
    assert np.array_equal(np.unique(word), ids)                                                # every id of every band is used
    w = word.reshape(oe.VOCAB_DOCS, oe.VOCAB_TOKENS)
    assert (np.diff(w, axis=1) > 0).all()                                                      # ascending and distinct in a document
    for lo in b:
        assert (((w >= lo) & (w < lo + oe.BAND)).sum(axis=1) == oe.VOCAB_TOKENS // 3).all()    # every document mixes the bands
    rows, topics, counts = oe.vocab_planted(V)
    assert len(set(zip(rows.tolist(), topics.tolist()))) == len(rows)
    new = oe.remap(ids, word)
    assert (np.diff(new.reshape(w.shape), axis=1) > 0).all() and new.max() == len(ids) - 1
    for lo in b:                                                                               # in every band: rows beyond 16 bits,
        in_band = (rows >= lo) & (rows < lo + oe.BAND)                                         # rows with bit 15 set, plain rows
        wide, high = set(rows[in_band & (counts == oe.WIDE_COUNT)].tolist()), set(rows[in_band & (counts == oe.HIGH_COUNT)].tolist())
        assert len(wide) > 300 and len(high) > 300 and not wide & high and len(wide | high) < oe.BAND - 300
    assert oe.WIDE_COUNT > 65535 > oe.HIGH_COUNT + 3 * oe.VOCAB_DOCS > oe.HIGH_COUNT > 32768


def test_oracle_on_the_used_columns_equals_the_whole_matrix(c_oracle):
    """llda_oracle_sweep_docs with row_len: words renumbered in order, n_k_v cut to their columns, the true V for V * beta -- the same
    topics and counts, bit for bit, as the call on the whole (K, V) matrix; and a V that differs changes them"""
    rng = np.random.default_rng(27)
    K, V, D, n = 12, 5000, 40, 30
    ids = np.sort(rng.choice(V, size=200, replace=False))
    word = np.concatenate([np.sort(rng.choice(ids, size=n, replace=False)) for _ in range(D)]).astype(np.int32)
    used = np.unique(word)
    doc_off = (n * np.arange(D + 1)).astype(np.int64)
    freq = rng.integers(1, 5, word.size).astype(np.int32)
    z = rng.integers(0, K, word.size).astype(np.int64)
    labs = (rng.random((D, K)) < 0.6).astype(np.uint8)
    labs[np.repeat(np.arange(D), n), z] = 1
    doc = np.repeat(np.arange(D), n)
    n_d_k = np.zeros((D, K), dtype=np.int64)
    np.add.at(n_d_k, (doc, z), freq)
    n_k_v = rng.integers(0, 50, (K, V)).astype(np.int64)          # (counts of documents that are not in the selection)
    np.add.at(n_k_v, (z, word), freq)
    n_zk = n_k_v.sum(axis=1)
    doc_ids = np.arange(D) + 1000
    for lab in (labs, None):
        dense = c_oracle.sweep_docs(doc_ids, doc_off, word, freq, z, lab, n_d_k, n_k_v, n_zk, V, 0.1, 0.01, 5, 3, threads=2)
        cut = c_oracle.sweep_docs(doc_ids, doc_off, oe.remap(used, word), freq, z, lab, n_d_k, np.ascontiguousarray(n_k_v[:, used]),
                                  n_zk, V, 0.1, 0.01, 5, 3, threads=2, row_len=len(used))
        assert np.array_equal(dense[0], cut[0]) and np.array_equal(dense[1], cut[1])
        assert (dense[0] != z).sum() > z.size // 3
        other = c_oracle.sweep_docs(doc_ids, doc_off, oe.remap(used, word), freq, z, lab, n_d_k, np.ascontiguousarray(n_k_v[:, used]),
                                    n_zk, 10 ** 9, 0.1, 0.01, 5, 3, threads=2, row_len=len(used))
        assert not np.array_equal(other[0], dense[0])              # V is not the row length: it enters V * beta
