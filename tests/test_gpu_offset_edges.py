"""llda_sweep at the top of its 32-bit offsets (sizes, cases and samples: tests/offsetedge.py, pinned on the host
by tests/test_offset_edge_host.py).

The sweep kernels address their site arrays, the site records, the commit log and the quad kernels' 16-bit image as a uniform base plus
a 32-bit byte offset, and the host bounds every call so that the offsets fit.  No other test runs a call in the upper half of any of
these ranges, where an offset that is sign-extended or loses its top bit would first show.  Every sweep case here checks, after each of
two production sweeps (debug_margin = 0):

  1. chosen documents against the C oracle (snapshot semantics, as tests/test_gpu_fullsize.py samples them): the first and the last 150
     of every call, the 150 around the site whose byte offset is 2^31, 150 random ones;
  2. the WHOLE state (z, n_dk, counts) against a run of the same corpus, seed and options cut into calls of at most 2^26 sites (2^24
     where the kernels read 16-byte records), whose offsets stay below 2^28 bytes -- that run has its own 150 random documents against
     the oracle;
  3. count conservation, counts == a recount from the final assignments, the status word.

Everything is collected before the test fails, so that a failure names every group and every comparison that broke."""
import json
import os
import time

import numpy as np
import pytest
import torch

import offsetedge as oe
from test_gpu_fullsize import check_conservation

pytestmark = pytest.mark.gpu

ALPHA, BETA, SAMPLER_SEED = 0.1, 0.01, 42
_corpus = {}                              # at most one entry: key -> (word, freq, z), generated for the largest S of the key


def _free_corpus():
    _corpus.clear()
    torch.cuda.empty_cache()


def corpus(case):
    """(doc_off on the host, word, freq, z on the device) of the case: a prefix of its key's corpus, which stays until a case of another
    key asks"""
    key = oe.corpus_key(case)
    if key not in _corpus:
        _free_corpus()
        _corpus[key] = oe.generate(case.K, case.V, oe.key_sites(key))
    word, freq, z = _corpus[key]
    return oe.doc_offsets(case.S), word[:case.S], freq[:case.S], z[:case.S]


def need_memory(name, key=None):
    """skip only where the device has less than 1.25 x the measured peak of the case for it (what is free plus what this module holds)"""
    peak = oe.PEAK_BYTES.get(name)
    if key not in _corpus:
        _free_corpus()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    if peak is not None:
        have = torch.cuda.mem_get_info()[0] + torch.cuda.memory_allocated()
        if have < 1.25 * peak:
            _free_corpus()
            pytest.skip("%s needs %.1f GB, %.1f GB are free" % (name, 1.25 * peak / 1e9, have / 1e9))


def report(name, t0, **more):
    """the measured figures of DESIGN.md 4.4k, written where OFFSET_EDGE_REPORT points"""
    path = os.environ.get("OFFSET_EDGE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=name, seconds=round(time.time() - t0, 2), peak_bytes=torch.cuda.max_memory_allocated(), **more)) + "\n")


def gather(s, sel):
    """the documents ``sel`` of the sampler: (ids on the device, local CSR offsets, site indices on the device)"""
    sel_t = torch.from_numpy(sel).to(s.device)
    lens = s.doc_off[sel_t + 1] - s.doc_off[sel_t]
    loc_off = torch.zeros(len(sel) + 1, dtype=torch.int64, device=s.device)
    torch.cumsum(lens, 0, out=loc_off[1:])
    idx = torch.repeat_interleave(s.doc_off[sel_t] - loc_off[:-1], lens) + torch.arange(int(loc_off[-1]), device=s.device)
    return sel_t, loc_off.cpu().numpy(), idx


def sweep_and_check(s, c_oracle, groups, lab=None):
    """one HIP sweep of everything; the documents of ``groups`` (name -> ascending ids) must come out as the C oracle leaves them.
    -> the names of the groups that hold a document which did not"""
    sel = np.unique(np.concatenate(list(groups.values())))
    sel_t, loc_off, idx = gather(s, sel)
    n_k_v, n_zk = s.n_k_v(), s.n_zk()                       # sweep-start counts, reference layout
    word, freq = s.word[idx].cpu().numpy(), s.freq[idx].cpu().numpy()
    z0 = s._pos_topic[s.z[idx].to(torch.int64)].cpu().numpy()
    ndk0 = s.n_dk[sel_t][:, s._topic_pos].cpu().numpy().astype(np.int64)
    labs_sel = None
    if lab is not None:
        labs_sel = np.zeros((len(sel), s.K), dtype=np.uint8)
        labs_sel[np.repeat(np.arange(len(sel)), lab.shape[1]), lab[sel_t].cpu().numpy().reshape(-1)] = 1
    sweep = s.sweeps_done
    s.sweep()
    z_want, ndk_want = c_oracle.sweep_docs(sel + s.doc_base, loc_off, word, freq, z0, labs_sel, ndk0, n_k_v, n_zk, s.V, s.alpha, s.beta,
                                           s.seed, sweep, stream=s.stream_id, threads=min(oe.ORACLE_THREADS, os.cpu_count() or 1))
    z_got = s._pos_topic[s.z[idx].to(torch.int64)].cpu().numpy()
    ndk_got = s.n_dk[sel_t][:, s._topic_pos].cpu().numpy().astype(np.int64)
    assert int((z_want != z0).sum()) > z0.size // 2          # the sampled sites really move
    bad_site = np.add.reduceat((z_got != z_want).astype(np.int64), loc_off[:-1]) * (np.diff(loc_off) > 0)
    bad = sel[(bad_site > 0) | (ndk_got != ndk_want).any(axis=1)]
    return [g for g, ids in groups.items() if np.isin(ids, bad).any()]


def make(case, doc_off, word, freq, z, labs=None, **kw):
    from lda_thesis_amd.sampler import GibbsSampler
    return GibbsSampler(doc_off, word, freq, z, case.K, case.V, ALPHA, BETA, labs=labs, counts=None, seed=SAMPLER_SEED, **kw)


def assert_form(s, case):
    """which kernel llda_sweep launches for this sampler, through what selects it (csrc/sweep_plan.hpp)"""
    form, lay = case.form, s.layout
    assert s.debug_margin == 0 and (lay.KP, lay.G, lay.tail) == oe.GEOMETRY[case.K]
    rec = s.site_rec is not None
    assert rec == (case.unit == 16) and s.plan.call_limit == oe.call_limit(case)
    if form in ("quad", "quad_rec"):                       # llda_sweep_quad_kernel<4 / 3 / 2>: 4-byte arrays or records, position << 2
        assert s.quad and s.n_kw16 is not None and s.row16 is not None and s.site_row is None and s.commit_log is not None
        assert rec == (form == "quad_rec") and s.live_off is None and 0 < s.max_doc_tokens < 65536
    elif form == "two_doc16":                              # llda_sweep_kernel<.., R16, W4>: site_row
        assert not s.quad and s.n_kw16 is not None and s.site_row is not None and s.commit_log is not None and not rec
        assert 0 < s.max_doc_tokens < 65536
    elif form in ("int32_logged", "int32_rec"):            # the general tiered kernel with the log (and the records)
        assert not s.quad and s.n_kw16 is None and s.commit_log is not None and s.live_off is None
    elif form == "int32_atomics":                          # ... with n_kw_delta atomics (K = 100: padded positions)
        assert not s.quad and s.n_kw16 is None and s.commit_log is None and s.csc_pos is None and s.live_off is None
    elif form == "sparse8":                                # llda_sweep_sparse_kernel<8, KParams, 8>
        assert s.live_off is not None and s.live_max == 8 and s._heavy is None and s.commit_log is not None
        assert s.n_kw_img is not None and s.n_kw_img.element_size() == 1 and not s.quad and s.n_kw16 is None
    elif form == "wide_f32":                               # llda_sweep_wide_f32_kernel
        assert lay.wide and s._scratch is not None and 0 < s.max_doc_tokens < 32768 and s.live_off is None and s.commit_log is not None
    else:
        raise AssertionError(form)
    if form != "sparse8":
        assert s.dense_mask


@pytest.mark.parametrize("name", list(oe.CASES))
def test_sweep_at_the_offset_edge(c_oracle, monkeypatch, name):
    from lda_thesis_amd.sampler import GibbsSampler
    case = oe.CASES[name]
    t0 = time.time()
    need_memory(name, oe.corpus_key(case))
    off, word, freq, z = corpus(case)
    labs = lab = None
    if case.sparse:
        lab, z = oe.sparse_labels(case.S, case.K)
        labs = (np.arange(0, 8 * lab.shape[0] + 1, 8, dtype=np.int64), lab.reshape(-1).cpu().numpy())
    s = make(case, off, word, freq, z, labs, **case.kw)
    with monkeypatch.context() as m:                        # the same shard in calls whose offsets stay small
        m.setattr(GibbsSampler, "MAX_CALL_SITES", oe.SPLIT_LIMIT)
        m.setattr(GibbsSampler, "MAX_CALL_SITES_REC", oe.SPLIT_LIMIT_REC if case.unit == 16 else oe.SPLIT_LIMIT)
        t = make(case, off, word, freq, z, labs, **case.kw)
    del z
    assert s.S == case.S and s.D == len(off) - 1
    assert_form(s, case)
    calls = [(lo, hi) for lo, hi, _ in s._calls]
    assert calls == oe.call_ranges(off, oe.call_limit(case)) and len(calls) == case.calls
    assert len(t._calls) > 7 and [(lo, hi) for lo, hi, _ in t._calls] == oe.call_ranges(off, oe.call_limit(case, split=True))
    assert (t.quad, t.n_kw16 is None, t.site_rec is None, t.commit_log is None, t.n_kw_img is None, t._scratch is None) == \
           (s.quad, s.n_kw16 is None, s.site_rec is None, s.commit_log is None, s.n_kw_img is None, s._scratch is None)
    if name == "two_calls":
        assert len(s._calls) == 2 and s._calls[0][1] < s.D and int(off[s._calls[1][0]]) > 2 ** 30 - 2 * oe.N

    failed = []
    rng = np.random.default_rng(2025)
    for i in range(2):
        groups = oe.sample_groups(off, calls, case.unit, rng)
        assert "around" in groups
        failed += ["sweep %d, oracle group %s" % (i, g) for g in sweep_and_check(s, c_oracle, groups, lab)]
        own = {"random": np.sort(rng.choice(t.D, size=oe.GROUP, replace=False))}
        failed += ["sweep %d, split run, oracle group %s" % (i, g) for g in sweep_and_check(t, c_oracle, own, lab)]
        failed += ["sweep %d, whole state: %s" % (i, what) for what, a, b in (("z", s.z, t.z), ("n_dk", s.n_dk, t.n_dk), ("counts", s._counts, t._counts))
                   if not torch.equal(a, b)]
    peak = dict(split_calls=len(t._calls))
    del t
    torch.cuda.empty_cache()
    for what, check in (("status", s.check_status), ("conservation", lambda: check_conservation(s))):
        try:
            check()
        except (AssertionError, ValueError, RuntimeError) as e:
            failed.append("%s: %s" % (what, str(e)[:200]))
    # counts maintained incrementally == counts rebuilt from the final assignments (z_topics(), kept on the device)
    r = make(case, off, word, freq, s._pos_topic[s.z.to(torch.int64)], None, commit_log=False, rows16=False, image=0)
    failed += ["recount: %s" % what for what, a, b in (("n_kw", r.n_kw, s.n_kw), ("n_dk", r.n_dk, s.n_dk), ("n_k", r.n_k, s.n_k)) if not torch.equal(a, b)]
    report(name, t0, **peak)
    del r, s, word, freq, lab, labs
    torch.cuda.empty_cache()
    assert not failed, "%s: %s" % (name, "; ".join(failed))


@pytest.mark.parametrize("name", list(oe.VOCAB_CASES))
def test_quad_image_rows_at_the_vocabulary_edge(c_oracle, name):
    """K = 512, four documents per wavefront: the rows of the 16-bit image past byte 2^31 and at the top of the 32-bit offset, read as
    16 bits and -- where a planted count does not fit -- as int32.  Every document against the C oracle, which gets the columns of the
    3 000 used words only (renumbered in order) and the true V for V * beta."""
    from lda_thesis_amd.sampler import GibbsSampler
    V, K = oe.VOCAB_CASES[name], oe.VOCAB_K
    t0 = time.time()
    need_memory(name)
    doc_off, word, freq, z = oe.vocab_corpus(V)
    ids = oe.vocab_ids(V)
    ids_t = torch.from_numpy(ids).cuda()
    counts = oe.vocab_counts(V, doc_off, word, freq, z)
    s = GibbsSampler(doc_off, word, freq, z, K, V, ALPHA, BETA, labs=None, counts=counts, seed=SAMPLER_SEED, commit_log=True, quad=True)
    del counts
    torch.cuda.empty_cache()
    assert s.quad and s.n_kw16 is not None and s.row16 is not None and s.commit_log is not None and s.site_rec is None
    assert s.debug_margin == 0 and len(s._calls) == 1 and s.n_kw16.numel() == V * K and (V - 1) * 2 * K >= 2 ** 31
    new_word = oe.remap(ids, word)
    sel = np.arange(s.D)
    z_now, ndk_now = z.astype(np.int32), s.n_d_k()
    start_total = int(s.n_kw.sum(dtype=torch.int64))
    for i in range(2):
        n_k_v = s.n_kw[ids_t][:, s._topic_pos].t().contiguous().cpu().numpy().astype(np.int64)      # (K, 3000): the used columns
        n_zk = s.n_zk()
        s.sweep()
        # both paths ran in every band: rows flagged as fitting 16 bits, and rows that are read as int32
        flags = s.row16[ids_t].cpu().numpy().reshape(3, oe.BAND)
        assert ((flags == 1).sum(axis=1) > 300).all() and ((flags == 0).sum(axis=1) > 300).all()
        z_now, ndk_now = c_oracle.sweep_docs(sel, doc_off, new_word, freq, z_now, None, ndk_now, n_k_v, n_zk, V, ALPHA, BETA, SAMPLER_SEED, i,
                                             threads=min(oe.ORACLE_THREADS, os.cpu_count() or 1), row_len=len(ids))
        np.testing.assert_array_equal(s.z_topics(), z_now)
        np.testing.assert_array_equal(s.n_d_k(), ndk_now)
        assert int((z_now != z).sum()) > z.size // 2
    s.check_status()
    # the counts: the planted ones stay where they were, the corpus' own follow the assignments; no other row was touched
    want = np.zeros((K, len(ids)), dtype=np.int64)
    np.add.at(want, (z_now, new_word), freq)
    rows, topics, planted = oe.vocab_planted(V)
    np.add.at(want, (topics, np.searchsorted(ids, rows)), planted)
    np.testing.assert_array_equal(s.n_kw[ids_t][:, s._topic_pos].t().cpu().numpy().astype(np.int64), want)
    np.testing.assert_array_equal(s.n_zk(), want.sum(axis=1))
    assert int(s.n_kw.sum(dtype=torch.int64)) == start_total == int(want.sum())
    report(name, t0)
    del s
    torch.cuda.empty_cache()
