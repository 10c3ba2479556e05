"""The second document a workgroup takes.  Kernels that cap their grid walk their documents with a stride (``for (d = blockIdx.x; d < D;
d += gridDim.x)``) and carry state from one document to the next in LDS, in registers or in a scratch row of the workgroup: cached
fp64 / fp32 factors, int16 count changes, LDS copies of n_dk / n_k, mask words, tp / fp / fn counters.  State that is not rebuilt is no
crash, only a wrong topic in document d + cap -- which no test reached for the kernels below.  Every case here has a few documents more
than one trip of the grid holds (tests/secondtrip.py: the pairs differ in masks and lengths, and the second has tokens on a topic
both allow), and everything is compared exactly: integers, or float64 as uint64.

  wide sweeps      llda_sweep_wide_f32_kernel FAT and SLIM, llda_sweep_wide_reg_kernel COMPACT and not, llda_sweep_wide_kernel tiered and
                   all-exact; WIDE_CAP = 4096 workgroups of one wavefront; against the C oracle, two sweeps of D = 4105 documents
  wide fold-in     llda_foldin_init_wide_kernel (a workgroup per SITE) and llda_foldin_wide_kernel, same cap; against tests/foldinref.py on
                   a fixed subset, device against device on every document
  llda_label_sets  1024 workgroups of 4 wavefronts: 4096 documents a trip; against tests/labelref.py, the LDS counters over both trips
  llda_attribute   K > 1024 (llda_attr_lds_kernel): 65 536 workgroups; against tests/attrref.py on the twelve documents with sites

The caps, the geometry of every K and the kernel form every sweep case selects are pinned on the host (tests/test_second_trip_host.py).

Left out, because their launches cap at 2^20 workgroups and a second trip needs millions of documents: doc_grid() with its default cap
(the held-out wave, wide and group kernels, the attribution wave and group kernels: 2^20 workgroups of 4 wavefronts or of 64 / G
documents each), llda_leftright_kernel (2^20 workgroups of one document), llda_rank_labels_kernel (2^20 tiles) and
llda_ecdf_totals_kernel (2^20 rounds).  The wide sparse-label sweep has no cap at all: ceil(D / documents per workgroup) workgroups."""
import functools

import numpy as np
import pytest

import attrref
import labelref
import secondtrip as st

pytestmark = pytest.mark.gpu

SWEEP_SEED, SWEEP_DOC_BASE = 77, 1000
REVERSED = ("k1100_f32_fat", "k2047_f32_slim_all_rare")          # cases that run once more with the documents taken in reverse


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------------------------
# 1. wide sweeps against the C oracle
# ------------------------------------------------------------------------------------------------
def differing_documents(doc_off, got_z, want_z, pairs):
    """which documents hold a site that differs, and their place in a workgroup's trips -- for the message of a failure"""
    sites = np.flatnonzero(np.asarray(got_z) != np.asarray(want_z))
    docs = sorted(set((np.searchsorted(doc_off, sites, side="right") - 1).tolist()))
    second = set(b for _, b in pairs)
    return "%d sites in %d documents differ; of the second trip: %s; others: %s" % (
        sites.size, len(docs), [d for d in docs if d in second], [d for d in docs if d not in second][:10])


@pytest.mark.parametrize("name,reverse", [(n, False) for n in sorted(st.SWEEP_CASES)] + [(n, True) for n in REVERSED])
def test_wide_sweep_second_trip_against_c_oracle(c_oracle, name, reverse):
    import torch
    from lda_thesis_amd.sampler import GibbsSampler
    K, margin, tiny, heavy, _ = st.SWEEP_CASES[name]
    doc_off, word, freq, labs, z = st.sweep_corpus(K, heavy)
    alpha, beta = st.sweep_priors(tiny)
    D, V, S = st.D_WIDE, st.SWEEP_V, int(doc_off[-1])
    s = GibbsSampler(doc_off, word, freq, z, K, V, alpha, beta, labs=labs, seed=SWEEP_SEED, doc_base=SWEEP_DOC_BASE, sort_docs=False,
                     sparse_labels=False)
    # what selects the kernel form (csrc/sweep_plan.hpp; the host test holds the plan itself against SWEEP_CASES)
    assert s.layout.wide and s.layout.NT == st.WIDE_GEOMETRY[K][2] and s.layout.KP == st.WIDE_GEOMETRY[K][0]
    assert s.live_off is None and not s.dense_mask and s._scratch is not None and s.D == D and len(s._calls) == 1
    assert s.max_doc_tokens >= 32768 if heavy else 0 < s.max_doc_tokens < 32768
    assert s.doc_order is None                                    # the documents in their own order: the pairs are (d, d + WIDE_CAP)
    order = None
    if reverse:
        order = np.arange(D)[::-1].copy()
        s.doc_order = torch.from_numpy(order.astype(np.int32)).to(s.device)
    pairs = st.trip_pairs(D, st.WIDE_CAP, order)
    st.assert_pairs_differ(pairs, doc_off, labs, z, freq, heavy)
    s.debug_margin = margin
    n_dk0, n_kv0, n_k0 = s.n_d_k(), s.n_k_v(), s.n_zk()
    for got, want in zip((n_dk0, n_kv0, n_k0), st.counts(doc_off, word, freq, z, K, V)):
        np.testing.assert_array_equal(got, want)
    cs = c_oracle.CState(doc_off, word, freq, z, labs, n_dk0, n_kv0, n_k0, V, alpha, beta)
    for i in range(2):
        s.sweep()
        cs.sweep(1, SWEEP_SEED, i, doc_base=SWEEP_DOC_BASE, threads=4)
        what = "%s sweep %d" % (name, i)
        got_z = s.z_topics()
        assert np.array_equal(got_z, cs.z), what + ": " + differing_documents(doc_off, got_z, cs.z, pairs)
        np.testing.assert_array_equal(s.n_d_k(), cs.n_d_k, err_msg=what)
        np.testing.assert_array_equal(s.n_k_v(), cs.n_k_v, err_msg=what)
        np.testing.assert_array_equal(s.n_zk(), cs.n_zk, err_msg=what)
        if name.endswith("all_rare"):                             # every site through the rare tiers, the exact pipeline included
            assert int(s.status[2]) == (i + 1) * S and int(s.status[1]) == (i + 1) * S
    s.check_status()
    assert not np.array_equal(cs.z, z)                            # (the sweeps moved something)


# ------------------------------------------------------------------------------------------------
# 2. wide fold-in
# ------------------------------------------------------------------------------------------------
def foldin_case(setting):
    import test_gpu_foldin_direct as fd
    assert fd.V == st.FOLDIN_V and len(fd.make_init_rows(st.FOLDIN_K)) == st.FOLDIN_ROWS
    corpus = st.foldin_corpus(fd.SETTINGS[setting]["beta_fallback"])
    c = fd.make_case(st.FOLDIN_K, setting, iters=2, thinning=1, **corpus)
    st.assert_foldin_sites_differ(c)
    return c


@functools.lru_cache(maxsize=None)
def foldin_device(setting, start, rotated=False):
    """the outputs of one llda_foldin call over all D documents; rotated: the documents FOLDIN_ROTATE .. D - 1, 0 .. FOLDIN_ROTATE - 1 in
    that order with their ids and streams spelled out, so that every document keeps its key"""
    import test_gpu_foldin_direct as fd
    c = foldin_case(setting)
    lay = st.layout(st.FOLDIN_K)
    assert lay.wide and lay.KP == st.WIDE_GEOMETRY[st.FOLDIN_K][0]
    if rotated:
        order = (np.arange(st.D_WIDE) + st.FOLDIN_ROTATE) % st.D_WIDE
        c = st.take_documents(c, order, doc_ids=c["doc_base"] + order, doc_stream=np.full(st.D_WIDE, fd.STREAM, dtype=np.uint64), doc_base=7)
    got = fd.device(c, start)
    assert got["status"] == 0
    return c, got


@functools.lru_cache(maxsize=None)
def foldin_reference(setting):
    """tests/foldinref.py on FOLDIN_SUBSET (a document's outputs depend on its own inputs and key only)"""
    import test_gpu_foldin_direct as fd
    c = foldin_case(setting)
    sub = st.take_documents(c, st.FOLDIN_SUBSET, doc_ids=c["doc_base"] + np.asarray(st.FOLDIN_SUBSET))
    want = fd.reference(sub)
    assert not want["raises"].any()
    return sub, want


@pytest.mark.parametrize("start", ["sites", "inside"])
@pytest.mark.parametrize("setting", ["flat", "llda"])
def test_wide_foldin_second_trip_against_foldinref(setting, start):
    c, got = foldin_device(setting, start)
    sub, want = foldin_reference(setting)
    ids = np.asarray(st.FOLDIN_SUBSET)
    what = "K=%d %s %s" % (st.FOLDIN_K, setting, start)
    # (a) the subset, bit for bit
    for i, d in enumerate(ids):
        a, b = slice(int(sub["doc_off"][i]), int(sub["doc_off"][i + 1])), slice(int(c["doc_off"][d]), int(c["doc_off"][d + 1]))
        msg = "%s document %d (%d sites)" % (what, d, b.stop - b.start)
        np.testing.assert_array_equal(got["z"][b], want["z"][a], err_msg=msg + ": z")
        np.testing.assert_array_equal(got["n_dk"][d], want["n_dk"][i], err_msg=msg + ": n_dk")
        np.testing.assert_array_equal(bits(got["th"][d]), bits(want["th"][i]), err_msg=msg + ": th")
    # (c) every document (fd.device has already held every z against the layout and the padding against zero)
    lens = np.diff(c["doc_off"])
    tokens = np.add.reduceat(np.append(c["freq"], 0).astype(np.int64), c["doc_off"][:-1]) * (lens > 0)
    np.testing.assert_array_equal(got["n_dk"].sum(axis=1), tokens, err_msg=what)
    assert got["n_dk"].min() >= 0 and ((got["z"] >= 0) & (got["z"] < st.FOLDIN_K)).all()
    assert not bits(got["th"][lens == 0]).any() and not got["n_dk"][lens == 0].any(), what + ": an empty document"
    doc =np.repeat(np.arange(st.D_WIDE), lens)
    assert (got["n_dk"][doc, got["z"]] >= c["freq"]).all(), what + ": a site's topic holds fewer tokens than the site"


@pytest.mark.parametrize("setting", ["flat", "llda"])
def test_wide_foldin_every_document_device_against_device(setting):
    """(b) both start paths leave the same outputs for ALL documents; and so does a call on the corpus rotated by nine documents, in
    which every document has another partner and the first nine are the second trip"""
    c, inside = foldin_device(setting, "inside")
    _, sites = foldin_device(setting, "sites")
    for n in ("z", "n_dk", "th"):
        assert np.array_equal(bits(inside[n]), bits(sites[n])), "%s: inside and sites differ in %s" % (setting, n)
    rc, rot = foldin_device(setting, "sites", True)
    order = (np.arange(st.D_WIDE) + st.FOLDIN_ROTATE) % st.D_WIDE
    assert dict(st.trip_pairs(st.D_WIDE, st.WIDE_CAP, order)) == {d + st.FOLDIN_ROTATE: d for d in range(st.N_PAIRS)}
    assert np.array_equal(rot["z"], sites["z"][rc["sites"]]), setting + ": z after the rotation"
    assert np.array_equal(rot["n_dk"], sites["n_dk"][order]), setting + ": n_dk after the rotation"
    assert np.array_equal(bits(rot["th"]), bits(sites["th"][order])), setting + ": th after the rotation"


# ------------------------------------------------------------------------------------------------
# 3. llda_label_sets
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alo", [0, 1])
@pytest.mark.parametrize("K", st.SETS_KS)
def test_label_sets_second_trip_against_labelref(K, alo):
    import test_gpu_label_sets as tls
    score, thr, truth = st.sets_case(K)
    D, first = st.SETS_D, st.SETS_FIRST
    assert D == st.SETS_CAP_DOCS + 5
    wants = [labelref.label_sets(score, thr, truth, first=first, at_least_one=bool(a), K=K) for a in (0, 1)]
    st.assert_sets_plants(K, *wants)
    want = wants[alo]
    what = "K=%d D=%d at_least_one=%d" % (K, D, alo)
    tls.check(tls.run(score, thr, truth, K, first, alo), want, D, K, what=what)
    tls.check(tls.run(score, thr, None, K, first, alo), want, D, K, with_truth=False, what=what + " truth=NULL")


# ------------------------------------------------------------------------------------------------
# 4. llda_attr_lds_kernel
# ------------------------------------------------------------------------------------------------
def test_attr_lds_second_trip_against_attrref():
    """D = 65 542 documents of K = 1025 loads: theta, theta_out and credit are 537 MB each and made on the device; the twelve documents
    with sites against tests/attrref.py bit for bit, every other document against its own loads"""
    import torch
    from lda_thesis_amd import _native
    import test_gpu_attribute as ta
    c = st.attr_case()
    st.assert_attr_pairs_differ(c)
    K, D, V, live = st.ATTR_K, st.ATTR_D, c["V"], list(st.ATTR_LIVE)
    iters, alpha, top_m = (st.ATTR_SETTINGS[n] for n in ("iters", "alpha", "top_m"))
    assert D == st.ATTR_LDS_CAP + 6 and live[6:] == [d + st.ATTR_LDS_CAP for d in live[:6]]
    want = attrref.attribute_ref(c["theta"], c["phi_t"], c["sub_off"], c["word"], c["freq"], K=K, V=V, iters=iters, alpha=alpha, top_m=top_m)
    assert want["tok"].min() > 0 and want["bad"].sum() > 0 and not np.array_equal(bits(want["theta_out"]), bits(c["theta"]))

    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(26)
    theta = torch.rand((D, K), dtype=torch.float64, device=dev, generator=gen)
    theta[up(np.asarray(live))] = up(c["theta"])
    S, G = int(c["doc_off"][-1]), ta.GUARD
    sizes = dict(theta_out=D * K, credit=D * K, site_idx=S * top_m, site_val=S * top_m, tok=D, bad=D)
    bufs = {n: torch.full((sizes[n] + 2 * G,), ta.PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in ta.OUTPUTS}
    _native.attribute(up(c["doc_off"]), up(c["word"]), up(c["freq"]), theta, up(c["phi_t"]), D, V, K, iters=iters, alpha=alpha, top_m=top_m,
                      ld_theta=K, ld_phi=K, ld_out=K, ld_credit=K, **{n: b[G:G + sizes[n]] for n, b in bufs.items()})
    torch.cuda.synchronize()
    for n, dt in ta.OUTPUTS:
        pat = ta.PATTERN[dt]
        assert (bufs[n][:G].cpu().numpy() == pat).all() and (bufs[n][G + sizes[n]:].cpu().numpy() == pat).all(), "guard words around " + n
    theta_out, credit = (bufs[n][G:G + D * K].view(D, K) for n in ("theta_out", "credit"))
    rows = up(np.asarray(live))
    got = dict(theta_out=theta_out[rows].cpu().numpy(), credit=credit[rows].cpu().numpy(),
               site_idx=bufs["site_idx"][G:G + S * top_m].cpu().numpy().reshape(S, top_m),
               site_val=bufs["site_val"][G:G + S * top_m].cpu().numpy().reshape(S, top_m),
               tok=bufs["tok"][G:G + D].cpu().numpy(), bad=bufs["bad"][G:G + D].cpu().numpy())
    for n in ("theta_out", "credit", "site_idx", "site_val"):
        diff = np.argwhere(bits(got[n]) != bits(want[n]))
        assert diff.shape[0] == 0, "%s differs at %s (rows: the documents %s)" % (n, diff[:5].tolist(), live)
    for n in ("tok", "bad"):
        np.testing.assert_array_equal(got[n][live], want[n], err_msg=n)
    # the documents without sites keep their loads and earn nothing: 64 of them on the host ...
    empty = np.linspace(6, st.ATTR_LDS_CAP - 1, 64).astype(np.int64)
    assert len(set(empty.tolist())) == 64 and not set(empty.tolist()) & set(live)
    e = up(empty)
    assert np.array_equal(bits(theta_out[e].cpu().numpy()), bits(theta[e].cpu().numpy()))
    assert not bits(credit[e].cpu().numpy()).any()
    is_live = np.zeros(D, dtype=bool)
    is_live[live] = True
    assert not got["tok"][~is_live].any() and not got["bad"][~is_live].any()
    # ... and all of them on the device
    changed = (theta_out.view(torch.int64) != theta.view(torch.int64)).any(dim=1).cpu().numpy()
    earned = (credit.view(torch.int64) != 0).any(dim=1).cpu().numpy()
    assert not changed[~is_live].any() and not earned[~is_live].any()
    assert changed[is_live].all() and earned[is_live].all()
