"""Host side of the second-trip tests (tests/secondtrip.py, tests/test_gpu_second_trip.py): the caps of the grid-stride launches as the
source states them, the geometry of the K the device tests run at, the kernel form csrc/sweep_plan.hpp picks for every wide sweep case,
and the properties the builders promise -- so that a cap that moves, a layout that changes or a builder that stops making the pairs
differ fails HERE, and the device tests never quietly stop reaching the second document of a workgroup."""
import os
import re

import numpy as np
import pytest

import attrref
import labelref
import secondtrip as st
from conftest import ROOT
from test_sweep_plan_host import FAMILIES, args as plan_args, layout as plan_layout, run_plans, wide_blocks  # noqa: F401 (run_plans: a fixture)

CSRC = os.path.join(ROOT, "lda_thesis_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(text, decl):
    """the value of the one line ``constexpr <decl> = <integer expression>;``"""
    found = re.findall(r"^constexpr %s = ([0-9 <*]+);" % re.escape(decl), text, flags=re.M)
    assert len(found) == 1, (decl, found)
    return int(eval(found[0], {"__builtins__": {}}))


def test_the_caps_are_the_ones_the_source_names():
    label, attr, hip = source("kernel_label.hpp"), source("kernel_attr.hpp"), source("llda_gibbs.hip")
    waves = constant(label, "int SETS_WAVES")
    assert constant(label, "int SETS_MAX_BLOCKS") * waves == st.SETS_CAP_DOCS and waves == 4
    assert constant(attr, "int64_t ATTR_LDS_MAX_BLOCKS") == st.ATTR_LDS_CAP
    # ... and the launches use them: a literal put back beside the name would pass the lines above
    assert "dim3((unsigned)(rounds < SETS_MAX_BLOCKS ? rounds : SETS_MAX_BLOCKS)), dim3(SETS_WAVES * 64)" in hip
    assert "const int64_t rounds = (a->D + SETS_WAVES - 1) / SETS_WAVES;" in hip
    assert "hipLaunchKernelGGL(llda_attr_lds_kernel<SITES>, doc_grid(P.D, ATTR_LDS_MAX_BLOCKS), dim3(64)" in hip
    assert "inline dim3 doc_grid(int64_t blocks, int64_t cap = 1 << 20) { return dim3((unsigned)(blocks < cap ? blocks : cap)); }" in hip
    # the wide launches (wide_blocks itself is pinned by tests/test_sweep_plan_host.py)
    assert wide_blocks(10 ** 9) == st.WIDE_CAP == wide_blocks(st.D_WIDE) and st.D_WIDE - st.WIDE_CAP == st.N_PAIRS
    assert "llda_foldin_init_wide_kernel, dim3(wide_blocks(P.n_sites)), dim3(64)" in hip
    assert "llda_foldin_wide_kernel, dim3(wide_blocks(P.D)), dim3(64)" in hip
    # K = 1025 is the first K of the attribution kernel that keeps its rows in LDS
    assert "doc_geom_is(1024, 0, 16)" in hip and "doc_geom_is(1025, 0, 0)" in hip and st.ATTR_K == 1025


@pytest.mark.parametrize("K", sorted(st.WIDE_GEOMETRY))
def test_geometry_of_the_wide_cases(K):
    lay = st.layout(K)
    assert lay.wide and (lay.KP, lay.T, lay.NT) == st.WIDE_GEOMETRY[K] and lay.G == 64 * lay.NT
    if K == st.FOLDIN_K:
        assert not st.layout(K - 1).wide                          # the first wide layout
    else:
        assert K in st.SWEEP_KS and st.D_WIDE * lay.KP * 4 < 60e6     # n_dk on the device: 25 and 50 MB


@pytest.mark.parametrize("name", sorted(st.SWEEP_CASES))
def test_every_sweep_case_takes_the_form_it_is_named_after(run_plans, name):
    """the plan of llda_sweep for the arguments the device test passes: family, SLIM / COMPACT / TIERED, one wavefront per workgroup,
    WIDE_CAP workgroups"""
    K, margin, tiny, heavy, want = st.SWEEP_CASES[name]
    doc_off, _, freq, _, _ = st.sweep_corpus(K, heavy)
    L = plan_layout(K)
    alpha, beta = st.sweep_priors(tiny)
    tokens = int(np.add.reduceat(np.append(freq, 0).astype(np.int64), doc_off[:-1])[np.diff(doc_off) > 0].max())
    assert (tokens >= 32768) == heavy
    a = plan_args(dm=margin, D=st.D_WIDE, V=st.SWEEP_V, n_sites=int(doc_off[-1]), dense_mask=0, alpha=alpha, beta=beta,
                  scratch=4096, scratch_bytes=st.WIDE_CAP * L["KP"] * 8, max_doc_tokens=tokens)
    got = run_plans([(L, a)])[0]
    assert got["rc"] == 0 and FAMILIES[got["family"]] == want["family"], got
    for field in ("slim", "compact", "tiered"):
        if field in want:
            assert got[field] == want[field], (field, got)
    assert got["grid"] == st.WIDE_CAP and got["block"] == 64 and got["nt"] == L["tiers"] == st.WIDE_GEOMETRY[K][2]
    if name.endswith("all_rare"):
        assert got["m0"] == 2.0 and got["margin_rel"] == 2.0      # no tier decides a site
    elif want["family"] == "wide_f32":
        assert 0 < got["m0"] < 1e-4 and got["margin_rel"] == 2.0 ** -40


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("K", st.SWEEP_KS)
def test_sweep_corpus_pairs_differ(K, heavy):
    doc_off, word, freq, labs, z = st.sweep_corpus(K, heavy)
    D = st.D_WIDE
    assert len(doc_off) == D + 1 and labs.shape == (D, K) and word.max() < st.SWEEP_V and freq.min() >= 1
    lens = np.diff(doc_off)
    assert lens.min() == 0 and lens.max() == 3 and int(doc_off[-1]) > st.WIDE_CAP
    assert freq.max() == (st.HEAVY_FREQ if heavy else 3)
    n_labs = labs.sum(axis=1)
    assert (labs[:, 0] == 1).all() and n_labs.min() >= 5 and n_labs.max() == 6 and (labs.sum(axis=0) > 0).sum() > K // 2
    pairs = st.trip_pairs(D, st.WIDE_CAP)
    assert pairs == [(d, d + st.WIDE_CAP) for d in range(st.N_PAIRS)]
    st.assert_pairs_differ(pairs, doc_off, labs, z, freq, heavy)
    # the documents in reverse: every pair the other way round, and still all of it
    back = st.trip_pairs(D, st.WIDE_CAP, np.arange(D)[::-1])
    assert back == [(D - 1 - i, D - 1 - i - st.WIDE_CAP) for i in range(st.N_PAIRS)]
    st.assert_pairs_differ(back, doc_off, labs, z, freq, heavy)
    if heavy:
        d, sh = st.HEAVY_DOC, st.shared_label(st.HEAVY_DOC, K)
        n_d_k, _, _ = st.counts(doc_off, word, freq, z, K, st.SWEEP_V)
        assert n_d_k[d, sh] >= st.HEAVY_FREQ and 0 < n_d_k[d + st.WIDE_CAP, sh] <= 9


def test_sweep_corpus_properties_are_not_vacuous():
    """assert_pairs_differ turns down pairs that are not what it asks for"""
    doc_off, word, freq, labs, z = st.sweep_corpus(1100)
    with pytest.raises(AssertionError):                           # neighbours share no label but the root
        st.assert_pairs_differ([(d, d + 1) for d in range(st.N_PAIRS)], doc_off, labs, z, freq)
    same = labs.copy()
    same[st.WIDE_CAP:] = same[:st.N_PAIRS]
    with pytest.raises(AssertionError):                           # equal masks
        st.assert_pairs_differ(st.trip_pairs(st.D_WIDE, st.WIDE_CAP), doc_off, same, z, freq)
    with pytest.raises(AssertionError):                           # not every kind of length change
        st.assert_pairs_differ(st.trip_pairs(st.D_WIDE, st.WIDE_CAP)[2:5], doc_off, labs, z, freq)


@pytest.mark.parametrize("zero_word", [False, True])
def test_foldin_corpus_reaches_the_second_trip_of_both_launches(zero_word):
    c = st.foldin_corpus(zero_word)
    st.assert_foldin_sites_differ(c)
    assert ((c["word"] == st.FOLDIN_V - 1).sum() > 3) == zero_word and c["word"].max() < st.FOLDIN_V
    assert set(c["init_idx"].tolist()) == set(range(st.FOLDIN_ROWS))
    sub = st.FOLDIN_SUBSET
    assert set(range(st.N_PAIRS)) <= set(sub) and set(range(st.WIDE_CAP, st.D_WIDE)) <= set(sub) and len(set(sub)) == len(sub)
    others = [d for d in sub if st.N_PAIRS <= d < st.WIDE_CAP]
    assert len(others) >= 100 and min(others) < 100 and max(others) > st.WIDE_CAP - 100
    t = st.take_documents(c, sub, doc_ids=1000 + np.asarray(sub))
    assert (np.diff(t["doc_off"]) == np.diff(c["doc_off"])[list(sub)]).all() and (t["word"] == c["word"][t["sites"]]).all()
    # the rotation of the device-against-device check gives every document another partner and the first nine the second trip
    D, r = st.D_WIDE, st.FOLDIN_ROTATE
    order = (np.arange(D) + r) % D
    before = dict(st.trip_pairs(D, st.WIDE_CAP))
    after = st.trip_pairs(D, st.WIDE_CAP, order)
    assert [b for _, b in after] == list(range(r)) and all(before.get(a) != b for a, b in after)


@pytest.mark.parametrize("K", st.SETS_KS)
def test_label_sets_plants_do_what_they_are_there_for(K):
    score, thr, truth = st.sets_case(K)
    assert score.shape == (st.SETS_D, K + 3) and truth.shape == (st.SETS_D, K) and st.SETS_D == st.SETS_CAP_DOCS + 5
    want = [labelref.label_sets(score, thr, truth, first=st.SETS_FIRST, at_least_one=bool(alo), K=K) for alo in (0, 1)]
    st.assert_sets_plants(K, *want)
    for w in want:                                                # the counters of the labels get their share in both trips
        first, second = (w["mask"][:st.SETS_CAP_DOCS] & (truth[:st.SETS_CAP_DOCS] != 0)), (w["mask"][st.SETS_CAP_DOCS:] & (truth[st.SETS_CAP_DOCS:] != 0))
        assert first.any() and second.any() and w["tp"].sum() > 0 and w["fp"].sum() > 0 and w["fn"].sum() > 0


def test_attr_case_pairs_differ():
    c = st.attr_case()
    st.assert_attr_pairs_differ(c)
    assert c["theta"].shape == (12, st.ATTR_K) and len(c["doc_off"]) == st.ATTR_D + 1 and st.ATTR_D == st.ATTR_LDS_CAP + 6
    lens = np.diff(c["doc_off"])
    assert np.flatnonzero(lens).tolist() == list(st.ATTR_LIVE)
    assert st.ATTR_D * st.ATTR_K * 8 > 500e6                      # (what the device test says about its memory)
    want = attrref.attribute_ref(c["theta"], c["phi_t"], c["sub_off"], c["word"], c["freq"], K=st.ATTR_K, V=c["V"], **st.ATTR_SETTINGS)
    assert want["tok"].min() > 0 and want["bad"].sum() > 0        # every document takes its EM steps, and sites that do not count are met
    moved = (want["theta_out"].view(np.uint64) != c["theta"].view(np.uint64)).any(axis=1)
    assert moved.all() and (want["site_idx"][:, 0] >= 0).any() and (want["site_idx"][:, -1] < 0).any()
