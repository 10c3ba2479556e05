"""Which kernel form the sampler picks (selection policy, not parity).  The file name sorts after every parity file: under
`pytest -x` a policy expectation that no longer holds cannot hide parity tests behind it."""
import pytest

pytestmark = pytest.mark.gpu


def test_16_bit_rows_are_chosen_by_document_and_n_kw_size():
    """rows16=None: on wherever every document is below 2^16 tokens (the four-wave form: faster than int32 rows at every size); with
    longer documents (three waves) only when n_kw is at least GibbsSampler.ROWS16_MIN_BYTES"""
    import torch
    from lda_thesis_amd.corpus import synthetic_corpus_blocks
    from lda_thesis_amd.sampler import GibbsSampler
    for zipf, V, long_doc, want in ((0.0, 1_000_000, False, True), (1.0, 100_000, False, True), (0.0, 20_000, False, True),
                                    (0.0, 20_000, True, False), (1.0, 100_000, True, True)):
        off, w, f, z = synthetic_corpus_blocks(0, 8000, 300, V, 512, 1234, "cuda", zipf_s=zipf, block=4000)
        if long_doc:
            f = f.clone()
            f[0] = 70000                                                  # one document of 70 299 tokens
        s = GibbsSampler(off, w, f, z, 512, V, 0.1, 0.01, labs=None, seed=1)
        assert (s.n_kw16 is not None) == want, (zipf, V, long_doc)
        # K = 512 with every document below 2^16 tokens: four documents per wavefront, flags per word from the library instead of
        # per-site row starts
        assert s.quad == (want and not long_doc)
        assert (s.site_row is not None) == (want and long_doc)
        if want:
            assert (0 < s.max_doc_tokens < 65536) == (not long_doc)
        s.sweep()
        s.check_status()
        del s


# ---- the sampler builds what sampler_plan.py says, on the smallest shapes that reach each branch ----
def _corpus(K, n_labels=0, long_doc=False, wide_doc=0, D=40, N=20, V=300):
    """D documents of N distinct words (f = 1), dense or with root + n_labels - 1 random labels each; long_doc: document 0 holds
    70 000 tokens; wide_doc: document 1 allows that many topics"""
    import numpy as np
    rng = np.random.RandomState(7)
    off = np.arange(D + 1, dtype=np.int64) * N
    word = np.concatenate([np.sort(rng.choice(V, N, replace=False)) for _ in range(D)]).astype(np.int32)
    freq = np.ones(D * N, dtype=np.int32)
    if long_doc:
        freq[0] = 70000 - (N - 1)
    if not n_labels:
        return off, word, freq, rng.randint(0, K, D * N), None
    sets = [np.concatenate([[0], 1 + np.sort(rng.choice(K - 1, (wide_doc if d == 1 and wide_doc else n_labels) - 1, replace=False))])
            for d in range(D)]
    z = np.concatenate([rng.choice(s, N) for s in sets])
    lab_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return off, word, freq, z, (lab_off, np.concatenate(sets).astype(np.int64))


def _check_against_plan(s, commit_log, rows16, quad, image, image_order):
    """every array the sampler holds is the one sampler_plan names for the facts the sampler measured -> the plan"""
    import torch
    from lda_thesis_amd import _native, sampler_plan as P
    lay = s.layout
    log = P.commit_log(commit_log, s.S, lay.G, s.MAX_CALL_SITES, s.MAX_CALL_SITES_REC)
    assert (s.commit_log is not None, s.site_rec is not None, s._call_limit) == tuple(log)
    assert (s.csc_pos is not None) == log.commit_log
    sparse, heavy = s.live_off is not None, 0 if s._heavy is None else int(s._heavy.sum())
    assert (s._scratch is not None) == P.scratch(lay.wide, s.D, sparse, heavy)
    opt = P.options(rows16, quad, image)
    assert s._quad_wanted == opt.quad
    r16ok, qok = _native.rows16_ok(s.K), _native.quad_ok(s.K)
    rows = P.Rows("int32", False, s.max_doc_tokens)
    if P.rows_possible(opt.rows16, opt.quad, s.S, s.dense_mask, log.commit_log, r16ok, qok, s.alpha, s.beta):
        assert not lay.wide                                     # (max_doc_tokens was 0 before the rows were decided)
        rows = P.rows(opt.rows16, opt.quad, s.S, s.V, lay.KP, r16ok, qok, 0, s._tokens_max, s._wide_share,
                      lambda: bool(s._rows16_fits().any()), s.ROWS16_MIN_BYTES, s.QUAD_MAX_WIDE_SITES)
    assert s.quad == (rows.form == "quad16") and (s.site_row is not None) == (rows.form == "two_doc16")
    assert (s.n_kw16 is not None) == (s.row16 is not None) == (rows.form != "int32")
    assert s.max_doc_tokens == rows.max_doc_tokens
    bits = P.image_bits(opt.image, s.S, s.V, lay.KP, sparse, s.live_max, s.alpha, s.beta, s._image_escape_rates,
                        s.IMAGE_MIN_BYTES, s.IMAGE_MIN_SITES, s.IMAGE_MAX_ESCAPES)
    assert (None if s.n_kw_img is None else s.n_kw_img.dtype) == {0: None, 8: torch.uint8, 16: torch.int16}[bits]
    ordered = bool(bits) and P.image_order_possible(image_order, lay.KP, bits)
    assert (s.image_lines_per_site is not None) == ordered
    ordered = ordered and P.image_order_taken(image_order, *s.image_lines_per_site)
    assert (s._img_src is not None) == (s._img_col is not None) == ordered
    plan = P.SamplerPlan(commit_log=log.commit_log, site_rec=log.site_rec, call_limit=log.call_limit, sparse=sparse, heavy_docs=heavy,
                         scratch=s._scratch is not None, rows=rows.form, max_doc_tokens=rows.max_doc_tokens, image_bits=bits,
                         image_order=ordered)
    assert s.plan == plan
    return plan


SHAPES = {
    # name: (K, corpus arguments, sampler arguments, environment, the fields of the plan that the shape is there for)
    "k512_quad": (512, {}, {}, {}, dict(rows="quad16", site_rec=False)),
    "k512_quad_off": (512, {}, {}, dict(LLDA_QUAD="off"), dict(rows="two_doc16")),
    "k512_long_rows16": (512, dict(long_doc=True), dict(rows16=True), {}, dict(rows="two_doc16")),
    "k512_long_auto": (512, dict(long_doc=True), {}, {}, dict(rows="int32", max_doc_tokens=0)),
    "k128_site_rec": (128, {}, {}, {}, dict(site_rec=True, call_limit=(1 << 28) - 1, rows="quad16")),
    "k2048_dense": (2048, {}, {}, {}, dict(scratch=True, sparse=False)),
    "k2048_labels": (2048, dict(n_labels=7), {}, {}, dict(scratch=False, sparse=True, heavy_docs=0)),
    "k2048_heavy": (2048, dict(n_labels=7, wide_doc=600), {}, {}, dict(scratch=True, sparse=True, heavy_docs=1)),
    "k512_image8": (512, dict(n_labels=7), dict(image=8), {}, dict(image_bits=8)),
    "k512_image16": (512, dict(n_labels=7), dict(image=16), {}, dict(image_bits=16)),
    "k512_image_auto": (512, dict(n_labels=7), {}, {}, dict(image_bits=0, image_order=False)),
    "k512_order_on": (512, dict(n_labels=7), dict(image=8, image_order=True), {}, dict(image_bits=8, image_order=True)),
    "k512_order_off": (512, dict(n_labels=7), dict(image=8, image_order=False), {}, dict(image_bits=8, image_order=False)),
}


def build_shape(name):
    from lda_thesis_amd.sampler import GibbsSampler
    K, corpus, kw, _, _ = SHAPES[name]
    off, word, freq, z, labs = _corpus(K, **corpus)
    return GibbsSampler(off, word, freq, z, K, 300, 0.1, 0.01, labs=labs, seed=1, commit_log=True, **kw)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_sampler_builds_what_the_plan_says(name, monkeypatch):
    for var in ("LLDA_ROWS16", "LLDA_QUAD", "LLDA_IMAGE"):
        monkeypatch.delenv(var, raising=False)
    K, corpus, kw, env, want = SHAPES[name]
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    s = build_shape(name)
    plan = _check_against_plan(s, True, kw.get("rows16"), kw.get("quad"), kw.get("image"), kw.get("image_order"))
    assert {k: getattr(plan, k) for k in want} == want
    if name == "k512_quad":
        assert s.row16 is not None and s.site_row is None
    if name == "k512_long_rows16":
        assert plan.max_doc_tokens >= 65536
    if name == "k2048_heavy":
        assert s._heavy is not None and int(s._heavy.sum()) == 1 and bool(s._heavy[1])
    s.sweep()
    s.check_status()


def test_an_invalid_environment_value_is_refused(monkeypatch):
    monkeypatch.setenv("LLDA_IMAGE", "4")
    with pytest.raises(ValueError, match="LLDA_IMAGE='4': expected one of 0, 8, 16"):
        build_shape("k512_image_auto")
