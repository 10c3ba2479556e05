"""llda_attribute on the device: bit for bit against its CPU restatement (tests/attrref.py) around every seam of the geometry --
the lane groups of K <= 32, the register forms up to K = 1024, the LDS form beyond -- with guard words before and behind every
output."""
import numpy as np
import pytest

import attrref

pytestmark = pytest.mark.gpu

MAX_K = 7688
KS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 392, 512, 513, 1024, 1025, 1031, MAX_K)
GUARD = 8
MAX_F = 2 ** 23 - 1
PATTERN = {"float64": np.float64(-1234.5), "int64": np.int64(-0x123456789ABCDEF), "int32": np.int32(-0x1234567)}
OUTPUTS = (("theta_out", "float64"), ("credit", "float64"), ("site_idx", "int32"), ("site_val", "float64"), ("tok", "int64"),
           ("bad", "int64"))
V = 61
W_ZERO, W_NAN, W_INF, W_ABOVE, W_BELOW = 0, 1, 2, 3, 4                   # words with a planted row of phi_t
# per document count: (iters, alpha, top_m, freq mode, padded row strides)
SETTINGS = {1: (0, 0.0, 1, "mixed", True), 3: (1, 0.1, 4, "mixed", True), 4: (3, 0.0, 0, "ones", False), 5: (0, 0.1, 4, "ones", True),
            63: (3, 0.1, 4, "mixed", True), 64: (1, 0.0, 1, None, False), 65: (3, 0.1, 1, "mixed", True), 257: (1, 0.1, 4, "mixed", True)}
# the same values turned against the document counts: no per-site output with mixed frequencies, padded strides and iters = 0; no
# frequencies with every iters; top_m = 4 with equal strides
ROTATED = {1: (1, 0.1, 0, "mixed", True), 3: (0, 0.0, 0, None, True), 4: (0, 0.1, 4, "mixed", False), 5: (3, 0.0, 1, None, True),
           63: (0, 0.0, 0, "mixed", True), 64: (3, 0.1, 4, "mixed", False), 65: (1, 0.0, 0, None, True), 257: (3, 0.0, 1, "ones", True)}
TABLES = {"settings": SETTINGS, "rotated": ROTATED}
PLANTS = (W_ZERO, W_NAN, W_INF, W_ABOVE, W_BELOW, V, -1)                   # every planted word; V and -1 are outside the vocabulary


def tie_cols(K):
    return (0, K - 1) if K >= 2 else (0, 0)


def model(rng, K, D, pad_theta=3, pad_phi=5):
    """theta (D, K + pad_theta), phi_t (V, K + pad_phi): NaN in every column >= K.  A theta row has few loads: the columns 0 and K-1
    with one and the same load, the largest of the row (an exact tie; phi_t's columns 0 and K-1 are equal too), and up to K - 3
    others; every other column is an exact zero.  (K = 2: every second row has the column 0 alone; K = 1: the one load.)
    Planted rows of phi_t: all zero (p = 0), a NaN and an inf in a column that is read, and two whose p lands just above and just
    below 2^-960 whatever the row of theta."""
    a, b = tie_cols(K)
    t = np.zeros((D, K))
    for d in range(D):
        n_other = 0 if K < 4 else int(min(K - 3, rng.choice((1, 1, 3, 7, 40))))
        if n_other:
            t[d, 1 + rng.choice(K - 2, size=n_other, replace=False)] = rng.gamma(0.5, size=n_other) + 1e-3
        t[d, a] = t[d].max() + 0.25
        if K >= 3 or d % 2 == 0:
            t[d, b] = t[d, a]
    theta = np.full((D, K + pad_theta), np.nan)
    theta[:, :K] = t / t.sum(axis=1, keepdims=True)
    phi_t = np.full((V, K + pad_phi), np.nan)
    phi_t[:, :K] = rng.gamma(0.2, size=(V, K)) / V + 1e-9
    phi_t[:, b] = phi_t[:, a]
    phi_t[W_ZERO, :K] = 0.0
    phi_t[W_NAN, rng.integers(0, K)] = np.nan
    phi_t[W_INF, rng.integers(0, K)] = np.inf
    phi_t[W_ABOVE, :K] = 2.0 ** -960 * (1 + 2.0 ** -20)
    phi_t[W_BELOW, :K] = 2.0 ** -960 * (1 - 2.0 ** -20)
    return theta, phi_t


def corpus(rng, D, lens, freq_mode="mixed"):
    n = rng.choice(lens, size=D)
    doc_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(5, V, size=S).astype(np.int32)
    plant = rng.random(S)
    for w, lo in ((W_ZERO, 0.0), (W_NAN, 0.02), (W_INF, 0.04), (W_ABOVE, 0.06), (W_BELOW, 0.10), (V, 0.14), (-1, 0.16)):
        word[(plant >= lo) & (plant < lo + (0.04 if w in (W_ABOVE, W_BELOW) else 0.02))] = w      # V and -1: outside the vocabulary
    if freq_mode is None:
        return doc_off, word, None
    if freq_mode == "ones":
        freq = np.ones(S, dtype=np.int32)
    else:
        freq = rng.integers(0, 10, size=S).astype(np.int32)               # f = 0 included
        freq[rng.random(S) < 0.1] = MAX_F
        freq[rng.random(S) < 0.3] = 1
    return doc_off, word, freq


def run(theta, phi_t, doc_off, word, freq, K, iters=0, alpha=0.0, top_m=0, skip=(), n_vocab=V, pad_out=2):
    """one llda_attribute call with guard words before and behind every output (and, with pad_out, behind every output row) ->
    dict of whole buffers"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    D, S = len(doc_off) - 1, int(doc_off[-1])
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_theta, d_phi, d_off, d_word, d_freq = up(theta), up(phi_t), up(doc_off), up(word), up(freq)
    if d_word.numel() == 0:
        d_word = torch.zeros((1,), dtype=torch.int32, device=dev)
    ld = K + pad_out
    sizes = dict(theta_out=D * ld, credit=D * ld, site_idx=S * top_m, site_val=S * top_m, tok=D, bad=D)
    bufs = {n: torch.full((sizes[n] + 2 * GUARD,), PATTERN[dt].item(), dtype=getattr(torch, dt), device=dev) for n, dt in OUTPUTS}
    _native.attribute(d_off, d_word, d_freq, d_theta, d_phi, D, n_vocab, K, iters=iters, alpha=alpha, top_m=top_m,
                      ld_theta=theta.shape[1], ld_phi=phi_t.shape[1], ld_out=ld, ld_credit=ld,
                      **{n: b[GUARD:GUARD + sizes[n]] for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def check(got, want, D, K, top_m, skip=(), what="", pad_out=2):
    ld = K + pad_out
    for name, dt in OUTPUTS:
        g, pat = got[name], PATTERN[dt]
        n = g.shape[0] - 2 * GUARD
        assert (g[:GUARD] == pat).all() and (g[GUARD + n:] == pat).all(), "%s: guard words around %s overwritten" % (what, name)
        body = g[GUARD:GUARD + n]
        if name in skip or (name.startswith("site_") and top_m == 0):
            assert (body == pat).all(), "%s: %s was written" % (what, name)
            continue
        w = want[name]
        if name in ("theta_out", "credit"):
            body = body.reshape(D, ld)
            assert (body[:, K:] == pat).all(), "%s: %s written behind column K" % (what, name)
            body = body[:, :K]
        else:
            body = body.reshape(w.shape)
        diff = np.argwhere(bits(body) != bits(w))
        assert diff.shape[0] == 0, "%s: %s differs at %s: got %s want %s" % (what, name, diff[:5].tolist(), body[tuple(diff[0])], w[tuple(diff[0])])


def lens_for(K):
    """site counts: none, one, the seams of the 64-site chunks; 65 at most where a row is long"""
    return (0, 1, 2, 3, 5, 63, 64, 65, 130) if K <= 513 else (0, 1, 2, 3, 5, 63, 64, 65)


def met(want, theta, word, K, top_m):
    """[good sites, bad sites, a good site with a padded site_idx, a tie ordered by topic id, a label that stayed 0] seen in want"""
    idx, val = want["site_idx"], want["site_val"]
    a, b = tie_cols(K)
    stayed = (theta[:, :K] == 0.0)
    assert (want["theta_out"][stayed] == 0.0).all() and (want["credit"][stayed] == 0.0).all()
    padded = tie = False
    if top_m > 1:
        good = idx[:, 0] >= 0
        padded = bool((good & (idx[:, -1] < 0)).any())
        tie = bool(((idx[:, 0] == a) & (idx[:, 1] == b) & (val[:, 0] == val[:, 1]) & (val[:, 0] > 0.0)).any()) and a != b
    return [int(want["tok"].sum() > 0), int(want["bad"].sum() > 0), int(padded), int(tie), int(stayed.any())]


@pytest.mark.parametrize("table", sorted(TABLES))
@pytest.mark.parametrize("K", KS)
def test_bit_for_bit_against_attrref(K, table):
    rng = np.random.default_rng((9000 if table == "settings" else 19000) + K)
    seen = np.zeros(5, dtype=np.int64)
    drawn = np.zeros(len(PLANTS), dtype=np.int64)
    for D, (iters, alpha, top_m, freq_mode, padded) in TABLES[table].items():
        theta, phi_t = model(rng, K, D, *((3, 5) if padded else (0, 0)))
        doc_off, word, freq = corpus(rng, D, lens_for(K)[:6] if D == 257 else lens_for(K), freq_mode)
        want = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, K=K, V=V, iters=iters, alpha=alpha, top_m=top_m)
        # the two planted words fall on both sides of the bound, against the start loads and against the final ones
        for th in (theta[:, :K], want["theta_out"]):
            assert (attrref.sum64(th * phi_t[W_ABOVE, :K]) >= attrref.MIN_P).all()
            assert (attrref.sum64(th * phi_t[W_BELOW, :K]) < attrref.MIN_P).all()
        drawn += [int((word == w).sum()) for w in PLANTS]
        got = run(theta, phi_t, doc_off, word, freq, K, iters, alpha, top_m, pad_out=2 if padded else 0)
        check(got, want, D, K, top_m, what="K %d D %d" % (K, D), pad_out=2 if padded else 0)
        if iters == 0:
            assert np.array_equal(bits(want["theta_out"]), bits(theta[:, :K]))
        seen += met(want, theta, word, K, top_m)
    assert (drawn > 0).all(), drawn                      # every planted row and both words outside the vocabulary were met
    need = [True, True, True, K >= 2, K >= 2]            # (K = 1: one label, so no tie and no label at 0)
    assert all(s > 0 for s, n in zip(seen, need) if n), seen


def test_long_document_and_empty_ones():
    """K = 64: no site, one site, 3 000 sites (47 chunks of 64, the last one short), then no site again"""
    rng = np.random.default_rng(64)
    K, D = 64, 4
    theta, phi_t = model(rng, K, D)
    doc_off = np.array([0, 0, 1, 3001, 3001], dtype=np.int64)
    word = rng.integers(5, V, size=3001).astype(np.int32)
    freq = rng.integers(1, 4, size=3001).astype(np.int32)
    want = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, K=K, iters=1, alpha=0.1, top_m=1)
    for d in (0, 3):                                                     # an empty document: its loads, no credit
        assert np.array_equal(bits(want["theta_out"][d]), bits(theta[d, :K])) and not want["credit"][d].any()
        assert want["tok"][d] == 0 and want["bad"][d] == 0
    assert want["tok"][2] >= 3000
    check(run(theta, phi_t, doc_off, word, freq, K, 1, 0.1, 1), want, D, K, 1, what="long")


@pytest.mark.parametrize("K", (7, 32, 65, 512, 1031))
def test_batch_independence(K):
    """the same documents alone, reversed, and inside a larger batch: identical bits per document"""
    rng = np.random.default_rng(7000 + K)
    D, iters, alpha, top_m = 11, 2, 0.1, 4
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 4, 9, 66))
    want = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, K=K, V=V, iters=iters, alpha=alpha, top_m=top_m)
    extra_theta, _ = model(rng, K, 6)
    extra_off, extra_word, extra_freq = corpus(rng, 6, (0, 3, 70))

    def gather(ids, theta_all, off_all, word_all, freq_all):
        n = np.diff(off_all)[ids]
        sites = np.concatenate([np.arange(off_all[d], off_all[d + 1]) for d in ids] + [np.zeros(0)]).astype(np.int64)
        return theta_all[ids], np.concatenate([[0], np.cumsum(n)]).astype(np.int64), word_all[sites], freq_all[sites], sites

    all_theta = np.concatenate([extra_theta[:3], theta, extra_theta[3:]])
    all_off = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(extra_off)[:3], np.diff(doc_off), np.diff(extra_off)[3:]]))]).astype(np.int64)
    cut = int(extra_off[3])
    all_word = np.concatenate([extra_word[:cut], word, extra_word[cut:]])
    all_freq = np.concatenate([extra_freq[:cut], freq, extra_freq[cut:]])
    plans = [("alone", [[d] for d in range(D)], theta, doc_off, word, freq, 0),
             ("reversed", [list(range(D))[::-1]], theta, doc_off, word, freq, 0),
             ("inside", [list(range(D + 6))], all_theta, all_off, all_word, all_freq, 3)]
    for what, batches, th_all, off_all, word_all, freq_all, shift in plans:
        got = {n: np.empty_like(want[n]) for n, _ in OUTPUTS}
        for ids in batches:
            th, off, w, f, sites = gather(np.asarray(ids), th_all, off_all, word_all, freq_all)
            r = run(th, phi_t, off, w, f, K, iters, alpha, top_m, pad_out=0)
            n_sites = int(off[-1])
            for i, d in enumerate(ids):
                if not shift <= d < shift + D:
                    continue
                for n in ("theta_out", "credit"):
                    got[n][d - shift] = r[n][GUARD:GUARD + len(ids) * K].reshape(len(ids), K)[i]
                for n in ("tok", "bad"):
                    got[n][d - shift] = r[n][GUARD + i]
                for n in ("site_idx", "site_val"):
                    rows = r[n][GUARD:GUARD + n_sites * top_m].reshape(n_sites, top_m)[off[i]:off[i + 1]]
                    got[n][doc_off[d - shift]:doc_off[d - shift + 1]] = rows
        for n, _ in OUTPUTS:
            assert np.array_equal(bits(got[n]), bits(want[n])), (K, what, n)


@pytest.mark.parametrize("K", (8, 129, 2000))
def test_every_output_may_be_null(K):
    rng = np.random.default_rng(8000 + K)
    D = 9
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 5, 20))
    want = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, K=K, V=V, iters=2, alpha=0.1, top_m=2)
    for skip in (("theta_out",), ("credit",), ("site_idx", "site_val"), ("tok",), ("bad",), tuple(n for n, _ in OUTPUTS)):
        check(run(theta, phi_t, doc_off, word, freq, K, 2, 0.1, 2, skip=skip), want, D, K, 2, skip=skip, what="K %d without %s" % (K, skip))
    import torch
    from lda_thesis_amd import _native
    t = torch.zeros((1, K), dtype=torch.float64, device="cuda:0")
    _native.attribute(None, None, None, t, t, 0, 1, K)                   # D = 0: a no-op, nothing is dereferenced
    with pytest.raises(_native.NativeError):                             # one of the pair alone: refused
        _native.attribute(t, t, None, t, t, 1, 1, K, top_m=1, site_val=t)


def test_python_surface():
    """attribution.attribute: numpy CSR, strided device tensors, the outputs ``want`` names, and its refusals"""
    import torch
    from lda_thesis_amd import attribution
    rng = np.random.default_rng(11)
    K, D = 40, 6
    theta, phi_t = model(rng, K, D)
    doc_off, word, freq = corpus(rng, D, (0, 1, 5, 20), "ones")
    freq = rng.integers(1, 6, size=freq.shape[0]).astype(np.int32)
    word[(word < 5) | (word >= V)] = 9
    dev = torch.device("cuda", 0)
    d_theta, d_phi = torch.from_numpy(theta).to(dev)[:, :K], torch.from_numpy(phi_t).to(dev)[:, :K]      # row strides K + 3, K + 5
    want = attrref.attribute_ref(theta, phi_t, doc_off, word, freq, K=K, iters=4, alpha=0.05, top_m=3)
    got = attribution.attribute(d_theta, d_phi, doc_off, word, freq, iters=4, alpha=0.05, top_m=3)
    assert sorted(got) == ["bad", "credit", "site_idx", "site_val", "theta", "tok"]
    for name, ref in (("theta", "theta_out"), ("credit", "credit"), ("site_idx", "site_idx"), ("site_val", "site_val"), ("tok", "tok"),
                      ("bad", "bad")):
        g = got[name].cpu().numpy()
        assert g.dtype == want[ref].dtype and np.array_equal(bits(g), bits(want[ref])), name
    only = attribution.attribute(d_theta, d_phi, doc_off, word, None, top_m=0, want=("credit", "sites"))
    assert sorted(only) == ["credit"]
    ones = attrref.attribute_ref(theta, phi_t, doc_off, word, None, K=K)
    assert np.array_equal(bits(only["credit"].cpu().numpy()), bits(ones["credit"]))
    lists = attribution.spans(doc_off, got["site_idx"].cpu().numpy(), got["site_val"].cpu().numpy())
    assert [x.shape for x in lists[0]] == [(int(n), 3) for n in np.diff(doc_off)]
    for bad in (dict(word=np.where(word == 9, V, word)), dict(freq=np.full_like(freq, 2 ** 23)), dict(doc_off=doc_off[:-1]),
                dict(phi=d_phi[:, :K - 1]), dict(theta=theta), dict(iters=-1), dict(alpha=-0.5), dict(alpha=float("nan")),
                dict(top_m=5), dict(want=("theta", "everything"))):
        args = dict(theta=d_theta, phi=d_phi, doc_off=doc_off, word=word, freq=freq, iters=1, alpha=0.1, top_m=1, want=("theta",))
        args.update(bad)
        with pytest.raises(ValueError):
            attribution.attribute(args["theta"], args["phi"], args["doc_off"], args["word"], args["freq"], iters=args["iters"],
                                  alpha=args["alpha"], top_m=args["top_m"], want=args["want"])
