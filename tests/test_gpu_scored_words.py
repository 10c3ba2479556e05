"""``llda_scored_words`` (include/llda_gibbs.h) bit for bit against its numpy restatement (tests/scoredref.py): both sources, every
layout, V below / at / above n and around the row-chunk seams, every power pair of the relevance family, ties, skipped words, NaN,
infinities and signed zeros, extreme counts and underflowing powers, poisoned padding, NULL outputs, a non-default stream.  Scores
are compared as uint64.  The output buffers carry guard words behind them and are pre-filled; the scratch is poisoned."""
import numpy as np
import pytest
import torch

import scoredref

pytestmark = pytest.mark.gpu

GUARD = 8
FILL_IDX, FILL_SCORE, FILL_NAN = -77, -123.25, -55
I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31
POWERS = ((1, 0), (1, 1), (2, 1), (5, 2), (8, 7))
DEV = "cuda:0"


def up(arr):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def run(V, K, n, a, *, n_kw=None, n_k=None, den=None, beta=0.0, mat=None, ld=None, wdiv=None, want=(True, True, True)):
    """the entry point on device tensors -> (top_idx, top_score as uint64, n_nan) numpy (None where not asked for)"""
    from lda_thesis_amd import _native
    nbytes = _native.scored_words_scratch_bytes(V, K, n)
    scratch = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    idx = torch.full((K * n + GUARD,), FILL_IDX, dtype=torch.int32, device=DEV)
    sc = torch.full((K * n + GUARD,), FILL_SCORE, dtype=torch.float64, device=DEV)
    nn = torch.full((K + GUARD,), FILL_NAN, dtype=torch.int32, device=DEV)
    _native.scored_words(V, K, n, a, scratch[:nbytes], n_kw=n_kw, n_k=n_k, den=den, beta=beta, mat=mat, ld=ld, wdiv=wdiv,
                         top_idx=idx if want[0] else None, top_score=sc if want[1] else None, n_nan=nn if want[2] else None)
    torch.cuda.current_stream(torch.device(DEV)).synchronize()
    idx_h, sc_h, nn_h = idx.cpu().numpy(), sc.cpu().numpy(), nn.cpu().numpy()
    assert (scratch[nbytes:] == 0x5A).all()
    assert (idx_h[K * n:] == FILL_IDX).all() and (sc_h[K * n:] == FILL_SCORE).all() and (nn_h[K:] == FILL_NAN).all()
    if not want[0]:
        assert (idx_h == FILL_IDX).all()
    if not want[1]:
        assert (sc_h == FILL_SCORE).all()
    if not want[2]:
        assert (nn_h == FILL_NAN).all()
    return (idx_h[:K * n].reshape(K, n) if want[0] else None, sc_h[:K * n].reshape(K, n).view(np.uint64) if want[1] else None,
            nn_h[:K] if want[2] else None)


def same(got, ref, n, what=""):
    """ref: a restatement for >= n words to take the first n of (the first n of the order are the order for n)"""
    idx, sc, nn = got
    if idx is not None:
        bad = np.flatnonzero((idx != ref[0][:, :n]).any(axis=1))
        assert bad.size == 0, "%s topics %s: got %s want %s" % (what, bad[:5], idx[bad[:1]], ref[0][bad[:1], :n])
    if sc is not None:
        assert np.array_equal(sc, np.ascontiguousarray(ref[1][:, :n]).view(np.uint64)), what
    if nn is not None:
        assert np.array_equal(nn, ref[2]), what


class Counts:
    """the device image of a (K, V) count matrix with its denominators"""

    def __init__(self, m, beta, pad=0, n_k=None, den=None, pad_den=np.nan):
        self.m = np.asarray(m)
        self.K, self.V = self.m.shape
        self.beta = float(beta)
        self.x = scoredref.x_of_counts(self.m, beta, den=den, n_k=n_k)
        self.n_kw = up(scoredref.device_rows(self.m, pad))
        if den is None:
            n_k = self.m.astype(np.int64).sum(axis=1) if n_k is None else np.asarray(n_k)
            self.n_k, self.den = up(scoredref.device_vector(n_k.astype(np.int32), self.K, pad)), None
        else:
            self.n_k, self.den = None, up(scoredref.device_vector(np.asarray(den, dtype=np.float64), self.K, pad_den))

    def run(self, n, a, wdiv=None, **kw):
        return run(self.V, self.K, n, a, n_kw=self.n_kw, n_k=self.n_k, den=self.den, beta=self.beta, wdiv=wdiv, **kw)


class Matrix:
    """the device image of a (V, K) float64 matrix with the leading dimension ld (the columns K .. ld-1 hold NaN)"""

    def __init__(self, x, ld=None):
        self.x = np.asarray(x, dtype=np.float64)
        self.V, self.K = self.x.shape
        self.ld = self.K if ld is None else ld
        self.mat = up(scoredref.matrix_rows(self.x, self.ld))

    def run(self, n, a, wdiv=None, **kw):
        return run(self.V, self.K, n, a, mat=self.mat, ld=self.ld, wdiv=wdiv, **kw)


@pytest.mark.parametrize("K", [1, 5, 12, 100, 130, 392, 512, 1031, 7688])
def test_every_layout_vocabulary_size_and_power(K):
    """both sources over every V and power pair; matrix mode with ld = K and ld = K + 3 (one of them even: 16-byte loads, the other
    odd: 8-byte loads)"""
    rng = np.random.default_rng(K)
    for V in (1, 7, 16, 17, 255, 256, 257, 300, 5000):
        if K == 7688 and V > 300:
            continue
        m = scoredref.skewed(rng, K, V)
        n_w = m.sum(axis=0)                          # (words nobody holds are not ranked: wdiv = 0)
        src = Counts(m, 0.01)
        mats = (Matrix(src.x), Matrix(src.x, K + 3))
        for a, b in POWERS:
            wdiv = None if b == 0 else scoredref.word_divisor_ref(n_w, b)
            ref = scoredref.scored_words_ref(src.x, 16, a, wdiv)
            wd = up(wdiv)
            for i, n in enumerate((1, 10, 16)):      # V < n: padding; V == n at V = 16
                same(src.run(n, a, wd), ref, n, "counts V=%d n=%d a=%d b=%d" % (V, n, a, b))
                same(mats[i % 2].run(n, a, wd), ref, n, "matrix V=%d n=%d a=%d b=%d" % (V, n, a, b))
            same(mats[0].run(10, a, wd), ref, 10, "matrix ld=K V=%d a=%d b=%d" % (V, a, b))


@pytest.mark.parametrize("K", [5, 130, 512, 1031])
def test_ties(K):
    """counts in {0, 1, 2} and n_w drawn from three values: the lists are decided by the word id"""
    rng = np.random.default_rng(100 + K)
    for V in (17, 300, 5000):
        m = rng.integers(0, 3, size=(K, V))
        n_w = rng.choice([3, 5, 40], size=V)
        src = Counts(m, 0.5)
        mat = Matrix(src.x)
        for a, b in POWERS:
            wdiv = None if b == 0 else scoredref.word_divisor_ref(n_w, b)
            ref = scoredref.scored_words_ref(src.x, 16, a, wdiv)
            for n in (1, 10, 16):
                same(src.run(n, a, up(wdiv)), ref, n)
                same(mat.run(n, a, up(wdiv)), ref, n)
    ids = np.tile(np.arange(16, dtype=np.int32), (K, 1))
    idx, sc, nn = Matrix(np.zeros((700, K))).run(16, 2)
    assert np.array_equal(idx, ids) and (sc == 0).all() and (nn == 0).all()          # an all-zero matrix: ids 0 .. n-1, scores +0.0
    zero = Counts(np.zeros((K, 700), dtype=np.int64), 0.01)
    idx, sc, nn = zero.run(16, 1)
    assert np.array_equal(idx, ids)
    same((idx, sc, nn), scoredref.scored_words_ref(zero.x, 16, 1, None), 16)


@pytest.mark.parametrize("K", [1, 12, 100, 512, 1031])
def test_position_of_the_maximum_and_the_row_chunk_seams(K):
    """the best word at the first and the last row of a row chunk, at V - 1, in every column (so also the last of a lane's pair), and
    equal maxima on both sides of the seams: the lower id wins"""
    from lda_thesis_amd import _native
    C = _native.TOPW_CHUNK_ROWS
    V = 5 * C + 20                                   # five whole row chunks and a short one
    rng = np.random.default_rng(200 + K)
    base_x = rng.random((V, K))
    base_m = rng.integers(0, 50, size=(K, V))
    wdiv = up(scoredref.word_divisor_ref(rng.integers(1, 9, size=V), 1))
    wd_h = wdiv.cpu().numpy()

    def both(x, m, ns):
        src, mat = Counts(m, 0.01), Matrix(x, K + (K & 1))
        for a, w, w_h in ((1, None, None), (2, wdiv, wd_h)):
            rc, rm = scoredref.scored_words_ref(src.x, 16, a, w_h), scoredref.scored_words_ref(x, 16, a, w_h)
            for n in ns:
                same(src.run(n, a, w), rc, n)
                same(mat.run(n, a, w), rm, n)

    rows = (0, C - 1, C, 2 * C - 1, V - 1)
    for start in range(len(rows) if K < len(rows) else 1):           # topic k has its best word at rows[(k + start) % 5]
        x, m = base_x.copy(), base_m.copy()
        for k in range(K):
            x[rows[(k + start) % len(rows)], k] = 1e6
            m[k, rows[(k + start) % len(rows)]] = 10 ** 6
        both(x, m, (10,))
    x, m = base_x.copy(), base_m.copy()
    for seam in range(C, V, C):
        x[seam - 1, :] = x[seam, :] = 64.0
        m[:, seam - 1] = m[:, seam] = 4096
    both(x, m, (1, 10, 16))
    x, m = base_x.copy(), base_m.copy()
    seams = np.arange(C, V, C)
    for k in range(K):
        s = seams[k % len(seams)]
        x[s - 4:s + 4, k] = 128.0                   # eight equal maxima straddling one seam, across the row phases of a workgroup
        m[k, s - 4:s + 4] = 8192
    both(x, m, (4, 10))


@pytest.mark.parametrize("K", [5, 130, 1031])
def test_skipped_words(K):
    rng = np.random.default_rng(300 + K)
    V = 700
    m = scoredref.skewed(rng, K, V)
    src = Counts(m, 0.01)
    mat = Matrix(src.x)
    wdiv = scoredref.word_divisor_ref(m.sum(axis=0) + 1, 2)
    off = rng.random(V) < 1 / 3                      # a random third of the words, either sign of zero
    wdiv[off] = np.where(rng.random(int(off.sum())) < 0.5, 0.0, -0.0)
    few = np.zeros(V)
    few[[3, 400, 699]] = 0.25                        # fewer than n words remain: padding
    for w in (wdiv, few, np.zeros(V), -np.zeros(V)):
        ref = scoredref.scored_words_ref(src.x, 16, 5, w)
        for n in (1, 10, 16):
            same(src.run(n, 5, up(w)), ref, n)
            same(mat.run(n, 5, up(w)), ref, n)
    idx, sc, nn = src.run(10, 5, up(few))
    assert (idx[:, 3:] == -1).all() and (sc[:, 3:] == 0x7FF8000000000000).all() and (idx[:, :3] >= 0).all()
    idx, sc, nn = mat.run(10, 5, up(np.zeros(V)))
    assert (idx == -1).all() and (sc == 0x7FF8000000000000).all() and (nn == 0).all()


@pytest.mark.parametrize("K", [5, 130, 1031])
def test_special_values_in_matrix_mode(K):
    rng = np.random.default_rng(400 + K)
    V = 700
    x = rng.standard_normal((V, K))                  # negative entries
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0])
    hit = rng.random((V, K)) < 0.05
    x[hit] = rng.choice(special, size=int(hit.sum()))
    x[10, :] = 0.0                                   # a +0.0 / -0.0 pair: ranks by id
    x[11, :] = -0.0
    x[12, ::2] = np.nan
    wdiv = rng.choice([1.0, -1.0, 0.5, 0.0, np.inf], size=V)      # (inf / inf and 0 * inf: more NaN)
    for ld in (K, K + 1):
        mat = Matrix(x, ld)
        for a in (1, 2, 5):
            for w in (None, wdiv):
                ref = scoredref.scored_words_ref(x, 16, a, w)
                assert ref[2].sum() > 0
                for n in (1, 10, 16):
                    same(mat.run(n, a, up(w)), ref, n, "ld=%d a=%d n=%d" % (ld, a, n))
    z = np.full((V, K), -5.0)
    z[20, :], z[21, :] = -0.0, 0.0
    idx, sc, _ = Matrix(z).run(2, 1)
    assert (idx == [20, 21]).all() and (sc[:, 0] == 0x8000000000000000).all() and (sc[:, 1] == 0).all()
    z[:, :] = -np.inf                                # real -inf entries beat the padding
    idx, sc, _ = Matrix(z).run(16, 1)
    assert np.array_equal(idx, np.tile(np.arange(16, dtype=np.int32), (K, 1))) and (sc == 0xFFF0000000000000).all()
    z[:, :] = np.nan                                 # every score a NaN
    idx, sc, nn = Matrix(z).run(10, 3)
    assert (idx == -1).all() and (sc == 0x7FF8000000000000).all() and (nn == V).all()


def test_a_matrix_that_is_only_8_byte_aligned():
    rng = np.random.default_rng(450)
    V, K = 300, 130
    x = rng.random((V, K))
    buf = torch.zeros((V * K + 1,), dtype=torch.float64, device=DEV)
    view = buf[1:]
    view.copy_(up(x).reshape(-1))
    assert view.data_ptr() % 16 == 8
    ref = scoredref.scored_words_ref(x, 10, 2, None)
    same(run(V, K, 10, 2, mat=view, ld=K), ref, 10)


@pytest.mark.parametrize("K", [5, 100, 512, 1031])
def test_extreme_counts_poisoned_padding_and_explicit_den(K):
    rng = np.random.default_rng(500 + K)
    V = 600
    m = rng.integers(-5, 6, size=(K, V)).astype(np.int64)              # negative counts: converted as signed int32
    m[:, 17] = I32MAX
    m[::2, 400] = I32MAX
    m[:, 300] = I32MIN
    m[1::2, 5] = I32MAX - 1
    n_k = rng.integers(1, I32MAX, size=K)
    wdiv = scoredref.word_divisor_ref(rng.integers(0, 4, size=V), 2)
    for beta in (1e-6, 2.0 ** 20):
        src = Counts(m, beta, pad=I32MAX, n_k=n_k)                      # the padding of n_kw and n_k holds 0x7fffffff
        for a, w in ((1, None), (5, wdiv), (8, wdiv)):
            ref = scoredref.scored_words_ref(src.x, 16, a, w)
            for n in (1, 10, 16):
                same(src.run(n, a, up(w)), ref, n, "beta=%g a=%d n=%d" % (beta, a, n))
    den = rng.random(K) * 1e6 + 1.0                                     # an explicit den; its padding holds NaN
    den[0] = 0.0                                                        # (0 + 0) / 0 where the count is 0 and beta = 0: counted as NaN
    src = Counts(rng.integers(0, 3, size=(K, V)), 0.0, pad=I32MIN, den=den)
    ref = scoredref.scored_words_ref(src.x, 16, 2, wdiv)
    assert ref[2][0] > 0
    for n in (1, 10, 16):
        same(src.run(n, 2, up(wdiv)), ref, n)


@pytest.mark.parametrize("K", [12, 512])
def test_powers_that_underflow(K):
    """a = 8 on entries near 1e-40: the powers are denormals or zero, the resulting ties rank by id, the bits still match"""
    rng = np.random.default_rng(600 + K)
    V = 600
    x = 10.0 ** rng.uniform(-41.5, -39.5, size=(V, K))
    x[rng.random((V, K)) < 0.1] = 1e-39
    wdiv = rng.choice([1.0, 0.25, 3.0, 1e-3], size=V)
    mat = Matrix(x)
    for w in (None, wdiv):
        ref = scoredref.scored_words_ref(x, 16, 8, w)
        s = scoredref.scores_of(x, 8, w)
        assert (s == 0).any() and ((s > 0) & (s < 2.0 ** -1022)).any()
        for n in (1, 10, 16):
            same(mat.run(n, 8, up(w)), ref, n)
    ref = scoredref.scored_words_ref(x[:, :1] * 1e-3, 16, 8, None)       # every power underflows to zero: ids 0 .. 15
    assert np.array_equal(ref[0][0], np.arange(16))
    same(Matrix(x[:, :1] * 1e-3).run(16, 8), ref, 16)


@pytest.mark.parametrize("K", [12, 1031])
def test_null_outputs(K):
    rng = np.random.default_rng(700 + K)
    m = scoredref.skewed(rng, K, 700)
    src = Counts(m, 0.01)
    mat = Matrix(src.x)
    wdiv = scoredref.word_divisor_ref(m.sum(axis=0), 2)
    ref = scoredref.scored_words_ref(src.x, 10, 5, wdiv)
    for want in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        same(src.run(10, 5, up(wdiv), want=want), ref, 10)
        same(mat.run(10, 5, up(wdiv), want=want), ref, 10)


def test_non_default_stream_and_the_python_surface():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(800)
    K, V, n = 130, 3000, 10
    m = scoredref.skewed(rng, K, V)
    src = Counts(m, 0.01)
    n_w = m.sum(axis=0)
    a, b = topics.relevance_powers(0.6)
    wdiv = topics.word_divisor(n_w, b)
    ref = scoredref.scored_words_ref(src.x, n, a, scoredref.word_divisor_ref(n_w, b))
    side = torch.cuda.Stream(torch.device(DEV))
    got = topics.scored_words(src.n_kw, K, n, a, wdiv, n_k=src.n_k, beta=0.01, stream=side)
    side.synchronize()
    same((got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint64), got[2].cpu().numpy()), ref, n)
    with torch.cuda.stream(side):
        got = topics.scored_words(up(src.x), K, n, a, up(wdiv))
        got = got[0].cpu().numpy(), got[1].cpu().numpy().view(np.uint64), got[2].cpu().numpy()
    same(got, ref, n)
    idx, sc, nn = topics.scored_words(up(src.x), K, n)
    assert idx.dtype == torch.int32 and sc.dtype == torch.float64 and nn.dtype == torch.int32
    assert tuple(idx.shape) == (K, n) == tuple(sc.shape) and tuple(nn.shape) == (K,) and idx.device == src.n_kw.device
    for kw in (dict(n=0), dict(n=17), dict(a=0), dict(a=9)):
        args = dict(n=n, a=1)
        args.update(kw)
        with pytest.raises(ValueError):
            topics.scored_words(up(src.x), K, args["n"], args["a"])
    with pytest.raises(ValueError):
        topics.scored_words(src.n_kw, K, n)                             # counts without beta and a denominator
    with pytest.raises(ValueError):
        topics.scored_words(up(src.x), K, n, beta=0.01)
    with pytest.raises(ValueError):
        topics.scored_words(up(src.x), K + 1, n)
    with pytest.raises(ValueError):
        topics.scored_words(up(src.x), K, n, 1, np.ones(V + 1))
