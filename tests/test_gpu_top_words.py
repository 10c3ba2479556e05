"""``llda_top_words`` (include/llda_gibbs.h) bit for bit against its numpy restatement (tests/topicref.py: one lexsort per
topic): every layout, V below / at / above n and around the row-chunk seams, ties, extreme counts, poisoned padding, NULL
outputs, a non-default stream.  The output buffers carry guard words behind them and are pre-filled."""
import numpy as np
import pytest
import torch

import topicref

pytestmark = pytest.mark.gpu

GUARD = 8
FILL_IDX, FILL_CNT = -77, -99
I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31


def run(n_k_v, n, pad=0, want_idx=True, want_cnt=True, poison_scratch=True):
    """the entry point on the device image of a (K, V) matrix -> (top_idx, top_cnt) numpy (None where not asked for)"""
    from lda_thesis_amd import _native
    n_k_v = np.asarray(n_k_v)
    K, V = n_k_v.shape
    dev = torch.device("cuda:0")
    rows = torch.from_numpy(topicref.device_rows(n_k_v, pad)).to(dev)
    nbytes = _native.top_words_scratch_bytes(V, K, n)
    scratch = torch.full((nbytes + GUARD,), 0x5A if poison_scratch else 0, dtype=torch.uint8, device=dev)
    idx = torch.full((K * n + GUARD,), FILL_IDX, dtype=torch.int32, device=dev)
    cnt = torch.full((K * n + GUARD,), FILL_CNT, dtype=torch.int32, device=dev)
    _native.top_words(rows, V, K, n, idx if want_idx else None, cnt if want_cnt else None, scratch[:nbytes])
    torch.cuda.current_stream(dev).synchronize()
    idx_h, cnt_h = idx.cpu().numpy(), cnt.cpu().numpy()
    assert (scratch[nbytes:] == (0x5A if poison_scratch else 0)).all()
    assert (idx_h[K * n:] == FILL_IDX).all() and (cnt_h[K * n:] == FILL_CNT).all()
    if not want_idx:
        assert (idx_h == FILL_IDX).all()
    if not want_cnt:
        assert (cnt_h == FILL_CNT).all()
    return (idx_h[:K * n].reshape(K, n) if want_idx else None), (cnt_h[:K * n].reshape(K, n) if want_cnt else None)


def check(n_k_v, n, ref=None, **kw):
    """ref: a (top_idx, top_cnt) restatement for 16 words to take the first n of (the first n of the order are the order for n)"""
    idx, cnt = run(n_k_v, n, **kw)
    want_idx, want_cnt = topicref.top_words_ref(n_k_v, n) if ref is None else (ref[0][:, :n], ref[1][:, :n])
    if idx is not None:
        bad = np.flatnonzero((idx != want_idx).any(axis=1))
        assert bad.size == 0, "topics %s: got %s want %s" % (bad[:5], idx[bad[:1]], want_idx[bad[:1]])
    if cnt is not None:
        assert np.array_equal(cnt, want_cnt)


def skewed(rng, K, V):
    """counts as a trained n_k_v has them: mostly 0, a few large, many ties"""
    m = rng.integers(0, 40, size=(K, V))
    m[rng.random((K, V)) < 0.6] = 0
    heavy = rng.random((K, V)) < 0.02
    m[heavy] = rng.integers(40, 100000, size=int(heavy.sum()))
    return m


@pytest.mark.parametrize("K", [1, 5, 12, 100, 130, 392, 512, 1031, 7688])
def test_every_layout_and_vocabulary_size(K):
    rng = np.random.default_rng(K)
    for V in (1, 7, 16, 17, 300, 5000):
        if K == 7688 and V > 300:
            continue
        m = skewed(rng, K, V)
        ref = topicref.top_words_ref(m, 16)
        for n in (1, 10, 16):                        # V < n: padding; V == n at V = 16
            check(m, n, ref)


@pytest.mark.parametrize("K", [5, 130, 512, 1031])
def test_ties(K):
    rng = np.random.default_rng(100 + K)
    for V in (17, 300, 5000):
        for n in (1, 2, 4, 8, 10, 16):                                # every list size the kernels are built for, each filled
            check(rng.integers(0, 3, size=(K, V)), n)                 # {0, 1, 2}: ties in every list
    idx, cnt = run(np.zeros((K, 700), dtype=np.int64), 16)
    assert np.array_equal(idx, np.tile(np.arange(16, dtype=np.int32), (K, 1))) and (cnt == 0).all()


@pytest.mark.parametrize("K", [1, 12, 100, 512, 1031])
def test_position_of_the_maximum_and_the_row_chunk_seams(K):
    from lda_thesis_amd import _native
    C = _native.TOPW_CHUNK_ROWS
    V = 5000
    assert V > 4 * C
    rng = np.random.default_rng(200 + K)
    base = rng.integers(0, 50, size=(K, V))
    m = base.copy()
    m[:, 0] = 1000                                   # the maximum in row 0 ...
    check(m, 10)
    m = base.copy()
    m[:, V - 1] = 1000                               # ... in row V - 1
    check(m, 10)
    m = base.copy()
    for seam in range(C, V, C):                      # equal maxima on both sides of every seam: the lower id must win the tie
        m[:, seam - 1] = m[:, seam] = 1000
    for n in (1, 10, 16):
        check(m, n)
    m = base.copy()
    seams = np.arange(C, V, C)
    for k in range(K):
        s = seams[k % len(seams)]
        m[k, s - 4:s + 4] = 2000                     # eight equal maxima straddling one seam, across the row phases of a workgroup
    check(m, 10)
    check(m, 4)


@pytest.mark.parametrize("K", [5, 100, 512, 1031])
def test_extreme_values_and_poisoned_padding(K):
    rng = np.random.default_rng(300 + K)
    V = 600
    m = rng.integers(-5, 6, size=(K, V)).astype(np.int64)              # negative counts: compared as signed int32
    m[:, 17] = I32MAX
    m[::2, 400] = I32MAX
    m[:, 300] = I32MIN
    m[1::2, 5] = I32MAX - 1
    for n in (1, 10, 16):
        check(m, n, pad=I32MAX)                                        # the padding holds 0x7fffffff: never emitted
    check(np.full((K, 40), I32MIN, dtype=np.int64), 16, pad=I32MAX)    # every count the smallest there is
    check(np.full((K, 40), I32MAX, dtype=np.int64), 16, pad=I32MIN)
    check(rng.integers(I32MIN, I32MAX, size=(K, 300), endpoint=True), 10, pad=I32MAX)


@pytest.mark.parametrize("K", [12, 1031])
def test_null_outputs(K):
    m = skewed(np.random.default_rng(400 + K), K, 700)
    check(m, 10, want_cnt=False)
    check(m, 10, want_idx=False)
    run(m, 10, want_idx=False, want_cnt=False)


def test_non_default_stream_and_the_python_surface():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(500)
    K, V, n = 130, 3000, 10
    m = skewed(rng, K, V)
    dev = torch.device("cuda:0")
    rows = torch.from_numpy(topicref.device_rows(m)).to(dev)
    want = topicref.top_words_ref(m, n)
    side = torch.cuda.Stream(dev)
    idx, cnt = topics.top_words(rows, K, n, stream=side)
    side.synchronize()
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(cnt.cpu().numpy(), want[1])
    with torch.cuda.stream(side):
        idx, cnt = topics.top_words(rows, K, n)
        got = idx.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (K, n) and idx.device == rows.device
    for bad in (0, 17):
        with pytest.raises(ValueError):
            topics.top_words(rows, K, bad)
