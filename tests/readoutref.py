"""numpy float64 restatement of the read-out entry points ``llda_readout_theta`` and ``llda_readout_phi`` (include/llda_gibbs.h),
written from the header and the reference's own expressions (LabeledLDA.py:231-239, 144-153; CascadeLDA.py:394-395), and the
inputs the read-out tests share (tests/test_readout_host.py, tests/test_gpu_readout_direct.py, the llda_loglik tests of
tests/test_gpu_count_kernels.py).

Pure numpy: nothing here needs a GPU; only the layout of K is asked of lda_thesis_amd.layout.group_layout.  Every matrix is in the
REFERENCE's order ((D, K), (K, V), topic k in column / row k) unless a name says ``device``.
"""
from fractions import Fraction

import numpy as np

NEGATIVE, NAN, NO_LOAD = 1, 2, 4                 # LLDA_READOUT_NEGATIVE / _NAN / _NO_LOAD
INT32_MAX = 2 ** 31 - 1
WIDE_GRID = 4096                                 # workgroups of a wide read-out at most (csrc/sweep_plan.hpp wide_blocks)

# keep * old + (share * cur) where a fused multiply-add gives another last bit, whichever of the two products it swallows:
# (keep, old, share, cur); cur = RN(1 / 3) is theta of a count of 1 beside a count of 2 (no label, so alpha does not enter) and phi
# of a count of 1 over a denominator of 3.  tests/test_readout_host.py proves the difference.
FMA_TRIPLE = (6.0 / 7.0, float.fromhex("0x1.273d27b04760cp-3"), 1.0 / 7.0, 1.0 / 3.0)
COEFFS = [(0.5, 0.5), (6.0 / 7.0, 1.0 / 7.0), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0)]          # (keep, share) of the running means
POISONS = [float("nan"), float("inf"), float("-inf"), -0.0, 5e-324]                      # values of ``old`` beside random doubles


def layout(K):
    from lda_thesis_amd.layout import group_layout
    return group_layout(K)


# ------------------------------------------------------------------------------------------------
# the operations
# ------------------------------------------------------------------------------------------------
def theta_ref(n_d_k, labs, alpha, with_sums=False):
    """get_theta (LabeledLDA.py:236-239): num = n_d_k + labs*alpha, num / np.sum(num) row by row.  The row sum is np.sum of each
    contiguous 1-D row: numpy's pairwise order with no doubt about the axis it iterates.  0/0 gives NaN as numpy gives."""
    num = np.ascontiguousarray(np.asarray(n_d_k).astype(np.int64) + np.asarray(labs).astype(np.float64) * float(alpha))
    rs = np.array([np.sum(np.ascontiguousarray(num[d])) for d in range(num.shape[0])], dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = num / rs[:, np.newaxis]
    return (out, num, rs) if with_sums else out


def phi_ref(n_k_v, n_zk, V, beta):
    """get_phi (LabeledLDA.py:231-234), the header's den == NULL case: (n_k_v + beta) / (n_zk[:, None] + V*beta)"""
    num = np.asarray(n_k_v).astype(np.int64) + float(beta)
    den = np.asarray(n_zk).astype(np.int64)[:, np.newaxis] + int(V) * float(beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den


def ph_rows_ref(n_k_v, den):
    """SubLDA.get_ph (CascadeLDA.py:394-395), the header's den != NULL case with beta = 0: n_k_v / den[:, None] with numpy's
    0/0 = NaN and x/0 = inf"""
    num = np.asarray(n_k_v).astype(np.int64) + 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / np.asarray(den, dtype=np.float64)[:, np.newaxis]


def running_mean_ref(old, cur, keep, share):
    """keep*old + (share*cur): three numpy operations, each rounded on its own (LabeledLDA.py:144-145, CascadeLDA.py:432)"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        a = np.multiply(np.float64(keep), np.asarray(old, dtype=np.float64))
        b = np.multiply(np.float64(share), np.asarray(cur, dtype=np.float64))
        return np.add(a, b)


def flags_ref(out):
    """the guards of LabeledLDA.py:146-153 on a finished (K, V) ``out``: bit 0 an entry < 0, bit 1 a NaN, bit 2 a column whose
    entries all compare equal to 0 (so -0.0 counts as zero and a NaN does not)"""
    out = np.asarray(out, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((NEGATIVE if (out < 0).any() else 0) | (NAN if np.isnan(out).any() else 0)
                | (NO_LOAD if (out == 0).all(axis=0).any() else 0))


def fma_exact(a, b, c):
    """RN(a*b + c) with one rounding (math.fma where the interpreter has it, else exact rationals)"""
    import math
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


# ------------------------------------------------------------------------------------------------
# reference order <-> device rows
# ------------------------------------------------------------------------------------------------
def device_dk(lay, n_d_k, pad=0):
    """(D, K) -> the (D, KP) int32 rows of n_dk: column topic_pos[k] holds n_d_k[:, k], the padding ``pad``"""
    n_d_k = np.asarray(n_d_k)
    rows = np.full((n_d_k.shape[0], lay.KP), pad, dtype=np.int32)
    rows[:, lay.topic_pos] = n_d_k.astype(np.int32)
    return rows


def device_kw(lay, n_k_v, pad=0):
    """(K, V) -> the (V, KP) int32 rows of n_kw"""
    return device_dk(lay, np.asarray(n_k_v).T, pad)


def device_vec(lay, x, pad=0, dtype=np.int32):
    """(K,) -> (KP,) in device order (n_k as int32, den as float64), the padding ``pad``"""
    v = np.full(lay.KP, pad, dtype=dtype)
    v[lay.topic_pos] = np.asarray(x).astype(dtype)
    return v


def padding_positions(lay):
    return np.flatnonzero(lay.pos_topic < 0)


def same_bits(got, want):
    """None when the two float64 arrays hold NaN at the same places and the same BITS elsewhere (-0.0 is not 0.0), else a
    description of the first difference"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return "shapes %r != %r" % (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~gn & ~wn & (got.view(np.uint64) != want.view(np.uint64)))
    if not bad.any():
        return None
    i = tuple(int(x) for x in np.argwhere(bad)[0])
    return "%d of %d entries differ, the first at %r: got %r (%s), want %r (%s)" % (
        int(bad.sum()), bad.size, i, float(got[i]), float(got[i]).hex(), float(want[i]), float(want[i]).hex())


def assert_same_bits(got, want, what=""):
    msg = same_bits(got, want)
    assert msg is None, "%s: %s" % (what, msg)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
MASKS = ("all", "root_and_3", "single", "mixed")


def label_rows(rng, D, K, masks):
    """(D, K) uint8.  all: every label; root_and_3: topic 0 and up to three more; single: one label; mixed: document d takes one
    of the three by d % 4 and NO label at all where d % 4 == 3 (from document 4096 on the kinds are shifted by one, so documents
    d and d + 4096, which one workgroup of a wide read-out walks in turn, are of different kinds)."""
    labs = np.zeros((D, K), dtype=np.uint8)
    for d in range(D):
        kind = masks if masks != "mixed" else ("all", "root_and_3", "single", "none")[(d + d // WIDE_GRID) % 4]
        if kind == "all":
            labs[d] = 1
        elif kind == "single":
            labs[d, rng.integers(0, K)] = 1
        elif kind == "root_and_3":
            labs[d, 0] = 1
            if K > 1:
                labs[d, 1 + rng.choice(K - 1, min(3, K - 1), replace=False)] = 1
    return labs


def theta_counts(rng, labs, masks):
    """(D, K) int64 counts for the label rows: small random counts on the labelled topics (and a few off them: the kernel reads
    counts whatever the mask says); document 0 (D > 2) holds counts near 2^31 - 1 in several topics, the last document a single
    non-zero count; with ``mixed`` masks the label-free documents alternate between counts and none (0/0: a NaN row)."""
    D, K = labs.shape
    n = (rng.integers(0, 40, (D, K)) * (labs != 0)).astype(np.int64)
    stray = rng.random((D, K)) < 0.02
    n[stray] += rng.integers(1, 9, int(stray.sum()))
    if masks == "mixed":
        for d in np.flatnonzero(labs.sum(axis=1) == 0):
            n[d] = 0
            if (d // 4) % 2 == 0:
                n[d, rng.integers(0, K, min(K, 3))] = rng.integers(1, 30, min(K, 3))
    if D > 2:
        hot = rng.choice(K, min(K, 5), replace=False)
        n[0, hot] = INT32_MAX - rng.integers(0, 3, len(hot))
        n[D - 1] = 0
        n[D - 1, rng.integers(0, K)] = 17
    return n


def poisoned_old(rng, shape):
    """random doubles in [0, 1) with NaN, +inf, -inf, -0.0 and a denormal planted at places spread over both axes"""
    old = rng.random(shape)
    flat = old.reshape(-1)
    n = flat.size
    if n >= 2 * len(POISONS):
        where = (np.arange(len(POISONS)) * (n // len(POISONS)) + rng.integers(0, n // len(POISONS), len(POISONS))) % n
    else:
        where = np.arange(min(n, len(POISONS)))
    for i, p in zip(where, POISONS):
        flat[i] = p
    return old


# ------------------------------------------------------------------------------------------------
# llda_loglik per document
# ------------------------------------------------------------------------------------------------
def loglik_case(K, masks, seed=8, D=70, lens=None, wide=False):
    """a corpus for llda_loglik: D documents over V = 53 words, documents of 0, 1 and 90 sites among them (or ``lens``), label
    rows by ``masks``, counts by a numpy count of a random assignment to labelled topics -- device rows with zero padding.
    -> (layout, D, V, lens, doc_off, word, labs, (n_dk, n_kw, n_k))"""
    lay = layout(K)
    assert bool(lay.wide) == wide
    V = 53
    rng = np.random.default_rng([seed, K, ("all", "root_and_3", "single").index(masks)])
    lens = np.resize([0, 1, 90, 5, 17, 2, 33], D) if lens is None else np.asarray(lens)
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    labs = np.zeros((D, K), dtype=np.uint8)
    for d in range(D):
        if masks == "all":
            labs[d] = 1
        elif masks == "single":
            labs[d, rng.integers(0, K)] = 1
        else:
            labs[d, 0] = 1
            labs[d, 1 + rng.choice(K - 1, 3, replace=False)] = 1
    word = rng.integers(0, V, S).astype(np.int32)
    freq = rng.integers(1, 20, S).astype(np.int32)
    topic = np.concatenate([rng.choice(np.flatnonzero(labs[d]), lens[d]) for d in range(D)]).astype(np.int64)
    z = lay.topic_pos[topic].astype(np.int64)
    rows = np.repeat(np.arange(D), lens)
    n_dk = np.zeros((D, lay.KP), dtype=np.int32)
    n_kw = np.zeros((V, lay.KP), dtype=np.int32)
    np.add.at(n_dk, (rows, z), freq)
    np.add.at(n_kw, (word.astype(np.int64), z), freq)
    n_k = np.bincount(z, weights=freq, minlength=lay.KP).astype(np.int32)
    return lay, D, V, lens, doc_off, word, labs, [n_dk, n_kw, n_k]


def loglik_high_precision(lay, doc_off, word, labs, n_dk, n_kw, n_k, V, alpha, beta):
    """out_doc in long double (64 significant bits on x86: its own error is 2^-11 of a double's)"""
    ld = np.longdouble
    tp = lay.topic_pos.astype(np.int64)
    num = n_dk[:, tp].astype(ld) + labs.astype(ld) * ld(alpha)
    th = num / num.sum(axis=1)[:, None]
    ph = (n_kw[:, tp].T.astype(ld) + ld(beta)) / (n_k[tp].astype(ld)[:, None] + ld(V) * ld(beta))
    out = np.zeros(len(doc_off) - 1, dtype=ld)
    for d in range(len(out)):
        w = word[doc_off[d]:doc_off[d + 1]]
        if len(w):
            out[d] = -np.log((th[d][:, None] * ph[:, w]).sum(axis=0)).sum()
    return out
