"""The kernels that carry a sweep's results into the counts and the counts into their narrow images, each called directly through
lda_thesis_amd._native and held against a plain numpy statement of the same operation -- exact integers everywhere but llda_loglik:

    llda_commit_log, llda_apply_rows, llda_apply_delta, llda_count_init, llda_loglik    tests/helpers.py OracleBackend (on CPU tensors)
    llda_pack_rows16, llda_pack_rows16_all, llda_pack_image, llda_pack_image_cols       tests/countref.py (written from the readers' side)

The shapes are the smallest that reach every branch of csrc/kernel_counts.hpp and of the packer at the end of csrc/kernel_quad.hpp:
the 16-byte path of the commit log with every head, its fall-back for differently aligned arrays, both flushes for int32 and
int16-pair rows, shared rows; the scalar tail, the unaligned path and the grid stride of llda_apply_delta; one and four wavefronts
per workgroup and the grid stride of llda_count_init; the ballot segments of llda_pack_rows16_all; the saturation of negative
counts and the second stride of the image packers.  Every buffer a kernel writes sits between two margins of 64 sentinel elements
(countref.Guarded), which must come back untouched."""
import numpy as np
import pytest

import countref
from countref import Guarded
from readoutref import loglik_case, loglik_high_precision

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
COMMIT_KS = [12, 130, 512, 1100, 7688]          # KP = 16, 192, 512, 1536 (wide), 8192 (128 KB of LDS for the commit log)
GAP = 0x3C3C3C3C                                # between the rows of a row table: never written


def _oracle():
    from helpers import OracleBackend
    return OracleBackend(None)


def _layout(K):
    from lda_thesis_amd.layout import group_layout
    return group_layout(K)


def _cpu(a):
    import torch
    return torch.from_numpy(a)


def _dev(a, shift=0):
    """device copy of the 1-D array ``a`` that starts ``shift`` elements behind a 16-byte boundary"""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.concatenate([np.zeros(16 + shift, dtype=a.dtype), a])).cuda()[16 + shift:]


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# llda_commit_log
# ------------------------------------------------------------------------------------------------
def _place_rows(rng, pair_of_row, KP):
    """rows of KP int32 or KP / 2 pair words in a random order, GAP words between them -> (row_off int64, buffer length)"""
    off = np.zeros(len(pair_of_row), dtype=np.int64)
    cur = 3
    for r in rng.permutation(len(pair_of_row)):
        off[r] = ~cur if pair_of_row[r] else cur
        cur += (KP // 2 if pair_of_row[r] else KP) + 3
    return off, cur


def build_commit_case(K, kind, seed=0):
    """One commit log that holds every item shape of the issue list for the target kind ``plain`` (row v at v * KP), ``rows32`` (a row
    table of int32 rows) or ``mixed`` (a row table of int32 rows and int16-pair rows).  -> dict of numpy arrays."""
    KP = _layout(K).KP
    rng = np.random.default_rng([seed, K, ("plain", "rows32", "mixed").index(kind)])
    items, word_pair = [], []                   # items: (word, shared, begin mod 4, zo, zn, f)

    def new_word(pair):
        word_pair.append(pair)
        return len(word_pair) - 1

    def entries(n, pair, contend=False, fmax=50):
        zo, zn = rng.integers(0, KP, n), rng.integers(0, KP, n)
        same = rng.random(n) < 0.2
        zn[same] = zo[same]                                     # no change
        f = rng.integers(1, fmax + 1, n)
        if contend:                                             # every entry on one pair of positions
            zo[:], zn[:] = rng.choice(KP, 2, replace=False)
        elif n >= 6:
            j = 2 * int(rng.integers(0, KP // 2))
            where = rng.choice(n, 6, replace=False)
            # no change; first <-> last position; the two halves of one pair word, both directions: the low half ends above its
            # start and the high half below it
            for i, (a, b) in zip(where, [(5, 5), (0, KP - 1), (KP - 1, 0), (j, j + 1), (j + 1, j), (j + 1, j)]):
                zo[i], zn[i] = a, b
            f[where[3:]] = 7, 30, 11
        if pair and f.sum() > 32767:                            # the mass of a word on a pair row stays <= 32767
            f[:] = 1
            f[:(32767 - n) // 49] = 50
            assert f.sum() <= 32767
        return zo, zn, f

    for pair in ([False, True] if kind == "mixed" else [False]):
        nw = KP // 2 if pair else KP                            # the threshold between the two flushes
        for n in sorted({0, 1, 3, 63, 64, 65, 255, 256, 257, nw - 1, nw, nw + 1, 4 * nw + 5}):
            for r in (range(4) if n >= 256 else [int(rng.integers(0, 4))]):      # begins = 0 .. 3 mod 4: heads of 0, 3, 2, 1 entries
                items.append((new_word(pair), False, r) + entries(n, pair))
        for n in (65, 257, 4 * nw + 5):
            items.append((new_word(pair), False, int(rng.integers(0, 4))) + entries(n, pair, contend=True))
        if pair:                                                # one word reaches exactly -32767 in one half and +32767 in the other
            j = 2 * int(rng.integers(0, KP // 2))
            f = np.full(700, 46)
            f[:567] += 1
            assert f.sum() == 32767
            items.append((new_word(True), False, 1, np.full(700, j), np.full(700, j + 1), f))
        hot = new_word(pair)                                    # a hot word cut into five items that share its row
        for i, n in enumerate((300, 17, 256, nw + 3, 64)):
            items.append((hot, True, i % 4) + entries(n, pair, fmax=6 if pair else 50))
    while len(items) % 4 != 3:
        items.append((new_word(False), False, 0) + entries(0, False))
    items = [items[i] for i in rng.permutation(len(items))]
    assert len(items) < 2000

    begins, cur = [], 0
    for _, _, r, zo, _, _ in items:
        cur += (r - cur) % 4
        begins.append(cur)
        cur += len(zo)
    total = cur + 3
    log = (rng.integers(0, KP, total) | (rng.integers(0, KP, total) << 16)).astype(np.uint32)     # (the gaps: entries of no item)
    freq = np.full(total, 99, dtype=np.int32)
    for b, (_, _, _, zo, zn, f) in zip(begins, items):
        log[b:b + len(zo)] = (zo | (zn << 16)).astype(np.uint32)
        freq[b:b + len(zo)] = f
    word_of = rng.permutation(len(word_pair))                   # word ids in no particular order
    pair_of_word = np.zeros(len(word_pair), dtype=bool)
    pair_of_word[word_of] = word_pair
    if kind == "plain":
        row_off, target = None, rng.integers(-1000, 1001, len(word_pair) * KP).astype(np.int32)
    else:
        row_off, n = _place_rows(rng, pair_of_word, KP)
        target = np.full(n, GAP, dtype=np.int32)
        for v, o in enumerate(row_off):
            if o < 0:
                target[~o:~o + KP // 2] = rng.integers(-50, 51, KP // 2)
            else:
                target[o:o + KP] = rng.integers(-1000, 1001, KP)
    item_word = np.array([int(word_of[w]) | (0x80000000 if sh else 0) for w, sh, _, _, _, _ in items], dtype=np.uint32).view(np.int32)
    return dict(K=K, KP=KP, item_begin=np.array(begins, dtype=np.int64), item_len=np.array([len(it[3]) for it in items], dtype=np.int32),
                item_word=item_word, log=log, freq=freq, row_off=row_off, target=target,
                n_k=rng.integers(0, 10 ** 6, KP).astype(np.int32), n_k_delta=rng.integers(-1000, 1001, KP).astype(np.int32))


_COMMIT_CASES = {}


def commit_case(K, kind):
    """the case and what the numpy statement makes of it (computed once, never changed)"""
    if (K, kind) not in _COMMIT_CASES:
        c = build_commit_case(K, kind)
        c["want"] = commit_expected(c, len(c["item_len"]), True)
        for k in c:
            if isinstance(c[k], np.ndarray):
                c[k].setflags(write=False)
        _COMMIT_CASES[K, kind] = c
    return _COMMIT_CASES[K, kind]


def commit_expected(c, n_items, with_nk):
    t, nk, nkd = _cpu(c["target"].copy()), _cpu(c["n_k"].copy()), _cpu(c["n_k_delta"].copy())
    _oracle().commit_log(_cpu(c["item_begin"][:n_items].copy()), _cpu(c["item_len"][:n_items].copy()), _cpu(c["item_word"][:n_items].copy()),
                         _cpu(c["log"].view(np.int32).copy()), _cpu(c["freq"].copy()), c["K"], t, nk if with_nk else None,
                         nkd if with_nk else None, None if c["row_off"] is None else _cpu(c["row_off"].copy()))
    return t.numpy(), nk.numpy(), nkd.numpy()


def run_commit(c, n_items, with_nk, shift_log=0, shift_freq=0):
    from lda_thesis_amd import _native as nat
    target, n_k, n_k_delta = Guarded(c["target"]), Guarded(c["n_k"]), Guarded(c["n_k_delta"])
    nat.commit_log(_dev(c["item_begin"][:n_items]), _dev(c["item_len"][:n_items]), _dev(c["item_word"][:n_items]),
                   _dev(c["log"], shift_log), _dev(c["freq"], shift_freq), c["K"], target.t, n_k.t if with_nk else None,
                   n_k_delta.t if with_nk else None, None if c["row_off"] is None else _dev(c["row_off"]))
    _sync()
    return target.host("target"), n_k.host("n_k"), n_k_delta.host("n_k_delta")


@pytest.mark.parametrize("arrays", ["same_alignment", "log_and_freq_aligned_differently"])
@pytest.mark.parametrize("kind", ["plain", "rows32", "mixed"])
@pytest.mark.parametrize("K", COMMIT_KS)
def test_commit_log_equals_the_numpy_fold(K, kind, arrays):
    """every item shape in one log (build_commit_case), 4 k + 3 items: lengths around 64, 256 and the threshold between the two
    flushes (KP entries for an int32 row, KP / 2 for a pair row), items of 256 entries and more at every begin mod 4, and the same
    log once more with ``log`` one and ``freq`` two entries behind a 16-byte boundary -- one entry per load.  The whole target is
    compared, the words between the rows of a row table included; n_k takes its delta and the delta is zeroed."""
    c = commit_case(K, kind)
    n = len(c["item_len"])
    assert n % 4 == 3
    sl, sf = (0, 0) if arrays == "same_alignment" else (1, 2)
    got = run_commit(c, n, True, sl, sf)
    for g, w, what in zip(got, c["want"], ("target", "n_k", "n_k_delta")):
        np.testing.assert_array_equal(g, w, err_msg="K=%d %s %s: %s" % (K, kind, arrays, what))
    np.testing.assert_array_equal(c["want"][1], c["n_k"] + c["n_k_delta"])
    assert not c["want"][2].any()
    assert (got[0] != c["target"]).any()


@pytest.mark.parametrize("with_nk", [True, False], ids=["n_k", "no_n_k"])
@pytest.mark.parametrize("n_items", [0, 1, 4, 5])
@pytest.mark.parametrize("K", [130, 512])
def test_commit_log_item_counts(K, n_items, with_nk):
    """the first 0, 1, 4, 5 items of the mixed log (a workgroup takes four): with no item at all n_k still takes its delta and the
    delta is zeroed, and without n_k nothing but the items' rows is touched"""
    c = commit_case(K, "mixed")
    want = commit_expected(c, n_items, with_nk)
    got = run_commit(c, n_items, with_nk)
    for g, w, what in zip(got, want, ("target", "n_k", "n_k_delta")):
        np.testing.assert_array_equal(g, w, err_msg="K=%d, %d items: %s" % (K, n_items, what))
    if n_items == 0:
        np.testing.assert_array_equal(got[0], c["target"])
    if with_nk:
        np.testing.assert_array_equal(got[1], c["n_k"] + c["n_k_delta"])
        assert not got[2].any()
    else:
        np.testing.assert_array_equal(got[1], c["n_k"])
        np.testing.assert_array_equal(got[2], c["n_k_delta"])


# ------------------------------------------------------------------------------------------------
# llda_apply_rows
# ------------------------------------------------------------------------------------------------
HALVES = [-32768, -1, 0, 1, 32767]


def build_rows_case(K, V, seed=1):
    KP = _layout(K).KP
    rng = np.random.default_rng([seed, K, V])
    n_rows = V + 1
    pair = rng.random(n_rows) < 0.5
    pair[0], pair[-1] = True, False
    row_off, n = _place_rows(rng, pair, KP)
    rows = np.full(n, GAP, dtype=np.int32)
    lo_hi = np.zeros((n_rows, KP // 2, 2), dtype=np.int64)      # the halves the pair words were made of
    combos = [(lo, hi) for lo in HALVES for hi in HALVES]
    nxt = 0
    for r, o in enumerate(row_off):
        if o < 0:
            h = rng.integers(-32768, 32768, (KP // 2, 2))
            h[rng.random(KP // 2) < 0.3] = 0                    # words of zero are skipped
            for j in rng.choice(KP // 2, min(KP // 2, 25), replace=False):
                h[j] = combos[nxt % 25]
                nxt += 1
            lo_hi[r] = h
            rows[~o:~o + KP // 2] = (h[:, 0] + h[:, 1] * 65536).astype(np.int32)      # (int32 arithmetic: wraps as the all-reduce's adds do)
        else:
            x = rng.integers(-10 ** 6, 10 ** 6, KP)
            x[rng.random(KP) < 0.3] = 0
            rows[o:o + KP] = x
    assert V < 25 or nxt >= 25
    counts = rng.integers(1, 10 ** 6, n_rows * KP).astype(np.int32)
    return dict(K=K, KP=KP, row_off=row_off, rows=rows, counts=counts, lo_hi=lo_hi)


@pytest.mark.parametrize("V", [1, 3, 4, 5, 203])
@pytest.mark.parametrize("K", COMMIT_KS)
def test_apply_rows_equals_the_numpy_decode(K, V):
    """V + 1 rows onto the fused [n_kw | n_k] buffer, int32 rows and int16-pair rows mixed, counts that are not zero before the
    call.  The pair words take every combination of the halves -32768, -1, 0, 1, 32767 (a negative low half borrows from the
    high one) besides random ones.  (-32768 in the high half under a negative low half is no int32: such a word wraps and both
    sides decode the wrapped word; every other word must come apart into exactly the halves it was made of.)"""
    from lda_thesis_amd import _native as nat
    c = build_rows_case(K, V)
    KP = c["KP"]
    want_rows, want_counts = _cpu(c["rows"].copy()), _cpu(c["counts"].copy())
    _oracle().apply_rows(_cpu(c["row_off"].copy()), want_rows, K, want_counts)
    want_rows, want_counts = want_rows.numpy(), want_counts.numpy().reshape(V + 1, KP)
    for r, o in enumerate(c["row_off"]):                         # the reference itself against the halves, where they are an int32
        if o < 0:
            lo, hi = c["lo_hi"][r, :, 0], c["lo_hi"][r, :, 1]
            ok = (hi * 65536 + lo >= I32_MIN) & (hi * 65536 + lo <= I32_MAX)
            assert ok.sum() >= KP // 2 - 8
            start = c["counts"].reshape(V + 1, KP)[r].astype(np.int64)
            np.testing.assert_array_equal(want_counts[r, 0::2][ok], (start[0::2] + lo)[ok])
            np.testing.assert_array_equal(want_counts[r, 1::2][ok], (start[1::2] + hi)[ok])
    rows, counts = Guarded(c["rows"]), Guarded(c["counts"])
    nat.apply_rows(_dev(c["row_off"]), rows.t, K, counts.t)
    _sync()
    got_rows = rows.host("rows")
    np.testing.assert_array_equal(counts.host("counts").reshape(V + 1, KP), want_counts)
    np.testing.assert_array_equal(got_rows, want_rows)
    for o in c["row_off"]:                                       # every row word is zero afterwards (and only those)
        assert not (got_rows[~o:~o + KP // 2] if o < 0 else got_rows[o:o + KP]).any()
    assert (got_rows == GAP).sum() == (c["rows"] == GAP).sum() == 3 * (V + 2)


# ------------------------------------------------------------------------------------------------
# llda_apply_delta
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ["both_aligned", "both_one_element_off", "counts_off", "delta_off"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 2 * 2097152 + 3])
def test_apply_delta_equals_numpy(n, align):
    """the scalar tail (n not a multiple of 4), pointers that are not 16-byte aligned (no vector path at all) and, with more than
    2 097 152 * 2 counts, the grid stride; half of the aligned groups of four have no delta at all and extremes sit at both ends
    (INT32_MAX - 1 + 1, INT32_MIN + 1 - 1)"""
    from lda_thesis_amd import _native as nat
    rng = np.random.default_rng([2, n])
    counts = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int32)
    delta = rng.integers(-10 ** 6, 10 ** 6, n).astype(np.int32)
    delta[np.repeat(rng.random((n + 3) // 4) < 0.5, 4)[:n]] = 0
    counts[0], delta[0] = I32_MAX - 1, 1
    if n > 1:
        counts[n - 1], delta[n - 1] = I32_MIN + 1, -1
    want_c, want_d = _cpu(counts.copy()), _cpu(delta.copy())
    _oracle().apply_delta(want_c, want_d)
    sc, sd = {"both_aligned": (0, 0), "both_one_element_off": (1, 1), "counts_off": (1, 0), "delta_off": (0, 1)}[align]
    c, d = Guarded(counts, sc), Guarded(delta, sd)
    assert (c.t.data_ptr() % 16, d.t.data_ptr() % 16) == (4 * sc, 4 * sd)
    nat.apply_delta(c.t, d.t)
    _sync()
    np.testing.assert_array_equal(c.host("counts"), want_c.numpy())
    got_d = d.host("delta")
    assert not got_d.any() and not want_d.numpy().any()
    assert want_c.numpy()[0] == I32_MAX and (n == 1 or want_c.numpy()[n - 1] == I32_MIN)


# ------------------------------------------------------------------------------------------------
# llda_count_init
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [5, 130, 512, 2048, 2400, 7688])
def test_count_init_equals_numpy_add_at(K):
    """np.add.at / bincount against the device histograms: K = 2048 is the last layout with four wavefronts per workgroup, K = 2400
    (KP = 3072) the first with one; 8 209 resp. 2 057 documents make every wavefront take a second document (the grid is capped at
    2 048 workgroups).  Lengths 0, 1, 63, 64, 65, 300 in turn, frequencies 1 .. 1000, word 0 in every document, one document with
    all of its sites on one position."""
    from lda_thesis_amd import _native as nat
    lay = _layout(K)
    KP, V = lay.KP, 97
    one_wave = 5 * KP * 4 > 48 * 1024
    assert one_wave == (K >= 2400)
    D = (2048 if one_wave else 8192 + 8) + 9
    rng = np.random.default_rng([3, K])
    lens = np.resize([0, 1, 63, 64, 65, 300], D)
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(0, V, S).astype(np.int32)
    word[doc_off[:-1][lens > 0]] = 0
    freq = rng.integers(1, 1001, S).astype(np.int32)
    z = lay.topic_pos[rng.integers(0, K, S)].astype(np.int32)
    z[doc_off[5]:doc_off[6]] = lay.topic_pos[K - 1]
    assert lens[5] == 300
    want = [_cpu(np.zeros(s, dtype=np.int32)) for s in ((D, KP), (V, KP), (KP,))]
    _oracle().count_init(_cpu(doc_off), _cpu(word), _cpu(freq), _cpu(z), D, K, *want)
    got = [Guarded(np.zeros(s, dtype=np.int32)) for s in (D * KP, V * KP, KP)]
    nat.count_init(_dev(doc_off), _dev(word), _dev(freq), _dev(z), D, K, *[g.t for g in got])
    _sync()
    for g, w, what in zip(got, want, ("n_dk", "n_kw", "n_k")):
        np.testing.assert_array_equal(g.host(what).reshape(w.shape), w.numpy(), err_msg="K=%d %s" % (K, what))
    assert int(want[2].sum()) == int(freq.astype(np.int64).sum())
    assert not want[2].numpy()[lay.pos_topic < 0].any()


# ------------------------------------------------------------------------------------------------
# llda_pack_rows16, llda_pack_rows16_all
# ------------------------------------------------------------------------------------------------
ROW_KS = [100, 128, 200, 256, 400, 512, 1024]
ROW_VS = [1, 2, 3, 4, 5, 9, 131]
PATTERN = 0x1234                                # what n_kw16 holds before a call
WIDE_VALUES = [65536, -1, I32_MIN]


def _plant(n_kw, G, v, place, value):
    """exactly one count of row v outside 0 .. 65535: in the first slot of the first lane, the last slot of the last lane, or
    in a lane in the middle"""
    g, s = {"first": (0, 0), "last": (G - 1, 15), "middle": (G // 2 - 1, 6)}[place]
    n_kw[v, ((s // 4) * G + g) * 4 + s % 4] = value


def rows_cases(G, V, rng):
    """-> [(n_kw (V, 16 G) int32, rows that hold a count outside 0 .. 65535)]: the small V with one such row at every position in
    turn (and none), V = 131 with twelve of them, eight rows apart and one position further inside its wavefront each time, so that
    every position of a row inside a wavefront (four rows for G = 8, two for G = 16) is taken with fitting neighbours"""
    plants = [(p, x) for p in ("first", "last", "middle") for x in WIDE_VALUES]
    out = []
    if V < 100:
        out.append((rng.integers(0, 65536, (V, 16 * G)).astype(np.int32), []))
        for v in range(V):
            n_kw = rng.integers(0, 65536, (V, 16 * G)).astype(np.int32)
            _plant(n_kw, G, v, *plants[(v + V) % 9])
            out.append((n_kw, [v]))
    else:
        n_kw = rng.integers(0, 65536, (V, 16 * G)).astype(np.int32)
        wide = [8 * i + i % 4 for i in range(12)] + [V - 1]
        for i, v in enumerate(wide):
            _plant(n_kw, G, v, *plants[i % 9])
        out.append((n_kw, wide))
    return out


@pytest.mark.parametrize("V", ROW_VS)
@pytest.mark.parametrize("K", ROW_KS)
def test_pack_rows16_all_flags_every_row_on_its_own(K, V):
    """row16 must equal the reference flag for EVERY row: no sweep result shows a flag that leaked from a row to the rows that share
    its wavefront (they are read from the int32 row instead, only slower), and a row flagged as fitting while it does not corrupts
    the state of the documents that draw the word.  The image is compared for the rows that fit (the others are never read)."""
    from lda_thesis_amd import _native as nat
    lay = _layout(K)
    if not nat.quad_ok(K):
        with pytest.raises(nat.NativeError):
            nat.pack_rows16_all(_dev(np.zeros(16, np.int32)), K, _dev(np.zeros(16, np.int16)), _dev(np.zeros(1, np.uint8)))
        return
    G = lay.G
    assert lay.T == 16 and G in (8, 16, 32)
    for n_kw, wide in rows_cases(G, V, np.random.default_rng([4, K, V])):
        img, flags = Guarded(np.full(V * 16 * G, PATTERN, dtype=np.uint16)), Guarded(np.full(V, 7, dtype=np.uint8))
        nat.pack_rows16_all(_dev(n_kw), K, img.t, flags.t)
        _sync()
        want_img, want_flags = countref.pack_rows16_all_ref(n_kw, G)
        assert np.flatnonzero(want_flags == 0).tolist() == sorted(wide)
        np.testing.assert_array_equal(flags.host("row16"), want_flags, err_msg="K=%d V=%d wide rows %s" % (K, V, wide))
        fits = want_flags == 1
        np.testing.assert_array_equal(img.host("n_kw16").reshape(V, -1)[fits], want_img[fits])
        # ... and the loader's order gives the counts back
        np.testing.assert_array_equal(countref.decode_quad(img.host().reshape(V, -1), G)[fits], countref.lane_slot(n_kw, G)[fits])


@pytest.mark.parametrize("V", ROW_VS)
@pytest.mark.parametrize("K", ROW_KS)
def test_pack_rows16_packs_the_flagged_rows_only(K, V):
    """rows that are not flagged keep what n_kw16 held; status bit 2 is set exactly when a FLAGGED row holds a count outside
    0 .. 65535, stays 0 when only unflagged rows do, and status = None is accepted"""
    from lda_thesis_amd import _native as nat
    lay = _layout(K)
    if not nat.rows16_ok(K):
        with pytest.raises(nat.NativeError):
            nat.pack_rows16(_dev(np.zeros(16, np.int32)), _dev(np.zeros(1, np.uint8)), K, _dev(np.zeros(16, np.int16)), None)
        return
    G = lay.G
    assert lay.T == 16 and G in (32, 64)
    rng = np.random.default_rng([5, K, V])
    for n_kw, wide in rows_cases(G, V, rng):
        flags = (rng.random(V) < 0.6).astype(np.uint8)
        flags[wide] = 0
        runs = [(flags, True), (flags, False)]
        if wide:
            hit = flags.copy()
            hit[wide[-1]] = 1
            runs.append((hit, True))
        for row16, with_status in runs:
            img, status = Guarded(np.full(V * 16 * G, PATTERN, dtype=np.uint16)), Guarded(np.zeros(4, dtype=np.int32))
            nat.pack_rows16(_dev(n_kw), _dev(row16), K, img.t, status.t if with_status else None)
            _sync()
            want_img, want_status = countref.pack_rows16_ref(n_kw, row16, G, np.full((V, 16 * G), PATTERN, dtype=np.uint16))
            assert want_status == (4 if wide and row16[wide[-1]] else 0)
            got = img.host("n_kw16").reshape(V, -1)
            np.testing.assert_array_equal(got, want_img, err_msg="K=%d V=%d flags %s" % (K, V, row16.tolist()))
            assert (got[row16 == 0] == PATTERN).all()
            np.testing.assert_array_equal(countref.decode_rows16(got, G)[row16 != 0] & 0xffff,
                                          countref.lane_slot(n_kw, G)[row16 != 0] & 0xffff)
            assert status.host("status").tolist() == [want_status if with_status else 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------
# llda_pack_image, llda_pack_image_cols
# ------------------------------------------------------------------------------------------------
SPECIAL = [I32_MIN, -1, 0, 254, 255, 256, 65534, 65535, 65536, I32_MAX]


def image_values(rng, n):
    """counts around both saturation values, anywhere in int32, and the special ones"""
    m = min(n, 1 << 20)                                         # (a longer array repeats: it is there for its length)
    kind = rng.integers(0, 4, m)
    v = np.where(kind == 0, rng.integers(0, 300, m), np.where(kind == 1, rng.integers(65000, 66000, m),
                 np.where(kind == 2, rng.integers(I32_MIN, I32_MAX + 1, m), rng.choice(SPECIAL, m))))
    return np.resize(v.astype(np.int32), n)


@pytest.mark.parametrize("n", [4, 8, 1028, 16777216 + 12])
@pytest.mark.parametrize("bits", [8, 16])
def test_pack_image_saturates_like_the_reference(bits, n):
    """min(count as uint32, 255 | 65535): a negative count saturates too.  16 777 216 + 12 counts (64 MB) are the fewest that make
    a thread take a second stride."""
    from lda_thesis_amd import _native as nat
    rng = np.random.default_rng([6, bits, n])
    for first in range(0, len(SPECIAL), n) if n < len(SPECIAL) else [0]:
        n_kw = image_values(rng, n)
        sp = SPECIAL[first:first + n]
        n_kw[:len(sp)] = sp
        if n >= 14:
            n_kw[n - 4:] = SPECIAL[0], SPECIAL[-1], SPECIAL[1], SPECIAL[8 if bits == 16 else 5]
        img = Guarded(np.full(n, 0x77, dtype=np.uint8 if bits == 8 else np.uint16))
        nat.pack_image(_dev(n_kw), img.t)
        _sync()
        want = countref.pack_image_ref(n_kw, bits)
        assert n < 14 or want[n - 4:].tolist() == [255 if bits == 8 else 65535] * 4
        np.testing.assert_array_equal(img.host("img"), want)


@pytest.mark.parametrize("K,V", [(5, 1), (5, 7), (5, 8192 + 5), (130, 1), (130, 7), (512, 1), (512, 7), (2048, 1), (2048, 7)])
@pytest.mark.parametrize("bits", [8, 16])
def test_pack_image_cols_gathers_and_saturates(bits, K, V):
    """the same image with its columns in the order of a random permutation of the positions; 8 192 + 5 rows make a workgroup take a
    second row"""
    import torch
    from lda_thesis_amd import _native as nat
    KP = _layout(K).KP
    rng = np.random.default_rng([7, bits, K, V])
    n_kw = image_values(rng, V * KP).reshape(V, KP)
    n_kw[0, :min(KP, len(SPECIAL))] = SPECIAL[:KP]
    n_kw[V - 1, KP - 4:] = SPECIAL[0], SPECIAL[-1], SPECIAL[1], SPECIAL[4]
    col_src = rng.permutation(KP).astype(np.int32)
    img = Guarded(np.full(V * KP, 0x77, dtype=np.uint8 if bits == 8 else np.uint16))
    nat.pack_image_cols(torch.from_numpy(n_kw).cuda(), K, _dev(col_src), img.t)
    _sync()
    np.testing.assert_array_equal(img.host("img").reshape(V, KP), countref.pack_image_ref(n_kw, bits, col_src))


# ------------------------------------------------------------------------------------------------
# llda_loglik on the tuned layouts
# ------------------------------------------------------------------------------------------------
U = 2.0 ** -53


# loglik_case (which refuses a wide layout here) and loglik_high_precision live in tests/readoutref.py: the test of the wide layouts,
# tests/test_gpu_readout_direct.py, shares them


@pytest.mark.parametrize("masks", ["all", "root_and_3", "single"])
@pytest.mark.parametrize("K", [5, 40, 130, 392, 512, 1000])
def test_loglik_per_document_on_the_tuned_layouts(K, masks):
    """out_doc document by document (one wrong document disappears in the perplexity of a corpus) against OracleBackend.loglik and
    against the same sum in long double, for 8, 16, 32 and 64 lanes per document, layouts with padding, and label masks of all
    topics, the root and three labels, a single label; documents of 0, 1 and 90 sites among the 70.  alpha is not a round number, so
    a mask that leaves it out of a denominator moves the value in its third digit.

    The bound is derived, not fitted.  u = 2^-53; a document of n sites whose value is S (every term -log(dot) is positive,
    dot < 1).  The kernel's dot: each theta carries 2 roundings and the error of its denominator (a sum of at most KP - 1
    additions of non-negative terms: relative error below (KP - 1) u), each phi 3 roundings, their product 1, and the sum of the
    products again below (KP - 1) u: dot is within (2 KP + 5) u of the true value, relatively, and so is log(dot) absolutely.  The
    device's log is good to 1 ulp (2 u |log|, S in total), and each of the n additions to the accumulator rounds by at most u S.
    Together  |device - exact| <= (n (2 KP + 5) + 2 S + n S) u,  asserted with 1 % on top for the second-order terms; the float64
    reference (numpy, the same operations in another order) is within the same bound, so the two float64 values may differ by twice
    as much.  The numpy reference itself uses at most 0.17 of the bound (K = 5, where the n S term of the accumulator dominates) and
    0.007 - 0.05 of it from K = 40 on; the test prints the device's ratio for every case (pytest -s).  The device's largest
    ratios, for this kernel and the wide one, are kept in profiles/readout_loglik_bound.md."""
    import torch
    from lda_thesis_amd import _native as nat
    lay, D, V, lens, doc_off, word, labs, (n_dk, n_kw, n_k) = loglik_case(K, masks)
    assert lay.G == {5: 8, 40: 8, 130: 16, 392: 32, 512: 32, 1000: 64}[K]
    alpha, beta = 0.37, 0.013
    lab_mask = lay.lane_masks(labs)
    ref = _cpu(np.zeros(D))
    _oracle().loglik(_cpu(doc_off), _cpu(word), _cpu(lab_mask.view(np.int16)), _cpu(n_dk), _cpu(n_kw), _cpu(n_k), D, V, K, alpha, beta, ref)
    ref = ref.numpy()
    out = Guarded(np.full(D, 7.0))
    nat.loglik(_dev(doc_off), _dev(word), _dev(lab_mask.view(np.int16)), torch.from_numpy(n_dk).cuda(), torch.from_numpy(n_kw).cuda(),
               _dev(n_k), D, V, K, alpha, beta, out.t)
    _sync()
    got = out.host("out_doc")
    assert (got[lens == 0] == 0.0).all() and (lens == 0).sum() == 10 and (got[lens > 0] > 0).all()
    bound = 1.01 * U * (lens * (2 * lay.KP + 5) + 2 * np.abs(ref) + lens * np.abs(ref))
    assert (np.abs(got - ref) <= 2 * bound).all(), (K, masks, np.abs(got - ref).max())
    if np.finfo(np.longdouble).nmant >= 63:
        exact = loglik_high_precision(lay, doc_off, word, labs, n_dk, n_kw, n_k, V, alpha, beta)
        err_dev, err_ref = np.abs(got - exact).astype(np.float64), np.abs(ref - exact).astype(np.float64)
        live = lens > 0
        print("loglik K=%d %s: max |dev - exact| / bound = %.4f, max |ref - exact| / bound = %.4f, max |dev - exact| = %.3g"
              % (K, masks, (err_dev[live] / bound[live]).max(), (err_ref[live] / bound[live]).max(), err_dev.max()))
        assert (err_dev <= bound).all(), (K, masks, (err_dev[live] / bound[live]).max())
        assert (err_ref <= bound).all()
