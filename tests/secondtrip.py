"""Inputs for the tests of the SECOND document a workgroup takes (tests/test_second_trip_host.py, tests/test_gpu_second_trip.py).

Several kernels cap their grid and let a workgroup take its documents in turn (``for (d = blockIdx.x; d < D; d += gridDim.x)``); what
the workgroup keeps in LDS, in registers or in its scratch row has to be rebuilt for every document.  The builders below make corpora
with a few documents MORE than one trip of the grid holds, so that the documents d and d + cap meet in one workgroup, and lay the two
out so that whatever the first leaves behind would change the second: other label masks, other lengths (none against some, short
against long, both ways round), tokens of the second on a topic both allow.

Host only: numpy and the layout of K, no torch.  Everything is a function of its arguments (fixed seeds); the cached builders hand
out the same arrays to every caller, which must leave them unchanged."""
import functools

import numpy as np

import readoutref

WIDE_CAP = readoutref.WIDE_GRID                  # workgroups of a wide sweep / fold-in at most (csrc/sweep_plan.hpp wide_blocks)
SETS_CAP_DOCS = 1024 * 4                         # llda_label_sets: SETS_MAX_BLOCKS workgroups of SETS_WAVES documents a trip
ATTR_LDS_CAP = 65536                             # llda_attr_lds_kernel: ATTR_LDS_MAX_BLOCKS workgroups of one document

N_PAIRS = 9                                      # documents of the second trip in the wide cases
D_WIDE = WIDE_CAP + N_PAIRS
SWEEP_V = 64
SWEEP_KS = (1100, 2047)
HEAVY_DOC, HEAVY_FREQ = 3, 40000                 # sweep_corpus(heavy=True): the site that takes its document beyond 2^15 tokens
# sites of the documents 0 .. 8 and of their partners WIDE_CAP .. WIDE_CAP + 8
HEAD_LENS = (0, 2, 1, 3, 3, 0, 2, 1, 2)
TAIL_LENS = (2, 0, 3, 1, 2, 3, 0, 3, 1)
PAIR_KINDS = ("empty_then_some", "some_then_empty", "shorter_then_longer", "longer_then_shorter")
# K -> (KP, T, tiers) of lda_thesis_amd.layout.group_layout
WIDE_GEOMETRY = {1100: (1536, 12, 2), 2047: (3072, 16, 3), 969: (2048, 16, 2)}
TINY_PRIOR = 1e-9                                # below the tiered kernels' domain: every site through the exact pipeline
# the wide sweeps: name -> (K, debug_margin, tiny priors, heavy, what csrc/sweep_plan.hpp makes of it).  The plan fields are checked on
# the host (tests/test_second_trip_host.py); the device test can only see what SELECTS the form.
SWEEP_CASES = {
    "k1100_f32_fat": (1100, 0, False, False, dict(family="wide_f32", slim=0, compact=1)),
    "k1100_f32_slim_forced": (1100, -7, False, False, dict(family="wide_f32", slim=1, compact=1)),
    "k1100_reg_compact": (1100, -5, False, False, dict(family="wide_reg", compact=1)),
    "k1100_reg_lds_copies": (1100, -4, False, False, dict(family="wide_reg", compact=0)),
    "k1100_lds_only_tiered": (1100, -3, False, False, dict(family="wide_lds", tiered=1)),
    "k1100_f32_fat_all_rare": (1100, -1, False, False, dict(family="wide_f32", slim=0, compact=1)),
    "k1100_lds_only_all_exact": (1100, 0, True, False, dict(family="wide_lds", tiered=0)),
    "k1100_reg_heavy_document": (1100, 0, False, True, dict(family="wide_reg", compact=0)),
    "k2047_f32_slim": (2047, 0, False, False, dict(family="wide_f32", slim=1, compact=1)),
    "k2047_f32_fat_forced": (2047, -6, False, False, dict(family="wide_f32", slim=0, compact=1)),
    "k2047_f32_slim_all_rare": (2047, -1, False, False, dict(family="wide_f32", slim=1, compact=1)),
}


def layout(K):
    return readoutref.layout(K)


def sweep_priors(tiny):
    """(alpha, beta) of a wide sweep case"""
    return (TINY_PRIOR, TINY_PRIOR) if tiny else (0.1, 0.01)


def wide_lengths(D=D_WIDE):
    """0 .. 3 sites per document; the documents of the first nine pairs (d, d + WIDE_CAP) by hand"""
    lens = np.random.default_rng(21).integers(0, 4, D)
    lens[:N_PAIRS] = HEAD_LENS
    lens[WIDE_CAP:WIDE_CAP + N_PAIRS] = TAIL_LENS
    return lens.astype(np.int64)


def pair_kind(a, b):
    """what a workgroup meets going from a document of a sites to one of b sites; None: nothing this file plants"""
    if a == 0 and b > 0:
        return "empty_then_some"
    if a > 0 and b == 0:
        return "some_then_empty"
    if 0 < a < b:
        return "shorter_then_longer"
    if a > b > 0:
        return "longer_then_shorter"
    return None


def trip_pairs(D, cap, order=None):
    """(first, second) documents that one workgroup of a launch of ``cap`` workgroups takes one after the other: the documents at the
    places i and i + cap of the processing order (``order`` None: the documents' own order)"""
    order = np.arange(D) if order is None else np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(D))
    return [(int(order[i]), int(order[i + cap])) for i in range(D - cap)]


def assert_pairs_differ(pairs, doc_off, labs, z, freq, heavy=False):
    """the properties sweep_corpus promises, on the pairs a launch really makes: every kind of length change; the two documents of a
    pair share at least two allowed topics and differ in at least two; a second document with sites has tokens on a shared topic"""
    lens = np.diff(doc_off)
    kinds = set(pair_kind(int(lens[a]), int(lens[b])) for a, b in pairs)
    assert kinds >= set(PAIR_KINDS), kinds
    for a, b in pairs:
        both = (labs[a] != 0) & (labs[b] != 0)
        assert int(both.sum()) >= 2 and int((labs[a] != labs[b]).sum()) >= 2, (a, b)
        if lens[b]:
            zb = z[doc_off[b]:doc_off[b + 1]]
            assert both[zb].any(), (a, b)
    for d in range(len(lens)):                                    # (every assignment is allowed)
        assert labs[d][z[doc_off[d]:doc_off[d + 1]]].all(), d
    tokens = np.add.reduceat(np.append(freq, 0).astype(np.int64), doc_off[:-1]) * (lens > 0)
    assert (int(tokens.max()) >= 32768) == bool(heavy)


def shared_label(d, K):
    """the label (never the root) the documents d and d + WIDE_CAP both carry"""
    return 1 + ((d % WIDE_CAP) * 37) % (K - 1)


@functools.lru_cache(maxsize=None)
def sweep_corpus(K, heavy=False):
    """doc_off, word, freq, labs (D, K) uint8, z (topic ids) of D = WIDE_CAP + 9 documents over SWEEP_V words.

    Labels: the root, shared_label(d) and up to four more -- of ODD topic ids for the documents of the first trip, of EVEN ones for the
    second, so the masks of a pair share two topics and differ in about eight.  The first site of every document sits on the shared
    label, the others on any allowed topic.  heavy: the first site of HEAVY_DOC (first trip, on the shared label) has frequency
    HEAVY_FREQ; its partner holds a handful of tokens there."""
    D = D_WIDE
    rng = np.random.default_rng([22, K])
    lens = wide_lengths(D)
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    word = np.concatenate([np.sort(rng.choice(SWEEP_V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = rng.integers(1, 4, S).astype(np.int32)
    labs = np.zeros((D, K), dtype=np.uint8)
    z = np.zeros(S, dtype=np.int64)
    for d in range(D):
        second = d >= WIDE_CAP
        own = 2 * rng.choice((K - 2) // 2, size=4, replace=False) + (2 if second else 1)
        sh = shared_label(d, K)
        labs[d, 0] = labs[d, sh] = 1
        labs[d, own] = 1
        n = int(lens[d])
        if n:
            allowed = np.flatnonzero(labs[d])
            z[doc_off[d]:doc_off[d + 1]] = rng.choice(allowed, size=n)
            z[doc_off[d]] = sh
    if heavy:
        assert lens[HEAVY_DOC] > 1 and lens[HEAVY_DOC + WIDE_CAP] > 0
        freq[doc_off[HEAVY_DOC]] = HEAVY_FREQ
    return doc_off, word, freq, labs, z


def counts(doc_off, word, freq, z, K, V):
    """n_d_k (D, K), n_k_v (K, V), n_zk (K,) int64 of the assignments z"""
    D = len(doc_off) - 1
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    n_d_k = np.zeros((D, K), dtype=np.int64)
    n_k_v = np.zeros((K, V), dtype=np.int64)
    np.add.at(n_d_k, (doc, z), freq)
    np.add.at(n_k_v, (z, word), freq)
    return n_d_k, n_k_v, n_d_k.sum(axis=0)


# ------------------------------------------------------------------------------------------------
# wide fold-in: K = 969, documents AND sites beyond one trip
# ------------------------------------------------------------------------------------------------
FOLDIN_K = 969                                   # the first wide layout (KP = 2048)
FOLDIN_V = 60                                    # tests/test_gpu_foldin_direct.py V: word V - 1 loads on no topic
FOLDIN_ROWS = 12                                 # rows of its make_init_rows
FOLDIN_ROTATE = N_PAIRS
# the documents the numpy reference runs on: both documents of every pair and every 40th of the rest
FOLDIN_SUBSET = tuple(range(N_PAIRS)) + tuple(range(N_PAIRS, WIDE_CAP, 40)) + tuple(range(WIDE_CAP, D_WIDE))


@functools.lru_cache(maxsize=None)
def foldin_corpus(zero_word):
    """dict(doc_off, word, freq, init_idx) of D = WIDE_CAP + 9 documents of wide_lengths(): more than WIDE_CAP sites too, and the sites s
    and s + WIDE_CAP -- one workgroup of the launch that draws the initial assignments -- lie in different documents and start from
    different rows.  zero_word: some sites hold the word no topic loads on (for the settings with the fall-back only)."""
    lens = wide_lengths()
    rng = np.random.default_rng([23, int(zero_word)])
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    S = int(doc_off[-1])
    word = rng.integers(0, FOLDIN_V - 1, S).astype(np.int32)
    if zero_word:
        word[rng.random(S) < 0.02] = FOLDIN_V - 1
        word[[doc_off[1], doc_off[WIDE_CAP + 1] - 1, S - 1]] = FOLDIN_V - 1     # in both trips
    freq = rng.integers(1, 5, S).astype(np.int32)
    init_idx = rng.integers(0, FOLDIN_ROWS, S).astype(np.int32)
    for s in range(WIDE_CAP, S):
        if init_idx[s] == init_idx[s - WIDE_CAP]:
            init_idx[s] = (init_idx[s] + 1) % FOLDIN_ROWS
    return dict(doc_off=doc_off, word=word, freq=freq, init_idx=init_idx)


def assert_foldin_sites_differ(c):
    doc_off, S = c["doc_off"], len(c["word"])
    assert S > WIDE_CAP + 1000 and len(doc_off) - 1 == D_WIDE
    doc = np.repeat(np.arange(len(doc_off) - 1), np.diff(doc_off))
    s = np.arange(S - WIDE_CAP)
    assert (doc[s] != doc[s + WIDE_CAP]).all() and (c["init_idx"][s] != c["init_idx"][s + WIDE_CAP]).all()
    lens = np.diff(doc_off)
    assert set(pair_kind(int(lens[a]), int(lens[b])) for a, b in trip_pairs(D_WIDE, WIDE_CAP)) >= set(PAIR_KINDS)


def take_documents(c, ids, **keys):
    """the CSR arrays of ``c`` for the documents ``ids`` in that order (a copy of c with doc_off / word / freq / init_idx replaced), plus
    ``sites``: where every site of the selection sits in c.  ``keys`` are set on the copy."""
    ids = np.asarray(ids, dtype=np.int64)
    off = c["doc_off"]
    n = np.diff(off)[ids]
    sites = np.concatenate([np.arange(off[d], off[d + 1]) for d in ids] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    out = dict(c)
    out.update(doc_off=np.concatenate(([0], np.cumsum(n))).astype(np.int64), word=c["word"][sites], freq=c["freq"][sites],
               init_idx=c["init_idx"][sites], sites=sites)
    out.update(keys)
    return out


# ------------------------------------------------------------------------------------------------
# llda_label_sets: D = SETS_CAP_DOCS + 5
# ------------------------------------------------------------------------------------------------
SETS_KS = (33, 130)
SETS_D = SETS_CAP_DOCS + 5
SETS_FIRST = 1
SETS_PLANTS = ("nan_then_ordinary", "filled_then_reaching", "reaching_then_filled", "other_mask_words")


@functools.lru_cache(maxsize=None)
def sets_case(K):
    """score (D, K + 3), thr, truth of tests/test_gpu_label_sets.make with D = SETS_CAP_DOCS + 5 and first = 1, and on top of them in
    the pairs (d, d + SETS_CAP_DOCS), d = 0 .. 3, which one wavefront takes one after the other:
      0  a NaN in an eligible column (its mask is cleared, n_pred = -1), then an ordinary document
      1  a document that reaches no threshold (at_least_one sets the bit of its best label), then one that reaches two
      2  the same the other way round
      3  predictions in the LAST mask word only, then in the FIRST only
    The thresholds of the columns 1, 2 and K - 1 are made finite for that (make's -inf in the last column would leave no set empty)."""
    from test_gpu_label_sets import make
    D, first = SETS_D, SETS_FIRST
    score, thr, truth = make(np.random.default_rng([24, K]), D, K, first, K + 3)
    thr[1], thr[2], thr[K - 1] = 0.25, 0.375, 0.5
    C = SETS_CAP_DOCS

    def row(d, **cols):
        score[d, first:K] = -1.0
        for k, v in cols.items():
            score[d, int(k[1:])] = v
    score[0, K - 1] = np.nan
    row(C + 0, k1=1.0, k2=0.375)
    row(1, k2=-0.5)                                               # best label: 2
    row(C + 1, k1=0.25, k2=7.0)
    row(2, k1=0.25, k2=7.0)
    row(C + 2, k1=-0.5)                                           # best label: 1
    row(3, **{"k%d" % (K - 1): 0.5})
    row(C + 3, k1=1.0, k2=1.0)
    return score, thr, truth


def assert_sets_plants(K, want0, want1):
    """what the planted pairs do under labelref (want0 / want1: at_least_one off / on)"""
    C, last = SETS_CAP_DOCS, (K - 1) // 32
    for want, alo in ((want0, 0), (want1, 1)):
        n, m = want["n_pred"], want["mask"]
        assert n[0] == -1 and not m[0].any() and n[C] == 2
        assert n[1] == alo and n[C + 1] == 2 and n[2] == 2 and n[C + 2] == alo
        if alo:
            assert np.flatnonzero(m[1]).tolist() == [2] and np.flatnonzero(m[C + 2]).tolist() == [1]
        words_a, words_b = set(np.flatnonzero(m[3]) // 32), set(np.flatnonzero(m[C + 3]) // 32)
        assert words_a == {last} and words_b == {0} and last > 0


# ------------------------------------------------------------------------------------------------
# llda_attr_lds_kernel: K = 1025, D = ATTR_LDS_CAP + 6
# ------------------------------------------------------------------------------------------------
ATTR_K = 1025                                    # the first K of the LDS form (llda_gibbs.hip doc_geom)
ATTR_D = ATTR_LDS_CAP + 6
ATTR_LIVE = tuple(range(6)) + tuple(range(ATTR_LDS_CAP, ATTR_LDS_CAP + 6))      # the only documents with sites
ATTR_LENS = (1, 5, 2, 66, 3, 7) + (4, 2, 65, 1, 9, 3)
ATTR_SETTINGS = dict(iters=2, alpha=0.1, top_m=4)


@functools.lru_cache(maxsize=None)
def attr_case():
    """dict(theta (12, K) the loads of ATTR_LIVE, phi_t (V, K), doc_off [ATTR_D + 1], sub_off [13], word, freq, V): every other
    document is empty, and its loads are the test's to make (on the device).  Model and vocabulary of tests/test_gpu_attribute.py:
    few loads per row, exact zeros elsewhere, the columns 0 and K - 1 loaded (and tied) in every row."""
    import test_gpu_attribute as ta
    K = ATTR_K
    rng = np.random.default_rng([25, K])
    theta, phi_t = ta.model(rng, K, len(ATTR_LIVE), 0, 0)
    sub_off = np.concatenate(([0], np.cumsum(ATTR_LENS))).astype(np.int64)
    S = int(sub_off[-1])
    word = rng.integers(0, ta.V, S).astype(np.int32)              # the planted rows of phi_t among them
    word[sub_off[:-1]] = 5 + np.arange(len(ATTR_LIVE))            # every document has a site that counts
    word[[2, S - 1]] = [ta.V, -1]                                 # outside the vocabulary
    freq = rng.integers(1, 10, S).astype(np.int32)
    lens = np.zeros(ATTR_D, dtype=np.int64)
    lens[list(ATTR_LIVE)] = ATTR_LENS
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    return dict(theta=theta, phi_t=phi_t, doc_off=doc_off, sub_off=sub_off, word=word, freq=freq, V=ta.V)


def assert_attr_pairs_differ(c):
    theta, lens = c["theta"], np.diff(c["sub_off"])
    assert (np.diff(c["doc_off"])[list(ATTR_LIVE)] == lens).all() and int(c["doc_off"][-1]) == int(lens.sum())
    for i in range(6):
        a, b = theta[i] > 0, theta[i + 6] > 0
        assert lens[i] != lens[i + 6] and lens[i] > 0 and lens[i + 6] > 0
        assert (a & b).any() and int((a != b).sum()) >= 2, i
    assert set(pair_kind(int(lens[i]), int(lens[i + 6])) for i in range(6)) == {"shorter_then_longer", "longer_then_shorter"}
