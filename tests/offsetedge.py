"""Inputs for the tests of llda_sweep at the top of its 32-bit offsets (tests/test_offset_edge_host.py, tests/test_gpu_offset_edges.py).

The sweep kernels form no 64-bit address in their site loops: a uniform base plus a 32-bit byte offset (csrc/device_common.hpp,
gload_i32 / gstore_i32).  Four bounds keep those offsets inside 32 bits:

  4 bytes per site    word, freq, z, csc_pos, site_row at (site - doc_off[0]) * 4      a call spans fewer than 2^30 sites
  16 bytes per site   site_rec of the layouts with 8 or 16 lanes per document           ... fewer than 2^28 sites
  the commit log      log position << 2 in the kernels of four and more documents       fewer than 2^30 sites in the SHARD
  the 16-bit image    word << 10 at K = 512 (2 KP bytes per row)                       V < 2^22

An offset that is sign-extended, or that loses its top bit, shows from the HALF of each range on.  The sizes below are the smallest at
which each offset passes 2^31 (``*_HALF``) and the largest the host accepts (``*_TOP``), plus a shard of two calls under the real limit.

Host part: numpy only, every function a function of its arguments.  ``generate`` / ``sparse_labels`` / ``vocab_counts`` make device
tensors (torch is imported inside them): nothing of these sizes is built on, or uploaded from, the host."""
import collections

import numpy as np

N = 1024                                  # sites per document: below 2^16 tokens (quad kernels) and 2^15 (compact wide form)
HEAD = 512                                # ... but document 0 holds the second half of one only, so that the site whose offset is
#                                           2^31 (a multiple of N sites into the call) lies INSIDE a document, not at its start
GROUP = 150                               # documents per sample group
ORACLE_THREADS = 16
SEED = 1234                               # of the corpus (bench.py's)
GEN_BLOCK = 32768                         # documents per block of corpus.synthetic_corpus_blocks here

S_HALF = 2 ** 29 + 1000 * N               # the 4-byte offsets pass 2^31 in document 2^19
S_TOP = 2 ** 30 - 1                       # sampler_plan.MAX_CALL_SITES: the largest single call
S_TWO = 2 ** 30 + 8 * N                   # two calls under the real limit
R_HALF = 2 ** 27 + 1000 * N               # the 16-byte records pass 2^31 in document 2^17
R_TOP = 2 ** 28 - 1                       # sampler_plan.MAX_CALL_SITES_REC
V_HALF = 2 ** 21 + 1024                   # K = 512: a row of the 16-bit image is 1024 bytes, row 2^21 starts at byte 2^31
V_TOP = 2 ** 22 - 1
# the run whose offsets stay small: a call of at most 2^26 sites keeps every 4-byte array below 2^28 bytes; where the kernels read
# 16-byte records, 2^24 sites do the same for the records (and cut the R_* corpora into more than seven calls as well)
SPLIT_LIMIT, SPLIT_LIMIT_REC = 1 << 26, 1 << 24

Case = collections.namedtuple("Case", "S K V sparse kw unit form calls")
# unit: bytes per site of the widest site-indexed array the kernel of the case reads (what decides where "around" is)
# form: what the sampler's attributes must show (tests/test_gpu_offset_edges.assert_form); calls: llda_sweep calls under the real limits
CASES = collections.OrderedDict([
    # K = 512, V = 100 000, every label in every document
    ("quad512_half", Case(S_HALF, 512, 100_000, False, {}, 4, "quad", 1)),
    ("twodoc16_half", Case(S_HALF, 512, 100_000, False, dict(quad=False), 4, "two_doc16", 1)),
    ("int32_half", Case(S_HALF, 512, 100_000, False, dict(rows16=False), 4, "int32_logged", 1)),
    ("atomics_half", Case(S_HALF, 512, 100_000, False, dict(rows16=False, commit_log=False), 4, "int32_atomics", 1)),
    ("quad512_top", Case(S_TOP, 512, 100_000, False, {}, 4, "quad", 1)),
    # 2^30 sites and more in the shard: log positions no longer fit the quad kernels' position << 2, so sampler_plan.rows hands the shard
    # to the two-document kernel (its log index is a plain 32-bit element index); the second call starts at doc_off[0] near 2^30
    ("two_calls", Case(S_TWO, 512, 100_000, False, {}, 4, "two_doc16", 2)),
    # the same words with root + 7 labels per document
    ("sparse512_half", Case(S_HALF, 512, 100_000, True, dict(image=8), 4, "sparse8", 1)),
    # K = 100: KP = 128, four padded positions.  8 lanes per document: with the commit log the kernels read site records, so a call
    # holds 2^28 - 1 sites and the defaults make three calls of S_HALF, each with its records past 2^31 (quad kernel, PAD); the general
    # kernel with padded positions meets 4-byte offsets past 2^31 only without the log
    ("tail_half", Case(S_HALF, 100, 50_000, False, {}, 16, "quad_rec", 3)),
    ("tail_atomics_half", Case(S_HALF, 100, 50_000, False, dict(commit_log=False), 4, "int32_atomics", 1)),
    # K = 128 / 256: 16-byte site records
    ("quad128_rec_half", Case(R_HALF, 128, 50_000, False, {}, 16, "quad_rec", 1)),
    ("rec128_half", Case(R_HALF, 128, 50_000, False, dict(quad=False), 16, "int32_rec", 1)),
    ("quad128_rec_top", Case(R_TOP, 128, 50_000, False, {}, 16, "quad_rec", 1)),
    ("quad256_rec_half", Case(R_HALF, 256, 50_000, False, {}, 16, "quad_rec", 1)),
    # K = 2048: one wavefront per document
    ("wide2048_half", Case(S_HALF, 2048, 20_000, False, {}, 4, "wide_f32", 1)),
])
# the layouts (lda_thesis_amd.layout.GroupLayout) the cases rely on: K -> (KP, lanes per document, padded positions)
GEOMETRY = {512: (512, 32, 0), 100: (128, 8, 4), 128: (128, 8, 0), 256: (256, 16, 0), 2048: (2048, 128, 0)}

# peak of torch.cuda.max_memory_allocated() per case as measured on the MI355X (bytes) -- a case skips only
# where less than 1.25 x this is free
GB = 10 ** 9
PEAK_BYTES = {"quad512_half": 56.1 * GB, "twodoc16_half": 58.3 * GB, "int32_half": 56.0 * GB, "atomics_half": 32.3 * GB,
              "quad512_top": 93.7 * GB, "two_calls": 98.0 * GB, "sparse512_half": 60.4 * GB, "tail_half": 54.8 * GB,
              "tail_atomics_half": 22.5 * GB, "quad128_rec_half": 16.5 * GB, "rec128_half": 16.5 * GB, "quad128_rec_top": 27.7 * GB,
              "quad256_rec_half": 14.5 * GB, "wide2048_half": 50.8 * GB, "V_half": 19.5 * GB, "V_top": 38.8 * GB}


def corpus_key(case):
    """cases with the same key share the words (and, dense, the initial topics): the cached corpus is generated once for the largest
    S of the key and the others take a prefix of it (synthetic_corpus_blocks seeds block by block)"""
    return (case.K, case.V)


def key_sites(key):
    return max(c.S for c in CASES.values() if corpus_key(c) == key)


def n_docs(S):
    return 1 + -(-(S - HEAD) // N)


def doc_offsets(S):
    """document 0 has HEAD sites, every other N, the last what is left of S"""
    off = np.minimum(HEAD + N * np.arange(n_docs(S), dtype=np.int64), S)
    return np.concatenate(([0], off)).astype(np.int64)


def call_ranges(doc_off, limit):
    """GibbsSampler._make_calls for one range of documents: [(lo, hi)] with doc_off[hi] - doc_off[lo] <= limit"""
    D, S = len(doc_off) - 1, int(doc_off[-1])
    if S <= limit:
        return [(0, D)]
    calls, lo = [], 0
    while lo < D:
        hi = int(np.searchsorted(doc_off, doc_off[lo] + limit, side="right")) - 1
        hi = max(min(hi, D), lo + 1)
        calls.append((lo, hi))
        lo = hi
    return calls


def call_limit(case, split=False):
    """sites one llda_sweep call of the case may span (sampler_plan.commit_log's call_limit), real or of the split run"""
    from lda_thesis_amd import sampler_plan as P
    G = GEOMETRY[case.K][1]
    big, rec = (SPLIT_LIMIT, SPLIT_LIMIT_REC) if split else (P.MAX_CALL_SITES, P.MAX_CALL_SITES_REC)
    return P.commit_log(case.kw.get("commit_log"), case.S, G, big, rec).call_limit


def crossing(doc_off, lo, hi, unit):
    """(site, document) of the call [lo, hi) whose offset from the call's first site is 2^31 bytes at ``unit`` bytes per site, or None
    when the call ends before it"""
    site = int(doc_off[lo]) + (1 << 31) // unit
    if site >= int(doc_off[hi]):
        return None
    return site, int(np.searchsorted(doc_off, site, side="right")) - 1


def sample_groups(doc_off, calls, unit, rng):
    """the documents that go through the oracle: name -> sorted ids.  Per call its first GROUP, its last GROUP and the GROUP around the
    crossing document; GROUP random ones of the shard -- and another GROUP for every call that has no crossing."""
    D = len(doc_off) - 1
    first, last, around, n_random = [], [], [], GROUP
    for lo, hi in calls:
        first.append(np.arange(lo, min(lo + GROUP, hi)))
        last.append(np.arange(max(hi - GROUP, lo), hi))
        c = crossing(doc_off, lo, hi, unit)
        if c is None:
            n_random += GROUP
        else:
            a = min(max(c[1] - GROUP // 2, lo), max(hi - GROUP, lo))
            around.append(np.arange(a, min(a + GROUP, hi)))
    g = collections.OrderedDict()
    g["first"], g["last"] = np.unique(np.concatenate(first)), np.unique(np.concatenate(last))
    if around:
        g["around"] = np.unique(np.concatenate(around))
    g["random"] = np.sort(rng.choice(D, size=min(n_random, D), replace=False))
    return g


# ------------------------------------------------------------------------------------------------
# device side
# ------------------------------------------------------------------------------------------------
def generate(K, V, S, device="cuda"):
    """(word int32 [S], freq, z int64 topic ids) for doc_offsets(S): the documents of corpus.synthetic_corpus_blocks(0, ...) with N sites
    each, less the first N - HEAD sites of document 0 -- every document keeps distinct ascending words"""
    from lda_thesis_amd.corpus import synthetic_corpus_blocks
    D_gen = -(-n_docs(S) // GEN_BLOCK) * GEN_BLOCK
    _, word, freq, z = synthetic_corpus_blocks(0, D_gen, N, V, K, SEED, device, block=GEN_BLOCK)
    skip = N - HEAD
    return word[skip:skip + S], freq[skip:skip + S], z[skip:skip + S]


def sparse_labels(S, K, device="cuda"):
    """root + 7 random labels per document and initial topics among them, drawn as tests/test_gpu_fullsize.sparse_corpus draws them:
    (lab int64 (D, 8) ascending, z int64 [S])"""
    import torch
    D = n_docs(S)
    gen = torch.Generator(device=device)
    gen.manual_seed(99)
    lab = torch.sort(torch.randint(1, K - 8, (D, 7), device=device, generator=gen), dim=1).values + torch.arange(7, device=device)
    lab = torch.cat([torch.zeros((D, 1), dtype=lab.dtype, device=device), lab], dim=1)
    pick = torch.randint(0, 8, (D, N), device=device, generator=gen)
    z = torch.gather(lab, 1, pick).reshape(-1)
    skip = N - HEAD
    return lab, z[skip:skip + S].contiguous()


# ------------------------------------------------------------------------------------------------
# the vocabulary edge of the quad kernel's 16-bit image
# ------------------------------------------------------------------------------------------------
VOCAB_K, VOCAB_DOCS, VOCAB_TOKENS, BAND = 512, 3000, 300, 1000
VOCAB_CASES = collections.OrderedDict([("V_half", V_HALF), ("V_top", V_TOP)])
WIDE_COUNT, HIGH_COUNT = 70_000, 40_000   # planted counts: beyond 16 bits (the row is read as int32) / with bit 15 set (it fits)


def bands(V):
    """first ids of the three bands of BAND words: the first rows, the rows around 2^21 (byte 2^31 of the image: centred on it, or
    as far down as keeps it clear of the third band -- V_HALF ends 1024 rows past 2^21), the last rows"""
    return (0, min(2 ** 21 - BAND // 2, V - 2 * BAND), V - BAND)


def vocab_ids(V):
    return np.concatenate([np.arange(b, b + BAND) for b in bands(V)]).astype(np.int64)


def vocab_corpus(V):
    """doc_off, word, freq, z of VOCAB_DOCS documents of VOCAB_TOKENS sites: a third from every band, ascending and distinct"""
    rng = np.random.default_rng([26, V])
    per = VOCAB_TOKENS // 3
    cols = [np.sort(np.argsort(rng.random((VOCAB_DOCS, BAND)), axis=1)[:, :per], axis=1) + b for b in bands(V)]
    word = np.concatenate(cols, axis=1).reshape(-1).astype(np.int32)
    doc_off = (VOCAB_TOKENS * np.arange(VOCAB_DOCS + 1)).astype(np.int64)
    freq = rng.integers(1, 4, word.size).astype(np.int32)
    z = rng.integers(0, VOCAB_K, word.size).astype(np.int64)
    return doc_off, word, freq, z


def vocab_planted(V):
    """(rows, topics, counts): counts that belong to no site (as SubLDA's phantom columns), on top of the corpus' own: of every three
    consecutive used words the first gets WIDE_COUNT on four topics, the second HIGH_COUNT on two, the third nothing"""
    ids = vocab_ids(V)
    rows, topics, counts = [], [], []
    for j, v in enumerate(ids):
        if j % 3 == 0:
            for i in range(4):
                rows.append(v), topics.append((7 * j + 131 * i) % VOCAB_K), counts.append(WIDE_COUNT)
        elif j % 3 == 1:
            for i in range(2):
                rows.append(v), topics.append((11 * j + 257 * i) % VOCAB_K), counts.append(HIGH_COUNT)
    return np.array(rows, dtype=np.int64), np.array(topics, dtype=np.int64), np.array(counts, dtype=np.int64)


def vocab_counts(V, doc_off, word, freq, z, device="cuda"):
    """counts= of the vocabulary case: n_d_k (D, K) on the host, n_k_v (K, V) int32 and n_zk ON THE DEVICE (8.6 GB at V_TOP)"""
    import torch
    K, D = VOCAB_K, len(doc_off) - 1
    doc = np.repeat(np.arange(D), np.diff(doc_off))
    n_d_k = np.zeros((D, K), dtype=np.int64)
    np.add.at(n_d_k, (doc, z), freq)
    n_k_v = torch.zeros((K, V), dtype=torch.int32, device=device)
    rows, topics, counts = vocab_planted(V)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=t)
    n_k_v.index_put_((dev(z, torch.int64), dev(word, torch.int64)), dev(freq, torch.int32), accumulate=True)
    n_k_v.index_put_((dev(topics, torch.int64), dev(rows, torch.int64)), dev(counts, torch.int32), accumulate=True)
    n_zk = n_k_v.sum(dim=1, dtype=torch.int64)
    assert int(n_zk.max()) < 2 ** 31
    return dict(n_d_k=n_d_k, n_k_v=n_k_v, n_zk=n_zk)


def remap(ids, word):
    """order-preserving new ids 0 .. len(ids) - 1 of the words (all of which are in the sorted ``ids``)"""
    new = np.searchsorted(ids, word)
    assert (ids[new] == word).all()
    return new.astype(np.int32)
