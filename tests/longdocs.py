"""Thesis-shaped corpora for the long-document and full-width-key tests (tests/test_gpu_long_docs_and_keys.py) and the
oracle runs with a deliberately mutilated draw key that show what those tests can tell (tests/test_long_docs_inputs.py).

The thesis trains on full texts: about 5 400 distinct words per document next to abstracts of a few dozen.  ``thesis_corpus``
builds that shape in the form ``doc2bow`` gives it -- word ids unique inside a document, ascending -- with documents of 0, 1, 2,
7, 64 and 300 sites next to documents of thousands and tens of thousands of sites IN CORPUS ORDER, so that with ``sort_docs=False``
long and short documents share a wavefront in every geometry (1, 2, 4, 8 or 16 documents per wavefront), and with token totals
set exactly on the boundaries the kernels switch on (2^15: the int16 changes of the wide kernels; 2^16: the four-wave / quad forms).

Pure numpy: nothing here needs a GPU or the native library.
"""
import numpy as np

LONG = 1000          # a document of at least this many sites counts as long (what_moved)

# (sites, tokens) per document in corpus order; tokens None = frequencies 1 .. 3 at random, "top" = the plan's top_tokens.
# narrow layouts: the document of 60 000 sites carries the 2^16 boundary, 12 345 and 10 000 sites carry the 2^15 one
_NARROW = [(1, None), (60000, "top"), (300, None), (20000, "second"), (5444, None), (7, None), (12345, 32767), (2, None),
           (3000, None), (64, None), (0, None), (10000, 32768), (4097, None), (33, None), (6, None), (1023, None), (300, None),
           (3, None), (2048, None)]
# wide layouts (one document per wavefront, K * sites is what a sweep costs): the long documents take their tokens from 3 000 to
# 5 000 sites
_WIDE = [(1, None), (5000, "top"), (300, None), (3000, "second"), (2, None), (4000, None), (7, None), (0, None), (64, None),
         (3500, None), (1025, None)]
# the draw-key corpus: small, but the Philox block counter (site >> 1) passes 256 in four documents
_KEYS = [(1, None), (700, None), (2, None), (1300, None), (0, None), (64, None), (650, None), (7, None), (300, None),
         (601, None), (5, None)]


def plan(kind, top_tokens):
    """[(sites, tokens or None)] of the documents.  kind 'narrow': top_tokens 65535 (every document below 2^16 tokens: the quad and
    four-wave kernels) or 65536 (then a document of 20 000 sites holds 65 535).  kind 'wide': top_tokens 32767 (every document
    below 2^15) or 32768.  kind 'keys': no boundary."""
    src = {"narrow": _NARROW, "wide": _WIDE, "keys": _KEYS}[kind]
    out = []
    for sites, tokens in src:
        if tokens == "top":
            tokens = top_tokens
        elif tokens == "second":
            # the boundary just below the top one, when the top document sits on the power of two itself
            tokens = top_tokens - 1 if top_tokens in (65536, 32768) else None
        out.append((sites, tokens))
    return out


def _freqs(rng, sites, tokens):
    if tokens is None:
        return rng.integers(1, 4, size=sites).astype(np.int32)
    assert sites >= 1 and tokens >= sites
    f = np.ones(sites, dtype=np.int64)
    f += np.bincount(rng.integers(0, sites, size=tokens - sites), minlength=sites)
    assert int(f.sum()) == tokens
    return f.astype(np.int32)


def label_sets(rng, lens, K, labels):
    """(D, K) uint8.  'dense': every topic everywhere.  'sparse': at most 8 allowed topics per document -- exactly 8 in the long
    ones, so that a site there has somewhere to go; 1 .. 8 in the others.  'heavy': more than a quarter of K but never all
    topics, in every document: label sets the sparse-label kernel does not take (sampler._make_live), so the general kernel runs
    with its masks."""
    D = len(lens)
    if labels == "dense":
        return np.ones((D, K), dtype=np.uint8)
    labs = np.zeros((D, K), dtype=np.uint8)
    for d in range(D):
        if labels == "sparse":
            n = min(K, 8) if lens[d] >= LONG else int(rng.integers(1, min(K, 8) + 1))
        elif labels == "heavy":
            n = int(rng.integers(K // 4 + 2, K))
        else:
            raise ValueError(labels)
        labs[d, rng.choice(K, size=n, replace=False)] = 1
    return labs


def thesis_corpus(K, labels="dense", kind="narrow", top_tokens=65535, seed=0, alpha=0.1, beta=0.01):
    """-> dict(doc_off, word, freq, labs, z, V, lens, tokens, alpha, beta).  V is as small as the unique-word rule allows: the longest document
    plus a margin of a thirtieth, so that the long documents overlap in almost all of their words."""
    rng = np.random.default_rng([seed, K, top_tokens])
    spec = plan(kind, top_tokens)
    lens = np.array([s for s, _ in spec], dtype=np.int64)
    D = len(lens)
    assert D % 32 != 0
    V = int(lens.max() + lens.max() // 30 + 8)
    doc_off = np.zeros(D + 1, dtype=np.int64)
    np.cumsum(lens, out=doc_off[1:])
    word = np.concatenate([np.sort(rng.choice(V, size=int(n), replace=False)) for n in lens]).astype(np.int32)
    freq = np.concatenate([_freqs(rng, int(n), t) for n, t in spec]).astype(np.int32)
    labs = label_sets(rng, lens, K, labels)
    z = np.zeros(int(doc_off[-1]), dtype=np.int64)
    for d in range(D):
        allowed = np.flatnonzero(labs[d])
        z[doc_off[d]:doc_off[d + 1]] = allowed[rng.integers(0, len(allowed), size=int(lens[d]))]
    tokens = np.bincount(np.repeat(np.arange(D), lens), weights=freq, minlength=D).astype(np.int64)
    return dict(doc_off=doc_off, word=word, freq=freq, labs=labs, z=z, V=V, lens=lens, tokens=tokens, alpha=alpha, beta=beta)


def initial_counts(c, K):
    """(n_d_k (D,K), n_k_v (K,V), n_zk (K,)) int64 of the corpus' assignments (LabeledLDA.py:89-92)."""
    D, V = len(c["lens"]), c["V"]
    rows = np.repeat(np.arange(D), c["lens"])
    f = c["freq"].astype(np.int64)
    n_d_k = np.zeros((D, K), dtype=np.int64)
    np.add.at(n_d_k, (rows, c["z"]), f)
    n_k_v = np.zeros((K, V), dtype=np.int64)
    np.add.at(n_k_v, (c["z"], c["word"].astype(np.int64)), f)
    return n_d_k, n_k_v, n_d_k.sum(axis=0)


def share_moved(c, z_before, z_after):
    """share of the sites of the LONG documents whose topic changed"""
    long_site = np.repeat(c["lens"] >= LONG, c["lens"])
    assert long_site.any()
    return float((np.asarray(z_before)[long_site] != np.asarray(z_after)[long_site]).mean())


# ------------------------------------------------------------------------------------------------
# the draw key (seed u64; sweep u32, stream u32, doc u32, site) and its mutilations
# ------------------------------------------------------------------------------------------------
SEEDS = (0x9E3779B97F4A7C15, 2 ** 64 - 1, 2 ** 32)              # (the last: key0 = 0, everything in key1)
# (seed, stream_id, first sweep, doc_base): every value the issue lists appears once; three sweeps each, so the sweep word runs
# 65 535 .. 65 537, 2^31 - 1 .. 2^31 + 1 and 2^32 - 3 .. 2^32 - 1; the document ids cross 2^31 resp. wrap at 2^32 inside the shard
KEYS = ((SEEDS[0], 0xC0DE0123, 65535, 2 ** 31 - 3),
        (SEEDS[1], 0xFFFFFFFF, 2 ** 31 - 1, 2 ** 32 - 4),
        (SEEDS[2], 0xC0DE0123, 2 ** 32 - 3, 2 ** 32 - 4))
KEY_SWEEPS = 3
# the long-document cases run under a wide key too: two sweeps, 2^31 - 1 and 2^31; ids 2^32 - 4 .. 2^32 - 1, 0, 1, ...
LONG_KEY = (SEEDS[0], 0xC0DE0123, 2 ** 31 - 1, 2 ** 32 - 4)
LONG_SWEEPS = 2

MUTILATIONS = ("seed_high_zeroed", "sweep_16_bits", "doc_31_bits", "block_counter_8_bits", "stream_zeroed")


def oracle_sweep_z(co, c, K, counts, seed, sweep, stream, doc_base, mutilation=None, threads=2):
    """z after ONE snapshot sweep of the C oracle from (c['z'], counts) with the draw key as given -- or with the key as a kernel
    with the named defect would build it.  The oracle is used as it is: a document's draws under snapshot semantics depend on the
    sweep-start counts and on itself only, so
      * a wrong seed, sweep or stream word is the same call with that word changed;
      * a document id cut to 31 bits is llda_oracle_sweep_docs with the cut ids;
      * a Philox block counter (site >> 1) cut to 8 bits is the document swept in pieces of 512 sites, each piece a 'document'
        of its own with the sites counted from 0 again, its n_d_k row carried over from the piece before and n_zk moved by what
        the earlier pieces of the SAME document changed (the sweep-start n_k_v plus the site's own removal is what every piece
        reads anyway).  With pieces longer than every document this is the plain sweep -- test_long_docs_inputs.py checks that."""
    n_d_k, n_k_v, n_zk = counts
    D = len(c["lens"])
    ids = (np.arange(D, dtype=np.int64) + int(doc_base)) & 0xFFFFFFFF
    if mutilation == "seed_high_zeroed":
        seed &= 0xFFFFFFFF
    elif mutilation == "sweep_16_bits":
        sweep &= 0xFFFF
    elif mutilation == "stream_zeroed":
        stream = 0
    elif mutilation == "doc_31_bits":
        ids &= 0x7FFFFFFF
    elif mutilation not in (None, "block_counter_8_bits") and not isinstance(mutilation, int):
        raise ValueError(mutilation)
    piece = 512 if mutilation == "block_counter_8_bits" else mutilation if isinstance(mutilation, int) else None
    n_k_v = np.ascontiguousarray(n_k_v, dtype=np.int64)
    n_zk = np.ascontiguousarray(n_zk, dtype=np.int64)
    if piece is None:
        z, _ = co.sweep_docs(ids, c["doc_off"], c["word"], c["freq"], c["z"], c["labs"], n_d_k, n_k_v, n_zk, c["V"], c["alpha"],
                             c["beta"], seed, sweep, stream=stream, threads=threads)
        return z.astype(np.int64)
    z = np.array(c["z"], dtype=np.int64)
    off = c["doc_off"]
    for d in range(D):
        row = np.array(n_d_k[d:d + 1], dtype=np.int64)
        start = row.copy()
        for a in range(int(off[d]), int(off[d + 1]), piece):
            b = min(a + piece, int(off[d + 1]))
            zz, row = co.sweep_docs(ids[d:d + 1], np.array([0, b - a]), c["word"][a:b], c["freq"][a:b], z[a:b], c["labs"][d:d + 1],
                                    row, n_k_v, n_zk + (row - start)[0], c["V"], c["alpha"], c["beta"], seed, sweep,
                                    stream=stream, threads=1)
            z[a:b] = zz
    return z
