"""What the inputs of tests/test_gpu_long_docs_and_keys.py can tell -- no GPU needed.

The GPU cases compare a kernel with the C oracle under full-width draw keys on corpora with long documents.  They can only catch
a kernel that builds the key wrongly if the WRONG key leaves a different state on these very inputs.  So the oracle is run here
with the key as such a kernel would build it (longdocs.oracle_sweep_z): high seed word dropped, sweep cut to 16 bits, document
id cut to 31 bits, Philox block counter cut to 8 bits, stream dropped -- each must leave a different z than the true key.  And
the corpus builder must hit the token totals on which the kernels change form exactly."""
import numpy as np
import pytest

import longdocs as L


def test_plans_mix_lengths_and_hit_the_token_boundaries():
    for kind, tops in (("narrow", (65535, 65536)), ("wide", (32767, 32768))):
        for top in tops:
            c = L.thesis_corpus(128, kind=kind, top_tokens=top)
            lens, tokens = c["lens"], c["tokens"]
            D = len(lens)
            assert D % 32 != 0 and D % 4 != 0
            for n in (0, 1, 2, 7, 64, 300):
                assert n in lens
            assert tokens.max() == top and int((tokens == top).sum()) == 1
            need = {"narrow": {32767: 10000, 32768: 10000, 65535: 20000, 65536: 20000}, "wide": {32767: 3000, 32768: 3000}}[kind]
            for total, sites in need.items():
                if total > top:
                    continue
                hit = np.flatnonzero(tokens == total)
                assert len(hit) >= 1 and lens[hit].min() >= sites, (kind, top, total)
            if kind == "narrow":
                assert 5444 in lens and 12345 in lens and 20000 in lens and lens.max() == 60000 and c["V"] <= 70000
            else:
                assert ((lens >= 3000) & (lens <= 5000)).sum() >= 4 and lens.max() <= 5000 and c["V"] <= 6000
            # doc2bow: word ids unique inside a document, ascending
            for d in range(D):
                w = c["word"][c["doc_off"][d]:c["doc_off"][d + 1]]
                assert (np.diff(w) > 0).all() and (len(w) == 0 or (0 <= w[0] and w[-1] < c["V"]))
            assert c["freq"].min() >= 1
            # long and short documents are neighbours in corpus order: every run of four holds one of each
            for a in range(0, D - 3, 4):
                assert lens[a:a + 4].min() <= 300 and lens[a:a + 4].max() >= L.LONG, a
    # below the top boundary no document reaches it
    assert L.thesis_corpus(128, top_tokens=65535)["tokens"].max() < 65536
    assert L.thesis_corpus(128, kind="wide", top_tokens=32767)["tokens"].max() < 32768
    k = L.thesis_corpus(64, kind="keys")
    assert (k["lens"] >= 600).sum() >= 4 and len(k["lens"]) % 32 != 0     # block counter (site >> 1) beyond 256 in four documents


def test_label_patterns():
    for K in (40, 392, 1031):
        c = L.thesis_corpus(K, labels="sparse", kind="wide", top_tokens=32767)
        n = c["labs"].sum(axis=1)
        assert n.min() >= 1 and n.max() == 8 and (n[c["lens"] >= L.LONG] == 8).all()
        assert (c["labs"][np.repeat(np.arange(len(n)), c["lens"]), c["z"]] == 1).all()        # the start respects the labels
    c = L.thesis_corpus(40, labels="heavy", kind="wide", top_tokens=32767)
    n = c["labs"].sum(axis=1)
    assert (n * 4 > 40).all() and (n < 40).all()
    assert (c["labs"][np.repeat(np.arange(len(n)), c["lens"]), c["z"]] == 1).all()
    assert L.thesis_corpus(40, labels="dense", kind="keys")["labs"].all()


def test_key_settings_cover_the_wide_words():
    seeds = {k[0] for k in L.KEYS}
    assert seeds == {0x9E3779B97F4A7C15, 2 ** 64 - 1, 2 ** 32}
    assert {k[1] for k in L.KEYS} == {0xC0DE0123, 0xFFFFFFFF}
    sweeps = {k[2] + i for k in L.KEYS for i in range(L.KEY_SWEEPS)}
    assert {65535, 65536, 65537, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32 - 1} <= sweeps and max(sweeps) < 2 ** 32
    D = len(L.thesis_corpus(8, kind="keys")["lens"])
    bases = {k[3] for k in L.KEYS}
    assert any(b < 2 ** 31 <= b + D - 1 for b in bases) and any(b < 2 ** 32 <= b + D - 1 for b in bases)


def test_oracle_uniform_takes_every_key_word(c_oracle):
    """the two oracles agree on the widest keys and every word matters (the C side is what the GPU cases compare with)"""
    import llda_oracle as orc
    for seed in L.SEEDS:
        for sweep, stream, doc, site in ((2 ** 32 - 1, 0xFFFFFFFF, 2 ** 32 - 1, 131071), (65536, 0xC0DE0123, 2 ** 31, 513)):
            u = c_oracle.uniform(seed, sweep, stream, doc, site)
            assert u == float(orc.keyed_uniform(seed, sweep, stream, doc, site))
            assert u != c_oracle.uniform(seed & 0xFFFFFFFF, sweep, stream, doc, site) or seed < 2 ** 32
            assert u != c_oracle.uniform(seed, sweep & 0xFFFF, stream, doc, site)
            assert u != c_oracle.uniform(seed, sweep, 0, doc, site)
            assert u != c_oracle.uniform(seed, sweep, stream, doc & 0x7FFFFFFF, site) or doc < 2 ** 31
            assert u != c_oracle.uniform(seed, sweep, stream, doc, site & 0x1FF)
    assert c_oracle.uniform(2 ** 32, 1, 2, 3, 4) != c_oracle.uniform(0, 1, 2, 3, 4)


def _mutilations_change_z(co, c, K, key, sweep_offset):
    seed, stream, sweep0, doc_base = key
    sweep = sweep0 + sweep_offset
    counts = L.initial_counts(c, K)
    true = L.oracle_sweep_z(co, c, K, counts, seed, sweep, stream, doc_base)
    # the selection form of the oracle used for the mutilations is the plain sweep ...
    cs = co.CState(c["doc_off"], c["word"], c["freq"], c["z"], c["labs"], *counts, c["V"], c["alpha"], c["beta"])
    cs.sweep(1, seed, sweep, stream=stream, doc_base=doc_base, threads=2)
    np.testing.assert_array_equal(cs.z, true)
    # ... and so is the sweep in pieces when no document is cut
    np.testing.assert_array_equal(L.oracle_sweep_z(co, c, K, counts, seed, sweep, stream, doc_base, mutilation=1 << 30), true)
    long_site = np.repeat(c["lens"] > 512, c["lens"])
    first = np.concatenate([np.arange(n) for n in c["lens"]]) < 512
    for m in L.MUTILATIONS:
        z = L.oracle_sweep_z(co, c, K, counts, seed, sweep, stream, doc_base, mutilation=m)
        differ = z != true
        assert differ.any(), m
        if m == "block_counter_8_bits":
            # sites 0 .. 511 of a document draw what they drew; from site 512 on a long document goes wrong
            assert not differ[first].any() and differ[long_site & ~first].mean() > 0.1
        elif m == "doc_31_bits":
            # documents with an id below 2^31 draw what they drew
            low = np.repeat(((np.arange(len(c["lens"])) + doc_base) & 0xFFFFFFFF) < 2 ** 31, c["lens"])
            assert not differ[low].any() and differ[~low].any()
        else:
            assert differ[long_site].mean() > 0.1, m


@pytest.mark.parametrize("key", range(len(L.KEYS)))
def test_a_mutilated_key_changes_the_small_corpus(c_oracle, key):
    """part 3's corpus under each of its key settings, at the second of the three sweeps (the first of 65 535 .. 65 537 has
    no bit above 16 to lose)"""
    K = 40
    c = L.thesis_corpus(K, labels="dense", kind="keys")
    _mutilations_change_z(c_oracle, c, K, L.KEYS[key], 1)


@pytest.mark.parametrize("K,labels,kind,top", [(128, "dense", "narrow", 65535), (40, "heavy", "narrow", 65536),
                                               (392, "sparse", "narrow", 65535), (1031, "sparse", "wide", 32767)])
def test_a_mutilated_key_changes_the_long_document_corpora(c_oracle, K, labels, kind, top):
    """part 2's corpora under part 2's key, both of its sweeps"""
    c = L.thesis_corpus(K, labels=labels, kind=kind, top_tokens=top)
    for i in range(L.LONG_SWEEPS):
        _mutilations_change_z(c_oracle, c, K, L.LONG_KEY, i)
