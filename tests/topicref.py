"""numpy restatement of ``llda_top_words`` and ``llda_word_cooc`` (include/llda_gibbs.h) and the inputs their tests share
(tests/test_topics_host.py, tests/test_gpu_top_words.py, tests/test_gpu_word_cooc.py, tests/test_gpu_topics_dropin.py).

Pure numpy: nothing here needs a GPU; only ``device_rows`` asks the native library for the (host-only) layout of K.
"""
import math

import numpy as np

INT32_MAX = 2 ** 31 - 1


def top_words_ref(n_k_v, n):
    """(top_idx, top_cnt), both (K, n) int32: for every row of the (K, V) integer matrix the n columns with the largest entries,
    ties by column ascending -- one lexsort per topic; entries i >= min(n, V) are -1 / 0."""
    n_k_v = np.asarray(n_k_v).astype(np.int64)
    K, V = n_k_v.shape
    ids = np.arange(V)
    idx = np.full((K, n), -1, dtype=np.int32)
    cnt = np.zeros((K, n), dtype=np.int32)
    m = min(n, V)
    for k in range(K):
        order = np.lexsort((ids, -n_k_v[k]))[:m]
        idx[k, :m] = order
        cnt[k, :m] = n_k_v[k, order]
    return idx, cnt


def phi_of(n_k_v, beta):
    """get_phi by the reference's formula (LabeledLDA.py:231-234) with n_zk = the row sums of n_k_v"""
    n_k_v = np.asarray(n_k_v).astype(np.int64)
    V = n_k_v.shape[1]
    return (n_k_v + beta) / (n_k_v.sum(axis=1)[:, np.newaxis] + V * beta)


def cooc_ref(doc_off, word, top_idx, lo=0, hi=None):
    """(K, n, n) int64: a per-document set loop.  R(d, k) = the ranks whose word document d holds; co[k][i][j] += 1 for i >= j in R."""
    top_idx = np.asarray(top_idx)
    K, n = top_idx.shape
    lists = {}
    for k in range(K):
        for r in range(n):
            if top_idx[k, r] >= 0:
                lists.setdefault(int(top_idx[k, r]), []).append((k, r))
    co = np.zeros((K, n, n), dtype=np.int64)
    hi = len(doc_off) - 1 if hi is None else hi
    for d in range(lo, hi):
        ranks = {}
        for w in set(np.asarray(word[int(doc_off[d]):int(doc_off[d + 1])]).tolist()):
            for k, r in lists.get(w, ()):
                ranks.setdefault(k, set()).add(r)
        for k, R in ranks.items():
            for i in R:
                for j in R:
                    if i >= j:
                        co[k, i, j] += 1
    return co


def membership_ref(top_idx):
    """{word: sorted list of topic*16 + rank} of a (K, n) id table"""
    out = {}
    top_idx = np.asarray(top_idx)
    for k in range(top_idx.shape[0]):
        for r in range(top_idx.shape[1]):
            if top_idx[k, r] >= 0:
                out.setdefault(int(top_idx[k, r]), []).append(k * 16 + r)
    return {w: sorted(v) for w, v in out.items()}


def umass_ref(co_k, eps, on):
    """one topic, a per-pair loop with math.log; -> (value or nan, sum of |term|, pairs)"""
    ranks = [r for r in range(co_k.shape[0]) if on[r]]
    if len(ranks) < 2 or any(int(co_k[r, r]) == 0 for r in ranks):
        return float("nan"), 0.0, 0
    tot = mag = 0.0
    pairs = 0
    for i in ranks:
        for j in ranks:
            if i > j:
                t = math.log((float(co_k[i, j]) + eps) / float(co_k[j, j]))
                tot += t
                mag += abs(t)
                pairs += 1
    return tot, mag, pairs


def npmi_ref(co_k, D, on):
    ranks = [r for r in range(co_k.shape[0]) if on[r]]
    if len(ranks) < 2 or any(int(co_k[r, r]) == 0 for r in ranks):
        return float("nan"), 0.0, 0
    tot = mag = 0.0
    pairs = 0
    D = float(D)
    for i in ranks:
        for j in ranks:
            if i > j:
                c, ci, cj = float(co_k[i, j]), float(co_k[i, i]), float(co_k[j, j])
                if c == 0:
                    t = -1.0
                elif c >= D:
                    t = 1.0
                else:
                    t = math.log((c * D) / (ci * cj)) / -math.log(c / D)
                tot += t
                mag += abs(t)
                pairs += 1
    return tot / pairs, mag / pairs, pairs


def device_rows(n_k_v, pad=0):
    """the (V, KP) int32 device image of a (K, V) matrix: column topic_pos[k] of row v holds n_k_v[k][v], the padding ``pad``"""
    from lda_thesis_amd import _native
    n_k_v = np.asarray(n_k_v)
    K, V = n_k_v.shape
    lay = _native.layout_init(K)
    rows = np.full((V, lay["KP"]), pad, dtype=np.int32)
    rows[:, lay["topic_pos"]] = n_k_v.T.astype(np.int32)
    return rows


def mixed_corpus(rng, V, lens, repeat=True):
    """(doc_off int64, word int32): documents of the given numbers of sites over V words, ids drawn WITH replacement (a word may
    repeat inside a document) and skewed towards the low ids, in corpus order."""
    lens = np.asarray(lens, dtype=np.int64)
    doc_off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=doc_off[1:])
    u = rng.random(int(doc_off[-1]))
    word = np.minimum((u * u * V).astype(np.int64), V - 1).astype(np.int32)
    if not repeat:
        word = np.concatenate([rng.choice(V, size=int(m), replace=False) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return doc_off, word


def random_lists(rng, K, n, V, holes=0.0):
    """a (K, n) id table: n distinct words per topic (or all of V when V < n, the rest -1), a share ``holes`` of entries set to -1"""
    t = np.full((K, n), -1, dtype=np.int32)
    m = min(n, V)
    for k in range(K):
        t[k, :m] = rng.choice(V, size=m, replace=False)
    if holes:
        t[rng.random((K, n)) < holes] = -1
    return t
