"""Top words per topic and topic coherence (``llda_top_words``, ``llda_word_cooc``, include/llda_gibbs.h).

What a topic consists of, and whether its top words belong together.  The reference's ``topwords_per_topic``
(LabeledLDA.py:241-254 there) sorts every row of the (K, V) float64 ``phi`` on the host; here one pass over the integer
counts ``n_kw`` on the device leaves the n best words of every topic, and a second pass over a corpus CSR the document and
co-document frequencies of those words -- the integers UMass coherence (Mimno et al., "Optimizing Semantic Coherence in Topic
Models", EMNLP 2011) and NPMI are made of.  The host downloads K*n ids and K*n*n counts, never ``phi``.

Count order is phi order: phi[k][v] = (n_kw[v][k] + beta) / den[k] is strictly increasing in the count for a fixed topic and two
different counts never round to one double (V*beta < 2^40), so ``np.argsort(-get_phi()[k], kind="stable")`` is the order by count
descending, then word id ascending.  numpy's default ``argsort`` in the reference leaves the order of equal phi open; this does not.

Everything the device produces is an exact integer, independent of the geometry and of the number of ranks; ``umass`` and ``npmi``
are numpy-only host functions of those integers.
"""
import numpy as np

from . import _native

MAX_N = _native.TOPW_MAX_N


def _check_n(n):
    n = int(n)
    if not 1 <= n <= MAX_N:
        raise ValueError("n must be in 1 .. %d" % MAX_N)
    return n


def top_words(n_kw, K, n, stream=None):
    """The n best words of every topic of ``n_kw`` -- int32 (V, KP) on the device, word-major, device (group-layout) order: device
    tensors (top_idx, top_cnt), both (K, n) int32 in reference topic order, padded with -1 / 0 when V < n.  Enqueues on ``stream``
    (default: the current one)."""
    import torch
    _native.lib()
    _native.require_device()
    n, K = _check_n(n), int(K)
    if not (isinstance(n_kw, torch.Tensor) and n_kw.is_cuda and n_kw.dtype == torch.int32 and n_kw.dim() == 2):
        raise ValueError("n_kw must be an int32 (V, KP) tensor on the device")
    V = int(n_kw.shape[0])
    n_kw = n_kw.contiguous()
    dev = n_kw.device
    nbytes = _native.top_words_scratch_bytes(V, K, n)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        top_idx = torch.empty((K, n), dtype=torch.int32, device=dev)
        top_cnt = torch.empty((K, n), dtype=torch.int32, device=dev)
        _native.top_words(n_kw, V, K, n, top_idx, top_cnt, scratch)
        n_kw.record_stream(stream)
    return top_idx, top_cnt


def _as_device_ids(top_idx, device=None):
    import torch
    if isinstance(top_idx, torch.Tensor):
        t = top_idx if device is None else top_idx.to(device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(top_idx, dtype=np.int64))
        if device is None:
            device = "cuda:%d" % torch.cuda.current_device() if torch.cuda.is_available() else "cpu"
        t = t.to(device)
    if t.dim() != 2 or not 1 <= int(t.shape[1]) <= MAX_N:
        raise ValueError("top_idx must be (K, n) with n in 1 .. %d" % MAX_N)
    return t.to(torch.int64)


def membership(top_idx, V, device=None):
    """The table ``llda_word_cooc`` looks words up in, built on the device from a (K, n) table of word ids (-1 = no word):
    (memb_off int32 [V+1], memb int32 [M]); the entries memb_off[w] .. memb_off[w+1]-1 of memb are topic*16 + rank for every
    (topic, rank) that lists word w.  One sort, one bincount, one cumsum."""
    import torch
    t = _as_device_ids(top_idx, device)
    V = int(V)
    K, n = int(t.shape[0]), int(t.shape[1])
    flat = t.reshape(-1)
    entry = (torch.arange(K, device=t.device, dtype=torch.int64)[:, None] * 16
             + torch.arange(n, device=t.device, dtype=torch.int64)[None, :]).reshape(-1)
    listed = flat >= 0
    words, entry = flat[listed], entry[listed]
    if words.numel() and int(words.max().item()) >= V:
        raise ValueError("top_idx holds a word id outside 0 .. V-1")
    order = torch.sort(words, stable=True)[1]
    memb = entry[order].to(torch.int32)
    memb_off = torch.zeros((V + 1,), dtype=torch.int64, device=t.device)
    torch.cumsum(torch.bincount(words, minlength=V), 0, out=memb_off[1:])
    return memb_off.to(torch.int32), memb


def cooccurrence(doc_off, word, V, top_idx, out=None, table=None):
    """Document and co-document frequencies of the words listed in ``top_idx`` (K, n) over the corpus CSR doc_off (int64 [D+1]) /
    word (int32 [S]), both device tensors: an int64 (K, n, n) device tensor, co[k][i][j] for i >= j = the number of documents that
    hold both the word of rank i and the word of rank j of topic k (the diagonal: the document frequency); j > i stays as it was.
    ``out`` (a contiguous int64 (K, n, n) device tensor) is ADDED to -- pass the corpus in several document ranges, or None to
    start from zeros; table = a ``membership(top_idx, V)`` result to reuse."""
    import torch
    _native.lib()
    _native.require_device()
    if not (isinstance(doc_off, torch.Tensor) and doc_off.is_cuda and doc_off.dtype == torch.int64 and doc_off.dim() == 1
            and doc_off.numel() >= 1 and doc_off.is_contiguous()):
        raise ValueError("doc_off must be a contiguous int64 [D+1] tensor on the device")
    if not (isinstance(word, torch.Tensor) and word.dtype == torch.int32 and word.dim() == 1 and word.is_contiguous()
            and word.device == doc_off.device):
        raise ValueError("word must be a contiguous int32 [S] tensor on the device of doc_off")
    dev = doc_off.device
    t = _as_device_ids(top_idx, dev)
    K, n = int(t.shape[0]), int(t.shape[1])
    if out is None:
        out = torch.zeros((K, n, n), dtype=torch.int64, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.int64 and tuple(out.shape) == (K, n, n) and out.is_contiguous()
              and out.device == dev):
        raise ValueError("out must be a contiguous int64 (K, n, n) tensor on the device of doc_off")
    D = int(doc_off.numel()) - 1
    if D == 0:
        return out
    memb_off, memb = table if table is not None else membership(t, V)
    if memb.numel() == 0:
        return out                                   # no topic lists a word: nothing to count
    _native.word_cooc(doc_off, word, D, int(V), K, n, memb_off, memb, out)
    return out


# ---------------------------------------------------------------------------------------------- host side, numpy only
def _listed(co, listed):
    co = np.asarray(co)
    if co.ndim != 3 or co.shape[1] != co.shape[2]:
        raise ValueError("co must be (K, n, n)")
    K, n = co.shape[0], co.shape[1]
    if listed is None:
        return co, np.ones((K, n), dtype=bool)
    listed = np.asarray(listed)
    if listed.shape != (K, n):
        raise ValueError("listed must be (K, n)")
    return co, (listed >= 0 if listed.dtype != bool else listed)


def _pairs(co, listed):
    """per topic: the pairs i > j of listed ranks in list order (i ascending, then j), as float64 arrays (c_ij, c_ii, c_jj); None for
    a topic that gets NaN -- fewer than two listed words, or a listed word no document holds"""
    co, on = _listed(co, listed)
    n = co.shape[1]
    ii, jj = np.tril_indices(n, -1)
    for k in range(co.shape[0]):
        df = np.diagonal(co[k])
        if int(on[k].sum()) < 2 or np.any(df[on[k]] == 0):
            yield None
            continue
        keep = on[k][ii] & on[k][jj]
        i, j = ii[keep], jj[keep]
        yield co[k][i, j].astype(np.float64), df[i].astype(np.float64), df[j].astype(np.float64)


def umass(co, eps=1.0, listed=None):
    """UMass coherence per topic (float64 [K]) from ``cooccurrence``'s integers: sum over the pairs i > j of a topic's listed words,
    ranks in list order, of log((co[i][j] + eps) / co[j][j]).  listed: the (K, n) id table (-1 = no word) or a boolean mask of the
    ranks that hold a word (default: all).  A topic that lists a word with document frequency 0, or fewer than two words, gets
    NaN; nothing raises."""
    out = []
    for p in _pairs(co, listed):
        out.append(np.nan if p is None else float(np.sum(np.log((p[0] + float(eps)) / p[2]))))
    return np.array(out, dtype=np.float64)


def npmi(co, D, listed=None):
    """NPMI coherence per topic (float64 [K]) over D documents: the mean over the pairs i > j of a topic's listed words of
    log(p_ij / (p_i p_j)) / -log(p_ij) with p = document frequency / D, evaluated as log((c_ij * D) / (c_ii * c_jj)) / -log(c_ij / D);
    -1 for a pair no document holds and 1 for a pair every document holds (the limit under complete co-occurrence).  NaN as in
    ``umass``."""
    D = float(D)
    out = []
    for p in _pairs(co, listed):
        if p is None:
            out.append(np.nan)
            continue
        c, ci, cj = p
        term = np.full(c.shape, -1.0)
        full = c >= D
        term[full] = 1.0
        mid = (c > 0) & ~full
        term[mid] = np.log((c[mid] * D) / (ci[mid] * cj[mid])) / -np.log(c[mid] / D)
        out.append(float(np.sum(term)) / term.shape[0])
    return np.array(out, dtype=np.float64)


def coherence(co, D, measure="umass", listed=None):
    """``umass`` or ``npmi`` by name."""
    if measure == "umass":
        return umass(co, listed=listed)
    if measure == "npmi":
        return npmi(co, D, listed=listed)
    raise ValueError("measure must be 'umass' or 'npmi'")
