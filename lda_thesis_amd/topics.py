"""Top words per topic and topic coherence (``llda_top_words``, ``llda_word_cooc``, ``llda_window_cooc``, include/llda_gibbs.h).

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

The sliding-window measures of Roeder, Both and Hinneburg ("Exploring the Space of Topic Coherence Measures", WSDM 2015) -- ``c_v``,
``c_uci``, ``c_npmi`` -- count windows of the running text instead of documents: ``token_csr`` keeps the token order that a
``doc2bow`` CSR drops, ``window_cooccurrence`` counts on the device (``llda_window_cooc``) and the three measures are host functions
of its integers and of ``window_count``.

Which words set a label apart is a float score, not a count: ``scored_words`` (``llda_scored_words``) ranks P_a(x) / wdiv with
96-bit (score, word) keys, ``relevance_powers`` turns LDAvis's lam (Sievert and Shirley 2014) into the integer powers whose
quotient has the order of relevance without a logarithm, and ``word_divisor`` builds the divisor from the words' totals.  Every
score is a fixed sequence of IEEE multiplications and one division of one element: numpy restates it bit for bit.

FREX (Bischof and Airoldi, "Summarizing topical content with word frequency and exclusivity", ICML 2012) scores a word by the
harmonic mean of two RANKS within the topic -- of its probability and of its exclusivity phi_kw / sum_j phi_jw -- so it needs every
topic's whole empirical distribution: ``ecdf_ranks`` (``llda_ecdf_ranks``: the segmented sort of ``llda_label_metrics`` over the
vocabulary) leaves the integer ranks, ``frex_select`` (``llda_frex_select``) orders the words by the exact integer fraction the two
ranks make, and ``frex_score`` is the float64 that is reported.  ``frex_words`` puts the three together in batches of labels.
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


def relevance_powers(lam):
    """(a, b) such that, within a topic, the order of LDAvis relevance lam * log(phi) + (1 - lam) * log(phi / p) is the order of
    phi^a / p^b: with lam = s / t (``Fraction(lam).limit_denominator(8)``) a = t and b = t - s.  1 -> (1, 0): phi itself; 0 -> (1, 1):
    lift; 0.5 -> (2, 1); 0.6 -> (5, 2)."""
    from fractions import Fraction
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:
        raise ValueError("lam must be in 0 .. 1")
    f = Fraction(lam).limit_denominator(_native.SCORED_MAX_A)
    return f.denominator, f.denominator - f.numerator


def _power(x, a):
    """P_a(x): a - 1 multiplications, left to right, each rounded"""
    p = x
    for _ in range(int(a) - 1):
        p = p * x
    return p


def word_divisor(n_w, b, min_count=1):
    """The divisor of ``scored_words`` for the power b of a word's overall share (numpy float64 [V]): p = n_w / sum(n_w),
    wdiv = P_b(p) by b - 1 multiplications (ones for b = 0), and 0 -- the word is not ranked -- where n_w < max(min_count, 1)."""
    n_w = np.asarray(n_w)
    b = int(b)
    if not 0 <= b <= _native.SCORED_MAX_A:
        raise ValueError("b must be in 0 .. %d" % _native.SCORED_MAX_A)
    p = n_w.astype(np.float64) / float(n_w.sum())
    wdiv = np.ones(p.shape, dtype=np.float64) if b == 0 else _power(p, b)
    wdiv[n_w < max(int(min_count), 1)] = 0.0
    return wdiv


def scored_words(source, K, n, a=1, wdiv=None, *, n_k=None, beta=None, den=None, stream=None):
    """The n best words of every topic by score = P_a(x) / wdiv (``llda_scored_words``): device tensors (top_idx (K, n) int32,
    top_score (K, n) float64, n_nan (K,) int32) in reference topic order, padded with -1 / NaN where a topic ranks fewer than n
    words.  ``source`` is either ``n_kw`` -- int32 (V, KP) on the device, word-major, device order; x is then phi of the counts,
    with ``beta`` and ``n_k`` (int32 [KP]) or ``den`` (float64 [KP]) as ``llda_readout_phi`` takes them -- or a float64 (V, ld)
    matrix on the device with its columns in reference topic order (x is the entry).  wdiv: float64 [V] (numpy or tensor) or
    None; a word whose wdiv is 0 is not ranked.  Enqueues on ``stream`` (default: the current one)."""
    import torch
    _native.lib()
    _native.require_device()
    n, K, a = _check_n(n), int(K), int(a)
    if not 1 <= a <= _native.SCORED_MAX_A:
        raise ValueError("a must be in 1 .. %d" % _native.SCORED_MAX_A)
    if not (isinstance(source, torch.Tensor) and source.is_cuda and source.dim() == 2 and source.dtype in (torch.int32, torch.float64)):
        raise ValueError("source must be an int32 (V, KP) or a float64 (V, ld) tensor on the device")
    counts = source.dtype == torch.int32
    dev = source.device
    V = int(source.shape[0])
    if counts:
        if beta is None or (n_k is None) == (den is None):
            raise ValueError("counts need beta and exactly one of n_k and den")
        source = source.contiguous()
        for name, t, dt in (("n_k", n_k, torch.int32), ("den", den, torch.float64)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dt and t.dim() == 1
                                      and t.is_contiguous() and int(t.numel()) == int(source.shape[1])):
                raise ValueError("%s must be a contiguous %s [KP] tensor on the device of the counts" % (name, dt))
    else:
        if n_k is not None or den is not None or beta is not None:
            raise ValueError("n_k, den and beta belong to the counts")
        if int(source.shape[1]) < K:
            raise ValueError("a matrix needs at least K columns")
        if source.stride(1) != 1 or source.stride(0) < int(source.shape[1]):
            source = source.contiguous()
    if wdiv is not None:
        wdiv = torch.as_tensor(wdiv).to(device=dev, dtype=torch.float64).contiguous()
        if tuple(wdiv.shape) != (V,):
            raise ValueError("wdiv must hold one value per word")
    nbytes = _native.scored_words_scratch_bytes(V, K, n)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        top_idx = torch.empty((K, n), dtype=torch.int32, device=dev)
        top_score = torch.empty((K, n), dtype=torch.float64, device=dev)
        n_nan = torch.empty((K,), dtype=torch.int32, device=dev)
        if counts:
            _native.scored_words(V, K, n, a, scratch, n_kw=source, n_k=n_k, den=den, beta=float(beta), wdiv=wdiv, top_idx=top_idx,
                                 top_score=top_score, n_nan=n_nan)
        else:
            _native.scored_words(V, K, n, a, scratch, mat=source, wdiv=wdiv, top_idx=top_idx, top_score=top_score, n_nan=n_nan)
        for t in (source, n_k, den, wdiv):
            if t is not None:
                t.record_stream(stream)
    return top_idx, top_score, n_nan


def frex_weight(w):
    """The weight on exclusivity as the fraction s / t ``llda_frex_select`` takes: ``Fraction(w).limit_denominator(64)``, 0 <= w <= 1
    (a ``Fraction`` or an (s, t) pair passes through).  0.5 -> 1/2, 0.7 -> 7/10, 1 -> 1/1, 0 -> 0/1."""
    from fractions import Fraction
    if isinstance(w, tuple):
        w = Fraction(int(w[0]), int(w[1]))
    if not 0.0 <= float(w) <= 1.0:                       # (false for a NaN)
        raise ValueError("the weight must be in 0 .. 1")
    f = w if isinstance(w, Fraction) else Fraction(float(w))
    return f.limit_denominator(_native.FREX_MAX_T)


def frex_score(rank_e, rank_f, Vc, s, t):
    """FREX = 1 / (omega / F_e + (1 - omega) / F_f) with omega = s / t and F = rank / Vc, as the float64 this project reports (numpy,
    element-wise): (float(t) * float(B)) / (float(Vc) * float(A)) with the integers A = s rf + (t - s) re and B = re rf, each step
    rounded; NaN where a rank is below 1.  A report: the order is decided on the integers (``frex_select``)."""
    re, rf = np.asarray(rank_e).astype(np.int64), np.asarray(rank_f).astype(np.int64)
    s, t = int(s), int(t)
    A, B = s * rf + (t - s) * re, re * rf
    ok = (re >= 1) & (rf >= 1)
    out = np.full(A.shape, np.nan, dtype=np.float64)
    out[ok] = (float(t) * B[ok].astype(np.float64)) / (float(int(Vc)) * A[ok].astype(np.float64))
    return out


def ecdf_ranks(mat, K, mode, cand=None, *, first=0, n_labels=None, chunk=0, value=False, stream=None):
    """Every word's ECDF rank within the columns first .. first + n_labels - 1 (default: all K) of ``mat``, a float64 (V, ld >= K)
    device tensor, word-major, reference topic order (``llda_ecdf_ranks``): device tensors (rank (n_labels, V) int32, n_cand (1,)
    int64[, value (n_labels, V) float64 with value=True]).  mode 0 ranks the entry, mode 1 the entry over the row's total (the
    exclusivity).  cand: uint8 / bool [V] (numpy or tensor) or None; a word outside it, or whose row total is not a positive
    finite number, gets rank 0.  rank = #{candidates with a value <= the word's}.  Enqueues on ``stream`` (default: the current)."""
    import torch
    _native.lib()
    _native.require_device()
    K, mode = int(K), int(mode)
    if mode not in (0, 1):
        raise ValueError("mode must be 0 or 1")
    if not (isinstance(mat, torch.Tensor) and mat.is_cuda and mat.dim() == 2 and mat.dtype == torch.float64):
        raise ValueError("mat must be a float64 (V, ld) tensor on the device")
    if int(mat.shape[1]) < K or K < 1:
        raise ValueError("the matrix needs at least K >= 1 columns")
    if mat.stride(1) != 1 or mat.stride(0) < int(mat.shape[1]):
        mat = mat.contiguous()
    V, dev = int(mat.shape[0]), mat.device
    n_labels = K - int(first) if n_labels is None else int(n_labels)
    if first < 0 or n_labels < 0 or first + n_labels > K:
        raise ValueError("first .. first + n_labels - 1 must lie in 0 .. K-1")
    if cand is not None:
        cand = torch.as_tensor(cand).to(device=dev).ne(0).to(torch.uint8).contiguous()
        if tuple(cand.shape) != (V,):
            raise ValueError("cand must hold one value per word")
    nbytes = _native.ecdf_scratch_bytes(V, n_labels, chunk)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        rank = torch.empty((n_labels, V), dtype=torch.int32, device=dev)
        val = torch.empty((n_labels, V), dtype=torch.float64, device=dev) if value else None
        n_cand = torch.zeros((1,), dtype=torch.int64, device=dev)
        _native.ecdf_ranks(mat, V, K, mode, first, n_labels, rank, scratch, chunk=chunk, cand=cand, value=val, n_cand=n_cand)
        for t in (mat, cand):
            if t is not None:
                t.record_stream(stream)
    return (rank, n_cand, val) if value else (rank, n_cand)


def frex_select(rank_f, rank_e, Vc, weight, n, probe=None, stream=None):
    """The n best words of every column by FREX from two int32 (L, V) device tensors of ranks in 0 .. Vc (``llda_frex_select``):
    device tensors (top_idx, top_rank_f, top_rank_e (L, n) int32, padded -1 / 0 / 0[, probe_rank_f, probe_rank_e (L, m) with
    probe (L, m) int32 word ids, -1 = no word]).  weight: the weight on exclusivity, anything ``frex_weight`` takes.  The order is
    exact: s / rank_e + (t - s) / rank_f ascending as integer fractions, then word id ascending."""
    import torch
    _native.lib()
    _native.require_device()
    n = int(n)
    if not 1 <= n <= _native.FREX_MAX_N:
        raise ValueError("n must be in 1 .. %d" % _native.FREX_MAX_N)
    f = frex_weight(weight)
    for r in (rank_f, rank_e):
        if not (isinstance(r, torch.Tensor) and r.is_cuda and r.dim() == 2 and r.dtype == torch.int32 and r.is_contiguous()):
            raise ValueError("rank_f and rank_e must be contiguous int32 (L, V) tensors on the device")
    if rank_f.shape != rank_e.shape or rank_f.device != rank_e.device:
        raise ValueError("rank_f and rank_e must have one shape and one device")
    L, V, dev = int(rank_f.shape[0]), int(rank_f.shape[1]), rank_f.device
    Vc = int(Vc)
    if not 1 <= Vc <= _native.ECDF_MAX_V:
        raise ValueError("Vc must be in 1 .. 2^30")
    m = 0
    if probe is not None:
        probe = torch.as_tensor(probe).to(device=dev, dtype=torch.int32).contiguous()
        if probe.dim() != 2 or int(probe.shape[0]) != L or not 1 <= int(probe.shape[1]) <= _native.FREX_MAX_N:
            raise ValueError("probe must be (L, m) with m in 1 .. %d" % _native.FREX_MAX_N)
        m = int(probe.shape[1])
    nbytes = _native.frex_scratch_bytes(V, L, n)
    stream = stream if stream is not None else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        out = [torch.empty((L, n), dtype=torch.int32, device=dev) for _ in range(3)]
        pr = [torch.empty((L, m), dtype=torch.int32, device=dev) for _ in range(2)] if m else [None, None]
        _native.frex_select(rank_f, rank_e, V, Vc, L, f.numerator, f.denominator, n, scratch, probe=probe, m=m, top_idx=out[0],
                            top_rank_f=out[1], top_rank_e=out[2], probe_rank_f=pr[0], probe_rank_e=pr[1])
        for t in (rank_f, rank_e, probe):
            if t is not None:
                t.record_stream(stream)
    return tuple(out) + (tuple(pr) if m else ())


def _frex_batch(V, K, free_bytes):
    """how many labels one batch of ``frex_words`` ranks: a label costs the sort's 24 bytes a (padded) word and its two rank rows"""
    Vp = -(-int(V) // _native.LABEL_CHUNK) * _native.LABEL_CHUNK
    return int(max(1, min(int(K), (int(free_bytes) // 2) // (24 * Vp + 8 * int(V)))))


def frex_words(phi_t, K, n, weight=0.5, cand=None, probe=None, batch=None):
    """The n FREX words of every topic of ``phi_t``, a float64 (V, ld >= K) device tensor, word-major, reference topic order: device
    tensors (top_idx, top_rank_f, top_rank_e (K, n) int32, Vc int[, probe_rank_f, probe_rank_e (K, m)]).  Two ``ecdf_ranks`` calls
    (phi, and phi over the word's total: the exclusivity) and one ``frex_select`` per batch of labels; batch = None sizes the batches
    to half of the device's free memory.  The batches change no bit.  No candidate word (Vc = 0): every list is padding."""
    import torch
    K, n = int(K), int(n)
    V, dev = int(phi_t.shape[0]), phi_t.device
    if batch is None:
        batch = _frex_batch(V, K, torch.cuda.mem_get_info(dev)[0])
    batch = max(1, int(batch))
    if probe is not None:
        probe = torch.as_tensor(probe).to(device=dev, dtype=torch.int32)
    tops, probes, Vc = [], [], 0
    for lo in range(0, K, batch):
        L = min(batch, K - lo)
        rank_f, n_cand = ecdf_ranks(phi_t, K, 0, cand, first=lo, n_labels=L)
        rank_e, _ = ecdf_ranks(phi_t, K, 1, cand, first=lo, n_labels=L)
        Vc = int(n_cand.item())
        if Vc == 0:
            tops.append((torch.full((L, n), -1, dtype=torch.int32, device=dev),) + tuple(torch.zeros((L, n), dtype=torch.int32, device=dev) for _ in range(2)))
            if probe is not None:
                probes.append(tuple(torch.zeros((L, int(probe.shape[1])), dtype=torch.int32, device=dev) for _ in range(2)))
            continue
        got = frex_select(rank_f, rank_e, Vc, weight, n, None if probe is None else probe[lo:lo + L])
        tops.append(got[:3])
        if probe is not None:
            probes.append(got[3:])
        del rank_f, rank_e
    out = tuple(torch.cat([b[i] for b in tops]) for i in range(3)) + (Vc,)
    if probe is not None:
        out = out + tuple(torch.cat([b[i] for b in probes]) for i in range(2))
    return out


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


def token_csr(texts, token2id):
    """Token lists -> (tok_off int64 [D+1], tok int32 [S]), numpy: the ids of ``token2id`` in reading order; a token it does not
    know becomes -1 and keeps its position."""
    tok_off = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=tok_off[1:])
    tok = np.fromiter((token2id.get(x, -1) for t in texts for x in t), dtype=np.int32, count=int(tok_off[-1]))
    return tok_off, tok


def _check_window(window):
    window = int(window)
    if not 0 <= window <= _native.WINDOW_MAX:
        raise ValueError("window must be in 0 .. %d" % _native.WINDOW_MAX)
    return window


def window_count(tok_off, window):
    """N, the number of windows ``window_cooccurrence`` visits: over the non-empty documents, L - window + 1 for a document of
    L > window tokens and 1 for a shorter one; window = 0 (the whole document) gives the number of non-empty documents."""
    s = _check_window(window)
    off = tok_off.cpu().numpy() if hasattr(tok_off, "cpu") else np.asarray(tok_off)
    L = np.diff(off.astype(np.int64))
    L = L[L > 0]
    return int(L.shape[0]) if s == 0 else int(np.maximum(1, L - s + 1).sum())


def window_cooccurrence(tok_off, tok, V, top_idx, window, out=None, table=None):
    """In how many sliding windows of ``window`` tokens the words listed in ``top_idx`` (K, n) meet, over the documents tok_off
    (int64 [D+1]) / tok (int32 [S], token ids in reading order, -1 = no dictionary word), both device tensors: an int64 (K, n, n)
    device tensor, co[k][i][j] for i >= j = the number of windows that hold both the word of rank i and the word of rank j of
    topic k (the diagonal: the windows that hold the word); j > i stays as it was.  A document no longer than the window, or
    window = 0, is one window.  ``out`` and ``table`` as in ``cooccurrence``."""
    import torch
    _native.lib()
    _native.require_device()
    window = _check_window(window)
    if not (isinstance(tok_off, torch.Tensor) and tok_off.is_cuda and tok_off.dtype == torch.int64 and tok_off.dim() == 1
            and tok_off.numel() >= 1 and tok_off.is_contiguous()):
        raise ValueError("tok_off must be a contiguous int64 [D+1] tensor on the device")
    if not (isinstance(tok, torch.Tensor) and tok.dtype == torch.int32 and tok.dim() == 1 and tok.is_contiguous()
            and tok.device == tok_off.device):
        raise ValueError("tok must be a contiguous int32 [S] tensor on the device of tok_off")
    dev = tok_off.device
    t = _as_device_ids(top_idx, dev)
    K, n = int(t.shape[0]), int(t.shape[1])
    if out is None:
        out = torch.zeros((K, n, n), dtype=torch.int64, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.int64 and tuple(out.shape) == (K, n, n) and out.is_contiguous()
              and out.device == dev):
        raise ValueError("out must be a contiguous int64 (K, n, n) tensor on the device of tok_off")
    D = int(tok_off.numel()) - 1
    if D == 0:
        return out
    memb_off, memb = table if table is not None else membership(t, V)
    if memb.numel() == 0:
        return out                                   # no topic lists a word: nothing to count
    _native.window_cooc(tok_off, tok, D, int(V), K, n, window, memb_off, memb, out)
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


# ---------------------------------------------------------------------------------------------- the sliding-window measures
EPS = 1e-12                                          # gensim's constant
DEFAULT_WINDOW = {"c_v": 110, "c_uci": 10, "c_npmi": 10}


def _window_topics(co, listed):
    """per topic: the symmetric float64 (m, m) table of the m listed ranks in rank order, c[a][b] = co[max][min] (the diagonal: c_a);
    None for a topic that gets NaN -- fewer than two listed words, or a listed word no window holds"""
    co, on = _listed(co, listed)
    for k in range(co.shape[0]):
        r = np.flatnonzero(on[k])
        low = np.tril(co[k][np.ix_(r, r)])
        if r.shape[0] < 2 or np.any(np.diagonal(low) == 0):
            yield None
            continue
        yield (low + np.tril(low, -1).T).astype(np.float64)


def _pmi_nlr(c, N):
    """(pmi, nlr) of a symmetric float64 count table, element by element: p = c / N, p_aa = p_a"""
    p = c / float(N)
    pi = np.diagonal(p)
    pmi = np.log((p + EPS) / (pi[:, None] * pi[None, :]))
    return pmi, pmi / -np.log(p + EPS)


def _pair_mean(co, N, listed, which):
    out = []
    for c in _window_topics(co, listed):
        if c is None:
            out.append(np.nan)
            continue
        term = np.ascontiguousarray(_pmi_nlr(c, N)[which][np.tril_indices(c.shape[0], -1)])
        out.append(float(np.sum(term)) / term.shape[0])
    return np.array(out, dtype=np.float64)


def c_uci(co, N, listed=None):
    """C_UCI per topic (float64 [K]) from ``window_cooccurrence``'s integers over N = ``window_count`` windows: the mean over the
    pairs i > j of a topic's listed words of pmi(i, j) = log((p_ij + EPS) / (p_i p_j)), p = windows / N.  NaN as in ``umass``."""
    return _pair_mean(co, N, listed, 0)


def c_npmi(co, N, listed=None):
    """C_NPMI per topic (float64 [K]): the mean over the same pairs of pmi(i, j) / -log(p_ij + EPS).  NaN as in ``umass``."""
    return _pair_mean(co, N, listed, 1)


def _cosine_mean(M):
    """the mean over the rows u_a of a symmetric float64 (m, m) matrix of cos(u_a, v), v = the sum of the rows; a cosine with a zero
    norm counts 0.0"""
    M = np.ascontiguousarray(M, dtype=np.float64)
    m = M.shape[0]
    v = np.array([np.sum(M[b]) for b in range(m)])                   # M is symmetric: the column sums, summed along rows
    nv = np.sqrt(np.sum(v * v))
    cos = np.zeros(m)
    for a in range(m):
        nu = np.sqrt(np.sum(M[a] * M[a]))
        if nu != 0.0 and nv != 0.0:
            cos[a] = np.sum(M[a] * v) / (nu * nv)
    return float(np.sum(cos)) / m


def c_v(co, N, listed=None):
    """C_V per topic (float64 [K]): every listed word a gets the vector u_a = (nlr(a, b))_b over the listed words b (nlr = pmi /
    -log(p_ab + EPS), p_aa = p_a), v is the sum of those vectors, and the value is the mean over a of the cosine of u_a and v
    (0.0 where a norm is 0).  NaN as in ``umass``."""
    return np.array([np.nan if c is None else _cosine_mean(_pmi_nlr(c, N)[1]) for c in _window_topics(co, listed)], dtype=np.float64)


def window_coherence(co, N, measure="c_v", listed=None):
    """``c_v``, ``c_uci`` or ``c_npmi`` by name."""
    if measure == "c_v":
        return c_v(co, N, listed=listed)
    if measure == "c_uci":
        return c_uci(co, N, listed=listed)
    if measure == "c_npmi":
        return c_npmi(co, N, listed=listed)
    raise ValueError("measure must be 'c_v', 'c_uci' or 'c_npmi'")
