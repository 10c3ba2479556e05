"""Cases and a runner for llda_sweep_batch driven DIRECTLY (test infrastructure; tests/test_gpu_batch_direct.py).

``Ensemble.sweep()`` always builds the same launches: one per lane class, every instance of the class, longest first.  Here the device
buffers still come from ``Ensemble`` (its construction is pinned by the goldens), but ``sweep_batch`` is called with ``order`` tensors
and ``lanes`` of the test's own, and the reference is ``helpers.OracleBackend.sweep_batch`` -- the C oracle, problem by problem -- on
CPU copies of the same tensors taken before the launch.  z, n_dk and delta are compared as WHOLE buffers, bit for bit, each with guard
words before and behind; counts must not change.

A case (``case(lanes)``) is one ensemble whose instances all belong to one lane class:

  * one vocabulary of V = 300 words, freq in 1 .. 3 (< V: SubLDA's phantom column ``f`` exists), words distinct inside a document;
  * the problems of the class (``CLASSES[lanes]["Ks"]``: every T = 1, 2, 4, 8, 12, 16 of a one-leaf layout, with and without a tail) take
    the documents ROUND-ROBIN: document j belongs to problem j % P, so in ``order_rr`` (document order) neighbouring lane groups never
    share a problem and every wavefront of more than one group holds several (K, KP) pairs;
  * document lengths come from LENS -- 0 (an instance without a site), and the seams of the kernel's batches of 8 sites -- in a pattern
    that gives the 64 / lanes groups of a wavefront pairwise different lengths;
  * label sets of lo .. min(K, hi) topics, the first document of a problem exactly min(K, hi), the second exactly lo;
  * non-identity RNG streams; "other documents'" counts added to n_kw and n_k (uneven rows), one topic of one problem never used at all
    (``unused``: its get_ph row is 0/0);
  * with ``empty=True`` one instance of three sites has NO allowed topic.

``predict_exact`` restates the kernel's one decision (sparse_decide_f64: unsure when a live prefix lies within margin * total of
u * total) on the oracle's trajectory, which gives the number of exact-tier sites a launch must report at any margin.
"""
import functools

import numpy as np

import llda_oracle as orc

LENS = (0, 1, 7, 8, 9, 16, 17, 40)
V = 300
ALPHA, BETA, SEED = 0.1, 0.01, 977
GUARD = 8
PATTERN = {"z": -1234567, "n_dk": -7654321, "delta": 1515870810}          # (the last: 0x5A5A5A5A)

CLASSES = {
    8: dict(Ks=(1, 2, 5, 8, 9, 17, 60, 96, 100, 128), lo=1, hi=8, n_inst=70),        # 32 + 32 + 6 groups: 26 idle in the last workgroup
    16: dict(Ks=(16, 17, 60, 96, 97, 128), lo=9, hi=16, n_inst=19),                   # 16 + 3
    32: dict(Ks=(32, 33, 60, 100, 128), lo=17, hi=32, n_inst=9),                      # 8 + 1
    64: dict(Ks=(64, 65, 100, 128), lo=33, hi=64, n_inst=5),                          # 4 + 1
}
UNUSED = {8: (100, 57), 16: (97, 96), 32: (100, 3), 64: (128, 127)}                   # lanes -> (K of the problem, topic nobody uses)
EMPTY_DOC = 14                                                                        # the document without a label (empty=True)


@functools.lru_cache(maxsize=None)
def case(lanes, empty=False):
    """-> dict(plans, z_local, doc_off, word, freq, streams, order_rr, extras, lens, prob_of_doc, n_allowed, unused=(problem, topic),
    empty_inst or None); host only"""
    cl = CLASSES[lanes]
    Ks, n = cl["Ks"], cl["n_inst"]
    P = len(Ks)
    rng = np.random.default_rng([77, lanes, int(empty)])
    per_wave = 64 // lanes
    j = np.arange(n)
    lens = np.array(LENS)[(5 * j + j // 8) % 8]
    if empty:
        lens[EMPTY_DOC] = 3
    prob_of_doc = j % P
    doc_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    word = np.concatenate([rng.choice(V, size=L, replace=False) for L in lens]).astype(np.int32)
    freq = rng.integers(1, 4, size=int(doc_off[-1])).astype(np.int32)
    unused_p = Ks.index(UNUSED[lanes][0])
    unused_t = UNUSED[lanes][1]
    plans, z_local, extras = [], [], []
    n_allowed_doc = np.zeros(n, dtype=np.int64)
    for p, K in enumerate(Ks):
        docs = np.flatnonzero(prob_of_doc == p).astype(np.int64)
        lo, hi = min(cl["lo"], K), min(cl["hi"], K)
        topics = np.array([t for t in range(K) if not (p == unused_p and t == unused_t)])
        hi = min(hi, len(topics))
        allowed = np.full((len(docs), hi), -1, dtype=np.int64)
        n_allowed = np.zeros(len(docs), dtype=np.int64)
        zs = []
        for i, d in enumerate(docs):
            a = hi if i == 0 else lo if i == 1 else int(rng.integers(lo, hi + 1))
            if empty and d == EMPTY_DOC:
                a = 0
            allowed[i, :a] = np.sort(rng.choice(topics, size=a, replace=False))
            n_allowed[i] = a
            n_allowed_doc[d] = a
            zs.append(rng.choice(allowed[i, :a], size=lens[d]) if a else np.zeros(lens[d], dtype=np.int64))
        plans.append(dict(K=K, docs=docs, allowed=allowed, n_allowed=n_allowed))
        z_local.append(np.concatenate(zs).astype(np.int64))
        ext = np.floor(np.exp(rng.uniform(0.0, 6.0, size=(K, V)))).astype(np.int64)
        ext[rng.random((K, V)) < 0.4] = 0
        if p == unused_p:
            ext[unused_t] = 0
        extras.append(ext)
    # instance index of document j in the Ensemble's problem-major numbering
    start = np.concatenate(([0], np.cumsum([len(pl["docs"]) for pl in plans])))
    order_rr = (start[prob_of_doc] + j // P).astype(np.int32)
    streams = 100 + 7 * np.roll(np.arange(P)[::-1], 1)                 # neither the identity nor ascending
    assert len(set(streams.tolist())) == P and (streams != np.arange(P)).all()
    # what the table of DESIGN.md 4.4n says about the waves
    for w in range(0, n, per_wave):
        grp = slice(w, min(w + per_wave, n))
        if grp.stop - grp.start > 1:
            assert len(set(lens[grp].tolist())) == grp.stop - grp.start and len(set(prob_of_doc[grp].tolist())) == grp.stop - grp.start
    ordinary = n_allowed_doc[n_allowed_doc > 0]
    assert ordinary.min() == min(cl["lo"], min(Ks)) and ordinary.max() == cl["hi"] and (ordinary > lanes // 2).all() | (lanes == 8)
    assert int(freq.max()) < V
    return dict(lanes=lanes, plans=plans, z_local=z_local, doc_off=doc_off, word=word, freq=freq, streams=streams, order_rr=order_rr,
                extras=extras, lens=lens, prob_of_doc=prob_of_doc, n_allowed=n_allowed_doc, unused=(unused_p, unused_t),
                empty_inst=int(order_rr[EMPTY_DOC]) if empty else None)


def _guarded(body, pattern):
    import torch
    n = body.numel()
    buf = torch.full((n + 2 * GUARD,), pattern, dtype=body.dtype, device=body.device)
    buf[GUARD:GUARD + n] = body
    return buf


class Run(object):
    """the device state of a case: an Ensemble whose z, n_dk and delta are views into guarded buffers.  ``native`` is the module the
    launches go to (lda_thesis_amd._native on the device; an OracleBackend to try the runner itself on the CPU)."""

    def __init__(self, c, native, device=None):
        import torch
        from lda_thesis_amd.ensemble import Ensemble
        self.c, self.native = c, native
        self.ens = ens = Ensemble(c["plans"], c["z_local"], c["doc_off"], c["word"], c["freq"], V, ALPHA, BETA, SEED, device=device,
                                  streams=c["streams"])
        assert [g for g, _ in ens.orders] == [c["lanes"]] and ens.I == len(c["lens"])
        cnt = ens.counts.cpu().numpy().copy()
        for i, ext in enumerate(c["extras"]):                    # the counts of "other documents", in the device's position order
            kp, tp = int(ens._kp_h[i]), ens._layouts[c["plans"][i]["K"]].topic_pos.astype(np.int64)
            kw0, nk0 = int(ens._kw_off_h[i]), int(ens._nk_off_h[i])
            cnt[kw0:kw0 + V * kp].reshape(V, kp)[:, tp] += ext.T.astype(np.int32)
            cnt[nk0:nk0 + kp][tp] += ext.sum(axis=1).astype(np.int32)
        ens.counts.copy_(torch.from_numpy(cnt).to(ens.device))
        self._adopt()

    @classmethod
    def of(cls, ens, native):
        """the same runner over an Ensemble the caller has built (tests/test_gpu_sweep_ties.py: planted counts written over it):
        its z, n_dk and delta as they are now become the start state, in guarded buffers"""
        self = cls.__new__(cls)
        self.c, self.native, self.ens = None, native, ens
        self._adopt()
        return self

    def _adopt(self):
        ens = self.ens
        self.start = dict(z=ens.z.clone(), n_dk=ens.n_dk.clone(), counts=ens.counts.clone())
        self.reset()

    def reset(self):
        """the state of the case before any sweep, in fresh guarded buffers"""
        import torch
        ens = self.ens
        self.buf = dict(z=_guarded(self.start["z"], PATTERN["z"]), n_dk=_guarded(self.start["n_dk"], PATTERN["n_dk"]),
                        delta=_guarded(torch.zeros_like(self.start["counts"]), PATTERN["delta"]))
        ens.z, ens.n_dk, ens.delta = (self.buf[k][GUARD:self.buf[k].numel() - GUARD] for k in ("z", "n_dk", "delta"))
        ens.counts = self.start["counts"].clone()
        ens.status = torch.zeros((4,), dtype=torch.int32, device=ens.device)
        ens.sweeps_done = 0

    def _args(self, t):
        return dict(inst_off=t["inst_off"], word=t["word"], freq=t["freq"], z=t["z"], inst_prob=t["inst_prob"], inst_doc=t["inst_doc"],
                    live_off=t["live_off"], live_pos=t["live_pos"], ndk_off=t["ndk_off"], n_dk=t["n_dk"], kw_off=t["kw_off"],
                    nk_off=t["nk_off"], kp=t["kp"], prob_stream=t["prob_stream"], k=t["k"], counts=t["counts"], delta=t["delta"],
                    V=self.ens.V, alpha=self.ens.alpha, beta=self.ens.beta, seed=self.ens.seed)

    def tensors(self):
        e = self.ens
        return dict(inst_off=e.inst_off, word=e.word, freq=e.freq, z=e.z, inst_prob=e.inst_prob, inst_doc=e.inst_doc, live_off=e.live_off,
                    live_pos=e.live_pos, ndk_off=e.ndk_off, n_dk=e.n_dk, kw_off=e.kw_off, nk_off=e.nk_off, kp=e.kp,
                    prob_stream=e.prob_stream, k=e.prob_k, counts=e.counts, delta=e.delta)

    def host(self):
        """CPU copies of every tensor a launch takes (what the oracle then works on)"""
        return {k: v.detach().cpu().clone() for k, v in self.tensors().items()}

    def launch(self, order, lanes, margin, sweep=0):
        """one llda_sweep_batch call on the guarded buffers"""
        import torch
        o = torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32)).to(self.ens.device)
        self.native.sweep_batch(order=o, status=self.ens.status, lanes=lanes, sweep=sweep, debug_margin=margin,
                                **self._args(self.tensors()))

    def fold(self):
        self.native.apply_delta(self.ens.counts, self.ens.delta)

    def oracle_launch(self, backend, host, order, sweep=0):
        """the same launch through the C oracle on the CPU copies ``host`` (changed in place)"""
        import torch
        backend.sweep_batch(order=torch.as_tensor(np.ascontiguousarray(order, dtype=np.int32)), status=None, lanes=0, sweep=sweep,
                            **self._args(host))

    def check(self, want, what=""):
        """z, n_dk, delta as whole buffers == the oracle's, guards intact, counts what ``want`` holds (a launch does not write them)"""
        for name in ("z", "n_dk", "delta"):
            g = self.buf[name].cpu().numpy()
            n = g.shape[0] - 2 * GUARD
            assert (g[:GUARD] == PATTERN[name]).all() and (g[GUARD + n:] == PATTERN[name]).all(), "%s: guard words around %s overwritten" % (what, name)
            np.testing.assert_array_equal(g[GUARD:GUARD + n], want[name].numpy(), err_msg="%s: %s" % (what, name))
        np.testing.assert_array_equal(self.ens.counts.cpu().numpy(), want["counts"].numpy(), err_msg="%s: counts" % what)

    def status(self):
        return [int(x) for x in self.ens.status.cpu().numpy()]

    # ---- which words of the buffers belong to an instance
    def z_slice(self, i):
        off = self.ens._inst_off_h
        return slice(int(off[i]), int(off[i + 1]))

    def ndk_slice(self, i):
        off = self.ens._ndk_off_h
        return slice(int(off[i]), int(off[i + 1]))

    def sites(self, order):
        off = self.ens._inst_off_h
        o = np.asarray(order, dtype=np.int64)
        return int((off[o + 1] - off[o]).sum())


def predict_exact(before, after, order, margin_rel, sweep=0):
    """How many sites of the launch ``order`` the kernel's fp64 decision leaves to the exact tier at ``margin_rel``, and how far (relative
    to the total) the closest site is from the edge of the band -- from the CPU tensors before the launch and the oracle's after it.
    The kernel's words: w = (n_dk + alpha) * ((x + beta) / (n_k + V beta)) over the allowed positions in draw order (the document sees
    the snapshot counts and its own changes of n_dk and n_k), unsure when some inclusive prefix Q has |Q - u * total| <= margin * total
    (or the total is not positive)."""
    ioff, ip, idoc = before["inst_off"].numpy(), before["inst_prob"].numpy(), before["inst_doc"].numpy()
    loff, lpos, noff = before["live_off"].numpy(), before["live_pos"].numpy().astype(np.int64), before["ndk_off"].numpy()
    cnt, wd, fr = before["counts"].numpy().astype(np.int64), before["word"].numpy().astype(np.int64), before["freq"].numpy().astype(np.int64)
    z0, z1, nd0 = before["z"].numpy(), after["z"].numpy(), before["n_dk"].numpy().astype(np.int64)
    kp, kw_off, nk_off, stream = before["kp"].numpy(), before["kw_off"].numpy(), before["nk_off"].numpy(), before["prob_stream"].numpy()
    vbeta = V * BETA
    n_exact, edge = 0, np.inf
    for i in np.asarray(order, dtype=np.int64):
        p = int(ip[i])
        KP, pos = int(kp[p]), lpos[loff[i]:loff[i + 1]]
        L = int(ioff[i + 1] - ioff[i])
        if L == 0:
            continue
        if len(pos) == 0:
            n_exact += L
            continue
        nd = nd0[noff[i]:noff[i] + KP][pos].astype(np.float64)
        nk = cnt[nk_off[p]:nk_off[p] + KP][pos].astype(np.float64)
        us = orc.keyed_uniform(SEED, sweep, int(stream[p]), int(idoc[i]), np.arange(L))
        for n in range(L):
            s = int(ioff[i]) + n
            f, own = float(fr[s]), pos == z0[s]
            assert own.sum() == 1
            nd[own] -= f
            nk[own] -= f
            x = cnt[kw_off[p] + wd[s] * KP + pos].astype(np.float64) - f * own
            w = (nd + ALPHA) * ((x + BETA) / (nk + vbeta))
            Q, tot = np.cumsum(w), float(np.sum(w))
            gap = float(np.abs(Q - us[n] * tot).min()) / tot
            n_exact += gap <= margin_rel
            edge = min(edge, abs(gap - margin_rel))
            new = pos == z1[s]
            assert new.sum() == 1
            nd[new] += f
            nk[new] += f
    return int(n_exact), edge


# ---- numpy statements of the Ensemble's read-outs, from raw CPU buffers
def canon(a):
    """the bit patterns of a float64 array, every NaN as the one numpy's own 0/0 has (tests/test_gpu_dropin.py, the abstracts ensemble)"""
    a = np.array(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        a[np.isnan(a)] = (np.zeros(1) / np.zeros(1))[0]
    return a.view(np.uint64)


def numpy_state(ens, c, host, i):
    """(n_k_v, n_d_k, n_zk, z topics, get_ph) of problem i from the CPU tensors ``host``"""
    K, kp = c["plans"][i]["K"], int(ens._kp_h[i])
    lay = ens._layouts[K]
    tp = lay.topic_pos.astype(np.int64)
    cnt, nd, z = host["counts"].numpy().astype(np.int64), host["n_dk"].numpy().astype(np.int64), host["z"].numpy().astype(np.int64)
    kw0, nk0 = int(ens._kw_off_h[i]), int(ens._nk_off_h[i])
    n_k_v = np.ascontiguousarray(cnt[kw0:kw0 + V * kp].reshape(V, kp)[:, tp].T)
    n_zk = cnt[nk0:nk0 + kp][tp]
    i0 = int(ens._n_docs_h[:i].sum())
    D = int(ens._n_docs_h[i])
    d0 = int(ens._ndk_off_h[i0])
    n_d_k = nd[d0:d0 + D * kp].reshape(D, kp)[:, tp]
    zt = lay.pos_topic[z[int(ens._inst_off_h[i0]):int(ens._inst_off_h[i0 + D])]].astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ph = n_k_v / n_k_v.sum(axis=1)[:, np.newaxis]                    # CascadeLDA.py:394-395, phantom columns included
    return n_k_v, n_d_k, n_zk, zt, ph
