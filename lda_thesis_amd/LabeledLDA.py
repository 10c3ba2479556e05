"""Drop-in module for the reference's ``LabeledLDA.py`` with the Gibbs sweep on MI355X.

Surface mirrored (names reached through ``from LabeledLDA import *`` in
/root/reference/evaluate_LabeledLDA.py:1): ``load_corpus``, class ``LabeledLDA``, ``split_data``,
``prune_dict``, ``train_it``, ``test_it`` and the leaked ``np``.

What differs from the reference:
  * ``training_iteration()`` (reference LabeledLDA.py:101-125) is one launch of the HIP sweep kernel
    over all documents (per-document snapshot semantics, keyed Philox draw) instead of a python loop;
  * the sufficient statistics live in HBM; ``n_d_k``, ``n_k_v``, ``n_zk``, ``z_dn`` are properties that
    materialise them on the host in the reference's shapes and dtypes (LabeledLDA.py:73-79);
  * ``perplexity()`` (LabeledLDA.py:256-265) and the test-time fold-in sampler run on the device;
  * new, off by default: ``optimize_priors()`` and ``run_training(..., optimize_interval=n)`` fit alpha and beta to the counts while
    training (the reference fixes both); ``prior_trace`` records the fitted values;
  * new: ``heldout_perplexity()`` scores unseen documents by document completion on the device (``heldout.py``).
  * new: ``left_to_right()`` estimates the likelihood of unseen documents with a particle sampler on the device (``leftright.py``).
  * new: ``word_credit()`` / ``explain()`` say which words are credited to which label, ``fold_in_em()`` / ``predict_em()`` fold unseen
    documents in by EM, without random numbers (``attribution.py``).
  * new: ``similar_documents()``, ``similar_labels()``, ``predict_knn()`` / ``score_test_knn()`` find the nearest training documents
    (or labels) of a text under the Hellinger affinity on the device (``similar.py``).
Text preparation uses ``lda_thesis_amd.text`` instead of gensim (not installable here).
"""
import csv
import re
import sys

import numpy as np

from . import text as _text
from .corpus import csr_from_doc_tups
from . import _native
from .sampler import GibbsSampler, HostOrDevice, shard_documents

__all__ = ["np", "load_corpus", "LabeledLDA", "split_data", "prune_dict", "train_it", "test_it"]

_JEL = re.compile(r"[A-Z]\d{2}")


def _world_size():
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _rank():
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _gather_rows(local):
    """concatenate the per-rank slices of a document- or site-indexed array (read-out path, host side)."""
    if _world_size() == 1:
        return local
    import torch.distributed as dist
    parts = [None] * _world_size()
    dist.all_gather_object(parts, local)
    return np.concatenate(parts, axis=0)


def _raise_csv_limit():
    limit = sys.maxsize
    while True:
        try:
            csv.field_size_limit(limit)
            return
        except OverflowError:
            limit //= 10


def _parse_labels(field, d):
    """label column -> list of labels truncated to depth d (reference LabeledLDA.py:31-41)."""
    if len(field) > 3:
        return [tok[:d] for tok in field.split(" ") if _JEL.search(tok)]
    return [field[:d]]


def load_corpus(filename, d):
    """CSV rows (id, text, space separated JEL codes) -> (token lists, label lists, labelset).
    Same outputs as reference LabeledLDA.py:7-46; tokenisation by lda_thesis_amd.text."""
    _raise_csv_limit()
    texts, labs, seen = [], [], {}
    with open(filename, "r") as fh:
        for row in csv.reader(fh):
            lab = _parse_labels(row[2], d)
            for x in lab:
                seen.setdefault(x, 1)
            texts.append(row[1])
            labs.append(list(set(lab)))
    print("Stemming documents ....")
    return _text.preprocess_documents(texts), labs, list(seen.keys())


class LabeledLDA(object):
    """Labeled LDA trained by collapsed Gibbs sampling on the GPU.

    Constructor arguments as the reference (LabeledLDA.py:50); ``seed`` keys the device RNG (default:
    one draw from numpy's global stream after the initial assignments, so ``np.random.seed`` makes a
    whole run reproducible) and ``device`` picks the GPU."""

    def __init__(self, docs, labs, labelset, dicti, alpha, beta, seed=None, device=None):
        labelset.insert(0, "root")                    # the caller's list is extended, as in the reference
        self.labelmap = {lab: i for i, lab in enumerate(labelset)}
        self.K = len(self.labelmap)
        self.dicti = dicti
        self.alpha = alpha
        self.beta = beta
        self.vocab = list(dicti.values())
        self.w_to_v = dicti.token2id
        self.v_to_w = dicti.id2token
        # labs[d] = set_label(labs[d]) for every document at once (reference LabeledLDA.py:63,94-99: root + the document's labels;
        # an unknown label is a KeyError there too)
        self.D = len(docs)
        lab_len = np.fromiter(map(len, labs), dtype=np.int64, count=len(labs))
        lab_col = np.fromiter((self.labelmap[x] for lab in labs for x in lab), dtype=np.int64, count=int(lab_len.sum()))
        self.labs = np.zeros((len(labs), self.K))
        self.labs[:, 0] = 1.0
        self.labs[np.repeat(np.arange(len(labs)), lab_len), lab_col] = 1.0
        self.doc_tups = [dicti.doc2bow(x) for x in docs]
        self.V = len(self.vocab)
        self._ph_hat = HostOrDevice(np.zeros((self.K, self.V), dtype=float))
        self._th_hat = HostOrDevice(np.zeros((self.D, self.K), dtype=float))
        self.cur_perplx = []
        self.prior_trace = []                         # (sweep, alpha, beta) of every optimize_priors() inside run_training

        doc_off, word, freq = csr_from_doc_tups(self.doc_tups)
        self._doc_off = doc_off
        lens = np.diff(doc_off)
        if len(lens) and int(lens.min()) == 0:
            raise ValueError("not enough values to unpack: a document has no in-vocabulary word")
        word_l, freq_l, off_l = word.tolist(), freq.tolist(), doc_off.tolist()
        self.docs = [word_l[a:b] for a, b in zip(off_l[:-1], off_l[1:])]
        self.freqs = [freq_l[a:b] for a, b in zip(off_l[:-1], off_l[1:])]
        # Initial assignments.  The reference draws np.random.choice(K, size=len(doc), p=lab / lab.sum()) per document
        # (LabeledLDA.py:80-88); numpy's legacy choice is cdf = p.cumsum(); cdf /= cdf[-1]; cdf.searchsorted(random_sample(n), 'right'),
        # so ONE random_sample of all sites in document order consumes the global stream identically and the searchsorted becomes a
        # lookup in the cdf table of the document's label-set size (ensemble.draw_initial_topics, checked against np.random.choice
        # itself in tests/test_host_logic.py) -- the same z under np.random.seed, without 4 171 python-level calls.
        z0 = self._initial_topics(lens)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        self.seed = seed
        # with torch.distributed initialised the documents are sharded over the ranks by site count
        # (every rank builds the same model object from the same data; it keeps only its slice on the GPU)
        self._bounds = shard_documents(doc_off, _world_size())
        lo, hi = self._bounds[_rank()], self._bounds[_rank() + 1]
        s0, s1 = int(doc_off[lo]), int(doc_off[hi])
        self._sampler = GibbsSampler(doc_off[lo:hi + 1] - doc_off[lo], word[s0:s1], freq[s0:s1], z0[s0:s1],
                                     self.K, self.V, alpha, beta, labs=self.labs[lo:hi], counts=None, seed=seed,
                                     doc_base=lo, device=device)

    # ---- state in the reference's shapes / dtypes ----
    # With torch.distributed initialised the documents are sharded over the ranks: n_d_k, z_dn, th_hat, get_theta()
    # and pickling (__getstate__) GATHER the per-rank slices and are therefore COLLECTIVE -- every rank must read
    # them (reading on one rank only, e.g. `if rank == 0: pickle.dump(model)`, blocks).  n_zk, n_k_v, ph_hat and
    # perplexity() are replicated / already reduced and can be read anywhere.
    # (materialising the state synchronises anyway: the status word is looked at first -- where the reference would have raised
    # inside the sweep, LabeledLDA.py:117-119, the caller gets the ValueError no later than here)
    @property
    def n_zk(self):
        self._sampler.check_status()
        return self._sampler.n_zk()

    @property
    def n_d_k(self):
        self._sampler.check_status()
        return _gather_rows(self._sampler.n_d_k())

    @property
    def n_k_v(self):
        self._sampler.check_status()
        return self._sampler.n_k_v()

    @property
    def z_dn(self):
        self._sampler.check_status()
        z = _gather_rows(self._sampler.z_topics())
        return [z[self._doc_off[d]:self._doc_off[d + 1]].copy() for d in range(self.D)]

    # running means of phi / theta: numpy arrays when read (reference LabeledLDA.py:65-66); between the
    # thinning read-outs of run_training they stay on the device
    @property
    def ph_hat(self):
        return self._ph_hat.get()

    @ph_hat.setter
    def ph_hat(self, value):
        self._ph_hat.set(value)

    @property
    def th_hat(self):
        return self._th_hat.get(_gather_rows)

    @th_hat.setter
    def th_hat(self, value):
        self._th_hat.set(value)

    def _initial_topics(self, lens):
        from .ensemble import draw_initial_topics
        if int(lens.sum()) == 0:
            return np.zeros(0, np.int64)
        n_allowed = self.labs.sum(axis=1).astype(np.int64)
        rows, cols = np.nonzero(self.labs)                       # row major: a document's allowed topics ascending
        first = np.zeros(self.D + 1, dtype=np.int64)
        np.cumsum(n_allowed, out=first[1:])
        allowed = np.full((self.D, int(n_allowed.max()) if self.D else 1), -1, dtype=np.int64)
        allowed[rows, np.arange(rows.shape[0]) - first[rows]] = cols
        u = np.random.random_sample(int(lens.sum()))
        return draw_initial_topics(allowed, n_allowed, np.repeat(np.arange(self.D), lens), u)

    def set_label(self, label):
        vec = np.zeros(len(self.labelmap))
        vec[0] = 1.0
        for x in label:
            vec[self.labelmap[x]] = 1.0
        return vec

    # ---- training ----
    def training_iteration(self):
        """One Gibbs sweep over every (document, word) site: reference LabeledLDA.py:101-125.  A site whose probabilities are all
        zero makes numpy raise at that site (LabeledLDA.py:117-119); here the kernels set a status bit, which a caller that loops this
        method sees a few sweeps later (an asynchronous copy, no synchronisation) and at the latest when it reads the counts."""
        self._sampler.sweep()
        self._sampler.post_status()

    def optimize_priors(self, alpha=True, beta=True, n_bins=65536):
        """Fit the symmetric priors to the current state: Minka's fixed point (``priors.py``) on the counts of counts of n_dk and
        n_kw, which ``llda_count_hist`` builds on the device.  alpha / beta = False leaves that prior as it is.  Sets self.alpha /
        self.beta and the sampler's priors (next sweep, read-outs, perplexity, fold-in, pickling) and returns the pair.
        COLLECTIVE with several ranks; rank 0's two doubles are broadcast so that every rank hands its kernels identical scalars."""
        from . import priors
        sm = self._sampler
        sm.check_status()
        hist_dk, over_dk, hist_kw, over_kw = sm.count_histograms(n_bins)
        est = priors.estimate(self.alpha if alpha else None, self.beta if beta else None, hist_dk=hist_dk, over_dk=over_dk,
                              classes=self._doc_classes(), hist_kw=hist_kw, over_kw=over_kw, n_k=sm.n_zk(), V=self.V)
        a = float(est.alpha) if alpha else float(self.alpha)
        b = float(est.beta) if beta else float(self.beta)
        if _world_size() > 1:
            import torch
            import torch.distributed as dist
            # (a SUM in which every rank but 0 adds zeros: exact, and the collective the sweeps already use)
            t = torch.tensor([a, b] if _rank() == 0 else [0.0, 0.0], dtype=torch.float64, device=sm.device)
            dist.all_reduce(t)
            a, b = float(t[0]), float(t[1])
        sm.set_priors(a, b)
        self.alpha, self.beta = a, b
        return a, b

    def _doc_classes(self):
        """the unique (allowed topics, tokens) pairs of ALL documents with their multiplicities (static; every rank holds the
        full labs and CSR on the host)"""
        from . import priors
        cls = self.__dict__.get("_classes")
        if cls is None:
            doc_off, _, freq = csr_from_doc_tups(self.doc_tups)
            pre = np.concatenate([[0], np.cumsum(np.asarray(freq, dtype=np.int64))])
            cls = self._classes = priors.doc_classes(self.labs.sum(axis=1), pre[doc_off[1:]] - pre[doc_off[:-1]])
        return cls

    def run_training(self, iters, thinning, optimize_interval=0, optimize_burn_in=0):
        """Sweep loop with thinning read-outs and running means: reference LabeledLDA.py:127-153.  phi, theta,
        their running means and the three guards are evaluated on the device (llda_readout_phi / _theta).
        optimize_interval = n > 0: after the sweeps optimize_burn_in + n, + 2n, ... of this call ``optimize_priors()`` refits
        alpha and beta (before that sweep's thinning read-out, if it has one) and (sweep, alpha, beta) is appended to
        ``self.prior_trace``; 0 (default): the priors never change."""
        import torch
        sm = self._sampler
        lo, hi = self._bounds[_rank()], self._bounds[_rank() + 1]
        for n in range(iters):
            self.training_iteration()
            print('Running iteration # %d ' % (n + 1))
            if optimize_interval > 0 and n + 1 > optimize_burn_in and (n + 1 - optimize_burn_in) % optimize_interval == 0:
                a, b = self.optimize_priors()
                self.__dict__.setdefault("prior_trace", []).append((n + 1, a, b))
            if (n + 1) % thinning != 0:
                continue
            sm.check_status()
            self.cur_perplx.append(self.perplexity())
            s = (n + 1) / thinning
            first = s == 1
            keep, share = (None, None) if first else ((s - 1) / s, 1 / s)
            flags = torch.zeros((1,), dtype=torch.int32, device=sm.device)
            sm.phi(self._ph_hat.on_device(sm.device, (self.K, self.V), fresh=first), keep, share, flags)
            sm.theta(self._th_hat.on_device(sm.device, (sm.D, self.K), fresh=first, rows=(lo, hi)), keep, share)
            bad = int(flags.item())
            if bad & _native.READOUT_NEGATIVE:
                raise ValueError('A negative value occurred in self.ph_hat while saving iteration %d ' % n)
            if bad & _native.READOUT_NAN:
                raise ValueError('A nan has creeped into ph_hat')
            if bad & _native.READOUT_NO_LOAD:
                raise ValueError('A word in dictionary has no z-value')

    def fit_em(self, iters=50, theta_steps=1, start="counts", chunk=4096, trace_every=0, sparse=False, sparse_trace=False):
        """Fit ``ph_hat`` / ``th_hat`` by EM on the device, without random numbers (``emfit.fit``): ``iters`` passes
        of the theta M-step (``theta_steps`` steps of llda_attribute with alpha), the word-side E-step (llda_credit_words) and the
        phi M-step (llda_phi_step with beta).  start = "counts": from ``get_theta()`` / ``get_phi()`` of the current counts (the
        random initial assignments break the symmetry between labels that always occur together); "ph_hat": from the running
        means.  Theta is 0 outside a document's labels at the start and stays 0.  The result goes to ``ph_hat`` / ``th_hat`` and the
        hats count as filled: ``word_credit``, ``fold_in_em``, ``predict_em``, ``heldout_perplexity``, ``left_to_right`` and
        ``label_words(source="ph_hat")`` read the EM estimates, and ``cur_perplx`` gets the perplexity of the training sites under
        them.  z, the counts, the priors and the draw keys are not touched: a later ``run_training`` continues the chain as if this
        had not been called, and its first thinning read-out starts the running means afresh.  trace_every = n > 0: the data term
        sum f log p every n iterations.  Returns dict(iterations=iters, trace=[(iteration, loglik, tokens, bad), ...]).
        sparse=True: the sparse-label form (``emfit.fit_sparse``) -- the label sets come from ``labs`` and the start
        loads are the same theta at those labels; a site then costs len(labels) entries of phi, not K, on both sides of the
        E-step.  At most 32 labels per document (ValueError beyond).  The sums pair their terms by slot, not by topic id, so the
        estimates differ from the default's in their last bits (not at all where every label set is a prefix 0 .. L - 1).
        sparse_trace=True (with sparse): the trace is scored on the slots too (llda_heldout_loglik_sparse), not on a (D, K) matrix.
        One device only: with several ranks it raises."""
        import torch
        from . import emfit, heldout
        if _world_size() > 1:
            raise ValueError("fit_em runs on one device only: it was called with %d ranks" % _world_size())
        if start not in ("counts", "ph_hat"):
            raise ValueError("start must be 'counts' or 'ph_hat'")
        if sparse_trace and not sparse:
            raise ValueError("sparse_trace=True goes with sparse=True")
        sm = self._sampler
        sm.check_status()
        dev = sm.device
        if start == "counts" or not self.cur_perplx:
            th0, ph0 = sm.theta(), sm.phi()
        else:
            ph0 = self._ph_hat.dev if self._ph_hat.dev is not None else torch.from_numpy(np.ascontiguousarray(self.ph_hat, dtype=np.float64))
            th0 = self._th_hat.dev if self._th_hat.dev is not None else torch.from_numpy(np.ascontiguousarray(self.th_hat, dtype=np.float64))
        doc_off, word, freq = csr_from_doc_tups(self.doc_tups)
        if sparse:
            from . import attribution, docmodel
            lab_off, lab = docmodel.label_csr(np.asarray(self.labs), K=self.K)
            docmodel.label_sets(lab_off, lab, len(lab_off) - 1, self.K)     # (more than 32 labels in a document: ValueError, before any launch)
            r = emfit.fit_sparse(attribution.gather_slots(th0.to(dev), lab_off, lab), ph0.to(dev).t().contiguous(), doc_off, word, freq,
                                 lab_off, lab, float(self.alpha), float(self.beta), iters, theta_steps=theta_steps, chunk=chunk,
                                 trace_every=trace_every, sparse_trace=bool(sparse_trace))
        else:
            r = emfit.fit(th0.to(dev), ph0.to(dev).t().contiguous(), doc_off, word, freq, float(self.alpha), float(self.beta), iters,
                          theta_steps=theta_steps, chunk=chunk, trace_every=trace_every)
        self._ph_hat.set(None)
        self._ph_hat.dev = r["phi_t"].t().contiguous()
        self._th_hat.set(None)
        self._th_hat.dev = r["theta"]
        mant, expo, tok, bad = heldout.loglik(r["theta"], r["phi_t"], doc_off, word, freq, weighted=False)
        s = heldout.perplexity_from(mant, expo, tok, bad)
        self.cur_perplx.append(float(np.exp(-s["loglik"] / max(s["tokens"], 1))))     # (sites unweighted, as in ``perplexity``)
        return dict(iterations=r["iterations"], trace=r["trace"])

    # ---- read-outs ----
    def get_phi(self):
        """(n_k_v + beta) / (n_zk + V*beta): reference LabeledLDA.py:231-234 (llda_readout_phi)."""
        return self._sampler.phi().cpu().numpy()

    def get_theta(self):
        """(n_d_k + labs*alpha) / row sums: reference LabeledLDA.py:236-239 (llda_readout_theta)."""
        return _gather_rows(self._sampler.theta().cpu().numpy())

    def perplexity(self):
        """exp(-sum_sites log(phi[:, w] . theta_d) / #sites), sites unweighted by frequency
        (reference LabeledLDA.py:256-265); evaluated by the llda_loglik HIP kernel."""
        return self._sampler.perplexity()

    def topwords_per_topic(self, topwords=10, device=False, lam=None):
        """[label, word, word, ...] for every label: reference LabeledLDA.py:241-254, from the downloaded ``get_phi()``.
        device=True takes the same lists from ``top_words`` (topwords <= 16): 8*K*topwords bytes come back instead of the (K, V)
        phi.  Ties then go by word id ascending, where the default ``argsort`` here and in the reference leaves the order of
        equal phi open; without ties the two agree.  lam = a relevance in 0 .. 1: the DISTINCTIVE words of ``label_words`` instead."""
        names = list(self.labelmap.keys())
        if lam is not None:
            idx, _ = self.label_words(topwords, lam)
            return [[names[k]] + [self.v_to_w[int(v)] for v in idx[k] if v >= 0] for k in range(self.K)]
        if device:
            idx, _ = self.top_words(topwords)
            return [[names[k]] + [self.v_to_w[int(v)] for v in idx[k] if v >= 0] for k in range(self.K)]
        ph = self.get_phi()
        return [[names[k]] + [self.v_to_w[v] for v in np.argsort(-ph[k, :])[:topwords]]
                for k in range(self.K)]

    # ---- topic summaries on the device (new): top words by count and their coherence ----
    def top_words(self, n=10):
        """The n <= 16 best words of every label: ((K, n) word ids, (K, n) counts) as numpy arrays, ids padded with -1 when
        V < n.  The order is count descending, then word id ascending: ``np.argsort(-get_phi()[k], kind="stable")[:n]``
        (``topics.py``).  n_k_v is replicated: no collective."""
        self._sampler.check_status()
        idx, cnt = self._sampler.top_words(n)
        return idx.cpu().numpy(), cnt.cpu().numpy()

    def _label_words_device(self, n, lam, min_count, source="counts"):
        """``label_words`` as device tensors (top_idx, top_score)"""
        from . import topics
        if source not in ("counts", "ph_hat"):
            raise ValueError("source must be 'counts' or 'ph_hat'")
        a, b = topics.relevance_powers(lam)
        sm = self._sampler
        sm.check_status()
        # lam = 1 and no minimum count: nothing divides and no word is left out
        wdiv = None if b == 0 and int(min_count) < 1 else topics.word_divisor(sm.word_totals().cpu().numpy(), b, min_count)
        if source == "counts":
            idx, score, _ = sm.scored_words(n, a, wdiv)
        else:
            idx, score, _ = topics.scored_words(self._phi_t_device(), self.K, n, a, wdiv)
        return idx, score

    def label_words(self, n=10, lam=0.6, min_count=1, source="counts"):
        """The n <= 16 most DISTINCTIVE words of every label: ((K, n) int32 word ids, (K, n) float64 scores) as numpy arrays, padded
        with -1 / NaN where a label ranks fewer than n words.  The order is that of LDAvis relevance (Sievert and Shirley 2014)
        lam * log(phi) + (1 - lam) * log(phi / p), p = a word's share of the corpus, at lam rounded to a fraction s / t with t <= 8
        (``topics.relevance_powers``): the score is phi^t / p^(t - s) -- no logarithm, so numpy restates it bit for bit -- descending,
        then word id ascending (llda_scored_words).  lam = 1 ranks by phi, lam = 0 by lift phi / p.  Words that occur fewer than
        max(min_count, 1) times in the corpus are not ranked (min_count < 1 at lam = 1: every word is).  source = "counts": phi of
        the current counts; "ph_hat": the running mean of the thinning read-outs (the current phi before the first one).
        n_k_v is replicated: no collective."""
        idx, score = self._label_words_device(n, lam, min_count, source)
        return idx.cpu().numpy(), score.cpu().numpy()

    def _frex_device(self, n, weight, min_count, source, probe_n=0):
        """``topics.frex_words`` on this model's phi (``source`` as in ``label_words``) with the words that occur at least
        max(min_count, 1) times as candidates; probe_n > 0: the probes are every label's probe_n most probable candidate words"""
        import torch
        from . import topics
        if source not in ("counts", "ph_hat"):
            raise ValueError("source must be 'counts' or 'ph_hat'")
        topics._check_n(n)
        f = topics.frex_weight(weight)
        sm = self._sampler
        sm.check_status()
        phi_t = sm.phi().t().contiguous() if source == "counts" else self._phi_t_device()
        cand = (sm.word_totals() >= max(int(min_count), 1)).to(device=phi_t.device, dtype=torch.uint8)
        probe = None
        if probe_n:
            probe = topics.scored_words(phi_t, self.K, probe_n, 1, cand.to(torch.float64))[0]
        return f, topics.frex_words(phi_t, self.K, n, f, cand, probe)

    def frex_words(self, n=10, weight=0.5, min_count=1, source="counts"):
        """The n <= 16 FREX words of every label (Bischof and Airoldi 2012; the default labelling of the ``stm`` package): ((K, n)
        int32 word ids, (K, n) float64 FREX) as numpy arrays, padded with -1 / NaN where a label ranks fewer than n words.
        FREX = 1 / (w / F_e + (1 - w) / F_f): F_f is the ECDF of phi within the label at the word, F_e the ECDF of the word's
        exclusivity phi_kw / sum_j phi_jw, both over the candidate words -- those that occur at least max(min_count, 1) times in the
        corpus -- and w = weight, the weight on exclusivity, rounded to a fraction s / t with t <= 64 (``topics.frex_weight``).  Equal
        values share the rank of the last of them (the ECDF itself; ``stm`` averages their ranks).  The order is FREX descending
        decided on the exact integer fraction of the two ranks, then word id ascending (llda_ecdf_ranks, llda_frex_select); the
        float64 is ``topics.frex_score``.  weight = 0 orders by phi, weight = 1 by exclusivity.  source as in ``label_words``.
        n_k_v is replicated: no collective."""
        from . import topics
        f, (idx, rf, re, Vc) = self._frex_device(n, weight, min_count, source)
        return idx.cpu().numpy(), topics.frex_score(re.cpu().numpy(), rf.cpu().numpy(), Vc, f.numerator, f.denominator)

    def exclusivity(self, n=10, weight=0.7, min_count=1, source="counts"):
        """Topic exclusivity (float64 [K]), the second axis of the "semantic coherence against exclusivity" plot of ``stm``: the
        sum of FREX (weight on exclusivity ``weight``, as in ``frex_words``) over the label's n <= 16 most probable candidate words
        -- the order of ``label_words(n, 1, min_count)``: phi descending, then word id ascending --, added in that order.  NaN for
        a label with no ranked word.  n_k_v is replicated: no collective."""
        from . import topics
        f, (_, _, _, Vc, prf, pre) = self._frex_device(1, weight, min_count, source, probe_n=topics._check_n(n))
        fx = topics.frex_score(pre.cpu().numpy(), prf.cpu().numpy(), Vc, f.numerator, f.denominator)
        listed = ~np.isnan(fx)
        total = np.zeros((self.K,), dtype=np.float64)
        for j in range(fx.shape[1]):
            total = total + np.where(listed[:, j], fx[:, j], 0.0)
        total[~listed.any(axis=1)] = np.nan
        return total

    def coherence(self, n=10, measure="umass", docs=None, lam=None, min_count=1):
        """Topic coherence of every label's n best words (float64 [K]; NaN for a label with fewer than two words or with a top
        word that the corpus never holds): measure = "umass" (Mimno et al. 2011) or "npmi", over the training corpus or, with
        ``docs`` (token lists, through ``dicti.doc2bow``), over that reference corpus.  The document and co-document
        frequencies are counted on the device (llda_word_cooc).  Over the training corpus COLLECTIVE with several ranks;
        ``docs`` are counted whole on every rank.  lam = a relevance in 0 .. 1: the coherence of the lists of
        ``label_words(n, lam, min_count)`` instead of the most frequent words."""
        from . import topics
        if measure not in ("umass", "npmi"):
            raise ValueError("measure must be 'umass' or 'npmi'")
        sm = self._sampler
        sm.check_status()
        idx = sm.top_words(n)[0] if lam is None else self._label_words_device(n, lam, min_count)[0]
        if docs is None:
            co, D = sm.word_cooccurrence(idx)
        else:
            import torch
            doc_off, word, _ = csr_from_doc_tups([self.dicti.doc2bow(x) for x in docs])
            co = topics.cooccurrence(torch.from_numpy(np.ascontiguousarray(doc_off, dtype=np.int64)).to(sm.device),
                                     torch.from_numpy(np.ascontiguousarray(word, dtype=np.int32)).to(sm.device), self.V, idx)
            co, D = co.cpu().numpy(), len(doc_off) - 1
        return topics.coherence(co, D, measure, listed=idx.cpu().numpy())

    def window_coherence(self, texts, n=10, measure="c_v", window=None, lam=None, min_count=1):
        """Sliding-window coherence of every label's n best words (float64 [K], NaN as in ``coherence``): measure = "c_v", "c_uci"
        or "c_npmi" (Roeder, Both and Hinneburg 2015) over ``texts``, token lists in reading order -- for instance the ``docs`` the
        constructor was given; a token outside the dictionary keeps its position and matches nothing.  window = None takes the
        measure's usual width (``topics.DEFAULT_WINDOW``: 110 for c_v, 10 for the others).  The windows are counted on the device
        (llda_window_cooc); the texts are counted whole on every rank: no collective.  lam = a relevance in 0 .. 1: the coherence of
        the lists of ``label_words(n, lam, min_count)`` instead of the most frequent words."""
        import torch
        from . import topics
        if measure not in topics.DEFAULT_WINDOW:
            raise ValueError("measure must be 'c_v', 'c_uci' or 'c_npmi'")
        window = topics.DEFAULT_WINDOW[measure] if window is None else window
        sm = self._sampler
        sm.check_status()
        idx = sm.top_words(n)[0] if lam is None else self._label_words_device(n, lam, min_count)[0]
        tok_off, tok = topics.token_csr(texts, self.dicti.token2id)
        co = topics.window_cooccurrence(torch.from_numpy(tok_off).to(sm.device), torch.from_numpy(tok).to(sm.device), self.V, idx, window)
        return topics.window_coherence(co.cpu().numpy(), topics.window_count(tok_off, window), measure, listed=idx.cpu().numpy())

    # ---- test time (reference LabeledLDA.py:155-212), on the device ----
    def prep4test(self, doc, seed=None, stream_id=None):
        """start state (ids, freqs, z_dn, n_dk) of one held-out token list: LabeledLDA.py:155-177."""
        from .foldin import TEST_STREAM, fold_in
        tups = self.dicti.doc2bow(doc)
        r = fold_in(self.ph_hat, self.alpha, [tups], 0, 1, self.seed if seed is None else seed,
                    TEST_STREAM if stream_id is None else stream_id)
        ids, freqs = zip(*tups)
        return ids, freqs, list(r["z"][0]), r["n_dk"][0]

    def run_test(self, newdocs, it, thinning, seed=None, stream_id=None, candidates=None):
        """thinned average of n_dk / sum(n_dk) over ``it`` fold-in sweeps per held-out document
        (LabeledLDA.py:179-212); all documents and sweeps in one llda_foldin launch.
        ``candidates`` (new; one list of label strings per document): the sampler runs over 'root' plus those labels only
        (llda_foldin_sparse; at most 32 per document, root included) and the (D, K) loads are +0.0 outside the lists.
        With every label as a candidate the loads are those of the default, bit for bit."""
        from .foldin import TEST_STREAM, fold_in
        if candidates is not None:
            from . import attribution
            th_s, lab_off, lab = self._test_slots_device(newdocs, it, thinning, seed, stream_id, candidates, None)
            return attribution.scatter_slots(th_s, lab_off, lab, self.K).cpu().numpy()
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat     # still on the device after training
        r = fold_in(ph, self.alpha, tups, it, thinning, self.seed if seed is None else seed,
                    TEST_STREAM if stream_id is None else stream_id)
        return r["th_hat"]

    # ---- predictions ----
    def get_pred(self, single_th, n=5):
        names = np.array(list(self.labelmap.keys()))
        order = np.argsort(-single_th)[:n]
        loads = np.flip(np.sort(single_th), axis=0)[:n]
        return list(zip(names[order], loads))

    def get_preds(self, all_th, n=5):
        return [self.get_pred(all_th[d, :], n) for d in range(all_th.shape[0])]

    # ---- predictions and metrics without the (D, K) download (new; the methods above are the reference's) ----
    def _test_theta_device(self, newdocs, it, thinning, seed, stream_id):
        from .foldin import TEST_STREAM, fold_in
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        return fold_in(ph, self.alpha, tups, it, thinning, self.seed if seed is None else seed,
                       TEST_STREAM if stream_id is None else stream_id, keep_device=True)

    def _test_phi_t_device(self):
        """ph_hat as ``run_test`` reads it, word-major (V, K) on the device"""
        import torch
        ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        if not isinstance(ph, torch.Tensor):
            ph = torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float64))
        return ph.to(device=self._attr_device(), dtype=torch.float64).t().contiguous()

    def shortlist_cols(self, tups, m, phi_t=None):
        """The shortlist of every doc2bow list: column 0 ('root') plus the m <= 16 labels with the most credit after ONE attribution
        pass from uniform loads (llda_attribute with no EM step, then llda_rank_labels without the root; equal credit by label
        index).  Columns ascending.  Nothing of size (D, K) comes to the host."""
        from . import attribution, ranking
        if not 1 <= int(m) <= ranking.MAX_TOP_N:
            raise ValueError("shortlist must be in 1 .. %d" % ranking.MAX_TOP_N)
        self._check_tups(tups)
        D = len(tups)
        if D == 0:
            return []
        credit = self._fold_in_em_device(tups, attribution.uniform_start(None, D, self.K), 0, want=("credit",),
                                         phi_t=self._test_phi_t_device() if phi_t is None else phi_t)["credit"]
        ranked = ranking.rank_labels(credit, None, first=1, top_n=int(m)).host()["top_idx"]
        return [[0] + sorted(int(k) for k in row if int(k) >= 1) for row in ranked]

    def _test_slots_device(self, newdocs, it, thinning, seed, stream_id, candidates, shortlist):
        """the fold-in on label lists: (th_s [NL] on the device, lab_off, lab on the host).  candidates: label strings per document;
        shortlist: m, the lists are built on the device (``shortlist_cols``)."""
        from . import attribution, docmodel
        from .foldin import TEST_STREAM, fold_in_sparse
        if candidates is not None and shortlist is not None:
            raise ValueError("candidates and shortlist exclude one another")
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        phi_t = self._test_phi_t_device()
        if candidates is not None:
            cols = attribution.explain_label_cols(self.labelmap, len(tups), labels=candidates)
        else:
            cols = self.shortlist_cols(tups, shortlist, phi_t=phi_t)
        lab_off, lab = docmodel.label_csr(cols, K=self.K)
        th_s, _, _ = fold_in_sparse(phi_t, self.alpha, tups, lab_off, lab, it, thinning, self.seed if seed is None else seed,
                                    TEST_STREAM if stream_id is None else stream_id, keep_device=True)
        return th_s, lab_off, lab

    def predict(self, newdocs, it, thinning, n=5, seed=None, stream_id=None, candidates=None, shortlist=None):
        """``get_preds(run_test(newdocs, it, thinning), n)`` with the ranking on the device (llda_rank_labels): the fold-in's loads
        never leave it, only the n (label, load) pairs per document do.  n <= 16.  Equal loads are ordered by label index
        ascending (``get_pred``'s argsort leaves their order open); the loads themselves are the same bits.
        ``candidates`` (label strings per document) or ``shortlist`` = m in 1 .. 16 (new): the sampler runs on
        'root' plus the candidates, or plus the m labels one attribution pass credits most (``shortlist_cols``), through
        llda_foldin_sparse.  The slots are ranked on a padded (D, longest list) matrix, the same tie rule; no (D, K) matrix is formed,
        and a document gets min(n, its list) pairs."""
        from . import ranking
        if candidates is not None or shortlist is not None:
            import torch
            th_s, lab_off, lab = self._test_slots_device(newdocs, it, thinning, seed, stream_id, candidates, shortlist)
            D, counts = len(lab_off) - 1, np.diff(lab_off)
            width = int(counts.max()) if D else 0
            dev = th_s.device
            rows = torch.from_numpy(np.repeat(np.arange(D, dtype=np.int64), counts)).to(dev)
            at = torch.from_numpy(np.arange(int(lab_off[-1]), dtype=np.int64) - np.repeat(lab_off[:-1], counts)).to(dev)
            pad = torch.full((D, width), float("-inf"), dtype=torch.float64, device=dev)
            pad[rows, at] = th_s
            val, order = torch.sort(pad, dim=1, descending=True, stable=True)        # (slots ascend in label id: ties by label index)
            m = min(int(n), width)
            val, order = val[:, :m].cpu().numpy(), order[:, :m].cpu().numpy()
            names = np.array(list(self.labelmap.keys()))
            return [list(zip(names[lab[lab_off[d] + order[d, :min(m, counts[d])]]], val[d, :min(m, counts[d])])) for d in range(D)]
        th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        r = ranking.rank_labels(th, None, first=0, top_n=n).host()
        names = np.array(list(self.labelmap.keys()))
        m = min(n, self.K)
        return [list(zip(names[idx[:m]], val[:m])) for idx, val in zip(r["top_idx"], r["top_val"])]

    def score_test(self, newdocs, labels, it, thinning, seed=None, stream_id=None, candidates=None, shortlist=None):
        """Fold ``newdocs`` in and score the loads against ``labels`` (one list of label strings per document, what
        ``evaluate.binary_yreal`` takes) by the rules of the harness's report: dict(auc, one_error, two_error, f1, kept, dropped)
        (``ranking.metrics``).  Per document 28 bytes come back to the host.  ``candidates`` / ``shortlist``: as in ``predict``; the
        loads are +0.0 outside the lists."""
        from . import ranking
        from .evaluate import binary_yreal
        if candidates is not None or shortlist is not None:
            from . import attribution
            th_s, lab_off, lab = self._test_slots_device(newdocs, it, thinning, seed, stream_id, candidates, shortlist)
            th = attribution.scatter_slots(th_s, lab_off, lab, self.K)
        else:
            th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        return ranking.metrics(ranking.rank_labels(th, binary_yreal(labels, self.labelmap), first=1, top_n=0))

    # ---- held-out perplexity by document completion (new; heldout.py) ----
    def heldout_perplexity(self, newdocs, it, thinning, weighted=True, seed=None, stream_id=None, scored_docs=None, labels=None):
        """How well the trained model predicts unseen text: dict(perplexity, loglik, tokens, documents, skipped).
        Every held-out token list goes through ``dicti.doc2bow``; its sites 0, 2, 4, ... are folded in exactly as ``run_test`` folds
        documents in (same seed and stream conventions, document ids 0, 1, ... over the documents that are kept), the loads are
        smoothed with the observed tokens W_d -- theta = (W_d th + alpha) / (W_d + K alpha) -- and the sites 1, 3, 5, ... are scored:
        perplexity = exp(-sum f log(theta_d . ph_hat[:, w]) / sum f).  ``scored_docs`` (token lists, one per document): ``newdocs``
        are observed whole and these are scored instead of the parity split.  weighted=False counts every scored site once, the
        convention of ``perplexity()`` (W_d stays the observed tokens).  Documents without an in-vocabulary word to observe are
        dropped and counted as ``skipped``; a document with nothing to score contributes no tokens.  perplexity is inf when a scored
        site has no finite positive probability, nan when no token was scored.
        ``ph_hat`` and the loads stay on the device (llda_foldin, llda_heldout_loglik); 32 bytes per document come back.  The
        documents are scored whole on every rank: no collective.
        ``labels`` (new; one list of label strings per document): the label-conditioned figure by sampling.  The observed halves
        are folded in over 'root' plus the document's own labels (llda_foldin_sparse; at most 32 per document), the loads are
        smoothed per slot with L_d in K's place (``heldout.smooth_slots``) and scored by ``heldout.loglik_sparse``; split, skip rules,
        ids and streams are the default's."""
        import torch
        from . import heldout
        from .foldin import TEST_STREAM, fold_in
        if labels is not None and len(labels) != len(newdocs):
            raise ValueError("labels must hold one list per document of newdocs")
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        if scored_docs is None:
            observed, scored = heldout.completion_split(tups)
        else:
            if len(scored_docs) != len(tups):
                raise ValueError("scored_docs must hold one token list per document of newdocs")
            observed, scored = tups, [self.dicti.doc2bow(x) for x in scored_docs]
        keep = [d for d, t in enumerate(observed) if t]
        skipped = len(tups) - len(keep)
        if not keep:
            return dict(perplexity=float("nan"), loglik=0.0, tokens=0, documents=0, skipped=skipped)
        observed, scored = [observed[d] for d in keep], [scored[d] for d in keep]
        if labels is not None:
            from . import attribution, docmodel
            from .foldin import fold_in_sparse
            cols = attribution.explain_label_cols(self.labelmap, len(keep), labels=[labels[d] for d in keep])
            lab_off, lab = docmodel.label_csr(cols, K=self.K)
            phi_t = self._test_phi_t_device()
            th_s, _, _ = fold_in_sparse(phi_t, self.alpha, observed, lab_off, lab, it, thinning, self.seed if seed is None else seed,
                                        TEST_STREAM if stream_id is None else stream_id, keep_device=True)
            w_obs = torch.from_numpy(heldout.observed_tokens(observed)).to(th_s.device)
            theta_s = heldout.smooth_slots(th_s, w_obs, lab_off, float(self.alpha))
            s_off, s_word, s_freq = csr_from_doc_tups(scored)
            r = heldout.perplexity_from(*heldout.loglik_sparse(theta_s, phi_t, s_off, s_word, s_freq, lab_off, lab, weighted=weighted))
            return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=skipped)
        ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        th = fold_in(ph, self.alpha, observed, it, thinning, self.seed if seed is None else seed,
                     TEST_STREAM if stream_id is None else stream_id, keep_device=True)
        dev = th.device
        w_obs = torch.from_numpy(heldout.observed_tokens(observed)).to(dev)
        theta = heldout.smooth_theta(th, w_obs, float(self.alpha))
        ph_dev = ph.to(device=dev, dtype=torch.float64) if isinstance(ph, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float64)).to(dev)
        doc_off, word, freq = csr_from_doc_tups(scored)
        r = heldout.perplexity_from(*heldout.loglik(theta, ph_dev.t().contiguous(), doc_off, word, freq, weighted=weighted))
        return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=skipped)

    def heldout_perplexity_em(self, newdocs, iters=50, labels=None, sparse=False, weighted=True, scored_docs=None):
        """Document completion without random numbers, the deterministic sibling of ``heldout_perplexity``: the same split
        (``heldout.completion_split``, or ``scored_docs``) and skip rules, the observed halves folded in by ``iters`` EM steps as
        ``fold_in_em`` does (``labels``: over 'root' plus the document's own labels; sparse=True, with ``labels``: through the
        sparse-label kernels), the loads smoothed with the observed tokens W_d and the scored halves scored on the device.
        Without labels theta = (W_d th + alpha) / (W_d + K alpha); with labels the label count L_d (root included) takes K's place
        on the allowed columns and theta is 0 elsewhere.  sparse=True keeps the loads per slot from the fold-in to the score
        (llda_attribute_sparse, llda_heldout_loglik_sparse): no (D, K) matrix is formed, at most 32 labels per document, and the
        figures equal the default's bit for bit where every label set is a prefix 0 .. L - 1.
        Returns dict(perplexity, loglik, tokens, documents, skipped).  The same call gives the same bits every time."""
        import torch
        from . import attribution, docmodel, heldout
        if sparse and labels is None:
            raise ValueError("sparse=True wants the label sets: labels must be given")
        if labels is not None and len(labels) != len(newdocs):
            raise ValueError("labels must hold one list per document of newdocs")
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        if scored_docs is None:
            observed, scored = heldout.completion_split(tups)
        else:
            if len(scored_docs) != len(tups):
                raise ValueError("scored_docs must hold one token list per document of newdocs")
            observed, scored = tups, [self.dicti.doc2bow(x) for x in scored_docs]
        keep = [d for d, t in enumerate(observed) if t]
        skipped = len(tups) - len(keep)
        if not keep:
            return dict(perplexity=float("nan"), loglik=0.0, tokens=0, documents=0, skipped=skipped)
        observed, scored = [observed[d] for d in keep], [scored[d] for d in keep]
        cols = None if labels is None else attribution.explain_label_cols(self.labelmap, len(keep), labels=[labels[d] for d in keep])
        start = attribution.uniform_start(cols, len(keep), self.K)
        dev = self._attr_device()
        phi_t = self._phi_t_device()
        alpha = float(self.alpha)
        w_obs = torch.from_numpy(heldout.observed_tokens(observed)).to(dev)
        o_off, o_word, o_freq = csr_from_doc_tups(observed)
        s_off, s_word, s_freq = csr_from_doc_tups(scored)
        if sparse:
            lab_off, lab = docmodel.label_csr(cols, K=self.K)
            th0 = attribution.gather_slots(torch.from_numpy(start).to(dev), lab_off, lab)
            th = attribution.attribute_sparse(th0, phi_t, o_off, o_word, o_freq, lab_off, lab, iters=iters, alpha=alpha, top_m=0,
                                              want=("theta",))["theta"]
            theta_s = heldout.smooth_slots(th, w_obs, lab_off, alpha)
            out = heldout.loglik_sparse(theta_s, phi_t, s_off, s_word, s_freq, lab_off, lab, weighted=weighted)
        else:
            th = self._fold_in_em_device(observed, start, iters, phi_t=phi_t)["theta"]
            theta = heldout.smooth_theta(th, w_obs, alpha) if labels is None else \
                heldout.smooth_theta_labels(th, w_obs, torch.from_numpy(start != 0.0).to(dev), alpha)
            out = heldout.loglik(theta, phi_t, s_off, s_word, s_freq, weighted=weighted)
        r = heldout.perplexity_from(*out)
        return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=skipped)

    # ---- left-to-right held-out likelihood (new; leftright.py) ----
    def left_to_right(self, newdocs, particles=10, labels=None, seed=None, stream_id=None, max_tokens=None, sparse=False):
        """An estimate of p(w_d | ph_hat, alpha) for every held-out token list by the left-to-right particle sampler of Wallach et al.
        (2009): dict(perplexity, loglik, tokens, documents, skipped, bad).  The token lists keep the text's own order; tokens the
        dictionary does not know are dropped; ``max_tokens`` scores only the first tokens of every document.  Documents with no
        token left, or with more than 4096 after truncation, are counted in ``skipped``; the others carry the ids 0, 1, ...
        ``labels`` (one list of label strings per document): the topics of every document are restricted to its labels and
        'root' -- the figure is then p(w_d | labels_d).  perplexity = exp(-loglik / tokens), inf when a token had no finite positive
        probability (``bad`` counts them).  ``ph_hat`` stays on the device (llda_left_to_right); 32 bytes per document come back.
        sparse=True (with ``labels``; at most 32 per document, root included -- ValueError beyond): through
        llda_left_to_right_sparse, where a draw reads the document's own columns of phi only.  It works for every K the model can
        have (the default raises above K = 1024) and gives the default's figure exactly where every label set is a prefix
        0 .. L - 1; elsewhere the sums pair by slot and the estimate differs.
        Every rank scores the documents whole: no collective."""
        import torch
        from . import heldout, leftright
        if labels is not None and len(labels) != len(newdocs):
            raise ValueError("labels must hold one list per document of newdocs")
        if sparse and labels is None:
            raise ValueError("sparse=True wants the label sets: labels must be given")
        t2i = self.dicti.token2id
        lists, keep = leftright.prepare_tokens([[t2i[x] for x in doc if x in t2i] for doc in newdocs], max_tokens)
        skipped = len(newdocs) - len(keep)
        if not keep:
            return dict(perplexity=float("nan"), loglik=0.0, tokens=0, documents=0, skipped=skipped, bad=0)
        sets = None
        if sparse:
            from . import attribution, docmodel
            sets = docmodel.label_csr(attribution.explain_label_cols(self.labelmap, len(keep), labels=[labels[d] for d in keep]), K=self.K)
            docmodel.label_sets(sets[0], sets[1], len(keep), self.K)        # (more than 32 labels in a document: ValueError, before any launch)
        allowed = None if labels is None or sparse else leftright.allowed_matrix([labels[d] for d in keep], self.labelmap, self.K)
        ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        dev = self._attr_device()
        ph_dev = ph.to(device=dev, dtype=torch.float64) if isinstance(ph, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float64)).to(dev)
        doc_off, word = leftright.tokens_csr(lists)
        seed, stream_id = self.seed if seed is None else seed, leftright.LR_STREAM if stream_id is None else stream_id
        if sparse:
            out = leftright.loglik_sparse(ph_dev.t().contiguous(), doc_off, word, sets[0], sets[1], float(self.alpha), particles, seed, stream_id)
        else:
            out = leftright.loglik(ph_dev.t().contiguous(), doc_off, word, float(self.alpha), particles, seed, stream_id, allowed=allowed)
        r = heldout.perplexity_from(*out)
        return dict(perplexity=r["perplexity"], loglik=r["loglik"], tokens=r["tokens"], documents=len(keep), skipped=skipped,
                    bad=r["bad"])

    # ---- credit attribution and the EM fold-in (new; attribution.py) ----
    def _attr_device(self):
        import torch
        return self._sampler.device if self.__dict__.get("_sampler") is not None else torch.device("cuda:%d" % torch.cuda.current_device())

    def _phi_t_device(self):
        """ph_hat (get_phi() before any thinning read-out) word-major on the device"""
        import torch
        dev = self._attr_device()
        if not self.cur_perplx:
            ph = self._sampler.phi()
        else:
            ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        if not isinstance(ph, torch.Tensor):
            ph = torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float64))
        return ph.to(device=dev, dtype=torch.float64).t().contiguous()

    def word_credit(self, top_m=1):
        """Credit attribution on the training corpus: for every site of every document its top_m <= 4 best labels with the word's
        posterior share per label, theta_k phi_k[w] / sum, against ``th_hat`` and ``ph_hat`` (``get_theta()`` and ``get_phi()`` before
        any thinning read-out).  Returns dict(labels=[(len(doc), top_m) int32 arrays, -1 = padding], shares=[(len(doc), top_m) float64
        arrays], credit=(D, K) float64: the tokens credited to every label).  th_hat is 0 outside a document's labels, so nothing is
        credited there.  One llda_attribute launch with no EM step.  COLLECTIVE with several ranks (it reads th_hat)."""
        import torch
        from . import attribution
        if not 1 <= int(top_m) <= attribution.MAX_TOP:
            raise ValueError("top_m must be in 1 .. %d" % attribution.MAX_TOP)
        dev = self._attr_device()
        phi_t = self._phi_t_device()
        if not self.cur_perplx:
            th = self.get_theta()
        elif self._th_hat.dev is not None and _world_size() == 1:
            th = self._th_hat.dev
        else:
            th = self.th_hat
        if not isinstance(th, torch.Tensor):
            th = torch.from_numpy(np.ascontiguousarray(th, dtype=np.float64))
        doc_off, word, freq = csr_from_doc_tups(self.doc_tups)
        r = attribution.attribute(th.to(dev), phi_t, doc_off, word, freq, iters=0, top_m=top_m, want=("credit", "sites"))
        idx, val = attribution.spans(doc_off, r["site_idx"].cpu().numpy(), r["site_val"].cpu().numpy())
        return dict(labels=idx, shares=val, credit=r["credit"].cpu().numpy())

    @staticmethod
    def _check_tups(tups):
        """a document with no in-vocabulary word raises, as in ``run_test``"""
        for t in tups:
            if not t:
                raise ValueError("not enough values to unpack: a document has no in-vocabulary word")

    def _em_start(self, tups, labels):
        from . import attribution
        self._check_tups(tups)
        cols = None if labels is None else attribution.explain_label_cols(self.labelmap, len(tups), labels=labels)
        return attribution.uniform_start(cols, len(tups), self.K)

    def _fold_in_em_device(self, tups, start, iters, top_m=0, want=("theta",), phi_t=None):
        """``iters`` EM steps from the rows ``start`` (numpy (D, K)); phi_t: ``_phi_t_device()`` where the caller has it already"""
        import torch
        from . import attribution
        doc_off, word, freq = csr_from_doc_tups(tups)
        th0 = torch.from_numpy(start).to(self._attr_device())
        return attribution.attribute(th0, self._phi_t_device() if phi_t is None else phi_t, doc_off, word, freq, iters=iters, alpha=float(self.alpha),
                                     top_m=top_m, want=want)

    def fold_in_em(self, newdocs, iters=50, labels=None, sparse=False):
        """Fold unseen documents in by EM: (D, K) float64 loads after ``iters`` steps of theta_k = (credit_k + alpha) / sum from the
        uniform start over all K labels, or -- with ``labels``, one list of label strings per document -- over 'root' plus the
        document's labels.  No random numbers: the same document gets the same loads on every call.  A document with no
        in-vocabulary word raises, as in ``run_test``.  The documents are independent: no collective.  sparse=True (with
        ``labels``; at most 32 per document, root included): through ``attribution.attribute_sparse``, which reads a document's
        own columns of phi only; the loads differ from the default's in their last bits."""
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        start = self._em_start(tups, labels)
        if not tups:
            return start
        if sparse:
            import torch
            from . import attribution, docmodel
            if labels is None:
                raise ValueError("sparse=True wants the label sets: labels must be given")
            lab_off, lab = docmodel.label_csr(attribution.explain_label_cols(self.labelmap, len(tups), labels=labels), K=self.K)
            doc_off, word, freq = csr_from_doc_tups(tups)
            th0 = attribution.gather_slots(torch.from_numpy(start).to(self._attr_device()), lab_off, lab)
            r = attribution.attribute_sparse(th0, self._phi_t_device(), doc_off, word, freq, lab_off, lab, iters=iters, alpha=float(self.alpha),
                                             top_m=0, want=("theta",))
            return attribution.scatter_slots(r["theta"], lab_off, lab, self.K).cpu().numpy()
        return self._fold_in_em_device(tups, start, iters)["theta"].cpu().numpy()

    def predict_em(self, newdocs, iters=50, n=5):
        """``predict`` on the loads of ``fold_in_em``: the n <= 16 best (label, load) pairs of every document, ranked on the device."""
        from . import ranking
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        if not tups:
            return []
        th = self._fold_in_em_device(tups, self._em_start(tups, None), iters)["theta"]
        r = ranking.rank_labels(th, None, first=0, top_n=n).host()
        names = np.array(list(self.labelmap.keys()))
        m = min(n, self.K)
        return [list(zip(names[idx[:m]], val[:m])) for idx, val in zip(r["top_idx"], r["top_val"])]

    def explain(self, newdocs, labels=None, iters=50, n=3):
        """Why a label: for every unseen document ([(token, f, [(label, share), ...])], {label: credited tokens}).  The label set is
        'root' plus the given ``labels`` (one list of label strings per document) or 'root' plus the n <= 3 best non-root labels of
        ``predict_em``; the loads are fitted on that set (``iters`` EM steps from its uniform start) and every word is attributed
        against them with its min(4, set size) best labels, shares descending.  With at most four labels in the set a word's shares
        sum to 1."""
        from . import attribution, ranking
        tups = [self.dicti.doc2bow(x) for x in newdocs]
        D = len(tups)
        if labels is None and not 1 <= int(n) <= 3:
            raise ValueError("n must be in 1 .. 3 (at most four labels per site: root and three)")
        if D == 0:
            return []
        self._check_tups(tups)
        phi_t = self._phi_t_device()
        if labels is not None:
            cols = attribution.explain_label_cols(self.labelmap, D, labels=labels)
        else:
            th = self._fold_in_em_device(tups, attribution.uniform_start(None, D, self.K), iters, phi_t=phi_t)["theta"]
            ranked = ranking.rank_labels(th, None, first=1, top_n=n).host()["top_idx"]
            cols = attribution.explain_label_cols(self.labelmap, D, ranked=ranked, n=n)
        top_m = min(attribution.MAX_TOP, max(len(c) for c in cols))
        r = self._fold_in_em_device(tups, attribution.uniform_start(cols, D, self.K), iters, top_m=top_m, want=("credit", "sites"),
                                    phi_t=phi_t)
        return attribution.explanations(tups, r["site_idx"].cpu().numpy(), r["site_val"].cpu().numpy(), r["credit"].cpu().numpy(),
                                        list(self.labelmap.keys()), self.v_to_w)

    # ---- nearest rows on the device (new; similar.py) ----
    def _similar_corpus(self, measure):
        """the affinity rows of this rank's training documents: ``th_hat`` while it is on the device, else the current theta"""
        from . import similar
        th = self._th_hat.dev if self._th_hat.dev is not None else self._sampler.theta()
        return similar.affinity_rows(th, measure)

    def _neighbours(self, queries, corpus, n, exclude=None):
        """(ids (Q, n) int64, affinity (Q, n) float64) of the affinity rows ``queries`` (the same on every rank) against this rank's
        ``corpus`` rows; with several ranks the per-rank lists are gathered and merged: 16 * Q * n bytes per rank travel."""
        from . import similar
        idx, val, _ = similar.nearest_rows(queries, corpus, n, exclude=exclude, row_base=int(self._bounds[_rank()]))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        if _world_size() > 1:
            import torch.distributed as dist
            parts = [None] * _world_size()
            dist.all_gather_object(parts, (idx, val))
            idx, val = similar.merge_lists([p[0] for p in parts], [p[1] for p in parts], n)
        return idx, val

    def similar_documents(self, newdocs=None, doc_ids=None, n=10, it=500, thinning=25, measure="hellinger", seed=None, stream_id=None):
        """The n <= 16 training documents most like each query: (ids (Q, n) int64, affinity (Q, n) float64), best first, equal
        affinities by document id ascending, padded with -1 / 0.0 when the corpus is smaller.  Exactly one of ``newdocs`` (held-out
        token lists, folded in as ``predict`` folds them in) and ``doc_ids`` (training documents, which never return themselves).
        measure = "hellinger": the Bhattacharyya coefficient sum_k sqrt(theta_q[k] theta_d[k]) in [0, 1], Hellinger distance =
        sqrt(1 - affinity); "cosine"; "dot".  The corpus is ``th_hat`` while the thinning read-outs hold it on the device, else the
        current ``theta``; neither it nor the Q x D affinities leave the device (llda_nearest_rows).  COLLECTIVE with several ranks."""
        import torch
        from . import similar
        if (newdocs is None) == (doc_ids is None):
            raise ValueError("give exactly one of newdocs and doc_ids")
        similar._check_n(n)
        if measure not in similar.MEASURES:
            raise ValueError("measure must be one of %s" % (similar.MEASURES,))
        self._sampler.check_status()
        corpus = self._similar_corpus(measure)
        if doc_ids is not None:
            ids = np.asarray(doc_ids, dtype=np.int64).reshape(-1)
            if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.D):
                raise ValueError("doc_ids must be in 0 .. %d" % (self.D - 1))
            lo, hi = int(self._bounds[_rank()]), int(self._bounds[_rank() + 1])
            mine = (ids >= lo) & (ids < hi)
            queries = torch.zeros((ids.shape[0], self.K), dtype=torch.float64, device=corpus.device)
            if mine.any():
                queries[torch.from_numpy(np.flatnonzero(mine)).to(corpus.device)] = corpus[torch.from_numpy(ids[mine] - lo).to(corpus.device)]
            if _world_size() > 1:
                import torch.distributed as dist
                dist.all_reduce(queries)                  # (every rank but the owner adds zeros: exact)
            return self._neighbours(queries, corpus, n, exclude=ids)
        if len(newdocs) == 0:
            return np.zeros((0, n), dtype=np.int64), np.zeros((0, n), dtype=np.float64)
        th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        return self._neighbours(similar.affinity_rows(th.to(corpus.device), measure), corpus, n)

    def similar_labels(self, n=5, measure="hellinger"):
        """For every label its n <= 16 nearest other labels by word distribution: [(label, [(other label, affinity), ...]), ...] in
        label order, best first.  The rows are ``ph_hat`` (``get_phi()`` before any thinning read-out), the inner length is V, every
        label leaves itself out.  n_k_v is replicated: no collective."""
        import torch
        from . import similar
        similar._check_n(n)
        self._sampler.check_status()
        dev = self._attr_device()
        if not self.cur_perplx:
            ph = self._sampler.phi()
        else:
            ph = self._ph_hat.dev if self._ph_hat.dev is not None else self.ph_hat
        if not isinstance(ph, torch.Tensor):
            ph = torch.from_numpy(np.ascontiguousarray(ph, dtype=np.float64))
        rows = similar.affinity_rows(ph.to(device=dev, dtype=torch.float64), measure)
        idx, val, _ = similar.nearest_rows(rows, rows, n, exclude=np.arange(self.K, dtype=np.int64))
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        names = list(self.labelmap.keys())
        return [(names[k], [(names[int(j)], float(v)) for j, v in zip(idx[k], val[k]) if j >= 0]) for k in range(self.K)]

    def _knn_votes(self, newdocs, it, thinning, k, measure, seed, stream_id):
        from . import similar
        similar._check_n(k)
        idx, val = self.similar_documents(newdocs=newdocs, n=k, it=it, thinning=thinning, measure=measure, seed=seed, stream_id=stream_id)
        return similar.knn_votes(idx, val, self.labs, k)

    def predict_knn(self, newdocs, it, thinning, k=10, n=5, measure="hellinger", seed=None, stream_id=None):
        """``predict`` by the k <= 16 nearest training documents instead of the document's own loads: every label's score is the sum
        of the affinities of the neighbours that carry it (``similar.knn_votes`` against ``labs``), ranked on the device; what
        ``predict`` returns.  COLLECTIVE with several ranks."""
        from . import ranking
        if len(newdocs) == 0:
            return []
        votes = self._knn_votes(newdocs, it, thinning, k, measure, seed, stream_id)
        r = ranking.rank_labels(votes, None, first=0, top_n=n).host()
        names = np.array(list(self.labelmap.keys()))
        m = min(n, self.K)
        return [list(zip(names[idx[:m]], val[:m])) for idx, val in zip(r["top_idx"], r["top_val"])]

    def score_test_knn(self, newdocs, labels, it, thinning, k=10, measure="hellinger", seed=None, stream_id=None):
        """``score_test`` for the votes of the k <= 16 nearest training documents: the baseline beside the model's own figures, the
        same dict through ``ranking.metrics``.  COLLECTIVE with several ranks."""
        from . import ranking
        from .evaluate import binary_yreal
        votes = self._knn_votes(newdocs, it, thinning, k, measure, seed, stream_id)
        return ranking.metrics(ranking.rank_labels(votes, binary_yreal(labels, self.labelmap), first=1, top_n=0))

    # ---- label-wise evaluation and tuned label sets (new; labelwise.py) ----
    def _label_result(self, newdocs, labels, it, thinning, seed, stream_id, order=False):
        from . import labelwise
        from .evaluate import binary_yreal
        th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        return labelwise.label_metrics(th, binary_yreal(labels, self.labelmap), first=1, order=order)

    def label_report(self, newdocs, labels, it, thinning, seed=None, stream_id=None):
        """Which labels does the model predict well?  Folds ``newdocs`` in as ``score_test`` does and ranks, for every label but
        'root', the documents by that label's load (llda_label_metrics): dict(table=[(name, support, auc, f1, threshold), ...] in
        label order, plus ``labelwise.macro``'s macro_auc, macro_f1, n_labels, skipped).  auc is the standard label-wise AUC (nan
        for a label that no or every document carries), f1 the best F1 any threshold reaches and threshold the load that reaches it.
        Every rank does the whole call: no collective."""
        from . import labelwise
        res = self._label_result(newdocs, labels, it, thinning, seed, stream_id)
        out = labelwise.macro(res)
        h = res.host()
        names = list(self.labelmap.keys())[1:]
        out["table"] = [(names[i], int(h["n_pos"][i]), float(h["auc"][i]), float(h["f1"][i]), float(h["thr"][i])) for i in range(len(names))]
        return out

    def tune_thresholds(self, valdocs, vallabels, it, thinning, seed=None, stream_id=None):
        """SCut: for every label the load threshold that maximises its F1 over the validation documents (folded in as ``score_test``
        folds them in).  Stores and returns ``self.label_thresholds``: K doubles, NaN -- never predicted -- for 'root' and for labels
        without a positive validation document.  Every rank does the whole call: no collective."""
        from . import labelwise
        self.label_thresholds = labelwise.thresholds(self._label_result(valdocs, vallabels, it, thinning, seed, stream_id))
        return self.label_thresholds

    def _tuned(self):
        thr = getattr(self, "label_thresholds", None)
        if thr is None:
            raise ValueError("no thresholds: call tune_thresholds(valdocs, vallabels, it, thinning) first")
        return thr

    def predict_sets(self, newdocs, it, thinning, at_least_one=True, seed=None, stream_id=None):
        """One list of label names per document, in label-index order: the labels whose load reaches their tuned threshold
        (llda_label_sets) instead of always n labels.  at_least_one: a document that reaches none gets its best label among those
        with a threshold.  Only the bit masks come back to the host."""
        from . import labelwise
        thr = self._tuned()
        if len(newdocs) == 0:
            return []
        th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        names = np.array(list(self.labelmap.keys()))
        return [list(names[row]) for row in labelwise.label_sets(th, thr, None, first=1, at_least_one=at_least_one).sets()]

    def score_test_sets(self, newdocs, labels, it, thinning, at_least_one=True, seed=None, stream_id=None):
        """Fold ``newdocs`` in, predict label sets with the tuned thresholds and score them against ``labels``:
        dict(micro_f1, macro_f1, example_f1, labels_scored, docs_scored) (``labelwise.set_scores``)."""
        from . import labelwise
        from .evaluate import binary_yreal
        thr = self._tuned()
        th = self._test_theta_device(newdocs, it, thinning, seed, stream_id)
        return dict(labelwise.label_sets(th, thr, binary_yreal(labels, self.labelmap), first=1, at_least_one=at_least_one).scores())

    # ---- pickling: pull the device state to the host (evaluate_LabeledLDA.py:142-145 pickles the model)
    def __getstate__(self):
        self.ph_hat, self.th_hat                      # bring the running means to the host
        state = {k: v for k, v in self.__dict__.items() if k != "_sampler"}
        state["_host_state"] = dict(n_zk=self.n_zk, n_d_k=self.n_d_k, n_k_v=self.n_k_v,
                                    z=_gather_rows(self._sampler.z_topics()),
                                    sweeps_done=self._sampler.sweeps_done)
        return state

    def __setstate__(self, state):
        host = state.pop("_host_state")
        self.__dict__.update(state)
        doc_off, word, freq = csr_from_doc_tups(self.doc_tups)
        self._bounds = shard_documents(doc_off, _world_size())
        lo, hi = self._bounds[_rank()], self._bounds[_rank() + 1]
        s0, s1 = int(doc_off[lo]), int(doc_off[hi])
        counts = dict(n_d_k=host["n_d_k"][lo:hi], n_k_v=host["n_k_v"], n_zk=host["n_zk"])
        self._sampler = GibbsSampler(doc_off[lo:hi + 1] - doc_off[lo], word[s0:s1], freq[s0:s1], host["z"][s0:s1],
                                     self.K, self.V, self.alpha, self.beta, labs=self.labs[lo:hi], counts=counts,
                                     seed=self.seed, doc_base=lo)
        self._sampler.sweeps_done = host["sweeps_done"]


def split_data(f, d=2):
    """shuffle + 90/10 split: reference LabeledLDA.py:268-278 (the labelset list object is shared)."""
    a, b, c = load_corpus(f, d)
    zipped = list(zip(a, b))
    np.random.shuffle(zipped)
    a, b = zip(*zipped)
    split = int(len(a) * 0.9)
    return (a[:split], b[:split], c), (a[split:], b[split:], c)


def prune_dict(docs, lower=0.1, upper=0.9):
    dicti = _text.Dictionary(docs)
    dicti.filter_extremes(no_above=upper, no_below=lower * len(docs))
    return dicti


def train_it(traindata, it=30, s=3, al=0.001, be=0.001, l=0.05, u=0.95, em=0, em_sparse=False):
    """em = n > 0: fit by ``fit_em(n)`` in place of ``run_training(it, s)``; em_sparse: its sparse-label form"""
    a, b, c = traindata
    dicti = prune_dict(a, lower=l, upper=u)
    llda = LabeledLDA(a, b, c, dicti, al, be)
    if em > 0:
        llda.fit_em(em, sparse=True) if em_sparse else llda.fit_em(em)
    else:
        llda.run_training(it, s)
    return llda


def test_it(model, testdata, it=500, thinning=25, n=5):
    known = set(model.vocab)
    testdocs = [[x for x in doc if x in known] for doc in testdata[0]]
    th_hat = model.run_test(testdocs, it, thinning)
    preds = model.get_preds(th_hat, n)
    th_hat = [[round(x, 4) for x in single_th] for single_th in th_hat]
    return th_hat, preds
