"""time of llda_credit_words and llda_phi_step (the kernels behind emfit.fit / LabeledLDA.fit_em) on the arrays of
tools/attribute_time.py -- D documents of N sites, f = 1, theta with a handful of loads per document, a skewed phi_t -- with the
words drawn uniformly over V ("uniform": every word has about D N / V sites, one chunk each) and from a power law ("skewed":
word = floor(V u^4), a few words with 10^5 sites and more, a tail with none).  Timed in ONE run, the variants taking turns
repetition by repetition:

    (a) llda_attribute(iters = 0, top_m = 0): the document side of the same E-step, the same row bytes (phi_t streamed, theta cached);
    (b) llda_credit_words with chunk = 1024, 4096, 16384 (theta streamed, phi_t cached);
    (c) llda_phi_step alone, and one EM iteration: llda_attribute(iters = 1), llda_credit_words(chunk = 4096), llda_phi_step;
    (d) for context the same expected counts as a chunked torch expression, cw.index_add_(0, word, t / t.sum(1)): floating-point
        atomics, so not bit-identical from run to run.

HIP events, a warm-up, the median of REPS repetitions, one process.  python tools/fit_em_time.py [--out FILE] [D:K[:N[:V]] ...]
(default: 100 000 documents x 150 sites at K = 512, 128 and 32, V = 100 000); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from attribute_time import ALPHA, BASE_REPS, CHUNK_BYTES, REPS, WARMUP, dev, inputs, timed_in_turns
from lda_thesis_amd import _native, emfit, heldout

CHUNKS = (1024, 4096, 16384)
BETA = 0.01


def torch_word_side(theta, phi_t, word, N, K, cw):
    S = word.numel()
    step = max(N, CHUNK_BYTES // (8 * K) // N * N)
    cw.zero_()
    for lo in range(0, S, step):
        hi = min(S, lo + step)
        w = word[lo:hi].long()
        t = theta[torch.arange(lo, hi, device=dev) // N] * phi_t[w]
        cw.index_add_(0, w, t / t.sum(1, keepdim=True))
    return cw


def one_case(D, K, N, V, skewed):
    th, ph, doc_off, word, freq, w_obs = inputs(D, K, N, V, 1000 + K)
    if skewed:
        g = torch.Generator(device=dev)
        g.manual_seed(77 + K)
        word = (torch.rand((D * N,), dtype=torch.float64, device=dev, generator=g) ** 4 * V).to(torch.int32).clamp_(max=V - 1)
    theta = heldout.smooth_theta(th, w_obs, ALPHA)
    phi_t = ph.t().contiguous()
    S = D * N
    word_off, site_doc, w_freq, _ = emfit.word_major(doc_off, word, freq, V, dev)
    runs = (word_off[1:] - word_off[:-1])
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    credit, theta_out, cw, phi_new = new((D, K)), new((D, K)), {c: new((V, K)) for c in CHUNKS}, new((V, K))
    tok_d, bad_d, tok_w, bad_w = (new((n,), torch.int64) for n in (D, D, V, V))
    scratch = new((max(_native.credit_words_scratch_bytes(V, S, K, min(CHUNKS)), _native.phi_step_scratch_bytes(V, K)),), torch.uint8)

    def words(chunk, th_in=theta):
        return lambda: _native.credit_words(word_off, site_doc, w_freq, th_in, phi_t, D, V, S, K, chunk, scratch, credit_w=cw[chunk],
                                            tok=tok_w, bad=bad_w)

    def iteration():
        _native.attribute(doc_off, word, freq, theta, phi_t, D, V, K, iters=1, alpha=ALPHA, theta_out=theta_out)
        words(4096, theta_out)()
        _native.phi_step(cw[4096], V, K, BETA, phi_new, scratch)

    fns = {"attribute": lambda: _native.attribute(doc_off, word, freq, theta, phi_t, D, V, K, credit=credit, tok=tok_d, bad=bad_d)}
    fns.update({"words_%d" % c: words(c) for c in CHUNKS})
    fns["phi_step"] = lambda: _native.phi_step(cw[1024], V, K, BETA, phi_new, scratch)
    ms = timed_in_turns(fns, REPS, WARMUP)
    assert int(bad_w.sum()) == 0 and int(tok_w.sum()) == S == int(tok_d.sum())
    for c in CHUNKS:                                                      # both sides add the same terms
        assert float((cw[c].sum(0) - credit.sum(0)).abs().max()) < 1e-9 * S
    assert float((phi_new.sum(0) - 1).abs().max()) < 1e-12
    it_ms = timed_in_turns({"iteration": iteration}, REPS, WARMUP)["iteration"]
    base = new((V, K))
    b_ms = timed_in_turns({"torch": lambda: torch_word_side(theta, phi_t, word, N, K, base)}, BASE_REPS, 1)["torch"]
    err = float((cw[1024] - base).abs().max())                             # (the iteration left another theta's credit in cw[4096])
    assert err < 1e-9 * float(runs.max()), "kernel and torch expression disagree: %g" % err
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(D=D, K=K, N=N, V=V, sites=S, words="skewed" if skewed else "uniform", longest_run=int(runs.max()),
               words_without_sites=int((runs == 0).sum()), chunks={c: int(((runs + c - 1) // c).sum()) for c in CHUNKS}, reps=REPS,
               ms=med, ms_min={k: float(v.min()) for k, v in ms.items()}, ms_max={k: float(v.max()) for k, v in ms.items()},
               words_over_attribute={c: med["words_%d" % c] / med["attribute"] for c in CHUNKS}, iteration_ms=float(np.median(it_ms)),
               torch_ms=float(np.median(b_ms)), gather_bytes=S * K * 8,
               gather_TBps={k: S * K * 8 / v / 1e9 for k, v in med.items() if k != "phi_step"}, max_abs_diff_to_torch=err)
    del th, ph, theta, phi_t, word, freq, credit, theta_out, cw, phi_new, base, scratch
    torch.cuda.empty_cache()
    return res


def main():
    args, out_path = sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    shapes = []
    for a in args:
        p = [int(x) for x in a.split(":")]
        shapes.append((p[0], p[1], p[2] if len(p) > 2 else 150, p[3] if len(p) > 3 else 100000))
    shapes = shapes or [(100000, 512, 150, 100000), (100000, 128, 150, 100000), (100000, 32, 150, 100000)]
    _native.lib()
    _native.require_device()
    cases = [one_case(*s, skewed=sk) for s in shapes for sk in (False, True)]
    line = json.dumps(dict(tool="fit_em_time", device=torch.cuda.get_device_name(0), cases=cases))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
