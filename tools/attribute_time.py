"""time of llda_attribute alone (the kernel behind attribution.attribute / LabeledLDA.word_credit, fold_in_em, explain) on D documents
of N sites, words uniform over V, f = 1, theta with a handful of loads per document smoothed as heldout.smooth_theta leaves it.
Timed in ONE run, the variants taking turns repetition by repetition:

    (a) iters = 0, the credit only (no per-site output);
    (b) the same with the per-site outputs, top_m = 1 and top_m = 4;
    (c) iters = 10 (loads and credit), from which one EM step = ((c) - (a)) / 10;
    (d) llda_heldout_loglik on the same inputs -- it reads exactly the bytes (a) reads -- and the E-step as a chunked torch
        expression on the same device: t = theta[site_doc] * phi_t[word]; credit.index_add_(site_doc, t / t.sum(1)).

HIP events, a warm-up, the median of REPS repetitions, one process.  python tools/attribute_time.py [--out FILE] [D:K[:N[:V]] ...]
(default: 100 000 documents x 150 sites at K = 512, 128 and 32, V = 100 000); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native, heldout

REPS, WARMUP, BASE_REPS, CHUNK_BYTES, EM_ITERS = 9, 2, 3, 1 << 30, 10
ALPHA = 0.1
dev = torch.device("cuda", 0)


def inputs(D, K, N, V, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    th = torch.zeros((D, K), dtype=torch.float64, device=dev)            # fold-in output: a few loads per document that sum to one
    cols = torch.randint(0, K, (D, 6), device=dev, generator=g)
    th.scatter_(1, cols, torch.rand((D, 6), dtype=torch.float64, device=dev, generator=g) + 0.05)
    th /= th.sum(dim=1, keepdim=True)
    ph = torch.rand((K, V), dtype=torch.float64, device=dev, generator=g) ** 8 + 1e-6       # (K, V), rows sum to one, skewed
    ph /= ph.sum(dim=1, keepdim=True)
    word = torch.randint(0, V, (D * N,), device=dev, generator=g).to(torch.int32)
    freq = torch.ones((D * N,), dtype=torch.int32, device=dev)
    doc_off = torch.arange(D + 1, dtype=torch.int64, device=dev) * N
    w_obs = torch.full((D,), float(N), dtype=torch.float64, device=dev)
    return th, ph, doc_off, word, freq, w_obs


def torch_estep(theta, phi_t, word, N, K, credit):
    """the credit of every document, chunked so that a (sites, K) temporary stays below CHUNK_BYTES"""
    S = word.numel()
    step = max(N, CHUNK_BYTES // (8 * K) // N * N)
    credit.zero_()
    for lo in range(0, S, step):
        hi = min(S, lo + step)
        site_doc = torch.arange(lo, hi, device=dev) // N
        t = theta[site_doc] * phi_t[word[lo:hi].long()]
        credit.index_add_(0, site_doc, t / t.sum(1, keepdim=True))
    return credit


def timed_in_turns(fns, reps, warmup):
    """{name: milliseconds [reps]}: every repetition runs each of fns once, in order"""
    ev = {name: [] for name in fns}
    for i in range(warmup + reps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            if i >= warmup:
                ev[name].append((a, b))
    torch.cuda.synchronize()
    return {name: np.array([a.elapsed_time(b) for a, b in pairs]) for name, pairs in ev.items()}


def one_shape(D, K, N, V):
    th, ph, doc_off, word, freq, w_obs = inputs(D, K, N, V, 1000 + K)
    theta = heldout.smooth_theta(th, w_obs, ALPHA)
    phi_t = ph.t().contiguous()
    S = D * N
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    credit, credit_em, theta_em, mant = new((D, K)), new((D, K)), new((D, K)), new((D,))
    expo, tok, bad = (new((D,), torch.int64) for _ in range(3))
    idx1, val1, idx4, val4 = new((S, 1), torch.int32), new((S, 1)), new((S, 4), torch.int32), new((S, 4))

    def attr(**kw):
        return lambda: _native.attribute(doc_off, word, freq, theta, phi_t, D, V, K, **kw)

    fns = {"credit": attr(credit=credit, tok=tok, bad=bad),
           "top1": attr(top_m=1, credit=credit, site_idx=idx1, site_val=val1),
           "top4": attr(top_m=4, credit=credit, site_idx=idx4, site_val=val4),
           "em10": attr(iters=EM_ITERS, alpha=ALPHA, credit=credit_em, theta_out=theta_em),
           "heldout": lambda: _native.heldout_loglik(doc_off, word, freq, theta, phi_t, D, V, K, mant=mant, expo=expo, tok=tok, bad=bad)}
    ms = timed_in_turns(fns, REPS, WARMUP)
    base = new((D, K))
    b_ms = timed_in_turns({"torch": lambda: torch_estep(theta, phi_t, word, N, K, base)}, BASE_REPS, 1)["torch"]
    assert int(bad.sum()) == 0 and int(tok.sum()) == S
    err = float((credit - base).abs().max())
    assert err < 1e-9 * N, "kernel and torch expression disagree: %g" % err
    assert float((theta_em.sum(1) - 1).abs().max()) < 1e-12 and float((credit.sum(1) - N).abs().max()) < 1e-9
    assert bool((val4[:, 0] == val1[:, 0]).all()) and bool((idx4[:, 0] == idx1[:, 0]).all())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(D=D, K=K, N=N, V=V, sites=S, reps=REPS, credit_ms=med["credit"], top1_ms=med["top1"], top4_ms=med["top4"],
               em10_ms=med["em10"], em_step_ms=(med["em10"] - med["credit"]) / EM_ITERS, heldout_ms=med["heldout"],
               credit_over_heldout=med["credit"] / med["heldout"], top1_over_credit=med["top1"] / med["credit"],
               top4_over_credit=med["top4"] / med["credit"], torch_ms=float(np.median(b_ms)),
               speedup_over_torch=float(np.median(b_ms)) / med["credit"],
               ms_min={k: float(v.min()) for k, v in ms.items()}, ms_max={k: float(v.max()) for k, v in ms.items()},
               gather_bytes=S * K * 8, credit_gather_TBps=S * K * 8 / med["credit"] / 1e9, heldout_gather_TBps=S * K * 8 / med["heldout"] / 1e9,
               site_output_MB={"top1": S * 12 / 1e6, "top4": S * 48 / 1e6}, max_abs_diff_to_torch=err)
    del th, ph, theta, phi_t, word, freq, credit, credit_em, theta_em, idx1, val1, idx4, val4, base
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
    line = json.dumps(dict(tool="attribute_time", device=torch.cuda.get_device_name(0), shapes=[one_shape(*s) for s in shapes]))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
