"""time of llda_count_hist (the counts of counts behind GibbsSampler.count_histograms / LabeledLDA.optimize_priors) next to two
yardsticks, on the counts of a bench workload after five sweeps:

    (a) a device-to-device copy of the same buffer: what touching the bytes costs;
    (b) the torch-only composition that gives the same histogram (label masks expanded to a boolean matrix, the selected entries,
        torch.bincount), with its peak temporary memory;

and what one estimate of the priors costs next to one sweep: count_histograms() (both kernels, the copies to the host) and the host
iterations of priors.estimate, timed separately.  HIP events, a warm-up, the median of REPS repetitions, the three alternating in one
process.  python tools/count_hist_time.py [--out FILE] [workload[:documents] ...]   (default: synth2 = BASELINE configs[3], and its sparse variant
at the same million documents); prints one JSON line per result, and --out FILE keeps them all in one JSON file"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from lda_thesis_amd import _native, priors

REPS, WARMUP, N_BINS = 25, 3, 65536
dev = torch.device("cuda", 0)


def torch_hist(counts, masks, lay, n_bins):
    """the same histogram from torch ops alone -> (hist, values outside 0 .. n_bins-1)"""
    shifts = torch.arange(lay.T, device=dev, dtype=torch.int32)
    rank = torch.from_numpy(lay.draw_rank.astype(np.int64)).to(dev)              # position -> lane * T + slot
    bits = masks.reshape(-1, lay.G).to(torch.int32) & 0xFFFF
    allowed = (((bits.unsqueeze(-1) >> shifts) & 1) != 0).reshape(bits.shape[0], lay.KP)[:, rank]
    vals = counts[allowed.expand(counts.shape)]
    inside = (vals >= 0) & (vals < n_bins)
    return torch.bincount(vals[inside], minlength=n_bins), vals[~inside]


def median_ms(fns, reps=REPS, warmup=WARMUP):
    """{name: median ms} of the callables, alternating, one event pair per call"""
    ev = {n: [] for n in fns}
    for i in range(warmup + reps):
        for n, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            if i >= warmup:
                ev[n].append((a, b))
    torch.cuda.synchronize()
    return {n: float(np.median([a.elapsed_time(b) for a, b in v])) for n, v in ev.items()}


def one_input(what, counts, masks, per_row, s):
    lay = s.layout
    hist = torch.zeros((N_BINS,), dtype=torch.int64, device=dev)
    over = torch.zeros((1 << 16,), dtype=torch.int32, device=dev)
    over_n = torch.zeros((1,), dtype=torch.int64, device=dev)
    _native.count_hist(counts, s.K, masks, per_row, hist, over, over_n)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    h2, o2 = torch_hist(counts, masks, lay, N_BINS)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert torch.equal(hist, h2) and int(over_n.item()) == o2.numel(), "the torch composition and llda_count_hist disagree"
    del h2, o2
    dst = torch.empty_like(counts)

    def kernel():
        hist.zero_()
        over_n.zero_()
        _native.count_hist(counts, s.K, masks, per_row, hist, over, over_n)
    ms = median_ms({"count_hist": kernel, "copy": lambda: dst.copy_(counts), "torch": lambda: torch_hist(counts, masks, lay, N_BINS)})
    nbytes = counts.numel() * 4
    top = int(torch.nonzero(hist).max().item())
    out = dict(input=what, rows=int(counts.shape[0]), KP=lay.KP, bytes=nbytes, count_hist_ms=ms["count_hist"], copy_ms=ms["copy"],
               torch_ms=ms["torch"], torch_peak_temp_bytes=int(peak), ratio_to_copy=ms["count_hist"] / ms["copy"],
               speedup_over_torch=ms["torch"] / ms["count_hist"], count_hist_GBps=nbytes / ms["count_hist"] / 1e6,
               share_zero=float(hist[0].item()) / max(int(hist.sum().item()), 1), share_below_4=float(hist[:4].sum().item()) / max(int(hist.sum().item()), 1),
               largest_value_in_hist=top, over_n=int(over_n.item()))
    del dst
    torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def main():
    results, args, out_path = [], sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    for spec in (args or ["synth2", "synth2_sparse:1000000"]):
        name, _, docs = spec.partition(":")
        s, info = bench.build_sampler(name, dev, 0, 1, False, docs_total=int(docs or 0))
        for _ in range(5):
            s.sweep()
        s.check_status()
        results.append(one_input(spec + " n_dk", s.n_dk, s.lab_mask, True, s))
        if s.dense_mask:
            results.append(one_input(spec + " n_kw", s.n_kw, s._u16(s._all_topics_row()), False, s))
        # one estimate of the priors next to one sweep
        sweep = median_ms({"sweep": s.sweep}, reps=10, warmup=1)["sweep"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = s.count_histograms(N_BINS)
        t1 = time.perf_counter()
        pre = torch.zeros((s.S + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(s.freq, 0, out=pre[1:])
        tokens = (pre[s.doc_off[1:]] - pre[s.doc_off[:-1]]).cpu().numpy()
        allowed = np.full(s.D, s.K) if s.live_off is None else (s.live_off[1:] - s.live_off[:-1]).cpu().numpy()
        cls = priors.doc_classes(allowed, tokens)
        n_k = s.n_zk()
        t2 = time.perf_counter()
        est = priors.estimate(s.alpha, s.beta, hist_dk=h[0], over_dk=h[1], classes=cls, hist_kw=h[2], over_kw=h[3], n_k=n_k, V=s.V)
        t3 = time.perf_counter()
        out = dict(input=spec + " optimize_priors", sweep_ms=sweep, count_histograms_ms=(t1 - t0) * 1e3, host_estimate_ms=(t3 - t2) * 1e3,
                   iterations=est.iterations, converged=bool(est.converged), alpha=est.alpha, beta=est.beta, doc_classes=int(cls.shape[0]),
                   cost_in_sweeps=((t1 - t0) + (t3 - t2)) * 1e3 / sweep)
        print(json.dumps(out), flush=True)
        results.append(out)
        del s, info
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
