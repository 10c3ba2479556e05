"""time of llda_rank_labels alone (the ranking behind ranking.rank_labels / LabeledLDA.predict / score_test) on scores shaped like
fold-in output -- one to eight positive loads per document, ratios of small integers, the rest exact zeros -- next to

    (a) the floor of reading score and truth once: D * L * 9 bytes over the time;
    (b) the host path (evaluate.rates + macro_auc_roc + get_f1 + n_error(1) + n_error(2)) on a 400-document sample of the same
        rows, SCALED to D documents (labelled as scaled: nobody waits for the full host run).

HIP events, a warm-up, the median of REPS launches, one process.  python tools/rank_time.py [--out FILE] [D:K ...]   (default: 100 000
documents at K = 512, 128 and 392 and 10 000 at K = 2 048; first = 1, top_n = 5); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native, evaluate, ranking

REPS, WARMUP, SAMPLE, FIRST, TOP_N = 25, 3, 400, 1, 5
dev = torch.device("cuda", 0)


def foldin_like(D, K, seed):
    """(scores (D, K) float64, truth (D, K) uint8) on the device"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nnz = torch.randint(1, 9, (D, 1), device=dev, generator=g)
    cols = torch.randint(0, K, (D, 8), device=dev, generator=g)
    vals = torch.randint(1, 30, (D, 8), device=dev, generator=g).to(torch.float64) / torch.randint(30, 60, (D, 8), device=dev, generator=g)
    vals = torch.where(torch.arange(8, device=dev)[None, :] < nnz, vals, torch.zeros((), dtype=torch.float64, device=dev))
    s = torch.zeros((D, K), dtype=torch.float64, device=dev)
    s.scatter_(1, cols, vals)                                    # (a column drawn twice keeps one of its values)
    truth = (torch.rand((D, K), device=dev, generator=g) < min(0.5, 4 / (K - FIRST))).to(torch.uint8)
    return s, truth


def host_path(th, y):
    """seconds of the host metrics on (n, L) loads"""
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        tps, tns, fps, fns, fprs, tprs = evaluate.rates(th, y)
        auc = evaluate.macro_auc_roc(fprs, tprs)
        f1 = evaluate.get_f1(tps, fps, tns, fns)
        e1, e2 = evaluate.n_error(th, y, 1), evaluate.n_error(th, y, 2)
        return time.perf_counter() - t0, (auc, f1, e1, e2)


def one_shape(D, K):
    L = K - FIRST
    s, truth = foldin_like(D, K, 1000 + K)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(top_idx=new((D, TOP_N), torch.int32), top_val=new((D, TOP_N), torch.float64), n_thr=new((D,), torch.int32),
               auc=new((D,), torch.float64), f1=new((D,), torch.float64), hit_rank=new((D,), torch.int32), flags=new((D,), torch.int32))
    ev = []
    for i in range(WARMUP + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _native.rank_labels(s, truth, D, K, FIRST, TOP_N, **out)
        b.record()
        if i >= WARMUP:
            ev.append((a, b))
    torch.cuda.synchronize()
    times = np.array([a.elapsed_time(b) for a, b in ev])
    ms = float(np.median(times))
    # the host path on a sample of the same rows, and the device's answer for those rows next to it
    n = min(SAMPLE, D)
    keep = np.flatnonzero((out["flags"][:n].cpu().numpy() & (ranking.ALL_ZERO | ranking.NO_POSITIVE | ranking.NO_NEGATIVE)) == 0)
    th, y = s[:n, FIRST:].cpu().numpy()[keep], truth[:n, FIRST:].cpu().numpy()[keep]
    host_s, (auc, f1, e1, e2) = host_path(th, y)
    d_auc, d_f1 = out["auc"][:n].cpu().numpy()[keep], out["f1"][:n].cpu().numpy()[keep]
    hit = out["hit_rank"][:n].cpu().numpy()[keep]
    assert abs(np.mean(d_auc) - auc) < 1e-12 and abs(np.mean(d_f1) - f1) < 1e-12, "device and host metrics disagree"
    floor_bytes = D * L * 9
    res = dict(D=D, K=K, first=FIRST, top_n=TOP_N, reps=REPS, rank_ms=ms, rank_ms_min=float(times.min()), rank_ms_max=float(times.max()),
               docs_per_s=D / ms * 1e3, read_once_bytes=floor_bytes, read_GBps=floor_bytes / ms / 1e6,
               host_sample_docs=int(keep.size), host_sample_s=host_s, host_ms_per_doc=host_s / max(keep.size, 1) * 1e3,
               host_scaled_to_D_s=host_s / max(keep.size, 1) * D, host_scaled=True,
               speedup_over_scaled_host=host_s / max(keep.size, 1) * D / (ms * 1e-3),
               sample_auc=float(auc), sample_f1=float(f1), sample_one_error=float(e1),
               sample_one_error_device=float(((hit > 0) & (hit <= 1)).mean()))
    del s, truth, out
    torch.cuda.empty_cache()
    return res


def main():
    args, out_path = sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    shapes = [tuple(int(x) for x in a.split(":")) for a in args] or [(100000, 512), (100000, 128), (100000, 392), (10000, 2048)]
    _native.lib()
    _native.require_device()
    line = json.dumps(dict(tool="rank_time", device=torch.cuda.get_device_name(0), shapes=[one_shape(D, K) for D, K in shapes]))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
