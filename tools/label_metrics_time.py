"""time of llda_label_metrics and llda_label_sets alone (labelwise.label_metrics / label_sets) on scores shaped like fold-in output --
one to eight positive loads per document, ratios of small integers, the rest exact zeros -- next to the same quantities in torch
on the same device tensors:

    label_metrics   torch.sort(scores[:, 1:].T.contiguous(), dim=1, descending=True, stable=True), gather of truth, cumsum
                    (torch_sort_ms: the yardstick), and with the Mann-Whitney count and the best F1 on top (torch_full_ms);
    label_sets      the comparison with the thresholds and the seven sums (at_least_one off on both sides).

Before anything is timed the script asserts that torch's integers equal the kernel's (order, P, T, A, thr_tp, thr_fp; masks and
counts).  HIP events, a warm-up, the median of REPS launches, one process.  The per-pass split of llda_label_metrics (keys / chunk
sort / each merge level / walk) is not visible from here: run this script with --metrics-only --reps 3 under a kernel trace.

python tools/label_metrics_time.py [--out FILE] [--metrics-only] [--reps N] [D:K ...]   (default: 100 000 documents at K = 512 and
1 000 000 at K = 128 for label_metrics, 100 000 at K = 512 for label_sets); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native

REPS, WARMUP, FIRST = 20, 3, 1
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
    s.scatter_(1, cols, vals)
    truth = ((s > 0) & (torch.rand((D, K), device=dev, generator=g) < 0.7)) | (torch.rand((D, K), device=dev, generator=g) < 2 / K)
    return s, truth.to(torch.uint8)


def timed(fn, reps):
    ev = []
    for i in range(WARMUP + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if i >= WARMUP:
            ev.append((a, b))
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(ms=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))


def torch_sorted(s, truth):
    st = s[:, FIRST:].T.contiguous()
    vals, idx = torch.sort(st, dim=1, descending=True, stable=True)
    t = torch.gather(truth[:, FIRST:].T.contiguous(), 1, idx)
    return vals, idx, t, torch.cumsum(t, dim=1, dtype=torch.int64)


def torch_full(s, truth):
    vals, idx, t, tp = torch_sorted(s, truth)
    L, D = vals.shape
    at = torch.arange(D, device=dev)
    end = torch.ones((L, D), dtype=torch.bool, device=dev)
    end[:, :-1] = vals[:, :-1] != vals[:, 1:]
    P = tp[:, -1]
    fp = at[None, :] + 1 - tp
    last = torch.cummax(torch.where(end, at[None, :], torch.full((), -1, device=dev)), dim=1).values
    prev = torch.cat([torch.full((L, 1), -1, device=dev), last[:, :-1]], dim=1)       # the threshold before every position
    pc = prev.clamp(min=0)
    has = (prev >= 0).to(torch.int64)
    term = (fp - torch.gather(fp, 1, pc) * has) * (tp + torch.gather(tp, 1, pc) * has)
    A = (term * end).sum(dim=1)
    # (rationals with denominators below 2^22 that differ do so by more than 2^-44: the float comparison finds a largest one, and
    # argmax takes the first of equal quotients)
    ratio = torch.where(end & (tp > 0), (2 * tp).to(torch.float64) / (at[None, :] + 1 + P[:, None]).to(torch.float64),
                        torch.full((), -1.0, dtype=torch.float64, device=dev))
    best = torch.argmax(ratio, dim=1, keepdim=True)
    btp = torch.gather(tp, 1, best)[:, 0]
    bfp = torch.gather(fp, 1, best)[:, 0]
    none = P == 0
    return dict(order=idx, n_pos=P, n_thr=end.sum(dim=1), auc_num=A, thr_tp=torch.where(none, 0, btp), thr_fp=torch.where(none, 0, bfp))


def metrics_shape(D, K, reps):
    L = K - FIRST
    s, truth = foldin_like(D, K, 2000 + K)
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = {n: new((L,), torch.int64) for n in ("n_pos", "n_thr", "auc_num", "thr_tp", "thr_fp")}
    out.update({n: new((L,), torch.float64) for n in ("auc", "f1", "thr")})
    out.update(flags=new((L,), torch.int32), order=new((L, D), torch.int32))
    scratch = new((_native.label_scratch_bytes(D, L),), torch.uint8)
    kern = lambda: _native.label_metrics(s, truth, D, K, FIRST, L, scratch, **out)
    kern()
    want = torch_full(s, truth)
    for name, w in want.items():
        assert torch.equal(out[name].to(torch.int64), w.to(torch.int64)), "torch and the kernel disagree on %s" % name
    del want
    torch.cuda.empty_cache()
    res = dict(D=D, K=K, first=FIRST, reps=reps, scratch_bytes=int(scratch.numel()), integers_equal=True)
    res.update({"label_metrics_" + k: v for k, v in timed(kern, reps).items()})
    res.update({"torch_sort_" + k: v for k, v in timed(lambda: torch_sorted(s, truth), reps).items()})
    res.update({"torch_full_" + k: v for k, v in timed(lambda: torch_full(s, truth), reps).items()})
    res["speedup_over_torch_sort"] = res["torch_sort_ms"] / res["label_metrics_ms"]
    del s, truth, out, scratch
    torch.cuda.empty_cache()
    return res


def torch_sets(s, thr, truth):
    elig = ~torch.isnan(thr)
    elig[:FIRST] = False
    pred = (s >= thr[None, :]) & elig[None, :]
    t = truth != 0
    t[:, :FIRST] = False
    hit = pred & t
    return dict(pred=pred, n_pred=pred.sum(dim=1), n_hit=hit.sum(dim=1), n_true=t.sum(dim=1), tp=hit.sum(dim=0), fp=(pred & ~t).sum(dim=0),
                fn=(~pred & t).sum(dim=0))


def sets_shape(D, K, reps):
    s, truth = foldin_like(D, K, 3000 + K)
    thr = torch.randint(1, 30, (K,), device=dev).to(torch.float64) / 45
    thr[::17] = float("nan")
    W = (K + 31) // 32
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    out = dict(mask=new((D, W), torch.int32), n_pred=new((D,), torch.int32), n_hit=new((D,), torch.int32), n_true=new((D,), torch.int32))
    cnt = {n: torch.zeros((K,), dtype=torch.int64, device=dev) for n in ("tp", "fp", "fn")}
    _native.label_sets(s, thr, truth, D, K, FIRST, False, **out, **cnt)
    want = torch_sets(s, thr, truth)
    for name in ("n_pred", "n_hit", "n_true", "tp", "fp", "fn"):
        got = (out if name in out else cnt)[name]
        assert torch.equal(got.to(torch.int64), want[name].to(torch.int64)), "torch and the kernel disagree on %s" % name
    bits = (out["mask"][:, :, None] >> torch.arange(32, device=dev)[None, None, :]) & 1
    assert torch.equal(bits.reshape(D, W * 32)[:, :K].to(torch.bool), want["pred"]), "torch and the kernel disagree on the masks"
    del want, bits
    res = dict(D=D, K=K, first=FIRST, reps=reps, integers_equal=True)

    def kern():
        for c in cnt.values():
            c.zero_()
        _native.label_sets(s, thr, truth, D, K, FIRST, False, **out, **cnt)
    res.update({"label_sets_" + k: v for k, v in timed(kern, reps).items()})
    res.update({"torch_" + k: v for k, v in timed(lambda: torch_sets(s, thr, truth), reps).items()})
    res["speedup_over_torch"] = res["torch_ms"] / res["label_sets_ms"]
    res["read_once_bytes"] = D * K * 9
    res["read_GBps"] = res["read_once_bytes"] / res["label_sets_ms"] / 1e6
    return res


def main():
    args, out_path, reps = sys.argv[1:], None, REPS
    for flag in ("--out", "--reps"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                reps = int(args[i + 1])
            del args[i:i + 2]
    metrics_only = "--metrics-only" in args
    args = [a for a in args if a != "--metrics-only"]
    shapes = [tuple(int(x) for x in a.split(":")) for a in args] or [(100000, 512), (1000000, 128)]
    _native.lib()
    _native.require_device()
    res = dict(tool="label_metrics_time", device=torch.cuda.get_device_name(0), label_metrics=[metrics_shape(D, K, reps) for D, K in shapes])
    if not metrics_only:
        res["label_sets"] = [sets_shape(100000, 512, reps)]
    line = json.dumps(res)
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
