"""time of llda_nearest_rows alone (the kernel behind similar.nearest_rows / LabeledLDA.similar_documents): Q queries against D rows of
inner length L, n = 10, rows like fold-in loads (square roots of sparse distributions) -- Q D L fused multiply-adds per launch -- and,
on the same tensors, the only route a user had before: torch.topk over a @ b.T, cut into row ranges of b so that the score buffer
stays at or below 1 GB, with the merge of the ranges.  The share of equal ids and the largest score difference of the two routes are reported.

HIP events, a warm-up, the median of REPS launches, one process.  python tools/nearest_rows_time.py [--out FILE] [Q:D:L[:n] ...]
(default: 1 024 x 1 000 000 x 512 and 1 024 x 100 000 x 128); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native, similar

REPS, WARMUP = 5, 1
SCORE_BYTES = 1 << 30
dev = torch.device("cuda", 0)


def timed(fn, reps, warmup):
    ev = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        if i >= warmup:
            ev.append((a, b))
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev])


def loads(rows, L, g):
    """square roots of distributions with about a tenth of their entries non-zero, in slices of at most 2^27 elements"""
    out = torch.empty((rows, L), dtype=torch.float64, device=dev)
    step = max(1, (1 << 27) // L)
    for r0 in range(0, rows, step):
        x = torch.rand((min(step, rows - r0), L), dtype=torch.float64, device=dev, generator=g)
        x = torch.where(x > 0.9, (x - 0.9) ** 2, torch.zeros_like(x))
        x[:, 0] += 1e-3
        out[r0:r0 + x.shape[0]] = torch.sqrt(x / x.sum(dim=1, keepdim=True))
    return out


def torch_route(a, b, n, step):
    vals, ids = [], []
    for r0 in range(0, b.shape[0], step):
        v, i = torch.topk(a @ b[r0:r0 + step].t(), min(n, b.shape[0] - r0), dim=1)
        vals.append(v)
        ids.append(i + r0)
    v, pick = torch.topk(torch.cat(vals, dim=1), n, dim=1)
    return v, torch.gather(torch.cat(ids, dim=1), 1, pick)


def one_shape(Q, D, L, n):
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + L)
    a, b = loads(Q, L, g), loads(D, L, g)
    nbytes = _native.nearest_scratch_bytes(Q, D, n, 0)
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    top_idx = torch.empty((Q, n), dtype=torch.int64, device=dev)
    top_val = torch.empty((Q, n), dtype=torch.float64, device=dev)
    n_nan = torch.empty((Q,), dtype=torch.int64, device=dev)
    ms = timed(lambda: _native.nearest_rows(a, b, Q, D, L, n, scratch, top_idx=top_idx, top_val=top_val, n_nan=n_nan), REPS, WARMUP)
    step = max(1, SCORE_BYTES // (8 * Q))
    t_ms = timed(lambda: torch_route(a, b, n, step), REPS, WARMUP)
    tv, ti = torch_route(a, b, n, step)
    assert int(n_nan.sum().item()) == 0
    same_ids = float((ti == top_idx).to(torch.float64).mean().item())
    val_err = float((tv - top_val).abs().max().item())
    fmas = Q * D * L
    med, t_med = float(np.median(ms)), float(np.median(t_ms))
    q_tiles = -(-Q // _native.NEAREST_TILE)
    return dict(Q=Q, D=D, L=L, n=n, reps=REPS, kernel_ms=med, kernel_ms_min=float(ms.min()), kernel_ms_max=float(ms.max()),
                fmas=fmas, fmas_per_s=fmas / med * 1e3, b_bytes=D * L * 8, b_bytes_requested=q_tiles * D * L * 8, scratch_bytes=nbytes,
                torch_ms=t_med, torch_ms_min=float(t_ms.min()), torch_ms_max=float(t_ms.max()), torch_rows_per_range=step,
                torch_score_bytes=8 * Q * min(step, D), torch_over_kernel=t_med / med, same_ids=same_ids, max_score_difference=val_err)


def main():
    args, out_path = sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    shapes = []
    for s in args:
        p = [int(x) for x in s.split(":")]
        shapes.append((p[0], p[1], p[2], p[3] if len(p) > 3 else 10))
    shapes = shapes or [(1024, 1000000, 512, 10), (1024, 100000, 128, 10)]
    _native.lib()
    _native.require_device()
    line = json.dumps(dict(tool="nearest_rows_time", device=torch.cuda.get_device_name(0), shapes=[one_shape(*s) for s in shapes]))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
