"""time of llda_left_to_right alone (the kernel behind leftright.loglik / LabeledLDA.left_to_right) on D documents of N tokens, words
uniform over V, every topic allowed, R particles -- R N (N + 1) / 2 categorical draws over K topics per document -- and, as context
from the same run, the draws per second of the fold-in sampler (foldin.fold_in, llda_foldin) on the same documents as bags of words:
the wall time of 20 sweeps minus that of none, so that the host's preparation drops out.

HIP events, a warm-up, the median of REPS launches, one process.  python tools/leftright_time.py [--out FILE] [D:K[:N[:V[:R]]] ...]
(default: 10 000 documents x 150 tokens at K = 512 and 128, V = 20 000, R = 10); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native, heldout, leftright
from lda_thesis_amd.foldin import fold_in

REPS, WARMUP, FOLD_SWEEPS = 5, 1, 20
ALPHA, SEED = 0.1, 12345
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


def fold_seconds(ph, tups, sweeps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fold_in(ph, ALPHA, tups, sweeps, max(1, sweeps), SEED, keep_device=True)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def one_shape(D, K, N, V, R):
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + K)
    ph = torch.rand((K, V), dtype=torch.float64, device=dev, generator=g) ** 8 + 1e-6       # (K, V), rows sum to one, skewed
    ph /= ph.sum(dim=1, keepdim=True)
    phi_t = ph.t().contiguous()
    word = torch.randint(0, V, (D * N,), device=dev, generator=g).to(torch.int32)
    doc_off = torch.arange(D + 1, dtype=torch.int64, device=dev) * N
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ms = timed(lambda: _native.left_to_right(doc_off, word, phi_t, D, V, K, particles=R, alpha=ALPHA, seed=SEED,
                                             stream_id=leftright.LR_STREAM, max_doc_tokens=N, mant=mant, expo=expo, tok=tok, bad=bad,
                                             status=status), REPS, WARMUP)
    r = heldout.perplexity_from(mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy())
    assert r["bad"] == 0 and r["tokens"] == D * N and int(status.item()) == 0
    draws = D * R * N * (N + 1) // 2
    med = float(np.median(ms))
    # context: the fold-in sampler on the same documents as bags of words
    w_h = word.cpu().numpy().reshape(D, N)
    tups, sites = [], 0
    for d in range(D):
        ids, cnt = np.unique(w_h[d], return_counts=True)
        tups.append(list(zip(ids.tolist(), cnt.tolist())))
        sites += len(ids)
    fold_seconds(ph, tups, 1)                                           # warm-up
    t0, t1 = fold_seconds(ph, tups, 0), fold_seconds(ph, tups, FOLD_SWEEPS)
    fold_draws = sites * FOLD_SWEEPS
    return dict(D=D, K=K, N=N, V=V, R=R, reps=REPS, kernel_ms=med, kernel_ms_min=float(ms.min()), kernel_ms_max=float(ms.max()),
                draws=draws, draws_per_s=draws / med * 1e3, perplexity=r["perplexity"],
                foldin_sweeps=FOLD_SWEEPS, foldin_sites=sites, foldin_s_0_sweeps=t0, foldin_s_20_sweeps=t1,
                foldin_draws_per_s=fold_draws / max(t1 - t0, 1e-9))


def main():
    args, out_path = sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    shapes = []
    for a in args:
        p = [int(x) for x in a.split(":")]
        shapes.append((p[0], p[1], p[2] if len(p) > 2 else 150, p[3] if len(p) > 3 else 20000, p[4] if len(p) > 4 else 10))
    shapes = shapes or [(10000, 512, 150, 20000, 10), (10000, 128, 150, 20000, 10)]
    _native.lib()
    _native.require_device()
    line = json.dumps(dict(tool="leftright_time", device=torch.cuda.get_device_name(0), shapes=[one_shape(*s) for s in shapes]))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
