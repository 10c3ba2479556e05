"""time of llda_heldout_loglik alone (the scoring pass behind heldout.loglik / LabeledLDA.heldout_perplexity) on D documents of N scored
sites, words uniform over V, f = 1, theta with a handful of loads per document smoothed as heldout.smooth_theta leaves it, next to

    (a) the same quantity as a chunked torch expression on the same device, (theta[site_doc] * phi_t[word]).sum(1).log(), summed;
    (b) the gather's bytes, S * K * 8, over the kernel's time: the rate at which rows of phi_t arrive;
    (c) everything behind the fold-in end to end -- smoothing, phi_t = ph_hat.t(), the kernel, 32 bytes per document back, the
        logarithms and their sum on the host -- against the host path (loads and ph_hat downloaded, the same expression in numpy)
        on a SAMPLE of the documents, scaled to D (labelled as scaled: nobody waits for the full host run).

HIP events, a warm-up, the median of REPS launches, one process.  python tools/heldout_time.py [--out FILE] [D:K[:N[:V]] ...]
(default: 100 000 documents x 150 sites at K = 512, 128 and 32, V = 100 000); prints one JSON line, --out FILE keeps it."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lda_thesis_amd import _native, heldout

REPS, WARMUP, BASE_REPS, CHUNK_BYTES, SAMPLE = 15, 3, 3, 1 << 30, 1000
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


def torch_baseline(theta, phi_t, word, N, K):
    """sum over the sites of log p, chunked so that a (sites, K) temporary stays below CHUNK_BYTES"""
    S = word.numel()
    step = max(N, CHUNK_BYTES // (8 * K) // N * N)
    total = torch.zeros((), dtype=torch.float64, device=dev)
    for lo in range(0, S, step):
        hi = min(S, lo + step)
        site_doc = torch.arange(lo, hi, device=dev) // N
        total += (theta[site_doc] * phi_t[word[lo:hi].long()]).sum(1).log().sum()
    return total


def timed(fn, reps, warmup):
    ev = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        if i >= warmup:
            ev.append((a, b))
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) for a, b in ev]), out


def one_shape(D, K, N, V):
    th, ph, doc_off, word, freq, w_obs = inputs(D, K, N, V, 1000 + K)
    theta = heldout.smooth_theta(th, w_obs, ALPHA)
    phi_t = ph.t().contiguous()
    S = D * N
    mant = torch.empty((D,), dtype=torch.float64, device=dev)
    expo, tok, bad = (torch.empty((D,), dtype=torch.int64, device=dev) for _ in range(3))
    k_ms, _ = timed(lambda: _native.heldout_loglik(doc_off, word, freq, theta, phi_t, D, V, K, mant=mant, expo=expo, tok=tok, bad=bad),
                    REPS, WARMUP)
    b_ms, base_total = timed(lambda: torch_baseline(theta, phi_t, word, N, K), BASE_REPS, 1)
    r = heldout.perplexity_from(mant.cpu().numpy(), expo.cpu().numpy(), tok.cpu().numpy(), bad.cpu().numpy())
    assert r["bad"] == 0 and r["tokens"] == S
    assert abs(r["loglik"] / float(base_total) - 1) < 1e-9, "kernel and torch expression disagree"
    ms = float(np.median(k_ms))
    # (c) end to end behind the fold-in
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e2e = heldout.perplexity_from(*heldout.loglik(heldout.smooth_theta(th, w_obs, ALPHA), ph.t().contiguous(), doc_off, word, freq))
    e2e_s = time.perf_counter() - t0
    assert e2e["loglik"] == r["loglik"]
    n = min(SAMPLE, D)
    t0 = time.perf_counter()
    th_h, ph_h = th[:n].cpu().numpy(), ph.cpu().numpy()                  # the host path downloads ph_hat whole, whatever the sample
    t_down = time.perf_counter() - t0
    w_h = word[:n * N].cpu().numpy()
    t0 = time.perf_counter()
    theta_h = heldout.smooth_theta(th_h, np.full(n, float(N)), ALPHA)
    phi_t_h = np.ascontiguousarray(ph_h.T)
    t_prep = time.perf_counter() - t0
    t0 = time.perf_counter()
    host_total = 0.0
    for d in range(n):
        host_total += float(np.log((theta_h[d][None, :] * phi_t_h[w_h[d * N:(d + 1) * N]]).sum(1)).sum())
    t_score = time.perf_counter() - t0
    down_rate = (ph.numel() + n * K) * 8 / max(t_down, 1e-9)            # bytes per second of the two downloads above
    host_scaled = t_down + (D - n) * K * 8 / down_rate + t_prep + t_score / n * D        # the loads of all D documents, the scoring of all
    res = dict(D=D, K=K, N=N, V=V, sites=S, reps=REPS, kernel_ms=ms, kernel_ms_min=float(k_ms.min()), kernel_ms_max=float(k_ms.max()),
               gather_bytes=S * K * 8, gather_TBps=S * K * 8 / ms / 1e9, sites_per_s=S / ms * 1e3,
               torch_ms=float(np.median(b_ms)), torch_ms_min=float(b_ms.min()), speedup_over_torch=float(np.median(b_ms)) / ms,
               phi_t_MB=V * K * 8 / 1e6, theta_MB=D * K * 8 / 1e6, perplexity=r["perplexity"],
               e2e_device_s=e2e_s, host_sample_docs=n, host_download_ph_s=t_down, host_prepare_s=t_prep, host_score_sample_s=t_score,
               host_scaled_to_D_s=host_scaled, host_scaled=True, e2e_speedup_over_scaled_host=host_scaled / e2e_s)
    del th, ph, theta, phi_t, word, freq
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
    line = json.dumps(dict(tool="heldout_time", device=torch.cuda.get_device_name(0), shapes=[one_shape(*s) for s in shapes]))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
