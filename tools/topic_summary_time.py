"""time of llda_top_words and llda_word_cooc (GibbsSampler.top_words / word_cooccurrence, LabeledLDA.coherence) next to their
yardsticks, on a bench workload after five sweeps, n = 10:

    llda_top_words   (a) a device-to-device copy of the same n_kw: what touching the bytes costs;
                     (b) the host path of topwords_per_topic: phi() on the device, its download, one argsort per topic -- the
                         argsort is timed on a SAMPLE of topics and scaled to K (the line says so);
    llda_word_cooc   (c) a device-to-device copy of ``word``;
                     (d) one sweep of the same sampler in the same run;
                     plus the global atomics per document (every atomic adds 1: the sum of ``co`` is their number) and the largest
                     entry of ``co`` (the adds the hottest address took).

HIP events, 3 warm-up rounds, the median of 25, the candidates alternating in one process.
python tools/topic_summary_time.py [--out FILE] [workload[:documents] ...]   (default: synth2 = BASELINE configs[3]); prints one
JSON line per result, and --out FILE keeps them all in one JSON file"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from lda_thesis_amd import _native, topics

REPS, WARMUP, N, ARGSORT_SAMPLE = 25, 3, 10, 8
dev = torch.device("cuda", 0)


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


def time_top_words(spec, s):
    V, K = s.V, s.K
    scratch = torch.empty((_native.top_words_scratch_bytes(V, K, N),), dtype=torch.uint8, device=dev)
    idx = torch.empty((K, N), dtype=torch.int32, device=dev)
    cnt = torch.empty((K, N), dtype=torch.int32, device=dev)
    dst = torch.empty_like(s.n_kw)
    ms = median_ms({"top_words": lambda: _native.top_words(s.n_kw, V, K, N, idx, cnt, scratch), "copy": lambda: dst.copy_(s.n_kw)})
    del dst
    # the host path: phi on the device, the download, argsort of a sample of topics
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    phi = s.phi().cpu().numpy()
    t1 = time.perf_counter()
    sample = np.linspace(0, K - 1, min(K, ARGSORT_SAMPLE)).astype(int)
    host = [np.argsort(-phi[k], kind="stable")[:N] for k in sample]
    t2 = time.perf_counter()
    got = idx.cpu().numpy()
    assert all(np.array_equal(got[k], h) for k, h in zip(sample, host)), "the device lists and argsort(-phi) disagree"
    host_ms = (t1 - t0) * 1e3 + (t2 - t1) * 1e3 * K / len(sample)
    nbytes = s.n_kw.numel() * 4
    out = dict(input=spec + " top_words", V=V, K=K, KP=int(s.n_kw.shape[1]), n=N, bytes=nbytes, scratch_bytes=int(scratch.numel()),
               top_words_ms=ms["top_words"], copy_ms=ms["copy"], ratio_to_copy=ms["top_words"] / ms["copy"],
               top_words_GBps=nbytes / ms["top_words"] / 1e6, host_phi_download_ms=(t1 - t0) * 1e3,
               host_argsort_ms_scaled=(t2 - t1) * 1e3 * K / len(sample), host_argsort_topics_timed=len(sample),
               host_path_ms_scaled=host_ms, speedup_over_host_path=host_ms / ms["top_words"])
    del phi
    print(json.dumps(out), flush=True)
    return out, idx


def time_cooc(spec, s, idx):
    K, V = s.K, s.V
    table = topics.membership(idx, V)
    co = torch.zeros((K, N, N), dtype=torch.int64, device=dev)

    def kernel():
        co.zero_()
        _native.word_cooc(s.doc_off, s.word, s.D, V, K, N, table[0], table[1], co)
    dst = torch.empty_like(s.word)
    ms = median_ms({"word_cooc": kernel, "copy": lambda: dst.copy_(s.word)})
    del dst
    sweep = median_ms({"sweep": s.sweep}, reps=10, warmup=1)["sweep"]
    host = co.cpu().numpy()
    out = dict(input=spec + " word_cooc", D=s.D, sites=s.S, K=K, n=N, listed_entries=int(table[1].numel()),
               word_cooc_ms=ms["word_cooc"], copy_word_ms=ms["copy"], ratio_to_copy=ms["word_cooc"] / ms["copy"], sweep_ms=sweep,
               cost_in_sweeps=ms["word_cooc"] / sweep, sites_per_us=s.S / ms["word_cooc"] / 1e3,
               atomics_total=int(host.sum()), atomics_per_document=float(host.sum()) / max(s.D, 1), largest_co=int(host.max()),
               atomics_per_us=float(host.sum()) / ms["word_cooc"] / 1e3)
    print(json.dumps(out), flush=True)
    return out


def main():
    results, args, out_path = [], sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    for spec in (args or ["synth2"]):
        name, _, docs = spec.partition(":")
        s, info = bench.build_sampler(name, dev, 0, 1, False, docs_total=int(docs or 0))
        for _ in range(5):
            s.sweep()
        s.check_status()
        out, idx = time_top_words(spec, s)
        results.append(out)
        results.append(time_cooc(spec, s, idx))
        del s, info
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
