"""time of llda_scored_words (GibbsSampler.scored_words, LabeledLDA.label_words) next to its yardsticks, on a bench workload after five
sweeps, n = 10:

    counts mode   (a, b) = (1, 0): phi itself, no divisor; and (5, 2): LDAvis's default relevance 0.6 with the divisor of the word totals;
    matrix mode   the same two on phi_t, the (V, K) float64 phi word-major;
    llda_top_words on the same n_kw, a device-to-device copy of n_kw, and the same (5, 2) score stated in torch on the device
    (phi, four multiplications, the divisor, ``torch.topk`` per topic).

Bytes a pass reads: V*KP*4 (counts) or V*K*8 (matrix), plus V*8 of the divisor.  Whether the kernel's scores equal the torch statement's
bit for bit is reported with the times.  HIP events, 3 warm-up rounds, the median of 25, the candidates alternating in one process.
python tools/scored_words_time.py [--out FILE] [workload[:documents] ...]   (default: synth2 = BASELINE configs[3]); prints one JSON
line per workload, and --out FILE keeps them all in one JSON file"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from lda_thesis_amd import _native, topics
from topic_summary_time import median_ms

N = 10
dev = torch.device("cuda", 0)


def time_scored(spec, s):
    V, K, KP = s.V, s.K, int(s.n_kw.shape[1])
    scratch = torch.empty((_native.scored_words_scratch_bytes(V, K, N),), dtype=torch.uint8, device=dev)
    scratch_top = torch.empty((_native.top_words_scratch_bytes(V, K, N),), dtype=torch.uint8, device=dev)
    idx = torch.empty((K, N), dtype=torch.int32, device=dev)
    sc = torch.empty((K, N), dtype=torch.float64, device=dev)
    nn = torch.empty((K,), dtype=torch.int32, device=dev)
    cnt = torch.empty((K, N), dtype=torch.int32, device=dev)
    a, b = topics.relevance_powers(0.6)
    wdiv = torch.from_numpy(topics.word_divisor(s.word_totals().cpu().numpy(), b)).to(dev)
    phi_t = s.phi().t().contiguous()

    def counts(a_, w):
        return lambda: _native.scored_words(V, K, N, a_, scratch, n_kw=s.n_kw, n_k=s.n_k, beta=s.beta, wdiv=w, top_idx=idx, top_score=sc, n_nan=nn)

    def matrix(a_, w):
        return lambda: _native.scored_words(V, K, N, a_, scratch, mat=phi_t, wdiv=w, top_idx=idx, top_score=sc, n_nan=nn)

    def torch_statement():
        x = s.phi()                                          # (K, V)
        p = x
        for _ in range(a - 1):
            p = p * x
        score = torch.where(wdiv != 0, p / wdiv, torch.full_like(p, -float("inf")))
        return torch.topk(score, N, dim=1)

    # do the lists agree?  (topk leaves the order of equal scores open: the scores are compared, and reported with the times)
    counts(a, wdiv)()
    want = torch_statement().values
    agree_counts = bool(torch.equal(sc, want))
    matrix(a, wdiv)()
    agree_matrix = bool(torch.equal(sc, want))
    dst = torch.empty_like(s.n_kw)
    ms = median_ms({"counts_1_0": counts(1, None), "counts_5_2": counts(a, wdiv), "matrix_1_0": matrix(1, None), "matrix_5_2": matrix(a, wdiv),
                    "top_words": lambda: _native.top_words(s.n_kw, V, K, N, idx, cnt, scratch_top), "copy": lambda: dst.copy_(s.n_kw),
                    "torch_topk_5_2": torch_statement})
    bytes_counts, bytes_matrix = V * KP * 4, V * K * 8
    out = dict(input=spec + " scored_words", V=V, K=K, KP=KP, n=N, a=a, b=b, bytes_counts=bytes_counts, bytes_matrix=bytes_matrix,
               bytes_wdiv=V * 8, scratch_bytes=int(scratch.numel()), ms=ms, scores_equal_torch=dict(counts=agree_counts, matrix=agree_matrix),
               counts_1_0_GBps=bytes_counts / ms["counts_1_0"] / 1e6, counts_5_2_GBps=(bytes_counts + V * 8) / ms["counts_5_2"] / 1e6,
               matrix_1_0_GBps=bytes_matrix / ms["matrix_1_0"] / 1e6, matrix_5_2_GBps=(bytes_matrix + V * 8) / ms["matrix_5_2"] / 1e6,
               top_words_GBps=bytes_counts / ms["top_words"] / 1e6, counts_5_2_over_top_words=ms["counts_5_2"] / ms["top_words"],
               counts_1_0_over_top_words=ms["counts_1_0"] / ms["top_words"], torch_over_counts_5_2=ms["torch_topk_5_2"] / ms["counts_5_2"])
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
        results.append(time_scored(spec, s))
        del s, info
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
