"""time of llda_window_cooc (topics.window_cooccurrence, LabeledLDA.window_coherence) next to llda_word_cooc on the same arrays, on
the token corpus of a bench workload after five sweeps, n = 10: the sampler's sites repeated by their frequency and shuffled inside
every document (a CSR has no reading order; any order of the same tokens costs the same walk), the lists = the sampler's top
words.  Timed: windows 10 (C_UCI, C_NPMI) and 110 (C_V), window 0 of the new kernel (one window per document: what llda_word_cooc
counts) and llda_word_cooc itself; with the windows visited, the moves played (a listed word entering or leaving: at most two per listed
token of a document longer than the window), the adds of run lengths that reached ``co`` in sum, and the largest entry.

HIP events, one warm-up launch (timed on the host to size the repeats: the median of 3 .. 25 launches), the candidates in turn.
python tools/window_cooc_time.py [--out FILE] [workload[:documents] ...]   (default: synth2 = BASELINE configs[3], then abstracts);
prints one JSON line per result, and --out FILE keeps them all in one JSON file"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from lda_thesis_amd import _native, topics

N, BUDGET_S = 10, 15.0
dev = torch.device("cuda", 0)


def token_corpus(s):
    """(tok_off int64 [D+1], tok int32 [S']) on the device: every site f times, the tokens of a document in random order"""
    f = s.freq.to(torch.int64)
    tok = torch.repeat_interleave(s.word, f)
    doc = torch.repeat_interleave(torch.arange(s.D, device=dev), s.doc_off[1:] - s.doc_off[:-1])
    doc = torch.repeat_interleave(doc, f)
    tok_off = torch.zeros((s.D + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(doc, minlength=s.D), 0, out=tok_off[1:])
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    key = doc * (1 << 31) + torch.randint(0, 1 << 31, doc.shape, device=dev, generator=g)
    order = torch.sort(key)[1]
    return tok_off, tok[order].contiguous()


def median_ms(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    reps = int(min(25, max(3, BUDGET_S / max(time.perf_counter() - t0, 1e-4))))
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        ev.append((a, b))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])), reps


def time_windows(spec, s, idx):
    K, V = s.K, s.V
    tok_off, tok = token_corpus(s)
    table = topics.membership(idx, V)
    co = torch.zeros((K, N, N), dtype=torch.int64, device=dev)
    lens = (tok_off[1:] - tok_off[:-1]).cpu().numpy()
    listed = (table[0][1:] > table[0][:-1])[tok.to(torch.int64)]                  # which tokens are a listed word
    doc_of = torch.repeat_interleave(torch.arange(s.D, device=dev), tok_off[1:] - tok_off[:-1])
    per_doc = torch.bincount(doc_of[listed], minlength=s.D).cpu().numpy()
    out = []
    for name, window in (("word_cooc", None), ("window 0", 0), ("window 10", 10), ("window 110", 110)):
        def kernel():
            co.zero_()
            if window is None:
                _native.word_cooc(tok_off, tok, s.D, V, K, N, table[0], table[1], co)
            else:
                _native.window_cooc(tok_off, tok, s.D, V, K, N, window, table[0], table[1], co)
        ms, reps = median_ms(kernel)
        host = co.cpu().numpy()
        w = window or 0
        slides = lens > w if w else np.zeros_like(lens, dtype=bool)
        r = dict(input="%s %s" % (spec, name), D=s.D, tokens=int(tok.numel()), K=K, n=N, listed_entries=int(table[1].numel()),
                 listed_tokens=int(per_doc.sum()), ms=ms, launches_timed=reps, tokens_per_us=int(tok.numel()) / ms / 1e3,
                 windows=topics.window_count(tok_off, w), moves_at_most=int(2 * per_doc[slides].sum()), sum_co=int(host.sum()),
                 largest_co=int(host.max()))
        print(json.dumps(r), flush=True)
        out.append(r)
    assert out[0]["sum_co"] == out[1]["sum_co"], "window 0 and llda_word_cooc disagree"
    return out


def main():
    results, args, out_path = [], sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    for spec in (args or ["synth2", "abstracts"]):
        name, _, docs = spec.partition(":")
        s, info = bench.build_sampler(name, dev, 0, 1, False, docs_total=int(docs or 0))
        for _ in range(5):
            s.sweep()
        s.check_status()
        idx, _ = s.top_words(N)
        results += time_windows(spec, s, idx)
        del s, info
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
