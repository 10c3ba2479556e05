"""time of llda_ecdf_ranks and llda_frex_select (topics.frex_words, LabeledLDA.frex_words / exclusivity) next to their yardsticks, on a
bench workload after five sweeps, n = 10, weight 1/2, every word a candidate, all K labels in one batch:

    ecdf_f, ecdf_e   llda_ecdf_ranks on phi_t, the (V, K) float64 phi word-major, in mode 0 and in mode 1;
    select           llda_frex_select on the two (K, V) rank tables;
    label_metrics    llda_label_metrics on a matrix of the same shape (phi_t as the scores of V "documents", a random truth): ONE sort by
                     the same engine, where FREX sorts twice;
    torch            the same statement in torch on the same tensors: the exclusivity, two torch.sort(dim=0), two searchsorted, the
                     harmonic mean in float64, torch.topk per topic.

Whether the kernels' ranks equal torch's, and whether the lists equal the topk lists (a double decides those: near ties may differ),
is reported with the times.  HIP events, 3 warm-up rounds, the median of 25, the candidates alternating in one process.
python tools/frex_words_time.py [--out FILE] [workload[:documents] ...]   (default: synth2:125000 = the vocabulary and the labels of
BASELINE configs[3]; the number of documents does not enter); prints one JSON line per workload, and --out FILE keeps them all in one
JSON file"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from lda_thesis_amd import _native
from topic_summary_time import median_ms

N, S, T = 10, 1, 2
dev = torch.device("cuda", 0)


def time_frex(spec, s):
    V, K = s.V, s.K
    phi_t = s.phi().t().contiguous()
    scratch = torch.empty((max(_native.ecdf_scratch_bytes(V, K), _native.label_scratch_bytes(V, K)),), dtype=torch.uint8, device=dev)
    scratch_sel = torch.empty((_native.frex_scratch_bytes(V, K, N),), dtype=torch.uint8, device=dev)
    rank_f = torch.empty((K, V), dtype=torch.int32, device=dev)
    rank_e = torch.empty((K, V), dtype=torch.int32, device=dev)
    n_cand = torch.zeros((1,), dtype=torch.int64, device=dev)
    top = [torch.empty((K, N), dtype=torch.int32, device=dev) for _ in range(3)]
    truth = (torch.rand((V, K), device=dev) < 0.05).to(torch.uint8)
    auc = torch.empty((K,), dtype=torch.float64, device=dev)
    f1 = torch.empty((K,), dtype=torch.float64, device=dev)

    def ecdf(mode, rank):
        return lambda: _native.ecdf_ranks(phi_t, V, K, mode, 0, K, rank, scratch, n_cand=n_cand)

    def select():
        _native.frex_select(rank_f, rank_e, V, V, K, S, T, N, scratch_sel, top_idx=top[0], top_rank_f=top[1], top_rank_e=top[2])

    def label_metrics():
        _native.label_metrics(phi_t, truth, V, K, 0, K, scratch, auc=auc, f1=f1)

    def torch_ranks():
        excl = phi_t / phi_t.sum(dim=1, keepdim=True)
        out = []
        for m in (phi_t, excl):
            col = m.t().contiguous()                                     # (K, V): a topic's values side by side
            out.append(torch.searchsorted(torch.sort(col, dim=1).values, col, right=True))
        return out

    def torch_statement():
        rf, re = torch_ranks()
        w = S / T
        frex = 1.0 / (w / (re.to(torch.float64) / V) + (1.0 - w) / (rf.to(torch.float64) / V))
        return torch.topk(frex, N, dim=1)

    ecdf(0, rank_f)()
    ecdf(1, rank_e)()
    select()
    want_f, want_e = torch_ranks()
    # (torch's row sum is not sum64: an exclusivity may differ in its last bit, and with it a rank)
    agree = dict(rank_f=bool(torch.equal(rank_f.to(torch.int64), want_f)), rank_e_differing=int((rank_e.to(torch.int64) != want_e).sum().item()),
                 lists_differing=int((top[0].to(torch.int64) != torch_statement().indices).any(dim=1).sum().item()), n_cand=int(n_cand.item()))
    del want_f, want_e
    ms = median_ms({"ecdf_f": ecdf(0, rank_f), "ecdf_e": ecdf(1, rank_e), "select": select, "label_metrics": label_metrics, "torch": torch_statement})
    total = ms["ecdf_f"] + ms["ecdf_e"] + ms["select"]
    out = dict(input=spec + " frex_words", V=V, K=K, n=N, weight="%d/%d" % (S, T), bytes_matrix=V * K * 8, scratch_bytes=int(scratch.numel()),
               ms=ms, frex_total_ms=total, agree_with_torch=agree, ecdf_e_over_label_metrics=ms["ecdf_e"] / ms["label_metrics"],
               ecdf_f_over_label_metrics=ms["ecdf_f"] / ms["label_metrics"], frex_total_over_label_metrics=total / ms["label_metrics"],
               torch_over_frex_total=ms["torch"] / total)
    print(json.dumps(out), flush=True)
    return out


def main():
    results, args, out_path = [], sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    for spec in (args or ["synth2:125000"]):
        name, _, docs = spec.partition(":")
        s, info = bench.build_sampler(name, dev, 0, 1, False, docs_total=int(docs or 0))
        for _ in range(5):
            s.sweep()
        s.check_status()
        results.append(time_frex(spec, s))
        del s, info
        torch.cuda.empty_cache()
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
