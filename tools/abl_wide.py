"""Wide layouts (K with more than 8 pairwise leaves): kernel time of the sweep for the kernel variants llda_sweep's
debug_margin selects -- 0 production (fp32 tier 0: float factors + int16 count changes in LDS, rare tiers on a scratch
row), -7 the fp32 tier with fp32 factors only in LDS (rare tiers on the scratch row), -6 with fp64 factors in LDS, -5 the fp64 kernel with the row in registers and int16 count changes, -4 the same with LDS copies of the counts,
-3 LDS-only kernel.  Each form runs ten sweeps, two to warm up and eight timed; next to the mean of the eight: the unsure / exact counters of all
ten and the state digests after them, so two
builds of the library (LLDA_GIBBS_LIB selects one, as in tools/ab_lib.sh) can be compared decision for decision.
python tools/abl_wide.py K [N V docs]"""


def main():
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import bench
    K = int(sys.argv[1])
    N, V, docs = (int(a) for a in sys.argv[2:5]) if len(sys.argv) > 4 else (100, 20000, 20000)
    bench.WORKLOADS["abl"] = (docs, N, V, K, 1.0, 1000, "ablation")
    dev = torch.device("cuda", 0)
    s, info = bench.build_sampler("abl", dev, 0, 1, False)
    out = []
    for dm in (0, -7, -6, -5, -4, -3):
        s.debug_margin = dm
        for _ in range(2):
            s.sweep()
        s.kernel_events = []
        for _ in range(8):
            s.sweep()
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in s.kernel_events]
        st = s.status.cpu().numpy()
        # (the digests of the state every form leaves: two builds that take the same decisions print the same integers)
        out.append("%d: %.3f ms %.0f M/s (unsure %d exact %d) digests %s" % (dm, sum(ms) / len(ms), s.S / (sum(ms) / len(ms)) / 1e3,
                                                                         int(st[1]), int(st[2]), bench.state_checksums(s)))
        s.status.zero_()
    print("K %d tiers %d T %d %s | " % (K, s.layout.NT, s.layout.T, os.environ.get("LLDA_GIBBS_LIB", "production").split("/")[-1])
          + " | ".join(out), flush=True)


if __name__ == "__main__":
    main()
