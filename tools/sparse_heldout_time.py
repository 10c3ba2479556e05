"""time of llda_heldout_loglik_sparse and llda_left_to_right_sparse against the dense entry points on the same label sets: every
document the root and 7 random labels, words uniform over V, a skewed phi_t (the inputs of tools/sparse_docmodel_time.py).

    score   D documents of N sites, f = 1:
            sparse   llda_heldout_loglik_sparse on the loads per slot
            scatter  the slots written into a zeroed (D, K) matrix (what emfit.fit_sparse's default trace does first)
            dense    llda_heldout_loglik on that matrix;  dense_route = scatter + dense, one after the other
    lr      D documents of N tokens, R particles:
            sparse   llda_left_to_right_sparse on the label lists
            dense    llda_left_to_right with the same sets as the allowed rows (K <= 1024 only)

HIP events, 2 warm-up rounds, the median of 9 repetitions with the variants taking turns, one process.  The tool asserts that the two
forms scored the same tokens and agree (score: 1e-9 relative in the log-likelihood -- they pair the terms of p differently; lr: the
corpus log-likelihood within 1 % -- the draws differ where the last bits of a prefix do).
python tools/sparse_heldout_time.py [--out FILE] score|lr D:K[:N[:V]] ...
prints one JSON line, --out FILE keeps it."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from attribute_time import ALPHA, REPS, WARMUP, dev, timed_in_turns
from lda_thesis_amd import _native
from sparse_docmodel_time import LABELS, inputs

PARTICLES = 10
SEED = 0x5EED


def summary(ms):
    return dict(ms={k: float(np.median(v)) for k, v in ms.items()}, ms_min={k: float(v.min()) for k, v in ms.items()},
                ms_max={k: float(v.max()) for k, v in ms.items()})


def loglik(mant, expo):
    return float((torch.log(mant) + expo.to(torch.float64) * math.log(2.0)).sum())


def score_case(D, K, N, V):
    theta, theta_s, lab_off, lab, phi_t, doc_off, word, freq = inputs(D, K, N, V, 2000 + K)
    NL = D * LABELS
    del theta
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    dense_theta = new((D, K))
    rows = torch.arange(D, device=dev).repeat_interleave(LABELS)
    cols = lab.long()
    out = {name: (new((D,)), new((D,), torch.int64), new((D,), torch.int64), new((D,), torch.int64)) for name in ("sparse", "dense")}

    def sparse():
        m, e, t, b = out["sparse"]
        _native.heldout_loglik_sparse(doc_off, word, freq, lab_off, lab, theta_s, phi_t, D, V, K, NL, LABELS, mant=m, expo=e, tok=t, bad=b)

    def scatter():
        dense_theta.zero_()
        dense_theta[rows, cols] = theta_s

    def dense():
        m, e, t, b = out["dense"]
        _native.heldout_loglik(doc_off, word, freq, dense_theta, phi_t, D, V, K, mant=m, expo=e, tok=t, bad=b)

    def dense_route():
        scatter()
        dense()

    scatter()
    ms = timed_in_turns(dict(sparse=sparse, scatter=scatter, dense=dense, dense_route=dense_route), REPS, WARMUP)
    S = D * N
    for name in out:
        assert int(out[name][2].sum()) == S and int(out[name][3].sum()) == 0, name
    ll = {name: loglik(out[name][0], out[name][1]) for name in out}
    assert abs(ll["sparse"] / ll["dense"] - 1) < 1e-9, ll
    res = dict(kind="score", D=D, K=K, N=N, V=V, sites=S, labels=LABELS, reps=REPS, loglik=ll,
               row_bytes_per_site=dict(dense=8 * K, sparse=8 * LABELS), **summary(ms))
    res["dense_route_over_sparse"] = res["ms"]["dense_route"] / res["ms"]["sparse"]
    res["faster_by_more_than_the_spread"] = res["ms_max"]["sparse"] < res["ms_min"]["dense_route"]
    return res


def lr_case(D, K, N, V):
    _, _, lab_off, lab, phi_t, doc_off, word, _ = inputs(D, K, N, V, 3000 + K)
    NL = D * LABELS
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    out = {name: (new((D,)), new((D,), torch.int64), new((D,), torch.int64), new((D,), torch.int64)) for name in ("sparse", "dense")}
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    with_dense = K <= _native.LR_MAX_K
    allowed = None
    if with_dense:
        allowed = torch.zeros((D, K), dtype=torch.uint8, device=dev)
        allowed[torch.arange(D, device=dev).repeat_interleave(LABELS), lab.long()] = 1

    def sparse():
        m, e, t, b = out["sparse"]
        _native.left_to_right_sparse(doc_off, word, phi_t, lab_off, lab, D, V, K, NL, LABELS, particles=PARTICLES, alpha=ALPHA, seed=SEED,
                                     stream_id=0, max_doc_tokens=N, mant=m, expo=e, tok=t, bad=b, status=status)

    def dense():
        m, e, t, b = out["dense"]
        _native.left_to_right(doc_off, word, phi_t, D, V, K, particles=PARTICLES, alpha=ALPHA, seed=SEED, stream_id=0, max_doc_tokens=N,
                              mant=m, expo=e, tok=t, bad=b, allowed=allowed, status=status)

    fns = dict(sparse=sparse, dense=dense) if with_dense else dict(sparse=sparse)
    ms = timed_in_turns(fns, REPS, WARMUP)
    S = D * N
    assert int(status.item()) == 0
    ll = {}
    for name in fns:
        assert int(out[name][2].sum()) == S and int(out[name][3].sum()) == 0, name
        ll[name] = loglik(out[name][0], out[name][1])
    res = dict(kind="lr", D=D, K=K, N=N, V=V, tokens=S, labels=LABELS, particles=PARTICLES, reps=REPS, loglik=ll,
               draws=D * PARTICLES * N * (N + 1) // 2, **summary(ms))
    if with_dense:
        assert abs(ll["sparse"] / ll["dense"] - 1) < 1e-2, ll
        res["dense_over_sparse"] = res["ms"]["dense"] / res["ms"]["sparse"]
        res["faster_by_more_than_the_spread"] = res["ms_max"]["sparse"] < res["ms_min"]["dense"]
    return res


def main():
    args, out_path = sys.argv[1:], None
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    if not args or args[0] not in ("score", "lr"):
        sys.exit(__doc__)
    kind, shapes = args[0], []
    for a in args[1:]:
        p = [int(x) for x in a.split(":")]
        shapes.append((p[0], p[1], p[2] if len(p) > 2 else 150, p[3] if len(p) > 3 else 100000))
    shapes = shapes or ([(100000, 512, 150, 100000), (100000, 2048, 150, 100000)] if kind == "score" else
                        [(10000, 512, 150, 100000), (10000, 2048, 150, 100000)])
    _native.lib()
    _native.require_device()
    cases = []
    for s in shapes:
        cases.append((score_case if kind == "score" else lr_case)(*s))
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="sparse_heldout_time", device=torch.cuda.get_device_name(0), cases=cases))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
