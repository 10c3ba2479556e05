"""time of the fold-in sampler on sparse label sets (llda_foldin_sparse) against the dense llda_foldin, and of the whole shortlist
route: every document the root and 7 random labels, words uniform over V, a skewed phi_t (the inputs of tools/sparse_heldout_time.py).

    dense      llda_foldin over all K topics on the prepared lane-major matrices (the launches of foldin.fold_in: the start draws
               and the sweeps; the column normalisation that fold_in does before them is NOT timed, n_dk is zeroed inside)
    sparse     llda_foldin_sparse on the documents' own label lists
    shortlist  the whole route of predict(shortlist=7): llda_attribute with no EM step from uniform loads (credit (D, K)),
               llda_rank_labels (first = 1, top 7), the lists built on the device (sort, root in front), llda_foldin_sparse on them

SWEEPS sweeps with thinning THIN.  HIP events, 2 warm-up rounds, the median of 9 repetitions with the variants taking turns, one
process.  The tool asserts that every form assigned every token (the counts sum to D x N) and raised nowhere.
python tools/sparse_foldin_time.py [--out FILE] D:K[:N[:V]] ...
prints one JSON line, --out FILE keeps it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from attribute_time import ALPHA, REPS, WARMUP, dev, timed_in_turns
from lda_thesis_amd import _native, foldin
from lda_thesis_amd.layout import group_layout
from sparse_docmodel_time import LABELS, inputs
from sparse_heldout_time import summary

SWEEPS, THIN = 50, 5
SHORT = LABELS - 1
SEED = 0x5EED
C_INIT, C_LOOP = 1.0000000005, 1.0000005            # foldin.fold_in's


def one_case(D, K, N, V):
    theta, _, lab_off, lab, phi_t, doc_off, word, freq = inputs(D, K, N, V, 4000 + K)
    del theta
    S, NL = D * N, D * LABELS
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    # ---- the dense launch, prepared as foldin.fold_in prepares it
    lay = group_layout(K)
    lm = torch.from_numpy(lay.lm_topic_pos.astype(np.int64)).to(dev)
    ph = phi_t.t()
    phn = ph / foldin.numpy_column_sums(ph)
    assert bool(torch.isfinite(phn).all())
    d_ph = torch.zeros((V, lay.KP), dtype=torch.float64, device=dev)
    d_ph[:, lm] = phi_t
    d_init = torch.zeros((V + 1, lay.KP), dtype=torch.float64, device=dev)
    d_init[:V, lm] = phn.t()
    d_init[V, lm] = 1 / K
    del phn
    valid = torch.from_numpy((lay.lm_pos_topic >= 0).astype(np.uint8)).to(dev)
    z_d, n_dk, th = new((S,), torch.int32), new((D, lay.KP), torch.int32), new((D, lay.KP))
    status = torch.zeros((3,), dtype=torch.int32, device=dev)
    # ---- the sparse launches
    z_s, n_dk_s, th_s = new((S,), torch.int32), new((NL,), torch.int32), new((NL,))
    z_c, n_dk_c, th_c = new((S,), torch.int32), new((NL,), torch.int32), new((NL,))
    uniform = torch.full((D, K), 1.0 / K, dtype=torch.float64, device=dev)
    credit = new((D, K))
    top_idx, top_val, n_thr, flags = new((D, SHORT), torch.int32), new((D, SHORT)), new((D,), torch.int32), new((D,), torch.int32)
    short_lab = torch.zeros((D, LABELS), dtype=torch.int32, device=dev)

    def dense():
        n_dk.zero_()
        _native.foldin(doc_off=doc_off, word=word, init_idx=word, freq=freq, ph=d_ph, init_rows=d_init, slot_valid=valid, z=z_d, n_dk=n_dk,
                       th=th, status=status[0:1], D=D, K=K, iters=SWEEPS, thinning=THIN, alpha=ALPHA, beta=0.0, c_init=C_INIT, c_loop=C_LOOP,
                       seed=SEED, stream_id=foldin.TEST_STREAM)

    def sparse_on(lists, z, nd, t, st):
        _native.foldin_sparse(doc_off, word, freq, phi_t, lab_off, lists, D, V, K, NL, LABELS, iters=SWEEPS, thinning=THIN, alpha=ALPHA,
                              c_init=C_INIT, c_loop=C_LOOP, seed=SEED, stream_id=foldin.TEST_STREAM, z=z, n_dk_s=nd, th_s=t, status=st)

    def sparse():
        sparse_on(lab, z_s, n_dk_s, th_s, status[1:2])

    def shortlist():
        _native.attribute(doc_off, word, freq, uniform, phi_t, D, V, K, iters=0, alpha=0.0, credit=credit)
        _native.rank_labels(credit, None, D, K, 1, SHORT, ld=K, top_idx=top_idx, top_val=top_val, n_thr=n_thr, flags=flags)
        short_lab[:, 1:] = top_idx.sort(dim=1).values
        sparse_on(short_lab.reshape(-1), z_c, n_dk_c, th_c, status[2:3])

    ms = timed_in_turns(dict(dense=dense, sparse=sparse, shortlist=shortlist), REPS, WARMUP)
    assert status.cpu().tolist() == [0, 0, 0], status
    assert int(n_dk.sum()) == S and int(n_dk_s.sum()) == S and int(n_dk_c.sum()) == S
    assert int((short_lab[:, 1:] >= 1).all()) and int((short_lab[:, 1:].diff(dim=1) > 0).all())
    own = float((short_lab[:, 1:, None] == lab.reshape(D, LABELS)[:, None, 1:]).any(dim=2).double().mean())
    res = dict(D=D, K=K, N=N, V=V, sites=S, labels=LABELS, sweeps=SWEEPS, thinning=THIN, reps=REPS, site_sweeps=S * (SWEEPS + 1),
               row_bytes_per_site=dict(dense=8 * lay.KP, sparse=8 * LABELS), shortlist_share_of_own_labels=own, **summary(ms))
    for name in ("sparse", "shortlist"):
        res["dense_over_" + name] = res["ms"]["dense"] / res["ms"][name]
        res[name + "_faster_by_more_than_the_spread"] = res["ms_max"][name] < res["ms_min"]["dense"]
    res["Gsite_sweeps_per_s"] = {k: res["site_sweeps"] / v * 1e-6 for k, v in res["ms"].items()}
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
    shapes = shapes or [(100000, 512, 150, 100000), (100000, 2048, 150, 100000)]
    _native.lib()
    _native.require_device()
    cases = []
    for s in shapes:
        cases.append(one_case(*s))
        torch.cuda.empty_cache()
    line = json.dumps(dict(tool="sparse_foldin_time", device=torch.cuda.get_device_name(0), cases=cases))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
