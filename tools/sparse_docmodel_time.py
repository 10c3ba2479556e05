"""time of llda_attribute_sparse and llda_credit_words_sparse (the kernels behind emfit.fit_sparse / LabeledLDA.fit_em(sparse=True))
against the dense llda_attribute / llda_credit_words on the same inputs expanded to (D, K): D documents of N sites, f = 1, words
uniform over V, every document the root and 7 random labels with random loads, a skewed phi_t.  Timed in ONE run, the variants
taking turns repetition by repetition:

    attribute         llda_attribute(iters = 1) on theta (D, K)            | attribute_sparse  llda_attribute_sparse(iters = 1)
    words             llda_credit_words(chunk = 4096) on theta (D, K)      | words_sparse      llda_credit_words_sparse(chunk = 4096)
    iteration         attribute, words, llda_phi_step: one emfit.fit pass  | iteration_sparse  one emfit.fit_sparse pass
    parent_attribute, parent_words: the two dense entry points of ANOTHER build of the library (--parent-lib FILE: the parent
                      commit's libllda_gibbs.so), on the same buffers

HIP events, a warm-up, the median of REPS repetitions, one process.  The tool asserts that the two forms agree (1e-9 relative: they
pair the terms of p differently) and that no site was bad.
python tools/sparse_docmodel_time.py [--out FILE] [--parent-lib FILE] [D:K[:N[:V]] ...]
(default: 100 000 documents x 150 sites at K = 512 and 2048, V = 100 000); prints one JSON line, --out FILE keeps it."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from attribute_time import ALPHA, REPS, WARMUP, dev, timed_in_turns
from lda_thesis_amd import _native, emfit

LABELS = 8                                                                 # the root and 7
CHUNK = 4096
BETA = 0.01


def inputs(D, K, N, V, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lab = torch.zeros((D, LABELS), dtype=torch.int64, device=dev)
    step = 10000                                                           # (a (step, K) temporary, not (D, K))
    for lo in range(0, D, step):
        n = min(step, D - lo)
        pick = torch.rand((n, K - 1), device=dev, generator=g).topk(LABELS - 1, dim=1).indices + 1
        lab[lo:lo + n, 1:] = pick.sort(dim=1).values
    theta_s = torch.rand((D, LABELS), dtype=torch.float64, device=dev, generator=g) + 0.05
    theta_s /= theta_s.sum(dim=1, keepdim=True)
    theta = torch.zeros((D, K), dtype=torch.float64, device=dev)
    theta.scatter_(1, lab, theta_s)
    ph = torch.rand((K, V), dtype=torch.float64, device=dev, generator=g) ** 8 + 1e-6
    ph /= ph.sum(dim=1, keepdim=True)
    word = torch.randint(0, V, (D * N,), device=dev, generator=g).to(torch.int32)
    freq = torch.ones((D * N,), dtype=torch.int32, device=dev)
    doc_off = torch.arange(D + 1, dtype=torch.int64, device=dev) * N
    lab_off = torch.arange(D + 1, dtype=torch.int64, device=dev) * LABELS
    return theta, theta_s.reshape(-1).contiguous(), lab_off, lab.reshape(-1).to(torch.int32).contiguous(), ph.t().contiguous(), doc_off, word, freq


def parent_calls(path):
    """llda_attribute / llda_credit_words of another build, on the structs of this binding (neither has changed)"""
    L = ctypes.CDLL(path)
    for fn, struct in ((L.llda_attribute, _native.LldaAttrArgs), (L.llda_credit_words, _native.LldaWcreditArgs)):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.POINTER(struct), ctypes.c_void_p]
    L.llda_struct_size.restype = ctypes.c_int
    L.llda_struct_size.argtypes = [ctypes.c_int]
    L.llda_wcredit_struct_bytes.restype = ctypes.c_int
    assert L.llda_struct_size(6) == ctypes.sizeof(_native.LldaAttrArgs) and L.llda_wcredit_struct_bytes() == ctypes.sizeof(_native.LldaWcreditArgs)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def attribute(doc_off, word, freq, theta, phi_t, D, V, K, theta_out):
        a = _native.LldaAttrArgs(p(doc_off), p(word), p(freq), p(theta), p(phi_t), D, V, K, K, K, K, K, 1, 0, 0, ALPHA, p(theta_out), None, None,
                                 None, None, None)
        assert L.llda_attribute(ctypes.byref(a), stream()) == 0

    def words(word_off, site_doc, freq, theta, phi_t, D, V, S, K, scratch, cw, tok, bad):
        a = _native.LldaWcreditArgs(ctypes.sizeof(_native.LldaWcreditArgs), K, CHUNK, 0, p(word_off), p(site_doc), p(freq), p(theta), p(phi_t), D, V,
                                    S, K, K, K, p(cw), p(tok), p(bad), p(scratch), int(scratch.numel()))
        assert L.llda_credit_words(ctypes.byref(a), stream()) == 0

    return attribute, words


def one_case(D, K, N, V, parent):
    theta, theta_s, lab_off, lab, phi_t, doc_off, word, freq = inputs(D, K, N, V, 2000 + K)
    S, NL = D * N, D * LABELS
    word_off, site_doc, w_freq, _ = emfit.word_major(doc_off, word, freq, V, dev)
    new = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)
    th_out, ths_out, cw, cw_s, cw_p, phi_new = new((D, K)), new((NL,)), new((V, K)), new((V, K)), new((V, K)), new((V, K))
    th_out_p = new((D, K))
    tok, bad, tok_s, bad_s, tok_p, bad_p = (new((V,), torch.int64) for _ in range(6))
    scratch = new((max(_native.credit_words_scratch_bytes(V, S, K, CHUNK), _native.phi_step_scratch_bytes(V, K)),), torch.uint8)

    def attribute(out=th_out):
        _native.attribute(doc_off, word, freq, theta, phi_t, D, V, K, iters=1, alpha=ALPHA, theta_out=out)

    def attribute_sparse(out=ths_out):
        _native.attribute_sparse(doc_off, word, freq, lab_off, lab, theta_s, phi_t, D, V, K, NL, LABELS, iters=1, alpha=ALPHA, theta_out=out)

    def words(th=theta):
        _native.credit_words(word_off, site_doc, w_freq, th, phi_t, D, V, S, K, CHUNK, scratch, credit_w=cw, tok=tok, bad=bad)

    def words_sparse(th=theta_s):
        _native.credit_words_sparse(word_off, site_doc, w_freq, lab_off, lab, th, phi_t, D, V, S, K, NL, LABELS, CHUNK, scratch, credit_w=cw_s,
                                    tok=tok_s, bad=bad_s)

    def iteration():
        attribute()
        words(th_out)
        _native.phi_step(cw, V, K, BETA, phi_new, scratch)

    def iteration_sparse():
        attribute_sparse()
        words_sparse(ths_out)
        _native.phi_step(cw_s, V, K, BETA, phi_new, scratch)

    fns = dict(attribute=attribute, attribute_sparse=attribute_sparse, words=words, words_sparse=words_sparse)
    if parent:
        p_attr, p_words = parent
        fns["parent_attribute"] = lambda: p_attr(doc_off, word, freq, theta, phi_t, D, V, K, th_out_p)
        fns["parent_words"] = lambda: p_words(word_off, site_doc, w_freq, theta, phi_t, D, V, S, K, scratch, cw_p, tok_p, bad_p)
    ms = timed_in_turns(fns, REPS, WARMUP)
    # the two forms agree (they pair the terms of p differently: last bits), and nothing was bad
    assert int(bad.sum()) == 0 == int(bad_s.sum()) and int(tok.sum()) == S == int(tok_s.sum())
    cw_err = float(((cw_s - cw).abs() / (cw.abs() + 1e-300)).max())
    th_err = float(((ths_out - th_out.gather(1, lab.view(D, LABELS).long()).reshape(-1)).abs() / ths_out).max())
    assert cw_err < 1e-9 and th_err < 1e-9, (cw_err, th_err)
    assert int((th_out != 0).sum()) == NL
    if parent:                                                             # the dense kernels did not move: the same bits
        assert torch.equal(cw_p, cw) and torch.equal(th_out_p, th_out) and torch.equal(tok_p, tok)
    ms.update(timed_in_turns(dict(iteration=iteration, iteration_sparse=iteration_sparse), REPS, WARMUP))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    res = dict(D=D, K=K, N=N, V=V, sites=S, labels=LABELS, chunk=CHUNK, reps=REPS, ms=med, ms_min={k: float(v.min()) for k, v in ms.items()},
               ms_max={k: float(v.max()) for k, v in ms.items()},
               dense_over_sparse={k: med[k] / med[k + "_sparse"] for k in ("attribute", "words", "iteration")},
               row_bytes_per_site=dict(dense=8 * K, sparse=8 * LABELS), max_rel_diff=dict(credit_w=cw_err, theta=th_err))
    del theta, theta_s, phi_t, th_out, th_out_p, cw, cw_s, cw_p, phi_new, scratch
    torch.cuda.empty_cache()
    return res


def main():
    args, out_path, parent = sys.argv[1:], None, None
    for flag in ("--out", "--parent-lib"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                parent = args[i + 1]
            del args[i:i + 2]
    shapes = []
    for a in args:
        p = [int(x) for x in a.split(":")]
        shapes.append((p[0], p[1], p[2] if len(p) > 2 else 150, p[3] if len(p) > 3 else 100000))
    shapes = shapes or [(100000, 512, 150, 100000), (100000, 2048, 150, 100000)]
    _native.lib()
    _native.require_device()
    calls = parent_calls(parent) if parent else None
    cases = [one_case(*s, parent=calls) for s in shapes]
    line = json.dumps(dict(tool="sparse_docmodel_time", device=torch.cuda.get_device_name(0), parent_lib=bool(parent), cases=cases))
    print(line, flush=True)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
