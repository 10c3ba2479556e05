"""llda_rank_labels on the device: bit for bit against its CPU restatement (tests/rankref.py) around every seam of the geometry,
and end to end (LabeledLDA.predict / score_test, the harness's --device-metrics) against the host path."""
import pickle
import warnings

import numpy as np
import pytest

import rankref

pytestmark = pytest.mark.gpu

MAX_K = 7688
SMALL_L = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 391, 511, 512, 513, 1023, 1024, 1025)
BIG_L = (2047, 2999, 4097, MAX_K - 1)
OUTPUTS = ("top_idx", "top_val", "n_thr", "auc", "f1", "hit_rank", "flags")
GUARD = 8
NAN_BITS = np.uint64(0x7FF8000000000000)


def planted_rows(rng, L):
    """(scores (R, L), truth (R, L)): the rows a sort or a scan gets wrong first"""
    S, Y = [], []

    def add(s, y=None):
        S.append(np.asarray(s, dtype=np.float64))
        Y.append(rankref.gen_truth(rng, 1, L)[0] if y is None else np.asarray(y, dtype=np.uint8))

    one = lambda j: np.eye(1, L, j, dtype=np.uint8)[0]
    add(np.full(L, 0.375))                                                       # all equal, non-zero
    add(np.zeros(L))                                                             # all zero
    add(np.where(np.arange(L) % 2 == 0, -0.0, 0.0))                              # -0.0 and +0.0 only
    add(np.where(np.arange(L) % 3 == 0, -0.0, 0.0), one(L - 1))
    add((rng.integers(0, 5, size=L) + 1) * 5e-324)                               # denormals
    s = -rng.random(L)
    s[L // 2] = np.inf
    s[0 if L // 2 else -1] = -np.inf if L > 1 else np.inf
    add(s)                                                                       # negative scores, +inf and -inf
    for at in (0, L - 1):                                                        # the maximum at the first / last ranked column
        s = rng.random(L)
        s[at] = 2.0
        add(s)
    for at in (0, L - 1):                                                        # the only true label at the first / last ranked column
        add(rankref.gen_scores(rng, "grid", 1, L)[0], one(at))
        add(rng.random(L), one(at))
    tie = np.where(np.arange(L) % 2 == 0, 0.5, 0.5 + rng.choice([-3, -2, -1, 1, 2, 3], size=L) / 8)       # the largest tie group: the even columns
    for at in (0, (L - 1) // 2 * 2):                                             # the only true label at its first / last place
        add(tie, one(at))
    add(rng.random(L), np.zeros(L))                                              # P = 0
    add(rng.random(L), np.ones(L))                                               # N = 0
    add(rankref.gen_scores(rng, "foldin", 1, L)[0], np.zeros(L))
    for at in (0, L - 1):                                                        # a NaN at the first / last ranked column
        s = rng.random(L)
        s[at] = np.nan
        add(s)
    return np.stack(S), np.stack(Y)


def random_rows(rng, D, L):
    n = -(-D // 4)
    s = np.stack([rankref.gen_scores(rng, kind, n, L) for kind in rankref.KINDS], axis=1).reshape(4 * n, L)[:D]
    return s, rankref.gen_truth(rng, D, L)


def rows(rng, D, L):
    """D rows: the planted ones first where they fit, random rows of the four kinds behind them"""
    if D == "planted":
        return planted_rows(rng, L)
    if D < 30:
        return random_rows(rng, D, L)
    ps, py = planted_rows(rng, L)
    rs, ry = random_rows(rng, D - ps.shape[0], L)
    return np.concatenate([ps, rs]), np.concatenate([py, ry])


def embed(s, y, first, ld):
    """(score (D, ld), truth (D, K)): every column the kernel must not read holds NaN / 0xFF"""
    D, L = s.shape
    K = L + first
    score = np.full((D, ld), np.nan)
    score[:, first:K] = s
    truth = np.full((D, K), 0xFF, dtype=np.uint8)
    truth[:, first:K] = y
    return score, truth


PATTERN = {"int32": np.int32(-0x12345679), "float64": np.float64(-1234.5)}


def run(score, truth, K, first, top_n, skip=(), device_inputs=None):
    """one llda_rank_labels call with guarded, pre-filled output buffers -> dict of numpy arrays (whole buffers, guards included)"""
    import torch
    from lda_thesis_amd import _native
    dev = torch.device("cuda", 0)
    D = score.shape[0]
    s, t = device_inputs if device_inputs is not None else \
        (torch.from_numpy(score).to(dev), None if truth is None else torch.from_numpy(truth).to(dev))
    shapes = dict(top_idx=(D * top_n, torch.int32), top_val=(D * top_n, torch.float64), n_thr=(D, torch.int32), auc=(D, torch.float64),
                  f1=(D, torch.float64), hit_rank=(D, torch.int32), flags=(D, torch.int32))
    bufs = {}
    for name, (n, dt) in shapes.items():
        bufs[name] = torch.full((n + GUARD,), PATTERN[str(dt).split(".")[1]].item(), dtype=dt, device=dev)
    _native.rank_labels(s, t, D, K, first, top_n, ld=score.shape[1], **{n: b for n, b in bufs.items() if n not in skip})
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        return np.where(np.isnan(a), NAN_BITS, a.view(np.uint64))
    return a


def check(got, want, D, top_n, with_truth=True, skip=(), what=""):
    for name in OUTPUTS:
        n = D * top_n if name.startswith("top_") else D
        g = got[name]
        pat = PATTERN[str(g.dtype)]
        assert (g[n:] == pat).all(), "%s: guard words behind %s overwritten" % (what, name)
        if name in skip or (not with_truth and name in ("auc", "f1", "hit_rank")):
            assert (g[:n] == pat).all(), "%s: %s was written" % (what, name)
            continue
        w = np.asarray(want[name]).reshape(-1)
        bad = np.flatnonzero(bits(g[:n]) != bits(w))
        assert bad.size == 0, "%s: %s differs at %s: got %s want %s" % (what, name, bad[:5], g[:n][bad[:5]], w[bad[:5]])


@pytest.mark.parametrize("L", SMALL_L + BIG_L)
def test_bit_for_bit_against_rankref(L):
    import torch
    rng = np.random.default_rng(1000 + L)
    dev = torch.device("cuda", 0)
    for D in ((1, 63, 257) if L <= 1025 else (5, "planted")):
        s, y = rows(rng, D, L)
        n = s.shape[0]
        for first in (0, 1):
            K = L + first
            if K > MAX_K:
                continue
            for pad in (0, 3):
                score, truth = embed(s, y, first, K + pad)
                inputs = (torch.from_numpy(score).to(dev), torch.from_numpy(truth).to(dev))
                for top_n in (0, 1, 5, 16):
                    want = rankref.rank_rows(score, truth, first=first, top_n=top_n, K=K)
                    got = run(score, truth, K, first, top_n, device_inputs=inputs)
                    check(got, want, n, top_n, what="L=%d D=%s first=%d ld=K+%d top_n=%d" % (L, D, first, pad, top_n))


def test_largest_k():
    """K = LLDA_MAX_K with first = 1 (L = 7 687) is in the list above; with first = 0 all 7 688 columns are ranked"""
    rng = np.random.default_rng(5)
    s, y = random_rows(rng, 3, MAX_K)
    score, truth = embed(s, y, 0, MAX_K + 3)
    check(run(score, truth, MAX_K, 0, 16), rankref.rank_rows(score, truth, first=0, top_n=16, K=MAX_K), 3, 16, what="K=7688")


@pytest.mark.parametrize("L", (9, 65, 511, 1025, 2999))
def test_without_truth_and_with_missing_outputs(L):
    rng = np.random.default_rng(L)
    s, y = rows(rng, 40, L)
    score, truth = embed(s, y, 1, L + 4)
    want = rankref.rank_rows(score, truth, first=1, top_n=5, K=L + 1)
    no_truth = rankref.rank_rows(score, None, first=1, top_n=5, K=L + 1)
    for name in ("top_idx", "top_val", "n_thr"):
        assert np.array_equal(bits(no_truth[name]), bits(want[name]))
    check(run(score, None, L + 1, 1, 5), no_truth, 40, 5, with_truth=False, what="truth = NULL")
    for name in OUTPUTS:                                  # every output pointer NULL in turn: the others are unchanged
        check(run(score, truth, L + 1, 1, 5, skip=(name,)), want, 40, 5, skip=(name,), what="%s = NULL" % name)


@pytest.mark.parametrize("L", (15, 100, 511, 1025, 2999))
def test_geometry_independence(L):
    """the same rows as one call of D documents and as calls of 1, 7 and D - 8 documents: identical bytes"""
    import torch
    rng = np.random.default_rng(L)
    D = 63 if L <= 1025 else 13
    s, y = rows(rng, D, L) if D >= 30 else random_rows(rng, D, L)
    score, truth = embed(s, y, 1, L + 1)
    whole = run(score, truth, L + 1, 1, 5)
    at = 0
    for n in (1, 7, D - 8):
        part = run(score[at:at + n], truth[at:at + n], L + 1, 1, 5)
        for name in OUTPUTS:
            w = 5 if name.startswith("top_") else 1
            assert np.array_equal(bits(part[name][:n * w]), bits(whole[name][at * w:(at + n) * w])), (name, at, n)
        at += n
    assert at == D


def test_python_surface_on_numpy_and_strided_input():
    import torch
    from lda_thesis_amd import ranking
    rng = np.random.default_rng(3)
    s, y = random_rows(rng, 50, 40)
    score, truth = embed(s, y, 1, 41)
    score[:, 0] = 0.5                                     # (numpy's sort would move a NaN; column 0 is simply not ranked)
    want = rankref.rank_rows(score, truth, first=1, top_n=5)
    wide = torch.from_numpy(np.concatenate([score, np.full((50, 7), np.nan)], axis=1)).to("cuda:0")
    for arg in (score, wide[:, :41]):                    # a numpy array is uploaded; a device view keeps its row stride
        r = ranking.rank_labels(arg, truth, first=1, top_n=5)
        h = r.host()
        for name in OUTPUTS:
            assert np.array_equal(bits(h[name]), bits(want[name])), name
    m = ranking.metrics(r)
    keep = (want["flags"] & rankref.ALL_ZERO) == 0
    assert m["kept"] == int(keep.sum()) and m["dropped"] == 50 - m["kept"]
    assert m["one_error"] == float(((want["hit_rank"][keep] > 0) & (want["hit_rank"][keep] <= 1)).mean())
    bad = score.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError):
        ranking.metrics(ranking.rank_labels(bad, truth))
    flat = score.copy()
    flat[2, 1:] = 0.25                                    # one distinct score: the host's trapezoid raises
    with pytest.raises(ValueError, match="At least 2 points"):
        ranking.metrics(ranking.rank_labels(flat, truth))
    with pytest.raises(ValueError):
        ranking.metrics(ranking.rank_labels(score))       # no truth, no metrics


# ---- end to end against the host path ----
def _model(name):
    from fixture_corpora import tiny_corpus
    from lda_thesis_amd.LabeledLDA import LabeledLDA
    from lda_thesis_amd.text import Dictionary
    docs, labs, labelset, alpha, beta, sweeps, npseed = tiny_corpus(name)
    np.random.seed(npseed)
    m = LabeledLDA(docs, labs, list(labelset), Dictionary(docs), alpha, beta, seed=12345)
    m.run_training(4, 2)
    held = [(d, l) for d, l in zip(docs, labs) if l]
    return m, [d for d, _ in held], [l for _, l in held]


def _host_metrics(th, y):
    from lda_thesis_amd import evaluate
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore")
        tps, tns, fps, fns, fprs, tprs = evaluate.rates(th, y)
        return dict(auc=evaluate.macro_auc_roc(fprs, tprs), one_error=evaluate.n_error(th, y, 1), two_error=evaluate.n_error(th, y, 2),
                    f1=evaluate.get_f1(tps, fps, tns, fns)), max(len(tp) for tp in tps)


@pytest.mark.parametrize("name", ("k12", "k130"))
def test_predict_and_score_test_against_the_host_path(name, capsys):
    from lda_thesis_amd.evaluate import binary_yreal
    m, docs, labs = _model(name)
    th = m.run_test(docs, 6, 2, seed=77)
    host = m.get_preds(th, 5)
    dev = m.predict(docs, 6, 2, n=5, seed=77)
    assert len(dev) == len(host)
    for d, (a, b) in enumerate(zip(host, dev)):
        assert [float(x) for _, x in a] == [float(x) for _, x in b]               # the loads: the same bits everywhere
        top = np.sort(th[d])[::-1][:6]
        if np.unique(top).size == top.size:                                       # the five highest loads distinct (and above the sixth)
            assert [str(x) for x, _ in a] == [str(x) for x, _ in b], d
    # score_test against evaluate.* on the downloaded loads, by report's rules
    y = binary_yreal(labs, m.labelmap)[:, 1:]
    keep = th[:, 1:].sum(axis=1) != 0
    want, t_max = _host_metrics(th[keep, 1:], y[keep])
    got = m.score_test(docs, labs, 6, 2, seed=77)
    n = int(keep.sum())
    assert got["kept"] == n and got["dropped"] == len(docs) - n
    eps = 2.0 ** -53
    print(name, got, want)
    assert np.isnan(want["auc"]) == np.isnan(got["auc"]) and np.isnan(want["f1"]) == np.isnan(got["f1"])
    if not np.isnan(want["auc"]):
        assert abs(got["auc"] - want["auc"]) <= (4 * t_max + 32 + n) * eps
    if not np.isnan(want["f1"]):
        assert abs(got["f1"] - want["f1"]) <= (8 * want["f1"] + n) * eps
    # (the loads of these corpora have ties among the zeros only: the first two places are decided wherever a document has two
    # positive loads; where it has one, the second place is a zero and the tie rule decides -- compare with the rule's order)
    order = np.argsort(-th[keep, 1:], axis=1, kind="stable")
    hit = np.take_along_axis(y[keep], order, axis=1)
    assert got["one_error"] == int((hit[:, :1].sum(axis=1) > 0).sum()) / n
    assert got["two_error"] == int((hit[:, :2].sum(axis=1) > 0).sum()) / n
    if all(np.unique(np.sort(r)[::-1][:3]).size == 3 for r in th[keep, 1:]):
        assert got["one_error"] == want["one_error"] and got["two_error"] == want["two_error"]


def _write_csv(path, n=120, seed=3):
    rng = np.random.default_rng(seed)
    codes = ["A11", "A12", "A21", "B11", "B21", "B22", "C31"]
    words = ["growth", "taxes", "labor", "market", "policy", "trade", "capital", "wages", "prices", "credit",
             "banking", "income", "health", "energy", "education", "housing", "export", "budget", "inflation"]
    topic_words = {c: rng.choice(len(words), size=6, replace=False) for c in codes}
    lines = []
    for i in range(n):
        labs = [codes[j] for j in rng.choice(len(codes), size=int(rng.integers(1, 3)), replace=False)]
        toks = [words[int(rng.choice(topic_words[labs[int(rng.integers(len(labs)))]]))] for _ in range(int(rng.integers(12, 40)))]
        lines.append('d%d,"%s","%s"' % (i, " ".join(toks), " ".join(labs)))
    path.write_text("\n".join(lines) + "\n")


def test_cli_device_metrics(tmp_path, capsys, monkeypatch):
    """--device-metrics prints the same four lines (values to 1e-12); without it the report is what evaluate.* gives on the pickled
    loads, line for line as before"""
    from lda_thesis_amd import evaluate
    from lda_thesis_amd import evaluate_LabeledLDA as H
    monkeypatch.chdir(tmp_path)
    _write_csv(tmp_path / "toy.csv")
    argv = ["-f", str(tmp_path / "toy.csv"), "-d", "3", "-i", "20", "-s", "5"]
    np.random.seed(0)
    H.main(argv + ["-p"])
    plain = capsys.readouterr().out
    np.random.seed(0)
    H.main(argv + ["--device-metrics"])
    device = capsys.readouterr().out
    tail = lambda out: out[out.index("Model:               Labeled LDA"):].splitlines()
    a, b = tail(plain), tail(device)
    assert len(a) == len(b) == 9 and a[:5] == b[:5]
    for x, y in zip(a[5:], b[5:]):
        label = x[:25]
        assert y[:25] == label and label.strip() in ("AUC ROC:", "one error:", "two error:", "F1 score (macro average)")
        assert abs(float(x[25:]) - float(y[25:])) <= 1e-12, (x, y)
    # the default run: exactly the host report on the loads it pickled
    model, test, th = (pickle.load(open(tmp_path / f, "rb")) for f in
                       ("LabeledLDA_model.pkl", "LabeledLDA_testset.pkl", "LabeledLDA_theta.pkl"))
    yb = evaluate.binary_yreal(test[1], model.labelmap)[:, 1:]
    keep = np.where(th[:, 1:].sum(axis=1) != 0)[0]
    yb, t = yb[keep, :], th[:, 1:][keep, :]
    tps, tns, fps, fns, fprs, tprs = evaluate.rates(t, yb)
    assert a[5:] == ["%s %s" % line for line in (("AUC ROC:                 ", evaluate.macro_auc_roc(fprs, tprs)),
                                                 ("one error:               ", evaluate.n_error(t, yb, 1)),
                                                 ("two error:               ", evaluate.n_error(t, yb, 2)),
                                                 ("F1 score (macro average) ", evaluate.get_f1(tps, fps, tns, fns)))]
