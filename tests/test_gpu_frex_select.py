"""``llda_frex_select`` (include/llda_gibbs.h) on synthetic ranks, exactly against its ``Fraction`` restatement (tests/frexref.py): the
planted equal costs, the planted near ties at Vc = 2^30 that no double tells apart, every weight, n below / at / above the number of
ranked words, rank 0 entries and ranks beyond Vc, probes with -1, a vocabulary that spans several partial lists with the best words
at the seams, NULL outputs.  The output buffers carry guard words behind them and are pre-filled; the scratch is poisoned."""
import numpy as np
import pytest
import torch

import frexref

pytestmark = pytest.mark.gpu

GUARD = 8
FILL = -77
DEV = "cuda:0"
WEIGHTS = ((0, 1), (1, 1), (1, 2), (7, 10), (63, 64))


def up(arr):
    return None if arr is None else torch.from_numpy(np.ascontiguousarray(arr)).to(DEV)


def run(rank_f, rank_e, Vc, s, t, n, probe=None, want=(True,) * 5):
    """the entry point on device tensors -> (top_idx, top_rank_f, top_rank_e[, probe_rank_f, probe_rank_e]) numpy, None where not
    asked for"""
    from lda_thesis_amd import _native
    L, V = (int(x) for x in rank_f.shape)
    m = 0 if probe is None else int(probe.shape[1])
    nbytes = _native.frex_scratch_bytes(V, L, n)
    scratch = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    sizes = (L * n,) * 3 + (L * m,) * 2
    bufs = [torch.full((sz + GUARD,), FILL, dtype=torch.int32, device=DEV) for sz in sizes]
    arg = [b if w else None for b, w in zip(bufs, want)]
    _native.frex_select(rank_f, rank_e, V, Vc, L, s, t, n, scratch[:nbytes], probe=probe, m=m, top_idx=arg[0], top_rank_f=arg[1],
                        top_rank_e=arg[2], probe_rank_f=arg[3] if m else None, probe_rank_e=arg[4] if m else None)
    torch.cuda.current_stream(torch.device(DEV)).synchronize()
    assert (scratch[nbytes:] == 0x5A).all()
    out = []
    for b, sz, w, cols in zip(bufs, sizes, want, (n, n, n, m, m)):
        h = b.cpu().numpy()
        assert (h[sz:] == FILL).all()
        if not w or not cols:
            assert (h == FILL).all()
        out.append(h[:sz].reshape(L, cols) if w and cols else None)
    return tuple(out if m else out[:3])


def same(got, ref, what=""):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        if g is not None:
            assert np.array_equal(g, r), "%s: got %s want %s" % (what, g[:2], r[:2])


@pytest.mark.parametrize("s,t", [(1, 2), (7, 10)])
def test_planted_equal_costs(s, t):
    """(i): different (re, rf) with EQUAL cost go by word id"""
    rank_f, rank_e, Vc, planted = frexref.planted_equal(s, t)
    for n in (1, 10, 16):
        same(run(up(rank_f), up(rank_e), Vc, s, t, n), frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, n), "n=%d" % n)


@pytest.mark.parametrize("s,t", frexref.PLANTED_WEIGHTS)
def test_planted_near_ties_at_two_to_the_thirty(s, t):
    """(ii): at Vc = 2^30 the head of the list is made of words whose costs differ while their doubles do not (checked on the CPU in
    tests/test_frex_host.py): the list is the exact one, and not the one a comparator on the double would give"""
    rank_f, rank_e, Vc = frexref.planted_near_ties(s, t)
    for n in (10, 16):
        ref = frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, n)
        got = run(up(rank_f), up(rank_e), Vc, s, t, n)
        same(got, ref, "n=%d" % n)
        assert got[0][0].tolist() != frexref.double_order(rank_f, rank_e, Vc, s, t, n)


@pytest.mark.parametrize("s,t", WEIGHTS)
def test_every_weight_list_length_rank_zero_and_probes(s, t):
    rng = np.random.default_rng(10 * s + t)
    L, V, Vc = 6, 700, 500
    rank_f = rng.integers(0, Vc + 1, size=(L, V)).astype(np.int32)
    rank_e = rng.integers(0, Vc + 1, size=(L, V)).astype(np.int32)
    rank_f[0, rng.random(V) < 0.5] = 0               # rank 0 entries: not ranked
    rank_e[0, rng.random(V) < 0.5] = 0
    rank_f[1] = rng.integers(1, 4, size=V)           # three values each: decided by the word id
    rank_e[1] = rng.integers(1, 4, size=V)
    rank_f[2], rank_e[2] = 0, 0                      # three ranked words: n is larger
    rank_f[2, [5, 300, 699]], rank_e[2, [5, 300, 699]] = (4, 9, 2), (7, 1, 2)
    rank_f[3], rank_e[3] = 0, rng.integers(1, Vc + 1, size=V)        # no ranked word at all
    rank_f[4, ::7], rank_e[4, 3::7] = Vc + 1, -5     # beyond 0 .. Vc: counts as 0
    probe = rng.integers(0, V, size=(L, 16)).astype(np.int32)
    probe[:, 3], probe[:, 9], probe[0, 0], probe[5, 15] = -1, -1, V, 2 ** 31 - 1
    probe[2, :3] = (5, 300, 6)
    for n in (1, 10, 16):
        same(run(up(rank_f), up(rank_e), Vc, s, t, n, up(probe)), frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, n, probe), "n=%d" % n)
    got = run(up(rank_f), up(rank_e), Vc, s, t, 10, up(probe[:, :1]))
    same(got, frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, 10, probe[:, :1]), "m=1")
    assert (got[0][2, 3:] == -1).all() and (got[1][2, 3:] == 0).all() and (got[2][2, 3:] == 0).all() and (got[0][3] == -1).all()
    assert (got[3][:, 0] == 0).sum() >= 2            # (the probe V of column 0, the unranked column 3)


def test_a_vocabulary_of_several_partial_lists():
    """V = 2 x 16384 + 232: three partial lists per column; the best words sit on both sides of the seams, with equal costs"""
    from lda_thesis_amd import _native
    C = _native.FREX_CHUNK
    rng = np.random.default_rng(5)
    L, V, Vc = 2, 2 * C + 232, 1 << 20
    rank_f = rng.integers(0, Vc // 2, size=(L, V)).astype(np.int32)
    rank_e = rng.integers(0, Vc // 2, size=(L, V)).astype(np.int32)
    seams = [0, C - 1, C, C + 1, 2 * C - 1, 2 * C, V - 1]
    rank_f[0, seams], rank_e[0, seams] = Vc, Vc      # seven equal best words: by id, from all three lists
    rank_f[1, seams], rank_e[1, seams] = Vc - np.arange(7, dtype=np.int32), Vc - np.arange(7, dtype=np.int32)[::-1]
    probe = np.array([seams + [-1], seams[::-1] + [7]], dtype=np.int32)
    for (s, t), n in (((1, 2), 16), ((7, 10), 10)):
        same(run(up(rank_f), up(rank_e), Vc, s, t, n, up(probe)), frexref.frex_select_ref(rank_f, rank_e, Vc, s, t, n, probe), "%d/%d" % (s, t))
    assert run(up(rank_f), up(rank_e), Vc, 1, 2, 16)[0][0, :7].tolist() == seams


def test_null_outputs_and_the_python_surface():
    from lda_thesis_amd import topics
    rng = np.random.default_rng(6)
    L, V, Vc = 3, 900, 800
    rank_f = rng.integers(0, Vc + 1, size=(L, V)).astype(np.int32)
    rank_e = rng.integers(0, Vc + 1, size=(L, V)).astype(np.int32)
    probe = rng.integers(-1, V, size=(L, 5)).astype(np.int32)
    ref = frexref.frex_select_ref(rank_f, rank_e, Vc, 7, 10, 10, probe)
    for off in range(5):
        want = tuple(i != off for i in range(5))
        same(run(up(rank_f), up(rank_e), Vc, 7, 10, 10, up(probe), want=want), ref, "without %d" % off)
    same(run(up(rank_f), up(rank_e), Vc, 7, 10, 10, up(probe), want=(False,) * 5), ref)
    side = torch.cuda.Stream(torch.device(DEV))
    got = topics.frex_select(up(rank_f), up(rank_e), Vc, 0.7, 10, probe, stream=side)
    side.synchronize()
    assert len(got) == 5 and all(g.dtype == torch.int32 for g in got) and tuple(got[0].shape) == (L, 10) and tuple(got[3].shape) == (L, 5)
    same(tuple(g.cpu().numpy() for g in got), ref)
    got = topics.frex_select(up(rank_f), up(rank_e), Vc, (7, 10), 10)
    same(tuple(g.cpu().numpy() for g in got), ref[:3])
    for bad in (dict(n=0), dict(n=17), dict(weight=1.5), dict(Vc=0), dict(probe=np.zeros((L + 1, 3))), dict(probe=np.zeros((L, 17)))):
        kw = dict(Vc=Vc, weight=0.5, n=10, probe=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            topics.frex_select(up(rank_f), up(rank_e), kw["Vc"], kw["weight"], kw["n"], kw["probe"])
    with pytest.raises(ValueError):
        topics.frex_select(up(rank_f), up(rank_e[:, :-1]), Vc, 0.5, 10)
    with pytest.raises(ValueError):
        topics.frex_select(up(rank_f.astype(np.int64)), up(rank_e), Vc, 0.5, 10)
