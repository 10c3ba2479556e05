"""The planted left-to-right inputs of tests/leftrightties.py are what they claim to be, and they discriminate (host only).

The integer model of the exact plants equals the restatement's trace on every plant, and the outputs name it; every class is present
at every boundary kind.  Each deliberately wrong draw below (``wrong_draw``, a local variant of leftrightref.draw64 patched in for
the test only) changes (mant, expo) of the documents it concerns:

    `>=` for `>`                      exactly the ``tie`` documents, no ``above`` or ``below`` one
    topic-major order                 exactly the plants that the integer model decides differently in that order (K > 64: ties of
                                      every kind among them)
    first positive on no hit          every overflow document
    last position on no hit           every overflow document
    the mask ignored                  every masked ``zero_lane`` document
    no x > 0 mask                     a subnormal document at least (the no-hit rule, reached there by rounding)
"""
import numpy as np
import pytest

import leftrightref as ref
import leftrightties as lt

KS = (2, 9, 64, 65, 130, 512, 1000)


def wrong_draw(ge=False, topic_major=False, fallback="last_positive", no_pos=False):
    """draw64 with one thing wrong"""
    def draw(x, u, stats=None):
        x = np.asarray(x, dtype=np.float64)
        P, K = x.shape
        if topic_major:                                                 # one prefix over the topics 0 .. K - 1
            with np.errstate(all="ignore"):
                q = np.cumsum(x, axis=1)
                flag = (x > 0.0) & (q > (np.asarray(u, dtype=np.float64) * q[:, -1])[:, None])
            at = np.where(flag.any(axis=1), np.argmax(flag, axis=1), K - 1 - np.argmax((x > 0.0)[:, ::-1], axis=1))
            return np.where((x > 0.0).any(axis=1), at, ref.NONE).astype(np.int64)
        NI = ref.slots(K)
        g = ref._grid(x, NI)
        there = ref._grid(np.ones((P, K)), NI) > 0                      # the positions that hold a topic
        with np.errstate(all="ignore"):
            q = g.copy()
            for i in range(1, NI):
                q[:, i] = q[:, i - 1] + g[:, i]
            X = q[:, NI - 1].copy()
            d = 1
            while d < 64:
                Y = X.copy()
                Y[:, d:] = X[:, :-d] + X[:, d:]
                X = Y
                d *= 2
            t = np.asarray(u, dtype=np.float64) * X[:, 63]
            tg = t[:, None] - np.concatenate([np.zeros((P, 1)), X[:, :-1]], axis=1)
            pos = there if no_pos else g > 0.0
            flag = pos & ((q >= tg[:, None, :]) if ge else (q > tg[:, None, :]))
        flat = lambda m: m.transpose(0, 2, 1).reshape(P, -1)
        topic_at = lambda at: at // NI + 64 * (at % NI)
        flag, pos, there = flat(flag), flat(pos), flat(there)
        n = pos.shape[1]
        first = np.argmax(flag, axis=1)
        last = n - 1 - np.argmax((there if fallback == "last_position" else pos)[:, ::-1], axis=1)
        if fallback == "first_positive":
            last = np.argmax(pos, axis=1)
        at = np.where(flag.any(axis=1), first, last)
        return np.where(pos.any(axis=1), topic_at(at), ref.NONE).astype(np.int64)
    return draw


def changed(c, want, monkeypatch, **wrong):
    """the documents whose (mant, expo) a wrong draw changes"""
    with monkeypatch.context() as m:
        if wrong.pop("no_mask", False):
            m.setattr(ref, "masked", lambda x, mask: x)
        if wrong:
            m.setattr(ref, "draw64", wrong_draw(**wrong))
        got = lt.expected(c, c["R"])
    return set(np.flatnonzero((got[0] != want[0]) | (got[1] != want[1])).tolist())


def test_the_variant_without_a_fault_is_draw64():
    rng = np.random.default_rng(1)
    for K in (9, 130, 1000):
        x = rng.gamma(0.3, size=(40, K)) * (rng.random((40, K)) < 0.5)
        x[0] = 0.0
        u = rng.random(40)
        np.testing.assert_array_equal(wrong_draw()(x, u), ref.draw64(x, u))
        stats = {}
        np.testing.assert_array_equal(ref.draw64(x, u, stats), ref.draw64(x, u))
        assert stats == {"draws": 39, "no_hit": 0}


@pytest.mark.parametrize("R,r_star", ((1, 0), (3, 2)))
@pytest.mark.parametrize("K", KS)
def test_exact_plants(K, R, r_star, monkeypatch):
    c = lt.exact_case(K, R, r_star)
    plants, where = c["plants"], c["where"]
    trace = {}
    want = lt.expected(c, R, trace=trace)
    assert want[4] == 0 and (want[2][where] == 2).all() and (want[3][where] == 0).all()
    # the integer model is the restatement's draw, and the outputs name it
    assert [int(t) for t in trace["z"][where, r_star, 0]] == [p["z0"] for p in plants]
    assert lt.decode_z0(c, want[0], want[1], trace["z"]) == [[p["z0"]] for p in plants]
    # every class at every kind (the masked and the unmasked zero lanes each), and what the classes mean
    for kind in lt.kinds_of(K):
        for cls in lt.CLASSES:
            keys = [(kind, cls, False), (kind, cls, True)] if kind == "zero_lane" else [(kind, cls)]
            assert all(c["count"].get(k, 0) >= 3 for k in keys), (kind, cls)
    assert set(lt.kinds_of(K)) == ({"lane0_first", "lane_end", "before_last"} if K == 2 else set(lt.KINDS) - ({"slot_seam"} if K <= 64 else set()))
    order = lt.lane_major(K)
    for p in plants:
        ranks = [order.index(k) for k in p["positives"]]
        assert ranks == sorted(ranks) and 2 <= len(ranks) <= 9
    lens = np.diff(c["doc_off"])
    assert (lens[where] == 2).all() and (c["doc_ids"] >= 2 ** 32).sum() >= 10 and len(set((c["doc_ids"] & 0xFFFFFFFF).tolist())) == len(lens)
    words, counts = np.unique(c["word"], return_counts=True)
    assert (counts[words >= lt.V_RANDOM] == 1).all()
    docs = lambda keep: {int(where[j]) for j, p in enumerate(plants) if keep(p)}
    # `>=`: the ties and nothing else, not even a random document
    assert changed(c, want, monkeypatch, ge=True) == docs(lambda p: p["cls"] == "tie")
    # topic-major: what the integer model says of that order (R = 1: with more particles the others' draws move as well)
    tm = changed(c, want, monkeypatch, topic_major=True)
    assert R > 1 or tm & set(where.tolist()) == docs(lambda p: p["z0_topic_major"] != p["z0"])
    if R > 1:
        pass
    elif K > 64:
        for kind in lt.kinds_of(K):
            assert docs(lambda p: p["kind"] == kind and p["cls"] == "tie") & tm, kind
    else:
        assert not tm
    # the mask ignored: every masked plant
    masked = docs(lambda p: p["masked"])
    assert (len(masked) >= 9 or K == 2) and masked <= changed(c, want, monkeypatch, no_mask=True)


@pytest.mark.parametrize("K", KS)
def test_tuned_plants(K):
    c = lt.tuned_case(K, 1, 0)
    facts = c["plants"]
    assert 16 <= len(facts) <= lt.N_TUNED
    assert sum(f["upper"] for f in facts) >= 6 and sum(not f["upper"] for f in facts) >= 6
    assert c["n_equal"] >= 8                                            # q == t_j exactly: the strict `>` alone decides the lower double
    assert {f["kind"] for f in facts} == set(lt.kinds_of(K))
    trace = {}
    lt.expected(c, 1, trace=trace)
    lens = np.diff(c["doc_off"])
    for f in facts:
        d = int(c["where"][f["doc"]])
        assert 4 <= lens[d] <= 10 and trace["z"][d, 0, lens[d] - 2] == f["topic"] == (f["k_at"] if f["upper"] else f["k_next"])
    # particle r_star of a launch with more particles is the tuned one
    c3 = lt.tuned_case(K, 3, 2)
    lt.expected(c3, 3, trace=trace)
    for f in c3["plants"]:
        d = int(c3["where"][f["doc"]])
        assert trace["z"][d, 2, np.diff(c3["doc_off"])[d] - 2] == f["topic"]


@pytest.mark.parametrize("K", (9, 130))
def test_ge_changes_tuned_plants_whose_prefix_equals_its_threshold(K, monkeypatch):
    """a lower double with q == t_j: `>=` takes the boundary there"""
    c = lt.tuned_case(K, 1, 0)
    want = lt.expected(c, 1)
    hit = changed(c, want, monkeypatch, ge=True)
    assert hit and hit <= {int(c["where"][f["doc"]]) for f in c["plants"] if f["equal"]}


@pytest.mark.parametrize("K", (40, 130, 1000))
def test_overflow_documents(K, monkeypatch):
    c = lt.overflow_case(K)
    assert len(c["pairs"]) == (4 if K <= 64 else 8) and min(c["no_hit"]) >= 5
    assert {last == k1 for (k1, _, _), last in zip(c["pairs"], c["last"])} == {True, False}
    stats, trace = {}, {}
    want = lt.expected(c, 2, stats=stats, trace=trace)
    assert stats["no_hit"] == sum(c["no_hit"])
    assert (trace["z"][:, :, 0] == np.array(c["last"])[:, None]).all()
    assert (want[2] == 7).all() and (want[3] == 1).all()                # B at position 5: S = inf
    every = set(range(len(c["pairs"])))
    assert changed(c, want, monkeypatch, fallback="first_positive") == every
    assert changed(c, want, monkeypatch, fallback="last_position") == every
    if K > 64:
        assert changed(c, want, monkeypatch, topic_major=True)


@pytest.mark.parametrize("scale", sorted(lt.SCALES))
@pytest.mark.parametrize("K", (9, 130, 1024))
def test_scales_land_where_they_say(K, scale, monkeypatch):
    c = lt.scaled_case(K, scale)
    stats, trace = {}, {}
    want = lt.expected(c, c["R"], stats=stats, trace=trace)
    lens = np.diff(c["doc_off"])
    assert (want[2] + want[3] == lens).all() and want[2].sum() > 0.9 * lens.sum()
    # p_n (n + A alpha) is the mean of the particles' totals
    A = (c["allowed"] != 0).sum(axis=1)
    p = trace["p"]
    n = np.arange(p.shape[1])[None, :]
    with np.errstate(all="ignore"):
        tot = p * (n + A[:, None] * c["alpha"])
    tot = tot[np.isfinite(p) & (p > 0)]
    E = lt.SCALES[scale]
    lg = np.log2(tot)
    if scale == "top":
        assert tot.min() > 1e300 and lg.max() < 1006
    else:
        assert E - 6 < lg.min() and lg.max() < E + 6
    if scale.startswith("sub"):
        assert p[np.isfinite(p)].max() < 2.0 ** -1022 and c["n_flushed"] > 0
    if scale == "sub1066":
        assert stats["no_hit"] > 0                                      # u * X[63] rounded up to X[63]
        # without the x > 0 mask such a draw returns the last position, a topic that is not allowed; at K = 1024 no p_n, a mean over
        # three particles rounded to a few steps of the subnormal grid, moves for it
        assert K == 1024 or changed(c, want, monkeypatch, no_pos=True)
    if scale in ("big960", "top"):
        assert stats["no_hit"] == 0
