"""The two references of the drain preview (tests/drain_ref.py) agree on the shared 32-node trace:
oracle/pysim.py's PySim without the drained nodes, asked pod after pod, and the integer walk
``fast_drain`` the GPU tests use on the larger clusters.  Exact integer equality; no device."""
import numpy as np
import pytest

import drain_ref as dr
import place_ref as pr

N = 32
SETS = {"first": [0], "last": [31], "every_third": list(range(0, N, 3)), "all": list(range(N))}


_sim_at, _state = dr.sim_at, dr.sim_state


def test_rebuilt_pysim_state_is_the_runs_own():
    """drain_ref.sim_at's shortcut gives the state place_ref's stepped PySim had: the `after` of a preview
    that places nothing new is that state, and place_ref kept it per tick."""
    r = pr.parity_case("feeds")
    for t in pr.TICKS:
        ps = _sim_at("feeds", t)
        placed = r["slow"][t]
        want = placed["after"].copy()
        for i in np.nonzero(placed["status"] == pr.OK)[0]:
            j = int(r["shape_of"][i])
            km = int(r["shapes"]["keymask"][j])
            for c in range(3):
                if (km >> c) & 1:
                    want[placed["node"][i], c] -= int(r["shapes"]["req"][j][c])
            want[placed["node"][i], 3] -= 1
        np.testing.assert_array_equal(_state(ps, t), want)


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_integer_walk_equals_pysim(case):
    r = pr.parity_case(case)
    enc = r["enc"]
    cfg = pr.engine_cfg(__import__("harness").MODES[r["mode"]], enc)
    binds = dict(pod=r["binds"][:, 0], node=r["binds"][:, 1], tick=r["binds"][:, 2], status=r["binds"][:, 3])
    seen = dict(ok=0, over=0, none=0, reused=0, evicted=0, idle=0)
    for t in pr.TICKS:
        ps = _sim_at(case, t)
        state = _state(ps, t)
        for name, drained in SETS.items():
            slow = dr.pysim_drain(ps, t, drained)
            ev, frm = slow["pod"].tolist(), slow["from_node"].tolist()
            if case != "feeds_irregular":
                ev2, frm2 = dr.running_on(r["tr"], enc, binds, t, drained)
                assert (ev2, frm2) == (ev, frm), (case, t, name)
            fast = dr.fast_drain(enc["alloc"], state, cfg, enc["pods"], ev, frm, drained)
            dr.assert_same(fast, slow, f"{case} tick {t} set {name}")
            assert fast["reused"] == slow["reused"]
            assert not slow["after"][drained].any()
            if name == "all":
                assert (slow["status"] == pr.NOT_FOUND).all() and (slow["candidates"] == 0).all() and not slow["after"].any()
            if case == "literal":
                assert (slow["candidates"] == N - len(drained)).all()
            seen["ok"] += slow["info"][1]
            seen["over"] += slow["info"][2]
            seen["none"] += slow["info"][3]
            seen["reused"] += len(slow["reused"])
            seen["evicted"] += len(ev)
            seen["idle"] += slow["info"][5]
    # the comparison cannot pass by every pod doing the same thing (about eight pods run at a time on
    # this trace: every outcome occurs, the dense trace below has the numbers)
    assert seen["evicted"] >= 40 and seen["ok"] >= 5 and seen["none"] >= 20 and seen["reused"] >= 1, seen
    assert seen["idle"] >= 1, seen
    if case == "literal":
        assert seen["over"] >= 3, seen


def test_integer_walk_equals_pysim_on_a_dense_trace():
    """The same recipe with phases three times as long (at four times the run stops with NotFound):
    some forty pods run at a time, so a drain evicts tens of pods, fills nodes and comes back to nodes
    it changed."""
    import headroom_ref as hr
    from harness import MODES, encoded
    from pysim import PySim
    tr = hr.shared_trace(3, n_pods=300)
    enc = encoded(tr)
    fm, fl, sc = MODES[pr.FEEDS]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    binds, err = ps.step(300)
    assert err is None
    cfg = pr.engine_cfg(MODES[pr.FEEDS], enc)
    state = _state(ps, 300)
    assert state[:, 3].sum() >= 30
    b = np.array(binds, np.int64).reshape(-1, 4)
    bd = dict(pod=b[:, 0], node=b[:, 1], tick=b[:, 2], status=b[:, 3])
    tot = dict(ok=0, none=0, reused=0)
    for name, drained in (("every_third", SETS["every_third"]), ("upper half", list(range(16, 32))),
                          ("all but three", list(range(3, 32)))):
        slow = dr.pysim_drain(ps, 300, drained)
        ev, frm = dr.running_on(tr, enc, bd, 300, drained)
        fast = dr.fast_drain(enc["alloc"], state, cfg, enc["pods"], ev, frm, drained)
        dr.assert_same(fast, slow, name)
        assert fast["reused"] == slow["reused"]
        tot["ok"] += slow["info"][1]
        tot["none"] += slow["info"][3]
        tot["reused"] += len(slow["reused"])
    assert tot["ok"] >= 30 and tot["none"] >= 20 and tot["reused"] >= 10, tot


def test_score_vector_equals_the_scalar_formula():
    """fast_drain's whole-cluster score vector against place_ref's one-node ``_total1``, also where
    BalancedAllocation's products leave 64 bits."""
    rng = np.random.default_rng(20261020)
    for i in range(60):
        n = int(rng.integers(1, 80))
        big = i % 3 == 0
        top = (1 << 55) if big else (1 << 20)
        A = rng.integers(1, top, size=(n, 4))
        A[:, 3] = rng.choice([110, 3, 1, 0], size=n)
        A[rng.random(n) < 0.1, int(rng.integers(3))] = -1
        A[rng.random(n) < 0.05, int(rng.integers(2))] = 0
        S = np.zeros((n, 4), np.int64)
        for c in range(3):
            S[:, c] = np.maximum(A[:, c], 0) // rng.integers(1, 6, n)
        S[:, 3] = rng.integers(0, 4, n)
        taint = rng.integers(0, 8, n).astype(np.uint64)
        label = rng.integers(0, 8, n).astype(np.uint64)
        live = rng.random(n) < 0.8
        cfg = dict(filter_mode=int(rng.integers(2)), filters=int(rng.choice([7, 1, 6, 0])),
                   scorers=((0, 1, int(rng.integers(4))), (1, int(rng.integers(1, 3)), 0), (2, int(rng.integers(1, 3)), 0)),
                   taint=taint, label=label)
        km = int(rng.choice([3, 7, 1, 2]))
        req = [int(rng.integers(0, top // 4)) if (km >> c) & 1 else 0 for c in range(3)]
        shape = (req, km, int(rng.integers(0, 8)), int(rng.integers(0, 4)))
        got = dr.score_vector(cfg, A, S, taint, label, live, shape)
        want = [pr._total1(cfg, A[j].tolist(), S[j].tolist(), int(taint[j]), int(label[j]), shape) if live[j] else 0
                for j in range(n)]
        assert got.tolist() == want, i
