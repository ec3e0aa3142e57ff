"""GPU parity of the headroom queries (include/ks_engine.h: ks_headroom_at, ks_headroom_series)
against oracle/pysim.py PySim stepped tick by tick: the [n][4] requested matrix after every tick's
bind, the trace's alloc and PySim's own taint / selector predicates give, in Python integers
(tests/headroom_ref.py), every count, limiting key and column.  Everything is exact integer equality.

Each reference is built once (``_model``, cached), checked on its own for the properties that keep
the comparison from passing vacuously, and never mutated afterwards.
"""
import functools
from math import gcd

import numpy as np
import pytest

import headroom_ref as hr
from harness import MODES, assert_same_binds, encoded, make_engine, small_trace

pytestmark = pytest.mark.gpu

T = 800
FEEDS, LITERAL = "feeds_all_lrba", "literal_lrba_filters_ignored"
# (mode, phase multiplier, irregular phases).  Literal mode ignores the fit filter, so nodes fill up and
# many binds are OverCapacity (they never count); with longer pods (the state-query tests' x8) too few
# pods run for 50 ticks to carry an expiry on a bind tick, which the series test needs.
CASES = {"feeds": (FEEDS, 1, False), "literal": (LITERAL, 1, False), "feeds_irregular": (FEEDS, 1, True)}
MEM_ODD = 3_000_000_000_001   # a memory request that is no multiple of the engine's memory unit (asserted)

# hand-made shapes: (req, keymask, tolerates every taint, selector no node carries).  Values in
# unmasked keys are junk on purpose: they must be ignored.
HAND = [
    ([500, -7, 1 << 60], 1, True, False),               # cpu only
    ([-1, MEM_ODD, -1], 2, True, False),                # memory only, not a multiple of the unit
    ([0, 0, 1000], 4, True, False),                     # gpu only
    ([9, 9, 9], 0, True, False),                        # empty keymask: the pods bound alone
    ([0, 1 << 30, 0], 3, True, False),                  # a request of 0 on a masked key
    ([1000, (1 << 30) * 1000, 0], 3, False, False),     # tolerates nothing
    ([1000, (1 << 30) * 1000, 0], 3, True, True),       # a selector no node carries
    ([8000, (64 << 30) * 1000, 4000], 7, True, False),  # 8 cpu / 64 Gi / 4 gpu
    ([100, 268_435_456_000, 0], 3, True, False),        # small
]


def _slice(shapes, idx):
    return {k: v[idx] for k, v in shapes.items()}


def _build(tr, mode, ticks, pod_ids, hand=HAND):
    enc = encoded(tr)
    m = hr.step_model(tr, MODES[mode], ticks)
    shapes, sim = hr.make_shapes(tr, enc, m, pod_ids, hand)
    elig = hr.eligibility(m, sim)
    cols, counts = hr.reference(enc["alloc"], m["req"], shapes, elig)
    return dict(tr=tr, enc=enc, m=m, shapes=shapes, elig=elig, cols=cols, counts=counts)


@functools.lru_cache(maxsize=None)
def _model(case):
    mode, mult, irregular = CASES[case]
    tr = hr.shared_trace(mult, irregular)
    r = _build(tr, mode, T, list(range(0, 24 * 33, 33)))
    assert r["m"]["err"] is None and len(r["shapes"]["keymask"]) == 33
    _assert_not_vacuous(case, r)
    return r


def _assert_not_vacuous(case, r):
    cols, elig, enc = r["cols"], r["elig"], r["enc"]
    for c in range(4, 8):
        assert (cols[:, :, c] > 0).any(), f"limiting-key column {c} is zero everywhere"
    if CASES[case][0] == FEEDS:
        assert (cols[:, :, 8] > 0).any(), "no ineligible node in feeds mode"
        assert 0 < elig[29].sum() < elig.shape[1] and elig[30].sum() == 0
    else:
        assert (cols[:, :, 8] == 0).all(), "an ineligible node in literal mode"
        assert (r["m"]["binds"][:, 3] == 1).sum() > 100, "too few OverCapacity binds"
    assert (cols[:, :, 1] < elig.sum(axis=1)[None, :]).any(), "every eligible node always has room"
    changes = (np.diff(cols[:, :, 0], axis=0) != 0).sum(axis=0)
    assert (changes > 100).sum() >= 8, f"column 0 moves on too few ticks: {sorted(changes)[-8:]}"
    # the engine's memory unit is the gcd of every memory quantity it was given
    unit = 0
    for v in list(enc["alloc"][:, 1]) + list(enc["pods"]["req"][:, 1]):
        unit = gcd(unit, int(v)) if v > 0 else unit
    assert unit > 1 and MEM_ODD % unit != 0
    # the series' dedupe path: ticks on which a node has both a bind and an expiry
    ends, both = {}, set()
    for node, a, b in hr.run_ticks(r["m"]):
        ends.setdefault(node, set()).add(b)
    for node, a, b in hr.run_ticks(r["m"]):
        if a in ends[node] and a <= T:
            both.add((node, a))
    assert len({t for _, t in both}) >= 50, f"only {len(both)} ticks with an expiry on a bind tick"


def _engine_run(tr, mode, ticks=T, batch_pods=64, engine_flags=0, shard=None):
    enc = encoded(tr)
    eng = make_engine(tr, enc, mode, batch_pods=batch_pods, engine_flags=engine_flags, shard=shard)
    eng.submit(enc["pods"])
    return eng, eng.step(ticks)


def _same_binds(eb, m):
    b = m["binds"]
    assert_same_binds(eb, dict(pod=b[:, 0], node=b[:, 1], tick=b[:, 2], status=b[:, 3]))


class _Runs:
    """The batched engine run of each case, made on first use and shared by the read-only tests."""

    def __init__(self):
        self.made = {}

    def __call__(self, case):
        if case not in self.made:
            r = _model(case)
            eng, eb = _engine_run(r["tr"], CASES[case][0])
            assert eng.last_step_stats()["launches"] > 10
            _same_binds(eb, r["m"])
            self.made[case] = eng
        return self.made[case]


@pytest.fixture(scope="module")
def runs():
    r = _Runs()
    yield r
    for eng in r.made.values():
        eng.close()


def _check_at(eng, r, t, shapes=None, sel=slice(None)):
    out, pn = eng.headroom_at(t, r["shapes"] if shapes is None else shapes, per_node=True)
    np.testing.assert_array_equal(pn, r["counts"][t][sel], err_msg=f"per-node counts at tick {t}")
    np.testing.assert_array_equal(out, r["cols"][t][sel], err_msg=f"columns at tick {t}")
    assert (out[:, 4:9].sum(axis=1) == eng.n).all()


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_headroom_at_every_tick_of_one_batched_step(runs, case):
    r = _model(case)
    eng = runs(case)
    for t in range(0, T + 1):
        _check_at(eng, r, t)
    # without per_node the columns are the same
    np.testing.assert_array_equal(eng.headroom_at(417, r["shapes"]), r["cols"][417])


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_headroom_series_matches_the_per_tick_columns(runs, case):
    from kubesim_amd.engine import KsError
    r = _model(case)
    eng = runs(case)
    want = r["cols"][:, :, :2]   # [tick][k][2]
    for lo, hi in ((1, T + 1), (0, 3), (300, 500), (T, T + 1)):
        np.testing.assert_array_equal(eng.headroom_series(lo, hi, r["shapes"]), want[lo:hi], err_msg=f"[{lo}, {hi})")
        for j in (0, 27):     # K = 1: a trace pod's shape and the empty keymask
            one = _slice(r["shapes"], slice(j, j + 1))
            np.testing.assert_array_equal(eng.headroom_series(lo, hi, one), want[lo:hi, j:j + 1],
                                          err_msg=f"[{lo}, {hi}) shape {j}")
    for lo, hi in ((10, 10), (20, 10), (1, T + 2), (T + 1, T + 2), (-1, 5)):
        with pytest.raises(KsError):
            eng.headroom_series(lo, hi, r["shapes"])


def test_headroom_series_rejects_more_than_2_22_shape_ticks():
    from kubesim_amd.engine import KsError
    tr = hr.shared_trace(1, n_nodes=16, n_pods=50)
    eng, _ = _engine_run(tr, FEEDS, ticks=(1 << 16) + 8)
    enc = encoded(tr)
    shapes = {k: np.concatenate([enc["pods"][k][:50], enc["pods"][k][:14]]) for k in ("req", "keymask", "tol", "sel")}
    full = eng.headroom_series(8, (1 << 16) + 8, shapes)      # 64 x 2^16 = 2^22: allowed
    assert full.shape == (1 << 16, 64, 2)
    at = eng.headroom_at((1 << 16) + 7, shapes)
    np.testing.assert_array_equal(full[-1], at[:, :2])
    np.testing.assert_array_equal(full[0], eng.headroom_at(8, shapes)[:, :2])
    with pytest.raises(KsError):
        eng.headroom_series(7, (1 << 16) + 8, shapes)         # 64 x (2^16 + 1)
    one = _slice(shapes, slice(0, 1))
    assert eng.headroom_series(7, (1 << 16) + 8, one).shape == ((1 << 16) + 1, 1, 2)
    eng.close()


@functools.lru_cache(maxsize=None)
def _model_600():
    """600 nodes: three 256-node workgroups, the last with 88 nodes; K = 64."""
    tr = small_trace(5, n_nodes=600, n_pods=400, arrival="stream", selectors=False)
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 997
    mode = (1, 7, ((1, 2, 0),))
    enc = encoded(tr)
    m = hr.step_model(tr, mode, 400)
    assert m["err"] is None
    shapes, sim = hr.make_shapes(tr, enc, m, list(range(0, 55 * 7, 7)), HAND)
    elig = hr.eligibility(m, sim)
    ticks = [150, 400] + list(range(250, 350))
    sub = m["req"][ticks]
    # reference rows in the order of ``ticks`` (every row is computed from its own state)
    cols, counts = hr.reference(enc["alloc"], sub, shapes, elig)
    return dict(tr=tr, enc=enc, m=m, mode=mode, shapes=shapes, cols=cols, counts=counts, ticks=ticks)


def test_three_workgroups_ragged_tail_64_shapes():
    r = _model_600()
    assert len(r["shapes"]["keymask"]) == 64
    # column 3's lowest-index rule: some shape's maximum is attained in two different workgroups
    c150 = r["counts"][0]
    spans = [np.unique(np.nonzero(c150[j] == c150[j].max())[0] // 256) for j in range(64) if c150[j].max() > 0]
    assert any(len(s) >= 2 for s in spans)
    assert (c150[:, 512:] > 0).any() and (r["cols"][:, :, 8] > 0).any()
    eng, eb = _engine_run(r["tr"], r["mode"], ticks=400)
    _same_binds(eb, r["m"])
    for row, t in enumerate(r["ticks"][:2]):
        out, pn = eng.headroom_at(t, r["shapes"], per_node=True)
        np.testing.assert_array_equal(pn, r["counts"][row])
        np.testing.assert_array_equal(out, r["cols"][row])
    np.testing.assert_array_equal(eng.headroom_series(250, 350, r["shapes"]), r["cols"][2:, :, :2])
    eng.close()


def test_series_equals_headroom_at_past_the_series_grid_cap():
    """4,500 nodes are more than the series kernel's grid covers in one pass (1,024 workgroups of
    four nodes), so its waves stride over nodes.  headroom_at is checked against the checker above;
    here the series must equal it tick by tick."""
    tr = small_trace(6, n_nodes=4500, n_pods=300, arrival="stream", selectors=False)
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 997
    eng, eb = _engine_run(tr, (1, 7, ((1, 2, 0),)), ticks=300)
    assert len(eb) > 250
    enc = encoded(tr)
    shapes = {k: np.ascontiguousarray(enc["pods"][k][:300:25]) for k in ("req", "keymask", "tol", "sel")}
    for lo, hi in ((0, 40), (200, 301)):
        want = np.stack([eng.headroom_at(t, shapes)[:, :2] for t in range(lo, hi)])
        assert (np.diff(want[:, :, 0], axis=0) != 0).any()
        np.testing.assert_array_equal(eng.headroom_series(lo, hi, shapes), want)
    out, pn = eng.headroom_at(300, shapes, per_node=True)
    assert (pn[:, 4096:] > 0).any() and (out[:, 4:].sum(axis=1) == 4500).all()
    eng.close()


# ---------------------------------------------------------------------------------------------
# domain edges on the device: a hand-made cluster and hand-made pods, no trace
# ---------------------------------------------------------------------------------------------
TOP = (1 << 59) - 1
MEM_UNIT = (1 << 30) * 1000      # every memory quantity of the edge cluster is a multiple of it
EDGE_MODE = (1, 1, ((1, 1, 0),))  # the fit filter feeds LeastRequested


def _edge_cluster():
    cpus = [TOP, TOP - 1, 1 << 58, (1 << 53) + 1, 1 << 53, (1 << 53) - 1, ((1 << 31) - 1) * 1000,
            ((1 << 31) - 2) * 1000 + 999, (1 << 22) + 1, 1 << 22, (1 << 22) - 1, 128000, 8000, 1000, 999, 1, 0, -1]
    mems = [TOP // MEM_UNIT * MEM_UNIT, (1 << 18) * MEM_UNIT, 4096 * MEM_UNIT, 512 * MEM_UNIT, 7 * MEM_UNIT, MEM_UNIT, 0, -1]
    gpus = [8000, 1000, 0, -1, (1 << 31) * 1000]
    aps = [110, 0, 1, 3, TOP, (1 << 31) - 1, 1 << 31, (1 << 31) - 2]
    rows = []
    for i in range(300):
        rows.append([cpus[i % len(cpus)], mems[(i // 3) % len(mems)], gpus[(i // 7) % len(gpus)], aps[(i // 2) % len(aps)]])
    return np.array(rows, np.int64)


def _edge_pods(m=30):
    req = np.zeros((m, 3), np.int64)
    req[:, 0] = [(1 << 57) + 1, 1 << 56, 3, 1000, (1 << 52) + 5, 7][:6] * (m // 6)
    req[:, 1] = [MEM_UNIT * x for x in (1 << 17, 3, 1, 500, 4000, 2)] * (m // 6)
    return dict(m=m, arrival=np.zeros(m, np.int64), req=req, keymask=np.full(m, 3, np.uint8),
                tol=np.zeros(m, np.uint64), sel=np.zeros(m, np.uint64), phase_off=np.arange(m + 1, dtype=np.int32),
                phase_sec=np.full(m, 100_000, np.int32), phase_use=np.zeros((m, 3), np.int64),
                flags=np.zeros(m, np.uint8))


def _edge_shapes(alloc, r10):
    f_max, d_max, q_clamp, clamp = 1 << 22, 1 << 53, 1 << 28, hr.NODE_MAX
    rows = []
    for q in (1, 2, 3, 1000, f_max - 1, f_max, f_max + 1, q_clamp - 1, q_clamp, q_clamp + 1, d_max - 1, d_max, d_max + 1,
              TOP // clamp, TOP // clamp + 1, (TOP - 1) // (clamp + 1), (1 << 58) // clamp, TOP - 1, TOP):
        rows.append(([q, 0, 0], 1))
    for q in (1, MEM_UNIT - 1, MEM_UNIT, MEM_UNIT + 1, 7 * MEM_UNIT + 3, (1 << 18) * MEM_UNIT // clamp,
              (1 << 18) * MEM_UNIT // clamp + 1, 3 * MEM_UNIT + 1, TOP):   # MEM_UNIT +- 1: coprime to the unit
        rows.append(([0, q, 0], 2))
    for q in (1, 1000, 1001, 0):
        rows.append(([0, 0, q], 4))
    rows += [([1000, MEM_UNIT + 1, 0], 3), ([3, 1, 1], 7), ([0, 0, 0], 7), ([0, 0, 0], 0), ([1 << 57, MEM_UNIT, 1000], 7)]
    # the free amount of a used node at tick 10, exactly and off by one
    used = np.nonzero(r10[:, 0] > 0)[0]
    for nd in used[:3]:
        free = int(alloc[nd, 0]) - int(r10[nd, 0])
        for q in (free, free + 1, max(free // 2, 1), max(free // clamp, 1)):
            rows.append(([min(q, TOP), 0, 0], 1))
    rows = rows[:64]
    k = len(rows)
    return dict(req=np.array([r for r, _ in rows], np.int64), keymask=np.array([m for _, m in rows], np.uint8),
                tol=np.zeros(k, np.uint64), sel=np.zeros(k, np.uint64))


def test_domain_edges_and_no_state_change():
    from kubesim_amd.engine import Engine
    alloc = _edge_cluster()
    pods = _edge_pods()
    zeros = np.zeros(len(alloc), np.uint64)

    def fresh():
        fm, fl, sc = EDGE_MODE
        e = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(alloc, zeros, zeros)
        e.submit(pods)
        return e, e.step(10)
    eng, b = fresh()
    twin, tb = fresh()
    assert len(b) == 10 and (b["status"] == 0).all()
    # the state at tick 10 from the binds alone: every pod runs for 10,000 ticks
    r10 = np.zeros((len(alloc), 4), np.int64)
    for pod, node in zip(b["pod"].tolist(), b["node"].tolist()):
        r10[node, :3] += pods["req"][pod]
        r10[node, 3] += 1
    assert (r10[:, 0] > 0).sum() >= 3
    shapes = _edge_shapes(alloc, r10)
    elig = np.ones((len(shapes["keymask"]), len(alloc)), bool)
    cols, counts = hr.reference(alloc, np.stack([np.zeros_like(r10), r10]), shapes, elig)
    assert (counts == hr.NODE_MAX).any() and (counts == hr.NODE_MAX - 1).any() and (counts == 0).any()
    for c in range(4, 8):
        assert (cols[:, :, c] > 0).any()
    for row, t in ((0, 0), (1, 10)):
        out, pn = eng.headroom_at(t, shapes, per_node=True)
        np.testing.assert_array_equal(pn, counts[row], err_msg=f"tick {t}")
        np.testing.assert_array_equal(out, cols[row], err_msg=f"tick {t}")
    np.testing.assert_array_equal(eng.headroom_series(0, 11, shapes)[[0, 10]], cols[:, :, :2])
    # a shape rescaled nothing: the state reads back as before and the run goes on as its twin's
    np.testing.assert_array_equal(eng.requested_at(10), r10)
    np.testing.assert_array_equal(eng.requested_at(10), twin.requested_at(10))
    nb, ntb = eng.step(10), twin.step(10)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    np.testing.assert_array_equal(eng.requested_at(20), twin.requested_at(20))
    eng.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# independence from the chain
# ---------------------------------------------------------------------------------------------
def test_headroom_answers_after_an_aborted_run():
    from kubesim_amd.engine import KsError
    tr = small_trace(9)   # 15 binds, then a pod whose selector no node carries
    r = _build(tr, FEEDS, 200, list(range(12)))
    m = r["m"]
    assert m["err"] == "NotFound" and len(m["binds"]) >= 8
    eng = make_engine(tr, r["enc"], FEEDS, batch_pods=64)
    eng.submit(r["enc"]["pods"])
    with pytest.raises(KsError) as ex:
        eng.step(200)
    assert ex.value.kind == "NotFound"
    _same_binds(ex.value.binds, m)
    now = eng.tick
    assert now == m["tick"] == len(m["req"]) - 1
    for t in range(0, now + 1):
        _check_at(eng, r, t)
    np.testing.assert_array_equal(eng.headroom_series(0, now + 1, r["shapes"]), r["cols"][:, :, :2])
    with pytest.raises(KsError):
        eng.headroom_at(now + 1, r["shapes"])
    eng.close()


def test_group_members_answer_for_their_own_scenario():
    from kubesim_amd.engine import Group
    fm, fl, sc = MODES[FEEDS]
    g = Group(2)
    refs, engs = [], []
    for seed in (11, 12):
        tr = small_trace(seed, n_nodes=24, n_pods=200, arrival="stream", selectors=False)
        tr["pods"]["phase_sec"][:] = 1 + (np.arange(len(tr["pods"]["phase_sec"])) * 7919) % 97
        r = _build(tr, FEEDS, 200, list(range(0, 200, 20)))
        e = g.add(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(r["enc"]["alloc"], r["enc"]["taint"], r["enc"]["label"])
        e.submit(r["enc"]["pods"])
        refs.append(r)
        engs.append(e)
    binds, counts, st, _ = g.step(200)
    assert (st == 0).all()
    for r, e, eb in zip(refs, engs, g.split(binds, counts)):
        assert r["m"]["err"] is None
        _same_binds(eb, r["m"])
        for t in (0, 77, 200):
            _check_at(e, r, t)
        np.testing.assert_array_equal(e.headroom_series(1, 201, r["shapes"]), r["cols"][1:, :, :2])
    g.close()


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_node_shards"])
def test_other_resolver_gives_identical_headroom(runs, how):
    from kubesim_amd import _lib
    r = _model("feeds")
    if how == "one_pod_resolver":
        oth, ob = _engine_run(r["tr"], FEEDS, engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER)
    else:
        oth, ob = _engine_run(r["tr"], FEEDS, shard=(1, 0, None, 2))
    _same_binds(ob, r["m"])
    for t in (1, 137, 417, T):
        _check_at(oth, r, t)
    np.testing.assert_array_equal(oth.headroom_series(300, 500, r["shapes"]), r["cols"][300:500, :, :2])
    np.testing.assert_array_equal(oth.headroom_series(300, 500, r["shapes"]), runs("feeds").headroom_series(300, 500, r["shapes"]))
    oth.close()


# ---------------------------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------------------------
def test_argument_errors(runs):
    from kubesim_amd.engine import Engine, KsError
    r = _model("feeds")
    eng = runs("feeds")
    ok = _slice(r["shapes"], slice(0, 4))
    assert eng.headroom_at(T, ok).shape == (4, 9)

    def shapes(k, **over):
        s = dict(req=np.tile(np.array([[1000, 1 << 30, 0]], np.int64), (k, 1)), keymask=np.full(k, 3, np.uint8),
                 tol=np.zeros(k, np.uint64), sel=np.zeros(k, np.uint64))
        s.update(over)
        return s
    bad = {
        "k = 0": shapes(0),
        "k = 65": shapes(65),
        "keymask 8": shapes(2, keymask=np.array([3, 8], np.uint8)),
        "negative masked request": shapes(2, req=np.array([[1000, 5, 0], [-1, 5, 0]], np.int64)),
        "masked request of 2^59": shapes(2, req=np.array([[1000, 5, 0], [1000, 1 << 59, 0]], np.int64)),
    }
    for what, s in bad.items():
        with pytest.raises(KsError) as ex:
            eng.headroom_at(T, s)
        assert ex.value.kind == "InvalidArgument", what
        with pytest.raises(KsError):
            eng.headroom_series(1, 5, s)
    assert eng.headroom_at(T, shapes(64)).shape == (64, 9)
    # the same values in an unmasked key are ignored
    junk = shapes(2, req=np.array([[1000, 5, -1], [1000, 5, 1 << 59]], np.int64))
    np.testing.assert_array_equal(eng.headroom_at(T, junk), eng.headroom_at(T, shapes(2, req=np.array([[1000, 5, 0]] * 2, np.int64))))
    for t in (T + 1, -1):
        with pytest.raises(KsError):
            eng.headroom_at(t, ok)
    # the failed calls changed nothing
    _check_at(eng, r, T)
    fm, fl, sc = MODES[FEEDS]
    empty = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    with pytest.raises(KsError):
        empty.headroom_at(0, ok)          # no nodes loaded
    with pytest.raises(KsError):
        empty.headroom_series(0, 1, ok)
    z = np.zeros(0, np.uint64)
    empty.load_nodes(np.zeros((0, 4), np.int64), z, z)
    out = empty.headroom_at(0, ok)        # n = 0: zeros, column 3 = -1
    want = np.zeros((4, 9), np.int64)
    want[:, 3] = -1
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(empty.headroom_series(0, 1, ok), np.zeros((1, 4, 2), np.int64))
    empty.close()
