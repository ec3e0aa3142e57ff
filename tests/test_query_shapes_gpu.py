"""Past-tick queries at the shapes the 800-tick parity suites never reach (include/ks_engine.h:
ks_requested_at, ks_cluster_series, ks_node_peaks, ks_headroom_at / _series, ks_usage_at / _digest).

* Hot nodes: 5 nodes (a ragged last workgroup of four-node kernels) that each list far more than 64
  pods, so the lane-stride loops of the peaks and headroom-series kernels take several rounds, with
  windows whose listed count sits on either side of a round boundary, and binds on expiry ticks.
* Long windows: 3,100 ticks on 32 nodes whose every column moves on most ticks, read over windows
  on either side of 1,024 and 2,048 ticks, so the prefix-sum kernels' threads hold chunks of 1, 2
  and 3 ticks and a wrong chunk boundary or carry shows.

Binds come from the C oracle and the states from tests/state_ref.py (pinned to PySim on the CPU by
tests/test_state_ref.py).  What keeps a comparison from being hollow is asserted on the reference
alone, before an engine exists.  Everything is exact integer equality.
"""
import functools

import numpy as np
import pytest

import headroom_ref as hr
import state_ref as sr
import usage_digest as ud
from harness import MODES, assert_same_binds, encoded, make_engine, small_trace
from pysim import PySim

pytestmark = pytest.mark.gpu

GI = (1 << 30) * 1000
MEM_UNIT = 256 * (1 << 20) * 1000      # the generator's memory step, in milli-bytes
FEEDS, LITERAL = "feeds_all_lrba", "literal_lrba_filters_ignored"


def _model(tr, mode):
    """What headroom_ref needs of a checker: PySim's own predicates on the submitted pods."""
    fm, fl, sc = MODES[mode]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    return dict(ps=ps, filter_mode=fm, filters=fl)


def _one(shapes, j):
    return {k: v[j:j + 1] for k, v in shapes.items()}


def _engine(r, ticks):
    eng = make_engine(r["tr"], r["enc"], r["mode"], batch_pods=64)
    eng.submit(r["enc"]["pods"])
    eb = eng.step(ticks)
    assert_same_binds(eb, r["ob"])
    return eng


# ---------------------------------------------------------------------------------------------
# hot nodes
# ---------------------------------------------------------------------------------------------
T_HOT = 1000
HOT = {"feeds": (FEEDS, 6), "literal": (LITERAL, 10)}      # (mode, phase multiplier)
HAND = [
    ([500, -7, 1 << 60], 1, True, False),               # cpu only; junk in the unmasked keys
    ([-1, 3_000_000_000_001, -1], 2, True, False),      # memory only, no multiple of the unit
    ([0, 0, 1000], 4, True, False),                     # gpu only
    ([9, 9, 9], 0, True, False),                        # empty keymask: the pods bound alone
    ([0, 1 << 30, 0], 3, True, False),                  # a request of 0 on a masked key
    ([1000, (1 << 30) * 1000, 0], 3, True, True),       # a selector no node carries
    ([8000, (64 << 30) * 1000, 4000], 7, True, False),  # 8 cpu / 64 Gi / 4 gpu
    ([100, 268_435_456_000, 0], 3, True, False),        # small
    ([30000, 100 * GI, 0], 3, True, False),             # about what a node has free: the count crosses 1
    ([20000, 80 * GI, 0], 3, True, False),
    ([40000, 160 * GI, 0], 3, True, False),
    ([50000, 64 * GI, 0], 3, True, False),
]


def _hot_trace(mult):
    tr = small_trace(31, n_nodes=5, n_pods=T_HOT, arrival="stream", selectors=False, taints=False)
    nd, p = tr["nodes"], tr["pods"]
    cpu = np.array([64, 96, 64, 128, 96])
    nd["alloc"][:, 0] = cpu * 1000
    nd["alloc"][:, 1] = cpu * 4 * GI
    nd["alloc"][:, 2] = 64000            # gpus never bind first: five nodes must take a thousand pods
    nd["alloc"][:, 3] = 110
    nd["alloc_has"][:] = 15
    p["arrival"][:] = 1 + np.arange(p["m"])
    p["phase_sec"][:] = (1 + (np.arange(len(p["phase_sec"])) * 7919) % 97) * mult
    return tr


@functools.lru_cache(maxsize=None)
def _hot(case):
    """The reference of a hot-node case and its windows; every assert here is on the oracle's binds
    alone."""
    mode, mult = HOT[case]
    tr = _hot_trace(mult)
    ob = sr.oracle_binds(tr, MODES[mode], T_HOT)           # asserts rc == 0
    ref = sr.IntervalRef(tr, ob)
    full = (0, T_HOT + 1)
    listed = ref.listed(*full)
    assert (listed >= 130).all(), f"listed pods per node {listed.tolist()}"    # 3 rounds of peaks, 5 of the series
    windows = {}
    for i, k in enumerate((63, 64, 65, 31, 32, 33)):
        w = sr.find_window(ref, k, T_HOT, t_from=40 + 90 * i)
        assert w is not None, f"no window with {k} listed pods on a node"
        assert ref.listed(w[0], w[1])[w[2]] == k and w[0] > 0
        windows[k] = (w[0], w[1])
    used = [full, (1, T_HOT + 1)] + list(windows.values()) + [(0, 1), (0, 2), (417, 418), (417, 419), (T_HOT, T_HOT + 1),
                                                             (T_HOT - 1, T_HOT + 1)]
    same = np.unique(np.concatenate([ref.same_tick_events(lo, hi) for lo, hi in used[2:8]]))
    assert len(same) >= 20, f"only {len(same)} ticks inside the k-windows with a bind and an expiry on one node"
    if case == "literal":
        st = ob["status"]
        assert (st == 1).sum() > 100, "too few OverCapacity binds"
        assert ((st[:-1] == 1) & (st[1:] == 0)).sum() > 30, "the OverCapacity binds do not sit between Ok ones"
    enc = encoded(tr)
    model = _model(tr, mode)
    shapes, sim = hr.make_shapes(tr, enc, model, list(range(0, 52 * 19, 19)), HAND)
    assert len(shapes["keymask"]) == 64
    states = ref.window(*full)
    cols, _ = hr.reference(enc["alloc"], states, shapes, hr.eligibility(model, sim))
    moves = (np.diff(cols[:, :, 1], axis=0) != 0).sum(axis=0)
    assert (moves > 50).sum() >= 3 and ((np.diff(cols[:, :, 0], axis=0) != 0).sum(axis=0) > 300).sum() >= 40
    return dict(tr=tr, enc=enc, mode=mode, ob=ob, ref=ref, windows=windows, used=used, shapes=shapes, states=states,
                cols=cols)


@pytest.fixture(scope="module")
def hot_engines():
    made = {}

    def get(case):
        if case not in made:
            made[case] = _engine(_hot(case), T_HOT)
        return made[case]
    yield get
    for eng in made.values():
        eng.close()


@pytest.mark.parametrize("case", ["feeds", "literal"])
def test_hot_nodes_peaks_and_state(hot_engines, case):
    r = _hot(case)
    eng = hot_engines(case)
    for lo, hi in r["used"]:
        np.testing.assert_array_equal(eng.node_peaks(lo, hi), r["states"][lo:hi].max(axis=0), err_msg=f"peaks [{lo}, {hi})")
        np.testing.assert_array_equal(eng.cluster_series(lo, hi), r["ref"].series(lo, hi), err_msg=f"series [{lo}, {hi})")
    for t in range(0, T_HOT + 1, 7):
        np.testing.assert_array_equal(eng.requested_at(t), r["states"][t], err_msg=f"requested at tick {t}")


@pytest.mark.parametrize("case", ["feeds", "literal"])
def test_hot_nodes_headroom_series(hot_engines, case):
    r = _hot(case)
    eng = hot_engines(case)
    want = r["cols"]
    for lo, hi in r["used"]:
        np.testing.assert_array_equal(eng.headroom_series(lo, hi, r["shapes"]), want[lo:hi, :, :2], err_msg=f"[{lo}, {hi})")
        for j in (0, 63):
            np.testing.assert_array_equal(eng.headroom_series(lo, hi, _one(r["shapes"], j)), want[lo:hi, j:j + 1, :2],
                                          err_msg=f"[{lo}, {hi}) shape {j}")
        for t in (lo, hi - 1):
            np.testing.assert_array_equal(eng.headroom_at(t, r["shapes"]), want[t], err_msg=f"headroom at tick {t}")


# ---------------------------------------------------------------------------------------------
# long windows
# ---------------------------------------------------------------------------------------------
T_LONG = 3100
LENGTHS = (1023, 1024, 1025, 2047, 2048, 2049, 3000)
STRETCH = 256


def _long_trace():
    """32 equal nodes in literal mode.  Pods arrive two per odd tick.  The first of a pair is between
    0.3 and 0.7 of a node and runs for an odd number of ticks, so binds fall on odd and expiries on
    even ticks and never cancel in a column; LeastRequested sends it to an empty node, of which the
    run always has one.  The second asks for more cpu than any node has: bound OverCapacity on the
    even tick, never listed.  So every tick moves the pending count, every odd one the running state
    and the Ok count, every even one the OverCapacity count."""
    tr = small_trace(31, n_nodes=32, n_pods=3200, arrival="stream", selectors=False)
    nd, p = tr["nodes"], tr["pods"]
    i = np.arange(p["m"])
    nd["alloc"][:, 0], nd["alloc"][:, 1], nd["alloc"][:, 2], nd["alloc"][:, 3] = 16000, 64 * GI, 8000, 110
    nd["alloc_has"][:] = 15
    p["arrival"][:] = 1 + 2 * (i // 2)
    first = i % 2 == 0
    p["req"][:, 0] = np.where(first, 4800 + 100 * ((i * 7919) % 65), 200000)
    p["req"][:, 1] = np.where(first, (77 + (i * 104729) % 103) * MEM_UNIT, 8 * GI)
    p["req"][:, 2] = 1000 * (1 + (i // 2) % 2)
    off = p["phase_off"]
    nph = np.diff(off)
    ticks = 15 + 2 * ((i * 7919) % 26)                   # 15 .. 65, odd
    per = ticks // nph
    sec = np.repeat(per, nph) * 10
    sec[off[1:] - 1] += (ticks - per * nph) * 10 - 3     # the last phase ends inside the pod's last tick
    p["phase_sec"][:] = sec
    pct = 25 * (1 + (np.arange(len(sec)) * 31) % 4)
    p["phase_use"][:] = p["req"][np.repeat(i, nph)] * pct[:, None] // 100
    return tr


def _long_shapes():
    rows = [([7600 + 200 * j, 0, 0], 1) for j in range(22)]                       # 0.47 .. 0.74 of a node's cpu
    rows += [([0, (121 + 3 * j) * MEM_UNIT + j % 3, 0], 2) for j in range(22)]     # the same of its memory, some odd
    rows += [([7600 + 300 * j, (121 + 5 * j) * MEM_UNIT, 0], 3) for j in range(16)]
    rows += [([0, 0, 7500], 4), ([0, 0, 8000], 4), ([11000, 170 * MEM_UNIT, 7100], 7), ([11000, 170 * MEM_UNIT, 6500], 7)]
    return [(r, km, True, False) for r, km in rows]


def _moving(col, what):
    """At least a third of every 256-tick stretch of the column changes value."""
    ch = np.diff(col.astype(np.int64)) != 0
    T = len(col)
    starts = list(range(0, T - STRETCH + 1, STRETCH)) + ([T - STRETCH] if T % STRETCH else [])
    for s in starts:
        n = int(ch[s:s + STRETCH - 1].sum())
        assert 3 * n >= STRETCH, f"{what}: only {n} of the {STRETCH} ticks from row {s} change value"


@functools.lru_cache(maxsize=None)
def _long():
    tr = _long_trace()
    ob = sr.oracle_binds(tr, MODES[LITERAL], T_LONG)
    ref = sr.IntervalRef(tr, ob)
    enc = encoded(tr)
    model = _model(tr, LITERAL)
    shapes, sim = hr.make_shapes(tr, enc, model, [], _long_shapes())
    assert len(shapes["keymask"]) == 64
    states = ref.window(0, T_LONG + 1)
    cols, _ = hr.reference(enc["alloc"], states, shapes, hr.eligibility(model, sim))
    series = ref.series(0, T_LONG + 1)
    digest = ud.digest_from_matrices(ref.usage_window(0, T_LONG + 1))
    windows = []
    for T in LENGTHS:
        windows += [(0, T), (min(1037, T_LONG + 1 - T), min(1037, T_LONG + 1 - T) + T)]
    for lo, hi in windows:
        assert lo == 0 or states[lo - 1].any(), "no state is carried into the window"
        for c in range(7):
            _moving(series[lo:hi, c], f"series column {c} over [{lo}, {hi})")
        for c in range(6):
            _moving(digest[lo:hi, c].view(np.int64), f"digest column {c} over [{lo}, {hi})")
        for j in range(64):
            for c in range(2):
                _moving(cols[lo:hi, j, c], f"headroom shape {j} column {c} over [{lo}, {hi})")
    assert len({cols[:, j, :2].tobytes() for j in range(64)}) >= 40, "the shapes' columns barely differ"
    # the shapes that fit twice into an empty node: their two columns differ
    assert sum((cols[:, j, 0] != cols[:, j, 1]).any() for j in range(64)) >= 6
    return dict(tr=tr, enc=enc, mode=LITERAL, ob=ob, ref=ref, shapes=shapes, states=states, cols=cols, series=series,
                digest=digest, windows=windows)


@pytest.fixture(scope="module")
def long_engine():
    eng = _engine(_long(), T_LONG)
    yield eng
    eng.close()


def test_long_windows_cluster_series_and_usage_digest(long_engine):
    r = _long()
    for lo, hi in r["windows"]:
        np.testing.assert_array_equal(long_engine.cluster_series(lo, hi), r["series"][lo:hi], err_msg=f"series [{lo}, {hi})")
        np.testing.assert_array_equal(long_engine.usage_digest(lo, hi), r["digest"][lo:hi], err_msg=f"digest [{lo}, {hi})")


def test_long_windows_headroom_series(long_engine):
    r = _long()
    for lo, hi in r["windows"]:
        np.testing.assert_array_equal(long_engine.headroom_series(lo, hi, r["shapes"]), r["cols"][lo:hi, :, :2],
                                      err_msg=f"[{lo}, {hi})")
        np.testing.assert_array_equal(long_engine.headroom_series(lo, hi, _one(r["shapes"], 5)), r["cols"][lo:hi, 5:6, :2],
                                      err_msg=f"[{lo}, {hi}) one shape")


def test_long_window_rows_equal_the_single_tick_queries(long_engine):
    r = _long()
    eng = long_engine
    lo, hi = r["windows"][-1]
    series, digest = eng.cluster_series(lo, hi), eng.usage_digest(lo, hi)
    head = eng.headroom_series(lo, hi, r["shapes"])
    usage = r["ref"].usage_window(0, T_LONG + 1)
    for t in (lo, lo + 1, 1023 + lo, 1024 + lo, 2047 + lo, 2048 + lo, 2999 + lo, 1500, 2600):
        req = eng.requested_at(t)
        np.testing.assert_array_equal(req, r["states"][t])
        np.testing.assert_array_equal(series[t - lo, :4], req[:, [3, 0, 1, 2]].sum(axis=0))
        u = eng.usage_at(t)
        np.testing.assert_array_equal(u, usage[t])
        np.testing.assert_array_equal(digest[t - lo], ud.digest_from_matrices(u[None])[0])
        at = eng.headroom_at(t, r["shapes"])
        np.testing.assert_array_equal(at, r["cols"][t])
        np.testing.assert_array_equal(head[t - lo], at[:, :2])
