"""CPU pin of tests/state_ref.py (the interval reference the long-run query tests use): equal to
oracle/pysim.py's PySim stepped tick by tick — ``_matrix`` and ``_series_from_model`` of
tests/test_state_queries_gpu.py — on that module's three cases, with the binds taken from the C
oracle.  ``feeds_irregular`` has a negative phase and an int32 wrap.  The usage matrices are pinned
against the C oracle's ``usage()`` after every tick."""
import numpy as np
import pytest

import state_ref as sr
import test_state_queries_gpu as sq
from harness import MODES, make_oracle

T = sq.T


@pytest.fixture(scope="module", params=["feeds", "literal", "feeds_irregular"])
def pinned(request):
    case = request.param
    mode, mult, irregular = sq.CASES[case]
    tr = sq._shared_trace(mult, irregular)
    m = sq._check_model(tr, mode, T)           # PySim, tick by tick: req[t] = _matrix after tick t
    assert m["err"] is None
    sq._assert_trace_properties(case, tr, m)
    ora = make_oracle(tr, mode)
    ora.submit(tr)
    binds = {f: [] for f in ("pod", "node", "tick", "status")}
    usage = [np.zeros((m["n"], 3), np.int64)]
    for _ in range(T):
        ob, rc = ora.step(1)
        assert rc == 0
        for f in binds:
            binds[f] += ob[f].tolist()
        usage.append(ora.usage())
    ob = {f: np.array(v, np.int64) for f, v in binds.items()}
    b = m["binds"]
    for i, f in enumerate(("pod", "node", "tick", "status")):
        np.testing.assert_array_equal(ob[f], b[:, i])
    return dict(case=case, tr=tr, m=m, ref=sr.IntervalRef(tr, ob), usage=np.stack(usage), mode=mode, ob=ob)


def test_one_call_of_the_oracle_gives_the_same_binds(pinned):
    ob = sr.oracle_binds(pinned["tr"], MODES[pinned["mode"]], T)
    for f in ("pod", "node", "tick", "status"):
        np.testing.assert_array_equal(ob[f], pinned["ob"][f])


def test_matrices_equal_pysim_at_every_tick(pinned):
    ref, want = pinned["ref"], pinned["m"]["req"]
    np.testing.assert_array_equal(ref.window(0, T + 1), want)
    np.testing.assert_array_equal(ref.window(300, 500), want[300:500])      # state carried in
    np.testing.assert_array_equal(ref.window(T, T + 1), want[T:])
    for t in (0, 1, 137, 417, T):
        np.testing.assert_array_equal(ref.at(t), want[t])
    if pinned["case"] == "feeds_irregular":
        # the pod whose int32 sum wraps below zero never runs
        d, p = ref.dur_all, pinned["tr"]["pods"]
        tot = np.add.reduceat(np.asarray(p["phase_sec"], np.int64), np.asarray(p["phase_off"][:-1], np.int64))
        assert (tot >= 2**31).any() and (d[tot >= 2**31] == 0).all()
        assert (np.asarray(p["phase_sec"]) < 0).any()


def test_series_equal_the_columns_rebuilt_from_pysim(pinned):
    ref = pinned["ref"]
    want = sq._series_from_model(pinned["tr"], pinned["m"])
    np.testing.assert_array_equal(ref.series(0, T + 1), want)
    np.testing.assert_array_equal(ref.series(300, 500), want[300:500])
    np.testing.assert_array_equal(ref.series(1, 2), want[1:2])


def test_peaks_and_listed_pods(pinned):
    ref, req = pinned["ref"], pinned["m"]["req"]
    b = pinned["m"]["binds"]
    d = ref.dur_all
    for lo, hi in ((0, T + 1), (1, T + 1), (300, 500), (417, 418), (799, 801)):
        np.testing.assert_array_equal(ref.peaks(lo, hi), req[lo:hi].max(axis=0))
        k = np.zeros(ref.n, np.int64)
        for pod, node, tick, status in b.tolist():          # the rule, pod by pod
            if status == 0 and d[pod] > 0 and tick <= hi - 1 and tick + d[pod] > lo:
                k[node] += 1
        np.testing.assert_array_equal(ref.listed(lo, hi), k)
    for kk in (3, 7):
        w = sr.find_window(ref, kk, T)
        assert w is not None and ref.listed(w[0], w[1])[w[2]] == kk


def test_same_tick_events_are_binds_on_expiry_ticks(pinned):
    ref = pinned["ref"]
    got = ref.same_tick_events(0, T + 1)
    want = set()
    ends = {}
    for node, e, d in zip(ref.node.tolist(), ref.e.tolist(), ref.dur.tolist()):
        if d > 0:
            ends.setdefault(node, set()).add(e)
    for node, b, d in zip(ref.node.tolist(), ref.b.tolist(), ref.dur.tolist()):
        if d > 0 and b in ends.get(node, ()) and 0 < b < T + 1:
            want.add(b)
    assert sorted(want) == got.tolist()


def test_usage_equals_the_oracle_after_every_tick(pinned):
    ref = pinned["ref"]
    np.testing.assert_array_equal(ref.usage_window(0, T + 1), pinned["usage"])
    np.testing.assert_array_equal(ref.usage_window(300, 500), pinned["usage"][300:500])
    assert (np.diff(pinned["usage"].sum(axis=(1, 2))) != 0).sum() > 300
