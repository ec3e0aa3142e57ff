"""ks_submit_pods' two upload paths and submits between steps (ks_engine.cpp):
one trace, encoded once and submitted as slices of the encoded arrays (phase_off re-based per slice),
must schedule the same however it is cut.

Engine A submits all 4,200 pods in one call: past the 4,096-pod staging limit, so the direct copies.
Engine B submits slices of 1, 7, 4,096 and 96 pods: the staged path, with the arena's growth and the
rewrites of phase_off's and exp_off's sentinels.  Engine C submits 500 pods, steps 300 ticks, submits
the other 3,700 and steps to the end, against an oracle fed and stepped the same way: expiries one
call left pending attach to the next call's pods.  The stream's arrivals run just ahead of the pod
index, so after 300 ticks no later pod is late; the same with 700 ticks in between has the arrivals of
some two hundred pods below tick + 1, which the bind-tick recurrence clamps.

Binds, statuses and ticks against the oracle (integer work: no tolerance); usage_at at three ticks and
pod_status over all pods equal between A and B.  The oracles run once per seed and are shared.
"""
import numpy as np
import pytest

from harness import assert_same_binds, encoded, make_engine, make_oracle, oracle_run, small_trace
from kubesim_amd import tracegen
from kubesim_amd.kubesim import slice_encoded

pytestmark = pytest.mark.gpu

MODE = "feeds_all_lrba"
PODS, FIRST, GAPS = 4200, 500, (300, 700)
TICKS = 6000  # past every bind tick of either feeding (the single-submit runs end at 4,352 and 4,244)
B_SLICES = (1, 7, 4096, 96)
_cases = {}


def _case(seed):
    """(trace, encoded trace, the single-submit oracle's binds, per gap the split-feed oracle's binds of its two steps)."""
    if seed not in _cases:
        tr = small_trace(seed, n_nodes=1500, n_pods=PODS, arrival="stream", selectors=False, taints=False)
        ora = make_oracle(tr, MODE)
        ora.submit(tr)
        whole, rc = oracle_run(ora, TICKS)
        assert rc == 0 and len(whole["pod"]) == PODS and (whole["status"] == 0).all()
        split = {}
        for gap in GAPS:
            ora = make_oracle(tr, MODE)
            ora.submit(tracegen.slice_pods(tr, 0, FIRST))
            s0, rc0 = oracle_run(ora, gap)
            ora.submit(tracegen.slice_pods(tr, FIRST, PODS))
            s1, rc1 = oracle_run(ora, TICKS)
            assert rc0 == 0 and rc1 == 0 and len(s0["pod"]) + len(s1["pod"]) == PODS
            split[gap] = (s0, s1)
        _cases[seed] = (tr, encoded(tr), whole, split)
    return _cases[seed]


def _submit_slices(eng, pods, sizes, lo=0):
    for k in sizes:
        eng.submit(slice_encoded(pods, lo, lo + k))
        lo += k
    return lo


@pytest.mark.parametrize("seed", [1, 2])
def test_direct_and_staged_submits_schedule_alike(seed):
    tr, enc, whole, _ = _case(seed)
    a = make_engine(tr, enc, MODE)
    a.submit(enc["pods"])
    b = make_engine(tr, enc, MODE)
    assert sum(B_SLICES) == PODS and _submit_slices(b, enc["pods"], B_SLICES) == PODS
    ba, bb = a.step(TICKS), b.step(TICKS)
    assert len(ba) == PODS and len(bb) == PODS
    assert_same_binds(ba, whole)
    assert_same_binds(bb, whole)
    last = int(whole["tick"][-1])
    print(f"seed {seed}: last bind tick {last}")
    for t in (40, last // 2, last):
        ua, ub = a.usage_at(t), b.usage_at(t)
        np.testing.assert_array_equal(ua, ub)
        assert t == 40 or ua.any()
    sa, sb = a.pod_status(), b.pod_status()
    assert len(sa) == PODS
    for f in ("phase", "node", "start_tick", "total_seconds"):
        np.testing.assert_array_equal(sa[f], sb[f])
    a.close()
    b.close()


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("seed", [1, 2])
def test_submit_between_steps(seed, gap):
    tr, enc, _, split = _case(seed)
    s0, s1 = split[gap]
    c = make_engine(tr, enc, MODE)
    c.submit(slice_encoded(enc["pods"], 0, FIRST))
    b0 = c.step(gap)
    assert_same_binds(b0, s0)
    late = int((np.asarray(enc["pods"]["arrival"])[FIRST:] <= gap).sum())
    print(f"seed {seed} gap {gap}: {len(b0)} binds before the second submit, {late} late arrivals in it")
    assert (late > 0) == (gap == 700)
    _submit_slices(c, enc["pods"], (PODS - FIRST,), FIRST)
    b1 = c.step(TICKS)
    assert_same_binds(b1, s1)
    assert len(b0) + len(b1) == PODS
    c.close()
