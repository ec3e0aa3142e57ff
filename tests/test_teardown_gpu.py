"""Teardown of every kind of engine (ks_engine.cpp engine_free and ks_group_destroy; the owners of
ks_own.h release what each kind built on first use): on one small trace, build, use briefly and
close one engine of each kind that owns a different bundle —

* per-tick stepping: the per-tick scratch and the staging arena;
* the chunk resolver with pruned lists: the window workspace and the bitmaps;
* a batched step long enough for the early read-back: the copy stream and its event, the read-back buffers;
* two host-exchange ranks of two virtual shards: the pipelined chain's stream, events and arguments;
* a group of three members, which borrow the group's stream, counters and argument slots;
* an engine closed right after load_nodes, and one closed before it

— twice in one process, and then a fresh engine still schedules bind for bind as the oracle.  Each used
engine's binds are checked against the oracle too.  No error path is provoked.
"""
import numpy as np
import pytest

from harness import (MODES, assert_same_binds, encoded, make_engine, make_oracle, oracle_run, shard_ranks, small_trace,
                     step_ranks)
from kubesim_amd import _lib

pytestmark = pytest.mark.gpu

MODE = "literal_lrba_filters_ignored"  # (with filters feeding the score this trace stops at a pod no node fits)
CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
PRUNED = _lib.KS_ENGINE_PRUNED_LISTS
PODS = 200
EARLY_BATCH = 8  # 25 rounds in one step: past the early read-back's minimum of 16 (ks_plan.h early_round)


def _round_of_engines(tr, enc, want):
    from kubesim_amd.engine import Engine, Group
    fm, fl, sc = MODES[MODE]
    cfg = dict(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc)

    eng = make_engine(tr, enc, MODE)  # per-tick stepping
    eng.submit(enc["pods"])
    got = []
    for _ in range(40):
        got.append(eng.step(1))
        assert len(got[-1]) == 1 and eng.last_step_stats()["launches"] == 1
    got.append(eng.step(PODS))
    assert_same_binds(np.concatenate(got), want)
    eng.close()

    eng = make_engine(tr, enc, MODE, engine_flags=CHUNK | PRUNED)  # window workspace and bitmaps
    eng.submit(enc["pods"])
    assert_same_binds(eng.step(PODS), want)
    assert eng.debug_window()
    eng.close()

    eng = make_engine(tr, enc, MODE, EARLY_BATCH, CHUNK)  # the early read-back
    eng.submit(enc["pods"])
    assert_same_binds(eng.step(PODS), want)
    ctr = eng.debug_counters()
    print("early read-back: launches", eng.last_step_stats()["launches"], "early", int(ctr[8]), "snapshot", int(ctr[9]))
    assert int(ctr[9]) >= 1
    eng.close()

    engs, x = shard_ranks(tr, enc, 2, 2, MODE, engine_flags=CHUNK)  # the pipelined sharded chain
    for b in step_ranks(engs, PODS, x):
        assert_same_binds(b, want)
    for e in engs:
        e.close()
    x.close()

    g = Group(3)  # members borrow the group's stream, counters and argument slots
    members = [g.add(**cfg) for _ in range(3)]
    for e in members:
        e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
        e.submit(enc["pods"])
    allb, cnt, st, _ = g.step(PODS)
    assert (st == 0).all()
    for b in g.split(allb, cnt):
        assert_same_binds(b, want)
    g.close()

    eng = make_engine(tr, enc, MODE)  # closed right after load_nodes
    eng.close()
    eng = Engine(**cfg)               # closed before load_nodes
    eng.close()


def test_every_kind_of_engine_closes_twice_over():
    tr = small_trace(3)
    enc = encoded(tr)
    ora = make_oracle(tr, MODE)
    ora.submit(tr)
    want, rc = oracle_run(ora, PODS)
    assert rc == 0 and len(want["pod"]) == PODS
    for _ in range(2):
        _round_of_engines(tr, enc, want)
    eng = make_engine(tr, enc, MODE)
    eng.submit(enc["pods"])
    assert_same_binds(eng.step(PODS), want)
    np.testing.assert_array_equal(eng.usage(), ora.usage())
    eng.close()
