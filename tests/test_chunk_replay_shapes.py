"""The traces of tests/test_chunk_replay_gpu.py on the oracle alone: they produce the events the
chunk resolver's replays must get right (tests/chunk_replay_cases.py replay_events).  The bounds
are the kernel's constants (ks_chunk.hip): 64-pod chunks, kSeg = 5 stored state segments per row,
kPend = 4 pending own expiries per node."""
import pytest

import chunk_replay_cases as cc
from harness import make_oracle, oracle_run

K_SEG, K_PEND = 5, 4


def _events(tr, mode, ticks):
    ora = make_oracle(tr, mode)
    ora.submit(tr)
    b, rc = oracle_run(ora, ticks)
    assert rc == 0 and len(b["pod"]) == ticks
    return cc.replay_events(b, cc.run_ticks(tr))


def test_dense_trace_rebinds_and_expires_across_chunks():
    ev = _events(cc.dense_trace(), "feeds_all_lrba", 1500)
    assert ev["rebind"] > 100 and ev["cross"] > 50 and ev["pending"] >= 2, ev


@pytest.mark.parametrize("name", sorted(cc.FEW_NODES))
def test_few_nodes_rebind_nodes_of_earlier_chunks(name):
    tr, mode = cc.few_nodes_trace(name)
    ev = _events(tr, mode, 600)
    assert ev["rebind"] > 100 and ev["cross"] > 20 and ev["binds"] > 8, ev
    assert ev["seg"] > K_SEG, ev  # a row passes its stored segments: the row-overflow stop
    if name == "pile40":
        assert ev["pending"] > K_PEND, ev  # the state-unknown stop
    if name != "spread24":
        assert ev["refused"] > 20, ev  # refused binds on nodes the batch bound before


def test_tight_trace_refuses_binds_on_replayed_nodes():
    ev = _events(cc.tight_trace(), "literal_const", 900)
    assert ev["refused"] > 100 and ev["rebind"] > 100, ev
