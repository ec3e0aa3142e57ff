"""The pipelined sharded chain's E-overflow branch (ks_step.cpp batch_pipe).  A sharded engine
whose rank scans more than kOverlapMaxBlocks = 256 blocks runs batch b + 1's speculative scan, part
merges and exchange on a second stream beside batch b's resolve.  When the window prep flags a
rescan (more changed nodes than E holds), the main stream scans every block of the cluster locally
(d_args_full, kRescanWgs workgroups) and merge_cl reads the rank's own block lists instead of the
exchanged cand_all (`own_fb && ws.rescan`).  The C5 goldens, the only other runs of this chain, never
rescan; KS_ENGINE_SMALL_E lowers the overflow threshold to 128 changed nodes, so 192-pod batches
overflow after every full batch.

Clusters of 257 scan blocks per rank, the smallest above kOverlapMaxBlocks: 65,792 nodes on one
engine with two parts, 131,584 nodes on two thread-ranks (there the rescan's own lists replace lists
that really were exchanged).  Every case is binds, statuses and usage against the oracle (integer
work: no tolerance); the oracle runs once per trace and is shared.

Measured (MI355X), side passes / rescans over the 1,536 pods: c2 22 / 7 with SMALL_E (full and pruned
lists) and 23 / 4 without; dense expiries 119 / 119 with SMALL_E and 119 / 0 without; two ranks 22 / 7
on each rank.
"""
import os

import numpy as np
import pytest

from harness import assert_same_binds, encoded, make_engine, make_oracle, oracle_run, shard_ranks, small_trace, step_ranks
from kubesim_amd import _lib, shard, tracegen

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
SMALL_E = _lib.KS_ENGINE_SMALL_E
PRUNED = _lib.KS_ENGINE_PRUNED_LISTS
MODE = "feeds_all_lrba"
BATCH = 192
PODS = 1536
STEPS = (700, 836)
OVERLAP_MAX_BLOCKS = 256  # csrc/ks_plan.h kOverlapMaxBlocks
NODES = (OVERLAP_MAX_BLOCKS + 1) * shard.BLOCK_NODES  # 65,792

_traces, _oracles = {}, {}


def _trace(case):
    if case not in _traces:
        if case == "c2":
            tr = tracegen.c2_trace(n_nodes=NODES, n_pods=PODS)
        elif case == "c2_two_ranks":
            tr = tracegen.c2_trace(n_nodes=2 * NODES, n_pods=PODS)
        else:  # dense expiries (tests/test_round_rescan_gpu.py) at this node count
            tr = small_trace(11, n_nodes=NODES, n_pods=PODS, taints=False, selectors=False, tolerations=False)
            tr["pods"]["phase_sec"][:] = 1 + (np.arange(len(tr["pods"]["phase_sec"])) % 12)
        _traces[case] = (tr, encoded(tr))
    return _traces[case]


def _oracle(case):
    """Per step: (the oracle's binds, error code, usage after the step)."""
    if case not in _oracles:
        tr, _ = _trace(case)
        ora = make_oracle(tr, MODE)
        ora.set_threads(int(os.environ.get("OMP_NUM_THREADS") or 0) or min(os.cpu_count() or 1, 16))
        ora.submit(tr)
        out = []
        for k in STEPS:
            ob, orc = oracle_run(ora, k)
            out.append((ob, orc, ora.usage().copy()))
        ora.close()
        _oracles[case] = out
    return _oracles[case]


def _lockstep(case, flags):
    """One engine with two parts (257 blocks: the pipelined chain), profiled, in lockstep with the
    oracle.  Returns (engine, binds, side passes summed over the steps).  Every step's launch counts
    are the pipelined chain's (N batches): a scan (or the conditional rescan) and a merge_cl per batch,
    no window prep counted, an exchange on the main stream once per pass (its first batch), the
    unfused resolve once per pass (its last), a side pass beside every fused resolve."""
    tr, enc = _trace(case)
    assert np.diff(shard.engine_part_blocks(tr["nodes"]["n"], 1, 2)).sum() == OVERLAP_MAX_BLOCKS + 1
    eng = make_engine(tr, enc, MODE, BATCH, flags, shard=(1, 0, None, 2))
    eng.submit(enc["pods"])
    eng.set_profiling(True)
    got, side = [], 0
    for k, (ob, orc, ou) in zip(STEPS, _oracle(case)):
        assert orc == 0
        eb = eng.step(k)
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ou)
        kn, n = eng.last_step_kernels(), eng.last_step_stats()["launches"]
        assert n > 0 and kn["scan_n"] == kn["merge_n"] == n and kn["prep_n"] == 0, (n, kn)
        assert kn["xchg_n"] == kn["resolve_n"] and kn["fused_n"] == kn["side_n"] == n - kn["resolve_n"], (n, kn)
        side += int(kn["side_n"])
        got.append(eb)
    return eng, np.concatenate(got), side


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


@pytest.mark.parametrize("pruned", [False, True], ids=["full_lists", "pruned_lists"])
@pytest.mark.parametrize("case", ["c2", "dense_expiries"])
def test_pipelined_chain_forced_rescans(case, pruned):
    """Every pipelined batch that follows a full one changed more than 128 nodes (one per bind on a
    cluster this size, plus the window's expiry nodes), so it rescans every block locally.  The pods
    run in at least P / 192 batches; a quarter of that many rescans is a loose floor — a handful
    would mean the path is not taken (tests/test_round_rescan_gpu.py test_forced_rescans)."""
    eng, _, side = _lockstep(case, CHUNK | SMALL_E | (PRUNED if pruned else 0))
    rescans = int(eng.debug_counters()[5])
    print(f"{case} pruned={pruned}: side_n {side}, {rescans} rescans, {PODS / BATCH:.0f}+ batches")
    assert side > 0, "the pipelined chain did not run"
    assert rescans >= PODS // (4 * BATCH), rescans
    _no_marks(eng)
    eng.close()


@pytest.mark.parametrize("case", ["c2", "dense_expiries"])
def test_pipelined_same_binds_with_and_without_small_e(case):
    """SMALL_E changes the batching only: the same binds, strictly fewer rescans without it."""
    a, ba, sa = _lockstep(case, CHUNK | SMALL_E)
    b, bb, sb = _lockstep(case, CHUNK)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(ba[f], bb[f])
    ra, rb = int(a.debug_counters()[5]), int(b.debug_counters()[5])
    print(f"{case}: rescans {ra} with SMALL_E, {rb} without; side_n {sa}, {sb}")
    assert sa > 0 and sb > 0
    assert ra > 0 and rb < ra, (ra, rb)
    _no_marks(a)
    _no_marks(b)
    a.close()
    b.close()


def test_pipelined_two_ranks_forced_rescans():
    """Two thread-ranks over LocalExchange on 131,584 nodes, 257 blocks each: the rescan's own lists
    replace lists that really were exchanged.  Both ranks bind-for-bind against the oracle; both
    take the same rescans (the resolvers are identical, so every rank's window prep sees the same
    changed nodes)."""
    tr, enc = _trace("c2_two_ranks")
    assert (np.diff(shard.engine_part_blocks(tr["nodes"]["n"], 2)) == OVERLAP_MAX_BLOCKS + 1).all()
    engs, x = shard_ranks(tr, enc, 2, 1, MODE, batch_pods=BATCH, engine_flags=CHUNK | SMALL_E)
    for e in engs:
        e.set_profiling(True)
    side = [0, 0]
    for k, (ob, orc, ou) in zip(STEPS, _oracle("c2_two_ranks")):
        assert orc == 0
        for r, eb in enumerate(step_ranks(engs, k, x)):
            assert_same_binds(eb, ob)
            np.testing.assert_array_equal(engs[r].usage(), ou)
            side[r] += int(engs[r].last_step_kernels()["side_n"])
    rescans = [int(e.debug_counters()[5]) for e in engs]
    print(f"two ranks: side_n {side}, rescans {rescans}")
    assert min(side) > 0, "the pipelined chain did not run"
    assert rescans[0] > 0 and rescans[0] == rescans[1], rescans
    for e in engs:
        _no_marks(e)
        e.close()
