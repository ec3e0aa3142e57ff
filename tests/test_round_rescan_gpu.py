"""The two-launch overlapped chain (ks_step.cpp batch_two_launch): a single-shard engine on
the fused overlap launches merge_cl -> chunk kernel per overlapped batch, with no conditional scan
in between.  merge_cl reads its E nodes from the node table and the node constants table, and a
window prep that must rescan (E overflow) publishes an empty batch whose round's fused scan lists
the same pods again (ks_prep.h).  KS_ENGINE_SMALL_E lowers the overflow threshold to 128 changed
nodes so that small clusters reach that path.

Every case is binds, statuses and usage against the oracle (integer work: no tolerance).  The
oracle runs once per (trace, mode, step lengths) and is shared.
"""
import numpy as np
import pytest

from harness import assert_same_binds, encoded, make_engine, make_oracle, oracle_run, small_trace
from kubesim_amd import _lib, tracegen
from kubesim_amd import encode as E

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
ONE_POD = _lib.KS_ENGINE_ONE_POD_RESOLVER
SMALL_E = _lib.KS_ENGINE_SMALL_E
PRUNED = _lib.KS_ENGINE_PRUNED_LISTS
BATCH = 192

_traces, _oracles = {}, {}


def _trace(case):
    if case not in _traces:
        if case == "c2":
            tr = tracegen.c2_trace(n_pods=12_000)
        else:  # dense expiries (tests/test_resolvers_gpu.py test_dense_expiries)
            tr = small_trace(11, n_nodes=2000, n_pods=6000, taints=False, selectors=False, tolerations=False)
            tr["pods"]["phase_sec"][:] = 1 + (np.arange(len(tr["pods"]["phase_sec"])) % 12)
        _traces[case] = (tr, encoded(tr))
    return _traces[case]


def _oracle(case, mode, steps):
    """Per step: (the oracle's binds, error code, usage after the step)."""
    key = (case, mode, tuple(steps))
    if key not in _oracles:
        tr, _ = _trace(case)
        ora = make_oracle(tr, mode)
        ora.submit(tr)
        out = []
        for k in steps:
            ob, orc = oracle_run(ora, k)
            out.append((ob, orc, ora.usage().copy()))
        _oracles[key] = out
    return _oracles[key]


def _lockstep(case, mode, steps, flags, shard=None, profile=False):
    """Step the engine and compare with the oracle after every step; returns the engine and its binds."""
    tr, enc = _trace(case)
    eng = make_engine(tr, enc, mode, BATCH, flags, shard=shard)
    eng.submit(enc["pods"])
    if profile:
        eng.set_profiling(True)
    got = []
    for k, (ob, orc, ou) in zip(steps, _oracle(case, mode, steps)):
        assert orc == 0
        eb = eng.step(k)
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ou)
        got.append(eb)
    return eng, np.concatenate(got)


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


CASES = {"dense_expiries": (6000, (1500,) * 4), "c2": (12_000, (5000, 7000))}


@pytest.mark.parametrize("mode", ["feeds_all_lrba", "literal_lrba_filters_ignored"], ids=["feeds", "literal"])
@pytest.mark.parametrize("pruned", [False, True], ids=["full_lists", "pruned_lists"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_forced_rescans(case, pruned, mode):
    """With 192-pod batches every overlapped batch that follows a full one changes more than 128
    nodes (one per bind on clusters of >= 2,000 nodes, plus the window's expiry nodes), so its window
    overflows and is retried after an empty round: about every second round is empty.  The pods run
    in at least P / 192 batches; a quarter of that many rescans is a loose floor — a handful would
    mean the path is not taken."""
    pods, steps = CASES[case]
    eng, _ = _lockstep(case, mode, steps, CHUNK | SMALL_E | (PRUNED if pruned else 0))
    rescans = int(eng.debug_counters()[5])
    print(f"{case} pruned={pruned} {mode}: {rescans} rescans, {pods / BATCH:.0f}+ batches")
    assert rescans >= pods // (4 * BATCH), rescans
    _no_marks(eng)
    eng.close()


def test_step_lengths_put_empty_rounds_everywhere():
    """Steps of 500, 193 and 1 ticks, mixed: passes of three, two and one batch, so empty rounds fall
    on a pass's last batch (the chunk kernel alone: nothing scanned, the next pass's first batch
    scans) and on a step's last launch.  (The resolver is forced, so a one-tick step is a one-batch
    pass of the chunk chain between the longer ones.)"""
    pat = (500, 1, 193, 193, 1, 1, 500, 193, 1, 500, 1, 193)
    steps, left = [], 6000
    while left > 0:
        k = min(pat[len(steps) % len(pat)], left)
        steps.append(k)
        left -= k
    eng, _ = _lockstep("dense_expiries", "feeds_all_lrba", steps, CHUNK | SMALL_E)
    assert int(eng.debug_counters()[5]) > 0
    _no_marks(eng)
    eng.close()


def test_same_binds_with_and_without_small_e():
    """SMALL_E changes the batching only."""
    steps = CASES["dense_expiries"][1]
    a, ba = _lockstep("dense_expiries", "feeds_all_lrba", steps, CHUNK | SMALL_E)
    b, bb = _lockstep("dense_expiries", "feeds_all_lrba", steps, CHUNK)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(ba[f], bb[f])
    assert int(a.debug_counters()[5]) > int(b.debug_counters()[5])
    a.close()
    b.close()


def _rescale_run(flags, batch=256, profile=False):
    """The 500-node, 1,200-pod trace whose first fractional-byte pod arrives between two batched
    steps, in lockstep with the oracle; yields the engine after each step."""
    tr = small_trace(31, n_nodes=500, n_pods=1200, taints=False, selectors=False, tolerations=False)
    tr["pods"]["req"][700:, 1] += 1  # +1 milli-byte: not a whole byte
    mode = "feeds_all_lrba"
    enc = encoded(tr)
    eng = make_engine(tr, enc, mode, batch, flags)
    eng.set_profiling(profile)
    ora = make_oracle(tr, mode)
    for lo, hi in ((0, 600), (600, 1200)):
        part = tracegen.slice_pods(tr, lo, hi)
        eng.submit(E.encode_pods(part["pods"], enc["taint_dict"], enc["label_dict"]))
        ora.submit(part)
        eb = eng.step(600)
        ob, orc = oracle_run(ora, 600)
        assert orc == 0
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ora.usage())
        yield eng
    eng.close()


def test_constants_table_after_a_rescale():
    """The first fractional-byte pod arrives between two batched steps (tests/test_engine_gpu.py
    test_memory_unit_rescale_mid_run, its sizes): the submit rescales the node table's memory
    fields, which the node constants table packs.  Chunk resolver forced, overlap on."""
    for step, eng in enumerate(_rescale_run(CHUNK)):
        if step == 1:  # (after the last step)
            _no_marks(eng)


def _launch_counts(eng):
    """(launches of the last step, its per-kernel statistics), profiling on."""
    k, n = eng.last_step_kernels(), eng.last_step_stats()["launches"]
    print(n, {f: v for f, v in k.items() if f.endswith("_n")})
    assert n > 0
    return n, k


@pytest.mark.parametrize("flags,batch", [(ONE_POD, 256), (0, 0)], ids=["one_pod_resolver", "small_resolver"])
def test_plain_chain_launches_every_kernel_per_batch(flags, batch):
    """The plain chain (ks_step.cpp batch_plain) is four launches per batch whatever the resolver:
    expiries, scan, merge and the resolver once each, nothing fused.  The role-split resolver forced
    on 256-pod batches; and no resolver flag with the engine's own batch size (64 pods on 500 nodes,
    within the register-table resolver's 128), which selects that resolver — with 256-pod batches the
    default would be the chunk resolver's two-launch chain, whose fused launches fail this."""
    for eng in _rescale_run(flags, batch, profile=True):
        n, k = _launch_counts(eng)
        assert k["prep_n"] == k["scan_n"] == k["merge_n"] == k["resolve_n"] == n, (n, k)
        assert k["fused_n"] == 0 and k["xchg_n"] == 0 and k["side_n"] == 0, k


def test_unchanged_chains_still_launch_their_scan():
    """A sharded overlapped engine keeps its conditional scan launch per batch (scan_n == merge_n);
    the single-shard overlapped engine launches a scan only for a pass's first batch, the batches
    whose window prep is a launch of its own (scan_n == prep_n).  Per chain, the launch counts of the
    step (N batches): the sharded overlap (ks_step.cpp batch_overlap_sharded) scans, merges and
    exchanges every batch, preps once per pass and resolves unfused once per pass (its last batch);
    the two-launch chain (batch_two_launch) merges every batch, scans only where it preps, and never
    exchanges."""
    steps = CASES["dense_expiries"][1]
    eng, _ = _lockstep("dense_expiries", "feeds_all_lrba", steps, CHUNK, shard=(1, 0, None, 2), profile=True)
    k = eng.last_step_kernels()
    assert k["merge_n"] > k["prep_n"] > 0 and k["scan_n"] == k["merge_n"], k
    n, k = _launch_counts(eng)
    assert k["scan_n"] == k["merge_n"] == k["xchg_n"] == n, (n, k)
    assert k["prep_n"] == k["resolve_n"] and k["fused_n"] == n - k["prep_n"], (n, k)
    eng.close()
    eng, _ = _lockstep("dense_expiries", "feeds_all_lrba", steps, CHUNK, profile=True)
    k = eng.last_step_kernels()
    assert k["merge_n"] > k["prep_n"] > 0 and k["fused_n"] > 0 and k["scan_n"] == k["prep_n"], k
    n, k = _launch_counts(eng)
    assert k["merge_n"] == n and k["scan_n"] == k["prep_n"] == k["resolve_n"], (n, k)
    assert k["fused_n"] == n - k["prep_n"] and k["xchg_n"] == 0, (n, k)
    eng.close()
