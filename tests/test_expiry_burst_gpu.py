"""Expiry bursts on every engine chain: hundreds of pods ending on one tick, at the real limits of
the expiry tables (tests/expiry_burst_cases.py lists the edges; tests/test_expiry_burst_cases.py pins
on the oracle alone that the traces produce them).

Every case compares the binds (pod, tick, node, status), the error code and usage() after every step
with the oracle — integer work, no tolerance.  Engines on the chunk resolver must leave no slot or E
mark behind (debug_invariants).  The oracle runs once per (trace, mode, plan) and is shared.

Which path ran is read from counters the engine already has, each as a lower bound only: the rescan
counter (debug_counters()[5]) across the step that holds the 2,100 burst, without KS_ENGINE_SMALL_E;
the batches of a step (last_step_stats()["launches"]).  last_step_kernels() does not tell the per-tick
launch from a batch: profiling keeps ks_step off the per-tick path altogether and the per-tick path
leaves those statistics alone, so that the 17-burst pod's one-tick step took the batch chain and the
16-burst pod's did not rests on the counts pinned on the oracle (16 and 17 live expiries attached to
those pods) and on tick_step's test, whose constant test_expiry_burst_cases.py compares.
"""
import numpy as np
import pytest

import expiry_burst_cases as ec
import group_cases as gc
import state_ref
from harness import MODES, assert_same_binds, make_engine, shard_ranks, step_ranks
from kubesim_amd import _lib, encode, shard, tracegen
from kubesim_amd.kubesim import KubeSim, TraceSubmitter

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
NO_OVERLAP = _lib.KS_ENGINE_NO_OVERLAP
PRUNED = _lib.KS_ENGINE_PRUNED_LISTS
ONE_POD = _lib.KS_ENGINE_ONE_POD_RESOLVER

# name: (batch_pods, engine_flags, shard, on the chunk resolver)
ENGINES = {
    "default": (0, 0, None, True),                     # chunk resolver, fused overlap, two-launch chain
    "plain": (0, CHUNK | NO_OVERLAP, None, True),      # the four-launch chain
    "pruned": (0, CHUNK | PRUNED, None, True),
    "one_pod_256": (256, ONE_POD, None, False),        # the role-split resolver
    "vshards3": (0, 0, (1, 0, None, 3), True),         # the sharded overlap with its conditional scan
}
RESCANS = ("default", "vshards3")   # chains whose window prep counts a rescan when E overflows


def _pods(name, lo, hi):
    c = ec.case(name)
    if (lo, hi) == (0, c["tr"]["pods"]["m"]):
        return c["enc"]["pods"]
    return encode.encode_pods(tracegen.slice_pods(c["tr"], lo, hi)["pods"], c["enc"]["taint_dict"],
                              c["enc"]["label_dict"])


def _engine(name, mode, engine="default"):
    c = ec.case(name)
    batch, flags, sh, _ = ENGINES[engine]
    return make_engine(c["tr"], c["enc"], mode, batch, flags, shard=sh)


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


def _burst_step(name, which, size):
    """Index of the plan's step that holds the burst tick of the burst of `size`."""
    f = next(f for f, lo, hi in ec.case(name)["bursts"] if hi - lo == size)
    return int(np.searchsorted(np.cumsum(ec.plan(name, which)), f))


def _lockstep(eng, name, mode, which, probe=False):
    """Step `eng` through the plan in lockstep with the oracle's record: the parts submitted at their
    ticks, after every step the binds, the usage and the tick compared, and with `probe` the engine's
    filter / score of the next queued pod against the oracle's evaluation.  Returns per step
    (rescans counted during it, batches it took)."""
    parts = {t: (lo, hi) for t, lo, hi in ec.case(name)["parts"]}
    eng.submit(_pods(name, *parts[0]))
    out = []
    for i, ref in enumerate(ec.reference(name, mode, which)):
        r0 = int(eng.debug_counters()[5])
        eb = eng.step(ref["k"])          # (a KsError fails the test: the oracle's code is 0)
        try:
            assert_same_binds(eb, ref["binds"])
        except AssertionError as ex:
            raise AssertionError(f"{name} {which} step {i} ({ref['k']} ticks): {ex}") from None
        np.testing.assert_array_equal(eng.usage(), ref["usage"], err_msg=f"{name} {which} step {i}: usage")
        assert eng.tick == ref["tick"]
        out.append((int(eng.debug_counters()[5]) - r0, int(eng.last_step_stats()["launches"])))
        if ref["tick"] in parts and ref["tick"] > 0:
            eng.submit(_pods(name, *parts[ref["tick"]]))
        if probe and ref["probe"] is not None:
            q, feas, score = ref["probe"]
            np.testing.assert_array_equal(eng.filter(q), feas, err_msg=f"{name} {which} step {i}: filter({q})")
            np.testing.assert_array_equal(eng.score(q), score, err_msg=f"{name} {which} step {i}: score({q})")
    return out


# ---- bursts3k on every chain ----------------------------------------------------------------------
def test_default_engine_is_the_chunk_resolver_on_the_two_launch_chain():
    """The host's choices for bursts3k's engines, from the rules restated in tests/group_cases.py and
    ks_plan.h plan_step: 3,000 nodes are past the small class at the default batch, chunk-eligible,
    12 scan blocks (at most kOverlapMaxBlocks: the fused overlap; one part: two launches per batch)."""
    tr = ec.case("bursts3k")["tr"]
    r = gc.restate(tr, ec.MODE)
    assert not r["small"] and gc.chunk_eligible(r) and r["blocks"] == 12 <= 256
    assert gc.small_class(128, ec.SMALL_NODES) and gc.restate(ec.case("small")["tr"], ec.MODE, 128)["small"]
    r = gc.restate(ec.case("bursts3k_refused")["tr"], ec.LITERAL)
    assert not r["small"] and gc.chunk_eligible(r)
    r = gc.restate(ec.case("gap")["tr"], ec.MODE)
    assert not r["small"] and gc.chunk_eligible(r)
    assert np.diff(shard.engine_part_blocks(ec.PIPE_NODES, 1, 2)).sum() == 257


@pytest.mark.parametrize("which", ["whole", "head", "mid"])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_bursts3k(engine, which):
    """`whole`: the bursts fall mid-pass and reach a head through the window cut.  `head`: every burst
    pod is a pass's first pod (the launched window prep, or expire_head).  `mid`: the burst pod is the
    98th of its pass's first batch."""
    eng = _engine("bursts3k", ec.MODE, engine)
    if which == "mid":
        eng.set_profiling(True)
    steps = _lockstep(eng, "bursts3k", ec.MODE, which)
    over = steps[_burst_step("bursts3k", which, 2100)]
    print(f"{engine} {which}: rescans per step {[s[0] for s in steps]}, batches {[s[1] for s in steps]}")
    if engine in RESCANS and which == "whole":
        assert over[0] > 0, "no rescan across the step that holds the 2,100 burst"
    if which == "mid":
        # 192 ticks: one default batch of the chunk resolver, had its window not held 513 expiries
        i = _burst_step("bursts3k", which, 513)
        assert ec.plan("bursts3k", which)[i] == 192 and steps[i][1] >= 2, steps[i]
        kn = eng.last_step_kernels()
        if engine == "default":
            assert kn["xchg_n"] == 0
        if engine == "vshards3":
            assert kn["xchg_n"] > 0
    if ENGINES[engine][3]:
        _no_marks(eng)
    eng.close()


def test_bursts3k_two_host_ranks():
    """Two thread-ranks over the host exchange: both must cut every batch at the same pod, or the
    exchange hangs (step_ranks fails rather than waits)."""
    c = ec.case("bursts3k")
    (ref,) = ec.reference("bursts3k", ec.MODE, "whole")
    engs, x = shard_ranks(c["tr"], c["enc"], 2, 1, ec.MODE)
    for r, eb in enumerate(step_ranks(engs, ref["k"], x)):
        assert_same_binds(eb, ref["binds"])
        np.testing.assert_array_equal(engs[r].usage(), ref["usage"])
    rescans = [int(e.debug_counters()[5]) for e in engs]
    print("two ranks: rescans", rescans)
    assert rescans[0] == rescans[1]
    for e in engs:
        _no_marks(e)
        e.close()


def test_bursts3k_spreading_mode():
    """feeds_fit_lr spreads the binds: a burst's members sit on as many nodes as it has pods."""
    eng = _engine("bursts3k", ec.SPREAD)
    steps = _lockstep(eng, "bursts3k", ec.SPREAD, "whole")
    print("spread: rescans", steps[0][0])
    assert steps[0][0] > 0
    _no_marks(eng)
    eng.close()


def test_bursts3k_state_queries_across_the_burst_ticks():
    """requested_at on both sides of every burst tick and the cluster series across it against
    tests/state_ref.py: up to 2,100 pods leave the requested state in one tick."""
    c = ec.case("bursts3k")
    eng = _engine("bursts3k", ec.MODE)
    _lockstep(eng, "bursts3k", ec.MODE, "whole")
    ref = state_ref.IntervalRef(c["tr"], ec.all_binds("bursts3k"))
    for f, lo, hi in c["bursts"]:
        before, after = eng.requested_at(f - 1), eng.requested_at(f)
        np.testing.assert_array_equal(before, ref.at(f - 1), err_msg=f"requested_at({f - 1})")
        np.testing.assert_array_equal(after, ref.at(f), err_msg=f"requested_at({f})")
        assert before[:, 3].sum() - after[:, 3].sum() >= hi - lo - 1   # the burst left (one pod was bound)
        np.testing.assert_array_equal(eng.cluster_series(f - 2, f + 2), ref.series(f - 2, f + 2),
                                      err_msg=f"cluster_series({f - 2}, {f + 2})")
    eng.close()


# ---- the small class --------------------------------------------------------------------------------
def test_small_class_single_engine():
    """Batches of 128 on 2,048 nodes: the register-table resolver, whose window holds 128 expiries,
    with expire_head_kernel in front of it (257 head expiries: its strided loop)."""
    c = ec.case("small")
    eng = make_engine(c["tr"], c["enc"], ec.MODE, 128)
    _lockstep(eng, "small", ec.MODE, "whole")
    eng.close()


def test_small_class_in_a_group():
    """The same member beside group_cases' `short` through ks_group_step."""
    from kubesim_amd.engine import Group
    c = ec.case("small")
    assert ec.plan("small", "group")[:len(gc.CHUNKS)] == gc.CHUNKS
    refs = ec.reference("small", ec.MODE, "group")
    short_tr, short_enc = gc.trace_of("short")
    short_ref = gc.reference("short")
    g = Group(2)
    try:
        engs = []
        for tr, enc, mode, batch in ((c["tr"], c["enc"], ec.MODE, 128),
                                     (short_tr, short_enc, gc.MEMBERS["short"]["mode"], gc.MEMBERS["short"]["batch_pods"])):
            fm, fl, sc = MODES[mode]
            e = g.add(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc, batch_pods=batch)
            e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
            e.submit(enc["pods"])
            engs.append(e)
        for i, ref in enumerate(refs):
            allb, cnt, st, _ = g.step(ref["k"])
            mine, other = g.split(allb, cnt)
            assert int(st[0]) == 0 and int(st[1]) == 0
            assert_same_binds(mine, ref["binds"])
            np.testing.assert_array_equal(engs[0].usage(), ref["usage"], err_msg=f"group step {i}")
            if i < len(short_ref):
                assert_same_binds(other, short_ref[i]["binds"])
                np.testing.assert_array_equal(engs[1].usage(), short_ref[i]["usage"])
            else:
                assert len(other) == 0
    finally:
        g.close()


# ---- refused members --------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "one_pod_256"])
def test_refused_members_are_never_applied(engine):
    """A share of every burst's members is bound OverCapacity: their expiries sit in the CSR (the
    window is cut by them) but must not be applied."""
    eng = _engine("bursts3k_refused", ec.LITERAL, engine)
    steps = _lockstep(eng, "bursts3k_refused", ec.LITERAL, "whole")
    print(f"refused {engine}: rescans {steps[0][0]}, batches {steps[0][1]}")
    if ENGINES[engine][3]:
        _no_marks(eng)
    eng.close()


# ---- bursts that end while the queue is empty -------------------------------------------------------
@pytest.mark.parametrize("engine", ["default", "one_pod_256"])
@pytest.mark.parametrize("how", ["step", "step_probed", "run", "run_windowed"])
def test_gap(engine, how):
    """A burst ends inside a pause of the arrivals and attaches to the first pod after it.  `step`:
    one ks_step.  `step_probed`: a step ends inside every pause after the burst tick and the next
    pod's filter / score are probed there (16 / 17 due and not applied: the by-value flush, and past
    it launch_flush).  `run` / `run_windowed`: the drop-in's loops (tests/test_dropin_gpu.py), where
    the pods are submitted tick by tick, so the burst waits in the engine's pending list."""
    c = ec.case("gap")
    eng = _engine("gap", ec.MODE, engine)
    if how in ("step", "step_probed"):
        _lockstep(eng, "gap", ec.MODE, "pause" if how == "step_probed" else "whole", probe=how == "step_probed")
    else:
        (ref,) = ec.reference("gap", ec.MODE, "whole")
        ks = KubeSim(eng, c["tr"]["tick_seconds"])
        ks.register_submitter(TraceSubmitter(c["enc"]["pods"]))
        if how == "run":
            ks.run(c["ticks"])
        else:
            ks.run_windowed(c["ticks"], 256)
        assert_same_binds(ks.all_binds(), ref["binds"])
        np.testing.assert_array_equal(eng.usage(), ref["usage"])
        assert eng.tick == ref["tick"]
    if ENGINES[engine][3]:
        _no_marks(eng)
    eng.close()


def test_ticks_plan_through_the_per_tick_path():
    """One-tick steps from F - 3 to F + 3 around the 16, 17 and 257 bursts on an engine with default
    flags and no profiling: the one-launch per-tick kernel with its by-value list of up to 16
    expiries, and past it the batch chain for that one pod.  After every step the next pod's filter /
    score are probed (on bulk arrivals nothing is due at a probe: the next pod's expiries end at its
    own bind tick; test_gap and test_pending probe with a burst due)."""
    eng = _engine("bursts3k", ec.MODE)
    steps = _lockstep(eng, "bursts3k", ec.MODE, "ticks", probe=True)
    assert sum(k == 1 for k in ec.plan("bursts3k", "ticks")) == 21
    print("ticks: batches per step", [s[1] for s in steps])
    _no_marks(eng)
    eng.close()


@pytest.mark.parametrize("name", ["pending16", "pending17_600"])
def test_pending(name):
    """Every submitted pod is bound when the burst ends, so its expiries wait in the engine's pending
    list: attached at the next submit, and due at the probe of the first new pod (for_each_due in
    flush_expiries: 16 by value, 17 and 600 through launch_flush)."""
    eng = _engine(name, ec.MODE)
    _lockstep(eng, name, ec.MODE, "parts", probe=True)
    _no_marks(eng)
    eng.close()


# ---- the pipelined chain -----------------------------------------------------------------------------
def test_bursts66k_pipelined_chain():
    """65,792 nodes in two parts on one rank (257 scan blocks: the pipelined chain, as
    tests/test_pipe_rescan_gpu.py sets it up), bursts of 513 and 2,100, no KS_ENGINE_SMALL_E."""
    c = ec.case("bursts66k")
    (ref,) = ec.reference("bursts66k", ec.MODE, "whole")
    eng = make_engine(c["tr"], c["enc"], ec.MODE, 192, CHUNK, shard=(1, 0, None, 2))
    eng.set_profiling(True)
    (step,) = _lockstep(eng, "bursts66k", ec.MODE, "whole")
    side = int(eng.last_step_kernels()["side_n"])
    print(f"66k: rescans {step[0]}, batches {step[1]}, side passes {side}")
    assert side > 0, "the pipelined chain did not run"
    assert step[0] > 0, "no rescan across the step that holds the 2,100 burst"
    _no_marks(eng)
    eng.close()
