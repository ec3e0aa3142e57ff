"""Run stops on every resolver chain: NotFound and InvalidArgument decided by state that changes
inside the batch (tests/stop_cases.py builds the traces; tests/test_stop_cases.py pins on the oracle
alone that each produces its event).

The stop is decided in four places — the chunk resolver (ks_chunk.hip), the small-cluster resolver
(ks_resolve.hip), the role-split one-pod resolver (ks_rolesplit.hip) and the per-tick kernel
(ks_tick.hip) — and unwound on the host by ks_step.cpp (the speculative scan of the next batch, the
early read-back, a sharded run's exchange).  A gpu is the scarce resource: the pods before X take
the last slots inside X's batch (X has candidates in the batch-start snapshot and must still reach
NotFound, never a stale node, never OverCapacity), or an expiry inside the window frees one (X's
snapshot list is empty and it must bind through the changed-node evaluation, not stop).

Every case runs in lockstep with the oracle's record of the same step plan: binds (pod, tick, node,
status), error code, tick, queue length and usage() — integers, no tolerance.  After a stop the
past-tick queries are compared with stop_cases.stopped_model (oracle/pysim.py's rules).

Where X really sits.  The batches of the step that holds X (last_step_stats()["launches"]) are
printed for every case.  One batch in a stopping step of B ticks means X sat at the planned index p
of its batch.  On the MI355X that holds on every chain for p = 0 and p = 1 and is asserted there
(HELD); from p = 63 on no chain keeps the batch whole: on this trace a batch commits 15-20 pods
before a top-L list is exhausted (3 batches up to p = 64, 10-11 up to p = B - 1 at B = 192; 2 and
6-8 at B = 256; 2 and 3-5 at B = 128), so X is then a pod of a later pass's batch, at an index the
counters do not tell.  There the count is printed and nothing is concluded from it.  The per-tick
path leaves those statistics alone.
"""
import threading

import numpy as np
import pytest

import group_cases as gc
import stop_cases as sc
from harness import MODES, assert_same_binds, make_engine
from kubesim_amd import _lib
from kubesim_amd.engine import Engine, Group, KsError, LocalExchange
from test_expiry_burst_gpu import ENGINES

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
EDGE = "rescued_in_batch_edge"
G32_ELSEWHERE = ("full", "rescued_own")   # the cases every chain but the default engine's runs on the g32 saturation
assert sc.CLUSTERS["3k"][1:] == sc.CLUSTERS["small"][1:]   # one set of plans for both


def _batch(engine):
    return ENGINES[engine][0] or sc.B_CHUNK


# the cases whose stop or rescue at p = 0 is decided on an empty snapshot list (or hangs on X's own expiry)
AT_HEAD = ("full", "too_late", "full_and_bad_key", "literal_bad_key", "bad_key", "rescued_own")


def _grid(b, default=False, head=AT_HEAD):
    """(sat, case, p, plan) rows.  `default`: on g6 every case at every position; on g32 every case
    at p in {0, B - 1} and at p = B with the step that ends before X.  Else on g6 every case at
    p = B - 1 and the `head` cases at p = 0 too; on g32 `full` and `rescued_own` at both.  The
    chunk-edge case runs at its own position (stop_cases.edge_p) where the batch holds it.
    (The pairs left out repeat a neighbour — p = 1 and 63 saw the same batches as 0 and 64 in the
    stopping step, see the module's docstring — and with them the file took longer than
    tests/test_expiry_burst_gpu.py.  No case is left out on any engine.)"""
    out = []
    for sat in sc.SATS:
        for name in sc.CASES:
            if name == EDGE:
                ps = (sc.edge_p(sat),) if sc.edge_p(sat) < b and (default or sat == "g6") else ()
            elif default:
                ps = sc.positions(b) if sat == "g6" else (0, b - 1, b)
            elif sat == "g6":
                ps = (0, b - 1) if name in head else (b - 1,)
            else:
                ps = (0, b - 1) if name in G32_ELSEWHERE else ()
            for p in ps:
                plans = sc.plans_at("3k", b, p)   # (the small cluster's plans are the same)
                for i, steps in enumerate(plans if sat == "g6" else plans[:1]):
                    out.append(pytest.param(sat, name, p, steps, id=f"{sat}-{name}-p{p}{'ab'[i] if p == b else ''}"))
    return out


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


def _text(code, pod, tick):
    return (f'node "" not found (pod {pod}, tick {tick})' if code == sc.KS_ENOTFOUND
            else f"pod {pod}: invalid pod key or simSpec (tick {tick})")


def _stopped_state(eng, key, r):
    """Everything a stopped engine must still answer, against the oracle's record `r` of the stopping
    step and the model of the stopped state."""
    c = sc.case(*key)
    code, pod = c["stop"]
    m = sc.stopped_model(*key)
    assert eng.tick == r["tick"] == m["tick"]
    assert eng.queued == r["queued"] == c["m"] - (pod + 1)      # the stop pod is popped
    np.testing.assert_array_equal(eng.usage(), r["usage"], err_msg="usage() after the stop")
    for t, want in m["req"].items():
        np.testing.assert_array_equal(eng.requested_at(t), want, err_msg=f"requested_at({t}), stop tick {m['tick']}")
    np.testing.assert_array_equal(eng.cluster_series(m["series_lo"], m["tick"] + 1), m["series"],
                                  err_msg="cluster_series up to the stop tick")
    for q, want in m["status"].items():
        got = eng.pod_status(q, 1)[0]
        assert (int(got["phase"]), int(got["node"]), int(got["start_tick"]), int(got["total_seconds"])) == want, (q, got)
    assert m["status"][pod - 1][0] != _lib.KS_PHASE_PENDING                       # bound
    assert m["status"][pod][0] == m["status"][pod + 1][0] == _lib.KS_PHASE_PENDING   # never bound
    for q in {pod, c["x"]}:
        with pytest.raises(KsError):
            eng.score_at(q)
    with pytest.raises(KsError):
        eng.requested_at(m["tick"] + 1)


def _lockstep(eng, key, steps, chunk, label, after_step=None):
    """Submit the case's pods and step `eng` through the plan beside the oracle's record.  Every step
    that the oracle finishes must return the same binds, usage and tick; the step it stops in must
    raise its code with the binds made before the stop pod, after which the engine is checked as
    stopped (and stays stopped).  Returns the batches of the step that holds X (the stop pod)."""
    c = sc.case(*key)
    ref = sc.reference(*key, steps)
    eng.submit(c["enc"]["pods"])
    watch = c["stop"][1] if c["stop"] else c["x"]
    seen, batches, held_k = 0, None, 0
    for i, r in enumerate(ref):
        holds = seen <= watch < seen + r["k"]
        if r["rc"] == 0:
            eb = eng.step(r["k"])       # (a KsError here fails the test: the oracle went on)
        else:
            with pytest.raises(KsError) as ex:
                eng.step(r["k"])
            eb = ex.value.binds
            assert ex.value.code == r["rc"] == c["stop"][0], (ex.value.code, r["rc"])
            assert _text(r["rc"], watch, r["tick"]) in str(ex.value), str(ex.value)
        if holds:
            batches, held_k = int(eng.last_step_stats()["launches"]), r["k"]
            print(f"LAUNCHES {label}: {batches} in the step of {r['k']} ticks that holds pod {watch}")
        try:
            assert_same_binds(eb, r["binds"])
        except AssertionError as e:
            raise AssertionError(f"{label} step {i} ({r['k']} ticks): {e}") from None
        np.testing.assert_array_equal(eng.usage(), r["usage"], err_msg=f"{label} step {i}: usage")
        assert eng.tick == r["tick"] and eng.queued == r["queued"]
        if chunk:
            _no_marks(eng)
        if after_step:
            after_step(i)
        seen += r["k"]
    last = ref[-1]
    if c["stop"]:
        assert last["rc"] != 0 and holds
        for after_queries in (False, True):   # sticky, before and after the queries
            with pytest.raises(KsError) as ex2:
                eng.step(1)
            assert ex2.value.code == last["rc"] and len(ex2.value.binds) == 0
            if not after_queries:
                _stopped_state(eng, key, last)
    else:                               # rescued: X bound Ok where the oracle bound it, the run went on to its end
        assert last["rc"] == 0 and len(ref) == len(steps) and eng.queued == 0
        got = eng.pod_status(c["x"], 1)[0]
        assert int(got["phase"]) == _lib.KS_PHASE_RUNNING and int(got["start_tick"]) == c["x"] + 1
        if c["freed"] is not None:
            assert int(got["node"]) == int(eng.pod_status(c["freed"], 1)[0]["node"])
    return batches, held_k


# The planned positions that one batch in the stopping step confirmed, on every chain (see above).
HELD = (0, 1)


def _position_held(key, p, b, held):
    batches, k = held
    c = sc.case(*key)
    if c["stop"] and c["stop"][1] == c["x"] and p in HELD and k == b:
        assert batches == 1, f"{batches} batches in the step that stops at X: X was not pod {p} of its batch"
    else:                       # (the stop pod in the warm step, a step that goes on past X, or a later p)
        assert batches >= 1


# ---- one engine, 3,000 nodes -------------------------------------------------------------------------
def _single(engine, sat, name, p, steps):
    batch, flags, sh, chunk = ENGINES[engine]
    key = (name, sat, "3k")
    c = sc.case(*key)
    eng = make_engine(c["tr"], c["enc"], c["mode"], _batch(engine), flags, shard=sh)
    try:
        _position_held(key, p, _batch(engine), _lockstep(eng, key, steps, chunk, f"{engine} {sat} {name} p={p}"))
    finally:
        eng.close()


@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_CHUNK, default=True))
def test_default_engine(sat, name, p, steps):
    """The chunk resolver on the fused two-launch chain (a one-tick step: the per-tick kernel): both
    saturations, every case; every position on g6, four of them on g32 (_grid)."""
    _single("default", sat, name, p, steps)


@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_CHUNK))
@pytest.mark.parametrize("engine", ["plain", "pruned", "vshards3"])
def test_chunk_resolver_chains(engine, sat, name, p, steps):
    """The four-launch chain, the pruned lists, and the sharded overlap with its conditional scan."""
    _single(engine, sat, name, p, steps)


@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_ONE_POD))
def test_one_pod_resolver(sat, name, p, steps):
    """The role-split one-pod resolver at batches of 256 (sh.err_code / sh.err_pod)."""
    _single("one_pod_256", sat, name, p, steps)


# ---- the small class -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_SMALL))
def test_small_class_single_engine(sat, name, p, steps):
    """2,048 nodes at batches of 128: the register-table resolver (stop = 2 / 3)."""
    key = (name, sat, "small")
    c = sc.case(*key)
    eng = make_engine(c["tr"], c["enc"], c["mode"], sc.B_SMALL)
    try:
        _position_held(key, p, sc.B_SMALL, _lockstep(eng, key, steps, False, f"small {sat} {name} p={p}"))
    finally:
        eng.close()


@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_SMALL))
def test_small_class_in_a_group(sat, name, p, steps):
    """The same member beside group_cases' `short` through ks_group_step: the step stops only that
    member, the other member's binds stay the oracle's to the end of its trace."""
    key = (name, sat, "small")
    c = sc.case(*key)
    ref = sc.reference(*key, steps)
    short_tr, short_enc = gc.trace_of("short")
    short_ref = sc.short_reference(steps)
    g = Group(2)
    try:
        engs = []
        for tr, enc, mode, batch in ((c["tr"], c["enc"], c["mode"], sc.B_SMALL),
                                     (short_tr, short_enc, gc.MEMBERS["short"]["mode"], gc.MEMBERS["short"]["batch_pods"])):
            fm, fl, scorers = MODES[mode]
            e = g.add(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=scorers, batch_pods=batch)
            e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
            e.submit(enc["pods"])
            engs.append(e)
        for i, k in enumerate(steps):
            r = ref[min(i, len(ref) - 1)]
            stopped = i >= len(ref)                      # a step after the member's stop
            allb, cnt, st, stats = g.step(k)
            mine, other = g.split(allb, cnt)
            assert int(st[1]) == 0
            assert_same_binds(other, short_ref[i][0])
            np.testing.assert_array_equal(engs[1].usage(), short_ref[i][1], err_msg=f"group step {i}: the other member")
            if stopped:
                assert int(st[0]) == r["rc"] != 0 and len(mine) == 0
            else:
                assert int(st[0]) == r["rc"]
                assert_same_binds(mine, r["binds"])
                np.testing.assert_array_equal(engs[0].usage(), r["usage"], err_msg=f"group step {i}")
                assert engs[0].tick == r["tick"] and engs[0].queued == r["queued"]
                if r["rc"]:
                    print(f"LAUNCHES group {sat} {name} p={p}: {stats['launches']} (the group's) in the stopping step")
                    _position_held(key, p, sc.B_SMALL, (int(stats["launches"]), k))
                    text = engs[0]._L.ks_last_error(engs[0].h).decode()
                    assert _text(r["rc"], c["stop"][1], r["tick"]) in text, text
            if r["rc"]:
                _stopped_state(engs[0], key, r)
        assert engs[1].queued == short_tr["pods"]["m"] - sum(steps)   # (still binding when the plan ends)
        if c["stop"]:
            assert len(ref) < len(steps)                  # the group was stepped on after the stop
        else:
            assert engs[0].queued == 0
    finally:
        g.close()


# ---- two host-exchange ranks ---------------------------------------------------------------------------
def _step_ranks(engs, k, x):
    """Every rank `k` ticks on a thread of its own.  Returns per rank the binds or the KsError of a
    scheduling stop.  A stop ends no exchange (both ranks must reach it by themselves); any other
    failure, or a rank that has not returned at the join timeout, aborts the exchange so that no
    rank waits, and fails."""
    out = [None] * len(engs)

    def run(r):
        try:
            out[r] = engs[r].step(k)
        except KsError as ex:
            out[r] = ex
            if ex.code not in (sc.KS_EINVAL, sc.KS_ENOTFOUND):
                x.abort()
        except Exception as ex:  # noqa: BLE001 - reported below
            out[r] = ex
            x.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(len(engs))]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    hung = any(t.is_alive() for t in th)
    if hung:
        x.abort()
        for t in th:
            t.join(30)
    assert not hung, "a rank hung in the exchange"
    for o in out:
        if isinstance(o, Exception) and not (isinstance(o, KsError) and o.code in (sc.KS_EINVAL, sc.KS_ENOTFOUND)):
            raise o
    return out


@pytest.mark.parametrize("sat,name,p,steps", _grid(sc.B_CHUNK, head=G32_ELSEWHERE))
def test_two_host_ranks(sat, name, p, steps):
    """Two thread-ranks over the host exchange: both stop at the same pod with the same binds."""
    key = (name, sat, "3k")
    c = sc.case(*key)
    ref = sc.reference(*key, steps)
    fm, fl, scorers = MODES[c["mode"]]
    x = LocalExchange(2)
    engs = []
    try:
        for rank in range(2):
            e = Engine(tick_seconds=c["tr"]["tick_seconds"], filter_mode=fm, filters=fl, scorers=scorers,
                       batch_pods=sc.B_CHUNK)
            engs.append(e)
            e.shard_host(2, rank, x, 1)
            e.load_nodes(c["enc"]["alloc"], c["enc"]["taint"], c["enc"]["label"])
            e.submit(c["enc"]["pods"])
        for i, r in enumerate(ref):
            got = _step_ranks(engs, r["k"], x)
            for rank, (e, o) in enumerate(zip(engs, got)):
                if r["rc"]:
                    assert isinstance(o, KsError), f"rank {rank} went on where the oracle stopped"
                    assert o.code == r["rc"] and _text(r["rc"], c["stop"][1], r["tick"]) in str(o), str(o)
                    o = o.binds
                else:
                    assert not isinstance(o, KsError), f"rank {rank}: {o}"
                try:
                    assert_same_binds(o, r["binds"])
                except AssertionError as ex:
                    raise AssertionError(f"rank {rank} step {i}: {ex}") from None
                np.testing.assert_array_equal(e.usage(), r["usage"], err_msg=f"rank {rank} step {i}: usage")
                assert e.tick == r["tick"] and e.queued == r["queued"]
                _no_marks(e)
            if r["rc"]:
                launches = [int(e.last_step_stats()["launches"]) for e in engs]
                print(f"LAUNCHES ranks {sat} {name} p={p}: {launches}")
                assert launches[0] == launches[1]
                _position_held(key, p, sc.B_CHUNK, (launches[0], r["k"]))
        for rank, e in enumerate(engs):
            if c["stop"]:
                with pytest.raises(KsError) as ex2:     # (a stopped engine returns before any exchange)
                    e.step(1)
                assert ex2.value.code == ref[-1]["rc"] and len(ex2.value.binds) == 0
                _stopped_state(e, key, ref[-1])
            else:
                assert e.queued == 0 and len(ref) == len(steps)
    finally:
        for e in engs:
            e.close()
        x.close()


# ---- the pipelined chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "rescued_own"])
@pytest.mark.parametrize("sat", list(sc.SATS))
def test_pipelined_chain(sat, name):
    """65,792 nodes in two parts on one rank (257 scan blocks), as
    tests/test_expiry_burst_gpu.py::test_bursts66k_pipelined_chain sets it up; X is pod 64 of its batch."""
    key = (name, sat, "pipe")
    c = sc.case(*key)
    eng = make_engine(c["tr"], c["enc"], c["mode"], sc.B_CHUNK, CHUNK, shard=(1, 0, None, 2))
    try:
        eng.set_profiling(True)
        side = []
        _lockstep(eng, key, sc.plan("pipe", sc.B_CHUNK, sc.KC), True, f"pipe {sat} {name} p={sc.KC}",
                  after_step=lambda i: side.append(int(eng.last_step_kernels()["side_n"])))
        print(f"pipe {sat} {name}: side passes per step {side}")
        assert side[0] > 0, "the pipelined chain did not run in the warm step"
    finally:
        eng.close()


# ---- the per-tick path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "rescued_own", "too_late"])
@pytest.mark.parametrize("sat", list(sc.SATS))
def test_per_tick_path(sat, name):
    """An engine with default flags and no profiling, one-tick steps from pod X - 3 through X: the
    one-launch per-tick kernel decides the stop (best == 0) with X's own expiry passed by value."""
    key = (name, sat, "3k")
    c = sc.case(*key)
    eng = make_engine(c["tr"], c["enc"], c["mode"])
    try:
        _lockstep(eng, key, sc.plan("3k", sc.B_CHUNK, 0, "ticks"), True, f"ticks {sat} {name}")
    finally:
        eng.close()
