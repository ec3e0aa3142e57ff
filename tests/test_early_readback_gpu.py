"""One wait per pass and the early read-back (ks_step.cpp step_body, ks_plan.h early_round; DESIGN.md
§2): a pass enqueues the copies of its counters and of its binds' node and status words behind its
last round and waits once; a two-launch pass of sixteen or more rounds reads the binds below a
snapshot of the start counter back early, on a copy stream, and finishes them on the host while the
last rounds run; a later pass hides the finishing of the earlier passes' binds; a long pass without
a snapshot leaves its binds to one copy after the loop.

Every case is binds, statuses and usage against the oracle after every step (integer work: no
tolerance), with the chunk resolver forced and the overlap on, so that these small clusters take the
two-launch chain.  The oracle runs once per (trace, step lengths) and is shared.
"""
import numpy as np
import pytest

from harness import assert_same_binds, encoded, make_engine, make_oracle, oracle_run, small_trace
from kubesim_amd import _lib, tracegen
from test_early_round_host import consts

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
SMALL_E = _lib.KS_ENGINE_SMALL_E
MODE = "feeds_all_lrba"
BATCHES = (65, 128, 192)
PODS = {"dense": 1500, "c2": 9600}

_traces, _oracles = {}, {}


def _dense():
    """The dense-expiry trace (tests/test_resolvers_gpu.py test_dense_expiries) at 300 nodes / 1,500 pods."""
    tr = small_trace(11, n_nodes=300, n_pods=PODS["dense"], taints=False, selectors=False, tolerations=False)
    tr["pods"]["phase_sec"][:] = 1 + (np.arange(len(tr["pods"]["phase_sec"])) % 12)
    return tr


def _trace(case):
    """case: "dense", "c2", or ("c2", kind, pod): the C2 prefix with a failing pod."""
    if case not in _traces:
        if case == "dense":
            tr = _dense()
        else:
            tr = tracegen.c2_trace(n_pods=PODS["c2"])
            if case != "c2":
                _, kind, pod = case
                if kind == "bad_key":
                    tr["pods"]["flags"][pod] = 1           # empty namespace/name: KS_EINVAL
                else:
                    tr["pods"]["req"][pod, 0] = 10_000_000  # 10,000 cores: fits no node, NotFound
        _traces[case] = (tr, encoded(tr))
    return _traces[case]


def _oracle(case, steps):
    """Per step: (the oracle's binds, error code, usage after the step, tick after the step)."""
    key = (case, tuple(steps))
    if key not in _oracles:
        tr, _ = _trace(case)
        ora = make_oracle(tr, MODE)
        ora.submit(tr)
        out = []
        for k in steps:
            ob, orc = oracle_run(ora, k)
            out.append((ob, orc, ora.usage().copy(), ora.tick))
            if orc:
                break
        _oracles[key] = out
    return _oracles[key]


def step_lengths(pods, B):
    """Step lengths for `pods` pods in batches of B, each wanted length taken while it fits: long
    enough for the early read-back (its minimum of sixteen rounds and six more), exactly k B and
    k B + 1 at that minimum, one round below it, a short one, one pod, two batches; the rest in steps
    of 20 B (a fresh cluster's launches stop early after a few dozen pods, so the first steps take
    several passes; by these later steps a launch commits most of its batch and a step is one long
    pass and a short one)."""
    c = consts()
    k = c["early_min"]
    steps, left = [], pods
    for want in ((k + c["early_k"]) * B, k * B, k * B + 1, (k - 1) * B, 3 * B + 5, 1, 2 * B):
        if left >= want:
            steps.append(want)
            left -= want
    while left:
        steps.append(min(left, 20 * B))
        left -= steps[-1]
    return steps


def _engine(case, B, flags=CHUNK, profile=False):
    tr, enc = _trace(case)
    eng = make_engine(tr, enc, MODE, B, flags)
    eng.submit(enc["pods"])
    eng.set_profiling(profile)
    return eng


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


def _lockstep(case, B, steps, flags=CHUNK, profile=False):
    """Step the engine in lockstep with the oracle.  After every step: binds, usage, the invariants
    and the launches (a round commits at most B pods), and what the step read back early
    (ks_debug_counters [8], [9]): binds finished before the last wait, and those of them that came
    below a snapshot — none on a step too short for one, some on every step long enough.  Returns
    the binds and per step (launches, kernel statistics, snapshot binds)."""
    c = consts()
    eng = _engine(case, B, flags, profile)
    got, rows = [], []
    for k, (ob, orc, ou, _) in zip(steps, _oracle(case, steps)):
        assert orc == 0
        eb = eng.step(k)
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ou)
        _no_marks(eng)
        n = eng.last_step_stats()["launches"]
        base = -(-k // B)
        ctr = eng.debug_counters()
        early, snap = int(ctr[8]), int(ctr[9])
        print(f"{case} B={B} step {k}: base {base} launches {n} early {early} snapshot {snap}")
        assert n >= base, (k, n)
        assert 0 <= snap <= early <= k, (k, early, snap)
        if base >= c["early_min"]:
            # the first pass takes a snapshot after its round base - 1 - early_k: at least one pod
            # is below it (rounds other than a rescan's empty ones bind one or more), at most a batch per round
            assert 1 <= snap <= (base - c["early_k"]) * B, (k, base, snap)
        elif n < c["early_min"]:
            assert snap == 0, (k, n, snap)  # (no pass of the step can have been long enough)
        if n == base:
            assert early == snap, (k, early, snap)  # (one pass: nothing else finishes early)
        rows.append((n, eng.last_step_kernels() if profile else None, snap))
        got.append(eb)
    eng.close()
    return np.concatenate(got), rows


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", ["dense", "c2"])
def test_step_lengths_and_consecutive_steps(case, B):
    """Steps long enough for the early read-back, of exactly k B and k B + 1 pods at its minimum of
    k = 16 rounds, one round below it, short ones and of one pod, back to back (six or more steps on
    the C2 prefix).  On the 300-node dense trace launches stop early after a handful of pods, so a
    step is many passes, long and short: the snapshot falls low, the later passes finish the earlier
    ones' binds, and where it fits no step is long enough for a snapshot at all (192-pod batches)."""
    steps = step_lengths(PODS[case], B)
    if case == "c2":
        assert len(steps) >= 6 and max(steps) >= consts()["early_min"] * B
    _lockstep(case, B, steps)


def test_profiling_changes_neither_binds_nor_launches():
    """The launch identities of tests/test_round_rescan_gpu.py, profiling on; the same launches and
    binds with profiling off."""
    steps = step_lengths(PODS["c2"], 192)
    b_off, r_off = _lockstep("c2", 192, steps)
    b_on, r_on = _lockstep("c2", 192, steps, profile=True)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(b_on[f], b_off[f])
    assert [(n, sn) for n, _, sn in r_on] == [(n, sn) for n, _, sn in r_off]
    for n, k, _ in r_on:
        assert k["merge_n"] == n and k["scan_n"] == k["prep_n"] == k["resolve_n"] >= 1, (n, k)
        assert k["fused_n"] == n - k["prep_n"] and k["xchg_n"] == 0, (n, k)


def test_many_passes_with_small_e():
    """KS_ENGINE_SMALL_E: about every second round of a 192-pod batch on 5,000 nodes is a rescan's
    empty round, so every long pass leaves about half its pods and several more passes run, long
    ones with a snapshot of their own among them.  The binds equal the run without the flag (and
    the oracle's)."""
    steps = step_lengths(PODS["c2"], 192)
    b_small, rows = _lockstep("c2", 192, steps, CHUNK | SMALL_E, profile=True)
    b_plain, _ = _lockstep("c2", 192, steps, CHUNK)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(b_small[f], b_plain[f])
    passes = [k["prep_n"] for _, k, _ in rows]
    print("passes per step", passes)
    assert max(passes) >= 2, passes


@pytest.mark.parametrize("cap_at", ["early", "late"])
def test_clipping(cap_at):
    """cap smaller than the step's binds: the first cap rows as before, the step itself complete —
    with cap inside the range read back early and inside the last rounds."""
    B, steps = 65, [PODS["dense"] - 200, 200]
    cap = 100 if cap_at == "early" else steps[0] - 3
    (ob0, _, ou0, _), (ob1, _, ou1, _) = _oracle("dense", steps)
    eng = _engine("dense", B)
    eb = eng.step(steps[0], cap=cap)
    assert len(eb) == cap
    assert_same_binds(eb, {f: ob0[f][:cap] for f in ("pod", "node", "status", "tick")})
    np.testing.assert_array_equal(eng.usage(), ou0)
    assert eng.queued == steps[1]
    assert_same_binds(eng.step(steps[1]), ob1)
    np.testing.assert_array_equal(eng.usage(), ou1)
    eng.close()


WARM, FAIL_STEP = 4224, 4224  # 22 batches of 192 each


@pytest.mark.parametrize("off", [300, 3100], ids=["early_range", "last_rounds"])
@pytest.mark.parametrize("kind", ["bad_key", "not_found"])
def test_failing_pod(kind, off):
    """A bad-key pod and a NotFound pod in a 4,224-pod step of 192-pod batches on the C2 prefix, after
    a 4,224-pod step has filled the cluster enough for launches to commit about a hundred pods: the
    step's first pass is 22 rounds with the snapshot after its sixteenth, so pod 300 of the step lies
    in the range read back early (the snapshot reads the counter stopped at it: exactly the binds
    before it come back on the copy stream) and pod 3,100 past anything sixteen rounds of 192 can
    bind: in the rounds after the snapshot or in a later pass (some binds came early, not all).
    The binds before the pod are returned, the run stops at the pod's tick with the pod popped, the
    error and its text are the oracle's and ks_step's as before, and it is sticky."""
    from kubesim_amd.engine import KsError
    pod = WARM + off
    case = ("c2", kind, pod)
    P = PODS["c2"]
    (ob0, orc0, ou0, _), (ob, orc, _, otick) = _oracle(case, [WARM, FAIL_STEP])
    assert orc0 == 0
    assert orc == (_lib.KS_EINVAL if kind == "bad_key" else _lib.KS_ENOTFOUND) and len(ob["pod"]) == off
    eng = _engine(case, 192)
    assert_same_binds(eng.step(WARM), ob0)
    np.testing.assert_array_equal(eng.usage(), ou0)
    with pytest.raises(KsError) as ex:
        eng.step(FAIL_STEP)
    snap = int(eng.debug_counters()[9])
    print(f"{kind} at +{off}: launches {eng.last_step_stats()['launches']} snapshot {snap}")
    assert snap == off if off == 300 else 16 <= snap < off, (off, snap)
    assert ex.value.code == orc
    assert_same_binds(ex.value.binds, ob)
    assert eng.tick == otick and eng.queued == P - (pod + 1)
    text = (f'node "" not found (pod {pod}, tick {otick})' if kind == "not_found"
            else f"pod {pod}: invalid pod key or simSpec (tick {otick})")
    assert text in str(ex.value), str(ex.value)
    with pytest.raises(KsError) as ex2:
        eng.step(1)
    assert ex2.value.code == orc and len(ex2.value.binds) == 0
    eng.close()


def test_host_mirrors_after_an_early_read_back():
    """The host mirrors the early read-back writes in pieces (bound node, status, expired flags) are
    what the per-tick path reads: after a long step with a snapshot on an engine left to choose its
    own resolver (so that one-pod steps take the per-tick path, which passes each pod's expiries by
    value from those mirrors), forty one-pod steps and a short batched step still equal the oracle."""
    steps = [4224] + [1] * 40 + [500]
    tr, enc = _trace("c2")
    eng = make_engine(tr, enc, MODE, 192, 0)
    eng.submit(enc["pods"])
    for i, (k, (ob, orc, ou, _)) in enumerate(zip(steps, _oracle("c2", steps))):
        assert orc == 0
        assert_same_binds(eng.step(k), ob)
        if i == 0:
            ctr = eng.debug_counters()
            print("long step: early", int(ctr[8]), "snapshot", int(ctr[9]), "launches", eng.last_step_stats()["launches"])
            assert int(ctr[9]) >= 16
        elif k == 1:
            assert eng.last_step_stats()["launches"] == 1
        if i in (0, 20, 40, 41):
            np.testing.assert_array_equal(eng.usage(), ou)
    eng.close()
