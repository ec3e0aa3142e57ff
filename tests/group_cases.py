"""Scenario groups whose members differ: the inputs of tests/test_group_mixed_gpu.py, pinned on the
traces and the oracle alone by tests/test_group_cases.py.

ks_group_step (ks_step.cpp) decides for the whole group, per step: the evaluator class (the widest
any member needs), the scan's key-table word (16 bits only if every member's totals fit), the
resolver (the register-table one only if every member is in the small class), the scan grid (largest
block count x largest batch) and the merge kernel (merge_small up to 8 blocks).  MEMBERS are
recipes that each force one side of one of those choices; GROUPS put them together so that
neighbouring groups differ in one choice.

`restate` repeats the host's per-engine choices from a trace and a configuration alone:
ks_load_nodes (units = gcd of the capacities, default batch, block count), ks_submit_pods (units
fall to the gcd with every submitted request), update_mode (class thresholds), key16,
small_resolver and chunk_eligible.  No engine is imported here.
"""
from __future__ import annotations

import functools

import numpy as np

from harness import MODES, make_oracle, small_trace
from kubesim_amd import _lib, tracegen

# ks_device.h kEval*: a lower number is a wider class (ks_group_step takes the minimum)
WIDE, NARROW, TINY, MICRO = 0, 1, 2, 3
# update_mode's thresholds (ks_device.h)
MICRO_CAP, MICRO_PROD, TINY_CAP, NARROW_CAP, MICRO_WEIGHT = 1 << 16, 1 << 24, 1 << 26, 1 << 29, 1 << 24
BLOCK_NODES = 256          # ks::block_nodes()
DEFAULT_BATCH = 256        # kDefaultBatch
SMALL_MAX_BATCH, SMALL_MAX_NODES = 128, 8192   # RSmall::kMaxB, RSmall::kFilterBits
SMALL_MAX_EXP = 128        # RSmall::kMaxExp = kTMax - kMaxB
MERGE_SMALL_BLOCKS = 8     # launch_merge: nl_max * kTopL <= 64 lanes
SPLIT_MIN = 64             # KS_GROUP_SPLIT_MIN
POOL_MIN_BINDS = 1 << 18   # ks_group_step: binds of a step from which the unpack runs on a thread pool

CHUNKS = (1, 37, 250, 1000)   # the ticks of test_mixed_group_matches_oracle's steps
SPLIT_STEPS = (50, 300, 400)  # of test_two_stream_split_ragged_halves


# ---- the host's choices, restated ------------------------------------------------------------
def default_batch(n: int, batch_pods: int = 0) -> int:
    """ks_load_nodes (a group member never takes the chunk resolver's batch)."""
    if batch_pods:
        return batch_pods
    if n < 16 * DEFAULT_BATCH:
        return int(min(max(n // 16 // 32 * 32, 64), DEFAULT_BATCH))
    return DEFAULT_BATCH


def block_count(n: int) -> int:
    return (max(n, 1) + BLOCK_NODES - 1) // BLOCK_NODES


def small_class(batch: int, n: int) -> bool:
    """small_resolver()."""
    return batch <= SMALL_MAX_BATCH and n <= SMALL_MAX_NODES


def weights(scorers):
    """engine_init: (const_total, w_lr, w_ba) of a scorer list (kind 0 const, 1 LeastRequested, 2 Balanced)."""
    const = sum(w * v for k, w, v in scorers if k == 0)
    return const, sum(w for k, w, _ in scorers if k == 1), sum(w for k, w, _ in scorers if k == 2)


def key16(scorers) -> bool:
    """key16(): every total + 1 fits 16 bits."""
    const, w_lr, w_ba = weights(scorers)
    return const + 10 * (w_lr + w_ba) + 1 < (1 << 16)


def units(trace, hi=None):
    """Per resource the gcd of every present capacity and of the requests of pods [0, hi)
    (ks_load_nodes, then ks_submit_pods), and the largest capacity."""
    nd, p = trace["nodes"], trace["pods"]
    hi = p["m"] if hi is None else hi
    unit, mx = [], []
    for k in range(3):
        cap = nd["alloc"][(nd["alloc_has"] >> k) & 1 == 1, k]
        req = p["req"][:hi][(p["req_has"][:hi] >> k) & 1 == 1, k]
        cap, req = cap[cap > 0].astype(np.int64), req[req > 0].astype(np.int64)
        # no positive capacity: the unit starts at 1 and stays there
        unit.append(int(np.gcd.reduce(np.concatenate([cap, req]))) if len(cap) else 1)
        mx.append(int(cap.max()) if len(cap) else 0)
    return unit, mx


def eval_class(scaled_max, scorers, engine_flags=0) -> int:
    """update_mode()."""
    m = scaled_max
    _, w_lr, w_ba = weights(scorers)
    narrow = max(m) < NARROW_CAP
    tiny = max(m) < TINY_CAP and m[0] * m[1] < TINY_CAP
    micro = max(m) < MICRO_CAP and m[0] * m[1] < MICRO_PROD and max(w_lr, w_ba) < MICRO_WEIGHT
    no_tiny = bool(engine_flags & _lib.KS_ENGINE_NO_TINY)
    if engine_flags & _lib.KS_ENGINE_FORCE_WIDE:
        return WIDE
    if micro and not no_tiny and not engine_flags & _lib.KS_ENGINE_NO_MICRO:
        return MICRO
    if tiny and not no_tiny:
        return TINY
    return NARROW if narrow else WIDE


def restate(trace, mode, batch_pods=0, engine_flags=0, hi=None):
    """What the host picks for an engine holding the trace's nodes and its pods [0, hi)."""
    _, _, scorers = MODES[mode] if isinstance(mode, str) else mode
    n = trace["nodes"]["n"]
    unit, mx = units(trace, hi)
    scaled = [m // u for m, u in zip(mx, unit)]
    b = default_batch(n, batch_pods)
    return dict(n=n, unit=unit, scaled_max=scaled, cls=eval_class(scaled, scorers, engine_flags), B=b,
                blocks=block_count(n), small=small_class(b, n), k16=key16(scorers))


def chunk_eligible(r) -> bool:
    """chunk_eligible() from restate's choices: batches of at most kWinMaxB pods, node state in
    32-bit words (the classes from narrow on; the wide class while every scaled capacity is below
    2^32 - 1) and totals in 16 bits."""
    words = r["cls"] >= NARROW or max(r["scaled_max"]) < 0xFFFFFFFF
    return r["B"] <= _lib.KS_WIN_MAX_B and words and r["k16"]


def group_choices(restated):
    """ks_group_step's group-wide picks from its members' restated choices."""
    return dict(mode=min(r["cls"] for r in restated), k16=all(r["k16"] for r in restated),
                resolver="RSmall" if all(r["small"] for r in restated) else "RBig",
                merge="merge_small" if max(r["blocks"] for r in restated) <= MERGE_SMALL_BLOCKS else "merge_kernel",
                batches=sorted({r["B"] for r in restated}))


def halves(s: int):
    """ks_group_step's scenario halves: [0, S / 2) and [S / 2, S) from KS_GROUP_SPLIT_MIN members on."""
    return [(0, s // 2), (s // 2, s)] if s >= SPLIT_MIN else [(0, s)]


# ---- member recipes ----------------------------------------------------------------------------
SHORT_SEED = 14  # the windows of the batches that start at pods 38 and 288 (step starts) hold 129 expiries


def _short():
    tr = small_trace(SHORT_SEED, n_nodes=500, n_pods=900, taints=False, selectors=False, tolerations=False)
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) % 12)  # as test_short_pods_many_expiries
    return tr


STREAM_SEED = 28  # runs to its end (most seeds stop with NotFound at 150 nodes), first arrival at tick 2


def _stream():
    """Arrivals 0-2 ticks apart; one selector pair per pod, as c4_scenario."""
    return small_trace(STREAM_SEED, n_nodes=150, n_pods=500, arrival="stream", max_sel_pairs=1)


RESCALE_CUT = 350


def _rescale(n_pods=700):
    """test_memory_unit_rescale_mid_run's recipe at 300 nodes and 700 pods: pods from RESCALE_CUT on
    request a fractional byte and are submitted later, between two group steps."""
    tr = small_trace(31, n_nodes=300, n_pods=n_pods, taints=False, selectors=False, tolerations=False)
    tr["pods"]["req"][RESCALE_CUT:, 1] += 1  # +1 milli-byte: not a whole byte
    return tr


def _c4(s, n, p, **kw):
    return lambda: tracegen.c4_scenario(s, n_nodes=n, n_pods=p, **kw)


def _m(build, mode, forces, batch_pods=0, engine_flags=0, late=None):
    """late = (chunk index before which the second part goes in, first pod of that part)."""
    return dict(build=build, mode=mode, batch_pods=batch_pods, engine_flags=engine_flags, forces=forces, late=late)


def _f(cls, B, blocks, small, k16=True):
    return dict(cls=cls, B=B, blocks=blocks, small=small, k16=k16)


K32_MODE = (1, 7, ((1, 4000, 0), (2, 3000, 0)))  # totals up to 70,001

MEMBERS = {
    "tiny64": _m(_c4(0, 64, 400), "feeds_all_lrba", _f(MICRO, 64, 1, True)),
    "c4": _m(_c4(1, 2000, 900), "feeds_all_lrba", _f(MICRO, 96, 8, True)),
    "b160": _m(_c4(2, 3000, 900), "feeds_fit_lr", _f(MICRO, 160, 12, False)),
    "big": _m(_c4(3, 5000, 700), "feeds_all_lrba", _f(MICRO, 256, 20, False)),
    "wideq": _m(_c4(4, 700, 800, mem_decimal=True), "feeds_all_lrba", _f(WIDE, 64, 3, True)),
    "forcedw": _m(_c4(5, 300, 600), "feeds_taint_sel_ba_const", _f(WIDE, 64, 2, True),
                  engine_flags=_lib.KS_ENGINE_FORCE_WIDE),
    "k32": _m(_c4(6, 300, 600), K32_MODE, _f(MICRO, 64, 2, True, k16=False)),
    "literal": _m(lambda: small_trace(7, n_nodes=200, n_pods=700), "literal_lrba_filters_ignored",
                  _f(MICRO, 3, 1, True), batch_pods=3),
    "short": _m(_short, "feeds_all_lrba", _f(MICRO, 128, 2, True), batch_pods=128),
    "stream": _m(_stream, "feeds_all_lrba", _f(MICRO, 64, 1, True)),
    "rescale": _m(_rescale, "feeds_all_lrba", _f(WIDE, 64, 2, True), late=(3, RESCALE_CUT)),
}

GROUPS = {
    "small_uniform_class": ("tiny64", "c4", "short"),
    "small_with_wide": ("tiny64", "c4", "wideq", "forcedw"),
    "small_with_k32": ("tiny64", "c4", "k32", "literal"),
    "role_by_batch": ("tiny64", "c4", "b160"),
    "everything": tuple(MEMBERS),
}
# the group-wide choices each is built to force (tests/test_group_cases.py asserts them)
GROUP_FORCES = {
    "small_uniform_class": dict(mode=MICRO, k16=True, resolver="RSmall", merge="merge_small", batches=[64, 96, 128]),
    "small_with_wide": dict(mode=WIDE, k16=True, resolver="RSmall", merge="merge_small", batches=[64, 96]),
    "small_with_k32": dict(mode=MICRO, k16=False, resolver="RSmall", merge="merge_small", batches=[3, 64, 96]),
    "role_by_batch": dict(mode=MICRO, k16=True, resolver="RBig", merge="merge_kernel", batches=[64, 96, 160]),
    "everything": dict(mode=WIDE, k16=False, resolver="RBig", merge="merge_kernel", batches=[3, 64, 96, 128, 160, 256]),
}
# members of several groups whose binds must not depend on their siblings
SHARED = ("tiny64", "c4", "literal", "short")


# ---- the 65-member groups ------------------------------------------------------------------------
SPLIT_N = 65
SPLIT_MODES = ("feeds_all_lrba", "feeds_fit_lr", "feeds_taint_sel_ba_const", "literal_lrba_filters_ignored")
SPLIT_WIDE = (5, 40)     # KS_ENGINE_FORCE_WIDE: one in each half
SPLIT_RESCALE = 50       # the `rescale` recipe; its second part goes in before the second step
# ... with 750 pods: the other members have at most 599, and the halves' longest queues must differ
# by two batches of 64 (with the recipe's 700 pods they differ by 101)
SPLIT_RESCALE_PODS = 750


def split_member(i: int):
    mode = SPLIT_MODES[i % 4]
    if i == SPLIT_RESCALE:
        return _m(lambda: _rescale(SPLIT_RESCALE_PODS), "feeds_all_lrba", None, late=(1, RESCALE_CUT))
    return _m(_c4(100 + i, 64 + (i * 29) % 137, 100 + (i * 37) % 500), mode, None,
              engine_flags=_lib.KS_ENGINE_FORCE_WIDE if i in SPLIT_WIDE else 0)


POOL_N, POOL_PODS = 65, 4200


def pool_member(i: int):
    return _m(lambda: small_trace(200 + i, n_nodes=64, n_pods=POOL_PODS), "literal_lrba_filters_ignored", None)


def recipe(key):
    """A member recipe by key: a MEMBERS name, ("split65", i) or ("pool65", i)."""
    if isinstance(key, str):
        return MEMBERS[key]
    return split_member(key[1]) if key[0] == "split65" else pool_member(key[1])


def steps_of(key):
    if isinstance(key, str):
        return CHUNKS
    return SPLIT_STEPS if key[0] == "split65" else (POOL_PODS,)


@functools.lru_cache(maxsize=None)
def trace_of(key):
    """(trace, encoded trace); built once, never changed afterwards."""
    from harness import encoded
    tr = recipe(key)["build"]()
    return tr, encoded(tr)


def parts_of(key):
    """[(step index before which the part is submitted, first pod, end pod)]."""
    tr, _ = trace_of(key)
    m, late = tr["pods"]["m"], recipe(key)["late"]
    return [(0, 0, m)] if late is None else [(0, 0, late[1]), (late[0], late[1], m)]


# ---- the oracle's run of a member, once ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(key):
    """The member's oracle run over its step schedule.  Per step: the binds, the stop code (sticky,
    as ks_group_step reports it), the usage, tick and queue length after it; a tick inside the step
    with the usage there; the next queued pod with the oracle's filter / score of it (None once the
    run has stopped or the queue is empty).  Nothing in it is changed afterwards."""
    tr, _ = trace_of(key)
    r = recipe(key)
    ora = make_oracle(tr, r["mode"])
    parts = parts_of(key)
    empty = lambda: dict(pod=np.zeros(0, np.int64), node=np.zeros(0, np.int32), tick=np.zeros(0, np.int64),
                         status=np.zeros(0, np.int32))
    steps, rc, tick, popped, submitted = [], 0, 0, 0, 0
    for s, k in enumerate(steps_of(key)):
        for at, lo, hi in parts:
            if at == s:
                ora.submit(tracegen.slice_pods(tr, lo, hi))
                submitted = hi
        st = dict(binds=empty(), rc=rc, usage=None, mid=None, probe=None, lo=tick)
        if rc == 0:
            h = max(1, k // 2)
            b1, rc = ora.step(h, cap=h)
            if rc == 0:
                st["mid"] = (tick + h, ora.usage())
                b2, rc = ora.step(k - h, cap=max(k - h, 1)) if k > h else (empty(), 0)
                b1 = {f: np.concatenate([b1[f], b2[f]]) for f in b1}
            st["binds"], st["rc"] = b1, rc
            popped += len(b1["pod"]) + (rc != 0)
            tick += k
            if rc == 0:
                st["usage"] = ora.usage()
                if popped < submitted:
                    st["probe"] = (popped,) + ora.eval(popped)
        st["tick"] = ora.tick
        st["queued"] = submitted - popped
        steps.append(st)
    ora.close()
    return steps


def all_binds(key):
    steps = reference(key)
    return {f: np.concatenate([s["binds"][f] for s in steps]) for f in ("pod", "node", "tick", "status")}


def final_code(key):
    return reference(key)[-1]["rc"]


def durations(trace):
    """Ticks a pod runs once bound Ok: ceil(int32 wrapping sum of its phase seconds / tick) if
    positive, else 0 (kubesim/pod/pod.go:155-162; ks_submit_pods)."""
    p = trace["pods"]
    sec = np.zeros(p["m"], np.int64)
    np.add.at(sec, np.repeat(np.arange(p["m"]), np.diff(p["phase_off"])), p["phase_sec"].astype(np.int64))
    sec = (sec + 2**31) % 2**32 - 2**31
    t = trace["tick_seconds"]
    return np.where(sec > 0, (sec + t - 1) // t, 0)
