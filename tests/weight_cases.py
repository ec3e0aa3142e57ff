"""Scorer weights at the thresholds of the configured maximum total const_total + 10 * (w_lr + w_ba):
the inputs of tests/test_weight_paths_gpu.py (the engine against the oracle on every path), pinned on
the oracle alone by tests/test_weight_cases.py.

The host changes how the device works at three values of that maximum (ks_engine.cpp, ks_plan.h): key16() keeps
the scan's 16-bit key table, and chunk_eligible() the chunk resolver, while maximum + 1 < 2^16;
update_mode() takes the micro evaluator while both weights are below kMicroWeight = 2^24; ks_create
accepts a maximum up to 2^30 - 3 (the resolvers' 30-bit key of total + 1).  CLASSES put a
configuration on either side of each.

A total equals the maximum only where LeastRequested = BalancedAllocation = 10: a pod that requests
0 cpu and 0 memory on a node whose running pods request nothing.  The traces plant such *top pods*
(the first three and every 16th) and keep a stripe of nodes that only they tolerate, so that nodes
with nothing requested exist throughout the run.

Nothing here imports the engine.  Traces and oracle runs are built once per process and never
changed afterwards.
"""
from __future__ import annotations

import functools

import numpy as np

from harness import encoded, make_oracle, small_trace
from kubesim_amd import tracegen

# (kind, weight, value): kind 0 const, 1 LeastRequested, 2 BalancedAllocation
CLASSES = {
    "w16": ((1, 3276, 0), (2, 3277, 0), (0, 1, 4)),
    "w16p": ((1, 3276, 0), (2, 3277, 0), (0, 1, 5)),
    "w17": ((1, 7000, 0), (2, 6000, 0), (0, 1, 3)),
    "wmicro": ((1, (1 << 24) - 1, 0), (2, (1 << 24) - 1, 0), (0, 1000, 1)),
    "wmicro1": ((1, 1 << 24, 0), (2, (1 << 24) - 1, 0), (0, 1000, 1)),
    "wmax": ((1, 53687090, 0), (2, 53687090, 0), (0, 3, 7)),
    "split8": ((1, 3000, 0), (0, 0, 9), (2, 1500, 0), (1, 1000, 0), (0, 7, 0), (2, 1500, 0), (1, 0, 0), (0, 1, 1)),
}
# the configured maximum total of each, written out (tests/test_weight_cases.py checks the sums)
MAXIMUM = {"w16": 65_534, "w16p": 65_535, "w17": 130_003, "wmicro": 335_545_300, "wmicro1": 335_545_310,
           "wmax": (1 << 30) - 3, "split8": 70_001}
SPLIT8_FOLDED = ((1, 4000, 0), (2, 3000, 0), (0, 1, 1))
FILTER_MODE, FILTERS = 1, 7


def mode(cls):
    """The (filter_mode, filters, scorers) tuple harness.make_engine / make_oracle take; `cls` is a
    CLASSES name or a scorer tuple."""
    return FILTER_MODE, FILTERS, CLASSES[cls] if isinstance(cls, str) else tuple(cls)


# name: (nodes, pods, seed).  Stream arrivals, one selector pair per pod; the seeds are ones whose
# oracle run binds every pod under every class (most seeds stop with NotFound at 400 nodes).
# "T" is the per-tick kernel's trace: five evaluating workgroups plus the copier.
SIZES = {"S": (400, 300, 28), "M": (2500, 1200, 28), "L": (9000, 1500, 28), "T": (5000, 600, 28)}
STEPS = (1, 37)            # the first two steps of every run; a third takes the rest
TOP_EVERY, TOP_FIRST = 16, 3
STRIPE_EVERY, STRIPE_AT = 8, 5     # nodes i % 8 == 5 carry the reserved taint
RESERVED_TAINT = ("weights.sim/reserved", "top")
SAMPLE_EVERY = 50          # pods whose whole score vector the reference keeps
PHASE_SHRINK = 16          # phases of 1 .. 226 ticks: expiries all through the run
# cpu and memory capacities halved (4 .. 64 cores, 16 .. 256 Gi): a pod of the trace is then a large
# part of a small node, so an ordinary pod meets totals below 2^16 beside its best (w17's truncation
# pin; at full size the argmax of the truncated totals moved for 9 of 24 sampled pods, not for half)
CAP_SHRINK = 2


def is_top(q):
    q = np.asarray(q)
    return (q < TOP_FIRST) | (q % TOP_EVERY == 0)


def _replace_rows(off, rows, keep, new_rows):
    """CSR (off, rows) with the rows of every item outside `keep` replaced by `new_rows`."""
    parts, counts = [], []
    for i in range(len(off) - 1):
        r = rows[off[i]:off[i + 1]] if keep[i] else new_rows
        parts.append(np.asarray(r, np.int32).reshape(-1, rows.shape[1]))
        counts.append(len(parts[-1]))
    out = np.concatenate(parts) if parts else rows[:0]
    new_off = np.zeros(len(off), np.int32)
    np.cumsum(counts, out=new_off[1:])
    return new_off, out.astype(np.int32)


def plant(tr):
    """Top pods and the reserved stripe, in place.  A top pod names cpu and memory with a request of
    0 (req_has = 3), has no selector and one toleration that tolerates every taint.  The stripe's
    nodes carry a NoExecute taint of their own; every other pod's tolerate-everything toleration
    (empty key, Exists, no effect) is narrowed to NoSchedule, so none of them tolerates it.  Phases
    are shortened (PHASE_SHRINK) and cpu / memory capacities halved (CAP_SHRINK)."""
    nd, p = tr["nodes"], tr["pods"]
    st = tracegen.StringTable()
    st.strings = list(tr["strings"])
    st.index = {x: i for i, x in enumerate(st.strings)}
    key, val = (st.intern(x) for x in RESERVED_TAINT)
    tr["strings"] = st.strings
    n, m = nd["n"], p["m"]
    top = is_top(np.arange(m))

    # the stripe: one more taint row per node
    stripe = np.arange(n) % STRIPE_EVERY == STRIPE_AT
    parts, counts = [], []
    for i in range(n):
        r = nd["taint"][nd["taint_off"][i]:nd["taint_off"][i + 1]]
        if stripe[i]:
            r = np.concatenate([r, np.array([[key, val, tracegen.NO_EXECUTE]], np.int32)])
        parts.append(r)
        counts.append(len(r))
    nd["taint"] = np.concatenate(parts).astype(np.int32)
    nd["taint_off"] = np.zeros(n + 1, np.int32)
    np.cumsum(counts, out=nd["taint_off"][1:])

    tol = p["tol"]
    everything = (tol[:, 0] == 0) & (tol[:, 1] == tracegen.OP_EXISTS) & (tol[:, 3] == tracegen.EFFECT_NONE)
    tol[everything, 3] = tracegen.NO_SCHEDULE
    p["tol_off"], p["tol"] = _replace_rows(p["tol_off"], tol, ~top,
                                           [[0, tracegen.OP_EXISTS, 0, tracegen.EFFECT_NONE]])
    p["sel_off"], p["sel"] = _replace_rows(p["sel_off"], p["sel"], ~top, np.zeros((0, 2), np.int32))
    p["req"][top] = 0
    p["req_has"][top] = tracegen.HAS_CPU | tracegen.HAS_MEM
    owner = np.repeat(np.arange(m), np.diff(p["phase_off"]))
    p["phase_use"][top[owner]] = 0
    p["phase_sec"][:] = 10 + (p["phase_sec"] - 10) // PHASE_SHRINK
    nd["alloc"][:, :2] //= CAP_SHRINK
    return tr


@functools.lru_cache(maxsize=None)
def trace_of(size):
    """(trace, encoded trace) of a SIZES entry."""
    n, m, seed = SIZES[size]
    tr = plant(small_trace(seed, n_nodes=n, n_pods=m, arrival="stream", max_sel_pairs=1))
    return tr, encoded(tr)


def ticks_of(size):
    """The ticks of a whole run: one past the last bind (a pod is bound at its arrival tick, or the
    tick after its predecessor's bind if that is later)."""
    tr, _ = trace_of(size)
    t = 0
    for a in tr["pods"]["arrival"].tolist():
        t = max(a, t + 1)
    return t + 1


def steps_of(size):
    return STEPS + (ticks_of(size) - sum(STEPS),)


def _argmax1(total1):
    """The lowest-index maximum of score + 1 (0: no entry), -1 if no node has an entry."""
    return int(np.argmax(total1)) if total1.max(initial=0) > 0 else -1


@functools.lru_cache(maxsize=None)
def reference(size, cls):
    """The oracle's run of (size, class), stepped tick by tick once.  binds: the whole run; usage:
    after each of steps_of(size); win_total: per bind the oracle's total of the winner just before the
    bind (ora.eval); trunc_moves: per bind whether the lowest-index maximum of (total + 1) & 0xFFFF
    is another node than that of total + 1; evals: {pod: (feasible, score)} of every SAMPLE_EVERY-th
    pod just before its bind.  ora.eval sees the state one tick before the bind: a pod that ends at
    the bind tick still counts on its node, so a count of binds won at the maximum read from
    win_total is a lower bound."""
    scorers = cls if not isinstance(cls, str) else CLASSES[cls]
    tr, _ = trace_of(size)
    m = tr["pods"]["m"]
    ora = make_oracle(tr, mode(scorers))
    ora.submit(tr)
    cuts = np.cumsum(steps_of(size))
    binds = {f: [] for f in ("pod", "node", "tick", "status")}
    usage, win_total, trunc_moves, evals = [], [], [], {}
    q, rc = 0, 0
    for t in range(1, int(cuts[-1]) + 1):
        feas = score = None
        if q < m:
            feas, score = ora.eval(q)
        b, rc = ora.step(1, cap=1)
        assert rc == 0, f"{size}/{cls}: the oracle stopped with {rc} at tick {t} (pod {q})"
        if len(b["pod"]):
            assert int(b["pod"][0]) == q
            for f in binds:
                binds[f].append(b[f][0])
            w = int(b["node"][0])
            win_total.append(int(score[w]))
            trunc_moves.append(_argmax1((score + 1) & 0xFFFF) != _argmax1(score + 1))
            if q % SAMPLE_EVERY == 0:
                evals[q] = (feas, score)
            q += 1
        if t in cuts:
            usage.append(ora.usage())
    ora.close()
    assert q == m, f"{size}/{cls}: {m - q} pods left in the queue"
    dt = dict(pod=np.int64, node=np.int32, tick=np.int64, status=np.int32)
    return dict(binds={f: np.array(v, dt[f]) for f, v in binds.items()}, usage=usage,
                win_total=np.array(win_total, np.int64), trunc_moves=np.array(trunc_moves, bool), evals=evals)


def step_binds(size, cls):
    """reference()'s binds cut at steps_of(size)."""
    b = reference(size, cls)["binds"]
    hi = np.searchsorted(b["tick"], np.cumsum(steps_of(size)), side="right")
    lo = np.concatenate([[0], hi[:-1]])
    return [{f: v[a:z] for f, v in b.items()} for a, z in zip(lo, hi)]


def state_before(size, cls, q, at_eval=False):
    """[n][4] requested state pod q was scheduled against, from state_ref on the oracle's binds: the
    pods running at its bind tick without the pod itself.  at_eval: the state reference()'s evals
    saw instead, one tick earlier (pods that end at the bind tick still count)."""
    import state_ref
    tr, enc = trace_of(size)
    b = reference(size, cls)["binds"]
    ref = state_ref.IntervalRef(tr, b)
    i = int(np.searchsorted(b["pod"], q))
    if at_eval:
        return ref.at(int(b["tick"][i]) - 1)
    state = ref.at(int(b["tick"][i]))
    if b["status"][i] == state_ref.OK and ref.dur_all[q] > 0:
        state[b["node"][i], :3] -= enc["pods"]["req"][q]
        state[b["node"][i], 3] -= 1
    return state


def score_before(size, scorers, state, q):
    """(score, mask) pod q would get against `state` under `scorers` — drain_ref.score_vector, the
    integer restatement of the scorers: -1 where the node has no entry."""
    import drain_ref
    import place_ref
    tr, enc = trace_of(size)
    e = enc["pods"]
    cfg = place_ref.engine_cfg(mode(scorers), enc)
    n = len(enc["alloc"])
    shape = ([int(x) for x in e["req"][q]], int(e["keymask"][q]), int(e["tol"][q]), int(e["sel"][q]))
    v = drain_ref.score_vector(cfg, np.asarray(enc["alloc"], np.int64), state, np.asarray(enc["taint"], np.uint64),
                               np.asarray(enc["label"], np.uint64), np.ones(n, bool), shape)
    return v - 1, (v > 0).astype(np.uint8)
