"""Run stops decided by state that changes inside a batch.  The traces, step plans and cached oracle
runs of tests/test_stop_gpu.py (every resolver chain against the oracle), pinned on the oracle alone
by tests/test_stop_cases.py.

A run stops when scheduleOne finds no node (NotFound, kubesim/kubesim.go:217-220) or CreatePod
rejects the pod (InvalidArgument).  Here the stop hangs on a scarce resource that saturates:

* every node's gpu capacity is 0 (key present) and every pod's gpu request 0, so cpu and memory
  (quartered: everything fits) never refuse a pod;
* G nodes at spread-out indices hold c gpus each: S = G * c slots;
* the S slot pods X - 2, X - 4 .. X - 2S each request 1 gpu and run LONG ticks; bulk arrivals, so
  pod i binds at tick i + 1 and the slots fill two ticks apart up to tick X - 1;
* the deciding pod X requests 1 gpu as well.

A case varies the run length of one slot pod (the freeing pod), the flags of a pod, or the mode:
whether X finds a node depends on what the pods just before it did — the only kind of stop a
batched resolver can get wrong.  Two saturations stand on either side of the resolvers' list lengths
(ks_device.h): g6 has fewer gpu nodes than kTopL, so a slot pod's snapshot list is short and never
full; g32 has more than KS_CHR, so lists are truncated or full and the exhausted-list rescan fires
before the final NotFound.

A plan puts X at index p of the first batch of a pass by ending the step before it p pods short of
X; the engines take batch_pods explicitly (B), so the positions are the test's choice.

No engine is imported here.
"""
from __future__ import annotations

import copy
import functools

import numpy as np

import expiry_burst_cases as ec
from chunk_replay_cases import set_run_ticks
from harness import MODES, encoded, make_oracle, small_trace
from kubesim_amd import tracegen
from pysim import PySim, RES

# restated from the sources (tests/test_stop_cases.py compares them)
TOP_L = 8          # ks_device.h kTopL: exact snapshot candidates kept per pod
CHR = 20           # ks_device.h KS_CHR: static candidates the chunk resolver keeps per pod
KC = 64            # ks_chunk.hip kC: pods per chunk
B_CHUNK = 192      # ks_engine.cpp kChunkBatch: the chunk-resolver engines' batch
B_ONE_POD = 256    # the role-split resolver's batch (ks_device.h kWinMaxB)
B_SMALL = 128      # RSmall::kMaxB
BLOCK_NODES = 256  # ks::block_nodes(): nodes per scan block

MODE = ec.MODE
LITERAL = ec.LITERAL
LONG = ec.LONG
KS_EINVAL, KS_ENOTFOUND = 1, 2   # include/ks_engine.h ks_status
BAD_KEY, BAD_SPEC = 1, 2         # pod flags (oracle/ks_oracle.h KO_FLAG_*)

SATS = {"g6": (6, 4), "g32": (32, 2)}   # name: (gpu nodes G, gpus per node c)
# name: (nodes, X, pods).  X - B >= 200 for every batch size: the warm step is a few hundred pods;
# pods >= X + B + 64: the step that holds X is full, and the one that runs through it goes on.
CLUSTERS = {
    "3k": (3000, 480, 800),            # past the small class, chunk-eligible, 12 scan blocks
    "small": (ec.SMALL_NODES, 480, 800),   # the small class at batch 128
    "pipe": (ec.PIPE_NODES, 272, 540),     # 257 scan blocks in two parts: the pipelined chain (a warm step of two batches)
}

STOPS = ("full", "too_late", "bad_key", "bad_spec", "full_and_bad_key", "literal_bad_key",
         "two_stops_key_first", "two_stops_full_first")
RESCUES = ("rescued_own", "rescued_earlier", "rescued_earlier_contended", "rescued_in_batch",
           "rescued_in_batch_edge")
CASES = STOPS + RESCUES


def slots(sat):
    g, c = SATS[sat]
    return g * c


def gpu_nodes(sat, n):
    """G indices spread over the whole cluster (several scan blocks, several parts of a sharded engine)."""
    return np.linspace(3, n - 5, SATS[sat][0]).astype(np.int64)


def edge_p(sat):
    """rescued_in_batch_edge: with X at this index of its batch the freeing pod X - 2S is the last pod
    of the batch's first chunk, and its expiry (attached to X - 1) lies in a later chunk."""
    return KC - 1 + 2 * slots(sat)


def spec(name, sat, x):
    """What a case changes on the saturated trace: dict(mode, runs {pod: ticks}, flags {pod: flag},
    stop (code, pod) or None, freed (the freeing pod, where X must bind on its node) or None, shift (the
    slot pods are X - shift - 2 .. X - shift - 2S), before (feasible nodes for X one tick
    before its own, None = not pinned), carried (live expiries attached to X))."""
    s = slots(sat)
    first = x - 2 * s                 # the earliest slot pod: bound at tick first + 1; X binds at x + 1
    d = dict(mode=MODE, runs={}, flags={}, stop=None, freed=None, before=None, carried=0, shift=0)
    if name == "full":
        d.update(stop=(KS_ENOTFOUND, x), before=0)
    elif name == "rescued_own":       # ends exactly at X's bind tick: the expiry is X's own
        d.update(runs={first: 2 * s}, freed=first, before=0, carried=1)
    elif name == "too_late":          # one tick later
        d.update(runs={first: 2 * s + 1}, stop=(KS_ENOTFOUND, x), before=0)
    elif name == "rescued_earlier":
        # ends 5 ticks before X's bind tick: attached to pod X - 5.  The slot pods are X - 6, X - 8 ..
        # here (shift 4), so that no slot pod binds between the expiry and X and the freed slot is X's
        d.update(runs={first - 4: 2 * s - 1}, freed=first - 4, before=1, shift=4)
    elif name == "rescued_earlier_contended":
        # the same end on the unshifted trace: the slot pods X - 4 and X - 2 bind after the expiry, so
        # three slots are open at X - 4 and X takes the one the two leave (not pinned to the freed node)
        d.update(runs={first: 2 * s - 5}, before=1)
    elif name == "rescued_in_batch":  # bound 4 pods before X, ends at tick X: attached to pod X - 1
        d.update(runs={x - 4: 3}, freed=x - 4, before=1)
    elif name == "rescued_in_batch_edge":
        d.update(runs={first: 2 * s - 1}, freed=first, before=1)
    elif name in ("bad_key", "bad_spec"):   # a slot is free, the pod itself is refused
        d.update(runs={first: 2 * s - 5}, flags={x: BAD_KEY if name == "bad_key" else BAD_SPEC},
                 stop=(KS_EINVAL, x), before=1)
    elif name == "full_and_bad_key":  # NotFound comes first (ks_oracle.c schedule_one)
        d.update(flags={x: BAD_KEY}, stop=(KS_ENOTFOUND, x), before=0)
    elif name == "literal_bad_key":   # filters ignored: the pod has a node, over capacity; refused before any bind
        d.update(mode=LITERAL, flags={x: BAD_KEY}, stop=(KS_EINVAL, x))
    elif name == "two_stops_key_first":
        d.update(flags={x - 3: BAD_KEY}, stop=(KS_EINVAL, x - 3))
    elif name == "two_stops_full_first":
        d.update(flags={x + 3: BAD_KEY}, stop=(KS_ENOTFOUND, x), before=0)
    else:
        raise KeyError(name)
    return d


# ---- traces -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(sat, cluster, shift=0):
    """The saturated trace with every slot pod running LONG ticks (case `full`), and its run lengths."""
    n, x, m = CLUSTERS[cluster]
    g, c = SATS[sat]
    s = g * c
    assert x - shift - 2 * s >= 100 and m >= x + (B_CHUNK if cluster == "pipe" else B_ONE_POD) + KC
    tr = ec._quarter(small_trace(11, n_nodes=n, n_pods=m, taints=False, selectors=False, tolerations=False,
                                 gpu_absent_p=0.0))
    nd, p = tr["nodes"], tr["pods"]
    assert (nd["alloc_has"] & tracegen.HAS_GPU).all()
    nd["alloc"][:, tracegen.GPU] = 0
    nd["alloc"][gpu_nodes(sat, n), tracegen.GPU] = c * tracegen.MILLI
    p["req"][:, tracegen.GPU] = 0
    p["phase_use"][:, tracegen.GPU] = 0
    want = np.concatenate([np.arange(x - shift - 2 * s, x - shift, 2), [x]])     # the slot pods and X
    p["req"][want, tracegen.GPU] = tracegen.MILLI
    owner = np.repeat(np.arange(m), np.diff(p["phase_off"]))
    p["phase_use"][np.isin(owner, want), tracegen.GPU] = tracegen.MILLI
    # the background: every third pod runs 1-12 ticks, none of them ends on X's bind tick or the next
    i = np.arange(m)
    run = np.where(i % 3 == 0, 1 + (i * 7) % 12, LONG).astype(np.int64)
    run[want] = LONG
    run[np.isin(i + 1 + run, (x + 1, x + 2))] = LONG
    return tr, run


@functools.lru_cache(maxsize=None)
def case(name, sat, cluster):
    """dict(tr, enc, run, x, m, n, s, nodes (the gpu nodes), + spec()'s fields); built once, never changed."""
    n, x, m = CLUSTERS[cluster]
    d = spec(name, sat, x)
    base, run = _base(sat, cluster, d["shift"])
    tr = copy.deepcopy(base)
    run = run.copy()
    for pod, ticks in d["runs"].items():
        run[pod] = ticks
    for pod, flag in d["flags"].items():
        tr["pods"]["flags"][pod] = flag
    set_run_ticks(tr, run)
    d.update(tr=tr, enc=encoded(tr), run=run, x=x, m=m, n=n, s=slots(sat), nodes=gpu_nodes(sat, n))
    return d


# ---- step plans -------------------------------------------------------------------------------------
def positions(b):
    """The indices of its batch at which X is put: a pass's first pod, its second, both sides of the
    first chunk edge, the batch's last pod, and (p = B) the first pod of the next batch."""
    return (0, 1, KC - 1, KC, b - 1, b)


def plan(cluster, b, p, how="step"):
    """Step lengths in ticks.  p < b: a warm step to X - p, one step of b ticks (one batch, X its p-th
    pod), the rest.  p == b: X is the first pod of the batch after the step's — `ends_before`: the
    step ends at X - 1 and a one-tick step takes X; `through`: one step of b + 64 ticks runs through
    X.  `ticks`: one-tick steps from pod X - 3 through X."""
    _, x, m = CLUSTERS[cluster]
    if how == "ticks":
        steps = [x - 3, 1, 1, 1, 1]
    elif p < b:
        assert how == "step"
        steps = [x - p, b]
    elif how == "ends_before":
        steps = [x - b, b, 1]
    else:
        assert how == "through" and p == b
        steps = [x - b, b + KC]
    steps.append(m + 20 - sum(steps))
    assert min(steps) > 0
    return tuple(steps)


def plans_at(cluster, b, p):
    """The plans that put X at position p: one, or the two of p == b."""
    return [plan(cluster, b, p)] if p < b else [plan(cluster, b, p, "ends_before"), plan(cluster, b, p, "through")]


# ---- the oracle's runs, once each -------------------------------------------------------------------
def _oracle(tr, mode):
    ora = make_oracle(tr, mode)
    if tr["nodes"]["n"] > 10_000:
        ora.set_threads(ec.threads())
    ora.submit(tr)
    return ora


@functools.lru_cache(maxsize=None)
def marks(cluster):
    """Every tick at which some plan of the cluster ends a step (every batch size, every position; the
    pipelined cluster has one plan), and tick X."""
    out = {CLUSTERS[cluster][1]}
    if cluster == "pipe":
        return tuple(sorted(out | set(np.cumsum(plan(cluster, B_CHUNK, KC)).tolist())))
    for b in (B_SMALL, B_CHUNK, B_ONE_POD):
        for p in positions(b) + tuple(edge_p(sat) for sat in SATS):
            if p <= b:
                for steps in plans_at(cluster, b, p):
                    out.update(np.cumsum(steps).tolist())
    out.update(np.cumsum(plan(cluster, B_CHUNK, 0, "ticks")).tolist())
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def record(name, sat, cluster):
    """The oracle's one run of a case, the same for every plan (it walks tick by tick: where a step
    ends changes nothing), stepped from mark to mark.  dict(binds (the whole run's), rc, tick (where
    it stopped, or its last), usage {mark: (nodes, rows)} — the rows of usage() that are not zero, at
    every mark reached and at the stop —, feasible (the mask of ko_eval for X at tick X, None if the
    run never got there)).  Nothing in it is changed afterwards."""
    c = case(name, sat, cluster)
    ora = _oracle(c["tr"], c["mode"])
    parts, usage, feas, rc, tick = [], {}, None, 0, 0

    def snap():
        u = ora.usage()
        nz = np.flatnonzero(u.any(axis=1))
        usage[int(ora.tick)] = (nz, u[nz].copy())
    for mark in marks(cluster):
        b, rc = ora.step(mark - tick, cap=mark - tick)
        parts.append(b)
        tick = int(ora.tick)
        snap()
        if rc:
            break
        if mark == c["x"]:
            feas = ora.eval(c["x"])[0].copy()
    ora.close()
    binds = {f: np.concatenate([q[f] for q in parts]) for f in ("pod", "node", "tick", "status")}
    return dict(binds=binds, rc=rc, tick=tick, usage=usage, feasible=feas)


def reference(name, sat, cluster, steps):
    """The oracle's run of a case cut along a plan (a tuple of step lengths, ending on marks).  Per
    step until the run stops or the plan ends: dict(k, binds, rc, usage, tick, queued)."""
    c = case(name, sat, cluster)
    rec = record(name, sat, cluster)
    bt = rec["binds"]["tick"]
    out, lo = [], 0
    for k in steps:
        hi = lo + k
        stops = rec["rc"] != 0 and rec["tick"] <= hi
        tick = rec["tick"] if stops else hi
        sel = slice(int(np.searchsorted(bt, lo, side="right")), int(np.searchsorted(bt, tick, side="right")))
        nz, rows = rec["usage"][tick]
        usage = np.zeros((c["n"], 3), np.int64)
        usage[nz] = rows
        popped = sel.stop + (1 if stops else 0)
        out.append(dict(k=k, binds={f: v[sel] for f, v in rec["binds"].items()}, rc=rec["rc"] if stops else 0,
                        usage=usage, tick=tick, queued=c["m"] - popped))
        if stops:
            break
        lo = hi
    return tuple(out)


def direct_reference(name, sat, cluster, steps):
    """reference() by an oracle run of its own that takes the plan's steps as they are (what
    tests/test_stop_cases.py holds the cut record against)."""
    c = case(name, sat, cluster)
    ora = _oracle(c["tr"], c["mode"])
    out, popped = [], 0
    for k in steps:
        b, rc = ora.step(k, cap=k)
        popped += len(b["pod"]) + (rc != 0)
        out.append(dict(k=k, binds=b, rc=rc, usage=ora.usage().copy(), tick=int(ora.tick), queued=c["m"] - popped))
        if rc:
            break
    ora.close()
    return tuple(out)


def all_binds(name, sat, cluster):
    rec = record(name, sat, cluster)
    return rec["binds"], rec["rc"]


def probe(name, sat, cluster):
    """(the code of a stop before X's tick or 0, the feasible mask of X at tick X — one tick before its own)."""
    rec = record(name, sat, cluster)
    return (0, rec["feasible"]) if rec["feasible"] is not None else (rec["rc"], None)


def carried(name, sat, cluster):
    """Live expiries attached to X: those of the pods bound Ok that finish in (X's predecessor's bind
    tick, X's bind tick] (expiry_burst_cases.attached, with X entered as a bind at its tick whether
    or not the run bound it)."""
    c = case(name, sat, cluster)
    b, _ = all_binds(name, sat, cluster)
    x = c["x"]
    keep = b["pod"] < x
    assert keep.sum() == x, "the run stopped before X"
    rows = {f: np.concatenate([b[f][keep], [v]]) for f, v in (("pod", x), ("tick", x + 1), ("status", 0))}
    live, _ = ec.attached(rows, c["run"])
    return int(live[x])


@functools.lru_cache(maxsize=None)
def short_reference(steps):
    """group_cases' `short` member (the other member of the small-class group) over a plan: per step
    (binds, usage); its run has no stop."""
    import group_cases as gc
    tr, _ = gc.trace_of("short")
    ora = make_oracle(tr, gc.MEMBERS["short"]["mode"])
    ora.submit(tr)
    out = []
    for k in steps:
        b, rc = ora.step(k, cap=k)
        assert rc == 0
        out.append((b, ora.usage().copy()))
    ora.close()
    return tuple(out)


# ---- the state after a stop, from oracle/pysim.py's rules ---------------------------------------------
SERIES_TICKS = 64
REQ_TICKS = 5


@functools.lru_cache(maxsize=None)
def _pysim_nodes(n):
    """A PySim that holds the nodes of the cluster of n nodes (of its g6 trace) and no pod; its node
    lists are never written."""
    return PySim(_base("g6", next(k for k, v in CLUSTERS.items() if v[0] == n))[0])


def _pysim(c):
    """A fresh PySim for a case: the cluster's taint and label lists shared (every saturation has the
    same), the capacities with the case's gpus, its own pods, pod maps and mode."""
    ps = copy.copy(_pysim_nodes(c["n"]))
    gpu = c["tr"]["nodes"]["alloc"][:, tracegen.GPU]
    ps.cap = [dict(cap, **{RES[2]: int(g)}) for cap, g in zip(ps.cap, gpu)]
    ps.filter_mode, ps.filters, scorers = MODES[c["mode"]]
    ps.scorers = list(scorers)
    ps.pods, ps.node_pods = [], [dict() for _ in range(ps.n)]
    ps.tick, ps.qhead, ps.err = 0, 0, None
    ps.submit(c["tr"])
    return ps


@functools.lru_cache(maxsize=None)
def stopped_model(name, sat, cluster):
    """The scheduler state around the stop of a stopping case, by the rules of oracle/pysim.py: a
    PySim that holds the trace, with the oracle's binds entered tick by tick as PySim.step stores
    them (node, status, t0, the node's pod map) and the stop pod popped.  PySim's own scheduling loop
    walks every node per scorer in Python — minutes at 3,000 nodes — so the binds are the C oracle's;
    the state is PySim's: _total_request and _running_num per node for the last REQ_TICKS ticks,
    _running per stored pod and the pods' request lists for the series, _total_seconds.
    Returns dict(tick, req {t: [n][4]}, series [SERIES_TICKS][7] for the ticks up to the stop tick,
    series_lo, status {pod: (phase, node, start_tick, total_seconds)} for the pods around the stop pod
    and X)."""
    c = case(name, sat, cluster)
    b, rc = all_binds(name, sat, cluster)
    code, stop_pod = c["stop"]
    assert rc == code
    ps = _pysim(c)
    total = {}                           # (PySim sums a pod's phases at every call: once per pod here)

    def total_seconds(q):
        if q["key"] not in total:
            total[q["key"]] = PySim._total_seconds(ps, q)
        return total[q["key"]]
    ps._total_seconds = total_seconds
    rows = list(zip(b["pod"].tolist(), b["node"].tolist(), b["tick"].tolist(), b["status"].tolist()))
    entered, held = 0, set()

    def enter(t):
        """The binds made up to tick t, as PySim.step stores them (a tick's state holds no later bind)."""
        nonlocal entered
        while entered < len(rows) and rows[entered][2] <= t:
            pod, node, tick, status = rows[entered]
            ps.pods[pod].update(node=node, status="Ok" if status == 0 else "OverCapacity", t0=tick)
            ps.node_pods[node][ps.pods[pod]["key"]] = pod
            held.add(node)
            entered += 1
        ps.tick = t

    def matrix(t):
        out = np.zeros((ps.n, 4), np.int64)
        for nd in held:
            tot = ps._total_request(nd, t)
            out[nd, :3] = [tot.get(r, 0) for r in RES]
            out[nd, 3] = ps._running_num(nd, t)
        return out
    now = stop_pod + 1                   # bulk arrivals: the stop pod's tick
    lo = now - SERIES_TICKS + 1
    series = np.zeros((SERIES_TICKS, 7), np.int64)
    arrival = np.maximum(np.asarray(c["tr"]["pods"]["arrival"], np.int64), 1)
    req = {}
    for i, t in enumerate(range(lo, now + 1)):
        enter(t)
        stored = [ps.pods[j] for nd in held for j in ps.node_pods[nd].values()]
        live = [q for q in stored if ps._running(q, t)]
        series[i, 0] = len(live)
        series[i, 1:4] = [sum(q["req"].get(r, 0) for q in live) for r in RES]
        series[i, 4] = sum(1 for q in stored if q["status"] == "Ok")
        series[i, 5] = sum(1 for q in stored if q["status"] == "OverCapacity")
        popped = min(t, stop_pod + 1)    # one pod a tick; the stop pod is popped at its tick
        series[i, 6] = np.searchsorted(arrival, t, side="right") - popped
        if t > now - REQ_TICKS:
            req[t] = matrix(t)
    assert entered == len(rows) and ps.tick == now
    assert len({q["key"] for q in ps.pods}) == len(ps.pods)   # (no key stored twice: `stored` is every bind)
    ps.qhead, ps.err = stop_pod + 1, "stopped"

    def status(pod):
        q = ps.pods[pod]
        if q["status"] is None:
            phase = 0                    # KS_PHASE_PENDING: never bound
        elif q["status"] != "Ok":
            phase = 3                    # KS_PHASE_FAILED
        else:
            phase = 1 if ps._running(q, now) else 2
        return (phase, -1 if q["node"] is None else q["node"], -1 if q["t0"] is None else q["t0"],
                ps._total_seconds(q))
    pods = sorted({stop_pod - 1, stop_pod, stop_pod + 1, c["x"] - 1, c["x"], c["x"] + 1})
    return dict(tick=now, req=req, series=series, series_lo=lo, status={q: status(q) for q in pods})
