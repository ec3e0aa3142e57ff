"""Traces for the chunk resolver's replay paths (ks_chunk.hip replay(): batch-wide bind rows, the
cache phase's single replay per bound node).  Shared by tests/test_chunk_replay_gpu.py (the engine
against the oracle) and tests/test_chunk_replay_shapes.py (the oracle alone: the shapes really
produce the events the GPU tests rely on).

Every pod arrives at tick 1 and one pod binds per tick, so a pod that runs d ticks expires d pods
after its bind: inside its own batch, and for d up to 12 often across a 64-pod chunk boundary."""
import numpy as np

from harness import small_trace

TICK = 10


def set_run_ticks(tr, ticks):
    """Give pod i a total run time of exactly ticks[i] ticks (its first phase takes the remainder)."""
    p = tr["pods"]
    off = p["phase_off"]
    nph = np.diff(off)
    p["phase_sec"][:] = 1
    p["phase_sec"][off[:-1]] = TICK * np.asarray(ticks, dtype=np.int64) - (nph - 1)
    return tr


def dense_trace():
    """test_dense_expiries' trace (tests/test_resolvers_gpu.py) at 300 nodes and 1,500 pods, run
    lengths 1-12 ticks."""
    tr = small_trace(11, n_nodes=300, n_pods=1500, taints=False, selectors=False, tolerations=False)
    return set_run_ticks(tr, 1 + np.arange(1500) % 12)


# (nodes, mode): few nodes, 600 pods, runs of 1-12 ticks.  The fit-only mode with the
# least-requested scorer spreads the binds (every node rebound every few dozen pods: final binds of
# earlier chunks under the later chunks' rows); the mode without the fit filter and with the balanced
# scorer piles them on a few nodes (rows past kSeg state changes, nodes past kPend pending own
# expiries, admission failures).
FEW_NODES = {
    "spread24": (24, "feeds_fit_lr"),
    "pile40": (40, "feeds_taint_sel_ba_const"),
    "pile32_literal": (32, "literal_lrba_filters_ignored"),
}


def few_nodes_trace(name):
    n, mode = FEW_NODES[name]
    tr = small_trace(5, n_nodes=n, n_pods=600, taints=False, selectors=False, tolerations=False)
    return set_run_ticks(tr, 1 + (np.arange(600) * 7) % 12), mode


def tight_trace():
    """test_list_exhaustion's set-up (tests/test_resolvers_gpu.py): equal requests, four pods per
    node — with the filters ignored the binds keep landing on full nodes and are refused."""
    tr = small_trace(21, n_nodes=300, n_pods=900, taints=False, labels=False, tolerations=False,
                     selectors=False)
    nd, p = tr["nodes"], tr["pods"]
    p["req"][:] = p["req"][0]
    nd["alloc"][:, :3] = 4 * p["req"][0]
    nd["alloc"][:, 3] = 110
    nd["alloc_has"][:] = 15
    return tr


def run_ticks(tr):
    p = tr["pods"]
    tot = np.add.reduceat(p["phase_sec"].astype(np.int64), p["phase_off"][:-1])
    return -(-tot // TICK)


def replay_events(binds, ticks, batch=256, chunk=64):
    """From a run's binds (one per tick, in order) and the pods' run lengths: per batch of `batch`
    consecutive binds, what the resolver's replays meet.  Returns the maxima over the batches of
    (binds on one node, own expiries pending at once on one node, state changes of one node inside
    one chunk) and the counts of (binds on a node bound in an earlier chunk of the batch, own expiries
    effective in a later chunk than their bind, refused binds on a node bound earlier in the batch)."""
    node, ok, pod = binds["node"], binds["status"] == 0, binds["pod"]
    d = ticks[pod]
    mx_binds = mx_pend = mx_seg = 0
    n_rebind = n_cross = n_refused = 0
    for b0 in range(0, len(node), batch):
        seen = {}
        for i in range(b0, min(b0 + batch, len(node))):
            n = int(node[i])
            if n < 0:
                continue
            ev = seen.setdefault(n, [])
            c = (i - b0) // chunk
            if ev:
                n_rebind += any((j - b0) // chunk < c for j, _ in ev)
                n_refused += not ok[i]
            if ok[i]:
                ev.append((i, i + int(d[i])))
                n_cross += (i + int(d[i]) - b0) // chunk > c and i + int(d[i]) < b0 + batch
            mx_binds = max(mx_binds, len(ev))
            mx_pend = max(mx_pend, sum(1 for j, e in ev if e > i))
        for ev in seen.values():
            for c0 in range(b0, b0 + batch, chunk):
                ch = sum(c0 <= j < c0 + chunk for j, _ in ev) + sum(c0 <= e < c0 + chunk for _, e in ev)
                mx_seg = max(mx_seg, ch)
    return dict(binds=mx_binds, pending=mx_pend, seg=mx_seg, rebind=n_rebind, cross=n_cross, refused=n_refused)
