"""Exact references for the consolidation preview (include/ks_engine.h: ks_consolidate_at).

The candidates are handled in the caller's order on one private state, with a set R of removed nodes
and a set V of destinations.  A candidate in V is a destination and nothing is tried; any other
candidate leaves the node set together with R and its running pods are asked pod after pod until one
is not bound Ok; all Ok (or no pod): the candidate is removed, its placements stay and their nodes join
V; otherwise everything is put back.

* ``fast_consolidate``: the chain in plain integers on ``drain_ref.score_vector``, ``_fits`` and
  ``running_on`` — what the GPU tests use on the larger clusters;
* ``pysim_consolidate``: the same chain on a deep copy of oracle/pysim.py's PySim: nodes leave its
  node set, the copy is restored on a block (its pod list and its nodes' stores are all an attempt
  changes), a node that received an evicted pod is a destination.

Both return ``dict(node, evicted, outcome, n_rows, block_status, first_row, rows, after, info)``:
arrays over the candidates in the caller's order, ``rows`` = drain_ref's FIELDS over the rows written
(a removed candidate's pods, a blocked one's up to and including the blocking pod), ``after`` [n][4],
``info`` = [None, removed, blocked, destinations, candidates of the single path (SINGLE pods or more
and no destination), pods moved].  ``fast_consolidate`` adds ``on_rolled_back``: the kept placements on
a node that an earlier, rolled-back attempt had placed a pod on.
"""
import copy

import numpy as np

import drain_ref as dr
import place_ref as pr
from pysim import RES

BLOCKED, REMOVED, DESTINATION = 0, 1, 2
SINGLE = 32          # KS_PLACE_L: a candidate with that many pods heads no round
SUMMARY = ("node", "evicted", "outcome", "n_rows", "block_status", "first_row")


def _assemble(nodes, evicted, outcome, block_status, per_rows, after, extra=None):
    m = len(nodes)
    n_rows = np.array([len(r) for r in per_rows], np.int32).reshape(m)
    out = dict(node=np.array(nodes, np.int32).reshape(m), evicted=np.array(evicted, np.int32).reshape(m),
               outcome=np.array(outcome, np.int32).reshape(m), n_rows=n_rows,
               block_status=np.array(block_status, np.int32).reshape(m))
    out["first_row"] = np.concatenate([[0], np.cumsum(n_rows)[:-1]]).astype(np.int64) if m else np.zeros(0, np.int64)
    flat = [r for rows in per_rows for r in rows]
    out["rows"] = {f: np.array([r[i] for r in flat], np.int32 if f in ("from_node", "node", "status") else np.int64)
                   for i, f in enumerate(dr.FIELDS)}
    out["after"] = after
    oc = out["outcome"]
    out["info"] = [None, int((oc == REMOVED).sum()), int((oc == BLOCKED).sum()), int((oc == DESTINATION).sum()),
                   int(((out["evicted"] >= SINGLE) & (oc != DESTINATION)).sum()), int(n_rows[oc == REMOVED].sum())]
    out.update(extra or {})
    return out


def fast_consolidate(tr, enc, binds, cfg, t, nodes, state=None, running=None):
    """binds: dict of arrays pod, node, tick, status (a run's binds); cfg: place_ref.engine_cfg;
    running: per candidate its running pods (default: ``drain_ref.running_on``)"""
    if state is None:
        state = pr.state_from_binds(tr, enc, binds, t)
    n = len(enc["alloc"])
    A = np.array(enc["alloc"], np.int64).reshape(n, 4)
    S = np.array(state, np.int64).reshape(n, 4).copy()
    assert A.max(initial=0) < 2**56 and S.max(initial=0) < 2**56
    taint, label = np.asarray(cfg["taint"], np.uint64), np.asarray(cfg["label"], np.uint64)
    pods = enc["pods"]
    live = np.ones(n, bool)
    V, touched = set(), set()
    evicted, outcome, block_status, per_rows = [], [], [], []
    on_rolled_back = 0
    for c in nodes:
        c = int(c)
        ev = running[c] if running is not None else dr.running_on(tr, enc, binds, t, [c])[0]
        evicted.append(len(ev))
        if c in V:
            outcome.append(DESTINATION), block_status.append(0), per_rows.append([])
            continue
        saved = S.copy()
        live[c] = False
        S[c] = 0
        rows, got, status = [], [], pr.OK
        for j in ev:
            km = int(pods["keymask"][j])
            req = [int(pods["req"][j][k]) if (km >> k) & 1 else 0 for k in range(3)]
            v = dr.score_vector(cfg, A, S, taint, label, live, (req, km, int(pods["tol"][j]), int(pods["sel"][j])))
            cand = int((v > 0).sum())
            if v.max() == 0:
                status = pr.NOT_FOUND
                rows.append((j, c, -1, status, -1, cand))
                break
            bn = int(v.argmax())            # argmax: the first (lowest-index) maximum
            status = pr.OK if dr._fits(A[bn].tolist(), S[bn].tolist(), req, km) else pr.OVER
            rows.append((j, c, bn, status, int(v[bn]) - 1, cand))
            if status != pr.OK:
                break
            S[bn, :3] += req
            S[bn, 3] += 1
            got.append(bn)
        per_rows.append(rows)
        if status == pr.OK:
            outcome.append(REMOVED), block_status.append(0)
            on_rolled_back += sum(b in touched for b in got)
            V.update(got)
        else:
            outcome.append(BLOCKED), block_status.append(status)
            touched.update(got)
            S = saved
            live[c] = True
    return _assemble(list(nodes), evicted, outcome, block_status, per_rows, S, dict(on_rolled_back=on_rolled_back, state=state))


def pysim_consolidate(ps, t, nodes):
    """``ps``: a PySim stepped to tick t (or stopped before it); it is not changed."""
    assert ps.tick == t or ps.err is not None
    base = ps
    ps = copy.deepcopy(base)
    R, V = set(), set()
    evicted, outcome, block_status, per_rows = [], [], [], []
    for c in nodes:
        c = int(c)
        # the pods running on c at t: the run's own (a pod moved here makes c a destination)
        ev = [j for j, pod in enumerate(base.pods)
              if pod["node"] == c and base.node_pods[c].get(pod["key"]) == j and base._running(pod, t)]
        evicted.append(len(ev))
        if c in V:
            outcome.append(DESTINATION), block_status.append(0), per_rows.append([])
            continue
        saved = (len(ps.pods), [dict(d) for d in ps.node_pods])   # all an attempt changes: appended pods, the stores
        live = [x for x in range(ps.n) if x not in R and x != c]
        ps.node_pods[c] = {}
        rows, got, status = [], [], pr.OK
        for j in ev:
            old = ps.pods[j]
            pod = dict(req=dict(old["req"]), tols=old["tols"], sel=old["sel"], arrival=t, flags=0,
                       spec=[(ps.tick_s * 1000, {})], key=("evicted", j), node=None, status=None, t0=None)
            scores = dr._score_map_live(ps, live, pod, t)
            best, bn = -1, None
            for x in sorted(scores):
                if scores[x] > best:
                    best, bn = scores[x], x
            if bn is None:
                status = pr.NOT_FOUND
                rows.append((j, c, -1, status, -1, len(scores)))
                break
            status = pr.OK if ps._fits(bn, pod, t) else pr.OVER
            rows.append((j, c, bn, status, best, len(scores)))
            if status != pr.OK:
                break
            pod.update(node=bn, status="Ok", t0=t)
            ps.pods.append(pod)
            ps.node_pods[bn][pod["key"]] = len(ps.pods) - 1
            got.append(bn)
        per_rows.append(rows)
        if status == pr.OK:
            outcome.append(REMOVED), block_status.append(0)
            R.add(c)
            V.update(got)
        else:
            outcome.append(BLOCKED), block_status.append(status)
            del ps.pods[saved[0]:]
            ps.node_pods = saved[1]
    after = np.zeros((ps.n, 4), np.int64)
    for x in range(ps.n):
        tot = ps._total_request(x, t)
        after[x, :3] = [tot.get(k, 0) for k in RES]
        after[x, 3] = ps._running_num(x, t)
    return _assemble(list(nodes), evicted, outcome, block_status, per_rows, after)


def assert_same(got, want, what="", rows=True, after=True):
    """got: Engine.consolidate_at's dict, or a reference's"""
    for f in SUMMARY:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    if rows:
        for f in dr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f], want["rows"][f], err_msg=f"{what}: rows {f}")
    if after:
        np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"{what}: after")
    assert [int(x) for x in got["info"][1:6]] == [int(x) for x in want["info"][1:6]], (what, got["info"], want["info"])
