"""Exact references for the drain preview (include/ks_engine.h: ks_drain_at).

* ``pysim_drain``: a deep copy of oracle/pysim.py's PySim stepped to tick t.  The drained nodes leave
  its node set (the loops of ``_score_map`` restated over the nodes that remain, with PySim's own
  string predicates and Fractions), their running pods are collected in pod order, taken off their
  nodes and asked pod after pod: the lowest-index maximum, PySim's own ``_fits``; an Ok pod joins its
  new node under a fresh key and runs at t.
* ``fast_drain``: the same walk in plain integers on the encoded arrays — one score vector per pod at
  its turn, computed for all remaining nodes at once (LeastRequested in int64, BalancedAllocation in
  Python integers of any size), written from the header's semantics and place_ref's formulas.
  ``score_vector`` is checked against place_ref's scalar ``_total1`` by tests/test_drain_ref.py.

Both return ``dict(pod, from_node, node, status, score, candidates, after, info, reused)``: arrays over
the evicted pods, ``after`` [n][4] int64, ``info`` = [None, Ok, OverCapacity, not found, None, drained
nodes that had no running pod], ``reused`` = the pods whose winner an earlier evicted pod had changed.
"""
import copy

import numpy as np

from place_ref import NOT_FOUND, OK, OVER, _fits, _total1   # noqa: F401  (re-exported for the tests)
from pysim import RES

FIELDS = ("pod", "from_node", "node", "status", "score", "candidates")


def _result(n, pods, frm, n_drain):
    k = len(pods)
    return dict(pod=np.array(pods, np.int64).reshape(k), from_node=np.array(frm, np.int32).reshape(k),
                node=np.full(k, -1, np.int32), status=np.full(k, NOT_FOUND, np.int32), score=np.full(k, -1, np.int64),
                candidates=np.zeros(k, np.int64), after=np.zeros((n, 4), np.int64),
                info=[None, 0, 0, 0, None, n_drain - len(set(frm))], reused=[])


# ---- PySim ---------------------------------------------------------------------------------------
def _score_map_live(ps, live, pod, t):
    """PySim._score_map over the nodes that remain in k.nodes (kubesim/kubesim.go:168-206)."""
    nodes = list(live)
    for bit, fn in ((1, lambda n: ps._fits(n, pod, t)), (2, lambda n: ps._taint_ok(n, pod)),
                    (4, lambda n: ps._selector_ok(n, pod))):
        if ps.filters & bit:
            nodes = [n for n in nodes if fn(n)]
    if ps.filter_mode == 0:
        nodes = list(live)
    scores = {}
    for kind, weight, value in ps.scorers:
        for n in nodes:
            sc = value if kind == 0 else (ps._lr(n, pod, t) if kind == 1 else ps._ba(n, pod, t))
            scores[n] = scores.get(n, 0) + sc * weight
    return scores


def pysim_drain(ps, t, drained):
    """``ps``: a PySim stepped to tick t (or stopped before it); it is not changed."""
    assert ps.tick == t or ps.err is not None
    ps = copy.deepcopy(ps)
    drained = sorted(set(int(d) for d in drained))
    dset = set(drained)
    live = [n for n in range(ps.n) if n not in dset]
    ev = [j for j, pod in enumerate(ps.pods)
          if pod["node"] in dset and ps.node_pods[pod["node"]].get(pod["key"]) == j and ps._running(pod, t)]
    frm = [ps.pods[j]["node"] for j in ev]
    for d in drained:
        ps.node_pods[d] = {}
    r = _result(ps.n, ev, frm, len(drained))
    changed = set()
    for i, j in enumerate(ev):
        old = ps.pods[j]
        pod = dict(req=dict(old["req"]), tols=old["tols"], sel=old["sel"], arrival=t, flags=0,
                   spec=[(ps.tick_s * 1000, {})], key=("evicted", j), node=None, status=None, t0=None)
        scores = _score_map_live(ps, live, pod, t)
        r["candidates"][i] = len(scores)
        best, bn = -1, None
        for n in sorted(scores):
            if scores[n] > best:
                best, bn = scores[n], n
        if bn is None:
            r["info"][3] += 1
            continue
        ok = ps._fits(bn, pod, t)
        r["node"][i], r["score"][i], r["status"][i] = bn, best, OK if ok else OVER
        r["info"][1 if ok else 2] += 1
        if bn in changed:
            r["reused"].append(i)
        if ok:
            pod.update(node=bn, status="Ok", t0=t)
            ps.pods.append(pod)
            ps.node_pods[bn][pod["key"]] = len(ps.pods) - 1
            assert ps._running(pod, t)
            changed.add(bn)
    for n in range(ps.n):
        tot = ps._total_request(n, t)
        r["after"][n, :3] = [tot.get(x, 0) for x in RES]
        r["after"][n, 3] = ps._running_num(n, t)
    return r


_sims = {}


def sim_at(case, t):
    """place_ref.parity_case's PySim in the state its own run had after tick t, rebuilt from the
    binds made by then (a PySim's whole state is its pods' node / status / start tick and the nodes'
    stores; tests/test_drain_ref.py checks it against the stepped run).  Built once; not to be changed."""
    if (case, t) in _sims:
        return _sims[case, t]
    import place_ref as pr
    from harness import MODES
    from pysim import PySim
    r = pr.parity_case(case)
    fm, fl, sc = MODES[r["mode"]]
    ps = PySim(r["tr"], filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(r["tr"])
    for pod, node, tick, status in r["binds"].tolist():
        if tick > t:
            break
        ps.pods[pod].update(node=node, status="Ok" if status == 0 else "OverCapacity", t0=tick)
        ps.node_pods[node][ps.pods[pod]["key"]] = pod
        ps.qhead = pod + 1
    ps.tick = t
    _sims[case, t] = ps
    return ps


def sim_state(ps, t):
    """[n][4] requested milli-units and running pods of a PySim at tick t"""
    state = np.zeros((ps.n, 4), np.int64)
    for n in range(ps.n):
        tot = ps._total_request(n, t)
        state[n, :3] = [tot.get(x, 0) for x in RES]
        state[n, 3] = ps._running_num(n, t)
    return state


# ---- plain integers on the encoded arrays --------------------------------------------------------
def score_vector(cfg, A, S, taint, label, live, shape):
    """aggregated score + 1 per node for one shape (int64 [n]); 0: no entry in the score map (also
    every node outside ``live``).  A, S: int64 [n][4]; quantities below 2^56 (asserted by the caller)."""
    req, km, tol, sel = shape
    n = len(A)
    if not cfg["scorers"]:
        return np.zeros(n, np.int64)
    ok = live.copy()
    if cfg["filter_mode"] == 1:
        fl = cfg["filters"]
        if fl & 1:
            fit = ~(S[:, 3] >= np.maximum(A[:, 3], 0))
            for c in range(3):
                if (km >> c) & 1:
                    fit &= (A[:, c] >= 0) & (S[:, c] + req[c] <= A[:, c])
            ok &= fit
        if fl & 2:
            ok &= (taint & ~np.uint64(tol)) == 0
        if fl & 4:
            ok &= (label & np.uint64(sel)) == np.uint64(sel)
    idx = np.nonzero(ok)[0]
    tot = np.zeros(len(idx), np.int64)
    a, s = A[idx], S[idx]
    for kind, weight, value in cfg["scorers"]:
        if kind == 0:
            tot += weight * value
        elif kind == 1:
            lr = np.zeros(len(idx), np.int64)
            for c in (0, 1):
                Ac, u = np.maximum(a[:, c], 0), s[:, c] + req[c]
                good = (Ac > 0) & (u <= Ac)
                lr += np.where(good, (Ac - u) * 10 // np.maximum(Ac, 1), 0)
            tot += weight * (lr // 2)
        else:
            ac, am = np.maximum(a[:, 0], 0).astype(object), np.maximum(a[:, 1], 0).astype(object)
            uc, um = (s[:, 0] + req[0]).astype(object), (s[:, 1] + req[1]).astype(object)
            good = (a[:, 0] > 0) & (a[:, 1] > 0) & (s[:, 0] + req[0] < a[:, 0]) & (s[:, 1] + req[1] < a[:, 1])
            D = ac * am
            D1 = np.where(good, D, 1)
            ba = 10 * (D1 - abs(uc * am - um * ac)) // D1    # Python integers: exact at any size
            tot += weight * np.where(good, ba, 0).astype(np.int64)
    out = np.zeros(n, np.int64)
    out[idx] = tot + 1
    return out


def running_on(tr, enc, binds, t, drained):
    """The pods of a run's binds (dict of arrays pod, node, tick, status) that run at tick t on a node
    of ``drained``, in pod order, with their nodes (place_ref.state_from_binds' rule)."""
    p = tr["pods"]
    sec = np.add.reduceat(np.asarray(p["phase_sec"], np.int64), np.asarray(p["phase_off"][:-1], np.int64))
    assert (np.asarray(p["phase_sec"]) > 0).all() and sec.max() < 2**31
    dur = (sec + tr["tick_seconds"] - 1) // tr["tick_seconds"]
    pod, node, tick, status = (np.asarray(binds[f], np.int64) for f in ("pod", "node", "tick", "status"))
    assert (np.diff(pod) > 0).all()
    mask = np.zeros(len(enc["alloc"]), bool)
    mask[np.asarray(list(drained), np.int64)] = True
    sel = (status == 0) & (tick <= t) & (t < tick + dur[pod]) & mask[np.clip(node, 0, None)]
    return pod[sel].tolist(), node[sel].tolist()


def fast_drain(alloc, state, cfg, pods, evicted, from_node, drained):
    """alloc [n][4] (encoded milli-units, -1 absent), state [n][4] at t; cfg: place_ref.engine_cfg;
    pods: the encoded pods (req, keymask, tol, sel); evicted / from_node: the pods running at t on the
    ``drained`` nodes, in pod order."""
    n = len(alloc)
    A = np.array(alloc, np.int64).reshape(n, 4)
    S = np.array(state, np.int64).reshape(n, 4).copy()
    assert A.max(initial=0) < 2**56 and S.max(initial=0) < 2**56
    drained = sorted(set(int(d) for d in drained))
    live = np.ones(n, bool)
    live[drained] = False
    S[drained] = 0
    taint, label = np.asarray(cfg["taint"], np.uint64), np.asarray(cfg["label"], np.uint64)
    r = _result(n, evicted, from_node, len(drained))
    changed = set()
    for i, j in enumerate(evicted):
        km = int(pods["keymask"][j])
        req = [int(pods["req"][j][c]) if (km >> c) & 1 else 0 for c in range(3)]
        shape = (req, km, int(pods["tol"][j]), int(pods["sel"][j]))
        v = score_vector(cfg, A, S, taint, label, live, shape)
        r["candidates"][i] = int((v > 0).sum())
        if n == 0 or v.max() == 0:
            r["info"][3] += 1
            continue
        bn = int(v.argmax())            # argmax: the first (lowest-index) maximum
        ok = _fits(A[bn].tolist(), S[bn].tolist(), req, km)
        r["node"][i], r["score"][i], r["status"][i] = bn, int(v[bn]) - 1, OK if ok else OVER
        r["info"][1 if ok else 2] += 1
        if bn in changed:
            r["reused"].append(i)
        if ok:
            S[bn, :3] += req
            S[bn, 3] += 1
            changed.add(bn)
    r["after"] = S
    return r


def assert_same(got, want, what=""):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"{what}: after")
    assert [int(x) for x in got["info"][1:4]] == [int(x) for x in want["info"][1:4]], what
    assert int(got["info"][5]) == int(want["info"][5]), what
