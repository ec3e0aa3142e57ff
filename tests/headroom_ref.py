"""Exact references for the headroom tests (include/ks_engine.h: ks_headroom_at, ks_headroom_series).

* ``count_exact``: the count and the limiting key of one node for one shape in Python integers,
  written from the header's closed form — not from ks_device.h;
* ``step_model``: oracle/pysim.py's PySim stepped tick by tick, keeping the [n][4] requested matrix
  after every tick's bind (Node.totalResourceRequest / runningPodsNum, kubesim/node/node.go:97-118);
* ``reference``: per tick, shape and node the counts and columns from those matrices, the trace's
  alloc and PySim's own taint / selector predicates on the shapes' string form.

A shape here is a pair: the encoded record (req[3], keymask, tol, sel — what the engine takes) and
the PySim pod dict (req, tols, sel as strings — what the checker takes).  Shapes taken from the
trace's pods carry both by construction; hand-made ones are written in both forms.
"""
import numpy as np

from pysim import PySim, RES

NODE_MAX = (1 << 31) - 1
CPU, MEM, GPU, PODS = 0, 1, 2, 3


def count_exact(alloc, run, req, keymask):
    """(count, limiting key).  alloc[4] (cpu memory gpu pods; -1 absent), run[4] (requested cpu memory
    gpu, running pods), req[3], all in the same units, Python integers."""
    bounds = []
    for k in range(3):
        if not (keymask >> k) & 1:
            continue
        A, r, q = int(alloc[k]), int(run[k]), int(req[k])
        if A < 0:
            bounds.append((0, k))          # the node lacks the key: also for a request of 0
        elif q == 0:
            continue                       # no bound
        else:
            bounds.append((min(max(A - r, 0) // q, NODE_MAX), k))
    bounds.append((min(max(int(alloc[3]) - int(run[3]), 0), NODE_MAX), PODS))
    c = min(b for b, _ in bounds)
    return c, next(k for b, k in bounds if b == c)


def step_model(tr, mode_tuple, ticks):
    """PySim over ``ticks`` ticks: dict(ps, req [ticks' + 1][n][4] int64 (row t = after tick t's bind,
    row 0 zeros), binds rows (pod, node, tick, status), err, tick)."""
    fm, fl, sc = mode_tuple
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    req = [np.zeros((ps.n, 4), np.int64)]
    binds, err = [], None
    for t in range(1, ticks + 1):
        b, err = ps.step(1)
        binds += b
        m = np.zeros((ps.n, 4), np.int64)
        for n in range(ps.n):
            tot = ps._total_request(n, t)
            m[n, :3] = [tot.get(r, 0) for r in RES]
            m[n, 3] = ps._running_num(n, t)
        req.append(m)
        if err:
            break
    return dict(ps=ps, req=np.stack(req), binds=np.array(binds, np.int64).reshape(-1, 4), err=err, tick=ps.tick,
                filter_mode=fm, filters=fl)


def eligibility(model, sim_pods):
    """[k][n] bool: the engine's eligibility rule on PySim's own predicates."""
    ps, fm, fl = model["ps"], model["filter_mode"], model["filters"]
    out = np.ones((len(sim_pods), ps.n), bool)
    if fm != 1:
        return out
    for j, pod in enumerate(sim_pods):
        for n in range(ps.n):
            ok = True
            if fl & 2:
                ok &= ps._taint_ok(n, pod)
            if fl & 4:
                ok &= ps._selector_ok(n, pod)
            out[j, n] = ok
    return out


def reference(alloc, req_t, shapes, elig):
    """alloc [n][4] (encoded: -1 absent); req_t [nt][n][4]; shapes: dict of arrays req [k][3], keymask
    [k]; elig [k][n].  Returns (cols [nt][k][9] int64, counts [nt][k][n] int64).  A node's count for a
    shape depends on its own (alloc, state) row only, so rows are memoised."""
    nt, n = req_t.shape[0], req_t.shape[1]
    k = len(shapes["keymask"])
    cols = np.zeros((nt, k, 9), np.int64)
    counts = np.zeros((nt, k, n), np.int64)
    a_rows = [[int(x) for x in alloc[i]] for i in range(n)]
    s_rows = [([int(x) for x in shapes["req"][j]], int(shapes["keymask"][j])) for j in range(k)]
    elig = np.asarray(elig, bool)
    cur_c = np.zeros((k, n), np.int64)
    cur_k = np.zeros((k, n), np.int64)
    for t in range(nt):
        # a node's counts change only when its state row does: the counts themselves are Python
        # integers (count_exact), only their bookkeeping is numpy int64 (sums of <= n * 2^31)
        changed = range(n) if t == 0 else np.nonzero((req_t[t] != req_t[t - 1]).any(axis=1))[0]
        for i in changed:
            r = [int(x) for x in req_t[t, i]]
            for j in range(k):
                c, key = count_exact(a_rows[i], r, *s_rows[j])
                cur_c[j, i] = c if elig[j, i] else 0
                cur_k[j, i] = key if elig[j, i] else 4
        counts[t] = cur_c
        cols[t, :, 0] = cur_c.sum(axis=1)
        cols[t, :, 1] = (cur_c >= 1).sum(axis=1)
        if n:
            cols[t, :, 2] = cur_c.max(axis=1)
            cols[t, :, 3] = np.where(cols[t, :, 2] > 0, cur_c.argmax(axis=1), -1)   # argmax: the first maximum
        else:
            cols[t, :, 3] = -1
        for key in range(5):
            cols[t, :, 4 + key] = (cur_k == key).sum(axis=1)
    return cols, counts


def shared_trace(mult, irregular=False, seed=31, n_nodes=32, n_pods=800):
    """The state-query tests' trace recipe (tests/test_state_queries_gpu.py _shared_trace): a stream of
    pods without nodeSelectors, phase lengths 1..97 s times ``mult``; ``irregular`` adds a negative
    phase and one that wraps the int32 sum (kubesim/pod/pod.go:148-162)."""
    from harness import small_trace
    tr = small_trace(seed, n_nodes=n_nodes, n_pods=n_pods, arrival="stream", selectors=False)
    p = tr["pods"]
    F = len(p["phase_sec"])
    p["phase_sec"][:] = (1 + (np.arange(F) * 7919) % 97) * mult
    if irregular:
        off = p["phase_off"]
        multi = np.nonzero(np.diff(off) >= 2)[0]
        p["phase_sec"][off[multi[3]]] = -25
        p["phase_sec"][off[multi[7]]] = 2**31 - 40
        p["phase_sec"][off[multi[7]] + 1] = 100
    return tr


def run_ticks(model):
    """Per Ok bind of the model (node, start tick, end tick): the pod runs on ticks [start, end),
    end = start + ceil(total seconds / tick) (Pod.IsRunning, kubesim/pod/pod.go:67-69)."""
    ps = model["ps"]
    out = []
    for pod, node, tick, status in model["binds"].tolist():
        if status != 0:
            continue
        S = ps._total_seconds(ps.pods[pod])
        d = (S + ps.tick_s - 1) // ps.tick_s if S > 0 else 0
        if d > 0:
            out.append((node, tick, tick + d))
    return out


TOLERATE_ALL = [dict(key="", op="Exists", value="", effect="")]   # toleration.go:37-56: matches every taint
ALL_BITS = np.uint64(0xFFFFFFFFFFFFFFFF)
SEL_IMPOSSIBLE = np.uint64(1) << np.uint64(63)


def make_shapes(tr, enc, model, pod_ids, hand):
    """Shapes from the trace's own pods ``pod_ids`` plus the hand-made ones: ``hand`` rows are
    (req[3], keymask, tolerate_all, impossible_selector).  Returns (encoded dict, PySim pod dicts)."""
    p = enc["pods"]
    req = [p["req"][j].tolist() for j in pod_ids]
    km = [int(p["keymask"][j]) for j in pod_ids]
    tol = [np.uint64(p["tol"][j]) for j in pod_ids]
    sel = [np.uint64(p["sel"][j]) for j in pod_ids]
    sim = [model["ps"].pods[j] for j in pod_ids]
    for r, m, tol_all, imposs in hand:
        req.append(list(r))
        km.append(m)
        tol.append(ALL_BITS if tol_all else np.uint64(0))
        sel.append(SEL_IMPOSSIBLE if imposs else np.uint64(0))
        sim.append(dict(tols=TOLERATE_ALL if tol_all else [],
                        sel={"no-such-label-key": "no-such-value"} if imposs else {}))
    shapes = dict(req=np.array(req, np.int64).reshape(-1, 3), keymask=np.array(km, np.uint8),
                  tol=np.array(tol, np.uint64), sel=np.array(sel, np.uint64))
    return shapes, sim
