"""Exact references for the gang admission preview (include/ks_engine.h: ks_gang_at).

* ``fast_gang``: the chain as the header writes it, on ``place_ref.fast_place``: for every gang a copy
  of the state, the attempt, and the copy adopted or discarded.  ``fast_place`` runs every pod of the
  gang; a pod not bound Ok changes nothing, so its rows up to the deciding pod are the attempt's, and
  an admitted gang (no early end) leaves ``fast_place``'s own ``after``.
* ``pysim_gang``: a deep copy of oracle/pysim.py's PySim asked pod after pod (``place_ref.pysim_place``'s
  step), the appended pods and the nodes' stores restored on a block.

Both return ``dict(first, size, outcome, tried, ok, over_capacity, not_found, block_status, rows, after,
info)``: arrays over the gangs, ``rows`` a dict of arrays over the k pods (an untried pod is
{-1, NOT_TRIED, -1, 0}), ``after`` [n][4] int64, ``info`` = [None, admitted, blocked, skipped, tried
gangs of more than ROUND pods, Ok pods of admitted gangs] (the rounds are the device algorithm's own).
"""
import copy

import numpy as np

import place_ref as pr
from pysim import RES

BLOCKED, ADMITTED, SKIPPED = 0, 1, 2
NOT_TRIED = -2
ROUND = 32           # KS_PLACE_L: a gang with more pods heads no round
SUMMARY = ("first", "size", "outcome", "tried", "ok", "over_capacity", "not_found", "block_status")
SIZES = [1, 2, 4, 8, 3, 16, 5, 33, 1, 6, 12, 2, 40, 7]


def _blank(k):
    return dict(node=np.full(k, -1, np.int32), status=np.full(k, NOT_TRIED, np.int32), score=np.full(k, -1, np.int64),
                candidates=np.zeros(k, np.int64))


def _gangs(first, min_ok):
    first = [int(x) for x in first]
    m = len(first) - 1
    size = [first[g + 1] - first[g] for g in range(m)]
    assert first[0] == 0 and min(size) >= 0
    mo = size if min_ok is None else [int(x) for x in min_ok]
    assert all(0 <= mo[g] <= size[g] for g in range(m))
    return first, size, mo


def _verdict(status, size, mo):
    """(outcome, tried, block_status) of an attempt whose pods would have these statuses in order"""
    bad = 0
    for i, st in enumerate(status):
        bad += st != pr.OK
        if bad > size - mo:
            return BLOCKED, i + 1, int(st)
    return ADMITTED, size, 0


def _assemble(first, size, summ, rows, after):
    res = {f: np.array([s[i] for s in summ], np.int32) for i, f in enumerate(SUMMARY[2:])}
    res["first"], res["size"] = np.array(first[:-1], np.int32), np.array(size, np.int32)
    oc = res["outcome"]
    res["rows"], res["after"] = rows, after
    res["info"] = [None, int((oc == ADMITTED).sum()), int((oc == BLOCKED).sum()), int((oc == SKIPPED).sum()),
                   int(((res["size"] > ROUND) & (oc != SKIPPED)).sum()), int(res["ok"][oc == ADMITTED].sum())]
    return res


def fast_gang(alloc, state, cfg, shapes, shape_of, first, min_ok=None, strict=False):
    """alloc, state, cfg, shapes, shape_of as for ``place_ref.fast_place``; first [m + 1]; min_ok [m] or None"""
    first, size, mo = _gangs(first, min_ok)
    k = len(shape_of)
    assert first[-1] == k
    S = np.array(state, np.int64).reshape(len(alloc), 4).copy()
    rows, summ, over = _blank(k), [], False
    for g in range(len(size)):
        lo, hi = first[g], first[g + 1]
        if over:
            summ.append((SKIPPED, 0, 0, 0, 0, 0))
            continue
        if size[g] == 0:
            summ.append((ADMITTED, 0, 0, 0, 0, 0))
            continue
        r = pr.fast_place(alloc, S, cfg, shapes, shape_of[lo:hi])      # (on copies: S is not changed)
        outcome, tried, bs = _verdict(r["status"].tolist(), size[g], mo[g])
        st = r["status"][:tried]
        for f in pr.FIELDS:
            rows[f][lo:lo + tried] = r[f][:tried]
        summ.append((outcome, tried, int((st == pr.OK).sum()), int((st == pr.OVER).sum()), int((st == pr.NOT_FOUND).sum()), bs))
        if outcome == ADMITTED:
            S = r["after"]
        over = strict and outcome == BLOCKED
    return _assemble(first, size, summ, rows, S)


def pysim_gang(ps, t, pods, first, min_ok=None, strict=False):
    """``ps``: a PySim stepped to tick t (or stopped before it); it is not changed.  ``pods``: the k
    preview pods in order (``place_ref.sim_pods`` dicts)."""
    assert ps.tick == t or ps.err is not None
    ps = copy.deepcopy(ps)
    first, size, mo = _gangs(first, min_ok)
    k = len(pods)
    assert first[-1] == k
    rows, summ, over = _blank(k), [], False
    for g in range(len(size)):
        if over:
            summ.append((SKIPPED, 0, 0, 0, 0, 0))
            continue
        saved = (len(ps.pods), [dict(d) for d in ps.node_pods])   # all an attempt changes: appended pods, the stores
        cnt, bad, outcome, bs, tried = {pr.OK: 0, pr.OVER: 0, pr.NOT_FOUND: 0}, 0, ADMITTED, 0, size[g]
        for i in range(first[g], first[g + 1]):
            shape = pods[i]
            pod = dict(req=dict(shape["req"]), tols=shape["tols"], sel=shape["sel"], arrival=t, flags=0,
                       spec=[(ps.tick_s * 1000, {})], key=("gang", i), node=None, status=None, t0=None)
            scores = ps._score_map(pod, t)
            best, bn = -1, None
            for n in sorted(scores):
                if scores[n] > best:
                    best, bn = scores[n], n
            if bn is None:
                st = pr.NOT_FOUND
                rows["node"][i], rows["status"][i], rows["score"][i], rows["candidates"][i] = -1, st, -1, len(scores)
            else:
                st = pr.OK if ps._fits(bn, pod, t) else pr.OVER
                rows["node"][i], rows["status"][i], rows["score"][i], rows["candidates"][i] = bn, st, best, len(scores)
            cnt[st] += 1
            if st == pr.OK:
                pod.update(node=bn, status="Ok", t0=t)
                ps.pods.append(pod)
                ps.node_pods[bn][pod["key"]] = len(ps.pods) - 1
            else:
                bad += 1
                if bad > size[g] - mo[g]:
                    outcome, bs, tried = BLOCKED, st, i - first[g] + 1
                    break
        summ.append((outcome, tried, cnt[pr.OK], cnt[pr.OVER], cnt[pr.NOT_FOUND], bs))
        if outcome == BLOCKED:
            del ps.pods[saved[0]:]
            ps.node_pods = saved[1]
            over = strict
    after = np.zeros((ps.n, 4), np.int64)
    for x in range(ps.n):
        tot = ps._total_request(x, t)
        after[x, :3] = [tot.get(c, 0) for c in RES]
        after[x, 3] = ps._running_num(x, t)
    return _assemble(first, size, summ, rows, after)


def assert_same(got, want, what="", rows=True, after=True):
    """got: Engine.gang_at's dict, or a reference's"""
    for f in SUMMARY:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    if rows:
        for f in pr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f], want["rows"][f], err_msg=f"{what}: rows {f}")
    if after:
        np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"{what}: after")
    assert [int(x) for x in got["info"][1:6]] == [int(x) for x in want["info"][1:6]], (what, got["info"], want["info"])


# ---- queues of gangs from a trace's own pods -----------------------------------------------------
def queue_from_trace(enc, n_gangs, sizes=SIZES, stride=37, inner=13):
    """Gang g has sizes[g % len(sizes)] pods; its pod i has the shape of trace pod (stride g + (inner i if
    g % 3 else 0)) mod the trace's pods: the encoded req, keymask, tol, sel.  Shapes are numbered in
    order of first appearance.  Returns (shapes dict, shape_of [k], first [n_gangs + 1], the trace pod
    each shape was taken from)."""
    e = enc["pods"]
    n_pods = len(e["keymask"])
    seen, ids, shape_of, first = {}, [], [], [0]
    for g in range(n_gangs):
        for i in range(sizes[g % len(sizes)]):
            j = (stride * g + (inner * i if g % 3 else 0)) % n_pods
            key = (tuple(int(x) for x in e["req"][j]), int(e["keymask"][j]), int(e["tol"][j]), int(e["sel"][j]))
            if key not in seen:
                seen[key] = len(ids)
                ids.append(j)
            shape_of.append(seen[key])
        first.append(len(shape_of))
    shapes = dict(req=np.ascontiguousarray(e["req"][ids], np.int64), keymask=np.ascontiguousarray(e["keymask"][ids], np.uint8),
                  tol=np.ascontiguousarray(e["tol"][ids], np.uint64), sel=np.ascontiguousarray(e["sel"][ids], np.uint64))
    return shapes, np.array(shape_of, np.int32), np.array(first, np.int32), ids


def three_quarters(first):
    """min_ok = max(1, ceil(3 size / 4)) per gang (0 for an empty one)"""
    size = np.diff(np.asarray(first, np.int64))
    return np.where(size > 0, np.maximum(1, (3 * size + 3) // 4), 0).astype(np.int32)


# ---- the shared 32-node parity trace (place_ref.parity_case) -------------------------------------
PARITY_SIZES = [1, 2, 4, 0, 8, 3, 5, 1, 6, 12, 2, 4]        # 48 pods: place_ref.N_PODS
PARITY_FIRST = np.concatenate([[0], np.cumsum(PARITY_SIZES)]).astype(np.int32)
PARITY_MIN_OK = np.array([1, 1, 3, 0, 5, 3, 0, 1, 4, 9, 2, 2], np.int32)
_queues = {}


def parity_queue(case):
    """place_ref.parity_case(case) with its 48 preview pods as PySim pod dicts: (the case, the pods)"""
    if case not in _queues:
        import drain_ref as dr
        import headroom_ref as hr
        r = pr.parity_case(case)
        shapes, sim = hr.make_shapes(r["tr"], r["enc"], dict(ps=dr.sim_at(case, pr.T)), list(pr.TRACE_PODS), pr.HAND)
        for f in shapes:
            np.testing.assert_array_equal(shapes[f], r["shapes"][f])
        pods = pr.sim_pods(shapes, sim)
        _queues[case] = (r, [pods[j] for j in r["shape_of"]])
    return _queues[case]
