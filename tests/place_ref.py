"""Exact references for the placement preview (include/ks_engine.h: ks_place_at).

* ``pysim_place``: oracle/pysim.py's PySim, stepped to tick t by the caller, asked pod after pod —
  its own ``_score_map`` (string predicates, Fractions), the lowest-index maximum, its own ``_fits``;
  an Ok pod joins the node under a fresh key and runs at t.  It mutates the PySim it is given: hand
  it a copy (``copy.deepcopy``).
* ``fast_place``: the same walk in plain Python integers on the encoded arrays, written from the
  header's semantics and pysim.py's LeastRequested / BalancedAllocation formulas — not from
  ks_query.h.  It keeps one score vector per shape and re-evaluates only the node a placement
  changed, so 1,024 pods on 600 nodes take seconds.

Both return ``dict(node, status, score, candidates, after, info, reused)``: arrays over the pods,
``after`` [n][4] int64, ``info`` = [None, placed Ok, placed OverCapacity, not found] (the rounds are
the device algorithm's own), ``reused`` = the pods whose winner an earlier preview pod had changed.
"""
import numpy as np

from pysim import RES

OK, OVER, NOT_FOUND = 0, 1, -1


def sim_pods(shapes, sim):
    """PySim pod dicts of the encoded shapes: the masked requests by resource name, and the string
    tolerations / selector of ``sim`` (headroom_ref.make_shapes' second value)."""
    out = []
    for j in range(len(shapes["keymask"])):
        km = int(shapes["keymask"][j])
        req = {RES[c]: int(shapes["req"][j][c]) for c in range(3) if (km >> c) & 1}
        out.append(dict(req=req, tols=sim[j]["tols"], sel=sim[j]["sel"]))
    return out


def _result(n, k):
    return dict(node=np.full(k, -1, np.int32), status=np.full(k, NOT_FOUND, np.int32), score=np.full(k, -1, np.int64),
                candidates=np.zeros(k, np.int64), after=np.zeros((n, 4), np.int64), info=[None, 0, 0, 0], reused=[])


def pysim_place(ps, t, pods):
    """``pods``: the preview pods in order (dicts with req, tols, sel).  ``ps`` is changed."""
    assert ps.tick == t or ps.err is not None
    k = len(pods)
    r = _result(ps.n, k)
    changed = set()
    for i, shape in enumerate(pods):
        pod = dict(req=dict(shape["req"]), tols=shape["tols"], sel=shape["sel"], arrival=t, flags=0,
                   spec=[(ps.tick_s * 1000, {})], key=("preview", i), node=None, status=None, t0=None)
        scores = ps._score_map(pod, t)
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


# ---- plain integers on the encoded arrays ------------------------------------------------------
def _fits(a, s, req, km):
    for c in range(3):
        if (km >> c) & 1 and (a[c] < 0 or s[c] + req[c] > a[c]):
            return False
    return not (s[3] >= max(a[3], 0))


def _lr(a, s, req):
    tot = 0
    for c in (0, 1):
        A, u = max(a[c], 0), s[c] + req[c]
        if A <= 0 or u > A:
            continue
        tot += (A - u) * 10 // A
    return tot // 2


def _ba(a, s, req):
    ac, am = max(a[0], 0), max(a[1], 0)
    uc, um = s[0] + req[0], s[1] + req[1]
    if ac <= 0 or am <= 0 or uc >= ac or um >= am:
        return 0
    D = ac * am
    return 10 * (D - abs(uc * am - um * ac)) // D   # floor(10 (1 - |uc/ac - um/am|))


def _total1(cfg, a, s, taint, label, shape):
    """aggregated score + 1 of one node for one shape, 0 when it has no entry in the score map"""
    req, km, tol, sel = shape
    if not cfg["scorers"]:
        return 0
    if cfg["filter_mode"] == 1:
        fl = cfg["filters"]
        if fl & 1 and not _fits(a, s, req, km):
            return 0
        if fl & 2 and taint & ~tol & 0xFFFFFFFFFFFFFFFF:
            return 0
        if fl & 4 and (label & sel) != sel:
            return 0
    tot = 0
    for kind, weight, value in cfg["scorers"]:
        tot += weight * (value if kind == 0 else (_lr(a, s, req) if kind == 1 else _ba(a, s, req)))
    return tot + 1


def fast_place(alloc, state, cfg, shapes, shape_of=None):
    """alloc [n][4] (encoded milli-units, -1 absent), state [n][4] (requested milli-units, running
    pods) at t; cfg: dict(filter_mode, filters, scorers, taint [n], label [n]); shapes: dict of arrays
    req [m][3], keymask, tol, sel; shape_of [k] or None (one pod per shape)."""
    n, m = len(alloc), len(shapes["keymask"])
    shape_of = list(range(m)) if shape_of is None else [int(x) for x in shape_of]
    k = len(shape_of)
    A = [[int(x) for x in row] for row in alloc]
    S = [[int(x) for x in row] for row in state]
    taint = [int(x) for x in cfg["taint"]]
    label = [int(x) for x in cfg["label"]]
    sh = []
    for j in range(m):
        km = int(shapes["keymask"][j])
        req = [int(shapes["req"][j][c]) if (km >> c) & 1 else 0 for c in range(3)]   # unmasked keys are ignored
        sh.append((req, km, int(shapes["tol"][j]), int(shapes["sel"][j])))
    used = sorted(set(shape_of))
    vec = {j: np.array([_total1(cfg, A[i], S[i], taint[i], label[i], sh[j]) for i in range(n)], np.int64) for j in used}
    r = _result(n, k)
    changed = set()
    for i, j in enumerate(shape_of):
        v = vec[j]
        r["candidates"][i] = int((v > 0).sum()) if n else 0
        if n == 0 or v.max() == 0:
            r["info"][3] += 1
            continue
        bn = int(v.argmax())            # argmax: the first (lowest-index) maximum
        ok = _fits(A[bn], S[bn], sh[j][0], sh[j][1])
        r["node"][i], r["score"][i], r["status"][i] = bn, int(v[bn]) - 1, OK if ok else OVER
        r["info"][1 if ok else 2] += 1
        if bn in changed:
            r["reused"].append(i)
        if ok:
            for c in range(3):
                S[bn][c] += sh[j][0][c]
            S[bn][3] += 1
            changed.add(bn)
            for jj in used:
                vec[jj][bn] = _total1(cfg, A[bn], S[bn], taint[bn], label[bn], sh[jj])
    r["after"] = np.array(S, np.int64).reshape(n, 4)
    return r


FIELDS = ("node", "status", "score", "candidates")


def assert_same(got, want, what=""):
    for f in FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"{what}: after")
    assert [int(x) for x in got["info"][1:4]] == [int(x) for x in want["info"][1:4]], what


# ---- the shared parity cases (tests/test_place_ref.py on the CPU, tests/test_place_gpu.py) -------
T = 800
TICKS = (0, 1, 137, 400, 799, 800)
FEEDS, LITERAL = "feeds_all_lrba", "literal_lrba_filters_ignored"
CASES = {"feeds": (FEEDS, 1, False), "literal": (LITERAL, 1, False), "feeds_irregular": (FEEDS, 1, True)}
MEM_ODD = 3_000_000_000_001   # a memory request that is no multiple of the engine's memory unit (asserted)
# hand-made shapes (headroom_ref.make_shapes rows): req, keymask, tolerates every taint, impossible selector
HAND = [
    ([1000, (1 << 30) * 1000, 0], 3, False, False),     # tolerates nothing
    ([1000, (1 << 30) * 1000, 0], 3, True, True),       # a selector no node carries
    ([-1, MEM_ODD, -1], 2, True, False),                # memory only, coprime to the unit; junk in unmasked keys
    ([8000, (64 << 30) * 1000, 4000], 7, True, False),  # 8 cpu / 64 Gi / 4 gpu
    ([100, 268_435_456_000, 0], 3, True, False),        # small
]
TRACE_PODS = (0, 33, 66, 99, 132, 165, 198)             # seven of the trace's own pods
N_PODS = 48


def engine_cfg(mode_tuple, enc):
    fm, fl, sc = mode_tuple
    return dict(filter_mode=fm, filters=fl, scorers=sc, taint=enc["taint"], label=enc["label"])


_cases = {}


def parity_case(case):
    """The shared 32-node, 800-pod trace of ``case`` stepped tick by tick on PySim; at every tick of
    TICKS both references for 48 preview pods over 12 shapes (seven trace pods' and HAND), the shapes
    interleaved.  Built once per process; nothing in it is changed afterwards."""
    if case in _cases:
        return _cases[case]
    import copy
    from math import gcd

    import headroom_ref as hr
    from harness import MODES, encoded
    from pysim import PySim
    mode, mult, irregular = CASES[case]
    tr = hr.shared_trace(mult, irregular)
    enc = encoded(tr)
    fm, fl, sc = MODES[mode]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    binds, snaps = [], {}
    for t in range(T + 1):
        if t:
            b, err = ps.step(1)
            assert err is None
            binds += b
        if t in TICKS:
            snaps[t] = copy.deepcopy(ps)
    shapes, sim = hr.make_shapes(tr, enc, dict(ps=ps), list(TRACE_PODS), HAND)
    assert len(shapes["keymask"]) == 12
    unit = 0
    for v in list(enc["alloc"][:, 1]) + list(enc["pods"]["req"][:, 1]):
        unit = gcd(unit, int(v)) if v > 0 else unit
    assert unit > 1 and gcd(MEM_ODD, unit) == 1, "the odd memory request is not coprime to the engine's unit"
    shape_of = np.array([(5 * i) % 12 for i in range(N_PODS)], np.int32)
    pods = sim_pods(shapes, sim)
    cfg = engine_cfg(MODES[mode], enc)
    # the trace's own shapes alone: every request is a whole multiple of the engine's unit (the gcd of
    # all it was given), so ks_place_at runs in device units; with MEM_ODD among the shapes it cannot
    whole = {f: np.ascontiguousarray(v[:len(TRACE_PODS)]) for f, v in shapes.items()}
    whole_of = np.array([(3 * i) % len(TRACE_PODS) for i in range(N_PODS)], np.int32)
    for c in range(3):
        u = 0
        for v in list(enc["alloc"][:, c]) + list(enc["pods"]["req"][:, c]):
            u = gcd(u, int(v)) if v > 0 else u
        assert all(int(q) % max(u, 1) == 0 for q in whole["req"][:, c])
    slow, fast, fast_whole = {}, {}, {}
    for t in TICKS:
        state = np.zeros((ps.n, 4), np.int64)
        for n in range(ps.n):
            tot = snaps[t]._total_request(n, t)
            state[n, :3] = [tot.get(x, 0) for x in RES]
            state[n, 3] = snaps[t]._running_num(n, t)
        fast[t] = fast_place(enc["alloc"], state, cfg, shapes, shape_of)
        fast_whole[t] = fast_place(enc["alloc"], state, cfg, whole, whole_of)
        slow[t] = pysim_place(snaps[t], t, [pods[j] for j in shape_of])
    _cases[case] = dict(tr=tr, enc=enc, mode=mode, shapes=shapes, shape_of=shape_of, slow=slow, fast=fast,
                        whole=whole, whole_of=whole_of, fast_whole=fast_whole,
                        binds=np.array(binds, np.int64).reshape(-1, 4))
    return _cases[case]


def assert_not_vacuous(case, refs):
    """On the reference alone: the comparison cannot pass by every pod doing the same thing."""
    st = np.concatenate([r["status"] for r in refs.values()])
    if CASES[case][0] == FEEDS:
        assert any(((r["status"][:-1] == NOT_FOUND) & (r["status"][1:] != NOT_FOUND)).any() for r in refs.values()), \
            "no NOT_FOUND pod followed by a placed one"
    else:
        assert (st == OVER).sum() >= 5, "fewer than five OverCapacity placements"
        assert all((r["candidates"] == len(r["after"])).all() for r in refs.values())
    nodes = np.concatenate([r["node"] for r in refs.values()])
    assert len(set(nodes[nodes >= 0].tolist())) >= 8, "fewer than eight distinct nodes used"
    assert any(len(r["reused"]) >= 1 for r in refs.values()), "no winner on a node an earlier preview pod changed"
    if CASES[case][0] == FEEDS:
        assert any(len(set(r["candidates"].tolist())) >= 3 for r in refs.values()), "candidates barely vary"


def state_from_binds(tr, enc, binds, t):
    """[n][4] requested milli-units and running pods at tick t from a run's binds (dict of arrays pod,
    node, tick, status) for a trace whose phase seconds are positive and do not wrap: a pod bound Ok at
    tick b runs on ticks [b, b + ceil(total seconds / tick)) (Pod.IsRunning, kubesim/pod/pod.go:67-69)."""
    p = tr["pods"]
    sec = np.add.reduceat(np.asarray(p["phase_sec"], np.int64), np.asarray(p["phase_off"][:-1], np.int64))
    assert (np.asarray(p["phase_sec"]) > 0).all() and sec.max() < 2**31
    dur = (sec + tr["tick_seconds"] - 1) // tr["tick_seconds"]
    state = np.zeros((len(enc["alloc"]), 4), np.int64)
    for pod, node, tick, status in zip(binds["pod"].tolist(), binds["node"].tolist(), binds["tick"].tolist(),
                                       binds["status"].tolist()):
        if status == 0 and tick <= t < tick + dur[pod]:
            state[node, :3] += enc["pods"]["req"][pod]
            state[node, 3] += 1
    return state
