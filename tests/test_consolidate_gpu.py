"""GPU parity of the consolidation preview (include/ks_engine.h: ks_consolidate_at) against
tests/consolidate_ref.py: the integer chain ``fast_consolidate`` on the C oracle's binds, and PySim with
nodes leaving its node set and the copy restored on a block on the shared 32-node trace (the two are
equal: tests/test_consolidate_ref.py).  Everything is exact integer equality.

Each reference is built once, checked on its own for the properties that keep the comparison from
passing vacuously before any engine call, and never changed afterwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import consolidate_ref as cr
import drain_ref as dr
import place_ref as pr
from harness import MODES, assert_same_binds, encoded, make_engine, make_oracle, shard_ranks, small_trace, step_ranks

pytestmark = pytest.mark.gpu

FEEDS, LITERAL = pr.FEEDS, pr.LITERAL
OK, OVER, NOT_FOUND = pr.OK, pr.OVER, pr.NOT_FOUND
FIVE = [(500, 1024), (1000, 2048), (2000, 1024), (1500, 4096), (4000, 8192)]   # milli-cpu, Mi
MI = (1 << 20) * 1000                                                           # a Mi in milli-bytes


@functools.lru_cache(maxsize=None)
def _model(seed, n_nodes, n_pods, mode, kind="plain"):
    """test_removable_gpu._model's recipe: the trace, its encoding and the C oracle's binds over n_pods
    ticks.  kind "five": five shapes in all; "tiny": requests so small that nodes fill up to their
    pods capacity."""
    tr = small_trace(seed, n_nodes=n_nodes, n_pods=n_pods, arrival="stream", selectors=False, tolerations=kind != "five")
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 99991
    for j in range(n_pods):
        if kind == "five":
            cpu, mi = FIVE[j % 5]
            p["req"][j] = (cpu, mi * MI, 0)
        elif kind == "tiny":
            p["req"][j] = (10 + j % 7, (16 + j % 5) * MI, 0)
    enc = encoded(tr)
    ora = make_oracle(tr, mode)
    ora.submit(tr)
    ob, rc = ora.step(n_pods, cap=n_pods)
    assert rc == 0, "the oracle's run stopped"
    return dict(tr=tr, enc=enc, ob=ob, mode=mode, cfg=pr.engine_cfg(MODES[mode], enc), T=n_pods)


@functools.lru_cache(maxsize=None)
def _ref(seed, n_nodes, n_pods, mode, t, kind="plain", nodes=None):
    """nodes: None (every node ascending), "desc", or a tuple"""
    m = _model(seed, n_nodes, n_pods, mode, kind)
    order = list(range(n_nodes)) if nodes is None else list(range(n_nodes - 1, -1, -1)) if nodes == "desc" else list(nodes)
    return cr.fast_consolidate(m["tr"], m["enc"], m["ob"], m["cfg"], t, order)


def _shape_count(m, pods):
    e = m["enc"]["pods"]
    return len({(tuple(int(x) for x in e["req"][j]), int(e["keymask"][j]), int(e["tol"][j]), int(e["sel"][j])) for j in pods})


def _engine(m, **kw):
    eng = make_engine(m["tr"], m["enc"], m["mode"], batch_pods=64, **kw)
    eng.submit(m["enc"]["pods"])
    eb = eng.step(m["T"])
    assert_same_binds(eb, m["ob"])
    return eng


def _check(eng, t, ref, what="", rows=True):
    got = eng.consolidate_at(t, ref["node"], rows=rows, after=True)
    cr.assert_same(got, ref, what or f"tick {t}", rows=rows)
    assert got["evicted_total"] == int(ref["evicted"].sum())
    return got


CASE1 = (7, 360, 1200, FEEDS)


@pytest.fixture(scope="module")
def eng360():
    eng = _engine(_model(*CASE1))
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------
# 1. 360 nodes / 1,200 pods, every node a candidate in ascending order, every row a shape of its own
# ---------------------------------------------------------------------------------------------
def test_every_node_ascending(eng360):
    m, ref = _model(*CASE1), _ref(*CASE1, 1200)
    oc, ev = ref["outcome"], ref["evicted"]
    # (the reference alone gives: 122 removed, 19 of them empty, 27 blocked, 18 of them after at
    # least one Ok pod, 211 destinations, 23 kept placements on a node a rolled-back attempt had
    # touched, 403 rows of 403 shapes)
    assert (oc == cr.REMOVED).sum() >= 100 and (oc == cr.BLOCKED).sum() >= 20
    assert ((oc == cr.BLOCKED) & (ref["n_rows"] >= 2)).sum() >= 10, "few attempts are rolled back after an Ok pod"
    assert (oc == cr.DESTINATION).sum() >= 150 and ref["on_rolled_back"] >= 15
    assert _shape_count(m, ref["rows"]["pod"].tolist()) >= 6 * 64
    assert ev.max() < cr.SINGLE and ref["info"][4] == 0
    got = _check(eng360, 1200, ref)
    assert got["info"][0] >= 7, got["info"]


# ---------------------------------------------------------------------------------------------
# 2. the same engine: a past tick, other orders, summaries only, a short buffer, prefixes
# ---------------------------------------------------------------------------------------------
def test_a_past_tick_other_orders_and_buffers(eng360):
    from kubesim_amd import _lib
    from kubesim_amd.engine import CONSOLIDATION_DTYPE, EVICTION_DTYPE
    m = _model(*CASE1)
    ref = _ref(*CASE1, 700)
    ob = m["ob"]
    later = set(ob["pod"][ob["tick"] > 700].tolist())
    assert ref["evicted"].sum() >= 300 and len(later) >= 200 and not later & set(ref["rows"]["pod"].tolist())
    assert ref["info"][1] >= 50 and ref["info"][3] >= 50
    got = _check(eng360, 700, ref)
    assert not later & set(got["rows"]["pod"].tolist())
    np.testing.assert_array_equal(eng360.requested_at(700).sum(axis=0), got["after"].sum(axis=0))
    # descending: another chain on the same state
    desc = _ref(*CASE1, 1200, "plain", "desc")
    asc = _ref(*CASE1, 1200)
    assert desc["info"][1] >= 50 and (desc["outcome"][::-1] != asc["outcome"]).sum() >= 50
    gd = _check(eng360, 1200, desc, "descending")
    np.testing.assert_array_equal(eng360.requested_at(1200).sum(axis=0), gd["after"].sum(axis=0))
    # a permuted subset, the bitmap's word edges and the scan's block edge among it
    rng = np.random.default_rng(360)
    sub = [0, 31, 32, 255, 256, 359] + [int(x) for x in rng.permutation(np.arange(33, 255))[:90]]
    sub = tuple(sub[i] for i in rng.permutation(len(sub)))
    assert list(sub) != sorted(sub)
    want = _ref(*CASE1, 700, "plain", sub)
    assert want["info"][1] >= 20 and want["info"][3] >= 5 and len(want["rows"]["pod"]) >= 30
    part = _check(eng360, 700, want, "permuted subset")
    # summaries only are the summaries with rows
    plain = _check(eng360, 700, want, "summaries only", rows=False)
    assert plain["rows"] is None
    np.testing.assert_array_equal(plain["info"], part["info"])
    # too little room: KS_ERANGE, the count, nothing else written
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nodes = np.arange(360, dtype=np.int32)
    total = int(ref["evicted"].sum())
    out = np.full(360 * CONSOLIDATION_DTYPE.itemsize, 0x5A, np.uint8)
    rows = np.full(100 * EVICTION_DTYPE.itemsize + 64, 0x5A, np.uint8)
    aft = np.full(360 * 4, 0x5A5A, np.int64)
    info = np.full(_lib.KS_CONSOLIDATE_INFO, 0x5A5A, np.int64)
    n_ev, n_rows = C.c_int64(-1), C.c_int64(-77)
    rc = eng360._L.ks_consolidate_at(eng360.h, 700, 360, p(nodes), p(out), p(rows), 100, C.byref(n_ev), C.byref(n_rows),
                                     p(aft), p(info))
    assert rc == _lib.KS_ERANGE and n_ev.value == total and total > 100 and n_rows.value == -77
    assert (out == 0x5A).all() and (rows == 0x5A).all() and (info == 0x5A5A).all() and (aft == 0x5A5A).all()


def test_prefix_and_first_candidate(eng360):
    ref = _ref(*CASE1, 1200)
    head = _ref(*CASE1, 1200, "plain", tuple(range(50)))
    for f in cr.SUMMARY:
        np.testing.assert_array_equal(ref[f][:50], head[f])
    assert head["info"][1] >= 10 and head["info"][3] >= 5 and head["info"][2] >= 1
    _check(eng360, 1200, head, "the first 50")
    # the first candidate of a call is its drain, truncated after the first pod not bound Ok
    busy = [int(c) for c in np.nonzero(ref["evicted"] >= 2)[0][:6]]
    blocked_alone = 0
    for c in busy + [int(c) for c in np.nonzero((ref["outcome"] == cr.BLOCKED))[0][:4]]:
        got = eng360.consolidate_at(1200, [c], after=True)
        one = eng360.drain_at(1200, [c], after=True)
        bad = np.nonzero(one["status"] != OK)[0]
        keep = len(one["pod"]) if len(bad) == 0 else int(bad[0]) + 1
        assert got["outcome"][0] == (cr.REMOVED if len(bad) == 0 else cr.BLOCKED) and got["n_rows"][0] == keep
        for f in dr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f], one[f][:keep], err_msg=f"node {c}: {f}")
        if len(bad) == 0:
            np.testing.assert_array_equal(got["after"], one["after"])
        else:
            blocked_alone += 1
            np.testing.assert_array_equal(got["after"], eng360.requested_at(1200))
    assert len(busy) == 6


# ---------------------------------------------------------------------------------------------
# 3. five shapes: one segment holds hundreds of pods, the lists are used up inside the round
# ---------------------------------------------------------------------------------------------
def test_five_shapes_lists_used_up_inside_a_round():
    case = (5, 400, 1200, FEEDS)
    m, ref = _model(*case, "five"), _ref(*case, 1200, "five")
    # (the reference alone gives: 205 removed, 195 destinations, 447 pods of five shapes)
    assert _shape_count(m, ref["rows"]["pod"].tolist()) == 5 and ref["evicted"].max() < cr.SINGLE
    assert ref["info"][1] >= 150 and ref["info"][3] >= 150
    eng = _engine(m)
    got = _check(eng, 1200, ref)
    assert got["info"][0] >= 2, "five shapes fit one segment: only a stop inside a candidate makes a second round"
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. many pods per node: candidates of the single path, removed and blocked
# ---------------------------------------------------------------------------------------------
def test_many_pods_per_node_take_the_single_path():
    case = (11, 40, 1200, FEEDS)
    m, ref = _model(*case, "tiny"), _ref(*case, 1200, "tiny", "desc")
    big = ref["evicted"] >= cr.SINGLE
    # (the reference alone gives, descending at t = 1200: see the assertion's message)
    seen = (int(big.sum()), int((big & (ref["outcome"] == cr.REMOVED)).sum()), int((big & (ref["outcome"] == cr.BLOCKED)).sum()))
    assert seen[0] >= 5 and seen[1] >= 1 and seen[2] >= 1, seen
    assert ref["info"][4] >= 5
    eng = _engine(m)
    got = _check(eng, 1200, ref)
    assert got["info"][4] >= 5
    eng.close()


# ---------------------------------------------------------------------------------------------
# 5. literal mode: a candidate blocks on OverCapacity
# ---------------------------------------------------------------------------------------------
def test_literal_mode_blocks_on_over_capacity():
    case = (7, 360, 1200, LITERAL)
    ref = _ref(*case, 1200, "plain", "desc")
    # (the reference alone gives: 299 removed, 46 blocked on OverCapacity, 15 destinations)
    blocked = ref["outcome"] == cr.BLOCKED
    assert blocked.sum() >= 20 and (ref["block_status"][blocked] == OVER).all() and ref["info"][1] >= 100
    feeds = _ref(*CASE1, 1200)
    assert (feeds["block_status"][feeds["outcome"] == cr.BLOCKED] == NOT_FOUND).any(), "both block statuses are covered"
    eng = _engine(_model(*case))
    got = _check(eng, 1200, ref)
    assert (got["block_status"][got["outcome"] == cr.BLOCKED] == OVER).all()
    eng.close()


# ---------------------------------------------------------------------------------------------
# 6. the other engine kinds
# ---------------------------------------------------------------------------------------------
def _parity_ref(case, t, nodes=None):
    return cr.pysim_consolidate(dr.sim_at(case, t), t, list(range(32)) if nodes is None else nodes)


def test_after_an_aborted_run():
    from kubesim_amd.engine import KsError
    from pysim import PySim
    tr = small_trace(9)   # 15 binds, then a pod whose selector no node carries
    enc = encoded(tr)
    fm, fl, sc = MODES[FEEDS]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    binds, err = ps.step(200)
    assert err == "NotFound" and len(binds) >= 8
    eng = make_engine(tr, enc, FEEDS, batch_pods=64)
    eng.submit(enc["pods"])
    with pytest.raises(KsError) as ex:
        eng.step(200)
    assert ex.value.kind == "NotFound" and eng.tick == ps.tick
    ref = cr.pysim_consolidate(ps, ps.tick, list(range(ps.n)))
    assert ref["evicted"].sum() >= 3 and ref["info"][1] >= 2
    _check(eng, eng.tick, ref, "aborted run")
    with pytest.raises(KsError):
        eng.consolidate_at(eng.tick + 1, [0])
    eng.close()


def test_group_members_answer_for_their_own_scenario():
    from kubesim_amd.engine import Group
    g = Group(2)
    cases = ("feeds", "feeds_irregular")
    engs = []
    for case in cases:
        r = pr.parity_case(case)
        fm, fl, sc = MODES[FEEDS]
        e = g.add(tick_seconds=r["tr"]["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(r["enc"]["alloc"], r["enc"]["taint"], r["enc"]["label"])
        e.submit(r["enc"]["pods"])
        engs.append(e)
    binds, counts, st, _ = g.step(pr.T)
    assert (st == 0).all()
    moved = 0
    for case, e in zip(cases, engs):
        for t in (400, pr.T):
            ref = _parity_ref(case, t)
            moved += int(ref["info"][5])
            _check(e, t, ref, f"group member {case} tick {t}")
    assert moved >= 8
    g.close()


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_ranks"])
def test_other_engine_kinds_give_the_same_chain(how):
    from kubesim_amd import _lib
    r = pr.parity_case("feeds")
    refs = {t: _parity_ref("feeds", t) for t in (137, pr.T)}
    assert sum(int(x["info"][5]) for x in refs.values()) >= 4 and any(x["info"][3] for x in refs.values())
    if how == "two_ranks":
        engs, x = shard_ranks(r["tr"], r["enc"], 2, 1, batch_pods=64)
        step_ranks(engs, pr.T, x)
    else:
        eng = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64, engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER)
        eng.submit(r["enc"]["pods"])
        eng.step(pr.T)
        engs = [eng]
    for t, ref in refs.items():
        for rank, eng in enumerate(engs):
            _check(eng, t, ref, f"{how} rank {rank} tick {t}")
    for eng in engs:
        eng.close()


def test_a_twin_that_made_no_call_steps_on_alike():
    r = pr.parity_case("feeds")

    def fresh():
        e = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64)
        e.submit(r["enc"]["pods"])
        return e, e.step(400)
    eng, eb = fresh()
    twin, tb = fresh()
    rng = np.random.default_rng(5)
    for t in (1, 137, 400):
        _check(eng, t, _parity_ref("feeds", t), f"tick {t}")
        order = [int(x) for x in rng.permutation(32)]
        _check(eng, t, _parity_ref("feeds", t, order), f"tick {t} permuted")
    np.testing.assert_array_equal(eng.requested_at(400), twin.requested_at(400))
    nb, ntb = eng.step(400), twin.step(400)
    assert len(nb) >= 100
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    np.testing.assert_array_equal(eng.requested_at(800), twin.requested_at(800))
    _check(eng, 800, _parity_ref("feeds", 800), "tick 800 after stepping on")
    eng.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# 7. errors on a live engine: nothing is written
# ---------------------------------------------------------------------------------------------
def _raw(eng, t, nodes, m=None, cap=4096, rows=True, out=True, n_ev=True, n_rows=True):
    """ks_consolidate_at itself on sentinel-filled outputs: (status, outputs untouched, ks_last_error)."""
    from kubesim_amd import _lib
    from kubesim_amd.engine import CONSOLIDATION_DTYPE, EVICTION_DTYPE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nd = np.ascontiguousarray(nodes, np.int32)
    res = np.full(max(len(nd), 1) * CONSOLIDATION_DTYPE.itemsize, 0x5A, np.uint8)
    buf = np.full(max(cap, 1) * EVICTION_DTYPE.itemsize, 0x5A, np.uint8)
    info = np.full(_lib.KS_CONSOLIDATE_INFO, 0x5A5A, np.int64)
    cnt = np.full(2, 0x5A5A, np.int64)
    q = lambda a, i: C.cast(a.ctypes.data + 8 * i, C.POINTER(C.c_int64))
    rc = eng._L.ks_consolidate_at(eng.h, t, len(nd) if m is None else m, p(nd) if len(nd) else p(np.zeros(1, np.int32)),
                                  p(res) if out else None, p(buf) if rows else None, cap,
                                  q(cnt, 0) if n_ev else None, q(cnt, 1) if n_rows else None, None, p(info))
    clean = bool((res == 0x5A).all() and (buf == 0x5A).all() and (info == 0x5A5A).all() and (cnt == 0x5A5A).all())
    return rc, clean, eng._L.ks_last_error(eng.h).decode()


def test_argument_errors_write_nothing():
    from kubesim_amd import _lib
    from kubesim_amd.engine import Engine, KsError
    r = pr.parity_case("feeds")
    eng = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64)
    eng.submit(r["enc"]["pods"])
    eng.step(400)
    bad = {
        "a node past the end": dict(t=400, nodes=[0, 32]),
        "a negative node": dict(t=400, nodes=[3, -1]),
        "a node listed twice": dict(t=400, nodes=[5, 9, 5]),
        "no nodes": dict(t=400, nodes=[], m=0),
        "more nodes than the cluster has": dict(t=400, nodes=list(range(32)) + [0], m=33),
        "a negative count": dict(t=400, nodes=[1], m=-1),
        "tick past the current one": dict(t=401, nodes=[1]),
        "negative tick": dict(t=-1, nodes=[1]),
        "rows NULL with room asked for": dict(t=400, nodes=[1], rows=False),
        "negative cap": dict(t=400, nodes=[1], cap=-1),
        "out NULL": dict(t=400, nodes=[1], out=False),
        "n_evicted NULL": dict(t=400, nodes=[1], n_ev=False),
        "n_rows NULL": dict(t=400, nodes=[1], n_rows=False),
    }
    quiet = ("rows NULL with room asked for", "negative cap", "out NULL", "n_evicted NULL", "n_rows NULL")
    for what, kw in bad.items():
        rc, clean, msg = _raw(eng, **kw)
        assert rc == _lib.KS_EINVAL and clean, what
        if what not in quiet:
            assert msg, what
    with pytest.raises(KsError) as ex:
        eng.consolidate_at(400, [7, 7])
    assert ex.value.kind == "InvalidArgument" and "twice" in str(ex.value)
    for nodes in ([31], list(range(32))):
        rc, clean, _ = _raw(eng, 400, nodes)
        assert rc == _lib.KS_OK and not clean
    rc, clean, _ = _raw(eng, 400, list(range(32)), cap=0, rows=False)
    assert rc == _lib.KS_OK and not clean
    fm, fl, sc = MODES[FEEDS]
    empty = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    rc, clean, msg = _raw(empty, 0, [0])
    assert rc == _lib.KS_EINVAL and clean and "no nodes" in msg
    z = np.zeros(0, np.uint64)
    empty.load_nodes(np.zeros((0, 4), np.int64), z, z)       # n = 0: no candidate, nothing evicted
    got = empty.consolidate_at(0, [], rows=True)
    assert len(got["node"]) == 0 and got["info"].tolist() == [0] * 6 and len(got["rows"]["pod"]) == 0
    empty.close()
    eng.close()
