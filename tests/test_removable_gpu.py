"""GPU parity of the removal scan (include/ks_engine.h: ks_removable_at) against tests/removable_ref.py:
``drain_ref.fast_drain`` once per candidate with ``drained=[c]`` on the C oracle's binds, PySim with
one node removed on the shared 32-node trace (the two are equal: tests/test_removable_ref.py), and the
engine's own ``drain_at(t, [c])``.  Everything is exact integer equality.

Each reference is built once, checked on its own for the properties that keep the comparison from
passing vacuously before any engine call, and never changed afterwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import drain_ref as dr
import place_ref as pr
import removable_ref as rr
from harness import MODES, assert_same_binds, encoded, make_engine, make_oracle, shard_ranks, small_trace, step_ranks

pytestmark = pytest.mark.gpu

FEEDS, LITERAL = pr.FEEDS, pr.LITERAL
OK, OVER, NOT_FOUND = pr.OK, pr.OVER, pr.NOT_FOUND
FIVE = [(500, 1024), (1000, 2048), (2000, 1024), (1500, 4096), (4000, 8192)]   # milli-cpu, Mi
MI = (1 << 20) * 1000                                                           # a Mi in milli-bytes


@functools.lru_cache(maxsize=None)
def _model(seed, n_nodes, n_pods, mode, kind="plain"):
    """test_drain_gpu._model's recipe: the trace, its encoding and the C oracle's binds over n_pods
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
    m = _model(seed, n_nodes, n_pods, mode, kind)
    return rr.fast_removable(m["tr"], m["enc"], m["ob"], m["cfg"], t, list(range(n_nodes)) if nodes is None else list(nodes))


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
    got = eng.removable_at(t, ref["node"], rows=rows)
    rr.assert_same(got, ref, what or f"tick {t}", rows=rows)
    return got


CASE1 = (7, 360, 1200, FEEDS)


@pytest.fixture(scope="module")
def eng360():
    eng = _engine(_model(*CASE1))
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------
# 1. 360 nodes / 1,200 pods, every node a candidate, (nearly) every pod a shape of its own
# ---------------------------------------------------------------------------------------------
def test_every_node_a_candidate(eng360):
    from kubesim_amd import _lib
    m, ref = _model(*CASE1), _ref(*CASE1, 1200)
    ev = ref["evicted"]
    occupied, total = int((ev > 0).sum()), int(ev.sum())
    shapes = _shape_count(m, ref["rows"]["pod"].tolist())
    # (the reference alone gives: 340 occupied, 20 empty, 1,152 pods of 1,148 shapes, at most 10 on a
    # node, 320 occupied candidates removable, 20 with a NOT_FOUND pod, 39 pods whose own node heads
    # their un-cordoned score vector and 493 with it in the top 32, 9 candidates that reuse a node)
    assert occupied >= 300 and (ev == 0).sum() >= 10 and total >= 1100 and shapes >= 18 * 64 - 63
    assert 1 <= ev.max() <= _lib.KS_REMOVABLE_MAX_BATCHED, "a candidate would take the single-drain path"
    removable = ref["removable"] & (ev > 0)
    assert removable.sum() >= 300 and (~ref["removable"]).sum() >= 10 and ref["not_found"].sum() >= 10
    ranks = rr.own_node_ranks(m["enc"], m["cfg"], ref["state"], ref)
    assert (ranks == 0).sum() >= 20, "few pods whose own node heads their un-cordoned score vector"
    assert ((ranks >= 0) & (ranks < 32)).sum() >= 300, "few pods with their own node in their snapshot list"
    assert len(rr.reusing_candidates(ref)) >= 5, "few candidates place two pods on one node"
    used = ref["rows"]["node"]
    assert (ev[:256] > 0).any() and (ev[256:] > 0).any() and ((used >= 0) & (used < 256)).any() and (used >= 256).any()
    got = _check(eng360, 1200, ref)
    info = got["info"].tolist()
    assert info[0] >= 18 and info[1] == occupied and info[2] == 0, info


# ---------------------------------------------------------------------------------------------
# 2. a past tick; a permuted subset in the caller's order; summaries only; a short row buffer
# ---------------------------------------------------------------------------------------------
def test_a_past_tick_and_a_permuted_subset(eng360):
    from kubesim_amd import _lib
    from kubesim_amd.engine import EVICTION_DTYPE, REMOVAL_DTYPE
    m, ref = _model(*CASE1), _ref(*CASE1, 700)
    ob = m["ob"]
    later = set(ob["pod"][ob["tick"] > 700].tolist())
    assert ref["evicted"].sum() >= 300 and len(later) >= 200 and not later & set(ref["rows"]["pod"].tolist())
    assert ref["removable"].sum() >= 100
    got = _check(eng360, 700, ref)
    assert not later & set(got["rows"]["pod"].tolist())
    np.testing.assert_array_equal(eng360.requested_at(700), ref["state"])
    # a permuted subset, the bitmap's word edges and the scan's block edge among it
    rng = np.random.default_rng(360)
    sub = [0, 31, 32, 255, 256, 359] + [int(x) for x in rng.permutation(np.arange(33, 255))[:60]]
    sub = [sub[i] for i in rng.permutation(len(sub))]
    assert sub != sorted(sub)
    want = rr.assemble(sub, [ref["per"][c] for c in sub])
    assert want["evicted"].sum() >= 50 and (want["evicted"] == 0).any() and (np.diff(want["rows"]["pod"]) < 0).any()
    part = eng360.removable_at(700, sub, rows=True)
    rr.assert_same(part, want, "permuted subset")
    # summaries only are the summaries with rows
    plain = _check(eng360, 700, want, "summaries only", rows=False)
    assert plain["rows"] is None
    np.testing.assert_array_equal(plain["info"], part["info"])
    # too little room: KS_ERANGE, the count, nothing else written
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nodes = np.arange(360, dtype=np.int32)
    total = int(ref["evicted"].sum())
    out = np.full(360 * REMOVAL_DTYPE.itemsize, 0x5A, np.uint8)
    rows = np.full(100 * EVICTION_DTYPE.itemsize + 64, 0x5A, np.uint8)
    info = np.full(_lib.KS_REMOVABLE_INFO, 0x5A5A, np.int64)
    n_rows = C.c_int64(-1)
    rc = eng360._L.ks_removable_at(eng360.h, 700, 360, p(nodes), p(out), p(rows), 100, C.byref(n_rows), p(info))
    assert rc == _lib.KS_ERANGE and n_rows.value == total
    assert (out == 0x5A).all() and (rows == 0x5A).all() and (info == 0x5A5A).all()


# ---------------------------------------------------------------------------------------------
# 3. literal mode: every other node is a candidate whatever its state
# ---------------------------------------------------------------------------------------------
def test_literal_mode_over_capacity():
    case = (5, 600, 1200, LITERAL)
    m, ref = _model(*case), _ref(*case, 1200)
    ev = ref["evicted"]
    # (the reference alone gives: 155 occupied, 260 pods, 6 removable, 149 with an OverCapacity pod)
    assert (ev > 0).sum() >= 100 and ev.sum() >= 200
    assert (ref["removable"] & (ev > 0)).sum() >= 3 and (ref["over_capacity"] > 0).sum() >= 100
    assert (ref["rows"]["candidates"] == 599).all()
    eng = _engine(m)
    got = _check(eng, 1200, ref)
    assert (got["rows"]["candidates"] == 599).all() and got["info"][2] == 0
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. many pods per node: the split between the batched kernel and the single-drain path
# ---------------------------------------------------------------------------------------------
def test_many_pods_per_node_take_the_single_drain_path():
    from kubesim_amd import _lib
    case = (5, 40, 1600, FEEDS)
    m, ref = _model(*case, "tiny"), _ref(*case, 1600, "tiny")
    ev = ref["evicted"]
    big, small = int((ev > _lib.KS_REMOVABLE_MAX_BATCHED).sum()), int(((ev > 0) & (ev <= _lib.KS_REMOVABLE_MAX_BATCHED)).sum())
    # (the reference alone gives: 16 occupied, 1,546 pods, up to 110 on a node, 15 candidates with 32
    # pods or more and 1 with fewer, all removable)
    assert (big, small) == (15, 1) and ev.max() >= 100 and ev.sum() >= 1500 and ref["removable"].all()
    eng = _engine(m)
    got = _check(eng, 1600, ref)
    assert got["info"].tolist()[1:4] == [1, 15, 24], got["info"]
    eng.close()


# ---------------------------------------------------------------------------------------------
# 5. shared shapes: one segment serves every candidate
# ---------------------------------------------------------------------------------------------
def test_five_shapes_one_segment():
    case = (5, 600, 1200, FEEDS)
    m, ref = _model(*case, "five"), _ref(*case, 1200, "five")
    ev = ref["evicted"]
    assert _shape_count(m, ref["rows"]["pod"].tolist()) == 5 and (ev > 0).sum() >= 100 and ev.max() <= 31
    eng = _engine(m)
    got = _check(eng, 1200, ref)
    assert got["info"][0] == 1 and got["info"][1] >= 100 and got["info"][2] == 0, got["info"]
    eng.close()


# ---------------------------------------------------------------------------------------------
# 6. the definition itself: the same engine's drain_at(t, [c])
# ---------------------------------------------------------------------------------------------
def test_equals_the_engines_own_single_node_drain(eng360):
    ref = _ref(*CASE1, 1200)
    stuck = [int(c) for c in np.nonzero(~ref["removable"])[0][:6]]
    reusing = rr.reusing_candidates(ref)[:4]
    empty = [int(c) for c in np.nonzero(ref["evicted"] == 0)[0][:2]]
    rest = [int(c) for c in np.nonzero(ref["removable"] & (ref["evicted"] >= 3))[0][:8]]
    sample = sorted(set(stuck + reusing + empty + rest))
    assert len(stuck) >= 5 and len(empty) == 2 and len(sample) >= 18
    got = eng360.removable_at(1200, sample, rows=True)
    for j, c in enumerate(sample):
        one = eng360.drain_at(1200, [c])
        a, b = int(got["first_row"][j]), int(got["first_row"][j] + got["evicted"][j])
        assert len(one["pod"]) == b - a == ref["evicted"][c]
        for f in dr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f][a:b], one[f], err_msg=f"node {c}: {f}")
        assert [got["ok"][j], got["over_capacity"][j], got["not_found"][j]] == one["info"][1:4].tolist()
        assert bool(got["removable"][j]) == bool(one["info"][1] == len(one["pod"]))


# ---------------------------------------------------------------------------------------------
# 7. the other engine kinds
# ---------------------------------------------------------------------------------------------
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
    ref = rr.pysim_removable(ps, ps.tick, list(range(ps.n)))
    assert ref["evicted"].sum() >= 3 and (ref["evicted"] > 0).sum() >= 2
    _check(eng, eng.tick, ref, "aborted run")
    with pytest.raises(KsError):
        eng.removable_at(eng.tick + 1, [0])
    eng.close()


def _parity_ref(case, t):
    return rr.pysim_removable(dr.sim_at(case, t), t, list(range(32)))


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
    evicted = 0
    for case, e in zip(cases, engs):
        for t in (400, pr.T):
            ref = _parity_ref(case, t)
            evicted += int(ref["evicted"].sum())
            _check(e, t, ref, f"group member {case} tick {t}")
    assert evicted >= 8
    g.close()


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_node_shards", "two_ranks"])
def test_other_engine_kinds_give_the_same_scan(how):
    from kubesim_amd import _lib
    r = pr.parity_case("feeds")
    refs = {t: _parity_ref("feeds", t) for t in (137, pr.T)}
    assert sum(int(x["evicted"].sum()) for x in refs.values()) >= 4 and any(x["ok"].any() for x in refs.values())
    if how == "two_ranks":
        engs, x = shard_ranks(r["tr"], r["enc"], 2, 1, batch_pods=64)
        step_ranks(engs, pr.T, x)
    else:
        kw = dict(engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER) if how == "one_pod_resolver" else dict(shard=(1, 0, None, 2))
        eng = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64, **kw)
        eng.submit(r["enc"]["pods"])
        eng.step(pr.T)
        engs = [eng]
    for t, ref in refs.items():
        for rank, eng in enumerate(engs):
            _check(eng, t, ref, f"{how} rank {rank} tick {t}")
    for eng in engs:
        eng.close()


# ---------------------------------------------------------------------------------------------
# 8. errors and isolation
# ---------------------------------------------------------------------------------------------
def _raw(eng, t, nodes, m=None, cap=4096, rows=True, out=True, n_rows=True):
    """ks_removable_at itself on sentinel-filled outputs: (status, outputs untouched, ks_last_error)."""
    from kubesim_amd import _lib
    from kubesim_amd.engine import EVICTION_DTYPE, REMOVAL_DTYPE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    nd = np.ascontiguousarray(nodes, np.int32)
    res = np.full(max(len(nd), 1) * REMOVAL_DTYPE.itemsize, 0x5A, np.uint8)
    buf = np.full(max(cap, 1) * EVICTION_DTYPE.itemsize, 0x5A, np.uint8)
    info = np.full(_lib.KS_REMOVABLE_INFO, 0x5A5A, np.int64)
    cnt = np.full(1, 0x5A5A, np.int64)
    rc = eng._L.ks_removable_at(eng.h, t, len(nd) if m is None else m, p(nd) if len(nd) else p(np.zeros(1, np.int32)),
                                p(res) if out else None, p(buf) if rows else None, cap,
                                cnt.ctypes.data_as(C.POINTER(C.c_int64)) if n_rows else None, p(info))
    clean = bool((res == 0x5A).all() and (buf == 0x5A).all() and (info == 0x5A5A).all() and (cnt == 0x5A5A).all())
    return rc, clean, eng._L.ks_last_error(eng.h).decode()


def test_argument_errors_and_no_side_effects():
    """Every KS_EINVAL of the header, with nothing written; and a run that made removal scans goes on
    exactly as a twin that made none."""
    from kubesim_amd import _lib
    from kubesim_amd.engine import Engine, KsError
    r = pr.parity_case("feeds")

    def fresh():
        e = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64)
        e.submit(r["enc"]["pods"])
        return e, e.step(400)
    eng, eb = fresh()
    twin, tb = fresh()
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
        "n_rows NULL": dict(t=400, nodes=[1], n_rows=False),
    }
    quiet = ("rows NULL with room asked for", "negative cap", "out NULL", "n_rows NULL")
    for what, kw in bad.items():
        rc, clean, msg = _raw(eng, **kw)
        assert rc == _lib.KS_EINVAL and clean, what
        if what not in quiet:
            assert msg, what
    with pytest.raises(KsError) as ex:
        eng.removable_at(400, [7, 7])
    assert ex.value.kind == "InvalidArgument" and "twice" in str(ex.value)
    # the limits themselves are accepted: one node, and all of them; summaries only with cap 0
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
    got = empty.removable_at(0, [], rows=True)
    assert len(got["node"]) == 0 and got["info"].tolist() == [0] * 6 and len(got["rows"]["pod"]) == 0
    rc, clean, msg = _raw(empty, 0, [0])
    assert rc == _lib.KS_EINVAL and clean
    empty.close()
    # scans at several ticks, then both engines step on: the same binds, the same state
    for t in (1, 137, 400):
        _check(eng, t, _parity_ref("feeds", t), f"tick {t}")
    np.testing.assert_array_equal(eng.requested_at(400), twin.requested_at(400))
    nb, ntb = eng.step(400), twin.step(400)
    assert len(nb) >= 100
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    np.testing.assert_array_equal(eng.requested_at(800), twin.requested_at(800))
    _check(eng, 800, _parity_ref("feeds", 800), "tick 800 after stepping on")
    eng.close()
    twin.close()
