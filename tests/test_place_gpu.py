"""GPU parity of the placement preview (include/ks_engine.h: ks_place_at) against the references of
tests/place_ref.py: oracle/pysim.py's PySim asked pod after pod on the shared 32-node trace, and the
integer walk ``fast_place`` (equal to it: tests/test_place_ref.py) on the larger clusters.
Everything is exact integer equality.

Each reference is built once, checked on its own for the properties that keep the comparison from
passing vacuously before any engine call, and never changed afterwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import headroom_ref as hr
import place_ref as pr
from harness import MODES, assert_same_binds, encoded, make_engine, make_oracle, small_trace

pytestmark = pytest.mark.gpu

T = pr.T
LRBA = (1, 7, ((1, 1, 0), (2, 1, 0)))    # the fit, taint and selector filters feed LeastRequested + BalancedAllocation


def _engine_run(tr, mode, ticks=T, batch_pods=64, engine_flags=0, shard=None):
    enc = encoded(tr)
    eng = make_engine(tr, enc, mode, batch_pods=batch_pods, engine_flags=engine_flags, shard=shard)
    eng.submit(enc["pods"])
    return eng, eng.step(ticks)


def _same_binds(eb, binds):
    assert_same_binds(eb, dict(pod=binds[:, 0], node=binds[:, 1], tick=binds[:, 2], status=binds[:, 3]))


def _check(eng, t, shapes, shape_of, want, what=""):
    got = eng.place_at(t, shapes, shape_of, after=True)
    pr.assert_same(got, want, what or f"tick {t}")
    assert got["info"][0] >= 1 and sum(got["info"][1:]) == len(want["node"])
    return got


# ---------------------------------------------------------------------------------------------
# 1. parity on the shared trace: 32 nodes are one ragged block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_parity_at_six_ticks_of_one_batched_step(case):
    r = pr.parity_case(case)
    pr.assert_not_vacuous(case, r["slow"])
    eng, eb = _engine_run(r["tr"], pr.CASES[case][0])
    assert eng.last_step_stats()["launches"] > 10
    _same_binds(eb, r["binds"])
    for t in pr.TICKS:
        _check(eng, t, r["shapes"], r["shape_of"], r["slow"][t], f"{case} tick {t}")
        # whole-unit requests only: the call runs in device units
        _check(eng, t, r["whole"], r["whole_of"], r["fast_whole"][t], f"{case} tick {t}, whole units")
    assert any(len(set(ref["node"].tolist())) >= 8 for ref in r["fast_whole"].values())
    # without after_out the placements are the same
    got = eng.place_at(400, r["shapes"], r["shape_of"])
    assert got["after"] is None
    for f in pr.FIELDS:
        np.testing.assert_array_equal(got[f], r["slow"][400][f])
    eng.close()


# ---------------------------------------------------------------------------------------------
# 2, 3. 600 nodes: three blocks and a ragged tail
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_600():
    tr = small_trace(5, n_nodes=600, n_pods=400, arrival="stream", selectors=False)
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 997
    enc = encoded(tr)
    ora = make_oracle(tr, LRBA)
    ora.submit(tr)
    ob, rc = ora.step(400, cap=400)
    assert rc == 0 and len(ob["pod"]) > 350
    state = pr.state_from_binds(tr, enc, ob, 400)
    assert state[:, 3].sum() > 50
    a = enc["alloc"]
    cpu6, mem6 = int(np.median(a[:, 0])) // 6, int(np.median(a[:, 1])) // 6
    # two shapes of about a sixth of a node (the second cpu-heavier; the first's memory is odd),
    # a whole large node, and 64 distinct ones
    two = dict(req=np.array([[cpu6, mem6 + 1, 0], [cpu6 // 2 * 3, mem6 // 2, 0]], np.int64), keymask=np.array([3, 3], np.uint8),
               tol=np.array([hr.ALL_BITS] * 2), sel=np.zeros(2, np.uint64))
    big = dict(req=np.array([[32000, int(np.median(a[:, 1])), 0]], np.int64), keymask=np.array([3], np.uint8),
               tol=np.array([hr.ALL_BITS]), sel=np.zeros(1, np.uint64))
    many, _ = hr.make_shapes(tr, enc, dict(ps=_Pods(400)), list(range(0, 59 * 6, 6)), pr.HAND)
    assert len(many["keymask"]) == 64 and len({tuple(r) for r in many["req"].tolist()}) > 30
    shape_of = np.concatenate([np.arange(512) % 2, (np.arange(512) // 64) % 2]).astype(np.int32)   # alternating, then runs
    cfg = pr.engine_cfg(LRBA, enc)
    return dict(tr=tr, enc=enc, ob=ob, state=state, cfg=cfg, two=two, big=big, many=many, shape_of=shape_of,
                ref_two=pr.fast_place(a, state, cfg, two, shape_of), ref_many=pr.fast_place(a, state, cfg, many))


class _Pods:
    """make_shapes only reads ps.pods[j] for the checker's string form, which fast_place does not use."""

    def __init__(self, m):
        self.pods = [dict(tols=[], sel={})] * m


@pytest.fixture(scope="module")
def eng600():
    r = _model_600()
    eng, eb = _engine_run(r["tr"], LRBA, ticks=400)
    assert_same_binds(eb, r["ob"])
    np.testing.assert_array_equal(eng.requested_at(400), r["state"])
    yield eng
    eng.close()


def test_rounds_1024_pods_of_two_shapes_on_600_nodes(eng600):
    r = _model_600()
    ref = r["ref_two"]
    used = ref["node"][ref["node"] >= 0]
    assert len(set(used.tolist())) >= 200 and len(ref["reused"]) >= 100
    assert (used < 256).any() and ((used >= 256) & (used < 512)).any() and (used >= 512).any()
    got = _check(eng600, 400, r["two"], r["shape_of"], ref)
    assert got["info"][0] >= 3, "the lists were never exhausted"


def test_single_shape_slices_agree_with_headroom(eng600):
    r = _model_600()
    a = r["enc"]["alloc"]
    k = 1024
    for name, sh in (("a sixth of a node", {f: v[:1] for f, v in r["two"].items()}), ("a large node", r["big"])):
        head = eng600.headroom_at(400, sh)
        so = np.zeros(k, np.int32)
        ref = pr.fast_place(a, r["state"], r["cfg"], sh, so)
        got = _check(eng600, 400, sh, so, ref, name)
        assert got["info"][1] == min(k, head[0, 0]), name
        assert got["candidates"][0] == head[0, 1], name
        assert got["info"][2] == 0
    # the large shape runs out of room inside the call: the tail is NOT_FOUND
    assert 0 < head[0, 0] < k and (got["status"][int(head[0, 0]):] == pr.NOT_FOUND).all()


def test_64_distinct_shapes_one_pod_each(eng600):
    r = _model_600()
    ref = r["ref_many"]
    assert len(set(ref["status"].tolist())) >= 2 and len(set(ref["candidates"].tolist())) >= 5
    got = _check(eng600, 400, r["many"], None, ref)
    assert len(got["node"]) == 64


# ---------------------------------------------------------------------------------------------
# 4. domain edges on the device, and no side effects: a hand-made cluster, no trace
# ---------------------------------------------------------------------------------------------
TOP = (1 << 59) - 1
MEM_UNIT = (1 << 30) * 1000      # every memory quantity of the edge cluster is a multiple of it
EDGE_MODE = (1, 1, ((1, 1, 0),))  # the fit filter feeds LeastRequested


def _edge_cluster():
    cpus = [TOP, TOP - 1, 1 << 58, (1 << 53) + 1, 1 << 53, (1 << 53) - 1, ((1 << 31) - 1) * 1000,
            ((1 << 31) - 2) * 1000 + 999, (1 << 22) + 1, 1 << 22, (1 << 22) - 1, 128000, 8000, 1000, 999, 1, 0, -1]
    mems = [TOP // MEM_UNIT * MEM_UNIT, (1 << 18) * MEM_UNIT, 4096 * MEM_UNIT, 512 * MEM_UNIT, 7 * MEM_UNIT, MEM_UNIT, 0, -1]
    gpus = [8000, 1000, 0, -1, (1 << 31) * 1000]
    aps = [110, 0, 1, 3, TOP, (1 << 31) - 1, 1 << 31, (1 << 31) - 2]
    rows = []
    for i in range(300):
        rows.append([cpus[i % len(cpus)], mems[(i // 3) % len(mems)], gpus[(i // 7) % len(gpus)], aps[(i // 2) % len(aps)]])
    return np.array(rows, np.int64)


def _edge_pods(m=30):
    req = np.zeros((m, 3), np.int64)
    req[:, 0] = [(1 << 57) + 1, 1 << 56, 3, 1000, (1 << 52) + 5, 7][:6] * (m // 6)
    req[:, 1] = [MEM_UNIT * x for x in (1 << 17, 3, 1, 500, 4000, 2)] * (m // 6)
    return dict(m=m, arrival=np.zeros(m, np.int64), req=req, keymask=np.full(m, 3, np.uint8),
                tol=np.zeros(m, np.uint64), sel=np.zeros(m, np.uint64), phase_off=np.arange(m + 1, dtype=np.int32),
                phase_sec=np.full(m, 100_000, np.int32), phase_use=np.zeros((m, 3), np.int64),
                flags=np.zeros(m, np.uint8))


def _edge_shapes():
    rows = []
    for q in (1, 3, 1000, (1 << 22) + 1, (1 << 53) + 1, TOP // 7, 1 << 58, TOP - 1, TOP):
        rows.append(([q, 0, 0], 1))
    for q in (1, MEM_UNIT - 1, MEM_UNIT + 1, 7 * MEM_UNIT + 3, (1 << 18) * MEM_UNIT // 3 + 1, TOP):   # coprime to the unit
        rows.append(([0, q, 0], 2))
    for q in (1, 1001, 0):
        rows.append(([0, 0, q], 4))
    rows += [([1000, MEM_UNIT + 1, 0], 3), ([3, 1, 1], 7), ([0, 0, 0], 7), ([9, 9, 9], 0), ([1 << 57, MEM_UNIT, 1000], 7),
             ([TOP // 3, TOP // MEM_UNIT * MEM_UNIT // 3 + 1, 0], 3), ([-5, 1 << 60, 1000], 4)]   # junk in unmasked keys
    k = len(rows)
    return dict(req=np.array([r for r, _ in rows], np.int64), keymask=np.array([m for _, m in rows], np.uint8),
                tol=np.zeros(k, np.uint64), sel=np.zeros(k, np.uint64))


def test_domain_edges_and_no_side_effects():
    from kubesim_amd.engine import Engine
    alloc = _edge_cluster()
    pods = _edge_pods()
    zeros = np.zeros(len(alloc), np.uint64)
    shapes = _edge_shapes()
    ns = len(shapes["keymask"])
    shape_of = (np.arange(300) * 7 % ns).astype(np.int32)

    def fresh(mode=EDGE_MODE, steps=10):
        fm, fl, sc = mode
        e = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(alloc, zeros, zeros)
        e.submit(pods)
        return e, (e.step(steps) if steps else None)
    eng, b = fresh()
    twin, tb = fresh()
    assert len(b) == 10 and (b["status"] == 0).all()
    r10 = np.zeros((len(alloc), 4), np.int64)     # every pod runs for 10,000 ticks
    for pod, node in zip(b["pod"].tolist(), b["node"].tolist()):
        r10[node, :3] += pods["req"][pod]
        r10[node, 3] += 1
    cfg = dict(filter_mode=1, filters=1, scorers=EDGE_MODE[2], taint=zeros, label=zeros)
    refs = {0: pr.fast_place(alloc, np.zeros_like(r10), cfg, shapes, shape_of), 10: pr.fast_place(alloc, r10, cfg, shapes, shape_of)}
    for t, ref in refs.items():
        assert {pr.OK, pr.NOT_FOUND} <= set(ref["status"].tolist()) and len(set(ref["node"].tolist())) >= 20
        assert (ref["after"][:, :3].max(axis=0) > 1 << 57).any()
        _check(eng, t, shapes, shape_of, ref, f"edge cluster tick {t}")
    # the wide BalancedAllocation (128-bit products) on the same cluster, never stepped
    lrba, _ = fresh(LRBA, steps=0)
    cfg2 = dict(filter_mode=1, filters=7, scorers=LRBA[2], taint=zeros, label=zeros)
    ref = pr.fast_place(alloc, np.zeros_like(r10), cfg2, shapes, shape_of)
    assert len(set(ref["score"].tolist())) >= 5
    _check(lrba, 0, shapes, shape_of, ref, "edge cluster, LeastRequested + BalancedAllocation")
    lrba.close()
    # nothing changed: the state reads back as before and the run goes on as its twin's
    np.testing.assert_array_equal(eng.requested_at(10), r10)
    np.testing.assert_array_equal(eng.requested_at(10), twin.requested_at(10))
    nb, ntb = eng.step(10), twin.step(10)
    assert len(nb) == 10
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    np.testing.assert_array_equal(eng.requested_at(20), twin.requested_at(20))
    eng.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# 5. engine kinds
# ---------------------------------------------------------------------------------------------
def test_preview_of_the_pod_an_aborted_run_stopped_at():
    from kubesim_amd.engine import KsError
    from pysim import PySim
    tr = small_trace(9)   # 15 binds, then a pod whose selector no node carries
    enc = encoded(tr)
    fm, fl, sc = MODES[pr.FEEDS]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    binds, err = ps.step(200)
    assert err == "NotFound" and len(binds) >= 8
    stopped = len(binds)                      # FIFO: the pod after the last bound one
    eng = make_engine(tr, enc, pr.FEEDS, batch_pods=64)
    eng.submit(enc["pods"])
    with pytest.raises(KsError) as ex:
        eng.step(200)
    assert ex.value.kind == "NotFound"
    _same_binds(ex.value.binds, np.array(binds, np.int64).reshape(-1, 4))
    assert eng.tick == ps.tick
    ids = [stopped, 0, stopped, 3]
    shapes = {f: np.ascontiguousarray(enc["pods"][f][ids]) for f in ("req", "keymask", "tol", "sel")}
    pods = [dict(req=ps.pods[j]["req"], tols=ps.pods[j]["tols"], sel=ps.pods[j]["sel"]) for j in ids]
    ref = pr.pysim_place(ps, ps.tick, pods)
    assert ref["status"][0] == ref["status"][2] == pr.NOT_FOUND and ref["candidates"][0] == 0
    assert ref["status"][1] == pr.OK
    _check(eng, eng.tick, shapes, None, ref)
    with pytest.raises(KsError):
        eng.place_at(eng.tick + 1, shapes)
    eng.close()


def test_group_members_answer_for_their_own_scenario():
    from kubesim_amd.engine import Group
    g = Group(2)
    cases = ("feeds", "feeds_irregular")
    engs = []
    for case in cases:
        r = pr.parity_case(case)
        fm, fl, sc = MODES[pr.FEEDS]
        e = g.add(tick_seconds=r["tr"]["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(r["enc"]["alloc"], r["enc"]["taint"], r["enc"]["label"])
        e.submit(r["enc"]["pods"])
        engs.append(e)
    binds, counts, st, _ = g.step(T)
    assert (st == 0).all()
    for case, e, eb in zip(cases, engs, g.split(binds, counts)):
        r = pr.parity_case(case)
        _same_binds(eb, r["binds"])
        for t in (1, 400, T):
            _check(e, t, r["shapes"], r["shape_of"], r["slow"][t], f"group member {case} tick {t}")
    g.close()


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_node_shards"])
def test_other_engine_kinds_give_the_same_preview(how):
    from kubesim_amd import _lib
    r = pr.parity_case("feeds")
    if how == "one_pod_resolver":
        eng, eb = _engine_run(r["tr"], pr.FEEDS, engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER)
    else:
        eng, eb = _engine_run(r["tr"], pr.FEEDS, shard=(1, 0, None, 2))
    _same_binds(eb, r["binds"])
    for t in (1, 137, T):
        _check(eng, t, r["shapes"], r["shape_of"], r["slow"][t], f"{how} tick {t}")
    eng.close()


def test_engine_without_scorers_finds_no_node():
    r = pr.parity_case("feeds")
    eng = make_engine(r["tr"], r["enc"], "no_scorers")
    got = eng.place_at(0, r["shapes"], r["shape_of"], after=True)
    assert (got["status"] == pr.NOT_FOUND).all() and (got["node"] == -1).all() and (got["score"] == -1).all()
    assert (got["candidates"] == 0).all() and not got["after"].any()
    assert got["info"].tolist() == [1, 0, 0, pr.N_PODS]
    eng.close()


# ---------------------------------------------------------------------------------------------
# 6. argument errors
# ---------------------------------------------------------------------------------------------
def _raw(eng, t, shapes, k, shape_of):
    """ks_place_at itself on sentinel-filled outputs: (status, outputs untouched, ks_last_error)."""
    from kubesim_amd.engine import PLACEMENT_DTYPE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    req = np.ascontiguousarray(shapes["req"], np.int64)
    km, tol, sel = (np.ascontiguousarray(shapes[f], d) for f, d in (("keymask", np.uint8), ("tol", np.uint64), ("sel", np.uint64)))
    out = np.full(max(k, 1) * PLACEMENT_DTYPE.itemsize + 64, 0x5A, np.uint8)
    after = np.full((eng.n, 4), 0x5A5A, np.int64)
    info = np.full(4, 0x5A5A, np.int64)
    so = None if shape_of is None else np.ascontiguousarray(shape_of, np.int32)
    rc = eng._L.ks_place_at(eng.h, t, len(km), p(req), p(km), p(tol), p(sel), k, None if so is None else p(so), p(out),
                            p(after), p(info))
    clean = bool((out == 0x5A).all() and (after == 0x5A5A).all() and (info == 0x5A5A).all())
    return rc, clean, eng._L.ks_last_error(eng.h).decode()


def test_argument_errors():
    from kubesim_amd import _lib
    from kubesim_amd.engine import Engine, KsError
    r = pr.parity_case("feeds")
    eng, eb = _engine_run(r["tr"], pr.FEEDS)
    _same_binds(eb, r["binds"])

    def shapes(k, **over):
        s = dict(req=np.tile(np.array([[1000, 1 << 30, 0]], np.int64), (k, 1)), keymask=np.full(k, 3, np.uint8),
                 tol=np.full(k, hr.ALL_BITS), sel=np.zeros(k, np.uint64))
        s.update(over)
        return s
    z = np.zeros
    bad = {
        "no shapes": (T, shapes(0), 1, z(1, np.int32)),
        "65 shapes": (T, shapes(65), 1, z(1, np.int32)),
        "no pods": (T, shapes(2), 0, z(1, np.int32)),
        "1025 pods": (T, shapes(2), 1025, z(1025, np.int32)),
        "shape_of = n_shapes": (T, shapes(2), 3, np.array([0, 2, 1], np.int32)),
        "shape_of = -1": (T, shapes(2), 3, np.array([0, 1, -1], np.int32)),
        "NULL shape_of, k != n_shapes": (T, shapes(2), 3, None),
        "keymask 8": (T, shapes(2, keymask=np.array([3, 8], np.uint8)), 2, None),
        "negative masked request": (T, shapes(2, req=np.array([[1000, 5, 0], [-1, 5, 0]], np.int64)), 2, None),
        "masked request of 2^59": (T, shapes(2, req=np.array([[1000, 5, 0], [1000, 1 << 59, 0]], np.int64)), 2, None),
        "tick past the current one": (T + 1, shapes(2), 2, None),
        "negative tick": (-1, shapes(2), 2, None),
    }
    for what, (t, s, k, so) in bad.items():
        rc, clean, msg = _raw(eng, t, s, k, so)
        assert rc == _lib.KS_EINVAL and clean and msg, what
    with pytest.raises(KsError) as ex:
        eng.place_at(T, shapes(2), np.array([0, 5], np.int32))
    assert ex.value.kind == "InvalidArgument" and "shape" in str(ex.value)
    # the limits themselves are accepted, and junk in an unmasked key is ignored
    rc, clean, _ = _raw(eng, T, shapes(64), 1024, np.arange(1024, dtype=np.int32) % 64)
    assert rc == _lib.KS_OK and not clean
    a = eng.place_at(T, shapes(2, req=np.array([[1000, 5, -1], [1000, 5, 1 << 59]], np.int64)))
    b = eng.place_at(T, shapes(2, req=np.array([[1000, 5, 0]] * 2, np.int64)))
    for f in pr.FIELDS:
        np.testing.assert_array_equal(a[f], b[f])
    # the failed calls changed nothing
    _check(eng, T, r["shapes"], r["shape_of"], r["slow"][T])
    eng.close()
    fm, fl, sc = MODES[pr.FEEDS]
    empty = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    rc, clean, msg = _raw(empty, 0, shapes(2), 2, None)
    assert rc == _lib.KS_EINVAL and clean and "no nodes" in msg
    e0 = z(0, np.uint64)
    empty.load_nodes(z((0, 4), np.int64), e0, e0)
    got = empty.place_at(0, shapes(2), np.array([0, 1, 1], np.int32), after=True)     # n = 0
    assert (got["status"] == pr.NOT_FOUND).all() and (got["node"] == -1).all() and (got["candidates"] == 0).all()
    assert got["info"].tolist() == [0, 0, 0, 3] and got["after"].shape == (0, 4)
    empty.close()
