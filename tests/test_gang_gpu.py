"""GPU parity of the gang admission preview (include/ks_engine.h: ks_gang_at) against tests/gang_ref.py:
the integer chain ``fast_gang`` on the C oracle's binds, and PySim restored on a block on the shared
32-node trace (the two are equal: tests/test_gang_ref.py).  Everything is exact integer equality.

Each reference is built once, checked on its own for the properties that keep the comparison from
passing vacuously before any engine call, and never changed afterwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import drain_ref as dr
import gang_ref as gr
import place_ref as pr
import preview_wide_cases as wc
from harness import MODES, assert_same_binds, encoded, make_engine, shard_ranks, small_trace, step_ranks
from test_consolidate_gpu import _model

pytestmark = pytest.mark.gpu

FEEDS, LITERAL = pr.FEEDS, pr.LITERAL
OK, OVER, NOT_FOUND = pr.OK, pr.OVER, pr.NOT_FOUND
CASE1 = (7, 360, 1200, FEEDS)
CASE_LIT = (7, 360, 1200, LITERAL)
CASE5 = (5, 200, 1200, FEEDS, "five")      # 200 nodes: the queue fills the cluster, gangs are blocked
N_GANGS = 60
MAX_SHAPES, MAX_PODS = 64, 1024        # KS_PLACE_MAX_SHAPES, KS_PLACE_MAX_PODS: a round's limits


@functools.lru_cache(maxsize=None)
def _queue(case, n_gangs=N_GANGS, sizes=tuple(gr.SIZES)):
    return gr.queue_from_trace(_model(*case)["enc"], n_gangs, list(sizes))


@functools.lru_cache(maxsize=None)
def _state(case, t):
    m = _model(*case)
    return pr.state_from_binds(m["tr"], m["enc"], m["ob"], t)


@functools.lru_cache(maxsize=None)
def _ref(case, t, kind="all", n_gangs=N_GANGS, sizes=tuple(gr.SIZES)):
    m = _model(*case)
    shapes, so, first, _ = _queue(case, n_gangs, sizes)
    mo = gr.three_quarters(first) if kind == "partial" else None
    return gr.fast_gang(m["enc"]["alloc"], _state(case, t), m["cfg"], shapes, so, first, mo, strict=kind == "strict")


def _engine(m, **kw):
    eng = make_engine(m["tr"], m["enc"], m["mode"], batch_pods=64, **kw)
    eng.submit(m["enc"]["pods"])
    eb = eng.step(m["T"])
    assert_same_binds(eb, m["ob"])
    return eng


def _check(eng, t, queue, ref, kind="all", what="", rows=True):
    shapes, so, first = queue[:3]
    mo = gr.three_quarters(first) if kind == "partial" else None
    got = eng.gang_at(t, shapes, so, first, min_ok=mo, strict=kind == "strict", rows=rows, after=True)
    gr.assert_same(got, ref, what or f"tick {t} {kind}", rows=rows)
    return got


def _segments(shape_of, first):
    """The rounds ks::gang_segment cuts for a queue without gangs of the single path: a round closes
    before the gang that would bring its 65th distinct shape or its 1,025th pod."""
    segs, shapes, pods = 1, set(), 0
    for g in range(len(first) - 1):
        own = set(int(x) for x in shape_of[first[g]:first[g + 1]])
        size = int(first[g + 1] - first[g])
        assert size <= gr.ROUND
        if len(shapes | own) > MAX_SHAPES or pods + size > MAX_PODS:
            segs, shapes, pods = segs + 1, set(), 0
        shapes |= own
        pods += size
    return segs


@pytest.fixture(scope="module")
def eng360():
    eng = _engine(_model(*CASE1))
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------
# 1. 360 nodes / 1,200 pods: 60 gangs of 575 pods in 372 shapes, the five cases of the recipe
# ---------------------------------------------------------------------------------------------
def test_the_recipe_is_what_the_reference_says():
    shapes, so, first, _ = _queue(CASE1)
    assert len(so) == 575 and len(shapes["keymask"]) == 372 and len(first) == 61
    aon, part, strict, past = (_ref(CASE1, 1200), _ref(CASE1, 1200, "partial"), _ref(CASE1, 1200, "strict"),
                               _ref(CASE1, 700))
    # (the reference alone gives: 48 / 12 with 9 blocked after an Ok pod and the gangs of 33 and 40 pods
    # four times admitted and four times blocked; 56 / 4 with 12 admitted with a failed pod; 7 / 1 / 52;
    # 60 / 0)
    oc, big = aon["outcome"], aon["size"] > gr.ROUND
    assert aon["info"][1] >= 45 and aon["info"][2] >= 10 and ((oc == gr.BLOCKED) & (aon["ok"] >= 1)).sum() >= 7
    assert (big & (oc == gr.ADMITTED)).sum() >= 2 and (big & (oc == gr.BLOCKED)).sum() >= 2 and aon["info"][4] >= 4
    assert part["info"][1] >= 52 and part["info"][2] >= 3
    assert ((part["outcome"] == gr.ADMITTED) & (part["ok"] < part["size"])).sum() >= 10
    assert strict["info"][1] >= 6 and strict["info"][2] == 1 and strict["info"][3] >= 50
    assert past["info"][1] == 60 and past["info"][2] == 0
    lit = _ref(CASE_LIT, 20)
    # (literal mode at t = 20: 10 admitted, 50 blocked on OverCapacity, 14 of them after an Ok pod)
    blocked = lit["outcome"] == gr.BLOCKED
    assert lit["info"][1] >= 8 and blocked.sum() >= 45 and (blocked & (lit["ok"] >= 1)).sum() >= 12
    assert (lit["block_status"][blocked] == OVER).all() and (aon["block_status"][oc == gr.BLOCKED] == NOT_FOUND).all()


@pytest.mark.parametrize("kind", ["all", "partial", "strict"])
def test_the_last_tick(eng360, kind):
    got = _check(eng360, 1200, _queue(CASE1), _ref(CASE1, 1200, kind), kind)
    if kind != "strict":
        assert got["info"][0] >= 6 and got["info"][4] >= 4, got["info"]


def test_a_past_tick_and_summaries_only(eng360):
    m = _model(*CASE1)
    ref = _ref(CASE1, 700)
    later = m["ob"]["tick"] > 700
    assert later.sum() >= 200
    got = _check(eng360, 700, _queue(CASE1), ref)
    np.testing.assert_array_equal(got["after"].sum(axis=0) - eng360.requested_at(700).sum(axis=0),
                                  ref["after"].sum(axis=0) - _state(CASE1, 700).sum(axis=0))
    for t, kind in ((700, "all"), (1200, "partial")):
        plain = _check(eng360, t, _queue(CASE1), _ref(CASE1, t, kind), kind, "summaries only", rows=False)
        assert plain["rows"] is None


def test_literal_mode_blocks_on_over_capacity():
    eng = _engine(_model(*CASE_LIT))
    got = _check(eng, 20, _queue(CASE_LIT), _ref(CASE_LIT, 20))
    assert (got["block_status"][got["outcome"] == gr.BLOCKED] == OVER).all()
    eng.close()


# ---------------------------------------------------------------------------------------------
# 2. the identities against place_at on the same engine
# ---------------------------------------------------------------------------------------------
def _sub(shapes, so, pods):
    """the shapes the pods use, numbered again, and the pods' shape_of among them"""
    used = sorted(set(int(so[j]) for j in pods))
    pos = {s: i for i, s in enumerate(used)}
    return ({f: np.ascontiguousarray(v[used]) for f, v in shapes.items()}, np.array([pos[int(so[j])] for j in pods], np.int32))


def test_gangs_of_one_and_one_open_gang_are_place_at(eng360):
    shapes, so, first, _ = _queue(CASE1)
    k = int(np.nonzero(so >= MAX_SHAPES)[0][0])           # the pods before the 65th shape
    assert 60 <= k <= MAX_PODS
    sh, sof = _sub(shapes, so, range(k))
    for t in (700, 1200):
        want = eng360.place_at(t, sh, sof, after=True)
        assert (want["status"] == OK).sum() >= 30 and (t == 700 or (want["status"] != OK).sum() >= 1)
        ones = eng360.gang_at(t, sh, sof, np.arange(k + 1), min_ok=np.ones(k, np.int32), after=True)
        for f in pr.FIELDS:
            np.testing.assert_array_equal(ones["rows"][f], want[f], err_msg=f"tick {t}: {f}")
        np.testing.assert_array_equal(ones["outcome"], (want["status"] == OK).astype(np.int32))
        np.testing.assert_array_equal(ones["after"], want["after"])
        one = eng360.gang_at(t, sh, sof, [0, k], min_ok=[0], after=True)
        assert one["outcome"].tolist() == [gr.ADMITTED] and one["tried"].tolist() == [k] and one["info"][4] == 1
        for f in pr.FIELDS:
            np.testing.assert_array_equal(one["rows"][f], want[f], err_msg=f"tick {t}, one gang: {f}")
        np.testing.assert_array_equal(one["after"], want["after"])
        assert [int(x) for x in one["info"][1:4]] == [1, 0, 0] and one["info"][5] == want["info"][1]


def test_a_gangs_rows_are_the_tail_of_place_at(eng360):
    shapes, so, first, _ = _queue(CASE1)
    ref = _ref(CASE1, 1200)
    got = eng360.gang_at(1200, shapes, so, first)
    kept, checked = [], {gr.ADMITTED: 0, gr.BLOCKED: 0}
    for g in range(N_GANGS):
        own = list(range(int(first[g]), int(first[g]) + int(ref["tried"][g])))
        pods = kept + own
        if len(pods) > MAX_PODS or len(set(int(so[j]) for j in pods)) > MAX_SHAPES:
            break
        sh, sof = _sub(shapes, so, pods)
        plain = eng360.place_at(1200, sh, sof)
        for f in pr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f][own], plain[f][len(kept):], err_msg=f"gang {g}: {f}")
        checked[int(ref["outcome"][g])] += 1
        if ref["outcome"][g] == gr.ADMITTED:
            kept += own
    assert checked[gr.ADMITTED] >= 5 and checked[gr.BLOCKED] >= 1, checked


# ---------------------------------------------------------------------------------------------
# 3. five shapes: a round's pod boundary, lists used up inside a round
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng_five():
    eng = _engine(_model(*CASE5))
    yield eng
    eng.close()


def test_more_pods_than_a_round_takes(eng_five):
    queue = _queue(CASE5, 300)
    shapes, so, first, _ = queue
    ref = _ref(CASE5, 1200, "all", 300)
    assert len(shapes["keymask"]) == 5 and len(so) > 2 * MAX_PODS
    # (the reference alone gives: 218 admitted, 82 blocked, 42 gangs of the single path, 2,009 Ok pods kept)
    big = ref["size"] > gr.ROUND
    assert ref["info"][1] >= 200 and ref["info"][2] >= 70 and ref["info"][4] >= 40, ref["info"]
    assert (big & (ref["outcome"] == gr.ADMITTED)).sum() >= 5 and (big & (ref["outcome"] == gr.BLOCKED)).sum() >= 5
    got = _check(eng_five, 1200, queue, ref)
    assert got["info"][0] >= 3


def test_lists_used_up_inside_a_round(eng_five):
    small = tuple(s for s in gr.SIZES if s <= gr.ROUND)
    queue = _queue(CASE5, 400, small)
    shapes, so, first, _ = queue
    ref = _ref(CASE5, 1200, "partial", 400, small)
    # (the reference alone gives: 2,226 pods in 3 segments, 359 admitted, 8 of them with a failed pod, 41 blocked)
    assert ref["info"][4] == 0 and ref["info"][1] >= 300 and ref["info"][2] >= 30 and _segments(so, first) == 3, ref["info"]
    got = _check(eng_five, 1200, queue, ref, "partial")
    assert got["info"][0] > _segments(so, first), "only a stop inside a round makes more rounds than segments"


# ---------------------------------------------------------------------------------------------
# 4. a wide cluster: more scan blocks than one trip of the merge folds
# ---------------------------------------------------------------------------------------------
def test_a_wide_cluster_past_one_scan_chunk():
    c = wc.wide_case("b65")
    so = np.concatenate([c["shape_of"][:16], np.full(wc.COPIES, wc.GATED, np.int32), c["shape_of"][16:]]).astype(np.int32)
    first = np.array([0, 16, 16 + wc.COPIES, len(so)], np.int32)
    mo = np.array([8, wc.COPIES, 20], np.int32)
    ref = gr.fast_gang(c["enc"]["alloc"], c["state"][wc.T_WIDE], c["cfg"], c["shapes"], so, first, mo)
    assert c["nblk"] == 65 and ref["info"][4] == 1 and ref["ok"].sum() >= 40, ref["info"]
    nodes = ref["rows"]["node"][ref["rows"]["status"] == OK]
    assert (nodes // wc.BLK >= wc.WAVE).any() and (nodes // wc.BLK < wc.WAVE).any(), "winners on both sides of block 64"
    eng = make_engine(c["tr"], c["enc"], c["mode"], batch_pods=64)
    eng.submit(c["enc"]["pods"])
    assert_same_binds(eng.step(wc.T_WIDE), c["ob"])
    got = eng.gang_at(wc.T_WIDE, c["shapes"], so, first, min_ok=mo, after=True)
    gr.assert_same(got, ref, "b65")
    eng.close()


# ---------------------------------------------------------------------------------------------
# 5. the other engine kinds
# ---------------------------------------------------------------------------------------------
def _parity_ref(case, t, kind="partial"):
    _, pods = gr.parity_queue(case)
    kw = dict(all=dict(), partial=dict(min_ok=gr.PARITY_MIN_OK), strict=dict(min_ok=gr.PARITY_MIN_OK, strict=True))[kind]
    return gr.pysim_gang(dr.sim_at(case, t), t, pods, gr.PARITY_FIRST, **kw)


def _parity_check(eng, case, t, kind="partial", what=""):
    r, _ = gr.parity_queue(case)
    got = eng.gang_at(t, r["shapes"], r["shape_of"], gr.PARITY_FIRST, min_ok=None if kind == "all" else gr.PARITY_MIN_OK,
                      strict=kind == "strict", after=True)
    gr.assert_same(got, _parity_ref(case, t, kind), what or f"{case} tick {t} {kind}")
    return got


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
    shapes, so, first, ids = gr.queue_from_trace(enc, 14)
    pods = pr.sim_pods(shapes, [ps.pods[j] for j in ids])
    mo = gr.three_quarters(first)
    ref = gr.pysim_gang(ps, ps.tick, [pods[j] for j in so], first, mo)
    assert ref["info"][1] >= 2 and ref["info"][2] >= 1 and ref["info"][4] >= 1, ref["info"]
    eng = make_engine(tr, enc, FEEDS, batch_pods=64)
    eng.submit(enc["pods"])
    with pytest.raises(KsError) as ex:
        eng.step(200)
    assert ex.value.kind == "NotFound" and eng.tick == ps.tick
    got = eng.gang_at(eng.tick, shapes, so, first, min_ok=mo, after=True)
    gr.assert_same(got, ref, "aborted run")
    with pytest.raises(KsError):
        eng.gang_at(eng.tick + 1, shapes, so, first)
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
    placed = 0
    for case, e in zip(cases, engs):
        for t in (400, pr.T):
            placed += int(_parity_check(e, case, t, what=f"group member {case} tick {t}")["info"][5])
    assert placed >= 8
    g.close()


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_ranks"])
def test_other_engine_kinds_give_the_same_chain(how):
    from kubesim_amd import _lib
    r = pr.parity_case("feeds")
    refs = {t: _parity_ref("feeds", t) for t in (137, pr.T)}
    assert sum(int(x["info"][5]) for x in refs.values()) >= 4 and any(x["info"][2] for x in refs.values())
    if how == "two_ranks":
        engs, x = shard_ranks(r["tr"], r["enc"], 2, 1, batch_pods=64)
        step_ranks(engs, pr.T, x)
    else:
        eng = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64, engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER)
        eng.submit(r["enc"]["pods"])
        eng.step(pr.T)
        engs = [eng]
    for t in refs:
        for rank, eng in enumerate(engs):
            _parity_check(eng, "feeds", t, what=f"{how} rank {rank} tick {t}")
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
    for t in (1, 137, 400):
        for kind in ("all", "partial", "strict"):
            _parity_check(eng, "feeds", t, kind)
    np.testing.assert_array_equal(eng.requested_at(400), twin.requested_at(400))
    nb, ntb = eng.step(400), twin.step(400)
    assert len(nb) >= 100
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    np.testing.assert_array_equal(eng.requested_at(800), twin.requested_at(800))
    _parity_check(eng, "feeds", 800, what="tick 800 after stepping on")
    eng.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# 6. errors on a live engine: nothing is written
# ---------------------------------------------------------------------------------------------
def _raw(eng, t, shapes, so, first, min_ok=None, flags=0, ns=None, k=None, m=None, null=()):
    """ks_gang_at itself on sentinel-filled outputs: (status, outputs untouched, ks_last_error)."""
    from kubesim_amd import _lib
    from kubesim_amd.engine import GANG_DTYPE, PLACEMENT_DTYPE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    a = dict(req=np.ascontiguousarray(shapes["req"], np.int64), keymask=np.ascontiguousarray(shapes["keymask"], np.uint8),
             tol=np.ascontiguousarray(shapes["tol"], np.uint64), sel=np.ascontiguousarray(shapes["sel"], np.uint64),
             shape_of=np.ascontiguousarray(so, np.int32), first=np.ascontiguousarray(first, np.int32))
    mo = None if min_ok is None else np.ascontiguousarray(min_ok, np.int32)
    out = np.full(max(len(a["first"]), 2) * GANG_DTYPE.itemsize, 0x5A, np.uint8)
    rows = np.full(max(len(a["shape_of"]), 1) * PLACEMENT_DTYPE.itemsize, 0x5A, np.uint8)
    aft = np.full(eng.n * 4 + 4, 0x5A5A, np.int64)
    info = np.full(_lib.KS_GANG_INFO, 0x5A5A, np.int64)
    arg = lambda f: None if f in null else p(a[f])
    rc = eng._L.ks_gang_at(eng.h, t, len(a["keymask"]) if ns is None else ns, arg("req"), arg("keymask"), arg("tol"),
                           arg("sel"), len(a["shape_of"]) if k is None else k, arg("shape_of"),
                           len(a["first"]) - 1 if m is None else m, arg("first"), None if mo is None else p(mo), flags,
                           None if "out" in null else p(out), p(rows), p(aft), p(info))
    clean = bool((out == 0x5A).all() and (rows == 0x5A).all() and (aft == 0x5A5A).all() and (info == 0x5A5A).all())
    return rc, clean, eng._L.ks_last_error(eng.h).decode()


def test_argument_errors_write_nothing():
    from kubesim_amd import _lib
    from kubesim_amd.engine import Engine, KsError
    r = pr.parity_case("feeds")
    eng = make_engine(r["tr"], r["enc"], FEEDS, batch_pods=64)
    eng.submit(r["enc"]["pods"])
    eng.step(400)
    sh, so, first = r["shapes"], r["shape_of"], gr.PARITY_FIRST
    junk = {f: v.copy() for f, v in sh.items()}
    junk["keymask"][3] = 8
    neg = {f: v.copy() for f, v in sh.items()}
    neg["req"][4, 0] = -5
    many = {f: np.ascontiguousarray(np.resize(v, (_lib.KS_GANG_MAX_SHAPES + 1,) + v.shape[1:])) for f, v in sh.items()}
    bad = {
        "tick past the current one": dict(t=401),
        "negative tick": dict(t=-1),
        "a shape out of range": dict(so=np.where(np.arange(48) == 7, 12, so)),
        "a negative shape": dict(so=np.where(np.arange(48) == 7, -1, so)),
        "keymask bits above 4": dict(shapes=junk),
        "a negative request": dict(shapes=neg),
        "no shapes": dict(ns=0),
        "too many shapes": dict(shapes=many),
        "no pods": dict(k=0),
        "too many pods": dict(k=_lib.KS_GANG_MAX_PODS + 1),
        "no gangs": dict(m=0),
        "too many gangs": dict(m=_lib.KS_GANG_MAX_GANGS + 1),
        "first does not start at 0": dict(first=np.concatenate([[1], first[1:]])),
        "first decreases": dict(first=np.concatenate([first[:5], [first[5] - 9], first[6:]])),
        "first does not end at k": dict(first=np.concatenate([first[:-1], [47]])),
        "min_ok above the size": dict(min_ok=np.where(np.arange(12) == 2, 5, gr.PARITY_MIN_OK)),
        "negative min_ok": dict(min_ok=np.where(np.arange(12) == 2, -1, gr.PARITY_MIN_OK)),
        "an unknown flag": dict(flags=2),
        "shape_of NULL": dict(null=("shape_of",)),
        "first NULL": dict(null=("first",)),
        "out NULL": dict(null=("out",)),
        "req NULL": dict(null=("req",)),
        "keymask NULL": dict(null=("keymask",)),
        "tol NULL": dict(null=("tol",)),
        "sel NULL": dict(null=("sel",)),
    }
    quiet = ("shape_of NULL", "first NULL", "out NULL", "req NULL", "keymask NULL", "tol NULL", "sel NULL")
    for what, kw in bad.items():
        args = dict(dict(t=400, shapes=sh, so=so, first=first, min_ok=gr.PARITY_MIN_OK), **kw)
        rc, clean, msg = _raw(eng, **args)
        assert rc == _lib.KS_EINVAL and clean, what
        if what not in quiet:
            assert msg, what
    with pytest.raises(KsError) as ex:
        eng.gang_at(400, sh, so, first, min_ok=np.full(12, 13))
    assert ex.value.kind == "InvalidArgument" and "min_ok" in str(ex.value)
    rc, clean, _ = _raw(eng, 400, sh, so, first, gr.PARITY_MIN_OK, flags=_lib.KS_GANG_STRICT)
    assert rc == _lib.KS_OK and not clean
    # as many shapes as a call takes, far more than a round does
    wide = {f: np.ascontiguousarray(np.resize(v, (_lib.KS_GANG_MAX_SHAPES,) + v.shape[1:])) for f, v in sh.items()}
    got = eng.gang_at(400, wide, so + 12 * (np.arange(48) % 300), first, min_ok=gr.PARITY_MIN_OK, after=True)
    gr.assert_same(got, _parity_ref("feeds", 400), "4,096 shapes")
    fm, fl, sc = MODES[FEEDS]
    empty = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    rc, clean, msg = _raw(empty, 0, sh, so, first)
    assert rc == _lib.KS_EINVAL and clean and "no nodes" in msg
    z = np.zeros(0, np.uint64)
    empty.load_nodes(np.zeros((0, 4), np.int64), z, z)       # n = 0: every pod is not found
    got = empty.gang_at(0, sh, so, first, min_ok=gr.PARITY_MIN_OK, after=True)
    want = gr.fast_gang(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), dict(pr.engine_cfg(MODES[FEEDS], r["enc"]), taint=z, label=z),
                        sh, so, first, gr.PARITY_MIN_OK)
    assert want["info"][1] == 2 and want["info"][2] == 10    # (the empty gang and the one with min_ok = 0)
    gr.assert_same(got, want, "no node")
    empty.close()
    eng.close()
