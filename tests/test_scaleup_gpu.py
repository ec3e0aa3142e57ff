"""GPU parity of the scale-up preview (include/ks_engine.h: ks_scale_up_at) against
tests/scaleup_ref.py — the placement reference on the cluster with the option's nodes appended — and,
through existing code, against ks_place_at on a twin engine that has the nodes for real.  Everything
is exact integer equality.

Each reference is built once, checked on its own for the properties that keep the comparison from
passing vacuously before any engine call, and never changed afterwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import place_ref as pr
import scaleup_ref as sr
from harness import MODES, assert_same_binds, encoded, make_engine, small_trace

pytestmark = pytest.mark.gpu

GI = (1 << 30) * 1000          # a gibibyte in milli-units
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _check(eng, t, shapes, shape_of, opts, want, what=""):
    got = eng.scale_up_at(t, shapes, opts, shape_of, rows=True)
    sr.assert_same(got, want, what=what or f"tick {t}")
    assert int(got["info"][3]) == len(shapes["keymask"])
    # the summaries alone are the same
    lean = eng.scale_up_at(t, shapes, opts, shape_of)
    assert lean["rows"] is None
    for f in sr.SUMMARY + ("path",):
        np.testing.assert_array_equal(lean[f], got[f])
    return got


def _hand_engine(alloc, mode, taint=None, label=None):
    """an engine on a hand-made cluster, never stepped: tick 0, nothing running"""
    from kubesim_amd.engine import Engine
    fm, fl, sc = mode
    n = len(alloc)
    e = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    e.load_nodes(np.array(alloc, np.int64).reshape(-1, 4), np.zeros(n, np.uint64) if taint is None else taint,
                 np.zeros(n, np.uint64) if label is None else label)
    return e


def _hand_ref(alloc, mode, shapes, shape_of, opts, taint=None, label=None):
    n = len(alloc)
    fm, fl, sc = mode
    cfg = dict(filter_mode=fm, filters=fl, scorers=sc, taint=np.zeros(n, np.uint64) if taint is None else taint,
               label=np.zeros(n, np.uint64) if label is None else label)
    return sr.scale_up(np.array(alloc, np.int64).reshape(-1, 4), np.zeros((n, 4), np.int64), cfg, shapes, shape_of, opts)


def _one_shape(cpu, mem, k, gpu=0, keymask=3, tol=0):
    return (dict(req=np.array([[cpu, mem, gpu]], np.int64), keymask=np.array([keymask], np.uint8),
                 tol=np.array([tol], np.uint64), sel=np.zeros(1, np.uint64)), np.zeros(k, np.int32))


# ---------------------------------------------------------------------------------------------
# 1. 300 nodes (two scan blocks, a ragged tail), 600 pods, one batched step
# ---------------------------------------------------------------------------------------------
_engines = {}


def _run300(mode):
    """the model's trace on the engine, one batched step to T300; one engine per mode and module"""
    if mode in _engines:
        return _engines[mode]
    m = sr.model_300(mode)
    eng = make_engine(m["tr"], m["enc"], m["mode"], batch_pods=64)
    eng.submit(m["enc"]["pods"])
    eb = eng.step(sr.T300)
    assert eng.last_step_stats()["launches"] > 10
    assert_same_binds(eb, m["ob"])
    for t in sr.TICKS300:
        np.testing.assert_array_equal(eng.requested_at(t), m["states"][t])
    _engines[mode] = eng
    return eng


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()


@pytest.mark.parametrize("mode", ["feeds", "literal"])
def test_parity_48_pods_6_shapes_5_options_at_three_ticks(mode):
    m = sr.model_300(mode)
    n = sr.N300
    refs = m["refs"]
    # on the reference alone
    if mode == "feeds":
        assert all(sum(w["summary"]["on_new"] > 0 for w in refs[t]) >= 3 for t in sr.TICKS300)
        assert all(refs[t][1]["summary"]["on_new"] == 6 and refs[t][1]["summary"]["nodes_used"] == 3 for t in sr.TICKS300), \
            "the two-pod nodes did not run out"
        assert any(len(set(w["candidates"].tolist())) >= 3 for w in refs[400])
    else:
        assert all((w["candidates"] == n + o["max_nodes"]).all() for t in sr.TICKS300 for o, w in zip(m["opts"], refs[t]))
        assert all(w["summary"]["over_capacity"] >= 5 for t in sr.TICKS300 for w in refs[t])
    assert all((w["node"] < n).any() for t in sr.TICKS300 for w in refs[t])
    eng = _run300(mode)
    for t in sr.TICKS300:
        got = _check(eng, t, m["shapes"], m["shape_of"], m["opts"], refs[t], f"{mode} tick {t}")
        assert (got["path"] == 0).all(), "48 pods of 6 shapes cannot use up a 32-entry list"


def test_no_appended_node_is_place_at():
    m = sr.model_300("feeds")
    eng = _run300("feeds")
    for t in sr.TICKS300:
        want = eng.place_at(t, m["shapes"], m["shape_of"])
        got = eng.scale_up_at(t, m["shapes"], [m["opts"][3]], m["shape_of"], rows=True)
        assert m["opts"][3]["max_nodes"] == 0
        for f in sr.ROWS:
            np.testing.assert_array_equal(got["rows"][f][0], want[f], err_msg=f"tick {t}: {f}")
        assert got["on_new"][0] == 0 and got["ok"][0] == want["info"][1]


def test_twin_engine_with_the_nodes_for_real_places_alike():
    """Through existing code: a twin loads the cluster plus the option's nodes behind a taint no trace
    pod tolerates, makes the same binds, and its ks_place_at for pods that do tolerate it is the
    answer ks_scale_up_at must give for that template — row for row, candidates included."""
    m = sr.model_300("feeds")
    enc, n = m["enc"], sr.N300
    fence = np.uint64(sr.FENCE)
    for opt in (dict(m["opts"][0], taint=sr.FENCE), dict(m["opts"][1], taint=sr.FENCE),
                sr.option([int(x) for x in enc["alloc"][7]], 6, sr.FENCE, int(enc["label"][7]))):   # a node of the cluster's own
        M = opt["max_nodes"]
        tenc = dict(enc)
        tenc["alloc"] = np.concatenate([enc["alloc"], np.tile(np.array(opt["alloc"], np.int64), (M, 1))])
        tenc["taint"] = np.concatenate([np.asarray(enc["taint"], np.uint64), np.full(M, opt["taint"], np.uint64)])
        tenc["label"] = np.concatenate([np.asarray(enc["label"], np.uint64), np.full(M, opt["label"], np.uint64)])
        twin = make_engine(m["tr"], tenc, m["mode"], batch_pods=64)
        twin.submit(enc["pods"])
        assert_same_binds(twin.step(sr.T300), m["ob"])
        shapes = dict(m["shapes"])
        shapes["tol"] = np.asarray(m["shapes"]["tol"], np.uint64) | fence
        eng = _run300("feeds")
        for t in sr.TICKS300:
            want = twin.place_at(t, shapes, m["shape_of"])
            got = eng.scale_up_at(t, shapes, [opt], m["shape_of"], rows=True)
            for f in sr.ROWS:
                np.testing.assert_array_equal(got["rows"][f][0], want[f], err_msg=f"{opt['alloc']} tick {t}: {f}")
            assert got["on_new"][0] == int(((want["node"] >= n) & (want["status"] == 0)).sum())
        twin.close()
    # (the first two templates put pods on the new nodes: seen on the reference in the parity test)


def test_template_no_shape_can_use():
    m = sr.model_300("feeds")
    eng = _run300("feeds")
    a = m["enc"]["alloc"]
    big = m["opts"][0]
    # (the second asks for more gpu than any node of the cluster has)
    gpu_pods = dict(req=np.array([[1000, GI, 1000], [500, GI, int(a[:, 2].max()) + 1000]], np.int64), keymask=np.array([7, 7], np.uint8),
                    tol=np.array([ALL, ALL]), sel=np.zeros(2, np.uint64))
    so = (np.arange(20) % 2).astype(np.int32)
    cases = {
        "a taint nobody tolerates": (m["shapes"], m["shape_of"], dict(big, taint=sr.FENCE)),
        "no gpu key for gpu pods": (gpu_pods, so, dict(big, alloc=big["alloc"][:2] + [-1, 110])),
    }
    assert (a[:, 2] > 0).any()
    for what, (shapes, shape_of, opt) in cases.items():
        want = eng.place_at(400, shapes, shape_of)
        assert (want["status"] == pr.OK).any(), what
        got = eng.scale_up_at(400, shapes, [opt], shape_of, rows=True)
        for f in sr.ROWS:
            np.testing.assert_array_equal(got["rows"][f][0], want[f], err_msg=f"{what}: {f}")
        assert got["on_new"][0] == 0 and got["nodes_used"][0] == 0 and got["path"][0] == 0, what
    # ... and the gpu pods do use a template that has the key
    with_gpu = [dict(big, alloc=[big["alloc"][0], big["alloc"][1], 64000, 110])]
    want = sr.scale_up(a, m["states"][400], m["cfg"], gpu_pods, so, with_gpu)
    assert want[0]["summary"]["on_new"] > 0
    _check(eng, 400, gpu_pods, so, with_gpu, want, "a template with the gpu key")


def test_milli_route_beside_the_whole_unit_route():
    """A template capacity that is no multiple of the engine's unit sends the whole call through
    milli-units; the whole-unit option beside it must come out as it does alone (device units)."""
    m = sr.model_300("feeds")
    eng = _run300("feeds")
    whole, odd = m["opts"][0], m["opts"][4]
    from math import gcd
    unit = 0
    for v in list(m["enc"]["alloc"][:, 1]) + list(m["enc"]["pods"]["req"][:, 1]):
        unit = gcd(unit, int(v)) if v > 0 else unit
    assert unit > 1 and odd["alloc"][1] % unit and whole["alloc"][1] % unit == 0
    assert all(int(q) % unit == 0 for q in m["shapes"]["req"][:, 1])
    ref = m["refs"][400]
    alone = eng.scale_up_at(400, m["shapes"], [whole], m["shape_of"], rows=True)
    both = eng.scale_up_at(400, m["shapes"], [whole, odd], m["shape_of"], rows=True)
    sr.assert_same(alone, [ref[0]], what="whole units")
    sr.assert_same(both, [ref[0], ref[4]], what="milli-units")
    assert ref[4]["summary"]["on_new"] > 0
    # an odd request does the same to the whole-unit template
    shapes = {f: v.copy() for f, v in m["shapes"].items()}
    shapes["req"][2, 1] += 1
    want = sr.scale_up(m["enc"]["alloc"], m["states"][400], m["cfg"], shapes, m["shape_of"], [whole])
    _check(eng, 400, shapes, m["shape_of"], [whole], want, "an odd request")


@functools.lru_cache(maxsize=None)
def _many():
    """64 options x 1,024 pods of 8 shapes at the last tick"""
    m = sr.model_300("feeds")
    enc = m["enc"]
    ids = sr.distinct_pods(enc, 8, start=100)
    shapes = {f: np.ascontiguousarray(enc["pods"][f][ids]) for f in ("req", "keymask", "tol", "sel")}
    shape_of = ((np.arange(1024) * 5) % 8).astype(np.int32)
    shape_of[512:] = (np.arange(512) // 64) % 8            # alternating, then runs
    big = m["opts"][0]["alloc"]
    labels = m["opts"][0]["label"]
    opts = []
    for g in range(64):
        alloc = [big[0] // (1 + g % 4), big[1] // (1 + g % 3), big[2], [110, 110, 3, 1][g % 4]]
        if g % 16 == 5:
            alloc[0] += 1                                  # (one odd capacity: the call runs in milli-units)
        opts.append(sr.option(alloc, [0, 1, 2, 5, 17, 60, 200, 1024][g % 8], 0 if g % 5 else 0x3, labels))
    refs = sr.scale_up(enc["alloc"], m["states"][sr.T300], m["cfg"], shapes, shape_of, opts)
    return shapes, shape_of, opts, refs


def test_64_options_of_1024_pods_of_8_shapes():
    shapes, shape_of, opts, refs = _many()
    used = [w["summary"]["nodes_used"] for w in refs]
    assert len(set(used)) >= 8 and max(used) >= 100 and min(used) == 0
    assert len({w["summary"]["ok"] for w in refs}) >= 3
    got = _check(_run300("feeds"), sr.T300, shapes, shape_of, opts, refs, "64 x 1024")
    assert got["info"][0] >= 1 and got["info"][1] >= 1, "one of the two paths was never taken"


# ---------------------------------------------------------------------------------------------
# 2. hand-made clusters, never stepped
# ---------------------------------------------------------------------------------------------
FIT_LR = (1, 1, ((1, 1, 0),))          # the fit filter feeds LeastRequested
LIT_LR = (0, 1, ((1, 1, 0),))
NODE = [16000, 64 * GI, 0, 110]


def test_single_path_is_reached_on_purpose():
    """40 copies of one shape under LeastRequested on 100 equal nodes: every copy lowers its node's
    score, so each takes the next list entry and pod 33 finds all 32 flagged — the option without
    nodes stops there and is answered by the rounds; a template that scores higher takes every pod."""
    from kubesim_amd import _lib
    alloc = [NODE] * 100
    shapes, so = _one_shape(4000, 16 * GI, 40)
    opts = [sr.option(NODE, 0), sr.option([32000, 128 * GI, 0, 110], 50)]
    want = _hand_ref(alloc, FIT_LR, shapes, so, opts)
    assert want[0]["node"].tolist() == list(range(40)) and want[1]["summary"]["on_new"] == 40
    eng = _hand_engine(alloc, FIT_LR)
    got = _check(eng, 0, shapes, so, opts, want)
    assert got["path"].tolist() == [_lib.KS_SCALEUP_PATH_SINGLE, _lib.KS_SCALEUP_PATH_BATCHED]
    assert got["info"].tolist() == [1, 1, 2, 1]
    # 32 copies use up no list
    got = eng.scale_up_at(0, shapes, opts[:1], so[:32])
    assert got["path"].tolist() == [0] and got["info"].tolist() == [1, 0, 1, 1]
    # the single path with appended nodes: equal nodes appended, which the rounds must scan as well
    opts = [sr.option(NODE, 30), sr.option(NODE, 0)]
    shapes, so = _one_shape(4000, 16 * GI, 120)
    want = _hand_ref(alloc, FIT_LR, shapes, so, opts)
    assert want[0]["node"][100:].tolist() == list(range(100, 120)) and want[0]["summary"]["nodes_used"] == 20
    got = _check(eng, 0, shapes, so, opts, want)
    assert got["path"].tolist() == [1, 1]
    eng.close()


@pytest.mark.parametrize("mode", [FIT_LR, LIT_LR], ids=["feeds", "literal"])
def test_two_small_appended_nodes_fill_up(mode):
    alloc = [[4000, 16 * GI, 0, 1]] * 3
    shapes, so = _one_shape(1000, 4 * GI, 12)
    opts = [sr.option([16000, 64 * GI, 0, 2], 2)]
    want = _hand_ref(alloc, mode, shapes, so, opts)
    w = want[0]
    # fresh, fresh, then back through the changed set (score 8 on a node with one pod or two)
    assert w["node"][:3].tolist() == [3, 4, 3] and w["score"][:4].tolist() == [9, 9, 8, 8]
    if mode is FIT_LR:
        # node 3 is full after its second pod: node 4, then the real nodes, then nothing fits
        assert w["node"][3:].tolist() == [4, 0, 1, 2] + [-1] * 5 and w["summary"]["not_found"] == 5
        assert w["candidates"].tolist() == [5, 5, 5, 4, 3, 2, 1] + [0] * 5
    else:
        # the filters gate nothing: the full node 3 ties with node 4 at 8 and wins again and again
        assert (w["node"][3:] == 3).all() and w["summary"]["over_capacity"] == 9 and (w["candidates"] == 5).all()
    eng = _hand_engine(alloc, mode)
    got = _check(eng, 0, shapes, so, opts, want)
    assert got["nodes_used"][0] == 2
    assert (got["on_new"][0], got["first_unplaced"][0]) == ((4, 7) if mode is FIT_LR else (3, 3))
    eng.close()


@pytest.mark.parametrize("mode", [(1, 7, ((0, 2, 3),)), (0, 7, ((0, 2, 3),))], ids=["feeds", "literal"])
def test_constant_scorers_never_choose_an_appended_node(mode):
    alloc = [NODE] * 300
    shapes, so = _one_shape(4000, 16 * GI, 64)
    opts = [sr.option([64000, 256 * GI, 0, 110], 9), sr.option(NODE, 1)]
    want = _hand_ref(alloc, mode, shapes, so, opts)
    assert all((w["node"] < 300).all() and w["summary"]["on_new"] == 0 for w in want)
    assert (want[0]["candidates"][:4] == 309).all() and (want[0]["score"] == 6).all()
    eng = _hand_engine(alloc, mode)
    _check(eng, 0, shapes, so, opts, want)
    eng.close()


def test_no_real_node_at_all():
    from kubesim_amd.engine import Engine
    e = Engine(tick_seconds=10, filter_mode=1, filters=7, scorers=FIT_LR[2])
    z = np.zeros(0, np.uint64)
    e.load_nodes(np.zeros((0, 4), np.int64), z, z)
    shapes, so = _one_shape(4000, 16 * GI, 10)
    opts = [sr.option(NODE, 0), sr.option([8000, 32 * GI, 0, 110], 3), sr.option([8000, 32 * GI + 1, 0, 1], 300)]
    cfg = dict(filter_mode=1, filters=7, scorers=FIT_LR[2], taint=z, label=z)
    want = sr.scale_up(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), cfg, shapes, so, opts)
    assert [w["summary"]["ok"] for w in want] == [0, 6, 10] and want[2]["node"].tolist() == list(range(10))
    got = _check(e, 0, shapes, so, opts, want, "n = 0")
    assert got["path"].tolist() == [1, 1, 1] and got["info"].tolist() == [0, 3, 1, 1]
    e.close()


# ---------------------------------------------------------------------------------------------
# 3. engine kinds, on the shared 32-node trace of tests/place_ref.py
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case32(case):
    r = pr.parity_case(case)
    opts = sr.trace_options(r["enc"])
    cfg = pr.engine_cfg(MODES[r["mode"]], r["enc"])
    refs = {t: sr.scale_up(r["enc"]["alloc"], sr.state_before(r["fast"][t], r["shapes"], r["shape_of"]), cfg, r["shapes"],
                           r["shape_of"], opts) for t in (1, 137, pr.T)}
    assert any(w["summary"]["on_new"] > 0 for t in refs for w in refs[t])
    return r, opts, refs


def _same_binds(eb, binds):
    assert_same_binds(eb, dict(pod=binds[:, 0], node=binds[:, 1], tick=binds[:, 2], status=binds[:, 3]))


@pytest.mark.parametrize("how", ["one_pod_resolver", "two_node_shards"])
def test_other_engine_kinds_give_the_same_preview(how):
    from kubesim_amd import _lib
    r, opts, refs = _case32("feeds")
    kw = dict(engine_flags=_lib.KS_ENGINE_ONE_POD_RESOLVER) if how == "one_pod_resolver" else dict(shard=(1, 0, None, 2))
    eng = make_engine(r["tr"], r["enc"], pr.FEEDS, batch_pods=64, **kw)
    eng.submit(r["enc"]["pods"])
    _same_binds(eng.step(pr.T), r["binds"])
    for t in refs:
        _check(eng, t, r["shapes"], r["shape_of"], opts, refs[t], f"{how} tick {t}")
    eng.close()


def test_group_members_answer_for_their_own_scenario():
    from kubesim_amd.engine import Group
    g = Group(2)
    cases = ("feeds", "feeds_irregular")
    engs = []
    for case in cases:
        r, _, _ = _case32(case)
        fm, fl, sc = MODES[pr.FEEDS]
        e = g.add(tick_seconds=r["tr"]["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc, batch_pods=64)
        e.load_nodes(r["enc"]["alloc"], r["enc"]["taint"], r["enc"]["label"])
        e.submit(r["enc"]["pods"])
        engs.append(e)
    binds, counts, st, _ = g.step(pr.T)
    assert (st == 0).all()
    for case, e, eb in zip(cases, engs, g.split(binds, counts)):
        r, opts, refs = _case32(case)
        _same_binds(eb, r["binds"])
        for t in refs:
            _check(e, t, r["shapes"], r["shape_of"], opts, refs[t], f"group member {case} tick {t}")
    g.close()


def test_engine_without_scorers_finds_no_node():
    r, opts, _ = _case32("feeds")
    eng = make_engine(r["tr"], r["enc"], "no_scorers")
    got = eng.scale_up_at(0, r["shapes"], opts, r["shape_of"], rows=True)
    assert (got["rows"]["status"] == pr.NOT_FOUND).all() and (got["rows"]["node"] == -1).all()
    assert (got["rows"]["candidates"] == 0).all() and (got["rows"]["score"] == -1).all()
    assert (got["not_found"] == pr.N_PODS).all() and (got["first_unplaced"] == 0).all() and (got["on_new"] == 0).all()
    assert got["info"].tolist() == [5, 0, 0, 12]
    eng.close()


def test_preview_after_an_aborted_run():
    from kubesim_amd.engine import KsError
    from pysim import RES, PySim
    tr = small_trace(9)   # 15 binds, then a pod whose selector no node carries
    enc = encoded(tr)
    fm, fl, sc = MODES[pr.FEEDS]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    binds, err = ps.step(200)
    assert err == "NotFound" and len(binds) >= 8
    stopped = len(binds)
    eng = make_engine(tr, enc, pr.FEEDS, batch_pods=64)
    eng.submit(enc["pods"])
    with pytest.raises(KsError) as ex:
        eng.step(200)
    assert ex.value.kind == "NotFound" and eng.tick == ps.tick
    t = ps.tick
    state = np.zeros((ps.n, 4), np.int64)
    for nd in range(ps.n):
        tot = ps._total_request(nd, t)
        state[nd, :3] = [tot.get(x, 0) for x in RES]
        state[nd, 3] = ps._running_num(nd, t)
    np.testing.assert_array_equal(eng.requested_at(t), state)
    ids = [stopped, 0, stopped, 3, 5, 0]
    shapes = {f: np.ascontiguousarray(enc["pods"][f][ids]) for f in ("req", "keymask", "tol", "sel")}
    a = enc["alloc"]
    opts = [sr.option([4 * int(a[:, 0].max()), 4 * int(a[:, 1].max()), int(a[:, 2].max()), 110], 4, 0, int(enc["pods"]["sel"][stopped])),
            sr.option([int(x) for x in a[0]], 2)]
    want = sr.scale_up(a, state, pr.engine_cfg(MODES[pr.FEEDS], enc), shapes, None, opts)
    # the pod the run stopped at finds a node only where the template carries its labels
    assert want[0]["status"][0] == pr.OK and want[0]["node"][0] >= ps.n and want[1]["status"][0] == pr.NOT_FOUND
    _check(eng, t, shapes, None, opts, want, "after the abort")
    with pytest.raises(KsError):
        eng.scale_up_at(t + 1, shapes, opts)
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. argument errors, and no side effects
# ---------------------------------------------------------------------------------------------
def _raw(eng, t, shapes, k, shape_of, opt, n_options=None):
    """ks_scale_up_at itself on sentinel-filled outputs: (status, outputs untouched, ks_last_error)."""
    from kubesim_amd.engine import PLACEMENT_DTYPE
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    req = np.ascontiguousarray(shapes["req"], np.int64)
    km, tol, sel = (np.ascontiguousarray(shapes[f], d) for f, d in (("keymask", np.uint8), ("tol", np.uint64), ("sel", np.uint64)))
    m = len(opt) if n_options is None else n_options
    out = np.full(max(m, 1) * 32 + 64, 0x5A, np.uint8)
    rows = np.full(max(m, 1) * max(k, 1) * PLACEMENT_DTYPE.itemsize + 64, 0x5A, np.uint8)
    info = np.full(4, 0x5A5A, np.int64)
    so = None if shape_of is None else np.ascontiguousarray(shape_of, np.int32)
    rc = eng._L.ks_scale_up_at(eng.h, t, len(km), p(req), p(km), p(tol), p(sel), k, None if so is None else p(so), m, p(opt),
                               p(out), p(rows), p(info))
    clean = bool((out == 0x5A).all() and (rows == 0x5A).all() and (info == 0x5A5A).all())
    return rc, clean, eng._L.ks_last_error(eng.h).decode()


def test_argument_errors_and_no_side_effects():
    from kubesim_amd import _lib
    from kubesim_amd.engine import SCALE_OPTION_DTYPE, Engine, KsError
    r, opts32, refs = _case32("feeds")
    T = pr.T

    def run():
        e = make_engine(r["tr"], r["enc"], pr.FEEDS, batch_pods=64)
        e.submit(r["enc"]["pods"])
        return e, e.step(400)
    eng, eb = run()
    twin, tb = run()       # makes no scale-up call

    def shapes(k, **over):
        s = dict(req=np.tile(np.array([[1000, 1 << 30, 0]], np.int64), (k, 1)), keymask=np.full(k, 3, np.uint8),
                 tol=np.full(k, ALL), sel=np.zeros(k, np.uint64))
        s.update(over)
        return s

    def option(n=1, **over):
        o = np.zeros(n, SCALE_OPTION_DTYPE)
        o["alloc"] = [16000, 64 * GI, -1, 110]
        o["max_nodes"] = 4
        for f, v in over.items():
            o[f][n - 1] = v
        return o
    z = np.zeros
    TOP = 1 << 59
    bad = {
        "no shapes": (400, shapes(0), 1, z(1, np.int32), option()),
        "65 shapes": (400, shapes(65), 1, z(1, np.int32), option()),
        "no pods": (400, shapes(2), 0, z(1, np.int32), option()),
        "1025 pods": (400, shapes(2), 1025, z(1025, np.int32), option()),
        "shape_of = n_shapes": (400, shapes(2), 3, np.array([0, 2, 1], np.int32), option()),
        "shape_of = -1": (400, shapes(2), 3, np.array([0, 1, -1], np.int32), option()),
        "NULL shape_of, k != n_shapes": (400, shapes(2), 3, None, option()),
        "keymask 8": (400, shapes(2, keymask=np.array([3, 8], np.uint8)), 2, None, option()),
        "negative masked request": (400, shapes(2, req=np.array([[1000, 5, 0], [-1, 5, 0]], np.int64)), 2, None, option()),
        "masked request of 2^59": (400, shapes(2, req=np.array([[1000, 5, 0], [1000, TOP, 0]], np.int64)), 2, None, option()),
        "tick past the current one": (401, shapes(2), 2, None, option()),
        "negative tick": (-1, shapes(2), 2, None, option()),
        "max_nodes -1": (400, shapes(2), 2, None, option(2, max_nodes=-1)),
        "max_nodes 65537": (400, shapes(2), 2, None, option(3, max_nodes=65537)),
        "alloc -2": (400, shapes(2), 2, None, option(2, alloc=[16000, -2, -1, 110])),
        "alloc 2^59": (400, shapes(2), 2, None, option(2, alloc=[TOP, 64 * GI, -1, 110])),
        "gpu alloc 2^59": (400, shapes(2), 2, None, option(1, alloc=[16000, 64 * GI, TOP, 110])),
        "pods -1": (400, shapes(2), 2, None, option(2, alloc=[16000, 64 * GI, -1, -1])),
        "pad 1": (400, shapes(2), 2, None, option(2, pad=1)),
    }
    for what, (t, s, k, so, opt) in bad.items():
        rc, clean, msg = _raw(eng, t, s, k, so, opt)
        assert rc == _lib.KS_EINVAL and clean and msg, what
    for m in (0, 65, -1):
        rc, clean, msg = _raw(eng, 400, shapes(2), 2, None, option(65), n_options=m)
        assert rc == _lib.KS_EINVAL and clean and "options" in msg, m
    with pytest.raises(KsError) as ex:
        eng.scale_up_at(400, shapes(2), [sr.option([1, 1, 1, 1], 70000)])
    assert ex.value.kind == "InvalidArgument" and "max_nodes" in str(ex.value)
    # the limits themselves are accepted
    lim = option(64, max_nodes=65536, alloc=[TOP - 1, TOP - 1, TOP - 1, TOP - 1])
    lim["max_nodes"][0] = 0
    rc, clean, _ = _raw(eng, 400, shapes(64), 1024, np.arange(1024, dtype=np.int32) % 64, lim)
    assert rc == _lib.KS_OK and not clean
    fm, fl, sc = MODES[pr.FEEDS]
    empty = Engine(tick_seconds=10, filter_mode=fm, filters=fl, scorers=sc)
    rc, clean, msg = _raw(empty, 0, shapes(2), 2, None, option())
    assert rc == _lib.KS_EINVAL and clean and "no nodes" in msg
    empty.close()
    # the calls changed nothing: the previews read as before and the run goes on as its twin's
    _check(eng, 137, r["shapes"], r["shape_of"], opts32, refs[137])
    np.testing.assert_array_equal(eng.requested_at(400), twin.requested_at(400))
    nb, ntb = eng.step(T - 400), twin.step(T - 400)
    for f in ("pod", "node", "status", "tick"):
        np.testing.assert_array_equal(nb[f], ntb[f])
    _same_binds(np.concatenate([eb, nb]), r["binds"])
    _check(eng, T, r["shapes"], r["shape_of"], opts32, refs[T])
    _check(twin, T, r["shapes"], r["shape_of"], opts32, refs[T])
    eng.close()
    twin.close()
