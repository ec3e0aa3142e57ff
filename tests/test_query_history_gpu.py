"""Past-tick queries on an engine with a history (include/ks_engine.h): three submits, two of which
lower the device unit and rescale the node table and every earlier pod record (ks_engine.cpp
ks_submit_pods, launch_rescale), steps of uneven lengths, and every query type asked between them.

The same 32-node, 800-pod trace goes to two engines.  A takes one submit and one ks_step(800).  B
takes the pods in three parts, each submitted before its first pod arrives: the second part's
memory requests are fractional bytes, the third part's cpu requests are one milli-cpu off the
common divisor.  B runs the chunk resolver (forced, overlap on) and is asked every query between
its steps.  The model is oracle/pysim.py's PySim, given the same parts at the same ticks and
stepped tick by tick.  B's binds equal A's and the model's; every answer, mid-run and at the end,
equals the model and A's.  Everything is exact integer equality.
"""
import functools

import numpy as np
import pytest

import headroom_ref as hr
import place_ref as pr
import usage_digest as ud
from harness import MODES, assert_same_binds, encoded, make_engine
from kubesim_amd import encode as E
from kubesim_amd import tracegen
from pysim import PySim
from test_state_queries_gpu import _matrix, _series_from_model

pytestmark = pytest.mark.gpu

T = 800
FEEDS, LITERAL = "feeds_all_lrba", "literal_lrba_filters_ignored"
# (mode, phase multiplier, capacity factor): pods long enough that more than a hundred run across
# each rescale; the literal cluster is the tighter one, so some of its binds are OverCapacity
CASES = {"feeds": (FEEDS, 12, 2), "literal": (LITERAL, 16, 1)}
STEPS = ((1, 37, 193), (1, 300), (200, 1, 67))      # the steps after the first, second and third submit
SUBMIT_AT = (0, 231, 532)
SAMPLE = 8
HAND = [
    ([0, 0, 500], 4, True, False),                      # half a gpu: fractional in the gpu unit at all times
    ([-1, 3_000_000_000_001, -1], 2, True, False),      # memory only, no multiple of any unit but 1
    ([9, 9, 9], 0, True, False),                        # empty keymask
    ([1000, (1 << 30) * 1000, 0], 3, False, False),     # tolerates nothing
    ([8000, (64 << 30) * 1000, 4000], 7, True, False),  # 8 cpu / 64 Gi / 4 gpu
]
SHAPE_PODS = (0, 33, 66, 99, 132, 165, 300, 340, 400, 600, 650, 790)   # six of the first part, three of each later one
N_WHOLE = 6
TICKS_END = (0, 1, 137, 231, 232, 400, 532, 533, 799, 800)
WINDOWS = ((0, T + 1), (200, 260), (500, 560), (231, 233), (532, 534))


def _trace(case):
    mode, mult, cap = CASES[case]
    tr = hr.shared_trace(mult)
    nd, p = tr["nodes"], tr["pods"]
    nd["alloc"][:, :2] *= cap
    nd["alloc"][:, 2] = 16000 * cap            # every node has gpus: they never bind first
    nd["alloc_has"][:] = 15
    cuts = [int(np.searchsorted(p["arrival"], s + 1)) for s in SUBMIT_AT] + [p["m"]]
    p["req"][cuts[1]:, 1] += 1                 # + 1 milli-byte: not a whole byte
    p["req"][cuts[2]:, 0] += 1                 # + 1 milli-cpu: off the 100 m grid
    return tr, cuts


def _gcd(tr, key, hi):
    nd, p = tr["nodes"], tr["pods"]
    vals = np.concatenate([nd["alloc"][(nd["alloc_has"] >> key) & 1 == 1, key],
                           p["req"][:hi][(p["req_has"][:hi] >> key) & 1 == 1, key]])
    return int(np.gcd.reduce(vals[vals > 0]))


@functools.lru_cache(maxsize=None)
def _model(case):
    """PySim given the parts at SUBMIT_AT and stepped tick by tick (tests/test_state_queries_gpu.py
    ``_check_model`` with staged submits, plus the usage after every tick), the shapes and their
    references.  Every assert here is on the trace and the model alone."""
    tr, cuts = _trace(case)
    mode = CASES[case][0]
    fm, fl, sc = MODES[mode]
    p = tr["pods"]
    assert cuts[0] == 0 and all(cuts[i] + 100 < cuts[i + 1] for i in range(3))
    for s, c in zip(SUBMIT_AT, cuts):
        assert p["arrival"][c] > s, "a part is submitted after its first pod's arrival"
    # the rescales, on the trace alone: memory's unit falls at the second submit, cpu's at the third
    mem = [_gcd(tr, 1, c) for c in cuts[1:]]
    cpu = [_gcd(tr, 0, c) for c in cuts[1:]]
    assert mem[1] < mem[0] and cpu[1] == cpu[0] and cpu[2] < cpu[1], (mem, cpu)
    parts = [tracegen.slice_pods(tr, cuts[i], cuts[i + 1]) for i in range(3)]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    req, usage, popped = [np.zeros((ps.n, 4), np.int64)], [np.zeros((ps.n, 3), np.int64)], [0]
    binds, seen = [], {}
    for t in range(1, T + 1):
        if t - 1 in SUBMIT_AT:
            ps.submit(parts[SUBMIT_AT.index(t - 1)])
        j, snap = ps.qhead, None
        if j < len(ps.pods) and ps.pods[j]["arrival"] <= t and len(binds) % SAMPLE == 0:
            pod = ps.pods[j]
            score = np.full(ps.n, -1, np.int64)
            for n, v in ps._score_map(pod, t).items():
                score[n] = v
            mask = np.ones(ps.n, np.uint8)
            for bit, fn in ((1, lambda n: ps._fits(n, pod, t)), (2, lambda n: ps._taint_ok(n, pod)),
                            (4, lambda n: ps._selector_ok(n, pod))):
                if fl & bit:
                    mask &= np.array([fn(n) for n in range(ps.n)], np.uint8)
            snap = (score, mask)
        b, err = ps.step(1)
        assert err is None
        binds += b
        if b and snap is not None:
            seen[b[0][0]] = snap
        req.append(_matrix(ps, t))
        usage.append(np.array(ps.usage(), np.int64))
        popped.append(ps.qhead)
    assert len(ps.pods) == p["m"]
    m = dict(binds=np.array(binds, np.int64).reshape(-1, 4), req=np.stack(req), usage=np.stack(usage),
             popped=np.array(popped), seen=seen, n=ps.n)
    b = m["binds"]
    assert len(b) > 600 and (np.diff(m["req"][:, :, 3].sum(axis=1)) < 0).sum() > 50
    assert sum(1 for q in seen if b[b[:, 0] == q][0, 2] <= SUBMIT_AT[1]) >= 20, "too few sampled pods before the first rescale"
    if case == "literal":
        assert (b[:, 3] == 1).sum() > 20, "too few OverCapacity binds"
    # more than a hundred pods bound Ok before each rescale still run after it
    ok = b[b[:, 3] == 0]
    for s in SUBMIT_AT[1:]:
        early = ok[ok[:, 2] <= s]
        still = sum(1 for q, n, t0, _ in early.tolist() if ps._running(ps.pods[q], s + 1))
        assert still >= 100, f"only {still} pods run across the rescale at tick {s}"
    enc = encoded(tr)
    model = dict(ps=ps, filter_mode=fm, filters=fl)
    shapes, sim = hr.make_shapes(tr, enc, model, list(SHAPE_PODS), HAND)
    assert all(cuts[1] <= q < cuts[2] for q in SHAPE_PODS[6:9]) and all(q >= cuts[2] for q in SHAPE_PODS[9:])
    elig = hr.eligibility(model, sim)
    cols, counts = hr.reference(enc["alloc"], m["req"], shapes, elig)
    assert (np.diff(cols[:, :, 0], axis=0) != 0).sum() > 2000
    whole = {f: np.ascontiguousarray(v[:N_WHOLE]) for f, v in shapes.items()}
    # whole: multiples of every unit B ever holds (the gcd after the first submit); the rest is not
    for key in range(3):
        u = _gcd(tr, key, cuts[1])
        assert (whole["req"][:, key] % u == 0).all()
    assert shapes["req"][0 + len(SHAPE_PODS), 2] % _gcd(tr, 2, p["m"]) != 0, "the half gpu is a whole unit"
    k = len(shapes["keymask"])
    shape_of = np.array([(5 * i) % k for i in range(2 * k)], np.int32)
    whole_of = np.array([(5 * i) % N_WHOLE for i in range(2 * k)], np.int32)
    return dict(tr=tr, cuts=cuts, parts=parts, mode=mode, enc=enc, m=m, shapes=shapes, cols=cols, counts=counts,
                whole=whole, shape_of=shape_of, whole_of=whole_of, cfg=pr.engine_cfg(MODES[mode], enc),
                series=_series_from_model(tr, m))


# ---- what an engine is asked, and what the model says ----------------------------------------
def _ask(eng, r, t, lo):
    """Every query type at tick t and over [lo, t + 1): a dict of answers."""
    sh = r["shapes"]
    out = dict(requested=eng.requested_at(t), usage=eng.usage_at(t), digest=eng.usage_digest(lo, t + 1),
               series=eng.cluster_series(lo, t + 1), peaks=eng.node_peaks(lo, t + 1),
               head=eng.headroom_at(t, sh, per_node=True), head_series=eng.headroom_series(lo, t + 1, sh),
               place=eng.place_at(t, sh, r["shape_of"], after=True),
               place_whole=eng.place_at(t, r["whole"], r["whole_of"], after=True))
    bound = [q for q in r["m"]["seen"] if q < _bound_by(r, t)]
    out["pods"] = {q: (eng.score_at(q), eng.filter_at(q)) for q in bound[:2] + bound[-2:]}
    return out


def _bound_by(r, t):
    return int((r["m"]["binds"][:, 2] <= t).sum())


def _assert_answer(r, got, t, lo, what):
    m = r["m"]
    eq = lambda a, b, name: np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name} at tick {t}, window from {lo}")
    eq(got["requested"], m["req"][t], "requested_at")
    eq(got["usage"], m["usage"][t], "usage_at")
    eq(got["digest"], ud.digest_from_matrices(m["usage"][lo:t + 1]), "usage_digest")
    eq(got["series"], r["series"][lo:t + 1], "cluster_series")
    eq(got["peaks"], m["req"][lo:t + 1].max(axis=0), "node_peaks")
    eq(got["head"][0], r["cols"][t], "headroom_at")
    eq(got["head"][1], r["counts"][t], "headroom_at per node")
    eq(got["head_series"], r["cols"][lo:t + 1, :, :2], "headroom_series")
    alloc = r["enc"]["alloc"]
    pr.assert_same(got["place"], pr.fast_place(alloc, m["req"][t], r["cfg"], r["shapes"], r["shape_of"]), f"{what}: place_at {t}")
    pr.assert_same(got["place_whole"], pr.fast_place(alloc, m["req"][t], r["cfg"], r["whole"], r["whole_of"]),
                   f"{what}: place_at {t}, whole units")
    for q, (score, mask) in got["pods"].items():
        eq(score, m["seen"][q][0], f"score_at pod {q}")
        eq(mask, m["seen"][q][1], f"filter_at pod {q}")


def _past_ticks(t):
    """(tick, window start) pairs asked when the engine stands at tick t: now, and past ticks on
    either side of the rescales behind it."""
    out = [(t, max(0, t - 150)), (t // 2, max(0, t // 2 - 40))]
    for s in SUBMIT_AT[1:]:
        if t > s:
            out += [(s, max(0, s - 30)), (s + 1, s)]
    return out


@pytest.fixture(scope="module", params=["feeds", "literal"])
def history(request):
    """A, B and every answer B gave between its steps."""
    from kubesim_amd import _lib
    r = _model(request.param)
    tr, enc = r["tr"], r["enc"]
    a = make_engine(tr, enc, r["mode"], batch_pods=64)
    a.submit(enc["pods"])
    ab = a.step(T)
    b = make_engine(tr, enc, r["mode"], batch_pods=64, engine_flags=_lib.KS_ENGINE_CHUNK_RESOLVER)
    bb, answers = [], []
    for part, at, steps in zip(r["parts"], SUBMIT_AT, STEPS):
        assert b.tick == at
        b.submit(E.encode_pods(part["pods"], enc["taint_dict"], enc["label_dict"]))
        for k in steps:
            bb.append(b.step(k))
            for t, lo in _past_ticks(b.tick):
                answers.append((b.tick, t, lo, _ask(b, r, t, lo)))
    assert b.tick == T
    yield dict(r=r, a=a, b=b, ab=ab, bb=np.concatenate(bb), answers=answers)
    a.close()
    b.close()


def test_interleaved_queries_and_rescales_change_no_bind(history):
    r = history["r"]
    mb = r["m"]["binds"]
    want = dict(pod=mb[:, 0], node=mb[:, 1], tick=mb[:, 2], status=mb[:, 3])
    assert_same_binds(history["ab"], want)
    assert_same_binds(history["bb"], want)
    np.testing.assert_array_equal(history["a"].usage(), history["b"].usage())


def test_every_answer_given_between_the_steps_equals_the_model(history):
    assert len(history["answers"]) >= 20
    for now, t, lo, got in history["answers"]:
        _assert_answer(history["r"], got, t, lo, f"asked at tick {now}")


def test_state_and_usage_at_every_tick_after_the_run(history):
    m = history["r"]["m"]
    for name in ("a", "b"):
        eng = history[name]
        for t in range(T + 1):
            np.testing.assert_array_equal(eng.requested_at(t), m["req"][t], err_msg=f"{name}: requested at tick {t}")
            np.testing.assert_array_equal(eng.usage_at(t), m["usage"][t], err_msg=f"{name}: usage at tick {t}")


def test_every_query_after_the_run_on_both_engines(history):
    r = history["r"]
    m = r["m"]
    for name in ("a", "b"):
        eng = history[name]
        for lo, hi in WINDOWS:
            _assert_answer(r, _ask(eng, r, hi - 1, lo), hi - 1, lo, f"{name} after the run")
        for t in TICKS_END:
            _assert_answer(r, _ask(eng, r, t, max(0, t - 3)), t, max(0, t - 3), f"{name} after the run")
        for q, (score, mask) in m["seen"].items():
            np.testing.assert_array_equal(eng.score_at(q), score, err_msg=f"{name}: score_at pod {q}")
            np.testing.assert_array_equal(eng.filter_at(q), mask, err_msg=f"{name}: filter_at pod {q}")
    assert len(m["seen"]) > 70
