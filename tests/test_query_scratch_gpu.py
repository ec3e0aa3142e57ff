"""The past-tick queries share two grow-only device scratches (ks_queries.cpp: d_qs, d_qi), each carved
anew by every call (ks_carve.h).  One engine makes ten kinds of query in an order in which both
scratches first grow, are then reused by smaller layouts and grow again — with the odd counts that
take the layouts' alignment paths — and then the same calls in reverse.  Every result must equal,
exactly, the same call on a twin engine that made no other query, and the Python references the
suite has for it (drain_ref, place_ref, headroom_ref, state_ref).  Everything is integer equality.
"""
import numpy as np
import pytest

import drain_ref as dr
import headroom_ref as hr
import place_ref as pr
import state_ref as sr
from harness import MODES, assert_same_binds, make_engine

pytestmark = pytest.mark.gpu

T = 400                  # ticks stepped
LO, HI = T - 64, T + 1   # the 65-tick window
SHAPES = [0, 1, 11]      # of place_ref.parity_case's twelve: two trace pods' and HAND's small one
K = 33


def _same(got, want, what):
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        for f in want:
            _same(got[f], want[f], f"{what}: {f}")
    elif isinstance(want, tuple):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{what}[{i}]")
    elif want is None:
        assert got is None, what
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


def _engine(r):
    eng = make_engine(r["tr"], r["enc"], pr.FEEDS, batch_pods=64)
    eng.submit(r["enc"]["pods"])
    return eng, eng.step(T)


def test_ten_query_kinds_on_one_engine_equal_a_fresh_twin_each():
    r = pr.parity_case("feeds")
    tr, enc = r["tr"], r["enc"]
    b = r["binds"][r["binds"][:, 2] <= T]
    binds = dict(pod=b[:, 0], node=b[:, 1], tick=b[:, 2], status=b[:, 3])
    ref = sr.IntervalRef(tr, binds)
    state = ref.at(T)
    ps = dr.sim_at("feeds", T)
    np.testing.assert_array_equal(state, dr.sim_state(ps, T))

    # the drained nodes: the shortest prefix of the nodes that runs an odd number >= 3 of pods at T
    m = next(m for m in range(1, 33) if state[:m, 3].sum() >= 3 and state[:m, 3].sum() % 2 == 1)
    drained = list(range(m))
    want_drain = dr.pysim_drain(ps, T, drained)
    n_ev = len(want_drain["pod"])
    assert n_ev >= 3 and n_ev % 2 == 1 and n_ev == state[:m, 3].sum(), "the reference's eviction count is not odd"

    all_shapes, sim = hr.make_shapes(tr, enc, dict(ps=ps), list(pr.TRACE_PODS), pr.HAND)
    _same(all_shapes, r["shapes"], "the case's shapes")
    shapes = {f: np.ascontiguousarray(v[SHAPES]) for f, v in all_shapes.items()}
    shape_of = (np.arange(K) % 3).astype(np.int32)
    fm, fl, _ = MODES[pr.FEEDS]
    elig = hr.eligibility(dict(ps=ps, filter_mode=fm, filters=fl), [sim[j] for j in SHAPES])
    want_cols, want_counts = hr.reference(enc["alloc"], ref.window(LO, HI), shapes, elig)
    want_place = pr.fast_place(enc["alloc"], state, pr.engine_cfg(MODES[pr.FEEDS], enc), shapes, shape_of)
    assert (want_place["status"] == pr.OK).sum() >= 3 and want_cols[:, :, 0].any()
    pod = int(binds["pod"][binds["node"] >= 0][-1])       # a bound pod, for score_at / filter_at

    calls = [
        ("drain_at", lambda e: e.drain_at(T, drained, after=True)),
        ("headroom_series", lambda e: e.headroom_series(LO, HI, shapes)),
        ("place_at", lambda e: e.place_at(T, shapes, shape_of, after=True)),
        ("node_peaks", lambda e: e.node_peaks(LO, HI)),
        ("headroom_at", lambda e: e.headroom_at(T, shapes, per_node=True)),
        ("requested_at", lambda e: e.requested_at(T)),
        ("score_at / filter_at", lambda e: (e.score_at(pod), e.filter_at(pod))),
        ("cluster_series", lambda e: e.cluster_series(LO, HI)),
        ("usage_at", lambda e: e.usage_at(T)),
        ("usage_digest", lambda e: e.usage_digest(LO, HI)),
    ]

    # a fresh twin per call kind: it makes that one call and nothing else
    alone = {}
    for name, call in calls:
        twin, tb = _engine(r)
        assert_same_binds(tb, binds)
        alone[name] = call(twin)
        twin.close()

    # the references, on the twins' answers (the engine's must equal those)
    dr.assert_same(alone["drain_at"], want_drain, "drain_at alone")
    pr.assert_same(alone["place_at"], want_place, "place_at alone")
    np.testing.assert_array_equal(alone["headroom_series"], want_cols[:, :, :2])
    np.testing.assert_array_equal(alone["headroom_at"][0], want_cols[-1])
    np.testing.assert_array_equal(alone["headroom_at"][1], want_counts[-1])
    np.testing.assert_array_equal(alone["requested_at"], state)
    np.testing.assert_array_equal(alone["node_peaks"], ref.peaks(LO, HI))
    np.testing.assert_array_equal(alone["cluster_series"], ref.series(LO, HI))
    np.testing.assert_array_equal(alone["usage_at"], ref.usage_window(T, T + 1)[0])
    score, mask = alone["score_at / filter_at"]
    assert int(score.argmax()) == int(binds["node"][binds["pod"] == pod][0]) and mask.any()
    assert alone["usage_digest"].shape == (HI - LO, 6) and alone["usage_digest"].any()

    eng, eb = _engine(r)
    assert_same_binds(eb, binds)
    for turn, order in (("forward", calls), ("reversed", calls[::-1])):
        for name, call in order:
            _same(call(eng), alone[name], f"{name}, {turn}")
    eng.close()
