"""The five previews on wide clusters and long histories, against the integer references of
tests/preview_wide_cases.py (pinned on their own by tests/test_preview_wide_cases.py).  Everything is
exact integer equality; the engine's binds are asserted equal to the C oracle's first.

Width: 64, 65 and 129 scan blocks — place_merge_kernel's lanes fold one, two and three block lists —
with the winners planted in the high blocks; one engine per cluster answers all five previews, and
the run goes on afterwards as the oracle's does.  Depth: 66,048 pods with a running pod in each of
258 gather blocks — drain_scan_kernel's second chunk and its carry — and the same questions at a tick
with 200 blocks as the control.
"""
import numpy as np
import pytest

import consolidate_ref as cr
import drain_ref as dr
import place_ref as pr
import preview_wide_cases as wc
import removable_ref as rr
import scaleup_ref as su
from harness import assert_same_binds, make_engine

pytestmark = pytest.mark.gpu


# ---- width ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(wc.WIDE))
def wide(request):
    c = wc.wide_case(request.param)
    eng = make_engine(c["tr"], c["enc"], c["mode"], batch_pods=64)
    eng.submit(c["enc"]["pods"])
    assert_same_binds(eng.step(wc.T_WIDE), c["ob"])
    yield request.param, c, eng
    eng.close()


def test_place_at_on_the_last_and_a_past_tick(wide):
    name, c, eng = wide
    for t in (wc.T_WIDE, wc.T_PAST):
        got = eng.place_at(t, c["shapes"], c["shape_of"], after=True)
        pr.assert_same(got, wc.place_ref(name, t), f"{name}: place at tick {t}")


def test_place_at_copies_of_the_gated_shape_take_two_rounds(wide):
    name, c, eng = wide
    got = eng.place_at(wc.T_WIDE, c["shapes"], np.full(wc.COPIES, wc.GATED, np.int32), after=True)
    pr.assert_same(got, wc.copies_ref(name), f"{name}: {wc.COPIES} copies")
    if c["mode"] == pr.FEEDS:
        assert got["info"][0] >= 2, "the copies were decided from one round's lists"


def test_drain_at(wide):
    name, c, eng = wide
    got = eng.drain_at(wc.T_WIDE, wc.drain_nodes(name), after=True)
    dr.assert_same(got, wc.drain_ref(name), f"{name}: drain")


def test_removable_at(wide):
    name, c, eng = wide
    got = eng.removable_at(wc.T_WIDE, wc.candidates(name), rows=True)
    rr.assert_same(got, wc.removable_ref(name), f"{name}: removable")


def test_consolidate_at(wide):
    name, c, eng = wide
    ref = wc.consolidate_ref(name)
    got = eng.consolidate_at(wc.T_WIDE, wc.candidates(name), rows=True, after=True)
    cr.assert_same(got, ref, f"{name}: consolidate")
    assert got["evicted_total"] == int(ref["evicted"].sum())


def test_scale_up_at(wide):
    name, c, eng = wide
    shapes = wc.scale_shapes(c)
    got = eng.scale_up_at(wc.T_WIDE, shapes, wc.scale_options(c), wc.SCALE_OF, rows=True)
    su.assert_same(got, wc.scale_ref(name), what=f"{name}: scale up")
    plain = eng.place_at(wc.T_WIDE, shapes, wc.SCALE_OF)     # the option that appends nothing
    for f in pr.FIELDS:
        np.testing.assert_array_equal(got["rows"][f][2], plain[f], err_msg=f"{name}: no-append option: {f}")


def test_no_preview_touched_the_run(wide):
    name, c, eng = wide
    np.testing.assert_array_equal(eng.usage(), c["usage"], err_msg=f"{name}: usage after the previews")
    assert_same_binds(eng.step(wc.T_NEXT), c["nxt"])


# ---- depth ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep():
    c = wc.deep_case()
    eng = make_engine(c["tr"], c["enc"], pr.FEEDS, batch_pods=256)
    eng.submit(c["enc"]["pods"])
    assert_same_binds(eng.step(wc.DEEP_T), c["ob"])
    yield c, eng
    eng.close()


@pytest.mark.parametrize("t", [wc.DEEP_LATE, wc.DEEP_EARLY], ids=["two_chunks", "one_chunk"])
def test_the_gather_past_one_scan_chunk(deep, t):
    c, eng = deep
    r = wc.deep_refs(t)
    nodes = r["nodes"]
    np.testing.assert_array_equal(eng.requested_at(t), r["state"], err_msg=f"requested at tick {t}")
    dr.assert_same(eng.drain_at(t, nodes, after=True), r["drain"], f"drain at tick {t}")
    rr.assert_same(eng.removable_at(t, nodes, rows=True), r["removable"], f"removable at tick {t}")
    for order, ref in zip((nodes, nodes[::-1]), r["consolidate"]):
        got = eng.consolidate_at(t, order, rows=True, after=True)
        cr.assert_same(got, ref, f"consolidate at tick {t}, from node {order[0]}")
        assert got["evicted_total"] == int(ref["evicted"].sum())
