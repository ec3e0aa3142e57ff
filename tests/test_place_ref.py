"""The two references of the placement preview agree (tests/place_ref.py): PySim asked pod after pod
with its own string predicates and Fractions, and the integer walk on the encoded arrays that the
larger GPU cases are checked against — on the shared 32-node trace at six ticks in feeds, literal
and irregular-phase modes, 48 pods over 12 shapes each, every field.  No device is needed."""
import pytest

import place_ref as pr


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_fast_place_equals_pysim_place(case):
    r = pr.parity_case(case)
    assert len(r["binds"]) > 700
    for t in pr.TICKS:
        pr.assert_same(r["fast"][t], r["slow"][t], f"{case} tick {t}")
        assert r["fast"][t]["reused"] == r["slow"][t]["reused"]
        assert sum(r["slow"][t]["info"][1:]) == pr.N_PODS
    pr.assert_not_vacuous(case, r["slow"])


def test_hand_shapes_do_what_they_are_for():
    r = pr.parity_case("feeds")
    so = r["shape_of"]
    for t in pr.TICKS:
        ref = r["slow"][t]
        assert (ref["status"][so == 8] == pr.NOT_FOUND).all(), "the impossible selector found a node"
        assert (ref["candidates"][so == 8] == 0).all()
        # the pod that tolerates nothing only sees untainted nodes
        assert (ref["candidates"][so == 7] < 32).all()
    assert any((r["slow"][t]["status"][so == 9] == pr.OK).any() for t in pr.TICKS), "the odd memory request never fits"
    lit = pr.parity_case("literal")
    assert all((lit["slow"][t]["status"] != pr.NOT_FOUND).all() for t in pr.TICKS)


def test_no_nodes_and_no_scorers():
    import numpy as np
    r = pr.parity_case("feeds")
    cfg = pr.engine_cfg((1, 7, ()), r["enc"])
    out = pr.fast_place(r["enc"]["alloc"], np.zeros((32, 4), np.int64), cfg, r["shapes"], r["shape_of"])
    assert (out["status"] == pr.NOT_FOUND).all() and (out["candidates"] == 0).all() and out["info"][3] == pr.N_PODS
    cfg = pr.engine_cfg((1, 7, ((1, 1, 0),)), dict(taint=[], label=[]))
    out = pr.fast_place(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), cfg, r["shapes"])
    assert (out["status"] == pr.NOT_FOUND).all() and len(out["node"]) == 12
