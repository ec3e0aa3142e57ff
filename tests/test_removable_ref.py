"""The two references of the removal scan (tests/removable_ref.py) agree on the shared 32-node trace:
oracle/pysim.py's PySim with one node removed, asked pod after pod, once per candidate, and the
integer walk ``fast_drain`` with ``drained=[c]`` the GPU tests use on the larger clusters.  Exact
integer equality; no device."""
import numpy as np
import pytest

import drain_ref as dr
import place_ref as pr
import removable_ref as rr

N = 32


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_integer_walk_per_candidate_equals_pysim_with_one_node_removed(case):
    from harness import MODES
    r = pr.parity_case(case)
    enc = r["enc"]
    cfg = pr.engine_cfg(MODES[r["mode"]], enc)
    binds = dict(pod=r["binds"][:, 0], node=r["binds"][:, 1], tick=r["binds"][:, 2], status=r["binds"][:, 3])
    nodes = list(range(N))
    seen = dict(evicted=0, ok=0, none=0, over=0, empty=0, removable=0, stuck=0)
    for t in pr.TICKS:
        ps = dr.sim_at(case, t)
        state = dr.sim_state(ps, t)
        slow = rr.pysim_removable(ps, t, nodes)
        if case != "feeds_irregular":
            fast = rr.fast_removable(r["tr"], enc, binds, cfg, t, nodes, state=state)
        else:   # (phases of irregular length: the running pods are PySim's own)
            fast = rr.assemble(nodes, [dr.fast_drain(enc["alloc"], state, cfg, enc["pods"], p["pod"].tolist(),
                                                     p["from_node"].tolist(), [c]) for c, p in zip(nodes, slow["per"])])
        for f in rr.SUMMARY:
            np.testing.assert_array_equal(fast[f], slow[f], err_msg=f"{case} tick {t}: {f}")
        for f in dr.FIELDS:
            np.testing.assert_array_equal(fast["rows"][f], slow["rows"][f], err_msg=f"{case} tick {t}: rows {f}")
        # the summary is the rows': contiguous, in the caller's order, every pod from its candidate
        assert slow["evicted"].sum() == len(slow["rows"]["pod"]) == state[:, 3].sum()
        for j, c in enumerate(nodes):
            a, b = int(slow["first_row"][j]), int(slow["first_row"][j] + slow["evicted"][j])
            assert (slow["rows"]["from_node"][a:b] == c).all() and (np.diff(slow["rows"]["pod"][a:b]) > 0).all()
            assert not (slow["rows"]["node"][a:b] == c).any(), "a pod went back to its own node"
            assert slow["evicted"][j] == state[c, 3]
        seen["evicted"] += int(slow["evicted"].sum())
        seen["ok"] += int(slow["ok"].sum())
        seen["none"] += int(slow["not_found"].sum())
        seen["over"] += int(slow["over_capacity"].sum())
        seen["empty"] += int((slow["evicted"] == 0).sum())
        seen["removable"] += int(slow["removable"].sum())
        seen["stuck"] += int((~slow["removable"]).sum())
    assert seen["evicted"] >= 20 and seen["ok"] >= 10 and seen["empty"] >= 10 and seen["removable"] >= 40, seen
    if case == "literal":
        assert seen["over"] >= 1 and seen["stuck"] >= 1, seen
        assert (slow["rows"]["candidates"] == N - 1).all()


def test_a_candidate_alone_is_not_the_set():
    """Candidates are independent: draining two busy nodes together differs from asking each alone
    (the pods of the second see the first's placements), so the reference must not share state."""
    from harness import MODES
    r = pr.parity_case("feeds")
    cfg = pr.engine_cfg(MODES[r["mode"]], r["enc"])
    differs = 0
    for t in pr.TICKS:
        ps = dr.sim_at("feeds", t)
        state = dr.sim_state(ps, t)
        busy = [int(c) for c in np.nonzero(state[:, 3] > 0)[0]]
        alone = rr.pysim_removable(ps, t, busy)
        together = dr.pysim_drain(ps, t, busy)
        assert sorted(alone["rows"]["pod"].tolist()) == together["pod"].tolist()
        by_pod = dict(zip(alone["rows"]["pod"].tolist(), alone["rows"]["node"].tolist()))
        differs += sum(by_pod[p] != nd for p, nd in zip(together["pod"].tolist(), together["node"].tolist()))
        # ... and the base state is left as it was
        np.testing.assert_array_equal(dr.sim_state(ps, t), state)
    assert differs >= 1
    assert cfg["filter_mode"] == 1
