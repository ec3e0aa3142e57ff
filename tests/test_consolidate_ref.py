"""The two references of the consolidation preview (tests/consolidate_ref.py) agree on the shared
32-node trace — oracle/pysim.py's PySim with nodes leaving its node set and the copy restored on a
block, and the integer chain the GPU tests use on the larger clusters — and the chain has the
properties its definition gives it.  Exact integer equality; no device."""
import numpy as np
import pytest

import consolidate_ref as cr
import drain_ref as dr
import place_ref as pr
import removable_ref as rr

N = 32


def _binds(r):
    return dict(pod=r["binds"][:, 0], node=r["binds"][:, 1], tick=r["binds"][:, 2], status=r["binds"][:, 3])


def _cfg(r):
    from harness import MODES
    return pr.engine_cfg(MODES[r["mode"]], r["enc"])


def _orders():
    rng = np.random.default_rng(32)
    return dict(ascending=list(range(N)), descending=list(range(N - 1, -1, -1)),
                permuted_subset=[int(x) for x in rng.permutation(N)[:20]])


@pytest.mark.parametrize("case", ["feeds", "literal", "feeds_irregular"])
def test_integer_chain_equals_pysim_with_nodes_leaving_and_rollback(case):
    r = pr.parity_case(case)
    enc, cfg, binds = r["enc"], _cfg(r), _binds(r)
    seen = dict(removed=0, blocked=0, dest=0, rows=0, late_block=0, empty=0)
    for t in pr.TICKS:
        ps = dr.sim_at(case, t)
        state = dr.sim_state(ps, t)
        for what, nodes in _orders().items():
            slow = cr.pysim_consolidate(ps, t, nodes)
            running = None
            if case == "feeds_irregular":   # (phases of irregular length: the running pods are PySim's own)
                running = {c: [j for j, pod in enumerate(ps.pods) if pod["node"] == c and
                               ps.node_pods[c].get(pod["key"]) == j and ps._running(pod, t)] for c in nodes}
            fast = cr.fast_consolidate(r["tr"], enc, binds, cfg, t, nodes, state=state, running=running)
            cr.assert_same(fast, slow, f"{case} tick {t} {what}")
            oc = slow["outcome"]
            assert (slow["evicted"] == state[nodes, 3]).all()
            assert (slow["n_rows"][oc == cr.REMOVED] == slow["evicted"][oc == cr.REMOVED]).all()
            assert (slow["n_rows"][oc == cr.DESTINATION] == 0).all() and (slow["n_rows"][oc == cr.BLOCKED] >= 1).all()
            seen["removed"] += int((oc == cr.REMOVED).sum())
            seen["blocked"] += int((oc == cr.BLOCKED).sum())
            seen["dest"] += int((oc == cr.DESTINATION).sum())
            seen["rows"] += len(slow["rows"]["pod"])
            seen["late_block"] += int(((oc == cr.BLOCKED) & (slow["n_rows"] >= 2)).sum())
            seen["empty"] += int(((oc == cr.REMOVED) & (slow["evicted"] == 0)).sum())
        np.testing.assert_array_equal(dr.sim_state(ps, t), state)   # the base sim is left as it was
    assert seen["removed"] >= 40 and seen["dest"] >= 10 and seen["rows"] >= 20 and seen["empty"] >= 10, seen
    if case == "literal":
        assert seen["blocked"] >= 1, seen


def _chain(case, t, nodes):
    r = pr.parity_case(case)
    ps = dr.sim_at(case, t)
    return cr.fast_consolidate(r["tr"], r["enc"], _binds(r), _cfg(r), t, nodes, state=dr.sim_state(ps, t)), r


@pytest.mark.parametrize("case", ["feeds", "literal"])
def test_one_candidate_is_its_drain_truncated(case):
    tried = 0
    for t in (400, 800):
        state = dr.sim_state(dr.sim_at(case, t), t)
        for c in range(N):
            got, r = _chain(case, t, [c])
            ev, frm = dr.running_on(r["tr"], r["enc"], _binds(r), t, [c])
            one = dr.fast_drain(r["enc"]["alloc"], state, _cfg(r), r["enc"]["pods"], ev, frm, [c])
            bad = np.nonzero(one["status"] != pr.OK)[0]
            keep = len(ev) if len(bad) == 0 else int(bad[0]) + 1
            assert got["outcome"][0] == (cr.REMOVED if len(bad) == 0 else cr.BLOCKED) and got["n_rows"][0] == keep
            for f in dr.FIELDS:
                np.testing.assert_array_equal(got["rows"][f], one[f][:keep], err_msg=f"{case} tick {t} node {c}: {f}")
            np.testing.assert_array_equal(got["after"], one["after"] if len(bad) == 0 else state)
            tried += len(ev) > 0
    assert tried >= 10


def test_a_prefix_of_the_answers_is_the_call_on_the_prefix():
    for t in (400, 800):
        full, _ = _chain("feeds", t, list(range(N)))
        for j in (1, 7, 20):
            part, _ = _chain("feeds", t, list(range(j)))
            for f in cr.SUMMARY:
                np.testing.assert_array_equal(full[f][:j], part[f], err_msg=f"tick {t} prefix {j}: {f}")
            k = len(part["rows"]["pod"])
            for f in dr.FIELDS:
                np.testing.assert_array_equal(full["rows"][f][:k], part["rows"][f])


@pytest.mark.parametrize("case", ["feeds", "literal"])
def test_every_pod_of_a_removed_node_moved_and_nothing_else_changed(case):
    moved = 0
    for t in pr.TICKS:
        state = dr.sim_state(dr.sim_at(case, t), t)
        for nodes in _orders().values():
            got, _ = _chain(case, t, nodes)
            np.testing.assert_array_equal(got["after"].sum(axis=0), state.sum(axis=0))
            removed = got["node"][got["outcome"] == cr.REMOVED]
            assert (got["after"][removed] == 0).all()
            ok_rows = got["rows"]["status"] == pr.OK
            kept = np.isin(got["rows"]["from_node"], removed)
            assert (ok_rows | ~kept).all(), "a removed candidate has a pod that is not bound Ok"
            dest = set(got["rows"]["node"][kept].tolist())
            assert not dest & set(removed.tolist()), "a destination was removed"
            untouched = [x for x in range(N) if x not in dest and x not in set(removed.tolist())]
            np.testing.assert_array_equal(got["after"][untouched], state[untouched])
            if len(removed) == 0:
                np.testing.assert_array_equal(got["after"], state)
            moved += int(kept.sum())
    assert moved >= 20


def test_nothing_removed_leaves_the_state():
    """literal mode, a full node first: every attempt that blocks is rolled back completely"""
    hit = 0
    for t in pr.TICKS:
        state = dr.sim_state(dr.sim_at("literal", t), t)
        got, _ = _chain("literal", t, list(range(N)))
        blocked = [int(c) for c in got["node"][got["outcome"] == cr.BLOCKED]]
        if not blocked:
            continue
        only, _ = _chain("literal", t, blocked[:1])
        assert only["outcome"].tolist() == [cr.BLOCKED] or only["outcome"].tolist() == [cr.REMOVED]
        if only["outcome"][0] == cr.BLOCKED:
            np.testing.assert_array_equal(only["after"], state)
            assert only["info"][1:4] == [0, 1, 0] and only["info"][5] == 0
            hit += 1
    assert hit >= 1


def test_the_chain_is_not_the_removal_scan():
    """Removable alone is not removable in the chain: earlier removals fill the nodes and make
    destinations, so the two answers differ on the same candidates."""
    differs = 0
    for t in (400, 800):
        r = pr.parity_case("feeds")
        state = dr.sim_state(dr.sim_at("feeds", t), t)
        nodes = list(range(N))
        alone = rr.fast_removable(r["tr"], r["enc"], _binds(r), _cfg(r), t, nodes, state=state)
        chain, _ = _chain("feeds", t, nodes)
        differs += int((alone["removable"] != (chain["outcome"] == cr.REMOVED)).sum())
        assert (chain["outcome"] == cr.REMOVED).sum() <= alone["removable"].sum() or differs
    assert differs >= 1
