"""Exact references for the removal scan (include/ks_engine.h: ks_removable_at).

For candidate c the answer is by definition that of ks_drain_at(t, 1, {c}), so the references are
tests/drain_ref.py's, called once per candidate with ``drained=[c]`` on the state at t:

* ``fast_removable``: ``drain_ref.fast_drain`` on ``place_ref.state_from_binds``;
* ``pysim_removable``: ``drain_ref.pysim_drain`` with that one node removed.

Both return ``dict(node, evicted, ok, over_capacity, not_found, removable, first_row, rows, per)``:
arrays over the candidates in the caller's order, ``rows`` = drain_ref's FIELDS concatenated in that
order (FIFO within a candidate), ``per`` = the per-candidate drain results.
"""
import numpy as np

import drain_ref as dr
import place_ref as pr

SUMMARY = ("node", "evicted", "ok", "over_capacity", "not_found", "removable", "first_row")


def assemble(nodes, per):
    """per[j]: a drain_ref result for drained = [nodes[j]]"""
    m = len(nodes)
    ev = np.array([len(r["pod"]) for r in per], np.int64).reshape(m)
    out = dict(node=np.array(nodes, np.int32).reshape(m), evicted=ev.astype(np.int32),
               ok=np.array([r["info"][1] for r in per], np.int32).reshape(m),
               over_capacity=np.array([r["info"][2] for r in per], np.int32).reshape(m),
               not_found=np.array([r["info"][3] for r in per], np.int32).reshape(m))
    out["removable"] = out["ok"] == out["evicted"]
    out["first_row"] = np.concatenate([[0], np.cumsum(ev)[:-1]]).astype(np.int64) if m else np.zeros(0, np.int64)
    out["rows"] = {f: np.concatenate([r[f] for r in per]) if m else np.zeros(0, np.int64) for f in dr.FIELDS}
    out["per"] = per
    return out


def fast_removable(tr, enc, binds, cfg, t, nodes, state=None):
    """binds: dict of arrays pod, node, tick, status (a run's binds); cfg: place_ref.engine_cfg"""
    if state is None:
        state = pr.state_from_binds(tr, enc, binds, t)
    per = []
    for c in nodes:
        ev, frm = dr.running_on(tr, enc, binds, t, [c])
        per.append(dr.fast_drain(enc["alloc"], state, cfg, enc["pods"], ev, frm, [c]))
    out = assemble(list(nodes), per)
    out["state"] = state
    return out


def pysim_removable(ps, t, nodes):
    return assemble(list(nodes), [dr.pysim_drain(ps, t, [c]) for c in nodes])


def own_node_ranks(enc, cfg, state, ref, L=32):
    """Per evicted pod of ``ref`` the rank of its own node in its un-cordoned score vector on the base
    state (0: it heads the vector; -1: it has no entry), by the engine's order: score descending, node
    index ascending.  The pods whose rank is below L have their own node in their snapshot list."""
    A = np.array(enc["alloc"], np.int64).reshape(-1, 4)
    S = np.array(state, np.int64).reshape(-1, 4)
    taint, label = np.asarray(cfg["taint"], np.uint64), np.asarray(cfg["label"], np.uint64)
    live = np.ones(len(A), bool)
    pods = enc["pods"]
    ranks = []
    for j, c in zip(ref["rows"]["pod"].tolist(), ref["rows"]["from_node"].tolist()):
        km = int(pods["keymask"][j])
        req = [int(pods["req"][j][k]) if (km >> k) & 1 else 0 for k in range(3)]
        v = dr.score_vector(cfg, A, S, taint, label, live, (req, km, int(pods["tol"][j]), int(pods["sel"][j])))
        ranks.append(-1 if v[c] == 0 else int((v > v[c]).sum() + (v[:c] == v[c]).sum()))
    return np.array(ranks, np.int64)


def reusing_candidates(ref):
    """candidates one of whose pods was placed on a node an earlier pod of the same candidate changed"""
    return [j for j, r in enumerate(ref["per"]) if r["reused"]]


def assert_same(got, want, what="", rows=True):
    """got: Engine.removable_at's dict"""
    for f in SUMMARY:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")
    if rows:
        for f in dr.FIELDS:
            np.testing.assert_array_equal(got["rows"][f], want["rows"][f], err_msg=f"{what}: rows {f}")
    info = [int(x) for x in got["info"]]
    ev = want["evicted"]
    assert info[3] == int((ev == 0).sum()) and info[4] == int(want["removable"].sum()) and info[5] == int(ev.sum()), (what, info)
    assert info[1] + info[2] + info[3] == len(ev), (what, info)
