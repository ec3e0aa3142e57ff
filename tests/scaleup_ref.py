"""Exact reference for the scale-up preview (include/ks_engine.h: ks_scale_up_at).

Option g is, by definition, the placement preview on the cluster plus ``max_nodes`` empty nodes of the
option's template appended after the real ones: ``scale_up`` concatenates the arrays (alloc, state,
taint, label) and hands them to ``place_ref.fast_place`` — nothing of the device algorithm (no
lists, no fresh-node key, no count start) is in it.

``scale_up`` returns per option ``dict(node, status, score, candidates, summary)`` with ``summary`` =
dict(ok, over_capacity, not_found, on_new, nodes_used, first_unplaced).
"""
import numpy as np

import place_ref as pr

SUMMARY = ("ok", "over_capacity", "not_found", "on_new", "nodes_used", "first_unplaced")
ROWS = pr.FIELDS


def option(alloc, max_nodes, taint=0, label=0):
    return dict(alloc=[int(x) for x in alloc], taint=int(taint), label=int(label), max_nodes=int(max_nodes))


def extended(alloc, state, cfg, opt):
    """The arrays of the cluster with the option's nodes appended."""
    m = opt["max_nodes"]
    a = np.concatenate([np.asarray(alloc, np.int64).reshape(-1, 4), np.tile(np.array(opt["alloc"], np.int64), (m, 1))])
    s = np.concatenate([np.asarray(state, np.int64).reshape(-1, 4), np.zeros((m, 4), np.int64)])
    c = dict(cfg)
    c["taint"] = np.concatenate([np.asarray(cfg["taint"], np.uint64), np.full(m, opt["taint"], np.uint64)])
    c["label"] = np.concatenate([np.asarray(cfg["label"], np.uint64), np.full(m, opt["label"], np.uint64)])
    return a, s, c


def summarize(r, n):
    st, nd = np.asarray(r["status"]), np.asarray(r["node"])
    ok = st == pr.OK
    bad = np.nonzero(~ok)[0]
    return dict(ok=int(ok.sum()), over_capacity=int((st == pr.OVER).sum()), not_found=int((st == pr.NOT_FOUND).sum()),
                on_new=int((ok & (nd >= n)).sum()), nodes_used=len(set(nd[ok & (nd >= n)].tolist())),
                first_unplaced=int(bad[0]) if len(bad) else -1)


def scale_up_one(alloc, state, cfg, shapes, shape_of, opt):
    n = len(alloc)
    a, s, c = extended(alloc, state, cfg, opt)
    r = pr.fast_place(a, s, c, shapes, shape_of)
    out = {f: r[f] for f in ROWS}
    out["summary"] = summarize(r, n)
    return out


def scale_up(alloc, state, cfg, shapes, shape_of, options):
    return [scale_up_one(alloc, state, cfg, shapes, shape_of, o) for o in options]


def assert_same(got, want, n_opts=None, what=""):
    """got: Engine.scale_up_at(..., rows=True); want: scale_up's list."""
    assert len(want) == len(got["ok"]), what
    for g, w in enumerate(want):
        for f in ROWS:
            np.testing.assert_array_equal(got["rows"][f][g], w[f], err_msg=f"{what}: option {g}: {f}")
        for f in SUMMARY:
            assert int(got[f][g]) == w["summary"][f], f"{what}: option {g}: {f} = {int(got[f][g])}, want {w['summary'][f]}"
    k = len(want[0]["node"])
    assert int(got["info"][0]) + int(got["info"][1]) == len(want), what
    assert int(got["info"][0]) == int((got["path"] == 0).sum()) and int(got["info"][1]) == int((got["path"] == 1).sum()), what
    assert int(got["info"][2]) == sum(w["summary"]["ok"] == k for w in want), what


def state_before(ref, shapes, shape_of):
    """The [n][4] state a placement reference started from: its ``after`` minus its own Ok placements
    (the parity cases of place_ref keep the results, not the state; the irregular trace's run lengths
    wrap, so the state cannot be rebuilt from the binds by a formula)."""
    state = np.array(ref["after"], np.int64)
    for i, j in enumerate(np.asarray(shape_of).tolist()):
        if ref["status"][i] == pr.OK:
            km = int(shapes["keymask"][j])
            for c in range(3):
                if (km >> c) & 1:
                    state[ref["node"][i], c] -= int(shapes["req"][j][c])
            state[ref["node"][i], 3] -= 1
    assert (state >= 0).all()
    return state


def highest_used(r, n):
    """the highest appended index an option's pods were bound to (any status), -1 if none"""
    nd = np.asarray(r["node"])
    return int(nd.max()) - n if (nd >= n).any() else -1


# ---- the 300-node model of tests/test_scaleup_gpu.py: two scan blocks and a ragged tail -------------
N300, P300, T300 = 300, 600, 600
TICKS300 = (150, 400, 600)
MODES300 = {"feeds": (1, 7, ((1, 1, 0), (2, 1, 0))), "literal": (0, 7, ((1, 1, 0), (2, 1, 0)))}
N_PODS, N_SHAPES = 48, 6
FENCE = 1 << 62      # a taint bit no trace pod tolerates (asserted): the twin engine's appended nodes sit behind it
_models = {}


def model_300(mode):
    """A 600-pod stream on 300 nodes run by the CPU oracle in ``mode``; at TICKS300 the state rebuilt
    from its binds and the reference of 48 preview pods of six of the trace's own shapes for
    ``trace_options``.  Built once per process; nothing in it is changed afterwards."""
    if mode in _models:
        return _models[mode]
    from harness import encoded, make_oracle, small_trace
    tr = small_trace(5, n_nodes=N300, n_pods=P300, arrival="stream", selectors=False)
    p = tr["pods"]
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 997
    enc = encoded(tr)
    assert not (np.asarray(enc["pods"]["tol"], np.uint64) & np.uint64(FENCE)).any()
    assert not (np.asarray(enc["taint"], np.uint64) & np.uint64(FENCE)).any()
    ora = make_oracle(tr, MODES300[mode])
    ora.submit(tr)
    ob, rc = ora.step(T300, cap=T300)
    assert rc == 0 and len(ob["pod"]) > 500
    states = {t: pr.state_from_binds(tr, enc, ob, t) for t in TICKS300}
    assert all(s[:, 3].sum() > 30 for s in states.values())
    ids = distinct_pods(enc, N_SHAPES)
    shapes = {f: np.ascontiguousarray(enc["pods"][f][ids]) for f in ("req", "keymask", "tol", "sel")}
    shape_of = np.array([(5 * i) % N_SHAPES for i in range(N_PODS)], np.int32)
    cfg = pr.engine_cfg(MODES300[mode], enc)
    opts = trace_options(enc)
    refs = {t: scale_up(enc["alloc"], states[t], cfg, shapes, shape_of, opts) for t in TICKS300}
    _models[mode] = dict(tr=tr, enc=enc, ob=ob, states=states, shapes=shapes, shape_of=shape_of, cfg=cfg, opts=opts,
                         refs=refs, mode=MODES300[mode])
    return _models[mode]


def distinct_pods(enc, count, start=0):
    """the first ``count`` pods from ``start`` whose (req, keymask, tol, sel) differ from one another"""
    p = enc["pods"]
    seen, ids = set(), []
    for j in range(start, len(p["keymask"])):
        key = (tuple(int(x) for x in p["req"][j]), int(p["keymask"][j]), int(p["tol"][j]), int(p["sel"][j]))
        if key not in seen:
            seen.add(key)
            ids.append(j)
            if len(ids) == count:
                return ids
    raise AssertionError(f"fewer than {count} distinct shapes")


# ---- the shared options of the 32-node parity trace (tests/test_scaleup_ref.py, test_scaleup_gpu.py) ----
def trace_options(enc):
    """Five templates for an encoded cluster, all of four times the largest node (an empty real node of
    the cluster's own size has the lower index and would win every tie): one every pod may use; one
    that takes two pods per node and runs out; one behind every taint of the cluster; none
    (max_nodes 0); one whose capacities are no multiple of any unit (the milli-unit route)."""
    a = np.asarray(enc["alloc"], np.int64)
    all_labels = int(np.bitwise_or.reduce(np.asarray(enc["label"], np.uint64))) if len(a) else 0
    all_taints = int(np.bitwise_or.reduce(np.asarray(enc["taint"], np.uint64))) if len(a) else 0
    big = [4 * int(a[:, 0].max()), 4 * int(a[:, 1].max()), int(a[:, 2].max()), 110]
    odd = [3 * int(a[:, 0].max()) + 1, 3 * int(a[:, 1].max()) + 1, int(a[:, 2].max()), 110]
    return [option(big, 8, 0, all_labels), option(big[:3] + [2], 3, 0, all_labels), option(big, 5, all_taints or 1, all_labels),
            option(big, 0, 0, all_labels), option(odd, 40, 0, all_labels)]
