"""Times of the drain preview on the C3 cluster after the bench's steady state, beside the two calls
it is measured against: ks_requested_at (the state rebuild it starts from) and
ks_place_at of the first 64 evicted pods given as 64 shapes (one segment's round).  Wall clock around
calls that end in a stream synchronise, the median and the minimum of ``--reps`` calls after one
warm-up call each, every call with its sizing call and its copies to the host; the evicted pods, the
segments and the rounds of each drain are recorded.  Kernel-only times are not taken.

    python tests/dev/drain_times.py [--steps 8] [--reps 20] [--out profiles/drain_times.json]

Drained sets: the first 1, 64 and 1,024 nodes, and the shortest prefix of the nodes that runs about
1,000 pods.  Also cross-checks at this size (196 node workgroups, 1,024 pod blocks): the 64-node
drain equals the integer walk of tests/drain_ref.py over all the nodes, and every drain evicts the
pods requested_at counts on its nodes, in pod order, onto nodes outside the set, with ``after`` =
requested_at with the drained rows zero plus its Ok re-placements.  Prints one JSON line (and writes
it to ``--out``).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-simulator_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(np.min(ts)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--pods-per-step", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--about", type=int, default=1000, help="evicted pods of the largest set")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from kubesim_amd import encode, tracegen
    from kubesim_amd.engine import Engine
    import drain_ref as dr
    import place_ref as pr

    S = args.pods_per_step
    trace = tracegen.c3_trace(n_nodes=args.nodes, n_pods=(args.steps + 1) * S)
    enc = encode.encode_trace(trace)
    mode = (1, 7, ((1, 1, 0), (2, 1, 0)))
    eng = Engine(tick_seconds=trace["tick_seconds"], filter_mode=mode[0], filters=mode[1], scorers=mode[2])
    eng.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    eng.submit(enc["pods"])
    bound = 0
    for _ in range(args.steps):
        bound += len(eng.step(S))
    now = eng.tick
    assert eng.queued > 0 and bound > 0
    r = eng.requested_at(now)
    cfg = pr.engine_cfg(mode, enc)
    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), running_now=int(r[:, 3].sum()),
               requested_at=timed(lambda: eng.requested_at(now), args.reps))

    run = np.cumsum(r[:, 3])
    about = int(np.searchsorted(run, args.about)) + 1
    sets = {"drain_1_node": 1, "drain_64_nodes": 64, "drain_1024_nodes": 1024, "drain_about_%d_pods" % args.about: about}
    first64 = None
    for name, m in sets.items():
        nodes = np.arange(min(m, args.nodes), dtype=np.int32)
        res = eng.drain_at(now, nodes, after=True)
        k = len(res["pod"])
        assert k == int(r[nodes, 3].sum()) and (np.diff(res["pod"]) > 0).all() and np.isin(res["from_node"], nodes).all()
        want = r.copy()
        want[nodes] = 0
        for j, nd, st in zip(res["pod"].tolist(), res["node"].tolist(), res["status"].tolist()):
            if st == 0:
                want[nd, :3] += enc["pods"]["req"][j]
                want[nd, 3] += 1
        assert (res["after"] == want).all() and not np.isin(res["node"], nodes).any()
        if m == 64:
            ref = dr.fast_drain(enc["alloc"], r, cfg, enc["pods"], res["pod"].tolist(), res["from_node"].tolist(), nodes.tolist())
            dr.assert_same(res, ref, name)
        info = res["info"]
        out[name] = dict(nodes=int(len(nodes)), evicted=k, segments=int(info[4]), rounds=int(info[0]), ok=int(info[1]),
                         not_found=int(info[3]), idle_nodes=int(info[5]),
                         **timed(lambda: eng.drain_at(now, nodes, after=True), args.reps))
        if k >= 64:
            first64 = res["pod"][:64]
    if first64 is not None:
        sh = {f: np.ascontiguousarray(enc["pods"][f][first64]) for f in ("req", "keymask", "tol", "sel")}
        res = eng.place_at(now, sh)
        out["place_first_64_evicted_as_64_shapes"] = dict(rounds=int(res["info"][0]), ok=int(res["info"][1]),
                                                          **timed(lambda: eng.place_at(now, sh), args.reps))
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
