"""Times of the scale-up preview on the C3 cluster after the bench's steady state:
1, 8 and 64 options x 64 and 1,024 pods, beside a loop of ``n_options`` existing ``Engine.place_at``
calls with the same pods on the same engine in the same session — existing code, and a lower bound
for a loop of per-option previews (it scans the cluster once per option and appends nothing).  Wall
clock around calls that end in a stream synchronise, the median and the minimum of ``--reps`` calls
after one warm-up call each.  Each call's share of batched and single-path options is recorded.

    python tests/dev/scaleup_times.py [--steps 8] [--reps 20] [--out profiles/scaleup_times.json]

Two kinds of pods: ``own`` — the trace's first 8 shapes, which fit the cluster (a template only ties
with the empty real nodes, so 1,024 of them use up their lists and every option takes the single
path); ``pending`` — the same shapes asking for more cpu than any real node has, the intended use:
they fit the template alone.  Cross-check at this size: every batched option of the 64-pod ``own`` call
equals tests/scaleup_ref.py on the 50,000 nodes.  Prints one JSON line (and writes it to ``--out``).
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from kubesim_amd import encode, tracegen
    from kubesim_amd.engine import Engine

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

    a = np.asarray(enc["alloc"], np.int64)
    labels = int(np.bitwise_or.reduce(np.asarray(enc["label"], np.uint64)))
    own = {f: np.ascontiguousarray(enc["pods"][f][:8]) for f in ("req", "keymask", "tol", "sel")}
    pending = {f: v.copy() for f, v in own.items()}
    pending["req"][:, 0] = int(a[:, 0].max()) + 1000          # more cpu than any real node has
    pending["keymask"] |= 1
    pending["sel"][:] = 0
    pending["tol"][:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    # G templates of eight to eleven times the largest node, up to 1,024 copies each
    def options(G):
        return [dict(alloc=[(8 + g % 4) * int(a[:, 0].max()), 8 * int(a[:, 1].max()), int(a[:, 2].max()), 110], taint=0,
                     label=labels, max_nodes=1024) for g in range(G)]

    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), running_now=int(eng.requested_at(now)[:, 3].sum()))
    # cross-check at this size
    import place_ref as pr
    import scaleup_ref as sr
    so64 = (np.arange(64) % 8).astype(np.int32)
    got = eng.scale_up_at(now, own, options(2), so64, rows=True)
    want = sr.scale_up(a, eng.requested_at(now), pr.engine_cfg(mode, enc), own, so64, options(2))
    sr.assert_same(got, want, what="64 pods on C3")

    for kind, shapes in (("own", own), ("pending", pending)):
        for k in (64, 1024):
            so = (np.arange(k) % 8).astype(np.int32)
            p = eng.place_at(now, shapes, so)
            loop1 = timed(lambda: eng.place_at(now, shapes, so), args.reps)
            for G in (1, 8, 64):
                opts = options(G)
                res = eng.scale_up_at(now, shapes, opts, so)
                row = dict(kind=kind, k=k, options=G, batched=int(res["info"][0]), single=int(res["info"][1]),
                           all_ok=int(res["info"][2]), on_new=int(res["on_new"].sum()), nodes_used=int(res["nodes_used"].max()),
                           place_at_rounds=int(p["info"][0]), place_at_ok=int(p["info"][1]))
                row["scale_up"] = timed(lambda: eng.scale_up_at(now, shapes, opts, so), args.reps)
                row["scale_up_rows"] = timed(lambda: eng.scale_up_at(now, shapes, opts, so, rows=True), max(args.reps // 4, 3))
                row["place_at_once"] = loop1
                row["place_at_loop"] = timed(lambda: [eng.place_at(now, shapes, so) for _ in range(G)],
                                             args.reps if G < 64 else max(args.reps // 4, 3))
                row["loop_over_scale_up"] = round(row["place_at_loop"]["median_ms"] / row["scale_up"]["median_ms"], 2)
                out[f"{kind}_{k}_pods_{G}_options"] = row
    eng.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
