"""Times of the removal scan on the C3 cluster after the bench's steady state, beside its yardstick
(DESIGN.md §3.6): a loop of ``drain_at(t, [c])`` over the same candidates on the same engine in the
same session.  Wall clock around calls that end in a stream synchronise, the median and the minimum
of ``--reps`` calls after one warm-up call each, every call with its copies to the host (the scan
without rows: the summaries are the answer; one figure with rows beside it); the loop's figure is
the time of one whole pass over the candidates (``--loop-reps`` passes).  Kernel-only times are not
taken here (``--scan-only`` runs the scans alone, for a kernel trace).

    python tests/dev/removable_times.py [--steps 8] [--reps 20] [--out profiles/removable_times.json]

Candidate sets: the first 64 and the first 1,024 occupied nodes, and every occupied node.  Also
cross-checks at this size: every set's scan equals the loop's answers row for row, and the first 64
equal the integer walk of tests/removable_ref.py.  Prints one JSON line (and writes it to ``--out``).
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
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(np.min(ts)), 4), reps=reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50_000)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--pods-per-step", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-reps", type=int, default=20, help="passes of the single-drain loop over a set")
    ap.add_argument("--scan-only", action="store_true", help="no loop, no cross-checks: the scans alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from kubesim_amd import encode, tracegen
    from kubesim_amd.engine import Engine
    import drain_ref as dr
    import place_ref as pr
    import removable_ref as rr

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
    occupied = np.nonzero(r[:, 3] > 0)[0].astype(np.int32)
    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), running_now=int(r[:, 3].sum()),
               occupied_nodes=int(len(occupied)), most_pods_on_a_node=int(r[:, 3].max()))

    sets = {"first_64_occupied": occupied[:64], "first_1024_occupied": occupied[:1024], "every_occupied_node": occupied}
    for name, nodes in sets.items():
        res = eng.removable_at(now, nodes, rows=True)
        info = res["info"]
        assert (res["evicted"] == r[nodes, 3]).all() and info[5] == int(r[nodes, 3].sum())
        row = dict(candidates=int(len(nodes)), evicted=int(info[5]), segments=int(info[0]), batched=int(info[1]),
                   single_drain=int(info[2]), removable=int(info[4]))
        row["scan"] = timed(lambda: eng.removable_at(now, nodes), args.reps)
        row["scan_with_rows"] = timed(lambda: eng.removable_at(now, nodes, rows=True), args.reps)
        if row["segments"]:
            row["scan_ms_per_segment"] = round(row["scan"]["median_ms"] / row["segments"], 4)
        if not args.scan_only:
            def loop():
                return [eng.drain_at(now, [int(c)]) for c in nodes]
            # the loop's answers are the scan's, row for row
            for j, one in enumerate(loop()):
                a, b = int(res["first_row"][j]), int(res["first_row"][j] + res["evicted"][j])
                for f in dr.FIELDS:
                    assert (res["rows"][f][a:b] == one[f]).all(), (name, j, f)
                assert [res["ok"][j], res["over_capacity"][j], res["not_found"][j]] == one["info"][1:4].tolist()
            row["single_drain_loop"] = timed(loop, args.loop_reps)
            row["loop_ms_per_candidate"] = round(row["single_drain_loop"]["median_ms"] / len(nodes), 4)
            row["loop_over_scan"] = round(row["single_drain_loop"]["median_ms"] / row["scan"]["median_ms"], 2)
            if len(nodes) == 64:
                cfg = pr.engine_cfg(mode, enc)
                per = []
                for j, c in enumerate(nodes.tolist()):
                    a, b = int(res["first_row"][j]), int(res["first_row"][j] + res["evicted"][j])
                    assert (res["rows"]["from_node"][a:b] == c).all() and (np.diff(res["rows"]["pod"][a:b]) > 0).all()
                    per.append(dr.fast_drain(enc["alloc"], r, cfg, enc["pods"], res["rows"]["pod"][a:b].tolist(), [c] * (b - a), [c]))
                rr.assert_same(res, rr.assemble(nodes.tolist(), per), name)
        out[name] = row
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
