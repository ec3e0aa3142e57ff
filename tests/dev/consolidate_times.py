"""Times of the consolidation preview on the C3 cluster after the bench's steady state, beside its
yardsticks.  No existing call gives the same answer; the yardsticks are existing code
on the same engine and candidates in the same session: ``removable_at`` (the same gather and lists,
independent answers) and a loop of ``drain_at(t, [c])``.  Wall clock around calls that end in a
stream synchronise, the median and the minimum of ``--reps`` calls after one warm-up call each, every
call with its copies to the host; the loop's figure is the time of one whole pass over the candidates
(``--loop-reps`` passes).  Kernel-only times are not taken here (``--calls-only`` runs the
consolidation calls alone, for a kernel trace).

    python tests/dev/consolidate_times.py [--steps 8] [--reps 20] [--out profiles/consolidate_times.json]

Candidate sets: the first 64 and the first 1,024 occupied nodes, and every occupied node, ascending.
Also cross-checks at this size: the first 64 equal the integer chain of tests/consolidate_ref.py, every
set's first candidate equals ``drain_at`` truncated, and the column sums of ``after`` are the state's.
Prints one JSON line (and writes it to ``--out``).
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
    ap.add_argument("--loop-reps", type=int, default=5, help="passes of the single-drain loop over a set")
    ap.add_argument("--calls-only", action="store_true", help="no yardsticks, no cross-checks: the calls alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from kubesim_amd import encode, tracegen
    from kubesim_amd.engine import Engine
    import consolidate_ref as cr
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
    occupied = np.nonzero(r[:, 3] > 0)[0].astype(np.int32)
    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), running_now=int(r[:, 3].sum()),
               occupied_nodes=int(len(occupied)), most_pods_on_a_node=int(r[:, 3].max()))

    sets = {"first_64_occupied": occupied[:64], "first_1024_occupied": occupied[:1024], "every_occupied_node": occupied}
    for name, nodes in sets.items():
        res = eng.consolidate_at(now, nodes, rows=True, after=True)
        info = res["info"]
        assert (res["evicted"] == r[nodes, 3]).all() and res["evicted_total"] == int(r[nodes, 3].sum())
        assert (res["after"].sum(axis=0) == r.sum(axis=0)).all()
        row = dict(candidates=int(len(nodes)), evicted=int(res["evicted_total"]), rounds=int(info[0]), removed=int(info[1]),
                   blocked=int(info[2]), destinations=int(info[3]), single_path=int(info[4]), pods_moved=int(info[5]))
        row["consolidate"] = timed(lambda: eng.consolidate_at(now, nodes, rows=False), args.reps)
        row["consolidate_with_rows"] = timed(lambda: eng.consolidate_at(now, nodes, rows=True), args.reps)
        row["consolidate_ms_per_round"] = round(row["consolidate"]["median_ms"] / max(row["rounds"], 1), 4)
        if not args.calls_only:
            row["removable_scan"] = timed(lambda: eng.removable_at(now, nodes), args.reps)

            def loop():
                return [eng.drain_at(now, [int(c)]) for c in nodes]
            row["single_drain_loop"] = timed(loop, args.loop_reps)
            row["loop_over_consolidate"] = round(row["single_drain_loop"]["median_ms"] / row["consolidate"]["median_ms"], 2)
            row["consolidate_over_removable"] = round(row["consolidate"]["median_ms"] / row["removable_scan"]["median_ms"], 2)
            # the first candidate of the chain is its drain, truncated after the first pod not bound Ok
            one = eng.drain_at(now, [int(nodes[0])])
            keep = int(res["n_rows"][0])
            for f in dr.FIELDS:
                assert (res["rows"][f][:keep] == one[f][:keep]).all(), (name, f)
            if len(nodes) == 64:
                alone = eng.removable_at(now, nodes, rows=True)
                running = {int(c): alone["rows"]["pod"][int(alone["first_row"][j]):int(alone["first_row"][j] + alone["evicted"][j])].tolist()
                           for j, c in enumerate(nodes.tolist())}
                want = cr.fast_consolidate(None, enc, None, pr.engine_cfg(mode, enc), now, nodes.tolist(), state=r, running=running)
                cr.assert_same(res, want, name)
        out[name] = row
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
