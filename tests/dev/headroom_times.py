"""Times of the headroom queries on the C3 cluster after the bench's steady state, beside the state
queries they build on: wall clock around calls that end in a stream synchronise,
the median and the minimum of ``--reps`` calls after one warm-up call each, every call with its
copy to the host.

    python tests/dev/headroom_times.py [--steps 8] [--reps 20] [--out profiles/headroom_times.json]

Shapes are the trace's first pods.  Also cross-checks at this size (196 node workgroups, many
candidate blocks): the series against headroom_at at three ticks of the window, the per-node counts
against the columns, and a shape's count against requested_at in plain integers on a few nodes.
Prints one JSON line (and writes it to ``--out``).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-simulator_amd"))


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
    eng = Engine(tick_seconds=trace["tick_seconds"], filter_mode=1, filters=7, scorers=((1, 1, 0), (2, 1, 0)))
    eng.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    eng.submit(enc["pods"])
    bound = 0
    for _ in range(args.steps):
        bound += len(eng.step(S))
    now = eng.tick
    lo, hi = now - S + 1, now + 1
    assert eng.queued > 0 and bound > 0

    def shapes(k):
        return {f: enc["pods"][f][:k] for f in ("req", "keymask", "tol", "sel")}

    # cross-checks at this size
    s8 = shapes(8)
    series = eng.headroom_series(lo, hi, s8)
    for t in (lo, lo + S // 3, now):
        cols, pn = eng.headroom_at(t, s8, per_node=True)
        assert (series[t - lo] == cols[:, :2]).all(), t
        assert (cols[:, 0] == pn.sum(axis=1, dtype=np.int64)).all() and (cols[:, 1] == (pn >= 1).sum(axis=1)).all()
        assert (cols[:, 2] == pn.max(axis=1)).all() and (cols[:, 3] == np.where(cols[:, 2] > 0, pn.argmax(axis=1), -1)).all()
        assert (cols[:, 4:].sum(axis=1) == args.nodes).all()
    r = eng.requested_at(now)
    cols, pn = eng.headroom_at(now, s8, per_node=True)
    for nd in (0, 1, 255, 256, args.nodes - 1):
        for j in range(8):
            ok = (int(enc["taint"][nd]) & ~int(s8["tol"][j])) == 0 and (int(enc["label"][nd]) & int(s8["sel"][j])) == int(s8["sel"][j])
            b = [max(int(enc["alloc"][nd, 3]) - int(r[nd, 3]), 0)]
            for k in range(3):
                if (int(s8["keymask"][j]) >> k) & 1:
                    A, q = int(enc["alloc"][nd, k]), int(s8["req"][j, k])
                    if A < 0:
                        b.append(0)
                    elif q > 0:
                        b.append((A - int(r[nd, k])) // q)
            assert int(pn[j, nd]) == (min(min(b), 2**31 - 1) if ok else 0), (nd, j)

    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), window=[int(lo), int(hi)],
               running_now=int(r[:, 3].sum()),
               requested_at=timed(lambda: eng.requested_at(now), args.reps),
               node_peaks=timed(lambda: eng.node_peaks(lo, hi), args.reps),
               cluster_series=timed(lambda: eng.cluster_series(lo, hi), args.reps))
    for k in (1, 8, 64):
        sk = shapes(k)
        out[f"headroom_at_k{k}"] = timed(lambda: eng.headroom_at(now, sk), args.reps)
        out[f"headroom_at_k{k}_per_node"] = timed(lambda: eng.headroom_at(now, sk, per_node=True), args.reps)
    for k in (1, 8):
        sk = shapes(k)
        out[f"headroom_series_k{k}"] = timed(lambda: eng.headroom_series(lo, hi, sk), args.reps)
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
