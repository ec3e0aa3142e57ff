"""Times of the past-tick state queries on the C3 cluster after the bench's steady state, beside
the calls they are compared with: wall clock around calls that end in a stream
synchronise, the median and the minimum of ``--reps`` calls after one warm-up call each.

    python tests/dev/query_times.py [--steps 8] [--reps 20]

Also cross-checks the queries against each other at this size (many candidate blocks): the series'
requested columns and the peaks of a one-tick window against requested_at, the peaks of a 64-tick
window against the max of 64 requested_at calls.  Prints one JSON line.
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

    # cross-checks at this size
    series = eng.cluster_series(lo, hi)
    for t in (lo, lo + S // 3, now):
        r = eng.requested_at(t)
        assert (series[t - lo, 0] == r[:, 3].sum()) and (series[t - lo, 1:4] == r[:, :3].sum(axis=0)).all(), t
        assert (eng.node_peaks(t, t + 1) == r).all(), t
    w = np.stack([eng.requested_at(t) for t in range(now - 63, now + 1)]).max(axis=0)
    assert (eng.node_peaks(now - 63, now + 1) == w).all()
    peaks = eng.node_peaks(lo, hi)
    assert (peaks >= w).all()
    sc = eng.score_at(bound - 1)
    node = int(eng.pod_status(bound - 1, 1)["node"][0])
    assert int(np.argmax(sc)) == node

    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), window=[int(lo), int(hi)],
               running_now=int(series[-1, 0]), running_at_window_start=int(series[0, 0]),
               peak_pods_per_node=int(peaks[:, 3].max()),
               usage_at=timed(lambda: eng.usage_at(now), args.reps),
               requested_at=timed(lambda: eng.requested_at(now), args.reps),
               score_queued=timed(lambda: eng.score(bound), args.reps),
               score_at=timed(lambda: eng.score_at(bound - 1), args.reps),
               filter_at=timed(lambda: eng.filter_at(bound - 1), args.reps),
               usage_digest=timed(lambda: eng.usage_digest(lo, hi), args.reps),
               cluster_series=timed(lambda: eng.cluster_series(lo, hi), args.reps),
               node_peaks=timed(lambda: eng.node_peaks(lo, hi), args.reps))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
