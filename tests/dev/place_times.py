"""Times of the placement preview on the C3 cluster after the bench's steady state, beside the two
queries it is measured against: ks_score_at of the last bound pod (the same state
rebuild plus one pass over the nodes) and ks_headroom_at with one shape.  Wall clock around calls
that end in a stream synchronise, the median and the minimum of ``--reps`` calls after one warm-up
call each, every call with its copy to the host; the rounds of each preview are recorded.

    python tests/dev/place_times.py [--steps 8] [--reps 20] [--lib libks_engine_pl8.so] [--copies-only]
                                    [--out profiles/place_times.json]

``--lib`` takes a diagnostic build (make -C kubernetes-simulator_amd/csrc variant NAME=pl8
DEFS=-DKS_PLACE_L=8, tests/dev/devlib.py) for the kPlaceL comparison; ``--copies-only`` times the
1,024-copies case alone.  Shapes are the trace's first pods.  Also cross-checks at this size (196
node workgroups): the Ok placements add up to ``after`` - requested_at, 16 pods of 16 shapes equal the
integer walk of tests/place_ref.py over all the nodes, and 1,024 copies of a shape place as many Ok
as ks_headroom_at's total allows.  Prints one JSON line (and writes it to ``--out``).
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
    ap.add_argument("--lib", default=None)
    ap.add_argument("--copies-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from kubesim_amd import _lib, encode, tracegen
    if args.lib:
        from devlib import lib_path
        _lib.LIB_PATH = lib_path(args.lib)
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
        binds = eng.step(S)
        bound += len(binds)
    now = eng.tick
    assert eng.queued > 0 and bound > 0
    last_pod = int(binds["pod"][-1])

    def shapes(k):
        return {f: enc["pods"][f][:k] for f in ("req", "keymask", "tol", "sel")}

    copies = np.zeros(1024, np.int32)
    out = dict(nodes=args.nodes, tick=int(now), bound=int(bound), lib=args.lib or "libks_engine.so")

    def place(name, k, sh, so):
        res = eng.place_at(now, sh, so)
        out[name] = dict(k=k, shapes=len(sh["keymask"]), rounds=int(res["info"][0]), ok=int(res["info"][1]),
                         not_found=int(res["info"][3]), **timed(lambda: eng.place_at(now, sh, so), args.reps))

    if not args.copies_only:
        # cross-checks at this size
        import place_ref as pr
        r = eng.requested_at(now)
        cfg = pr.engine_cfg(mode, enc)
        s8 = shapes(8)
        so = (np.arange(1024) % 8).astype(np.int32)
        res = eng.place_at(now, s8, so, after=True)
        add = np.zeros_like(r)
        for j, nd, st in zip(so.tolist(), res["node"].tolist(), res["status"].tolist()):
            if st == 0:
                add[nd, :3] += np.where((int(s8["keymask"][j]) >> np.arange(3)) & 1, s8["req"][j], 0)
                add[nd, 3] += 1
        assert (res["after"] == r + add).all() and res["info"][1] == (res["status"] == 0).sum() > 0
        # 16 pods of 16 shapes against the integer walk over all 50,000 nodes
        s64 = shapes(64)
        ref = pr.fast_place(enc["alloc"], r, cfg, shapes(16))
        pr.assert_same(eng.place_at(now, shapes(16), after=True), ref, "16 shapes on C3")
        # 1,024 copies of one shape: as many Ok as the cluster's headroom allows
        s1 = shapes(1)
        res = eng.place_at(now, s1, copies)
        head = eng.headroom_at(now, s1)
        assert res["info"][1] == min(1024, head[0, 0]) and res["candidates"][0] == head[0, 1]

        out["running_now"] = int(r[:, 3].sum())
        out["requested_at"] = timed(lambda: eng.requested_at(now), args.reps)
        out["score_at_last_pod"] = timed(lambda: eng.score_at(last_pod), args.reps)
        out["headroom_at_k1"] = timed(lambda: eng.headroom_at(now, s1), args.reps)
        place("place_1_pod_1_shape", 1, s1, None)
        place("place_64_copies_1_shape", 64, s1, np.zeros(64, np.int32))
        place("place_64_pods_64_shapes", 64, s64, None)
        out["place_64_single_calls"] = timed(lambda: [eng.place_at(now, s1) for _ in range(64)], max(args.reps // 4, 3))
    place("place_1024_copies_1_shape", 1024, shapes(1), copies)
    if not args.copies_only:
        place("place_1024_pods_8_shapes", 1024, shapes(8), (np.arange(1024) % 8).astype(np.int32))
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
