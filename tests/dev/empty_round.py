"""Dev tool (not a test): what an empty round costs (the two-launch chain's rescan).

    rocprofv3 --kernel-trace -d DIR -o run -- python tests/dev/empty_round.py
        four 32,768-pod steps of the C3 cluster with KS_ENGINE_SMALL_E: every overlapped batch
        overflows E, so every second round is empty; prints pods, launches, rescans per step
    python tests/dev/empty_round.py summary DIR/run_results.db OUT.txt
        the trace's merge_cl -> chunk_scan rounds split into empty ones (a no-op merge_cl, < 6 us) and
        real ones: per class the mean merge_cl, gap, chunk_scan and gap after"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "kubernetes-simulator_amd"))


def run():
    from kubesim_amd import _lib, encode, tracegen
    from kubesim_amd.engine import Engine
    tr = tracegen.c3_trace(n_pods=4 * 32768)
    enc = encode.encode_trace(tr)
    eng = Engine(tick_seconds=tr["tick_seconds"], filter_mode=1, filters=7, scorers=((1, 1, 0), (2, 1, 0)),
                 engine_flags=_lib.KS_ENGINE_SMALL_E)
    eng.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    eng.submit(enc["pods"])
    for _ in range(4):
        b = eng.step(32768)
        print(len(b), eng.last_step_stats()["launches"], int(eng.debug_counters()[5]))
    eng.close()


def summary(db, out):
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    ks = sorted((float(s), float(e), n) for n, s, e in c.execute("select name, start, end from kernels"))
    rows = {"empty": [], "real": []}
    for (s0, e0, n0), (s1, e1, n1), (s2, _, n2) in zip(ks, ks[1:], ks[2:]):
        if "merge_cl_kernel" in n0 and "chunk_scan_kernel" in n1 and "merge_cl_kernel" in n2:
            rows["empty" if e0 - s0 < 6000 else "real"].append((e0 - s0, s1 - e0, e1 - s1, s2 - e1))
    with open(out, "w") as f:
        for k, v in rows.items():
            if not v:
                f.write(f"{k} rounds: none\n")
                continue
            m = [statistics.mean(x[j] for x in v) / 1e3 for j in range(4)]
            f.write(f"{k} rounds: {len(v)} x merge_cl {m[0]:.2f} us, gap {m[1]:.2f}, chunk_scan {m[2]:.2f}, "
                    f"gap {m[3]:.2f}, round {sum(m):.2f} us\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "summary":
        summary(sys.argv[2], sys.argv[3])
    else:
        run()
