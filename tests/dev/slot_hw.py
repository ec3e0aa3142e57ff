"""Dev tool (not a test): candidate-slot high-water marks and the between-step invariants
(ks_debug_invariants) of chunk-resolver engines at the bench's configurations — which of them claim
more than kSlotMax candidate slots in a batch (the round-6 slot_node overflow, ks_device.h WinWS).
KS_LIB selects a build (tests/dev/devlib.py).  The suite that does pass kSlotMax under the oracle is
tests/test_candidate_capacity_gpu.py."""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from devlib import lib_path  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "kubernetes-simulator_amd"))
from kubesim_amd import _lib  # noqa: E402
_lib.LIB_PATH = lib_path(os.environ.get("KS_LIB", "libks_engine.so"))
from kubesim_amd import encode, tracegen  # noqa: E402
from kubesim_amd.engine import Engine, LocalExchange  # noqa: E402

SC = ((1, 1, 0), (2, 1, 0))
W = 32768


def one(tr, enc, steps, flags=0):
    e = Engine(tick_seconds=10, filter_mode=1, filters=7, scorers=SC, engine_flags=flags)
    e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    e.submit(enc["pods"])
    for s in range(steps):
        e.step(W)
        print(f"   step {s}: {e.debug_invariants()}", flush=True)
    e.close()


def ranks(tr, enc, world, steps):
    x = LocalExchange(world)
    es = []
    for r in range(world):
        e = Engine(tick_seconds=10, filter_mode=1, filters=7, scorers=SC)
        e.shard_host(world, r, x, 1)
        e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
        e.submit(enc["pods"])
        es.append(e)
    for s in range(steps):
        th = [threading.Thread(target=es[r].step, args=(W,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        print(f"   step {s}: rank 0 {es[0].debug_invariants()}", flush=True)
    for e in es:
        e.close()


which = sys.argv[1:] or ["c3", "c5", "c5w8", "c5w16"]
if "c3" in which:
    tr = tracegen.c3_trace(n_pods=3 * W)
    enc = encode.encode_trace(tr)
    print("C3 (overlap)", flush=True)
    one(tr, enc, 3)
    print("C3 (plain chain)", flush=True)
    one(tr, enc, 2, _lib.KS_ENGINE_NO_OVERLAP)
if any(w.startswith("c5") for w in which):
    tr = tracegen.c5_trace(n_pods=2 * W)
    enc = encode.encode_trace(tr)
    if "c5" in which:
        print("C5 unsharded", flush=True)
        one(tr, enc, 2)
    for w in (8, 16):
        if f"c5w{w}" in which:
            print(f"C5 {w} ranks", flush=True)
            ranks(tr, enc, w, 2)
