"""The batched step above 65,536 nodes: the traces and cached oracle runs of tests/test_width_gpu.py,
and the properties of those runs that tests/test_width_cases.py pins on the oracle alone.

The device code of ks_step changes its path by cluster width (a scan block is 256 nodes):

    65,536 nodes   the role-split resolver's touched filter (ks_rolesplit.hip, kFilterBits) is exact up to
                   here; above, nodes x and x + 65,536 share a filter bit, a set bit is confirmed in the
                   hash, and every in-loop winner is hash-inserted;
    256 blocks     merge_kernel (ks_scan.hip) folds one block list per thread up to here, the lists
                   tid, tid + 256, ... above; from 1,025 lists on it runs 1,024 threads;
    256 blocks     the last two-launch plan of an unsharded engine (ks_plan.h kOverlapMaxBlocks): the
                   plain chain and lists of kTopL keys above;
    1,024 blocks   pruned block lists by default (ks_step.cpp kPruneMinBlocks);
    1,024 nodes    one workgroup of tick_kernel (ks_tick.hip).

WIDTHS puts a cluster on either side of each.  The best nodes are planted by hand: every node gets
the smallest cpu and memory choice, the planted ones the largest, so LeastRequested and
BalancedAllocation bind on planted nodes only.  The planted nodes are alias groups — x, x + 65,536,
x + 131,072, ... as far as the cluster goes — whose members share a filter bit and lie in different
trips of the merge.

Nothing here imports the engine.  Traces and oracle runs are built once per process and never
changed afterwards.
"""
from __future__ import annotations

import functools
import os
import time

import numpy as np

import weight_cases
from harness import encoded, make_oracle, small_trace
from kubesim_amd import tracegen

BLK = 256                    # nodes per scan block (ks::block_nodes())
ALIAS = 1 << 16              # the touched filter's bits (ks_rolesplit.hip kFilterBits)
MERGE_NARROW, MERGE_WIDE = 256, 1024   # merge_kernel's threads: 1,024 from 1,025 lists on
PRUNE_MIN_BLOCKS = 1024      # ks_step.cpp KS_PRUNE_MIN_BLOCKS
OVERLAP_MAX_BLOCKS = 256     # ks_plan.h KS_OVERLAP_MAX_BLOCKS
TICK_WG_NODES = 1024         # ks_tick.hip kTickThreads * kTickNodes
WIDTHS = {"b256": 65_536, "b257a": 65_537, "b257": 65_792, "b513": 131_328, "b1023": 261_888,
          "b1024": 262_144, "b1025": 262_400}
MODE = "feeds_all_lrba"
SEED, N_PODS, WINDOW = 11, 768, 192
STEPS = (300, 473)           # the two uneven steps of every batched run
TICK_STEPS = 96              # the per-tick kernel's share of its run
CUTS = (TICK_STEPS, STEPS[0], sum(STEPS))    # the ticks at which an oracle run records its usage
FALLBACK = ("b257", "b513")  # also run under weight_cases' w16p scorers: no chunk resolver, no flag
MORE_SEEDS = (("b257", 12), ("b513", 12))
SHARD_WIDTHS = ("b257", "b1025")             # three virtual shards: 85 / 86 / 86 and 341 / 342 / 342 blocks
TICK_WIDTHS = ("b257a", "b513", "b1025")     # the per-tick kernel: 65, 129 and 257 evaluating workgroups

# The alias groups' lowest members.  LOW: offsets in block 0, so that the group reaches block 256 (b257),
# block 512 (b513) and block 1,024 (b1025): the word and wave edges first.  SPREAD: (block, offset) in
# blocks 1 .. 255, the last two blocks first: their groups reach the last blocks of b256, b1023 and
# b1024.  A width takes a prefix of each (GROUPS), about fifty planted nodes in all: ties go to the
# lowest index, so a run uses the lowest planted nodes that hold its running pods and no others.
LOW = (0, 255, 64, 5, 63, 128, 31, 200, 32, 127, 192, 100, 1, 254, 33, 65, 77, 129, 150, 191, 222, 240, 250, 253)
SPREAD = tuple(b * BLK + o for b, o in (
    (254, 3), (255, 0), (254, 200), (255, 255), (254, 255), (255, 128), (37, 130), (128, 64), (200, 255), (1, 0),
    (100, 7), (255, 63), (2, 74), (17, 117), (50, 58), (64, 64), (99, 79), (127, 91), (129, 165), (160, 32),
    (191, 155), (192, 192), (222, 22), (253, 145)))
# name: (groups from LOW, groups from SPREAD).  b257a has one node past the filter's range: few planted
# nodes, so that nodes 0 and 65,536 take dozens of binds each
GROUPS = {"b256": (24, 24), "b257a": (4, 10), "b257": (24, 4), "b513": (10, 9), "b1023": (4, 8), "b1024": (4, 8),
          "b1025": (9, 3)}
PHASE_STEP = 120             # phases of 1 .. 1,321 seconds: some sixty pods run at a time


def blocks_of(name):
    return -(-WIDTHS[name] // BLK)


def trip_blocks(name):
    """the blocks of one trip of merge_kernel's fold loop: its thread count"""
    return MERGE_WIDE if blocks_of(name) > MERGE_WIDE else MERGE_NARROW


def trips_of(name):
    return -(-blocks_of(name) // trip_blocks(name))


def trip_of(name, node):
    return np.asarray(node) // BLK // trip_blocks(name)


def planted(name):
    """the planted nodes of a width, ascending: every member x + k * 65,536 below n of every group"""
    n = WIDTHS[name]
    lo, sp = GROUPS[name]
    xs = LOW[:lo] + SPREAD[:sp]
    return sorted({x + k * ALIAS for x in xs for k in range(-(-n // ALIAS)) if x + k * ALIAS < n})


def alias_groups(name):
    """the planted alias groups of more than one node: lists of nodes with one filter bit"""
    g = {}
    for x in planted(name):
        g.setdefault(x % ALIAS, []).append(x)
    return [v for v in g.values() if len(v) > 1]


@functools.lru_cache(maxsize=None)
def width_trace(name, seed=SEED):
    """(trace, encoded trace): 768 pods that all arrive at tick 1, one bound per tick"""
    n = WIDTHS[name]
    tr = small_trace(seed, n_nodes=n, n_pods=N_PODS, taints=False, selectors=False, tolerations=False)
    nd, p = tr["nodes"], tr["pods"]
    nd["alloc"][:, tracegen.CPU] = tracegen.CPU_CHOICES[0]
    nd["alloc"][:, tracegen.MEM] = tracegen.MEM_CHOICES[0]
    pl = planted(name)
    nd["alloc"][pl, tracegen.CPU] = tracegen.CPU_CHOICES[-1]
    nd["alloc"][pl, tracegen.MEM] = tracegen.MEM_CHOICES[-1]
    # every planted node carries gpus: a pod that asks for one is not pushed off the planted set
    nd["alloc"][pl, tracegen.GPU] = tracegen.GPU_CHOICES[-1]
    nd["alloc_has"][pl] = 15
    # expiries land on planted nodes inside later batches
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) % 12) * PHASE_STEP
    return tr, encoded(tr)


def mode_of(scorers=None):
    return MODE if scorers is None else weight_cases.mode(scorers)


@functools.lru_cache(maxsize=None)
def oracle_run(name, scorers=None, seed=SEED):
    """The oracle's run of a width, once: dict(binds (the whole run), usage {tick: [n][3]} at CUTS, rc,
    seconds).  scorers: a weight_cases.CLASSES name instead of MODE's."""
    tr, _ = width_trace(name, seed)
    t0 = time.perf_counter()
    ora = make_oracle(tr, mode_of(scorers))
    ora.set_threads(int(os.environ.get("OMP_NUM_THREADS") or 0) or min(os.cpu_count() or 1, 16))
    ora.submit(tr)
    parts, usage, rc, at = [], {}, 0, 0
    for t in CUTS:
        b, rc = ora.step(t - at, cap=t - at)
        assert rc == 0, f"{name}: the oracle stopped with {rc}"
        parts.append(b)
        usage[t] = ora.usage().copy()
        at = t
    ora.close()
    binds = {f: np.concatenate([b[f] for b in parts]) for f in ("pod", "node", "tick", "status")}
    return dict(binds=binds, usage=usage, rc=rc, seconds=time.perf_counter() - t0)


def binds_between(binds, lo, hi):
    """the binds of the ticks lo < tick <= hi"""
    a, z = np.searchsorted(binds["tick"], [lo, hi], side="right")
    return {f: v[a:z] for f, v in binds.items()}


@functools.lru_cache(maxsize=None)
def small_member():
    """the what-if group's second member: 2,000 nodes; (trace, encoded trace, its oracle's binds and usage
    after sum(STEPS) ticks)"""
    tr = small_trace(SEED, n_nodes=2000, n_pods=N_PODS, taints=False, selectors=False, tolerations=False)
    tr["pods"]["phase_sec"][:] = 1 + (np.arange(len(tr["pods"]["phase_sec"])) % 12) * PHASE_STEP
    ora = make_oracle(tr, MODE)
    ora.submit(tr)
    b, rc = ora.step(sum(STEPS), cap=sum(STEPS))
    assert rc == 0
    usage = ora.usage().copy()
    ora.close()
    return tr, encoded(tr), b, usage


# ---- the properties of a run, from the oracle's binds alone ------------------------------------------
def events(name, scorers=None, seed=SEED):
    """Over the nominal 192-pod windows of the FIFO.  A fresh win is an Ok bind on a node that no earlier
    pod of the same window was bound to: only a fresh win reaches the resolver through the merged
    lists (a touched node is re-evaluated whatever the merge did).  An alias while untouched is a
    fresh win on w when another node with w's filter bit was already bound in the window; an alias
    both touched is a bind on an already bound w when such a node is bound too.

    dict(ok, on_planted, binds_on {node: binds}, fresh (nodes, one array per window), untouched, both,
    fresh_per_trip, fresh_last_block, trips_per_window, full_groups (per window the alias groups whose
    every member is bound in it), pair_windows (windows that bind both node 0 and node 65,536))"""
    b = oracle_run(name, scorers, seed)["binds"]
    ok = b["status"] == 0
    pl = set(planted(name))
    fresh, untouched, both, full, pair = [], 0, 0, [], []
    for w0 in range(0, N_PODS, WINDOW):
        sel = (b["pod"] >= w0) & (b["pod"] < w0 + WINDOW) & ok
        seen, bits, fw = set(), {}, []
        for node in b["node"][sel].tolist():
            others = bits.get(node % ALIAS, set()) - {node}
            if node not in seen:
                fw.append(node)
                untouched += bool(others)
            else:
                both += bool(others)
            seen.add(node)
            bits.setdefault(node % ALIAS, set()).add(node)
        fresh.append(np.array(fw, np.int64))
        full.append([g for g in alias_groups(name) if set(g) <= seen])
        pair.append(0 in seen and ALIAS in seen)
    allf = np.concatenate(fresh)
    nodes, counts = np.unique(b["node"][ok], return_counts=True)
    return dict(ok=int(ok.sum()), on_planted=int(sum(x in pl for x in b["node"][ok].tolist())),
                binds_on=dict(zip(nodes.tolist(), counts.tolist())), fresh=fresh, untouched=untouched, both=both,
                fresh_per_trip=np.bincount(trip_of(name, allf), minlength=trips_of(name)).tolist(),
                fresh_last_block=int((allf // BLK == blocks_of(name) - 1).sum()),
                trips_per_window=[len(set(trip_of(name, f).tolist())) for f in fresh],
                full_groups=full, pair_windows=pair)
