"""The inputs of tests/test_width_gpu.py, pinned on the oracle alone (tests/width_cases.py): without
these conditions the engine comparison could pass without ever reaching the hashed touched filter or
a second trip of the merge.  They are conditions on the inputs: a trace that misses one is changed in
width_cases.py; the conditions here stay.  Every test prints the counts it measured.

At two widths conditions are stated otherwise than planned, because no trace can meet the planned ones:

  * b257a has a single node past 65,535 — node 65,536, all of block 256, all of the merge's second
    trip, and node 0's only alias.  A node is a fresh win at most once per window and the 768 pods
    make four windows, so "12 aliases while untouched", "20 fresh wins per trip" and "8 fresh wins in
    the last block" cannot exceed 4 there.  b257a must reach that maximum instead: node 65,536 is a
    fresh win of every window and an alias while untouched (of node 0, or node 0 of it) in every
    window.  Its counts of binds (>= 20 on each of the two nodes) and of aliases both touched (>= 50)
    are the planned ones.
  * b256 has one merge trip, so no window can span two; the fresh wins of one window must lie in at
    least 20 different blocks instead (one list per merge thread: 20 threads' lists meet in the merge).
"""
import os
import re

import numpy as np
import pytest

import group_cases as gc
import weight_cases
import width_cases as wc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kubernetes-simulator_amd", "csrc")
ALL = list(wc.WIDTHS)
N_WINDOWS = wc.N_PODS // wc.WINDOW
# every (width, scorers, seed) the engine tests run
RUNS = [(w, None, wc.SEED) for w in ALL] + [(w, "w16p", wc.SEED) for w in wc.FALLBACK] + \
       [(w, None, s) for w, s in wc.MORE_SEEDS]
IDS = [f"{w}-{sc or 'lrba'}-{seed}" for w, sc, seed in RUNS]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_restated_constants_are_the_sources():
    role, scan, plan, step, tick, dev = (_src(f) for f in ("ks_rolesplit.hip", "ks_scan.hip", "ks_plan.h", "ks_step.cpp",
                                                            "ks_tick.hip", "ks_device.h"))
    assert "constexpr int kFilterBits = 1 << 16;" in role and wc.ALIAS == 1 << 16
    assert "const bool exact = a.c.n_nodes <= kFilterBits;" in role
    assert "(uint32_t)node & (kFilterBits - 1)" in role
    assert f"in.nl_max > {wc.MERGE_WIDE} ? {wc.MERGE_WIDE} : {wc.MERGE_NARROW}" in scan
    assert "for (int j = tid; j < nfl; j += nthr)" in scan, "merge_kernel's fold loop no longer strides by its threads"
    assert int(re.search(r"#define KS_OVERLAP_MAX_BLOCKS (\d+)", plan).group(1)) == wc.OVERLAP_MAX_BLOCKS
    assert int(re.search(r"#define KS_PRUNE_MIN_BLOCKS (\d+)", step).group(1)) == wc.PRUNE_MIN_BLOCKS
    threads = int(re.search(r"constexpr int kTickThreads = (\d+);", tick).group(1))
    assert threads * int(re.search(r"constexpr int kTickNodes = (\d+);", tick).group(1)) == wc.TICK_WG_NODES
    assert "kBlockNodes = kScanWaves * kWave" in dev and wc.BLK == gc.BLOCK_NODES == 256
    assert wc.WINDOW == int(re.search(r"constexpr int kChunkBatch = (\d+);", _src("ks_engine.cpp")).group(1))


def test_the_widths_stand_on_both_sides_of_every_switch():
    assert [wc.WIDTHS[w] for w in ALL] == [65_536, 65_537, 65_792, 131_328, 261_888, 262_144, 262_400]
    assert [wc.blocks_of(w) for w in ALL] == [256, 257, 257, 513, 1023, 1024, 1025]
    assert [wc.trips_of(w) for w in ALL] == [1, 2, 2, 3, 4, 4, 2]       # b1025: 1,024 threads, thread 0 twice
    assert [wc.blocks_of(w) <= wc.OVERLAP_MAX_BLOCKS for w in ALL] == [True] + [False] * 6
    assert [wc.blocks_of(w) >= wc.PRUNE_MIN_BLOCKS for w in ALL] == [False] * 5 + [True] * 2
    assert [wc.WIDTHS[w] <= wc.ALIAS for w in ALL] == [True] + [False] * 6
    assert wc.WIDTHS["b257a"] - 256 * wc.BLK == 1, "block 256 of b257a is not a single node"
    # the per-tick kernel's evaluating workgroups
    assert [-(-wc.WIDTHS[w] // wc.TICK_WG_NODES) for w in wc.TICK_WIDTHS] == [65, 129, 257]
    # the virtual shards' uneven parts
    from kubesim_amd import shard
    parts = [sorted(np.diff(shard.engine_part_blocks(wc.WIDTHS[w], 1, 3)).tolist()) for w in wc.SHARD_WIDTHS]
    assert parts == [[85, 86, 86], [341, 342, 342]]
    # two uneven steps that cut the 192-pod windows and run past the last bind
    assert sum(wc.STEPS) > wc.N_PODS and wc.STEPS[0] % wc.WINDOW and wc.STEPS[1] % wc.WINDOW


def test_the_resolver_each_engine_takes():
    """The host's choices restated (tests/group_cases.py): the planted traces are chunk-eligible under
    the plain scorers, so the role-split kernel needs its flag there; under w16p the 16-bit key table
    is one short, which is the fallback; a group with a member above the small class takes it too."""
    for w in ALL:
        tr, _ = wc.width_trace(w)
        r = gc.restate(tr, wc.MODE)
        assert gc.chunk_eligible(r) and not r["small"], (w, r)
    for w in wc.FALLBACK:
        tr, _ = wc.width_trace(w)
        r = gc.restate(tr, wc.mode_of("w16p"))
        assert not r["k16"] and not gc.chunk_eligible(r) and not r["small"], (w, r)
    assert weight_cases.MAXIMUM["w16p"] + 1 == 1 << 16
    big, small = gc.restate(wc.width_trace("b257")[0], wc.MODE), gc.restate(wc.small_member()[0], wc.MODE)
    assert small["small"] and not big["small"]
    assert gc.group_choices([big, small])["resolver"] == "RBig" and gc.group_choices([big, small])["merge"] == "merge_kernel"


@pytest.mark.parametrize("width,scorers,seed", RUNS, ids=IDS)
def test_every_run_binds_on_the_planted_nodes(width, scorers, seed):
    r = wc.oracle_run(width, scorers, seed)
    ev = wc.events(width, scorers, seed)
    b = r["binds"]
    print(f"{width} scorers={scorers} seed={seed}: oracle {r['seconds']:.2f} s, planted {len(wc.planted(width))}, "
          f"Ok {ev['ok']}, on planted nodes {ev['on_planted']}, distinct nodes {len(ev['binds_on'])}")
    assert r["rc"] == 0 and len(b["pod"]) == wc.N_PODS and ev["ok"] >= 700
    np.testing.assert_array_equal(b["pod"], np.arange(wc.N_PODS))
    np.testing.assert_array_equal(b["tick"], 1 + np.arange(wc.N_PODS))      # one bind per tick from tick 1
    assert ev["on_planted"] >= 700
    assert wc.WIDTHS[width] - 1 in wc.planted(width) and ev["binds_on"].get(wc.WIDTHS[width] - 1, 0) >= 1
    # the usage differs at the three cuts, and pods have ended by each: expiries ran inside the steps
    u = r["usage"]
    assert all((u[a] != u[z]).any() for a, z in zip(wc.CUTS, wc.CUTS[1:]))


@pytest.mark.parametrize("width,scorers,seed", RUNS, ids=IDS)
def test_alias_events(width, scorers, seed):
    ev = wc.events(width, scorers, seed)
    groups = wc.alias_groups(width)
    print(f"{width} scorers={scorers} seed={seed}: alias groups {len(groups)} (of 3+: {sum(len(g) >= 3 for g in groups)}), "
          f"alias while untouched {ev['untouched']}, both touched {ev['both']}, "
          f"groups bound whole per window {[len(g) for g in ev['full_groups']]}")
    if width == "b256":                              # the control: no two nodes share a filter bit
        assert not groups and ev["untouched"] == 0 and ev["both"] == 0 and max(ev["binds_on"]) < wc.ALIAS
        return
    if width == "b257a":
        assert groups == [[0, wc.ALIAS]]
        assert ev["untouched"] == N_WINDOWS, "nodes 0 and 65,536 do not meet as a fresh win in every window"
        assert ev["binds_on"][0] >= 20 and ev["binds_on"][wc.ALIAS] >= 20 and any(ev["pair_windows"])
    else:
        assert len(groups) >= 12 and ev["untouched"] >= 12
    assert ev["both"] >= 50
    if wc.WIDTHS[width] > 2 * wc.ALIAS:
        assert any(len(g) >= 3 for w in ev["full_groups"] for g in w), "no window binds x, x + 65,536 and x + 131,072"


@pytest.mark.parametrize("width,scorers,seed", RUNS, ids=IDS)
def test_fresh_wins_in_every_trip_of_the_merge(width, scorers, seed):
    ev = wc.events(width, scorers, seed)
    blocks = [len(set((f // wc.BLK).tolist())) for f in ev["fresh"]]
    print(f"{width} scorers={scorers} seed={seed}: trips {wc.trips_of(width)} of {wc.trip_blocks(width)} blocks, fresh wins per trip "
          f"{ev['fresh_per_trip']}, in the last block {ev['fresh_last_block']}, trips per window {ev['trips_per_window']}, "
          f"blocks per window {blocks}")
    assert len(ev["fresh_per_trip"]) == wc.trips_of(width)
    if width == "b257a":
        assert ev["fresh_per_trip"][0] >= 20
        assert ev["fresh_per_trip"][1] == ev["fresh_last_block"] == N_WINDOWS, "node 65,536 is not a fresh win of every window"
    else:
        assert min(ev["fresh_per_trip"]) >= 20
        assert ev["fresh_last_block"] >= 8
    if wc.trips_of(width) > 1:
        assert max(ev["trips_per_window"]) >= 2
        assert min(ev["trips_per_window"]) == wc.trips_of(width)      # (more than asked: every window, every trip)
    else:
        assert max(blocks) >= 20


def test_the_small_member_of_the_group():
    tr, enc, b, usage = wc.small_member()
    assert tr["nodes"]["n"] == 2000 and len(b["pod"]) == wc.N_PODS and (b["status"] == 0).sum() >= 700
    assert usage.any()
