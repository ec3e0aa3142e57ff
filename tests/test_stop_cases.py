"""The inputs of tests/test_stop_gpu.py, pinned on the traces and the CPU oracle alone
(tests/stop_cases.py): every case stops, or does not, at the pod and with the code its GPU test
relies on; one tick before X the oracle sees the planned number of feasible nodes (none in `full`,
`too_late` and `rescued_own`); a rescued X binds on the node the freeing pod ran on; X carries the
planned expiries; the plans put X where they say; the constants restated in the cases module are the
sources'.  A trace that misses its condition is changed in stop_cases.py; the conditions here stay.
"""
import os
import re

import numpy as np
import pytest

import group_cases as gc
import state_ref
import stop_cases as sc
from kubesim_amd import shard, tracegen

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kubernetes-simulator_amd", "csrc")
GRID = [(cl, sat, name) for cl in ("3k", "small") for sat in sc.SATS for name in sc.CASES]
PIPE = [("pipe", sat, name) for sat in sc.SATS for name in ("full", "rescued_own")]


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ---- per case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cluster,sat,name", GRID + PIPE)
def test_case_produces_its_planned_event(cluster, sat, name):
    c = sc.case(name, sat, cluster)
    x, m, s = c["x"], c["m"], c["s"]
    b, rc = sc.all_binds(name, sat, cluster)
    np.testing.assert_array_equal(b["pod"], np.arange(len(b["pod"])))      # FIFO, one a tick: pod i at tick i + 1
    np.testing.assert_array_equal(b["tick"], b["pod"] + 1)
    over = int((b["status"] != 0).sum())
    prc, feas = sc.probe(name, sat, cluster)
    print(f"{cluster} {sat} {name}: code {rc}, {len(b['pod'])} binds, {over} OverCapacity, "
          f"feasible for X at tick {x}: {None if feas is None else int(feas.sum())}")
    if name in sc.STOPS:
        code, pod = c["stop"]
        assert rc == code and len(b["pod"]) == pod           # every pod before the stop pod bound, none after
    else:
        assert rc == 0 and len(b["pod"]) == m                 # the run goes on to the end of the trace
        assert b["status"][x] == 0
    if c["mode"] == sc.LITERAL:
        assert over > 0 and name == "literal_bad_key"         # X would have been bound somewhere, over capacity
    else:
        assert over == 0
    # one tick before X's own
    if name == "two_stops_key_first":
        assert prc == sc.KS_EINVAL and c["stop"][1] == x - 3   # the run never reaches X
        return
    assert prc == 0
    if c["before"] is not None:
        assert int(feas.sum()) == c["before"], (name, int(feas.sum()))
    if c["mode"] == sc.MODE:
        assert not feas[np.setdiff1d(np.arange(c["n"]), c["nodes"])].any()   # only a gpu node can ever take X
    # the slot pods sit on the gpu nodes; at X every slot but the freed one is taken
    slot = np.arange(x - c["shift"] - 2 * s, x - c["shift"], 2)
    if c["mode"] == sc.MODE:
        assert np.isin(b["node"][slot], c["nodes"]).all()
        assert len(np.unique(b["node"][slot])) == sc.SATS[sat][0]            # every gpu node is used
    if c["freed"] is not None:
        assert b["node"][x] == b["node"][c["freed"]], "X is not on the node the freeing pod ran on"
    assert sc.carried(name, sat, cluster) == c["carried"]
    if name == "too_late":   # ... and the pod after X would have carried it
        first = x - 2 * s
        assert first + 1 + c["run"][first] == x + 2


@pytest.mark.parametrize("sat", list(sc.SATS))
def test_freeing_pod_ends_where_the_case_says(sat):
    """From the run lengths alone: the end tick of each case's freeing pod against X's bind tick X + 1."""
    _, x, _ = sc.CLUSTERS["3k"]
    s = sc.slots(sat)
    end = lambda name, pod: pod + 1 + int(sc.case(name, sat, "3k")["run"][pod])
    assert end("full", x - 2 * s) > x + 1000
    assert end("rescued_own", x - 2 * s) == x + 1
    assert end("too_late", x - 2 * s) == x + 2
    assert end("rescued_earlier", x - 4 - 2 * s) == x + 1 - 5
    assert end("rescued_earlier_contended", x - 2 * s) == x + 1 - 5
    assert end("bad_key", x - 2 * s) == end("bad_spec", x - 2 * s) == x + 1 - 5
    # bound inside X's batch (4 pods before X) and ended one tick before X's own: bind and expiry in one batch
    assert end("rescued_in_batch", x - 4) == x
    # ... and with X at edge_p the freeing pod is the last pod of the first chunk, its expiry's pod X - 1 past the edge
    assert end("rescued_in_batch_edge", x - 2 * s) == x
    p = sc.edge_p(sat)
    assert p - 2 * s == sc.KC - 1 and p - 1 >= sc.KC and p < sc.B_CHUNK
    # no background pod ends on X's tick or the next: X carries the freeing pod's expiry or none
    c = sc.case("full", sat, "3k")
    ends = np.arange(c["m"]) + 1 + c["run"]
    assert not np.isin(ends, (x + 1, x + 2)).any()
    assert ((ends > x - 64) & (ends <= x)).sum() >= 10     # while the batch around X sees the usual trickle


# ---- the saturations -------------------------------------------------------------------------------------
def test_saturations_stand_on_either_side_of_the_list_lengths():
    (g6, c6), (g32, c32) = sc.SATS["g6"], sc.SATS["g32"]
    assert g6 < sc.TOP_L and g32 > sc.CHR and (g6 * c6, g32 * c32) == (24, 64)
    assert 2 * 64 < sc.B_SMALL - 1 + 2      # at p = B - 1 every slot pod lies in X's batch, for every B
    for cluster, (n, x, m) in sc.CLUSTERS.items():
        for sat in sc.SATS:
            nodes = sc.gpu_nodes(sat, n)
            assert len(set(nodes.tolist())) == sc.SATS[sat][0] and nodes.min() >= 0 and nodes.max() < n
            assert len(set((nodes // sc.BLOCK_NODES).tolist())) >= 6          # several scan blocks
            for world, vsh in ((1, 3), (2, 1), (1, 2)):                        # vshards3, two ranks, the pipelined parts
                lo = shard.part_blocks(n, world, vsh) * sc.BLOCK_NODES
                parts = np.searchsorted(lo, nodes, side="right")
                assert len(set(parts.tolist())) == world * vsh, (cluster, sat, world, vsh)
            tr = sc.case("full", sat, cluster)["tr"]
            gpu = tr["nodes"]["alloc"][:, tracegen.GPU]
            assert (tr["nodes"]["alloc_has"] & tracegen.HAS_GPU).all()        # capacity 0 with the key present
            assert (gpu > 0).sum() == sc.SATS[sat][0] and gpu.sum() == sc.slots(sat) * tracegen.MILLI
            req = tr["pods"]["req"][:, tracegen.GPU]
            assert (req > 0).sum() == sc.slots(sat) + 1 and req[x] == tracegen.MILLI


def test_host_choices_for_the_clusters():
    """The resolver each cluster selects, from the rules restated in tests/group_cases.py."""
    tr = sc.case("full", "g6", "3k")["tr"]
    r = gc.restate(tr, sc.MODE, sc.B_CHUNK)
    assert not r["small"] and gc.chunk_eligible(r) and r["blocks"] == 12
    r = gc.restate(tr, sc.MODE, sc.B_ONE_POD)
    assert not r["small"]
    r = gc.restate(sc.case("literal_bad_key", "g6", "3k")["tr"], sc.LITERAL, sc.B_CHUNK)
    assert not r["small"] and gc.chunk_eligible(r)
    r = gc.restate(sc.case("full", "g6", "small")["tr"], sc.MODE, sc.B_SMALL)
    assert r["small"] and gc.small_class(sc.B_SMALL, sc.CLUSTERS["small"][0])
    assert gc.MEMBERS["short"]["batch_pods"] == sc.B_SMALL and gc.MEMBERS["short"]["forces"]["small"]
    assert np.diff(shard.part_blocks(sc.CLUSTERS["pipe"][0], 1, 2)).sum() == 257


# ---- plans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,cluster", [(sc.B_CHUNK, "3k"), (sc.B_ONE_POD, "3k"), (sc.B_SMALL, "small")])
def test_plans_put_x_where_they_say(b, cluster):
    n, x, m = sc.CLUSTERS[cluster]
    assert sc.positions(b) == (0, 1, 63, 64, b - 1, b)
    whole_stop, _ = sc.all_binds("full", "g6", cluster)
    whole_go, _ = sc.all_binds("rescued_own", "g6", cluster)
    for p in sc.positions(b) + (sc.edge_p("g6"),):
        if p >= b and p != b:
            continue
        for steps in sc.plans_at(cluster, b, p):
            assert steps[0] >= 200 and sum(steps) == m + 20
            stop = sc.reference("full", "g6", cluster, steps)
            go = sc.reference("rescued_own", "g6", cluster, steps)
            # the warm step ends p pods before X; the stopping step is the plan's second (third: ends_before)
            assert stop[0]["rc"] == 0 and len(stop[0]["binds"]["pod"]) == steps[0] == x - min(p, b)
            last = stop[-1]
            assert last["rc"] == sc.KS_ENOTFOUND and last["tick"] == x + 1 and last["queued"] == m - (x + 1)
            if p < b:
                assert len(stop) == 2 and last["k"] == b and len(last["binds"]["pod"]) == p
                assert go[1]["binds"]["pod"][p] == x and len(go[1]["binds"]["pod"]) == b
            elif len(steps) == 4:      # ends_before: the step before X's returns OK with all B binds
                assert len(stop) == 3 and stop[1]["rc"] == 0 and len(stop[1]["binds"]["pod"]) == b
                assert stop[1]["binds"]["pod"][-1] == x - 1 and last["k"] == 1 and len(last["binds"]["pod"]) == 0
                assert go[2]["binds"]["pod"].tolist() == [x]
            else:                      # through: X is the step's pod b, the first of its second batch
                assert len(stop) == 2 and last["k"] == b + sc.KC and len(last["binds"]["pod"]) == b
                assert go[1]["binds"]["pod"][b] == x
            # the steps cut the run's binds and leave none out
            for whole, steps_ in ((whole_stop, stop), (whole_go, go)):
                for f in whole:
                    np.testing.assert_array_equal(np.concatenate([s["binds"][f] for s in steps_]), whole[f])
            assert set(np.cumsum(steps).tolist()) <= set(sc.marks(cluster))
            assert go[-1]["rc"] == 0 and go[-1]["queued"] == 0
    steps = sc.plan(cluster, b, 0, "ticks")
    assert steps[:5] == (x - 3, 1, 1, 1, 1)
    ref = sc.reference("too_late", "g6", cluster, steps)
    assert [len(s["binds"]["pod"]) for s in ref] == [x - 3, 1, 1, 1, 0] and ref[-1]["rc"] == sc.KS_ENOTFOUND


@pytest.mark.parametrize("name,sat,cluster,b,p", [
    ("too_late", "g6", "3k", sc.B_CHUNK, 64), ("rescued_own", "g32", "3k", sc.B_CHUNK, 192),
    ("two_stops_key_first", "g6", "3k", sc.B_ONE_POD, 0), ("literal_bad_key", "g32", "small", sc.B_SMALL, 127),
    ("rescued_in_batch_edge", "g6", "small", sc.B_SMALL, 111), ("full", "g6", "pipe", sc.B_CHUNK, 64)])
def test_the_cut_record_equals_an_oracle_run_of_the_plan(name, sat, cluster, b, p):
    """stop_cases.reference cuts one oracle run per case along a plan; an oracle stepped with the
    plan's own steps returns the same binds, codes, ticks, queue lengths and usage."""
    for steps in sc.plans_at(cluster, b, p) + ([sc.plan(cluster, b, 0, "ticks")] if cluster != "pipe" else []):
        got, want = sc.reference(name, sat, cluster, steps), sc.direct_reference(name, sat, cluster, steps)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g["k"], g["rc"], g["tick"], g["queued"]) == (w["k"], w["rc"], w["tick"], w["queued"])
            for f in w["binds"]:
                np.testing.assert_array_equal(g["binds"][f], w["binds"][f])
            np.testing.assert_array_equal(g["usage"], w["usage"])


def test_the_other_group_member_runs_on():
    steps = sc.plan("small", sc.B_SMALL, sc.KC)
    ref = sc.short_reference(steps)
    tr, _ = gc.trace_of("short")
    # (its 900 pods outlast the plan's 820 ticks: it is still binding when the plan ends)
    assert sum(len(b["pod"]) for b, _ in ref) == sum(steps) == 820 < tr["pods"]["m"]


# ---- the model of the stopped state -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["too_late", "literal_bad_key", "two_stops_key_first"])
def test_stopped_model_agrees_with_the_interval_reference(name):
    """stop_cases.stopped_model (oracle/pysim.py's rules on the oracle's binds) against
    tests/state_ref.py's vectorised rules on the same binds, and what it says about the stop tick."""
    c = sc.case(name, "g6", "3k")
    m = sc.stopped_model(name, "g6", "3k")
    b, _ = sc.all_binds(name, "g6", "3k")
    code, pod = c["stop"]
    assert m["tick"] == pod + 1 == len(b["pod"]) + 1
    ref = state_ref.IntervalRef(c["tr"], b)
    assert sorted(m["req"]) == list(range(m["tick"] - 4, m["tick"] + 1))
    for t, mat in m["req"].items():
        np.testing.assert_array_equal(mat, ref.at(t))
    want = ref.series(m["series_lo"], m["tick"] + 1)
    np.testing.assert_array_equal(m["series"][:, :6], want[:, :6])
    # pending: every pod arrived at tick 1, one is popped a tick, the stop pod at its own tick
    np.testing.assert_array_equal(m["series"][:, 6], c["m"] - np.minimum(np.arange(m["series_lo"], m["tick"] + 1), pod + 1))
    assert m["series"][-1, 4] + m["series"][-1, 5] == pod
    assert m["status"][pod - 1][0] in (1, 2, 3) and m["status"][pod - 1][2] == pod
    assert m["status"][pod][:3] == (0, -1, -1) and m["status"][pod + 1][:3] == (0, -1, -1)
    if name == "too_late":
        # the freeing pod still runs at the stop tick: its gpu is still requested there
        x, s = c["x"], c["s"]
        node = int(b["node"][x - 2 * s])
        assert m["req"][m["tick"]][c["nodes"], 2].sum() == s * tracegen.MILLI
        assert m["req"][m["tick"]][node, 2] == sc.SATS["g6"][1] * tracegen.MILLI


# ---- the constants, restated ----------------------------------------------------------------------------------
def test_restated_constants_agree_with_the_sources():
    dev, chunk, eng, res, host = (_src(f) for f in ("ks_device.h", "ks_chunk.hip", "ks_engine.cpp", "ks_resolve.hip",
                                                    "ks_host.h"))
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    assert const(dev, "kTopL") == sc.TOP_L == 8
    assert int(re.search(r"#define KS_CHR (\d+)", dev).group(1)) == sc.CHR == 20 and "constexpr int kChR = KS_CHR;" in dev
    assert const(chunk, "kC") == sc.KC == 64
    assert const(eng, "kChunkBatch") == sc.B_CHUNK == 192
    assert const(dev, "kWinMaxB") == const(host, "kDefaultBatch") == sc.B_ONE_POD == 256
    m = re.search(r"using RSmall = Cfg4<\d+, \d+, (\d+), (\d+), \d+, \d+>;", res)
    assert m and int(m.group(2)) == sc.B_SMALL == gc.SMALL_MAX_BATCH == 128
    assert sc.BLOCK_NODES == shard.BLOCK_NODES == gc.BLOCK_NODES == 256
    # the stop's four deciders and the host's unwinding, where the cases' docstrings say they are
    assert "stop_code" in chunk and "cend" in chunk
    assert "err_code" in _src("ks_rolesplit.hip") and "err_pod" in _src("ks_rolesplit.hip")
    assert 'node \\"\\" not found (pod %lld, tick %lld)' in _src("ks_step.cpp")
    assert "pod %lld: invalid pod key or simSpec (tick %lld)" in _src("ks_step.cpp")
    from kubesim_amd import _lib
    assert (_lib.KS_EINVAL, _lib.KS_ENOTFOUND) == (sc.KS_EINVAL, sc.KS_ENOTFOUND)
    ora = open(os.path.join(CSRC, "..", "..", "oracle", "ks_oracle.h")).read()
    assert re.search(r"KO_FLAG_BAD_KEY\s*=?\s*1\b", ora) and re.search(r"KO_FLAG_BAD_SPEC\s*=?\s*2\b", ora)
