"""The inputs of tests/test_group_mixed_gpu.py, pinned on the traces and the CPU oracle alone
(tests/group_cases.py): every member forces the choice it is listed for, every group the group-wide
evaluator class / key word / resolver / merge kernel it is built for, and the oracle's runs have the
stops, OverCapacity binds, expiry windows and empty-queue ticks the GPU tests rely on.  A recipe that
misses its condition is changed in group_cases.py; the conditions here stay.
"""
import numpy as np
import pytest

import group_cases as gc
from expiry_burst_cases import attached, window_sums
from kubesim_amd import _lib


def _restated(key):
    r = gc.recipe(key)
    return gc.restate(gc.trace_of(key)[0], r["mode"], r["batch_pods"], r["engine_flags"])


def _ran_to_end(key):
    return gc.final_code(key) == 0 and len(gc.all_binds(key)["pod"]) == gc.trace_of(key)[0]["pods"]["m"]


# ---- per member --------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(gc.MEMBERS))
def test_member_forces_what_it_is_listed_for(key):
    got, want = _restated(key), gc.MEMBERS[key]["forces"]
    print(key, got)
    assert {f: got[f] for f in want} == want


def test_restated_rules_at_their_edges():
    """The default batch rule at the node counts the issue lists, and the thresholds' edges."""
    assert [gc.default_batch(n) for n in (64, 2000, 3000, 4095, 4096, 5000)] == [64, 96, 160, 224, 256, 256]
    assert gc.default_batch(5000, 3) == 3
    assert [gc.block_count(n) for n in (1, 64, 256, 257, 2000, 2048, 2049, 3000, 5000)] == [1, 1, 1, 2, 8, 8, 9, 12, 20]
    assert gc.small_class(128, 8192) and not gc.small_class(129, 64) and not gc.small_class(64, 8193)
    assert gc.key16(((1, 3276, 0), (2, 3277, 0), (0, 1, 4))) and not gc.key16(((1, 3276, 0), (2, 3277, 0), (0, 1, 5)))
    sc = ((1, 1, 0), (2, 1, 0))
    assert gc.eval_class([255, 65535, 0], sc) == gc.MICRO and gc.eval_class([256, 65536, 0], sc) == gc.TINY
    assert gc.eval_class([1, (1 << 26) - 1, 0], sc) == gc.TINY and gc.eval_class([1, 1 << 26, 0], sc) == gc.NARROW
    assert gc.eval_class([1, (1 << 29) - 1, 0], sc) == gc.NARROW and gc.eval_class([1, 1 << 29, 0], sc) == gc.WIDE
    assert gc.eval_class([1, 1, 1], ((1, 1 << 24, 0),)) == gc.TINY
    assert gc.eval_class([1, 1, 1], sc, _lib.KS_ENGINE_FORCE_WIDE) == gc.WIDE


def test_wideq_is_wide_by_its_memory_alone():
    got = _restated("wideq")
    assert got["scaled_max"][1] == 1 << 31 and max(got["scaled_max"][0], got["scaled_max"][2]) < gc.MICRO_CAP


def test_rescale_unit_falls_and_class_widens_at_the_second_submit():
    tr, _ = gc.trace_of("rescale")
    before = gc.restate(tr, "feeds_all_lrba", hi=gc.RESCALE_CUT)
    after = gc.restate(tr, "feeds_all_lrba")
    print("rescale before", before, "after", after)
    assert before["unit"][1] == 256 * (1 << 20) * 1000 and after["unit"][1] == 1   # 256 MiB -> 1 milli-byte
    assert before["unit"][0] == after["unit"][0] and before["unit"][2] == after["unit"][2]
    assert before["cls"] == gc.MICRO and after["cls"] == gc.WIDE
    assert gc.parts_of("rescale") == [(0, 0, gc.RESCALE_CUT), (3, gc.RESCALE_CUT, 700)]
    # pods of the first part are still queued when the second goes in (after tick 288)
    assert gc.reference("rescale")[2]["queued"] == gc.RESCALE_CUT - sum(gc.CHUNKS[:3])


# ---- per group -----------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(gc.GROUPS))
def test_group_forces_its_group_wide_choices(group):
    got = gc.group_choices([_restated(k) for k in gc.GROUPS[group]])
    print(group, got)
    assert got == gc.GROUP_FORCES[group]
    assert len(got["batches"]) >= 2


def test_groups_are_what_the_tests_name():
    assert list(gc.GROUPS["everything"]) == list(gc.MEMBERS) and len(gc.MEMBERS) == 11
    for k in gc.SHARED:
        assert sum(k in g for g in gc.GROUPS.values()) >= 2, k
    # a small-class member run by the role-split resolver because of a sibling
    small = [_restated(k)["small"] for k in gc.GROUPS["role_by_batch"]]
    assert small == [True, True, False]
    # wide kernels evaluating micro members
    assert [_restated(k)["cls"] for k in gc.GROUPS["small_with_wide"]] == [gc.MICRO, gc.MICRO, gc.WIDE, gc.WIDE]


# ---- the oracle's runs -----------------------------------------------------------------------------
def test_everything_has_members_that_stop_and_members_that_finish():
    stopped = [k for k in gc.MEMBERS if gc.final_code(k) == _lib.KS_ENOTFOUND
               and len(gc.all_binds(k)["pod"]) < gc.trace_of(k)[0]["pods"]["m"] - 1]
    done = [k for k in gc.MEMBERS if _ran_to_end(k)]
    print("stopped", stopped, "ran to the end", done)
    assert len(stopped) >= 2 and len(done) >= 6
    assert set(stopped) | set(done) == set(gc.MEMBERS)
    # the members whose binds are compared across groups include one that stops
    assert set(stopped) & set(gc.SHARED)


def test_literal_binds_over_capacity_and_never_stops():
    b = gc.all_binds("literal")
    assert _ran_to_end("literal")
    assert (b["status"] == _lib.KS_POD_OVER_CAPACITY).sum() >= 1 and (b["status"] == _lib.KS_POD_OK).sum() >= 1


def _window_expiries(key, batch):
    """Per pod s: the expiries the resolver's window holds for the batch of `batch` pods that starts
    at s — those attached to pods s + 1 .. s + batch - 1, i.e. finishing in (bind tick of s, bind
    tick of s + batch - 1] (ks_submit_pods attaches an expiry to the first pod bound at or after it)."""
    tr, _ = gc.trace_of(key)
    _, csr = attached(gc.all_binds(key), gc.durations(tr))
    return window_sums(csr, batch)


def test_short_overflows_the_small_resolvers_expiry_window():
    """Batches of `short`'s 128 pods whose windows hold more than RSmall::kMaxExp expiries: any run of
    128 consecutive pods, and the two batches that start where a step of CHUNKS starts (pods 38 and
    288: batch starts whatever the earlier batches committed)."""
    assert gc.MEMBERS["short"]["forces"]["B"] == gc.SMALL_MAX_BATCH == 128 and _ran_to_end("short")
    b = gc.all_binds("short")
    assert (b["tick"] == b["pod"] + 1).all() and (b["status"] == 0).all()
    cnt = _window_expiries("short", 128)
    starts = [int(np.searchsorted(b["tick"], t + 1)) for t in np.cumsum(gc.CHUNKS)[:-1]]
    print("windows over 128:", int((cnt > gc.SMALL_MAX_EXP).sum()), "max", cnt.max(), "at step starts", starts, cnt[starts])
    assert starts == [1, 38, 288]
    assert (cnt > gc.SMALL_MAX_EXP).any()
    assert cnt[38] > gc.SMALL_MAX_EXP and cnt[288] > gc.SMALL_MAX_EXP


def test_stream_queue_runs_empty_inside_every_step():
    assert _ran_to_end("stream")
    ticks = set(gc.all_binds("stream")["tick"].tolist())
    lo = 0
    for k in gc.CHUNKS:
        empty = [t for t in range(lo + 1, lo + k + 1) if t not in ticks]
        print(f"ticks {lo + 1}..{lo + k}: {len(empty)} without a bind")
        assert empty
        lo += k
    # drained well inside the last step: the steps after it have nothing due
    assert max(ticks) < sum(gc.CHUNKS) - 100


# ---- split65 / pool65 --------------------------------------------------------------------------------
def _split_keys():
    return [("split65", i) for i in range(gc.SPLIT_N)]


def test_split65_halves_are_ragged():
    assert gc.SPLIT_N >= gc.SPLIT_MIN and gc.halves(gc.SPLIT_N) == [(0, 32), (32, 65)]
    assert gc.halves(63) == [(0, 63)] and gc.halves(64) == [(0, 32), (32, 64)]
    half = lambda i: 0 if i < 32 else 1
    assert sorted(half(i) for i in gc.SPLIT_WIDE) == [0, 1]
    assert half(gc.SPLIT_RESCALE) == 1 and gc.SPLIT_RESCALE not in gc.SPLIT_WIDE
    for i in range(gc.SPLIT_N):
        r, (tr, _) = gc.split_member(i), gc.trace_of(("split65", i))
        if i == gc.SPLIT_RESCALE:
            assert r["late"] == (1, gc.RESCALE_CUT) and tr["nodes"]["n"] == 300
            continue
        assert tr["nodes"]["n"] == 64 + (i * 29) % 137 and 64 <= tr["nodes"]["n"] <= 200
        assert tr["pods"]["m"] == 100 + (i * 37) % 500 and r["mode"] == gc.SPLIT_MODES[i % 4]
        assert (r["engine_flags"] == _lib.KS_ENGINE_FORCE_WIDE) == (i in gc.SPLIT_WIDE)
    pods = [gc.trace_of(k)[0]["pods"]["m"] for k in _split_keys()]
    most = [max(pods[lo:hi]) for lo, hi in gc.halves(gc.SPLIT_N)]
    print("largest pod count per half", most)
    assert abs(most[0] - most[1]) >= 2 * 64
    # group-wide: wide kernels, 16-bit keys, the register-table resolver, merge_small, several batches
    got = gc.group_choices([_restated(k) for k in _split_keys()])
    print("split65", got)
    assert got == dict(mode=gc.WIDE, k16=True, resolver="RSmall", merge="merge_small", batches=[64])
    # (every member's default batch is 64: ragged here are the halves' rounds, not the batches)


def test_split65_both_halves_hold_stopped_and_running_members():
    for lo, hi in gc.halves(gc.SPLIT_N):
        stopped = [i for i in range(lo, hi) if gc.final_code(("split65", i)) == _lib.KS_ENOTFOUND]
        other = [i for i in range(lo, hi) if gc.final_code(("split65", i)) == 0]
        print(f"half [{lo}, {hi}): {len(stopped)} stop with NotFound, {len(other)} do not")
        assert len(stopped) >= 3 and len(other) >= 20
    # the longest queue of a step sets the half's rounds: in the last step one half is done two
    # batches of 64 before the other
    for s in range(len(gc.SPLIT_STEPS)):
        due = [max(len(gc.reference(("split65", i))[s]["binds"]["pod"]) for i in range(lo, hi))
               for lo, hi in gc.halves(gc.SPLIT_N)]
        print(f"step {s}: most binds of a member per half {due}")
    assert abs(due[0] - due[1]) >= 2 * 64
    # the rescaled member is still binding then
    assert len(gc.reference(("split65", gc.SPLIT_RESCALE))[2]["binds"]["pod"]) > 0


def test_pool65_binds_every_pod_of_every_member():
    total = 0
    for i in range(gc.POOL_N):
        key = ("pool65", i)
        b = gc.all_binds(key)
        assert gc.final_code(key) == 0 and len(b["pod"]) == gc.POOL_PODS == 4200
        total += len(b["pod"])
    assert total == 273_000 >= gc.POOL_MIN_BINDS
    got = gc.group_choices([_restated(("pool65", i)) for i in range(gc.POOL_N)])
    print("pool65", got)
    assert got == dict(mode=gc.MICRO, k16=True, resolver="RSmall", merge="merge_small", batches=[64])
    # the members differ: a partition that hands a member another one's rows shows
    first = [tuple(gc.all_binds(("pool65", i))["node"][:40]) for i in range(gc.POOL_N)]
    assert len(set(first)) == gc.POOL_N
