"""ks_step above 65,536 nodes, against the cached oracle runs of tests/width_cases.py (pinned on the
oracle alone by tests/test_width_cases.py): the role-split resolver's hashed touched filter — forced
by flag, as the fallback for totals past the 16-bit key table, and in a what-if group — merge_kernel
with two to four block lists per thread and with 1,024 threads, the unsharded plan's switch from the
two-launch chain to the plain chain at 257 scan blocks, pruned lists on both sides of their default
switch at 1,024 blocks, three uneven virtual shards, and the per-tick kernel with up to 257
evaluating workgroups.

Every run compares the binds (pod, node, tick, status) and the usage with the oracle's after each of
two uneven steps (300 and 473 ticks: they cut the 192-pod batches); everything is exact integer
equality.  The widths, what switches at each, and the planted alias groups: tests/width_cases.py.
"""
import numpy as np
import pytest

import width_cases as wc
from harness import MODES, assert_same_binds, make_engine
from kubesim_amd import _lib

pytestmark = pytest.mark.gpu
ALL = list(wc.WIDTHS)
ONE_POD, CHUNK = _lib.KS_ENGINE_ONE_POD_RESOLVER, _lib.KS_ENGINE_CHUNK_RESOLVER
PRUNED, NO_OVERLAP = _lib.KS_ENGINE_PRUNED_LISTS, _lib.KS_ENGINE_NO_OVERLAP
AROUND_PRUNE = ["b1023", "b1024", "b1025"]


def _run(width, batch=0, flags=0, shard=None, scorers=None, seed=wc.SEED, profile=False, check=None):
    """One engine over wc.STEPS: binds and usage against the oracle's after each step; then check(eng,
    the last step's per-kernel statistics or None, the between-step invariants)."""
    tr, enc = wc.width_trace(width, seed)
    ref = wc.oracle_run(width, scorers, seed)
    eng = make_engine(tr, enc, wc.mode_of(scorers), batch, flags, shard)
    try:
        eng.submit(enc["pods"])
        eng.set_profiling(profile)
        at = 0
        for k in wc.STEPS:
            eb = eng.step(k)
            assert_same_binds(eb, wc.binds_between(ref["binds"], at, at + k))
            at += k
            np.testing.assert_array_equal(eng.usage(), ref["usage"][at], err_msg=f"{width}: usage after tick {at}")
        assert eng.queued == 0
        inv = eng.debug_invariants()
        assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv
        if check:
            check(eng, eng.last_step_kernels() if profile else None, inv)
    finally:
        eng.close()


def _role_split(eng, k, inv):
    """the chunk resolver's workspace was never made: every batch went through resolve_kernel"""
    assert inv["slot_max"] == 0 and inv["nslot_hw"] == 0, inv
    if k is not None:
        assert k["resolve_n"] > 0 and k["fused_n"] == 0, k
        assert k["prep_n"] == k["scan_n"] == k["merge_n"] == k["resolve_n"], k


def _chunk(eng, k, inv):
    assert inv["nslot_hw"] > 0 and inv["slot_max"] > 0, inv


# ---- 1. the role-split resolver, forced ---------------------------------------------------------------
@pytest.mark.parametrize("width", ALL)
def test_role_split_resolver(width):
    _run(width, 192, ONE_POD, check=_role_split)


def test_role_split_resolver_batches_of_256():
    _run("b257", 256, ONE_POD, check=_role_split)


@pytest.mark.parametrize("width,seed", wc.MORE_SEEDS)
def test_role_split_resolver_another_seed(width, seed):
    _run(width, 192, ONE_POD, seed=seed, check=_role_split)


# ---- 2. the role-split resolver as the fallback -------------------------------------------------------
@pytest.mark.parametrize("width", wc.FALLBACK)
def test_role_split_resolver_is_the_fallback_past_the_16_bit_key_table(width):
    """w16p: the maximum total + 1 is 2^16, so the engine is not chunk-eligible and, with no flag set,
    every batch is expire_head -> scan (32-bit keys) -> merge -> resolve."""
    _run(width, scorers="w16p", profile=True, check=_role_split)


# ---- 3. the default engine ----------------------------------------------------------------------------
@pytest.mark.parametrize("width", ALL)
def test_default_engine_and_its_chain(width):
    """No flags: the chunk resolver on the two-launch chain up to 256 scan blocks (a scan only where a
    pass preps: its first batch), on the plain chain above (a scan per merge, nothing fused)."""
    def chain(eng, k, inv):
        _chunk(eng, k, inv)
        print(width, {f: v for f, v in k.items() if f.endswith("_n")})
        assert k["merge_n"] > 0
        if wc.blocks_of(width) <= wc.OVERLAP_MAX_BLOCKS:
            assert k["fused_n"] > 0 and k["scan_n"] == k["prep_n"], k
        else:
            assert k["fused_n"] == 0 and k["scan_n"] == k["merge_n"], k
    _run(width, profile=True, check=chain)


@pytest.mark.parametrize("flags", [PRUNED, CHUNK | NO_OVERLAP], ids=["pruned_lists", "chunk_no_overlap"])
@pytest.mark.parametrize("width", AROUND_PRUNE)
def test_both_list_forms_on_both_sides_of_the_pruning_default(width, flags):
    _run(width, flags=flags, check=_chunk)


# ---- 4. three uneven virtual shards -------------------------------------------------------------------
@pytest.mark.parametrize("resolver", ["role_split", "default"])
@pytest.mark.parametrize("width", wc.SHARD_WIDTHS)
def test_three_virtual_shards(width, resolver):
    if resolver == "role_split":
        _run(width, 192, ONE_POD, shard=(1, 0, None, 3), check=_role_split)
    else:
        _run(width, shard=(1, 0, None, 3), check=_chunk)


# ---- 5. the per-tick kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("width", wc.TICK_WIDTHS)
def test_per_tick_kernel(width):
    """ks_step(1) for the first 96 ticks — one launch each, one workgroup per 1,024 nodes plus the
    copier (the whole trace was submitted before the first) — then the rest in one step."""
    tr, enc = wc.width_trace(width)
    ref = wc.oracle_run(width)
    eng = make_engine(tr, enc, wc.MODE)
    try:
        eng.submit(enc["pods"])
        for t in range(1, wc.TICK_STEPS + 1):
            eb = eng.step(1)
            assert eng.last_step_stats()["launches"] == 1, f"tick {t} did not take the one-launch path"
            assert_same_binds(eb, wc.binds_between(ref["binds"], t - 1, t))
        assert eng.tick == wc.TICK_STEPS
        np.testing.assert_array_equal(eng.usage(), ref["usage"][wc.TICK_STEPS], err_msg=f"{width}: usage after tick {wc.TICK_STEPS}")
        end = sum(wc.STEPS)
        assert_same_binds(eng.step(end - wc.TICK_STEPS), wc.binds_between(ref["binds"], wc.TICK_STEPS, end))
        np.testing.assert_array_equal(eng.usage(), ref["usage"][end], err_msg=f"{width}: usage after tick {end}")
    finally:
        eng.close()


# ---- 6. a what-if group -------------------------------------------------------------------------------
def test_group_with_a_member_above_the_filter_range():
    """A group of the b257 cluster and a 2,000-node one: the big member is above the small class, so
    ks_group_step runs the role-split kernel (and merge_kernel over 257 and 8 lists) for both."""
    from kubesim_amd.engine import Group
    big_tr, big_enc = wc.width_trace("b257")
    ref = wc.oracle_run("b257")
    small_tr, small_enc, small_binds, small_usage = wc.small_member()
    fm, fl, sc = MODES[wc.MODE]
    g = Group(2)
    try:
        engs = []
        for tr, enc in ((big_tr, big_enc), (small_tr, small_enc)):
            e = g.add(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc)
            e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
            e.submit(enc["pods"])
            engs.append(e)
        at = 0
        for k in wc.STEPS:
            allb, cnt, st, _ = g.step(k)
            assert st.tolist() == [0, 0]
            big, small = g.split(allb, cnt)
            assert_same_binds(big, wc.binds_between(ref["binds"], at, at + k))
            assert_same_binds(small, wc.binds_between(small_binds, at, at + k))
            at += k
            np.testing.assert_array_equal(engs[0].usage(), ref["usage"][at], err_msg=f"big member: usage after tick {at}")
        np.testing.assert_array_equal(engs[1].usage(), small_usage, err_msg="small member: usage")
    finally:
        g.close()
