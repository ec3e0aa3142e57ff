"""Scenario groups whose members differ (tests/group_cases.py), every member against its own oracle
run: binds (pod, node, tick, status), stop code and usage after every step.  Exact integer equality.

ks_group_step picks one evaluator class, key word, resolver, scan grid and merge kernel for the
whole group; tests/test_group_cases.py pins, without a GPU, which of them each group here forces
and the properties of the oracle's runs these tests rely on.
"""
import time

import numpy as np
import pytest

import group_cases as gc
from harness import MODES, assert_same_binds, engine_run, make_engine, make_oracle
from kubesim_amd import _lib, encode, tracegen

pytestmark = pytest.mark.gpu


def _member(g, key):
    """A loaded member engine of group g for the recipe `key` (no pods yet)."""
    r = gc.recipe(key)
    tr, enc = gc.trace_of(key)
    fm, fl, sc = MODES[r["mode"]] if isinstance(r["mode"], str) else r["mode"]
    e = g.add(tick_seconds=tr["tick_seconds"], filter_mode=fm, filters=fl, scorers=sc,
              batch_pods=r["batch_pods"], engine_flags=r["engine_flags"])
    e.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    return e


def _pods(key, lo, hi):
    tr, enc = gc.trace_of(key)
    if (lo, hi) == (0, tr["pods"]["m"]):
        return enc["pods"]
    return encode.encode_pods(tracegen.slice_pods(tr, lo, hi)["pods"], enc["taint_dict"], enc["label_dict"])


def _group(keys):
    from kubesim_amd.engine import Group
    g = Group(len(keys))
    return g, [_member(g, k) for k in keys]


def _check_member(key, e, ref, eb, rc, where):
    """Member `key` after a step against the step's record of gc.reference."""
    try:
        assert_same_binds(eb, ref["binds"])
    except AssertionError as ex:
        raise AssertionError(f"{where}: {ex}") from None
    assert rc == ref["rc"], (where, rc, ref["rc"])
    if ref["rc"] == 0:
        np.testing.assert_array_equal(e.usage(), ref["usage"], err_msg=f"{where}: usage")
        assert (e.tick, e.queued) == (ref["tick"], ref["queued"]), where


def _run(keys, steps, probes=True):
    """Step a group of the recipes `keys` through `steps`, every member checked against its oracle
    after every step.  Returns (per member the binds of the whole run, per step the stats)."""
    g, engs = _group(keys)
    refs = [gc.reference(k) for k in keys]
    binds, stats_all = [[] for _ in keys], []
    try:
        for s, k in enumerate(steps):
            for key, e in zip(keys, engs):
                for at, lo, hi in gc.parts_of(key):
                    if at == s:
                        e.submit(_pods(key, lo, hi))
            allb, cnt, st, stats = g.step(k)
            stats_all.append(stats)
            for i, (key, e, eb) in enumerate(zip(keys, engs, g.split(allb, cnt))):
                _check_member(key, e, refs[i][s], eb, int(st[i]), f"step {s} ({k} ticks), member {i} {key}")
                binds[i].append(eb)
                if s and refs[i][s - 1]["rc"] != 0:  # stopped earlier: same code, nothing returned
                    assert len(eb) == 0 and st[i] == refs[i][s - 1]["rc"]
            if not probes:
                continue
            # between steps, on one running member: the next queued pod's filter and score, and the
            # usage at a tick inside the step just made
            cands = [i for i in range(len(keys)) if refs[i][s]["probe"] is not None]
            if cands:
                i = cands[s % len(cands)]
                pod, feas, score = refs[i][s]["probe"]
                np.testing.assert_array_equal(engs[i].filter(pod), feas, err_msg=f"filter, member {keys[i]} step {s}")
                np.testing.assert_array_equal(engs[i].score(pod), score, err_msg=f"score, member {keys[i]} step {s}")
                t, usage = refs[i][s]["mid"]
                assert refs[i][s]["lo"] < t <= refs[i][s]["lo"] + k
                np.testing.assert_array_equal(engs[i].usage_at(t), usage, err_msg=f"usage_at({t}), member {keys[i]}")
    finally:
        g.close()
    return [np.concatenate(b) for b in binds], stats_all


@pytest.fixture(scope="module")
def group_runs():
    """The checked run of each GROUPS entry, made when first asked for: {group: {member: binds}}."""
    done = {}

    def get(name):
        if name not in done:
            t0 = time.perf_counter()
            binds, _ = _run(gc.GROUPS[name], gc.CHUNKS)
            print(f"{name}: {len(gc.GROUPS[name])} members, {time.perf_counter() - t0:.2f} s")
            done[name] = dict(zip(gc.GROUPS[name], binds))
        return done[name]
    return get


# ---- a. mixed groups ---------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(gc.GROUPS))
def test_mixed_group_matches_oracle(group_runs, group):
    got = group_runs(group)
    for key, b in got.items():  # the run's binds are the oracle's whole run
        assert_same_binds(b, gc.all_binds(key))


# ---- b. a member's binds do not depend on who else is in the group -------------------------------
def test_member_binds_do_not_depend_on_its_siblings(group_runs):
    ticks = sum(gc.CHUNKS)
    for key in gc.SHARED:
        groups = [g for g in gc.GROUPS if key in gc.GROUPS[g]]
        assert len(groups) >= 2
        runs = [group_runs(g)[key] for g in groups]
        for g, b in zip(groups[1:], runs[1:]):
            np.testing.assert_array_equal(b, runs[0], err_msg=f"{key}: {g} against {groups[0]}")
        r = gc.recipe(key)
        tr, enc = gc.trace_of(key)
        eng = make_engine(tr, enc, r["mode"], r["batch_pods"], r["engine_flags"])
        eng.submit(enc["pods"])
        alone, code = engine_run(eng, ticks, ticks)
        eng.close()
        np.testing.assert_array_equal(alone, runs[0], err_msg=f"{key}: stepped alone (ks_step)")
        assert code == gc.final_code(key)


# ---- c. two streams, ragged halves ------------------------------------------------------------------
def test_two_stream_split_ragged_halves():
    keys = [("split65", i) for i in range(gc.SPLIT_N)]
    t0 = time.perf_counter()
    _, stats = _run(keys, gc.SPLIT_STEPS, probes=False)
    print(f"split65: {time.perf_counter() - t0:.2f} s, launches {[s['launches'] for s in stats]}")
    for s, st in enumerate(stats):
        # rounds: a member's pods of the step (the one it stopped at included) over its batch of 64
        most = max(len(gc.reference(k)[s]["binds"]["pod"]) + (gc.reference(k)[s]["rc"] != 0
                   and (s == 0 or gc.reference(k)[s - 1]["rc"] == 0)) for k in keys)
        assert st["launches"] >= -(-most // 64), (s, st["launches"], most)
        assert st["pods"] == sum(len(gc.reference(k)[s]["binds"]["pod"]) for k in keys)


# ---- d. the pooled unpack ---------------------------------------------------------------------------
def test_pooled_unpack_every_member():
    keys = [("pool65", i) for i in range(gc.POOL_N)]
    g, engs = _group(keys)
    try:
        for key, e in zip(keys, engs):
            e.submit(_pods(key, 0, gc.POOL_PODS))
        t0 = time.perf_counter()
        allb, cnt, st, stats = g.step(gc.POOL_PODS)
        print(f"pool65: step {time.perf_counter() - t0:.2f} s")
        assert stats["pods"] >= gc.POOL_MIN_BINDS  # the unpack ran on the thread pool
        assert (cnt == gc.POOL_PODS).all() and (g.full_counts == gc.POOL_PODS).all()
        for i, (key, e, eb) in enumerate(zip(keys, engs, g.split(allb, cnt))):
            _check_member(key, e, gc.reference(key)[0], eb, int(st[i]), f"member {i}")
    finally:
        g.close()


# ---- e. members that sit a step out, and the call's edges ------------------------------------------
def test_member_without_nodes_sits_every_step_out():
    """A member that never had ks_load_nodes between two live ones: KS_EINVAL and no binds in every
    step (its zeroed kernel arguments return on the counters); the live members are undisturbed."""
    from kubesim_amd.engine import Group
    keys = ("tiny64", "forcedw")
    g = Group(3)
    try:
        a = _member(g, keys[0])
        idle = g.add(filter_mode=1, filters=7, scorers=((1, 1, 0), (2, 1, 0)))
        b = _member(g, keys[1])
        for key, e in zip(keys, (a, b)):
            e.submit(_pods(key, 0, gc.trace_of(key)[0]["pods"]["m"]))
        for s, k in enumerate(gc.CHUNKS):
            allb, cnt, st, stats = g.step(k)
            parts = g.split(allb, cnt)
            assert st[1] == _lib.KS_EINVAL and cnt[1] == 0 and g.full_counts[1] == 0
            assert idle.tick == 0
            for i, key, e in ((0, keys[0], a), (2, keys[1], b)):
                _check_member(key, e, gc.reference(key)[s], parts[i], int(st[i]), f"step {s}, {key}")
    finally:
        g.close()


def test_step_of_zero_ticks_changes_nothing():
    keys = ("tiny64", "forcedw")
    g, engs = _group(keys)
    try:
        for key, e in zip(keys, engs):
            e.submit(_pods(key, 0, gc.trace_of(key)[0]["pods"]["m"]))
        for s, k in enumerate(gc.CHUNKS):
            before = [(e.tick, e.queued) for e in engs]
            allb, cnt, st, stats = g.step(0)
            assert len(allb) == 0 and (cnt == 0).all() and (g.full_counts == 0).all() and stats["launches"] == 0
            assert [(e.tick, e.queued) for e in engs] == before
            if s:  # a stopped member keeps its code, a running one reports none
                assert [int(x) for x in st] == [gc.reference(key)[s - 1]["rc"] for key in keys]
            allb, cnt, st, _ = g.step(k)
            for i, (key, e, eb) in enumerate(zip(keys, engs, g.split(allb, cnt))):
                _check_member(key, e, gc.reference(key)[s], eb, int(st[i]), f"step {s}, {key}")
    finally:
        g.close()


def test_step_with_nothing_due_then_a_further_submit():
    """Both members' queues are empty after CHUNKS: a step launches nothing and binds nothing; pods
    submitted to one member afterwards are bound as the oracle binds them."""
    keys = ("stream", "literal")
    binds, _ = _run(keys, gc.CHUNKS, probes=False)
    assert [len(b) for b in binds] == [500, 700]
    g, engs = _group(keys)
    try:
        tr, _ = gc.trace_of("stream")
        ora = make_oracle(tr, gc.recipe("stream")["mode"])
        ora.submit(tr)
        for key, e in zip(keys, engs):
            e.submit(_pods(key, 0, gc.trace_of(key)[0]["pods"]["m"]))
        total = sum(gc.CHUNKS)
        g.step(total)
        ora.step(total, cap=total)
        assert [e.queued for e in engs] == [0, 0]
        allb, cnt, st, stats = g.step(100)
        ob, orc = ora.step(100, cap=100)
        assert stats["launches"] == 0 and stats["pods"] == 0 and (cnt == 0).all() and (st == 0).all()
        assert len(ob["pod"]) == 0 and orc == 0
        assert [e.tick for e in engs] == [total + 100] * 2 == [ora.tick] * 2
        np.testing.assert_array_equal(engs[0].usage(), ora.usage())
        # 60 more pods (the trace's first 60 under fresh keys, arriving from now on) for the stream
        # member alone
        more = tracegen.slice_pods(tr, 0, 60)
        more["pods"]["key_id"] = more["pods"]["key_id"] + 10_000
        more["pods"]["arrival"] = more["pods"]["arrival"] + total + 100
        enc = gc.trace_of("stream")[1]
        engs[0].submit(encode.encode_pods(more["pods"], enc["taint_dict"], enc["label_dict"]))
        ora.submit(more)
        allb, cnt, st, stats = g.step(80)
        ob, orc = ora.step(80, cap=80)
        eb = g.split(allb, cnt)
        assert_same_binds(eb[0], ob)
        assert st[0] == orc and len(eb[1]) == 0 and st[1] == 0 and stats["launches"] >= 1
        assert len(ob["pod"]) >= 30 and ob["pod"][0] == 500 and ob["tick"][0] > total + 100
        if orc == 0:
            np.testing.assert_array_equal(engs[0].usage(), ora.usage())
    finally:
        g.close()


def test_cap_below_the_binds_keeps_the_count_and_the_state():
    """cap = 10 on a step of 50 binds per member: the first 10 rows come back, n_out still says 50,
    and the members are where the oracle is after 50 ticks."""
    keys = ("c4", "forcedw")
    g, engs = _group(keys)
    oras = []
    try:
        for key, e in zip(keys, engs):
            tr, _ = gc.trace_of(key)
            e.submit(_pods(key, 0, tr["pods"]["m"]))
            o = make_oracle(tr, gc.recipe(key)["mode"])
            o.submit(tr)
            oras.append(o)
        allb, cnt, st, stats = g.step(50, cap=10)
        assert (cnt == 10).all() and (st == 0).all()
        np.testing.assert_array_equal(g.full_counts, [50, 50])
        assert stats["pods"] == 100
        for i, (key, e, o, eb) in enumerate(zip(keys, engs, oras, g.split(allb, cnt))):
            ob, orc = o.step(50, cap=50)
            assert orc == 0 and len(ob["pod"]) == 50
            assert_same_binds(eb, {f: v[:10] for f, v in ob.items()})
            assert (e.tick, e.queued) == (50, gc.trace_of(key)[0]["pods"]["m"] - 50) and o.tick == 50
            np.testing.assert_array_equal(e.usage(), o.usage(), err_msg=key)
        allb, cnt, st, _ = g.step(50)
        for key, e, o, eb in zip(keys, engs, oras, g.split(allb, cnt)):
            ob, orc = o.step(50, cap=50)
            assert eb["pod"][0] == 50 and eb["tick"][0] == 51
            assert_same_binds(eb, ob)
            np.testing.assert_array_equal(e.usage(), o.usage(), err_msg=key)
        np.testing.assert_array_equal(g.full_counts, cnt)
    finally:
        g.close()


def test_full_group_refuses_a_member_and_a_group_of_one_steps_like_an_engine():
    from kubesim_amd.engine import Group, KsError
    key = "tiny64"
    g = Group(1)
    try:
        e = _member(g, key)
        with pytest.raises(KsError) as ex:
            g.add(filter_mode=1, filters=7, scorers=((1, 1, 0),))
        assert ex.value.code == _lib.KS_EINVAL
        assert len(g.members) == 1
        e.submit(_pods(key, 0, gc.trace_of(key)[0]["pods"]["m"]))
        for s, k in enumerate(gc.CHUNKS):
            allb, cnt, st, _ = g.step(k)
            eb, = g.split(allb, cnt)
            _check_member(key, e, gc.reference(key)[s], eb, int(st[0]), f"step {s}")
        assert gc.final_code(key) == _lib.KS_ENOTFOUND  # the run this checks includes the stop
    finally:
        g.close()
