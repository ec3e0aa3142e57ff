"""The two references of the gang admission preview (tests/gang_ref.py) agree, and the identities the
header states hold on them — no device is needed.

``pysim_gang`` (a deep copy of oracle/pysim.py's simulator, restored on a block) against ``fast_gang``
(the chain on ``place_ref.fast_place``) on the shared 32-node trace in feeds, literal and irregular
modes at ``place_ref.TICKS``.  Everything is exact integer equality; the references are built once and
checked for non-vacuity on their own.
"""
import functools

import numpy as np
import pytest

import drain_ref as dr
import gang_ref as gr
import place_ref as pr

CASES = list(pr.CASES)
KINDS = {"all_or_nothing": dict(min_ok=None), "partial": dict(min_ok=gr.PARITY_MIN_OK),
         "strict": dict(min_ok=gr.PARITY_MIN_OK, strict=True)}


@functools.lru_cache(maxsize=None)
def _fast(case, t, kind):
    r, _ = gr.parity_queue(case)
    state = dr.sim_state(dr.sim_at(case, t), t)
    return gr.fast_gang(r["enc"]["alloc"], state, pr.engine_cfg(_modes(r), r["enc"]), r["shapes"], r["shape_of"],
                        gr.PARITY_FIRST, **KINDS[kind])


def _modes(r):
    from harness import MODES
    return MODES[r["mode"]]


@functools.lru_cache(maxsize=None)
def _slow(case, t, kind):
    _, pods = gr.parity_queue(case)
    return gr.pysim_gang(dr.sim_at(case, t), t, pods, gr.PARITY_FIRST, **KINDS[kind])


def test_the_queue_is_not_vacuous():
    assert gr.PARITY_FIRST[-1] == pr.N_PODS and 0 in gr.PARITY_SIZES and max(gr.PARITY_SIZES) >= 12
    assert all(0 <= m <= s for m, s in zip(gr.PARITY_MIN_OK, gr.PARITY_SIZES))
    seen = {k: set() for k in KINDS}
    partial_with_fail = rolled_back_ok = 0
    for case in CASES:
        for t in pr.TICKS:
            for kind in KINDS:
                r = _fast(case, t, kind)
                seen[kind] |= set(r["outcome"].tolist())
                partial_with_fail += int(((r["outcome"] == gr.ADMITTED) & (r["ok"] < r["size"])).sum())
                rolled_back_ok += int(((r["outcome"] == gr.BLOCKED) & (r["ok"] >= 1)).sum())
                assert (r["rows"]["status"][r["first"][r["outcome"] == gr.SKIPPED]] == gr.NOT_TRIED).all()
    assert seen["all_or_nothing"] == {gr.ADMITTED, gr.BLOCKED} and seen["strict"] == {gr.ADMITTED, gr.BLOCKED, gr.SKIPPED}
    assert partial_with_fail >= 10, "no gang is admitted with a failed pod"
    assert rolled_back_ok >= 10, "no attempt is rolled back after an Ok pod"


@pytest.mark.parametrize("case", CASES)
def test_pysim_and_the_integer_chain_agree(case):
    for t in pr.TICKS:
        for kind in KINDS:
            gr.assert_same(_slow(case, t, kind), _fast(case, t, kind), f"{case} tick {t} {kind}")


@pytest.mark.parametrize("case", CASES)
def test_gangs_of_one_and_one_open_gang_are_place_at(case):
    r, _ = gr.parity_queue(case)
    cfg = pr.engine_cfg(_modes(r), r["enc"])
    k = pr.N_PODS
    for t in pr.TICKS:
        state = dr.sim_state(dr.sim_at(case, t), t)
        want = r["fast"][t]
        ones = gr.fast_gang(r["enc"]["alloc"], state, cfg, r["shapes"], r["shape_of"], np.arange(k + 1), np.ones(k, np.int32))
        for f in pr.FIELDS:
            np.testing.assert_array_equal(ones["rows"][f], want[f], err_msg=f"{case} tick {t}: {f}")
        np.testing.assert_array_equal(ones["outcome"], (want["status"] == pr.OK).astype(np.int32))
        np.testing.assert_array_equal(ones["after"], want["after"])
        one = gr.fast_gang(r["enc"]["alloc"], state, cfg, r["shapes"], r["shape_of"], [0, k], [0])
        assert one["outcome"].tolist() == [gr.ADMITTED] and one["tried"].tolist() == [k]
        for f in pr.FIELDS:
            np.testing.assert_array_equal(one["rows"][f], want[f], err_msg=f"{case} tick {t}: {f}")
        np.testing.assert_array_equal(one["after"], want["after"])


@pytest.mark.parametrize("case", CASES)
def test_a_gangs_rows_are_the_tail_of_place_at_on_the_admitted_pods_and_its_own(case):
    r, _ = gr.parity_queue(case)
    cfg = pr.engine_cfg(_modes(r), r["enc"])
    checked_blocked = 0
    for t in (pr.TICKS[0], pr.TICKS[3], pr.TICKS[-1]):
        state = dr.sim_state(dr.sim_at(case, t), t)
        ref = _fast(case, t, "partial")
        kept = []
        for g in range(len(gr.PARITY_SIZES)):
            lo, tried = int(ref["first"][g]), int(ref["tried"][g])
            own = list(range(lo, lo + tried))
            if tried:
                plain = pr.fast_place(r["enc"]["alloc"], state, cfg, r["shapes"], r["shape_of"][kept + own])
                for f in pr.FIELDS:
                    np.testing.assert_array_equal(ref["rows"][f][own], plain[f][len(kept):], err_msg=f"{case} tick {t} gang {g}: {f}")
            if ref["outcome"][g] == gr.ADMITTED:
                # (a pod of an admitted gang that was not bound Ok changed nothing: it may stay in the list)
                kept += own
            else:
                checked_blocked += 1
    assert checked_blocked >= 1 or case != "feeds"


@pytest.mark.parametrize("case", CASES)
def test_prefix_strict_and_the_state_left_behind(case):
    r, _ = gr.parity_queue(case)
    cfg = pr.engine_cfg(_modes(r), r["enc"])
    for t in pr.TICKS:
        state = dr.sim_state(dr.sim_at(case, t), t)
        full, strict = _fast(case, t, "partial"), _fast(case, t, "strict")
        # a prefix of the gangs gives a prefix of the answers
        head = gr.fast_gang(r["enc"]["alloc"], state, cfg, r["shapes"], r["shape_of"][:gr.PARITY_FIRST[7]], gr.PARITY_FIRST[:8],
                            gr.PARITY_MIN_OK[:7])
        for f in gr.SUMMARY:
            np.testing.assert_array_equal(head[f], full[f][:7])
        for f in pr.FIELDS:
            np.testing.assert_array_equal(head["rows"][f], full["rows"][f][:gr.PARITY_FIRST[7]])
        # strict equals non-strict up to and including the first block, and skips the rest
        blocked = np.nonzero(full["outcome"] == gr.BLOCKED)[0]
        cut = len(full["outcome"]) if len(blocked) == 0 else int(blocked[0]) + 1
        for f in gr.SUMMARY[2:]:
            np.testing.assert_array_equal(strict[f][:cut], full[f][:cut])
        assert (strict["outcome"][cut:] == gr.SKIPPED).all() and (strict["tried"][cut:] == 0).all()
        assert (strict["rows"]["status"][gr.PARITY_FIRST[cut]:] == gr.NOT_TRIED).all()
        # after minus the state is the sum of the admitted gangs' Ok pods
        for ref in (full, strict):
            want = np.array(state, np.int64).copy()
            for g in np.nonzero(ref["outcome"] == gr.ADMITTED)[0]:
                for j in range(int(ref["first"][g]), int(ref["first"][g]) + int(ref["size"][g])):
                    if ref["rows"]["status"][j] == pr.OK:
                        sh = int(r["shape_of"][j])
                        km = int(r["shapes"]["keymask"][sh])
                        for c in range(3):
                            if (km >> c) & 1:
                                want[ref["rows"]["node"][j], c] += int(r["shapes"]["req"][sh][c])
                        want[ref["rows"]["node"][j], 3] += 1
            np.testing.assert_array_equal(ref["after"], want)
            assert int(ref["info"][5]) == int((ref["after"][:, 3] - np.asarray(state)[:, 3]).sum())
