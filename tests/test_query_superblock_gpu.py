"""Past-tick queries past a super block of the run-interval index (ks_queries.cpp usage_blocks): a
super block is 64 blocks of 256 pods, dropped whole from a query over ticks >= t_lo when its latest
run end is <= t_lo.

17,500 pods, one per tick, run for 20 ticks at the most — except four stragglers that run past the
end of the run: in blocks 3 and 40, at index 16,383 (the last pod of super block 0) and at 16,384
(the first of super block 1).  A query late in the run must keep exactly the stragglers' blocks of
super block 0; on the twin trace without stragglers it must skip super block 0.  Binds come from the
C oracle, states from tests/state_ref.py, counts and placements from tests/headroom_ref.py and
tests/place_ref.py.  Everything is exact integer equality.

The gather of the drain family (ks_drain.hip) walks the same candidate blocks: at every tick of AT the
nodes the stragglers run on and two others are drained, scanned for removal and consolidated, on
both traces, against tests/drain_ref.py, removable_ref.py and consolidate_ref.py.  On the twin those
nodes run only pods of super block 1 once super block 0 has ended: a gather that kept a block of
super block 0, or dropped one of super block 1, changes the eviction list.
"""
import functools

import numpy as np
import pytest

import consolidate_ref as cr
import drain_ref as dr
import headroom_ref as hr
import place_ref as pr
import removable_ref as rr
import state_ref as sr
import usage_digest as ud
from harness import MODES, assert_same_binds, encoded, make_engine, small_trace
from pysim import PySim

pytestmark = pytest.mark.gpu

MODE = "feeds_all_lrba"
N_PODS = TICKS = 17_500
BLK, SUP = 256, 64 * 256
STRAGGLERS = (3 * BLK + 17, 40 * BLK + 201, SUP - 1, SUP)
AT = (16_300, 16_384, 16_385, 16_400, 16_640, 17_000, 17_500)
WINDOWS = ((16_900, 17_501), (16_380, 16_391))
HAND = [
    ([1000, (1 << 30) * 1000, 0], 3, False, False),     # tolerates nothing
    ([-1, 3_000_000_000_001, -1], 2, True, False),      # memory only, no multiple of the unit
    ([8000, (64 << 30) * 1000, 4000], 7, True, False),  # 8 cpu / 64 Gi / 4 gpu
    ([9, 9, 9], 0, True, False),                        # the pods bound alone
]
SHAPE_PODS = (0, 4_000, 9_001, 16_383, 16_384, 16_390, 17_000, 17_499)


def _trace(stragglers):
    tr = small_trace(31, n_nodes=32, n_pods=N_PODS, arrival="stream", selectors=False)
    p = tr["pods"]
    p["arrival"][:] = 1 + np.arange(N_PODS)
    p["phase_sec"][:] = 1 + (np.arange(len(p["phase_sec"])) * 7919) % 50     # four phases at the most: <= 20 ticks
    if stragglers:
        for q in STRAGGLERS:
            p["phase_sec"][p["phase_off"][q]] = 180_000 + 10 * q                # >= 18,000 ticks
            p["req"][q] = (100, 256 * (1 << 20) * 1000, 0)
            a, b = p["phase_off"][q], p["phase_off"][q + 1]
            p["phase_use"][a:b] = p["req"][q] * (1 + np.arange(b - a))[:, None] // 4
    return tr


@functools.lru_cache(maxsize=None)
def _case(stragglers):
    tr = _trace(stragglers)
    ob = sr.oracle_binds(tr, MODES[MODE], TICKS)
    assert len(ob["pod"]) == N_PODS
    ref = sr.IntervalRef(tr, ob)
    # -- on the reference alone -------------------------------------------------------------------
    if stragglers:
        assert (ob["status"][list(STRAGGLERS)] == 0).all(), "a straggler was not bound Ok"
        run = ref.pod[(ref.b <= 17_000) & (17_000 < ref.e)]
        assert sorted(set((run[run < SUP] // BLK).tolist())) == [3, 40, 63], "blocks of super block 0 running at tick 17,000"
        assert (run == SUP).any() and (run > SUP + BLK).any()
        assert ref.e[np.isin(ref.pod, STRAGGLERS)].min() > TICKS + 500
    else:
        assert ref.e[ref.pod < SUP].max() <= 16_500, "a pod of super block 0 runs past tick 16,500"
    assert (ob["status"] == 0).sum() > 17_000
    enc = encoded(tr)
    fm, fl, sc = MODES[MODE]
    ps = PySim(tr, filter_mode=fm, filters=fl, scorers=sc)
    ps.submit(tr)
    model = dict(ps=ps, filter_mode=fm, filters=fl)
    shapes, sim = hr.make_shapes(tr, enc, model, list(SHAPE_PODS), HAND)
    elig = hr.eligibility(model, sim)
    return dict(tr=tr, enc=enc, ob=ob, ref=ref, shapes=shapes, elig=elig, cfg=pr.engine_cfg(MODES[MODE], enc))


@functools.lru_cache(maxsize=None)
def _drained():
    """the nodes the stragglers run on plus the two others that run the most pods over the ticks of AT
    on the twin (the same nodes on both traces)"""
    on = sorted(set(int(x) for x in _case(True)["ob"]["node"][list(STRAGGLERS)]))
    busy = sum(_case(False)["ref"].at(t)[:, 3] for t in AT)
    return tuple(on + [int(x) for x in np.argsort(-busy, kind="stable") if x not in on][:2])


@functools.lru_cache(maxsize=None)
def _drain_refs(stragglers, t):
    """(drain, removal scan, consolidation in the given and the reverse order) of _drained() at tick t"""
    r = _case(stragglers)
    tr, enc, ob, cfg, nodes = r["tr"], r["enc"], r["ob"], r["cfg"], _drained()
    state = r["ref"].at(t)
    ev, frm = dr.running_on(tr, enc, ob, t, nodes)
    drain = dr.fast_drain(enc["alloc"], state, cfg, enc["pods"], ev, frm, nodes)
    # -- on the reference alone -------------------------------------------------------------------
    assert (np.diff(drain["pod"]) > 0).all()
    if stragglers:
        assert set(STRAGGLERS) <= set(drain["pod"].tolist()) or t < STRAGGLERS[-1] + 1
    elif t >= 16_640:
        assert len(ev) >= 1 and min(ev) >= SUP, "the twin's drained nodes run a pod of super block 0"
    rem = rr.fast_removable(tr, enc, ob, cfg, t, nodes, state=state)
    cons = [cr.fast_consolidate(tr, enc, ob, cfg, t, order, state=state) for order in (nodes, nodes[::-1])]
    return drain, rem, cons


def _check(stragglers):
    r = _case(stragglers)
    ref, enc, shapes = r["ref"], r["enc"], r["shapes"]
    eng = make_engine(r["tr"], enc, MODE, batch_pods=64)
    eng.submit(enc["pods"])
    assert_same_binds(eng.step(TICKS), r["ob"])
    k = len(shapes["keymask"])
    shape_of = np.array([(5 * i) % k for i in range(2 * k)], np.int32)
    for t in AT:
        state = ref.at(t)
        assert state[:, 3].sum() >= (4 if stragglers else 1)
        np.testing.assert_array_equal(eng.requested_at(t), state, err_msg=f"requested at tick {t}")
        np.testing.assert_array_equal(eng.usage_at(t), ref.usage_window(t, t + 1)[0], err_msg=f"usage at tick {t}")
        cols, counts = hr.reference(enc["alloc"], state[None], shapes, r["elig"])
        out, pn = eng.headroom_at(t, shapes, per_node=True)
        np.testing.assert_array_equal(pn, counts[0], err_msg=f"headroom counts at tick {t}")
        np.testing.assert_array_equal(out, cols[0], err_msg=f"headroom at tick {t}")
        want = pr.fast_place(enc["alloc"], state, r["cfg"], shapes, shape_of)
        pr.assert_same(eng.place_at(t, shapes, shape_of, after=True), want, f"place at tick {t}")
        nodes = _drained()
        drain, rem, cons = _drain_refs(stragglers, t)
        dr.assert_same(eng.drain_at(t, nodes, after=True), drain, f"drain at tick {t}")
        rr.assert_same(eng.removable_at(t, nodes, rows=True), rem, f"removable at tick {t}")
        for order, want in zip((nodes, nodes[::-1]), cons):
            cr.assert_same(eng.consolidate_at(t, order, rows=True, after=True), want, f"consolidate at tick {t} from {order[0]}")
    for lo, hi in WINDOWS:
        w = ref.window(lo, hi)
        np.testing.assert_array_equal(eng.node_peaks(lo, hi), w.max(axis=0), err_msg=f"peaks [{lo}, {hi})")
        np.testing.assert_array_equal(eng.cluster_series(lo, hi), ref.series(lo, hi), err_msg=f"series [{lo}, {hi})")
        np.testing.assert_array_equal(eng.usage_digest(lo, hi), ud.digest_from_matrices(ref.usage_window(lo, hi)),
                                      err_msg=f"digest [{lo}, {hi})")
        cols, _ = hr.reference(enc["alloc"], w, shapes, r["elig"])
        np.testing.assert_array_equal(eng.headroom_series(lo, hi, shapes), cols[:, :, :2], err_msg=f"headroom [{lo}, {hi})")
    eng.close()


def test_queries_past_a_super_block_with_and_without_stragglers():
    _case(True), _case(False)       # both references and their conditions before any engine
    assert 3 <= len(_drained()) <= 6
    moved = [sum(len(_drain_refs(s, t)[0]["pod"]) for t in AT) for s in (True, False)]
    assert min(moved) >= len(AT), moved    # on either trace the gather has a pod to find at most ticks
    _check(True)
    _check(False)                   # the twin: super block 0 is skipped whole at every tick past 16,500
