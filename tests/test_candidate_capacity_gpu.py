"""The chunk resolver's candidate capacities under the oracle (ks_cand.hip cand_list; ks_chunk.hip
setup and commit; ks_device.h WinWS).  merge_cl hands one slot to each distinct candidate node of a
batch — up to 256 x kChR — but stages records for the first kSlotMax slots only, and the chunk
kernel numbers at most kCid candidates: it cuts the batch before the first pod that needs a higher
id, and its commit resets the marks of every claim, the ones past the staged slots included.  The
disjoint-selector traces (tracegen.spread_trace; pinned on the oracle by
tests/test_candidate_capacity.py) drive every 256-pod batch past those capacities on 4,096 nodes:

  over      more claims than staged slots (nslot_hw > slot_max): the claims past kSlotMax, the
            commit's reset of them, the cut at the cid limit on every batch, pod 0's private cids
            (claim-order engines), the direct reads past the staged slots (first-appearance engines)
  mid       kCid < nslot_hw <= slot_max: every slot staged, the batch still cut at the cid limit
  notfound  "mid" at a seed whose run stops with NotFound inside a batch that passed the cid limit

Every case is binds, ticks, statuses and usage against the oracle after each of the steps
(700, 1, rest) — integer work, no tolerance — with no slot or E-index mark left set afterwards.  The
oracle runs once per (trace, mode) and is shared.  After a cut, the next batch starts inside the
lists the previous merge kept (ks_prep.h `reuse`, counter 6) on every chain with speculative lists.

The measured nslot_hw, early stops and list reuses per engine (MI355X; slot_max 1,536) stand in each
test's docstring.  The claim-order engines number the candidates as the merge workgroups happen to
claim them, so a cut can fall on any pod after the first: their batches commit few pods each
(hundreds of early stops; the counts vary a little from run to run), while the first-appearance
engines commit about 1,024 / 8 pods per cut batch (14 early stops on "over").
"""
import numpy as np
import pytest

from harness import (SPREAD_MODES, assert_same_binds, make_engine, make_oracle, oracle_run, shard_ranks, spread_case,
                     step_ranks)
from kubesim_amd import _lib
from kubesim_amd.engine import KsError

pytestmark = pytest.mark.gpu

CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
# 256-pod batches, the largest: asked for, since a chunk-resolver engine's own default is 192 pods
# (ks_engine.cpp kChunkBatch), whose 192 x 8 static entries stay below the staged slots
BATCH = _lib.KS_WIN_MAX_B
# name -> (engine flags, shard, thread-ranks, has speculative lists)
ENGINES = {
    "single": (CHUNK, None, 0, True),                                      # two-launch overlapped chain, claim-order cids
    "plain_chain": (CHUNK | _lib.KS_ENGINE_NO_OVERLAP, None, 0, False),
    "pruned": (CHUNK | _lib.KS_ENGINE_PRUNED_LISTS, None, 0, True),
    "two_parts": (CHUNK, (1, 0, None, 2), 0, True),                        # sharded overlap, first-appearance cids
    "two_ranks": (CHUNK, None, 2, True),                                   # the same over LocalExchange
}

_oracles = {}


def _steps(m):
    return (700, 1, m - 701)


def _oracle(case, mode):
    """Per step: (the oracle's binds, error code, usage after the step); stops at an error."""
    key = (case, mode)
    if key not in _oracles:
        tr, _ = spread_case(case)
        ora = make_oracle(tr, SPREAD_MODES[mode])
        ora.submit(tr)
        out = []
        for k in _steps(tr["pods"]["m"]):
            ob, orc = oracle_run(ora, k)
            out.append((ob, orc, ora.usage().copy()))
            if orc != 0:
                break
        ora.close()
        _oracles[key] = out
    return _oracles[key]


def _run(case, mode, engine):
    """The engine(s) in lockstep with the oracle.  Returns (engines, the early stops summed over the
    steps per engine — counter 4 restarts with every step —, the error code the run ended with)."""
    flags, shard, world, _spec = ENGINES[engine]
    tr, enc = spread_case(case)
    x = None
    if world:
        engs, x = shard_ranks(tr, enc, world, 1, SPREAD_MODES[mode], batch_pods=BATCH, engine_flags=flags)
    else:
        engs = [make_engine(tr, enc, SPREAD_MODES[mode], BATCH, flags, shard=shard)]
        engs[0].submit(enc["pods"])
    early = [0] * len(engs)
    code = 0
    for k, (ob, orc, ou) in zip(_steps(tr["pods"]["m"]), _oracle(case, mode)):
        if world:
            assert orc == 0
            got = [(b, 0) for b in step_ranks(engs, k, x)]
        else:
            try:
                got = [(engs[0].step(k), 0)]
            except KsError as ex:
                got = [(ex.binds, ex.code)]
        for r, (eb, rc) in enumerate(got):
            assert rc == orc, (r, rc, orc)
            assert_same_binds(eb, ob)
            np.testing.assert_array_equal(engs[r].usage(), ou)
            early[r] += int(engs[r].debug_counters()[4])
        code = orc
    return engs, early, code


def _check_marks_and_slots(case, mode, engine, engs, early):
    """No mark left set; prints what the capacity and counter assertions read; returns per engine
    (nslot_hw, slot_max, early stops, list reuses)."""
    out = []
    for r, e in enumerate(engs):
        inv = e.debug_invariants()
        reuse = int(e.debug_counters()[6])
        print(f"{case} {mode} {engine} rank {r}: nslot_hw {inv['nslot_hw']} slot_max {inv['slot_max']} "
              f"early stops {early[r]} list reuses {reuse}")
        assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, (r, inv)
        assert inv["slot_max"] == _lib.KS_SLOT_MAX
        out.append((inv["nslot_hw"], inv["slot_max"], early[r], reuse))
    return out


def _check_reuse(engine, reuse):
    if ENGINES[engine][3]:
        assert reuse > 0, "a batch that follows a cut reuses the merged lists kept for its first pods"
    else:
        assert reuse == 0, "the plain chain has no speculative lists"


@pytest.mark.parametrize("mode", sorted(SPREAD_MODES))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_over_more_claims_than_staged_slots(engine, mode):
    """period 256, 2,048 pods: every batch claims more slots than merge_cl stages, so every batch is
    cut at the cid limit (at least half of the 8 full batches stop early: a loose floor — each cut
    batch is followed by shorter ones that may finish).

    Measured nslot_hw / early stops / list reuses, modes all_lrba, ba3_const, lr2:
      single       2,034 / 306 / 193   2,016 / 275 / 175   2,012 / 340 / 212
      plain_chain  2,011 / 345 / 0     2,011 / 483 / 0     2,011 / 324 / 0
      pruned       2,011 / 344 / 210   2,011 / 298 / 187   2,011 / 313 / 191
      two_parts    2,003 / 14 / 10 in every mode
      two_ranks    2,003 / 14 / 10 in every mode, on both ranks
    """
    engs, early, code = _run("over", mode, engine)
    assert code == 0
    m = spread_case("over")[0]["pods"]["m"]
    for hw, smax, stops, reuse in _check_marks_and_slots("over", mode, engine, engs, early):
        assert hw > smax, (hw, smax)
        assert hw <= BATCH * _lib.KS_CHR
        assert stops >= (m // BATCH) // 2, stops
        _check_reuse(engine, reuse)
    for e in engs:
        e.close()


@pytest.mark.parametrize("mode", sorted(SPREAD_MODES))
@pytest.mark.parametrize("engine", list(ENGINES))
def test_mid_more_claims_than_cids_all_staged(engine, mode):
    """period 128, 1,536 pods: more claims than the chunk kernel numbers, all of them staged.  (The
    engine keeps the E nodes that reach a list's threshold too, so its count sits a little above
    the oracle model's 1,271 .. 1,345.)

    Measured nslot_hw / early stops / list reuses, modes all_lrba, ba3_const, lr2:
      single       1,378 / 107 / 61   1,380 / 139 / 86   1,364 / 85 / 48
      plain_chain  1,354 / 91 / 0     1,366 / 73 / 0     1,341 / 95 / 0
      pruned       1,349 / 94 / 56    1,367 / 83 / 49    1,341 / 97 / 57
      two_parts    1,323 / 9 / 6      1,354 / 9 / 6      1,312 / 9 / 6
      two_ranks    as two_parts, on both ranks
    """
    engs, early, code = _run("mid", mode, engine)
    assert code == 0
    for hw, smax, stops, reuse in _check_marks_and_slots("mid", mode, engine, engs, early):
        assert _lib.KS_CHUNK_CIDS < hw <= smax, (hw, smax)
        assert stops > 0
        _check_reuse(engine, reuse)
    for e in engs:
        e.close()


@pytest.mark.parametrize("engine", ["single", "two_parts"])
def test_notfound_inside_a_batch_past_the_cid_limit(engine):
    """Seed 9: pod 1,205 finds no node (NotFound, kubesim/kubesim.go:217-220) in the batch that starts
    at pod 1,024 and claims more slots than cids.  The same error code as the oracle, the same binds
    up to it, the same usage, and the stopped batch's marks all reset.
    Measured nslot_hw / early stops / list reuses: single 1,401 / 65 / 37, two_parts 1,323 / 7 / 5."""
    engs, early, code = _run("notfound", "all_lrba", engine)
    assert code == _lib.KS_ENOTFOUND
    for hw, smax, _stops, _reuse in _check_marks_and_slots("notfound", "all_lrba", engine, engs, early):
        assert hw > _lib.KS_CHUNK_CIDS
    for e in engs:
        e.close()
