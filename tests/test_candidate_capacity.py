"""The inputs of tests/test_candidate_capacity_gpu.py, pinned on the CPU oracle alone: how many
distinct candidate nodes the 256 pods of a batch keep on the disjoint-selector traces
(tracegen.spread_trace; harness.SPREAD_CASES), against the chunk resolver's two capacities
(_lib.KS_SLOT_MAX, _lib.KS_CHUNK_CIDS).

The model.  At each batch start 0, 256, 512, ... every pod of the batch is evaluated on the
oracle's state at that point (COracle.eval) and keeps its first 8 feasible nodes by score descending,
then node index ascending — fewer than the engine keeps per pod (kChR, plus the E nodes that reach
a list's threshold), so the union of the kept nodes is a floor of the slots the engine's merge_cl
hands out for the batch.  Then the oracle steps the batch's 256 ticks.
"""
import numpy as np
import pytest

from harness import SPREAD_CASES, SPREAD_MODES, make_oracle, spread_case
from kubesim_amd import _lib

BATCH = _lib.KS_WIN_MAX_B
KEEP = 8


def _unions(tr, mode):
    """(per full batch: distinct kept nodes; the binds of the whole run; its error code)."""
    m = tr["pods"]["m"]
    ora = make_oracle(tr, mode)
    ora.submit(tr)
    nodes = np.arange(tr["nodes"]["n"])
    unions, binds, rc = [], [], 0
    for s in range(0, m, BATCH):
        if s + BATCH <= m:
            kept = set()
            for q in range(s, s + BATCH):
                feas, score = ora.eval(q)
                ok = nodes[(feas != 0) & (score >= 0)]
                kept.update(ok[np.lexsort((ok, -score[ok]))][:KEEP].tolist())
            unions.append(len(kept))
        b, rc = ora.step(BATCH, cap=BATCH)
        binds.append(b)
        if rc != 0:
            break
    ora.close()
    return unions, {k: np.concatenate([b[k] for b in binds]) for k in binds[0]}, rc


def test_spread_trace_groups_are_disjoint_and_in_every_block():
    tr, enc = spread_case("over")
    n = tr["nodes"]["n"]
    assert n == 4096 and len(np.unique(enc["label"])) == 256
    for blk in range(0, n, 256):  # every scan block holds every group once
        assert len(np.unique(enc["label"][blk:blk + 256])) == 256
    sel = enc["pods"]["sel"]
    assert len(np.unique(sel[:256])) == 256 and (sel[256:512] == sel[:256]).all()
    match = (enc["label"][None, :] & sel[:256, None]) == sel[:256, None]
    assert (match.sum(axis=1) == 16).all() and (match.sum(axis=0) == 1).all()
    # 16 label pairs: one mask holds them (bit positions are the encoder's)
    assert bin(int(np.bitwise_or.reduce(enc["label"]))).count("1") == 16


@pytest.mark.parametrize("mode", sorted(SPREAD_MODES))
def test_over_claims_more_than_the_staged_slots(mode):
    """period 256, 2,048 pods: every batch keeps more than kSlotMax + 10 % distinct nodes
    (measured on the oracle: 1,916 .. 2,003)."""
    tr, _ = spread_case("over")
    unions, binds, rc = _unions(tr, SPREAD_MODES[mode])
    print(f"over {mode}: unions {unions}")
    assert rc == 0 and len(binds["pod"]) == tr["pods"]["m"] and (binds["status"] == _lib.KS_POD_OK).all()
    assert len(unions) == tr["pods"]["m"] // BATCH
    assert all(u > _lib.KS_SLOT_MAX * 11 // 10 for u in unions), unions


@pytest.mark.parametrize("mode", sorted(SPREAD_MODES))
def test_mid_claims_between_the_cids_and_the_staged_slots(mode):
    """period 128, 1,536 pods: every batch keeps more distinct nodes than the chunk kernel numbers
    and fewer than kSlotMax - 10 % (measured on the oracle: 1,271 .. 1,345)."""
    tr, _ = spread_case("mid")
    unions, binds, rc = _unions(tr, SPREAD_MODES[mode])
    print(f"mid {mode}: unions {unions}")
    assert rc == 0 and len(binds["pod"]) == tr["pods"]["m"] and (binds["status"] == _lib.KS_POD_OK).all()
    assert len(unions) == tr["pods"]["m"] // BATCH
    assert all(_lib.KS_CHUNK_CIDS < u < _lib.KS_SLOT_MAX * 9 // 10 for u in unions), unions


def test_notfound_case_stops_inside_a_batch_past_the_cid_limit():
    """Seed 9, period 128: no node of pod 1,205's group has room left, so the oracle stops there
    with NotFound (kubesim/kubesim.go:217-220) — inside the batch that starts at pod 1,024."""
    assert SPREAD_CASES["notfound"] == dict(seed=9, n_pods=1536, period=128)
    tr, _ = spread_case("notfound")
    unions, binds, rc = _unions(tr, "feeds_all_lrba")
    print(f"notfound: unions {unions}, {len(binds['pod'])} binds, rc {rc}")
    assert rc == _lib.KS_ENOTFOUND
    assert len(binds["pod"]) == 1205 and (binds["pod"] == np.arange(1205)).all()
    assert (binds["status"] == _lib.KS_POD_OK).all()
    assert all(u > _lib.KS_CHUNK_CIDS for u in unions[:5]), unions
