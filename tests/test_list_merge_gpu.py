"""merge_cl's score-class list merge (ks_device.h class_merge_wave / class_merge_final, ks_cand.hip)
and its E marks taken from LDS.

The merge alone: ks_selftest KS_SELFTEST_LIST_MERGE runs the kernel's merge routine and its
thread-to-list assignment on synthetic block lists against the host's topl_insert fold (the cases:
include/ks_engine.h).  The engine, chunk resolver forced, against the oracle: binds, statuses and usage
after every step (integer work: no tolerance) at node counts that put the merge at each of its shapes,
on identical nodes (one score class) and on mixed capacities whose best 12 nodes span >= 8 classes
(tests/list_merge_cases.py, pinned on the oracle by tests/test_list_merge_shapes.py).  The oracle runs
once per trace and is shared."""
import numpy as np
import pytest

import list_merge_cases as lc
from harness import assert_same_binds, encoded, make_engine
from kubesim_amd import _lib
from kubesim_amd.engine import selftest

pytestmark = pytest.mark.gpu
CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
NO_OVERLAP = _lib.KS_ENGINE_NO_OVERLAP


def test_list_merge_selftest():
    assert selftest(_lib.KS_SELFTEST_LIST_MERGE) == 0


def _no_marks(eng):
    inv = eng.debug_invariants()
    assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv


def _lockstep(tr, mode, steps, ref, batch, flags, after_step=None):
    enc = encoded(tr)
    eng = make_engine(tr, enc, mode, batch, flags)
    eng.submit(enc["pods"])
    for k, (ob, orc, ousage) in zip(steps, ref):
        assert orc == 0
        eb = eng.step(k)
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ousage)
        _no_marks(eng)
        if after_step:
            after_step(eng)
    eng.close()


@pytest.mark.parametrize("kind", ["same", "mixed"])
@pytest.mark.parametrize("n_nodes", lc.NODE_COUNTS)
def test_engine_matches_oracle(n_nodes, kind):
    """The default chain (lists of 12, the E records read directly); steps of 1, 193 and the rest."""
    _lockstep(lc.trace(n_nodes, kind), lc.MODES[kind], lc.STEPS, lc.oracle_steps(n_nodes, kind), 0, CHUNK)


@pytest.mark.parametrize("kind", ["same", "mixed"])
@pytest.mark.parametrize("n_nodes", lc.NODE_COUNTS[1:3])
def test_engine_matches_oracle_plain_chain(n_nodes, kind):
    """Without the overlap: lists of 8, the E records staged by the scan launch."""
    _lockstep(lc.trace(n_nodes, kind), lc.MODES[kind], lc.STEPS, lc.oracle_steps(n_nodes, kind), 0,
              CHUNK | NO_OVERLAP)


def test_dense_expiries_pass_two_e_nodes_per_thread():
    """256-pod batches on the dense-expiry trace: some batch's E holds more than 512 nodes (two per
    merge_cl thread), so the E marks and E keys of the nodes past them come from the plain loops."""
    n_e = []

    def window(eng):
        n_e.append(int(np.frombuffer(eng.debug_window()[:16], np.int32)[2]))

    _lockstep(lc.dense_trace(), lc.MODES["same"], lc.DENSE_STEPS, lc.dense_oracle_steps(), lc.DENSE_BATCH, CHUNK,
              after_step=window)
    print("n_e after each step:", n_e)
    assert max(n_e) > 512, n_e
