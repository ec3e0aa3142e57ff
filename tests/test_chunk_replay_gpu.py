"""The chunk resolver's replays (ks_chunk.hip replay()) against the oracle: final binds read from
the batch-wide bind rows across chunk boundaries, the cache phase's single replay per bound node
(through c0 into its row over [c0, c1)), pending own expiries carried over a chunk boundary, the
row-overflow and state-unknown stops, and refused binds on replayed nodes.  The traces and what
they produce: tests/chunk_replay_cases.py, checked on the oracle by tests/test_chunk_replay_shapes.py.
Binds, statuses and usage are compared after every step."""
import numpy as np
import pytest

import chunk_replay_cases as cc
from harness import assert_same_binds, encoded, engine_run, make_engine, make_oracle, oracle_run
from kubesim_amd import _lib

pytestmark = pytest.mark.gpu
CHUNK = _lib.KS_ENGINE_CHUNK_RESOLVER
# steps cut inside the first chunk, just before and after a chunk boundary, and after three chunks
STEPS = (1, 63, 65, 193)
_oracle = {}


def _oracle_steps(key, tr, mode, steps):
    """The oracle's (binds, error code, usage) after every step, computed once per (trace, mode)."""
    if key not in _oracle:
        ora = make_oracle(tr, mode)
        ora.submit(tr)
        out = []
        for k in steps:
            b, rc = oracle_run(ora, k)
            out.append((b, rc, ora.usage().copy()))
        _oracle[key] = out
    return _oracle[key]


def _steps(total):
    return STEPS + (total - sum(STEPS),)


def _check(key, tr, mode, total, batch, flags):
    steps = _steps(total)
    ref = _oracle_steps((key, str(mode)), tr, mode, steps)
    enc = encoded(tr)
    eng = make_engine(tr, enc, mode, batch, flags)
    eng.submit(enc["pods"])
    got = []
    for k, (ob, orc, ousage) in zip(steps, ref):
        eb, erc = engine_run(eng, k, k)
        assert_same_binds(eb, ob)
        assert erc == orc, (erc, orc)
        np.testing.assert_array_equal(eng.usage(), ousage)
        got.append(eb)
    eng.close()
    return np.concatenate(got)


@pytest.mark.parametrize("batch", [65, 128, 129, 192, 256])
def test_final_binds_across_chunk_boundaries(batch):
    """Batches of 65 .. 256 pods: chunks start at c0 = 64, 128 and 192, with one-pod and full last
    chunks."""
    _check("dense", cc.dense_trace(), "feeds_all_lrba", 1500, batch, CHUNK)


@pytest.mark.parametrize("batch", [129, 256])
@pytest.mark.parametrize("name", sorted(cc.FEW_NODES))
def test_many_binds_on_few_nodes(name, batch):
    tr, mode = cc.few_nodes_trace(name)
    _check(name, tr, mode, 600, batch, CHUNK)


@pytest.mark.parametrize("batch", [129, 192])
@pytest.mark.parametrize("mode", ["literal_const", "literal_lrba_filters_ignored"])
def test_admission_failures_on_replayed_nodes(mode, batch):
    _check("tight", cc.tight_trace(), mode, 900, batch, CHUNK)


def test_overlap_on_and_off_bind_identically():
    """The default engine (the next batch's scan fused into the chunk kernel) and the plain chain."""
    tr = cc.dense_trace()
    on = _check("dense", tr, "feeds_all_lrba", 1500, 192, CHUNK)
    off = _check("dense", tr, "feeds_all_lrba", 1500, 192, CHUNK | _lib.KS_ENGINE_NO_OVERLAP)
    for f in ("pod", "tick", "node", "status"):
        np.testing.assert_array_equal(on[f], off[f])
