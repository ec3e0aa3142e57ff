"""The traces of tests/test_list_merge_gpu.py on the oracle alone (tests/list_merge_cases.py): they put
merge_cl's score-class merge at both ends — one class holding every best node, and a top 12 spread
over many thin classes — and the dense-expiry trace keeps three pre-batch expiries per two ticks going."""
import numpy as np
import pytest

import list_merge_cases as lc


@pytest.mark.parametrize("n_nodes", lc.NODE_COUNTS)
def test_mixed_capacities_spread_a_top12_over_many_classes(n_nodes):
    got, classes = lc.top_classes(n_nodes, "mixed", lc.MIXED_POD)
    assert got == 12 and classes >= 8, (got, classes)


@pytest.mark.parametrize("n_nodes", lc.NODE_COUNTS[:2])
def test_identical_nodes_tie_in_one_class(n_nodes):
    for after in (0, 200):
        assert lc.top_classes(n_nodes, "same", after) == (12, 1)


@pytest.mark.parametrize("kind", sorted(lc.MODES))
def test_every_pod_binds(kind):
    for b, rc, _ in lc.oracle_steps(lc.NODE_COUNTS[0], kind):
        assert rc == 0 and (b["status"] == 0).all()


def test_dense_trace_expires_three_pods_in_two_ticks():
    """While pods DENSE_LONG .. are scheduled (one per tick), the long pods end three per two ticks:
    any 256 consecutive ticks there see about 384 of them end — below the window's 512 slots, so the
    batch is not cut, and with the previous batch's bound nodes past 512 E nodes."""
    tr = lc.dense_trace()
    p = tr["pods"]
    ticks = -(-np.add.reduceat(p["phase_sec"].astype(np.int64), p["phase_off"][:-1]) // tr["tick_seconds"])
    end = np.arange(lc.DENSE_LONG) + 1 + ticks[:lc.DENSE_LONG]
    for lo in (lc.DENSE_LONG + 100, lc.DENSE_LONG + 700, lc.DENSE_LONG + 1200):
        n = int(((end >= lo) & (end < lo + 256)).sum())
        assert 330 <= n <= 450, (lo, n)
    assert sum(lc.DENSE_STEPS) == lc.DENSE_PODS
    for b, rc, _ in lc.dense_oracle_steps():
        assert rc == 0 and (b["status"] == 0).all()
