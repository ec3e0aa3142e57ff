"""The evaluator batches the device tests run (tests/evaluator_cases.py), on the CPU: the host build of
every evaluator equals the exact Python-integer total on every boundary-biased generator, the
generators stay inside their domains, and no batch is degenerate.

Shares asserted per (generator, configuration), from the exact reference alone:
* candidates (total1 > 0): at least 30 % — with every filter on, the masks of the host micro test
  pass about six cases in ten, the pods capacity (nr = ap in a quarter of the cases) and the
  requests above the free amount (free amount -1 and -2, absent and zero capacities, the clamp
  thresholds) about eight in ten of those; filters off, every case is a candidate;
* cases with a scored term exactly on a floor boundary (10 (A - u) / A or 10 (D - X) / D an
  integer, the term inside its domain): at least 5 % — LeastRequested is on one at u = A and u = 0
  (two of the eleven placements, three fifths of them without jitter) and wherever 10 divides k A;
  BalancedAllocation alone where the generator sets X = k D / 10 (a fifth of the cases, three
  fifths of them without jitter, fewer once an absent capacity or a clamp request takes the term out).
"""
from fractions import Fraction

import numpy as np
import pytest

import evaluator_cases as ec

MIN_CANDIDATES = 0.30
MIN_ON_FLOOR = 0.05

_cache = {}


def batch(domain):
    if domain not in _cache:
        _cache[domain] = ec.edge_cases(domain)
    return _cache[domain]


@pytest.mark.parametrize("domain", sorted(ec.DOMAINS))
def test_generator_stays_in_its_domain(domain):
    b = batch(domain)
    dom = ec.DOMAINS[domain]
    alloc, run, req = b["alloc"], b["run"], b["req"]
    assert len(b["keymask"]) <= 100_000
    assert (alloc[:, :3] >= -1).all() and (alloc[:, :3] < dom["cap"]).all()
    # the limit is reached: a capacity at cap - 1 (at cap - 2 for the 32-bit words' 2^32 - 2)
    assert alloc[:, :2].max() >= dom["cap"] - 2
    if dom["prod"] is not None:
        prod = np.maximum(alloc[:, 0], 0) * np.maximum(alloc[:, 1], 0)
        assert (prod < dom["prod"]).all() and prod.max() == dom["prod"] - 1
    assert (run >= 0).all() and (run[:, :3] <= np.maximum(alloc[:, :3], 0)).all()
    assert (run[:, 3] < ec.INT_MAX).all() and (alloc[:, 3] >= 0).all() and (alloc[:, 3] > ec.INT_MAX).any()
    assert (req >= 0).all() and (req < (1 << 59)).all()
    for k in range(3):  # an absent key requests nothing
        assert (req[(b["keymask"] >> k) & 1 == 0, k] == 0).all()
    # every listed edge is present: absent and zero capacities, free amount 0 and -1, the pods
    # capacity reached and one short of it, the clamp thresholds
    free = alloc[:, :3] - run[:, :3] - req
    asked = ((b["keymask"][:, None] >> np.arange(3)) & 1) == 1
    assert (alloc[:, :3] == -1).any() and (alloc[:, :3] == 0).any()
    assert ((free == 0) & asked & (alloc[:, :3] > 0)).sum() > 100 and ((free == -1) & asked).sum() > 100
    assert (run[:, 3] == alloc[:, 3]).any() and (run[:, 3] == alloc[:, 3] - 1).any()
    for q in ec.CLAMP_REQS:
        assert (req == q).any(), q


def test_exact_reference_matches_the_rational_formula():
    """total1_exact's integer BalancedAllocation floor against pysim's Fraction expression."""
    b = batch("wide")
    cfg = ec.mk_cfg(0, 0, 0, 1, 0)
    t1, _ = ec.total1_exact(cfg, **{k: v[:3000] for k, v in b.items()})
    for i in range(3000):
        ac, am = max(int(b["alloc"][i, 0]), 0), max(int(b["alloc"][i, 1]), 0)
        uc, um = int(b["run"][i, 0] + b["req"][i, 0]), int(b["run"][i, 1] + b["req"][i, 1])
        want = 0
        if not (ac <= 0 or am <= 0 or uc >= ac or um >= am):
            want = int((1 - abs(Fraction(uc, ac) - Fraction(um, am))) * 10)
        assert int(t1[i]) - 1 == want


@pytest.mark.parametrize("domain", sorted(ec.DOMAINS))
def test_host_build_equals_exact_total(domain):
    b = batch(domain)
    modes = ec.modes_for(domain)
    n = len(b["keymask"])
    for cfg in ec.CONFIGS[domain]:
        exact, on_floor = ec.total1_exact(cfg, **b)
        assert (exact > 0).mean() >= MIN_CANDIDATES, cfg
        assert on_floor.mean() >= MIN_ON_FLOOR, cfg
        total1, tmax, live = ec.host_eval(cfg, b, modes, scan=ec.MICRO in modes)
        for m in modes:
            np.testing.assert_array_equal(total1[m], exact, err_msg=f"mode {m} {cfg}")
            # the bound is sound, and live is its definition
            cand = exact > 0
            assert (tmax[m][cand].astype(np.int64) >= exact[cand].astype(np.int64) - 1).all(), (m, cfg)
            np.testing.assert_array_equal(live[m], ec.live_exact(cfg, b))
        if ec.MICRO in modes:
            np.testing.assert_array_equal(total1[4], exact, err_msg=f"scan {cfg}")
    none = dict(ec.CONFIGS[domain][0], has_scorers=0)  # no scorer: no candidate, nothing live
    total1, tmax, live = ec.host_eval(none, b, modes, scan=ec.MICRO in modes)
    assert (total1 == 0).all() and (live == 0).all() and n > 0
