"""CPU checks of the device evaluator's integer math (ks_device.h compiled for the host).

* narrow (32-bit, float-estimate + exact correction) LeastRequested / BalancedAllocation floors
  against exact integer arithmetic;
* narrow total == wide total wherever the narrow evaluator is selected (capacities < 2^29);
* the resolver's float prune bound never undercuts the exact total (prune_tmax >= total) and is
  tight (equal to it but for values within the float slack of an integer).

The generators and exact floors live in tests/evaluator_cases.py, shared with the device tests.

This is the host build: rcp_est is an exact 1 / x here, and mul24 / umad24 / usad / f2u_sat are their
plain-C fallbacks.  The device forms (v_rcp, the 24-bit multiplies, v_sad_u32, the saturating
conversion, the 128-bit path compiled for the GPU) run the same cases and the boundary-biased ones
against exact integers in tests/test_evaluator_device_gpu.py (ks_selftest_eval, ks_selftest test 1);
tests/test_evaluator_cases.py holds the host build to the same exact reference on those cases.
"""
import ctypes as C

import numpy as np
import pytest

from evaluator_cases import Cfg, _ba_exact, _lr_exact, _micro_cases, _narrow_cases, _nodes, _p, host_lib


@pytest.fixture(scope="module")
def lib():
    return host_lib()


def test_lr_narrow_exact(lib):
    rng = np.random.default_rng(11)
    A, u = _narrow_cases(rng, 200_000)
    out = np.zeros(len(A), np.int32)
    lib.ks_host_lr_n_batch(len(A), _p(A), _p(u), _p(out))
    np.testing.assert_array_equal(out, _lr_exact(A, u))


def test_ba_narrow_exact(lib):
    rng = np.random.default_rng(12)
    n = 60_000
    Ac, uc = _narrow_cases(rng, n)
    Am, um = _narrow_cases(rng, n)
    # balanced cases: um/Am close to uc/Ac (X small, BA near 10)
    bal = rng.random(n) < 0.3
    um[bal] = np.clip((uc[bal].astype(np.int64) * Am[bal]) // Ac[bal] + rng.integers(-2, 3, bal.sum()),
                      0, (1 << 30)).astype(np.int32)
    out = np.zeros(n, np.int32)
    lib.ks_host_ba_n_batch(n, _p(Ac), _p(Am), _p(uc), _p(um), _p(out))
    np.testing.assert_array_equal(out, _ba_exact(Ac, Am, uc, um))


def test_ba_wide_exact(lib):
    rng = np.random.default_rng(13)
    n = 40_000
    Ac = rng.integers(1, 1 << 58, n, dtype=np.int64)
    Am = rng.integers(1, 1 << 58, n, dtype=np.int64)
    uc = (Ac * rng.random(n)).astype(np.int64)
    um = (Am * rng.random(n)).astype(np.int64)
    out = np.zeros(n, np.int32)
    lib.ks_host_ba_batch(n, _p(Ac), _p(Am), _p(uc), _p(um), _p(out))
    np.testing.assert_array_equal(out, _ba_exact(Ac, Am, uc, um))


def _nodes(rng, n, cap_bits):
    alloc = np.zeros((n, 4), np.int64)
    for k in range(3):
        alloc[:, k] = rng.integers(0, 1 << cap_bits, n)
    alloc[rng.random(n) < 0.05, 0] = -1
    alloc[rng.random(n) < 0.05, 1] = -1
    alloc[rng.random(n) < 0.05, 1] = 0
    alloc[:, 3] = 110
    run = np.zeros((n, 3), np.int64)
    for k in range(3):
        frac = rng.random(n) ** 0.5
        run[:, k] = np.maximum(alloc[:, k], 0) * frac
    req = np.zeros((n, 3), np.int64)
    for k in range(3):
        req[:, k] = (np.maximum(alloc[:, k], 1) * rng.random(n) ** 3 * 0.5).astype(np.int64)
    req[rng.random(n) < 0.1, 0] = 0
    return alloc, run, req


@pytest.mark.parametrize("feeds,const,w_lr,w_ba", [(1, 0, 1, 1), (0, 0, 1, 1), (1, 5, 2, 0), (0, 3, 0, 3),
                                                   (1, 0, 7, 13), (0, 1000, 50, 50)])
@pytest.mark.parametrize("cap_bits", [20, 28])
def test_prune_bound_sound(lib, feeds, const, w_lr, w_ba, cap_bits):
    rng = np.random.default_rng(cap_bits * 1000 + w_lr * 10 + w_ba + const)
    n = 50_000
    alloc, run, req = _nodes(rng, n, cap_bits)
    c = Cfg(n_nodes=n, nwb=0, filter_feeds=feeds, filters=1 if feeds else 0, has_scorers=1, w_lr=w_lr,
            w_ba=w_ba, const_total=const, tick_seconds=1)
    t1 = np.zeros(n, np.uint32); t1n = np.zeros(n, np.uint32); tm = np.zeros(n, np.uint32)
    t1t = np.zeros(n, np.uint32)
    lib.ks_host_prune_batch(C.byref(c), n, _p(alloc), _p(run), _p(req), _p(t1), _p(t1n), _p(tm), _p(t1t))
    np.testing.assert_array_equal(t1n, t1)  # narrow == wide below 2^29
    live = t1 > 0
    assert live.sum() > n // 3
    total = t1[live].astype(np.int64) - 1
    assert (total <= tm[live].astype(np.int64)).all(), "prune bound below the exact total"
    # and the bound is useful: mostly within a couple of points of the exact total
    assert np.mean(tm[live].astype(np.int64) - total) < 0.2 * (w_lr + w_ba) + 0.5


@pytest.mark.parametrize("feeds,const,w_lr,w_ba", [(1, 0, 1, 1), (0, 0, 1, 1), (1, 5, 2, 0), (0, 3, 0, 3)])
@pytest.mark.parametrize("cap_bits", [6, 11, 13])
def test_tiny_eval_exact(lib, feeds, const, w_lr, w_ba, cap_bits):
    """eval_total1_tiny == the wide evaluator while capacities and Ac*Am stay below 2^26,
    including C3-like small-denominator states (exact integer LR / BA values)."""
    rng = np.random.default_rng(1000 + cap_bits * 7 + w_lr * 3 + w_ba + const + feeds)
    n = 80_000
    alloc, run, req = _nodes(rng, n, cap_bits)
    # C3-like: multiples of small units, requests up to the capacity and beyond (clamp path)
    run[:, :2] = (run[:, :2] // 8) * 8
    req[rng.random(n) < 0.05, 0] = 1 << 40
    req[rng.random(n) < 0.05, 1] = (1 << 27) + 5
    assert (np.maximum(alloc[:, 0], 0) * np.maximum(alloc[:, 1], 0) < (1 << 26)).all()
    c = Cfg(n_nodes=n, nwb=0, filter_feeds=feeds, filters=1 if feeds else 0, has_scorers=1, w_lr=w_lr,
            w_ba=w_ba, const_total=const, tick_seconds=1)
    t1 = np.zeros(n, np.uint32); t1n = np.zeros(n, np.uint32); tm = np.zeros(n, np.uint32)
    t1t = np.zeros(n, np.uint32)
    lib.ks_host_prune_batch(C.byref(c), n, _p(alloc), _p(run), _p(req), _p(t1), _p(t1n), _p(tm), _p(t1t))
    np.testing.assert_array_equal(t1t, t1)


@pytest.mark.parametrize("feeds,filters,const,w_lr,w_ba", [(1, 7, 0, 1, 1), (0, 0, 0, 1, 1), (1, 1, 5, 2, 0),
                                                           (0, 0, 3, 0, 3), (1, 7, 0, 7, 13),
                                                           (1, 3, 1000, (1 << 24) - 1, 50)])
@pytest.mark.parametrize("cap_bits", [4, 11, 12])
def test_micro_eval_exact(lib, feeds, filters, const, w_lr, w_ba, cap_bits):
    """eval_total1_micro == the wide evaluator on the micro domain (capacities < 2^16, Ac*Am < 2^24,
    weights < 2^24): fit boundaries (free amount 0 / -1), absent (-1) and zero capacities, absent
    request keys, clamped requests, the pods capacity and the taint / selector masks."""
    rng = np.random.default_rng(5000 + cap_bits * 11 + w_lr % 97 * 3 + w_ba + const + filters)
    n = 100_000
    alloc, run, req, keymask, masks = _micro_cases(rng, n, cap_bits)
    c = Cfg(n_nodes=n, nwb=0, filter_feeds=feeds, filters=filters, has_scorers=1, w_lr=w_lr,
            w_ba=w_ba, const_total=const, tick_seconds=1)
    t1 = np.zeros(n, np.uint32); t1m = np.zeros(n, np.uint32)
    lib.ks_host_micro_batch(C.byref(c), n, _p(alloc), _p(run), _p(req), _p(keymask), _p(masks), _p(t1), _p(t1m))
    assert (t1 > 0).sum() > n // 10
    np.testing.assert_array_equal(t1m, t1)
    # the scan's form (per-pod ScanRec: clamped / fit-biased requests, complemented tolerations)
    t1s = np.zeros(n, np.uint32)
    lib.ks_host_scan_micro_batch(C.byref(c), n, _p(alloc), _p(run), _p(req), _p(keymask), _p(masks), _p(t1s))
    np.testing.assert_array_equal(t1s, t1)
    c.has_scorers = 0  # no scorer: no candidate
    lib.ks_host_scan_micro_batch(C.byref(c), n, _p(alloc), _p(run), _p(req), _p(keymask), _p(masks), _p(t1s))
    assert (t1s == 0).all()
