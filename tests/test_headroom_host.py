"""The headroom count of ks_query.h (headroom_count / head_div: a float or double estimate with an
exact step either way, an early clamp test, an exact 64-bit fallback), compiled for the host
(tests/native/headroom_host.cpp) and checked against Python integers (tests/headroom_ref.py
count_exact, written from the header's closed form) and against the literal loop that admits copies
one at a time with fits() — Node.CreatePod's admission test (kubesim/node/node.go:44-47) — until it
fails.  Everything is exact integer equality; no device is needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from headroom_ref import NODE_MAX, count_exact

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "headroom_host.cpp")
DEV_H = [os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc", h) for h in ("ks_device.h", "ks_query.h")]
LIB = os.path.join(HERE, "native", "libks_hosthead.so")

TOP = (1 << 59) - 1          # the largest admitted quantity
LOOP_MAX = 10_000            # the literal loop runs on the cases whose count is at most this


@functools.lru_cache(maxsize=None)
def host_lib():
    """ks_query.h's headroom functions compiled for the host (rebuilt when a source is newer)."""
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [SRC, *DEV_H]):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    L = C.CDLL(LIB)
    p = C.c_void_p
    L.ks_host_headroom_batch.argtypes = [C.c_int64] + [p] * 7
    L.ks_host_headroom_batch.restype = None
    L.ks_host_headroom_loop.argtypes = [C.c_int64] + [p] * 4 + [C.c_int64, p]
    L.ks_host_headroom_loop.restype = None
    L.ks_host_head_div_batch.argtypes = [C.c_int64, p, p, p]
    L.ks_host_head_div_batch.restype = None
    L.ks_host_head_thresholds.argtypes = [p]
    L.ks_host_head_thresholds.restype = None
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def thresholds():
    out = np.zeros(4, np.uint64)
    host_lib().ks_host_head_thresholds(_p(out))
    return [int(x) for x in out]   # float tier, double tier, clamp request bound, clamp


# a case: (alloc_dev[4], run_dev[4], scale[3], req[3], keymask), Python integers
def _case(free, q, key=0, scale=1, used=0, ap=1 << 40, nr=0, keymask=None):
    """One key `key` with `free` milli-units left (a multiple of scale) above `used` device units."""
    assert free % scale == 0
    alloc, run, sc, req = [-1, -1, -1, ap], [0, 0, 0, nr], [1, 1, 1], [0, 0, 0]
    alloc[key], run[key], sc[key], req[key] = free // scale + used, used, scale, q
    assert alloc[key] * scale <= TOP
    return alloc, run, sc, req, (1 << key) if keymask is None else keymask


def edge_cases():
    f_max, d_max, q_clamp, clamp = thresholds()
    assert clamp == NODE_MAX
    out = []
    for q in (1, 2, 3, 7, 1000, 4097, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, (1 << 28) - 1, 1 << 28, (1 << 28) + 1,
              (1 << 31) - 1, 1 << 31, (1 << 32) + 1, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, TOP - 1, TOP):
        for key in range(3):
            # free amount 0, q - 1, q, q + 1 and the same around larger multiples
            for free in (0, q - 1, q, q + 1, 2 * q - 1, 2 * q, 5 * q + q // 2, 1000 * q - 1, 1000 * q):
                if 0 <= free <= TOP:
                    out.append(_case(free, q, key))
            # numerators on either side of each fast-path threshold
            for edge in (f_max, d_max, q * q_clamp, q * clamp):
                for free in (edge - 2, edge - 1, edge, edge + 1, edge + q):
                    if 0 <= free <= TOP:
                        out.append(_case(free, q, key))
    # counts at the clamp - 1, the clamp, the clamp + 1 (clamped), resources and pods
    for q in (1, 3, 1000, (1 << 28) - 1):
        for c in (clamp - 1, clamp, clamp + 1):
            for extra in (0, q - 1):
                if c * q + extra <= TOP:
                    out.append(_case(c * q + extra, q, 1))
    for c in (clamp - 1, clamp, clamp + 1, TOP):
        out.append(_case(TOP, 1, 0, ap=c))
        out.append(_case(TOP, 1, 0, ap=c, keymask=0))
    # A = 2^59 - 1 with scale 1 and with a large scale; q = 2^59 - 1; q = 1
    big = 1 << 40
    for q in (1, 2, (1 << 27) + 1, (1 << 28) + 3, (1 << 58) + 12345, TOP):
        out.append(_case(TOP, q, 1))
        out.append(_case(TOP // big * big, q, 1, scale=big))
        out.append(_case((TOP // big - 5) * big, q, 1, scale=big, used=5))
        out.append(_case(TOP // 1000 * 1000, q, 0, scale=1000, used=0))
    # a request coprime to the unit, free amounts around its multiples
    for scale, q in ((1000, 7), (1000, 1001), (268435456000, 12348030976001), (1 << 20, (1 << 33) + 1)):
        for mult in (1, 2, 33, 4000):
            for d in (-1, 0, 1):
                free = (mult * q) // scale * scale + d * scale
                if 0 <= free <= TOP:
                    out.append(_case(free, q, 1, scale=scale, used=3))
    # an absent key with a request of 0 (and with a request), all-zero requests, an empty keymask
    out.append(([-1, 100, 100, 110], [0, 0, 0, 0], [1, 1, 1], [0, 10, 10], 7))
    out.append(([100, -1, 100, 110], [0, 0, 0, 0], [1, 1, 1], [10, 0, 10], 7))
    out.append(([100, 100, -1, 110], [0, 0, 0, 0], [1, 1, 1], [10, 10, 0], 7))
    out.append(([100, 100, -1, 110], [0, 0, 0, 0], [1, 1, 1], [10, 10, 5], 3))   # the absent key is not masked
    out.append(([-1, -1, -1, 110], [0, 0, 0, 7], [1, 1, 1], [5, 5, 5], 0))
    out.append(([100, 100, 100, 110], [10, 20, 30, 4], [1, 1, 1], [0, 0, 0], 7))
    out.append(([100, 100, 100, 110], [10, 20, 30, 4], [1, 1, 1], [9, 9, 9], 0))
    out.append(([0, 0, 0, 110], [0, 0, 0, 0], [1, 1, 1], [0, 0, 0], 7))
    out.append(([0, 0, 0, 110], [0, 0, 0, 0], [1, 1, 1], [1, 1, 1], 7))
    # ap = 0, nr = ap, nr > ap
    for ap, nr in ((0, 0), (0, 3), (110, 110), (110, 111), (110, 109), (TOP, TOP), (TOP, 0), (TOP, TOP - 1)):
        out.append(([100, 100, 100, ap], [0, 0, 0, nr], [1, 1, 1], [10, 10, 10], 7))
        out.append(([100, 100, 100, ap], [0, 0, 0, nr], [1, 1, 1], [10, 10, 10], 0))
    # every limiting-key tie: bounds equal on each subset of {cpu, memory, gpu, pods}
    for tie in range(1, 16):
        b = [4 if (tie >> k) & 1 else 9 for k in range(4)]
        out.append(([b[0] * 10, b[1] * 7 + 6, b[2] * 3 + 2, b[3] + 2], [0, 0, 0, 2], [1, 1, 1], [10, 7, 3], 7))
        out.append(([b[0] * 10, b[1] * 7 + 6, b[2] * 3 + 2, b[3] + 2], [0, 0, 0, 2], [5, 3, 2], [50, 21, 6], 7))
    # ties at 0 and at the clamp
    out.append(([5, 5, 5, 0], [0, 0, 0, 0], [1, 1, 1], [10, 10, 10], 7))
    out.append(([50, 5, 5, 3], [0, 0, 0, 0], [1, 1, 1], [10, 10, 10], 6))
    out.append(([1 << 40, 1 << 41, 1 << 42, 1 << 43], [0, 0, 0, 0], [1, 1, 1], [1, 1, 1], 7))
    out.append(([1 << 20, 1 << 41, 1 << 42, 1 << 43], [0, 0, 0, 0], [1, 1, 1], [1, 1, 1], 6))
    return out


def fuzz_cases(n, seed=20260):
    """Boundary-biased random cases over the whole admitted domain."""
    rng = np.random.default_rng(seed)
    pick = lambda *xs: xs[int(rng.integers(len(xs)))]
    out = []
    for _ in range(n):
        alloc, run, sc, req = [0] * 4, [0] * 4, [1] * 3, [0] * 3
        for k in range(3):
            scale = pick(1, 1, 1, 10, 1000, 1 << int(rng.integers(0, 41)), 268435456000, int(rng.integers(1, 1 << 20)))
            a_milli = int(rng.integers(0, 1 << int(rng.integers(1, 60))))
            a = a_milli // scale
            u = pick(0, a, a - min(a, int(rng.integers(0, 4))), int(rng.integers(0, a + 1)), int(rng.integers(0, a + 1)))
            if rng.random() < 0.04:
                a, u = -1, 0
            free = max(a - u, 0) * scale
            how = int(rng.integers(0, 8))
            if how == 0:
                q = 0
            elif how <= 3 and free > 0:     # the free amount near a multiple of the request
                q = max(free // int(rng.integers(1, 1 << int(rng.integers(1, 34)))) + int(rng.integers(-1, 2)), 0)
            elif how == 4:
                q = int(rng.integers(1, 1 << 12))
            else:
                q = int(rng.integers(0, 1 << int(rng.integers(1, 60))))
            alloc[k], run[k], sc[k], req[k] = a, u, scale, min(q, TOP)
        ap = pick(0, 110, int(rng.integers(0, 300)), 1 << 40, 1 << 40, NODE_MAX + int(rng.integers(-2, 3)),
                  int(rng.integers(0, 1 << int(rng.integers(1, 60)))))
        nr = pick(0, 0, ap, ap + 1, int(rng.integers(0, ap + 1)), max(ap - int(rng.integers(0, 40)), 0))
        alloc[3], run[3] = ap, min(nr, TOP)
        out.append((alloc, run, sc, req, int(rng.integers(0, 8))))
    return out


@functools.lru_cache(maxsize=None)
def batch():
    cases = edge_cases() + fuzz_cases(200_000)
    exact = [count_exact([a * s if a >= 0 else -1 for a, s in zip(al[:3], sc)] + [al[3]],
                         [r * s for r, s in zip(ru[:3], sc)] + [ru[3]], rq, km)
             for al, ru, sc, rq, km in cases]
    return cases, exact


def _arrays(cases):
    i64 = lambda rows: np.array(rows, np.int64)
    return (i64([c[0] for c in cases]), i64([c[1] for c in cases]), i64([c[2] for c in cases]),
            i64([c[3] for c in cases]), np.array([c[4] for c in cases], np.uint32))


def test_batch_is_not_degenerate():
    cases, exact = batch()
    assert len(cases) >= 200_000
    counts = np.array([c for c, _ in exact], np.int64)
    keys = np.array([k for _, k in exact])
    for k in range(4):
        assert (keys == k).sum() > 1000, f"limiting key {k} on too few cases"
    assert (counts == NODE_MAX).sum() > 100, "too few cases at the clamp"
    assert (counts == 0).sum() > 1000
    assert ((counts > 0) & (counts <= LOOP_MAX)).sum() > 10_000, "too few cases for the literal loop"
    assert ((counts > LOOP_MAX) & (counts < NODE_MAX)).sum() > 1000, "too few large counts below the clamp"
    # every tier of the division is reached: numerators below the float bound, below the double
    # bound, above it; requests on both sides of the clamp's bound
    f_max, d_max, q_clamp, _ = thresholds()
    nums = [max(al[k] - ru[k], 0) * sc[k] for al, ru, sc, rq, km in cases for k in range(3) if (km >> k) & 1 and rq[k] > 0]
    assert sum(1 for x in nums if 0 < x < f_max) > 1000
    assert sum(1 for x in nums if f_max <= x < d_max) > 1000
    assert sum(1 for x in nums if x >= d_max) > 1000


def test_count_and_limiting_key_equal_python_integers():
    cases, exact = batch()
    alloc, run, scale, req, km = _arrays(cases)
    n = len(cases)
    count, key = np.zeros(n, np.int32), np.zeros(n, np.int32)
    host_lib().ks_host_headroom_batch(n, _p(alloc), _p(run), _p(scale), _p(req), _p(km), _p(count), _p(key))
    want_c = np.array([c for c, _ in exact], np.int64)
    want_k = np.array([k for _, k in exact], np.int64)
    bad = np.nonzero((count != want_c) | (key != want_k))[0]
    assert len(bad) == 0, f"{len(bad)} mismatches; first: case {cases[bad[0]]} got ({count[bad[0]]}, {key[bad[0]]}) " \
                          f"want {exact[bad[0]]}"


def test_count_equals_the_literal_admission_loop():
    cases, exact = batch()
    small = [i for i, (c, _) in enumerate(exact) if c <= LOOP_MAX]
    sub = [cases[i] for i in small]
    alloc, run, scale, req, km = _arrays(sub)
    # the loop works in milli-units: alloc and state times the scale
    alloc_m, run_m = alloc.copy(), run.copy()
    alloc_m[:, :3] = np.where(alloc[:, :3] >= 0, alloc[:, :3] * scale, -1)
    run_m[:, :3] = run[:, :3] * scale
    got = np.zeros(len(sub), np.int64)
    host_lib().ks_host_headroom_loop(len(sub), _p(alloc_m), _p(run_m), _p(req), _p(km), LOOP_MAX + 1, _p(got))
    want = np.array([exact[i][0] for i in small], np.int64)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, f"{len(bad)} mismatches; first: case {sub[bad[0]]} loop {got[bad[0]]} closed form {want[bad[0]]}"


def test_division_alone_around_its_thresholds():
    f_max, d_max, q_clamp, clamp = thresholds()
    rng = np.random.default_rng(7)
    num, q = [], []
    for edge in (f_max, d_max, 1 << 32, 1 << 24, TOP):
        for d in range(-3, 4):
            x = edge + d
            if not 0 <= x <= TOP:
                continue
            for qq in (1, 2, 3, 5, 1000, x // 3 + 1, x // 2, max(x - 1, 1), x, min(x + 1, TOP), (1 << 28) - 1, 1 << 28,
                       int(rng.integers(1, 1 << 30))):
                num.append(x)
                q.append(max(qq, 1))
    for _ in range(100_000):
        x = int(rng.integers(0, 1 << int(rng.integers(1, 60))))
        qq = int(rng.integers(1, 1 << int(rng.integers(1, 60))))
        if rng.random() < 0.5 and x:     # exact multiples and their neighbours
            m = int(rng.integers(1, 1 << int(rng.integers(1, 32))))
            qq = max(x // m, 1)
            x = min(qq * m + int(rng.integers(-1, 2)), TOP)
        num.append(max(x, 0))
        q.append(qq)
    a, b = np.array(num, np.uint64), np.array(q, np.uint64)
    out = np.zeros(len(num), np.int64)
    host_lib().ks_host_head_div_batch(len(num), _p(a), _p(b), _p(out))
    want = np.array([min(x // y, clamp) for x, y in zip(num, q)], np.int64)
    bad = np.nonzero(out != want)[0]
    assert len(bad) == 0, f"first: {num[bad[0]]} / {q[bad[0]]} got {out[bad[0]]} want {want[bad[0]]}"
