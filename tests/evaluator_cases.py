"""Cases and exact references for the evaluator tests (host build and device).

* the generators and exact floors the host tests use (tests/test_evaluator_host.py);
* `total1_exact`: the fused Filter + Score total in Python integers, written from the formulas of
  oracle/pysim.py (`_fits`, `_lr`, `_ba`, the taint / selector tests) — not from ks_device.h;
* one boundary-biased generator per evaluator domain (`edge_cases`), and the scorer / filter
  configurations each domain is run under (`CONFIGS`);
* the host build of the evaluators (tests/native/eval_host.cpp) behind `host_eval`.

A case is one node and one pod: alloc[n][4] (cpu memory gpu pods; -1 absent), run[n][4] (requested
cpu memory gpu of the running pods, running pods), req[n][3], keymask[n], masks[n][4] (taint label
tol sel).  Usage never exceeds a present capacity and is zero for an absent one (admission): the
32-bit state types rely on it.  The request of an absent key is 0, as in a PodRec.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "eval_host.cpp")
DEV_H = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc", "ks_device.h")
LIB = os.path.join(HERE, "native", "libks_hosteval.so")

WIDE, NARROW, TINY, MICRO = 0, 1, 2, 3  # ks_device.h kEval*
INT_MAX = (1 << 31) - 1


class Cfg(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("nwb", C.c_int32), ("filter_feeds", C.c_int32),
                ("filters", C.c_uint32), ("has_scorers", C.c_int32), ("w_lr", C.c_int32),
                ("w_ba", C.c_int32), ("const_total", C.c_int32), ("tick_seconds", C.c_int32),
                ("pad_", C.c_int32)]


_host = None


def host_lib():
    """ks_device.h compiled for the host (rebuilt when a source is newer)."""
    global _host
    if _host is not None:
        return _host
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(DEV_H)):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC],
                       check=True)
    L = C.CDLL(LIB)
    p = lambda: C.c_void_p
    L.ks_host_lr_n_batch.argtypes = [C.c_int64] + [p()] * 3
    L.ks_host_ba_n_batch.argtypes = [C.c_int64] + [p()] * 5
    L.ks_host_ba_batch.argtypes = [C.c_int64] + [p()] * 5
    L.ks_host_prune_batch.argtypes = [C.POINTER(Cfg), C.c_int64] + [p()] * 7
    L.ks_host_micro_batch.argtypes = [C.POINTER(Cfg), C.c_int64] + [C.c_void_p] * 7
    L.ks_host_scan_micro_batch.argtypes = [C.POINTER(Cfg), C.c_int64] + [C.c_void_p] * 6
    L.ks_host_eval_batch.argtypes = [C.POINTER(Cfg), C.c_int64] + [p()] * 5 + [C.c_uint32] + [p()] * 3
    _host = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------------------
# the host tests' generators and exact floors
# ---------------------------------------------------------------------------------------------
def _lr_exact(A, u):
    A = A.astype(np.int64); u = u.astype(np.int64)
    out = np.zeros(len(A), np.int64)
    ok = (A > 0) & (u <= A)
    out[ok] = ((A[ok] - u[ok]) * 10) // A[ok]
    return out


def _ba_exact(Ac, Am, uc, um):
    Ac = [int(x) for x in Ac]; Am = [int(x) for x in Am]; uc = [int(x) for x in uc]; um = [int(x) for x in um]
    out = []
    for a, b, x, y in zip(Ac, Am, uc, um):
        if a <= 0 or b <= 0 or x >= a or y >= b:
            out.append(0)
            continue
        D = a * b
        X = abs(x * b - y * a)
        out.append((10 * (D - X)) // D)
    return np.array(out, np.int64)


def _narrow_cases(rng, n):
    A = rng.integers(1, 1 << 29, n).astype(np.int32)
    # bias towards the floor boundaries: u = A - k*A/10 +- small
    k = rng.integers(0, 11, n)
    jitter = rng.integers(-3, 4, n)
    u = np.clip(A.astype(np.int64) - (k * A.astype(np.int64)) // 10 + jitter, 0, (1 << 30)).astype(np.int32)
    rnd = rng.random(n) < 0.3
    u[rnd] = rng.integers(0, 1 << 29, rnd.sum()).astype(np.int32)
    return A, u


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


def _mask_cases(rng, n):
    """The taint / label / toleration / selector masks of the host micro test."""
    masks = np.zeros((n, 4), np.uint64)
    bits = lambda p: np.where(rng.random(n) < p, np.uint64(1) << rng.integers(0, 64, n).astype(np.uint64), np.uint64(0))
    masks[:, 0] = bits(0.3) | bits(0.2)  # node taints
    masks[:, 1] = bits(0.5) | bits(0.5)  # node labels
    masks[:, 2] = masks[:, 0] | bits(0.3)  # tolerations: usually all
    masks[rng.random(n) < 0.2, 2] = 0
    masks[:, 3] = np.where(rng.random(n) < 0.5, masks[:, 1] & bits(1.0), bits(0.2))  # selectors
    return masks


def _micro_cases(rng, n, cap_bits):
    """The host micro test's batch: fit boundaries (free amount 0 / -1), absent (-1) and zero
    capacities, absent request keys, clamped requests, the pods capacity, the masks."""
    alloc, run3, req = _nodes(rng, n, cap_bits)
    alloc[:, 3] = rng.integers(0, 4, n)
    run = np.zeros((n, 4), np.int64)
    run[:, :3] = run3
    run[:, 3] = rng.integers(0, 4, n)
    # exact-fit and one-over boundaries, C3-like unit multiples, clamp path
    for k in range(3):
        cap = np.maximum(alloc[:, k], 0)
        edge = rng.random(n) < 0.15
        req[edge, k] = np.maximum(cap[edge] - run[edge, k] + rng.integers(-1, 2, edge.sum()), 0)
    req[rng.random(n) < 0.03, 0] = 1 << 40
    req[rng.random(n) < 0.03, 1] = (1 << 17) + 5
    req[rng.random(n) < 0.03, 2] = (1 << 17) - 1
    assert (np.maximum(alloc[:, 0], 0) * np.maximum(alloc[:, 1], 0) < (1 << 24)).all()
    keymask = rng.integers(0, 8, n).astype(np.uint32)
    masks = _mask_cases(rng, n)
    return alloc, run, req, keymask, masks


# ---------------------------------------------------------------------------------------------
# the exact total (oracle/pysim.py's formulas on one node and one pod)
# ---------------------------------------------------------------------------------------------
def total1_exact(cfg, alloc, run, req, keymask, masks):
    """(total1, on_floor): total + 1 per case (0: not a candidate) in Python integers, and whether a
    scored term of the case sits exactly on a floor boundary (10 (A - u) / A or 10 (D - X) / D an
    integer with the term inside its domain).

    pysim.py: capacity and request keys are dict entries — an absent capacity reads as 0 in the
    scores (`cap.get(name, 0)`) and fails the fit of any pod that requests the key
    (`resource_list_ge`); an absent request adds 0.  The running pods' own keys cannot fail the
    fit: their sums passed admission against the same capacity (run <= alloc, 0 where absent)."""
    n = len(keymask)
    out = np.zeros(n, np.uint32)
    on_floor = np.zeros(n, bool)
    if not cfg["has_scorers"]:
        return out, on_floor
    feeds, filters = cfg["filter_feeds"], cfg["filters"]
    w_lr, w_ba, const = cfg["w_lr"], cfg["w_ba"], cfg["const_total"]
    A_, R_, Q_, K_, M_ = alloc.tolist(), run.tolist(), req.tolist(), keymask.tolist(), masks.tolist()
    for i in range(n):
        a, r, km = A_[i], R_[i], K_[i]
        q = [Q_[i][k] if (km >> k) & 1 else 0 for k in range(3)]
        if feeds:
            ok = True
            if filters & 1:  # _fits
                for k in range(3):
                    if (km >> k) & 1 and (a[k] < 0 or a[k] < r[k] + q[k]):
                        ok = False
                if r[3] >= a[3]:
                    ok = False
            taint, label, tol, sel = M_[i]
            if filters & 2 and taint & ~tol:  # _taint_ok: every taint tolerated
                ok = False
            if filters & 4 and (label & sel) != sel:  # _selector_ok: every selector label present
                ok = False
            if not ok:
                continue
        ac, am = max(a[0], 0), max(a[1], 0)  # cap.get(name, 0)
        uc, um = r[0] + q[0], r[1] + q[1]
        lr = 0
        for cap, u in ((ac, uc), (am, um)):  # _lr
            if cap <= 0 or u > cap:
                continue
            lr += (cap - u) * 10 // cap
            on_floor[i] |= w_lr > 0 and (cap - u) * 10 % cap == 0
        lr //= 2
        ba = 0
        if not (ac <= 0 or am <= 0 or uc >= ac or um >= am):  # _ba: floor(10 (1 - |uc/ac - um/am|))
            D = ac * am
            X = abs(uc * am - um * ac)
            ba = 10 * (D - X) // D
            on_floor[i] |= w_ba > 0 and 10 * (D - X) % D == 0
        out[i] = const + w_lr * lr + w_ba * ba + 1
    return out, on_floor


# ---------------------------------------------------------------------------------------------
# boundary-biased generators, one per evaluator domain
# ---------------------------------------------------------------------------------------------
# capacity limit (exclusive) per resource, limit of cpu * memory (exclusive, None: none), and the
# (cpu, memory) pairs at and just under the limits
DOMAINS = {
    "micro": dict(cap=1 << 16, prod=1 << 24, mode=MICRO, pairs=[
        (65535, 256), (256, 65535), (4095, 4097), (4093, 4099), (257, 65279), (4000, 4194), (1280, 2048),
        (1000, 1000), (65535, 1), (1, 65535), (10, 10), (7, 3), (1, 1)]),
    "tiny": dict(cap=1 << 26, prod=1 << 26, mode=TINY, pairs=[
        ((1 << 26) - 1, 1), (1, (1 << 26) - 1), (8191, 8193), (8192, 8191), (65535, 1024), (1280, 2048),
        (6700, 10000), (3, (1 << 24) + 1), ((1 << 25) + 1, 1)]),
    "narrow": dict(cap=1 << 29, prod=None, mode=NARROW, pairs=[
        ((1 << 29) - 1, (1 << 29) - 1), ((1 << 29) - 1, (1 << 29) - 3), (1 << 28, (1 << 29) - 1),
        ((1 << 29) - 1, 1000), (7, (1 << 29) - 1), (500000000, 500000000), (1 << 26, 1 << 26),
        ((1 << 26) + 1, 3)]),
    # the chunk resolver's wide class: capacities in one 32-bit word, evaluated by the wide evaluator
    "words": dict(cap=(1 << 32) - 1, prod=None, mode=WIDE, pairs=[
        (1 << 31, 1 << 31), ((1 << 32) - 2, (1 << 32) - 2), ((1 << 31) - 1, (1 << 31) + 1),
        ((1 << 32) - 2, 1 << 29), (1 << 29, (1 << 32) - 2), (4000000000, 4000000000), (1 << 31, 10),
        (3, (1 << 32) - 2)]),
    # bit lengths summing to 59 (BalancedAllocation in 64 bits) and 60 and above (in 128 bits)
    "wide": dict(cap=1 << 59, prod=None, mode=WIDE, pairs=[
        ((1 << 30) - 1, (1 << 29) - 1), (1 << 29, 1 << 28), ((1 << 30) - 1, (1 << 30) - 1), (1 << 29, 1 << 29),
        ((1 << 59) - 1, (1 << 59) - 1), ((1 << 59) - 1, 1), (1, (1 << 59) - 1), ((1 << 58) + 1, 10),
        (10 ** 17, 10 ** 17), ((1 << 40) + 1, (1 << 19) - 1), ((1 << 40) + 1, 1 << 19),
        ((1 << 58), (1 << 58) + 1)]),
}

# requests at each evaluator's clamp threshold (2^17 micro, 2^27 tiny, 2^30 narrow) +- 1, and far above
CLAMP_REQS = [t + d for t in (1 << 17, 1 << 27, 1 << 30) for d in (-1, 0, 1)] + [1 << 40, (1 << 59) - 1]
# pods capacities: 0, small, the clamp INT_MAX and above it
PODS_CAPS = [0, 1, 3, 110, INT_MAX - 1, INT_MAX, INT_MAX + 1, INT_MAX + 6, 1 << 40]


def _rand_caps(rng, n, dom):
    """Random (cpu, memory) in the domain, log-uniform in size, the product limit kept."""
    cap, prod = dom["cap"], dom["prod"]
    bits = np.log2(cap)
    ac = np.minimum((2.0 ** (rng.random(n) * bits)).astype(np.float64), cap - 1)
    lim = np.full(n, float(cap - 1)) if prod is None else np.minimum(cap - 1, np.floor((prod - 1) / np.maximum(ac, 1)))
    ac_i = [min(max(1, int(x)), cap - 1) for x in ac]
    am_i = [min(max(1, int(l * f)), cap - 1) for l, f in zip(lim, rng.random(n) ** 2)]
    return ac_i, am_i


def edge_cases(domain, n=20000, seed=0):
    """n cases of one evaluator domain, biased to where a floor or a comparison can flip."""
    dom = DOMAINS[domain]
    rng = np.random.default_rng(seed * 7919 + sorted(DOMAINS).index(domain))
    cap = dom["cap"]
    pairs = dom["pairs"]
    for a, b in pairs:
        assert 0 < a < cap and 0 < b < cap and (dom["prod"] is None or a * b < dom["prod"]), (domain, a, b)
    rc_, rm_ = _rand_caps(rng, n, dom)
    pick = rng.integers(0, len(pairs), n)
    named = rng.random(n) < 0.6
    A = [[pairs[pick[i]][0] if named[i] else rc_[i], pairs[pick[i]][1] if named[i] else rm_[i], 0, 0]
         for i in range(n)]
    gcap = rng.random(n)
    for i in range(n):
        A[i][2] = int(gcap[i] ** 3 * (cap - 1)) if gcap[i] < 0.9 else cap - 1
    # absent and zero capacities
    for k in range(3):
        for i in np.flatnonzero(rng.random(n) < 0.04):
            A[i][k] = -1
        for i in np.flatnonzero(rng.random(n) < 0.03):
            A[i][k] = 0
    ap = rng.integers(0, len(PODS_CAPS), n)
    # usage u = running + request: at A - floor(k A / 10) + j (k = 0..10, j = -2..2), BalancedAllocation-balanced
    # (um ~ uc Am / Ac +- 2), or anywhere
    kk = rng.integers(0, 11, (n, 3)); jj = rng.integers(-2, 3, (n, 3))
    jj[rng.random((n, 3)) < 0.4] = 0
    kind = rng.random((n, 3)); frac = rng.random((n, 3)); split = rng.random((n, 3))
    bal = rng.random(n) < 0.25; bj = rng.integers(-2, 3, n)
    baf = rng.random(n) < 0.3
    run = np.zeros((n, 4), object); req = np.zeros((n, 3), object)
    for i in range(n):
        u = [0, 0, 0]
        for k in range(3):
            a = max(A[i][k], 0)
            if kind[i, k] < 0.75:
                u[k] = a - (int(kk[i, k]) * a) // 10 + int(jj[i, k])
            else:
                u[k] = int(frac[i, k] * (a + 1))
            u[k] = max(u[k], 0)
        if bal[i] and A[i][0] > 0 and A[i][1] > 0:
            u[1] = max(u[0] * A[i][1] // A[i][0] + int(bj[i]), 0)
        elif baf[i] and A[i][0] >= 10 and A[i][1] > 0:
            # BalancedAllocation on a floor boundary or one unit off: X = uc Am = k D / 10 (+- Am)
            A[i][0] -= A[i][0] % 10
            u[0] = max(int(kk[i, 0]) % 10 * (A[i][0] // 10) + (int(bj[i]) if abs(bj[i]) == 1 else 0), 0)
            u[1] = 0
        for k in range(3):
            a = max(A[i][k], 0)
            s = split[i, k]
            r = min(u[k], a) if s < 0.3 else 0 if s < 0.5 else int(min(u[k], a) * (s - 0.5) * 2)
            run[i, k] = r
            req[i, k] = min(u[k] - r, (1 << 59) - 1)  # ks_submit_pods admits requests below 2^59
        A[i][3] = PODS_CAPS[ap[i]]
    # running pods against the pods capacity: 0, ap - 1, ap, a few (below INT_MAX: one node never
    # runs 2^31 - 1 pods, and with ap clamped to INT_MAX the test nr < ap stays exact below it)
    nk = rng.integers(0, 4, n); few = rng.integers(0, 4, n)
    for i in range(n):
        a3 = A[i][3]
        nr = (0, a3 - 1, a3, int(few[i]))[nk[i]]
        run[i, 3] = min(max(nr, 0), INT_MAX - 1)
    # requests at the clamp thresholds
    cl = rng.random((n, 3)) < 0.04; cv = rng.integers(0, len(CLAMP_REQS), (n, 3))
    for i, k in zip(*np.nonzero(cl)):
        req[i, k] = CLAMP_REQS[cv[i, k]]
    # absent request keys (their request is 0)
    keymask = np.where(rng.random(n) < 0.6, 7, rng.integers(0, 8, n)).astype(np.uint32)
    for k in range(3):
        req[(keymask >> k) & 1 == 0, k] = 0
    alloc = np.array(A, np.int64)
    run = run.astype(np.int64); req = req.astype(np.int64)
    for k in range(3):  # the invariant
        assert ((run[:, k] >= 0) & (run[:, k] <= np.maximum(alloc[:, k], 0))).all()
    return dict(alloc=alloc, run=run, req=req, keymask=keymask, masks=_mask_cases(rng, n))


def nodes_cases(cap_bits, seed, n=50000):
    """The host prune test's `_nodes` batch in the case layout (no running pods, every key requested,
    no masks)."""
    rng = np.random.default_rng(seed)
    alloc, run3, req = _nodes(rng, n, cap_bits)
    run = np.zeros((n, 4), np.int64)
    run[:, :3] = run3
    return dict(alloc=alloc, run=run, req=req, keymask=np.full(n, 7, np.uint32), masks=np.zeros((n, 4), np.uint64))


def mk_cfg(feeds, filters, w_lr, w_ba, const, has_scorers=1):
    return dict(filter_feeds=feeds, filters=filters, has_scorers=has_scorers, w_lr=w_lr, w_ba=w_ba, const_total=const)


# Scorer / filter configurations per domain: unit weights under every filter, filters off (u > A
# states are scored), one weight alone, and the largest weights — 2^24 - 1 each for the micro
# evaluator's 24-bit multiplies, elsewhere up to ks_create's limit const + 10 (w_lr + w_ba) < 2^30 - 2.
_BIG = mk_cfg(1, 1, 53_000_000, 54_000_000, 3_741_000)
assert _BIG["const_total"] + 10 * (_BIG["w_lr"] + _BIG["w_ba"]) < (1 << 30) - 2
_COMMON = [mk_cfg(1, 7, 1, 1, 0), mk_cfg(0, 0, 7, 13, 5), mk_cfg(1, 3, 0, 3, 3), mk_cfg(1, 5, 2, 0, 0)]
CONFIGS = {d: _COMMON + [_BIG] for d in DOMAINS}
CONFIGS["micro"] = _COMMON + [mk_cfg(1, 1, (1 << 24) - 1, (1 << 24) - 1, 1000)]


def modes_for(domain):
    """The evaluators whose domain admits every case of the generator (each is exact on every
    narrower domain); the 32-bit state forms also need capacities below 2^32 - 1."""
    return list(range(WIDE, DOMAINS[domain]["mode"] + 1))


def words_ok(domain):
    return DOMAINS[domain]["cap"] <= (1 << 32) - 1


# ---------------------------------------------------------------------------------------------
# the host build
# ---------------------------------------------------------------------------------------------
def host_eval(cfg, cases, modes, scan=False, prune=True):
    """The host build's columns: total1[5][n] (modes 0..3, 4 the scan form), tmax[4][n], live[4][n]."""
    L = host_lib()
    n = len(cases["keymask"])
    c = Cfg(n_nodes=n, nwb=0, filter_feeds=cfg["filter_feeds"], filters=cfg["filters"],
            has_scorers=cfg["has_scorers"], w_lr=cfg["w_lr"], w_ba=cfg["w_ba"], const_total=cfg["const_total"],
            tick_seconds=1)
    variants = 0
    for m in modes:
        variants |= 1 << m
        if prune:
            variants |= 1 << (5 + m)
    if scan:
        variants |= 1 << 4
    total1 = np.zeros((5, n), np.uint32); tmax = np.zeros((4, n), np.uint32); live = np.zeros((4, n), np.uint32)
    L.ks_host_eval_batch(C.byref(c), n, _p(cases["alloc"]), _p(cases["run"]), _p(cases["req"]), _p(cases["keymask"]),
                         _p(cases["masks"]), variants, _p(total1), _p(tmax), _p(live))
    return total1, tmax, live


def live_exact(cfg, cases):
    """PruneF.live's definition: some pod can make the node a candidate."""
    full = cases["run"][:, 3] >= cases["alloc"][:, 3]
    fit_on = bool(cfg["filter_feeds"]) and bool(cfg["filters"] & 1)
    return (np.full(len(full), bool(cfg["has_scorers"])) & ~(fit_on & full)).astype(np.uint32)
