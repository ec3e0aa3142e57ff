"""The consolidation preview's host-side pieces of ks_query.h and ks_carve.h, compiled for the host
(tests/native/consolidate_host.cpp): a serial restatement of the rounds — lists of the committed state
with the removed nodes cordoned, the candidates of a round walked as transactions, the single path —
which must equal the chain as written, a copy of the cluster restored on every block; the roll-back's
three parts, each of which decides cases; who decides a candidate; the round walk; and the scratch
layout.  Exact integer equality; no device is needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import place_ref as pr
import test_drain_host as tdh
import test_place_host as tph

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "consolidate_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "native", "place_serial.h"), os.path.join(CSRC, "ks_carve.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(CSRC, "ks_query.h")]
PODREC = tdh.PODREC
RES = np.dtype([("node", np.int32), ("evicted", np.int32), ("outcome", np.int32), ("rows", np.int32),
                ("block_status", np.int32), ("pad", np.int32), ("first_row", np.int64)])
MAX_SHAPES, MAX_PODS = 64, 1024


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostconsolidate.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    p = C.c_void_p
    case = [C.c_int32, p, p, p, p, p, p, C.c_int32, p, p, p, p, C.c_int32, p, C.c_int32, p, p]
    lb.ks_host_consolidate_brute.argtypes = case + [p, p, p]
    lb.ks_host_consolidate.argtypes = case + [C.c_int32, p, p, p, p, p]
    lb.ks_host_consolidate.restype = lb.ks_host_consolidate_brute.restype = C.c_int
    lb.ks_host_consolidate_segment.argtypes = [C.c_int64, p, p, C.c_int64, p, p, p, p]
    lb.ks_host_consolidate_segment.restype = C.c_int64
    lb.ks_host_consolidate_route.argtypes = [C.c_int64]
    lb.ks_host_consolidate_route.restype = C.c_int
    lb.ks_host_consolidate_limits.argtypes = [p]
    lb.ks_host_consolidate_carve.restype = C.c_int64
    return lb


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def limits():
    out = np.zeros(10, np.int32)
    host_lib().ks_host_consolidate_limits(_p(out))
    return out.tolist()


def test_limits_are_the_headers():
    from kubesim_amd import _lib
    from kubesim_amd.engine import CONSOLIDATION_DTYPE
    lim = limits()
    assert lim[0] == _lib.KS_PLACE_MAX_SHAPES == MAX_SHAPES and lim[4] == _lib.KS_PLACE_MAX_PODS == MAX_PODS
    assert lim[1] == lim[2] - 1 == _lib.KS_CONSOLIDATE_MAX_ROUND
    assert lim[3] == CONSOLIDATION_DTYPE.itemsize == RES.itemsize == 32 and CONSOLIDATION_DTYPE == RES
    assert lim[7:10] == [_lib.KS_CONSOLIDATE_BLOCKED, _lib.KS_CONSOLIDATE_REMOVED, _lib.KS_CONSOLIDATE_DESTINATION]


def test_who_decides_a_candidate():
    lb = host_lib()
    rnd, single = limits()[5:7]
    assert rnd != single and limits()[2] == 32, "the cases below are the default list length's"
    want = {0: rnd, 1: rnd, 31: rnd, 32: single, 33: single, 110: single, 65536: single}
    assert {k: lb.ks_host_consolidate_route(k) for k in want} == want


def test_scratch_layout():
    assert host_lib().ks_host_consolidate_carve() == 0


# ---- the rounds against the chain as written ---------------------------------------------------
def run(c, nodes, counts, brute=False, mode=0):
    lb = host_lib()
    n, k, m = len(c["alloc"]), len(c["shape_of"]), len(nodes)
    assert int(np.sum(counts)) == k
    nodes, counts = np.ascontiguousarray(nodes, np.int32), np.ascontiguousarray(counts, np.int32)
    out = np.zeros(max(k, 1), tph.REC)
    res = np.zeros(m, RES)
    after = np.zeros((n, 4), np.int64)
    info, stats = np.zeros(2, np.int64), np.zeros(4, np.int64)
    args = [n, _p(c["alloc"]), _p(c["scale"]), _p(c["state"]), _p(c["taint"]), _p(c["label"]), _p(c["cfg"]),
            len(c["req"]), _p(c["req"]), _p(c["keymask"]), _p(c["tol"]), _p(c["sel"]), k, _p(c["shape_of"]), m, _p(nodes), _p(counts)]
    if brute:
        rc = lb.ks_host_consolidate_brute(*args, _p(out), _p(res), _p(after))
    else:
        rc = lb.ks_host_consolidate(*args, mode, _p(out), _p(res), _p(after), _p(info), _p(stats))
    return rc, dict(out=out, res=res, after=after, info=info, stats=stats)


def same(a, b):
    if not (a["res"] == b["res"]).all() or not (a["after"] == b["after"]).all():
        return False
    for r in a["res"]:
        lo, hi = int(r["first_row"]), int(r["first_row"] + r["rows"])
        if not (a["out"][lo:hi] == b["out"][lo:hi]).all():
            return False
    return True


def split(rng, c, big=0.15):
    """the case's k pods dealt to m distinct candidate nodes in a random order: some get none, some
    kPlaceL pods or more"""
    n, k = len(c["alloc"]), len(c["shape_of"])
    m = int(rng.integers(1, n + 1)) if rng.random() < 0.5 else min(n, int(rng.integers(1, 40)))
    nodes = rng.permutation(n)[:m]
    counts = np.zeros(m, np.int64)
    left = k
    for j in rng.permutation(m):
        if left == 0:
            break
        u = rng.random()
        take = 0 if u < 0.15 else int(rng.integers(32, 120)) if u < 0.15 + big else int(rng.integers(1, 12))
        counts[j] = min(take, left)
        left -= counts[j]
    counts[int(rng.integers(m))] += left
    return nodes, counts


def test_fuzzed_chains_equal_the_chain_as_written():
    """test_place_host's fuzz recipe; its pods are dealt to candidate nodes"""
    rng = np.random.default_rng(20261101)
    seen = dict(removed=0, blocked=0, dest=0, late_block=0, stops=0, undone=0, single=0, rounds2=0, from_d=0,
                flags=0, counts=0, nchg=0)
    statuses = set()
    n_cases = 1200
    for i in range(n_cases):
        c = tph.fuzz_case(rng)
        nodes, counts = split(rng, c)
        rc, got = run(c, nodes, counts)
        assert rc == 0, f"fuzz case {i}: the rounds stopped with {rc}"
        _, want = run(c, nodes, counts, brute=True)
        np.testing.assert_array_equal(got["res"], want["res"], err_msg=f"fuzz case {i}")
        np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"fuzz case {i}: after")
        assert same(got, want), f"fuzz case {i}: rows"
        oc = want["res"]["outcome"]
        seen["removed"] += int((oc == 1).sum())
        seen["blocked"] += int((oc == 0).sum())
        seen["dest"] += int((oc == 2).sum())
        seen["late_block"] += int(got["stats"][0])
        seen["stops"] += int(got["stats"][1])
        seen["undone"] += int(got["stats"][2])
        seen["from_d"] += int(got["stats"][3])
        seen["single"] += int(got["info"][1])
        seen["rounds2"] += int(got["info"][0] >= 2)
        statuses |= set(want["res"]["block_status"][oc == 0].tolist())
        if got["stats"][0] or got["stats"][1]:
            # each part of the roll-back alone decides cases: without it the answer differs
            for mode, key in ((1, "flags"), (2, "counts"), (3, "nchg")):
                rcm, wrong = run(c, nodes, counts, mode=mode)
                seen[key] += int(rcm != 0 or not same(wrong, want))
    assert seen["removed"] >= 3000 and seen["blocked"] >= 1000 and seen["dest"] >= 1000, seen
    assert seen["late_block"] >= 300 and seen["stops"] >= 20 and seen["undone"] >= 100 and seen["single"] >= 100, seen
    assert seen["rounds2"] >= 200 and seen["from_d"] >= 1000, seen
    assert seen["flags"] >= 50 and seen["counts"] >= 50 and seen["nchg"] >= 50, seen
    assert statuses == {pr.OVER, pr.NOT_FOUND}


def test_a_blocked_candidate_is_a_destination_later():
    """Nodes that take one pod each, a constant score: candidate 0 has two pods; the second finds no
    node in feeds mode when only one other node is free.  Rolled back, node 1 is as it was, and the
    next candidate's pod goes there: the blocked candidate's flags, counts and slots are all undone."""
    c = tph.uniform(3, 3, tph.FEEDS_CONST, ap=1)
    c["state"][2, 3] = 1            # node 2 is full
    rc, got = run(c, [0, 2], [2, 1])
    _, want = run(c, [0, 2], [2, 1], brute=True)
    assert rc == 0 and same(got, want)
    assert got["res"]["outcome"].tolist() == [0, 1] and got["res"]["rows"].tolist() == [2, 1]
    assert got["res"]["block_status"].tolist() == [pr.NOT_FOUND, 0]
    assert got["out"]["node"].tolist() == [1, -1, 0], "the pod of node 2 goes to node 0, the lowest free index"
    for mode in (1, 2, 3):
        rcm, wrong = run(c, [0, 2], [2, 1], mode=mode)
        assert rcm != 0 or not same(wrong, want), mode


# ---- the round walk ------------------------------------------------------------------------------
def segment(counts, ids, start=0):
    counts, ids = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(ids, np.int64)
    assert counts.sum() == len(ids)
    ns, npods = np.zeros(1, np.int32), np.zeros(1, np.int32)
    shape_of = np.full(MAX_PODS + 64, -1, np.int32)
    shapes = np.zeros(MAX_SHAPES, PODREC)
    end = host_lib().ks_host_consolidate_segment(len(counts), _p(counts), _p(ids), start, _p(ns), _p(npods), _p(shape_of), _p(shapes))
    first = int(counts[:start].sum())
    seg = ids[first:first + int(npods[0])].tolist()
    order = list(dict.fromkeys(seg))
    assert len(order) == ns[0] and shape_of[:npods[0]].tolist() == [order.index(x) for x in seg]
    # (rows past the round's pods may be numbered: a candidate that did not fit; never past a round's room)
    assert npods[0] == counts[start:end].sum() and (shape_of[MAX_PODS:] == -1).all()
    assert [int(r["req"][0]) for r in shapes[:ns[0]]] == [1000 + x for x in order] and (shapes["flags"] == 0).all()
    assert (shapes["req"][:ns[0], 1] == 0).all(), "an unmasked request is not part of the shape"
    return int(end), int(ns[0]), int(npods[0])


def test_round_boundaries():
    # the 65th shape: one pod per candidate, every pod a shape of its own
    assert segment(np.ones(200, int), np.arange(200)) == (64, 64, 64)
    assert segment(np.ones(200, int), np.arange(200), start=64) == (128, 64, 64)
    assert segment(np.ones(200, int), np.arange(200), start=192) == (200, 8, 8)
    # 60 shapes, then a candidate with 5 new ones: it moves whole to the next round; with 4 it stays
    ids = np.concatenate([np.arange(60), 100 + np.arange(5), [0]])
    assert segment([30, 30, 5, 1], ids) == (2, 60, 60) and segment([30, 30, 5, 1], ids, start=2) == (4, 6, 6)
    assert segment([30, 30, 4, 1], np.concatenate([np.arange(60), 100 + np.arange(4), [200]])) == (3, 64, 64)
    # the 1,025th pod: 64 candidates of 16 pods fill a round exactly; one pod more moves its candidate
    assert segment([16] * 70, np.arange(16 * 70) % 5) == (64, 5, 1024)
    assert segment([16] * 63 + [17, 3], np.arange(16 * 63 + 20) % 5) == (63, 5, 1008)
    assert segment([16] * 63 + [15, 1, 1], np.arange(16 * 64 + 1) % 5) == (65, 5, 1024)
    # candidates without pods ride along, also at the end; a candidate of the single path closes the round
    assert segment([0, 3, 0, 0, 2, 0], np.arange(5)) == (6, 5, 5)
    assert segment([0, 0, 0], []) == (3, 0, 0)
    assert segment([2, 31, 32, 1], np.arange(66) % 7) == (2, 7, 33)
    assert segment([2, 31, 32, 1], np.arange(66) % 7, start=2) == (2, 0, 0), "it heads no round: the single path"
    assert segment([2, 31, 32, 1], np.arange(66) % 7, start=3) == (4, 1, 1)
