"""The gang admission preview's host-side pieces of ks_query.h and ks_carve.h, compiled for the host
(tests/native/gang_host.cpp): a serial restatement of the rounds — lists of the committed state, the
gangs of a round walked as transactions, kPlaceStop inside a gang, the single path — which must equal
the chain as written, a copy of the cluster restored on every block; the roll-back's four parts, each
of which decides cases; who decides a gang; the round walk; and the scratch layout.  Exact integer
equality; no device is needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import place_ref as pr
import test_drain_host as tdh
import test_place_host as tph

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "gang_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(HERE, "native", "place_serial.h"), os.path.join(CSRC, "ks_carve.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(CSRC, "ks_query.h")]
PODREC = tdh.PODREC
RES = np.dtype([("first", np.int32), ("size", np.int32), ("outcome", np.int32), ("tried", np.int32), ("ok", np.int32),
                ("over_capacity", np.int32), ("not_found", np.int32), ("block_status", np.int32)])
MAX_SHAPES, MAX_PODS = 64, 1024
BLOCKED, ADMITTED, SKIPPED, NOT_TRIED = 0, 1, 2, -2


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostgang.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    p = C.c_void_p
    case = [C.c_int32, p, p, p, p, p, p, C.c_int32, p, p, p, p, C.c_int32, p, C.c_int32, p, p, C.c_int32]
    lb.ks_host_gang_brute.argtypes = case + [p, p, p]
    lb.ks_host_gang.argtypes = case + [C.c_int32, p, p, p, p, p]
    lb.ks_host_gang.restype = lb.ks_host_gang_brute.restype = C.c_int
    lb.ks_host_gang_segment.argtypes = [C.c_int64, p, p, C.c_int64, p, p, p, p]
    lb.ks_host_gang_segment.restype = C.c_int64
    lb.ks_host_gang_route.argtypes = [C.c_int64]
    lb.ks_host_gang_route.restype = C.c_int
    lb.ks_host_gang_limits.argtypes = [p]
    lb.ks_host_gang_carve.restype = C.c_int64
    return lb


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def limits():
    out = np.zeros(14, np.int32)
    host_lib().ks_host_gang_limits(_p(out))
    return out.tolist()


def test_limits_are_the_headers():
    from kubesim_amd import _lib
    from kubesim_amd.engine import GANG_DTYPE
    lim = limits()
    assert lim[0] == _lib.KS_PLACE_MAX_SHAPES == MAX_SHAPES and lim[4] == _lib.KS_PLACE_MAX_PODS == MAX_PODS
    assert lim[1] == lim[2] == _lib.KS_GANG_MAX_ROUND
    assert lim[3] == GANG_DTYPE.itemsize == RES.itemsize == 32 and GANG_DTYPE == RES and lim[13] == 16
    assert lim[7:10] == [_lib.KS_GANG_BLOCKED, _lib.KS_GANG_ADMITTED, _lib.KS_GANG_SKIPPED] == [BLOCKED, ADMITTED, SKIPPED]
    assert lim[10:13] == [_lib.KS_GANG_NOT_TRIED, _lib.KS_GANG_MAX_SHAPES, _lib.KS_GANG_MAX_GANGS]


def test_who_decides_a_gang():
    lb = host_lib()
    rnd, single = limits()[5:7]
    L = limits()[2]
    assert rnd != single and L == 32, "the cases below are the default list length's"
    want = {0: rnd, 1: rnd, L - 1: rnd, L: rnd, L + 1: single, 110: single, 65536: single}
    assert {k: lb.ks_host_gang_route(k) for k in want} == want


def test_scratch_layout():
    assert host_lib().ks_host_gang_carve() == 0


# ---- the rounds against the chain as written ---------------------------------------------------
def run(c, first, min_ok, strict=False, brute=False, mode=0):
    lb = host_lib()
    n, k, m = len(c["alloc"]), len(c["shape_of"]), len(first) - 1
    first, min_ok = np.ascontiguousarray(first, np.int32), np.ascontiguousarray(min_ok, np.int32)
    assert first[0] == 0 and first[-1] == k and len(min_ok) == m
    out = np.zeros(max(k, 1), tph.REC)
    res = np.zeros(m, RES)
    after = np.zeros((n, 4), np.int64)
    info, stats = np.zeros(2, np.int64), np.zeros(5, np.int64)
    args = [n, _p(c["alloc"]), _p(c["scale"]), _p(c["state"]), _p(c["taint"]), _p(c["label"]), _p(c["cfg"]),
            len(c["req"]), _p(c["req"]), _p(c["keymask"]), _p(c["tol"]), _p(c["sel"]), k, _p(c["shape_of"]), m, _p(first),
            _p(min_ok), int(strict)]
    if brute:
        rc = lb.ks_host_gang_brute(*args, _p(out), _p(res), _p(after))
    else:
        rc = lb.ks_host_gang(*args, mode, _p(out), _p(res), _p(after), _p(info), _p(stats))
    return rc, dict(out=out[:k], res=res, after=after, info=info, stats=stats)


def same(a, b):
    return bool((a["res"] == b["res"]).all() and (a["after"] == b["after"]).all() and (a["out"] == b["out"]).all())


def split(rng, c, big=0.12):
    """the case's k pods dealt to gangs of 0 to 119 pods with mixed min_ok"""
    k = len(c["shape_of"])
    sizes = []
    left = k
    while left > 0:
        u = rng.random()
        take = 0 if u < 0.1 else int(rng.integers(33, 120)) if u < 0.1 + big else int(rng.integers(1, 33))
        take = min(take, left)
        sizes.append(take)
        left -= take
    if rng.random() < 0.3:
        sizes.append(0)
    sizes = np.array(sizes, np.int64)
    u = rng.random(len(sizes))
    min_ok = np.where(u < 0.5, sizes, np.where(u < 0.6, 0, np.floor(sizes * rng.random(len(sizes))).astype(np.int64)))
    return np.concatenate([[0], np.cumsum(sizes)]), np.minimum(min_ok, sizes)


def test_fuzzed_chains_equal_the_chain_as_written():
    """test_place_host's fuzz recipe; its pods are dealt to gangs"""
    rng = np.random.default_rng(20261121)
    seen = dict(admitted=0, blocked=0, skipped=0, partial=0, late_block=0, stops=0, undone=0, single=0, single_blocked=0,
                rounds2=0, from_d=0, not_ok_kept=0, flags=0, counts=0, nchg=0, ok_only=0)
    statuses = set()
    for i in range(1200):
        c = tph.fuzz_case(rng)
        first, min_ok = split(rng, c)
        strict = rng.random() < 0.25
        rc, got = run(c, first, min_ok, strict)
        assert rc == 0, f"fuzz case {i}: the rounds stopped with {rc}"
        _, want = run(c, first, min_ok, strict, brute=True)
        np.testing.assert_array_equal(got["res"], want["res"], err_msg=f"fuzz case {i}")
        np.testing.assert_array_equal(got["after"], want["after"], err_msg=f"fuzz case {i}: after")
        np.testing.assert_array_equal(got["out"], want["out"], err_msg=f"fuzz case {i}: rows")
        r = want["res"]
        oc = r["outcome"]
        untried = np.concatenate([np.arange(a + t, a + s) for a, s, t in zip(r["first"], r["size"], r["tried"])] + [[]]).astype(int)
        assert (want["out"]["status"][untried] == NOT_TRIED).all() and (r["tried"][oc == SKIPPED] == 0).all()
        seen["admitted"] += int((oc == ADMITTED).sum())
        seen["blocked"] += int((oc == BLOCKED).sum())
        seen["skipped"] += int((oc == SKIPPED).sum())
        seen["partial"] += int(((oc == ADMITTED) & (r["ok"] < r["size"])).sum())
        seen["single_blocked"] += int(((oc == BLOCKED) & (r["size"] > 32)).sum())
        for key, j in (("late_block", 0), ("stops", 1), ("undone", 2), ("from_d", 3), ("not_ok_kept", 4)):
            seen[key] += int(got["stats"][j])
        seen["single"] += int(got["info"][1])
        seen["rounds2"] += int(got["info"][0] >= 2)
        statuses |= set(r["block_status"][oc == BLOCKED].tolist())
        if got["stats"][0] or got["stats"][1] or got["stats"][4]:
            # each part of the roll-back alone decides cases: without it the answer differs
            for mode, key in ((1, "flags"), (2, "counts"), (3, "nchg"), (4, "ok_only")):
                rcm, wrong = run(c, first, min_ok, strict, mode=mode)
                seen[key] += int(rcm != 0 or not same(wrong, want))
    assert seen["admitted"] >= 3000 and seen["blocked"] >= 1000 and seen["skipped"] >= 200 and seen["partial"] >= 100, seen
    assert seen["late_block"] >= 300 and seen["stops"] >= 20 and seen["undone"] >= 100, seen
    assert seen["single"] >= 100 and seen["single_blocked"] >= 20 and seen["rounds2"] >= 200 and seen["from_d"] >= 1000, seen
    assert seen["flags"] >= 50 and seen["counts"] >= 50 and seen["nchg"] >= 50 and seen["ok_only"] >= 20, seen
    assert statuses == {pr.OVER, pr.NOT_FOUND}


def test_a_blocked_gang_leaves_nothing_behind():
    """Nodes that take one pod each, a constant score: the first gang has three pods for two free
    nodes and is blocked on its third; rolled back, nodes 0 and 1 are free again and the next gang's
    pods go there: the blocked gang's flags, counts and slots are all undone."""
    c = tph.uniform(3, 5, tph.FEEDS_CONST, ap=1)
    c["state"][2, 3] = 1            # node 2 is full
    rc, got = run(c, [0, 3, 5], [3, 2])
    _, want = run(c, [0, 3, 5], [3, 2], brute=True)
    assert rc == 0 and same(got, want)
    assert got["res"]["outcome"].tolist() == [BLOCKED, ADMITTED] and got["res"]["tried"].tolist() == [3, 2]
    assert got["res"]["block_status"].tolist() == [pr.NOT_FOUND, 0]
    assert got["out"]["node"].tolist() == [0, 1, -1, 0, 1]
    assert got["after"][:, 3].tolist() == [1, 1, 1]
    for mode in (1, 2):
        rcm, wrong = run(c, [0, 3, 5], [3, 2], mode=mode)
        assert rcm != 0 or not same(wrong, want), mode
    # (here the slots the attempt appended are harmless if they stay: the next gang fills the same nodes.)  Nodes
    # with room for one more pod each and two gangs that are both blocked: slots that stayed would be committed
    d = tph.uniform(3, 6, tph.FEEDS_CONST, ap=2)
    d["state"][:, 3] = (1, 1, 2)
    rc, got = run(d, [0, 3, 6], [3, 3])
    _, want3 = run(d, [0, 3, 6], [3, 3], brute=True)
    assert rc == 0 and same(got, want3) and got["res"]["outcome"].tolist() == [BLOCKED, BLOCKED]
    assert got["after"][:, 3].tolist() == [1, 1, 2] and got["out"]["node"].tolist() == [0, 1, -1, 0, 1, -1]
    for mode in (1, 2, 3):
        rcm, wrong = run(d, [0, 3, 6], [3, 3], mode=mode)
        assert rcm != 0 or not same(wrong, want3), mode
    # two of three is enough: the gang stays with its failed pod, the next one finds no room and is blocked
    rc, got = run(c, [0, 3, 5], [2, 2])
    _, want = run(c, [0, 3, 5], [2, 2], brute=True)
    assert rc == 0 and same(got, want)
    assert got["res"]["outcome"].tolist() == [ADMITTED, BLOCKED] and got["res"]["tried"].tolist() == [3, 1]
    assert got["res"]["not_found"].tolist() == [1, 1] and got["out"]["status"].tolist() == [0, 0, -1, -1, NOT_TRIED]
    # strict: the rest of the queue is skipped
    rc, got = run(c, [0, 3, 4, 5], [3, 1, 1], strict=True)
    _, want = run(c, [0, 3, 4, 5], [3, 1, 1], strict=True, brute=True)
    assert rc == 0 and same(got, want) and got["res"]["outcome"].tolist() == [BLOCKED, SKIPPED, SKIPPED]
    assert got["after"][:, 3].tolist() == [0, 0, 1]


def test_only_pods_bound_ok_are_taken_back_out():
    """Literal mode, two nodes that take two pods each and a constant score: every pod goes to node 0.
    Gang 0 (one pod) stays; gang 1's first pod fills node 0, its second is bound OverCapacity there and
    blocks it: one pod, not two, leaves node 0's kept slot."""
    c = tph.uniform(2, 3, tph.LITERAL_CONST, ap=2)
    rc, got = run(c, [0, 1, 3], [1, 2])
    _, want = run(c, [0, 1, 3], [1, 2], brute=True)
    assert rc == 0 and same(got, want)
    assert got["res"]["outcome"].tolist() == [ADMITTED, BLOCKED] and got["res"]["block_status"].tolist() == [0, pr.OVER]
    assert got["out"]["node"].tolist() == [0, 0, 0] and got["after"][:, 3].tolist() == [1, 0] and got["stats"][4] == 1
    rcm, wrong = run(c, [0, 1, 3], [1, 2], mode=4)
    assert wrong["after"][:, 3].tolist() == [0, 0] and not same(wrong, want)


# ---- the round walk ------------------------------------------------------------------------------
def segment(counts, ids, start=0):
    counts, ids = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(ids, np.int64)
    assert counts.sum() == len(ids)
    ns, npods = np.zeros(1, np.int32), np.zeros(1, np.int32)
    shape_of = np.full(MAX_PODS + 64, -1, np.int32)
    shapes = np.zeros(MAX_SHAPES, PODREC)
    end = host_lib().ks_host_gang_segment(len(counts), _p(counts), _p(ids), start, _p(ns), _p(npods), _p(shape_of), _p(shapes))
    first = int(counts[:start].sum())
    seg = ids[first:first + int(npods[0])].tolist()
    order = list(dict.fromkeys(seg))
    assert len(order) == ns[0] and shape_of[:npods[0]].tolist() == [order.index(x) for x in seg]
    # (rows past the round's pods may be numbered: a gang that did not fit; never past a round's room)
    assert npods[0] == counts[start:end].sum() and (shape_of[MAX_PODS:] == -1).all()
    assert [int(r["req"][0]) for r in shapes[:ns[0]]] == [1000 + x for x in order] and (shapes["flags"] == 0).all()
    assert (shapes["req"][:ns[0], 1] == 0).all(), "an unmasked request is not part of the shape"
    return int(end), int(ns[0]), int(npods[0])


def test_round_boundaries():
    # the 65th shape: one pod per gang, every pod a shape of its own
    assert segment(np.ones(200, int), np.arange(200)) == (64, 64, 64)
    assert segment(np.ones(200, int), np.arange(200), start=64) == (128, 64, 64)
    assert segment(np.ones(200, int), np.arange(200), start=192) == (200, 8, 8)
    # 60 shapes, then a gang with 5 new ones: it moves whole to the next round; with 4 it stays
    ids = np.concatenate([np.arange(60), 100 + np.arange(5), [0]])
    assert segment([30, 30, 5, 1], ids) == (2, 60, 60) and segment([30, 30, 5, 1], ids, start=2) == (4, 6, 6)
    assert segment([30, 30, 4, 1], np.concatenate([np.arange(60), 100 + np.arange(4), [200]])) == (3, 64, 64)
    # the 1,025th pod: 32 gangs of 32 pods fill a round exactly; one pod more moves its gang
    assert segment([32] * 40, np.arange(32 * 40) % 5) == (32, 5, 1024)
    assert segment([32] * 31 + [31, 2, 3], np.arange(32 * 32 + 4) % 5) == (32, 5, 1023)
    assert segment([32] * 31 + [31, 1, 1], np.arange(32 * 32 + 1) % 5) == (33, 5, 1024)
    # empty gangs ride along, also at the end; a gang of the single path closes the round
    assert segment([0, 3, 0, 0, 2, 0], np.arange(5)) == (6, 5, 5)
    assert segment([0, 0, 0], []) == (3, 0, 0)
    assert segment([2, 32, 33, 1], np.arange(68) % 7) == (2, 7, 34)
    assert segment([2, 32, 33, 1], np.arange(68) % 7, start=2) == (2, 0, 0), "it heads no round: the single path"
    assert segment([2, 32, 33, 1], np.arange(68) % 7, start=3) == (4, 1, 1)


def test_stand_alone_program_runs_clean():
    """gang_host.cpp has a main: the scratch layout, a small chain against the chain as written, the
    route.  (Built once with -fsanitize=address,undefined on the host side and run as a program for the
    change that added it: no report.)"""
    exe = os.path.join(HERE, "native", "gang_host_main")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-DKS_GANG_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "DIFFERENT" not in r.stdout and r.stdout.count("equal") == 2, r.stdout + r.stderr
