"""The drain preview's host-side pieces of ks_query.h, compiled for the host
(tests/native/drain_host.cpp): the segment walk (drain_segment), the gather's rank arithmetic
(drain_rank over wave ballots, block counts and the chunked scan, restated serially) and the rounds
algorithm with the cordon in its scan, which must equal the plain sequential argmax over the nodes
that remain.  Exact integer equality; no device is needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import place_ref as pr
import test_place_host as tph

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "drain_host.cpp")
DEV_H = [os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc", h) for h in ("ks_device.h", "ks_query.h")]
PODREC = np.dtype([("req", np.int64, 3), ("tol", np.uint64), ("sel", np.uint64), ("keymask", np.uint32), ("flags", np.uint32)])
MAX_SHAPES, MAX_PODS = 64, 1024


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostdrain.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in [SRC, *DEV_H]):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    p = C.c_void_p
    case = [C.c_int32, p, p, p, p, p, p, C.c_int32, p, p, p, p, C.c_int32, p, p]
    lb.ks_host_drain_place.argtypes = lb.ks_host_drain_place_brute.argtypes = case + [p, p, p]
    lb.ks_host_drain_place.restype = lb.ks_host_drain_place_brute.restype = C.c_int
    lb.ks_host_drain_segments.argtypes = [C.c_int64, p, p, p, p, p, C.c_int64, p, p, p, p]
    lb.ks_host_drain_segments.restype = C.c_int64
    lb.ks_host_drain_ranks.argtypes = [C.c_int64, p, p]
    lb.ks_host_drain_ranks.restype = C.c_int64
    lb.ks_host_drain_limits.argtypes = [p]
    return lb


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_limits_are_the_headers():
    from kubesim_amd import _lib
    out = np.zeros(6, np.int32)
    host_lib().ks_host_drain_limits(_p(out))
    assert out.tolist()[:3] == [MAX_SHAPES, MAX_PODS, 256] and out[4] == 40
    assert (out[0], out[1], out[5]) == (_lib.KS_PLACE_MAX_SHAPES, _lib.KS_PLACE_MAX_PODS, _lib.KS_DRAIN_MAX_PODS)
    assert PODREC.itemsize == 48


# ---- segments --------------------------------------------------------------------------------
def segments(shape_ids, junk=None):
    """The walk over pods whose shape is shape_ids[i] (a distinct record per id).  Returns
    (seg_end, seg_shapes, shape_of, shapes [segments][64])."""
    ids = np.asarray(shape_ids, np.int64)
    n = len(ids)
    keymask = (1 + ids % 7).astype(np.uint32)                 # 1..7: every mask
    req = np.stack([1000 + ids * 3, (ids // 7 + 1) << 20, ids % 5], axis=1).astype(np.int64)
    tol = ids.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)      # mod 2^64, odd factor: distinct per id
    sel = (ids % 3).astype(np.uint64)
    flags = np.zeros(n, np.uint32)
    if junk is not None:
        # what a shape ignores: the words of unmasked keys and the flags
        for c in range(3):
            off = ((keymask >> c) & 1) == 0
            req[off, c] = junk.integers(-5, 1 << 40, int(off.sum()))
        flags = junk.integers(0, 4, n).astype(np.uint32)
    cap = n + 1
    seg_end, seg_shapes = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    shape_of = np.full(max(n, 1), -1, np.int32)
    shapes = np.zeros((cap, MAX_SHAPES), PODREC)
    ns = host_lib().ks_host_drain_segments(n, _p(req), _p(keymask), _p(tol), _p(sel), _p(flags), cap, _p(seg_end),
                                           _p(seg_shapes), _p(shape_of), _p(shapes))
    assert ns >= 0
    return seg_end[:ns], seg_shapes[:ns], shape_of[:n], shapes[:ns], dict(req=req, keymask=keymask, tol=tol, sel=sel)


def check_segments(ids, junk=None):
    ids = np.asarray(ids, np.int64)
    n = len(ids)
    seg_end, seg_shapes, shape_of, shapes, rec = segments(ids, junk)
    # they tile the pods
    assert (len(seg_end) == 0) == (n == 0)
    if n == 0:
        return seg_end, seg_shapes
    assert seg_end[-1] == n and (np.diff(np.concatenate([[0], seg_end])) >= 1).all()
    start = 0
    for s, end in enumerate(seg_end.tolist()):
        seg = ids[start:end]
        first, order = {}, []
        for x in seg.tolist():
            if x not in first:
                first[x] = len(order)
                order.append(x)
        # limits, shape numbering by first appearance, and the shape table's rows
        assert 1 <= len(seg) <= MAX_PODS and len(order) == seg_shapes[s] <= MAX_SHAPES
        assert shape_of[start:end].tolist() == [first[x] for x in seg.tolist()]
        for j, x in enumerate(order):
            q = start + int(np.nonzero(seg == x)[0][0])
            km = int(rec["keymask"][q])
            row = shapes[s][j]
            assert row["keymask"] == km and row["tol"] == rec["tol"][q] and row["sel"] == rec["sel"][q] and row["flags"] == 0
            assert row["req"].tolist() == [int(rec["req"][q][c]) if (km >> c) & 1 else 0 for c in range(3)]
        # maximal: it closed before the pod that would be its 65th shape or its 1,025th pod
        if end < n:
            assert len(seg) == MAX_PODS or (len(order) == MAX_SHAPES and int(ids[end]) not in first), (s, len(seg), len(order))
        start = end
    return seg_end, seg_shapes


def test_segment_boundaries():
    # every pod a distinct shape: the 65th distinct shape is the 65th pod
    e, m = check_segments(np.arange(379))
    assert e.tolist() == [64, 128, 192, 256, 320, 379] and m.tolist() == [64] * 5 + [59]
    # exactly 64 shapes never close a segment; the 65th does, wherever it comes
    e, m = check_segments(np.arange(640) % 64)
    assert e.tolist() == [640] and m.tolist() == [64]
    e, m = check_segments(np.concatenate([np.arange(500) % 64, [64], np.arange(100) % 64]))
    # (the second segment opens with shape 64 and takes 0..62 beside it: shape 63 is its 65th)
    assert e.tolist() == [500, 564, 601] and m.tolist() == [64, 64, 37]
    # one shape: the 1,025th pod closes the segment
    e, m = check_segments(np.zeros(1024, np.int64))
    assert e.tolist() == [1024]
    e, m = check_segments(np.zeros(1025, np.int64))
    assert e.tolist() == [1024, 1025] and m.tolist() == [1, 1]
    e, m = check_segments(np.arange(3000) % 5)
    assert e.tolist() == [1024, 2048, 3000]
    # both limits at the same pod: 1,024 pods of 64 shapes, then a new shape
    e, m = check_segments(np.concatenate([np.arange(1024) % 64, [99]]))
    assert e.tolist() == [1024, 1025]
    check_segments([])
    check_segments([7])


def test_fuzzed_shape_sequences_tile_within_the_limits():
    rng = np.random.default_rng(20261020)
    closed_by = {"shapes": 0, "pods": 0}
    for i in range(300):
        n = int(rng.integers(1, 5000)) if i % 4 else int(rng.integers(1, 200))
        pool = int(rng.choice([1, 3, 40, 64, 65, 70, 200, 5000]))
        how = rng.integers(3)
        if how == 0:
            ids = rng.integers(pool, size=n)
        elif how == 1:
            ids = np.arange(n) % pool
        else:
            ids = (np.arange(n) // int(rng.integers(1, 40))) % pool     # runs
        e, m = check_segments(ids, junk=rng)
        lens = np.diff(np.concatenate([[0], e]))
        closed_by["pods"] += int((lens[:-1] == MAX_PODS).sum())
        closed_by["shapes"] += int((lens[:-1] < MAX_PODS).sum())
    assert closed_by["pods"] >= 50 and closed_by["shapes"] >= 500, closed_by


# ---- the gather's ranks ------------------------------------------------------------------------
def check_ranks(sel):
    sel = np.ascontiguousarray(sel, np.uint8)
    assert len(sel) % 256 == 0
    rank = np.full(len(sel), -7, np.int64)
    total = host_lib().ks_host_drain_ranks(len(sel) // 256, _p(sel), _p(rank))
    want = np.where(sel != 0, np.cumsum(sel != 0) - 1, -1)       # a plain filter: the order of the pods
    np.testing.assert_array_equal(rank, want)
    assert total == int((sel != 0).sum())


def _block(count, rng, how):
    b = np.zeros(256, np.uint8)
    if how == "low":
        b[:count] = 1
    elif how == "high":
        b[256 - count:] = 1
    else:
        b[rng.choice(256, count, replace=False)] = 1
    return b


def test_gather_ranks_equal_a_plain_filter():
    rng = np.random.default_rng(4242)
    counts = [0, 1, 63, 64, 65, 255, 256, 257]     # per block; 257 = a full block and one pod of the next
    for how in ("low", "high", "random"):
        blocks = []
        for c in counts:
            blocks.append(_block(min(c, 256), rng, how))
            if c > 256:
                blocks.append(_block(c - 256, rng, how))
            blocks += [np.zeros(256, np.uint8)] * int(rng.integers(0, 3))     # empty blocks in between
        check_ranks(np.concatenate(blocks))
    check_ranks(np.zeros(0, np.uint8))
    check_ranks(np.zeros(256 * 5, np.uint8))
    check_ranks(np.ones(256 * 3, np.uint8))
    # one selected pod in each lane position of each wave
    for pos in (0, 63, 64, 127, 128, 191, 192, 255):
        b = np.zeros(256 * 2, np.uint8)
        b[pos] = b[256 + pos] = 1
        check_ranks(b)
    # more blocks than one chunk of the scan: 256 and 257 blocks, and a 1M-pod run's 4,096
    for nb in (255, 256, 257, 513, 4096):
        check_ranks(rng.random(nb * 256) < rng.choice([0.01, 0.3, 0.9]))


# ---- the cordoned rounds -------------------------------------------------------------------------
def run(c, cordon_nodes, brute):
    lb = host_lib()
    n, k = len(c["alloc"]), len(c["shape_of"])
    bits = np.zeros((n + 31) // 32 + 1, np.uint32)
    for nd in cordon_nodes:
        bits[nd >> 5] |= np.uint32(1 << (nd & 31))
    out = np.zeros(k, tph.REC)
    after = np.zeros((n, 4), np.int64)
    info = np.zeros(4, np.int64)
    args = [n, _p(c["alloc"]), _p(c["scale"]), _p(c["state"]), _p(c["taint"]), _p(c["label"]), _p(c["cfg"]),
            len(c["req"]), _p(c["req"]), _p(c["keymask"]), _p(c["tol"]), _p(c["sel"]), k, _p(c["shape_of"]), _p(bits)]
    rc = (lb.ks_host_drain_place_brute if brute else lb.ks_host_drain_place)(*args, _p(out), _p(after), _p(info))
    assert rc == 0, f"the driver stopped with {rc}"
    return dict(node=out["node"], status=out["status"], score=out["score"], candidates=out["candidates"], after=after,
                info=info)


def fuzz_cordon(rng, n):
    u = rng.random()
    if u < 0.1:
        return list(range(n))                                     # everything
    if u < 0.2:
        return [int(rng.integers(n))]
    frac = rng.choice([0.05, 0.33, 0.66, 0.95])
    return np.nonzero(rng.random(n) < frac)[0].tolist()


def test_cordoned_rounds_equal_the_argmax_over_the_remaining_nodes():
    rng = np.random.default_rng(20261021)
    rounds, statuses, hit = [], set(), 0
    for i in range(1200):
        c = tph.fuzz_case(rng)
        n = len(c["alloc"])
        cordon = fuzz_cordon(rng, n)
        got, want = run(c, cordon, False), run(c, cordon, True)
        pr.assert_same(got, want, f"fuzz case {i}")
        placed = got["node"][got["node"] >= 0]
        assert not np.isin(placed, cordon).any(), f"fuzz case {i}: a cordoned node was chosen"
        assert not got["after"][cordon].any()
        ff, _, has = (int(x) for x in c["cfg"][:3])
        if not ff and has:
            assert (got["candidates"] == n - len(cordon)).all()
        # the cordon matters: the unrestricted argmax would have used a cordoned node
        free = tph.run(c, True)
        hit += int(np.isin(free["node"][free["node"] >= 0], cordon).any())
        rounds.append(int(got["info"][0]))
        statuses |= set(got["status"].tolist())
    rounds = np.array(rounds)
    assert hit >= 600 and (rounds >= 2).mean() >= 0.05 and statuses == {pr.OK, pr.OVER, pr.NOT_FOUND}, (hit, rounds.mean())


def test_cordon_edges():
    # ties across block boundaries with every other node cordoned: the lowest remaining index wins
    c = tph.uniform(600, 600, tph.FEEDS_CONST, ap=2)
    cordon = list(range(0, 600, 2))
    got = run(c, cordon, False)
    pr.assert_same(got, run(c, cordon, True))
    np.testing.assert_array_equal(got["node"], 1 + 2 * (np.arange(600) // 2))
    np.testing.assert_array_equal(got["candidates"], 300 - np.arange(600) // 2)
    # a whole 256-node block cordoned, and the bitmap's word edges
    for cordon in (list(range(256, 512)), [0, 31, 32, 255, 256, 511, 512, 599], list(range(599))):
        got = run(c, cordon, False)
        pr.assert_same(got, run(c, cordon, True), str(cordon[:3]))
        assert not np.isin(got["node"], cordon).any()
    # all nodes cordoned: nothing is a candidate, one round
    got = run(c, list(range(600)), False)
    assert (got["status"] == pr.NOT_FOUND).all() and (got["candidates"] == 0).all() and got["info"][0] == 1
    assert not got["after"].any()
