"""The removal scan's host-side pieces of ks_query.h and ks_carve.h, compiled for the host
(tests/native/removable_host.cpp): a serial restatement of the per-candidate resolver — shared base
lists with no cordon, the candidate's own entries flagged from the start, its candidate counts
corrected — which must equal the plain sequential argmax over the other nodes; the split between the
batched resolver and the single-drain path; the candidate-aligned segment walk; and the scratch
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
SRC = os.path.join(HERE, "native", "removable_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "ks_carve.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(CSRC, "ks_query.h")]
PODREC = tdh.PODREC
MAX_SHAPES = 64


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostremovable.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    p = C.c_void_p
    case = [C.c_int32, p, p, p, p, p, p, C.c_int32, p, p, p, p, C.c_int32, p, C.c_int32]
    lb.ks_host_removable_brute.argtypes = case + [p, p]
    lb.ks_host_removable.argtypes = case + [C.c_int32, p, p, p]
    lb.ks_host_removable.restype = lb.ks_host_removable_brute.restype = C.c_int
    lb.ks_host_removable_segments.argtypes = [C.c_int64, p, p, p, p, p, p, C.c_int64, p, p, p, p]
    lb.ks_host_removable_segments.restype = C.c_int64
    lb.ks_host_group_rows.argtypes = [C.c_int32, p, C.c_int64, C.c_int64, p, p, p, p, p, p]
    lb.ks_host_group_rows.restype = C.c_int64
    lb.ks_host_removable_route.argtypes = [C.c_int64]
    lb.ks_host_removable_route.restype = C.c_int
    lb.ks_host_removable_limits.argtypes = [p]
    lb.ks_host_removable_carve.restype = C.c_int64
    return lb


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def limits():
    out = np.zeros(9, np.int32)
    host_lib().ks_host_removable_limits(_p(out))
    return out.tolist()


def test_limits_are_the_headers():
    from kubesim_amd import _lib
    from kubesim_amd.engine import REMOVAL_DTYPE
    lim = limits()
    assert lim[0] == _lib.KS_PLACE_MAX_SHAPES == MAX_SHAPES and lim[1] == lim[2] - 1 == _lib.KS_REMOVABLE_MAX_BATCHED
    assert lim[3] == REMOVAL_DTYPE.itemsize == 32 and lim[4] == 16
    # a closed segment holds more than 64 - 31 shapes, each on a row of its own
    assert lim[5] == 65536 // (64 - lim[1] + 1) + 1


def test_the_split_between_the_batched_resolver_and_the_single_drain_path():
    lb = host_lib()
    empty, batched, drain = limits()[6:9]
    assert len({empty, batched, drain}) == 3
    max_b = limits()[1]
    assert max_b == 31, "the cases below are the default list length's"
    want = {-1: empty, 0: empty, 1: batched, 2: batched, 30: batched, 31: batched, 32: drain, 33: drain, 110: drain, 65536: drain}
    assert {k: lb.ks_host_removable_route(k) for k in want} == want


def test_scratch_layout():
    assert host_lib().ks_host_removable_carve() == 0


# ---- the per-candidate resolver ---------------------------------------------------------------
def run(c, cand, brute=False, mode=0):
    lb = host_lib()
    n, k = len(c["alloc"]), len(c["shape_of"])
    out = np.zeros(k, tph.REC)
    info, stats = np.zeros(4, np.int64), np.zeros(3, np.int64)
    args = [n, _p(c["alloc"]), _p(c["scale"]), _p(c["state"]), _p(c["taint"]), _p(c["label"]), _p(c["cfg"]),
            len(c["req"]), _p(c["req"]), _p(c["keymask"]), _p(c["tol"]), _p(c["sel"]), k, _p(c["shape_of"]), cand]
    if brute:
        rc = lb.ks_host_removable_brute(*args, _p(out), _p(info))
    else:
        rc = lb.ks_host_removable(*args, mode, _p(out), _p(info), _p(stats))
    return rc, dict(node=out["node"], status=out["status"], score=out["score"], candidates=out["candidates"], info=info,
                    stats=stats)


def same(a, b):
    return all((a[f] == b[f]).all() for f in ("node", "status", "score", "candidates"))


def test_fuzzed_candidates_equal_the_argmax_over_the_other_nodes():
    """test_place_host's fuzz recipe, at most 31 pods, one candidate per case: half the time the node
    the first pod would have chosen with nothing removed — its own node heads its list."""
    rng = np.random.default_rng(20261022)
    max_b = limits()[1]
    seen = dict(own_in_list=0, own_first=0, from_d=0, flags_matter=0, counts_matter=0, full=0)
    statuses = set()
    n_cases = 1500
    for i in range(n_cases):
        c = tph.fuzz_case(rng)
        n = len(c["alloc"])
        k = int(rng.integers(1, max_b + 1)) if rng.random() < 0.7 else max_b
        c["shape_of"] = np.ascontiguousarray(c["shape_of"][:k])
        free = tph.run(c, True)
        cand = int(rng.integers(n))
        if rng.random() < 0.5 and free["node"][0] >= 0:
            cand = int(free["node"][0])
            seen["own_first"] += 1
        rc, got = run(c, cand)
        assert rc == 0, f"fuzz case {i}: the resolver stopped with {rc}"
        _, want = run(c, cand, brute=True)
        for f in ("node", "status", "score", "candidates"):
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"fuzz case {i}: {f}")
        assert got["info"].tolist() == want["info"].tolist()
        assert not (got["node"] == cand).any(), f"fuzz case {i}: the candidate itself was chosen"
        ff, _, has = (int(x) for x in c["cfg"][:3])
        if not ff and has:
            assert (got["candidates"] == n - 1).all()
        seen["own_in_list"] += int(got["stats"][2] > 0)
        seen["from_d"] += int(got["stats"][0])
        seen["full"] += int(len(c["shape_of"]) == max_b)
        statuses |= set(got["status"].tolist())
        # each correction alone decides cases: without it the answer differs
        rc1, no_flags = run(c, cand, mode=1)
        seen["flags_matter"] += int(rc1 != 0 or not same(no_flags, want))
        rc2, no_counts = run(c, cand, mode=2)
        seen["counts_matter"] += int(rc2 != 0 or not same(no_counts, want))
    assert seen["own_in_list"] >= 700 and seen["own_first"] >= 500 and seen["from_d"] >= 500 and seen["full"] >= 300, seen
    assert seen["flags_matter"] >= 400 and seen["counts_matter"] >= 500, seen
    assert statuses == {pr.OK, pr.OVER, pr.NOT_FOUND}


def test_thirty_one_pods_fill_the_flag_word_without_stopping():
    """40 equal nodes that take one pod each and a constant score: every list is nodes 0..31, the
    candidate (node 0) among them.  Its 31 pods take 31 distinct nodes: with its own entry that is all
    32 flags, and the 31st pod is still decided from the list.  A 32nd pod is not: the split."""
    L = limits()[2]
    for shapes in (1, 2):
        kw = {} if shapes == 1 else dict(req=[(1000, 4000, 0), (1100, 4000, 0)], keymask=[3, 3], tol=[0, 0], sel=[0, 0])
        k = L - 1
        c = tph.uniform(L + 8, k, tph.FEEDS_CONST, ap=1, shape_of=(np.arange(k) % shapes).astype(np.int32), **kw)
        rc, got = run(c, 0)
        assert rc == 0
        np.testing.assert_array_equal(got["node"], np.arange(1, L))
        assert (got["status"] == pr.OK).all() and got["stats"].tolist() == [0, L, shapes]
        np.testing.assert_array_equal(got["candidates"], L + 7 - np.arange(k))
        _, want = run(c, 0, brute=True)
        assert same(got, want)
        # one pod more meets a full list with every entry flagged and no changed node that takes it
        c = tph.uniform(L + 8, L, tph.FEEDS_CONST, ap=1, shape_of=(np.arange(L) % shapes).astype(np.int32), **kw)
        rc, _ = run(c, 0)
        assert rc == -1
        # ... unless the candidate is outside the list: then L pods are decided
        rc, got = run(c, L + 3)
        assert rc == 0 and got["node"].tolist() == list(range(L))


def test_own_node_first_and_a_changed_node_reused():
    """The candidate heads every list: the first pod takes the second entry.  Tiny requests leave the
    score as it is, so that node wins again from the changed set."""
    c = tph.uniform(40, 20, tph.FEEDS_LRBA, req=(1, 1, 0))
    rc, got = run(c, 0)
    assert rc == 0 and (got["node"] == 1).all() and got["stats"][0] == 19 and (got["candidates"] == 39).all()
    assert same(got, run(c, 0, brute=True)[1])
    rc, wrong = run(c, 0, mode=1)
    assert (wrong["node"] == 0).all(), "without its flags the candidate itself wins"


# ---- the candidate-aligned segment walk ----------------------------------------------------------
def segments(counts, ids, junk=None):
    counts, ids = np.asarray(counts, np.int32), np.asarray(ids, np.int64)
    n_cand, rows = len(counts), len(ids)
    assert counts.sum() == rows
    keymask = (1 + ids % 7).astype(np.uint32)
    req = np.stack([1000 + ids * 3, (ids // 7 + 1) << 20, ids % 5], axis=1).astype(np.int64)
    tol = ids.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    sel = (ids % 3).astype(np.uint64)
    flags = np.zeros(rows, np.uint32)
    if junk is not None:
        for col in range(3):
            off = ((keymask >> col) & 1) == 0
            req[off, col] = junk.integers(-5, 1 << 40, int(off.sum()))
        flags = junk.integers(0, 4, rows).astype(np.uint32)
    cap = n_cand + 1
    seg_end, seg_shapes = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
    shape_of = np.full(max(rows, 1), -1, np.int32)
    shapes = np.zeros((cap, MAX_SHAPES), PODREC)
    ns = host_lib().ks_host_removable_segments(n_cand, _p(counts), _p(req), _p(keymask), _p(tol), _p(sel), _p(flags), cap,
                                               _p(seg_end), _p(seg_shapes), _p(shape_of), _p(shapes))
    assert ns >= 0
    return seg_end[:ns], seg_shapes[:ns], shape_of[:rows], shapes[:ns], dict(req=req, keymask=keymask, tol=tol, sel=sel)


def check_segments(counts, ids, junk=None):
    counts, ids = np.asarray(counts, np.int64), np.asarray(ids, np.int64)
    seg_end, seg_shapes, shape_of, shapes, rec = segments(counts, ids, junk)
    first_row = np.concatenate([[0], np.cumsum(counts)])
    n_cand = len(counts)
    assert (len(seg_end) == 0) == (n_cand == 0)
    if n_cand == 0:
        return seg_end, seg_shapes
    # they tile the candidates: a candidate is never split
    assert seg_end[-1] == n_cand and (np.diff(np.concatenate([[0], seg_end])) >= 1).all()
    start = 0
    for s, end in enumerate(seg_end.tolist()):
        r0, r1 = int(first_row[start]), int(first_row[end])
        seg = ids[r0:r1]
        first, order = {}, []
        for x in seg.tolist():
            if x not in first:
                first[x] = len(order)
                order.append(x)
        assert len(order) == seg_shapes[s] <= MAX_SHAPES
        assert shape_of[r0:r1].tolist() == [first[x] for x in seg.tolist()]
        for j, x in enumerate(order):
            q = r0 + int(np.nonzero(seg == x)[0][0])
            km = int(rec["keymask"][q])
            row = shapes[s][j]
            assert row["keymask"] == km and row["tol"] == rec["tol"][q] and row["sel"] == rec["sel"][q] and row["flags"] == 0
            assert row["req"].tolist() == [int(rec["req"][q][col]) if (km >> col) & 1 else 0 for col in range(3)]
        # maximal: it closed before the candidate that would have brought its 65th shape
        if end < n_cand:
            nxt = set(ids[int(first_row[end]):int(first_row[end + 1])].tolist())
            assert len(set(order) | nxt) > MAX_SHAPES, (s, len(order), len(nxt))
        start = end
    return seg_end, seg_shapes


def test_segment_boundaries_at_the_sixty_fifth_shape():
    # one pod per candidate, every pod a shape of its own: the 65th shape is the 65th candidate
    e, m = check_segments(np.ones(200, int), np.arange(200))
    assert e.tolist() == [64, 128, 192, 200] and m.tolist() == [64, 64, 64, 8]
    # exactly 64 shapes never close a segment
    e, m = check_segments(np.ones(640, int), np.arange(640) % 64)
    assert e.tolist() == [640] and m.tolist() == [64]
    # 60 shapes, then a candidate with 5 new ones: it moves whole to the next segment although four
    # of its shapes would still fit, and the rows it had been given are numbered again there
    e, m = check_segments([30, 30, 5, 1], np.concatenate([np.arange(60), 100 + np.arange(5), [0]]))
    assert e.tolist() == [2, 4] and m.tolist() == [60, 6]
    # ... with 4 new ones it stays (64 exactly); the next new shape closes
    e, m = check_segments([30, 30, 4, 1], np.concatenate([np.arange(60), 100 + np.arange(4), [200]]))
    assert e.tolist() == [3, 4] and m.tolist() == [64, 1]
    # a candidate of 31 pods of 31 shapes always fits an empty segment; three of them do not fit one
    e, m = check_segments([31, 31, 31], np.arange(93))
    assert e.tolist() == [2, 3] and m.tolist() == [62, 31]
    # shapes shared between candidates are counted once
    e, m = check_segments([31] * 10, np.tile(np.arange(31), 10))
    assert e.tolist() == [10] and m.tolist() == [31]
    check_segments([], [])
    check_segments([1], [7])


# ---- the gather's rows grouped by candidate ------------------------------------------------------
def group_rows(nodes, n, frm):
    nodes, frm = np.asarray(nodes, np.int32), np.asarray(frm, np.int32)
    m, n_ev = len(nodes), len(frm)
    ids = (1000 + 7 * np.arange(n_ev)).astype(np.int64)
    evicted, first_row = np.full(m, -9, np.int32), np.full(m, -9, np.int64)
    perm, rec_ids = np.full(max(n_ev, 1), -9, np.int32), np.full(max(n_ev, 1), -9, np.int64)
    bad = host_lib().ks_host_group_rows(m, _p(nodes), n, n_ev, _p(frm), _p(ids), _p(evicted), _p(first_row), _p(perm), _p(rec_ids))
    return bad, evicted, first_row, perm[:n_ev], rec_ids[:n_ev], ids


def check_group_rows(nodes, n, frm):
    """the expected grouping in numpy: a stable sort of the rows on their candidate's position"""
    nodes, frm = np.asarray(nodes, np.int64), np.asarray(frm, np.int64)
    m = len(nodes)
    pos = np.full(n, -1, np.int64)
    pos[nodes] = np.arange(m)
    assert (pos[frm] >= 0).all()
    want_perm = np.argsort(pos[frm], kind="stable")
    want_evicted = np.bincount(pos[frm], minlength=m)
    want_first = np.cumsum(want_evicted) - want_evicted  # the exclusive prefix sum
    bad, evicted, first_row, perm, rec_ids, ids = group_rows(nodes, n, frm)
    assert bad == -1
    assert evicted.tolist() == want_evicted.tolist() and first_row.tolist() == want_first.tolist()
    assert perm.tolist() == want_perm.tolist() and rec_ids.tolist() == ids[want_perm].tolist()
    return evicted.tolist(), first_row.tolist(), perm.tolist()


def test_group_rows_is_a_stable_sort_on_the_candidates_position():
    # one candidate: the rows as gathered
    assert check_group_rows([5], 9, [5, 5, 5]) == ([3], [0], [0, 1, 2])
    assert check_group_rows([0], 1, [0]) == ([1], [0], [0])
    # candidates with no row at the front, in the middle and at the end: empty ranges at the next row
    ev, first, _ = check_group_rows([7, 2, 4, 9, 0], 10, [2, 9, 2, 9, 9])
    assert ev == [0, 2, 0, 3, 0] and first == [0, 0, 2, 2, 5]
    # the candidates in the reverse of node order: the rows follow the caller's order, not the nodes'
    ev, first, perm = check_group_rows([8, 6, 3, 1], 9, [1, 3, 3, 6, 8, 8])
    assert ev == [2, 1, 2, 1] and first == [0, 2, 3, 5] and perm == [4, 5, 3, 1, 2, 0]
    # two candidates whose rows interleave: FIFO within each
    ev, first, perm = check_group_rows([4, 1], 5, [1, 4, 1, 4, 4, 1])
    assert ev == [3, 3] and first == [0, 3] and perm == [1, 3, 4, 0, 2, 5]
    # no row at all
    assert check_group_rows([3, 0], 4, []) == ([0, 0], [0, 0], [])
    # every node a candidate, rows in a fixed shuffle
    rng = np.random.default_rng(20261021)
    check_group_rows(rng.permutation(300), 300, rng.integers(300, size=5000))
    # a row on no candidate: the first such row's index
    assert group_rows([2, 5], 8, [2, 5, 3, 5])[0] == 2      # a node that is no candidate
    assert group_rows([2, 5], 8, [2, 5, 5, 4, 3])[0] == 3   # ... the first of two
    assert group_rows([2, 5], 8, [-1, 5])[0] == 0           # below the node range
    assert group_rows([2, 5], 8, [2, 5, 2, 8])[0] == 3      # node n itself
    assert group_rows([0], 1, [1])[0] == 0


def test_fuzzed_candidate_sequences_tile_at_candidate_boundaries():
    rng = np.random.default_rng(20261023)
    max_b = limits()[1]
    closed, exact = 0, 0
    for i in range(300):
        n_cand = int(rng.integers(1, 400))
        counts = rng.integers(1, max_b + 1, n_cand) if i % 3 else rng.integers(1, 4, n_cand)
        rows = int(counts.sum())
        pool = int(rng.choice([3, 40, 64, 65, 70, 200, 5000]))
        ids = rng.integers(pool, size=rows) if i % 2 else (np.arange(rows) // int(rng.integers(1, 9))) % pool
        e, m = check_segments(counts, ids, junk=rng)
        closed += len(e) - 1
        exact += int((m[:-1] == MAX_SHAPES).sum())
    assert closed >= 500 and exact >= 20, (closed, exact)
