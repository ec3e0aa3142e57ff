"""The scale-up preview's helpers of ks_query.h (scaleup_fresh_key, scaleup_count_start,
scaleup_takes_fresh, scaleup_template, scaleup_whole_units) compiled for the host
(tests/native/scaleup_host.cpp).  A serial restatement of scaleup_resolve_kernel's pod loop — shared
snapshot lists over the real nodes, the fresh appended node standing for every unchanged one, no
commit — must equal the plain sequential argmax over the extended cluster on every field, on
tests/test_place_host.py's fuzz recipe; where it stops (a snapshot list used up) the pods before the
stop must.  Exact integer equality; no device is needed."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import place_ref as pr
import scaleup_ref as sr
import test_place_host as tph

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "scaleup_host.cpp")
CSRC = os.path.join(HERE, "..", "kubernetes-simulator_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "ks_carve.h"), os.path.join(CSRC, "ks_device.h"),
        os.path.join(CSRC, "ks_query.h")]
REC = tph.REC
RES = ("ok", "over_capacity", "not_found", "on_new", "nodes_used", "first_unplaced", "path", "pad")
N_FUZZ = 1500


@functools.lru_cache(maxsize=None)
def host_lib():
    lib = os.path.join(HERE, "native", "libks_hostscaleup.so")
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(f) for f in DEPS):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", lib, SRC], check=True)
    lb = C.CDLL(lib)
    p = C.c_void_p
    case = [C.c_int32, p, p, p, p, p, p, C.c_int32, p, p, p, p, C.c_int32, p, p]
    lb.ks_host_scaleup_brute.argtypes = case + [p]
    lb.ks_host_scaleup.argtypes = case + [C.c_int32, p, p, p]
    lb.ks_host_scaleup_whole.argtypes = [C.c_int32, p, p, C.c_int32, p, p]
    lb.ks_host_scaleup_template.argtypes = [p, C.c_uint64, C.c_uint64, p, p]
    lb.ks_host_scaleup_carve.restype = C.c_int64
    return lb


_p = tph._p


def template(alloc_m, max_nodes, taint=0, label=0):
    """tmpl[7] of the driver: alloc[4] in milli-units, taint, label, max_nodes"""
    return np.array([*alloc_m, taint, label, max_nodes], np.int64)


def _args(c, tmpl):
    return [len(c["alloc"]), _p(c["alloc"]), _p(c["scale"]), _p(c["state"]), _p(c["taint"]), _p(c["label"]), _p(c["cfg"]),
            len(c["req"]), _p(c["req"]), _p(c["keymask"]), _p(c["tol"]), _p(c["sel"]), len(c["shape_of"]), _p(c["shape_of"]),
            _p(tmpl)]


def brute(c, tmpl):
    out = np.zeros(len(c["shape_of"]), REC)
    assert host_lib().ks_host_scaleup_brute(*_args(c, tmpl), _p(out)) == 0
    return out


def resolve(c, tmpl, ablate=0):
    """(rows, pods decided, summary dict, stats)"""
    k = len(c["shape_of"])
    out = np.zeros(k, REC)
    res = np.zeros(8, np.int32)
    stats = np.zeros(4, np.int64)
    done = host_lib().ks_host_scaleup(*_args(c, tmpl), ablate, _p(out), _p(res), _p(stats))
    assert 0 <= done <= k, f"the driver stopped with {done}"
    return out, done, dict(zip(RES, res.tolist())), stats


def summary_of(rows, n):
    return sr.summarize(dict(status=rows["status"], node=rows["node"]), n)


def check(c, tmpl, what=""):
    """the resolver against the brute force; returns (rows, decided, summary, stats)"""
    want = brute(c, tmpl)
    got, done, res, stats = resolve(c, tmpl)
    k, n = len(want), len(c["alloc"])
    for f in REC.names:
        np.testing.assert_array_equal(got[f][:done], want[f][:done], err_msg=f"{what}: {f}")
    if done == k:
        assert res["path"] == 0 and {f: res[f] for f in sr.SUMMARY} == summary_of(want, n), what
    else:
        assert res["path"] == -1, what
    return got, done, res, stats


def fuzz_template(rng, c):
    """A template for a tests/test_place_host.py fuzz case: often one of the cluster's own node
    sizes (equal scores: ties with real nodes), sometimes larger, tiny, tainted or without a key."""
    n = len(c["alloc"])
    sc = c["scale"]
    row = c["alloc"][int(rng.integers(n))]
    alloc = [int(row[i]) * int(sc[i]) if row[i] >= 0 else -1 for i in range(3)] + [int(row[3])]
    u = rng.random()
    if u < 0.2:
        alloc = [a * 2 if a > 0 and a < (1 << 57) else a for a in alloc[:3]] + [110]
    elif u < 0.3:
        alloc = [max(a // 8, 1) if a > 0 else a for a in alloc[:3]] + [int(rng.choice([1, 2, 110]))]
    elif u < 0.4:
        alloc[int(rng.integers(3))] = -1
    if rng.random() < 0.3:
        alloc = [a + int(rng.integers(1, 3)) if a > 0 and a < (1 << 58) else a for a in alloc[:3]] + alloc[3:]   # off the unit
    taint = int(rng.integers(1, 8)) if rng.random() < 0.2 else 0
    label = int(rng.integers(0, 16)) if rng.random() < 0.7 else 0
    m = int(rng.choice([0, 1, 2, 3, 7, 40, 300, 5000]))
    return template(alloc, m, taint, label)


def test_fuzzed_clusters_resolver_equals_the_argmax_over_the_extended_cluster():
    rng = np.random.default_rng(20261020)
    sizes, stops, full = [], 0, 0
    fresh = changed = ran_out = tied = ineligible = 0
    for i in range(N_FUZZ):
        c = tph.fuzz_case(rng)
        tmpl = fuzz_template(rng, c)
        if i % 300 == 299:
            tmpl[6] = 65536        # KS_SCALEUP_MAX_NODES
        n, m = len(c["alloc"]), int(tmpl[6])
        got, done, res, stats = check(c, tmpl, f"fuzz case {i}")
        sizes.append(n)
        stops += done < len(got)
        full += done == len(got)
        fresh += int(stats[0])
        changed += int(stats[1])
        g = got[:done]
        on = g["node"][g["node"] >= n]
        ran_out += m > 0 and len(set(on.tolist())) == m and (g["node"][-1:] < n).any()
        ineligible += m > 0 and len(on) == 0 and (g["status"] == pr.OK).any()
        # a real node that wins at a score an appended node wins at too: the tie went to the lower index
        real_scores = set(g["score"][(g["node"] >= 0) & (g["node"] < n)].tolist())
        tied += bool(real_scores & set(g["score"][g["node"] >= n].tolist()))
        if i < 100 and n <= 120 and m <= 40:      # ... and against the Python integers on the concatenated arrays
            alloc = c["alloc"].astype(object)
            for col in range(3):
                alloc[:, col] = [int(a) * int(c["scale"][col]) if a >= 0 else -1 for a in c["alloc"][:, col]]
            ff, fl, has, w_lr, w_ba, const = (int(x) for x in c["cfg"])
            scorers = ((0, 1, const),) + (((1, w_lr, 0),) if w_lr else ()) + (((2, w_ba, 0),) if w_ba else ()) if has else ()
            cfg = dict(filter_mode=ff, filters=fl, scorers=scorers, taint=c["taint"], label=c["label"])
            shapes = dict(req=c["req"], keymask=c["keymask"], tol=c["tol"], sel=c["sel"])
            want = sr.scale_up_one(np.array(alloc.tolist(), np.int64), c["state"], cfg, shapes, c["shape_of"],
                                   sr.option(tmpl[:4], m, tmpl[4], tmpl[5]))
            for f in sr.ROWS:
                np.testing.assert_array_equal(got[f][:done], want[f][:done], err_msg=f"fuzz case {i} against Python: {f}")
    assert min(sizes) == 1 and max(sizes) >= 650
    assert full >= N_FUZZ // 2 and stops >= 20, (full, stops)
    assert fresh > 2000 and changed > 2000, (fresh, changed)
    assert ran_out >= 20 and tied >= 20 and ineligible >= 20, (ran_out, tied, ineligible)


# ---- edges -----------------------------------------------------------------------------------
FEEDS_CONST, FEEDS_LRBA, LITERAL_CONST = tph.FEEDS_CONST, tph.FEEDS_LRBA, tph.LITERAL_CONST
NODE = [16000, 64000, 8000, 110]     # tph.uniform's node


def test_template_that_wins_ties_is_ineligible_and_runs_out():
    L = host_lib().ks_host_scaleup_l()
    # LeastRequested + BalancedAllocation on half-full equal nodes: the empty template scores higher
    c = tph.uniform(20, 12, FEEDS_LRBA, ap=110)
    c["state"][:, 0], c["state"][:, 1], c["state"][:, 3] = 8000, 32000, 1
    got, done, res, stats = check(c, template(NODE, 3))
    assert done == 12 and res["on_new"] >= 3 and res["nodes_used"] == 3 and got["node"][0] == 20
    assert (got["candidates"] == 23).all()
    # a constant score: every key ties, node 0 wins and never an appended node
    got, done, res, _ = check(tph.uniform(20, 12, FEEDS_CONST), template(NODE, 5))
    assert done == 12 and (got["node"] == 0).all() and res["on_new"] == 0 and (got["candidates"] == 25).all()
    # the same with one pod per node: the real nodes fill first, in index order, then the appended ones
    got, done, res, stats = check(tph.uniform(5, 12, FEEDS_CONST, ap=1), template(NODE[:3] + [1], 4))
    assert done == 12 and got["node"].tolist() == list(range(9)) + [-1] * 3
    assert got["candidates"].tolist() == list(range(9, 0, -1)) + [0] * 3
    assert (res["ok"], res["not_found"], res["on_new"], res["nodes_used"], res["first_unplaced"]) == (9, 3, 4, 4, 9)
    assert stats[0] == 4
    # a tainted template nobody tolerates, and one without the key the pods ask for: as if not there
    plain = check(tph.uniform(5, 12, FEEDS_CONST, ap=1), template(NODE, 0))[0]
    for tmpl in (template(NODE, 7, taint=1), template([-1] + NODE[1:], 7)):
        got, done, res, _ = check(tph.uniform(5, 12, FEEDS_CONST, ap=1), tmpl)
        assert done == 12 and res["on_new"] == 0
        for f in REC.names:
            np.testing.assert_array_equal(got[f], plain[f])
    # literal mode: the filters gate nothing, so the tainted nodes count and an overfull one repeats
    got, done, res, _ = check(tph.uniform(3, 8, LITERAL_CONST, ap=1), template(NODE[:3] + [1], 2, taint=1))
    assert done == 8 and (got["candidates"] == 5).all() and (got["node"] == 0).all() and res["over_capacity"] == 7
    # two small appended nodes that fill up: pods come back to them through D, then go to real nodes
    c = tph.uniform(4, 10, FEEDS_LRBA, ap=110)
    c["state"][:, 0], c["state"][:, 1], c["state"][:, 3] = 8000, 32000, 1
    # (LeastRequested of the 1000 / 4000 pod: 7 on an empty 4000 / 16000 node, 5 on it with one pod, 4 on
    # a half-full real node; two pods fill the appended node's pods capacity)
    got, done, res, stats = check(c, template([4000, 16000, 8000, 2], 2))
    assert done == 10 and res["on_new"] == 4 and res["nodes_used"] == 2 and stats[0] == 2 and stats[1] >= 2
    assert got["node"][:4].tolist() == [4, 5, 4, 5] and (got["node"][4:] < 4).all()
    assert L >= 8


def test_without_the_fresh_key_or_the_count_start_the_answers_differ():
    c = tph.uniform(20, 12, FEEDS_LRBA, ap=110)
    c["state"][:, 0], c["state"][:, 1], c["state"][:, 3] = 8000, 32000, 1
    tmpl = template(NODE, 3)
    want = brute(c, tmpl)
    got = resolve(c, tmpl)[0]
    no_key = resolve(c, tmpl, ablate=1)[0]
    no_count = resolve(c, tmpl, ablate=2)[0]
    for f in REC.names:
        np.testing.assert_array_equal(got[f], want[f])
    assert (no_key["node"] != want["node"]).any() and (no_key["node"] < 20).all()
    np.testing.assert_array_equal(no_count["node"], want["node"])
    np.testing.assert_array_equal(no_count["candidates"] + 3, want["candidates"])


def test_forced_stop_at_exactly_l_flagged_entries():
    """L + 8 copies of one shape under LeastRequested on equal nodes: each copy consumes a list entry,
    so pod L (0-based) finds all L entries flagged and the option stops there — unless the template
    beats the list's last key, which case (3) of place_decide still decides."""
    L = host_lib().ks_host_scaleup_l()
    c = tph.uniform(3 * L, L + 8, (1, 7, 1, 1, 0, 0), req=(4000, 16000, 0))
    want = brute(c, template(NODE, 0))
    got, done, res, stats = check(c, template(NODE, 0))
    assert done == L and res["path"] == -1 and stats[2] == L
    np.testing.assert_array_equal(got["node"][:L], np.arange(L))
    # one list entry fewer: no stop
    c2 = tph.uniform(3 * L, L, (1, 7, 1, 1, 0, 0), req=(4000, 16000, 0))
    got, done, res, stats = check(c2, template(NODE, 0))
    assert done == L and res["path"] == 0 and stats[2] == L - 1
    # a larger template: after the first L pods its key is above the list's last one, so it is decided
    got, done, res, stats = check(c, template([32000, 128000, 8000, 110], 50))
    assert done == L + 8 and res["path"] == 0 and res["on_new"] >= 8
    assert want["node"][L] >= 0


def test_whole_units_and_the_template_record():
    lb = host_lib()
    req = np.array([[2000, 4 << 20, 0], [1000, 1 << 20, 7]], np.int64)
    km = np.array([3, 3], np.uint32)           # gpu unmasked: 7 is ignored
    scale = np.array([1000, 1 << 20, 1000], np.int64)

    def whole(opts):
        o = np.array(opts, np.int64).reshape(-1, 7)
        return lb.ks_host_scaleup_whole(2, _p(req), _p(km), len(o), _p(o), _p(scale))
    ok = [16000, 64 << 20, -1, 110, 0, 0, 5]
    assert whole([ok]) == 1 and whole([ok, [16000, 64 << 20, 0, 3, 9, 9, 0]]) == 1
    assert whole([ok, [16001, 64 << 20, -1, 110, 0, 0, 5]]) == 0      # cpu off the unit
    assert whole([[16000, (64 << 20) + 1, -1, 110, 0, 0, 5], ok]) == 0  # memory off the unit, first option
    assert whole([[16000, 64 << 20, 1, 110, 0, 0, 5]]) == 0           # gpu off the unit
    assert whole([[16000, 64 << 20, 4000, 7, 0, 0, 5]]) == 1          # the pods count has no unit
    req[1, 0] = 1001
    assert whole([ok]) == 0                                           # a request off the unit
    out = np.zeros(10, np.int64)
    lb.ks_host_scaleup_template(_p(np.array([16000, 64 << 20, -1, 110], np.int64)), 5, 9, _p(scale), _p(out))
    assert out.tolist() == [16, 64, -1, 110, 0, 0, 0, 0, 5, 9]
    lb.ks_host_scaleup_template(_p(np.array([16001, 0, 3, 0], np.int64)), 0, 1 << 63, _p(np.array([1, 1, 1], np.int64)), _p(out))
    assert out.tolist() == [16001, 0, 3, 0, 0, 0, 0, 0, 0, -(1 << 63)]


def test_carve_scale_up():
    assert host_lib().ks_host_scaleup_carve() == 0
