"""The inputs of tests/test_weight_paths_gpu.py, pinned on the traces and the CPU oracle alone
(tests/weight_cases.py): every class reaches its configured maximum total, a total cut to 16 bits
(or a weight cut to 24) would choose other nodes, and the host's restated rules put every case on the
path it is listed for.  A case that misses its condition is changed in weight_cases.py; the
conditions here stay.
"""
import numpy as np
import pytest

import group_cases as gc
import weight_cases as wc

RUN_SIZES = ("S", "M", "L")


def test_maxima_are_the_configured_sums():
    for cls, sc in wc.CLASSES.items():
        const, w_lr, w_ba = gc.weights(sc)
        assert const + 10 * (w_lr + w_ba) == wc.MAXIMUM[cls], cls
    assert wc.MAXIMUM["w16"] + 1 == (1 << 16) - 1 and wc.MAXIMUM["w16p"] + 1 == 1 << 16
    assert wc.MAXIMUM["wmax"] + 1 == (1 << 30) - 2
    assert gc.weights(wc.CLASSES["split8"]) == gc.weights(wc.SPLIT8_FOLDED) == (1, 4000, 3000)
    assert len(wc.CLASSES["split8"]) == 8
    assert max(gc.weights(wc.CLASSES["wmicro"])[1:]) == gc.MICRO_WEIGHT - 1
    assert gc.weights(wc.CLASSES["wmicro1"])[1] == gc.MICRO_WEIGHT


@pytest.mark.parametrize("size", list(wc.SIZES))
def test_planted_trace(size):
    """Top pods request 0 cpu and 0 memory with both keys present and pass every taint and selector;
    no other pod passes the stripe's taint; the stripe's nodes have cpu and memory."""
    tr, enc = wc.trace_of(size)
    n, m, _ = wc.SIZES[size]
    assert (tr["nodes"]["n"], tr["pods"]["m"]) == (n, m)
    top = wc.is_top(np.arange(m))
    assert top[:3].all() and top[16] and not top[17] and top.sum() == 3 + (m - 1) // 16
    e = enc["pods"]
    assert (e["req"][top] == 0).all() and (e["keymask"][top] == 3).all() and (e["sel"][top] == 0).all()
    stripe = np.arange(n) % wc.STRIPE_EVERY == wc.STRIPE_AT
    taint = np.asarray(enc["taint"], np.uint64)
    passes = (taint[None, :] & ~np.asarray(e["tol"], np.uint64)[:, None]) == 0     # [pod][node]
    assert passes[top].all()
    assert not passes[~top][:, stripe].any()
    assert (enc["alloc"][stripe, :2] > 0).all()
    assert np.diff(tr["pods"]["arrival"]).max() == 2 and np.diff(tr["pods"]["arrival"]).min() == 0


@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("cls", list(wc.CLASSES))
def test_reaches_the_top(size, cls):
    """At least 20 binds are won with exactly the class's maximum total, every pod is bound, and
    the stripe keeps nodes with nothing requested to the end."""
    r = wc.reference(size, cls)
    b = r["binds"]
    at_top = r["win_total"] == wc.MAXIMUM[cls]
    print(size, cls, "binds won at the maximum:", int(at_top.sum()), "largest winning total:", int(r["win_total"].max()))
    assert len(b["pod"]) == wc.SIZES[size][1] and (b["status"] == 0).all()
    assert at_top.sum() >= 20
    assert r["win_total"].max() == wc.MAXIMUM[cls]
    assert wc.is_top(b["pod"][at_top]).all()
    if cls == "w16":
        assert (r["win_total"][at_top] + 1 == 65535).all()
    if cls == "w16p":
        assert (r["win_total"][at_top] + 1 == 65536).all()
    if cls == "wmax":
        assert (r["win_total"][at_top] + 1 == (1 << 30) - 2).all()
    assert len(r["usage"]) == 3


@pytest.mark.parametrize("size", RUN_SIZES)
@pytest.mark.parametrize("cls", ["w17", "wmicro", "wmax"])
def test_truncated_totals_choose_other_nodes(size, cls):
    """Pods 50 apart: for at least half, the lowest-index maximum of (total + 1) & 0xFFFF is another
    node than the true winner."""
    r = wc.reference(size, cls)
    sampled = sorted(r["evals"])
    assert sampled == list(range(0, wc.SIZES[size][1], wc.SAMPLE_EVERY))
    moved = [bool(r["trunc_moves"][q]) for q in sampled]   # bind i is pod i: every pod is bound
    print(size, cls, "argmax moves for", sum(moved), "of", len(moved))
    assert 2 * sum(moved) >= len(moved)


@pytest.mark.parametrize("size", RUN_SIZES)
def test_w16p_top_pods_truncate_to_zero(size):
    r = wc.reference(size, "w16p")
    at_top = r["win_total"] == wc.MAXIMUM["w16p"]
    assert ((r["win_total"][at_top] + 1) & 0xFFFF == 0).all()
    assert r["trunc_moves"][at_top].all()
    assert r["trunc_moves"][wc.is_top(r["binds"]["pod"])].all()


@pytest.mark.parametrize("size", RUN_SIZES)
def test_wmicro1_weight_cut_to_24_bits_changes_every_total(size):
    """w_lr & (2^24 - 1) = 0 for wmicro1: with that weight every scored node's total differs from the
    true one.  The integer restatement used for it (and by the GPU tests' past-tick checks) equals the
    oracle's own evaluation on the true weights first."""
    sc = wc.CLASSES["wmicro1"]
    cut = tuple((k, w & ((1 << 24) - 1), v) if k == 1 else (k, w, v) for k, w, v in sc)
    assert gc.weights(cut)[1] == 0 and gc.weights(cut)[2] == gc.weights(sc)[2]
    r = wc.reference(size, "wmicro1")
    scored = 0
    for q, (feas, score) in r["evals"].items():
        state = wc.state_before(size, "wmicro1", q, at_eval=True)
        true, mask = wc.score_before(size, sc, state, q)
        np.testing.assert_array_equal(true, score, err_msg=f"pod {q}")
        np.testing.assert_array_equal(mask, feas, err_msg=f"pod {q}")
        # at the bind tick itself the restatement's lowest-index maximum is the node the pod got
        at_bind, _ = wc.score_before(size, sc, wc.state_before(size, "wmicro1", q), q)
        assert int(np.argmax(at_bind)) == int(r["binds"]["node"][q]), f"pod {q}"
        wrong, _ = wc.score_before(size, cut, state, q)
        on = score >= 0
        assert on.any() and (wrong[on] != true[on]).all(), f"pod {q}"
        scored += int(on.sum())
    print(size, "scored (pod, node) pairs:", scored)


def test_every_case_is_on_the_path_it_is_listed_for():
    for size in wc.SIZES:
        tr, _ = wc.trace_of(size)
        r16, r16p = gc.restate(tr, wc.mode("w16")), gc.restate(tr, wc.mode("w16p"))
        assert r16["k16"] and not r16p["k16"]
        assert gc.chunk_eligible(r16) and not gc.chunk_eligible(r16p)
        for cls in ("w17", "wmicro", "wmicro1", "wmax", "split8"):
            rr = gc.restate(tr, wc.mode(cls))
            assert not rr["k16"] and not gc.chunk_eligible(rr), cls
        assert gc.restate(tr, wc.mode("wmicro"))["cls"] == gc.MICRO
        assert gc.restate(tr, wc.mode("wmicro1"))["cls"] == gc.TINY
        # the same capacities, and every other class is micro by them
        assert gc.restate(tr, wc.mode("wmicro"))["scaled_max"] == gc.restate(tr, wc.mode("wmicro1"))["scaled_max"]
        for cls in ("w16", "w16p", "w17", "split8"):
            assert gc.restate(tr, wc.mode(cls))["cls"] == gc.MICRO, cls
        assert gc.restate(tr, wc.mode("wmax"))["cls"] == gc.TINY   # its weights are past 2^24 too
    s, m, l, t = (wc.trace_of(x)[0] for x in ("S", "M", "L", "T"))
    big = gc.restate(l, wc.mode("w17"))
    assert not big["small"] and big["B"] == gc.DEFAULT_BATCH and big["blocks"] == 36
    assert l["nodes"]["n"] > gc.SMALL_MAX_NODES
    for tr in (s, m):
        assert gc.restate(tr, wc.mode("w17"), batch_pods=64)["small"]
    assert gc.restate(m, wc.mode("w17"), batch_pods=128)["small"]
    assert not gc.restate(m, wc.mode("w17"), batch_pods=256)["small"]
    assert gc.restate(m, wc.mode("w16"), batch_pods=256)["B"] <= 256 and gc.chunk_eligible(gc.restate(m, wc.mode("w16"), batch_pods=256))
    assert gc.restate(t, wc.mode("wmax"))["blocks"] == 20   # 5,000 nodes: five 1,024-node workgroups of the per-tick kernel


@pytest.mark.parametrize("size", RUN_SIZES)
def test_split8_binds_as_its_folded_form(size):
    a, b = wc.reference(size, "split8")["binds"], wc.reference(size, wc.SPLIT8_FOLDED)["binds"]
    for f in a:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    for x, y in zip(wc.reference(size, "split8")["usage"], wc.reference(size, wc.SPLIT8_FOLDED)["usage"]):
        np.testing.assert_array_equal(x, y)
    # and not as a single-entry reading of it would
    assert gc.weights(wc.CLASSES["split8"][:1]) != gc.weights(wc.SPLIT8_FOLDED)


def test_step_cuts_cover_the_run():
    for size in RUN_SIZES:
        parts = wc.step_binds(size, "w17")
        assert sum(len(p["pod"]) for p in parts) == wc.SIZES[size][1]
        assert all(len(p["pod"]) > 0 for p in parts[1:])
        assert sum(wc.steps_of(size)) == wc.ticks_of(size)
        assert (parts[0]["tick"] <= 1).all() and (parts[1]["tick"] <= 38).all() and (parts[2]["tick"] > 38).all()
