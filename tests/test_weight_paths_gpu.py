"""Scorer weights past the 16-bit key edge on every engine path, against the oracle: the small,
role-split and chunk resolvers, the default choice above the small class (the fused chunk chain at
total + 1 = 65,535; the 32-bit key table with the XCD-ordered scan one past it), sharded merges, the
per-tick kernel, and the past-tick queries and previews.  The classes, the traces and the cached
oracle runs: tests/weight_cases.py, pinned on the oracle alone by tests/test_weight_cases.py (every
class wins binds at exactly its configured maximum, and totals cut to 16 bits would bind elsewhere).
Binds (pod, node, tick, status) and usage are compared after every step; everything is exact."""
import numpy as np
import pytest

import drain_ref as dr
import place_ref as pr
import state_ref
import weight_cases as wc
from harness import assert_same_binds, engine_run, make_engine, make_oracle, shard_ranks, step_ranks
from kubesim_amd import _lib

pytestmark = pytest.mark.gpu
ALL = list(wc.CLASSES)
CHUNK, ONE_POD = _lib.KS_ENGINE_CHUNK_RESOLVER, _lib.KS_ENGINE_ONE_POD_RESOLVER
EVAL_FLAGS = {"0": 0, "FORCE_WIDE": _lib.KS_ENGINE_FORCE_WIDE, "NO_TINY": _lib.KS_ENGINE_NO_TINY,
              "NO_MICRO": _lib.KS_ENGINE_NO_MICRO}
FIELDS = ("pod", "node", "tick", "status")


def _run(size, cls, batch=0, flags=0, shard=None, chunk=None, keep=False):
    """One engine over steps_of(size): binds and usage against the oracle after every step.  chunk:
    whether the chunk resolver must have run (True: its between-step invariants hold after every
    step and batches claimed candidate slots; False: its workspace was never made).  Returns the
    engine's binds (and the engine with `keep`)."""
    tr, enc = wc.trace_of(size)
    usage = wc.reference(size, cls)["usage"]
    eng = make_engine(tr, enc, wc.mode(cls), batch, flags, shard)
    eng.submit(enc["pods"])
    got = []
    for k, ob, ou in zip(wc.steps_of(size), wc.step_binds(size, cls), usage):
        eb, rc = engine_run(eng, k, k)
        assert rc == 0
        assert_same_binds(eb, ob)
        np.testing.assert_array_equal(eng.usage(), ou)
        inv = eng.debug_invariants()
        assert inv["slot_marks"] == 0 and inv["e_marks"] == 0, inv
        got.append(eb)
    assert eng.queued == 0
    if chunk is not None:
        assert (inv["nslot_hw"] > 0 and inv["slot_max"] > 0) if chunk else inv["slot_max"] == 0, inv
    got = np.concatenate(got)
    if keep:
        return eng, got
    eng.close()
    return got


# ---- 1. the small (register-table) resolver --------------------------------------------------------
@pytest.mark.parametrize("flag", list(EVAL_FLAGS))
@pytest.mark.parametrize("cls", ALL)
def test_small_resolver_every_evaluator(cls, flag):
    _run("S", cls, 64, EVAL_FLAGS[flag])


@pytest.mark.parametrize("cls", ALL)
def test_small_resolver_ten_blocks(cls):
    _run("M", cls, 128)


# ---- 2. the role-split resolver --------------------------------------------------------------------
@pytest.mark.parametrize("cls", ALL)
def test_batch_256_outside_the_small_class(cls):
    """Batches of 256 pods: the role-split resolver for every class but w16, which the chunk
    resolver takes by default."""
    _run("M", cls, 256, chunk=cls == "w16")


@pytest.mark.parametrize("cls", ["w16", "w16p", "wmax"])
def test_role_split_resolver_forced(cls):
    """With the flag also the one-pod first step stays on the resolver (w16: its 16-bit key table at
    total + 1 = 65,535)."""
    _run("M", cls, 256, ONE_POD, chunk=False)


# ---- 3. the chunk resolver at its top value --------------------------------------------------------
@pytest.mark.parametrize("extra", ["0", "NO_OVERLAP", "PRUNED_LISTS", "SMALL_E"])
def test_chunk_resolver_at_65535(extra):
    _run("M", "w16", 0, CHUNK | (0 if extra == "0" else getattr(_lib, "KS_ENGINE_" + extra)), chunk=True)


def test_chunk_flag_one_past_its_domain():
    """w16p is not eligible: the flag is ignored and the binds are the oracle's all the same."""
    _run("M", "w16p", 0, CHUNK, chunk=False)
    _run("M", "w16p", 256, CHUNK, chunk=False)


# ---- 4. the default choice above the small class ---------------------------------------------------
@pytest.mark.parametrize("cls", ["w16", "w16p", "w17", "wmax"])
def test_default_chain_above_8192_nodes(cls):
    """9,000 nodes, 36 scan blocks, no flags: w16 on the fused chunk chain, the others on the 32-bit
    key table with the XCD-ordered scan and the role-split resolver."""
    _run("L", cls, chunk=cls == "w16")


def test_pruned_lists_flag_on_the_32_bit_table():
    _run("L", "w17", 0, _lib.KS_ENGINE_PRUNED_LISTS)


# ---- 5. shards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["w17", "wmax"])
def test_three_virtual_shards(cls):
    _run("M", cls, 0, 0, shard=(1, 0, None, 3))


@pytest.mark.parametrize("cls", ["w17", "wmax"])
def test_two_ranks(cls):
    tr, enc = wc.trace_of("M")
    engs, x = shard_ranks(tr, enc, 2, 1, mode=wc.mode(cls))
    for k, ob, ou in zip(wc.steps_of("M"), wc.step_binds("M", cls), wc.reference("M", cls)["usage"]):
        for b in step_ranks(engs, k, x):
            assert_same_binds(b, ob)
        for e in engs:
            np.testing.assert_array_equal(e.usage(), ou)
    for e in engs:
        e.close()
    x.close()


# ---- 6. the per-tick kernel -------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["w16p", "wmicro", "wmicro1", "wmax"])
def test_per_tick_kernel_and_head_probes(cls):
    """KubeSim.run: one submit and ks_step(1) per tick on 5,000 nodes; ks_filter / ks_score of the
    queue's head against the oracle's evaluation every tick.  ks_score returns the weighted total
    itself: the configured maximum for the top pods."""
    from kubesim_amd.kubesim import KubeSim, TraceSubmitter
    tr, enc = wc.trace_of("T")
    T = wc.ticks_of("T")
    ora = make_oracle(tr, wc.mode(cls))
    ora.submit(tr)
    obinds, seen = [], dict(probes=0, at_top=0, one_launch=0, head=False)

    def probe(eng, tick):
        if seen["head"]:   # the step before this probe had a pod to bind: the one-launch path took it
            seen["one_launch"] += int(eng.last_step_stats()["launches"] == 1)
        seen["head"] = eng.queued > 0
        while ora.tick < tick - 1:
            b, rc = ora.step(1, cap=1)
            assert rc == 0
            obinds.append(b)
        if eng.queued > 0:
            q = eng._submitted - eng.queued
            feas, score = ora.eval(q)
            got = eng.score(q)
            assert got.dtype == np.int64
            np.testing.assert_array_equal(got, score, err_msg=f"ks_score pod {q} tick {tick}")
            np.testing.assert_array_equal(eng.filter(q), feas, err_msg=f"ks_filter pod {q} tick {tick}")
            seen["probes"] += 1
            seen["at_top"] += int(got.max() == wc.MAXIMUM[cls])

    eng = make_engine(tr, enc, wc.mode(cls))
    ks = KubeSim(eng, tr["tick_seconds"])
    ks.register_submitter(TraceSubmitter(enc["pods"]))
    ks.run(T, probe=probe)
    b, rc = ora.step(T - ora.tick, cap=T)
    assert rc == 0
    obinds.append(b)
    ob = {f: np.concatenate([x[f] for x in obinds]) for f in FIELDS}
    assert len(ob["pod"]) == tr["pods"]["m"]
    assert_same_binds(ks.all_binds(), ob)
    np.testing.assert_array_equal(eng.usage(), ora.usage())
    assert ks.calls["step"] == T and seen["probes"] == tr["pods"]["m"] and seen["at_top"] >= 20, seen
    assert seen["one_launch"] >= tr["pods"]["m"] - 1, seen   # (the last pod's step has no probe after it)
    eng.close()
    ora.close()


# ---- 7. past-tick queries and previews ---------------------------------------------------------------
QUERY_PODS = [0, 1, 2, 16, 32, 48, 64, 80, 96, 112, 7, 37, 67, 97, 127, 157, 187, 217, 247, 277]


@pytest.fixture(scope="module", params=["wmax", "w16p"])
def ran(request):
    eng, eb = _run("S", request.param, keep=True)
    yield request.param, eng, eb
    eng.close()


def _state(cls, t):
    tr, _ = wc.trace_of("S")
    return state_ref.IntervalRef(tr, wc.reference("S", cls)["binds"]).at(t)


def test_score_at_and_filter_at(ran):
    cls, eng, eb = ran
    at_top = 0
    for q in QUERY_PODS:
        score, mask = wc.score_before("S", wc.CLASSES[cls], wc.state_before("S", cls, q), q)
        got = eng.score_at(q)
        np.testing.assert_array_equal(got, score, err_msg=f"score_at pod {q}")
        np.testing.assert_array_equal(eng.filter_at(q), mask, err_msg=f"filter_at pod {q}")
        assert int(np.argmax(got)) == int(eb["node"][q])
        at_top += int(got.max() == wc.MAXIMUM[cls])
    assert at_top >= 10


def _place_shapes(pods):
    e = wc.trace_of("S")[1]["pods"]
    return {f: np.ascontiguousarray(np.asarray(e[f])[pods]) for f in ("req", "keymask", "tol", "sel")}


@pytest.mark.parametrize("t", [160, None])
def test_place_at(ran, t):
    """64 copies of the top pods' shape (every one scores the maximum on a node with nothing
    requested), and 64 pods over four shapes: a top pod's and three of the trace's."""
    cls, eng, _ = ran
    _, enc = wc.trace_of("S")
    t = wc.ticks_of("S") if t is None else t
    state = _state(cls, t)
    cfg = pr.engine_cfg(wc.mode(cls), enc)
    one, four = _place_shapes([16]), _place_shapes([16, 7, 37, 67])
    for what, sh, so in (("one shape", one, np.zeros(64, np.int32)), ("four shapes", four, (np.arange(64) * 3 % 4).astype(np.int32))):
        want = pr.fast_place(enc["alloc"], state, cfg, sh, so)
        assert (want["status"] == pr.OK).sum() >= 48 and want["score"].max() == wc.MAXIMUM[cls]
        pr.assert_same(eng.place_at(t, sh, so, after=True), want, f"{cls} tick {t}: {what}")
    assert len(set(want["score"].tolist())) >= 3 and len(set(want["node"].tolist())) >= 3


@pytest.mark.parametrize("t", [160, None])
def test_drain_at(ran, t):
    """The 16 nodes that run the most pods: their pods are scored again without them."""
    cls, eng, _ = ran
    tr, enc = wc.trace_of("S")
    t = wc.ticks_of("S") if t is None else t
    state = _state(cls, t)
    drained = np.argsort(-state[:, 3], kind="stable")[:16].tolist()
    ob = wc.reference("S", cls)["binds"]
    ev, frm = dr.running_on(tr, enc, ob, t, drained)
    want = dr.fast_drain(enc["alloc"], state, pr.engine_cfg(wc.mode(cls), enc), enc["pods"], ev, frm, drained)
    assert len(ev) >= 16 and (want["status"] == dr.OK).sum() >= 12 and want["score"].max() == wc.MAXIMUM[cls]
    dr.assert_same(eng.drain_at(t, drained, after=True), want, f"{cls} tick {t}")


# ---- 8. eight scorer entries ------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["S", "M"])
def test_split8_binds_as_its_folded_form(size):
    a = _run(size, "split8")
    tr, enc = wc.trace_of(size)
    eng = make_engine(tr, enc, wc.mode(wc.SPLIT8_FOLDED))
    eng.submit(enc["pods"])
    b, rc = engine_run(eng, wc.ticks_of(size), wc.ticks_of(size))
    assert rc == 0
    for f in FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    eng.close()


# ---- 9. ks_create's bound (the rejections need no device: tests/test_abi.py) ------------------------
def test_largest_accepted_total():
    from kubesim_amd.engine import Engine, KsError
    Engine(filter_mode=1, filters=7, scorers=wc.CLASSES["wmax"]).close()
    with pytest.raises(KsError) as ex:
        Engine(filter_mode=1, filters=7, scorers=wc.CLASSES["wmax"] + ((0, 1, 1),))   # 2^30 - 2
    assert ex.value.code == _lib.KS_EINVAL
