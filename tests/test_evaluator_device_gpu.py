"""The device build of every evaluator variant against exact integers (ks_selftest_eval, ks_selftest).

The host tests run ks_device.h with an exact reciprocal and plain-C multiplies; here the same cases
and the boundary-biased ones of tests/evaluator_cases.py run on the hardware forms (v_rcp_f32 /
v_rcp_f64, the 24-bit multiplies, v_sad_u32, the saturating conversion, the 128-bit path), through
every node-state type the resolvers feed them: the 64-bit node, the 12-word record, the chunk
resolver's 32-bit words and the register resolver's entries.  Each column must equal
`total1_exact` (Python integers, oracle/pysim.py's formulas) and the host build's column; the float
prune bound must never undercut the total.  The last test goes through the real ABI on clusters at
each domain's edge whose nodes run pods.
"""
from math import gcd

import numpy as np
import pytest

import evaluator_cases as ec
from harness import encoded, make_engine, make_oracle, small_trace

pytestmark = pytest.mark.gpu

FORMS = ("node", "rec12", "words", "entry")  # total1 column 4 * form + mode
PRUNE_FORMS = ("node", "words", "entry")     # tmax / live column 4 * form + mode
PRUNE_BIT, SCAN_COL = 17, 16

_cache = {}


def batch(domain):
    if domain not in _cache:
        _cache[domain] = ec.edge_cases(domain)
    return _cache[domain]


def variants_for(domain):
    """Every column whose evaluator and state form admit the generator's cases."""
    v = 0
    for m in ec.modes_for(domain):
        for g, form in enumerate(FORMS):
            # the wide entry is the 64-bit node itself; the other 32-bit forms need one-word capacities
            if form in ("rec12", "words") and not ec.words_ok(domain):
                continue
            v |= 1 << (4 * g + m)
        for g, form in enumerate(PRUNE_FORMS):
            if form == "words" and not ec.words_ok(domain):
                continue
            v |= 1 << (PRUNE_BIT + 4 * g + m)
    if ec.MICRO in ec.modes_for(domain):
        v |= 1 << SCAN_COL
    return v


def _cols(variants, lo, hi):
    return [b - lo for b in range(lo, hi) if (variants >> b) & 1]


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("domain", sorted(ec.DOMAINS))
def test_device_columns_equal_exact_total(domain, k):
    from kubesim_amd.engine import selftest_eval
    b = batch(domain)
    cfg = ec.CONFIGS[domain][k]
    variants = variants_for(domain)
    exact, _ = ec.total1_exact(cfg, **b)
    unfiltered, _ = ec.total1_exact(dict(cfg, filter_feeds=0), **b)  # the bound ignores the filters
    modes = ec.modes_for(domain)
    h_total1, _, _ = ec.host_eval(cfg, b, modes, scan=ec.MICRO in modes, prune=False)
    total1, tmax, live = selftest_eval(cfg, variants=variants, **b)
    cols = _cols(variants, 0, PRUNE_BIT)
    assert len(cols) >= 2 * len(modes)
    for c in cols:
        m = 3 if c == SCAN_COL else c % 4
        np.testing.assert_array_equal(total1[c], exact, err_msg=f"column {c} {cfg}")
        np.testing.assert_array_equal(total1[c], h_total1[4 if c == SCAN_COL else m])
    want_live = ec.live_exact(cfg, b)
    for c in _cols(variants, PRUNE_BIT, PRUNE_BIT + 12):
        np.testing.assert_array_equal(live[c], want_live, err_msg=f"live column {c} {cfg}")
        on = want_live == 1
        short = tmax[c][on].astype(np.int64) < unfiltered[on].astype(np.int64) - 1
        assert not short.any(), f"prune bound below the exact total: column {c} {cfg} case {np.flatnonzero(on)[short][:5]}"
    # columns not asked for stay untouched
    for c in set(range(17)) - set(cols):
        assert (total1[c] == 0).all()


@pytest.mark.parametrize("feeds,const,w_lr,w_ba", [(1, 0, 1, 1), (0, 0, 1, 1), (1, 5, 2, 0), (0, 3, 0, 3),
                                                   (1, 0, 7, 13), (0, 1000, 50, 50)])
@pytest.mark.parametrize("cap_bits", [20, 28])
def test_prune_bound_sound_and_tight_on_device(feeds, const, w_lr, w_ba, cap_bits):
    """The host prune test's batches on the device: narrow == wide, the bound never below the total and
    mostly within a couple of points of it (the host test's inequality, on device values)."""
    from kubesim_amd.engine import selftest_eval
    b = ec.nodes_cases(cap_bits, cap_bits * 1000 + w_lr * 10 + w_ba + const)
    n = len(b["keymask"])
    cfg = ec.mk_cfg(feeds, 1 if feeds else 0, w_lr, w_ba, const)
    variants = 0
    for m in (ec.WIDE, ec.NARROW):
        for g in range(4):
            variants |= 1 << (4 * g + m)
        for g in range(3):
            variants |= 1 << (PRUNE_BIT + 4 * g + m)
    total1, tmax, _ = selftest_eval(cfg, variants=variants, **b)
    exact, _ = ec.total1_exact(cfg, **b)
    for c in _cols(variants, 0, PRUNE_BIT):
        np.testing.assert_array_equal(total1[c], exact)
    live = exact > 0
    assert live.sum() > n // 3
    total = exact[live].astype(np.int64) - 1
    for c in _cols(variants, PRUNE_BIT, PRUNE_BIT + 12):
        tm = tmax[c]
        assert (total <= tm[live].astype(np.int64)).all(), "prune bound below the exact total"
        assert np.mean(tm[live].astype(np.int64) - total) < 0.2 * (w_lr + w_ba) + 0.5


def test_micro_states_selftest():
    """Every usage of thirteen micro capacity pairs, eval_total1_micro and eval_scan_micro against
    exact 64-bit integers on the device (ks_selftest test 1)."""
    from kubesim_amd import _lib
    from kubesim_amd.engine import selftest
    assert selftest(_lib.KS_SELFTEST_MICRO_STATES) == 0


def test_batch_outside_a_domain_refused():
    from kubesim_amd import _lib
    from kubesim_amd.engine import KsError, selftest_eval
    cfg = ec.mk_cfg(1, 7, 1, 1, 0)

    def one(ac, am, ag=0, rc=0, nr=0, req=1):
        return dict(alloc=np.array([[ac, am, ag, 110]], np.int64), run=np.array([[rc, 0, 0, nr]], np.int64),
                    req=np.array([[req, 1, 0]], np.int64), keymask=np.array([7], np.uint32),
                    masks=np.zeros((1, 4), np.uint64))

    def refused(cfg, variants, case):
        with pytest.raises(KsError) as ex:
            selftest_eval(cfg, variants=variants, **case)
        return ex.value.code == _lib.KS_EINVAL

    col = lambda form, m: 1 << (4 * FORMS.index(form) + m)
    prune = lambda form, m: 1 << (PRUNE_BIT + 4 * PRUNE_FORMS.index(form) + m)
    for form in FORMS:
        assert refused(cfg, col(form, ec.MICRO), one(1 << 16, 1))            # kMicroCap
        assert refused(cfg, col(form, ec.MICRO), one(4096, 4096))            # kMicroProd
        assert refused(cfg, col(form, ec.MICRO), one(1, 1, ag=1 << 16))
        assert refused(ec.mk_cfg(1, 7, 1 << 24, 1, 0), col(form, ec.MICRO), one(10, 10))  # kMicroWeight
        assert refused(cfg, col(form, ec.TINY), one(1 << 26, 1))             # kTinyCap
        assert refused(cfg, col(form, ec.TINY), one(8192, 8192))             # cpu * memory
        assert refused(cfg, col(form, ec.NARROW), one(1 << 29, 1))           # kNarrowCap
        selftest_eval(cfg, variants=col(form, ec.MICRO), **one(4095, 4097))  # the edges themselves pass
        selftest_eval(cfg, variants=col(form, ec.TINY), **one(8191, 8193))
        selftest_eval(cfg, variants=col(form, ec.NARROW), **one((1 << 29) - 1, (1 << 29) - 1))
    assert refused(cfg, 1 << SCAN_COL, one(1 << 16, 1))
    for form in ("rec12", "words"):  # the word limit 2^32 - 1
        assert refused(cfg, col(form, ec.WIDE), one((1 << 32) - 1, 1))
        selftest_eval(cfg, variants=col(form, ec.WIDE), **one((1 << 32) - 2, (1 << 32) - 2))
    assert refused(cfg, prune("words", ec.WIDE), one(1, (1 << 32) - 1))
    assert refused(cfg, prune("node", ec.MICRO), one(1 << 16, 1))
    selftest_eval(cfg, variants=col("node", ec.WIDE) | col("entry", ec.WIDE), **one((1 << 59) - 1, (1 << 59) - 1))
    # what no evaluator is given: usage above its capacity, values out of range, unknown columns
    assert refused(cfg, col("node", ec.WIDE), one(10, 10, rc=11))
    assert refused(cfg, col("node", ec.WIDE), one(-1, 10, rc=1))
    assert refused(cfg, col("node", ec.WIDE), one(1 << 59, 10))
    assert refused(cfg, col("node", ec.WIDE), one(10, 10, req=1 << 59))
    assert refused(cfg, col("node", ec.WIDE), one(10, 10, req=-1))
    assert refused(cfg, col("node", ec.WIDE), one(10, 10, nr=(1 << 31) - 1))
    assert refused(cfg, 1 << 29, one(10, 10))
    assert refused(cfg, 0, one(10, 10))
    assert refused(ec.mk_cfg(1, 7, 1 << 27, 0, 0), col("node", ec.WIDE), one(10, 10))  # ks_create's total limit


# ---------------------------------------------------------------------------------------------
# through the real ABI: clusters at each domain's edge, nodes running pods
# ---------------------------------------------------------------------------------------------
# the largest cpu and memory capacity of the cluster (the engine's mode choice takes the maxima:
# micro needs max cpu * max memory < 2^24, tiny < 2^26), and the engine flags under which the
# domain's evaluator, then each wider one, runs
E2E = {
    "micro": dict(max=(4095, 4097), picked=ec.MICRO, flags=("0", "NO_MICRO", "NO_TINY", "FORCE_WIDE")),
    "tiny": dict(max=(8191, 8193), picked=ec.TINY, flags=("0", "NO_TINY", "FORCE_WIDE")),
    "narrow": dict(max=((1 << 29) - 1, (1 << 29) - 3), picked=ec.NARROW, flags=("0", "FORCE_WIDE")),
    "wide": dict(max=((1 << 59) - 3, (1 << 33) + 1), picked=ec.WIDE, flags=("0",)),  # (requests stay below 2^59)
}
E2E_NODES, E2E_PODS, E2E_BOUND = 4096, 6200, 6144
_e2e = {}


def picked_mode(alloc, w_lr, w_ba):
    """ks_engine.cpp update_mode on capacities whose gcd scale is 1."""
    m = [int(alloc[:, k].max()) for k in range(3)]
    if max(m) < (1 << 16) and m[0] * m[1] < (1 << 24) and max(w_lr, w_ba) < (1 << 24):
        return ec.MICRO
    if max(m) < (1 << 26) and m[0] * m[1] < (1 << 26):
        return ec.TINY
    return ec.NARROW if max(m) < (1 << 29) else ec.WIDE


def e2e_case(domain):
    """(trace, encoded, oracle stepped E2E_BOUND ticks, its binds): built and stepped once per domain."""
    if domain in _e2e:
        return _e2e[domain]
    mc, mm = E2E[domain]["max"]
    rng = np.random.default_rng(sorted(E2E).index(domain) + 77)
    tr = small_trace(61, n_nodes=E2E_NODES, n_pods=E2E_PODS)
    nd, p = tr["nodes"], tr["pods"]
    N, P = E2E_NODES, E2E_PODS

    def caps(mx):  # the maximum, just under it, and sizes down to a 64th of it
        c = np.maximum((mx * 2.0 ** (-6 * rng.random(N))).astype(np.int64), 1)
        c = np.where(rng.random(N) < 0.2, mx - rng.integers(0, 7, N), c)
        c[0] = mx
        return c
    nd["alloc"][:, 0] = caps(mc)
    nd["alloc"][:, 1] = caps(mm)
    nd["alloc"][:, 2] = np.minimum(nd["alloc"][:, 2], min(mc, mm) - 1)
    nd["alloc"][1, 0] = mc - 1  # consecutive values: the gcd scale of each resource is 1
    nd["alloc"][1, 1] = mm - 1
    nd["alloc"][2:4, 2] = (3, 2)
    for k in range(3):
        has = (nd["alloc_has"] >> k) & 1 == 1
        nd["alloc"][~has, k] = 0
    # requests a few to a node of median size, some past the small nodes
    p["req"][:, 0] = np.maximum((mc * 2.0 ** (-3 - 5 * rng.random(P))).astype(np.int64), 1)
    p["req"][:, 1] = np.maximum((mm * 2.0 ** (-3 - 5 * rng.random(P))).astype(np.int64), 1)
    p["req"][:, 2] = np.where(rng.random(P) < 0.7, 0, 1)
    # among the pods still queued after the steps: requests above every capacity, an absent key, a
    # request that is exactly a capacity
    q = E2E_BOUND
    p["req"][q + 1, 0] = mc + 1
    p["req"][q + 2, 1] = min(mm * 3, (1 << 59) - 1)
    p["req_has"][q + 3] = 6
    p["req"][q + 3, 0] = 0
    p["req_has"][q + 4] = 5
    p["req"][q + 4, 1] = 0
    p["req"][q + 5, :2] = (mc, mm)
    p["req"][q + 6, :2] = (1, 1)
    owner = np.repeat(np.arange(P), np.diff(p["phase_off"]))
    p["phase_use"][:] = p["req"][owner] * rng.integers(1, 5, len(owner))[:, None] // 4
    enc = encoded(tr)
    for k in range(3):  # the device unit of every resource is 1
        g = 0
        for v in enc["alloc"][:, k]:
            g = gcd(g, max(int(v), 0))
        assert g == 1, (domain, k, g)
    assert picked_mode(enc["alloc"], 1, 1) == E2E[domain]["picked"]
    ora = make_oracle(tr, "feeds_all_lrba")
    ora.submit(tr)
    ob, rc = ora.step(E2E_BOUND, cap=E2E_BOUND)
    assert rc == 0 and len(ob["pod"]) == E2E_BOUND
    ok = ob["status"] == 0
    assert len(np.unique(ob["node"][ok])) > E2E_NODES // 2, "most nodes run pods"
    evals = {pod: ora.eval(pod) for pod in range(E2E_BOUND, E2E_BOUND + 8)}
    _e2e[domain] = (tr, enc, ob, evals)
    return _e2e[domain]


@pytest.mark.parametrize("domain,flag", [(d, f) for d in E2E for f in E2E[d]["flags"]])
def test_filter_and_score_on_loaded_nodes_match_oracle(domain, flag):
    from kubesim_amd import _lib
    from harness import assert_same_binds, engine_run
    tr, enc, ob, evals = e2e_case(domain)
    flags = 0 if flag == "0" else getattr(_lib, "KS_ENGINE_" + flag)
    eng = make_engine(tr, enc, "feeds_all_lrba", engine_flags=flags)
    eng.submit(enc["pods"])
    eb, rc = engine_run(eng, E2E_BOUND, 2048)
    assert rc == 0
    assert_same_binds(eb, ob)
    for pod, (feas, score) in evals.items():
        np.testing.assert_array_equal(eng.filter(pod), feas, err_msg=f"pod {pod}")
        np.testing.assert_array_equal(eng.score(pod), score, err_msg=f"pod {pod}")
    eng.close()
