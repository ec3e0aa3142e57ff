"""The five previews (ks_place_at, ks_drain_at, ks_removable_at, ks_consolidate_at, ks_scale_up_at) at
width and depth: the inputs and cached references of tests/test_preview_wide_gpu.py, pinned on the
references alone by tests/test_preview_wide_cases.py.

Width (WIDE): place_merge_kernel (ks_place.hip) folds the block lists b = lane, lane + 64, ... per
lane; up to 64 scan blocks of 256 nodes no lane folds a second list.  The clusters here have 64, 65
and 129 scan blocks, and their best nodes are planted by hand:

    base      8 cpu / 32 Gi, untainted: every other node — every block counts candidates, none wins;
    hosts     128 cpu / 512 Gi, untainted, at the offsets HOST_AT of each of the blocks 0, 63, 64, 65 and the
              last: the trace's own pods tolerate nothing and score these highest, so they run there;
    idle      128 cpu / 512 Gi behind a NoSchedule taint, at IDLE_AT in each of IDLE_BLOCKS and the last
              block: no trace pod runs there, so for a preview shape that tolerates the taint they all
              tie at the top and the lower index wins — blocks b, b + 64 and b + 128 of one lane;
    extras    64 cpu / 256 Gi behind the taint, one in each of EXTRA_BLOCKS: with the idle nodes the
              "os-wide" label's nodes, more than one list holds;
    reserve   128 cpu / 512 Gi with room for one pod, untainted, two in each of RESERVE_BLOCKS: a trace
              pod fills one until it ends; those whose pod ended after the last arrival are idle at the
              queried tick and head every evicted pod's list;
    short     the "gpu-short" label on fewer than L nodes, all in blocks >= 64 (at 64 blocks: >= 32).

Depth (deep_case): drain_scan_kernel (ks_drain.hip) scans the candidate pod blocks' counts in chunks
of 256 with a carry; more than 256 candidate blocks need a pod that still runs in each of 258 blocks.

No engine is imported here.  Everything is built once and never changed afterwards.
"""
from __future__ import annotations

import functools

import numpy as np

import consolidate_ref as cr
import drain_ref as dr
import place_ref as pr
import removable_ref as rr
import scaleup_ref as su
import state_ref as sr
from chunk_replay_cases import set_run_ticks
from harness import MODES, encoded, small_trace
from kubesim_amd import tracegen

L = cr.SINGLE                      # KS_PLACE_L (tests/test_preview_wide_cases.py compares it with the source)
BLK = 256                          # nodes per scan block (ks_place.hip kPBlk), pods per gather block (kDrainBlk)
WAVE = 64                          # lists per trip of the merge
FEEDS, LITERAL = pr.FEEDS, pr.LITERAL
GI = (1 << 30) * 1000              # a Gi in milli-bytes
MI = (1 << 20) * 1000

# ---- width -------------------------------------------------------------------------------------------
# name: (nodes, mode, what the only node of a one-node last block is).  At 65 blocks that node is all of
# block 64: as a host it runs pods (the drain family's candidate in a second-trip block, the cordon's
# word 512), as an idle node it ties with block 0's idle nodes, which the same lane folds
WIDE = {"b64": (16_384, FEEDS, "host"), "b65": (16_385, FEEDS, "host"), "b65_idle": (16_385, FEEDS, "idle"),
        "b129": (32_770, FEEDS, "host"), "b65_literal": (16_385, LITERAL, "host")}
BASE, BIG, MID = (8_000, 32 * GI, 0, 110), (128_000, 512 * GI, 8_000, 110), (64_000, 256 * GI, 0, 110)
HOST_BLOCKS = (0, 63, 64, 65)      # and the last block
HOST_AT = (0, 31, 32, 100, 200, 255)          # offsets in the block: the cordon bitmap's word edges among them
IDLE_BLOCKS = (0, 5, 63, 64, 69, 127, 128)
IDLE_AT = (7, 130, 254)
EXTRA_BLOCKS = tuple(range(70, 100)) + tuple(range(8, 32))
EXTRA_AT = 77
RESERVE_BLOCKS = (3, 20, 33, 40, 50, 62, 66, 67, 70, 100, 126)
RESERVE_AT = (50, 150)
RESERVE = BIG[:3] + (1,)           # room for one pod
N_TRACE, T_WIDE, T_PAST = 260, 400, 160
N_LATER, T_NEXT = 20, 50           # pods that arrive after T_WIDE, two ticks apart; the ticks of the step after the previews
N_PODS = 48                        # preview pods of the mixed call
COPIES = 40                        # of the wide-gated shape: more distinct nodes than one list holds
SCALE_M = 300                      # appended nodes: n .. n + 299 crosses a scan-block edge at every width


def _plant(n, lone="host"):
    """dict(host, idle, extra, reserve, short): node indices of a cluster of n nodes"""
    nblk = -(-n // BLK)
    last = nblk - 1
    tail = n - last * BLK
    host, idle = [], []
    for b in sorted(set(HOST_BLOCKS + (last,))):
        if b < nblk:
            host += [b * BLK + o for o in HOST_AT if b * BLK + o < n]
    for b in sorted(set(IDLE_BLOCKS + (last,))):
        if b < nblk:
            idle += [b * BLK + o for o in IDLE_AT if b * BLK + o < n]
    if tail < BLK:                 # the ragged block: its last node idles, the rest host
        idle.append(n - 1)
        host = [x for x in host if x != n - 1]
        if tail == 1 and lone == "host":   # ... unless it is the only one and hosts (it is labelled all the same)
            idle.remove(n - 1)
            host.append(n - 1)
    idle = sorted(set(idle) - set(host))
    extra = [b * BLK + EXTRA_AT for b in EXTRA_BLOCKS if b < nblk]
    reserve = [b * BLK + o for b in RESERVE_BLOCKS if b < nblk for o in RESERVE_AT if b * BLK + o < n]
    lo = WAVE if nblk > WAVE else WAVE // 2
    short = [x for x in host + idle + extra if x // BLK >= lo][::2][:L - 5]
    return dict(host=sorted(host), idle=idle, extra=extra, reserve=reserve, short=sorted(short))


def wide_trace(n, lone="host"):
    tr = small_trace(41, n_nodes=n, n_pods=N_TRACE, arrival="stream", selectors=False, taints=False, tolerations=False)
    nd, p, st = tr["nodes"], tr["pods"], tr["strings"]
    pl = _plant(n, lone)
    nd["alloc"][:] = BASE
    nd["alloc_has"][:] = 15
    nd["alloc"][pl["host"] + pl["idle"]] = BIG
    nd["alloc"][pl["extra"]] = MID
    nd["alloc"][pl["reserve"]] = RESERVE
    # the taint of the idle nodes and the extras
    for s in ("planted", "idle"):
        st.append(s)
    behind = np.zeros(n, bool)
    behind[pl["idle"] + pl["extra"]] = True
    nd["taint_off"] = np.concatenate([[0], np.cumsum(behind)]).astype(np.int32)
    nd["taint"] = np.tile(np.array([[len(st) - 2, len(st) - 1, tracegen.NO_SCHEDULE]], np.int32), (int(behind.sum()), 1))
    # the gates: label family 3 (one value in the generated cluster) and family 2
    for s in ("os-wide", "gpu-short"):
        st.append(s)
    lab = nd["label"].reshape(n, 4, 2)
    lab[pl["idle"] + pl["extra"] + ([n - 1] if n - 1 in pl["host"] else []), 3, 1] = len(st) - 2
    lab[pl["short"], 2, 1] = len(st) - 1
    # the trace's pods: no gpu (the base nodes have none), runs of 1 .. 600 ticks
    p["req"][:, 2] = 0
    p["phase_use"][:, 2] = 0
    set_run_ticks(tr, 1 + (np.arange(N_TRACE) * 7919) % 600)
    assert p["arrival"][N_TRACE - N_LATER - 1] < T_WIDE - 100
    p["arrival"][N_TRACE - N_LATER:] = T_WIDE + 1 + 2 * np.arange(N_LATER)
    return tr, pl


def _bit(enc, strings, value):
    (i,) = [i for i, (k, v) in enumerate(enc["label_dict"]) if strings[v] == value]
    return np.uint64(1) << np.uint64(i)


def wide_shapes(tr, enc):
    """Eight shapes: 0 tolerates all (the idle nodes tie at the top); 1 small; 2 tolerates nothing; 3 the
    short gate; 4 the wide gate; 5 a trace pod's; 6 memory only, no multiple of the unit; 7 a selector
    no node carries."""
    ALL = np.uint64(0xFFFFFFFFFFFFFFFF)
    wide, short = _bit(enc, tr["strings"], "os-wide"), _bit(enc, tr["strings"], "gpu-short")
    p = enc["pods"]
    rows = [
        ([16_000, 64 * GI, 0], 3, ALL, 0),
        ([100, 256 * MI, 0], 3, ALL, 0),
        ([4_000, 16 * GI, 0], 3, 0, 0),
        ([8_000, 24 * GI, 0], 3, ALL, short),
        ([16_000, 64 * GI, 0], 3, ALL, wide),
        (p["req"][7].tolist(), int(p["keymask"][7]), p["tol"][7], p["sel"][7]),
        ([-1, pr.MEM_ODD, -1], 2, ALL, 0),
        ([1_000, GI, 0], 3, ALL, np.uint64(1) << np.uint64(63)),
    ]
    return dict(req=np.array([r[0] for r in rows], np.int64), keymask=np.array([r[1] for r in rows], np.uint8),
                tol=np.array([r[2] for r in rows], np.uint64), sel=np.array([r[3] for r in rows], np.uint64))


TIE, SMALL, PLAIN, SHORT, GATED = 0, 1, 2, 3, 4


def score_vectors(c, t, shapes=None):
    """[shapes][n] aggregated score + 1 on the state at t (0: no entry in the score map)"""
    enc, sh = c["enc"], shapes or c["shapes"]
    A, S = np.array(enc["alloc"], np.int64), np.array(c["state"][t], np.int64)
    taint, label = np.asarray(enc["taint"], np.uint64), np.asarray(enc["label"], np.uint64)
    live = np.ones(len(A), bool)
    out = []
    for j in range(len(sh["keymask"])):
        km = int(sh["keymask"][j])
        req = [int(sh["req"][j][k]) if (km >> k) & 1 else 0 for k in range(3)]
        out.append(dr.score_vector(c["cfg"], A, S, taint, label, live, (req, km, int(sh["tol"][j]), int(sh["sel"][j]))))
    return np.array(out)


def winners(v):
    """the first L nodes of a score vector in the engine's order (score descending, index ascending)"""
    order = np.lexsort((np.arange(len(v)), -v))
    return order[:L][v[order[:L]] > 0]


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """dict(n, nblk, tr, enc, mode, cfg, plant, ob (the oracle's binds over T_WIDE ticks), usage (its
    usage then), nxt (its binds of the next T_NEXT ticks), state {t}, shapes, shape_of)"""
    from harness import make_oracle
    n, mode, lone = WIDE[name]
    tr, pl = wide_trace(n, lone)
    enc = encoded(tr)
    ora = make_oracle(tr, mode)
    ora.set_threads(8)
    ora.submit(tr)
    ob, rc = ora.step(T_WIDE, cap=T_WIDE)
    assert rc == 0
    usage = ora.usage().copy()
    nxt, rc = ora.step(T_NEXT, cap=T_NEXT)
    assert rc == 0
    ora.close()
    state = {t: pr.state_from_binds(tr, enc, ob, t) for t in (T_PAST, T_WIDE)}
    shapes = wide_shapes(tr, enc)
    return dict(name=name, n=n, nblk=-(-n // BLK), tr=tr, enc=enc, mode=mode, cfg=pr.engine_cfg(MODES[mode], enc),
                plant=pl, ob=ob, nxt=nxt, usage=usage, state=state, shapes=shapes,
                shape_of=np.array([(5 * i) % 8 for i in range(N_PODS)], np.int32))


@functools.lru_cache(maxsize=None)
def place_ref(name, t):
    c = wide_case(name)
    return pr.fast_place(c["enc"]["alloc"], c["state"][t], c["cfg"], c["shapes"], c["shape_of"])


@functools.lru_cache(maxsize=None)
def copies_ref(name):
    c = wide_case(name)
    return pr.fast_place(c["enc"]["alloc"], c["state"][T_WIDE], c["cfg"], c["shapes"], np.full(COPIES, GATED, np.int32))


def busy(c, t, blocks):
    """per block of ``blocks`` (those the cluster has) the host node that runs the most pods at t"""
    run = c["state"][t][:, 3]
    out = []
    for b in blocks:
        h = [x for x in c["plant"]["host"] if x // BLK == b]
        if h:
            out.append(max(h, key=lambda x: (run[x], -x)))
    return out


def idle_reserve(c, t):
    """the reserve nodes that run no pod at t, ascending"""
    return [x for x in c["plant"]["reserve"] if c["state"][t][x, 3] == 0]


def drain_nodes(name):
    """Hosts running pods in blocks 0, 63, 64, 65 and the last; every other idle reserve node from the
    lowest on — the lowest heads every evicted pod's list, where the idle ones tie; the two highest
    tainted idle nodes and the lowest, which wins the preview shapes' tie."""
    c = wide_case(name)
    last = c["nblk"] - 1
    hosts = busy(c, T_WIDE, sorted(set(HOST_BLOCKS + (last,))))
    idle = c["plant"]["idle"]
    return sorted(set(hosts + idle_reserve(c, T_WIDE)[::2] + idle[-2:] + idle[:1]))


@functools.lru_cache(maxsize=None)
def drain_ref(name):
    c = wide_case(name)
    nodes = drain_nodes(name)
    ev, frm = dr.running_on(c["tr"], c["enc"], c["ob"], T_WIDE, nodes)
    return dr.fast_drain(c["enc"]["alloc"], c["state"][T_WIDE], c["cfg"], c["enc"]["pods"], ev, frm, nodes)


def candidates(name):
    """24 candidates in a permuted order: the drained nodes, the other hosts from the highest down,
    the other idle reserve nodes and tainted idle nodes."""
    c = wide_case(name)
    pl = c["plant"]
    more = pl["host"][::-1] + idle_reserve(c, T_WIDE)[1::2] + pl["idle"][1::3]
    pool = list(dict.fromkeys(drain_nodes(name) + more))
    pool = pool[:20] + pool[-4:] if len(pool) > 24 else pool
    rng = np.random.default_rng(len(pool) + c["n"])
    return tuple(int(pool[i]) for i in rng.permutation(len(pool)))


@functools.lru_cache(maxsize=None)
def removable_ref(name):
    c = wide_case(name)
    return rr.fast_removable(c["tr"], c["enc"], c["ob"], c["cfg"], T_WIDE, candidates(name), state=c["state"][T_WIDE])


@functools.lru_cache(maxsize=None)
def consolidate_ref(name):
    c = wide_case(name)
    return cr.fast_consolidate(c["tr"], c["enc"], c["ob"], c["cfg"], T_WIDE, candidates(name), state=c["state"][T_WIDE])


SCALE_SHAPES = (TIE, PLAIN, GATED, 5)


def scale_options(c):
    """Four templates: four times the largest node (it outscores every real node); a mid-sized one
    behind no taint (it loses to the planted nodes); none appended; one that takes two pods a node."""
    label = int(np.bitwise_or.reduce(np.asarray(c["enc"]["label"], np.uint64)))
    big = [4 * BIG[0], 4 * BIG[1], BIG[2], 110]
    return [su.option(big, SCALE_M, 0, label), su.option([32_000, 128 * GI, 0, 110], SCALE_M, 0, label),
            su.option(big, 0, 0, label), su.option(big[:3] + [2], 7, 0, label)]


def scale_shapes(c):
    return {f: np.ascontiguousarray(v[list(SCALE_SHAPES)]) for f, v in c["shapes"].items()}


SCALE_OF = np.array([(3 * i) % len(SCALE_SHAPES) for i in range(32)], np.int32)


@functools.lru_cache(maxsize=None)
def scale_ref(name):
    c = wide_case(name)
    return su.scale_up(c["enc"]["alloc"], c["state"][T_WIDE], c["cfg"], scale_shapes(c), SCALE_OF, scale_options(c))


@functools.lru_cache(maxsize=None)
def scale_place_ref(name):
    """place_at's answer for the scale-up's pods: what the option that appends nothing must give"""
    c = wide_case(name)
    return pr.fast_place(c["enc"]["alloc"], c["state"][T_WIDE], c["cfg"], scale_shapes(c), SCALE_OF)


# ---- depth -------------------------------------------------------------------------------------------
DEEP_BLOCKS = 258
DEEP_PODS = DEEP_BLOCKS * BLK      # 66,048
DEEP_NODES = 64
DEEP_T = DEEP_PODS + 20            # every pod arrives at tick 1 and one binds per tick
DEEP_LATE = DEEP_T                 # every block holds a running straggler: two scan chunks
DEEP_EARLY = 200 * BLK             # 200 blocks bound: one chunk
LANES = (0, 63, 64, 255)           # drain_rank's wave and lane terms
TRIPLE_BLOCK = 257                 # three stragglers in one block of the second chunk


def deep_stragglers():
    """At least one per block: lane (37 b) % 256; the lanes of LANES in the blocks 1, 255, 256; three
    in TRIPLE_BLOCK."""
    s = {b * BLK + (37 * b) % BLK for b in range(DEEP_BLOCKS)}
    for b in (1, 255, 256):
        s |= {b * BLK + o for o in LANES}
    s |= {TRIPLE_BLOCK * BLK + o for o in (5, 64, 200)}
    return np.array(sorted(s), np.int64)


@functools.lru_cache(maxsize=None)
def deep_case():
    """66,048 pods on 64 nodes, one bound per tick; every pod runs 1-3 ticks except the stragglers,
    which run past the end.  dict(tr, enc, ob, cfg, ref (state_ref.IntervalRef), stragglers)"""
    tr = small_trace(23, n_nodes=DEEP_NODES, n_pods=DEEP_PODS, selectors=False, taints=False, tolerations=False,
                     gpu_absent_p=0.0)
    p = tr["pods"]
    p["req"][:] = (500, 2 * GI, 0)
    p["req"][::3] = (1_000, GI, 0)
    p["req"][::7] = (250, 512 * MI, 0)
    own = np.repeat(np.arange(DEEP_PODS), np.diff(p["phase_off"]))
    p["phase_use"][:] = p["req"][own] // 2
    run = 1 + np.arange(DEEP_PODS) % 3
    s = deep_stragglers()
    run[s] = 100_000
    set_run_ticks(tr, run)
    enc = encoded(tr)
    ob = sr.oracle_binds(tr, MODES[FEEDS], DEEP_T)
    return dict(tr=tr, enc=enc, ob=ob, cfg=pr.engine_cfg(MODES[FEEDS], enc), ref=sr.IntervalRef(tr, ob), stragglers=s)


def deep_running_blocks(t):
    """the pod blocks that hold a pod running at tick t"""
    ref = deep_case()["ref"]
    return np.unique(ref.pod[(ref.b <= t) & (t < ref.e)] // BLK)


def deep_nodes(t):
    """Up to six nodes: those of stragglers of the blocks 255 and 256, of TRIPLE_BLOCK's three and of
    block 1; the same nodes at either tick (the control asks the same question earlier)."""
    c = deep_case()
    node = dict(zip(c["ob"]["pod"].tolist(), c["ob"]["node"].tolist()))
    want = [255 * BLK, 256 * BLK] + [TRIPLE_BLOCK * BLK + o for o in (5, 64, 200)] + [255 * BLK + 255, 256 * BLK + 63, BLK]
    return tuple(dict.fromkeys(int(node[q]) for q in want))[:6]


@functools.lru_cache(maxsize=None)
def deep_refs(t):
    """dict(nodes, state, drain, removable, consolidate (two orders)) at tick t"""
    c = deep_case()
    nodes = deep_nodes(t)
    state = c["ref"].at(t)
    ev, frm = dr.running_on(c["tr"], c["enc"], c["ob"], t, nodes)
    drain = dr.fast_drain(c["enc"]["alloc"], state, c["cfg"], c["enc"]["pods"], ev, frm, nodes)
    rem = rr.fast_removable(c["tr"], c["enc"], c["ob"], c["cfg"], t, nodes, state=state)
    cons = [cr.fast_consolidate(c["tr"], c["enc"], c["ob"], c["cfg"], t, order, state=state)
            for order in (nodes, nodes[::-1])]
    return dict(nodes=nodes, state=state, drain=drain, removable=rem, consolidate=cons)
