"""Expiry bursts: hundreds of pods ending on one tick.  The traces, step plans and cached oracle runs
of tests/test_expiry_burst_gpu.py (every engine chain against the oracle), pinned on the oracle
alone by tests/test_expiry_burst_cases.py.

The engine's expiry code has fixed-capacity tables, each with its own overflow path:

    16 / 17        live expiries attached to the next pod   kTickMaxExp (ks_step.cpp tick_step,
                                                            ks_engine.cpp flush_expiries)
    128 / 129      in a batch's window                      RSmall::kMaxExp (ks_resolve.hip)
    256 / 257      attached to a batch's first pod          expire_head_kernel's 256 threads
    512 / 513      in a window                              kWinSlots (ks_prep.h fits_win), ks_rolesplit.hip kMaxExp
    1,024 / 1,025  head expiries                            window_prep_kernel's kPrepThreads
    2,048          e_cnt + head + touched (+ previous E)    kEMax (EngineArgs::e_lim)

A burst of m is planted by run lengths: m pods bound one per tick each run exactly up to the burst
tick F, so the first pod bound at or after F (ks_submit_pods attaches an expiry to the first pod
bound at or after its finish tick) has m expiries attached.  Every third background pod runs 1-12
ticks, the rest LONG ticks (past every run's end); a short background pod whose end would attach to
a burst's pod is made long, so each burst pod carries exactly its planned count.

No engine is imported here.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from chunk_replay_cases import set_run_ticks
from harness import encoded, make_oracle, small_trace
from kubesim_amd import tracegen

# the table's edges, restated (tests/test_expiry_burst_cases.py compares them with the sources)
TICK_MAX_EXP = 16      # ks_device.h kTickMaxExp
SMALL_MAX_EXP = 128    # ks_resolve.hip RSmall::kMaxExp = kTMax - kMaxB = 256 - 128
HEAD_THREADS = 256     # ks_scan.hip expire_head_kernel's workgroup
WIN_SLOTS = 512        # ks_device.h kWinSlots; ks_rolesplit.hip kMaxExp = 768 - 256
BIG_TMAX, BIG_MAX_B = 768, 256
PREP_THREADS = 1024    # ks_cand.hip kPrepThreads
E_MAX = 2048           # ks_device.h kEMax
EDGES = (TICK_MAX_EXP, SMALL_MAX_EXP, HEAD_THREADS, WIN_SLOTS, PREP_THREADS, E_MAX)

LONG = 100_000         # run ticks of a pod that never ends inside a run
LEAD = 40              # background pods between a burst's last member and its burst pod
CLEAR = 300            # pods between a burst pod and the next burst's first member
MID = 98               # plan `mid`: the burst pod is the MID-th pod of its pass
NEAR = 1720            # the burst for PrepLDS::xn and the E hash near capacity: with the ~70 window
#                        expiries of the background and the up to 256 nodes the previous batch
#                        changed, still at most E_MAX (the sum holds values no trace can pin)
BURSTS = (16, 17, 128, 129, 256, 257, 512, 513, 1024, 1025, NEAR, 2100)
# bursts3k_refused: members planted per burst.  Below an edge the members are the edge itself (the
# live count falls under it); past an edge more members than the edge, so that the live count stays
# past it although a share of them is bound OverCapacity (chosen on the oracle)
REFUSED_BURSTS = (16, 28, 128, 200, 256, 400, 512, 800, 1024, 1600, NEAR, 3200)
REFUSED_SIDE = (-1, +1, -1, +1, -1, +1, -1, +1, -1, +1, 0, +1)   # live count: <= edge / > edge / not pinned
REFUSED_EDGE = (16, 16, 128, 128, 256, 256, 512, 512, 1024, 1024, 0, 2048)
# Requests at full size and no node without a gpu entry.  (Such a node refuses every pod, never
# fills, and so keeps the best score: under the literal mode it takes every later bind.  The refusals
# here are gpu requests on nodes whose gpus are taken — the scorers do not look at gpus — 11-25 % of
# every burst.  The node count changes little: 3,000 keeps the default engine on the chunk resolver.)
REFUSED_NODES = 3000
GAP_BURSTS = (16, 17, 257, 513, 1025)
GAP_PAUSE, GAP_INTO = 400, 100   # idle ticks planted; a burst ends GAP_INTO ticks into its pause
PIPE_NODES = 257 * 256           # tests/test_pipe_rescan_gpu.py NODES: 257 scan blocks per part pair
PIPE_BURSTS = (513, 2100)
SMALL_NODES = 2048               # small class at batch 128 (RSmall::kFilterBits = 8,192 nodes at the most)
SMALL_LAST = 257                 # the small-class runs take the plan up to this burst

# bursts whose pod has no other expiry within 256 pods on either side: a window that holds the burst
# holds exactly its count, so a window of exactly 128 / 512 goes through whole and one of 129 / 513 is cut
QUIET = (128, 129, 512, 513)

MODE = "feeds_all_lrba"
SPREAD = "feeds_fit_lr"
LITERAL = "literal_lrba_filters_ignored"


# ---- counting -------------------------------------------------------------------------------------
def attached(binds, run):
    """From a run's binds (in bind order) and the pods' run lengths in ticks: per bind index the
    expiries attached to that pod — those of pods finishing in (previous bind tick, this bind tick].
    Returns (live, csr): `csr` counts every bound pod that runs at all (ks_submit_pods builds the
    CSR before any status is known), `live` only the pods bound Ok (what is applied).  Index
    len(binds) holds the expiries no bound pod carries."""
    bt = np.asarray(binds["tick"], np.int64)
    d = np.asarray(run, np.int64)[binds["pod"]]
    at = np.searchsorted(bt, bt + d, side="left")
    runs = d > 0
    csr = np.bincount(at[runs], minlength=len(bt) + 1)
    live = np.bincount(at[runs & (binds["status"] == 0)], minlength=len(bt) + 1)
    return live, csr


def window_sums(cnt, batch):
    """Per bind index s: the expiries the resolver's window holds for the batch of `batch` pods that
    starts at s — those attached to pods s + 1 .. s + batch - 1 (the first pod's are the head)."""
    c = np.concatenate([[0], np.cumsum(cnt[:-1])])
    s = np.arange(len(cnt) - batch)
    return c[s + batch] - c[s + 1]


# ---- planting -------------------------------------------------------------------------------------
def bulk_layout(sizes, first=60):
    """Bursts on a bulk trace (pod i binds at tick i + 1): [(F, lo, hi)], members the pods
    [lo, hi) bound up to tick F - LEAD - 1, the burst pod F - 1 bound at tick F.  Consecutive burst
    ticks are at least 300 apart and CLEAR pods lie between a burst pod and the next members."""
    out, f = [], first
    for m in sizes:
        f += m + LEAD
        out.append((f, f - LEAD - m, f - LEAD))
        f += CLEAR
    return out


def plant(bt, bursts, rest=LONG):
    """Run lengths in ticks for pods with (predicted) bind ticks `bt` and bursts [(F, lo, hi)].
    Asserts that every burst pod carries exactly its members' expiries."""
    bt = np.asarray(bt, np.int64)
    m = len(bt)
    i = np.arange(m)
    run = np.where(i % 3 == 0, 1 + (i * 7) % 12, rest).astype(np.int64)
    member = np.zeros(m, bool)
    for f, lo, hi in bursts:
        assert 0 <= lo < hi <= m and not member[lo:hi].any() and (bt[lo:hi] < f).all(), (f, lo, hi)
        run[lo:hi] = f - bt[lo:hi]
        member[lo:hi] = True
    carriers = np.array([np.searchsorted(bt, f) for f, _, _ in bursts])
    assert (carriers < m).all() and len(set(carriers.tolist())) == len(bursts)
    at = np.searchsorted(bt, bt + run)
    run[~member & np.isin(at, carriers)] = LONG   # no background pod ends on a burst's pod
    for (f, lo, hi), c in zip(bursts, carriers):  # ... and none within a batch of a QUIET burst's pod
        if hi - lo in QUIET:
            run[~member & (np.abs(at - c) <= BIG_MAX_B)] = LONG
    at = np.searchsorted(bt, bt + run)
    for (f, lo, hi), c in zip(bursts, carriers):
        assert (at == c).sum() == hi - lo and (at[lo:hi] == c).all(), (f, lo, hi)
    return run


def _quarter(tr, div=4):
    """cpu and memory requests divided by `div`: quartered, every pod of the plan fits the cluster at once."""
    p = tr["pods"]
    p["req"][:, :2] //= div
    p["phase_use"][:, :2] //= div
    return tr


def _case(tr, run, bt, bursts, parts=None, pauses=()):
    set_run_ticks(tr, run)
    m = tr["pods"]["m"]
    return dict(tr=tr, enc=encoded(tr), run=np.asarray(run, np.int64), bt=np.asarray(bt, np.int64),
                bursts=tuple(bursts), parts=parts or ((0, 0, m),), pauses=tuple(pauses), ticks=int(bt[-1]) + 50)


def _bulk_case(n_nodes, sizes, div=4, rest=LONG, **kw):
    bursts = bulk_layout(sizes)
    m = bursts[-1][0] + CLEAR + 60
    tr = small_trace(11, n_nodes=n_nodes, n_pods=m, taints=False, selectors=False, tolerations=False, **kw)
    bt = np.arange(1, m + 1)
    return _case(_quarter(tr, div), plant(bt, bursts, rest), bt, bursts)


def _gap_case():
    """Arrivals 0-2 ticks apart with a pause of GAP_PAUSE ticks after each burst's members; the burst
    ends GAP_INTO ticks into the pause, so its expiries attach to the first pod after the idle ticks."""
    firsts, c = [], 100
    for m in GAP_BURSTS:
        c += m + 150
        firsts.append(c)            # the first pod after the pause
    n = firsts[-1] + 300
    tr = _quarter(small_trace(28, n_nodes=3000, n_pods=n, taints=False, selectors=False, tolerations=False,
                              arrival="stream"))
    arr = tr["pods"]["arrival"]
    bt = np.zeros(n, np.int64)
    bursts, pauses, prev = [], [], 0
    for i in range(n):
        if i in firsts:             # the queue has drained GAP_PAUSE ticks before this pod arrives
            arr[i:] += max(prev + GAP_PAUSE + 1 - arr[i], 0)
            m = GAP_BURSTS[firsts.index(i)]
            bursts.append((int(prev) + GAP_INTO, i - 5 - m, i - 5))
            pauses.append((int(prev) + 1, int(arr[i]) - 1))
        prev = bt[i] = max(prev + 1, arr[i])
    return _case(tr, plant(bt, bursts), bt, bursts, pauses=pauses)


def _pending_case(sizes):
    """Parts submitted one after another, each only once every earlier pod is bound and 100 ticks
    have passed: a burst of its last members ends 50 ticks after a part's last bind, with nothing
    queued.  parts: (tick at which the part is submitted, first pod, end pod)."""
    parts, bursts, bt, lo, tick = [], [], [], 0, 0
    for m in sizes + (None,):
        k = 300 if m is None else m + 150
        parts.append((tick, lo, lo + k))
        bt += list(range(tick + 1, tick + k + 1))
        if m is not None:
            bursts.append((tick + k + 50, lo + k - 5 - m, lo + k - 5))
        lo, tick = lo + k, tick + k + 100
    tr = _quarter(small_trace(11, n_nodes=3000, n_pods=lo, taints=False, selectors=False, tolerations=False))
    return _case(tr, plant(bt, bursts), bt, bursts, parts=tuple(parts))


_BUILD = {
    "bursts3k": lambda: _bulk_case(3000, BURSTS),
    "bursts3k_refused": lambda: _bulk_case(REFUSED_NODES, REFUSED_BURSTS, div=1, gpu_absent_p=0.0),
    "gap": _gap_case,
    "pending16": lambda: _pending_case((16,)),
    "pending17_600": lambda: _pending_case((17, 600)),
    "bursts66k": lambda: _bulk_case(PIPE_NODES, PIPE_BURSTS),
    "small": lambda: _small_case(),
}


def _small_case():
    """bursts3k's plan up to the SMALL_LAST burst on a cluster of the small class."""
    return _bulk_case(SMALL_NODES, BURSTS[:BURSTS.index(SMALL_LAST) + 1])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(tr, enc, run, bt, bursts [(F, lo, hi)], parts, pauses, ticks); built once, never changed."""
    return _BUILD[name]()


# ---- step plans -----------------------------------------------------------------------------------
TICKS_BURSTS = (16, 17, 257)


def plan(name, which):
    """Step lengths.  `whole`: one step (per part).  `head`: a step ends at F - 1 for every burst tick
    F (the burst pod is a pass's first pod).  `mid`: a step ends at F - MID, and the step after it is
    192 ticks (the burst pod is the MID-th pod of a pass; the 192 pods are one default batch of the
    chunk resolver unless the window cuts it).  `ticks`: one-tick steps from F - 3 to F + 3 around
    the TICKS_BURSTS bursts.  `pause` (gap): a step ends GAP_INTO + 50 ticks into every pause.
    `parts` (pending): per part, a step to 100 ticks past its last bind.  `group` (small): the steps
    of group_cases.CHUNKS, which the other member of its group takes, then the rest."""
    c = case(name)
    ends = []
    for f, lo, hi in c["bursts"]:
        if which == "head":
            ends.append(f - 1)
        elif which == "mid":
            ends += [f - MID, f - MID + 192]
        elif which == "ticks" and hi - lo in TICKS_BURSTS:
            ends += list(range(f - 4, f + 4))
        elif which == "pause":
            ends.append(f + 50)
    if which == "parts":
        ends = [t for t, _, _ in c["parts"][1:]]
    elif which == "group":
        from group_cases import CHUNKS
        ends = [int(t) for t in np.cumsum(CHUNKS)]
    else:
        assert which in ("whole", "head", "mid", "ticks", "pause"), which
    ends.append(c["ticks"])
    assert ends == sorted(set(ends))
    return tuple(int(k) for k in np.diff([0] + ends))


# ---- the oracle's runs, once each --------------------------------------------------------------------
def threads():
    return int(os.environ.get("OMP_NUM_THREADS") or 0) or min(os.cpu_count() or 1, 16)


@functools.lru_cache(maxsize=None)
def reference(name, mode, which):
    """The oracle's run of a case over a plan.  Per step: dict(k, binds, rc, usage, tick, probe) —
    `probe` is (pod, feasible, score) of the next pod as the oracle evaluates it after the step (and
    after the submit of a part that goes in at that tick), None when nothing is queued.  Nothing in
    it is changed afterwards."""
    c = case(name)
    tr = c["tr"]
    ora = make_oracle(tr, mode)
    if tr["nodes"]["n"] > 10_000:
        ora.set_threads(threads())
    parts = {t: (lo, hi) for t, lo, hi in c["parts"]}
    whole = len(parts) == 1

    def submit(t):
        if t in parts:
            ora.submit(tr if whole else tracegen.slice_pods(tr, *parts[t]))
            return parts[t][1]
        return None
    submitted, bound, tick, steps = submit(0), 0, 0, []
    for k in plan(name, which):
        b, rc = ora.step(k, cap=k)
        assert rc == 0, (name, mode, which, rc)
        bound += len(b["pod"])
        tick += k
        st = dict(k=k, binds=b, rc=rc, usage=ora.usage().copy(), tick=tick, probe=None, queued=submitted - bound)
        submitted = submit(tick) or submitted
        if bound < submitted:
            st["probe"] = (bound,) + ora.eval(bound)
        steps.append(st)
    ora.close()
    return steps


def all_binds(name, mode=MODE, which="whole"):
    steps = reference(name, mode, which)
    return {f: np.concatenate([s["binds"][f] for s in steps]) for f in ("pod", "node", "tick", "status")}


def burst_counts(name, mode=MODE, which="whole"):
    """Per burst of the case: (planned members, live count, CSR count, members bound OverCapacity)
    at the burst's pod in the oracle's run."""
    c = case(name)
    b = all_binds(name, mode, which)
    live, csr = attached(b, c["run"])
    out = []
    for f, lo, hi in c["bursts"]:
        at = int(np.searchsorted(b["tick"], f))
        refused = int((b["status"][np.isin(b["pod"], np.arange(lo, hi))] != 0).sum())
        out.append((hi - lo, int(live[at]), int(csr[at]), refused))
    return out
