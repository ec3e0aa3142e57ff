"""The inputs of tests/test_list_merge_gpu.py (merge_cl's score-class list merge on the engine against
the oracle), pinned on the oracle alone by tests/test_list_merge_shapes.py.

Node counts put the merge at each of its list-to-thread shapes (256-node scan blocks, 256 merge
threads up to 1,024 blocks): 300 nodes = 2 blocks, 16,640 = 65 (one list per thread, two waves),
70,144 = 274 (two lists per thread), 262,400 = 1,025 (1,024 threads, the pruned form).  "same" makes
every node identical, so every feasible node of a pod is in one score class until it is bound;
"mixed" runs with scorer weights (100, 1) on small nodes of six capacity pairs (the trace's largest
pods just fit) with a ladder of 36 nodes among them, spread over the whole index range, whose cpu and
memory are 1.3 .. 8 times that, every pair of factors once: a larger pod's best nodes are ladder nodes
in many thin classes (MIXED_POD: a pod whose best 12 nodes span >= 8 classes at every node count).

Nothing here imports the engine.  Traces and oracle runs are built once per process and never changed
afterwards.
"""
from __future__ import annotations

import functools

import numpy as np

from harness import make_oracle, oracle_run
from kubesim_amd import tracegen

NODE_COUNTS = (300, 16_640, 70_144, 262_400)
PODS = 520
STEPS = (1, 193, PODS - 194)
MODES = {"same": (1, 7, ((1, 1, 0), (2, 1, 0))), "mixed": (1, 7, ((1, 100, 0), (2, 1, 0)))}
SEED = 41
LADDER = 36
LADDER_X = np.array([13, 17, 22, 30, 45, 80], dtype=np.int64)  # tenths
MIXED_POD = 48
PHASE_SHRINK = 64  # phases of 1 .. 57 ticks: expiries all through a 520-tick run

# the dense-expiry run: 256-pod batches whose windows hold more than 512 E nodes
DENSE_NODES, DENSE_LONG, DENSE_PODS = 20_000, 3000, 4500
# (a step ends where the resolver leaves it: the second 366-pod step ends on an overlapped batch whose
# window holds 559 E nodes)
DENSE_STEPS = (DENSE_LONG, 366, 366, 516, 252)
DENSE_BATCH = 256


def _plain(n_nodes, n_pods):
    return tracegen.synth_trace(n_nodes, n_pods, SEED, taints=False, labels=False, tolerations=False,
                                selectors=False, gpu_absent_p=0.0)


@functools.lru_cache(maxsize=None)
def trace(n_nodes, kind):
    tr = _plain(n_nodes, PODS)
    nd, p = tr["nodes"], tr["pods"]
    if kind == "same":
        nd["alloc"][:] = nd["alloc"][0]
    else:
        i = np.arange(n_nodes, dtype=np.int64)
        gi = tracegen.GI * tracegen.MILLI
        step = max(1, n_nodes // LADDER)
        rung = (i % step == 7 % step) & (i // step < LADDER)
        j = np.minimum(i // step, LADDER - 1)
        nd["alloc"][:, tracegen.CPU] = np.where(rung, 820 * LADDER_X[j % 6], 8200 + 100 * (i % 3))
        nd["alloc"][:, tracegen.MEM] = np.where(rung, 33 * LADDER_X[j // 6] * gi // 10, (33 + i % 2) * gi)
    p["phase_sec"][:] = np.maximum(10, p["phase_sec"] // PHASE_SHRINK)
    return tr


@functools.lru_cache(maxsize=None)
def oracle_steps(n_nodes, kind):
    """Per step of STEPS: (the oracle's binds, error code, usage after the step)."""
    tr = trace(n_nodes, kind)
    ora = make_oracle(tr, MODES[kind])
    ora.set_threads(8)
    ora.submit(tr)
    out = []
    for k in STEPS:
        b, rc = oracle_run(ora, k)
        out.append((b, rc, ora.usage().copy()))
    ora.close()
    return out


def top_classes(n_nodes, kind, after, length=12):
    """The score classes among the best `length` feasible nodes of the pod scheduled after `after`
    ticks, on the oracle's state then."""
    tr = trace(n_nodes, kind)
    ora = make_oracle(tr, MODES[kind])
    ora.set_threads(8)
    ora.submit(tr)
    b, rc = oracle_run(ora, after)
    assert rc == 0 and len(b["pod"]) == after
    feas, score = ora.eval(after)
    ora.close()
    s = np.sort(score[feas != 0])[::-1][:length]
    return len(s), len(np.unique(s))


@functools.lru_cache(maxsize=None)
def dense_trace():
    """One pod binds per tick.  Pod i < DENSE_LONG runs until about tick DENSE_LONG + 2 i / 3, so three
    of them expire every two ticks while the later pods (which outlive the run) are scheduled: a
    256-pod batch's window holds about 384 slots on nodes of pre-batch pods, and the previous batch's
    bound nodes join them in E.  Taints, labels, tolerations and selectors as in the C3 trace: the
    pods' candidate lists differ, so batches commit most of their pods and a step often ends on an
    overlapped batch's window."""
    tr = tracegen.synth_trace(DENSE_NODES, DENSE_PODS, SEED, taints=True, labels=True, tolerations=True,
                              selectors=True)
    p = tr["pods"]
    nph = np.diff(p["phase_off"]).astype(np.int64)
    owner = np.repeat(np.arange(DENSE_PODS), nph)
    ticks = np.where(owner < DENSE_LONG, DENSE_LONG - owner // 3, DENSE_PODS)
    p["phase_sec"][:] = np.maximum(10, tr["tick_seconds"] * ticks // nph[owner])
    return tr


@functools.lru_cache(maxsize=None)
def dense_oracle_steps():
    tr = dense_trace()
    ora = make_oracle(tr, MODES["same"])
    ora.set_threads(8)
    ora.submit(tr)
    out = []
    for k in DENSE_STEPS:
        b, rc = oracle_run(ora, k)
        out.append((b, rc, ora.usage().copy()))
    ora.close()
    return out

