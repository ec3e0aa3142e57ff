"""Python handle over the C-ABI (include/ks_engine.h): the device scheduling engine.

``Engine`` mirrors the reference's engine surface (kubesim/kubesim.go):

=====================  ==============================================================
reference              here
=====================  ==============================================================
NewKubeSim             ``Engine(tick_seconds, filter_mode, filters, scorers)`` +
                       ``load_nodes`` (kubesim/kubesim.go:32-61)
RegisterFilter /       ``filters`` bits / ``scorers`` list, fixed at creation
RegisterScorer         (kubesim/kubesim.go:78-86); built-in device plugins only
submit (Submitter)     ``submit`` (kubesim/kubesim.go:126-139)
Run                    ``step(ticks)`` — advances the tick loop (kubesim/kubesim.go:90-123)
api.Filter / Scorer    ``filter(pod)`` / ``score(pod)``
scheduleOne's trace    ``filter_at(pod)`` / ``score_at(pod)`` for bound pods; node state at a
                       past tick: ``requested_at``, ``cluster_series``, ``node_peaks``
Node.CreatePod's test  ``headroom_at`` / ``headroom_series``: how many more pods of a shape
                       each node would admit at a past tick (kubesim/node/node.go:44-47)
scheduleOne, what-if   ``place_at``: where k more pods would be bound at a past tick, on a
                       private copy of the state (kubesim/kubesim.go:143-225);
                       ``drain_at``: where the pods running on a node set would go if the
                       set left k.nodes (kubesim/kubesim.go:168-206); ``removable_at``: that
                       answer for each of m candidate nodes on its own;
                       ``consolidate_at``: the candidates one after another as a scale-down
                       pass handles them, removals kept, failed attempts rolled back;
                       ``gang_at``: ``place_at``'s pods in groups admitted all-or-nothing
                       (or from ``min_ok`` members up), in queue order;
                       ``scale_up_at``:
                       ``place_at`` on the cluster plus up to M empty nodes of a node-group
                       template, for each of G templates on its own
=====================  ==============================================================

Errors come back as :class:`KsError` with the reference's kind (``InvalidArgument`` /
``NotFound``); binds made before an aborting error are still returned by ``step``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import KsBind, KsConfig, KsStepStats


class KsError(RuntimeError):
    def __init__(self, code: int, msg: str, binds=None):
        super().__init__(f"{_lib.STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code
        self.kind = _lib.STATUS_NAMES.get(code, str(code))
        self.binds = binds


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


# ks_placement (include/ks_engine.h)
PLACEMENT_DTYPE = np.dtype([("node", np.int32), ("status", np.int32), ("score", np.int64), ("candidates", np.int64)])
assert PLACEMENT_DTYPE.itemsize == 24
# ks_eviction (include/ks_engine.h)
EVICTION_DTYPE = np.dtype([("pod", np.int64), ("from", np.int32), ("node", np.int32), ("status", np.int32),
                           ("pad", np.int32), ("score", np.int64), ("candidates", np.int64)])
assert EVICTION_DTYPE.itemsize == 40
# ks_removal (include/ks_engine.h)
REMOVAL_DTYPE = np.dtype([("node", np.int32), ("evicted", np.int32), ("ok", np.int32), ("over_capacity", np.int32),
                          ("not_found", np.int32), ("removable", np.int32), ("first_row", np.int64)])
assert REMOVAL_DTYPE.itemsize == 32
# ks_consolidation (include/ks_engine.h)
CONSOLIDATION_DTYPE = np.dtype([("node", np.int32), ("evicted", np.int32), ("outcome", np.int32), ("rows", np.int32),
                                ("block_status", np.int32), ("pad", np.int32), ("first_row", np.int64)])
assert CONSOLIDATION_DTYPE.itemsize == _lib.KS_CONSOLIDATION_BYTES
# ks_gang (include/ks_engine.h)
GANG_DTYPE = np.dtype([("first", np.int32), ("size", np.int32), ("outcome", np.int32), ("tried", np.int32),
                       ("ok", np.int32), ("over_capacity", np.int32), ("not_found", np.int32),
                       ("block_status", np.int32)])
assert GANG_DTYPE.itemsize == _lib.KS_GANG_BYTES
# ks_scale_option, ks_scale_result (include/ks_engine.h)
SCALE_OPTION_DTYPE = np.dtype([("alloc", np.int64, (4,)), ("taint", np.uint64), ("label", np.uint64),
                               ("max_nodes", np.int32), ("pad", np.int32)])
SCALE_RESULT_DTYPE = np.dtype([("ok", np.int32), ("over_capacity", np.int32), ("not_found", np.int32),
                               ("on_new", np.int32), ("nodes_used", np.int32), ("first_unplaced", np.int32),
                               ("path", np.int32), ("pad", np.int32)])
assert SCALE_OPTION_DTYPE.itemsize == 56 and SCALE_RESULT_DTYPE.itemsize == 32


def _config(tick_seconds, filter_mode, filters, scorers, device, batch_pods, engine_flags):
    cfg = KsConfig()
    cfg.abi_version = _lib.KS_ABI_VERSION
    cfg.tick_seconds = tick_seconds
    cfg.filter_mode = filter_mode
    cfg.filters = filters
    cfg.n_scorers = len(scorers)
    for i, (k, w, v) in enumerate(scorers):
        cfg.scorers[i].kind, cfg.scorers[i].weight, cfg.scorers[i].value = k, w, v
    cfg.device = device
    cfg.batch_pods = batch_pods
    cfg.engine_flags = engine_flags
    return cfg


class Engine:
    """``engine_flags``: ``_lib.KS_ENGINE_*`` bits (include/ks_engine.h) — A/B and test switches that
    never change the binds.  ``KS_ENGINE_SMALL_E`` is test-only: the batch window's changed-node set
    overflows at 128 nodes instead of 2,048, so small clusters reach the rescan path."""

    def __init__(self, *, tick_seconds=10, filter_mode=_lib.KS_FILTER_REFERENCE_LITERAL, filters=0,
                 scorers=((_lib.KS_SCORER_CONST, 1, 1),), device=0, batch_pods=0, engine_flags=0,
                 _group=None):
        L = _lib.load()
        self._group = _group
        cfg = _config(tick_seconds, filter_mode, filters, scorers, device, batch_pods, engine_flags)
        h = C.c_void_p()
        if _group is None:
            rc = L.ks_create(C.byref(cfg), C.byref(h))
        else:
            rc = L.ks_group_add(_group.h, C.byref(cfg), C.byref(h))
        if rc != _lib.KS_OK:
            raise KsError(rc, "ks_create / ks_group_add rejected the configuration")
        self._L = L
        self.h = h
        self.n = 0
        self._submitted = 0

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_group", None) is None:  # a group's members die with the group
                self._L.ks_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, binds=None):
        if rc != _lib.KS_OK:
            raise KsError(rc, self._L.ks_last_error(self.h).decode(), binds)

    # -- node sharding ------------------------------------------------------
    def shard(self, world: int, rank: int, comm_id: bytes | None = None, vshards: int = 1):
        """Scan only this rank's node range; candidates are all-gathered per batch over RCCL
        (comm_id from :func:`comm_unique_id` on rank 0, broadcast by the caller).  Before
        ``load_nodes``.  ``vshards`` > 1 splits the range further (one-GPU testing)."""
        buf = None
        if comm_id is not None:
            if len(comm_id) != _lib.KS_COMM_ID_BYTES:
                raise ValueError("comm_id must be KS_COMM_ID_BYTES long")
            buf = (C.c_uint8 * _lib.KS_COMM_ID_BYTES).from_buffer_copy(comm_id)
        self._check(self._L.ks_shard(self.h, world, rank, buf, vshards))

    def shard_host(self, world: int, rank: int, exchange: "LocalExchange", vshards: int = 1):
        """Node sharding with a host exchange instead of RCCL (ks_shard_host): ranks are engines
        driven by threads of this process, exchanging candidates through ``exchange``."""
        self._xchg = exchange  # keep alive
        self._check(self._L.ks_shard_host(self.h, world, rank, vshards, exchange.fn, exchange.h))

    # -- cluster / queue ---------------------------------------------------------------------
    def load_nodes(self, alloc, taint, label):
        alloc = _c(alloc, np.int64).reshape(-1, 4)
        self.n = len(alloc)
        self._check(self._L.ks_load_nodes(self.h, self.n, _p(alloc), _p(_c(taint, np.uint64)),
                                          _p(_c(label, np.uint64))))

    def submit(self, pods: dict):
        """Append encoded pods (see kubesim_amd.encode.encode_pods).  ``key_id`` (optional,
        int64 per pod): interned namespace-name keys; absent/None = every pod its own key."""
        m = int(pods["m"])
        arrs = [_c(pods["arrival"], np.int64), _c(pods["req"], np.int64).reshape(-1, 3),
                _c(pods["keymask"], np.uint8), _c(pods["tol"], np.uint64), _c(pods["sel"], np.uint64),
                _c(pods["phase_off"], np.int32), _c(pods["phase_sec"], np.int32),
                _c(pods["phase_use"], np.int64).reshape(-1, 3), _c(pods["flags"], np.uint8)]
        keys = pods.get("key_id")
        if keys is not None:
            keys = _c(keys, np.int64)
        # the C side reads these lengths blindly: check them here
        per_pod = {"arrival": arrs[0], "req": arrs[1], "keymask": arrs[2], "tol": arrs[3], "sel": arrs[4],
                   "flags": arrs[8]}
        if keys is not None:
            per_pod["key_id"] = keys
        for name, a in per_pod.items():
            if len(a) != m:
                raise ValueError(f"pods[{name!r}] has {len(a)} rows, expected m = {m}")
        off = arrs[5]
        if len(off) != m + 1:
            raise ValueError(f"pods['phase_off'] has {len(off)} entries, expected m + 1 = {m + 1}")
        nf = int(off[-1]) if m else 0
        if m and (off[0] != 0 or (np.diff(off) < 0).any()):
            raise ValueError("pods['phase_off'] must start at 0 and be non-decreasing")
        if len(arrs[6]) < nf or len(arrs[7]) < nf:
            raise ValueError(f"phase arrays shorter than phase_off[-1] = {nf}")
        ptrs = [_p(a) for a in arrs] + [_p(keys) if keys is not None else None]
        self._check(self._L.ks_submit_pods(self.h, m, *ptrs))
        self._submitted += m

    # -- tick loop ---------------------------------------------------------------------------
    def step(self, ticks: int, cap: int | None = None):
        """Advance ``ticks`` ticks; returns binds as a structured numpy array
        (pod, node, status, tick).  ``cap`` defaults to the binds the step can make (at most one
        per tick and one per queued pod)."""
        if cap is None:
            cap = max(0, min(ticks, self.queued))
        out = (KsBind * max(cap, 1))()
        n = C.c_int64(0)
        rc = self._L.ks_step(self.h, ticks, out, cap, C.byref(n))
        k = min(n.value, cap)
        arr = np.frombuffer(out, dtype=np.dtype([("pod", "<i8"), ("node", "<i4"), ("status", "<i4"),
                                                 ("tick", "<i8")]), count=k).copy()
        self._check(rc, arr)
        return arr

    def filter(self, pod: int):
        mask = np.zeros(self.n, np.uint8)
        self._check(self._L.ks_filter(self.h, pod, _p(mask)))
        return mask

    def score(self, pod: int):
        score = np.zeros(self.n, np.int64)
        self._check(self._L.ks_score(self.h, pod, _p(score)))
        return score

    def usage(self):
        out = np.zeros((self.n, 3), np.int64)
        self._check(self._L.ks_usage(self.h, _p(out)))
        return out

    def usage_at(self, t: int):
        """Per-node usage [n][3] at any past tick 0 <= t <= the current tick."""
        out = np.zeros((self.n, 3), np.int64)
        self._check(self._L.ks_usage_at(self.h, t, _p(out)))
        return out

    def usage_digest(self, t_lo: int, t_hi: int):
        """[t_hi - t_lo][6] uint64: per tick Σ_n usage[n][k] (k < 3) and Σ_n mix(n) usage[n][k-3]."""
        out = np.zeros((max(t_hi - t_lo, 0), 6), np.uint64)
        self._check(self._L.ks_usage_digest(self.h, t_lo, t_hi, _p(out)))
        return out

    # -- scheduler state at past ticks (include/ks_engine.h, ks_requested_at ...) --------------
    def requested_at(self, t: int):
        """[n][4] int64 at any past tick 0 <= t <= the current tick: per node Σ requested cpu /
        memory / gpu (milli-units) and the running pods (kubesim/node/node.go:97-118)."""
        out = np.zeros((self.n, 4), np.int64)
        self._check(self._L.ks_requested_at(self.h, t, _p(out)))
        return out

    def filter_at(self, pod: int):
        """``filter(pod)`` as it was when the already-bound ``pod`` was scheduled."""
        mask = np.zeros(self.n, np.uint8)
        self._check(self._L.ks_filter_at(self.h, pod, _p(mask)))
        return mask

    def score_at(self, pod: int):
        """``score(pod)`` as it was when the already-bound ``pod`` was scheduled (-1 = no entry);
        its lowest-index argmax is the node the pod was bound to."""
        score = np.zeros(self.n, np.int64)
        self._check(self._L.ks_score_at(self.h, pod, _p(score)))
        return score

    def cluster_series(self, t_lo: int, t_hi: int):
        """[t_hi - t_lo][KS_SERIES_COLS] int64 per tick: running pods, Σ requested cpu / memory /
        gpu, pods bound Ok so far, bound OverCapacity so far, pending pods."""
        out = np.zeros((max(t_hi - t_lo, 0), _lib.KS_SERIES_COLS), np.int64)
        self._check(self._L.ks_cluster_series(self.h, t_lo, t_hi, _p(out)))
        return out

    def node_peaks(self, t_lo: int, t_hi: int):
        """[n][4] int64: per node and column the maximum of ``requested_at(t)`` over t_lo <= t < t_hi."""
        out = np.zeros((self.n, 4), np.int64)
        self._check(self._L.ks_node_peaks(self.h, t_lo, t_hi, _p(out)))
        return out

    # -- headroom (include/ks_engine.h, ks_headroom_at / ks_headroom_series) --------------------
    @staticmethod
    def _shapes(shapes: dict):
        """The shape arrays of a dict with encode.encode_pods' keys (req, keymask, tol, sel); a slice
        of an encoded pod set passes as it is."""
        req = _c(shapes["req"], np.int64).reshape(-1, 3)
        km, tol, sel = _c(shapes["keymask"], np.uint8), _c(shapes["tol"], np.uint64), _c(shapes["sel"], np.uint64)
        k = len(req)
        if not (len(km) == len(tol) == len(sel) == k):
            raise ValueError(f"shapes: req has {k} rows, keymask {len(km)}, tol {len(tol)}, sel {len(sel)}")
        return k, req, km, tol, sel

    def headroom_at(self, t: int, shapes: dict, per_node: bool = False):
        """How many more pods of each shape fit at tick t (Node.CreatePod's admission test,
        kubesim/node/node.go:44-47, applied repeatedly).  Returns [k][KS_HEADROOM_COLS] int64: Σ over
        nodes of the count, nodes with a count >= 1, the largest count, its lowest node (-1 if none),
        the eligible nodes limited by cpu / memory / gpu / pods, the ineligible nodes; with
        ``per_node`` also the [k][n] int32 counts."""
        k, req, km, tol, sel = self._shapes(shapes)
        out = np.zeros((k, _lib.KS_HEADROOM_COLS), np.int64)
        pn = np.zeros((k, self.n), np.int32) if per_node else None
        self._check(self._L.ks_headroom_at(self.h, t, k, _p(req), _p(km), _p(tol), _p(sel), _p(out),
                                           _p(pn) if per_node else None))
        return (out, pn) if per_node else out

    def headroom_series(self, t_lo: int, t_hi: int, shapes: dict):
        """[t_hi - t_lo][k][2] int64: columns 0 and 1 of ``headroom_at`` at every tick t_lo <= t < t_hi."""
        k, req, km, tol, sel = self._shapes(shapes)
        out = np.zeros((max(t_hi - t_lo, 0), k, 2), np.int64)
        self._check(self._L.ks_headroom_series(self.h, t_lo, t_hi, k, _p(req), _p(km), _p(tol), _p(sel), _p(out)))
        return out

    # -- placement preview (include/ks_engine.h, ks_place_at) -----------------------------------
    def place_at(self, t: int, shapes: dict, shape_of=None, after: bool = False):
        """Where k more pods would be bound at tick t: scheduleOne (kubesim/kubesim.go:143-225) for
        the pods one after another on a private copy of the state at t — no engine state changes.
        ``shapes`` as for ``headroom_at``; pod j has shape ``shape_of[j]`` (None: one pod per shape,
        in order).  Returns a dict of arrays over the pods — ``node`` (-1: none), ``status``
        (KS_POD_OK, KS_POD_OVER_CAPACITY, KS_PLACE_NOT_FOUND), ``score`` (-1: none), ``candidates``
        — plus ``info`` (rounds, placed Ok, placed OverCapacity, not found) and ``after``: with
        ``after=True`` the [n][4] requested state at t plus every Ok placement, else None."""
        ns, req, km, tol, sel = self._shapes(shapes)
        so = None if shape_of is None else _c(shape_of, np.int32)
        k = ns if so is None else len(so)
        rec = np.zeros(max(k, 1), PLACEMENT_DTYPE)
        aft = np.zeros((self.n, 4), np.int64) if after else None
        info = np.zeros(_lib.KS_PLACE_INFO, np.int64)
        self._check(self._L.ks_place_at(self.h, t, ns, _p(req), _p(km), _p(tol), _p(sel), k,
                                        None if so is None else _p(so), _p(rec), _p(aft) if after else None,
                                        _p(info)))
        rec = rec[:k]
        return dict(node=rec["node"].copy(), status=rec["status"].copy(), score=rec["score"].copy(),
                    candidates=rec["candidates"].copy(), after=aft, info=info)

    # -- drain preview (include/ks_engine.h, ks_drain_at) ---------------------------------------
    def drain_at(self, t: int, nodes, after: bool = False):
        """Where the pods running on ``nodes`` at tick t would go if those nodes left the cluster:
        the drained nodes are in no Filter loop and no score map (kubesim/kubesim.go:168-206), their
        running pods are evicted and handed in FIFO order to scheduleOne on a private copy of the
        state — no engine state changes.  ``nodes``: distinct node indices.  Returns a dict of arrays
        over the evicted pods — ``pod``, ``from_node``, ``node`` (-1: none), ``status``, ``score``
        (-1: none), ``candidates`` — plus ``info`` (rounds, re-placed Ok, OverCapacity, not found,
        segments, drained nodes that had no running pod) and ``after``: with ``after=True`` the
        [n][4] requested state at t without the drained nodes plus every Ok re-placement, else None.
        It makes the sizing call itself."""
        nd = _c(nodes, np.int32).reshape(-1)
        n_out = C.c_int64(0)
        aft = np.zeros((self.n, 4), np.int64) if after else None
        info = np.zeros(_lib.KS_DRAIN_INFO, np.int64)
        pa, pi = (_p(aft) if after else None), _p(info)
        rc = self._L.ks_drain_at(self.h, t, len(nd), _p(nd), None, 0, C.byref(n_out), pa, pi)
        rec = np.zeros(max(n_out.value, 1), EVICTION_DTYPE)
        if rc == _lib.KS_ERANGE and 0 < n_out.value <= _lib.KS_DRAIN_MAX_PODS:
            rc = self._L.ks_drain_at(self.h, t, len(nd), _p(nd), _p(rec), n_out.value, C.byref(n_out), pa, pi)
        self._check(rc)
        rec = rec[:n_out.value]
        return dict(pod=rec["pod"].copy(), from_node=rec["from"].copy(), node=rec["node"].copy(),
                    status=rec["status"].copy(), score=rec["score"].copy(), candidates=rec["candidates"].copy(),
                    after=aft, info=info)

    # -- removal scan (include/ks_engine.h, ks_removable_at) ------------------------------------
    def removable_at(self, t: int, nodes, rows: bool = False):
        """Which of ``nodes`` could each be taken out on its own at tick t: for candidate c the answer
        of ``drain_at(t, [c])`` — candidates are independent, no engine state changes.  ``nodes``:
        distinct node indices.  Returns a dict of arrays over the candidates, in the caller's order —
        ``node``, ``evicted`` (pods running on it), ``ok`` / ``over_capacity`` / ``not_found`` (their
        re-placements), ``removable`` (bool: every pod re-bound Ok, also when none runs there),
        ``first_row`` — plus ``info`` (segments, candidates resolved by the batched kernel, candidates
        answered through the single-drain path, candidates with no running pod, removable candidates,
        evicted pods) and ``rows``: with ``rows=True`` ``drain_at``'s arrays over the evicted pods
        (``pod``, ``from_node``, ``node``, ``status``, ``score``, ``candidates``), the candidates'
        rows concatenated in the caller's order, candidate j's at ``first_row[j]``; else None.  It
        makes the sizing call itself."""
        nd = _c(nodes, np.int32).reshape(-1)
        m = len(nd)
        out = np.zeros(max(m, 1), REMOVAL_DTYPE)
        n_rows = C.c_int64(0)
        info = np.zeros(_lib.KS_REMOVABLE_INFO, np.int64)
        if rows:
            # a one-row buffer first: KS_ERANGE comes back with the count as soon as the gather has it
            rec = np.zeros(1, EVICTION_DTYPE)
            rc = self._L.ks_removable_at(self.h, t, m, _p(nd), _p(out), _p(rec), 1, C.byref(n_rows), _p(info))
            if rc == _lib.KS_ERANGE and 1 < n_rows.value <= _lib.KS_DRAIN_MAX_PODS:
                rec = np.zeros(n_rows.value, EVICTION_DTYPE)
                rc = self._L.ks_removable_at(self.h, t, m, _p(nd), _p(out), _p(rec), n_rows.value, C.byref(n_rows),
                                             _p(info))
        else:
            rc = self._L.ks_removable_at(self.h, t, m, _p(nd), _p(out), None, 0, C.byref(n_rows), _p(info))
        self._check(rc)
        out = out[:m]
        res = {f: out[f].copy() for f in ("node", "evicted", "ok", "over_capacity", "not_found", "first_row")}
        res["removable"] = out["removable"] != 0
        res["info"] = info
        res["rows"] = None
        if rows:
            rec = rec[:n_rows.value]
            res["rows"] = dict(pod=rec["pod"].copy(), from_node=rec["from"].copy(), node=rec["node"].copy(),
                               status=rec["status"].copy(), score=rec["score"].copy(),
                               candidates=rec["candidates"].copy())
        return res

    # -- consolidation preview (include/ks_engine.h, ks_consolidate_at) --------------------------
    def consolidate_at(self, t: int, nodes, rows: bool = True, after: bool = False):
        """Which of ``nodes`` a scale-down pass would remove at tick t when it handles them in the
        given order on one private state: a candidate whose running pods are all re-bound Ok is
        removed and its placements stay; an attempt that meets a pod not bound Ok is rolled back;
        a node that received a moved pod is not tried — no engine state changes.  ``nodes``: distinct
        node indices.  Returns a dict of arrays over the candidates, in the caller's order — ``node``,
        ``evicted`` (pods running on it), ``outcome`` (KS_CONSOLIDATE_BLOCKED / _REMOVED /
        _DESTINATION), ``n_rows`` (rows written for it), ``block_status``, ``first_row`` — plus
        ``evicted_total``, ``info`` (rounds, removed, blocked, destinations, candidates decided
        through the single path, pods moved), ``rows``: with ``rows=True`` ``drain_at``'s arrays over
        the rows (a removed candidate's pods, a blocked one's up to the blocking pod), candidate j's
        at ``first_row[j]``, else None; and ``after``: with ``after=True`` the [n][4] final private
        state, else None.  It makes the sizing call itself."""
        nd = _c(nodes, np.int32).reshape(-1)
        m = len(nd)
        out = np.zeros(max(m, 1), CONSOLIDATION_DTYPE)
        n_ev, n_rows = C.c_int64(0), C.c_int64(0)
        aft = np.zeros((self.n, 4), np.int64) if after else None
        info = np.zeros(_lib.KS_CONSOLIDATE_INFO, np.int64)
        pa = _p(aft) if after else None
        if rows:
            # a one-row buffer first: KS_ERANGE comes back with the count as soon as the gather has it
            rec = np.zeros(1, EVICTION_DTYPE)
            rc = self._L.ks_consolidate_at(self.h, t, m, _p(nd), _p(out), _p(rec), 1, C.byref(n_ev), C.byref(n_rows),
                                           pa, _p(info))
            if rc == _lib.KS_ERANGE and 1 < n_ev.value <= _lib.KS_DRAIN_MAX_PODS:
                rec = np.zeros(n_ev.value, EVICTION_DTYPE)
                rc = self._L.ks_consolidate_at(self.h, t, m, _p(nd), _p(out), _p(rec), n_ev.value, C.byref(n_ev),
                                               C.byref(n_rows), pa, _p(info))
        else:
            rc = self._L.ks_consolidate_at(self.h, t, m, _p(nd), _p(out), None, 0, C.byref(n_ev), C.byref(n_rows), pa,
                                           _p(info))
        self._check(rc)
        out = out[:m]
        res = {f: out[f].copy() for f in ("node", "evicted", "outcome", "block_status", "first_row")}
        res["n_rows"] = out["rows"].copy()
        res["evicted_total"] = n_ev.value
        res["info"] = info
        res["after"] = aft
        res["rows"] = None
        if rows:
            rec = rec[:n_rows.value]
            res["rows"] = dict(pod=rec["pod"].copy(), from_node=rec["from"].copy(), node=rec["node"].copy(),
                               status=rec["status"].copy(), score=rec["score"].copy(),
                               candidates=rec["candidates"].copy())
        return res

    # -- gang admission preview (include/ks_engine.h, ks_gang_at) --------------------------------
    def gang_at(self, t: int, shapes: dict, shape_of, first, min_ok=None, strict: bool = False, rows: bool = True,
                after: bool = False):
        """Which pod groups of a queue would be admitted at tick t, in the given order on one private
        state, and where their pods would be bound: gang g is pods ``first[g] .. first[g + 1] - 1`` of
        the k pods (``shapes`` / ``shape_of`` as for ``place_at``; ``first`` has m + 1 entries, from 0
        to k).  Its pods go to scheduleOne one after another as ``place_at`` would handle them; the
        attempt ends once more than ``size - min_ok[g]`` of them were not bound Ok (``min_ok`` None:
        all-or-nothing).  A gang with at least ``min_ok`` Ok pods is admitted and its placements stay;
        a blocked gang is rolled back; with ``strict`` every gang after the first blocked one is
        skipped — no engine state changes.  Returns a dict of arrays over the gangs — ``first``,
        ``size``, ``outcome`` (KS_GANG_BLOCKED / _ADMITTED / _SKIPPED), ``tried``, ``ok``,
        ``over_capacity``, ``not_found``, ``block_status`` — plus ``info`` (rounds, admitted, blocked,
        skipped, gangs decided through the single path, Ok pods of admitted gangs), ``rows``: with
        ``rows=True`` ``place_at``'s arrays over the k pods (an untried pod has status
        KS_GANG_NOT_TRIED), else None; and ``after``: with ``after=True`` the [n][4] final private
        state, else None."""
        ns, req, km, tol, sel = self._shapes(shapes)
        so = _c(shape_of, np.int32).reshape(-1)
        fi = _c(first, np.int32).reshape(-1)
        k, m = len(so), len(fi) - 1
        mo = None if min_ok is None else _c(min_ok, np.int32).reshape(-1)
        if mo is not None and len(mo) != m:
            raise ValueError(f"min_ok has {len(mo)} entries for {m} gangs")
        out = np.zeros(max(m, 1), GANG_DTYPE)
        rec = np.zeros(max(k, 1), PLACEMENT_DTYPE) if rows else None
        aft = np.zeros((self.n, 4), np.int64) if after else None
        info = np.zeros(_lib.KS_GANG_INFO, np.int64)
        self._check(self._L.ks_gang_at(self.h, t, ns, _p(req), _p(km), _p(tol), _p(sel), k, _p(so), m, _p(fi),
                                       None if mo is None else _p(mo), _lib.KS_GANG_STRICT if strict else 0, _p(out),
                                       _p(rec) if rows else None, _p(aft) if after else None, _p(info)))
        out = out[:max(m, 0)]
        res = {f: out[f].copy() for f in GANG_DTYPE.names}
        res["info"] = info
        res["after"] = aft
        res["rows"] = None
        if rows:
            rec = rec[:k]
            res["rows"] = dict(node=rec["node"].copy(), status=rec["status"].copy(), score=rec["score"].copy(),
                               candidates=rec["candidates"].copy())
        return res

    # -- scale-up preview (include/ks_engine.h, ks_scale_up_at) ---------------------------------
    def scale_up_at(self, t: int, shapes: dict, options, shape_of=None, rows: bool = False):
        """Where the pending pods would be bound at tick t if up to ``max_nodes`` empty nodes of a
        node-group template were appended to the cluster (at indices n .. n + max_nodes - 1), for each
        option on its own: by definition ``place_at`` on that extended cluster — options are
        independent, no engine state changes.  ``shapes`` / ``shape_of`` as for ``place_at``;
        ``options``: dicts (or a SCALE_OPTION_DTYPE array) with ``alloc`` [4] as ``load_nodes`` takes
        it, ``taint``, ``label`` and ``max_nodes``.  Returns a dict of arrays over the options —
        ``ok`` / ``over_capacity`` / ``not_found``, ``on_new`` (pods bound Ok to an appended node),
        ``nodes_used`` (appended nodes holding a pod), ``first_unplaced`` (-1: every pod bound Ok),
        ``path`` (0 batched kernel, 1 single path) — plus ``info`` (options decided by the batched
        kernel, options answered through the single path, options in which every pod was bound Ok,
        distinct shapes) and ``rows``: with ``rows=True`` ``place_at``'s arrays (``node``, ``status``,
        ``score``, ``candidates``), each [options][k]; a ``node`` >= n names appended node
        ``node - n``; else None."""
        ns, req, km, tol, sel = self._shapes(shapes)
        so = None if shape_of is None else _c(shape_of, np.int32)
        k = ns if so is None else len(so)
        if isinstance(options, np.ndarray) and options.dtype == SCALE_OPTION_DTYPE:
            opt = np.ascontiguousarray(options).reshape(-1)
        else:
            opt = np.zeros(len(options), SCALE_OPTION_DTYPE)
            for g, o in enumerate(options):
                opt[g]["alloc"] = _c(o["alloc"], np.int64).reshape(4)
                opt[g]["taint"], opt[g]["label"] = int(o.get("taint", 0)), int(o.get("label", 0))
                opt[g]["max_nodes"] = int(o["max_nodes"])
        m = len(opt)
        out = np.zeros(max(m, 1), SCALE_RESULT_DTYPE)
        rec = np.zeros(max(m * k, 1), PLACEMENT_DTYPE) if rows else None
        info = np.zeros(_lib.KS_SCALEUP_INFO, np.int64)
        self._check(self._L.ks_scale_up_at(self.h, t, ns, _p(req), _p(km), _p(tol), _p(sel), k,
                                           None if so is None else _p(so), m, _p(opt), _p(out),
                                           _p(rec) if rows else None, _p(info)))
        out = out[:m]
        res = {f: out[f].copy() for f in ("ok", "over_capacity", "not_found", "on_new", "nodes_used", "first_unplaced",
                                          "path")}
        res["info"] = info
        res["rows"] = None
        if rows:
            rec = rec[:m * k].reshape(m, k)
            res["rows"] = {f: rec[f].copy() for f in ("node", "status", "score", "candidates")}
        return res

    def pod_lookup(self, node: int, key_id: int):
        """Node.GetPod: FIFO index of the pod stored on ``node`` under ``key_id`` (KsError NotFound)."""
        q = C.c_int64(-1)
        self._check(self._L.ks_pod_lookup(self.h, node, key_id, C.byref(q)))
        return q.value

    def node_pods(self, node: int):
        """Node.GetPodList: FIFO indices of the pods stored on ``node`` (one per key)."""
        n = C.c_int64(0)
        self._check(self._L.ks_node_pods(self.h, node, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.int64)
        self._check(self._L.ks_node_pods(self.h, node, _p(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def pod_status(self, pod_lo: int = 0, n: int | None = None):
        """Pod.BuildStatus phases (kubesim/pod/pod.go:78-145) at the current tick: structured
        array (phase, node, start_tick, total_seconds); phases _lib.KS_PHASE_*."""
        n = (self._submitted - pod_lo) if n is None else n
        out = (_lib.KsPodInfo * max(n, 1))()
        self._check(self._L.ks_pod_status(self.h, pod_lo, n, out))
        dt = np.dtype([("phase", "<i4"), ("node", "<i4"), ("start_tick", "<i8"), ("total_seconds", "<i4"),
                       ("pad", "<i4")])
        return np.frombuffer(out, dtype=dt, count=n).copy()

    @property
    def tick(self):
        return self._L.ks_current_tick(self.h)

    @property
    def queued(self):
        return self._L.ks_queued_pods(self.h)

    def last_step_stats(self):
        s = KsStepStats()
        self._L.ks_last_step_stats(self.h, C.byref(s))
        return dict(step_ms=s.step_ms, scan_ms=s.scan_ms, resolve_ms=s.resolve_ms, launches=s.launches,
                    pods=s.pods, other_ms=s.other_ms)

    def last_step_kernels(self):
        """Per-kernel event times of the last profiled step (include/ks_engine.h ks_kernel_stats)."""
        s = _lib.KsKernelStats()
        self._check(self._L.ks_last_step_kernels(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in s._fields_}

    def debug_counters(self):
        out = np.zeros(32, np.int64)
        self._check(self._L.ks_debug_counters(self.h, _p(out)))
        return out

    def debug_invariants(self):
        """Between-step invariants (include/ks_engine.h ks_debug_invariants): slot marks left set,
        E-index marks left set (both must be 0), the most candidate slots a batch claimed, the staged
        slots."""
        out = np.zeros(4, np.int64)
        self._check(self._L.ks_debug_invariants(self.h, _p(out)))
        return dict(slot_marks=int(out[0]), e_marks=int(out[1]), nslot_hw=int(out[2]), slot_max=int(out[3]))

    def debug_window(self) -> bytes:
        """The raw batch window workspace (include/ks_engine.h ks_debug_window; diagnostics)."""
        n = C.c_int64(0)
        self._check(self._L.ks_debug_window(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self._check(self._L.ks_debug_window(self.h, buf, n.value, C.byref(n)))
        return buf.raw

    def debug_watch(self, pod: int):
        """Record pod's batch in the window workspace (a -DKS_BATCH_LOG diagnostic build only)."""
        self._check(self._L.ks_debug_watch(self.h, pod))

    def set_profiling(self, on: bool):
        self._L.ks_set_profiling(self.h, 1 if on else 0)


def engine_for_trace(trace, enc, **cfg):
    """Create an Engine loaded with an encoded trace's nodes."""
    eng = Engine(tick_seconds=trace["tick_seconds"], **cfg)
    eng.load_nodes(enc["alloc"], enc["taint"], enc["label"])
    return eng


def selftest(test: int = _lib.KS_SELFTEST_LR_MICRO, device: int = 0) -> int:
    """Run a device self-test (include/ks_engine.h, ks_selftest); returns the failure count."""
    L = _lib.load()
    n = C.c_int64(-1)
    rc = L.ks_selftest(device, test, C.byref(n))
    if rc != 0:
        raise KsError(rc, "ks_selftest failed")
    return n.value


def selftest_eval(cfg: dict, alloc, run, req, keymask, masks, variants: int, device: int = 0):
    """One (node, pod) case per row through the device evaluators (include/ks_engine.h,
    ks_selftest_eval).  cfg: filter_feeds, filters, has_scorers, w_lr, w_ba, const_total.
    Returns (total1 [KS_EVAL_TOTAL_COLS][n], tmax [KS_EVAL_PRUNE_COLS][n], live [same]) as uint32;
    only the columns whose bit `variants` sets are filled.  A batch outside a requested evaluator's
    domain raises KsError(KS_EINVAL)."""
    L = _lib.load()
    alloc, run, req = _c(alloc, np.int64), _c(run, np.int64), _c(req, np.int64)
    keymask, masks = _c(keymask, np.uint32), _c(masks, np.uint64)
    n = len(keymask)
    if alloc.shape != (n, 4) or run.shape != (n, 4) or req.shape != (n, 3) or masks.shape != (n, 4):
        raise ValueError("selftest_eval: alloc[n][4], run[n][4], req[n][3], keymask[n], masks[n][4]")
    c = _lib.KsEvalCfg(**{k: int(cfg[k]) for k in ("filter_feeds", "filters", "has_scorers", "w_lr", "w_ba",
                                                   "const_total")})
    total1 = np.zeros((_lib.KS_EVAL_TOTAL_COLS, n), np.uint32)
    tmax = np.zeros((_lib.KS_EVAL_PRUNE_COLS, n), np.uint32)
    live = np.zeros((_lib.KS_EVAL_PRUNE_COLS, n), np.uint32)
    rc = L.ks_selftest_eval(device, C.byref(c), n, _p(alloc), _p(run), _p(req), _p(keymask), _p(masks),
                            int(variants), _p(total1), _p(tmax), _p(live))
    if rc != 0:
        raise KsError(rc, "ks_selftest_eval failed")
    return total1, tmax, live


class LocalExchange:
    """An in-process all-gather for ``world`` engines sharded with :meth:`Engine.shard_host`
    (ks_local_allgather, include/ks_kubesim.h)."""

    def __init__(self, world: int):
        self._R = _lib.load_run()
        self.h = self._R.ks_local_exchange_create(world)
        if not self.h:
            raise ValueError("bad world size")
        self.fn = C.cast(self._R.ks_local_allgather, C.c_void_p)

    def abort(self):
        """End every current and later exchange with KS_EDEVICE (a rank failed before its
        deposit: the others would wait for it forever; ks_local_exchange_abort)."""
        if getattr(self, "h", None):
            self._R.ks_local_exchange_abort(self.h)

    def close(self):
        if getattr(self, "h", None):
            self._R.ks_local_exchange_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id for :meth:`Engine.shard` (create on rank 0 only)."""
    L = _lib.load()
    buf = (C.c_uint8 * _lib.KS_COMM_ID_BYTES)()
    rc = L.ks_comm_unique_id(buf)
    if rc != 0:
        raise KsError(rc, "ks_comm_unique_id failed")
    return bytes(buf)


class Group:
    """Independent what-if scenarios (BASELINE.json configs[3]) stepped together on one device:
    one launch per kernel for all members (include/ks_engine.h, ks_group_*)."""

    def __init__(self, max_scenarios: int, device: int = 0):
        self._L = _lib.load()
        h = C.c_void_p()
        rc = self._L.ks_group_create(device, max_scenarios, C.byref(h))
        if rc != _lib.KS_OK:
            raise KsError(rc, "ks_group_create failed")
        self.h = h
        self.device = device
        self.members = []

    def add(self, **cfg) -> Engine:
        """A member engine (same keyword configuration as :class:`Engine`)."""
        cfg.setdefault("device", self.device)
        e = Engine(_group=self, **cfg)
        self.members.append(e)
        return e

    def step(self, ticks: int, cap: int | None = None):
        """Advance every member ``ticks`` ticks.  Returns (binds, counts, statuses, stats):
        ``binds`` is one structured array (pod, node, status, tick) holding member i's binds at
        rows [i * cap, i * cap + counts[i]) — :meth:`split` cuts it per member."""
        S = len(self.members)
        if cap is None:  # at most one bind per tick and per queued pod of the longest queue
            cap = max(0, min(ticks, max((e.queued for e in self.members), default=0)))
        if getattr(self, "_out_n", -1) < S * cap:  # reused across steps (no per-step 10s of MB)
            self._out = (KsBind * max(S * cap, 1))()
            self._out_n = S * cap
        n = np.zeros(S, np.int64)
        st = np.zeros(S, np.int32)
        stats = KsStepStats()
        rc = self._L.ks_group_step(self.h, ticks, self._out, cap, _p(n), _p(st), C.byref(stats))
        if rc != _lib.KS_OK:
            raise KsError(rc, "ks_group_step failed")
        dt = np.dtype([("pod", "<i8"), ("node", "<i4"), ("status", "<i4"), ("tick", "<i8")])
        allb = np.frombuffer(self._out, dtype=dt, count=S * cap) if S * cap else np.zeros(0, dt)
        self._cap = cap
        self._full_counts = n
        return allb, np.minimum(n, cap), st, dict(step_ms=stats.step_ms, launches=stats.launches, pods=stats.pods)

    @property
    def full_counts(self):
        """The binds each member made in the last :meth:`step` as ``ks_group_step`` reported them
        (``n_out``): not clipped to ``cap``, so a member whose count exceeds ``cap`` lost rows."""
        return self._full_counts.copy()

    def split(self, binds, counts):
        """Per-member copies of the binds returned by :meth:`step`."""
        return [binds[i * self._cap:i * self._cap + int(c)].copy() for i, c in enumerate(counts)]

    def close(self):
        if getattr(self, "h", None):
            for e in self.members:
                e.h = None
            self._L.ks_group_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()
