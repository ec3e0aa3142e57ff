"""Interval reference for the past-tick queries: the scheduler state after every tick rebuilt from a
run's binds and the trace alone, vectorised (difference arrays and ``np.add.at``) so that runs of
tens of thousands of ticks cost milliseconds where oracle/pysim.py's PySim, which walks every pod a
node ever held at every tick, costs minutes.

The rules are the reference's:

* a pod bound Ok at tick b is running at tick t iff passed = (t - b) * tick_seconds is below S, the
  wrapping int32 sum of its phase seconds (Pod.IsRunning / totalSeconds, kubesim/pod/pod.go:67-69,
  148-162; pysim.py ``_total_seconds``): ticks [b, b + dur), dur = ceil(S / tick_seconds) if S > 0
  else 0.  A pod bound OverCapacity never runs;
* a node's requested state is the sum of its running pods' requests over the keys each pod names,
  plus their number (Node.totalResourceRequest / runningPodsNum, kubesim/node/node.go:97-118);
* a running pod uses what the first phase whose wrapped cumulative seconds exceed ``passed`` names
  (Pod.ResourceUsage, kubesim/pod/pod.go:47-65; pysim.py ``_usage``).

tests/test_state_ref.py proves it equal to PySim stepped tick by tick.  Everything is int64; the
callers' traces keep every sum far below 2^63.
"""
import numpy as np

OK, OVER = 0, 1


def _wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) % (1 << 32)) - (1 << 31)


def _masked(vals, has):
    vals = np.asarray(vals, np.int64).reshape(-1, 3)
    return np.where(((np.asarray(has, np.int64)[:, None] >> np.arange(3)) & 1) == 1, vals, 0)


def durations(tr):
    """Per pod of the trace: ticks it runs once bound Ok."""
    p, ts = tr["pods"], int(tr["tick_seconds"])
    off = np.asarray(p["phase_off"], np.int64)
    cs = np.concatenate([[0], np.cumsum(np.asarray(p["phase_sec"], np.int64))])
    S = _wrap32(cs[off[1:]] - cs[off[:-1]])       # a wrapping sum is the exact sum mod 2^32
    return np.where(S > 0, (S + ts - 1) // ts, 0)


class IntervalRef:
    """``binds``: dict of arrays pod, node, tick, status of a run that stopped with no error (every
    pod taken off the queue was bound).  ``submit_tick``: per pod of the trace the engine tick at
    which it was submitted (default 0); a pod waits from max(arrival, submit tick + 1)."""

    def __init__(self, tr, binds, submit_tick=None):
        p = tr["pods"]
        self.tr, self.ts, self.n, self.m = tr, int(tr["tick_seconds"]), int(tr["nodes"]["n"]), int(p["m"])
        pod = np.asarray(binds["pod"], np.int64)
        st = np.asarray(binds["status"], np.int64)
        assert ((st == OK) | (st == OVER)).all()
        self.bind_tick = np.asarray(binds["tick"], np.int64)      # every bind, FIFO order
        self.bind_status = st
        ok = st == OK
        self.pod, self.node, self.b = pod[ok], np.asarray(binds["node"], np.int64)[ok], self.bind_tick[ok]
        self.dur_all = durations(tr)
        self.dur = self.dur_all[self.pod]
        self.e = self.b + self.dur
        self.req = _masked(p["req"], p["req_has"])[self.pod]
        sub = np.zeros(self.m, np.int64) if submit_tick is None else np.asarray(submit_tick, np.int64)
        self.arrival = np.sort(np.maximum(np.asarray(p["arrival"], np.int64), sub + 1))

    # -- requested state ------------------------------------------------------------------------
    def _spread(self, t_lo, t_hi, node, a, z, vals):
        """[T][n][c] of per-node sums: row i of ``vals`` counts on ``node[i]`` for ticks [a[i], z[i])."""
        T = t_hi - t_lo
        d = np.zeros((T + 1, self.n, vals.shape[1]), np.int64)
        a, z = np.maximum(a, t_lo), np.minimum(z, t_hi)
        live = a < z
        np.add.at(d, (a[live] - t_lo, node[live]), vals[live])
        np.add.at(d, (z[live] - t_lo, node[live]), -vals[live])
        return np.cumsum(d[:T], axis=0)

    def window(self, t_lo, t_hi):
        """[t_hi - t_lo][n][4]: requested cpu / memory / gpu and running pods at ticks t_lo .. t_hi - 1."""
        vals = np.concatenate([self.req, np.ones((len(self.pod), 1), np.int64)], axis=1)
        return self._spread(t_lo, t_hi, self.node, self.b, self.e, vals)

    def at(self, t):
        """The [n][4] matrix at tick t alone."""
        run = (self.b <= t) & (t < self.e)
        out = np.zeros((self.n, 4), np.int64)
        np.add.at(out[:, :3], self.node[run], self.req[run])
        np.add.at(out[:, 3], self.node[run], 1)
        return out

    def peaks(self, t_lo, t_hi):
        return self.window(t_lo, t_hi).max(axis=0)

    def series(self, t_lo, t_hi):
        """The seven cluster_series columns: running pods, requested cpu / memory / gpu, bound Ok so
        far, bound OverCapacity so far, pending (arrived and still queued)."""
        w = self.window(t_lo, t_hi)
        ticks = np.arange(t_lo, t_hi)
        out = np.zeros((t_hi - t_lo, 7), np.int64)
        out[:, 0] = w[:, :, 3].sum(axis=1)
        out[:, 1:4] = w[:, :, :3].sum(axis=1)
        out[:, 4] = np.searchsorted(self.bind_tick[self.bind_status == OK], ticks, side="right")
        out[:, 5] = np.searchsorted(self.bind_tick[self.bind_status == OVER], ticks, side="right")
        out[:, 6] = np.searchsorted(self.arrival, ticks, side="right") - np.searchsorted(self.bind_tick, ticks, side="right")
        return out

    def listed(self, t_lo, t_hi):
        """Per node the pods that run somewhere in [t_lo, the run's end) and were bound by t_hi - 1:
        bound Ok, dur > 0, bind tick <= t_hi - 1, bind + dur > t_lo."""
        sel = (self.dur > 0) & (self.b <= t_hi - 1) & (self.e > t_lo)
        return np.bincount(self.node[sel], minlength=self.n)

    def same_tick_events(self, t_lo, t_hi):
        """Ticks of (t_lo, t_hi) on which some node has a bind and an expiry of listed pods."""
        sel = (self.dur > 0) & (self.b <= t_hi - 1) & (self.e > t_lo)
        key = lambda node, t: node * (1 << 40) + t
        both = np.intersect1d(key(self.node[sel], self.b[sel]), key(self.node[sel], self.e[sel])) % (1 << 40)
        return np.unique(both[(both > t_lo) & (both < t_hi)])

    # -- usage ----------------------------------------------------------------------------------
    def usage_window(self, t_lo, t_hi):
        """[t_hi - t_lo][n][3]: per-node usage, the input of usage_digest.digest_from_matrices."""
        p, ts = self.tr["pods"], self.ts
        off = np.asarray(p["phase_off"], np.int64)
        sec = np.asarray(p["phase_sec"], np.int64)
        nph = np.diff(off)
        F = len(sec)
        assert (t_hi - int(self.b.min(initial=t_hi))) * ts < (1 << 31), "passed seconds would wrap"
        # wrapped cumulative seconds of every phase and the largest one before it, slot by slot
        acc, before = np.zeros(F, np.int64), np.zeros(F, np.int64)
        run = np.zeros(self.m, np.int64)
        top = np.zeros(self.m, np.int64)          # passed >= 0: a phase starts at 0 at the earliest
        for k in range(int(nph.max(initial=0))):
            has = np.nonzero(nph > k)[0]
            f = off[has] + k
            run[has] = _wrap32(run[has] + sec[f])
            acc[f], before[f] = run[has], top[has]
            top[has] = np.maximum(top[has], run[has])
        S = run                                    # the pod's wrapped total
        owner = np.repeat(np.arange(self.m), nph)
        lo, hi = before, np.minimum(acc, S[owner])
        use = _masked(p["phase_use"], p["phase_has"])
        # per Ok bind: its phases
        cnt = nph[self.pod]
        bi = np.repeat(np.arange(len(self.pod)), cnt)
        f = np.repeat(off[self.pod], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        live = hi[f] > lo[f]
        f, bi = f[live], bi[live]
        a = self.b[bi] + (lo[f] + ts - 1) // ts
        z = self.b[bi] + (hi[f] + ts - 1) // ts
        return self._spread(t_lo, t_hi, self.node[bi], a, z, use[f])


def oracle_binds(tr, mode_tuple, ticks):
    """The C oracle's binds of one submit and ``ticks`` ticks; the run must end without an error."""
    from pyoracle import COracle
    fm, fl, sc = mode_tuple
    ora = COracle(tr, filter_mode=fm, filters=fl, scorers=sc)
    ora.submit(tr)
    ob, rc = ora.step(ticks, cap=ticks)
    ora.close()
    assert rc == 0, f"the oracle stopped with {rc}"
    return ob


def find_window(ref, k, t_max, t_from=0):
    """The first (t_lo, t_hi, node) with t_lo >= t_from, t_hi - 1 <= t_max and exactly ``k`` listed
    pods on ``node``, or None.  For a given t_lo a node's listed count grows with t_hi one bind at a
    time (binds fall on distinct ticks), so the first t_hi that reaches k has exactly k."""
    for t_lo in range(t_from, t_max):
        for node in range(ref.n):
            sel = (ref.node == node) & (ref.dur > 0) & (ref.e > t_lo)
            bs = np.sort(ref.b[sel])
            if len(bs) >= k and t_lo < bs[k - 1] <= t_max:
                t_hi = int(bs[k - 1]) + 1
                if ref.listed(t_lo, t_hi)[node] == k:
                    return t_lo, t_hi, node
    return None
