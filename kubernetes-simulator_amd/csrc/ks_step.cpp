// ks_step.cpp — ks_step and ks_group_step: the host side of the hot path.
//
// A batched step (step_body) reads top to bottom: prepare the counters, take the per-tick shortcut
// when exactly one pod binds, decide the plan once (ks_plan.h: which of the four launch chains, the
// block lists' length), upload the argument records, then per pass issue the chain's batches,
// enqueue the counters' and the binds' copies behind them and wait once; on a long pass the binds
// below a snapshot of the start counter come back early, on a copy stream, and are finished while
// the last rounds run (ks_plan.h early_round), and a later pass hides the finishing of the earlier
// passes' binds.  A pass that leaves pods is followed by another.  At the end account the profile
// and finish the remaining binds.  Each chain has one function that issues one batch's launches in stream order
// (batch_plain, batch_overlap_sharded, batch_two_launch, batch_pipe); the only conditions left inside
// are the batch's position in the pass and, on the plain chain, which kernels the resolver takes.
// Profile marks (ks_plan.h Mark) are recorded by name around the launches while profiling is on and
// cost nothing otherwise.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "ks_host.h"

using namespace ks_host;

namespace {

constexpr int kRescanWgs = 1024;  // the pipelined chain's conditional local rescan: workgroups
// a pass copies the words of at most this many pods behind its last round, before it knows how many
// of them were bound (step_body): 16 KB per array
constexpr int64_t kCopyBehindMax = 4096;

// ks_step, first half: the pods whose bind tick falls in (tick, tick + ticks] and the device
// counters for them.  Returns false when there is nothing to schedule (the caller just advances
// the tick once the step as a whole has succeeded).
bool step_prepare(ks_engine* e, int64_t ticks, int64_t* p_hi_out) {
    const int64_t t_end = e->tick + ticks;
    const int64_t p_hi = std::upper_bound(e->h_bind_tick.begin() + e->done, e->h_bind_tick.end(), t_end) -
                         e->h_bind_tick.begin();
    *p_hi_out = p_hi;
    e->stats = ks_step_stats{};
    e->kstats = ks_kernel_stats{};
    e->h_ctr[0] = e->done;
    e->h_ctr[1] = std::max(p_hi, e->done);
    e->h_ctr[2] = 0;
    e->h_ctr[3] = -1;
    e->h_ctr[4] = 0;
    *e->h_args = make_args(e);
    return p_hi > e->done;
}

// A device failure inside a step leaves the device counters and the binds of the step unknown:
// the engine stops (sticky KS_EDEVICE) with its tick and binds at the last completed step.
ks_status device_stop(ks_engine* e, ks_status r) {
    if (r == KS_EDEVICE && e->err == KS_OK) {
        e->err = KS_EDEVICE;
        if (e->errmsg.empty()) e->errmsg = "device failure during a step";
    }
    return r;
}

// The binds of pods [lo, hi) of a step that began at pod e->done (node / status: the words of the
// step's pods from e->done on, copied back by the caller) into the caller's rows, clipped at cap,
// and into the host mirror.
void bind_rows(ks_engine* e, int64_t lo, int64_t hi, const int32_t* node, const int32_t* status, ks_bind* out,
               int64_t cap) {
    const int64_t base = e->done;
    for (int64_t j = lo; j < hi && j - base < cap; j++) {
        ks_bind& o = out[j - base];
        o.pod = j;
        o.node = node[j - base];
        o.status = status[j - base];
        o.tick = e->h_bind_tick[j];
    }
    for (int64_t j = lo; j < hi; j++) {
        e->h_node[j] = node[j - base];
        e->h_status[j] = (int8_t)status[j - base];
    }
}

// ks_step's end once the rows of [done, new_done) are written: the counts, the error as Run would
// return it (kubesim.go:114-120, 217-220), the tick.
ks_status step_close(ks_engine* e, int64_t t_end, int64_t new_done, int64_t* n_out) {
    *n_out = new_done - e->done;
    e->done = new_done;
    if (e->h_ctr[2] != 0) {
        const int64_t pod = e->h_ctr[3];
        e->err = (int)e->h_ctr[2];
        e->tick = e->h_bind_tick[pod];
        e->done = pod + 1;  // popped from the queue, not bound
        if (e->err == KS_ENOTFOUND)
            fail(e, KS_ENOTFOUND, "node \"\" not found (pod %lld, tick %lld)", (long long)pod, (long long)e->tick);
        else
            fail(e, KS_EINVAL, "pod %lld: invalid pod key or simSpec (tick %lld)", (long long)pod, (long long)e->tick);
        return (ks_status)e->err;
    }
    e->tick = t_end;
    return KS_OK;
}

// ks_step, second half: the binds [done, new_done) (node / status copied back by the caller) and the
// step's end.
ks_status step_finish(ks_engine* e, int64_t t_end, int64_t new_done, const int32_t* node, const int32_t* status,
                      ks_bind* out, int64_t cap, int64_t* n_out) {
    bind_rows(e, e->done, new_done, node, status, out, cap);
    return step_close(e, t_end, new_done, n_out);
}

// Expiries attached to pods [lo, hi) have been applied on the device (the batch path applies
// every expiry attached to a processed pod whose pod was bound Ok): mirror them.
void mirror_expired(ks_engine* e, int64_t lo, int64_t hi) {
    for (int64_t j = lo; j < hi; j++)
        for (int64_t u = e->h_exp_off[j]; u < e->h_exp_off[j + 1]; u++) {
            const int32_t q = e->h_exp_pod[u];
            if (e->h_status[q] == KS_POD_OK) e->h_expired[q] = 1;
        }
}

// a buffer of n T, every byte set to `byte` in the stream's order
template <typename T>
hipError_t alloc_set(ks_own::Dev<T>& o, size_t n, int byte, hipStream_t st) {
    KS_TRY(ks_own::dev_alloc(o, n));
    return hipMemsetAsync(o, byte, sizeof(T) * n, st);
}

// The per-tick path (ks_tick.hip): exactly one pod binds in this step — one launch does the
// staged submits, the pod's expiries, the full-cluster evaluation, the argmax and the bind.
// Returns false (nothing done) when the pod's expiries do not fit the launch's by-value list.
bool tick_step(ks_engine* e, int64_t t_end, ks_bind* out, int64_t cap, int64_t* n_out, ks_status* rc) {
    const int64_t j = e->done;
    ks::TickArgs a{};
    for (int64_t u = e->h_exp_off[j]; u < e->h_exp_off[j + 1]; u++) {
        const int32_t q = e->h_exp_pod[u];
        if (e->h_status[q] != KS_POD_OK || e->h_expired[q]) continue;
        if (a.n_exp == ks::kTickMaxExp) return false;
        ks::TickExp& x = a.exp[a.n_exp++];
        x.node = e->h_node[q];
        x.q = q;
        for (int k = 0; k < 3; k++) x.req[k] = e->h_pods[q].req[k];
    }
    *rc = KS_OK;
    if (!e->tickset) {
        const hipError_t r = ks_own::build(e->tickset, [&](TickSet& t) {
            KS_TRY(alloc_set(t.d_tick, 1, 0, e->st));
            return ks_own::pinned_alloc(t.h_tick, 1, hipHostMallocMapped);
        });
        if (r != hipSuccess) { *rc = fail(e, KS_EDEVICE, "per-tick path setup: %s", hipGetErrorString(r)); return true; }
    }
    a.c = e->dc;
    a.s = e->s;
    a.pod = e->h_pods[j];
    a.j = j;
    a.run = e->h_dur[j] > 0;
    a.b_node = e->b_node.p;
    a.b_status = e->b_status.p;
    a.expired = e->expired.p;
    a.scr = e->tickset->d_tick;
    a.out = e->tickset->h_tick.dev;
    if (stage_xpos(e) != hipSuccess) { *rc = fail(e, KS_EDEVICE, "per-tick path: staging failed"); return true; }
    // the pending staged rows inline in the arguments when they fit (one pod's submit does), else
    // one scatter launch ahead of the kernel
    {
        int32_t off = 0;
        bool fits = e->nseg - e->seg_done <= ks::kTickInlSeg;
        for (int k = e->seg_done; fits && k < e->nseg; k++) {
            off += (int32_t)((e->arena->segs[k].bytes + 15) / 16 * 16);
            fits = off <= ks::kTickInl;
        }
        if (fits) {
            off = 0;
            for (int k = e->seg_done; k < e->nseg; k++) {
                const ks::CopySeg& sg = e->arena->segs[k];
                std::memcpy(a.inl + off, e->arena->mem + (sg.src - e->arena->mem.dev), (size_t)sg.bytes);
                a.iseg[a.n_iseg++] = ks::TickSeg{sg.dst, off, (int32_t)sg.bytes};
                off += (int32_t)((sg.bytes + 15) / 16 * 16);
            }
            e->seg_done = e->nseg;
        } else if (stage_flush(e) != hipSuccess) {
            *rc = fail(e, KS_EDEVICE, "per-tick path: staging failed");
            return true;
        }
    }
    __atomic_store_n(&e->tickset->h_tick->code, -1, __ATOMIC_RELAXED);
    hipError_t r = ks::launch_tick(a, e->mode, e->st);
    if (r == hipSuccess) r = hipEventRecord(e->stage_ev, e->st);
    // the result: poll the host-mapped code the last workgroup stores (release) after node and
    // status — microseconds sooner than a stream synchronisation; the stream is queried now and
    // then so that a failed launch still ends the wait
    for (uint32_t spin = 1; r == hipSuccess; spin++) {
        if (__atomic_load_n(&e->tickset->h_tick->code, __ATOMIC_ACQUIRE) >= 0) break;
        if ((spin & 1023) == 0) {
            const hipError_t q = hipStreamQuery(e->st);
            if (q == hipSuccess) break;  // done: the code is read below
            if (q != hipErrorNotReady) r = q;
        }
        __builtin_ia32_pause();
    }
    if (r != hipSuccess) { *rc = fail(e, KS_EDEVICE, "per-tick launch: %s", hipGetErrorString(r)); return true; }
    ks::TickOut o;
    o.code = __atomic_load_n(&e->tickset->h_tick->code, __ATOMIC_ACQUIRE);
    o.node = ((volatile ks::TickOut*)e->tickset->h_tick)->node;
    o.status = ((volatile ks::TickOut*)e->tickset->h_tick)->status;
    for (int k = 0; k < a.n_exp; k++) e->h_expired[a.exp[k].q] = 1;
    e->stats = ks_step_stats{};
    e->stats.launches = 1;
    e->h_ctr[2] = o.code;
    e->h_ctr[3] = j;
    if (o.code < 0) { *rc = fail(e, KS_EDEVICE, "per-tick kernel wrote no result"); return true; }
    const int32_t node = o.node, status = o.status;
    *rc = step_finish(e, t_end, o.code ? j : j + 1, &node, &status, out, cap, n_out);
    e->stats.pods = *n_out;
    return true;
}

}  // namespace

// pruned block lists for chunk-resolver engines of >= this many scan blocks (or KS_ENGINE_PRUNED_LISTS)
#ifndef KS_PRUNE_MIN_BLOCKS
#define KS_PRUNE_MIN_BLOCKS 1024  // (A/B: make variant NAME=noprune DEFS=-DKS_PRUNE_MIN_BLOCKS=1000000)
#endif
constexpr int kPruneMinBlocks = KS_PRUNE_MIN_BLOCKS;

// The batch window workspace (~0.8 MB) with the node -> E index, the pruned lists' bitmaps and the
// pipelined sharded chain's stream, events and full-range arguments, each made on the first step that
// runs a resolver using it (what-if group members never do).
ks_status ks_host::ensure_window_ws(ks_engine* e) {
    hipStream_t st = e->st;
    const int r = resolver_of(e);
    // (on a failed build only: prune is set once the bitmaps are there, and the pipelined set is
    // looked for on every call, not only on the one that made the window workspace)
    const bool prune = r == kResolveChunk && !e->group && (e->nblk >= kPruneMinBlocks || (e->flags & KS_ENGINE_PRUNED_LISTS));
    ks_status s = KS_OK;
    if (prune && !e->bits) {
        e->nwl = (e->nblk + 63) / 64;
        s = ks_own::build(e->bits, [&](PruneBits& b) {
            HIPCHK(e, alloc_set(b.lbit, 2 * (size_t)e->B * e->nwl, 0, st));  // two sets (EngineArgs)
            HIPCHK(e, alloc_set(b.lthr, 2 * ks::kThrCopies * (size_t)e->B, 0, st));
            return KS_OK;
        });
    }
    if (s != KS_OK) return s;
    e->prune = prune;
    if (r != kResolveChunk) return KS_OK;
    if (!e->win) s = ks_own::build(e->win, [&](WindowWs& w) {
        HIPCHK(e, alloc_set(w.d_sweep, 1, 0, st));
        HIPCHK(e, alloc_set(w.d_eidx, e->n_pad, 0xFF, st));
        HIPCHK(e, alloc_set(w.d_nslot, e->n_pad, 0xFF, st));
        HIPCHK(e, alloc_set(w.d_first, e->n_pad, 0x7F, st));  // kNoFirst
        HIPCHK(e, alloc_set(w.d_spec, 2 * ks::kSpecStride, 0, st));
        HIPCHK(e, ks_own::dev_alloc(w.d_args_spec, 2));
        HIPCHK(e, ks_own::pinned_alloc(w.h_args_spec, 2));
        int cus = 0;  // the fused scan's workgroups: one per CU beside the resolver's (its LDS footprint allows one per CU)
        HIPCHK(e, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device));
#ifndef KS_SCAN_WORKERS_DIV
#define KS_SCAN_WORKERS_DIV 1  // (A/B builds: make variant DEFS=-DKS_SCAN_WORKERS_DIV=2)
#endif
        w.scan_workers = std::max(15, cus / KS_SCAN_WORKERS_DIV - 1);  // (>= 15: every XCD deals its share to at least one)
        return KS_OK;
    });
    if (s == KS_OK && !e->pipe && e->world * e->vsh > 1) s = ks_own::build(e->pipe, [&](PipeSet& p) {
        HIPCHK(e, ks_own::stream_create(p.st2));
        HIPCHK(e, ks_own::event_create(p.pev_m, hipEventDisableTiming));
        HIPCHK(e, ks_own::event_create(p.pev_x, hipEventDisableTiming));
        HIPCHK(e, ks_own::dev_alloc(p.d_args_full, 1));
        HIPCHK(e, ks_own::pinned_alloc(p.h_args_full, 1));
        return KS_OK;
    });
    return s;
}

namespace {

// This rank's per-part merges of its block lists into its parts' slices of cand_all (a: the
// argument record whose counters name the batch; lset_fixed >= 0: that list set's bitmaps)
hipError_t part_merges(ks_engine* e, const ks::EngineArgs* a, hipStream_t s, int lset_fixed) {
    const int64_t L = e->L, BL = (int64_t)e->B * L;
    ks::MergeOpts o;
    o.bits = e->prune ? (uint64_t*)e->bits->lbit : nullptr;
    o.nwl = e->nwl;
    o.lset_fixed = lset_fixed;
    o.L = (int)L;
    for (int v = 0; v < e->vsh; v++) {
        const int p = e->rank * e->vsh + v;
        ks::ListSet in;  // the blocks of part p among the engine's block lists
        in.lists = e->lists + (int64_t)e->part_lo[p] * L;
        in.pod_stride = (int64_t)e->nblk * L;
        in.nl = in.nl_max = e->part_lo[p + 1] - e->part_lo[p];
        in.list_stride = L;
        o.blk0 = e->part_lo[p];
        const hipError_t r = ks::launch_merge(a, 1, e->B, in, e->cand_all + p * BL, s, o);
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}

// The all-gather of every rank's parts of cand_all on stream s: RCCL, or the host callback
ks_status exchange(ks_engine* e, hipStream_t s) {
    const int64_t BL = (int64_t)e->B * e->L;
    if (e->comm) {
        const ncclResult_t nr = ncclAllGather(e->cand_all + (int64_t)e->rank * e->vsh * BL, e->cand_all,
                                              (size_t)e->vsh * BL, ncclUint64, e->comm, s);
        if (nr != ncclSuccess) return fail(e, KS_EDEVICE, "ncclAllGather: %s", ncclGetErrorString(nr));
    } else if (e->xfn) {  // host exchange: this rank's parts out, every rank's parts back
        const int64_t slice = (int64_t)e->vsh * BL, off = (int64_t)e->rank * slice;
        HIPCHK(e, hipMemcpyAsync(e->h_xbuf + off, e->cand_all + off, sizeof(uint64_t) * slice, hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipStreamSynchronize(s));
        const ks_status xr = e->xfn(e->xuser, e->rank, e->world, e->h_xbuf, (int64_t)sizeof(uint64_t) * slice);
        if (xr != KS_OK) return fail(e, KS_EDEVICE, "host exchange failed (%d)", (int)xr);
        HIPCHK(e, hipMemcpyAsync(e->cand_all, e->h_xbuf, sizeof(uint64_t) * slice * e->world, hipMemcpyHostToDevice, s));
    }
    return KS_OK;
}

// A batch's position in its pass.
struct BatchPos {
    int64_t b;   // index in the pass (its parity names the speculative counters' buffer)
    bool first;  // the pass's first batch: nothing speculative precedes it
    bool more;   // another batch of the pass follows: the resolve launch carries its scan or window
};

// ---- profile marks ---------------------------------------------------------------------------
// One step's marks: a pooled HIP event per mark and batch (ks_engine::prof_ev, kept across steps)
// and the batches' records.  Off the profiling path begin() and mark() do nothing: no event call,
// no allocation.  The events around the scan kernel alone and the resolve kernel alone are on the
// engine's stream, so their averages agree with rocprofv3's kernel trace.
struct StepProfile {
    ks_engine* e;
    std::vector<BatchRecord> recs;

    // a batch starts: what it will launch (ks_plan.h batch_record)
    hipError_t begin(Chain chain, const BatchPos& pos, bool sharded) {
        if (!e->profiling) return hipSuccess;
        recs.push_back(batch_record(chain, pos.first, pos.more, sharded));
        while (e->prof_ev.size() < (size_t)kMarkCount * recs.size()) {
            ks_own::Event x;
            KS_TRY(ks_own::event_create(x));
            e->prof_ev.push_back(std::move(x));
        }
        return hipSuccess;
    }
    hipEvent_t event(size_t batch, Mark m) const { return e->prof_ev[(size_t)kMarkCount * batch + m]; }
    hipError_t mark(Mark m, hipStream_t s) {
        if (!e->profiling) return hipSuccess;
        recs.back().recorded |= 1u << m;
        return hipEventRecord(event(recs.size() - 1, m), s);
    }
    // after the step's last synchronisation: every batch's intervals into the statistics
    void account(ks_kernel_stats& ks, StepSums& sums) const {
        for (size_t l = 0; l < recs.size(); l++) {
            float t[kIvCount] = {};
            for (int iv = 0; iv < kIvCount; iv++)
                if (interval_recorded(recs[l], iv))
                    (void)hipEventElapsedTime(&t[iv], event(l, kIntervalEnds[iv][0]), event(l, kIntervalEnds[iv][1]));
            account_batch(recs[l], t, ks, sums);
        }
    }
};

// ---- stages the chains share -------------------------------------------------------------------

// a scan in the engine's list form (pruned or not, the lists' length); the caller names what else it wants
ks::ScanOpts scan_opts(const ks_engine* e) {
    ks::ScanOpts o;
    o.prune = e->prune;
    o.L = e->L;
    return o;
}

// the scan of blk_n blocks by the argument record a on stream s
hipError_t scan(ks_engine* e, const ks::EngineArgs* a, int blk_n, hipStream_t s, const ks::ScanOpts& o) {
    return ks::launch_scan(a, 1, blk_n, e->B, e->PG, e->mode, key16(e), s, o);
}

// this rank's part merges and the exchange on stream s, a mark after each
ks_status parts_and_exchange(ks_engine* e, StepProfile& pf, const ks::EngineArgs* a, hipStream_t s, int lset_fixed,
                             Mark after_parts, Mark after_xchg) {
    HIPCHK(e, part_merges(e, a, s, lset_fixed));
    HIPCHK(e, pf.mark(after_parts, s));
    if (ks_status r = exchange(e, s); r != KS_OK) return r;
    HIPCHK(e, pf.mark(after_xchg, s));
    return KS_OK;
}

// A sharded engine's merge on the main stream: part merges -> exchange -> the second merge over
// every part's kTopL lists (merge_cl with the candidate lists for the chunk resolver)
ks_status sharded_merge(ks_engine* e, StepProfile& pf, bool fused) {
    if (ks_status r = parts_and_exchange(e, pf, e->d_args, e->st, -1, kMarkParts, kMarkXchg); r != KS_OK) return r;
    const ks::ListSet in = ks::exchanged_lists(e->cand_all, e->world * e->vsh, e->B, ks::kTopL);
    HIPCHK(e, fused ? ks::launch_merge_cl(e->d_args, e->mode, e->B, in, e->st)
                    : ks::launch_merge(e->d_args, 1, e->B, in, e->cand, e->st));
    return KS_OK;
}

// The chunk kernel of batch pos.b: with the next batch's window (and, by `workers` scan workgroups,
// its speculative scan) fused in while the pass goes on, alone on its last batch
hipError_t chunk_resolve(ks_engine* e, const BatchPos& pos, int workers, int L) {
    if (!pos.more) return ks::launch_chunk_only(e->d_args, e->mode, e->st);
    return ks::launch_chunk_scan(e->d_args, e->win->d_args_spec + (pos.b & 1), workers, (int)((pos.b + 1) & 1), e->mode,
                                 e->prune, L, e->st);
}

// ---- the four chains: one batch each, in stream order ------------------------------------------

// The plain chain, four launches: expiries (with the window, for the chunk resolver) -> scan ->
// merge (sharded: part merges, exchange, second merge) -> resolver.
ks_status batch_plain(ks_engine* e, const StepPlan& plan, const BatchPos& pos, StepProfile& pf) {
    hipStream_t st = e->st;
    const ks::EngineArgs* d = e->d_args;
    const bool fused = plan.resolver == kResolveChunk, sharded = e->world * e->vsh > 1;
    HIPCHK(e, pf.begin(kChainPlain, pos, sharded));
    HIPCHK(e, pf.mark(kMarkBegin, st));
    HIPCHK(e, fused ? ks::launch_window_prep(d, true, false, (int)(pos.b & 1), st) : ks::launch_expire_head(d, 1, st));
    HIPCHK(e, pf.mark(kMarkPrep, st));
    ks::ScanOpts so = scan_opts(e);
    so.stage = fused;  // (chunk class: the scan launch also stages the batch's E records for merge_cl)
    HIPCHK(e, scan(e, d, e->blk_n, st, so));
    HIPCHK(e, pf.mark(kMarkScan, st));
    if (sharded) {
        if (ks_status r = sharded_merge(e, pf, fused); r != KS_OK) return r;
    } else if (fused) {
        ks::MergeClOpts o;
        o.L = e->L;
        HIPCHK(e, ks::launch_merge_cl(d, e->mode, e->B, ks::own_block_lists(e->nblk), st, o));
    } else {
        HIPCHK(e, ks::launch_merge(d, 1, e->B, ks::own_block_lists(e->nblk), nullptr, st));
    }
    HIPCHK(e, pf.mark(kMarkMerge, st));
    HIPCHK(e, fused ? ks::launch_chunk_only(d, e->mode, st) : launch_resolver(d, 1, e->mode, plan.resolver, st));
    HIPCHK(e, pf.mark(kMarkResolve, st));
    return KS_OK;
}

// The fused overlap on a sharded engine.  A pass's first batch: window prep -> scan; a later one
// takes the lists the previous chunk kernel's scan workers wrote (its window was computed there
// too, after the commit) and launches only the conditional rescan, for when they do not fit
// (ks_cand.hip window_prep_kernel).  Then the sharded merge, every batch, and the chunk kernel with
// the next batch's scan beside it.
ks_status batch_overlap_sharded(ks_engine* e, const BatchPos& pos, StepProfile& pf) {
    hipStream_t st = e->st;
    HIPCHK(e, pf.begin(kChainOverlapSharded, pos, true));
    HIPCHK(e, pf.mark(kMarkBegin, st));
    if (pos.first) HIPCHK(e, ks::launch_window_prep(e->d_args, true, false, (int)(pos.b & 1), st));
    HIPCHK(e, pf.mark(kMarkPrep, st));
    ks::ScanOpts so = scan_opts(e);
    so.cond = !pos.first;  // (a later batch: only when the window prep flagged a rescan)
    so.stage = true;       // (it also stages the batch's E records for merge_cl)
    HIPCHK(e, scan(e, e->d_args, e->blk_n, st, so));
    HIPCHK(e, pf.mark(kMarkScan, st));
    if (ks_status r = sharded_merge(e, pf, true); r != KS_OK) return r;
    HIPCHK(e, pf.mark(kMarkMerge, st));
    HIPCHK(e, chunk_resolve(e, pos, e->win->scan_workers, e->L));
    HIPCHK(e, pf.mark(kMarkResolve, st));
    return KS_OK;
}

// The two-launch chain (the fused overlap on one shard).  A pass's first batch: window prep -> scan
// -> merge_cl -> chunk kernel; every later one: merge_cl -> chunk kernel, no scan launch and no E
// staging (merge_cl's direct form reads the node table and the constants table step_body filled).
ks_status batch_two_launch(ks_engine* e, const BatchPos& pos, StepProfile& pf) {
    hipStream_t st = e->st;
    HIPCHK(e, pf.begin(kChainTwoLaunch, pos, false));
    HIPCHK(e, pf.mark(kMarkBegin, st));
    if (pos.first) HIPCHK(e, ks::launch_window_prep(e->d_args, true, false, (int)(pos.b & 1), st));
    HIPCHK(e, pf.mark(kMarkPrep, st));
    if (pos.first) HIPCHK(e, scan(e, e->d_args, e->blk_n, st, scan_opts(e)));
    HIPCHK(e, pf.mark(kMarkScan, st));
    ks::MergeClOpts o;
    o.L = e->L;
    o.direct = true;
    HIPCHK(e, ks::launch_merge_cl(e->d_args, e->mode, e->B, ks::own_block_lists(e->nblk), st, o));
    HIPCHK(e, pf.mark(kMarkMerge, st));
    HIPCHK(e, chunk_resolve(e, pos, e->win->scan_workers, e->L));
    HIPCHK(e, pf.mark(kMarkResolve, st));
    return KS_OK;
}

// The pipelined sharded chain.  Main stream: [the pass's first batch: window prep, scan of this
// rank's blocks, part merges, exchange | later batches: wait for the second stream's exchange, the
// conditional local rescan (E overflow only) with the E staging] -> merge_cl -> the resolve with the
// next batch's window in its tail.  Second stream, once merge_cl has read the lists and cleared the
// speculative set: the next batch's speculative scan of this rank's blocks (the counters this
// batch's window prep wrote), its part merges and the exchange — beside the resolve.  cand_all and
// the block lists are single-buffered: each side pass starts after the merge_cl that read the
// previous one.  A batch that starts inside its predecessor (an early stop) reuses its merged lists
// (ks_prep.h), so the exchanged lists always serve; when E overflows, the rescan scans every block
// locally (no second exchange: every rank holds the whole table) and merge_cl merges those.
ks_status batch_pipe(ks_engine* e, const BatchPos& pos, StepProfile& pf) {
    hipStream_t st = e->st, s2 = e->pipe->st2;
    const ks::EngineArgs* d = e->d_args;
    HIPCHK(e, pf.begin(kChainPipe, pos, true));
    HIPCHK(e, pf.mark(kMarkBegin, st));
    if (pos.first) {
        HIPCHK(e, ks::launch_window_prep(d, true, false, (int)(pos.b & 1), st));
        HIPCHK(e, pf.mark(kMarkPrep, st));
        ks::ScanOpts so = scan_opts(e);
        so.stage = true;
        HIPCHK(e, scan(e, d, e->blk_n, st, so));
        HIPCHK(e, pf.mark(kMarkScan, st));
        if (ks_status r = parts_and_exchange(e, pf, d, st, -1, kMarkParts, kMarkXchg); r != KS_OK) return r;
    } else {
        HIPCHK(e, hipStreamWaitEvent(st, e->pipe->pev_x, 0));
        HIPCHK(e, pf.mark(kMarkPrep, st));
        ks::ScanOpts rescan = scan_opts(e);  // every block, only when the window prep flagged it
        rescan.cond = true;
        rescan.stage = true;
        rescan.pw = kRescanWgs;  // (a small persistent grid)
        HIPCHK(e, scan(e, e->pipe->d_args_full, e->nblk, st, rescan));
        HIPCHK(e, pf.mark(kMarkScan, st));
        HIPCHK(e, pf.mark(kMarkParts, st));  // (on the second stream: zero intervals here)
        HIPCHK(e, pf.mark(kMarkXchg, st));
    }
    ks::MergeClOpts mo;
    mo.L = e->L;
    mo.own_fallback = !pos.first;
    HIPCHK(e, ks::launch_merge_cl(d, e->mode, e->B, ks::exchanged_lists(e->cand_all, e->world * e->vsh, e->B, e->L), st, mo));
    HIPCHK(e, pf.mark(kMarkMerge, st));
    if (pos.more) HIPCHK(e, hipEventRecord(e->pipe->pev_m, st));
    // (no scan workers: the resolver and the next window only; the list length is the workers')
    HIPCHK(e, chunk_resolve(e, pos, 0, ks::kTopL));
    HIPCHK(e, pf.mark(kMarkResolve, st));
    if (pos.more) {
        const ks::EngineArgs* ds = e->win->d_args_spec + (pos.b & 1);
        HIPCHK(e, hipStreamWaitEvent(s2, e->pipe->pev_m, 0));
        HIPCHK(e, pf.mark(kMarkSideBegin, s2));
        HIPCHK(e, scan(e, ds, e->blk_n, s2, scan_opts(e)));
        HIPCHK(e, pf.mark(kMarkSideScan, s2));
        if (ks_status r = parts_and_exchange(e, pf, ds, s2, 0, kMarkSideParts, kMarkSideXchg); r != KS_OK) return r;
        HIPCHK(e, hipEventRecord(e->pipe->pev_x, s2));
    }
    return KS_OK;
}

ks_status chain_batch(ks_engine* e, const StepPlan& plan, const BatchPos& pos, StepProfile& pf) {
    switch (plan.chain) {
        case kChainOverlapSharded: return batch_overlap_sharded(e, pos, pf);
        case kChainTwoLaunch: return batch_two_launch(e, pos, pf);
        case kChainPipe: return batch_pipe(e, pos, pf);
        default: return batch_plain(e, plan, pos, pf);
    }
}

// The argument records of the step's chain, after the counters on the engine's stream: the engine's
// own; the pipelined chain's full-range record (its rescan: every block, the engine's own list set);
// the two speculative records of the chains whose next batch is scanned ahead (ctr = the
// speculative counters of either parity, pruned lists: set 0).  The two-launch chain also fills the
// node constants table here (after the stage flush, and after any rescale: ks_submit_pods runs it).
ks_status upload_args(ks_engine* e, const StepPlan& plan) {
    hipStream_t st = e->st;
    const bool two = plan.chain == kChainTwoLaunch;
    e->h_args->two_launch = two ? 1 : 0;
    HIPCHK(e, hipMemcpyAsync(e->d_args, e->h_args, sizeof(ks::EngineArgs), hipMemcpyHostToDevice, st));
    if (two) HIPCHK(e, ks::launch_node_consts(e->s, e->n_pad, e->d_ncst, st));
    if (plan.chain == kChainPipe) {
        PipeSet& p = *e->pipe;
        *p.h_args_full = *e->h_args;
        p.h_args_full->blk_lo = 0;
        p.h_args_full->blk_n = e->nblk;
        HIPCHK(e, hipMemcpyAsync(p.d_args_full, p.h_args_full, sizeof(ks::EngineArgs), hipMemcpyHostToDevice, st));
    }
    if (plan.chain != kChainPlain) {
        WindowWs& w = *e->win;
        for (int k = 0; k < 2; k++) {
            w.h_args_spec[k] = *e->h_args;
            w.h_args_spec[k].ctr = w.d_spec + ks::kSpecStride * k;
            w.h_args_spec[k].lset = 0;
        }
        HIPCHK(e, hipMemcpyAsync(w.d_args_spec, w.h_args_spec, 2 * sizeof(ks::EngineArgs), hipMemcpyHostToDevice, st));
    }
    return KS_OK;
}

// The step's read-back buffers: pinned node and status words for n pods, allocated once and grown
// geometrically (nothing is in flight into them between steps); `early`: the chain may read back
// early, on its copy stream.
ks_status ensure_readback(ks_engine* e, int64_t n, bool early) {
    if (const int64_t cap = e->rb ? e->rb->cap : 0; n > cap) {
        e->rb.reset();  // (freed before the larger ones are made)
        const ks_status r = ks_own::build(e->rb, [&](Readback& b) {
            b.cap = std::max<int64_t>({n, 2 * cap, 4096});
            HIPCHK(e, ks_own::pinned_alloc(b.h_bnode, b.cap));
            HIPCHK(e, ks_own::pinned_alloc(b.h_bstat, b.cap));
            return KS_OK;
        });
        if (r != KS_OK) return r;
    }
    if (!early || e->early) return KS_OK;
    return ks_own::build(e->early, [&](EarlyCopy& c) {
        HIPCHK(e, ks_own::stream_create(c.st_copy));
        HIPCHK(e, ks_own::event_create(c.snap_ev, hipEventDisableTiming));
        return KS_OK;
    });
}

// the node and status words of pods [lo, hi) into the read-back buffers (which begin at pod done0), on stream s
ks_status copy_binds(ks_engine* e, int64_t done0, int64_t lo, int64_t hi, hipStream_t s) {
    if (hi <= lo) return KS_OK;
    const size_t bytes = sizeof(int32_t) * (size_t)(hi - lo);
    HIPCHK(e, hipMemcpyAsync(e->rb->h_bnode + (lo - done0), e->b_node.p + lo, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(e->rb->h_bstat + (lo - done0), e->b_status.p + lo, bytes, hipMemcpyDeviceToHost, s));
    return KS_OK;
}

// Diagnostic build only (-DKS_TAIL_SPLIT): host timestamps around the sections of step_body outside
// the rounds, one line per step on stderr (us since the step began) — the product executes none of it.
#ifdef KS_TAIL_SPLIT
}  // namespace
#include <chrono>
#include <cstdio>
namespace {
enum { kTsPrepare, kTsUpload, kTsEnqueue, kTsSnapWait, kTsEarlyCopy, kTsEarlyRows, kTsEarlyMirror, kTsSync, kTsStats,
       kTsRows, kTsMirror, kTsCount };
constexpr const char* kTsNames[kTsCount] = {"prepare", "upload", "enqueue", "snap_wait", "early_copy", "early_rows",
                                            "early_mirror", "sync", "stats", "rows", "mirror"};
#define TAIL_BEGIN()                                               \
    double tail_us[kTsCount] = {};                                 \
    auto tail_t = std::chrono::steady_clock::now()
#define TAIL_AT(I)                                                                             \
    do {                                                                                       \
        const auto t_ = std::chrono::steady_clock::now();                                      \
        tail_us[I] += std::chrono::duration<double, std::micro>(t_ - tail_t).count();          \
        tail_t = t_;                                                                           \
    } while (0)
#define TAIL_PRINT()                                                                           \
    do {                                                                                       \
        std::fprintf(stderr, "tail_split");                                                    \
        for (int i_ = 0; i_ < kTsCount; i_++) std::fprintf(stderr, " %s=%.1f", kTsNames[i_], tail_us[i_]); \
        std::fprintf(stderr, "\n");                                                            \
    } while (0)
#else
#define TAIL_BEGIN()
#define TAIL_AT(I)
#define TAIL_PRINT()
#endif

ks_status step_body(ks_engine* e, int64_t ticks, ks_bind* out, int64_t cap, int64_t* n_out) {
    TAIL_BEGIN();
    HIPCHK(e, hipSetDevice(e->device));
    if (ks_status r = ensure_window_ws(e); r != KS_OK) return r;
    const int64_t t_end = e->tick + ticks;
    int64_t p_hi = 0;
    if (!step_prepare(e, ticks, &p_hi)) {
        e->tick = t_end;
        return KS_OK;
    }
    // (an explicitly forced resolver keeps one-pod steps on that resolver: its A/B tests)
    if (p_hi == e->done + 1 && !e->group && e->world * e->vsh == 1 && e->n > 0 && !e->profiling &&
        !(e->flags & (KS_ENGINE_CHUNK_RESOLVER | KS_ENGINE_ONE_POD_RESOLVER))) {
        ks_status rc = KS_OK;
        if (tick_step(e, t_end, out, cap, n_out, &rc)) return rc;
    }
    const int64_t done0 = e->done;
    HIPCHK(e, stage_flush(e));
    hipStream_t st = e->st;
    PlanFacts facts{};
    facts.resolver = resolver_of(e);
    facts.overlap = e->overlap;
    facts.spec_args = e->win.has_value();
    facts.key16 = key16(e);
    facts.blk_n = e->blk_n;
    facts.parts = e->world * e->vsh;
    facts.prune = e->prune;
    facts.side_stream = e->pipe.has_value();
    const StepPlan plan = plan_step(facts);
    e->L = plan.L;
    if (ks_status r = ensure_readback(e, p_hi - done0, plan.chain == kChainTwoLaunch); r != KS_OK) return r;
    TAIL_AT(kTsPrepare);
    HIPCHK(e, hipMemcpyAsync(e->d_ctr, e->h_ctr, 5 * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (ks_status r = upload_args(e, plan); r != KS_OK) return r;
    TAIL_AT(kTsUpload);
    HIPCHK(e, hipEventRecord(e->ev[kEvStepBegin], st));
    int64_t start = done0;
    int64_t launches = 0;
    // The read-back buffers hold the final words of pods [done0, have); of those, [done0, fin) are
    // finished on the host: rows written, mirrored, their expiries mirrored.  fin <= have <= start
    // throughout.  A pass is one of three kinds:
    //  * a snapshot pass (two-launch, long, every earlier bind buffered: have == start): the binds
    //    below the snapshot come back on the copy stream and are finished under the last rounds,
    //    the few above it are copied behind the last round;
    //  * a short pass with every earlier bind buffered: its words are copied behind its last round;
    //  * any other (a long pass without a snapshot, or a pass after one): nothing is copied, have
    //    stays behind start, and one copy after the loop fetches [have, new_done) as ks_step always did.
    // In the first two kinds the pass's one wait also delivers its binds, and have follows start.
    int64_t have = done0, fin = done0, snap_pods = 0;
    const int32_t* const node = e->rb->h_bnode;
    const int32_t* const status = e->rb->h_bstat;
    StepProfile pf{e, {}};
    while (true) {
        const int64_t rounds = (p_hi - start + e->B - 1) / e->B;
        const int64_t snap_at = early_round(rounds, plan.chain);
        for (int64_t b = 0; b < rounds; b++, launches++) {
            if (ks_status r = chain_batch(e, plan, BatchPos{b, b == 0, b + 1 < rounds}, pf); r != KS_OK) return r;
            if (b == snap_at) {  // between two rounds: every bind below the counter is visible
                HIPCHK(e, hipMemcpyAsync(e->h_ctr + 8, e->d_ctr + ks::kCtrStart, sizeof(int64_t), hipMemcpyDeviceToHost, st));
                HIPCHK(e, hipEventRecord(e->early->snap_ev, st));
            }
        }
        HIPCHK(e, hipEventRecord(e->ev[kEvStepEnd], st));
        HIPCHK(e, hipMemcpyAsync(e->h_ctr, e->d_ctr, 5 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        TAIL_AT(kTsEnqueue);
        if (fin < have) {  // a later pass: the earlier passes' binds finish under it
            bind_rows(e, fin, have, node, status, out, cap);
            mirror_expired(e, fin, have);
            fin = have;
            TAIL_AT(kTsEarlyMirror);
        }
        int64_t lo = start;  // the pass's binds are [lo, its end): below lo they are in the buffers or come early
        const bool snapped = snap_at >= 0 && have == start;
        if (snapped) {
            // The early read-back: the binds below the snapshot come back on the copy stream and are
            // finished here while the pass's last rounds run.  Should the step fail after this (a
            // device failure, or a pod's error past the snapshot), the host mirrors of these pods
            // and of their expiries are already written, where a failed step used to leave them
            // untouched: acceptable only because the engine is then sticky-failed (ks_step returns
            // its error from then on) and the binds themselves are final — the device committed them.
            HIPCHK(e, hipEventSynchronize(e->early->snap_ev));
            TAIL_AT(kTsSnapWait);
            lo = std::clamp(e->h_ctr[8], start, p_hi);
        }
        // The words of [lo, p_hi) behind the pass's last round, with the counters, when they are few
        // (after a snapshot, or a short pass): one wait ends the pass.  A long pass without a snapshot
        // would copy mostly unbound pods' words, once per pass: its binds are copied after the loop.
        const bool behind = have == start && p_hi - lo <= kCopyBehindMax;
        if (behind)
            if (ks_status r = copy_binds(e, done0, lo, p_hi, st); r != KS_OK) return r;
        if (snapped && lo > have) {
            if (ks_status r = copy_binds(e, done0, have, lo, e->early->st_copy); r != KS_OK) return r;
            HIPCHK(e, hipStreamSynchronize(e->early->st_copy));
            snap_pods += lo - have;
            have = lo;
            TAIL_AT(kTsEarlyCopy);
            bind_rows(e, fin, have, node, status, out, cap);
            TAIL_AT(kTsEarlyRows);
            mirror_expired(e, fin, have);
            TAIL_AT(kTsEarlyMirror);
            fin = have;
        }
        HIPCHK(e, hipStreamSynchronize(st));  // the pass's only wait for the main stream
        TAIL_AT(kTsSync);
        const int64_t prev = start;
        start = e->h_ctr[0];
        if (behind) have = std::clamp(start, have, p_hi);  // (the words below the counter are final)
        if (e->h_ctr[2] != 0 || start >= p_hi) break;
        // every launch commits at least its first pod (resolve_kernel): no progress is a bug
        if (start <= prev) return fail(e, KS_EDEVICE, "scheduling made no progress at pod %lld", (long long)start);
    }
    if (have < start) {  // the binds no pass copied behind its rounds
        if (ks_status r = copy_binds(e, done0, have, start, st); r != KS_OK) return r;
        HIPCHK(e, hipStreamSynchronize(st));
        TAIL_AT(kTsSync);
    }
    const int64_t new_done = start;
    const int64_t nb = new_done - done0;
    e->early_pods = fin - done0;  // (diagnostics: ks_debug_counters [8], [9])
    e->snap_pods = snap_pods;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e->ev[kEvStepBegin], e->ev[kEvStepEnd]);
    ks_kernel_stats ks{};
    StepSums sums;
    pf.account(ks, sums);
    e->kstats = ks;
    e->stats.step_ms = ms;
    e->stats.scan_ms = sums.scan_ms;
    e->stats.resolve_ms = sums.resolve_ms;
    e->stats.other_ms = sums.other_ms;
    e->stats.launches = launches;
    e->stats.pods = nb;
    TAIL_AT(kTsStats);
    bind_rows(e, std::min(fin, new_done), new_done, node, status, out, cap);
    TAIL_AT(kTsRows);
    const ks_status rc = step_close(e, t_end, new_done, n_out);
    if (rc == KS_OK) mirror_expired(e, std::min(fin, new_done), new_done);
    TAIL_AT(kTsMirror);
    TAIL_PRINT();
    return rc;
}

}  // namespace

extern "C" {

ks_status ks_step(ks_engine* e, int64_t ticks, ks_bind* out, int64_t cap, int64_t* n_out) {
    if (!e || !n_out || ticks < 0 || cap < 0 || (cap > 0 && !out)) return KS_EINVAL;
    *n_out = 0;
    if (e->err) return (ks_status)e->err;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (e->P > 0 && !in_passed_domain(e, e->h_bind_tick[0], e->tick + ticks))
        return fail(e, KS_ERANGE, "step to tick %lld: more than 2^31 s after the first bind (tick %lld)",
                    (long long)(e->tick + ticks), (long long)e->h_bind_tick[0]);
    return device_stop(e, step_body(e, ticks, out, cap, n_out));
}

// groups of at least this many scenarios run as two halves on two streams
#ifndef KS_GROUP_SPLIT_MIN
#define KS_GROUP_SPLIT_MIN 64
#endif
constexpr int kGroupSplitMin = KS_GROUP_SPLIT_MIN;

ks_status ks_group_step(ks_group* g, int64_t ticks, ks_bind* out, int64_t cap, int64_t* n_out, int32_t* status_out,
                        ks_step_stats* stats) {
    if (!g || !n_out || !status_out || ticks < 0 || cap < 0) return KS_EINVAL;
    const int S = (int)g->engs.size();
    if (S == 0) return KS_OK;
    if (hipSetDevice(g->device) != hipSuccess) return KS_EDEVICE;
    std::vector<int64_t> p_hi(S, 0), t_end(S, 0);
    std::vector<char> live(S, 0), part(S, 0);  // part: takes part in this step
    int mode = ks::kEvalMicro, blk_n = 0, B = 0;  // B: the largest member batch (grid size)
    bool k16 = true, small = true;
    for (ks_engine* e : g->engs) {
        B = std::max(B, e->B);
        k16 = k16 && key16(e);
        small = small && small_resolver(e);
    }
    // (the chunk resolver takes one engine per launch: not in groups)
    const int which = small ? kResolveSmall : kResolveRole;
    int64_t blocks = 0;
    for (int i = 0; i < S; i++) {
        ks_engine* e = g->engs[i];
        n_out[i] = 0;
        status_out[i] = KS_OK;
        const bool out_of_domain = e->P > 0 && !in_passed_domain(e, e->h_bind_tick[0], e->tick + ticks);
        if (e->err || !e->nodes_loaded || e->world * e->vsh != 1 || out_of_domain) {
            status_out[i] = e->err ? e->err : out_of_domain ? KS_ERANGE : KS_EINVAL;
            if (!e->err) {
                if (out_of_domain) fail(e, KS_ERANGE, "step past 2^31 s after the first bind");
                else fail(e, KS_EINVAL, "group step needs loaded, unsharded nodes");
            }
            e->h_ctr[0] = e->h_ctr[1] = e->done;
            e->h_ctr[2] = 0;
            *e->h_args = e->nodes_loaded ? make_args(e) : ks::EngineArgs{};
            e->h_args->ctr = e->d_ctr;
            e->h_args->blk_n = 0;
            continue;
        }
        t_end[i] = e->tick + ticks;
        part[i] = 1;
        live[i] = step_prepare(e, ticks, &p_hi[i]);
        // the widest evaluator any scenario needs (each is exact on every narrower domain)
        mode = std::min(mode, e->mode);
        blk_n = std::max(blk_n, e->blk_n);
        blocks += e->blk_n;
    }
    // pods per scan workgroup for the whole group: the most node-record reuse that still leaves
    // >= ~2048 workgroups per scan
    int pg = 1;
    while (pg < ks::max_pods_per_scan_wg() && pg < B && blocks * ((B + pg * 2 - 1) / (pg * 2)) >= 2048) pg *= 2;
    for (int i = 0; i < S; i++) g->h_args[i].PG = pg;
    hipStream_t st = g->st;
    auto dev = [&](hipError_t r) { return r == hipSuccess; };
    // a device failure leaves every participating member's step unknown: sticky KS_EDEVICE, ticks
    // and binds stay at the last completed step
    auto dev_fail = [&](const char* what) {
        g->errmsg = what;
        for (int i = 0; i < S; i++)
            if (part[i]) {
                ks_engine* e = g->engs[i];
                e->err = KS_EDEVICE;
                e->errmsg = what;
                status_out[i] = KS_EDEVICE;
            }
        return KS_EDEVICE;
    };
    if (!dev(hipMemcpyAsync(g->d_ctr, g->h_ctr, sizeof(int64_t) * 32 * S, hipMemcpyHostToDevice, st)) ||
        !dev(hipMemcpyAsync(g->d_args, g->h_args, sizeof(ks::EngineArgs) * S, hipMemcpyHostToDevice, st)) ||
        !dev(hipEventRecord(g->ev[kEvStepBegin], st)))
        return dev_fail("group step: argument upload failed");
    std::vector<int64_t> start(S);
    for (int i = 0; i < S; i++) start[i] = g->engs[i]->done;
    int64_t launches = 0;
    // scenario halves [h_lo[h], h_lo[h + 1]) on streams st / st2 (one stream for small groups)
    const int nh = S >= kGroupSplitMin ? 2 : 1;
    const int h_lo[3] = {0, nh == 2 ? S / 2 : S, S};
    hipStream_t hst[2] = {st, g->st2};
    if (nh == 2 && (!dev(hipEventRecord(g->xev, st)) || !dev(hipStreamWaitEvent(g->st2, g->xev, 0))))
        return dev_fail("group step: stream ordering failed");
    while (true) {
        int64_t nbat[2] = {0, 0};
        for (int h = 0; h < nh; h++)
            for (int i = h_lo[h]; i < h_lo[h + 1]; i++)
                if (live[i]) nbat[h] = std::max(nbat[h], (p_hi[i] - start[i] + B - 1) / B);
        if (nbat[0] == 0 && nbat[1] == 0) break;
        // the halves' rounds issued alternately: independent scenarios, no ordering between them
        // (a token that made the halves' scans take turns measured no better)
        for (int64_t b = 0; b < std::max(nbat[0], nbat[1]); b++) {
            for (int h = 0; h < nh; h++) {
                if (b >= nbat[h]) continue;
                const ks::EngineArgs* d = g->d_args + h_lo[h];
                const int Sh = h_lo[h + 1] - h_lo[h];
                if (!dev(ks::launch_expire_head(d, Sh, hst[h])) ||
                    !dev(ks::launch_scan(d, Sh, blk_n, B, pg, mode, k16, hst[h])) ||
                    !dev(ks::launch_merge(d, Sh, B, ks::own_block_lists(blk_n), nullptr, hst[h])) ||
                    !dev(launch_resolver(d, Sh, mode, which, hst[h])))
                    return dev_fail("group step: kernel launch failed");
            }
            launches++;
        }
        for (int h = 0; h < nh; h++) {
            const int64_t lo = h_lo[h], n = h_lo[h + 1] - h_lo[h];
            if (n && !dev(hipMemcpyAsync(g->h_ctr + 32 * lo, g->d_ctr + 32 * lo, sizeof(int64_t) * 32 * n,
                                         hipMemcpyDeviceToHost, hst[h])))
                return dev_fail("group step: device synchronisation failed");
        }
        for (int h = 0; h < nh; h++)
            if (!dev(hipStreamSynchronize(hst[h]))) return dev_fail("group step: device synchronisation failed");
        for (int i = 0; i < S; i++) {
            if (!live[i]) continue;
            ks_engine* e = g->engs[i];
            const int64_t prev = start[i];
            start[i] = e->h_ctr[0];
            if (e->h_ctr[2] != 0 || start[i] >= p_hi[i]) live[i] = 0;
            else if (start[i] <= prev)  // every launch commits at least its first pod
                return dev_fail("group step: scheduling made no progress");
        }
    }
    // binds back: one gather into a packed buffer, one copy
    int64_t total = 0, max_n = 0;
    for (int i = 0; i < S; i++) {
        ks_engine* e = g->engs[i];
        const int64_t nb = status_out[i] == KS_OK && part[i] ? start[i] - e->done : 0;
        g->h_seg[i] = ks::BindSeg{e->b_node.p, e->b_status.p, e->done, std::max<int64_t>(nb, 0), total};
        total += std::max<int64_t>(nb, 0);
        max_n = std::max(max_n, nb);
    }
    if (const int64_t cap0 = g->out ? g->out->cap : 0; total > cap0) {
        g->out.reset();  // (freed before the larger ones are made)
        if (!dev(ks_own::build(g->out, [&](ks_group::OutBuf& b) {
                b.cap = std::max<int64_t>(total, 2 * cap0);
                KS_TRY(ks_own::dev_alloc(b.d_out, 2 * b.cap));
                return ks_own::pinned_alloc(b.h_out, 2 * b.cap);
            })))
            return dev_fail("group step: bind buffer allocation failed");
    }
    int32_t* const h_out = total ? (int32_t*)g->out->h_out : nullptr;
    if (total) {
        int32_t* const d_out = g->out->d_out;
        if (!dev(hipMemcpyAsync(g->d_seg, g->h_seg, sizeof(ks::BindSeg) * S, hipMemcpyHostToDevice, st)) ||
            !dev(ks::launch_gather_binds(g->d_seg, S, max_n, d_out, d_out + total, st)) ||
            !dev(hipMemcpyAsync(h_out, d_out, sizeof(int32_t) * 2 * total, hipMemcpyDeviceToHost, st)))
            return dev_fail("group step: bind copy failed");
    }
    if (!dev(hipEventRecord(g->ev[kEvStepEnd], st)) || !dev(hipStreamSynchronize(st)))
        return dev_fail("group step: device synchronisation failed");
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g->ev[kEvStepBegin], g->ev[kEvStepEnd]);
    // unpack into the caller's ks_bind rows: members are independent, so large groups fill them
    // on several host threads (this is host-memory-bound: 24 B written per bind)
    auto finish = [&](int lo, int hi) {
        for (int i = lo; i < hi; i++) {
            ks_engine* e = g->engs[i];
            if (status_out[i] != KS_OK || !part[i]) continue;
            const ks::BindSeg& sg = g->h_seg[i];
            status_out[i] = step_finish(e, t_end[i], start[i], h_out + sg.off, h_out + total + sg.off,
                                        out ? out + (int64_t)i * cap : nullptr, out ? cap : 0, &n_out[i]);
        }
    };
    // the host's CPU share: OMP_NUM_THREADS when the job sets it (the GPU box does: 16), else the
    // hardware threads, at most 32
    int hw = (int)std::thread::hardware_concurrency();
    if (const char* v = std::getenv("OMP_NUM_THREADS"))
        if (std::atoi(v) > 0) hw = std::atoi(v);
    const int nth = total >= (1 << 18) ? std::min<int>(S, std::clamp<int>(hw, 1, 32)) : 1;
    if (nth <= 1) {
        finish(0, S);
    } else {
        std::vector<std::thread> pool;
        for (int k = 1; k < nth; k++) pool.emplace_back(finish, (int)((int64_t)S * k / nth), (int)((int64_t)S * (k + 1) / nth));
        finish(0, (int)((int64_t)S / nth));
        for (auto& th : pool) th.join();
    }
    if (stats) {
        *stats = ks_step_stats{};
        stats->step_ms = ms;
        stats->launches = launches;
        for (int i = 0; i < S; i++) stats->pods += n_out[i];
    }
    return KS_OK;
}

}  // extern "C"
