// ks_engine.cpp — host side of the C-ABI declared in include/ks_engine.h: create / destroy, load,
// submit, scenario groups' life cycle, node sharding, debug and statistics.  The engine record is in
// ks_host.h, the owners that release its GPU resources in ks_own.h (engine_free only waits and deletes);
// ks_step and ks_group_step are in ks_step.cpp; the entry points that answer about a run after the fact (filter / score, usage,
// past-tick state, headroom, name-keyed lookups) are in ks_queries.cpp, the five previews in
// ks_previews.cpp, the device self-tests in ks_selftest.cpp.
//
// Host responsibilities (everything that is independent of placements):
//  * FIFO + one-pod-per-tick: the bind tick of pod j is max(bind_tick[j-1] + 1, arrival_j)
//    (kubesim/kubesim.go:105-121 pops at most one pod per tick and always binds it), so bind
//    ticks are fixed at submit time (bind_tick below).
//  * expiry schedule: a bound-Ok pod q runs while (t - t0) * tick < Σ phase seconds
//    (kubesim/pod/pod.go:67-69), i.e. for dur = ceil(S / tick) ticks (run_ticks below).  Its
//    expiry is attached to the first later pod whose bind tick reaches t0 + dur; the device applies
//    it (if q was bound Ok) right before that pod is scheduled (ks_submit_pods).
//  * resource scale: quantities arrive in milli-units; the device holds resource k in units of
//    g_k = gcd of every capacity and request of k seen so far (exact: every fit / LeastRequested
//    / BalancedAllocation result is unit-free).  A pod whose request g_k does not divide shrinks
//    the unit (rescale_kernel multiplies the device state by g_k / g_k').  When every scaled
//    capacity is < 2^29 the kernels use the narrow (32-bit) evaluator, when moreover every scaled
//    capacity and the largest cpu x memory product are < 2^26 the tiny (int32-only) one, else
//    the 64/128-bit one.
//  * batching: launches (expire_head, scan, merge, resolve) until the device counter says
//    every pod due in [tick+1, tick+ticks] is bound, then copies the binds back.
//  * node sharding (ks_shard): every rank holds the whole node state and runs
//    the identical resolver; rank r scans only its contiguous block range, merges it to a
//    per-pod top-L, and one RCCL all-gather per batch exchanges the [B][L] lists, which a
//    second merge reduces to the exact global top-L (the union of exact per-shard top-L lists
//    contains the global top-L).  Binds are then identical on every rank with no further
//    exchange.  Virtual shards (several parts per rank) run the same merge path on one GPU.
// Placements themselves are decided on the device only.
#include <cmath>
#include <numeric>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "ks_host.h"

using namespace ks_host;

ks_status ks_host::fail(ks_engine* e, ks_status code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) e->errmsg = buf;
    return code;
}

namespace {

constexpr int64_t kMaxNodes = 1LL << 24;  // node ids fit the packed key; lists stay < 2^31 entries
constexpr int kMaxBatch = 256;
constexpr int kChunkBatch = 192;  // default batch of engines on the chunk resolver (ks_load_nodes)
constexpr int64_t kStageMaxPods = 4096;  // submits of up to this many pods are host-staged
#ifndef KS_PG_MIN_WG
#define KS_PG_MIN_WG 2048  // scan workgroups to keep when raising the pods per workgroup
#endif

// ks_destroy's body; a group frees its members with it
void engine_free(ks_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    // every stream that may still work on the engine's buffers, before the owners release anything
    for (hipStream_t s : {e->st, e->pipe ? (hipStream_t)e->pipe->st2 : nullptr,
                          e->early ? (hipStream_t)e->early->st_copy : nullptr})
        if (s) (void)hipStreamSynchronize(s);
    delete e;
}

}  // namespace

// Pod.passedSeconds is int32(clock.Sub(start).Seconds()) (kubesim/pod/pod.go:148-153): past 2^31
// seconds Go's float -> int32 conversion is implementation-defined (amd64: INT32_MIN, so
// IsRunning, pod.go:67-69, would revive every finished pod).  The engine's domain: every tick at
// which a bound pod is evaluated stays below 2^31 seconds after the run's first bind; steps,
// submits and usage queries past it are refused with KS_ERANGE (the oracle refuses the same).
bool ks_host::in_passed_domain(const ks_engine* e, int64_t first_bind, int64_t t) {
    return t - first_bind <= (int64_t)INT32_MAX / e->cfg.tick_seconds;
}

ks::EngineArgs ks_host::make_args(ks_engine* e) {
    ks::EngineArgs a{};
    a.c = e->dc;
    a.s = e->s;
    a.pods = e->pods.p;
    a.dur = e->dur.p;
    a.exp_off = e->exp_off.p;
    a.exp_pod = e->exp_pod.p;
    a.exp_pos = e->exp_pos.p;
    a.b_node = e->b_node.p;
    a.b_status = e->b_status.p;
    a.expired = e->expired.p;
    a.lists = e->lists;
    a.cand = e->cand;
    a.nblk = e->nblk;
    a.blk_lo = e->blk_lo;
    a.blk_n = e->blk_n;
    a.ctr = e->d_ctr;
    a.B = e->B;
    a.PG = e->PG;
    if (const WindowWs* w = e->win ? &*e->win : nullptr) {
        a.sw = w->d_sweep; a.e_idx = w->d_eidx; a.n_slot = w->d_nslot; a.n_first = w->d_first; a.spec_ctr = w->d_spec;
    }
    a.det_cids = e->world * e->vsh > 1 ? 1 : 0;
    if (e->prune) { a.lbit = e->bits->lbit; a.lthr = e->bits->lthr; }
    a.nwl = e->nwl;
    a.lset = 1;  // the engine's own scans (the speculative scan's record: set 0, ks_step.cpp upload_args)
    a.srec = e->srec.p;
    a.ncst = e->d_ncst;
    a.two_launch = 0;  // (ks_step.cpp upload_args sets it for the chain the step runs)
    a.e_lim = (e->flags & KS_ENGINE_SMALL_E) ? ks::kSmallE : ks::kEMax;
    return a;
}

namespace {

// ---- host-staged submits ---------------------------------------------------------------------
// Staged rows are applied in submission order by one scatter launch (stage_flush) or by the
// per-tick kernel, always before the device work that reads them (stream order).  The arena is
// reused once the launch that consumed its last segment has completed.

// room for `bytes` more in the arena and one more segment
hipError_t stage_room(ks_engine* e, int64_t bytes) {
    if (e->nseg > 0 && e->seg_done == e->nseg && hipEventQuery(e->stage_ev) == hipSuccess) {
        e->stage_used = 0;
        e->nseg = e->seg_done = 0;
    }
    const int64_t cap = e->arena ? e->arena->cap : 0;
    if (e->stage_used + bytes + 16 <= cap && e->nseg < kSegCap) return hipSuccess;
    KS_TRY(stage_flush(e));
    KS_TRY(hipStreamSynchronize(e->st));
    e->stage_used = 0;
    e->nseg = e->seg_done = 0;
    if (bytes + 16 <= cap) return hipSuccess;
    e->arena.reset();  // (freed before the larger one is made)
    return ks_own::build(e->arena, [&](StageArena& a) {
        a.cap = std::max<int64_t>(bytes + 16, std::max<int64_t>(2 * cap, 1 << 20));
        KS_TRY(ks_own::pinned_alloc(a.mem, a.cap, hipHostMallocMapped));
        return ks_own::pinned_alloc(a.segs, kSegCap, hipHostMallocMapped);
    });
}

// one staged copy of `bytes` host bytes to device address dst
hipError_t stage_copy(ks_engine* e, void* dst, const void* src, int64_t bytes) {
    if (bytes <= 0) return hipSuccess;
    KS_TRY(stage_room(e, bytes));
    StageArena& a = *e->arena;
    std::memcpy(a.mem + e->stage_used, src, bytes);
    a.segs[e->nseg++] = ks::CopySeg{(uint8_t*)dst, a.mem.dev + e->stage_used, bytes};
    e->stage_used += (bytes + 15) / 16 * 16;
    return hipSuccess;
}

// DVec::append through the arena (growth flushes first: the copy of the old contents must
// follow the staged rows written into them)
template <typename T>
hipError_t stage_append(ks_engine* e, DVec<T>& v, const T* h, int64_t k) {
    if (v.n + k > v.cap) {
        KS_TRY(stage_flush(e));
        KS_TRY(v.reserve(v.n + k, e->st));
    }
    v.n += k;
    return stage_copy(e, v.p + (v.n - k), h, sizeof(T) * k);
}

}  // namespace

// The rows of exp_pos that submits rewrote since the last flush, as one segment from the host
// mirror: per-submit rewrites overlap, and the scatter applies segments in parallel.
hipError_t ks_host::stage_xpos(ks_engine* e) {
    const int64_t lo = e->xpos_lo;
    if (lo >= e->P) return hipSuccess;
    e->xpos_lo = INT64_MAX;
    return stage_copy(e, e->exp_pos.p + lo, e->h_exp_pos.data() + lo, sizeof(int64_t) * (e->P - lo));
}

hipError_t ks_host::stage_flush(ks_engine* e) {
    KS_TRY(stage_xpos(e));
    if (e->seg_done >= e->nseg) return hipSuccess;
    hipError_t r = ks::launch_scatter(e->arena->segs.dev + e->seg_done, e->nseg - e->seg_done, e->st);
    if (r == hipSuccess) r = hipEventRecord(e->stage_ev, e->st);
    e->seg_done = e->nseg;
    return r;
}

bool ks_host::key16(const ks_engine* e) {
    return (int64_t)e->dc.const_total + 10 * ((int64_t)e->dc.w_lr + e->dc.w_ba) + 1 < (1 << 16);
}

bool ks_host::small_resolver(const ks_engine* e) {
    return e->B <= ks::small_resolver_max_batch() && e->dc.n_nodes <= ks::small_resolver_max_nodes();
}

namespace {

// the chunk resolver (the resolvers: ks_plan.h Resolver): node state in 32-bit words (every scaled capacity < 2^32 - 1: the modes >=
// narrow, and the wide mode's decimal-SI memory class, whose capacities scale to 2^31), totals in
// 16 bits
bool chunk_eligible(const ks_engine* e) {
    bool words = e->mode >= ks::kEvalNarrow;
    if (!words) {
        words = true;
        for (int k = 0; k < 3; k++) words &= e->max_alloc[k] / e->scale[k] < (int64_t)0xFFFFFFFF;
    }
    return e->B <= ks::kWinMaxB && words && key16(e);
}

}  // namespace

// an explicit resolver flag wins over the size class (every resolver is exact on every engine
// its limits admit; the flags exist to test them against each other)
int ks_host::resolver_of(const ks_engine* e) {
    if ((e->flags & KS_ENGINE_CHUNK_RESOLVER) && chunk_eligible(e)) return kResolveChunk;
    if (e->flags & KS_ENGINE_ONE_POD_RESOLVER) return kResolveRole;
    // default: the register-table resolver for the small class, else the chunk resolver where
    // its limits admit the engine (C3: 8.8e5 vs 7.2e5 pods/s with the one-pod kernel), else
    // the one-pod kernel
    if (small_resolver(e)) return kResolveSmall;
    return chunk_eligible(e) ? kResolveChunk : kResolveRole;
}

// (the chunk resolver runs fused into the batch chain, ks_step.cpp)
hipError_t ks_host::launch_resolver(const ks::EngineArgs* d, int S, int mode, int which, hipStream_t st) {
    return which == kResolveSmall ? ks::launch_resolve_small(d, S, mode, st) : ks::launch_resolve(d, S, mode, st);
}

// Apply every not-yet-applied expiry with finish tick <= the current tick (ks_filter / ks_score
// see the state Run's next scheduleOne would).  While the run is live the host knows them
// exactly: every expiry attached to a pod < done has been applied (mirror_expired), an expiry
// attached to a later pod j > done finishes after bind_tick[j - 1] >= bind_tick[done] > tick, so
// only the next pod's attached expiries and the unattached ones (pending, when every submitted pod
// is bound) can be due — usually none, and no launch is made.
ks_status ks_host::flush_expiries(ks_engine* e) {
    std::vector<int32_t> qs;
    auto add = [&](int64_t q) {
        if (e->h_status[q] == KS_POD_OK && !e->h_expired[q] && e->h_fin[q] <= e->tick) qs.push_back((int32_t)q);
    };
    if (e->err == KS_OK) {
        if (e->done < e->P)
            for (int64_t u = e->h_exp_off[e->done]; u < e->h_exp_off[e->done + 1]; u++) add(e->h_exp_pod[u]);
        e->pending.for_each_due(e->tick, add);
    }
    if (e->err != KS_OK || (int)qs.size() > ks::kTickMaxExp) {
        HIPCHK(e, ks::launch_flush(e->s, e->pods.p, e->fin.p, e->tick, e->done, e->b_node.p, e->b_status.p,
                                   e->expired.p, e->st));
    } else if (!qs.empty()) {
        ks::ExpList L{};
        for (int32_t q : qs) {
            ks::TickExp& x = L.x[L.n++];
            x.node = e->h_node[q];
            x.q = q;
            for (int k = 0; k < 3; k++) x.req[k] = e->h_pods[q].req[k];
        }
        HIPCHK(e, ks::launch_apply_exp(e->s, e->expired.p, L, e->st));
    }
    for (int32_t q : qs) e->h_expired[q] = 1;
    return KS_OK;
}

namespace {

void update_mode(ks_engine* e) {
    int64_t m[3];
    for (int k = 0; k < 3; k++) m[k] = e->max_alloc[k] / e->scale[k];
    const bool narrow = m[0] < ks::kNarrowCap && m[1] < ks::kNarrowCap && m[2] < ks::kNarrowCap;
    const bool tiny = m[0] < ks::kTinyCap && m[1] < ks::kTinyCap && m[2] < ks::kTinyCap && m[0] * m[1] < ks::kTinyCap;
    const bool micro = m[0] < ks::kMicroCap && m[1] < ks::kMicroCap && m[2] < ks::kMicroCap &&
                       m[0] * m[1] < ks::kMicroProd && e->dc.w_lr < ks::kMicroWeight &&
                       e->dc.w_ba < ks::kMicroWeight;
    const bool no_tiny = (e->flags & KS_ENGINE_NO_TINY) != 0;
    e->mode = (e->flags & KS_ENGINE_FORCE_WIDE) ? ks::kEvalWide
            : (micro && !no_tiny && !(e->flags & KS_ENGINE_NO_MICRO)) ? ks::kEvalMicro
            : (tiny && !no_tiny) ? ks::kEvalTiny
            : narrow ? ks::kEvalNarrow : ks::kEvalWide;
}

// Validation and host-side construction shared by ks_create and ks_group_add (no HIP calls).
ks_status engine_init(const ks_config* cfg, ks_engine** out) {
    if (!cfg || !out) return KS_EINVAL;
    *out = nullptr;
    if (cfg->abi_version != KS_ABI_VERSION) return KS_EINVAL;
    if (cfg->tick_seconds < 1) return KS_EINVAL;
    if (cfg->filter_mode != KS_FILTER_REFERENCE_LITERAL && cfg->filter_mode != KS_FILTER_FEEDS_SCORE)
        return KS_EINVAL;
    if (cfg->filters & ~7u) return KS_EINVAL;
    if (cfg->n_scorers < 0 || cfg->n_scorers > 8) return KS_EINVAL;
    if (cfg->batch_pods < 0 || cfg->batch_pods > kMaxBatch) return KS_EINVAL;
    if (cfg->engine_flags &
        ~(uint32_t)(KS_ENGINE_FORCE_WIDE | KS_ENGINE_NO_TINY | KS_ENGINE_NO_MICRO | KS_ENGINE_ONE_POD_RESOLVER |
                    KS_ENGINE_CHUNK_RESOLVER | KS_ENGINE_NO_OVERLAP | KS_ENGINE_PRUNED_LISTS | KS_ENGINE_SMALL_E))
        return KS_EINVAL;
    int64_t const_total = 0, w_lr = 0, w_ba = 0;
    for (int i = 0; i < cfg->n_scorers; i++) {
        const ks_scorer& sc = cfg->scorers[i];
        if (sc.weight < 0) return KS_EINVAL;
        switch (sc.kind) {
            case KS_SCORER_CONST:
                if (sc.value < 0) return KS_EINVAL;
                const_total += (int64_t)sc.weight * sc.value;
                break;
            case KS_SCORER_LEAST_REQUESTED: w_lr += sc.weight; break;
            case KS_SCORER_BALANCED: w_ba += sc.weight; break;
            default: return KS_EINVAL;
        }
    }
    if (const_total + 10 * (w_lr + w_ba) >= (1LL << 30) - 2) return KS_EINVAL;  // total + 1 < 2^30 (resolver ikey)

    ks_engine* e = new ks_engine();
    e->cfg = *cfg;
    e->device = cfg->device;
    e->B = cfg->batch_pods ? cfg->batch_pods : kDefaultBatch;
    e->flags = cfg->engine_flags;
    e->overlap = !(cfg->engine_flags & KS_ENGINE_NO_OVERLAP);
    e->dc.filter_feeds = cfg->filter_mode == KS_FILTER_FEEDS_SCORE;
    e->dc.filters = cfg->filters;
    e->dc.has_scorers = cfg->n_scorers > 0;
    e->dc.w_lr = (int32_t)w_lr;
    e->dc.w_ba = (int32_t)w_ba;
    e->dc.const_total = (int32_t)const_total;
    e->dc.tick_seconds = cfg->tick_seconds;
    *out = e;
    return KS_OK;
}

// ---- ks_submit_pods' rules, each defined once --------------------------------------------------
constexpr int64_t kNever = std::numeric_limits<int64_t>::max();
// the arrival the bind-tick recurrence uses: a pod submitted late arrives at the next tick
int64_t eff_arrival(int64_t arrival, int64_t tick) { return std::max(arrival, tick + 1); }
// FIFO, one pod per tick: the bind tick of the pod after one bound at prev
int64_t bind_tick(int64_t prev, int64_t arrival, int64_t tick) { return std::max(prev + 1, eff_arrival(arrival, tick)); }
// Σ seconds of phases [lo, hi): S wraps int32 as Pod.totalSeconds does (kubesim/pod/pod.go:155-162), wide
// does not; cum (optional) takes the wrapping running sums
struct PhaseSum { int32_t S; int64_t wide; bool nonneg; };
PhaseSum phase_sum(const int32_t* sec, int32_t lo, int32_t hi, int32_t* cum = nullptr) {
    uint32_t acc = 0;
    PhaseSum s{0, 0, true};
    for (int32_t f = lo; f < hi; f++) {
        acc += (uint32_t)sec[f];
        s.wide += sec[f];
        s.nonneg &= sec[f] >= 0;
        if (cum) cum[f] = (int32_t)acc;
    }
    s.S = (int32_t)acc;
    return s;
}
// the ticks a pod of S total seconds runs: while (t - t0) * tick < S, i.e. ceil(S / tick); none for S <= 0
int64_t run_ticks(int32_t S, int64_t tick_seconds) { return S > 0 ? ((int64_t)S + tick_seconds - 1) / tick_seconds : 0; }

}  // namespace

extern "C" {

ks_status ks_create(const ks_config* cfg, ks_engine** out) {
    ks_engine* e = nullptr;
    const ks_status v = engine_init(cfg, &e);
    if (v != KS_OK) return v;
    hipError_t r = hipSetDevice(e->device);
    if (r == hipSuccess) r = ks_own::stream_create(e->own.st);
    if (r == hipSuccess) r = ks_own::dev_alloc(e->own.d_ctr, 32);
    if (r == hipSuccess) r = ks_own::pinned_alloc(e->own.h_ctr, 32);
    if (r == hipSuccess) r = ks_own::dev_alloc(e->own.d_args, 1);
    if (r == hipSuccess) r = ks_own::pinned_alloc(e->own.h_args, 1);
    for (int i = 0; i < 4 && r == hipSuccess; i++) r = ks_own::event_create(e->ev[i]);
    if (r == hipSuccess) r = ks_own::event_create(e->stage_ev, hipEventDisableTiming);
    e->st = e->own.st; e->d_ctr = e->own.d_ctr; e->h_ctr = e->own.h_ctr;  // the views of its own
    e->d_args = e->own.d_args; e->h_args = e->own.h_args;
    if (r == hipSuccess) r = hipMemsetAsync(e->d_ctr, 0, 32 * sizeof(int64_t), e->st);
    if (r == hipSuccess) r = hipStreamSynchronize(e->st);
    if (r != hipSuccess) {
        engine_free(e);
        return KS_EDEVICE;
    }
    *out = e;
    return KS_OK;
}

// a group's members are destroyed with their group (ks_group_destroy)
void ks_destroy(ks_engine* e) {
    if (e && !e->group) engine_free(e);
}

ks_status ks_comm_unique_id(uint8_t* id_out) {
    if (!id_out) return KS_EINVAL;
    ncclUniqueId uid;
    if (ncclGetUniqueId(&uid) != ncclSuccess) return KS_EDEVICE;
    static_assert(sizeof(uid) == KS_COMM_ID_BYTES, "RCCL unique id size");
    std::memcpy(id_out, &uid, sizeof uid);
    return KS_OK;
}

ks_status ks_shard(ks_engine* e, int32_t world, int32_t rank, const uint8_t* id, int32_t vshards) {
    if (!e) return KS_EINVAL;
    if (e->nodes_loaded) return fail(e, KS_EINVAL, "ks_shard must precede ks_load_nodes");
    if (e->comm) return fail(e, KS_EINVAL, "already sharded");
    if (world < 1 || rank < 0 || rank >= world || vshards < 1 || (int64_t)world * vshards > 4096)
        return fail(e, KS_EINVAL, "bad shard geometry world=%d rank=%d vshards=%d", world, rank, vshards);
    if (world > 1 && !id) return fail(e, KS_EINVAL, "world > 1 needs a communicator id");
    HIPCHK(e, hipSetDevice(e->device));
    if (id) {
        ncclUniqueId uid;
        std::memcpy(&uid, id, sizeof uid);
        const ncclResult_t r = ks_own::comm_init(e->comm, world, uid, rank);
        if (r != ncclSuccess) return fail(e, KS_EDEVICE, "ncclCommInitRank: %s", ncclGetErrorString(r));
    }
    e->world = world;
    e->rank = rank;
    e->vsh = vshards;
    return KS_OK;
}

ks_status ks_shard_host(ks_engine* e, int32_t world, int32_t rank, int32_t vshards, ks_allgather_fn fn, void* user) {
    if (!e) return KS_EINVAL;
    if (e->nodes_loaded) return fail(e, KS_EINVAL, "ks_shard_host must precede ks_load_nodes");
    if (e->comm || e->xfn) return fail(e, KS_EINVAL, "already sharded");
    if (!fn || world < 1 || rank < 0 || rank >= world || vshards < 1 || (int64_t)world * vshards > 4096)
        return fail(e, KS_EINVAL, "bad host-exchange shard geometry world=%d rank=%d vshards=%d", world, rank, vshards);
    e->world = world;
    e->rank = rank;
    e->vsh = vshards;
    e->xfn = fn;
    e->xuser = user;
    return KS_OK;
}

ks_status ks_merge_candidates(const uint64_t* cand_all, int32_t parts, int32_t B, uint64_t* out) {
    if (!cand_all || !out || parts < 1 || B < 0) return KS_EINVAL;
    constexpr int L = ks::kTopL;
    for (int64_t b = 0; b < B; b++) {
        uint64_t top[L] = {};
        for (int64_t p = 0; p < parts; p++) {
            uint64_t lv[L];
            std::memcpy(lv, cand_all + (p * B + b) * L, sizeof(lv));
            ks::topl_insert(top, lv);
        }
        std::memcpy(out + b * L, top, sizeof(top));
    }
    return KS_OK;
}

ks_status ks_shard_layout(int64_t n_nodes, int32_t world, int32_t vshards, int32_t* part_lo_out) {
    if (!part_lo_out || n_nodes < 0 || n_nodes > kMaxNodes || world < 1 || vshards < 1 || (int64_t)world * vshards > 4096)
        return KS_EINVAL;
    const int64_t n_pad = std::max<int64_t>(64, (n_nodes + 63) / 64 * 64);
    const int64_t nblk = (n_pad + ks::block_nodes() - 1) / ks::block_nodes();
    const int G = world * vshards;
    for (int p = 0; p <= G; p++) part_lo_out[p] = (int32_t)((int64_t)p * nblk / G);
    return KS_OK;
}

ks_status ks_load_nodes(ks_engine* e, int64_t n, const int64_t* alloc, const uint64_t* taint, const uint64_t* label) {
    if (!e) return KS_EINVAL;
    if (e->nodes_loaded) return fail(e, KS_EINVAL, "nodes already loaded");
    if (n < 0 || n > kMaxNodes) return fail(e, KS_EINVAL, "node count %lld outside [0, %lld]", (long long)n, (long long)kMaxNodes);
    if (n && (!alloc || !taint || !label)) return fail(e, KS_EINVAL, "null node buffer");
    for (int64_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++)
            if (alloc[i * 4 + k] < -1 || alloc[i * 4 + k] >= kMaxValue)
                return fail(e, KS_EINVAL, "node %lld: capacity %d out of range", (long long)i, k);
        if (alloc[i * 4 + 3] < 0 || alloc[i * 4 + 3] >= kMaxValue)
            return fail(e, KS_EINVAL, "node %lld: pods capacity out of range", (long long)i);
    }
    HIPCHK(e, hipSetDevice(e->device));
    e->n = n;
    e->n_pad = std::max<int64_t>(64, (n + 63) / 64 * 64);
    e->nwb = (int)(e->n_pad / 64);
    const int64_t np = e->n_pad;
    // host staging in SoA order: ac am ag ap rc rm rg nr taint label
    for (int k = 0; k < 3; k++) {
        int64_t g = 0, mx = 0;
        for (int64_t i = 0; i < n; i++) {
            const int64_t v = alloc[i * 4 + k];
            if (v > 0) { g = std::gcd(g, v); mx = std::max(mx, v); }
        }
        e->scale[k] = g > 0 ? g : 1;
        e->max_alloc[k] = mx;
    }
    update_mode(e);
    std::vector<int64_t> h(10 * np, 0);
    for (int64_t i = 0; i < np; i++) {
        const bool real = i < n;
        for (int k = 0; k < 4; k++) h[k * np + i] = real ? alloc[i * 4 + k] : (k == 3 ? 0 : -1);
        for (int k = 0; k < 3; k++)
            if (real && h[k * np + i] > 0) h[k * np + i] /= e->scale[k];
        h[8 * np + i] = real ? (int64_t)taint[i] : 0;
        h[9 * np + i] = real ? (int64_t)label[i] : 0;
    }
    HIPCHK(e, ks_own::dev_alloc(e->node_mem, 10 * np));
    HIPCHK(e, hipMemcpyAsync(e->node_mem, h.data(), sizeof(int64_t) * 10 * np, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, ks_own::dev_alloc(e->d_ncst, 2 * np));
    int64_t* b = e->node_mem;
    e->s.ac = b; e->s.am = b + np; e->s.ag = b + 2 * np; e->s.ap = b + 3 * np;
    e->s.rc = b + 4 * np; e->s.rm = b + 5 * np; e->s.rg = b + 6 * np; e->s.nr = b + 7 * np;
    e->s.taint = (uint64_t*)(b + 8 * np); e->s.label = (uint64_t*)(b + 9 * np);
    e->dc.n_nodes = (int32_t)n;
    e->dc.nwb = e->nwb;
    e->nblk = (int)((e->n_pad + ks::block_nodes() - 1) / ks::block_nodes());
    const int G = e->world * e->vsh;
    e->part_lo.assign(G + 1, 0);
    (void)ks_shard_layout(n, e->world, e->vsh, e->part_lo.data());
    e->blk_lo = e->part_lo[e->rank * e->vsh];
    e->blk_n = e->part_lo[(e->rank + 1) * e->vsh] - e->blk_lo;
    // default batch: small clusters exhaust a pod's top-L list after fewer binds, so a batch of
    // 256 would mostly commit early and rescan; ~n/16 pods rounded down to a multiple of 32
    // (>= 64) keeps most of each batch (C4's 2,000-node scenarios: 96 pods 2.64e11 evals/s, 128
    // pods 2.57e11, 64 pods 2.56-2.63e11; round 1: 256 pods 6.1e7 pods/s vs 128 pods 7.9e7)
    if (!e->cfg.batch_pods && n < 16 * kDefaultBatch)
        e->B = (int)std::clamp<int64_t>(n / 16 / 32 * 32, 64, kDefaultBatch);
    // the chunk resolver's default batch: three 64-pod chunks.  Its per-chunk cache of earlier
    // binds grows with the chunk's position, and 256-pod batches hit the candidate-id table
    // (~215 pods committed): 192 pods binds more per second on C3 (9.96e5 vs 9.12e5 pods/s,
    // 224: 9.53e5, 176: 9.64e5, 128: 9.49e5) and C5 (3.67e5 vs 3.19e5; tests/dev/ab_resolvers.py)
    if (!e->cfg.batch_pods && !e->group && !small_resolver(e) && chunk_eligible(e) &&
        !(e->flags & KS_ENGINE_ONE_POD_RESOLVER))
        e->B = kChunkBatch;
    // pods per scan workgroup: the most pod reuse per node load that still leaves >= ~2048
    // workgroups (8 per CU) per scan
    int pg = 1;
    while (pg < ks::max_pods_per_scan_wg() && pg < e->B &&
           (int64_t)e->blk_n * ((e->B + pg * 2 - 1) / (pg * 2)) >= KS_PG_MIN_WG)
        pg *= 2;
    e->PG = pg;
    // (the two-launch chain's engines may scan lists of kTopLOverlap keys: ks_plan.h plan_step)
    // (and the pipelined sharded engines': every sharded engine may)
    const int lmax = (G == 1 && e->blk_n <= kOverlapMaxBlocks) || G > 1 ? ks::kTopLOverlap : ks::kTopL;
    HIPCHK(e, ks_own::dev_alloc(e->lists, (size_t)e->B * e->nblk * lmax));
    HIPCHK(e, ks_own::dev_alloc(e->cand, (size_t)e->B * ks::kTopL));
    if (G > 1) HIPCHK(e, ks_own::dev_alloc(e->cand_all, (size_t)G * e->B * ks::kTopLOverlap));
    if (G > 1 && e->xfn) HIPCHK(e, ks_own::pinned_alloc(e->h_xbuf, (size_t)G * e->B * ks::kTopLOverlap));
    HIPCHK(e, ks_own::dev_alloc(e->d_mask, std::max<int64_t>(n, 1)));
    HIPCHK(e, ks_own::dev_alloc(e->d_score, std::max<int64_t>(n, 1)));
    HIPCHK(e, ks_own::dev_alloc(e->d_usage, 3 * std::max<int64_t>(n, 1)));
    HIPCHK(e, hipStreamSynchronize(e->st));
    e->nodes_loaded = true;
    return KS_OK;
}

ks_status ks_submit_pods(ks_engine* e, int64_t m, const int64_t* arrival, const int64_t* req, const uint8_t* keymask,
                         const uint64_t* tol, const uint64_t* sel, const int32_t* phase_off, const int32_t* phase_sec,
                         const int64_t* phase_use, const uint8_t* flags, const int64_t* key_id) {
    if (!e) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "ks_load_nodes must precede ks_submit_pods");
    if (m < 0) return fail(e, KS_EINVAL, "negative pod count");
    if (m == 0) return KS_OK;
    if (!arrival || !req || !keymask || !tol || !sel || !phase_off) return fail(e, KS_EINVAL, "null pod buffer");
    if (e->P + m >= (1LL << 31)) return fail(e, KS_EINVAL, "too many pods");
    if (phase_off[0] != 0) return fail(e, KS_EINVAL, "phase_off[0] must be 0");
    const int64_t nf = phase_off[m];
    if (nf && (!phase_sec || !phase_use)) return fail(e, KS_EINVAL, "null phase buffer");
    // validate first, mutate after
    int64_t last = e->last_arrival;
    for (int64_t i = 0; i < m; i++) {
        if (arrival[i] < last) return fail(e, KS_EINVAL, "arrival ticks must be non-decreasing (pod %lld)", (long long)(e->P + i));
        last = arrival[i];
        if (phase_off[i + 1] < phase_off[i]) return fail(e, KS_EINVAL, "phase_off must be non-decreasing");
        if (key_id && key_id[i] < 0) return fail(e, KS_EINVAL, "pod %lld: key ids must be >= 0", (long long)(e->P + i));
        for (int k = 0; k < 3; k++)
            if (req[i * 3 + k] < 0 || req[i * 3 + k] >= kMaxValue)
                return fail(e, KS_EINVAL, "pod %lld: request out of range", (long long)(e->P + i));
    }
    for (int64_t f = 0; f < nf * 3; f++)
        if (phase_use[f] < 0 || phase_use[f] >= kMaxValue) return fail(e, KS_EINVAL, "usage out of range");
    // the int32 passed-seconds domain (kubesim/pod/pod.go:148-153): every bind tick must stay
    // within 2^31 seconds of the run's first bind
    const int64_t last_bind = e->P ? e->h_bind_tick[e->P - 1] : e->tick;
    const int64_t first = e->P ? e->h_bind_tick[0] : bind_tick(last_bind, arrival[0], e->tick);
    for (int64_t i = 0, pb = last_bind; i < m; i++) {
        pb = bind_tick(pb, arrival[i], e->tick);
        if (!in_passed_domain(e, first, pb))
            return fail(e, KS_ERANGE, "pod %lld: bind tick %lld is %lld ticks after the first bind (tick %lld): "
                        "(t - t0) * %d s reaches 2^31 and Go's int32(passed seconds) leaves its domain",
                        (long long)(e->P + i), (long long)pb, (long long)(pb - first), (long long)first,
                        e->cfg.tick_seconds);
    }
    // Pod keys: a Store over a same-key pod that is still running on the chosen node would drop
    // that pod from the node's totals (kubesim/node/node.go:58).  Refuse the one case where that
    // can happen — an earlier pod with the key may still run at this pod's bind tick — so every
    // accepted trace schedules exactly as the reference (ks_engine.h, ks_submit_pods).
    std::unordered_map<int64_t, int64_t> new_end;  // this call's keys -> latest run end
    for (int64_t i = 0, bt = last_bind; key_id && i < m; i++) {
        bt = bind_tick(bt, arrival[i], e->tick);
        int64_t prev = std::numeric_limits<int64_t>::min();
        auto it = new_end.find(key_id[i]);
        if (it != new_end.end()) prev = it->second;
        else if (auto jt = e->key_end.find(key_id[i]); jt != e->key_end.end()) prev = jt->second;
        if (prev > bt)
            return fail(e, KS_ERANGE, "pod %lld: key %lld reused at bind tick %lld while an earlier pod with it may run "
                        "until tick %lld (Store would replace a running pod: outside the exact domain)",
                        (long long)(e->P + i), (long long)key_id[i], (long long)bt, (long long)prev);
        const int32_t S = phase_sum(phase_sec, phase_off[i], phase_off[i + 1]).S;
        new_end[key_id[i]] = std::max(prev, bt + run_ticks(S, e->cfg.tick_seconds));
    }

    {
        int64_t f[3] = {1, 1, 1};
        bool any = false;
        for (int k = 0; k < 3; k++) {
            int64_t g = e->scale[k];
            for (int64_t i = 0; i < m; i++)
                if ((keymask[i] >> k & 1) && req[i * 3 + k] > 0) g = std::gcd(g, req[i * 3 + k]);
            f[k] = e->scale[k] / g;
            any |= f[k] != 1;
            e->scale[k] = g;
        }
        if (any) {
            HIPCHK(e, hipSetDevice(e->device));
            HIPCHK(e, stage_flush(e));
            HIPCHK(e, ks::launch_rescale(e->s, e->n_pad, e->pods.p, e->P, f, e->st));
            HIPCHK(e, hipStreamSynchronize(e->st));
            for (ks::PodRec& r : e->h_pods)
                for (int k = 0; k < 3; k++) r.req[k] *= f[k];
            update_mode(e);
            if (e->P) {  // the scan records of the rescaled requests
                std::vector<ks::ScanRec> sr(e->P);
                for (int64_t q = 0; q < e->P; q++) sr[q] = ks::scan_rec_micro(e->dc, e->h_pods[q]);
                HIPCHK(e, hipMemcpy(e->srec.p, sr.data(), sizeof(ks::ScanRec) * e->P, hipMemcpyHostToDevice));
            }
        }
    }
    std::vector<ks::PodRec> recs(m);
    std::vector<ks::ScanRec> srecs(m);
    std::vector<int32_t> dur(m), poff(m), cum(nf), tsec(m), neg(m, -1), epod;
    std::vector<int64_t> t0(m), fin(m), eoff(m), run_end(m);
    std::vector<int64_t> arr_eff(m);  // the arrival the recurrence uses (ks_cluster_series' pending column)
    std::vector<uint8_t> reg(m), zero(m, 0);
    epod.reserve(m);
    const int64_t epod_base = e->exp_pod.n;
    e->h_exp_pos.resize(e->P + m, -1);
    int64_t pos_lo = e->P;  // lowest pod whose expiry position changed
    int64_t prev_bind = last_bind;
    for (int64_t i = 0; i < m; i++) {
        const int64_t j = e->P + i;
        ks::PodRec& r = recs[i];
        const uint8_t km = keymask[i] & 7;
        for (int k = 0; k < 3; k++) r.req[k] = (km >> k & 1) ? req[i * 3 + k] / e->scale[k] : 0;
        r.tol = tol[i];
        r.sel = sel[i];
        r.keymask = km;
        r.flags = flags ? flags[i] : 0;
        srecs[i] = ks::scan_rec_micro(e->dc, r);
        arr_eff[i] = eff_arrival(arrival[i], e->tick);
        const int64_t bt = prev_bind = bind_tick(prev_bind, arrival[i], e->tick);
        const PhaseSum ps = phase_sum(phase_sec, phase_off[i], phase_off[i + 1], cum.data());
        const int64_t d = run_ticks(ps.S, e->cfg.tick_seconds);
        tsec[i] = ps.S;
        dur[i] = (int32_t)d;
        t0[i] = bt;
        fin[i] = d > 0 ? bt + d : kNever;
        run_end[i] = bt + d;
        // the digest's segment form: cumulative seconds non-decreasing and (t - t0) * tick never
        // wraps int32 while the pod runs (else the exact per-tick form)
        reg[i] = ps.nonneg && ps.wide <= (int64_t)INT32_MAX - e->cfg.tick_seconds;
        poff[i] = (int32_t)(e->F + phase_off[i]);
        // expiries due before pod j binds: finish tick in (bind_tick[j-1], bind_tick[j]]
        while (!e->pending.empty() && e->pending.top().first <= bt) {
            const int64_t q = e->pending.top().second;
            e->h_exp_pos[q] = epod_base + (int64_t)epod.size();
            pos_lo = std::min(pos_lo, q);
            epod.push_back((int32_t)q);
            e->pending.pop();
        }
        eoff[i] = e->h_exp_off.back() + (int64_t)epod.size();
        if (d > 0) e->pending.push({fin[i], j});
    }
    // device uploads: small submits (a drop-in's per-tick calls) are staged in pinned memory and
    // applied by the next launch (no copy call, no synchronisation here); large ones are copied.  Either
    // way the rows go behind the device arrays they extend in one order: app(v, h, k) appends the k rows at h to v
    hipStream_t st = e->st;
    HIPCHK(e, hipSetDevice(e->device));
    const int32_t tail = (int32_t)(e->F + nf);
    const int64_t z0 = 0, P1 = e->P + m;
    auto rows = [&](auto app) -> ks_status {
        HIPCHK(e, app(e->pods, recs.data(), m));
        HIPCHK(e, app(e->srec, srecs.data(), m));
        HIPCHK(e, app(e->dur, dur.data(), m));
        HIPCHK(e, app(e->t0, t0.data(), m));
        HIPCHK(e, app(e->fin, fin.data(), m));
        HIPCHK(e, app(e->b_node, neg.data(), m));
        HIPCHK(e, app(e->b_status, neg.data(), m));
        HIPCHK(e, app(e->expired, zero.data(), m));
        HIPCHK(e, app(e->preg, reg.data(), m));
        if (e->phase_off.n) e->phase_off.n -= 1;  // phase_off holds P+1 entries: overwrite the sentinel
        HIPCHK(e, app(e->phase_off, poff.data(), m));
        HIPCHK(e, app(e->phase_off, &tail, 1));
        HIPCHK(e, app(e->cum_sec, cum.data(), nf));
        HIPCHK(e, app(e->use, phase_use, nf * 3));
        if (e->exp_off.n == 0) HIPCHK(e, app(e->exp_off, &z0, 1));
        HIPCHK(e, app(e->exp_off, eoff.data(), m));
        HIPCHK(e, app(e->exp_pod, epod.data(), (int64_t)epod.size()));
        return KS_OK;
    };
    if (!e->group && m <= kStageMaxPods) {
        if (ks_status r = rows([&](auto& v, const auto* h, int64_t k) { return stage_append(e, v, h, k); }); r != KS_OK) return r;
        if (e->exp_pos.cap < P1) {
            HIPCHK(e, stage_flush(e));
            HIPCHK(e, e->exp_pos.reserve(P1, st));
        }
        e->xpos_lo = std::min(e->xpos_lo, pos_lo);  // staged at the next flush (stage_xpos)
    } else {
        HIPCHK(e, stage_flush(e));
        if (ks_status r = rows([&](auto& v, const auto* h, int64_t k) { return v.append(h, k, st); }); r != KS_OK) return r;
        HIPCHK(e, e->exp_pos.reserve(P1, st));
        HIPCHK(e, hipMemcpyAsync(e->exp_pos.p + pos_lo, e->h_exp_pos.data() + pos_lo, sizeof(int64_t) * (P1 - pos_lo),
                                 hipMemcpyHostToDevice, st));
        HIPCHK(e, hipStreamSynchronize(st));  // host staging vectors die here
    }
    e->exp_pos.n = P1;
    e->h_pods.insert(e->h_pods.end(), recs.begin(), recs.end());
    e->h_exp_pod.insert(e->h_exp_pod.end(), epod.begin(), epod.end());
    e->h_expired.resize(e->P + m, 0);
    e->h_bind_tick.insert(e->h_bind_tick.end(), t0.begin(), t0.end());
    e->h_fin.insert(e->h_fin.end(), fin.begin(), fin.end());
    e->h_dur.insert(e->h_dur.end(), dur.begin(), dur.end());
    e->h_total_sec.insert(e->h_total_sec.end(), tsec.begin(), tsec.end());
    e->h_exp_off.insert(e->h_exp_off.end(), eoff.begin(), eoff.end());
    // default keys (key_id NULL) live in their own namespace: pod j is key -(j + 1), explicit
    // keys are >= 0, so a mix of both on one engine never aliases
    for (int64_t i = 0; i < m; i++) e->h_key.push_back(key_id ? key_id[i] : -(e->P + i) - 1);
    for (const auto& kv : new_end) e->key_end[kv.first] = kv.second;
    e->h_node.resize(e->P + m, -1);
    e->h_status.resize(e->P + m, -1);
    // run-interval index (usage queries)
    e->h_end.insert(e->h_end.end(), run_end.begin(), run_end.end());
    e->h_arr.insert(e->h_arr.end(), arr_eff.begin(), arr_eff.end());
    for (int64_t q = e->P; q < e->P + m; q++) {
        const int64_t b = q / kUBlk, s = b / kUSup;
        if ((int64_t)e->blk_end.size() <= b) e->blk_end.push_back(std::numeric_limits<int64_t>::min());
        if ((int64_t)e->sup_end.size() <= s) e->sup_end.push_back(std::numeric_limits<int64_t>::min());
        e->blk_end[b] = std::max(e->blk_end[b], e->h_end[q]);
        e->sup_end[s] = std::max(e->sup_end[s], e->h_end[q]);
    }
    e->P += m;
    e->F += nf;
    e->last_arrival = last;
    return KS_OK;
}


// Scenario groups (struct ks_group: ks_host.h; ks_group_step: ks_step.cpp)
ks_status ks_group_create(int32_t device, int32_t max_scenarios, ks_group** out) {
    if (!out || max_scenarios < 1 || max_scenarios > 65535) return KS_EINVAL;
    *out = nullptr;
    ks_group* g = new ks_group();
    g->device = device;
    g->cap = max_scenarios;
    hipError_t r = hipSetDevice(device);
    const size_t S = (size_t)max_scenarios;
    if (r == hipSuccess) r = ks_own::stream_create(g->st);
    if (r == hipSuccess) r = ks_own::stream_create(g->st2);
    if (r == hipSuccess) r = ks_own::event_create(g->xev, hipEventDisableTiming);
    if (r == hipSuccess) r = ks_own::dev_alloc(g->d_ctr, 32 * S);
    if (r == hipSuccess) r = ks_own::pinned_alloc(g->h_ctr, 32 * S);
    if (r == hipSuccess) r = ks_own::dev_alloc(g->d_args, S);
    if (r == hipSuccess) r = ks_own::pinned_alloc(g->h_args, S);
    if (r == hipSuccess) r = ks_own::dev_alloc(g->d_seg, S);
    if (r == hipSuccess) r = ks_own::pinned_alloc(g->h_seg, S);
    for (int i = 0; i < 2 && r == hipSuccess; i++) r = ks_own::event_create(g->ev[i]);
    if (r == hipSuccess) r = hipMemsetAsync(g->d_ctr, 0, sizeof(int64_t) * 32 * max_scenarios, g->st);
    if (r == hipSuccess) r = hipStreamSynchronize(g->st);
    if (r != hipSuccess) {
        ks_group_destroy(g);
        return KS_EDEVICE;
    }
    *out = g;
    return KS_OK;
}

void ks_group_destroy(ks_group* g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    for (ks_engine* e : g->engs) engine_free(e);
    if (g->st2) (void)hipStreamSynchronize(g->st2);
    delete g;
}

ks_status ks_group_add(ks_group* g, const ks_config* cfg, ks_engine** out) {
    if (!g || !cfg || !out) return KS_EINVAL;
    *out = nullptr;
    if ((int)g->engs.size() >= g->cap) return KS_EINVAL;
    if (cfg->device != g->device) return KS_EINVAL;
    ks_engine* e = nullptr;
    const ks_status v = engine_init(cfg, &e);
    if (v != KS_OK) return v;
    const int idx = (int)g->engs.size();
    e->group = g;
    e->st = g->st; e->d_ctr = g->d_ctr + 32 * idx; e->h_ctr = g->h_ctr + 32 * idx;  // the views of the group's
    e->d_args = g->d_args + idx; e->h_args = g->h_args + idx;
    hipError_t r = hipSetDevice(g->device);
    for (int i = 0; i < 4 && r == hipSuccess; i++) r = ks_own::event_create(e->ev[i]);
    if (r != hipSuccess) {
        engine_free(e);
        return KS_EDEVICE;
    }
    g->engs.push_back(e);
    *out = e;
    return KS_OK;
}

int32_t ks_group_size(const ks_group* g) { return g ? (int32_t)g->engs.size() : -1; }


int64_t ks_current_tick(const ks_engine* e) { return e ? e->tick : -1; }
int32_t ks_tick_seconds(const ks_engine* e) { return e ? e->cfg.tick_seconds : -1; }
int64_t ks_queued_pods(const ks_engine* e) { return e ? e->P - e->done : -1; }
const char* ks_last_error(const ks_engine* e) { return e ? e->errmsg.c_str() : "null engine"; }

ks_status ks_last_step_stats(const ks_engine* e, ks_step_stats* out) {
    if (!e || !out) return KS_EINVAL;
    *out = e->stats;
    return KS_OK;
}

ks_status ks_last_step_kernels(const ks_engine* e, ks_kernel_stats* out) {
    if (!e || !out) return KS_EINVAL;
    *out = e->kstats;
    return KS_OK;
}

ks_status ks_debug_counters(ks_engine* e, int64_t* out32) {
    if (!e || !out32) return KS_EINVAL;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(out32, e->d_ctr, 32 * sizeof(int64_t), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
#if !defined(KS_CHUNK_DIAG) && !defined(KS_MCL_DIAG)  // (those builds count in ctr[8], ctr[9] on the device)
    out32[8] = e->early_pods;  // host side: no kernel of the product writes ctr[8] or ctr[9]
    out32[9] = e->snap_pods;
#endif
    return KS_OK;
}

#ifndef KS_SRC_HASH
#define KS_SRC_HASH "unhashed"
#endif
const char* ks_build_id(void) { return KS_SRC_HASH; }

ks_status ks_debug_invariants(ks_engine* e, int64_t* out4) {
    if (!e || !out4) return KS_EINVAL;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!e->win) return KS_OK;  // (no chunk-resolver batch ran: nothing to check)
    HIPCHK(e, hipSetDevice(e->device));
    std::vector<int32_t> ns(e->n_pad), ei(e->n_pad), fi(e->n_pad);
    int32_t hw = 0;
    HIPCHK(e, hipMemcpyAsync(ns.data(), e->win->d_nslot, sizeof(int32_t) * e->n_pad, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(fi.data(), e->win->d_first, sizeof(int32_t) * e->n_pad, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(ei.data(), e->win->d_eidx, sizeof(int32_t) * e->n_pad, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipMemcpyAsync(&hw, &e->win->d_sweep->nslot_hw, sizeof hw, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    for (int64_t i = 0; i < e->n_pad; i++) {
        out4[0] += ns[i] != -1 || fi[i] != ks::kNoFirst;
        out4[1] += ei[i] != -1;
    }
    out4[2] = hw;
    out4[3] = ks::kSlotMax;
    return KS_OK;
}

ks_status ks_debug_window(ks_engine* e, void* out, int64_t cap, int64_t* size_out) {
    if (!e || !size_out) return KS_EINVAL;
    *size_out = (int64_t)sizeof(ks::WinWS);
    if (!e->win || !out || cap <= 0) return KS_OK;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(out, e->win->d_sweep, std::min<int64_t>(cap, sizeof(ks::WinWS)), hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

ks_status ks_debug_watch(ks_engine* e, int64_t pod) {
    if (!e) return KS_EINVAL;
#ifdef KS_BATCH_LOG
    if (ks_status r = ensure_window_ws(e); r != KS_OK || !e->win) return r != KS_OK ? r : KS_EINVAL;  // (chunk resolver only)
    const int32_t w[2] = {(int32_t)pod, 0};
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpyAsync(&e->win->d_sweep->watch_pod, w, sizeof w, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
#else
    (void)pod;
    return KS_EINVAL;  // (a KS_BATCH_LOG diagnostic build only)
#endif
}

void ks_set_profiling(ks_engine* e, int enable) {
    if (e) e->profiling = enable != 0;
}
}  // extern "C"
