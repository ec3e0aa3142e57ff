// ks_host.h — the engine record and the few host functions its translation units share
// (internal: ks_engine.cpp owns the engine's life cycle and loads it, ks_step.cpp steps it,
// ks_queries.cpp and ks_previews.cpp answer about it after the fact; what those two share is
// ks_queries.h).  Every GPU resource of the engine and of a group
// is held by an owner of ks_own.h and released by the record's destructor; what is allocated on first
// use is a bundle in an optional slot, whole or absent (ks_own::build).
#pragma once
#include <algorithm>
#include <functional>
#include <optional>
#include <queue>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ks_engine.h"
#include "ks_device.h"
#include "ks_own.h"
#include "ks_plan.h"

namespace ks_host {

using namespace ks_own;

constexpr int64_t kMaxValue = 1LL << 59;
constexpr int kDefaultBatch = 256;
constexpr int64_t kUBlk = 256;   // usage index: pods per block (= the usage kernels' workgroup)
constexpr int64_t kUSup = 64;    // blocks per super block
constexpr int64_t kMaxDigestTicks = 1 << 20;

// Growable device array (stream-ordered copies on growth); move-only, freed with its holder.
template <typename T>
struct DVec {
    Dev<T> p;
    int64_t n = 0, cap = 0;
    DVec() = default;
    DVec(DVec&& o) noexcept { *this = std::move(o); }
    DVec& operator=(DVec&& o) noexcept {
        p = std::move(o.p), n = std::exchange(o.n, 0), cap = std::exchange(o.cap, 0);
        return *this;
    }
    hipError_t reserve(int64_t want, hipStream_t st) {
        if (want <= cap) return hipSuccess;
        const int64_t nc = std::max<int64_t>(want, std::max<int64_t>(cap * 2, 1024));
        Dev<T> q;  // (freed here when the copy of the old contents fails)
        KS_TRY(ks_own::dev_alloc(q, nc));
        if (n) {
            KS_TRY(hipMemcpyAsync(q, p, sizeof(T) * n, hipMemcpyDeviceToDevice, st));
            KS_TRY(hipStreamSynchronize(st));
        }
        p = std::move(q);
        cap = nc;
        return hipSuccess;
    }
    hipError_t append(const T* h, int64_t k, hipStream_t st) {
        KS_TRY(reserve(n + k, st));
        n += k;
        return k ? hipMemcpyAsync(p + (n - k), h, sizeof(T) * k, hipMemcpyHostToDevice, st) : hipSuccess;
    }
};

// (finish tick, pod) min-heap whose array can be walked: the entries due by a tick are the heap's
// top subtree (flush_expiries visits them without copying or popping the heap)
struct PendingHeap : std::priority_queue<std::pair<int64_t, int64_t>, std::vector<std::pair<int64_t, int64_t>>,
                                         std::greater<std::pair<int64_t, int64_t>>> {
    template <class F>
    void for_each_due(int64_t t, F&& f) const {
        std::vector<size_t> st;
        if (!c.empty() && c[0].first <= t) st.push_back(0);
        while (!st.empty()) {
            const size_t i = st.back();
            st.pop_back();
            f(c[i].second);
            for (size_t k = 2 * i + 1; k <= 2 * i + 2 && k < c.size(); k++)
                if (c[k].first <= t) st.push_back(k);
        }
    }
};

// ---- what an engine makes on first use: one bundle per slot of ks_engine, whole or absent ---------
// pruned block lists (ks_scan.h): per-pod bitmaps of the blocks that wrote a list [2][B][nwl], thresholds [2][kThrCopies][B]
struct PruneBits { Dev<uint64_t> lbit, lthr; };
// the chunk resolver's batch window workspace, and the overlap of the next batch's scan with the
// resolver: the speculative scan's counters, argument records (ctr = d_spec + parity), workgroups
struct WindowWs {
    Dev<ks::WinWS> d_sweep;
    Dev<int32_t> d_eidx;   // node -> E index (n_pad, -1)
    Dev<int32_t> d_nslot;  // node -> candidate slot of the batch (ks_cand.hip), -1
    Dev<int32_t> d_first;  // node -> its first kept entry of the batch, kNoFirst
    Dev<int64_t> d_spec;
    Dev<ks::EngineArgs> d_args_spec;  // [2]: ctr = d_spec + kSpecStride * parity
    Pinned<ks::EngineArgs> h_args_spec;
    int scan_workers = 0;
};
// the pipelined sharded chain (batch_pipe): the next batch's speculative scan, part merges and exchange on a second
// stream beside the resolve; a rescan scans every block locally (d_args_full: every block, the engine's own list set)
struct PipeSet { Stream st2; Event pev_m, pev_x; Dev<ks::EngineArgs> d_args_full; Pinned<ks::EngineArgs> h_args_full; };
// the per-tick path (ks_tick.hip): its scratch and its mapped result (h_tick.dev)
struct TickSet { Dev<ks::TickScratch> d_tick; Pinned<ks::TickOut> h_tick; };
// a batched step's read-back (step_body): the node and status words of its pods [done, p_hi), grown geometrically
struct Readback { Pinned<int32_t> h_bnode, h_bstat; int64_t cap = 0; };
// the copy stream and the event of the early read-back (ks_plan.h early_round)
struct EarlyCopy { Stream st_copy; Event snap_ev; };
// host-staged submits: rows for the device arrays in a mapped arena and the table of kSegCap segments naming
// them, applied by one scatter (or by the per-tick kernel) before any device work reads them
struct StageArena { Pinned<uint8_t> mem; int64_t cap = 0; Pinned<ks::CopySeg> segs; };
constexpr int kSegCap = 1 << 16;
// what ks_create makes for an engine of its own; a group's member borrows the group's (ks_group_add)
struct EngineOwn { Stream st; Dev<int64_t> d_ctr; Pinned<int64_t> h_ctr; Dev<ks::EngineArgs> d_args; Pinned<ks::EngineArgs> h_args; };

}  // namespace ks_host

struct ks_engine {
    template <typename T> using DVec = ks_host::DVec<T>;
    template <typename T> using Dev = ks_own::Dev<T>;
    // The streams' owners first, the communicator right after: members are destroyed in reverse, so every
    // buffer and event goes before the communicator and that before the streams (all waited for by engine_free).
    ks_host::EngineOwn own;
    std::optional<ks_host::PipeSet> pipe;
    std::optional<ks_host::EarlyCopy> early;
    ks_own::Comm comm;

    ks_config cfg{};
    ks::Cfg dc{};
    hipStream_t st = nullptr;
    int device = 0;
    bool profiling = false;

    // nodes
    int64_t n = 0, n_pad = 0;
    int nwb = 0;
    bool nodes_loaded = false;
    Dev<int64_t> node_mem;  // [10][n_pad], the fields of s
    Dev<uint4> d_ncst;      // the node constants table (ks::EngineArgs::ncst), [n_pad][2]
    ks::NodeSoA s{};

    // pods (device)
    DVec<ks::PodRec> pods;
    DVec<int32_t> dur, b_node, b_status, phase_off, cum_sec, exp_pod;
    DVec<int64_t> exp_off, t0, fin, use, exp_pos;
    DVec<uint8_t> expired;
    DVec<ks::ScanRec> srec;  // the pods' scan records (ks_device.h scan_rec_micro), rebuilt on a rescale
    // pods (host mirror of placement-independent facts)
    std::vector<int64_t> h_bind_tick, h_fin;
    std::vector<int64_t> h_exp_off{0};
    std::vector<int32_t> h_dur;
    std::vector<int32_t> h_total_sec;  // Σ phase seconds, int32 wrapping (Pod.totalSeconds)
    ks_host::PendingHeap pending;  // (finish tick, pod) not yet attached to a later pod
    int64_t P = 0, F = 0;
    int64_t last_arrival = 0;
    int64_t scale[3] = {1, 1, 1};   // device unit of cpu / memory / gpu, in milli-units
    int64_t max_alloc[3] = {0, 0, 0};  // largest capacity per resource, milli-units
    int mode = ks::kEvalWide;  // evaluator variant (ks_device.h)
    uint32_t flags = 0;        // KS_ENGINE_*
    std::vector<int64_t> h_exp_pos;  // global exp_pod index holding pod q's own expiry, or -1
    // pod keys (Node.CreatePod's pods.Store(key, pod), kubesim/node/node.go:58)
    std::vector<int64_t> h_key;
    std::unordered_map<int64_t, int64_t> key_end;  // key -> latest run end among pods with it
    // host mirror of the binds (name-keyed queries): node (-1 = not bound) and status
    std::vector<int32_t> h_node;
    std::vector<int8_t> h_status;
    // host mirrors the per-tick path passes by value: device-unit pod records, the expiry CSR's
    // pods, the device's expired flags (exact while err == KS_OK: every expiry attached to a pod
    // < done has been applied, plus the ones a flush applied)
    std::vector<ks::PodRec> h_pods;
    std::vector<int32_t> h_exp_pod;
    std::vector<uint8_t> h_expired;
    // host-staged submits: the arena (rebuilt larger when a submit outgrows it), its fill, the segments applied
    std::optional<ks_host::StageArena> arena;
    int64_t stage_used = 0;
    int nseg = 0, seg_done = 0;
    int64_t xpos_lo = INT64_MAX;        // exp_pos rows [xpos_lo, P) changed since the last flush
    // recorded after the launch that consumed the last segments.  ks_create makes it; a group's member has none
    // and needs none: both its users, the staged submit path and the per-tick path, are closed to members
    ks_own::Event stage_ev;
    std::optional<ks_host::TickSet> tickset;  // per-tick path (ks_tick.hip)
    // name-keyed index over binds [0, idx_upto), extended on each query
    int64_t idx_upto = 0;
    std::vector<std::vector<int64_t>> node_pods;      // per node: every pod bound there, FIFO
    // run-interval index for the usage queries: pod q may run only in [t0, end) (end = t0 when
    // it never runs); per block of kUBlk pods and per super block of kUSup blocks the max end
    std::vector<int64_t> h_end, blk_end, sup_end;
    DVec<uint8_t> preg;  // 1: phases non-negative and no int32 wrap (digest by segments)

    // progress
    int64_t tick = 0, done = 0;
    int err = KS_OK;
    std::string errmsg;

    // batch machinery
    int B = ks_host::kDefaultBatch, PG = 32;
    Dev<uint64_t> lists, cand;
    int nblk = 0;
    // node sharding (comm above: RCCL)
    int world = 1, rank = 0, vsh = 1;
    ks_allgather_fn xfn = nullptr;  // host exchange (ks_shard_host) instead of RCCL
    void* xuser = nullptr;
    ks_own::Pinned<uint64_t> h_xbuf;  // [world][vsh][B][L]
    std::vector<int> part_lo;  // [world * vsh + 1] block boundaries of the parts
    int blk_lo = 0, blk_n = 0;  // this rank's scan range
    Dev<uint64_t> cand_all;  // [world * vsh][B][L]
    // pruned block lists: in use (then bits is there), the words per bitmap
    bool prune = false;
    int L = ks::kTopL;  // the block lists' length (kTopLOverlap: the overlap's single-shard engines)
    std::optional<ks_host::PruneBits> bits;
    int nwl = 0;
    // views all code reads (with st): the counters ([8] of h_ctr: the early read-back's snapshot of the start
    // counter), the kernels' argument record and its pinned host staging — own's, or the group's slots
    int64_t *d_ctr = nullptr, *h_ctr = nullptr;
    ks::EngineArgs *d_args = nullptr, *h_args = nullptr;
    std::optional<ks_host::Readback> rb;
    // the last batched step's binds finished on the host before its last wait, and those of them that
    // came back below a snapshot, on the copy stream
    int64_t early_pods = 0, snap_pods = 0;
    bool overlap = true;  // the next batch's scan beside the chunk resolver (chunk class)
    std::optional<ks_host::WindowWs> win;
    ks_group* group = nullptr;  // group membership (ks_group_add)
    ks_own::Event ev[4];  // (kEvStepBegin ... kEvUsageEnd)
    std::vector<ks_own::Event> prof_ev;
    ks_step_stats stats{};
    ks_kernel_stats kstats{};

    // scratch for queries
    Dev<uint8_t> d_mask;
    Dev<int64_t> d_score;
    Dev<unsigned long long> d_usage;
    DVec<int32_t> d_blk;                  // usage query: candidate pod blocks
    std::vector<int32_t> h_blk;
    DVec<unsigned long long> d_digest;    // [6][T + 1] difference arrays, then the prefix sums
    // past-tick state queries (ks_requested_at ... ks_node_peaks): the arrival tick the bind-tick
    // recurrence used per pod (non-decreasing), prefix counts of Ok / OverCapacity binds over the
    // pods [0, cum_upto) (extended on each query), 64-bit and 32-bit device scratch
    std::vector<int64_t> h_arr;
    std::vector<int64_t> cum_ok{0}, cum_over{0};
    int64_t cum_upto = 0;
    DVec<unsigned long long> d_qs;
    DVec<int32_t> d_qi;
    std::vector<ks::PodRec> h_shapes;  // ks_headroom_*: the call's shape records (requests in milli-units)
};

namespace ks_host {

// ks_engine::ev (the first two: ks_group::ev): a step's first and last stream operation (step_ms), a profiled usage kernel
enum { kEvStepBegin = 0, kEvStepEnd = 1, kEvUsageBegin = 2, kEvUsageEnd = 3 };

// record the message for ks_last_error and return code
ks_status fail(ks_engine* e, ks_status code, const char* fmt, ...);

#define HIPCHK(e, expr)                                                                                        \
    do {                                                                                                       \
        if (hipError_t _r = (expr); _r != hipSuccess)                                                          \
            return ks_host::fail((e), KS_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(_r));              \
    } while (0)

// apply the staged submits (ks_engine.cpp, host-staged submits): before any device work reads them
hipError_t stage_flush(ks_engine* e);
// stage the rows of exp_pos that submits rewrote since the last flush (stage_flush does; the per-tick path inlines them)
hipError_t stage_xpos(ks_engine* e);
// the kernels' argument record of the engine as it stands (ks_engine.cpp)
ks::EngineArgs make_args(ks_engine* e);
// tick t lies in the int32 passed-seconds domain of a run whose first bind is at first_bind
bool in_passed_domain(const ks_engine* e, int64_t first_bind, int64_t t);
// every total + 1 fits the scan's 16-bit key table (weights and constant values are >= 0)
bool key16(const ks_engine* e);
// the small (register-table) resolver holds this engine's batches
bool small_resolver(const ks_engine* e);
// the engine's resolver (Resolver, ks_plan.h): an explicit flag, else by size class
int resolver_of(const ks_engine* e);
// the role-split or the register-table resolver (the chunk resolver runs fused into the batch chain)
hipError_t launch_resolver(const ks::EngineArgs* d, int S, int mode, int which, hipStream_t st);
// the window workspace, pruned-list bitmaps and pipelined chain's set, made on the first step that needs them (ks_step.cpp)
ks_status ensure_window_ws(ks_engine* e);
// apply every not-yet-applied expiry with finish tick <= the current tick (ks_engine.cpp)
ks_status flush_expiries(ks_engine* e);

}  // namespace ks_host

// Scenario groups (BASELINE.json configs[3]): independent what-if clusters stepped together, one
// launch per kernel for all of them (scenario = a grid dimension; one resolve workgroup each).
// ks_engine.cpp creates, fills and destroys them, ks_step.cpp steps them.
struct ks_group {
    int device = 0;
    int cap = 0;
    // the second half of the scenarios runs its batch rounds on its own stream: one half's
    // latency-bound resolvers then share the GPU with the other half's throughput-bound scans
    ks_own::Stream st, st2;  // (first: destroyed last)
    std::vector<ks_engine*> engs;
    // each with its pinned mirror: counters [cap][32], argument records [cap], bind segments [cap]
    ks_own::Dev<int64_t> d_ctr; ks_own::Pinned<int64_t> h_ctr;
    ks_own::Dev<ks::EngineArgs> d_args; ks_own::Pinned<ks::EngineArgs> h_args;
    ks_own::Dev<ks::BindSeg> d_seg; ks_own::Pinned<ks::BindSeg> h_seg;
    struct OutBuf { ks_own::Dev<int32_t> d_out; ks_own::Pinned<int32_t> h_out; int64_t cap = 0; };
    std::optional<OutBuf> out;  // packed binds of a step: node, then status; grown geometrically
    ks_own::Event ev[2];
    ks_own::Event xev;  // argument upload done (st -> st2)
    std::string errmsg;
};
