// ks_host.h — the engine record and the few host functions its translation units share
// (internal: ks_engine.cpp owns the engine's life cycle and loads it, ks_step.cpp steps it,
// ks_queries.cpp answers about it after the fact).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <functional>
#include <queue>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ks_engine.h"
#include "ks_device.h"
#include "ks_plan.h"

namespace ks_host {

constexpr int64_t kMaxValue = 1LL << 59;
constexpr int kDefaultBatch = 256;
constexpr int64_t kUBlk = 256;   // usage index: pods per block (= the usage kernels' workgroup)
constexpr int64_t kUSup = 64;    // blocks per super block
constexpr int64_t kMaxDigestTicks = 1 << 20;

// Growable device array (stream-ordered copies on growth).
template <typename T>
struct DVec {
    T* p = nullptr;
    int64_t n = 0, cap = 0;
    hipError_t reserve(int64_t want, hipStream_t st) {
        if (want <= cap) return hipSuccess;
        int64_t nc = std::max<int64_t>(want, std::max<int64_t>(cap * 2, 1024));
        T* q = nullptr;
        hipError_t e = hipMalloc(&q, sizeof(T) * nc);
        if (e != hipSuccess) return e;
        if (n) {
            e = hipMemcpyAsync(q, p, sizeof(T) * n, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) return e;
            e = hipStreamSynchronize(st);
            if (e != hipSuccess) return e;
        }
        if (p) (void)hipFree(p);
        p = q;
        cap = nc;
        return hipSuccess;
    }
    hipError_t append(const T* h, int64_t k, hipStream_t st) {
        hipError_t e = reserve(n + k, st);
        if (e != hipSuccess) return e;
        if (k) e = hipMemcpyAsync(p + n, h, sizeof(T) * k, hipMemcpyHostToDevice, st);
        n += k;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = cap = 0;
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

}  // namespace ks_host

struct ks_engine {
    template <typename T>
    using DVec = ks_host::DVec<T>;
    ks_config cfg{};
    ks::Cfg dc{};
    hipStream_t st = nullptr;
    int device = 0;
    bool profiling = false;

    // nodes
    int64_t n = 0, n_pad = 0;
    int nwb = 0;
    bool nodes_loaded = false;
    void* node_mem = nullptr;
    uint4* d_ncst = nullptr;  // the node constants table (ks::EngineArgs::ncst), [n_pad][2]
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
    // host-staged submits: rows for the device arrays in a pinned, device-visible arena, applied by
    // one scatter (or by the per-tick kernel) before any device work reads them
    uint8_t* stage = nullptr;           // pinned host arena
    uint8_t* stage_dev = nullptr;       // its device address
    int64_t stage_cap = 0, stage_used = 0;
    ks::CopySeg* segs = nullptr;        // pinned segment table
    ks::CopySeg* segs_dev = nullptr;
    int seg_cap = 0, nseg = 0, seg_done = 0;
    int64_t xpos_lo = INT64_MAX;        // exp_pos rows [xpos_lo, P) changed since the last flush
    hipEvent_t stage_ev = nullptr;      // recorded after the launch that consumed the last segments
    // per-tick path (ks_tick.hip)
    ks::TickScratch* d_tick = nullptr;
    ks::TickOut* h_tick = nullptr;      // pinned, device-visible
    ks::TickOut* h_tick_dev = nullptr;
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
    uint64_t* lists = nullptr;
    uint64_t* cand = nullptr;
    int nblk = 0;
    // node sharding
    int world = 1, rank = 0, vsh = 1;
    ncclComm_t comm = nullptr;
    ks_allgather_fn xfn = nullptr;  // host exchange (ks_shard_host) instead of RCCL
    void* xuser = nullptr;
    uint64_t* h_xbuf = nullptr;     // pinned [world][vsh][B][L]
    std::vector<int> part_lo;  // [world * vsh + 1] block boundaries of the parts
    int blk_lo = 0, blk_n = 0;  // this rank's scan range
    uint64_t* cand_all = nullptr;  // [world * vsh][B][L]
    // pruned block lists (ks_scan.h): per-pod bitmaps of the blocks that wrote a list and thresholds
    bool prune = false;
    int L = ks::kTopL;  // the block lists' length (kTopLOverlap: the overlap's single-shard engines)
    uint64_t* lbit = nullptr;  // [B][nwl]
    uint64_t* lthr = nullptr;  // [2][kThrCopies][B]
    int nwl = 0;
    int64_t* d_ctr = nullptr;
    int64_t* h_ctr = nullptr;  // pinned ([8]: the early read-back's snapshot of the start counter)
    // a batched step's read-back (ks_step.cpp step_body): the node and status words of the step's
    // pods [done, p_hi), pinned, grown geometrically; the copy stream and the event of the early
    // read-back (ks_plan.h early_round)
    int32_t* h_bnode = nullptr;
    int32_t* h_bstat = nullptr;
    int64_t bind_cap = 0;
    hipStream_t st_copy = nullptr;
    hipEvent_t snap_ev = nullptr;
    // the last batched step's binds finished on the host before its last wait, and those of them that
    // came back below a snapshot, on the copy stream
    int64_t early_pods = 0, snap_pods = 0;
    ks::EngineArgs* d_args = nullptr;  // the kernels' argument record (device)
    ks::EngineArgs* h_args = nullptr;  // its pinned host staging
    // overlap of the next batch's scan with the chunk resolver (chunk class, one shard): the
    // speculative scan's argument records (ctr = d_spec + parity) and counters, its workgroups
    bool overlap = true;
    int scan_workers = 0;
    int64_t* d_spec = nullptr;
    ks::EngineArgs* d_args_spec = nullptr;  // [2]: ctr = d_spec + kSpecStride * parity
    ks::EngineArgs* h_args_spec = nullptr;
    // the pipelined sharded chain (round 6, ks_step.cpp batch_pipe): the next batch's speculative scan, per-part
    // merges and exchange on a second stream beside the resolve; a rescan scans every block locally
    // (d_args_full: the whole block range, the engine's own list set)
    hipStream_t st2 = nullptr;
    hipEvent_t pev_m = nullptr, pev_x = nullptr;
    ks::EngineArgs* d_args_full = nullptr;
    ks::EngineArgs* h_args_full = nullptr;
    // group membership (ks_group_add): stream, counters and argument slots belong to the group
    ks_group* group = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // (kEvStepBegin ... kEvUsageEnd)
    std::vector<hipEvent_t> prof_ev;
    ks_step_stats stats{};
    ks_kernel_stats kstats{};

    // scratch for queries
    uint8_t* d_mask = nullptr;
    int64_t* d_score = nullptr;
    ks::WinWS* d_sweep = nullptr;    // batch window workspace and node -> E index (n_pad, -1)
    int32_t* d_eidx = nullptr;
    int32_t* d_nslot = nullptr;      // node -> candidate slot of the batch (ks_cand.hip), -1
    int32_t* d_first = nullptr;      // node -> its first kept entry of the batch, kNoFirst
    unsigned long long* d_usage = nullptr;
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

// ks_engine::ev (and the first two: ks_group::ev): a step's first and last stream operation (ks_step_stats'
// step_ms), a profiled usage query's kernel
enum { kEvStepBegin = 0, kEvStepEnd = 1, kEvUsageBegin = 2, kEvUsageEnd = 3 };

// record the message for ks_last_error and return code
ks_status fail(ks_engine* e, ks_status code, const char* fmt, ...);

#define HIPCHK(e, expr)                                                                              \
    do {                                                                                             \
        hipError_t _r = (expr);                                                                      \
        if (_r != hipSuccess)                                                                        \
            return ks_host::fail((e), KS_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(_r));    \
    } while (0)

// apply the staged submits (ks_engine.cpp, host-staged submits): before any device work reads them
hipError_t stage_flush(ks_engine* e);
// stage the rows of exp_pos that submits rewrote since the last flush (stage_flush does; the per-tick
// path passes the staged rows inline instead)
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
// the batch window workspace, pruned-list bitmaps and the second stream, allocated on the first
// step that runs a resolver using them (ks_step.cpp)
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
    hipStream_t st = nullptr;
    std::vector<ks_engine*> engs;
    int64_t* d_ctr = nullptr;           // [cap][32]
    int64_t* h_ctr = nullptr;           // pinned
    ks::EngineArgs* d_args = nullptr;   // [cap]
    ks::EngineArgs* h_args = nullptr;   // pinned
    ks::BindSeg* d_seg = nullptr;       // [cap]
    ks::BindSeg* h_seg = nullptr;       // pinned
    int32_t* d_out = nullptr;           // packed binds: node, then status
    int32_t* h_out = nullptr;           // pinned mirror of d_out
    int64_t out_cap = 0;
    hipEvent_t ev[2] = {nullptr, nullptr};
    // the second half of the scenarios runs its batch rounds on its own stream: one half's
    // latency-bound resolvers then share the GPU with the other half's throughput-bound scans
    hipStream_t st2 = nullptr;
    hipEvent_t xev = nullptr;  // argument upload done (st -> st2)
    std::string errmsg;
};
