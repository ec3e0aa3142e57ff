// ks_rolesplit.hip — the role-split resolver (gfx950): resolve_kernel, one 16-wave workgroup per
// engine, one pod per barrier ("the other resolvers").
//
// The resolver that takes any engine.  The plain chain (ks_step.cpp batch_plain: expire_head -> scan
// -> merge -> resolve) launches it for the engines the chunk resolver refuses — scaled capacities
// >= 2^32 or totals + 1 >= 2^16 — and for engines created with KS_ENGINE_ONE_POD_RESOLVER, the A/B
// reference every other resolver is held against; ks_group_step launches it for scenarios past the
// register-table resolver's limits (ks_resolve.hip).  Its speed no longer decides a benchmark; its
// exactness does, because whatever the chunk resolver refuses lands here.
//
// The exactness argument is the scan's (ks_scan.hip): a node's key for pod i can differ from the
// batch snapshot only if a bind or an expiry of this batch touched it.  Touched nodes live in an LDS
// table and are re-evaluated exactly for every pod; the best untouched node is the first untouched
// entry of the pod's sorted top-L list — exact because any node outside the list scores below
// every list entry.  winner = max(those).  If all L entries of a full list are touched the batch
// commits early and the next batch rescans.
#include "ks_device.h"

namespace ks {

constexpr int kResolveThreads = 1024;    // 16 waves
constexpr int kOwnerWave0 = 3;           // waves 3..15 own the touched entries, except
constexpr int kWriterWave = 5;           // the bind's bookkeeping writer (off the critical path)
// Resolver size (the LDS footprint): any cluster, 256-pod batches, 1024 threads, ~150 KB of LDS (one
// workgroup per CU).  Small batches of small clusters (what-if scenarios) go to the register-table
// resolver instead (ks_resolve.hip).
constexpr int kTMax = 768;               // touched-node table entries
constexpr int kHashLog2 = 11;            // open-addressing node -> entry map slots (log2)
constexpr int kHash = 1 << kHashLog2;
constexpr int kMaxBatchR = 256;          // pods per launch
constexpr int kMaxExp = kTMax - kMaxBatchR;  // expiries pre-inserted per batch
constexpr int kFilterBits = 1 << 16;     // touched filter bits (the filter is exact — no hash confirmation — for
                                         // clusters of at most that many nodes)
static_assert(kWriterWave < kResolveThreads / kWave, "the writer wave exists");
static_assert(kTMax <= (kResolveThreads / kWave - kOwnerWave0 - 1) * kWave, "one touched entry per owner thread");
static_assert(kMaxExp <= kResolveThreads, "one thread per pre-inserted expiry");

// owner slot of a resolve wave, or -1
__device__ __forceinline__ int owner_slot(int wave) {
    if (wave < kOwnerWave0 || wave == kWriterWave) return -1;
    return wave - kOwnerWave0 - (wave > kWriterWave);
}

// ------------------------------------------------------------------------------------------
// resolve: one workgroup, sequential over the batch in FIFO order (one bind per tick).
//
// One barrier per pod.  Pod i's winner is a single LDS word ctl[i % 3].best: every contributor of
// pod i (list candidate, re-evaluated touched entries) folds its key in with an LDS atomic max
// during iteration i-1, so after the barrier every wave reads the decision (and the NotFound /
// InvalidArgument / exhausted-list stops) with one load.  Internal key (ikey):
//     (total + 1) << 34 | (2^24 - 1 - node) << 10 | entry          (entry 1023 = untouched)
// orders exactly like the packed key (node < 2^24, total + 1 < 2^30: ks_engine.cpp) and carries
// the winner's table entry.  Between two barriers the waves split the bind of pod i and the
// evaluation of pod i+1:
//   wave 0    table insert of an untouched winner; pod i+1's best untouched list node (chosen
//             from two prefetched candidates, see below) staged in LDS; pod i+2's list walk and
//             HBM prefetch
//   wave 1    CreatePod admission + bind on the winner's entry (and pod i+1's expiries that
//             land on it); outputs; pod i+1's exact key on that entry
//   wave 2    pod i+1's other expiries; pod i+1's exact keys on those entries
//   3..15     owner threads: thread r keeps touched entry r in registers (reloading the
//             mutable fields when an entry was modified the iteration before) and computes pod
//             i+1's exact key on it, unless wave 1 or 2 owns the entry this iteration
// Writers (waves 1, 2) touch disjoint entries and every reader of those skips them.
//
// Prefetch: pod i+2's list is walked in iteration i; its first two untouched entries' records
// are loaded into wave 0's registers (lane = slot * 10 + field).  In iteration i+1 exactly one
// node can join the table (pod i+1's winner), so pod i+2's first untouched entry is the first
// prefetched one unless that node just won, else the second.
//
// Pruning (exact): pod i+1's winner is >= its first untouched list entry >= its L-th list
// entry (lists are sorted; a full list with every entry touched stops the batch before the
// winner matters; wave 0 publishes a tighter bound, see prefetch_issue).  A touched entry whose
// float upper bound (prune_tmax) is below it is not evaluated, and exact keys below it are not
// folded into best.
// ------------------------------------------------------------------------------------------
// Per-pod control read by every wave right after the barrier: one 16/32-byte LDS load each,
// issued together (a chain of dependent reads here costs ~150 cycles per link).
struct alignas(16) Ctl {
    uint64_t best;   // pod's winner (ikey), folded during the previous iteration
    uint64_t lbk_next;  // lower bound of the NEXT pod's winner key (prefetch_issue), read with best
    int32_t kfull;   // every entry of a full list touched: the batch must stop
    int32_t ntab;    // table size when the pod is evaluated
    int32_t pad[2];
};
// Per-pod control read by every wave each iteration: one 16-byte LDS load (pod i's flags, run
// ticks and own expiry slot; pod i+1's expiry window)
struct alignas(16) PodCC {
    uint32_t w0;     // flags | (exp_slot + 1) << 2
    int32_t dur;     // ticks the pod runs if bound Ok
    int32_t ex_lo1;  // pod i+1's expiry window [ex_lo1, ex_hi1) (empty for the batch's last pod)
    int32_t ex_hi1;
};

struct ResolveShared {
    int64_t ts[8][kTMax];       // touched-node state: ac am ag ap rc rm rg nr
    uint64_t tu[2][kTMax];      // taint label
    int32_t tnode[kTMax];
    int32_t dirty[kTMax];       // iteration at which the owner must reload the mutable fields
    int32_t hkey[kHash];        // node id or -1
    int32_t hval[kHash];        // entry index
    uint32_t tfilt[kFilterBits / 32];
    PodRec pod[kMaxBatchR + 1];  // +1: pod i + 1 is read unconditionally
    float podf[kMaxBatchR][2];  // cpu / memory requests as float (prune_tmax)
    PodCC pcc[kMaxBatchR];
    uint64_t cand[kMaxBatchR][kL];
    int32_t ex_q[kMaxExp];
    int32_t ex_node[kMaxExp];
    int32_t ex_ok[kMaxExp];     // the expiring pod was bound Ok and has not expired yet
    int32_t ex_entry[kMaxExp];  // table entry of its node (set at the bind for in-batch pods)
    int64_t ex_req[kMaxExp][3];
    Ctl ctl[3];                 // pod i's decision state, slot i % 3
    int64_t stage[2][10];       // snapshot fields of the pod's best untouched list node
    int32_t n_t, committed, err_code, err_pod, nb, e_cnt;
};

constexpr int kEntUntouched = 1023;
static_assert(kTMax < kEntUntouched, "entry index fits 10 bits");

__device__ __forceinline__ uint64_t ikey(uint64_t key, int ent) {
    const uint32_t node = 0xFFFFFFFFu - (uint32_t)key;
    return ((key >> 32) << 34) | ((uint64_t)(0xFFFFFFu - node) << 10) | (uint64_t)(uint32_t)ent;
}
__device__ __forceinline__ int32_t ikey_node(uint64_t b) { return (int32_t)(0xFFFFFFu - (uint32_t)((b >> 10) & 0xFFFFFFu)); }
__device__ __forceinline__ int ikey_ent(uint64_t b) {
    const int e = (int)(b & 1023u);
    return e == kEntUntouched ? -1 : e;
}
__device__ __forceinline__ void fold_best(uint64_t* slot, uint64_t k) {
    atomicMax((unsigned long long*)slot, (unsigned long long)k);
}

__device__ __forceinline__ uint32_t hslot(int32_t node) {
    return ((uint32_t)node * 2654435761u) >> (32 - kHashLog2);
}

// entry index of `node` in the touched table, or -1
__device__ __forceinline__ int h_find(const ResolveShared& sh, int32_t node) {
    uint32_t s = hslot(node);
    for (int i = 0; i < kHash; ++i) {
        const int32_t k = sh.hkey[s];
        if (k == node) return sh.hval[s];
        if (k == -1) return -1;
        s = (s + 1) & (kHash - 1);
    }
    return -1;
}

// single-lane insert of a node known to be absent
__device__ __forceinline__ void h_insert(ResolveShared& sh, int32_t node, int32_t idx) {
    uint32_t s = hslot(node);
    while (sh.hkey[s] != -1) s = (s + 1) & (kHash - 1);
    sh.hkey[s] = node;
    sh.hval[s] = idx;
    const uint32_t f = (uint32_t)node & (kFilterBits - 1);
    sh.tfilt[f >> 5] |= 1u << (f & 31);
}

// touched? — one LDS read; the filter is exact (node & 0xFFFF is injective) when the cluster has
// at most kFilterBits nodes, otherwise a set bit is confirmed in the hash
__device__ __forceinline__ bool is_touched(const ResolveShared& sh, int32_t node, bool exact) {
    const uint32_t f = (uint32_t)node & (kFilterBits - 1);
    if (!((sh.tfilt[f >> 5] >> (f & 31)) & 1u)) return false;
    return exact || h_find(sh, node) >= 0;
}

// table insert of an in-loop winner: with an exact filter only the filter bit (the hash is
// consulted only by the batch-start pre-insert and by inexact filters)
__device__ __forceinline__ void t_insert(ResolveShared& sh, int32_t node, int32_t idx, bool exact) {
    if (exact) {
        const uint32_t f = (uint32_t)node & (kFilterBits - 1);
        atomicOr(&sh.tfilt[f >> 5], 1u << (f & 31));
    } else {
        h_insert(sh, node, idx);
    }
}

__device__ __forceinline__ NodeV t_node(const ResolveShared& sh, int e) {
    NodeV v;
    v.ac = sh.ts[0][e]; v.am = sh.ts[1][e]; v.ag = sh.ts[2][e]; v.ap = sh.ts[3][e];
    v.rc = sh.ts[4][e]; v.rm = sh.ts[5][e]; v.rg = sh.ts[6][e]; v.nr = sh.ts[7][e];
    v.taint = sh.tu[0][e]; v.label = sh.tu[1][e];
    return v;
}

__device__ __forceinline__ NodeV stage_node(const ResolveShared& sh, int b) {
    NodeV v;
    v.ac = sh.stage[b][0]; v.am = sh.stage[b][1]; v.ag = sh.stage[b][2]; v.ap = sh.stage[b][3];
    v.rc = sh.stage[b][4]; v.rm = sh.stage[b][5]; v.rg = sh.stage[b][6]; v.nr = sh.stage[b][7];
    v.taint = (uint64_t)sh.stage[b][8]; v.label = (uint64_t)sh.stage[b][9];
    return v;
}

// field f (0..9, NodeV order) of node i: the SoA is one allocation with a fixed field stride
__device__ __forceinline__ int64_t node_field(const NodeSoA& s, int f, int64_t i) {
    return gptr(s.ac)[(int64_t)f * (s.am - s.ac) + i];
}

__device__ __forceinline__ int32_t key_node(uint64_t key) { return (int32_t)(0xFFFFFFFFu - (uint32_t)key); }

// A pod record read from LDS as three 16-byte loads issued together, pinned in registers by an
// empty asm use (otherwise the compiler sinks each field's load into the config branch that
// uses it, turning one LDS round trip into several dependent ones).
__device__ __forceinline__ PodRec pod_regs(const PodRec* src) {
    const uint4* w = reinterpret_cast<const uint4*>(src);
    const uint4 w0 = w[0], w1 = w[1], w2 = w[2];
    asm volatile("" ::"v"(w0.x), "v"(w0.y), "v"(w0.z), "v"(w0.w), "v"(w1.x), "v"(w1.y), "v"(w1.z), "v"(w1.w),
                 "v"(w2.x), "v"(w2.y), "v"(w2.z), "v"(w2.w));
    PodRec p;
    static_assert(sizeof(PodRec) == 3 * sizeof(uint4), "PodRec is three 16-byte words");
    __builtin_memcpy(&p, &w0, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p) + 16, &w1, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p) + 32, &w2, 16);
    return p;
}

// two records, all six loads issued before the single pin
__device__ __forceinline__ void pod_regs2(const PodRec* s0, const PodRec* s1, PodRec& p0, PodRec& p1) {
    const uint4* a = reinterpret_cast<const uint4*>(s0);
    const uint4* b = reinterpret_cast<const uint4*>(s1);
    const uint4 a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
    asm volatile("" ::"v"(a0.x), "v"(a0.y), "v"(a0.z), "v"(a0.w), "v"(a1.x), "v"(a1.y), "v"(a1.z), "v"(a1.w),
                 "v"(a2.x), "v"(a2.y), "v"(a2.z), "v"(a2.w), "v"(b0.x), "v"(b0.y), "v"(b0.z), "v"(b0.w),
                 "v"(b1.x), "v"(b1.y), "v"(b1.z), "v"(b1.w), "v"(b2.x), "v"(b2.y), "v"(b2.z), "v"(b2.w));
    __builtin_memcpy(&p0, &a0, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p0) + 16, &a1, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p0) + 32, &a2, 16);
    __builtin_memcpy(&p1, &b0, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p1) + 16, &b1, 16);
    __builtin_memcpy(reinterpret_cast<char*>(&p1) + 32, &b2, 16);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

// Wave 0 prefetch state for one pod: its first two list entries whose node is untouched
// (key1, key2; 0 = none), whether the list holds L candidates (so "none" means exhausted, not
// "no candidates"), and their records: lanes 0..19 hold field (lane % 10) of entry lane / 10.
struct Prefetch {
    int64_t val;
    uint64_t key1, key2;
    bool full;
};

// Walk pod p's list against the table and issue the record loads.  Also publishes pod p's
// winner lower bound: the first untouched entry when pod p is decided is key1 or key2 (or none:
// then the batch stops at a full list, or the list is short and the bound is 0), so key2 — or
// key1 when the list is full and has no second — is <= it.
__device__ __forceinline__ void prefetch_issue(const EngineArgs& a, ResolveShared& sh, int p, int lane, bool exact,
                                               Prefetch& pf) {
    const uint64_t c = lane < kL ? sh.cand[p][lane] : 0ull;
    const bool ok = c != 0 && !is_touched(sh, key_node(c), exact);
    uint64_t m = __ballot(ok);
    pf.full = __popcll(__ballot(c != 0)) == kL;
    const int pa1 = m ? __ffsll((unsigned long long)m) - 1 : -1;
    m &= m - 1;
    const int pa2 = m ? __ffsll((unsigned long long)m) - 1 : -1;
    pf.key1 = pa1 >= 0 ? readlane64(c, pa1) : 0ull;
    pf.key2 = pa2 >= 0 ? readlane64(c, pa2) : 0ull;
    // into pod p-1's slot: read by every wave together with pod p-1's decision
    if (lane == 0) sh.ctl[(p + 2) % 3].lbk_next = pf.key2 ? pf.key2 : (pf.full ? pf.key1 : 0ull);
    const uint64_t ks = lane < 10 ? pf.key1 : pf.key2;
    if (lane < 20 && ks != 0) pf.val = node_field(a.s, lane % 10, key_node(ks));
}

// Wave 0: pod p's best untouched list node given that `winner` just joined the table (-1:
// none): stage its record, fold its key into ctl[bslot].best, set kfull.
__device__ __forceinline__ void prefetch_commit(ResolveShared& sh, int lane, const Prefetch& pf, int32_t winner,
                                                int stage_buf, int bslot) {
    const int slot = (pf.key1 != 0 && key_node(pf.key1) == winner) ? 1 : 0;
    const uint64_t key = slot ? pf.key2 : pf.key1;
    if (key != 0 && lane < 20 && lane / 10 == slot) sh.stage[stage_buf][lane % 10] = pf.val;
    if (lane == 0) {
        if (key != 0) fold_best(&sh.ctl[bslot].best, ikey(key, kEntUntouched));
        sh.ctl[bslot].kfull = key == 0 && pf.full;
    }
}

// The expiries due before pod j + 1 binds (window range [e0, e1)) that land on entry t — pod
// j's own included when it was bound Ok and runs one tick — subtracted from n.  Lane-parallel:
// one LDS round for the whole range; the (usually zero or one) hits are folded via a ballot.
// Marks them expired when `expired` is given (the writer wave).
__device__ __forceinline__ void expire_on(const ResolveShared& sh, int e0, int e1, int t, int64_t j, bool ok,
                                          int lane, NodeV& n, uint8_t* expired) {
    for (int x0 = e0; x0 < e1; x0 += kWave) {
        const int x = x0 + lane;
        bool hit = false;
        int32_t q = 0;
        int64_t r0 = 0, r1 = 0, r2 = 0;
        if (x < e1) {
            q = sh.ex_q[x];
            hit = q == j ? ok : (sh.ex_entry[x] == t && sh.ex_ok[x] != 0);
            r0 = sh.ex_req[x][0]; r1 = sh.ex_req[x][1]; r2 = sh.ex_req[x][2];
        }
        if (hit && expired) gptr(expired)[q] = 1;
        uint64_t m = __ballot(hit);
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            n.rc -= (int64_t)readlane64((uint64_t)r0, l);
            n.rm -= (int64_t)readlane64((uint64_t)r1, l);
            n.rg -= (int64_t)readlane64((uint64_t)r2, l);
            n.nr -= 1;
        }
    }
}

template <int kMode>
__global__ __launch_bounds__(kResolveThreads) void resolve_kernel(const EngineArgs* __restrict__ A) {
    __shared__ ResolveShared sh;
    const EngineArgs a = A[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    const int64_t start = a.ctr[kCtrStart], end = a.ctr[kCtrEnd];
    if (a.ctr[kCtrErr] != 0) return;
    const bool exact = a.c.n_nodes <= kFilterBits;  // touched filter needs no hash confirmation
    int nb = (int)min<int64_t>(min<int64_t>(a.B, kMaxBatchR), end - start);
    if (nb <= 0) return;

    // window: expiries of pods start+1 .. start+nb-1 (pod start's were applied by expire_head);
    // shrink the batch so that they fit the pre-insert budget
    // largest nb' <= nb whose window fits: exp_off is non-decreasing, so the count of fitting
    // prefixes is nb' (one HBM round trip for all candidates instead of a serial bisection)
    const int64_t e_base = a.exp_off[start + 1];
    const int64_t off_mid = tid < nb ? a.exp_off[start + tid + 1] : 0;
    const bool fits_win = tid < nb && off_mid - e_base <= kMaxExp;
    if (tid == 0) {
        sh.n_t = 0; sh.err_code = 0; sh.err_pod = -1;
        for (int b = 0; b < 3; ++b) sh.ctl[b] = Ctl{0, 0, 0, 0, {0, 0}};
    }
    for (int h = tid; h < kHash; h += kResolveThreads) sh.hkey[h] = -1;
    for (int w = tid; w < kFilterBits / 32; w += kResolveThreads) sh.tfilt[w] = 0;
    nb = __syncthreads_count(fits_win);
    if (tid == nb - 1) { sh.nb = nb; sh.committed = nb; sh.e_cnt = nb > 1 ? (int32_t)(off_mid - e_base) : 0; }
    __syncthreads();
    const int64_t e_cnt = sh.e_cnt;

    for (int i = tid; i < nb; i += kResolveThreads) {
        sh.pod[i] = a.pods[start + i];
        sh.podf[i][0] = (float)a.pods[start + i].req[0];
        sh.podf[i][1] = (float)a.pods[start + i].req[1];
        const int64_t pos = a.exp_pos[start + i];
        const int32_t exp_slot = (pos >= e_base && pos - e_base < e_cnt) ? (int32_t)(pos - e_base) : -1;
        PodCC pc;
        pc.w0 = a.pods[start + i].flags | (uint32_t)(exp_slot + 1) << 2;
        pc.dur = a.dur[start + i];
        // pod i+1's window: the expiries due before it binds (pod start's were applied by expire_head)
        const bool nx = i + 1 < nb;
        pc.ex_lo1 = !nx || i + 1 <= 1 ? 0 : (int32_t)(a.exp_off[start + i + 1] - e_base);
        pc.ex_hi1 = !nx ? 0 : (int32_t)(a.exp_off[start + i + 2] - e_base);
        sh.pcc[i] = pc;
    }
    for (int i = tid; i < nb * kL; i += kResolveThreads) sh.cand[i / kL][i % kL] = a.cand[i];
    for (int e = tid; e < e_cnt; e += kResolveThreads) {
        const int32_t q = a.exp_pod[e_base + e];
        const PodRec& pq = a.pods[q];
        sh.ex_q[e] = q;
        sh.ex_entry[e] = -1;
        sh.ex_req[e][0] = pq.req[0]; sh.ex_req[e][1] = pq.req[1]; sh.ex_req[e][2] = pq.req[2];
        if (q < start) {
            sh.ex_node[e] = a.b_node[q];
            sh.ex_ok[e] = (a.b_status[q] == 0) && !a.expired[q];
        } else {
            sh.ex_node[e] = -1;
            sh.ex_ok[e] = 0;  // set when the pod binds
        }
    }
    __syncthreads();
    // pre-insert every node an expiry of this batch lands on (q bound before the batch): the
    // per-pod expiry step then never waits on HBM.  One thread per expiry (e_cnt <= kMaxExp <
    // kResolveThreads): claim the node's hash slot with a CAS (duplicates find it), number the
    // claimed slots, then read the entry back.  Entry numbering order is immaterial: an entry
    // index only names a node, it never takes part in a comparison between distinct nodes.
    const bool pre_want = tid < e_cnt && sh.ex_ok[tid];
    int pre_slot = -1;
    bool pre_claim = false;
    if (pre_want) {
        const int32_t nd = sh.ex_node[tid];
        uint32_t hs = hslot(nd);
        for (;;) {  // the table holds <= kMaxExp < kHash nodes: terminates
            const int32_t prev = atomicCAS(&sh.hkey[hs], -1, nd);
            if (prev == -1 || prev == nd) { pre_slot = (int)hs; pre_claim = prev == -1; break; }
            hs = (hs + 1) & (kHash - 1);
        }
    }
    __syncthreads();
    if (pre_claim) {
        const int32_t nd = sh.ex_node[tid];
        const int idx = atomicAdd(&sh.n_t, 1);
        sh.hval[pre_slot] = idx;
        sh.tnode[idx] = nd;
        const uint32_t f = (uint32_t)nd & (kFilterBits - 1);
        atomicOr(&sh.tfilt[f >> 5], 1u << (f & 31));
    }
    __syncthreads();
    if (pre_want) sh.ex_entry[tid] = sh.hval[pre_slot];
    __syncthreads();
    for (int e = tid; e < kTMax; e += kResolveThreads) sh.dirty[e] = -1;
    for (int e = tid; e < sh.n_t; e += kResolveThreads) {
        const NodeV v = load_node(a.s, sh.tnode[e]);
        sh.ts[0][e] = v.ac; sh.ts[1][e] = v.am; sh.ts[2][e] = v.ag; sh.ts[3][e] = v.ap;
        sh.ts[4][e] = v.rc; sh.ts[5][e] = v.rm; sh.ts[6][e] = v.rg; sh.ts[7][e] = v.nr;
        sh.tu[0][e] = v.taint; sh.tu[1][e] = v.label;
    }
    __syncthreads();

    // owner registers (waves 3..15): entry r = tid - 192
    const int oslot = owner_slot(wave);
    const int r = oslot >= 0 ? oslot * kWave + lane : kTMax;
    bool loaded = false;
    NodeV own{};
    int32_t own_node = 0;
    PruneF own_pf{};      // prune_tmax state of the entry
    Prefetch pf{};        // wave 0

    // ---- prologue: pod 0's contributions into ctl[0].best; pod 1's prefetch
    if (wave == 0) {
        Prefetch p0;
        prefetch_issue(a, sh, 0, lane, exact, p0);
        prefetch_commit(sh, lane, p0, -1, 0, 0);
        // Pod 0 never stops on an exhausted list: its own expiries were applied before the scan
        // and nothing else has changed yet, so every touched entry still holds its snapshot key
        // and is evaluated exactly below — a node outside the list cannot beat them.  (Stopping
        // here would commit nothing, and the next launch would rescan the same state forever.)
        if (lane == 0) { sh.ctl[0].ntab = sh.n_t; sh.ctl[0].kfull = 0; }
        if (nb > 1) prefetch_issue(a, sh, 1, lane, exact, pf);
    } else if (oslot >= 0 && r < sh.n_t) {
        own = t_node(sh, r);
        own_node = sh.tnode[r];
        own_pf = prune_prep_t<kMode>(a.c, own);
        loaded = true;
        const uint64_t k = make_key(eval_t<kMode>(a.c, sh.pod[0], own), (uint32_t)own_node);
        if (k != 0 && k >= sh.cand[0][kL - 1]) fold_best(&sh.ctl[0].best, ikey(k, r));
    }
    __syncthreads();
    // The table grows by at most one entry per pod, so owner waves whose first entry lies past
    // n_t + nb can never own one: they end here.  s_barrier waits only for the surviving waves of
    // the workgroup (CDNA ISA, S_BARRIER), and their threads have no share in the write-back
    // (tid >= 64 * (oslot + 3) > n_t + nb >= the final table size).
    if (oslot >= 0 && oslot * kWave >= sh.n_t + nb) return;

    for (int i = 0; i < nb; ++i) {
        const int64_t j = start + i;
        const int cur = i & 1, nxt = cur ^ 1;
        const int b_cur = i % 3, b_nxt = (i + 1) % 3;
        // ---- every wave: pod i's winner and the stop decision (identical in all waves)
        const Ctl cc = sh.ctl[b_cur];
        const PodCC pci = sh.pcc[i];
        const uint64_t lbk = cc.lbk_next;
        const uint64_t bw = cc.best;
        int stop = 0;
        if (cc.kfull) stop = 1;                                       // list exhausted: rescan
        else if (bw == 0) stop = 2;                                   // NotFound
        else if (pci.w0 & (kFlagBadKey | kFlagBadSpec)) stop = 3;     // InvalidArgument
        if (stop) {
            if (tid == 0) {
                sh.committed = i;
                if (stop > 1) { sh.err_code = stop == 2 ? kErrNotFound : kErrEinval; sh.err_pod = (int32_t)j; }
            }
            break;
        }
        const int went = ikey_ent(bw);
        const int32_t nd = ikey_node(bw);
        const int nt = cc.ntab;
        const int t = went >= 0 ? went : nt;  // an untouched winner becomes entry nt
        const bool has_next = i + 1 < nb;
        const int e0 = pci.ex_lo1, e1 = pci.ex_hi1;

        if (oslot >= 0) {
            if (has_next && oslot * kWave < nt) {
                // one round of independent LDS reads, then the (rare) reload
                const int32_t dr = sh.dirty[r < kTMax ? r : 0];
                const float qfc = sh.podf[i + 1][0], qfm = sh.podf[i + 1][1];
                const PodRec pn = pod_regs(&sh.pod[i + 1]);
                if (r < nt) {
                    if (!loaded) {
                        own = t_node(sh, r);
                        own_node = sh.tnode[r];
                        own_pf = prune_prep_t<kMode>(a.c, own);
                        loaded = true;
                    } else if (dr == i) {
                        own.rc = sh.ts[4][r]; own.rm = sh.ts[5][r]; own.rg = sh.ts[6][r]; own.nr = sh.ts[7][r];
                        own_pf = prune_prep_t<kMode>(a.c, own);
                    }
                }
                bool want = r < nt && own_pf.live && r != went;
                if (lbk != 0 && want) {
                    const uint32_t tm = prune_tmax(a.c, own_pf, qfc, qfm);
                    want = make_key(tm + 1u, (uint32_t)own_node) >= lbk;
                }
                if (__ballot(want)) {
                    for (int x = e0; x < e1; ++x)  // wave 2 owns the entries pod i+1's expiries land on
                        want &= !(sh.ex_entry[x] == r && sh.ex_q[x] != j);
                    if (want) {
                        const uint64_t k = make_key(eval_t<kMode>(a.c, pn, own), (uint32_t)own_node);
                        if (k != 0 && k >= lbk) fold_best(&sh.ctl[b_nxt].best, ikey(k, r));
                    }
                }
            }
        } else if (wave == 0) {
            if (lane == 0) {
                if (went < 0) { sh.tnode[t] = nd; t_insert(sh, nd, t, exact); }
                sh.ctl[b_nxt].ntab = went < 0 ? nt + 1 : nt;
                sh.ctl[(i + 2) % 3].best = 0;  // read in iteration i-1, folded into in iteration i+1
            }
            if (has_next) prefetch_commit(sh, lane, pf, went < 0 ? nd : -1, nxt, b_nxt);
            if (i + 2 < nb) prefetch_issue(a, sh, i + 2, lane, exact, pf);
        } else if (wave == 1 || wave == kWriterWave) {
            // the bind of pod i on entry t: wave 1 computes pod i+1's key on the new state (the
            // critical path), the writer wave stores the state and the outputs
            PodRec p, pnext;  // pod i + 1 <= nb: a readable slot
            pod_regs2(&sh.pod[i], &sh.pod[i + 1], p, pnext);
            NodeV n = went >= 0 ? t_node(sh, t) : stage_node(sh, cur);
            const bool ok = fits(p, n);  // CreatePod admission (kubesim/node/node.go:44-47)
            if (ok && pci.dur > 0) { n.rc += p.req[0]; n.rm += p.req[1]; n.rg += p.req[2]; n.nr += 1; }
            expire_on(sh, e0, e1, t, j, ok, lane, n, wave == 1 ? nullptr : a.expired);
            if (wave == 1) {
                if (lane == 0 && has_next) {
                    const uint64_t k = make_key(eval_t<kMode>(a.c, pnext, n), (uint32_t)nd);
                    if (k != 0) fold_best(&sh.ctl[b_nxt].best, ikey(k, t));
                }
            } else if (lane == 0) {
                if (went < 0) {
                    sh.ts[0][t] = n.ac; sh.ts[1][t] = n.am; sh.ts[2][t] = n.ag; sh.ts[3][t] = n.ap;
                    sh.tu[0][t] = n.taint; sh.tu[1][t] = n.label;
                }
                sh.ts[4][t] = n.rc; sh.ts[5][t] = n.rm; sh.ts[6][t] = n.rg; sh.ts[7][t] = n.nr;
                sh.dirty[t] = i + 1;
                const int slot = (int)(pci.w0 >> 2) - 1;
                if (slot >= 0) { sh.ex_entry[slot] = t; sh.ex_ok[slot] = ok ? 1 : 0; }
                gptr(a.b_node)[j] = nd;
                gptr(a.b_status)[j] = ok ? 0 : 1;
            }
        } else if (wave == 2) {
            if (has_next && e1 > e0) {
                // pod i+1's other expiries, lane-parallel: LDS atomics apply them (several may hit
                // one entry), then each lane evaluates its expiry's entry on the final state
                // (LDS operations of one wave complete in order)
                const PodRec pn = pod_regs(&sh.pod[i + 1]);
                for (int x0 = e0; x0 < e1; x0 += kWave) {  // apply every expiry first ...
                    const int x = x0 + lane;
                    if (x < e1) {
                        const int32_t q = sh.ex_q[x];
                        const int tq = sh.ex_entry[x];
                        const int okx = sh.ex_ok[x];
                        const int64_t r0 = sh.ex_req[x][0], r1 = sh.ex_req[x][1], r2 = sh.ex_req[x][2];
                        if (q != j && tq >= 0 && tq != t && okx) {
                            atomicAdd((unsigned long long*)&sh.ts[4][tq], (unsigned long long)-r0);
                            atomicAdd((unsigned long long*)&sh.ts[5][tq], (unsigned long long)-r1);
                            atomicAdd((unsigned long long*)&sh.ts[6][tq], (unsigned long long)-r2);
                            atomicAdd((unsigned long long*)&sh.ts[7][tq], (unsigned long long)-1ll);
                            sh.dirty[tq] = i + 1;
                            gptr(a.expired)[q] = 1;
                        }
                    }
                }
                for (int x0 = e0; x0 < e1; x0 += kWave) {  // ... then evaluate their entries
                    const int x = x0 + lane;
                    if (x < e1) {
                        const int tq = sh.ex_entry[x];
                        if (sh.ex_q[x] != j && tq >= 0 && tq != t) {
                            const uint64_t k = make_key(eval_t<kMode>(a.c, pn, t_node(sh, tq)), (uint32_t)sh.tnode[tq]);
                            if (k != 0) fold_best(&sh.ctl[b_nxt].best, ikey(k, tq));
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    __syncthreads();

    // ---- write back the mutable fields of every touched node
    const int n_final = sh.ctl[sh.committed % 3].ntab;
    for (int e = tid; e < n_final; e += kResolveThreads) {
        const int64_t ndx = sh.tnode[e];
        a.s.rc[ndx] = sh.ts[4][e];
        a.s.rm[ndx] = sh.ts[5][e];
        a.s.rg[ndx] = sh.ts[6][e];
        a.s.nr[ndx] = sh.ts[7][e];
    }
    if (tid == 0) {
        a.ctr[kCtrStart] = start + sh.committed;
        if (sh.committed < a.B && sh.err_code == 0 && start + sh.committed < end) a.ctr[kCtrEarly] += 1;
        if (sh.err_code) { a.ctr[kCtrErr] = sh.err_code; a.ctr[kCtrErrPod] = sh.err_pod; }
    }
}

int max_batch_pods() { return kMaxBatchR; }

hipError_t launch_resolve(const EngineArgs* d, int S, int mode, hipStream_t st) {
    with_eval_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(resolve_kernel<decltype(m)::value>, dim3(S), dim3(kResolveThreads), 0, st, d);
    });
    return hipGetLastError();
}
}  // namespace ks
