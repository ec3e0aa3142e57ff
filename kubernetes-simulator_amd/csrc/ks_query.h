// ks_query.h — the device contract of the code that answers about a run after the fact: the
// past-tick state queries, headroom, and the placement, drain, removal, scale-up and consolidation
// previews (records, exactness arguments, host-testable helpers, launchers).  No hot-path
// translation unit includes it: the step kernels and their host code see ks_device.h alone.
#pragma once
#include <vector>

#include "ks_device.h"

namespace ks {

// past-tick state queries (ks_query.hip), over the same candidate blocks
struct QScale { int64_t f[3]; };  // milli-units per device unit of cpu / memory / gpu (1: device units)
constexpr int kSeriesCols = 7;
struct SeriesInit { int64_t v[kSeriesCols]; };  // the columns' values before the window's first tick
// word k of node nd at out[nd * node_stride + k * col_stride] (zeroed): Σ req[0..2] * sc.f, running pods
hipError_t launch_requested(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                            const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                            const PodRec* pods, const QScale& sc, int64_t node_stride, int64_t col_stride,
                            unsigned long long* out, hipStream_t st);
// diff: [kSeriesCols][t_hi - t_lo + 1] zeroed; out: [t_hi - t_lo][kSeriesCols]; pods [q_lo, q_hi) left the
// queue at ticks inside (t_lo, t_hi); arr[n_arr]: the arrival ticks inside (t_lo, t_hi)
hipError_t launch_series(const int32_t* blocks, int64_t nblocks, int64_t q_lo, int64_t q_hi, int64_t t_lo,
                         int64_t t_hi, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                         const PodRec* pods, const QScale& sc, const int64_t* arr, int64_t n_arr,
                         const SeriesInit& init, unsigned long long* diff, unsigned long long* out, hipStream_t st);
// cnt[n_nodes] zeroed, off[n_nodes + 1], cur[n_nodes], list[list_cap >= nblocks * usage_block_pods()];
// out: [n_nodes][4]
hipError_t launch_node_peaks(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t_lo, int32_t n_nodes,
                             const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                             const PodRec* pods, const QScale& sc, int32_t* cnt, int32_t* off, int32_t* cur,
                             int32_t* list, int32_t list_cap, long long* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Headroom (ks_headroom_at / ks_headroom_series): how many copies of a pod shape Node.CreatePod
// (kubesim/node/node.go:44-47) would admit one after another on a node, nothing finishing in
// between.  Per masked key the bound is 0 on a node that lacks the key (even for a request of 0,
// kubesim/node/resource.go:54-55), none for a request of 0, else floor((A - r) / q); the pods
// bound is max(ap - nr, 0) (runningPodsNum >= cap.Pods(), node.go:47).  Every bound is clamped to
// kHeadMax, the count is their minimum and the limiting key the first bound, in the order cpu,
// memory, gpu, pods, that attains it (so at the clamp: the first bound that reaches the clamp).
//
// The node is in device units (alloc -1 absent; rc rm rg nr the rebuilt state), sc the milli-units
// per device unit, the shape's requests in milli-units and not necessarily multiples of sc: the
// numerator (A - r) * sc is the free amount in milli-units, < 2^59 like every admitted quantity.
// ---------------------------------------------------------------------------------------------
constexpr int64_t kHeadMax = 2147483647;        // KS_HEADROOM_NODE_MAX
constexpr uint64_t kHeadFloat = 1ull << 22;     // numerators below it: float estimate
constexpr uint64_t kHeadDouble = 1ull << 53;    // numerators below it: double estimate
constexpr uint64_t kHeadClampQ = 1ull << 28;    // requests at or above it never reach the clamp (q * kHeadMax >= 2^59)
constexpr int64_t kHeadReqMax = 1LL << 59;      // a masked request is 0 <= q < 2^59

// min(floor(num / q), kHeadMax) for q >= 1, num < 2^59.  gfx950 has no 64-bit divide: an estimate
// from the float (num < 2^22: error < 1) or double (num < 2^53, one Newton step on the reciprocal)
// pipe, one exact step either way, and the result is proved (t <= num < t + q) before it is
// returned; anything else takes the compiler's exact 64-bit division.
__host__ __device__ __forceinline__ int64_t head_div(uint64_t num, uint64_t q) {
    if (num < q) return 0;
    if (q < kHeadClampQ && num >= q * (uint64_t)kHeadMax) return kHeadMax;  // early clamp: the quotient is < 2^31 below
    uint64_t c;
    if (num < kHeadFloat) {
        c = (uint64_t)(uint32_t)((float)(uint32_t)num * rcp_est((float)(uint32_t)q));
    } else if (num < kHeadDouble) {
        const double d = (double)q;
        double y = rcp_est(d);
        y = __builtin_fma(__builtin_fma(-d, y, 1.0), y, y);
        const double est = (double)num * y;
        c = est > 0.0 ? (uint64_t)est : 0ull;
    } else {
        return (int64_t)(num / q);
    }
    // a sane estimate has c q ~ num < 2^53; one whose product could leave 64 bits is not used
    if (bitlen(c) + bitlen(q) > 62) return (int64_t)(num / q);
    uint64_t t = c * q;
    if (t > num) { c -= 1; t -= q; }
    else if (num - t >= q) { c += 1; t += q; }
    if (t <= num && num - t < q) return (int64_t)c;
    return (int64_t)(num / q);
}

// one key's bound: -1 = none (the key is not masked, or its request is 0 on a node that has it)
__host__ __device__ __forceinline__ int64_t head_key_bound(bool masked, int64_t A, int64_t r, int64_t sc, int64_t q) {
    if (!masked) return -1;
    if (A < 0) return 0;
    if (q == 0) return -1;
    return A > r ? head_div((uint64_t)(A - r) * (uint64_t)sc, (uint64_t)q) : 0;
}

// The count (0..kHeadMax) and, in *key, the limiting key (0 cpu, 1 memory, 2 gpu, 3 pods).  Taints
// and selectors are the caller's (head_eligible): an ineligible node has count 0 and no key.
__host__ __device__ __forceinline__ int32_t headroom_count(const NodeV& n, const QScale& sc, const PodRec& shape,
                                                           int32_t* key) {
    const int64_t free_pods = n.ap - n.nr;
    int64_t c = free_pods > 0 ? (free_pods < kHeadMax ? free_pods : kHeadMax) : 0;
    int32_t lim = 3;
    // gpu, memory, cpu: a tie goes to the key that comes first
    const int64_t bg = head_key_bound(shape.keymask & 4, n.ag, n.rg, sc.f[2], shape.req[2]);
    if (bg >= 0 && bg <= c) { c = bg; lim = 2; }
    const int64_t bm = head_key_bound(shape.keymask & 2, n.am, n.rm, sc.f[1], shape.req[1]);
    if (bm >= 0 && bm <= c) { c = bm; lim = 1; }
    const int64_t bc = head_key_bound(shape.keymask & 1, n.ac, n.rc, sc.f[0], shape.req[0]);
    if (bc >= 0 && bc <= c) { c = bc; lim = 0; }
    *key = lim;
    return (int32_t)c;
}

// eligibility of a node for a shape: the taint / selector predicates of the fused evaluator
// (eval_total1), applied only when the engine's filters gate the candidates
__host__ __device__ __forceinline__ bool head_eligible(int32_t filter_feeds, uint32_t filters, const NodeV& n,
                                                       const PodRec& shape) {
    if (!filter_feeds) return true;
    bool ok = true;
    if (filters & kFilterTaint) ok &= (n.taint & ~shape.tol) == 0;
    if (filters & kFilterSelector) ok &= (n.label & shape.sel) == shape.sel;
    return ok;
}

constexpr int kHeadCols = 9;        // KS_HEADROOM_COLS
constexpr int kHeadMaxShapes = 64;  // KS_HEADROOM_MAX_SHAPES (= one wave: the series gives a lane to each shape)
// state: rc rm rg nr at t in device units, [4][n_pad] (launch_requested with unit scale, strides (1, n_pad));
// shapes[k]: requests in milli-units; part: [ceil(n / 256)][k][3] scratch; out: [k][kHeadCols];
// per_node: [k][n_nodes] or null
hipError_t launch_headroom(const NodeSoA& s, const int64_t* state, int64_t n_pad, int32_t n_nodes, int32_t filter_feeds,
                           uint32_t filters, const QScale& sc, const PodRec* shapes, int32_t k,
                           unsigned long long* part, long long* out, int32_t* per_node, hipStream_t st);
// cnt / off / cur / list: launch_node_peaks' counting sort scratch; diff: [2 k][t_hi - t_lo + 1] zeroed;
// out: [t_hi - t_lo][k][2]
hipError_t launch_headroom_series(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t_lo, int64_t t_hi,
                                  const NodeSoA& s, int32_t n_nodes, int32_t filter_feeds, uint32_t filters,
                                  const QScale& sc, const PodRec* shapes, int32_t k, const int32_t* b_node,
                                  const int32_t* b_status, const int64_t* t0, const int32_t* dur, const PodRec* pods,
                                  int32_t* cnt, int32_t* off, int32_t* cur, int32_t* list, int32_t list_cap,
                                  unsigned long long* diff, unsigned long long* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Placement preview (ks_place_at, ks_place.hip): scheduleOne's Filter -> Score -> argmax ->
// CreatePod (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60) for k preview pods one after
// another on a private copy of the state at tick t.  A call runs in one unit throughout, sc
// milli-units per device unit of each key: the node's alloc is alloc * sc (an absent key stays -1),
// the state is rebuilt times sc, the requests are held in that unit, the pods capacity and the
// running count are plain counts.  sc is the engine's scale — the call runs in milli-units, any
// request is representable — unless every request is a whole multiple of the engine's unit: then
// sc = 1 and the call runs in device units (place_whole_units, below).  Either way every quantity
// is < 2^59, so the wide evaluator eval_total1 is exact (its BalancedAllocation goes to 128 bits
// when Ac * Am needs it), and every fit / score result is unit-free: both routes place alike.
//
// Exactness of a round.  Keys are make_key(total + 1, node); keys of different nodes differ.  A round
// starts from a committed state with an empty changed set and, per distinct shape, the exact global
// top-L keys of that state, descending (the snapshot list; fewer than L non-zero entries: the list
// is complete, every other node's key is 0).  A node joins the changed set when a preview pod is
// placed on it; its list entries (in every shape's list) are flagged (one bit each) once the pod is
// decided.  For pod i of shape s:
//   S = the first unflagged entry of list s; D = the largest exact key of shape s over the changed
//   nodes on their current state (0: none is a candidate).
//   - S exists: every unchanged node still has its snapshot key; those above S in the list are all
//     changed, those below it or outside the list are smaller.  The argmax is max(S, D).
//   - no S, list complete: every unchanged node has key 0.  The argmax is D, or there is none.
//   - no S, all L entries changed, D > the list's last key: every unchanged node is outside the
//     list, so below its last key.  The argmax is D.
//   - otherwise an unchanged node outside the list may win: the round ends before pod i, the
//     changed nodes' states are committed and the next round scans again.
// The changed set grows by at most one node per pod, so a pod that finds a full list entirely
// flagged has at least L pods before it in its round: a round decides at least min(L, pods left)
// pods, and the first pod of a round is always decided (nothing is flagged yet).
// ---------------------------------------------------------------------------------------------
#ifndef KS_PLACE_L
#define KS_PLACE_L 32  // (A/B: make variant DEFS=-DKS_PLACE_L=16; 8, 16, 32 measured: DESIGN.md §3.4)
#endif
constexpr int kPlaceL = KS_PLACE_L;
static_assert(kPlaceL == 8 || kPlaceL == 16 || kPlaceL == 32, "snapshot list length");
constexpr int kPlaceMaxPods = 1024;  // KS_PLACE_MAX_PODS (= the changed set's capacity)
constexpr int kPlaceMaxShapes = 64;  // KS_PLACE_MAX_SHAPES
enum : int32_t { kPlaceOk = 0, kPlaceOverCapacity = 1, kPlaceNotFound = -1 };
enum : int { kPlaceWin = 0, kPlaceNone = 1, kPlaceStop = 2 };

struct Placement {  // = ks_placement
    int32_t node, status;
    int64_t score, candidates;
};
static_assert(sizeof(Placement) == 24, "ks_placement layout");

// a node's constants in milli-units (in place)
__host__ __device__ __forceinline__ void place_scale_alloc(NodeV& v, const QScale& sc) {
    v.ac = v.ac < 0 ? -1 : v.ac * sc.f[0];
    v.am = v.am < 0 ? -1 : v.am * sc.f[1];
    v.ag = v.ag < 0 ? -1 : v.ag * sc.f[2];
}

// node nd in the call's units (sc per device unit): constants from the cluster, state from the scratch
__device__ __forceinline__ NodeV place_load(const NodeSoA& s, const int64_t* state, int64_t n_pad, const QScale& sc,
                                            int64_t nd) {
    NodeV v;
    v.ac = s.ac[nd]; v.am = s.am[nd]; v.ag = s.ag[nd]; v.ap = s.ap[nd];
    v.taint = s.taint[nd]; v.label = s.label[nd];
    place_scale_alloc(v, sc);
    v.rc = state[nd]; v.rm = state[n_pad + nd]; v.rg = state[2 * n_pad + nd]; v.nr = state[3 * n_pad + nd];
    return v;
}

// Whether every masked request of the shapes is a whole multiple of the engine's unit sc.  Then the
// call runs in device units instead (scale 1, requests divided by sc, `after` multiplied back):
// every fit / LeastRequested / BalancedAllocation result is unit-free, so the placements are the
// same, and the smaller numbers keep BalancedAllocation's products in 64 bits.
__host__ __device__ __forceinline__ bool place_whole_units(const PodRec* shapes, int n_shapes, const QScale& sc) {
    bool whole = true;
    for (int j = 0; j < n_shapes; ++j)
        for (int c = 0; c < 3; ++c)
            if ((shapes[j].keymask >> c & 1) && shapes[j].req[c] % sc.f[c] != 0) whole = false;
    return whole;
}

__host__ __device__ __forceinline__ uint32_t place_key_node(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

__host__ __device__ __forceinline__ uint64_t place_key(const Cfg& c, const PodRec& p, const NodeV& n, uint32_t node) {
    return make_key(eval_total1(c, p, n), node);
}

// entries of a snapshot list (sorted descending, 0-padded)
template <int L = kPlaceL>
__host__ __device__ __forceinline__ int place_list_len(const uint64_t* list) {
    int len = 0;
    for (int e = 0; e < L; ++e) len += list[e] != 0;
    return len;
}

// index of the first of a snapshot list's `len` entries whose bit in `flagged` is clear, L if none
template <int L = kPlaceL>
__host__ __device__ __forceinline__ int place_first_unchanged(int len, uint32_t flagged) {
    static_assert(L <= 32, "one flag word per list");
    const uint32_t open = ~flagged & (len >= 32 ? 0xFFFFFFFFu : (1u << len) - 1u);
    return open ? __builtin_ctz(open) : L;
}

// The decision of one pod (above).  S: its list's first unflagged key or 0; last: the list's L-th
// key (0: the list is complete); D: the best key over the changed nodes.  kPlaceWin: *win is the
// argmax key; kPlaceNone: no node has an entry in the score map; kPlaceStop: the round ends here.
__host__ __device__ __forceinline__ int place_decide(uint64_t S, uint64_t last, uint64_t D, uint64_t* win) {
    *win = 0;
    if (S) {
        *win = S > D ? S : D;
        return kPlaceWin;
    }
    if (!last || D > last) {
        *win = D;
        return D ? kPlaceWin : kPlaceNone;
    }
    return kPlaceStop;
}

// CreatePod on the chosen node (kubesim/node/node.go:44-58): the admission test, and on Ok the
// pod's masked requests and one running pod join the node's state.
__host__ __device__ __forceinline__ int32_t place_bind(const PodRec& p, NodeV& n) {
    if (!fits(p, n)) return kPlaceOverCapacity;
    if (p.keymask & 1) n.rc += p.req[0];
    if (p.keymask & 2) n.rm += p.req[1];
    if (p.keymask & 4) n.rg += p.req[2];
    n.nr += 1;
    return kPlaceOk;
}

// whether the node has an entry in the pod's score map: eval_total1(c, p, n) != 0 without the scores
__host__ __device__ __forceinline__ bool place_is_cand(const Cfg& c, const PodRec& p, const NodeV& n) {
    if (!c.has_scorers) return false;
    if (!c.filter_feeds) return true;
    bool ok = true;
    if (c.filters & kFilterFit) ok &= fits(p, n);
    if (c.filters & kFilterTaint) ok &= (n.taint & ~p.tol) == 0;
    if (c.filters & kFilterSelector) ok &= (n.label & p.sel) == p.sel;
    return ok;
}

// what a bind changes in shape j's candidate count: cand(after) - cand(before) on the bound node
__host__ __device__ __forceinline__ int32_t place_cand_delta(const Cfg& c, const PodRec& shape, const NodeV& before,
                                                             const NodeV& after) {
    return (int32_t)place_is_cand(c, shape, after) - (int32_t)place_is_cand(c, shape, before);
}

struct PlaceCfg {
    Cfg c;
    QScale sc;
    int32_t n_nodes, k, n_shapes, nblk;
};
// Scratch of one call (device): state [4][n_pad] rc rm rg nr at t in the units of PlaceCfg::sc
// (launch_requested with that scale, strides (1, n_pad)): milli-units per state unit — the engine's
// scale when the call runs in milli-units, 1 when it runs in device units (place_whole_units);
// shapes [n_shapes]; shape_of [k]; lists [64][nblk][kPlaceL], cnt [64][nblk] (nblk = ceil(n / 256));
// top [64][kPlaceL], ccount [64]; out [k] (read once, after the last round); rb [4], the 16 bytes the
// host reads after every round: the first undecided pod, 1 if the round decided none, the changed
// nodes it committed, 0.
struct PlaceBufs {
    int64_t* state;
    int64_t n_pad;
    const PodRec* shapes;
    const int32_t* shape_of;
    uint64_t* lists;
    int32_t* cnt;
    uint64_t* top;
    long long* ccount;
    Placement* out;
    int32_t* rb;
};
// one round from pod `first`: scan + merge for the shapes in `active` (bit j: a pod >= first has
// shape j), then the resolver.  cordon (ks_drain_at; null: none): bit nd % 32 of word nd / 32 takes
// node nd out of the scan.
//
// Exactness with a cordon.  The scan writes key 0 for a cordoned node, whatever its state: to every
// shape it is a node without an entry in the score map, which is what leaving k.nodes means
// (kubesim/kubesim.go:168-206 never visit it).  A block list, a candidate count and the merged top-L
// are functions of the keys alone, so they are those of the cluster without the cordoned nodes.  The
// resolver reads nodes through list entries (non-zero keys) and through the changed set (winners,
// which come from list entries): key 0 is never a list entry, so a cordoned node is never S, never
// joins the changed set, never contributes to D and is never committed — place_decide's argument
// above holds verbatim over the non-cordoned nodes.
hipError_t launch_place_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, int32_t first, uint64_t active,
                              hipStream_t st, const uint32_t* cordon = nullptr);
// the lists alone (ks_removable_at, ks_scale_up_at; a round's first half): scan + merge for the shapes
// in `active` on the state as it is — b.top and b.ccount of pc.n_shapes shapes; no resolver, nothing
// is committed
hipError_t launch_place_lists(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, uint64_t active, hipStream_t st,
                              const uint32_t* cordon = nullptr);
// after[n][4] from state [4][n_pad], the three quantities times sc
hipError_t launch_place_after(const int64_t* state, int64_t n_pad, int32_t n_nodes, const QScale& sc, long long* after,
                              hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Drain preview (ks_drain_at, ks_drain.hip): the pods running at tick t on a set of nodes, in FIFO
// order, re-placed by the rounds above on the state at t without those nodes (the cordon).
//
// The evicted pods are gathered by an ordered compaction without atomics over the candidate pod
// blocks the host lists in ascending order: a count per block (wave ballots), an exclusive scan of
// the counts, and a fill with the same predicate whose rank is
//   the block's offset + the selected pods of the waves before it + the selected lanes below it,
// so the output order is the pod order whatever the order of execution.  The records are the pods'
// own (whole device units), so the rounds always run in device units (scale 1).
//
// A round takes at most kPlaceMaxShapes distinct shapes and kPlaceMaxPods pods: the host feeds the
// evicted pods in segments (drain_segment) and the scratch state carries from one to the next.
// ---------------------------------------------------------------------------------------------
constexpr int kDrainBlk = 256;             // pods per gather workgroup (= the usage index's block)
constexpr int64_t kDrainMaxPods = 65536;   // KS_DRAIN_MAX_PODS

struct Eviction {  // = ks_eviction
    int64_t pod;
    int32_t from, node, status, pad;
    int64_t score, candidates;
};
static_assert(sizeof(Eviction) == 40, "ks_eviction layout");

// the set lanes of a wave ballot below `lane` (v_mbcnt on the device)
__host__ __device__ __forceinline__ int32_t drain_below(uint64_t ballot, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return (int32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
#else
    return __builtin_popcountll(ballot & ((1ull << lane) - 1ull));
#endif
}

// rank of a selected pod: its block's offset, the counts of the waves before its own, the lanes below it
__host__ __device__ __forceinline__ int64_t drain_rank(int64_t block_off, const int32_t* wave_cnt, int wave,
                                                       uint64_t ballot, int lane) {
    int64_t r = block_off;
    for (int w = 0; w < wave; ++w) r += wave_cnt[w];
    return r + drain_below(ballot, lane);
}

// whether a node's bit is set in a cordon bitmap
__host__ __device__ __forceinline__ bool drain_cordoned(const uint32_t* cordon, int32_t nd) {
    return (cordon[nd >> 5] >> (nd & 31)) & 1u;
}

// two pods have the same shape: masked requests, keymask, tol, sel (flags are ignored)
__host__ __device__ __forceinline__ bool drain_same_shape(const PodRec& a, const PodRec& b) {
    if (a.keymask != b.keymask || a.tol != b.tol || a.sel != b.sel) return false;
    for (int c = 0; c < 3; ++c)
        if ((a.keymask >> c & 1) && a.req[c] != b.req[c]) return false;
    return true;
}

// The segment that starts at pod `start` of recs[n]: it closes before the pod that would be its
// (kPlaceMaxShapes + 1)-th distinct shape or its (kPlaceMaxPods + 1)-th pod.  Returns its end
// (exclusive; > start when start < n), its distinct shapes in shapes[0, *n_shapes) in order of first
// appearance (masked requests, flags 0) and shape_of[i - start] for its pods.
inline int64_t drain_segment(const PodRec* recs, int64_t n, int64_t start, PodRec* shapes, int32_t* n_shapes,
                             int32_t* shape_of) {
    int32_t ns = 0;
    int64_t i = start;
    for (; i < n && i - start < kPlaceMaxPods; ++i) {
        int32_t j = 0;
        while (j < ns && !drain_same_shape(shapes[j], recs[i])) ++j;
        if (j == ns) {
            if (ns == kPlaceMaxShapes) break;
            PodRec r{};
            for (int c = 0; c < 3; ++c) r.req[c] = (recs[i].keymask >> c & 1) ? recs[i].req[c] : 0;
            r.tol = recs[i].tol; r.sel = recs[i].sel; r.keymask = recs[i].keymask;
            shapes[ns++] = r;
        }
        shape_of[i - start] = j;
    }
    *n_shapes = ns;
    return i;
}

// Scratch of the gather (device): cordon [ceil(n / 32)]; bcnt / boff [nblocks]; total [1];
// ev_pod / ev_from / ev_rec [cap] (the fill writes ranks < cap only).
struct DrainBufs {
    const uint32_t* cordon;
    int32_t* bcnt;
    int32_t* boff;
    long long* total;
    long long* ev_pod;
    int32_t* ev_from;
    PodRec* ev_rec;
    int64_t cap;
};
// bcnt, boff and *total over the candidate blocks (ascending) of the pods < q_hi
hipError_t launch_drain_count(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                              const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                              const DrainBufs& d, hipStream_t st);
// the evicted pods' rows, in pod order (after launch_drain_count on the same arguments)
hipError_t launch_drain_fill(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                             const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                             const PodRec* pods, const DrainBufs& d, hipStream_t st);
// zero the cordoned nodes' four words of state [4][n_pad]
hipError_t launch_drain_clear(const uint32_t* cordon, int32_t n_nodes, int64_t* state, int64_t n_pad, hipStream_t st);
// out[i] = {ev_pod[i], ev_from[i], placed[i]} for i < n_ev
hipError_t launch_drain_pack(const long long* ev_pod, const int32_t* ev_from, const Placement* placed, int64_t n_ev,
                             Eviction* out, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Removal scan (ks_removable_at, ks_removable.hip): for each of m candidate nodes on its own, the
// answer of the drain preview above with that node alone as the set.  Candidates are independent:
// every one starts from the same state at t, only the cordoned node differs.
//
// Exactness of one shared scan.  The snapshot top-L lists and the candidate counts of a segment's
// shapes are built once, on the base state at t with no cordon (launch_place_lists).  For
// candidate c the resolver
//   - starts its private flag words with every list entry whose node is c flagged, and never puts c
//     in its changed set;
//   - starts its running candidate counts at the base count minus place_is_cand(shape, c's base
//     record).
// Read "changed or removed" for "changed" in the argument above place_decide, over the nodes other
// than c: a flagged entry is a node that is changed or removed; an unflagged entry is a node other
// than c that no pod of this candidate was placed on, so it still has its snapshot key; those above
// the first unflagged entry S are all changed or removed, those below it or outside the list are
// smaller; a complete list (fewer than L entries) still means every node outside it — c included or
// not — has key 0; with all L entries flagged and D above the list's last key every unchanged node
// other than c lies outside the list, so below that key.  The three cases of place_decide hold
// verbatim.  c is never S (its entries are flagged from the start), so never a winner, never in the
// changed set and never in D; its pods' own requests stay in its base record, which nothing reads
// but the count correction.  That c's row is not emptied (ks_drain_at zeroes it) changes nothing: a
// cordoned node's state is never read there either.
//
// Progress.  A node is flagged when a pod is placed on it from the list, at most one per pod, so
// pod i (1-based) of a candidate finds at most (i - 1) + 1 flagged entries in its list.  kPlaceStop
// needs all L entries flagged, so a candidate with at most kRemovableMaxPods = L - 1 evicted pods is
// decided completely from one set of lists, with no rescan and nothing committed.  A candidate with
// more pods is answered through ks_drain_at's own path (removable_route): the same result by
// definition.
//
// Segments.  A resolver launch shares the lists of at most kPlaceMaxShapes shapes, so the host walks
// the batched candidates in the caller's order and closes a segment before the candidate that would
// bring its (kPlaceMaxShapes + 1)-th distinct shape (removable_segment); a candidate has at most
// L - 1 shapes, so it always fits an empty segment.  Segments are independent: all start from the
// base state.
// ---------------------------------------------------------------------------------------------
constexpr int kRemovableMaxPods = kPlaceL - 1;  // evicted pods of a candidate the batched resolver decides
static_assert(kRemovableMaxPods < kWave && kRemovableMaxPods < kPlaceMaxShapes, "a lane per changed node; a candidate fits a segment");
enum : int { kRemovableEmpty = 0, kRemovableBatched = 1, kRemovableDrain = 2 };

struct Removal {  // = ks_removal
    int32_t node, evicted, ok, over_capacity, not_found, removable;
    int64_t first_row;
};
static_assert(sizeof(Removal) == 32, "ks_removal layout");

// a batched candidate: its node, its pods' rows [first, first + count) in the caller-ordered rows
struct RemovalCand {
    int64_t first;
    int32_t node, count;
};
static_assert(sizeof(RemovalCand) == 16, "RemovalCand layout");

// who answers a candidate with `pods` running pods
__host__ __device__ __forceinline__ int removable_route(int64_t pods) {
    return pods <= 0 ? kRemovableEmpty : pods <= kRemovableMaxPods ? kRemovableBatched : kRemovableDrain;
}

// bit e: entry e of a snapshot list is a key of `node`
template <int L = kPlaceL>
__host__ __device__ __forceinline__ uint32_t removable_entries_on(const uint64_t* list, uint32_t node) {
    uint32_t bits = 0u;
    for (int e = 0; e < L; ++e)
        if (list[e] && place_key_node(list[e]) == node) bits |= 1u << e;
    return bits;
}

// The segment that starts at batched candidate `start` of cands[n_cand] (rows of recs, each
// candidate's contiguous): it closes before the candidate that would bring its (kPlaceMaxShapes +
// 1)-th distinct shape.  Returns its end (exclusive; > start when start < n_cand: a candidate has at
// most kRemovableMaxPods shapes), its distinct shapes in shapes[0, *n_shapes) in order of first
// appearance (masked requests, flags 0) and shape_of[row] for its candidates' rows.
inline int64_t removable_segment(const PodRec* recs, const RemovalCand* cands, int64_t n_cand, int64_t start,
                                 PodRec* shapes, int32_t* n_shapes, int32_t* shape_of) {
    int32_t ns = 0;
    int64_t a = start;
    for (; a < n_cand; ++a) {
        const int32_t before = ns;
        bool fits_in = true;
        for (int64_t row = cands[a].first; row < cands[a].first + cands[a].count; ++row) {
            int32_t j = 0;
            while (j < ns && !drain_same_shape(shapes[j], recs[row])) ++j;
            if (j == ns) {
                if (ns == kPlaceMaxShapes) {
                    fits_in = false;
                    break;
                }
                PodRec r{};
                for (int c = 0; c < 3; ++c) r.req[c] = (recs[row].keymask >> c & 1) ? recs[row].req[c] : 0;
                r.tol = recs[row].tol; r.sel = recs[row].sel; r.keymask = recs[row].keymask;
                shapes[ns++] = r;
            }
            shape_of[row] = j;
        }
        if (!fits_in) {
            ns = before;  // (the next segment numbers this candidate's rows again)
            break;
        }
    }
    *n_shapes = ns;
    return a;
}

// The gather's rows grouped by candidate (the removal scan and the consolidation preview): row i of
// the n_ev gathered rows runs on node from[i] of n and has the record fifo[i]; nodes[m] are the
// candidates, distinct and in [0, n).  A stable counting sort on the position in nodes[]: candidate
// j's evicted[j] rows stand at [first_row[j], first_row[j] + evicted[j]) in the caller's candidate
// order, FIFO within a candidate; perm[row] is the row's gather index and recs[row] its record.
// Returns -1, or the first row whose node is no candidate (the outputs are then unspecified).
inline int64_t group_rows(const int32_t* nodes, int32_t m, int64_t n, const int32_t* from, const PodRec* fifo, int64_t n_ev,
                          int32_t* evicted, int64_t* first_row, int32_t* perm, PodRec* recs) {
    std::vector<int32_t> pos(n, -1);
    for (int32_t j = 0; j < m; ++j) {
        pos[nodes[j]] = j;
        evicted[j] = 0;
    }
    for (int64_t i = 0; i < n_ev; ++i) {
        if ((uint32_t)from[i] >= (uint32_t)n || pos[from[i]] < 0) return i;
        evicted[pos[from[i]]]++;
    }
    std::vector<int64_t> next(m, 0);  // the next free row of each candidate
    for (int32_t j = 1; j < m; ++j) next[j] = next[j - 1] + evicted[j - 1];
    for (int32_t j = 0; j < m; ++j) first_row[j] = next[j];
    for (int64_t i = 0; i < n_ev; ++i) {
        const int64_t row = next[pos[from[i]]]++;
        perm[row] = (int32_t)i;
        recs[row] = fifo[i];
    }
    return -1;
}

// Scratch of the resolver (device): cands [batched candidates], in the caller's order; seg_shapes
// [segments][kPlaceMaxShapes]; shape_of [rows] (a row's shape among its segment's); ev_pod [rows] in
// gather order and perm [rows], the gather index of each caller-ordered row; rows [rows] and out
// [batched candidates], the results.
struct RemovableBufs {
    const RemovalCand* cands;
    const PodRec* seg_shapes;
    const int32_t* shape_of;
    const long long* ev_pod;
    const int32_t* perm;
    Eviction* rows;
    Removal* out;
};
// one segment: candidates [cand0, cand0 + n_cand) against the lists b.top / b.ccount of the
// pc.n_shapes shapes at `shapes` (after launch_place_lists on the same shapes)
hipError_t launch_removable_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const RemovableBufs& r,
                                    const PodRec* shapes, int64_t cand0, int64_t n_cand, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Scale-up preview (ks_scale_up_at, ks_scaleup.hip): for each of G options on its own, the answer of
// the placement preview above on the cluster plus max_nodes empty nodes of the option's template,
// appended at indices n .. n + max_nodes - 1 (k.nodes extended before the Filter loop,
// kubesim/kubesim.go:168-206).  Options are independent: every one starts from the same state at t,
// only the appended nodes differ.
//
// Exactness of one shared scan.  The snapshot top-L lists and the candidate counts are built once,
// on the base state at t over the n real nodes (launch_place_lists).  An appended node is in no
// list.  For option g the resolver keeps
//   - the invariant that the appended nodes in its changed set are a prefix n .. n + u - 1.  Every
//     other appended node is the empty template record: identical but for the index.  Among
//     identical nodes the key make_key(total + 1, node) is largest at the lowest index, so node
//     n + u stands for all of them: its key F (scaleup_fresh_key; 0 when u = max_nodes or the
//     template has no entry in the pod's score map) is the maximum over the unchanged appended nodes;
//   - D' = max(D, F) in D's place, D the largest key over the changed nodes, real and appended;
//   - running candidate counts that start at the base count plus max_nodes times
//     place_is_cand(shape, empty template) (scaleup_count_start) and move by place_cand_delta like
//     any other bind.
// Read the argument above place_decide over the real nodes, with the appended nodes on D's side:
// "entries above S are changed, everything below S or outside the list is smaller and unchanged"
// still covers every unchanged real node, because appended nodes are outside every list and never
// S.  The extended cluster's argmax is the maximum of the real nodes' argmax and the appended
// nodes' argmax max(D over appended changed nodes, F); cases (1)-(3) of place_decide give the
// former from S and D over the real changed nodes, and the maximum is monotone, so
// place_decide(S, last, D') is the extended argmax in each of them: (1) max(S, D'); (2) the list is
// complete, every unchanged real node has key 0: D' or none; (3) every unchanged real node is below
// the list's last key < D'.  When n + u wins it joins the changed set and u grows by one
// (scaleup_takes_fresh): the prefix holds.  A real node beats an equal appended node, and n + u
// beats n + u + 1, by the index half of the key alone.
//
// Case (4), kPlaceStop: an unchanged real node outside the list may win.  The resolver commits
// nothing, so it cannot rescan: it marks the option stopped and the host answers that option from
// pod 0 on its extended cluster built on the device (the single path: place_rounds on n + max_nodes
// nodes), which is the definition itself.  A stop needs all L entries of one list flagged, so at
// least L earlier pods bound to distinct real list nodes.
// ---------------------------------------------------------------------------------------------
constexpr int kScaleMaxOptions = 64;      // KS_SCALEUP_MAX_OPTIONS
constexpr int kScaleMaxNodes = 65536;     // KS_SCALEUP_MAX_NODES
enum : int32_t { kScaleBatched = 0, kScaleSingle = 1, kScaleStopped = -1 };

struct ScaleOption {  // an option on the device: the empty template node in the call's units
    NodeV tmpl;
    int32_t max_nodes, pad;
};
static_assert(sizeof(ScaleOption) == 88, "ScaleOption layout");

struct ScaleResult {  // = ks_scale_result
    int32_t ok, over_capacity, not_found, on_new, nodes_used, first_unplaced, path, pad;
};
static_assert(sizeof(ScaleResult) == 32, "ks_scale_result layout");

// The empty node of a template: alloc[4] in milli-units (-1 absent), divided by `unit` (the engine's
// scale when the call runs in device units, 1 when it runs in milli-units).
__host__ __device__ __forceinline__ NodeV scaleup_template(const int64_t* alloc, uint64_t taint, uint64_t label,
                                                           const QScale& unit) {
    NodeV v{};
    v.ac = alloc[0] > 0 ? alloc[0] / unit.f[0] : alloc[0];
    v.am = alloc[1] > 0 ? alloc[1] / unit.f[1] : alloc[1];
    v.ag = alloc[2] > 0 ? alloc[2] / unit.f[2] : alloc[2];
    v.ap = alloc[3];
    v.taint = taint; v.label = label;
    return v;
}

// place_whole_units' sibling: also every present template capacity is a whole multiple of sc
__host__ __device__ __forceinline__ bool scaleup_whole_units(const PodRec* shapes, int n_shapes, const int64_t* alloc,
                                                             int n_options, int64_t alloc_stride, const QScale& sc) {
    bool whole = place_whole_units(shapes, n_shapes, sc);
    for (int g = 0; g < n_options; ++g)
        for (int c = 0; c < 3; ++c)
            if (alloc[g * alloc_stride + c] > 0 && alloc[g * alloc_stride + c] % sc.f[c] != 0) whole = false;
    return whole;
}

// F: the key of appended node n + u on the empty template record, the largest over the appended
// nodes outside the changed set; 0 when there is none left
__host__ __device__ __forceinline__ uint64_t scaleup_fresh_key(const Cfg& c, const PodRec& p, const NodeV& tmpl,
                                                               int32_t n, int32_t u, int32_t max_nodes) {
    return u < max_nodes ? place_key(c, p, tmpl, (uint32_t)n + (uint32_t)u) : 0ull;
}

// a shape's running candidate count before the first pod: every appended node is the empty template
__host__ __device__ __forceinline__ long long scaleup_count_start(const Cfg& c, const PodRec& shape, const NodeV& tmpl,
                                                                  long long base, int32_t max_nodes) {
    return base + (place_is_cand(c, shape, tmpl) ? (long long)max_nodes : 0);
}

// the prefix rule: the winner X is the first appended node outside the changed set, so it joins it
__host__ __device__ __forceinline__ bool scaleup_takes_fresh(uint32_t X, int32_t n, int32_t u, int32_t max_nodes) {
    return u < max_nodes && X == (uint32_t)n + (uint32_t)u;
}

// Scratch of the batched resolver (device): opts [n_options]; rows [n_options][k]; out [n_options].
struct ScaleBufs {
    const ScaleOption* opts;
    Placement* rows;
    ScaleResult* out;
};
// every option against the lists b.top / b.ccount of pc.n_shapes shapes (after launch_place_lists on
// the same shapes and state); b.state is read only
hipError_t launch_scaleup_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ScaleBufs& sb,
                                  int32_t n_options, hipStream_t st);
// An option's extended cluster (the single path): the six constant fields of n_ext = n + max_nodes
// rows at dst (field f at dst + f * np_ext: ac am ag ap taint label), rows < n the cluster's times sc,
// rows n .. n_ext - 1 the template, the padding rows absent (-1, pods 0)
hipError_t launch_scaleup_extend(const NodeSoA& s, int32_t n, const QScale& sc, const ScaleOption& opt, int64_t np_ext,
                                 int64_t* dst, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Consolidation preview (ks_consolidate_at, ks_consolidate.hip): m candidate nodes handled in the
// caller's order as a chain of transactions on one private state.  R: the nodes removed so far; V:
// the nodes that received a moved pod.  A candidate in V is a destination and nothing is tried; any
// other candidate c leaves k.nodes together with R and its pods go to scheduleOne in FIFO order
// until one is not bound Ok; all Ok (or no pod): c joins R, the placements stay, their nodes join V;
// otherwise everything is as it was before c.
//
// Exactness of a round.  A round scans the committed scratch state with R as the cordon (the
// argument above launch_place_round: the lists and the counts are those of the cluster without R)
// and then walks candidates in order with one changed set, one set of flags and one set of running
// counts.  Read "changed, removed in this round, or the open candidate" for "changed" in the
// argument above place_decide: the resolver flags every list entry on the open candidate c before
// c's first pod and corrects the counts by place_is_cand(shape, c's record) (the removal scan's
// argument, above removable_route: c is never S, never a winner, never in the changed set, never in
// D; c is in no changed set because a changed node is a destination and is not tried).  An
// unflagged entry is a node no pod was placed on in this round, not removed and not c: it still has
// its snapshot key, so place_decide's three cases hold verbatim over the nodes outside R and c.
//   accept  c's flags and its count correction stay: for the rest of the round c is a removed
//           node.  Its row of the scratch is zeroed and its cordon bit set for the next scan.
//   block   the state must be exactly the state before c.  The attempt changed four things: the
//           changed nodes' records (place_bind adds the masked requests and one pod on Ok and
//           nothing else, so subtracting them per Ok pod restores a slot that existed before c;
//           slots appended by the attempt lie at [nchg before c, nchg) and are dropped), the flag
//           words, the running counts (both restored from the copies taken before c's own flags
//           were set) and nchg.  A dropped slot's node is unchanged again and its entries are
//           unflagged again: it has its snapshot key, as the argument needs.
// A removed node is never in V (a destination is not tried) and a node in V is never removed, so
// the round's commit — the changed nodes' records, the `received` bits, the removed nodes' zero rows
// and cordon bits — never writes one node twice.
//
// Progress.  A round's first candidate finds fresh lists with nothing flagged but its own entries,
// so its pod i (1-based) finds at most (i - 1) + 1 flagged entries: with at most kConsMaxPods =
// L - 1 pods it is decided in that round (the removal scan's argument).  kPlaceStop inside a later
// candidate rolls that candidate back and ends the round; it opens the next one.  A candidate with
// more pods (consolidate_route) is answered by the host's single path when it is the next to be
// decided: a copy of the scratch state, the placement rounds with the cordon R + c, adopted iff
// every pod was bound Ok.  The segment walk closes before such a candidate, so it always heads a
// round of its own; whether it is a destination is read from `received` first.
// ---------------------------------------------------------------------------------------------
constexpr int kConsMaxPods = kPlaceL - 1;  // pods of a candidate the rounds decide
enum : int32_t { kConsBlocked = 0, kConsRemoved = 1, kConsDestination = 2 };  // KS_CONSOLIDATE_*
enum : int { kConsRound = 0, kConsSingle = 1 };

struct Consolidation {  // = ks_consolidation
    int32_t node, evicted, outcome, rows, block_status, pad;
    int64_t first_row;
};
static_assert(sizeof(Consolidation) == 32, "ks_consolidation layout");

// who decides a candidate with `pods` running pods (when it is not a destination)
__host__ __device__ __forceinline__ int consolidate_route(int64_t pods) {
    return pods <= kConsMaxPods ? kConsRound : kConsSingle;
}

// The round that starts at candidate `start` of cands[m] (rows of recs, each candidate's
// contiguous, in the caller's order): it closes before the candidate that would bring its
// (kPlaceMaxShapes + 1)-th distinct shape or its (kPlaceMaxPods + 1)-th pod, and before a candidate
// of the single path.  Returns its end (exclusive; > start when cands[start] is of the round path: such
// a candidate has at most kConsMaxPods pods and shapes), its distinct shapes in shapes[0, *n_shapes)
// in order of first appearance (masked requests, flags 0), shape_of[row - cands[start].first] for
// its rows and their number in *n_pods.
inline int64_t consolidate_segment(const PodRec* recs, const RemovalCand* cands, int64_t m, int64_t start,
                                   PodRec* shapes, int32_t* n_shapes, int32_t* shape_of, int32_t* n_pods) {
    int32_t ns = 0, np = 0;
    int64_t a = start;
    const int64_t row0 = start < m ? cands[start].first : 0;
    for (; a < m; ++a) {
        if (consolidate_route(cands[a].count) != kConsRound || np + cands[a].count > kPlaceMaxPods) break;
        const int32_t before = ns;
        bool fits_in = true;
        for (int64_t row = cands[a].first; row < cands[a].first + cands[a].count; ++row) {
            int32_t j = 0;
            while (j < ns && !drain_same_shape(shapes[j], recs[row])) ++j;
            if (j == ns) {
                if (ns == kPlaceMaxShapes) {
                    fits_in = false;
                    break;
                }
                PodRec r{};
                for (int c = 0; c < 3; ++c) r.req[c] = (recs[row].keymask >> c & 1) ? recs[row].req[c] : 0;
                r.tol = recs[row].tol; r.sel = recs[row].sel; r.keymask = recs[row].keymask;
                shapes[ns++] = r;
            }
            shape_of[row - row0] = j;
        }
        if (!fits_in) {
            ns = before;  // (the next round numbers this candidate's rows again)
            break;
        }
        np += cands[a].count;
    }
    *n_shapes = ns;
    *n_pods = np;
    return a;
}

// One round on the device: cands [m], every candidate in the caller's order (rows [first, first +
// count) of the caller-ordered rows); the round's candidates [c0, c1) and row0 = cands[c0].first;
// cordon / received [ceil(n / 32)], the bitmaps of R and V; out [m], the answers.
struct ConsRound {
    const RemovalCand* cands;
    int32_t c0, c1;
    int64_t row0;
    uint32_t* cordon;
    uint32_t* received;
    Consolidation* out;
};
// scan + merge of pc.n_shapes shapes on b.state with cr.cordon (none when the round has no pod:
// pc.k = pc.n_shapes = 0), then the resolver: pods [0, pc.k) are rows [row0, row0 + pc.k), their
// placements go to b.out[0, pc.k), b.rb gets {the next candidate, 1 if none was decided, the changed
// nodes committed, the pods before the next candidate}
hipError_t launch_consolidate_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ConsRound& cr,
                                    hipStream_t st);
// the single path: node leaves (its cordon bit set, its row of state [4][n_pad] zeroed) ...
hipError_t launch_consolidate_take(uint32_t* cordon, int64_t* state, int64_t n_pad, int32_t n_nodes, int32_t node,
                                   hipStream_t st);
// ... and, once adopted, the nodes of its k placements join `received`
hipError_t launch_consolidate_mark(const Placement* placed, int64_t k, int32_t n_nodes, uint32_t* received, hipStream_t st);

// ---------------------------------------------------------------------------------------------
// Gang admission preview (ks_gang_at, ks_gang.hip): m pod groups handled in the caller's order as a
// chain of transactions on one private state.  Gang g's pods go to scheduleOne one after another; a
// pod bound Ok joins its node, a pod not bound Ok changes nothing and the attempt goes on until
// more than size - min_ok of them were not bound Ok.  At least min_ok Ok pods at the gang's end: the
// gang is admitted and its placements stay; otherwise everything is as it was before g.
//
// Exactness of a round.  A round scans the committed scratch state with no cordon and then walks
// gangs in order with one changed set, one set of flags and one set of running counts: the
// argument above place_decide holds as it stands, a gang's opening sets no flag and corrects no
// count.  A pod bound OverCapacity may append its node to the changed set with its record as it
// was: the node is evaluated exactly on D's side from then on, which the argument allows.
//   admit   nothing is restored: the flags, the counts and the changed set stay for the rest of
//           the round.
//   block   the state must be exactly the state before g.  The attempt changed four things: the
//           changed nodes' records (place_bind adds the masked requests and one pod on Ok and
//           nothing else, so subtracting them for every tried pod whose own status is Ok restores
//           a slot that existed before g — a pod not bound Ok added nothing and subtracts nothing;
//           slots appended by the attempt lie at [nchg before g, nchg) and are dropped), the flag
//           words, the running counts (both restored from the copies taken when g opened) and
//           nchg.  A dropped slot's node is unchanged again and its entries are unflagged again: it
//           has its snapshot key, as the argument needs.
// The round's commit is the placement rounds': the changed nodes' records, each node once.
//
// Progress.  A round's first gang finds fresh lists with nothing flagged, so its pod i (1-based)
// finds at most i - 1 flagged entries: with at most kGangMaxPods = L pods (so at most L <= 64
// shapes) it is decided in that round.  kPlaceStop inside a later gang rolls that gang back and ends
// the round; it opens the next one.  A gang with more pods (gang_route) is answered by the host's
// single path when it is the next to be decided: a copy of the scratch state, the drain preview's
// segmented rounds on the gang's pods with no cordon, the early end applied to the finished rows
// (exact: a pod not bound Ok changes nothing, so the rows up to the deciding pod are the attempt's),
// adopted iff the gang is admitted.  The segment walk closes before such a gang.
// ---------------------------------------------------------------------------------------------
constexpr int kGangMaxPods = kPlaceL;       // pods of a gang the rounds decide
constexpr int64_t kGangMaxGangs = 65536;    // KS_GANG_MAX_GANGS
constexpr int32_t kGangMaxShapes = 4096;    // KS_GANG_MAX_SHAPES
constexpr int32_t kGangNotTried = -2;       // KS_GANG_NOT_TRIED
enum : int32_t { kGangBlocked = 0, kGangAdmitted = 1, kGangSkipped = 2, kGangUndecided = -1 };  // KS_GANG_*
enum : int { kGangRound = 0, kGangSingle = 1 };
static_assert(kGangMaxPods <= kPlaceMaxShapes && kGangMaxPods <= kPlaceMaxPods, "a round-path gang fits a round");

struct Gang {  // = ks_gang
    int32_t first, size, outcome, tried, ok, over_capacity, not_found, block_status;
};
static_assert(sizeof(Gang) == 32, "ks_gang layout");
struct GangIn {  // a gang as the resolver reads it: rows [first, first + size) of the call's pods
    int32_t first, size, min_ok, pad;
};
static_assert(sizeof(GangIn) == 16, "one scalar load");

// who decides a gang of `pods` pods
__host__ __device__ __forceinline__ int gang_route(int64_t pods) { return pods <= kGangMaxPods ? kGangRound : kGangSingle; }

// The round that starts at gang `start` of gangs[m] (rows of recs): it closes before the gang that
// would bring its (kPlaceMaxShapes + 1)-th distinct shape or its (kPlaceMaxPods + 1)-th pod, and
// before a gang of the single path.  Returns its end (exclusive; > start when gangs[start] is of the
// round path), its distinct shapes in shapes[0, *n_shapes) in order of first appearance (masked
// requests, flags 0), shape_of[row - gangs[start].first] for its rows and their number in *n_pods.
inline int64_t gang_segment(const PodRec* recs, const GangIn* gangs, int64_t m, int64_t start, PodRec* shapes,
                            int32_t* n_shapes, int32_t* shape_of, int32_t* n_pods) {
    int32_t ns = 0, np = 0;
    int64_t a = start;
    const int64_t row0 = start < m ? gangs[start].first : 0;
    for (; a < m; ++a) {
        if (gang_route(gangs[a].size) != kGangRound || np + gangs[a].size > kPlaceMaxPods) break;
        const int32_t before = ns;
        bool fits_in = true;
        for (int64_t row = gangs[a].first; row < (int64_t)gangs[a].first + gangs[a].size; ++row) {
            int32_t j = 0;
            while (j < ns && !drain_same_shape(shapes[j], recs[row])) ++j;
            if (j == ns) {
                if (ns == kPlaceMaxShapes) {
                    fits_in = false;
                    break;
                }
                PodRec r{};
                for (int c = 0; c < 3; ++c) r.req[c] = (recs[row].keymask >> c & 1) ? recs[row].req[c] : 0;
                r.tol = recs[row].tol; r.sel = recs[row].sel; r.keymask = recs[row].keymask;
                shapes[ns++] = r;
            }
            shape_of[row - row0] = j;
        }
        if (!fits_in) {
            ns = before;  // (the next round numbers this gang's rows again)
            break;
        }
        np += gangs[a].size;
    }
    *n_shapes = ns;
    *n_pods = np;
    return a;
}

// One round on the device: gangs [m], every gang in the caller's order; the round's gangs [g0, g1)
// and row0 = gangs[g0].first; strict: the first blocked gang ends the pass; out [m], the answers.
struct GangRound {
    const GangIn* gangs;
    int32_t g0, g1, m, strict;
    int64_t row0;
    Gang* out;
};
// scan + merge of pc.n_shapes shapes on b.state (none when the round has no pod: pc.k = pc.n_shapes
// = 0), then the resolver: pods [0, pc.k) are rows [row0, row0 + pc.k), their placements go to
// b.out[0, pc.k), b.rb gets {the next gang (m: a strict pass ended), 1 if none was decided, the
// changed nodes committed, the pods before the next gang}
hipError_t launch_gang_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const GangRound& gr, hipStream_t st);


}  // namespace ks
