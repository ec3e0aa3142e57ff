// ks_previews.cpp — the six previews of include/ks_engine.h: what scheduleOne would do on a private
// copy of the state at a past tick (ks_place_at, ks_drain_at, ks_removable_at, ks_consolidate_at,
// ks_gang_at, ks_scale_up_at).  They open like the past-tick queries of ks_queries.cpp (ks_queries.h), read the
// engine and write nothing a later ks_step reads; their device contract is ks_query.h.
#include <cstring>

#include "ks_queries.h"

using namespace ks_host;

// a field stands at the same offset in the C record and in the device's
#define SAME_FIELD(c_rec, ks_rec, f) (offsetof(c_rec, f) == offsetof(ks::ks_rec, f))

extern "C" {

// ---- placement preview (ks_place.hip) ----------------------------------------------------------
// scheduleOne for k preview pods on a private copy of the state at tick t: the rebuilt rc rm rg nr in
// milli-units (the shapes' own units; nothing of the engine is rescaled) in the query scratch — or in
// device units when every request is a whole multiple of the engine's unit — decided in rounds:
// scan + merge give the exact top-kPlaceL snapshot list of every shape still to be placed, one
// workgroup decides pods in order until one needs a node outside its list (ks_query.h), and the
// host reads back 16 bytes per round: the first undecided pod.
static_assert(KS_PLACE_MAX_PODS == ks::kPlaceMaxPods && KS_PLACE_MAX_SHAPES == ks::kPlaceMaxShapes &&
              KS_PLACE_MAX_SHAPES == KS_HEADROOM_MAX_SHAPES && KS_PLACE_NOT_FOUND == ks::kPlaceNotFound &&
              KS_POD_OK == ks::kPlaceOk && KS_POD_OVER_CAPACITY == ks::kPlaceOverCapacity && KS_PLACE_INFO == 4 &&
              sizeof(ks_placement) == sizeof(ks::Placement) && SAME_FIELD(ks_placement, Placement, score) &&
              SAME_FIELD(ks_placement, Placement, candidates),
              "ks_place_at constants and record");

// One upload for a set of rounds: the shape records (ns of KS_PLACE_MAX_SHAPES), then shape_of[k].
// h_up is the caller's: it outlives the copy.
static ks_status upload_shapes(ks_engine* e, const ks::PlaceBufs& b, std::vector<unsigned long long>& h_up,
                               const ks::PodRec* shapes, int32_t ns, const int32_t* so, int32_t k) {
    const int64_t words = kShapeWords + (k + 1) / 2;
    if ((int64_t)h_up.size() < words) h_up.resize(words, 0ull);
    std::memcpy(h_up.data(), shapes, sizeof(ks::PodRec) * ns);
    std::memcpy(h_up.data() + kShapeWords, so, sizeof(int32_t) * k);
    HIPCHK(e, hipMemcpyAsync((void*)b.shapes, h_up.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, e->st));
    return KS_OK;
}

// k pods' shapes, checked: so[j] = shape_of[j], or j without shape_of (then k = n_shapes)
static ks_status pod_shapes(ks_engine* e, const char* what, int32_t k, const int32_t* shape_of, int32_t n_shapes,
                            std::vector<int32_t>* so) {
    if (k < 1 || k > KS_PLACE_MAX_PODS) return fail(e, KS_EINVAL, "%s: %d pods outside [1, %d]", what, (int)k, KS_PLACE_MAX_PODS);
    if (!shape_of && k != n_shapes)
        return fail(e, KS_EINVAL, "%s: %d pods without shape_of need %d shapes, not %d", what, (int)k, (int)k, (int)n_shapes);
    so->resize(k);
    for (int32_t j = 0; j < k; j++) {
        const int32_t sh = (*so)[j] = shape_of ? shape_of[j] : j;
        if (sh < 0 || sh >= n_shapes)
            return fail(e, KS_EINVAL, "%s: pod %d has shape %d outside [0, %d)", what, (int)j, (int)sh, (int)n_shapes);
    }
    return KS_OK;
}

// the call's units: device units when `whole` (e->h_shapes are divided into them), else milli-units
static ks::QScale call_units(ks_engine* e, bool whole, const ks::QScale& milli) {
    if (whole)
        for (ks::PodRec& r : e->h_shapes)
            for (int c = 0; c < 3; c++) r.req[c] /= milli.f[c];
    return whole ? kDeviceUnits : milli;
}
// `active` for the lists of all ns shapes; info[1..3] by a pod's status: bound Ok, bound OverCapacity, not found
static uint64_t all_shapes(int32_t ns) { return ns >= 64 ? ~0ull : (1ull << ns) - 1ull; }
static void tally(int64_t* info, int32_t status) { info[status == KS_POD_OK ? 1 : status == KS_POD_OVER_CAPACITY ? 2 : 3]++; }
// a preview's last step: after_out (null: none) is the scratch state times sc as [n][4] rows; the stream's end
static ks_status finish_after(ks_engine* e, const ks::PlaceBufs& b, const ks::QScale& sc, long long* after, int64_t* after_out) {
    if (after_out) {
        HIPCHK(e, ks::launch_place_after(b.state, b.n_pad, (int32_t)e->n, sc, after, e->st));
        HIPCHK(e, hipMemcpyAsync(after_out, after, sizeof(int64_t) * 4 * e->n, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

// A round's 16 bytes, read back: *next is where it ended — the first pod, or candidate, it left
// undecided — or -1 unless that lies in (first, limit].  A round decides its first at the least
// (nothing is changed yet; ks_query.h, Progress): anything else is a fault, which the caller names.
static ks_status round_end(ks_engine* e, const ks::PlaceBufs& b, int32_t first, int32_t limit, int32_t* next) {
    int32_t rb[4] = {0, 1, 0, 0};
    HIPCHK(e, hipMemcpyAsync(rb, b.rb, sizeof(rb), hipMemcpyDeviceToHost, e->st));  // 16 bytes per round
    HIPCHK(e, hipStreamSynchronize(e->st));
    *next = rb[1] != 0 || rb[0] <= first || rb[0] > limit ? -1 : rb[0];
    return KS_OK;
}

// The rounds that decide pods [0, pc.k) of the uploaded shapes: each launches scan + merge + resolver
// from the first undecided pod and reads back 16 bytes.  nodes: the cluster's constants (e->s, or an
// extended cluster of ks_scale_up_at).  what and pod_base name the pod in the message
// of a round that decided none; *rounds grows by the rounds run.
static ks_status place_rounds(ks_engine* e, const ks::NodeSoA& nodes, const ks::PlaceCfg& pc, const ks::PlaceBufs& b,
                              const int32_t* so, const uint32_t* cordon, const char* what, int64_t pod_base,
                              int64_t* rounds) {
    int32_t first = 0;
    for (int64_t r = 1; first < pc.k; r++) {
        uint64_t active = 0;
        for (int32_t j = first; j < pc.k; j++) active |= 1ull << so[j];
        HIPCHK(e, ks::launch_place_round(nodes, pc, b, first, active, e->st, cordon));
        int32_t next = -1;
        if (ks_status rc = round_end(e, b, first, pc.k, &next); rc != KS_OK) return rc;
        if (next < 0 || r > pc.k) return fail(e, KS_EDEVICE, "%s %lld decided no pod", what, (long long)(pod_base + first));
        first = next;
        ++*rounds;
    }
    return KS_OK;
}

ks_status ks_place_at(ks_engine* e, int64_t t, int32_t n_shapes, const int64_t* req, const uint8_t* keymask,
                      const uint64_t* tol, const uint64_t* sel, int32_t k, const int32_t* shape_of, ks_placement* out,
                      int64_t* after_out, int64_t* info_out) {
    if (!e || !req || !keymask || !tol || !sel || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = head_shapes(e, n_shapes, req, keymask, tol, sel, "place"); r != KS_OK) return r;
    std::vector<int32_t> so;
    if (ks_status r = pod_shapes(e, "place", k, shape_of, n_shapes, &so); r != KS_OK) return r;
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    int64_t info[KS_PLACE_INFO] = {0, 0, 0, 0};
    if (e->n == 0) {
        for (int32_t j = 0; j < k; j++) out[j] = ks_placement{-1, KS_PLACE_NOT_FOUND, -1, 0};
        info[3] = k;
        if (info_out) std::copy(info, info + KS_PLACE_INFO, info_out);
        return KS_OK;
    }
    const int64_t q_hi = bound_by(e, t);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    PlaceScratch s;
    CARVE_SCRATCH(e, s = carve_place_at(qs, qi, n, np, nblk, k));
    const ks::PlaceBufs& b = s.b;  // state in milli-units, or device units (below)
    // whole-unit requests: the call runs in device units (same placements, 64-bit BalancedAllocation)
    const ks::QScale milli = milli_scale(e);
    const bool whole = ks::place_whole_units(e->h_shapes.data(), n_shapes, milli);
    const ks::QScale sc = call_units(e, whole, milli);
    if (ks_status r = rebuild_state(e, nb, q_hi, t, sc, 1, np, (unsigned long long*)b.state); r != KS_OK) return r;
    std::vector<unsigned long long> h_up;
    if (ks_status r = upload_shapes(e, b, h_up, e->h_shapes.data(), n_shapes, so.data(), k); r != KS_OK) return r;
    const ks::PlaceCfg pc{e->dc, sc, (int32_t)n, k, n_shapes, (int32_t)nblk};
    if (ks_status r = place_rounds(e, e->s, pc, b, so.data(), nullptr, "place: the round from pod", 0, &info[0]); r != KS_OK)
        return r;
    // rb[4], then out[k]: one range, read once
    constexpr int64_t PW = sizeof(ks::Placement) / sizeof(unsigned long long);
    std::vector<unsigned long long> h_down(2 + PW * k, 0ull);
    HIPCHK(e, hipMemcpyAsync(h_down.data(), b.rb, sizeof(unsigned long long) * h_down.size(), hipMemcpyDeviceToHost, e->st));
    if (ks_status r = finish_after(e, b, whole ? milli : kDeviceUnits, s.after, after_out); r != KS_OK) return r;
    std::memcpy(out, h_down.data() + 2, sizeof(ks_placement) * k);
    for (int32_t j = 0; j < k; j++) tally(info, out[j].status);
    if (info_out) std::copy(info, info + KS_PLACE_INFO, info_out);
    return KS_OK;
}

// ---- drain preview (ks_drain.hip) ---------------------------------------------------------------
// The pods running at t on the cordoned nodes, gathered on the device in FIFO order (count, scan,
// fill: the host reads the 8-byte total first and sizes the rest from it), then ks_place_at's round
// loop over them in segments of at most KS_PLACE_MAX_SHAPES distinct shapes and KS_PLACE_MAX_PODS
// pods (ks::drain_segment) on the state at t with the cordoned rows zeroed.  The pods' records are
// whole device units, so the rounds run in device units throughout; a round commits its changed
// nodes to the scratch, which carries the state from one segment to the next.
static_assert(KS_DRAIN_MAX_PODS == ks::kDrainMaxPods && KS_DRAIN_INFO == 6 && sizeof(ks_eviction) == sizeof(ks::Eviction) &&
              SAME_FIELD(ks_eviction, Eviction, pod) && SAME_FIELD(ks_eviction, Eviction, from) &&
              SAME_FIELD(ks_eviction, Eviction, node) && SAME_FIELD(ks_eviction, Eviction, status) &&
              SAME_FIELD(ks_eviction, Eviction, score) && SAME_FIELD(ks_eviction, Eviction, candidates) &&
              kUBlk == ks::kDrainBlk,
              "ks_drain_at constants and record");

// A query's node set as a bitmap: nodes[n_set] distinct indices in [0, n), n_set in [1, n] (n = 0: 0)
static ks_status node_set(ks_engine* e, const char* what, int32_t n_set, const int32_t* nodes, std::vector<uint32_t>* bits) {
    const int64_t n = e->n;
    if (n_set < (n ? 1 : 0) || n_set > n)
        return fail(e, KS_EINVAL, "%s: %d nodes outside [%d, %lld]", what, (int)n_set, n ? 1 : 0, (long long)n);
    bits->assign((n + 31) / 32, 0u);
    for (int32_t j = 0; j < n_set; j++) {
        const int32_t nd = nodes[j];
        if (nd < 0 || nd >= n) return fail(e, KS_EINVAL, "%s: node %d outside [0, %lld)", what, (int)nd, (long long)n);
        if ((*bits)[nd >> 5] >> (nd & 31) & 1u) return fail(e, KS_EINVAL, "%s: node %d is listed twice", what, (int)nd);
        (*bits)[nd >> 5] |= 1u << (nd & 31);
    }
    return KS_OK;
}

// The gather's count: the candidate blocks at t, the int32 scratch (carve_drain_gather), the node set
// uploaded as the cordon, and n_ev, the pods running at t on the set (8 bytes read back first)
struct DrainCount {
    int64_t q_hi, nb, n_ev;
    DrainGather g;
};
static ks_status drain_count(ks_engine* e, const char* what, int64_t t, const std::vector<uint32_t>& h_cordon,
                             DrainCount* c) {
    const int64_t n = e->n, nblk = (n + 255) / 256, CW = (int64_t)h_cordon.size();
    c->q_hi = bound_by(e, t);
    c->nb = 0;
    if (ks_status r = query_blocks(e, t, c->q_hi, &c->nb); r != KS_OK) return r;
    if (c->nb * kUBlk > INT32_MAX)
        return fail(e, KS_EINVAL, "%s: tick %lld holds too many candidate pods", what, (long long)t);
    { CARVE_SCRATCH(e, c->g = carve_drain_gather(qi, CW, c->nb, nblk)); }
    const ks::DrainBufs& d = c->g.d;
    HIPCHK(e, hipMemcpyAsync((void*)d.cordon, h_cordon.data(), sizeof(uint32_t) * CW, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, ks::launch_drain_count(e->d_blk.p, c->nb, c->q_hi, t, (int32_t)n, e->b_node.p, e->b_status.p, e->t0.p,
                                     e->dur.p, d, e->st));
    long long total = 0;
    HIPCHK(e, hipMemcpyAsync(&total, d.total, sizeof(total), hipMemcpyDeviceToHost, e->st));  // 8 bytes first
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (total < 0 || total > c->nb * kUBlk) return fail(e, KS_EDEVICE, "%s: the gather counted %lld pods", what, total);
    c->n_ev = total;
    return KS_OK;
}

// ... and its rows once the scratch is carved (d: the gather's buffers with ev_* set): the n_ev
// pods' records, and the nodes they run on when `from` is asked for, read back in FIFO order
static ks_status drain_rows(ks_engine* e, int64_t t, const DrainCount& c, const ks::DrainBufs& d,
                            std::vector<ks::PodRec>* recs, std::vector<int32_t>* from) {
    HIPCHK(e, ks::launch_drain_fill(e->d_blk.p, c.nb, c.q_hi, t, (int32_t)e->n, e->b_node.p, e->b_status.p, e->t0.p,
                                    e->dur.p, e->pods.p, d, e->st));
    recs->resize(c.n_ev);
    HIPCHK(e, hipMemcpyAsync(recs->data(), d.ev_rec, sizeof(ks::PodRec) * c.n_ev, hipMemcpyDeviceToHost, e->st));
    if (from) {
        from->resize(c.n_ev);
        HIPCHK(e, hipMemcpyAsync(from->data(), d.ev_from, sizeof(int32_t) * c.n_ev, hipMemcpyDeviceToHost, e->st));
    }
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

// The opening of the three node-set previews: the node set as a bitmap, the tick, the gather's
// count, and the check that its rows fit — room is what the caller's rows hold (ks_drain_at: cap,
// always; the others: cap when rows are asked for), KS_DRAIN_MAX_PODS at the most.  *n_ev is
// set once known; on a cluster of no node nothing is counted, *n_ev is 0 and the caller answers.
static ks_status gather_open(ks_engine* e, const char* what, int64_t t, int32_t n_set, const int32_t* nodes, int64_t room,
                             std::vector<uint32_t>* set, DrainCount* gc, int64_t* n_ev) {
    if (ks_status r = node_set(e, what, n_set, nodes, set); r != KS_OK) return r;
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    gc->n_ev = 0;
    if (e->n)
        if (ks_status r = drain_count(e, what, t, *set, gc); r != KS_OK) return r;
    *n_ev = gc->n_ev;
    room = std::min<int64_t>(room, KS_DRAIN_MAX_PODS);
    if (gc->n_ev > room)
        return fail(e, KS_ERANGE, "%s: %lld evicted pods, room for %lld (at most %d per call)", what, (long long)gc->n_ev,
                    (long long)room, KS_DRAIN_MAX_PODS);
    return KS_OK;
}

// ks_drain_at's rounds over the rows recs[0, count), in segments (ks::drain_segment): a segment
// uploads its shapes and place_rounds decides its pods with `cordon` on b.state, which carries from
// one segment to the next; row i's placement goes to out[i].  what and pod_base name a row in the
// messages; *rounds and *segments (null: not counted) grow by those run.  after (empty: none) is
// called once the segment [start, start + k) is decided and says whether to go on.  sc: the records'
// units (evicted pods' own records: device units).
using SegmentHook = std::function<ks_status(int64_t start, int32_t k, bool* go_on)>;
static ks_status drain_rounds(ks_engine* e, ks::PlaceBufs b, ks::Placement* out, const ks::PodRec* recs, int64_t count,
                              const uint32_t* cordon, const char* what, int64_t pod_base, int64_t* rounds,
                              int64_t* segments, const SegmentHook& after = {}, const ks::QScale& sc = kDeviceUnits) {
    const std::string round_what = std::string(what) + ": the round from evicted pod";
    std::vector<unsigned long long> h_up;
    std::vector<int32_t> so(KS_PLACE_MAX_PODS);
    ks::PodRec seg_shapes[KS_PLACE_MAX_SHAPES];
    bool go_on = true;
    for (int64_t start = 0; start < count && go_on;) {
        int32_t ns = 0;
        const int64_t end = ks::drain_segment(recs, count, start, seg_shapes, &ns, so.data());
        const int32_t k = (int32_t)(end - start);
        if (k < 1 || ns < 1)
            return fail(e, KS_EDEVICE, "%s: empty segment at evicted pod %lld", what, (long long)(pod_base + start));
        if (ks_status r = upload_shapes(e, b, h_up, seg_shapes, ns, so.data(), k); r != KS_OK) return r;
        b.out = out + start;
        const ks::PlaceCfg pc{e->dc, sc, (int32_t)e->n, k, ns, (int32_t)((e->n + 255) / 256)};
        if (ks_status r = place_rounds(e, e->s, pc, b, so.data(), cordon, round_what.c_str(), pod_base + start, rounds); r != KS_OK)
            return r;
        if (segments) ++*segments;
        if (after)
            if (ks_status r = after(start, k, &go_on); r != KS_OK) return r;
        start = end;
    }
    return KS_OK;
}

ks_status ks_drain_at(ks_engine* e, int64_t t, int32_t n_drain, const int32_t* nodes, ks_eviction* out, int64_t cap,
                      int64_t* n_out, int64_t* after_out, int64_t* info_out) {
    if (!e || !nodes || !n_out || cap < 0 || (cap > 0 && !out)) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    // ---- the gather's count (cap always counts: every evicted pod has a row) ----
    std::vector<uint32_t> h_cordon;
    DrainCount gc;
    if (ks_status r = gather_open(e, "drain", t, n_drain, nodes, cap, &h_cordon, &gc, n_out); r != KS_OK) return r;
    const int64_t CW = (int64_t)h_cordon.size();
    int64_t info[KS_DRAIN_INFO] = {0, 0, 0, 0, 0, 0};
    if (n == 0) {
        if (info_out) std::copy(info, info + KS_DRAIN_INFO, info_out);
        return KS_OK;
    }
    DrainGather& g = gc.g;
    ks::DrainBufs& d = g.d;
    const int64_t n_ev = gc.n_ev, nb = gc.nb, q_hi = gc.q_hi;
    // ---- the rest of the scratch, sized from the total ----
    DrainScratch s;
    CARVE_SCRATCH(e, s = carve_drain(qs, n, np, nblk, n_ev, &d));
    ks::PlaceBufs b = s.b;
    b.cnt = g.cnt;
    if (ks_status r = rebuild_state(e, nb, q_hi, t, kDeviceUnits, 1, np, (unsigned long long*)b.state); r != KS_OK) return r;
    HIPCHK(e, ks::launch_drain_clear(d.cordon, (int32_t)n, b.state, np, e->st));
    std::vector<ks::Eviction> h_ev(n_ev);
    if (n_ev) {
        std::vector<ks::PodRec> recs;
        if (ks_status r = drain_rows(e, t, gc, d, &recs, nullptr); r != KS_OK) return r;
        if (ks_status r = drain_rounds(e, b, s.b.out, recs.data(), n_ev, d.cordon, "drain", 0, &info[0], &info[4]); r != KS_OK)
            return r;
        HIPCHK(e, ks::launch_drain_pack(d.ev_pod, d.ev_from, s.b.out, n_ev, s.evict, e->st));
        HIPCHK(e, hipMemcpyAsync(h_ev.data(), s.evict, sizeof(ks::Eviction) * n_ev, hipMemcpyDeviceToHost, e->st));
    }
    if (ks_status r = finish_after(e, b, milli_scale(e), s.after, after_out); r != KS_OK) return r;
    std::vector<uint32_t> seen(CW, 0u);
    int64_t busy = 0;
    for (int64_t i = 0; i < n_ev; i++) {
        const ks::Eviction& v = h_ev[i];
        tally(info, v.status);
        if ((uint32_t)v.from < (uint32_t)n && !(seen[v.from >> 5] >> (v.from & 31) & 1u)) {
            seen[v.from >> 5] |= 1u << (v.from & 31);
            busy++;
        }
    }
    info[5] = n_drain - busy;
    if (n_ev) std::memcpy(out, h_ev.data(), sizeof(ks_eviction) * n_ev);
    if (info_out) std::copy(info, info + KS_DRAIN_INFO, info_out);
    return KS_OK;
}

// ---- removal scan (ks_removable.hip) -------------------------------------------------------------
// ks_drain_at's question for each of m candidate nodes on its own.  One gather with the candidates as
// the node set; the host groups the rows by candidate (a stable counting sort on the position in
// nodes[]: FIFO within a candidate) and routes each candidate (ks::removable_route): no pod, the
// batched resolver (at most kRemovableMaxPods pods), or ks_drain_at itself.  The batched candidates
// are walked in segments of at most KS_PLACE_MAX_SHAPES distinct shapes that close at candidate
// boundaries (ks::removable_segment); every segment's scan, merge and resolver are queued back to
// back on the base state and the stream is synchronised once.  The single-drain candidates follow:
// they use the same scratch.
static_assert(KS_REMOVABLE_INFO == 6 && sizeof(ks_removal) == sizeof(ks::Removal) && SAME_FIELD(ks_removal, Removal, node) &&
              SAME_FIELD(ks_removal, Removal, evicted) && SAME_FIELD(ks_removal, Removal, ok) &&
              SAME_FIELD(ks_removal, Removal, over_capacity) && SAME_FIELD(ks_removal, Removal, not_found) &&
              SAME_FIELD(ks_removal, Removal, removable) && SAME_FIELD(ks_removal, Removal, first_row),
              "ks_removable_at constants and record");

ks_status ks_removable_at(ks_engine* e, int64_t t, int32_t m, const int32_t* nodes, ks_removal* out, ks_eviction* rows_out,
                          int64_t cap, int64_t* n_rows, int64_t* info_out) {
    if (!e || !nodes || !out || !n_rows || cap < 0 || (cap > 0 && !rows_out)) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    // ---- one gather for every candidate (cap counts when rows are asked for) ----
    std::vector<uint32_t> h_set;
    DrainCount gc;
    if (ks_status r = gather_open(e, "removable", t, m, nodes, rows_out ? cap : KS_DRAIN_MAX_PODS, &h_set, &gc, n_rows); r != KS_OK)
        return r;
    int64_t info[KS_REMOVABLE_INFO] = {0, 0, 0, 0, 0, 0};
    if (n == 0) {
        if (info_out) std::copy(info, info + KS_REMOVABLE_INFO, info_out);
        return KS_OK;
    }
    const int64_t n_ev = gc.n_ev;
    std::vector<ks::Removal> h_out(m);
    std::vector<ks::Eviction> h_rows(n_ev);
    std::vector<int32_t> slow;  // positions in nodes[] of the candidates ks_drain_at answers
    for (int32_t j = 0; j < m; j++) h_out[j] = ks::Removal{nodes[j], 0, 0, 0, 0, 1, 0};
    if (n_ev) {
        ks::DrainBufs d = gc.g.d;
        RemovableScratch s;
        CARVE_SCRATCH(e, s = carve_removable(qs, np, nblk, n_ev, m, &d));
        ks::PlaceBufs b = s.b;
        b.cnt = gc.g.cnt;
        if (ks_status r = rebuild_state(e, gc.nb, gc.q_hi, t, kDeviceUnits, 1, np, (unsigned long long*)b.state); r != KS_OK)
            return r;
        std::vector<ks::PodRec> fifo;
        std::vector<int32_t> from;
        if (ks_status r = drain_rows(e, t, gc, d, &fifo, &from); r != KS_OK) return r;
        // ---- group by candidate: rows in the caller's order, FIFO within a candidate ----
        std::vector<int32_t> evicted(m), perm(n_ev);
        std::vector<int64_t> first_row(m);
        std::vector<ks::PodRec> recs(n_ev);
        if (const int64_t i = ks::group_rows(nodes, m, n, from.data(), fifo.data(), n_ev, evicted.data(), first_row.data(),
                                             perm.data(), recs.data());
            i >= 0)
            return fail(e, KS_EDEVICE, "removable: evicted pod %lld runs on node %d, no candidate", (long long)i, (int)from[i]);
        std::vector<ks::RemovalCand> cands;
        std::vector<int32_t> cand_pos;
        for (int32_t j = 0; j < m; j++) {
            h_out[j].evicted = evicted[j];
            h_out[j].first_row = first_row[j];
            const int route = ks::removable_route(h_out[j].evicted);
            if (route == ks::kRemovableBatched) {
                cands.push_back(ks::RemovalCand{h_out[j].first_row, nodes[j], h_out[j].evicted});
                cand_pos.push_back(j);
            } else if (route == ks::kRemovableDrain) {
                slow.push_back(j);
            }
        }
        const int64_t n_cand = (int64_t)cands.size();
        if (n_cand) {
            // ---- the segment walk, then every segment's kernels back to back ----
            struct Seg { int64_t cand0, n_cand; int32_t ns; };
            std::vector<Seg> segs;
            std::vector<ks::PodRec> seg_shapes;
            std::vector<int32_t> so(n_ev, 0);
            for (int64_t start = 0; start < n_cand;) {
                seg_shapes.resize((segs.size() + 1) * KS_PLACE_MAX_SHAPES, ks::PodRec{});
                int32_t ns = 0;
                const int64_t end = ks::removable_segment(recs.data(), cands.data(), n_cand, start,
                                                          seg_shapes.data() + segs.size() * KS_PLACE_MAX_SHAPES, &ns, so.data());
                if (end <= start || ns < 1 || (int64_t)segs.size() >= s.seg_cap)
                    return fail(e, KS_EDEVICE, "removable: empty segment at candidate %lld", (long long)start);
                segs.push_back(Seg{start, end - start, ns});
                start = end;
            }
            HIPCHK(e, hipMemcpyAsync((void*)s.r.seg_shapes, seg_shapes.data(), sizeof(ks::PodRec) * seg_shapes.size(),
                                     hipMemcpyHostToDevice, e->st));
            HIPCHK(e, hipMemcpyAsync((void*)s.r.shape_of, so.data(), sizeof(int32_t) * n_ev, hipMemcpyHostToDevice, e->st));
            HIPCHK(e, hipMemcpyAsync((void*)s.r.perm, perm.data(), sizeof(int32_t) * n_ev, hipMemcpyHostToDevice, e->st));
            HIPCHK(e, hipMemcpyAsync((void*)s.r.cands, cands.data(), sizeof(ks::RemovalCand) * n_cand, hipMemcpyHostToDevice, e->st));
            for (size_t g = 0; g < segs.size(); g++) {
                const ks::PlaceCfg pc{e->dc, kDeviceUnits, (int32_t)n, 0, segs[g].ns, (int32_t)nblk};
                b.shapes = s.r.seg_shapes + g * KS_PLACE_MAX_SHAPES;
                HIPCHK(e, ks::launch_place_lists(e->s, pc, b, all_shapes(segs[g].ns), e->st));
                HIPCHK(e, ks::launch_removable_resolve(e->s, pc, b, s.r, b.shapes, segs[g].cand0, segs[g].n_cand, e->st));
            }
            std::vector<ks::Removal> got(n_cand);
            HIPCHK(e, hipMemcpyAsync(got.data(), s.r.out, sizeof(ks::Removal) * n_cand, hipMemcpyDeviceToHost, e->st));
            if (rows_out)
                HIPCHK(e, hipMemcpyAsync(h_rows.data(), s.r.rows, sizeof(ks::Eviction) * n_ev, hipMemcpyDeviceToHost, e->st));
            HIPCHK(e, hipStreamSynchronize(e->st));
            for (int64_t a = 0; a < n_cand; a++) {
                const ks::Removal& v = got[a];
                ks::Removal& o = h_out[cand_pos[a]];
                if (v.node != o.node || v.evicted != o.evicted || v.first_row != o.first_row || v.removable < 0 ||
                    v.ok + v.over_capacity + v.not_found != v.evicted)
                    return fail(e, KS_EDEVICE, "removable: candidate node %d was not decided", (int)o.node);
                o = v;
            }
            info[0] = (int64_t)segs.size();
            info[1] = n_cand;
        }
    }
    // ---- the candidates with more pods than one set of lists decides: ks_drain_at, one by one ----
    std::vector<ks_eviction> one;
    for (int32_t j : slow) {
        ks::Removal& o = h_out[j];
        one.resize(o.evicted);
        int64_t k = 0, dinfo[KS_DRAIN_INFO];
        if (ks_status r = ks_drain_at(e, t, 1, &o.node, one.data(), o.evicted, &k, nullptr, dinfo); r != KS_OK) return r;
        if (k != o.evicted) return fail(e, KS_EDEVICE, "removable: node %d evicts %lld pods, not %d", (int)o.node, (long long)k, (int)o.evicted);
        o.ok = (int32_t)dinfo[1]; o.over_capacity = (int32_t)dinfo[2]; o.not_found = (int32_t)dinfo[3];
        o.removable = o.ok == o.evicted;
        std::memcpy(h_rows.data() + o.first_row, one.data(), sizeof(ks_eviction) * k);
    }
    info[2] = (int64_t)slow.size();
    for (int32_t j = 0; j < m; j++) {
        info[3] += h_out[j].evicted == 0;
        info[4] += h_out[j].removable;
    }
    info[5] = n_ev;
    std::memcpy(out, h_out.data(), sizeof(ks_removal) * m);
    if (rows_out && n_ev) std::memcpy(rows_out, h_rows.data(), sizeof(ks_eviction) * n_ev);
    if (info_out) std::copy(info, info + KS_REMOVABLE_INFO, info_out);
    return KS_OK;
}

// ---- consolidation preview (ks_consolidate.hip) --------------------------------------------------
// The removal scan's candidates as a chain.  One gather with the candidates as the node set, rows
// grouped by candidate as in ks_removable_at; then the candidates in order: a round (scan + merge with
// the removed nodes cordoned, then the resolver's transactions: ks::launch_consolidate_round) takes
// candidates up to KS_PLACE_MAX_SHAPES distinct shapes and KS_PLACE_MAX_PODS pods
// (ks::consolidate_segment) and reports where it ended in 16 bytes; a candidate with more pods than
// one set of lists decides (ks::consolidate_route) heads no round: the host asks `received` whether
// it is a destination and otherwise runs ks_drain_at's rounds for it on a copy of the state, which is
// adopted iff every pod was bound Ok.  Answers, placements and pod indices are read back once, at
// the end, and the rows are packed in the caller's order.
static_assert(KS_CONSOLIDATE_INFO == 6 && sizeof(ks_consolidation) == sizeof(ks::Consolidation) &&
              SAME_FIELD(ks_consolidation, Consolidation, node) && SAME_FIELD(ks_consolidation, Consolidation, evicted) &&
              SAME_FIELD(ks_consolidation, Consolidation, outcome) && SAME_FIELD(ks_consolidation, Consolidation, rows) &&
              SAME_FIELD(ks_consolidation, Consolidation, block_status) &&
              SAME_FIELD(ks_consolidation, Consolidation, first_row) &&
              KS_CONSOLIDATE_BLOCKED == ks::kConsBlocked && KS_CONSOLIDATE_REMOVED == ks::kConsRemoved &&
              KS_CONSOLIDATE_DESTINATION == ks::kConsDestination,
              "ks_consolidate_at constants and record");

ks_status ks_consolidate_at(ks_engine* e, int64_t t, int32_t m, const int32_t* nodes, ks_consolidation* out,
                            ks_eviction* rows_out, int64_t cap, int64_t* n_evicted, int64_t* n_rows, int64_t* after_out,
                            int64_t* info_out) {
    if (!e || !nodes || !out || !n_evicted || !n_rows || cap < 0 || (cap > 0 && !rows_out)) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    // ---- one gather for every candidate (cap counts when rows are asked for) ----
    std::vector<uint32_t> h_set;
    DrainCount gc;
    if (ks_status r = gather_open(e, "consolidate", t, m, nodes, rows_out ? cap : KS_DRAIN_MAX_PODS, &h_set, &gc, n_evicted);
        r != KS_OK)
        return r;
    const int64_t CW = (int64_t)h_set.size(), n_ev = gc.n_ev;
    int64_t info[KS_CONSOLIDATE_INFO] = {0, 0, 0, 0, 0, 0};
    if (n == 0) {
        *n_rows = 0;
        if (info_out) std::copy(info, info + KS_CONSOLIDATE_INFO, info_out);
        return KS_OK;
    }
    ks::DrainBufs d = gc.g.d;
    ConsolidateScratch s;
    CARVE_SCRATCH(e, s = carve_consolidate(qs, n, np, nblk, n_ev, m, CW, &d));
    ks::PlaceBufs b = s.b;
    b.cnt = gc.g.cnt;
    if (ks_status r = rebuild_state(e, gc.nb, gc.q_hi, t, kDeviceUnits, 1, np, (unsigned long long*)b.state); r != KS_OK)
        return r;
    std::vector<ks::PodRec> fifo;
    std::vector<int32_t> from;
    if (n_ev)
        if (ks_status r = drain_rows(e, t, gc, d, &fifo, &from); r != KS_OK) return r;
    // ---- group by candidate: rows in the caller's order, FIFO within a candidate ----
    std::vector<ks::Consolidation> h_out(m);
    std::vector<ks::RemovalCand> cands(m);
    std::vector<int32_t> evicted(m), perm(n_ev);
    std::vector<int64_t> first_row(m);
    std::vector<ks::PodRec> recs(n_ev);
    if (const int64_t i = ks::group_rows(nodes, m, n, from.data(), fifo.data(), n_ev, evicted.data(), first_row.data(),
                                         perm.data(), recs.data());
        i >= 0)
        return fail(e, KS_EDEVICE, "consolidate: evicted pod %lld runs on node %d, no candidate", (long long)i, (int)from[i]);
    for (int32_t j = 0; j < m; j++) {
        h_out[j] = ks::Consolidation{nodes[j], evicted[j], -1, 0, 0, 0, first_row[j]};
        cands[j] = ks::RemovalCand{first_row[j], nodes[j], evicted[j]};
    }
    HIPCHK(e, hipMemcpyAsync((void*)s.cands, cands.data(), sizeof(ks::RemovalCand) * m, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipMemcpyAsync((void*)s.out, h_out.data(), sizeof(ks::Consolidation) * m, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, hipMemsetAsync(s.cordon, 0, sizeof(uint32_t) * CW, e->st));
    HIPCHK(e, hipMemsetAsync(s.received, 0, sizeof(uint32_t) * CW, e->st));
    // ---- the chain ----
    std::vector<unsigned long long> h_up;
    std::vector<int32_t> so(KS_PLACE_MAX_PODS);
    std::vector<char> by_host(m, 0);  // answered here: the single path, and its destinations
    std::vector<ks::Placement> seg_rows;
    ks::PodRec seg_shapes[KS_PLACE_MAX_SHAPES];
    for (int32_t cur = 0; cur < m;) {
        const ks::RemovalCand& cd = cands[cur];
        if (ks::consolidate_route(cd.count) == ks::kConsSingle) {
            ks::Consolidation& o = h_out[cur];
            by_host[cur] = 1;
            uint32_t word = 0;
            HIPCHK(e, hipMemcpyAsync(&word, s.received + (cd.node >> 5), sizeof(word), hipMemcpyDeviceToHost, e->st));
            HIPCHK(e, hipStreamSynchronize(e->st));
            cur++;
            if (word >> (cd.node & 31) & 1u) {
                o.outcome = KS_CONSOLIDATE_DESTINATION;
                continue;
            }
            // the single path: the chain's state and cordon copied, c taken out, ks_drain_at's rounds
            HIPCHK(e, hipMemcpyAsync(s.state2, b.state, sizeof(int64_t) * 4 * np, hipMemcpyDeviceToDevice, e->st));
            HIPCHK(e, hipMemcpyAsync(s.cordon2, s.cordon, sizeof(uint32_t) * CW, hipMemcpyDeviceToDevice, e->st));
            HIPCHK(e, ks::launch_consolidate_take(s.cordon2, s.state2, np, (int32_t)n, cd.node, e->st));
            ks::PlaceBufs x = b;
            x.state = s.state2;
            o.outcome = KS_CONSOLIDATE_REMOVED;
            o.rows = cd.count;
            ks::Placement* placed = s.b.out + cd.first;
            // a segment's rows are read back at once: the attempt ends at the first pod not bound Ok
            const SegmentHook until_blocked = [&](int64_t start, int32_t k, bool* go_on) -> ks_status {
                seg_rows.resize(k);
                HIPCHK(e, hipMemcpyAsync(seg_rows.data(), placed + start, sizeof(ks::Placement) * k, hipMemcpyDeviceToHost, e->st));
                HIPCHK(e, hipStreamSynchronize(e->st));
                for (int32_t i = 0; i < k && *go_on; i++)
                    if (seg_rows[i].status != KS_POD_OK) {  // the copy is dropped
                        o.outcome = KS_CONSOLIDATE_BLOCKED;
                        o.rows = (int32_t)(start + i + 1);
                        o.block_status = seg_rows[i].status;
                        *go_on = false;
                    }
                return KS_OK;
            };
            if (ks_status r = drain_rounds(e, x, placed, recs.data() + cd.first, cd.count, s.cordon2, "consolidate", cd.first,
                                           &info[0], nullptr, until_blocked);
                r != KS_OK)
                return r;
            if (o.outcome == KS_CONSOLIDATE_REMOVED) {  // adopted: state, cordon, and the destinations
                HIPCHK(e, hipMemcpyAsync(b.state, s.state2, sizeof(int64_t) * 4 * np, hipMemcpyDeviceToDevice, e->st));
                HIPCHK(e, hipMemcpyAsync(s.cordon, s.cordon2, sizeof(uint32_t) * CW, hipMemcpyDeviceToDevice, e->st));
                HIPCHK(e, ks::launch_consolidate_mark(s.b.out + cd.first, cd.count, (int32_t)n, s.received, e->st));
            }
            info[4]++;
            continue;
        }
        int32_t ns = 0, k = 0;
        const int64_t end = ks::consolidate_segment(recs.data(), cands.data(), m, cur, seg_shapes, &ns, so.data(), &k);
        if (end <= cur) return fail(e, KS_EDEVICE, "consolidate: empty round at candidate %d", (int)cur);
        if (k)
            if (ks_status r = upload_shapes(e, b, h_up, seg_shapes, ns, so.data(), k); r != KS_OK) return r;
        b.out = s.b.out + cd.first;
        const ks::PlaceCfg pc{e->dc, kDeviceUnits, (int32_t)n, k, ns, (int32_t)nblk};
        const ks::ConsRound cr{s.cands, cur, (int32_t)end, cd.first, s.cordon, s.received, s.out};
        HIPCHK(e, ks::launch_consolidate_round(e->s, pc, b, cr, e->st));
        int32_t next = -1;
        if (ks_status r = round_end(e, b, cur, (int32_t)end, &next); r != KS_OK) return r;
        if (next < 0) return fail(e, KS_EDEVICE, "consolidate: the round from candidate %d decided none", (int)cur);
        cur = next;
        info[0]++;
    }
    // ---- one read-back: the answers, every row's placement and pod ----
    std::vector<ks::Consolidation> got(m);
    std::vector<ks::Placement> placed(n_ev);
    std::vector<long long> ev_pod(n_ev);
    HIPCHK(e, hipMemcpyAsync(got.data(), s.out, sizeof(ks::Consolidation) * m, hipMemcpyDeviceToHost, e->st));
    if (n_ev) {
        HIPCHK(e, hipMemcpyAsync(placed.data(), s.b.out, sizeof(ks::Placement) * n_ev, hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipMemcpyAsync(ev_pod.data(), d.ev_pod, sizeof(long long) * n_ev, hipMemcpyDeviceToHost, e->st));
    }
    if (ks_status r = finish_after(e, b, milli_scale(e), s.after, after_out); r != KS_OK) return r;
    int64_t row = 0;
    for (int32_t j = 0; j < m; j++) {
        ks::Consolidation& o = h_out[j];
        if (!by_host[j]) {
            const ks::Consolidation& v = got[j];
            const bool sane = v.outcome == KS_CONSOLIDATE_REMOVED ? v.rows == v.evicted && v.block_status == 0
                              : v.outcome == KS_CONSOLIDATE_DESTINATION ? v.rows == 0 && v.block_status == 0
                              : v.outcome == KS_CONSOLIDATE_BLOCKED
                                  ? v.rows >= 1 && v.rows <= v.evicted &&
                                        (v.block_status == KS_POD_OVER_CAPACITY || v.block_status == KS_PLACE_NOT_FOUND)
                                  : false;
            if (v.node != o.node || v.evicted != o.evicted || v.first_row != o.first_row || !sane)
                return fail(e, KS_EDEVICE, "consolidate: candidate node %d was not decided", (int)o.node);
            o.outcome = v.outcome;
            o.rows = v.rows;
            o.block_status = v.block_status;
        }
        const int64_t src = o.first_row;  // (its rows among all evicted pods')
        o.first_row = row;
        if (rows_out)
            for (int32_t i = 0; i < o.rows; i++) {
                const ks::Placement& p = placed[src + i];
                rows_out[row + i] = ks_eviction{ev_pod[perm[src + i]], o.node, p.node, p.status, 0, p.score, p.candidates};
            }
        row += o.rows;
        info[o.outcome == KS_CONSOLIDATE_REMOVED ? 1 : o.outcome == KS_CONSOLIDATE_BLOCKED ? 2 : 3]++;
        if (o.outcome == KS_CONSOLIDATE_REMOVED) info[5] += o.rows;
    }
    *n_rows = row;
    std::memcpy(out, h_out.data(), sizeof(ks_consolidation) * m);
    if (info_out) std::copy(info, info + KS_CONSOLIDATE_INFO, info_out);
    return KS_OK;
}

// ---- gang admission preview (ks_gang.hip) --------------------------------------------------------
// ks_place_at's pods in groups, each a transaction.  The gangs in order: a round (scan + merge, then
// the resolver's transactions: ks::launch_gang_round) takes gangs up to KS_PLACE_MAX_SHAPES distinct
// shapes and KS_PLACE_MAX_PODS pods (ks::gang_segment; the caller's shapes are numbered again per
// round) and reports where it ended in 16 bytes; a gang with more pods than one set of lists decides
// (ks::gang_route) heads no round: the host runs ks_drain_at's segmented rounds for it on a copy of
// the state, applies the early end to the finished rows and adopts the copy iff the gang is
// admitted.  Answers and placements are read back once, at the end.
static_assert(KS_GANG_MAX_GANGS == ks::kGangMaxGangs && KS_GANG_MAX_PODS == ks::kDrainMaxPods &&
              KS_GANG_MAX_SHAPES == ks::kGangMaxShapes && KS_GANG_NOT_TRIED == ks::kGangNotTried && KS_GANG_INFO == 6 &&
              KS_GANG_BLOCKED == ks::kGangBlocked && KS_GANG_ADMITTED == ks::kGangAdmitted &&
              KS_GANG_SKIPPED == ks::kGangSkipped && sizeof(ks_gang) == sizeof(ks::Gang) && SAME_FIELD(ks_gang, Gang, first) &&
              SAME_FIELD(ks_gang, Gang, size) && SAME_FIELD(ks_gang, Gang, outcome) && SAME_FIELD(ks_gang, Gang, tried) &&
              SAME_FIELD(ks_gang, Gang, ok) && SAME_FIELD(ks_gang, Gang, over_capacity) &&
              SAME_FIELD(ks_gang, Gang, not_found) && SAME_FIELD(ks_gang, Gang, block_status),
              "ks_gang_at constants and record");

// A gang's answer from the rows of its attempt, read in order: *go_on turns false at the pod that
// blocks it (more than size - min_ok pods not bound Ok), which ends the attempt.
static void gang_tally(ks::Gang& o, int32_t min_ok, const ks::Placement* rows, int32_t count, bool* go_on) {
    for (int32_t i = 0; i < count && *go_on; i++) {
        const int32_t st = rows[i].status;
        (st == KS_POD_OK ? o.ok : st == KS_POD_OVER_CAPACITY ? o.over_capacity : o.not_found)++;
        o.tried++;
        if (o.over_capacity + o.not_found > o.size - min_ok) {
            o.outcome = KS_GANG_BLOCKED;
            o.block_status = st;
            *go_on = false;
        }
    }
}

ks_status ks_gang_at(ks_engine* e, int64_t t, int32_t n_shapes, const int64_t* req, const uint8_t* keymask,
                     const uint64_t* tol, const uint64_t* sel, int32_t k, const int32_t* shape_of, int32_t m,
                     const int32_t* first, const int32_t* min_ok, uint32_t flags, ks_gang* out, ks_placement* rows_out,
                     int64_t* after_out, int64_t* info_out) {
    if (!shape_of || !first || !out) return KS_EINVAL;
    if (!e || !req || !keymask || !tol || !sel) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (flags & ~KS_GANG_STRICT) return fail(e, KS_EINVAL, "gang: unknown flag bits %#x", (unsigned)(flags & ~KS_GANG_STRICT));
    if (k < 1 || k > KS_GANG_MAX_PODS) return fail(e, KS_EINVAL, "gang: %d pods outside [1, %d]", (int)k, KS_GANG_MAX_PODS);
    if (m < 1 || m > KS_GANG_MAX_GANGS) return fail(e, KS_EINVAL, "gang: %d gangs outside [1, %d]", (int)m, KS_GANG_MAX_GANGS);
    if (ks_status r = head_shapes(e, n_shapes, req, keymask, tol, sel, "gang", KS_GANG_MAX_SHAPES); r != KS_OK) return r;
    for (int32_t j = 0; j < k; j++)
        if (shape_of[j] < 0 || shape_of[j] >= n_shapes)
            return fail(e, KS_EINVAL, "gang: pod %d has shape %d outside [0, %d)", (int)j, (int)shape_of[j], (int)n_shapes);
    if (first[0] != 0 || first[m] != k) return fail(e, KS_EINVAL, "gang: first[0] = %d, first[m] = %d, not 0 and %d", (int)first[0], (int)first[m], (int)k);
    std::vector<ks::GangIn> gangs(m);
    for (int32_t g = 0; g < m; g++) {
        if (first[g + 1] < first[g]) return fail(e, KS_EINVAL, "gang %d: first decreases", (int)g);
        const int32_t size = first[g + 1] - first[g], mo = min_ok ? min_ok[g] : size;
        if (mo < 0 || mo > size) return fail(e, KS_EINVAL, "gang %d: min_ok %d outside [0, %d]", (int)g, (int)mo, (int)size);
        gangs[g] = ks::GangIn{first[g], size, mo, 0};
    }
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    const bool strict = flags & KS_GANG_STRICT;
    int64_t info[KS_GANG_INFO] = {0, 0, 0, 0, 0, 0};
    std::vector<ks::Gang> h_out(m);
    std::vector<ks::Placement> placed(k, ks::Placement{-1, ks::kPlaceNotFound, -1, 0});
    std::vector<char> by_host(m, 0);  // answered here: the single path (and every gang of a cluster of no node)
    for (int32_t g = 0; g < m; g++) h_out[g] = ks::Gang{gangs[g].first, gangs[g].size, ks::kGangUndecided, 0, 0, 0, 0, 0};
    bool over = false;  // a strict pass met its blocked gang
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    GangScratch s{};
    ks::PlaceBufs b{};
    ks::QScale back = kDeviceUnits;  // the scratch state's units in milli-units
    if (n == 0) {
        // no node: every pod is not found, the gangs follow from that
        for (int32_t g = 0; g < m && !over; g++) {
            ks::Gang& o = h_out[g];
            by_host[g] = 1;
            o.outcome = KS_GANG_ADMITTED;
            bool go_on = true;
            gang_tally(o, gangs[g].min_ok, placed.data() + o.first, o.size, &go_on);
            over = strict && o.outcome == KS_GANG_BLOCKED;
        }
    } else {
        const int64_t q_hi = bound_by(e, t);
        int64_t nb = 0;
        if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
        CARVE_SCRATCH(e, s = carve_gang(qs, qi, n, np, nblk, k, m));
        b = s.b;
        // whole-unit requests: the call runs in device units, as ks_place_at does
        const ks::QScale milli = milli_scale(e);
        const bool whole = ks::place_whole_units(e->h_shapes.data(), n_shapes, milli);
        const ks::QScale sc = call_units(e, whole, milli);
        back = whole ? milli : kDeviceUnits;
        if (ks_status r = rebuild_state(e, nb, q_hi, t, sc, 1, np, (unsigned long long*)b.state); r != KS_OK) return r;
        std::vector<ks::PodRec> recs(k);
        for (int32_t j = 0; j < k; j++) recs[j] = e->h_shapes[shape_of[j]];
        HIPCHK(e, hipMemcpyAsync((void*)s.gangs, gangs.data(), sizeof(ks::GangIn) * m, hipMemcpyHostToDevice, e->st));
        HIPCHK(e, hipMemcpyAsync((void*)s.out, h_out.data(), sizeof(ks::Gang) * m, hipMemcpyHostToDevice, e->st));
        // ---- the chain ----
        std::vector<unsigned long long> h_up;
        std::vector<int32_t> so(KS_PLACE_MAX_PODS);
        std::vector<ks::Placement> seg_rows;
        ks::PodRec seg_shapes[KS_PLACE_MAX_SHAPES];
        for (int32_t cur = 0; cur < m && !over;) {
            const ks::GangIn& gd = gangs[cur];
            if (ks::gang_route(gd.size) == ks::kGangSingle) {
                // the single path: the chain's state copied, ks_drain_at's rounds without a cordon
                ks::Gang& o = h_out[cur];
                by_host[cur] = 1;
                HIPCHK(e, hipMemcpyAsync(s.state2, b.state, sizeof(int64_t) * 4 * np, hipMemcpyDeviceToDevice, e->st));
                ks::PlaceBufs x = b;
                x.state = s.state2;
                o.outcome = KS_GANG_ADMITTED;
                ks::Placement* rows = s.b.out + gd.first;
                // a segment's rows are read back at once: the attempt ends at the pod that blocks the gang
                const SegmentHook until_blocked = [&](int64_t start, int32_t kk, bool* go_on) -> ks_status {
                    seg_rows.resize(kk);
                    HIPCHK(e, hipMemcpyAsync(seg_rows.data(), rows + start, sizeof(ks::Placement) * kk, hipMemcpyDeviceToHost, e->st));
                    HIPCHK(e, hipStreamSynchronize(e->st));
                    gang_tally(o, gd.min_ok, seg_rows.data(), kk, go_on);
                    return KS_OK;
                };
                if (ks_status r = drain_rounds(e, x, rows, recs.data() + gd.first, gd.size, nullptr, "gang", gd.first, &info[0],
                                               nullptr, until_blocked, sc);
                    r != KS_OK)
                    return r;
                if (o.outcome == KS_GANG_ADMITTED)  // adopted
                    HIPCHK(e, hipMemcpyAsync(b.state, s.state2, sizeof(int64_t) * 4 * np, hipMemcpyDeviceToDevice, e->st));
                over = strict && o.outcome == KS_GANG_BLOCKED;
                info[4]++;
                cur++;
                continue;
            }
            int32_t ns = 0, kk = 0;
            const int64_t end = ks::gang_segment(recs.data(), gangs.data(), m, cur, seg_shapes, &ns, so.data(), &kk);
            if (end <= cur) return fail(e, KS_EDEVICE, "gang: empty round at gang %d", (int)cur);
            if (kk)
                if (ks_status r = upload_shapes(e, b, h_up, seg_shapes, ns, so.data(), kk); r != KS_OK) return r;
            b.out = s.b.out + gd.first;
            const ks::PlaceCfg pc{e->dc, sc, (int32_t)n, kk, ns, (int32_t)nblk};
            const ks::GangRound gr{s.gangs, cur, (int32_t)end, m, strict ? 1 : 0, gd.first, s.out};
            HIPCHK(e, ks::launch_gang_round(e->s, pc, b, gr, e->st));
            int32_t rb[4] = {0, 1, 0, 0};
            HIPCHK(e, hipMemcpyAsync(rb, b.rb, sizeof(rb), hipMemcpyDeviceToHost, e->st));  // 16 bytes per round
            HIPCHK(e, hipStreamSynchronize(e->st));
            const bool ended = strict && rb[0] == m;  // (its blocked gang is found in the answers, below)
            if (rb[1] != 0 || rb[0] <= cur || (rb[0] > end && !ended))
                return fail(e, KS_EDEVICE, "gang: the round from gang %d decided none", (int)cur);
            cur = rb[0];
            info[0]++;
        }
        // ---- one read-back: the answers and every pod's placement ----
        std::vector<ks::Gang> got(m);
        HIPCHK(e, hipMemcpyAsync(got.data(), s.out, sizeof(ks::Gang) * m, hipMemcpyDeviceToHost, e->st));
        if (rows_out) HIPCHK(e, hipMemcpyAsync(placed.data(), s.b.out, sizeof(ks::Placement) * k, hipMemcpyDeviceToHost, e->st));
        std::vector<int64_t> h_after(after_out ? 4 * n : 0);
        if (ks_status r = finish_after(e, b, back, s.after, after_out ? h_after.data() : nullptr); r != KS_OK) return r;
        over = false;
        for (int32_t g = 0; g < m; g++) {
            ks::Gang& o = h_out[g];
            if (!by_host[g]) {
                const ks::Gang& v = got[g];
                const int32_t allow = o.size - gangs[g].min_ok, bad = v.over_capacity + v.not_found;
                const bool sane = over ? v.outcome == ks::kGangUndecided
                                  : v.outcome == KS_GANG_ADMITTED
                                      ? v.tried == v.size && v.ok + bad == v.size && bad <= allow && v.block_status == 0
                                  : v.outcome == KS_GANG_BLOCKED
                                      ? v.tried >= 1 && v.tried <= v.size && v.ok + bad == v.tried && bad == allow + 1 &&
                                            (v.block_status == KS_POD_OVER_CAPACITY || v.block_status == KS_PLACE_NOT_FOUND)
                                      : false;
                if (v.first != o.first || v.size != o.size || !sane)
                    return fail(e, KS_EDEVICE, "gang: gang %d was not decided", (int)g);
                o = v;
            } else if (over && o.outcome != ks::kGangUndecided) {
                return fail(e, KS_EDEVICE, "gang: gang %d was tried after the pass ended", (int)g);
            }
            if (!over && o.outcome == ks::kGangUndecided) return fail(e, KS_EDEVICE, "gang: gang %d was not decided", (int)g);
            over = over || (strict && o.outcome == KS_GANG_BLOCKED);
        }
        if (after_out) std::memcpy(after_out, h_after.data(), sizeof(int64_t) * h_after.size());
    }
    for (int32_t g = 0; g < m; g++) {
        ks::Gang& o = h_out[g];
        if (o.outcome == ks::kGangUndecided) o = ks::Gang{o.first, o.size, KS_GANG_SKIPPED, 0, 0, 0, 0, 0};
        info[o.outcome == KS_GANG_ADMITTED ? 1 : o.outcome == KS_GANG_BLOCKED ? 2 : 3]++;
        if (o.outcome == KS_GANG_ADMITTED) info[5] += o.ok;
        if (rows_out)
            for (int32_t i = 0; i < o.size; i++)
                rows_out[o.first + i] = i < o.tried ? ks_placement{placed[o.first + i].node, placed[o.first + i].status,
                                                                   placed[o.first + i].score, placed[o.first + i].candidates}
                                                    : ks_placement{-1, KS_GANG_NOT_TRIED, -1, 0};
    }
    std::memcpy(out, h_out.data(), sizeof(ks_gang) * m);
    if (info_out) std::copy(info, info + KS_GANG_INFO, info_out);
    return KS_OK;
}

// ---- scale-up preview (ks_scaleup.hip) -----------------------------------------------------------
// ks_place_at's question on n_options extended clusters: the engine's cluster plus up to max_nodes
// empty nodes of a template.  One rebuild of the state at t and one scan + merge over the real nodes
// serve every option (ks::launch_place_lists); one workgroup per option decides the pods from those
// lists (ks::launch_scaleup_resolve) and the host reads the summaries back once.  An option the
// resolver stopped at — a snapshot list used up — is answered from pod 0 through the single path:
// its extended cluster is built in the scratch (ks::launch_scaleup_extend, the state rebuilt at the
// new stride) and ks_place_at's own rounds run on it, which is the definition itself.  With no real
// node every option takes the single path.
// Units: the call runs in device units when every masked request and every present template
// capacity is a whole multiple of the engine's unit (ks::scaleup_whole_units), else in milli-units.
static_assert(KS_SCALEUP_MAX_OPTIONS == ks::kScaleMaxOptions && KS_SCALEUP_MAX_NODES == ks::kScaleMaxNodes &&
              KS_SCALEUP_INFO == 4 && sizeof(ks_scale_option) == 56 && sizeof(ks_scale_result) == sizeof(ks::ScaleResult) &&
              offsetof(ks_scale_option, alloc) == 0 && SAME_FIELD(ks_scale_result, ScaleResult, ok) &&
              SAME_FIELD(ks_scale_result, ScaleResult, on_new) && SAME_FIELD(ks_scale_result, ScaleResult, nodes_used) &&
              SAME_FIELD(ks_scale_result, ScaleResult, first_unplaced) && SAME_FIELD(ks_scale_result, ScaleResult, path),
              "ks_scale_up_at constants and records");

// an option's summary from its k rows on a cluster of n real nodes (the single path; the batched
// kernel counts the same on the device)
static ks::ScaleResult scale_summary(const ks::Placement* rows, int32_t k, int64_t n) {
    ks::ScaleResult r{0, 0, 0, 0, 0, -1, ks::kScaleSingle, 0};
    std::vector<int32_t> used;
    for (int32_t i = 0; i < k; i++) {
        const ks::Placement& v = rows[i];
        if (v.status == KS_POD_OK) {
            r.ok++;
            if (v.node >= n) {
                r.on_new++;
                used.push_back(v.node);
            }
            continue;
        }
        (v.status == KS_POD_OVER_CAPACITY ? r.over_capacity : r.not_found)++;
        if (r.first_unplaced < 0) r.first_unplaced = i;
    }
    std::sort(used.begin(), used.end());
    r.nodes_used = (int32_t)(std::unique(used.begin(), used.end()) - used.begin());
    return r;
}

ks_status ks_scale_up_at(ks_engine* e, int64_t t, int32_t n_shapes, const int64_t* req, const uint8_t* keymask,
                         const uint64_t* tol, const uint64_t* sel, int32_t k, const int32_t* shape_of, int32_t n_options,
                         const ks_scale_option* options, ks_scale_result* out, ks_placement* rows_out, int64_t* info_out) {
    if (!e || !req || !keymask || !tol || !sel || !options || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = head_shapes(e, n_shapes, req, keymask, tol, sel, "scale_up"); r != KS_OK) return r;
    std::vector<int32_t> so;
    if (ks_status r = pod_shapes(e, "scale_up", k, shape_of, n_shapes, &so); r != KS_OK) return r;
    if (n_options < 1 || n_options > KS_SCALEUP_MAX_OPTIONS)
        return fail(e, KS_EINVAL, "scale_up: %d options outside [1, %d]", (int)n_options, KS_SCALEUP_MAX_OPTIONS);
    int64_t max_ext = 0;
    for (int32_t g = 0; g < n_options; g++) {
        const ks_scale_option& o = options[g];
        if (o.max_nodes < 0 || o.max_nodes > KS_SCALEUP_MAX_NODES)
            return fail(e, KS_EINVAL, "scale_up option %d: max_nodes %d outside [0, %d]", (int)g, (int)o.max_nodes, KS_SCALEUP_MAX_NODES);
        for (int c = 0; c < 3; c++)
            if (o.alloc[c] < -1 || o.alloc[c] >= kMaxValue)
                return fail(e, KS_EINVAL, "scale_up option %d: capacity %d out of range", (int)g, c);
        if (o.alloc[3] < 0 || o.alloc[3] >= kMaxValue) return fail(e, KS_EINVAL, "scale_up option %d: pods capacity out of range", (int)g);
        if (o.pad != 0) return fail(e, KS_EINVAL, "scale_up option %d: pad is %d, not 0", (int)g, (int)o.pad);
        max_ext = std::max<int64_t>(max_ext, o.max_nodes);
    }
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    // the call's units: device units when every request and template capacity is whole, else milli-units
    const ks::QScale milli = milli_scale(e);
    static_assert(sizeof(ks_scale_option) % sizeof(int64_t) == 0, "alloc stride in words");
    const bool whole = ks::scaleup_whole_units(e->h_shapes.data(), n_shapes, options[0].alloc, n_options,
                                               sizeof(ks_scale_option) / sizeof(int64_t), milli);
    const ks::QScale sc = call_units(e, whole, milli);
    std::vector<ks::ScaleOption> h_opts(n_options);
    for (int32_t g = 0; g < n_options; g++)
        h_opts[g] = ks::ScaleOption{ks::scaleup_template(options[g].alloc, options[g].taint, options[g].label,
                                                         whole ? milli : kDeviceUnits),
                                    options[g].max_nodes, 0};
    std::vector<ks::ScaleResult> h_out(n_options);
    std::vector<ks::Placement> h_rows((size_t)n_options * k);
    std::vector<int32_t> single;  // the options the single path answers
    int64_t info[KS_SCALEUP_INFO] = {0, 0, 0, n_shapes};
    const int64_t q_hi = bound_by(e, t);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
    ScaleScratch s;
    CARVE_SCRATCH(e, s = carve_scale_up(qs, qi, n, np, nblk, k, n_options, max_ext));
    std::vector<unsigned long long> h_up;
    if (n > 0) {
        // ---- one state, one set of lists, every option's workgroup, one read-back ----
        if (ks_status r = rebuild_state(e, nb, q_hi, t, sc, 1, np, (unsigned long long*)s.b.state); r != KS_OK) return r;
        if (ks_status r = upload_shapes(e, s.b, h_up, e->h_shapes.data(), n_shapes, so.data(), k); r != KS_OK) return r;
        HIPCHK(e, hipMemcpyAsync((void*)s.sb.opts, h_opts.data(), sizeof(ks::ScaleOption) * n_options, hipMemcpyHostToDevice, e->st));
        const ks::PlaceCfg pc{e->dc, sc, (int32_t)n, k, n_shapes, (int32_t)nblk};
        HIPCHK(e, ks::launch_place_lists(e->s, pc, s.b, all_shapes(n_shapes), e->st));
        HIPCHK(e, ks::launch_scaleup_resolve(e->s, pc, s.b, s.sb, n_options, e->st));
        HIPCHK(e, hipMemcpyAsync(h_out.data(), s.sb.out, sizeof(ks::ScaleResult) * n_options, hipMemcpyDeviceToHost, e->st));
        if (rows_out)
            HIPCHK(e, hipMemcpyAsync(h_rows.data(), s.sb.rows, sizeof(ks::Placement) * h_rows.size(), hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
        for (int32_t g = 0; g < n_options; g++) {
            const ks::ScaleResult& v = h_out[g];
            if (v.path == ks::kScaleStopped) single.push_back(g);
            else if (v.path != ks::kScaleBatched || v.ok + v.over_capacity + v.not_found != k)
                return fail(e, KS_EDEVICE, "scale_up: option %d was not decided", (int)g);
        }
    } else {
        for (int32_t g = 0; g < n_options; g++) single.push_back(g);
    }
    // ---- the single path: ks_place_at's rounds on the option's extended cluster ----
    for (int32_t g : single) {
        ks::Placement* rows = h_rows.data() + (size_t)g * k;
        const int64_t n_ext = n + h_opts[g].max_nodes;
        if (n_ext == 0) {  // no node at all
            for (int32_t j = 0; j < k; j++) rows[j] = ks::Placement{-1, ks::kPlaceNotFound, -1, 0};
            h_out[g] = scale_summary(rows, k, n);
            continue;
        }
        const int64_t np_g = std::max<int64_t>(64, (n_ext + 63) / 64 * 64), nblk_g = (n_ext + 255) / 256;
        if (np_g > s.np_ext || nblk_g > s.nblk_ext) return fail(e, KS_EDEVICE, "scale_up: option %d outgrows the scratch", (int)g);
        HIPCHK(e, ks::launch_scaleup_extend(e->s, (int32_t)n, sc, h_opts[g], np_g, s.ext_node, e->st));
        ks::PlaceBufs x = s.x;
        x.n_pad = np_g;
        // the state at the new stride: rows >= n are written by no bind, so the appended nodes start empty
        if (n > 0) {
            if (ks_status r = rebuild_state(e, nb, q_hi, t, sc, 1, np_g, (unsigned long long*)x.state); r != KS_OK) return r;
        } else {
            HIPCHK(e, hipMemsetAsync(x.state, 0, sizeof(int64_t) * 4 * np_g, e->st));
        }
        if (ks_status r = upload_shapes(e, x, h_up, e->h_shapes.data(), n_shapes, so.data(), k); r != KS_OK) return r;
        const ks::NodeSoA sx = scale_up_nodes(s.ext_node, x.state, np_g);
        // (the extended constants are in the call's units already: scale 1)
        const ks::PlaceCfg pc{e->dc, kDeviceUnits, (int32_t)n_ext, k, n_shapes, (int32_t)nblk_g};
        int64_t rounds = 0;
        if (ks_status r = place_rounds(e, sx, pc, x, so.data(), nullptr, "scale_up: the round from pod", 0, &rounds); r != KS_OK)
            return r;
        HIPCHK(e, hipMemcpyAsync(rows, x.out, sizeof(ks::Placement) * k, hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
        h_out[g] = scale_summary(rows, k, n);
    }
    info[1] = (int64_t)single.size();
    info[0] = n_options - info[1];
    for (int32_t g = 0; g < n_options; g++) info[2] += h_out[g].ok == k;
    std::memcpy(out, h_out.data(), sizeof(ks_scale_result) * n_options);
    if (rows_out) std::memcpy(rows_out, h_rows.data(), sizeof(ks_placement) * h_rows.size());
    if (info_out) std::copy(info, info + KS_SCALEUP_INFO, info_out);
    return KS_OK;
}

}  // extern "C"
