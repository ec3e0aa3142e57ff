// ks_carve.h — the query scratch (ks_engine::d_qs, d_qi) carved into typed ranges; host only.
//
// A layout is written once, as a sequence of Carve::take() calls, and run twice: with a null base
// the cursor only counts and `at` is the size to reserve; with the real base the same calls give
// the pointers.  The reserved size and the ranges therefore cannot disagree.  The layouts of the
// placement, drain, scale-up, consolidation and gang previews and of the removal scan live here too,
// so a stand-alone host program can check them.
#pragma once
#include <cstdint>

#include "ks_query.h"

namespace ks_host {

struct Carve {
    int64_t word;          // bytes per scratch word (8: d_qs, 4: d_qi)
    char* base = nullptr;  // null: the sizing pass
    int64_t at = 0;        // words taken so far
    explicit Carve(int64_t word_bytes, void* base_ = nullptr) : word(word_bytes), base((char*)base_) {}
    // count elements of T from the next multiple of align_words (2 words of d_qs: PodRec's 16 bytes)
    template <typename T>
    T* take(int64_t count, int64_t align_words = 1) {
        at = (at + align_words - 1) / align_words * align_words;
        T* p = base ? (T*)(base + at * word) : nullptr;
        at += (count * (int64_t)sizeof(T) + word - 1) / word;
        return p;
    }
};

// the shape records of one upload (shape_of follows them on a 16-byte boundary)
constexpr int64_t kShapeWords = (int64_t)sizeof(ks::PodRec) / 8 * ks::kPlaceMaxShapes;
static_assert(kShapeWords % 2 == 0, "shape_of follows the shape records on a 16-byte boundary");

// The rounds' buffers in d_qs (ks_query.h PlaceBufs; cnt is the caller's, in d_qi): a round set
// uploads up to so_cap pods' shape_of, the call places n_placed pods in all.  ks_place_at: both k;
// ks_drain_at: a segment's KS_PLACE_MAX_PODS and every evicted pod.
inline ks::PlaceBufs carve_place(Carve& qs, int64_t np, int64_t nblk, int64_t so_cap, int64_t n_placed) {
    constexpr int64_t S = ks::kPlaceMaxShapes, L = ks::kPlaceL;
    ks::PlaceBufs b{};
    b.state = qs.take<int64_t>(4 * np);  // [4][np]: rc rm rg nr at t
    b.n_pad = np;
    b.shapes = qs.take<ks::PodRec>(S, 2);  // one upload: the shape records, then shape_of
    b.shape_of = qs.take<int32_t>(so_cap);
    b.lists = qs.take<uint64_t>(S * nblk * L);
    b.top = qs.take<uint64_t>(S * L);
    b.ccount = qs.take<long long>(S);
    b.rb = qs.take<int32_t>(4);                // read back every round
    b.out = qs.take<ks::Placement>(n_placed);  // (ks_place_at reads rb and out back as one range)
    return b;
}

struct PlaceScratch {
    ks::PlaceBufs b;
    long long* after;  // [n][4]
};
inline PlaceScratch carve_place_at(Carve& qs, Carve& qi, int64_t n, int64_t np, int64_t nblk, int64_t k) {
    PlaceScratch s{};
    s.b = carve_place(qs, np, nblk, k, k);
    s.after = qs.take<long long>(4 * n);
    s.b.cnt = qi.take<int32_t>(ks::kPlaceMaxShapes * nblk);
    return s;
}

// ks_drain_at, before the evicted pods are counted: the gather's int32 scratch (cordon [cw], block
// counts and offsets [nb], the 8-byte total) and the rounds' cnt
struct DrainGather {
    ks::DrainBufs d;
    int32_t* cnt;
};
inline DrainGather carve_drain_gather(Carve& qi, int64_t cw, int64_t nb, int64_t nblk) {
    DrainGather g{};
    g.d.cordon = qi.take<uint32_t>(cw);
    g.d.bcnt = qi.take<int32_t>(nb);
    g.d.boff = qi.take<int32_t>(nb);
    g.d.total = qi.take<long long>(1, 2);
    g.cnt = qi.take<int32_t>(ks::kPlaceMaxShapes * nblk);
    return g;
}

// ... and once n_ev is known: the rounds' buffers, the gathered rows (into d), the packed records
struct DrainScratch {
    ks::PlaceBufs b;  // b.out: every evicted pod's placement, a segment's at its first pod
    ks::Eviction* evict;
    long long* after;  // [n][4]
};
inline DrainScratch carve_drain(Carve& qs, int64_t n, int64_t np, int64_t nblk, int64_t n_ev, ks::DrainBufs* d) {
    DrainScratch s{};
    s.b = carve_place(qs, np, nblk, ks::kPlaceMaxPods, n_ev);
    d->ev_pod = qs.take<long long>(n_ev);
    d->ev_from = qs.take<int32_t>(n_ev);
    d->ev_rec = qs.take<ks::PodRec>(n_ev, 2);
    d->cap = n_ev;
    s.evict = qs.take<ks::Eviction>(n_ev);
    s.after = qs.take<long long>(4 * n);
    return s;
}

// ks_removable_at, once n_ev is known (the gather's int32 scratch is carve_drain_gather's): the
// lists' buffers on the base state (b.shape_of: a row's shape among its segment's, every row; no
// placements: the resolver writes rows), the gathered rows (into d), and the resolver's buffers for
// at most min(m, n_ev) batched candidates in at most removable_seg_cap(n_ev) segments
struct RemovableScratch {
    ks::PlaceBufs b;
    ks::RemovableBufs r;
    int64_t cand_cap, seg_cap;
};
// A segment closes only before a candidate that would bring its 65th shape; that candidate has at
// most kRemovableMaxPods shapes, so a closed segment holds more than kPlaceMaxShapes -
// kRemovableMaxPods shapes, each on a row of its own.
constexpr int64_t removable_seg_cap(int64_t n_ev) {
    return n_ev / (ks::kPlaceMaxShapes - ks::kRemovableMaxPods + 1) + 1;
}
inline RemovableScratch carve_removable(Carve& qs, int64_t np, int64_t nblk, int64_t n_ev, int64_t m, ks::DrainBufs* d) {
    RemovableScratch s{};
    s.cand_cap = m < n_ev ? m : n_ev;
    s.seg_cap = removable_seg_cap(n_ev);
    s.b = carve_place(qs, np, nblk, n_ev, 0);
    d->ev_pod = qs.take<long long>(n_ev);
    d->ev_from = qs.take<int32_t>(n_ev);
    d->ev_rec = qs.take<ks::PodRec>(n_ev, 2);
    d->cap = n_ev;
    s.r.seg_shapes = qs.take<ks::PodRec>(s.seg_cap * ks::kPlaceMaxShapes, 2);
    s.r.shape_of = s.b.shape_of;
    s.r.ev_pod = d->ev_pod;
    s.r.perm = qs.take<int32_t>(n_ev);
    s.r.cands = qs.take<ks::RemovalCand>(s.cand_cap);
    s.r.rows = qs.take<ks::Eviction>(n_ev);
    s.r.out = qs.take<ks::Removal>(s.cand_cap);
    return s;
}

// ks_consolidate_at, once n_ev is known (the gather's int32 scratch is carve_drain_gather's): the
// rounds' buffers on the chain's state (b.shape_of: a round's KS_PLACE_MAX_PODS; b.out: every row's
// placement at its caller-ordered row, a round's at its first row), the gathered rows (into d), the
// single path's second state copy and its cordon, the bitmaps of the removed nodes (cordon) and of
// the destinations (received) [cw words each], the candidate table and the answers [m]
struct ConsolidateScratch {
    ks::PlaceBufs b;
    int64_t* state2;  // [4][np]
    uint32_t *cordon, *received, *cordon2;
    ks::RemovalCand* cands;
    ks::Consolidation* out;
    long long* after;  // [n][4]
};
inline ConsolidateScratch carve_consolidate(Carve& qs, int64_t n, int64_t np, int64_t nblk, int64_t n_ev, int64_t m,
                                            int64_t cw, ks::DrainBufs* d) {
    ConsolidateScratch s{};
    s.b = carve_place(qs, np, nblk, ks::kPlaceMaxPods, n_ev);
    d->ev_pod = qs.take<long long>(n_ev);
    d->ev_from = qs.take<int32_t>(n_ev);
    d->ev_rec = qs.take<ks::PodRec>(n_ev, 2);
    d->cap = n_ev;
    s.state2 = qs.take<int64_t>(4 * np);
    s.cordon = qs.take<uint32_t>(cw);
    s.received = qs.take<uint32_t>(cw);
    s.cordon2 = qs.take<uint32_t>(cw);
    s.cands = qs.take<ks::RemovalCand>(m, 2);
    s.out = qs.take<ks::Consolidation>(m);
    s.after = qs.take<long long>(4 * n);
    return s;
}

// ks_gang_at: the rounds' buffers on the chain's state (b.shape_of: a round's KS_PLACE_MAX_PODS;
// b.out: every pod's placement at its own index, a round's at its first pod), the single path's
// second state copy, the gang table and the answers [m]
struct GangScratch {
    ks::PlaceBufs b;
    int64_t* state2;  // [4][np]
    ks::GangIn* gangs;
    ks::Gang* out;
    long long* after;  // [n][4]
};
inline GangScratch carve_gang(Carve& qs, Carve& qi, int64_t n, int64_t np, int64_t nblk, int64_t k, int64_t m) {
    GangScratch s{};
    s.b = carve_place(qs, np, nblk, ks::kPlaceMaxPods, k);
    s.state2 = qs.take<int64_t>(4 * np);
    s.gangs = qs.take<ks::GangIn>(m, 2);
    s.out = qs.take<ks::Gang>(m);
    s.after = qs.take<long long>(4 * n);
    s.b.cnt = qi.take<int32_t>(ks::kPlaceMaxShapes * nblk);
    return s;
}

// ks_scale_up_at: the shared lists' buffers on the base state (b: n real nodes, k pods' shape_of, no
// placements of its own), the batched resolver's options, rows [n_options][k] and summaries, and
// the single path's extended cluster for the largest option: n + max_ext rows padded to 64 (np_ext),
// its six constant fields (ext_node, field f at ext_node + f * np_ext), and its own round buffers x
// (state [4][np_ext], lists over nblk_ext blocks, out [k])
struct ScaleScratch {
    ks::PlaceBufs b;
    ks::ScaleBufs sb;
    int64_t n_ext, np_ext, nblk_ext;
    int64_t* ext_node;
    ks::PlaceBufs x;
};
inline ScaleScratch carve_scale_up(Carve& qs, Carve& qi, int64_t n, int64_t np, int64_t nblk, int64_t k,
                                   int64_t n_options, int64_t max_ext) {
    ScaleScratch s{};
    s.b = carve_place(qs, np, nblk, k, 0);
    s.b.cnt = qi.take<int32_t>(ks::kPlaceMaxShapes * nblk);
    s.sb.opts = qs.take<ks::ScaleOption>(n_options);
    s.sb.rows = qs.take<ks::Placement>(n_options * k);
    s.sb.out = qs.take<ks::ScaleResult>(n_options);
    s.n_ext = n + max_ext;
    s.np_ext = (s.n_ext + 63) / 64 * 64;
    if (s.np_ext < 64) s.np_ext = 64;
    s.nblk_ext = (s.n_ext + 255) / 256;
    s.ext_node = qs.take<int64_t>(6 * s.np_ext);
    s.x = carve_place(qs, s.np_ext, s.nblk_ext, k, k);
    s.x.cnt = qi.take<int32_t>(ks::kPlaceMaxShapes * s.nblk_ext);
    return s;
}
// an option's extended cluster as a node table at its own stride np_g <= np_ext: the constants of
// ext_node, the state [4][np_g]
inline ks::NodeSoA scale_up_nodes(int64_t* ext_node, int64_t* state, int64_t np_g) {
    ks::NodeSoA sx{};
    sx.ac = ext_node; sx.am = ext_node + np_g; sx.ag = ext_node + 2 * np_g; sx.ap = ext_node + 3 * np_g;
    sx.taint = (uint64_t*)(ext_node + 4 * np_g); sx.label = (uint64_t*)(ext_node + 5 * np_g);
    sx.rc = state; sx.rm = state + np_g; sx.rg = state + 2 * np_g; sx.nr = state + 3 * np_g;
    return sx;
}

// ks_node_peaks / ks_headroom_series: per node the offset, cursor and count of its pods in list[cap]
struct NodeLists {
    int32_t *off, *cur, *cnt, *list;
};
inline NodeLists carve_node_lists(Carve& qi, int64_t n, int64_t cap) {
    NodeLists l{};
    l.off = qi.take<int32_t>(n + 1);
    l.cur = qi.take<int32_t>(n);
    l.cnt = qi.take<int32_t>(n);
    l.list = qi.take<int32_t>(cap);
    return l;
}

}  // namespace ks_host
