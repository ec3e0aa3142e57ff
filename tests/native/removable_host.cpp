// Host build of the removal scan's host-side pieces (ks_query.h: removable_route,
// removable_entries_on, removable_segment, group_rows and the placement functions; ks_carve.h:
// carve_removable), for CPU tests only.
//   ks_host_removable          a serial restatement of removable_resolve_kernel (ks_removable.hip) for
//                              one candidate, on place_serial.h's list builder and pod loop: the lists
//                              and counts of the base state with no cordon, the candidate's own entries
//                              flagged from the start, its counts corrected, its pods decided from that
//                              one set of lists, a veto on the candidate itself;
//   ks_host_removable_brute    the plain sequential argmax over the nodes other than the candidate;
//   ks_host_removable_segments ks_removable_at's candidate-aligned segment walk;
//   ks_host_group_rows         the gather's rows grouped by candidate;
//   ks_host_removable_route    the split between the batched resolver and the single-drain path;
//   ks_host_removable_carve    carve_removable run twice, as ks_removable_at does.
// Not part of the product.
#include <cstdio>
#include <cstring>

#include "../../kubernetes-simulator_amd/csrc/ks_carve.h"
#include "place_serial.h"

using namespace place_serial;

#define CASE_ARGS CLUSTER_ARGS, int32_t k, const int32_t *shape_of, int32_t cand
#define CASE_PASS CLUSTER_PASS

// scheduleOne as written, over the nodes other than the candidate (whose own state is never read)
extern "C" int ks_host_removable_brute(CASE_ARGS, ks::Placement* out, int64_t* info) {
    Cluster s = make_cluster(CASE_PASS);
    for (int32_t i = 0; i < k; i++) {
        const ks::PodRec& p = s.shapes[shape_of[i]];
        uint64_t best = 0;
        int64_t cnd = 0;
        for (int32_t nd = 0; nd < n; nd++) {
            if (nd == cand) continue;
            const uint64_t key = ks::place_key(s.c, p, s.node[nd], (uint32_t)nd);
            cnd += key != 0;
            best = key > best ? key : best;
        }
        if (!best) {
            out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cnd};
            continue;
        }
        const uint32_t X = ks::place_key_node(best);
        const int32_t st = ks::place_bind(p, s.node[X]);
        out[i] = ks::Placement{(int32_t)X, st, (int64_t)(best >> 32) - 1, cnd};
    }
    tally(out, k, info);
    return 0;
}

// The resolver of one candidate.  `mode` takes out one of the two corrections, to show that the tests
// see them: 1: the own-node flags are not pre-set; 2: the counts are not corrected.  Returns 0, -1 when
// a pod met kPlaceStop (more pods than one set of lists decides), -2 when the candidate itself won.
// stats[0]: pods decided from a changed node, stats[1]: the most flagged entries of a list at the end,
// stats[2]: lists the candidate's own node is in.
extern "C" int ks_host_removable(CASE_ARGS, int32_t mode, ks::Placement* out, int64_t* info, int64_t* stats) {
    const Cluster s = make_cluster(CASE_PASS);
    // launch_place_lists: every shape, the base state, no cordon; then the candidate's two corrections
    Lists l = build_lists(s, nullptr, node_key(s));
    stats[0] = stats[1] = stats[2] = 0;
    for (int32_t j = 0; j < n_shapes; j++) {
        const uint32_t own = ks::removable_entries_on<L>(&l.top[(size_t)j * L], (uint32_t)cand);
        stats[2] += own != 0;
        if (mode != 1) l.flag[j] = own;
        if (mode != 2) l.cc[j] -= ks::place_is_cand(s.c, s.shapes[j], s.node[cand]);
    }
    struct Self : Hooks {
        int32_t cand, mode;
        int veto(uint32_t X) const { return (int32_t)X == cand && mode == 0 ? -2 : 0; }
    } h{{}, cand, mode};
    std::vector<Chg> chg;
    const Run r = decide_pods(s, l, shape_of, 0, k, chg, h, out);
    stats[0] = r.from_changed;
    if (r.stopped) return -1;
    if (r.veto) return r.veto;
    for (int32_t j = 0; j < n_shapes; j++) stats[1] = std::max<int64_t>(stats[1], __builtin_popcount(l.flag[j]));
    tally(out, k, info);
    return 0;
}

// ks_removable_at's segment walk over n_cand batched candidates, candidate a's pods the next cnt[a]
// rows, row i's shape the record of id ids[i]: seg_end[s] (in candidates, exclusive) and seg_shapes[s]
// per segment, shape_of[row], the shape tables in shapes_out[segment * 64 + shape].  Returns the number
// of segments, -1 when more than seg_cap or a segment is empty.
extern "C" int64_t ks_host_removable_segments(int64_t n_cand, const int32_t* cnt, const int64_t* req, const uint32_t* keymask,
                                              const uint64_t* tol, const uint64_t* sel, const uint32_t* flags,
                                              int64_t seg_cap, int64_t* seg_end, int32_t* seg_shapes, int32_t* shape_of,
                                              ks::PodRec* shapes_out) {
    std::vector<ks::RemovalCand> cands(n_cand);
    int64_t rows = 0;
    for (int64_t a = 0; a < n_cand; a++) {
        cands[a] = ks::RemovalCand{rows, (int32_t)a, cnt[a]};
        rows += cnt[a];
    }
    std::vector<ks::PodRec> recs(rows);
    for (int64_t i = 0; i < rows; i++) {
        recs[i] = ks::PodRec{};
        for (int c = 0; c < 3; c++) recs[i].req[c] = req[i * 3 + c];  // unmasked words as given
        recs[i].tol = tol[i]; recs[i].sel = sel[i]; recs[i].keymask = keymask[i]; recs[i].flags = flags[i];
    }
    int64_t ns = 0;
    for (int64_t start = 0; start < n_cand;) {
        if (ns >= seg_cap) return -1;
        int32_t m = 0;
        const int64_t end = ks::removable_segment(recs.data(), cands.data(), n_cand, start,
                                                  shapes_out + ns * ks::kPlaceMaxShapes, &m, shape_of);
        if (end <= start) return -1;
        seg_end[ns] = end;
        seg_shapes[ns] = m;
        ns++;
        start = end;
    }
    return ns;
}

// ks::group_rows as ks_removable_at and ks_consolidate_at call it: gathered row i runs on node from[i]
// and its record carries ids[i] (in req[0]); rec_ids[row] is the id of the record grouped to `row`.
extern "C" int64_t ks_host_group_rows(int32_t m, const int32_t* nodes, int64_t n, int64_t n_ev, const int32_t* from,
                                      const int64_t* ids, int32_t* evicted, int64_t* first_row, int32_t* perm,
                                      int64_t* rec_ids) {
    std::vector<ks::PodRec> fifo(n_ev, ks::PodRec{}), recs(n_ev, ks::PodRec{});
    for (int64_t i = 0; i < n_ev; i++) fifo[i].req[0] = ids[i];
    const int64_t bad = ks::group_rows(nodes, m, n, from, fifo.data(), n_ev, evicted, first_row, perm, recs.data());
    for (int64_t i = 0; i < n_ev; i++) rec_ids[i] = recs[i].req[0];
    return bad;
}

extern "C" int ks_host_removable_route(int64_t pods) { return ks::removable_route(pods); }

extern "C" int ks_host_removable_limits(int32_t* out) {
    out[0] = ks::kPlaceMaxShapes; out[1] = ks::kRemovableMaxPods; out[2] = L; out[3] = (int32_t)sizeof(ks::Removal);
    out[4] = (int32_t)sizeof(ks::RemovalCand); out[5] = (int32_t)ks_host::removable_seg_cap(65536);
    out[6] = ks::kRemovableEmpty; out[7] = ks::kRemovableBatched; out[8] = ks::kRemovableDrain;
    return 0;
}

// carve_removable at edge counts, twice as ks_removable_at runs it: every range inside the reserved
// size, aligned for its element, overlapping no other, and written.  Returns the violated checks.
extern "C" int64_t ks_host_removable_carve() {
    using ks_host::Carve;
    struct Range { const char* name; const void* p; int64_t bytes, align; };
    int64_t bad = 0;
    auto fail = [&](const char* what, const char* name, int64_t a, int64_t b) {
        if (bad++ < 20) std::fprintf(stderr, "carve_removable: %s: %s (%lld, %lld)\n", name, what, (long long)a, (long long)b);
    };
    for (int64_t n : {1, 255, 256, 257, 600})
        for (int64_t n_ev : {1, 3, 33, 34, 35, 1000, 65536})
            for (int64_t m : {(int64_t)1, n}) {
                const int64_t np = (n + 63) / 64 * 64, nblk = (n + 255) / 256;
                ks::DrainBufs d{};
                Carve qs(8);
                ks_host::carve_removable(qs, np, nblk, n_ev, m, &d);
                const int64_t words = qs.at;
                std::vector<long double> mem((words * 8 + 15) / 16 + 1);
                char* base = (char*)mem.data();
                qs = Carve(8, base);
                const ks_host::RemovableScratch s = ks_host::carve_removable(qs, np, nblk, n_ev, m, &d);
                if (qs.at != words) fail("the two passes differ", "d_qs", qs.at, words);
                const int64_t cands = std::min(m, n_ev), segs = n_ev / (64 - (L - 1) + 1) + 1, S = ks::kPlaceMaxShapes;
                if (s.cand_cap != cands || s.seg_cap != segs || d.cap != n_ev || s.b.n_pad != np || s.r.shape_of != s.b.shape_of ||
                    s.r.ev_pod != d.ev_pod)
                    fail("capacities", "removable", s.cand_cap, s.seg_cap);
                const std::vector<Range> rs = {
                    {"state", s.b.state, 32 * np, 8},
                    {"shapes", s.b.shapes, 48 * S, 16},
                    {"shape_of", s.b.shape_of, 4 * n_ev, 4},
                    {"lists", s.b.lists, 8 * S * nblk * L, 8},
                    {"top", s.b.top, 8 * S * L, 8},
                    {"ccount", s.b.ccount, 8 * S, 8},
                    {"rb", s.b.rb, 16, 4},
                    {"ev_pod", d.ev_pod, 8 * n_ev, 8},
                    {"ev_from", d.ev_from, 4 * n_ev, 4},
                    {"ev_rec", d.ev_rec, 48 * n_ev, 16},
                    {"seg_shapes", s.r.seg_shapes, 48 * S * segs, 16},
                    {"perm", s.r.perm, 4 * n_ev, 4},
                    {"cands", s.r.cands, 16 * cands, 8},
                    {"rows", s.r.rows, 40 * n_ev, 8},
                    {"out", s.r.out, 32 * cands, 8}};
                for (const Range& r : rs) {
                    const int64_t off = (const char*)r.p - base;
                    if (off < 0 || off + r.bytes > words * 8) fail("outside the reserved size", r.name, off, r.bytes);
                    else std::memset(base + off, 0x5A, r.bytes);
                    if (off % r.align) fail("misaligned", r.name, off, r.align);
                    for (const Range& q : rs)
                        if (&q != &r && r.bytes && q.bytes && (const char*)q.p < (const char*)r.p + r.bytes &&
                            (const char*)r.p < (const char*)q.p + q.bytes)
                            fail("overlaps", r.name, off, (const char*)q.p - base);
                }
            }
    return bad;
}

#ifdef KS_REMOVABLE_MAIN
int main() {
    const int64_t bad = ks_host_removable_carve();
    std::printf("carve_removable check: %lld violated\n", (long long)bad);
    return bad != 0;
}
#endif
