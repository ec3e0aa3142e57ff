// Host build of the removal scan's host-side pieces (ks_device.h: removable_route,
// removable_entries_on, removable_segment and the placement functions; ks_carve.h: carve_removable),
// for CPU tests only.
//   ks_host_removable          a serial restatement of removable_resolve_kernel (ks_removable.hip) for
//                              one candidate: the shapes' top-L lists and candidate counts of the base
//                              state with no cordon, the candidate's own entries flagged from the
//                              start, its counts corrected, its pods decided from that one set of lists;
//   ks_host_removable_brute    the plain sequential argmax over the nodes other than the candidate;
//   ks_host_removable_segments ks_removable_at's candidate-aligned segment walk;
//   ks_host_removable_route    the split between the batched resolver and the single-drain path;
//   ks_host_removable_carve    carve_removable run twice, as ks_removable_at does.
// Not part of the product.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../kubernetes-simulator_amd/csrc/ks_carve.h"

namespace {

constexpr int L = ks::kPlaceL;
constexpr int kBlk = 256;

struct Case {
    int32_t n;
    std::vector<ks::NodeV> node;
    ks::Cfg c{};
    std::vector<ks::PodRec> shapes;
};

// cfg[6]: filter_feeds, filters, has_scorers, w_lr, w_ba, const_total
Case make_case(int32_t n, const int64_t* alloc_dev, const int64_t* scale, const int64_t* state_m, const uint64_t* taint,
               const uint64_t* label, const int32_t* cfg, int32_t n_shapes, const int64_t* req, const uint32_t* keymask,
               const uint64_t* tol, const uint64_t* sel) {
    Case s;
    s.n = n;
    const ks::QScale sc{{scale[0], scale[1], scale[2]}};
    for (int32_t i = 0; i < n; i++) {
        ks::NodeV v{};
        v.ac = alloc_dev[i * 4 + 0]; v.am = alloc_dev[i * 4 + 1]; v.ag = alloc_dev[i * 4 + 2]; v.ap = alloc_dev[i * 4 + 3];
        ks::place_scale_alloc(v, sc);
        v.rc = state_m[i * 4 + 0]; v.rm = state_m[i * 4 + 1]; v.rg = state_m[i * 4 + 2]; v.nr = state_m[i * 4 + 3];
        v.taint = taint[i]; v.label = label[i];
        s.node.push_back(v);
    }
    s.c.n_nodes = n;
    s.c.filter_feeds = cfg[0]; s.c.filters = (uint32_t)cfg[1]; s.c.has_scorers = cfg[2];
    s.c.w_lr = cfg[3]; s.c.w_ba = cfg[4]; s.c.const_total = cfg[5];
    for (int32_t j = 0; j < n_shapes; j++) {
        ks::PodRec p{};
        for (int c = 0; c < 3; c++)
            if (keymask[j] >> c & 1) p.req[c] = req[j * 3 + c];
        p.tol = tol[j]; p.sel = sel[j]; p.keymask = keymask[j];
        s.shapes.push_back(p);
    }
    return s;
}

void count(const ks::Placement* out, int32_t k, int64_t* info) {
    info[1] = info[2] = info[3] = 0;
    for (int32_t i = 0; i < k; i++) info[out[i].status == ks::kPlaceOk ? 1 : out[i].status == ks::kPlaceOverCapacity ? 2 : 3]++;
}

}  // namespace

#define CASE_ARGS                                                                                                  \
    int32_t n, const int64_t *alloc_dev, const int64_t *scale, const int64_t *state_m, const uint64_t *taint,     \
        const uint64_t *label, const int32_t *cfg, int32_t n_shapes, const int64_t *req, const uint32_t *keymask,   \
        const uint64_t *tol, const uint64_t *sel, int32_t k, const int32_t *shape_of, int32_t cand
#define CASE_PASS n, alloc_dev, scale, state_m, taint, label, cfg, n_shapes, req, keymask, tol, sel

// scheduleOne as written, over the nodes other than the candidate (whose own state is never read)
extern "C" int ks_host_removable_brute(CASE_ARGS, ks::Placement* out, int64_t* info) {
    Case s = make_case(CASE_PASS);
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
    count(out, k, info);
    return 0;
}

// The resolver of one candidate.  `mode` takes out one of the two corrections, to show that the tests
// see them: 1: the own-node flags are not pre-set; 2: the counts are not corrected.  Returns 0, -1 when
// a pod met kPlaceStop (more pods than one set of lists decides), -2 when the candidate itself won.
// stats[0]: pods decided from a changed node, stats[1]: the most flagged entries of a list at the end,
// stats[2]: lists the candidate's own node is in.
extern "C" int ks_host_removable(CASE_ARGS, int32_t mode, ks::Placement* out, int64_t* info, int64_t* stats) {
    Case s = make_case(CASE_PASS);
    const int32_t nblk = (n + kBlk - 1) / kBlk;
    // launch_place_lists: every shape, the base state, no cordon
    std::vector<uint64_t> top((size_t)n_shapes * L, 0ull);
    std::vector<uint32_t> flag(n_shapes, 0u);
    std::vector<int> len(n_shapes, 0);
    std::vector<int64_t> cc(n_shapes, 0);
    stats[0] = stats[1] = stats[2] = 0;
    for (int32_t j = 0; j < n_shapes; j++) {
        uint64_t t[L] = {};
        for (int32_t b = 0; b < nblk; b++) {
            std::vector<uint64_t> keys;
            for (int32_t nd = b * kBlk; nd < std::min(n, (b + 1) * kBlk); nd++)
                keys.push_back(ks::place_key(s.c, s.shapes[j], s.node[nd], (uint32_t)nd));
            std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b2) { return a > b2; });
            uint64_t lv[L] = {};
            for (int e = 0; e < L && e < (int)keys.size(); e++) lv[e] = keys[e];
            for (uint64_t key : keys) cc[j] += key != 0;
            ks::topl_insert<L>(t, lv);
        }
        std::copy(t, t + L, top.begin() + (size_t)j * L);
        len[j] = ks::place_list_len<L>(t);
        // the candidate's two corrections
        const uint32_t own = ks::removable_entries_on<L>(t, (uint32_t)cand);
        stats[2] += own != 0;
        if (mode != 1) flag[j] = own;
        if (mode != 2) cc[j] -= ks::place_is_cand(s.c, s.shapes[j], s.node[cand]);
    }
    struct Chg { int32_t node; ks::NodeV v; };
    std::vector<Chg> chg;
    for (int32_t i = 0; i < k; i++) {
        const int sh = shape_of[i];
        const ks::PodRec& p = s.shapes[sh];
        uint64_t D = 0;
        int32_t d_idx = -1;
        for (size_t c = 0; c < chg.size(); c++) {
            const uint64_t key = ks::place_key(s.c, p, chg[c].v, (uint32_t)chg[c].node);
            if (key > D) { D = key; d_idx = (int32_t)c; }
        }
        const uint64_t* list = &top[(size_t)sh * L];
        const int eS = ks::place_first_unchanged<L>(len[sh], flag[sh]);
        const uint64_t S = eS < L ? list[eS] : 0ull;
        uint64_t W;
        const int dec = ks::place_decide(S, list[L - 1], D, &W);
        if (dec == ks::kPlaceStop) return -1;
        const int64_t cnd = cc[sh];
        if (dec == ks::kPlaceNone) {
            out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cnd};
            continue;
        }
        const uint32_t X = ks::place_key_node(W);
        if ((int32_t)X == cand && mode == 0) return -2;
        int32_t idx;
        if (W == D) {
            idx = d_idx;
            stats[0]++;
        } else {
            idx = (int32_t)chg.size();
            chg.push_back(Chg{(int32_t)X, s.node[X]});
            for (int32_t j = 0; j < n_shapes; j++) flag[j] |= ks::removable_entries_on<L>(&top[(size_t)j * L], X);
        }
        const ks::NodeV before = chg[idx].v;
        ks::NodeV aft = before;
        const int32_t st = ks::place_bind(p, aft);
        if (st == ks::kPlaceOk)
            for (int32_t j = 0; j < n_shapes; j++) cc[j] += ks::place_cand_delta(s.c, s.shapes[j], before, aft);
        out[i] = ks::Placement{(int32_t)X, st, (int64_t)(W >> 32) - 1, cnd};
        if (st == ks::kPlaceOk) chg[idx].v = aft;
    }
    for (int32_t j = 0; j < n_shapes; j++) stats[1] = std::max<int64_t>(stats[1], __builtin_popcount(flag[j]));
    count(out, k, info);
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
