// Host build of the gang admission preview's host-side pieces (ks_query.h: gang_route, gang_segment
// and the placement functions; ks_carve.h: carve_gang), for CPU tests only.
//   ks_host_gang          a serial restatement of ks_gang_at's rounds on place_serial.h's list builder
//                         and pod loop: the lists of the committed state, the gangs of a round walked as
//                         transactions (roll-back of the changed set, the flags, the counts and nchg on
//                         a block or a stop; only the tried pods bound Ok subtract), the single path for
//                         a gang of more than kPlaceL pods;
//   ks_host_gang_brute    the chain as written: the plain sequential argmax over the nodes, a copy of
//                         the cluster restored on a block;
//   ks_host_gang_segment  the round walk (gang_segment);
//   ks_host_gang_route    who decides a gang;
//   ks_host_gang_carve    carve_gang run twice, as ks_gang_at does.
// Gang g's pods are rows [first[g], first[g + 1]) of shape_of / out.  Not part of the product.
#include <cstdio>
#include <cstring>

#include "../../kubernetes-simulator_amd/csrc/ks_carve.h"
#include "place_serial.h"

using namespace place_serial;

#define CASE_ARGS                                                                                              \
    CLUSTER_ARGS, int32_t k, const int32_t *shape_of, int32_t m, const int32_t *first, const int32_t *min_ok, \
        int32_t strict
#define CASE_PASS CLUSTER_PASS

static const ks::Placement kUntried{-1, ks::kGangNotTried, -1, 0};

// a pod's status joins the gang's tally; whether it blocks the gang
static bool tally_blocks(ks::Gang& o, int32_t min_ok, int32_t status) {
    (status == ks::kPlaceOk ? o.ok : status == ks::kPlaceOverCapacity ? o.over_capacity : o.not_found)++;
    o.tried++;
    if (o.over_capacity + o.not_found <= o.size - min_ok) return false;
    o.outcome = ks::kGangBlocked;
    o.block_status = status;
    return true;
}

// The chain as the header states it.
extern "C" int ks_host_gang_brute(CASE_ARGS, ks::Placement* out, ks::Gang* res, int64_t* after) {
    Cluster s = make_cluster(CASE_PASS);
    for (int32_t i = 0; i < k; i++) out[i] = kUntried;
    bool over = false;
    for (int32_t g = 0; g < m; g++) {
        const int32_t lo = first[g], size = first[g + 1] - first[g];
        res[g] = ks::Gang{lo, size, over ? ks::kGangSkipped : ks::kGangAdmitted, 0, 0, 0, 0, 0};
        if (over) continue;
        const Cluster saved = s;
        for (int32_t i = lo; i < lo + size; i++) {
            const ks::PodRec& p = s.shapes[shape_of[i]];
            uint64_t best = 0;
            int64_t cnd = 0;
            for (int32_t nd = 0; nd < n; nd++) {
                const uint64_t key = ks::place_key(s.c, p, s.node[nd], (uint32_t)nd);
                cnd += key != 0;
                best = key > best ? key : best;
            }
            int32_t status = ks::kPlaceNotFound;
            if (!best) {
                out[i] = ks::Placement{-1, status, -1, cnd};
            } else {
                const uint32_t X = ks::place_key_node(best);
                status = ks::place_bind(p, s.node[X]);
                out[i] = ks::Placement{(int32_t)X, status, (int64_t)(best >> 32) - 1, cnd};
            }
            if (tally_blocks(res[g], min_ok[g], status)) break;
        }
        if (res[g].outcome == ks::kGangBlocked) {
            s = saved;
            over = strict != 0;
        }
    }
    state_out(s, after);
    return 0;
}

// The rounds.  `mode` takes one part of the roll-back out, to show that the tests see it: 1: the flag
// words are not restored, 2: the running counts are not restored, 3: nchg is not restored (the slots
// the attempt appended stay), 4: every tried pod that had a winner subtracts, not only those bound Ok.
// info[0]: rounds of the chain, info[1]: gangs of the single path; stats[0]: roll-backs after at
// least one Ok pod, [1]: rounds ended by kPlaceStop inside a gang, [2]: Ok pods taken back out of a
// slot that existed before the attempt, [3]: pods decided from the changed set, [4]: tried pods not
// bound Ok on a kept slot in a rolled-back attempt.  Returns 0, -1: a round decided no gang, -3: the
// single path's rounds failed.
extern "C" int ks_host_gang(CASE_ARGS, int32_t mode, ks::Placement* out, ks::Gang* res, int64_t* after, int64_t* info,
                            int64_t* stats) {
    Cluster s = make_cluster(CASE_PASS);
    std::vector<ks::GangIn> gangs(m);
    for (int32_t g = 0; g < m; g++) {
        gangs[g] = ks::GangIn{first[g], first[g + 1] - first[g], min_ok[g], 0};
        res[g] = ks::Gang{gangs[g].first, gangs[g].size, ks::kGangUndecided, 0, 0, 0, 0, 0};
    }
    for (int32_t i = 0; i < k; i++) out[i] = kUntried;
    std::vector<ks::PodRec> recs(k);
    for (int32_t i = 0; i < k; i++) recs[i] = s.shapes[shape_of[i]];
    info[0] = info[1] = 0;
    for (int j = 0; j < 5; j++) stats[j] = 0;
    std::vector<int32_t> so(ks::kPlaceMaxPods);
    Hooks h;
    bool over = false;
    for (int32_t cur = 0; cur < m && !over;) {
        const ks::GangIn gd = gangs[cur];
        if (ks::gang_route(gd.size) == ks::kGangSingle) {
            // the single path: a copy, the drain preview's segmented rounds, the early end on the finished rows
            Cluster x = s;
            ks::Gang& o = res[cur];
            o.outcome = ks::kGangAdmitted;
            std::vector<ks::Placement> rows(gd.size);
            bool go_on = true;
            for (int64_t start = 0; start < gd.size && go_on;) {
                Cluster seg = x;
                seg.shapes.assign(ks::kPlaceMaxShapes, ks::PodRec{});
                int32_t ns = 0;
                const int64_t end = ks::drain_segment(recs.data() + gd.first, gd.size, start, seg.shapes.data(), &ns, so.data());
                if (end <= start) return -3;
                seg.shapes.resize(ns);
                int64_t rinfo[4] = {0, 0, 0, 0};
                if (run_rounds(seg, so.data(), (int32_t)(end - start), node_key(seg), h, rows.data() + start, rinfo, nullptr)) return -3;
                x.node = seg.node;
                info[0] += rinfo[0];
                for (int64_t i = start; i < end && go_on; i++) {
                    out[gd.first + i] = rows[i];
                    go_on = !tally_blocks(o, gd.min_ok, rows[i].status);
                }
                start = end;
            }
            if (o.outcome == ks::kGangAdmitted) s = x;
            over = strict && o.outcome == ks::kGangBlocked;
            info[1]++;
            cur++;
            continue;
        }
        // ---- one round: the segment, its lists on the committed state, the transactions ----
        Cluster seg = s;
        seg.shapes.assign(ks::kPlaceMaxShapes, ks::PodRec{});
        int32_t ns = 0, k_seg = 0;
        const int64_t end = ks::gang_segment(recs.data(), gangs.data(), m, cur, seg.shapes.data(), &ns, so.data(), &k_seg);
        if (end <= cur) return -1;
        seg.shapes.resize(ns);
        Lists l = build_lists(seg, nullptr, node_key(seg));
        std::vector<Chg> chg;
        std::vector<ks::Placement> got(std::max(k_seg, 1));
        bool stopped = false;
        int32_t a = cur;
        for (; a < end && !stopped && !over; a++) {
            const ks::GangIn c = gangs[a];
            ks::Gang o = res[a];
            o.outcome = ks::kGangAdmitted;
            const size_t nchg_s = chg.size();
            const std::vector<uint32_t> flag_s = l.flag;
            const std::vector<long long> cc_s = l.cc;
            const int32_t beg = c.first - gd.first;
            int32_t i = beg;
            for (; i < beg + c.size; i++) {
                const Run r = decide_pods(seg, l, so.data(), i, i + 1, chg, h, got.data());
                stats[3] += r.from_changed;
                if (r.stopped) {
                    stopped = true;
                    break;
                }
                if (tally_blocks(o, c.min_ok, got[i].status)) {
                    i++;
                    break;
                }
            }
            if (!stopped && o.outcome == ks::kGangAdmitted) {  // admit: nothing is restored
                for (int32_t q = beg; q < beg + c.size; q++) out[gd.first + q] = got[q];
                res[a] = o;
                continue;
            }
            // roll back: pods [beg, i) were tried
            stats[0] += o.ok > 0;
            for (int32_t q = beg; q < i; q++) {
                if (got[q].node < 0 || (got[q].status != ks::kPlaceOk && mode != 4)) continue;
                size_t slot = 0;
                while (slot < chg.size() && chg[slot].node != got[q].node) slot++;
                if (slot >= nchg_s) continue;  // (appended by the attempt: dropped below)
                if (got[q].status != ks::kPlaceOk) stats[4]++;
                const ks::PodRec& p = seg.shapes[so[q]];
                if (p.keymask & 1) chg[slot].v.rc -= p.req[0];
                if (p.keymask & 2) chg[slot].v.rm -= p.req[1];
                if (p.keymask & 4) chg[slot].v.rg -= p.req[2];
                chg[slot].v.nr -= 1;
                stats[2]++;
            }
            if (mode != 4)
                for (int32_t q = beg; q < i; q++) {  // (counted for the tests: what mode 4 would take out wrongly)
                    if (got[q].node < 0 || got[q].status == ks::kPlaceOk) continue;
                    size_t slot = 0;
                    while (slot < chg.size() && chg[slot].node != got[q].node) slot++;
                    stats[4] += slot < nchg_s;
                }
            if (mode != 1) l.flag = flag_s;
            if (mode != 2) l.cc = cc_s;
            if (mode != 3) chg.resize(nchg_s);
            if (stopped) {
                stats[1]++;
                break;  // (a is the gang that opens the next round)
            }
            for (int32_t q = beg; q < i; q++) out[gd.first + q] = got[q];
            res[a] = o;
            over = strict != 0;
        }
        if ((int64_t)chg.size() > ks::kPlaceMaxPods) return -1;
        for (const Chg& x : chg) s.node[x.node] = x.v;  // commit
        if (a == cur) return -1;
        cur = a;
        info[0]++;
    }
    for (int32_t g = 0; g < m; g++)
        if (res[g].outcome == ks::kGangUndecided) res[g].outcome = ks::kGangSkipped;
    state_out(s, after);
    return 0;
}

// gang_segment from gang `start` over m gangs, gang g's pods the next cnt[g] rows, row i's shape the
// record of id ids[i].  Returns the end, the shapes in *n_shapes and shapes_out, the pods in *n_pods
// and shape_of[row - first row of start].
extern "C" int64_t ks_host_gang_segment(int64_t m, const int32_t* cnt, const int64_t* ids, int64_t start, int32_t* n_shapes,
                                        int32_t* n_pods, int32_t* shape_of, ks::PodRec* shapes_out) {
    std::vector<ks::GangIn> gangs(m);
    int32_t rows = 0;
    for (int64_t a = 0; a < m; a++) {
        gangs[a] = ks::GangIn{rows, cnt[a], cnt[a], 0};
        rows += cnt[a];
    }
    std::vector<ks::PodRec> recs(rows);
    for (int32_t i = 0; i < rows; i++) {
        recs[i] = ks::PodRec{};
        recs[i].req[0] = 1000 + ids[i];
        recs[i].req[1] = 77;  // (unmasked: ignored)
        recs[i].keymask = 1;
        recs[i].tol = (uint64_t)ids[i] * 0x9E3779B97F4A7C15ull;
        recs[i].flags = (uint32_t)(ids[i] & 3);
    }
    return ks::gang_segment(recs.data(), gangs.data(), m, start, shapes_out, n_shapes, shape_of, n_pods);
}

extern "C" int ks_host_gang_route(int64_t pods) { return ks::gang_route(pods); }

extern "C" int ks_host_gang_limits(int32_t* out) {
    out[0] = ks::kPlaceMaxShapes; out[1] = ks::kGangMaxPods; out[2] = L; out[3] = (int32_t)sizeof(ks::Gang);
    out[4] = ks::kPlaceMaxPods; out[5] = ks::kGangRound; out[6] = ks::kGangSingle;
    out[7] = ks::kGangBlocked; out[8] = ks::kGangAdmitted; out[9] = ks::kGangSkipped;
    out[10] = ks::kGangNotTried; out[11] = ks::kGangMaxShapes; out[12] = (int32_t)ks::kGangMaxGangs; out[13] = (int32_t)sizeof(ks::GangIn);
    return 0;
}

// carve_gang at edge counts, twice as ks_gang_at runs it: every range inside the reserved size,
// aligned for its element, overlapping no other, and written.  Returns the violated checks.
extern "C" int64_t ks_host_gang_carve() {
    using ks_host::Carve;
    struct Range { const char* name; const void* p; int64_t bytes, align; };
    int64_t bad = 0;
    auto fail = [&](const char* what, const char* name, int64_t a, int64_t b) {
        if (bad++ < 20) std::fprintf(stderr, "carve_gang: %s: %s (%lld, %lld)\n", name, what, (long long)a, (long long)b);
    };
    for (int64_t n : {1, 31, 32, 33, 255, 256, 257, 600})
        for (int64_t k : {1, 3, 33, 1000, 1025, 65536})
            for (int64_t m : {(int64_t)1, k, (int64_t)65536}) {
                const int64_t np = (n + 63) / 64 * 64, nblk = (n + 255) / 256;
                Carve qs(8), qi(4);
                ks_host::carve_gang(qs, qi, n, np, nblk, k, m);
                const int64_t words = qs.at, iwords = qi.at;
                std::vector<long double> mem((words * 8 + 15) / 16 + 1), imem((iwords * 4 + 15) / 16 + 1);
                char* base = (char*)mem.data();
                char* ibase = (char*)imem.data();
                qs = Carve(8, base);
                qi = Carve(4, ibase);
                const ks_host::GangScratch s = ks_host::carve_gang(qs, qi, n, np, nblk, k, m);
                if (qs.at != words || qi.at != iwords) fail("the two passes differ", "d_qs", qs.at, words);
                if (s.b.n_pad != np) fail("capacities", "gang", s.b.n_pad, np);
                const int64_t S = ks::kPlaceMaxShapes;
                const int64_t cnt_off = (const char*)s.b.cnt - ibase;
                if (cnt_off < 0 || cnt_off + 4 * S * nblk > iwords * 4) fail("outside the reserved size", "cnt", cnt_off, 4 * S * nblk);
                else std::memset(ibase + cnt_off, 0x5A, 4 * S * nblk);
                const std::vector<Range> rs = {
                    {"state", s.b.state, 32 * np, 8},
                    {"shapes", s.b.shapes, 48 * S, 16},
                    {"shape_of", s.b.shape_of, 4 * ks::kPlaceMaxPods, 4},
                    {"lists", s.b.lists, 8 * S * nblk * L, 8},
                    {"top", s.b.top, 8 * S * L, 8},
                    {"ccount", s.b.ccount, 8 * S, 8},
                    {"rb", s.b.rb, 16, 4},
                    {"placed", s.b.out, 24 * k, 8},
                    {"state2", s.state2, 32 * np, 8},
                    {"gangs", s.gangs, 16 * m, 16},
                    {"out", s.out, 32 * m, 8},
                    {"after", s.after, 32 * n, 8}};
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

#ifdef KS_GANG_MAIN
// A small chain on a hand-made cluster (rounds against the chain as written, a gang of the single
// path and a strict pass among them), the route, the round walk and the scratch layout.
int main() {
    int64_t bad = ks_host_gang_carve();
    std::printf("carve_gang check: %lld violated\n", (long long)bad);
    const int32_t n = 40, ns = 3, m = 9;
    std::vector<int64_t> alloc(n * 4), state(n * 4, 0);
    std::vector<uint64_t> taint(n, 0), label(n, 0);
    for (int32_t i = 0; i < n; i++) {
        alloc[i * 4] = 4000 + 500 * (i % 5); alloc[i * 4 + 1] = 8000; alloc[i * 4 + 2] = 0; alloc[i * 4 + 3] = 3;
        state[i * 4] = 250 * (i % 7); state[i * 4 + 3] = i % 2;
    }
    const int64_t scale[3] = {1, 1, 1};
    const int32_t cfg[6] = {1, 1, 1, 1, 1, 0};
    const int64_t req[ns * 3] = {1000, 1000, 0, 2500, 500, 0, 700, 3000, 0};
    const uint32_t keymask[ns] = {3, 3, 3};
    const uint64_t tol[ns] = {0, 0, 0}, sel[ns] = {0, 0, 0};
    const int32_t sizes[m] = {3, 0, 40, 7, 33, 12, 50, 1, 5};
    std::vector<int32_t> first(m + 1, 0), min_ok(m), shape_of;
    for (int32_t g = 0; g < m; g++) {
        first[g + 1] = first[g] + sizes[g];
        min_ok[g] = g % 3 == 2 ? sizes[g] * 3 / 4 : sizes[g];
        for (int32_t i = 0; i < sizes[g]; i++) shape_of.push_back((g + i) % ns);
    }
    const int32_t k = first[m];
    for (int32_t strict = 0; strict < 2; strict++) {
        std::vector<ks::Placement> a(k), b(k);
        std::vector<ks::Gang> ra(m), rb(m);
        std::vector<int64_t> fa(n * 4), fb(n * 4);
        int64_t info[2], stats[5];
        const int rc = ks_host_gang(n, alloc.data(), scale, state.data(), taint.data(), label.data(), cfg, ns, req, keymask, tol, sel, k,
                                    shape_of.data(), m, first.data(), min_ok.data(), strict, 0, a.data(), ra.data(), fa.data(), info, stats);
        ks_host_gang_brute(n, alloc.data(), scale, state.data(), taint.data(), label.data(), cfg, ns, req, keymask, tol, sel, k,
                           shape_of.data(), m, first.data(), min_ok.data(), strict, b.data(), rb.data(), fb.data());
        const bool same = rc == 0 && !std::memcmp(a.data(), b.data(), sizeof(ks::Placement) * k) &&
                          !std::memcmp(ra.data(), rb.data(), sizeof(ks::Gang) * m) && fa == fb;
        int32_t adm = 0, blk = 0;
        for (const ks::Gang& g : rb) { adm += g.outcome == ks::kGangAdmitted; blk += g.outcome == ks::kGangBlocked; }
        std::printf("chain (strict %d): rc %d, %s, %d admitted, %d blocked, %lld rounds, %lld single\n", strict, rc,
                    same ? "equal" : "DIFFERENT", adm, blk, (long long)info[0], (long long)info[1]);
        bad += !same;
    }
    bad += ks::gang_route(L) != ks::kGangRound || ks::gang_route(L + 1) != ks::kGangSingle;
    return bad != 0;
}
#endif
