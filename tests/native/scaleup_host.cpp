// Host build of the scale-up preview's helpers (ks_query.h: scaleup_template, scaleup_whole_units,
// scaleup_fresh_key, scaleup_count_start, scaleup_takes_fresh, with the placement preview's
// functions), for CPU tests only.  ks_host_scaleup is a serial restatement of
// resolve_kernel<true>'s pod loop (ks_place.hip) for one option, on place_serial.h's list builder
// and pod loop: the snapshot lists and candidate counts of the n real nodes, the count start, the fresh appended
// node n + u standing for every unchanged one as the loop's extra candidate, no commit, a stop where
// the kernel stops.  ks_host_scaleup_brute is the plain sequential argmax over the n + max_nodes
// nodes of the extended cluster it must equal.  ks_host_scaleup_carve checks carve_scale_up's layout
// (ks_carve.h).  Not part of the product.
#include <cstdio>
#include <cstring>

#include "../../kubernetes-simulator_amd/csrc/ks_carve.h"
#include "place_serial.h"

using namespace place_serial;

// tmpl[7]: alloc[4] in milli-units, taint, label, max_nodes
#define CASE_ARGS CLUSTER_ARGS, int32_t k, const int32_t *shape_of, const int64_t *tmpl
#define CASE_PASS CLUSTER_PASS

static ks::NodeV make_tmpl(const int64_t* tmpl) {  // milli-units
    return ks::scaleup_template(tmpl, (uint64_t)tmpl[4], (uint64_t)tmpl[5], ks::QScale{{1, 1, 1}});
}

// scheduleOne as written, on the extended cluster
extern "C" int ks_host_scaleup_brute(CASE_ARGS, ks::Placement* out) {
    Cluster s = make_cluster(CASE_PASS);
    for (int32_t a = 0; a < (int32_t)tmpl[6]; a++) s.node.push_back(make_tmpl(tmpl));
    const int32_t n_ext = (int32_t)s.node.size();
    for (int32_t i = 0; i < k; i++) {
        const ks::PodRec& p = s.shapes[shape_of[i]];
        uint64_t best = 0;
        int64_t cand = 0;
        for (int32_t nd = 0; nd < n_ext; nd++) {
            const uint64_t key = ks::place_key(s.c, p, s.node[nd], (uint32_t)nd);
            cand += key != 0;
            best = key > best ? key : best;
        }
        if (!best) {
            out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cand};
            continue;
        }
        const uint32_t X = ks::place_key_node(best);
        const int32_t st = ks::place_bind(p, s.node[X]);
        out[i] = ks::Placement{(int32_t)X, st, (int64_t)(best >> 32) - 1, cand};
    }
    return 0;
}

// The per-option resolver.  Returns the pods decided: k, or the pod it stopped at (kPlaceStop).
// ablate bit 0: no fresh-node key (F = 0); bit 1: no count start.  stats[0]: pods won by the fresh
// node, stats[1]: pods won by a changed node (real or appended), stats[2]: the most flagged entries
// a pod found in its list, stats[3]: the changed set's final size; res: ks_scale_result's eight words.
extern "C" int ks_host_scaleup(CASE_ARGS, int32_t ablate, ks::Placement* out, int32_t* res, int64_t* stats) {
    const Cluster s = make_cluster(CASE_PASS);
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    // the fresh node n + u as the loop's extra candidate (thread nchg of the kernel)
    struct Fresh : Hooks {
        const Cluster& s;
        ks::NodeV tmpl;
        int32_t max_nodes, u;
        bool off;
        uint64_t extra_key(const ks::PodRec& p) const {
            return off ? 0ull : ks::scaleup_fresh_key(s.c, p, tmpl, s.n, u, max_nodes);
        }
        bool extra_joins(uint32_t X, ks::NodeV* v) {
            if (off || !ks::scaleup_takes_fresh(X, s.n, u, max_nodes)) return false;
            *v = tmpl;
            ++u;
            return true;
        }
    } h{{}, s, make_tmpl(tmpl), (int32_t)tmpl[6], 0, (ablate & 1) != 0};
    // ---- the shared lists and counts: the n real nodes on the base state; the count start ----
    Lists l = build_lists(s, nullptr, node_key(s));
    if (!(ablate & 2))
        for (int32_t j = 0; j < n_shapes; j++) l.cc[j] = ks::scaleup_count_start(s.c, s.shapes[j], h.tmpl, l.cc[j], h.max_nodes);
    std::vector<Chg> chg;
    const Run run = decide_pods(s, l, shape_of, 0, k, chg, h, out);
    stats[0] = run.from_extra; stats[1] = run.from_changed; stats[2] = run.most_flagged;
    if ((int64_t)chg.size() > ks::kPlaceMaxPods) return -2;
    // ---- the option's summary, from its rows and the final changed set ----
    ks::ScaleResult r{0, 0, 0, 0, 0, -1, run.stopped ? ks::kScaleStopped : ks::kScaleBatched, 0};
    for (int32_t i = 0; i < run.next; i++) {
        if (out[i].status == ks::kPlaceOk) {
            r.ok++;
            r.on_new += out[i].node >= n;
            continue;
        }
        (out[i].status == ks::kPlaceOverCapacity ? r.over_capacity : r.not_found)++;
        if (r.first_unplaced < 0) r.first_unplaced = i;
    }
    // the prefix invariant, checked on the final changed set
    int32_t seen = 0;
    for (const Chg& c : chg)
        if (c.node >= n) {
            if (c.node != n + seen) return -3;
            ++seen;
            r.nodes_used += c.v.nr > 0;
        }
    if (seen != h.u) return -3;
    stats[3] = (int64_t)chg.size();
    std::memcpy(res, &r, sizeof(r));
    return run.next;
}

// scaleup_whole_units on n_options templates of ks_scale_option's layout (7 words each)
extern "C" int ks_host_scaleup_whole(int32_t n_shapes, const int64_t* req, const uint32_t* keymask, int32_t n_options,
                                     const int64_t* options, const int64_t* scale) {
    std::vector<ks::PodRec> shapes(n_shapes);
    for (int32_t j = 0; j < n_shapes; j++) {
        for (int c = 0; c < 3; c++)
            if (keymask[j] >> c & 1) shapes[j].req[c] = req[j * 3 + c];
        shapes[j].keymask = keymask[j];
    }
    return ks::scaleup_whole_units(shapes.data(), n_shapes, options, n_options, 7, ks::QScale{{scale[0], scale[1], scale[2]}});
}

// out[10]: the template of alloc[4] (milli-units) divided by unit[3]
extern "C" void ks_host_scaleup_template(const int64_t* alloc, uint64_t taint, uint64_t label, const int64_t* unit, int64_t* out) {
    const ks::NodeV v = ks::scaleup_template(alloc, taint, label, ks::QScale{{unit[0], unit[1], unit[2]}});
    const int64_t w[10] = {v.ac, v.am, v.ag, v.ap, v.rc, v.rm, v.rg, v.nr, (int64_t)v.taint, (int64_t)v.label};
    std::memcpy(out, w, sizeof(w));
}

// carve_scale_up: two passes agree, every range lies inside the reserved size, is aligned and
// overlaps no other (each range is written); returns the violated checks
extern "C" int64_t ks_host_scaleup_carve() {
    using ks_host::Carve;
    int64_t bad = 0;
    struct Range { const char* name; const void* p; int64_t bytes, align; };
    for (int64_t n : {0, 1, 255, 256, 300, 600})
        for (int64_t k : {1, 33, 1024})
            for (int64_t g : {1, 5, 64})
                for (int64_t m : {0, 1, 213, 65536}) {
                    const int64_t np = std::max<int64_t>(64, (n + 63) / 64 * 64), nblk = (n + 255) / 256;
                    Carve qs(8), qi(4);
                    ks_host::carve_scale_up(qs, qi, n, np, nblk, k, g, m);
                    std::vector<long double> m_qs((qs.at * 8 + 15) / 16 + 1), m_qi((qi.at * 4 + 15) / 16 + 1);
                    const int64_t w_qs = qs.at, w_qi = qi.at;
                    qs = Carve(8, m_qs.data());
                    qi = Carve(4, m_qi.data());
                    const ks_host::ScaleScratch s = ks_host::carve_scale_up(qs, qi, n, np, nblk, k, g, m);
                    if (qs.at != w_qs || qi.at != w_qi) bad++;
                    const int64_t ne = n + m, npe = std::max<int64_t>(64, (ne + 63) / 64 * 64), nbe = (ne + 255) / 256;
                    if (s.n_ext != ne || s.np_ext != npe || s.nblk_ext != nbe || s.b.n_pad != np || s.x.n_pad != npe) bad++;
                    constexpr int64_t S = ks::kPlaceMaxShapes;
                    const std::vector<Range> r8 = {
                        {"state", s.b.state, 32 * np, 8}, {"shapes", s.b.shapes, 48 * S, 16}, {"shape_of", s.b.shape_of, 4 * k, 4},
                        {"lists", s.b.lists, 8 * S * nblk * L, 8}, {"top", s.b.top, 8 * S * L, 8}, {"ccount", s.b.ccount, 8 * S, 8},
                        {"rb", s.b.rb, 16, 4}, {"opts", s.sb.opts, 88 * g, 8}, {"rows", s.sb.rows, 24 * g * k, 8},
                        {"out", s.sb.out, 32 * g, 8}, {"ext_node", s.ext_node, 48 * npe, 8}, {"x.state", s.x.state, 32 * npe, 8},
                        {"x.shapes", s.x.shapes, 48 * S, 16}, {"x.shape_of", s.x.shape_of, 4 * k, 4},
                        {"x.lists", s.x.lists, 8 * S * nbe * L, 8}, {"x.top", s.x.top, 8 * S * L, 8},
                        {"x.ccount", s.x.ccount, 8 * S, 8}, {"x.rb", s.x.rb, 16, 4}, {"x.out", s.x.out, 24 * k, 8}};
                    const std::vector<Range> r4 = {{"cnt", s.b.cnt, 4 * S * nblk, 4}, {"x.cnt", s.x.cnt, 4 * S * nbe, 4}};
                    auto check = [&](char* base, int64_t bytes, const std::vector<Range>& rs) {
                        for (const Range& r : rs) {
                            const int64_t off = (const char*)r.p - base;
                            if (off < 0 || off + r.bytes > bytes) { bad++; continue; }
                            std::memset(base + off, 0x5A, r.bytes);
                            if (off % r.align) bad++;
                            for (const Range& q : rs)
                                if (&q != &r && r.bytes && q.bytes && (const char*)q.p < (const char*)r.p + r.bytes &&
                                    (const char*)r.p < (const char*)q.p + q.bytes)
                                    bad++;
                        }
                    };
                    check((char*)m_qs.data(), w_qs * 8, r8);
                    check((char*)m_qi.data(), w_qi * 4, r4);
                }
    return bad;
}

extern "C" int ks_host_scaleup_l() { return L; }

#ifdef KS_SCALEUP_MAIN
// a stand-alone program (for a sanitizer build: -fsanitize=address,undefined on the host side): the
// layout check, and 40 equal nodes + 3 of a larger template for 200 pods through both drivers
int main() {
    const int64_t bad = ks_host_scaleup_carve();
    const int32_t n = 40, k = 200;
    std::vector<int64_t> alloc(n * 4), state(n * 4, 0);
    for (int32_t i = 0; i < n; i++) { alloc[i * 4] = 16000; alloc[i * 4 + 1] = 64000; alloc[i * 4 + 2] = 8000; alloc[i * 4 + 3] = 3; }
    std::vector<uint64_t> taint(n, 0), label(n, 0);
    const int64_t scale[3] = {1, 1, 1}, req[3] = {1000, 4000, 0}, tmpl[7] = {32000, 128000, 8000, 5, 0, 0, 3};
    const int32_t cfg[6] = {1, 7, 1, 1, 1, 0};
    const uint32_t km[1] = {3};
    const uint64_t tol[1] = {0}, sel[1] = {0};
    std::vector<int32_t> so(k, 0);
    std::vector<ks::Placement> a(k), b(k);
    int32_t res[8];
    int64_t stats[4];
    ks_host_scaleup_brute(n, alloc.data(), scale, state.data(), taint.data(), label.data(), cfg, 1, req, km, tol, sel, k, so.data(),
                          tmpl, a.data());
    const int done = ks_host_scaleup(n, alloc.data(), scale, state.data(), taint.data(), label.data(), cfg, 1, req, km, tol, sel, k,
                                     so.data(), tmpl, 0, b.data(), res, stats);
    int64_t differ = done < 0;
    for (int i = 0; i < done; i++) differ += std::memcmp(&a[i], &b[i], sizeof(ks::Placement)) != 0;
    std::printf("scale-up host check: %lld layout violations, %d of %d pods decided, %lld rows differ\n", (long long)bad, done, k,
                (long long)differ);
    return bad != 0 || differ != 0;
}
#endif
