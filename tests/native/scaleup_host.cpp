// Host build of the scale-up preview's helpers (ks_device.h: scaleup_template, scaleup_whole_units,
// scaleup_fresh_key, scaleup_count_start, scaleup_takes_fresh, with the placement preview's
// place_key / place_first_unchanged / place_decide / place_bind / place_cand_delta / topl_insert), for
// CPU tests only.  ks_host_scaleup is a serial restatement of scaleup_resolve_kernel's pod loop for one
// option: the snapshot lists and candidate counts of the n real nodes, the changed set, the fresh
// appended node n + u standing for every unchanged one, no commit, a stop where the kernel stops.
// ks_host_scaleup_brute is the plain sequential argmax over the n + max_nodes nodes of the extended
// cluster it must equal.  ks_host_scaleup_carve checks carve_scale_up's layout (ks_carve.h).  Not
// part of the product.
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
    std::vector<ks::NodeV> node;  // milli-units
    ks::Cfg c{};
    std::vector<ks::PodRec> shapes;
    int32_t k;
    const int32_t* shape_of;
    ks::NodeV tmpl{};
    int32_t max_nodes;
};

// cfg[6]: filter_feeds, filters, has_scorers, w_lr, w_ba, const_total; tmpl[7]: alloc[4] in
// milli-units, taint, label, max_nodes
Case make_case(int32_t n, const int64_t* alloc_dev, const int64_t* scale, const int64_t* state_m, const uint64_t* taint,
               const uint64_t* label, const int32_t* cfg, int32_t n_shapes, const int64_t* req, const uint32_t* keymask,
               const uint64_t* tol, const uint64_t* sel, int32_t k, const int32_t* shape_of, const int64_t* tmpl) {
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
    s.k = k;
    s.shape_of = shape_of;
    s.tmpl = ks::scaleup_template(tmpl, (uint64_t)tmpl[4], (uint64_t)tmpl[5], ks::QScale{{1, 1, 1}});  // milli-units
    s.max_nodes = (int32_t)tmpl[6];
    return s;
}

}  // namespace

#define CASE_ARGS                                                                                                  \
    int32_t n, const int64_t *alloc_dev, const int64_t *scale, const int64_t *state_m, const uint64_t *taint,     \
        const uint64_t *label, const int32_t *cfg, int32_t n_shapes, const int64_t *req, const uint32_t *keymask,   \
        const uint64_t *tol, const uint64_t *sel, int32_t k, const int32_t *shape_of, const int64_t *tmpl
#define CASE_PASS n, alloc_dev, scale, state_m, taint, label, cfg, n_shapes, req, keymask, tol, sel, k, shape_of, tmpl

// scheduleOne as written, on the extended cluster
extern "C" int ks_host_scaleup_brute(CASE_ARGS, ks::Placement* out) {
    Case s = make_case(CASE_PASS);
    for (int32_t a = 0; a < s.max_nodes; a++) s.node.push_back(s.tmpl);
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
    Case s = make_case(CASE_PASS);
    const int32_t nblk = (n + kBlk - 1) / kBlk;
    // ---- the shared lists and counts: the n real nodes on the base state ----
    std::vector<uint64_t> top((size_t)n_shapes * L, 0ull);
    std::vector<uint32_t> flag(n_shapes, 0u);
    std::vector<int> len(n_shapes, 0);
    std::vector<long long> cc(n_shapes, 0);
    for (int32_t j = 0; j < n_shapes; j++) {
        uint64_t t[L] = {};
        long long base = 0;
        for (int32_t b = 0; b < nblk; b++) {
            std::vector<uint64_t> keys;
            for (int32_t nd = b * kBlk; nd < std::min(n, (b + 1) * kBlk); nd++)
                keys.push_back(ks::place_key(s.c, s.shapes[j], s.node[nd], (uint32_t)nd));
            std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b2) { return a > b2; });
            uint64_t lv[L] = {};
            for (int e = 0; e < L && e < (int)keys.size(); e++) lv[e] = keys[e];
            for (uint64_t key : keys) base += key != 0;
            ks::topl_insert<L>(t, lv);
        }
        std::copy(t, t + L, top.begin() + (size_t)j * L);
        len[j] = ks::place_list_len<L>(t);
        cc[j] = (ablate & 2) ? base : ks::scaleup_count_start(s.c, s.shapes[j], s.tmpl, base, s.max_nodes);
    }
    // ---- the pod loop ----
    struct Chg { int32_t node; ks::NodeV v; };
    std::vector<Chg> chg;
    int32_t u = 0, i = 0;
    ks::ScaleResult r{0, 0, 0, 0, 0, -1, ks::kScaleBatched, 0};
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    for (; i < k; i++) {
        const int sh = shape_of[i];
        const ks::PodRec& p = s.shapes[sh];
        uint64_t D = 0;
        int32_t d_idx = -1;
        for (size_t c = 0; c < chg.size(); c++) {
            const uint64_t key = ks::place_key(s.c, p, chg[c].v, (uint32_t)chg[c].node);
            if (key > D) { D = key; d_idx = (int32_t)c; }
        }
        const uint64_t F = (ablate & 1) ? 0ull : ks::scaleup_fresh_key(s.c, p, s.tmpl, n, u, s.max_nodes);
        if (F > D) { D = F; d_idx = (int32_t)chg.size(); }  // (slot nchg: the fresh node's, if it wins)
        const uint64_t* list = &top[(size_t)sh * L];
        stats[2] = std::max<int64_t>(stats[2], __builtin_popcount(flag[sh]));
        const int eS = ks::place_first_unchanged<L>(len[sh], flag[sh]);
        const uint64_t S = eS < L ? list[eS] : 0ull;
        uint64_t W;
        const int dec = ks::place_decide(S, list[L - 1], D, &W);
        if (dec == ks::kPlaceStop) {
            r.path = ks::kScaleStopped;
            break;
        }
        const int64_t cand = cc[sh];
        if (dec == ks::kPlaceNone) {
            out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cand};
            r.not_found++;
            if (r.first_unplaced < 0) r.first_unplaced = i;
            continue;
        }
        const uint32_t X = ks::place_key_node(W);
        const bool from_d = W == D;
        const bool fresh = from_d && !(ablate & 1) && ks::scaleup_takes_fresh(X, n, u, s.max_nodes);
        int32_t idx;
        if (from_d) {
            idx = d_idx;
            if (fresh) {
                chg.push_back(Chg{(int32_t)X, s.tmpl});
                ++u;
                stats[0]++;
            } else {
                stats[1]++;
            }
        } else {
            idx = (int32_t)chg.size();
            chg.push_back(Chg{(int32_t)X, s.node[X]});
            for (size_t e = 0; e < top.size(); e++)
                if (top[e] && ks::place_key_node(top[e]) == X) flag[e / L] |= 1u << (e % L);
        }
        const ks::NodeV before = chg[idx].v;
        ks::NodeV aft = before;
        const int32_t st = ks::place_bind(p, aft);
        if (st == ks::kPlaceOk) {
            for (int32_t j = 0; j < n_shapes; j++) cc[j] += ks::place_cand_delta(s.c, s.shapes[j], before, aft);
            chg[idx].v = aft;
            r.ok++;
            r.on_new += X >= (uint32_t)n;
        } else {
            r.over_capacity++;
            if (r.first_unplaced < 0) r.first_unplaced = i;
        }
        out[i] = ks::Placement{(int32_t)X, st, (int64_t)(W >> 32) - 1, cand};
    }
    if ((int64_t)chg.size() > ks::kPlaceMaxPods) return -2;
    // the prefix invariant, checked on the final changed set
    int32_t seen = 0;
    for (const Chg& c : chg)
        if (c.node >= n) {
            if (c.node != n + seen) return -3;
            ++seen;
            r.nodes_used += c.v.nr > 0;
        }
    if (seen != u) return -3;
    stats[3] = (int64_t)chg.size();
    std::memcpy(res, &r, sizeof(r));
    return i;
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
