// Host build of the placement preview's decision and bookkeeping functions (ks_device.h:
// place_key, place_first_unchanged, place_decide, place_bind, place_cand_delta, topl_insert), for
// CPU tests only.  ks_host_place runs the whole rounds algorithm of ks_place.hip serially — per
// 256-node block the exact top-L list and the candidate count, the topl_insert merge, the resolver's
// pod loop over the snapshot lists and the changed set, the commit, the rescan for the remaining
// shapes — with the same source the kernels inline; ks_host_place_brute is the plain sequential
// argmax over all nodes it must equal.  Not part of the product.
#include <algorithm>
#include <vector>

#include "../../kubernetes-simulator_amd/csrc/ks_device.h"

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
};

// cfg[6]: filter_feeds, filters, has_scorers, w_lr, w_ba, const_total
Case make_case(int32_t n, const int64_t* alloc_dev, const int64_t* scale, const int64_t* state_m, const uint64_t* taint,
               const uint64_t* label, const int32_t* cfg, int32_t n_shapes, const int64_t* req, const uint32_t* keymask,
               const uint64_t* tol, const uint64_t* sel, int32_t k, const int32_t* shape_of) {
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
            if (keymask[j] >> c & 1) p.req[c] = req[j * 3 + c];  // unmasked keys are ignored (ks_queries.cpp head_shapes)
        p.tol = tol[j]; p.sel = sel[j]; p.keymask = keymask[j];
        s.shapes.push_back(p);
    }
    s.k = k;
    s.shape_of = shape_of;
    return s;
}

void finish(const Case& s, const ks::Placement* out, int64_t* after, int64_t* info) {
    for (int32_t i = 0; i < s.n; i++) {
        after[i * 4 + 0] = s.node[i].rc; after[i * 4 + 1] = s.node[i].rm; after[i * 4 + 2] = s.node[i].rg;
        after[i * 4 + 3] = s.node[i].nr;
    }
    info[1] = info[2] = info[3] = 0;
    for (int32_t i = 0; i < s.k; i++)
        info[out[i].status == ks::kPlaceOk ? 1 : out[i].status == ks::kPlaceOverCapacity ? 2 : 3]++;
}

}  // namespace

#define CASE_ARGS                                                                                                  \
    int32_t n, const int64_t *alloc_dev, const int64_t *scale, const int64_t *state_m, const uint64_t *taint,     \
        const uint64_t *label, const int32_t *cfg, int32_t n_shapes, const int64_t *req, const uint32_t *keymask,   \
        const uint64_t *tol, const uint64_t *sel, int32_t k, const int32_t *shape_of
#define CASE_PASS n, alloc_dev, scale, state_m, taint, label, cfg, n_shapes, req, keymask, tol, sel, k, shape_of

// the sequential argmax over all nodes: scheduleOne as written
extern "C" int ks_host_place_brute(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info) {
    Case s = make_case(CASE_PASS);
    for (int32_t i = 0; i < k; i++) {
        const ks::PodRec& p = s.shapes[shape_of[i]];
        uint64_t best = 0;
        int64_t cand = 0;
        for (int32_t nd = 0; nd < n; nd++) {
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
    info[0] = 0;
    finish(s, out, after, info);
    return 0;
}

// the rounds algorithm; info[0] = rounds; -1: a round decided no pod; stats[0]: pods decided from a
// changed node (D), stats[1]: the largest changed set of a round
static int run_rounds(Case& s, ks::Placement* out, int64_t* info, int64_t* stats) {
    const int32_t n = s.n, k = s.k, n_shapes = (int32_t)s.shapes.size();
    const int32_t* shape_of = s.shape_of;
    const int32_t nblk = (n + kBlk - 1) / kBlk;
    int32_t first = 0;
    info[0] = 0;
    stats[0] = stats[1] = 0;
    struct Chg { int32_t node; ks::NodeV v; };
    while (first < k) {
        uint64_t active = 0;
        for (int32_t i = first; i < k; i++) active |= 1ull << shape_of[i];
        // scan + merge
        std::vector<uint64_t> top((size_t)n_shapes * L, 0ull);
        std::vector<uint32_t> flag(n_shapes, 0u);
        std::vector<int> len(n_shapes, 0);
        std::vector<int64_t> cc(n_shapes, 0);
        for (int32_t j = 0; j < n_shapes; j++) {
            if (!(active >> j & 1)) continue;
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
        }
        // resolve
        std::vector<Chg> chg;
        int32_t i = first;
        for (; i < k; i++) {
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
            if (dec == ks::kPlaceStop) break;
            const int64_t cand = cc[sh];
            if (dec == ks::kPlaceNone) {
                out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cand};
                continue;
            }
            const uint32_t X = ks::place_key_node(W);
            int32_t idx;
            if (W == D) {
                idx = d_idx;
                stats[0]++;
            } else {
                idx = (int32_t)chg.size();
                chg.push_back(Chg{(int32_t)X, s.node[X]});
                for (size_t e = 0; e < top.size(); e++)
                    if (top[e] && ks::place_key_node(top[e]) == X) flag[e / L] |= 1u << (e % L);
            }
            const ks::NodeV before = chg[idx].v;
            ks::NodeV aft = before;
            const int32_t st = ks::place_bind(p, aft);
            if (st == ks::kPlaceOk)
                for (int32_t j = 0; j < n_shapes; j++) cc[j] += ks::place_cand_delta(s.c, s.shapes[j], before, aft);
            out[i] = ks::Placement{(int32_t)X, st, (int64_t)(W >> 32) - 1, cand};
            if (st == ks::kPlaceOk) chg[idx].v = aft;
        }
        if ((int64_t)chg.size() > ks::kPlaceMaxPods) return -2;
        stats[1] = std::max<int64_t>(stats[1], (int64_t)chg.size());
        for (const Chg& c : chg) s.node[c.node] = c.v;  // commit
        if (i == first) return -1;
        first = i;
        info[0]++;
    }
    return 0;
}

extern "C" int ks_host_place(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info, int64_t* stats) {
    Case s = make_case(CASE_PASS);
    if (int rc = run_rounds(s, out, info, stats); rc != 0) return rc;
    finish(s, out, after, info);
    return 0;
}

// As ks_place_at chooses: when every masked request is a whole multiple of the unit
// (place_whole_units) the rounds run in device units — alloc as given, state_m and the requests
// divided by the scale, `after` multiplied back.  stats[2] = 1 when they did.  state_m must hold
// whole units then (the engine's state always does).
extern "C" int ks_host_place_units(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info, int64_t* stats) {
    Case m = make_case(CASE_PASS);
    const ks::QScale sc{{scale[0], scale[1], scale[2]}};
    stats[2] = ks::place_whole_units(m.shapes.data(), n_shapes, sc) ? 1 : 0;
    if (!stats[2]) return ks_host_place(CASE_PASS, out, after, info, stats);
    const int64_t one[3] = {1, 1, 1};
    std::vector<int64_t> st(state_m, state_m + (size_t)n * 4), rq(req, req + (size_t)n_shapes * 3);
    for (int32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) {
            if (st[i * 4 + c] % scale[c]) return -3;
            st[i * 4 + c] /= scale[c];
        }
    for (int32_t j = 0; j < n_shapes; j++)
        for (int c = 0; c < 3; c++)
            if (keymask[j] >> c & 1) rq[j * 3 + c] /= scale[c];
    Case s = make_case(n, alloc_dev, one, st.data(), taint, label, cfg, n_shapes, rq.data(), keymask, tol, sel, k, shape_of);
    if (int rc = run_rounds(s, out, info, stats); rc != 0) return rc;
    finish(s, out, after, info);
    for (int32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) after[i * 4 + c] *= scale[c];
    return 0;
}

extern "C" int ks_host_place_l() { return L; }
