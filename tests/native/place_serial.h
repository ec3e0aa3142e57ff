// The one serial restatement of the previews' resolver (ks_place.hip: the scan, the merge and
// resolve_kernel's pod loop), shared by place_host.cpp, drain_host.cpp, removable_host.cpp and
// scaleup_host.cpp, for CPU tests only: the case a test hands over, the list builder, the pod loop
// over a changed set, and the rounds around both.  Everything that decides is ks_query.h's own
// source (place_key, topl_insert, place_first_unchanged, place_decide, place_bind,
// place_cand_delta).  Not part of the product.
// The tests' libraries are rebuilt when their .cpp, ks_device.h, ks_query.h or ks_carve.h is newer
// than the library; this header is not in that list, so after an edit here alone touch the four .cpp files
// (or remove tests/native/libks_host*.so) before running tests/test_*_host.py.
#pragma once
#include <algorithm>
#include <vector>

#include "../../kubernetes-simulator_amd/csrc/ks_query.h"

namespace place_serial {

constexpr int L = ks::kPlaceL;
constexpr int kBlk = 256;

struct Cluster {
    int32_t n;
    std::vector<ks::NodeV> node;  // the call's units
    ks::Cfg c{};
    std::vector<ks::PodRec> shapes;
};

#define CLUSTER_ARGS                                                                                               \
    int32_t n, const int64_t *alloc_dev, const int64_t *scale, const int64_t *state_m, const uint64_t *taint,     \
        const uint64_t *label, const int32_t *cfg, int32_t n_shapes, const int64_t *req, const uint32_t *keymask,   \
        const uint64_t *tol, const uint64_t *sel
#define CLUSTER_PASS n, alloc_dev, scale, state_m, taint, label, cfg, n_shapes, req, keymask, tol, sel

// cfg[6]: filter_feeds, filters, has_scorers, w_lr, w_ba, const_total
inline Cluster make_cluster(CLUSTER_ARGS) {
    Cluster s;
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
    return s;
}

// after[n][4]: the nodes' rc rm rg nr
inline void state_out(const Cluster& s, int64_t* after) {
    for (int32_t i = 0; i < s.n; i++) {
        after[i * 4 + 0] = s.node[i].rc; after[i * 4 + 1] = s.node[i].rm; after[i * 4 + 2] = s.node[i].rg;
        after[i * 4 + 3] = s.node[i].nr;
    }
}

// info[1..3]: pods bound Ok, bound OverCapacity, not found
inline void tally(const ks::Placement* out, int32_t k, int64_t* info) {
    info[1] = info[2] = info[3] = 0;
    for (int32_t i = 0; i < k; i++) info[out[i].status == ks::kPlaceOk ? 1 : out[i].status == ks::kPlaceOverCapacity ? 2 : 3]++;
}

// the scan's key of node nd for shape p: the cluster as it is
inline auto node_key(const Cluster& s) {
    return [&s](const ks::PodRec& p, int32_t nd) { return ks::place_key(s.c, p, s.node[nd], (uint32_t)nd); };
}

// Per shape the snapshot list, its length, its flags (bit e: entry e's node is in the changed set)
// and the running candidate count: plain data, a caller may preset flags and counts before the loop.
struct Lists {
    std::vector<uint64_t> top;
    std::vector<uint32_t> flag;
    std::vector<int> len;
    std::vector<long long> cc;
};

// (a) place_scan_kernel + place_merge_kernel: per 256-node block the exact top-L keys and the count
// of non-zero keys, merged by topl_insert; the shapes outside `active` (null: none) keep empty lists.
template <class Key>
Lists build_lists(const Cluster& s, const uint64_t* active, Key key) {
    const int32_t n_shapes = (int32_t)s.shapes.size(), nblk = (s.n + kBlk - 1) / kBlk;
    Lists l{std::vector<uint64_t>((size_t)n_shapes * L, 0ull), std::vector<uint32_t>(n_shapes, 0u), std::vector<int>(n_shapes, 0),
            std::vector<long long>(n_shapes, 0)};
    for (int32_t j = 0; j < n_shapes; j++) {
        if (active && !(*active >> j & 1)) continue;
        uint64_t t[L] = {};
        for (int32_t b = 0; b < nblk; b++) {
            std::vector<uint64_t> keys;
            for (int32_t nd = b * kBlk; nd < std::min(s.n, (b + 1) * kBlk); nd++) keys.push_back(key(s.shapes[j], nd));
            std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b2) { return a > b2; });
            uint64_t lv[L] = {};
            for (int e = 0; e < L && e < (int)keys.size(); e++) lv[e] = keys[e];
            for (uint64_t x : keys) l.cc[j] += x != 0;
            ks::topl_insert<L>(t, lv);
        }
        std::copy(t, t + L, l.top.begin() + (size_t)j * L);
        l.len[j] = ks::place_list_len<L>(t);
    }
    return l;
}

struct Chg {
    int32_t node;
    ks::NodeV v;
};

// What a preview adds to the loop; these are the placement preview's: nothing.
struct Hooks {
    // an extra candidate on D's side: its key for pod p (0: none) ...
    uint64_t extra_key(const ks::PodRec&) const { return 0ull; }
    // ... and, when the winner X came from D's side, whether X is that candidate: then *v joins the changed set
    bool extra_joins(uint32_t, ks::NodeV*) { return false; }
    // a winner the preview must never see: a non-zero code ends the loop
    int veto(uint32_t) const { return 0; }
};

struct Run {
    int32_t next;            // the first undecided pod: k, or the pod that met kPlaceStop or a veto
    int veto = 0;            // the hook's code
    bool stopped = false;    // kPlaceStop
    int64_t from_changed = 0, from_extra = 0;  // pods won on D's side: by a changed node, by the extra candidate
    int64_t most_flagged = 0;                  // the most flagged entries a pod found in its list
};

// (b) resolve_kernel's pod loop, serially, over pods [first, k): D over the changed set (and the hook's
// extra candidate), S, place_decide, the winner's entries flagged, place_bind, the counts moved.
template <class H>
Run decide_pods(const Cluster& s, Lists& l, const int32_t* shape_of, int32_t first, int32_t k, std::vector<Chg>& chg, H& h,
                ks::Placement* out) {
    Run r{first};
    const int32_t n_shapes = (int32_t)s.shapes.size();
    for (int32_t& i = r.next; i < k; i++) {
        const int sh = shape_of[i];
        const ks::PodRec& p = s.shapes[sh];
        uint64_t D = 0;
        int32_t d_idx = -1;
        for (size_t c = 0; c < chg.size(); c++) {
            const uint64_t key = ks::place_key(s.c, p, chg[c].v, (uint32_t)chg[c].node);
            if (key > D) { D = key; d_idx = (int32_t)c; }
        }
        const uint64_t F = h.extra_key(p);
        if (F > D) { D = F; d_idx = (int32_t)chg.size(); }  // (the slot it takes if it wins)
        const uint64_t* list = &l.top[(size_t)sh * L];
        r.most_flagged = std::max<int64_t>(r.most_flagged, __builtin_popcount(l.flag[sh]));
        const int eS = ks::place_first_unchanged<L>(l.len[sh], l.flag[sh]);
        const uint64_t S = eS < L ? list[eS] : 0ull;
        uint64_t W;
        const int dec = ks::place_decide(S, list[L - 1], D, &W);
        if (dec == ks::kPlaceStop) {
            r.stopped = true;
            break;
        }
        const long long cand = l.cc[sh];
        if (dec == ks::kPlaceNone) {
            out[i] = ks::Placement{-1, ks::kPlaceNotFound, -1, cand};
            continue;
        }
        const uint32_t X = ks::place_key_node(W);
        if ((r.veto = h.veto(X)) != 0) break;
        int32_t idx;
        ks::NodeV joins{};
        if (W == D) {
            idx = d_idx;
            if (h.extra_joins(X, &joins)) {
                chg.push_back(Chg{(int32_t)X, joins});
                r.from_extra++;
            } else {
                r.from_changed++;
            }
        } else {
            idx = (int32_t)chg.size();
            chg.push_back(Chg{(int32_t)X, s.node[X]});
            for (size_t e = 0; e < l.top.size(); e++)
                if (l.top[e] && ks::place_key_node(l.top[e]) == X) l.flag[e / L] |= 1u << (e % L);
        }
        const ks::NodeV before = chg[idx].v;
        ks::NodeV aft = before;
        const int32_t st = ks::place_bind(p, aft);
        if (st == ks::kPlaceOk) {
            for (int32_t j = 0; j < n_shapes; j++) l.cc[j] += ks::place_cand_delta(s.c, s.shapes[j], before, aft);
            chg[idx].v = aft;
        }
        out[i] = ks::Placement{(int32_t)X, st, (int64_t)(W >> 32) - 1, cand};
    }
    return r;
}

// ks_place_at's rounds (place_rounds, ks_previews.cpp): lists for the shapes still to be placed, the
// loop, the commit, again from the first undecided pod.  info[0] = rounds; stats (null: none)[0]:
// pods decided from a changed node, [1]: the largest changed set of a round.  Returns 0, -1: a round
// decided no pod, -2: the changed set overflowed, or the hook's veto.
template <class Key, class H>
int run_rounds(Cluster& s, const int32_t* shape_of, int32_t k, Key key, H& h, ks::Placement* out, int64_t* info,
               int64_t* stats) {
    info[0] = 0;
    for (int32_t first = 0; first < k; info[0]++) {
        uint64_t active = 0;
        for (int32_t i = first; i < k; i++) active |= 1ull << shape_of[i];
        Lists l = build_lists(s, &active, key);
        std::vector<Chg> chg;
        const Run r = decide_pods(s, l, shape_of, first, k, chg, h, out);
        if (r.veto) return r.veto;
        if ((int64_t)chg.size() > ks::kPlaceMaxPods) return -2;
        if (stats) {
            stats[0] += r.from_changed;
            stats[1] = std::max<int64_t>(stats[1], (int64_t)chg.size());
        }
        for (const Chg& c : chg) s.node[c.node] = c.v;  // commit
        if (r.next == first) return -1;
        first = r.next;
    }
    return 0;
}

}  // namespace place_serial
