// Host build of the placement preview's decision and bookkeeping functions (ks_query.h:
// place_key, place_first_unchanged, place_decide, place_bind, place_cand_delta, topl_insert), for
// CPU tests only.  ks_host_place runs the whole rounds algorithm of ks_place.hip serially — the
// shared restatement of place_serial.h with no hook: lists, pod loop, commit, rescan for the
// remaining shapes — with the same source the kernels inline; ks_host_place_brute is the plain
// sequential argmax over all nodes it must equal.  Not part of the product.
#include "place_serial.h"

using namespace place_serial;

#define CASE_ARGS CLUSTER_ARGS, int32_t k, const int32_t *shape_of
#define CASE_PASS CLUSTER_PASS, k, shape_of

static void finish(const Cluster& s, int32_t k, const ks::Placement* out, int64_t* after, int64_t* info) {
    state_out(s, after);
    tally(out, k, info);
}

// the sequential argmax over all nodes: scheduleOne as written
extern "C" int ks_host_place_brute(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info) {
    Cluster s = make_cluster(CLUSTER_PASS);
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
    finish(s, k, out, after, info);
    return 0;
}

// the rounds algorithm; info[0] = rounds; -1: a round decided no pod; stats[0]: pods decided from a
// changed node (D), stats[1]: the largest changed set of a round
static int rounds(Cluster& s, int32_t k, const int32_t* shape_of, ks::Placement* out, int64_t* info, int64_t* stats) {
    stats[0] = stats[1] = 0;
    Hooks none;
    return run_rounds(s, shape_of, k, node_key(s), none, out, info, stats);
}

extern "C" int ks_host_place(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info, int64_t* stats) {
    Cluster s = make_cluster(CLUSTER_PASS);
    if (int rc = rounds(s, k, shape_of, out, info, stats); rc != 0) return rc;
    finish(s, k, out, after, info);
    return 0;
}

// As ks_place_at chooses: when every masked request is a whole multiple of the unit
// (place_whole_units) the rounds run in device units — alloc as given, state_m and the requests
// divided by the scale, `after` multiplied back.  stats[2] = 1 when they did.  state_m must hold
// whole units then (the engine's state always does).
extern "C" int ks_host_place_units(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info, int64_t* stats) {
    const Cluster m = make_cluster(CLUSTER_PASS);
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
    Cluster s = make_cluster(n, alloc_dev, one, st.data(), taint, label, cfg, n_shapes, rq.data(), keymask, tol, sel);
    if (int rc = rounds(s, k, shape_of, out, info, stats); rc != 0) return rc;
    finish(s, k, out, after, info);
    for (int32_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) after[i * 4 + c] *= scale[c];
    return 0;
}

extern "C" int ks_host_place_l() { return L; }
