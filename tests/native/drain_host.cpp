// Host build of the drain preview's host-side pieces (ks_query.h: drain_segment, drain_rank,
// drain_below, drain_cordoned and the placement functions), for CPU tests only.
//   ks_host_drain_segments   ks_drain_at's segment walk over a sequence of pod records;
//   ks_host_drain_ranks      a serial restatement of the gather (ks_drain.hip): per 256-pod block
//                            and 64-lane wave the ballot and its count, the block counts, their
//                            exclusive scan in chunks of 256 with a carry, and every selected pod's
//                            rank from drain_rank;
//   ks_host_drain_place      the rounds of place_serial.h with the cordon in the scan (key 0 for a
//                            cordoned node) and a veto on a cordoned winner, and
//                            ks_host_drain_place_brute, the plain sequential argmax over the nodes
//                            that are not cordoned.
// Not part of the product.
#include "place_serial.h"

using namespace place_serial;

#define CASE_ARGS CLUSTER_ARGS, int32_t k, const int32_t *shape_of, const uint32_t *cordon
#define CASE_PASS CLUSTER_PASS, cordon

// a drained node's rows are emptied
static Cluster make_case(CLUSTER_ARGS, const uint32_t* cordon) {
    Cluster s = make_cluster(CLUSTER_PASS);
    for (int32_t i = 0; i < n; i++)
        if (ks::drain_cordoned(cordon, i)) s.node[i].rc = s.node[i].rm = s.node[i].rg = s.node[i].nr = 0;
    return s;
}

static void finish(const Cluster& s, int32_t k, const ks::Placement* out, int64_t* after, int64_t* info) {
    state_out(s, after);
    tally(out, k, info);
}

// scheduleOne as written, over the nodes that remain
extern "C" int ks_host_drain_place_brute(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info) {
    Cluster s = make_case(CASE_PASS);
    for (int32_t i = 0; i < k; i++) {
        const ks::PodRec& p = s.shapes[shape_of[i]];
        uint64_t best = 0;
        int64_t cand = 0;
        for (int32_t nd = 0; nd < n; nd++) {
            if (cordon[nd / 32] >> (nd % 32) & 1u) continue;
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

// the rounds; info[0] = rounds; -1: a round decided no pod; -2: the changed set overflowed; -3: a
// cordoned node reached the resolver
extern "C" int ks_host_drain_place(CASE_ARGS, ks::Placement* out, int64_t* after, int64_t* info) {
    Cluster s = make_case(CASE_PASS);
    struct Cordon : Hooks {
        const uint32_t* cordon;
        int veto(uint32_t X) const { return ks::drain_cordoned(cordon, (int32_t)X) ? -3 : 0; }
    } h{{}, cordon};
    // the scan's key: 0 for a cordoned node (place_scan_kernel<true>)
    const auto key = [&](const ks::PodRec& p, int32_t nd) {
        return ks::drain_cordoned(cordon, nd) ? 0ull : ks::place_key(s.c, p, s.node[nd], (uint32_t)nd);
    };
    if (int rc = run_rounds(s, shape_of, k, key, h, out, info, nullptr); rc != 0) return rc;
    finish(s, k, out, after, info);
    return 0;
}

// ks_drain_at's segment walk: seg_end[s] (exclusive) and seg_shapes[s] per segment, shape_of[n] per pod
// (its index among its segment's shapes), the shapes' first pods in first_pod[segment * 64 + shape].
// Returns the number of segments, -1 when more than seg_cap or a segment is empty.
extern "C" int64_t ks_host_drain_segments(int64_t n, const int64_t* req, const uint32_t* keymask, const uint64_t* tol,
                                          const uint64_t* sel, const uint32_t* flags, int64_t seg_cap, int64_t* seg_end,
                                          int32_t* seg_shapes, int32_t* shape_of, ks::PodRec* shapes_out) {
    std::vector<ks::PodRec> recs(n);
    for (int64_t i = 0; i < n; i++) {
        recs[i] = ks::PodRec{};
        for (int c = 0; c < 3; c++) recs[i].req[c] = req[i * 3 + c];  // unmasked words as given
        recs[i].tol = tol[i]; recs[i].sel = sel[i]; recs[i].keymask = keymask[i]; recs[i].flags = flags[i];
    }
    int64_t ns = 0;
    for (int64_t start = 0; start < n;) {
        if (ns >= seg_cap) return -1;
        int32_t m = 0;
        const int64_t end = ks::drain_segment(recs.data(), n, start, shapes_out + ns * ks::kPlaceMaxShapes, &m,
                                              shape_of + start);
        if (end <= start) return -1;
        seg_end[ns] = end;
        seg_shapes[ns] = m;
        ns++;
        start = end;
    }
    return ns;
}

// The gather over nblocks blocks of 256 pods, sel[nblocks * 256] the predicate: rank[q] for a
// selected pod (-1 otherwise); returns the total the scan leaves.
extern "C" int64_t ks_host_drain_ranks(int64_t nblocks, const uint8_t* sel, int64_t* rank) {
    constexpr int kWaves = ks::kDrainBlk / ks::kWave;
    std::vector<int32_t> bcnt(nblocks), boff(nblocks), wcnt((size_t)nblocks * kWaves);
    std::vector<uint64_t> ballot((size_t)nblocks * kWaves);
    // drain_count_kernel
    for (int64_t b = 0; b < nblocks; b++) {
        int32_t sum = 0;
        for (int w = 0; w < kWaves; w++) {
            uint64_t m = 0;
            for (int l = 0; l < ks::kWave; l++) m |= (uint64_t)(sel[b * ks::kDrainBlk + w * ks::kWave + l] != 0) << l;
            ballot[b * kWaves + w] = m;
            wcnt[b * kWaves + w] = __builtin_popcountll(m);
            sum += wcnt[b * kWaves + w];
        }
        bcnt[b] = sum;
    }
    // drain_scan_kernel: chunks of 256 counts, an inclusive Hillis-Steele scan each, a carry between them
    long long carry = 0;
    for (int64_t base = 0; base < nblocks; base += ks::kDrainBlk) {
        int32_t buf[2][ks::kDrainBlk];
        int cur = 0;
        for (int t = 0; t < ks::kDrainBlk; t++) buf[0][t] = base + t < nblocks ? bcnt[base + t] : 0;
        for (int o = 1; o < ks::kDrainBlk; o <<= 1) {
            for (int t = 0; t < ks::kDrainBlk; t++) buf[cur ^ 1][t] = buf[cur][t] + (t >= o ? buf[cur][t - o] : 0);
            cur ^= 1;
        }
        for (int t = 0; t < ks::kDrainBlk && base + t < nblocks; t++)
            boff[base + t] = (int32_t)(carry + buf[cur][t] - bcnt[base + t]);
        carry += buf[cur][ks::kDrainBlk - 1];
    }
    // drain_fill_kernel
    for (int64_t b = 0; b < nblocks; b++)
        for (int w = 0; w < kWaves; w++)
            for (int l = 0; l < ks::kWave; l++) {
                const int64_t q = b * ks::kDrainBlk + w * ks::kWave + l;
                rank[q] = sel[q] ? ks::drain_rank(boff[b], &wcnt[b * kWaves], w, ballot[b * kWaves + w], l) : -1;
            }
    return carry;
}

extern "C" int ks_host_drain_limits(int32_t* out) {
    out[0] = ks::kPlaceMaxShapes; out[1] = ks::kPlaceMaxPods; out[2] = ks::kDrainBlk; out[3] = L;
    out[4] = (int32_t)sizeof(ks::Eviction); out[5] = (int32_t)ks::kDrainMaxPods;
    return 0;
}
