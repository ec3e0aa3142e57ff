// ks_removable.hip — removal scan: which candidate nodes could each be drained alone at a past tick
// (gfx950, wave64).
//
// ks_removable_at asks ks_drain_at's question for m candidate nodes, each on its own: would every pod
// running on the node be re-bound Ok once the node has left k.nodes (kubesim/kubesim.go:168-206)?
// Every candidate starts from the same state at t, so the cluster is scanned once per segment of at
// most 64 distinct shapes on the un-cordoned base state (launch_place_lists, ks_place.hip) and
//   removable_resolve_kernel   one wave per candidate decides its pods in FIFO order from those lists:
//                              the candidate's own entries flagged from the start, its running counts
//                              corrected for its own node (the argument is in ks_query.h, above
//                              removable_route), its changed set private in LDS.
// Integers only, no atomics, no communication between workgroups; nothing is written but the
// candidate's own rows and its summary, so the scratch state stays the base state for every segment.
#include "ks_query.h"

namespace ks {
namespace {

// Lane j holds shape j of the segment: its record, the nodes of its list's entries, its flag word,
// its list length and its running candidate count, all in registers.  Lane c < nchg evaluates
// changed node c for D.  What a pod needs of its own shape is broadcast from that shape's lane.
//
// Per pod (uniform control flow, two barriers of a one-wave workgroup):
//   D = the wave max of the lanes' keys on the changed nodes; S from the pod's shape's flags;
//   place_decide; a winner from the list loads its record from the base scratch and joins the changed
//   set, and every lane flags its own list's entries on that node; a winner from D is the slot of the
//   lane whose key is D; place_bind; the lanes adjust their counts by place_cand_delta;
//   (A) every lane has read the changed set; lane 0 writes the slot's new state and the pod's row;
//   (B) the next pod reads it.
// All loops are bounded by the candidate's pods (<= kRemovableMaxPods), L and 64.
__global__ __launch_bounds__(kWave) void removable_resolve_kernel(NodeSoA s, const int64_t* __restrict__ state,
                                                                  int64_t n_pad, PlaceCfg pc,
                                                                  const PodRec* __restrict__ shapes,
                                                                  const int32_t* __restrict__ shape_of,
                                                                  const RemovalCand* __restrict__ cands,
                                                                  const uint64_t* __restrict__ top,
                                                                  const long long* __restrict__ ccount,
                                                                  const long long* __restrict__ ev_pod,
                                                                  const int32_t* __restrict__ perm,
                                                                  Eviction* __restrict__ rows,
                                                                  Removal* __restrict__ out) {
    __shared__ NodeV chg[kRemovableMaxPods];
    __shared__ int32_t chg_node[kRemovableMaxPods];
    const int lane = threadIdx.x;
    const RemovalCand cd = cands[blockIdx.x];
    const int32_t count = cd.count < kRemovableMaxPods ? cd.count : kRemovableMaxPods;  // (the host routes by the same bound)
    const bool on = lane < pc.n_shapes;

    // ---- this lane's shape: record, list, flags with the candidate's own entries set, count ----
    const PodRec mine = on ? shapes[lane] : PodRec{};
    uint32_t enode[kPlaceL];
    int32_t len = 0;
    uint32_t flag = 0u;
#pragma unroll
    for (int e = 0; e < kPlaceL; ++e) {
        const uint64_t key = on ? top[lane * kPlaceL + e] : 0ull;
        enode[e] = place_key_node(key);  // (key 0: 0xFFFFFFFF, no node's index)
        len += key != 0;
        if (key && enode[e] == (uint32_t)cd.node) flag |= 1u << e;
    }
    const NodeV own = place_load(s, state, n_pad, pc.sc, cd.node);
    long long cc = on ? ccount[lane] - (long long)place_is_cand(pc.c, mine, own) : 0;

    int32_t nchg = 0, n_ok = 0, n_over = 0, n_nf = 0;
    bool stopped = false;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t row = cd.first + i;
        const int sh = shape_of[row] & (kPlaceMaxShapes - 1);
        const PodRec p = shapes[sh];
        uint64_t dk = 0ull;
        if (lane < nchg) dk = place_key(pc.c, p, chg[lane], (uint32_t)chg_node[lane]);
        const uint64_t D = wave_max_u64(dk);
        const uint32_t fl = (uint32_t)__shfl((int)flag, sh, kWave);
        const int ln = __shfl(len, sh, kWave);
        const long long cand = __shfl(cc, sh, kWave);
        const int eS = place_first_unchanged<kPlaceL>(ln, fl);
        const uint64_t S = eS < kPlaceL ? top[sh * kPlaceL + eS] : 0ull;
        uint64_t W;
        const int dec = place_decide(S, top[sh * kPlaceL + kPlaceL - 1], D, &W);
        if (dec == kPlaceStop) {  // (cannot happen with count <= L - 1: reported, never guessed)
            stopped = true;
            break;
        }
        if (dec == kPlaceNone) {
            if (lane == 0) rows[row] = Eviction{ev_pod[perm[row]], cd.node, -1, kPlaceNotFound, 0, -1, cand};
            ++n_nf;
            continue;
        }
        const uint32_t X = place_key_node(W);
        const bool from_d = W == D;  // S and D are keys of different nodes: never equal
        int32_t idx;
        NodeV before;
        if (from_d) {
            idx = __ffsll((unsigned long long)__ballot(lane < nchg && dk == W)) - 1;
            before = chg[idx];
        } else {
            idx = nchg;
            before = place_load(s, state, n_pad, pc.sc, X);
#pragma unroll
            for (int e = 0; e < kPlaceL; ++e)
                if (enode[e] == X) flag |= 1u << e;
        }
        NodeV after = before;
        const int32_t status = place_bind(p, after);
        if (status == kPlaceOk && on) cc += place_cand_delta(pc.c, mine, before, after);
        __syncthreads();  // (A)
        if (lane == 0) {
            chg[idx] = after;  // (OverCapacity: after == before)
            chg_node[idx] = (int32_t)X;
            rows[row] = Eviction{ev_pod[perm[row]], cd.node, (int32_t)X, status, 0, (int64_t)(W >> 32) - 1, cand};
        }
        __syncthreads();  // (B)
        if (!from_d) ++nchg;
        if (status == kPlaceOk) ++n_ok; else ++n_over;
    }
    if (lane == 0)
        out[blockIdx.x] = Removal{cd.node, cd.count, n_ok, n_over, n_nf,
                                  stopped || count != cd.count ? -1 : (int32_t)(n_ok == cd.count), cd.first};
}

}  // namespace

hipError_t launch_removable_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const RemovableBufs& r,
                                    const PodRec* shapes, int64_t cand0, int64_t n_cand, hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.n_shapes <= 0 || pc.n_shapes > kPlaceMaxShapes || cand0 < 0 || n_cand <= 0 ||
        n_cand > 0x7FFFFFFF)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(removable_resolve_kernel, dim3((unsigned)n_cand), dim3(kWave), 0, st, s, (const int64_t*)b.state,
                       b.n_pad, pc, shapes, r.shape_of, r.cands + cand0, (const uint64_t*)b.top,
                       (const long long*)b.ccount, r.ev_pod, r.perm, r.rows, r.out + cand0);
    return hipGetLastError();
}

}  // namespace ks
