// ks_gang.hip — gang admission preview: a queue of pod groups admitted all-or-nothing (or from
// min_ok members up) one after another at a past tick, each attempt a transaction on one private
// state (gfx950, wave64).
//
// ks_gang_at walks m gangs in the caller's order the way a coscheduling queue does: a gang's pods go
// to scheduleOne one after another (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60); a gang
// with at least min_ok pods bound Ok is admitted and its placements stay, any other attempt is
// rolled back.  A round is
//   place_scan_kernel + place_merge_kernel (launch_place_lists, ks_place.hip) on the committed
//                              scratch state, no cordon;
//   resolve_kernel<false, false, true> (ks_place_resolve.h) one workgroup walks the round's gangs with
//                              the placement rounds' pod loop inside a transaction per gang, commits
//                              the kept placements and reports the next gang.
// The argument is in ks_query.h, above gang_route.  A gang with more pods than one set of lists
// decides is the host's: the drain preview's segmented rounds on a copy of the state.
#include "ks_query.h"
#include "ks_place_resolve.h"

namespace ks {

hipError_t launch_gang_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const GangRound& gr, hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.k < 0 || pc.k > kPlaceMaxPods || pc.n_shapes < 0 || pc.n_shapes > kPlaceMaxShapes ||
        (pc.k > 0) != (pc.n_shapes > 0) || gr.g0 < 0 || gr.g1 <= gr.g0 || gr.g1 > gr.m || !gr.gangs || !gr.out)
        return hipErrorInvalidValue;
    const uint64_t active = pc.n_shapes >= 64 ? ~0ull : (1ull << pc.n_shapes) - 1ull;
    if (pc.n_shapes)
        if (hipError_t r = launch_place_lists(s, pc, b, active, st); r != hipSuccess) return r;
    hipLaunchKernelGGL((resolve_kernel<false, false, true>), dim3(1), dim3(kPRes), 0, st, s, b.state, b.n_pad, pc, b.shapes,
                       b.shape_of, (const uint64_t*)b.top, (const long long*)b.ccount, (const ScaleOption*)nullptr, b.out,
                       (ScaleResult*)nullptr, 0, active, b.rb, gr);
    return hipGetLastError();
}

}  // namespace ks
