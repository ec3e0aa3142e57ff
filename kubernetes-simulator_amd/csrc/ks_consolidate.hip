// ks_consolidate.hip — consolidation preview: a chain of candidate nodes removed one after another
// at a past tick, each attempt a transaction on one private state (gfx950, wave64).
//
// ks_consolidate_at walks m candidates in the caller's order the way a scale-down pass does
// (kubesim/kubesim.go:168-206 range over k.nodes without the removed nodes; scheduleOne,
// kubesim.go:143-225, kubesim/node/node.go:36-60, re-places a candidate's pods): a candidate whose
// pods are all re-bound Ok is removed and its placements stay, any other attempt is rolled back, and
// a node that received a moved pod is not tried.  A round is
//   place_scan_kernel<true> + place_merge_kernel (launch_place_lists, ks_place.hip) on the committed
//                              scratch state with the removed nodes cordoned;
//   resolve_kernel<false, true> (ks_place_resolve.h) one workgroup walks the round's candidates with the
//                              placement rounds' pod loop inside a transaction per candidate, commits
//                              the kept placements and reports the next candidate.
// The argument is in ks_query.h, above consolidate_route.  The two small kernels below serve the
// host's single path for a candidate with more pods than one set of lists decides.
#include "ks_query.h"
#include "ks_place_resolve.h"

namespace ks {
namespace {

__global__ __launch_bounds__(kWave) void consolidate_take_kernel(uint32_t* cordon, int64_t* state, int64_t n_pad,
                                                                 int32_t node) {
    if (threadIdx.x < 4) state[threadIdx.x * n_pad + node] = 0;
    if (threadIdx.x == 0) cordon[node >> 5] |= 1u << (node & 31);  // (one thread of one workgroup)
}

// ORs commute and nobody reads the words in this launch
__global__ __launch_bounds__(256) void consolidate_mark_kernel(const Placement* __restrict__ placed, int64_t k,
                                                               int32_t n_nodes, uint32_t* received) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const int32_t nd = placed[i].node;
    if ((uint32_t)nd < (uint32_t)n_nodes) atomicOr(received + (nd >> 5), 1u << (nd & 31));
}

}  // namespace

hipError_t launch_consolidate_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ConsRound& cr,
                                    hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.k < 0 || pc.k > kPlaceMaxPods || pc.n_shapes < 0 || pc.n_shapes > kPlaceMaxShapes ||
        (pc.k > 0) != (pc.n_shapes > 0) || cr.c0 < 0 || cr.c1 <= cr.c0 || !cr.cands || !cr.cordon || !cr.received ||
        !cr.out)
        return hipErrorInvalidValue;
    const uint64_t active = pc.n_shapes >= 64 ? ~0ull : (1ull << pc.n_shapes) - 1ull;
    if (pc.n_shapes)
        if (hipError_t r = launch_place_lists(s, pc, b, active, st, cr.cordon); r != hipSuccess) return r;
    hipLaunchKernelGGL((resolve_kernel<false, true>), dim3(1), dim3(kPRes), 0, st, s, b.state, b.n_pad, pc, b.shapes,
                       b.shape_of, (const uint64_t*)b.top, (const long long*)b.ccount, (const ScaleOption*)nullptr, b.out,
                       (ScaleResult*)nullptr, 0, active, b.rb, cr);
    return hipGetLastError();
}

hipError_t launch_consolidate_take(uint32_t* cordon, int64_t* state, int64_t n_pad, int32_t n_nodes, int32_t node,
                                   hipStream_t st) {
    if (node < 0 || node >= n_nodes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(consolidate_take_kernel, dim3(1), dim3(kWave), 0, st, cordon, state, n_pad, node);
    return hipGetLastError();
}

hipError_t launch_consolidate_mark(const Placement* placed, int64_t k, int32_t n_nodes, uint32_t* received, hipStream_t st) {
    if (k <= 0) return hipSuccess;
    hipLaunchKernelGGL(consolidate_mark_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, placed, k, n_nodes,
                       received);
    return hipGetLastError();
}

}  // namespace ks
