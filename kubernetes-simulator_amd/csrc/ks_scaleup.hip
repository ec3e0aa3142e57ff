// ks_scaleup.hip — scale-up preview: where k pending pods would be bound at a past tick if up to
// max_nodes empty nodes of a node-group template were appended to the cluster, for G options at
// once (gfx950, wave64).
//
// ks_scale_up_at asks ks_place_at's question on G extended clusters.  Every option starts from the
// same state at t and differs only in its appended nodes, so the cluster is scanned once on the base
// state (launch_place_lists) and one workgroup per option decides the k pods from those lists
// (resolve_kernel<true>, launch_scaleup_resolve): the shared pod loop of ks_place.hip.  This file
// keeps
//   scaleup_extend_kernel    the node constants of one option's extended cluster, for the options
//                            the resolver stopped at (the host re-places them with ks_place_at's own
//                            rounds on n + max_nodes nodes).
#include "ks_query.h"

namespace ks {
namespace {

// field f of row r at dst[f * np_ext + r]: ac am ag ap taint label
__global__ __launch_bounds__(256) void scaleup_extend_kernel(NodeSoA s, int32_t n, QScale sc, ScaleOption opt,
                                                             int64_t np_ext, int64_t* __restrict__ dst) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= np_ext) return;
    NodeV v{};
    v.ac = v.am = v.ag = -1;  // padding: absent keys, no pods
    if (r < n) {
        v.ac = s.ac[r]; v.am = s.am[r]; v.ag = s.ag[r]; v.ap = s.ap[r];
        v.taint = s.taint[r]; v.label = s.label[r];
        place_scale_alloc(v, sc);
    } else if (r < (int64_t)n + opt.max_nodes) {
        v = opt.tmpl;
    }
    dst[r] = v.ac;
    dst[np_ext + r] = v.am;
    dst[2 * np_ext + r] = v.ag;
    dst[3 * np_ext + r] = v.ap;
    dst[4 * np_ext + r] = (int64_t)v.taint;
    dst[5 * np_ext + r] = (int64_t)v.label;
}

}  // namespace

hipError_t launch_scaleup_extend(const NodeSoA& s, int32_t n, const QScale& sc, const ScaleOption& opt, int64_t np_ext,
                                 int64_t* dst, hipStream_t st) {
    if (n < 0 || opt.max_nodes < 0 || opt.max_nodes > kScaleMaxNodes || np_ext < (int64_t)n + opt.max_nodes || np_ext <= 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(scaleup_extend_kernel, dim3((unsigned)((np_ext + 255) / 256)), dim3(256), 0, st, s, n, sc, opt,
                       np_ext, dst);
    return hipGetLastError();
}

}  // namespace ks
