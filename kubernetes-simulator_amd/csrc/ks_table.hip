// ks_table.hip — node-table upkeep and the api shims (gfx950): small kernels outside the batch
// chains (ks_filter / ks_score; §2: the constants table; §5: what-if groups).  None of
// them is on a step's hot path.
//   eval_pod     ks_filter / ks_score and the past-tick score queries (ks_queries.cpp): one pod
//                against every node.
//   flush        the expiries due by the engine's tick, before a filter / score call
//                (ks_engine.cpp).
//   rescale      a submit whose quantities the resource unit does not divide (ks_engine.cpp).
//   gather_binds ks_group_step's packed copy of every scenario's new binds (ks_step.cpp).
//   node_consts  the two-launch chain's constants table, once per step (ks_step.cpp chain_batch).
#include <algorithm>

#include "ks_device.h"

namespace ks {

// ------------------------------------------------------------------------------------------
// Filter mask / score of one pod against every node (api.Filter / api.Scorer shims).
// ------------------------------------------------------------------------------------------
template <int kMode>
__global__ __launch_bounds__(256) void eval_pod_kernel(Cfg c, NodeSoA s, const PodRec* pod, uint32_t filters,
                                                        uint8_t* mask, int64_t* score) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_nodes) return;
    const NodeV n = load_node(s, i);
    const PodRec p = *pod;
    bool ok = true;
    if (filters & kFilterFit) ok &= fits(p, n);
    if (filters & kFilterTaint) ok &= (n.taint & ~p.tol) == 0;
    if (filters & kFilterSelector) ok &= (n.label & p.sel) == p.sel;
    mask[i] = ok ? 1 : 0;
    const uint32_t t1 = eval_t<kMode>(c, p, n);
    score[i] = t1 ? (int64_t)t1 - 1 : -1;
}

// Apply every not-yet-applied expiry with finish tick <= t (before ks_filter / ks_score).
__global__ __launch_bounds__(256) void flush_kernel(NodeSoA s, const PodRec* pods, const int64_t* fin, int64_t t,
                                                     int64_t n_done, const int32_t* b_node, const int32_t* b_status,
                                                     uint8_t* expired) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_done; q += (int64_t)gridDim.x * blockDim.x) {
        if (fin[q] > t || b_status[q] != 0 || expired[q]) continue;
        const int32_t nd = b_node[q];
        const PodRec& p = pods[q];
        atomicAdd((unsigned long long*)&s.rc[nd], (unsigned long long)(-p.req[0]));
        atomicAdd((unsigned long long*)&s.rm[nd], (unsigned long long)(-p.req[1]));
        atomicAdd((unsigned long long*)&s.rg[nd], (unsigned long long)(-p.req[2]));
        atomicAdd((unsigned long long*)&s.nr[nd], (unsigned long long)(-1ll));
        expired[q] = 1;
    }
}

// Multiply every device quantity of resource k by f[k] (node capacity unless absent, requested
// totals, pod requests): the unit of resource k shrinks to a divisor of the old one when a pod
// brings a quantity the old unit does not divide (see ks_engine.cpp, resource scale).
__global__ __launch_bounds__(256) void rescale_kernel(NodeSoA s, int64_t n_pad, PodRec* pods, int64_t P,
                                                      int64_t f0, int64_t f1, int64_t f2) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += stride) {
        if (s.ac[i] >= 0) s.ac[i] *= f0;
        if (s.am[i] >= 0) s.am[i] *= f1;
        if (s.ag[i] >= 0) s.ag[i] *= f2;
        s.rc[i] *= f0; s.rm[i] *= f1; s.rg[i] *= f2;
    }
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < P; q += stride) {
        pods[q].req[0] *= f0; pods[q].req[1] *= f1; pods[q].req[2] *= f2;
    }
}

// Packed copy of each scenario's new binds (ks_group_step): one D2H copy for the whole group.
__global__ __launch_bounds__(256) void gather_binds_kernel(const BindSeg* __restrict__ segs, int32_t* node,
                                                            int32_t* status) {
    const BindSeg g = segs[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * blockDim.x) {
        node[g.off + i] = g.node[g.lo + i];
        status[g.off + i] = g.status[g.lo + i];
    }
}

hipError_t launch_gather_binds(const BindSeg* segs, int S, int64_t max_n, int32_t* node, int32_t* status,
                               hipStream_t st) {
    if (S <= 0 || max_n <= 0) return hipSuccess;
    const unsigned bx = (unsigned)std::min<int64_t>((max_n + 255) / 256, 64);
    hipLaunchKernelGGL(gather_binds_kernel, dim3(bx, S), dim3(256), 0, st, segs, node, status);
    return hipGetLastError();
}

// The node constants table (EngineArgs::ncst): per node the six fields no batch kernel writes, in
// the 12-word record's words 0 and 2 (put_rec12).
__global__ __launch_bounds__(256) void node_consts_kernel(const NodeSoA s, int64_t n_pad, uint4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pad) return;
    const int64_t ap = s.ap[i];
    const uint64_t t = s.taint[i], l = s.label[i];
    out[2 * i] = make_uint4((uint32_t)s.ac[i], (uint32_t)s.am[i], (uint32_t)s.ag[i],
                            (uint32_t)(ap > 0x7FFFFFFF ? 0x7FFFFFFF : ap));
    out[2 * i + 1] = make_uint4((uint32_t)t, (uint32_t)(t >> 32), (uint32_t)l, (uint32_t)(l >> 32));
}

hipError_t launch_node_consts(const NodeSoA& s, int64_t n_pad, uint4* out, hipStream_t st) {
    if (n_pad <= 0) return hipSuccess;
    hipLaunchKernelGGL(node_consts_kernel, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, st, s, n_pad, out);
    return hipGetLastError();
}

hipError_t launch_rescale(const NodeSoA& s, int64_t n_pad, PodRec* pods, int64_t P, const int64_t f[3], hipStream_t st) {
    hipLaunchKernelGGL(rescale_kernel, dim3(1024), dim3(256), 0, st, s, n_pad, pods, P, f[0], f[1], f[2]);
    return hipGetLastError();
}

hipError_t launch_eval_pod(const Cfg& c, const NodeSoA& s, const PodRec* pod, uint32_t filters, uint8_t* mask,
                           int64_t* score, int mode, hipStream_t st) {
    const dim3 g((c.n_nodes + 255) / 256);
    with_eval_mode(mode, [&](auto m) {
        hipLaunchKernelGGL(eval_pod_kernel<decltype(m)::value>, g, dim3(256), 0, st, c, s, pod, filters, mask, score);
    });
    return hipGetLastError();
}

hipError_t launch_flush(const NodeSoA& s, const PodRec* pods, const int64_t* fin, int64_t t, int64_t n_done,
                        const int32_t* b_node, const int32_t* b_status, uint8_t* expired, hipStream_t st) {
    if (n_done <= 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n_done + 255) / 256, 2048);
    hipLaunchKernelGGL(flush_kernel, dim3((unsigned)blocks), dim3(256), 0, st, s, pods, fin, t, n_done, b_node,
                       b_status, expired);
    return hipGetLastError();
}
}  // namespace ks
