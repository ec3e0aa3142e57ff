// ks_drain.hip — drain preview: the pods running on a node set at a past tick, gathered in FIFO
// order for the placement rounds of ks_place.hip (gfx950, wave64).
//
// ks_drain_at takes a set of nodes out of k.nodes at tick t (kubesim/kubesim.go:168-206 no longer
// visit them) and hands every pod running on them, in pod order, to scheduleOne on a private copy of
// the state.  This file holds what ks_place.hip lacks for that:
//   drain_count_kernel   per candidate 256-pod block the pods selected (bound Ok before q_hi, running
//                        at t, on a cordoned node): wave ballots, the waves' counts through LDS;
//   drain_scan_kernel    one workgroup: the exclusive scan of the block counts in chunks of 256 with a
//                        carry, and the total;
//   drain_fill_kernel    the same predicate; a pod's rank is its block's offset + the counts of the
//                        waves before its own + the selected lanes below it (drain_rank, ks_query.h),
//                        and it writes its index, its node and its 48-byte record there;
//   drain_clear_kernel   zeroes the cordoned nodes' rc rm rg nr in the 4 x N_pad scratch state;
//   drain_pack_kernel    the ks_eviction rows from the gather and the rounds' placements.
// The host lists the candidate blocks in ascending order, so ranks follow the pod index: the output
// is the FIFO order by construction, with no atomics and whatever the order of execution.
#include "ks_query.h"

namespace ks {
namespace {

constexpr int kDWaves = kDrainBlk / kWave;
static_assert(kDrainBlk == 256 && kDWaves == 4, "gather workgroup = the usage index's block");

__device__ __forceinline__ bool drain_runs_at(int64_t t, int64_t t0, int32_t dur) {
    const int64_t dt = t - t0;
    return dt >= 0 && dt < dur;
}

// the gather's predicate for pod q (requested_kernel's, and the pod's node is cordoned)
__device__ __forceinline__ bool drain_selected(int64_t q, int64_t q_hi, int64_t t, int32_t n_nodes,
                                               const int32_t* __restrict__ b_node,
                                               const int32_t* __restrict__ b_status, const int64_t* __restrict__ t0,
                                               const int32_t* __restrict__ dur, const uint32_t* __restrict__ cordon,
                                               int32_t* node) {
    *node = -1;
    if (q >= q_hi || b_status[q] != 0) return false;
    if (!drain_runs_at(t, t0[q], dur[q])) return false;
    const int32_t nd = b_node[q];
    if ((uint32_t)nd >= (uint32_t)n_nodes) return false;
    *node = nd;
    return drain_cordoned(cordon, nd);
}

__global__ __launch_bounds__(kDrainBlk) void drain_count_kernel(const int32_t* __restrict__ blocks, int64_t q_hi,
                                                                int64_t t, int32_t n_nodes, const int32_t* b_node,
                                                                const int32_t* b_status, const int64_t* t0,
                                                                const int32_t* dur, const uint32_t* cordon,
                                                                int32_t* __restrict__ bcnt) {
    __shared__ int32_t wc[kDWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blocks[blockIdx.x] * kDrainBlk + threadIdx.x;
    int32_t nd;
    const bool sel = drain_selected(q, q_hi, t, n_nodes, b_node, b_status, t0, dur, cordon, &nd);
    const uint64_t ballot = __ballot(sel);
    if (lane == 0) wc[wave] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) bcnt[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// exclusive scan of bcnt[nblocks] into boff, the sum into *total: chunks of 256 counts, each scanned
// in LDS (Hillis-Steele, double-buffered), the chunks chained by a carry every thread keeps
__global__ __launch_bounds__(kDrainBlk) void drain_scan_kernel(const int32_t* __restrict__ bcnt, int64_t nblocks,
                                                               int32_t* __restrict__ boff,
                                                               long long* __restrict__ total) {
    __shared__ int32_t buf[2][kDrainBlk];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int64_t base = 0; base < nblocks; base += kDrainBlk) {
        const int64_t b = base + tid;
        const int32_t c = b < nblocks ? bcnt[b] : 0;
        int cur = 0;
        buf[0][tid] = c;
        __syncthreads();
        for (int o = 1; o < kDrainBlk; o <<= 1) {
            const int32_t v = buf[cur][tid] + (tid >= o ? buf[cur][tid - o] : 0);
            buf[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        const int32_t incl = buf[cur][tid], sum = buf[cur][kDrainBlk - 1];
        if (b < nblocks) boff[b] = (int32_t)(carry + incl - c);
        carry += sum;
        __syncthreads();  // buf[0] is written again by the next chunk
    }
    if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(kDrainBlk) void drain_fill_kernel(const int32_t* __restrict__ blocks, int64_t q_hi,
                                                               int64_t t, int32_t n_nodes, const int32_t* b_node,
                                                               const int32_t* b_status, const int64_t* t0,
                                                               const int32_t* dur, const PodRec* __restrict__ pods,
                                                               const uint32_t* cordon,
                                                               const int32_t* __restrict__ boff, int64_t cap,
                                                               long long* __restrict__ ev_pod,
                                                               int32_t* __restrict__ ev_from,
                                                               PodRec* __restrict__ ev_rec) {
    __shared__ int32_t wc[kDWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blocks[blockIdx.x] * kDrainBlk + threadIdx.x;
    int32_t nd;
    const bool sel = drain_selected(q, q_hi, t, n_nodes, b_node, b_status, t0, dur, cordon, &nd);
    const uint64_t ballot = __ballot(sel);
    if (lane == 0) wc[wave] = __popcll(ballot);
    __syncthreads();
    if (!sel) return;
    const int64_t rank = drain_rank(boff[blockIdx.x], wc, wave, ballot, lane);
    if (rank < 0 || rank >= cap) return;  // the host sized cap from the same count
    ev_pod[rank] = q;
    ev_from[rank] = nd;
    PodRec r = pods[q];
    r.flags = 0u;
    ev_rec[rank] = r;
}

__global__ __launch_bounds__(256) void drain_clear_kernel(const uint32_t* __restrict__ cordon, int32_t n_nodes,
                                                          int64_t* __restrict__ state, int64_t n_pad) {
    const int32_t nd = blockIdx.x * 256 + threadIdx.x;
    if (nd >= n_nodes || !drain_cordoned(cordon, nd)) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) state[c * n_pad + nd] = 0;
}

__global__ __launch_bounds__(256) void drain_pack_kernel(const long long* __restrict__ ev_pod,
                                                         const int32_t* __restrict__ ev_from,
                                                         const Placement* __restrict__ placed, int64_t n_ev,
                                                         Eviction* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_ev) return;
    const Placement p = placed[i];
    out[i] = Eviction{ev_pod[i], ev_from[i], p.node, p.status, 0, p.score, p.candidates};
}

}  // namespace

hipError_t launch_drain_count(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                              const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                              const DrainBufs& d, hipStream_t st) {
    if (nblocks < 0 || nblocks > 0x7FFFFFFF || n_nodes <= 0) return hipErrorInvalidValue;
    if (nblocks)
        hipLaunchKernelGGL(drain_count_kernel, dim3((unsigned)nblocks), dim3(kDrainBlk), 0, st, blocks, q_hi, t, n_nodes,
                           b_node, b_status, t0, dur, d.cordon, d.bcnt);
    hipLaunchKernelGGL(drain_scan_kernel, dim3(1), dim3(kDrainBlk), 0, st, (const int32_t*)d.bcnt, nblocks, d.boff,
                       d.total);
    return hipGetLastError();
}

hipError_t launch_drain_fill(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                             const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                             const PodRec* pods, const DrainBufs& d, hipStream_t st) {
    if (nblocks <= 0 || nblocks > 0x7FFFFFFF || n_nodes <= 0 || d.cap <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(drain_fill_kernel, dim3((unsigned)nblocks), dim3(kDrainBlk), 0, st, blocks, q_hi, t, n_nodes,
                       b_node, b_status, t0, dur, pods, d.cordon, (const int32_t*)d.boff, d.cap, d.ev_pod, d.ev_from,
                       d.ev_rec);
    return hipGetLastError();
}

hipError_t launch_drain_clear(const uint32_t* cordon, int32_t n_nodes, int64_t* state, int64_t n_pad, hipStream_t st) {
    if (n_nodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(drain_clear_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, st, cordon, n_nodes,
                       state, n_pad);
    return hipGetLastError();
}

hipError_t launch_drain_pack(const long long* ev_pod, const int32_t* ev_from, const Placement* placed, int64_t n_ev,
                             Eviction* out, hipStream_t st) {
    if (n_ev <= 0) return hipSuccess;
    hipLaunchKernelGGL(drain_pack_kernel, dim3((unsigned)((n_ev + 255) / 256)), dim3(256), 0, st, ev_pod, ev_from,
                       placed, n_ev, out);
    return hipGetLastError();
}

}  // namespace ks
