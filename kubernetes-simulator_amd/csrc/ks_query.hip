// ks_query.hip — scheduler state at past ticks, rebuilt from the binds (gfx950).
//
// The reference shows its state as it goes: Node.totalResourceRequest / runningPodsNum
// (kubesim/node/node.go:97-118) before every admission, the filtered node list and the nodeScore
// map of every scheduleOne (kubesim/kubesim.go:170,184,194,205).  A batched ks_step keeps none of
// it, but binds are final and FIFO-monotone in time, so the state after tick t's bind is a function
// of (b_node, b_status, t0, dur, PodRec.req) alone: pod q counts on its node while it was bound Ok
// and 0 <= t - t0[q] < dur[q] (Pod.IsRunning, kubesim/pod/pod.go:67-69, its int32 arithmetic folded
// into dur at submit).  Every kernel here reads those arrays and nothing else of the engine: the
// live node table, the scan and the resolvers are not involved.
//
// Grids follow the host's run-interval index (ks_engine.cpp usage_blocks): one workgroup per
// candidate block of kQBlk pods, so the cost follows the pods that may run in the queried ticks.
#include "ks_device.h"

namespace ks {
namespace {

constexpr int kQBlk = 256;  // pods per candidate block (= the usage index's block)

__device__ __forceinline__ bool runs_at(int64_t t, int64_t t0, int32_t dur) {
    const int64_t dt = t - t0;
    return dt >= 0 && dt < dur;
}

// ---------------------------------------------------------------------------------------------
// ks_requested_at / ks_filter_at / ks_score_at: per node {Σ req cpu, Σ req memory, Σ req gpu,
// running pods} over the pods < q_hi running at t, scattered with 64-bit atomic adds (exact).
// Word k of node nd is out[nd * node_stride + k * col_stride]: (4, 1) keeps a node's four words
// together ([n][4], the query's output), (1, n_pad) is the node table's rc rm rg nr layout.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kQBlk) void requested_kernel(const int32_t* __restrict__ blocks, int64_t q_hi, int64_t t,
                                                          int32_t n_nodes, const int32_t* b_node,
                                                          const int32_t* b_status, const int64_t* t0,
                                                          const int32_t* dur, const PodRec* pods, QScale sc,
                                                          int64_t node_stride, int64_t col_stride,
                                                          unsigned long long* out) {
    const int64_t q = (int64_t)blocks[blockIdx.x] * kQBlk + threadIdx.x;
    if (q >= q_hi || b_status[q] != 0) return;
    if (!runs_at(t, t0[q], dur[q])) return;
    const int32_t nd = b_node[q];
    if ((uint32_t)nd >= (uint32_t)n_nodes) return;
    unsigned long long* o = out + (int64_t)nd * node_stride;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t v = (uint64_t)(pods[q].req[k] * sc.f[k]);
        if (v) atomicAdd(&o[k * col_stride], (unsigned long long)v);
    }
    atomicAdd(&o[3 * col_stride], 1ull);
}

// ---------------------------------------------------------------------------------------------
// ks_cluster_series: seven per-tick columns over ticks [t_lo, t_hi) as difference arrays
// diff[7][T + 1] (T = t_hi - t_lo) and one prefix sum.  Columns 0..3 (running pods, Σ requested
// cpu / memory / gpu): a pod running over ticks [a0, a1) of the window adds at a0 and takes back at
// a1.  A block's adds at the window's first tick (every pod that was already running there) are
// summed in LDS first: one global atomic per block and column instead of one per pod.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kQBlk) void series_run_kernel(const int32_t* __restrict__ blocks, int64_t q_hi,
                                                           int64_t t_lo, int64_t t_hi, const int32_t* b_status,
                                                           const int64_t* t0, const int32_t* dur, const PodRec* pods,
                                                           QScale sc, unsigned long long* diff) {
    __shared__ unsigned long long head[4];
    if (threadIdx.x < 4) head[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t T = t_hi - t_lo, T1 = T + 1;
    const int64_t q = (int64_t)blocks[blockIdx.x] * kQBlk + threadIdx.x;
    if (q < q_hi && b_status[q] == 0) {
        const int64_t d = dur[q], s = t0[q];
        const int64_t a0 = max(s, t_lo), a1 = min(s + d, t_hi);
        if (d > 0 && a0 < a1) {
            const int64_t lo = a0 - t_lo, hi = a1 - t_lo;  // 0 <= lo < hi <= T
            uint64_t v[4];
            v[0] = 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) v[1 + k] = (uint64_t)(pods[q].req[k] * sc.f[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!v[k]) continue;
                if (lo == 0) atomicAdd(&head[k], (unsigned long long)v[k]);
                else atomicAdd(&diff[k * T1 + lo], (unsigned long long)v[k]);
                if (hi < T) atomicAdd(&diff[k * T1 + hi], (unsigned long long)(0ull - v[k]));  // [T] is never summed
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && head[threadIdx.x]) atomicAdd(&diff[threadIdx.x * T1], head[threadIdx.x]);
}

// Columns 4..6 (bound Ok so far, bound OverCapacity so far, pending): counts at the bind ticks of
// the pods [q_lo, q_lo + n_q) taken off the queue inside the window and at the arrival ticks
// arr[0, n_arr) that fall inside it; their values at t_lo are the scan's start values.
__global__ __launch_bounds__(256) void series_event_kernel(int64_t q_lo, int64_t n_q, int64_t t_lo, int64_t T,
                                                            const int32_t* b_status, const int64_t* t0,
                                                            const int64_t* __restrict__ arr, int64_t n_arr,
                                                            unsigned long long* diff) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t T1 = T + 1;
    if (i < n_q) {
        const int64_t q = q_lo + i, idx = t0[q] - t_lo;
        if (idx >= 0 && idx < T) {
            const int32_t st = b_status[q];
            if (st == 0) atomicAdd(&diff[4 * T1 + idx], 1ull);
            else if (st == 1) atomicAdd(&diff[5 * T1 + idx], 1ull);
            atomicAdd(&diff[6 * T1 + idx], ~0ull);  // popped from the queue (bound or not)
        }
    }
    if (i < n_arr) {
        const int64_t idx = arr[i] - t_lo;
        if (idx >= 0 && idx < T) atomicAdd(&diff[6 * T1 + idx], 1ull);
    }
}

// out[T][kSeriesCols] = start value + prefix sums of diff[kSeriesCols][T + 1]: one workgroup per
// column, each thread a contiguous chunk, a workgroup scan of the chunk sums.
__global__ __launch_bounds__(1024) void series_scan_kernel(const unsigned long long* __restrict__ diff, int64_t T,
                                                            SeriesInit init, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[1024];
    const int k = blockIdx.x, tid = threadIdx.x;
    const unsigned long long* d = diff + (int64_t)k * (T + 1);
    const int64_t chunk = (T + 1023) / 1024, lo = min<int64_t>(T, tid * chunk), hi = min<int64_t>(T, lo + chunk);
    unsigned long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += d[i];
    part[tid] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = tid >= off ? part[tid - off] : 0ull;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned long long run = (unsigned long long)init.v[k] + (tid ? part[tid - 1] : 0ull);
    for (int64_t i = lo; i < hi; ++i) {
        run += d[i];
        out[i * kSeriesCols + k] = run;
    }
}

// ---------------------------------------------------------------------------------------------
// ks_node_peaks: per node and column the maximum of the requested state over ticks [t_lo, t_hi).
// Requests are non-negative, so a column rises only when a pod starts: the peak is the maximum of
// the state at t_lo and of the state right after each Ok bind on the node inside the window.  The
// candidate pods (Ok, running somewhere at or after t_lo) are grouped by node with a counting sort
// (count, exclusive scan, fill); then one wave per node: each lane takes start events of the node,
// sums the node's pods running at its event, and a wave max-reduce gives the peak.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int32_t peak_node(int64_t q, int64_t q_hi, int64_t t_lo, int32_t n_nodes,
                                             const int32_t* b_node, const int32_t* b_status, const int64_t* t0,
                                             const int32_t* dur) {
    if (q >= q_hi || b_status[q] != 0) return -1;
    const int64_t d = dur[q];
    if (d <= 0 || t0[q] + d <= t_lo) return -1;
    const int32_t nd = b_node[q];
    return (uint32_t)nd < (uint32_t)n_nodes ? nd : -1;
}

__global__ __launch_bounds__(kQBlk) void peaks_count_kernel(const int32_t* __restrict__ blocks, int64_t q_hi,
                                                            int64_t t_lo, int32_t n_nodes, const int32_t* b_node,
                                                            const int32_t* b_status, const int64_t* t0,
                                                            const int32_t* dur, int32_t* cnt) {
    const int64_t q = (int64_t)blocks[blockIdx.x] * kQBlk + threadIdx.x;
    const int32_t nd = peak_node(q, q_hi, t_lo, n_nodes, b_node, b_status, t0, dur);
    if (nd >= 0) atomicAdd(&cnt[nd], 1);
}

// off[n + 1] = exclusive prefix sums of cnt[n] (one workgroup), cur[n] = the fill's cursors
__global__ __launch_bounds__(1024) void peaks_scan_kernel(const int32_t* __restrict__ cnt, int32_t n, int32_t* off,
                                                           int32_t* cur) {
    __shared__ int32_t part[1024];
    const int tid = threadIdx.x;
    const int32_t chunk = (n + 1023) / 1024, lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int32_t s = 0;
    for (int32_t i = lo; i < hi; ++i) s += cnt[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int32_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int32_t run = tid ? part[tid - 1] : 0;
    for (int32_t i = lo; i < hi; ++i) {
        off[i] = run;
        cur[i] = run;
        run += cnt[i];
    }
    if (tid == 1023) off[n] = part[1023];
}

__global__ __launch_bounds__(kQBlk) void peaks_fill_kernel(const int32_t* __restrict__ blocks, int64_t q_hi,
                                                           int64_t t_lo, int32_t n_nodes, const int32_t* b_node,
                                                           const int32_t* b_status, const int64_t* t0,
                                                           const int32_t* dur, int32_t* cur, int32_t* list,
                                                           int32_t list_cap) {
    const int64_t q = (int64_t)blocks[blockIdx.x] * kQBlk + threadIdx.x;
    const int32_t nd = peak_node(q, q_hi, t_lo, n_nodes, b_node, b_status, t0, dur);
    if (nd < 0) return;
    const int32_t pos = atomicAdd(&cur[nd], 1);
    if ((uint32_t)pos < (uint32_t)list_cap) list[pos] = (int32_t)q;
}

__global__ __launch_bounds__(256) void peaks_kernel(const int32_t* __restrict__ off, const int32_t* __restrict__ list,
                                                     int32_t n_nodes, int64_t t_lo, const int64_t* t0,
                                                     const int32_t* dur, const PodRec* pods, QScale sc,
                                                     long long* out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int32_t nd = blockIdx.x * (256 / kWave) + (threadIdx.x >> 6);
    if (nd >= n_nodes) return;  // whole waves leave together
    const int32_t a = off[nd], k = off[nd + 1] - a;
    long long m[4] = {0, 0, 0, 0};
    // event e < k: right after the bind of the node's e-th pod (one inside the window; an earlier
    // one folds onto t_lo); event k: t_lo itself
    for (int32_t e = lane; e <= k; e += kWave) {
        const int64_t tau = e < k ? max(t0[list[a + e]], t_lo) : t_lo;
        long long s[4] = {0, 0, 0, 0};
        for (int32_t j = 0; j < k; ++j) {
            const int32_t q = list[a + j];
            if (!runs_at(tau, t0[q], dur[q])) continue;
            s[0] += pods[q].req[0];
            s[1] += pods[q].req[1];
            s[2] += pods[q].req[2];
            s[3] += 1;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) m[c] = max(m[c], s[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        for (int o = kWave / 2; o > 0; o >>= 1) m[c] = max(m[c], __shfl_xor(m[c], o, kWave));
    }
    if (lane == 0) {
        out[(int64_t)nd * 4 + 0] = m[0] * sc.f[0];
        out[(int64_t)nd * 4 + 1] = m[1] * sc.f[1];
        out[(int64_t)nd * 4 + 2] = m[2] * sc.f[2];
        out[(int64_t)nd * 4 + 3] = m[3];
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Launchers, called by ks_engine.cpp.
// ---------------------------------------------------------------------------------------------
hipError_t launch_requested(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t, int32_t n_nodes,
                            const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                            const PodRec* pods, const QScale& sc, int64_t node_stride, int64_t col_stride,
                            unsigned long long* out, hipStream_t st) {
    if (nblocks > 0)
        hipLaunchKernelGGL(requested_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t, n_nodes,
                           b_node, b_status, t0, dur, pods, sc, node_stride, col_stride, out);
    return hipGetLastError();
}

hipError_t launch_series(const int32_t* blocks, int64_t nblocks, int64_t q_lo, int64_t q_hi, int64_t t_lo,
                         int64_t t_hi, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                         const PodRec* pods, const QScale& sc, const int64_t* arr, int64_t n_arr,
                         const SeriesInit& init, unsigned long long* diff, unsigned long long* out, hipStream_t st) {
    const int64_t T = t_hi - t_lo;
    if (nblocks > 0)
        hipLaunchKernelGGL(series_run_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t_lo, t_hi,
                           b_status, t0, dur, pods, sc, diff);
    const int64_t n_q = q_hi - q_lo, n_ev = n_q > n_arr ? n_q : n_arr;
    if (n_ev > 0)
        hipLaunchKernelGGL(series_event_kernel, dim3((unsigned)((n_ev + 255) / 256)), dim3(256), 0, st, q_lo, n_q, t_lo,
                           T, b_status, t0, arr, n_arr, diff);
    hipLaunchKernelGGL(series_scan_kernel, dim3(kSeriesCols), dim3(1024), 0, st, diff, T, init, out);
    return hipGetLastError();
}

hipError_t launch_node_peaks(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t_lo, int32_t n_nodes,
                             const int32_t* b_node, const int32_t* b_status, const int64_t* t0, const int32_t* dur,
                             const PodRec* pods, const QScale& sc, int32_t* cnt, int32_t* off, int32_t* cur,
                             int32_t* list, int32_t list_cap, long long* out, hipStream_t st) {
    if (n_nodes <= 0) return hipSuccess;
    if (nblocks > 0)
        hipLaunchKernelGGL(peaks_count_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t_lo, n_nodes,
                           b_node, b_status, t0, dur, cnt);
    hipLaunchKernelGGL(peaks_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, n_nodes, off, cur);
    if (nblocks > 0)
        hipLaunchKernelGGL(peaks_fill_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t_lo, n_nodes,
                           b_node, b_status, t0, dur, cur, list, list_cap);
    const int per = 256 / kWave;
    hipLaunchKernelGGL(peaks_kernel, dim3((unsigned)((n_nodes + per - 1) / per)), dim3(256), 0, st, off, list, n_nodes,
                       t_lo, t0, dur, pods, sc, out);
    return hipGetLastError();
}

}  // namespace ks
