// ks_query.hip — scheduler state at past ticks, rebuilt from the binds (gfx950).
//
// The reference shows its state as it goes: Node.totalResourceRequest / runningPodsNum
// (kubesim/node/node.go:97-118) before every admission, the filtered node list and the nodeScore
// map of every scheduleOne (kubesim/kubesim.go:170,184,194,205).  A batched ks_step keeps none of
// it, but binds are final and FIFO-monotone in time, so the state after tick t's bind is a function
// of (b_node, b_status, t0, dur, PodRec.req) alone: pod q counts on its node while it was bound Ok
// and 0 <= t - t0[q] < dur[q] (Pod.IsRunning, kubesim/pod/pod.go:67-69, its int32 arithmetic folded
// into dur at submit).  Every kernel here reads those arrays and nothing else of the engine: the
// live node table, the scan and the resolvers are not involved.  (The headroom kernels also read
// the cluster's constants — alloc, taints, labels — which nothing writes after ks_load_nodes but
// the unit rescale of a submit, never in flight beside a query.)
//
// Grids follow the host's run-interval index (ks_engine.cpp usage_blocks): one workgroup per
// candidate block of kQBlk pods, so the cost follows the pods that may run in the queried ticks.
#include "ks_query.h"

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

// ---------------------------------------------------------------------------------------------
// ks_headroom_at: per shape the nine columns of include/ks_engine.h over the counts c(node, shape)
// (headroom_count, ks_query.h) at the rebuilt state.  One thread per node: its six constants and
// four state words stay in registers while the k shape records come through scalar loads.  A
// workgroup reduces three words per shape — Σ c; the argmax key (c << 32 | ~node: the highest
// count, then the lowest node); the six small counters (nodes with c >= 1, limiting cpu / memory /
// gpu / pods, ineligible) packed ten bits each (<= 256 per workgroup) — with wave shuffles and one
// LDS pass, and a second kernel reduces the workgroups' partials.  Integers only, no atomics: every
// column is the same whatever the order of execution.
// ---------------------------------------------------------------------------------------------
constexpr int kHBlk = 256;     // nodes per workgroup
constexpr int kHeadWords = 3;  // partial words per (workgroup, shape): sum, argmax key, packed counters
constexpr int kHeadCtrBits = 10, kHeadCtrs = 6;
// workgroups of the series kernel at the most (4 per CU): every workgroup ends in one atomic per
// column on the window's first slot, and same-address atomics serialise
constexpr int kHeadSeriesWgs = 1024;
static_assert(kHBlk < (1 << kHeadCtrBits) && kHeadCtrBits * kHeadCtrs <= 64, "packed counters hold a workgroup");

struct HeadCfg {
    int32_t n_nodes, k, filter_feeds;
    uint32_t filters;
    QScale sc;
};

// count of one node for one shape, and its counter word: slot 0 c >= 1, 1 + key, 5 ineligible
__device__ __forceinline__ int32_t head_eval(const HeadCfg& hc, const NodeV& v, const PodRec& sh, uint64_t* ctr) {
    if (!head_eligible(hc.filter_feeds, hc.filters, v, sh)) {
        *ctr = 1ull << (5 * kHeadCtrBits);
        return 0;
    }
    int32_t key;
    const int32_t c = headroom_count(v, hc.sc, sh, &key);
    *ctr = (1ull << ((1 + key) * kHeadCtrBits)) | (c >= 1 ? 1ull : 0ull);
    return c;
}

__global__ __launch_bounds__(kHBlk) void headroom_kernel(NodeSoA s, const int64_t* __restrict__ state, int64_t n_pad,
                                                         HeadCfg hc, const PodRec* __restrict__ shapes,
                                                         unsigned long long* __restrict__ part,
                                                         int32_t* __restrict__ per_node) {
    __shared__ unsigned long long red[kHeadMaxShapes][kHBlk / kWave][kHeadWords];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int32_t nd = blockIdx.x * kHBlk + threadIdx.x;
    const bool real = nd < hc.n_nodes;
    NodeV v{};
    if (real) {
        v.ac = s.ac[nd]; v.am = s.am[nd]; v.ag = s.ag[nd]; v.ap = s.ap[nd];
        v.taint = s.taint[nd]; v.label = s.label[nd];
        v.rc = state[nd]; v.rm = state[n_pad + nd]; v.rg = state[2 * n_pad + nd]; v.nr = state[3 * n_pad + nd];
    }
    for (int j = 0; j < hc.k; ++j) {
        const PodRec sh = sload(shapes + j);
        unsigned long long sum = 0, key = 0, ctr = 0;
        if (real) {
            uint64_t w;
            const int32_t c = head_eval(hc, v, sh, &w);
            sum = (unsigned long long)c;
            key = make_key((uint32_t)c, (uint32_t)nd);
            ctr = w;
            if (per_node) per_node[(int64_t)j * hc.n_nodes + nd] = c;
        }
        for (int o = kWave / 2; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, kWave);
            ctr += __shfl_xor(ctr, o, kWave);
            const unsigned long long other = __shfl_xor(key, o, kWave);
            key = other > key ? other : key;
        }
        if (lane == 0) {
            red[j][wave][0] = sum;
            red[j][wave][1] = key;
            red[j][wave][2] = ctr;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < hc.k; j += kHBlk) {
        unsigned long long sum = 0, key = 0, ctr = 0;
#pragma unroll
        for (int w = 0; w < kHBlk / kWave; ++w) {
            sum += red[j][w][0];
            key = red[j][w][1] > key ? red[j][w][1] : key;
            ctr += red[j][w][2];
        }
        unsigned long long* o = part + ((int64_t)blockIdx.x * hc.k + j) * kHeadWords;
        o[0] = sum; o[1] = key; o[2] = ctr;
    }
}

// out[k][kHeadCols] from part[nblk][k][kHeadWords]: one workgroup per shape
__global__ __launch_bounds__(256) void headroom_reduce_kernel(const unsigned long long* __restrict__ part, int32_t nblk,
                                                               int32_t k, long long* __restrict__ out) {
    __shared__ unsigned long long red[256 / kWave][2 + kHeadCtrs];
    const int j = blockIdx.x, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    unsigned long long w[2 + kHeadCtrs] = {};  // sum, key, the six counters unpacked
    for (int32_t b = threadIdx.x; b < nblk; b += 256) {
        const unsigned long long* p = part + ((int64_t)b * k + j) * kHeadWords;
        w[0] += p[0];
        w[1] = p[1] > w[1] ? p[1] : w[1];
#pragma unroll
        for (int c = 0; c < kHeadCtrs; ++c) w[2 + c] += (p[2] >> (c * kHeadCtrBits)) & ((1ull << kHeadCtrBits) - 1);
    }
#pragma unroll
    for (int c = 0; c < 2 + kHeadCtrs; ++c) {
        for (int o = kWave / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(w[c], o, kWave);
            w[c] = c == 1 ? (other > w[c] ? other : w[c]) : w[c] + other;
        }
        if (lane == 0) red[wave][c] = w[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r[2 + kHeadCtrs];
#pragma unroll
        for (int c = 0; c < 2 + kHeadCtrs; ++c) {
            r[c] = red[0][c];
            for (int x = 1; x < 256 / kWave; ++x) r[c] = c == 1 ? (red[x][c] > r[c] ? red[x][c] : r[c]) : r[c] + red[x][c];
        }
        long long* o = out + (int64_t)j * kHeadCols;
        o[0] = (long long)r[0];
        o[1] = (long long)r[2];
        o[2] = (long long)(r[1] >> 32);
        o[3] = r[1] ? (long long)(0xFFFFFFFFu - (uint32_t)r[1]) : -1;
        o[4] = (long long)r[3]; o[5] = (long long)r[4]; o[6] = (long long)r[5]; o[7] = (long long)r[6];
        o[8] = (long long)r[7];
    }
}

// ---------------------------------------------------------------------------------------------
// ks_headroom_series: Σ_n c and the nodes with c >= 1 per shape for every tick of [t_lo, t_hi), as
// difference arrays diff[2 k][T + 1] and one prefix sum per column — driven by the events, not by
// the ticks.  A node's count changes only where its state does: at a listed pod's start t0 or end
// t0 + dur (the peaks' counting sort lists, per node, the Ok pods that run somewhere in the window).
// One wave per node:
//   (a) the state at t_lo from the listed pods; lane j adds shape j's c and [c >= 1] to the
//       workgroup's head[] in LDS, which goes to the window's first slot with one global atomic per
//       workgroup and column (series_run_kernel's head[]);
//   (b) each lane takes events of the node; for the first event of every distinct tick tau in
//       (t_lo, t_hi) it sums the state at tau and at tau - 1 and adds c(tau) - c(tau - 1) at tau for
//       every shape (mod 2^64).  Further events on the same tick (an expiry on a bind tick) add nothing.
// Integer adds commute, so the atomics' order cannot change a result.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void headroom_series_kernel(const int32_t* __restrict__ off,
                                                               const int32_t* __restrict__ list, NodeSoA s, HeadCfg hc,
                                                               const PodRec* __restrict__ shapes, int64_t t_lo,
                                                               int64_t t_hi, const int64_t* t0, const int32_t* dur,
                                                               const PodRec* pods, unsigned long long* diff) {
    __shared__ unsigned long long head[2 * kHeadMaxShapes];
    if (threadIdx.x < 2 * kHeadMaxShapes) head[threadIdx.x] = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t T1 = t_hi - t_lo + 1;
    // a wave strides over nodes, so head[] gathers many nodes before its one atomic per column
    for (int32_t nd = blockIdx.x * (256 / kWave) + (threadIdx.x >> 6); nd < hc.n_nodes;
         nd += gridDim.x * (256 / kWave)) {
        const int32_t a = off[nd], k = off[nd + 1] - a;
        NodeV v{};
        v.ac = s.ac[nd]; v.am = s.am[nd]; v.ag = s.ag[nd]; v.ap = s.ap[nd];
        v.taint = s.taint[nd]; v.label = s.label[nd];
        // (a) the state at t_lo
        long long st[4] = {0, 0, 0, 0};
        for (int32_t j = lane; j < k; j += kWave) {
            const int32_t q = list[a + j];
            if (!runs_at(t_lo, t0[q], dur[q])) continue;
            st[0] += pods[q].req[0]; st[1] += pods[q].req[1]; st[2] += pods[q].req[2]; st[3] += 1;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            for (int o = kWave / 2; o > 0; o >>= 1) st[c] += __shfl_xor(st[c], o, kWave);
        if (lane < hc.k) {
            NodeV w = v;
            w.rc = st[0]; w.rm = st[1]; w.rg = st[2]; w.nr = st[3];
            uint64_t ctr;
            const int32_t c = head_eval(hc, w, shapes[lane], &ctr);
            if (c) {
                atomicAdd(&head[2 * lane], (unsigned long long)c);
                atomicAdd(&head[2 * lane + 1], 1ull);
            }
        }
        // (b) event 2 j: the start of the node's j-th pod, 2 j + 1: its end
        for (int32_t e = lane; e < 2 * k; e += kWave) {
            const int32_t qe = list[a + (e >> 1)];
            const int64_t tau = t0[qe] + ((e & 1) ? (int64_t)dur[qe] : 0);
            if (tau <= t_lo || tau >= t_hi) continue;
            long long now[4] = {0, 0, 0, 0}, was[4] = {0, 0, 0, 0};
            bool first = true;
            for (int32_t j = 0; j < k; ++j) {
                const int32_t q = list[a + j];
                const int64_t b = t0[q];
                const int32_t d = dur[q];
                // an earlier event of the node on the same tick already carries the change
                if ((b == tau && 2 * j < e) || (b + d == tau && 2 * j + 1 < e)) { first = false; break; }
                const bool r1 = runs_at(tau, b, d), r0 = runs_at(tau - 1, b, d);
                if (!r1 && !r0) continue;
                const long long q0 = pods[q].req[0], q1 = pods[q].req[1], q2 = pods[q].req[2];
                if (r1) { now[0] += q0; now[1] += q1; now[2] += q2; now[3] += 1; }
                if (r0) { was[0] += q0; was[1] += q1; was[2] += q2; was[3] += 1; }
            }
            if (!first) continue;
            if (now[0] == was[0] && now[1] == was[1] && now[2] == was[2] && now[3] == was[3]) continue;
            NodeV w1 = v, w0 = v;
            w1.rc = now[0]; w1.rm = now[1]; w1.rg = now[2]; w1.nr = now[3];
            w0.rc = was[0]; w0.rm = was[1]; w0.rg = was[2]; w0.nr = was[3];
            const int64_t idx = tau - t_lo;  // 0 < idx < T
            for (int j = 0; j < hc.k; ++j) {
                const PodRec sh = shapes[j];
                uint64_t ctr;
                const int32_t c1 = head_eval(hc, w1, sh, &ctr), c0 = head_eval(hc, w0, sh, &ctr);
                if (c1 == c0) continue;
                atomicAdd(&diff[(int64_t)(2 * j) * T1 + idx], (unsigned long long)((long long)c1 - (long long)c0));
                const int f1 = c1 >= 1, f0 = c0 >= 1;
                if (f1 != f0) atomicAdd(&diff[(int64_t)(2 * j + 1) * T1 + idx], (unsigned long long)(long long)(f1 - f0));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * hc.k && head[threadIdx.x]) atomicAdd(&diff[(int64_t)threadIdx.x * T1], head[threadIdx.x]);
}

// out[T][ncols] = prefix sums of diff[ncols][T + 1] (start value 0): series_scan_kernel's scheme for
// any number of columns, one workgroup per column
__global__ __launch_bounds__(1024) void cols_scan_kernel(const unsigned long long* __restrict__ diff, int64_t T,
                                                          int32_t ncols, unsigned long long* __restrict__ out) {
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
    unsigned long long run = tid ? part[tid - 1] : 0ull;
    for (int64_t i = lo; i < hi; ++i) {
        run += d[i];
        out[i * ncols + k] = run;
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

hipError_t launch_headroom(const NodeSoA& s, const int64_t* state, int64_t n_pad, int32_t n_nodes, int32_t filter_feeds,
                           uint32_t filters, const QScale& sc, const PodRec* shapes, int32_t k,
                           unsigned long long* part, long long* out, int32_t* per_node, hipStream_t st) {
    if (n_nodes <= 0 || k <= 0 || k > kHeadMaxShapes) return hipErrorInvalidValue;
    const HeadCfg hc{n_nodes, k, filter_feeds, filters, sc};
    const int32_t nblk = (n_nodes + kHBlk - 1) / kHBlk;
    hipLaunchKernelGGL(headroom_kernel, dim3((unsigned)nblk), dim3(kHBlk), 0, st, s, state, n_pad, hc, shapes, part,
                       per_node);
    hipLaunchKernelGGL(headroom_reduce_kernel, dim3((unsigned)k), dim3(256), 0, st, part, nblk, k, out);
    return hipGetLastError();
}

hipError_t launch_headroom_series(const int32_t* blocks, int64_t nblocks, int64_t q_hi, int64_t t_lo, int64_t t_hi,
                                  const NodeSoA& s, int32_t n_nodes, int32_t filter_feeds, uint32_t filters,
                                  const QScale& sc, const PodRec* shapes, int32_t k, const int32_t* b_node,
                                  const int32_t* b_status, const int64_t* t0, const int32_t* dur, const PodRec* pods,
                                  int32_t* cnt, int32_t* off, int32_t* cur, int32_t* list, int32_t list_cap,
                                  unsigned long long* diff, unsigned long long* out, hipStream_t st) {
    if (k <= 0 || k > kHeadMaxShapes || t_hi <= t_lo) return hipErrorInvalidValue;
    if (n_nodes > 0) {
        if (nblocks > 0)
            hipLaunchKernelGGL(peaks_count_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t_lo,
                               n_nodes, b_node, b_status, t0, dur, cnt);
        hipLaunchKernelGGL(peaks_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, n_nodes, off, cur);
        if (nblocks > 0)
            hipLaunchKernelGGL(peaks_fill_kernel, dim3((unsigned)nblocks), dim3(kQBlk), 0, st, blocks, q_hi, t_lo,
                               n_nodes, b_node, b_status, t0, dur, cur, list, list_cap);
        const HeadCfg hc{n_nodes, k, filter_feeds, filters, sc};
        const int per = 256 / kWave;
        const int wgs = (n_nodes + per - 1) / per;
        hipLaunchKernelGGL(headroom_series_kernel, dim3((unsigned)(wgs < kHeadSeriesWgs ? wgs : kHeadSeriesWgs)), dim3(256), 0, st, off,
                           list, s, hc, shapes, t_lo, t_hi, t0, dur, pods, diff);
    }
    hipLaunchKernelGGL(cols_scan_kernel, dim3((unsigned)(2 * k)), dim3(1024), 0, st, diff, t_hi - t_lo, 2 * k, out);
    return hipGetLastError();
}

}  // namespace ks
