// ks_scaleup.hip — scale-up preview: where k pending pods would be bound at a past tick if up to
// max_nodes empty nodes of a node-group template were appended to the cluster, for G options at
// once (gfx950, wave64).
//
// ks_scale_up_at asks ks_place_at's question on G extended clusters.  Every option starts from the
// same state at t and differs only in its appended nodes, so the cluster is scanned once on the base
// state (launch_place_lists, ks_place.hip) and
//   scaleup_resolve_kernel   one workgroup per option decides the k pods in order from those lists,
//                            its changed set private in LDS, the unchanged appended nodes stood for
//                            by the first of them (the argument is in ks_device.h, above
//                            scaleup_fresh_key); it commits nothing and reads top / ccount / state
//                            read-only;
//   scaleup_extend_kernel    the node constants of one option's extended cluster, for the options
//                            the resolver stopped at (the host re-places them with ks_place_at's own
//                            rounds on n + max_nodes nodes).
// Integers only, no global atomics, no communication between workgroups.  The flag bits are set with
// LDS atomics as in place_resolve_kernel: the sets of one pod commute and barriers separate them
// from every read of the flags.
#include "ks_device.h"

namespace ks {
namespace {

constexpr int kSRes = 1024;  // threads of the resolver: one per changed node
constexpr int kSEnt = (kPlaceMaxShapes * kPlaceL + kSRes - 1) / kSRes;  // list entries a resolver thread owns
static_assert(kPlaceMaxPods <= kSRes, "a resolver thread per changed node, and one for the fresh node");

// ---------------------------------------------------------------------------------------------
// place_resolve_kernel's layout (ks_place.hip): LDS holds the lists and their flags, the shapes, the
// pods' shape indices, the running candidate counts and the changed set; every global read is issued
// before the pod loop; list entry (shape, e) belongs to thread (shape * L + e) % kSRes.
//
// The appended nodes: thread nchg — the first thread without a changed node — evaluates the fresh
// node n + u on the empty template (scaleup_fresh_key), so the wave maxima give D' = max(D, F) with
// no further step.  When its key wins, the same thread puts the template into slot nchg and names
// the slot; nchg and u grow by one (scaleup_takes_fresh).  nchg <= the pods decided < k <= kSRes
// inside the loop, so thread nchg exists.
//
// Per pod (uniform control flow, three barriers): as place_resolve_kernel.  kPlaceStop ends the
// workgroup: out[g].path = kScaleStopped and the rows are the host's to fill.
// All loops are bounded by k, L and the changed set.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSRes) void scaleup_resolve_kernel(NodeSoA s, const int64_t* __restrict__ state,
                                                                int64_t n_pad, PlaceCfg pc,
                                                                const PodRec* __restrict__ shapes,
                                                                const int32_t* __restrict__ shape_of,
                                                                const uint64_t* __restrict__ top,
                                                                const long long* __restrict__ ccount,
                                                                const ScaleOption* __restrict__ opts,
                                                                Placement* __restrict__ rows,
                                                                ScaleResult* __restrict__ out) {
    __shared__ NodeV chg[kPlaceMaxPods];
    __shared__ int32_t chg_node[kPlaceMaxPods];
    __shared__ uint64_t lst[kPlaceMaxShapes][kPlaceL];
    __shared__ uint32_t lflag[kPlaceMaxShapes];  // bit e: entry e's node is in the changed set
    __shared__ int32_t llen[kPlaceMaxShapes];
    __shared__ PodRec shp[kPlaceMaxShapes];
    __shared__ long long cc[kPlaceMaxShapes];
    __shared__ uint8_t sof[kPlaceMaxPods];
    __shared__ uint64_t wmax[2][kSRes / kWave];
    __shared__ int32_t slot[2];
    __shared__ int32_t used[kSRes / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    constexpr int kEntries = kPlaceMaxShapes * kPlaceL;
    const ScaleOption opt = sload(opts + blockIdx.x);
    const NodeV tmpl = opt.tmpl;
    const int32_t max_nodes = opt.max_nodes < 0 ? 0 : opt.max_nodes > kScaleMaxNodes ? kScaleMaxNodes : opt.max_nodes;
    const int32_t k = pc.k < kPlaceMaxPods ? pc.k : kPlaceMaxPods;  // (the host admits no more)
    Placement* const my_rows = rows + (int64_t)blockIdx.x * pc.k;

    // ---- every global read of the option ----
    uint64_t ekey[kSEnt];
    NodeV ent[kSEnt];
#pragma unroll
    for (int q = 0; q < kSEnt; ++q) {
        const int id = tid + q * kSRes;
        ekey[q] = 0ull;
        ent[q] = NodeV{};
        if (id < kEntries) {
            const int sh = id / kPlaceL;
            if (sh < pc.n_shapes) ekey[q] = top[id];
            (&lst[0][0])[id] = ekey[q];
            if (ekey[q]) {
                const uint32_t nd = place_key_node(ekey[q]);
                if (nd < (uint32_t)pc.n_nodes) ent[q] = place_load(s, state, n_pad, pc.sc, nd);
                else ekey[q] = 0ull;  // (no list holds a node outside the cluster: never flagged, never loaded)
            }
        }
    }
    if (tid < kPlaceMaxShapes) {
        const bool on = tid < pc.n_shapes;
        shp[tid] = on ? shapes[tid] : PodRec{};
        cc[tid] = on ? scaleup_count_start(pc.c, shapes[tid], tmpl, ccount[tid], max_nodes) : 0;
    }
    if (tid < kPlaceMaxPods) sof[tid] = tid < k ? (uint8_t)(shape_of[tid] & (kPlaceMaxShapes - 1)) : 0;
    __syncthreads();
    if (tid < kPlaceMaxShapes) {
        lflag[tid] = 0u;
        llen[tid] = place_list_len<kPlaceL>(lst[tid]);
    }
    __syncthreads();

    int32_t nchg = 0, u = 0, i = 0;
    int32_t n_ok = 0, n_over = 0, n_nf = 0, on_new = 0, first_un = -1;
    bool stopped = false;
    Placement mine{};  // pod tid's result: every thread knows every decision, thread i keeps pod i's
    for (; i < k; ++i) {
        const int sh = sof[i];
        const PodRec p = shp[sh];
        const int par = i & 1;
        const int32_t nev = nchg + (u < max_nodes ? 1 : 0);  // the changed nodes, then the fresh one
        uint64_t dk = 0ull;
        if (wave * kWave < nev) {  // uniform per wave
            if (tid < nchg) dk = place_key(pc.c, p, chg[tid], (uint32_t)chg_node[tid]);
            else if (tid == nchg) dk = scaleup_fresh_key(pc.c, p, tmpl, pc.n_nodes, u, max_nodes);
            const uint64_t m = wave_max_u64(dk);
            if (lane == 0) wmax[par][wave] = m;
        } else if (lane == 0) {
            wmax[par][wave] = 0ull;
        }
        __syncthreads();  // (A)
        uint64_t D = 0ull;  // D' of ks_device.h
#pragma unroll
        for (int w = 0; w < kSRes / kWave; ++w) D = wmax[par][w] > D ? wmax[par][w] : D;
        const int eS = place_first_unchanged<kPlaceL>(llen[sh], lflag[sh]);
        const uint64_t S = eS < kPlaceL ? lst[sh][eS] : 0ull;
        uint64_t W;
        const int dec = place_decide(S, lst[sh][kPlaceL - 1], D, &W);
        if (dec == kPlaceStop) {
            stopped = true;
            break;
        }
        const long long cand = cc[sh];
        if (dec == kPlaceNone) {
            if (tid == i) mine = Placement{-1, kPlaceNotFound, -1, cand};
            ++n_nf;
            if (first_un < 0) first_un = i;
            continue;
        }
        const uint32_t X = place_key_node(W);
        const bool from_d = W == D;  // S and D' are keys of different nodes: never equal
        const bool fresh = from_d && scaleup_takes_fresh(X, pc.n_nodes, u, max_nodes);
        if (from_d) {
            if (tid < nev && dk == W) {
                slot[par] = tid;
                if (fresh) {  // (tid == nchg: its key is the only one on node n + u)
                    chg[tid] = tmpl;
                    chg_node[tid] = (int32_t)X;
                }
            }
        } else {
            const int id = sh * kPlaceL + eS;
            if (tid == id % kSRes) {
#pragma unroll
                for (int q = 0; q < kSEnt; ++q)
                    if (q == id / kSRes) chg[nchg] = ent[q];
                chg_node[nchg] = (int32_t)X;
            }
        }
        __syncthreads();  // (B)
        // every thread has read lflag for this pod (all passed (B)); the next read is after the next (A)
        if (!from_d) {
#pragma unroll
            for (int q = 0; q < kSEnt; ++q)
                if (ekey[q] && place_key_node(ekey[q]) == X) {
                    const int me = tid + q * kSRes;
                    atomicOr(&lflag[me / kPlaceL], 1u << (me % kPlaceL));  // (LDS; several owners may share a word)
                }
        }
        const int32_t idx = from_d ? slot[par] : nchg;
        const NodeV before = chg[idx];
        NodeV after = before;
        const int32_t status = place_bind(p, after);
        if (status == kPlaceOk && tid < pc.n_shapes) cc[tid] += place_cand_delta(pc.c, shp[tid], before, after);
        if (tid == i) mine = Placement{(int32_t)X, status, (int64_t)(W >> 32) - 1, cand};
        if (status == kPlaceOk) {
            ++n_ok;
            on_new += X >= (uint32_t)pc.n_nodes;
        } else {
            ++n_over;
            if (first_un < 0) first_un = i;
        }
        __syncthreads();  // (C)
        if (tid == idx && status == kPlaceOk) chg[idx] = after;
        if (!from_d || fresh) ++nchg;
        if (fresh) ++u;
    }
    __syncthreads();
    // ---- the option's rows and summary; nothing is committed ----
    if (tid < i) my_rows[tid] = mine;
    // appended nodes that hold a pod: the template starts with none running
    const bool holds = tid < nchg && chg_node[tid] >= pc.n_nodes && chg[tid].nr > 0;
    const uint64_t bal = __ballot(holds);
    if (lane == 0) used[wave] = __popcll(bal);
    __syncthreads();
    if (tid == 0) {
        int32_t nu = 0;
        for (int w = 0; w < kSRes / kWave; ++w) nu += used[w];
        out[blockIdx.x] = ScaleResult{n_ok, n_over, n_nf, on_new, nu, first_un, stopped ? kScaleStopped : kScaleBatched, 0};
    }
}

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

hipError_t launch_scaleup_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ScaleBufs& sb,
                                  int32_t n_options, hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.n_shapes <= 0 || pc.n_shapes > kPlaceMaxShapes || pc.k <= 0 || pc.k > kPlaceMaxPods ||
        n_options <= 0 || n_options > kScaleMaxOptions)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(scaleup_resolve_kernel, dim3((unsigned)n_options), dim3(kSRes), 0, st, s, (const int64_t*)b.state,
                       b.n_pad, pc, b.shapes, b.shape_of, (const uint64_t*)b.top, (const long long*)b.ccount, sb.opts,
                       sb.rows, sb.out);
    return hipGetLastError();
}

hipError_t launch_scaleup_extend(const NodeSoA& s, int32_t n, const QScale& sc, const ScaleOption& opt, int64_t np_ext,
                                 int64_t* dst, hipStream_t st) {
    if (n < 0 || opt.max_nodes < 0 || opt.max_nodes > kScaleMaxNodes || np_ext < (int64_t)n + opt.max_nodes || np_ext <= 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(scaleup_extend_kernel, dim3((unsigned)((np_ext + 255) / 256)), dim3(256), 0, st, s, n, sc, opt,
                       np_ext, dst);
    return hipGetLastError();
}

}  // namespace ks
