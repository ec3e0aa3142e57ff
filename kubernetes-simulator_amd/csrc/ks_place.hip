// ks_place.hip — placement preview: where k more pods would be bound at a past tick (gfx950).
//
// ks_place_at hands k preview pods, one after another, to scheduleOne's Filter -> Score -> argmax ->
// CreatePod (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60) on a private copy of the state
// at tick t: the 4 x N_pad scratch requested_kernel (ks_query.hip) rebuilds from the binds, here in
// milli-units (or, when every request is a whole multiple of the engine's unit, in device units:
// place_whole_units, ks_device.h).  The engine's node table, its lists and its resolvers are not involved; the kernels
// read the cluster's constants (alloc, taints, labels) and write the scratch only.
//
// The call runs in rounds (the exactness argument is in ks_device.h, above place_decide):
//   place_scan_kernel     per 256-node block and active shape the block's exact top-L keys and its
//                         candidate count;
//   place_merge_kernel    per active shape the exact global top-L (topl_insert) and the count;
//   resolve_kernel<false> one workgroup decides pods in order until one cannot be decided from the
//                         lists and the changed nodes, commits the changed nodes to the scratch and
//                         reports the first undecided pod.
// The scale-up preview (ks_scale_up_at, ks_scaleup.hip) runs the same pod loop on the same lists:
//   resolve_kernel<true>  one workgroup per option decides the k pods in order, its changed set
//                         private in LDS, the unchanged appended nodes stood for by the first of
//                         them (the argument is in ks_device.h, above scaleup_fresh_key); it commits
//                         nothing and reads top / ccount / state read-only.
// Integers only, no global atomics, no communication between workgroups.  The resolver sets flag
// bits with LDS atomics: the sets of one pod commute with each other, and barriers separate them
// from every read of the flags, so the result does not depend on the order of execution.
#include "ks_device.h"

namespace ks {
namespace {

constexpr int kPBlk = 256;      // nodes per scan workgroup
constexpr int kPChunk = 16;     // shapes per pass over the scan's key table (32 KB of LDS)
constexpr int kPRes = 1024;     // threads of the resolver: one per changed node
constexpr int kPEnt = (kPlaceMaxShapes * kPlaceL + kPRes - 1) / kPRes;  // list entries a resolver thread owns
static_assert(kPlaceMaxPods <= kPRes, "a resolver thread per changed node, and one for the fresh node");
static_assert(kPBlk == 4 * kWave, "the extraction reads four keys per lane");

__device__ __forceinline__ bool shape_active(uint64_t active, int sh) { return (active >> sh) & 1ull; }

// ---------------------------------------------------------------------------------------------
// Scan: a node's ten words are loaded once; the shape records are workgroup-uniform (scalar loads).
// Per pass of kPChunk shapes every thread writes its key into tab[shape][thread]; then each wave
// takes shapes of the pass: four keys per lane, L times a wave max (DPP) whose owner drops its key —
// keys are distinct, so exactly one lane does.  lists[(shape * nblk + block) * L ..] descending,
// 0-padded; cnt[shape * nblk + block] the block's non-zero keys.
// kCordon (ks_drain_at): a node whose bit is set in `cordon` gets key 0 for every shape — it is in
// no list and no count (the argument is in ks_device.h, above launch_place_round).
// ---------------------------------------------------------------------------------------------
template <bool kCordon>
__global__ __launch_bounds__(kPBlk) void place_scan_kernel(NodeSoA s, const int64_t* __restrict__ state, int64_t n_pad,
                                                          PlaceCfg pc, const PodRec* __restrict__ shapes,
                                                          uint64_t active, uint64_t* __restrict__ lists,
                                                          int32_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ cordon) {
    __shared__ uint64_t tab[kPChunk][kPBlk];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int32_t nd = blockIdx.x * kPBlk + threadIdx.x;
    bool real = nd < pc.n_nodes;
    if constexpr (kCordon) real = real && !drain_cordoned(cordon, nd);
    NodeV v{};
    if (real) v = place_load(s, state, n_pad, pc.sc, nd);
    for (int base = 0; base < pc.n_shapes; base += kPChunk) {
        for (int j = 0; j < kPChunk; ++j) {
            const int sh = base + j;
            if (sh >= pc.n_shapes || !shape_active(active, sh)) continue;  // uniform
            const PodRec p = sload(shapes + sh);
            tab[j][threadIdx.x] = real ? place_key(pc.c, p, v, (uint32_t)nd) : 0ull;
        }
        __syncthreads();
        for (int j = wave; j < kPChunk; j += kPBlk / kWave) {
            const int sh = base + j;
            if (sh >= pc.n_shapes || !shape_active(active, sh)) continue;  // uniform per wave
            uint64_t k0 = tab[j][lane], k1 = tab[j][lane + 64], k2 = tab[j][lane + 128], k3 = tab[j][lane + 192];
            int32_t c = (k0 != 0) + (k1 != 0) + (k2 != 0) + (k3 != 0);
            for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
            uint64_t* dst = lists + ((int64_t)sh * pc.nblk + blockIdx.x) * kPlaceL;
            for (int e = 0; e < kPlaceL; ++e) {
                const uint64_t a = k0 > k1 ? k0 : k1, b = k2 > k3 ? k2 : k3;
                const uint64_t m = wave_max_u64(a > b ? a : b);
                if (lane == 0) dst[e] = m;
                k0 = k0 == m ? 0ull : k0;
                k1 = k1 == m ? 0ull : k1;
                k2 = k2 == m ? 0ull : k2;
                k3 = k3 == m ? 0ull : k3;
            }
            if (lane == 0) cnt[(int64_t)sh * pc.nblk + blockIdx.x] = c;
        }
        __syncthreads();
    }
}

// Merge: one wave per shape.  Each lane folds the block lists b = lane, lane + 64, ... into its own
// top-L (topl_insert); the global top-L is then L wave maxes over the lanes' heads (keys are distinct:
// one lane owns each maximum and pops it).  The counts are summed alongside.
__global__ __launch_bounds__(kWave) void place_merge_kernel(const uint64_t* __restrict__ lists,
                                                            const int32_t* __restrict__ cnt, int32_t nblk,
                                                            uint64_t active, uint64_t* __restrict__ top,
                                                            long long* __restrict__ ccount) {
    const int sh = blockIdx.x, lane = threadIdx.x;
    if (!shape_active(active, sh)) return;
    uint64_t t[kPlaceL];
#pragma unroll
    for (int e = 0; e < kPlaceL; ++e) t[e] = 0ull;
    long long c = 0;
    for (int32_t b = lane; b < nblk; b += kWave) {
        const uint64_t* l = lists + ((int64_t)sh * nblk + b) * kPlaceL;
        uint64_t lv[kPlaceL];
#pragma unroll
        for (int e = 0; e < kPlaceL; ++e) lv[e] = l[e];
        topl_insert<kPlaceL>(t, lv);
        c += cnt[(int64_t)sh * nblk + b];
    }
    for (int o = kWave / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, kWave);
    // the lanes' lists are sorted: L times the wave max of their heads, whose owner pops its head
    for (int e = 0; e < kPlaceL; ++e) {
        const uint64_t m = wave_max_u64(t[0]);
        if (lane == 0) top[sh * kPlaceL + e] = m;
        if (m && t[0] == m) {
#pragma unroll
            for (int x = 0; x + 1 < kPlaceL; ++x) t[x] = t[x + 1];
            t[kPlaceL - 1] = 0ull;
        }
    }
    if (lane == 0) ccount[sh] = c;
}

// ---------------------------------------------------------------------------------------------
// Resolver: one pod loop, instantiated twice, a workgroup of kPRes threads each.  LDS holds the
// lists and their flags, the shapes, the pods' shape indices, the running candidate counts and the
// changed set (node + its ten words, current state; the call's units, PlaceCfg::sc).  Every global
// read is issued before the pod loop: list entry (shape, e) belongs to thread (shape * L + e) %
// kPRes, which keeps that entry's node record in registers and hands it to the changed set when the
// entry wins.
//
// Per pod (uniform control flow, three barriers):
//   thread c < nchg evaluates changed node c; waves reduce (DPP), wmax[] holds the waves' maxima;
//   (A) every thread folds wmax into D, finds S (place_first_unchanged) and decides (place_decide);
//   the winner joins the changed set (from its entry owner's registers) unless it is in it — then
//   the thread whose key is D names its slot;
//   (B) the entry owners flag the list entries on the winner's node — only now, when every thread
//   has taken its S from the flags: a flag set before (B) could reach a wave that has not decided
//   yet and give it another S; every thread reads the winner's record; place_bind decides Ok /
//   OverCapacity; lanes = shapes adjust the running counts by place_cand_delta; thread i keeps pod
//   i's result in registers (a global store per pod would put an HBM round trip under the next
//   barrier's wait);
//   (C) the slot's own thread writes the new state: it alone reads that slot before the next (A).
// All loops are bounded by k, L and the changed set (<= the pods decided <= kPlaceMaxPods).
//
// Three guards change nothing on any input the host admits (k <= kPlaceMaxPods, shape_of < n_shapes
// <= kPlaceMaxShapes, list keys of nodes < n_nodes) and keep every LDS index in range on any other:
// k is clamped, shape_of is masked to 6 bits, and a list key whose node lies outside the cluster is
// dropped (never loaded, never flagged).
//
// kScale = false, the placement preview's rounds: one workgroup decides pods [first, k) of the shapes
// in `active` until kPlaceStop ends the round, commits the changed nodes to the scratch and reports
// the first undecided pod in rb.
// kScale = true, the scale-up preview: one workgroup per option (opt, rows and res at blockIdx.x)
// decides pods [0, k) of every shape with the option's appended nodes on D's side.  Thread nchg —
// the first thread without a changed node — evaluates the fresh node n + u on the empty template
// (scaleup_fresh_key), so the wave maxima give D' = max(D, F) with no further step.  When its key
// wins, the same thread puts the template into slot nchg and names the slot; nchg and u grow by one
// (scaleup_takes_fresh).  nchg <= the pods decided < k <= kPRes inside the loop, so thread nchg
// exists.  kPlaceStop ends the option: path = kScaleStopped and the rows are the host's to fill.
// Nothing is committed; the state is read only.  The option, the template, max_nodes, ScaleRegs,
// `stopped` and used[] are this instantiation's alone: in the other they are empty or unused
// constants and leave no register behind.
// ---------------------------------------------------------------------------------------------
template <bool kScale>
struct ScaleRegs {};
template <>
struct ScaleRegs<true> {
    int32_t u = 0;  // appended nodes in the changed set: n .. n + u - 1
    int32_t n_ok = 0, n_over = 0, n_nf = 0, on_new = 0, first_un = -1;
};
// The option as the kernel reads it: blockIdx.x's record for scale-up, an empty one for place.
struct NoOption {
    struct {} tmpl;
    int32_t max_nodes;
};
template <bool kScale>
__device__ __forceinline__ std::conditional_t<kScale, ScaleOption, NoOption> scale_option(const ScaleOption* opts) {
    if constexpr (kScale) return sload(opts + blockIdx.x);
    else return {};
}

template <bool kScale>
__global__ __launch_bounds__(kPRes) void resolve_kernel(NodeSoA s, std::conditional_t<kScale, const int64_t*, int64_t*> state,
                                                        int64_t n_pad, PlaceCfg pc, const PodRec* __restrict__ shapes,
                                                        const int32_t* __restrict__ shape_of,
                                                        const uint64_t* __restrict__ top,
                                                        const long long* __restrict__ ccount,
                                                        const ScaleOption* __restrict__ opt, Placement* rows,
                                                        ScaleResult* __restrict__ res, int32_t first, uint64_t active,
                                                        int32_t* rb) {
    __shared__ NodeV chg[kPlaceMaxPods];
    __shared__ int32_t chg_node[kPlaceMaxPods];
    __shared__ uint64_t lst[kPlaceMaxShapes][kPlaceL];
    __shared__ uint32_t lflag[kPlaceMaxShapes];  // bit e: entry e's node is in the changed set
    __shared__ int32_t llen[kPlaceMaxShapes];
    __shared__ PodRec shp[kPlaceMaxShapes];
    __shared__ long long cc[kPlaceMaxShapes];
    __shared__ uint8_t sof[kPlaceMaxPods];
    __shared__ uint64_t wmax[2][kPRes / kWave];
    __shared__ int32_t slot[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    constexpr int kEntries = kPlaceMaxShapes * kPlaceL;
    // (plain const locals and a plain bool for `stopped`, as scaleup_resolve_kernel had them: with the
    // template or the flag held in a record that the loop also updates, scaleup_fresh_key's fit tests
    // came out as branches and the kernel needed another VGPR)
    const auto option = scale_option<kScale>(opt);
    [[maybe_unused]] const auto tmpl = option.tmpl;
    [[maybe_unused]] const int32_t max_nodes =
        option.max_nodes < 0 ? 0 : option.max_nodes > kScaleMaxNodes ? kScaleMaxNodes : option.max_nodes;
    const int32_t k = pc.k < kPlaceMaxPods ? pc.k : kPlaceMaxPods;
    if constexpr (kScale) {
        first = 0;
        rows += (int64_t)blockIdx.x * pc.k;
    }
    const auto listed = [&](int sh) { return sh < pc.n_shapes && (kScale || shape_active(active, sh)); };

    // ---- every global read of the round / the option ----
    uint64_t ekey[kPEnt];
    NodeV ent[kPEnt];
#pragma unroll
    for (int q = 0; q < kPEnt; ++q) {
        const int id = tid + q * kPRes;
        ekey[q] = 0ull;
        ent[q] = NodeV{};
        if (id < kEntries) {
            if (listed(id / kPlaceL)) ekey[q] = top[id];
            (&lst[0][0])[id] = ekey[q];
            if (ekey[q]) {
                const uint32_t nd = place_key_node(ekey[q]);
                if (nd < (uint32_t)pc.n_nodes) ent[q] = place_load(s, state, n_pad, pc.sc, nd);
                else ekey[q] = 0ull;  // (no list holds a node outside the cluster: never flagged, never loaded)
            }
        }
    }
    if (tid < kPlaceMaxShapes) {
        shp[tid] = tid < pc.n_shapes ? shapes[tid] : PodRec{};
        long long c0 = 0;
        if (listed(tid)) {
            c0 = ccount[tid];
            if constexpr (kScale) c0 = scaleup_count_start(pc.c, shapes[tid], tmpl, c0, max_nodes);
        }
        cc[tid] = c0;
    }
    if (tid < kPlaceMaxPods) sof[tid] = tid >= first && tid < k ? (uint8_t)(shape_of[tid] & (kPlaceMaxShapes - 1)) : 0;
    __syncthreads();
    if (tid < kPlaceMaxShapes) {
        lflag[tid] = 0u;
        llen[tid] = place_list_len<kPlaceL>(lst[tid]);
    }
    __syncthreads();

    int32_t nchg = 0, i = first;
    ScaleRegs<kScale> su;
    [[maybe_unused]] bool stopped = false;
    Placement mine{};  // pod tid's result: every thread knows every decision, thread i keeps pod i's
    for (; i < k; ++i) {
        const int sh = sof[i];
        const PodRec p = shp[sh];
        const int par = i & 1;
        int32_t nev = nchg;  // the slots evaluated: the changed nodes, then (scale-up) the fresh one
        if constexpr (kScale) nev += su.u < max_nodes ? 1 : 0;
        uint64_t dk = 0ull;
        if (wave * kWave < nev) {  // uniform per wave
            if (tid < nchg) {
                dk = place_key(pc.c, p, chg[tid], (uint32_t)chg_node[tid]);
            } else if constexpr (kScale) {  // (one evaluation per thread: the fresh key is the else side)
                if (tid == nchg) dk = scaleup_fresh_key(pc.c, p, tmpl, pc.n_nodes, su.u, max_nodes);
            }
            const uint64_t m = wave_max_u64(dk);
            if (lane == 0) wmax[par][wave] = m;
        } else if (lane == 0) {
            wmax[par][wave] = 0ull;
        }
        __syncthreads();  // (A)
        uint64_t D = 0ull;  // (scale-up: D' of ks_device.h)
#pragma unroll
        for (int w = 0; w < kPRes / kWave; ++w) D = wmax[par][w] > D ? wmax[par][w] : D;
        const int eS = place_first_unchanged<kPlaceL>(llen[sh], lflag[sh]);
        const uint64_t S = eS < kPlaceL ? lst[sh][eS] : 0ull;
        uint64_t W;
        const int dec = place_decide(S, lst[sh][kPlaceL - 1], D, &W);
        if (dec == kPlaceStop) {
            if constexpr (kScale) stopped = true;
            break;
        }
        const long long cand = cc[sh];
        if (dec == kPlaceNone) {
            if (tid == i) mine = Placement{-1, kPlaceNotFound, -1, cand};
            if constexpr (kScale) {
                ++su.n_nf;
                if (su.first_un < 0) su.first_un = i;
            }
            continue;
        }
        const uint32_t X = place_key_node(W);
        const bool from_d = W == D;  // S and D are keys of different nodes: never equal
        bool fresh = false;
        if constexpr (kScale) fresh = from_d && scaleup_takes_fresh(X, pc.n_nodes, su.u, max_nodes);
        if (from_d) {
            if (tid < nev && dk == W) {
                slot[par] = tid;
                if constexpr (kScale)
                    if (fresh) {  // (tid == nchg: its key is the only one on node n + u)
                        chg[tid] = tmpl;
                        chg_node[tid] = (int32_t)X;
                    }
            }
        } else {
            const int id = sh * kPlaceL + eS;
            if (tid == id % kPRes) {
#pragma unroll
                for (int q = 0; q < kPEnt; ++q)
                    if (q == id / kPRes) chg[nchg] = ent[q];
                chg_node[nchg] = (int32_t)X;
            }
        }
        __syncthreads();  // (B)
        // every thread has read lflag for this pod (all passed (B)); the next read is after the next (A)
        if (!from_d) {
#pragma unroll
            for (int q = 0; q < kPEnt; ++q)
                if (ekey[q] && place_key_node(ekey[q]) == X) {
                    const int me = tid + q * kPRes;
                    atomicOr(&lflag[me / kPlaceL], 1u << (me % kPlaceL));  // (LDS; several owners may share a word)
                }
        }
        const int32_t idx = from_d ? slot[par] : nchg;
        const NodeV before = chg[idx];
        NodeV after = before;
        const int32_t status = place_bind(p, after);
        if (status == kPlaceOk && tid < pc.n_shapes) cc[tid] += place_cand_delta(pc.c, shp[tid], before, after);
        if (tid == i) mine = Placement{(int32_t)X, status, (int64_t)(W >> 32) - 1, cand};
        if constexpr (kScale) {
            if (status == kPlaceOk) {
                ++su.n_ok;
                su.on_new += X >= (uint32_t)pc.n_nodes;
            } else {
                ++su.n_over;
                if (su.first_un < 0) su.first_un = i;
            }
        }
        __syncthreads();  // (C)
        if (tid == idx && status == kPlaceOk) chg[idx] = after;
        if (!from_d || fresh) ++nchg;
        if constexpr (kScale)
            if (fresh) ++su.u;
    }
    __syncthreads();
    // ---- the decided pods' rows ----
    if (tid >= first && tid < i) rows[tid] = mine;
    if constexpr (kScale) {
        // the option's summary; appended nodes that hold a pod: the template starts with none running
        __shared__ int32_t used[kPRes / kWave];
        const bool holds = tid < nchg && chg_node[tid] >= pc.n_nodes && chg[tid].nr > 0;
        const uint64_t bal = __ballot(holds);
        if (lane == 0) used[wave] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            int32_t nu = 0;
            for (int w = 0; w < kPRes / kWave; ++w) nu += used[w];
            res[blockIdx.x] = ScaleResult{su.n_ok, su.n_over, su.n_nf, su.on_new, nu, su.first_un,
                               stopped ? kScaleStopped : kScaleBatched, 0};
        }
    } else {
        // the changed nodes to the scratch, and the round's 16 bytes
        if (tid < nchg) {
            const int64_t nd = chg_node[tid];
            state[nd] = chg[tid].rc;
            state[n_pad + nd] = chg[tid].rm;
            state[2 * n_pad + nd] = chg[tid].rg;
            state[3 * n_pad + nd] = chg[tid].nr;
        }
        if (tid == 0) {
            rb[0] = i;
            rb[1] = i == first ? 1 : 0;
            rb[2] = nchg;
            rb[3] = 0;
        }
    }
}

__global__ __launch_bounds__(256) void place_after_kernel(const int64_t* __restrict__ state, int64_t n_pad,
                                                          int32_t n_nodes, QScale sc, long long* __restrict__ after) {
    const int32_t nd = blockIdx.x * 256 + threadIdx.x;
    if (nd >= n_nodes) return;
#pragma unroll
    for (int c = 0; c < 4; ++c) after[(int64_t)nd * 4 + c] = state[c * n_pad + nd] * (c < 3 ? sc.f[c] : 1);
}

}  // namespace

hipError_t launch_place_lists(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, uint64_t active, hipStream_t st,
                              const uint32_t* cordon) {
    if (pc.n_nodes <= 0 || pc.n_shapes <= 0 || pc.n_shapes > kPlaceMaxShapes ||
        pc.nblk != (pc.n_nodes + kPBlk - 1) / kPBlk)
        return hipErrorInvalidValue;
    const auto scan = cordon ? place_scan_kernel<true> : place_scan_kernel<false>;
    hipLaunchKernelGGL(scan, dim3((unsigned)pc.nblk), dim3(kPBlk), 0, st, s, (const int64_t*)b.state, b.n_pad, pc,
                       b.shapes, active, b.lists, b.cnt, cordon);
    hipLaunchKernelGGL(place_merge_kernel, dim3((unsigned)pc.n_shapes), dim3(kWave), 0, st, (const uint64_t*)b.lists,
                       (const int32_t*)b.cnt, pc.nblk, active, b.top, b.ccount);
    return hipGetLastError();
}

hipError_t launch_place_round(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, int32_t first, uint64_t active,
                              hipStream_t st, const uint32_t* cordon) {
    if (pc.k <= 0 || pc.k > kPlaceMaxPods || first < 0 || first >= pc.k) return hipErrorInvalidValue;
    if (hipError_t r = launch_place_lists(s, pc, b, active, st, cordon); r != hipSuccess) return r;
    hipLaunchKernelGGL(resolve_kernel<false>, dim3(1), dim3(kPRes), 0, st, s, b.state, b.n_pad, pc, b.shapes, b.shape_of,
                       (const uint64_t*)b.top, (const long long*)b.ccount, (const ScaleOption*)nullptr, b.out,
                       (ScaleResult*)nullptr, first, active, b.rb);
    return hipGetLastError();
}

hipError_t launch_scaleup_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ScaleBufs& sb,
                                  int32_t n_options, hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.n_shapes <= 0 || pc.n_shapes > kPlaceMaxShapes || pc.k <= 0 || pc.k > kPlaceMaxPods ||
        n_options <= 0 || n_options > kScaleMaxOptions)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(resolve_kernel<true>, dim3((unsigned)n_options), dim3(kPRes), 0, st, s, (const int64_t*)b.state,
                       b.n_pad, pc, b.shapes, b.shape_of, (const uint64_t*)b.top, (const long long*)b.ccount, sb.opts,
                       sb.rows, sb.out, 0, ~0ull, (int32_t*)nullptr);
    return hipGetLastError();
}

hipError_t launch_place_after(const int64_t* state, int64_t n_pad, int32_t n_nodes, const QScale& sc, long long* after,
                              hipStream_t st) {
    if (n_nodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(place_after_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, st, state, n_pad,
                       n_nodes, sc, after);
    return hipGetLastError();
}

}  // namespace ks
