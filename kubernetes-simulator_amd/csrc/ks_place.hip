// ks_place.hip — placement preview: where k more pods would be bound at a past tick (gfx950).
//
// ks_place_at hands k preview pods, one after another, to scheduleOne's Filter -> Score -> argmax ->
// CreatePod (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60) on a private copy of the state
// at tick t: the 4 x N_pad scratch requested_kernel (ks_query.hip) rebuilds from the binds, here in
// milli-units (or, when every request is a whole multiple of the engine's unit, in device units:
// place_whole_units, ks_query.h).  The engine's node table, its lists and its resolvers are not involved; the kernels
// read the cluster's constants (alloc, taints, labels) and write the scratch only.
//
// The call runs in rounds (the exactness argument is in ks_query.h, above place_decide):
//   place_scan_kernel     per 256-node block and active shape the block's exact top-L keys and its
//                         candidate count;
//   place_merge_kernel    per active shape the exact global top-L (topl_insert) and the count;
//   resolve_kernel<false> one workgroup decides pods in order until one cannot be decided from the
//                         lists and the changed nodes, commits the changed nodes to the scratch and
//                         reports the first undecided pod (the pod loop is ks_place_resolve.h's, which
//                         ks_consolidate.hip and ks_gang.hip instantiate again).
// The scale-up preview (ks_scale_up_at, ks_scaleup.hip) runs the same pod loop on the same lists:
//   resolve_kernel<true>  one workgroup per option decides the k pods in order, its changed set
//                         private in LDS, the unchanged appended nodes stood for by the first of
//                         them (the argument is in ks_query.h, above scaleup_fresh_key); it commits
//                         nothing and reads top / ccount / state read-only.
// Integers only, no global atomics, no communication between workgroups.  The resolver sets flag
// bits with LDS atomics: the sets of one pod commute with each other, and barriers separate them
// from every read of the flags, so the result does not depend on the order of execution.
#include "ks_query.h"
#include "ks_place_resolve.h"

namespace ks {
namespace {

constexpr int kPBlk = 256;      // nodes per scan workgroup
constexpr int kPChunk = 16;     // shapes per pass over the scan's key table (32 KB of LDS)
static_assert(kPBlk == 4 * kWave, "the extraction reads four keys per lane");

// ---------------------------------------------------------------------------------------------
// Scan: a node's ten words are loaded once; the shape records are workgroup-uniform (scalar loads).
// Per pass of kPChunk shapes every thread writes its key into tab[shape][thread]; then each wave
// takes shapes of the pass: four keys per lane, L times a wave max (DPP) whose owner drops its key —
// keys are distinct, so exactly one lane does.  lists[(shape * nblk + block) * L ..] descending,
// 0-padded; cnt[shape * nblk + block] the block's non-zero keys.
// kCordon (ks_drain_at): a node whose bit is set in `cordon` gets key 0 for every shape — it is in
// no list and no count (the argument is in ks_query.h, above launch_place_round).
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

// (the resolver, resolve_kernel: ks_place_resolve.h)

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
                       (ScaleResult*)nullptr, first, active, b.rb, NoRound{});
    return hipGetLastError();
}

hipError_t launch_scaleup_resolve(const NodeSoA& s, const PlaceCfg& pc, const PlaceBufs& b, const ScaleBufs& sb,
                                  int32_t n_options, hipStream_t st) {
    if (pc.n_nodes <= 0 || pc.n_shapes <= 0 || pc.n_shapes > kPlaceMaxShapes || pc.k <= 0 || pc.k > kPlaceMaxPods ||
        n_options <= 0 || n_options > kScaleMaxOptions)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(resolve_kernel<true>, dim3((unsigned)n_options), dim3(kPRes), 0, st, s, (const int64_t*)b.state,
                       b.n_pad, pc, b.shapes, b.shape_of, (const uint64_t*)b.top, (const long long*)b.ccount, sb.opts,
                       sb.rows, sb.out, 0, ~0ull, (int32_t*)nullptr, NoRound{});
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
