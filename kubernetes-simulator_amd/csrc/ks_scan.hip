// ks_scan.hip — the scan family (gfx950): expire_head, scan, merge, merge_small.
//
// A batch's first half: the snapshot candidates of every pod, which a resolver then walks in FIFO
// order.  Who launches what (ks_step.cpp):
//   expire_head  the plain chain of the role-split and register-table resolvers, and a what-if
//                group's scenarios (ks_group_step): the expiries due before the batch's first pod.
//                The chunk resolver's chains apply them in window_prep instead (ks_prep.h).
//   scan         every chain.  One (256-node block, pod group) item per workgroup — the item's body
//                is ks_scan.h, shared with the chunk kernel's fused scan workers — into per-block
//                exact top-L lists.  The plain chain scans every batch; the overlapped chains scan a
//                pass's first batch here and later ones only as the conditional rescan (cond, pers).
//                For the chunk class the launch's first workgroups also stage the batch's E records
//                for merge_cl (stage).
//   merge        per pod the exact global top-L of its block lists by extraction rounds: the plain
//                chain off the chunk resolver, a sharded engine's per-part merges and, off the
//                chunk resolver, its second merge over the exchanged parts.  The chunk resolver's
//                own merge is merge_cl's score-class merge (ks_cand.hip).
//   merge_small  the same for <= 64 candidates per pod, one wave per pod — launch_merge picks it:
//                clusters of <= 2,048 nodes (what-if groups) and merges of <= 8 parts.
//
// Exactness of the lists: a node's key for a pod can differ from the snapshot only if a bind or an
// expiry of this batch touched the node; the resolvers re-evaluate those nodes themselves, and any
// node outside a pod's top-L scores below every entry of it.
//
// scan_kernel exists once per evaluator (ks_device.h: kEvalMicro, kEvalTiny, kEvalNarrow, kEvalWide;
// the host picks the narrowest that holds the cluster's capacities), key table width, list form
// (pruned or not) and list length.  Packed key: (total + 1) << 32 | (0xFFFFFFFF - node); 0 = no
// candidate (NotFound).  Max key = highest total, ties to the lowest node index.
#include <algorithm>

#include "ks_device.h"
#include "ks_scan.h"

namespace ks {

// Every batch kernel takes the device array of its engines' arguments: one engine for ks_step,
// a group's scenarios side by side for ks_group_step (BASELINE configs[3]: independent what-if
// clusters in one launch).  The scenario index is a grid dimension, so every field read is
// uniform (scalar loads).

// ------------------------------------------------------------------------------------------
// expire_head: grid (S).  Expiries due before the batch's first pod, applied straight to the
// node SoA.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void expire_head_kernel(const EngineArgs* __restrict__ A) {
    const EngineArgs a = A[blockIdx.x];
    const int64_t start = a.ctr[kCtrStart], end = a.ctr[kCtrEnd];
    if (a.ctr[kCtrErr] != 0 || start >= end) return;
    const int64_t e0 = a.exp_off[start], e1 = a.exp_off[start + 1];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += blockDim.x) {
        const int32_t q = a.exp_pod[e];
        if (a.b_status[q] != 0 || a.expired[q]) continue;
        const int32_t nd = a.b_node[q];
        const PodRec& p = a.pods[q];
        atomicAdd((unsigned long long*)&a.s.rc[nd], (unsigned long long)(-p.req[0]));
        atomicAdd((unsigned long long*)&a.s.rm[nd], (unsigned long long)(-p.req[1]));
        atomicAdd((unsigned long long*)&a.s.rg[nd], (unsigned long long)(-p.req[2]));
        atomicAdd((unsigned long long*)&a.s.nr[nd], (unsigned long long)(-1ll));
        a.expired[q] = 1;
    }
}

// ------------------------------------------------------------------------------------------
// scan: grid (blk_n, ceil(B / PG), S).  A workgroup owns one 256-node block (lane = node within
// its wave's 64) and PG pods.  Phase 1: every wave evaluates its nodes for all PG pods into an
// LDS key table (one u32 total+1 per pod and node).  Phase 2: one wave per pod extracts the
// block's exact top-L from the 256 keys (4 per lane).  Scores are small integers, so the top-L
// is usually one or two "tie classes": take the max, every node at it in node order, repeat below
// it — a lane max of 4, a 32-bit wave max and 4 ballots per class.
// ------------------------------------------------------------------------------------------
// KT: the key table's word, uint16_t when every total + 1 < 2^16 (the host's check on the scorer
// weights) — half the LDS per workgroup, so more workgroups fit a CU.
constexpr int kStageWgs = 8;  // workgroups staging the E records (grid-stride over n_e <= kEMax)
template <int kMode, typename KT, bool kPrune, int kLL>
__global__ __launch_bounds__(256) void scan_kernel(const EngineArgs* __restrict__ A, int xcd, int cond, int stage,
                                                   int pers) {
    extern __shared__ uint32_t kv_raw[];
    KT* const kv = reinterpret_cast<KT*>(kv_raw);  // [PG][kBlockNodes]: total+1 per (pod, node of the block)
    const EngineArgs& a = A[blockIdx.z];
    // stage: the chunk class — the first kStageWgs workgroups also stage the batch's E records for
    // merge_cl (WinWS::e_rec; one node per thread, grid-stride), before their own work.  launch_scan
    // launches at least kStageWgs workgroups when staging, also for a rank with no scan blocks.
    if (stage && blockIdx.x < kStageWgs) {
        const WinWS& ws = *a.sw;
        const int n_e = ws.n_e;
        for (int k = (int)blockIdx.x * kBlockNodes + (int)threadIdx.x; k < n_e; k += kStageWgs * kBlockNodes)
            put_rec12(a.sw->e_rec[k], load_node(a.s, ws.e_node[k]));
    }
    // cond: the overlap's fallback scan, needed only when window prep flagged a rescan
    if (cond && *(volatile const int32_t*)&a.sw->rescan == 0) return;
    const int64_t start = sload(a.ctr + kCtrStart), end = sload(a.ctr + kCtrEnd);
    if (sload(a.ctr + kCtrErr) != 0) return;
    const int64_t nb = min<int64_t>(a.B, end - start);
    if (nb <= 0) return;
    const int groups = (int)((nb + a.PG - 1) / a.PG);
    // work items (block, pod group), item = block * groups + group, one per workgroup: grid
    // (blk_n, groups, S), or — one engine (xcd) — a 1-D grid dealt XCD-aware: blocks b and b + 8
    // share an XCD (round-robin dispatch, MI355X_MICROARCH.md), so workgroup w takes item
    // (w % 8) * per + w / 8 — each XCD a contiguous item range, the groups of a node block on one
    // XCD back to back: the block's node records come from HBM once and from that XCD's L2 for
    // the other groups (the placement is for speed only; any placement gives the same lists)
    int64_t it_lo;
    if (xcd && pers) {  // (the pipelined engines' rescan: a fixed grid, each workgroup loops over its XCD's items)
        const int64_t tot = (int64_t)a.blk_n * groups, per = (tot + 7) / 8;
        const int64_t lo = (int64_t)(blockIdx.x % 8) * per, hi = min<int64_t>(tot, lo + per);
        for (int64_t it = lo + blockIdx.x / 8; it < hi; it += gridDim.x / 8) {
            if (it != lo + blockIdx.x / 8) __syncthreads();  // (the previous item's extraction has read kv)
            scn::scan_item<kMode, KT, kPrune, kLL>(a, kv, start, nb, groups, it, true, threadIdx.x, (int)(blockIdx.x % kThrCopies));
        }
        return;
    }
    if (xcd) {
        const int64_t tot = (int64_t)a.blk_n * groups, per = (tot + 7) / 8;
        const int64_t k = blockIdx.x / 8;
        if (k >= per) return;
        it_lo = (int64_t)(blockIdx.x % 8) * per + k;
        if (it_lo >= tot) return;
    } else {
        if ((int)blockIdx.x >= a.blk_n || (int)blockIdx.y >= groups) return;  // scenarios may differ in size
        it_lo = (int64_t)blockIdx.x * groups + blockIdx.y;
    }
    scn::scan_item<kMode, KT, kPrune, kLL>(a, kv, start, nb, groups, it_lo, true, threadIdx.x, (int)(blockIdx.x % kThrCopies));
}

// ------------------------------------------------------------------------------------------
// merge: grid (B, S), one workgroup per pod (256 threads, or 1024 for more than 1024 lists);
// exact top-L over nl sorted lists (the scan's block lists of one shard, or the shards'
// all-gathered lists).  src == nullptr: the scenario's own block lists into its candidate lists.
// ------------------------------------------------------------------------------------------
constexpr int kMergeMaxWaves = 16;
// bits != nullptr (a pruned engine's per-part merge, ks_scan.h): only the blocks pod b's bitmap
// bits[b * nwl ...] flags among blocks [blk0, blk0 + nl) (list k = block blk0 + k) are read
// kLL: the lists' length (kTopL; kTopLOverlap for the pipelined sharded engines' per-part merges)
template <int kLL>
__global__ __launch_bounds__(1024) void merge_kernel(const EngineArgs* __restrict__ A, const uint64_t* src,
                                                      int64_t pod_stride, int32_t nl, int64_t list_stride,
                                                      uint64_t* out, const uint64_t* bits, int32_t nwl, int32_t blk0,
                                                      int32_t lset_fixed) {
    const EngineArgs a = A[blockIdx.y];
    if (src == nullptr) {
        src = a.lists;
        pod_stride = (int64_t)a.nblk * kLL;
        nl = a.nblk;
        list_stride = kLL;
        out = a.cand;
    }
    const int64_t start = a.ctr[kCtrStart], end = a.ctr[kCtrEnd];
    if (a.ctr[kCtrErr] != 0) return;
    const int64_t nb = min<int64_t>(a.B, end - start);
    const int b = blockIdx.x;
    if (b >= nb) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t top[kLL];  // per-thread sorted (descending) top-L over its blocks
#pragma unroll
    for (int k = 0; k < kLL; ++k) top[k] = 0;
    const uint64_t* lists = src + (int64_t)b * pod_stride;
    const int nthr = blockDim.x, nwav = nthr / kWave;
    __shared__ scn::FlagLDS F;
    // (a sharded chunk engine's per-part merge: bits = the two sets, [2][B][nwl]; the batch's set is
    // the one its window prep named)
    // (lset_fixed >= 0: the pipelined engines' speculative part merges, which run beside the window
    // prep that rewrites a.sw->lset)
    const int lset = lset_fixed >= 0 ? lset_fixed : (bits && a.sw ? a.sw->lset : 1);
    const int nfl = bits ? scn::flagged_index(bits + ((int64_t)lset * a.B + b) * nwl, blk0, nl, F) : nl;
    for (int j = tid; j < nfl; j += nthr) {
        const int blk = bits ? scn::flagged_block(j, blk0, nl, F) : j;
        // the whole list in one round trip (16-byte loads), then the insertions
        const ulonglong2* lp = reinterpret_cast<const ulonglong2*>(lists + (int64_t)blk * list_stride);
        uint64_t lv[kLL];
#pragma unroll
        for (int k = 0; k < kLL / 2; ++k) {
            const ulonglong2 w = lp[k];
            lv[2 * k] = w.x;
            lv[2 * k + 1] = w.y;
        }
        topl_insert<kLL>(top, lv);
    }
    // each wave: L rounds of its max thread head (the owner advances), no barrier; then wave 0
    // merges the wave lists (<= 16 x kLL candidates, kPer per lane) the same way
    __shared__ uint64_t wl[kMergeMaxWaves][kLL];
    int head = 0;
    for (int r = 0; r < kLL; ++r) {
        uint64_t h = 0;
#pragma unroll
        for (int k = 0; k < kLL; ++k) h = (k == head) ? top[k] : h;
        const uint64_t m = wave_max_u64(h);
        const uint64_t hit = __ballot(h == m && m != 0);
        if (lane == 0) wl[wave][r] = m;
        if (hit && lane == __ffsll((unsigned long long)hit) - 1) head++;
    }
    __syncthreads();
    if (wave != 0) return;
    constexpr int kPer = (kMergeMaxWaves * kLL + kWave - 1) / kWave;
    const int nc = nwav * kLL;
    uint64_t v[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
        const int c = lane + q * kWave;
        v[q] = c < nc ? wl[c / kLL][c % kLL] : 0ull;
    }
#pragma unroll
    for (int r = 0; r < kLL; ++r) {
        uint64_t lm = v[0];
#pragma unroll
        for (int q = 1; q < kPer; ++q) lm = lm > v[q] ? lm : v[q];
        const uint64_t m = wave_max_u64(lm);
        if (lane == 0) out[(int64_t)b * kLL + r] = m;
        if (m == 0) continue;
        bool done = false;  // keys are distinct: exactly one holder
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const uint64_t h = __ballot(!done && v[q] == m);
            if (h && lane == __ffsll((unsigned long long)h) - 1) v[q] = 0;
            done = done || h != 0;
        }
    }
}

// merge_small: the same for nl * L <= 64 candidates per pod (clusters of <= 2048 nodes — a
// what-if group's scenarios — or a merge of <= 8 shards): one wave per pod, lane = candidate,
// L rounds of a wave max.  Grid (ceil(B / 4), S).
__global__ __launch_bounds__(256) void merge_small_kernel(const EngineArgs* __restrict__ A, const uint64_t* src,
                                                           int64_t pod_stride, int32_t nl, int64_t list_stride,
                                                           uint64_t* out) {
    const EngineArgs a = A[blockIdx.y];
    if (src == nullptr) {
        src = a.lists;
        pod_stride = (int64_t)a.nblk * kL;
        nl = a.nblk;
        list_stride = kL;
        out = a.cand;
    }
    const int64_t start = a.ctr[kCtrStart], end = a.ctr[kCtrEnd];
    if (a.ctr[kCtrErr] != 0) return;
    const int64_t nb = min<int64_t>(a.B, end - start);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int b = blockIdx.x * (blockDim.x / kWave) + wave;
    if (b >= nb) return;  // wave-uniform: the wave max below needs every lane
    const int li = lane / kL, le = lane % kL;
    uint64_t v = li < nl ? src[(int64_t)b * pod_stride + (int64_t)li * list_stride + le] : 0ull;
#pragma unroll
    for (int r = 0; r < kL; ++r) {
        const uint64_t m = wave_max_u64(v);
        if (lane == 0) out[(int64_t)b * kL + r] = m;
        const uint64_t hit = __ballot(v == m && m != 0);
        if (hit && lane == __ffsll((unsigned long long)hit) - 1) v = 0;
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers, called by the host code (ks_engine.cpp, ks_step.cpp, ks_queries.cpp).
// ---------------------------------------------------------------------------------------------
int max_pods_per_scan_wg() { return kMaxPG; }
int block_nodes() { return kBlockNodes; }

hipError_t launch_expire_head(const EngineArgs* d, int S, hipStream_t st) {
    hipLaunchKernelGGL(expire_head_kernel, dim3(S), dim3(256), 0, st, d);
    return hipGetLastError();
}

hipError_t launch_scan(const EngineArgs* d, int S, int blk_n, int B, int PG, int mode, bool key16, hipStream_t st,
                       const ScanOpts& o) {
    // (a staging launch runs even when this rank scans no blocks: merge_cl reads the E records)
    if ((blk_n > 0 || (o.stage && S == 1)) && S > 0) {
        // one (block, pod group) item per workgroup; one engine: the XCD-aware 1-D deal
        const int groups = (B + PG - 1) / PG;
        const size_t lds = (key16 ? sizeof(uint16_t) : sizeof(uint32_t)) * kBlockNodes * PG;
        const bool xcd = S == 1;
        int64_t wgs = std::max<int64_t>(((int64_t)blk_n * groups + 7) / 8 * 8, o.stage ? kStageWgs : 0);
        if (o.pw > 0 && S == 1) wgs = std::max<int64_t>(std::min<int64_t>(wgs, o.pw / 8 * 8), kStageWgs);  // (persistent)
        const dim3 g = xcd ? dim3((unsigned)wgs, 1, 1) : dim3(blk_n, groups, S);
        const int x = xcd ? 1 : 0, c = o.cond ? 1 : 0, sg = o.stage && xcd ? 1 : 0, pers = o.pw > 0 ? 1 : 0;
        // one instantiation per (evaluator, key width, pruned, list length); kt: a value of the key type
        auto go = [&](auto kt, auto prune, auto ll) {
            with_eval_mode(mode, [&](auto m) {
                hipLaunchKernelGGL((scan_kernel<decltype(m)::value, decltype(kt), decltype(prune)::value, decltype(ll)::value>),
                                   g, dim3(kBlockNodes), lds, st, d, x, c, sg, pers);
            });
        };
        using std::integral_constant;
        // (kTopLOverlap: the two-launch chain's lists and the pipelined sharded engines', ks_plan.h)
        if (o.L != kTopL && o.L != kTopLOverlap) return hipErrorInvalidValue;
        auto with_len = [&](auto kt, auto prune) {
            if (o.L != kTopL) go(kt, prune, integral_constant<int, kTopLOverlap>{});
            else go(kt, prune, integral_constant<int, kTopL>{});
        };
        auto with_prune = [&](auto kt) {
            if (o.prune) with_len(kt, std::true_type{});
            else with_len(kt, std::false_type{});
        };
        if (key16) with_prune(uint16_t{});
        else with_prune(uint32_t{});
    }
    return hipGetLastError();
}

hipError_t launch_merge(const EngineArgs* d, int S, int B, const ListSet& in, uint64_t* out, hipStream_t st,
                        const MergeOpts& o) {
    const dim3 g(B, S), t(in.nl_max > 1024 ? 1024 : 256);
    if (o.L == kTopLOverlap && o.L != kTopL) {
        hipLaunchKernelGGL(merge_kernel<kTopLOverlap>, g, t, 0, st, d, in.lists, in.pod_stride, in.nl, in.list_stride, out,
                           o.bits, o.nwl, o.blk0, o.lset_fixed);
    } else if (o.L != kTopL) {
        return hipErrorInvalidValue;
    } else if ((int64_t)in.nl_max * kL <= kWave && !o.bits) {
        hipLaunchKernelGGL(merge_small_kernel, dim3((B + 3) / 4, S), dim3(256), 0, st, d, in.lists, in.pod_stride, in.nl,
                           in.list_stride, out);
    } else {
        hipLaunchKernelGGL(merge_kernel<kTopL>, g, t, 0, st, d, in.lists, in.pod_stride, in.nl, in.list_stride, out, o.bits,
                           o.nwl, o.blk0, o.lset_fixed);
    }
    return hipGetLastError();
}
}  // namespace ks
