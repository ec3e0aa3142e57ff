// ks_place_resolve.h — the previews' resolver: one pod loop on the snapshot lists (gfx950, wave64).
//
// ks_place.hip instantiates it for the placement rounds and the scale-up preview,
// ks_consolidate.hip for the consolidation rounds, ks_gang.hip for the gang admission rounds.  Device code only; each translation unit gets its
// own instantiations.
#pragma once
#include "ks_query.h"

namespace ks {
namespace {

constexpr int kPRes = 1024;     // threads of the resolver: one per changed node
constexpr int kPEnt = (kPlaceMaxShapes * kPlaceL + kPRes - 1) / kPRes;  // list entries a resolver thread owns
static_assert(kPlaceMaxPods <= kPRes, "a resolver thread per changed node, and one for the fresh node");

__device__ __forceinline__ bool shape_active(uint64_t active, int sh) { return (active >> sh) & 1ull; }

// ---------------------------------------------------------------------------------------------
// Resolver: one pod loop, instantiated four times, a workgroup of kPRes threads each.  LDS holds the
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
// kCons = true, the consolidation preview's rounds (ks_consolidate_at): one workgroup walks the
// candidates [c0, c1) of ConsRound in order; pods [0, k) are their pods, candidate after candidate.
// A candidate is a transaction around the same pod loop (the argument is in ks_query.h, above
// consolidate_route):
//   open    (where the previous candidate ended; one loop closes a candidate and opens the next, so a
//           candidate without pods is accepted by its next turn) a candidate that is a destination —
//           in the changed set, or in `received` from an earlier round — is answered and its pods
//           are skipped.  Otherwise lflag[], cc[] (copies in LDS) and nchg are kept;
//           the entry owners flag the list entries on the candidate's node and shape j's count
//           drops by place_is_cand(shape j, the candidate's record): the candidate is never S, so
//           never a winner, never in the changed set, never in D;
//   pods    the loop below; pod i's slot is kept too;
//   accept  (every pod bound Ok, or none) the kept values are dropped: the flags and the counts stay
//           as they are for the rest of the round; thread 0 zeroes the node's row of the scratch
//           and sets its cordon bit;
//   block   (a pod is not bound Ok) thread j of an Ok pod of the attempt takes its masked requests
//           and one running pod back out of its slot (LDS atomics: several pods may share a slot,
//           integer adds commute; place_bind is additive, so this is exact); lflag, cc and nchg get
//           their kept values back — slots the attempt appended fall off the end; the candidate's
//           later pods are skipped;
//   stop    (kPlaceStop inside a candidate) the same roll-back, and the round ends: the candidate
//           opens the next round.
// This is the one instantiation that reads global memory inside the loop: once per candidate its
// table entry (a scalar load), its `received` word and its node's record.
// The round commits the changed nodes like the placement rounds, sets their `received` bits and
// reports the next candidate in rb.  Cordon and received bits are set with global atomic ORs whose
// results nobody reads in this launch: ORs commute.
// kGang = true, the gang admission preview's rounds (ks_gang_at): one workgroup walks the gangs
// [g0, g1) of GangRound in order; pods [0, k) are their pods, gang after gang.  A gang is the same
// transaction with less around it (the argument is in ks_query.h, above gang_route):
//   open    lflag[], cc[] (copies in LDS) and nchg are kept; nothing is flagged, no count corrected;
//   pods    the loop below; pod i's slot is kept; a pod not bound Ok counts (uniform) and the attempt
//           ends once more than size - min_ok of them did;
//   admit   (at least min_ok pods bound Ok at the gang's end) the kept values are dropped;
//   block   thread j of a tried pod whose own status is Ok takes its requests and one running pod
//           back out of its kept slot; lflag, cc and nchg get their kept values back; the gang's
//           later pods are not tried; with GangRound::strict the round ends and reports m;
//   stop    (kPlaceStop inside a gang) the same roll-back, and the round ends: the gang opens the next.
// Inside the loop it reads global memory once per gang: its table entry (a scalar load).
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

// What a consolidation round keeps between a candidate's opening and its end.
template <bool kCons>
struct ConsRegs {};
template <>
struct ConsRegs<true> {
    int32_t a, node = -1, count = 0;  // the candidate: its index, node and pods
    int32_t beg = 0, end = 0;         // its pods among the round's
    bool open = false;                // a transaction is open
    int32_t nchg_s = 0;               // nchg at the opening
    int32_t blk = -1, blk_status = 0; // the pod that ended the attempt unbound, and its status
};
// ... and in LDS: lflag[] and cc[] at the opening, and every pod's slot (registers are short: DESIGN.md 3.8)
template <bool kCons>
struct ConsKept {};
template <>
struct ConsKept<true> {
    uint32_t lflag[kPlaceMaxShapes];
    long long cc[kPlaceMaxShapes];
    uint16_t slot[kPlaceMaxPods];
};
struct NoRound {};

// What a gang round keeps between a gang's opening and its end (in LDS: ConsKept<true>).
template <bool kGang>
struct GangRegs {};
template <>
struct GangRegs<true> {
    int32_t a, first = 0, size = 0, allow = 0;  // the gang: its index, rows, and size - min_ok
    int32_t beg = 0, end = 0, tried = 0;        // its pods among the round's; the end of those tried
    bool open = false, blocked = false, strict_end = false;
    int32_t nchg_s = 0;                         // nchg at the opening
    int32_t n_ok = 0, n_over = 0, n_nf = 0, blk_status = 0;
};
template <bool kCons, bool kGang>
using RoundArg = std::conditional_t<kCons, ConsRound, std::conditional_t<kGang, GangRound, NoRound>>;

template <bool kScale, bool kCons = false, bool kGang = false>
__global__ __launch_bounds__(kPRes) void resolve_kernel(NodeSoA s, std::conditional_t<kScale, const int64_t*, int64_t*> state,
                                                        int64_t n_pad, PlaceCfg pc, const PodRec* __restrict__ shapes,
                                                        const int32_t* __restrict__ shape_of,
                                                        const uint64_t* __restrict__ top,
                                                        const long long* __restrict__ ccount,
                                                        const ScaleOption* __restrict__ opt, Placement* rows,
                                                        ScaleResult* __restrict__ res, int32_t first, uint64_t active,
                                                        int32_t* rb, RoundArg<kCons, kGang> cr) {
    static_assert(!(kScale && (kCons || kGang)) && !(kCons && kGang), "a round of transactions commits; an option does not");
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
    if constexpr (kCons || kGang) first = 0;
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
    ConsRegs<kCons> cn;
    GangRegs<kGang> gn;
    [[maybe_unused]] __shared__ ConsKept<kCons || kGang> kept;
    if constexpr (kCons) cn.a = cr.c0 - 1;
    if constexpr (kGang) {
        gn.a = cr.g0 - 1;
        mine = Placement{-1, kGangNotTried, -1, 0};  // (a pod no attempt reached)
    }
    for (; kCons || kGang || i < k; ++i) {
        if constexpr (kGang) {
            // uniform: no gang is open, or the open one has no pod left to try (or never had one)
            while (i == gn.end) {
                if (gn.open && (gn.blocked || stopped)) {  // roll back
                    __syncthreads();  // the last pod's slot is written, every read of lflag / cc / chg is done
                    if (tid >= gn.beg && tid < gn.tried && mine.status == kPlaceOk && kept.slot[tid] < gn.nchg_s) {
                        const PodRec& q = shp[sof[tid]];  // an Ok pod on a kept slot
                        unsigned long long* v = (unsigned long long*)&chg[kept.slot[tid]].rc;  // rc rm rg nr
                        for (int c = 0; c < 3; ++c)
                            if (q.keymask >> c & 1) atomicAdd(v + c, 0ull - (unsigned long long)q.req[c]);
                        atomicAdd(v + 3, ~0ull);
                    }
                    if (tid < kPlaceMaxShapes) {
                        lflag[tid] = kept.lflag[tid];
                        cc[tid] = kept.cc[tid];
                    }
                    nchg = gn.nchg_s;
                    if (!stopped && tid == 0)
                        cr.out[gn.a] = Gang{gn.first, gn.size, kGangBlocked, gn.tried - gn.beg, gn.n_ok, gn.n_over, gn.n_nf,
                                            gn.blk_status};
                    if (!stopped && cr.strict) gn.strict_end = true;
                    __syncthreads();
                } else if (gn.open && tid == 0) {  // at least min_ok pods bound Ok: admitted
                    cr.out[gn.a] = Gang{gn.first, gn.size, kGangAdmitted, gn.size, gn.n_ok, gn.n_over, gn.n_nf, 0};
                }
                gn.open = false;
                gn.blocked = false;
                if (stopped || gn.strict_end || ++gn.a >= cr.g1) break;  // (stopped: the rolled-back gang opens the next round)
                // ---- the next gang opens ----
                const GangIn gd = sload(cr.gangs + gn.a);
                gn.first = gd.first;
                gn.size = gd.size;
                const int64_t b0 = (int64_t)gd.first - cr.row0, b1 = b0 + gd.size;
                gn.beg = b0 < 0 ? 0 : b0 > k ? k : (int32_t)b0;  // (the host's rows: within [0, k])
                gn.end = b1 < gn.beg ? gn.beg : b1 > k ? k : (int32_t)b1;
                gn.tried = gn.end;
                const int32_t mo = gd.min_ok < 0 ? 0 : gd.min_ok > gd.size ? gd.size : gd.min_ok;  // (the host checked)
                gn.allow = gd.size - mo;
                gn.n_ok = gn.n_over = gn.n_nf = gn.blk_status = 0;
                if (tid < kPlaceMaxShapes) {  // (read back by the same thread alone)
                    kept.lflag[tid] = lflag[tid];
                    kept.cc[tid] = cc[tid];
                }
                gn.nchg_s = nchg;
                gn.open = true;
                i = gn.beg;  // (== gn.end for an empty gang: admitted by the next turn of this loop)
            }
            if (stopped || gn.strict_end || gn.a >= cr.g1) break;
        }
        if constexpr (kCons) {
            // uniform: no candidate is open, or the open one has no pod left (or never had one)
            while (i == cn.end) {
                if (cn.open && cn.blk >= 0) {  // pod blk was not bound Ok (or stopped the round): roll back
                    __syncthreads();  // the last pod's slot is written, every read of lflag / cc / chg is done
                    if (tid >= cn.beg && tid < cn.blk && kept.slot[tid] < cn.nchg_s) {  // an Ok pod on a kept slot
                        const PodRec& q = shp[sof[tid]];
                        unsigned long long* v = (unsigned long long*)&chg[kept.slot[tid]].rc;  // rc rm rg nr
                        for (int c = 0; c < 3; ++c)
                            if (q.keymask >> c & 1) atomicAdd(v + c, 0ull - (unsigned long long)q.req[c]);
                        atomicAdd(v + 3, ~0ull);
                    }
                    if (tid < kPlaceMaxShapes) {
                        lflag[tid] = kept.lflag[tid];
                        cc[tid] = kept.cc[tid];
                    }
                    nchg = cn.nchg_s;
                    if (!stopped && tid == 0)
                        cr.out[cn.a] = Consolidation{cn.node, cn.count, kConsBlocked, cn.blk - cn.beg + 1, cn.blk_status, 0,
                                                     cr.row0 + cn.beg};
                    __syncthreads();
                } else if (cn.open && tid == 0) {  // every pod bound Ok, or none runs there: removed
                    cr.out[cn.a] = Consolidation{cn.node, cn.count, kConsRemoved, cn.count, 0, 0, cr.row0 + cn.beg};
                    atomicOr(cr.cordon + (cn.node >> 5), 1u << (cn.node & 31));
                    for (int c = 0; c < 4; ++c) state[c * n_pad + cn.node] = 0;
                }
                cn.open = false;
                cn.blk = -1;
                if (stopped || ++cn.a >= cr.c1) break;  // (stopped: the rolled-back candidate opens the next round)
                // ---- the next candidate opens ----
                const RemovalCand cd = sload(cr.cands + cn.a);
                cn.node = cd.node;
                cn.count = cd.count;
                const int64_t b0 = cd.first - cr.row0, b1 = b0 + cd.count;
                cn.beg = b0 < 0 ? 0 : b0 > k ? k : (int32_t)b0;  // (the host's rows: within [0, k])
                cn.end = b1 < cn.beg ? cn.beg : b1 > k ? k : (int32_t)b1;
                const bool real = (uint32_t)cd.node < (uint32_t)pc.n_nodes;  // (the host checked)
                if (tid < kPlaceMaxShapes) {  // kept before any flag of this candidate is set
                    kept.lflag[tid] = lflag[tid];
                    kept.cc[tid] = cc[tid];
                }
                cn.nchg_s = nchg;
                const bool got = !real || ((cr.received[cd.node >> 5] >> (cd.node & 31)) & 1u) ||
                                 (tid < nchg && chg_node[tid] == cd.node);
                // (readfirstlane: the OR is the same in every lane and the compiler must see that, or every
                // index that follows would live in vector registers)
                if (__builtin_amdgcn_readfirstlane(__syncthreads_or(got))) {  // a destination: nothing is tried
                    if (tid == 0)
                        cr.out[cn.a] = Consolidation{cd.node, cd.count, kConsDestination, 0, 0, 0, cr.row0 + cn.beg};
                    i = cn.end;  // (its pods are skipped)
                    continue;
                }
#pragma unroll
                for (int q = 0; q < kPEnt; ++q)
                    if (ekey[q] && place_key_node(ekey[q]) == (uint32_t)cd.node) {
                        const int me = tid + q * kPRes;
                        atomicOr(&lflag[me / kPlaceL], 1u << (me % kPlaceL));
                    }
                if (tid < pc.n_shapes)
                    cc[tid] -= (long long)place_is_cand(pc.c, shp[tid], place_load(s, state, n_pad, pc.sc, cd.node));
                cn.open = true;
                i = cn.beg;  // (== cn.end when no pod runs on it: accepted by the next turn of this loop)
                __syncthreads();  // the flags and the counts, before the candidate's first pod reads them
            }
            if (stopped || cn.a >= cr.c1) break;
        }
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
        uint64_t D = 0ull;  // (scale-up: D' of ks_query.h)
#pragma unroll
        for (int w = 0; w < kPRes / kWave; ++w) D = wmax[par][w] > D ? wmax[par][w] : D;
        const int eS = place_first_unchanged<kPlaceL>(llen[sh], lflag[sh]);
        const uint64_t S = eS < kPlaceL ? lst[sh][eS] : 0ull;
        uint64_t W;
        const int dec = place_decide(S, lst[sh][kPlaceL - 1], D, &W);
        if (dec == kPlaceStop) {
            if constexpr (kScale) stopped = true;
            if constexpr (kCons) {  // the open candidate is rolled back (above) and starts the next round
                stopped = true;
                cn.blk = i;
                i = cn.end - 1;
                continue;
            }
            if constexpr (kGang) {  // the open gang is rolled back (above) and starts the next round
                stopped = true;
                gn.tried = i;
                i = gn.end - 1;
                continue;
            }
            break;
        }
        const long long cand = cc[sh];
        if (dec == kPlaceNone) {
            if (tid == i) mine = Placement{-1, kPlaceNotFound, -1, cand};
            if constexpr (kScale) {
                ++su.n_nf;
                if (su.first_un < 0) su.first_un = i;
            }
            if constexpr (kCons) {
                cn.blk = i;
                cn.blk_status = kPlaceNotFound;
                i = cn.end - 1;
            }
            if constexpr (kGang) {
                ++gn.n_nf;
                if (gn.n_over + gn.n_nf > gn.allow) {
                    gn.blocked = true;
                    gn.blk_status = kPlaceNotFound;
                    gn.tried = i + 1;
                    i = gn.end - 1;
                }
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
        if constexpr (kCons || kGang)
            if (tid == i) kept.slot[i] = (uint16_t)idx;
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
        if constexpr (kCons)
            if (status != kPlaceOk) {
                cn.blk = i;
                cn.blk_status = status;
                i = cn.end - 1;
            }
        if constexpr (kGang) {
            if (status == kPlaceOk) {
                ++gn.n_ok;
            } else if (++gn.n_over + gn.n_nf > gn.allow) {
                gn.blocked = true;
                gn.blk_status = status;
                gn.tried = i + 1;
                i = gn.end - 1;
            }
        }
    }
    __syncthreads();
    // ---- the decided pods' rows (consolidation: a skipped pod's row is never read) ----
    if constexpr (kCons) i = stopped ? cn.beg : k;  // (stopped: cn.a is still the rolled-back candidate)
    if constexpr (kGang) i = stopped ? gn.beg : k;  // (an untried pod's row says so)
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
        if constexpr (kCons) {
            if (tid < nchg) atomicOr(cr.received + (chg_node[tid] >> 5), 1u << (chg_node[tid] & 31));
            if (tid == 0) {  // the next candidate, 1 if the round decided none, the changed nodes, the pods before it
                rb[0] = cn.a;
                rb[1] = cn.a == cr.c0 ? 1 : 0;
                rb[2] = nchg;
                rb[3] = i;
            }
        } else if constexpr (kGang) {
            if (tid == 0) {  // the next gang (m: a strict pass is over), 1 if the round decided none
                rb[0] = gn.strict_end ? cr.m : gn.a;
                rb[1] = !gn.strict_end && gn.a == cr.g0 ? 1 : 0;
                rb[2] = nchg;
                rb[3] = i;
            }
        } else if (tid == 0) {
            rb[0] = i;
            rb[1] = i == first ? 1 : 0;
            rb[2] = nchg;
            rb[3] = 0;
        }
    }
}

}  // namespace
}  // namespace ks
