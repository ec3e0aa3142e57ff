// ks_plan.h — what a batched ks_step decides before its first launch and how it accounts its
// profile afterwards (host only, no HIP calls: ks_step.cpp runs it, tests/native/plan_host.cpp
// checks it without a device).
//  * StepPlan: which of the four launch chains the step's batches take and the block lists' length.
//  * Mark / BatchRecord: the profile marks a chain records around its launches, by name, and what
//    one batch launched.
//  * account_batch: a batch's mark intervals into ks_kernel_stats and ks_step_stats' sums.
#pragma once
#include <stdint.h>

#include "../../include/ks_engine.h"
#include "ks_device.h"

namespace ks_host {

// the fused overlap's limit on a rank's scan blocks (plan_step)
#ifndef KS_OVERLAP_MAX_BLOCKS
#define KS_OVERLAP_MAX_BLOCKS 256
#endif
constexpr int kOverlapMaxBlocks = KS_OVERLAP_MAX_BLOCKS;

// Resolvers, the same binds: the role-split resolve_kernel (16 waves, ks_rolesplit.hip) takes any
// engine; the register-table resolver (4 waves, ks_resolve.hip) is lighter — four per CU, so a
// what-if group's resolvers run side by side (C4 2.29e11 against 2.16e11 evals/s with the
// role-split kernel's half-size class); the chunk resolver (ks_chunk.hip) takes one
// engine per launch, batches of <= kWinMaxB pods, and runs fused into the batch chain.
enum Resolver { kResolveRole = 0, kResolveSmall = 1, kResolveChunk = 4 };

// The launch chain of a step's batches (ks_step.cpp has one function per chain):
//  * plain: prep -> scan -> merge -> resolve, four launches per batch; any resolver, any sharding.
//  * overlap, sharded: the chunk kernel of batch b carries batch b + 1's scan of this rank's blocks
//    (and its window prep), over the pods after batch b (the speculative counters window prep writes);
//    every rank's lists are speculative alike and its touched nodes (the same on every rank: the
//    resolvers are identical) join E; the exchange runs every batch whether or not window prep
//    flagged a rescan, so every rank issues the same collectives.
//  * two-launch (the overlap on one shard): an overlapped batch is merge_cl -> chunk kernel, with no
//    conditional scan launch in front; merge_cl reads its E nodes from the node table and the
//    constants table; a window prep that must rescan publishes an empty batch instead, whose round's
//    fused scan lists the same pods again (ks_prep.h).
//  * pipelined (sharded engines the fused overlap does not take, e.g. C5 on 8 ranks, 512 blocks
//    each): batch b + 1's speculative scan, per-part merges and exchange run on a second stream
//    beside batch b's resolve, so only the resolve (with the next window in its tail), the E staging
//    and merge_cl stay on the critical path.
enum Chain { kChainPlain, kChainOverlapSharded, kChainTwoLaunch, kChainPipe };

struct StepPlan {
    int resolver;  // Resolver
    Chain chain;
    int L;  // the block lists' length: kTopL, or kTopLOverlap where speculative lists go stale
};

// The facts the choice rests on.
struct PlanFacts {
    int resolver;      // resolver_of(e)
    bool overlap;      // the engine allows it (no KS_ENGINE_NO_OVERLAP)
    bool spec_args;    // the speculative scan's argument records exist (ensure_window_ws)
    bool key16;        // every total + 1 fits the scan's 16-bit key table
    int blk_n;         // this rank's scan blocks
    int parts;         // world * vsh
    bool prune;        // pruned block lists
    bool side_stream;  // the second stream exists
};

// In the fused kernel the scan runs one workgroup per CU (the resolver's LDS fixes the kernel's),
// ~3 blocks per us: ranks scanning more than kOverlapMaxBlocks blocks keep their scan at full
// occupancy (C5 on 8 ranks, 512 blocks each: fused kernel 129 us against a 78 us resolve + a 37 us
// scan; C3: 196 blocks hide under the resolve).  Profiling does not change the plan: the marks
// bracket the same launches.
inline StepPlan plan_step(const PlanFacts& f) {
    const bool fused = f.resolver == kResolveChunk;
    const bool overlap = fused && f.overlap && f.spec_args && f.key16 && f.blk_n <= kOverlapMaxBlocks;
    const bool pipe = fused && !overlap && f.overlap && f.side_stream && f.parts > 1;
    StepPlan p{f.resolver, kChainPlain, ks::kTopL};
    if (pipe) p.chain = kChainPipe;
    else if (overlap) p.chain = f.parts == 1 ? kChainTwoLaunch : kChainOverlapSharded;
    // the two-launch chain's lists are longer (ks_device.h kTopLOverlap, ks_cand.hip cand_list), and
    // the pipelined chain's: its speculative lists go stale like the overlap's
    if ((p.chain == kChainTwoLaunch && !f.prune) || p.chain == kChainPipe) p.L = ks::kTopLOverlap;
    return p;
}

// ---- the early read-back -------------------------------------------------------------------------
// A pass enqueues its ceil(n / B) rounds blind and waits once, after the last.  On a two-launch pass
// of at least kEarlyMinRounds rounds the host takes a snapshot of the start counter after round
// early_round() (a kernel boundary: every bind below it is visible) and copies and finishes the
// binds below it while the last kEarlyK rounds run: ~0.55 ms of device work at C3, about twice the
// host's work on a 32,768-pod step, and the ~1,100 binds of those rounds are all that is left after
// the wait.  -1: no snapshot (shorter passes, the other chains).
#ifndef KS_EARLY_READBACK
#define KS_EARLY_READBACK 1  // (A/B: make variant NAME=noearly DEFS=-DKS_EARLY_READBACK=0)
#endif
constexpr int kEarlyMinRounds = 16;
constexpr int kEarlyK = 6;
inline int64_t early_round(int64_t rounds, Chain chain) {
    return KS_EARLY_READBACK && chain == kChainTwoLaunch && rounds >= kEarlyMinRounds ? rounds - 1 - kEarlyK : -1;
}

// ---- profile marks ---------------------------------------------------------------------------
// One pooled HIP event per mark and batch while profiling is on.  A chain records the marks around
// its launches in stream order; a mark it does not reach is not recorded for that batch.
enum Mark {
    kMarkBegin,      // main stream: before the batch's first launch
    kMarkPrep,       // after the window prep / expire_head (pipelined: after the wait for the side exchange)
    kMarkScan,       // after the scan (or where an overlapped batch has none)
    kMarkParts,      // sharded: after this rank's part merges
    kMarkXchg,       // sharded: after the exchange
    kMarkMerge,      // after the merge / merge_cl
    kMarkResolve,    // after the resolve launch
    kMarkSideBegin,  // pipelined chain's second stream: before the next batch's speculative scan
    kMarkSideScan,
    kMarkSideParts,
    kMarkSideXchg,
    kMarkCount
};

// What one batch launched.
struct BatchRecord {
    Chain chain;
    bool prep_launched;  // a window prep / expire_head launch (not inside the previous chunk kernel)
    bool scan_launched;  // a scan launch
    bool fused;          // the resolve launch carried the next batch's scan or window
    bool sharded;        // part merges and an exchange
    uint32_t recorded;   // bit m: mark m was recorded
};

// The record of a batch of `chain` at its position in the pass (first: nothing speculative precedes
// it; more: another batch follows, whose scan or window the resolve launch carries).
inline BatchRecord batch_record(Chain chain, bool first, bool more, bool sharded) {
    switch (chain) {
        case kChainPlain: return BatchRecord{chain, true, true, false, sharded, 0};
        case kChainOverlapSharded: return BatchRecord{chain, first, true, more, true, 0};  // (later batches: the conditional rescan)
        case kChainTwoLaunch: return BatchRecord{chain, first, first, more, false, 0};
        default: return BatchRecord{chain, first, true, more, true, 0};  // pipelined (later batches: the conditional rescan)
    }
}

// The intervals between marks that the accounting reads.
enum Interval {
    kIvPrep,       // begin -> prep
    kIvScan,       // prep -> scan
    kIvParts,      // scan -> part merges
    kIvXchg,       // part merges -> exchange
    kIvMergeTail,  // exchange -> merge
    kIvMergeAll,   // scan -> merge (with a sharded engine's part merges and exchange)
    kIvResolve,    // merge -> resolve
    kIvSideScan,
    kIvSideParts,
    kIvSideXchg,
    kIvCount
};
constexpr Mark kIntervalEnds[kIvCount][2] = {
    {kMarkBegin, kMarkPrep},        {kMarkPrep, kMarkScan},          {kMarkScan, kMarkParts},
    {kMarkParts, kMarkXchg},        {kMarkXchg, kMarkMerge},         {kMarkScan, kMarkMerge},
    {kMarkMerge, kMarkResolve},     {kMarkSideBegin, kMarkSideScan}, {kMarkSideScan, kMarkSideParts},
    {kMarkSideParts, kMarkSideXchg}};
inline bool interval_recorded(const BatchRecord& r, int iv) {
    return (r.recorded >> kIntervalEnds[iv][0] & 1) && (r.recorded >> kIntervalEnds[iv][1] & 1);
}

// ks_step_stats' three sums
struct StepSums {
    double scan_ms = 0, resolve_ms = 0, other_ms = 0;
};

// One batch's intervals (ms; 0 where not recorded) into the step's kernel statistics and sums.
// The pipelined chain: its first interval is the wait for the side stream's exchange (a pass's
// first batch: its window prep, so that falls in wait_ms and prep_n is never counted); part merges
// and the exchange are on the main stream only in a pass's first batch (later batches record those
// marks back to back).
inline void account_batch(const BatchRecord& r, const float* t, ks_kernel_stats& ks, StepSums& s) {
    const float rs = t[kIvResolve];
    if (r.chain == kChainPipe) {
        const float w = t[kIvPrep], sc = t[kIvScan], pm = t[kIvParts], xc = t[kIvXchg], mg = t[kIvMergeTail];
        ks.wait_ms += w;
        ks.scan_ms += sc; ks.scan_n += 1; s.scan_ms += sc;
        ks.merge_ms += pm + xc + mg; ks.merge_n += 1; s.other_ms += pm + xc + mg + w;
        if (r.prep_launched) { ks.part_ms += pm; ks.xchg_ms += xc; ks.xchg_n += 1; }
        if (r.fused) {
            ks.side_scan_ms += t[kIvSideScan]; ks.side_part_ms += t[kIvSideParts]; ks.side_xchg_ms += t[kIvSideXchg];
            ks.side_n += 1;
        }
    } else {
        if (r.sharded) { ks.part_ms += t[kIvParts]; ks.xchg_ms += t[kIvXchg]; ks.xchg_n += 1; }
        s.other_ms += t[kIvPrep] + t[kIvMergeAll];
        s.scan_ms += t[kIvScan];
        ks.prep_ms += t[kIvPrep]; ks.prep_n += r.prep_launched ? 1 : 0;
        ks.scan_ms += t[kIvScan]; ks.scan_n += r.scan_launched ? 1 : 0;  // (scan launches actually made)
        ks.merge_ms += t[kIvMergeAll]; ks.merge_n += 1;
    }
    if (r.fused) { ks.fused_ms += rs; ks.fused_n += 1; }
    else { ks.resolve_ms += rs; ks.resolve_n += 1; }
    s.resolve_ms += rs;
}

}  // namespace ks_host
