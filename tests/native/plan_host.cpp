// Host check of the step plan and the profile accounting (kubernetes-simulator_amd/csrc/ks_plan.h),
// for CPU tests only.  Both are compared with the formulas ks_step's body held before the plan was
// split out, restated here literally:
//   * ks_host_plan_check(): plan_step() over every combination of the three resolvers, overlap on /
//     off, speculative records present / absent, key16, blk_n in {0, 1, 256, 257}, parts in {1, 2, 16},
//     prune and the second stream, against the four booleans (fused, overlap, pipe, two) and the rule
//     for the list length;
//   * ks_host_account_check(): batch_record() and account_batch() for each chain (the plain chain
//     sharded and not, with each resolver class) at a pass's first, middle and last batch, with a
//     distinct duration per interval so that a swapped pair shows, against the accounting by event
//     index E[0..10] and the packed `kind` byte (1 window prep launched, 2 fused resolve, 4 sharded,
//     8 pipelined, 16 scan launched); the mark pairs of the ten intervals against those indices.
// Each returns the number of violated checks.  With -DKS_PLAN_MAIN the file is a stand-alone program
// (for a sanitizer build: -fsanitize=address,undefined on the host side).  Not part of the product.
#include <cstdio>
#include <cstring>

#include "../../kubernetes-simulator_amd/csrc/ks_plan.h"

namespace {

using namespace ks_host;

int64_t g_bad = 0;
void fail(const char* what, long long a, long long b, long long c) {
    if (g_bad++ < 20) std::fprintf(stderr, "plan: %s (%lld, %lld, %lld)\n", what, a, b, c);
}

// the event index each mark had: ev[0..4] in stream order around prep | scan | merge | resolve,
// ev[5], ev[6] after the part merges and the exchange, ev[7..10] on the second stream
int old_index(Mark m) {
    switch (m) {
        case kMarkBegin: return 0;
        case kMarkPrep: return 1;
        case kMarkScan: return 2;
        case kMarkMerge: return 3;
        case kMarkResolve: return 4;
        case kMarkParts: return 5;
        case kMarkXchg: return 6;
        case kMarkSideBegin: return 7;
        case kMarkSideScan: return 8;
        case kMarkSideParts: return 9;
        case kMarkSideXchg: return 10;
        default: return -1;
    }
}

// a distinct duration for each (from, to) pair of event indices the earlier accounting read
float el(int from, int to) {
    static const int pairs[10][2] = {{0, 1}, {1, 2}, {2, 5}, {5, 6}, {6, 3}, {2, 3}, {3, 4}, {7, 8}, {8, 9}, {9, 10}};
    static const float ms[10] = {1.0f, 2.5f, 4.25f, 8.125f, 16.0625f, 33.5f, 67.75f, 131.25f, 259.5f, 515.125f};
    for (int i = 0; i < 10; i++)
        if (pairs[i][0] == from && pairs[i][1] == to) return ms[i];
    fail("an interval the earlier accounting never read", from, to, 0);
    return 0;
}

bool same(const ks_kernel_stats& a, const ks_kernel_stats& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// One batch as the earlier loop body accounted it (kind as it packed it, E as it indexed it).
void old_account(uint8_t kind, ks_kernel_stats& ks, double& scan_ms, double& res_ms, double& other_ms) {
    float t[4] = {};
    if (kind & 8) {
        float w = el(0, 1), sc = el(1, 2), pm = el(2, 5), xc = el(5, 6), mg = el(6, 3), rs = el(3, 4);
        ks.wait_ms += w;
        ks.scan_ms += sc; ks.scan_n += 1; scan_ms += sc;
        ks.merge_ms += pm + xc + mg; ks.merge_n += 1; other_ms += pm + xc + mg + w;
        if (kind & 1) { ks.part_ms += pm; ks.xchg_ms += xc; ks.xchg_n += 1; }
        if (kind & 2) { ks.fused_ms += rs; ks.fused_n += 1; } else { ks.resolve_ms += rs; ks.resolve_n += 1; }
        res_ms += rs;
        if (kind & 2) {
            float a0 = el(7, 8), a1 = el(8, 9), a2 = el(9, 10);
            ks.side_scan_ms += a0; ks.side_part_ms += a1; ks.side_xchg_ms += a2; ks.side_n += 1;
        }
        return;
    }
    for (int k = 0; k < 4; k++) t[k] = el(k, k + 1);
    if (kind & 4) {
        float pm = el(2, 5), xc = el(5, 6);
        ks.part_ms += pm; ks.xchg_ms += xc;
        ks.xchg_n += 1;
    }
    other_ms += t[0] + t[2];
    scan_ms += t[1];
    res_ms += t[3];
    ks.prep_ms += t[0]; ks.prep_n += kind & 1;
    ks.scan_ms += t[1]; ks.scan_n += kind & 16 ? 1 : 0;
    ks.merge_ms += t[2]; ks.merge_n += 1;
    if (kind & 2) { ks.fused_ms += t[3]; ks.fused_n += 1; }
    else { ks.resolve_ms += t[3]; ks.resolve_n += 1; }
}

}  // namespace

extern "C" int64_t ks_host_plan_check() {
    g_bad = 0;
    int64_t combos = 0;
    for (int which : {(int)kResolveRole, (int)kResolveSmall, (int)kResolveChunk})
        for (int e_overlap = 0; e_overlap < 2; e_overlap++)
            for (int d_args_spec = 0; d_args_spec < 2; d_args_spec++)
                for (int key16 = 0; key16 < 2; key16++)
                    for (int blk_n : {0, 1, 256, 257})
                        for (int parts : {1, 2, 16})
                            for (int prune = 0; prune < 2; prune++)
                                for (int st2 = 0; st2 < 2; st2++) {
                                    // the earlier body, literally (kOverlapMaxBlocks = 256)
                                    const bool fused = which == kResolveChunk;
                                    const bool overlap = fused && e_overlap && d_args_spec && key16 && blk_n <= 256;
                                    const bool pipe = fused && !overlap && e_overlap && st2 && parts > 1;
                                    const bool two = overlap && parts == 1;
                                    const int L = (overlap && parts == 1 && !prune) || pipe ? ks::kTopLOverlap : ks::kTopL;
                                    const Chain want = pipe ? kChainPipe : two ? kChainTwoLaunch
                                                       : overlap ? kChainOverlapSharded : kChainPlain;
                                    PlanFacts f{};
                                    f.resolver = which;
                                    f.overlap = e_overlap;
                                    f.spec_args = d_args_spec;
                                    f.key16 = key16;
                                    f.blk_n = blk_n;
                                    f.parts = parts;
                                    f.prune = prune;
                                    f.side_stream = st2;
                                    const StepPlan p = plan_step(f);
                                    if (p.chain != want) fail("chain", p.chain, want, combos);
                                    if (p.L != L) fail("list length", p.L, L, combos);
                                    if (p.resolver != which) fail("resolver", p.resolver, which, combos);
                                    // the booleans the chains stood for, both ways
                                    if ((p.chain == kChainPipe) != pipe || (p.chain == kChainTwoLaunch) != two ||
                                        (p.chain == kChainTwoLaunch || p.chain == kChainOverlapSharded) != overlap)
                                        fail("booleans", p.chain, overlap, pipe);
                                    combos++;
                                }
    if (combos != 3 * 2 * 2 * 2 * 4 * 3 * 2 * 2) fail("combinations", combos, 0, 0);
    if (kOverlapMaxBlocks != 256) fail("kOverlapMaxBlocks", kOverlapMaxBlocks, 256, 0);
    return g_bad;
}

extern "C" int64_t ks_host_account_check() {
    g_bad = 0;
    if (kMarkCount != 11 || kIvCount != 10) fail("11 marks, 10 intervals", kMarkCount, kIvCount, 0);
    float t[kIvCount];
    for (int iv = 0; iv < kIvCount; iv++) t[iv] = el(old_index(kIntervalEnds[iv][0]), old_index(kIntervalEnds[iv][1]));
    for (int a = 0; a < kIvCount; a++)
        for (int b = a + 1; b < kIvCount; b++)
            if (t[a] == t[b]) fail("two intervals over one pair of marks", a, b, 0);
    struct Case { Chain chain; bool fused_resolver, sharded; };
    const Case cases[] = {{kChainPlain, false, false}, {kChainPlain, false, true}, {kChainPlain, true, false},
                          {kChainPlain, true, true},   {kChainOverlapSharded, true, true},
                          {kChainTwoLaunch, true, false}, {kChainPipe, true, true}};
    int64_t id = 0;
    for (const Case& c : cases)
        for (int pos = 0; pos < 4; pos++, id++) {  // first of several, middle, last, the only batch of its pass
            const int64_t nbat = pos == 3 ? 1 : 3, b = pos == 3 ? 0 : pos;
            // the earlier loop body's conditions, literally
            const bool pipe = c.chain == kChainPipe;
            const bool overlap = c.chain == kChainOverlapSharded || c.chain == kChainTwoLaunch;
            const bool two = c.chain == kChainTwoLaunch;
            const int G = c.sharded ? 2 : 1;
            uint8_t kind;
            if (pipe) {
                kind = (uint8_t)(8 | (b == 0 ? 1 : 0) | (b + 1 < nbat ? 2 : 0));
            } else {
                const bool spec = overlap && b > 0;
                const bool scan = !(two && spec);
                kind = (uint8_t)((!spec ? 1 : 0) | (overlap && b + 1 < nbat ? 2 : 0) | (G > 1 ? 4 : 0) | (scan ? 16 : 0));
            }
            ks_kernel_stats want{}, got{};
            double scan_ms = 0, res_ms = 0, other_ms = 0;
            StepSums sums;
            // twice: the sums accumulate
            for (int rep = 0; rep < 2; rep++) {
                old_account(kind, want, scan_ms, res_ms, other_ms);
                const BatchRecord r = batch_record(c.chain, b == 0, b + 1 < nbat, c.sharded);
                if (r.chain != c.chain || r.recorded != 0) fail("record", id, r.chain, r.recorded);
                account_batch(r, t, got, sums);
            }
            if (!same(want, got)) {
                fail("kernel statistics", id, kind, 0);
                std::fprintf(stderr, "  n: prep %lld/%lld scan %lld/%lld merge %lld/%lld resolve %lld/%lld fused %lld/%lld xchg %lld/%lld side %lld/%lld\n",
                             (long long)got.prep_n, (long long)want.prep_n, (long long)got.scan_n, (long long)want.scan_n,
                             (long long)got.merge_n, (long long)want.merge_n, (long long)got.resolve_n, (long long)want.resolve_n,
                             (long long)got.fused_n, (long long)want.fused_n, (long long)got.xchg_n, (long long)want.xchg_n,
                             (long long)got.side_n, (long long)want.side_n);
            }
            if (sums.scan_ms != scan_ms || sums.resolve_ms != res_ms || sums.other_ms != other_ms)
                fail("step sums", id, kind, 0);
        }
    // which intervals a batch's recorded marks give (the driver reads no event that was not recorded)
    BatchRecord r = batch_record(kChainTwoLaunch, true, true, false);
    for (Mark m : {kMarkBegin, kMarkPrep, kMarkScan, kMarkMerge, kMarkResolve}) r.recorded |= 1u << m;
    for (int iv = 0; iv < kIvCount; iv++) {
        const bool want = iv == kIvPrep || iv == kIvScan || iv == kIvMergeAll || iv == kIvResolve;
        if (interval_recorded(r, iv) != want) fail("interval_recorded", iv, want, 0);
    }
    return g_bad;
}

#ifdef KS_PLAN_MAIN
int main() {
    const int64_t bad = ks_host_plan_check() + ks_host_account_check();
    std::printf("plan check: %lld violated\n", (long long)bad);
    return bad != 0;
}
#endif
