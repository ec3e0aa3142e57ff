// ks_selftest.cpp — the device self-tests of include/ks_engine.h (ks_selftest, ks_selftest_eval):
// the evaluators of ks_device.h run on the device over the caller's cases.  They need no engine.
#include <algorithm>
#include <functional>
#include <vector>

#include "ks_host.h"  // kMaxValue: the value range ks_load_nodes / ks_submit_pods accept

using ks_host::kMaxValue;

namespace {

// The evaluator mode of a ks_selftest_eval column and whether the column holds the node in 32-bit words.
struct EvColumn { int mode; bool words; };
EvColumn ev_column(int bit) {
    if (bit == ks::kEvScanCol) return {ks::kEvalMicro, false};
    const int col = bit < ks::kEvPruneBit ? bit : bit - ks::kEvPruneBit;
    const int group = col / 4;
    // totals: NodeV, record, NS32, conv; bounds: NodeV, NS32, conv (conv's wide entry is a NodeV)
    const bool words = bit < ks::kEvPruneBit ? (group == 1 || group == 2) : group == 1;
    return {col % 4, words};
}

// The batch respects what ks_load_nodes / ks_submit_pods guarantee every evaluator (values in range,
// usage within its capacity) and the domain of every requested column's evaluator (update_mode).
bool ev_batch_valid(const ks::Cfg& c, int64_t n, const int64_t* alloc, const int64_t* run, const int64_t* req,
                    uint32_t variants) {
    bool need[4] = {false, false, false, false}, words = false;
    for (int b = 0; b < ks::kEvPruneBit + ks::kEvPruneCols; b++) {
        if (!((variants >> b) & 1u)) continue;
        const EvColumn col = ev_column(b);
        need[col.mode] = true;
        words |= col.words;
    }
    if (need[ks::kEvalMicro] && (c.w_lr >= ks::kMicroWeight || c.w_ba >= ks::kMicroWeight)) return false;
    for (int64_t i = 0; i < n; i++) {
        const int64_t* a = alloc + i * 4;
        const int64_t* r = run + i * 4;
        for (int k = 0; k < 3; k++) {
            if (a[k] < -1 || a[k] >= kMaxValue) return false;
            if (r[k] < 0 || r[k] > std::max<int64_t>(a[k], 0)) return false;
            if (req[i * 3 + k] < 0 || req[i * 3 + k] >= kMaxValue) return false;
        }
        if (a[3] < 0 || a[3] >= kMaxValue || r[3] < 0 || r[3] >= INT32_MAX) return false;  // (nr < ap stays exact with ap clamped to INT_MAX)
        const int64_t m = std::max(std::max(a[0], a[1]), a[2]);
        const int64_t prod = m < ks::kTinyCap ? std::max<int64_t>(a[0], 0) * std::max<int64_t>(a[1], 0) : 0;
        if (words && m >= (int64_t)0xFFFFFFFF) return false;
        if (need[ks::kEvalNarrow] && m >= ks::kNarrowCap) return false;
        if (need[ks::kEvalTiny] && (m >= ks::kTinyCap || prod >= ks::kTinyCap)) return false;
        if (need[ks::kEvalMicro] && (m >= ks::kMicroCap || prod >= ks::kMicroProd)) return false;
    }
    return true;
}

// ---- KS_SELFTEST_LIST_MERGE: merge_cl's list merge against the host fold ----------------------
// A case: per-node totals (total + 1, 0 = infeasible) over nl 256-node blocks.  Its block lists are
// each block's top-L keys; `prune` cuts them to a threshold prefix as the pruned scan does (ks_scan.h:
// any key that L keys reach is a valid threshold, and blocks read different ones): none, the last key
// of the first full list, or the exact L-th key, by block index.
struct MergeCase { int nl, threads; bool prune; std::vector<uint32_t> tot; };

template <int L>
void merge_case_lists(const MergeCase& c, std::vector<uint64_t>& lists, uint64_t (&want)[L]) {
    constexpr int kBlk = 256;
    lists.assign((size_t)c.nl * L, 0ull);
    std::vector<uint64_t> keys;
    for (int b = 0; b < c.nl; b++) {
        keys.clear();
        for (int t = 0; t < kBlk; t++) {
            const size_t n = (size_t)b * kBlk + t;
            const uint64_t k = n < c.tot.size() ? ks::make_key(c.tot[n], (uint32_t)n) : 0ull;
            if (k) keys.push_back(k);
        }
        std::sort(keys.begin(), keys.end(), std::greater<uint64_t>());
        for (size_t k = 0; k < keys.size() && k < (size_t)L; k++) lists[(size_t)b * L + k] = keys[k];
    }
    auto fold = [&](uint64_t (&top)[L]) {
        for (int k = 0; k < L; k++) top[k] = 0;
        for (int b = 0; b < c.nl; b++) {
            uint64_t lv[L];
            for (int k = 0; k < L; k++) lv[k] = lists[(size_t)b * L + k];
            ks::topl_insert<L>(top, lv);
        }
    };
    fold(want);
    if (!c.prune) return;
    uint64_t first_full = 0;
    for (int b = 0; b < c.nl && !first_full; b++) first_full = lists[(size_t)b * L + L - 1];
    const uint64_t thr[3] = {0ull, first_full, want[L - 1]};
    for (int b = 0; b < c.nl; b++)
        for (int k = 0; k < L; k++)
            if (lists[(size_t)b * L + k] < thr[b % 3]) lists[(size_t)b * L + k] = 0ull;
    uint64_t again[L];
    fold(again);  // (pruning drops nothing the top L needs)
    for (int k = 0; k < L; k++)
        if (again[k] != want[k]) want[k] = ~0ull;  // a broken case fails the test
}

std::vector<MergeCase> merge_cases(int L) {
    std::vector<MergeCase> cs;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng >> 33); };
    auto add = [&](int nl, bool prune, auto&& f) {
        MergeCase c{nl, nl > 1024 ? 1024 : 256, prune, std::vector<uint32_t>((size_t)nl * 256)};
        for (size_t n = 0; n < c.tot.size(); n++) c.tot[n] = f((int64_t)n);
        cs.push_back(std::move(c));
    };
    const int sizes[] = {1, 2, 63, 64, 65, 196, 256, 257, 600, 1025, 4096};
    for (int nl : sizes) {
        const int64_t n = (int64_t)nl * 256;
        add(nl, false, [](int64_t) { return 7u; });  // one class everywhere
        // a few small classes, the top one rare: ties dominate, the top L spans one to three classes
        add(nl, false, [&](int64_t) { const uint32_t r = rnd() % (uint32_t)(n / 3 + 2); return r == 0 ? 9u : r < 4 ? 8u : 7u - r % 3; });
        add(nl, true, [&](int64_t) { const uint32_t r = rnd() % (uint32_t)(n / 5 + 2); return r == 0 ? 9u : r < 3 ? 8u : 7u - r % 3; });
        // every total distinct, scattered (40507 is coprime to every n here: a bijection mod n)
        add(nl, false, [&](int64_t i) { return (uint32_t)(1 + (i * 40507 + 17) % n); });
        add(nl, true, [&](int64_t i) { return (uint32_t)(1 + (n - 1 - i)); });  // distinct, the top at the lowest nodes
        add(nl, false, [&](int64_t i) { return (uint32_t)(1 + i); });  // distinct, the top at the highest nodes
        add(nl, false, [](int64_t) { return 0u; });  // all lists empty
        // fewer than L feasible nodes in all (every step-th node, step >= n / (L - 1)), two classes
        const int64_t step = (n + L - 2) / (L - 1);
        add(nl, false, [&](int64_t i) { return i % step == 5 ? 3u + (uint32_t)(i & 1) : 0u; });
    }
    // 256 lists at 256 threads: lane l holds block l's list.  Two classes (9 above 5):
    auto two = [&](auto&& top_class) {
        add(256, false, [&](int64_t i) { return top_class((int)(i / 256), (int)(i % 256)) ? 9u : 5u; });
        add(256, true, [&](int64_t i) { return top_class((int)(i / 256), (int)(i % 256)) ? 9u : 5u; });
    };
    two([](int b, int t) { return b == 0 && t < 2; });                 // the class boundary inside lane 0's list, the cut inside its run
    two([](int b, int t) { return b == 5 && t >= 253; });              // three top keys in lane 5, the cut inside lane 0's run of the second class
    two([](int b, int t) { return (b == 3 && t < 2) || (b == 40 && t == 7); });  // boundary inside wave 0
    two([](int b, int t) { return b >= 60 && b < 64 && t == 9; });     // the top class ends exactly at a wave boundary
    two([&](int b, int t) { return b >= 64 - L && b < 64 && t == 0; });  // L top keys end at the wave boundary
    two([&](int b, int t) { return b >= 64 - L + 1 && b <= 64 && t == 0; });  // ... one past it
    two([](int b, int t) { return (b == 63 || b == 64 || b == 128) && t >= 254; });  // runs on both sides of wave boundaries
    // one block holding >= L of the top class while lower-index blocks hold 1-3 each
    two([&](int b, int t) { return (b == 9 && t < L + 4) || (b == 1 && t == 3) || (b == 2 && t < 2) || (b == 4 && t >= 253); });
    two([&](int b, int t) { return (b == 200 && t < L) || (b == 66 && t == 3) || (b == 130 && t < 3); });
    // the second class only in a few lanes: runs of different lengths, nothing below
    add(256, false, [&](int64_t i) { const int b = (int)(i / 256), t = (int)(i % 256);
                                      return b == 70 && t == 1 ? 9u : (b == 10 && t < 3) || (b == 50 && t < 2) || (b == 63 && t < L) ? 5u : 0u; });
    return cs;
}

template <int L>
bool run_merge_cases(uint64_t* d_lists, uint64_t* d_out, int64_t& bad) {
    std::vector<uint64_t> lists;
    for (const MergeCase& c : merge_cases(L)) {
        uint64_t want[L], got[L];
        merge_case_lists<L>(c, lists, want);
        if (hipMemcpy(d_lists, lists.data(), lists.size() * 8, hipMemcpyHostToDevice) != hipSuccess) return false;
        if (ks::launch_list_merge_test(d_lists, c.nl, L, c.threads, d_out, nullptr) != hipSuccess) return false;
        if (hipMemcpy(got, d_out, sizeof got, hipMemcpyDeviceToHost) != hipSuccess) return false;
        for (int k = 0; k < L; k++) bad += got[k] != want[k];
    }
    return true;
}

ks_status selftest_list_merge(int64_t* failures) {
    constexpr int kMaxLists = 4096;
    ks_own::Dev<uint64_t> d_lists, d_out;
    int64_t bad = 0;
    bool ok = ks_own::dev_alloc(d_lists, (size_t)kMaxLists * ks::kTopLOverlap) == hipSuccess;
    ok = ok && ks_own::dev_alloc(d_out, ks::kTopLOverlap) == hipSuccess;
    ok = ok && run_merge_cases<ks::kTopL>(d_lists, d_out, bad);
    if constexpr (ks::kTopLOverlap != ks::kTopL) ok = ok && run_merge_cases<ks::kTopLOverlap>(d_lists, d_out, bad);
    if (!ok) return KS_EDEVICE;
    *failures = bad;
    return KS_OK;
}

}  // namespace

extern "C" {

ks_status ks_selftest(int32_t device, int32_t test, int64_t* failures) {
    if (!failures || (test != KS_SELFTEST_LR_MICRO && test != KS_SELFTEST_MICRO_STATES && test != KS_SELFTEST_LIST_MERGE))
        return KS_EINVAL;
    *failures = -1;
    if (hipSetDevice(device) != hipSuccess) return KS_EDEVICE;
    if (test == KS_SELFTEST_LIST_MERGE) return selftest_list_merge(failures);
    ks_own::Dev<unsigned long long> d;
    unsigned long long h = 0;
    bool ok = ks_own::dev_alloc(d, 1) == hipSuccess;
    ok = ok && hipMemset(d, 0, sizeof h) == hipSuccess;
    ok = ok && (test == KS_SELFTEST_LR_MICRO ? ks::launch_selftest_lr_micro(d, nullptr)
                                             : ks::launch_selftest_micro_states(d, nullptr)) == hipSuccess;
    ok = ok && hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return KS_EDEVICE;
    *failures = (int64_t)h;
    return KS_OK;
}

ks_status ks_selftest_eval(int32_t device, const ks_eval_cfg* cfg, int64_t n, const int64_t* alloc,
                           const int64_t* run, const int64_t* req, const uint32_t* keymask, const uint64_t* masks,
                           uint32_t variants, uint32_t* total1, uint32_t* tmax, uint32_t* live) {
    constexpr uint32_t kAll = (1u << (ks::kEvPruneBit + ks::kEvPruneCols)) - 1u;
    constexpr uint32_t kTotals = (1u << ks::kEvPruneBit) - 1u;
    static_assert(ks::kEvTotalCols == KS_EVAL_TOTAL_COLS && ks::kEvPruneCols == KS_EVAL_PRUNE_COLS, "column counts");
    if (!cfg || !alloc || !run || !req || !keymask || !masks || n < 1 || n > KS_EVAL_MAX_CASES) return KS_EINVAL;
    if (!variants || (variants & ~kAll)) return KS_EINVAL;
    if ((variants & kTotals) && !total1) return KS_EINVAL;
    if ((variants & ~kTotals) && (!tmax || !live)) return KS_EINVAL;
    if ((cfg->filters & ~7u) || cfg->w_lr < 0 || cfg->w_ba < 0 || cfg->const_total < 0) return KS_EINVAL;
    if ((int64_t)cfg->const_total + 10 * ((int64_t)cfg->w_lr + cfg->w_ba) >= (1LL << 30) - 2) return KS_EINVAL;
    ks::EvalCases ec{};
    ec.c.n_nodes = (int32_t)n;
    ec.c.filter_feeds = cfg->filter_feeds != 0;
    ec.c.filters = cfg->filters;
    ec.c.has_scorers = cfg->has_scorers != 0;
    ec.c.w_lr = cfg->w_lr; ec.c.w_ba = cfg->w_ba; ec.c.const_total = cfg->const_total;
    ec.c.tick_seconds = 1;
    ec.n = n;
    ec.variants = variants;
    if (!ev_batch_valid(ec.c, n, alloc, run, req, variants)) return KS_EINVAL;
    // the scan's per-pod records, on the host as ks_submit_pods builds them
    std::vector<ks::ScanRec> srec((size_t)n);
    ks::EvalCases hc = ec;
    hc.alloc = alloc; hc.run = run; hc.req = req; hc.keymask = keymask; hc.masks = masks;
    for (int64_t i = 0; i < n; i++) srec[(size_t)i] = ks::scan_rec_micro(ec.c, ks::evcase_pod(hc, i));

    if (hipSetDevice(device) != hipSuccess) return KS_EDEVICE;
    const size_t sz_alloc = (size_t)n * 4 * 8, sz_req = (size_t)n * 3 * 8, sz_km = (size_t)n * 4;
    const size_t sz_scan = (size_t)n * sizeof(ks::ScanRec);
    const size_t sz_tot = (size_t)n * 4 * ks::kEvTotalCols, sz_pr = (size_t)n * 4 * ks::kEvPruneCols;
    ks_own::Dev<char> buf[9];
    const size_t size[9] = {sz_alloc, sz_alloc, sz_req, sz_km, sz_alloc, sz_scan, sz_tot, sz_pr, sz_pr};
    const void* src[6] = {alloc, run, req, keymask, masks, srec.data()};
    bool ok = true;
    for (int k = 0; k < 9 && ok; k++) ok = ks_own::dev_alloc(buf[k], size[k]) == hipSuccess;
    for (int k = 0; k < 6 && ok; k++) ok = hipMemcpy(buf[k], src[k], size[k], hipMemcpyHostToDevice) == hipSuccess;
    for (int k = 6; k < 9 && ok; k++) ok = hipMemset(buf[k], 0, size[k]) == hipSuccess;
    char* const bp[9] = {buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], buf[6], buf[7], buf[8]};
    ec.alloc = (const int64_t*)bp[0]; ec.run = (const int64_t*)bp[1]; ec.req = (const int64_t*)bp[2];
    ec.keymask = (const uint32_t*)bp[3]; ec.masks = (const uint64_t*)bp[4]; ec.scan = (const ks::ScanRec*)bp[5];
    ec.total1 = (uint32_t*)bp[6]; ec.tmax = (uint32_t*)bp[7]; ec.live = (uint32_t*)bp[8];
    ok = ok && ks::launch_evtest_nodev(ec, nullptr) == hipSuccess;
    ok = ok && ks::launch_evtest_rec12(ec, nullptr) == hipSuccess;
    ok = ok && ks::launch_evtest_ns32(ec, nullptr) == hipSuccess;
    ok = ok && ks::launch_evtest_conv(ec, nullptr) == hipSuccess;
    ok = ok && hipDeviceSynchronize() == hipSuccess;
    // only the requested columns reach the caller
    for (int b = 0; b < ks::kEvPruneBit + ks::kEvPruneCols && ok; b++) {
        if (!((variants >> b) & 1u)) continue;
        const size_t col = (size_t)n * 4;
        if (b < ks::kEvPruneBit) {
            ok = hipMemcpy(total1 + (size_t)b * n, buf[6] + b * col, col, hipMemcpyDeviceToHost) == hipSuccess;
        } else {
            const size_t j = (size_t)(b - ks::kEvPruneBit);
            ok = hipMemcpy(tmax + j * n, buf[7] + j * col, col, hipMemcpyDeviceToHost) == hipSuccess;
            ok = ok && hipMemcpy(live + j * n, buf[8] + j * col, col, hipMemcpyDeviceToHost) == hipSuccess;
        }
    }
    return ok ? KS_OK : KS_EDEVICE;
}

}  // extern "C"
