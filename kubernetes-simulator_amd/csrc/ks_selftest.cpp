// ks_selftest.cpp — the device self-tests of include/ks_engine.h (ks_selftest, ks_selftest_eval):
// the evaluators of ks_device.h run on the device over the caller's cases.  They need no engine.
#include <algorithm>
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

}  // namespace

extern "C" {

ks_status ks_selftest(int32_t device, int32_t test, int64_t* failures) {
    if (!failures || (test != KS_SELFTEST_LR_MICRO && test != KS_SELFTEST_MICRO_STATES)) return KS_EINVAL;
    *failures = -1;
    if (hipSetDevice(device) != hipSuccess) return KS_EDEVICE;
    unsigned long long* d = nullptr;
    unsigned long long h = 0;
    bool ok = hipMalloc(&d, sizeof h) == hipSuccess;
    ok = ok && hipMemset(d, 0, sizeof h) == hipSuccess;
    ok = ok && (test == KS_SELFTEST_LR_MICRO ? ks::launch_selftest_lr_micro(d, nullptr)
                                             : ks::launch_selftest_micro_states(d, nullptr)) == hipSuccess;
    ok = ok && hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
    if (d) (void)hipFree(d);
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
    void* buf[9] = {};
    const size_t size[9] = {sz_alloc, sz_alloc, sz_req, sz_km, sz_alloc, sz_scan, sz_tot, sz_pr, sz_pr};
    const void* src[6] = {alloc, run, req, keymask, masks, srec.data()};
    bool ok = true;
    for (int k = 0; k < 9 && ok; k++) ok = hipMalloc(&buf[k], size[k]) == hipSuccess;
    for (int k = 0; k < 6 && ok; k++) ok = hipMemcpy(buf[k], src[k], size[k], hipMemcpyHostToDevice) == hipSuccess;
    for (int k = 6; k < 9 && ok; k++) ok = hipMemset(buf[k], 0, size[k]) == hipSuccess;
    ec.alloc = (const int64_t*)buf[0]; ec.run = (const int64_t*)buf[1]; ec.req = (const int64_t*)buf[2];
    ec.keymask = (const uint32_t*)buf[3]; ec.masks = (const uint64_t*)buf[4]; ec.scan = (const ks::ScanRec*)buf[5];
    ec.total1 = (uint32_t*)buf[6]; ec.tmax = (uint32_t*)buf[7]; ec.live = (uint32_t*)buf[8];
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
            ok = hipMemcpy(total1 + (size_t)b * n, (char*)buf[6] + b * col, col, hipMemcpyDeviceToHost) == hipSuccess;
        } else {
            const size_t j = (size_t)(b - ks::kEvPruneBit);
            ok = hipMemcpy(tmax + j * n, (char*)buf[7] + j * col, col, hipMemcpyDeviceToHost) == hipSuccess;
            ok = ok && hipMemcpy(live + j * n, (char*)buf[8] + j * col, col, hipMemcpyDeviceToHost) == hipSuccess;
        }
    }
    for (int k = 0; k < 9; k++)
        if (buf[k]) (void)hipFree(buf[k]);
    return ok ? KS_OK : KS_EDEVICE;
}

}  // extern "C"
