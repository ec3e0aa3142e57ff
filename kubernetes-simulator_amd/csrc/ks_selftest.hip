// ks_selftest.hip — the device half of the self-tests (gfx950; the host half is ks_selftest.cpp;
// DESIGN.md §2 "Integer arithmetic").
//
// No chain launches these: ks_selftest runs the micro evaluator's two exhaustive checks (tests 0
// and 1), ks_selftest_eval the NodeV columns of the caller's cases.  The kernels of the other state
// types live with the resolvers that own them (ks_cand.hip, ks_chunk.hip, ks_resolve.hip), so the
// checked code is the code the resolvers run.
#include <algorithm>

#include "ks_device.h"

namespace ks {

// Self-test of the micro evaluator's correction-free LeastRequested floor: every (x, A) pair with
// 0 <= x <= A < 2^16 against the exact integer floor (one thread per A).
__global__ __launch_bounds__(256) void selftest_lr_micro_kernel(unsigned long long* bad) {
    const int32_t A = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x) + 1;
    if (A >= kMicroCap) return;
    const float r = 10.f * rcp_est((float)A);
    unsigned long long nbad = 0;
    for (int32_t x = 0; x <= A; ++x) {
        const int64_t q = lr10_micro(x, r), y = 10ll * x;
        nbad += (q * A <= y && y < (q + 1) * A) ? 0ull : 1ull;
    }
    if (nbad) atomicAdd(bad, nbad);
}

hipError_t launch_selftest_lr_micro(unsigned long long* bad, hipStream_t st) {
    hipLaunchKernelGGL(selftest_lr_micro_kernel, dim3((unsigned)((kMicroCap + 255) / 256)), dim3(256), 0, st, bad);
    return hipGetLastError();
}

// Self-test of the whole micro evaluator and its scan form: every usage (uc, um) in [0, Ac + 2] x
// [0, Am + 2] of a list of capacity pairs (Ac Am < 2^24: both domain edges, primes, multiples of
// ten, the C3 shape, the degenerate ones), filters off so that u > A is included.  The exact value
// uses 64-bit integers and multiplications only: the floor q of 10 y / A is the q with
// q A <= 10 y < (q + 1) A — no float, no reciprocal, no division.
constexpr int kStPairs = 13, kStCfgs = 3;
constexpr int32_t kStPair[kStPairs][2] = {{65535, 256}, {256, 65535}, {4095, 4097}, {4093, 4099}, {257, 65279},
                                          {4000, 4194}, {1280, 2048}, {1000, 1000}, {65535, 1},   {1, 65535},
                                          {10, 10},     {2, 3},       {1, 1}};

// floor(10 y / a) for 0 <= 10 y <= 10 a, a > 0, by multiplication checks
__device__ __forceinline__ int64_t st_floor10(int64_t y, int64_t a) {
    int64_t q = 0;
    while ((q + 1) * a <= 10 * y) ++q;
    return q;
}
__device__ __forceinline__ int64_t st_lr(int64_t A, int64_t u) { return u > A ? 0 : st_floor10(A - u, A); }
__device__ __forceinline__ int64_t st_ba(int64_t Ac, int64_t Am, int64_t uc, int64_t um) {
    if (uc >= Ac || um >= Am) return 0;
    const int64_t D = Ac * Am, a = uc * Am, b = um * Ac;
    return st_floor10(D - (a > b ? a - b : b - a), D);
}

__global__ __launch_bounds__(256) void selftest_micro_states_kernel(int32_t ac, int32_t am, unsigned long long* bad) {
    constexpr int32_t kStCfg[kStCfgs][3] = {{1, 0, 0}, {0, 1, 0}, {7, 13, 5}};  // w_lr, w_ba, const
    const int64_t Ac = ac, Am = am;
    const int64_t wm = Am + 3, states = (Ac + 3) * wm;
    unsigned long long nbad = 0;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < states; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t uc = (int64_t)((uint32_t)s / (uint32_t)wm), um = s - uc * wm;  // states < 2^25
        const int64_t lr = (st_lr(Ac, uc) + st_lr(Am, um)) >> 1, ba = st_ba(Ac, Am, uc, um);
        for (int split = 0; split < 2; ++split) {
            NodeV v{};
            v.ac = Ac; v.am = Am; v.ag = 0; v.ap = 110;
            // usage as running = min(u, A) + request = the rest, or as the request alone
            v.rc = split ? 0 : (uc < Ac ? uc : Ac);
            v.rm = split ? 0 : (um < Am ? um : Am);
            PodRec p{};
            p.req[0] = uc - v.rc; p.req[1] = um - v.rm;
            p.keymask = 3;
            for (int k = 0; k < kStCfgs; ++k) {
                Cfg c{};
                c.has_scorers = 1;
                c.w_lr = kStCfg[k][0]; c.w_ba = kStCfg[k][1]; c.const_total = kStCfg[k][2];
                const uint32_t want = (uint32_t)(c.const_total + c.w_lr * lr + c.w_ba * ba) + 1u;
                nbad += eval_total1_micro(c, p, v) != want;
                nbad += eval_scan_micro(c, scan_rec_micro(c, p), v, scan_npen(c, v)) != want;
            }
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}

hipError_t launch_selftest_micro_states(unsigned long long* bad, hipStream_t st) {
    for (int k = 0; k < kStPairs; ++k) {
        static_assert(kStPair[2][0] * (int64_t)kStPair[2][1] == kMicroProd - 1, "the product edge");
        const int64_t states = ((int64_t)kStPair[k][0] + 3) * ((int64_t)kStPair[k][1] + 3);
        const unsigned blocks = (unsigned)std::min<int64_t>((states + 255) / 256, 8192);
        hipLaunchKernelGGL(selftest_micro_states_kernel, dim3(blocks), dim3(256), 0, st, kStPair[k][0], kStPair[k][1], bad);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ks_selftest_eval, the NodeV columns: each evaluator and the scan form on the wide node state, and
// the prune bound prepared from it (prune_prep, prune_prep_t of the narrower modes)
__global__ __launch_bounds__(256) void evtest_nodev_kernel(EvalCases e) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= e.n) return;
    const NodeV v = evcase_node(e, i);
    const PodRec p = evcase_pod(e, i);
    if (evcase_wants(e, kEvalWide)) evcase_total(e, kEvalWide, i, eval_t<kEvalWide>(e.c, p, v));
    if (evcase_wants(e, kEvalNarrow)) evcase_total(e, kEvalNarrow, i, eval_t<kEvalNarrow>(e.c, p, v));
    if (evcase_wants(e, kEvalTiny)) evcase_total(e, kEvalTiny, i, eval_t<kEvalTiny>(e.c, p, v));
    if (evcase_wants(e, kEvalMicro)) evcase_total(e, kEvalMicro, i, eval_t<kEvalMicro>(e.c, p, v));
    if (evcase_wants(e, kEvScanCol))  // the record from the host, npen per node as ks_scan.h
        evcase_total(e, kEvScanCol, i, eval_scan_micro(e.c, e.scan[i], v, scan_npen(e.c, v)));
    if (evcase_wants(e, kEvPruneBit + kEvalWide)) evcase_prune(e, kEvalWide, i, p, prune_prep(e.c, v));
    if (evcase_wants(e, kEvPruneBit + kEvalNarrow)) evcase_prune(e, kEvalNarrow, i, p, prune_prep_t<kEvalNarrow>(e.c, v));
    if (evcase_wants(e, kEvPruneBit + kEvalTiny)) evcase_prune(e, kEvalTiny, i, p, prune_prep_t<kEvalTiny>(e.c, v));
    if (evcase_wants(e, kEvPruneBit + kEvalMicro)) evcase_prune(e, kEvalMicro, i, p, prune_prep_t<kEvalMicro>(e.c, v));
}

hipError_t launch_evtest_nodev(const EvalCases& e, hipStream_t st) {
    hipLaunchKernelGGL(evtest_nodev_kernel, dim3((unsigned)((e.n + 255) / 256)), dim3(256), 0, st, e);
    return hipGetLastError();
}
}  // namespace ks
