// Host access to the early read-back's rule in kubernetes-simulator_amd/csrc/ks_plan.h (early_round and
// its constants), for CPU tests only: tests/test_early_round_host.py calls it through ctypes and checks
// it over every chain.  No device code runs.  With -DKS_EARLY_MAIN the file is a stand-alone program
// that walks the same grid (for a sanitizer build of the host side).  Not part of the product.
#include <cstdio>

#include "../../kubernetes-simulator_amd/csrc/ks_plan.h"

using namespace ks_host;

extern "C" {

int64_t ks_host_early_round(int64_t rounds, int chain) { return early_round(rounds, (Chain)chain); }
// which: 0 kEarlyMinRounds, 1 kEarlyK, 2 kChainTwoLaunch, 3 the number of chains
int64_t ks_host_early_const(int which) {
    switch (which) {
        case 0: return kEarlyMinRounds;
        case 1: return kEarlyK;
        case 2: return kChainTwoLaunch;
        case 3: return kChainPipe + 1;
        default: return -1;
    }
}

}  // extern "C"

#ifdef KS_EARLY_MAIN
int main() {
    int64_t bad = 0;
    for (int chain = 0; chain <= kChainPipe; chain++)
        for (int64_t rounds : {0, 1, kEarlyMinRounds - 1, kEarlyMinRounds, kEarlyMinRounds + 1, 171, 100000}) {
            const int64_t r = early_round(rounds, (Chain)chain);
            if (chain == kChainTwoLaunch && rounds >= kEarlyMinRounds) bad += r != rounds - 1 - kEarlyK || r < 0 || r >= rounds - 1;
            else bad += r != -1;
        }
    std::printf("early_round: %lld violations\n", (long long)bad);
    return bad != 0;
}
#endif
