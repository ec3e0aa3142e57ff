// The owners and the build-then-commit helper of kubernetes-simulator_amd/csrc/ks_own.h over counting
// fakes, for CPU tests only: tests/test_own_host.py calls the two checks through ctypes.  No device
// call is made: the owners are instantiated with a free function that counts, the bundle's members
// are "allocated" by a fake that can be told to fail at its k-th call.  With -DKS_OWN_MAIN the file
// is a stand-alone program that runs both checks (for a sanitizer build).  Not part of the product.
#include <cstdint>
#include <cstdio>

#include "../../kubernetes-simulator_amd/csrc/ks_own.h"

namespace {

// a fake resource: a handle is a pointer to its count of frees
int g_slot[64];
int g_made = 0, g_freed = 0;
struct CountFree {
    void operator()(int* h) const {
        ++*h;
        ++g_freed;
    }
};
using Fake = ks_own::Own<int*, CountFree>;
using FakePinned = ks_own::Pinned<int, CountFree>;

void reset_world() {
    for (int& s : g_slot) s = 0;
    g_made = g_freed = 0;
}
int* make_handle() { return &g_slot[g_made++]; }
// every handle made so far was freed exactly `want` times
int64_t frees_differ(int want) {
    int64_t bad = 0;
    for (int i = 0; i < g_made; i++) bad += g_slot[i] != want;
    return bad;
}

// the fake factory of the bundle's members: its g_fail_at-th call fails (0: none)
int g_calls = 0, g_fail_at = 0;
hipError_t fake_alloc(Fake& o) {
    if (++g_calls == g_fail_at) return hipErrorOutOfMemory;
    o = Fake(make_handle());
    return hipSuccess;
}
struct Five {
    Fake a, b, c, d, e;
    int tag = 0;
};
hipError_t fill_five(Five& f, int tag) {
    KS_TRY(fake_alloc(f.a));
    KS_TRY(fake_alloc(f.b));
    KS_TRY(fake_alloc(f.c));
    KS_TRY(fake_alloc(f.d));
    KS_TRY(fake_alloc(f.e));
    f.tag = tag;
    return hipSuccess;
}

}  // namespace

extern "C" {

// the owners' rules; returns the number of violations
int64_t ks_host_own_check() {
    int64_t bad = 0;
    reset_world();
    {   // the destructor frees once
        Fake a(make_handle());
        bad += (int*)a != &g_slot[0] || g_freed != 0;
    }
    bad += g_freed != 1 || frees_differ(1);
    reset_world();
    {   // a moved-from owner frees nothing: one free for the two objects
        Fake a(make_handle());
        Fake b(std::move(a));
        bad += (int*)a != nullptr || (int*)b != &g_slot[0] || g_freed != 0;
    }
    bad += g_freed != 1 || frees_differ(1);
    reset_world();
    {   // move-assignment over a live owner frees the old one once, at once; the new one at the end
        Fake a(make_handle()), b(make_handle());
        a = std::move(b);
        bad += g_slot[0] != 1 || g_slot[1] != 0 || (int*)a != &g_slot[1] || (int*)b != nullptr;
        Fake& self = a;
        a = std::move(self);  // onto itself: nothing happens
        bad += g_slot[1] != 0 || (int*)a != &g_slot[1];
    }
    bad += g_freed != 2 || frees_differ(1);
    reset_world();
    {   // reset frees once and empties; again it frees nothing
        Fake a(make_handle());
        a.reset();
        bad += g_slot[0] != 1 || (int*)a != nullptr || a;
        a.reset();
        bad += g_slot[0] != 1;
    }
    bad += g_freed != 1;
    reset_world();
    {   // an empty owner frees nothing, however it goes
        Fake a, b;
        a = std::move(b);
        a.reset();
    }
    bad += g_freed != 0;
    reset_world();
    {   // pinned memory: the device address travels with the host pointer and leaves the moved-from owner, one free
        FakePinned a(make_handle());
        a.dev = &g_slot[63];
        FakePinned b;
        b = std::move(a);
        bad += (int*)b != &g_slot[0] || b.dev != &g_slot[63] || (int*)a != nullptr || a.dev != nullptr || g_freed != 0;
        FakePinned c(std::move(b));  // (and by construction)
        bad += (int*)c != &g_slot[0] || c.dev != &g_slot[63] || (int*)b != nullptr || b.dev != nullptr || g_freed != 0;
    }
    bad += g_freed != 1 || frees_differ(1);
    return bad;
}

// build-then-commit over a bundle of five: for each k the k-th allocation fails; returns the violations
int64_t ks_host_build_check() {
    int64_t bad = 0;
    for (int k = 1; k <= 5; k++) {
        reset_world();
        {
            std::optional<Five> slot;
            g_calls = 0;
            g_fail_at = k;
            bad += ks_own::build(slot, [](Five& f) { return fill_five(f, 7); }) != hipErrorOutOfMemory;
            bad += slot.has_value();                         // the slot is still empty
            bad += g_made != k - 1 || g_freed != g_made || frees_differ(1);  // what was made is released
            g_fail_at = 0;                                   // a following build fills the slot
            bad += ks_own::build(slot, [](Five& f) { return fill_five(f, 9); }) != hipSuccess;
            bad += !slot.has_value() || slot->tag != 9 || !slot->a || !slot->e;
            bad += g_made != k - 1 + 5 || g_freed != k - 1;  // (moving the bundle into the slot frees nothing)
        }
        bad += g_freed != g_made || frees_differ(1);         // the slot's destructor frees the five, once each
    }
    reset_world();
    {   // a failed build over a full slot leaves the slot as it was
        std::optional<Five> slot;
        g_calls = g_fail_at = 0;
        bad += ks_own::build(slot, [](Five& f) { return fill_five(f, 1); }) != hipSuccess;
        g_calls = 0;
        g_fail_at = 3;
        bad += ks_own::build(slot, [](Five& f) { return fill_five(f, 2); }) == hipSuccess;
        bad += !slot || slot->tag != 1 || (int*)slot->a != &g_slot[0] || g_slot[0] != 0 || g_freed != 2;
        g_fail_at = 0;
    }
    bad += g_freed != g_made || frees_differ(1);
    return bad;
}

}  // extern "C"

#ifdef KS_OWN_MAIN
int main() {
    const int64_t a = ks_host_own_check(), b = ks_host_build_check();
    std::printf("owners: %lld violations, build-then-commit: %lld violations\n", (long long)a, (long long)b);
    return a != 0 || b != 0;
}
#endif
