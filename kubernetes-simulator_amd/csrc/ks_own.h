// ks_own.h — move-only owners of the host code's GPU resources and the build-then-commit helper for
// the bundles of them that are made on first use (ks_host.h).  An owner frees exactly once, in its
// destructor, and reads as the handle it holds.  The free function is a type parameter only so that
// a host test can count frees (tests/native/own_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <optional>
#include <utility>

namespace ks_own {

template <typename H, typename Free>
class Own {
    H h{};

  public:
    Own() = default;
    explicit Own(H x) : h(x) {}
    Own(Own&& o) noexcept : h(std::exchange(o.h, H{})) {}
    Own& operator=(Own&& o) noexcept { if (this != &o) reset(std::exchange(o.h, H{})); return *this; }
    ~Own() { reset(); }
    void reset(H x = H{}) { if (h) Free{}(h); h = x; }
    operator H() const { return h; }
    H operator->() const { return h; }
};

struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct StreamFree { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventFree { void operator()(hipEvent_t v) const { (void)hipEventDestroy(v); } };
struct CommFree { void operator()(ncclComm_t c) const { (void)ncclCommDestroy(c); } };

template <typename T, typename Free = DevFree>
using Dev = Own<T*, Free>;
template <typename T, typename Free = PinFree>
struct Pinned : Own<T*, Free> {  // pinned host memory; dev: its device address when it is mapped
    T* dev = nullptr;
    explicit Pinned(T* x = nullptr) : Own<T*, Free>(x) {}
    Pinned(Pinned&& o) noexcept : Own<T*, Free>(std::move(o)), dev(std::exchange(o.dev, nullptr)) {}
    Pinned& operator=(Pinned&& o) noexcept {
        Own<T*, Free>::operator=(std::move(o));
        dev = std::exchange(o.dev, nullptr);  // (a moved-from owner is empty throughout)
        return *this;
    }
};
using Stream = Own<hipStream_t, StreamFree>;
using Event = Own<hipEvent_t, EventFree>;
using Comm = Own<ncclComm_t, CommFree>;

// return a failed call's error from the enclosing function
#define KS_TRY(expr) do { if (hipError_t r_ = (expr); r_ != hipSuccess) return r_; } while (0)

// The factories: the owner takes the new resource (and frees its old one) only on success.
template <typename T>
hipError_t dev_alloc(Dev<T>& o, size_t count) {
    T* q = nullptr;
    KS_TRY(hipMalloc(&q, sizeof(T) * count));
    o.reset(q);
    return hipSuccess;
}
template <typename T>
hipError_t pinned_alloc(Pinned<T>& o, size_t count, unsigned flags = hipHostMallocDefault) {
    T* q = nullptr;
    KS_TRY(hipHostMalloc(&q, sizeof(T) * count, flags));
    Pinned<T> t(q);
    if (flags & hipHostMallocMapped) KS_TRY(hipHostGetDevicePointer((void**)&t.dev, q, 0));
    o = std::move(t);
    return hipSuccess;
}
inline hipError_t stream_create(Stream& o) {
    hipStream_t s = nullptr;
    KS_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    o.reset(s);
    return hipSuccess;
}
inline hipError_t event_create(Event& o, unsigned flags = hipEventDefault) {
    hipEvent_t v = nullptr;
    KS_TRY(hipEventCreateWithFlags(&v, flags));
    o.reset(v);
    return hipSuccess;
}
inline ncclResult_t comm_init(Comm& o, int world, ncclUniqueId uid, int rank) {
    ncclComm_t c = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c, world, uid, rank);
    if (r == ncclSuccess) o.reset(c);
    return r;
}

// Build-then-commit: a bundle B of owners is made locally and filled by fill(b); it moves into its slot only
// when the fill returned its status type's zero (hipSuccess, KS_OK), else the local's destructors release what
// was made and the slot stays as it was.  A slot is whole or empty: "is the bundle there" is the slot's own test.
template <typename B, typename Fill>
auto build(std::optional<B>& slot, Fill&& fill) {
    B b;
    const auto r = fill(b);
    if (r == decltype(r){}) slot.emplace(std::move(b));
    return r;
}

}  // namespace ks_own
