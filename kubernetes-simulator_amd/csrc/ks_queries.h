// ks_queries.h — what the two translation units that answer about a run after the fact share
// (internal: ks_queries.cpp defines it and holds the state queries, headroom and the name-keyed
// lookups; ks_previews.cpp holds the five previews).
#pragma once
#include "ks_carve.h"
#include "ks_host.h"

namespace ks_host {

// t is a tick of the run so far
ks_status check_tick(ks_engine* e, const char* what, int64_t t);
// pods bound at ticks <= t (a FIFO prefix of the binds made so far)
int64_t bound_by(const ks_engine* e, int64_t t);
// Every past-tick query opens with this: the device, the staged submits, and the candidate blocks
// of the pods [0, q_hi) over ticks >= t_lo, uploaded to d_blk (*nb of them).
ks_status query_blocks(ks_engine* e, int64_t t_lo, int64_t q_hi, int64_t* nb);
// Reserve what the sizing pass of a layout counted and rewind the cursors onto the scratch.
ks_status reserve_scratch(ks_engine* e, Carve* qs, Carve* qi);
// A call's scratch: `layout` takes its ranges from the cursors qs (over d_qs) and qi (over d_qi) and
// runs twice (ks_carve.h) — to size the two scratches, then, once they are reserved, for the pointers.
#define CARVE_SCRATCH(e, layout)                                                          \
    Carve qs(sizeof(unsigned long long)), qi(sizeof(int32_t));                            \
    layout;                                                                               \
    if (ks_status r_ = reserve_scratch((e), &qs, &qi); r_ != KS_OK) return r_;            \
    layout

ks::QScale milli_scale(const ks_engine* e);
constexpr ks::QScale kDeviceUnits{{1, 1, 1}};
// The node table's rc rm rg nr at tick t, rebuilt from the binds into dst: the pods q < q_hi of the
// nb uploaded blocks that were bound Ok and run at t, times scale; word c of node nd at
// dst[nd * stride + c * pitch] ([n][4] rows: 4, 1; [4][pitch] planes: 1, n_pad).
ks_status rebuild_state(ks_engine* e, int64_t nb, int64_t q_hi, int64_t t, const ks::QScale& scale, int64_t stride,
                        int64_t pitch, unsigned long long* dst);
// the tail of a query over n > 0 nodes: copy the result out once its kernels are queued (rc: theirs)
ks_status copy_result(ks_engine* e, ks_status rc, void* dst, const void* src, size_t bytes);
// the call's shape records (e->h_shapes, requests in milli-units) from k checked shapes, max_shapes at the most
ks_status head_shapes(ks_engine* e, int32_t k, const int64_t* req, const uint8_t* keymask, const uint64_t* tol,
                      const uint64_t* sel, const char* what = "headroom", int32_t max_shapes = KS_HEADROOM_MAX_SHAPES);

}  // namespace ks_host
