// Host build of the headroom count (ks_query.h headroom_count / head_div), for CPU tests only: the
// same source the kernels inline, compiled for the host so its integer math can be checked against
// Python integers without a GPU.  Not part of the product.
#include "../../kubernetes-simulator_amd/csrc/ks_query.h"

static ks::NodeV node_of(const int64_t* alloc, const int64_t* run, int64_t i) {
    ks::NodeV v{};
    v.ac = alloc[i * 4 + 0]; v.am = alloc[i * 4 + 1]; v.ag = alloc[i * 4 + 2]; v.ap = alloc[i * 4 + 3];
    v.rc = run[i * 4 + 0]; v.rm = run[i * 4 + 1]; v.rg = run[i * 4 + 2]; v.nr = run[i * 4 + 3];
    return v;
}

// case i: node alloc[i][4] / run[i][4] in device units, scale[i][3] milli-units per device unit, shape
// req[i][3] in milli-units with keymask[i]: count[i], key[i]
extern "C" void ks_host_headroom_batch(int64_t n, const int64_t* alloc, const int64_t* run, const int64_t* scale,
                                       const int64_t* req, const uint32_t* keymask, int32_t* count, int32_t* key) {
    for (int64_t i = 0; i < n; i++) {
        const ks::NodeV v = node_of(alloc, run, i);
        const ks::QScale sc{{scale[i * 3 + 0], scale[i * 3 + 1], scale[i * 3 + 2]}};
        ks::PodRec p{};
        p.req[0] = req[i * 3 + 0]; p.req[1] = req[i * 3 + 1]; p.req[2] = req[i * 3 + 2];
        p.keymask = keymask[i];
        count[i] = ks::headroom_count(v, sc, p, &key[i]);
    }
}

// The literal loop: admit copies one at a time with fits() (Node.CreatePod's admission test) until
// it fails or `limit` copies are in.  Everything in milli-units (alloc_m / run_m: [n][4]).
extern "C" void ks_host_headroom_loop(int64_t n, const int64_t* alloc_m, const int64_t* run_m, const int64_t* req,
                                      const uint32_t* keymask, int64_t limit, int64_t* count) {
    for (int64_t i = 0; i < n; i++) {
        ks::NodeV v = node_of(alloc_m, run_m, i);
        ks::PodRec p{};
        p.req[0] = req[i * 3 + 0]; p.req[1] = req[i * 3 + 1]; p.req[2] = req[i * 3 + 2];
        p.keymask = keymask[i];
        int64_t c = 0;
        while (c < limit && ks::fits(p, v)) {
            if (p.keymask & 1) v.rc += p.req[0];
            if (p.keymask & 2) v.rm += p.req[1];
            if (p.keymask & 4) v.rg += p.req[2];
            v.nr += 1;
            c++;
        }
        count[i] = c;
    }
}

extern "C" int64_t ks_host_head_div(uint64_t num, uint64_t q) { return ks::head_div(num, q); }
extern "C" void ks_host_head_div_batch(int64_t n, const uint64_t* num, const uint64_t* q, int64_t* out) {
    for (int64_t i = 0; i < n; i++) out[i] = ks::head_div(num[i], q[i]);
}
extern "C" void ks_host_head_thresholds(uint64_t* out4) {
    out4[0] = ks::kHeadFloat; out4[1] = ks::kHeadDouble; out4[2] = ks::kHeadClampQ; out4[3] = (uint64_t)ks::kHeadMax;
}
