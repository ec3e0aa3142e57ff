// ks_queries.cpp — the entry points of include/ks_engine.h that answer about a run after the fact:
// filter / score of a pod, usage, the past-tick state queries, headroom and the name-keyed lookups
// (the five previews: ks_previews.cpp), and the pieces both share (ks_queries.h).  They read the
// engine (ks_host.h) and write nothing a later ks_step reads; their device scratch is the grow-only
// d_qs / d_qi, carved by ks_carve.h.
#include "ks_queries.h"

using namespace ks_host;

static ks_status check_window(ks_engine* e, const char* what, int64_t t_lo, int64_t t_hi) {
    if (t_lo < 0 || t_hi <= t_lo || t_hi - 1 > e->tick || t_hi - t_lo > kMaxDigestTicks)
        return fail(e, KS_EINVAL, "%s window [%lld, %lld) outside [0, %lld] or longer than %lld ticks", what,
                    (long long)t_lo, (long long)t_hi, (long long)e->tick + 1, (long long)kMaxDigestTicks);
    return KS_OK;
}

// Candidate pod blocks of a usage query over ticks >= t_lo: blocks of the pods [0, q_hi) (bind
// ticks are FIFO-monotone, so q_hi bounds the start side) holding a pod whose run end is > t_lo;
// super blocks whose every pod ended by t_lo are skipped whole.
static int64_t usage_blocks(ks_engine* e, int64_t t_lo, int64_t q_hi) {
    e->h_blk.clear();
    const int64_t nblk = (q_hi + kUBlk - 1) / kUBlk;
    for (int64_t s = 0; s * kUSup < nblk; s++) {
        if (e->sup_end[s] <= t_lo) continue;
        const int64_t b1 = std::min(nblk, (s + 1) * kUSup);
        for (int64_t b = s * kUSup; b < b1; b++)
            if (e->blk_end[b] > t_lo) e->h_blk.push_back((int32_t)b);
    }
    return (int64_t)e->h_blk.size();
}

static_assert(kUBlk == 256, "usage index block = the usage kernels' workgroup");

// ---- the pieces the queries and the previews share (ks_queries.h) -------------------------------
namespace ks_host {

ks_status check_tick(ks_engine* e, const char* what, int64_t t) {
    if (t < 0 || t > e->tick)
        return fail(e, KS_EINVAL, "%stick %lld outside [0, %lld]", what, (long long)t, (long long)e->tick);
    return KS_OK;
}

int64_t bound_by(const ks_engine* e, int64_t t) {
    return std::upper_bound(e->h_bind_tick.begin(), e->h_bind_tick.begin() + e->done, t) - e->h_bind_tick.begin();
}

ks_status query_blocks(ks_engine* e, int64_t t_lo, int64_t q_hi, int64_t* nb) {
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, stage_flush(e));
    *nb = usage_blocks(e, t_lo, q_hi);
    if (!*nb) return KS_OK;
    HIPCHK(e, e->d_blk.reserve(*nb, e->st));
    HIPCHK(e, hipMemcpyAsync(e->d_blk.p, e->h_blk.data(), sizeof(int32_t) * *nb, hipMemcpyHostToDevice, e->st));
    return KS_OK;
}

ks_status reserve_scratch(ks_engine* e, Carve* qs, Carve* qi) {
    HIPCHK(e, e->d_qs.reserve(qs->at, e->st));
    HIPCHK(e, e->d_qi.reserve(qi->at, e->st));
    *qs = Carve(sizeof(unsigned long long), e->d_qs.p);
    *qi = Carve(sizeof(int32_t), e->d_qi.p);
    return KS_OK;
}

ks::QScale milli_scale(const ks_engine* e) { return ks::QScale{{e->scale[0], e->scale[1], e->scale[2]}}; }

ks_status rebuild_state(ks_engine* e, int64_t nb, int64_t q_hi, int64_t t, const ks::QScale& scale, int64_t stride,
                        int64_t pitch, unsigned long long* dst) {
    const int64_t words = stride == 1 ? 4 * pitch : 4 * e->n;
    HIPCHK(e, hipMemsetAsync(dst, 0, sizeof(unsigned long long) * words, e->st));
    HIPCHK(e, ks::launch_requested(e->d_blk.p, nb, q_hi, t, (int32_t)e->n, e->b_node.p, e->b_status.p, e->t0.p, e->dur.p,
                                   e->pods.p, scale, stride, pitch, dst, e->st));
    return KS_OK;
}

ks_status copy_result(ks_engine* e, ks_status rc, void* dst, const void* src, size_t bytes) {
    if (rc != KS_OK) return rc;
    if (e->n) HIPCHK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

ks_status head_shapes(ks_engine* e, int32_t k, const int64_t* req, const uint8_t* keymask, const uint64_t* tol,
                      const uint64_t* sel, const char* what, int32_t max_shapes) {
    if (k < 1 || k > max_shapes) return fail(e, KS_EINVAL, "%s: %d shapes outside [1, %d]", what, (int)k, (int)max_shapes);
    e->h_shapes.assign(k, ks::PodRec{});
    for (int32_t j = 0; j < k; j++) {
        if (keymask[j] & ~7u) return fail(e, KS_EINVAL, "%s shape %d: keymask %u has bits above 4", what, (int)j, (unsigned)keymask[j]);
        ks::PodRec& r = e->h_shapes[j];
        for (int c = 0; c < 3; c++) {
            if (!(keymask[j] >> c & 1)) continue;  // unmasked keys are ignored
            const int64_t q = req[j * 3 + c];
            if (q < 0 || q >= ks::kHeadReqMax) return fail(e, KS_EINVAL, "%s shape %d: request %d out of range", what, (int)j, c);
            r.req[c] = q;
        }
        r.tol = tol[j];
        r.sel = sel[j];
        r.keymask = keymask[j];
    }
    return KS_OK;
}

}  // namespace ks_host

extern "C" {

// ---- filter / score of a queued pod, usage ------------------------------------------------------

static ks_status eval_pod(ks_engine* e, int64_t pod) {
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (pod < 0 || pod >= e->P) return fail(e, KS_EINVAL, "pod %lld out of range", (long long)pod);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, stage_flush(e));
    ks_status r = flush_expiries(e);
    if (r != KS_OK) return r;
    if (e->n == 0) return KS_OK;
    HIPCHK(e, ks::launch_eval_pod(e->dc, e->s, e->pods.p + pod, e->cfg.filters, e->d_mask, e->d_score, e->mode, e->st));
    return KS_OK;
}

ks_status ks_filter(ks_engine* e, int64_t pod, uint8_t* mask_out) {
    if (!e || !mask_out) return KS_EINVAL;
    return copy_result(e, eval_pod(e, pod), mask_out, e->d_mask, e->n);
}

ks_status ks_score(ks_engine* e, int64_t pod, int64_t* score_out) {
    if (!e || !score_out) return KS_EINVAL;
    return copy_result(e, eval_pod(e, pod), score_out, e->d_score, sizeof(int64_t) * e->n);
}

ks_status ks_usage_at(ks_engine* e, int64_t t, int64_t* usage_out) {
    if (!e || !usage_out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = check_tick(e, "usage ", t); r != KS_OK) return r;
    if (e->n == 0) return KS_OK;
    const int64_t q_hi = bound_by(e, t);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
    HIPCHK(e, hipMemsetAsync(e->d_usage, 0, sizeof(unsigned long long) * 3 * e->n, e->st));
    if (nb) {
        // (profiling: HIP events around the usage kernel alone — its roofline in bench.py)
        if (e->profiling && e->ev[kEvUsageBegin]) HIPCHK(e, hipEventRecord(e->ev[kEvUsageBegin], e->st));
        HIPCHK(e, ks::launch_usage(e->d_blk.p, nb, q_hi, t, e->cfg.tick_seconds, e->b_node.p, e->b_status.p, e->t0.p,
                                   e->dur.p, e->phase_off.p, e->cum_sec.p, e->use.p, e->d_usage, e->st));
        if (e->profiling && e->ev[kEvUsageEnd]) HIPCHK(e, hipEventRecord(e->ev[kEvUsageEnd], e->st));
    }
    HIPCHK(e, hipMemcpyAsync(usage_out, e->d_usage, sizeof(int64_t) * 3 * e->n, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    if (e->profiling && nb && e->ev[kEvUsageBegin]) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e->ev[kEvUsageBegin], e->ev[kEvUsageEnd]);
        e->kstats.usage_ms += ms;
        e->kstats.usage_n += 1;
        e->kstats.usage_pods += (int64_t)nb * ks::usage_block_pods();
    }
    return KS_OK;
}

ks_status ks_usage(ks_engine* e, int64_t* usage_out) {
    if (!e) return KS_EINVAL;
    return ks_usage_at(e, e->tick, usage_out);
}

ks_status ks_usage_digest(ks_engine* e, int64_t t_lo, int64_t t_hi, uint64_t* out) {
    if (!e || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = check_window(e, "digest", t_lo, t_hi); r != KS_OK) return r;
    const int64_t T = t_hi - t_lo;
    const int64_t q_hi = bound_by(e, t_hi - 1);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t_lo, q_hi, &nb); r != KS_OK) return r;
    HIPCHK(e, e->d_digest.reserve(6 * (T + 1) + 6 * T, e->st));
    unsigned long long* diff = e->d_digest.p;
    unsigned long long* res = diff + 6 * (T + 1);
    HIPCHK(e, hipMemsetAsync(diff, 0, sizeof(unsigned long long) * 6 * (T + 1), e->st));
    HIPCHK(e, ks::launch_usage_digest(e->d_blk.p, nb, q_hi, t_lo, t_hi, e->cfg.tick_seconds, e->b_node.p, e->b_status.p,
                                      e->t0.p, e->dur.p, e->preg.p, e->phase_off.p, e->cum_sec.p, e->use.p, diff, res,
                                      e->st));
    HIPCHK(e, hipMemcpyAsync(out, res, sizeof(uint64_t) * 6 * T, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

// ---- past-tick state queries (ks_query.hip) ----------------------------------------------------
// The node table's rc rm rg nr at any past tick, rebuilt from the binds: the pods q < q_hi that
// were bound Ok and run at t.  They share the usage queries' run-interval index, read only the
// bind arrays and the pod records, and leave the live table and the expiry state alone — so they
// answer after an aborted run too (on the binds made before it).

ks_status ks_requested_at(ks_engine* e, int64_t t, int64_t* out) {
    if (!e || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    if (e->n == 0) return KS_OK;
    const int64_t q_hi = bound_by(e, t);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
    unsigned long long* state;  // [n][4], milli-units
    CARVE_SCRATCH(e, state = qs.take<unsigned long long>(4 * e->n));
    if (ks_status r = rebuild_state(e, nb, q_hi, t, milli_scale(e), 4, 1, state); r != KS_OK) return r;
    return copy_result(e, KS_OK, out, state, sizeof(int64_t) * 4 * e->n);
}

// Filter mask and score of an already-bound pod as scheduleOne saw them: the evaluator of
// ks_filter / ks_score on a copy of the node table whose rc rm rg nr are the state rebuilt from the
// pods q < pod running at the pod's bind tick (every one of them was bound at an earlier tick).
static ks_status eval_pod_at(ks_engine* e, int64_t pod) {
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (pod < 0 || pod >= e->done || e->h_node[pod] < 0)
        return fail(e, KS_EINVAL, "pod %lld is not bound (queued pods: ks_filter / ks_score)", (long long)pod);
    if (e->n == 0) return KS_OK;
    const int64_t t = e->h_bind_tick[pod], np = e->n_pad;
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, pod, &nb); r != KS_OK) return r;
    int64_t* b;  // [4][np], device units
    CARVE_SCRATCH(e, b = qs.take<int64_t>(4 * np));
    if (ks_status r = rebuild_state(e, nb, pod, t, kDeviceUnits, 1, np, (unsigned long long*)b); r != KS_OK) return r;
    ks::NodeSoA s = e->s;
    s.rc = b; s.rm = b + np; s.rg = b + 2 * np; s.nr = b + 3 * np;
    HIPCHK(e, ks::launch_eval_pod(e->dc, s, e->pods.p + pod, e->cfg.filters, e->d_mask, e->d_score, e->mode, e->st));
    return KS_OK;
}

ks_status ks_filter_at(ks_engine* e, int64_t pod, uint8_t* mask_out) {
    if (!e || !mask_out) return KS_EINVAL;
    return copy_result(e, eval_pod_at(e, pod), mask_out, e->d_mask, e->n);
}

ks_status ks_score_at(ks_engine* e, int64_t pod, int64_t* score_out) {
    if (!e || !score_out) return KS_EINVAL;
    return copy_result(e, eval_pod_at(e, pod), score_out, e->d_score, sizeof(int64_t) * e->n);
}

// prefix counts of the Ok / OverCapacity binds, extended over the pods [cum_upto, done)
static void count_binds(ks_engine* e) {
    for (int64_t q = e->cum_upto; q < e->done; q++) {
        e->cum_ok.push_back(e->cum_ok.back() + (e->h_status[q] == KS_POD_OK && e->h_node[q] >= 0));
        e->cum_over.push_back(e->cum_over.back() + (e->h_status[q] == KS_POD_OVER_CAPACITY && e->h_node[q] >= 0));
    }
    e->cum_upto = e->done;
}

static_assert(KS_SERIES_COLS == ks::kSeriesCols, "ks_cluster_series columns");

ks_status ks_cluster_series(ks_engine* e, int64_t t_lo, int64_t t_hi, int64_t* out) {
    if (!e || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = check_window(e, "series", t_lo, t_hi); r != KS_OK) return r;
    const int64_t T = t_hi - t_lo;
    // pods off the queue by t_lo / by the window's last tick; arrivals likewise (both FIFO prefixes)
    const int64_t q_lo = bound_by(e, t_lo), q_hi = bound_by(e, t_hi - 1);
    const int64_t a_lo = std::upper_bound(e->h_arr.begin(), e->h_arr.end(), t_lo) - e->h_arr.begin();
    const int64_t a_hi = std::upper_bound(e->h_arr.begin(), e->h_arr.end(), t_hi - 1) - e->h_arr.begin();
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t_lo, q_hi, &nb); r != KS_OK) return r;
    count_binds(e);
    ks::SeriesInit init{};
    init.v[4] = e->cum_ok[q_lo];
    init.v[5] = e->cum_over[q_lo];
    init.v[6] = a_lo - q_lo;
    const int64_t C = ks::kSeriesCols, n_arr = a_hi - a_lo;
    unsigned long long *diff, *res;
    int64_t* arr;
    CARVE_SCRATCH(e, {
        diff = qs.take<unsigned long long>(C * (T + 1));
        res = qs.take<unsigned long long>(C * T);
        arr = qs.take<int64_t>(n_arr);
    });
    HIPCHK(e, hipMemsetAsync(diff, 0, sizeof(unsigned long long) * C * (T + 1), e->st));
    if (n_arr)
        HIPCHK(e, hipMemcpyAsync(arr, e->h_arr.data() + a_lo, sizeof(int64_t) * n_arr, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, ks::launch_series(e->d_blk.p, nb, q_lo, q_hi, t_lo, t_hi, e->b_status.p, e->t0.p, e->dur.p, e->pods.p,
                                milli_scale(e), arr, n_arr, init, diff, res, e->st));
    HIPCHK(e, hipMemcpyAsync(out, res, sizeof(int64_t) * C * T, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

ks_status ks_node_peaks(ks_engine* e, int64_t t_lo, int64_t t_hi, int64_t* out) {
    if (!e || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = check_window(e, "peaks", t_lo, t_hi); r != KS_OK) return r;
    if (e->n == 0) return KS_OK;
    const int64_t q_hi = bound_by(e, t_hi - 1);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t_lo, q_hi, &nb); r != KS_OK) return r;
    const int64_t n = e->n, cap = nb * kUBlk;
    if (cap > INT32_MAX) return fail(e, KS_EINVAL, "peaks window holds too many candidate pods");
    long long* peaks;
    NodeLists l;
    CARVE_SCRATCH(e, {
        peaks = qs.take<long long>(4 * n);
        l = carve_node_lists(qi, n, cap);
    });
    HIPCHK(e, hipMemsetAsync(l.cnt, 0, sizeof(int32_t) * n, e->st));
    HIPCHK(e, ks::launch_node_peaks(e->d_blk.p, nb, q_hi, t_lo, (int32_t)n, e->b_node.p, e->b_status.p, e->t0.p,
                                    e->dur.p, e->pods.p, milli_scale(e), l.cnt, l.off, l.cur, l.list, (int32_t)cap, peaks,
                                    e->st));
    return copy_result(e, KS_OK, out, peaks, sizeof(int64_t) * 4 * n);
}

// ---- headroom queries (ks_query.hip) -----------------------------------------------------------
// How many more pods of a shape Node.CreatePod (kubesim/node/node.go:44-47) would admit per node at a
// past tick: the rebuilt rc rm rg nr against the cluster's alloc / taints / labels.  Shapes live only
// for the call: nothing is appended, rescaled or written back (their requests stay in milli-units,
// the device multiplies the free amount by e->scale instead of dividing the request).
static_assert(KS_HEADROOM_COLS == ks::kHeadCols && KS_HEADROOM_MAX_SHAPES == ks::kHeadMaxShapes &&
              KS_HEADROOM_NODE_MAX == ks::kHeadMax, "ks_headroom_* constants");
constexpr int64_t kMaxHeadSeries = 1LL << 22;  // k * (t_hi - t_lo) at the most

ks_status ks_headroom_at(ks_engine* e, int64_t t, int32_t k, const int64_t* req, const uint8_t* keymask,
                         const uint64_t* tol, const uint64_t* sel, int64_t* out, int32_t* per_node_out) {
    if (!e || !req || !keymask || !tol || !sel || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = head_shapes(e, k, req, keymask, tol, sel); r != KS_OK) return r;
    if (ks_status r = check_tick(e, "", t); r != KS_OK) return r;
    if (e->n == 0) {
        for (int32_t j = 0; j < k; j++)
            for (int c = 0; c < KS_HEADROOM_COLS; c++) out[j * KS_HEADROOM_COLS + c] = c == 3 ? -1 : 0;
        return KS_OK;
    }
    const int64_t q_hi = bound_by(e, t);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t, q_hi, &nb); r != KS_OK) return r;
    const int64_t n = e->n, np = e->n_pad, nblk = (n + 255) / 256;
    unsigned long long *state, *part;
    ks::PodRec* shapes;
    long long* res;
    int32_t* per_node;
    CARVE_SCRATCH(e, {
        state = qs.take<unsigned long long>(4 * np);  // [4][np]: rc rm rg nr at t, device units
        shapes = qs.take<ks::PodRec>(k, 2);
        part = qs.take<unsigned long long>(nblk * k * 3);  // [nblk][k][3]
        res = qs.take<long long>((int64_t)k * KS_HEADROOM_COLS);
        per_node = qi.take<int32_t>(per_node_out ? (int64_t)k * n : 0);
    });
    if (ks_status r = rebuild_state(e, nb, q_hi, t, kDeviceUnits, 1, np, state); r != KS_OK) return r;
    HIPCHK(e, hipMemcpyAsync(shapes, e->h_shapes.data(), sizeof(ks::PodRec) * k, hipMemcpyHostToDevice, e->st));
    HIPCHK(e, ks::launch_headroom(e->s, (const int64_t*)state, np, (int32_t)n, e->dc.filter_feeds, e->cfg.filters,
                                  milli_scale(e), shapes, k, part, res, per_node_out ? per_node : nullptr, e->st));
    HIPCHK(e, hipMemcpyAsync(out, res, sizeof(int64_t) * k * KS_HEADROOM_COLS, hipMemcpyDeviceToHost, e->st));
    if (per_node_out)
        HIPCHK(e, hipMemcpyAsync(per_node_out, per_node, sizeof(int32_t) * k * n, hipMemcpyDeviceToHost, e->st));
    HIPCHK(e, hipStreamSynchronize(e->st));
    return KS_OK;
}

ks_status ks_headroom_series(ks_engine* e, int64_t t_lo, int64_t t_hi, int32_t k, const int64_t* req,
                             const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel, int64_t* out) {
    if (!e || !req || !keymask || !tol || !sel || !out) return KS_EINVAL;
    if (!e->nodes_loaded) return fail(e, KS_EINVAL, "no nodes loaded");
    if (ks_status r = head_shapes(e, k, req, keymask, tol, sel); r != KS_OK) return r;
    if (ks_status r = check_window(e, "headroom", t_lo, t_hi); r != KS_OK) return r;
    const int64_t T = t_hi - t_lo, C2 = 2 * (int64_t)k;
    if (k * T > kMaxHeadSeries)
        return fail(e, KS_EINVAL, "headroom series: %d shapes x %lld ticks is more than %lld", (int)k, (long long)T,
                    (long long)kMaxHeadSeries);
    if (e->n == 0) {
        std::fill(out, out + C2 * T, (int64_t)0);
        return KS_OK;
    }
    const int64_t q_hi = bound_by(e, t_hi - 1);
    int64_t nb = 0;
    if (ks_status r = query_blocks(e, t_lo, q_hi, &nb); r != KS_OK) return r;
    const int64_t n = e->n, cap = nb * kUBlk;
    if (cap > INT32_MAX) return fail(e, KS_EINVAL, "headroom window holds too many candidate pods");
    unsigned long long *diff, *res;
    ks::PodRec* shapes;
    NodeLists l;
    CARVE_SCRATCH(e, {
        diff = qs.take<unsigned long long>(C2 * (T + 1));  // [2 k][T + 1]
        res = qs.take<unsigned long long>(C2 * T);         // [T][k][2]
        shapes = qs.take<ks::PodRec>(k, 2);
        l = carve_node_lists(qi, n, cap);
    });
    HIPCHK(e, hipMemsetAsync(diff, 0, sizeof(unsigned long long) * C2 * (T + 1), e->st));
    HIPCHK(e, hipMemsetAsync(l.cnt, 0, sizeof(int32_t) * n, e->st));
    HIPCHK(e, hipMemcpyAsync(shapes, e->h_shapes.data(), sizeof(ks::PodRec) * k, hipMemcpyHostToDevice, e->st));
    // the listed pods' requests stay in device units (QScale 1): the count takes e->scale itself
    HIPCHK(e, ks::launch_headroom_series(e->d_blk.p, nb, q_hi, t_lo, t_hi, e->s, (int32_t)n, e->dc.filter_feeds,
                                         e->cfg.filters, milli_scale(e), shapes, k, e->b_node.p, e->b_status.p,
                                         e->t0.p, e->dur.p, e->pods.p, l.cnt, l.off, l.cur, l.list, (int32_t)cap, diff,
                                         res, e->st));
    return copy_result(e, KS_OK, out, res, sizeof(int64_t) * C2 * T);
}

// ---- name-keyed lookups --------------------------------------------------------------------------

uint64_t ks_node_mix(int64_t node) {
    uint64_t z = (uint64_t)(node + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Name-keyed index: every pod bound per node in FIFO order, extended over the binds
// [idx_upto, done) on each query; a key's stored pod is the last one bound there (Store
// replaces, kubesim/node/node.go:58).
static void index_binds(ks_engine* e) {
    if ((int64_t)e->node_pods.size() < e->n) e->node_pods.resize(e->n);
    for (int64_t q = e->idx_upto; q < e->done; q++) {
        const int32_t nd = e->h_node[q];
        if (nd < 0) continue;  // the pod an aborted run stopped at is never stored
        e->node_pods[nd].push_back(q);
    }
    e->idx_upto = e->done;
}

ks_status ks_pod_lookup(ks_engine* e, int32_t node, int64_t key_id, int64_t* pod_out) {
    if (!e || !pod_out) return KS_EINVAL;
    *pod_out = -1;
    if (node < 0 || node >= e->n) return fail(e, KS_EINVAL, "node %d out of range", node);
    index_binds(e);
    const std::vector<int64_t>& v = e->node_pods[node];
    for (auto it = v.rbegin(); it != v.rend(); ++it)  // the last Store under the key wins
        if (e->h_key[*it] == key_id) {
            *pod_out = *it;
            return KS_OK;
        }
    return fail(e, KS_ENOTFOUND, "pod with key %lld not found on node %d", (long long)key_id, node);
}

ks_status ks_node_pods(ks_engine* e, int32_t node, int64_t* pods_out, int64_t cap, int64_t* n_out) {
    if (!e || !n_out || cap < 0 || (cap > 0 && !pods_out)) return KS_EINVAL;
    *n_out = 0;
    if (node < 0 || node >= e->n) return fail(e, KS_EINVAL, "node %d out of range", node);
    index_binds(e);
    const std::vector<int64_t>& v = e->node_pods[node];
    // one pod per key: the last one bound here (a pod is listed iff no later pod on this node
    // has its key)
    std::unordered_map<int64_t, int64_t> last;
    last.reserve(v.size());
    for (int64_t q : v) last[e->h_key[q]] = q;
    int64_t k = 0;
    for (int64_t q : v)
        if (last[e->h_key[q]] == q) {
            if (k < cap) pods_out[k] = q;
            k++;
        }
    *n_out = k;
    return KS_OK;
}

ks_status ks_pod_status(ks_engine* e, int64_t pod_lo, int64_t n, ks_pod_info* out) {
    if (!e || (n > 0 && !out) || pod_lo < 0 || n < 0 || pod_lo + n > e->P) return KS_EINVAL;
    if (n == 0) return KS_OK;
    const int64_t hi = std::min(pod_lo + n, e->done), nb = std::max<int64_t>(hi - pod_lo, 0);
    std::vector<int32_t> node(nb), status(nb);
    if (nb) {
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, stage_flush(e));
        HIPCHK(e, hipMemcpyAsync(node.data(), e->b_node.p + pod_lo, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipMemcpyAsync(status.data(), e->b_status.p + pod_lo, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, e->st));
        HIPCHK(e, hipStreamSynchronize(e->st));
    }
    for (int64_t i = 0; i < n; i++) {
        const int64_t q = pod_lo + i;
        ks_pod_info& o = out[i];
        o.total_seconds = e->h_total_sec[q];
        const bool bound = i < nb && node[i] >= 0;
        o.node = bound ? node[i] : -1;
        o.start_tick = bound ? e->h_bind_tick[q] : -1;
        if (!bound) o.phase = KS_PHASE_PENDING;
        else if (status[i] != KS_POD_OK) o.phase = KS_PHASE_FAILED;  // CapacityExceeded
        else {
            // IsRunning (kubesim/pod/pod.go:67-69): passed = (t - t0) * tick < Σ phase seconds
            const int64_t dt = e->tick - e->h_bind_tick[q];
            o.phase = (dt >= 0 && dt < e->h_dur[q]) ? KS_PHASE_RUNNING : KS_PHASE_SUCCEEDED;
        }
    }
    return KS_OK;
}

}  // extern "C"
