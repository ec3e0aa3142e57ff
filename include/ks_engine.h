/*
 * ks_engine.h — C-ABI of the MI355X-native kubesim scheduling engine.
 *
 * This is the boundary a kubesim host binds (cgo / ctypes / JNI).
 * Plain C types only: caller-owned host buffers are copied in, outputs go to
 * caller-allocated buffers with explicit lengths, device state is owned by the opaque
 * handle.  A handle is single-threaded (not re-entrant), like the reference's
 * single-goroutine Run loop (kubesim/kubesim.go:101-122).
 *
 * What each entry point replaces in the reference (wangchen615/kubernetes-simulator):
 *   ks_create / ks_load_nodes ... NewKubeSim node construction (kubesim/kubesim.go:32-61,
 *                                 kubesim/config/config.go:44-90, kubesim/node/node.go:22-27)
 *   ks_submit_pods .............. submit + podQueue.append (kubesim/kubesim.go:126-139,
 *                                 kubesim/podqueue.go:18-23); api.Submitter output
 *                                 (api/submitter.go:15) with its arrival tick
 *   ks_step ..................... Run's tick loop + scheduleOne (kubesim/kubesim.go:90-166):
 *                                 Filter (:168-188), Score + argmax (:190-225),
 *                                 Node.CreatePod (kubesim/node/node.go:36-60)
 *   ks_filter ................... api.Filter.Filter for every node (api/scheduler.go:19)
 *   ks_score .................... api.Scorer.Score aggregated over the registered scorers
 *                                 (api/scheduler.go:36, kubesim/kubesim.go:193-206)
 *   ks_usage / ks_usage_at ...... Σ Pod.ResourceUsage(clock) per node (kubesim/pod/pod.go:47-63)
 *   ks_usage_digest ............. the same for every tick of a window, as a fingerprint
 *   ks_requested_at / ks_node_peaks  Node.totalResourceRequest / runningPodsNum (kubesim/node/node.go:97-118)
 *   ks_filter_at / ks_score_at .. the filtered nodes and nodeScore map scheduleOne logs per pod
 *                                 (kubesim/kubesim.go:170,184,194,205), for a pod already bound
 *   ks_cluster_series ........... running / requested / bound / failed / queued curves per tick
 *   ks_headroom_at / _series .... Node.CreatePod's admission test (kubesim/node/node.go:44-47) applied
 *                                 repeatedly: how many more pods of a shape each node would take
 *   ks_place_at ................. scheduleOne (kubesim/kubesim.go:143-225) for k preview pods on a
 *                                 private copy of a past tick's state: where they would be bound
 *   ks_drain_at ................. the same for the pods running on a node set that leaves k.nodes
 *                                 (kubesim/kubesim.go:168-206 range over it): where they would go
 *   ks_removable_at ............. ks_drain_at's answer for each of m candidate nodes on its own:
 *                                 which of them could be taken out
 *   ks_consolidate_at ........... the same candidates handled one after another, as a scale-down pass
 *                                 does: a removal's placements stay, a failed attempt is rolled back
 *   ks_gang_at .................. ks_place_at's pods in groups (gangs) admitted all-or-nothing, or from
 *                                 min_ok members up, in queue order: a blocked gang is rolled back
 *   ks_scale_up_at .............. ks_place_at's answer on the cluster plus up to max_nodes empty nodes
 *                                 of a node-group template, for each of G templates on its own
 *   ks_pod_status ............... Pod.BuildStatus phase / times (kubesim/pod/pod.go:78-167)
 *   ks_pod_lookup / ks_node_pods  Node.GetPod / GetPodStatus / GetPodList (kubesim/node/node.go:62-93)
 *   ks_group_* .................. one KubeSim.Run per what-if scenario, stepped together
 *   ks_last_error ............... the error text Run would return
 *
 * Status codes map 1:1 onto the reference's error kinds (strongerrors):
 *   KS_EINVAL    InvalidArgument (bad names, bad simSpec, bad quantities, bad config)
 *   KS_ENOTFOUND NotFound — no node selected; the run stops exactly as kubesim.go:217-220
 *   KS_EDEVICE   HIP / RCCL failure (no reference counterpart)
 * After KS_ENOTFOUND or a bind-time KS_EINVAL the run is aborted: later ks_step calls return
 * the same code, as Run would have returned.  A KS_EDEVICE from ks_step / ks_group_step is
 * sticky too (the engine's tick and binds stay at the last completed step).
 *
 * Units: cpu, memory and nvidia.com/gpu quantities are int64 milli-units (exact for every
 * resource.Quantity that is a whole number of milli-units); the pods capacity is
 * Capacity.Pods().Value() (a count; absent ⇒ 0).  An absent cpu / memory / gpu capacity key
 * is -1.  All inputs must be non-negative and below 2^59.
 */
#ifndef KS_ENGINE_H
#define KS_ENGINE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_ABI_VERSION 2  /* 2: ks_submit_pods takes key_id */

typedef enum {
    KS_OK = 0,
    KS_EINVAL = 1,
    KS_ENOTFOUND = 2,
    KS_EDEVICE = 3,
    KS_ENOMEM = 4,
    KS_ERANGE = 5,  /* valid input outside the engine's exact domain (ks_ingest.h) */
} ks_status;

/* filter_mode: the reference discards the Filter result (kubesim/kubesim.go:182) —
 * REFERENCE_LITERAL reproduces that; FEEDS_SCORE lets the filters gate the candidates. */
enum { KS_FILTER_REFERENCE_LITERAL = 0, KS_FILTER_FEEDS_SCORE = 1 };
/* filters (bitmask) */
enum { KS_FILTER_FIT = 1, KS_FILTER_TAINT = 2, KS_FILTER_SELECTOR = 4 };
/* scorers: CONST returns `value` for every node (examples/main.go:147-155 with value 1);
 * LEAST_REQUESTED / BALANCED are the integer forms of SURVEY.md §8(a14). */
enum { KS_SCORER_CONST = 0, KS_SCORER_LEAST_REQUESTED = 1, KS_SCORER_BALANCED = 2 };
/* bind status (kubesim/pod/pod.go:20-27) */
enum { KS_POD_OK = 0, KS_POD_OVER_CAPACITY = 1 };
/* per-pod flags: the pod will fail at bind with InvalidArgument
 * (empty namespace/name: kubesim/node/node.go:133-143; bad simSpec: kubesim/pod/pod.go:31-39) */
enum { KS_PODFLAG_BAD_KEY = 1, KS_PODFLAG_BAD_SPEC = 2 };

typedef struct {
    int32_t kind;   /* KS_SCORER_* */
    int32_t weight; /* >= 0 */
    int32_t value;  /* CONST only, >= 0 */
} ks_scorer;
/* ks_create rejects (KS_EINVAL) a scorer set whose maximum total
 * sum(weight*value) + 10*sum(weight of LR/BA) is >= 2^30 - 2. */

typedef struct {
    int32_t abi_version;  /* KS_ABI_VERSION */
    int32_t tick_seconds; /* config `tick` (kubesim/kubesim.go:239), >= 1 */
    int32_t filter_mode;  /* KS_FILTER_REFERENCE_LITERAL / KS_FILTER_FEEDS_SCORE */
    uint32_t filters;     /* KS_FILTER_* bits */
    int32_t n_scorers;    /* 0..8; registration order */
    ks_scorer scorers[8];
    int32_t device;       /* HIP device ordinal */
    int32_t batch_pods;   /* pods resolved per scan (0 = default) */
    uint32_t engine_flags; /* KS_ENGINE_* */
    int32_t reserved[7];
} ks_config;

/* engine_flags: the engine picks the narrowest exact evaluator the scaled capacities allow
 * (micro 24-bit / tiny int32 / narrow 32x32->64 / wide 64/128-bit).  FORCE_WIDE keeps the wide
 * one, NO_TINY skips tiny and micro, NO_MICRO skips micro; all are exact, the flags exist to test
 * them against each other. */
enum { KS_ENGINE_FORCE_WIDE = 1, KS_ENGINE_NO_TINY = 2, KS_ENGINE_NO_MICRO = 4,
       /* resolvers for batches of clusters above the small class (both give the same binds; the
        * flags exist to test them against each other): ONE_POD = the role-split one-pod-per-
        * barrier resolver; CHUNK = chunked Jacobi sweeps in one workgroup's LDS (ks_step only,
        * evaluator modes >= narrow, totals < 2^16).  Bits 16, 32 and 128 (the retired pair, sweep
        * and sequential resolvers) are rejected.
        * NO_OVERLAP: the chunk resolver's batches run the plain chain (each batch's scan before its
        * resolve) instead of fusing the next batch's speculative scan into the resolve launch — the
        * same binds; for A/B timing and to test the two chains against each other. */
       KS_ENGINE_ONE_POD_RESOLVER = 8, KS_ENGINE_CHUNK_RESOLVER = 64, KS_ENGINE_NO_OVERLAP = 256,
       /* PRUNED_LISTS: the scan writes a block's top-L list only when it can reach the pod's global
        * top-L (a running per-pod threshold) and the merge reads only those — the default for chunk-
        * resolver clusters of >= 1,024 scan blocks (262,144 nodes); the flag forces it at every size
        * (same binds; to test the two list forms against each other). */
       KS_ENGINE_PRUNED_LISTS = 512,
       /* SMALL_E (test only): the window prep's E overflow test trips at 128 changed nodes instead of
        * 2,048 (array sizes stay), so small shapes reach the rescan path — on single-shard overlapped
        * engines an empty round whose fused scan lists the same pods again, elsewhere the conditional
        * scan.  Same binds; batching differs. */
       KS_ENGINE_SMALL_E = 2048 };

typedef struct {
    int64_t pod;    /* FIFO index (submission order) */
    int32_t node;   /* node index (ks_load_nodes order) */
    int32_t status; /* KS_POD_* */
    int64_t tick;   /* bind tick (clock = start + tick * tick_seconds) */
} ks_bind;

typedef struct ks_engine ks_engine;

ks_status ks_create(const ks_config* cfg, ks_engine** out);
void ks_destroy(ks_engine* eng);

/* Scenario groups (BASELINE.json configs[3]: independent what-if clusters × pod traces).  A
 * group owns a stream and up to max_scenarios engines created with ks_group_add (same device;
 * ks_load_nodes / ks_submit_pods / ks_usage / ks_filter / ks_score / ks_step work on them as on
 * any engine).  Members may differ in everything else — node count, batch size (the default
 * already follows the node count), filters and scorers, evaluator class: the grid is sized by the
 * largest member, and the group runs the widest evaluator, the 32-bit key table and the role-split
 * resolver as soon as one member needs them (each is exact on the others' domains too).  A member
 * without nodes, or one that has stopped, sits the step out with its status.
 * ks_group_step advances every member by `ticks` ticks with one launch
 * per kernel for all of them (scenario = a grid dimension, one resolve workgroup each) — the
 * reference would run one KubeSim.Run per scenario (kubesim/kubesim.go:90-123).  Per member i:
 * binds into out[i * cap ...] (out may be NULL), their count in n_out[i] and the member's status
 * in status_out[i] (an aborting error stops only that scenario).  Members are destroyed with the
 * group (ks_destroy on a member is a no-op).  stats (may be NULL): device ms of the whole step,
 * batch rounds, pods bound. */
typedef struct ks_group ks_group;
ks_status ks_group_create(int32_t device, int32_t max_scenarios, ks_group** out);
void ks_group_destroy(ks_group* g);
ks_status ks_group_add(ks_group* g, const ks_config* cfg, ks_engine** out);
int32_t ks_group_size(const ks_group* g);

/* Node sharding across ranks (the reference's argmax over all nodes,
 * kubesim/kubesim.go:208-222, becomes an exact merge of per-shard candidate lists).  One
 * process per GPU; every rank loads the whole cluster and submits the same pods, scans only its
 * contiguous node range, and all-gathers the per-pod top-L candidates once per batch over RCCL.
 * Binds are identical on every rank.  Call on every rank before ks_load_nodes; rank 0 creates
 * the communicator id with ks_comm_unique_id and the host broadcasts it (any channel).
 * vshards > 1 splits each rank's range further (same merge path; lets one GPU test it).
 * id may be NULL when world == 1 (no communicator). */
/* The layout ks_load_nodes and ks_step use for n_nodes over world ranks x vshards parts:
 * part_lo_out[world * vshards + 1] = first 256-node scan block of each part (the last entry = the
 * block count); rank r scans parts [r * vshards, (r + 1) * vshards).  Exchange: part p's per-pod
 * top-L keys fill cand_all[p][B][L]; rank r's parts are one contiguous all-gather slice; the
 * second merge reads cand_all[p][b][*] for every part p.  Pure host function (no device). */
ks_status ks_shard_layout(int64_t n_nodes, int32_t world, int32_t vshards, int32_t* part_lo_out);
/* The second merge on the host: out[B][L] = exact top-L over parts of cand_all[parts][B][L]
 * (each list sorted descending, 0-padded) — the device merge's per-list step (topl_insert,
 * ks_device.h), for checking an exchange without a GPU.  Pure host function. */
ks_status ks_merge_candidates(const uint64_t* cand_all, int32_t parts, int32_t B, uint64_t* out);
#define KS_COMM_ID_BYTES 128
ks_status ks_comm_unique_id(uint8_t* id_out /* [KS_COMM_ID_BYTES] */);
ks_status ks_shard(ks_engine* eng, int32_t world, int32_t rank, const uint8_t* id, int32_t vshards);
/* The same sharding with a host exchange instead of RCCL (no communicator): at every batch the
 * engine copies this rank's parts of cand_all[G][B][L] to host memory and calls fn with a buffer of
 * world x bytes_per_rank bytes (rank-major, this rank's slice filled); fn must fill the other
 * ranks' slices (an all-gather) and return KS_OK, after which the whole array goes back to the
 * device.  For ranks that share no RCCL communicator: threads of one process on one or several
 * GPUs (ks_local_allgather, ks_kubesim.h), or any host transport.  Before ks_load_nodes. */
typedef ks_status (*ks_allgather_fn)(void* user, int32_t rank, int32_t world, void* buf, int64_t bytes_per_rank);
ks_status ks_shard_host(ks_engine* eng, int32_t world, int32_t rank, int32_t vshards, ks_allgather_fn fn,
                        void* user);

/* Load the cluster (once).  alloc[n][4] = {cpu, memory, nvidia.com/gpu, pods};
 * taint[n] = OR of dictionary bits of the node's NoSchedule/NoExecute taints;
 * label[n] = OR of dictionary bits of its (key,value) labels (W = 1). */
ks_status ks_load_nodes(ks_engine* eng, int64_t n, const int64_t* alloc, const uint64_t* taint,
                        const uint64_t* label);

/* Append m pods to the FIFO.  arrival_tick = the tick whose Submit call returned the pod
 * (non-decreasing; <= the current tick means "next tick").  req[m][3] container-summed
 * requests with keymask (1 cpu, 2 memory, 4 gpu); tol = dictionary taints tolerated; sel =
 * dictionary labels required (bit 63 = impossible); simSpec as CSR: phase_off[m+1],
 * phase_sec[Φ] (int32), phase_use[Φ][3]; flags = KS_PODFLAG_* (may be NULL).
 *
 * key_id[m] (>= 0; may be NULL: every pod its own key, key id = -(FIFO index) - 1, a namespace
 * no explicit key shares): the caller's interned
 * "namespace-name" pod key (kubesim/node/node.go:146-160).  Node.CreatePod stores the pod under
 * its key, replacing a same-key pod already stored on that node (node.go:58,
 * kubesim/pod/podmap.go:27-29); a replaced pod that is still running stops counting toward the
 * node's totals at that moment.  The engine keeps placements exact by refusing, with KS_ERANGE
 * and nothing appended, a pod whose key was used by an earlier pod that may still be running at
 * the new pod's bind tick (the only case in which the replacement can change a placement or a
 * usage; which node each lands on is not known at submit).  Reused keys of finished pods are
 * accepted and resolved exactly by ks_pod_lookup / ks_node_pods. */
ks_status ks_submit_pods(ks_engine* eng, int64_t m, const int64_t* arrival_tick,
                         const int64_t* req, const uint8_t* keymask, const uint64_t* tol,
                         const uint64_t* sel, const int32_t* phase_off, const int32_t* phase_sec,
                         const int64_t* phase_use, const uint8_t* flags, const int64_t* key_id);

/* Advance `ticks` ticks.  Writes up to `cap` binds to out (one per tick that had a queued
 * pod) and the number of binds made to *n_out.
 *
 * Domain: Pod.passedSeconds is int32(seconds since the pod's start) (kubesim/pod/pod.go:148-153);
 * past 2^31 s Go's conversion is implementation-defined and IsRunning (pod.go:67-69) may revive
 * finished pods.  A step that would take the clock 2^31 s or more past the run's first bind, and
 * a ks_submit_pods whose pods would bind there, are refused with KS_ERANGE (nothing changes). */
ks_status ks_step(ks_engine* eng, int64_t ticks, ks_bind* out, int64_t cap, int64_t* n_out);

/* Filter mask (all enabled filters) / aggregated score (-1 = no entry) of queued pod `pod`
 * against the cluster state at the current tick.  mask_out[n], score_out[n]. */
ks_status ks_filter(ks_engine* eng, int64_t pod, uint8_t* mask_out);
ks_status ks_score(ks_engine* eng, int64_t pod, int64_t* score_out);

/* usage_out[n][3]: Σ over pods on each node of ResourceUsage at the current tick. */
ks_status ks_usage(ks_engine* eng, int64_t* usage_out);

/* usage_out[n][3] at any past tick 0 <= t <= the current tick (Pod.ResourceUsage,
 * kubesim/pod/pod.go:47-63, sampled after tick t's bind): placements of every pod bound by t are
 * final, so any tick of a batched ks_step can be read back.  Cost: the pods that may run at t
 * (an index over run intervals skips finished pods), not the run's length. */
ks_status ks_usage_at(ks_engine* eng, int64_t t, int64_t* usage_out);

/* Per-tick usage digest for ticks t_lo <= t < t_hi (t_hi - 1 <= the current tick, t_hi - t_lo
 * <= 2^20): out[(t - t_lo) * 6 + k] for k = 0..2 is Σ over nodes of usage[node][k] at tick t, and
 * for k = 3..5 Σ over nodes of ks_node_mix(node) * usage[node][k - 3] (mod 2^64) — a per-tick
 * fingerprint of the whole [n][3] usage matrix, computed from the pods' phase segments
 * (difference arrays + a prefix sum) instead of one [n][3] reduction per tick. */
ks_status ks_usage_digest(ks_engine* eng, int64_t t_lo, int64_t t_hi, uint64_t* out);
/* the digest's node weight: z = (node + 1) * 0x9E3779B97F4A7C15, then the splitmix64 finaliser
 * (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31) */
uint64_t ks_node_mix(int64_t node);

/* Scheduler state at past ticks, rebuilt from the binds (final once made).  "At tick t" is sampled
 * after tick t's bind, as ks_usage_at; 0 <= t <= the current tick.  A pod counts on its node while
 * it was bound Ok and 0 <= t - bind tick < its run length in ticks (Pod.IsRunning,
 * kubesim/pod/pod.go:67-69, int32 arithmetic included); OverCapacity pods never count.  Quantities
 * are int64 milli-units.  All of them answer after an aborted run (KS_ENOTFOUND / KS_EINVAL) on the
 * binds made before it, on sharded engines and on scenario-group members.  Cost: the pods that
 * run in, or are bound in, the queried ticks (the usage queries' run-interval index), not the
 * run's length.
 *
 * ks_requested_at: out[n][4] = per node {Σ requested cpu, memory, nvidia.com/gpu, running pods}
 * over the pods running at t — Node.totalResourceRequest and runningPodsNum
 * (kubesim/node/node.go:97-118), the state CreatePod's admission test reads (node.go:44-47). */
ks_status ks_requested_at(ks_engine* eng, int64_t t, int64_t* out);
/* ks_filter_at / ks_score_at: what ks_filter / ks_score would have returned for the already-bound
 * pod `pod` at the moment scheduleOne handled it — the filtered node list and the nodeScore map the
 * reference logs per pod (kubesim/kubesim.go:170,184,194,205): node state = the pods before it in
 * the FIFO that run at its bind tick, with the cluster's alloc / taints / labels.  The lowest-index
 * argmax of score_out is the node the pod was bound to (kubesim.go:208-222).  KS_EINVAL for a pod
 * that is not bound: queued (use ks_filter / ks_score), out of range, or the pod an aborted run
 * stopped at.  mask_out[n], score_out[n] (-1 = no entry). */
ks_status ks_filter_at(ks_engine* eng, int64_t pod, uint8_t* mask_out);
ks_status ks_score_at(ks_engine* eng, int64_t pod, int64_t* score_out);
/* ks_cluster_series: cluster-wide curves for ticks t_lo <= t < t_hi (t_hi - 1 <= the current tick,
 * t_hi - t_lo <= 2^20): out[(t - t_lo) * KS_SERIES_COLS + c], c = 0 running pods; 1..3 Σ over nodes
 * of requested cpu / memory / gpu (Σ_n ks_requested_at(t)); 4 pods bound Ok so far; 5 pods bound
 * OverCapacity so far (PodFailed, kubesim/pod/pod.go:20-27); 6 pending = pods arrived by t minus
 * pods taken off the queue by t (len(podQueue) after tick t's scheduleOne, kubesim/podqueue.go:18-42;
 * the pod an aborted run stopped at was popped, kubesim/kubesim.go:144-158).  Arrival = the tick the
 * bind-tick recurrence used: an arrival_tick at or before the tick of its ks_submit_pods call counts
 * as the next tick. */
#define KS_SERIES_COLS 7
ks_status ks_cluster_series(ks_engine* eng, int64_t t_lo, int64_t t_hi, int64_t* out);
/* ks_node_peaks: out[n][4] = per node and column the maximum of ks_requested_at(t) over
 * t_lo <= t < t_hi (window bounds as ks_cluster_series) — how full each node got; what a sweep of
 * Node.totalResourceRequest / runningPodsNum (kubesim/node/node.go:97-118) over every tick of the
 * window would find.  Extra cost: per node, the square of its pods that run in the window. */
ks_status ks_node_peaks(ks_engine* eng, int64_t t_lo, int64_t t_hi, int64_t* out);

/* Headroom: how many more pods of a shape fit, at any past tick ("at tick t" as above: after tick
 * t's bind, 0 <= t <= the current tick).  A shape is a pod template in ks_submit_pods' fields and
 * units: req[3] (cpu, memory, nvidia.com/gpu; int64 milli-units), keymask (1 cpu, 2 memory, 4 gpu),
 * tol and sel masks.  Shapes are never appended to the FIFO and change no engine state (no unit
 * rescale: a request need not be a multiple of anything the engine holds).
 *
 * The count c(node, shape) is the number of copies of the shape Node.CreatePod would give status Ok
 * when handed them one after another at tick t with nothing finishing in between — its admission
 * test (kubesim/node/node.go:44-47) against Node.totalResourceRequest / runningPodsNum
 * (node.go:97-118, ks_requested_at(t)), applied repeatedly.  In closed form, with A the node's
 * alloc, r its requested state at t and q the shape's request, as exact integers:
 *   per key k in keymask: 0 if the node lacks the key (alloc -1; also for a request of 0,
 *     kubesim/node/resource.go:54-55); no bound if q[k] = 0; else floor((A[k] - r[k]) / q[k]);
 *   pods: max(alloc pods - running pods, 0) (runningPodsNum >= cap.Pods(), node.go:47);
 *   every bound is clamped to KS_HEADROOM_NODE_MAX = 2^31 - 1 (per-node counts stay int32, every
 *   sum stays inside int64) and c is the minimum of the bounds.
 * The limiting key is the first bound, in the order cpu, memory, gpu, pods, that attains the minimum
 * (a key without a bound never limits; at the clamp it is the first bound that reaches the clamp).
 * Every eligible node has exactly one limiting key, also when c = 0.  The admission test always
 * applies, whatever filters are registered.  A node is eligible for a shape unless the engine runs
 * KS_FILTER_FEEDS_SCORE with KS_FILTER_TAINT and / or KS_FILTER_SELECTOR and the shape fails that
 * predicate on it ((taint & ~tol) == 0, (label & sel) == sel: toleration.go:37-56 and the
 * nodeSelector match, as ks_filter); in KS_FILTER_REFERENCE_LITERAL mode every node is eligible
 * (kubesim/kubesim.go:182 discards the Filter result).  An ineligible node has c = 0 and no
 * limiting key.
 *
 * ks_headroom_at: out[k][KS_HEADROOM_COLS] per shape: 0 = sum over nodes of c; 1 = nodes with
 * c >= 1; 2 = the largest c; 3 = the lowest node index attaining column 2, or -1 when column 2 is 0;
 * 4..7 = eligible nodes whose limiting key is cpu / memory / gpu / pods; 8 = ineligible nodes
 * (columns 4..8 sum to n).  per_node_out (may be NULL): [k][n] the counts.  With n = 0: KS_OK,
 * zeros and column 3 = -1.
 * ks_headroom_series: out[t_hi - t_lo][k][2] = columns 0 and 1 of ks_headroom_at at every tick
 * t_lo <= t < t_hi (window bounds as ks_cluster_series; also k * (t_hi - t_lo) <= 2^22).  Cost: the
 * pods that run in the window (per node, the square of them, as ks_node_peaks) times k — not one
 * pass over the cluster per tick.
 * KS_EINVAL: a NULL engine, req, keymask, tol, sel or out (before the handle is read); k outside
 * 1..KS_HEADROOM_MAX_SHAPES; a keymask bit above 4; a request that is negative or >= 2^59 in a
 * masked key (unmasked keys are ignored); t or the window out of range; no nodes loaded.  Both
 * answer after an aborted run, on sharded engines and on scenario-group members, like the state
 * queries above. */
#define KS_HEADROOM_COLS 9
#define KS_HEADROOM_MAX_SHAPES 64
#define KS_HEADROOM_NODE_MAX 2147483647
ks_status ks_headroom_at(ks_engine* eng, int64_t t, int32_t k, const int64_t* req /* [k][3] */,
                         const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel,
                         int64_t* out /* [k][KS_HEADROOM_COLS] */, int32_t* per_node_out /* [k][n] or NULL */);
ks_status ks_headroom_series(ks_engine* eng, int64_t t_lo, int64_t t_hi, int32_t k, const int64_t* req,
                             const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel,
                             int64_t* out /* [t_hi - t_lo][k][2] */);

/* Placement preview: where k more pods would be bound, at any past tick ("at tick t" as above: after
 * tick t's bind, 0 <= t <= the current tick).  The k preview pods are handed, one after another in
 * the order given and all at tick t with nothing finishing in between, to scheduleOne
 * (kubesim/kubesim.go:143-225) on a private copy of the state at t: no engine state changes.
 *
 * A pod's shape is exactly a headroom shape: req[3] in int64 milli-units, keymask, tol, sel; unmasked
 * keys are ignored, a request need not be a multiple of anything the engine holds (it is never
 * queued, there is no unit rescale).  Pod j has shape shape_of[j]; with shape_of NULL, k must equal
 * n_shapes and pod j has shape j.
 *
 * Each pod goes through the engine's configured filter mode, filters and scorers exactly as in
 * ks_step: the Filter loop (kubesim.go:168-188; its result gates the candidates only in
 * KS_FILTER_FEEDS_SCORE mode, kubesim.go:182 discards it) and the score aggregation
 * (kubesim.go:190-206) on ks_requested_at(t) plus the preview pods already placed Ok; the highest
 * aggregated score wins, the lowest node index among equals (kubesim.go:208-222).  Node.CreatePod's
 * admission test then gives KS_POD_OK or KS_POD_OVER_CAPACITY (kubesim/node/node.go:44-47); only an Ok
 * placement adds the pod's masked requests and one running pod to its node (node.go:58, 97-118).
 * Preview pods carry fresh keys (no Store replaces a stored pod), no flags, and never expire.
 * A pod for which the nodeScore map is empty — no candidate node, or no scorer registered — gets
 * KS_PLACE_NOT_FOUND, node -1, score -1; it changes nothing and the preview goes on with the next
 * pod.  (A run aborts there with KS_ENOTFOUND, kubesim.go:218-220; a preview reports it per pod.)
 *
 * out[k]: node (-1: none), status, score (the chosen node's aggregated score as ks_score gives it,
 * -1: none), candidates (the nodes with an entry in the nodeScore map at this pod's turn; in
 * KS_FILTER_REFERENCE_LITERAL mode with scorers: n).  after_out (may be NULL): [n][4]
 * ks_requested_at(t) plus every Ok placement, milli-units and running pods.  info_out (may be NULL):
 * {rounds of the device algorithm (0 with n = 0), pods placed Ok, pods placed OverCapacity, pods
 * not found}.  With n = 0: KS_OK and every pod is KS_PLACE_NOT_FOUND with 0 candidates.
 * KS_EINVAL: a NULL engine, req, keymask, tol, sel or out (before the handle is read); n_shapes
 * outside 1..KS_PLACE_MAX_SHAPES; k outside 1..KS_PLACE_MAX_PODS; a shape_of entry outside
 * [0, n_shapes); a NULL shape_of with k != n_shapes; a keymask bit above 4; a request that is negative
 * or >= 2^59 in a masked key; t out of range; no nodes loaded.  It answers after an aborted run, on
 * sharded engines and on scenario-group members, like the state queries above: it reads the bind
 * arrays, the pod records and the cluster's alloc / taints / labels only. */
#define KS_PLACE_MAX_PODS 1024
#define KS_PLACE_MAX_SHAPES 64 /* = KS_HEADROOM_MAX_SHAPES */
#define KS_PLACE_NOT_FOUND (-1) /* status of a pod no node was selected for */
#define KS_PLACE_INFO 4
typedef struct {
    int32_t node;       /* bind node, -1 when none */
    int32_t status;     /* KS_POD_OK, KS_POD_OVER_CAPACITY, KS_PLACE_NOT_FOUND */
    int64_t score;      /* aggregated score of the chosen node (as ks_score), -1 when none */
    int64_t candidates; /* nodes with an entry in the nodeScore map at this pod's turn */
} ks_placement;
ks_status ks_place_at(ks_engine* eng, int64_t t, int32_t n_shapes, const int64_t* req /* [n_shapes][3] */,
                      const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel, int32_t k,
                      const int32_t* shape_of /* [k], or NULL: k == n_shapes, pod j is shape j */,
                      ks_placement* out /* [k] */, int64_t* after_out /* [n][4] or NULL */,
                      int64_t* info_out /* [KS_PLACE_INFO] or NULL */);

/* Drain preview: where the pods running on a set of nodes would go if those nodes were taken out, at
 * any past tick ("at tick t" as above: after tick t's bind, 0 <= t <= the current tick).  No engine
 * state changes.
 *
 * nodes[n_drain] are distinct node indices in [0, n), 1 <= n_drain <= n (with n = 0: n_drain = 0).
 * The drained nodes leave k.nodes: from then on they are in no Filter loop and no score map
 * (kubesim/kubesim.go:168-206 range over k.nodes).  Every pod running on a drained node at t is
 * evicted — running as ks_requested_at counts it: bound Ok with 0 <= t - bind tick < its run length
 * (Pod.IsRunning, kubesim/pod/pod.go:67-69); OverCapacity pods and finished pods are not evicted.
 * The evicted pods are handed in FIFO order (ascending pod index), all at tick t with nothing
 * finishing in between, to scheduleOne (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60) on a
 * private copy of the state: ks_requested_at(t) with the drained nodes' rows emptied.  Each pod goes
 * through the engine's configured filter mode, filters and scorers exactly as in ks_place_at; its own
 * record supplies req / keymask / tol / sel, its flags are ignored.  Statuses, the rule that a
 * KS_PLACE_NOT_FOUND pod changes nothing and the preview goes on, score and candidates are
 * ks_place_at's; in KS_FILTER_REFERENCE_LITERAL mode with scorers candidates = n - n_drain.
 * Keys: ks_submit_pods refuses a key reused while an earlier holder may still run, so the Store of an
 * evicted pod on its new node (node.go:58) can only replace a finished pod, which changes no totals.
 *
 * *n_out = the number of evicted pods, always.  If it exceeds cap or KS_DRAIN_MAX_PODS: KS_ERANGE and
 * nothing else is written — the caller sizes out and calls again; cap = 0 with out NULL is the sizing
 * call (KS_OK when nothing is evicted).  out[*n_out]: the evicted pod, the node it ran on, and its
 * ks_placement fields.  after_out (may be NULL): [n][4] milli-units and running pods, the emptied state
 * plus every Ok re-placement; the drained nodes' rows are zero.  info_out (may be NULL):
 * {rounds of the device algorithm, re-placed Ok, OverCapacity, not found, segments (the rounds take
 * KS_PLACE_MAX_SHAPES distinct shapes and KS_PLACE_MAX_PODS pods at a time), drained nodes that had no
 * running pod}.  With n = 0 or no evicted pod: KS_OK, *n_out = 0, after_out = the emptied state.
 * KS_EINVAL: a NULL engine, nodes or n_out (before the handle is read); out NULL with cap > 0; cap < 0;
 * a node out of range or listed twice; n_drain out of range; t out of range; no nodes loaded.  It
 * answers after an aborted run, on sharded engines and on scenario-group members, like the state
 * queries above: it reads the bind arrays, the pod records and the cluster's alloc / taints / labels
 * only. */
#define KS_DRAIN_MAX_PODS 65536
#define KS_DRAIN_INFO 6
typedef struct {
    int64_t pod;        /* the evicted pod (FIFO index) */
    int32_t from;       /* the drained node it ran on */
    int32_t node;       /* the node it would be bound to, -1 when none */
    int32_t status;     /* KS_POD_OK, KS_POD_OVER_CAPACITY, KS_PLACE_NOT_FOUND */
    int32_t pad;
    int64_t score;      /* aggregated score of the chosen node, -1 when none */
    int64_t candidates; /* nodes with an entry in the nodeScore map at this pod's turn */
} ks_eviction;
ks_status ks_drain_at(ks_engine* eng, int64_t t, int32_t n_drain, const int32_t* nodes /* [n_drain] */,
                      ks_eviction* out /* [cap] or NULL */, int64_t cap, int64_t* n_out,
                      int64_t* after_out /* [n][4] or NULL */, int64_t* info_out /* [KS_DRAIN_INFO] or NULL */);

/* Removal scan: which of m candidate nodes could each be taken out on its own, at any past tick ("at
 * tick t" as above).  No engine state changes.
 *
 * nodes[m] are distinct node indices in [0, n), 1 <= m <= n (with n = 0: m = 0).  For candidate c the
 * answer is by definition that of ks_drain_at(t, 1, {c}): c alone leaves k.nodes
 * (kubesim/kubesim.go:168-206 range over k.nodes), the pods running on it at t (Pod.IsRunning,
 * kubesim/pod/pod.go:67-69) are evicted and handed in FIFO order to scheduleOne
 * (kubesim/kubesim.go:143-225, kubesim/node/node.go:36-60) on a private copy of ks_requested_at(t)
 * with c's row emptied; each pod's node / status / score / candidates are ks_drain_at's.  Candidates
 * are independent: none sees another's evictions or placements.
 *
 * out[j] answers nodes[j], in the caller's order: the pods running on it, the statuses of their
 * re-placements, removable = 1 iff every one of them was re-bound KS_POD_OK (also when none runs
 * there), and first_row, the index of its first row — filled whether or not rows are asked for.
 * rows_out (may be NULL with cap = 0: summaries only): the candidates' ks_eviction rows concatenated
 * in the caller's order, FIFO within a candidate.  *n_rows = the total of evicted pods, always.  If it
 * exceeds KS_DRAIN_MAX_PODS, or rows_out is given and it exceeds cap: KS_ERANGE and nothing else is
 * written.  info_out (may be NULL): {segments (the shared lists take KS_PLACE_MAX_SHAPES distinct
 * shapes at a time), candidates resolved by the batched kernel, candidates answered through the
 * single-drain path (more pods than one set of lists decides: KS_PLACE_L - 1), candidates with no
 * running pod, removable candidates, evicted pods}.
 * KS_EINVAL: a NULL engine, nodes, out or n_rows (before the handle is read); rows_out NULL with
 * cap > 0; cap < 0; a node out of range or listed twice; m out of range; t out of range; no nodes
 * loaded.  It answers after an aborted run, on sharded engines and on scenario-group members, like
 * ks_drain_at. */
#define KS_REMOVABLE_INFO 6
typedef struct {
    int32_t node;          /* the candidate */
    int32_t evicted;       /* pods running on it at t */
    int32_t ok, over_capacity, not_found;   /* statuses of their re-placements */
    int32_t removable;     /* 1 iff ok == evicted (also when evicted == 0) */
    int64_t first_row;     /* index of its first row in rows_out (rows of a candidate are contiguous) */
} ks_removal;              /* 32 bytes */
ks_status ks_removable_at(ks_engine* eng, int64_t t, int32_t m, const int32_t* nodes /* [m] */,
                          ks_removal* out /* [m] */, ks_eviction* rows_out /* [cap] or NULL */,
                          int64_t cap, int64_t* n_rows, int64_t* info_out /* [KS_REMOVABLE_INFO] or NULL */);

/* Consolidation preview: which of m candidate nodes a scale-down pass would remove when it handles
 * them one after another, at any past tick ("at tick t" as above).  No engine state changes.
 *
 * nodes[m] are distinct node indices in [0, n), 1 <= m <= n (with n = 0: m = 0).  The call keeps a
 * private copy of ks_requested_at(t), a set R of removed nodes and a set V of destination nodes, both
 * empty at the start, and handles the candidates in the caller's order.  For candidate c:
 *   - c in V: KS_CONSOLIDATE_DESTINATION.  Nothing is tried, no rows are written, nothing changes.
 *   - otherwise c leaves k.nodes together with R (kubesim/kubesim.go:168-206 range over k.nodes).  The
 *     pods running on c at t — exactly those ks_drain_at would evict from c (Pod.IsRunning,
 *     kubesim/pod/pod.go:67-69) — are handed in FIFO order to scheduleOne (kubesim/kubesim.go:143-225,
 *     kubesim/node/node.go:36-60) on the private state with c's row emptied.  Filter mode, filters,
 *     scorers, score, candidates and the lowest-index tie-break are ks_place_at's and ks_drain_at's;
 *     candidates counts nodes outside R and c.  The attempt ends at the first pod whose status is not
 *     KS_POD_OK; later pods of c are not tried.
 *   - every pod bound Ok, or none runs on c: KS_CONSOLIDATE_REMOVED.  c joins R, its row stays zero,
 *     the placements stay and every node that received a pod joins V.
 *   - otherwise KS_CONSOLIDATE_BLOCKED: the private state, V and R are exactly what they were before
 *     c; c stays in k.nodes with its pods and may still become a destination of a later candidate.
 * A removed node is never in V and a node in V is never removed.
 *
 * out[j] answers nodes[j].  *n_evicted = the pods running on all candidates, the upper bound of the
 * rows, always written.  If it exceeds KS_DRAIN_MAX_PODS, or rows_out is given and cap is smaller:
 * KS_ERANGE and nothing else is written.  rows_out (may be NULL with cap = 0: summaries only; rows and
 * first_row are filled all the same): ks_eviction rows concatenated in the caller's order, FIFO within
 * a candidate — all of a removed candidate's pods, a blocked candidate's up to and including the
 * blocking pod, none of a destination's.  *n_rows = the rows written.  after_out (may be NULL): [n][4]
 * milli-units and running pods, the final private state: removed nodes' rows zero, plus every kept
 * placement.  info_out (may be NULL): {rounds of the device algorithm, removed, blocked, destinations,
 * candidates decided through the single path (more pods than one set of lists decides: KS_PLACE_L - 1,
 * and no destination), pods moved = the rows of removed candidates}.
 * KS_EINVAL: a NULL engine, nodes, out, n_evicted or n_rows (before the handle is read); rows_out NULL
 * with cap > 0; cap < 0; a node out of range or listed twice; m out of range; t out of range; no nodes
 * loaded.  It answers after an aborted run, on sharded engines and on scenario-group members, like
 * ks_drain_at. */
enum { KS_CONSOLIDATE_BLOCKED = 0, KS_CONSOLIDATE_REMOVED = 1, KS_CONSOLIDATE_DESTINATION = 2 };
#define KS_CONSOLIDATE_INFO 6
typedef struct {
    int32_t node;          /* the candidate */
    int32_t evicted;       /* pods running on it at t (also when nothing was tried) */
    int32_t outcome;       /* KS_CONSOLIDATE_* */
    int32_t rows;          /* rows written for it: evicted when removed; up to and including the
                              blocking pod when blocked; 0 for a destination */
    int32_t block_status;  /* blocked: the blocking pod's status (KS_POD_OVER_CAPACITY / KS_PLACE_NOT_FOUND); else 0 */
    int32_t pad;
    int64_t first_row;     /* index of its first row in rows_out */
} ks_consolidation;        /* 32 bytes */
ks_status ks_consolidate_at(ks_engine* eng, int64_t t, int32_t m, const int32_t* nodes /* [m] */,
                            ks_consolidation* out /* [m] */, ks_eviction* rows_out /* [cap] or NULL */,
                            int64_t cap, int64_t* n_evicted, int64_t* n_rows,
                            int64_t* after_out /* [n][4] or NULL */, int64_t* info_out /* [KS_CONSOLIDATE_INFO] or NULL */);

/* Gang admission preview: which of m pod groups (gangs: the PodGroup minMember of coscheduling,
 * all-or-nothing admission) a queue would admit when it handles them one after another, and where
 * their pods would be bound, at any past tick ("at tick t" as above).  No engine state changes.
 *
 * Shapes (n_shapes, req, keymask, tol, sel) and the k pods' shape_of are ks_place_at's; shape_of is
 * required, and a call takes up to KS_GANG_MAX_SHAPES shapes and KS_GANG_MAX_PODS pods.  Gang g is pods
 * first[g] .. first[g + 1] - 1: first[0] = 0, first is non-decreasing, first[m] = k; an empty gang is
 * allowed.  min_ok[g] lies in 0 .. size (NULL: size, all-or-nothing).  The call keeps one private
 * copy of ks_requested_at(t) and handles the gangs in the caller's order.  For gang g:
 *   - its pods go one after another to scheduleOne (kubesim/kubesim.go:143-225,
 *     kubesim/node/node.go:36-60) on the private state, exactly as ks_place_at would handle them: filter
 *     mode, filters, scorers, score, candidates and the lowest-index tie-break are ks_place_at's.  A pod
 *     bound Ok adds to its node; a pod bound OverCapacity or not found (KS_PLACE_NOT_FOUND) changes
 *     nothing and the attempt goes on.  The attempt ends as soon as the pods not bound Ok number more
 *     than size - min_ok; later pods of g are not tried, and that pod's status is block_status.
 *   - at least min_ok pods bound Ok at its end (also an empty gang, also min_ok = 0): KS_GANG_ADMITTED.
 *     Every Ok placement stays for the later gangs.
 *   - otherwise KS_GANG_BLOCKED: the private state is exactly what it was before g.
 *   - with KS_GANG_STRICT in flags every gang after the first blocked one is KS_GANG_SKIPPED and
 *     nothing is tried; without it the pass goes on (backfill).
 * So with every gang admitted the rows are ks_place_at's on the k pods, and gang g's tried rows are
 * the tail of ks_place_at on the pods of the gangs admitted before g followed by g's pods.
 *
 * out[g] answers gang g.  rows_out (may be NULL: summaries only) answers pod j at index j: a tried pod
 * gets the ks_placement it had in its attempt (a blocked gang's rows show the attempt that was rolled
 * back), an untried pod {-1, KS_GANG_NOT_TRIED, -1, 0}.  after_out (may be NULL): [n][4] milli-units
 * and running pods, the final private state.  info_out (may be NULL): {rounds of the device
 * algorithm, admitted, blocked, skipped, gangs decided through the single path (more pods than one
 * set of lists decides: KS_PLACE_L), Ok pods of admitted gangs}.
 * KS_EINVAL, and nothing is written: ks_place_at's argument errors; a NULL shape_of, first or out
 * (before the handle is read); first[0] != 0, first decreasing or first[m] != k; a min_ok outside
 * 0 .. size; an unknown flag bit; k outside [1, KS_GANG_MAX_PODS]; m outside [1, KS_GANG_MAX_GANGS];
 * n_shapes outside [1, KS_GANG_MAX_SHAPES].  It answers after an aborted run, on sharded engines and on
 * scenario-group members, like ks_place_at. */
#define KS_GANG_MAX_GANGS  65536
#define KS_GANG_MAX_PODS   65536   /* = KS_DRAIN_MAX_PODS */
#define KS_GANG_MAX_SHAPES 4096
#define KS_GANG_NOT_TRIED  (-2)    /* status of a pod no attempt reached */
#define KS_GANG_STRICT     1u      /* flags: the first blocked gang ends the pass */
enum { KS_GANG_BLOCKED = 0, KS_GANG_ADMITTED = 1, KS_GANG_SKIPPED = 2 };
#define KS_GANG_INFO 6
typedef struct {
    int32_t first, size;      /* its pods: rows [first, first + size) */
    int32_t outcome;          /* KS_GANG_* */
    int32_t tried;            /* pods the attempt handled: size when admitted; up to and including the
                                 deciding pod when blocked; 0 when skipped */
    int32_t ok, over_capacity, not_found;  /* statuses among the tried pods */
    int32_t block_status;     /* blocked: status of the pod that decided it; else 0 */
} ks_gang;                    /* 32 bytes */
ks_status ks_gang_at(ks_engine* eng, int64_t t, int32_t n_shapes, const int64_t* req /* [n_shapes][3] */,
                     const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel,
                     int32_t k, const int32_t* shape_of /* [k] */,
                     int32_t m, const int32_t* first /* [m + 1] */, const int32_t* min_ok /* [m] or NULL */,
                     uint32_t flags, ks_gang* out /* [m] */, ks_placement* rows_out /* [k] or NULL */,
                     int64_t* after_out /* [n][4] or NULL */, int64_t* info_out /* [KS_GANG_INFO] or NULL */);

/* Scale-up preview: where k pending pods would be bound if up to max_nodes nodes of a node-group
 * template were added, at any past tick ("at tick t" as above), for n_options templates, each on its
 * own.  No engine state changes.
 *
 * Shapes, shape_of, k and the per-pod fields are exactly ks_place_at's.  The answer for option g is
 * by definition that of ks_place_at on a cluster that is the engine's cluster plus options[g].max_nodes
 * empty nodes of option g's template: the appended nodes come after the n real ones, at indices
 * n .. n + max_nodes - 1 — in effect k.nodes is extended before the Filter loop
 * (kubesim/kubesim.go:168-206 range over k.nodes); each has the template's alloc (as ks_load_nodes
 * takes it: cpu, memory, nvidia.com/gpu in milli-units, -1 absent, and the pods capacity), taint and
 * label, no requested quantities and no running pods (kubesim/node/node.go:36-60 on a fresh node).
 * The same filter mode, filters and scorers apply; the highest aggregated score wins, the lowest
 * index among equals (kubesim.go:208-222), so a real node beats an equal appended node.
 * Node.CreatePod's admission test (kubesim/node/node.go:44-47) and the KS_PLACE_NOT_FOUND rule apply
 * as in ks_place_at; candidates counts appended nodes too; a row's node >= n names appended node
 * node - n.  A template capacity need not be a multiple of anything the engine holds.  Options are
 * independent: none sees another's nodes or placements.
 *
 * out[g]: the statuses of option g's k pods, on_new (pods bound KS_POD_OK to an appended node),
 * nodes_used (appended nodes holding at least one Ok pod), first_unplaced (the first pod whose status
 * is not KS_POD_OK, -1 if none) and path: 0 when the batched kernel decided the option from the one
 * shared scan, 1 when it was answered by ks_place_at's own rounds on the extended cluster (the
 * batched kernel stops at a pod whose snapshot list is used up; the result is the same by
 * definition).  rows_out (may be NULL): [n_options][k] ks_placement.  info_out (may be NULL):
 * {options decided by the batched kernel, options answered through the single path, options in
 * which every pod was bound Ok, distinct shapes (n_shapes)}.  With n = 0 the call still works: the
 * appended nodes are the whole cluster.
 * KS_EINVAL with nothing written: ks_place_at's argument errors (a NULL engine, req, keymask, tol or
 * sel before the handle is read), a NULL options or out (likewise), n_options outside
 * 1..KS_SCALEUP_MAX_OPTIONS, max_nodes outside 0..KS_SCALEUP_MAX_NODES, an alloc below -1 or
 * >= 2^59, a pods count < 0 or >= 2^59, a non-zero pad.  It answers after an aborted run, on sharded
 * engines and on scenario-group members, as ks_place_at does. */
#define KS_SCALEUP_MAX_OPTIONS 64
#define KS_SCALEUP_MAX_NODES 65536
#define KS_SCALEUP_INFO 4
typedef struct {
    int64_t alloc[4];      /* cpu, memory, nvidia.com/gpu in milli-units (-1 absent), pods: as ks_load_nodes */
    uint64_t taint, label; /* dictionary bits, as ks_load_nodes */
    int32_t max_nodes;     /* 0..KS_SCALEUP_MAX_NODES copies may be appended */
    int32_t pad;           /* 0 */
} ks_scale_option;         /* 56 bytes */
typedef struct {
    int32_t ok, over_capacity, not_found; /* statuses of the k pods */
    int32_t on_new;         /* pods bound KS_POD_OK to an appended node */
    int32_t nodes_used;     /* appended nodes holding >= 1 Ok pod */
    int32_t first_unplaced; /* first pod whose status is not KS_POD_OK, -1 if none */
    int32_t path;           /* 0 batched kernel, 1 single path */
    int32_t pad;
} ks_scale_result;          /* 32 bytes */
ks_status ks_scale_up_at(ks_engine* eng, int64_t t, int32_t n_shapes, const int64_t* req /* [n_shapes][3] */,
                         const uint8_t* keymask, const uint64_t* tol, const uint64_t* sel, int32_t k,
                         const int32_t* shape_of /* [k], or NULL: k == n_shapes, pod j is shape j */,
                         int32_t n_options, const ks_scale_option* options /* [n_options] */,
                         ks_scale_result* out /* [n_options] */, ks_placement* rows_out /* [n_options][k] or NULL */,
                         int64_t* info_out /* [KS_SCALEUP_INFO] or NULL */);

/* Name-keyed queries over the binds made so far (Node.GetPod / GetPodStatus / GetPodList,
 * kubesim/node/node.go:62-93).  ks_pod_lookup: the FIFO index of the pod stored on `node` under
 * key_id (the last one bound there), KS_ENOTFOUND if none ("pod %q not found").  ks_node_pods:
 * the FIFO indices of every pod stored on `node` (one per key, any bind status), in FIFO order;
 * writes min(count, cap) and the count to *n_out.  Phases/times: ks_pod_status. */
ks_status ks_pod_lookup(ks_engine* eng, int32_t node, int64_t key_id, int64_t* pod_out);
ks_status ks_node_pods(ks_engine* eng, int32_t node, int64_t* pods_out, int64_t cap, int64_t* n_out);

/* Pod status (Pod.BuildStatus, kubesim/pod/pod.go:78-145) at the current tick, for pods
 * [pod_lo, pod_lo + n) of the FIFO: PENDING = not bound (queued, or the pod an aborted run stopped
 * at — the reference never stores it); FAILED = bound OverCapacity (PodFailed / CapacityExceeded);
 * RUNNING / SUCCEEDED = bound Ok and IsRunning (pod.go:67-69) or not.  start_tick = the bind tick
 * (StartTime = start clock + start_tick * tick), total_seconds = Σ phase seconds as the reference's
 * int32 sum (FinishedAt = StartTime + total_seconds, pod.go:165-167). */
enum { KS_PHASE_PENDING = 0, KS_PHASE_RUNNING = 1, KS_PHASE_SUCCEEDED = 2, KS_PHASE_FAILED = 3 };
typedef struct {
    int32_t phase;
    int32_t node;           /* -1 when not bound */
    int64_t start_tick;     /* -1 when not bound */
    int32_t total_seconds;
    int32_t pad;
} ks_pod_info;
ks_status ks_pod_status(ks_engine* eng, int64_t pod_lo, int64_t n, ks_pod_info* out);

int64_t ks_current_tick(const ks_engine* eng);
/* the configured tick in seconds (ks_config.tick_seconds); -1 for NULL */
int32_t ks_tick_seconds(const ks_engine* eng);
int64_t ks_queued_pods(const ks_engine* eng);
const char* ks_last_error(const ks_engine* eng);

/* Timing of the last ks_step on the engine's stream (HIP events, recorded only while
 * ks_set_profiling is on): total device ms; the summed ms of the scan kernel alone, of the
 * resolve kernel alone and of everything else (expire_head, merge, RCCL exchange); the number of
 * batches (one launch of each kernel per batch) and of pods bound. */
typedef struct {
    double step_ms;
    double scan_ms;
    double resolve_ms;
    int64_t launches;
    int64_t pods;
    double other_ms;
} ks_step_stats;
ks_status ks_last_step_stats(const ks_engine* eng, ks_step_stats* out);
/* The same per kernel of the batch chain (profiling on): summed HIP-event ms and launch counts of
 * the window prep (launched for a pass's first batch and on the plain chain; an overlapped batch's
 * window is computed inside the previous chunk kernel), the scan (scan_n: the scan launches actually made —
 * one per batch with, on sharded overlapped engines, the conditional rescan, mostly an empty launch;
 * on a single-shard overlapped engine only a pass's first batch launches one, so scan_n == prep_n
 * and the other batches' scan interval brackets nothing), the list merge (with the candidate lists, a sharded engine's
 * per-part merges and exchange), and the resolve launch — the chunk kernel alone, or fused with the
 * next batch's speculative scan and window prep.  Sharded engines: part_ms = the per-part merges
 * and xchg_ms = the exchange (RCCL all-gather, or the host exchange's copies, callback and wait),
 * both inside merge_ms, xchg_n batches. */
typedef struct {
    double prep_ms, scan_ms, merge_ms, resolve_ms, fused_ms, part_ms, xchg_ms;
    int64_t prep_n, scan_n, merge_n, resolve_n, fused_n, xchg_n;
    /* the pipelined sharded chain (engines the fused overlap does not take): the next batch's
     * speculative scan, part merges and exchange on the second stream beside the resolve (side_n
     * batches), and the main stream's wait for that exchange (inside merge_ms's batches) */
    double side_scan_ms, side_part_ms, side_xchg_ms, wait_ms;
    int64_t side_n;
    /* ks_usage_at calls made while profiling is on (summed since the last ks_step): the usage kernel's
     * HIP-event ms, its launches, and the pods of the candidate blocks it read */
    double usage_ms;
    int64_t usage_n, usage_pods;
} ks_kernel_stats;
ks_status ks_last_step_kernels(const ks_engine* eng, ks_kernel_stats* out);
ks_status ks_group_step(ks_group* g, int64_t ticks, ks_bind* out, int64_t cap, int64_t* n_out,
                        int32_t* status_out, ks_step_stats* stats);
/* Device counters (diagnostics): [0] next pod, [1] step end, [2] error, [3] error pod,
 * [4] batches that committed early (top-L list exhausted), [5] / [6] batches whose lists were
 * rescanned / reused from the previous batch (cumulative, chunk resolver), [8] the binds of the last
 * batched ks_step that the host had copied back and finished before the step's last wait (the early
 * read-back; 0 when the step took none) and [9] those of them that came back below a snapshot of the
 * start counter, on the copy stream. */
ks_status ks_debug_counters(ks_engine* eng, int64_t* out32);
/* Between-step invariants of a chunk-resolver engine (diagnostics / regression tests): out4[0] =
 * nodes whose candidate-slot or first-entry mark is set (must be 0: every batch's commit resets the
 * marks of every node its merge claimed), out4[1] = nodes whose E-index mark is set (must be 0), out4[2] = the most
 * candidate slots any batch claimed so far, out4[3] = the slots whose records are staged (beyond
 * them a batch is cut before the first pod that needs one).  All 0 before the first batch. */
ks_status ks_debug_invariants(ks_engine* eng, int64_t* out4);
/* Diagnostics: the raw batch window workspace (ks_device.h WinWS; *size_out = its size, up to cap
 * bytes copied to out), and — in a -DKS_BATCH_LOG diagnostic build only (KS_EINVAL otherwise) — the
 * pod whose batch the chunk resolver records in it. */
ks_status ks_debug_window(ks_engine* eng, void* out, int64_t cap, int64_t* size_out);
ks_status ks_debug_watch(ks_engine* eng, int64_t pod);
/* Device self-test of an evaluator identity the exactness argument rests on (no engine needed).
 * test 0: the micro evaluator's correction-free LeastRequested floor for every (x, A) with
 * 0 <= x <= A < 2^16 (ks_device.h).  *failures = mismatching cases (0 = pass). */
/* test 1: the whole micro evaluator and its scan form on every usage (uc, um) in [0, Ac + 2] x
 * [0, Am + 2] of thirteen capacity pairs with Ac * Am < 2^24 (both domain edges, primes, multiples
 * of ten, degenerate ones), filters off, three scorer configurations, against exact 64-bit integers. */
/* test 2: merge_cl's score-class list merge (ks_device.h) against the host's topl_insert fold, for list
 * lengths 8 and 12: 1 .. 600 lists at 256 threads and 1,025 / 4,096 at 1,024; one class everywhere, two
 * classes with the boundary inside a lane's run, inside a wave and at a wave boundary, one block holding
 * the whole top class behind blocks holding 1-3, every total distinct, fewer feasible nodes than the list
 * length, empty lists, and threshold-prefix (pruned) lists.  *failures = mismatching output words. */
enum { KS_SELFTEST_LR_MICRO = 0, KS_SELFTEST_MICRO_STATES = 1, KS_SELFTEST_LIST_MERGE = 2 };
ks_status ks_selftest(int32_t device, int32_t test, int64_t* failures);
/* Device batch of the fused Filter + Score evaluator (diagnostics / tests; no engine needed): case i is
 * one node (alloc[i][4] cpu memory gpu pods, -1 absent; run[i][4] requested cpu memory gpu of the running
 * pods and their count; masks[i][0..1] taint, label) and one pod (req[i][3], keymask[i], masks[i][2..3]
 * tolerations, selector), all in device units, under the configuration cfg.  Bit b < 17 of `variants`
 * asks for total1[b][n] (total + 1, 0 = not a candidate): b = 4 g + m is evaluator m (0 wide, 1 narrow,
 * 2 tiny, 3 micro) on state form g (0 the 64-bit node, 1 the 12-word record, 2 the chunk resolver's
 * 32-bit words, 3 the register resolver's entry), b = 16 the scan's form of the micro evaluator.  Bit
 * 17 + j asks for tmax[j][n] and live[j][n], the resolvers' float upper bound of the total and whether
 * any pod can make the node a candidate: j = 4 g + m with g = 0 the 64-bit node, 1 the 32-bit words,
 * 2 the register entry.  Columns not asked for are left untouched.  KS_EINVAL when a value is out of
 * the range ks_load_nodes / ks_submit_pods admit, a usage exceeds its capacity, or the batch leaves
 * the domain of a requested evaluator (micro: capacities < 2^16, cpu * memory < 2^24, weights < 2^24;
 * tiny: capacities and cpu * memory < 2^26; narrow: capacities < 2^29; 32-bit words: < 2^32 - 1). */
typedef struct ks_eval_cfg {
    int32_t filter_feeds;  /* 1: the filters gate the candidates (KS_FILTER_FEEDS_SCORE) */
    uint32_t filters;      /* KS_FILTER_* bits */
    int32_t has_scorers;
    int32_t w_lr, w_ba;    /* summed LeastRequested / BalancedAllocation weights */
    int32_t const_total;   /* sum of weight * value over the constant scorers */
} ks_eval_cfg;
enum { KS_EVAL_TOTAL_COLS = 17, KS_EVAL_PRUNE_COLS = 12, KS_EVAL_SCAN_MICRO = 16, KS_EVAL_PRUNE_BIT = 17,
       KS_EVAL_MAX_CASES = 1 << 22 };
ks_status ks_selftest_eval(int32_t device, const ks_eval_cfg* cfg, int64_t n, const int64_t* alloc,
                           const int64_t* run, const int64_t* req, const uint32_t* keymask, const uint64_t* masks,
                           uint32_t variants, uint32_t* total1, uint32_t* tmax, uint32_t* live);
void ks_set_profiling(ks_engine* eng, int enable);
/* Provenance: the first 16 hex digits of the SHA-256 of the sources the library was built from
 * (kubernetes-simulator_amd/csrc/Makefile HASHED, in that order); the Python binding refuses a
 * library whose id differs from the hash of the sources beside it. */
const char* ks_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
