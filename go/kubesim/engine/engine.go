// Package engine binds kubesim to the MI355X scheduling engine (libks_engine.so, C-ABI in
// include/ks_engine.h) through cgo.
//
// Placement in the reference: this directory is meant to sit at kubesim/engine/ of
// github.com/ordovicia/kubernetes-simulator, with include/ and the built libks_engine.so under
// third_party/ks/ (INTEGRATION.md).  It is written against the reference's interfaces
// (api/scheduler.go, api/submitter.go, kubesim/kubesim.go) and the header; neither this image
// nor the GPU box has a Go toolchain, so it has not been compiled here.
package engine

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/ks/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/ks/lib -lks_engine -Wl,-rpath,${SRCDIR}/../../third_party/ks/lib
#include <stdlib.h>
#include "ks_engine.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/cpuguy83/strongerrors"
	"github.com/pkg/errors"
)

// ErrOutOfDomain: a valid input the engine refuses because it cannot keep results exact for it
// (KS_ERANGE: a quantity that is not a whole number of milli-units, a pod key reused while its
// earlier pod may still run, ...).  The caller may fall back to the reference's Go loop.
var ErrOutOfDomain = errors.New("outside the engine's exact domain")

// Engine is one simulated cluster on one device (a handle is single-threaded, like Run).
// n is the node count of LoadNodes: every per-node output buffer is sized from it, never from a
// caller's argument (the C side always writes n rows).
type Engine struct {
	h *C.ks_engine
	n int
}

func status(e *Engine, rc C.ks_status) error {
	msg := ""
	if e != nil && e.h != nil {
		msg = C.GoString(C.ks_last_error(e.h))
	}
	switch rc {
	case C.KS_OK:
		return nil
	case C.KS_ENOTFOUND: // kubesim/kubesim.go:217-220
		return strongerrors.NotFound(errors.New(msg))
	case C.KS_EINVAL:
		return strongerrors.InvalidArgument(errors.New(msg))
	case C.KS_ERANGE:
		return errors.Wrap(ErrOutOfDomain, msg)
	default:
		return errors.Errorf("ks_engine: device error (%d): %s", int(rc), msg)
	}
}

// Scorer kinds of ks_config (include/ks_engine.h).
const (
	ScorerConst          = C.KS_SCORER_CONST
	ScorerLeastRequested = C.KS_SCORER_LEAST_REQUESTED
	ScorerBalanced       = C.KS_SCORER_BALANCED
)

// Filter bits of ks_config.
const (
	FilterFit      = uint32(C.KS_FILTER_FIT)
	FilterTaint    = uint32(C.KS_FILTER_TAINT)
	FilterSelector = uint32(C.KS_FILTER_SELECTOR)
)

// Engine flags of ks_config (include/ks_engine.h): A/B and test switches; the defaults are the
// engine's choice.
const (
	FlagNoOverlap   = uint32(C.KS_ENGINE_NO_OVERLAP)   // the plain batch chain (no fused next-batch scan)
	FlagPrunedLists = uint32(C.KS_ENGINE_PRUNED_LISTS) // pruned block lists at any cluster size
	FlagSmallE      = uint32(C.KS_ENGINE_SMALL_E)      // test only: E overflows at 128 changed nodes (rescan path)
)

// ScorerSpec is one registered device scorer (registration order is kept).
type ScorerSpec struct {
	Kind, Weight, Value int32
}

// Config of an engine.  FeedsScore=false reproduces the reference literally: its Filter result
// is discarded (kubesim/kubesim.go:182).
type Config struct {
	TickSeconds int
	FeedsScore  bool
	Filters     uint32
	Scorers     []ScorerSpec
	Device      int
	BatchPods   int
	EngineFlags uint32 // Flag* above (0: the engine's defaults)
}

func (c Config) toC() (C.ks_config, error) {
	var cfg C.ks_config
	if len(c.Scorers) > 8 {
		return cfg, strongerrors.InvalidArgument(errors.New("at most 8 scorers"))
	}
	cfg.abi_version = C.KS_ABI_VERSION
	cfg.tick_seconds = C.int32_t(c.TickSeconds)
	if c.FeedsScore {
		cfg.filter_mode = C.KS_FILTER_FEEDS_SCORE
	}
	cfg.filters = C.uint32_t(c.Filters)
	cfg.n_scorers = C.int32_t(len(c.Scorers))
	for i, s := range c.Scorers {
		cfg.scorers[i].kind = C.int32_t(s.Kind)
		cfg.scorers[i].weight = C.int32_t(s.Weight)
		cfg.scorers[i].value = C.int32_t(s.Value)
	}
	cfg.device = C.int32_t(c.Device)
	cfg.batch_pods = C.int32_t(c.BatchPods)
	cfg.engine_flags = C.uint32_t(c.EngineFlags)
	return cfg, nil
}

// New creates an engine (ks_create).
func New(c Config) (*Engine, error) {
	cfg, err := c.toC()
	if err != nil {
		return nil, err
	}
	e := &Engine{}
	if rc := C.ks_create(&cfg, &e.h); rc != C.KS_OK {
		return nil, errors.Errorf("ks_create rejected the configuration (%d)", int(rc))
	}
	// A caller written against the reference API never calls Close (kubesim.KubeSim has none):
	// the device state is released when the Engine becomes unreachable.
	runtime.SetFinalizer(e, (*Engine).Close)
	return e, nil
}

// Close releases the device state.
func (e *Engine) Close() {
	if e.h != nil {
		C.ks_destroy(e.h)
		e.h = nil
	}
	runtime.SetFinalizer(e, nil)
}

// CommUniqueID makes the RCCL communicator id rank 0 broadcasts to the others (ks_comm_unique_id).
func CommUniqueID() ([]byte, error) {
	id := make([]byte, C.KS_COMM_ID_BYTES)
	if rc := C.ks_comm_unique_id((*C.uint8_t)(unsafe.Pointer(&id[0]))); rc != C.KS_OK {
		return nil, status(nil, rc)
	}
	return id, nil
}

// Shard makes this engine rank `rank` of `world` node-sharded engines (one per GPU, ks_shard):
// each scans its node range and the per-pod candidate lists are all-gathered over RCCL once per
// batch; every rank loads the whole cluster and submits the same pods, and all binds are
// identical.  Call before LoadNodes.
func (e *Engine) Shard(world, rank int, id []byte, vshards int) error {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	if len(id) != C.KS_COMM_ID_BYTES {
		return errors.Errorf("communicator id: %d bytes, want %d", len(id), C.KS_COMM_ID_BYTES)
	}
	rc := C.ks_shard(e.h, C.int32_t(world), C.int32_t(rank), (*C.uint8_t)(unsafe.Pointer(&id[0])), C.int32_t(vshards))
	return status(e, rc)
}

// LoadNodes loads the cluster once: alloc = n*4 {milli cpu, milli memory, milli gpu, pods}
// (-1 = key absent), taint / label = dictionary bitmasks (Dicts).
func (e *Engine) LoadNodes(alloc []int64, taint, label []uint64) error {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	n := len(taint)
	if len(alloc) != 4*n || len(label) != n {
		return strongerrors.InvalidArgument(errors.New("LoadNodes: alloc must hold 4 values per node"))
	}
	if n == 0 {
		return status(e, C.ks_load_nodes(e.h, 0, nil, nil, nil))
	}
	err := status(e, C.ks_load_nodes(e.h, C.int64_t(n), (*C.int64_t)(unsafe.Pointer(&alloc[0])),
		(*C.uint64_t)(unsafe.Pointer(&taint[0])), (*C.uint64_t)(unsafe.Pointer(&label[0]))))
	if err == nil {
		e.n = n
	}
	return err
}

// Pods is a batch of encoded pods in FIFO order (EncodePods builds it from []*v1.Pod).
type Pods struct {
	Arrival  []int64 // the tick whose Submit returned the pod
	Req      []int64 // 3 per pod, milli-units
	KeyMask  []uint8 // request keys present: 1 cpu, 2 memory, 4 gpu
	Tol, Sel []uint64
	PhaseOff []int32 // len(Arrival)+1
	PhaseSec []int32
	PhaseUse []int64 // 3 per phase
	Flags    []uint8 // KS_PODFLAG_*
	Key      []int64 // interned "namespace-name" (KeyTable)
}

func i64p(s []int64) *C.int64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int64_t)(unsafe.Pointer(&s[0]))
}
func u64p(s []uint64) *C.uint64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&s[0]))
}
func i32p(s []int32) *C.int32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&s[0]))
}
func u8p(s []uint8) *C.uint8_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&s[0]))
}

// SubmitPods appends pods to the FIFO (submit + podQueue.append, kubesim/kubesim.go:126-139).
func (e *Engine) SubmitPods(p *Pods) error {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	m := len(p.Arrival)
	if m == 0 {
		return nil
	}
	if len(p.Req) != 3*m || len(p.KeyMask) != m || len(p.Tol) != m || len(p.Sel) != m ||
		len(p.PhaseOff) != m+1 || len(p.Flags) != m || len(p.Key) != m ||
		int(p.PhaseOff[m]) > len(p.PhaseSec) || 3*int(p.PhaseOff[m]) > len(p.PhaseUse) {
		return strongerrors.InvalidArgument(errors.New("SubmitPods: inconsistent array lengths"))
	}
	return status(e, C.ks_submit_pods(e.h, C.int64_t(m), i64p(p.Arrival), i64p(p.Req), u8p(p.KeyMask),
		u64p(p.Tol), u64p(p.Sel), i32p(p.PhaseOff), i32p(p.PhaseSec), i64p(p.PhaseUse), u8p(p.Flags),
		i64p(p.Key)))
}

// Bind is one scheduling decision: FIFO index, node index, status (0 Ok, 1 OverCapacity,
// kubesim/pod/pod.go:20-27) and bind tick.
type Bind struct {
	Pod    int64
	Node   int32
	Status int32
	Tick   int64
}

// Queued is the number of submitted pods not popped yet.
func (e *Engine) Queued() int64 {
	defer runtime.KeepAlive(e)
	return int64(C.ks_queued_pods(e.h))
}

// Tick is the engine's current tick.
func (e *Engine) Tick() int64 {
	defer runtime.KeepAlive(e)
	return int64(C.ks_current_tick(e.h))
}

// TickSeconds is the simulated seconds per tick (ks_tick_seconds): the submitters' clock is
// start + Tick() * TickSeconds().
func (e *Engine) TickSeconds() int64 {
	defer runtime.KeepAlive(e)
	return int64(C.ks_tick_seconds(e.h))
}

// Step advances `ticks` ticks of Run's loop (at most one bind per tick).  Binds made before an
// aborting error (NotFound / InvalidArgument) are returned with the error.
func (e *Engine) Step(ticks int64) ([]Bind, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	cap := ticks
	if q := e.Queued(); q < cap {
		cap = q
	}
	if cap < 0 {
		cap = 0
	}
	out := make([]C.ks_bind, cap+1)
	var n C.int64_t
	rc := C.ks_step(e.h, C.int64_t(ticks), &out[0], C.int64_t(cap), &n)
	k := int64(n)
	if k > cap {
		k = cap
	}
	binds := make([]Bind, k)
	for i := range binds {
		binds[i] = Bind{int64(out[i].pod), int32(out[i].node), int32(out[i].status), int64(out[i].tick)}
	}
	return binds, status(e, rc)
}

// FilterMask is api.Filter over every node for queued pod `pod` (ks_filter): one byte per
// loaded node.
func (e *Engine) FilterMask(pod int64) ([]uint8, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	mask := make([]uint8, e.n+1)
	return mask[:e.n], status(e, C.ks_filter(e.h, C.int64_t(pod), u8p(mask)))
}

// Scores is the aggregated score of every loaded node for queued pod `pod` (-1 = no entry,
// ks_score).
func (e *Engine) Scores(pod int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	s := make([]int64, e.n+1)
	return s[:e.n], status(e, C.ks_score(e.h, C.int64_t(pod), i64p(s)))
}

// UsageAt is Σ Pod.ResourceUsage per node at tick t <= Tick() (3 per loaded node: cpu, memory,
// gpu milli).
func (e *Engine) UsageAt(t int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	u := make([]int64, 3*e.n+1)
	return u[:3*e.n], status(e, C.ks_usage_at(e.h, C.int64_t(t), i64p(u)))
}

// SeriesCols is KS_SERIES_COLS: the columns of ClusterSeries per tick (running pods, Σ requested
// cpu / memory / gpu milli, pods bound Ok so far, bound OverCapacity so far, pending pods).
const SeriesCols = 7

// RequestedAt is Node.totalResourceRequest and runningPodsNum (kubesim/node/node.go:97-118) of
// every node at tick t <= Tick(): 4 per loaded node (requested cpu, memory, gpu milli; running
// pods), ks_requested_at.
func (e *Engine) RequestedAt(t int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	r := make([]int64, 4*e.n+1)
	return r[:4*e.n], status(e, C.ks_requested_at(e.h, C.int64_t(t), i64p(r)))
}

// FilterMaskAt is FilterMask as it was when the already-bound pod `pod` was scheduled
// (ks_filter_at; the filtered node list scheduleOne logs, kubesim/kubesim.go:170,184).
func (e *Engine) FilterMaskAt(pod int64) ([]uint8, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	mask := make([]uint8, e.n+1)
	return mask[:e.n], status(e, C.ks_filter_at(e.h, C.int64_t(pod), u8p(mask)))
}

// ScoresAt is Scores as it was when the already-bound pod `pod` was scheduled (ks_score_at; the
// nodeScore map scheduleOne logs, kubesim/kubesim.go:194,205): its lowest-index maximum is the
// node the pod was bound to.
func (e *Engine) ScoresAt(pod int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	s := make([]int64, e.n+1)
	return s[:e.n], status(e, C.ks_score_at(e.h, C.int64_t(pod), i64p(s)))
}

// ClusterSeries is the cluster-wide curves for ticks tLo <= t < tHi (tHi-1 <= Tick(), at most
// 2^20 ticks): SeriesCols values per tick (ks_cluster_series).
func (e *Engine) ClusterSeries(tLo, tHi int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	n := 0
	if tHi > tLo && tHi-tLo <= 1<<20 { // (a longer window is rejected by the call: nothing to hold)
		n = int(tHi-tLo) * SeriesCols
	}
	s := make([]int64, n+1)
	return s[:n], status(e, C.ks_cluster_series(e.h, C.int64_t(tLo), C.int64_t(tHi), i64p(s)))
}

// NodePeaks is, per node and column, the maximum of RequestedAt(t) over tLo <= t < tHi (4 per
// loaded node, ks_node_peaks): how full each node got.
func (e *Engine) NodePeaks(tLo, tHi int64) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	r := make([]int64, 4*e.n+1)
	return r[:4*e.n], status(e, C.ks_node_peaks(e.h, C.int64_t(tLo), C.int64_t(tHi), i64p(r)))
}

// Headroom constants (include/ks_engine.h): the columns of HeadroomAt per shape (Σ over nodes of the
// count, nodes with a count >= 1, the largest count, its lowest node or -1, eligible nodes limited by
// cpu / memory / gpu / pods, ineligible nodes), the most shapes per call, the per-node clamp.
const (
	HeadroomCols      = 9
	HeadroomMaxShapes = 64
	HeadroomNodeMax   = 2147483647
)

// Shapes are pod templates for the headroom queries, in SubmitPods' fields and units: nothing is
// appended to the FIFO and no engine state changes.
type Shapes struct {
	Req      []int64 // 3 per shape, milli-units
	KeyMask  []uint8 // request keys present: 1 cpu, 2 memory, 4 gpu
	Tol, Sel []uint64
}

func (s *Shapes) count() (int, error) {
	k := len(s.KeyMask)
	if k < 1 || k > HeadroomMaxShapes || len(s.Req) != 3*k || len(s.Tol) != k || len(s.Sel) != k {
		return 0, strongerrors.InvalidArgument(errors.New("headroom: 1..64 shapes with consistent array lengths"))
	}
	return k, nil
}

// HeadroomAt is, per shape, how many more pods of it the cluster would take at tick t <= Tick():
// Node.CreatePod's admission test (kubesim/node/node.go:44-47) applied repeatedly on every node
// against RequestedAt(t) (ks_headroom_at).  Returns HeadroomCols values per shape and, with
// perNode, the per-node counts (Nodes() per shape).
func (e *Engine) HeadroomAt(t int64, s *Shapes, perNode bool) ([]int64, []int32, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	k, err := s.count()
	if err != nil {
		return nil, nil, err
	}
	out := make([]int64, k*HeadroomCols)
	var pn []int32
	if perNode {
		pn = make([]int32, k*e.n+1)
	}
	err = status(e, C.ks_headroom_at(e.h, C.int64_t(t), C.int32_t(k), i64p(s.Req), u8p(s.KeyMask), u64p(s.Tol),
		u64p(s.Sel), i64p(out), i32p(pn)))
	if perNode {
		pn = pn[:k*e.n]
	}
	return out, pn, err
}

// HeadroomSeries is columns 0 and 1 of HeadroomAt (Σ over nodes of the count, nodes with room) for
// every tick tLo <= t < tHi: 2 values per shape per tick (ks_headroom_series; window bounds as
// ClusterSeries, and at most 2^22 shape-ticks).
func (e *Engine) HeadroomSeries(tLo, tHi int64, s *Shapes) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	k, err := s.count()
	if err != nil {
		return nil, err
	}
	n := 0
	if tHi > tLo && int64(k)*(tHi-tLo) <= 1<<22 { // (a longer window is rejected by the call: nothing to hold)
		n = int(tHi-tLo) * k * 2
	}
	out := make([]int64, n+1)
	return out[:n], status(e, C.ks_headroom_series(e.h, C.int64_t(tLo), C.int64_t(tHi), C.int32_t(k), i64p(s.Req),
		u8p(s.KeyMask), u64p(s.Tol), u64p(s.Sel), i64p(out)))
}

// Placement preview constants (include/ks_engine.h): the most pods per PlaceAt call, the status of
// a pod no node was selected for, the words of Placements.Info.
const (
	PlaceMaxPods  = 1024
	PlaceNotFound = -1
	PlaceInfo     = 4
)

// Placement is one preview pod's outcome (ks_placement): the bind node (-1: none), the status
// (0 Ok, 1 OverCapacity, PlaceNotFound), the chosen node's aggregated score (-1: none) and the
// number of nodes with an entry in the nodeScore map at this pod's turn.
type Placement struct {
	Node, Status      int32
	Score, Candidates int64
}

// Placements is the result of PlaceAt: one Placement per pod, with after the requested state
// (4 values per node: cpu, memory, gpu in milli-units, running pods) at t plus every Ok placement,
// and Info = rounds of the device algorithm, pods placed Ok, placed OverCapacity, not found.
type Placements struct {
	Pods  []Placement
	After []int64
	Info  [PlaceInfo]int64
}

// PlaceAt is where len(shapeOf) more pods would be bound at tick t <= Tick(): scheduleOne
// (kubesim/kubesim.go:143-225) for the pods one after another on a private copy of the state at t
// (ks_place_at).  Pod j has shape shapeOf[j] of s; a nil shapeOf places one pod per shape, in
// order.  No engine state changes; a pod without a candidate is reported PlaceNotFound and the
// preview goes on.
func (e *Engine) PlaceAt(t int64, s *Shapes, shapeOf []int32, after bool) (*Placements, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	ns, err := s.count()
	if err != nil {
		return nil, err
	}
	k := ns
	if shapeOf != nil {
		k = len(shapeOf)
	}
	if k < 1 || k > PlaceMaxPods {
		return nil, strongerrors.InvalidArgument(errors.New("place: 1..1024 pods"))
	}
	r := &Placements{Pods: make([]Placement, k)}
	if after {
		r.After = make([]int64, 4*e.n+1)
	}
	err = status(e, C.ks_place_at(e.h, C.int64_t(t), C.int32_t(ns), i64p(s.Req), u8p(s.KeyMask), u64p(s.Tol),
		u64p(s.Sel), C.int32_t(k), i32p(shapeOf), (*C.ks_placement)(unsafe.Pointer(&r.Pods[0])), i64p(r.After),
		(*C.int64_t)(unsafe.Pointer(&r.Info[0]))))
	if after {
		r.After = r.After[:4*e.n]
	}
	return r, err
}

// Drain preview constants (include/ks_engine.h): the most evicted pods per DrainAt call, the words
// of Evictions.Info.
const (
	DrainMaxPods = 65536
	DrainInfo    = 6
)

// Eviction is one evicted pod's outcome (ks_eviction, 40 bytes): the pod's FIFO index, the drained
// node it ran on, and its Placement fields on the cluster without the drained nodes.
type Eviction struct {
	Pod               int64
	From, Node        int32
	Status, _         int32
	Score, Candidates int64
}

// Evictions is the result of DrainAt: one Eviction per evicted pod in FIFO order, After the
// requested state (4 values per node) at t with the drained nodes' rows zero plus every Ok
// re-placement, and Info = rounds of the device algorithm, re-placed Ok, OverCapacity, not found,
// segments, drained nodes that had no running pod.
type Evictions struct {
	Pods  []Eviction
	After []int64
	Info  [DrainInfo]int64
}

// DrainAt is where the pods running on `nodes` at tick t <= Tick() would go if those nodes left
// k.nodes (kubesim/kubesim.go:168-206 range over it): every pod running on them is evicted and
// handed in FIFO order to scheduleOne (kubesim.go:143-225) on a private copy of the state at t
// without the drained nodes (ks_drain_at).  nodes are distinct indices in [0, Nodes()).  No engine
// state changes.  It makes the sizing call itself; more than DrainMaxPods evicted pods are
// ErrOutOfDomain.
func (e *Engine) DrainAt(t int64, nodes []int32, after bool) (*Evictions, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	if len(nodes) == 0 && e.n > 0 {
		return nil, strongerrors.InvalidArgument(errors.New("drain: no nodes given"))
	}
	nd := nodes
	if len(nd) == 0 {
		nd = make([]int32, 1) // n = 0: the pointer must not be NULL, the count is 0
	}
	r := &Evictions{}
	if after {
		r.After = make([]int64, 4*e.n+1)
	}
	info := (*C.int64_t)(unsafe.Pointer(&r.Info[0]))
	var k C.int64_t
	rc := C.ks_drain_at(e.h, C.int64_t(t), C.int32_t(len(nodes)), i32p(nd), nil, 0, &k, i64p(r.After), info)
	if rc == C.KS_ERANGE && k > 0 && k <= DrainMaxPods {
		r.Pods = make([]Eviction, int(k))
		rc = C.ks_drain_at(e.h, C.int64_t(t), C.int32_t(len(nodes)), i32p(nd),
			(*C.ks_eviction)(unsafe.Pointer(&r.Pods[0])), k, &k, i64p(r.After), info)
	}
	if after {
		r.After = r.After[:4*e.n]
	}
	return r, status(e, rc)
}

// RemovableInfo is the words of Removals.Info (include/ks_engine.h, KS_REMOVABLE_INFO).
const RemovableInfo = 6

// Removal is one candidate's summary (ks_removal, 32 bytes): the pods running on it at t, the
// statuses of their re-placements with the candidate alone out of k.nodes, Removable = 1 iff every
// one was re-bound Ok (also when none runs there), and the index of its first row in Removals.Rows.
type Removal struct {
	Node, Evicted              int32
	Ok, OverCapacity, NotFound int32
	Removable                  int32
	FirstRow                   int64
}

// Removals is the result of RemovableAt: one Removal per candidate in the caller's order, Rows (when
// asked for) the candidates' Eviction rows concatenated in that order, FIFO within a candidate, and
// Info = segments, candidates resolved by the batched kernel, candidates answered through the
// single-drain path, candidates with no running pod, removable candidates, evicted pods.
type Removals struct {
	Nodes []Removal
	Rows  []Eviction
	Info  [RemovableInfo]int64
}

// RemovableAt says which of `nodes` could each be taken out on its own at tick t <= Tick(): for
// candidate c the answer of DrainAt(t, {c}) (kubesim/kubesim.go:168-206 range over k.nodes without
// c; its running pods go in FIFO order through scheduleOne, kubesim.go:143-225) — candidates are
// independent (ks_removable_at).  nodes are distinct indices in [0, Nodes()).  No engine state
// changes.  With rows it sizes the row buffer itself; more than DrainMaxPods evicted pods in all
// are ErrOutOfDomain.
func (e *Engine) RemovableAt(t int64, nodes []int32, rows bool) (*Removals, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	if len(nodes) == 0 && e.n > 0 {
		return nil, strongerrors.InvalidArgument(errors.New("removable: no nodes given"))
	}
	nd := nodes
	if len(nd) == 0 {
		nd = make([]int32, 1) // n = 0: the pointer must not be NULL, the count is 0
	}
	r := &Removals{Nodes: make([]Removal, len(nodes)+1)}
	out := (*C.ks_removal)(unsafe.Pointer(&r.Nodes[0]))
	info := (*C.int64_t)(unsafe.Pointer(&r.Info[0]))
	m := C.int32_t(len(nodes))
	var k C.int64_t
	var rc C.ks_status
	if !rows {
		rc = C.ks_removable_at(e.h, C.int64_t(t), m, i32p(nd), out, nil, 0, &k, info)
	} else {
		// a one-row buffer first: KS_ERANGE comes back with the count as soon as the gather has it
		r.Rows = make([]Eviction, 1)
		rc = C.ks_removable_at(e.h, C.int64_t(t), m, i32p(nd), out, (*C.ks_eviction)(unsafe.Pointer(&r.Rows[0])), 1, &k, info)
		if rc == C.KS_ERANGE && k > 1 && k <= DrainMaxPods {
			r.Rows = make([]Eviction, int(k))
			rc = C.ks_removable_at(e.h, C.int64_t(t), m, i32p(nd), out, (*C.ks_eviction)(unsafe.Pointer(&r.Rows[0])), k, &k, info)
		}
		if rc == C.KS_OK {
			r.Rows = r.Rows[:int(k)]
		}
	}
	r.Nodes = r.Nodes[:len(nodes)]
	return r, status(e, rc)
}

// Consolidation outcomes (include/ks_engine.h, KS_CONSOLIDATE_*) and the words of
// Consolidations.Info (KS_CONSOLIDATE_INFO).
const (
	ConsolidateBlocked     = 0
	ConsolidateRemoved     = 1
	ConsolidateDestination = 2
	ConsolidateInfo        = 6
)

// Consolidation is one candidate's answer (ks_consolidation, 32 bytes): the pods running on it at
// t, its outcome, the rows written for it (all of a removed candidate's pods, a blocked one's up to
// and including the blocking pod, none of a destination's), the blocking pod's status, and the
// index of its first row in Consolidations.Rows.
type Consolidation struct {
	Node, Evicted int32
	Outcome, Rows int32
	BlockStatus   int32
	Pad           int32
	FirstRow      int64
}

// Consolidations is the result of ConsolidateAt: one Consolidation per candidate in the caller's
// order, Evicted the pods running on all candidates, Rows (when asked for) the Eviction rows
// concatenated in that order, FIFO within a candidate, After (when asked for) [Nodes()][4] the
// final private state, and Info = rounds of the device algorithm, removed, blocked, destinations,
// candidates decided through the single path, pods moved.
type Consolidations struct {
	Nodes   []Consolidation
	Evicted int64
	Rows    []Eviction
	After   []int64
	Info    [ConsolidateInfo]int64
}

// ConsolidateAt says which of `nodes` a scale-down pass would remove at tick t <= Tick() when it
// handles them in the given order on one private state (ks_consolidate_at): a candidate that
// received a moved pod is a destination and nothing is tried; any other leaves k.nodes together
// with the nodes removed before it (kubesim/kubesim.go:168-206 range over k.nodes) and its running
// pods go in FIFO order through scheduleOne (kubesim.go:143-225) until one is not bound Ok; all Ok
// (or no pod): removed, the placements stay; otherwise blocked, and everything is as it was before
// the candidate.  nodes are distinct indices in [0, Nodes()).  No engine state changes.  With rows
// it sizes the row buffer itself; more than DrainMaxPods pods on the candidates are ErrOutOfDomain.
func (e *Engine) ConsolidateAt(t int64, nodes []int32, rows, after bool) (*Consolidations, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	if len(nodes) == 0 && e.n > 0 {
		return nil, strongerrors.InvalidArgument(errors.New("consolidate: no nodes given"))
	}
	nd := nodes
	if len(nd) == 0 {
		nd = make([]int32, 1) // n = 0: the pointer must not be NULL, the count is 0
	}
	r := &Consolidations{Nodes: make([]Consolidation, len(nodes)+1)}
	if after {
		r.After = make([]int64, 4*e.n+1)
	}
	out := (*C.ks_consolidation)(unsafe.Pointer(&r.Nodes[0]))
	info := (*C.int64_t)(unsafe.Pointer(&r.Info[0]))
	m := C.int32_t(len(nodes))
	var ev, k C.int64_t
	var rc C.ks_status
	if !rows {
		rc = C.ks_consolidate_at(e.h, C.int64_t(t), m, i32p(nd), out, nil, 0, &ev, &k, i64p(r.After), info)
	} else {
		// a one-row buffer first: KS_ERANGE comes back with the count as soon as the gather has it
		r.Rows = make([]Eviction, 1)
		rc = C.ks_consolidate_at(e.h, C.int64_t(t), m, i32p(nd), out, (*C.ks_eviction)(unsafe.Pointer(&r.Rows[0])), 1, &ev, &k, i64p(r.After), info)
		if rc == C.KS_ERANGE && ev > 1 && ev <= DrainMaxPods {
			r.Rows = make([]Eviction, int(ev))
			rc = C.ks_consolidate_at(e.h, C.int64_t(t), m, i32p(nd), out, (*C.ks_eviction)(unsafe.Pointer(&r.Rows[0])), ev, &ev, &k, i64p(r.After), info)
		}
		if rc == C.KS_OK {
			r.Rows = r.Rows[:int(k)]
		}
	}
	r.Evicted = int64(ev)
	r.Nodes = r.Nodes[:len(nodes)]
	if after {
		r.After = r.After[:4*e.n]
	}
	return r, status(e, rc)
}

// Gang admission preview constants (include/ks_engine.h): the most gangs, pods and shapes per
// GangAt call, the status of a pod no attempt reached, a gang's outcomes, the words of Gangs.Info.
const (
	GangMaxGangs  = 65536
	GangMaxPods   = 65536
	GangMaxShapes = 4096
	GangNotTried  = -2
	GangBlocked   = 0
	GangAdmitted  = 1
	GangSkipped   = 2
	GangInfo      = 6
)

// Gang is one gang's answer (ks_gang, 32 bytes): its pods (rows [First, First+Size) of Gangs.Pods),
// its outcome, the pods its attempt handled (Size when admitted, up to and including the deciding
// pod when blocked, 0 when skipped), their statuses counted, and the deciding pod's status.
type Gang struct {
	First, Size                int32
	Outcome, Tried             int32
	Ok, OverCapacity, NotFound int32
	BlockStatus                int32
}

// Gangs is the result of GangAt: one Gang per gang in the caller's order, Pods (when asked for) one
// Placement per pod at its own index (an untried pod has status GangNotTried), After (when asked
// for) [Nodes()][4] the final private state, and Info = rounds of the device algorithm, admitted,
// blocked, skipped, gangs decided through the single path, Ok pods of admitted gangs.
type Gangs struct {
	Gangs []Gang
	Pods  []Placement
	After []int64
	Info  [GangInfo]int64
}

// GangAt says which pod groups of a queue would be admitted at tick t <= Tick(), in the given order
// on one private state, and where their pods would be bound (ks_gang_at).  Pod j has shape
// shapeOf[j] of s (up to GangMaxShapes shapes); gang g is pods first[g] .. first[g+1]-1, with
// first[0] = 0 and first[len(first)-1] = len(shapeOf).  A gang's pods go through scheduleOne
// (kubesim/kubesim.go:143-225) one after another as PlaceAt would handle them; the attempt ends once
// more than size - minOk[g] of them were not bound Ok (nil minOk: all-or-nothing).  A gang with at
// least minOk[g] pods bound Ok is admitted and its placements stay for the later gangs; any other is
// blocked and everything is as it was before it; with strict every gang after the first blocked one
// is skipped.  No engine state changes.
func (e *Engine) GangAt(t int64, s *Shapes, shapeOf, first, minOk []int32, strict, rows, after bool) (*Gangs, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	ns := len(s.KeyMask)
	if ns < 1 || ns > GangMaxShapes || len(s.Req) != 3*ns || len(s.Tol) != ns || len(s.Sel) != ns {
		return nil, strongerrors.InvalidArgument(errors.New("gang: 1..4096 shapes with consistent array lengths"))
	}
	k, m := len(shapeOf), len(first)-1
	if k < 1 || k > GangMaxPods || m < 1 || m > GangMaxGangs || (minOk != nil && len(minOk) != m) {
		return nil, strongerrors.InvalidArgument(errors.New("gang: 1..65536 pods in 1..65536 gangs, one minOk per gang"))
	}
	r := &Gangs{Gangs: make([]Gang, m)}
	var pods *C.ks_placement
	if rows {
		r.Pods = make([]Placement, k)
		pods = (*C.ks_placement)(unsafe.Pointer(&r.Pods[0]))
	}
	if after {
		r.After = make([]int64, 4*e.n+1)
	}
	var flags C.uint32_t
	if strict {
		flags = C.KS_GANG_STRICT
	}
	err := status(e, C.ks_gang_at(e.h, C.int64_t(t), C.int32_t(ns), i64p(s.Req), u8p(s.KeyMask), u64p(s.Tol), u64p(s.Sel),
		C.int32_t(k), i32p(shapeOf), C.int32_t(m), i32p(first), i32p(minOk), flags,
		(*C.ks_gang)(unsafe.Pointer(&r.Gangs[0])), pods, i64p(r.After), (*C.int64_t)(unsafe.Pointer(&r.Info[0]))))
	if after {
		r.After = r.After[:4*e.n]
	}
	return r, err
}

// Scale-up preview constants (include/ks_engine.h): the most options per ScaleUpAt call, the most
// nodes an option may append, the words of ScaleUps.Info.
const (
	ScaleUpMaxOptions = 64
	ScaleUpMaxNodes   = 65536
	ScaleUpInfo       = 4
)

// ScaleOption is one node-group template (ks_scale_option, 56 bytes): Alloc as LoadNodes takes it
// (cpu, memory, nvidia.com/gpu in milli-units, -1 absent, pods), the taint and label dictionary bits,
// and how many copies may be appended.
type ScaleOption struct {
	Alloc        [4]int64
	Taint, Label uint64
	MaxNodes, _  int32
}

// ScaleResult is one option's summary (ks_scale_result, 32 bytes): the statuses of the k pods, the
// pods bound Ok to an appended node, the appended nodes holding a pod, the first pod that was not
// bound Ok (-1: none) and Path: 0 the batched kernel decided it, 1 the single path.
type ScaleResult struct {
	Ok, OverCapacity, NotFound int32
	OnNew, NodesUsed           int32
	FirstUnplaced, Path, _     int32
}

// ScaleUps is the result of ScaleUpAt: one ScaleResult per option, Rows (when asked for) the
// options' Placement rows, option g's at Rows[g*k : (g+1)*k], and Info = options decided by the
// batched kernel, options answered through the single path, options in which every pod was bound
// Ok, distinct shapes.
type ScaleUps struct {
	Options []ScaleResult
	Rows    []Placement
	Info    [ScaleUpInfo]int64
}

// ScaleUpAt is where len(shapeOf) pending pods would be bound at tick t <= Tick() if up to
// MaxNodes empty nodes of a template were appended to k.nodes (kubesim/kubesim.go:168-206 range
// over it) at indices Nodes() .. Nodes()+MaxNodes-1, for each option on its own: by definition
// PlaceAt on that extended cluster (ks_scale_up_at).  A Placement's Node >= Nodes() names appended
// node Node-Nodes().  Options are independent; no engine state changes.
func (e *Engine) ScaleUpAt(t int64, s *Shapes, shapeOf []int32, options []ScaleOption, rows bool) (*ScaleUps, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	ns, err := s.count()
	if err != nil {
		return nil, err
	}
	k := ns
	if shapeOf != nil {
		k = len(shapeOf)
	}
	if k < 1 || k > PlaceMaxPods {
		return nil, strongerrors.InvalidArgument(errors.New("scale_up: 1..1024 pods"))
	}
	if len(options) < 1 || len(options) > ScaleUpMaxOptions {
		return nil, strongerrors.InvalidArgument(errors.New("scale_up: 1..64 options"))
	}
	r := &ScaleUps{Options: make([]ScaleResult, len(options))}
	var rp *C.ks_placement
	if rows {
		r.Rows = make([]Placement, len(options)*k)
		rp = (*C.ks_placement)(unsafe.Pointer(&r.Rows[0]))
	}
	err = status(e, C.ks_scale_up_at(e.h, C.int64_t(t), C.int32_t(ns), i64p(s.Req), u8p(s.KeyMask), u64p(s.Tol),
		u64p(s.Sel), C.int32_t(k), i32p(shapeOf), C.int32_t(len(options)),
		(*C.ks_scale_option)(unsafe.Pointer(&options[0])), (*C.ks_scale_result)(unsafe.Pointer(&r.Options[0])), rp,
		(*C.int64_t)(unsafe.Pointer(&r.Info[0]))))
	return r, err
}

// Nodes is the node count of LoadNodes.
func (e *Engine) Nodes() int { return e.n }

// PodLookup is Node.GetPod by key (kubesim/node/node.go:62-75): the FIFO index stored there.
func (e *Engine) PodLookup(node int32, key int64) (int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	var q C.int64_t
	err := status(e, C.ks_pod_lookup(e.h, C.int32_t(node), C.int64_t(key), &q))
	return int64(q), err
}

// NodePods is Node.GetPodList (kubesim/node/node.go:77-82): FIFO indices, one per key.
func (e *Engine) NodePods(node int32) ([]int64, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	var n C.int64_t
	if err := status(e, C.ks_node_pods(e.h, C.int32_t(node), nil, 0, &n)); err != nil {
		return nil, err
	}
	out := make([]int64, int(n)+1)
	err := status(e, C.ks_node_pods(e.h, C.int32_t(node), i64p(out), n, &n))
	return out[:int(n)], err
}

// PodPhase values of ks_pod_info.
const (
	PhasePending   = C.KS_PHASE_PENDING
	PhaseRunning   = C.KS_PHASE_RUNNING
	PhaseSucceeded = C.KS_PHASE_SUCCEEDED
	PhaseFailed    = C.KS_PHASE_FAILED
)

// PodInfo is Pod.BuildStatus's data (kubesim/pod/pod.go:78-167) at the current tick.
type PodInfo struct {
	Phase        int32
	Node         int32
	StartTick    int64
	TotalSeconds int32
}

// PodStatus returns the status of FIFO pods [lo, lo+n).
func (e *Engine) PodStatus(lo, n int64) ([]PodInfo, error) {
	defer runtime.KeepAlive(e) // e.h must outlive the C call (the finalizer runs ks_destroy)
	out := make([]C.ks_pod_info, n+1)
	if err := status(e, C.ks_pod_status(e.h, C.int64_t(lo), C.int64_t(n), &out[0])); err != nil {
		return nil, err
	}
	r := make([]PodInfo, n)
	for i := range r {
		r[i] = PodInfo{int32(out[i].phase), int32(out[i].node), int64(out[i].start_tick), int32(out[i].total_seconds)}
	}
	return r, nil
}

// Device self-tests of ks_selftest (include/ks_engine.h): no engine needed, a deployment can run
// them once at start-up.
const (
	SelftestLRMicro     = int32(C.KS_SELFTEST_LR_MICRO)     // the micro evaluator's LeastRequested floor, every (x, A)
	SelftestMicroStates = int32(C.KS_SELFTEST_MICRO_STATES) // the micro evaluator and its scan form, every usage of 13 capacity pairs
	SelftestListMerge   = int32(C.KS_SELFTEST_LIST_MERGE)   // merge_cl's score-class list merge against the host fold
)

// Selftest runs one device self-test and returns the number of mismatching cases (0 = pass).
func Selftest(device int, test int32) (int64, error) {
	var n C.int64_t
	if err := status(nil, C.ks_selftest(C.int32_t(device), C.int32_t(test), &n)); err != nil {
		return -1, err
	}
	return int64(n), nil
}

// EvalConfig is the ks_eval_cfg of SelftestEval: the filter and scorer configuration in the
// engine's summed form.
type EvalConfig struct {
	FeedsScore         bool
	Filters            uint32
	HasScorers         bool
	WeightLR, WeightBA int32
	ConstTotal         int32
}

// Column counts and bits of SelftestEval (include/ks_engine.h).
const (
	EvalTotalCols = int(C.KS_EVAL_TOTAL_COLS)
	EvalPruneCols = int(C.KS_EVAL_PRUNE_COLS)
	EvalScanMicro = uint(C.KS_EVAL_SCAN_MICRO)
	EvalPruneBit  = uint(C.KS_EVAL_PRUNE_BIT)
)

// SelftestEval runs n (node, pod) cases through the device evaluators (ks_selftest_eval,
// diagnostics): alloc and run hold 4 values per case, req 3, masks 4 (taint, label, tolerations,
// selector), keymask 1.  It returns total1 (EvalTotalCols columns of n), tmax and live
// (EvalPruneCols columns of n); only the columns whose bit `variants` sets are filled.  A batch
// outside a requested evaluator's domain is InvalidArgument.
func SelftestEval(device int, c EvalConfig, alloc, run, req []int64, keymask []uint32, masks []uint64,
	variants uint32) (total1, tmax, live []uint32, err error) {
	n := len(keymask)
	if n == 0 || len(alloc) != 4*n || len(run) != 4*n || len(req) != 3*n || len(masks) != 4*n {
		return nil, nil, nil, strongerrors.InvalidArgument(errors.New("SelftestEval: slice lengths"))
	}
	b := func(v bool) C.int32_t {
		if v {
			return 1
		}
		return 0
	}
	cc := C.ks_eval_cfg{filter_feeds: b(c.FeedsScore), filters: C.uint32_t(c.Filters), has_scorers: b(c.HasScorers),
		w_lr: C.int32_t(c.WeightLR), w_ba: C.int32_t(c.WeightBA), const_total: C.int32_t(c.ConstTotal)}
	total1 = make([]uint32, EvalTotalCols*n)
	tmax = make([]uint32, EvalPruneCols*n)
	live = make([]uint32, EvalPruneCols*n)
	u32p := func(s []uint32) *C.uint32_t { return (*C.uint32_t)(unsafe.Pointer(&s[0])) }
	rc := C.ks_selftest_eval(C.int32_t(device), &cc, C.int64_t(n), i64p(alloc), i64p(run), i64p(req),
		u32p(keymask), u64p(masks), C.uint32_t(variants), u32p(total1), u32p(tmax), u32p(live))
	if err = status(nil, rc); err != nil {
		return nil, nil, nil, err
	}
	return total1, tmax, live, nil
}
