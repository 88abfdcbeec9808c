// Package servicegraph puts the MI355X ServiceGraph engine (include/servicegraph.h, libservicegraph.so) behind Alaz's own
// plugin interface, datastore.DataStore (datastore/datastore.go:3-20).  GraphDS DECORATES the data store the agent already
// has: every call is forwarded to it unchanged, and the edge-relevant fields are also fed to the GPU engine, which emits one
// scored row per EDGE per window.  It is injected where the reference injects its BackendDS — the last argument of
// aggregator.NewAggregator (aggregator/data.go:135-140, main.go:103):
//
//	dsBackend := datastore.NewBackendDS(ctx, config.BackendDSConfig{...})          // main.go:82-93, unchanged
//	gds, err := servicegraph.New(dsBackend, servicegraph.Config{MaxKnownNodes: 1 << 16, MaxEdges: 1 << 21, Layers: 2})
//	var ds datastore.DataStore = dsBackend
//	if err == nil { ds = gds; go gds.Run(ctx, time.Second, onEdges) }            // no GPU: the CPU path stays as it is
//	a := aggregator.NewAggregator(ctx, ct, kubeEvents, ec.EbpfEvents(), ec.EbpfProcEvents(), ec.EbpfTcpEvents(), ec.TlsAttachQueue(), ds)
//
// The C++ mirror of this file, alaz_amd/csrc/host/graph_ds.{hpp,cpp}, is what the repository's tests drive (no Go toolchain
// exists in its build environment: this file is written against the reference's sources, not compiled there).  Behaviour
// that must match it: one node id per live UID, reference-counted by the IPs bound to it and recycled only after the next
// FlushWindow; DELETE never creates an id; ReverseDirection() is undone before the event is handed over (K1 re-applies it
// after its own join); the engine is never allowed to block the aggregator (sg_ingest drops and counts on a full ring).
package servicegraph

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../alaz_amd/lib -lservicegraph
#include <stdlib.h>
#include <string.h>
#include "servicegraph.h"
*/
import "C"

import (
	"context"
	"fmt"
	"net"
	"strings"
	"sync"
	"sync/atomic"
	"time"
	"unsafe"

	"github.com/ddosify/alaz/datastore"
	"github.com/ddosify/alaz/ebpf/l7_req"
)

// Config is the subset of sg_config a deployment chooses; everything else keeps the engine's default.
type Config struct {
	Device          int
	MaxKnownNodes   uint32 // live pods + services
	MaxLabels       uint32 // distinct Host-header names of outbound destinations
	MaxOutboundIPs  uint32 // distinct raw-IP outbound destinations per window
	MaxEdges        uint64 // distinct edges per window
	MaxWindowEvents uint64 // most events one window may carry (sizes the K1 record slabs)
	Layers          uint32 // GraphSAGE layers, 1..4
	EdgeHistogram   bool   // p50 / p99 per edge (SG_CFG_EDGE_HISTOGRAM)
	Divert          bool   // true: PersistRequest / PersistKafkaEvent are NOT forwarded to the inner store (edge rows replace them)
	Weights         []float32
}

// EdgeRow is one scored edge of a closed window (sg_edge_out with the refs resolved to the reference's (Type, UID) pairs).
type EdgeRow struct {
	FromType, FromUID, ToType, ToUID string
	Count, ErrCount                  uint32
	SumNs, MaxNs, SumSqUs            uint64
	Score, LatZ, ErrRatio            float32
	Alive, P50Us, P99Us              uint32
}

const (
	kindPod     = uint8(C.SG_NODE_POD)
	kindService = uint8(C.SG_NODE_SERVICE)
	noID        = ^uint32(0)
	nShards     = 8
	batchCap    = 4096 // events per cgo call: a call costs 50-100 ns, sg_ingest copies the batch
)

type shard struct {
	mu    sync.Mutex
	batch []C.sg_event
}

// GraphDS implements datastore.DataStore.
type GraphDS struct {
	inner  datastore.DataStore
	h      C.sg_handle
	divert bool

	idMu    sync.Mutex
	ids     map[string]uint32 // UID -> node id
	uidOf   []string
	kindOf  []uint8
	refs    []uint32          // IPs bound to the id
	freeIDs []uint32
	retired []uint32          // ids whose last IP went away since the last FlushWindow
	podIP   map[uint32]uint32 // ip -> id: what sg_upsert_pod / sg_delete_pod were told
	svcIP   map[uint32]uint32
	maxKnown uint32

	lblMu  sync.RWMutex
	labels map[string]uint32 // Host header -> label id (>= 1), cumulative
	names  []string

	shards  [nShards]shard
	next    atomic.Uint32
	flushMu sync.Mutex
	nQ      int // quantiles per entity and side, as SetQuantiles set them last (K20; guarded by flushMu)

	// (flushMu) the workload baseline's capacity and the rows its vanished list holds, as the engine resolves a 0
	wlEntries uint64
	wlVanRows int

	// the service binding (idMu): the groups AssignGroups was told, the Services by "namespace/name", the pods behind each, and back
	bindOn    bool
	nodeGroup map[uint32]uint32
	svcUID    map[string]string
	epPods    map[string][]string
	podEps    map[string][]string

	maxEdges int     // sg_config.max_edges
	selOn    bool    // SetSelection (under flushMu): FlushWindow returns the selected rows only
	selK     uint32
	selMin   float32

	EngineErrors   atomic.Uint64 // SG_ENOSPC and friends from the engine (the inner store still got the call)
	BatchesDropped atomic.Uint64 // SG_EAGAIN: staging ring full, batch dropped and counted by the engine
	// Filter, when set, is asked before an event of the early tap (IngestL7) is packed: the aggregator's own
	// parsePostgresCommand / parseMySQLCommand / parseMongoEvent results (aggregator/data.go:1251-1362) — false drops the event.
	Filter func(*l7_req.L7Event) bool
}

var _ datastore.DataStore = (*GraphDS)(nil)

func ip4(s string) (uint32, bool) {
	p := net.ParseIP(s).To4()
	if p == nil {
		return 0, false
	}
	return uint32(p[0])<<24 | uint32(p[1])<<16 | uint32(p[2])<<8 | uint32(p[3]), true
}

func ipString(ip uint32) string { // aggregator/data.go:1751-1758 IntToIPv4
	return fmt.Sprintf("%d.%d.%d.%d", ip>>24, (ip>>16)&255, (ip>>8)&255, ip&255)
}

// New creates the engine.  It fails when no usable MI355X is present: there is no CPU fallback, the caller keeps `inner`.
func New(inner datastore.DataStore, c Config) (*GraphDS, error) {
	if uint32(C.sg_abi_version()) != uint32(C.SG_ABI_VERSION) {
		return nil, fmt.Errorf("servicegraph: library ABI %d, header ABI %d", uint32(C.sg_abi_version()), uint32(C.SG_ABI_VERSION))
	}
	var cfg C.sg_config
	C.memset(unsafe.Pointer(&cfg), 0, C.size_t(unsafe.Sizeof(cfg)))
	cfg.struct_size = C.uint32_t(unsafe.Sizeof(cfg))
	cfg.abi_version = C.SG_ABI_VERSION
	cfg.device = C.int32_t(c.Device)
	cfg.max_known_nodes = C.uint32_t(c.MaxKnownNodes)
	cfg.max_labels = C.uint32_t(c.MaxLabels)
	cfg.max_outbound_ips = C.uint32_t(c.MaxOutboundIPs)
	cfg.max_ips = C.uint32_t(c.MaxKnownNodes)
	cfg.max_edges = C.uint64_t(c.MaxEdges)
	cfg.max_batch = C.uint32_t(batchCap)
	cfg.max_window_events = C.uint64_t(c.MaxWindowEvents)
	cfg.layers = C.uint32_t(c.Layers)
	cfg.world = 1
	cfg.windows_in_flight = 1
	if c.EdgeHistogram {
		cfg.flags |= C.SG_CFG_EDGE_HISTOGRAM
	}
	g := &GraphDS{inner: inner, divert: c.Divert, ids: map[string]uint32{}, podIP: map[uint32]uint32{}, svcIP: map[uint32]uint32{},
		labels: map[string]uint32{}, maxKnown: c.MaxKnownNodes, maxEdges: int(c.MaxEdges),
		nodeGroup: map[uint32]uint32{}, svcUID: map[string]string{}, epPods: map[string][]string{}, podEps: map[string][]string{}}
	if rc := C.sg_create(&cfg, &g.h); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_create = %d (no usable gfx950 device, or bad config)", int(rc))
	}
	if n := int(C.sg_weights_count(C.uint32_t(c.Layers))); len(c.Weights) == n {
		C.sg_load_weights(g.h, (*C.float)(unsafe.Pointer(&c.Weights[0])), C.size_t(n))
	} else if len(c.Weights) != 0 {
		C.sg_destroy(g.h)
		return nil, fmt.Errorf("servicegraph: %d weights given, the %d-layer model has %d", len(c.Weights), c.Layers, n)
	}
	return g, nil
}

// Close flushes nothing and frees the engine; no call may be in flight.
func (g *GraphDS) Close() { C.sg_destroy(g.h) }

// Stats: what the engine dropped or waited for since New (sg_stats, ABI 6).  DroppedRing are batches the staging ring had no room
// for (sg_ingest never blocks: the reference's PersistRequest would, datastore/backend.go:844); IngestWaits the sg_ingest calls that
// met a window boundary being marked and waited for it — the only wait the library ever imposes on an aggregator goroutine.
// WindowsWarm / WindowsCold: of the windows FlushWindow has read, how many were closed out of the kept edge set and how many were
// rebuilt (a service map whose edges hardly change should settle on warm; both stay 0 for an engine that keeps no state).
// WindowsDelta: of WindowsWarm, the windows that met edges the kept set lacked and merged them in (new edges cost a warm window a
// little more, not a rebuild).  WindowsPlain: windows closed without touching the kept state at all (the engine's back-off after
// repeated fall-backs, streams of raw outbound IPs) — counted in neither WindowsWarm nor WindowsCold, so the two need not add up to
// Windows.
type Stats struct {
	EventsIn, DroppedSrc, DroppedRing, DroppedCap, Windows, IngestWaits, WindowsWarm, WindowsCold, WindowsDelta, WindowsPlain uint64
}

func (g *GraphDS) Stats() Stats {
	var st C.sg_stats
	C.sg_stats_get(g.h, &st)
	return Stats{EventsIn: uint64(st.events_in), DroppedSrc: uint64(st.events_dropped_src), DroppedRing: uint64(st.events_dropped_ring),
		DroppedCap: uint64(st.events_dropped_cap), Windows: uint64(st.windows), IngestWaits: uint64(st.ingest_waits),
		WindowsWarm: uint64(st.windows_warm), WindowsCold: uint64(st.windows_cold),
		WindowsDelta: uint64(st.windows_delta), WindowsPlain: uint64(st.windows_plain)}
}

// SetClock hands over FirstKernelTime / FirstUserspaceTime (ebpf/l7_req/l7.go:707-710) for the early tap's StartTime.
func (g *GraphDS) SetClock(firstKernelNs, firstUserNs uint64) {
	C.sg_set_clock(g.h, C.uint64_t(firstKernelNs), C.uint64_t(firstUserNs))
}

// ---- node ids (idMu held) --------------------------------------------------------------------------------------------

func (g *GraphDS) intern(uid string, kind uint8) uint32 {
	if id, ok := g.ids[uid]; ok {
		g.kindOf[id] = kind
		return id
	}
	var id uint32
	if n := len(g.freeIDs); n > 0 {
		id = g.freeIDs[n-1]
		g.freeIDs = g.freeIDs[:n-1]
		g.uidOf[id], g.kindOf[id], g.refs[id] = uid, kind, 0
	} else {
		if uint32(len(g.uidOf)) >= g.maxKnown {
			return noID // the engine's id space is full (sg_config.max_known_nodes bounds the LIVE pods + services)
		}
		id = uint32(len(g.uidOf))
		g.uidOf, g.kindOf, g.refs = append(g.uidOf, uid), append(g.kindOf, kind), append(g.refs, 0)
	}
	g.ids[uid] = id
	return id
}

func (g *GraphDS) bind(m map[uint32]uint32, ip, id uint32) {
	old, had := m[ip]
	if had && old == id {
		return
	}
	g.refs[id]++ // before the unbind: re-binding an id's only IP must not retire it
	m[ip] = id
	if had {
		if g.refs[old]--; g.refs[old] == 0 {
			g.retired = append(g.retired, old)
		}
	}
}

func (g *GraphDS) unbind(m map[uint32]uint32, ip uint32) {
	id, ok := m[ip]
	if !ok {
		return
	}
	delete(m, ip)
	if g.refs[id]--; g.refs[id] == 0 {
		g.retired = append(g.retired, id) // the open window may still name it: recycled after the next FlushWindow
	}
}

// ---- k8s resources: PodIPToPodUid / ServiceIPToServiceUid (aggregator/persist.go:55-71, 114-130) ------------------------

func (g *GraphDS) upsertOrDelete(svc bool, uid, ipStr, eventType string) {
	ip, ok := ip4(ipStr)
	if !ok {
		return // pods without an IP never reach the data store (persist.go:37-40); not IPv4: nothing the join could do
	}
	g.idMu.Lock()
	defer g.idMu.Unlock()
	m, kind := g.podIP, kindPod
	if svc {
		m, kind = g.svcIP, kindService
	}
	switch eventType {
	case "ADD", "UPDATE":
		id := g.intern(uid, kind)
		if id == noID {
			g.EngineErrors.Add(1)
			return
		}
		var rc C.int
		if svc {
			rc = C.sg_upsert_service(g.h, C.uint32_t(ip), C.uint32_t(id))
		} else {
			rc = C.sg_upsert_pod(g.h, C.uint32_t(ip), C.uint32_t(id))
		}
		if rc != 0 {
			g.EngineErrors.Add(1)
			return
		}
		g.bind(m, ip, id)
	case "DELETE": // never creates an id
		if svc {
			C.sg_delete_service(g.h, C.uint32_t(ip))
		} else {
			C.sg_delete_pod(g.h, C.uint32_t(ip))
		}
		g.unbind(m, ip)
	}
}

func (g *GraphDS) PersistPod(pod datastore.Pod, eventType string) error {
	g.upsertOrDelete(false, pod.UID, pod.IP, eventType)
	g.idMu.Lock()
	g.bindServicesOfPod(pod.UID) // a pod added or removed: the Services it stands behind
	g.idMu.Unlock()
	return g.inner.PersistPod(pod, eventType)
}

// The aggregator keys its table on Spec.ClusterIP (persist.go:117), which the DTO carries as ClusterIPs[0]
// (ClusterIP itself is never filled in, persist.go:105-112).
func (g *GraphDS) PersistService(service datastore.Service, eventType string) error {
	ip := service.ClusterIP
	if len(service.ClusterIPs) > 0 {
		ip = service.ClusterIPs[0]
	}
	if service.Name != "" && eventType == "DELETE" { // forget the entry: a bound Service leaves its group first
		key := service.Namespace + "/" + service.Name
		g.idMu.Lock()
		if uid, ok := g.svcUID[key]; ok {
			if id, ok := g.ids[uid]; ok {
				g.assignLocked(id, NoGroup)
			}
			delete(g.svcUID, key)
		}
		g.idMu.Unlock()
	}
	g.upsertOrDelete(true, service.UID, ip, eventType)
	if service.Name != "" && (eventType == "ADD" || eventType == "UPDATE") {
		key := service.Namespace + "/" + service.Name
		g.idMu.Lock()
		g.svcUID[key] = service.UID
		g.bindService(key)
		g.idMu.Unlock()
	}
	return g.inner.PersistService(service, eventType)
}

// ---- the service binding (idMu held) -----------------------------------------------------------------------------------

// assignLocked sends one sg_group_assign when the engine does not hold the value already.
func (g *GraphDS) assignLocked(id, group uint32) {
	cur, ok := g.nodeGroup[id]
	if !ok {
		cur = NoGroup
	}
	if cur == group {
		return
	}
	cid, cg := C.uint32_t(id), C.uint32_t(group)
	if rc := C.sg_group_assign(g.h, &cid, &cg, 1); rc != 0 {
		g.EngineErrors.Add(1)
		return
	}
	if group == NoGroup {
		delete(g.nodeGroup, id)
	} else {
		g.nodeGroup[id] = group
	}
}

// bindService applies the rule to the Service at key: group g iff its Endpoints name at least one pod that has an IP here and
// every such pod is in g; otherwise none.
func (g *GraphDS) bindService(key string) {
	uid, ok := g.svcUID[key]
	if !ok {
		return
	}
	sid, ok := g.ids[uid]
	if !ok || g.kindOf[sid] != kindService {
		return
	}
	group, some, one := NoGroup, false, true
	if g.bindOn {
		for _, pod := range g.epPods[key] {
			pid, ok := g.ids[pod]
			if !ok || g.kindOf[pid] != kindPod || g.refs[pid] == 0 {
				continue // a pod the store does not know
			}
			pg, ok := g.nodeGroup[pid]
			if !ok || (some && pg != group) {
				one = false // an ungrouped pod among them, or two workloads behind it
			}
			group, some = pg, true
		}
	}
	if !some || !one {
		group = NoGroup
	}
	g.assignLocked(sid, group)
}

func (g *GraphDS) bindServicesOfPod(podUID string) {
	for _, key := range g.podEps[podUID] {
		g.bindService(key)
	}
}

func (g *GraphDS) bindAllServices() {
	for key := range g.svcUID {
		g.bindService(key)
	}
}

// SetServiceBinding switches the service binding on or off (off by default; behind SetGroups).  With it on, a Service's node id
// joins the group of the pods behind it, so that pod -> ClusterIP traffic contracts to workload -> workload and call chains run
// through Services: (namespace, name) -> Service comes from PersistService, (namespace, name) -> pod UIDs from PersistEndpoints
// (addresses of Type "Pod" with an ID), the pods' groups from AssignGroups.  A Service is in group g iff its Endpoints name at
// least one pod that has an IP here and every such pod is in g; no Endpoints, no known pod, an ungrouped pod among them or two
// workloads behind it leave it in none.  Every change of an input re-evaluates it, and one sg_group_assign is sent only when the
// value changes.  Off un-assigns every bound Service.
func (g *GraphDS) SetServiceBinding(on bool) {
	g.idMu.Lock()
	g.bindOn = on
	g.bindAllServices()
	g.idMu.Unlock()
}

func (g *GraphDS) PersistReplicaSet(rs datastore.ReplicaSet, eventType string) error { return g.inner.PersistReplicaSet(rs, eventType) }
func (g *GraphDS) PersistDeployment(d datastore.Deployment, eventType string) error  { return g.inner.PersistDeployment(d, eventType) }

// PersistEndpoints is forwarded unchanged; the pods behind (namespace, name) are remembered for SetServiceBinding (the addresses
// whose Type is "Pod" with a non-empty ID: TargetRef's, aggregator/persist.go:247-267).  DELETE forgets the entry.
func (g *GraphDS) PersistEndpoints(e datastore.Endpoints, eventType string) error {
	if eventType == "ADD" || eventType == "UPDATE" || eventType == "DELETE" {
		key := e.Namespace + "/" + e.Name
		g.idMu.Lock()
		for _, pod := range g.epPods[key] {
			keys := g.podEps[pod][:0]
			for _, k := range g.podEps[pod] {
				if k != key {
					keys = append(keys, k)
				}
			}
			if len(keys) == 0 {
				delete(g.podEps, pod)
			} else {
				g.podEps[pod] = keys
			}
		}
		delete(g.epPods, key)
		if eventType != "DELETE" {
			seen := map[string]bool{}
			var pods []string
			for _, a := range e.Addresses {
				for _, ip := range a.IPs {
					if ip.Type == "Pod" && ip.ID != "" && !seen[ip.ID] {
						seen[ip.ID] = true
						pods = append(pods, ip.ID)
					}
				}
			}
			g.epPods[key] = pods
			for _, pod := range pods {
				g.podEps[pod] = append(g.podEps[pod], key)
			}
		}
		g.bindService(key)
		g.idMu.Unlock()
	}
	return g.inner.PersistEndpoints(e, eventType)
}
func (g *GraphDS) PersistContainer(c datastore.Container, eventType string) error    { return g.inner.PersistContainer(c, eventType) }
func (g *GraphDS) PersistDaemonSet(ds datastore.DaemonSet, eventType string) error   { return g.inner.PersistDaemonSet(ds, eventType) }
func (g *GraphDS) PersistStatefulSet(ss datastore.StatefulSet, eventType string) error {
	return g.inner.PersistStatefulSet(ss, eventType)
}

// ---- events ----------------------------------------------------------------------------------------------------------

func (g *GraphDS) label(name string) uint32 {
	g.lblMu.RLock()
	id, ok := g.labels[name]
	g.lblMu.RUnlock()
	if ok {
		return id
	}
	g.lblMu.Lock()
	defer g.lblMu.Unlock()
	if id, ok = g.labels[name]; ok {
		return id
	}
	g.names = append(g.names, name)
	id = uint32(len(g.names)) // ids start at 1: 0 = no Host header
	g.labels[name] = id
	return id
}

func (g *GraphDS) knownIP(ip uint32) bool {
	g.idMu.Lock()
	_, p := g.podIP[ip]
	_, s := g.svcIP[ip]
	g.idMu.Unlock()
	return p || s
}

func protoID(p string) (C.uint8_t, bool) { // (id, tls implied by the "HTTPS" rewrite of aggregator/data.go:1240-1242)
	switch p {
	case l7_req.L7_PROTOCOL_HTTP:
		return C.SG_PROTO_HTTP, false
	case "HTTPS":
		return C.SG_PROTO_HTTP, true
	case l7_req.L7_PROTOCOL_AMQP:
		return C.SG_PROTO_AMQP, false
	case l7_req.L7_PROTOCOL_POSTGRES:
		return C.SG_PROTO_POSTGRES, false
	case l7_req.L7_PROTOCOL_HTTP2:
		return C.SG_PROTO_HTTP2, false
	case l7_req.L7_PROTOCOL_REDIS:
		return C.SG_PROTO_REDIS, false
	case l7_req.L7_PROTOCOL_KAFKA:
		return C.SG_PROTO_KAFKA, false
	case l7_req.L7_PROTOCOL_MYSQL:
		return C.SG_PROTO_MYSQL, false
	case l7_req.L7_PROTOCOL_MONGO:
		return C.SG_PROTO_MONGO, false
	}
	return C.SG_PROTO_UNKNOWN, false
}

func clamp16(v uint32) C.uint16_t {
	if v > 0xFFFF {
		v = 0xFFFF
	}
	return C.uint16_t(v)
}

// hostHeader is parseHttpPayload's Host rule (aggregator/data.go:508-531): the second space-separated field of the first
// line after the request line that starts with "Host:", '\r' trimmed.
func hostHeader(payload string) string {
	lines := strings.Split(payload, "\n")
	for _, line := range lines[1:] {
		if strings.HasPrefix(line, "Host:") {
			if parts := strings.Split(line, " "); len(parts) >= 2 {
				return strings.TrimSuffix(parts[1], "\r")
			}
		}
	}
	return ""
}

// add appends packed events to one of eight batches (goroutines on different Ps rarely meet) and hands a full batch to the
// engine.  sg_ingest copies and never blocks: a full staging ring drops the batch and counts it (the reference's
// PersistRequest would block there, datastore/backend.go:844).
func (g *GraphDS) add(ev C.sg_event, copies int) {
	s := &g.shards[g.next.Add(1)%nShards]
	s.mu.Lock()
	for i := 0; i < copies; i++ {
		s.batch = append(s.batch, ev)
		if len(s.batch) >= batchCap {
			g.flushShard(s)
		}
	}
	s.mu.Unlock()
}

func (g *GraphDS) flushShard(s *shard) { // s.mu held
	if len(s.batch) == 0 {
		return
	}
	switch rc := C.sg_ingest(g.h, (*C.sg_event)(unsafe.Pointer(&s.batch[0])), C.size_t(len(s.batch))); rc {
	case 0:
	case C.SG_EAGAIN:
		g.BatchesDropped.Add(1)
	default:
		g.EngineErrors.Add(1)
	}
	s.batch = s.batch[:0]
}

// PersistRequest is the data-store-boundary tap: the aggregator already ran setFromToV2 (aggregator/data.go:827-870); the
// engine repeats the join on the GPU from the two IPs.  The DTO is only read during the call.
func (g *GraphDS) PersistRequest(request *datastore.Request) error {
	if request == nil {
		return nil
	}
	r := request
	var ev C.sg_event
	proto, tls := protoID(r.Protocol)
	ev.protocol = proto
	// ReverseDirection() was applied for AMQP DELIVER / Redis PUSHED_EVENT (data.go:1110-1112, 1151-1153): undone here
	rev := (proto == C.SG_PROTO_AMQP && r.Method == l7_req.DELIVER) || (proto == C.SG_PROTO_REDIS && r.Method == l7_req.REDIS_PUSHED_EVENT)
	sip, dip, dtype, duid := r.FromIP, r.ToIP, r.ToType, r.ToUID
	if rev {
		sip, dip, dtype, duid = r.ToIP, r.FromIP, r.FromType, r.FromUID
	}
	s, ok1 := ip4(sip)
	d, ok2 := ip4(dip)
	if ok1 && ok2 {
		ev.saddr, ev.daddr = C.uint32_t(s), C.uint32_t(d)
		ev.status = clamp16(r.StatusCode)
		if tls || r.Tls {
			ev.flags |= C.SG_EV_TLS
		}
		if rev {
			ev.flags |= C.SG_EV_REVERSE
		}
		ev.duration_ns = C.uint64_t(r.Latency)
		ev.write_time_ns = C.uint64_t(uint64(r.StartTime) * 1000000) // already wall-clock ms: the engine clock stays (0, 0) for this tap
		if dtype == "outbound" && duid != dip {                      // named by Host header or reverse DNS (data.go:851-861): a label
			ev.host_label = C.uint32_t(g.label(duid))
		}
		g.add(ev, 1)
	}
	if g.divert {
		return nil
	}
	return g.inner.PersistRequest(request)
}

func (g *GraphDS) PersistKafkaEvent(request *datastore.KafkaEvent) error {
	if request == nil {
		return nil
	}
	k := request
	s, ok1 := ip4(k.FromIP)
	d, ok2 := ip4(k.ToIP)
	if ok1 && ok2 {
		var ev C.sg_event
		ev.saddr, ev.daddr, ev.protocol, ev.status = C.uint32_t(s), C.uint32_t(d), C.SG_PROTO_KAFKA, 1
		if k.Tls {
			ev.flags |= C.SG_EV_TLS
		}
		if k.Type == "CONSUME" {
			ev.flags |= C.SG_EV_CONSUME
		}
		ev.duration_ns, ev.write_time_ns = C.uint64_t(k.Latency), C.uint64_t(uint64(k.StartTime)*1000000)
		g.add(ev, 1)
	}
	if g.divert {
		return nil
	}
	return g.inner.PersistKafkaEvent(request)
}

// PersistAliveConnection: sendOpenConnection already resolved the UIDs (aggregator/data.go:1628-1679); the engine repeats
// the join from the two IPs and only counts the open connection on the edge.
func (g *GraphDS) PersistAliveConnection(trace *datastore.AliveConnection) error {
	if trace != nil {
		if s, ok := ip4(trace.FromIP); ok {
			if d, ok := ip4(trace.ToIP); ok {
				var ev C.sg_event
				ev.saddr, ev.daddr, ev.flags = C.uint32_t(s), C.uint32_t(d), C.SG_EV_ALIVE
				g.add(ev, 1)
			}
		}
	}
	return g.inner.PersistAliveConnection(trace)
}

// IngestL7 is the earlier tap: a second consumer of the ebpf channel, fed the same *l7_req.L7Event processL7 gets
// (aggregator/data.go:1364-1383), which also takes extractAddressPair / setFromToV2 off the CPU.  kafkaMsgs = the number of
// messages the aggregator decoded from a Kafka payload (data.go:1035-1040; 1 otherwise).  HTTP/2 frames are assembled by the
// aggregator first: the finished request comes through IngestHttp2.
func (g *GraphDS) IngestL7(d *l7_req.L7Event, kafkaMsgs int) {
	if d == nil || d.Protocol == l7_req.L7_PROTOCOL_HTTP2 || (g.Filter != nil && !g.Filter(d)) {
		return
	}
	var ev C.sg_event
	ev.saddr, ev.daddr = C.uint32_t(d.Saddr), C.uint32_t(d.Daddr)
	ev.status, ev.duration_ns, ev.write_time_ns = clamp16(d.Status), C.uint64_t(d.Duration), C.uint64_t(d.WriteTimeNs)
	ev.protocol, _ = protoID(d.Protocol)
	if d.Tls {
		ev.flags |= C.SG_EV_TLS
	}
	copies := 1
	switch d.Protocol {
	case l7_req.L7_PROTOCOL_HTTP: // the Host header only decides the identity of an UNKNOWN destination (data.go:851-854)
		if !g.knownIP(d.Daddr) {
			n := d.PayloadSize
			if n > uint32(len(d.Payload)) {
				n = uint32(len(d.Payload))
			}
			if host := hostHeader(string(d.Payload[:n])); host != "" {
				ev.host_label = C.uint32_t(g.label(host))
			}
		}
	case l7_req.L7_PROTOCOL_AMQP:
		if d.Method == l7_req.DELIVER {
			ev.flags |= C.SG_EV_REVERSE
		}
	case l7_req.L7_PROTOCOL_REDIS:
		if d.Method == l7_req.REDIS_PUSHED_EVENT {
			ev.flags |= C.SG_EV_REVERSE
		}
	case l7_req.L7_PROTOCOL_KAFKA:
		ev.status = 1
		if kafkaMsgs < 1 {
			return // the payload decoded to no message: the reference persists nothing (data.go:1041-1079)
		}
		copies = kafkaMsgs
	}
	g.add(ev, copies)
}

// IngestHttp2 takes the request of one finished HTTP/2 stream, next to a.ds.PersistRequest(req) in persistReq
// (aggregator/data.go:576-616); authority = the :authority pseudo-header.
func (g *GraphDS) IngestHttp2(d *l7_req.L7Event, req *datastore.Request, authority string) {
	if d == nil || req == nil {
		return
	}
	var ev C.sg_event
	ev.saddr, ev.daddr, ev.protocol = C.uint32_t(d.Saddr), C.uint32_t(d.Daddr), C.SG_PROTO_HTTP2
	ev.status, ev.duration_ns, ev.write_time_ns = clamp16(req.StatusCode), C.uint64_t(req.Latency), C.uint64_t(d.WriteTimeNs)
	if d.Tls {
		ev.flags |= C.SG_EV_TLS
	}
	if authority != "" && !g.knownIP(d.Daddr) {
		ev.host_label = C.uint32_t(g.label(authority))
	}
	g.add(ev, 1)
}

// ---- window close ----------------------------------------------------------------------------------------------------

// FlushWindow closes the window: K1 pass B .. K5 on the GPU, rows left in the engine's page-locked host buffer
// (sg_flush_begin + sg_flush_end_view: valid until the next flush, so they are converted before this returns).
// SetSelection: from the next FlushWindow on, only the window's selected rows are returned, in selection order — k = 0 every row
// scoring >= minScore in canonical order, 1 <= k <= SG_SELECT_MAX_K the k highest-scoring of them, descending (sg_flush_window_top).
// Only those rows cross PCIe.  ClearSelection returns to every row.
func (g *GraphDS) SetSelection(k uint32, minScore float32) error {
	if k > C.SG_SELECT_MAX_K {
		return fmt.Errorf("servicegraph: selection k = %d beyond SG_SELECT_MAX_K", k)
	}
	g.flushMu.Lock()
	g.selOn, g.selK, g.selMin = true, k, minScore
	g.flushMu.Unlock()
	return nil
}

func (g *GraphDS) ClearSelection() {
	g.flushMu.Lock()
	g.selOn = false
	g.flushMu.Unlock()
}

func (g *GraphDS) FlushWindow(windowEndMs int64) ([]EdgeRow, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	for i := range g.shards { // what the feeders append from here on belongs to the next window
		s := &g.shards[i]
		s.mu.Lock()
		g.flushShard(s)
		s.mu.Unlock()
	}
	g.lblMu.RLock()
	nLabels := len(g.names)
	g.lblMu.RUnlock()
	C.sg_set_label_count(g.h, C.uint32_t(nLabels))
	g.idMu.Lock()
	retire := g.retired
	g.retired = nil
	g.idMu.Unlock()

	// The close in two halves (ABI 3): sg_flush_begin marks the window boundary and returns with K1 pass B .. K5 enqueued;
	// sg_flush_end_view waits for them and fetches the rows WITHOUT the engine lock, so the worker goroutines' sg_ingest calls
	// (add -> flushShard) go on while the rows come back — they belong to the next window.
	var rows *C.sg_edge_out
	var n C.size_t
	if g.selOn { // the selection: only the selected rows leave the device, copied into memory of this call
		capRows := int(g.selK)
		if capRows == 0 || capRows > g.maxEdges {
			capRows = g.maxEdges
		}
		buf := make([]C.sg_edge_out, capRows+1)
		var nsel C.size_t
		if rc := C.sg_flush_window_top(g.h, C.uint64_t(windowEndMs), C.uint32_t(g.selK), C.float(g.selMin), &buf[0], nil, C.size_t(capRows), &nsel, &n); rc != 0 {
			return nil, fmt.Errorf("servicegraph: sg_flush_window_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		rows, n = &buf[0], nsel
		if int(n) > capRows {
			n = C.size_t(capRows)
		}
	} else {
		if rc := C.sg_flush_begin(g.h, C.uint64_t(windowEndMs)); rc != 0 {
			return nil, fmt.Errorf("servicegraph: sg_flush_begin = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		if rc := C.sg_flush_end_view(g.h, &rows, &n); rc != 0 {
			return nil, fmt.Errorf("servicegraph: sg_flush_end_view = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
	}
	var nob C.size_t
	C.sg_window_outbound_ips(g.h, nil, 0, &nob)
	obips := make([]uint32, int(nob))
	if nob > 0 {
		C.sg_window_outbound_ips(g.h, (*C.uint32_t)(unsafe.Pointer(&obips[0])), nob, &nob)
	}
	g.lblMu.RLock() // AFTER the close: a label interned while the window was closing may already be named by a row
	names := g.names
	g.lblMu.RUnlock()

	out := make([]EdgeRow, int(n))
	view := unsafe.Slice(rows, int(n))
	g.idMu.Lock()
	name := func(ref uint32) (string, string) {
		t, v := ref>>30, ref&0x3FFFFFFF
		switch {
		case t == C.SG_REF_KNOWN && int(v) < len(g.uidOf):
			if g.kindOf[v] == kindService {
				return "service", g.uidOf[v]
			}
			return "pod", g.uidOf[v]
		case t == C.SG_REF_LABEL && int(v) < len(names):
			return "outbound", names[v]
		case t == C.SG_REF_OBIP && int(v) < len(obips):
			return "outbound", ipString(obips[v])
		}
		return "unknown", ""
	}
	for i := range view {
		r, o := &view[i], &out[i]
		o.FromType, o.FromUID = name(uint32(r.from_ref))
		o.ToType, o.ToUID = name(uint32(r.to_ref))
		o.Count, o.ErrCount, o.SumNs, o.MaxNs, o.SumSqUs = uint32(r.count), uint32(r.err_count), uint64(r.sum_ns), uint64(r.max_ns), uint64(r.sumsq_us)
		o.Score, o.LatZ, o.ErrRatio = float32(r.score), float32(r.lat_z), float32(r.err_ratio)
		o.Alive, o.P50Us, o.P99Us = uint32(r.alive), uint32(r.p50_us), uint32(r.p99_us)
	}
	// the window that could still name the retired ids has been read: they may be handed out again, unless an IP was
	// bound to them in the meantime
	for _, id := range retire {
		if g.refs[id] != 0 || g.uidOf[id] == "" {
			continue
		}
		if cur, ok := g.ids[g.uidOf[id]]; ok && cur == id {
			delete(g.ids, g.uidOf[id])
		}
		if g.kindOf[id] == kindService {
			g.assignLocked(id, NoGroup) // a Service that was bound leaves its group with its id (never assigned: no call)
		}
		g.uidOf[id], g.kindOf[id] = "", 0
		g.freeIDs = append(g.freeIDs, id)
	}
	g.idMu.Unlock()
	return out, nil
}

// ---- culprit ranking (K11) ---------------------------------------------------------------------------------------------

// Culprit is one service of a window's culprit ranking: Share of the walk's mass that ended at it (sg_node_rank.share), and the
// node's own score from the rollup.
type Culprit struct {
	Type, UID string
	Share     float32
	Score     float32
}

// SetRank switches the per-window culprit ranking on (the node rollup with it): a walk over each window's own graph, caller to
// callee along anomalous rows; iters and dampingQ8 0 = the defaults (20, 218).  ClearRank switches it off and keeps the rollup.
func (g *GraphDS) SetRank(iters, dampingQ8 uint32, uniformSeed bool) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_nodes(g.h, 1); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_nodes = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	var rp C.sg_rank_params
	rp.struct_size = C.uint32_t(unsafe.Sizeof(rp))
	rp.iters, rp.damping_q8, rp.seed = C.uint32_t(iters), C.uint32_t(dampingQ8), C.SG_RANK_SEED_SCORE
	if uniformSeed {
		rp.seed = C.SG_RANK_SEED_UNIFORM
	}
	if rc := C.sg_set_rank(g.h, &rp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_rank = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearRank() {
	g.flushMu.Lock()
	C.sg_set_rank(g.h, nil)
	g.flushMu.Unlock()
}

// WindowCulprits returns the k (1 <= k <= SG_SELECT_MAX_K) highest-ranked services of the window FlushWindow returned last,
// descending, with share >= minShare (sg_window_rank_top: only they cross PCIe).
func (g *GraphDS) WindowCulprits(k uint32, minShare float32) ([]Culprit, error) {
	if k == 0 || k > C.SG_SELECT_MAX_K {
		return nil, fmt.Errorf("servicegraph: culprits k = %d outside 1..SG_SELECT_MAX_K", k)
	}
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	nodes := make([]C.sg_node_out, int(k))
	ranks := make([]C.sg_node_rank, int(k))
	var nsel, nn C.size_t
	if rc := C.sg_window_rank_top(g.h, C.uint32_t(k), C.float(minShare), &nodes[0], &ranks[0], nil, C.size_t(k), &nsel, &nn); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_rank_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if nsel > C.size_t(k) {
		nsel = C.size_t(k)
	}
	var nob C.size_t
	C.sg_window_outbound_ips(g.h, nil, 0, &nob)
	obips := make([]uint32, int(nob))
	if nob > 0 {
		C.sg_window_outbound_ips(g.h, (*C.uint32_t)(unsafe.Pointer(&obips[0])), nob, &nob)
	}
	g.lblMu.RLock()
	names := g.names
	g.lblMu.RUnlock()
	out := make([]Culprit, int(nsel))
	g.idMu.Lock()
	for i := range out {
		ref := uint32(ranks[i].ref)
		t, v := ref>>30, ref&0x3FFFFFFF
		o := &out[i]
		o.Type, o.UID = "unknown", ""
		switch {
		case t == C.SG_REF_KNOWN && int(v) < len(g.uidOf):
			o.Type, o.UID = "pod", g.uidOf[v]
			if g.kindOf[v] == kindService {
				o.Type = "service"
			}
		case t == C.SG_REF_LABEL && int(v) < len(names):
			o.Type, o.UID = "outbound", names[v]
		case t == C.SG_REF_OBIP && int(v) < len(obips):
			o.Type, o.UID = "outbound", ipString(obips[v])
		}
		o.Share, o.Score = float32(ranks[i].share), float32(nodes[i].score)
	}
	g.idMu.Unlock()
	return out, nil
}

// ---- incidents (K12) ---------------------------------------------------------------------------------------------------

// Incident is one connected component of a window's anomalous rows (sg_incident_out): how many services and rows it spans, the
// requests and errors on its rows, its worst row, and the positions (in the window's node rows) of its first, its most anomalous
// and — with the ranking on — its likely culprit service (NoIncident without it).
type Incident struct {
	Nodes, Edges                              uint32
	Count, Err, SumNs                         uint64
	ValueMax                                  float32
	WorstRow, FirstNode, TopNode, CulpritNode uint32
}

// NoIncident is SG_NO_INCIDENT: Incident.CulpritNode when the ranking is off.
const NoIncident = uint32(C.SG_NO_INCIDENT)

// SetIncidents switches the per-window incident grouping on (the node rollup with it): a row is anomalous when its score is at
// least minScore.  ClearIncidents switches it off and keeps the rollup.
func (g *GraphDS) SetIncidents(minScore float32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_nodes(g.h, 1); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_nodes = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	var ip C.sg_incident_params
	ip.struct_size = C.uint32_t(unsafe.Sizeof(ip))
	ip.by, ip.min_value = C.SG_SEL_SCORE, C.float(minScore)
	if rc := C.sg_set_incidents(g.h, &ip); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearIncidents() {
	g.flushMu.Lock()
	C.sg_set_incidents(g.h, nil)
	g.flushMu.Unlock()
}

// WindowIncidents returns the incidents of the window FlushWindow returned last, numbered by their first service
// (sg_window_incidents: one 72-byte row per incident crosses PCIe).
func (g *GraphDS) WindowIncidents() ([]Incident, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_incidents(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	incs := make([]C.sg_incident_out, int(n))
	if rc := C.sg_window_incidents(g.h, &incs[0], C.size_t(len(incs)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(incs) {
		incs = incs[:int(n)]
	}
	out := make([]Incident, len(incs))
	for i := range incs {
		inc, o := &incs[i], &out[i]
		o.Nodes, o.Edges = uint32(inc.nodes), uint32(inc.edges)
		o.Count, o.Err, o.SumNs = uint64(inc.count), uint64(inc.err), uint64(inc.sum_ns)
		o.ValueMax, o.WorstRow = float32(inc.value_max), uint32(inc.worst_row)
		o.FirstNode, o.TopNode, o.CulpritNode = uint32(inc.first_node), uint32(inc.top_node), uint32(inc.culprit_node)
	}
	return out, nil
}

// ---- tracks (K13) ------------------------------------------------------------------------------------------------------

// IncidentTrack is the track of one incident of a window (sg_incident_track): an incident followed over time.  Track never
// changes and is never reused; Parent is the track an opened one broke off from (NoTrack: none); FirstWindow and Windows count
// windows since SetTracks; Kept, Moved and Joined say how many of its services were on this track, on another, or on none.
type IncidentTrack struct {
	Track, Parent, FirstWindow, Windows uint32
	Kept, Moved, Joined                 uint32
	New, Split, Merged                  bool
}

// TrackEntry is one track as the table holds it (sg_track_entry): what WindowTracksEnded lists when a track goes quiet.
type TrackEntry struct {
	Track, Parent, FirstWindow, LastWindow, Windows, PeakNodes uint32
	Count, Err                                                 uint64
}

// NoTrack is SG_NO_TRACK: the parent of a track that continues none.
const NoTrack = uint32(C.SG_NO_TRACK)

// SetTracks switches the tracking of incidents across windows on (SetIncidents first): a track that goes quiet survives
// quietWindows silent windows (0..15) before its id is forgotten.  maxTracks caps the table (88 bytes of device memory a
// position); 0 sizes it so that nothing is ever cut, (quietWindows + 1) x the node capacity — on a large shard set it to what the
// deployment's incident counts need.  Every SetIncidents / ClearIncidents call switches tracking off.
func (g *GraphDS) SetTracks(quietWindows, maxTracks uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_track_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.quiet_windows, tp.max_tracks = C.uint32_t(quietWindows), C.uint32_t(maxTracks)
	if rc := C.sg_set_tracks(g.h, &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearTracks() {
	g.flushMu.Lock()
	C.sg_set_tracks(g.h, nil)
	g.flushMu.Unlock()
}

// WindowIncidentTracks returns the track of every incident of the window FlushWindow returned last: element i belongs to
// WindowIncidents()[i] (sg_window_incident_tracks: one 32-byte row per incident crosses PCIe).
func (g *GraphDS) WindowIncidentTracks() ([]IncidentTrack, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_incident_tracks(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_incident_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	trs := make([]C.sg_incident_track, int(n))
	if rc := C.sg_window_incident_tracks(g.h, &trs[0], C.size_t(len(trs)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_incident_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(trs) {
		trs = trs[:int(n)]
	}
	return incidentTracksOf(trs), nil
}

// incidentTracksOf turns sg_incident_track rows, K13's or K19's, into IncidentTracks.
func incidentTracksOf(trs []C.sg_incident_track) []IncidentTrack {
	out := make([]IncidentTrack, len(trs))
	for i := range trs {
		tr, o := &trs[i], &out[i]
		o.Track, o.Parent, o.FirstWindow, o.Windows = uint32(tr.track), uint32(tr.parent), uint32(tr.first_window), uint32(tr.windows)
		o.Kept, o.Moved, o.Joined = uint32(tr.kept_nodes), uint32(tr.moved_nodes), uint32(tr.joined_nodes)
		o.New, o.Split, o.Merged = tr.flags&C.SG_TRACK_NEW != 0, tr.flags&C.SG_TRACK_SPLIT != 0, tr.flags&C.SG_TRACK_MERGED != 0
	}
	return out
}

// WindowTracksEnded returns the tracks that went quiet in the window FlushWindow returned last, as they stood, in id order
// (sg_window_tracks_ended): each track is listed once, in its first silent window.
func (g *GraphDS) WindowTracksEnded() ([]TrackEntry, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_tracks_ended(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_tracks_ended = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ents := make([]C.sg_track_entry, int(n))
	if rc := C.sg_window_tracks_ended(g.h, &ents[0], C.size_t(len(ents)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_tracks_ended = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(ents) {
		ents = ents[:int(n)]
	}
	return trackEntriesOf(ents), nil
}

// trackEntriesOf turns sg_track_entry rows, K13's or K19's, into TrackEntries.
func trackEntriesOf(ents []C.sg_track_entry) []TrackEntry {
	out := make([]TrackEntry, len(ents))
	for i := range ents {
		en, o := &ents[i], &out[i]
		o.Track, o.Parent, o.FirstWindow, o.LastWindow = uint32(en.track), uint32(en.parent), uint32(en.first_window), uint32(en.last_window)
		o.Windows, o.PeakNodes, o.Count, o.Err = uint32(en.windows), uint32(en.peak_nodes), uint64(en.count), uint64(en.err)
	}
	return out
}

// GroupEdge is one edge of a window's service map contracted to workloads (sg_group_edge): every row from a pod of one group
// (or one ungrouped node) to a pod of another, folded into one.  FromRef / ToRef are group refs: IsGroup(ref) tells a group
// (its id in the low 30 bits) from the node ref of an ungrouped node.
type GroupEdge struct {
	FromRef, ToRef                                 uint32
	Count, ErrCount, SumNs, SumSqUs, MaxNs, ScoreQ uint64
	Edges, FromNodes, First, Alive, WorstRow       uint32
	ScoreMax                                       float32
}

// NoGroup is SG_NO_GROUP: AssignGroups takes a node out of its group with it.
const NoGroup = uint32(C.SG_NO_GROUP)

// IsGroup tells whether a GroupEdge ref names a group (then ref & 0x3FFFFFFF is its id) rather than a node.
func IsGroup(ref uint32) bool { return ref>>30 == uint32(C.SG_REF_GROUP) }

// SetGroups switches the per-window contraction to workloads on (maxGroups = 0: as many groups as node ids) with nothing
// grouped; ClearGroups switches it off.  It needs none of the other stages.
func (g *GraphDS) SetGroups(maxGroups uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var gp C.sg_group_params
	gp.struct_size = C.uint32_t(unsafe.Sizeof(gp))
	gp.max_groups = C.uint32_t(maxGroups)
	if rc := C.sg_set_groups(g.h, &gp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_groups = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	g.idMu.Lock()
	g.nodeGroup = map[uint32]uint32{} // the engine's map starts over
	g.idMu.Unlock()
	return nil
}

func (g *GraphDS) ClearGroups() {
	g.flushMu.Lock()
	C.sg_set_groups(g.h, nil)
	g.flushMu.Unlock()
	g.idMu.Lock()
	g.nodeGroup = map[uint32]uint32{}
	g.idMu.Unlock()
}

// AssignGroups puts node nodeIDs[i] into group groups[i] (NoGroup: into none), in that order; the windows closed from now on
// see it.  The ids are the node ids PersistPod / PersistService interned (the pod's workload is the caller's to resolve:
// Pod.OwnerID, its ReplicaSet's OwnerID).
func (g *GraphDS) AssignGroups(nodeIDs, groups []uint32) error {
	if len(nodeIDs) != len(groups) {
		return fmt.Errorf("servicegraph: AssignGroups: %d ids, %d groups", len(nodeIDs), len(groups))
	}
	if len(nodeIDs) == 0 {
		return nil
	}
	ids := (*C.uint32_t)(unsafe.Pointer(&nodeIDs[0]))
	gs := (*C.uint32_t)(unsafe.Pointer(&groups[0]))
	g.idMu.Lock()
	defer g.idMu.Unlock()
	if rc := C.sg_group_assign(g.h, ids, gs, C.size_t(len(nodeIDs))); rc != 0 {
		return fmt.Errorf("servicegraph: sg_group_assign = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	for i, id := range nodeIDs { // what the engine holds now; the Services behind which a re-grouped pod stands follow it
		if groups[i] == NoGroup {
			delete(g.nodeGroup, id)
		} else {
			g.nodeGroup[id] = groups[i]
		}
	}
	for _, id := range nodeIDs {
		if int(id) < len(g.uidOf) && g.kindOf[id] == kindPod {
			g.bindServicesOfPod(g.uidOf[id])
		}
	}
	return nil
}

// WindowGroupEdges returns the group edges of the window FlushWindow returned last, ascending by (from, to) with the groups
// first (sg_window_groups: 80 bytes per group edge cross PCIe, not 64 per row).
func (g *GraphDS) WindowGroupEdges() ([]GroupEdge, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_groups(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_groups = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ges := make([]C.sg_group_edge, int(n))
	if rc := C.sg_window_groups(g.h, &ges[0], C.size_t(len(ges)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_groups = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(ges) {
		ges = ges[:int(n)]
	}
	return goGroupEdges(ges), nil
}

func goGroupEdges(ges []C.sg_group_edge) []GroupEdge {
	out := make([]GroupEdge, len(ges))
	for i := range ges {
		ge, o := &ges[i], &out[i]
		o.FromRef, o.ToRef = uint32(ge.from_ref), uint32(ge.to_ref)
		o.Count, o.ErrCount, o.SumNs, o.SumSqUs = uint64(ge.count), uint64(ge.err_count), uint64(ge.sum_ns), uint64(ge.sumsq_us)
		o.MaxNs, o.ScoreQ = uint64(ge.max_ns), uint64(ge.score_q32)
		o.Edges, o.FromNodes, o.First, o.Alive = uint32(ge.edges), uint32(ge.from_nodes), uint32(ge.first), uint32(ge.alive)
		o.WorstRow, o.ScoreMax = uint32(ge.worst_row), float32(ge.score_max)
	}
	return out
}

// EdgeTrend is one group edge against its own past (sg_edge_trend): the deviations of this window's latency and error share from
// the workload baseline in units of its mean absolute deviation, the baseline's mean latency, and the windows it has seen.
type EdgeTrend struct {
	LatDev, ErrDev, BaseMeanUs float32
	WindowsSeen                uint32
}

// VanishedWorkload is one workload dependency that went silent (sg_edge_vanished over workload keys): a key below 2^32 is a group
// id, any other (1 + ref type) << 32 | value of an ungrouped node.  Row is the window's group edge with the key and no request
// (open connections only), or 0xFFFFFFFF.
type VanishedWorkload struct {
	FromKey, ToKey                    uint64
	LatMean, LatDev, ErrMean, ErrDev float64
	N, Last, Row                      uint32
}

// The keys of WindowWorkloadsTop (SG_SEL_*).
const (
	ByScore  = uint32(C.SG_SEL_SCORE)
	ByLatDev = uint32(C.SG_SEL_LAT_DEV)
	ByErrDev = uint32(C.SG_SEL_ERR_DEV)
	ByNew    = uint32(C.SG_SEL_NEW)
)

// SetWorkloadTrend switches the per-workload-edge baseline on, behind SetGroups (a 0 is the parameter's default: shift 4, warmup 4,
// ttl 64, maxEntries 2 x max_edges); it starts empty.  The baseline is keyed by workload, so it survives a rollout that gives a
// Deployment new pods.  Any SetGroups call switches it off.
func (g *GraphDS) SetWorkloadTrend(shift, warmup, ttl uint32, maxEntries uint64) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_trend_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.shift, tp.warmup, tp.ttl, tp.max_entries = C.uint32_t(shift), C.uint32_t(warmup), C.uint32_t(ttl), C.uint64_t(maxEntries)
	if rc := C.sg_set_group_trend(g.h, &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if g.wlEntries = maxEntries; maxEntries == 0 {
		if g.wlEntries = 2 * uint64(g.maxEdges); g.wlEntries == 0 {
			g.wlEntries = 2
		} else if g.wlEntries > 1<<31 {
			g.wlEntries = 1 << 31
		}
	}
	return nil
}

// SetWorkloadVanished switches the list of vanished workload dependencies on, behind SetWorkloadTrend (a 0 is the parameter's
// default: silent for 1 window, seen in warmup windows, 65536 rows).  Any SetWorkloadTrend call switches it off.
func (g *GraphDS) SetWorkloadVanished(silentWindows, minSeen, maxRows uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var vp C.sg_vanished_params
	vp.struct_size = C.uint32_t(unsafe.Sizeof(vp))
	vp.silent_windows, vp.min_seen, vp.max_rows = C.uint32_t(silentWindows), C.uint32_t(minSeen), C.uint32_t(maxRows)
	if rc := C.sg_set_group_vanished(g.h, &vp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_vanished = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if g.wlVanRows = int(maxRows); maxRows == 0 { // (sg_vanished_params' default)
		if g.wlVanRows = 65536; g.wlEntries < 65536 {
			g.wlVanRows = int(g.wlEntries)
		}
	}
	return nil
}

// WindowWorkloadTrend returns the trend rows of the window FlushWindow returned last: row k for group edge k of WindowGroupEdges,
// or, with an index (WindowWorkloadsTop's), the rows of those group edges only.
func (g *GraphDS) WindowWorkloadTrend(index []uint32) ([]EdgeTrend, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	var idx *C.uint32_t
	if index != nil {
		if len(index) == 0 {
			return nil, nil
		}
		idx, n = (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index))
	} else if rc := C.sg_window_group_trend(g.h, nil, 0, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ts := make([]C.sg_edge_trend, int(n))
	if rc := C.sg_window_group_trend(g.h, idx, C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	out := make([]EdgeTrend, len(ts))
	for i := range ts {
		out[i] = EdgeTrend{float32(ts[i].lat_dev), float32(ts[i].err_dev), float32(ts[i].base_mean_us), uint32(ts[i].windows_seen)}
	}
	return out, nil
}

// WindowWorkloadsTop selects from the group edges of the window FlushWindow returned last on the device (sg_window_groups_top):
// the k group edges with the highest value >= minValue, descending, ties by position (k = 0: every such group edge, in order),
// and their indices.  by: ByScore (the group edge's ScoreMax; it needs SetGroups only), ByLatDev, ByErrDev, ByNew (group edges
// with requests that the baseline has not seen).
func (g *GraphDS) WindowWorkloadsTop(by, k uint32, minValue float32) ([]GroupEdge, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_groups_top(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, fmt.Errorf("servicegraph: sg_window_groups_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil
	}
	ges, index := make([]C.sg_group_edge, room), make([]uint32, room)
	if rc := C.sg_window_groups_top(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), &ges[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, fmt.Errorf("servicegraph: sg_window_groups_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ges, index = ges[:int(sel)], index[:int(sel)]
	}
	return goGroupEdges(ges), index, nil
}

// WindowWorkloadsVanished returns the workload dependencies that went silent in the window FlushWindow returned last, ascending by
// key, and the count of all of them (the list holds at most the maxRows of SetWorkloadVanished).
func (g *GraphDS) WindowWorkloadsVanished() ([]VanishedWorkload, int, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_vanished(g.h, nil, 0, &n); rc != 0 {
		return nil, 0, fmt.Errorf("servicegraph: sg_window_group_vanished = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 || g.wlVanRows == 0 {
		return nil, int(n), nil
	}
	room := int(n) // n counts every vanished entry; the list holds at most maxRows of them
	if room > g.wlVanRows {
		room = g.wlVanRows
	}
	vs := make([]C.sg_edge_vanished, room)
	if rc := C.sg_window_group_vanished(g.h, &vs[0], C.size_t(len(vs)), &n); rc != 0 {
		return nil, 0, fmt.Errorf("servicegraph: sg_window_group_vanished = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	out := make([]VanishedWorkload, 0, len(vs))
	for i := range vs {
		v := &vs[i]
		out = append(out, VanishedWorkload{uint64(v.from_key), uint64(v.to_key), float64(v.lat_mean), float64(v.lat_dev),
			float64(v.err_mean), float64(v.err_dev), uint32(v.n), uint32(v.last), uint32(v.row)})
	}
	return out, int(n), nil
}

// WorkloadNode is one workload row of a window (sg_node_out over group edges, K16): Ref is a group ref — type 3 and the group id,
// or the node's own ref when it is ungrouped.  The Out fields reduce the group edges the workload calls through, the In fields
// those it is called through; Edges count peer workloads, not rows; WorstRow is a row index of the window's rows.
type WorkloadNode struct {
	Ref                                                                  uint32
	OutCount, InCount, OutErr, InErr, OutSumNs, InSumNs                  uint64
	OutSumSqUs, InSumSqUs, OutMaxNs, InMaxNs, OutScoreQ32, InScoreQ32    uint64
	OutEdges, InEdges, OutAlive, InAlive, OutWorstRow, InWorstRow        uint32
	OutScoreMax, InScoreMax, Score                                       float32
}

// NodeTrend is one workload row against its own past (sg_node_trend), a side each for the calls it receives and those it makes.
type NodeTrend struct {
	InLatDev, InErrDev, OutLatDev, OutErrDev, InBaseMeanUs, OutBaseMeanUs float32
	InSeen, OutSeen                                                       uint32
}

// The keys of WindowWorkloadNodesTop (SG_NSEL_*).
const (
	NodeByScore     = uint32(C.SG_NSEL_SCORE)
	NodeByInLatDev  = uint32(C.SG_NSEL_IN_LAT_DEV)
	NodeByInErrDev  = uint32(C.SG_NSEL_IN_ERR_DEV)
	NodeByOutLatDev = uint32(C.SG_NSEL_OUT_LAT_DEV)
	NodeByOutErrDev = uint32(C.SG_NSEL_OUT_ERR_DEV)
	NodeByNew       = uint32(C.SG_NSEL_NEW)
)

// SetWorkloadNodes switches the per-window workload rows on or off, behind SetGroups: every window's group edges rolled up per
// workload on the device.  Any SetGroups call switches them off.
func (g *GraphDS) SetWorkloadNodes(on bool) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	v := C.int(0)
	if on {
		v = 1
	}
	if rc := C.sg_set_group_nodes(g.h, v); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_nodes = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// SetWorkloadNodeTrend switches the per-workload baseline on, behind SetWorkloadNodes (a 0 is the parameter's default: shift 4,
// warmup 4, ttl 64, maxEntries 4 x the row capacity); it starts empty.  It is keyed by workload and survives a rollout.
func (g *GraphDS) SetWorkloadNodeTrend(shift, warmup, ttl uint32, maxEntries uint64) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_trend_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.shift, tp.warmup, tp.ttl, tp.max_entries = C.uint32_t(shift), C.uint32_t(warmup), C.uint32_t(ttl), C.uint64_t(maxEntries)
	if rc := C.sg_set_group_node_trend(g.h, &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_node_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func goWorkloadNodes(ns []C.sg_node_out) []WorkloadNode {
	out := make([]WorkloadNode, len(ns))
	for i := range ns {
		n, o := &ns[i], &out[i]
		o.Ref = uint32(n.ref)
		o.OutCount, o.InCount, o.OutErr, o.InErr = uint64(n.out_count), uint64(n.in_count), uint64(n.out_err), uint64(n.in_err)
		o.OutSumNs, o.InSumNs, o.OutSumSqUs, o.InSumSqUs = uint64(n.out_sum_ns), uint64(n.in_sum_ns), uint64(n.out_sumsq_us), uint64(n.in_sumsq_us)
		o.OutMaxNs, o.InMaxNs, o.OutScoreQ32, o.InScoreQ32 = uint64(n.out_max_ns), uint64(n.in_max_ns), uint64(n.out_score_q32), uint64(n.in_score_q32)
		o.OutEdges, o.InEdges, o.OutAlive, o.InAlive = uint32(n.out_edges), uint32(n.in_edges), uint32(n.out_alive), uint32(n.in_alive)
		o.OutWorstRow, o.InWorstRow = uint32(n.out_worst_row), uint32(n.in_worst_row)
		o.OutScoreMax, o.InScoreMax, o.Score = float32(n.out_score_max), float32(n.in_score_max), float32(n.score)
	}
	return out
}

// WindowWorkloadNodes returns the workload rows of the window FlushWindow returned last, ascending by group key: the workloads by
// id, then the ungrouped nodes.
func (g *GraphDS) WindowWorkloadNodes() ([]WorkloadNode, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_nodes(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_nodes = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ns := make([]C.sg_node_out, int(n))
	if rc := C.sg_window_group_nodes(g.h, &ns[0], C.size_t(len(ns)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_nodes = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(ns) {
		ns = ns[:int(n)]
	}
	return goWorkloadNodes(ns), nil
}

// WindowWorkloadNodeTrend returns the trend rows of the window FlushWindow returned last: row k for row k of WindowWorkloadNodes,
// or, with an index (WindowWorkloadNodesTop's), the rows of those workloads only.
func (g *GraphDS) WindowWorkloadNodeTrend(index []uint32) ([]NodeTrend, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	var idx *C.uint32_t
	if index != nil {
		if len(index) == 0 {
			return nil, nil
		}
		idx, n = (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index))
	} else if rc := C.sg_window_group_node_trend(g.h, nil, 0, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_node_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ts := make([]C.sg_node_trend, int(n))
	if rc := C.sg_window_group_node_trend(g.h, idx, C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_node_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	out := make([]NodeTrend, len(ts))
	for i := range ts {
		t := &ts[i]
		out[i] = NodeTrend{float32(t.in_lat_dev), float32(t.in_err_dev), float32(t.out_lat_dev), float32(t.out_err_dev),
			float32(t.in_base_mean_us), float32(t.out_base_mean_us), uint32(t.in_seen), uint32(t.out_seen)}
	}
	return out, nil
}

// WindowWorkloadNodesTop selects from the workload rows of the window FlushWindow returned last on the device
// (sg_window_group_nodes_top): the k rows with the highest value >= minValue, descending, ties by position (k = 0: every such
// row, in order), and their indices.  by: NodeByScore (it needs SetWorkloadNodes only) or a key of the baseline.
func (g *GraphDS) WindowWorkloadNodesTop(by, k uint32, minValue float32) ([]WorkloadNode, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_group_nodes_top(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil
	}
	ns, index := make([]C.sg_node_out, room), make([]uint32, room)
	if rc := C.sg_window_group_nodes_top(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), &ns[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, index = ns[:int(sel)], index[:int(sel)]
	}
	return goWorkloadNodes(ns), index, nil
}

// ---- workload ranking (K17) ----------------------------------------------------------------------------------------------

// WorkloadCulprit is one workload of a window's workload ranking: its row as WindowWorkloadNodes gives it, the walk's mass that
// ended at it (sg_node_rank.rank, of 2^56) and that as a share.
type WorkloadCulprit struct {
	Node  WorkloadNode
	Rank  uint64
	Share float32
}

// SetWorkloadRank switches the per-window workload ranking on, behind SetWorkloadNodes: K11's walk over the window's group edges and
// workload rows, so that the answer is a workload and survives a rollout; iters and dampingQ8 0 = the defaults (20, 218).  It is
// independent of SetRank.  ClearWorkloadRank switches it off; SetWorkloadNodes(false) and any SetGroups call do so too.
func (g *GraphDS) SetWorkloadRank(iters, dampingQ8 uint32, uniformSeed bool, seedMinScore float32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var rp C.sg_rank_params
	rp.struct_size = C.uint32_t(unsafe.Sizeof(rp))
	rp.iters, rp.damping_q8, rp.seed, rp.seed_min_score = C.uint32_t(iters), C.uint32_t(dampingQ8), C.SG_RANK_SEED_SCORE, C.float(seedMinScore)
	if uniformSeed {
		rp.seed = C.SG_RANK_SEED_UNIFORM
	}
	if rc := C.sg_set_group_rank(g.h, &rp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_rank = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearWorkloadRank() {
	g.flushMu.Lock()
	C.sg_set_group_rank(g.h, nil)
	g.flushMu.Unlock()
}

// WindowWorkloadCulprits selects from the workload rank rows of the window FlushWindow returned last on the device
// (sg_window_group_rank_top): the k highest-ranked workloads with share >= minShare, descending, ties by position (k = 0: every
// such workload, in row order), and their indices into WindowWorkloadNodes.  Only they cross PCIe.
func (g *GraphDS) WindowWorkloadCulprits(k uint32, minShare float32) ([]WorkloadCulprit, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_group_rank_top(g.h, 0, C.float(minShare), nil, nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, fmt.Errorf("servicegraph: sg_window_group_rank_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil
	}
	ns, rs, index := make([]C.sg_node_out, room), make([]C.sg_node_rank, room), make([]uint32, room)
	if rc := C.sg_window_group_rank_top(g.h, C.uint32_t(k), C.float(minShare), &ns[0], &rs[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, fmt.Errorf("servicegraph: sg_window_group_rank_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, rs, index = ns[:int(sel)], rs[:int(sel)], index[:int(sel)]
	}
	nodes := goWorkloadNodes(ns)
	out := make([]WorkloadCulprit, len(nodes))
	for i := range out {
		out[i] = WorkloadCulprit{nodes[i], uint64(rs[i].rank), float32(rs[i].share)}
	}
	return out, index, nil
}

// ---- workload incidents (K18) --------------------------------------------------------------------------------------------

// SetWorkloadIncidents switches the per-window workload incident grouping on, behind SetWorkloadNodes: K12's grouping over the
// window's group edges and workload rows.  A group edge is anomalous when its value is at least minValue; by is "score" (the group
// edge's largest score), "lat_dev" or "err_dev" (the workload baseline's deviation, SetGroupTrend first: it survives a rollout).
// It is independent of SetIncidents.  ClearWorkloadIncidents switches it off; SetWorkloadNodes(false) and any SetGroups call do so too.
func (g *GraphDS) SetWorkloadIncidents(by string, minValue float32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var ip C.sg_incident_params
	ip.struct_size = C.uint32_t(unsafe.Sizeof(ip))
	ip.min_value = C.float(minValue)
	switch by {
	case "", "score":
		ip.by = C.SG_SEL_SCORE
	case "lat_dev":
		ip.by = C.SG_SEL_LAT_DEV
	case "err_dev":
		ip.by = C.SG_SEL_ERR_DEV
	default:
		return fmt.Errorf("servicegraph: SetWorkloadIncidents by %q: score, lat_dev or err_dev", by)
	}
	if rc := C.sg_set_group_incidents(g.h, &ip); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearWorkloadIncidents() {
	g.flushMu.Lock()
	C.sg_set_group_incidents(g.h, nil)
	g.flushMu.Unlock()
}

// WindowWorkloadIncidents returns the workload incidents of the window FlushWindow returned last, numbered by their first workload
// (sg_window_group_incidents: one 72-byte row per incident crosses PCIe).  FirstNode, TopNode and CulpritNode (NoIncident without
// SetWorkloadRank) index WindowWorkloadNodes; WorstRow indexes the window's group edges.
func (g *GraphDS) WindowWorkloadIncidents() ([]Incident, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_incidents(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	incs := make([]C.sg_incident_out, int(n))
	if rc := C.sg_window_group_incidents(g.h, &incs[0], C.size_t(len(incs)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_incidents = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(incs) {
		incs = incs[:int(n)]
	}
	out := make([]Incident, len(incs))
	for i := range incs {
		inc, o := &incs[i], &out[i]
		o.Nodes, o.Edges = uint32(inc.nodes), uint32(inc.edges)
		o.Count, o.Err, o.SumNs = uint64(inc.count), uint64(inc.err), uint64(inc.sum_ns)
		o.ValueMax, o.WorstRow = float32(inc.value_max), uint32(inc.worst_row)
		o.FirstNode, o.TopNode, o.CulpritNode = uint32(inc.first_node), uint32(inc.top_node), uint32(inc.culprit_node)
	}
	return out, nil
}

// ---- workload tracks (K19) -----------------------------------------------------------------------------------------------

// WorkloadImpact is one impact row of the workload impact (K22): who depends on a workload incident.  FarHops / FarRow: the
// largest distance among the exposed workloads and the smallest workload row that has it (FarRow = NoIncident when nothing is
// exposed; FarHops equal to SetWorkloadImpact's maxHops: the search may have been cut).
type WorkloadImpact struct {
	Exposed, Direct, Entries, EntryCount, EntryErr, IntoCount, IntoErr uint64
	FarHops, FarRow                                                    uint32
}

// SetWorkloadImpact switches the upstream impact of the workload incidents on, behind SetWorkloadIncidents: the first maxIncidents
// incidents of a window are covered (1 .. 1024) and the search against the call edges is cut at maxHops (1 .. 64).
// ClearWorkloadImpact switches it off; every SetWorkloadIncidents / ClearWorkloadIncidents call does so too.
func (g *GraphDS) SetWorkloadImpact(maxIncidents, maxHops uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_group_impact(g.h, C.uint32_t(maxIncidents), C.uint32_t(maxHops)); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_impact = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearWorkloadImpact() {
	g.flushMu.Lock()
	C.sg_set_group_impact(g.h, 0, 0)
	g.flushMu.Unlock()
}

// WindowWorkloadImpact returns the impact rows of the window FlushWindow returned last: row i belongs to
// WindowWorkloadIncidents()[i] (sg_window_group_impact: 64 bytes per covered incident cross PCIe, no group edge does).
func (g *GraphDS) WindowWorkloadImpact() ([]WorkloadImpact, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_impact(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_impact = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	w := make([]uint64, int(n)*int(C.SG_IMPACT_WORDS))
	if rc := C.sg_window_group_impact(g.h, (*C.uint64_t)(unsafe.Pointer(&w[0])), n, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_impact = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	out := make([]WorkloadImpact, int(n))
	for i := range out {
		r := w[i*int(C.SG_IMPACT_WORDS):]
		out[i] = WorkloadImpact{Exposed: r[C.SG_IMPACT_EXPOSED], Direct: r[C.SG_IMPACT_DIRECT], FarHops: uint32(r[C.SG_IMPACT_FAR] >> 32),
			FarRow: uint32(r[C.SG_IMPACT_FAR]), Entries: r[C.SG_IMPACT_ENTRIES], EntryCount: r[C.SG_IMPACT_ENTRY_COUNT],
			EntryErr: r[C.SG_IMPACT_ENTRY_ERR], IntoCount: r[C.SG_IMPACT_INTO_COUNT], IntoErr: r[C.SG_IMPACT_INTO_ERR]}
	}
	return out, nil
}

// SetWorkloadTracks switches the tracking of workload incidents across windows on, behind SetWorkloadIncidents: K13's tracking
// over the workload incidents and workload rows, so that an incident keeps its track when a rollout replaces every pod of a
// Deployment.  quietWindows and maxTracks are SetTracks' (maxTracks 0: (quietWindows + 1) x the workload rows' capacity).  It is
// independent of SetTracks.  ClearWorkloadTracks switches it off; every SetWorkloadIncidents / ClearWorkloadIncidents call,
// SetWorkloadNodes(false) and any SetGroups call do so too.  A pod that moves to another workload does not take its membership
// along: the old workload's fades after quietWindows.
func (g *GraphDS) SetWorkloadTracks(quietWindows, maxTracks uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_track_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.quiet_windows, tp.max_tracks = C.uint32_t(quietWindows), C.uint32_t(maxTracks)
	if rc := C.sg_set_group_tracks(g.h, &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_group_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func (g *GraphDS) ClearWorkloadTracks() {
	g.flushMu.Lock()
	C.sg_set_group_tracks(g.h, nil)
	g.flushMu.Unlock()
}

// WindowWorkloadIncidentTracks returns the track of every workload incident of the window FlushWindow returned last: element i
// belongs to WindowWorkloadIncidents()[i] (sg_window_group_incident_tracks: one 32-byte row per incident crosses PCIe).
func (g *GraphDS) WindowWorkloadIncidentTracks() ([]IncidentTrack, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_incident_tracks(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_incident_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	trs := make([]C.sg_incident_track, int(n))
	if rc := C.sg_window_group_incident_tracks(g.h, &trs[0], C.size_t(len(trs)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_incident_tracks = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(trs) {
		trs = trs[:int(n)]
	}
	return incidentTracksOf(trs), nil
}

// WindowWorkloadTracksEnded returns the workload tracks that went quiet in the window FlushWindow returned last, as they stood, in
// id order (sg_window_group_tracks_ended): each track is listed once, in its first silent window.
func (g *GraphDS) WindowWorkloadTracksEnded() ([]TrackEntry, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var n C.size_t
	if rc := C.sg_window_group_tracks_ended(g.h, nil, 0, &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_tracks_ended = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if n == 0 {
		return nil, nil
	}
	ents := make([]C.sg_track_entry, int(n))
	if rc := C.sg_window_group_tracks_ended(g.h, &ents[0], C.size_t(len(ents)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_group_tracks_ended = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(n) < len(ents) {
		ents = ents[:int(n)]
	}
	return trackEntriesOf(ents), nil
}

// ---- latency percentiles (K20) -------------------------------------------------------------------------------------------

// The spaces of SetQuantiles (SG_Q_*).
const (
	QuantileNodes     uint32 = 1
	QuantileWorkEdges uint32 = 2
	QuantileWorkloads uint32 = 4
)

// SetQuantiles switches the per-window latency histograms and percentiles on for the spaces given (QuantileNodes needs
// SetNodes, QuantileWorkEdges SetGroups, QuantileWorkloads SetWorkloadNodes; the engine was created with the edge histogram):
// percentiles do not average, so a service's or a workload's p99 comes from the merged histogram of its rows only.  permille
// holds up to eight values in 1 .. 1000; none means {500, 990}.  spaces 0 switches the stage off.
func (g *GraphDS) SetQuantiles(spaces uint32, permille ...uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var p *C.uint32_t
	if len(permille) > 0 {
		p = (*C.uint32_t)(unsafe.Pointer(&permille[0]))
	}
	if rc := C.sg_set_quantiles(g.h, C.uint32_t(spaces), p, C.size_t(len(permille))); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_quantiles = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	g.nQ = len(permille)
	if g.nQ == 0 {
		g.nQ = 2
	}
	return nil
}

// latencyRows reads one space's quantiles of the window FlushWindow returned last: words uint32 per entity, every entity
// (index nil) or those at index (only they cross PCIe).
func (g *GraphDS) latencyRows(which int, index []uint32, words int) ([]uint32, int, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	read := func(idx *C.uint32_t, nIdx C.size_t, out *C.uint32_t, cap C.size_t, n *C.size_t) C.int {
		switch which {
		case 0:
			return C.sg_window_node_quantiles(g.h, idx, nIdx, out, cap, n)
		case 1:
			return C.sg_window_group_quantiles(g.h, idx, nIdx, out, cap, n)
		}
		return C.sg_window_group_node_quantiles(g.h, idx, nIdx, out, cap, n)
	}
	var idx *C.uint32_t
	n := C.size_t(len(index))
	if index == nil {
		if rc := read(nil, 0, nil, 0, &n); rc != 0 {
			return nil, 0, fmt.Errorf("servicegraph: latency read = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
	} else if len(index) > 0 {
		idx = (*C.uint32_t)(unsafe.Pointer(&index[0]))
	}
	if n == 0 {
		return nil, 0, nil
	}
	out := make([]uint32, int(n)*words)
	if rc := read(idx, C.size_t(len(index)), (*C.uint32_t)(unsafe.Pointer(&out[0])), n, &n); rc != 0 {
		return nil, 0, fmt.Errorf("servicegraph: latency read = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return out, int(n), nil
}

// NodeLatency returns the quantiles, in microseconds, of the node rows of the window FlushWindow returned last: element
// [k*2*nQ + side*nQ + j] is quantile j of side (0 out, 1 in) of node row k (sg_window_node_quantiles); nQ is the number of
// per-mille values SetQuantiles took.  index nil: every node row.
func (g *GraphDS) NodeLatency(index []uint32) (us []uint32, rows int, err error) {
	return g.latencyRows(0, index, 2*g.nQ)
}

// WorkloadEdgeLatency returns the quantiles of the group edges: element [k*nQ + j] (sg_window_group_quantiles).
func (g *GraphDS) WorkloadEdgeLatency(index []uint32) (us []uint32, rows int, err error) {
	return g.latencyRows(1, index, g.nQ)
}

// WorkloadLatency returns the quantiles of the workload rows, laid out as NodeLatency's (sg_window_group_node_quantiles).
func (g *GraphDS) WorkloadLatency(index []uint32) (us []uint32, rows int, err error) {
	return g.latencyRows(2, index, 2*g.nQ)
}

// ---- tail baselines (K21) ------------------------------------------------------------------------------------------------

// SetTailTrend switches the tail baselines on for the spaces given (QuantileNodes, QuantileWorkEdges, QuantileWorkloads; each
// among those SetQuantiles has on): an exponentially weighted baseline of ONE quantile — permille, one of the values SetQuantiles
// took — per service side, workload edge and workload side, with the keys of the mean baseline of that space, so a workload's
// history survives a rollout.  A 0 is the parameter's default (shift 4, warmup 4, ttl 64, maxEntries as the mean baseline of the
// space).  Every call starts empty baselines; any SetQuantiles call switches the stage off.
func (g *GraphDS) SetTailTrend(spaces, permille, shift, warmup, ttl uint32, maxEntries uint64) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_trend_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.shift, tp.warmup, tp.ttl, tp.max_entries = C.uint32_t(shift), C.uint32_t(warmup), C.uint32_t(ttl), C.uint64_t(maxEntries)
	if rc := C.sg_set_quantile_trend(g.h, C.uint32_t(spaces), C.uint32_t(permille), &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_quantile_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// ClearTailTrend switches the tail baselines off and frees them.
func (g *GraphDS) ClearTailTrend() error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_quantile_trend(g.h, 0, 0, nil); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_quantile_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// WindowTailRegressions answers "which workloads' tail latency left its own normal band" for the window FlushWindow returned
// last, on the device (sg_window_group_nodes_top_tail): the k workload rows with the highest value >= minValue of key by
// (NodeByInLatDev: the deviation of the tracked quantile of the calls the workload receives; any NodeBy* key), descending, with
// their tail rows (sg_window_group_node_quantile_trend at the selected indices) and their indices into WindowWorkloadNodes.
// k = 0: every such row, in order.  It needs SetTailTrend over QuantileWorkloads.
func (g *GraphDS) WindowTailRegressions(by, k uint32, minValue float32) ([]WorkloadNode, []NodeTrend, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_group_nodes_top_tail(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_tail = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil, nil
	}
	ns, index := make([]C.sg_node_out, room), make([]uint32, room)
	if rc := C.sg_window_group_nodes_top_tail(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), &ns[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_tail = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, index = ns[:int(sel)], index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil, nil
	}
	var n C.size_t
	ts := make([]C.sg_node_trend, len(index))
	if rc := C.sg_window_group_node_quantile_trend(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_node_quantile_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	trends := make([]NodeTrend, len(ts))
	for i := range ts {
		t := &ts[i]
		trends[i] = NodeTrend{float32(t.in_lat_dev), float32(t.in_err_dev), float32(t.out_lat_dev), float32(t.out_err_dev),
			float32(t.in_base_mean_us), float32(t.out_base_mean_us), uint32(t.in_seen), uint32(t.out_seen)}
	}
	return goWorkloadNodes(ns), trends, index, nil
}

// ---- traffic baselines (K23) ---------------------------------------------------------------------------------------------

// The spaces of the traffic baselines (SG_T_*), the directions of a selection by a traffic row and the side they are ORed with on
// services and workloads (SG_TSEL_*).
const (
	TrafficEdges     = uint32(C.SG_T_EDGES)
	TrafficNodes     = uint32(C.SG_T_NODES)
	TrafficWorkEdges = uint32(C.SG_T_GROUPS)
	TrafficWorkloads = uint32(C.SG_T_GROUP_NODES)

	TrafficSurge    = uint32(C.SG_TSEL_SURGE)
	TrafficDrop     = uint32(C.SG_TSEL_DROP)
	TrafficLoadUp   = uint32(C.SG_TSEL_LOAD_UP)
	TrafficLoadDown = uint32(C.SG_TSEL_LOAD_DOWN)
	TrafficIn       = uint32(C.SG_TSEL_IN)
	TrafficOut      = uint32(C.SG_TSEL_OUT)
)

// TrafficStats is the running statistics of one traffic baseline (sg_trend_stats).
type TrafficStats struct {
	Windows, Entries, Inserted, Expired, Dropped uint64
}

// SetTrafficTrend switches the traffic baselines on for the spaces given (TrafficEdges needs nothing, TrafficNodes SetNodes,
// TrafficWorkEdges SetGroups, TrafficWorkloads SetWorkloadNodes): an exponentially weighted baseline of HOW MUCH traffic each edge,
// service side, workload edge and workload side carries — its requests per window and its busy time — with the keys of the mean
// baseline of that space, so a workload's history survives a rollout.  A partial drop or a surge shows here while latency and
// error ratio stay calm; windows are assumed to be of equal length.  A 0 is the parameter's default (shift 4, warmup 4, ttl 64,
// maxEntries as the mean baseline of the space, rateFloor 8 requests, loadFloorNs 1 ms).  Every call starts empty baselines.
func (g *GraphDS) SetTrafficTrend(spaces, shift, warmup, ttl uint32, maxEntries uint64, rateFloor uint32, loadFloorNs uint64) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tp C.sg_traffic_params
	tp.struct_size = C.uint32_t(unsafe.Sizeof(tp))
	tp.shift, tp.warmup, tp.ttl, tp.max_entries = C.uint32_t(shift), C.uint32_t(warmup), C.uint32_t(ttl), C.uint64_t(maxEntries)
	tp.rate_floor, tp.load_floor_ns = C.uint32_t(rateFloor), C.uint64_t(loadFloorNs)
	if rc := C.sg_set_traffic_trend(g.h, C.uint32_t(spaces), &tp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_traffic_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// ClearTrafficTrend switches the traffic baselines off and frees them.
func (g *GraphDS) ClearTrafficTrend() error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_traffic_trend(g.h, 0, nil); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_traffic_trend = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func goNodeTrends(ts []C.sg_node_trend) []NodeTrend {
	out := make([]NodeTrend, len(ts))
	for i := range ts {
		t := &ts[i]
		out[i] = NodeTrend{float32(t.in_lat_dev), float32(t.in_err_dev), float32(t.out_lat_dev), float32(t.out_err_dev),
			float32(t.in_base_mean_us), float32(t.out_base_mean_us), uint32(t.in_seen), uint32(t.out_seen)}
	}
	return out
}

func goEdgeTrends(ts []C.sg_edge_trend) []EdgeTrend {
	out := make([]EdgeTrend, len(ts))
	for i := range ts {
		out[i] = EdgeTrend{float32(ts[i].lat_dev), float32(ts[i].err_dev), float32(ts[i].base_mean_us), uint32(ts[i].windows_seen)}
	}
	return out
}

// WindowTrafficShifts answers "which workloads' traffic left its own normal band" for the window FlushWindow returned last, on the
// device (sg_window_group_nodes_top_traffic): the k workload rows with the highest signed value >= minValue of key by — a
// direction ORed with a side: TrafficDrop | TrafficIn ranks the workloads whose inbound request rate fell furthest — descending,
// with their traffic rows (sg_window_group_node_traffic at the selected indices: InLatDev is the rate deviation, InErrDev the load
// deviation, InBaseMeanUs the baseline rate in requests per window) and their indices into WindowWorkloadNodes.  k = 0: every
// such row, in order.  It needs SetTrafficTrend over TrafficWorkloads.
func (g *GraphDS) WindowTrafficShifts(by, k uint32, minValue float32) ([]WorkloadNode, []NodeTrend, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_group_nodes_top_traffic(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil, nil
	}
	ns, index := make([]C.sg_node_out, room), make([]uint32, room)
	if rc := C.sg_window_group_nodes_top_traffic(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), &ns[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, index = ns[:int(sel)], index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil, nil
	}
	var n C.size_t
	ts := make([]C.sg_node_trend, len(index))
	if rc := C.sg_window_group_node_traffic(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_node_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return goWorkloadNodes(ns), goNodeTrends(ts), index, nil
}

// WindowWorkloadEdgeTrafficShifts is WindowTrafficShifts over the workload edges (sg_window_groups_top_traffic; by is a direction
// alone: an edge has one side): the selected group edges, their traffic rows (sg_window_group_traffic) and their indices into
// WindowGroupEdges.  It needs SetTrafficTrend over TrafficWorkEdges.
func (g *GraphDS) WindowWorkloadEdgeTrafficShifts(by, k uint32, minValue float32) ([]GroupEdge, []EdgeTrend, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_groups_top_traffic(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_groups_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil, nil
	}
	ges, index := make([]C.sg_group_edge, room), make([]uint32, room)
	if rc := C.sg_window_groups_top_traffic(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), &ges[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_groups_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ges, index = ges[:int(sel)], index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil, nil
	}
	var n C.size_t
	ts := make([]C.sg_edge_trend, len(index))
	if rc := C.sg_window_group_traffic(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return goGroupEdges(ges), goEdgeTrends(ts), index, nil
}

// WindowServiceTrafficTop selects the services of the window FlushWindow returned last by a traffic key (sg_window_nodes_top_traffic;
// by as WindowTrafficShifts takes it): the indices of the selected node rows and their traffic rows (sg_window_node_traffic).  It
// needs SetTrafficTrend over TrafficNodes.
func (g *GraphDS) WindowServiceTrafficTop(by, k uint32, minValue float32) ([]NodeTrend, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_nodes_top_traffic(g.h, C.uint32_t(by), 0, C.float(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, fmt.Errorf("servicegraph: sg_window_nodes_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil
	}
	index := make([]uint32, room)
	if rc := C.sg_window_nodes_top_traffic(g.h, C.uint32_t(by), C.uint32_t(k), C.float(minValue), nil, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, fmt.Errorf("servicegraph: sg_window_nodes_top_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		index = index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil
	}
	var n C.size_t
	ts := make([]C.sg_node_trend, len(index))
	if rc := C.sg_window_node_traffic(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, nil, fmt.Errorf("servicegraph: sg_window_node_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return goNodeTrends(ts), index, nil
}

// WindowEdgeTraffic returns the traffic rows of the edge rows at index (the row indices another selection gave; the pod-edge space
// has no selection of its own) of the window FlushWindow returned last (sg_window_traffic).  It needs SetTrafficTrend over
// TrafficEdges.
func (g *GraphDS) WindowEdgeTraffic(index []uint32) ([]EdgeTrend, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if len(index) == 0 {
		return nil, nil
	}
	var n C.size_t
	ts := make([]C.sg_edge_trend, len(index))
	if rc := C.sg_window_traffic(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), &ts[0], C.size_t(len(ts)), &n); rc != 0 {
		return nil, fmt.Errorf("servicegraph: sg_window_traffic = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return goEdgeTrends(ts), nil
}

// TrafficTrendStats returns the running statistics of the traffic baseline of one space (a Traffic* constant) and the number of
// entries it holds (sg_traffic_trend_stats_get, sg_traffic_trend_entries).
func (g *GraphDS) TrafficTrendStats(space uint32) (TrafficStats, int, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var tst C.sg_trend_stats
	if rc := C.sg_traffic_trend_stats_get(g.h, C.uint32_t(space), &tst); rc != 0 {
		return TrafficStats{}, 0, fmt.Errorf("servicegraph: sg_traffic_trend_stats_get = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	var n C.size_t
	if rc := C.sg_traffic_trend_entries(g.h, C.uint32_t(space), nil, 0, &n); rc != 0 {
		return TrafficStats{}, 0, fmt.Errorf("servicegraph: sg_traffic_trend_entries = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return TrafficStats{uint64(tst.windows), uint64(tst.entries), uint64(tst.inserted), uint64(tst.expired), uint64(tst.dropped)}, int(n), nil
}

// WindowTrafficBuffer returns the device address of the traffic rows of one space of the window that ran last
// (sg_window_traffic_buffer), for a consumer that reads them on the device.
func (g *GraphDS) WindowTrafficBuffer(space uint32) (uintptr, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var p unsafe.Pointer
	if rc := C.sg_window_traffic_buffer(g.h, C.uint32_t(space), &p); rc != 0 {
		return 0, fmt.Errorf("servicegraph: sg_window_traffic_buffer = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return uintptr(p), nil
}

// Run closes a window every `every` until ctx is done and hands its rows to sink (e.g. a POST of the /edges/ payload of
// INTEGRATION.md §4 through the inner store's HTTP client).
func (g *GraphDS) Run(ctx context.Context, every time.Duration, sink func(windowEndMs int64, rows []EdgeRow)) {
	t := time.NewTicker(every)
	defer t.Stop()
	for {
		select {
		case <-ctx.Done():
			return
		case now := <-t.C:
			ms := now.UnixMilli()
			if rows, err := g.FlushWindow(ms); err == nil && sink != nil {
				sink(ms, rows)
			} else if err != nil {
				g.EngineErrors.Add(1)
			}
		}
	}
}

// ---- SLO burn rates (K24) ---------------------------------------------------------------------------------------------

// SLO spaces, selection keys and row flags of include/servicegraph.h ("SLO burn rates").
const (
	SLOServices  = uint32(C.SG_Q_NODES)
	SLOWorkloads = uint32(C.SG_Q_GROUP_NODES)
	SLOErr       = uint32(C.SG_SLOSEL_ERR)
	SLOSlow      = uint32(C.SG_SLOSEL_SLOW)
	SLOIn        = uint32(C.SG_SLOSEL_IN)
	SLOOut       = uint32(C.SG_SLOSEL_OUT)
	SLOUntracked = uint64(C.SG_SLO_UNTRACKED)
	sloWords     = int(C.SG_SLO_WORDS)
)

// SLOParams is sg_slo_params: a request is slow when its latency bin is above LatencyBin (duration >= 2^(17 + LatencyBin) ns); the
// targets are in ppm (990000 = 99 %); a kind burns when its burn over the last ShortWindows and over the last LongWindows windows
// are both >= MinBurnQ10 (1/1024 of "exactly on budget": 14746 = 14.4 x) and the long span holds MinRequests requests.
type SLOParams struct {
	LatencyBin, LatencyTargetPpm, ErrorTargetPpm, ShortWindows, LongWindows, MinBurnQ10 uint32
	MinRequests                                                                           uint64
}

// SLOSide is one side of an SLO row: the exact sums of requests, errors and slow requests over the short and the long span, and
// the four burn rates in 1/1024 of "exactly on budget".
type SLOSide struct {
	TotalShort, ErrShort, SlowShort, TotalLong, ErrLong, SlowLong uint64
	BurnErrShort, BurnErrLong, BurnSlowShort, BurnSlowLong        uint32
}

// SLORow is sg_window_group_node_slo's row of one workload row: the calls it receives (In), the calls it makes (Out), the flags
// (SLOUntracked, then err / slow burning per side), the objective word it was judged by (0: the defaults) and the windows each
// span covers.
type SLORow struct {
	In, Out                   SLOSide
	Flags, Objective          uint32
	ShortCovers, LongCovers   uint32
}

// SetSLO switches the SLO stage on for the spaces given (SLOServices needs SetLatencyQuantiles over the services, SLOWorkloads over
// the workloads): per service and workload key the exact sums of the last ShortWindows and LongWindows windows and their burn
// rates against an absolute objective.  State belongs to the key, so a workload keeps its sums through a rollout.  Every call
// starts empty state; the ring is LongWindows x keys x 48 bytes.
func (g *GraphDS) SetSLO(spaces uint32, p SLOParams) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sp C.sg_slo_params
	sp.struct_size = C.uint32_t(unsafe.Sizeof(sp))
	sp.latency_bin, sp.latency_target_ppm, sp.error_target_ppm = C.uint32_t(p.LatencyBin), C.uint32_t(p.LatencyTargetPpm), C.uint32_t(p.ErrorTargetPpm)
	sp.short_windows, sp.long_windows, sp.min_burn_q10 = C.uint32_t(p.ShortWindows), C.uint32_t(p.LongWindows), C.uint32_t(p.MinBurnQ10)
	sp.min_requests = C.uint64_t(p.MinRequests)
	if rc := C.sg_set_slo(g.h, C.uint32_t(spaces), &sp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_slo = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// ClearSLO switches the SLO stage off and frees it.
func (g *GraphDS) ClearSLO() error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_slo(g.h, 0, nil); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_slo = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// SLOObjective packs an objective word (SG_SLO_OBJECTIVE): a latency bin (0 .. 14) and the two budgets as mant x 10^exp ppm, mant
// 1 .. 1000, exp 0 .. 3.  99.9 % is a budget of 1000 ppm: (1, 3), (10, 2), (100, 1) or (1000, 0).
func SLOObjective(latencyBin, latMant, latExp, errMant, errExp uint32) uint32 {
	return latencyBin<<28 | (latExp<<10|latMant)<<12 | (errExp<<10 | errMant)
}

// SetWorkloadObjective sets the objective word (SLOObjective; 0: the defaults of SetSLO) of the workload with this group id, the
// id AssignGroups was told.  It takes effect with the next window; history is not rewritten, the sums are counts.
func (g *GraphDS) SetWorkloadObjective(group, objective uint32) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	ref := C.uint32_t(uint32(C.SG_REF_GROUP)<<30 | group&0x3FFFFFFF)
	obj := C.uint32_t(objective)
	if rc := C.sg_slo_assign(g.h, C.SG_Q_GROUP_NODES, &ref, &obj, 1); rc != 0 {
		return fmt.Errorf("servicegraph: sg_slo_assign = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func goSLOSide(w []uint64) SLOSide {
	return SLOSide{w[0], w[1], w[2], w[3], w[4], w[5], uint32(w[6]), uint32(w[6] >> 32), uint32(w[7]), uint32(w[7] >> 32)}
}

// WindowSLOBurn selects the workloads of the window FlushWindow returned last by a burn rate (sg_window_group_nodes_top_slo): by is
// SLOErr or SLOSlow ORed with SLOIn or SLOOut, a row's value min(short burn, long burn), 0 below MinRequests; the k largest values
// >= minValueQ10, descending, with their SLO rows (sg_window_group_node_slo at the selected indices) and their indices into
// WindowWorkloadNodes.  k = 0: every such row, in order.  WindowSLOBurn(SLOErr|SLOIn, 20, 1024) is "the 20 workloads burning
// their error budget fastest".  It needs SetSLO over SLOWorkloads.
func (g *GraphDS) WindowSLOBurn(by, k, minValueQ10 uint32) ([]WorkloadNode, []SLORow, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_group_nodes_top_slo(g.h, C.uint32_t(by), 0, C.uint32_t(minValueQ10), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_slo = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil, nil
	}
	ns, index := make([]C.sg_node_out, room), make([]uint32, room)
	if rc := C.sg_window_group_nodes_top_slo(g.h, C.uint32_t(by), C.uint32_t(k), C.uint32_t(minValueQ10), &ns[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_nodes_top_slo = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, index = ns[:int(sel)], index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil, nil
	}
	var n C.size_t
	words := make([]uint64, len(index)*sloWords)
	if rc := C.sg_window_group_node_slo(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), (*C.uint64_t)(unsafe.Pointer(&words[0])), C.size_t(len(index)), &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_group_node_slo = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	rows := make([]SLORow, len(index))
	for i := range rows {
		w := words[i*sloWords : (i+1)*sloWords]
		rows[i] = SLORow{goSLOSide(w[0:8]), goSLOSide(w[8:16]), uint32(w[16]), uint32(w[16] >> 32), uint32(w[17]), uint32(w[17] >> 32)}
	}
	return goWorkloadNodes(ns), rows, index, nil
}

// ---- replica outliers (K25) -------------------------------------------------------------------------------------------

// Selection keys and row flags of include/servicegraph.h ("replica outliers").
const (
	ReplicaErr      = uint32(C.SG_RSEL_ERR)
	ReplicaLat      = uint32(C.SG_RSEL_LAT)
	ReplicaTail     = uint32(C.SG_RSEL_TAIL)
	ReplicaShare    = uint32(C.SG_RSEL_SHARE)
	ReplicaIn       = uint32(C.SG_RSEL_IN)
	ReplicaOut      = uint32(C.SG_RSEL_OUT)
	ReplicaMember   = uint32(C.SG_REPL_MEMBER)
	ReplicaJudged   = uint32(C.SG_REPL_JUDGED_IN) // a side's flags: Judged, ErrFlag, LatFlag, TailFlag; << 4 for the out side
	ReplicaErrFlag  = uint32(C.SG_REPL_ERR_IN)
	ReplicaLatFlag  = uint32(C.SG_REPL_LAT_IN)
	ReplicaTailFlag = uint32(C.SG_REPL_TAIL_IN)
	replicaWords    = int(C.SG_REPLICA_WORDS)
)

// ReplicaParams is sg_replica_params; a zero is the engine's default: a side is judged with MinReplicas (3) active replicas and
// MinRequests (20) requests on the pod and on its peers; it is an outlier from MinErrExcessQ20 (20972: two points of error rate),
// MinLatRatioQ10 (2048: twice the peers' mean) or, with TailPermille set, MinTailBins (2) octaves of that percentile.
type ReplicaParams struct {
	MinReplicas                                                 uint32
	MinRequests                                                 uint64
	MinErrExcessQ20, MinLatRatioQ10, TailPermille, MinTailBins uint32
}

// ReplicaSide is one side of a pod row: the error rate above the peers' (2^20 = 100 points), the mean latency over the peers'
// mean and the share of the fair share (1024 = 1), the percentile's K20 bin of the pod and of its peers, and the active replicas.
type ReplicaSide struct {
	ErrExcessQ20          int32
	LatRatioQ10, ShareQ10 uint32
	TailPod, TailPeers    uint32
	Replicas              uint32
}

// ReplicaRow is sg_window_replicas' row of one node row: the workload row it is a member of, the flags, the calls it receives
// (In) and the calls it makes (Out).
type ReplicaRow struct {
	Workload, Flags uint32
	In, Out         ReplicaSide
}

// SetReplicaOutliers switches the replica stage on: each pod of a workload against the leave-one-out remainder of its siblings, per
// window and without state.  It needs the node rollup, AssignGroups' map and the workload rows, and with TailPermille the latency
// quantiles over the services.
func (g *GraphDS) SetReplicaOutliers(p ReplicaParams) error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sp C.sg_replica_params
	sp.struct_size = C.uint32_t(unsafe.Sizeof(sp))
	sp.min_replicas, sp.min_requests = C.uint32_t(p.MinReplicas), C.uint64_t(p.MinRequests)
	sp.min_err_excess_q20, sp.min_lat_ratio_q10 = C.uint32_t(p.MinErrExcessQ20), C.uint32_t(p.MinLatRatioQ10)
	sp.tail_permille, sp.min_tail_bins = C.uint32_t(p.TailPermille), C.uint32_t(p.MinTailBins)
	if rc := C.sg_set_replicas(g.h, &sp); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_replicas = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

// ClearReplicaOutliers switches the replica stage off and frees it.
func (g *GraphDS) ClearReplicaOutliers() error {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	if rc := C.sg_set_replicas(g.h, nil); rc != 0 {
		return fmt.Errorf("servicegraph: sg_set_replicas = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	return nil
}

func goReplicaSide(w []uint32) ReplicaSide {
	return ReplicaSide{int32(w[0]), w[1], w[2], w[3] & 255, w[3] >> 8 & 255, w[4]}
}

// WindowReplicaOutliers selects the pods of the window FlushWindow returned last by a replica value (sg_window_replicas_top): by is
// ReplicaErr, ReplicaLat, ReplicaTail or ReplicaShare ORed with ReplicaIn or ReplicaOut; the k largest values >= minValue of
// judged sides, descending, with their pod rows (sg_window_replicas at the selected indices) and their indices into the node
// rows.  k = 0: every such pod, in order.  WindowReplicaOutliers(ReplicaErr|ReplicaIn, 20, 1) is "the 20 replicas furthest above
// their peers' error rate".  The first result holds NODE rows, one per selected pod: sg_node_out is the row type of the node rows and
// of the workload rows alike, and WorkloadNode is this package's one Go form of it; Ref is the pod's KNOWN ref here, not a group's.
func (g *GraphDS) WindowReplicaOutliers(by, k, minValue uint32) ([]WorkloadNode, []ReplicaRow, []uint32, error) {
	g.flushMu.Lock()
	defer g.flushMu.Unlock()
	var sel, total C.size_t
	room := int(k)
	if k == 0 { // the count first
		if rc := C.sg_window_replicas_top(g.h, C.uint32_t(by), 0, C.uint32_t(minValue), nil, nil, 0, &sel, &total); rc != 0 {
			return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_replicas_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
		}
		room = int(sel)
	}
	if room == 0 {
		return nil, nil, nil, nil
	}
	ns, index := make([]C.sg_node_out, room), make([]uint32, room)
	if rc := C.sg_window_replicas_top(g.h, C.uint32_t(by), C.uint32_t(k), C.uint32_t(minValue), &ns[0], (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(room), &sel, &total); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_replicas_top = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	if int(sel) < room {
		ns, index = ns[:int(sel)], index[:int(sel)]
	}
	if len(index) == 0 {
		return nil, nil, nil, nil
	}
	var n C.size_t
	words := make([]uint32, len(index)*replicaWords)
	if rc := C.sg_window_replicas(g.h, (*C.uint32_t)(unsafe.Pointer(&index[0])), C.size_t(len(index)), (*C.uint32_t)(unsafe.Pointer(&words[0])), C.size_t(len(index)), &n); rc != 0 {
		return nil, nil, nil, fmt.Errorf("servicegraph: sg_window_replicas = %d: %s", int(rc), C.GoString(C.sg_last_error(g.h)))
	}
	pods := make([]ReplicaRow, len(index))
	for i := range pods {
		w := words[i*replicaWords : (i+1)*replicaWords]
		pods[i] = ReplicaRow{w[0], w[1], goReplicaSide(w[2:7]), goReplicaSide(w[7:12])}
	}
	return goWorkloadNodes(ns), pods, index, nil
}
