// Package hip binds libplacement, the MI355X gang-placement engine (include/placement.h), for the
// training operator.  Mechanically thin on purpose: one Go method per C entry point, Go slices
// pinned for the duration of the call and never retained by C, every non-zero return code turned
// into an error carrying pe_last_error.
//
// This file is the reference-side binding a maintainer adds as pkg/placement/hip.  There is no Go
// toolchain in the build pipeline that produced it (SURVEY.md sec. 0.3), so it is not compiled
// there; tests/test_go_binding.py checks that it calls every pe_* function of the header with the
// header's arity.
//
// Reference interfaces it serves (paths relative to the training-operator repo):
//
//	PGMinResources(ModeV1, ...)  pkg/controller.v1/common/util.go:108 CalcPGMinResources
//	PGMinResources(ModeV2, ...)  pkg/runtime.v2/framework/plugins/coscheduling/coscheduling.go:103-118 Build
//	New / Close                   the plugin instance lifetime, pkg/runtime.v2/framework/plugins/registry.go:32-42
package hip

/*
#cgo LDFLAGS: -lplacement
#include <stdlib.h>
#include "placement.h"

// The Go side cannot hand a Go func to C as a pe_allgather_fn; sharded contexts use RCCL
// (comm_id), which needs no callback, or the library's own shared-memory all-gather (HostExchange).
static pe_allgather_fn hx_allgather_fn(void) { return pe_host_exchange_allgather; }
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	corev1 "k8s.io/api/core/v1"
)

// Aggregation modes (PE_MODE_*).
const (
	ModeV1 = int(C.PE_MODE_V1) // CalcPGMinResources: priority order, pods counted up to minMember
	ModeV2 = int(C.PE_MODE_V2) // CoScheduling.Build: sum of Replicas x PodRequests
)

// Container record kinds (cont_flags bits 4-5) and the presence bits (0-3) of pe_pg_min_resources.
const (
	KindContainer = uint8(C.PE_KIND_CONTAINER)
	KindInit      = uint8(C.PE_KIND_INIT)
	KindSidecar   = uint8(C.PE_KIND_SIDECAR)
	KindOverhead  = uint8(C.PE_KIND_OVERHEAD)
	KindShift     = uint(C.PE_KIND_SHIFT)
)

// Job status of PlaceGreedy.
const (
	JobPlaced        = int32(C.PE_JOB_PLACED)
	JobUnschedulable = int32(C.PE_JOB_UNSCHEDULABLE)
	// LabelIsland is node label bit 31 (set by the engine when island >= 0); a greedy group whose
	// need carries NeedIsland is placed as one unit on one island node (placement.h).
	LabelIsland = uint32(C.PE_LABEL_ISLAND)
	NeedIsland  = uint32(C.PE_NEED_ISLAND)
	// CapMax is where GangCapacity's per-node capacity saturates.
	CapMax = int32(C.PE_CAP_MAX)
	// MaxDomains bounds GangCapacityDomains' nDomains.
	MaxDomains = int32(C.PE_MAX_DOMAINS)
	// MaxLevels bounds GangCapacityTree's levels.
	MaxLevels = int32(C.PE_MAX_LEVELS)
)

// Node inventory update ops.
const (
	NodeSet    = uint8(C.PE_NODE_SET)
	NodeRemove = uint8(C.PE_NODE_REMOVE)
)

// Device mask layouts (FitMaskLayout).
const (
	MaskNodeTiles  = int32(C.PE_MASK_NODE_TILES)
	MaskJobBits    = int32(C.PE_MASK_JOB_BITS)
	MaskNodeBlocks = int32(C.PE_MASK_NODE_BLOCKS)
	MaskRows       = int32(C.PE_MASK_ROWS)
)

// Dims is the number of engine resource dimensions: cpu (milli), memory (B), the accelerator
// resource named in Config.GPUResourceName (count), ephemeral-storage (B).
const Dims = int(C.PE_DIMS)

// CommIDBytes is the size of an RCCL unique id (CommID).
const CommIDBytes = int(C.PE_COMM_ID_BYTES)

// ErrOverflow: an aggregation overflowed int64 -- the reference's resource.Quantity would have
// switched to inf.Dec.  The per-job Overflow flags say which job; the caller takes the exact
// reference path for those jobs.
var ErrOverflow = errors.New("placement: int64 overflow (reference would switch to inf.Dec)")

// ErrNoDevice: no usable GPU.  The engine has no CPU fallback.
var ErrNoDevice = errors.New("placement: no usable GPU")

// Config mirrors pe_config.  Zero values take the engine defaults.
type Config struct {
	DeviceID        int32  // HIP ordinal; -1 = the calling thread's current device
	Rank, WorldSize int32  // inventory shard of this process (WorldSize 0 = 1)
	CommID          []byte // CommIDBytes from CommID() on rank 0 (RCCL), for WorldSize > 1
	MaxNodes        int64
	GPUResourceName string // dim 2's resource key, e.g. "amd.com/gpu"
	TopK            int32
	WindowGroups    int32
	WindowPods      int64
	FitPathMask     int32
	GreedyFlags     int32
	ResortNodes     int32
	// HostExchange replaces RCCL for ranks of one node (e.g. when the communicator set-up failed on
	// some rank: PE_ERCCL there means every rank drops its engine and creates a new one).
	HostExchange *HostExchange
}

// HostExchange is pe_host_exchange: an all-gather through a POSIX shared-memory segment, for the
// ranks of one node.  Every rank opens the same name ("/..."); rank 0 creates the segment.
type HostExchange struct {
	h    *C.pe_host_exchange
	rank int32
	size int32
}

// OpenHostExchange opens (rank 0: creates) the segment; maxBytes bounds one rank's block per call
// (WindowGroups x (16 + 8 x TopK) for the greedy windows).  Passed as Config.HostExchange, the
// library recognises its own exchange and runs the greedy windows zero-copy: each rank's walk writes
// into the segment and an exchange thread merges every group on the host (Stats.xchg_zc_windows).
func OpenHostExchange(name string, rank, world int32, maxBytes int) (*HostExchange, error) {
	cn := C.CString(name)
	defer C.free(unsafe.Pointer(cn))
	x := &HostExchange{rank: rank, size: world}
	if rc := C.pe_host_exchange_open(cn, C.int32_t(rank), C.int32_t(world), C.size_t(maxBytes), &x.h); rc != C.PE_OK {
		return nil, fmt.Errorf("placement: pe_host_exchange_open: %d", int(rc))
	}
	runtime.SetFinalizer(x, (*HostExchange).Close)
	return x, nil
}

// Allgather gathers every rank's send block into recv (world x len(send) bytes, rank order).
func (x *HostExchange) Allgather(send, recv []byte) error {
	if len(recv) < int(x.size)*len(send) {
		return errors.New("placement: HostExchange.Allgather: recv too small")
	}
	var sp, rp unsafe.Pointer
	if len(send) > 0 {
		sp, rp = unsafe.Pointer(&send[0]), unsafe.Pointer(&recv[0])
	}
	if rc := C.pe_host_exchange_allgather(unsafe.Pointer(x.h), sp, rp, C.size_t(len(send))); rc != C.PE_OK {
		return fmt.Errorf("placement: pe_host_exchange_allgather: %d", int(rc))
	}
	runtime.KeepAlive(x) // the finalizer must not unmap the segment during the call
	return nil
}

// Close unmaps the segment.  Idempotent; the engines using it must be closed first.
func (x *HostExchange) Close() {
	if x.h != nil {
		C.pe_host_exchange_close(x.h)
		x.h = nil
	}
}

// Engine is one pe_ctx: a GPU, an inventory shard, a stream.  Safe for concurrent use (the
// context holds a mutex and selects its device on every call).
type Engine struct {
	ctx  *C.pe_ctx
	name *C.char
	// hx keeps the HostExchange the context was created with reachable for the context's lifetime:
	// its walks and exchange thread use the mapped segment, which HostExchange's finalizer unmaps.
	hx *HostExchange
}

// Stats mirrors pe_stats.
type Stats = C.pe_stats

func ptr64(s []int64) *C.int64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int64_t)(unsafe.Pointer(&s[0]))
}

func ptr32(s []int32) *C.int32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.int32_t)(unsafe.Pointer(&s[0]))
}

func ptru32(s []uint32) *C.uint32_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint32_t)(unsafe.Pointer(&s[0]))
}

func ptr8(s []uint8) *C.uint8_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&s[0]))
}

func ptru64(s []uint64) *C.uint64_t {
	if len(s) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&s[0]))
}

// ABIVersion is PE_ABI_VERSION of the loaded library.
func ABIVersion() int { return int(C.pe_abi_version()) }

// CommID makes an RCCL unique id (rank 0; broadcast the bytes to every rank).
func CommID() ([]byte, error) {
	buf := make([]byte, CommIDBytes)
	if rc := C.pe_comm_id((*C.uint8_t)(unsafe.Pointer(&buf[0]))); rc != C.PE_OK {
		return nil, fmt.Errorf("placement: pe_comm_id: %d", int(rc))
	}
	return buf, nil
}

// New creates an engine context (pe_create).
func New(cfg Config) (*Engine, error) {
	e := &Engine{name: C.CString(cfg.GPUResourceName)}
	var c C.pe_config
	c.device_id = C.int32_t(cfg.DeviceID)
	c.rank = C.int32_t(cfg.Rank)
	c.world_size = C.int32_t(cfg.WorldSize)
	if c.world_size == 0 {
		c.world_size = 1
	}
	var id unsafe.Pointer
	if len(cfg.CommID) > 0 {
		if len(cfg.CommID) != CommIDBytes {
			C.free(unsafe.Pointer(e.name))
			return nil, fmt.Errorf("placement: comm id must be %d bytes", CommIDBytes)
		}
		id = C.CBytes(cfg.CommID)
		defer C.free(id)
		c.comm_id = (*C.uint8_t)(id)
	}
	c.max_nodes = C.int64_t(cfg.MaxNodes)
	c.gpu_resource_name = e.name
	c.topk = C.int32_t(cfg.TopK)
	c.window_groups = C.int32_t(cfg.WindowGroups)
	c.window_pods = C.int64_t(cfg.WindowPods)
	c.fit_path_mask = C.int32_t(cfg.FitPathMask)
	c.greedy_flags = C.int32_t(cfg.GreedyFlags)
	c.resort_nodes = C.int32_t(cfg.ResortNodes)
	if cfg.HostExchange != nil {
		c.exchange = C.hx_allgather_fn()
		c.exchange_user = unsafe.Pointer(cfg.HostExchange.h)
		e.hx = cfg.HostExchange
	}
	rc := C.pe_create(&c, &e.ctx)
	if rc != C.PE_OK {
		C.free(unsafe.Pointer(e.name))
		if rc == C.PE_ENODEV {
			return nil, ErrNoDevice
		}
		return nil, fmt.Errorf("placement: pe_create: %d", int(rc))
	}
	runtime.SetFinalizer(e, (*Engine).Close)
	return e, nil
}

// Close releases the context (pe_destroy).  Idempotent.
func (e *Engine) Close() {
	if e.ctx != nil {
		C.pe_destroy(e.ctx)
		e.ctx = nil
		C.free(unsafe.Pointer(e.name))
		e.hx = nil // the segment may be unmapped now (the caller's Close, or its finalizer)
	}
}

func (e *Engine) err(rc C.int, what string) error {
	switch rc {
	case C.PE_OK:
		return nil
	case C.PE_EOVERFLOW:
		return ErrOverflow
	case C.PE_ENODEV:
		return ErrNoDevice
	}
	return fmt.Errorf("placement: %s: %d: %s", what, int(rc), C.GoString(C.pe_last_error(e.ctx)))
}

// LoadNodes loads the GLOBAL inventory (SoA [4][n]: row d = dim d); the context keeps its shard.
func (e *Engine) LoadNodes(n int64, capacity, used []int64, labels []uint32, island []int32) error {
	if int64(len(capacity)) < int64(Dims)*n || int64(len(used)) < int64(Dims)*n {
		return fmt.Errorf("placement: LoadNodes: cap/used need %d values", int64(Dims)*n)
	}
	return e.err(C.pe_load_nodes(e.ctx, C.int64_t(n), ptr64(capacity), ptr64(used), ptru32(labels), ptr32(island)),
		"pe_load_nodes")
}

// ResetResiduals restores residual := cap - used on the device.
func (e *Engine) ResetResiduals() error { return e.err(C.pe_reset_residuals(e.ctx), "pe_reset_residuals") }

// UpdateNodes applies Node informer events: per entry NodeSet (cap/used [n][4], labels, island
// replace the slot) or NodeRemove.  Validated as a whole before anything changes.
func (e *Engine) UpdateNodes(slots []int64, ops []uint8, capacity, used []int64, labels []uint32, island []int32) error {
	if len(ops) != len(slots) {
		return errors.New("placement: UpdateNodes: one op per slot")
	}
	return e.err(C.pe_update_nodes(e.ctx, C.int64_t(len(slots)), ptr64(slots), ptr8(ops), ptr64(capacity), ptr64(used),
		ptru32(labels), ptr32(island)), "pe_update_nodes")
}

// ShardRange is this context's node range [begin, end).
func (e *Engine) ShardRange() (begin, end int64, err error) {
	var b, en C.int64_t
	if rc := C.pe_shard_range(e.ctx, &b, &en); rc != C.PE_OK {
		return 0, 0, e.err(rc, "pe_shard_range")
	}
	return int64(b), int64(en), nil
}

// CommRanks is the RCCL communicator size (0 without one).
func (e *Engine) CommRanks() (int32, error) {
	var n C.int32_t
	if rc := C.pe_comm_ranks(e.ctx, &n); rc != C.PE_OK {
		return 0, e.err(rc, "pe_comm_ranks")
	}
	return int32(n), nil
}

// ReadResiduals copies this shard's residuals ([4][end-begin]).
func (e *Engine) ReadResiduals() ([]int64, error) {
	b, en, err := e.ShardRange()
	if err != nil {
		return nil, err
	}
	out := make([]int64, int64(Dims)*(en-b))
	return out, e.err(C.pe_read_residuals(e.ctx, ptr64(out)), "pe_read_residuals")
}

// CSR is the flattened batch of pe_pg_min_resources (include/placement.h).
type CSR struct {
	JobGroupOff   []int32 // [J+1]
	MinMember     []int32 // [J] (v1)
	GroupReplicas []int32 // [G], -1 = nil (v1)
	GroupContOff  []int32 // [G+1]
	ContReq       []int64 // [C][4] canonical int64
	ContFlags     []uint8 // [C] presence bits 0-3 | kind << KindShift
}

// Agg holds the per-job results of PGMinResources.
type Agg struct {
	MinRes   []int64 // [J][4]
	Present  []uint8 // bit d = key d present (keys with value 0 included)
	Members  []int32
	Overflow []uint8 // 1 = int64 overflow: take the reference's exact path for this job
}

// PGMinResources aggregates a batch of PodGroups on the GPU.  Overflowed jobs are flagged, not an
// error: the batch's other jobs are exact.
func (e *Engine) PGMinResources(mode int, b *CSR) (*Agg, error) {
	J := len(b.JobGroupOff) - 1
	if J < 0 {
		return nil, errors.New("placement: JobGroupOff needs J+1 entries")
	}
	out := &Agg{make([]int64, Dims*J), make([]uint8, J), make([]int32, J), make([]uint8, J)}
	if J == 0 {
		return out, nil
	}
	rc := C.pe_pg_min_resources(e.ctx, C.int32_t(mode), C.int64_t(J), ptr32(b.JobGroupOff), ptr32(b.MinMember),
		ptr32(b.GroupReplicas), ptr32(b.GroupContOff), ptr64(b.ContReq), ptr8(b.ContFlags), ptr64(out.MinRes),
		ptr8(out.Present), ptr32(out.Members), ptr8(out.Overflow))
	if rc == C.PE_EOVERFLOW {
		return out, nil
	}
	return out, e.err(rc, "pe_pg_min_resources")
}

// MaxKeys is PE_MAX_KEYS: the keys of one pe_pg_min_resources_keys call (a batch with more takes one
// call per slice of keys; keys never interact).
const MaxKeys = int(C.PE_MAX_KEYS)

// KeysKindShift is PE_KEYS_KIND_SHIFT: the kind bits of a key-table container flag word.
const KeysKindShift = uint(C.PE_KEYS_KIND_SHIFT)

// KeyAgg holds the per-job results of PGMinResourcesKeys over the batch's key table.
type KeyAgg struct {
	Keys     []corev1.ResourceName
	Scale    []int32 // per key: MinRes values are counts of 10^Scale
	MinRes   []int64 // [J][len(Keys)]
	Present  []bool  // [J][len(Keys)] (keys with value 0 included)
	Members  []int32
	Overflow []uint8 // 1 = a sum (or a value) with no int64 at its key's scale: the reference's inf.Dec case
}

// PGMinResourcesKeys aggregates a batch over its per-call key table (pe_pg_min_resources_keys): any
// resource key, each at the finest decimal scale its quantities need (KeyCSR.Scales), one engine call
// per slice of MaxKeys keys.  A value with no int64 at its key's scale flags its job like an
// overflowed sum; flagged jobs are the caller's to hand to the reference.  Every other outcome is
// exact; an engine error is returned.
func (e *Engine) PGMinResourcesKeys(mode int, b *KeyCSR) (*KeyAgg, error) {
	J := len(b.JobGroupOff) - 1
	if J < 0 {
		return nil, errors.New("placement: JobGroupOff needs J+1 entries")
	}
	nk := len(b.Keys)
	out := &KeyAgg{Keys: b.Keys, Scale: b.Scales(), MinRes: make([]int64, J*nk), Present: make([]bool, J*nk),
		Members: make([]int32, J), Overflow: make([]uint8, J)}
	if J == 0 {
		return out, nil
	}
	val, jobOvf := b.scaledValues(out.Scale)
	for j := 0; j < J; j++ {
		out.Overflow[j] = jobOvf[j]
	}
	nc := len(b.ContKind)
	flags := make([]uint32, nc)
	pres := make([]uint16, J)
	ovf := make([]uint8, J)
	for lo := 0; lo < nk || (lo == 0 && nk == 0); lo += MaxKeys {
		n := nk - lo
		if n > MaxKeys {
			n = MaxKeys
		}
		if n < 1 {
			n = 1 // no key at all: one empty key, for Members
		}
		req := make([]int64, nc*n)
		res := make([]int64, J*n)
		for c := 0; c < nc; c++ {
			f := uint32(b.ContKind[c]) << KeysKindShift
			for x := b.EntOff[c]; x < b.EntOff[c+1]; x++ {
				k := int(b.EntKey[x]) - lo
				if k < 0 || k >= n || lo+k >= nk {
					continue
				}
				req[c*n+k] = val[x]
				f |= 1 << uint(k)
			}
			flags[c] = f
		}
		rc := C.pe_pg_min_resources_keys(e.ctx, C.int32_t(mode), C.int64_t(J), C.int32_t(n), ptr32(b.JobGroupOff),
			ptr32(b.MinMember), ptr32(b.GroupReplicas), ptr32(b.GroupContOff), ptr64(req), ptru32(flags), ptr64(res),
			(*C.uint16_t)(unsafe.Pointer(&pres[0])), ptr32(out.Members), ptr8(ovf))
		if rc != C.PE_OK && rc != C.PE_EOVERFLOW {
			return nil, e.err(rc, "pe_pg_min_resources_keys")
		}
		for j := 0; j < J; j++ {
			out.Overflow[j] |= ovf[j]
			for k := 0; k < n && lo+k < nk; k++ {
				out.MinRes[j*nk+lo+k] = res[j*n+k]
				out.Present[j*nk+lo+k] = pres[j]>>uint(k)&1 != 0
			}
		}
		if nk == 0 {
			break
		}
	}
	return out, nil
}

// KeyAggWide is the result of PGMinResourcesWide: KeyAgg with every sum as a signed 128-bit integer.
type KeyAggWide struct {
	Keys     []corev1.ResourceName
	Scale    []int32  // per key: values are counts of 10^Scale
	Lo       []uint64 // [J][len(Keys)] low limb
	Hi       []int64  // [J][len(Keys)] high limb (two's complement: the sign extension when Overflow is 0)
	Present  []bool   // [J][len(Keys)] (keys with value 0 included)
	Members  []int32
	Overflow []uint8 // 0 = the int64 path answered, 1 = exact 128-bit value, 2 = no 128-bit answer (values 0)
}

// PGMinResourcesWide is PGMinResourcesKeys with an exact answer past int64 (pe_pg_min_resources_wide):
// a value with no int64 at its key's scale travels as two limbs, and a job whose sums leave int64 is
// summed by the engine's 128-bit kernel instead of being flagged for the reference.  Overflow[j] is 2
// only for a job with no 128-bit answer (or a value the engine does not take); that job's values are 0.
func (e *Engine) PGMinResourcesWide(mode int, b *KeyCSR) (*KeyAggWide, error) {
	J := len(b.JobGroupOff) - 1
	if J < 0 {
		return nil, errors.New("placement: JobGroupOff needs J+1 entries")
	}
	nk := len(b.Keys)
	out := &KeyAggWide{Keys: b.Keys, Scale: b.Scales(), Lo: make([]uint64, J*nk), Hi: make([]int64, J*nk),
		Present: make([]bool, J*nk), Members: make([]int32, J), Overflow: make([]uint8, J)}
	if J == 0 {
		return out, nil
	}
	vlo, vhi, jobBad, wide := b.scaledLimbs(out.Scale)
	nc := len(b.ContKind)
	flags := make([]uint32, nc)
	pres := make([]uint16, J)
	ovf := make([]uint8, J)
	for lo := 0; lo < nk || (lo == 0 && nk == 0); lo += MaxKeys {
		n := nk - lo
		if n > MaxKeys {
			n = MaxKeys
		}
		if n < 1 {
			n = 1 // no key at all: one empty key, for Members
		}
		reqLo := make([]uint64, nc*n)
		var reqHi []uint64 // stays nil (NULL) when every value of the batch is an int64
		if wide {
			reqHi = make([]uint64, nc*n)
		}
		resLo := make([]uint64, J*n)
		resHi := make([]int64, J*n)
		for c := 0; c < nc; c++ {
			f := uint32(b.ContKind[c]) << KeysKindShift
			for x := b.EntOff[c]; x < b.EntOff[c+1]; x++ {
				k := int(b.EntKey[x]) - lo
				if k < 0 || k >= n || lo+k >= nk {
					continue
				}
				reqLo[c*n+k] = vlo[x]
				if wide {
					reqHi[c*n+k] = vhi[x]
				}
				f |= 1 << uint(k)
			}
			flags[c] = f
		}
		rc := C.pe_pg_min_resources_wide(e.ctx, C.int32_t(mode), C.int64_t(J), C.int32_t(n), ptr32(b.JobGroupOff),
			ptr32(b.MinMember), ptr32(b.GroupReplicas), ptr32(b.GroupContOff), ptru64(reqLo), ptru64(reqHi), ptru32(flags),
			ptru64(resLo), ptr64(resHi), (*C.uint16_t)(unsafe.Pointer(&pres[0])), ptr32(out.Members), ptr8(ovf))
		if rc != C.PE_OK && rc != C.PE_EOVERFLOW {
			return nil, e.err(rc, "pe_pg_min_resources_wide")
		}
		for j := 0; j < J; j++ {
			if ovf[j] > out.Overflow[j] {
				out.Overflow[j] = ovf[j]
			}
			for k := 0; k < n && lo+k < nk; k++ {
				out.Lo[j*nk+lo+k] = resLo[j*n+k]
				out.Hi[j*nk+lo+k] = resHi[j*n+k]
				out.Present[j*nk+lo+k] = pres[j]>>uint(k)&1 != 0
			}
		}
		if nk == 0 {
			break
		}
	}
	for j := 0; j < J; j++ {
		if jobBad[j] != 0 {
			out.Overflow[j] = 2
		}
		if out.Overflow[j] == 2 { // no answer in one key slice: none for the job
			for k := 0; k < nk; k++ {
				out.Lo[j*nk+k], out.Hi[j*nk+k] = 0, 0
			}
		}
	}
	return out, nil
}

// FitMask evaluates every job against every node of the shard (device-resident mask); returns the
// per-job feasible counts of this shard and the mask's words per row.
func (e *Engine) FitMask(req []int64, need []uint32) (counts []int64, wordsPerRow int64, err error) {
	J := len(req) / Dims
	counts = make([]int64, J)
	var dev *C.uint64_t
	var wpr C.int64_t
	rc := C.pe_fit_mask(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr64(counts), &dev, &wpr)
	return counts, int64(wpr), e.err(rc, "pe_fit_mask")
}

// JobsUpload stages a fit batch on the device (plan + H2D); FitMaskRun evaluates it asynchronously;
// FitCounts synchronizes and returns the per-job counts.
func (e *Engine) JobsUpload(req []int64, need []uint32) error {
	return e.err(C.pe_jobs_upload(e.ctx, C.int64_t(len(req)/Dims), ptr64(req), ptru32(need)), "pe_jobs_upload")
}

func (e *Engine) FitMaskRun() error { return e.err(C.pe_fit_mask_run(e.ctx), "pe_fit_mask_run") }

func (e *Engine) FitCounts(nJobs int) ([]int64, error) {
	out := make([]int64, nJobs)
	return out, e.err(C.pe_fit_counts(e.ctx, ptr64(out)), "pe_fit_counts")
}

// FitMaskRows copies rows [row0, row0+nRows) of the mask, row-major [nRows][wordsPerRow].
func (e *Engine) FitMaskRows(row0, nRows, wordsPerRow int64) ([]uint64, error) {
	out := make([]uint64, nRows*wordsPerRow)
	return out, e.err(C.pe_fit_mask_rows(e.ctx, C.int64_t(row0), C.int64_t(nRows), ptru64(out)), "pe_fit_mask_rows")
}

// FitMaskLayout and FitMaskRowPitch describe the device mask (for callers that map it).
func (e *Engine) FitMaskLayout() (int32, error) {
	var l C.int32_t
	rc := C.pe_fit_mask_layout(e.ctx, &l)
	return int32(l), e.err(rc, "pe_fit_mask_layout")
}

func (e *Engine) FitMaskRowPitch() (int64, error) {
	var w C.int64_t
	rc := C.pe_fit_mask_row_pitch(e.ctx, &w)
	return int64(w), e.err(rc, "pe_fit_mask_row_pitch")
}

// GangCapacity answers, per job shape (req [J][4], need [J] or nil) and against the shard's current
// residuals, how many pods of that shape fit: slots = the sum over the nodes (a gang of identical pods
// fits iff its size <= slots), maxNode = the largest single node (an island gang, NeedIsland in need,
// fits iff its size <= maxNode), nodes = the nodes holding at least one (FitMask's count).  Read-only:
// residuals and the staged fit batch stay as they are.  Sharded: add slots and nodes over the shards,
// take the maximum of maxNode.
func (e *Engine) GangCapacity(req []int64, need []uint32) (slots []int64, maxNode []int32, nodes []int64, err error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, nil, nil, fmt.Errorf("GangCapacity: %d needs for %d jobs", len(need), J)
	}
	slots = make([]int64, J)
	maxNode = make([]int32, J)
	nodes = make([]int64, J)
	rc := C.pe_gang_capacity(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr64(slots), ptr32(maxNode), ptr64(nodes))
	return slots, maxNode, nodes, e.err(rc, "pe_gang_capacity")
}

// Signatures of FitExplain (PE_EXPLAIN_*).
const (
	ExplainBins   = 32 // one per 5-bit signature
	ExplainLabels = 4  // signature bit of the label test
	ExplainAny    = -1 // a jobDomain entry: the whole shard for that job
)

// ExplainNames are the resource names Message uses by default.
var ExplainNames = [Dims]string{"cpu", "memory", "amd.com/gpu", "ephemeral-storage"}

// FitExplanation is FitExplain's answer.
type FitExplanation struct {
	Hist []int64  // [J][32]: live nodes in job j's scope per signature (bit d: req_d > res_d, bit 4: labels)
	Near []uint64 // [J][4]: the smallest shortfall among the nodes failing on dimension d alone, 0 = none; nil if not asked for
}

// Message is job j's histogram in kube-scheduler's manner: "{fits}/{live} nodes are available: {c} Insufficient
// {name}, ..., {c} node(s) didn't match the required labels."  Reasons in the order cpu, memory, gpu, ephemeral,
// labels with inclusive counts; zero counts are left out; with no reason the text ends after "available.".
func (x *FitExplanation) Message(j int, names [Dims]string) string {
	h := x.Hist[j*ExplainBins : (j+1)*ExplainBins]
	var incl [5]int64
	var live int64
	for s, c := range h {
		live += c
		for r := 0; r < 5; r++ {
			if s>>r&1 == 1 {
				incl[r] += c
			}
		}
	}
	msg := fmt.Sprintf("%d/%d nodes are available", h[0], live)
	sep := ": "
	for d := 0; d < Dims; d++ {
		if incl[d] != 0 {
			msg += fmt.Sprintf("%s%d Insufficient %s", sep, incl[d], names[d])
			sep = ", "
		}
	}
	if incl[ExplainLabels] != 0 {
		msg += fmt.Sprintf("%s%d node(s) didn't match the required labels", sep, incl[ExplainLabels])
	}
	return msg + "."
}

// FitExplain answers why job j's shape (req [J][4], need [J] or nil) fits no node: per job the shard's live nodes
// counted by signature and, with near, per dimension the nearest miss.  jobDomain ([J] or nil = the whole shard;
// ExplainAny = the whole shard for that job) restricts job j to one domain of `level` in the hierarchy levelSize /
// parent, as for PlaceGreedyDomains.  Read-only.  Sharded: add the histograms over the shards and take the minimum
// of the non-zero near values.
func (e *Engine) FitExplain(req []int64, need []uint32, jobDomain []int32, level int32, levelSize, parent []int32, near bool) (*FitExplanation, error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, fmt.Errorf("FitExplain: %d needs for %d jobs", len(need), J)
	}
	if jobDomain != nil && len(jobDomain) != J {
		return nil, fmt.Errorf("FitExplain: %d domains for %d jobs", len(jobDomain), J)
	}
	out := &FitExplanation{Hist: make([]int64, J*ExplainBins)}
	if near {
		out.Near = make([]uint64, J*Dims)
	}
	rc := C.pe_fit_explain(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr32(jobDomain), C.int32_t(level), C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr64(out.Hist), ptru64(out.Near))
	return out, e.err(rc, "pe_fit_explain")
}

// DomainCapacity is GangCapacityDomains' answer; a part that was not asked for is nil.
type DomainCapacity struct {
	DomSlots    []int64 // [J][nDomains]: pods of job j's shape that domain k holds
	DomNodes    []int64 // [J][nDomains]: its nodes holding at least one
	Domain      []int32 // [J]: the domain with the smallest DomSlots >= count, ties to the smallest id; -1 = none
	DomainSlots []int64 // [J]: that domain's slots, 0 when none
	Feasible    []int32 // [J]: domains with DomSlots >= count
}

// GangCapacityDomains answers GangCapacity's question per topology domain: the domain of a node is its
// island id in [0, nDomains) as last given by LoadNodes / UpdateNodes; a node with another id, or a
// removed slot, counts nowhere.  tables asks for the [J][nDomains] tables.  With count ([J], each >= 1)
// the device also picks, per job, the best-fitting domain; with tables false only those J-sized
// answers cross.  count nil: no selection.  A sharded engine answers tables only (a domain may span
// shards: add the shards' tables, then select).  Read-only, like GangCapacity.
func (e *Engine) GangCapacityDomains(req []int64, need []uint32, count []int32, nDomains int32, tables bool) (*DomainCapacity, error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, fmt.Errorf("GangCapacityDomains: %d needs for %d jobs", len(need), J)
	}
	if count != nil && len(count) != J {
		return nil, fmt.Errorf("GangCapacityDomains: %d counts for %d jobs", len(count), J)
	}
	out := &DomainCapacity{}
	if tables && nDomains >= 1 && nDomains <= MaxDomains {
		out.DomSlots = make([]int64, J*int(nDomains))
		out.DomNodes = make([]int64, J*int(nDomains))
	}
	if count != nil {
		out.Domain = make([]int32, J)
		out.DomainSlots = make([]int64, J)
		out.Feasible = make([]int32, J)
	}
	rc := C.pe_gang_capacity_domains(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr32(count), C.int32_t(nDomains),
		ptr64(out.DomSlots), ptr64(out.DomNodes), ptr32(out.Domain), ptr64(out.DomainSlots), ptr32(out.Feasible))
	return out, e.err(rc, "pe_gang_capacity_domains")
}

// TreeCapacity is GangCapacityTree's answer; a part that was not asked for is nil.  T is the sum of the
// level sizes; the column of domain k of level l is the sum of the lower levels' sizes plus k.
type TreeCapacity struct {
	TreeSlots   []int64 // [J][T]: pods of job j's shape that each domain of each level holds
	TreeNodes   []int64 // [J][T]: its nodes holding at least one
	Level       []int32 // [J]: the lowest level <= maxLevel at which one domain holds the gang; -1 = none
	Domain      []int32 // [J]: that level's domain with the smallest slots >= count, ties to the smallest id; -1 = none
	DomainSlots []int64 // [J]: that domain's slots, 0 when none
	Feasible    []int32 // [J][nLevels]: domains of each level with slots >= count
}

// GangCapacityTree answers GangCapacityDomains' question over a hierarchy of topology levels (node -> rack
// -> block -> zone): levelSize[l] domains at level l, level 0 being the nodes' island ids, and
// parent[off_l+k] the level-(l+1) domain that holds domain k of level l, or -1 (nil allowed with one
// level).  tables asks for the [J][T] tables.  With count ([J], each >= 1) the device also picks, per
// job, the lowest level <= maxLevel[j] (nil: the top level) at which one domain holds the gang, and the
// best-fitting domain there; with tables false only those answers cross.  count nil: no selection.  A
// sharded engine answers tables only: add the shards' tables, then select.  Read-only, like GangCapacity.
func (e *Engine) GangCapacityTree(req []int64, need []uint32, count, maxLevel, levelSize, parent []int32, tables bool) (*TreeCapacity, error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, fmt.Errorf("GangCapacityTree: %d needs for %d jobs", len(need), J)
	}
	if count != nil && len(count) != J {
		return nil, fmt.Errorf("GangCapacityTree: %d counts for %d jobs", len(count), J)
	}
	if maxLevel != nil && (count == nil || len(maxLevel) != J) {
		return nil, fmt.Errorf("GangCapacityTree: %d max levels for %d jobs with a count", len(maxLevel), J)
	}
	L := len(levelSize)
	valid := L >= 1 && L <= int(MaxLevels)
	T := 0
	for _, s := range levelSize {
		valid = valid && s >= 1 && s <= MaxDomains
		T += int(s)
	}
	if valid && parent != nil && len(parent) != T-int(levelSize[L-1]) {
		return nil, fmt.Errorf("GangCapacityTree: %d parents for %d columns below the top level", len(parent), T-int(levelSize[L-1]))
	}
	out := &TreeCapacity{}
	if tables && valid {
		out.TreeSlots = make([]int64, J*T)
		out.TreeNodes = make([]int64, J*T)
	}
	if count != nil && valid {
		out.Level = make([]int32, J)
		out.Domain = make([]int32, J)
		out.DomainSlots = make([]int64, J)
		out.Feasible = make([]int32, J*L)
	}
	rc := C.pe_gang_capacity_tree(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr32(count), ptr32(maxLevel),
		C.int32_t(L), ptr32(levelSize), ptr32(parent), ptr64(out.TreeSlots), ptr64(out.TreeNodes), ptr32(out.Level),
		ptr32(out.Domain), ptr64(out.DomainSlots), ptr32(out.Feasible))
	return out, e.err(rc, "pe_gang_capacity_tree")
}

// TreeSplit is GangSplitTree's answer.
type TreeSplit struct {
	Level      []int32 // [J]: GangCapacityTree's level; -1 = none
	Domain     []int32 // [J]: GangCapacityTree's domain; -1 = none
	Parts      []int32 // [J]: number of (leaf, pods) parts; 0 = none selected, SplitTooMany
	PartDomain []int32 // [J][maxParts]: the parts' leaf ids in list order, the tail -1
	PartPods   []int32 // [J][maxParts]: their pods (>= 1, adding up to count), the tail 0
	Spread     []int32 // [J][nLevels]: domains of each level the gang touches, 0 above the level
}

const (
	// MaxSplitParts bounds GangSplitTree's maxParts.
	MaxSplitParts = int32(C.PE_MAX_SPLIT_PARTS)
	// SplitTooMany in Parts: the gang touches more than maxParts domains at some level.
	SplitTooMany = int32(C.PE_SPLIT_TOO_MANY)
)

// GangSplitTree is GangCapacityTree's selection followed, on the device, by the descent from the selected
// domain to the leaf level: at every level the children with the most slots first, so that the gang touches
// the fewest domains, the remainder by best fit.  The parts of one job -- distinct leaves, pods adding up to
// count[j], each within its leaf's slots -- go to PlaceGreedyDomains at level 0 as one job each and are all
// placed.  count is required; maxLevel nil: the top level; levelSize and parent as for GangCapacityTree.  A
// sharded engine refuses the call.  Read-only, like GangCapacity.
func (e *Engine) GangSplitTree(req []int64, need []uint32, count, maxLevel, levelSize, parent []int32, maxParts int32) (*TreeSplit, error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, fmt.Errorf("GangSplitTree: %d needs for %d jobs", len(need), J)
	}
	if len(count) != J {
		return nil, fmt.Errorf("GangSplitTree: %d counts for %d jobs", len(count), J)
	}
	if maxLevel != nil && len(maxLevel) != J {
		return nil, fmt.Errorf("GangSplitTree: %d max levels for %d jobs", len(maxLevel), J)
	}
	L := len(levelSize)
	valid := L >= 1 && L <= int(MaxLevels)
	T := 0
	for _, s := range levelSize {
		valid = valid && s >= 1 && s <= MaxDomains
		T += int(s)
	}
	if valid && parent != nil && len(parent) != T-int(levelSize[L-1]) {
		return nil, fmt.Errorf("GangSplitTree: %d parents for %d columns below the top level", len(parent), T-int(levelSize[L-1]))
	}
	out := &TreeSplit{}
	if valid && maxParts >= 1 && maxParts <= MaxSplitParts {
		out.Level = make([]int32, J)
		out.Domain = make([]int32, J)
		out.Parts = make([]int32, J)
		out.PartDomain = make([]int32, J*int(maxParts))
		out.PartPods = make([]int32, J*int(maxParts))
		out.Spread = make([]int32, J*L)
	}
	rc := C.pe_gang_split_tree(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr32(count), ptr32(maxLevel),
		C.int32_t(L), ptr32(levelSize), ptr32(parent), C.int32_t(maxParts), ptr32(out.Level), ptr32(out.Domain),
		ptr32(out.Parts), ptr32(out.PartDomain), ptr32(out.PartPods), ptr32(out.Spread))
	return out, e.err(rc, "pe_gang_split_tree")
}

// TreeSlices is GangSliceTree's answer: TreeSplit's, with the selected domain's units.
type TreeSlices struct {
	Level       []int32 // [J]: lowest level in [max(sliceLevel, 0), maxLevel] with a domain of units >= count / sliceSize; -1 = none
	Domain      []int32 // [J]: that level's domain with the smallest such units, ties to the smallest id
	DomainUnits []int64 // [J]: that domain's units (whole slices), 0 when none
	Parts       []int32 // [J]: number of (leaf, pods) parts; 0 = none selected, SplitTooMany
	PartDomain  []int32 // [J][maxParts]: the parts' leaf ids in list order, the tail -1
	PartPods    []int32 // [J][maxParts]: their pods (>= 1, adding up to count), the tail 0
	Spread      []int32 // [J][nLevels]: domains of each level the gang touches, 0 above the level
}

// SliceNode as a slice level: every slice inside one node.
const SliceNode = int32(C.PE_SLICE_NODE)

// GangSliceTree is GangSplitTree for gangs made of slices of sliceSize[j] pods (nil: 1) that must each sit
// inside one domain of level sliceLevel[j] (nil: 0; SliceNode: inside one node) -- a tensor-parallel group per
// node, per rack or per block.  Capacity counts whole slices at and above the slice level (a block's units are
// the sum of its racks' units) and pods below it.  count[j] must be a multiple of sliceSize[j].  With
// sliceLevel >= 0 the parts are placed as GangSplitTree's; with SliceNode part (leaf, a*z) is one job of a
// groups {count z, need | NeedIsland} in that leaf.  A sharded engine refuses the call.  Read-only.
func (e *Engine) GangSliceTree(req []int64, need []uint32, count, sliceSize, sliceLevel, maxLevel, levelSize, parent []int32, maxParts int32) (*TreeSlices, error) {
	J := len(req) / Dims
	if need != nil && len(need) != J {
		return nil, fmt.Errorf("GangSliceTree: %d needs for %d jobs", len(need), J)
	}
	if len(count) != J {
		return nil, fmt.Errorf("GangSliceTree: %d counts for %d jobs", len(count), J)
	}
	for _, a := range [][]int32{sliceSize, sliceLevel, maxLevel} {
		if a != nil && len(a) != J {
			return nil, fmt.Errorf("GangSliceTree: %d per-job values for %d jobs", len(a), J)
		}
	}
	L := len(levelSize)
	valid := L >= 1 && L <= int(MaxLevels)
	T := 0
	for _, s := range levelSize {
		valid = valid && s >= 1 && s <= MaxDomains
		T += int(s)
	}
	if valid && parent != nil && len(parent) != T-int(levelSize[L-1]) {
		return nil, fmt.Errorf("GangSliceTree: %d parents for %d columns below the top level", len(parent), T-int(levelSize[L-1]))
	}
	out := &TreeSlices{}
	if valid && maxParts >= 1 && maxParts <= MaxSplitParts {
		out.Level = make([]int32, J)
		out.Domain = make([]int32, J)
		out.DomainUnits = make([]int64, J)
		out.Parts = make([]int32, J)
		out.PartDomain = make([]int32, J*int(maxParts))
		out.PartPods = make([]int32, J*int(maxParts))
		out.Spread = make([]int32, J*L)
	}
	rc := C.pe_gang_slice_tree(e.ctx, C.int64_t(J), ptr64(req), ptru32(need), ptr32(count), ptr32(sliceSize),
		ptr32(sliceLevel), ptr32(maxLevel), C.int32_t(L), ptr32(levelSize), ptr32(parent), C.int32_t(maxParts),
		ptr32(out.Level), ptr32(out.Domain), ptr64(out.DomainUnits), ptr32(out.Parts), ptr32(out.PartDomain),
		ptr32(out.PartPods), ptr32(out.Spread))
	return out, e.err(rc, "pe_gang_slice_tree")
}

// Gangs is a greedy placement batch: jobs of groups of identical pods (include/placement.h).
type Gangs struct {
	JobGroupOff []int32  // [J+1]
	Priority    []int32  // [J]
	GroupCount  []int32  // [G] pods to place
	GroupReq    []int64  // [G][4]
	GroupNeed   []uint32 // [G] required label bits
}

func (g *Gangs) pods() int {
	n := 0
	for _, c := range g.GroupCount {
		n += int(c)
	}
	return n
}

// PlaceGreedy places the batch best-fit, all-or-nothing per job (SURVEY.md Appendix B).  Every rank
// of a sharded engine makes the same call and gets the same answer.
func (e *Engine) PlaceGreedy(g *Gangs) (podNode, jobStatus []int32, err error) {
	J := len(g.JobGroupOff) - 1
	podNode = make([]int32, g.pods())
	jobStatus = make([]int32, J)
	rc := C.pe_place_greedy(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.Priority), ptr32(g.GroupCount),
		ptr64(g.GroupReq), ptru32(g.GroupNeed), ptr32(podNode), ptr32(jobStatus))
	return podNode, jobStatus, e.err(rc, "pe_place_greedy")
}

// PlaceGreedyDomains is PlaceGreedy with job j's pods confined to the nodes whose level-`level` domain is
// jobDomain[j] ([J], each in [0, levelSize[level])): the call that acts on GangCapacityTree's answer.
// levelSize and parent describe the hierarchy exactly as for GangCapacityTree (parent nil allowed with one
// level); one call has one level.  Residuals are updated in place.  A sharded engine refuses the call.
func (e *Engine) PlaceGreedyDomains(g *Gangs, jobDomain []int32, level int32, levelSize, parent []int32) (podNode, jobStatus []int32, err error) {
	J := len(g.JobGroupOff) - 1
	if jobDomain != nil && len(jobDomain) != J {
		return nil, nil, fmt.Errorf("PlaceGreedyDomains: %d domains for %d jobs", len(jobDomain), J)
	}
	podNode = make([]int32, g.pods())
	jobStatus = make([]int32, J)
	rc := C.pe_place_greedy_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.Priority), ptr32(g.GroupCount),
		ptr64(g.GroupReq), ptru32(g.GroupNeed), ptr32(jobDomain), C.int32_t(level), C.int32_t(len(levelSize)),
		ptr32(levelSize), ptr32(parent), ptr32(podNode), ptr32(jobStatus))
	return podNode, jobStatus, e.err(rc, "pe_place_greedy_domains")
}

// MinMemberAll as a minMember: the whole job is mandatory (PE_MIN_MEMBER_ALL).
const MinMemberAll = int32(C.PE_MIN_MEMBER_ALL)

// PlaceMinMemberDomains is PlaceGreedyDomains for gangs that are schedulable at minMember[j] pods (the PodGroup's
// MinMember; nil or MinMemberAll: the whole job).  The mandatory pods -- the job's first minMember pod slots,
// plus the rest of an island group the cut falls in -- are placed all-or-nothing; after that every group's
// optional pods are placed as far as they fit, and the rest of the group keeps -1 and stays pending.  groupPods[g]
// and jobPods[j] count the pods that hold a node; podNode and groupPods can be handed straight to ReleaseGangs /
// AssumeGangs.  Residuals are updated in place.  A sharded engine refuses the call.
func (e *Engine) PlaceMinMemberDomains(g *Gangs, minMember, jobDomain []int32, level int32, levelSize, parent []int32) (podNode, jobStatus, groupPods []int32, jobPods []int64, err error) {
	J := len(g.JobGroupOff) - 1
	if minMember != nil && len(minMember) != J {
		return nil, nil, nil, nil, fmt.Errorf("PlaceMinMemberDomains: %d min members for %d jobs", len(minMember), J)
	}
	if jobDomain != nil && len(jobDomain) != J {
		return nil, nil, nil, nil, fmt.Errorf("PlaceMinMemberDomains: %d domains for %d jobs", len(jobDomain), J)
	}
	podNode = make([]int32, g.pods())
	jobStatus = make([]int32, J)
	groupPods = make([]int32, len(g.GroupCount))
	jobPods = make([]int64, J)
	rc := C.pe_place_min_member_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.Priority), ptr32(g.GroupCount),
		ptr64(g.GroupReq), ptru32(g.GroupNeed), ptr32(minMember), ptr32(jobDomain), C.int32_t(level),
		C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr32(podNode), ptr32(jobStatus), ptr32(groupPods),
		ptr64(jobPods))
	return podNode, jobStatus, groupPods, jobPods, e.err(rc, "pe_place_min_member_domains")
}

// GangFitDomains answers, for every pair p, whether PlaceGreedyDomains would place job pairJob[p] ALONE in the
// level-`level` domain pairDomain[p] against the current residuals (Gangs.Priority is not read).  Read-only.
// fits[p] is 1 or 0, failGroup[p] -1 or the job's first group that was not placed in full, pods[p] the pods
// placed when the rule stopped, first[j] the smallest fitting pair of job j or -1: first fit in the caller's
// pair order.  selectionOnly leaves the three per-pair answers nil (they never cross).  levelSize and parent
// describe the hierarchy exactly as for GangCapacityTree.  A sharded engine refuses the call.
func (e *Engine) GangFitDomains(g *Gangs, pairJob, pairDomain []int32, level int32, levelSize, parent []int32, selectionOnly bool) (fits []uint8, failGroup []int32, pods []int64, first []int32, err error) {
	J := len(g.JobGroupOff) - 1
	P := len(pairJob)
	if len(pairDomain) != P {
		return nil, nil, nil, nil, fmt.Errorf("GangFitDomains: %d jobs for %d domains", P, len(pairDomain))
	}
	first = make([]int32, J)
	if !selectionOnly {
		fits = make([]uint8, P)
		failGroup = make([]int32, P)
		pods = make([]int64, P)
	}
	rc := C.pe_gang_fit_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.GroupCount), ptr64(g.GroupReq),
		ptru32(g.GroupNeed), C.int64_t(P), ptr32(pairJob), ptr32(pairDomain), C.int32_t(level), C.int32_t(len(levelSize)),
		ptr32(levelSize), ptr32(parent), ptr8(fits), ptr32(failGroup), ptr64(pods), ptr32(first))
	return fits, failGroup, pods, first, e.err(rc, "pe_gang_fit_domains")
}

// PlaceFirstFitDomains places every job, in (priority desc, index asc) order, in the first of its candidate
// domains -- its pairs in ascending p, as for GangFitDomains -- in which PlaceGreedyDomains would place it against
// the residuals as the earlier jobs of the batch left them: the batch form of GangFitDomains followed by
// PlaceGreedyDomains, exact where that pair of calls is not (every job there selects on the untouched residuals).
// A job whose candidates all fail, or that is in no pair, is unschedulable.  jobPair[j] is the pair that placed job
// j or -1.  levelSize and parent describe the hierarchy exactly as for GangCapacityTree.  Residuals are updated in
// place.  A sharded engine refuses the call.
func (e *Engine) PlaceFirstFitDomains(g *Gangs, pairJob, pairDomain []int32, level int32, levelSize, parent []int32) (podNode, jobStatus, jobPair []int32, err error) {
	J := len(g.JobGroupOff) - 1
	P := len(pairJob)
	if len(pairDomain) != P {
		return nil, nil, nil, fmt.Errorf("PlaceFirstFitDomains: %d jobs for %d domains", P, len(pairDomain))
	}
	podNode = make([]int32, g.pods())
	jobStatus = make([]int32, J)
	jobPair = make([]int32, J)
	rc := C.pe_place_first_fit_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.Priority), ptr32(g.GroupCount),
		ptr64(g.GroupReq), ptru32(g.GroupNeed), C.int64_t(P), ptr32(pairJob), ptr32(pairDomain), C.int32_t(level),
		C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr32(podNode), ptr32(jobStatus), ptr32(jobPair))
	return podNode, jobStatus, jobPair, e.err(rc, "pe_place_first_fit_domains")
}

// Victims are placed gangs in the shape the placement calls take and return: victim v has the groups
// [GroupOff[v], GroupOff[v+1]) with GroupCount pods of GroupReq each ([VG][4], flattened), and PodNode holds the
// global node id of every pod slot, groups in input order, -1 for a slot that was skipped.
type Victims struct {
	GroupOff   []int32
	GroupCount []int32
	GroupReq   []int64
	PodNode    []int32
}

// MaxPairVictims is PE_MAX_PAIR_VICTIMS: the longest list of candidate victims of one pair.
const MaxPairVictims = C.PE_MAX_PAIR_VICTIMS

// GangPreemptDomains answers, for every pair p of GangFitDomains with the candidate victims
// pairVic[pairVicOff[p]:pairVicOff[p+1]] in eviction order, which of them must go for job pairJob[p] to be placed
// ALONE in the level-`level` domain pairDomain[p].  prefix[p] is the smallest prefix of the list whose release
// places the job (0: it fits as things stand, -1: it never does); victims[p] is the set that remains after every
// victim the job is placed without was put back, last candidate first (bit i = list position i); count[p] is its
// size, or -1; best[j] is the pair of job j with the smallest count, ties to the smallest p, or -1.  Read-only: a
// caller evicts, lets the Node informer's PE_NODE_SET bring the new residuals and then calls PlaceGreedyDomains.
// selectionOnly leaves the three per-pair answers nil (they never cross).  A sharded engine refuses the call.
func (e *Engine) GangPreemptDomains(g *Gangs, v *Victims, pairJob, pairDomain, pairVicOff, pairVic []int32, level int32, levelSize, parent []int32, selectionOnly bool) (prefix []int32, victims []uint64, count []int32, best []int32, err error) {
	J := len(g.JobGroupOff) - 1
	V := len(v.GroupOff) - 1
	P := len(pairJob)
	if len(pairDomain) != P {
		return nil, nil, nil, nil, fmt.Errorf("GangPreemptDomains: %d jobs for %d domains", P, len(pairDomain))
	}
	if len(pairVicOff) != P+1 {
		return nil, nil, nil, nil, fmt.Errorf("GangPreemptDomains: %d list offsets for %d pairs", len(pairVicOff), P)
	}
	best = make([]int32, J)
	if !selectionOnly {
		prefix = make([]int32, P)
		victims = make([]uint64, P)
		count = make([]int32, P)
	}
	rc := C.pe_gang_preempt_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.GroupCount), ptr64(g.GroupReq),
		ptru32(g.GroupNeed), C.int64_t(V), ptr32(v.GroupOff), ptr32(v.GroupCount), ptr64(v.GroupReq), ptr32(v.PodNode),
		C.int64_t(P), ptr32(pairJob), ptr32(pairDomain), ptr32(pairVicOff), ptr32(pairVic), C.int32_t(level),
		C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr32(prefix), ptru64(victims), ptr32(count), ptr32(best))
	return prefix, victims, count, best, e.err(rc, "pe_gang_preempt_domains")
}

// ReleaseGangs gives back what placed gangs hold (pe_release_gangs): every pod slot of v on a node that is not a
// removed slot adds its group's request to the node's residuals; -1 slots count nothing, so the arguments and
// outputs of a placement call -- an Unreserve, or the victims GangPreemptDomains names -- can be handed straight
// back.  All-or-nothing: a call that would raise a residual above the reset snapshot fails and changes nothing.
// Works on a sharded engine (every rank makes the same call).  pods is the number of pod slots that counted.
func (e *Engine) ReleaseGangs(v *Victims) (pods int64, err error) {
	var n C.int64_t
	rc := C.pe_release_gangs(e.ctx, C.int64_t(len(v.GroupOff)-1), ptr32(v.GroupOff), ptr32(v.GroupCount), ptr64(v.GroupReq),
		ptr32(v.PodNode), &n)
	return int64(n), e.err(rc, "pe_release_gangs")
}

// AssumeGangs is the inverse (pe_assume_gangs): every counted pod slot takes its group's request off its node's
// residuals -- the replay of the placements still in flight after LoadNodes or ResetResiduals.  It fails and
// changes nothing when a residual would fall below 0; only these totals are checked, not labels, needs or the
// best-fit rule.
func (e *Engine) AssumeGangs(v *Victims) (pods int64, err error) {
	var n C.int64_t
	rc := C.pe_assume_gangs(e.ctx, C.int64_t(len(v.GroupOff)-1), ptr32(v.GroupOff), ptr32(v.GroupCount), ptr64(v.GroupReq),
		ptr32(v.PodNode), &n)
	return int64(n), e.err(rc, "pe_assume_gangs")
}

// DrainFitDomains answers, for every candidate c, whether the pods that the book of placed gangs v has on node
// candNode[c] would all find a node in the level-`level` domain candDomain[c] with the node itself taken out, and
// where (pe_drain_fit_domains).  groupNeed ([VG], nil = 0) holds the groups' required label bits: a move respects
// labels.  fits[c] is 1 or 0, moved[c] the pods that had found a node when the rule stopped, failSlot[c] -1 or the
// pod slot of the first pod that found no node, target[s] the node the pod of slot s moves to, or -1.  Read-only: a
// caller acts on the answer with ReleaseGangs of the node's slots and AssumeGangs of the same groups at the targets.
// withTargets false leaves target nil (it never crosses).  levelSize and parent describe the hierarchy exactly as for
// GangCapacityTree.  A sharded engine refuses the call.
func (e *Engine) DrainFitDomains(v *Victims, groupNeed []uint32, candNode, candDomain []int32, level int32, levelSize, parent []int32, withTargets bool) (fits []uint8, moved, failSlot []int64, target []int32, err error) {
	nc := len(candNode)
	if len(candDomain) != nc {
		return nil, nil, nil, nil, fmt.Errorf("DrainFitDomains: %d nodes for %d domains", nc, len(candDomain))
	}
	if groupNeed != nil && len(groupNeed) != len(v.GroupCount) {
		return nil, nil, nil, nil, fmt.Errorf("DrainFitDomains: %d needs for %d groups", len(groupNeed), len(v.GroupCount))
	}
	fits = make([]uint8, nc)
	moved = make([]int64, nc)
	failSlot = make([]int64, nc)
	if withTargets {
		target = make([]int32, len(v.PodNode))
	}
	rc := C.pe_drain_fit_domains(e.ctx, C.int64_t(len(v.GroupOff)-1), ptr32(v.GroupOff), ptr32(v.GroupCount), ptr64(v.GroupReq),
		ptru32(groupNeed), ptr32(v.PodNode), C.int64_t(nc), ptr32(candNode), ptr32(candDomain), C.int32_t(level),
		C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr8(fits), ptr64(moved), ptr64(failSlot), ptr32(target))
	return fits, moved, failSlot, target, e.err(rc, "pe_drain_fit_domains")
}

// ScaleUp is ScaleUpDomains' answer: per pair the fewest new nodes (-1 = none up to the pair's maximum), the deciding
// attempt's failing group (-1 = placed), its pods and those of them on new nodes; per job the pair with the fewest
// new nodes, ties to the smallest pair, -1 = none.  With selectionOnly the per-pair slices are nil.
type ScaleUp struct {
	Nodes, FailGroup []int32
	Pods, NewPods    []int64
	Best             []int32
}

// ScaleUpDomains answers, for every pair p, how many nodes of template pairTemplate[p] -- free residual tmplRes[t]
// ([T][4] flattened), labels tmplLabels[t] (nil = 0) -- would have to join the level-`level` domain pairDomain[p] for
// PlaceGreedyDomains to place job pairJob[p] alone there (pe_scale_up_domains).  The i-th new node has id newSlot[i],
// a removed slot of the inventory; attempts run with 0, 1, ... pairMax[p] new nodes (nil = len(newSlot)) in that
// order, since the answer is not monotone.  Read-only.  selectionOnly leaves the four per-pair answers out (nothing
// pair-sized crosses).  levelSize and parent describe the hierarchy exactly as for GangCapacityTree.  A sharded engine
// refuses the call.
func (e *Engine) ScaleUpDomains(g *Gangs, tmplRes []int64, tmplLabels []uint32, newSlot, pairJob, pairDomain, pairTemplate, pairMax []int32, level int32, levelSize, parent []int32, selectionOnly bool) (ScaleUp, error) {
	J := len(g.JobGroupOff) - 1
	P := len(pairJob)
	T := len(tmplRes) / 4
	if len(pairDomain) != P || len(pairTemplate) != P || (pairMax != nil && len(pairMax) != P) {
		return ScaleUp{}, fmt.Errorf("ScaleUpDomains: %d jobs for %d domains, %d templates and %d maxima", P, len(pairDomain), len(pairTemplate), len(pairMax))
	}
	if len(tmplRes) != 4*T || (tmplLabels != nil && len(tmplLabels) != T) {
		return ScaleUp{}, fmt.Errorf("ScaleUpDomains: %d residual cells and %d labels for %d templates", len(tmplRes), len(tmplLabels), T)
	}
	out := ScaleUp{Best: make([]int32, J)}
	if !selectionOnly {
		out.Nodes = make([]int32, P)
		out.FailGroup = make([]int32, P)
		out.Pods = make([]int64, P)
		out.NewPods = make([]int64, P)
	}
	rc := C.pe_scale_up_domains(e.ctx, C.int64_t(J), ptr32(g.JobGroupOff), ptr32(g.GroupCount), ptr64(g.GroupReq),
		ptru32(g.GroupNeed), C.int32_t(T), ptr64(tmplRes), ptru32(tmplLabels), C.int32_t(len(newSlot)), ptr32(newSlot),
		C.int64_t(P), ptr32(pairJob), ptr32(pairDomain), ptr32(pairTemplate), ptr32(pairMax), C.int32_t(level),
		C.int32_t(len(levelSize)), ptr32(levelSize), ptr32(parent), ptr32(out.Nodes), ptr32(out.FailGroup), ptr64(out.Pods),
		ptr64(out.NewPods), ptr32(out.Best))
	return out, e.err(rc, "pe_scale_up_domains")
}

// Synchronize waits for the context's stream; Stream is its hipStream_t (for event timing).
func (e *Engine) Synchronize() error { return e.err(C.pe_synchronize(e.ctx), "pe_synchronize") }

func (e *Engine) Stream() unsafe.Pointer { return unsafe.Pointer(C.pe_stream(e.ctx)) }

// Stats and ResetStats: engine counters (fit evaluations, windows, placements, timings).
func (e *Engine) Stats() (Stats, error) {
	var s C.pe_stats
	rc := C.pe_get_stats(e.ctx, &s)
	return s, e.err(rc, "pe_get_stats")
}

func (e *Engine) ResetStats() error { return e.err(C.pe_reset_stats(e.ctx), "pe_reset_stats") }

// Resolver is the host half of the windowed greedy (pe_resolver_*), for callers that gather the
// per-shard candidate blobs over their own transport.  No device is touched.
type Resolver struct {
	r    *C.pe_resolver
	jobs int
	pods int
}

func NewResolver(g *Gangs) (*Resolver, error) {
	res := &Resolver{jobs: len(g.JobGroupOff) - 1, pods: g.pods()}
	rc := C.pe_resolver_create(C.int64_t(res.jobs), ptr32(g.JobGroupOff), ptr32(g.Priority), ptr32(g.GroupCount),
		ptr64(g.GroupReq), ptru32(g.GroupNeed), &res.r)
	if rc != C.PE_OK {
		return nil, fmt.Errorf("placement: pe_resolver_create: %d", int(rc))
	}
	return res, nil
}

func (r *Resolver) Close() {
	if r.r != nil {
		C.pe_resolver_destroy(r.r)
		r.r = nil
	}
}

// SetNodes bounds the node ids the blobs and seeds may list (pe_resolver_set_nodes): a blob from any
// transport with a header count outside [0, topK], an id >= nNodes or unsorted keys is then refused
// (PE_EINVAL) before the resolver moves.
func (r *Resolver) SetNodes(nNodes int64) error {
	if rc := C.pe_resolver_set_nodes(r.r, C.int64_t(nNodes)); rc != C.PE_OK {
		return fmt.Errorf("placement: pe_resolver_set_nodes: %d", int(rc))
	}
	return nil
}

func (r *Resolver) Done() bool { return C.pe_resolver_done(r.r) != 0 }

// NextWindow returns the global group ids of the next scan window.
func (r *Resolver) NextWindow(maxGroups int32, maxPods int64) ([]int32, error) {
	out := make([]int32, maxGroups)
	var n C.int32_t
	if rc := C.pe_resolver_next_window(r.r, C.int32_t(maxGroups), C.int64_t(maxPods), ptr32(out), &n); rc != C.PE_OK {
		return nil, fmt.Errorf("placement: pe_resolver_next_window: %d", int(rc))
	}
	return out[:n], nil
}

// Resolve consumes one window's blob (n_shards blocks, see placement.h) and returns the residual
// updates to flush ([n][5] = node id, res[4]) and whether the window was consumed.
func (r *Resolver) Resolve(groups []int32, blob []byte, nShards, topK int32) ([]int64, bool, error) {
	maxUpd := int64(2*r.pods + 64)
	upd := make([]int64, 5*maxUpd)
	var nu C.int64_t
	var consumed C.int32_t
	rc := C.pe_resolver_resolve(r.r, C.int32_t(len(groups)), ptr32(groups), ptr8(blob), C.int32_t(nShards),
		C.int32_t(topK), ptr64(upd), C.int64_t(maxUpd), &nu, &consumed)
	if rc != C.PE_OK {
		return nil, false, fmt.Errorf("placement: pe_resolver_resolve: %d", int(rc))
	}
	return upd[:5*int64(nu)], consumed != 0, nil
}

// ResolveSeeded is Resolve for the pipelined protocol: seeds ([n][6] int64: node id, res[0..3],
// labels) are the nodes changed since the snapshot the blob was scanned on, with current state.
func (r *Resolver) ResolveSeeded(groups []int32, blob []byte, nShards, topK int32, seeds []int64) ([]int64, bool, error) {
	if len(seeds)%6 != 0 {
		return nil, false, fmt.Errorf("placement: seeds must be [n][6]")
	}
	maxUpd := int64(2*r.pods + 64)
	upd := make([]int64, 5*maxUpd)
	var nu C.int64_t
	var consumed C.int32_t
	rc := C.pe_resolver_resolve_seeded(r.r, C.int32_t(len(groups)), ptr32(groups), ptr8(blob), C.int32_t(nShards),
		C.int32_t(topK), C.int64_t(len(seeds)/6), ptr64(seeds), ptr64(upd), C.int64_t(maxUpd), &nu, &consumed)
	if rc != C.PE_OK {
		return nil, false, fmt.Errorf("placement: pe_resolver_resolve_seeded: %d", int(rc))
	}
	return upd[:5*int64(nu)], consumed != 0, nil
}

// Results: the node of every pod slot (-1 = none) and every job's status.
func (r *Resolver) Results() (podNode, jobStatus []int32, err error) {
	podNode = make([]int32, r.pods)
	jobStatus = make([]int32, r.jobs)
	if rc := C.pe_resolver_results(r.r, ptr32(podNode), ptr32(jobStatus)); rc != C.PE_OK {
		return nil, nil, fmt.Errorf("placement: pe_resolver_results: %d", int(rc))
	}
	return podNode, jobStatus, nil
}
