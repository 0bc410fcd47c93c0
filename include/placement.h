/*
 * placement.h -- C ABI of libplacement, the MI355X-native gang-placement engine.
 *
 * Drop-in boundary for the training operator's PodGroup / coscheduling hot path.  Plain C11:
 * plain pointers and sizes, no C++ or torch types, integer return codes, no exceptions or
 * aborts across the ABI.  The reference is Go; the binding a maintainer adds on the reference
 * side (cgo package pkg/placement/hip) is in INTEGRATION.md.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo root):
 *   pe_pg_min_resources(PE_MODE_V1, ...)
 *       pkg/controller.v1/common/util.go:108  func CalcPGMinResources(minMember int32,
 *           replicas map[ReplicaType]*ReplicaSpec, pcGetFunc PriorityClassGetFunc) *v1.ResourceList
 *       (called from pkg/controller.v1/common/job.go:275-277,455-457; AddResourceList util.go:79-104)
 *   pe_pg_min_resources(PE_MODE_V2, ...)
 *       pkg/runtime.v2/framework/plugins/coscheduling/coscheduling.go:103-118  (*CoScheduling).Build
 *       aggregation loop, fed by pkg/runtime.v2/runtime.go:115-145 NewInfo (kueue TotalRequests)
 *   pe_fit_mask / pe_fit_mask_run, pe_place_greedy
 *       NO reference function: node fit / score / placement is done by the external gang
 *       scheduler (scheduler-plugins coscheduling / Volcano) that consumes the PodGroup the
 *       operator writes (pkg/controller.v1/control/podgroup_control.go:36-54).  The rule is
 *       build-defined and exposed here so the plugin can answer
 *       feasibility / placement itself.
 *   pe_create / pe_destroy / pe_last_error
 *       lifetime of the plugin instance: pkg/runtime.v2/framework/plugins/registry.go:32-42
 *       factory + coscheduling.go:71-85 New(); errors follow framework.go:117-121 (first error
 *       stops the phase) -> every call returns a code and sets a message.
 *
 * Units (canonical int64): dim 0 cpu in milli-cores, dim 1 memory in
 * bytes, dim 2 accelerator count (resource name given by pe_config.gpu_resource_name), dim 3
 * ephemeral-storage in bytes.  Values must be >= 0; int64 overflow is flagged, never wrapped
 * (where Go's resource.Quantity would fall back to inf.Dec); pe_pg_min_resources_wide answers those
 * jobs exactly in 128 bits.
 *
 * Ownership: the caller owns every host pointer for the duration of the call only; the library
 * never retains them.  Device memory is library-owned; pointers it hands out stay valid until
 * the next call that re-sizes the same buffer, or pe_destroy.
 * Threading: one mutex per context; every call selects the context's device itself (callers
 * such as cgo goroutines may migrate between OS threads).
 */
#ifndef PLACEMENT_H_
#define PLACEMENT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PE_ABI_VERSION 7
#define PE_DIMS 4
#define PE_COMM_ID_BYTES 128
#define PE_MAX_NODES (1LL << 24) /* node ids live in the low 24 bits of the best-fit key */

enum {
  PE_OK = 0,
  PE_EINVAL = -1,    /* bad argument (negative request, ids out of range, null pointer) */
  PE_EOVERFLOW = -2, /* int64 overflow in an aggregation (per-job flags say which job) */
  PE_ENOMEM = -3,
  PE_EHIP = -4,      /* HIP runtime error, see pe_last_error */
  PE_ERCCL = -5,     /* RCCL error */
  PE_ESTATE = -6,    /* call order (e.g. fit mask before pe_load_nodes) */
  PE_ENODEV = -7     /* no usable GPU: the engine has no CPU fallback */
};

enum { PE_MODE_V1 = 1, PE_MODE_V2 = 2 };
enum { PE_JOB_PLACED = 0, PE_JOB_UNSCHEDULABLE = 1 };
/* xGMI islands (SURVEY.md Appendix B extension; BASELINE config 4).  Label bit 31 of every node is
 * the engine's: set iff the node has an island (island >= 0 at pe_load_nodes / pe_update_nodes;
 * the caller's bit 31 is replaced).  A greedy group whose need has bit 31 is an ISLAND GROUP: its
 * group_count pods are co-located on ONE node with an island, chosen as a unit -- the node with
 * the smallest Appendix-B key for the summed request count x request (exact int64; a sum that
 * overflows fits nowhere) -- and all of them land on it, or the job fails (all-or-nothing).
 * Islands are single nodes in this model (one 8-GPU node = one xGMI island). */
#define PE_LABEL_ISLAND 0x80000000u
#define PE_NEED_ISLAND PE_LABEL_ISLAND

/* container record flags for pe_pg_min_resources: bits 0-3 = which dims are present in the
 * container's ResourceList (keys with value 0 are present), bits 4-5 = kind */
#define PE_KIND_SHIFT 4
enum { PE_KIND_CONTAINER = 0, PE_KIND_INIT = 1, PE_KIND_SIDECAR = 2, PE_KIND_OVERHEAD = 3 };

/* Host all-gather used instead of RCCL when set (tests run several shards on one GPU):
 * gather `bytes` from every rank into recv[rank * bytes]; return 0 on success. */
typedef int (*pe_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);

/* Intra-node host exchange (no reference counterpart: the transport of the sharded greedy when the
 * ranks share one node and RCCL cannot be set up, e.g. several ranks on one GPU).  An all-gather
 * through a POSIX shared-memory segment `name` ("/..."), one barrier per call; rank 0 creates it,
 * the other ranks wait for it (PE_HX_TIMEOUT_S, default 300 s) and the last rank to attach unlinks
 * the name.  Use as pe_config.exchange = pe_host_exchange_allgather, exchange_user = the handle;
 * every rank must make the same sequence of calls with the same byte counts (<= max_bytes).  A peer
 * that does not arrive within PE_HX_TIMEOUT_S makes the call return PE_ERCCL. */
typedef struct pe_host_exchange pe_host_exchange;
int pe_host_exchange_open(const char* name, int32_t rank, int32_t world, size_t max_bytes, pe_host_exchange** out);
int pe_host_exchange_allgather(void* user, const void* send, void* recv, size_t bytes);
void pe_host_exchange_close(pe_host_exchange* hx);

typedef struct pe_ctx pe_ctx;

typedef struct {
  int32_t device_id;             /* HIP ordinal; -1 = the calling thread's current device */
  int32_t rank;                  /* inventory shard owned by this process, 0..world_size-1 */
  int32_t world_size;            /* shards of the node inventory (1 = unsharded) */
  const uint8_t* comm_id;        /* PE_COMM_ID_BYTES from pe_comm_id() on rank 0 (RCCL); at
                                    world_size 1 it builds a 1-rank communicator */
  pe_allgather_fn exchange;      /* optional host exchange replacing RCCL */
  void* exchange_user;
  int64_t max_nodes;             /* global inventory capacity (<= PE_MAX_NODES) */
  const char* gpu_resource_name; /* resource key of dim 2, e.g. "amd.com/gpu" (informational) */
  int32_t topk;                  /* best-fit candidates kept per group and window (0 = 256; above
                                    1023 the windows take the full scan instead of the sorted walk) */
  int32_t window_groups;         /* groups per scan window (0 = 112) */
  int64_t window_pods;           /* pods per scan window (0 = 1024) */
  int32_t fit_path_mask;         /* allowed fit-mask kernels: bit0 int64 compare, bit1 int32 compare,
                                    bit2 dictionary-coded, bit4 bit planes (batches with more than 32
                                    distinct request values split into plane sets); bit3 set = no thermometer
                                    form of the coded kernel; bit5 set = bit planes through the
                                    block-major kernel (PE_MASK_NODE_BLOCKS) instead of the row-major
                                    sweep (PE_MASK_ROWS); no kernel bit set = all kernels (the
                                    int64 path is always allowed) */
  int32_t greedy_flags;          /* bit0 set = sequential greedy windows.  Default (clear): pipelined --
                                    the GPU scans the next window while the host resolves the current
                                    one, and the current window's changes are seeded as dirty nodes
                                    into the next one's resolution (exact either way).
                                    bit1 set = every window scans all nodes of the shard (scan +
                                    merge kernels) instead of the sorted walk */
  int32_t resort_nodes;          /* sorted walk: rebuild the sorted index once this many node updates
                                    were applied since the last build (0 = 20480) */
} pe_config;

typedef struct {
  int64_t fit_evals;     /* job x node fit evaluations (fit mask) */
  int64_t scan_evals;    /* group x node key evaluations (greedy full scans, greedy_flags bit1) */
  int64_t windows;       /* greedy scan windows */
  int64_t rescans;       /* windows cut short because a candidate list ran dry */
  int64_t groups_scanned;
  int64_t pods_placed;
  int64_t jobs_placed;
  int64_t jobs_failed;
  double last_greedy_ms; /* wall time of the last pe_place_greedy */
  double greedy_wait_ms; /* host time blocked on window scans + transfers (cumulative) */
  double greedy_host_ms; /* host time parsing + resolving windows (cumulative) */
  int64_t fit_runs_i32;  /* fit-mask launches on the exact 32-bit path (scaled requests) */
  int64_t fit_runs_i64;  /* fit-mask launches on the general 64-bit path */
  int64_t fit_runs_coded; /* fit-mask launches on the dictionary-coded path (SWAR or thermometer) */
  int64_t fit_runs_therm; /* ... of which used the thermometer code (3 VALU per 64 evaluations) */
  int64_t fit_runs_planes; /* fit-mask launches on the bit-plane path (5-way AND per 32 nodes) */
  int64_t resorts;       /* sorted-walk index builds (greedy) */
  int64_t fit_runs_lds;  /* fit-mask launches on the LDS digit-plane path (any cardinality) */
  int64_t fit_runs_sets; /* ... bit-plane launches that swept more than one plane set */
  int64_t walk_rounds;   /* greedy sorted walk: 1024-entry rounds walked, summed over groups */
  int64_t walk_overlay;  /* greedy sorted walk: overlay entries evaluated, summed over groups */
  int64_t walk_groups;   /* greedy sorted walk: group blocks launched */
  int64_t walk_prepass;  /* greedy sorted walk: round summaries read (rounds x groups) */
  double walk_ms;        /* walk kernel time by hipEvents, only when PE_WALK_EVENTS=1 in the environment */
  int64_t walk_pend_updates; /* greedy sorted walk: node updates applied while a side-stream index rebuild
                                was pending (written into both index sets' overlays) */
  int64_t xchg_zc_windows;   /* multi-rank greedy windows exchanged zero-copy through the shared-memory
                                exchange's registered segment (no host copy, no host barrier) */
  /* (ABI 6) the host exchange's cost, summed over windows: time its thread waited for the ranks'
     lists (zero-copy: spinning on peers' group signals; copying: inside the all-gather callback) and
     time it spent merging them on the host (zero-copy windows) */
  double xchg_wait_ms;
  double xchg_merge_ms;
  /* (ABI 7) aggregation calls above 8192 jobs (the chunked path): segments packed, how many of them crossed with
     narrowed request records (value >> per-key shift in 32 bits), and the packed bytes that crossed to
     the device, cumulative */
  int64_t agg_segments;
  int64_t agg_narrow_segments;
  int64_t agg_wire_bytes;
  /* (ABI 7, additive) jobs answered by the 128-bit aggregation kernel (pe_pg_min_resources_wide), cumulative */
  int64_t agg_wide_jobs;
} pe_stats;

int pe_abi_version(void);
/* RCCL unique id for a sharded context (call on rank 0, broadcast the bytes to every rank). */
int pe_comm_id(uint8_t out[PE_COMM_ID_BYTES]);
/* With a comm_id, pe_create waits for the RCCL communicator at most PE_RCCL_INIT_TIMEOUT_S seconds
 * (environment, default 120) and returns PE_ERCCL past that bound.  The abandoned set-up keeps
 * running on a detached thread (RCCL's bootstrap cannot be cancelled), so peers that arrive late may
 * still get a communicator whose collectives would hang.  PE_ERCCL on ANY rank is therefore a
 * collective decision: every rank must destroy its context (and, if it goes on, create a new one
 * with a host `exchange` or a fresh comm_id), as bench.py does through its gloo vote.  A process
 * that abandoned a set-up should leave with _exit(). */
int pe_create(const pe_config* cfg, pe_ctx** out);
void pe_destroy(pe_ctx* ctx);
const char* pe_last_error(const pe_ctx* ctx); /* valid until the next call on ctx */

/* Inventory: caller-owned host SoA [4][n] (row d = dim d) of the GLOBAL inventory; the context
 * keeps its shard [rank*n/world, (rank+1)*n/world) device-resident.  residual = cap - used.
 * The call is validated before anything is applied: n out of range, a missing array or a negative
 * cap / used cell ANYWHERE in the global arrays (this rank's shard or another's) is PE_EINVAL, and a
 * refused load leaves the context exactly as it was -- the inventory loaded before, its shard range,
 * residuals and reset snapshot, and the staged fit batch, which only an accepted load invalidates.
 * A load that fails on the device after that (PE_ENOMEM, PE_EHIP) leaves the context without an
 * inventory: PE_ESTATE until a load succeeds. */
int pe_load_nodes(pe_ctx* ctx, int64_t n, const int64_t* cap, const int64_t* used, const uint32_t* labels,
                  const int32_t* island);
int pe_reset_residuals(pe_ctx* ctx); /* residual := cap - used (device-side copy) */
/* Incremental inventory ingestion (Node list/watch -> SoA deltas).  The
 * loaded inventory is a table of n_total slots; the caller (the Node informer's event handler)
 * keeps the node-name -> slot map and a free-slot list, so an added node takes a free slot, an
 * updated node rewrites its slot and a deleted node empties it.  Per update i:
 *   op[i] = PE_NODE_SET:    cap[i][4], used[i][4], labels[i], island[i] replace slot slots[i]; its
 *                           residual (and the pe_reset_residuals snapshot) becomes cap - used,
 *                           replacing whatever placements had taken from it
 *   op[i] = PE_NODE_REMOVE: the slot is empty (nothing fits it, no labels, island -1)
 * Later entries for the same slot win.  Every rank of a sharded context gets the whole batch and
 * scatters the slots of its own shard on the device.  The batch is validated before anything is
 * applied (slot out of range, unknown op, negative capacity/usage: PE_EINVAL, nothing changes).
 * labels / island may be NULL (0 / -1). */
enum { PE_NODE_SET = 0, PE_NODE_REMOVE = 1 };
int pe_update_nodes(pe_ctx* ctx, int64_t n, const int64_t* slots, const uint8_t* op, const int64_t* cap /*[n][4]*/,
                    const int64_t* used /*[n][4]*/, const uint32_t* labels, const int32_t* island);
int pe_shard_range(const pe_ctx* ctx, int64_t* begin, int64_t* end);
/* Ranks of the context's RCCL communicator (ncclCommCount); 0 when the shards exchange through the
 * host callback, or an unsharded context was created without a comm_id. */
int pe_comm_ranks(const pe_ctx* ctx, int32_t* nranks);
int pe_read_residuals(pe_ctx* ctx, int64_t* res_out /* [4][end-begin] of this shard */);

/* Batched PodGroup MinResources (one job per lane on the GPU).
 *   groups of job j: [job_group_off[j], job_group_off[j+1]); containers of group g:
 *   [group_cont_off[g], group_cont_off[g+1]); cont_req [C][4], cont_flags [C].
 *   V1: groups in CalcPGMinResources order (priority desc; ties: type name asc), group_replicas
 *       -1 = nil, only PE_KIND_CONTAINER records count, pods counted until min_member[j];
 *       out_members = pods counted.
 *   V2: group = runtime.Info TotalRequests entry with its pod's containers (kueue formula),
 *       out_members = sum of replicas (Go int32 wrap-around), min_member ignored (may be NULL).
 * Outputs per job: out_min_res[j][4], out_present[j] (bit d = key d present), out_members[j],
 * out_overflow[j] (1 = int64 overflow: the reference would have switched to inf.Dec; that job's
 * out_min_res values are then defined as 0, its presence bits and members are still exact).
 * Returns PE_EOVERFLOW if any job overflowed (outputs still written).  A negative request is
 * PE_EINVAL (the first offending index in pe_last_error); a large batch streams to the device in
 * chunks, so the outputs of jobs before the offending chunk may then be written. */
int pe_pg_min_resources(pe_ctx* ctx, int32_t mode, int64_t n_jobs, const int32_t* job_group_off,
                        const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                        const int64_t* cont_req, const uint8_t* cont_flags, int64_t* out_min_res,
                        uint8_t* out_present, int32_t* out_members, uint8_t* out_overflow);

/* (ABI 7) The same aggregation over a per-call KEY TABLE: any ResourceName the reference sums
 * (util.go:80-103 AddResourceList; coscheduling.go:112-116), not only the four engine dimensions --
 * hugepages-2Mi, rdma/hca, several accelerator names, cpu finer than 1m.  The caller numbers the
 * call's distinct keys 0..n_keys-1 (n_keys <= PE_MAX_KEYS; a batch with more keys takes one call
 * per key slice: keys never interact) and gives each key a decimal scale s_k of its choosing:
 * cont_req[c][k] is container c's quantity of key k as an exact int64 count of 10^s_k units (e.g.
 * s = -9 for "1500u" cpu = 1500000 x 1e-9; bytes at s = 0).  The engine sums the integers per key,
 * exactly as pe_pg_min_resources does per dimension, and the caller reads result k back at s_k.
 * A value with no exact int64 at s_k, or a sum that overflows int64 (out_overflow), is what Go
 * would hold in inf.Dec: the caller's fallback to the reference is for those jobs only.
 *   cont_flags[c] = presence bits 0..n_keys-1 (keys with value 0 are present) | kind << PE_KEYS_KIND_SHIFT
 *   out_min_res[J][n_keys], out_present[J] (bit k = key k present), out_members / out_overflow as above.
 * Other bits in cont_flags are PE_EINVAL. */
#define PE_MAX_KEYS 16
#define PE_KEYS_KIND_SHIFT 16
int pe_pg_min_resources_keys(pe_ctx* ctx, int32_t mode, int64_t n_jobs, int32_t n_keys, const int32_t* job_group_off,
                             const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                             const int64_t* cont_req, const uint32_t* cont_flags, int64_t* out_min_res,
                             uint16_t* out_present, int32_t* out_members, uint8_t* out_overflow);

/* (ABI 7, additive) The key-table aggregation with an exact answer past int64 -- what the reference
 * holds in inf.Dec (util.go:83-86,98-101 Quantity.Add; coscheduling.go:113-115 Quantity.Mul).  Key
 * table, flags, modes, n_keys limits and PE_EINVAL rules are those of pe_pg_min_resources_keys.
 * Inputs: a request is the non-negative 128-bit integer hi * 2^64 + lo.
 *   cont_req_hi == NULL: hi = 0 and lo is read as int64; a negative lo is PE_EINVAL (first index in
 *                        pe_last_error), as in pe_pg_min_resources_keys.
 *   cont_req_hi != NULL: lo is a full uint64 and hi must be < 2^63, else PE_EINVAL with the index.  This
 *                        is how a value with no int64 at its key's scale travels.
 * Result per (job, key): the exact sum as a signed two's-complement 128-bit integer out_hi:out_lo
 * (signed: V2 multiplies by the int32 replica count, which may be negative).  out_overflow[j]:
 *   0  the int64 path answered: out_lo is bit-equal to pe_pg_min_resources_keys' out_min_res and
 *      out_hi is its sign extension
 *   1  some int64 step overflowed, or an input was wider than int64 (hi != 0, or lo >= 2^63 with hi
 *      given): the value is the exact 128-bit one, summed on the device by the 128-bit kernel
 *   2  some intermediate left [-2^127, 2^127) (sticky per job): that job's values are defined as 0
 * out_present / out_members are exact in every case.  Returns PE_OK unless some job is 2; then
 * PE_EOVERFLOW with every output still written.  Only the jobs that need it (flag != 0) are gathered
 * into a compact sub-batch for the 128-bit kernel; every other job of the batch takes the int64 path
 * of pe_pg_min_resources_keys, and a batch without such a job is that call. */
int pe_pg_min_resources_wide(pe_ctx* ctx, int32_t mode, int64_t n_jobs, int32_t n_keys, const int32_t* job_group_off,
                             const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                             const uint64_t* cont_req_lo /*[C][n_keys]*/, const uint64_t* cont_req_hi /*[C][n_keys] or NULL*/,
                             const uint32_t* cont_flags, uint64_t* out_lo /*[J][n_keys]*/, int64_t* out_hi /*[J][n_keys]*/,
                             uint16_t* out_present, int32_t* out_members, uint8_t* out_overflow);

/* What-if feasibility (config 5): bit (j, n) = fit(job j, node n) against the CURRENT residuals
 * of this shard, device-resident.  The kernel picks the fastest exact path for the batch and the
 * device layout follows it (pe_fit_mask_layout):
 *   PE_MASK_NODE_TILES (compare paths): word (j, c) holds nodes 64c..64c+63 (bit n%64) at
 *     ((j / 16) * Wt + c / 4) * 64 + (j % 16) * 4 + c % 4,   Wt = ceil(words_per_row / 4);
 *     ceil(J / 16) * Wt * 64 words
 *   PE_MASK_JOB_BITS (dictionary-coded path): word (b, n) holds jobs 64b..64b+63 (bit j%64) for
 *     node n at b * St + n,  St = shard nodes rounded up to 1024;  ceil(J / 64) * St words
 *   PE_MASK_ROWS (bit-plane path, default, and the LDS digit-plane path): row-major, word (j, c) at
 *     j * P + c;  J * P words.  The pitch P is whatever pe_fit_mask_row_pitch returns: at least
 *     words_per_row and a whole number of 128-B lines (16 words) -- on the bit-plane path a whole number
 *     of 8192-node blocks (128 words), on the LDS digit-plane path a whole number of that path's 2048-,
 *     4096- or 8192-node blocks, which may be fewer words than one 8192-node block
 *   PE_MASK_NODE_BLOCKS (bit-plane path, fit_path_mask bit5): word (j, c) at
 *     ((c / 128) * J + j) * 128 + c % 128, i.e. per 8192-node block a [J][128]-word slab;
 *     ceil(S / 8192) * J * 128 words, S = shard nodes
 * All layouts are written as whole 128-B lines, and every run writes every word of the extent stated
 * above.  Padding inside it -- bits of nodes >= S, words the formulas address for no (job, node) pair, job
 * bits >= J of PE_MASK_JOB_BITS -- is 0 in every layout, with two exceptions.  Rows J .. 16 * ceil(J / 16)
 * - 1 of PE_MASK_NODE_TILES are unspecified: the job table is padded with a request that a node with
 * INT64_MAX in every dimension and every label bit still fits.  With the study knob
 * PE_ROW_PITCH_BLOCKS above its default the words of a PE_MASK_ROWS row past the last 8192-node block
 * are unspecified (never written).  pe_fit_mask_rows always hands rows back
 * row-major [n_rows][words_per_row].  Counts are per job over this shard (sum across shards).
 * One-shot form: upload + compute + counts to host; *dev_mask receives the device pointer.  The
 * pointer is valid until the next pe_fit_mask, pe_jobs_upload, pe_load_nodes or pe_destroy on the
 * context, and every pe_fit_mask_run until then writes the same buffer. */
int pe_fit_mask(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/, const uint32_t* need,
                int64_t* out_feasible_count, const uint64_t** dev_mask, int64_t* words_per_row);
/* Staged form (device-resident inputs, used by the benchmark).  pe_jobs_upload (and pe_fit_mask)
 * plans the batch for the shard loaded at that moment; every pe_fit_mask_run re-reads the CURRENT
 * residuals and labels, so pe_update_nodes, pe_reset_residuals, pe_place_greedy and pe_gang_capacity
 * keep the staged batch valid and the next run sees their effect.  pe_load_nodes invalidates it:
 * after a load, pe_fit_mask_run, pe_fit_counts and pe_fit_mask_rows return PE_ESTATE until the next
 * pe_jobs_upload or pe_fit_mask. */
int pe_jobs_upload(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need);
int pe_fit_mask_run(pe_ctx* ctx); /* asynchronous on the context stream */
int pe_fit_counts(pe_ctx* ctx, int64_t* out_feasible_count); /* synchronizes */
int pe_fit_mask_rows(pe_ctx* ctx, int64_t row0, int64_t n_rows, uint64_t* out /*[n_rows][words_per_row]*/);
enum { PE_MASK_NODE_TILES = 0, PE_MASK_JOB_BITS = 1, PE_MASK_NODE_BLOCKS = 2, PE_MASK_ROWS = 3 };
int pe_fit_mask_layout(const pe_ctx* ctx, int32_t* layout);
/* u64 words between consecutive job rows of the device mask in the PE_MASK_ROWS layout (0 for
 * the other layouts). */
int pe_fit_mask_row_pitch(const pe_ctx* ctx, int64_t* words);

/* (ABI 7, additive) Gang capacity: how many pods of job j's shape the shard holds right now -- the
 * read-only what-if of a gang, where the fit mask answers for one pod.  NO reference function: the
 * consumers are the gang schedulers that read the PodGroup the operator writes (scheduler-plugins
 * coscheduling PreFilter, Volcano enqueue; pkg/controller.v1/control/podgroup_control.go:36-54), which
 * compare MinResources with what the cluster has free before they place anything.  The rule is
 * SURVEY.md Appendix B's: one pod of shape q on node n lowers floor(res_d / q_d) by exactly one in
 * every dimension with q_d > 0.  With fit(j, n) as pe_fit_mask defines it, against the CURRENT
 * residuals of this shard:
 *   cap(j, n) = 0                                                              if !fit(j, n)
 *             = min(PE_CAP_MAX, min over d with req_d > 0 of floor(res_d / req_d))   otherwise
 *               (no d with req_d > 0: PE_CAP_MAX)
 *   out_slots[j]    = sum over n of cap(j, n)   a gang of identical pods fits iff its size <= out_slots
 *   out_max_node[j] = max over n of cap(j, n)   (0 on an empty shard) an island gang -- PE_NEED_ISLAND in
 *                                               need[j], matched like any label bit -- fits iff its size
 *                                               <= out_max_node
 *   out_nodes[j]    = nodes with cap(j, n) >= 1 = pe_fit_mask's count for the same row
 * Exact: integer division of the int64 residuals, no rounding.  Per shard, as pe_fit_mask's counts:
 * the caller adds out_slots and out_nodes over shards and takes the maximum of out_max_node.  A job
 * of several groups needs every group's capacity, which is necessary, not sufficient: its exact
 * read-only answer within a domain is pe_gang_fit_domains (against the whole shard: pe_place_greedy,
 * which places it).  Residuals and the staged fit-mask state (pe_jobs_upload ...
 * pe_fit_mask_rows) are left as they are.  Each out_* may be NULL; need NULL = 0.  A negative request
 * is PE_EINVAL (the first offending index in pe_last_error), a call before pe_load_nodes PE_ESTATE. */
#define PE_CAP_MAX 2147483647 /* per-node capacity saturates here: the largest group_count */
int pe_gang_capacity(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/, const uint32_t* need /* or NULL = 0 */,
                     int64_t* out_slots, int32_t* out_max_node, int64_t* out_nodes);

/* (ABI 7, additive) Gang capacity per topology domain: which rack, scale-up domain or xGMI island group
 * holds a whole gang -- the level between pe_gang_capacity's out_max_node (one node) and out_slots (the
 * whole shard) that a topology-aware gang scheduler asks about before it admits a training job.
 * The DOMAIN of node n is island[n] as last given by pe_load_nodes or pe_update_nodes: an id in
 * [0, n_domains).  A node with island < 0 or island >= n_domains, and a removed slot, belongs to no domain
 * and counts nowhere.  The island-group greedy of pe_place_greedy (PE_NEED_ISLAND: the gang on ONE node
 * that has an island) is unchanged; there an island is still a single node.
 * With cap(j, n) exactly as pe_gang_capacity defines it, against the CURRENT residuals of this shard:
 *   out_dom_slots[j][k] = sum of cap(j, n) over the nodes n of domain k
 *   out_dom_nodes[j][k] = number of those nodes with cap(j, n) >= 1
 * When every island id is below n_domains, the sum over k of out_dom_slots[j][k] is pe_gang_capacity's
 * out_slots for need[j] | PE_NEED_ISLAND, and the sum of out_dom_nodes[j][k] its out_nodes.
 * Selection, on the device (only the three J-sized arrays cross for it; a caller who wants just the
 * answer passes the tables NULL and never pays for J x n_domains values):
 *   out_domain[j]       = the domain with the smallest out_dom_slots[j][k] >= count[j], ties to the
 *                         smallest k; -1 if there is none.  Best fit at the domain level: large domains
 *                         stay free for large gangs.
 *   out_domain_slots[j] = that domain's slots, 0 when none
 *   out_feasible[j]     = number of domains with out_dom_slots[j][k] >= count[j]
 * A non-NULL selection output requires count with every count[j] >= 1, else PE_EINVAL (the first
 * offending index in pe_last_error); without one, count is not read and may be NULL.
 * Sharded contexts: the tables are per shard, like pe_gang_capacity's counts -- a domain may span shards
 * and the caller adds the tables.  Selecting from one shard's table would be wrong, so with
 * world_size > 1 a non-NULL selection output is PE_EINVAL.
 * Read-only: residuals and the staged fit-mask state (pe_jobs_upload ... pe_fit_mask_rows) are left as
 * they are, and the call keeps nothing that a later pe_update_nodes or pe_load_nodes could invalidate.
 * Each out_* may be NULL; need NULL = 0.  PE_EINVAL: a negative request (the first offending index in
 * pe_last_error), n_domains outside [1, PE_MAX_DOMAINS].  PE_ESTATE: a call before pe_load_nodes.  An
 * empty shard or n_jobs == 0 is PE_OK: tables 0, out_domain -1, out_domain_slots and out_feasible 0. */
#define PE_MAX_DOMAINS 65536
int pe_gang_capacity_domains(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/,
                             const uint32_t* need /* or NULL = 0 */, const int32_t* count /*[j] or NULL*/,
                             int32_t n_domains, int64_t* out_dom_slots /*[j][n_domains] or NULL*/,
                             int64_t* out_dom_nodes /*[j][n_domains] or NULL*/, int32_t* out_domain /*[j] or NULL*/,
                             int64_t* out_domain_slots /*[j] or NULL*/, int32_t* out_feasible /*[j] or NULL*/);

/* (ABI 7, additive) Gang capacity over a topology hierarchy, such as node -> rack -> block -> zone: what is
 * the LOWEST level at which one domain holds the whole gang, and which domain of that level fits it best --
 * the question of topology-aware gang admission (Kueue's topology-aware scheduling: a gang that fits no
 * rack may fit one block; one with a "required: rack" policy must not be admitted at block level).
 * Levels and columns: level 0 is the leaf level, whose domains are the island ids in [0, level_size[0])
 * exactly as in pe_gang_capacity_domains (a node with another id, and a removed slot, counts nowhere at
 * any level).  n_levels in [1, PE_MAX_LEVELS], every level_size[l] in [1, PE_MAX_DOMAINS], T = the sum of
 * the level sizes.  The column of domain k of level l is off_l + k, off_0 = 0, off_{l+1} = off_l + level_size[l].
 * Parent map, an argument of the call (nothing about it is kept in the context): parent[off_l + k] is the
 * level-(l + 1) domain that contains domain k of level l, in [0, level_size[l + 1]), or -1: the domain
 * counts at its own level and nowhere above.  The top level has no entries.
 * Tables, against the CURRENT residuals of this shard:
 *   out_tree_slots[j][off_0 + k], out_tree_nodes[j][off_0 + k] = pe_gang_capacity_domains' out_dom_slots[j][k],
 *                                    out_dom_nodes[j][k] for n_domains = level_size[0]
 *   out_tree_slots[j][off_{l+1} + p] = sum of out_tree_slots[j][off_l + c] over the children c with
 *                                    parent[off_l + c] == p; out_tree_nodes by the same rule
 * Every node counts at most once per level, so all sums stay below 2^55: exact int64.
 * Selection, on the device (requested by any non-NULL out_level, out_domain, out_domain_slots or
 * out_feasible; the tables may be NULL and then never cross):
 *   out_level[j]        = the smallest l <= max_level[j] at which some domain has out_tree_slots >= count[j];
 *                         -1 if there is none.  "Required at level r" is max_level[j] = r; "preferred
 *                         lowest" is max_level NULL (= n_levels - 1 for every job).
 *   out_domain[j]       = the domain of that level (its id within the level, not its column) with the
 *                         smallest such slots, ties to the smallest id; -1 when none
 *   out_domain_slots[j] = that domain's slots, 0 when none
 *   out_feasible[j][l]  = number of level-l domains with out_tree_slots >= count[j], for EVERY level,
 *                         those above max_level[j] included
 * A selection requires count with every count[j] >= 1 and every max_level[j] in [0, n_levels); without one
 * neither array is read.  With n_levels == 1 every output equals the corresponding output of
 * pe_gang_capacity_domains (out_level 0 or -1).
 * Sharded contexts, as pe_gang_capacity_domains: the tables are per shard and the caller adds them over
 * the shards (the roll-up is linear, so the summed table is the global one); with world_size > 1 a
 * non-NULL selection output is PE_EINVAL.
 * Read-only: residuals, the staged fit-mask state and everything a later pe_gang_capacity_domains call
 * relies on are left as they are.  Each out_* may be NULL; need NULL = 0.
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): a negative
 * request, a count below 1, a max_level out of range, n_levels or a level size out of range, a parent
 * outside [-1, level_size[l + 1]), a NULL level_size, a NULL parent with n_levels > 1.  PE_ESTATE: a call
 * before pe_load_nodes.  An empty shard or n_jobs == 0 is PE_OK: tables 0, out_level and out_domain -1,
 * out_domain_slots and out_feasible 0. */
#define PE_MAX_LEVELS 4
int pe_gang_capacity_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/,
                          const uint32_t* need /* or NULL = 0 */, const int32_t* count /*[j] or NULL*/,
                          const int32_t* max_level /*[j] or NULL = n_levels - 1*/,
                          int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                          const int32_t* parent /*[T - level_size[n_levels-1]], NULL allowed when n_levels == 1*/,
                          int64_t* out_tree_slots /*[j][T] or NULL*/, int64_t* out_tree_nodes /*[j][T] or NULL*/,
                          int32_t* out_level /*[j] or NULL*/, int32_t* out_domain /*[j] or NULL*/,
                          int64_t* out_domain_slots /*[j] or NULL*/, int32_t* out_feasible /*[j][n_levels] or NULL*/);

/* (ABI 7, additive) A gang spread over the fewest domains: pe_gang_capacity_tree's selection, followed by the
 * descent from the selected domain down to the leaf level -- the second phase of Kueue's topology-aware
 * scheduling.  A gang that fits no rack but fits a block gets "these racks, with this many pods each", the
 * fewest racks that hold it.  Levels, columns, level_size, parent, req, need, count, max_level and the table
 * tree_slots[j][.] mean exactly what they mean in pe_gang_capacity_tree; slots(l, k) below is
 * tree_slots[j][off_l + k] against the CURRENT residuals.
 * Step 1, selection: out_level[j] and out_domain[j] are pe_gang_capacity_tree's, bit for bit: the lowest
 * level <= max_level[j] with a domain of slots >= count[j], and there the best fit.  When there is none, both
 * are -1, out_parts[j] is 0, out_spread[j][.] is 0 and the part rows are -1 (domains) and 0 (pods).
 * Step 2, descent: S_L = [(out_domain[j], count[j])] with L = out_level[j].  For l = L down to 1 and for every
 * (P, a) of S_l in list order: the children of P are the level-(l - 1) domains c with parent[off_{l-1} + c]
 * == P (their slots add up to P's, so a <= slots(P) holds at every step).  Order them by (slots descending,
 * id ascending) and walk them with r = a: while the current child's slots are < r it is a WHOLE part, gets all
 * its slots, and r -= slots; at the first child with slots >= r the walk stops and the LAST part gets r pods.
 * The last part goes to the child with the smallest slots >= r among those not yet taken, ties to the smallest
 * id -- best fit for the remainder, so that large domains stay free for large gangs.  The parts are appended
 * to S_{l-1}: the whole parts in walk order, then the last part.  S_0 is the answer, in list order:
 *   out_part_domain[j][i] = a leaf id, out_part_pods[j][i] >= 1 for i < out_parts[j] = |S_0|; the unused
 *                           tail of both rows ([max_parts] per job) is -1 / 0
 *   out_spread[j][l]      = |S_l| for l <= L and 0 above: the domains of level l the gang touches.
 *                           out_spread[j][L] = 1, out_spread[j][0] = out_parts[j]
 * Consequences: the pods of a job's parts add up to count[j]; every part has pods <= slots(0, leaf); the
 * leaves are distinct; per parent the number of children used is the smallest k for which the k largest
 * children hold its allotment; a child without slots is never a part; with n_levels == 1 or out_level[j] == 0
 * there is one part (out_domain[j], count[j]).
 * max_parts in [1, PE_MAX_SPLIT_PARTS].  |S_l| never shrinks on the way down: a job whose |S_l| exceeds
 * max_parts at ANY level has out_parts[j] = PE_SPLIT_TOO_MANY, part rows -1 / 0 and out_spread[j][.] 0, while
 * out_level[j] and out_domain[j] stay valid.
 * Acting on the answer: for need without PE_NEED_ISLAND give the parts of ONE job to pe_place_greedy_domains
 * in one call, each part as a job of its own with one group (req, need, count = the part's pods), job_domain
 * = the part's leaf, level 0.  All of them are placed: distinct leaves are disjoint nodes, and pods <= slots
 * is exact by pe_gang_capacity's rule.  (Two jobs of one call may have been given the same free slots: place
 * one, then ask again.)  With PE_NEED_ISLAND the bit is matched as a label bit, as in every capacity call.
 * Read-only: residuals, host mirror, reset snapshot, staged fit-mask state and pe_stats are untouched, and
 * nothing of the hierarchy is kept in the context.  Each out_* may be NULL; need NULL = 0, max_level NULL =
 * n_levels - 1 for every job.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (the selection needs the global table; add the
 * shards' tables and apply the rule on the host).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): everything
 * pe_gang_capacity_tree refuses for a selection (count is required), and max_parts out of range.  PE_ESTATE:
 * a call before pe_load_nodes.  An empty shard or n_jobs == 0 is PE_OK with -1 / 0 everywhere. */
#define PE_MAX_SPLIT_PARTS 1024
#define PE_SPLIT_TOO_MANY (-1)
int pe_gang_split_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/,
                       const uint32_t* need /* or NULL = 0 */, const int32_t* count /*[j], >= 1*/,
                       const int32_t* max_level /*[j] or NULL = n_levels - 1*/,
                       int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                       const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                       int32_t max_parts,
                       int32_t* out_level /*[j] or NULL*/, int32_t* out_domain /*[j] or NULL*/,
                       int32_t* out_parts /*[j] or NULL*/, int32_t* out_part_domain /*[j][max_parts] or NULL*/,
                       int32_t* out_part_pods /*[j][max_parts] or NULL*/, int32_t* out_spread /*[j][n_levels] or NULL*/);

/* (ABI 7, additive) A gang in slices, each inside one domain: pe_gang_split_tree for a gang that is made of
 * groups of z pods -- tensor- or pipeline-parallel groups -- which must each sit inside one scale-up domain
 * (a node, a rack, a block) while the groups are free to spread: Kueue's podset slices (sliceSize,
 * sliceRequiredTopology).  Capacity is counted in slices at and above the slice level and in pods below it.
 * Unless stated otherwise levels, columns, level_size, parent, req, need, count, max_level, max_parts, cap(j, n)
 * and slots(l, k), the -1 / 0 tails, PE_SPLIT_TOO_MANY, NULL outputs, read-only-ness, the empty shard and
 * n_jobs == 0 mean exactly what they mean in pe_gang_split_tree.
 * For job j write z = slice_size[j] (NULL = 1), sl = slice_level[j] (NULL = 0; PE_SLICE_NODE = every slice on
 * one node), m = max(sl, 0) and u = count[j] / z, the slices wanted.
 * Units: units(l, k) is defined for l >= m, against the CURRENT residuals.
 *   sl == PE_SLICE_NODE: units(0, k) = sum over the nodes n of leaf domain k of floor(cap(j, n) / z)
 *   sl >= 0:             units(sl, k) = floor(slots(sl, k) / z)
 *   l > m:               units(l, p) = the sum of units(l - 1, c) over the children c of p -- NOT
 *                        floor(slots(l, p) / z): two racks with 12 slots each hold 2 slices of 8, not 3.
 * Selection: out_level[j] = the smallest l in [m, max_level[j]] at which some domain has units >= u;
 * out_domain[j] = the domain of that level with the smallest such units, ties to the smallest id;
 * out_domain_units[j] = that domain's units.  When there is none: -1, -1, 0, no parts, spread 0.
 * Descent: S_L = [(out_domain[j], u)], in units.
 *   1. For l = L down to m + 1: pe_gang_split_tree's step, word for word, with units(l - 1, .) in the place of
 *      the slots.
 *   2. At level m every entry (D, a) becomes (D, a * z), in pods.
 *   3. For l = m down to 1: the same step with slots(l - 1, .).  a * z <= slots(m, D) because
 *      a <= floor(slots(m, D) / z), so the step's premise is kept.
 *   4. S_0 is the answer; out_spread[j][l] = |S_l|.  PE_SPLIT_TOO_MANY as soon as a list passes max_parts, with
 *      out_level[j], out_domain[j] and out_domain_units[j] still valid.
 * Consequences: the pods of a job's parts add up to count[j]; with sl <= 0 every part is a multiple of z; with
 * sl >= 1 the pods that land under any one level-sl domain are a multiple of z; every part has pods <=
 * slots(0, leaf); with sl == PE_SLICE_NODE every part's slices are <= units(0, leaf); the leaves are distinct;
 * with z == 1 and sl in {PE_SLICE_NODE, 0} every output this call shares with pe_gang_split_tree is bit-equal
 * to that call's.
 * Acting on the answer.  sl >= 0: as pe_gang_split_tree, one one-group job per part at level 0.
 * sl == PE_SLICE_NODE: part (leaf, a * z) goes to pe_place_greedy_domains as ONE job of a groups, each
 * {count z, req, need | PE_NEED_ISLAND}, job_domain = leaf, level 0; the jobs of one answer in one call are all
 * placed: an island group fits node n exactly when cap(j, n) >= z, and taking z pods lowers floor(cap / z) of
 * that node by exactly one.  (Every node of a domain has an island, so the label bit matches.)
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): everything
 * pe_gang_split_tree refuses, a slice_size below 1, a count that is not a multiple of its slice_size, a
 * slice_level outside [PE_SLICE_NODE, n_levels), a max_level (given or defaulted) below max(slice_level, 0),
 * world_size > 1 (node-level units cannot be had from the shards' tables).  PE_ESTATE: a call before
 * pe_load_nodes. */
#define PE_SLICE_NODE (-1)
int pe_gang_slice_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/,
                       const uint32_t* need /* or NULL = 0 */, const int32_t* count /*[j], >= 1*/,
                       const int32_t* slice_size /*[j] or NULL = 1*/, const int32_t* slice_level /*[j] or NULL = 0*/,
                       const int32_t* max_level /*[j] or NULL = n_levels - 1*/,
                       int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                       const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                       int32_t max_parts,
                       int32_t* out_level /*[j] or NULL*/, int32_t* out_domain /*[j] or NULL*/,
                       int64_t* out_domain_units /*[j] or NULL*/,
                       int32_t* out_parts /*[j] or NULL*/, int32_t* out_part_domain /*[j][max_parts] or NULL*/,
                       int32_t* out_part_pods /*[j][max_parts] or NULL*/, int32_t* out_spread /*[j][n_levels] or NULL*/);

/* Greedy best-fit all-or-nothing gang placement.  Jobs in (priority
 * desc, index asc) order, groups of a job in the given order, pods of a group identical.
 *   job_group_off[J+1], priority[J], group_count[G] (pods to place), group_req[G][4],
 *   group_need[G] (required label bits).
 * out_pod_node[sum(group_count)]: GLOBAL node id per pod slot (groups in input order), -1 = none.
 * out_job_status[J]: PE_JOB_PLACED / PE_JOB_UNSCHEDULABLE.  Residuals are updated in place
 * (successful placements stay; failed jobs are rolled back).  Every rank of a sharded context
 * must make the same call; all ranks return the same placements.  group_need bit 31
 * (PE_NEED_ISLAND) makes the group an island group (see PE_LABEL_ISLAND).
 * RCCL transport: a window whose all-gather does not complete within PE_RCCL_TIMEOUT_S seconds
 * (environment, default 60; a peer lost mid-batch) makes the call return PE_ERCCL; the context's
 * communicator is then aborted (ncclCommAbort, on a thread of its own: the call returns at once)
 * and every later sharded call on the context returns PE_ERCCL -- destroy it and rebuild (e.g. on a
 * pe_host_exchange), as bench.py does.  The host exchange's bound is PE_HX_TIMEOUT_S. */
int pe_place_greedy(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                    const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                    int32_t* out_pod_node, int32_t* out_job_status);

/* (ABI 7, additive) Gang placement inside a chosen topology domain: the call that acts on
 * pe_gang_capacity_tree's answer ("rack 1733 holds this gang" -> place the gang in rack 1733; Kueue's
 * "required: rack").  NO reference function, as pe_place_greedy.  Levels, columns, level_size and parent
 * mean exactly what they mean in pe_gang_capacity_tree (nothing of the hierarchy is kept in the context).
 * The level-l domain of node n:
 *   dom_0(n)     = island[n] if it lies in [0, level_size[0]), else none (a removed slot is in no domain)
 *   dom_{l+1}(n) = parent[off_l + dom_l(n)], or none if that is -1 or dom_l(n) is none
 * The rule is pe_place_greedy's with one more condition in fit: job j's pods land
 * only on nodes with dom_level(n) == job_domain[j].  Everything else is unchanged: jobs in (priority desc,
 * index asc) order, groups in the given order, each pod on the argmin-key node, all-or-nothing with
 * rollback, PE_NEED_ISLAND groups as one unit of count x request on one node (a product that overflows
 * fits nowhere), out_pod_node slots in group input order with GLOBAL node ids and -1 for none,
 * out_job_status as before, residuals updated in place (successful placements stay).  Equivalently: per
 * domain, pe_place_greedy on the sub-inventory of that domain's nodes with that domain's jobs.
 * One call has one level; every job_domain[j] lies in [0, level_size[level]) (an unconstrained job belongs
 * to pe_place_greedy).  A job whose domain has no node is PE_JOB_UNSCHEDULABLE, a job with no pods
 * PE_JOB_PLACED; n_jobs == 0 is PE_OK.  Jobs of different domains touch disjoint nodes, so the device
 * places all domains in parallel, one workgroup each, and the sequential rule binds only inside a domain.
 * After the call the device residuals and the host mirror both hold the new residuals: a following
 * pe_place_greedy, fit-mask run or capacity call sees them; pe_reset_residuals restores as usual and the
 * staged fit batch stays valid.  pe_stats: adds to pods_placed, jobs_placed and jobs_failed only.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing changed and no output written (the first offending index in pe_last_error where there
 * is one): everything pe_place_greedy refuses (a negative request or count, bad offsets, a missing array),
 * a NULL job_domain, a job_domain out of range, level outside [0, n_levels), and everything
 * pe_gang_capacity_tree refuses about the hierarchy.  PE_ESTATE: a call before pe_load_nodes. */
int pe_place_greedy_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                            const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need /* or NULL = 0 */,
                            const int32_t* job_domain /*[J]*/, int32_t level,
                            int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                            const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                            int32_t* out_pod_node, int32_t* out_job_status);

/* (ABI 7, additive) MinMember first, the rest as fits: pe_place_greedy_domains for a PodGroup whose MinMember
 * is below its pod total (an elastic PyTorchJob, any job with SchedulingPolicy.MinAvailable).  The gang is
 * schedulable once min_member[j] pods hold a node; the other pods are bound as far as they fit and stay pending
 * otherwise -- what Volcano and the coscheduling plugin do with the PodGroup.  The smallest case: a rack of two
 * nodes with 8 free GPUs each, Master = 1 pod x 2 GPUs followed by Workers = 6 pods x 3 GPUs: 7 pods, 20 GPUs
 * against 16 free, so pe_place_greedy_domains places nothing.  With min_member 4 the master and three workers
 * are mandatory; the node that took the master holds two workers (6 / 3), the other node two (8 / 3): the job
 * is placed with 5 pods, out_group_pods {1, 4}, the last two worker slots -1, and 0 and 2 GPUs left.  With
 * min_member 6 the job is unschedulable and the residuals are untouched.
 * NO reference function, as pe_place_greedy_domains.  Everything not said here means what it means in that
 * call: jobs in (priority desc, index asc) order, groups in the given order, each pod on the argmin-key node of
 * job_domain[j] at `level`, PE_NEED_ISLAND groups as one unit of count x request on one node (a product that
 * overflows fits nowhere), zero-count groups skipped, pod slots in group input order with GLOBAL node ids.
 * Totals and the mandatory share.  T_j is job j's pod total, b_g the pods of the job's groups before group g.
 *   M_j = T_j when min_member is NULL or min_member[j] == PE_MIN_MEMBER_ALL, else min_member[j]
 *   m_g = clamp(M_j - b_g, 0, count_g)    the mandatory pods of group g; an island group is indivisible:
 *                                         m_g > 0 makes it count_g
 *   o_g = count_g - m_g                   its optional pods
 * So the mandatory pods are pod slots [0, M_j) of the job, plus the rest of an island group that M_j cuts.  With
 * the groups given in CalcPGMinResources order these are the pods that aggregation mode V1 counts ("until
 * podCnt == minMember"): MinResources of the PodGroup is the request of exactly the mandatory pods.
 * Phase 1 (mandatory) is pe_place_greedy_domains' treatment of the job with the counts m_g: all-or-nothing,
 * rolled back in full on the first pod that finds no node.  On failure the job is PE_JOB_UNSCHEDULABLE, every
 * one of its pod slots is -1 (the optional ones too), its out_group_pods and out_job_pods are 0, the residuals
 * are as before the job, and phase 2 is not tried.
 * Phase 2 (optional), only after a placed phase 1, runs over the job's groups in order with o_g > 0.  A group
 * without PE_NEED_ISLAND places its optional pods one at a time by the same argmin rule until a pod finds no
 * node; the remaining slots of THAT group are -1 and the rule goes on with the next group.  An optional island
 * group is placed as its one unit or not at all.  Nothing of phase 2 is rolled back; the job is PE_JOB_PLACED.
 * Within a group the slots that hold a node are a prefix of its slots: mandatory first, then optional.
 *   out_group_pods[g] = the pods of group g that hold a node
 *   out_job_pods[j]   = their sum over the job's groups
 * Every pod slot and every status is written; out_group_pods and out_job_pods may be NULL.  A job without groups
 * or pods is placed.  A domain without nodes: a job with M_j == 0 is placed with 0 pods, a job with a mandatory
 * pod is unschedulable.  n_jobs == 0 is PE_OK.
 * Identities: with min_member NULL, or M_j == T_j for every job, out_pod_node, out_job_status and the residuals
 * equal pe_place_greedy_domains'.  The outputs can be handed straight to pe_release_gangs / pe_assume_gangs
 * (slots holding -1 count nothing).
 * After the call the device residuals and the host mirror both hold the new residuals; pe_reset_residuals
 * restores as usual and the staged fit batch stays valid.  pe_stats: adds to pods_placed (pods that hold a
 * node), jobs_placed and jobs_failed only.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing changed and no output written (the first offending index in pe_last_error where there
 * is one): everything pe_place_greedy_domains refuses, a min_member[j] below -1 and a min_member[j] above T_j.
 * PE_ESTATE: a call before pe_load_nodes. */
#define PE_MIN_MEMBER_ALL (-1)
int pe_place_min_member_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                                const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need /* or NULL = 0 */,
                                const int32_t* min_member /*[J], or NULL = every job PE_MIN_MEMBER_ALL*/,
                                const int32_t* job_domain /*[J]*/, int32_t level,
                                int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                                const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                                int32_t* out_pod_node, int32_t* out_job_status,
                                int32_t* out_group_pods /*[G] or NULL*/, int64_t* out_job_pods /*[J] or NULL*/);

/* (ABI 7, additive) Exact what-if of a whole gang per domain: would this job, all its groups in order, be
 * placed in this domain right now?  The read-only link between pe_gang_capacity_tree (which domains hold a
 * gang of ONE shape) and pe_place_greedy_domains (which places the gang and changes the residuals).  For a
 * job of several groups -- a PyTorchJob's Master and Workers, an MPIJob's launcher and workers -- every
 * capacity call can say yes for a domain in which the placement then fails.  The smallest case: a rack of
 * two nodes with 8 free GPUs each, group A = 2 pods x 5 GPUs followed by group B = 3 pods x 2 GPUs.
 * MinResources is 16 <= 16 free, A's slots are 2 >= 2, B's slots are 8 >= 3; but once A has taken one node
 * each, 3 + 3 GPUs are left and B places two of its three pods.  This call answers 0, fail_group 1, pods 4.
 * NO reference function, as pe_place_greedy_domains.  Levels, columns, level_size, parent and dom_level(n)
 * mean exactly what they mean in pe_place_greedy_domains; nothing of the hierarchy is kept in the context;
 * one call has one level.
 * Pair p asks: against the CURRENT residuals of the context, with no other job in the call, would
 * pe_place_greedy_domains given the single job pair_job[p] with job_domain = pair_domain[p] return
 * PE_JOB_PLACED?  The rule is that call's, unchanged: groups in the given order, each pod on the argmin-key
 * node of the domain, PE_NEED_ISLAND groups as one unit of count x request on one node (a product that
 * overflows fits nowhere), zero-count groups skipped, a job without groups or pods is placed, a domain
 * without nodes holds only a job with no pod to place.  There is no priority: every pair is judged alone.
 *   out_fits[p]       = 1 or 0
 *   out_fail_group[p] = -1 when the pair fits, else the index within the job (0 = its first group) of the
 *                       first group that could not be placed in full
 *   out_pods[p]       = the pods the rule had placed when it stopped: the job's pod total when the pair fits,
 *                       else the pods of the earlier groups plus the pods of the failing group placed before
 *                       the first pod that found no node (a failing island group contributes 0)
 *   out_first[j]      = the smallest p with pair_job[p] == j and out_fits[p] == 1, -1 when there is none:
 *                       first fit in the CALLER's order, who expresses preference by ordering the pairs
 *                       (pe_gang_capacity_tree's slots, lowest level first over several calls, ...)
 * out_first is computed on the device; a caller who wants only the selection passes the three P-sized
 * outputs NULL and they never cross.  Each out_* may be NULL; group_need NULL = 0.
 * The pairs may come in any order, need not be grouped by job, may repeat and may name any number of
 * domains; a job in no pair has out_first -1.  n_pairs == 0 and n_jobs == 0 are PE_OK (with n_jobs > 0
 * and no pairs out_first is all -1).
 * Read-only: the device residuals, the host mirror, the staged fit-mask state (pe_jobs_upload ...
 * pe_fit_mask_rows) and pe_stats are left exactly as they are, and the call keeps nothing that a later
 * pe_update_nodes or pe_load_nodes could invalidate.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): everything
 * pe_place_greedy_domains refuses about the groups, the hierarchy and level; a NULL pair_job or pair_domain
 * with n_pairs > 0; n_pairs outside [0, 2^31 - 1); a pair_job outside [0, n_jobs); a pair_domain outside
 * [0, level_size[level]).  PE_ESTATE: a call before pe_load_nodes.  PE_ENOMEM: the working copies of
 * domains too large for the workgroup's local memory could not be allocated (at most four times the shard's
 * nodes x 32 B, whatever n_pairs is). */
int pe_gang_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off /*[J+1]*/,
                        const int32_t* group_count /*[G]*/, const int64_t* group_req /*[G][4]*/,
                        const uint32_t* group_need /*[G] or NULL = 0*/,
                        int64_t n_pairs, const int32_t* pair_job /*[P]*/, const int32_t* pair_domain /*[P]*/,
                        int32_t level, int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                        const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                        uint8_t* out_fits /*[P] or NULL*/, int32_t* out_fail_group /*[P] or NULL*/,
                        int64_t* out_pods /*[P] or NULL*/, int32_t* out_first /*[J] or NULL*/);

/* (ABI 7, additive) First-fit placement of a batch over candidate domains: place each gang in the first of
 * its candidate domains that still holds it.  The batch form of the chain pe_gang_capacity_tree ->
 * pe_gang_fit_domains -> pe_place_greedy_domains, which is exact for one job at a time only: out_first is
 * judged "with no other job in the call", so two jobs may both be told that rack 7 is their first fit when
 * rack 7 holds one of them.  Here every job comes with an ordered list of candidate domains and is placed in
 * the first that fits the residuals AS THE EARLIER JOBS OF THE BATCH LEFT THEM (Kueue's "required: rack, try
 * these racks in this order").  NO reference function, as pe_place_greedy_domains.
 * Groups, counts, requests, needs, priority, pod slots, out_job_status and the in-place residuals mean what
 * they mean in pe_place_greedy_domains; levels, level_size, parent and dom_level(n) likewise; pair_job and
 * pair_domain mean what they mean in pe_gang_fit_domains: any order, ungrouped, repeats allowed, a job may
 * be in no pair.  A job's candidates are its pairs in ascending p.
 * The rule: jobs are handled in (priority desc, index asc) order.  Job j tries its candidates in order; an
 * attempt at pair p is exactly pe_place_greedy_domains on the single job j with job_domain = pair_domain[p],
 * against the residuals as they stand after every earlier job of that order.  The first attempt that returns
 * PE_JOB_PLACED stands: its pods stay and the residuals keep them.  A failed attempt is rolled back in full
 * before the next one.  A job whose candidates all fail, or that is in no pair (whatever its groups), is
 * PE_JOB_UNSCHEDULABLE with -1 in all its pod slots.  out_job_pair[j] = the pair that placed job j, or -1.
 * Two identities follow: with exactly one pair per job every output equals pe_place_greedy_domains with
 * job_domain[j] = pair_domain[pair of j]; with one job in the call out_job_pair[0] equals
 * pe_gang_fit_domains' out_first[0] on the same residuals.
 * The device runs the rule exactly, in rounds of one launch each, one workgroup per active domain; a
 * workgroup never waits for another.  At most n_pairs + 1 rounds are launched; a
 * batch that were not settled by then is PE_EHIP (never seen: the bound is proven).
 * After the call the device residuals and the host mirror both hold the new residuals; pe_reset_residuals
 * restores as usual and the staged fit batch stays valid.  pe_stats: adds to pods_placed, jobs_placed and
 * jobs_failed only.  n_jobs == 0 is PE_OK; n_pairs == 0 with jobs is PE_OK with every job unschedulable.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing changed and no output written (the first offending index in pe_last_error where there
 * is one): everything pe_place_greedy_domains refuses about the batch, the hierarchy and level, and
 * everything pe_gang_fit_domains refuses about the pairs.  PE_ESTATE: a call before pe_load_nodes. */
int pe_place_first_fit_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                               const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need /* or NULL = 0 */,
                               int64_t n_pairs, const int32_t* pair_job /*[P]*/, const int32_t* pair_domain /*[P]*/,
                               int32_t level, int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                               const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                               int32_t* out_pod_node, int32_t* out_job_status, int32_t* out_job_pair /*[J] or NULL*/);

/* (ABI 7, additive) Which gangs must go for a gang to fit: the question behind pe_gang_fit_domains' "no".  A
 * high-priority job finds its racks full; which of the lower-priority gangs already placed there would have
 * to be evicted for it to be placed in this rack, and which candidate rack needs the fewest evictions?  The
 * procedure is Kueue's and the kube-scheduler's: remove candidates in order until the incoming workload fits,
 * then put back those that were not needed.  NO reference function, as pe_gang_fit_domains.  Read-only.
 * The incoming jobs, levels, level_size, parent, dom_level(n), pair_job, pair_domain and the judgement "would
 * pe_place_greedy_domains, given this single job in this domain and no other job, return PE_JOB_PLACED" mean
 * exactly what they mean in pe_gang_fit_domains.
 * The victims are placed gangs in the shape the placement calls take and return: victim v has the groups
 * [vic_group_off[v], vic_group_off[v + 1]) with vic_group_count and vic_group_req, and vic_pod_node holds the
 * GLOBAL node id of every pod slot, groups in input order (a group of count c owns c slots), -1 = slot skipped.
 * Pair p comes with its candidate victims in eviction order: pair_vic[pair_vic_off[p] .. pair_vic_off[p + 1]),
 * K_p of them, each an index into the victims.
 * The residuals a judgement sees are R(E), for a set E of positions of pair p's list: the CURRENT residuals of
 * the domain's nodes, and for every position i in E every pod of victim pair_vic[pair_vic_off[p] + i] whose
 * node n has dom_level(n) == pair_domain[p] gives its group's request back to n in all four dimensions.
 * Victim pods on nodes outside the domain, on removed slots and slots holding -1 count nothing; an island
 * group of a victim is its pods like any other.  That victims really hold what they claim is the caller's
 * business: running pods live in `used`, not in the reset snapshot, so there is nothing to check it against.
 * The greedy best-fit rule is not monotone in the residuals (a release can make an earlier group choose another
 * node and a later group fail), so neither "release everything, then test" nor a bisection is exact; the
 * prefixes are walked in order:
 *   Phase 1   out_prefix[p] = the smallest k in [0, K_p] for which the job is placed against R({0 .. k-1}),
 *             the prefixes tried in ascending order; -1 when there is none.  k = 0 is pe_gang_fit_domains'
 *             out_fits[p].
 *   Phase 2   (fill-back; only when out_prefix[p] = k >= 2)  E = {0 .. k-1}; for i = k-2 down to 0: if the job
 *             is placed against R(E \ {i}) then E := E \ {i}.  Position k-1 is never tried.
 *   out_victims[p] = E as a bit mask over the list positions (bit i = position i); 0 when the prefix is 0 or -1
 *   out_count[p]   = the mask's popcount; -1 when the prefix is -1
 *   out_best[j]    = the pair of job j with the smallest out_count >= 0, ties to the smallest p; -1 when there
 *                    is none.  With empty lists it equals pe_gang_fit_domains' out_first.
 * A pair costs at most (K_p + 1) + max(0, k - 1) judgements.  out_best is computed on the device; a caller who
 * wants only the selection passes the three P-sized outputs NULL and they never cross.  Each out_* may be NULL;
 * group_need NULL = 0.  n_pairs == 0, n_jobs == 0 and n_victims == 0 are PE_OK (no pairs: out_best all -1).
 * A caller acts on the answer by evicting; the Node informer's PE_NODE_SET brings the new residuals, and
 * pe_place_greedy_domains then places the gang.
 * Read-only: the device residuals, the host mirror, the reset snapshot, the staged fit-mask state and pe_stats
 * are left exactly as they are, and the call keeps nothing between calls.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): everything
 * pe_gang_fit_domains refuses; about the victims' offsets, counts and requests everything pe_place_greedy
 * refuses about a batch's; a NULL vic_pod_node when some victim group has pods; a vic_pod_node outside
 * [-1, n_total); a NULL pair_vic_off with n_pairs > 0 or a pair_vic_off that does not rise from 0; a list
 * longer than PE_MAX_PAIR_VICTIMS; a pair_vic outside [0, n_victims); the same victim twice in one pair's
 * list (the same victim in many pairs is fine); and overflow: a node n that is not a removed slot and a
 * dimension d for which the current residual plus the requests of ALL the call's victim pods on n exceeds
 * INT64_MAX (so that no R(E) can overflow).  PE_ESTATE: a call before pe_load_nodes.  PE_ENOMEM: as
 * pe_gang_fit_domains. */
#define PE_MAX_PAIR_VICTIMS 64
int pe_gang_preempt_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off /*[J+1]*/,
                            const int32_t* group_count /*[G]*/, const int64_t* group_req /*[G][4]*/,
                            const uint32_t* group_need /*[G] or NULL = 0*/,
                            int64_t n_victims, const int32_t* vic_group_off /*[V+1]*/,
                            const int32_t* vic_group_count /*[VG]*/, const int64_t* vic_group_req /*[VG][4]*/,
                            const int32_t* vic_pod_node /*[sum of counts]: global node id per pod slot, -1 = skipped*/,
                            int64_t n_pairs, const int32_t* pair_job /*[P]*/, const int32_t* pair_domain /*[P]*/,
                            const int32_t* pair_vic_off /*[P+1]*/, const int32_t* pair_vic /*victim indices*/,
                            int32_t level, int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                            const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                            int32_t* out_prefix /*[P] or NULL*/, uint64_t* out_victims /*[P] or NULL*/,
                            int32_t* out_count /*[P] or NULL*/, int32_t* out_best /*[J] or NULL*/);

/* (ABI 7, additive) Give back and re-take placed gangs: the way back that the placement calls lack.  A gang
 * scheduler's Unreserve (Permit timed out, a bind failed) returns one gang exactly; a caller replays the
 * placements still in flight after pe_load_nodes or pe_reset_residuals; and the answer of
 * pe_gang_preempt_domains can be carried out on the engine (release the victims, place the gang) without
 * waiting for the Node informer.  NO reference function, as pe_place_greedy.
 * The gangs are placed gangs in the shape the placement calls take and return, exactly pe_gang_preempt_domains'
 * victims: gang v has the groups [gang_group_off[v], gang_group_off[v + 1]) with group_count and group_req,
 * and pod_node holds the GLOBAL node id of every pod slot, groups in input order (a group of count c owns c
 * slots), -1 = slot skipped.  The arguments and outputs of any placement call can be handed straight back.
 * Rule: for every pod slot whose node n is >= 0 and not a removed slot, in all four dimensions d,
 *   pe_release_gangs   res[n][d] += group_req[g][d]
 *   pe_assume_gangs    res[n][d] -= group_req[g][d]
 * Slots holding -1 and pods on removed slots count nothing (pe_gang_preempt_domains' R(E)), so the all -1 rows
 * of an unschedulable job are harmless.  *out_pods (or NULL) = the pod slots that did count.
 * All-or-nothing, validated in full before anything changes.  With sum[n][d] the call's total on node n, and
 * only in the dimensions with sum[n][d] > 0 (a dimension the call does not move is not looked at: cap - used may
 * legitimately be negative), products and sums formed in 128 bits so that nothing wraps:
 *   release is refused unless res[n][d] + sum[n][d] <= the reset snapshot of n (cap - used as last loaded or set):
 *           more is given back than was taken
 *   assume  is refused unless res[n][d] - sum[n][d] >= 0: the pods do not fit
 * A refusal is PE_EINVAL, pe_last_error names the offending node (the first at which the bound is crossed, in slot
 * order), nothing is changed and out_pods is not written.  pe_assume_gangs checks these totals ONLY: labels,
 * group needs and the best-fit rule are not consulted -- the caller vouches that the gangs sit where it says.
 * Consequences:
 *   - a placement call followed by pe_release_gangs of its own arguments and outputs leaves the residuals
 *     bit-equal to those before it;
 *   - pe_reset_residuals followed by pe_assume_gangs of the same placement gives the residuals the placement
 *     call left;
 *   - a release followed by an assume of the same gangs, or the other way round, is the identity;
 *   - PE_NODE_SET of a node folds the placements on it into `used` and the reset snapshot: a later release of
 *     them is refused, and the caller drops them.
 * After the call the device residuals and the host mirror hold the new values; the reset snapshot, labels,
 * islands, the staged fit batch and pe_stats are untouched, and the next pe_fit_mask_run, capacity call, what-if
 * or placement (greedy walk or full scan) sees the new residuals.
 * Sharded contexts: the calls work with world_size > 1.  Every rank makes the same call, as pe_update_nodes;
 * every rank validates against its mirror of the global inventory, so all ranks decide alike without any
 * exchange; every rank updates the whole mirror and, on the device, the nodes of its own shard.
 * PE_EINVAL, nothing changed (the first offending index in pe_last_error where there is one): n_gangs < 0;
 * everything pe_gang_preempt_domains refuses about its victims' offsets, counts and requests; a NULL pod_node
 * when some group has pods; a pod_node outside [-1, n_total); the two refusals above.  PE_ESTATE: a call before
 * pe_load_nodes.  n_gangs == 0 is PE_OK (*out_pods = 0).  PE_EHIP: as pe_place_greedy_domains, the mirror is not
 * committed and the device residuals of the touched nodes are undefined until pe_reset_residuals or
 * pe_load_nodes. */
int pe_release_gangs(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off /*[V+1]*/,
                     const int32_t* group_count /*[VG]*/, const int64_t* group_req /*[VG][4]*/,
                     const int32_t* pod_node /*[sum of counts]: global node id per pod slot, -1 = skipped*/,
                     int64_t* out_pods /* or NULL */);
int pe_assume_gangs(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off /*[V+1]*/,
                    const int32_t* group_count /*[VG]*/, const int64_t* group_req /*[VG][4]*/,
                    const int32_t* pod_node /*[sum of counts]: global node id per pod slot, -1 = skipped*/,
                    int64_t* out_pods /* or NULL */);

/* (ABI 7, additive) Why a pod shape fits no node, counted per reason: the numbers behind the Unschedulable
 * condition a gang scheduler owes its users on the PodGroup and the job -- kube-scheduler's "0/5000 nodes are
 * available: 3200 Insufficient amd.com/gpu, 1800 node(s) didn't match ..." -- and behind the two decisions
 * that follow a "no": preemption helps only on nodes that fail on resources alone, and a scale-up is sized by
 * how much the nearest miss lacks.  NO reference function, as all of fit and placement.  Read-only.
 * With residuals, labels and removed slots exactly as pe_fit_mask sees them now, the SIGNATURE of (job j,
 * node n) is a 5-bit value:
 *   bit d (d = 0 .. 3)          set iff req[j][d] > res[n][d]  (signed int64: a zero request is still
 *                               insufficient on a negative residual; the negation of fit's req_d <= res_d)
 *   bit 4 (PE_EXPLAIN_LABELS)   set iff (labels[n] & need[j]) != need[j]  (bit 31 is the engine's island bit,
 *                               matched like any label bit)
 * Signature 0 is fit(j, n).  A node is LIVE iff its slot is not removed and it lies in this shard; removed
 * slots and padding count nowhere.
 *   out_hist[j][s], s in 0 .. 31 = the live nodes in job j's scope with signature s
 *   out_near[j][d]               = min over the live nodes in scope whose signature is exactly 1 << d of
 *                                  req[j][d] - res[n][d], as an exact unsigned 64-bit value in [1, 2^64 - 2]
 *                                  (a residual of -(2^63 - 1) against a request of 2^63 - 1 does not wrap);
 *                                  0 when there is no such node
 * Scope: job_domain NULL -- every live node of the shard, with or without an island.  Otherwise level,
 * n_levels, level_size, parent and dom_level(n) mean exactly what they mean in pe_place_greedy_domains, and job
 * j counts only the nodes with dom_level(n) == job_domain[j]; job_domain[j] == PE_EXPLAIN_ANY is the whole
 * shard for that job.  Nothing of the hierarchy is kept in the context.
 * Worked example: the job (4000 m cpu, 64 Gi memory, 8 GPUs, 0 ephemeral) with need = bit 0, and the nodes, as
 * free (cpu, memory Gi, GPUs): n0 (8000, 128, 8) with bit 0 -> 0; n1 (8000, 128, 4) with bit 0 -> 4; n2 (2000,
 * 32, 0) with bit 0 -> 7; n3 (8000, 128, 8) without labels -> 16; n4 (8000, 128, 6) with bit 0 -> 4; n5 removed
 * -> not counted.  out_hist = {0: 1, 4: 2, 7: 1, 16: 1}, 5 live nodes, out_near = {0, 0, 2, 0}; inclusive
 * counts: cpu 1, memory 1, gpu 3, ephemeral 0, labels 1 -- "1/5 nodes are available: 1 Insufficient cpu, 1
 * Insufficient memory, 3 Insufficient amd.com/gpu, 1 node(s) didn't match the required labels."
 * Identities:
 *   - out_hist[j][0] is pe_fit_mask's count and pe_gang_capacity's out_nodes for the same row;
 *   - the sum over s of out_hist[j][s] is the number of live nodes in scope;
 *   - the INCLUSIVE count of reason r is the sum over the s with bit r set: a node lacking cpu and gpu counts
 *     under both, as kube-scheduler reports it; bin 1 << d holds the nodes that fail on dimension d ALONE;
 *   - the domain form summed over every domain of a level, plus the nodes in no domain of that level, is the
 *     unrestricted form.
 * Sharded contexts: the call works with world_size > 1; the tables are per shard, like pe_gang_capacity's
 * counts.  The caller adds the histograms and takes the minimum of the non-zero near values.
 * The device residuals, the host mirror, the reset snapshot, the staged fit-mask state and pe_stats are
 * untouched.  need NULL = 0; each out_* may be NULL (without out_near the near values are not computed).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): n_jobs < 0; a
 * negative request; and with job_domain given: everything pe_gang_capacity_tree refuses about the hierarchy,
 * level outside [0, n_levels), a job_domain outside [-1, level_size[level]).  With job_domain NULL the four
 * hierarchy arguments are not read.  PE_ESTATE: a call before pe_load_nodes.  n_jobs == 0, an empty shard and
 * a domain without nodes are PE_OK with zeros. */
#define PE_EXPLAIN_BINS 32
#define PE_EXPLAIN_LABELS 4   /* signature bit of the label test */
#define PE_EXPLAIN_ANY (-1)
int pe_fit_explain(pe_ctx* ctx, int64_t n_jobs, const int64_t* req /*[j][4]*/, const uint32_t* need /* or NULL = 0 */,
                   const int32_t* job_domain /*[j] or NULL = whole shard*/, int32_t level, int32_t n_levels,
                   const int32_t* level_size, const int32_t* parent,
                   int64_t* out_hist /*[j][32] or NULL*/, uint64_t* out_near /*[j][4] or NULL*/);

/* (ABI 7, additive) Can a node's pods move elsewhere, and where: the question about pods that are already
 * placed.  Maintenance (cordon and drain before a firmware update: which of these nodes can go now without
 * killing a gang?), defragmentation (free whole nodes by moving the small pods that sit on them) and a node hot
 * swap (a replacement inside the same rack) all ask it, and without this call the only way to learn the answer
 * is to remove the node, place its pods and reload.  NO reference function, as pe_gang_fit_domains.  Read-only.
 * The residents are placed gangs in exactly the shape pe_release_gangs takes -- gang v has the groups
 * [gang_group_off[v], gang_group_off[v + 1]) with group_count and group_req, pod_node holds the GLOBAL node id of
 * every pod slot, groups in input order, -1 = slot skipped; S = the sum of the counts -- plus the groups' need: a
 * move respects labels, which a release never looks at.  A caller may hand over its whole book of placed gangs;
 * slots on nodes that are no candidate are ignored.  Levels, level_size, parent and dom_level(n) mean exactly what
 * they mean in pe_place_greedy_domains; nothing is kept in the context; one call has one level.
 * Candidate c, with n = cand_node[c] and D = cand_domain[c], is judged alone against the CURRENT residuals:
 *   Evicted pods   the pod slots s with pod_node[s] == n, in ascending s: gang order, group order, slot order.
 *   Runs           consecutive evicted slots of one group form a RUN of r pods of that group's request and need:
 *                  the pods of a group are identical, so the run is a group of count r.  A run of a group whose
 *                  need has PE_NEED_ISLAND moves as one unit of r x request onto one node (a product that
 *                  overflows fits nowhere): the island group of every placement call.
 *   The move       the answer is what pe_place_greedy_domains would give for the single job whose groups are the
 *                  runs in that order, with job_domain = D, on an inventory in which slot n is a removed slot and
 *                  every other node has its current residual.  Node n is out of every decision, whether or not
 *                  it lies in D, and nothing is given back to it: it is gone.  D need not be n's own domain:
 *                  "into the same rack" is D = n's rack, "out of this rack" is another one.
 * A candidate that is itself a removed slot: its pods count nothing (the ledger's rule); it fits with 0 pods.
 *   out_fits[c]      = 1 or 0
 *   out_moved[c]     = the pods that had found a node when the rule stopped: all of them when the candidate fits;
 *                      a failing island run contributes 0
 *   out_fail_slot[c] = -1 when it fits, else the slot index, in pod_node, of the first pod that found no node
 *                      (for an island run, the run's first slot)
 *   out_target[s]    = for every slot of the call: the GLOBAL node the pod of slot s moves to when its node is a
 *                      candidate that fits, -1 otherwise (slots on non-candidates, slots holding -1, slots on
 *                      removed nodes and every slot of a candidate that does not fit); every cell is written
 * A candidate without pods fits with 0 pods; a domain with no node other than n holds only a candidate without
 * pods.  n_cands == 0 and n_gangs == 0 are PE_OK, with every out_target -1.  Each out_* may be NULL; group_need
 * NULL = 0.
 * Worked example: one rack holds A, B and C; B has 3 free GPUs and C has 4, cpu and memory equal and ample.  A
 * holds three pods in slot order: two of one group of 2 GPUs each, then one of another group with 3 GPUs.  Drain
 * A: the first 2-GPU pod takes B (the best fit, 1 left), the second takes C (2 left), the 3-GPU pod finds
 * nothing -- fits 0, moved 2, fail_slot 2, all targets -1.  With the 3-GPU gang first in the book it takes B and
 * the two 2-GPU pods take C -- fits 1, moved 3, targets (B, C, C).  The answer is the greedy rule's in the
 * caller's slot order, not a bin-packing optimum: the caller orders the book.
 * Acting on the answer: pe_release_gangs of the candidate's slots, then pe_assume_gangs of the same groups with
 * pod_node = the targets.  Two candidates of one call may have been given the same free slots: act on one, then
 * ask again.
 * Read-only: the device residuals, the host mirror, the reset snapshot, labels and islands, the staged fit batch
 * and pe_stats are left exactly as they are.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one): everything
 * pe_release_gangs refuses about offsets, counts, requests and pod_node; more than 2^31 - 1 pod slots; n_cands
 * outside [0, 2^31 - 1); a NULL cand_node or cand_domain with n_cands > 0; a cand_node outside [0, n_total); the
 * same node twice in cand_node (one target per slot is only defined then; several target domains for one node
 * are several calls); everything pe_gang_fit_domains refuses about the hierarchy and level; a cand_domain outside
 * [0, level_size[level]).  PE_ESTATE: a call before pe_load_nodes.  PE_ENOMEM: as pe_gang_fit_domains. */
int pe_drain_fit_domains(pe_ctx* ctx, int64_t n_gangs, const int32_t* gang_group_off /*[V+1]*/,
                         const int32_t* group_count /*[VG]*/, const int64_t* group_req /*[VG][4]*/,
                         const uint32_t* group_need /*[VG] or NULL = 0*/,
                         const int32_t* pod_node /*[S]: global node id per pod slot, -1 = skipped*/,
                         int64_t n_cands, const int32_t* cand_node /*[C]*/, const int32_t* cand_domain /*[C]*/,
                         int32_t level, int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                         const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                         uint8_t* out_fits /*[C] or NULL*/, int64_t* out_moved /*[C] or NULL*/,
                         int64_t* out_fail_slot /*[C] or NULL*/, int32_t* out_target /*[S] or NULL*/);

/* (ABI 7, additive) Fewest new nodes for a gang to fit a domain: the question that follows pe_gang_fit_domains' "no"
 * when nothing can be evicted.  How many nodes of THIS node type would have to join THIS rack for the gang to be
 * placed there, and which (node type, rack) choice needs the fewest?  It is the cluster autoscaler's scale-up
 * simulation (binpacking estimator, "least nodes" expander) and what Kueue's provisioning request asks before it
 * admits a gang; without this call the only way to learn the answer is PE_NODE_SET of k template nodes, a
 * pe_gang_fit_domains and PE_NODE_REMOVE, once per k.  NO reference function, as pe_gang_fit_domains.  Read-only.
 * Jobs, groups, counts, requests, needs, pair_job, pair_domain, level, level_size, parent and dom_level(n) mean
 * exactly what they mean in pe_gang_fit_domains, and so does the judgement: would pe_place_greedy_domains, given
 * this single job in this domain and no other job, return PE_JOB_PLACED?
 *   Templates   tmpl_res[t] is the free residual of a fresh node of type t (cap - used with the daemonsets
 *               counted, every cell >= 0), tmpl_labels[t] its labels.
 *   New slots   new_slot lists the free slots the caller's Node informer would hand to new nodes, in the order it
 *               would hand them out: each in [0, n_total), a removed slot now, named once.  The i-th new node of
 *               ANY pair has id new_slot[i]; ids matter because the Appendix-B key breaks score ties by node id.
 *   Attempt k   of pair p, 0 <= k <= K_p = pair_max[p], is the judgement on a widened inventory: the nodes of
 *               domain pair_domain[p] with their CURRENT residuals plus k further members of the domain, new node
 *               i < k with residual tmpl_res[pair_template[p]], labels tmpl_labels[...] | PE_LABEL_ISLAND (a node
 *               in a domain has an island; the caller's bit 31 is replaced) and id new_slot[i].  Every attempt
 *               starts from fresh residuals, real and new.  Equivalently: what pe_gang_fit_domains answers for
 *               (job, domain) after PE_NODE_SET put the template on new_slot[0 .. k) with used 0 and an island
 *               that is a leaf under the domain.
 * The answer is NOT monotone in k, so the attempts are tried in ascending order and the first that places the job
 * is the answer -- no bisection, no try from the top:
 *   out_nodes[p]      = the smallest k in [0, K_p] whose attempt places the job, -1 when there is none.  With
 *                       K_p = 0 it is pe_gang_fit_domains' out_fits[p] - 1.
 *   The DECIDING attempt is k = out_nodes[p], or attempt K_p when the answer is -1.
 *   out_fail_group[p],
 *   out_pods[p]       = pe_gang_fit_domains' two outputs for the deciding attempt: -1 and the job's pod total when
 *                       the pair is answered, else what still does not fit with every allowed node present (a
 *                       group larger than the template shows here)
 *   out_new_pods[p]   = the pods of the deciding attempt that sit on new nodes (an island group: its count)
 *   out_best[j]       = the pair of job j with the smallest out_nodes >= 0, ties to the smallest p, -1 when there
 *                       is none.  With every K_p = 0 it equals pe_gang_fit_domains' out_first.
 * out_best is computed on the device; a caller who wants only the selection passes the four P-sized outputs NULL
 * and nothing P-sized crosses.  Each out_* may be NULL; group_need NULL = 0, tmpl_labels NULL = 0, pair_max NULL =
 * n_new for every pair.
 * A domain without nodes is a legitimate pair: with k >= 1 it holds what k template nodes hold.  Pairs are judged
 * alone: two pairs may be promised the same new nodes, so act on one and ask again.  n_pairs == 0 and n_jobs == 0
 * are PE_OK (with n_jobs > 0 and no pairs out_best is all -1).
 * Worked example: a rack holds one node with 8 free GPUs, the template has 4 GPUs, the job is A = 1 x 4 GPUs
 * followed by B = 1 x 8 GPUs.  k = 0: A takes the only node and B fails.  k = 1: A takes the new node, the
 * tightest fit, and B takes the old one -- out_nodes 1, out_new_pods 1.
 * A non-monotone case (cpu m, GPUs; memory and storage 0): a rack of two nodes with (15000, 8) and (14000, 7) free,
 * the template (9000, 2), new ids above the real ones, and the job 2 x (6000, 1), 1 x (7000, 7), 1 x (2000, 1),
 * 2 x (8000, 0).  It is placed with k = 1, 3 and 4 new nodes and NOT with k = 0 or 2: out_nodes 1.
 * Acting on the answer: once the nodes have arrived (PE_NODE_SET), pe_place_greedy_domains gives the pods' nodes.
 * Read-only: the device residuals, the host mirror, the reset snapshot, labels and islands, the staged fit batch
 * and pe_stats are left exactly as they are, and nothing is kept between calls.
 * Sharded contexts: with world_size > 1 the call is PE_EINVAL (a domain may span shards).
 * PE_EINVAL, nothing written (the first offending index in pe_last_error where there is one), checked in this
 * order: everything pe_gang_fit_domains refuses; n_templates < 0, or < 1 with pairs; a NULL tmpl_res with
 * templates; a negative tmpl_res cell; n_new outside [0, PE_MAX_SCALE_NODES]; a NULL new_slot with n_new > 0; a
 * new_slot that is out of range, not a removed slot, or repeated; a NULL pair_template with pairs; a pair_template
 * outside [0, n_templates); a pair_max outside [0, n_new].  PE_ESTATE / PE_ENOMEM: as pe_gang_fit_domains. */
#define PE_MAX_SCALE_NODES 64
int pe_scale_up_domains(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off /*[J+1]*/,
                        const int32_t* group_count /*[G]*/, const int64_t* group_req /*[G][4]*/,
                        const uint32_t* group_need /*[G] or NULL = 0*/,
                        int32_t n_templates, const int64_t* tmpl_res /*[T][4]*/, const uint32_t* tmpl_labels /*[T] or NULL = 0*/,
                        int32_t n_new, const int32_t* new_slot /*[n_new]*/,
                        int64_t n_pairs, const int32_t* pair_job /*[P]*/, const int32_t* pair_domain /*[P]*/,
                        const int32_t* pair_template /*[P]*/, const int32_t* pair_max /*[P] or NULL = n_new*/,
                        int32_t level, int32_t n_levels, const int32_t* level_size /*[n_levels]*/,
                        const int32_t* parent /* as pe_gang_capacity_tree; NULL allowed when n_levels == 1 */,
                        int32_t* out_nodes /*[P] or NULL*/, int32_t* out_fail_group /*[P] or NULL*/,
                        int64_t* out_pods /*[P] or NULL*/, int64_t* out_new_pods /*[P] or NULL*/,
                        int32_t* out_best /*[J] or NULL*/);

/* ---- Host resolver: the host half of pe_place_greedy, exposed on its own so a caller (or a
 * CPU test) can drive the windowed protocol with candidate blobs it obtained elsewhere, e.g. one
 * blob per shard gathered over any transport.  No device is touched.
 * Window blob layout (what the device merge kernel writes, per shard, per window group):
 *   16-B header {int32 n; int32 flags; uint64 limit} + K records of 48 B
 *   {uint64 key; int64 res[4]; uint64 labels}; shards are concatenated.
 * Updates are returned as [n][5] int64 {global node id, res[0..3]} (absolute residuals).
 * An island group's (PE_NEED_ISLAND) lists must be scanned for group_count x request. */
typedef struct pe_resolver pe_resolver;
int pe_resolver_create(int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                       const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                       pe_resolver** out);
void pe_resolver_destroy(pe_resolver* r);
/* (ABI 7) Inventory size for the id checks below (default PE_MAX_NODES).  Blobs may arrive over any
 * transport, so pe_resolver_resolve* validate every header and record before the resolver moves: a
 * header count outside [0, topk], a listed node id >= n_nodes or keys not strictly ascending within a
 * shard list (and a seed id >= n_nodes) return PE_EINVAL with no update written and the resolver's
 * position unchanged -- never a read past the blob. */
int pe_resolver_set_nodes(pe_resolver* r, int64_t n_nodes);
int pe_resolver_done(const pe_resolver* r); /* 1 when every job is decided */
int pe_resolver_next_window(pe_resolver* r, int32_t max_groups, int64_t max_pods, int32_t* out_groups,
                            int32_t* out_n);
int pe_resolver_resolve(pe_resolver* r, int32_t n_groups, const int32_t* groups, const uint8_t* blob,
                        int32_t n_shards, int32_t topk, int64_t* out_updates, int64_t max_updates,
                        int64_t* out_n_updates, int32_t* out_consumed);
/* Pipelined form (what pe_place_greedy does internally): the blob's lists were scanned on a
 * snapshot that misses some changes; seeds [n_seeds][6] = {global node id, res[0..3], labels} are
 * every node changed since that snapshot, with its CURRENT state (e.g. the previous window's
 * updates).  They count as dirty for the whole window and are scored by a helper thread ahead of
 * the resolution.  Updates returned as by pe_resolver_resolve (nodes this window changed). */
int pe_resolver_resolve_seeded(pe_resolver* r, int32_t n_groups, const int32_t* groups, const uint8_t* blob,
                               int32_t n_shards, int32_t topk, int64_t n_seeds, const int64_t* seeds,
                               int64_t* out_updates, int64_t max_updates, int64_t* out_n_updates,
                               int32_t* out_consumed);
int pe_resolver_results(const pe_resolver* r, int32_t* out_pod_node, int32_t* out_job_status);

int pe_synchronize(pe_ctx* ctx);
void* pe_stream(pe_ctx* ctx); /* hipStream_t the context launches on (for event timing) */
int pe_get_stats(const pe_ctx* ctx, pe_stats* out);
int pe_reset_stats(pe_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PLACEMENT_H_ */
