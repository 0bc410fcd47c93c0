// Device-side building blocks of libplacement (gfx950).  Host code in pe_engine.cpp, pe_engine_greedy.cpp,
// pe_engine_capacity.cpp, pe_engine_place.cpp and pe_engine_fit.cpp launches these through the wrappers below;
// nothing here is part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pe {

constexpr int D = 4;                    // cpu milli, memory B, gpu count, ephemeral-storage B
constexpr uint64_t SCORE_MAX = (1ull << 40) - 1;
constexpr uint64_t NO_KEY = ~0ull;
constexpr int64_t NEVER = INT64_MIN;    // residual of padding nodes: nothing fits

// One request vector (a pod template / a fit-mask job), 64 B so a wave loads it with one
// scalar s_load_dwordx16 and it never straddles two scalar-cache lines.
struct alignas(64) ReqRec {
  int64_t q[D];
  uint32_t need;
  uint32_t pad_[7];
};
static_assert(sizeof(ReqRec) == 64, "ReqRec must be 64 B");

// Exact 32-bit form of a request batch: q32[d] = q[d] >> shift[d] where 2^shift[d] divides every
// request of the batch in dim d, so  q <= r  <=>  q32 <= sat32(floor(r / 2^shift))  (r's floor
// loses nothing because q is a multiple of 2^shift; r >= 2^31 saturates, r < 0 becomes -1).
struct alignas(32) ReqRec32 {
  int32_t q[D];
  uint32_t need;
  uint32_t pad_[3];
};
static_assert(sizeof(ReqRec32) == 32, "ReqRec32 must be 32 B");

// Per-group candidate list shipped to the host resolver: a header + K keys (ascending).  The keys
// carry the node id (low 24 bits); the host reads the node's residual snapshot from its own mirror
// of the inventory, so the device ships 8 B per candidate instead of a 48-B record.
struct CandHdr {
  int32_t n;       // valid keys (ascending)
  int32_t flags;   // merge: bit0 = overflowed LDS, list truncated to the exact minimum; signalled walk: the window generation, written last
  uint64_t limit;  // every clean node with key < limit is in the list
};
static_assert(sizeof(CandHdr) == 16, "CandHdr must be 16 B");
// CandHdr.n values that are not a count: a zero-copy exchange wait timed out (limit = the xwait status),
// and a merged group one of whose shard lists was corrupt (a shard header with n outside [0, K]).  The
// host resolver raises on either (pe_resolver.cpp parse_group_keys); it never reads past a list.
constexpr int32_t CAND_TIMEOUT = -1;
constexpr int32_t CAND_CORRUPT = -2;

__host__ __device__ inline size_t cand_group_bytes(int K) { return sizeof(CandHdr) + (size_t)K * sizeof(uint64_t); }

// ---- geometry shared by host and device
constexpr int FM_CH = 4;       // fit mask: 64-node chunks per wave tile (256 nodes in VGPRs)
constexpr int FM_JT = 256;     // fit mask: jobs per wave
constexpr int SC_M = 16;       // scan: nodes per lane (wave span 1024 nodes)
constexpr int SC_GT = 4;       // scan: groups per wave (top-2 state in registers)
constexpr int SC_SPAN = 64 * SC_M;
constexpr int SC_WPB = 16;     // scan: waves (group tiles) per block, all on one node span
constexpr int MG_CAP = 16384;  // merge / walk: LDS candidate capacity per group (128 KiB of keys)
constexpr int MG_THREADS = 1024;
constexpr int MG_SEL = 1024;   // merge: keys kept after the histogram cut (sorted instead of all)

// ---- PodGroup aggregation call path (pe_pg_min_resources).  The host packs the batch into
// SEGMENTS in one pinned, device-mapped staging buffer: a segment holds up to AGG_SEG_JOBS
// consecutive jobs with their groups and containers, offsets rebased to the segment, every
// section 16-B aligned, so one block copies its whole segment into LDS with one round trip of
// coalesced 16-B loads and runs one job per lane from LDS -- reading the pinned buffer over PCIe for
// calls up to 8192 jobs, a device copy (one DMA per chunk) for larger ones.  Outputs go straight into
// a pinned output buffer in the caller's layout.  A segment larger than AGG_SEG_BYTES (one job with
// very many groups / containers) is read in place.
constexpr int AGG_SEG_JOBS = 256;
constexpr int64_t AGG_SEG_BYTES = 48 * 1024;
struct AggSegHdr {
  int64_t j0;            // first job of the segment (index in the call's batch)
  int32_t nj, ng, nc;    // jobs, groups, containers
  int32_t g0, c0;        // the segment's first group / container: its jgo / gco sections hold the caller's
                         // absolute offsets (copied as they are), the kernel rebases
  int32_t narrow;        // 1: the request section is narrowed (agg_seg_layout), 0: nc x nd i64
};
static_assert(sizeof(AggSegHdr) == 32, "AggSegHdr must be 32 B");
__host__ __device__ inline int64_t agg_r16(int64_t x) { return (x + 15) & ~int64_t(15); }
// Key layout of a call: nd int64 values per container record and per job result, fb bytes of flags
// per container.  {4, 1}: the fixed engine dimensions (pe_pg_min_resources: presence bits 0-3 | kind
// << 4, u8 presence out); {4 | 8 | 16, 4}: a per-call key table (pe_pg_min_resources_keys: presence
// bits 0-15 | kind << 16, u16 presence out), n_keys rounded up to nd.
struct AggKeys {
  int nd = 4;
  int fb = 1;
};
constexpr int AGG_MAX_KEYS = 16;
// byte offsets of the sections in a segment: [0] jgo (nj+1 i32, absolute group ids), [1] min_member
// (nj i32, V1 only), [2] replicas (ng i32), [3] gco (ng+1 i32, absolute container ids), [4] req
// (nc x nd i64; narrowed: 16 shift bytes, then nc x nd u32), [5] flags (nc x fb), [6] = size.
// A narrowed request section holds value >> shift[key] in 32 bits, shift[key] = the fewest trailing
// zero bits of the key's values in the segment -- exact whenever every value of a key spans <= 32 bits
// above its shift (quantities in canonical units are: milli-cpu, memory in multiples of 2^k bytes),
// and half the bytes over PCIe.  The host narrows a segment only when it can, and when it pays.
__host__ __device__ inline int64_t agg_req_bytes(int64_t nc, int nd, bool narrow) {
  return narrow ? 16 + agg_r16(nc * 4 * nd) : nc * 8 * nd;
}
__host__ __device__ inline void agg_seg_layout(int64_t nj, int64_t ng, int64_t nc, bool v1, int64_t off[7],
                                               AggKeys ak = AggKeys{}, bool narrow = false) {
  off[0] = (int64_t)sizeof(AggSegHdr);
  off[1] = off[0] + agg_r16((nj + 1) * 4);
  off[2] = off[1] + (v1 ? agg_r16(nj * 4) : 0);
  off[3] = off[2] + agg_r16(ng * 4);
  off[4] = off[3] + agg_r16((ng + 1) * 4);
  off[5] = off[4] + agg_req_bytes(nc, ak.nd, narrow);
  off[6] = off[5] + agg_r16(nc * ak.fb);
}
// Output buffer layout (the caller's arrays back to back): res [J][nd] i64, members [J] i32,
// present [J] (u8, or u16 for a key table), overflow [J] u8, each 16-B aligned.
__host__ __device__ inline void agg_out_layout(int64_t J, int64_t off[4], AggKeys ak = AggKeys{}) {
  off[0] = 0;
  off[1] = agg_r16(J * 8 * ak.nd);
  off[2] = off[1] + agg_r16(J * 4);
  off[3] = off[2] + agg_r16(J * (ak.fb == 1 ? 1 : 2));
}

// ---- launch wrappers (return hipError_t of the launch)
// Segmented aggregation: nseg segments; segment s spans blob[seg_off[s], seg_off[s+1]) (seg_off
// may be NULL for one segment of nbytes0 bytes at blob[0]).  out = output buffer (agg_out_layout,
// J jobs).  flag != NULL (latency launches): every block publishes its outputs system-wide and counts
// itself in done_ctr (device memory, 0 between launches; unused for one block); the last one resets
// it and stores flag_val (release, system scope) -- the host waits on the flag, not on the stream.
hipError_t launch_pg_agg_segments(hipStream_t s, int mode, const uint8_t* blob, const int64_t* seg_off, int64_t nseg,
                                  int64_t nbytes0, uint8_t* out, int64_t J, uint32_t* flag, uint32_t flag_val,
                                  uint32_t* done_ctr, AggKeys ak = AggKeys{});
// One segment of <= AGG_KARG_BYTES (a multiple of 16) passed by value in the kernel arguments.
constexpr int64_t AGG_KARG_BYTES = 512;   // (a 3 KB argument block cost ~1.5 us more per launch call)
struct AggKarg {
  alignas(16) uint8_t b[AGG_KARG_BYTES];
};
hipError_t launch_pg_agg_karg(hipStream_t s, int mode, const AggKarg& blob, int64_t nbytes, uint8_t* out, int64_t J,
                              uint32_t* flag, uint32_t flag_val, AggKeys ak = AggKeys{});
hipError_t launch_pg_min_resources(hipStream_t s, int mode, int64_t n_jobs, const int32_t* job_group_off,
                                   const int32_t* min_member, const int32_t* group_replicas,
                                   const int32_t* group_cont_off, const int64_t* cont_req,
                                   const uint8_t* cont_flags, int64_t* out_res, uint8_t* out_present,
                                   int32_t* out_members, uint8_t* out_overflow);
// 128-bit aggregation of a compact CSR sub-batch (device-resident, offsets rebased to it), one lane per
// (job, key) pair: requests req_hi * 2^64 + req_lo ([C][n_keys]; req_hi NULL = 0), results out_hi:out_lo
// [n_jobs][n_keys] as signed 128-bit two's complement, out_flag [n_jobs][n_keys] = 1 where an
// intermediate of the pair left [-2^127, 2^127) (its value is then 0).
hipError_t launch_pg_agg_wide(hipStream_t s, int mode, int64_t n_jobs, int n_keys, const int32_t* job_group_off,
                              const int32_t* min_member, const int32_t* group_replicas,
                              const int32_t* group_cont_off, const uint64_t* req_lo, const uint64_t* req_hi,
                              const uint32_t* cont_flags, uint64_t* out_lo, int64_t* out_hi, uint8_t* out_flag);

// Device mask layout (tile-major, so every store writes whole 128-B lines): tiles of 16 jobs x 4
// words (256 nodes); word (j, c) -- bit n%64 of chunk c = n/64 = fit(job j, local node n) -- sits at
//   ((j / 16) * Wt + c / 4) * 64 + (j % 16) * 4 + c % 4,      Wt = ceil(ceil(Ns/64) / 4).
// Rows are padded to FM_JT, chunks to a multiple of 4; pe_fit_mask_rows returns row-major.
__host__ __device__ inline int64_t fm_word_index(int64_t j, int64_t c, int64_t Wt) {
  return ((j >> 4) * Wt + (c >> 2)) * 64 + (j & 15) * 4 + (c & 3);
}
hipError_t launch_fit_mask(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                           int64_t Ns, int64_t Wt, const ReqRec* jobs, int64_t J, int64_t tiles_per_wave,
                           uint64_t* mask, unsigned long long* counts);

// 32-bit path: residuals compressed per fit run (res32 = sat32(res >> shift)), then the same kernel
// with v_cmp_le_i32 instead of the (quarter-rate) v_cmp_le_i64.
hipError_t launch_compress_res(hipStream_t s, const int64_t* res, int32_t* res32, int64_t stride, int64_t Ns,
                               const int* shift);
hipError_t launch_fit_mask32(hipStream_t s, const int32_t* res32, int64_t stride, const uint32_t* labels,
                             int64_t Ns, int64_t Wt, const ReqRec32* jobs, int64_t J, int64_t tiles_per_wave,
                             uint64_t* mask, unsigned long long* counts);

// ---- dictionary-coded SWAR path (fit mask).  Per batch the host ranks the distinct request
// values of each dimension (and a chain of label needs); field f of a node's 32-bit code word is
// (#batch values <= residual) + guard bit, the job's word holds its values' ranks.  Then
//   fit(j, n)  <=>  ((X[n] - C[j]) | ~M) == 0xFFFFFFFF   (every field keeps its guard bit)
// exactly, for all 4 dimensions and the labels at once.
constexpr int CODE_FIELDS = 5;   // cpu, memory, gpu, ephemeral, label-chain
constexpr int CODE_MAXV = 128;   // distinct values per field the device tables hold
struct CodeSpec {
  int off[CODE_FIELDS];
  int width[CODE_FIELDS];       // SWAR: code bits + 1 guard bit; thermometer: nvals bits
  int nvals[CODE_FIELDS];
  uint32_t guard;               // SWAR: M (guard bits); thermometer: unused
  int therm;                    // 1: thermometer fields, fit <=> (X | ~Y) == ~0 (3 VALU per 64 evals)
};
constexpr int FC_CH = 16;       // coded fit: 64-node chunks per wave tile (X in 16 VGPRs)
constexpr int FC_JT = 64;       // coded fit: jobs per wave (one 64-bit word per node)

// vals: [4][CODE_MAXV] sorted int64 request values; needs: [CODE_MAXV] label chain (inclusion order)
hipError_t launch_encode_nodes(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                               int64_t n_pad, CodeSpec spec, const int64_t* vals, const uint32_t* needs, uint32_t* X);
// Coded-path mask layout (bits over jobs): word (b, n) = jobs 64b..64b+63 at node n (bit j%64),
// stored at b * node_stride + n, node_stride = ceil(Ns/1024)*1024 (whole wave tiles of FC_CH chunks).
// therm = 0: jcode = C (ranks), k = ~M;   therm = 1: jcode = ~Y (one bit per field cleared), k unused
hipError_t launch_fit_mask_coded(hipStream_t s, int therm, const uint32_t* X, int64_t Ns, int64_t node_stride,
                                 const uint32_t* jcode, uint32_t not_guard, int64_t J, int64_t tiles_per_wave,
                                 uint64_t* mask, unsigned long long* counts);

// ---- bit-plane path (fit mask).  Per batch the host lists the distinct request values of each
// dimension and the distinct label needs; plane p of a node is one predicate, evaluated exactly in
// int64 when the planes are encoded:
//   kind d < 4:  res[d][n] >= val        kind 4:  (labels[n] & need) == need
// and is stored transposed, 32 nodes per u32 word (padding nodes 0).  A job selects one plane per
// dimension and one for its need, so for 32 nodes at once
//   fit word = P[i0] & P[i1] & P[i2] & P[i3] & P[i4]
// -- two v_bitop3 per 2048 (job, node) pairs per wave instead of one VALU op per 64.
constexpr int PL_MAX = 32;      // planes a batch may use (held in VGPRs, dynamic index via gpr_idx)
constexpr int PL_R = 4;         // u32 node words per lane: one 16-B store per job and lane
constexpr int PL_BLK = 64 * PL_R * 32;   // nodes per wave block (8192)
struct PlaneSpec {
  int32_t n;                    // planes in use
  int32_t kind[PL_MAX];         // 0..3 resource dimension, 4 label need
  int64_t val[PL_MAX];          // request value (kind < 4) or need bits (kind 4)
};
// planes: [nblk][PL_MAX][64 * PL_R] u32; word w of block b covers nodes b*PL_BLK + 32w .. +31
hipError_t launch_encode_planes(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                int64_t Ns, int64_t nblk, const PlaneSpec& spec, const PlaneSpec* spec_d,
                                uint32_t* planes, unsigned long long* zero = nullptr,
                                int64_t n_zero = 0);   // spec_d: the same spec on the device; + zero[0..n_zero)
// jcode[j] = 5 fields of 7 bits (dims 0..3 at bits 0/7/14/21, need at bit 32), each 4 x the plane index.  Mask block-major:
// u32 word w of row j (nodes 32w..32w+31) at (w / 256 * J + j) * 256 + w % 256, i.e. per 8192-node
// block a [J][1 KiB] slab.
hipError_t launch_fit_mask_planes(hipStream_t s, const uint32_t* planes, int64_t nblk, const uint64_t* jcode,
                                  int64_t J, int64_t jobs_per_wave, uint32_t* mask, unsigned long long* counts);
// Row-major form (the default): nblk x R persistent waves, one per SIMD, R job phases; wave
// (blk, r) takes jobs r, r+R, ...; u32 word w of row j at j * nblk * 256 + w.  jcode and counts are
// phase-major: entry r * Jr + i belongs to job r + R * i (Jr = ceil(J / R) rounded up to 4), so
// every wave reads and counts a contiguous run.
// pitch_blk >= nblk: mask row pitch in 8192-node blocks (1 KiB each).  pitch_blk > nblk only with the study knob
// PE_ROW_PITCH_BLOCKS: the words past nblk are then not written (placement.h: unspecified)
// unit_ctr (nblk zeroed counters, or nullptr): the waves of a block share its (phase, 64-job batch)
// units through the block's counter instead of each taking its own phase -- same rows, same counts.
hipError_t launch_fit_mask_planes_rows(hipStream_t s, const uint32_t* planes, int64_t nblk, const uint64_t* jcode,
                                       int64_t J, int64_t R, uint32_t* mask, unsigned long long* counts,
                                       int64_t pitch_blk, unsigned long long* unit_ctr = nullptr);
// Plane-set form (batches with more than PL_MAX distinct request values), all sets in one launch
// each: encode writes set t's planes at planes + t * nblk * PL_MAX * 256; the sweep has the rows
// kernel's grid (R phases common to all sets); set t's codes and counts start at meta[3t] (phase-
// major, stride meta[3t+2], meta[3t+1] jobs), each code carrying its job's mask row in bits 40-63.
hipError_t launch_encode_planes_sets(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                     int64_t Ns, int64_t nblk, const PlaneSpec* specs, int nsets, uint32_t* planes);
hipError_t launch_fit_mask_planes_sets(hipStream_t s, const uint32_t* planes, int64_t nblk, const uint64_t* jcode,
                                       const int64_t* meta, int nsets, int64_t R, uint32_t* mask,
                                       unsigned long long* counts, int64_t pitch_blk);

// ---- LDS digit-plane path (fit mask, any number of distinct request values).  Per dimension the
// host ranks the batch's distinct request values v_1 < ... < v_m; a job asks rank c (v_c = its
// request), a node has rank R = #{v_i <= residual}, and  q <= res  <=>  c <= R  exactly.  R >= c is
// decided digit by digit (mixed radix, most significant first): with threshold planes
// GE_k(v) = [digit_k(R) >= v],
//     [R >= c] = GE_top(c_top + 1) | (GE_top(c_top) & ( ... GE_0(c_0) ... ))
// so a field of m values costs L digit levels (m^(1/L)-ish planes each) and 2L - 1 plane reads per
// job; a single-level field is one plane per value.  Label needs are one plane each, and
// dimensions with a single requested value are folded into those.  Single-level fields may be
// CROSSED with the needs instead: one plane per (need, value of each crossed field), the AND of the
// label test and the crossed thresholds, so the job reads one plane for all of them.  The workgroup builds its node
// block's planes in LDS (scatter of the equality bits + suffix OR), then streams the jobs: per job
// a handful of LDS reads, AND/AND-OR combines, one store of the block's slice of the mask row.
constexpr int LD_MAXF = 4;        // digit fields (dimensions with >= 2 distinct values)
constexpr int LD_MAXL = 4;        // digit levels per field
constexpr int LD_MAXNEED = 64;    // distinct label needs
constexpr int LD_CODE = 16;       // u16 plane indices per job: field f's levels at lds_field_off(f) + k, then
                                  // the need plane at lds_need_slot (right after the fields: one readlane fewer)
constexpr int LD_NEED_SLOT = 15;  // the last slot: at most 15 field entries
// First code entry of field fi when the fields are ordered N4 four-level, N3 three-level, N2 two-level,
// then one-level (the kernel's template shape; the sum of the levels must stay <= LD_NEED_SLOT).
__host__ __device__ constexpr int lds_field_off(int fi, int n4, int n3, int n2) {
  return fi <= n4                ? 4 * fi
         : fi <= n4 + n3         ? 4 * n4 + 3 * (fi - n4)
         : fi <= n4 + n3 + n2    ? 4 * n4 + 3 * n3 + 2 * (fi - n4 - n3)
                                 : 4 * n4 + 3 * n3 + 2 * n2 + (fi - n4 - n3 - n2);
}
// The need plane's code entry: the first one after the fields, so that it shares the last field's
// dword (the kernel reads one dword per readlane) instead of sitting alone in the code's last dword.
__host__ __device__ constexpr int lds_need_slot(int n4, int n3, int n2, int n1) {
  return 4 * n4 + 3 * n3 + 2 * n2 + n1;
}
constexpr int LD_THREADS = 1024;  // 16 waves per workgroup, one node block per workgroup
struct LdsSpec {
  int32_t nf;                       // digit fields
  int32_t dim[LD_MAXF];             // resource dimension of field f
  int32_t L[LD_MAXF];               // digit levels of field f
  // level slot k (0 = least significant): digit = (R / div) % mod (mod 0 = no modulus); threshold
  // planes GE(v) for v in [vlo, vlo + nv) at planes pbase + v - vlo
  uint32_t div[LD_MAXF][LD_MAXL];
  uint32_t mod[LD_MAXF][LD_MAXL];
  int32_t pbase[LD_MAXF][LD_MAXL];
  int32_t vlo[LD_MAXF][LD_MAXL];
  int32_t nv[LD_MAXF][LD_MAXL];
  int32_t nneed, need_pbase, nplanes, nfold;
  // crossed single-level fields (ranks rows nf .. nf + nx - 1, dim / voff / m at nf + i): need plane
  // need_pbase + i * xprod + sum_f c_f * xstride[f] = need i AND rank_f >= c_f + 1 for every crossed f
  int32_t nx, xprod;
  int32_t xstride[LD_MAXF];
  uint32_t needs[LD_MAXNEED];
  int32_t fold_dim[D];              // single-valued dimensions folded into the need planes:
  int64_t fold_val[D];              // a node passes them iff res[fold_dim] >= fold_val
  int64_t voff[LD_MAXF];            // field f's sorted distinct values at vals[voff[f] .. voff[f] + m[f])
  int64_t m[LD_MAXF];
};
// ranks: [nf + nx][npad] u32 (npad = node blocks x S, padding nodes 0); aux: [2][npad] u32, row 0 = 1 for
// a shard node passing the folded dimensions (else 0), row 1 = its labels (0 for padding).
// spec: device copy.
hipError_t launch_node_ranks(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                             int64_t npad, const LdsSpec* spec, const int64_t* vals, uint32_t* ranks, uint32_t* aux);
// S = 2048 * W nodes per workgroup block (W u32 words per lane per plane); grid = nblk x R
// workgroups, wave w of workgroup (blk, r) takes jobs j = r + R (w + 16 t).  codes: LD_CODE u16 per
// job, job j's at position (r * 16 + w) * Tpad + t (Tpad >= the longest run, a multiple of 16).
// Mask row-major (PE_MASK_ROWS): row j at mask + j * pitch_bytes, block blk's S/8 bytes at + blk * S/8.
// slots: [R * 16 * Tpad] u32 count slots (zeroed by the caller), slot (r * 16 + w) * Tpad + t = job
// r + R (w + 16 t); launch_lds_counts turns them into per-job u64 counts through the slots' rows.  spec: device copy;
// nplanes = spec->nplanes.  shape = {N4, N3, N2, N1}: fields 0 .. N4-1 have 4 digit levels (W >= 2
// only), the next N3 three, then N2 two, the last N1 one.  The mask has J rows.
hipError_t launch_fit_mask_lds(hipStream_t s, int W, const int shape[4], const LdsSpec* spec, int nplanes,
                               const uint32_t* ranks, int64_t npad, const uint32_t* aux, int64_t nblk,
                               const uint16_t* codes, int64_t J, int64_t R, int64_t Tpad, int64_t pitch_bytes,
                               uint8_t* mask, uint32_t* slots, uint32_t* units = nullptr);   // units: nblk zeroed counters
hipError_t launch_lds_counts(hipStream_t s, const uint32_t* slots, const uint32_t* rows, int64_t nslots,
                             unsigned long long* counts);

// kn / lo: the node-only score terms of prep_nodes (K(n) = (S(n) << 24) | gid, lo20(r1), lo24(r3)),
// kept current by apply; see pe_kernels.hip node_prep for the exactness argument.
hipError_t launch_prep_nodes(hipStream_t s, const int64_t* res, int64_t stride, int64_t Ns, uint64_t id_base,
                             uint64_t* kn, uint32_t* lo /* [2][stride] */);
hipError_t launch_scan(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, const uint64_t* kn,
                       const uint32_t* lo, int64_t Ns, uint64_t id_base, const ReqRec* groups, int Wg, uint64_t* cand,
                       int32_t* cnt, uint64_t* bound, int nwaves);

hipError_t launch_merge(hipStream_t s, const uint64_t* cand, const int32_t* cnt, const uint64_t* bound,
                        int nwaves, int K, uint8_t* out, int Wg);

// ---- sorted walk (the default greedy window path).  The shard's nodes sorted by the node-only
// key K(n) = (S(n) << 24) | gid, copied into sorted SoA order and summarised per 1024-entry round
// (max residual per dimension, OR of labels, first key).  A fitting node has S(n) >= s(q), and its
// key is K(n) - ((s(q) + borrows) << 24) with borrows <= 2, so a group walks the rounds from the
// first that can hold K >= s(q) << 24 and stops once K + 1 collected keys lie below every key the
// unvisited rounds can produce.  Nodes changed since the sort (apply) and nodes whose terms can
// saturate form the overlay, evaluated in full by every group; their sorted entries are
// invalidated (WK_INVALID).  Negative-residual nodes fit nothing and appear in neither.
constexpr int WK_ROUND = 1024;          // sorted entries per round = walk threads per group
constexpr int WK_MAXR = 16384;          // rounds per shard (PE_MAX_NODES / WK_ROUND)
constexpr uint64_t WK_INVALID = ~0ull;
// Walk steps: one round at a time for the first WK_MULTI_AFTER rounds, then up to WK_MULTI candidate
// rounds per step (their loads in flight together, one barrier and one stop test per step).  Round 5
// (tools/walk_ab.py, interleaved, one box): 4 rounds per step after 4 single ones 43.8-45.7 us per
// launch, 2 after 1 39.1-40.2, 2 after 0 / 2 / 4 39.8-41.1, 3 after 2 41.1-42.1 -- with the stop test
// no longer rescanning every key, finer steps collect fewer surplus keys for the selection.
#ifndef WK_MULTI
#define WK_MULTI 2
#endif
#ifndef WK_MULTI_AFTER
#define WK_MULTI_AFTER 1
#endif
struct WalkIndex {
  uint64_t* sk;        // [Ns] sorted keys (WK_INVALID = not walked)
  int64_t* sr;         // [4][sstride] residuals in sorted order
  uint32_t* sl;        // [Ns] labels in sorted order
  uint32_t* pos;       // [stride] sorted index of each local node (~0u = none)
  uint64_t* rmin;      // [nr] first key of each round (at sort time)
  int64_t* rmax;       // [4][nr] max residual per dimension over the round's valid entries
  uint32_t* ror;       // [nr] OR of the round's labels
  int32_t* ovl;        // [stride] overlay local node ids
  int32_t* ovl_n;      // overlay size
  uint32_t* in_ovl;    // [stride] 1 = in the overlay
  uint32_t* ovl_idx;   // [stride] a node's overlay slot (valid while in_ovl)
  int64_t* ovl_res;    // [4][sstride] residuals by overlay slot (kept current by apply)
  uint32_t* ovl_lab;   // [stride] labels by overlay slot
  uint64_t* ovl_kn;    // [stride] K(n) of each overlay slot's state (node_prep; KEY_SLOW: always evaluated)
  unsigned long long* stat;   // nullable: [0] += rounds walked, [1] += overlay entries, per group
  int64_t sstride, nr;
};
// kin[n] = K(n) of a walkable node (no negative residual, not saturating), else WK_INVALID; the
// saturating ones are appended to the overlay (cleared by the caller beforehand) -- or, with `slow`
// (a rebuild on the side stream, whose overlay only the main stream's applies write), flagged in
// slow[n] for walk_switch to add.
hipError_t launch_walk_prep(hipStream_t s, const int64_t* res, int64_t stride, int64_t Ns, const uint64_t* kn,
                            const uint32_t* labels, uint64_t* kin, const WalkIndex& w, uint32_t* slow = nullptr);
// Takes over an index rebuilt on the side stream (pe_engine walk_resort_async), on the main stream
// once the rebuild is done: every node an apply moved into nx's overlay while it was rebuilt leaves
// nx's sorted walk (its entry may hold a state read mid-update), and the flagged saturating nodes
// join nx's overlay with their current state.
hipError_t launch_walk_switch(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                              const uint32_t* slow, const WalkIndex& nx);
// rocPRIM radix sort of n u64 keys (temp == nullptr: *temp_bytes = the scratch size needed).
hipError_t sort_keys_u64(void* temp, size_t* temp_bytes, const uint64_t* in, uint64_t* out, int64_t n, hipStream_t s);
// Sorted SoA copy, pos[], round summaries from the sorted keys w.sk.
hipError_t launch_walk_build(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                             uint64_t id_base, const WalkIndex& w);
// Multi-rank window: world gathered shard blobs (key lists) -> one list per group (the K smallest
// keys below the smallest shard limit, limit = the (K+1)-th or that minimum); gen != 0 signals each
// group as the walk does.  world * K <= MG_CAP.
// rank_stride: bytes between the ranks' blocks in gath (0 = Wg x cand_group_bytes(K), back to back; the
// shared-memory exchange's slots are further apart).  xstatus (zero-copy exchange, device word
// written by launch_xwait before it on the stream): nonzero = a rank's lists never arrived, every
// group is written with n = -1 and limit = *xstatus (signalled) instead of a list.
// sys_scope: the lists may sit in host memory other processes write (this kernel always reads so).
hipError_t launch_merge_shards(hipStream_t s, const uint8_t* gath, int world, int Wg, int K, uint8_t* out, uint32_t gen,
                               int64_t rank_stride = 0, const uint64_t* xstatus = nullptr, bool sys_scope = true);
// Zero-copy exchange: one block waits until every rank's header of every group (slot r at gath +
// r * rank_stride) carries in_gen, at most timeout_ticks of wall_clock64 (100 MHz); *xstatus = 0,
// or 1 << 63 | rank << 32 | the generation that rank's slot still held.
constexpr int XW_THREADS = 256;
hipError_t launch_xwait(hipStream_t s, const uint8_t* gath, int world, int Wg, int K, int64_t rank_stride,
                        uint32_t in_gen, int64_t timeout_ticks, uint64_t* xstatus);
// The same merge by rank (merge_ranked_kernel, the default): 256-thread blocks, the lists and the
// merged list in LDS (merge_ranked_lds bytes of dynamic LDS, at most RM_MAX_LDS), a cut of each list
// ranked by lock-step binary searches, no sort.  sys_scope = false: gath is device memory written by
// an earlier kernel of the stream (the RCCL all-gather), read with plain loads.
constexpr int RM_THREADS = 256, RM_MAX_WORLD = 16;
constexpr size_t RM_MAX_LDS = 64 * 1024;
size_t merge_ranked_lds(int world, int K);
hipError_t launch_merge_ranked(hipStream_t s, const uint8_t* gath, int world, int Wg, int K, uint8_t* out, uint32_t gen,
                               int64_t rank_stride = 0, const uint64_t* xstatus = nullptr, bool sys_scope = true);
// Wg empty lists (n = 0, limit = NO_KEY), signalled with gen
hipError_t launch_empty_groups(hipStream_t s, int Wg, int K, uint8_t* out, uint32_t gen);
// Test knob (PE_TEST_STALL_*): one thread that holds the stream for `ticks` of wall_clock64 (100 MHz),
// sleeping between polls -- bounded, so the stream always drains
hipError_t launch_stall(hipStream_t s, int64_t ticks);
// One block per group: overlay + walk, exact top-K keys and limit, same blob as merge.  gen != 0:
// each group's header.flags is set to gen after its keys, n and limit are visible to the host
// (system-scope release; out is pinned host memory the host polls per group).  K_stride: the blob's
// list capacity per group (cand_group_bytes(K_stride) apart; 0 = K), K <= K_stride.
hipError_t launch_walk(hipStream_t s, const ReqRec* groups, int Wg, int K, const WalkIndex& w, const int64_t* res,
                       int64_t stride, const uint32_t* labels, int64_t Ns, uint64_t id_base, uint8_t* out,
                       uint32_t gen = 0, int K_stride = 0);

// upd: [n] records {local node (i64), res[4]} -> res[d][node] = value (absolute)
// (kn, lo nullable: refreshed for the updated nodes when given; w nullable: the updated nodes
// leave the sorted walk and join its overlay; nx nullable: an index being rebuilt on the side
// stream -- the updated nodes join its overlay too, its sorted entries are left to walk_switch)
hipError_t launch_apply(hipStream_t s, int64_t* res, int64_t stride, const int64_t* upd, int64_t n, uint64_t id_base,
                        uint64_t* kn, uint32_t* lo, const uint32_t* labels, const WalkIndex* w,
                        const WalkIndex* nx = nullptr);

// Inventory delta for one slot of this shard (pe_update_nodes): residual written to both the
// live and the reset copy, labels and island replaced.  Slots are unique within a launch.
struct NodeUpd {
  int64_t local;
  int64_t res[D];
  uint32_t labels;
  int32_t island;
};
static_assert(sizeof(NodeUpd) == 48, "NodeUpd must be 48 B");
hipError_t launch_scatter_nodes(hipStream_t s, int64_t* res, int64_t* res0, int64_t stride, uint32_t* labels,
                                int32_t* island, const NodeUpd* upd, int64_t n);

// ---- gang capacity (pe_gang_capacity, pe_capacity.hip)
constexpr int CP_THREADS = 256;                  // threads per block
constexpr int CP_NPT = 4;                        // nodes per thread, kept in registers
constexpr int CP_SPAN = CP_THREADS * CP_NPT;     // nodes per block
constexpr int CP_TS = 64;                        // shapes between two block folds
constexpr uint64_t CP_CAP_MAX = 2147483647;      // PE_CAP_MAX
__host__ __device__ inline int64_t cap_node_blocks(int64_t Ns) { return (Ns + CP_SPAN - 1) / CP_SPAN; }
// One distinct pod shape: the request, the label need and per dimension with q > 0 the reciprocal of
// the request (pe_divmagic.h div_magic; unused where q == 0).  96 B, read through a uniform address.
struct alignas(32) CapShape {
  int64_t q[D];
  uint64_t m[D];
  uint32_t sh[D];
  uint32_t need;
  uint32_t pad_[3];
};
static_assert(sizeof(CapShape) == 96, "CapShape must be 96 B");
// A shape's result over a set of nodes: sum of the capacities, the largest one, nodes with capacity >= 1.
struct CapAcc {
  uint64_t slots;
  uint32_t max_node;
  uint32_t nodes;
};
static_assert(sizeof(CapAcc) == 16, "CapAcc must be 16 B");
// out[s] (s < S) over the shard's Ns nodes; partials: cap_node_blocks(Ns) * S records of scratch.
hipError_t launch_gang_capacity(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels, int64_t Ns,
                                const CapShape* shapes, int64_t S, CapAcc* partials, CapAcc* out);

// ---- why a shape fits no node (pe_fit_explain, pe_explain.hip; records and chunking: pe_explain_plan.h)
constexpr int EX_TS = 32;                        // records between two block folds
struct ExplainRec;
// hist[S][32] += per record the shard's live nodes in the record's scope by 5-bit signature, near[S][4] = min per
// dimension d over the nodes with signature 1 << d of req_d - res_d as u64 (near NULL: not computed).  The caller
// zeroes hist and fills near with ~0 (no such node).  leaf_dom[n_leaf] (pe_explain_plan.h explain_leaf_dom) is
// read only when with_domains: without it every record counts the whole shard.
hipError_t launch_fit_explain(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                              const int32_t* island, int64_t Ns, const int32_t* leaf_dom, int n_leaf, bool with_domains,
                              const ExplainRec* recs, int64_t S, uint64_t* hist, uint64_t* near);

// ---- gang capacity per topology domain: the leaf table of both table calls (pe_domains.hip)
constexpr int DM_MAX_DOMAINS = 65536;            // PE_MAX_DOMAINS
// dom_slots / dom_nodes [S][n_domains] += over the shard's Ns nodes (the caller zeroes them; dom_nodes may be
// NULL: not computed), domain of node n = island[n].
hipError_t launch_gang_capacity_domains(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                        const int32_t* island, int64_t Ns, const CapShape* shapes, int64_t S,
                                        int n_domains, uint64_t* dom_slots, uint32_t* dom_nodes);

// ---- gang capacity over a topology hierarchy (pe_gang_capacity_tree, and pe_gang_capacity_domains as the
// hierarchy of one level; pe_tree.hip; the plan: pe_tree_plan.h)
constexpr int TR_MAX_LEVELS = 4;                 // PE_MAX_LEVELS
// A distinct (shape, count, max_level) of a call that asks for a selection; its answer.
struct TreePick {
  uint32_t shape;     // index into the call's distinct shapes
  int32_t count;      // >= 1
  int32_t max_level;  // in [0, n_levels)
  int32_t pad_;
};
struct TreeSel {
  uint64_t slots;   // the chosen domain's slots, 0 when none
  int32_t domain;   // of the lowest level <= max_level that holds the gang: smallest slots >= count, ties to the
                    // smallest id; -1 when none
  int32_t level;    // that level, -1 when none
};
static_assert(sizeof(TreePick) == 16 && sizeof(TreeSel) == 16, "TreePick / TreeSel layout");
// The levels of a call, by value: level l has size[l] domains; level 0's rows are the leaf table's, level
// l >= 1 begins at column col[l] of the upper table's rows (pitch = the sum of the upper sizes).
struct TreeLevels {
  int32_t n_levels;
  int32_t size[TR_MAX_LEVELS];
  int32_t col[TR_MAX_LEVELS];
  int32_t pitch;
};
// One level from the level below, for S shapes: up[s][p] = sum of lo[s][c] over the children c of parent p
// (start[n_parents + 1] / child: the level's CSR), slots and -- unless lo_nodes is NULL -- nodes.  lo_* / up_*
// point at the level's first column; every (s, p) is stored, a childless parent as 0.  width: lanes per
// parent, a power of two in [1, 64].
hipError_t launch_tree_rollup(hipStream_t s, const uint64_t* lo_slots, const uint32_t* lo_nodes, int64_t lo_pitch,
                              const int32_t* start, const int32_t* child, int n_parents, int width, int64_t S,
                              uint64_t* up_slots, uint32_t* up_nodes, int64_t up_pitch);
// out[p] and feasible[p][n_levels] for every pick p < P whose shape lies in [s0, s0 + S), from the rows
// leaf_slots[shape - s0] ([S][size[0]]) and upper_slots[shape - s0] ([S][pitch]; unused at n_levels 1).
hipError_t launch_tree_select(hipStream_t s, const uint64_t* leaf_slots, const uint64_t* upper_slots, int64_t s0,
                              int64_t S, const TreeLevels& levels, const TreePick* picks, int64_t P, TreeSel* out,
                              uint32_t* feasible);

// ---- a gang spread over the fewest domains (pe_gang_split_tree, pe_split.hip; the arithmetic, the slice
// buffer's layout and the scatter: pe_split_plan.h)
// Where the CSR of level l >= 1 lies in the plan's words (pe_tree_plan.h start_at / child_at).
struct SplitCsr {
  int32_t start_at[TR_MAX_LEVELS];
  int32_t child_at[TR_MAX_LEVELS];
};
// The descent for the picks [p0, p0 + n) whose shape lies in [s0, s0 + S), after launch_tree_select wrote
// sel[p] for them from the same tables: their rows of the slice buffer buf (SplitLayout{n, max_parts}) get the
// parts (domain and pods, the unused tail -1 / 0), the number of parts (0: none selected, SPLIT_TOO_MANY) and
// the spread per level.  max_parts in [1, SPLIT_MAX_PARTS].
hipError_t launch_tree_split(hipStream_t s, const uint64_t* leaf_slots, const uint64_t* upper_slots, int64_t s0,
                             int64_t S, const TreeLevels& levels, const SplitCsr& csr, const int32_t* plan,
                             const TreePick* picks, const TreeSel* sel, int64_t p0, int64_t n, int max_parts,
                             int32_t* buf);

// ---- a gang in slices, each inside one domain (pe_gang_slice_tree, pe_slice.hip; rows, picks and the unit
// conversion: pe_slice_plan.h).  A call's tables have one row per distinct (shape, z, sl): slots below level
// max(sl, 0), units at and above it.  A pick is a TreePick whose shape is the row, count the units wanted and
// pad_ the lowest level max(sl, 0).
struct SliceRow;
// launch_gang_capacity_domains without the node table, for R rows: a record whose pad_[0] holds z >= 2 (a
// node-level row) adds floor(cap / z) per node, a record with pad_[0] == 0 the node's capacity.
hipError_t launch_slice_leaf(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                             const int32_t* island, int64_t Ns, const CapShape* shapes, int64_t R, int n_domains,
                             uint64_t* dom_units);
// table[r][k] = floor(table[r][k] / rows[r].z) for k < n_cols and every r < R with rows[r].sl == level: the
// launch's rows of one level from slots to units, in place.  rows: the launch's first row.
hipError_t launch_slice_units(hipStream_t s, uint64_t* table, int64_t pitch, int n_cols, const SliceRow* rows, int64_t R,
                              int level);
// launch_tree_select from the pick's lowest level upward, without the per-level counts.
hipError_t launch_slice_select(hipStream_t s, const uint64_t* leaf_units, const uint64_t* upper_units, int64_t r0,
                               int64_t R, const TreeLevels& levels, const TreePick* picks, int64_t P, TreeSel* out);
// launch_tree_split with the lists turned from units to pods at the pick's lowest level.  rows: the call's
// first row (a pick names its row by its number in the call).
hipError_t launch_slice_split(hipStream_t s, const uint64_t* leaf_units, const uint64_t* upper_units, int64_t r0,
                              int64_t R, const TreeLevels& levels, const SplitCsr& csr, const int32_t* plan,
                              const SliceRow* rows, const TreePick* picks, const TreeSel* sel, int64_t p0, int64_t n,
                              int max_parts, int32_t* buf);

// ---- gang placement inside a chosen domain (pe_place_greedy_domains, pe_place.hip; the plan: pe_place_plan.h)
constexpr int PL_THREADS = 256;       // threads of a domain's workgroup
// A domain's working state (four residuals, labels, node id: 40 B per node) lives in LDS up to this many
// nodes and in the compact global segment beyond.  1016 nodes are 40 640 B; with the 128 B of the waves' minima
// a workgroup stays within 40 KiB, so four workgroups of four waves share a CU's 160 KiB (1024 nodes would
// leave room for three).  A rack fits, a zone does not.
constexpr int PL_LDS_NODES = 1016;
// One group of the batch: request, need and count, and its first pod slot.
struct alignas(64) PlaceGroup {
  int64_t q[D];
  uint32_t need;
  int32_t count;
  int64_t pod0;
  uint32_t pad_[4];
};
static_assert(sizeof(PlaceGroup) == 64, "PlaceGroup must be 64 B");
// One job, in plan order: its index in the caller's batch and its groups [g0, g1).
struct PlaceJob {
  int32_t job, g0, g1, pad_;
};
static_assert(sizeof(PlaceJob) == 16, "PlaceJob must be 16 B");
// The per-domain member lists of one call.  The caller zeroes cnt[A]; after the launch seg_off[A + 1] holds the
// active domains' segment bounds and segment a's places [seg_off[a], seg_off[a + 1]) its nodes' state: global
// id, labels (lab = gid + seg_stride) and the four residuals ([D][seg_stride]), in any order.  leaf_dom[n_leaf] / act_of: the plan's
// maps; a node whose island id lies outside [0, n_leaf), whose leaf has no domain or whose domain is inactive
// is in no list.  cursor[A]: scratch.
struct PlaceSegs {
  int32_t* cnt;
  int32_t* seg_off;
  int32_t* cursor;
  uint32_t* gid;
  uint32_t* lab;
  int64_t* res;
  int64_t seg_stride;
};
hipError_t launch_place_members(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                const int32_t* island, int64_t Ns, uint64_t id_base, const int32_t* leaf_dom,
                                int n_leaf, const int32_t* act_of, int A, const PlaceSegs& segs);
// One workgroup per active domain a < A: its jobs jobs[job_start[a] .. job_start[a + 1]) in that order, placed
// on its segment by the Appendix-B rule.  out_pod [P] (every slot of a job with pods is written), out_status by
// the caller's job index, log: 3 int32 of scratch per pod slot; at the end the segment's residuals go back to res.
hipError_t launch_place_domains(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* job_start,
                                int A, const PlaceSegs& segs, int64_t* res, int64_t stride, uint64_t id_base,
                                int32_t* out_pod, int32_t* out_status, int32_t* log);

// ---- MinMember first, the rest as fits (pe_place_min_member_domains, pe_place_min.hip; the plan:
// pe_place_min_plan.h).  Group g comes as one PlaceGroup -- its MANDATORY share: count = its mandatory pods, pod0 =
// its first mandatory slot in the mandatory numbering -- and one PlaceMinOpt, its OPTIONAL share.
struct PlaceMinOpt {
  int64_t pod0;    // its first optional slot among all slots
  int32_t count;   // its optional pods
  int32_t pad_;
};
static_assert(sizeof(PlaceMinOpt) == 16, "PlaceMinOpt must be 16 B");
// One job, in plan order: its index in the caller's batch, its groups [g0, g1), its mandatory records [g0, gm),
// `shift` from a mandatory slot to the slot among all slots, and its pod total.  32 B, so that no record straddles
// a 64-B line, and the shift itself rather than something to derive it from: the workgroup reads one record per
// job with nothing else to do meanwhile (DESIGN.md section 24 has the measurements).
struct PlaceMinJob {
  int32_t job, g0, gm, g1;
  int64_t shift, pods;
};
static_assert(sizeof(PlaceMinJob) == 32, "PlaceMinJob must be 32 B");
// One workgroup per active domain a < A: its jobs in that order; phase 1 is launch_place_domains' all-or-nothing
// loop over the mandatory records, phase 2 places the optional shares as far as they fit and rolls nothing back.
// out_pod [P] (every slot of every job is written), out_group_pods [G] (zeroed by the caller; a placed job writes
// every one of its groups, a failed job none), out_status by the caller's job index,
// log: 3 int32 of scratch per MANDATORY pod; at the end the segment's residuals go back to res.
hipError_t launch_place_min_domains(hipStream_t s, const PlaceGroup* groups, const PlaceMinOpt* opt,
                                    const PlaceMinJob* jobs, const int32_t* job_start, int A, const PlaceSegs& segs,
                                    int64_t* res, int64_t stride, uint64_t id_base, int32_t* out_pod, int32_t* out_status,
                                    int32_t* out_group_pods, int32_t* log);

// ---- first-fit placement of a batch over candidate domains (pe_place_first_fit_domains, pe_place.hip; the plan:
// pe_first_fit_plan.h).  The member lists are launch_place_members'; the segments stay the working residuals of
// their domains from round to round.
// One entry of an active domain's queue: candidate k of `job` (its pair `pair` of the caller's list), last = 1
// when k is the job's last candidate.  A queue is sorted by (the job's rank in the job order, k).
struct FirstFitEntry {
  int32_t job, k, pair, last;
};
static_assert(sizeof(FirstFitEntry) == 16, "FirstFitEntry must be 16 B");
constexpr uint32_t FF_SETTLED = 0x80000000u;
// The state the rounds carry.  word[J]: per job, low half = the position k of the candidate it tries next, with
// FF_SETTLED set once it is placed or out of candidates (k then the position of its last attempt), high half =
// the round that wrote the word; the caller zeroes it.  cursor[A]: per active domain the next entry of its
// queue, set to q_start[a] by the caller.  open: the jobs not yet settled, set by the caller to the number of
// jobs with a candidate.
struct FirstFitState {
  uint64_t* word;
  int32_t* cursor;
  uint32_t* open;
};
// Round `round` (1, 2, ...): one workgroup per active domain works off the head of its queue as far as the words
// AS THEY STOOD WHEN THE ROUND BEGAN allow and returns.  jobs[J] by the caller's job index.  out_pod [P] and
// out_pair [J] preset to -1 and out_status [J] to 1 by the caller; log as for launch_place_domains.  kinds: which
// of the two kernel instances to launch, FF_SMALL for the segments of at most PL_LDS_NODES nodes, FF_LARGE for
// the larger ones; a caller who does not know the segments' sizes passes both.
constexpr int FF_SMALL = 1, FF_LARGE = 2;
hipError_t launch_first_fit_round(hipStream_t s, const PlaceGroup* groups, const PlaceJob* jobs, const int32_t* q_start,
                                  const FirstFitEntry* queue, int A, const PlaceSegs& segs, int kinds, uint32_t round,
                                  const FirstFitState& st, int32_t* out_pod, int32_t* out_status, int32_t* out_pair,
                                  int32_t* log);
// The segments' residuals back to the live SoA, once, after the last round.
hipError_t launch_first_fit_finish(hipStream_t s, const PlaceSegs& segs, int A, int64_t Ns, int64_t* res, int64_t stride,
                                   uint64_t id_base);

// ---- exact what-if of a whole gang per domain (pe_gang_fit_domains, pe_fit.hip; the plan and its FitUnit /
// FitLarge records: pe_fit_plan.h).  The member lists are launch_place_members', read-only here.
struct FitUnit;
struct FitLarge;
// One (job, domain) pair in plan order: its index in the caller's list, its job and the job's groups [g0, g1).
struct FitPair {
  int32_t pair, job, g0, g1;
};
static_assert(sizeof(FitPair) == 16, "FitPair must be 16 B");
// The answers of a call, on the device: first[J] (the caller sets every cell to -1; unsigned minimum of the
// fitting pairs' indices), and per pair fits, fail_group and pods, by the caller's pair index.
struct FitOut {
  uint32_t* first;
  uint8_t* fits;
  int32_t* fail_group;
  int64_t* pods;
};
// large == NULL: one workgroup per unit u < blocks; those whose segment has at most PL_LDS_NODES nodes judge their
// pairs on a working copy in LDS, the others leave at once.  Otherwise one workgroup per record of
// large[0 .. blocks): the units of a larger segment that the record names, on the working copy
// scratch[at + d * n] (n = the segment's nodes).  PlaceGroup.pod0 is not read.
hipError_t launch_fit(hipStream_t s, const PlaceGroup* groups, const FitPair* pairs, const FitUnit* units, int64_t blocks,
                      const FitLarge* large, int64_t* scratch, const PlaceSegs& segs, const FitOut& out);

// ---- which gangs must go for a gang to fit (pe_gang_preempt_domains, pe_preempt.hip; the plan and its PreRec
// records: pe_preempt_plan.h; units and FitLarge records as for the fit call).  The member lists are
// launch_place_members', read-only here.
struct PreRec;
// One pair in plan order: its index in the caller's list, its job, the job's groups [g0, g1) and its candidate
// victims list[v0 .. v1), at most 64.
struct PrePair {
  int32_t pair, job, g0, g1, v0, v1, pad_[2];
};
static_assert(sizeof(PrePair) == 32, "PrePair must be 32 B");
// What the judging kernels read besides the segments.  node_place[Ns]: the place of local node n in the
// segments' arrays, -1 = in no active domain (launch_preempt_place_map).
struct PreIn {
  const PlaceGroup* groups;
  const PrePair* pairs;
  const FitUnit* units;
  const int32_t* list;        // victim indices, the pairs' lists back to back
  const int32_t* rec_start;   // [V + 1]
  const PreRec* recs;
  const int32_t* node_place;
  int64_t Ns;
  uint64_t id_base;
};
// The answers of a call, on the device: best[J] (the caller sets every cell to ~0; unsigned minimum of
// count << 32 | pair over the pairs with an answer), judged (one cell the caller zeroes: judgements made), and per
// pair, by the caller's pair index, the mask, the prefix and the count.
struct PreOut {
  unsigned long long* best;
  unsigned long long* judged;
  uint64_t* victims;
  int32_t* prefix;
  int32_t* count;
};
// node_place[n] = s for every place s of the segments (the caller preset every cell to -1).
hipError_t launch_preempt_place_map(hipStream_t s, const PlaceSegs& segs, int A, int64_t Ns, uint64_t id_base,
                                    int32_t* node_place);
// As launch_fit, for the two-phase walk of every pair.
hipError_t launch_preempt(hipStream_t s, const PreIn& in, int64_t blocks, const FitLarge* large, int64_t* scratch,
                          const PlaceSegs& segs, const PreOut& out);

// ---- giving back and re-taking placed gangs (pe_release_gangs, pe_assume_gangs, pe_ledger.hip)
constexpr int LG_THREADS = 256;       // threads per block
constexpr int LG_MAX_BLOCKS = 256;    // one block per CU; beyond LG_THREADS x LG_MAX_BLOCKS records the grid strides
// One touched node of this shard: its local index and its four residuals after the call (absolute, the format
// of launch_apply's updates).  The host computed them against its mirror; locals are unique within a launch.
struct LedgerRec {
  int64_t local;
  int64_t res[D];
};
static_assert(sizeof(LedgerRec) == 40, "LedgerRec must be 40 B");
// res[d][rec.local] = rec.res[d] for every record: plain stores, no read of the old value.  Every local must lie
// in [0, stride).
hipError_t launch_ledger_scatter(hipStream_t s, int64_t* res, int64_t stride, const LedgerRec* recs, int64_t n);

// ---- can a node's pods move elsewhere, and where (pe_drain_fit_domains, pe_drain.hip; the plan: pe_drain_plan.h;
// units and FitLarge records as for the fit call).  The member lists are launch_place_members', read-only here.
// One candidate in plan order: its index in the caller's list, its node's GLOBAL id and its runs [g0, g1) --
// PlaceGroup records whose count is the run's pods and whose pod0 is the run's first place in the slot list.  A
// candidate's runs are consecutive in the slot list: its slots are the places [pod0 of g0, pod0 + count of g1 - 1).
struct DrainPair {
  int32_t cand, node, g0, g1;
};
static_assert(sizeof(DrainPair) == 16, "DrainPair must be 16 B");
// The answers of a call, on the device, by the caller's candidate index: fits, moved and fail_slot; and target[S]
// by pod slot (the caller sets every cell to -1; only the STORE instances touch it, and may be NULL for the others).
struct DrainOut {
  uint8_t* fits;
  int64_t* moved;
  int64_t* fail_slot;
  int32_t* target;
};
// As launch_fit, with the candidate's node taken out of the working copy.  slot_list: the evicted pod slots, every
// candidate's back to back.  store: write out.target.
hipError_t launch_drain(hipStream_t s, const PlaceGroup* runs, const DrainPair* pairs, const FitUnit* units, int64_t blocks,
                        const FitLarge* large, int64_t* scratch, const int32_t* slot_list, const PlaceSegs& segs,
                        const DrainOut& out, bool store);

// ---- fewest new nodes for a gang to fit a domain (pe_scale_up_domains, pe_scale.hip; the plan: pe_scale_plan.h;
// units -- cut by weight -- and FitLarge records as for the fit call).  The member lists are launch_place_members',
// read-only here.
constexpr int SCALE_MAX_NODES = 64;   // PE_MAX_SCALE_NODES: a thread holds at most one new place
static_assert(SCALE_MAX_NODES <= PL_THREADS, "one new place per thread");
// One pair in plan order: its index in the caller's list, its job, the job's groups [g0, g1), its template and the
// largest number of new nodes to try, in [0, n_new].
struct ScalePair {
  int32_t pair, job, g0, g1, tmpl, kmax, pad_[2];
};
static_assert(sizeof(ScalePair) == 32, "ScalePair must be 32 B");
// What the judging kernels read besides the segments.  tmpl_res [T][4] and tmpl_lab [T]: a fresh node's residual
// and its labels, the island bit already set; new_slot [n_new]: the GLOBAL ids of the new nodes, in the order
// they are handed out.
struct ScaleIn {
  const PlaceGroup* groups;
  const ScalePair* pairs;
  const FitUnit* units;
  const int64_t* tmpl_res;
  const uint32_t* tmpl_lab;
  const int32_t* new_slot;
  int32_t n_new;
};
// The answers of a call, on the device: best[J] (the caller sets every cell to ~0; unsigned minimum of
// nodes << 32 | pair over the pairs with an answer), and per pair, by the caller's pair index, nodes, fail_group,
// pods and new_pods.
struct ScaleOut {
  unsigned long long* best;
  int32_t* nodes;
  int32_t* fail_group;
  int64_t* pods;
  int64_t* new_pods;
};
// As launch_fit, for the ascending attempts of every pair.  PlaceGroup.pod0 is not read.
hipError_t launch_scale(hipStream_t s, const ScaleIn& in, int64_t blocks, const FitLarge* large, int64_t* scratch,
                        const PlaceSegs& segs, const ScaleOut& out);

}  // namespace pe
