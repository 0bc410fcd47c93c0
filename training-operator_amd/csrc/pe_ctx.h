// libplacement internals shared by the engine's units (pe_engine.cpp, pe_engine_greedy.cpp,
// pe_engine_capacity.cpp, pe_domain_call.cpp, pe_engine_place.cpp, pe_engine_fit.cpp, pe_engine_first_fit.cpp,
// pe_engine_preempt.cpp, pe_engine_ledger.cpp, pe_engine_drain.cpp): device and pinned buffers, the helper threads, error mapping, input
// checks and the context itself.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <immintrin.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pe_drain_plan.h"
#include "pe_explain_plan.h"
#include "pe_hostx.h"
#include "pe_kernels.h"
#include "pe_ledger_plan.h"
#include "pe_resolver.h"
#include "pe_slice_plan.h"
#include "placement.h"

// (a namespace of their own: the inline functions below are visible outside the shared library, where
// plain names such as hipchk could meet another library's)
namespace pe_engine {

using pe::ReqRec;

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  // flags: hipExtMallocWithFlags flags (hipDeviceMallocContiguous falls back to a plain hipMalloc
  // when the driver cannot provide it)
  hipError_t ensure(size_t count, unsigned flags = 0) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipErrorOutOfMemory;
    if (flags) {
      e = hipExtMallocWithFlags((void**)&p, bytes, flags);
      if (e != hipSuccess) (void)hipGetLastError();
    }
    if (e != hipSuccess) e = hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// Pinned host buffer.  Coherent (fine-grained) ones are also read and written by kernels directly
// (dev = the device-side address): per-window inputs and the candidate blob skip the copy engines.
template <class T>
struct HostBuf {
  T* p = nullptr;
  T* dev = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t count, unsigned flags = hipHostMallocDefault) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = dev = nullptr;
    n = 0;
    hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T), flags);
    // zeroed: several of these buffers carry completion flags (signalled groups, the aggregation
    // flag) that a recycled allocation could otherwise hold from an earlier engine's generations
    if (e == hipSuccess) std::memset((void*)p, 0, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&dev, p, 0);
    if (e == hipSuccess) n = count;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = dev = nullptr;
    n = 0;
  }
};
constexpr unsigned kZeroCopy = hipHostMallocCoherent | hipHostMallocMapped;

// One helper thread that runs a posted task while the caller does other work (pipelined greedy:
// the next window's launches are issued while the host resolves the current one).  Spin handoff:
// the wake-up of a sleeping thread would cost about as much as the launches it hides.
class SpinWorker {
 public:
  explicit SpinWorker(int device) : th_([this, device] {
    (void)hipSetDevice(device);   // the current device is per thread
    loop();
  }) {}
  ~SpinWorker() {
    while (state_.load(std::memory_order_acquire) == 1) _mm_pause();   // a posted task finishes first
    state_.store(3, std::memory_order_release);
    th_.join();
  }
  void pin(const cpu_set_t& set) { (void)pthread_setaffinity_np(th_.native_handle(), sizeof(set), &set); }
  void post(std::function<void()> f) {
    task_ = std::move(f);
    err_ = nullptr;
    posted_ = true;
    state_.store(1, std::memory_order_release);
  }
  bool busy() const { return state_.load(std::memory_order_acquire) == 1; }   // a posted task not done yet
  bool failed() const { return state_.load(std::memory_order_acquire) == 2 && err_ != nullptr; }
  void wait() {   // rethrows what the task threw; returns at once when nothing is posted
    if (!posted_) return;
    posted_ = false;
    for (int spin = 0; state_.load(std::memory_order_acquire) != 2; ++spin)
      if (spin < 4096) _mm_pause();
      else std::this_thread::yield();   // the helper is not running (oversubscribed host)
    state_.store(0, std::memory_order_relaxed);
    if (err_) std::rethrow_exception(err_);
  }

 private:
  void loop() {
    int idle = 0;
    for (;;) {
      const int st = state_.load(std::memory_order_acquire);
      if (st == 3) return;
      if (st != 1) {
        if (++idle < 4096) _mm_pause();
        else std::this_thread::yield();   // long idle (host resolving): let others run
        continue;
      }
      idle = 0;
      try {
        task_();
      } catch (...) {
        err_ = std::current_exception();
      }
      state_.store(2, std::memory_order_release);
    }
  }
  std::atomic<int> state_{0};
  bool posted_ = false;   // (the posting thread's own view: a task posted and not waited for yet)
  std::function<void()> task_;
  std::exception_ptr err_;
  std::thread th_;   // last: starts after the members above exist
};

// A SpinWorker with a queue: post() does not wait for the previous task (up to kCap in flight), the
// tasks run in order on the thread, wait() waits for all of them.  After a task threw, the rest are
// skipped and wait() rethrows.  (The host-merged zero-copy exchange: the main thread posts each
// window's merge as it launches the window, without waiting for the previous merge to finish.)
class SpinQueue {
 public:
  static constexpr unsigned kCap = 8;
  explicit SpinQueue(int device) : th_([this, device] {
    (void)hipSetDevice(device);
    loop();
  }) {}
  ~SpinQueue() {
    while (busy()) _mm_pause();
    stop_.store(true, std::memory_order_release);
    th_.join();
  }
  void pin(const cpu_set_t& set) { (void)pthread_setaffinity_np(th_.native_handle(), sizeof(set), &set); }
  void post(std::function<void()> f) {
    const unsigned t = tail_.load(std::memory_order_relaxed);
    while (t - head_.load(std::memory_order_acquire) >= kCap) _mm_pause();   // full: the oldest first
    q_[t % kCap] = std::move(f);
    tail_.store(t + 1, std::memory_order_release);
  }
  bool busy() const { return head_.load(std::memory_order_acquire) != tail_.load(std::memory_order_acquire); }
  bool failed() const { return failed_.load(std::memory_order_acquire); }
  void wait() {   // every posted task done; rethrows the first error (once)
    for (int spin = 0; busy(); ++spin)
      if (spin < 4096) _mm_pause();
      else std::this_thread::yield();
    if (failed_.load(std::memory_order_acquire)) {
      failed_.store(false, std::memory_order_relaxed);
      std::exception_ptr e = err_;
      err_ = nullptr;
      if (e) std::rethrow_exception(e);
    }
  }

 private:
  void loop() {
    int idle = 0;
    for (;;) {
      const unsigned h = head_.load(std::memory_order_relaxed);
      if (h == tail_.load(std::memory_order_acquire)) {
        if (stop_.load(std::memory_order_acquire)) return;
        if (++idle < 4096) _mm_pause();
        else std::this_thread::yield();
        continue;
      }
      idle = 0;
      if (!failed_.load(std::memory_order_relaxed)) {
        try {
          q_[h % kCap]();
        } catch (...) {
          err_ = std::current_exception();
          failed_.store(true, std::memory_order_release);
        }
      }
      q_[h % kCap] = nullptr;
      head_.store(h + 1, std::memory_order_release);
    }
  }
  std::function<void()> q_[kCap];
  std::atomic<unsigned> head_{0}, tail_{0};
  std::atomic<bool> failed_{false}, stop_{false};
  std::exception_ptr err_;
  std::thread th_;   // last: starts after the members above exist
};


struct PeError {
  int code;
  std::string msg;
};

[[noreturn]] inline void raise(int code, const std::string& msg) { throw PeError{code, msg}; }

inline void hipchk(hipError_t e, const char* what) {
  if (e != hipSuccess) raise(PE_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

inline void ncclchk(ncclResult_t r, const char* what) {
  if (r != ncclSuccess) raise(PE_ERCCL, std::string(what) + ": " + ncclGetErrorString(r));
}

// Bound of one RCCL window of the greedy: PE_RCCL_TIMEOUT_S seconds (default 60) blocked on a window
// whose all-gather has not completed (a peer lost mid-batch) -- then the communicator is aborted and
// the call returns PE_ERCCL.
inline double rccl_timeout_s() {
  const char* e = std::getenv("PE_RCCL_TIMEOUT_S");
  const double s = e ? std::atof(e) : 60.0;
  return s > 0 ? s : 60.0;
}

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// pe_config.fit_path_mask bits
constexpr int kMaxMergers = 7;   // zero-copy exchange: merge helper threads per rank (at most)
constexpr int PATH_I64 = 1, PATH_I32 = 2, PATH_CODED = 4, PATH_NO_THERM = 8, PATH_PLANES = 16, PATH_PLANES_BLOCKS = 32,
              PATH_LDS = 64;
constexpr int PATHS_ALL = PATH_I64 | PATH_I32 | PATH_CODED | PATH_PLANES | PATH_LDS;

// One segment of the packed aggregation batch (pe_kernels.h AggSegHdr).
struct AggSeg {
  int64_t j0;
  int32_t nj, ng, nc;
  int64_t bytes;
  bool narrow;            // the request section narrowed (pe_kernels.h agg_seg_layout), shifts in sh
  uint8_t sh[pe::AGG_MAX_KEYS];
};

}  // namespace pe_engine
using namespace pe_engine;

struct pe_ctx {
  std::mutex mu;
  int device = 0;
  int rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  // a greedy window's collective timed out: the communicator was handed to comm_abort (ncclCommAbort
  // on its own thread -- it returns once the device work it aborts has drained) and every later
  // sharded call fails with PE_ERCCL; the caller rebuilds the context (e.g. on the host exchange)
  bool comm_aborted = false;
  std::thread comm_abort;
  std::unique_ptr<pe::Resolver> resolver;   // the greedy's host resolver, reset per batch
  pe_allgather_fn exchange = nullptr;
  void* exchange_user = nullptr;
  void* zc_hx = nullptr;   // the shared-memory exchange whose zero-copy use the ranks agreed on (zc_ok)
  bool zc_ok = false;
  int topk = 256, window_groups = 112;
  bool pipeline = true;   // greedy: scan window w+1 while the host resolves window w (greedy_flags bit0 = off)
  int64_t window_pods = 1024;
  int64_t max_nodes = 0;
  std::string gpu_name, err;
  hipStream_t stream = nullptr;
  // inventory shard
  int64_t n_total = 0, begin = 0, end = 0, Ns = 0, stride = 0;
  bool loaded = false;
  // host mirror of the GLOBAL inventory (node states by id, and the reset copy): the greedy
  // windows ship candidate keys only and the resolver reads node states here
  std::vector<pe::NodeState, pe::HugeAlloc<pe::NodeState>> m_nodes, m_nodes0;   // (2 MiB pages: random reads)
  DevBuf<int64_t> res0, res;
  DevBuf<uint32_t> labels;
  DevBuf<int32_t> island;
  DevBuf<pe::NodeUpd> n_upd;   // pe_update_nodes staging
  // fit mask
  int64_t fit_J = 0, fit_Jp = 0, Wn = 0, Wt = 0;
  bool fit_uploaded = false;
  DevBuf<ReqRec> fit_jobs;
  DevBuf<pe::ReqRec32> fit_jobs32;
  DevBuf<int32_t> res32;
  bool fit32 = false;      // batch is exactly representable in 32 bits (see ReqRec32)
  int fit_shift[pe::D] = {0, 0, 0, 0};
  int fit_path = 0;        // 0 int64 compare, 1 int32 compare, 2 dictionary-coded, 3 bit planes, 4 LDS digit planes
  // LDS digit-plane path (pe_kernels.h LdsSpec): spec, node-block geometry, codes, ranks
  pe::LdsSpec lds{};
  int lds_W = 4;                          // u32 words per lane per plane: block = 2048 W nodes
  int lds_shape[4] = {0, 0, 0, 0};        // fields with 4 / 3 / 2 / 1 digit levels (kernel template)
  int64_t lds_nblk = 0, lds_R = 1, lds_Tpad = 0, lds_npad = 0, lds_pitch = 0;   // pitch in u64 words
  DevBuf<pe::LdsSpec> lds_spec_d;
  DevBuf<int64_t> lds_vals;
  DevBuf<uint16_t> lds_codes;
  DevBuf<uint32_t> lds_ranks, lds_aux, lds_slots;   // lds_slots: the fit kernel's per-job u32 count slots
  DevBuf<uint32_t> lds_rows;                         // the job (mask row) of each count slot, ~0 = none
  int num_cu = 256;
  int fit_path_mask = PATHS_ALL;   // allowed paths (pe_config.fit_path_mask)
  pe::PlaneSpec plane{};
  int64_t pl_nblk = 0;                   // planes path: 8192-node blocks
  bool pl_rows = true;                   // planes path: row-major sweep kernel (else block-major streams)
  int64_t pl_R = 1;                      // row-major kernel: job phases of the uploaded batch
  int64_t pl_pitch = 0;                  // row-major mask pitch in 8192-node blocks (>= pl_nblk)
  // A batch with more than PL_MAX distinct (dimension, value) pairs is split into plane sets of at
  // most PL_MAX pairs each (row-major layout only); each set is encoded and swept on its own by
  // the indexed-row kernel, its jobs' codes carrying their mask rows.
  struct PlaneSet {
    pe::PlaneSpec spec;
    int64_t J, R, Jr, off;   // jobs, phases, phase stride, first code / count slot
  };
  std::vector<PlaneSet> pl_sets;        // empty: one set (ctx->plane, the rows kernel)
  DevBuf<pe::PlaneSpec> pl_specs_d;     // multi-set: the sets' specs and {off, J, Jr} on the device
  DevBuf<int64_t> pl_meta_d;
  std::vector<int64_t> pl_cnt_row;      // multi-set: count slot -> job row (-1: padding)
  int64_t pl_counts_n = 0;              // count slots of the planes path
  DevBuf<uint32_t> planes;
  DevBuf<uint64_t> plane_jobs;
  pe::CodeSpec code{};
  int64_t code_Jp = 0, node_stride = 0;
  DevBuf<int64_t> code_vals;
  DevBuf<uint32_t> code_needs, code_jobs, code_x;
  DevBuf<uint64_t> mask;
  DevBuf<unsigned long long> counts;
  HostBuf<unsigned long long> h_counts;
  // aggregation: segmented batch and outputs in pinned, device-mapped host memory (pe_kernels.h
  // AggSegHdr); the device-resident arrays below only serve the PE_AGG_DEVICE=1 A/B path
  HostBuf<uint8_t> a_stage, a_outh;
  DevBuf<uint8_t> a_dstage;              // large batches: the packed batch DMA'd to the device chunk by chunk
  hipStream_t a_h2d = nullptr;           // ... on this copy stream (the kernels wait on its events)
  std::vector<hipEvent_t> a_ev_h2d;
  HostBuf<int64_t> a_segoff;
  HostBuf<uint32_t> a_flag;
  std::vector<hipEvent_t> a_ev;   // large batches: one per chunk (its outputs are copied out when it is done)
  DevBuf<uint32_t> a_ctr;   // latency launches: blocks done (the last one stores the flag)
  uint32_t agg_gen = 0;
  std::vector<std::vector<AggSeg>> agg_segs;   // per planning range, reused across calls (no allocation per call)
  std::vector<AggSeg> agg_all;                 // all segments in order
  DevBuf<int32_t> a_jgo, a_mm, a_rep, a_gco, a_mem;
  DevBuf<int64_t> a_req, a_out;
  DevBuf<uint8_t> a_fl, a_pres, a_ovf;
  // 128-bit aggregation (pe_pg_min_resources_wide): the gathered sub-batch, its device copy (inputs then
  // outputs) and the outputs read back; the jobs that go wide, the per-job wide-input marks and the
  // int64 pass's copy of the low limbs with those jobs zeroed.  Grow and are reused.
  HostBuf<uint8_t> aw_stage, aw_outh;
  DevBuf<uint8_t> aw_dev;
  std::vector<int64_t> aw_jobs, aw_lo;
  std::vector<uint8_t> aw_mark;
  // gang capacity (pe_engine_capacity.cpp; the shapes, their dedupe and the events serve all three calls):
  // the call's distinct shapes and pe_gang_capacity's results (pinned), the device copies, the
  // per-node-block partials, the dedupe table and each job's shape.  Grow and are reused; nothing of the
  // staged fit mask is shared.
  HostBuf<pe::CapShape> cp_hshapes;
  HostBuf<pe::CapAcc> cp_hout;
  DevBuf<pe::CapShape> cp_shapes;
  DevBuf<pe::CapAcc> cp_part, cp_out;
  std::vector<pe::CapShape> cp_uniq;
  std::vector<int32_t> cp_tab, cp_of;
  hipEvent_t cp_ev[2] = {nullptr, nullptr};   // PE_CAP_EVENTS=1: around the call's kernels
  // gang capacity over topology levels (pe_gang_capacity_domains = one level, pe_gang_capacity_tree: one host
  // path, pe_engine_capacity.cpp capacity_levels; shapes, dedupe and events are cp_*).  Every call sizes and
  // fills what it uses, so calls of any shape may alternate.  Grow and are reused; nothing outlives a call.
  DevBuf<uint64_t> lv_leaf;     // per launch of sc shapes: slots u64 [sc][L0], then nodes u32 [sc][L0]
  DevBuf<uint64_t> lv_upper;    // the same for the U columns of the levels above the leaves
  HostBuf<uint64_t> lv_hslots;  // a launch's tables on their way out: leaf rows [sc][L0], then upper rows [sc][U]
  HostBuf<uint32_t> lv_hnodes;
  HostBuf<int32_t> lv_hin;      // one copy in: the plan's words, then (16-B aligned) the P picks
  DevBuf<int32_t> lv_in;
  DevBuf<uint32_t> lv_out;      // one copy out: P TreeSel records, then the counts [P][n_levels]
  HostBuf<uint32_t> lv_hout;
  DevBuf<int32_t> lv_split;     // pe_gang_split_tree: one slice of picks' parts (pe_split_plan.h SplitLayout), 64 MiB at most
  HostBuf<int32_t> lv_hsplit;
  std::vector<uint64_t> lv_pkeys;          // the call's distinct (shape, count, max_level), packed
  std::vector<int32_t> lv_ptab, lv_pof;    // their dedupe table, each job's pick
  pe::SlicePlan sl_plan;                   // pe_gang_slice_tree: the call's rows and picks (its buffers are cp_* and lv_*)
  // why a shape fits no node (pe_fit_explain, pe_engine_explain.cpp): the call's distinct (request, need, domain)
  // records, their dedupe table and each job's record, the leaf -> level-domain map; one block in (the records, then
  // the map), one launch's tables on the device ([chunk][32] counts, then [chunk][4] near values) and every
  // launch's tables on their way out.  Grow and are reused; nothing outlives a call.
  std::vector<pe::ExplainRec> ex_uniq;
  std::vector<int32_t> ex_tab, ex_of, ex_leaf;
  HostBuf<uint8_t> ex_hin;
  DevBuf<uint8_t> ex_in;
  DevBuf<uint64_t> ex_out;
  HostBuf<uint64_t> ex_hout;
  // the domain calls (pe_place_greedy_domains and pe_place_min_member_domains, pe_engine_place.cpp;
  // pe_gang_fit_domains, pe_engine_fit.cpp; pe_place_first_fit_domains, pe_engine_first_fit.cpp;
  // pe_gang_preempt_domains, pe_engine_preempt.cpp; their shared host path: pe_domain_call.h).  One set for all of
  // them: calls on a context are serialised (guarded), and every call sizes and fills what it reads -- each span it
  // reads back is written by its kernels or preset by its own memsets -- so calls of any shape may alternate with
  // each other and with every other entry point; nothing of a hierarchy, a batch, a pair list or a victim list
  // outlives a call.  Grow and are reused.
  HostBuf<uint8_t> dm_hin;      // one copy in: the call's own block, G PlaceGroup first, the plan's words last (each
  DevBuf<uint8_t> dm_in;        // unit's *_at offsets)
  DevBuf<uint8_t> dm_out;       // one copy out: the call's answers, again in its own layout
  HostBuf<uint8_t> dm_hout;
  DevBuf<int32_t> dm_log;       // the placing calls' rollback logs, [pods][3]
  DevBuf<int32_t> dm_dom;       // per active domain: node count [A], segment bounds [A + 1], fill cursor [A]
  DevBuf<int64_t> dm_seg;       // the segments' residuals [4][stride]: read-only to the judging calls, the working
                                // residuals of the placing ones
  DevBuf<uint32_t> dm_segw;     // their global ids and labels, [2][stride]
  HostBuf<int32_t> dm_hoff;     // the segment bounds read back (only when the shard has more than PL_LDS_NODES nodes)
  hipEvent_t dm_ev = nullptr;   // ... and the event behind that copy: the host waits for it, not for the units behind it
  HostBuf<uint8_t> dm_hlarge;   // the FitLarge records of the segments above PL_LDS_NODES nodes
  DevBuf<uint8_t> dm_large;
  DevBuf<int64_t> dm_scratch;   // their working copies: at most (1 + FIT_SCRATCH_MULT) x Ns nodes of 4 int64
  DevBuf<int32_t> pp_place;     // pe_gang_preempt_domains: node -> place in the segments' arrays [Ns], -1 = in no
                                // active domain
  DevBuf<uint64_t> ff_state;    // pe_place_first_fit_domains: the rounds' state: the jobs' words [J], the unsettled
                                // count, the queue cursors [A]
  HostBuf<uint32_t> ff_hopen;   // ... and the unsettled count read back
  // giving back and re-taking placed gangs (pe_release_gangs, pe_assume_gangs, pe_engine_ledger.cpp): the plan with
  // its node -> scratch map (kept all -1 between calls, sized by the inventory) and the records of this shard's
  // touched nodes on their way in.  Grow and are reused; nothing of the gangs outlives a call.
  pe::LedgerPlan ld_plan;
  HostBuf<pe::LedgerRec> ld_hin;
  DevBuf<pe::LedgerRec> ld_in;
  // can a node's pods move elsewhere (pe_drain_fit_domains, pe_engine_drain.cpp): the plan with its node ->
  // candidate map (kept all -1 between calls, sized by the inventory); the buffers are the domain calls' dm_*.
  pe::DrainPlan dr_plan;
  // greedy
  DevBuf<ReqRec> g_groups;
  DevBuf<uint64_t> g_cand, g_bound;
  DevBuf<int32_t> g_cnt;
  DevBuf<uint8_t> g_out, g_gath;
  DevBuf<int64_t> g_upd;
  DevBuf<uint64_t> g_kn;   // scan: node-only score terms K(n) (prep_nodes), refreshed by apply
  DevBuf<uint32_t> g_lo;   // scan: lo20(r1) / lo24(r3), [2][stride]
  HostBuf<ReqRec> h_groups, h_groups2;   // h_groups2: the window requests of blob buffer 1 (signalled walk)
  HostBuf<ReqRec> h_groupsx[2];           // blob buffers 2, 3 (pipeline depth 2, 3)
  HostBuf<uint8_t> h_outx[2];             // blob buffers 2, 3
  HostBuf<int64_t> h_updx[2];             // update staging slots 1, 2 (pipeline depth 2, 3)
  uint32_t walk_gen = 0;                  // generation of the last signalled walk window (never 0)
  int pin_cpu = -2;                       // greedy thread pinning at world > 1: a CPU of this rank's L3 (-2: not chosen yet)
  HostBuf<uint8_t> h_out, h_out2, h_own;   // h_out2: the pipelined loop's second blob buffer (h_outx: 3rd, 4th)
  HostBuf<uint8_t> h_merged;                // host-exchange windows: the device-merged lists
  HostBuf<uint8_t> h_xg[4];                 // pipelined host exchange: the gathered lists of blob buffer b
  std::vector<const uint64_t*> x_lists;     // host merge of the gathered lists (exchange thread scratch)
  std::vector<int32_t> x_ns, x_hd;
  HostBuf<int64_t> h_upd;
  // greedy sorted walk (pe_kernels.h WalkIndex; the default window path, greedy_flags bit1 = full scan)
  bool walk = true;
  int64_t resort_nodes = 20480;  // re-sort once this many applied updates joined the overlay
  int64_t w_est = 0;             // updates applied since the last sort (>= overlay size)
  // two index sets: the walks read ws[w_cur]; the next one is rebuilt on the side stream w_s2
  // (lowest priority) while the walks go on (walk_resort_async), then taken over (walk_switch)
  struct WalkSet {
    DevBuf<uint64_t> sk, rmin;
    DevBuf<int64_t> sr, rmax;
    DevBuf<uint32_t> sl, pos, ror, inovl, ovidx, ovlab;
    DevBuf<int64_t> ovres;
    DevBuf<uint64_t> ovkn;
    DevBuf<int32_t> ovl, ovln;
    void release() {
      sk.release(); rmin.release(); sr.release(); rmax.release(); sl.release(); pos.release(); ror.release();
      inovl.release(); ovidx.release(); ovlab.release(); ovres.release(); ovkn.release(); ovl.release(); ovln.release();
    }
  } ws[2];
  int w_cur = 0;
  bool w_pending = false;        // ws[1 - w_cur] is being rebuilt on w_s2
  int64_t w_pend_est = 0;        // updates applied since that rebuild's snapshot
  int64_t w_pend_windows = 0;    // windows launched while that rebuild was pending
  hipStream_t w_s2 = nullptr;
  hipEvent_t w_ev_snap = nullptr, w_ev_done = nullptr;
  DevBuf<uint64_t> w_kin;
  DevBuf<uint32_t> w_slow;       // saturating nodes of the side-stream rebuild (walk_switch adds them)
  DevBuf<uint8_t> w_temp;
  DevBuf<uint32_t> w_flush;   // PE_WALK_FLUSH: 512 MiB rewritten before each walk (cold-cache diagnostics)
  DevBuf<unsigned long long> w_stat;   // walk counters of the current pe_place_greedy (rounds, overlay)
  DevBuf<uint64_t> g_xstatus;          // zero-copy exchange: the window's wait status (launch_xwait)
  pe_stats stats{};

  ~pe_ctx() {
    (void)hipSetDevice(device);
    if (comm_abort.joinable()) comm_abort.join();
    if (stream) (void)hipStreamSynchronize(stream);
    res0.release(); res.release(); labels.release(); island.release(); n_upd.release();
    fit_jobs.release(); fit_jobs32.release(); res32.release(); mask.release();
    code_vals.release(); code_needs.release(); code_jobs.release(); code_x.release(); counts.release(); h_counts.release();
    planes.release(); plane_jobs.release();
    lds_spec_d.release(); lds_vals.release(); lds_codes.release(); lds_ranks.release(); lds_aux.release(); lds_slots.release(); lds_rows.release();
    a_stage.release(); a_outh.release(); a_segoff.release(); a_flag.release(); a_ctr.release();
    for (hipEvent_t e : a_ev) (void)hipEventDestroy(e);
    if (a_h2d) (void)hipStreamSynchronize(a_h2d);
    for (hipEvent_t e : a_ev_h2d) (void)hipEventDestroy(e);
    if (a_h2d) (void)hipStreamDestroy(a_h2d);
    a_dstage.release();
    a_jgo.release(); a_mm.release(); a_rep.release(); a_gco.release(); a_mem.release();
    a_req.release(); a_out.release(); a_fl.release(); a_pres.release(); a_ovf.release();
    aw_stage.release(); aw_outh.release(); aw_dev.release();
    cp_hshapes.release(); cp_hout.release(); cp_shapes.release(); cp_part.release(); cp_out.release();
    lv_leaf.release(); lv_upper.release(); lv_hslots.release(); lv_hnodes.release();
    lv_hin.release(); lv_in.release(); lv_out.release(); lv_hout.release(); lv_split.release(); lv_hsplit.release();
    dm_hin.release(); dm_in.release(); dm_out.release(); dm_hout.release(); dm_log.release(); dm_dom.release();
    dm_seg.release(); dm_segw.release(); dm_hoff.release(); dm_hlarge.release(); dm_large.release(); dm_scratch.release();
    pp_place.release(); ff_state.release(); ff_hopen.release();
    ex_hin.release(); ex_in.release(); ex_out.release(); ex_hout.release();
    ld_hin.release(); ld_in.release();
    if (dm_ev) (void)hipEventDestroy(dm_ev);
    for (hipEvent_t e : cp_ev)
      if (e) (void)hipEventDestroy(e);
    g_groups.release(); g_cand.release(); g_bound.release(); g_cnt.release(); g_out.release(); g_gath.release();
    g_upd.release(); g_kn.release(); g_lo.release(); h_groups.release(); h_groups2.release(); h_out.release(); h_out2.release(); h_own.release(); h_merged.release(); h_upd.release();
    for (auto& x : h_xg) x.release();
    for (int i = 0; i < 2; ++i) {
      h_groupsx[i].release();
      h_outx[i].release();
      h_updx[i].release();
    }
    if (w_s2) (void)hipStreamSynchronize(w_s2);
    for (auto& x : ws) x.release();
    w_kin.release(); w_slow.release(); w_temp.release(); w_stat.release(); w_flush.release(); g_xstatus.release();
    if (w_ev_snap) (void)hipEventDestroy(w_ev_snap);
    if (w_ev_done) (void)hipEventDestroy(w_ev_done);
    if (w_s2) (void)hipStreamDestroy(w_s2);
    if (comm) (void)ncclCommDestroy(comm);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace pe_engine {

// A collective timed out (pe::CollectiveTimeout): abort the communicator without blocking the caller.
// ncclCommAbort raises the communicator's abort flag, which the stuck collective kernel polls, and then
// frees its resources (the frees wait for the device work in flight); on its own thread, so the call
// that timed out returns PE_ERCCL within the bound; pe_destroy joins it.
inline void rccl_abort(pe_ctx* ctx) {
  if (!ctx->comm) return;
  ncclComm_t c = ctx->comm;
  ctx->comm = nullptr;
  ctx->comm_aborted = true;
  const int dev = ctx->device;
  ctx->comm_abort = std::thread([c, dev] {
    (void)hipSetDevice(dev);
    (void)ncclCommAbort(c);
  });
}

// Every ABI entry runs its body through here: lock, select device, map exceptions to codes.
template <class F>
int guarded(pe_ctx* ctx, F&& body) {
  if (!ctx) return PE_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->err.clear();
  try {
    hipchk(hipSetDevice(ctx->device), "hipSetDevice");
    return body();
  } catch (const PeError& e) {
    ctx->err = e.msg;
    return e.code;
  } catch (const std::bad_alloc&) {
    ctx->err = "host allocation failed";
    return PE_ENOMEM;
  } catch (const pe::CollectiveTimeout& e) {   // an RCCL window's all-gather never completed
    ctx->err = e.what();
    rccl_abort(ctx);
    return PE_ERCCL;
  } catch (const pe::ExchangeError& e) {   // a zero-copy window's peer lists never arrived
    ctx->err = e.what();
    return PE_ERCCL;
  } catch (const std::runtime_error& e) {   // pe::WindowFeed: a walk group the device never signalled
    ctx->err = e.what();
    return PE_EHIP;
  } catch (...) {
    ctx->err = "unexpected C++ exception";
    return PE_EINVAL;
  }
}

inline void need_ptr(const void* p, const char* name) {
  if (!p) raise(PE_EINVAL, std::string(name) + " is NULL");
}

// PE_CAP_EVENTS=1 (diagnostics, tools/gang_capacity*_latency.py, tools/place_domains_latency.py,
// tools/gang_fit_latency.py, tools/first_fit_latency.py): hipEvents on the context's stream around a call's
// kernels; a successful call then leaves "S=<shapes> [P=<picks>] kernels_ms=<time>" (the capacity calls),
// "A=<active domains> kernels_ms=<time>" (pe_place_greedy_domains), "A=<active domains> U=<units>
// kernels_ms=<time>" (pe_gang_fit_domains) or "A=<active domains> rounds=<rounds launched> kernels_ms=<time>"
// (pe_place_first_fit_domains) or "A=<active domains> U=<units> judged=<judgements> kernels_ms=<time>"
// (pe_gang_preempt_domains) or "T=<records of this shard> steps=<steps> plan_us=<host plan time> kernels_ms=<time>"
// (pe_release_gangs, pe_assume_gangs) or "A=<active domains> U=<units> E=<evicted pods> kernels_ms=<time>"
// (pe_drain_fit_domains) in pe_last_error.  The variable is read on EVERY call, unlike the greedy's knobs: the latency tools switch
// it on and off inside one process.
struct CapEvents {
  pe_ctx* ctx;
  const bool on;
  bool recorded = false;
  explicit CapEvents(pe_ctx* c) : ctx(c), on(std::getenv("PE_CAP_EVENTS") != nullptr) {}
  void begin() {
    if (!on) return;
    for (hipEvent_t& e : ctx->cp_ev)
      if (!e) hipchk(hipEventCreate(&e), "event create");
    hipchk(hipEventRecord(ctx->cp_ev[0], ctx->stream), "event record");
  }
  void end() {
    if (!on) return;
    hipchk(hipEventRecord(ctx->cp_ev[1], ctx->stream), "event record");
    recorded = true;
  }
  // after the stream was synchronised; P < 0: the call has no picks; no kernels ran: 0 ms
  void report(int64_t S, int64_t P = -1) {
    report_as("S=" + std::to_string(S) + (P < 0 ? "" : " P=" + std::to_string(P)));
  }
  void report_as(const std::string& what) {
    if (!on) return;
    float ms = 0.f;
    if (recorded) hipchk(hipEventElapsedTime(&ms, ctx->cp_ev[0], ctx->cp_ev[1]), "event elapsed");
    ctx->err = what + " kernels_ms=" + std::to_string(ms);
  }
};

// pe_engine.cpp's planning pool: f(0) on the caller, f(1 .. n-1) on pool threads; returns when all are
// done, rethrows the first exception.
void plan_pool_run(int n, const std::function<void(int)>& f);

// The first index in [0, n) where bad(i) holds, or n: chunks of 4096 reduced branch-free (the
// loops vectorise), on the planning pool for large arrays (the aggregation validates ~10^7 values
// per call).
template <class Bad>
int64_t first_bad(int64_t n, Bad bad) {
  constexpr int64_t kChunk = 4096;
  auto scan = [&](int64_t b, int64_t e) -> int64_t {
    for (int64_t c = b; c < e; c += kChunk) {
      const int64_t ce = std::min(e, c + kChunk);
      bool any = false;
      for (int64_t i = c; i < ce; ++i) any |= bad(i);
      if (any)
        for (int64_t i = c; i < ce; ++i)
          if (bad(i)) return i;
    }
    return e;
  };
  if (n < (int64_t(1) << 20)) return scan(0, n);
  constexpr int kT = 8;
  int64_t first[kT];
  plan_pool_run(kT, [&](int t) {
    const int64_t b = n * t / kT, e = n * (t + 1) / kT;
    const int64_t r = scan(b, e);
    first[t] = r < e ? r : n;
  });
  int64_t r = n;
  for (int t = 0; t < kT; ++t) r = std::min(r, first[t]);
  return r;
}

// (pe_engine.cpp)
void check_req(const int64_t* req, int64_t n, const char* what);
void check_offsets(const int32_t* off, int64_t n, int64_t limit, const char* what);
// (pe_domain_call.cpp) What pe_place_greedy checks of a batch's groups (n_jobs > 0): the offsets, the counts
// and the requests, with the first offending index; returns G.  And a refused hierarchy (pe_tree_plan.h
// TreePlanError, `bad` its index) in pe_gang_capacity_tree's words.
int64_t check_gang_groups(int64_t n_jobs, const int32_t* job_group_off, const int32_t* group_count,
                          const int64_t* group_req);
[[noreturn]] void raise_tree(int tree_error, int64_t bad);
// (pe_domain_call.cpp) What pe_place_greedy_domains checks of a batch (n_jobs > 0) and its outputs; returns G.
int64_t check_place_batch(int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                          const int32_t* group_count, const int64_t* group_req, const int32_t* out_pod_node,
                          const int32_t* out_job_status);

inline void fill_req(ReqRec& r, const int64_t* q, uint32_t need) {
  std::memset(&r, 0, sizeof(r));
  for (int d = 0; d < pe::D; ++d) r.q[d] = q[d];
  r.need = need;
}

}  // namespace pe_engine
