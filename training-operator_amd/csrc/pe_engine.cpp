// libplacement: context, device-resident inventory, C ABI entry points (include/placement.h) -- all but
// the greedy placement, which is pe_engine_greedy.cpp, and the gang-capacity calls, which are
// pe_engine_capacity.cpp; the context itself is pe_ctx.h.
//
// One context = one process = one GPU = one contiguous shard of the node inventory.  The
// inventory lives on the device as int64 struct-of-arrays res[4][stride] (+ labels, islands),
// so every kernel streams each dimension coalesced.  Sharded contexts exchange per-group
// candidate lists with one RCCL all-gather per scan window (or a host callback in tests).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <immintrin.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <condition_variable>
#include <atomic>
#include <chrono>
#include <exception>
#include <functional>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

#include "pe_ctx.h"
#include "pe_hostx.h"
#include "pe_kernels.h"
#include "pe_resolver.h"
#include "placement.h"

namespace {

// Bound of the communicator set-up: PE_RCCL_INIT_TIMEOUT_S seconds (default 120).
double rccl_init_timeout_ms() {
  const char* e = std::getenv("PE_RCCL_INIT_TIMEOUT_S");
  const double s = e ? std::atof(e) : 120.0;
  return (s > 0 ? s : 120.0) * 1e3;
}

// ncclCommInitRank with a time bound: a rank whose peers never arrive (a wrong comm_id, a dead
// peer) gets PE_ERCCL instead of hanging in the bootstrap, which has no timeout of its own.  The
// blocking call runs on a helper thread; past the bound the call is abandoned: the thread stays
// behind (detached) and destroys the communicator itself if the peers ever do arrive.  (A
// non-blocking communicator, ncclConfig_t.blocking = 0, still blocked in the bootstrap on this
// RCCL, and ncclCommAbort of a set-up in progress waits for it: profiles/r10_rccl_init.txt.)
ncclComm_t comm_init_bounded(int device, int world, const ncclUniqueId& id, int rank, double timeout_ms) {
  struct State {
    std::mutex m;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclResult_t r = ncclSuccess;
    ncclComm_t comm = nullptr;
  };
  auto st = std::make_shared<State>();
  std::thread([st, device, world, id, rank] {
    (void)hipSetDevice(device);   // the current device is per thread
    ncclComm_t c = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c, world, id, rank);
    std::lock_guard<std::mutex> lk(st->m);
    if (st->abandoned) {
      if (r == ncclSuccess && c) (void)ncclCommDestroy(c);
      return;
    }
    st->r = r;
    st->comm = c;
    st->done = true;
    st->cv.notify_all();
  }).detach();
  std::unique_lock<std::mutex> lk(st->m);
  if (!st->cv.wait_for(lk, std::chrono::duration<double, std::milli>(timeout_ms), [&] { return st->done; })) {
    st->abandoned = true;
    raise(PE_ERCCL, "ncclCommInitRank: the " + std::to_string(world) + " ranks did not meet within " +
                        std::to_string((int)(timeout_ms / 1e3)) + " s (PE_RCCL_INIT_TIMEOUT_S)");
  }
  ncclchk(st->r, "ncclCommInitRank");
  return st->comm;
}

// Persistent helpers for the batch planning (pe_jobs_upload is on the batch's path; creating and
// joining a thread per task cost tens of us each).  run(n, f): f(0) on the caller, f(1 .. n-1) on
// up to 7 pool threads, returns when all are done, rethrows the first exception.  The threads
// sleep on a condition variable between calls; the pool lives for the process.
// PE_NO_POOL=1: a thread per task instead (A/B).
class PlanPool {
 public:
  static constexpr int kMax = 16;
  static PlanPool& get() {
    static PlanPool* p = new PlanPool();   // never destroyed: its threads may still wait at exit
    return *p;
  }
  void run(int n, const std::function<void(int)>& f) {
    n = std::max(1, std::min(n, kMax));
    std::vector<std::exception_ptr> err((size_t)n);
    if (n > 1 && std::getenv("PE_NO_POOL")) {
      std::vector<std::thread> th;
      for (int t = 1; t < n; ++t)
        th.emplace_back([&, t] {
          try {
            f(t);
          } catch (...) {
            err[(size_t)t] = std::current_exception();
          }
        });
      try {
        f(0);
      } catch (...) {
        err[0] = std::current_exception();
      }
      for (auto& x : th) x.join();
    } else if (n > 1) {
      std::lock_guard<std::mutex> serial(call_mu_);   // one planning call at a time on the pool
      {
        std::lock_guard<std::mutex> lk(mu_);
        while ((int)th_.size() < n - 1) {
          const int id = (int)th_.size();
          th_.emplace_back([this, id] { loop(id); });
        }
        task_ = &f;
        errs_ = &err;
        want_ = n - 1;
        left_ = n - 1;
        ++gen_;
        agen_.store(gen_, std::memory_order_release);
      }
      cv_.notify_all();
      try {
        f(0);
      } catch (...) {
        err[0] = std::current_exception();
      }
      std::unique_lock<std::mutex> lk(mu_);
      done_cv_.wait(lk, [this] { return left_ == 0; });
      task_ = nullptr;
    } else {
      try {
        f(0);
      } catch (...) {
        err[0] = std::current_exception();
      }
    }
    for (auto& e : err)
      if (e) std::rethrow_exception(e);
  }

 private:
  // A worker that just finished spins for up to spin_us() before it sleeps on the condition variable:
  // a chunked call dispatches plan / pack / copy-out back to back (24 dispatches in a 1M-job
  // aggregation), and a futex wake-up per dispatch cost ~50 us each.
  static int spin_us() {   // PE_POOL_SPIN_US (0..2000, default 150; A/B)
    static const int v = [] {
      const char* e = std::getenv("PE_POOL_SPIN_US");
      return e ? std::max(0, std::min(2000, std::atoi(e))) : 150;
    }();
    return v;
  }
  void loop(int id) {
    uint64_t seen = 0;
    bool ran = false;
    for (;;) {
      const std::function<void(int)>* f;
      std::vector<std::exception_ptr>* errs;
      if (ran && spin_us() > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned i = 1; agen_.load(std::memory_order_acquire) == seen; ++i) {
          _mm_pause();
          if ((i & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us())) break;
        }
      }
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        ran = id < want_;
        if (!ran) continue;   // not needed for this call
        f = task_;
        errs = errs_;
      }
      try {
        (*f)(id + 1);
      } catch (...) {
        (*errs)[(size_t)id + 1] = std::current_exception();
      }
      std::lock_guard<std::mutex> lk(mu_);
      if (--left_ == 0) done_cv_.notify_one();
    }
  }
  std::mutex call_mu_, mu_;
  std::condition_variable cv_, done_cv_;
  std::vector<std::thread> th_;
  const std::function<void(int)>* task_ = nullptr;
  std::vector<std::exception_ptr>* errs_ = nullptr;
  int want_ = 0, left_ = 0;
  uint64_t gen_ = 0;
  std::atomic<uint64_t> agen_{0};   // gen_, for the spinning workers (written under mu_)
};

}  // namespace

namespace pe_engine {

void plan_pool_run(int n, const std::function<void(int)>& f) { PlanPool::get().run(n, f); }

void check_req(const int64_t* req, int64_t n, const char* what) {
  const int64_t i = first_bad(n * pe::D, [req](int64_t k) { return req[k] < 0; });
  if (i < n * pe::D) raise(PE_EINVAL, std::string(what) + ": negative request at index " + std::to_string(i));
}

void check_offsets(const int32_t* off, int64_t n, int64_t limit, const char* what) {
  if (off[0] != 0) raise(PE_EINVAL, std::string(what) + "[0] must be 0");
  if (first_bad(n, [off](int64_t i) { return off[i + 1] < off[i]; }) < n)
    raise(PE_EINVAL, std::string(what) + " is not monotonic");
  if (limit >= 0 && off[n] > limit) raise(PE_EINVAL, std::string(what) + " exceeds its array");
}

}  // namespace pe_engine

namespace {

// body(j0, j1) over [0, n) in contiguous chunks: on up to 8 threads for large batches (the batch
// planning is on the upload's path), inline for small ones.  Exceptions are rethrown here.
template <class Body>
void parallel_for(int64_t n, Body body) {
  const int64_t nt = n < 32768 ? 1 : std::min<int64_t>(8, std::max(1u, std::thread::hardware_concurrency()));
  if (nt <= 1) {
    body(0, n);
    return;
  }
  PlanPool::get().run((int)nt, [&](int t) { body(n * t / nt, n * (t + 1) / nt); });
}

}  // namespace

extern "C" {

int pe_abi_version(void) { return PE_ABI_VERSION; }

int pe_comm_id(uint8_t out[PE_COMM_ID_BYTES]) {
  if (!out) return PE_EINVAL;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return PE_ERCCL;
  static_assert(sizeof(id) <= PE_COMM_ID_BYTES, "unique id size");
  std::memset(out, 0, PE_COMM_ID_BYTES);
  std::memcpy(out, &id, sizeof(id));
  return PE_OK;
}

int pe_create(const pe_config* cfg, pe_ctx** out) {
  if (!cfg || !out) return PE_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PE_ENODEV;
  if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) return PE_EINVAL;
  if (cfg->max_nodes < 0 || cfg->max_nodes > PE_MAX_NODES) return PE_EINVAL;
  pe_ctx* ctx = new (std::nothrow) pe_ctx();
  if (!ctx) return PE_ENOMEM;
  int dev = cfg->device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= ndev) {
    delete ctx;
    return PE_EINVAL;
  }
  ctx->device = dev;
  ctx->rank = cfg->rank;
  ctx->world = cfg->world_size;
  ctx->exchange = cfg->exchange;
  ctx->exchange_user = cfg->exchange_user;
  ctx->max_nodes = cfg->max_nodes > 0 ? cfg->max_nodes : PE_MAX_NODES;
  ctx->topk = cfg->topk > 0 ? std::min(cfg->topk, pe::MG_CAP) : 256;
  // 112 groups per window (round 5, 4 interleaved reps on the bench batch: 128 / 112 / 104 / 96 groups
  // 9.53 / 9.25 / 9.53 / 9.50 ms per batch, host 7.98 / 7.65 / 7.70 / 7.38 ms -- smaller windows shrink
  // the resolver's dirty sets, below ~112 the walk + apply chain per window outlasts the resolve)
  ctx->window_groups = cfg->window_groups > 0 ? cfg->window_groups : 112;
  ctx->window_pods = cfg->window_pods > 0 ? cfg->window_pods : 1024;
  ctx->gpu_name = cfg->gpu_resource_name ? cfg->gpu_resource_name : "amd.com/gpu";
  ctx->fit_path_mask = cfg->fit_path_mask & (PATHS_ALL | PATH_NO_THERM | PATH_PLANES_BLOCKS);
  ctx->pl_rows = !(ctx->fit_path_mask & PATH_PLANES_BLOCKS);
  ctx->pipeline = (cfg->greedy_flags & 1) == 0;
  // the walk's block holds K + 1 <= WK_ROUND selected keys; larger K takes the full scan + merge
  ctx->walk = (cfg->greedy_flags & 2) == 0 && ctx->topk + 1 <= pe::WK_ROUND;
  if (cfg->resort_nodes < 0) raise(PE_EINVAL, "resort_nodes < 0");
  ctx->resort_nodes = cfg->resort_nodes > 0 ? cfg->resort_nodes : 20480;   // (profiles/r12_async_resort.txt)
  if (!(ctx->fit_path_mask & PATHS_ALL)) ctx->fit_path_mask |= PATHS_ALL;   // no kernel bits = all kernels
  ctx->fit_path_mask |= PATH_I64;                                           // always available
  int rc = PE_OK;
  try {
    hipchk(hipSetDevice(dev), "hipSetDevice");
    hipchk(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking), "hipStreamCreate");
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0)
      ctx->num_cu = ncu;
    // RCCL whenever shards exchange without a host callback; a comm_id at world_size 1 also
    // builds a 1-rank communicator (exercises the RCCL window path on a single GPU)
    if (!ctx->exchange && (ctx->world > 1 || cfg->comm_id)) {
      if (!cfg->comm_id) raise(PE_EINVAL, "world_size > 1 needs comm_id or an exchange callback");
      ncclUniqueId id;
      std::memcpy(&id, cfg->comm_id, sizeof(id));
      ctx->comm = comm_init_bounded(ctx->device, ctx->world, id, ctx->rank, rccl_init_timeout_ms());
    }
  } catch (const PeError& e) {
    rc = e.code;
  }
  if (rc != PE_OK) {
    delete ctx;
    return rc;
  }
  *out = ctx;
  return PE_OK;
}

void pe_destroy(pe_ctx* ctx) { delete ctx; }

const char* pe_last_error(const pe_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// A node's device / mirror labels: the caller's bits 0-30, bit 31 = the node has an xGMI island
// (PE_LABEL_ISLAND, what an island group's need requires).
static uint32_t node_labels(const uint32_t* labels, const int32_t* island, int64_t i) {
  const uint32_t l = labels ? labels[i] : 0u;
  const bool has = island && island[i] >= 0;
  return (l & ~PE_LABEL_ISLAND) | (has ? PE_LABEL_ISLAND : 0u);
}

int pe_load_nodes(pe_ctx* ctx, int64_t n, const int64_t* cap, const int64_t* used, const uint32_t* labels,
                  const int32_t* island) {
  return guarded(ctx, [&]() -> int {
    if (n < 0 || n > ctx->max_nodes) raise(PE_EINVAL, "node count out of range");
    if (n > 0) {
      need_ptr(cap, "cap");
      need_ptr(used, "used");
    }
    // validate the whole (global) inventory first: a refused load leaves the context as it was
    for (int64_t c = 0; c < (int64_t)pe::D * n; ++c)
      if (cap[c] < 0 || used[c] < 0) raise(PE_EINVAL, "negative capacity/usage");
    // the new state is built aside and taken over once the device holds it
    const int64_t begin = n * ctx->rank / ctx->world, end = n * (ctx->rank + 1) / ctx->world;
    const int64_t Ns = end - begin, stride = round_up(std::max<int64_t>(Ns, 1), 256);
    const size_t cells = (size_t)pe::D * (size_t)stride;
    std::vector<int64_t> r(cells, pe::NEVER);
    std::vector<uint32_t> lab((size_t)stride, 0u);
    std::vector<int32_t> isl((size_t)stride, -1);
    for (int d = 0; d < pe::D; ++d)
      for (int64_t i = 0; i < Ns; ++i) {
        const int64_t g = begin + i;
        r[(size_t)d * stride + i] = cap[d * n + g] - used[d * n + g];
      }
    for (int64_t i = 0; i < Ns; ++i) {
      lab[i] = node_labels(labels, island, begin + i);
      isl[i] = island ? island[begin + i] : -1;
    }
    decltype(ctx->m_nodes) nodes;
    nodes.assign((size_t)n, pe::NodeState{});
    for (int d = 0; d < pe::D; ++d)
      for (int64_t g = 0; g < n; ++g) nodes[g].res[d] = cap[d * n + g] - used[d * n + g];
    for (int64_t g = 0; g < n; ++g) nodes[g].labels = node_labels(labels, island, g);
    decltype(ctx->m_nodes0) nodes0(nodes.begin(), nodes.end());
    try {
      hipchk(ctx->res0.ensure(cells), "alloc res0");
      hipchk(ctx->res.ensure(cells), "alloc res");
      hipchk(ctx->labels.ensure((size_t)stride), "alloc labels");
      hipchk(ctx->island.ensure((size_t)stride), "alloc island");
      hipchk(hipMemcpyAsync(ctx->res0.p, r.data(), cells * 8, hipMemcpyHostToDevice, ctx->stream), "H2D res0");
      hipchk(hipMemcpyAsync(ctx->res.p, r.data(), cells * 8, hipMemcpyHostToDevice, ctx->stream), "H2D res");
      hipchk(hipMemcpyAsync(ctx->labels.p, lab.data(), lab.size() * 4, hipMemcpyHostToDevice, ctx->stream), "H2D lab");
      hipchk(hipMemcpyAsync(ctx->island.p, isl.data(), isl.size() * 4, hipMemcpyHostToDevice, ctx->stream), "H2D isl");
      hipchk(hipStreamSynchronize(ctx->stream), "sync load");
    } catch (...) {
      ctx->loaded = false;   // the device buffers may hold neither inventory: PE_ESTATE until a load succeeds
      throw;
    }
    ctx->n_total = n;
    ctx->begin = begin;
    ctx->end = end;
    ctx->Ns = Ns;
    ctx->stride = stride;
    ctx->m_nodes = std::move(nodes);
    ctx->m_nodes0 = std::move(nodes0);
    // the staged fit batch was planned for the old shard (Wn, Wt, block counts, buffer sizes): a run
    // or a read with the new Ns is PE_ESTATE until the next pe_jobs_upload / pe_fit_mask
    ctx->fit_uploaded = false;
    ctx->loaded = true;
    return PE_OK;
  });
}

int pe_update_nodes(pe_ctx* ctx, int64_t n, const int64_t* slots, const uint8_t* op, const int64_t* cap,
                    const int64_t* used, const uint32_t* labels, const int32_t* island) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (n < 0) raise(PE_EINVAL, "n < 0");
    if (n == 0) return PE_OK;
    need_ptr(slots, "slots");
    need_ptr(op, "op");
    // validate the whole batch first: nothing is applied unless every entry is valid
    bool any_set = false;
    for (int64_t i = 0; i < n; ++i) {
      if (slots[i] < 0 || slots[i] >= ctx->n_total) raise(PE_EINVAL, "slot out of range");
      if (op[i] != PE_NODE_SET && op[i] != PE_NODE_REMOVE) raise(PE_EINVAL, "unknown node op");
      any_set |= op[i] == PE_NODE_SET;
    }
    if (any_set) {
      need_ptr(cap, "cap");
      need_ptr(used, "used");
      for (int64_t i = 0; i < n; ++i)
        if (op[i] == PE_NODE_SET)
          for (int d = 0; d < pe::D; ++d)
            if (cap[i * pe::D + d] < 0 || used[i * pe::D + d] < 0) raise(PE_EINVAL, "negative capacity/usage");
    }
    // the host mirror takes every entry in order (global inventory)
    for (int64_t i = 0; i < n; ++i) {
      const int64_t g = slots[i];
      pe::NodeState& m = ctx->m_nodes[g];
      for (int d = 0; d < pe::D; ++d)
        m.res[d] = op[i] == PE_NODE_SET ? cap[i * pe::D + d] - used[i * pe::D + d] : pe::NEVER;
      m.labels = op[i] == PE_NODE_SET ? node_labels(labels, island, i) : 0u;
      ctx->m_nodes0[g] = m;
    }
    // last entry per slot wins; keep only this shard's slots
    std::unordered_map<int64_t, int64_t> last;
    last.reserve((size_t)n * 2);
    for (int64_t i = 0; i < n; ++i)
      if (slots[i] >= ctx->begin && slots[i] < ctx->end) last[slots[i]] = i;
    std::vector<pe::NodeUpd> upd;
    upd.reserve(last.size());
    for (int64_t i = 0; i < n; ++i) {
      auto it = last.find(slots[i]);
      if (it == last.end() || it->second != i) continue;
      pe::NodeUpd u{};
      u.local = slots[i] - ctx->begin;
      if (op[i] == PE_NODE_SET) {
        for (int d = 0; d < pe::D; ++d) u.res[d] = cap[i * pe::D + d] - used[i * pe::D + d];
        u.labels = node_labels(labels, island, i);
        u.island = island ? island[i] : -1;
      } else {
        for (int d = 0; d < pe::D; ++d) u.res[d] = pe::NEVER;
        u.labels = 0u;
        u.island = -1;
      }
      upd.push_back(u);
    }
    if (upd.empty()) return PE_OK;
    hipchk(ctx->n_upd.ensure(upd.size()), "alloc node updates");
    hipchk(hipMemcpyAsync(ctx->n_upd.p, upd.data(), upd.size() * sizeof(pe::NodeUpd), hipMemcpyHostToDevice,
                          ctx->stream),
           "H2D node updates");
    hipchk(pe::launch_scatter_nodes(ctx->stream, ctx->res.p, ctx->res0.p, ctx->stride, ctx->labels.p, ctx->island.p,
                                    ctx->n_upd.p, (int64_t)upd.size()),
           "launch scatter_nodes");
    hipchk(hipStreamSynchronize(ctx->stream), "sync node updates");   // the host vector dies here
    return PE_OK;
  });
}

int pe_reset_residuals(pe_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    hipchk(hipMemcpyAsync(ctx->res.p, ctx->res0.p, (size_t)pe::D * ctx->stride * 8, hipMemcpyDeviceToDevice,
                          ctx->stream),
           "D2D reset");
    ctx->m_nodes = ctx->m_nodes0;
    return PE_OK;
  });
}

int pe_shard_range(const pe_ctx* ctx, int64_t* begin, int64_t* end) {
  if (!ctx || !begin || !end) return PE_EINVAL;
  *begin = ctx->begin;
  *end = ctx->end;
  return PE_OK;
}

int pe_comm_ranks(const pe_ctx* ctx, int32_t* nranks) {
  if (!ctx || !nranks) return PE_EINVAL;
  *nranks = 0;
  if (!ctx->comm) return PE_OK;
  int n = 0;
  if (ncclCommCount(ctx->comm, &n) != ncclSuccess) return PE_ERCCL;
  *nranks = n;
  return PE_OK;
}

int pe_read_residuals(pe_ctx* ctx, int64_t* res_out) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    need_ptr(res_out, "res_out");
    for (int d = 0; d < pe::D; ++d)
      hipchk(hipMemcpyAsync(res_out + (size_t)d * ctx->Ns, ctx->res.p + (size_t)d * ctx->stride,
                            (size_t)ctx->Ns * 8, hipMemcpyDeviceToHost, ctx->stream),
             "D2H res");
    hipchk(hipStreamSynchronize(ctx->stream), "sync read");
    return PE_OK;
  });
}

}  // extern "C"

namespace {

// Wait for the one-segment aggregation kernel's flag (pinned host memory, written after its outputs).
// The stream is polled now and then: a faulted kernel surfaces as its HIP error, a kernel that ended
// without the flag as PE_EHIP.
void agg_wait_flag(pe_ctx* ctx, uint32_t gen) {
  for (unsigned spin = 1;; ++spin) {
    if (__atomic_load_n(ctx->a_flag.p, __ATOMIC_ACQUIRE) == gen) return;
    _mm_pause();
    if ((spin & 1023) == 0) {
      const hipError_t e = hipStreamQuery(ctx->stream);
      if (e == hipErrorNotReady) continue;
      hipchk(e, "aggregation kernel");
      if (__atomic_load_n(ctx->a_flag.p, __ATOMIC_ACQUIRE) == gen) return;
      raise(PE_EHIP, "aggregation kernel finished without signalling");
    }
  }
}

// The r2 call path (device copies of the six input arrays, four D2H copies): PE_AGG_DEVICE=1 A/B.
void agg_device_path(pe_ctx* ctx, int32_t mode, int64_t n_jobs, int64_t G, int64_t C, const int32_t* job_group_off,
                     const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                     const int64_t* cont_req, const uint8_t* cont_flags, int64_t* out_min_res, uint8_t* out_present,
                     int32_t* out_members, uint8_t* out_overflow) {
  if (C > 0) check_req(cont_req, C, "cont_req");
  hipStream_t s = ctx->stream;
  hipchk(ctx->a_jgo.ensure(n_jobs + 1), "alloc");
  hipchk(ctx->a_mm.ensure(n_jobs), "alloc");
  hipchk(ctx->a_rep.ensure(G), "alloc");
  hipchk(ctx->a_gco.ensure(G + 1), "alloc");
  hipchk(ctx->a_req.ensure((size_t)C * pe::D), "alloc");
  hipchk(ctx->a_fl.ensure(C), "alloc");
  hipchk(ctx->a_out.ensure((size_t)n_jobs * pe::D), "alloc");
  hipchk(ctx->a_pres.ensure(n_jobs), "alloc");
  hipchk(ctx->a_mem.ensure(n_jobs), "alloc");
  hipchk(ctx->a_ovf.ensure(n_jobs), "alloc");
  hipchk(hipMemcpyAsync(ctx->a_jgo.p, job_group_off, (n_jobs + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  if (mode == PE_MODE_V1) hipchk(hipMemcpyAsync(ctx->a_mm.p, min_member, n_jobs * 4, hipMemcpyHostToDevice, s), "H2D");
  if (G > 0) {
    hipchk(hipMemcpyAsync(ctx->a_rep.p, group_replicas, G * 4, hipMemcpyHostToDevice, s), "H2D");
    hipchk(hipMemcpyAsync(ctx->a_gco.p, group_cont_off, (G + 1) * 4, hipMemcpyHostToDevice, s), "H2D");
  }
  if (C > 0) {
    hipchk(hipMemcpyAsync(ctx->a_req.p, cont_req, (size_t)C * pe::D * 8, hipMemcpyHostToDevice, s), "H2D");
    hipchk(hipMemcpyAsync(ctx->a_fl.p, cont_flags, C, hipMemcpyHostToDevice, s), "H2D");
  }
  hipchk(pe::launch_pg_min_resources(s, mode, n_jobs, ctx->a_jgo.p, ctx->a_mm.p, ctx->a_rep.p, ctx->a_gco.p,
                                     ctx->a_req.p, ctx->a_fl.p, ctx->a_out.p, ctx->a_pres.p, ctx->a_mem.p, ctx->a_ovf.p),
         "launch pg_min_resources");
  hipchk(hipMemcpyAsync(out_min_res, ctx->a_out.p, (size_t)n_jobs * pe::D * 8, hipMemcpyDeviceToHost, s), "D2H");
  hipchk(hipMemcpyAsync(out_present, ctx->a_pres.p, n_jobs, hipMemcpyDeviceToHost, s), "D2H");
  hipchk(hipMemcpyAsync(out_members, ctx->a_mem.p, n_jobs * 4, hipMemcpyDeviceToHost, s), "D2H");
  hipchk(hipMemcpyAsync(out_overflow, ctx->a_ovf.p, n_jobs, hipMemcpyDeviceToHost, s), "D2H");
  hipchk(hipStreamSynchronize(s), "sync pg_min_resources");
}

// Per-key OR of rows x 4 int64 request records (the narrowing test of a segment, below)
__attribute__((target("avx2"))) void or_rows4(const int64_t* q, int64_t rows, uint64_t orv[4]) {
  __m256i a = _mm256_setzero_si256(), b = _mm256_setzero_si256();
  int64_t r = 0;
  for (; r + 2 <= rows; r += 2) {
    a = _mm256_or_si256(a, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(q + r * 4)));
    b = _mm256_or_si256(b, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(q + r * 4 + 4)));
  }
  if (r < rows) a = _mm256_or_si256(a, _mm256_loadu_si256(reinterpret_cast<const __m256i*>(q + r * 4)));
  _mm256_storeu_si256(reinterpret_cast<__m256i*>(orv), _mm256_or_si256(a, b));
}

// rows x 4 int64 records -> rows x 4 u32 of value >> sh[key] (the values are known to fit)
// NT: non-temporal stores (dst 16-B aligned): the staging buffer is written once and read by the DMA
// engine, so no line of it is read for ownership first (the pack's host-memory traffic is otherwise
// read + RFO + write)
template <bool NT>
__attribute__((target("avx2"))) void narrow_rows4(uint32_t* dst, const int64_t* q, int64_t rows, const uint8_t sh[4]) {
  const __m256i vs = _mm256_set_epi64x(sh[3], sh[2], sh[1], sh[0]);
  const __m256i even = _mm256_set_epi32(7, 5, 3, 1, 6, 4, 2, 0);
  for (int64_t r = 0; r < rows; ++r) {
    const __m256i v = _mm256_srlv_epi64(_mm256_loadu_si256(reinterpret_cast<const __m256i*>(q + r * 4)), vs);
    const __m128i lo = _mm256_castsi256_si128(_mm256_permutevar8x32_epi32(v, even));
    if constexpr (NT) _mm_stream_si128(reinterpret_cast<__m128i*>(dst + r * 4), lo);
    else _mm_storeu_si128(reinterpret_cast<__m128i*>(dst + r * 4), lo);
  }
}

// memcpy into a 16-B aligned staging section with non-temporal stores (whole 16-B chunks; the tail
// with plain stores)
__attribute__((target("avx2"))) void nt_copy(void* dst, const void* src, size_t bytes) {
  uint8_t* d = static_cast<uint8_t*>(dst);
  const uint8_t* s = static_cast<const uint8_t*>(src);
  size_t i = 0;
  for (; i + 16 <= bytes; i += 16)
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i), _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i)));
  if (i < bytes) std::memcpy(d + i, s + i, bytes - i);
}

// dst[0, n) = src[0, n) and the OR of all values (its sign says whether any is negative), in one
// pass: the aggregation's request records are validated while they are packed.
template <bool NT>
__attribute__((target("avx2"))) int64_t copy_or_i64(int64_t* dst, const int64_t* src, int64_t n) {
  __m256i acc = _mm256_setzero_si256();
  int64_t i = 0;
  for (; i + 4 <= n; i += 4) {
    const __m256i v = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(src + i));
    if constexpr (NT) {   // (dst 16-B aligned: two 16-B streams)
      _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i), _mm256_castsi256_si128(v));
      _mm_stream_si128(reinterpret_cast<__m128i*>(dst + i + 2), _mm256_extracti128_si256(v, 1));
    } else {
      _mm256_storeu_si256(reinterpret_cast<__m256i*>(dst + i), v);
    }
    acc = _mm256_or_si256(acc, v);
  }
  alignas(32) int64_t lanes[4];
  _mm256_store_si256(reinterpret_cast<__m256i*>(lanes), acc);
  int64_t any = lanes[0] | lanes[1] | lanes[2] | lanes[3];
  for (; i < n; ++i) {
    dst[i] = src[i];
    any |= src[i];
  }
  return any;
}

// Grow-only pinned buffer (a 1M-job batch needs ~170 MB; hipHostMalloc costs ms, so keep it).
template <class T>
void ensure_pinned(HostBuf<T>& b, size_t count, const char* what) {
  if (count <= b.n && b.p) return;
  hipchk(b.ensure(std::max(count, b.n + b.n / 2), kZeroCopy), what);
}

// Call path (pe_kernels.h AggSegHdr): validate + pack the batch into segments of <= 256 jobs in a
// pinned, device-mapped staging buffer (on the planning pool for large batches), one block per
// segment (the segment comes into LDS in one round of coalesced 16-B loads), outputs written by the
// kernel straight into a pinned buffer in the caller's layout, then copied out.  Up to 8192 jobs: one
// launch reading the pinned segments over PCIe, the host waiting on a flag the kernel stores in pinned
// memory (the operator's per-reconcile call: one job).  Larger batches: chunks planned, packed, DMA'd
// to the device and launched one after another (below).
// ak / n_keys: the fixed four dimensions ({4, 1}, n_keys 4) or a per-call key table of n_keys <= 16
// keys padded to ak.nd (pe_pg_min_resources_keys); cont_flags / out_present are u8 or u32 / u16.
// agg_call_locked: the call's body, run under the context's lock (guarded); errors are raised.
int agg_call_locked(pe_ctx* ctx, int32_t mode, int64_t n_jobs, pe::AggKeys ak, int n_keys, const int32_t* job_group_off,
                    const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                    const int64_t* cont_req, const void* cont_flags_v, int64_t* out_min_res, void* out_present_v,
                    int32_t* out_members, uint8_t* out_overflow) {
  const uint8_t* cont_flags = static_cast<const uint8_t*>(cont_flags_v);
  uint8_t* out_present = static_cast<uint8_t*>(out_present_v);
  const bool wide = ak.fb != 1;
  const int ND = ak.nd;
  const int pb = wide ? 2 : 1;   // presence bytes per job out
  {
    if (mode != PE_MODE_V1 && mode != PE_MODE_V2) raise(PE_EINVAL, "mode must be PE_MODE_V1 or PE_MODE_V2");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (n_jobs == 0) return PE_OK;
    need_ptr(job_group_off, "job_group_off");
    need_ptr(out_min_res, "out_min_res");
    need_ptr(out_present, "out_present");
    need_ptr(out_members, "out_members");
    need_ptr(out_overflow, "out_overflow");
    if (mode == PE_MODE_V1) need_ptr(min_member, "min_member");
    check_offsets(job_group_off, n_jobs, -1, "job_group_off");
    const int64_t G = job_group_off[n_jobs];
    if (G > 0) {
      need_ptr(group_replicas, "group_replicas");
      need_ptr(group_cont_off, "group_cont_off");
      check_offsets(group_cont_off, G, -1, "group_cont_off");
    }
    const int64_t C = G > 0 ? group_cont_off[G] : 0;
    if (C > 0) {
      need_ptr(cont_req, "cont_req");
      need_ptr(cont_flags, "cont_flags");
    }
    if (wide && C > 0) {   // a key table's flags: presence bits of the call's keys and the kind only
      const uint32_t allowed = ((n_keys >= 32 ? 0u : (1u << n_keys)) - 1u) | (3u << PE_KEYS_KIND_SHIFT);
      const uint32_t* f32 = static_cast<const uint32_t*>(cont_flags_v);
      for (int64_t c = 0; c < C; ++c)
        if (f32[c] & ~allowed)
          raise(PE_EINVAL, "cont_flags[" + std::to_string(c) + "]: presence bit past n_keys or unknown bits");
    }
    if (!wide && std::getenv("PE_AGG_DEVICE")) {
      agg_device_path(ctx, mode, n_jobs, G, C, job_group_off, min_member, group_replicas, group_cont_off, cont_req,
                      cont_flags, out_min_res, out_present, out_members, out_overflow);
    } else {
      const bool v1 = mode == PE_MODE_V1;
      const int32_t* gco = G > 0 ? group_cont_off : nullptr;
      // PE_AGG_TRACE=1: phase times of the call on stderr (diagnostics)
      const bool trace = std::getenv("PE_AGG_TRACE") != nullptr;
      auto now = [] { return std::chrono::steady_clock::now(); };
      const auto tt0 = now();
      double t_pack = 0;
      // 1. segments, per job range (one range below 32k jobs; segments never span ranges)
      // PE_AGG_THREADS (1..16, default 8): host threads planning / packing / copying out a large batch
      static const int kAggT = [] {
        const char* e = std::getenv("PE_AGG_THREADS");
        return e ? std::max(1, std::min(PlanPool::kMax, std::atoi(e))) : 8;
      }();
      const int T = n_jobs < 32768 ? 1 : kAggT;
      // Calls of <= kLatJobs jobs are one launch the host waits on through the kernel's flag; up to
      // 2048 jobs with segments of 32 jobs, so a 256-job call spreads its ~40 KB over 8 CUs (one
      // CU's zero-copy reads come in at a few GB/s: 41 KB through one block took ~27 us, 8 blocks
      // 19 us); larger batches take 256-job segments, above kLatJobs in chunks with a stream sync.
      // PE_AGG_SEG_JOBS overrides the segment size (A/B, profiles/r10_agg_latency.txt).
      constexpr int64_t kLatJobs = 8192;
      int64_t seg_jobs = n_jobs <= 2048 ? 32 : pe::AGG_SEG_JOBS;   // (8192 jobs: 94 us with 256, 112 with 32)
      if (const char* e = std::getenv("PE_AGG_SEG_JOBS")) seg_jobs = std::max<int64_t>(1, std::min<int64_t>(pe::AGG_SEG_JOBS, std::atoll(e)));
      // Large batches run in chunks (PE_AGG_CHUNKS, 1..64, default 8): chunk k's segments are planned
      // and packed by the planning pool while chunk k - 1 crosses PCIe, so the link starts after the
      // first chunk's plan and pack instead of the whole batch's plan (0.3 ms of a 1M-job call).
      static const int64_t kChunks = [] {
        const char* e = std::getenv("PE_AGG_CHUNKS");
        return e ? std::max<int64_t>(1, std::min<int64_t>(64, std::atoll(e))) : 8;
      }();
      const int64_t CH = n_jobs > kLatJobs && T > 1 ? kChunks : 1;
      // PE_AGG_ONE_PLAN=1 (A/B): the whole batch planned before the first chunk is packed
      static const bool one_plan = std::getenv("PE_AGG_ONE_PLAN") != nullptr;
      auto& segs = ctx->agg_segs;
      if (segs.size() < (size_t)T) segs.resize((size_t)T);
      // A segment's requests cross narrowed (pe_kernels.h agg_seg_layout) when every key's values span
      // <= 32 bits above their common trailing zeros, none is negative, and it saves bytes; else as the
      // caller's int64 records.  PE_AGG_WIDE=1: never narrowed (A/B).
      static const bool no_narrow = std::getenv("PE_AGG_WIDE") != nullptr;
      auto narrow_seg = [&](AggSeg& sg) {
        sg.narrow = false;
        if (no_narrow || sg.nc == 0 ||
            pe::agg_req_bytes(sg.nc, ND, true) >= pe::agg_req_bytes(sg.nc, ND, false))
          return;
        const int64_t* q = cont_req + (int64_t)gco[job_group_off[sg.j0]] * n_keys;
        uint64_t orv[pe::AGG_MAX_KEYS] = {0};
        if (n_keys == 4) {
          or_rows4(q, sg.nc, orv);
        } else {
          for (int64_t c = 0; c < sg.nc; ++c)
            for (int k = 0; k < n_keys; ++k) orv[k] |= (uint64_t)q[c * n_keys + k];
        }
        for (int k = 0; k < ND; ++k) {
          const uint64_t v = k < n_keys ? orv[k] : 0;
          if (v >> 63) return;   // a negative request: the wide pack reports it
          const int tz = v ? __builtin_ctzll(v) : 0;
          if (v && 63 - __builtin_clzll(v) - tz > 31) return;
          sg.sh[k] = (uint8_t)tz;
        }
        sg.narrow = true;
        int64_t off[7];
        pe::agg_seg_layout(sg.nj, sg.ng, sg.nc, v1, off, ak, true);
        sg.bytes = off[6];
      };
      auto plan = [&](int t, int64_t pa, int64_t pb) {   // thread t's share of jobs [pa, pb)
        const int64_t ja = pa + (pb - pa) * t / T, jb = pa + (pb - pa) * (t + 1) / T;
        auto& out = segs[(size_t)t];
        out.clear();
        int64_t off[7];
        for (int64_t j = ja; j < jb;) {
          AggSeg sg{j, 0, 0, 0, 0, false, {}};
          while (j < jb && sg.nj < seg_jobs) {
            const int64_t g0 = job_group_off[j], g1 = job_group_off[j + 1];
            const int64_t nc = gco ? (int64_t)gco[g1] - gco[g0] : 0;
            pe::agg_seg_layout(sg.nj + 1, sg.ng + (g1 - g0), sg.nc + nc, v1, off, ak);
            if (sg.nj > 0 && off[6] > pe::AGG_SEG_BYTES) break;
            ++sg.nj;
            sg.ng += (int32_t)(g1 - g0);
            sg.nc += (int32_t)nc;
            sg.bytes = off[6];
            ++j;
          }
          narrow_seg(sg);
          out.push_back(sg);
        }
      };
      auto& all = ctx->agg_all;   // every planned segment so far, in job order
      all.clear();
      // chunk c: plan jobs [n c / CH, n (c + 1) / CH), its segments appended to all and their offsets to so
      int64_t* so = nullptr;
      auto plan_chunk = [&](int64_t c) {   // (c = -1: every job, in one pass)
        const int64_t pa = c < 0 ? 0 : n_jobs * c / CH, pb = c < 0 ? n_jobs : n_jobs * (c + 1) / CH;
        if (T == 1) plan(0, pa, pb);
        else PlanPool::get().run(T, [&](int t) { plan(t, pa, pb); });
        const size_t k0 = all.size();
        for (int t = 0; t < T; ++t) all.insert(all.end(), segs[t].begin(), segs[t].end());
        if (so)
          for (size_t k = k0; k < all.size(); ++k) so[k + 1] = so[k] + all[k].bytes;
      };
      // Pinned staging sized before the first chunk is planned (a chunked call writes chunk 0 before the
      // rest is planned): raw section bytes plus at most 8 + 5 x 15 B of padding and a header per
      // segment; a segment ends at seg_jobs jobs, at a chunk or thread boundary, or where it and the
      // next job would pass AGG_SEG_BYTES -- each job's bytes are in at most two such sums.
      const int64_t raw = n_jobs * 8 + G * 8 + C * (8 * ND + ak.fb);
      const int64_t seg_cap = n_jobs / seg_jobs + 2 * raw / (pe::AGG_SEG_BYTES - 128) + CH * T + 2;
      const int64_t seg_over = (int64_t)sizeof(pe::AggSegHdr) + 8 + 5 * 15;
      int64_t nseg = 0, total = 0;
      if (CH == 1 || one_plan) {
        plan_chunk(-1);
        nseg = (int64_t)all.size();
        ensure_pinned(ctx->a_segoff, (size_t)nseg + 1, "alloc pinned segment offsets");
        so = ctx->a_segoff.p;
        so[0] = 0;
        for (int64_t k = 0; k < nseg; ++k) so[k + 1] = so[k] + all[(size_t)k].bytes;
        total = so[nseg];
      } else {
        ensure_pinned(ctx->a_segoff, (size_t)seg_cap + 1, "alloc pinned segment offsets");
        so = ctx->a_segoff.p;
        so[0] = 0;
        total = raw + seg_cap * seg_over;   // (an upper bound: the staging capacity)
      }
      int64_t oo[4];
      pe::agg_out_layout(n_jobs, oo, ak);
      const int64_t out_bytes = oo[3] + pe::agg_r16(n_jobs);
      ensure_pinned(ctx->a_stage, (size_t)total, "alloc pinned aggregation batch");
      ensure_pinned(ctx->a_outh, (size_t)out_bytes, "alloc pinned aggregation outputs");
      if (!ctx->a_flag.p) {
        hipchk(ctx->a_flag.ensure(16, kZeroCopy), "alloc pinned flag");
        // pinned memory may come back recycled (e.g. the flag of an engine destroyed earlier): clear
        // it, and start the generations past whatever it held, so no stale value matches a wait
        __atomic_store_n(ctx->a_flag.p, 0u, __ATOMIC_RELEASE);
        ctx->agg_gen = 0;
      }
      if (!ctx->a_ctr.p) {
        hipchk(ctx->a_ctr.ensure(1), "alloc done counter");
        hipchk(hipMemsetAsync(ctx->a_ctr.p, 0, 4, ctx->stream), "memset done counter");
      }
      const auto tt1 = now();
      // 2. pack (and the negative-request check, on the copied values); 3. launch
      int64_t bad[PlanPool::kMax];
      std::fill(bad, bad + PlanPool::kMax, INT64_MAX);
      // non-temporal stores for the request records of large calls (PE_AGG_NO_NT=1: plain stores, A/B)
      static const bool nt_env = std::getenv("PE_AGG_NO_NT") == nullptr;
      const bool nt = nt_env && n_jobs > kLatJobs;
      auto pack = [&](int64_t s0, int64_t s1, int64_t& badv) {
        struct Fence {   // the streamed lines are globally visible before the pack returns (the DMA reads them)
          bool on;
          ~Fence() {
            if (on) _mm_sfence();
          }
        } fence{nt};
        for (int64_t k = s0; k < s1; ++k) {
          const AggSeg& sg = all[(size_t)k];
          uint8_t* b = ctx->a_stage.p + so[k];
          pe::AggSegHdr h{};
          h.j0 = sg.j0;
          h.nj = sg.nj;
          h.ng = sg.ng;
          h.nc = sg.nc;
          const int32_t g0 = job_group_off[sg.j0];
          h.g0 = g0;
          h.c0 = sg.ng > 0 ? gco[g0] : 0;
          h.narrow = sg.narrow ? 1 : 0;
          std::memcpy(b, &h, sizeof(h));
          int64_t off[7];
          pe::agg_seg_layout(sg.nj, sg.ng, sg.nc, v1, off, ak, sg.narrow);
          // offsets copied as they are (the kernel rebases by h.g0 / h.c0): every section is a memcpy
          auto copy = [nt](void* d, const void* src, size_t bytes) {
            if (nt) nt_copy(d, src, bytes);
            else std::memcpy(d, src, bytes);
          };
          copy(b + off[0], job_group_off + sg.j0, (size_t)(sg.nj + 1) * 4);
          if (v1) copy(b + off[1], min_member + sg.j0, (size_t)sg.nj * 4);
          if (sg.ng > 0) {
            copy(b + off[2], group_replicas + g0, (size_t)sg.ng * 4);
            const int32_t c0 = h.c0;
            copy(b + off[3], gco + g0, (size_t)(sg.ng + 1) * 4);
            if (sg.nc > 0) {
              const int64_t* q = cont_req + (int64_t)c0 * n_keys;
              const int64_t nq = (int64_t)sg.nc * n_keys;
              int64_t any;
              if (sg.narrow) {   // (no negative value: narrow_seg checked)
                std::memcpy(b + off[4], sg.sh, 16);
                uint32_t* d = reinterpret_cast<uint32_t*>(b + off[4] + 16);
                if (n_keys == 4 && ND == 4) {
                  if (nt) narrow_rows4<true>(d, q, sg.nc, sg.sh);
                  else narrow_rows4<false>(d, q, sg.nc, sg.sh);
                } else {
                  for (int32_t c = 0; c < sg.nc; ++c) {
                    for (int k = 0; k < n_keys; ++k)
                      d[(int64_t)c * ND + k] = (uint32_t)((uint64_t)q[(int64_t)c * n_keys + k] >> sg.sh[k]);
                    for (int k = n_keys; k < ND; ++k) d[(int64_t)c * ND + k] = 0;
                  }
                }
                any = 0;
              } else if (n_keys == ND) {
                any = nt ? copy_or_i64<true>(reinterpret_cast<int64_t*>(b + off[4]), q, nq)   // one pass
                         : copy_or_i64<false>(reinterpret_cast<int64_t*>(b + off[4]), q, nq);
              } else {   // a key table narrower than its kernel: rows padded with zeros (never present)
                int64_t* d = reinterpret_cast<int64_t*>(b + off[4]);
                int64_t acc = 0;
                for (int32_t c = 0; c < sg.nc; ++c) {
                  for (int k = 0; k < n_keys; ++k) acc |= d[(int64_t)c * ND + k] = q[(int64_t)c * n_keys + k];
                  for (int k = n_keys; k < ND; ++k) d[(int64_t)c * ND + k] = 0;
                }
                any = acc;
              }
              copy(b + off[5], cont_flags + (int64_t)c0 * ak.fb, (size_t)sg.nc * ak.fb);
              if (any < 0 && badv == INT64_MAX)
                for (int64_t i = 0; i < nq; ++i)
                  if (q[i] < 0) {
                    badv = (int64_t)c0 * n_keys + i;
                    break;
                  }
            }
          } else {
            reinterpret_cast<int32_t*>(b + off[3])[0] = 0;   // (h.c0 = 0)
          }
        }
      };
      uint8_t* const od = ctx->a_outh.dev;
      const uint8_t* oh = ctx->a_outh.p;
      auto unpack = [&](int64_t a, int64_t e) {   // outputs of jobs [a, e) into the caller's arrays
        if (n_keys == ND) {
          std::memcpy(out_min_res + a * n_keys, oh + oo[0] + a * 8 * ND, (size_t)(e - a) * 8 * ND);
        } else {
          const int64_t* src = reinterpret_cast<const int64_t*>(oh + oo[0]);
          for (int64_t j = a; j < e; ++j) std::memcpy(out_min_res + j * n_keys, src + j * ND, (size_t)n_keys * 8);
        }
        std::memcpy(out_members + a, oh + oo[1] + a * 4, (size_t)(e - a) * 4);
        std::memcpy(out_present + a * pb, oh + oo[2] + a * pb, (size_t)(e - a) * pb);
        std::memcpy(out_overflow + a, oh + oo[3] + a, (size_t)(e - a));
      };
      int64_t unpacked = 0;   // jobs [0, unpacked) already copied out
      int64_t first_neg = INT64_MAX;
      double t_launch = 0, t_wait = 0;
      if (n_jobs <= kLatJobs) {   // latency path: one launch, the host waits on the flag
        const auto tp = now();
        pack(0, nseg, bad[0]);
        first_neg = bad[0];
        t_pack = std::chrono::duration<double, std::milli>(now() - tp).count();
        if (first_neg == INT64_MAX) {
          if (++ctx->agg_gen == 0) ++ctx->agg_gen;
          const auto tl = now();
          if (nseg == 1 && total <= pe::AGG_KARG_BYTES && !std::getenv("PE_AGG_NO_KARG")) {
            // the segment in the kernel arguments (no zero-copy read; PE_AGG_NO_KARG=1: A/B)
            static thread_local pe::AggKarg karg;   // (512 B)
            std::memcpy(karg.b, ctx->a_stage.p, (size_t)total);
            hipchk(pe::launch_pg_agg_karg(ctx->stream, mode, karg, total, od, n_jobs, ctx->a_flag.dev, ctx->agg_gen, ak),
                   "launch pg_agg_karg");
          } else {
            hipchk(pe::launch_pg_agg_segments(ctx->stream, mode, ctx->a_stage.dev,
                                              nseg == 1 ? nullptr : ctx->a_segoff.dev, nseg, total, od, n_jobs,
                                              ctx->a_flag.dev, ctx->agg_gen, ctx->a_ctr.p, ak),
                   "launch pg_agg_segments");
          }
          const auto tw = now();
          agg_wait_flag(ctx, ctx->agg_gen);
          t_launch = std::chrono::duration<double, std::milli>(tw - tl).count();
          t_wait = std::chrono::duration<double, std::milli>(now() - tw).count();
        }
      } else {
        // chunks of segments, each planned and packed by the planning pool and launched at once: chunk
        // k's segments cross PCIe while the host plans and packs chunk k + 1, and chunk k - 1's outputs
        // are copied out once its kernel is done (an event per chunk).  The input crosses as one DMA per
        // chunk (a copy engine on its own stream, pinned -> device; the chunk's kernel waits on its event
        // and reads the segments from HBM): the copy engine streams the link at its rate, where the
        // kernels' own zero-copy reads reached ~2/3 of it beside their output writes (round 5: 3.35 ms
        // of kernel for a 2.2 ms input stream).  Outputs stay zero-copy writes into pinned memory: the
        // link's other direction.  PE_AGG_ZEROCOPY=1: the kernels read the pinned batch directly (A/B).
        const bool dma = !std::getenv("PE_AGG_ZEROCOPY");
        while ((int64_t)ctx->a_ev.size() < CH) {
          hipEvent_t e;
          hipchk(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
          ctx->a_ev.push_back(e);
        }
        if (dma) {
          hipchk(ctx->a_dstage.ensure((size_t)total), "alloc device aggregation batch");
          if (!ctx->a_h2d) hipchk(hipStreamCreateWithFlags(&ctx->a_h2d, hipStreamNonBlocking), "stream");
          while ((int64_t)ctx->a_ev_h2d.size() < CH) {
            hipEvent_t e;
            hipchk(hipEventCreateWithFlags(&e, hipEventDisableTiming), "event");
            ctx->a_ev_h2d.push_back(e);
          }
        }
        const uint8_t* const blob = dma ? ctx->a_dstage.p : ctx->a_stage.dev;
        int64_t prev_s0 = -1, prev_s1 = -1, prev_c = -1;   // prev_c: event of the last launched chunk
        auto job_end = [&](int64_t s1) { return all[(size_t)s1 - 1].j0 + all[(size_t)s1 - 1].nj; };
        for (int64_t c = 0; c < CH && first_neg == INT64_MAX; ++c) {
          const auto tp = now();
          const bool planned = CH == 1 || one_plan;   // (every chunk planned above)
          const int64_t s0 = planned ? nseg * c / CH : (int64_t)all.size();
          if (!planned) plan_chunk(c);
          const int64_t s1 = planned ? nseg * (c + 1) / CH : (int64_t)all.size();
          if (!planned && (s1 > seg_cap || so[s1] > total))   // (the bounds above hold by construction)
            raise(PE_ENOMEM, "aggregation staging bound exceeded");
          if (s1 == s0) continue;
          if (T == 1) pack(s0, s1, bad[0]);
          else PlanPool::get().run(T, [&](int t) { pack(s0 + (s1 - s0) * t / T, s0 + (s1 - s0) * (t + 1) / T, bad[t]); });
          t_pack += std::chrono::duration<double, std::milli>(now() - tp).count();
          first_neg = *std::min_element(bad, bad + T);
          if (first_neg != INT64_MAX) break;
          if (dma) {   // the chunk's bytes at the same offsets in the device copy (seg_off stays valid)
            hipchk(hipMemcpyAsync(ctx->a_dstage.p + so[s0], ctx->a_stage.p + so[s0], (size_t)(so[s1] - so[s0]),
                                  hipMemcpyHostToDevice, ctx->a_h2d),
                   "H2D aggregation chunk");
            hipchk(hipEventRecord(ctx->a_ev_h2d[(size_t)c], ctx->a_h2d), "event record");
            hipchk(hipStreamWaitEvent(ctx->stream, ctx->a_ev_h2d[(size_t)c], 0), "stream wait");
          }
          hipchk(pe::launch_pg_agg_segments(ctx->stream, mode, blob, ctx->a_segoff.dev + s0, s1 - s0, 0, od,
                                            n_jobs, nullptr, 0, nullptr, ak),
                 "launch pg_agg_segments");
          hipchk(hipEventRecord(ctx->a_ev[(size_t)c], ctx->stream), "event record");
          if (prev_s1 > prev_s0) {   // the previous chunk's outputs, while this chunk runs
            hipchk(hipEventSynchronize(ctx->a_ev[(size_t)prev_c]), "event sync");
            const int64_t ja = all[(size_t)prev_s0].j0, jb = job_end(prev_s1);
            parallel_for(jb - ja, [&](int64_t a, int64_t e) { unpack(ja + a, ja + e); });
            unpacked = jb;
          }
          prev_s0 = s0;
          prev_s1 = s1;
          prev_c = c;
        }
        nseg = (int64_t)all.size();
        hipchk(hipStreamSynchronize(ctx->stream), "sync pg_agg_segments");
        ctx->stats.agg_segments += nseg;
        ctx->stats.agg_wire_bytes += nseg > 0 ? so[nseg] : 0;
        for (int64_t k = 0; k < nseg; ++k) ctx->stats.agg_narrow_segments += all[(size_t)k].narrow ? 1 : 0;   // (also before an EINVAL:
                                                                             // launched chunks read the batch)
      }
      if (first_neg != INT64_MAX) raise(PE_EINVAL, "cont_req: negative request at index " + std::to_string(first_neg));
      const auto tt2 = now();
      if (T == 1) unpack(unpacked, n_jobs);
      else parallel_for(n_jobs - unpacked, [&](int64_t a, int64_t e) { unpack(unpacked + a, unpacked + e); });
      if (trace) {
        const auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
          return std::chrono::duration<double, std::milli>(b - a).count();
        };
        std::fprintf(stderr, "agg: J %lld segs %lld bytes %lld | plan %.4f ms, pack %.4f ms, pack+launch+wait %.4f ms "
                             "(launch call %.4f, flag wait %.4f), unpack %.4f ms\n",
                     (long long)n_jobs, (long long)nseg, (long long)total, ms(tt0, tt1), t_pack, ms(tt1, tt2), t_launch,
                     t_wait, ms(tt2, now()));
      }
    }
    const void* o1 = std::memchr(out_overflow, 1, (size_t)n_jobs);
    if (o1) {
      ctx->err = "int64 overflow in job " + std::to_string(static_cast<const uint8_t*>(o1) - out_overflow);
      return PE_EOVERFLOW;
    }
    return PE_OK;
  }
}

int agg_call(pe_ctx* ctx, int32_t mode, int64_t n_jobs, pe::AggKeys ak, int n_keys, const int32_t* job_group_off,
             const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
             const int64_t* cont_req, const void* cont_flags_v, int64_t* out_min_res, void* out_present_v,
             int32_t* out_members, uint8_t* out_overflow) {
  return guarded(ctx, [&]() -> int {
    return agg_call_locked(ctx, mode, n_jobs, ak, n_keys, job_group_off, min_member, group_replicas, group_cont_off,
                           cont_req, cont_flags_v, out_min_res, out_present_v, out_members, out_overflow);
  });
}

// pe_pg_min_resources_wide, the 128-bit pass: gather jobs `jobs` (ascending) of the caller's batch into a
// compact CSR sub-batch with rebased offsets and both limbs, upload it, run pg_agg_wide_kernel (one
// lane per (job, key) pair) and scatter the results into the caller's arrays.  Every sum happens on the
// device; the host only moves records.  out_overflow[j] becomes 1, or 2 where a pair of the job left
// [-2^127, 2^127) (the job's values are then 0).  Returns whether some job is 2.
bool agg_wide_pass(pe_ctx* ctx, int32_t mode, int n_keys, const int32_t* job_group_off, const int32_t* min_member,
                   const int32_t* group_replicas, const int32_t* group_cont_off, const uint64_t* lo,
                   const uint64_t* hi, const uint32_t* cont_flags, const std::vector<int64_t>& jobs, uint64_t* out_lo,
                   int64_t* out_hi, uint8_t* out_overflow) {
  const int64_t nw = (int64_t)jobs.size();
  const bool v1 = mode == PE_MODE_V1;
  int64_t G = 0, C = 0;
  for (const int64_t j : jobs) {
    const int32_t g0 = job_group_off[j], g1 = job_group_off[j + 1];
    G += g1 - g0;
    if (g1 > g0) C += group_cont_off[g1] - group_cont_off[g0];
  }
  // sections (16-B aligned): inputs jgo, min_member, replicas, gco, lo, hi, flags; outputs lo, hi, flags
  int64_t off[11];
  off[0] = 0;
  off[1] = off[0] + pe::agg_r16((nw + 1) * 4);
  off[2] = off[1] + (v1 ? pe::agg_r16(nw * 4) : 0);
  off[3] = off[2] + pe::agg_r16(G * 4);
  off[4] = off[3] + pe::agg_r16((G + 1) * 4);
  off[5] = off[4] + pe::agg_r16(C * n_keys * 8);
  off[6] = off[5] + (hi ? pe::agg_r16(C * n_keys * 8) : 0);
  off[7] = off[6] + pe::agg_r16(C * 4);            // end of the inputs
  off[8] = off[7] + pe::agg_r16(nw * n_keys * 8);
  off[9] = off[8] + pe::agg_r16(nw * n_keys * 8);
  off[10] = off[9] + pe::agg_r16(nw * n_keys);
  const int64_t in_bytes = off[7], out_bytes = off[10] - off[7];
  ensure_pinned(ctx->aw_stage, (size_t)in_bytes, "alloc pinned wide batch");
  ensure_pinned(ctx->aw_outh, (size_t)out_bytes, "alloc pinned wide outputs");
  if ((size_t)off[10] > ctx->aw_dev.n)
    hipchk(ctx->aw_dev.ensure(std::max((size_t)off[10], ctx->aw_dev.n + ctx->aw_dev.n / 2)), "alloc device wide batch");
  uint8_t* b = ctx->aw_stage.p;
  int32_t* s_jgo = reinterpret_cast<int32_t*>(b + off[0]);
  int32_t* s_mm = reinterpret_cast<int32_t*>(b + off[1]);
  int32_t* s_rep = reinterpret_cast<int32_t*>(b + off[2]);
  int32_t* s_gco = reinterpret_cast<int32_t*>(b + off[3]);
  uint64_t* s_lo = reinterpret_cast<uint64_t*>(b + off[4]);
  uint64_t* s_hi = reinterpret_cast<uint64_t*>(b + off[5]);
  uint32_t* s_fl = reinterpret_cast<uint32_t*>(b + off[6]);
  int64_t g = 0, c = 0;
  s_jgo[0] = 0;
  s_gco[0] = 0;
  for (int64_t w = 0; w < nw; ++w) {
    const int64_t j = jobs[(size_t)w];
    const int32_t g0 = job_group_off[j], g1 = job_group_off[j + 1];
    if (v1) s_mm[w] = min_member[j];
    if (g1 > g0) {
      const int32_t c0 = group_cont_off[g0], c1 = group_cont_off[g1];
      std::memcpy(s_rep + g, group_replicas + g0, (size_t)(g1 - g0) * 4);
      for (int32_t q = g0; q < g1; ++q) s_gco[g + (q - g0) + 1] = (int32_t)(c + (group_cont_off[q + 1] - c0));
      if (c1 > c0) {
        std::memcpy(s_lo + c * n_keys, lo + (int64_t)c0 * n_keys, (size_t)(c1 - c0) * n_keys * 8);
        if (hi) std::memcpy(s_hi + c * n_keys, hi + (int64_t)c0 * n_keys, (size_t)(c1 - c0) * n_keys * 8);
        std::memcpy(s_fl + c, cont_flags + c0, (size_t)(c1 - c0) * 4);
      }
      g += g1 - g0;
      c += c1 - c0;
    }
    s_jgo[w + 1] = (int32_t)g;
  }
  uint8_t* d = ctx->aw_dev.p;
  hipchk(hipMemcpyAsync(d, b, (size_t)in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D wide batch");
  hipchk(pe::launch_pg_agg_wide(ctx->stream, mode, nw, n_keys, reinterpret_cast<const int32_t*>(d + off[0]),
                                v1 ? reinterpret_cast<const int32_t*>(d + off[1]) : nullptr,
                                reinterpret_cast<const int32_t*>(d + off[2]),
                                reinterpret_cast<const int32_t*>(d + off[3]),
                                reinterpret_cast<const uint64_t*>(d + off[4]),
                                hi ? reinterpret_cast<const uint64_t*>(d + off[5]) : nullptr,
                                reinterpret_cast<const uint32_t*>(d + off[6]), reinterpret_cast<uint64_t*>(d + off[7]),
                                reinterpret_cast<int64_t*>(d + off[8]), d + off[9]),
         "launch pg_agg_wide");
  hipchk(hipMemcpyAsync(ctx->aw_outh.p, d + off[7], (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream),
         "D2H wide outputs");
  hipchk(hipStreamSynchronize(ctx->stream), "sync pg_agg_wide");
  ctx->stats.agg_wide_jobs += nw;
  const uint64_t* r_lo = reinterpret_cast<const uint64_t*>(ctx->aw_outh.p);
  const int64_t* r_hi = reinterpret_cast<const int64_t*>(ctx->aw_outh.p + (off[8] - off[7]));
  const uint8_t* r_fl = ctx->aw_outh.p + (off[9] - off[7]);
  bool any2 = false;
  for (int64_t w = 0; w < nw; ++w) {
    const int64_t j = jobs[(size_t)w];
    const bool left = std::memchr(r_fl + w * n_keys, 1, (size_t)n_keys) != nullptr;
    if (left) {
      std::memset(out_lo + j * n_keys, 0, (size_t)n_keys * 8);
      std::memset(out_hi + j * n_keys, 0, (size_t)n_keys * 8);
    } else {
      std::memcpy(out_lo + j * n_keys, r_lo + w * n_keys, (size_t)n_keys * 8);
      std::memcpy(out_hi + j * n_keys, r_hi + w * n_keys, (size_t)n_keys * 8);
    }
    out_overflow[j] = left ? 2 : 1;
    any2 |= left;
  }
  return any2;
}

}  // namespace

extern "C" {

int pe_pg_min_resources(pe_ctx* ctx, int32_t mode, int64_t n_jobs, const int32_t* job_group_off,
                        const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                        const int64_t* cont_req, const uint8_t* cont_flags, int64_t* out_min_res,
                        uint8_t* out_present, int32_t* out_members, uint8_t* out_overflow) {
  return agg_call(ctx, mode, n_jobs, pe::AggKeys{4, 1}, 4, job_group_off, min_member, group_replicas, group_cont_off,
                  cont_req, cont_flags, out_min_res, out_present, out_members, out_overflow);
}

int pe_pg_min_resources_keys(pe_ctx* ctx, int32_t mode, int64_t n_jobs, int32_t n_keys, const int32_t* job_group_off,
                             const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                             const int64_t* cont_req, const uint32_t* cont_flags, int64_t* out_min_res,
                             uint16_t* out_present, int32_t* out_members, uint8_t* out_overflow) {
  if (n_keys < 1 || n_keys > PE_MAX_KEYS) {
    if (ctx) ctx->err = "n_keys must be in [1, " + std::to_string(PE_MAX_KEYS) + "]";
    return PE_EINVAL;
  }
  const pe::AggKeys ak{n_keys <= 4 ? 4 : n_keys <= 8 ? 8 : 16, 4};
  return agg_call(ctx, mode, n_jobs, ak, n_keys, job_group_off, min_member, group_replicas, group_cont_off, cont_req,
                  cont_flags, out_min_res, out_present, out_members, out_overflow);
}

// The int64 pass of pe_pg_min_resources_keys over the whole batch, then the 128-bit pass over the jobs
// it flagged plus the jobs holding an input wider than int64 (agg_wide_pass).  Without such a job the
// call is the keys call, the sign extension into out_hi and a memchr.
int pe_pg_min_resources_wide(pe_ctx* ctx, int32_t mode, int64_t n_jobs, int32_t n_keys, const int32_t* job_group_off,
                             const int32_t* min_member, const int32_t* group_replicas, const int32_t* group_cont_off,
                             const uint64_t* cont_req_lo, const uint64_t* cont_req_hi, const uint32_t* cont_flags,
                             uint64_t* out_lo, int64_t* out_hi, uint16_t* out_present, int32_t* out_members,
                             uint8_t* out_overflow) {
  if (n_keys < 1 || n_keys > PE_MAX_KEYS) {
    if (ctx) ctx->err = "n_keys must be in [1, " + std::to_string(PE_MAX_KEYS) + "]";
    return PE_EINVAL;
  }
  const pe::AggKeys ak{n_keys <= 4 ? 4 : n_keys <= 8 ? 8 : 16, 4};
  return guarded(ctx, [&]() -> int {
    const int64_t* narrow_req = reinterpret_cast<const int64_t*>(cont_req_lo);
    bool wide_in = false;
    if (cont_req_hi && n_jobs > 0) {
      // the wide-input scan walks the offsets: the checks agg_call_locked makes on them come first
      if (mode != PE_MODE_V1 && mode != PE_MODE_V2) raise(PE_EINVAL, "mode must be PE_MODE_V1 or PE_MODE_V2");
      need_ptr(job_group_off, "job_group_off");
      check_offsets(job_group_off, n_jobs, -1, "job_group_off");
      const int64_t G = job_group_off[n_jobs];
      if (G > 0) {
        need_ptr(group_cont_off, "group_cont_off");
        check_offsets(group_cont_off, G, -1, "group_cont_off");
      }
      const int64_t C = G > 0 ? group_cont_off[G] : 0;
      if (C > 0) need_ptr(cont_req_lo, "cont_req_lo");
      auto& mark = ctx->aw_mark;
      mark.assign((size_t)n_jobs, 0);
      for (int64_t j = 0; j < n_jobs && C > 0; ++j) {
        const int64_t i0 = (int64_t)group_cont_off[job_group_off[j]] * n_keys;
        const int64_t i1 = (int64_t)group_cont_off[job_group_off[j + 1]] * n_keys;
        uint64_t any = 0, any_hi = 0;
        for (int64_t i = i0; i < i1; ++i) {
          any_hi |= cont_req_hi[i];
          any |= cont_req_hi[i] | (cont_req_lo[i] >> 63);
        }
        if (any_hi >> 63)
          for (int64_t i = i0; i < i1; ++i)
            if (cont_req_hi[i] >> 63)
              raise(PE_EINVAL, "cont_req_hi: request of 2^127 or more at index " + std::to_string(i));
        if (any) mark[(size_t)j] = 1, wide_in = true;
      }
      if (wide_in) {   // those jobs reach the int64 kernels as zeros; their int64 outputs are not used
        auto& cp = ctx->aw_lo;
        cp.resize((size_t)(C * n_keys));
        std::memcpy(cp.data(), cont_req_lo, (size_t)(C * n_keys) * 8);
        for (int64_t j = 0; j < n_jobs; ++j)
          if (mark[(size_t)j]) {
            const int64_t i0 = (int64_t)group_cont_off[job_group_off[j]] * n_keys;
            const int64_t i1 = (int64_t)group_cont_off[job_group_off[j + 1]] * n_keys;
            std::memset(cp.data() + i0, 0, (size_t)(i1 - i0) * 8);
          }
        narrow_req = cp.data();
      }
    }
    if (n_jobs > 0) need_ptr(out_hi, "out_hi");
    const int rc = agg_call_locked(ctx, mode, n_jobs, ak, n_keys, job_group_off, min_member, group_replicas,
                                   group_cont_off, narrow_req, cont_flags, reinterpret_cast<int64_t*>(out_lo),
                                   out_present, out_members, out_overflow);
    if (n_jobs <= 0) return rc;
    const int64_t* olo = reinterpret_cast<const int64_t*>(out_lo);
    for (int64_t i = 0; i < n_jobs * n_keys; ++i) out_hi[i] = olo[i] >> 63;   // sign extension
    if (rc == PE_OK && !wide_in) return PE_OK;
    auto& jobs = ctx->aw_jobs;
    jobs.clear();
    for (int64_t j = 0; j < n_jobs; ++j)
      if (out_overflow[j] || (wide_in && ctx->aw_mark[(size_t)j])) jobs.push_back(j);
    ctx->err.clear();
    if (agg_wide_pass(ctx, mode, n_keys, job_group_off, min_member, group_replicas, group_cont_off, cont_req_lo,
                      cont_req_hi, cont_flags, jobs, out_lo, out_hi, out_overflow)) {
      const void* o2 = std::memchr(out_overflow, 2, (size_t)n_jobs);
      ctx->err = "128-bit overflow in job " + std::to_string(static_cast<const uint8_t*>(o2) - out_overflow);
      return PE_EOVERFLOW;
    }
    return PE_OK;
  });
}

// ------------------------------------------------------------------ fit mask

// The batch's dictionary, built once per upload and shared by every fit path's planning: per field
// (dims 0-3, field 4 = label need) the distinct values ascending and each job's index into them.
// One hashing pass per field (first-seen ids), then only the distinct values are sorted -- O(J)
// for the usual few-valued batches instead of five O(J log J) sorts.
struct BatchDict {
  static constexpr int F = pe::D + 1;
  std::vector<int64_t> vals[F];
  std::vector<uint32_t> rank[F];
};

extern "C++" {   // (this part of the file sits in the ABI's extern "C" block)
template <class V>
static void dict_field(int64_t n, V value, std::vector<int64_t>& vals, std::vector<uint32_t>& rank) {
  size_t cap = 64;
  while (cap < 2 * (size_t)n) cap *= 2;
  std::vector<int64_t> keys(cap);
  std::vector<uint32_t> ids(cap, UINT32_MAX);
  const size_t mask = cap - 1;
  vals.clear();
  rank.resize((size_t)n);
  for (int64_t j = 0; j < n; ++j) {
    const int64_t v = value(j);
    size_t h = (size_t)(((uint64_t)v * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    while (ids[h] != UINT32_MAX && keys[h] != v) h = (h + 1) & mask;
    if (ids[h] == UINT32_MAX) {
      keys[h] = v;
      ids[h] = (uint32_t)vals.size();
      vals.push_back(v);
    }
    rank[j] = ids[h];
  }
  // order the distinct values: (value, first-seen id) pairs, LSD radix (11-bit digits, passes whose
  // digit is constant skipped) for many values, a comparison sort for few
  const size_t m = vals.size();
  std::vector<std::pair<uint64_t, uint32_t>> pr(m), tmp;
  for (size_t i = 0; i < m; ++i) pr[i] = {(uint64_t)vals[i] ^ (1ull << 63), (uint32_t)i};   // signed order
  if (m < 4096) {
    std::sort(pr.begin(), pr.end());
  } else {
    tmp.resize(m);
    uint64_t orv = 0, andv = ~0ull;
    for (const auto& e : pr) {
      orv |= e.first;
      andv &= e.first;
    }
    for (int sh = 0; sh < 64; sh += 11) {
      if ((((orv ^ andv) >> sh) & 0x7FF) == 0) continue;   // every value has the same digit here
      size_t cnt[2049] = {0};
      for (const auto& e : pr) ++cnt[((e.first >> sh) & 0x7FF) + 1];
      for (int b = 0; b < 2048; ++b) cnt[b + 1] += cnt[b];
      for (const auto& e : pr) tmp[cnt[(e.first >> sh) & 0x7FF]++] = e;
      pr.swap(tmp);
    }
  }
  std::vector<uint32_t> pos(m);
  for (size_t i = 0; i < m; ++i) {
    pos[pr[i].second] = (uint32_t)i;
    vals[i] = (int64_t)(pr[i].first ^ (1ull << 63));
  }
  for (int64_t j = 0; j < n; ++j) rank[j] = pos[rank[j]];
}
}  // extern "C++"

static void build_dict(BatchDict& bd, int64_t n_jobs, const int64_t* req, const uint32_t* need) {
  auto field = [&](int f) {
    if (f < pe::D)
      dict_field(n_jobs, [&](int64_t j) { return req[j * pe::D + f]; }, bd.vals[f], bd.rank[f]);
    else
      dict_field(n_jobs, [&](int64_t j) { return (int64_t)(need ? need[j] : 0u); }, bd.vals[f], bd.rank[f]);
  };
  if (n_jobs < 16384) {
    for (int f = 0; f < BatchDict::F; ++f) field(f);
    return;
  }
  // large batches: the five independent fields on five threads (the upload is on the batch's path)
  PlanPool::get().run(BatchDict::F, [&](int f) { field(f); });
}

// Dictionary codes of one batch (pe_kernels.h, CodeSpec): per dimension the sorted distinct request
// values, per job their ranks packed with guard bits; label needs must form an inclusion chain.
// Returns false when the batch does not fit the 32-bit code word (the compare paths take it).
static bool build_codes(pe_ctx* ctx, int64_t n_jobs, const BatchDict& bd) {
  if (n_jobs == 0) return false;
  const std::vector<int64_t>* vals = bd.vals;
  for (int d = 0; d < pe::D; ++d)
    if ((int)vals[d].size() >= pe::CODE_MAXV) return false;
  if ((int)bd.vals[4].size() >= pe::CODE_MAXV) return false;
  std::vector<uint32_t> needs;
  for (int64_t v : bd.vals[4]) needs.push_back((uint32_t)v);
  std::sort(needs.begin(), needs.end(), [](uint32_t a, uint32_t b) {
    return __builtin_popcount(a) != __builtin_popcount(b) ? __builtin_popcount(a) < __builtin_popcount(b) : a < b;
  });
  // need dictionary index -> position in the inclusion chain
  std::vector<uint32_t> need_pos(bd.vals[4].size());
  for (size_t i = 0; i < bd.vals[4].size(); ++i)
    need_pos[i] = (uint32_t)(std::find(needs.begin(), needs.end(), (uint32_t)bd.vals[4][i]) - needs.begin());
  if ((int)needs.size() >= pe::CODE_MAXV) return false;
  for (size_t i = 0; i + 1 < needs.size(); ++i)
    if ((needs[i] & needs[i + 1]) != needs[i]) return false;   // not a chain under inclusion
  pe::CodeSpec sp{};
  int therm_bits = 0;
  for (int f = 0; f < pe::CODE_FIELDS; ++f) therm_bits += f < pe::D ? (int)vals[f].size() : (int)needs.size();
  // thermometer fields (one bit per distinct value) when they fit 31 bits -- bit 31 stays free for
  // the never-fitting padding jobs -- else log-width SWAR fields with guard bits
  sp.therm = (ctx->fit_path_mask & PATH_NO_THERM) == 0 && therm_bits <= 31 ? 1 : 0;
  int off = 0;
  for (int f = 0; f < pe::CODE_FIELDS; ++f) {
    const int k = f < pe::D ? (int)vals[f].size() : (int)needs.size();
    const int bits = 32 - __builtin_clz((unsigned)k);
    sp.nvals[f] = k;
    sp.width[f] = sp.therm ? k : bits + 1;
    sp.off[f] = off;
    off += sp.width[f];
  }
  if (off > 32) return false;
  sp.guard = 0;
  if (!sp.therm)
    for (int f = 0; f < pe::CODE_FIELDS; ++f) sp.guard |= 1u << (sp.off[f] + sp.width[f] - 1);
  const int64_t Jp = round_up(n_jobs, pe::FC_JT);
  // padding jobs never fit: SWAR code M (every field fails); thermometer ~Y with bit 31 cleared
  std::vector<uint32_t> jc((size_t)Jp, sp.therm ? ~(1u << 31) : sp.guard);
  for (int64_t j = 0; j < n_jobs; ++j) {
    uint32_t c = 0;
    for (int d = 0; d < pe::D; ++d) c |= (bd.rank[d][j] + 1) << sp.off[d];
    c |= (need_pos[bd.rank[4][j]] + 1) << sp.off[4];
    if (sp.therm) {
      uint32_t y = 0;   // one bit per field: rank c <=> bit c-1
      for (int f = 0; f < pe::CODE_FIELDS; ++f) {
        const uint32_t r = (c >> sp.off[f]) & ((1u << sp.width[f]) - 1);   // ranks < 2^width here
        y |= 1u << (sp.off[f] + r - 1);
      }
      c = ~y;
    }
    jc[j] = c;
  }
  std::vector<int64_t> vt((size_t)pe::D * pe::CODE_MAXV, INT64_MAX);
  for (int d = 0; d < pe::D; ++d) std::copy(vals[d].begin(), vals[d].end(), vt.begin() + (size_t)d * pe::CODE_MAXV);
  std::vector<uint32_t> nt((size_t)pe::CODE_MAXV, 0xFFFFFFFFu);
  std::copy(needs.begin(), needs.end(), nt.begin());
  ctx->code = sp;
  ctx->code_Jp = Jp;
  ctx->node_stride = round_up(std::max<int64_t>(ctx->Ns, 1), 64 * pe::FC_CH);
  hipchk(ctx->code_vals.ensure(vt.size()), "alloc code vals");
  hipchk(ctx->code_needs.ensure(nt.size()), "alloc code needs");
  hipchk(ctx->code_jobs.ensure(jc.size()), "alloc code jobs");
  hipchk(ctx->code_x.ensure((size_t)ctx->node_stride), "alloc code x");
  hipchk(hipMemcpyAsync(ctx->code_vals.p, vt.data(), vt.size() * 8, hipMemcpyHostToDevice, ctx->stream), "H2D vals");
  hipchk(hipMemcpyAsync(ctx->code_needs.p, nt.data(), nt.size() * 4, hipMemcpyHostToDevice, ctx->stream), "H2D needs");
  hipchk(hipMemcpyAsync(ctx->code_jobs.p, jc.data(), jc.size() * 4, hipMemcpyHostToDevice, ctx->stream), "H2D codes");
  return true;
}

// Bit planes of one batch (pe_kernels.h, PlaneSpec): one plane per distinct request value of each
// dimension and per distinct label need, each job selecting five.  Any int64 values and any need
// sets.  A batch with more than PL_MAX distinct (dimension, value) pairs is split into plane sets
// (row-major layout only, at most PL_MAX_SETS); returns false when it cannot be held either way.
constexpr int PL_MAX_SETS = 256;
constexpr int64_t PL_SETS_BYTES = int64_t(2) << 30;   // planes of all sets (4 MiB per set at 1M nodes)

static bool build_planes(pe_ctx* ctx, int64_t n_jobs, const BatchDict& bd, bool allow_sets) {
  if (n_jobs == 0) return false;
  constexpr int F = pe::D + 1;
  const std::vector<int64_t>* vals = bd.vals;
  int64_t off[F], P = 0;
  for (int f = 0; f < F; ++f) {
    off[f] = P;
    P += (int64_t)vals[f].size();
  }
  if (P > pe::PL_MAX && !allow_sets) return false;
  // pair id (global over the fields) of each job's five selections (the plane-set path)
  std::vector<int32_t> pid;
  if (P > pe::PL_MAX) {
    pid.resize((size_t)n_jobs * F);
    parallel_for(n_jobs, [&](int64_t j0, int64_t j1) {
      for (int64_t j = j0; j < j1; ++j)
        for (int f = 0; f < F; ++f) pid[(size_t)j * F + f] = (int32_t)(off[f] + bd.rank[f][j]);
    });
  }
  auto pair_spec = [&](int64_t p, int& kind, int64_t& val) {
    int f = F - 1;
    while (off[f] > p) --f;
    kind = f;
    val = vals[f][(size_t)(p - off[f])];
  };
  // field f's plane index sits at bits 0/7/14/21 (dims) and 32 (need) as 4 x index (register offset)
  auto field_shift = [](int f) { return f < pe::D ? 7 * f : 32; };
  ctx->pl_nblk = (std::max<int64_t>(ctx->Ns, 1) + pe::PL_BLK - 1) / pe::PL_BLK;
  // row-major mask pitch in blocks (PE_ROW_PITCH_BLOCKS: a study knob; the words past nblk are
  // never written)
  static const int64_t pitch_env = std::getenv("PE_ROW_PITCH_BLOCKS") ? std::atoll(std::getenv("PE_ROW_PITCH_BLOCKS")) : 0;
  ctx->pl_pitch = std::max(ctx->pl_nblk, pitch_env);
  // phases of a set of J jobs: one wave per SIMD (1024 on 256 CUs) = nblk x R; codes phase-major.
  // (Padding the row to 1024 / R blocks, i.e. an aligned 1 MiB store window, was measured no
  // faster: profiles/r5c_row_pitch.txt.)
  // PE_PL_WAVES / PE_PL_JPW (A/B studies): a fixed wave count, or R from a jobs-per-wave target
  static const int64_t pl_waves = std::getenv("PE_PL_WAVES") ? std::max(1ll, std::atoll(std::getenv("PE_PL_WAVES"))) : 1024;
  static const int64_t pl_jpw = std::getenv("PE_PL_JPW") ? std::max(1ll, std::atoll(std::getenv("PE_PL_JPW"))) : 0;
  auto phases = [&](int64_t J, int64_t& R, int64_t& Jr) {
    R = ctx->pl_rows ? std::min<int64_t>(J, std::max<int64_t>(1, pl_waves / ctx->pl_nblk)) : 1;
    if (ctx->pl_rows && pl_jpw) R = std::min<int64_t>(J, std::max<int64_t>(R, (J + pl_jpw - 1) / pl_jpw));
    Jr = ctx->pl_rows ? ((J + R - 1) / R + 3) / 4 * 4 : J;   // = the kernel's phase stride
  };
  std::vector<uint64_t> jc;
  ctx->pl_sets.clear();
  ctx->pl_cnt_row.clear();
  if (P <= pe::PL_MAX) {   // one set: every pair is a plane
    pe::PlaneSpec sp{};
    for (int64_t p = 0; p < P; ++p) {
      int kind;
      pair_spec(p, kind, sp.val[sp.n]);
      sp.kind[sp.n++] = kind;
    }
    ctx->plane = sp;
    hipchk(ctx->pl_specs_d.ensure(1), "alloc plane spec");
    hipchk(hipMemcpyAsync(ctx->pl_specs_d.p, &ctx->plane, sizeof(pe::PlaneSpec), hipMemcpyHostToDevice, ctx->stream),
           "H2D plane spec");
    int64_t R, Jr;
    phases(n_jobs, R, Jr);
    // each job's code straight into its phase-major slot (row-major kernel) or job order
    jc.assign((size_t)(ctx->pl_rows ? R * Jr : n_jobs), 0);
    parallel_for(n_jobs, [&](int64_t j0, int64_t j1) {
      for (int64_t j = j0; j < j1; ++j) {
        uint64_t c = 0;
        for (int f = 0; f < F; ++f) c |= (uint64_t)(4 * (off[f] + bd.rank[f][j])) << field_shift(f);
        jc[ctx->pl_rows ? (size_t)((j % R) * Jr + j / R) : (size_t)j] = c;
      }
    });
    ctx->pl_R = R;
    ctx->pl_counts_n = R * Jr;
  } else {
    if (!allow_sets || !ctx->pl_rows || n_jobs >= (int64_t(1) << 24)) return false;
    // Sets: jobs ordered by their selections, the field with the most distinct values first, then
    // swept greedily; a set closes when the next job would take it past PL_MAX planes.
    int ford[F];
    for (int f = 0; f < F; ++f) ford[f] = f;
    std::sort(ford, ford + F, [&](int x, int y) { return vals[x].size() > vals[y].size(); });
    std::vector<int64_t> order((size_t)n_jobs);
    for (int64_t j = 0; j < n_jobs; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
      for (int f : ford)
        if (pid[(size_t)x * F + f] != pid[(size_t)y * F + f]) return pid[(size_t)x * F + f] < pid[(size_t)y * F + f];
      return x < y;
    });
    std::vector<int32_t> stamp((size_t)P, -1), local((size_t)P, 0);
    std::vector<std::vector<int64_t>> members;
    std::vector<std::vector<uint64_t>> codes;
    std::vector<pe::PlaneSpec> specs;
    int cur = -1, ncur = 0;
    for (int64_t j : order) {
      int add = 0;
      for (int f = 0; f < F; ++f) add += cur < 0 || stamp[pid[(size_t)j * F + f]] != cur;
      if (cur < 0 || ncur + add > pe::PL_MAX) {
        if ((int)specs.size() == PL_MAX_SETS ||
            (int64_t)(specs.size() + 1) * ctx->pl_nblk * pe::PL_MAX * 64 * pe::PL_R * 4 > PL_SETS_BYTES)
          return false;
        ++cur;
        ncur = 0;
        members.emplace_back();
        codes.emplace_back();
        specs.push_back(pe::PlaneSpec{});
      }
      uint64_t c = (uint64_t)j << 40;   // the job's mask row
      for (int f = 0; f < F; ++f) {
        const int32_t p = pid[(size_t)j * F + f];
        if (stamp[p] != cur) {
          stamp[p] = cur;
          local[p] = ncur++;
          pe::PlaneSpec& sp = specs[cur];
          int kind;
          pair_spec(p, kind, sp.val[sp.n]);
          sp.kind[sp.n++] = kind;
        }
        c |= (uint64_t)(4 * local[p]) << field_shift(f);
      }
      members[cur].push_back(j);
      codes[cur].push_back(c);
    }
    // each set's jobs in row order: the sweep's stores in flight then stay in a narrow band of
    // rows (the partition order scattered them over the whole mask)
    for (size_t t = 0; t < members.size(); ++t) {
      std::vector<size_t> ix(members[t].size());
      for (size_t i = 0; i < ix.size(); ++i) ix[i] = i;
      std::sort(ix.begin(), ix.end(), [&](size_t x, size_t y) { return members[t][x] < members[t][y]; });
      std::vector<int64_t> m2(ix.size());
      std::vector<uint64_t> c2(ix.size());
      for (size_t i = 0; i < ix.size(); ++i) {
        m2[i] = members[t][ix[i]];
        c2[i] = codes[t][ix[i]];
      }
      members[t].swap(m2);
      codes[t].swap(c2);
    }
    // one launch sweeps every set: the phase count is common (one wave per SIMD over nblk blocks)
    const int64_t R = std::max<int64_t>(1, 1024 / ctx->pl_nblk);
    int64_t total = 0;
    std::vector<int64_t> meta;
    for (size_t t = 0; t < specs.size(); ++t) {
      pe_ctx::PlaneSet st{specs[t], (int64_t)members[t].size(), R, 0, total};
      st.Jr = ((st.J + R - 1) / R + 3) / 4 * 4;
      total += R * st.Jr;
      ctx->pl_sets.push_back(st);
      meta.insert(meta.end(), {st.off, st.J, st.Jr});
    }
    hipchk(ctx->pl_specs_d.ensure(specs.size()), "alloc plane specs");
    hipchk(ctx->pl_meta_d.ensure(meta.size()), "alloc plane set meta");
    hipchk(hipMemcpyAsync(ctx->pl_specs_d.p, specs.data(), specs.size() * sizeof(pe::PlaneSpec),
                          hipMemcpyHostToDevice, ctx->stream),
           "H2D plane specs");
    hipchk(hipMemcpyAsync(ctx->pl_meta_d.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, ctx->stream),
           "H2D plane set meta");
    hipchk(hipStreamSynchronize(ctx->stream), "sync plane sets");   // the host vectors die here
    jc.assign((size_t)total, 0);
    ctx->pl_cnt_row.assign((size_t)total, -1);
    for (size_t t = 0; t < specs.size(); ++t) {
      const pe_ctx::PlaneSet& st = ctx->pl_sets[t];
      for (int64_t i = 0; i < st.J; ++i) {
        const size_t k = (size_t)(st.off + (i % st.R) * st.Jr + i / st.R);
        jc[k] = codes[t][i];
        ctx->pl_cnt_row[k] = members[t][i];
      }
    }
    ctx->pl_R = 1;
    ctx->pl_counts_n = total;
  }
  hipchk(ctx->planes.ensure((size_t)std::max<size_t>(ctx->pl_sets.size(), 1) * ctx->pl_nblk * pe::PL_MAX * 64 *
                            pe::PL_R),
         "alloc planes");
  hipchk(ctx->plane_jobs.ensure(jc.size()), "alloc plane jobs");
  hipchk(hipMemcpyAsync(ctx->plane_jobs.p, jc.data(), jc.size() * 8, hipMemcpyHostToDevice, ctx->stream),
         "H2D plane jobs");
  return true;
}

// LDS digit planes of one batch (pe_kernels.h LdsSpec): per dimension with >= 2 distinct values a
// digit field of L levels (chosen with the node-block size W to minimise plane reads per job within
// the LDS budget), dimensions with one value folded into the need planes, one plane per distinct
// need -- or, with single-level fields crossed into them, one per (need, crossed values): a job then
// reads one plane for its labels and those fields.  Returns false when no configuration fits 160 KiB
// of LDS (the other paths take the batch).  PE_LDS_W=1|2|4 forces the block size, PE_LDS_MAXL=1..4
// caps the levels, PE_LDS_CROSS=0 crosses nothing (tuning / tests).
static bool build_lds(pe_ctx* ctx, int64_t n_jobs, const BatchDict& bd) {
  if (n_jobs == 0 || ctx->Ns == 0) return false;
  const std::vector<int64_t>* vals = bd.vals;
  std::vector<uint32_t> needs;
  for (int64_t v : bd.vals[4]) needs.push_back((uint32_t)v);   // ascending
  if ((int)needs.size() > pe::LD_MAXNEED) return false;
  pe::LdsSpec sp{};
  int fdim[pe::LD_MAXF];
  for (int d = 0; d < pe::D; ++d) {
    if (vals[d].size() == 1) {
      sp.fold_dim[sp.nfold] = d;
      sp.fold_val[sp.nfold++] = vals[d][0];
    } else {
      fdim[sp.nf++] = d;
    }
  }
  // planes of a field with m values at L levels (lower levels base B, top level whatever is left):
  // level 0 has B planes, levels 1 .. L-2 B + 1 (their GE(c + 1) is read too), the top m / B^(L-1) + 2
  auto plan = [](int64_t m, int L, int64_t& B) -> int64_t {
    if (L == 1) {
      B = m;
      return m;
    }
    int64_t best = INT64_MAX;
    for (int64_t b = 2; b <= m; ++b) {
      int64_t low = 1;
      for (int k = 1; k < L; ++k) low *= b;
      const int64_t T = m / low + 1;
      const int64_t p = (T + 1) + (L - 2) * (b + 1) + b;
      if (p < best) {
        best = p;
        B = b;
      }
      if (low / b * b * b > 4 * m + 4) break;   // past the square-ish optimum
    }
    return best;
  };
  int maxl = pe::LD_MAXL;
  if (const char* e = std::getenv("PE_LDS_MAXL")) maxl = std::max(1, std::min(pe::LD_MAXL, std::atoi(e)));
  int forced_w = 0;
  if (const char* e = std::getenv("PE_LDS_W")) forced_w = std::atoi(e);
  const int64_t nneed = (int64_t)needs.size();
  bool cross = true;
  if (const char* e = std::getenv("PE_LDS_CROSS")) cross = std::atoi(e) != 0;
  int bestW = 0, bestL[pe::LD_MAXF] = {1, 1, 1, 1}, bestX = 0;   // bestX: bit i = field i crossed
  int64_t bestB[pe::LD_MAXF] = {0, 0, 0, 0};
  double bestCost = 1e300;
  for (int W : {4, 2, 1}) {
    if (forced_w && W != forced_w) continue;
    const int64_t budget = 163840 / (256 * W);
    int combos = 1;
    for (int i = 0; i < sp.nf; ++i) combos *= maxl;
    for (int cix = 0; cix < combos; ++cix) {
      int L[pe::LD_MAXF];
      int64_t B[pe::LD_MAXF], P[pe::LD_MAXF];
      bool ok = true;
      for (int i = 0, x = cix; i < sp.nf; ++i, x /= maxl) {
        L[i] = 1 + x % maxl;
        const int64_t m = (int64_t)vals[fdim[i]].size();
        if (L[i] > 1 && m < 4) L[i] = 1;
        if (L[i] == 4 && W == 1) ok = false;     // four-level kernels exist for W >= 2 only
        P[i] = plan(m, L[i], B[i]);
      }
      if (!ok) continue;
      // crossed sets: the k single-level fields with the fewest values, k = 0 .. all of them
      int one[pe::LD_MAXF], n1 = 0;
      for (int i = 0; i < sp.nf; ++i)
        if (L[i] == 1) one[n1++] = i;
      std::sort(one, one + n1, [&](int a, int b) { return vals[fdim[a]].size() < vals[fdim[b]].size(); });
      // a crossing must not cost the second workgroup per CU (LDS <= 80 KiB) the uncrossed plan has:
      // store-bound batches need the waves more than the plane read they save ("many": R 4 -> 2, 90 KB,
      // 2.32 -> 2.68 ms when crossing pushed the LDS past half the CU's)
      int64_t planes0 = nneed;
      for (int i = 0; i < sp.nf; ++i) planes0 += P[i];
      const int64_t half = 81920 / (256 * W);
      for (int k = 0; k <= (cross ? n1 : 0); ++k) {
        int xs = 0;
        int64_t xprod = 1;
        for (int t = 0; t < k; ++t) {
          xs |= 1 << one[t];
          xprod *= (int64_t)vals[fdim[one[t]]].size();
        }
        int64_t planes = nneed * xprod, reads = 1, entries = 0, nfk = 0;
        for (int i = 0; i < sp.nf; ++i) {
          if (xs >> i & 1) continue;
          planes += P[i];
          reads += 2 * L[i] - 1;
          entries += L[i];
          ++nfk;
        }
        if (entries > pe::LD_NEED_SLOT || planes > budget || planes > 65535) continue;
        if (k > 0 && planes > half && planes0 <= half) continue;
        // per job and 8192 nodes, in CU cycles: LDS plane reads (b128 / b64 / read2st64_b64: 4 per
        // KiB, b32: 8) -- the kernel's bound -- plus its VALU at ~0.6 CU cycles per wave instruction:
        // per entry a readlane half and an address, ~6 fixed, and the three-input combines (2 per
        // extra level and word, 4 per 8192 nodes whatever W)
        const double valu = (4.0 / W) * (1.5 * (double)entries + 6.0) + 4.0 * (double)(reads - 1 - nfk + nfk / 2);
        const double cost = reads * (W == 1 ? 8.0 : 4.0) + 0.625 * valu;
        if (cost < bestCost - 1e-9) {
          bestCost = cost;
          bestW = W;
          bestX = xs;
          for (int i = 0; i < sp.nf; ++i) {
            bestL[i] = L[i];
            bestB[i] = B[i];
          }
        }
      }
    }
  }
  if (!bestW) return false;
  // fields in the kernel's order: four-level first, then three-, two- and single-level; the crossed
  // fields last (they keep a rank row but no digit planes)
  const int nx = __builtin_popcount(bestX);
  {
    int ord[pe::LD_MAXF] = {0, 1, 2, 3};
    auto key = [&](int x) { return (bestX >> x & 1) ? 0 : bestL[x]; };
    std::stable_sort(ord, ord + sp.nf, [&](int x, int y) { return key(x) > key(y); });
    int d2[pe::LD_MAXF], L2[pe::LD_MAXF];
    int64_t B2[pe::LD_MAXF];
    for (int i = 0; i < sp.nf; ++i) {
      d2[i] = fdim[ord[i]];
      L2[i] = bestL[ord[i]];
      B2[i] = bestB[ord[i]];
    }
    for (int i = 0; i < sp.nf; ++i) {
      fdim[i] = d2[i];
      bestL[i] = L2[i];
      bestB[i] = B2[i];
    }
  }
  sp.nf -= nx;
  int shape[4] = {0, 0, 0, 0};
  for (int i = 0; i < sp.nf; ++i) ++shape[4 - bestL[i]];
  // level specs, plane bases
  int32_t p = 0;
  int64_t voff = 0;
  std::vector<int64_t> allv;
  for (int i = 0; i < sp.nf; ++i) {
    const int64_t m = (int64_t)vals[fdim[i]].size(), B = bestB[i];
    const int L = bestL[i];
    sp.dim[i] = fdim[i];
    sp.L[i] = L;
    sp.voff[i] = voff;
    sp.m[i] = m;
    allv.insert(allv.end(), vals[fdim[i]].begin(), vals[fdim[i]].end());
    voff += m;
    for (int k = 0; k < L; ++k) {
      const bool top = k == L - 1;
      int64_t dv = 1;
      for (int t = 0; t < k; ++t) dv *= B;
      sp.div[i][k] = (uint32_t)dv;
      sp.mod[i][k] = top ? 0u : (uint32_t)B;
      if (L == 1) {
        sp.vlo[i][k] = 1;
        sp.nv[i][k] = (int32_t)m;
      } else {
        sp.vlo[i][k] = 0;
        sp.nv[i][k] = (int32_t)(top ? m / dv + 2 : (k == 0 ? B : B + 1));
      }
      sp.pbase[i][k] = p;
      p += sp.nv[i][k];
    }
  }
  sp.nx = nx;
  sp.xprod = 1;
  for (int x = 0; x < nx; ++x) {   // crossed fields: rank rows and values after the digit fields
    const int i = sp.nf + x;
    const int64_t m = (int64_t)vals[fdim[i]].size();
    sp.dim[i] = fdim[i];
    sp.L[i] = 1;
    sp.voff[i] = voff;
    sp.m[i] = m;
    allv.insert(allv.end(), vals[fdim[i]].begin(), vals[fdim[i]].end());
    voff += m;
    sp.xstride[x] = sp.xprod;
    sp.xprod *= (int32_t)m;
  }
  sp.need_pbase = p;
  sp.nneed = (int32_t)nneed;
  for (int64_t i = 0; i < nneed; ++i) sp.needs[i] = needs[i];
  sp.nplanes = p + (int32_t)(nneed * sp.xprod);
  // geometry: W words per lane, blocks of 2048 W nodes, R job phases for an even spread over the CUs
  const int W = bestW;
  const int64_t S = 2048 * W;
  const int64_t nblk = (ctx->Ns + S - 1) / S;
  const int64_t lds_bytes = (int64_t)sp.nplanes * S / 8;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, 163840 / std::max<int64_t>(lds_bytes, 1)));
  const int64_t slots = (int64_t)ctx->num_cu * per_cu;
  // job phases R: every workgroup builds its block's planes before its share (1/R) of the jobs, so
  // minimise rounds(R) x (prologue + 1/R) -- the prologue being ~2 % of one block's full job sweep
  int64_t R = 1;
  double best_t = 1e300;
  for (int64_t r = 1; r <= 64 && (r == 1 || 16 * r <= n_jobs); ++r) {
    const int64_t rounds = (nblk * r + slots - 1) / slots;
    const double t = (double)rounds * (0.02 + 1.0 / (double)r);
    if (t < best_t - 1e-9) {
      best_t = t;
      R = r;
    }
  }
  if (const char* ev = std::getenv("PE_LDS_R")) R = std::max<int64_t>(1, std::atoll(ev));
  const int64_t Tmax = ((n_jobs + R - 1) / R + 15) / 16;
  const int64_t Tpad = round_up(std::max<int64_t>(Tmax, 1), 16);
  // job codes: u16 plane indices, per job first
  std::vector<uint16_t> jc((size_t)n_jobs * pe::LD_CODE, 0);
  parallel_for(n_jobs, [&](int64_t j0, int64_t j1) {
  for (int64_t j = j0; j < j1; ++j) {
    uint16_t* c = jc.data() + (size_t)j * pe::LD_CODE;
    for (int i = 0; i < sp.nf; ++i) {
      const int64_t rank = (int64_t)bd.rank[fdim[i]][j] + 1;
      const int o = pe::lds_field_off(i, shape[0], shape[1], shape[2]);
      if (sp.L[i] == 1) {
        c[o] = (uint16_t)(sp.pbase[i][0] + rank - 1);
      } else {
        int64_t x = rank;
        for (int k = 0; k < sp.L[i]; ++k) {
          const int64_t digit = sp.mod[i][k] ? x % sp.mod[i][k] : x;
          x = sp.mod[i][k] ? x / sp.mod[i][k] : 0;
          c[o + k] = (uint16_t)(sp.pbase[i][k] + digit);
        }
      }
    }
    int64_t xc = 0;   // the job's crossed values (0-based value index: the node's rank must exceed it)
    for (int x = 0; x < sp.nx; ++x) xc += (int64_t)bd.rank[fdim[sp.nf + x]][j] * sp.xstride[x];
    c[pe::lds_need_slot(shape[0], shape[1], shape[2], shape[3])] =
        (uint16_t)(sp.need_pbase + bd.rank[4][j] * sp.xprod + xc);
  }
  });
  // slot (r * 16 + w) * Tpad + t = job r + R (w + 16 t), the t-th of wave w's run in phase r (the
  // kernel's consumption order); each slot's job in lds_rows for the counts
  std::vector<uint16_t> codes((size_t)(R * 16 * Tpad * pe::LD_CODE), 0);
  std::vector<uint32_t> rows((size_t)(R * 16 * Tpad), ~0u);
  {
    int64_t pos = 0;
    for (int64_t v = 0; v < R * 16; ++v) {
      const int64_t r = v / 16, w = v % 16, j0 = r + R * w;
      const int64_t T = j0 < n_jobs ? (n_jobs - j0 + 16 * R - 1) / (16 * R) : 0;
      for (int64_t t = 0; t < T; ++t, ++pos) {
        const uint32_t j = (uint32_t)(j0 + 16 * R * t);
        std::memcpy(codes.data() + (size_t)((v * Tpad + t) * pe::LD_CODE), jc.data() + (size_t)j * pe::LD_CODE,
                    pe::LD_CODE * 2);
        rows[(size_t)(v * Tpad + t)] = j;
      }
    }
    if (pos != n_jobs) raise(PE_EINVAL, "lds: run lengths do not cover the batch");
  }
  if (std::getenv("PE_LDS_DEBUG")) {   // diagnostics: the chosen configuration
    std::fprintf(stderr, "lds: W %d nblk %lld R %lld planes %d need %d fold %d cross %d x %d |", W, (long long)nblk,
                 (long long)R, sp.nplanes, sp.nneed, sp.nfold, sp.nx, sp.xprod);
    for (int i = 0; i < sp.nf; ++i)
      std::fprintf(stderr, " dim %d m %lld L %d B %u", sp.dim[i], (long long)sp.m[i], sp.L[i], sp.mod[i][0]);
    std::fprintf(stderr, "\n");
  }
  ctx->lds = sp;
  ctx->lds_W = W;
  for (int i = 0; i < 4; ++i) ctx->lds_shape[i] = shape[i];
  ctx->lds_nblk = nblk;
  ctx->lds_R = R;
  ctx->lds_Tpad = Tpad;
  // (+ the kernel's per-block work-unit counters, zeroed with the slots every step)
  hipchk(ctx->lds_slots.ensure((size_t)R * 16 * Tpad + (size_t)ctx->lds_nblk), "alloc count slots");
  hipchk(ctx->lds_rows.ensure((size_t)R * 16 * Tpad), "alloc count rows");
  hipchk(hipMemcpyAsync(ctx->lds_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, ctx->stream),
         "H2D lds rows");
  ctx->lds_npad = nblk * S;
  ctx->lds_pitch = nblk * S / 64;
  hipchk(ctx->lds_spec_d.ensure(1), "alloc lds spec");
  hipchk(ctx->lds_vals.ensure(std::max<size_t>(allv.size(), 1)), "alloc lds vals");
  hipchk(ctx->lds_codes.ensure(codes.size()), "alloc lds codes");
  hipchk(ctx->lds_ranks.ensure((size_t)std::max(sp.nf + sp.nx, 1) * ctx->lds_npad), "alloc lds ranks");
  hipchk(ctx->lds_aux.ensure((size_t)2 * ctx->lds_npad), "alloc lds aux");
  hipchk(hipMemcpyAsync(ctx->lds_spec_d.p, &ctx->lds, sizeof(pe::LdsSpec), hipMemcpyHostToDevice, ctx->stream),
         "H2D lds spec");
  if (!allv.empty())
    hipchk(hipMemcpyAsync(ctx->lds_vals.p, allv.data(), allv.size() * 8, hipMemcpyHostToDevice, ctx->stream),
           "H2D lds vals");
  hipchk(hipMemcpyAsync(ctx->lds_codes.p, codes.data(), codes.size() * 2, hipMemcpyHostToDevice, ctx->stream),
         "H2D lds codes");
  hipchk(hipStreamSynchronize(ctx->stream), "sync lds upload");   // the host vectors die here
  return true;
}

static void fit_upload(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need) {
  if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
  if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
  if (n_jobs > 0) {
    need_ptr(req, "req");
    check_req(req, n_jobs, "req");
  }
  const int64_t Jp = round_up(std::max<int64_t>(n_jobs, 1), pe::FM_JT);
  ctx->fit_J = n_jobs;
  ctx->fit_Jp = Jp;
  ctx->Wn = (ctx->Ns + 63) / 64;
  ctx->Wt = (ctx->Wn + 3) / 4;
  // one bit-plane set (register planes) > LDS digit planes > bit-plane sets > coded > int32 > int64
  const bool planes_ok = ctx->fit_path_mask & PATH_PLANES;
  ctx->fit_path = -1;
  if (n_jobs > 0 && (ctx->fit_path_mask & (PATH_PLANES | PATH_LDS | PATH_CODED))) {
    BatchDict bd;
    build_dict(bd, n_jobs, req, need);
    if (planes_ok && build_planes(ctx, n_jobs, bd, false)) ctx->fit_path = 3;
    else if ((ctx->fit_path_mask & PATH_LDS) && build_lds(ctx, n_jobs, bd)) ctx->fit_path = 4;
    else if (planes_ok && build_planes(ctx, n_jobs, bd, true)) ctx->fit_path = 3;
    else if ((ctx->fit_path_mask & PATH_CODED) && build_codes(ctx, n_jobs, bd)) ctx->fit_path = 2;
  }
  if (ctx->fit_path < 0) {
    // compare paths.  Exact 32-bit form: per dim the shift that brings the largest request below
    // 2^31, valid only if 2^shift divides every request of the batch in that dim
    bool use32 = true;
    for (int d = 0; d < pe::D && use32; ++d) {
      int64_t mx = 0, orv = 0;
      for (int64_t j = 0; j < n_jobs; ++j) {
        mx = std::max(mx, req[j * pe::D + d]);
        orv |= req[j * pe::D + d];
      }
      int sh = 0;
      while (sh < 62 && (mx >> sh) > (int64_t)INT32_MAX) ++sh;
      if (orv & ((int64_t(1) << sh) - 1)) use32 = false;
      ctx->fit_shift[d] = sh;
    }
    ctx->fit32 = use32 && (ctx->fit_path_mask & PATH_I32);
    ctx->fit_path = ctx->fit32 ? 1 : 0;
    if (ctx->fit32) {
      std::vector<pe::ReqRec32> r32((size_t)Jp);
      for (int64_t j = 0; j < Jp; ++j) {
        std::memset(&r32[j], 0, sizeof(pe::ReqRec32));
        for (int d = 0; d < pe::D; ++d)
          r32[j].q[d] = j < n_jobs ? (int32_t)(req[j * pe::D + d] >> ctx->fit_shift[d]) : INT32_MAX;
        r32[j].need = j < n_jobs ? (need ? need[j] : 0u) : 0xFFFFFFFFu;
      }
      hipchk(ctx->fit_jobs32.ensure(Jp), "alloc fit jobs32");
      hipchk(ctx->res32.ensure((size_t)pe::D * ctx->stride), "alloc res32");
      hipchk(hipMemcpyAsync(ctx->fit_jobs32.p, r32.data(), Jp * sizeof(pe::ReqRec32), hipMemcpyHostToDevice,
                            ctx->stream),
             "H2D fit jobs32");
      hipchk(hipStreamSynchronize(ctx->stream), "sync fit jobs32");   // the host vector dies here
    } else {
      std::vector<ReqRec> recs((size_t)Jp);
      for (int64_t j = 0; j < Jp; ++j) {
        if (j < n_jobs) fill_req(recs[j], req + j * pe::D, need ? need[j] : 0u);
        else {
          const int64_t never[pe::D] = {INT64_MAX, INT64_MAX, INT64_MAX, INT64_MAX};
          fill_req(recs[j], never, 0xFFFFFFFFu);
        }
      }
      hipchk(ctx->fit_jobs.ensure(Jp), "alloc fit jobs");
      hipchk(hipMemcpyAsync(ctx->fit_jobs.p, recs.data(), Jp * sizeof(ReqRec), hipMemcpyHostToDevice, ctx->stream),
             "H2D fit jobs");
      hipchk(hipStreamSynchronize(ctx->stream), "sync fit jobs");
    }
  }
  const size_t mask_words = ctx->fit_path == 4   ? (size_t)std::max<int64_t>(n_jobs, 1) * ctx->lds_pitch
                            : ctx->fit_path == 3 ? (size_t)std::max<int64_t>(n_jobs, 1) *
                                                       (ctx->pl_rows ? ctx->pl_pitch : ctx->pl_nblk) * 128
                            : ctx->fit_path == 2 ? (size_t)(ctx->code_Jp / 64) * ctx->node_stride
                                                 : (size_t)Jp * std::max<int64_t>(ctx->Wt, 1) * 4;
  static const unsigned mask_flags = std::getenv("PE_MASK_CONTIG") ? hipDeviceMallocContiguous : 0u;
  hipchk(ctx->mask.ensure(mask_words, mask_flags), "alloc fit mask");
  const int64_t n_counts = std::max<int64_t>(Jp, ctx->fit_path == 3 ? ctx->pl_counts_n : 0);
  // (+ the row sweep's per-block work-unit counters, zeroed with the counts every step)
  hipchk(ctx->counts.ensure(n_counts + (ctx->fit_path == 3 ? ctx->pl_nblk : 0)), "alloc fit counts");
  hipchk(ctx->h_counts.ensure(n_counts), "alloc pinned counts");
  hipchk(hipStreamSynchronize(ctx->stream), "sync fit upload");
  ctx->fit_uploaded = true;
}

static void fit_run(pe_ctx* ctx) {
  if (!ctx->fit_uploaded) raise(PE_ESTATE, "pe_jobs_upload first");
  const int64_t J = ctx->fit_J;
  // the single-plane-set encode zeroes the count slots itself (one launch fewer per step)
  const bool encode_zeroes = ctx->fit_path == 3 && ctx->pl_sets.empty() && J > 0 && ctx->Ns > 0 && ctx->pl_nblk > 0;
  if (!encode_zeroes)
    hipchk(hipMemsetAsync(ctx->counts.p, 0, ctx->counts.n * sizeof(unsigned long long), ctx->stream), "memset counts");
  if (J == 0 || ctx->Ns == 0) return;
  // enough waves to fill 256 CUs several times over; at most 16 tiles (4096 nodes) per wave
  const int64_t waves_y = (J + pe::FM_JT - 1) / pe::FM_JT;
  const int64_t want_x = std::max<int64_t>(1, (16384 + waves_y - 1) / waves_y);
  int64_t tpw = (ctx->Ns + 256 * want_x - 1) / (256 * want_x);
  tpw = std::min<int64_t>(16, std::max<int64_t>(1, tpw));
  if (ctx->fit_path == 4) {
    hipchk(hipMemsetAsync(ctx->lds_slots.p, 0, ((size_t)ctx->lds_R * 16 * ctx->lds_Tpad + ctx->lds_nblk) * 4, ctx->stream),
           "memset count slots");
    hipchk(pe::launch_node_ranks(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->lds_npad,
                                 ctx->lds_spec_d.p, ctx->lds_vals.p, ctx->lds_ranks.p, ctx->lds_aux.p),
           "launch node_ranks");
    hipchk(pe::launch_fit_mask_lds(ctx->stream, ctx->lds_W, ctx->lds_shape, ctx->lds_spec_d.p, ctx->lds.nplanes,
                                   ctx->lds_ranks.p,
                                   ctx->lds_npad, ctx->lds_aux.p, ctx->lds_nblk, ctx->lds_codes.p, J,
                                   ctx->lds_R, ctx->lds_Tpad, ctx->lds_pitch * 8,
                                   reinterpret_cast<uint8_t*>(ctx->mask.p), ctx->lds_slots.p,
                                   std::getenv("PE_FIT_STATIC") ? nullptr
                                                                : ctx->lds_slots.p + (size_t)ctx->lds_R * 16 * ctx->lds_Tpad),
           "launch fit_mask_lds");
    hipchk(pe::launch_lds_counts(ctx->stream, ctx->lds_slots.p, ctx->lds_rows.p, ctx->lds_R * 16 * ctx->lds_Tpad,
                                 ctx->counts.p),
           "launch lds_counts");
    ctx->stats.fit_runs_lds += 1;
  } else if (ctx->fit_path == 3) {
    // ~16k waves: every 8192-node block times enough job ranges, at least 64 jobs per wave
    if (!ctx->pl_sets.empty()) {   // plane sets: one encode pass and one sweep for all of them
      const int ns = (int)ctx->pl_sets.size();
      hipchk(pe::launch_encode_planes_sets(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->pl_nblk,
                                           ctx->pl_specs_d.p, ns, ctx->planes.p),
             "launch encode_planes_sets");
      hipchk(pe::launch_fit_mask_planes_sets(ctx->stream, ctx->planes.p, ctx->pl_nblk, ctx->plane_jobs.p,
                                             ctx->pl_meta_d.p, ns, ctx->pl_sets[0].R,
                                             reinterpret_cast<uint32_t*>(ctx->mask.p), ctx->counts.p, ctx->pl_pitch),
             "launch fit_mask_planes_sets");
      ctx->stats.fit_runs_planes += 1;
      ctx->stats.fit_runs_sets += 1;
      ctx->stats.fit_evals += J * ctx->Ns;
      return;
    }
    hipchk(pe::launch_encode_planes(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->pl_nblk,
                                    ctx->plane, ctx->pl_specs_d.p, ctx->planes.p, ctx->counts.p, ctx->counts.n),
           "launch encode_planes");
    if (ctx->pl_rows) {
      // PE_FIT_STATIC=1: every wave keeps its own phase (no work units; A/B, read per call)
      unsigned long long* const units = std::getenv("PE_FIT_STATIC") ? nullptr : ctx->counts.p + ctx->pl_counts_n;
      hipchk(pe::launch_fit_mask_planes_rows(ctx->stream, ctx->planes.p, ctx->pl_nblk, ctx->plane_jobs.p, J, ctx->pl_R,
                                             reinterpret_cast<uint32_t*>(ctx->mask.p), ctx->counts.p, ctx->pl_pitch,
                                             units),
             "launch fit_mask_planes_rows");
    } else {
      const int64_t ranges = std::max<int64_t>(1, (16384 + ctx->pl_nblk - 1) / ctx->pl_nblk);
      const int64_t jpw = std::max<int64_t>(64, (J + ranges - 1) / ranges);
      hipchk(pe::launch_fit_mask_planes(ctx->stream, ctx->planes.p, ctx->pl_nblk, ctx->plane_jobs.p, J, jpw,
                                        reinterpret_cast<uint32_t*>(ctx->mask.p), ctx->counts.p),
             "launch fit_mask_planes");
    }
    ctx->stats.fit_runs_planes += 1;
  } else if (ctx->fit_path == 2) {
    const int64_t jblocks = ctx->code_Jp / pe::FC_JT;
    const int64_t want_x2 = std::max<int64_t>(1, (16384 + jblocks - 1) / jblocks);
    int64_t tpw2 = (ctx->Ns + 64 * pe::FC_CH * want_x2 - 1) / (64 * pe::FC_CH * want_x2);
    tpw2 = std::min<int64_t>(64, std::max<int64_t>(1, tpw2));
    hipchk(pe::launch_encode_nodes(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->node_stride,
                                   ctx->code, ctx->code_vals.p, ctx->code_needs.p, ctx->code_x.p),
           "launch encode_nodes");
    hipchk(pe::launch_fit_mask_coded(ctx->stream, ctx->code.therm, ctx->code_x.p, ctx->Ns, ctx->node_stride, ctx->code_jobs.p,
                                     ~ctx->code.guard, J, tpw2, ctx->mask.p, ctx->counts.p),
           "launch fit_mask_coded");
    ctx->stats.fit_runs_coded += 1;
    ctx->stats.fit_runs_therm += ctx->code.therm;
  } else if (ctx->fit32) {
    hipchk(pe::launch_compress_res(ctx->stream, ctx->res.p, ctx->res32.p, ctx->stride, ctx->Ns, ctx->fit_shift),
           "launch compress_res");
    hipchk(pe::launch_fit_mask32(ctx->stream, ctx->res32.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->Wt,
                                 ctx->fit_jobs32.p, J, tpw, ctx->mask.p, ctx->counts.p),
           "launch fit_mask32");
    ctx->stats.fit_runs_i32 += 1;
  } else {
    hipchk(pe::launch_fit_mask(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->Wt,
                               ctx->fit_jobs.p, J, tpw, ctx->mask.p, ctx->counts.p),
           "launch fit_mask");
    ctx->stats.fit_runs_i64 += 1;
  }
  ctx->stats.fit_evals += J * ctx->Ns;
}

static void fit_counts(pe_ctx* ctx, int64_t* out) {
  const int64_t J = ctx->fit_J;
  if (J == 0) return;
  if (ctx->fit_path == 3 && !ctx->pl_sets.empty()) {   // plane sets: slot -> row
    hipchk(hipMemcpyAsync(ctx->h_counts.p, ctx->counts.p, ctx->pl_counts_n * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, ctx->stream),
           "D2H counts");
    hipchk(hipStreamSynchronize(ctx->stream), "sync counts");
    for (int64_t k = 0; k < ctx->pl_counts_n; ++k)
      if (ctx->pl_cnt_row[k] >= 0) out[ctx->pl_cnt_row[k]] = (int64_t)ctx->h_counts.p[k];
    return;
  }
  const bool phased = ctx->fit_path == 3 && ctx->pl_rows;
  const int64_t R = phased ? ctx->pl_R : 1, Jr = phased ? ((J + R - 1) / R + 3) / 4 * 4 : J;
  hipchk(hipMemcpyAsync(ctx->h_counts.p, ctx->counts.p, R * Jr * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        ctx->stream),
         "D2H counts");
  hipchk(hipStreamSynchronize(ctx->stream), "sync counts");
  for (int64_t j = 0; j < J; ++j) out[j] = (int64_t)ctx->h_counts.p[(j % R) * Jr + j / R];
}

int pe_jobs_upload(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need) {
  return guarded(ctx, [&]() -> int {
    fit_upload(ctx, n_jobs, req, need);
    return PE_OK;
  });
}

int pe_fit_mask_run(pe_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    fit_run(ctx);
    return PE_OK;
  });
}

int pe_fit_counts(pe_ctx* ctx, int64_t* out) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->fit_uploaded) raise(PE_ESTATE, "pe_jobs_upload first");
    need_ptr(out, "out_feasible_count");
    fit_counts(ctx, out);
    return PE_OK;
  });
}

int pe_fit_mask_rows(pe_ctx* ctx, int64_t row0, int64_t n_rows, uint64_t* out) {
  return guarded(ctx, [&]() -> int {
    if (!ctx->fit_uploaded) raise(PE_ESTATE, "pe_jobs_upload first");
    if (row0 < 0 || n_rows < 0 || row0 + n_rows > ctx->fit_J) raise(PE_EINVAL, "row range");
    if (n_rows == 0 || ctx->Wn == 0) return PE_OK;
    need_ptr(out, "out");
    if ((ctx->fit_path == 3 && ctx->pl_rows) || ctx->fit_path == 4) {   // row-major
      const int64_t pitch = ctx->fit_path == 4 ? ctx->lds_pitch : ctx->pl_pitch * 128;
      hipchk(hipMemcpy2DAsync(out, (size_t)ctx->Wn * 8, ctx->mask.p + (size_t)row0 * pitch, (size_t)pitch * 8,
                              (size_t)ctx->Wn * 8, (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream),
             "D2H mask rows");
      hipchk(hipStreamSynchronize(ctx->stream), "sync mask");
      return PE_OK;
    }
    if (ctx->fit_path == 3) {   // block-major: one strided copy per 8192-node block (128 u64 per row)
      for (int64_t b = 0; b * 128 < ctx->Wn; ++b) {
        const int64_t w = std::min<int64_t>(128, ctx->Wn - b * 128);
        hipchk(hipMemcpy2DAsync(out + b * 128, (size_t)ctx->Wn * 8, ctx->mask.p + ((size_t)b * ctx->fit_J + row0) * 128,
                                128 * 8, (size_t)w * 8, (size_t)n_rows, hipMemcpyDeviceToHost, ctx->stream),
               "D2H mask rows");
      }
      hipchk(hipStreamSynchronize(ctx->stream), "sync mask");
      return PE_OK;
    }
    if (ctx->fit_path == 2) {
      // bits-over-jobs layout: copy the 64-job bands, transpose the rows out
      const int64_t b0 = row0 / 64, b1 = (row0 + n_rows - 1) / 64;
      const size_t band = (size_t)ctx->node_stride;
      std::vector<uint64_t> bands((size_t)(b1 - b0 + 1) * band);
      hipchk(hipMemcpyAsync(bands.data(), ctx->mask.p + (size_t)b0 * band, bands.size() * 8, hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H mask");
      hipchk(hipStreamSynchronize(ctx->stream), "sync mask");
      for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t j = row0 + r;
        const uint64_t* bw = bands.data() + (size_t)(j / 64 - b0) * band;
        const int bit = (int)(j % 64);
        for (int64_t c = 0; c < ctx->Wn; ++c) {
          uint64_t word = 0;
          for (int i = 0; i < 64 && c * 64 + i < ctx->Ns; ++i) word |= ((bw[c * 64 + i] >> bit) & 1ull) << i;
          out[(size_t)r * ctx->Wn + c] = word;
        }
      }
      return PE_OK;
    }
    // copy the 16-row tile bands covering the rows, then untile into row-major
    const int64_t t0 = row0 / 16, t1 = (row0 + n_rows - 1) / 16;
    const size_t band = (size_t)ctx->Wt * 64;
    std::vector<uint64_t> tiles((size_t)(t1 - t0 + 1) * band);
    hipchk(hipMemcpyAsync(tiles.data(), ctx->mask.p + (size_t)t0 * band, tiles.size() * 8, hipMemcpyDeviceToHost,
                          ctx->stream),
           "D2H mask");
    hipchk(hipStreamSynchronize(ctx->stream), "sync mask");
    for (int64_t r = 0; r < n_rows; ++r)
      for (int64_t c = 0; c < ctx->Wn; ++c)
        out[(size_t)r * ctx->Wn + c] = tiles[(size_t)(pe::fm_word_index(row0 + r, c, ctx->Wt) - t0 * (int64_t)band)];
    return PE_OK;
  });
}

int pe_fit_mask(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, int64_t* out_feasible_count,
                const uint64_t** dev_mask, int64_t* words_per_row) {
  return guarded(ctx, [&]() -> int {
    fit_upload(ctx, n_jobs, req, need);
    fit_run(ctx);
    if (out_feasible_count) fit_counts(ctx, out_feasible_count);
    else hipchk(hipStreamSynchronize(ctx->stream), "sync fit");
    if (dev_mask) *dev_mask = ctx->mask.p;
    if (words_per_row) *words_per_row = ctx->Wn;
    return PE_OK;
  });
}

int pe_fit_mask_layout(const pe_ctx* ctx, int32_t* layout) {
  if (!ctx || !layout) return PE_EINVAL;
  *layout = ctx->fit_path == 4   ? PE_MASK_ROWS
            : ctx->fit_path == 3 ? (ctx->pl_rows ? PE_MASK_ROWS : PE_MASK_NODE_BLOCKS)
            : ctx->fit_path == 2 ? PE_MASK_JOB_BITS
                                 : PE_MASK_NODE_TILES;
  return PE_OK;
}

int pe_fit_mask_row_pitch(const pe_ctx* ctx, int64_t* words) {
  if (!ctx || !words) return PE_EINVAL;
  *words = ctx->fit_path == 4 ? ctx->lds_pitch : ctx->fit_path == 3 && ctx->pl_rows ? ctx->pl_pitch * 128 : 0;
  return PE_OK;
}

int pe_synchronize(pe_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    hipchk(hipStreamSynchronize(ctx->stream), "sync");
    return PE_OK;
  });
}

void* pe_stream(pe_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int pe_get_stats(const pe_ctx* ctx, pe_stats* out) {
  if (!ctx || !out) return PE_EINVAL;
  *out = ctx->stats;
  return PE_OK;
}

int pe_reset_stats(pe_ctx* ctx) {
  if (!ctx) return PE_EINVAL;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->stats = pe_stats{};
  return PE_OK;
}

}  // extern "C"
