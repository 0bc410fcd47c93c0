// libplacement: the greedy placement (pe_place_greedy).  Which protocol a call runs -- unsharded walk or
// full scan, RCCL windows, the copying or the zero-copy host exchange, pipeline depth, early post -- is
// decided once per call in pe_greedy_mode.h (GreedyKnobs: the environment, GreedyMode: what follows from
// it and the context); GreedyRun below holds one call's state and runs it.
#include <chrono>
#include <cstdio>
#include <deque>
#include <utility>

#include "pe_ctx.h"
#include "pe_greedy_mode.h"
#include "pe_merge.h"

namespace {

using Clock = std::chrono::steady_clock;
double ms(Clock::duration d) { return std::chrono::duration<double, std::milli>(d).count(); }
double us(Clock::duration d) { return std::chrono::duration<double, std::micro>(d).count(); }
double ms_since(Clock::time_point t) { return ms(Clock::now() - t); }
double us_since(Clock::time_point t) { return us(Clock::now() - t); }

const pe::GreedyLimits kLimits{pe::WK_ROUND,   pe::MG_CAP,  pe::MG_THREADS,        pe::RM_MAX_WORLD,
                               pe::RM_MAX_LDS, kMaxMergers, &pe::cand_group_bytes, &pe::merge_ranked_lds};

// The next generation of a signalled window (never 0: an unsignalled window's).
uint32_t next_gen(pe_ctx* ctx) {
  if (++ctx->walk_gen == 0) ++ctx->walk_gen;
  return ctx->walk_gen;
}

// The sorted-walk index of the shard over the current residuals (g_kn must be current): sort the
// walkable nodes by K(n), gather the sorted SoA copy and the round summaries, empty the overlay
// (then holding only the saturating nodes).
pe::WalkIndex walk_index(pe_ctx* ctx, int set) {
  pe_ctx::WalkSet& x = ctx->ws[set];
  pe::WalkIndex w{};
  w.sk = x.sk.p;
  w.sr = x.sr.p;
  w.sl = x.sl.p;
  w.pos = x.pos.p;
  w.rmin = x.rmin.p;
  w.rmax = x.rmax.p;
  w.ror = x.ror.p;
  w.ovl = x.ovl.p;
  w.ovl_n = x.ovln.p;
  w.in_ovl = x.inovl.p;
  w.ovl_idx = x.ovidx.p;
  w.ovl_res = x.ovres.p;
  w.ovl_lab = x.ovlab.p;
  w.ovl_kn = x.ovkn.p;
  w.stat = ctx->w_stat.p;
  w.sstride = ctx->stride;
  w.nr = (ctx->Ns + pe::WK_ROUND - 1) / pe::WK_ROUND;
  return w;
}
pe::WalkIndex walk_index(pe_ctx* ctx) { return walk_index(ctx, ctx->w_cur); }

// Index set `set` allocated and its overlay / pos cleared on stream s; returns the sort scratch size.
size_t walk_set_prepare(pe_ctx* ctx, int set, hipStream_t s) {
  const int64_t Ns = ctx->Ns, st = std::max<int64_t>(ctx->stride, 1);
  const int64_t nr = std::max<int64_t>(1, (Ns + pe::WK_ROUND - 1) / pe::WK_ROUND);
  if (nr > pe::WK_MAXR) raise(PE_EINVAL, "shard too large for the sorted walk");
  pe_ctx::WalkSet& x = ctx->ws[set];
  hipchk(x.sk.ensure(st), "alloc walk keys");
  hipchk(ctx->w_kin.ensure(st), "alloc walk keys");
  hipchk(x.sr.ensure((size_t)pe::D * st), "alloc walk residuals");
  hipchk(x.sl.ensure(st), "alloc walk labels");
  hipchk(x.pos.ensure(st), "alloc walk pos");
  hipchk(x.rmin.ensure(nr), "alloc walk rounds");
  hipchk(x.rmax.ensure((size_t)pe::D * nr), "alloc walk rounds");
  hipchk(x.ror.ensure(nr), "alloc walk rounds");
  hipchk(x.ovl.ensure(st), "alloc overlay");
  hipchk(x.ovln.ensure(1), "alloc overlay");
  hipchk(x.inovl.ensure(st), "alloc overlay");
  hipchk(x.ovidx.ensure(st), "alloc overlay");
  hipchk(x.ovlab.ensure(st), "alloc overlay");
  hipchk(x.ovres.ensure((size_t)pe::D * st), "alloc overlay");
  hipchk(x.ovkn.ensure(st), "alloc overlay");
  size_t tb = 0;
  hipchk(pe::sort_keys_u64(nullptr, &tb, ctx->w_kin.p, x.sk.p, Ns, s), "sort size");
  hipchk(ctx->w_temp.ensure(tb), "alloc sort scratch");
  hipchk(hipMemsetAsync(x.ovln.p, 0, sizeof(int32_t), s), "memset overlay");
  hipchk(hipMemsetAsync(x.inovl.p, 0, (size_t)st * 4, s), "memset overlay");
  hipchk(hipMemsetAsync(x.pos.p, 0xFF, (size_t)st * 4, s), "memset pos");
  return tb;
}

// A side-stream rebuild still running is waited for and dropped (the caller rebuilds in line).
void walk_drop_pending(pe_ctx* ctx) {
  if (!ctx->w_pending) return;
  hipchk(hipStreamSynchronize(ctx->w_s2), "sync walk rebuild");
  ctx->w_pending = false;
}

// In-line rebuild of the current set on the main stream (the walks after it wait for it).
void walk_resort(pe_ctx* ctx) {
  walk_drop_pending(ctx);
  hipStream_t s = ctx->stream;
  const int64_t Ns = ctx->Ns;
  size_t tb = walk_set_prepare(ctx, ctx->w_cur, s);
  const pe::WalkIndex w = walk_index(ctx);
  hipchk(pe::launch_walk_prep(s, ctx->res.p, ctx->stride, Ns, ctx->g_kn.p, ctx->labels.p, ctx->w_kin.p, w),
         "launch walk_prep");
  hipchk(pe::sort_keys_u64(ctx->w_temp.p, &tb, ctx->w_kin.p, w.sk, Ns, s), "sort walk keys");
  hipchk(pe::launch_walk_build(s, ctx->res.p, ctx->stride, ctx->labels.p, Ns, (uint64_t)ctx->begin, w),
         "launch walk_build");
  ctx->w_est = 0;
  ctx->stats.resorts += 1;
}

// Rebuild the other set on the side stream from the residuals as of now (the main stream's point
// `snap`), while the main stream's walks keep using the current set: the applies after `snap`
// update both overlays (apply_kernel nx), and walk_switch drops their nodes' possibly torn sorted
// entries from the new set once it is built.  The side stream has the lowest priority, so the
// walks' blocks are dispatched first.  Correct for the same reason as the in-line rebuild: every
// node changed after the snapshot is in the new overlay with its current state, every other node's
// sorted entry and round summaries are exact (a torn entry only widens its round's summary).
void walk_resort_async(pe_ctx* ctx) {
  if (!ctx->w_s2) {
    int least = 0, greatest = 0;
    hipchk(hipDeviceGetStreamPriorityRange(&least, &greatest), "stream priorities");
    hipchk(hipStreamCreateWithPriority(&ctx->w_s2, hipStreamNonBlocking, least), "side stream");
    hipchk(hipEventCreateWithFlags(&ctx->w_ev_snap, hipEventDisableTiming), "event");
    hipchk(hipEventCreateWithFlags(&ctx->w_ev_done, hipEventDisableTiming), "event");
  }
  hipStream_t s = ctx->stream, s2 = ctx->w_s2;
  const int nx = 1 - ctx->w_cur;
  const int64_t Ns = ctx->Ns;
  size_t tb = walk_set_prepare(ctx, nx, s);   // (cleared on the main stream: before any apply that writes it)
  hipchk(ctx->w_slow.ensure((size_t)std::max<int64_t>(ctx->stride, 1)), "alloc walk slow flags");
  hipchk(hipMemsetAsync(ctx->w_slow.p, 0, (size_t)std::max<int64_t>(ctx->stride, 1) * 4, s), "memset slow flags");
  hipchk(hipEventRecord(ctx->w_ev_snap, s), "event record");
  hipchk(hipStreamWaitEvent(s2, ctx->w_ev_snap, 0), "stream wait");
  const pe::WalkIndex w = walk_index(ctx, nx);
  hipchk(pe::launch_walk_prep(s2, ctx->res.p, ctx->stride, Ns, ctx->g_kn.p, ctx->labels.p, ctx->w_kin.p, w,
                              ctx->w_slow.p),
         "launch walk_prep");
  hipchk(pe::sort_keys_u64(ctx->w_temp.p, &tb, ctx->w_kin.p, w.sk, Ns, s2), "sort walk keys");
  hipchk(pe::launch_walk_build(s2, ctx->res.p, ctx->stride, ctx->labels.p, Ns, (uint64_t)ctx->begin, w),
         "launch walk_build");
  hipchk(hipEventRecord(ctx->w_ev_done, s2), "event record");
  ctx->w_pending = true;
  ctx->w_pend_est = 0;
  ctx->w_pend_windows = 0;
}

// Take over the side-stream rebuild (the main stream waits for it if it is not done yet).
void walk_switch(pe_ctx* ctx) {
  hipStream_t s = ctx->stream;
  const int nx = 1 - ctx->w_cur;
  hipchk(hipStreamWaitEvent(s, ctx->w_ev_done, 0), "stream wait");
  hipchk(pe::launch_walk_switch(s, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->w_slow.p, walk_index(ctx, nx)),
         "launch walk_switch");
  ctx->w_cur = nx;
  ctx->w_pending = false;
  ctx->w_est = ctx->w_pend_est;
  ctx->stats.resorts += 1;
}

// One group's list header of every rank (group_at(r): rank r's list of the group): the smallest shard
// limit *L, each rank's keys and their number cut to [0, K].  False when a header is corrupt (n outside
// [0, K]): no key is taken then, the merged group says so (never read past a list).
template <class At>
bool read_rank_lists(int W, int K, At group_at, const uint64_t** lists, int32_t* ns, uint64_t* L) {
  bool bad = false;
  *L = pe::NO_KEY;
  for (int r = 0; r < W; ++r) {
    const uint8_t* g = group_at(r);
    pe::CandHdr h;
    std::memcpy(&h, g, sizeof(h));
    *L = std::min(*L, h.limit);
    lists[r] = reinterpret_cast<const uint64_t*>(g + sizeof(h));
    bad |= h.n < 0 || h.n > K;
    ns[r] = std::max(0, std::min(h.n, K));
  }
  return !bad;
}

// The caller's batch (pe_place_greedy's arguments, checked).
struct GreedyBatch {
  int64_t n_jobs, G;
  const int32_t *job_group_off, *priority, *group_count;
  const int64_t* group_req;
  const uint32_t* group_need;
};

// The resolver, the seed scorer (pe_resolver.cpp) and the launch helper hand cache lines to each
// other every window / group: keep the three on the CPUs that share this thread's L3 (one CCD)
// for the call -- intersected with the caller's affinity, restored on return; PE_NO_PIN=1 skips.
// With several ranks on one host (world > 1), rank r takes the (r mod n)-th of the n L3 domains
// its affinity allows, so ranks do not pile their spinning threads onto one CCD.
struct Pin {
  cpu_set_t old_set, l3;
  bool on = false;
  Pin(bool no_pin, int rank, int world, int& picked) {
    if (no_pin || pthread_getaffinity_np(pthread_self(), sizeof(old_set), &old_set) != 0) return;
    if (world > 1 && picked == -2) picked = pe::l3_pick(old_set, rank);   // sysfs walk once per context
    const int cpu = world > 1 ? picked : sched_getcpu();
    if (!pe::l3_cpus(cpu, &l3)) return;
    CPU_AND(&l3, &l3, &old_set);
    on = CPU_COUNT(&l3) >= 3 && pthread_setaffinity_np(pthread_self(), sizeof(l3), &l3) == 0;
  }
  ~Pin() {
    if (on) (void)pthread_setaffinity_np(pthread_self(), sizeof(old_set), &old_set);
  }
};

// The signalled window's feed asks this while a group is not signalled yet.
struct StreamIdle {
  hipStream_t s;
  const SpinQueue* x = nullptr;   // the exchange thread (split exchange): a merge it has not launched yet
  // a faulted walk / merge kernel surfaces as its own HIP error (PE_EHIP with the HIP string),
  // and a failed exchange as its own error, not as the feed's "never signalled"
  static bool stream_busy(hipStream_t s) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipErrorNotReady) return true;
    hipchk(e, "walk window stream");
    return false;
  }
  static bool busy(void* u) {
    auto* t = static_cast<StreamIdle*>(u);
    if (t->x && t->x->failed()) const_cast<SpinQueue*>(t->x)->wait();   // rethrows the exchange's error
    return (t->x && t->x->busy()) || stream_busy(t->s);
  }
};

struct DumpClose {
  FILE*& f;
  ~DumpClose() {
    if (f) std::fclose(f);
  }
};

struct TraceOut {
  int& helper_cpu;
  const bool& on;
  std::vector<double>& a; std::vector<double>& b; std::vector<double>& c;
  std::vector<double>& d; std::vector<double>& e; std::vector<double>& f;
  ~TraceOut() {
    if (!on || a.empty()) return;
    auto pr = [](const char* n, std::vector<double>& v) {
      if (v.empty()) return;
      std::sort(v.begin(), v.end());
      double sum = 0;
      for (double x : v) sum += x;
      std::fprintf(stderr, "%s n %zu sum %.2f ms mean %.1f us p10 %.1f p50 %.1f p90 %.1f max %.1f\n", n, v.size(),
                   sum / 1e3, sum / v.size(), v[v.size() / 10], v[v.size() / 2], v[v.size() * 9 / 10], v.back());
    };
    pr("wait   ", a);
    pr("resolve", b);
    pr("post   ", c);
    pr("xspin  ", d);   // exchange thread: waiting for the ranks' signals, per window
    pr("xmerge ", e);   // exchange thread: merging, per window
    pr("xblock ", f);   // main thread: waiting for the exchange thread before posting
    auto sib = [](int cpu) {
      char path[128], buf[64] = {0};
      std::snprintf(path, sizeof path, "/sys/devices/system/cpu/cpu%d/topology/thread_siblings_list", cpu);
      FILE* f = std::fopen(path, "r");
      if (f) {
        if (!std::fgets(buf, sizeof buf, f)) buf[0] = 0;
        std::fclose(f);
      }
      buf[std::strcspn(buf, "\n")] = 0;
      return std::string(buf);
    };
    const int mc = sched_getcpu();
    std::fprintf(stderr, "cpus: main %d (siblings %s) helper %d (siblings %s)\n", mc, sib(mc).c_str(), helper_cpu,
                 helper_cpu >= 0 ? sib(helper_cpu).c_str() : "-");
  }
};

struct EventsFree {
  std::vector<std::pair<hipEvent_t, hipEvent_t>>& v;
  ~EventsFree() {
    for (auto& p : v) {
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
  }
};

struct XWait {   // every exit: the exchange thread's task is over before the buffers it uses go
  std::unique_ptr<SpinQueue>& w;
  ~XWait() {
    if (w) try {
        w->wait();
      } catch (...) {
      }
  }
};

// A window scanned ahead (the pipelined loop, GreedyRun::run).
struct Flight {
  std::vector<int32_t> groups;
  pe::Cursor end;
  int buf = 0;
  size_t ver = 0;   // updates of the epoch's windows [0, ver) were applied before its scan
};

// One pe_place_greedy call past its set-up: the window protocol of mode m.
// Member order is destruction order reversed, and it matters for the helper threads against the state
// their tasks use: the flights and update sets (fl .. to_scan) go first -- no task is running then, run()
// waits for the launch helper before it lets an error unwind --, then xwait_exit waits for the exchange
// thread's task, then the merge helpers and the exchange thread are joined (xmergers, xworker), the feed
// goes, the launch helper is joined (worker), and only then the
// candidate lists, the walk events (events_free), the trace (trace_out prints) and the dump (dump_close).
// The driver's Pin restores the caller's affinity after all of them.
struct GreedyRun {
  pe_ctx* const ctx;
  const pe::GreedyKnobs kn;
  const pe::GreedyMode m;
  pe::Resolver& R;
  const uint32_t* const group_need;
  pe_host_exchange* const hx;   // the shared-memory exchange (zero-copy windows)
  const hipStream_t s;
  const size_t gb;   // bytes of one group's list in a blob (stride m.K)
  const int Wmax, nwaves;
  int k_win;         // list length walked (changed only while the helper threads are idle)
  const bool async_resort, wev, wflush;
  const int64_t kResortEarly, kResortLate;
  decltype(&pe::launch_merge_shards) const merge_fn;
  // blob buffer b (0: h_out, 1: h_out2, 2-3: h_outx): the windows scanned ahead land in their own
  // buffers while the host still resolves from the current one's; likewise their requests
  HostBuf<uint8_t>* const h_blob[4];
  HostBuf<ReqRec>* const h_req[4];
  uint8_t* outbuf(int b) const { return h_blob[b]->p; }
  uint8_t* outbufdev(int b) const { return h_blob[b]->dev; }
  HostBuf<ReqRec>& hgroups(int b) const { return *h_req[m.signalled ? b : 0]; }   // (unsignalled: one buffer)

  FILE* dump = nullptr;
  DumpClose dump_close{dump};
  int64_t dump_left;
  std::vector<double> tr_wait, tr_res, tr_post, tr_xspin, tr_xmerge, tr_xblock;
  int helper_cpu = -1;
  TraceOut trace_out{helper_cpu, kn.trace, tr_wait, tr_res, tr_post, tr_xspin, tr_xmerge, tr_xblock};
  std::vector<std::pair<hipEvent_t, hipEvent_t>> walk_events;
  EventsFree events_free{walk_events};
  int64_t walk_launch_groups = 0;
  std::vector<pe::GroupCands> cands;
  int cb = 0;   // the blob buffer of the window being resolved
  std::unique_ptr<SpinWorker> worker;
  const Pin& pin;   // (the driver's: the caller's thread is pinned before anything is allocated or registered)
  const uint8_t* last_blob = nullptr;   // the parsed blob of the window being resolved (one list per group
                                        // unless the shards are merged on the host)
  uint32_t buf_gen[4] = {0, 0, 0, 0};
  int buf_k[4];   // the list stride each blob buffer's window was written with
  pe::WindowFeed feed;
  StreamIdle stream_idle;
  // RCCL transport: every wait for the stream is bounded (PE_RCCL_TIMEOUT_S) -- a collective that
  // never completes keeps the stream busy, which the idle test above cannot tell from a slow walk
  const double coll_tmo;
  double feed_spin_seen = 0;   // feed.spin_ms() already counted as device wait
  std::unique_ptr<SpinQueue> xworker;
  std::vector<std::unique_ptr<SpinWorker>> xmergers;
  XWait xwait_exit{xworker};
  // the pipelined loop (run)
  std::deque<Flight> fl;
  std::vector<std::vector<pe::Update>> hist;   // updates of the epoch's resolved windows
  size_t n_app = 0;                             // of which posted for apply
  int next_buf = 0, upd_slot = 0;
  bool posted = false;   // the helper already has this iteration's task (early post)
  std::vector<pe::Update> seed, upd;
  // the helper's next task: previous windows' updates applied, then windows scanned up to D ahead
  std::vector<std::pair<const std::vector<pe::Update>*, int>> to_apply;
  std::vector<Flight*> to_scan;
  Clock::time_point t_setup, t_loop;

  GreedyRun(pe_ctx* c, const GreedyBatch& batch, const pe::GreedyKnobs& knobs, const pe::GreedyMode& mode,
            pe::Resolver& resolver, const Pin& pinned)
      : ctx(c), kn(knobs), m(mode), R(resolver), group_need(batch.group_need),
        hx(pe::hx_is(c->exchange) ? static_cast<pe_host_exchange*>(c->exchange_user) : nullptr), s(c->stream),
        gb(pe::cand_group_bytes(mode.K)), Wmax(c->window_groups),
        nwaves((int)std::max<int64_t>(1, (c->Ns + pe::SC_SPAN - 1) / pe::SC_SPAN)), k_win(mode.K0),
        async_resort(mode.walk && knobs.async_resort), wev(mode.walk && knobs.walk_events),
        wflush(mode.walk && knobs.walk_flush), kResortEarly(std::min<int64_t>(4096, c->resort_nodes / 4)),
        kResortLate(std::max<int64_t>(1, c->resort_nodes / 2)),
        merge_fn(mode.ranked ? &pe::launch_merge_ranked : &pe::launch_merge_shards),
        h_blob{&c->h_out, &c->h_out2, &c->h_outx[0], &c->h_outx[1]},
        h_req{&c->h_groups, &c->h_groups2, &c->h_groupsx[0], &c->h_groupsx[1]}, dump_left(knobs.dump_max),
        pin(pinned), buf_k{mode.K, mode.K, mode.K, mode.K}, stream_idle{c->stream},
        coll_tmo(!mode.use_exchange && c->comm ? rccl_timeout_s() : 0.0) {
    open_dump(batch);
    if (m.pipelined) {
      worker.reset(new SpinWorker(ctx->device));
      if (pin.on) worker->pin(pin.l3);
    }
    if (pin.on) R.pin_helper(pin.l3);
    feed.idle = &StreamIdle::busy;
    feed.idle_user = &stream_idle;
    feed.timeout_s = coll_tmo;
    // a timed-out window starts the communicator's abort where it is detected, before the unwinding
    // (the launch helper's and the events' clean-up) could wait on anything the stuck collective holds
    feed.on_timeout = [](void* u) { rccl_abort(static_cast<pe_ctx*>(u)); };
    feed.timeout_user = ctx;
    if (m.split_x) {
      xworker.reset(new SpinQueue(ctx->device));
      if (pin.on) xworker->pin(pin.l3);
      stream_idle.x = xworker.get();
      if (m.zc_host) {
        for (int t = 1; t < m.T; ++t) {
          xmergers.emplace_back(new SpinWorker(ctx->device));
          if (pin.on) xmergers.back()->pin(pin.l3);
          xmergers.back()->post(&pe::merge_warm);   // (waited for before the first window's share)
        }
        xworker->post(&pe::merge_warm);
      }
    }
  }

  void open_dump(const GreedyBatch& b) {   // PE_DUMP_WINDOWS
    if (!kn.dump_path) return;
    dump = std::fopen(kn.dump_path, "wb");
    if (!dump) return;
    const int64_t hdr[3] = {b.n_jobs, b.G, (int64_t)m.K};   // (the blob stride)
    std::fwrite(hdr, 8, 3, dump);
    std::fwrite(b.job_group_off, 4, (size_t)b.n_jobs + 1, dump);
    std::fwrite(b.priority, 4, (size_t)b.n_jobs, dump);
    std::fwrite(b.group_count, 4, (size_t)b.G, dump);
    std::fwrite(b.group_req, 8, (size_t)b.G * pe::D, dump);
    std::fwrite(b.group_need, 4, (size_t)b.G, dump);
    std::fwrite(&ctx->n_total, 8, 1, dump);   // the host mirror at the batch start
    std::fwrite(ctx->m_nodes.data(), sizeof(pe::NodeState), ctx->m_nodes.size(), dump);
  }

  void sync_stream(const char* what) {
    if (coll_tmo <= 0) return hipchk(hipStreamSynchronize(s), what);
    const auto ts = Clock::now();
    for (unsigned spin = 1;; ++spin) {
      const hipError_t e = hipStreamQuery(s);
      if (e != hipErrorNotReady) return hipchk(e, what);
      if (spin > 64) std::this_thread::sleep_for(std::chrono::microseconds(20));
      if ((spin & 63) == 0 && std::chrono::duration<double>(Clock::now() - ts).count() > coll_tmo) {
        rccl_abort(ctx);   // (at the throw site: see feed.on_timeout)
        throw pe::CollectiveTimeout(std::string(what) + ": the stream did not drain within " +
                                    std::to_string(coll_tmo) +
                                    " s -- a window's all-gather is stuck (a peer stalled or was lost; PE_RCCL_TIMEOUT_S)");
      }
    }
  }

  // merge_shards_kernel's rule on the host: the keys below the smallest shard limit, the K + 1
  // smallest of them (two shards: a branch-free two-way merge); group w of shard r at
  // gath + r * stride + w * gb
  // (W ranks, lists of stride K and gb bytes; Kc: the merged list's length, the window's -- the stride may
  // be longer.  Plain values, no object: the exchange thread and its helpers run this per group)
  static void host_merge_zc(const uint8_t* gath, size_t stride, int w, uint8_t* out, uint32_t gen, int W, int K, int Kc,
                            size_t gb) {
    uint8_t* og = out + (size_t)w * gb;
    uint64_t* dst = reinterpret_cast<uint64_t*>(og + sizeof(pe::CandHdr));
    uint64_t L;
    static_assert(pe::HX_ZC_MAX_WORLD >= pe::RM_MAX_WORLD, "zero-copy merge arrays");
    const uint64_t* lists[pe::HX_ZC_MAX_WORLD];   // (zero-copy windows: world <= HX_ZC_MAX_WORLD)
    int ns[pe::HX_ZC_MAX_WORLD];
    const bool bad = !read_rank_lists(
        W, K, [&](int r) { return gath + (size_t)r * stride + (size_t)w * gb; }, lists, ns, &L);
    uint64_t lim = L;
    const int n = bad ? pe::CAND_CORRUPT : pe::merge_rank_lists(lists, ns, W, L, Kc, dst, &lim);
    pe::CandHdr* hp = reinterpret_cast<pe::CandHdr*>(og);
    hp->n = n;
    hp->limit = bad ? 0 : lim;
    __atomic_store_n(&hp->flags, (int32_t)gen, __ATOMIC_RELEASE);   // the group's signal, last
  }

  // PE_XCHG_HOST_MERGE (xhost_merge): the same rule, a k-way merge of the gathered lists
  void host_merge_group(const uint8_t* gath, int Wg, int w, uint8_t* out, uint32_t gen) {
    const int W = ctx->world, K = m.K;
    std::vector<const uint64_t*>& lists = ctx->x_lists;
    std::vector<int32_t>& ns = ctx->x_ns;
    std::vector<int32_t>& hd = ctx->x_hd;
    lists.resize((size_t)W);
    ns.resize((size_t)W);
    hd.assign((size_t)W, 0);
    uint64_t L;
    const bool bad = !read_rank_lists(
        W, K, [&](int r) { return gath + ((size_t)r * Wg + w) * gb; }, lists.data(), ns.data(), &L);
    uint8_t* og = out + (size_t)w * gb;
    uint64_t* dst = reinterpret_cast<uint64_t*>(og + sizeof(pe::CandHdr));
    int n = bad ? pe::CAND_CORRUPT : 0;
    uint64_t lim = L;
    for (; !bad;) {
      int br = -1;
      uint64_t bk = L;   // (only keys below the smallest limit count)
      for (int r = 0; r < W; ++r)
        if (hd[(size_t)r] < ns[(size_t)r] && lists[(size_t)r][hd[(size_t)r]] < bk) {
          bk = lists[(size_t)r][hd[(size_t)r]];
          br = r;
        }
      if (br < 0) break;
      if (n == K) {   // a (K+1)-th key below the limit: it is the list's limit
        lim = bk;
        break;
      }
      dst[n++] = bk;
      ++hd[(size_t)br];
    }
    pe::CandHdr* hp = reinterpret_cast<pe::CandHdr*>(og);
    hp->n = n;
    hp->limit = lim;
    __atomic_store_n(&hp->flags, (int32_t)gen, __ATOMIC_RELEASE);   // the group's signal, last
  }

  // A host-merged zero-copy window: every rank's lists are in the segment, each group is merged as all
  // ranks signalled it (the exchange thread and its merge helpers)
  void exchange_window_zc(int b, int Wg, uint32_t gen, const pe::HxWindow* hw) {
    const bool trace = kn.trace;
    const double tmo = pe::hx_timeout_s();
    const auto t0 = Clock::now();
    const int T = 1 + (int)xmergers.size();   // the exchange thread + its merge helpers, groups w = t mod T
    const int world = ctx->world, K = m.K, Kc = k_win;   // (locals: read per group by every share)
    const size_t gb = this->gb;
    uint8_t* const out = outbuf(b);
    const hipStream_t s = this->s;
    const size_t pf_bytes = pe::merge_read_bytes(world, Kc, gb);
    // one share of the window: groups t, t + T, ... (waited / merged / spun: this share's times)
    auto share = [&, hw, gen, Wg](int t, double* waited, double* spun, double* merged) {
      for (int w = t; w < Wg; w += T) {
        const auto ts = trace ? Clock::now() : t0;
        for (int r = 0; r < world; ++r) {
          const pe::CandHdr* h = reinterpret_cast<const pe::CandHdr*>(hw->host + (size_t)r * hw->slot + (size_t)w * gb);
          if (__atomic_load_n(&h->flags, __ATOMIC_ACQUIRE) == (int32_t)hw->gen) continue;
          const auto tw = Clock::now();
          for (unsigned spin = 1; __atomic_load_n(&h->flags, __ATOMIC_ACQUIRE) != (int32_t)hw->gen; ++spin) {
            _mm_pause();
            if ((spin & 4095) == 0) {
              if (t == 0) {   // (HIP calls from the exchange thread only) a faulted walk of this rank: its own error
                const hipError_t e = hipStreamQuery(s);
                if (e != hipErrorNotReady) hipchk(e, "walk window stream");
              }
              if (std::chrono::duration<double>(Clock::now() - t0).count() > tmo)
                throw pe::ExchangeError("host exchange: rank " + std::to_string(r) +
                                        "'s candidate lists never arrived (peer stalled or failed; PE_HX_TIMEOUT_S)");
            }
          }
          *waited += ms_since(tw);
        }
        const auto tm = trace ? Clock::now() : t0;
        // this share's next groups on their way from DRAM (the device wrote them past the CPU caches;
        // a line fetched before the device's write is snooped out again, harmless) -- the heads the
        // merge reads, not whole slots -- and the output lines owned for writing
        for (int a = 1; a <= 2 && w + a * T < Wg; ++a) {
          const int wn = w + a * T;
          for (int r = 0; r < world; ++r) {
            const uint8_t* gl = hw->host + (size_t)r * hw->slot + (size_t)wn * gb;
            for (size_t o = 0; o < pf_bytes; o += 64) __builtin_prefetch(gl + o, 0, 3);
          }
          uint8_t* ol = out + (size_t)wn * gb;
          for (size_t o = 0; o < gb; o += 64) __builtin_prefetch(ol + o, 1, 3);
        }
        host_merge_zc(hw->host, hw->slot, w, out, gen, world, K, Kc, gb);
        if (trace) {
          *spun += us(tm - ts);
          *merged += us_since(tm);
        }
      }
    };
    struct Times {
      double waited = 0, spun = 0, merged = 0, busy = 0;   // busy: the share's wall time less its waits
    };
    Times tt[kMaxMergers + 1];
    auto timed_share = [&share](int t, Times* x) {
      const auto a = Clock::now();
      share(t, &x->waited, &x->spun, &x->merged);
      x->busy = ms_since(a) - x->waited;
    };
    for (int t = 1; t < T; ++t) {
      Times* x = &tt[t];
      xmergers[(size_t)t - 1]->wait();   // (the warm-up task, before the first window)
      xmergers[(size_t)t - 1]->post([&timed_share, t, x] { timed_share(t, x); });
    }
    std::exception_ptr err;
    try {
      timed_share(0, &tt[0]);
    } catch (...) {
      err = std::current_exception();
    }
    for (int t = 1; t < T; ++t) try {   // every helper is done with the window before it is released
        xmergers[(size_t)t - 1]->wait();
      } catch (...) {
        if (!err) err = std::current_exception();
      }
    if (err) std::rethrow_exception(err);
    double busy = 0, spun = 0, merged = 0;
    for (int t = 0; t < T; ++t) {
      busy = std::max(busy, tt[t].busy);   // the merge's critical path: the busiest share (they run side by side)
      spun += tt[t].spun;
      merged += tt[t].merged;
    }
    if (trace) {
      tr_xspin.push_back(spun);
      tr_xmerge.push_back(merged);
    }
    const double all_ms = ms_since(t0);
    ctx->stats.xchg_merge_ms += busy;
    ctx->stats.xchg_wait_ms += std::max(0.0, all_ms - busy);   // the rest of the window's exchange: waiting
    pe::hx_zc_consumed(hx, *hw);
  }

  // The host exchange of window b (the exchange thread, the launch helper, or the main thread at a
  // restart): own lists out, every rank's lists in, merged.
  void exchange_window(int b, int Wg, uint32_t gen, bool own_direct, const SpinWorker* launcher,
                       const pe::HxWindow* hw = nullptr) {
    if (m.zc_host) return exchange_window_zc(b, Wg, gen, hw);
    const int K = m.K;
    const size_t bytes = (size_t)Wg * gb;
    if (own_direct && ctx->Ns > 0) {   // every own group signalled: the lists are in h_own
      struct Idle {   // busy while the launcher has not launched the walk yet, or the stream runs
        const SpinWorker* l;
        hipStream_t s;
        static bool busy(void* u) {
          auto* x = static_cast<Idle*>(u);
          return (x->l && x->l->busy()) || StreamIdle::stream_busy(x->s);
        }
      } idle{launcher, s};
      pe::WindowFeed own;
      std::vector<pe::GroupCands> own_cands;
      own.idle = &Idle::busy;
      own.idle_user = &idle;
      own.reset(ctx->h_own.p, Wg, K, gen, &own_cands);
      own.wait((size_t)Wg - 1);
    } else {
      hipchk(hipMemcpyAsync(ctx->h_own.p, ctx->g_out.p, bytes, hipMemcpyDeviceToHost, s), "D2H cands");
      hipchk(hipStreamSynchronize(s), "sync own cands");
    }
    const auto tx = Clock::now();
    if (ctx->exchange(ctx->exchange_user, ctx->h_own.p, m.dev_merge ? ctx->h_xg[b].p : outbuf(b), bytes) != 0)
      raise(PE_ERCCL, "exchange callback failed");
    ctx->stats.xchg_wait_ms += ms_since(tx);
    if (m.xhost_merge) {
      const auto tm = Clock::now();
      for (int w = 0; w < Wg; ++w) host_merge_group(ctx->h_xg[b].p, Wg, w, outbuf(b), gen);
      ctx->stats.xchg_merge_ms += ms_since(tm);
    } else if (m.dev_merge) {   // the gathered lists (pinned) merged on the device, signalled per group
      hipchk(merge_fn(s, ctx->h_xg[b].dev, ctx->world, Wg, K, outbufdev(b), gen, 0, nullptr, true),
             "launch merge_shards");
    }
  }

  // The window's candidate lists on the device, written to dst: the sorted walk (with the index
  // rebuilds it is due), the full scan, or -- an empty shard -- empty lists.
  void launch_lists(const HostBuf<ReqRec>& hg, int b, int Wg, int Kw, uint8_t* dst, uint32_t gen, const pe::HxWindow& hw) {
    const int K = m.K;
    if (m.walk) {   // one 64-B request per block: read from pinned host memory, no H2D copy
      // PE_WALK_SWITCH_DELAY=n (test knob): take a finished rebuild over only after n windows ran
      // with it pending, so the dual overlay writes of those windows' applies are exercised
      if (ctx->w_pending && (ctx->w_est > ctx->resort_nodes + kResortLate ||
                             (ctx->w_pend_windows++ >= kn.switch_delay && hipEventQuery(ctx->w_ev_done) == hipSuccess)))
        walk_switch(ctx);
      if (!ctx->w_pending) {
        if (async_resort && ctx->w_est > ctx->resort_nodes - kResortEarly) walk_resort_async(ctx);
        else if (ctx->w_est > ctx->resort_nodes) walk_resort(ctx);
      }
      std::pair<hipEvent_t, hipEvent_t> evp{nullptr, nullptr};
      if (wflush) hipchk(hipMemsetD32Async((hipDeviceptr_t)ctx->w_flush.p, ctx->walk_gen, (size_t)128 << 20, s), "flush");
      if (wev) {
        hipchk(hipEventCreate(&evp.first), "event");
        hipchk(hipEventCreate(&evp.second), "event");
        walk_events.push_back(evp);
        hipchk(hipEventRecord(evp.first, s), "event record");
      }
      hipchk(pe::launch_walk(s, hg.dev, Wg, k_win, walk_index(ctx), ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns,
                             (uint64_t)ctx->begin, dst, m.zc ? hw.gen : m.direct_out || m.own_direct ? gen : 0u, Kw),
             "launch walk");
      if (wev) hipchk(hipEventRecord(evp.second, s), "event record");
      walk_launch_groups += Wg;
    } else if (ctx->Ns > 0) {
      const int Wgp = (int)round_up(Wg, pe::SC_GT);
      hipchk(hipMemcpyAsync(ctx->g_groups.p, hg.p, Wgp * sizeof(ReqRec), hipMemcpyHostToDevice, s), "H2D window");
      hipchk(pe::launch_scan(s, ctx->res.p, ctx->stride, ctx->labels.p, ctx->g_kn.p, ctx->g_lo.p, ctx->Ns,
                             (uint64_t)ctx->begin, ctx->g_groups.p, Wg, ctx->g_cand.p, ctx->g_cnt.p, ctx->g_bound.p,
                             nwaves),
             "launch scan");
      hipchk(pe::launch_merge(s, ctx->g_cand.p, ctx->g_cnt.p, ctx->g_bound.p, nwaves, K, dst, Wg),
             "launch merge");
    } else if (m.zc) {   // an empty shard: empty lists, signalled in stream order like a walk's
      hipchk(pe::launch_empty_groups(s, Wg, Kw, dst, hw.gen), "launch empty groups");
    } else {
      const size_t gbw = pe::cand_group_bytes(Kw);
      std::vector<uint8_t> empty((size_t)Wg * gbw, 0);
      for (int w = 0; w < Wg; ++w) {
        pe::CandHdr h{0, 0, pe::NO_KEY};
        std::memcpy(empty.data() + (size_t)w * gbw, &h, sizeof(h));
      }
      if (m.direct_out) {
        std::memcpy(outbuf(b), empty.data(), empty.size());
      } else {
        hipchk(hipMemcpyAsync(dst, empty.data(), empty.size(), hipMemcpyHostToDevice, s), "H2D empty");
        hipchk(hipStreamSynchronize(s), "sync empty");
      }
    }
  }

  // ---- one window on the device: group requests H2D, scan, merge, (RCCL all-gather), blob D2H
  // gen_in: the window's generation assigned by the caller (split exchange: the exchange thread
  // must know it before the launch); defer_x: leave the exchange to the exchange thread
  void enqueue_window(const std::vector<int32_t>& groups, int b, uint32_t gen_in = 0, bool defer_x = false,
                      const pe::HxWindow* hw_in = nullptr) {
    const int K = m.K;
    const int Wg = (int)groups.size();
    const int Wgp = (int)round_up(Wg, pe::SC_GT);
    const int Kw = m.rccl_grow ? k_win : K;   // the window's list stride (RCCL: its length, see rccl_grow)
    auto& hg = hgroups(b);
    for (int w = 0; w < Wgp; ++w) {
      const int g = groups[std::min(w, Wg - 1)];
      fill_req(hg.p[w], R.scan_req(g), group_need[g]);   // island groups: count x request
    }
    pe::HxWindow hw;   // zero-copy: this window's slots and their generation (every rank, every window)
    if (m.zc) {
      hw = hw_in ? *hw_in : pe::hx_zc_next(hx);
      if (m.zc_host && !pe::hx_zc_wait_reuse(hx, hw))   // (every rank read the window that used the slots)
        throw pe::ExchangeError("host exchange: a rank never finished reading a window (peer stalled or failed)");
    }
    // unsharded: the kernel writes the blob straight into pinned host memory (no D2H copy); so does
    // a pipelined host exchange's walk (its own lists, signalled per group: no D2H, no stream sync)
    uint8_t* const dst = m.zc           ? hw.dev + (size_t)ctx->rank * hw.slot
                         : m.direct_out ? outbufdev(b)
                         : m.own_direct ? ctx->h_own.dev
                                        : ctx->g_out.p;
    uint32_t gen = 0;   // signalled window: its generation (the walk's or the shard merge's)
    if (gen_in) gen = gen_in;
    else if (m.signalled || m.own_direct) gen = next_gen(ctx);
    buf_gen[b] = gen;
    buf_k[b] = Kw;
    launch_lists(hg, b, Wg, Kw, dst, gen, hw);
    const size_t bytes = (size_t)Wg * pe::cand_group_bytes(Kw);
    if (m.direct_out) {
      // written in place
    } else if (m.zc_host) {   // the exchange thread (or, not deferred, this thread) merges on the host
      ctx->stats.xchg_zc_windows += 1;
      if (!defer_x) exchange_window(b, Wg, gen, false, nullptr, &hw);
    } else if (m.zc) {   // merged once every rank's walk signalled every group (pe_hostx.h)
      ctx->stats.xchg_zc_windows += 1;
      hipchk(pe::launch_xwait(s, hw.dev, ctx->world, Wg, K, (int64_t)hw.slot, hw.gen, kn.zc_ticks, ctx->g_xstatus.p),
             "launch exchange wait");
      hipchk(merge_fn(s, hw.dev, ctx->world, Wg, K, outbufdev(b), gen, (int64_t)hw.slot,
                                     ctx->g_xstatus.p, true),
             "launch merge_shards");
    } else if (m.use_exchange) {
      if (!m.pipelined)
        hipchk(hipMemcpyAsync(ctx->h_own.p, ctx->g_out.p, bytes, hipMemcpyDeviceToHost, s), "D2H cands");
      else if (!defer_x)   // (the launch helper, or the main thread at a restart) exchange now
        exchange_window(b, Wg, gen, m.own_direct, nullptr);
    } else {
      if (kn.stall_window >= 0 && ctx->stats.windows == kn.stall_window && kn.stall_ticks > 0)
        hipchk(pe::launch_stall(s, kn.stall_ticks), "launch stall (test knob)");
      ncclchk(ncclAllGather(ctx->g_out.p, ctx->g_gath.p, bytes, ncclUint8, ctx->comm, s), "ncclAllGather");
      if (m.dev_merge)
        hipchk(merge_fn(s, ctx->g_gath.p, ctx->world, Wg, Kw, outbufdev(b), gen, 0, nullptr, false),   // (device lists)
               "launch merge_shards");
      else
        hipchk(hipMemcpyAsync(outbuf(b), ctx->g_gath.p, bytes * ctx->world, hipMemcpyDeviceToHost, s),
               "D2H gathered");
    }
    ctx->stats.windows += 1;
    ctx->stats.groups_scanned += Wg;
    if (!m.walk) ctx->stats.scan_evals += (int64_t)Wg * ctx->Ns;
  }

  // ---- wait for the window's blob (and run the host exchange when one is configured), parse it
  void collect_window(const std::vector<int32_t>& groups, int b) {
    const int Wg = (int)groups.size();
    const size_t bytes = (size_t)Wg * gb;
    const auto tw = Clock::now();
    if (m.signalled && buf_gen[b] != 0) {   // the first group's list (and so every earlier launch) is done
      last_blob = outbuf(b);
      feed.reset(outbuf(b), Wg, buf_k[b], buf_gen[b], &cands);
      feed.wait(0);
      feed_spin_seen = feed.spin_ms();
      const auto th = Clock::now();
      ctx->stats.greedy_wait_ms += ms(th - tw);
      if (kn.trace) tr_wait.push_back(us(th - tw));
      return;
    }
    sync_stream("sync window");
    last_blob = outbuf(b);
    if (m.use_exchange && !m.pipelined) {
      const auto tx = Clock::now();
      if (ctx->exchange(ctx->exchange_user, ctx->h_own.p, outbuf(b), bytes) != 0)
        raise(PE_ERCCL, "exchange callback failed");
      ctx->stats.xchg_wait_ms += ms_since(tx);
      if (m.dev_merge) {   // the gathered blob (pinned) merged by the device into h_merged
        hipchk(merge_fn(s, outbufdev(b), ctx->world, Wg, m.K, ctx->h_merged.dev, 0u, 0, nullptr, true),
               "launch merge_shards");
        sync_stream("sync merge");
        last_blob = ctx->h_merged.p;
      }
    }
    const auto th = Clock::now();
    ctx->stats.greedy_wait_ms += ms(th - tw);
    if (kn.trace) tr_wait.push_back(us(th - tw));
    pe::parse_window_keys(last_blob, m.dev_merge ? 1 : ctx->world, Wg, buf_k[b], cands);   // lists point into the blob

    ctx->stats.greedy_host_ms += ms_since(th);
  }

  // ---- residual updates of this shard: the apply kernel reads the records from pinned staging
  //      slot `slot` (no H2D copy); a slot is rewritten only once a later launch is known to have
  //      started (a signalled group seen, or a stream sync) -- the pipelined loop below rotates D
  void enqueue_apply(const std::vector<pe::Update>& updates, int slot) {
    int64_t nu = 0;
    HostBuf<int64_t>& hu = slot == 0 ? ctx->h_upd : ctx->h_updx[slot - 1];
    hipchk(hu.ensure(std::max<size_t>(updates.size(), 1) * (pe::D + 1), kZeroCopy), "alloc pinned upd");
    for (const pe::Update& u : updates) {
      if (u.gid < ctx->begin || u.gid >= ctx->end) continue;
      int64_t* o = hu.p + nu * (pe::D + 1);
      o[0] = u.gid - ctx->begin;
      for (int d = 0; d < pe::D; ++d) o[1 + d] = u.res[d];
      ++nu;
    }
    if (nu > 0) {   // the kernel reads the pinned records directly (no H2D copy)
      const pe::WalkIndex w = walk_index(ctx);
      const pe::WalkIndex wn = walk_index(ctx, 1 - ctx->w_cur);   // (read only while a rebuild is pending)
      hipchk(pe::launch_apply(s, ctx->res.p, ctx->stride, hu.dev, nu, (uint64_t)ctx->begin, ctx->g_kn.p,
                              ctx->g_lo.p, ctx->labels.p, m.walk ? &w : nullptr,
                              m.walk && ctx->w_pending ? &wn : nullptr),
             "launch apply");
      ctx->w_est += nu;
      if (ctx->w_pending) {
        ctx->w_pend_est += nu;
        ctx->stats.walk_pend_updates += nu;   // applied into both index sets' overlays
      }
    }
  }

  bool timed_resolve(const std::vector<int32_t>& groups, std::vector<pe::Update>& updates,
                     const std::vector<pe::Update>* seeds) {
    if (dump && dump_left-- == 0) {   // PE_DUMP_MAX_WINDOWS reached
      std::fclose(dump);
      dump = nullptr;
    }
    if (dump) {   // {Wg, groups, blob, n_seed, seeds}: what this resolve call reads
      if (m.signalled) feed.wait(groups.size() - 1);   // (diagnostics: the whole blob first)
      const int32_t wg = (int32_t)groups.size(), ns = seeds ? (int32_t)seeds->size() : 0;
      std::fwrite(&wg, 4, 1, dump);
      std::fwrite(groups.data(), 4, (size_t)wg, dump);
      std::fwrite(last_blob, 1, (size_t)wg * gb * (m.dev_merge || m.direct_out ? 1 : ctx->world), dump);
      std::fwrite(&ns, 4, 1, dump);
      if (ns) std::fwrite(seeds->data(), sizeof(pe::Update), (size_t)ns, dump);
    }
    const auto th = Clock::now();
    updates.clear();
    const bool fed = m.signalled && buf_gen[cb] != 0;
    const bool consumed = R.resolve(groups, cands, updates, seeds, fed ? &feed : nullptr);
    // time the resolver spent blocked on groups not yet signalled is device wait, not host work
    const double spun = fed ? feed.spin_ms() - feed_spin_seen : 0.0;
    if (kn.trace) tr_res.push_back(us_since(th) - spun * 1e3);
    for (const pe::Update& u : updates)          // the mirror follows every placement (all shards)
      for (int d = 0; d < pe::D; ++d) ctx->m_nodes[u.gid].res[d] = u.res[d];
    ctx->stats.greedy_host_ms += ms_since(th) - spun;
    ctx->stats.greedy_wait_ms += spun;
    return consumed;
  }

  Flight* add_flight(const pe::Cursor& from) {   // main thread; nullptr: no window left
    Flight f;
    R.next_window_from(from, Wmax, ctx->window_pods, f.groups, &f.end);
    if (f.groups.empty()) return nullptr;
    f.buf = next_buf;
    next_buf = (next_buf + 1) % m.nbuf;
    f.ver = hist.size();
    fl.push_back(std::move(f));
    return &fl.back();
  }

  void restart() {   // nothing in flight, every update applied: a fresh epoch at the cursor
    fl.clear();
    hist.clear();
    n_app = 0;
    next_buf = 0;
    Flight* f = add_flight(R.cursor());
    if (!f) return;
    if (m.split_x && m.zc_host) {
      // a zero-copy window: merged group by group on the exchange thread as in the loop below, so
      // the resolver starts on the first merged group (merging the whole window here first put the
      // walk's tail and the full merge in front of every batch start and every rescan)
      const uint32_t gen = next_gen(ctx);
      const pe::HxWindow hw = pe::hx_zc_next(hx);
      enqueue_window(f->groups, f->buf, gen, true, &hw);
      const int b = f->buf, wg = (int)f->groups.size();
      xworker->post([this, b, wg, gen, hw] { exchange_window(b, wg, gen, true, worker.get(), &hw); });
    } else {
      enqueue_window(f->groups, f->buf);
    }
  }

  void plan_post() {
    to_apply.clear();
    to_scan.clear();
    for (; n_app < hist.size(); ++n_app) {
      to_apply.emplace_back(&hist[n_app], upd_slot);
      upd_slot = (upd_slot + 1) % m.upd_slots;
    }
    while ((int)fl.size() < m.depth + 1)
      if (Flight* f = add_flight(fl.back().end)) to_scan.push_back(f);
      else break;
  }

  void post_scan() {   // (the non-split helper task)
    worker->post([this, to_apply = to_apply, to_scan = to_scan] {
      const auto tp = Clock::now();
      if (kn.trace) helper_cpu = sched_getcpu();
      for (const auto& a : to_apply) enqueue_apply(*a.first, a.second);
      for (Flight* f : to_scan) enqueue_window(f->groups, f->buf);
      if (kn.trace) tr_post.push_back(us_since(tp));
    });
  }

  // The split exchange's tasks of one iteration: the launch helper applies and launches the walks,
  // the exchange thread exchanges (and merges) the windows behind them.
  void post_split() {
    plan_post();
    // generations assigned here, in launch order: the exchange thread waits for these windows' own
    // lists (signalled with them) while the launch helper launches the walks
    // (zero-copy: the windows' slots too, taken in the same order on every rank)
    struct XWin {
      int buf, wg;
      uint32_t gen;
      pe::HxWindow hw;
    };
    std::vector<XWin> xs;
    std::vector<std::pair<Flight*, XWin>> ws;
    for (Flight* f : to_scan) {
      const uint32_t gen = next_gen(ctx);
      xs.push_back(XWin{f->buf, (int)f->groups.size(), gen, m.zc_host ? pe::hx_zc_next(hx) : pe::HxWindow{}});
      ws.emplace_back(f, xs.back());
    }
    const auto txb = Clock::now();
    // (the copying exchange: the previous window's exchange is over before the next one, its
    // buffers are shared; host-merged zero-copy windows queue up -- slot reuse is counted)
    if (!m.zc_host) xworker->wait();
    if (kn.trace) tr_xblock.push_back(us_since(txb));
    worker->post([this, to_apply = to_apply, ws] {
      const auto tp = Clock::now();
      if (kn.trace) helper_cpu = sched_getcpu();
      for (const auto& a : to_apply) enqueue_apply(*a.first, a.second);
      for (const auto& w : ws)
        enqueue_window(w.first->groups, w.first->buf, w.second.gen, true, m.zc_host ? &w.second.hw : nullptr);
      if (kn.trace) tr_post.push_back(us_since(tp));
    });
    xworker->post([this, xs] {
      for (const XWin& x : xs) exchange_window(x.buf, x.wg, x.gen, true, worker.get(), m.zc_host ? &x.hw : nullptr);
    });
  }

  // Pipelined (exact), depth D: while the host resolves window i, the device holds windows
  // i+1 .. i+D scanned (or scanning), each speculating that the windows before it are consumed.  A
  // window scanned after the updates of the epoch's windows < v were applied misses the changes of
  // windows v .. i-1, which its resolution takes as dirty seeds (their current states are known
  // here).  Each iteration the helper thread applies the previous window's updates and scans the
  // window D ahead into the next free buffer.  A window cut short, or a cursor that did not land
  // where the speculation started, syncs, applies everything and restarts from the cursor.
  // Staging-buffer reuse: the apply posted in iteration j is followed, in the same post, by the
  // scan of window j + D; the slot is written again in iteration j + D, when that window's first
  // group has been seen, i.e. after every earlier launch of the stream finished (with the early post,
  // two slots: see GreedyMode::early_post).  Blob / request buffer b is reused D + 1 windows later,
  // after the windows in between were resolved.
  void run() {
    t_setup = Clock::now();
    restart();
    while (!fl.empty()) {
      Flight& cur = fl.front();
      cb = cur.buf;
      collect_window(cur.groups, cur.buf);       // cur's lists: snapshot = device state at its launch
      if (!m.pipelined) {
        if (!timed_resolve(cur.groups, upd, nullptr)) k_win = m.K;
        enqueue_apply(upd, 0);
        if (R.done()) break;
        fl.clear();
        next_buf = 0;
        if (Flight* f = add_flight(R.cursor())) enqueue_window(f->groups, f->buf);
        continue;
      }
      if (posted) {
        posted = false;
      } else if (m.split_x) {
        post_split();
      } else {
        plan_post();
        post_scan();
      }
      // seeds: the changes of the windows resolved since cur's scan (later states overwrite)
      seed.clear();
      for (size_t k = cur.ver; k < hist.size(); ++k) seed.insert(seed.end(), hist[k].begin(), hist[k].end());
      bool consumed = false;
      try {
        consumed = timed_resolve(cur.groups, upd, &seed);
      } catch (...) {
        // the helper task still reads the flights and update sets: let it finish before the
        // unwinding frees them, then report the resolver's error (the helper's is secondary)
        try {
          worker->wait();
        } catch (...) {
        }
        if (xworker) xworker->wait();   // (a failed exchange is the cause: its error wins)
        throw;
      }
      worker->wait();
      const bool landed = consumed && R.cursor() == cur.end && fl.size() > 1;
      if (landed && !R.done()) {
        hist.push_back(std::move(upd));
        upd = {};
        fl.pop_front();
        if (m.early_post) {   // the next iteration's task, now
          plan_post();
          post_scan();
          posted = true;
        }
        continue;
      }
      // done, or speculation dropped: finish the device work, apply what is left, in order (one
      // launch per window: a node may be in several windows' updates)
      if (xworker) xworker->wait();   // (its merge launch first: it is stream work too)
      sync_stream("sync speculative");
      for (; n_app < hist.size(); ++n_app) {   // (depth > 1 only; slot 0 is rewritten after each)
        enqueue_apply(hist[n_app], 0);
        sync_stream("sync apply");
      }
      enqueue_apply(upd, 0);
      if (R.done()) break;
      if (!consumed) k_win = m.K;   // lists ran out: longer ones from here (the helper is idle now)
      restart();
    }
    t_loop = Clock::now();
    if (xworker) xworker->wait();
    sync_stream("sync greedy");
    walk_drop_pending(ctx);   // (the next call rebuilds in line anyway)
  }

  void walk_stats() {
    if (!m.walk) return;
    unsigned long long wc[2] = {0, 0};
    hipchk(hipMemcpy(wc, ctx->w_stat.p, sizeof(wc), hipMemcpyDeviceToHost), "D2H walk counters");
    ctx->stats.walk_rounds += (int64_t)wc[0];
    ctx->stats.walk_overlay += (int64_t)wc[1];
    ctx->stats.walk_groups += walk_launch_groups;
    ctx->stats.walk_prepass += walk_launch_groups * ((ctx->Ns + pe::WK_ROUND - 1) / pe::WK_ROUND);
    for (auto& p : walk_events) {
      float t = 0.f;
      hipchk(hipEventElapsedTime(&t, p.first, p.second), "event elapsed");
      ctx->stats.walk_ms += t;
    }
  }
};

// The caller's arrays checked; sets b.G and returns the batch's number of pods.
int64_t check_batch(GreedyBatch& b, const int32_t* out_pod_node, const int32_t* out_job_status) {
  need_ptr(b.job_group_off, "job_group_off");
  need_ptr(b.priority, "priority");
  need_ptr(out_job_status, "out_job_status");
  check_offsets(b.job_group_off, b.n_jobs, -1, "job_group_off");
  b.G = b.job_group_off[b.n_jobs];
  int64_t P = 0;
  if (b.G > 0) {
    need_ptr(b.group_count, "group_count");
    need_ptr(b.group_req, "group_req");
    check_req(b.group_req, b.G, "group_req");
    for (int64_t g = 0; g < b.G; ++g) {
      if (b.group_count[g] < 0) raise(PE_EINVAL, "negative group_count");
      P += b.group_count[g];
    }
  }
  if (P > 0) need_ptr(out_pod_node, "out_pod_node");
  return P;
}

// The shard's node keys and walk index over the current residuals, queued on the stream.
void prep_device(pe_ctx* ctx) {
  hipchk(ctx->g_kn.ensure((size_t)std::max<int64_t>(ctx->stride, 1)), "alloc node keys");
  hipchk(ctx->g_lo.ensure((size_t)2 * std::max<int64_t>(ctx->stride, 1)), "alloc node lows");
  // residuals may have changed since the last call (reset, pe_update_nodes): one pass over the shard
  hipchk(pe::launch_prep_nodes(ctx->stream, ctx->res.p, ctx->stride, ctx->Ns, (uint64_t)ctx->begin, ctx->g_kn.p,
                               ctx->g_lo.p),
         "launch prep_nodes");
  hipchk(ctx->w_stat.ensure(2), "alloc walk counters");
  hipchk(hipMemsetAsync(ctx->w_stat.p, 0, 2 * sizeof(unsigned long long), ctx->stream), "memset walk counters");
  if (ctx->walk && ctx->Ns > 0) walk_resort(ctx);
}

pe::GreedyFacts greedy_facts(const pe_ctx* ctx) {
  pe::GreedyFacts f;
  f.world = ctx->world;
  f.rank = ctx->rank;
  f.has_comm = ctx->comm != nullptr;
  f.has_exchange = ctx->exchange != nullptr;
  f.hx = pe::hx_is(ctx->exchange);
  f.hx_slot_bytes = f.hx ? pe::hx_slot_bytes(static_cast<const pe_host_exchange*>(ctx->exchange_user)) : 0;
  f.ctx_walk = ctx->walk;
  f.has_nodes = ctx->Ns > 0;
  f.pipeline = ctx->pipeline;
  f.topk = ctx->topk;
  f.window_groups = ctx->window_groups;
  return f;
}

// The ranks' agreement on the zero-copy use of the shared-memory exchange, once per context and segment:
// each says whether it could register the segment and its slots hold a window (lists of stride K).
bool zc_agreed(pe_ctx* ctx, int K) {
  pe_host_exchange* const hx = static_cast<pe_host_exchange*>(ctx->exchange_user);
  if (ctx->zc_hx != hx) {
    const uint8_t ok = ctx->world <= pe::HX_ZC_MAX_WORLD && pe::hx_zc_register(hx) &&
                               (size_t)ctx->window_groups * pe::cand_group_bytes(K) <= pe::hx_slot_bytes(hx) ? 1 : 0;
    std::vector<uint8_t> all((size_t)ctx->world, 0);
    if (ctx->exchange(ctx->exchange_user, &ok, all.data(), 1) != 0) raise(PE_ERCCL, "exchange callback failed");
    ctx->zc_ok = std::all_of(all.begin(), all.end(), [](uint8_t v) { return v == 1; });
    ctx->zc_hx = hx;
  }
  return ctx->zc_ok;
}

// The call's device and pinned buffers (they grow and are reused).
void size_buffers(pe_ctx* ctx, const pe::GreedyKnobs& kn, const pe::GreedyMode& m) {
  const size_t gb = pe::cand_group_bytes(m.K);
  const int Wmax = ctx->window_groups;
  const int Wpad = (int)round_up(Wmax, pe::SC_GT);
  const int nwaves = (int)std::max<int64_t>(1, (ctx->Ns + pe::SC_SPAN - 1) / pe::SC_SPAN);
  hipchk(ctx->g_groups.ensure(Wpad), "alloc groups");
  hipchk(ctx->h_groups.ensure(Wpad, kZeroCopy), "alloc pinned groups");
  hipchk(ctx->g_cand.ensure((size_t)Wpad * nwaves * 64), "alloc cand");
  hipchk(ctx->g_cnt.ensure((size_t)Wpad * nwaves), "alloc cnt");
  hipchk(ctx->g_bound.ensure((size_t)Wpad * nwaves), "alloc bound");
  hipchk(ctx->g_out.ensure((size_t)Wmax * gb), "alloc out");
  hipchk(ctx->h_out.ensure((size_t)Wmax * gb * ctx->world, kZeroCopy), "alloc pinned out");
  if (m.pipelined) hipchk(ctx->h_out2.ensure((size_t)Wmax * gb * ctx->world, kZeroCopy), "alloc pinned out");
  if (ctx->world > 1 || ctx->comm) {
    hipchk(ctx->g_gath.ensure((size_t)Wmax * gb * ctx->world), "alloc gather");
    hipchk(ctx->h_own.ensure((size_t)Wmax * gb, kZeroCopy), "alloc pinned own");
  }
  if (m.walk && kn.walk_flush) hipchk(ctx->w_flush.ensure((size_t)512 << 20), "alloc flush buffer");
  if (m.zc) hipchk(ctx->g_xstatus.ensure(1), "alloc exchange status");
  if (m.signalled) hipchk(ctx->h_groups2.ensure(Wpad, kZeroCopy), "alloc pinned groups");
  for (int b = 2; b <= m.depth; ++b) {
    hipchk(ctx->h_groupsx[b - 2].ensure(Wpad, kZeroCopy), "alloc pinned groups");
    hipchk(ctx->h_outx[b - 2].ensure((size_t)Wmax * gb * ctx->world, kZeroCopy), "alloc pinned out");
  }
  if (m.dev_merge && m.use_exchange && !m.pipelined)
    hipchk(ctx->h_merged.ensure((size_t)Wmax * gb, kZeroCopy), "alloc pinned merged");
  if (m.dev_merge && m.use_exchange && m.pipelined)
    for (int b = 0; b <= std::max(m.depth, 1); ++b)
      hipchk(ctx->h_xg[b].ensure((size_t)Wmax * gb * ctx->world, kZeroCopy), "alloc pinned gathered");
}

}  // namespace

extern "C" {

int pe_place_greedy(pe_ctx* ctx, int64_t n_jobs, const int32_t* job_group_off, const int32_t* priority,
                    const int32_t* group_count, const int64_t* group_req, const uint32_t* group_need,
                    int32_t* out_pod_node, int32_t* out_job_status) {
  return guarded(ctx, [&]() -> int {
    const auto t0 = Clock::now();
    if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
    if (ctx->comm_aborted)
      raise(PE_ERCCL, "the RCCL communicator was aborted after a window's all-gather timed out; recreate the context");
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (n_jobs == 0) return PE_OK;
    GreedyBatch batch{n_jobs, 0, job_group_off, priority, group_count, group_req, group_need};
    const int64_t P = check_batch(batch, out_pod_node, out_job_status);
    std::vector<uint32_t> no_need;
    if (!batch.group_need) {
      no_need.assign((size_t)std::max<int64_t>(batch.G, 1), 0u);
      batch.group_need = group_need = no_need.data();
    }
    prep_device(ctx);   // (asynchronous: it runs while the host builds the resolver)
    const auto t_prep = Clock::now();
    // one resolver per context, reset per batch (its arrays and seed helper thread are reused)
    if (ctx->resolver) ctx->resolver->reset(n_jobs, job_group_off, priority, group_count, group_req, group_need);
    else ctx->resolver.reset(new pe::Resolver(n_jobs, job_group_off, priority, group_count, group_req, group_need));
    pe::Resolver& R = *ctx->resolver;
    R.set_mirror(pe::Mirror{ctx->m_nodes.data(), ctx->n_total});
    const auto t_res = Clock::now();

    // which protocol this call runs (pe_greedy_mode.h)
    const pe::GreedyKnobs kn = pe::GreedyKnobs::from_env();
    // pinned first: what the call allocates and registers from here on (first call: the pinned buffers,
    // the shared-memory segment) is touched on the CPUs this rank then runs on
    const Pin pin(kn.no_pin, ctx->rank, ctx->world, ctx->pin_cpu);
    const pe::GreedyFacts facts = greedy_facts(ctx);
    const bool zc = pe::greedy_zc_wanted(facts, kn, kLimits) && zc_agreed(ctx, pe::greedy_mode_base(facts, kn, kLimits).K);
    const pe::GreedyMode m = pe::greedy_mode(facts, kn, kLimits, zc);
    size_buffers(ctx, kn, m);

    GreedyRun run(ctx, batch, kn, m, R, pin);
    run.run();
    run.walk_stats();
    if (P > 0) std::memcpy(out_pod_node, R.pod_node().data(), (size_t)P * 4);
    std::memcpy(out_job_status, R.job_status().data(), (size_t)n_jobs * 4);
    ctx->stats.rescans += R.rescans();
    ctx->stats.pods_placed += R.pods_placed();
    ctx->stats.jobs_placed += R.jobs_placed();
    ctx->stats.jobs_failed += R.jobs_failed();
    ctx->stats.last_greedy_ms = ms_since(t0);
    if (kn.trace)
      std::fprintf(stderr, "greedy phases (us): checks+prep %.0f resolver %.0f setup %.0f loop %.0f tail %.0f\n",
                   us(t_prep - t0), us(t_res - t_prep), us(run.t_setup - t_res), us(run.t_loop - run.t_setup),
                   us_since(run.t_loop));
    return PE_OK;
  });
}

}  // extern "C"
