// Which protocol one pe_place_greedy call runs: its environment knobs (GreedyKnobs, read once per call),
// what it reads from the context (GreedyFacts) and everything derived from the two (GreedyMode).  No HIP
// or RCCL here: the decision is plain arithmetic, tested on the CPU (tests/cpp/test_greedy_mode.cc); the
// kernel geometry it needs is passed in (GreedyLimits, filled from pe_kernels.h by pe_engine_greedy.cpp).
//
// Two steps, because the ranks of a shared-memory exchange agree on its zero-copy use with one exchange
// round in between: greedy_zc_wanted(facts, knobs) says whether this rank asks for it, greedy_mode(facts,
// knobs, zc) takes the agreed answer.  Of all of this only zero-copy and the list growth are agreed on by
// the ranks (growth: by construction, it depends on nothing a rank holds alone); every other knob that
// feeds greedy_mode must be set alike on every rank of a sharded run.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

namespace pe {

// Kernel geometry the decision depends on (pe_kernels.h, which needs HIP; kMaxMergers of pe_ctx.h).
struct GreedyLimits {
  int wk_round, mg_cap, mg_threads, rm_max_world;   // WK_ROUND, MG_CAP, MG_THREADS, RM_MAX_WORLD
  size_t rm_max_lds;                                // RM_MAX_LDS
  int max_mergers;                                  // kMaxMergers
  size_t (*cand_group_bytes)(int K);
  size_t (*merge_ranked_lds)(int world, int K);
};

// Every environment variable pe_place_greedy reads (A/B, diagnostics and test knobs; read per call: tests
// flip them between calls of one process).
struct GreedyKnobs {
  // PE_NO_LIST_GROWTH=1 keeps topk throughout on an UNSHARDED context (A/B) -- a per-process variable
  // cannot steer sharded ranks, which must agree on the stride.
  bool no_list_growth = false;
  // PE_ASYNC_RESORT=0: rebuild the walk index in line, on the main stream (A/B).  Otherwise the rebuild
  // starts kResortEarly updates before the threshold on the side stream and is taken over once done --
  // or waited for past kResortLate updates over the threshold.
  bool async_resort = true;
  // PE_WALK_SWITCH_DELAY=n (test knob): take a finished rebuild over only after n windows ran with it
  // pending, so the dual overlay writes of those windows' applies are exercised
  int64_t switch_delay = 0;
  // PE_DUMP_WINDOWS=<file>: record the batch and every window's groups + blob (host resolver replay,
  // tools/replay_resolver.cc), PE_DUMP_MAX_WINDOWS of them at most; diagnostics only
  const char* dump_path = nullptr;
  int64_t dump_max = INT64_MAX;
  // PE_GREEDY_TRACE=1: per-window wait / resolve / post times, summarised on stderr (diagnostics)
  bool trace = false;
  // PE_WALK_EVENTS=1: hipEvents around every walk launch, summed into stats.walk_ms (diagnostics: the
  // greedy roofline of bench.py; the events cost a few us of host time per window)
  bool walk_events = false;
  // PE_WALK_FLUSH=1 (diagnostics, with PE_WALK_EVENTS: the COLD-cache greedy roofline): before every
  // walk launch a 512 MiB device buffer is rewritten, evicting the walk index (sorted keys, residual
  // copy, round summaries: ~50 MB at 1M nodes) from L2 and the 256 MiB Infinity Cache, so the walk
  // reads come from HBM.  The fill is outside the walk's events.
  bool walk_flush = false;
  bool no_pin = false;            // PE_NO_PIN=1: the call's threads are not pinned to one L3 domain
  bool host_merge = false;        // PE_HOST_MERGE=1: see GreedyMode::dev_merge
  bool merge_ranked = false;      // PE_MERGE_RANKED=1 / PE_MERGE_SORT=1: see GreedyMode::ranked
  bool merge_sort = false;
  bool no_group_signal = false;   // PE_NO_GROUP_SIGNAL=1: see GreedyMode::signalled
  bool no_zc_exchange = false;    // PE_NO_ZC_EXCHANGE=1 (every rank): the copying exchange, see GreedyMode::zc
  int pipe_depth = 1;             // PE_PIPE_DEPTH (1..3): see GreedyMode::depth
  // PE_TEST_STALL_WINDOW=n, PE_TEST_STALL_MS=m (test knob, RCCL transport): a one-thread kernel that
  // holds the stream for m ms (wall clock, bounded) is queued right before window n's all-gather --
  // a stand-in for a collective whose peer is gone
  int64_t stall_window = -1;
  int64_t stall_ticks = 0;   // wall_clock64: 100 MHz; at most 30 s
  // a rank whose peer stalls: its device wait of a zero-copy window gives up after PE_HX_GPU_TIMEOUT_S
  // (default 60) and the resolver raises (the merged lists come back with n = -1), the GPU is not held
  int64_t zc_ticks = (int64_t)(60.0 * 1e8);   // wall_clock64: 100 MHz
  bool zc_dev_merge = false;        // PE_ZC_DEV_MERGE=1 (A/B): see GreedyMode::zc_dev
  bool no_split_exchange = false;   // PE_NO_SPLIT_EXCHANGE=1: see GreedyMode::split_x
  bool xchg_threads_set = false;    // PE_XCHG_THREADS: see GreedyMode::T (clamped there: 1..kMaxMergers + 1)
  int xchg_threads = 0;
  bool xchg_host_merge = false;     // PE_XCHG_HOST_MERGE=1 (A/B): see GreedyMode::xhost_merge
  bool early_post = true;           // PE_EARLY_POST=0: off (A/B), see GreedyMode::early_post

  static GreedyKnobs from_env() {
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    auto not_zero = [](const char* name) {   // off only when set and atoi == 0
      const char* e = std::getenv(name);
      return !(e && std::atoi(e) == 0);
    };
    GreedyKnobs k;
    k.no_list_growth = set("PE_NO_LIST_GROWTH");
    k.async_resort = not_zero("PE_ASYNC_RESORT");
    if (const char* e = std::getenv("PE_WALK_SWITCH_DELAY")) k.switch_delay = std::atoll(e);
    k.dump_path = std::getenv("PE_DUMP_WINDOWS");
    if (const char* e = std::getenv("PE_DUMP_MAX_WINDOWS")) k.dump_max = std::atoll(e);
    k.trace = set("PE_GREEDY_TRACE");
    k.walk_events = set("PE_WALK_EVENTS");
    k.walk_flush = set("PE_WALK_FLUSH");
    k.no_pin = set("PE_NO_PIN");
    k.host_merge = set("PE_HOST_MERGE");
    k.merge_ranked = set("PE_MERGE_RANKED");
    k.merge_sort = set("PE_MERGE_SORT");
    k.no_group_signal = set("PE_NO_GROUP_SIGNAL");
    k.no_zc_exchange = set("PE_NO_ZC_EXCHANGE");
    if (const char* e = std::getenv("PE_PIPE_DEPTH")) k.pipe_depth = std::min(3, std::max(1, std::atoi(e)));
    if (const char* e = std::getenv("PE_TEST_STALL_WINDOW")) k.stall_window = std::atoll(e);
    if (const char* e = std::getenv("PE_TEST_STALL_MS"))
      k.stall_ticks = (int64_t)(std::min(std::max(std::atof(e), 0.0), 30000.0) * 1e5);
    if (const char* e = std::getenv("PE_HX_GPU_TIMEOUT_S")) {
      const double t = std::atof(e);
      k.zc_ticks = (int64_t)((t > 0 ? t : 60.0) * 1e8);
    }
    k.zc_dev_merge = set("PE_ZC_DEV_MERGE");
    k.no_split_exchange = set("PE_NO_SPLIT_EXCHANGE");
    if (const char* e = std::getenv("PE_XCHG_THREADS")) {
      k.xchg_threads_set = true;
      k.xchg_threads = std::atoi(e);
    }
    k.xchg_host_merge = set("PE_XCHG_HOST_MERGE");
    k.early_post = not_zero("PE_EARLY_POST");
    return k;
  }
};

// What the decision reads from the context.
struct GreedyFacts {
  int world = 1, rank = 0;
  bool has_comm = false;       // an RCCL communicator
  bool has_exchange = false;   // an exchange callback
  bool hx = false;             // ... which is the shared-memory exchange (pe_hostx.h)
  size_t hx_slot_bytes = 0;    // its slot size (hx only)
  bool ctx_walk = true;        // ctx->walk
  bool has_nodes = true;       // Ns > 0: this rank's shard is not empty
  bool pipeline = true;
  int topk = 256, window_groups = 112;
};

struct GreedyMode {
  bool walk = false;        // sorted-walk windows (else the full scan): ctx->walk and a shard to walk
  bool rccl_path = false;   // the windows go through ncclAllGather (a communicator and no exchange callback)
  // Candidate lists that grow after a rescan (sorted walk): windows start with lists of topk keys (K0);
  // once a window's lists ran out (a rescan: its groups consumed more list entries than it had --
  // whole-node gangs, all of a window's groups after the same few nodes), the rest of the batch walks
  // lists of 2 x topk (Kg).  Longer lists cost walk time (cfg3: 0.58 -> 1.25 ms of device wait at 512),
  // rescans cost a drained pipeline each (cfg4: 41 rescans at 256, none at 384).  The blob capacity K
  // is the grown length from the start.  Sharded runs grow alike on every rank (each resolves every
  // window identically, so all switch at the same window): over a node's shared-memory segment when
  // its slots hold the grown stride (the host merge cuts at the window's length), and over RCCL, whose
  // windows are written, gathered and merged at the window's own list length (rccl_grow: the
  // all-gather moves k_win keys per group, not the capacity).  The decision depends on nothing a rank
  // holds alone (its shard may be empty): ctx->walk, the segment, the communicator.
  bool kgrow = false, rccl_grow = false;
  int K0 = 0, Kg = 0;
  int K = 0;   // blob stride (list capacity)
  bool direct_out = false;     // unsharded: the kernel writes the blob straight into pinned host memory
  bool use_exchange = false;   // the windows go through the exchange callback
  // The host exchange is a synchronous callback.  Pipelined, the launch helper runs it: after it
  // issued window w+1's scan it waits for the own lists, exchanges them and launches the device
  // merge, signalled per group like an RCCL window -- all while the host resolves window w.
  bool pipelined = false;
  // Multi-rank windows (RCCL all-gather, or the host exchange): the gathered shard lists are merged
  // on the device into one list per group (merge_shards), written into pinned host memory and
  // signalled like an unsharded walk window -- no D2H of every shard's lists, no host k-way merge.
  // PE_HOST_MERGE=1: the gathered blob is copied and merged lazily on the host instead.
  // (PE_HOST_MERGE=1 with a host exchange, measured: the lazy host merge doubled the resolve --
  // the seed helper cannot pre-skip merged lists -- 20.4 vs 8.9 ms per 2-rank cfg3 batch)
  // (merge_shards_kernel stages one header per rank in a wave's lanes: world <= MG_THREADS / 64;
  // wider sharded runs take the host merge)
  bool dev_merge = false;
  // the shard merge kernel: at 1-2 ranks the rank merge (256-thread blocks, a cut of each list ranked,
  // no sort), from 3 ranks the top-K sort merge (1024-thread blocks) -- measured alone on one MI355X,
  // 112 groups of K = 256 (tools/bench_merge_dev.cc, profiles/r23_merge_dev.txt): rank 13.7 / 19.9 /
  // 35.0 / 102 us per window at 2 / 4 / 8 / 16 ranks, sort 18.0 / 14.8 / 15.2 / 19.3 us.
  // PE_MERGE_RANKED=1 / PE_MERGE_SORT=1 force one (A/B; the rank merge only where its LDS holds the lists).
  bool ranked = false;
  // Pipelined walk windows written in place are SIGNALLED per group (pe::WindowFeed): the host
  // takes each group's list when its block is done, not at a stream sync after the slowest block.
  // The window requests are then double-buffered like the blobs (a walk may still be running when
  // the next window's requests are written); seeing any group of window w signalled proves that
  // every earlier launch of the stream is complete (kernels of one stream run in order), which is
  // what the pinned update records need.  PE_NO_GROUP_SIGNAL=1: stream sync per window instead.
  // Sharded windows are signalled by the device merge (dev_merge).
  bool signalled = false;
  // Zero-copy shared-memory exchange (pe_hostx.h): each window's walk writes this rank's lists into
  // its slot of the registered segment and the shard merge, queued behind it, waits on the device
  // for every rank's signal of its group -- no exchange thread, no host barrier, no copies.  The
  // ranks agree on it once per context and segment (each says whether it could register the
  // segment); PE_NO_ZC_EXCHANGE=1 (every rank): the copying exchange.
  // Merging a zero-copy window: by default on the host, by the exchange thread, group by group as
  // every rank's walk signals it into the segment (zc_host: no kernel, no PCIe read-back, the
  // resolver streams the merged groups as in an unsharded window); PE_ZC_DEV_MERGE=1 (A/B): a
  // one-block device wait and the merge kernel behind the walk (zc_dev).
  bool zc = false, zc_dev = false, zc_host = false;
  // A copying split exchange reads this rank's lists from the one h_own buffer while the walk of the
  // next window would overwrite it: depth 1 there (only zero-copy windows go deeper).
  bool copy_split = false;
  // Pipeline depth D (signalled windows; PE_PIPE_DEPTH, 1..3, default 1): windows i+1 .. i+D are
  // scanned while window i is resolved (D + 1 blob / request buffers, D update staging slots).  (2
  // measured on a 2-rank host-exchange run: 36 vs 22 ms per cfg3 batch -- every dropped speculation
  // throws away two scans.)  0: not pipelined.
  int depth = 0;
  // A pipelined host exchange with device merge runs on its own thread (split_x): the launch helper
  // only launches window w+1's walk (its lists signalled into pinned memory), the exchange thread
  // waits for them, exchanges and launches the device merge, while the host resolves window w --
  // the resolver then waits for the merged groups' signals only, not for the whole chain.
  // PE_NO_SPLIT_EXCHANGE=1: the launch helper runs the exchange.
  bool split_x = false;
  // PE_XCHG_HOST_MERGE=1 (A/B): the exchange thread merges the gathered lists on the host, group by
  // group, each signalled as written, instead of the device merge -- measured 36.7 vs 18.5 ms per
  // 2-rank cfg3 batch (the merge of world x K keys per group is host work the resolver waits on).
  // The rule is merge_shards_kernel's: the keys below the smallest shard limit, the K + 1 smallest
  // of them; limit = the (K+1)-th, else that minimum.
  bool xhost_merge = false;
  // a pipelined copying exchange's walk writes its own lists into pinned host memory (h_own), signalled
  // per group: no D2H, no stream sync
  bool own_direct = false;
  // Early post (signalled windows at depth 1, one rank or a non-split exchange; PE_EARLY_POST=0: off,
  // A/B; unsignalled windows share one request buffer, which the next walk may still read): once window i
  // landed, the helper is given apply(i) and the scan of window i + 2 at once -- queued behind the walk
  // of window i + 1 -- instead of after the first group of window i + 1 was seen, so the device never
  // idles while the host posts them.  The apply records then need two staging slots: apply(i) may be
  // written while apply(i - 1) has not run yet; the slot it reuses was read by apply(i - 2), which ran
  // before the walk of window i, all of whose groups were resolved.
  bool early_post = false;
  int upd_slots = 1, nbuf = 2;   // update staging slots; blob / request buffers (depth + 1)
  // Zero-copy windows of 3+ ranks: the exchange thread's host merge grows with the world (8 ranks:
  // ~1-2 us per group against ~0.5 us of resolve; tools/bench_merge.cc), so the window's groups are
  // shared among the exchange thread and helpers, group w on thread w mod T (T = 1 + helpers: 2 up to
  // 4 ranks, 4 above; PE_XCHG_THREADS overrides).  The resolver still takes the groups in order.
  // 0: no window is merged on the host (not zc_host); 1 without the exchange thread (not split_x).
  int T = 0;
};

// The part of the mode that does not depend on the zero-copy agreement.
inline GreedyMode greedy_mode_base(const GreedyFacts& f, const GreedyKnobs& kn, const GreedyLimits& lim) {
  GreedyMode m;
  m.walk = f.ctx_walk && f.has_nodes;
  m.rccl_path = f.has_comm && !f.has_exchange;
  m.direct_out = f.world == 1 && !f.has_comm;
  const bool no_growth = m.direct_out && kn.no_list_growth;
  m.K0 = f.topk;
  m.Kg = std::max(m.K0, std::min(2 * m.K0, lim.wk_round - 1));
  const bool hx_grow = f.world > 1 && f.hx;
  m.kgrow = f.ctx_walk && !no_growth &&
            (m.direct_out || m.rccl_path ||
             (hx_grow && (size_t)f.window_groups * lim.cand_group_bytes(m.Kg) <= f.hx_slot_bytes));
  m.rccl_grow = m.kgrow && m.rccl_path;
  m.K = m.kgrow ? m.Kg : m.K0;
  m.use_exchange = f.has_exchange && !m.direct_out;
  m.pipelined = f.pipeline;
  m.dev_merge = !m.direct_out && (int64_t)f.world * m.K <= lim.mg_cap && f.world <= lim.mg_threads / 64 && !kn.host_merge;
  m.ranked = (kn.merge_ranked || (f.world <= 2 && !kn.merge_sort)) && f.world <= lim.rm_max_world &&
             lim.merge_ranked_lds(f.world, m.K) <= lim.rm_max_lds;
  m.signalled = m.pipelined && !kn.no_group_signal && (m.direct_out ? m.walk : m.dev_merge);
  return m;
}

// Does this rank ask for the zero-copy exchange?  (Then the ranks agree: pe_place_greedy.)
inline bool greedy_zc_wanted(const GreedyFacts& f, const GreedyKnobs& kn, const GreedyLimits& lim) {
  const GreedyMode m = greedy_mode_base(f, kn, lim);
  return f.hx && m.use_exchange && m.pipelined && m.signalled && f.ctx_walk && !kn.no_zc_exchange;
}

// zc: the ranks' agreement (false where greedy_zc_wanted is).
inline GreedyMode greedy_mode(const GreedyFacts& f, const GreedyKnobs& kn, const GreedyLimits& lim, bool zc) {
  GreedyMode m = greedy_mode_base(f, kn, lim);
  m.zc = zc;
  m.zc_dev = zc && kn.zc_dev_merge;
  m.zc_host = zc && !m.zc_dev;
  m.copy_split = m.use_exchange && m.walk && !zc;
  m.depth = !m.pipelined ? 0 : !m.signalled || m.copy_split ? 1 : kn.pipe_depth;
  m.split_x = m.use_exchange && m.pipelined && m.signalled && m.walk && !m.zc_dev && !kn.no_split_exchange;
  m.xhost_merge = m.use_exchange && m.dev_merge && kn.xchg_host_merge;
  m.own_direct = m.walk && m.use_exchange && m.pipelined && !zc;
  m.early_post = m.signalled && m.depth == 1 && !m.split_x && kn.early_post;
  m.upd_slots = m.early_post ? 2 : std::max(m.depth, 1);
  m.nbuf = std::max(m.depth, 1) + 1;
  if (m.zc_host && m.split_x) {
    int T = f.world <= 2 ? 1 : f.world <= 4 ? 2 : 4;
    if (kn.xchg_threads_set) T = kn.xchg_threads;
    m.T = std::max(1, std::min(T, lim.max_mergers + 1));
  } else {
    m.T = m.zc_host ? 1 : 0;
  }
  return m;
}

}  // namespace pe
