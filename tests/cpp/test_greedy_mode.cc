// The greedy placement's mode decision (training-operator_amd/csrc/pe_greedy_mode.h): which protocol a
// (world, transport, flags, knobs) combination runs.  Built and run by tests/test_greedy_mode_cpu.py with
// plain g++: the header needs neither HIP nor a GPU.
//
// The expected rows were written by reading pe_place_greedy as it was before the decision moved into the
// header (one 1000-line function computing each value where it was first needed); none was produced by
// running greedy_mode.  Every row states every field.
#include <stdio.h>
#include <stdlib.h>

#include "pe_greedy_mode.h"

using pe::GreedyFacts;
using pe::GreedyKnobs;
using pe::GreedyLimits;
using pe::GreedyMode;

static int failed = 0;

// pe_kernels.h: a 16-B header and K 8-B keys per group
static size_t group_bytes(int K) { return 16 + (size_t)K * 8; }
// the rank merge's LDS need is an input of the decision: one that fits, one that does not
static size_t lds_fits(int, int) { return 1000; }
static size_t lds_too_large(int, int) { return (size_t)1 << 20; }

static GreedyLimits limits(size_t (*lds)(int, int) = &lds_fits) {
  return GreedyLimits{1024, 16384, 1024, 16, (size_t)64 * 1024, 7, &group_bytes, lds};
}

static void expect(const char* name, const GreedyMode& got, const GreedyMode& want) {
  int bad = 0;
#define FIELD(f)                                                                        \
  if ((long)got.f != (long)want.f) {                                                    \
    printf("FAIL %s: %s = %ld, expected %ld\n", name, #f, (long)got.f, (long)want.f); \
    ++bad;                                                                              \
  }
  FIELD(walk) FIELD(rccl_path) FIELD(kgrow) FIELD(rccl_grow) FIELD(K0) FIELD(Kg) FIELD(K) FIELD(direct_out)
  FIELD(use_exchange) FIELD(pipelined) FIELD(dev_merge) FIELD(ranked) FIELD(signalled) FIELD(zc) FIELD(zc_dev)
  FIELD(zc_host) FIELD(copy_split) FIELD(depth) FIELD(split_x) FIELD(xhost_merge) FIELD(own_direct)
  FIELD(early_post) FIELD(upd_slots) FIELD(nbuf) FIELD(T)
#undef FIELD
  if (bad) ++failed;
  else printf("ok   %s\n", name);
}

static void check(const char* name, bool cond) {
  if (cond) {
    printf("ok   %s\n", name);
  } else {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static GreedyMode mode(const GreedyFacts& f, const GreedyKnobs& k, bool zc) { return pe::greedy_mode(f, k, limits(), zc); }
static bool wanted(const GreedyFacts& f, const GreedyKnobs& k) { return pe::greedy_zc_wanted(f, k, limits()); }

// ---- the contexts (defaults: topk 256, window_groups 112, pipeline on, walk on, a shard with nodes)
static GreedyFacts unsharded() { return GreedyFacts{}; }
static GreedyFacts rccl(int world) {
  GreedyFacts f;
  f.world = world;
  f.has_comm = true;
  return f;
}
static GreedyFacts shm(int world, size_t slot = (size_t)16 << 20) {   // the shared-memory exchange
  GreedyFacts f;
  f.world = world;
  f.has_exchange = f.hx = true;
  f.hx_slot_bytes = slot;
  return f;
}

// ---- the expected rows
static GreedyMode row1() {   // unsharded
  GreedyMode e;
  e.walk = true, e.rccl_path = false, e.kgrow = true, e.rccl_grow = false;
  e.K0 = 256, e.Kg = 512, e.K = 512;
  e.direct_out = true, e.use_exchange = false, e.pipelined = true, e.dev_merge = false;
  e.ranked = true;   // (one rank: the rank merge would be eligible; no merge runs)
  e.signalled = true;
  e.zc = e.zc_dev = e.zc_host = false, e.copy_split = false;
  e.depth = 1, e.split_x = false, e.xhost_merge = false, e.own_direct = false;
  e.early_post = true, e.upd_slots = 2, e.nbuf = 2, e.T = 0;
  return e;
}
static GreedyMode row6() {   // RCCL, world 2
  GreedyMode e = row1();
  e.rccl_path = true, e.rccl_grow = true, e.direct_out = false, e.dev_merge = true;
  return e;
}
static GreedyMode row8(int depth) {   // shared-memory exchange, world 2, zero-copy agreed
  GreedyMode e = row1();
  e.direct_out = false, e.use_exchange = true, e.dev_merge = true;
  e.zc = e.zc_host = true;
  e.depth = depth, e.split_x = true, e.early_post = false, e.upd_slots = depth, e.nbuf = depth + 1, e.T = 1;
  return e;
}
static GreedyMode row10() {   // ... not agreed: the copying split exchange
  GreedyMode e = row8(1);
  e.zc = e.zc_host = false, e.copy_split = true, e.own_direct = true, e.T = 0;
  return e;
}

static void test_unsharded() {
  GreedyKnobs k;
  expect("1 unsharded", mode(unsharded(), k, false), row1());
  check("1 unsharded: no zero-copy asked for", !wanted(unsharded(), k));

  GreedyMode e = row1();
  k = GreedyKnobs{};
  k.no_group_signal = true;
  e.signalled = false, e.early_post = false, e.upd_slots = 1;
  expect("2 unsharded, PE_NO_GROUP_SIGNAL", mode(unsharded(), k, false), e);

  GreedyFacts f = unsharded();
  f.pipeline = false;
  e = row1();
  e.pipelined = false, e.signalled = false, e.depth = 0, e.early_post = false, e.upd_slots = 1, e.nbuf = 2;
  expect("3 unsharded, pipeline off", mode(f, GreedyKnobs{}, false), e);

  f = unsharded();
  f.ctx_walk = false;
  e = row1();
  e.walk = false, e.kgrow = false, e.K = 256, e.signalled = false, e.early_post = false, e.upd_slots = 1;
  expect("4 unsharded, full scan", mode(f, GreedyKnobs{}, false), e);

  k = GreedyKnobs{};
  k.no_list_growth = true;
  e = row1();
  e.kgrow = false, e.K = 256;
  expect("5 unsharded, PE_NO_LIST_GROWTH", mode(unsharded(), k, false), e);
  expect("5 RCCL world 2, PE_NO_LIST_GROWTH: no effect", mode(rccl(2), k, false), row6());
  GreedyFacts one = rccl(1);   // one rank with a communicator is not "unsharded"
  e = row6();
  expect("5 RCCL world 1, PE_NO_LIST_GROWTH: no effect", mode(one, k, false), e);
}

static void test_rccl() {
  GreedyKnobs k;
  expect("6 RCCL world 2", mode(rccl(2), k, false), row6());
  check("6 RCCL: no zero-copy asked for", !wanted(rccl(2), k));

  GreedyMode e = row6();
  k.host_merge = true;
  e.dev_merge = false, e.signalled = false, e.early_post = false, e.upd_slots = 1;
  expect("6 RCCL world 2, PE_HOST_MERGE", mode(rccl(2), k, false), e);

  k = GreedyKnobs{};
  k.merge_sort = true;
  e = row6();
  e.ranked = false;
  expect("6 RCCL world 2, PE_MERGE_SORT", mode(rccl(2), k, false), e);

  k = GreedyKnobs{};
  k.pipe_depth = 3;
  e = row6();
  e.depth = 3, e.early_post = false, e.upd_slots = 3, e.nbuf = 4;
  expect("6 RCCL world 2, PE_PIPE_DEPTH=3", mode(rccl(2), k, false), e);

  e = row6();   // more ranks than merge_shards_kernel stages headers for (MG_THREADS / 64 = 16)
  e.dev_merge = false, e.ranked = false, e.signalled = false, e.early_post = false, e.upd_slots = 1;
  expect("7 RCCL world 17", mode(rccl(17), GreedyKnobs{}, false), e);

  // 14: the rank merge past two ranks only when forced, where its LDS holds the lists, up to RM_MAX_WORLD
  k = GreedyKnobs{};
  e = row6();
  e.ranked = false;
  expect("14 RCCL world 3: sort merge", mode(rccl(3), k, false), e);
  k.merge_ranked = true;
  e.ranked = true;
  expect("14 RCCL world 3, PE_MERGE_RANKED", mode(rccl(3), k, false), e);
  e.ranked = false;
  expect("14 RCCL world 3, PE_MERGE_RANKED, lists too long for LDS",
         pe::greedy_mode(rccl(3), k, limits(&lds_too_large), false), e);
  expect("14 RCCL world 2, lists too long for LDS", pe::greedy_mode(rccl(2), GreedyKnobs{}, limits(&lds_too_large), false), e);
  e = row6();
  e.dev_merge = false, e.ranked = false, e.signalled = false, e.early_post = false, e.upd_slots = 1;
  expect("14 RCCL world 17, PE_MERGE_RANKED: never ranked", mode(rccl(17), k, false), e);
}

static void test_shared_memory() {
  GreedyKnobs k;
  check("8 shared memory world 2: zero-copy asked for", wanted(shm(2), k));
  expect("8 shared memory world 2, zero-copy", mode(shm(2), k, true), row8(1));
  k.pipe_depth = 2;
  expect("8 shared memory world 2, zero-copy, PE_PIPE_DEPTH=2", mode(shm(2), k, true), row8(2));

  GreedyMode e = row8(1);   // the mergers: 1 up to 2 ranks, 2 up to 4, 4 above; PE_XCHG_THREADS 1 .. 8
  e.ranked = false, e.T = 2;
  expect("8 shared memory world 4: T 2", mode(shm(4), GreedyKnobs{}, true), e);
  e.T = 4;
  expect("8 shared memory world 8: T 4", mode(shm(8), GreedyKnobs{}, true), e);
  k = GreedyKnobs{};
  k.xchg_threads_set = true, k.xchg_threads = 100;
  e = row8(1);
  e.T = 8;
  expect("8 shared memory world 2, PE_XCHG_THREADS=100: T 8", mode(shm(2), k, true), e);
  k.xchg_threads = 0;
  e.T = 1;
  expect("8 shared memory world 2, PE_XCHG_THREADS=0: T 1", mode(shm(2), k, true), e);

  k = GreedyKnobs{};
  k.zc_dev_merge = true;
  e = row8(1);
  e.zc_dev = true, e.zc_host = false, e.split_x = false, e.T = 0, e.early_post = true, e.upd_slots = 2;
  expect("9 shared memory world 2, PE_ZC_DEV_MERGE", mode(shm(2), k, true), e);
  k.pipe_depth = 2;
  e.depth = 2, e.early_post = false, e.upd_slots = 2, e.nbuf = 3;
  expect("9 shared memory world 2, PE_ZC_DEV_MERGE, PE_PIPE_DEPTH=2", mode(shm(2), k, true), e);

  expect("10 shared memory world 2, copying", mode(shm(2), GreedyKnobs{}, false), row10());
  k = GreedyKnobs{};
  k.pipe_depth = 3;
  expect("10 shared memory world 2, copying, PE_PIPE_DEPTH=3: depth 1", mode(shm(2), k, false), row10());
  k = GreedyKnobs{};
  k.no_split_exchange = true;
  e = row10();
  e.split_x = false, e.early_post = true, e.upd_slots = 2;
  expect("10 shared memory world 2, copying, PE_NO_SPLIT_EXCHANGE", mode(shm(2), k, false), e);
  k = GreedyKnobs{};
  k.xchg_host_merge = true;
  e = row10();
  e.xhost_merge = true;
  expect("10 shared memory world 2, copying, PE_XCHG_HOST_MERGE", mode(shm(2), k, false), e);

  GreedyFacts cb = shm(2);   // 11: a caller's own exchange callback
  cb.hx = false, cb.hx_slot_bytes = 0;
  e = row10();
  e.kgrow = false, e.K = 256;
  check("11 exchange callback: no zero-copy asked for", !wanted(cb, GreedyKnobs{}));
  expect("11 exchange callback world 2", mode(cb, GreedyKnobs{}, false), e);

  // 12: slots that hold a window of topk lists but not of the grown ones
  const GreedyFacts small = shm(2, 112 * group_bytes(512) - 1);
  expect("12 shared memory, small slots: no growth", mode(small, GreedyKnobs{}, false), e);
  e = row8(1);
  e.kgrow = false, e.K = 256;
  expect("12 shared memory, small slots, zero-copy", mode(small, GreedyKnobs{}, true), e);
  expect("12 shared memory, slots just large enough", mode(shm(2, 112 * group_bytes(512)), GreedyKnobs{}, true), row8(1));

  // 16: a rank whose shard is empty still asks (the condition is ctx->walk: nothing a rank holds alone),
  // but launches no walk: its exchange does not split
  GreedyFacts empty = shm(2);
  empty.has_nodes = false;
  check("16 shared memory, empty shard: zero-copy asked for", wanted(empty, GreedyKnobs{}));
  e = row8(1);
  e.walk = false, e.split_x = false, e.early_post = true, e.upd_slots = 2, e.T = 1;
  expect("16 shared memory, empty shard, zero-copy", mode(empty, GreedyKnobs{}, true), e);
}

static void test_zc_wanted() {   // 13: each missing precondition in turn
  GreedyFacts f = shm(2);
  f.pipeline = false;
  check("13 not wanted: pipeline off", !wanted(f, GreedyKnobs{}));
  GreedyKnobs k;
  k.no_group_signal = true;
  check("13 not wanted: PE_NO_GROUP_SIGNAL", !wanted(shm(2), k));
  k = GreedyKnobs{};
  k.host_merge = true;
  check("13 not wanted: PE_HOST_MERGE", !wanted(shm(2), k));
  f = shm(2);
  f.ctx_walk = false;
  check("13 not wanted: full scan", !wanted(f, GreedyKnobs{}));
  k = GreedyKnobs{};
  k.no_zc_exchange = true;
  check("13 not wanted: PE_NO_ZC_EXCHANGE", !wanted(shm(2), k));
  check("13 not wanted: world 17 (host merge)", !wanted(shm(17), GreedyKnobs{}));
}

static void test_from_env() {   // 15
  static const char* const names[] = {
      "PE_NO_LIST_GROWTH", "PE_ASYNC_RESORT", "PE_WALK_SWITCH_DELAY", "PE_DUMP_WINDOWS", "PE_DUMP_MAX_WINDOWS",
      "PE_GREEDY_TRACE", "PE_WALK_EVENTS", "PE_WALK_FLUSH", "PE_NO_PIN", "PE_HOST_MERGE", "PE_MERGE_RANKED",
      "PE_MERGE_SORT", "PE_NO_GROUP_SIGNAL", "PE_NO_ZC_EXCHANGE", "PE_PIPE_DEPTH", "PE_TEST_STALL_WINDOW",
      "PE_TEST_STALL_MS", "PE_HX_GPU_TIMEOUT_S", "PE_ZC_DEV_MERGE", "PE_NO_SPLIT_EXCHANGE", "PE_XCHG_THREADS",
      "PE_XCHG_HOST_MERGE", "PE_EARLY_POST"};
  for (const char* n : names) unsetenv(n);
  GreedyKnobs k = GreedyKnobs::from_env();
  check("15 nothing set: the defaults",
        !k.no_list_growth && k.async_resort && k.switch_delay == 0 && !k.dump_path && k.dump_max == INT64_MAX &&
            !k.trace && !k.walk_events && !k.walk_flush && !k.no_pin && !k.host_merge && !k.merge_ranked &&
            !k.merge_sort && !k.no_group_signal && !k.no_zc_exchange && k.pipe_depth == 1 && k.stall_window == -1 &&
            k.stall_ticks == 0 && k.zc_ticks == 6000000000LL && !k.zc_dev_merge && !k.no_split_exchange &&
            !k.xchg_threads_set && !k.xchg_host_merge && k.early_post);
  setenv("PE_ASYNC_RESORT", "0", 1);
  setenv("PE_EARLY_POST", "0", 1);
  k = GreedyKnobs::from_env();
  check("15 PE_ASYNC_RESORT=0, PE_EARLY_POST=0: off", !k.async_resort && !k.early_post);
  setenv("PE_ASYNC_RESORT", "1", 1);
  setenv("PE_EARLY_POST", "1", 1);
  k = GreedyKnobs::from_env();
  check("15 PE_ASYNC_RESORT=1, PE_EARLY_POST=1: on", k.async_resort && k.early_post);
  const int depth_in[] = {0, 2, 9}, depth_out[] = {1, 2, 3};
  for (int i = 0; i < 3; ++i) {
    char v[8];
    snprintf(v, sizeof v, "%d", depth_in[i]);
    setenv("PE_PIPE_DEPTH", v, 1);
    check("15 PE_PIPE_DEPTH clamps to 1..3", GreedyKnobs::from_env().pipe_depth == depth_out[i]);
  }
  setenv("PE_TEST_STALL_MS", "99999", 1);
  setenv("PE_TEST_STALL_WINDOW", "3", 1);
  k = GreedyKnobs::from_env();
  check("15 PE_TEST_STALL_MS=99999: 30 s of 100 MHz ticks", k.stall_ticks == 3000000000LL && k.stall_window == 3);
  setenv("PE_TEST_STALL_MS", "-5", 1);
  check("15 PE_TEST_STALL_MS=-5: none", GreedyKnobs::from_env().stall_ticks == 0);
  setenv("PE_HX_GPU_TIMEOUT_S", "-1", 1);
  check("15 PE_HX_GPU_TIMEOUT_S=-1: 60 s of ticks", GreedyKnobs::from_env().zc_ticks == 6000000000LL);
  setenv("PE_HX_GPU_TIMEOUT_S", "2.5", 1);
  check("15 PE_HX_GPU_TIMEOUT_S=2.5", GreedyKnobs::from_env().zc_ticks == 250000000LL);
  setenv("PE_XCHG_THREADS", "3", 1);
  k = GreedyKnobs::from_env();
  check("15 PE_XCHG_THREADS=3", k.xchg_threads_set && k.xchg_threads == 3);
  // presence-only knobs: any value, "0" and "" included
  setenv("PE_HOST_MERGE", "0", 1);
  setenv("PE_NO_ZC_EXCHANGE", "", 1);
  setenv("PE_ZC_DEV_MERGE", "1", 1);
  setenv("PE_DUMP_WINDOWS", "/tmp/x", 1);
  setenv("PE_DUMP_MAX_WINDOWS", "7", 1);
  setenv("PE_WALK_SWITCH_DELAY", "4", 1);
  k = GreedyKnobs::from_env();
  check("15 presence-only knobs", k.host_merge && k.no_zc_exchange && k.zc_dev_merge && !k.merge_sort);
  check("15 dump and switch-delay knobs", k.dump_path && k.dump_max == 7 && k.switch_delay == 4);
}

int main() {
  test_unsharded();
  test_rccl();
  test_shared_memory();
  test_zc_wanted();
  test_from_env();
  printf("%d failed checks\n", failed);
  return failed ? 1 : 0;
}
