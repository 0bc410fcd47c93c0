// The plan of pe_place_min_member_domains (training-operator_amd/csrc/pe_place_min_plan.h): every group's mandatory
// and optional share and the records built from them against a brute force that walks the job's pod slots one by
// one, min_member at its bounds with counts of 2^31 - 1, and every refusal with its index.  Built and run by
// tests/test_place_min_plan_cpu.py with g++ and the address and undefined-behaviour sanitizers: the header needs
// neither HIP nor a GPU.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "pe_place_min_plan.h"

using pe::PlaceMinPlan;

static int failed = 0;
static long plans = 0, jobs_checked = 0, groups_checked = 0;
static const int32_t BIG = 2147483647;

static void check(const char* name, bool cond) {
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool same_plan(const PlaceMinPlan& a, const PlaceMinPlan& b) {
  return a.base.level == b.base.level && a.base.n_leaf == b.base.n_leaf && a.base.n_dom == b.base.n_dom &&
         a.base.leaf_dom == b.base.leaf_dom && a.base.act_of == b.base.act_of && a.base.active == b.base.active &&
         a.base.job_start == b.base.job_start && a.base.jobs == b.base.jobs && a.base.pod_off == b.base.pod_off &&
         a.mand == b.mand && a.opt == b.opt && a.mand_pod0 == b.mand_pod0 && a.opt_pod0 == b.opt_pod0 &&
         a.job_gm == b.job_gm && a.job_shift == b.job_shift && a.job_pods == b.job_pods && a.mand_pods == b.mand_pods;
}

struct Batch {
  std::vector<int32_t> off, priority, count, domain, min_member;
  std::vector<uint32_t> need;
};

static int build(PlaceMinPlan& p, const Batch& b, bool with_min, bool with_need, int32_t n_dom, int64_t* bad,
                 pe::PlacePlanError* be = nullptr) {
  const int32_t sizes[1] = {n_dom};
  return pe::place_min_plan_build(p, (int64_t)b.priority.size(), b.off.data(), b.priority.data(), b.count.data(),
                                  with_need ? b.need.data() : nullptr, with_min ? b.min_member.data() : nullptr,
                                  b.domain.data(), 0, 1, sizes, nullptr, be, nullptr, bad);
}

// The shares of one job by walking its pod slots: slot s < M is mandatory; an island group with a mandatory slot is
// mandatory as a whole.  Small counts only.
static void brute(const Batch& b, int j, bool with_need, int64_t M, std::vector<int32_t>& m) {
  int64_t slot = 0;
  for (int32_t g = b.off[(size_t)j]; g < b.off[(size_t)j + 1]; ++g) {
    int32_t mine = 0;
    for (int32_t k = 0; k < b.count[(size_t)g]; ++k, ++slot)
      if (slot < M) ++mine;
    if (mine > 0 && with_need && (b.need[(size_t)g] & 0x80000000u)) mine = b.count[(size_t)g];
    m[(size_t)g] = mine;
  }
}

static void verify(const char* name, const Batch& b, bool with_min, bool with_need, int32_t n_dom) {
  PlaceMinPlan p;
  int64_t bad = 7;
  const int e = build(p, b, with_min, with_need, n_dom, &bad);
  check(name, e == pe::PLACE_MIN_OK && bad == -1);
  if (e != pe::PLACE_MIN_OK) return;
  ++plans;
  const size_t J = b.priority.size(), G = b.count.size();
  check(name, p.mand.size() == G && p.opt.size() == G && p.mand_pod0.size() == G && p.opt_pod0.size() == G);
  check(name, p.job_gm.size() == J && p.job_shift.size() == J && p.job_pods.size() == J);
  if (failed) return;
  std::vector<int32_t> m(G, 0);
  int64_t pod = 0, mpod = 0;   // slots among all pods, among the mandatory pods
  for (size_t j = 0; j < J; ++j) {
    int64_t T = 0;
    for (int32_t g = b.off[j]; g < b.off[j + 1]; ++g) T += b.count[(size_t)g];
    const int64_t M = (!with_min || b.min_member[j] == -1) ? T : b.min_member[j];
    brute(b, (int)j, with_need, M, m);
    check(name, p.job_pods[j] == T && p.job_shift[j] == pod - mpod);
    int32_t gm = b.off[j];
    for (int32_t g = b.off[j]; g < b.off[j + 1]; ++g) {
      const size_t u = (size_t)g;
      check(name, p.mand[u] == m[u] && p.opt[u] == b.count[u] - m[u]);
      check(name, p.mand_pod0[u] == mpod && p.opt_pod0[u] == pod + m[u] && p.base.pod_off[u] == pod);
      // a mandatory slot plus the job's shift is the pod's slot among all slots
      if (m[u] > 0) check(name, p.mand_pod0[u] + p.job_shift[j] == pod);
      if (m[u] > 0) gm = g + 1;
      pod += b.count[u];
      mpod += m[u];
      ++groups_checked;
    }
    check(name, p.job_gm[j] == gm);
    // the mandatory records [g0, gm) are contiguous in the mandatory numbering and no later group has one
    for (int32_t g = gm; g < b.off[j + 1]; ++g) check(name, p.mand[(size_t)g] == 0);
    ++jobs_checked;
  }
  check(name, p.mand_pods == mpod && p.pods() == pod);
}

static Batch random_batch(std::mt19937& rng, int J, int32_t n_dom) {
  Batch b;
  b.off.push_back(0);
  for (int j = 0; j < J; ++j) {
    const int g = (int)(rng() % 5);
    int64_t T = 0;
    std::vector<int64_t> edges;
    for (int k = 0; k < g; ++k) {
      const int32_t c = (int32_t)(rng() % 4 == 0 ? 0 : rng() % 9);
      b.count.push_back(c);
      b.need.push_back(rng() % 3 == 0 ? 0x80000001u : (uint32_t)(rng() % 2));
      T += c;
      edges.push_back(T);
    }
    b.off.push_back((int32_t)b.count.size());
    b.priority.push_back((int32_t)(rng() % 4) - 1);
    b.domain.push_back((int32_t)(rng() % (uint32_t)n_dom));
    int64_t mm;
    switch (rng() % 7) {
      case 0: mm = 0; break;
      case 1: mm = 1; break;
      case 2: mm = T - 1; break;
      case 3: mm = T; break;
      case 4: mm = -1; break;
      case 5: mm = edges.empty() ? 0 : edges[rng() % edges.size()]; break;
      default: mm = T > 0 ? (int64_t)(rng() % (uint64_t)(T + 1)) : 0;
    }
    b.min_member.push_back((int32_t)std::min<int64_t>(std::max<int64_t>(mm, -1), T));
  }
  return b;
}

int main() {
  std::mt19937 rng(20240607);
  for (int it = 0; it < 400; ++it) {
    const int32_t n_dom = 1 + (int32_t)(rng() % 6);
    const Batch b = random_batch(rng, 1 + (int)(rng() % 30), n_dom);
    verify("random", b, true, true, n_dom);
    if (it % 4 == 0) verify("random, no need", b, true, false, n_dom);
    if (it % 4 == 1) verify("random, no min_member", b, false, true, n_dom);
  }
  // ---- the bounds: 0, -1, T and 2^31 - 1 with counts of 2^31 - 1
  {
    Batch b;
    b.off = {0, 1, 2, 3, 5, 7, 9};
    b.count = {BIG, BIG, BIG, BIG, BIG, BIG, BIG, 5, BIG};
    b.need = {0, 0, 0, 0, 0, 0x80000000u, 0, 0, 0x80000000u};
    b.priority = {0, 0, 0, 0, 0, 0};
    b.domain = {0, 0, 0, 0, 0, 0};
    b.min_member = {0, -1, BIG, BIG, BIG, 3};
    PlaceMinPlan p;
    int64_t bad = 7;
    check("bounds", build(p, b, true, true, 1, &bad) == pe::PLACE_MIN_OK && bad == -1);
    const int64_t B = BIG;
    check("bounds M=0", p.mand[0] == 0 && p.opt[0] == BIG && p.job_gm[0] == 0 && p.job_pods[0] == B);
    check("bounds M=-1", p.mand[1] == BIG && p.opt[1] == 0 && p.job_gm[1] == 2);
    check("bounds M=T", p.mand[2] == BIG && p.opt[2] == 0 && p.job_gm[2] == 3);
    // T = 2 (2^31 - 1): the first group mandatory in full, the second optional in full
    check("bounds M=2^31-1 of 2T", p.mand[3] == BIG && p.opt[3] == 0 && p.mand[4] == 0 && p.opt[4] == BIG &&
                                       p.job_gm[3] == 4 && p.job_pods[3] == 2 * B);
    // an island group mandatory in full; the cut on its far edge leaves the next group optional
    check("bounds island then the edge", p.mand[5] == BIG && p.mand[6] == 0 && p.opt[6] == BIG && p.job_gm[4] == 6);
    // the cut inside group 7 (3 of 5); the island group of 2^31 - 1 after it stays optional
    check("bounds inside", p.mand[7] == 3 && p.opt[7] == 2 && p.mand[8] == 0 && p.opt[8] == BIG && p.job_gm[5] == 8);
    check("bounds slots", p.pods() == 8 * B + 5 && p.mand_pods == 4 * B + 3 && p.opt_pod0[8] == 7 * B + 5 &&
                              p.mand_pod0[7] == 4 * B && p.job_shift[5] == 3 * B && p.opt_pod0[7] == 7 * B + 3);
    // the island flag moves to the second group: on the edge it stays optional as a whole ...
    b.need[5] = 0;
    b.need[6] = 0x80000000u;
    check("bounds rebuild", build(p, b, true, true, 1, &bad) == pe::PLACE_MIN_OK && p.mand[6] == 0);
    b.count[5] = BIG - 1;    // ... and a cut one pod into it makes it mandatory as a whole: 2^32 - 2 mandatory pods
    check("bounds island cut", build(p, b, true, true, 1, &bad) == pe::PLACE_MIN_OK && p.mand[5] == BIG - 1 &&
                                   p.mand[6] == BIG && p.opt[6] == 0 && p.job_gm[4] == 7);
    ++plans;
  }
  // ---- refusals: the index, and the plan as it was
  {
    std::mt19937 r2(5);
    const Batch good = random_batch(r2, 12, 3);
    PlaceMinPlan kept;
    int64_t bad = 7;
    check("refusal base", build(kept, good, true, true, 3, &bad) == pe::PLACE_MIN_OK);
    struct Bad {
      const char* name;
      int job;
      int32_t value;
      int want;
    };
    auto total = [&](int j) {
      int64_t T = 0;
      for (int32_t g = good.off[(size_t)j]; g < good.off[(size_t)j + 1]; ++g) T += good.count[(size_t)g];
      return (int32_t)T;
    };
    const Bad cases[] = {{"below at 0", 0, -2, pe::PLACE_MIN_BELOW},
                         {"below at 7", 7, INT32_MIN, pe::PLACE_MIN_BELOW},
                         {"above at 3", 3, total(3) + 1, pe::PLACE_MIN_ABOVE},
                         {"above at 11", 11, BIG, pe::PLACE_MIN_ABOVE},
                         {"above at 0", 0, total(0) + 1, pe::PLACE_MIN_ABOVE}};
    for (const Bad& c : cases) {
      Batch b = good;
      b.min_member[(size_t)c.job] = c.value;
      PlaceMinPlan p = kept;
      bad = 7;
      check(c.name, build(p, b, true, true, 3, &bad) == c.want && bad == c.job && same_plan(p, kept));
    }
    {   // two offenders: the first one is named
      Batch b = good;
      b.min_member[9] = -3;
      b.min_member[4] = total(4) + 2;
      PlaceMinPlan p = kept;
      check("first offender", build(p, b, true, true, 3, &bad) == pe::PLACE_MIN_ABOVE && bad == 4 && same_plan(p, kept));
    }
    {   // the base plan's refusals come first and pass through with their index
      Batch b = good;
      b.domain[5] = 3;
      b.min_member[1] = -9;
      PlaceMinPlan p = kept;
      pe::PlacePlanError be = pe::PLACE_OK;
      check("base first", build(p, b, true, true, 3, &bad, &be) == pe::PLACE_MIN_BASE && be == pe::PLACE_BAD_DOMAIN &&
                              bad == 5 && same_plan(p, kept));
    }
    {   // no jobs: an empty plan
      Batch b;
      b.off = {0};
      PlaceMinPlan p = kept;
      check("no jobs", build(p, b, true, true, 3, &bad) == pe::PLACE_MIN_OK && p.mand.empty() && p.job_gm.empty() &&
                           p.mand_pods == 0 && p.pods() == 0);
    }
  }
  printf("%ld plans, %ld jobs, %ld groups checked, %d failures\n", plans, jobs_checked, groups_checked, failed);
  return failed ? 1 : 0;
}
