// The layout of the domain calls' pinned blocks (training-operator_amd/csrc/pe_block.h): the fit call's answer block
// and its read-back spans, a span against a brute force over every subset of wanted parts, the alignment of a mixed
// block in with reads and writes through its parts on a buffer of exactly bytes() bytes, the preempt call's block in
// against the offset chain written out by hand, and empty parts.  Stand-alone; tests/test_block_layout_cpu.py builds
// and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pe_block.h"
#include "pe_preempt_plan.h"

using pe::BlockLayout;
using pe::BlockPart;

static int failed = 0;
static long checks = 0;

static void check(const char* name, bool cond) {
  ++checks;
  if (!cond) {
    printf("FAIL %s\n", name);
    ++failed;
  }
}

static bool span_is(const BlockLayout& b, size_t lo, size_t hi) { return b.any && b.lo == lo && b.hi == hi; }

// pe_gang_fit_domains' answers at J = 3, P = 5; want: bit 0 first, 1 fits, 2 fail_group, 3 pods.
static BlockLayout fit_answers(unsigned want, size_t at[4]) {
  BlockLayout b;
  at[0] = b.add<int32_t>(3, 16, want & 1).at;
  at[1] = b.add<uint8_t>(5, 16, want & 2).at;
  at[2] = b.add<int32_t>(5, 16, want & 4).at;
  at[3] = b.add<int64_t>(5, 16, want & 8).at;
  return b;
}

static void test_fit_answers() {
  size_t at[4];
  const BlockLayout none = fit_answers(0, at);
  check("fit offsets", at[0] == 0 && at[1] == 16 && at[2] == 32 && at[3] == 64 && none.bytes() == 104);
  check("fit nothing wanted", !none.any);
  check("fit fail_group alone", span_is(fit_answers(4, at), 32, 52));
  check("fit first and fits", span_is(fit_answers(3, at), 0, 21));
  check("fit pods alone", span_is(fit_answers(8, at), 64, 104));
  check("fit everything", span_is(fit_answers(15, at), 0, 104));
}

// Four parts of odd counts and four types; every subset of wanted parts against the minimum offset and the
// maximum end over the wanted ones.
static void test_every_subset() {
  for (unsigned want = 0; want < 16; ++want) {
    BlockLayout b;
    size_t at[4], end[4];
    const auto p0 = b.add<uint8_t>(1, 16, want & 1);
    const auto p1 = b.add<int32_t>(3, 16, want & 2);
    const auto p2 = b.add<int64_t>(5, 8, want & 4);
    const auto p3 = b.add<int16_t>(7, 2, want & 8);
    at[0] = p0.at, at[1] = p1.at, at[2] = p2.at, at[3] = p3.at;
    end[0] = p0.end(), end[1] = p1.end(), end[2] = p2.end(), end[3] = p3.end();
    check("subset offsets", at[0] == 0 && at[1] == 16 && at[2] == 32 && at[3] == 72 && b.bytes() == 86);
    size_t lo = SIZE_MAX, hi = 0;
    for (int i = 0; i < 4; ++i)
      if (want >> i & 1) {
        if (at[i] < lo) lo = at[i];
        if (end[i] > hi) hi = end[i];
      }
    check("subset any", b.any == (want != 0));
    if (want) check("subset span", span_is(b, lo, hi));
  }
}

struct Rec8 {   // 8-B aligned, as PreRec
  int64_t q;
  int32_t node, sat;
};

// An int32_t part of odd count, then 8-B aligned records: the second offset is rounded up, and every cell of both
// parts is written and read on a buffer of exactly bytes() bytes.
static void test_mixed_alignment() {
  BlockLayout b;
  const auto words = b.add<int32_t>(3);
  const auto recs = b.add<Rec8>(2);
  const auto tail = b.add<int32_t>(1);
  check("mixed offsets", words.at == 0 && recs.at == 16 && tail.at == 48 && b.bytes() == 52);
  uint8_t* const block = (uint8_t*)malloc(b.bytes());   // ASan guards the byte behind bytes()
  for (size_t i = 0; i < words.count; ++i) words.in(block)[i] = (int32_t)i + 1;
  for (size_t i = 0; i < recs.count; ++i) recs.in(block)[i] = Rec8{(int64_t)1 << 40 | (int64_t)i, (int32_t)i, -1};
  tail.in(block)[0] = 77;
  const uint8_t* const ro = block;
  check("mixed alignment", (uintptr_t)recs.in(ro) % alignof(Rec8) == 0);
  check("mixed words", words.in(ro)[0] == 1 && words.in(ro)[2] == 3);
  check("mixed recs", recs.in(ro)[1].q == ((int64_t)1 << 40 | 1) && recs.in(ro)[1].node == 1 && recs.in(ro)[0].sat == -1);
  check("mixed tail", tail.in(ro)[0] == 77);
  free(block);
}

// pe_kernels.h needs HIP, so PlaceGroup and PrePair stand here as copies of their size and alignment: a change of
// the real records does not reach this test (their own static_asserts in pe_kernels.h hold the sizes).
struct alignas(64) Group64 {   // PlaceGroup's size and alignment
  int64_t q[8];
};
struct Pair32 {   // PrePair's
  int32_t w[8];
};
static_assert(sizeof(Group64) == 64 && sizeof(Pair32) == 32 && sizeof(pe::FitUnit) == 16 && sizeof(pe::PreRec) == 40, "");

// pe_gang_preempt_domains' block in at small odd counts: natural alignment adds no padding to the order of parts
// the call uses, so the offsets are the hand chain's.
static void test_preempt_block_in() {
  const int64_t G = 1, P = 3, U = 1, R = 3, V = 2, NL = 5, L0 = 3, ND = 2;
  const size_t pairs_at = (size_t)G * 64;
  const size_t units_at = pairs_at + (size_t)P * 32;
  const size_t recs_at = units_at + (size_t)U * 16;
  const size_t rstart_at = recs_at + (size_t)R * 40;
  const size_t list_at = rstart_at + (size_t)(V + 1) * 4;
  const size_t words_at = list_at + (size_t)NL * 4;
  const size_t in_bytes = words_at + (size_t)(L0 + ND) * 4;
  BlockLayout b;
  const auto groups = b.add<Group64>(G);
  const auto pairs = b.add<Pair32>(P);
  const auto units = b.add<pe::FitUnit>(U);
  const auto recs = b.add<pe::PreRec>(R);
  const auto rstart = b.add<int32_t>(V + 1);
  const auto list = b.add<int32_t>(NL);
  const auto words = b.add<int32_t>(L0 + ND);
  check("preempt in offsets", groups.at == 0 && pairs.at == pairs_at && units.at == units_at && recs.at == recs_at &&
                                  rstart.at == rstart_at && list.at == list_at && words.at == words_at);
  check("preempt in bytes", b.bytes() == in_bytes && in_bytes == 348);
  check("preempt recs 8-B aligned", recs.at % alignof(pe::PreRec) == 0 && alignof(pe::PreRec) == 8);
}

// Empty parts at the front, in the middle and at the end; a wanted empty part reaches no further than its offset.
static void test_empty_parts() {
  BlockLayout b;
  const auto e0 = b.add<int64_t>(0);
  const auto p1 = b.add<int32_t>(3);
  const auto e1 = b.add<int64_t>(0);
  const auto p2 = b.add<uint8_t>(2);
  const auto e2 = b.add<int32_t>(0, 16);
  check("empty offsets", e0.at == 0 && e0.end() == 0 && p1.at == 0 && e1.at == 16 && e1.bytes() == 0 && p2.at == 16 &&
                             e2.at == 32 && b.bytes() == 32);
  BlockLayout w;
  w.add<int32_t>(3, 16);
  const auto mid = w.add<int64_t>(0, 16, true);
  w.add<int32_t>(3, 16);
  check("empty wanted alone", span_is(w, mid.at, mid.at) && mid.at == 16);
  BlockLayout v;
  v.add<int32_t>(3, 16, true);
  v.add<int64_t>(0, 16, true);   // at 16, behind the last wanted byte: the span ends at its offset
  v.add<int32_t>(3, 16);
  check("empty wanted last", span_is(v, 0, 16));
  BlockLayout u;
  u.add<int64_t>(0, 16, true);
  u.add<int32_t>(3, 16, true);
  check("empty wanted first", span_is(u, 0, 12));
  BlockLayout z;
  check("no part", z.bytes() == 0 && !z.any);
}

int main() {
  test_fit_answers();
  test_every_subset();
  test_mixed_alignment();
  test_preempt_block_in();
  test_empty_parts();
  printf("%ld checks, %d failures\n", checks, failed);
  return failed ? 1 : 0;
}
