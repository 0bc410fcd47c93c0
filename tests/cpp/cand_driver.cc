// Driver for the candidate-list kernels (pe_kernels.h: launch_merge_shards, launch_merge_ranked, launch_merge,
// launch_empty_groups), for tests/test_gpu_cand_kernels.py.  Reads a file of cases, launches each on one stream and
// writes the raw output buffers to a second file.  It holds no checking logic: tests/cand_lists.py writes the cases
// and judges the outputs against a sorted union.
//
//   cand_driver <cases file> <output file>
//
// Cases file: u32 magic 'CAND', u32 number of cases, then per case 12 int64
//   kind, world (merge: nwaves), Wg, K, rank_stride, gen, has_xstatus, xstatus, in_bytes, out_bytes, guard_bytes, 0
// followed by in_bytes of input.  Kinds: 0 merge_shards (input in pinned host memory), 1 merge_ranked with
// system-scope loads (pinned host memory), 2 merge_ranked with plain loads (device memory), 3 merge (input = cand
// [Wg][nwaves][64] u64, bound [Wg][nwaves] u64, cnt [Wg][nwaves] i32, back to back), 4 empty_groups (no input).
// The output buffer (device memory) is out_bytes + guard_bytes, prefilled with FILL.
// Output file: u32 magic, u32 number of cases, then per case int32 launch error, int32 sync error, int64 bytes and
// the whole output buffer, guard included.
// A case whose input is smaller than what its launch may read is refused here (exit 2), before anything runs.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pe_kernels.h"

namespace {

constexpr uint32_t MAGIC = 0x444e4143;   // "CAND"
constexpr int FILL = 0xA5;
enum Kind : int64_t { MERGE_SHARDS = 0, RANKED_SYS = 1, RANKED_PLAIN = 2, MERGE = 3, EMPTY = 4 };

#define CK(x)                                                                                    \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) {                                                                      \
      std::fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));     \
      std::exit(1);                                                                              \
    }                                                                                            \
  } while (0)

void need(bool ok, const char* what, long long c) {
  if (ok) return;
  std::fprintf(stderr, "case %lld: %s\n", c, what);
  std::exit(2);
}

void read_all(std::FILE* f, void* p, size_t n) {
  if (n && std::fread(p, 1, n, f) != n) {
    std::fprintf(stderr, "cases file: short read\n");
    std::exit(2);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: cand_driver <cases file> <output file>\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) {
    std::fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  uint32_t head[2];
  read_all(in, head, sizeof head);
  need(head[0] == MAGIC, "bad magic", -1);
  std::fwrite(head, 4, 2, out);
  hipStream_t s;
  CK(hipStreamCreate(&s));
  uint64_t* d_xs = nullptr;
  CK(hipMalloc(&d_xs, 8));
  std::vector<uint8_t> hin, hout;
  for (long long c = 0; c < (long long)head[1]; ++c) {
    int64_t h[12];
    read_all(in, h, sizeof h);
    const int64_t kind = h[0], world = h[1], Wg = h[2], K = h[3], rank_stride = h[4], gen = h[5], has_xs = h[6];
    const uint64_t xs = (uint64_t)h[7];
    const int64_t in_bytes = h[8], out_bytes = h[9], guard = h[10];
    need(kind >= MERGE_SHARDS && kind <= EMPTY, "unknown kind", c);
    need(world >= 1 && world <= (1 << 16) && Wg >= 1 && Wg <= (1 << 16) && K >= 1 && K <= (1 << 16), "shape", c);
    need(in_bytes >= 0 && in_bytes <= (int64_t)1 << 30 && guard >= 0 && guard <= (1 << 20), "sizes", c);
    const int64_t gb = (int64_t)pe::cand_group_bytes((int)K);
    need(out_bytes == Wg * gb, "out_bytes is not Wg lists", c);
    if (kind == MERGE) {
      need(in_bytes == Wg * world * (64 * 8 + 8 + 4), "merge input size", c);
    } else if (kind != EMPTY) {   // every slot a launch may read lies inside the input
      need(rank_stride == 0 || rank_stride >= Wg * gb, "rank_stride below a window", c);
      need(in_bytes >= (world - 1) * (rank_stride > 0 ? rank_stride : Wg * gb) + Wg * gb, "input smaller than the slots", c);
    }
    hin.resize((size_t)in_bytes);
    read_all(in, hin.data(), hin.size());

    uint8_t *p_in = nullptr, *d_in = nullptr, *d_out = nullptr;
    const bool pinned = kind == MERGE_SHARDS || kind == RANKED_SYS;
    if (in_bytes > 0) {
      if (pinned) {
        CK(hipHostMalloc(&p_in, (size_t)in_bytes, hipHostMallocMapped));
        std::memcpy(p_in, hin.data(), hin.size());
        CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_in), p_in, 0));
      } else {
        CK(hipMalloc(&d_in, (size_t)in_bytes));
        CK(hipMemcpy(d_in, hin.data(), hin.size(), hipMemcpyHostToDevice));
      }
    }
    const size_t total = (size_t)(out_bytes + guard);
    CK(hipMalloc(&d_out, total));
    CK(hipMemset(d_out, FILL, total));
    if (has_xs) CK(hipMemcpy(d_xs, &xs, 8, hipMemcpyHostToDevice));
    CK(hipDeviceSynchronize());
    const uint64_t* xp = has_xs ? d_xs : nullptr;
    hipError_t le = hipSuccess;
    switch (kind) {
      case MERGE_SHARDS:
        le = pe::launch_merge_shards(s, d_in, (int)world, (int)Wg, (int)K, d_out, (uint32_t)gen, rank_stride, xp, true);
        break;
      case RANKED_SYS:
      case RANKED_PLAIN:
        le = pe::launch_merge_ranked(s, d_in, (int)world, (int)Wg, (int)K, d_out, (uint32_t)gen, rank_stride, xp,
                                     kind == RANKED_SYS);
        break;
      case MERGE: {
        const size_t slots = (size_t)(Wg * world);
        const uint64_t* cand = reinterpret_cast<const uint64_t*>(d_in);
        const uint64_t* bound = cand + slots * 64;
        const int32_t* cnt = reinterpret_cast<const int32_t*>(bound + slots);
        le = pe::launch_merge(s, cand, cnt, bound, (int)world, (int)K, d_out, (int)Wg);
        break;
      }
      default:
        le = pe::launch_empty_groups(s, (int)Wg, (int)K, d_out, (uint32_t)gen);
    }
    const hipError_t se = hipStreamSynchronize(s);
    hout.assign(total, 0);
    if (se == hipSuccess) CK(hipMemcpy(hout.data(), d_out, total, hipMemcpyDeviceToHost));
    const int32_t errs[2] = {(int32_t)le, (int32_t)se};
    const int64_t nb = (int64_t)total;
    std::fwrite(errs, 4, 2, out);
    std::fwrite(&nb, 8, 1, out);
    std::fwrite(hout.data(), 1, total, out);
    if (se != hipSuccess) {   // a failed kernel: nothing more runs on this device from here
      std::fprintf(stderr, "case %lld: %s\n", c, hipGetErrorString(se));
      std::fclose(out);
      return 3;
    }
    if (d_in) CK(pinned ? hipHostFree(p_in) : hipFree(d_in));
    CK(hipFree(d_out));
  }
  if (std::fclose(out) != 0) return 2;
  std::printf("cand_driver: %u cases\n", head[1]);
  return 0;
}
