// Gang capacity per topology domain (pe_gang_capacity_domains): per distinct pod shape s and domain k
//   dom_slots[s][k] = sum of cap(s, n) over the nodes n with island[n] == k
//   dom_nodes[s][k] = number of those nodes with cap(s, n) >= 1
// with cap as pe_capacity.hip defines it (pe_capacity_eval.h restates its per-node evaluation).  Domain
// ids are arbitrary: nothing here assumes that the nodes of a domain are adjacent or sorted, and nothing
// is kept between calls.
//
// gang_capacity_domains_kernel (its body: pe_domains_body.h, which pe_slice.hip shares): block (x, y) owns CP_SPAN nodes -- CP_NPT CONSECUTIVE nodes per thread,
// loaded once and kept in registers with their island ids -- and the shapes [y * spb, (y + 1) * spb).
//   1. Dictionary, once per block: the block's distinct in-range ids (at most CP_SPAN) go into an LDS
//      open-addressing table of 2 * CP_SPAN keys by compare-and-swap; the winner of a key numbers it
//      (dense local slot 0 .. nd - 1) and notes its domain id.  Each node keeps its local slot, -1 for a
//      node of no domain (id < 0, id >= n_domains, removed slot, lane past the shard).
//   2. Reduction width, once per wave: where a thread's CP_NPT nodes share one slot in every lane they
//      are folded in the thread, and where aligned groups of w lanes share a slot (w the largest such
//      power of two) the group is folded by a butterfly before one lane adds to LDS.  Contiguous racks
//      of 32 give 1 value per thread and w = 8; interleaved ids give w = 1 and one LDS add per node.
//   3. Per shape: cap per node, count and sum packed into one u64 (count << 48 | sum: a block's sum is
//      below 2^41), folded as in 2 and added to the shape's LDS accumulators with ds_add_u64.  DM_ACC
//      accumulators hold min(CP_TS, DM_ACC / nd) shapes between two block syncs.
//   4. Flush: every non-zero accumulator is added to the zeroed global table with one 64-bit and one
//      32-bit vector atomicAdd (the latter only when the node table is asked for), and zeroed.
// Integers throughout: the result does not depend on any order.
// The selection from a table's rows is pe_tree.hip's tree_select_kernel, at one level for this call.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "pe_domains_body.h"

namespace pe {

namespace {

__global__ __launch_bounds__(CP_THREADS) void gang_capacity_domains_kernel(
    const int64_t* __restrict__ res, int64_t stride, const uint32_t* __restrict__ labels,
    const int32_t* __restrict__ island, int64_t Ns, const CapShape* __restrict__ shapes, int S, int spb, int n_domains,
    unsigned long long* __restrict__ dom_slots, uint32_t* __restrict__ dom_nodes) {
  gang_capacity_domains_body<false>(res, stride, labels, island, Ns, shapes, S, spb, n_domains, dom_slots, dom_nodes);
}

}  // namespace

hipError_t launch_gang_capacity_domains(hipStream_t s, const int64_t* res, int64_t stride, const uint32_t* labels,
                                        const int32_t* island, int64_t Ns, const CapShape* shapes, int64_t S,
                                        int n_domains, uint64_t* dom_slots, uint32_t* dom_nodes) {
  if (S <= 0 || Ns <= 0) return hipSuccess;
  const int64_t gx = cap_node_blocks(Ns);
  // enough blocks to fill the chip when the shard alone has too few node blocks: split the shapes
  int64_t gy = std::min<int64_t>(S, std::max<int64_t>(1, 2048 / gx));
  const int64_t spb = (S + gy - 1) / gy;
  gy = (S + spb - 1) / spb;
  hipLaunchKernelGGL(gang_capacity_domains_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(CP_THREADS), 0, s, res,
                     stride, labels, island, Ns, shapes, (int)S, (int)spb, n_domains, (unsigned long long*)dom_slots,
                     dom_nodes);
  return hipGetLastError();
}

}  // namespace pe
