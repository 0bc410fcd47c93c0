// libplacement: the gang-capacity calls -- pe_gang_capacity (the whole shard), pe_gang_capacity_domains
// (per topology domain) and pe_gang_capacity_tree (over a hierarchy of levels) -- and pe_gang_split_tree, the
// tree call's selection followed by the descent that spreads the gang over the fewest domains.  All reduce the
// batch to its distinct pod shapes (cap_dedupe) and stage them the same way; the table calls and the split are
// one host path, capacity_levels: a domain table is the tree of one level.  pe_gang_slice_tree, the split of a
// gang in slices that each stay inside one domain, runs beside it (slice_levels) on tables with one row per
// distinct (shape, slice size, slice level) and its own kernels (pe_slice.hip).  Own buffers (pe_ctx.h cp_*, lv_*):
// neither the residuals nor the staged fit-mask state are touched, and nothing is kept between calls.
#include <type_traits>

#include "pe_ctx.h"
#include "pe_divmagic.h"
#include "pe_first_seen.h"
#include "pe_slice_plan.h"
#include "pe_split_plan.h"
#include "pe_tree_plan.h"

static_assert(pe::TREE_MAX_LEVELS == PE_MAX_LEVELS && pe::TR_MAX_LEVELS == PE_MAX_LEVELS, "PE_MAX_LEVELS");
static_assert(pe::TREE_MAX_LEVEL_SIZE == PE_MAX_DOMAINS, "PE_MAX_DOMAINS");
static_assert(pe::SPLIT_MAX_PARTS == PE_MAX_SPLIT_PARTS && pe::SPLIT_TOO_MANY == PE_SPLIT_TOO_MANY &&
                  pe::SPLIT_LEVELS == PE_MAX_LEVELS && pe::SPLIT_BUFFER_BYTES == (int64_t(64) << 20),
              "pe_split_plan.h");
static_assert(pe::SLICE_NODE == PE_SLICE_NODE, "pe_slice_plan.h");
static_assert(PE_MAX_LEVELS == 4, "a pick's key keeps max_level in 2 bits; the scatter of the counts names 1 .. 4");

namespace {

// What every capacity call checks before it looks at its outputs' shapes, in the order the callers see the
// refusals (the entry points check n_jobs < 0 and their own arguments first).  select: the call has a
// selection output, so count is read.  Returns false when there are no jobs: the call is complete.
bool cap_prologue(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, bool select, const int32_t* count) {
  if (!ctx->loaded) raise(PE_ESTATE, "no inventory loaded");
  if (select && ctx->world > 1)
    raise(PE_EINVAL, "selection outputs on a sharded context: a domain may span shards (add the tables, then select)");
  if (n_jobs == 0) return false;
  if (n_jobs > (int64_t)INT32_MAX) raise(PE_EINVAL, "n_jobs above 2^31 - 1");
  need_ptr(req, "req");
  check_req(req, n_jobs, "req");
  if (select) {
    need_ptr(count, "count");
    const int64_t i = first_bad(n_jobs, [count](int64_t k) { return count[k] < 1; });
    if (i < n_jobs) raise(PE_EINVAL, "count: value below 1 at index " + std::to_string(i));
  }
  return true;
}

// The batch's distinct (request, need) shapes in first-seen order -> ctx->cp_uniq (with the reciprocals of
// their requests, pe_divmagic.h), each job's shape -> ctx->cp_of.
void cap_dedupe(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need) {
  auto& uniq = ctx->cp_uniq;
  uniq.clear();
  auto need_of = [need](int64_t j) { return need ? need[j] : 0u; };
  pe::first_seen(
      n_jobs, ctx->cp_tab, ctx->cp_of,
      [&](int64_t j) {
        uint64_t h = need_of(j);
        for (int d = 0; d < pe::D; ++d) h = pe::first_seen_mix(h ^ (uint64_t)req[j * pe::D + d]);
        return h;
      },
      [&](int64_t j, int32_t u) {
        const int64_t* q = req + j * pe::D;
        const pe::CapShape& s = uniq[(size_t)u];
        return s.q[0] == q[0] && s.q[1] == q[1] && s.q[2] == q[2] && s.q[3] == q[3] && s.need == need_of(j);
      },
      [&](int64_t j) {
        const int64_t* q = req + j * pe::D;
        pe::CapShape sp{};
        for (int d = 0; d < pe::D; ++d) {
          sp.q[d] = q[d];
          if (q[d] > 0) {
            const pe::DivMagic dm = pe::div_magic((uint64_t)q[d]);
            sp.m[d] = dm.m;
            sp.sh[d] = dm.shift;
          }
        }
        sp.need = need_of(j);
        uniq.push_back(sp);
      });
}

// ctx->cp_uniq to the pinned buffer and from there to the device (ctx->cp_shapes); returns their number S.
int64_t cap_stage_shapes(pe_ctx* ctx) {
  const size_t S = ctx->cp_uniq.size();
  hipchk(ctx->cp_hshapes.ensure(S), "alloc pinned shapes");
  hipchk(ctx->cp_shapes.ensure(S), "alloc shapes");
  std::memcpy((void*)ctx->cp_hshapes.p, ctx->cp_uniq.data(), S * sizeof(pe::CapShape));
  hipchk(hipMemcpyAsync(ctx->cp_shapes.p, ctx->cp_hshapes.p, S * sizeof(pe::CapShape), hipMemcpyHostToDevice, ctx->stream),
         "H2D shapes");
  return (int64_t)S;
}

// The outputs of a table call over `plan`'s levels (T columns in all), each optional.
struct LevelOut {
  int64_t* slots;          // [J][T]
  int64_t* nodes;          // [J][T]
  int32_t* level;          // [J]
  int32_t* domain;         // [J]
  int64_t* domain_slots;   // [J]
  int32_t* feasible;       // [J][n_levels]
  // pe_gang_split_tree alone (split: the call is one, whichever outputs it asked for)
  bool split = false;
  int32_t max_parts = 0;
  int32_t* parts = nullptr;          // [J]
  int32_t* part_domain = nullptr;    // [J][max_parts]
  int32_t* part_pods = nullptr;      // [J][max_parts]
  int32_t* spread = nullptr;         // [J][n_levels]
};

// Gang capacity over the levels of `plan`, for both table calls.  gang_capacity_domains_kernel adds every
// node's capacity to the [shape][leaf] tables of its island id (pe_domains.hip); one tree_rollup_kernel launch
// per upper level folds them along the plan's child lists into a table of the upper levels' columns; for a
// selection, tree_select_kernel answers each distinct (shape, count, max_level) from the shape's rows
// (pe_tree.hip).  The plan's words and the picks go in with one copy, the picks' answers and their per-level
// counts come back with one.  Both tables exist on the device for one chunk of shapes at a time (12 B per
// shape and column, 64 MiB at most, 16 shapes at least); requested tables are copied out per chunk and
// scattered to the jobs here, otherwise only the picks' answers cross.  max_level NULL: the top level.
// A split call runs tree_split_kernel (pe_split.hip) behind the selection of every chunk, on slices of the
// picks whose parts stay within 64 MiB on the device (pe_split_plan.h); a slice's answers come back with one
// copy of the blocks the caller asked for and are scattered to the jobs at once.
int capacity_levels(pe_ctx* ctx, const pe::TreePlan& plan, int64_t n_jobs, const int64_t* req, const uint32_t* need,
                    const int32_t* count, const int32_t* max_level, const LevelOut& out) {
  const int32_t n_levels = plan.n_levels;
  const bool select = out.split || out.level || out.domain || out.domain_slots || out.feasible;
  const bool parts = out.parts || out.part_domain || out.part_pods || out.spread;
  const bool tables = out.slots || out.nodes;
  if (!cap_prologue(ctx, n_jobs, req, select, count)) return PE_OK;
  if (select && max_level) {
    const int64_t i =
        first_bad(n_jobs, [max_level, n_levels](int64_t k) { return max_level[k] < 0 || max_level[k] >= n_levels; });
    if (i < n_jobs) raise(PE_EINVAL, "max_level: value outside [0, n_levels) at index " + std::to_string(i));
  }
  const int64_t T = plan.columns(), L0 = plan.size[0], U = plan.upper_columns();
  if (ctx->Ns == 0) {   // an empty shard holds nothing
    if (out.slots) std::memset(out.slots, 0, (size_t)(n_jobs * T) * sizeof(int64_t));
    if (out.nodes) std::memset(out.nodes, 0, (size_t)(n_jobs * T) * sizeof(int64_t));
    if (out.feasible) std::memset(out.feasible, 0, (size_t)(n_jobs * n_levels) * sizeof(int32_t));
    if (out.parts) std::memset(out.parts, 0, (size_t)n_jobs * sizeof(int32_t));
    if (out.spread) std::memset(out.spread, 0, (size_t)(n_jobs * n_levels) * sizeof(int32_t));
    if (out.part_domain) std::fill_n(out.part_domain, n_jobs * out.max_parts, -1);
    if (out.part_pods) std::memset(out.part_pods, 0, (size_t)(n_jobs * out.max_parts) * sizeof(int32_t));
    for (int64_t j = 0; j < n_jobs; ++j) {
      if (out.level) out.level[j] = -1;
      if (out.domain) out.domain[j] = -1;
      if (out.domain_slots) out.domain_slots[j] = 0;
    }
    return PE_OK;
  }
  cap_dedupe(ctx, n_jobs, req, need);
  const auto& of = ctx->cp_of;
  // distinct (shape, count, max_level) picks, in first-seen order.  The dedupe works on the three packed
  // into 64 bits -- shape < 2^31, count in [1, 2^31), max_level < 4 -- so a probe compares one word and the
  // keys of a large batch take half the cache of the device's 16-byte records.
  auto& keys = ctx->lv_pkeys;
  const auto& pof = ctx->lv_pof;
  keys.clear();
  if (select) {
    const uint64_t top = (uint64_t)(n_levels - 1);
    auto key_of = [&](int64_t j) {
      return ((uint64_t)of[(size_t)j] << 33) | ((uint64_t)count[j] << 2) | (max_level ? (uint64_t)max_level[j] : top);
    };
    pe::first_seen(
        n_jobs, ctx->lv_ptab, ctx->lv_pof, [&](int64_t j) { return pe::first_seen_mix(key_of(j)); },
        [&](int64_t j, int32_t u) { return keys[(size_t)u] == key_of(j); }, [&](int64_t j) { keys.push_back(key_of(j)); });
  }
  const int64_t P = (int64_t)keys.size();
  CapEvents ev(ctx);
  const int64_t S = cap_stage_shapes(ctx);
  // shapes per launch: the tables of all levels (12 B per shape and column) stay within 64 MiB (16 shapes at least)
  const int64_t fit64 = (int64_t(64) << 20) / (12 * T);
  const int64_t chunk = std::min<int64_t>(S, std::max<int64_t>(16, fit64));
  hipchk(ctx->lv_leaf.ensure((size_t)(chunk * L0 + (chunk * L0 + 1) / 2)), "alloc leaf tables");
  if (U > 0) hipchk(ctx->lv_upper.ensure((size_t)(chunk * U + (chunk * U + 1) / 2)), "alloc upper tables");
  if (out.slots) hipchk(ctx->lv_hslots.ensure((size_t)(chunk * T)), "alloc pinned table slots");
  if (out.nodes) hipchk(ctx->lv_hnodes.ensure((size_t)(chunk * T)), "alloc pinned table nodes");
  // the call's inputs beside the shapes, in one pinned block and one copy: the plan's words, then the picks
  const size_t words = plan.words.size(), pick_at = (words + 3) / 4 * 4;   // picks 16-B aligned
  const size_t in_words = pick_at + (size_t)P * (sizeof(pe::TreePick) / sizeof(int32_t));
  if (in_words > 0) {
    hipchk(ctx->lv_hin.ensure(in_words), "alloc pinned plan and picks");
    hipchk(ctx->lv_in.ensure(in_words), "alloc plan and picks");
    if (words) std::memcpy((void*)ctx->lv_hin.p, plan.words.data(), words * sizeof(int32_t));
    pe::TreePick* const h_picks = (pe::TreePick*)(ctx->lv_hin.p + pick_at);
    for (int64_t p = 0; p < P; ++p) {   // the keys unpacked, straight into the pinned block
      const uint64_t k = keys[(size_t)p];
      h_picks[p] = pe::TreePick{(uint32_t)(k >> 33), (int32_t)((k >> 2) & 0x7FFFFFFF), (int32_t)(k & 3), 0};
    }
    hipchk(hipMemcpyAsync(ctx->lv_in.p, ctx->lv_hin.p, in_words * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream),
           "H2D plan and picks");
  }
  const int32_t* const d_plan = ctx->lv_in.p;
  const pe::TreePick* const d_picks = (const pe::TreePick*)(ctx->lv_in.p + pick_at);
  // the answers likewise: P selections, then their [P][n_levels] counts (one copy back)
  const size_t sel_words = (size_t)P * (sizeof(pe::TreeSel) / sizeof(uint32_t));
  const size_t out_words = sel_words + (size_t)(P * n_levels);
  if (select) {
    hipchk(ctx->lv_out.ensure(out_words), "alloc selections");
    hipchk(ctx->lv_hout.ensure(out_words), "alloc pinned selections");
  }
  pe::TreeSel* const d_sel = (pe::TreeSel*)ctx->lv_out.p;
  uint32_t* const d_feas = ctx->lv_out.p + sel_words;
  // the split's slices of picks: one device buffer and its pinned twin, sized for the largest slice
  const int64_t slice = parts ? std::min<int64_t>(P, pe::split_slice_picks(out.max_parts)) : 0;
  pe::SplitCsr csr{};
  if (parts) {
    const size_t w = (size_t)pe::SplitLayout{slice, out.max_parts}.words();
    hipchk(ctx->lv_split.ensure(w), "alloc parts");
    hipchk(ctx->lv_hsplit.ensure(w), "alloc pinned parts");
    for (int l = 1; l < n_levels; ++l) {
      csr.start_at[l] = plan.start_at[l];
      csr.child_at[l] = plan.child_at[l];
    }
  }
  pe::TreeLevels lv{};
  lv.n_levels = n_levels;
  lv.pitch = (int32_t)U;
  for (int l = 0; l < n_levels; ++l) {
    lv.size[l] = plan.size[l];
    lv.col[l] = l == 0 ? 0 : plan.off[l] - plan.size[0];
  }
  ev.begin();
  bool ev_open = true;   // kernels were launched since the events' end was last recorded
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    const int64_t sc = std::min(chunk, S - s0);
    ev_open = true;
    // a table's slots and nodes are adjacent: one memset for the leaves (every cell of the upper table is
    // stored).  The node tables exist only for a caller who reads them (the selection reads the slots alone):
    // without them the leaf flush costs half the global atomics.
    uint64_t* const d_slots = ctx->lv_leaf.p;
    uint32_t* const d_nodes = out.nodes ? (uint32_t*)(d_slots + sc * L0) : nullptr;
    uint64_t* const u_slots = U > 0 ? ctx->lv_upper.p : nullptr;
    uint32_t* const u_nodes = U > 0 && out.nodes ? (uint32_t*)(u_slots + sc * U) : nullptr;
    hipchk(hipMemsetAsync(d_slots, 0, (size_t)(sc * L0) * (sizeof(uint64_t) + (d_nodes ? sizeof(uint32_t) : 0)),
                          ctx->stream),
           "zero leaf tables");
    hipchk(pe::launch_gang_capacity_domains(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                            ctx->cp_shapes.p + s0, sc, (int)L0, d_slots, d_nodes),
           "launch gang_capacity_domains");
    for (int l = 1; l < n_levels; ++l) {   // level l from level l - 1
      const bool leaf = l == 1;
      const int64_t lo_col = leaf ? 0 : lv.col[l - 1];
      hipchk(pe::launch_tree_rollup(ctx->stream, (leaf ? d_slots : u_slots) + lo_col,
                                    out.nodes ? (leaf ? d_nodes : u_nodes) + lo_col : nullptr, leaf ? L0 : U,
                                    d_plan + plan.start_at[l], d_plan + plan.child_at[l], plan.size[l], plan.width[l],
                                    sc, u_slots + lv.col[l], u_nodes ? u_nodes + lv.col[l] : nullptr, U),
             "launch tree_rollup");
    }
    if (select)
      hipchk(pe::launch_tree_select(ctx->stream, d_slots, u_slots, s0, sc, lv, d_picks, P, d_sel, d_feas),
             "launch tree_select");
    for (int64_t p0 = 0; parts && p0 < P; p0 += slice) {
      const int64_t n = std::min(slice, P - p0);
      // a pick is answered by the launch that holds its shape's rows
      auto live = [&](int64_t p) {
        const int64_t s = (int64_t)(keys[(size_t)p] >> 33) - s0;
        return s >= 0 && s < sc;
      };
      if (sc < S && first_bad(n, [&](int64_t k) { return live(p0 + k); }) == n) continue;   // none of this chunk
      const pe::SplitLayout sl{n, out.max_parts};
      hipchk(pe::launch_tree_split(ctx->stream, d_slots, u_slots, s0, sc, lv, csr, d_plan, d_picks, d_sel, p0, n,
                                   out.max_parts, ctx->lv_split.p),
             "launch tree_split");
      ev.end();   // before the slice's copy and scatter: with one slice the events span the kernels alone
      ev_open = false;
      const pe::SplitRange r = pe::split_copy_range(sl, out.part_domain, out.parts || out.spread, out.part_pods);
      hipchk(hipMemcpyAsync(ctx->lv_hsplit.p + r.first, ctx->lv_split.p + r.first, (size_t)r.count * sizeof(int32_t),
                            hipMemcpyDeviceToHost, ctx->stream),
             "D2H parts");
      hipchk(hipStreamSynchronize(ctx->stream), "sync parts");
      // rows of up to 8 KiB per job from picks all over the slice: a large batch is scattered by the planning pool
      const int kT = n_jobs * pe::split_row_words(out.max_parts) >= (int64_t(1) << 20) ? 8 : 1;
      plan_pool_run(kT, [&](int t) {
        pe::split_scatter((const int32_t*)ctx->lv_hsplit.p, sl, p0, n_jobs * t / kT, n_jobs * (t + 1) / kT, pof.data(),
                          n_levels, live, out.parts, out.part_domain, out.part_pods, out.spread);
      });
    }
    if (!tables) continue;
    // pinned copies: the chunk's leaf rows [sc][L0], then its upper rows [sc][U]
    if (out.slots) {
      hipchk(hipMemcpyAsync(ctx->lv_hslots.p, d_slots, (size_t)(sc * L0) * sizeof(uint64_t), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H leaf slots");
      if (U > 0)
        hipchk(hipMemcpyAsync(ctx->lv_hslots.p + sc * L0, u_slots, (size_t)(sc * U) * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, ctx->stream),
               "D2H upper slots");
    }
    if (out.nodes) {
      hipchk(hipMemcpyAsync(ctx->lv_hnodes.p, d_nodes, (size_t)(sc * L0) * sizeof(uint32_t), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H leaf nodes");
      if (U > 0)
        hipchk(hipMemcpyAsync(ctx->lv_hnodes.p + sc * L0, u_nodes, (size_t)(sc * U) * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, ctx->stream),
               "D2H upper nodes");
    }
    hipchk(hipStreamSynchronize(ctx->stream), "sync capacity tables");
    for (int64_t j = 0; j < n_jobs; ++j) {   // the chunk's rows to their jobs
      const int64_t s = (int64_t)of[(size_t)j] - s0;
      if (s < 0 || s >= sc) continue;
      if (out.slots) {   // below 2^55: the bits are the int64's
        int64_t* o = out.slots + j * T;
        std::memcpy(o, (const void*)(ctx->lv_hslots.p + s * L0), (size_t)L0 * sizeof(int64_t));
        if (U > 0) std::memcpy(o + L0, (const void*)(ctx->lv_hslots.p + sc * L0 + s * U), (size_t)U * sizeof(int64_t));
      }
      if (out.nodes) {
        int64_t* o = out.nodes + j * T;
        const uint32_t* lrow = ctx->lv_hnodes.p + s * L0;
        for (int64_t k = 0; k < L0; ++k) o[k] = (int64_t)lrow[k];
        const uint32_t* urow = ctx->lv_hnodes.p + sc * L0 + s * U;
        for (int64_t k = 0; k < U; ++k) o[L0 + k] = (int64_t)urow[k];
      }
    }
  }
  if (ev_open) ev.end();
  if (select)
    hipchk(hipMemcpyAsync(ctx->lv_hout.p, ctx->lv_out.p, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
           "D2H selections");
  hipchk(hipStreamSynchronize(ctx->stream), "sync capacity levels");
  if (select) {
    const pe::TreeSel* a = (const pe::TreeSel*)ctx->lv_hout.p;
    const uint32_t* f = ctx->lv_hout.p + sel_words;
    for (int64_t j = 0; j < n_jobs; ++j) {
      const pe::TreeSel& r = a[pof[(size_t)j]];
      if (out.level) out.level[j] = r.level;
      if (out.domain) out.domain[j] = r.domain;
      if (out.domain_slots) out.domain_slots[j] = (int64_t)r.slots;
    }
    // the counts, rows of [P][n_levels] to [J][n_levels]: with the row length a constant a row is a few moves
    // (one level: a plain gather); a run-time length costs a loop per job, 60 us more per 100 000 jobs at
    // one level than the gather (timing)
    auto rows = [&](auto L) {
      for (int64_t j = 0; j < n_jobs; ++j)
        for (int l = 0; l < L(); ++l) out.feasible[j * L() + l] = (int32_t)f[(int64_t)pof[(size_t)j] * L() + l];
    };
    if (out.feasible) {
      switch (n_levels) {
        case 1: rows(std::integral_constant<int, 1>()); break;
        case 2: rows(std::integral_constant<int, 2>()); break;
        case 3: rows(std::integral_constant<int, 3>()); break;
        default: rows(std::integral_constant<int, 4>()); break;   // PE_MAX_LEVELS
      }
    }
  }
  ev.report(S, P);
  return PE_OK;
}

// pe_gang_slice_tree: capacity_levels' path for a split, on tables with one row per distinct (shape, z, sl)
// (pe_slice_plan.h) that hold slots below the level m = max(sl, 0) and units at and above it.  Per chunk of rows
// (8 B per row and column, 64 MiB at most, 16 rows at least): slice_leaf_kernel fills the leaf rows -- node-level
// rows in units --, slice_units_kernel turns the sl = 0 rows' leaves into units, tree_rollup_kernel folds level
// after level as it does for every table call, slice_units_kernel again behind the roll-up of a level that some
// row names; slice_select_kernel then answers the picks from their level m upward and slice_split_kernel
// descends, in slices of picks as in capacity_levels.  The plan's words, the rows and the picks go in with one
// copy; a slice's parts come back with one copy of the blocks asked for, the selections with one at the end.
struct SliceOut {
  int32_t max_parts;
  int32_t* level;          // [J]
  int32_t* domain;         // [J]
  int64_t* domain_units;   // [J]
  int32_t* parts;          // [J]
  int32_t* part_domain;    // [J][max_parts]
  int32_t* part_pods;      // [J][max_parts]
  int32_t* spread;         // [J][n_levels]
};
int slice_levels(pe_ctx* ctx, const pe::TreePlan& plan, int64_t n_jobs, const int64_t* req, const uint32_t* need,
                 const int32_t* count, const int32_t* slice_size, const int32_t* slice_level, const int32_t* max_level,
                 const SliceOut& out) {
  const int32_t n_levels = plan.n_levels;
  const bool parts = out.parts || out.part_domain || out.part_pods || out.spread;
  if (!cap_prologue(ctx, n_jobs, req, true, count)) return PE_OK;
  if (max_level) {
    const int64_t i =
        first_bad(n_jobs, [max_level, n_levels](int64_t k) { return max_level[k] < 0 || max_level[k] >= n_levels; });
    if (i < n_jobs) raise(PE_EINVAL, "max_level: value outside [0, n_levels) at index " + std::to_string(i));
  }
  int64_t bad = -1;
  switch (pe::slice_validate(n_jobs, count, slice_size, slice_level, max_level, n_levels, &bad)) {
    case pe::SLICE_OK: break;
    case pe::SLICE_BAD_SIZE: raise(PE_EINVAL, "slice_size: value below 1 at index " + std::to_string(bad));
    case pe::SLICE_BAD_COUNT: raise(PE_EINVAL, "count: not a multiple of slice_size at index " + std::to_string(bad));
    case pe::SLICE_BAD_LEVEL:
      raise(PE_EINVAL, "slice_level: value outside [PE_SLICE_NODE, n_levels) at index " + std::to_string(bad));
    case pe::SLICE_BAD_MAX_LEVEL:
      raise(PE_EINVAL, "max_level: value below max(slice_level, 0) at index " + std::to_string(bad));
  }
  if (ctx->Ns == 0) {   // an empty shard holds nothing
    if (out.parts) std::memset(out.parts, 0, (size_t)n_jobs * sizeof(int32_t));
    if (out.spread) std::memset(out.spread, 0, (size_t)(n_jobs * n_levels) * sizeof(int32_t));
    if (out.part_domain) std::fill_n(out.part_domain, n_jobs * out.max_parts, -1);
    if (out.part_pods) std::memset(out.part_pods, 0, (size_t)(n_jobs * out.max_parts) * sizeof(int32_t));
    for (int64_t j = 0; j < n_jobs; ++j) {
      if (out.level) out.level[j] = -1;
      if (out.domain) out.domain[j] = -1;
      if (out.domain_units) out.domain_units[j] = 0;
    }
    return PE_OK;
  }
  cap_dedupe(ctx, n_jobs, req, need);
  pe::SlicePlan& sp = ctx->sl_plan;
  pe::slice_plan_build(sp, n_jobs, ctx->cp_of.data(), count, slice_size, slice_level, max_level, n_levels);
  const int64_t S = (int64_t)ctx->cp_uniq.size(), R = (int64_t)sp.rows.size(), P = (int64_t)sp.picks.size();
  const int64_t T = plan.columns(), L0 = plan.size[0], U = plan.upper_columns();
  CapEvents ev(ctx);
  // the rows' shape records: a node-level row carries its z for the leaf kernel (pe_domains_body.h)
  bool at_level[PE_MAX_LEVELS] = {false, false, false, false};   // levels whose rows need the conversion
  hipchk(ctx->cp_hshapes.ensure((size_t)R), "alloc pinned shapes");
  hipchk(ctx->cp_shapes.ensure((size_t)R), "alloc shapes");
  for (int64_t r = 0; r < R; ++r) {
    const pe::SliceRow& row = sp.rows[(size_t)r];
    pe::CapShape rec = ctx->cp_uniq[row.shape];
    rec.pad_[0] = row.sl == pe::SLICE_NODE ? (uint32_t)row.z : 0u;
    std::memcpy((void*)(ctx->cp_hshapes.p + r), &rec, sizeof(rec));
    if (row.sl >= 0 && row.z > 1) at_level[row.sl] = true;
  }
  hipchk(hipMemcpyAsync(ctx->cp_shapes.p, ctx->cp_hshapes.p, (size_t)R * sizeof(pe::CapShape), hipMemcpyHostToDevice,
                        ctx->stream),
         "H2D shapes");
  const int64_t fit64 = (int64_t(64) << 20) / (8 * T);
  const int64_t chunk = std::min<int64_t>(R, std::max<int64_t>(16, fit64));
  hipchk(ctx->lv_leaf.ensure((size_t)(chunk * L0)), "alloc leaf tables");
  if (U > 0) hipchk(ctx->lv_upper.ensure((size_t)(chunk * U)), "alloc upper tables");
  // one pinned block and one copy in: the plan's words, then (16-B aligned) the rows, then the picks
  static_assert(sizeof(pe::SliceRow) == 16 && sizeof(pe::TreePick) == 16, "16-B records");
  const size_t words = plan.words.size(), row_at = (words + 3) / 4 * 4, pick_at = row_at + (size_t)R * 4;
  const size_t in_words = pick_at + (size_t)P * 4;
  hipchk(ctx->lv_hin.ensure(in_words), "alloc pinned plan, rows and picks");
  hipchk(ctx->lv_in.ensure(in_words), "alloc plan, rows and picks");
  if (words) std::memcpy((void*)ctx->lv_hin.p, plan.words.data(), words * sizeof(int32_t));
  std::memcpy((void*)(ctx->lv_hin.p + row_at), sp.rows.data(), (size_t)R * sizeof(pe::SliceRow));
  pe::TreePick* const h_picks = (pe::TreePick*)(ctx->lv_hin.p + pick_at);
  for (int64_t p = 0; p < P; ++p) {
    const uint64_t k = sp.picks[(size_t)p];
    const uint32_t row = pe::slice_pick_row(k);
    h_picks[p] = pe::TreePick{row, pe::slice_pick_units(k), pe::slice_pick_max_level(k), pe::slice_floor(sp.rows[row].sl)};
  }
  hipchk(hipMemcpyAsync(ctx->lv_in.p, ctx->lv_hin.p, in_words * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream),
         "H2D plan, rows and picks");
  const int32_t* const d_plan = ctx->lv_in.p;
  const pe::SliceRow* const d_rows = (const pe::SliceRow*)(ctx->lv_in.p + row_at);
  const pe::TreePick* const d_picks = (const pe::TreePick*)(ctx->lv_in.p + pick_at);
  const size_t sel_words = (size_t)P * (sizeof(pe::TreeSel) / sizeof(uint32_t));
  hipchk(ctx->lv_out.ensure(sel_words), "alloc selections");
  hipchk(ctx->lv_hout.ensure(sel_words), "alloc pinned selections");
  pe::TreeSel* const d_sel = (pe::TreeSel*)ctx->lv_out.p;
  const int64_t slice = parts ? std::min<int64_t>(P, pe::split_slice_picks(out.max_parts)) : 0;
  pe::SplitCsr csr{};
  if (parts) {
    const size_t w = (size_t)pe::SplitLayout{slice, out.max_parts}.words();
    hipchk(ctx->lv_split.ensure(w), "alloc parts");
    hipchk(ctx->lv_hsplit.ensure(w), "alloc pinned parts");
    for (int l = 1; l < n_levels; ++l) {
      csr.start_at[l] = plan.start_at[l];
      csr.child_at[l] = plan.child_at[l];
    }
  }
  pe::TreeLevels lv{};
  lv.n_levels = n_levels;
  lv.pitch = (int32_t)U;
  for (int l = 0; l < n_levels; ++l) {
    lv.size[l] = plan.size[l];
    lv.col[l] = l == 0 ? 0 : plan.off[l] - plan.size[0];
  }
  ev.begin();
  bool ev_open = true;   // kernels were launched since the events' end was last recorded
  for (int64_t r0 = 0; r0 < R; r0 += chunk) {
    const int64_t rc = std::min(chunk, R - r0);
    ev_open = true;
    uint64_t* const d_leaf = ctx->lv_leaf.p;
    uint64_t* const d_upper = U > 0 ? ctx->lv_upper.p : nullptr;
    hipchk(hipMemsetAsync(d_leaf, 0, (size_t)(rc * L0) * sizeof(uint64_t), ctx->stream), "zero leaf tables");
    hipchk(pe::launch_slice_leaf(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->island.p, ctx->Ns,
                                 ctx->cp_shapes.p + r0, rc, (int)L0, d_leaf),
           "launch slice_leaf");
    if (at_level[0])
      hipchk(pe::launch_slice_units(ctx->stream, d_leaf, L0, (int)L0, d_rows + r0, rc, 0), "launch slice_units");
    for (int l = 1; l < n_levels; ++l) {   // level l from level l - 1
      const bool leaf = l == 1;
      hipchk(pe::launch_tree_rollup(ctx->stream, leaf ? d_leaf : d_upper + lv.col[l - 1], nullptr, leaf ? L0 : U,
                                    d_plan + plan.start_at[l], d_plan + plan.child_at[l], plan.size[l], plan.width[l], rc,
                                    d_upper + lv.col[l], nullptr, U),
             "launch tree_rollup");
      if (at_level[l])
        hipchk(pe::launch_slice_units(ctx->stream, d_upper + lv.col[l], U, plan.size[l], d_rows + r0, rc, l),
               "launch slice_units");
    }
    hipchk(pe::launch_slice_select(ctx->stream, d_leaf, d_upper, r0, rc, lv, d_picks, P, d_sel), "launch slice_select");
    for (int64_t p0 = 0; parts && p0 < P; p0 += slice) {
      const int64_t n = std::min(slice, P - p0);
      // a pick is answered by the launch that holds its row
      auto live = [&](int64_t p) {
        const int64_t r = (int64_t)pe::slice_pick_row(sp.picks[(size_t)p]) - r0;
        return r >= 0 && r < rc;
      };
      if (rc < R && first_bad(n, [&](int64_t k) { return live(p0 + k); }) == n) continue;   // none of this chunk
      const pe::SplitLayout sl{n, out.max_parts};
      hipchk(pe::launch_slice_split(ctx->stream, d_leaf, d_upper, r0, rc, lv, csr, d_plan, d_rows, d_picks, d_sel, p0, n,
                                    out.max_parts, ctx->lv_split.p),
             "launch slice_split");
      ev.end();   // before the slice's copy and scatter: with one slice the events span the kernels alone
      ev_open = false;
      const pe::SplitRange rg = pe::split_copy_range(sl, out.part_domain, out.parts || out.spread, out.part_pods);
      hipchk(hipMemcpyAsync(ctx->lv_hsplit.p + rg.first, ctx->lv_split.p + rg.first, (size_t)rg.count * sizeof(int32_t),
                            hipMemcpyDeviceToHost, ctx->stream),
             "D2H parts");
      hipchk(hipStreamSynchronize(ctx->stream), "sync parts");
      const int kT = n_jobs * pe::split_row_words(out.max_parts) >= (int64_t(1) << 20) ? 8 : 1;
      plan_pool_run(kT, [&](int t) {
        pe::split_scatter((const int32_t*)ctx->lv_hsplit.p, sl, p0, n_jobs * t / kT, n_jobs * (t + 1) / kT,
                          sp.pick_of.data(), n_levels, live, out.parts, out.part_domain, out.part_pods, out.spread);
      });
    }
  }
  if (ev_open) ev.end();
  hipchk(hipMemcpyAsync(ctx->lv_hout.p, ctx->lv_out.p, sel_words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream),
         "D2H selections");
  hipchk(hipStreamSynchronize(ctx->stream), "sync slice levels");
  const pe::TreeSel* a = (const pe::TreeSel*)ctx->lv_hout.p;
  for (int64_t j = 0; j < n_jobs; ++j) {
    const pe::TreeSel& r = a[sp.pick_of[(size_t)j]];
    if (out.level) out.level[j] = r.level;
    if (out.domain) out.domain[j] = r.domain;
    if (out.domain_units) out.domain_units[j] = (int64_t)r.slots;
  }
  ev.report_as("S=" + std::to_string(S) + " R=" + std::to_string(R) + " P=" + std::to_string(P));
  return PE_OK;
}

}  // namespace

extern "C" {

// Gang capacity: the distinct (request, need) shapes of the batch go to the device with the reciprocals of
// their requests, gang_capacity_kernel answers per shape over the shard's current residuals
// (pe_capacity.hip), and the host scatters the answers back to the jobs.
int pe_gang_capacity(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, int64_t* out_slots,
                     int32_t* out_max_node, int64_t* out_nodes) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (!cap_prologue(ctx, n_jobs, req, false, nullptr)) return PE_OK;
    cap_dedupe(ctx, n_jobs, req, need);
    const auto& of = ctx->cp_of;
    const int64_t S = (int64_t)ctx->cp_uniq.size();
    CapEvents ev(ctx);
    hipchk(ctx->cp_hout.ensure((size_t)S), "alloc pinned capacity results");
    if (ctx->Ns == 0) {   // an empty shard holds nothing
      std::memset((void*)ctx->cp_hout.p, 0, (size_t)S * sizeof(pe::CapAcc));
    } else {
      cap_stage_shapes(ctx);
      hipchk(ctx->cp_out.ensure((size_t)S), "alloc capacity results");
      // shapes per launch: the partials (one record per node block and shape) stay within 64 MiB
      const int64_t gx = pe::cap_node_blocks(ctx->Ns);
      const int64_t fit64 = (int64_t(4) << 20) / gx / pe::CP_TS * pe::CP_TS;
      const int64_t chunk = std::min<int64_t>(S, std::max<int64_t>(pe::CP_TS, fit64));
      hipchk(ctx->cp_part.ensure((size_t)(gx * chunk)), "alloc capacity partials");
      ev.begin();
      for (int64_t s0 = 0; s0 < S; s0 += chunk)
        hipchk(pe::launch_gang_capacity(ctx->stream, ctx->res.p, ctx->stride, ctx->labels.p, ctx->Ns, ctx->cp_shapes.p + s0,
                                        std::min(chunk, S - s0), ctx->cp_part.p, ctx->cp_out.p + s0),
               "launch gang_capacity");
      ev.end();
      hipchk(hipMemcpyAsync(ctx->cp_hout.p, ctx->cp_out.p, (size_t)S * sizeof(pe::CapAcc), hipMemcpyDeviceToHost,
                            ctx->stream),
             "D2H capacity results");
      hipchk(hipStreamSynchronize(ctx->stream), "sync gang_capacity");
    }
    const pe::CapAcc* a = ctx->cp_hout.p;
    for (int64_t j = 0; j < n_jobs; ++j) {
      const pe::CapAcc& r = a[of[(size_t)j]];
      if (out_slots) out_slots[j] = (int64_t)r.slots;
      if (out_max_node) out_max_node[j] = (int32_t)r.max_node;
      if (out_nodes) out_nodes[j] = (int64_t)r.nodes;
    }
    ev.report(S);
    return PE_OK;
  });
}

// Gang capacity per topology domain: the hierarchy of one level, n_domains leaves and no parent map.  The
// per-job count of domains that hold the gang, [J], is capacity_levels' [J][1].
int pe_gang_capacity_domains(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* count,
                             int32_t n_domains, int64_t* out_dom_slots, int64_t* out_dom_nodes, int32_t* out_domain,
                             int64_t* out_domain_slots, int32_t* out_feasible) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    pe::TreePlan plan;
    if (pe::tree_plan_build(plan, 1, &n_domains, nullptr) != pe::TREE_OK)   // one level: only its size can be refused
      raise(PE_EINVAL, "n_domains outside [1, PE_MAX_DOMAINS]");
    return capacity_levels(ctx, plan, n_jobs, req, need, count, nullptr,
                           LevelOut{out_dom_slots, out_dom_nodes, nullptr, out_domain, out_domain_slots, out_feasible});
  });
}

// Gang capacity over a topology hierarchy.  The parent map is validated and turned into per-level child
// lists by pe_tree_plan.h, once per call; nothing of it is kept.
int pe_gang_capacity_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* count,
                          const int32_t* max_level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                          int64_t* out_tree_slots, int64_t* out_tree_nodes, int32_t* out_level, int32_t* out_domain,
                          int64_t* out_domain_slots, int32_t* out_feasible) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    pe::TreePlan plan;
    int64_t bad = -1;
    switch (pe::tree_plan_build(plan, n_levels, level_size, parent, &bad)) {
      case pe::TREE_OK: break;
      case pe::TREE_BAD_LEVELS: raise(PE_EINVAL, "n_levels outside [1, PE_MAX_LEVELS]");
      case pe::TREE_NO_SIZES: raise(PE_EINVAL, "level_size is NULL");
      case pe::TREE_BAD_SIZE:
        raise(PE_EINVAL, "level_size: value outside [1, PE_MAX_DOMAINS] at index " + std::to_string(bad));
      case pe::TREE_NO_PARENT: raise(PE_EINVAL, "parent is NULL with n_levels > 1");
      case pe::TREE_BAD_PARENT:
        raise(PE_EINVAL, "parent: value outside [-1, size of the level above) at index " + std::to_string(bad));
    }
    return capacity_levels(ctx, plan, n_jobs, req, need, count, max_level,
                           LevelOut{out_tree_slots, out_tree_nodes, out_level, out_domain, out_domain_slots, out_feasible});
  });
}

// The tree call's selection and, behind it on the same device tables, the descent to (leaf, pods) parts.
int pe_gang_split_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* count,
                       const int32_t* max_level, int32_t n_levels, const int32_t* level_size, const int32_t* parent,
                       int32_t max_parts, int32_t* out_level, int32_t* out_domain, int32_t* out_parts,
                       int32_t* out_part_domain, int32_t* out_part_pods, int32_t* out_spread) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (max_parts < 1 || max_parts > PE_MAX_SPLIT_PARTS) raise(PE_EINVAL, "max_parts outside [1, PE_MAX_SPLIT_PARTS]");
    pe::TreePlan plan;
    int64_t bad = -1;
    const pe::TreePlanError te = pe::tree_plan_build(plan, n_levels, level_size, parent, &bad);
    if (te != pe::TREE_OK) raise_tree(te, bad);
    LevelOut out{nullptr, nullptr, out_level, out_domain, nullptr, nullptr};
    out.split = true;
    out.max_parts = max_parts;
    out.parts = out_parts;
    out.part_domain = out_part_domain;
    out.part_pods = out_part_pods;
    out.spread = out_spread;
    return capacity_levels(ctx, plan, n_jobs, req, need, count, max_level, out);
  });
}

// A gang in slices: the rows, the selection in units and the descent (slice_levels).
int pe_gang_slice_tree(pe_ctx* ctx, int64_t n_jobs, const int64_t* req, const uint32_t* need, const int32_t* count,
                       const int32_t* slice_size, const int32_t* slice_level, const int32_t* max_level, int32_t n_levels,
                       const int32_t* level_size, const int32_t* parent, int32_t max_parts, int32_t* out_level,
                       int32_t* out_domain, int64_t* out_domain_units, int32_t* out_parts, int32_t* out_part_domain,
                       int32_t* out_part_pods, int32_t* out_spread) {
  return guarded(ctx, [&]() -> int {
    if (n_jobs < 0) raise(PE_EINVAL, "n_jobs < 0");
    if (max_parts < 1 || max_parts > PE_MAX_SPLIT_PARTS) raise(PE_EINVAL, "max_parts outside [1, PE_MAX_SPLIT_PARTS]");
    pe::TreePlan plan;
    int64_t bad = -1;
    const pe::TreePlanError te = pe::tree_plan_build(plan, n_levels, level_size, parent, &bad);
    if (te != pe::TREE_OK) raise_tree(te, bad);
    return slice_levels(ctx, plan, n_jobs, req, need, count, slice_size, slice_level, max_level,
                        SliceOut{max_parts, out_level, out_domain, out_domain_units, out_parts, out_part_domain,
                                 out_part_pods, out_spread});
  });
}

}  // extern "C"
