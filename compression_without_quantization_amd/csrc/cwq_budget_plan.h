// cwq_budget_plan.h -- what a call whose blocks carry a bit count each launches
// (DESIGN.md 4c): from the facts the device reports about the blocks sorted by
// budget to the refusal or the buckets, defined once for the three entry points
// and checked on the host by tests/test_budget_plan.py.  Pure functions of the
// facts and the call's shape (roff is offset, never read); nothing from HIP.
#pragma once
#include <stdint.h>

#include "cwq_dispatch.h"
#include "cwq_workspace.h"

namespace cwq {

// What the host reads back (one copy) to launch the buckets of a sorted CSR
// call: bucket b holds the sorted rows [start[b], start[b] + counts[b]), their
// dims[b] dims lie at [pre[b], pre[b] + dims[b]) of the sorted arrays, and none
// of its blocks is longer than maxd[b].  bad_len: blocks of negative length
// (they count as empty everywhere).  Bin 31: bit counts outside [0, 30].
struct VbcFacts {
  int64_t dims[32], maxd[32], pre[32];
  uint32_t counts[32], start[32];
  int64_t bad_len;
};
static_assert(sizeof(VbcFacts) == kVbcFactsBytes, "var_csr_ws sizes the facts by it");

// The facts of uniform blocks of d dims follow from the sort's counts.
inline VbcFacts uniform_facts(const uint32_t counts[32], int64_t d) {
  VbcFacts f{};  // bad_len = 0
  for (int64_t b = 0, row = 0; b < kVbBins; ++b) {
    f.counts[b] = counts[b];
    f.start[b] = (uint32_t)row;
    f.pre[b] = row * d;
    f.dims[b] = (int64_t)counts[b] * d;
    f.maxd[b] = counts[b] ? d : 0;
    row += counts[b];
  }
  return f;
}

// One budget's slice of the sorted arrays: rows [r0, r0 + count) and dims
// [d0, d0 + dims), none of its blocks longer than maxd (its own longest: short
// blocks stay off the long-block path).  Its launches get the arrays shifted to
// r0 / d0, the offsets block_off (relative to d0; nullptr: uniform) and the
// shape's own candidate count, tiling and path.
struct BudgetBucket {
  int bits;
  int64_t r0, d0, count, dims, maxd;
  const int64_t* block_off;
  int64_t tiles_per_block, cand_per_tile;
  bool rows_wave;
};
// Why a call is refused, in the order of the checks.  The message prints got
// and limit: bit counts outside [0, 30] of nb, blocks of negative length, the
// blocks' dims against total_dims, the longest block against max_block_dim.
enum class BudgetRefusal { None, BitsOutOfRange, BadLength, TooManyDims, BlockTooLong };
struct BudgetPlan {
  BudgetBucket buckets[kVbBins - 1];  // the non-empty ones, from 30 bits down to 0
  int n_buckets, top;                 // top: the largest bit count of a bucket (none: 0)
  int64_t sum_dims, longest;          // over the buckets
  int64_t got, limit;
};

// roff: launch_vbc_layout's (bucket b's own offsets start at roff + start[b] + b), unused
// for uniform blocks.  No rule reads n_steps yet.  (static: the library exports no name for it.)
static inline BudgetRefusal budget_plan(const VbcFacts& f, bool csr, int64_t nb,
                                        int64_t total_dims, int64_t max_block_dim, int /*n_steps*/,
                                        int prune_mode, const int64_t* roff, BudgetPlan* p) {
  *p = BudgetPlan{};
  for (int b = kVbBins - 2; b >= 0; --b) {
    p->sum_dims += f.dims[b];
    p->longest = p->longest > f.maxd[b] ? p->longest : f.maxd[b];
    if (f.counts[b] == 0) continue;
    if (p->n_buckets == 0) p->top = b;
    BudgetBucket& k = p->buckets[p->n_buckets++];
    k = {b, f.start[b], f.pre[b], f.counts[b], f.dims[b], f.maxd[b]};
    k.block_off = csr ? roff + k.r0 + b : nullptr;
    choose_tiling(k.count, (int64_t)1 << b, &k.tiles_per_block, &k.cand_per_tile);
    k.rows_wave = csr && bucket_takes_rows_wave(b, k.dims, k.count, prune_mode);
  }
  auto refuse = [&](BudgetRefusal r, int64_t got, int64_t limit) {
    p->got = got, p->limit = limit;
    return r;
  };
  if (f.counts[31] != 0) return refuse(BudgetRefusal::BitsOutOfRange, f.counts[31], nb);
  if (f.bad_len != 0) return refuse(BudgetRefusal::BadLength, f.bad_len, 0);
  if (p->sum_dims > total_dims) return refuse(BudgetRefusal::TooManyDims, p->sum_dims, total_dims);
  if (p->longest > max_block_dim)
    return refuse(BudgetRefusal::BlockTooLong, p->longest, max_block_dim);
  return BudgetRefusal::None;
}

}  // namespace cwq
