// Host build of the budget calls' plan (csrc/cwq_budget_plan.h) with the rules
// it reads (csrc/cwq_dispatch.h) for tests/test_budget_plan.py.  Test-only
// shim; not part of the product.
#include <stdint.h>
#include <string.h>

#include "../../compression_without_quantization_amd/csrc/cwq_budget_plan.h"

namespace {
using namespace cwq;

// The facts as 5 x 32 + 1 int64: dims, maxd, pre, counts, start, then bad_len.
constexpr int kFactWords = 5 * 32 + 1;
VbcFacts facts_in(const int64_t* v) {
  VbcFacts f;
  for (int b = 0; b < 32; ++b) {
    f.dims[b] = v[b];
    f.maxd[b] = v[32 + b];
    f.pre[b] = v[64 + b];
    f.counts[b] = (uint32_t)v[96 + b];
    f.start[b] = (uint32_t)v[128 + b];
  }
  f.bad_len = v[160];
  return f;
}
}  // namespace

extern "C" {

int bp_fact_words(void) { return kFactWords; }

void bp_uniform_facts(const uint32_t* counts, int64_t d, int64_t* out) {
  const VbcFacts f = uniform_facts(counts, d);
  for (int b = 0; b < 32; ++b) {
    out[b] = f.dims[b];
    out[32 + b] = f.maxd[b];
    out[64 + b] = f.pre[b];
    out[96 + b] = f.counts[b];
    out[128 + b] = f.start[b];
  }
  out[160] = f.bad_len;
}

// head = refusal, got, limit, n_buckets, top, sum_dims, longest; buckets: 10
// int64 each (bits, r0, d0, count, dims, maxd, block_off - roff in entries or
// -1 when null, tiles_per_block, cand_per_tile, rows_wave).  Returns the refusal.
int bp_plan(const int64_t* facts, int csr, int64_t nb, int64_t total_dims, int64_t max_block_dim,
            int n_steps, int prune_mode, int64_t* head, int64_t* buckets) {
  static int64_t roff[(1 << 16) + 33];  // offset, never read: nb <= 2^16 here
  BudgetPlan p;
  memset(&p, 0xff, sizeof(p));
  const BudgetRefusal r = budget_plan(facts_in(facts), csr != 0, nb, total_dims, max_block_dim,
                                      n_steps, prune_mode, roff, &p);
  head[0] = (int64_t)r;
  head[1] = p.got;
  head[2] = p.limit;
  head[3] = p.n_buckets;
  head[4] = p.top;
  head[5] = p.sum_dims;
  head[6] = p.longest;
  for (int i = 0; i < p.n_buckets; ++i) {
    const BudgetBucket& k = p.buckets[i];
    int64_t* o = buckets + 10 * i;
    o[0] = k.bits, o[1] = k.r0, o[2] = k.d0, o[3] = k.count, o[4] = k.dims, o[5] = k.maxd;
    o[6] = k.block_off ? (int64_t)(k.block_off - roff) : -1;
    o[7] = k.tiles_per_block, o[8] = k.cand_per_tile, o[9] = k.rows_wave;
  }
  return (int)r;
}

void bp_choose_tiling(int64_t nb, int64_t n_cand, int64_t* out) {
  choose_tiling(nb, n_cand, &out[0], &out[1]);
}
int bp_rows_wave(int bits, int64_t dims, int64_t count, int prune) {
  return bucket_takes_rows_wave(bits, dims, count, prune);
}
}
