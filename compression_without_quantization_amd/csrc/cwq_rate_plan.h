// cwq_rate_plan.h -- the launches of one cwq_rate_table call (cwq_ratetable.hip,
// DESIGN.md 4j), as a pure function of the call's shape: the levels launch that
// scores rows [0, 2^L) of every block once, and the budgets above L that each
// take one launch_encode.  tests/test_rate_plan.py holds it to a table of
// shapes on the host.  Nothing here needs HIP; rate_level alone also runs on the device.
#pragma once
#include <stdint.h>

#include "cwq_dispatch.h"

#if defined(__HIPCC__)
#define CWQ_RATE_HD __host__ __device__ inline
#else
#define CWQ_RATE_HD inline
#endif

namespace cwq {

// The levels launch covers every budget below kCsrPrunedMinCand candidates:
// budgets 0 .. kRateMaxLevel, rows [0, 2^kRateMaxLevel).
constexpr int kRateMaxLevel = 11;
constexpr int kRateLevels = kRateMaxLevel + 1;  // lkeys holds this many u64 per block
static_assert(((int64_t)1 << kRateLevels) == kCsrPrunedMinCand,
              "the levels launch ends where the screened encoders begin");

// Level of candidate row n: 0 for row 0, else 32 - clz(n); level r >= 1 is rows
// [2^(r-1), 2^r), so budget b's candidates are levels 0 .. b.
CWQ_RATE_HD int rate_level(uint32_t n) { return n ? 32 - __builtin_clz(n) : 0; }

struct RateShape {
  bool csr;       // ragged blocks (block_off given); false: uniform blocks of ud dims
  int64_t ud;     // uniform block length (csr: unused)
  int64_t max_d;  // longest block (uniform: ud); -1: unknown
  int64_t nb;
  int max_bits;   // B
};

struct RatePlan {
  int levels;               // L = min(B, kRateMaxLevel): the levels launch's budgets 0 .. L
  bool long_rows;           // blocks of at least CWQ_CSR_COOP_MIN_D dims take a wave per row
                            // (shorter blocks of the same call keep a lane per row)
  int64_t tiles_per_block;  // the levels launch: tiles of rows_per_tile rows (a multiple of
  int64_t rows_per_tile;    // 256) over [0, 2^L), choose_tiling's split
  int64_t tiles;            // nb * tiles_per_block
  unsigned workgroups;      // of 256 threads; 0: no block, nothing is launched
  int high_first;           // budgets high_first .. B take one launch_encode each, highest
  int high_count;           // first; high_count == 0: none
};

constexpr unsigned kRateGridCap = 1u << 16;  // the levels launch strides over the tiles beyond

inline RatePlan rate_plan(const RateShape& s) {
  RatePlan p{};
  p.levels = s.max_bits < kRateMaxLevel ? s.max_bits : kRateMaxLevel;
  // rows count as long by the rule of the budget buckets (bucket_takes_rows_wave):
  // from CWQ_CSR_COOP_MIN_D dims a lane per row leaves the chip idle below
  // kCsrPrunedMinCand candidates.  An unknown length may be long.
  p.long_rows = s.max_d < 0 || s.max_d >= CWQ_CSR_COOP_MIN_D;
  choose_tiling(s.nb, (int64_t)1 << p.levels, &p.tiles_per_block, &p.rows_per_tile);
  p.tiles = s.nb > 0 ? s.nb * p.tiles_per_block : 0;
  p.workgroups = s.nb > 0 ? grid_for(p.tiles, 1, kRateGridCap) : 0u;
  p.high_first = kRateLevels;
  p.high_count = s.max_bits > kRateMaxLevel ? s.max_bits - kRateMaxLevel : 0;
  return p;
}

}  // namespace cwq
