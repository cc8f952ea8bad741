// Host build of the rate table's plan and workspace layout (csrc/cwq_rate_plan.h,
// rate_ws in csrc/cwq_workspace.h) for tests/test_rate_plan.py.  Test-only shim;
// not part of the product.
#include <stdint.h>

#include "../../compression_without_quantization_amd/csrc/cwq_rate_plan.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

extern "C" {

// out: levels, long_rows, tiles_per_block, rows_per_tile, tiles, workgroups,
// high_first, high_count
void rp_plan(int csr, int64_t ud, int64_t max_d, int64_t nb, int max_bits, int64_t* out) {
  const cwq::RatePlan p = cwq::rate_plan(cwq::RateShape{csr != 0, ud, max_d, nb, max_bits});
  out[0] = p.levels;
  out[1] = p.long_rows;
  out[2] = p.tiles_per_block;
  out[3] = p.rows_per_tile;
  out[4] = p.tiles;
  out[5] = p.workgroups;
  out[6] = p.high_first;
  out[7] = p.high_count;
}

int rp_level(uint32_t n) { return cwq::rate_level(n); }

// out: kRateMaxLevel, kRateLevels, kCsrPrunedMinCand, CWQ_CSR_COOP_MIN_D, kRateGridCap,
// CWQ_TARGET_TILES
void rp_consts(int64_t* out) {
  out[0] = cwq::kRateMaxLevel;
  out[1] = cwq::kRateLevels;
  out[2] = cwq::kCsrPrunedMinCand;
  out[3] = CWQ_CSR_COOP_MIN_D;
  out[4] = cwq::kRateGridCap;
  out[5] = CWQ_TARGET_TILES;
}

// out: (off, bytes) of enc, lkeys, hkeys, sample, idx; then the total, the
// encoder's own total inside enc, and the deferral layout's total (uniform
// blocks; ragged: the encoder's)
void rp_ws(int csr, int64_t nb, int64_t total_dims, int64_t max_block_dim, int max_bits,
           int64_t* out) {
  const cwq::RateWs l = cwq::rate_ws(csr != 0, nb, total_dims, max_block_dim, max_bits);
  const cwq::Region* r = &l.enc;
  for (int i = 0; i < 5; ++i) {
    out[2 * i] = (int64_t)r[i].off;
    out[2 * i + 1] = (int64_t)r[i].bytes;
  }
  out[10] = (int64_t)l.total;
  out[11] = (int64_t)l.encl.total;
  out[12] = (int64_t)(csr ? l.encl.total
                          : cwq::defer_ws(l.encl.total, nb, max_block_dim).total);
}
}
