// Host build of backfitting's dispatch rules (csrc/cwq_dispatch.h) for
// tests/test_backfit_capi.py.  Test-only shim; not part of the product.
#include <stdint.h>
#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"

extern "C" {
// 0: a wave per block, 1: a lane per block
int bf_path(int64_t max_d, int64_t nb) {
  return cwq::backfit_plan(max_d, nb) == cwq::BackfitPath::LanePerBlock ? 1 : 0;
}
int64_t bf_lane_min_blocks() { return cwq::kBackfitLaneMinBlocks; }
// The encoder path of a scoring launch (EncodePath's order), keys_only as given.
int bf_encode_path(int csr, int64_t ud, int64_t max_d, int64_t nb, int64_t n_cand, int prune,
                   int keys_only) {
  cwq::EncodeShape s = {csr != 0, ud, max_d, nb, n_cand, prune, false};
  s.keys_only = keys_only != 0;
  const cwq::EncodePlan p = cwq::encode_plan(s);
  return (int)p.path * 2 + (p.self_finalizing ? 1 : 0);
}
}
