// Host build of the beam encoder's per-block counts (csrc/cwq_beam_plan.h),
// its tiling rule (csrc/cwq_dispatch.h) and its workspace (csrc/cwq_workspace.h)
// for tests/test_beam_var_plan.py.  Test-only shim; not part of the product.
#include <stdint.h>

#include "../../compression_without_quantization_amd/csrc/cwq_beam_plan.h"
#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

extern "C" {
int bvp_live(int b, int step, int beam) { return cwq::beam_live(b, step, beam); }
int bvp_keep(int b, int step, int beam) { return cwq::beam_keep(b, step, beam); }
int bvp_clamp(int32_t b, int max_bits) { return cwq::beam_clamp_bits(b, max_bits); }
int bvp_tab_len(void) { return cwq::kBeamVarTabLen; }
int64_t bvp_tiles_cap(int64_t nb) { return cwq::beam_tiles_cap(nb); }
int64_t bvp_tiles_per_block(int path, int64_t nb, int64_t n_cand, int quarter) {
  return cwq::beam_tiles_per_block(path ? cwq::BeamPath::WavePerRow : cwq::BeamPath::LanePerRow,
                                   nb, n_cand, quarter != 0);
}
int64_t bvp_tiles_bytes(int64_t nb, int64_t total_dims, int n_steps, int beam) {
  return (int64_t)cwq::beam_ws(nb, total_dims, n_steps, beam).tiles.bytes;
}
}
