// Host build of the beam encoder's dispatch rule (csrc/cwq_dispatch.h) for
// tests/test_beam_capi.py.  Test-only shim; not part of the product.
#include <stdint.h>
#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"

extern "C" {
int bp_path(int64_t max_d) { return cwq::beam_plan(max_d) == cwq::BeamPath::WavePerRow ? 1 : 0; }
int64_t bp_tiles_cap(int64_t nb) { return cwq::beam_tiles_cap(nb); }
int64_t bp_tiles_per_block(int path, int64_t nb, int64_t n_cand, int quarter) {
  return cwq::beam_tiles_per_block(path ? cwq::BeamPath::WavePerRow : cwq::BeamPath::LanePerRow,
                                   nb, n_cand, quarter != 0);
}
}
