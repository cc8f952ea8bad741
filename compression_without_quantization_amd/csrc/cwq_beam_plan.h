// cwq_beam_plan.h -- the beam encoder's per-block counts under per-block bit
// budgets (cwq_beam_encode_var, cwq_beam.hip), as integer
// arithmetic that the kernels and the host share: tests/test_beam_var_plan.py
// drives tests/native/beam_var_plan.cpp, which checks it on the CPU.
//
// A block at b bits has L_0 = 1 live beams and L_{i+1} = min(B, L_i 2^b) after
// step i, i.e. L_i = min(B, 2^(b i)): by induction min(B, min(B, 2^(b i)) 2^b)
// = min(B, B 2^b, 2^(b (i + 1))), and B 2^b >= B.  The closed form lets every
// kernel take a block's counts from its bit count and the step alone.
//
// Pure integer functions; nothing from HIP is included.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CWQ_BEAM_PLAN_HD __host__ __device__ __forceinline__
#else
#define CWQ_BEAM_PLAN_HD inline
#endif

namespace cwq {

// Most bits per step (CWQ_MAX_BITS_PER_STEP) and with them the entries of a
// tiles-per-block table indexed by the bit count.
constexpr int kBeamVarMaxBits = 30;
constexpr int kBeamVarTabLen = kBeamVarMaxBits + 1;

// A count read from device memory, as the var call reads it: clamped to
// [0, max_bits] (max_bits itself is host-checked to lie in [0, 30]).
CWQ_BEAM_PLAN_HD int beam_clamp_bits(int32_t b, int max_bits) {
  return b < 0 ? 0 : (b > max_bits ? max_bits : (int)b);
}

// L_step: the live beams of a block at b bits when step `step` begins,
// min(beam, 2^(b step)).  64-bit: 16 << 30 and b * step do not fit in 32.
CWQ_BEAM_PLAN_HD int beam_live(int b, int step, int beam) {
  const int64_t e = (int64_t)b * (int64_t)step;
  if (e <= 0) return 1;
  if (e >= 31) return beam;  // beam <= 16 < 2^31
  const int64_t n = (int64_t)1 << e;
  return n < (int64_t)beam ? (int)n : beam;
}

// L': the keys step `step` keeps, the next step's live count.
CWQ_BEAM_PLAN_HD int beam_keep(int b, int step, int beam) { return beam_live(b, step + 1, beam); }

}  // namespace cwq
