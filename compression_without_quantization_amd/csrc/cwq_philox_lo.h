// cwq_philox_lo.h -- Philox-10 of a counter (c0, 0, c2, c3) whose c2, c3 and
// key are the same for many blocks (a stream's blocks below 2^32), written so
// that the host can compile it too: tests/native/philox_fold_check.cpp holds
// it to cwq_math.h's philox10.  The kernels reach it through cwq_device.h.
//
// Rounds 0-2 carry terms that depend on the stream alone: round 0's n0 and
// round 1's products of it, round 1's c3.  Their XORs with the round keys are
// folded per stream into four words (PhiloxLo), so each of those rounds needs
// one two-operand XOR with such a word instead of a three-input one.
//
// Round 0's only per-block work is the product M0 * c0.  Where a block index
// is a sum X + g with M0 * g at hand (philox_round0_addend), the product is
// M0 * X + (M0 * g) taken in 64 bits: equal to M0 * (X + g) whenever X + g is
// below 2^32, because then neither side wraps (both are below 2^64).  The
// multiply-add that forms it is the multiply round 0 needs anyway.
#pragma once
#include <stdint.h>

#include "cwq_math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define CWQ_XOR3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)  // one v_bitop3_b32
#else
#define CWQ_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#endif

namespace cwq {

struct PhiloxLo {
  uint32_t A, B, C, D;
};

// the four words of a stream (the device wraps them in an opaque move:
// philox_lo_key in cwq_device.h)
CWQ_HD PhiloxLo philox_lo_words(const PhiloxStream& s) {
  const uint64_t p1 = (uint64_t)kPhiloxM1 * s.c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ s.k0;       // round 0's n0
  const uint64_t q0 = (uint64_t)kPhiloxM0 * n0;           // round 1's first product
  PhiloxLo o;
  o.A = s.c3 ^ s.k1;                                      // round 0: n2 = hi(M0 c0) ^ A
  o.B = (uint32_t)p1 ^ (s.k0 + kPhiloxW0);                // round 1: n0 = hi(M1 n2) ^ B
  o.C = (uint32_t)(q0 >> 32) ^ (s.k1 + kPhiloxW1);        // round 1: n2 = lo(M0 c0) ^ C
  o.D = (uint32_t)q0 ^ (s.k1 + 2u * kPhiloxW1);           // round 2: n2 = hi(M0 c0') ^ D
  return o;
}

// M0 * g: what a block index's constant part g adds to round 0's product
CWQ_HD uint64_t philox_round0_addend(uint32_t g) { return (uint64_t)kPhiloxM0 * g; }
// round 0's product of the block X + g, g given by its addend; X + g < 2^32
CWQ_HD uint64_t philox_round0_product(uint32_t X, uint64_t addend) {
  return (uint64_t)kPhiloxM0 * X + addend;
}

// Philox-10 of (c0, 0, c2, c3) from round 0's product p0 = M0 * c0.
// k0, k1: the stream's key (callers may pass it through an opaque move)
CWQ_HD U4 philox10_lo_p0(uint64_t p0, const PhiloxLo& K, uint32_t k0, uint32_t k1) {
  const uint32_t r0n2 = (uint32_t)(p0 >> 32) ^ K.A;             // round 0
  const uint64_t q1 = (uint64_t)kPhiloxM1 * r0n2;               // round 1
  uint32_t x0 = (uint32_t)(q1 >> 32) ^ K.B;
  uint32_t x1 = (uint32_t)q1;
  uint32_t x2 = (uint32_t)p0 ^ K.C;
  const uint64_t s0 = (uint64_t)kPhiloxM0 * x0;                 // round 2
  const uint64_t s1 = (uint64_t)kPhiloxM1 * x2;
  x0 = CWQ_XOR3((uint32_t)(s1 >> 32), x1, k0 + 2u * kPhiloxW0);
  x2 = (uint32_t)(s0 >> 32) ^ K.D;
  x1 = (uint32_t)s1;
  uint32_t x3 = (uint32_t)s0;
  k0 += 3u * kPhiloxW0;
  k1 += 3u * kPhiloxW1;
#pragma unroll
  for (int r = 3; r < 10; ++r) {
    const uint64_t a0 = (uint64_t)kPhiloxM0 * x0;
    const uint64_t a1 = (uint64_t)kPhiloxM1 * x2;
    const uint32_t n0 = CWQ_XOR3((uint32_t)(a1 >> 32), x1, k0);
    const uint32_t n2 = CWQ_XOR3((uint32_t)(a0 >> 32), x3, k1);
    x1 = (uint32_t)a1;
    x3 = (uint32_t)a0;
    x0 = n0;
    x2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return U4{x0, x1, x2, x3};
}

// the same from the block index itself
CWQ_HD U4 philox10_lo(uint32_t c0, const PhiloxLo& K, uint32_t k0, uint32_t k1) {
  return philox10_lo_p0((uint64_t)kPhiloxM0 * c0, K, k0, k1);
}

}  // namespace cwq
