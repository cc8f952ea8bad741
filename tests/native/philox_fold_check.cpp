// Host check of csrc/cwq_philox_lo.h against cwq_math.h's philox10: round 0's
// product taken as M0 X + (M0 g) equals M0 (X + g) in 64 bits whenever X + g
// is below 2^32, and philox10_lo_p0 fed with it (the entry k_encode_prune's
// screening loop uses) gives philox10 of the counter (X + g, 0, c2, c3).
// 10^6 random (X, g, stream) triples with g < 16, and the edges X + g =
// 2^32 - 1 and X = 0 for every g.  tests/test_refill_desc_plan.py builds and
// runs this; it prints "ok" and exits 0, or says what broke and exits 1.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../compression_without_quantization_amd/csrc/cwq_philox_lo.h"

namespace {

int g_fail = 0;

void one(uint32_t X, uint32_t g, const cwq::PhiloxStream& st) {
  const uint64_t add = cwq::philox_round0_addend(g);
  const uint64_t p0 = cwq::philox_round0_product(X, add);
  const uint32_t blk = X + g;
  bool ok = (uint64_t)X + g < (1ull << 32) && p0 == (uint64_t)cwq::kPhiloxM0 * blk;
  const cwq::PhiloxLo K = cwq::philox_lo_words(st);
  const cwq::U4 a = cwq::philox10_lo_p0(p0, K, st.k0, st.k1);
  const cwq::U4 b = cwq::philox10_lo(blk, K, st.k0, st.k1);
  const cwq::U4 w = cwq::philox10(blk, 0u, st.c2, st.c3, st.k0, st.k1);
  ok = ok && a.x == w.x && a.y == w.y && a.z == w.z && a.w == w.w;
  ok = ok && b.x == w.x && b.y == w.y && b.z == w.z && b.w == w.w;
  if (!ok && ++g_fail <= 20) std::printf("FAIL: X=%u g=%u key=%08x %08x\n", X, g, st.k0, st.k1);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20240607);
  for (int i = 0; i < 1000000; ++i) {
    const uint64_t r0 = rng(), r1 = rng(), r2 = rng();
    const uint32_t g = (uint32_t)(r0 & 15u);
    uint32_t X = (uint32_t)(r0 >> 32);
    if (X > UINT32_MAX - g) X = UINT32_MAX - g;  // X + g stays a 32-bit block index
    one(X, g, cwq::PhiloxStream{(uint32_t)r1, (uint32_t)(r1 >> 32), (uint32_t)r2, (uint32_t)(r2 >> 32)});
  }
  const cwq::PhiloxStream real = cwq::generate_key(cwq::step_seed(42, 0), 42);
  for (uint32_t g = 0; g < 16; ++g) {
    one(UINT32_MAX - g, g, real);  // X + g = 2^32 - 1
    one(0u, g, real);              // X = 0
    one(UINT32_MAX - g, g, cwq::PhiloxStream{~0u, ~0u, ~0u, ~0u});
  }
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
