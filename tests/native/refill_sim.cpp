// Host replay of how k_encode_prune hands the rows of a wave's share to its
// lanes (csrc/cwq_refill.h; the loop's tail in csrc/cwq_kernels.hip): static
// rows by stride, pool rows by rank.  Which lanes finish in an iteration is
// random here; the hand-out has to start every row of [0, R) exactly once, and
// no other, whatever the lanes do.  tests/test_refill_plan.py builds and runs
// this; it prints "R S pool_start" per share size and exits 0, or says what
// broke and exits 1.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_refill.h"

namespace {

int g_fail = 0;
#define CHECK(c, ...)                    \
  do {                                   \
    if (!(c)) {                          \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");                 \
      if (++g_fail > 20) return;         \
    }                                    \
  } while (0)

// one wave's loop over a share of R rows of G Philox blocks each; a lane on a
// row finishes it with probability p_done per iteration (at the latest after
// G iterations, as a row of G units does)
void run(uint32_t R, uint32_t G, double p_done, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::bernoulli_distribution fin(p_done);
  const uint32_t S = cwq::refill_static_rows(R);
  const uint32_t ng_end = R * G, ng_stat = S * G;
  uint32_t wnext_g = cwq::refill_pool_start(S) * G;
  std::vector<uint32_t> started(R, 0u);
  uint32_t ng[64], units[64];
  bool active[64];
  bool any = false;
  for (uint32_t l = 0; l < 64; ++l) {
    ng[l] = l * G;
    units[l] = 0;
    active[l] = ng[l] < ng_end;
    if (active[l]) ++started[l];
    any = any || active[l];
  }
  uint64_t iters = 0, slow = 0;
  while (any) {
    ++iters;
    CHECK(iters <= (uint64_t)R * G + 64, "R=%u G=%u: the loop does not end", R, G);
    bool done[64], pool[64], any_pool = false;
    for (uint32_t l = 0; l < 64; ++l) {
      ++units[l];
      done[l] = !active[l] || units[l] == G || fin(rng);
      if (done[l]) {
        CHECK(ng[l] <= UINT32_MAX - 64u * G, "R=%u G=%u lane %u: ng + 64 G wraps", R, G, l);
        ng[l] += 64u * G;
        units[l] = 0;
      }
      pool[l] = done[l] && ng[l] >= ng_stat;
      any_pool = any_pool || pool[l];
    }
    if (any_pool) {
      ++slow;
      uint32_t rank = 0;
      for (uint32_t l = 0; l < 64; ++l)
        if (pool[l]) ng[l] = wnext_g + (rank++) * G;
      wnext_g += rank * G;
      wnext_g = wnext_g < ng_end ? wnext_g : ng_end;
      any = false;
      for (uint32_t l = 0; l < 64; ++l) {
        const bool a = ng[l] < ng_end;
        // the compare may change `active` only for the lanes refilled here
        CHECK(pool[l] || a == active[l], "R=%u G=%u lane %u: active changed without a refill", R,
              G, l);
        active[l] = a;
        any = any || a;
      }
    } else {
      // the loop carries the active mask over: no lane may be out of range
      // (an inactive lane is finished every iteration and takes the refill)
      for (uint32_t l = 0; l < 64; ++l)
        CHECK(active[l] && ng[l] < ng_end, "R=%u G=%u lane %u: out of range on the fast path", R,
              G, l);
    }
    for (uint32_t l = 0; l < 64; ++l) {
      CHECK(ng[l] < ng_end + 128u * G, "R=%u G=%u lane %u: ng = %u past its bound", R, G, l,
            ng[l]);
      if (done[l] && active[l]) {
        CHECK(ng[l] % G == 0, "R=%u G=%u lane %u: ng = %u is no row", R, G, l, ng[l]);
        ++started[ng[l] / G];
        // a static row belongs to the lane l = row % 64
        if (ng[l] < ng_stat)
          CHECK((ng[l] / G) % 64u == l, "R=%u G=%u: lane %u on row %u", R, G, l, ng[l] / G);
      }
    }
  }
  for (uint32_t r = 0; r < R; ++r)
    CHECK(started[r] == 1u, "R=%u G=%u p=%.2f: row %u started %u times", R, G, p_done, r,
          started[r]);
  (void)slow;
}

}  // namespace

int main() {
  const uint32_t shares[] = {0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 1000, 16384};
  for (uint32_t R : shares) {
    const uint32_t S = cwq::refill_static_rows(R);
    std::printf("%u %u %u\n", R, S, cwq::refill_pool_start(S));
    if (S % 64u != 0 || (uint64_t)S * 8u > (uint64_t)R * 7u || (R < 128 && S != 0) ||
        (R >= 128 && ((uint64_t)S + 64u) * 8u <= (uint64_t)R * 7u)) {
      std::printf("FAIL: S(%u) = %u\n", R, S);
      return 1;
    }
    uint64_t seed = 1;
    for (uint32_t G : {2u, 8u, 16u})
      for (double p : {0.0, 0.05, 0.4, 0.9, 1.0})
        for (int rep = 0; rep < 3; ++rep) run(R, G, p, seed++ * 0x9e3779b97f4a7c15ull + R);
  }
  // a share of 2^24 Philox blocks
  for (uint32_t G : {2u, 16u}) run((1u << 24) / G, G, 0.9, 7);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
