// Host replay of how k_encode_prune hands the rows of a wave's share to its
// lanes when the static rows go downwards (CWQ_BORROW_REFILL; the loop's tail
// in csrc/cwq_kernels.hip), in the kernel's 32-bit arithmetic.  A lane carries
// ng = (row - w0) G.  It starts on its last static row, l + S - 64, and steps
// down with ng -= 64 G; the subtract's borrow, taken for the finished lanes
// only, puts a lane into the mask `left`, and the finished lanes of `left`
// take pool rows by rank in the same iteration.  Which lanes finish in an
// iteration is random here.  Checked, whatever the lanes do:
//   * every row of [0, R) is started exactly once, and no other; a static row
//     by its own lane (row % 64);
//   * the only subtract that wraps outside `left` is the one on row l, and a
//     lane whose ng has wrapped takes a pool row (or becomes inactive) before
//     the next iteration forms its Philox block;
//   * the Philox block of every visit, w0 G + ng + g with g < G, is below 2^32
//     as an integer, so that round 0's product M0 ng + M0 (w0 G + g) is
//     M0 (w0 G + ng + g) in 64 bits (csrc/cwq_philox_lo.h), for a wave at
//     row 0 and for the last wave of a stream whose blocks end at 2^32;
//   * no lane is out of range on the path that skips the range test: the
//     iterations without a pool refill, and the refills whose counter shows
//     that every row handed out is in range.
// tests/test_refill_desc_plan.py builds and runs this; it prints "ok" and
// exits 0, or says what broke and exits 1.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_philox_lo.h"
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

// one wave's loop over a share of R rows of G Philox blocks each, the wave's
// first row being w0 (w0g = w0 G mod 2^32, as the kernel holds it); a lane on
// a row finishes it with probability p_done per iteration (at the latest
// after G iterations, as a row of G units does)
void run(uint32_t R, uint32_t G, uint64_t w0, double p_done, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::bernoulli_distribution fin(p_done);
  const uint32_t S = cwq::refill_static_rows(R);
  const uint32_t ng_end = R * G, ng_stat = S * G;
  const uint32_t w0g = (uint32_t)(w0 * G);
  CHECK((w0 + R) * (uint64_t)G <= (1ull << 32), "R=%u G=%u: the share passes 2^32 blocks", R, G);
  uint32_t wnext_g = cwq::refill_pool_start(S) * G;
  const uint32_t ng_first = ng_stat != 0u ? ng_stat - 64u * G : 0u;
  std::vector<uint32_t> started(R, 0u);
  uint32_t ng[64], units[64];
  bool active[64], left[64], wrapped[64];
  bool any = false;
  for (uint32_t l = 0; l < 64; ++l) {
    ng[l] = ng_first + l * G;
    units[l] = 0;
    left[l] = ng_stat == 0u;
    wrapped[l] = false;
    active[l] = ng[l] < ng_end;
    if (active[l]) ++started[ng[l] / G];
    any = any || active[l];
  }
  uint64_t iters = 0;
  while (any) {
    ++iters;
    CHECK(iters <= (uint64_t)R * G + 64, "R=%u G=%u: the loop does not end", R, G);
    // the visit: every lane forms a Philox block; an active lane's must be a
    // real one, and no lane may come here with a wrapped ng
    for (uint32_t l = 0; l < 64; ++l) {
      CHECK(!wrapped[l], "R=%u G=%u lane %u: reaches the Philox call with a wrapped ng", R, G, l);
      if (!active[l]) continue;
      const uint32_t g = units[l];  // any group below G
      const uint64_t blk = (uint64_t)w0 * G + ng[l] + g;
      CHECK(blk < (1ull << 32), "R=%u G=%u lane %u: block %llu", R, G, l, (unsigned long long)blk);
      const uint64_t p = cwq::philox_round0_product(ng[l], cwq::philox_round0_addend(w0g + g));
      CHECK(p == (uint64_t)cwq::kPhiloxM0 * (uint32_t)blk, "R=%u G=%u lane %u: round 0's product",
            R, G, l);
    }
    bool done[64], pool[64], any_pool = false;
    for (uint32_t l = 0; l < 64; ++l) {
      ++units[l];
      done[l] = !active[l] || units[l] == G || fin(rng);
      pool[l] = false;
      if (done[l]) {
        const bool borrow = ng[l] < 64u * G;
        // outside `left` the borrow comes on the lane's own row l and nowhere else
        if (!left[l])
          CHECK(borrow == (ng[l] == l * G), "R=%u G=%u lane %u: borrow on ng = %u", R, G, l, ng[l]);
        ng[l] -= 64u * G;
        wrapped[l] = borrow;
        left[l] = left[l] || borrow;
        units[l] = 0;
        pool[l] = left[l];
      }
      any_pool = any_pool || pool[l];
    }
    bool compared = false;
    if (any_pool) {
      uint32_t rank = 0;
      for (uint32_t l = 0; l < 64; ++l)
        if (pool[l]) {
          CHECK(wnext_g <= UINT32_MAX - 64u * G, "R=%u G=%u: pool row wraps", R, G);
          ng[l] = wnext_g + (rank++) * G;
          wrapped[l] = false;
        }
      const uint32_t want = wnext_g + rank * G;
      if (want <= ng_end) {  // no compare: the refilled lanes are active, the others as before
        wnext_g = want;
        for (uint32_t l = 0; l < 64; ++l) {
          if (pool[l]) active[l] = true;
          CHECK(active[l] == (ng[l] < ng_end), "R=%u G=%u lane %u: skipped compare is wrong", R, G,
                l);
        }
      } else {
        wnext_g = ng_end;
        compared = true;
        for (uint32_t l = 0; l < 64; ++l) {
          const bool a = ng[l] < ng_end;
          // the compare may change `active` only for the lanes refilled here
          CHECK(pool[l] || a == active[l], "R=%u G=%u lane %u: active changed without a refill", R,
                G, l);
          active[l] = a;
        }
      }
    }
    (void)compared;
    any = false;
    for (uint32_t l = 0; l < 64; ++l) {
      any = any || active[l];
      // the range test is needed in the pool branch only: elsewhere the
      // carried `active` is what the compare would give
      if (!pool[l])
        CHECK(!wrapped[l] && active[l] == (ng[l] < ng_end),
              "R=%u G=%u lane %u: ng = %u out of range off the pool branch", R, G, l, ng[l]);
      // an inactive lane is finished every iteration and in `left`
      if (!active[l]) CHECK(left[l], "R=%u G=%u lane %u: inactive outside left", R, G, l);
      if (done[l] && active[l]) {
        CHECK(ng[l] % G == 0, "R=%u G=%u lane %u: ng = %u is no row", R, G, l, ng[l]);
        ++started[ng[l] / G];
        // a static row belongs to the lane l = row % 64, and is taken outside `left`
        if (ng[l] < ng_stat)
          CHECK((ng[l] / G) % 64u == l && !left[l], "R=%u G=%u: lane %u on row %u", R, G, l,
                ng[l] / G);
        else
          CHECK(left[l], "R=%u G=%u lane %u: pool row %u outside left", R, G, l, ng[l] / G);
      }
    }
  }
  for (uint32_t r = 0; r < R; ++r)
    CHECK(started[r] == 1u, "R=%u G=%u p=%.2f: row %u started %u times", R, G, p_done, r,
          started[r]);
}

}  // namespace

int main() {
  const uint32_t shares[] = {0, 1, 63, 64, 65, 127, 128, 129, 192, 255, 256, 1000, 16384};
  uint64_t seed = 1;
  for (uint32_t R : shares)
    for (uint32_t G : {2u, 8u, 16u})
      // a wave at row 0, and the last wave of a stream of 2^32 blocks: w1 G = 2^32
      for (uint64_t w0 : {(uint64_t)0, (uint64_t)((1ull << 32) / G - R)})
        for (double p : {0.0, 0.05, 0.4, 0.9, 1.0})
          for (int rep = 0; rep < 3; ++rep) run(R, G, w0, p, seed++ * 0x9e3779b97f4a7c15ull + R);
  // a share of 2^24 Philox blocks, at the end of the stream
  for (uint32_t G : {2u, 16u}) run((1u << 24) / G, G, ((1ull << 32) - (1u << 24)) / G, 0.9, 7);
  if (g_fail) return 1;
  std::printf("ok\n");
  return 0;
}
