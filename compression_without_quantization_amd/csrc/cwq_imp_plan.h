// cwq_imp_plan.h -- which paths one launch_importance_encode call takes,
// defined once for the kernels and the launcher (cwq_importance.hip) and for
// the host, where tests/test_importance_plan.py checks the shapes of
// tests/importance_shapes.py against it (DESIGN.md "Importance coder paths").
//
// Everything here is a pure function of the launch's shape (group counts and
// lengths, call form); no device pointer is read.  The value gate of the
// screening pass (imp_screen_dim: scales and constants in range, finite) reads
// the inputs on the device and is not part of the plan: a group whose shape
// says "pruned" or "short" still takes the exact loop when the gate rejects it.
// Includes nothing from HIP; the same definitions compile for the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CWQ_IMP_HD __host__ __device__ __forceinline__
#else
#define CWQ_IMP_HD inline
#endif

// Tuning switches (tools/variants.sh builds with -D...).
// Groups of at most this many candidates are coded by k_imp_small (one wave
// per group, every row exact) and get no k_imp_eval tile: most groups of a
// batch of small latents draw a few dozen candidates (I2: 81% of 13,852
// groups have N <= 128, 1.6% of the candidates), and a tile's fixed cost (its
// group search, the screening constants, four barriers, the hand-out
// counter) exceeded their rows' work.  A/B (tools/variants.sh is0..is1024,
// one box, two rounds): I2's scoring 0.299 -> 0.207 ms, pln_is 0.36 -> 0.18 ms,
// I1 unchanged (8.39 / 8.41 ms); 128 and 256 tie, 1024 is slower on I1.
// 0 disables.
#ifndef CWQ_IMP_SMALL_N
#define CWQ_IMP_SMALL_N 128
#endif
// Tile size: the launch's candidates cut into about CWQ_IMP_TARGET_TILES tiles
// (a few per CU, so one image's ~600 groups do not leave most of a fixed grid
// idle), a power of two in [kImpMinCandPerTile, kImpCandPerTile].
#ifndef CWQ_IMP_TARGET_TILES
#define CWQ_IMP_TARGET_TILES 2048
#endif
#ifndef CWQ_IMP_MIN_CPT
#define CWQ_IMP_MIN_CPT 1024
#endif
#ifndef CWQ_IMP_DYNAMIC_MIN_GROUPS
#define CWQ_IMP_DYNAMIC_MIN_GROUPS 4096  // dynamic tile hand-out from this many groups
#endif
// ... or, when the host knows the launch's tile count, from this many tiles:
// below it the one-address hand-out counter (an atomic per tile from every
// workgroup) cost more than the balance it buys (I2's batch, ~4.4k tiles:
// 0.206 -> 0.185 ms static; pln_is 0.18 -> 0.13 ms; I1's 99.9k tiles need it:
// 8.40 -> 9.83 ms static)
#ifndef CWQ_IMP_DYNAMIC_MIN_TILES
#define CWQ_IMP_DYNAMIC_MIN_TILES 8192
#endif
#ifndef CWQ_IMP_PERMUTE
#define CWQ_IMP_PERMUTE 1  // 0: dynamic tiles go out in order
#endif
#ifndef CWQ_IMP_SURVIVOR_CAP
#define CWQ_IMP_SURVIVOR_CAP 1024  // survivor list of one tile; past it rows are scored in line
#endif

namespace cwq {

constexpr int64_t kImpSmallN = CWQ_IMP_SMALL_N;
constexpr int64_t kImpCandPerTile = 16384;
constexpr int64_t kImpMinCandPerTile = CWQ_IMP_MIN_CPT;
constexpr int kImpScreenMaxD = 256;   // screening pass: per-dim constants live in LDS
constexpr int64_t kImpPruneMinD = 5;  // rows of >= 5 dims take the pruned screening loop
// k_imp_tiles scans 1,024 groups per round and holds the counts of up to this
// many rounds (16,384 groups) in registers; more groups: it reads them twice
constexpr int kImpTilesRegRounds = 16;
constexpr int64_t kImpTilesRound = 1024;
constexpr uint64_t kImpPermPrime = 0x7FFFFFFFull;  // 2^31 - 1

// A group's candidate count as every kernel reads it.
CWQ_IMP_HD int64_t imp_count(int64_t n_samples) { return n_samples > 1 ? n_samples : 1; }

// The tile-size rule (k_imp_tiles on the device; the launcher on the host
// when it knows the launch's candidate count T = sum imp_count(N_g)).
CWQ_IMP_HD int64_t imp_cand_per_tile(int64_t T) {
  int64_t cpt = kImpMinCandPerTile;
  while (cpt < kImpCandPerTile && cpt * CWQ_IMP_TARGET_TILES < T) cpt <<= 1;
  return cpt;
}

// k_imp_small's groups (no tile) against k_imp_eval's.
CWQ_IMP_HD bool imp_is_small(int64_t count) { return count <= kImpSmallN; }

// Whether k_imp_tiles holds every count in registers.
CWQ_IMP_HD bool imp_tiles_in_regs(int64_t nb) {
  return (nb + kImpTilesRound - 1) / kImpTilesRound <= kImpTilesRegRounds;
}

// Dynamic hand-out (tiles drawn from a global counter) against the static
// assignment.  total_tiles: the launch's tile count when the host knows it, -1
// otherwise (then the group count decides).
CWQ_IMP_HD bool imp_dynamic_handout(int64_t total_tiles, int64_t nb) {
  return total_tiles >= 0 ? total_tiles >= CWQ_IMP_DYNAMIC_MIN_TILES
                          : nb >= CWQ_IMP_DYNAMIC_MIN_GROUPS;
}

// Dynamic hand-out order t -> tile (t * P) mod total, P = 2^31 - 1 prime (a
// permutation while total < P).  1: tiles go out in order.
// This rule and CWQ_IMP_SCREEN_BY_SHAPE are macros, which k_imp_eval expands
// in place with its own operands (`dynamic` a pointer there): the kernel
// spills scalar registers, and a call, once inlined, shifted its allocation.
#define CWQ_IMP_PERM_MULTIPLIER(dynamic, total)                                       \
  ((CWQ_IMP_PERMUTE && (dynamic) && (total) > 1 && (total) < 0x7FFFFFFFll)             \
       ? 0x7FFFFFFFull % (uint64_t)(total)                                            \
       : 1ull)
static_assert(kImpPermPrime == 0x7FFFFFFFull, "the macro's prime");
CWQ_IMP_HD uint64_t imp_perm_multiplier(bool dynamic, int64_t total) {
  return CWQ_IMP_PERM_MULTIPLIER(dynamic, total);
}

// The launch's tile size is kImpCandPerTile and the host knows it: the CPT_MAX
// instantiation of k_imp_eval.  total_cands < 0: unknown.
CWQ_IMP_HD bool imp_cpt_max(int64_t total_cands) {
  return total_cands >= 0 && imp_cand_per_tile(total_cands) == kImpCandPerTile;
}

// Every Philox block index (n d + j) / 4 of the group is below 2^32: counter
// word 1 is 0 and the screening Box-Muller takes its 32-bit form (HI0).
CWQ_IMP_HD bool imp_lo32(int64_t count, int64_t d) {
  return (uint64_t)count * (uint64_t)d <= (1ull << 34);
}

// A row may be screened at all: the per-dim constants fit the LDS arrays.
#define CWQ_IMP_SCREEN_BY_SHAPE(allow_screen, d) \
  ((allow_screen) && (d) >= 1 && (d) <= ::cwq::kImpScreenMaxD)
CWQ_IMP_HD bool imp_screen_by_shape(int allow_screen, int64_t d) {
  return CWQ_IMP_SCREEN_BY_SHAPE(allow_screen, d);
}

// Row form of one group by its shape.  Exact: a row of 0 or more than
// kImpScreenMaxD dims, or screening switched off (prune_mode below 2).
enum class ImpRowForm : uint8_t { Small = 0, Pruned = 1, Short = 2, Exact = 3 };
CWQ_IMP_HD ImpRowForm imp_row_form(int64_t count, int64_t d, int allow_screen) {
  if (imp_is_small(count)) return ImpRowForm::Small;
  if (!imp_screen_by_shape(allow_screen, d)) return ImpRowForm::Exact;
  return d >= kImpPruneMinD ? ImpRowForm::Pruned : ImpRowForm::Short;
}

// The k_imp_eval tile count of a launch from host copies of its counts
// (total_cands: sum of imp_count(N_g)).
inline int64_t imp_tile_count(const int64_t* n_samples_host, int64_t nb, int64_t total_cands) {
  const int64_t cpt = imp_cand_per_tile(total_cands);  // k_imp_tiles' rule
  int64_t tiles = 0;
  for (int64_t g = 0; g < nb; ++g) {
    const int64_t n = imp_count(n_samples_host[g]);
    tiles += imp_is_small(n) ? 0 : (n + cpt - 1) / cpt;
  }
  return tiles;
}

struct ImpLaunchPlan {
  int64_t total_cands;    // T
  int64_t cpt;            // candidates per tile
  int64_t tiles;          // k_imp_eval tiles
  int64_t small_groups;   // groups k_imp_small codes
  bool dynamic;           // tiles drawn from the counter
  bool permuted;          // ... in the permuted order
  uint64_t multiplier;    // the permutation's multiplier (1: in order)
  bool per_block, cpt_max;  // k_imp_eval<PER_BLOCK, CPT_MAX>
  bool tiles_in_regs;     // k_imp_tiles: counts in registers (else streamed twice)
};
constexpr uint8_t kImpFormHi0 = 0x80;  // row_form[g]: the group's HI0 flag

// Everything launch_importance_encode and its kernels choose by shape.
// total_known: the caller passes the launch's candidate and tile counts (the
// grouped and batch calls); else k_imp_tiles finds them on the device
// (cwq_importance_encode).  per_block_seeds: group seeds given per group (a
// batch of items).  row_form (nb entries, may be null; needs block_off_host):
// ImpRowForm of each group, | kImpFormHi0.
inline ImpLaunchPlan imp_launch_plan(const int64_t* n_samples_host, const int64_t* block_off_host,
                                     int64_t nb, bool total_known, bool per_block_seeds,
                                     int allow_screen, uint8_t* row_form = nullptr) {
  ImpLaunchPlan p = {};
  for (int64_t g = 0; g < nb; ++g) {
    const int64_t n = imp_count(n_samples_host[g]);
    p.total_cands += n;
    p.small_groups += imp_is_small(n) ? 1 : 0;
  }
  p.cpt = imp_cand_per_tile(p.total_cands);
  p.tiles = imp_tile_count(n_samples_host, nb, p.total_cands);
  p.dynamic = imp_dynamic_handout(total_known ? p.tiles : -1, nb);
  p.multiplier = imp_perm_multiplier(p.dynamic, p.tiles);
  p.permuted = p.multiplier != 1ull;
  p.per_block = per_block_seeds;
  p.cpt_max = imp_cpt_max(total_known ? p.total_cands : -1);
  p.tiles_in_regs = imp_tiles_in_regs(nb);
  if (row_form && block_off_host)
    for (int64_t g = 0; g < nb; ++g) {
      const int64_t n = imp_count(n_samples_host[g]);
      const int64_t d = block_off_host[g + 1] - block_off_host[g];
      row_form[g] = (uint8_t)imp_row_form(n, d, allow_screen) | (imp_lo32(n, d) ? kImpFormHi0 : 0);
    }
  return p;
}

}  // namespace cwq
