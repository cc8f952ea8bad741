// cwq_dispatch.h -- which encoder path one launch_encode call takes, defined
// once for the workspace layout (cwq_capi.hip), the launchers
// (cwq_kernels.hip) and the host, where tests/test_encode_plan.py checks a
// table of shapes against it (DESIGN.md "Encode dispatch"); and which decoder
// kernel one launch_decode call takes (DESIGN.md "Decode dispatch",
// tests/test_decode_plan.py).
//
// Everything here is a pure function of the call's shape; no pointer is read.
// Host only: no kernel needs it, and it includes nothing from HIP.
#pragma once
#include <stdint.h>

// Tuning switches of the dispatch (tools/variants.sh builds with -D...).
#ifndef CWQ_CSR_LDS_DIMS
#define CWQ_CSR_LDS_DIMS 1024  // general pruned kernel: blocks up to this d keep their
                               // screening constants in LDS (longer: abp records)
#endif
#ifndef CWQ_CSR_COOP_MIN_D
#define CWQ_CSR_COOP_MIN_D 256  // rows of at least this many dims count as long: the general
                                // pruned kernel walks them cooperatively, and a budget bucket
                                // of this mean length takes k_encode_rows_wave
#endif
#ifndef CWQ_CSR_COOP_ROWS_PER_LANE
#define CWQ_CSR_COOP_ROWS_PER_LANE 8  // cooperative rows below this many rows per lane, for
#endif                                // blocks of at least CWQ_CSR_COOP_MIN_D dims
#ifndef CWQ_SMALL_MIN_CAND
#define CWQ_SMALL_MIN_CAND 64  // fewer candidates: the exact kernel (screening would not pay)
#endif
#ifndef CWQ_FUSED_DMAX
#define CWQ_FUSED_DMAX 64  // longest block of the small pipeline
#endif
#ifndef CWQ_SMALL_FUSED
#define CWQ_SMALL_FUSED 1  // 0: the three-kernel path for every block length (d <= 64 too)
#endif
#ifndef CWQ_SMALL_PIPE
#define CWQ_SMALL_PIPE 1  // 0: the three-kernel path for these shapes too
#endif
#ifndef CWQ_VAR_ROWS_WAVE
#define CWQ_VAR_ROWS_WAVE 1  // 0: every bucket on the paths it took before (A/B builds)
#endif
#ifndef CWQ_ENCODE_SPLIT
#define CWQ_ENCODE_SPLIT 3  // most parts a multi-step CSR encode forks into
#endif
#ifndef CWQ_SPLIT_FEW
#define CWQ_SPLIT_FEW 3  // parts of a cooperative (few long rows) launch
#endif
#ifndef CWQ_DECODE_GLDS
#define CWQ_DECODE_GLDS 1  // 0: the register-prefetch decoder for single-step codes too
#endif

namespace cwq {

// From this many candidates per block the general pruned kernel takes a
// screened launch; below, the small-candidate paths.
constexpr int64_t kCsrPrunedMinCand = 4096;
constexpr int64_t kChipLanes = 1536 * 256;  // lanes the whole chip holds

#ifndef CWQ_TARGET_TILES
#define CWQ_TARGET_TILES 16384  // tiles per launch the tiling aims for (tuning builds)
#endif
inline void choose_tiling(int64_t nb, int64_t n_cand, int64_t* tiles_per_block,
                          int64_t* cand_per_tile) {
  const int64_t kTargetTiles = CWQ_TARGET_TILES;
  int64_t want = nb > 0 ? (kTargetTiles + nb - 1) / nb : 1;
  int64_t max_split = (n_cand + 255) / 256;  // at least one candidate per lane
  if (want > max_split) want = max_split;
  if (want < 1) want = 1;
  int64_t cpt = (n_cand + want - 1) / want;
  cpt = (cpt + 255) / 256 * 256;
  if (cpt < 256) cpt = 256;
  *cand_per_tile = cpt;
  *tiles_per_block = (n_cand + cpt - 1) / cpt;
}

// The tile queue of k_encode_prune (launch_prune_t): a persistent grid of
// queue_grid workgroups draws tiles from a counter in the workspace.  Only for
// tiles of real work: with tiny tiles (C1: 16 candidates) the counter's reset
// and a round trip per tile cost more than the slots they keep busy (C1 0.039
// -> 0.065 ms with the queue), and only with more tiles than the grid holds.
#ifndef CWQ_QUEUE_GRID
#define CWQ_QUEUE_GRID 1536
#endif
#ifndef CWQ_QUEUE_MIN_CPT
#define CWQ_QUEUE_MIN_CPT 4096
#endif
inline bool takes_tile_queue(int64_t ntiles, int64_t cand_per_tile, int64_t queue_grid) {
  return ntiles < (1LL << 31) && cand_per_tile >= CWQ_QUEUE_MIN_CPT && ntiles > queue_grid;
}

struct EncodeShape {
  bool csr;        // ragged blocks (block_off given); false: uniform blocks of ud dims
  int64_t ud;      // uniform block length (csr: unused)
  int64_t max_d;   // longest block (uniform: ud); -1: unknown
  int64_t nb;
  int64_t n_cand;  // 2^n_bits_per_step
  int prune;       // cwq_options.prune_mode
  bool rows_wave;  // the caller forces k_encode_rows_wave (bucket_takes_rows_wave)
  // the caller wants the step's argmax keys and nothing else (backfitting,
  // DESIGN.md 4g): the small pipeline writes indices and sample itself, so its
  // shapes take the three-kernel path
  bool keys_only = false;
};

enum class EncodePath { RowsWave, UniformPruned, CsrPruned, SmallPipe, SmallThree, Eval };

struct EncodePlan {
  EncodePath path;
  bool coop;             // CsrPruned: long rows are walked cooperatively by 16 lanes
  bool self_finalizing;  // the small pipeline: no k_prep_dims before, no key reset between
                         // steps, no k_encode_finalize* after them, k_destandardise folded in
};

// Blocks the uniform fast pruned kernel takes (d % 8 == 0, 8 <= d <= 64) need
// only keys + the per-dim shard constants; everything else (CSR, other d) also
// gets the general pruned kernel's screening constants, the screened
// small-candidate path's survivor slots and the small pipeline's arrays.
inline bool has_screen_arrays(bool csr, int64_t ud, int64_t nb) {
  return csr || (nb > 0 && !(ud % 8 == 0 && ud >= 8 && ud <= 64));
}
// ... and, when some block may exceed CWQ_CSR_LDS_DIMS dims, the visit-order
// records of the long blocks (max_d: the longest block; uniform: d).
inline bool has_long_block_records(bool csr, int64_t max_d, int64_t nb) {
  return has_screen_arrays(csr, max_d, nb) && max_d > CWQ_CSR_LDS_DIMS;
}

// Few long rows: fewer than CWQ_CSR_COOP_ROWS_PER_LANE candidate rows per lane
// of the chip.  The general pruned kernel then walks long rows cooperatively,
// and a forked call splits in CWQ_SPLIT_FEW parts.
inline bool few_rows(int64_t nb, int64_t n_cand) {
  return nb * n_cand < (int64_t)CWQ_CSR_COOP_ROWS_PER_LANE * kChipLanes;
}

// The path of one block range (a whole call, or one part of a forked call).
inline EncodePlan encode_plan(const EncodeShape& s) {
  const bool screened = s.prune >= 2 && has_screen_arrays(s.csr, s.ud, s.nb);
  EncodePath path = EncodePath::Eval;
  if (s.rows_wave)
    path = EncodePath::RowsWave;
  // uniform D % 8 == 0, D <= 64, Philox block index n*D/4 < 2^32
  else if (!s.csr && s.prune >= 1 && s.ud % 8 == 0 && s.ud >= 8 && s.ud <= 64 &&
           s.n_cand * (s.ud / 4) <= (1LL << 32))
    path = EncodePath::UniformPruned;
  else if (screened && s.n_cand >= kCsrPrunedMinCand)
    path = EncodePath::CsrPruned;
  else if (screened && s.n_cand >= CWQ_SMALL_MIN_CAND)
    path = CWQ_SMALL_PIPE && CWQ_SMALL_FUSED && !s.keys_only && s.max_d >= 0 &&
                   s.max_d <= CWQ_FUSED_DMAX && s.nb < (1LL << 32)
               ? EncodePath::SmallPipe
               : EncodePath::SmallThree;
  return {path, path == EncodePath::CsrPruned && few_rows(s.nb, s.n_cand),
          path == EncodePath::SmallPipe};
}

// Parts a call's block range forks into (1: no fork).  Only a multi-step CSR
// encode forks; launches of few long rows overlap best in CWQ_SPLIT_FEW parts,
// others in two (tools/stream_overlap.py).
inline int encode_fork_parts(const EncodeShape& s, int n_steps) {
  if (CWQ_ENCODE_SPLIT <= 1 || !s.csr || n_steps <= 1 || s.nb < 2) return 1;
  int k = few_rows(s.nb, s.n_cand) ? CWQ_SPLIT_FEW : 2;
  k = k < CWQ_ENCODE_SPLIT ? k : CWQ_ENCODE_SPLIT;
  return (int64_t)k < s.nb ? k : (int)s.nb;
}

// ---- beam search over steps (cwq_beam.hip) -------------------
// Which scoring kernel a beam encode takes: a lane per candidate row while the
// longest block fits the lane kernel's LDS row (CWQ_FUSED_DMAX dims), a wave
// per row otherwise (and when the longest block is unknown).
enum class BeamPath { LanePerRow, WavePerRow };
inline BeamPath beam_plan(int64_t max_d) {
  return max_d >= 0 && max_d <= CWQ_FUSED_DMAX ? BeamPath::LanePerRow : BeamPath::WavePerRow;
}
constexpr int64_t kBeamTargetTiles = 2048;  // tiles a scoring launch aims for
constexpr int64_t kBeamLaneTile = 128;      // smallest tile (rows): a row per lane
constexpr int64_t kBeamWaveTile = 4;        // ... a row per wave
// Most tiles one block is ever split into; a function of nb alone, so the
// workspace (one key list per tile) can be sized without the bit count.  The
// factor 4 is the tests' quarter-tile knob.
inline int64_t beam_tiles_cap(int64_t nb) {
  const int64_t want = nb > 0 ? (kBeamTargetTiles + nb - 1) / nb : 1;
  int64_t t = 1;
  while (t < want) t <<= 1;
  return 4 * t;
}
// Tiles per block (a power of two dividing n_cand = 2^b) of one launch.
inline int64_t beam_tiles_per_block(BeamPath path, int64_t nb, int64_t n_cand, bool quarter) {
  const int64_t mt = path == BeamPath::LanePerRow ? kBeamLaneTile : kBeamWaveTile;
  const int64_t most = n_cand > mt ? n_cand / mt : 1;  // tiles of at least mt rows
  int64_t t = beam_tiles_cap(nb) / 4;
  t = t < most ? t : most;
  if (quarter) t = 4 * t < n_cand ? 4 * t : n_cand;
  return t;
}

// ---- backfitting (cwq_backfit.hip) ---------------------------
// Who handles one block in k_backfit_accept: a wave, or a lane when no block
// exceeds CWQ_FUSED_DMAX dims and there are blocks enough for it.  A lane walks
// its block's dims one after the other (at most CWQ_FUSED_DMAX terms per step
// row), a wave takes 64 dims at a time but leaves 63 lanes idle on a row of a
// few dims.  With a wave per block the chip's 6,144 resident waves hold 6,144
// blocks; from kBackfitLaneMinBlocks blocks on a lane per block keeps as many
// lanes busy in one round (16,384 lanes = 256 waves) and the launch shrinks 64
// times.  Below it the waves are too few to matter and the wave kernel, whose
// latency per block is lower, runs.  An unknown length (-1) takes the wave kernel.
enum class BackfitPath { WavePerBlock, LanePerBlock };
constexpr int64_t kBackfitLaneMinBlocks = 16384;
inline BackfitPath backfit_plan(int64_t max_d, int64_t nb) {
  return max_d >= 0 && max_d <= CWQ_FUSED_DMAX && nb >= kBackfitLaneMinBlocks
             ? BackfitPath::LanePerBlock
             : BackfitPath::WavePerBlock;
}

// ---- greedy decoders (launch_decode, DESIGN.md "Decode dispatch") -----------
// Workgroups of a grid-stride launch: `per_block` items of `work` each, at
// least one, at most `cap`.
inline unsigned grid_for(int64_t work, int64_t per_block, unsigned cap) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// The float4 lane-per-Philox-block kernels (k_decode_q4, k_decode_q4_glds,
// k_encode_finalize_q4): uniform d % 4 == 0, d <= 256.
inline bool q4_shape(bool csr, int64_t ud) {
  return !csr && ud > 0 && ud % 4 == 0 && ud <= 256;
}

struct DecodeShape {
  bool csr;            // ragged blocks (block_off given); false: uniform blocks of ud dims
  int64_t ud;          // uniform block length (csr: unused)
  int64_t nb;
  int64_t total_dims;  // uniform: nb * ud
  int n_steps;
  bool aligned16;      // p_loc, p_scale and out_sample all lie on 16-byte boundaries
};

// General: k_decode, a thread per dim.  Q4: k_decode_q4, a lane per Philox
// block of a row, inputs prefetched in registers.  Q4Glds: k_decode_q4_glds,
// the same mapping for single-step codes, inputs streamed through LDS.
enum class DecodeKernel { General, Q4, Q4Glds };

struct DecodePlan {
  DecodeKernel kernel;
  uint32_t qpb, bpw;    // Q4*: Philox blocks per row, blocks per chunk (General: 0)
  int64_t groups;       // Q4*: wave groups of bpw * qpb blocks (General: 0)
  unsigned workgroups;  // of 256 threads; 0: nothing to launch (no block)
};

constexpr unsigned kDecodeGeneralGridCap = 16384;  // k_decode strides over the dims beyond
constexpr unsigned kDecodeQ4GridCap = 1u << 20;    // the q4 kernels over the groups beyond

inline DecodePlan decode_plan(const DecodeShape& s) {
  if (s.nb <= 0) return {DecodeKernel::General, 0u, 0u, 0, 0u};
  if (q4_shape(s.csr, s.ud) && s.aligned16) {
    const uint32_t qpb = (uint32_t)(s.ud / 4), bpw = 64u / qpb;
    const int64_t B = (int64_t)bpw * qpb;
    const int64_t groups = (s.nb + B - 1) / B;
    return {CWQ_DECODE_GLDS && s.n_steps == 1 ? DecodeKernel::Q4Glds : DecodeKernel::Q4, qpb, bpw,
            groups, grid_for(groups, 4, kDecodeQ4GridCap)};  // a wave per group
  }
  return {DecodeKernel::General, 0u, 0u, 0, grid_for(s.total_dims, 256, kDecodeGeneralGridCap)};
}

// cwq_greedy_encode_var's bucket rule.  Long rows at few candidates (DESIGN.md
// 4e): below kCsrPrunedMinCand candidates the other paths walk a row with one
// lane, so a bucket of `count` blocks at `bits` bits whose mean block reaches
// the length from which rows count as long gives every row to a wave.
// prune_mode 0 keeps k_encode_eval, as it promises.
inline bool bucket_takes_rows_wave(int bits, int64_t dims, int64_t count, int prune) {
  return CWQ_VAR_ROWS_WAVE && ((int64_t)1 << bits) < kCsrPrunedMinCand &&
         dims >= (int64_t)CWQ_CSR_COOP_MIN_D * count && prune != 0;
}

}  // namespace cwq
