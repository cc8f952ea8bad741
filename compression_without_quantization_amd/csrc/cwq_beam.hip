// cwq_beam.hip -- the greedy coder with a beam over its steps.
//
// The greedy coder keeps the one best partial sum after every step; here the
// B best are kept.  Every beam of a step is scored against the same candidate
// rows (the step's stream), so a path is still one row index per step and the
// decoders are unchanged.  With B = 1 the result is the greedy coder's.
//
// One step is four launches:
//   * score: a tile = (block g, row range [n0, n1)) per workgroup.  A row is
//     drawn once (Philox, exact Box-Muller, shard) and kept in LDS; each live
//     beam k then adds its sum, takes the log-density and folds it in the Eigen
//     order (eval_row's value).  Candidate c = k 2^b + n gets argmax_key(v, c);
//     the workgroup keeps the L' largest keys of its tile in an LDS list
//     (atomic maxima only: no retry loop) and stores the list.  Two kernels: a lane per row (blocks of at most
//     CWQ_FUSED_DMAX dims) and a wave per row (exact_row_wave's staging).
//   * select: a wave per block merges the block's tile lists into the L'
//     largest keys, sorted.  Keys are distinct, so the list is a function of
//     the candidate set alone: neither the tiling nor the order of the LDS
//     inserts can change it.
//   * advance: new beam j = its parent's sum + its row, into the other half of
//     the ping-pong beams array.
// and a final launch walks beam 0's parents back for the indices.
//
// Under per-block bit budgets (cwq_beam_encode_var) the same
// launches serve every budget at once: the kernel bodies are templates whose
// VAR form takes the block's bit count b_g from n_bits[g], clamped to
// [0, max_bits], and its live and keep counts from b_g and the step
// (cwq_beam_plan.h).  The fixed instances read the launch's own numbers, as
// they always did.  (The lane scoring kernel has the two forms as two kernels.)
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "cwq_beam_plan.h"
#include "cwq_device.h"
#include "cwq_kernels.h"

namespace cwq {
namespace {

constexpr int kLaneThreads = (int)kBeamLaneTile;
constexpr int kRowChunk = 248;  // exact_row_wave's chunk: a multiple of 8, at most 63 Philox blocks
constexpr unsigned kBeamGridCap = 4096;  // workgroups of a scoring launch (tiles are strided)

__global__ void __launch_bounds__(256) k_beam_prep(
    const float* __restrict__ t_scale, const float* __restrict__ p_loc,
    const float* __restrict__ p_scale, int64_t n, float nst, float sdiv, float rho,
    float* __restrict__ loc_s, float* __restrict__ scale_s, float* __restrict__ lognorm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float ls, ss;
    shard_consts(p_loc[i], p_scale[i], nst, sdiv, rho, ls, ss);
    loc_s[i] = ls;
    scale_s[i] = ss;
    lognorm[i] = lognorm_of(t_scale[i]);
  }
}

// The workgroup's sorted list of the lp largest keys offered so far (0: empty
// slot; no candidate's key is 0).  An insert walks the list once: slot i takes
// the larger of its key and the one carried in, and the smaller is carried on.
// Every key offered either rests in slot 0 at the end or is carried to slot 1,
// by its own walk or by the walk that displaced it, so slot 0 ends as the
// largest key offered, slot 1 as the largest of the rest, and so on: the list
// is the lp largest in decreasing order whatever the order of the inserts.
// No walk waits for another (lp atomic maxima, no retry), and the last slot,
// which only grows, is the threshold below which a key cannot enter.
__device__ __forceinline__ void top_insert(unsigned long long* top, int lp, uint64_t key) {
  if (key <= __atomic_load_n(&top[lp - 1], __ATOMIC_RELAXED)) return;
  for (int i = 0; i < lp; ++i) {
    const uint64_t old = atomicMax(&top[i], (unsigned long long)key);
    key = old < key ? old : key;  // the displaced key, or this one if the slot's was larger
    if (key == 0) return;         // an empty slot was filled: nothing is carried on
  }
}

struct ScoreArgs {
  const float* t_loc;
  const float* t_scale;
  const float* loc_s;
  const float* scale_s;
  const float* lognorm;
  const float* beams;  // this step's sums: beam k at beams + k * bstride (step 0: not read)
  int64_t bstride;
  const int64_t* block_off;
  int64_t ud, ntiles, tiles_per_block, cand_per_tile;
  int n_bits;
  SeedSpec sd;
  int32_t step;
  int live, keep, beam;  // L, L' and B
  unsigned long long* tiles;  // [ntiles][beam]
};

// What the VAR forms have beyond the fixed ones' arguments.  tpb[b] is
// beam_tiles_per_block at 2^b candidates for b <= max_bits; the rule is
// monotone in 2^b, so stride = tpb[max_bits] bounds every block's tiles and the
// tile slots of block g are [g stride, (g + 1) stride): `tiles` holds
// [nb][stride][beam], inside the [nb][beam_tiles_cap(nb)][beam] of beam_ws.
struct VarTab {
  const int32_t* n_bits;  // device [nb]; read as clamped to [0, max_bits]
  int32_t max_bits;
  int32_t stride;
  int32_t tpb[kBeamVarTabLen];
};

struct Tile {
  int64_t g, n0, n1;
  BlockSpan sp;
};
__device__ __forceinline__ Tile tile_of(const ScoreArgs& a, int64_t tile) {
  Tile t;
  t.g = tile / a.tiles_per_block;
  const int64_t tt = tile - t.g * a.tiles_per_block;
  const int64_t n_cand = (int64_t)1 << a.n_bits;
  t.n0 = tt * a.cand_per_tile;
  t.n1 = t.n0 + a.cand_per_tile < n_cand ? t.n0 + a.cand_per_tile : n_cand;
  t.sp = block_span(a.block_off, a.ud, t.g);
  return t;
}

// The tile with its block's own counts, for the kernel bodies that serve both
// forms: the fixed instances read the launch's numbers, the VAR ones the
// block's (tile slot `tile` names block g = tile / stride and its tile
// tt = tile % stride).
struct BlockTile : Tile {
  int b, live, keep;  // the block's bits, L and L'
  bool skip;          // VAR: a slot past the block's own tiles
};
template <bool VAR>
__device__ __forceinline__ BlockTile block_tile_of(const ScoreArgs& a, const VarTab* vt,
                                                   int64_t tile) {
  BlockTile t;
  if constexpr (VAR) {
    t.g = tile / vt->stride;
    const int64_t tt = tile - t.g * vt->stride;
    t.b = beam_clamp_bits(vt->n_bits[t.g], vt->max_bits);
    const int64_t tpb = vt->tpb[t.b];
    const int64_t cpt = ((int64_t)1 << t.b) / tpb;  // tpb is a power of two dividing 2^b
    t.skip = tt >= tpb;
    t.n0 = tt * cpt;
    t.n1 = t.n0 + cpt;
    t.live = beam_live(t.b, a.step, a.beam);
    t.keep = beam_keep(t.b, a.step, a.beam);
    t.sp = block_span(a.block_off, a.ud, t.g);
  } else {
    static_cast<Tile&>(t) = tile_of(a, tile);
    t.b = a.n_bits;
    t.live = a.live;
    t.keep = a.keep;
    t.skip = false;
  }
  return t;
}

// A lane per candidate row, blocks of at most CWQ_FUSED_DMAX dims.  The lane
// draws its row once into its LDS column; every beam is then one pass over the
// column in eval_row_f's order.
__global__ void __launch_bounds__(kLaneThreads) k_beam_score_lane(const ScoreArgs a) {
  __shared__ double logtab[32];
  __shared__ float srow[CWQ_FUSED_DMAX][kLaneThreads];
  __shared__ unsigned long long top[kMaxBeam];
  fill_logtab(logtab);
  const int tid = (int)threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const Tile t = tile_of(a, tile);
    if (tid < kMaxBeam) top[tid] = 0ull;
    __syncthreads();
    const int64_t d = t.sp.d;
    if (d <= CWQ_FUSED_DMAX) {  // the launcher's rule; longer rows would not fit srow
      const PhiloxStream st = generate_key(step_seed(a.sd.of(t.g), a.step), 42);
      const float* __restrict__ ls = a.loc_s + t.sp.off;
      const float* __restrict__ ss = a.scale_s + t.sp.off;
      const float* __restrict__ mu = a.t_loc + t.sp.off;
      const float* __restrict__ sg = a.t_scale + t.sp.off;
      const float* __restrict__ cn = a.lognorm + t.sp.off;
      const int64_t vec = d & ~(int64_t)7;
      for (int64_t n = t.n0 + tid; n < t.n1; n += kLaneThreads) {
        if (d > 0) {
          const uint64_t kbase = (uint64_t)n * (uint64_t)d;
          const uint64_t blk1 = (kbase + (uint64_t)d - 1) >> 2;
          for (uint64_t blk = kbase >> 2; blk <= blk1; ++blk) {
            const F4 z = normal4_dev(st, blk, logtab);
            const int64_t e0 = (int64_t)(blk << 2) - (int64_t)kbase;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const int64_t e = e0 + w;
              if (e >= 0 && e < d) {
                const float sc = ss[e];
                srow[e][tid] = shard_sample(ls[e], sc, f4_word(z, (uint32_t)w));
              }
            }
          }
        }
        for (int k = 0; k < a.live; ++k) {
          const float* __restrict__ bk = a.beams + (int64_t)k * a.bstride + t.sp.off;
          auto term = [&](int64_t e) -> float {
            const float b = a.step == 0 ? 0.0f : bk[e];
            return log_prob(b + srow[e][tid], mu[e], sg[e], cn[e]);  // :57, :59
          };
          float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int64_t j = 0; j < vec; j += 8) {
#pragma unroll
            for (int l = 0; l < 8; ++l) p[l] = p[l] + term(j + l);
          }
          float tl = 0.0f;
          for (int64_t j = vec; j < d; ++j) tl = tl + term(j);
          const float v = eigen_fold8(p, tl);
          const uint32_t c = (uint32_t)(((int64_t)k << a.n_bits) + n);
          top_insert(top, a.keep, argmax_key(v, c));
        }
      }
    }
    __syncthreads();
    if (tid < a.keep) a.tiles[tile * a.beam + tid] = top[tid];
    __syncthreads();
  }
}

// The same kernel under per-block bit budgets.  It is a kernel of its own and
// not an instance of one template with k_beam_score_lane (as the other four
// pairs are): the fixed kernel built from a shared body allocated its scalar
// registers otherwise (it spills them to lanes) and ran 2-4% slower on 65,536
// blocks of 32 dims, so its text stays as it was.
__global__ void __launch_bounds__(kLaneThreads) k_beam_score_lane_var(const ScoreArgs a,
                                                                      const VarTab v) {
  const VarTab* vt = &v;
  __shared__ double logtab[32];
  __shared__ float srow[CWQ_FUSED_DMAX][kLaneThreads];
  __shared__ unsigned long long top[kMaxBeam];
  fill_logtab(logtab);
  const int tid = (int)threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const BlockTile t = block_tile_of<true>(a, vt, tile);
    // The skip test depends only on the slot and the block's bit count, which
    // every thread of the workgroup reads alike: the whole workgroup skips, and
    // every __syncthreads() below stays workgroup-uniform.
    if (t.skip) continue;
    if (tid < kMaxBeam) top[tid] = 0ull;
    __syncthreads();
    const int64_t d = t.sp.d;
    if (d <= CWQ_FUSED_DMAX) {  // the launcher's rule; longer rows would not fit srow
      const PhiloxStream st = generate_key(step_seed(a.sd.of(t.g), a.step), 42);
      const float* __restrict__ ls = a.loc_s + t.sp.off;
      const float* __restrict__ ss = a.scale_s + t.sp.off;
      const float* __restrict__ mu = a.t_loc + t.sp.off;
      const float* __restrict__ sg = a.t_scale + t.sp.off;
      const float* __restrict__ cn = a.lognorm + t.sp.off;
      const int64_t vec = d & ~(int64_t)7;
      for (int64_t n = t.n0 + tid; n < t.n1; n += kLaneThreads) {
        if (d > 0) {
          const uint64_t kbase = (uint64_t)n * (uint64_t)d;
          const uint64_t blk1 = (kbase + (uint64_t)d - 1) >> 2;
          for (uint64_t blk = kbase >> 2; blk <= blk1; ++blk) {
            const F4 z = normal4_dev(st, blk, logtab);
            const int64_t e0 = (int64_t)(blk << 2) - (int64_t)kbase;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const int64_t e = e0 + w;
              if (e >= 0 && e < d) {
                const float sc = ss[e];
                srow[e][tid] = shard_sample(ls[e], sc, f4_word(z, (uint32_t)w));
              }
            }
          }
        }
        for (int k = 0; k < t.live; ++k) {
          const float* __restrict__ bk = a.beams + (int64_t)k * a.bstride + t.sp.off;
          auto term = [&](int64_t e) -> float {
            const float b = a.step == 0 ? 0.0f : bk[e];
            return log_prob(b + srow[e][tid], mu[e], sg[e], cn[e]);  // :57, :59
          };
          float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          for (int64_t j = 0; j < vec; j += 8) {
#pragma unroll
            for (int l = 0; l < 8; ++l) p[l] = p[l] + term(j + l);
          }
          float tl = 0.0f;
          for (int64_t j = vec; j < d; ++j) tl = tl + term(j);
          const float v = eigen_fold8(p, tl);
          const uint32_t c = (uint32_t)(((int64_t)k << t.b) + n);
          top_insert(top, t.keep, argmax_key(v, c));
        }
      }
    }
    __syncthreads();
    if (tid < t.keep) a.tiles[tile * a.beam + tid] = top[tid];
    __syncthreads();
  }
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// A wave per candidate row, any block length.  Per 248-dim chunk the wave
// stages the row's shard values once (a lane per Philox block, as
// exact_row_wave); the beams then take the chunk four at a time: all lanes
// write the four beams' terms, and the 16-lane row q of the wave folds beam
// 4 i + q -- lanes 0-7 of the row the eight Eigen accumulators, lane 8 the
// tail, in exact_row_wave's order.
template <bool VAR>
__device__ __forceinline__ void score_wave(const ScoreArgs& a, const VarTab* vt) {
  __shared__ double logtab[32];
  __shared__ float sbuf[4][kRowChunk];
  __shared__ float tbuf[4][4][kRowChunk];
  __shared__ unsigned long long top[kMaxBeam];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t row = lane >> 4, rl = lane & 15u;
  for (int64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const BlockTile t = block_tile_of<VAR>(a, vt, tile);
    if (VAR && t.skip) continue;  // the whole workgroup: see k_beam_score_lane_var
    const int live = t.live;
    if (threadIdx.x < kMaxBeam) top[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t d = t.sp.d;
    const int64_t vec = d & ~(int64_t)7;
    const PhiloxStream st = generate_key(step_seed(a.sd.of(t.g), a.step), 42);
    const float* __restrict__ ls = a.loc_s + t.sp.off;
    const float* __restrict__ ss = a.scale_s + t.sp.off;
    const float* __restrict__ mu = a.t_loc + t.sp.off;
    const float* __restrict__ sg = a.t_scale + t.sp.off;
    const float* __restrict__ cn = a.lognorm + t.sp.off;
    // wave-uniform loop: a wave takes a row as a whole
    for (int64_t n = t.n0 + wv; n < t.n1; n += 4) {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};  // beams 4 i + row: p[rl] (rl < 8), the tail (rl == 8)
      const uint64_t kbase = (uint64_t)n * (uint64_t)d;
      for (int64_t j0 = 0; j0 < d; j0 += kRowChunk) {
        const int64_t cnt = (d - j0) < kRowChunk ? d - j0 : kRowChunk;
        const uint64_t k0 = kbase + (uint64_t)j0;
        const uint64_t blk = (k0 >> 2) + lane;
        const int64_t ef = (int64_t)(blk << 2) - (int64_t)k0;  // chunk index of the block's word 0
        if (ef < cnt) {
          const F4 z = normal4_dev(st, blk, logtab);
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int64_t e = ef + w;
            if (e >= 0 && e < cnt) {
              const float sc = ss[j0 + e];
              sbuf[wv][e] = shard_sample(ls[j0 + e], sc, f4_word(z, (uint32_t)w));
            }
          }
        }
        wave_sync_lds();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (4 * i >= live) continue;  // wave-uniform
          for (int q = 0; q < 4 && 4 * i + q < live; ++q) {
            const float* __restrict__ bk = a.beams + (int64_t)(4 * i + q) * a.bstride + t.sp.off;
            for (int64_t e = lane; e < cnt; e += 64) {
              const int64_t j = j0 + e;
              const float b = a.step == 0 ? 0.0f : bk[j];
              tbuf[wv][q][e] = log_prob(b + sbuf[wv][e], mu[j], sg[j], cn[j]);  // :57, :59
            }
          }
          wave_sync_lds();
          if (4 * i + (int)row < live) {
            if (rl < 8) {
              for (int64_t e = rl; e < cnt && j0 + e < vec; e += 8) acc[i] = acc[i] + tbuf[wv][row][e];
            } else if (rl == 8) {
              for (int64_t e = (vec > j0 ? vec - j0 : 0); e < cnt; ++e)
                acc[i] = acc[i] + tbuf[wv][row][e];
            }
          }
          wave_sync_lds();
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (4 * i >= live) continue;
        float p[8];
#pragma unroll
        for (int l = 0; l < 8; ++l) p[l] = __shfl(acc[i], (int)(lane & 48u) + l, 64);
        const float v = eigen_fold8(p, __shfl(acc[i], (int)(lane & 48u) + 8, 64));
        const int k = 4 * i + (int)row;
        if (rl == 0 && k < live) {
          const uint32_t c = (uint32_t)(((int64_t)k << t.b) + n);
          top_insert(top, t.keep, argmax_key(v, c));
        }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < t.keep) a.tiles[tile * a.beam + threadIdx.x] = top[threadIdx.x];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) k_beam_score_wave(const ScoreArgs a) {
  score_wave<false>(a, nullptr);
}
__global__ void __launch_bounds__(256) k_beam_score_wave_var(const ScoreArgs a, const VarTab v) {
  score_wave<true>(a, &v);
}

// The keep largest keys of block g's tile lists, in decreasing order: pass j
// takes the largest key below pass j - 1's.  VAR: the block's own keep count
// and its own tpb[b_g] tiles of the `tiles_per_block` (= stride) slots it has.
template <bool VAR>
__device__ __forceinline__ void select_keys(
    const unsigned long long* __restrict__ tiles, int64_t nb, int64_t tiles_per_block, int beam,
    int keep, int n_steps, int32_t step, unsigned long long* __restrict__ sel,
    const VarTab* vt) {
  const uint32_t lane = threadIdx.x;
  int64_t cnt = tiles_per_block * keep;
  for (int64_t g = blockIdx.x; g < nb; g += gridDim.x) {
    if constexpr (VAR) {
      const int b = beam_clamp_bits(vt->n_bits[g], vt->max_bits);
      keep = beam_keep(b, step, beam);
      cnt = (int64_t)vt->tpb[b] * keep;
    }
    const unsigned long long* __restrict__ tl = tiles + g * tiles_per_block * beam;
    uint64_t prev = ~0ull;
    for (int j = 0; j < keep; ++j) {
      uint64_t m = 0;
      for (int64_t i = lane; i < cnt; i += 64) {
        const int64_t tt = i / keep;
        const uint64_t v = tl[tt * beam + (i - tt * keep)];
        if (v < prev && v > m) m = v;
      }
      m = wave_max_u64(m);
      if (lane == 0) sel[(g * n_steps + step) * beam + j] = m;
      prev = m;
    }
  }
}
__global__ void __launch_bounds__(64) k_beam_select(
    const unsigned long long* __restrict__ tiles, int64_t nb, int64_t tiles_per_block, int beam,
    int keep, int n_steps, int32_t step, unsigned long long* __restrict__ sel) {
  select_keys<false>(tiles, nb, tiles_per_block, beam, keep, n_steps, step, sel, nullptr);
}
__global__ void __launch_bounds__(64) k_beam_select_var(
    const unsigned long long* __restrict__ tiles, int64_t nb, int beam, int n_steps, int32_t step,
    unsigned long long* __restrict__ sel, const VarTab v) {
  select_keys<true>(tiles, nb, v.stride, beam, 0, n_steps, step, sel, &v);
}

__device__ __forceinline__ int64_t block_of_dim(const int64_t* __restrict__ off, int64_t nb,
                                                int64_t i) {
  int64_t lo = 0, hi = nb;  // off[lo] <= i < off[hi]; empty blocks are skipped
  while (hi - lo > 1) {
    const int64_t m = (lo + hi) >> 1;
    if (off[m] <= i) lo = m; else hi = m;
  }
  return lo;
}

// New beam j of every block: its parent's sum plus its row (the float32 add of
// :57), a thread per (beam, dim).  VAR: `keep` is the host's bound over all
// blocks, min(beam, 2^(max_bits (step + 1))); a thread whose j is not below its
// block's own L' returns.  Slots [L'_g, beam) of a block are never read later,
// because L_g of the next step is L'_g.
template <bool VAR>
__device__ __forceinline__ void advance_beams(
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, int64_t total_dims,
    const SeedSpec& sd, int32_t step, int n_steps, int n_bits, int beam, int keep,
    const unsigned long long* __restrict__ sel, const float* __restrict__ cur,
    float* __restrict__ nxt, int64_t bstride, const VarTab* vt) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  const int64_t nt = total_dims * keep;
  uint32_t rmask = (uint32_t)(((int64_t)1 << n_bits) - 1);
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nt;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = t / total_dims;
    const int64_t i = t - j * total_dims;
    const int64_t g = block_off ? block_of_dim(block_off, nb, i) : i / ud;
    if constexpr (VAR) {
      n_bits = beam_clamp_bits(vt->n_bits[g], vt->max_bits);
      if (j >= beam_keep(n_bits, step, beam)) continue;
      rmask = (uint32_t)(((int64_t)1 << n_bits) - 1);
    }
    const int64_t off = block_off ? block_off[g] : g * ud;
    const int64_t d = block_off ? block_off[g + 1] - off : ud;
    const uint64_t key = sel[(g * n_steps + step) * beam + j];
    const uint32_t c = key ? argmax_key_index(key) : 0u;  // (a key is never 0)
    const uint32_t r = c & rmask;
    const uint32_t par = (c >> n_bits) < (uint32_t)beam ? c >> n_bits : 0u;  // always: c < L 2^b
    const PhiloxStream st = generate_key(step_seed(sd.of(g), step), 42);
    const uint64_t k = (uint64_t)r * (uint64_t)d + (uint64_t)(i - off);
    const float zz = f4_word(normal4_dev(st, k >> 2, logtab), (uint32_t)(k & 3u));
    const float sc = scale_s[i];
    const float sv = shard_sample(loc_s[i], sc, zz);
    const float b = step == 0 ? 0.0f : cur[(int64_t)par * bstride + i];
    nxt[j * bstride + i] = b + sv;
  }
}
__global__ void __launch_bounds__(256) k_beam_advance(
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, int64_t total_dims,
    SeedSpec sd, int32_t step, int n_steps, int n_bits, int beam, int keep,
    const unsigned long long* __restrict__ sel, const float* __restrict__ cur,
    float* __restrict__ nxt, int64_t bstride) {
  advance_beams<false>(loc_s, scale_s, block_off, ud, nb, total_dims, sd, step, n_steps, n_bits,
                       beam, keep, sel, cur, nxt, bstride, nullptr);
}
__global__ void __launch_bounds__(256) k_beam_advance_var(
    const float* __restrict__ loc_s, const float* __restrict__ scale_s,
    const int64_t* __restrict__ block_off, int64_t ud, int64_t nb, int64_t total_dims,
    SeedSpec sd, int32_t step, int n_steps, int beam, int keep,
    const unsigned long long* __restrict__ sel, const float* __restrict__ cur,
    float* __restrict__ nxt, int64_t bstride, const VarTab v) {
  advance_beams<true>(loc_s, scale_s, block_off, ud, nb, total_dims, sd, step, n_steps, 0, beam,
                      keep, sel, cur, nxt, bstride, &v);
}

// Beam 0 of the last step: its row indices (walking the parents back), its sum
// and the value its key holds.  VAR: the block's own mask and shift.
template <bool VAR>
__device__ __forceinline__ void final_paths(
    const unsigned long long* __restrict__ sel, int64_t nb, int64_t total_dims, int n_steps,
    int n_bits, int beam, const float* __restrict__ fin, int32_t* __restrict__ out_idx,
    float* __restrict__ out_sample, float* __restrict__ out_value, const VarTab* vt) {
  uint32_t rmask = (uint32_t)(((int64_t)1 << n_bits) - 1);
  const int64_t nt = nb > total_dims ? nb : total_dims;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < nt;
       t += (int64_t)gridDim.x * blockDim.x) {
    if (t < total_dims) out_sample[t] = fin[t];
    if (t >= nb) continue;
    if constexpr (VAR) {
      n_bits = beam_clamp_bits(vt->n_bits[t], vt->max_bits);
      rmask = (uint32_t)(((int64_t)1 << n_bits) - 1);
    }
    uint32_t j = 0;
    for (int s = n_steps - 1; s >= 0; --s) {
      const uint64_t key = sel[(t * n_steps + s) * beam + j];
      if (s == n_steps - 1 && out_value) out_value[t] = unord_f32((uint32_t)(key >> 32));
      const uint32_t c = key ? argmax_key_index(key) : 0u;
      out_idx[t * n_steps + s] = (int32_t)(c & rmask);
      j = (c >> n_bits) < (uint32_t)beam ? c >> n_bits : 0u;  // always: c < L 2^b
    }
  }
}
__global__ void __launch_bounds__(256) k_beam_final(
    const unsigned long long* __restrict__ sel, int64_t nb, int64_t total_dims, int n_steps,
    int n_bits, int beam, const float* __restrict__ fin, int32_t* __restrict__ out_idx,
    float* __restrict__ out_sample, float* __restrict__ out_value) {
  final_paths<false>(sel, nb, total_dims, n_steps, n_bits, beam, fin, out_idx, out_sample,
                     out_value, nullptr);
}
__global__ void __launch_bounds__(256) k_beam_final_var(
    const unsigned long long* __restrict__ sel, int64_t nb, int64_t total_dims, int n_steps,
    int beam, const float* __restrict__ fin, int32_t* __restrict__ out_idx,
    float* __restrict__ out_sample, float* __restrict__ out_value, const VarTab v) {
  final_paths<true>(sel, nb, total_dims, n_steps, 0, beam, fin, out_idx, out_sample, out_value,
                    &v);
}

}  // namespace

hipError_t launch_beam_encode(const BeamArgs& a, hipStream_t stream) {
  if (a.nb <= 0) return hipSuccess;
  hipError_t e;
  const BeamWs l = beam_ws(a.nb, a.total_dims, a.n_steps, a.beam);
  float* loc_s = at<float>(a.workspace, l.loc_s);
  float* scale_s = at<float>(a.workspace, l.scale_s);
  float* lognorm = at<float>(a.workspace, l.lognorm);
  float* beams = at<float>(a.workspace, l.beams);
  unsigned long long* tiles = at<unsigned long long>(a.workspace, l.tiles);
  unsigned long long* sel = at<unsigned long long>(a.workspace, l.sel);
  const int64_t D = a.total_dims;
  const int64_t half = (int64_t)a.beam * D;
  const float nst = (float)a.n_steps;
  const float sdiv = (float)__builtin_sqrt((double)a.n_steps);
  const SeedSpec sd{a.seed, a.block_id_base, nullptr};
  // Per-block budgets: a.n_bits is the caller's bound max_bits, every host-side
  // count below is the bound over all blocks, and the kernels take each block's
  // own from n_bits_dev.
  const bool var = a.n_bits_dev != nullptr;
  const int64_t n_cand = (int64_t)1 << a.n_bits;
  if (D > 0) {
    hipLaunchKernelGGL(k_beam_prep, dim3(grid_for(D, 256, 1u << 16)), dim3(256), 0, stream,
                       a.t_scale, a.p_loc, a.p_scale, D, nst, sdiv, a.rho, loc_s, scale_s, lognorm);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  VarTab vt{};
  if (var) {
    vt.n_bits = a.n_bits_dev;
    vt.max_bits = a.n_bits;
    for (int b = 0; b <= a.n_bits && b < kBeamVarTabLen; ++b)
      vt.tpb[b] = (int32_t)beam_tiles_per_block(a.path, a.nb, (int64_t)1 << b, a.quarter_tiles);
    vt.stride = vt.tpb[a.n_bits];  // the rule is monotone in 2^b: <= beam_tiles_cap(nb)
  }
  ScoreArgs s;
  s.t_loc = a.t_loc;
  s.t_scale = a.t_scale;
  s.loc_s = loc_s;
  s.scale_s = scale_s;
  s.lognorm = lognorm;
  s.bstride = D;
  s.block_off = a.block_off;
  s.ud = a.ud;
  s.tiles_per_block = beam_tiles_per_block(a.path, a.nb, n_cand, a.quarter_tiles);
  s.cand_per_tile = n_cand / s.tiles_per_block;
  s.ntiles = a.nb * s.tiles_per_block;  // var: nb * stride tile slots
  s.n_bits = a.n_bits;
  s.sd = sd;
  s.beam = a.beam;
  s.tiles = tiles;
  const unsigned sgrid = grid_for(s.ntiles, 1, kBeamGridCap);
  int live = 1;
  int cur = 0;
  for (int step = 0; step < a.n_steps; ++step) {
    const int64_t cands = (int64_t)live * n_cand;
    const int keep = cands < a.beam ? (int)cands : a.beam;
    s.beams = beams + cur * half;
    s.step = step;
    s.live = live;
    s.keep = keep;
    if (step == 0 && a.ev_start &&
        (e = hipEventRecord((hipEvent_t)a.ev_start, stream)) != hipSuccess)
      return e;
    if (var) {
      if (a.path == BeamPath::LanePerRow)
        hipLaunchKernelGGL(k_beam_score_lane_var, dim3(sgrid), dim3(kLaneThreads), 0, stream, s,
                           vt);
      else
        hipLaunchKernelGGL(k_beam_score_wave_var, dim3(sgrid), dim3(256), 0, stream, s, vt);
    } else if (a.path == BeamPath::LanePerRow) {
      hipLaunchKernelGGL(k_beam_score_lane, dim3(sgrid), dim3(kLaneThreads), 0, stream, s);
    } else {
      hipLaunchKernelGGL(k_beam_score_wave, dim3(sgrid), dim3(256), 0, stream, s);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (step == a.n_steps - 1 && a.ev_stop &&
        (e = hipEventRecord((hipEvent_t)a.ev_stop, stream)) != hipSuccess)
      return e;
    if (var)
      hipLaunchKernelGGL(k_beam_select_var, dim3(grid_for(a.nb, 1, 1u << 20)), dim3(64), 0, stream,
                         tiles, a.nb, a.beam, a.n_steps, step, sel, vt);
    else
      hipLaunchKernelGGL(k_beam_select, dim3(grid_for(a.nb, 1, 1u << 20)), dim3(64), 0, stream,
                         tiles, a.nb, s.tiles_per_block, a.beam, keep, a.n_steps, step, sel);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (D > 0) {
      // var: keep = min(beam, 2^(max_bits (step + 1))), no block keeps more
      if (var)
        hipLaunchKernelGGL(k_beam_advance_var, dim3(grid_for(D * keep, 256, 1u << 16)), dim3(256),
                           0, stream, loc_s, scale_s, a.block_off, a.ud, a.nb, D, sd, step,
                           a.n_steps, a.beam, keep, sel, beams + cur * half,
                           beams + (1 - cur) * half, D, vt);
      else
        hipLaunchKernelGGL(k_beam_advance, dim3(grid_for(D * keep, 256, 1u << 16)), dim3(256), 0,
                           stream, loc_s, scale_s, a.block_off, a.ud, a.nb, D, sd, step, a.n_steps,
                           a.n_bits, a.beam, keep, sel, beams + cur * half,
                           beams + (1 - cur) * half, D);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    cur = 1 - cur;
    live = keep;
  }
  const int64_t nt = a.nb > D ? a.nb : D;
  if (var)
    hipLaunchKernelGGL(k_beam_final_var, dim3(grid_for(nt, 256, 1u << 16)), dim3(256), 0, stream,
                       sel, a.nb, D, a.n_steps, a.beam, beams + cur * half, a.out_idx,
                       a.out_sample, a.out_value, vt);
  else
    hipLaunchKernelGGL(k_beam_final, dim3(grid_for(nt, 256, 1u << 16)), dim3(256), 0, stream, sel,
                       a.nb, D, a.n_steps, a.n_bits, a.beam, beams + cur * half, a.out_idx,
                       a.out_sample, a.out_value);
  return hipGetLastError();
}

}  // namespace cwq
