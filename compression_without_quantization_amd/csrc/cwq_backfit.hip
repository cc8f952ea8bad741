// cwq_backfit.hip -- backfitting for the greedy coder.
//
// Coordinate ascent over the steps of a finished code: for step s the other
// steps' rows stay, every row of step s's stream is scored against their sum,
// and the best one replaces the step's row if the decoded sample's value gets
// larger.  A code is still one row index per step, so the decoders and the bit
// string are unchanged, and no block ever ends below the code it started from.
//
// The selected row of every step lives in rows[n_steps][total_dims]; a block's
// value v in value[g].  One step of a sweep is
//   * k_backfit_base: best[j] = the decoder-order sum of the cached rows with
//     step s skipped, into the vector the scoring kernels carry; keys = 0;
//   * the encoder's scoring launches of step s in their step > 0 form
//     (launch_score_step): keys[g] = the best row's key;
//   * k_backfit_accept: r* from the key; if it differs from the step's index,
//     the row is drawn, the decoder-order sum with it is valued in the Eigen
//     order and compared with v; on accept the index, the cached row, v and
//     the count are stored.  One wave (or one lane) handles a block alone.
// k_backfit_init fills the cache and v before the first sweep, k_backfit_final
// writes the sample and the value after the last.
//
// Under per-block bit budgets (cwq_greedy_backfit_var) the blocks
// arrive sorted by budget and only the scoring differs: one launch sequence per
// budget bucket on that bucket's slice of the shared arrays (BudgetBucket),
// between the same k_backfit_base and accept launch over all blocks.  None of
// the kernels here reads a bit count: they read indices and keys.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "cwq_device.h"
#include "cwq_kernels.h"

namespace cwq {
namespace {

constexpr int kRowChunk = 248;  // exact_row_wave's chunk: a multiple of 8, at most 63 Philox blocks
constexpr int kChunkPerLane = (kRowChunk + 63) / 64;

struct BfArgs {
  const float* t_loc;
  const float* t_scale;
  const float* loc_s;
  const float* scale_s;
  const float* lognorm;
  const int64_t* block_off;
  int64_t ud, nb, total_dims;
  int n_steps;
  SeedSpec sd;
  float* rows;                       // [n_steps][total_dims]
  float* value;                      // [nb]
  int32_t* count;                    // [nb]
  int32_t* idx;                      // [nb][n_steps]
  const unsigned long long* keys;    // [nb]
};

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The value a key holds for v: NaN and values <= -FLT_MAX read as -FLT_MAX, -0 as +0.
__device__ __forceinline__ float keyed_value(float v) {
  return unord_f32((uint32_t)(argmax_key(v, 0u) >> 32));
}

// Dims [j0, j0 + cnt) of row r of the stream st, a lane per Philox block, into buf.
__device__ __forceinline__ void stage_row_chunk(const PhiloxStream& st, uint64_t kbase, int64_t j0,
                                                int64_t cnt, const float* __restrict__ ls,
                                                const float* __restrict__ ss,
                                                const double* logtab, float* buf, uint32_t lane) {
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
        buf[e] = shard_sample(ls[j0 + e], sc, f4_word(z, (uint32_t)w));
      }
    }
  }
}

// The value of block (sp, g) by a whole wave: the decoder-order sum of the
// steps' rows, the log-density terms, and their fold in exact_row_wave's order
// (lanes 0-7 the eight strided accumulators, lane 8 the tail).  ALL: every
// step's row is drawn from a.idx and also stored to the cache (k_backfit_init).
// Otherwise the cache is read, except step s_new, whose row r_new is drawn.
// Every lane returns the (unkeyed) value.  Full exec mask.
template <bool ALL>
__device__ __forceinline__ float wave_block_value(const BfArgs& a, int64_t g, const BlockSpan sp,
                                                  int s_new, uint32_t r_new, const double* logtab,
                                                  float* sbuf, float* tbuf, uint32_t lane) {
  const int64_t d = sp.d;
  const int64_t vec = d & ~(int64_t)7;
  const float* __restrict__ ls = a.loc_s + sp.off;
  const float* __restrict__ ss = a.scale_s + sp.off;
  const int32_t bseed = a.sd.of(g);
  float acc = 0.0f;  // lane l < 8: p[l]; lane 8: the tail sum
  for (int64_t j0 = 0; j0 < d; j0 += kRowChunk) {
    const int64_t cnt = (d - j0) < kRowChunk ? d - j0 : kRowChunk;
    float x[kChunkPerLane];
#pragma unroll
    for (int i = 0; i < kChunkPerLane; ++i) x[i] = 0.0f;  // the decoder's +0
    for (int t = 0; t < a.n_steps; ++t) {
      const bool draw = ALL || t == s_new;  // wave-uniform
      if (draw) {
        const uint32_t r = ALL ? (uint32_t)a.idx[g * a.n_steps + t] : r_new;
        const PhiloxStream st = generate_key(step_seed(bseed, t), 42);
        stage_row_chunk(st, (uint64_t)r * (uint64_t)d, j0, cnt, ls, ss, logtab, sbuf, lane);
        wave_sync_lds();
      }
      float* __restrict__ rt = a.rows + (int64_t)t * a.total_dims + sp.off + j0;
#pragma unroll
      for (int i = 0; i < kChunkPerLane; ++i) {
        const int64_t e = (int64_t)lane + 64 * i;
        if (e < cnt) {
          const float rv = draw ? sbuf[e] : rt[e];
          if (ALL) rt[e] = rv;
          x[i] = x[i] + rv;
        }
      }
      if (draw) wave_sync_lds();
    }
#pragma unroll
    for (int i = 0; i < kChunkPerLane; ++i) {
      const int64_t e = (int64_t)lane + 64 * i;
      if (e < cnt) {
        const int64_t j = sp.off + j0 + e;
        tbuf[e] = log_prob(x[i], a.t_loc[j], a.t_scale[j], a.lognorm[j]);
      }
    }
    wave_sync_lds();
    if (lane < 8) {
      for (int64_t e = lane; e < cnt && j0 + e < vec; e += 8) acc = acc + tbuf[e];
    } else if (lane == 8) {
      for (int64_t e = (vec > j0 ? vec - j0 : 0); e < cnt; ++e) acc = acc + tbuf[e];
    }
    wave_sync_lds();
  }
  float p[8];
#pragma unroll
  for (int l = 0; l < 8; ++l) p[l] = __shfl(acc, l, 64);
  return eigen_fold8(p, __shfl(acc, 8, 64));
}

// The cache of every step's selected row and v, a wave per block.
__global__ void __launch_bounds__(256) k_backfit_init(const BfArgs a) {
  __shared__ double logtab[32];
  __shared__ float sbuf[4][kRowChunk];
  __shared__ float tbuf[4][kRowChunk];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;
  // wave-uniform loop: a wave takes a block as a whole
  for (int64_t g = 4 * (int64_t)blockIdx.x + wv; g < a.nb; g += 4 * (int64_t)gridDim.x) {
    const BlockSpan sp = block_span(a.block_off, a.ud, g);
    const float v = wave_block_value<true>(a, g, sp, -1, 0u, logtab, sbuf[wv], tbuf[wv], lane);
    if (lane == 0) {
      a.value[g] = keyed_value(v);
      a.count[g] = 0;
    }
  }
}

// best[i] = ((+0 + row(0)) + row(1)) + ... with step s skipped, a thread per
// dim; keys[g] = 0 for the scoring launches.
__global__ void __launch_bounds__(256) k_backfit_base(const float* __restrict__ rows,
                                                      int64_t total_dims, int64_t nb, int n_steps,
                                                      int s, float* __restrict__ best,
                                                      unsigned long long* __restrict__ keys) {
  const int64_t nt = total_dims > nb ? total_dims : nb;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nt;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nb) keys[i] = 0ull;
    if (i >= total_dims) continue;
    float x = 0.0f;
    for (int t = 0; t < n_steps; ++t)
      if (t != s) x = x + rows[(int64_t)t * total_dims + i];
    best[i] = x;
  }
}

// Step s's accept test, a wave per block.
__global__ void __launch_bounds__(256) k_backfit_accept_wave(const BfArgs a, int s) {
  __shared__ double logtab[32];
  __shared__ float sbuf[4][kRowChunk];
  __shared__ float tbuf[4][kRowChunk];
  fill_logtab(logtab);
  const uint32_t wv = wave_id();
  const uint32_t lane = threadIdx.x & 63u;
  for (int64_t g = 4 * (int64_t)blockIdx.x + wv; g < a.nb; g += 4 * (int64_t)gridDim.x) {
    const uint32_t r = key_index(a.keys[g]);
    if (r == (uint32_t)a.idx[g * a.n_steps + s]) continue;  // wave-uniform
    const BlockSpan sp = block_span(a.block_off, a.ud, g);
    const float v = keyed_value(
        wave_block_value<false>(a, g, sp, s, r, logtab, sbuf[wv], tbuf[wv], lane));
    if (!(v > a.value[g])) continue;  // wave-uniform: every lane holds the same v
    // accepted: the row is drawn once more, into the cache
    const PhiloxStream st = generate_key(step_seed(a.sd.of(g), s), 42);
    float* __restrict__ rs = a.rows + (int64_t)s * a.total_dims + sp.off;
    for (int64_t j0 = 0; j0 < sp.d; j0 += kRowChunk) {
      const int64_t cnt = (sp.d - j0) < kRowChunk ? sp.d - j0 : kRowChunk;
      stage_row_chunk(st, (uint64_t)r * (uint64_t)sp.d, j0, cnt, a.loc_s + sp.off,
                      a.scale_s + sp.off, logtab, sbuf[wv], lane);
      wave_sync_lds();
      for (int64_t e = lane; e < cnt; e += 64) rs[j0 + e] = sbuf[wv][e];
      wave_sync_lds();
    }
    if (lane == 0) {
      a.idx[g * a.n_steps + s] = (int32_t)r;
      a.value[g] = v;
      a.count[g] = a.count[g] + 1;
    }
  }
}

// Step s's accept test, a lane per block of at most CWQ_FUSED_DMAX dims: the
// lane walks the dims in eval_row_f's order.
__global__ void __launch_bounds__(256) k_backfit_accept_lane(const BfArgs a, int s) {
  __shared__ double logtab[32];
  fill_logtab(logtab);
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < a.nb;
       g += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = key_index(a.keys[g]);
    if (r == (uint32_t)a.idx[g * a.n_steps + s]) continue;
    const BlockSpan sp = block_span(a.block_off, a.ud, g);
    const int64_t d = sp.d;
    const int64_t vec = d & ~(int64_t)7;
    const uint64_t kbase = (uint64_t)r * (uint64_t)d;
    const PhiloxStream st = generate_key(step_seed(a.sd.of(g), s), 42);
    const float* __restrict__ ls = a.loc_s + sp.off;
    const float* __restrict__ ss = a.scale_s + sp.off;
    F4 z = {0.f, 0.f, 0.f, 0.f};
    auto drawn = [&](int64_t e) -> float {  // dim e of the row; e ascends
      const uint64_t k = kbase + (uint64_t)e;
      if ((k & 3u) == 0 || e == 0) z = normal4_dev(st, k >> 2, logtab);
      const float sc = ss[e];
      return shard_sample(ls[e], sc, f4_word(z, (uint32_t)(k & 3u)));
    };
    auto term = [&](int64_t e) -> float {
      const float nv = drawn(e);
      float x = 0.0f;
      for (int t = 0; t < a.n_steps; ++t)
        x = x + (t == s ? nv : a.rows[(int64_t)t * a.total_dims + sp.off + e]);
      const int64_t j = sp.off + e;
      return log_prob(x, a.t_loc[j], a.t_scale[j], a.lognorm[j]);
    };
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t j = 0; j < vec; j += 8) {
#pragma unroll
      for (int l = 0; l < 8; ++l) p[l] = p[l] + term(j + l);
    }
    float tl = 0.0f;
    for (int64_t j = vec; j < d; ++j) tl = tl + term(j);
    const float v = keyed_value(eigen_fold8(p, tl));
    if (!(v > a.value[g])) continue;
    float* __restrict__ rs = a.rows + (int64_t)s * a.total_dims + sp.off;
    for (int64_t e = 0; e < d; ++e) rs[e] = drawn(e);
    a.idx[g * a.n_steps + s] = (int32_t)r;
    a.value[g] = v;
    a.count[g] = a.count[g] + 1;
  }
}

// out_sample = the decoder-order sum of the cached rows; the value and count.
__global__ void __launch_bounds__(256) k_backfit_final(
    const float* __restrict__ rows, const float* __restrict__ value,
    const int32_t* __restrict__ count, int64_t total_dims, int64_t nb, int n_steps,
    float* __restrict__ out_sample, float* __restrict__ out_value,
    int32_t* __restrict__ out_accepted) {
  const int64_t nt = total_dims > nb ? total_dims : nb;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nt;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (i < nb) {
      if (out_value) out_value[i] = value[i];
      if (out_accepted) out_accepted[i] = count[i];
    }
    if (i >= total_dims) continue;
    float x = 0.0f;
    for (int t = 0; t < n_steps; ++t) x = x + rows[(int64_t)t * total_dims + i];
    out_sample[i] = x;
  }
}

}  // namespace

hipError_t launch_backfit(const BackfitArgs& b, hipStream_t stream) {
  const EncodeArgs& e = b.enc;
  if (e.nb <= 0) return hipSuccess;
  hipError_t err;
  const int64_t D = e.total_dims;
  // the shard constants and normalisers (also: out_sample = 0, keys = 0)
  err = launch_prep_dims(e.t_scale, e.p_loc, e.p_scale, D, e.n_steps, e.rho, e.loc_s, e.scale_s,
                         e.lognorm, e.out_sample, e.keys, e.nb, stream);
  if (err != hipSuccess) return err;
  BfArgs a;
  a.t_loc = e.t_loc;
  a.t_scale = e.t_scale;
  a.loc_s = e.loc_s;
  a.scale_s = e.scale_s;
  a.lognorm = e.lognorm;
  a.block_off = e.block_off;
  a.ud = e.ud;
  a.nb = e.nb;
  a.total_dims = D;
  a.n_steps = e.n_steps;
  a.sd = SeedSpec{e.seed, e.block_id_base, e.seeds};
  a.rows = b.rows;
  a.value = b.value;
  a.count = b.count;
  a.idx = e.out_idx;
  a.keys = e.keys;
  // step s's scoring launches: the call's own, or one sequence per budget
  // bucket on that bucket's slice of the shared arrays.  The
  // screening arrays are not shifted: the buckets use them in stream order and
  // each sequence initialises what it reads.
  auto score = [&](int s) -> hipError_t {
    if (!b.buckets) return launch_score_step(e, s, stream);
    for (int i = 0; i < b.n_buckets; ++i) {
      const BudgetBucket& k = b.buckets[i];
      EncodeArgs p = e;
      p.t_loc = e.t_loc + k.d0;
      p.t_scale = e.t_scale + k.d0;
      p.p_loc = e.p_loc + k.d0;
      p.p_scale = e.p_scale + k.d0;
      p.loc_s = e.loc_s + k.d0;
      p.scale_s = e.scale_s + k.d0;
      p.lognorm = e.lognorm + k.d0;
      p.out_sample = e.out_sample + k.d0;
      p.keys = e.keys + k.r0;
      p.out_idx = e.out_idx + k.r0 * e.n_steps;
      p.block_id_base = e.block_id_base + k.r0;
      if (e.seeds) p.seeds = e.seeds + k.r0;
      p.block_off = k.block_off;
      p.nb = k.count;
      p.total_dims = k.dims;
      p.max_d = k.maxd;
      p.n_cand = (int64_t)1 << k.bits;
      p.tiles_per_block = k.tiles_per_block;
      p.cand_per_tile = k.cand_per_tile;
      p.rows_wave = k.rows_wave;
      const hipError_t se = launch_score_step(p, s, stream);
      if (se != hipSuccess) return se;
    }
    return hipSuccess;
  };
  const unsigned wgrid = grid_for(e.nb, 4, 1u << 16);
  const unsigned dgrid = grid_for(D > e.nb ? D : e.nb, 256, 1u << 16);
  hipLaunchKernelGGL(k_backfit_init, dim3(wgrid), dim3(256), 0, stream, a);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  // a code of one step is returned as given (include/cwq.h: there is no other
  // step to fit it to)
  const int sweeps = e.n_steps > 1 ? b.sweeps : 0;
  for (int k = 0; k < sweeps; ++k) {
    for (int s = 0; s < e.n_steps; ++s) {
      hipLaunchKernelGGL(k_backfit_base, dim3(dgrid), dim3(256), 0, stream, b.rows, D, e.nb,
                         e.n_steps, s, e.out_sample, e.keys);
      if ((err = hipGetLastError()) != hipSuccess) return err;
      if (k == 0 && s == 0 && e.ev_start &&
          (err = hipEventRecord((hipEvent_t)e.ev_start, stream)) != hipSuccess)
        return err;
      if ((err = score(s)) != hipSuccess) return err;
      if (k == sweeps - 1 && s == e.n_steps - 1 && e.ev_stop &&
          (err = hipEventRecord((hipEvent_t)e.ev_stop, stream)) != hipSuccess)
        return err;
      if (b.path == BackfitPath::LanePerBlock)
        hipLaunchKernelGGL(k_backfit_accept_lane, dim3(grid_for(e.nb, 256, 1u << 16)), dim3(256),
                           0, stream, a, s);
      else
        hipLaunchKernelGGL(k_backfit_accept_wave, dim3(wgrid), dim3(256), 0, stream, a, s);
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
  }
  if (sweeps == 0 && e.ev_start) {  // no scoring launch: an empty bracket
    if ((err = hipEventRecord((hipEvent_t)e.ev_start, stream)) != hipSuccess) return err;
    if ((err = hipEventRecord((hipEvent_t)e.ev_stop, stream)) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_backfit_final, dim3(dgrid), dim3(256), 0, stream, b.rows, b.value, b.count,
                     D, e.nb, e.n_steps, e.out_sample, b.out_value, b.out_accepted);
  return hipGetLastError();
}

}  // namespace cwq
