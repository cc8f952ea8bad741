// cwq_device.h -- device helpers shared by the gfx950 kernels (greedy and
// importance coders): LDS log table, wave reductions, block spans, the
// device-tuned Philox / Box-Muller / division, and the Eigen-order row
// evaluator.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cwq_dispatch.h"
#include "cwq_math.h"
#include "cwq_philox_lo.h"
#include "cwq_screen.h"

namespace cwq {

static __constant__ double kLogTabConst[32] = CWQ_LOGF_TAB_INIT;

__device__ __forceinline__ void fill_logtab(double* lds) {
  if (threadIdx.x < 32) lds[threadIdx.x] = kLogTabConst[threadIdx.x];
  __syncthreads();
}

// A target dim's log-density normaliser c = 0.5 log(2 pi) + log(scale) (cwq_math.h A.5)
__device__ __forceinline__ float lognorm_of(float t_scale) {
  return kHalfLog2Pi + logf_full(t_scale, kLogTabConst);
}

// Per-dim KL(a || b) of two Gaussians, TFP <= 0.7 form in float32
// (coded_greedy_sampler.py:201): k_kl_normal_normal, the grouped coders' prep
// kernels and k_block_bits (cwq_varbits.hip) all take it from here.
__device__ __forceinline__ float kl_normal_normal_1(float a_loc, float a_scale, float b_loc,
                                                    float b_scale) {
  const float sa2 = a_scale * a_scale;
  const float sb2 = b_scale * b_scale;
  const float ratio = sa2 / sb2;
  const float dl = a_loc - b_loc;
  const float t1 = (dl * dl) / (2.0f * sb2);
  const float t2 = 0.5f * ((ratio - 1.0f) - logf_full(ratio, kLogTabConst));
  return t1 + t2;
}

__device__ __forceinline__ uint32_t wave_id() {
  return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}

__device__ __forceinline__ double wave_sum_f64(double v) {  // full exec mask
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {  // full exec mask
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    uint64_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// ---------------------------------------------------------------------------
// Device-tuned arithmetic.  Same results as the portable restatement in
// cwq_math.h (the Box-Muller pieces are verified exhaustively on the GPU by
// tests/test_gpu.py via cwq_selftest_bm_tables), fewer instructions:
//   * Philox: the two 3-input XORs of a round are one v_bitop3_b32 each.
//   * sqrt for the Box-Muller radius: the argument -2 logf(u1) lies in
//     [2.4e-7, 32.3] (normal, finite), so the correctly rounded sqrt is
//     v_sqrt_f32 plus the two one-ulp corrections, without the denormal
//     scaling and special-case fixups of the general sequence.
//   * angle: Uint32ToFloat(x1) = m * 2^-23 exactly, so
//     RN64(2pi * U) = RN64((2pi * 2^-23) * m) and m converts exactly.
// ---------------------------------------------------------------------------
__device__ __forceinline__ U4 philox10_dev(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
    const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return U4{c0, c1, c2, c3};
}

// Philox-10 of the counter (c0, 0, c2, c3) with c2, c3 and the key
// wave-uniform: cwq_philox_lo.h (PhiloxLo, philox10_lo, and philox10_lo_p0,
// which takes round 0's product).  The stream's four words stay scalars, so
// rounds 0-2 need one two-operand v_xor_b32 with a scalar each instead of a
// three-input v_bitop3_b32 with two scalars (the constant bus takes one: a
// v_mov per round) or a uniform value held in a VGPR.
// Same results as philox10_dev(c0, 0, c2, c3, k0, k1) (tests/test_gpu.py).
__device__ __forceinline__ PhiloxLo philox_lo_key(const PhiloxStream& s) {
  PhiloxLo o = philox_lo_words(s);
  // opaque scalars: the compiler must not re-associate the XORs into
  // three-input bitop3 forms with two scalar operands
  asm volatile("" : "+s"(o.A), "+s"(o.B), "+s"(o.C), "+s"(o.D));
  return o;
}

__device__ __forceinline__ U4 philox_block_dev(const PhiloxStream& s, uint64_t grp) {
  return philox10_dev((uint32_t)grp, (uint32_t)(grp >> 32), s.c2, s.c3, s.k0, s.k1);
}

__device__ __forceinline__ float sqrt_cr_bm(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float sd = u2f(f2u(s) - 1u);
  const float su = u2f(f2u(s) + 1u);
  const float rd = __builtin_fmaf(-sd, s, x);
  const float ru = __builtin_fmaf(-su, s, x);
  const float t = (rd <= 0.0f) ? sd : s;
  return (ru > 0.0f) ? su : t;
}

__device__ __forceinline__ float bm_radius_dev(uint32_t x0, const double* logtab) {
  float u1 = uint32_to_float(x0);
  u1 = fmaxf(u1, 1.0e-7f);  // == (u1 < 1e-7f ? 1e-7f : u1): u1 is never NaN
  return sqrt_cr_bm(-2.0f * logf_core(u1, logtab));
}

__device__ __forceinline__ float bm_angle_dev(uint32_t x1) {
  return (float)((double)(x1 & 0x7fffffu) * 0x1.921fb54442d18p-21);
}

__device__ __forceinline__ void box_muller_dev(uint32_t x0, uint32_t x1, const double* logtab,
                                               float& f0, float& f1) {
  const float u2 = bm_radius_dev(x0, logtab);
  float s, c;
  sincosf_pos(bm_angle_dev(x1), s, c);
  f0 = s * u2;
  f1 = c * u2;
}

// Screening Box-Muller (approximate).  The hardware transcendentals
// v_log_f32 / v_sqrt_f32 / v_sin_f32 / v_cos_f32 (sin and cos take the angle in
// revolutions, so U = Uint32ToFloat(x1) needs no scaling or range reduction).
// Used ONLY by the screening passes, which turn the values into rigorous
// bounds: the largest deviation from the exact pair over every possible input
// (2^23 each) is a measured constant, kScreenEr / kScreenEs, re-checked
// exhaustively on the GPU by tests/test_gpu.py.
//
// The radius is carried without its constant factor: q~ = sqrt(-log2 u1) =
// r~ / sqrt(2 ln 2), and box_muller_screen returns z~ / sqrt(2 ln 2); the
// per-dim constants fold kSqrt2Ln2 in (cwq_screen.h: one multiply less per pair).
__device__ __forceinline__ float bm_qradius_screen(uint32_t x0) {
  const float u1 = fmaxf(uint32_to_float(x0), 1.0e-7f);
  return __builtin_amdgcn_sqrtf(-__builtin_amdgcn_logf(u1));
}
__device__ __forceinline__ void bm_sincos_screen(uint32_t x1, float& s, float& c) {
  // 1 + U (exact, in [1, 2)): sin/cos in revolutions are 1-periodic, so the
  // "- 1.0f" of Uint32ToFloat is not needed here (the error table covers it)
  const float V = u2f((x1 & 0x7fffffu) | 0x3f800000u);
  s = __builtin_amdgcn_sinf(V);
  c = __builtin_amdgcn_cosf(V);
}
__device__ __forceinline__ void box_muller_screen(uint32_t x0, uint32_t x1, float& f0, float& f1) {
  const float q = bm_qradius_screen(x0);
  float s, c;
  bm_sincos_screen(x1, s, c);
  f0 = s * q;
  f1 = c * q;
}

__device__ __forceinline__ F4 normal4_screen(const PhiloxStream& s, uint64_t grp) {
  const U4 x = philox_block_dev(s, grp);
  F4 z;
  box_muller_screen(x.x, x.y, z.a, z.b);
  box_muller_screen(x.z, x.w, z.c, z.d);
  return z;
}

// normal4_screen of a block below 2^32, K = philox_lo_key(s)
__device__ __forceinline__ F4 normal4_screen_lo(const PhiloxStream& s, const PhiloxLo& K,
                                                uint32_t grp) {
  const U4 x = philox10_lo(grp, K, s.k0, s.k1);
  F4 z;
  box_muller_screen(x.x, x.y, z.a, z.b);
  box_muller_screen(x.z, x.w, z.c, z.d);
  return z;
}

__device__ __forceinline__ F4 normal4_dev(const PhiloxStream& s, uint64_t grp,
                                          const double* logtab) {
  const U4 x = philox_block_dev(s, grp);
  F4 z;
  box_muller_dev(x.x, x.y, logtab, z.a, z.b);
  box_muller_dev(x.z, x.w, logtab, z.c, z.d);
  return z;
}

// Correctly rounded a / b for 2^-60 <= |a| <= 2^60 (or a == 0) and
// 2^-60 <= b <= 2^60, given y = RN(1/b).  q0 = RN(a y) is within 2 ulps;
// one residual step brings q1 within 1 ulp; with q1 within 1 ulp and y within
// half an ulp of 1/b, the residual b*q1 - a is exact and the final fused step
// rounds to RN(a/b) (Markstein's theorem).  The ranges keep
// every intermediate normal.  Callers route other operands to IEEE division.
__device__ __forceinline__ float div_rn_markstein(float a, float b, float y) {
  const float q0 = a * y;
  const float r0 = __builtin_fmaf(-b, q0, a);
  const float q1 = __builtin_fmaf(r0, y, q0);
  const float r1 = __builtin_fmaf(-b, q1, a);
  return __builtin_fmaf(r1, y, q1);
}
// 2^-60 <= |a| < 2^60 (biased exponent 67..186) or a == +-0, branch-free.
// True when all four numerators lie in [2^-60, 2^60].  Exact zeros fail
// too (they are rare, and the caller's IEEE fallback handles them), which lets
// the test be two 3-input min/max ops and two compares.  A NaN numerator may
// pass: both division paths then yield NaN, which the score clamps anyway.
__device__ __forceinline__ bool markstein_ok4(float a, float b, float c, float d) {
  const float ma = __builtin_fabsf(a), mb = __builtin_fabsf(b);
  const float mc = __builtin_fabsf(c), md = __builtin_fabsf(d);
  const float hi = __builtin_fmaxf(__builtin_fmaxf(ma, mb), __builtin_fmaxf(mc, md));
  const float lo = __builtin_fminf(__builtin_fminf(ma, mb), __builtin_fminf(mc, md));
  return (hi <= 0x1p60f) & (lo >= 0x1p-60f);
}

struct BlockSpan {
  int64_t off;
  int64_t d;
};

__device__ __forceinline__ BlockSpan block_span(const int64_t* __restrict__ block_off,
                                                int64_t ud, int64_t g) {
  if (block_off == nullptr) return BlockSpan{g * ud, ud};
  int64_t a = block_off[g];
  int64_t b = block_off[g + 1];
  return BlockSpan{a, b - a};
}

__device__ __forceinline__ int32_t block_seed(int32_t seed, int64_t block_id) {
  return (int32_t)((uint32_t)seed + (uint32_t)block_id);
}

// The encoders' block seeds: block g of a launch is coded with seed
// `seed + base + g` (coded_greedy_sampler.py:282), or with per_block[g] when
// the launch codes several independent jobs at once (a batch of images, each
// numbering its groups from 0 with its own seed).
struct SeedSpec {
  int32_t seed;
  int64_t base;
  const int32_t* per_block;  // device [nb] or nullptr
  __device__ __forceinline__ int32_t of(int64_t g) const {
    return per_block ? per_block[g] : block_seed(seed, base + g);
  }
};

__device__ __forceinline__ uint32_t ord_f32(float v) {
  const uint32_t b = f2u(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unord_f32(uint32_t o) {
  return u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
#ifndef CWQ_WAVE_MAX_ASM
#define CWQ_WAVE_MAX_ASM 1  // 1: one v_max_f32_dpp per step (inline asm)
#endif
// Wave-wide max with GFX9 DPP (quad perms, row mirrors, row_bcast:15/31):
// six v_max_f32_dpp and one readlane.  Requires a full exec mask.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float v) {
  const int ninf = (int)0xff800000u;  // -inf: identity for the rows DPP leaves unwritten
  const int o = __builtin_amdgcn_update_dpp(ninf, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf,
                                            false);
  return fmaxf(v, __builtin_bit_cast(float, o));
}
#if CWQ_WAVE_MAX_ASM
// The same six steps as one v_max_f32_dpp each: v = max(v[dpp], v), and lanes a
// step's row mask leaves unwritten keep v.  Through the builtins each step is a
// v_mov_b32_dpp from a -inf "old" value plus two v_max_f32 (fmaxf's IEEE
// canonicalisation of the moved value): 25 VALU instructions against 6 (the
// tau sharing of the pruned loops, every 16 units).  Each step starts with the
// two wait states a DPP read of a VGPR written by the previous VALU needs, and
// the last ends with them before the readlane.  tau is never a signalling NaN,
// for which the two forms would differ.
#define CWQ_DPP_MAX_STEP(v, ctl, rmask) \
  asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " ctl " row_mask:" rmask " bank_mask:0xf" \
               : "+v"(v))
__device__ __forceinline__ float wave_max_f32(float v) {
  CWQ_DPP_MAX_STEP(v, "quad_perm:[1,0,3,2]", "0xf");
  CWQ_DPP_MAX_STEP(v, "quad_perm:[2,3,0,1]", "0xf");
  CWQ_DPP_MAX_STEP(v, "row_half_mirror", "0xf");
  CWQ_DPP_MAX_STEP(v, "row_mirror", "0xf");
  CWQ_DPP_MAX_STEP(v, "row_bcast:15", "0xa");
  CWQ_DPP_MAX_STEP(v, "row_bcast:31", "0xc");
  asm volatile("s_nop 1" : "+v"(v));
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
#else
__device__ __forceinline__ float wave_max_f32(float v) {
  v = dpp_max_step<0xb1, 0xf>(v);   // quad_perm [1,0,3,2]
  v = dpp_max_step<0x4e, 0xf>(v);   // quad_perm [2,3,0,1]
  v = dpp_max_step<0x141, 0xf>(v);  // row_half_mirror
  v = dpp_max_step<0x140, 0xf>(v);  // row_mirror: every lane holds its row's max
  v = dpp_max_step<0x142, 0xa>(v);  // row_bcast:15 into rows 1, 3
  v = dpp_max_step<0x143, 0xc>(v);  // row_bcast:31 into rows 2, 3: lane 63 holds the max
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
#endif
// max(a, b) as one v_max_f32, for thresholds that are never NaN.  fmaxf adds a
// v_max_f32 x, x, x per operand the compiler cannot prove quiet (a value out of
// a readlane or an LDS atomic, for instance).
__device__ __forceinline__ float max_f32_quiet(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// The pruned loops' threshold tau, kept wave-uniform.  Raising it: the wave max
// of `lower` over the lanes with `on` set (the others contribute the identity,
// -inf; a NaN `lower` is dropped, as fmaxf would), then every lane's
// tau = max(tau, that).  Requires a full exec mask, so the caller branches on
// the ballot of `on`, not on `on`.
__device__ __forceinline__ float tau_raise_wave(float tau, bool on, float lower) {
  return max_f32_quiet(tau, wave_max_f32((on && lower == lower) ? lower : -__builtin_inff()));
}
// Sharing it through the workgroup's LDS cell (a float, never NaN): lane 0
// does one returning max, cell = max(cell, tau), and every lane takes
// max(tau, old cell).  tau is the same in all lanes before and after.
// Written out, with the exec mask set to lane 0 around the one ds_max_rtn_f32:
// as an atomicrmw the compiler's atomic optimizer wraps it in a lane election
// of its own (two v_mbcnt and a compare) or, for a value it cannot prove
// uniform, in a lane-by-lane reduction loop.  Full exec mask on entry.
__device__ __forceinline__ float tau_share_wave(float* cell, float tau) {
  const uint32_t addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float*)cell;
  uint64_t sv;
  float old;
  int oldu;
  asm volatile(
      "s_mov_b64 %1, exec\n\t"
      "s_mov_b64 exec, 1\n\t"
      "ds_max_rtn_f32 %0, %2, %3\n\t"
      "s_mov_b64 exec, %1\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(old), "=&s"(sv)
      : "v"(addr), "v"(tau)
      : "memory");
  oldu = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, old));
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "s"(oldu), "v"(tau));
  return r;
}
// Sum over each 16-lane DPP row, the same value in all 16 lanes: butterflies
// (quad xor 1, quad xor 2, half-row mirror, row mirror) pair lanes
// symmetrically and float addition commutes, so every lane forms the
// identical ((x0+x1)+(x2+x3)) + ... tree.  Requires a full exec mask.
template <int CTRL>
__device__ __forceinline__ float dpp_add_step(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false);
  return v + __builtin_bit_cast(float, o);
}
__device__ __forceinline__ float row16_sum_f32(float v) {
  v = dpp_add_step<0xb1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add_step<0x4e>(v);   // quad_perm [2,3,0,1]
  v = dpp_add_step<0x141>(v);  // row_half_mirror: quad 0 <-> quad 1 of each half row
  v = dpp_add_step<0x140>(v);  // row_mirror: half 0 <-> half 1
  return v;
}

// The span vote of k_small_screen and k_small_one.  A lane holds the screened
// sums rs of its span's four rows ns .. ns + 3 (those below n1 exist).  tau is
// raised from the lane's best row: the lower bound is monotone in the screened
// value, and any row's lower bound is a valid threshold, so one wave max per
// span replaces one per row.  Then one ballot per row: m[q] holds the lanes
// whose row q exists and whose upper bound reaches tau.  Returns the number of
// such rows in the wave.  Requires a full exec mask.
__device__ __forceinline__ uint32_t span_vote(const float (&rs)[4], int64_t ns, int64_t n1,
                                              float c1, float c2, float As, float Pq, float B,
                                              float& tau, uint64_t (&m)[4]) {
  float smax = -__builtin_inff();
  bool any = false;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq)
    if (ns + qq < n1) {
      smax = fmaxf(smax, rs[qq]);
      any = true;
    }
  const float lower = any ? screen_row_lower(smax, c2, As, Pq) : -__builtin_inff();
  tau = fmaxf(tau, wave_max_f32(lower));
  uint32_t cnt = 0;
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    m[qq] = __ballot(ns + qq < n1 && screen_row_upper(rs[qq], c1, B) >= tau);
    cnt += (uint32_t)__builtin_popcountll(m[qq]);
  }
  return cnt;
}
template <int DC, class ElemF>
__device__ __forceinline__ float eval_row_f(const PhiloxStream& st, uint64_t kbase, int64_t d_rt,
                                            int align_rt, const double* logtab, ElemF&& val) {
  const int64_t d = DC > 0 ? (int64_t)DC : d_rt;
  const int align = (DC > 0 && (DC % 4) == 0) ? 0 : align_rt;
  const int64_t vec = d & ~(int64_t)7;
  float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  F4 z = {0.f, 0.f, 0.f, 0.f};

  auto elem = [&](int64_t e) -> float {
    const int w = (align + (int)(e & 3)) & 3;  // wave-uniform
    if (w == 0 || e == 0) z = normal4_dev(st, (kbase + (uint64_t)e) >> 2, logtab);
    const float zz = w == 0 ? z.a : (w == 1 ? z.b : (w == 2 ? z.c : z.d));
    return val(e, zz);
  };

  for (int64_t j = 0; j < vec; j += 8) {
#pragma unroll
    for (int l = 0; l < 8; ++l) p[l] = p[l] + elem(j + l);
  }
  float t = 0.0f;
  for (int64_t j = vec; j < d; ++j) t = t + elem(j);
  return eigen_fold8(p, t);
}

// grid_for: cwq_dispatch.h (the decode plan computes launch sizes with it)

}  // namespace cwq
