// Host build of the product's device-math restatement (csrc/cwq_math.h) and of
// the screening bound (csrc/cwq_screen.h), of the encode and decode dispatch
// (csrc/cwq_dispatch.h) and of the importance coder's launch plan
// (csrc/cwq_imp_plan.h).  tests/test_math_exhaustive.py compares the first
// with the host glibc over the full Box-Muller input domains;
// tests/test_screen_bound.py checks the second's inequalities,
// tests/test_encode_plan.py and tests/test_decode_plan.py the third's tables
// of shapes and
// tests/test_importance_plan.py the fourth's; tests/test_imp_screen_bound.py
// checks the importance coder's screening bound (csrc/cwq_imp_screen.h).
// Test-only shim; not part of the product.
#include <stdint.h>
#include <vector>
#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"
#include "../../compression_without_quantization_amd/csrc/cwq_imp_plan.h"
#include "../../compression_without_quantization_amd/csrc/cwq_imp_screen.h"
#include "../../compression_without_quantization_amd/csrc/cwq_math.h"
#include "../../compression_without_quantization_amd/csrc/cwq_screen.h"

static const double kTab[32] = CWQ_LOGF_TAB_INIT;

extern "C" {
void mc_bm_radius_table(uint32_t m0, int64_t count, float* out) {
  for (int64_t i = 0; i < count; ++i) out[i] = cwq::bm_radius((uint32_t)(m0 + i), kTab);
}
void mc_bm_sincos_table(uint32_t m0, int64_t count, float* s, float* c) {
  for (int64_t i = 0; i < count; ++i) cwq::sincosf_pos(cwq::bm_angle((uint32_t)(m0 + i)), s[i], c[i]);
}
void mc_bm_angle_table(uint32_t m0, int64_t count, float* out) {
  for (int64_t i = 0; i < count; ++i) out[i] = cwq::bm_angle((uint32_t)(m0 + i));
}
void mc_logf_table(const float* x, int64_t n, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = cwq::logf_full(x[i], kTab);
}
void mc_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  cwq::U4 r = cwq::philox10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}
void mc_philox_many(const uint32_t* ctr, const uint32_t* key, int64_t n, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) mc_philox(ctr + 4 * i, key + 2 * i, out + 4 * i);
}

// out = fmaf(a, b, c), one rounding (numpy has no float fma)
void mc_fmaf_many(int64_t n, const float* a, const float* b, const float* c, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = __builtin_fmaf(a[i], b[i], c[i]);
}
double mc_screen_ez(void) { return cwq::kScreenEz; }
double mc_screen_sqrt2ln2(void) { return cwq::kSqrt2Ln2; }

// out = (sa, sb, A, C, ok)
void mc_screen_dim(int step0, float ls, float ss, float mu, float sg, float c, float bb,
                   float* out) {
  const cwq::ScreenDim o = step0 ? cwq::screen_dim<true>(ls, ss, mu, sg, c, bb)
                                 : cwq::screen_dim<false>(ls, ss, mu, sg, c, bb);
  out[0] = o.sa; out[1] = o.sb; out[2] = o.A; out[3] = o.C; out[4] = o.ok ? 1.0f : 0.0f;
}
// n dims at once: out[5 n]
void mc_screen_dim_many(int64_t n, const uint8_t* step0, const float* ls, const float* ss,
                        const float* mu, const float* sg, const float* c, const float* bb,
                        float* out) {
  for (int64_t i = 0; i < n; ++i)
    mc_screen_dim(step0[i], ls[i], ss[i], mu[i], sg[i], c[i], bb[i], out + 5 * i);
}
// sums = (sum M, sum |M|, sum (|M| + M), sum A^2, sum C, max A, ok);
// out = (gamma, sl, c1, c2, As, Pq, B, finite)
void mc_screen_block(const double* sums, int64_t d, double h_s, double* out) {
  cwq::ScreenSums u;
  u.sm = sums[0]; u.sa = sums[1]; u.sk = sums[2]; u.s2 = sums[3]; u.cs = sums[4]; u.mx = sums[5];
  u.ok = sums[6] != 0.0;
  const cwq::ScreenBlock b = cwq::screen_block_consts(u, d, h_s);
  out[0] = b.gam; out[1] = b.sl; out[2] = b.c1; out[3] = b.c2; out[4] = b.as; out[5] = b.pq;
  out[6] = b.bf; out[7] = b.finite ? 1.0 : 0.0;
}

// A block of d dims (its sums accumulated as k_small_prep does, h_s = d) and
// rows of it: zp[r d + j] the screening normals z' of row r, lp[r d + j] the
// exact float log-densities.  For each row s = the sequential sum of -a^2, E =
// the Eigen-order sum of lp, and out[3 r ..] = (lower, E, upper).  Returns 1,
// or 0 when the block fails k_small_prep's gate (out is then untouched).
int mc_screen_row_bounds(int step0, int64_t d, const float* ls, const float* ss, const float* mu,
                         const float* sg, const float* c, const float* bb, int64_t rows,
                         const float* zp, const float* lp, float* out) {
  cwq::ScreenSums u;
  std::vector<cwq::ScreenDim> o(d);
  for (int64_t j = 0; j < d; ++j) {
    o[j] = step0 ? cwq::screen_dim<true>(ls[j], ss[j], mu[j], sg[j], c[j], bb[j])
                 : cwq::screen_dim<false>(ls[j], ss[j], mu[j], sg[j], c[j], bb[j]);
    u.add(o[j]);
  }
  const cwq::ScreenBlock b = cwq::screen_block_consts(u, d, (double)d);
  if (!(u.ok && b.finite && b.bf - b.bf == 0.0f && d > 0)) return 0;
  for (int64_t r = 0; r < rows; ++r) {
    float s = 0.0f;
    for (int64_t j = 0; j < d; ++j) {
      const float a = __builtin_fmaf(o[j].sa, zp[r * d + j], o[j].sb);
      s = __builtin_fmaf(-a, a, s);
    }
    const float* x = lp + r * d;
    const int64_t vec = d & ~(int64_t)7;
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t j = 0; j < vec; j += 8)
      for (int l = 0; l < 8; ++l) p[l] = p[l] + x[j + l];
    float t = 0.0f;
    for (int64_t j = vec; j < d; ++j) t = t + x[j];
    out[3 * r] = cwq::screen_row_lower(s, b.c2, b.as, b.pq);
    out[3 * r + 1] = cwq::eigen_fold8(p, t);
    out[3 * r + 2] = cwq::screen_row_upper(s, b.c1, b.bf);
  }
  return 1;
}

// The importance coder's screening bound (csrc/cwq_imp_screen.h).
// n dims at once: out[7 n] = (A, B, C, err, mag, umax, gated in)
void mc_imp_screen_dim_many(int64_t n, const float* tl, const float* ts, const float* pl,
                            const float* ps, const float* ct, const float* cp, float* out) {
  for (int64_t i = 0; i < n; ++i) {
    cwq::ImpScreenDim o = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool ok = cwq::imp_screen_dim(tl[i], ts[i], pl[i], ps[i], ct[i], cp[i], o);
    float* q = out + 7 * i;
    q[0] = o.A; q[1] = o.B; q[2] = o.C; q[3] = o.err; q[4] = o.mag; q[5] = o.umax;
    q[6] = ok ? 1.0f : 0.0f;
  }
}
// screened[i] = the screened term of dim constants (A, B, C) at z'
void mc_imp_screen_term_many(int64_t n, const float* A, const float* B, const float* C,
                             const float* zp, float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = cwq::imp_screen_term(A[i], B[i], C[i], zp[i]);
}
// A group of d dims (its row bound E and suffix sums as thread 0 of k_imp_eval
// builds them) and rows of it: zp[r d + j] the screening normals z' of row r,
// tx[r d + j] the exact float terms.  For each row, in the kernel's float
// order: out[4 r ..] = (s, slack, exact, E) with s the screened sum of the
// completed row, slack = imp_screen_slack(E, s) and exact the Eigen-order sum
// of tx; pre[4 r + a] = the least (s_j + slack_j) + dsuf[j] - exact over the
// prefix lengths j < d at which the pruned loop tests a row whose first Philox
// block is entered at word a (j = 4 - a, 8 - a, ...), +inf if there is none.
// dsuf_out (d + 1 floats, may be null) gets the suffix sums.  Returns 1, or 0
// when the value gate rejects a dim or E is not finite (outputs untouched).
int mc_imp_screen_row_bounds(int64_t d, const float* tl, const float* ts, const float* pl,
                             const float* ps, const float* ct, const float* cp, int64_t rows,
                             const float* zp, const float* tx, float* out, double* pre,
                             float* dsuf_out) {
  if (d < 1 || d > cwq::kImpScreenMaxD) return 0;
  std::vector<cwq::ImpScreenDim> o(d);
  std::vector<float> derr(d), dmag(d), dumax(d), dsuf(d + 1);
  for (int64_t j = 0; j < d; ++j) {
    if (!cwq::imp_screen_dim(tl[j], ts[j], pl[j], ps[j], ct[j], cp[j], o[j])) return 0;
    derr[j] = o[j].err; dmag[j] = o[j].mag; dumax[j] = o[j].umax;
  }
  const float E = cwq::imp_screen_row_bound(derr.data(), dmag.data(), d);
  cwq::imp_screen_suffix(dumax.data(), d, dsuf.data());
  if (!(E - E == 0.0f)) return 0;
  if (dsuf_out) for (int64_t j = 0; j <= d; ++j) dsuf_out[j] = dsuf[j];
  for (int64_t r = 0; r < rows; ++r) {
    const float* x = tx + r * d;
    const int64_t vec = d & ~(int64_t)7;
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t j = 0; j < vec; j += 8)
      for (int l = 0; l < 8; ++l) p[l] = p[l] + x[j + l];
    float t = 0.0f;
    for (int64_t j = vec; j < d; ++j) t = t + x[j];
    const float exact = cwq::eigen_fold8(p, t);
    double least[4] = {__builtin_inf(), __builtin_inf(), __builtin_inf(), __builtin_inf()};
    float s = 0.0f;
    for (int64_t j = 0; j < d; ++j) {
      s = s + cwq::imp_screen_term(o[j].A, o[j].B, o[j].C, zp[r * d + j]);
      const int64_t v = j + 1;  // dims visited
      if (v == d) break;
      const float slack = cwq::imp_screen_slack(E, s);
      const float upper = cwq::imp_screen_upper(s, slack, dsuf[v]);
      const int a = (int)((4 - (v & 3)) & 3);  // the loop stops after v dims iff v = 4 - a mod 4
      const double m = (double)upper - (double)exact;
      least[a] = m < least[a] ? m : least[a];
    }
    out[4 * r] = s;
    out[4 * r + 1] = cwq::imp_screen_slack(E, s);
    out[4 * r + 2] = exact;
    out[4 * r + 3] = E;
    for (int a = 0; a < 4; ++a) pre[4 * r + a] = least[a];
  }
  return 1;
}

// The encode dispatch (csrc/cwq_dispatch.h) of one block range.
// out = (path, coop, self_finalizing, fork parts); path in EncodePath's order.
void mc_encode_plan(int csr, int64_t ud, int64_t max_d, int64_t nb, int64_t n_cand, int prune,
                    int rows_wave, int n_steps, int* out) {
  const cwq::EncodeShape s = {csr != 0, ud, max_d, nb, n_cand, prune, rows_wave != 0};
  const cwq::EncodePlan p = cwq::encode_plan(s);
  out[0] = (int)p.path; out[1] = p.coop; out[2] = p.self_finalizing;
  out[3] = cwq::encode_fork_parts(s, n_steps);
}
int mc_has_screen_arrays(int csr, int64_t ud, int64_t nb) {
  return cwq::has_screen_arrays(csr != 0, ud, nb);
}
int mc_has_long_block_records(int csr, int64_t max_d, int64_t nb) {
  return cwq::has_long_block_records(csr != 0, max_d, nb);
}
int mc_few_rows(int64_t nb, int64_t n_cand) { return cwq::few_rows(nb, n_cand); }
int mc_bucket_takes_rows_wave(int bits, int64_t dims, int64_t count, int prune) {
  return cwq::bucket_takes_rows_wave(bits, dims, count, prune);
}
// (CWQ_CSR_COOP_ROWS_PER_LANE * lanes of the chip, CWQ_CSR_COOP_MIN_D, CWQ_CSR_LDS_DIMS)
void mc_dispatch_consts(int64_t* out) {
  out[0] = (int64_t)CWQ_CSR_COOP_ROWS_PER_LANE * cwq::kChipLanes;
  out[1] = CWQ_CSR_COOP_MIN_D;
  out[2] = CWQ_CSR_LDS_DIMS;
}
// The uniform encoder's tiling and k_encode_prune's tile queue.
// out = (tiles_per_block, cand_per_tile, CWQ_QUEUE_MIN_CPT, CWQ_QUEUE_GRID).
void mc_choose_tiling(int64_t nb, int64_t n_cand, int64_t* out) {
  cwq::choose_tiling(nb, n_cand, &out[0], &out[1]);
  out[2] = CWQ_QUEUE_MIN_CPT;
  out[3] = CWQ_QUEUE_GRID;
}
int mc_takes_tile_queue(int64_t ntiles, int64_t cand_per_tile, int64_t queue_grid) {
  return cwq::takes_tile_queue(ntiles, cand_per_tile, queue_grid);
}

// The decode dispatch (csrc/cwq_dispatch.h) of one launch_decode call.
// out = (kernel, qpb, bpw, groups, workgroups); kernel in DecodeKernel's order.
void mc_decode_plan(int csr, int64_t ud, int64_t nb, int64_t total_dims, int n_steps,
                    int aligned16, int64_t* out) {
  const cwq::DecodePlan p =
      cwq::decode_plan(cwq::DecodeShape{csr != 0, ud, nb, total_dims, n_steps, aligned16 != 0});
  out[0] = (int64_t)p.kernel; out[1] = p.qpb; out[2] = p.bpw; out[3] = p.groups;
  out[4] = p.workgroups;
}
// (k_decode's grid cap, the q4 kernels' grid cap, CWQ_DECODE_GLDS)
void mc_decode_consts(int64_t* out) {
  out[0] = cwq::kDecodeGeneralGridCap; out[1] = cwq::kDecodeQ4GridCap; out[2] = CWQ_DECODE_GLDS;
}

// The importance coder's launch plan (csrc/cwq_imp_plan.h).
// out = (T, tile size, tiles, small groups, dynamic, permuted, multiplier,
// PER_BLOCK, CPT_MAX, k_imp_tiles in registers); forms[g] (may be null) =
// ImpRowForm | 0x80 when the group's screening counters are 32-bit (HI0).
void mc_importance_plan(const int64_t* n_samples, const int64_t* block_off, int64_t nb,
                        int total_known, int per_block_seeds, int allow_screen, int64_t* out,
                        uint8_t* forms) {
  const cwq::ImpLaunchPlan p = cwq::imp_launch_plan(n_samples, block_off, nb, total_known != 0,
                                                    per_block_seeds != 0, allow_screen, forms);
  out[0] = p.total_cands; out[1] = p.cpt; out[2] = p.tiles; out[3] = p.small_groups;
  out[4] = p.dynamic; out[5] = p.permuted; out[6] = (int64_t)p.multiplier;
  out[7] = p.per_block; out[8] = p.cpt_max; out[9] = p.tiles_in_regs;
}
// importance_tile_count's definition (the launcher's hand-out argument)
int64_t mc_importance_tile_count(const int64_t* n_samples, int64_t nb, int64_t total_cands) {
  return cwq::imp_tile_count(n_samples, nb, total_cands);
}
int64_t mc_importance_cand_per_tile(int64_t T) { return cwq::imp_cand_per_tile(T); }
// (kImpSmallN, kImpMinCandPerTile, kImpCandPerTile, CWQ_IMP_TARGET_TILES,
//  CWQ_IMP_DYNAMIC_MIN_GROUPS, CWQ_IMP_DYNAMIC_MIN_TILES, register rounds of
//  k_imp_tiles x groups per round, kImpPruneMinD, kImpScreenMaxD,
//  CWQ_IMP_SURVIVOR_CAP)
void mc_importance_consts(int64_t* out) {
  out[0] = cwq::kImpSmallN; out[1] = cwq::kImpMinCandPerTile; out[2] = cwq::kImpCandPerTile;
  out[3] = CWQ_IMP_TARGET_TILES; out[4] = CWQ_IMP_DYNAMIC_MIN_GROUPS;
  out[5] = CWQ_IMP_DYNAMIC_MIN_TILES;
  out[6] = (int64_t)cwq::kImpTilesRegRounds * cwq::kImpTilesRound;
  out[7] = cwq::kImpPruneMinD; out[8] = cwq::kImpScreenMaxD; out[9] = CWQ_IMP_SURVIVOR_CAP;
}
}
