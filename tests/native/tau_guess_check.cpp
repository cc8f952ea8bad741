// Host run of csrc/cwq_tau_guess.h for tests/test_tau_guess.py.
//
// Reads sections from the file named on the command line:
//   int64 nb, d, n_cand; float32 [nb][d][5] = loc_s, scale_s, mu, sigma, best
// For every block it forms the screening constants as k_encode_prune does
// (screen_dim of cwq_screen.h; alpha = sa / sqrt(2 ln 2), beta = sb), at step 0
// (best ignored) and at a later step (beta shifted by best), and prints one
// line per block and step:
//   q_m alpha_0 .. alpha_{d-1} beta_0 .. beta_{d-1}
// with q_m = tau_guess_q(...) (-1: no guess).  The first line is "m <M>", the
// compiled-in CWQ_TAU_GUESS_M; the last is "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../compression_without_quantization_amd/csrc/cwq_screen.h"
#include "../../compression_without_quantization_amd/csrc/cwq_tau_guess.h"

template <bool STEP0>
static void one(const float* blk, int d, int64_t n_cand) {
  std::vector<float> al(d), be(d);
  const float inv = (float)(1.0 / cwq::kSqrt2Ln2);
  for (int j = 0; j < d; ++j) {
    const float* f = blk + 5 * j;
    const float c = cwq::kHalfLog2Pi + logf(f[3]);
    const cwq::ScreenDim o = cwq::screen_dim<STEP0>(f[0], f[1], f[2], f[3], c, f[4]);
    al[j] = o.sa * inv;
    be[j] = o.sb;
  }
  const cwq::TauGuessHostDims dims{al.data(), be.data(), d};
  const float q = cwq::tau_guess_q(dims, n_cand, cwq::kTauGuessM);
  std::printf("%.9g", (double)q);
  for (int j = 0; j < d; ++j) std::printf(" %.9g", (double)al[j]);
  for (int j = 0; j < d; ++j) std::printf(" %.9g", (double)be[j]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  std::printf("m %d\n", cwq::kTauGuessM);
  int64_t hd[3];
  while (std::fread(hd, sizeof(int64_t), 3, fp) == 3) {
    const int64_t nb = hd[0], d = hd[1], n_cand = hd[2];
    if (nb < 0 || d < 1 || d > 4096 || nb > (1 << 20)) return 3;
    std::vector<float> buf((size_t)(nb * d * 5));
    if (std::fread(buf.data(), sizeof(float), buf.size(), fp) != buf.size()) return 3;
    for (int64_t g = 0; g < nb; ++g) {
      one<true>(buf.data() + g * d * 5, (int)d, n_cand);
      one<false>(buf.data() + g * d * 5, (int)d, n_cand);
    }
  }
  std::fclose(fp);
  std::printf("ok\n");
  return 0;
}
