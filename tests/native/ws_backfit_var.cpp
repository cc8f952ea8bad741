// Host build of backfit_var_ws (csrc/cwq_workspace.h) for
// tests/test_backfit_var_capi.py, in ws_layout.cpp's text form: "name off
// bytes" per region, then "total N"; `name!` is packed right behind the region
// before it.  Test-only shim; not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../compression_without_quantization_amd/csrc/cwq_dispatch.h"
#include "../../compression_without_quantization_amd/csrc/cwq_workspace.h"

extern "C" {

// v = (csr, nb, total_dims, max_block_dim, n_steps).  Returns the text's
// length, or -2 when cap is too small.
int wsb_dump(const int64_t* v, char* out, int cap) {
  using namespace cwq;
  const BackfitVarWs l = backfit_var_ws(v[0] != 0, v[1], v[2], v[3], (int)v[4]);
  static const char* const sorted[] = {"sorted_in", "t_loc",   "t_scale", "p_loc",
                                       "p_scale",   "sample",  "seeds",   "perm",
                                       "hist",      "counts",  "wgfacts", "facts",
                                       "soff",      "roff",    "src",     "partial"};
  static const char* const own[] = {"bad!", "table", "enc", "rows", "value", "count"};
  int n = 0;
  // regions [r, end) under the names (one per region)
  auto regions = [&](const Region* r, const void* end, const char* const* names, size_t count) {
    if ((size_t)((const Region*)end - r) != count) return false;
    for (size_t i = 0; i < count; ++i) {
      const int w = snprintf(out + n, cap - n, "%s %zu %zu\n", names[i], r[i].off, r[i].bytes);
      if (w < 0 || w >= cap - n) return false;
      n += w;
    }
    return true;
  };
  if (!regions(&l.s.sorted_in, &l.bad, sorted, sizeof(sorted) / sizeof(sorted[0])) ||
      !regions(&l.bad, &l.total, own, sizeof(own) / sizeof(own[0])))
    return -2;
  const int w = snprintf(out + n, cap - n, "total %zu\n", l.total);
  if (w < 0 || w >= cap - n) return -2;
  return n + w;
}

// The encoder layout's total for a bucket's shape: ragged (nb, dims, longest)
// or uniform (nb, d).
int64_t wsb_enc_total(int csr, int64_t nb, int64_t dims, int64_t longest) {
  return (int64_t)(csr ? cwq::enc_ws_csr(nb, dims, longest) : cwq::enc_ws_uniform(nb, longest))
      .total;
}
// The last array of the layout nested in `enc` ends inside it.
int64_t wsb_encl_total(const int64_t* v) {
  return (int64_t)cwq::backfit_var_ws(v[0] != 0, v[1], v[2], v[3], (int)v[4]).encl.total;
}
}
