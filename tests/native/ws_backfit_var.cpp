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
  static const char* const names[] = {"t_loc",   "t_scale", "p_loc", "p_scale", "sorted_in",
                                      "sample",  "seeds",   "perm",  "hist",    "counts",
                                      "bad!",    "wgfacts", "facts", "soff",    "roff",
                                      "src",     "partial", "table", "enc",     "rows",
                                      "value",   "count"};
  const Region* r = &l.t_loc;
  const int n_regions = (int)((const Region*)&l.total - r);
  if (n_regions != (int)(sizeof(names) / sizeof(names[0]))) return -2;
  int n = 0;
  for (int i = 0; i < n_regions; ++i) {
    const int w = snprintf(out + n, cap - n, "%s %zu %zu\n", names[i], r[i].off, r[i].bytes);
    if (w < 0 || w >= cap - n) return -2;
    n += w;
  }
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
