// The 4-bit first pass's band (tostore_amd/csrc/tsh_scan_i4_band.h, host only) behind C entry points, for tests that need
// the band of a query from the header itself and not from the library under test or from its NumPy model:
// tests/scan_i4_inputs.py compiles this with g++ into a shared object of its own and calls it through ctypes.
#include "../../tostore_amd/csrc/tsh_scan_i4_band.h"
#include "../../tostore_amd/csrc/tsh_scan_widths.h"

// out: a_s, a_r, a_c, a_v, beta, qbias (w_i = min(a_s s_i, a_r rho_i + a_c s_i) + a_v |v_i| + beta).  The groups are the
// row's: ld = dim rounded up to 4 elements, as the library stores it.  Returns 1 when the query is inside the model.
extern "C" int scan_i4_band_of(int dim, const float *q, float max_norm, float max_abs, float *out) {
  const long long ld = ((long long)dim + 3) / 4 * 4;
  const tsh::ScanI4Band b = tsh::scan_i4_band(dim, tsh::scan_i4_groups(ld), q, max_norm, max_abs);
  out[0] = b.a_s;
  out[1] = b.a_r;
  out[2] = b.a_c;
  out[3] = b.a_v;
  out[4] = b.beta;
  out[5] = b.qbias;
  return b.ok ? 1 : 0;
}

// does the int8 family -- and with it the 4-bit pass in front of it -- serve rows of this width?
extern "C" int scan_i4_width_ok(int dim) { return tsh::scan_i8_supported(tsh::pick_nch((dim + 3) / 4)) ? 1 : 0; }

extern "C" int scan_i4_groups_of(int dim) { return tsh::scan_i4_groups(((long long)dim + 3) / 4 * 4); }
