// The int8 scan's band (tostore_amd/csrc/tsh_scan_i8_band.h, host only) behind C entry points, for tests that need the
// band of a query and the scale of a row from the header itself and not from the library under test:
// tests/scale_inputs.py compiles this with g++ into a shared object of its own and calls it through ctypes.
#include "../../tostore_amd/csrc/tsh_scan_i8_band.h"
#include "../../tostore_amd/csrc/tsh_scan_widths.h"

// out: a_s, a_v, beta, qbias (L2 / IP: w_i = a_s s_i + a_v |v_i| + beta; cosine: w_i = a_s s_i / |v_i| + beta).
// Returns 1 when the query is inside the model, 0 otherwise.
extern "C" int scan_i8_band_of(int metric, int dim, const float *q, float max_norm, float min_norm, float max_abs, float *out) {
  const tsh::ScanI8Band b = tsh::scan_i8_band(metric, dim, tsh::pick_nch((dim + 3) / 4), q, max_norm, min_norm, max_abs);
  out[0] = b.a_s;
  out[1] = b.a_v;
  out[2] = b.beta;
  out[3] = b.qbias;
  return b.ok ? 1 : 0;
}

// the scale of a row of the copy, from its largest |element|
extern "C" float scan_i8_scale_of(float mx) { return tsh::scan_i8_scale(mx); }
