// The fp16 scan's band (tostore_amd/csrc/tsh_scan_f16_band.h, host only) behind one C entry point, for tests that
// need the band of a query from the header itself and not from the library under test: tests/test_gpu_scan_widths.py
// compiles this with g++ into a shared object of its own and calls it through ctypes.
// out: alpha, beta, w_max (w_i = alpha |v_i| + beta).  Returns 1 when the query is inside the model, 0 otherwise.
#include "../../tostore_amd/csrc/tsh_scan_f16_band.h"
#include "../../tostore_amd/csrc/tsh_scan_widths.h"

extern "C" int scan_f16_band_of(int metric, int dim, const float *q, float max_norm, float min_norm, float max_abs, float *out) {
  int v_exp = 0;
  if (!tsh::scan_f16_exp(max_abs, &v_exp)) return 0;
  const tsh::ScanF16Band b = tsh::scan_f16_band(metric, dim, tsh::pick_nch((dim + 3) / 4), q, max_norm, min_norm, v_exp);
  out[0] = b.alpha;
  out[1] = b.beta;
  out[2] = b.w_max;
  return b.ok ? 1 : 0;
}

// The scale of the fp16 copy for a shard whose largest |element| is max_abs: *v_exp is set either way.  Returns 1 when
// the scale is inside the guard of scan_f16_exp, 0 when the scan stays on f32 (tests/scale_inputs.py).
extern "C" int scan_f16_exp_of(float max_abs, int *v_exp) { return tsh::scan_f16_exp(max_abs, v_exp) ? 1 : 0; }
