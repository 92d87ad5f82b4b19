// The batched call's plan (tostore_amd/csrc/tsh_batch_plan.h) and tile order (tsh_batch_tiles.h), both host only, behind
// C entry points: tests/batch_shape_inputs.py compiles this with g++ into a shared object of its own and calls it through
// ctypes, so that the tests of the batched key kernels take the sample's size and place, the tiles, the candidate cap and
// the keys' error bounds from the headers themselves -- neither from the library under test nor from copied numbers.
#include "../../tostore_amd/csrc/tsh_batch_plan.h"
#include "../../tostore_amd/csrc/tsh_batch_tiles.h"

namespace {
tsh::BatchShardFacts facts(int metric, int dim, int64_t rows, float max_norm, float min_norm, float max_abs, int kernel, int group) {
  tsh::BatchShardFacts s;
  s.rows = rows;
  s.cap = rows;
  s.ld = tsh::round_up(dim, 4);
  s.dim = dim;
  s.metric = metric;
  s.max_norm = max_norm;
  s.min_norm = min_norm;
  s.max_abs = max_abs;
  s.batch_kernel = kernel;
  s.batch_group = group != 0;
  return s;
}
}  // namespace

// out: tile, nq_pad, kern, hchunks, tile_n, n_sample, k_est, cand_cap, want_group, listed, scan_rows.  kept: rows a
// pointer mask keeps, -1 without a mask.
extern "C" void batch_plan_of(int metric, int dim, int64_t rows, float max_norm, float min_norm, float max_abs, int kernel,
                              int group, int nq, int k, int64_t kept, int64_t *out) {
  const tsh::BatchShardFacts s = facts(metric, dim, rows, max_norm, min_norm, max_abs, kernel, group);
  tsh::BatchCallFacts c;
  c.nq = nq;
  c.k = k;
  c.mask = kept >= 0 ? tsh::BatchMask::POINTER : tsh::BatchMask::NONE;
  c.kept = kept;
  const tsh::BatchPlan p = tsh::plan_batch(s, c);
  const int64_t v[11] = {p.tile, p.nq_pad, p.kern, p.hchunks, p.tile_n, p.n_sample, p.k_est, p.cand_cap, p.want_group, p.listed, p.scan_rows};
  for (int i = 0; i < 11; ++i) out[i] = v[i];
}

// out: delta2 (twice the shared part of the bound), alpha (the per-row part; 0 but for fp16 keys of L2 / inner product),
// chain2.  A key of row v is within alpha |v| + delta2 / 2 (+ chain |thr'|, fp16 L2 / IP) of its exact value.
extern "C" int batch_band_of(int metric, int dim, int64_t rows, float max_norm, float min_norm, float max_abs, int kernel,
                             double qn2, float *out) {
  const tsh::BatchShardFacts s = facts(metric, dim, rows, max_norm, min_norm, max_abs, kernel, 1);
  float d2 = 0.f, qsq = 0.f, alpha = 0.f;
  if (!tsh::batch_delta2(s, kernel, qn2, &d2, &qsq, &alpha)) return 0;
  out[0] = d2;
  out[1] = alpha;
  out[2] = tsh::batch_chain2(s, kernel);
  return 1;
}

// The sample's window behind a mask: pre[t] = kept rows in the mask's 64-row words [0, t).  out: s0, rows it keeps.
extern "C" void batch_sample_window_of(const int32_t *pre, int32_t n_words, int64_t rows, int64_t n_sample, int group, int64_t *out) {
  const tsh::SampleWindow w = tsh::sample_window(pre, n_words, rows, n_sample, group != 0);
  out[0] = w.s0;
  out[1] = w.best;
}

// The power-of-two scale of the fp16 operands whose largest magnitude is `top` (rows: f16_rows_top; queries: the batch's
// largest element).  Returns 1 inside the guard of f16_scale_exp, 0 where the plan turns to bf16x3 (rows) or the batch
// answers its queries one by one (queries); *exp is set either way (tests/scale_inputs.py).
extern "C" int batch_f16_scale_exp_of(float top, int *exp) { return tsh::f16_scale_exp(top, exp) ? 1 : 0; }

// Does a call of nq queries on a shard of `rows` rows go to the matrix cores (shard_takes_batch)?  batch_min_nq: the
// option (0 never, 1 by cost, n >= 2 from n queries on).
extern "C" int batch_takes_of(int metric, int dim, int64_t rows, int batch_min_nq, int nq, int k) {
  const tsh::BatchShardFacts s = facts(metric, dim, rows, 1.f, 1.f, 1.f, 3, 1);
  return tsh::shard_takes_batch(s, batch_min_nq, nq, k) ? 1 : 0;
}

extern "C" int batch_k_est_of(int k, int64_t rows, int64_t n_sample) { return tsh::batch_k_est(k, rows, n_sample); }

extern "C" void batch_tile_slot(int q_tiles, int n_tiles, int b, int *out) { tsh::batch_tile_of(q_tiles, n_tiles, b, &out[0], &out[1]); }
