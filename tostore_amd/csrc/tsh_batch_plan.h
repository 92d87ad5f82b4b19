// tsh_batch_plan.h -- what a batched (matrix-core) call decides before it touches the device: whether a call is batched
// at all, which key kernel scores it and at which power-of-two scale, listed mode, the sample's size and place, the
// order statistic of the estimate, the error bands of the keys, the chunks of the tail.  Pure host arithmetic on a dozen
// facts of the shard and of the call, no HIP: compiled into the library (tsh_host_batch.inl.h carries the plan out) and,
// on its own, by tests/cpp/batch_plan_test.cpp.  Counters and flags a decision reads or moves -- the fp16 denial, the
// estimate's back-off, the probe overrides -- are the caller's: they come in as values.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/tostore_hip.h"

namespace tsh {

constexpr float BIG_ABS = 1.0e15f;  // beyond this f32 squares can overflow
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

constexpr int BATCH_TILE_ROWS = 256;     // rows of the widest key-kernel tile; the planes' row groups (PLANE_GROUP)
constexpr int BATCH_BLOCK_ROWS = 8192;   // a block of the norm-grouped plane (PG_ROWS, tsh_batch_f16.hip.h)
constexpr int BATCH_FINAL_MAX = 512;     // candidates per query the finalising kernel takes (RF_MAX, tsh_batch.hip.h)
constexpr int BATCH_EXACT_MAX = 16384;   // rows the exact scan takes at most (EX_MAX_ROWS, tsh_exact.hip.h)
constexpr int HUB_ROWS = 4096;  // sixteen 256-row tiles of the key kernel: a dense pass of 1 / 250 of a 1 M-row shard

// ---- what the decisions read ----------------------------------------------------------------------------------------
struct BatchShardFacts {
  int64_t rows = 0, cap = 0, ld = 0;
  int32_t dim = 0, metric = TSH_METRIC_L2;
  float min_norm = 0.f, max_norm = 0.f, max_abs = 0.f;
  int batch_kernel = 3;  // TSH_OPT_BATCH_KERNEL: 0 f32 MFMA, 1 bf16x3, 2 f16, 3 auto (f16_keys_fit)
  bool batch_group = true, batch_hub = false;
  int exact_rows = BATCH_EXACT_MAX;
  bool safe_mode = false;
};
enum class BatchMask { NONE, POINTER, HANDLE };
struct BatchCallFacts {
  int32_t nq = 0, k = 0;
  int32_t entries = 0;    // of a candidate block, as the call runs with them
  int force_kernel = -1;  // >= 0: that key kernel instead of the shard's option
  BatchMask mask = BatchMask::NONE;
  int64_t kept = -1;         // rows the mask keeps (tombstones not subtracted); -1: no mask
  bool handle_list = false;  // a handle's: it carries the kept rows as a list
  bool f16_denied = false;   // the automatic choice is off fp16 keys for this call (Shard::f16_denied_calls, read once)
  bool sample_force = false;  // the error-model probes: the dense sample covers every row
  int32_t est_backoff = 0;    // calls left during which the estimated threshold stays off
  int forced_tile = 0;        // experiments (TSH_BATCH_TILE): 128 or 256, else the rule's
  int sample_div = 32;        // experiments (TSH_SAMPLE_DIV): the sample is rows / this
  bool proven_tau = false;    // experiments (TSH_BATCH_PROVEN_TAU): no estimate
};

// ---- the sample -----------------------------------------------------------------------------------------------------
// Which order statistic of the sample the filter threshold is taken from (SampleSelArgs::k_est, tsh_batch.hip.h).
// The k smallest keys of all `rows` rows fall into the n_sample sample rows Binomial(k, n_sample / rows) at a time
// when rows are exchangeable; the p-th smallest sample key fails as a bound on the k-th smallest key overall only if
// p or more of them did.  p = the smallest value that makes this rarer than 1e-6 per query; B2 detects the failure
// and the query is redone, so a corpus that is NOT exchangeable (rows clustered by insertion time) costs time, never
// correctness -- and a call that sees more than a few failures switches the estimate off for the next calls.
inline int32_t batch_k_est(int32_t k, int64_t rows, int64_t n_sample, int32_t est_backoff = 0, bool proven_tau = false) {
  if (proven_tau || n_sample >= rows || n_sample <= 0 || k <= 8 || est_backoff > 0) return k;
  const double pr = (double)n_sample / (double)rows;
  if (pr > 0.5) return k;  // (most of the rows are in the sample: its k-th key is as good as proven)
  // tail P(Binomial(k, pr) >= p) from p = k downwards
  std::vector<double> pmf((size_t)k + 1);
  const double lq = std::log1p(-pr), lp = std::log(pr);
  for (int i = 0; i <= k; ++i)
    pmf[(size_t)i] = std::exp(std::lgamma(k + 1.0) - std::lgamma(i + 1.0) - std::lgamma(k - i + 1.0) + i * lp + (k - i) * lq);
  double tail = 0;
  int p = k;
  for (; p >= 1; --p) {
    tail += pmf[(size_t)p];
    if (tail > 1e-6) break;
  }
  return std::min(k, std::max(p + 1, 4));
}

// Sample size: the filtered pass keeps about k * rows / n_sample rows per query and every survivor costs an atomic
// append, so the sample grows with k (survivors <= ~3000).
inline int64_t batch_sample_rows(int64_t rows, int32_t k, bool whole_blocks = false, int div = 32) {
  if (whole_blocks) {  // a norm-grouped plane: whole blocks of BATCH_BLOCK_ROWS positions (an unbiased sample of the norms)
    const int64_t n = round_up(batch_sample_rows(rows, k, false, div), BATCH_BLOCK_ROWS);
    return n >= rows ? rows : n;
  }
  if (rows <= 16384) return rows;
  int64_t n = std::max<int64_t>(rows / div, (int64_t)k * rows / (3000 * div / 32));
  n = std::max<int64_t>(round_up(n, 256), 8192);  // whole row tiles of either tile shape
  n = std::max<int64_t>(n, round_up((int64_t)k * 4, 256));
  return std::min(n, rows);
}

// Where the sample sits.  The first n_sample rows serve any mask that keeps rows everywhere; a WHERE clause that
// keeps one id RANGE leaves them without a single kept row -- no threshold, every kept row a survivor, every list
// overflowing, every query redone by a scan of its own (1 M x 768, a 10 % range, 64-query calls: 5.5 k queries/s where
// Bernoulli masks reach 120 k).  With a mask the window of n_sample consecutive rows (whole 256-row tiles; whole blocks
// of a norm-grouped plane) that keeps the most rows is taken instead -- candidates every half window -- and the first
// one on a tie.  The bound needs nothing of the sample but k kept rows inside it; an estimate it makes unrepresentative
// is caught by B2 as ever.  pre[t] = kept rows in the mask's 64-row words [0, t), n_tiles_all + 1 entries.
struct SampleWindow {
  int64_t s0 = 0;     // first row of the window
  int64_t best = -1;  // rows it keeps
};
inline SampleWindow sample_window(const int32_t *pre, int32_t n_tiles_all, int64_t rows, int64_t n_sample, bool want_group) {
  const int64_t wa = want_group ? BATCH_BLOCK_ROWS / 64 : 4;  // in 64-row mask words
  const int64_t wt = n_sample / 64, step = std::max<int64_t>(wa, wt / 2 / wa * wa);
  SampleWindow w;
  for (int64_t w0 = 0; w0 * 64 + n_sample <= rows; w0 += step) {
    const int64_t kept = pre[(size_t)std::min<int64_t>(w0 + wt, n_tiles_all)] - pre[(size_t)w0];
    if (kept > w.best) {
      w.best = kept;
      w.s0 = w0 * 64;
    }
  }
  return w;
}

// ---- the key kernel -------------------------------------------------------------------------------------------------
// The automatic choice (batch_kernel 3): fp16 keys?  Cosine keys are scale-free (unit rows, unit query), so fp16's fixed
// relative precision gives a band that is narrow against ANY data.  L2 / inner product: with a band PER ROW
// (alpha |v| + beta, batch_delta2) a row's own norm no longer widens its neighbours' bands, so the choice asks what is
// left -- the SHARED term.  Inner product: beta is a few u |q| max|v|, nothing against the spacing of the keys that
// matter (the longest rows'): fp16 whatever the norms.  L2: beta ~ c (|q|^2 + max|v|^2) has to stay small against the
// spacing of the SHORT rows' keys, ~0.1 |q| min|v| near a query's k-th neighbour: fp16 while
// c (1 + max|v|^2) <= 0.02 min|v| (|q| ~ 1 assumed; norms U(0.1, 3.2), a factor 32 apart: 4.8e-5 against 2e-3 -- 482 k
// queries/s where bf16x3 gives 199 k; norms 2^-6 .. 2^6: 1.2e-2 against 3e-4 -- every short row would be a candidate:
// bf16x3, whose error is 25 x tighter).  denied: a shard whose fp16 lists kept overflowing all the same is served
// bf16x3 keys for a while -- F16_DENIAL_CALLS batched calls -- and then tried again (the corpus, or the calls' masks, may
// have changed).
inline bool f16_keys_fit(const BatchShardFacts &sh, bool denied) {
  if (sh.metric == TSH_METRIC_COSINE) return true;
  if (denied) return false;
  if (sh.metric != TSH_METRIC_L2) return true;
  const double c_acc = (double)((sh.dim + 63) / 64 + 12) * 1.1920928955078125e-07;
  return sh.min_norm > 0.f && c_acc * (1.0 + (double)sh.max_norm * (double)sh.max_norm) <= 0.02 * (double)sh.min_norm;
}

// fp16 operands are scaled by 2^exp so that the largest magnitude `top` lands in [2^13, 2^14).  false: a scale near the
// edge of f32's exponent range -- no fp16 keys (*exp is set all the same)
inline bool f16_scale_exp(float top, int *exp) {
  int e = 0;
  if (top > 0.f) std::frexp(top, &e);  // top = m * 2^e, m in [0.5, 1)
  *exp = 14 - e;
  return *exp <= 55 && *exp >= -55;
}
// ... the largest magnitude of the rows' plane: cosine planes hold unit rows
inline float f16_rows_top(const BatchShardFacts &sh) { return sh.metric == TSH_METRIC_COSINE ? 1.0f : sh.max_abs; }

// LISTED mode (round 6): a mask that keeps at most LISTED_MAX rows, a small part of the shard.  Scoring all rows and
// dropping all but a percent in the epilogue is the wrong way round: the kept rows' fp16 copy is GATHERED (their ids are
// the mask as a list -- a handle's resident one, or the call's), and the dense pass scores just them: the "sample" is
// every row there is, its threshold proven (k_est = k), and no filtered pass follows.  1 M x 768, keep 1 %: a
// 64-query call 0.55 -> 0.2 ms, a 1024-query call 1.8 -> 0.3 ms.  fp16 keys only (the kernel that maps plane positions
// to row ids); everything behind the candidate lists sees row ids, as ever.
constexpr int64_t LISTED_MAX = 16384, LISTED_PART = 24;
inline bool listed_mode(int64_t kept, int64_t rows) { return kept >= 1 && kept <= LISTED_MAX && kept * LISTED_PART <= rows; }

// ---- the plan of one call -------------------------------------------------------------------------------------------
struct BatchPlan {
  int want_kernel = 3;  // the option the call goes by (3: automatic)
  // Workgroup tile (queries x rows).  f32 MFMA: 128 x 128.  bf16x3: 256 x 256 for batches of more than 128 queries,
  // 128 x 128 otherwise.  f16: 256 x 256 resp. 128 x 256.  The padding of the batch depends on the query side only.
  int32_t tile = 128, nq_pad = 0;
  bool want_group = false;  // the fp16 plane of this shard would be norm-grouped: sample windows of whole blocks
  bool listed = false;
  int kern = 0;   // the key kernel that runs: 0 f32 MFMA, 1 bf16x3, 2 f16
  int v_exp = 0;  // f16: rows are scaled by 2^v_exp
  // K-chunks of 32 for both plane formats; the f16 kernel walks its ring of four stages in whole turns, so its
  // planes are zero-padded to a multiple of four chunks
  int32_t hchunks = 0;
  int32_t tile_n = 128;  // rows per workgroup tile: the f16 kernel's is 256 x 256 / 128 x 256, the others' square
  int64_t n_sample = 0;  // rows of the dense pass
  int64_t scan_rows = 0;  // rows the key passes score
  int32_t k_est = 0;      // (a windowed sample: taken again from the kept rows, batch_k_est)
  int32_t cand_cap = 0;   // candidates per query the key passes may append
  // The hub rows' bound (Shard::d_hub) is still a candidate: fp16 keys of an L2 / inner-product shard whose norms
  // differ at all, no caller mask (the bound counts rows the mask may drop), big enough that sixteen more tiles are
  // noise.  TSH_OPT_BATCH_HUB.  (Either cure for crowded rows, not both: not with a norm-grouped plane.)
  bool hub = false;
};

inline BatchPlan plan_batch(const BatchShardFacts &sh, const BatchCallFacts &c) {
  BatchPlan p;
  p.want_kernel = c.force_kernel >= 0 ? c.force_kernel : sh.batch_kernel;
  p.tile = (c.forced_tile == 128 || c.forced_tile == 256) && p.want_kernel != 0
               ? c.forced_tile
               : ((p.want_kernel != 0 && c.nq > 128) ? 256 : 128);  // (the f32 kernel has the 128 tile only)
  p.nq_pad = (int32_t)round_up(c.nq, p.tile);
  // (decided from what is known before the key kernel is -- a superset; whole blocks suit every kernel)
  p.want_group = sh.batch_group && sh.metric != TSH_METRIC_COSINE && p.want_kernel >= 2;
  const bool f16_auto = p.want_kernel == 3 && f16_keys_fit(sh, c.f16_denied);
  p.kern = p.want_kernel == 3 ? (f16_auto ? 2 : 1) : p.want_kernel;
  if (p.kern == 2 && !f16_scale_exp(f16_rows_top(sh), &p.v_exp)) p.kern = 1;  // bf16x3 instead
  p.listed = p.kern == 2 && listed_mode(c.kept, sh.rows) && !c.sample_force &&
             (c.mask != BatchMask::HANDLE || c.handle_list);
  p.hchunks = p.kern == 2 ? (int32_t)round_up((sh.dim + 31) / 32, 4) : (int32_t)((sh.dim + 31) / 32);
  p.tile_n = p.kern == 2 ? 256 : p.tile;
  p.scan_rows = p.listed ? c.kept : sh.rows;
  p.n_sample = p.listed ? c.kept : (c.sample_force ? sh.rows : batch_sample_rows(sh.rows, c.k, p.want_group, c.sample_div));
  const int64_t ratio = p.scan_rows / std::max<int64_t>(p.n_sample, 1) + 1;
  p.k_est = batch_k_est(c.k, p.scan_rows, p.n_sample, c.est_backoff, c.proven_tau);
  p.cand_cap = (int32_t)std::min<int64_t>(65536, std::max<int64_t>(4096, round_up(4 * (int64_t)c.k * ratio, 64)));
  p.hub = sh.batch_hub && c.mask == BatchMask::NONE && !p.listed && !c.sample_force && sh.metric != TSH_METRIC_COSINE &&
          sh.rows >= 16 * HUB_ROWS && sh.max_norm > 1.02f * sh.min_norm && c.k <= HUB_ROWS / 4 && p.kern == 2;
  return p;
}

// ---- the tail's chunks ----------------------------------------------------------------------------------------------
// The tail (final select, re-rank) runs in chunks of queries: while the GPU re-ranks chunk c + 1, the host already
// finalises chunk c.  One chunk when nobody finalises chunk by chunk (256 queries: 1.00 -> 0.94 ms; 128: no gain).
inline int batch_n_chunks(int32_t nq, bool one_chunk) { return one_chunk ? 1 : (nq >= 512 ? 4 : (nq >= 256 ? 2 : 1)); }
// chunk c = queries [chunk_q(c), chunk_q(c + 1)): the last chunk is the small one -- its finalisation is all that is
// left to do on the host once the GPU is done
inline int32_t chunk_q(int n_chunks, int32_t nq, int c) {
  static const int cut4[5] = {0, 31, 62, 87, 100}, cut2[3] = {0, 60, 100};
  if (c <= 0) return 0;
  if (c >= n_chunks) return nq;
  const int pct = n_chunks == 4 ? cut4[c] : (n_chunks == 2 ? cut2[c] : 100 * c / n_chunks);
  return (int32_t)((int64_t)nq * pct / 100);
}

// ---- the queries ----------------------------------------------------------------------------------------------------
// Sum of squares (f64, element order, one rounding per addition: == query_mag_a) and largest magnitude of up to
// QN_GROUP queries at once: a query's sum is one serial chain of additions, so a lone query waits out the add latency
// dim times; eight chains side by side keep the adder busy (1024 x 768: 85-100 -> 60-85 us of a call's preparation).
// ok[j] = every element of query j is within the error model (finite, |x| <= BIG_ABS).
constexpr int QN_GROUP = 8;
inline void query_norms(const float *q0, int64_t stride, int dim, int n, double *qn2, float *qmax, char *ok) {
  double acc[QN_GROUP] = {0, 0, 0, 0, 0, 0, 0, 0};
  float mx[QN_GROUP] = {0, 0, 0, 0, 0, 0, 0, 0};
  const float *p[QN_GROUP];
  for (int j = 0; j < QN_GROUP; ++j) p[j] = q0 + (int64_t)(j < n ? j : 0) * stride;
  for (int i = 0; i < dim; ++i)
    for (int j = 0; j < QN_GROUP; ++j) {
      const float v = p[j][i], a = std::fabs(v);
      mx[j] = a > mx[j] ? a : mx[j];  // (a NaN never becomes the maximum: caught below through the sum)
      acc[j] = acc[j] + (double)v * (double)v;
    }
  for (int j = 0; j < n; ++j) {
    qn2[j] = acc[j];
    qmax[j] = mx[j];
    ok[j] = mx[j] <= BIG_ABS && acc[j] == acc[j] && acc[j] < INFINITY;  // NaN / inf elements poison the sum
  }
}

// The per-query side inputs of the key and select kernels: six planes of nq_pad floats each, in one buffer on the host
// (BatchCtx::qaux.h) and one on the device.  [qsq | delta2] and [kmax | alpha] are uploaded as pairs; thr and tau_est
// are the device's own.
struct QAux {
  float *base;
  size_t nq_pad;
  static constexpr int PLANES = 6;
  float *qsq() const { return base; }                    // |q|^2
  float *delta2() const { return base + nq_pad; }        // the band every key of the query shares, doubled
  float *thr() const { return base + 2 * nq_pad; }       // the filter threshold (B0s)
  uint32_t *tau_est() const { return reinterpret_cast<uint32_t *>(base + 3 * nq_pad); }  // the estimate it came from
  float *kmax() const { return base + 4 * nq_pad; }      // the largest key a row can have
  float *alpha() const { return base + 5 * nq_pad; }     // per-row part of the band (fp16 keys, L2 / inner product; else 0)
};

inline double hld_f16(const BatchShardFacts &sh) { return (double)round_up(sh.dim, 64); }  // padded reduction length of the fp16 planes

// The error band of a batched key, per query.  qn2: query_norms.
//   out_delta2   2 * (the part of the bound every key of the query shares), absolute, rounded up
//   out_alpha    fp16 keys of an L2 / inner-product index (round 5): the bound of the key of row v is
//                alpha |v| + delta2 / 2 + chain |thr'| -- the operand roundings act on the products, 2^-10 |q| |v| a row, so
//                a short row's key is known that much better than a long one's; 0 where every key has the same band
//   (chain: batch_chain2(), per call; thr': the threshold the filtered pass starts its accumulators from)
inline bool batch_delta2(const BatchShardFacts &s, int kernel, double qn2, float *out_delta2, float *out_qsq, float *out_alpha = nullptr) {
  const double qn = std::sqrt(qn2) * (1.0 + 1e-6), vmax = (double)s.max_norm * (1.0 + 1e-6);
  const double u2 = 1.1920928955078125e-07;        // 2^-23
  double gam = ((double)s.ld + 8.0) * u2;   // k-ordered fma chain of ld terms
  if (kernel == 1) {
    // three partial products per k accumulate in f32 (chain of 3 ld terms, each product exact),
    // and hi + lo drops up to 2^-15 |q_i||v_i| per element (tsh_batch.hip.h, bf16x3 variant; 8.001: its 1 + 2^-19).  (It was
    // 3.1 * 2^-18 -- a bf16 rounding taken as 2^-9 where it is 2^-8: rows of one chunk, where the chain's term is as small,
    // came out 1.04 bounds from their exact keys, tests/test_gpu_batch_shapes.py at d = 1.)
    const double hld = (double)round_up(s.dim, 32);
    gam = (3.0 * hld + 8.0) * u2 * (1.0 + 0.00391) + 8.001 * 3.814697265625e-06;
  } else if (kernel == 2) {
    // both operands rounded to fp16 (2^-11 each, + their product), exact products accumulated in f32;
    // 2^-21: the f32 scaling / normalisation before the rounding; 2^-30: fp16 subnormal steps, which
    // sit >= 27 binades under the largest operand value after the power-of-two scaling
    const double hld = (double)round_up(s.dim, 64);
    // (a query is only batched when its largest element is within 2^8 of the batch's, see batch_prepare_queries)
    // The filtered cosine pass starts its accumulators at -theta (|theta| <= |q| (1 + 1e-2), capped by
    // BatchArgs::kmax) instead of zero: the chain carries twice the magnitude, and the key is formed from the
    // accumulator by one more subtraction and one multiplication by a power of two (tsh_batch_f16pp.hip.h)
    gam = 2.0 * (hld + 10.0) * u2 * (1.0 + 0.01) + 9.765625e-04 * (1.0 + 0.001) + 4.76837158203125e-07 +
          std::sqrt(hld) * 9.3e-10;
  }
  double delta, alpha = 0.0;
  if (kernel == 2 && s.metric != TSH_METRIC_COSINE) {
    // fp16 keys, L2 / inner product: per-row bands (round 5).  In key units the accumulator of (q, v) runs through
    //   L2:  thr' - |q|^2 - |v|^2 + alpha |v|  (its start)  ... + 2 q.v      inner product:  -thr' + alpha |v| ... + q.v
    // so its hld + 12 roundings (the chain's, the start value's fma, the key's subtraction) cost at most
    //   c P,  c = (hld + 12) u,  P = |thr'| + |q|^2 + |v|^2 + alpha |v| + 2 |q| |v| (1 + 2^-10)      (L2)
    //                            P = |thr'| + alpha |v| + |q| |v| (1 + 2^-10)                        (inner product)
    // and the operand roundings act on the products only: 2 e_op |q| |v| (L2), e_op |q| |v| (inner product).  Sorted
    // by what they multiply:  alpha |v|  (alpha appears on both sides: solved for)  +  c |thr'|  (known on the device
    // only: batch_chain2)  +  the rest, the same for every row of the query.  Roundings of |q|^2, |v|^2 (f32 from f64
    // sums), of the seed and of the select kernels' key +- width arithmetic: 14 u A + 8 u kmax.
    const double hld = hld_f16(s), c = (hld + 12.0) * u2;
    const double e_op = 9.765625e-04 * (1.0 + 0.001) + 4.76837158203125e-07 + std::sqrt(hld) * 9.3e-10;
    const double pq = qn * (1.0 + 9.765625e-04);
    // (the fp16 subnormal steps are ABSOLUTE -- 2^-30 of the largest operand value, whatever the row's own norm: a short
    // row's small elements sit in them -- so that part of e_op goes with max|v| into the shared term)
    const double sub = std::sqrt(hld) * 9.3e-10 * qn * vmax;
    if (s.metric == TSH_METRIC_L2) {
      const double A = qn * qn + vmax * vmax, kmax = 1.01 * (qn + vmax) * (qn + vmax);
      alpha = (2.0 * e_op * qn + 2.0 * c * pq) / (1.0 - c);
      delta = c * A + 14.0 * u2 * A + 8.0 * u2 * kmax + 2.0 * sub;
    } else {
      const double kmax = 1.01 * qn * vmax;
      alpha = (e_op * qn + c * pq) / (1.0 - c);
      delta = 6.0 * u2 * qn * vmax + 8.0 * u2 * kmax + sub;
    }
    alpha *= 1.0 + 1e-6;
  } else if (s.metric == TSH_METRIC_IP) delta = gam * qn * vmax;
  else if (s.metric == TSH_METRIC_COSINE) delta = qn * (gam + 4.76837158203125e-07) * (kernel == 2 ? 1.0 + 1e-6 : 1.0);
  else delta = 2.0 * gam * qn * vmax + 6.0 * u2 * (qn * qn + vmax * vmax);
  delta += (double)s.dim * 7.5e-37;
  double d2 = 2.0 * delta * 1.0001;
  if (!(d2 < 1e30) || !(alpha < 1e30)) return false;
  *out_delta2 = (float)d2;
  if ((double)*out_delta2 < d2) *out_delta2 = std::nextafter(*out_delta2, INFINITY);
  *out_qsq = (float)qn2;
  if (out_alpha) {
    *out_alpha = (float)alpha;
    if ((double)*out_alpha < alpha) *out_alpha = std::nextafter(*out_alpha, INFINITY);
  }
  return true;
}
// fp16 keys of an L2 / inner-product index: c of batch_delta2 as the select kernels take it -- 2 c / (1 - 2 c), rounded
// up (the filter threshold thr' must still cover the k-th key once the band has grown by c |thr'| on either side); 0
// for every other key kernel / metric
inline float batch_chain2(const BatchShardFacts &s, int kernel) {
  if (kernel != 2 || s.metric == TSH_METRIC_COSINE) return 0.f;
  const double c = (hld_f16(s) + 12.0) * 1.1920928955078125e-07;
  const double v = 2.0 * c / (1.0 - 2.0 * c) * (1.0 + 1e-6);
  float f = (float)v;
  if ((double)f < v) f = std::nextafter(f, INFINITY);
  return f;
}

// ---- batched or one by one? -----------------------------------------------------------------------------------------
// does a call of nq queries on this shard go to the matrix cores?  kept: rows a mask of the call keeps (-1: none / unknown)
inline bool shard_takes_batch(const BatchShardFacts &s, int32_t batch_min_nq, int32_t nq, int32_t k, int64_t kept = -1) {
  // batch_min_nq == 1: decide by cost.  Measured: a batched call costs about 0.30 ms plus one
  // pass over the converted rows at ~4 TB/s, whatever nq <= 128 is; pipelined single-query scans cost one
  // pass over the f32 rows at ~6.6 TB/s plus ~25 us each.  At 1 M x 768 that is 0.67 vs 1.04 ms for TWO queries.
  // With a mask (round 6) both sides change: a query of its own reads the kept rows only -- from their exact sums in two
  // dispatches when there are at most exact_rows of them (16.7 us per query at 10 k kept rows of 768 floats, pipelined),
  // by a masked scan otherwise (57-65 us at 100 k) --, and a batched call behind a selective mask scores a gathered
  // copy of the kept rows (listed_mode: ~0.2 ms whatever nq <= 128 is).  Eight queries behind a 1 % mask of 1 M rows:
  // 0.13 ms one by one, 0.2 ms batched (0.55 before the listed mode) -- the model used to send every masked call of two
  // queries or more to the matrix cores.
  bool enough = batch_min_nq > 1 && nq >= batch_min_nq;
  if (batch_min_nq == 1 && nq >= 2) {
    const int kern = s.batch_kernel == 3 ? 2 : s.batch_kernel;
    const double plane_b = kern == 0 ? 4.0 : (kern == 1 ? 4.0 : 2.0);
    double t_batch = 300.0 + (double)s.rows * (double)s.dim * plane_b / 4.0e6 * ((nq + 127) / 128);
    double t_single = (double)nq * ((double)s.rows * (double)s.ld * 4.0 / 6.6e6 + 25.0);
    if (kept >= 0 && kept < s.rows) {
      const double kept_bytes = (double)std::max<int64_t>(kept, 1) * (double)s.ld * 4.0;
      if (kept <= std::min<int64_t>(s.exact_rows, BATCH_EXACT_MAX)) t_single = (double)nq * (8.0 + kept_bytes / 3.5e6);
      else t_single = (double)nq * (25.0 + kept_bytes / 5.5e6);
      if (kern >= 2 && listed_mode(kept, s.rows))
        t_batch = 180.0 + (double)kept * (double)s.dim * 2.0 / 4.0e6 * ((nq + 127) / 128) + 0.3 * (double)nq;
    }
    enough = t_single > t_batch;
  }
  return enough && !s.safe_mode && s.rows >= 4096 && k <= 1024 && s.rows < 0x7FFFFF00ll;
}

}  // namespace tsh
