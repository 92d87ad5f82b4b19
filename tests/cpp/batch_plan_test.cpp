// Host-only check of tostore_amd/csrc/tsh_batch_plan.h: the decisions of a batched (matrix-core) call.  Expectations are
// DESIGN.md's stated figures and brute-force restatements written here (a long-double binomial tail, a window search over
// the mask's bits, serial f64 sums, the simplest error-band formulas), never the header's own results.
// Prints "batch plan ok"; exit status 1 on a miss.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <random>
#include <vector>

#include "../../tostore_amd/csrc/tsh_batch_plan.h"

using namespace tsh;

static int fails = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      printf("MISS %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);        \
      printf("\n");               \
      ++fails;                    \
    }                             \
  } while (0)

static BatchShardFacts shard(int64_t rows, int dim, int metric, float min_norm = 1.f, float max_norm = 1.f, float max_abs = 0.25f) {
  BatchShardFacts s;
  s.rows = rows;
  s.cap = rows;
  s.dim = dim;
  s.ld = (dim + 3) / 4 * 4;
  s.metric = metric;
  s.min_norm = min_norm;
  s.max_norm = max_norm;
  s.max_abs = max_abs;
  return s;
}
static BatchCallFacts call(int32_t nq, int32_t k) {
  BatchCallFacts c;
  c.nq = nq;
  c.k = k;
  c.entries = 512;
  return c;
}
static BatchCallFacts masked(int32_t nq, int32_t k, BatchMask m, int64_t kept, bool handle_list = false) {
  BatchCallFacts c = call(nq, k);
  c.mask = m;
  c.kept = kept;
  c.handle_list = handle_list;
  return c;
}

// ---- batch_sample_rows ----------------------------------------------------------------------------------------------
static void test_sample_rows() {
  CHECK(batch_sample_rows(16384, 10) == 16384 && batch_sample_rows(100, 10) == 100 && batch_sample_rows(16384, 10, true) == 16384,
        "rows <= 16384: all rows");
  CHECK(batch_sample_rows(16385, 10) == 8192, "16385 rows: %lld", (long long)batch_sample_rows(16385, 10));
  CHECK(batch_sample_rows(16385, 10, true) == 8192, "16385 rows, whole blocks");
  // DESIGN.md section 6's two figures
  CHECK(batch_sample_rows(1000000, 10) == 31488, "1 M rows, k = 10: %lld", (long long)batch_sample_rows(1000000, 10));
  CHECK(batch_sample_rows(1000000, 10, true) == 32768, "1 M rows, k = 10, whole blocks: %lld", (long long)batch_sample_rows(1000000, 10, true));
  for (int64_t rows : {4096ll, 16385ll, 20000ll, 40000ll, 100000ll, 262144ll, 1000000ll, 10000001ll})
    for (int32_t k : {1, 10, 100, 1024})
      for (int blocks = 0; blocks < 2; ++blocks) {
        const int64_t n = batch_sample_rows(rows, k, blocks != 0);
        const int64_t unit = blocks ? 8192 : 256;
        CHECK(n == rows || n % unit == 0, "rows %lld k %d blocks %d: %lld is no multiple of %lld", (long long)rows, k, blocks, (long long)n, (long long)unit);
        CHECK(n <= rows && n >= 1, "rows %lld k %d: %lld out of range", (long long)rows, k, (long long)n);
        CHECK(n == rows || n >= (4ll * k + 255) / 256 * 256, "rows %lld k %d: %lld below 4 k", (long long)rows, k, (long long)n);
      }
}

// ---- batch_k_est ----------------------------------------------------------------------------------------------------
// P(Binomial(k, p) >= m), directly: the mass function by its recurrence, summed from the top
static long double binom_tail(int k, long double p, int m) {
  std::vector<long double> pmf((size_t)k + 1);
  pmf[0] = std::pow(1.0L - p, (long double)k);
  for (int i = 0; i < k; ++i) pmf[(size_t)i + 1] = pmf[(size_t)i] * (long double)(k - i) / (long double)(i + 1) * p / (1.0L - p);
  long double t = 0;
  for (int i = k; i >= m; --i) t += pmf[(size_t)i];
  return t;
}
static void test_k_est() {
  const int64_t rows = 1 << 20;
  for (int k : {1, 8, 9, 10, 100, 1024}) {
    for (int64_t n_sample : {rows / 32, rows / 4, rows / 2, rows / 2 + 1, rows}) {
      int expect = k;
      if (k > 8 && 2 * n_sample <= rows) {
        const long double p = (long double)n_sample / (long double)rows;
        int m = 1;
        while (m <= k && binom_tail(k, p, m) > 1e-6L) ++m;  // the smallest m with a tail <= 1e-6 (k + 1: none -- an empty tail)
        expect = std::min(k, std::max(m, 4));
      }
      const int got = batch_k_est(k, rows, n_sample);
      CHECK(got == expect, "k_est(k %d, sample %lld of %lld) = %d, expected %d", k, (long long)n_sample, (long long)rows, got, expect);
      CHECK(batch_k_est(k, rows, n_sample, 3) == k, "k_est during a back-off");
      CHECK(batch_k_est(k, rows, n_sample, 0, true) == k, "k_est with the estimate switched off");
    }
  }
  CHECK(batch_k_est(100, rows, rows / 32) < 100 && batch_k_est(100, rows, rows / 32) >= 4, "k = 100 at 1 / 32: an estimate");
}

// ---- the key kernel -------------------------------------------------------------------------------------------------
static void test_kernel_choice() {
  const int64_t rows = 1000000;
  const int d = 768;
  auto kern = [&](const BatchShardFacts &s, const BatchCallFacts &c) { return plan_batch(s, c).kern; };
  // cosine and inner product: fp16 whatever the norms
  for (float lo : {0.f, 0.015625f, 0.1f, 1.f})
    for (float hi : {1.f, 3.2f, 64.f}) {
      CHECK(kern(shard(rows, d, TSH_METRIC_COSINE, lo, hi), call(64, 10)) == 2, "cosine, norms %g .. %g", lo, hi);
      CHECK(kern(shard(rows, d, TSH_METRIC_IP, lo, hi), call(64, 10)) == 2, "inner product, norms %g .. %g", lo, hi);
    }
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 0.1f, 3.2f), call(64, 10)) == 2, "L2, norms 0.1 .. 3.2: fp16");
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 0.015625f, 64.f), call(64, 10)) == 1, "L2, norms 2^-6 .. 2^6: bf16x3");
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 0.f, 1.f), call(64, 10)) == 1, "L2, min_norm = 0: bf16x3");
  // the rule itself, c (1 + max^2) <= 0.02 min with c = (768 / 64 + 12) 2^-23 = 2.861e-6: at min = 1 the largest norm
  // may reach sqrt(0.02 / c - 1) = 83.6
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 1.f, 83.f), call(64, 10)) == 2, "L2, norms 1 .. 83: fp16");
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 1.f, 84.f), call(64, 10)) == 1, "L2, norms 1 .. 84: bf16x3");
  CHECK(f16_keys_fit(shard(rows, d, TSH_METRIC_L2, 1.f, 83.f), false) && !f16_keys_fit(shard(rows, d, TSH_METRIC_L2, 1.f, 84.f), false),
        "f16_keys_fit at the edge");
  // denied
  BatchCallFacts den = call(64, 10);
  den.f16_denied = true;
  CHECK(kern(shard(rows, d, TSH_METRIC_IP, 0.5f, 2.f), den) == 1, "inner product, denied: bf16x3");
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 0.5f, 2.f), den) == 1, "L2, denied: bf16x3");
  CHECK(kern(shard(rows, d, TSH_METRIC_L2, 0.5f, 2.f), call(64, 10)) == 2, "L2, norms 0.5 .. 2, not denied: fp16");
  // an explicit kernel is obeyed, and force_kernel wins
  for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP, TSH_METRIC_COSINE})
    for (int want : {0, 1, 2}) {
      BatchShardFacts s = shard(rows, d, metric, 0.015625f, 64.f);
      s.batch_kernel = want;
      CHECK(kern(s, call(64, 10)) == want, "explicit kernel %d, metric %d", want, metric);
      CHECK(kern(s, den) == want, "explicit kernel %d is not the automatic choice's to deny", want);
      BatchCallFacts f = call(64, 10);
      f.force_kernel = 0;
      CHECK(kern(s, f) == 0 && plan_batch(s, f).tile == 128, "force_kernel = 0 over option %d", want);
    }
  // the scale: 14 - e = +-55 stays fp16, +-56 does not (and is not listed).  max_abs = 1.5 * 2^(e - 1) has exponent e
  for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP})
    for (int option : {2, 3})
      for (int v_exp : {55, -55, 56, -56, 14, 0}) {
        BatchShardFacts s = shard(rows, d, metric, 1.f, 1.f, std::ldexp(1.5f, 14 - v_exp - 1));
        s.batch_kernel = option;
        const bool in = v_exp <= 55 && v_exp >= -55;
        const BatchPlan p = plan_batch(s, call(64, 10));
        CHECK(p.kern == (in ? 2 : 1), "metric %d option %d scale 2^%d: kernel %d", metric, option, v_exp, p.kern);
        CHECK(!in || p.v_exp == v_exp, "scale exponent %d, expected %d", p.v_exp, v_exp);
        const BatchPlan pl = plan_batch(s, masked(64, 10, BatchMask::POINTER, 1000));
        CHECK(pl.listed == in && pl.kern == (in ? 2 : 1), "metric %d option %d scale 2^%d behind a 0.1 %% mask: listed %d", metric, option, v_exp, (int)pl.listed);
      }
  int e = 0;
  CHECK(f16_scale_exp(1.0f, &e) && e == 13, "1.0 = 0.5 * 2^1 -> 2^13");
  CHECK(f16_scale_exp(0.f, &e) && e == 14, "no magnitude at all");
  // a cosine plane holds unit rows: max_abs does not matter
  BatchShardFacts cs = shard(rows, d, TSH_METRIC_COSINE, 1.f, 1.f, 1e-30f);
  CHECK(plan_batch(cs, call(64, 10)).kern == 2 && plan_batch(cs, call(64, 10)).v_exp == 13, "cosine: the scale of unit rows");
  // tiles and chunks of the plan
  BatchShardFacts s = shard(rows, d, TSH_METRIC_COSINE);
  CHECK(plan_batch(s, call(128, 10)).tile == 128 && plan_batch(s, call(129, 10)).tile == 256, "the query tile");
  CHECK(plan_batch(s, call(129, 10)).nq_pad == 256 && plan_batch(s, call(9, 10)).nq_pad == 128 && plan_batch(s, call(1024, 10)).nq_pad == 1024, "padding");
  CHECK(plan_batch(s, call(64, 10)).hchunks == 24 && plan_batch(s, call(64, 10)).tile_n == 256, "fp16: 768 / 32 = 24 chunks, 256-row tiles");
  CHECK(plan_batch(shard(rows, 100, TSH_METRIC_COSINE), call(64, 10)).hchunks == 4, "fp16 planes: whole turns of four chunks");
  s.batch_kernel = 1;
  CHECK(plan_batch(shard(rows, 100, TSH_METRIC_COSINE), call(64, 10)).hchunks == 4 && plan_batch(s, call(200, 10)).tile_n == 256 &&
            plan_batch(s, call(64, 10)).tile_n == 128 && plan_batch(s, call(64, 10)).hchunks == 24,
        "bf16x3: square tiles");
  BatchShardFacts b100 = shard(rows, 100, TSH_METRIC_COSINE);
  b100.batch_kernel = 1;
  CHECK(plan_batch(b100, call(64, 10)).hchunks == 4, "bf16x3 planes: ceil(100 / 32) chunks");
  b100.dim = 130;
  CHECK(plan_batch(b100, call(64, 10)).hchunks == 5, "bf16x3 planes: ceil(130 / 32) chunks");
  b100.batch_kernel = 2;
  CHECK(plan_batch(b100, call(64, 10)).hchunks == 8, "fp16 planes: 5 chunks padded to 8");
  // norm-grouped windows: fp16 or automatic, L2 / inner product, option on
  CHECK(plan_batch(shard(rows, d, TSH_METRIC_L2), call(64, 10)).want_group && !plan_batch(shard(rows, d, TSH_METRIC_COSINE), call(64, 10)).want_group,
        "want_group by metric");
  BatchShardFacts ng = shard(rows, d, TSH_METRIC_L2);
  ng.batch_group = false;
  CHECK(!plan_batch(ng, call(64, 10)).want_group && plan_batch(ng, call(64, 10)).n_sample == 31488, "grouping off: the row-order sample");
  CHECK(plan_batch(shard(rows, d, TSH_METRIC_L2), call(64, 10)).n_sample == 32768, "grouping on: whole blocks");
}

// ---- listed mode ----------------------------------------------------------------------------------------------------
static void test_listed() {
  for (int64_t kept : {0ll, 1ll, 16384ll, 16385ll})
    for (int edge = 0; edge < 2; ++edge) {
      const int64_t rows = kept == 0 ? 100000 + edge : 24 * kept - 1 + edge;
      const bool expect = kept >= 1 && kept <= 16384 && edge == 1;
      CHECK(listed_mode(kept, rows) == expect, "listed_mode(%lld, %lld)", (long long)kept, (long long)rows);
      for (BatchMask m : {BatchMask::POINTER, BatchMask::HANDLE}) {
        const BatchShardFacts s = shard(rows, 768, TSH_METRIC_COSINE);
        const BatchPlan p = plan_batch(s, masked(64, 10, m, kept, true));
        CHECK(p.listed == expect, "plan: kept %lld of %lld rows, listed %d", (long long)kept, (long long)rows, (int)p.listed);
        if (p.listed) CHECK(p.n_sample == kept && p.scan_rows == kept && p.k_est == 10 && p.kern == 2 && !p.hub, "a listed plan");
        else CHECK(p.scan_rows == rows, "an unlisted plan scores every row");
      }
    }
  const int64_t rows = 1000000, kept = 10000;
  for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP, TSH_METRIC_COSINE}) {
    BatchShardFacts s = shard(rows, 768, metric);
    CHECK(plan_batch(s, masked(1024, 100, BatchMask::POINTER, kept)).listed, "a 1 %% pointer mask is listed (metric %d)", metric);
    CHECK(plan_batch(s, masked(1024, 100, BatchMask::HANDLE, kept, true)).listed, "a 1 %% handle with a list is listed");
    CHECK(!plan_batch(s, masked(1024, 100, BatchMask::HANDLE, kept, false)).listed, "a handle without a list is not");
    BatchCallFacts f = masked(1024, 100, BatchMask::POINTER, kept);
    f.sample_force = true;
    CHECK(!plan_batch(s, f).listed && plan_batch(s, f).n_sample == rows, "sample_force: every row, not listed");
    for (int option : {0, 1}) {
      s.batch_kernel = option;
      CHECK(!plan_batch(s, masked(1024, 100, BatchMask::POINTER, kept)).listed, "kernel %d is never listed", option);
    }
    s.batch_kernel = 2;
    BatchCallFacts f0 = masked(1024, 100, BatchMask::POINTER, kept);
    f0.force_kernel = 0;
    CHECK(!plan_batch(s, f0).listed && plan_batch(s, f0).kern == 0, "force_kernel = 0 is never listed");
    // a listed plan's estimate is the proven one whatever k is
    CHECK(plan_batch(s, masked(1024, 100, BatchMask::POINTER, kept)).k_est == 100, "listed: k_est = k");
  }
  // the automatic choice, denied: no fp16 keys, so no list (cosine keys are never denied)
  BatchCallFacts den = masked(64, 10, BatchMask::POINTER, kept);
  den.f16_denied = true;
  CHECK(!plan_batch(shard(rows, 768, TSH_METRIC_IP), den).listed && plan_batch(shard(rows, 768, TSH_METRIC_COSINE), den).listed, "listed and the denial");
  CHECK(!plan_batch(shard(rows, 768, TSH_METRIC_L2, 0.015625f, 64.f), masked(64, 10, BatchMask::POINTER, kept)).listed, "L2, wide norms: bf16x3, no list");
}

// ---- sample_window --------------------------------------------------------------------------------------------------
static void window_case(const char *what, const std::vector<char> &keep, int64_t n_sample, bool grouped, int64_t expect_s0 = -1) {
  const int64_t rows = (int64_t)keep.size();
  const int32_t n_tiles = (int32_t)((rows + 63) / 64);
  std::vector<int32_t> pre((size_t)n_tiles + 1, 0);
  for (int64_t r = 0; r < rows; ++r) pre[(size_t)(r / 64) + 1] += keep[(size_t)r] ? 1 : 0;
  for (int32_t t = 0; t < n_tiles; ++t) pre[(size_t)t + 1] += pre[(size_t)t];
  // brute force over the same candidate starts: every half window, aligned down to 256 rows (whole blocks: 8192), at
  // least one alignment unit apart; counted bit by bit; the first on a tie
  const int64_t unit = grouped ? 8192 : 256;
  const int64_t step = std::max<int64_t>(unit, n_sample / 2 / unit * unit);
  int64_t best = -1, s0 = 0;
  for (int64_t st = 0; st + n_sample <= rows; st += step) {
    int64_t n = 0;
    for (int64_t r = st; r < st + n_sample; ++r) n += keep[(size_t)r] ? 1 : 0;
    if (n > best) best = n, s0 = st;
  }
  const SampleWindow w = sample_window(pre.data(), n_tiles, rows, n_sample, grouped);
  CHECK(w.s0 == s0 && w.best == best, "%s: window at %lld keeps %lld, brute force %lld keeps %lld", what, (long long)w.s0, (long long)w.best, (long long)s0, (long long)best);
  int64_t inside = 0;
  for (int64_t r = w.s0; r < w.s0 + n_sample && r < rows; ++r) inside += keep[(size_t)r] ? 1 : 0;
  CHECK(inside == w.best, "%s: best %lld, the window keeps %lld", what, (long long)w.best, (long long)inside);
  CHECK(w.s0 % unit == 0 && w.s0 + n_sample <= rows && w.s0 >= 0, "%s: window at %lld", what, (long long)w.s0);
  if (expect_s0 >= 0) CHECK(w.s0 == expect_s0, "%s: window at %lld, expected %lld", what, (long long)w.s0, (long long)expect_s0);
}
static void test_sample_window() {
  std::mt19937_64 rng(7);
  for (int64_t rows : {40000ll, 100000ll})
    for (int grouped = 0; grouped < 2; ++grouped)
      for (int64_t n_sample : {batch_sample_rows(rows, 10, grouped != 0), (int64_t)(grouped ? 16384 : 12288)}) {
        const int64_t unit = grouped ? 8192 : 256, step = std::max<int64_t>(unit, n_sample / 2 / unit * unit);
        auto range = [&](int64_t a, int64_t b) {
          std::vector<char> m((size_t)rows, 0);
          for (int64_t r = std::max<int64_t>(a, 0); r < std::min(b, rows); ++r) m[(size_t)r] = 1;
          return m;
        };
        window_case("a range at the start", range(0, 3000), n_sample, grouped != 0, 0);
        window_case("a range in the middle", range(rows / 2, rows / 2 + 3000), n_sample, grouped != 0);
        window_case("a range at the end", range(rows - 3000, rows), n_sample, grouped != 0);
        window_case("a range across two candidates", range(2 * step - 700, 2 * step + 1500), n_sample, grouped != 0);
        window_case("nothing kept", range(0, 0), n_sample, grouped != 0, 0);
        window_case("everything kept", range(0, rows), n_sample, grouped != 0, 0);
        std::vector<char> half((size_t)rows);
        for (char &x : half) x = (rng() & 1) != 0;
        window_case("Bernoulli 50 %", half, n_sample, grouped != 0);
        // two windows tied: the same 500 rows at the head of the candidates at `step` and at `3 step`
        if (3 * step + n_sample <= rows) {
          std::vector<char> tie = range(step, step + 500);
          for (int64_t r = 3 * step; r < 3 * step + 500; ++r) tie[(size_t)r] = 1;
          window_case("two windows tied", tie, n_sample, grouped != 0);
        }
      }
  // the tie, spelled out: 40 000 rows, a window of 8192 (candidates every 4096): ranges at 8192 and at 24576 are each
  // wholly inside the candidates at 4096 / 8192 resp. 20480 / 24576 -- four windows keep 500 rows, the one at 4096 is first
  std::vector<char> tie(40000, 0);
  for (int r = 8192; r < 8692; ++r) tie[(size_t)r] = 1;
  for (int r = 24576; r < 25076; ++r) tie[(size_t)r] = 1;
  window_case("tie, row order", tie, 8192, false, 4096);
  window_case("tie, whole blocks", tie, 8192, true, 8192);
}

// ---- the tail's chunks ----------------------------------------------------------------------------------------------
static void test_chunks() {
  const int nqs[5] = {255, 256, 511, 512, 1024}, expect_n[5] = {1, 2, 2, 4, 4};
  for (int i = 0; i < 5; ++i) {
    const int nq = nqs[i], n = batch_n_chunks(nq, false);
    CHECK(n == expect_n[i], "%d queries: %d chunks", nq, n);
    CHECK(batch_n_chunks(nq, true) == 1, "device-finalised: one chunk");
    for (int nc : {1, n}) {
      CHECK(chunk_q(nc, nq, 0) == 0 && chunk_q(nc, nq, nc) == nq && chunk_q(nc, nq, -1) == 0 && chunk_q(nc, nq, nc + 1) == nq, "the ends");
      for (int c = 0; c < nc; ++c) CHECK(chunk_q(nc, nq, c) < chunk_q(nc, nq, c + 1), "chunk %d of %d is empty or out of order", c, nc);
    }
    if (n == 4)
      CHECK(chunk_q(4, nq, 1) == nq * 31 / 100 && chunk_q(4, nq, 2) == nq * 62 / 100 && chunk_q(4, nq, 3) == nq * 87 / 100, "cuts at 31 / 62 / 87 %%");
    if (n == 2) CHECK(chunk_q(2, nq, 1) == nq * 60 / 100, "cut at 60 %%");
  }
  CHECK(chunk_q(4, 1024, 1) == 317 && chunk_q(4, 1024, 2) == 634 && chunk_q(4, 1024, 3) == 890 && chunk_q(2, 256, 1) == 153, "the cuts of 1024 and 256 queries");
}

// ---- cand_cap -------------------------------------------------------------------------------------------------------
static void test_cand_cap() {
  for (int64_t rows : {4096ll, 20000ll, 1000000ll, 100000000ll})
    for (int32_t k : {1, 10, 100, 1024})
      for (int masked_call = 0; masked_call < 2; ++masked_call) {
        const BatchPlan p = plan_batch(shard(rows, 768, TSH_METRIC_L2), masked_call ? masked(64, k, BatchMask::POINTER, std::max<int64_t>(rows / 100, 1)) : call(64, k));
        CHECK(p.cand_cap >= 4096 && p.cand_cap <= 65536 && p.cand_cap % 64 == 0, "rows %lld k %d: cand_cap %d", (long long)rows, k, p.cand_cap);
        CHECK(p.cand_cap >= std::min<int64_t>(65536, 4ll * k), "cand_cap %d below 4 k", p.cand_cap);
      }
}

// ---- batched or one by one ------------------------------------------------------------------------------------------
static void test_takes_batch() {
  const BatchShardFacts s = shard(1000000, 768, TSH_METRIC_COSINE);
  // DESIGN.md's three decisions at 1 M x 768
  CHECK(shard_takes_batch(s, 1, 2, 10), "two unmasked queries go to the matrix cores");
  CHECK(!shard_takes_batch(s, 1, 4, 10, 10000), "four queries behind a 1 %% mask go one by one");
  CHECK(shard_takes_batch(s, 1, 64, 10, 10000), "sixty-four behind the same mask go batched");
  // ... and between them the listed mode's price decides: sixteen exact scans of 10 k rows at 16.7 us are 0.27 ms, a
  // listed call about 0.2 ms -- an unlisted one (0.3 ms + a pass over the plane, 0.68 ms) would lose
  CHECK(shard_takes_batch(s, 1, 16, 10, 10000), "sixteen behind a 1 %% mask go batched, as a listed call");
  CHECK(!shard_takes_batch(s, 1, 8, 10, 50000), "eight behind a 5 %% mask (no list, no exact scan: 8 x 53 us against 0.68 ms) go one by one");
  CHECK(!shard_takes_batch(s, 1, 1, 10), "a lone query is never batched by cost");
  CHECK(shard_takes_batch(s, 8, 8, 10) && !shard_takes_batch(s, 8, 7, 10) && !shard_takes_batch(s, 0, 1024, 10), "an explicit minimum");
  BatchShardFacts g = s;
  g.safe_mode = true;
  CHECK(!shard_takes_batch(g, 1, 64, 10) && !shard_takes_batch(g, 8, 64, 10), "safe mode");
  g = s;
  g.rows = 4095;
  CHECK(!shard_takes_batch(g, 8, 64, 10), "rows < 4096");
  g.rows = 4096;
  CHECK(shard_takes_batch(g, 8, 64, 10), "rows = 4096");
  CHECK(!shard_takes_batch(s, 8, 64, 1025) && shard_takes_batch(s, 8, 64, 1024), "k > 1024");
}

// ---- the bands ------------------------------------------------------------------------------------------------------
static void test_bands() {
  const double u2 = std::ldexp(1.0, -23);
  // the f32 MFMA kernel's formulas restated: gamma = (ld + 8) u over |q| (1 + 1e-6) and max|v| (1 + 1e-6)
  for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP, TSH_METRIC_COSINE})
    for (double qn2 : {1.0, 0.3, 977.0, 1e-12})
      for (float vmax_f : {1.0f, 3.3f, 1e-3f}) {
        const BatchShardFacts s = shard(100000, 771, metric, 0.5f * vmax_f, vmax_f);
        const double qn = std::sqrt(qn2) * (1.0 + 1e-6), vmax = (double)vmax_f * (1.0 + 1e-6), gam = ((double)s.ld + 8.0) * u2;
        double delta = metric == TSH_METRIC_IP ? gam * qn * vmax
                       : metric == TSH_METRIC_COSINE ? qn * (gam + std::ldexp(1.0, -21))
                                                     : 2.0 * gam * qn * vmax + 6.0 * u2 * (qn * qn + vmax * vmax);
        delta += 771 * 7.5e-37;
        const double d2 = 2.0 * delta * 1.0001;
        float got = -1.f, qsq = -1.f, alpha = -1.f;
        CHECK(batch_delta2(s, 0, qn2, &got, &qsq, &alpha), "a finite band");
        CHECK((double)got >= d2 && (double)std::nextafter(got, 0.f) < d2, "metric %d: delta2 %.9g rounds %.17g up", metric, (double)got, d2);
        CHECK(qsq == (float)qn2 && alpha == 0.f, "qsq and alpha of the f32 kernel");
      }
  // the chain term: 2 c / (1 - 2 c) (1 + 1e-6) with c = (round_up(dim, 64) + 12) u, rounded up; fp16, L2 / inner product only
  for (int dim : {64, 100, 768, 771, 4096}) {
    const double c = ((double)((dim + 63) / 64 * 64) + 12.0) * u2, v = 2.0 * c / (1.0 - 2.0 * c) * (1.0 + 1e-6);
    for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP}) {
      const float f = batch_chain2(shard(100000, dim, metric), 2);
      CHECK((double)f >= v && (double)std::nextafter(f, 0.f) < v, "chain2 at dim %d: %.9g rounds %.17g up", dim, (double)f, v);
      CHECK(batch_chain2(shard(100000, dim, metric), 0) == 0.f && batch_chain2(shard(100000, dim, metric), 1) == 0.f, "chain2 of kernels 0 / 1");
    }
    CHECK(batch_chain2(shard(100000, dim, TSH_METRIC_COSINE), 2) == 0.f, "chain2 of cosine keys");
  }
  // alpha: per-row bands are the fp16 kernel's, L2 / inner product
  for (int metric : {TSH_METRIC_L2, TSH_METRIC_IP, TSH_METRIC_COSINE})
    for (int kernel : {0, 1, 2}) {
      float d2 = 0, qsq = 0, alpha = -1.f;
      CHECK(batch_delta2(shard(100000, 768, metric, 0.5f, 2.f), kernel, 1.7, &d2, &qsq, &alpha), "a finite band");
      const bool per_row = kernel == 2 && metric != TSH_METRIC_COSINE;
      CHECK(per_row ? alpha > 0.f : alpha == 0.f, "alpha %g of kernel %d, metric %d", (double)alpha, kernel, metric);
      CHECK(d2 > 0.f, "a band of zero width");
      // monotone in |q| and max|v|
      float last_d2 = 0, last_alpha = 0;
      for (double qn2 : {1e-6, 0.01, 1.0, 1.0000001, 50.0, 1e6}) {
        float a2 = 0, b2 = 0, q2 = 0;
        CHECK(batch_delta2(shard(100000, 768, metric, 0.5f, 2.f), kernel, qn2, &b2, &q2, &a2), "a finite band");
        CHECK(b2 >= last_d2 && a2 >= last_alpha, "kernel %d metric %d: the band shrinks as |q| grows", kernel, metric);
        last_d2 = b2, last_alpha = a2;
      }
      last_d2 = 0, last_alpha = 0;
      for (float vmax : {0.001f, 0.5f, 1.f, 1.0000001f, 30.f, 1e4f}) {
        float a2 = 0, b2 = 0, q2 = 0;
        CHECK(batch_delta2(shard(100000, 768, metric, 0.0005f, vmax), kernel, 1.3, &b2, &q2, &a2), "a finite band");
        CHECK(b2 >= last_d2 && a2 >= last_alpha, "kernel %d metric %d: the band shrinks as max|v| grows", kernel, metric);
        last_d2 = b2, last_alpha = a2;
      }
      // no band: a non-finite or overlarge one
      float x = 0, y = 0, z = 0;
      CHECK(!batch_delta2(shard(100000, 768, metric, 0.5f, 2.f), kernel, INFINITY, &x, &y, &z), "an infinite query");
      CHECK(!batch_delta2(shard(100000, 768, metric, 0.5f, 2.f), kernel, std::nan(""), &x, &y, &z), "a NaN query");
      CHECK(!batch_delta2(shard(100000, 768, metric, 0.5f, 1e19f), kernel, 1e76, &x, &y, &z), "a band beyond 1e30");
    }
}

// ---- query_norms ----------------------------------------------------------------------------------------------------
static void test_query_norms() {
  std::mt19937 rng(11);
  std::normal_distribution<float> nd(0.f, 1.f);
  const int dim = 37, stride = 41;
  std::vector<float> q((size_t)stride * 8);
  for (float &x : q) x = nd(rng) * 3.f;
  for (int n = 1; n <= 8; ++n) {
    double qn2[8];
    float qmax[8];
    char ok[8];
    std::memset(ok, 7, sizeof ok);
    query_norms(q.data(), stride, dim, n, qn2, qmax, ok);
    for (int j = 0; j < n; ++j) {
      double acc = 0;
      float mx = 0;
      for (int i = 0; i < dim; ++i) {
        const float v = q[(size_t)j * stride + i];
        acc = acc + (double)v * (double)v;
        mx = std::fabs(v) > mx ? std::fabs(v) : mx;
      }
      CHECK(std::memcmp(&acc, &qn2[j], 8) == 0 && mx == qmax[j] && ok[j] == 1, "n = %d, query %d: %.17g against %.17g", n, j, qn2[j], acc);
    }
  }
  const float poison[3] = {std::nanf(""), INFINITY, 2.0e15f};
  for (int which = 0; which < 3; ++which)
    for (int at : {0, dim - 1}) {
      std::vector<float> p = q;
      p[(size_t)3 * stride + at] = poison[which];
      double qn2[8];
      float qmax[8];
      char ok[8];
      query_norms(p.data(), stride, dim, 8, qn2, qmax, ok);
      for (int j = 0; j < 8; ++j) CHECK(ok[j] == (j != 3), "poison %d at %d: ok[%d] = %d", which, at, j, (int)ok[j]);
    }
  CHECK(BIG_ABS == 1.0e15f, "BIG_ABS");
  std::vector<float> edge = q;
  edge[5] = 1.0e15f;
  edge[6] = -1.0e15f;
  double qn2[8];
  float qmax[8];
  char ok[8];
  query_norms(edge.data(), stride, dim, 1, qn2, qmax, ok);
  CHECK(ok[0] == 1 && qmax[0] == 1.0e15f, "|x| = BIG_ABS is inside the error model");
}

// ---- QAux -----------------------------------------------------------------------------------------------------------
static void test_qaux() {
  std::vector<float> buf(6 * 384);
  const QAux a{buf.data(), 384};
  CHECK(QAux::PLANES == 6 && a.qsq() == buf.data() && a.delta2() == buf.data() + 384 && a.thr() == buf.data() + 768 &&
            (float *)a.tau_est() == buf.data() + 1152 && a.kmax() == buf.data() + 1536 && a.alpha() == buf.data() + 1920,
        "the six planes, in the order the kernels' uploads take them: [qsq | delta2] and [kmax | alpha] are neighbours");
}

// ---- the hub bound --------------------------------------------------------------------------------------------------
static void test_hub() {
  BatchShardFacts s = shard(1000000, 768, TSH_METRIC_L2, 0.5f, 2.f);
  CHECK(!plan_batch(s, call(64, 10)).hub, "off by default");
  s.batch_hub = true;
  CHECK(plan_batch(s, call(64, 10)).hub, "on: an L2 shard with varying norms");
  CHECK(!plan_batch(s, masked(64, 10, BatchMask::POINTER, 500000)).hub, "not behind a mask");
  CHECK(!plan_batch(s, call(64, 1025)).hub && plan_batch(s, call(64, 1024)).hub, "k <= 1024");
  BatchShardFacts t = s;
  t.rows = 65535;
  CHECK(!plan_batch(t, call(64, 10)).hub, "a small shard");
  t = s;
  t.max_norm = 0.505f;
  CHECK(!plan_batch(t, call(64, 10)).hub, "norms all but equal");
  t = s;
  t.metric = TSH_METRIC_COSINE;
  CHECK(!plan_batch(t, call(64, 10)).hub, "cosine");
  t = s;
  t.batch_kernel = 1;
  CHECK(!plan_batch(t, call(64, 10)).hub, "bf16x3 keys");
}

int main() {
  test_sample_rows();
  test_k_est();
  test_kernel_choice();
  test_listed();
  test_sample_window();
  test_chunks();
  test_cand_cap();
  test_takes_batch();
  test_bands();
  test_query_norms();
  test_qaux();
  test_hub();
  if (fails) {
    printf("%d misses\n", fails);
    return 1;
  }
  printf("batch plan ok\n");
  return 0;
}
