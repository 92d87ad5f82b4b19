// tsh_host_batch.inl.h -- host side of the batched (matrix-core) path: the scratch sets, and a call as a sequence of
// stages that carry out the plan of tsh_batch_plan.h (every decision of a call is made there, host only and CPU-tested)
// Part of the single translation unit tsh_lib.hip (textually included there; not compiled alone).

// ---- batched (matrix-core) path ---------------------------------------------------
static_assert(BATCH_TILE_ROWS == PLANE_GROUP && BATCH_BLOCK_ROWS == PG_ROWS && BATCH_FINAL_MAX == RF_MAX && BATCH_EXACT_MAX == EX_MAX_ROWS,
              "tsh_batch_plan.h restates the kernels' constants");
#ifdef TSH_PROBES
static uint64_t *g_f16_dbg_buf = nullptr;  // TSH_F16_DBG & 32 probe (probe builds only: -DTSH_PROBES)
#endif
struct BatchCtx;
// One buffer of a scratch set: device memory, with TWIN a pinned host array of the same size beside it, and the capacity
// of either in elements.  Every buffer is an allocation of its own: one that failed to grow reads as empty on the next call.
template <typename T, bool TWIN = false>
struct BatchBuf {
  T *d = nullptr, *h = nullptr;
  int64_t cap = 0;
  int grow(int64_t want, BatchCtx *b);
  void free() {
    hipFree(d);
    if (TWIN) hipHostFree(h);
  }
};
// ... and pinned host memory the device stores into (zero-copy): host pointer + the address the device uses
template <typename T>
struct BatchPinned {
  T *h = nullptr, *dev = nullptr;
  int64_t cap = 0;
  int grow(int64_t want, BatchCtx *b);
  void free() { hipHostFree(h); }
};

struct BatchCtx {
  std::mutex mu;  // one call at a time per scratch set (a shard has two: Shard::batch, batch2)
  BatchBuf<float, true> Q;     // the padded queries
  BatchBuf<u32x4> Qs;          // their bf16 / fp16 planes
  BatchBuf<float, true> qaux;  // QAux: six planes of nq_pad
  BatchBuf<float> dense;       // the sample's keys (nq_pad x n_sample)
  BatchBuf<float> wnorm;       // upper bounds of the sample rows' norms (per-row bands of the fp16 keys)
  BatchBuf<uint32_t> ck, cr, cc;  // candidate keys, rows (nq x cand_cap) and counts (nq_pad x CC_STRIDE)
  BatchBuf<uint8_t, true> blocks;
  uint8_t *h_blocks_dev = nullptr;  // blocks.h as the device sees it (results are stored straight into it)
  BatchBuf<uint32_t> final_rows;
  BatchBuf<uint64_t, true> mask;  // a pointer mask's slice, in 64-row words
  BatchBuf<float> dense2;         // the hub rows' dense keys (nq_pad x HUB_ROWS)
  // a call behind a SELECTIVE mask (listed_mode): the kept rows' ids, their fp16 copy and norms
  BatchBuf<uint32_t, true> list;
  BatchBuf<u32x4> gplane;
  BatchBuf<float> gsq;
  BatchBuf<BlockEntry, true> quar_out;  // [query][quarantined row] exact sums
  // results finalised on the device (rerank_final_kernel): pinned host arrays the kernel stores into
  BatchPinned<int64_t> fin_ids;    // nq x k
  BatchPinned<double> fin_dist;    // nq x k
  BatchPinned<int32_t> fin_cnt;    // nq
  BatchPinned<uint32_t> fin_info;  // nq: flags << 24 | count of each list's header
  BatchBuf<double, true> sqrt_mag;  // per query: sqrt(mag_a)
  template <typename F>
  void each_buf(F f) {
    f(Q), f(Qs), f(qaux), f(dense), f(wnorm), f(ck), f(cr), f(cc), f(blocks), f(final_rows), f(mask), f(dense2), f(list);
    f(gplane), f(gsq), f(quar_out), f(fin_ids), f(fin_dist), f(fin_cnt), f(fin_info), f(sqrt_mag);
  }
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr, e3 = nullptr, e_done = nullptr;
  hipEvent_t e_chunk[3] = {nullptr, nullptr, nullptr};  // tail chunks but the last
  hipEvent_t e_up = nullptr;  // the call's inputs have arrived (upload stream -> batch stream)
  int64_t bytes = 0;
  double last_gemm_us = 0, last_flops = 0;  // key passes of the last TIMED call
  // timed: events around the key passes (tsh_bench_batch, TSH_TRACE_BATCH).  Off otherwise: every record between two
  // kernels is a packet the queue works through while the GPU idles (~6 us each, three of them per call)
  bool timed = false;
  int32_t est_backoff = 0;  // calls left during which the estimated threshold stays off (it failed too often)
  int64_t est_unverified = 0;  // queries whose estimated threshold turned out too tight (redone exactly)
  int64_t last_nq = 0, last_nq_pad = 0, last_sample = 0;  // shape of dense / qaux.h after the last call (tsh_probe_batch_keys)
  int32_t last_sample_force = 0;  // tsh_probe_batch_keys: the next call's dense sample covers every row
  double last_wait_us = 0;  // how long the previous call waited for the GPU after enqueueing
  std::vector<double> mag_a;  // per query of the current call: sum of q[i]^2 in element order
};

void batch_free(BatchCtx *b) {
  b->each_buf([](auto &buf) { buf.free(); });
  for (hipEvent_t e : {b->e0, b->e1, b->e2, b->e3, b->e_done, b->e_chunk[0], b->e_chunk[1], b->e_chunk[2], b->e_up})
    if (e) hipEventDestroy(e);
}

// TSH_TEST_FAIL_ALLOC_OVER=bytes (tests; obeyed only after TSH_OPT_TEST_HOOKS, see test_env): device allocations of the batched path at or above this size fail as if the
// device were full -- the degrade ladder of shard_search_any (planes -> f32 MFMA -> single-query scans) can then be
// walked deterministically, beside the test that really fills the device
inline bool alloc_fault(int64_t bytes) {
  const char *e = test_env("TSH_TEST_FAIL_ALLOC_OVER");  // (not cached: the hooks may be switched on after the first call)
  const int64_t over = e ? atoll(e) : 0;
  return over > 0 && bytes >= over;
}

// Is there room on the current device for an allocation of `bytes`?  Asked BEFORE hipMalloc for the batched path's big
// buffers: the runtime's own out-of-memory path is best not entered -- it walks its queues to release memory, and in
// a process that had created and destroyed CU-masked streams before (the test-suite; a host that opens and closes
// indexes) a failing 200 MB hipMalloc ended in a segmentation fault inside libhsa-runtime64 instead of
// hipErrorOutOfMemory (native backtrace: tools/abort_trace.sh).  Not a reservation -- another thread may take the room
// in between, and then hipMalloc's own verdict stands.
inline bool device_has_room(int64_t bytes) {
  if (bytes < (4ll << 20)) return true;  // (small buffers: not worth the query)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return true;
  }
  return (int64_t)free_b >= bytes + (16ll << 20);
}

template <typename T, bool TWIN>
int BatchBuf<T, TWIN>::grow(int64_t want, BatchCtx *b) {
  if (want <= cap) return TSH_OK;
  hipFree(d);
  d = nullptr;
  if (TWIN) {
    hipHostFree(h);
    h = nullptr;
  }
  b->bytes -= cap * (int64_t)sizeof(T);  // (a failed allocation below leaves an empty buffer, not a dangling capacity)
  cap = 0;
  if (alloc_fault(want * (int64_t)sizeof(T))) return set_err(TSH_E_OOM, "hipMalloc failed: out of memory (injected)");
  if (!device_has_room(want * (int64_t)sizeof(T)))
    return set_err(TSH_E_OOM, "no room on the device for %lld bytes of batch scratch", (long long)(want * (int64_t)sizeof(T)));
  hipError_t e = hipMalloc(&d, (size_t)want * sizeof(T));
  if (e == hipSuccess && TWIN) {
    e = hipHostMalloc(&h, (size_t)want * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) {
      hipFree(d);
      d = nullptr;
    }
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();  // the runtime's sticky copy: a later hipGetLastError() must not report this again
    return set_err(e == hipErrorOutOfMemory ? TSH_E_OOM : TSH_E_HIP, "hipMalloc of %lld bytes failed: %s",
                   (long long)(want * (int64_t)sizeof(T)), hipGetErrorString(e));
  }
  b->bytes += want * (int64_t)sizeof(T);
  cap = want;
  return TSH_OK;
}

template <typename T>
int BatchPinned<T>::grow(int64_t want, BatchCtx *b) {
  if (want <= cap) return TSH_OK;
  hipHostFree(h);
  h = nullptr;
  dev = nullptr;
  b->bytes -= cap * (int64_t)sizeof(T);
  cap = 0;
  HIPCHK(hipHostMalloc(&h, (size_t)want * sizeof(T), hipHostMallocDefault));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), h, 0));
  b->bytes += want * (int64_t)sizeof(T);
  cap = want;
  return TSH_OK;
}

// (launch_batch_score_m: tsh_batch_tu.hip -- the key kernels compile as a translation unit of their own)

inline bool trace_batch() {
  static const bool on = getenv("TSH_TRACE_BATCH") != nullptr;
  return on;
}

// what tsh_batch_plan.h reads of a shard
BatchShardFacts batch_shard_facts(const Shard *s) {
  BatchShardFacts f;
  f.rows = s->rows;
  f.cap = s->cap;
  f.ld = s->ld;
  f.dim = s->dim;
  f.metric = s->metric;
  f.min_norm = s->min_norm;
  f.max_norm = s->max_norm;
  f.max_abs = s->max_abs;
  f.batch_kernel = s->batch_kernel;
  f.batch_group = s->batch_group;
  f.batch_hub = s->batch_hub;
  f.exact_rows = s->exact_rows;
  f.safe_mode = s->safe_mode();
  return f;
}
inline int probe_sample_div() {
  static const int div = probe_env("TSH_SAMPLE_DIV") ? std::max(4, atoi(probe_env("TSH_SAMPLE_DIV"))) : 32;  // experiments
  return div;
}

// ---- the hub rows (Shard::d_hub) -------------------------------------------------------------------------------------
// (Re)builds the gathered fp16 copy of the HUB_ROWS rows with the smallest (L2) / largest (inner product) norm.  Caller
// holds batch_enq_mu and s->mu shared; everything is enqueued on `st` but the selection, which needs the norms on the
// host once (4 MB for 1 M rows + a partial sort: a few milliseconds, at the first batched call and after the shard
// grew by a quarter).
int hub_build(Shard *s, hipStream_t st, int32_t hchunks, int v_exp) {
  const int64_t rows = s->rows;
  std::vector<float> sq((size_t)rows);
  HIPCHK(hipMemcpyAsync(sq.data(), s->d_sqnorm, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<uint32_t> ids((size_t)rows);
  for (int64_t i = 0; i < rows; ++i) ids[(size_t)i] = (uint32_t)i;
  const bool shortest = s->metric == TSH_METRIC_L2;
  // (quarantined and absent rows carry |v|^2 = 0: under L2 they would crowd the hub -- they are never live, the dense
  // pass drops them -- so rows of norm zero go last either way)
  auto better = [&](uint32_t x, uint32_t y) {
    const float a = sq[x], b2 = sq[y];
    if ((a > 0.f) != (b2 > 0.f)) return a > 0.f;
    return shortest ? (a < b2 || (a == b2 && x < y)) : (a > b2 || (a == b2 && x < y));
  };
  std::nth_element(ids.begin(), ids.begin() + HUB_ROWS, ids.end(), better);
  ids.resize(HUB_ROWS);
  std::sort(ids.begin(), ids.end());  // (row order: neighbouring hub rows share pages)
  std::vector<float> hsq(HUB_ROWS);
  for (int i = 0; i < HUB_ROWS; ++i) hsq[(size_t)i] = sq[ids[(size_t)i]];
  const int64_t bytes = (int64_t)HUB_ROWS * hchunks * 64;
  if (!s->d_hub || s->hub_chunks != hchunks) {
    hipFree(s->d_hub);
    s->d_hub = nullptr;
    s->bytes -= s->hub_bytes;
    s->hub_bytes = 0;
    if (alloc_fault(bytes) || !device_has_room(bytes)) return set_err(TSH_E_OOM, "no room for the hub rows' copy");
    HIPCHK(hipMalloc(&s->d_hub, (size_t)bytes));
    if (!s->d_hub_ids) HIPCHK(hipMalloc(&s->d_hub_ids, (size_t)HUB_ROWS * 4));
    if (!s->d_hub_sq) HIPCHK(hipMalloc(&s->d_hub_sq, (size_t)HUB_ROWS * 4));
    s->hub_bytes = bytes + HUB_ROWS * 8;
    s->bytes += s->hub_bytes;
  }
  HIPCHK(hipMemcpyAsync(s->d_hub_ids, ids.data(), (size_t)HUB_ROWS * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(s->d_hub_sq, hsq.data(), (size_t)HUB_ROWS * 4, hipMemcpyHostToDevice, st));
  Half32Args ha{};
  ha.rows = s->d_rows;
  ha.inv_norm = nullptr;
  ha.out = s->d_hub;
  ha.ld = s->ld;
  ha.first = 0;
  ha.n = HUB_ROWS;
  ha.dim = s->dim;
  ha.kchunks = hchunks;
  ha.scale = std::ldexp(1.0f, v_exp);
  ha.ids = s->d_hub_ids;
  const int64_t total = (int64_t)HUB_ROWS * hchunks * 4;
  half_rows32_kernel<<<(unsigned)std::min<int64_t>((total + 255) / 256, 65536), 256, 0, st>>>(ha);
  HIPCHK(hipStreamSynchronize(st));  // (ids / hsq are this function's own vectors)
  HIPCHK(hipGetLastError());
  s->hub_rows_built = rows;
  s->hub_n = HUB_ROWS;
  s->hub_exp = v_exp;
  s->hub_chunks = hchunks;
  return TSH_OK;
}

// ---- one batched call, stage by stage --------------------------------------------------------------------------------
// What the stages of shard_search_batch pass on: the call as given, its plan, and what the earlier stages found out.
struct BatchCall {
  Shard *s;
  BatchCtx *b;
  const float *queries;
  int32_t nq, k, entries;
  const MaskSrc &mask;
  SearchOut *out;
  std::vector<int32_t> *redo;
  size_t bb = 0;  // bytes of a candidate block
  BatchShardFacts sh;
  BatchCallFacts cf;
  BatchPlan p;
  // the mask: this shard's slice of it, host and device (a handle's words are resident; a pointer mask's are this call's)
  int32_t n_tiles_all = 0;
  int64_t kept = -1;  // rows the mask keeps (tombstones not subtracted); -1: no mask
  const uint64_t *h_mw = nullptr, *d_mw = nullptr;
  std::vector<uint32_t> quar_sel;  // quarantined rows (not live on the device) the mask keeps
  bool gpu_final = false;          // the finaliser runs on the device too (rerank_final_kernel)
  std::vector<char> bad;           // per query: outside the error model -- a zero query here, redone alone
  int q_exp = 0;                   // f16: queries are scaled by 2^q_exp
  int64_t s0 = 0;                  // first row of the sample
  int32_t k_est = 0;
  bool grouped = false;  // the plane this call scores is norm-grouped
  bool use_hub = false;
  int n_chunks = 1;
  int32_t n_unverified = 0, n_band_over = 0;
  double t_in = 0, t_prep = 0, t_enq = 0, t_gpu = 0;

  bool use_f16() const { return p.kern == 2; }
  // per-row bands: fp16 keys of an L2 / inner-product index (batch_delta2)
  // (the error-model probes, BatchCtx::last_sample_force, read the dense pass's keys as they are: no widths there -- what that call
  // answers is discarded)
  bool roww() const { return use_f16() && sh.metric != TSH_METRIC_COSINE && !cf.sample_force; }
  bool quar_host() const { return !quar_sel.empty() && !out->d_blocks; }  // host mode: the quarantined rows' sums come back
  QAux haux() const { return QAux{b->qaux.h, (size_t)p.nq_pad}; }
  QAux daux() const { return QAux{b->qaux.d, (size_t)p.nq_pad}; }
  const uint32_t *list_ids() const { return mask.part ? mask.part->list.d : b->list.d; }  // listed: the kept rows
};

// the shard's first scratch set stands for "either": a call that finds it taken by a concurrent call uses the second
std::unique_lock<std::mutex> batch_take_scratch(Shard *s, BatchCtx **b) {
  std::unique_lock<std::mutex> lk((*b)->mu, std::defer_lock);
  if (*b == s->batch && s->batch2 && !lk.try_lock()) {
    std::unique_lock<std::mutex> lk2(s->batch2->mu, std::try_to_lock);
    if (lk2.owns_lock()) {
      *b = s->batch2;
      lk = std::move(lk2);
    }
  }
  if (!lk.owns_lock()) lk.lock();
  return lk;
}

// The mask, early: how many rows it keeps decides how the call is scored.  A pointer mask is sliced and counted into the
// call's scratch; a mask handle's words are resident, host and device: no copy of them here.
int batch_resolve_mask(BatchCall &c) {
  BatchCtx *b = c.b;
  c.n_tiles_all = (int32_t)((c.sh.rows + 63) / 64);
  int rc;
  if (c.mask.bytes && (rc = b->mask.grow((int64_t)c.n_tiles_all, b))) return rc;
  if (c.mask.part) {
    c.kept = c.mask.part->kept;
    c.h_mw = c.mask.part->h_words.data();
    c.d_mw = c.mask.part->words.d;
  } else if (c.mask.bytes) {
    slice_mask(c.s, c.mask.bytes, b->mask.h, c.n_tiles_all);  // (bits past the last row keep nothing: slice_mask clears them)
    c.kept = popcount_words(b->mask.h, (size_t)c.n_tiles_all);
    c.h_mw = b->mask.h;
    c.d_mw = b->mask.d;
  }
  return TSH_OK;
}

// The call's facts for plan_batch.  The fp16 denial is read HERE, once: listed mode and the key kernel's choice go by
// the same value, and batch_grow_scratch counts the call against it.
BatchCallFacts batch_call_facts(const BatchCall &c, int force_kernel) {
  static const int forced_tile = probe_env("TSH_BATCH_TILE") ? atoi(probe_env("TSH_BATCH_TILE")) : 0;  // experiments
  static const bool proven_tau = probe_env("TSH_BATCH_PROVEN_TAU") != nullptr && probe_env("TSH_BATCH_PROVEN_TAU")[0] == '1';
  BatchCallFacts f;
  f.nq = c.nq;
  f.k = c.k;
  f.entries = c.entries;
  f.force_kernel = force_kernel;
  f.mask = c.mask.part ? BatchMask::HANDLE : (c.mask.bytes ? BatchMask::POINTER : BatchMask::NONE);
  f.kept = c.kept;
  f.handle_list = c.mask.part && c.mask.part->list.d && c.mask.part->list_padded > 0;
  f.f16_denied = (force_kernel >= 0 ? force_kernel : c.sh.batch_kernel) == 3 && c.s->f16_denied_calls.load() > 0;
  f.sample_force = c.b->last_sample_force != 0;
  f.est_backoff = c.b->est_backoff;
  f.forced_tile = forced_tile;
  f.sample_div = probe_sample_div();
  f.proven_tau = proven_tau;
  return f;
}

// Every allocation of the call but the mask's slice (batch_resolve_mask) and the hub rows' keys (hub_ensure), in a
// fixed order: a failing one returns TSH_E_OOM with the buffers before it grown and the ones behind it as they were.
int batch_grow_scratch(BatchCall &c) {
  Shard *s = c.s;
  BatchCtx *b = c.b;
  const BatchPlan &p = c.p;
  const int32_t nq = c.nq;
  int rc;
  if (!b->e0) {
    const unsigned wait_flag = blocking_wait() ? hipEventBlockingSync : 0;
    for (hipEvent_t *e : {&b->e0, &b->e1, &b->e2}) HIPCHK(hipEventCreate(e));
    HIPCHK(hipEventCreateWithFlags(&b->e3, wait_flag));  // timed, and the call's longest wait (the end of the key passes)
    HIPCHK(hipEventCreateWithFlags(&b->e_done, hipEventDisableTiming | wait_flag));
    for (hipEvent_t &e : b->e_chunk) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | wait_flag));
    HIPCHK(hipEventCreateWithFlags(&b->e_up, hipEventDisableTiming));
  }
  if ((rc = b->Q.grow((int64_t)p.nq_pad * c.sh.ld, b))) return rc;
  if ((rc = b->qaux.grow((int64_t)p.nq_pad * QAux::PLANES, b))) return rc;
  if ((rc = b->dense.grow((int64_t)p.nq_pad * p.n_sample, b))) return rc;
  if ((rc = b->wnorm.grow(p.n_sample, b))) return rc;
  if ((rc = b->ck.grow((int64_t)nq * p.cand_cap, b))) return rc;
  if ((rc = b->cr.grow((int64_t)nq * p.cand_cap, b))) return rc;
  if ((rc = b->cc.grow((int64_t)p.nq_pad * CC_STRIDE, b))) return rc;
  if ((rc = b->blocks.grow((int64_t)nq * (int64_t)c.bb, b))) return rc;
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->h_blocks_dev), b->blocks.h, 0));
  if ((rc = b->final_rows.grow((int64_t)nq * c.entries, b))) return rc;
  // the call runs: it is one of the F16_DENIAL_CALLS a denied shard sits out, and its kernel is the one tsh_counters names
  if (c.cf.f16_denied && s->f16_denied_calls.fetch_sub(1) == 1) s->f16_strikes.store(0);
  s->batch_kernel_last = p.kern;
  if (p.kern != 0 && (rc = b->Qs.grow(round_up(p.nq_pad, PLANE_GROUP) * p.hchunks * 8, b)))
    return rc;  // (sized for the bf16 hi + lo planes; the fp16 ones are half of it)
  if (p.listed) {  // the kept rows' fp16 copy (whole 256-row groups), their norms, their ids (a pointer mask's list: this call's)
    const int64_t prow = round_up(c.kept, PLANE_GROUP);
    if ((rc = b->gplane.grow(prow * p.hchunks * 4, b))) return rc;
    if ((rc = b->gsq.grow(prow, b))) return rc;
    if (!c.mask.part && (rc = b->list.grow(c.kept + 64, b))) return rc;
  }
  if (c.quar_host()) {  // their exact sums for every query, added to the blocks on the host
    if (!c.out->extra) return set_err(TSH_E_BAD_ARG, "no room for the quarantined rows' entries");
    if ((rc = b->quar_out.grow((int64_t)nq * (int64_t)s->quar_ids.size(), b))) return rc;
  }
  if (c.gpu_final) {
    if ((rc = b->fin_ids.grow((int64_t)nq * c.k, b))) return rc;
    if ((rc = b->fin_dist.grow((int64_t)nq * c.k, b))) return rc;
    if ((rc = b->fin_cnt.grow((int64_t)nq, b))) return rc;
    if ((rc = b->fin_info.grow((int64_t)nq, b))) return rc;
    if ((rc = b->sqrt_mag.grow((int64_t)nq, b))) return rc;
  }
  return TSH_OK;
}

// Host prep: padded queries, per-query bands (QAux), the queries the error model or the fp16 scale cannot cover (bad[]).
void batch_prepare_queries(BatchCall &c) {
  BatchCtx *b = c.b;
  const BatchShardFacts &sh = c.sh;
  const int32_t nq = c.nq, nq_pad = c.p.nq_pad;
  const int64_t ld = sh.ld;
  const int kern = c.p.kern;
  const float *queries = c.queries;
  const QAux ha = c.haux();
  float *h_qsq = ha.qsq(), *h_d2 = ha.delta2(), *h_kmax = ha.kmax(), *h_alpha = ha.alpha();
  // the largest key a row can have (IP: -dot <= |q| max|v|; cosine planes hold unit rows; L2: (|q| + max|v|)^2): caps
  // the thresholds of the fp16 kernel's filtered pass.  1 % above it: a row AT the largest key still passes an
  // "everything passes" threshold with its key's error (<= 0.13 % of that scale) on top
  const double kmax_v = sh.metric == TSH_METRIC_COSINE ? 1.0 : (double)sh.max_norm;
  std::vector<char> &bad = c.bad;
  bad.assign((size_t)nq, 0);
  std::vector<float> qmax((size_t)nq_pad, 0.f);
  b->mag_a.resize((size_t)nq);  // the finaliser's sum of q[i]^2 (cosine), a by-product of the band computation
  parallel_for((nq_pad + QN_GROUP - 1) / QN_GROUP, [&](int32_t g) {
    const int32_t g0 = g * QN_GROUP, g1 = std::min(nq_pad, g0 + QN_GROUP), gn = std::max(0, std::min(nq, g1) - g0);
    char ok[QN_GROUP];
    if (gn > 0) query_norms(queries + (size_t)g0 * sh.dim, sh.dim, sh.dim, gn, &b->mag_a[(size_t)g0], &qmax[(size_t)g0], ok);
    for (int32_t q = g0; q < g1; ++q) {
      float *dst = b->Q.h + (size_t)q * ld;
      h_kmax[q] = 0.f;
      h_alpha[q] = 0.f;
      if (q < nq && ok[q - g0] && batch_delta2(sh, kern, b->mag_a[(size_t)q], &h_d2[q], &h_qsq[q], &h_alpha[q])) {
        memcpy(dst, queries + (size_t)q * sh.dim, (size_t)sh.dim * sizeof(float));
        for (int64_t i = sh.dim; i < ld; ++i) dst[i] = 0.f;
        const double qn_q = std::sqrt(b->mag_a[(size_t)q]);
        const double km = (sh.metric == TSH_METRIC_L2 ? (qn_q + kmax_v) * (qn_q + kmax_v) : qn_q * kmax_v) * 1.01 + 1e-30;
        h_kmax[q] = km < 3e38 ? (float)km : 3e38f;
      } else {
        if (q < nq) {
          qmax[(size_t)q] = 0.f;
          bad[(size_t)q] = 1;  // outside the error model: a zero query here, redone alone
        }
        memset(dst, 0, (size_t)ld * sizeof(float));
        h_d2[q] = 0.f;
        h_qsq[q] = 0.f;
        h_alpha[q] = 0.f;
      }
    }
  });
  // f16: one power-of-two scale for the whole batch; queries much smaller than the largest one would sit
  // in fp16's subnormal range, so they are answered alone
  auto drop = [&](int32_t q) {
    bad[(size_t)q] = 1;
    memset(b->Q.h + (size_t)q * ld, 0, (size_t)ld * sizeof(float));
    h_d2[q] = 0.f;
    h_qsq[q] = 0.f;
  };
  c.q_exp = 0;
  if (c.use_f16()) {
    float top_q = 0.f;
    for (int32_t q = 0; q < nq; ++q) top_q = std::max(top_q, qmax[(size_t)q]);
    for (int32_t q = 0; q < nq; ++q)
      if (!bad[(size_t)q] && !(qmax[(size_t)q] >= top_q * 0.00390625f)) drop(q);
    if (top_q > 0.f && !f16_scale_exp(top_q, &c.q_exp)) {  // same guard on the query side: answer them one by one
      c.q_exp = 0;
      for (int32_t q = 0; q < nq; ++q)
        if (!bad[(size_t)q]) drop(q);
    }
  }
  if (c.gpu_final)
    for (int32_t q = 0; q < nq; ++q) b->sqrt_mag.h[q] = std::sqrt(b->mag_a[(size_t)q]);
}

// Where the sample sits behind a mask (sample_window), and a listed call's list of kept rows.
void batch_place_sample(BatchCall &c) {
  BatchCtx *b = c.b;
  const BatchPlan &p = c.p;
  if (p.listed && !c.mask.part) list_mask_bits(b->mask.h, c.n_tiles_all, c.kept, b->list.h);  // ascending ids of the kept rows
  c.s0 = 0;
  c.k_est = p.k_est;
  if (!c.mask || p.listed || p.n_sample >= c.sh.rows) return;
  std::vector<int32_t> pre_own;
  if (!c.mask.part) {
    pre_own.assign((size_t)c.n_tiles_all + 1, 0);
    for (int32_t t = 0; t < c.n_tiles_all; ++t) pre_own[(size_t)t + 1] = pre_own[(size_t)t] + __builtin_popcountll(c.h_mw[t]);
  }
  const std::vector<int32_t> &pre = c.mask.part ? c.mask.part->pre : pre_own;  // (a handle counted its words when it was made)
  const SampleWindow w = sample_window(pre.data(), c.n_tiles_all, c.sh.rows, p.n_sample, p.want_group);
  c.s0 = w.s0;
  // the estimate's order statistic counts KEPT rows: a range mask may have half of them inside the window, where
  // n_sample / rows would say a thirtieth -- and a threshold taken that much too low fails its check for every query
  c.k_est = batch_k_est(c.k, std::max<int64_t>(pre[(size_t)c.n_tiles_all], 1), std::max<int64_t>(w.best, 0), c.cf.est_backoff,
                        c.cf.proven_tau);
}

// The inputs travel on the device's upload stream: with two calls in flight they arrive while the call in front
// still computes (on the batch stream the 3 MB of a 1024 x 768 batch were 50-60 us of idle matrix cores per call:
// two callers 450-600 k queries/s against 608-638 k on one box, tools/ab_batch.sh; one caller: no difference)
int batch_upload(BatchCall &c) {
  BatchCtx *b = c.b;
  const int32_t nq = c.nq, nq_pad = c.p.nq_pad;
  const QAux ha = c.haux(), da = c.daux();
  hipStream_t up = c.s->upload_stream;
  HIPCHK(hipMemcpyAsync(b->Q.d, b->Q.h, (size_t)nq_pad * c.sh.ld * sizeof(float), hipMemcpyHostToDevice, up));
  HIPCHK(hipMemcpyAsync(da.qsq(), ha.qsq(), (size_t)nq_pad * 2 * sizeof(float), hipMemcpyHostToDevice, up));    // qsq, delta2
  HIPCHK(hipMemcpyAsync(da.kmax(), ha.kmax(), (size_t)nq_pad * 2 * sizeof(float), hipMemcpyHostToDevice, up));  // kmax, alpha
  if (c.mask.bytes) HIPCHK(hipMemcpyAsync(b->mask.d, b->mask.h, (size_t)c.n_tiles_all * 8, hipMemcpyHostToDevice, up));
  if (c.p.listed && !c.mask.part) HIPCHK(hipMemcpyAsync(b->list.d, b->list.h, (size_t)c.kept * 4, hipMemcpyHostToDevice, up));
  if (c.gpu_final) HIPCHK(hipMemcpyAsync(b->sqrt_mag.d, b->sqrt_mag.h, (size_t)nq * sizeof(double), hipMemcpyHostToDevice, up));
  HIPCHK(hipEventRecord(b->e_up, up));
  return TSH_OK;
}

// bf16x3 / f16 kernels: the shard's converted copy of the rows, its perm / psq maps (a norm-grouped fp16 plane) and the
// split_* bookkeeping.  Allocation and invalidation only -- the conversion of stale rows is enqueued with the call
// (batch_enqueue_operands).  Caller holds batch_enq_mu.  A listed call scores a gathered copy of its own: the shard's
// copy is neither needed nor built.
int planes_ensure(BatchCall &c) {
  Shard *s = c.s;
  const int kern = c.p.kern, v_exp = c.p.v_exp;
  c.grouped = false;
  if (kern == 0 || c.p.listed) return TSH_OK;
  const bool use_f16 = c.use_f16();
  const int64_t row_bytes = (int64_t)c.p.hchunks * (use_f16 ? 64 : 128);  // fp16: 2 B per element, bf16 hi + lo: 4 B
  if (s->split_mode != kern || (use_f16 && s->split_exp != v_exp)) s->split_valid = 0;  // other format / scale
  if (s->split_cap < s->cap || s->split_mode != kern) {  // first use, other format, or the row store grew
    if (s->d_split) hipFree(s->d_split);
    s->d_split = nullptr;
    s->bytes -= s->split_bytes;
    s->split_bytes = 0;
    s->split_cap = 0;
    s->split_valid = 0;
    const int64_t prow = round_up(s->cap, PLANE_GROUP);  // whole 256-row groups (plane_piece)
    // (no kernel of this call has been launched yet: a device too full for the copy is the caller's cue to score
    // with the f32 kernel instead, shard_search_any.  The call's inputs ARE on their way -- H2D copies out of the
    // pinned buffers the retry will rewrite -- so they are waited for before this call gives up)
    const hipError_t pe = alloc_fault(prow * row_bytes) || !device_has_room(prow * row_bytes)
                              ? hipErrorOutOfMemory
                              : hipMalloc(&s->d_split, (size_t)prow * (size_t)row_bytes);
    if (pe != hipSuccess) {
      s->d_split = nullptr;
      (void)hipGetLastError();
      (void)hipEventSynchronize(c.b->e_up);
      return set_err(pe == hipErrorOutOfMemory ? TSH_E_OOM : TSH_E_HIP, "hipMalloc of the %s copy of the rows (%lld bytes) failed: %s",
                     use_f16 ? "fp16" : "bf16x3", (long long)(prow * row_bytes), hipGetErrorString(pe));
    }
    s->split_cap = s->cap;
    s->split_bytes = prow * row_bytes;
    s->bytes += s->split_bytes;
  }
  s->split_mode = kern;
  s->split_exp = v_exp;
  c.grouped = use_f16 && c.p.want_group;
  if (c.grouped && s->perm_cap < s->split_cap) {  // (a device too full for the two maps: the plane stays in row order)
    hipFree(s->d_perm);
    hipFree(s->d_psq);
    s->d_perm = nullptr;
    s->d_psq = nullptr;
    s->bytes -= s->perm_bytes;
    s->perm_bytes = 0;
    s->perm_cap = 0;
    const int64_t prow = round_up(s->split_cap, PLANE_GROUP);
    if (alloc_fault(prow * 8) || !device_has_room(prow * 8) || hipMalloc(&s->d_perm, (size_t)prow * 4) != hipSuccess ||
        hipMalloc(&s->d_psq, (size_t)prow * 4) != hipSuccess) {
      (void)hipGetLastError();
      hipFree(s->d_perm);
      s->d_perm = nullptr;
      c.grouped = false;
    } else {
      s->perm_cap = s->split_cap;
      s->perm_bytes = prow * 8;
      s->bytes += s->perm_bytes;
    }
  }
  if (s->split_grouped != c.grouped) {  // the other order: the whole plane again
    s->split_valid = 0;
    s->split_grouped = c.grouped;
  }
  return TSH_OK;
}

// The hub rows' bound, where the plan left it a candidate: the rows' copy current (hub_build) and room for their keys.
// A device too full for either, or any failure on the way: the call goes without the bound.  Caller holds batch_enq_mu.
void hub_ensure(BatchCall &c) {
  Shard *s = c.s;
  c.use_hub = c.p.hub && !c.grouped;  // (either cure for crowded rows, not both)
  if (c.use_hub && (s->hub_rows_built < 0 || s->hub_exp != c.p.v_exp || s->hub_chunks != c.p.hchunks ||
                    c.sh.rows - s->hub_rows_built > s->hub_rows_built / 4)) {
    if (hub_build(s, s->aux_stream, c.p.hchunks, c.p.v_exp) != TSH_OK) c.use_hub = false;
  }
  if (c.use_hub && c.b->dense2.grow((int64_t)c.p.nq_pad * HUB_ROWS, c.b) != TSH_OK) c.use_hub = false;
}

// The key kernels' operands: the shard's planes brought up to its rows (or a listed call's gathered copy), the queries'
// planes, and the fields of BatchArgs that name them.
int batch_enqueue_operands(BatchCall &c, hipStream_t st, BatchArgs *a) {
  Shard *s = c.s;
  BatchCtx *b = c.b;
  const BatchPlan &p = c.p;
  const int64_t rows = c.sh.rows, ld = c.sh.ld;
  const int32_t hchunks = p.hchunks;
  if (p.kern == 1) {
    auto split = [&](const float *src, int64_t first, int64_t n, u32x4 *dst) {
      SplitArgs sa{};
      sa.rows = src;
      sa.out = dst;
      sa.ld = ld;
      sa.first = first;
      sa.n = n;
      sa.dim = s->dim;
      sa.hchunks = hchunks;
      const int64_t total = n * hchunks * 4;
      split_rows_kernel<<<(unsigned)std::min<int64_t>((total + 255) / 256, 65536), 256, 0, st>>>(sa);
    };
    if (s->split_valid < rows) {
      split(s->d_rows, s->split_valid, rows - s->split_valid, s->d_split);
      s->split_valid = rows;
    }
    split(b->Q.d, 0, p.nq_pad, b->Qs.d);
    a->Qs = b->Qs.d;
    a->Vs = s->d_split;
    a->hchunks = hchunks;
  } else if (p.kern == 2) {
    auto half = [&](const float *src, const float *inv, int64_t first, int64_t n, u32x4 *dst, int e, const uint32_t *ids = nullptr) {
      Half32Args ha{};
      ha.ids = ids;
      ha.rows = src;
      ha.inv_norm = inv;
      ha.out = dst;
      ha.ld = ld;
      ha.first = first;
      ha.n = n;
      ha.dim = s->dim;
      ha.kchunks = hchunks;
      ha.scale = std::ldexp(1.0f, e);
      const int64_t total = n * hchunks * 4;
      half_rows32_kernel<<<(unsigned)std::min<int64_t>((total + 255) / 256, 65536), 256, 0, st>>>(ha);
    };
    const float *inv = s->metric == TSH_METRIC_COSINE ? s->d_inv_norm : nullptr;
    const uint32_t *d_ids = p.listed ? c.list_ids() : nullptr;
    if (p.listed) {  // the kept rows, gathered: norms by list position, fp16 rows by list position
      gather_f32_kernel<<<(unsigned)((c.kept + 255) / 256), 256, 0, st>>>(s->d_sqnorm, d_ids, b->gsq.d, (int32_t)c.kept);
      half(s->d_rows, inv, 0, c.kept, b->gplane.d, p.v_exp, d_ids);
    } else if (s->split_valid < rows) {
      int64_t from = s->split_valid;
      if (c.grouped) {  // whole blocks again from the one the first stale row sits in: positions [from, rows) and their rows
        from = from / PG_ROWS * PG_ROWS;
        PlaneGroupArgs ga{};
        ga.sqnorm = s->d_sqnorm;
        ga.perm = s->d_perm;
        ga.psq = s->d_psq;
        ga.first = from;
        ga.rows = rows;
        ga.longest_first = s->metric == TSH_METRIC_IP ? 1 : 0;
        plane_group_kernel<<<(unsigned)((rows - from + PG_ROWS - 1) / PG_ROWS), 1024, 0, st>>>(ga);
      }
      half(s->d_rows, inv, from, rows - from, s->d_split, p.v_exp, c.grouped ? s->d_perm + from : nullptr);
      s->split_valid = rows;
    }
    half(b->Q.d, nullptr, 0, p.nq_pad, b->Qs.d, c.q_exp);
    a->Qs = b->Qs.d;
    a->Vs = p.listed ? b->gplane.d : s->d_split;
    a->row_ids = d_ids;
    a->hchunks = hchunks;
    a->dot_scale = std::ldexp(1.0f, -(c.q_exp + p.v_exp));
#ifdef TSH_PROBES
    static const int f16_dbg = probe_env("TSH_F16_DBG") ? atoi(probe_env("TSH_F16_DBG")) : 0;  // probes: results are wrong
    a->dbg = f16_dbg;
    static uint64_t *d_dbg = nullptr;
    if ((f16_dbg & 32) && !d_dbg) HIPCHK(hipMalloc(&d_dbg, (4 * 96 * 12 + 16) * sizeof(uint64_t)));
    if (f16_dbg & 32) HIPCHK(hipMemsetAsync(d_dbg, 0, (4 * 96 * 12 + 16) * sizeof(uint64_t), st));
    a->dbg_buf = d_dbg;
    g_f16_dbg_buf = d_dbg;
#endif
  }
  return TSH_OK;
}

// The call's sequence on the shard's batch stream (unmasked: the GEMM scales with CU count): B0 dense keys of the sample,
// B0s per-query thresholds, B1 everything else filtered, B2 final select, re-rank -- the tail in chunks, an event each.
// Caller holds batch_enq_mu: one call's sequence at a time on the one in-order stream.
int batch_enqueue(BatchCall &c) {
  Shard *s = c.s;
  BatchCtx *b = c.b;
  SearchOut *out = c.out;
  const BatchPlan &p = c.p;
  const int32_t nq = c.nq, nq_pad = p.nq_pad, k = c.k, entries = c.entries, tile_n = p.tile_n, cand_cap = p.cand_cap;
  const int64_t rows = c.sh.rows, ld = c.sh.ld, n_sample = p.n_sample, s0 = c.s0;
  const size_t bb = c.bb;
  const bool listed = p.listed, roww = c.roww(), gpu_final = c.gpu_final;
  const int32_t n_quar = (int32_t)s->quar_ids.size();
  const QAux da = c.daux();
  hipStream_t st = s->batch_stream;
  HIPCHK(hipStreamWaitEvent(st, b->e_up, 0));
  if (c.quar_host()) {
    QuarArgs qa{};
    qa.rows = s->d_rows;
    qa.Q = b->Q.d;
    qa.list = s->d_quar;
    qa.out = b->quar_out.d;
    qa.ld = ld;
    qa.ldq = ld;
    qa.row_base = s->row_base;
    qa.dim = s->dim;
    qa.cap = n_quar;
    qa.metric = s->metric;
    quarantine_kernel<<<dim3((unsigned)((n_quar + 63) / 64), (unsigned)nq), 64, 0, st>>>(qa);
    HIPCHK(hipMemcpyAsync(b->quar_out.h, b->quar_out.d, (size_t)nq * n_quar * sizeof(BlockEntry), hipMemcpyDeviceToHost, st));
  }
  BatchArgs a{};
  int rc;
  if ((rc = batch_enqueue_operands(c, st, &a))) return rc;
  a.Q = b->Q.d;
  a.V = s->d_rows;
  a.inv_norm = c.use_f16() ? nullptr : s->d_inv_norm;  // f16 planes of a cosine corpus hold unit rows
  if (listed) {
    a.sqnorm = b->gsq.d;
  } else {
    a.sqnorm = c.grouped ? s->d_psq : s->d_sqnorm;  // (by plane position, like everything the key kernel indexes by column)
    a.row_ids = c.grouped ? s->d_perm : nullptr;
  }
  a.qsq = da.qsq();
  a.thr = da.thr();
  a.kmax = da.kmax();
  const float chain2 = batch_chain2(c.sh, p.kern);
  a.alpha = roww ? da.alpha() : nullptr;
  // (listed: the list IS the mask; its rows' live bits are always looked up -- a handle's list may name rows deleted since)
  a.live = listed ? s->d_live : (s->all_live ? nullptr : s->d_live);
  a.mask = listed ? nullptr : c.d_mw;
  a.dense = b->dense.d;
  a.cand_key = b->ck.d;
  a.cand_row = b->cr.d;
  a.cand_cnt = b->cc.d;
  a.ld = ld;
  a.dense_ld = n_sample;
  a.nq = nq;
  a.nq_pad = nq_pad;
  a.kchunks = (int32_t)((ld + BT_K - 1) / BT_K);
  a.cand_cap = cand_cap;
  a.tile_m = p.tile;
  a.q_tiles = nq_pad / p.tile;
  // B0: dense keys of the sample rows
  a.row0 = (int32_t)s0;
  a.row1 = (int32_t)(s0 + n_sample);
  a.n_tiles = (int32_t)((n_sample + tile_n - 1) / tile_n);
  const bool timed = b->timed || trace_batch();
  if (timed) HIPCHK(hipEventRecord(b->e0, st));
  launch_batch_score_m(s->metric, a, true, st, s->cus);
  if (c.use_hub) {  // the hub rows, densely: a gathered copy with its own norms and a map back to the rows' live bits
    BatchArgs ah = a;
    ah.Vs = s->d_hub;
    ah.sqnorm = s->d_hub_sq;
    ah.row_ids = s->d_hub_ids;
    ah.dense = b->dense2.d;
    ah.dense_ld = HUB_ROWS;
    ah.row0 = 0;
    ah.row1 = HUB_ROWS;
    ah.n_tiles = HUB_ROWS / tile_n;
    launch_batch_score_m(s->metric, ah, true, st, s->cus);
  }
  if (timed) HIPCHK(hipEventRecord(b->e1, st));
  // B0s: per-query threshold + the sample's own candidates
  SampleSelArgs ss{};
  ss.dense = b->dense.d;
  ss.delta2 = da.delta2();
  ss.thr = da.thr();
  ss.cand_key = b->ck.d;
  ss.cand_row = b->cr.d;
  ss.cand_cnt = b->cc.d;
  ss.dense_ld = n_sample;
  ss.n_sample = (int32_t)n_sample;
  ss.k = k;
  ss.k_est = c.k_est;
  ss.tau_est = da.tau_est();
  ss.cand_cap = cand_cap;
  ss.row0 = (int32_t)s0;
  ss.alpha = a.alpha;
  ss.sqnorm = s->d_sqnorm;
  ss.chain2 = chain2;
  ss.norm_max = s->max_norm;
  ss.hub_dense = c.use_hub ? b->dense2.d : nullptr;
  ss.hub_ld = HUB_ROWS;
  ss.hub_n = HUB_ROWS;
  ss.row_ids = a.row_ids;
  if (roww) {  // the sample rows' norms, once per call
    sample_norms_kernel<<<(unsigned)((n_sample + 255) / 256), 256, 0, st>>>(a.sqnorm + s0, b->wnorm.d, (int32_t)n_sample);
    ss.wnorm = b->wnorm.d;
  }
  // one workgroup per query: a small batch leaves most CUs empty, so its workgroups get sixteen waves instead of
  // four (128 queries: 76 -> 54 and 58 -> 50 us); with a thousand workgroups the wide shape loses (the one-wave
  // bisect phases idle fifteen waves: 103 -> 235 us)
  const bool wide_select = nq <= 256;
  if (roww) {
    if (wide_select) batch_sample_select_roww_kernel<BS_THREADS_WIDE><<<nq, BS_THREADS_WIDE, 0, st>>>(ss);
    else batch_sample_select_roww_kernel<BS_THREADS><<<nq, BS_THREADS, 0, st>>>(ss);
  } else if (wide_select) batch_sample_select_kernel<BS_THREADS_WIDE><<<nq, BS_THREADS_WIDE, 0, st>>>(ss);
  else batch_sample_select_kernel<BS_THREADS><<<nq, BS_THREADS, 0, st>>>(ss);
  // B1: everything else, filtered
  if (timed) HIPCHK(hipEventRecord(b->e2, st));
  if (s0 > 0 && !listed) {  // (a sample window inside the rows: the filtered pass runs on either side of it)
    a.row0 = 0;
    a.row1 = (int32_t)s0;
    a.n_tiles = (int32_t)((s0 + tile_n - 1) / tile_n);
    launch_batch_score_m(s->metric, a, false, st, s->cus);
  }
  if (!listed && rows > s0 + n_sample) {
    a.row0 = (int32_t)(s0 + n_sample);
    a.row1 = (int32_t)rows;
    a.n_tiles = (int32_t)((rows - s0 - n_sample + tile_n - 1) / tile_n);
    launch_batch_score_m(s->metric, a, false, st, s->cus);
  }
  HIPCHK(hipEventRecord(b->e3, st));
  // B2 + rerank
  FinalSelArgs fs{};
  fs.cand_key = b->ck.d;
  fs.cand_row = b->cr.d;
  fs.cand_cnt = b->cc.d;
  fs.delta2 = da.delta2();
  fs.tau_est = da.tau_est();
  // host mode: headers and re-ranked entries are stored straight into pinned host memory (only the `count`
  // valid entries cross PCIe, and no copy sits between the last kernel and the host)
  const bool zero_copy = out->d_blocks == nullptr;
  fs.blocks = b->blocks.d;
  // (device-finalised calls: the re-rank's launch reports each header in one word beside the results; the headers'
  // own stores into host memory, 1024 small PCIe writes in front of that launch, are left out)
  fs.blocks_host = zero_copy && !gpu_final ? b->h_blocks_dev : nullptr;
  fs.final_rows = b->final_rows.d;
  fs.block_bytes = (int64_t)bb;
  fs.row_base = s->row_base;
  fs.shard_rows = rows;
  fs.k = k;
  fs.cand_cap = cand_cap;
  fs.entries = entries;
  fs.metric = s->metric;
  fs.alpha = a.alpha;
  fs.sqnorm = s->d_sqnorm;
  fs.thr = da.thr();
  fs.kmax = a.kmax;
  fs.chain2 = chain2;
  if (roww) {
    if (wide_select) batch_final_select_roww_kernel<BS_THREADS_WIDE><<<nq, BS_THREADS_WIDE, 0, st>>>(fs);
    else batch_final_select_roww_kernel<BS_THREADS><<<nq, BS_THREADS, 0, st>>>(fs);
  } else if (wide_select) batch_final_select_kernel<BS_THREADS_WIDE><<<nq, BS_THREADS_WIDE, 0, st>>>(fs);
  else batch_final_select_kernel<BS_THREADS><<<nq, BS_THREADS, 0, st>>>(fs);
  RerankBatchArgs rb{};
  rb.rows = s->d_rows;
  rb.Q = b->Q.d;
  rb.final_rows = b->final_rows.d;
  rb.blocks = b->blocks.d;
  rb.out_blocks = zero_copy ? b->h_blocks_dev : b->blocks.d;
  rb.block_bytes = (int64_t)bb;
  rb.ld = ld;
  rb.row_base = s->row_base;
  rb.dim = s->dim;
  rb.entries = entries;
  rb.metric = s->metric;
  // the tail runs in chunks of queries: while the GPU re-ranks chunk c + 1, the host already finalises chunk c
  // (out->on_chunk).  (One launch over all chunks, each reporting through a pinned word when its last workgroup
  // has stored its entries, was tried: 167 us against 4 x 48 -- no overlap to speak of -- and the waits for the
  // host-memory stores to land doubled it.  Consecutive chunks on two streams: no change, a chunk's 512 workgroups of
  // 70 KB LDS fill every CU and the next chunk's only start as they leave.)
  c.n_chunks = batch_n_chunks(nq, gpu_final || !out->on_chunk);
  if (gpu_final) {
    // one launch for the whole call: a re-ranking wave is latency-bound, so the more of them are in flight the better,
    // and with the finaliser on the device no host work is left to overlap chunk by chunk
    RerankFinalArgs rf{};
    rf.r = rb;
    rf.r.q0 = 0;
    rf.sqrt_mag_a = b->sqrt_mag.d;
    rf.thr = out->fin_thr;
    rf.out_ids = b->fin_ids.dev;
    rf.out_dist = b->fin_dist.dev;
    rf.out_count = b->fin_cnt.dev;
    rf.out_info = b->fin_info.dev;
    rf.k = k;
    static const bool old_shape = probe_env("TSH_RF_SHAPE") != nullptr && probe_env("TSH_RF_SHAPE")[0] == '2';  // A/B: two waves, 64-float pieces
    if (old_shape) rerank_final_kernel<RwBig><<<(unsigned)nq, 64 * RwBig::WAVES, 0, st>>>(rf);
    else rerank_final_kernel<RwFin><<<(unsigned)nq, 64 * RwFin::WAVES, 0, st>>>(rf);
    HIPCHK(hipEventRecord(b->e_done, st));
    return TSH_OK;
  }
  for (int ch = 0; ch < c.n_chunks; ++ch) {
    const int32_t q0 = chunk_q(c.n_chunks, nq, ch), q1 = chunk_q(c.n_chunks, nq, ch + 1);
    rb.q0 = q0;
    rerank_batch_kernel<<<dim3((unsigned)((entries + RW_CAND - 1) / RW_CAND), (unsigned)(q1 - q0)), 64 * RwBig::WAVES, 0, st>>>(rb);
    if (!c.quar_sel.empty() && out->d_blocks) {  // shard mode: the quarantined rows go into the device blocks
      QuarAppendArgs qa{};
      qa.rows = s->d_rows;
      qa.Q = b->Q.d + (size_t)q0 * ld;
      qa.list = s->d_quar;
      qa.mask = c.d_mw;
      qa.blocks = b->blocks.d + (size_t)q0 * bb;
      qa.ld = ld;
      qa.ldq = ld;
      qa.row_base = s->row_base;
      qa.block_bytes = (int64_t)bb;
      qa.dim = s->dim;
      qa.entries = entries;
      qa.metric = s->metric;
      quarantine_append_kernel<<<dim3((unsigned)((n_quar + 63) / 64), (unsigned)(q1 - q0)), 64, 0, st>>>(qa);
    }
    if (!zero_copy)
      HIPCHK(hipMemcpyAsync(b->blocks.h + (size_t)q0 * bb, b->blocks.d + (size_t)q0 * bb, (size_t)(q1 - q0) * bb,
                            hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ch + 1 < c.n_chunks ? b->e_chunk[ch] : b->e_done, st));
  }
  return TSH_OK;
}

// The chunk waits: as each chunk of the tail arrives its queries are sorted into done or redo and handed to the caller
// (callbacks, or a copy); then the timed figures.
int batch_collect(BatchCall &c) {
  Shard *s = c.s;
  BatchCtx *b = c.b;
  SearchOut *out = c.out;
  const int32_t nq = c.nq;
  const size_t bb = c.bb;
  const bool gpu_final = c.gpu_final;
  const int32_t n_quar = (int32_t)s->quar_ids.size();
  // the finalisation below starts the moment the GPU is done: if that is within a millisecond (going by the
  // previous call), the pool's workers keep polling through the wait instead of parking (waking them cost 50-70 us
  // of a 128-query call's 90 us of finalisation)
  if ((out->on_chunk || gpu_final) && b->last_wait_us > 0 && b->last_wait_us < 900.0)
    HostPool::get().stay_awake_until(c.t_enq + b->last_wait_us * 1.1 + 50.0);
  std::vector<char> skip((size_t)nq, 0);
  // From the end of the key passes on the pool gets a job every few dozen microseconds (one per chunk of the tail):
  // the long wait blocks, then the workers are woken and poll until the call is over
  // (ranks that outnumber the CPU quota: a device-finalised call has one copy left for the pool -- not worth workers
  // polling through the select and re-rank kernels)
  std::unique_ptr<HostPool::Hold> hold;
  if ((out->on_chunk || gpu_final) && nq >= 24 && !(gpu_final && blocking_wait())) {
    HIPCHK(hipEventSynchronize(b->e3));
    hold.reset(new HostPool::Hold());
  }
  for (int ch = 0; ch < c.n_chunks; ++ch) {
    const int32_t q0 = chunk_q(c.n_chunks, nq, ch), q1 = chunk_q(c.n_chunks, nq, ch + 1);
    HIPCHK(hipEventSynchronize(ch + 1 < c.n_chunks ? b->e_chunk[ch] : b->e_done));
    if (ch == 0) b->last_wait_us = now_us() - c.t_enq;
    if (ch + 1 == c.n_chunks) {
      HIPCHK(hipGetLastError());
      c.t_gpu = now_us();
    }
    for (int32_t q = q0; q < q1; ++q) {
      const BlockHeader *h = reinterpret_cast<const BlockHeader *>(b->blocks.h + (size_t)q * bb);
      const uint32_t h_flags = gpu_final ? b->fin_info.h[q] >> 24 : h->flags;
      const uint32_t h_count = gpu_final ? b->fin_info.h[q] & 0xFFFFFFu : h->count;
      if (c.bad[(size_t)q] || (h_flags & FLAG_LIST_OVERFLOW)) {
        if (h_flags & FLAG_TAU_UNVERIFIED) ++c.n_unverified;
        else if (!c.bad[(size_t)q]) ++c.n_band_over;  // a threshold existed and held: the band itself was too wide for the list
        c.redo->push_back(q);
        skip[(size_t)q] = 1;
      } else {
        s->c_cands += h_count;
        if (c.quar_host()) {  // the quarantined rows join this query's candidates
          std::vector<BlockEntry> &ex = (*out->extra)[(size_t)(out->q_base + q)];
          ex.clear();
          for (uint32_t i : c.quar_sel) ex.push_back(b->quar_out.h[(size_t)q * n_quar + i]);
        }
      }
    }
    const double t_c0 = now_us();
    if (gpu_final) {
      out->on_final(q0, q1, skip.data(), b->fin_ids.h, b->fin_dist.h, b->fin_cnt.h);  // a copy is all that is left
    } else if (out->on_chunk) {
      out->on_chunk(q0, q1, skip.data(), b->blocks.h, b->mag_a.data());  // finalised straight from the pinned buffer
      // (queries the single-query path will redo write their blocks to out->h_blocks themselves)
    } else if (out->h_blocks) {
      memcpy(out->h_blocks + (size_t)q0 * bb, b->blocks.h + (size_t)q0 * bb, (size_t)(q1 - q0) * bb);
    }
    if (trace_batch()) fprintf(stderr, "[tsh batch]   chunk %d: event at %.0f us, finalised in %.0f us\n", ch, t_c0 - c.t_enq, now_us() - t_c0);
  }
  if (b->timed || trace_batch()) {
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(hipEventElapsedTime(&ms0, b->e0, b->e1));
    HIPCHK(hipEventElapsedTime(&ms1, b->e2, b->e3));
    b->last_gemm_us = ((double)ms0 + (double)ms1) * 1e3;
    b->last_flops = 2.0 * nq * (double)c.p.scan_rows * (double)s->dim;
  }
  return TSH_OK;
}

// What the call leaves behind: the fp16 strikes and denial, the estimate's back-off, the shape the probes read, the
// counters -- and, in device mode, the blocks in the caller's buffer.
int batch_account(BatchCall &c) {
  Shard *s = c.s;
  BatchCtx *b = c.b;
  const int32_t nq = c.nq;
  // auto mode: fp16 keys whose band keeps overflowing the lists of this corpus (every overflow is a whole scan) give
  // way to bf16x3 ones, 25 x narrower, after two such calls (cosine keys are scale-free: never)
  // Counted: queries whose threshold held and whose list still overflowed.  Not counted: queries the error model
  // rejected (bad[]), failed estimates, and calls with a caller mask (a mask that leaves the sample fewer than k kept
  // rows has no threshold at all: every kept row survives, whatever the key kernel).
  if (c.p.kern == 2 && c.p.want_kernel == 3 && s->metric != TSH_METRIC_COSINE && c.entries >= RF_MAX && !c.mask &&
      !c.cf.sample_force) {  // (at the widest lists only)
    if (c.n_band_over > std::max(2, nq / 16)) {
      if (s->f16_strikes.fetch_add(1) + 1 >= 2) s->f16_denied_calls.store(F16_DENIAL_CALLS);
    } else if (c.n_band_over == 0) {
      s->f16_strikes.store(0);
    }
  }
  b->est_unverified += c.n_unverified;
  if (b->est_backoff > 0) --b->est_backoff;
  else if (c.n_unverified > std::max(1, nq / 64)) b->est_backoff = 64;  // the sample does not represent these rows
  b->last_nq = nq;
  b->last_nq_pad = c.p.nq_pad;
  b->last_sample = c.p.n_sample;
  s->c_batches++;
  s->c_searches += nq - (int64_t)c.redo->size();
  if (c.out->d_blocks) {
    hipStream_t us = c.out->user_stream ? c.out->user_stream : s->batch_stream;
    HIPCHK(hipMemcpyAsync(c.out->d_blocks, b->blocks.d, (size_t)nq * c.bb, hipMemcpyDeviceToDevice, us));
    if (blocking_wait()) {  // (hipStreamSynchronize spins)
      HIPCHK(hipEventRecord(b->e_done, us));
      HIPCHK(hipEventSynchronize(b->e_done));
    } else {
      HIPCHK(hipStreamSynchronize(us));
    }
  }
  return TSH_OK;
}

#ifdef TSH_PROBES
// probe (TSH_F16_DBG & 32): the ping-pong kernel's raw stamps of two waves of workgroup 0 (main pass: the last launch),
// relative to the wave's first, one line per chunk (points 0-9)
int batch_probe_timeline(int32_t nq) {
  if (!g_f16_dbg_buf || nq < 1024) return TSH_OK;
  std::vector<uint64_t> hb(4 * 96 * 12 + 16);
  HIPCHK(hipMemcpy(hb.data(), g_f16_dbg_buf, hb.size() * 8, hipMemcpyDeviceToHost));
  fprintf(stderr, "[pp cnt] wave tiles %llu, crowded %llu, more than two per lane %llu, hit blocks %llu\n", (unsigned long long)hb[4 * 96 * 12],
          (unsigned long long)hb[4 * 96 * 12 + 1], (unsigned long long)hb[4 * 96 * 12 + 2], (unsigned long long)hb[4 * 96 * 12 + 3]);
  const int wv[4] = {0, 4, 1, 5};
  for (int w = 0; w < 4; ++w) {
    const uint64_t *b0 = &hb[(size_t)(w * 96) * 12];
    fprintf(stderr, "[pp dbg] wave %d hw_id 0x%llx simd %llu\n", wv[w], (unsigned long long)b0[11], (unsigned long long)((b0[11] >> 4) & 3));
    for (int st2 = 0; st2 < 60; ++st2) {
      const uint64_t *t = &hb[(size_t)(w * 96 + st2) * 12];
      fprintf(stderr, "[pp dbg]  w%d c%02d:", wv[w], st2);
      for (int pt = 0; pt < 12; ++pt) fprintf(stderr, " %7lld", t[pt] ? (long long)(t[pt] - hb[0]) : -1ll);
      fprintf(stderr, "\n");
    }
  }
  return TSH_OK;
}
#endif

// All nq queries in one pass over the rows on the matrix cores.  Queries the
// error model cannot cover, or whose lists overflow (ties), are reported in
// *redo and answered by the single-query path.  Caller holds s->mu shared.
// force_kernel >= 0: that key kernel instead of the handle's choice (0 = f32 MFMA on the rows as stored, the one that
// needs no converted copy: shard_search_any falls to it when the copy cannot be allocated).  An allocation failure
// returns TSH_E_OOM with nothing of the call left in flight and nothing written: the caller may retry or answer
// another way.
int shard_search_batch(Shard *s, BatchCtx *b, const float *queries, int32_t nq, int32_t k,
                       const MaskSrc &mask, int32_t entries, SearchOut *out, std::vector<int32_t> *redo,
                       int force_kernel = -1) {
  std::unique_lock<std::mutex> lk = batch_take_scratch(s, &b);
  BatchCall c{s, b, queries, nq, k, entries, mask, out, redo};
  c.t_in = now_us();
  HIPCHK(hipSetDevice(s->device));
  // A call the device finalises (below: gpu_final) never shows its candidate blocks to anybody, so their size is this
  // function's own business: as wide as the finalising kernel takes.  The caller's default (k + 156) is the
  // single-query path's, whose f32 keys have a band 100 x narrower than fp16 ones: an L2 / IP corpus whose norms
  // vary (band ~ max|v|, interesting rows ~ min|v|) overflowed 256-entry lists for a third of its queries, and every
  // overflow is a query redone by a whole scan (1 M x 768 L2, 1024 queries: 97 ms per call instead of 2.4).
  if (out->on_final && !out->d_blocks && s->quar_ids.empty() && entries <= RF_MAX && k <= entries) c.entries = RF_MAX;
  c.bb = (size_t)tsh_candidate_block_bytes(c.entries);
  c.sh = batch_shard_facts(s);
  int rc;
  if ((rc = batch_resolve_mask(c))) return rc;
  c.cf = batch_call_facts(c, force_kernel);
  c.p = plan_batch(c.sh, c.cf);
  // quarantined rows (not live on the device): their exact sums for every query join the blocks.  The finaliser runs on
  // the device too when the caller wants final results on the host and nothing but the device's own candidate lists
  // goes into them
  if (!s->quar_ids.empty()) quarantine_select(s, c.h_mw, &c.quar_sel);
  c.gpu_final = out->on_final && !out->d_blocks && c.quar_sel.empty() && c.entries <= RF_MAX && k <= c.entries;
  if ((rc = batch_grow_scratch(c))) return rc;
  batch_prepare_queries(c);
  batch_place_sample(c);
  c.t_prep = now_us();
  if ((rc = batch_upload(c))) return rc;
  {
    std::lock_guard<std::mutex> enq(s->batch_enq_mu);  // one call's sequence at a time, and the planes' upkeep
    if ((rc = planes_ensure(c))) return rc;
    hub_ensure(c);
    if ((rc = batch_enqueue(c))) return rc;
  }
  c.t_enq = now_us();
  if ((rc = batch_collect(c))) return rc;
  if ((rc = batch_account(c))) return rc;
#ifdef TSH_PROBES
  if ((rc = batch_probe_timeline(nq))) return rc;
#endif
  if (trace_batch())
    fprintf(stderr, "[tsh batch] nq=%d prep %.0f us, enqueue %.0f us, gpu wait %.0f us, post %.0f us (gemm %.0f us)\n", nq,
            c.t_prep - c.t_in, c.t_enq - c.t_prep, c.t_gpu - c.t_enq, now_us() - c.t_gpu, b->last_gemm_us);
  return TSH_OK;
}

// rows a caller's mask keeps on this shard (the pointer form, counted for the cost model below: tsh_host_sync.h)
int64_t mask_kept_rows(const Shard *s, const uint8_t *bytes) { return tsh::mask_kept_rows(s->row_base, s->rows, bytes); }

// (the cost model: tsh_batch_plan.h)
inline bool shard_takes_batch(const Shard *s, int32_t batch_min_nq, int32_t nq, int32_t k, int64_t kept = -1) {
  return tsh::shard_takes_batch(batch_shard_facts(s), batch_min_nq, nq, k, kept);
}

// nq queries on one shard: matrix-core batch when it pays, single-query pipeline
// otherwise and for whatever the batch hands back.
int shard_search_any(Shard *s, BatchCtx *b, int32_t batch_min_nq, const float *queries, int32_t nq, int32_t k,
                     const MaskSrc &mask, int32_t entries, SearchOut *out) {
  // (a mask's kept rows, for the cost model: a handle knows them; a pointer mask is counted when the answer can matter)
  int64_t kept = -1;
  if (mask && batch_min_nq == 1 && nq >= 2 && nq <= 512) kept = mask.part ? mask.part->kept : mask_kept_rows(s, mask.bytes);
  const bool use_batch = shard_takes_batch(s, batch_min_nq, nq, k, kept);
  if (!use_batch) return shard_search_blocks(s, queries, nq, k, mask, entries, out, PIPE_DEPTH);
  std::vector<int32_t> redo;
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  // the dense sample matrix (nq_pad x n_sample floats) is kept under 8 GB per call
  const int64_t per_q = batch_sample_rows(s->rows, k, false, probe_sample_div()) * 4;
  const int32_t chunk = (int32_t)std::max<int64_t>(256, (int64_t)(8e9 / (double)per_q) / 256 * 256);
  for (int32_t q0 = 0; q0 < nq; q0 += chunk) {
    const int32_t nc = std::min(chunk, nq - q0);
    SearchOut part;
    part.h_blocks = out->h_blocks ? out->h_blocks + (size_t)q0 * bb : nullptr;
    part.d_blocks = out->d_blocks ? out->d_blocks + (size_t)q0 * bb : nullptr;
    part.user_stream = out->user_stream;
    part.extra = out->extra;
    part.q_base = out->q_base + q0;
    part.fin_thr = out->fin_thr;
    if (out->on_final)
      part.on_final = [out, q0, k](int32_t a, int32_t b2, const char *skip, const int64_t *ids, const double *dist, const int32_t *cnt) {
        out->on_final(q0 + a, q0 + b2, skip - q0, ids - (size_t)q0 * k, dist - (size_t)q0 * k, cnt - q0);
      };
    if (out->on_chunk)  // indices of the callback are the caller's: shift this part's
      part.on_chunk = [out, q0, bb](int32_t a, int32_t b2, const char *skip, const uint8_t *base, const double *mag_a) {
        out->on_chunk(q0 + a, q0 + b2, skip - q0, base - (size_t)q0 * bb, mag_a - q0);
      };
    std::vector<int32_t> r;
    const int force = s->planes_denied.load() > 0 && s->batch_kernel != 0 ? 0 : -1;
    int rc = shard_search_batch(s, b, queries + (size_t)q0 * s->dim, nc, k, mask, entries, &part, &r, force);
    // A device too full for this call's allocations is no reason to fail a search the rows themselves can answer:
    // first without the converted copy of the rows (f32 MFMA kernel on the rows as stored, smaller scratch), then
    // without the batched path at all (pipelined single-query scans need nothing beyond their contexts).  Same
    // results on every path; tsh_counters says which ran.
    if (rc == TSH_E_OOM && force != 0 && s->batch_kernel != 0) {
      r.clear();
      rc = shard_search_batch(s, b, queries + (size_t)q0 * s->dim, nc, k, mask, entries, &part, &r, 0);
      if (rc == TSH_OK) {
        s->c_plane_fallbacks++;
        s->planes_denied.store(64);  // the copy is tried again after that many calls, not on every one
      }
    } else if (rc == TSH_OK && force == 0) {
      s->c_plane_fallbacks++;
      s->planes_denied.fetch_sub(1);
    }
    if (rc == TSH_E_OOM) {
      s->c_scan_fallbacks++;
      r.clear();
      // (no callbacks: the blocks land in the caller's buffers and the caller finalises them, as it does for
      // queries the batch hands back)
      std::vector<std::vector<BlockEntry>> sp((size_t)(out->spill ? nc : 0)), ex((size_t)(out->extra ? nc : 0));
      SearchOut scans;
      scans.h_blocks = part.h_blocks;
      scans.d_blocks = part.d_blocks;
      scans.user_stream = part.user_stream;
      scans.spill = out->spill ? &sp : nullptr;
      scans.extra = out->extra ? &ex : nullptr;
      rc = shard_search_blocks(s, queries + (size_t)q0 * s->dim, nc, k, mask, entries, &scans, PIPE_DEPTH);
      for (int32_t q = 0; q < nc && rc == TSH_OK; ++q) {
        if (out->spill) (*out->spill)[(size_t)(q0 + q)] = std::move(sp[(size_t)q]);
        if (out->extra) (*out->extra)[(size_t)(out->q_base + q0 + q)] = std::move(ex[(size_t)q]);
      }
    }
    if (rc) return rc;
    for (int32_t q : r) redo.push_back(q0 + q);
  }
  int rc = TSH_OK;
  for (int32_t q : redo) {
    SearchOut one;
    std::vector<std::vector<BlockEntry>> sp(1), ex(1);
    one.h_blocks = out->h_blocks ? out->h_blocks + (size_t)q * bb : nullptr;
    one.d_blocks = out->d_blocks ? out->d_blocks + (size_t)q * bb : nullptr;
    one.user_stream = out->user_stream;
    one.spill = out->spill ? &sp : nullptr;
    one.extra = out->extra ? &ex : nullptr;
    rc = shard_search_blocks(s, queries + (size_t)q * s->dim, 1, k, mask, entries, &one, 1);
    if (rc) return rc;
    if (out->spill) (*out->spill)[(size_t)q] = std::move(sp[0]);
    if (out->extra) (*out->extra)[(size_t)(out->q_base + q)] = std::move(ex[0]);
  }
  return TSH_OK;
}

