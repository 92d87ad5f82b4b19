// tsh_lib.hip -- host side of libtostore_hip.so (C-ABI in include/tostore_hip.h).
//
// Owns the device-resident copy of one vector index's float32 embedding column
// (the data the reference keeps in <index>/ngh/rawvec pages,
// /root/reference/lib/src/core/ngh_page.dart:310-450) and answers
// NghGraphEngine.search-shaped queries (ngh_graph_engine.dart:67-135) with the
// kernels in tsh_kernels.hip.h.  No CPU fallback exists: without a device every
// compute entry returns TSH_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cctype>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "../../include/tostore_hip.h"
#include "tsh_after.hip.h"
#include "tsh_after_band.h"
#include "tsh_count.hip.h"
#include "tsh_count_band.h"
#include "tsh_group.hip.h"
#include "tsh_group_rows.hip.h"
#include "tsh_batch.hip.h"
#include "tsh_batch_f16.hip.h"
#include "tsh_batch_plan.h"
#include "tsh_exact.hip.h"
#include "tsh_finalize.h"
#include "tsh_host_sync.h"
#include "tsh_kernels.hip.h"
#include "tsh_launch.h"
#include "tsh_mask.hip.h"
#include "tsh_pq.hip.h"
#include "tsh_scan_f16_band.h"
#include "tsh_scan_i8.hip.h"
#include "tsh_scan_i8_band.h"
#include "tsh_scan_i4.hip.h"
#include "tsh_where.hip.h"
#include "tsh_tags.hip.h"
#include "tsh_facet.hip.h"

using namespace tsh;

namespace {

thread_local std::string g_err;

int set_err(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return set_err(e_ == hipErrorOutOfMemory ? TSH_E_OOM : TSH_E_HIP, "%s failed: %s", \
                     #expr, hipGetErrorString(e_));                                   \
  } while (0)

int device_count_cached() {
  static int n = [] {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    return c;
  }();
  return n;
}

constexpr int MAX_CTX = 8;            // contexts (queries in flight) per shard
constexpr int PIPE_DEPTH = 8;         // queries a multi-query call keeps in flight
constexpr int F16_DENIAL_CALLS = 256; // batched calls a shard stays off fp16 keys after its lists kept overflowing
constexpr uint32_t QUARANTINE_MAX = 1024;  // quarantined rows per shard; beyond that the shard goes to safe mode
constexpr int SUBMIT_THREADS = 1;     // host threads that submit a multi-query call (more did not help: the pipeline is GPU-bound)
constexpr int MAX_DIM_SCAN = 4096;    // register-resident query (NCH <= 16; the reference's f32 pages hold d <= 4073)
// (BIG_ABS, round_up: tsh_batch_plan.h)

// (the finaliser -- Hit, Cursor, Cursors, sort_hits, finalize_query, count_entries -- is in tsh_finalize.h: host only, CPU-tested)

// ---- kernel dispatch ---------------------------------------------------------
// (pick_nch -- row width -> the chunk count of its scan instantiation -- is in tsh_scan_widths.h: host only, CPU-tested)

// the scan kernels' launchers live in their own translation unit (tsh_scan_tu.hip): 144 instantiations that
// compile beside this file instead of in front of it
// ---- per-search scratch: one context = one query in flight ---------------------
struct Ctx {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_done = nullptr;  // recorded after a job's last kernel
  hipEvent_t ev_scanned = nullptr;  // scan stream -> tail stream hand-off
  uint8_t *h_block_dev = nullptr;  // device-side address of h_block (zero-copy result stores)
  float *d_query = nullptr;  // ld floats
  float *h_query = nullptr;  // pinned, ld floats
  uint64_t *d_mask = nullptr;
  uint64_t *h_mask = nullptr;  // pinned
  int64_t mask_words = 0;
  uint64_t mask_epoch = 0;  // which caller mask the device copy holds
  uint32_t *d_list = nullptr, *h_list = nullptr;  // selective masks: the kept rows' ids (scan_list_kernel), h_ pinned
  uint32_t *h_list_dev = nullptr;                 // ... and mapped: the exact path's first scan of a list reads it in place
  int64_t list_cap = 0;
  uint64_t list_epoch = 0;
  uint32_t *d_keys = nullptr;
  uint32_t *d_gmin = nullptr;
  uint32_t *d_hist = nullptr;  // radix select of the fallback path (256 bins)
  int64_t tiles_cap = 0;
  uint8_t *d_block = nullptr;  // header + entries
  uint8_t *h_block = nullptr;  // pinned
  uint32_t *d_cand = nullptr;  // entries
  int64_t entries_cap = 0;
  // wide-band fallback
  uint32_t *d_big_rows = nullptr;
  BlockEntry *d_big_entries = nullptr;
  uint32_t *d_big_count = nullptr;
  int64_t big_cap = 0;
  BlockEntry *h_quar = nullptr, *h_quar_dev = nullptr;  // pinned + mapped: sums of the quarantined rows
  // short searches (tsh_exact.hip.h): per entry the order key of its exact distance and its two f64 sums
  uint64_t *d_xkey = nullptr;
  double *d_xsum = nullptr;
  uint64_t *d_xpick = nullptr;  // exact_pick_kernel: [0] its counter (zero between searches), [1 ..] E1's wave minima
  int64_t x_cap = 0;
  // the coarse int8 scan's tail (tsh_scan_i8.hip.h): [tau, survivor total] and the survivor list of I8_LIST_CAP ids
  uint32_t *d_i8 = nullptr, *d_i8_list = nullptr;
  // the 4-bit first pass in front of it (tsh_scan_i4.hip.h): A's lower sides and tile minima, W's mask words, tau,
  // and, pinned + mapped, the survivors' total as the host reads it
  uint32_t *d_i4_keys = nullptr, *d_i4_gmin = nullptr, *d_i4_ctl = nullptr;
  uint64_t *d_i4_mask = nullptr;
  uint32_t *h_i4 = nullptr, *h_i4_dev = nullptr;
  int64_t i4_tiles_cap = 0;
  // cursor searches (tsh_after.hip.h): the side list of the rows the floor pass could not decide, its two count words
  // (side_flip: the one the next cursor job counts in -- the job before it left it at zero) and, pinned + mapped, their
  // count and entries: [0].id = count, [1 ..] the entries.  Count jobs (tsh_count.hip.h) use the same list and words, and a
  // third word, d_side_cnt[2], for the rows their window pass counted (zero between jobs)
  uint32_t *d_side_rows = nullptr, *d_side_cnt = nullptr;
  BlockEntry *h_side = nullptr, *h_side_dev = nullptr;
  int64_t side_cap = 0;
  int side_flip = 0;
  bool side_dirty = false;  // a cursor job is out, or one failed on the way: the count words are cleared before the next
  // grouped searches (tsh_group.hip.h): the heads array and its tile minima (sized like d_keys / d_gmin) and the head table,
  // a 64-bit word per group -- reserved by the context's first grouped job, cleared in front of every one
  uint32_t *d_heads = nullptr, *d_hmin = nullptr;
  int64_t heads_tiles = 0;
  unsigned long long *d_gm = nullptr;
  int64_t gm_cap = 0;
  // grouped searches with several rows per group (tsh_group_rows.hip.h): the control words and the three per-slot arrays
  // (count, placed, offset) in one allocation, and the member segments -- reserved by the context's first such job
  uint32_t *d_gr_ctl = nullptr;
  int64_t gr_slots = 0;
  unsigned long long *d_gr_seg = nullptr;
  int64_t gr_seg_cap = 0;
  int64_t bytes = 0;
};

// Streams are a finite resource (CU-masked ones especially: about 85 open indexes with their own
// five streams plus context streams crashed the runtime), and everything on one GPU shares its HBM and
// CUs anyway -- so all shards of a device share ONE set, created on first use and never destroyed.
constexpr int TAIL_CUS = 16;  // of a split device: two CUs of every XCD for the tails (make_scan_streams), the rest scan
struct DeviceStreams {
  hipStream_t ingest = nullptr;
  hipStream_t scan = nullptr, scan2 = nullptr;  // pipeline streams (240-CU mask when cu_split)
  hipStream_t tail = nullptr, tail2 = nullptr;  // the other 16 CUs (two queues: the tails of consecutive queries overlap)
  hipStream_t batch = nullptr;                  // unmasked: matrix-core batches
  hipStream_t aux = nullptr;                    // rare synchronous work (fallback filter, bench hooks)
  hipStream_t upload = nullptr;                 // a batched call's queries on their way in, beside the call before it
  bool cu_split = false;
  std::mutex scan_mu;                           // one enqueue sequence (scan + hand-off + tail) at a time
  // small shards run their scans on two streams: which scans of either are still out (guarded by scan_mu).  A new
  // scan goes to the stream with fewer of them -- two scans side by side do not share the HBM evenly, and with strict
  // alternation one stream ended a call a scan or two behind the other, which sat idle meanwhile
  struct ScanOut {
    const void *owner;  // the context whose job this scan belongs to
    hipEvent_t ev;      // rides on the scan's dispatch packet
    int which;
  };
  std::vector<ScanOut> scan_out;
  int scans_out[2] = {0, 0};
  uint64_t enq_counter = 0;  // jobs enqueued on this device's streams so far (guarded by scan_mu)
  int rc = TSH_OK;
  std::string err;
  int users = 0;                                // shards alive on this device (device_streams / device_streams_release)
  int cus = 0;
};
DeviceStreams *device_streams(int device);  // defined after set_err / HIPCHK users below
void device_streams_release(int device);

// What a shard keeps per reduced-precision scan route (the fp16 copy's, the int8 copy's).  A scan of the route whose
// list overflowed is redone through the f32 scan (redo_overflowed_scan); two such scans in a row and the shard's next
// SCAN_ROUTE_DENIED_SCANS eligible scans skip the route.
constexpr int SCAN_ROUTE_DENIED_SCANS = 256;
struct ScanRouteState {
  std::atomic<int64_t> scans{0}, redone{0};
  std::atomic<int> strikes{0};  // scans in a row whose list overflowed
  std::atomic<int> denied{0};   // eligible scans left that skip the route
  // an eligible scan uses up a denial, if any are left, whatever its band
  bool take_denial() {
    if (denied.load() <= 0) return false;
    denied.fetch_sub(1);
    return true;
  }
};

// One lazily kept reduced-precision copy of the row store (the fp16 copy, the int8 copy): row-major, one allocation.  Kept
// current where a scan is enqueued (row_copy_ensure): rows [0, valid) are converted; appends past the watermark are
// converted in front of the next scan; an overwrite of a stored row, a reallocation of the row store or (fp16) another
// scale reset it to 0.  Tombstones do not touch it.  Guarded by Shard::row_copies_mu under a shared s->mu; appends change
// it under the exclusive lock.
struct RowCopy {
  explicit RowCopy(int mode_) : mode(mode_) {}
  void *d = nullptr;
  int64_t cap = 0, valid = 0, bytes = 0;
  bool denied = false;  // the copy did not fit on the device: its route is off until the row store is reallocated
  std::atomic<int64_t> converted{0};
  ScanRouteState route;  // (overflow: of the fp16 scan's candidate list, the int8 scan's survivor list)
  int mode;  // TSH_OPT_SCAN_F16 / TSH_OPT_SCAN_I8: 0 never, 1 shards larger than the Infinity Cache, 2 every eligible scan
  void release(struct Shard *s);  // the buffer goes, with its bytes, its watermark and its denial
  void overwritten(int64_t first) {  // rows from `first` on were written: a stored row among them and the copy is rebuilt
    if (first < valid) valid = 0;
  }
};
// The fp16 copy: ld halves per row, elements scaled by 2^exp
struct RowCopyF16 : RowCopy {
  using RowCopy::RowCopy;
  int exp = 0;
  int mode_masked = 1;  // TSH_OPT_SCAN_F16_MASKED: the same three for tile scans behind a mask, tombstones, quarantined
                        // rows or gaps (none of them while mode == 0)
};
// The int8 copy: ld biased bytes per row and behind the rows, in the same allocation, a scale per row
struct RowCopyI8 : RowCopy {
  using RowCopy::RowCopy;
#ifndef TSH_SCAN_I8_MASKED_DEFAULT
#define TSH_SCAN_I8_MASKED_DEFAULT 1  // (A/B builds: -DTSH_SCAN_I8_MASKED_DEFAULT=0, like TSH_SCAN_I8_DEFAULT)
#endif
  int mode_masked = TSH_SCAN_I8_MASKED_DEFAULT;  // TSH_OPT_SCAN_I8_MASKED: the same three for tile scans behind a mask, tombstones,
                                                 // quarantined rows or gaps (none of them while mode == 0)
};
// The 4-bit plane (tsh_scan_i4.hip.h): groups x 16 bytes per row, tile-blocked, and behind the rows, in the same
// allocation, rho per row.  Made from the int8 copy.  Its route is denied by the survivors' share, not by overflows:
// two scans in a row that keep more than SCAN_I4_MAX_SHARE of the rows and the shard's next `deny_len` eligible scans take
// the plain int8 route; a denial that follows the previous one's end directly doubles, up to SCAN_I4_DENY_CAP scans.
#ifndef TSH_SCAN_I4_MAX_SHARE
// measured break-even 0.336 less the larger spread's 0.012 (profiles/scan_i4_bench_ab.json; tools/ab_scan_i4.py)
#define TSH_SCAN_I4_MAX_SHARE 0.32  // (A/B builds: -DTSH_SCAN_I4_MAX_SHARE=2.0 never denies)
#endif
#ifndef TSH_SCAN_I4_MIN_BYTES
// auto: row stores above this take the route.  T, W and three more launches are a fixed cost in front of a scan that saves
// bytes: at 768 f32 the route loses at 125 k and 250 k rows (27.6 -> 43.4, 32.3 -> 42.6 us per query), breaks even near
// 410 k and wins at 500 k (1.54 GB: 59.6 -> 53.9) and 1 M (113.9 -> 90.0)
#define TSH_SCAN_I4_MIN_BYTES (1400ll << 20)
#endif
constexpr double SCAN_I4_MAX_SHARE = TSH_SCAN_I4_MAX_SHARE;
constexpr int64_t SCAN_I4_MIN_BYTES = TSH_SCAN_I4_MIN_BYTES;
constexpr int SCAN_I4_DENY_CAP = 1 << 16;
struct RowCopyI4 : RowCopy {
  using RowCopy::RowCopy;
  std::atomic<int64_t> survivors{0};   // rows A left to B, over all scans
  std::atomic<int64_t> denials{0};     // times the route was denied
  std::atomic<int> deny_len{SCAN_ROUTE_DENIED_SCANS};
  std::atomic<bool> probation{false};  // a denial has run out and no scan under the share was seen since: another denial now doubles
  // an eligible scan uses up a denial, if any are left; the one that uses up the last starts the probation
  bool take_denial() {
    if (!route.take_denial()) return false;
    if (route.denied.load() <= 0) probation.store(true);
    return true;
  }
};
inline float *rows4_rho(const RowCopy &c, int groups) {
  return c.d ? reinterpret_cast<float *>(static_cast<uint8_t *>(c.d) + c.cap * groups * 16) : nullptr;
}
inline float *rows8_scales(const RowCopy &c, int64_t ld) {
  return c.d ? reinterpret_cast<float *>(static_cast<uint8_t *>(c.d) + c.cap * ld) : nullptr;
}

struct Shard {
  int device = 0;
  int dim = 0, metric = 0, nch = 0;
  int64_t ld = 0;
  int64_t row_base = 0;  // global id of local row 0
  int64_t rows = 0;      // local rows (next local id)
  int64_t cap = 0;       // allocated rows (multiple of 64)
  float *d_rows = nullptr;
  float *d_inv_norm = nullptr;
  float *d_sqnorm = nullptr;  // |row|^2 (batched L2 key)
  uint64_t *d_live = nullptr;
  IngestStats *d_stats = nullptr;
  bool holds_streams = false;  // counted in its device's DeviceStreams::users
  uint32_t *d_tmp_u32 = nullptr;
  int64_t *d_del_ids = nullptr;  // tsh_index_set_deleted's id buffer, kept between calls
  int64_t del_ids_cap = 0;
  int64_t deleted = 0;
  bool all_live = true;  // every row in [0,rows) is present and not deleted
  float max_norm = 0.f, max_abs = 0.f;
  float min_norm = 0.f;  // smallest |row| seen (0 until rows exist, or when a zero row exists)
  uint32_t nonfinite_rows = 0, tiny_rows = 0;
  // Rows the f32 error model cannot cover (non-finite / > 1e15 elements, tiny cosine norms) are QUARANTINED: their
  // live bit stays clear, so no scan / batch kernel ever offers them, and every search adds their exact sums
  // (quarantine_kernel) to its candidates instead -- a few broken embeddings then do not push every search of
  // the shard onto the rerank-everything path.  Sorted local ids + device copy ([0] = count); changed under the
  // exclusive lock only.  Host-side searches hand the entries to the finaliser as an extra list; shard mode
  // (tsh_search_shard) appends them to the device blocks (quarantine_append_kernel).  More than
  // QUARANTINE_MAX of them fall back to safe mode.
  std::vector<uint32_t> quar_ids;
  uint32_t *d_quar = nullptr;
  uint32_t *d_irr = nullptr;  // 1 + QUARANTINE_MAX: count and ids of the irregular rows of one append
  // a facet call's keys and 64-bit counters (tsh_attr_facets, tsh_tags_facets): 2 |S| + 3 words, grown on demand and kept
  // between calls; facet_mu covers a call's upload, launch and copy back on this shard
  int64_t *d_facet = nullptr;
  int64_t facet_cap = 0;
  std::mutex facet_mu;
  hipStream_t ingest_stream = nullptr;  // all streams below belong to the device's DeviceStreams
  hipStream_t aux_stream = nullptr;
  // every query's scan -> select -> rerank runs on this one in-order stream,
  // back to back; only the small input / result copies use the context streams.
  // (Running a query's tail beside the next query's scan was measured 10-25x
  // slower per tail: each dependent load queues behind the scan's loads.)
  hipStream_t scan_stream = nullptr;
  // small shards, and big ones' scans over the int8 / fp16 copy, alternate between two streams (pick_scan_stream)
  hipStream_t scan_stream2 = nullptr;
  uint64_t scan_seq = 0;  // guarded by scan_mu
  int scan_streams = 0;   // TSH_OPT_SCAN_STREAMS: 0 the rule (scan_two_streams), 1 one stream, 2 two whenever queries overlap
  // When several queries are in flight, a query's select + rerank run here, on
  // CUs the scan stream's CU mask leaves free (2 per XCD), so they overlap the
  // next query's scan without queueing behind its loads on the same CU.
  hipStream_t tail_stream = nullptr, tail_stream2 = nullptr;
  uint64_t tail_seq = 0;  // guarded by scan_mu
  bool cu_split = false;
  hipStream_t batch_stream = nullptr;  // matrix-core batches: compute-bound, so all CUs (no mask)
  hipStream_t upload_stream = nullptr;  // H2D copies of a batched call's inputs (they overlap the call in front)
  std::mutex *scan_mu = nullptr;  // the device's (DeviceStreams): streams are shared by its shards
  DeviceStreams *dstreams = nullptr;
  std::atomic<int> inflight{0};

  RwLock mu;  // search: shared; append/delete: exclusive
  std::mutex ctx_mu;
  std::condition_variable ctx_cv;
  std::vector<std::unique_ptr<Ctx>> ctx_all;
  std::vector<Ctx *> ctx_free;
  std::atomic<uint64_t> mask_epoch_src{1};

  std::atomic<int64_t> c_searches{0}, c_scans{0}, c_batches{0}, c_fallbacks{0}, c_cands{0};
  std::atomic<int64_t> c_plane_fallbacks{0}, c_scan_fallbacks{0};  // batched calls degraded by a full device
  std::atomic<int64_t> c_list_scans{0};  // scans of a compacted row list (selective masks)
  std::atomic<int64_t> c_exact_scans{0};  // searches answered by the exact scan of a few thousand rows (tsh_exact.hip.h)
  int exact_rows = EX_MAX_ROWS;  // TSH_OPT_EXACT_SCAN_ROWS: searches that look at no more rows than this take that path
  bool exact_pick = true;        // TSH_OPT_EXACT_SELECT: the wide pick (exact_pick_kernel) behind the exact scan
  std::atomic<int64_t> c_pick_redone{0};  // picks whose cut bin overflowed the block: finished by exact_select_kernel
  // cursor searches (tsh_search_after_stats): all of them, rows their floor passes sent to the side list, searches redone
  // with a larger side list, searches answered without a floor pass (safe mode, a +inf / NaN cursor)
  std::atomic<int64_t> c_after{0}, c_after_side{0}, c_after_redone{0}, c_after_nofloor{0};
  // counts (tsh_search_count_stats): all of them, rows their window passes sent to the side list, counts redone with a
  // larger side list, counts answered without a window pass on the device
  std::atomic<int64_t> c_count{0}, c_count_side{0}, c_count_redone{0}, c_count_nowindow{0};
  // grouped searches (tsh_search_grouped_stats): all of them, rows their side passes sent to the side list, searches redone
  // with a larger side list, searches answered without the device group passes (safe mode)
  std::atomic<int64_t> c_grouped{0}, c_grouped_side{0}, c_grouped_redone{0}, c_grouped_nodev{0};
  // grouped cursor searches and group counts (tsh_search_grouped_after_stats): the searches, the counts, rows their passes
  // sent to the side list, jobs redone with a larger side list, jobs answered by the exact-all route.  These jobs move
  // none of the counters above
  std::atomic<int64_t> c_gafter{0}, c_gcount{0}, c_gafter_side{0}, c_gafter_redone{0}, c_gafter_all{0};
  // grouped searches with rows per group (tsh_search_grouped_rows_stats): the searches, groups their mark passes marked,
  // member rows sent to the side list, jobs redone with larger lists, jobs answered by the exact-all route.  These jobs
  // move none of the counters above either
  std::atomic<int64_t> c_grows{0}, c_grows_marked{0}, c_grows_side{0}, c_grows_redone{0}, c_grows_all{0};
  int cus = 0;  // compute units of the shard's device (grid of the persistent key kernels)
  std::atomic<int> f16_strikes{0};      // batched calls in a row whose fp16 bands overflowed many candidate lists
  std::atomic<int> f16_denied_calls{0};  // auto key-kernel choice: bf16x3 instead of fp16 for this many more batched calls
  std::atomic<int> planes_denied{0};  // batched calls left that go straight to the f32 kernel (the copy did not fit)
  double scan_us_sum = 0;  // guarded by ctx_mu
  int64_t scan_us_samples = 0;
  int64_t bytes = 0;
  struct BatchCtx *batch = nullptr;  // matrix-core path scratch (created with the shard)
  // A second scratch set: two batched calls (two host threads, or one call per isolate) overlap -- the later one's
  // host preparation runs while the GPU works on the earlier one, whose finalisation runs while the GPU works on
  // the later one.  The GPU side stays one in-order stream: batch_enq_mu covers a call's enqueue sequence and the
  // upkeep of the converted planes.
  struct BatchCtx *batch2 = nullptr;
  std::mutex batch_enq_mu;
  // bf16 (hi, lo) planes of the rows for the bf16x3 batch kernel; built lazily by the first
  // batch search, kept current from split_valid (guarded by batch_enq_mu under a shared s->mu;
  // appends lower split_valid under the exclusive lock)
  u32x4 *d_split = nullptr;
  int64_t split_cap = 0;    // rows allocated
  int64_t split_valid = 0;  // rows [0, split_valid) are converted
  int batch_kernel = 3;     // TSH_OPT_BATCH_KERNEL: 0 f32 MFMA, 1 bf16x3, 2 f16, 3 auto (f16_keys_fit, tsh_batch_plan.h: fp16 unless an L2 shard's norms spread too far)
  // TSH_OPT_BATCH_HUB: the hub rows' bound beside the sample's (fp16 keys, L2 / inner product).  OFF by default: measured
  // on the bench's L2 corpus (norms U(0.5, 2), 1 M x 768, 1024 queries; same box, alternating, tools/r6_hub_ab.sh) it cuts
  // the key passes 1510-1536 -> 1463-1468 us -- the 4096 shortest rows reach |v| <= 0.506, the bound lets ~300 rows per query
  // through where the estimate lets 480 -- and the call as a whole gains nothing (520-530 k against 529-533 k queries/s):
  // sixteen more dense tiles and a second order statistic per query cost what the thinner epilogue saves; inner product
  // and unit-norm rows: no difference; norms U(0.1, 3.2): + 1.8 %.
  bool batch_hub = false;
  std::atomic<int> batch_kernel_last{-1};  // variant the last batched search ran
  int split_mode = 0;       // which kernel the planes were built for (1 / 2); 0 = none
  int64_t split_bytes = 0;
  int split_exp = 0;        // f16 planes: rows were scaled by 2^split_exp
  // TSH_OPT_BATCH_GROUP (default on): the fp16 plane of an L2 / inner-product shard holds its rows by norm inside
  // blocks of PG_ROWS (plane_group_kernel, tsh_batch_f16.hip.h): d_perm[position] = row, d_psq[position] = that row's
  // |v|^2.  Kept current with the plane (same guards); split_grouped = how the plane as built is ordered.
  bool batch_group = true;
  bool split_grouped = false;
  uint32_t *d_perm = nullptr;
  float *d_psq = nullptr;
  int64_t perm_cap = 0, perm_bytes = 0;  // positions allocated
  // The HUB rows of an L2 / inner-product shard (round 6): the few thousand rows whose norm alone puts them near every
  // query -- the shortest (L2) resp. the longest (inner product) --, as a gathered fp16 copy beside the planes.  A batched
  // call scores them densely beside its sample; their k-th smallest key is a PROVEN bound on the k-th key overall
  // (SampleSelArgs::hub_dense).  Built by the first batched call that wants it (guarded by batch_enq_mu like the planes);
  // rows appended later are simply not in it (any subset of the rows gives a valid bound) until they are a quarter of
  // the shard; an overwrite of rows it may hold drops it.
  u32x4 *d_hub = nullptr;
  uint32_t *d_hub_ids = nullptr;  // plane position -> local row id
  float *d_hub_sq = nullptr;      // |v|^2 of the hub rows, in plane order
  int64_t hub_rows_built = -1;    // rows the shard had when it was built (-1: none)
  int hub_n = 0, hub_exp = 0, hub_chunks = 0;
  int64_t hub_bytes = 0;

  // The fp16 copy of the rows that big shards' tile scans, dense or masked, read (scan_f16_kernel), and the int8 copy
  // that their scans, dense or masked, read as a coarse first pass (scan_i8_kernel).  One mutex guards both.
#ifndef TSH_SCAN_I8_DEFAULT
#define TSH_SCAN_I8_DEFAULT 1  // (A/B builds: -DTSH_SCAN_I8_DEFAULT=0, a variant library of its own -- tostore_amd/build.py)
#endif
  RowCopyF16 rows16{1};
  RowCopyI8 rows8{TSH_SCAN_I8_DEFAULT};
#ifndef TSH_SCAN_I4_DEFAULT
#define TSH_SCAN_I4_DEFAULT 1  // (A/B builds: -DTSH_SCAN_I4_DEFAULT=0)
#endif
  RowCopyI4 rows4{TSH_SCAN_I4_DEFAULT};  // TSH_OPT_SCAN_I4: the 4-bit first pass in front of a dense L2 int8 scan
  std::mutex row_copies_mu;
  RowCopy *row_copy(RowStore st) {
    if (st == RowStore::F16) return &rows16;
    return st == RowStore::I8 ? &rows8 : nullptr;
  }

  bool safe_mode() const {
    if (nonfinite_rows) return true;
    if (max_abs > BIG_ABS) return true;
    if (metric == TSH_METRIC_COSINE && tiny_rows) return true;
    return false;
  }
};

// (the copy follows the row store's capacity: built again by the next eligible scan)
void RowCopy::release(Shard *s) {
  if (d) {
    hipFree(d);
    d = nullptr;
    s->bytes -= bytes;
    bytes = 0;
  }
  cap = valid = 0;
  denied = false;
}

// The stream sets live as long as the process -- except the CU-masked streams: left to the runtime's own teardown
// they crash a python host at exit under rocprofv3 (tools/exitcheck.sh: SIGSEGV in __cxa_finalize after the tool
// wrote its output; plain streams are fine).  They are destroyed when the LAST shard on their device is (and made
// again for the next one), so a host that destroys its handles -- every host should -- has none left at exit.  The
// atexit handler only covers leaked handles; it is registered after the first HIP call, so it runs before the
// runtime's exit handlers.  (Round 3: with torch in the process rocprofv3 finalises its tool BEFORE that handler, and
// a HIP call after that aborts -- tools/exitcheck_bench.sh; hence the reference count, which leaves the handler idle.)
static std::mutex g_streams_mu;
static std::map<int, DeviceStreams *> *g_stream_sets = nullptr;  // never freed
static void destroy_masked_streams(DeviceStreams *ds) {  // g_streams_mu held, the device current
  for (hipStream_t *st : {&ds->scan, &ds->scan2, &ds->tail, &ds->tail2})
    if (*st) {
      (void)hipStreamSynchronize(*st);
      (void)hipStreamDestroy(*st);
      *st = nullptr;
    }
  ds->cu_split = false;
}
static void destroy_masked_streams_at_exit() {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  if (!g_stream_sets) return;
  for (auto &kv : *g_stream_sets) {
    DeviceStreams *ds = kv.second;
    if (!ds->cu_split || hipSetDevice(kv.first) != hipSuccess) continue;
    destroy_masked_streams(ds);
  }
}

// the pipeline / tail streams: CU-masked where the device allows it, one plain stream otherwise
static hipError_t make_scan_streams(DeviceStreams *ds) {
  // CU mask bit i = CU slot i/8 of XCD i%8 on MI355X (measured, tools/cumask_probe.hip):
  // bits 0..15 = two CUs of every XCD, reserved for the tails.
  const char *env = probe_env("TSH_NO_CU_SPLIT");
  const int cus = ds->cus;
  if (!(env && env[0] == '1') && cus >= 64 && cus % 32 == 0) {
    std::vector<uint32_t> scan_mask((size_t)cus / 32, 0xFFFFFFFFu), tail_mask((size_t)cus / 32, 0u);
    scan_mask[0] = 0xFFFF0000u;
    tail_mask[0] = 0x0000FFFFu;
    if (hipExtStreamCreateWithCUMask(&ds->scan, (uint32_t)scan_mask.size(), scan_mask.data()) == hipSuccess &&
        hipExtStreamCreateWithCUMask(&ds->scan2, (uint32_t)scan_mask.size(), scan_mask.data()) == hipSuccess &&
        hipExtStreamCreateWithCUMask(&ds->tail, (uint32_t)tail_mask.size(), tail_mask.data()) == hipSuccess &&
        hipExtStreamCreateWithCUMask(&ds->tail2, (uint32_t)tail_mask.size(), tail_mask.data()) == hipSuccess) {
      ds->cu_split = true;
      return hipSuccess;
    }
    if (ds->scan) (void)hipStreamDestroy(ds->scan);
    if (ds->scan2) (void)hipStreamDestroy(ds->scan2);
    if (ds->tail) (void)hipStreamDestroy(ds->tail);
    if (ds->tail2) (void)hipStreamDestroy(ds->tail2);
    ds->scan = ds->scan2 = ds->tail = ds->tail2 = nullptr;
    (void)hipGetLastError();
  }
  return hipStreamCreateWithFlags(&ds->scan, hipStreamNonBlocking);
}

// One more shard on `device`: its stream set (made on first use; the masked streams made again if the last shard
// before this one took them along).  Pair with device_streams_release.
DeviceStreams *device_streams(int device) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  if (!g_stream_sets) {
    g_stream_sets = new std::map<int, DeviceStreams *>();
    atexit(destroy_masked_streams_at_exit);
  }
  std::map<int, DeviceStreams *> &sets = *g_stream_sets;
  auto it = sets.find(device);
  if (it != sets.end()) {
    DeviceStreams *ds = it->second;
    if (ds->rc == TSH_OK && !ds->scan) {
      hipError_t e = hipSetDevice(device);
      if (e == hipSuccess) e = make_scan_streams(ds);
      if (e != hipSuccess) {
        ds->rc = e == hipErrorOutOfMemory ? TSH_E_OOM : TSH_E_HIP;
        ds->err = std::string("hipStreamCreate failed: ") + hipGetErrorString(e);
      }
    }
    if (ds->rc == TSH_OK) ++ds->users;
    return ds;
  }
  DeviceStreams *ds = new DeviceStreams();
  sets[device] = ds;
  auto fail = [&](hipError_t e, const char *what) {
    ds->rc = e == hipErrorOutOfMemory ? TSH_E_OOM : TSH_E_HIP;
    ds->err = std::string(what) + " failed: " + hipGetErrorString(e);
    return ds;
  };
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(e, "hipSetDevice");
  if ((e = hipStreamCreateWithFlags(&ds->ingest, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail(e, "hipGetDeviceProperties");
  ds->cus = prop.multiProcessorCount;
  if ((e = make_scan_streams(ds)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipStreamCreateWithFlags(&ds->batch, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipStreamCreateWithFlags(&ds->aux, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipStreamCreateWithFlags(&ds->upload, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
  ++ds->users;
  return ds;
}

void device_streams_release(int device) {
  std::lock_guard<std::mutex> lk(g_streams_mu);
  if (!g_stream_sets) return;
  auto it = g_stream_sets->find(device);
  if (it == g_stream_sets->end()) return;
  DeviceStreams *ds = it->second;
  if (ds->users > 0 && --ds->users == 0 && ds->cu_split && hipSetDevice(device) == hipSuccess) destroy_masked_streams(ds);
}

int shard_init(Shard *s) {
  HIPCHK(hipSetDevice(s->device));
  DeviceStreams *ds = device_streams(s->device);
  if (ds->rc != TSH_OK) return set_err(ds->rc, "%s", ds->err.c_str());
  s->ingest_stream = ds->ingest;
  s->scan_stream = ds->scan;
  s->scan_stream2 = ds->scan2;
  s->tail_stream = ds->tail;
  s->tail_stream2 = ds->tail2;
  s->batch_stream = ds->batch;
  s->aux_stream = ds->aux;
  s->upload_stream = ds->upload;
  s->cu_split = ds->cu_split;
  s->cus = ds->cus;
  s->scan_mu = &ds->scan_mu;
  s->dstreams = ds;
  s->holds_streams = true;
  HIPCHK(hipMalloc(&s->d_stats, sizeof(IngestStats)));
  HIPCHK(hipMemset(s->d_stats, 0, sizeof(IngestStats)));
  HIPCHK(hipMalloc(&s->d_tmp_u32, 64));
  HIPCHK(hipMalloc(&s->d_quar, (1 + QUARANTINE_MAX) * sizeof(uint32_t)));
  HIPCHK(hipMalloc(&s->d_irr, (1 + QUARANTINE_MAX) * sizeof(uint32_t)));
  HIPCHK(hipMemset(s->d_quar, 0, 4));
  return TSH_OK;
}

int shard_reserve(Shard *s, int64_t want_rows) {
  if (want_rows <= s->cap) return TSH_OK;
  int64_t ncap = std::max<int64_t>(round_up(want_rows, 64), 64);
  if (s->cap > 0) ncap = std::max<int64_t>(ncap, round_up(s->cap + s->cap / 2, 64));
  HIPCHK(hipSetDevice(s->device));
  float *nrows = nullptr, *ninv = nullptr, *nsq = nullptr;
  uint64_t *nlive = nullptr;
  size_t row_bytes = (size_t)ncap * (size_t)s->ld * sizeof(float);
  HIPCHK(hipMalloc(&nrows, row_bytes));
  if (hipMalloc(&ninv, (size_t)ncap * sizeof(float)) != hipSuccess ||
      hipMalloc(&nsq, (size_t)ncap * sizeof(float)) != hipSuccess ||
      hipMalloc(&nlive, (size_t)(ncap / 64) * sizeof(uint64_t)) != hipSuccess) {
    hipFree(nrows);
    if (ninv) hipFree(ninv);
    if (nsq) hipFree(nsq);
    return set_err(TSH_E_OOM, "hipMalloc failed for %lld rows", (long long)ncap);
  }
  hipStream_t st = s->ingest_stream;
  size_t old_bytes = (size_t)s->cap * (size_t)s->ld * sizeof(float);
  if (s->cap > 0) {
    HIPCHK(hipMemcpyAsync(nrows, s->d_rows, old_bytes, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(ninv, s->d_inv_norm, (size_t)s->cap * sizeof(float),
                          hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(nsq, s->d_sqnorm, (size_t)s->cap * sizeof(float), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(nlive, s->d_live, (size_t)(s->cap / 64) * sizeof(uint64_t),
                          hipMemcpyDeviceToDevice, st));
  }
  // rows past the old capacity read as zeros until written (tiles are whole)
  HIPCHK(hipMemsetAsync((char *)nrows + old_bytes, 0, row_bytes - old_bytes, st));
  HIPCHK(hipMemsetAsync(ninv + s->cap, 0, (size_t)(ncap - s->cap) * sizeof(float), st));
  HIPCHK(hipMemsetAsync(nsq + s->cap, 0, (size_t)(ncap - s->cap) * sizeof(float), st));
  HIPCHK(hipMemsetAsync(nlive + s->cap / 64, 0, (size_t)((ncap - s->cap) / 64) * sizeof(uint64_t), st));
  HIPCHK(hipStreamSynchronize(st));
  if (s->d_rows) hipFree(s->d_rows);
  if (s->d_inv_norm) hipFree(s->d_inv_norm);
  if (s->d_sqnorm) hipFree(s->d_sqnorm);
  if (s->d_live) hipFree(s->d_live);
  s->rows16.release(s);
  s->rows8.release(s);
  s->rows4.release(s);
  s->d_rows = nrows;
  s->d_inv_norm = ninv;
  s->d_sqnorm = nsq;
  s->d_live = nlive;
  s->bytes += (int64_t)(row_bytes - old_bytes) + (ncap - s->cap) * 8 + (ncap - s->cap) / 8;
  s->cap = ncap;
  return TSH_OK;
}

// rows [first, first+n) local ids; src host or device
// device copy of the quarantine list; caller holds s->mu exclusively
int quarantine_upload(Shard *s) {
  std::vector<uint32_t> h(1 + s->quar_ids.size());
  h[0] = (uint32_t)s->quar_ids.size();
  std::copy(s->quar_ids.begin(), s->quar_ids.end(), h.begin() + 1);
  HIPCHK(hipMemcpyAsync(s->d_quar, h.data(), h.size() * 4, hipMemcpyHostToDevice, s->ingest_stream));
  HIPCHK(hipStreamSynchronize(s->ingest_stream));
  return TSH_OK;
}

// indices into quar_ids of the quarantined rows a caller's mask lets through (mask_words: the shard's slice,
// bit r = local row r; NULL = all)
void quarantine_select(const Shard *s, const uint64_t *mask_words, std::vector<uint32_t> *sel) {
  sel->clear();
  for (uint32_t i = 0; i < (uint32_t)s->quar_ids.size(); ++i) {
    const uint32_t r = s->quar_ids[i];
    if (!mask_words || ((mask_words[r >> 6] >> (r & 63)) & 1ull)) sel->push_back(i);
  }
}

int shard_append(Shard *s, int64_t first, int64_t n, const float *src, bool src_is_device) {
  if (n <= 0) return TSH_OK;
  int rc = shard_reserve(s, first + n);
  if (rc) return rc;
  HIPCHK(hipSetDevice(s->device));
  hipStream_t st = s->ingest_stream;
  float *dst = s->d_rows + first * s->ld;
  hipMemcpyKind kind = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (s->ld == s->dim) {
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)n * s->dim * sizeof(float), kind, st));
  } else {
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)s->ld * sizeof(float), src, (size_t)s->dim * sizeof(float),
                            (size_t)s->dim * sizeof(float), (size_t)n, kind, st));
  }
  // quarantine: rows of [first, first + n) are replaced, so their old entries go; the kernel lists the new ones
  uint32_t irr_cap = 0;
  bool quar_dirty = false;
  {
    auto lo = std::lower_bound(s->quar_ids.begin(), s->quar_ids.end(), (uint32_t)first);
    auto hi = std::lower_bound(lo, s->quar_ids.end(), (uint32_t)std::min<int64_t>(first + n, 0xFFFFFFFFll));
    if (lo != hi) {
      s->quar_ids.erase(lo, hi);
      quar_dirty = true;
    }
    irr_cap = QUARANTINE_MAX - (uint32_t)s->quar_ids.size();
    HIPCHK(hipMemsetAsync(s->d_irr, 0, 4, st));
  }
  int blocks = (int)std::min<int64_t>((n + 3) / 4, 2048);
  ingest_kernel<<<blocks, 256, 0, st>>>(s->d_rows, s->ld, s->dim, first, n, s->d_inv_norm, s->d_sqnorm, s->d_stats,
                                        s->d_irr, irr_cap,
                                        s->metric == TSH_METRIC_COSINE ? 1 : 0);
  int lb = (int)std::min<int64_t>(((first + n - 1) / 64 - first / 64 + 1 + 255) / 256, 1024);
  live_range_kernel<<<lb, 256, 0, st>>>(s->d_live, first, n, 1);
  IngestStats hs;
  uint32_t n_irr = 0;
  HIPCHK(hipMemcpyAsync(&hs, s->d_stats, sizeof hs, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&n_irr, s->d_irr, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  n_irr = std::min(n_irr, irr_cap);
  if (n_irr) {
    std::vector<uint32_t> ids(n_irr);
    live_clear_u32_kernel<<<(n_irr + 255) / 256, 256, 0, st>>>(s->d_live, s->d_irr + 1, n_irr);
    HIPCHK(hipMemcpyAsync(ids.data(), s->d_irr + 1, (size_t)n_irr * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->quar_ids.insert(s->quar_ids.end(), ids.begin(), ids.end());
    std::sort(s->quar_ids.begin(), s->quar_ids.end());
    s->all_live = false;
    quar_dirty = true;
  }
  if (quar_dirty) {
    rc = quarantine_upload(s);
    if (rc) return rc;
  }
  uint32_t mb = hs.max_norm_bits, ab = hs.max_abs_bits;
  memcpy(&s->max_norm, &mb, 4);
  memcpy(&s->max_abs, &ab, 4);
  s->nonfinite_rows = hs.nonfinite_rows;
  s->tiny_rows = hs.tiny_rows;
  {
    uint32_t nb = hs.inv_min_norm_bits ? ~hs.inv_min_norm_bits : 0u;
    memcpy(&s->min_norm, &nb, 4);
  }
  if (first > s->rows) s->all_live = false;  // gap of absent rows
  if (first + n > s->rows) s->rows = first + n;
  s->split_valid = std::min(s->split_valid, first);  // overwritten / new rows need re-splitting
  s->rows16.overwritten(first);
  s->rows8.overwritten(first);
  s->rows4.overwritten(first);
  if (first < s->hub_rows_built) s->hub_rows_built = -1;  // (an overwritten row may be a hub row: its copy is stale)
  return TSH_OK;
}

void ctx_free_all(Ctx *c) {
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->ev_done) hipEventDestroy(c->ev_done);
  if (c->ev_scanned) hipEventDestroy(c->ev_scanned);
  hipFree(c->d_query);
  hipHostFree(c->h_query);
  hipFree(c->d_mask);
  hipHostFree(c->h_mask);
  hipFree(c->d_list);
  hipHostFree(c->h_list);
  hipFree(c->d_keys);
  hipFree(c->d_gmin);
  hipFree(c->d_hist);
  hipFree(c->d_block);
  hipHostFree(c->h_block);
  hipHostFree(c->h_quar);
  hipFree(c->d_cand);
  hipFree(c->d_big_rows);
  hipFree(c->d_big_entries);
  hipFree(c->d_big_count);
  hipFree(c->d_xkey);
  hipFree(c->d_xsum);
  hipFree(c->d_xpick);
  hipFree(c->d_i8);
  hipFree(c->d_i8_list);
  hipFree(c->d_i4_keys);
  hipFree(c->d_i4_gmin);
  hipFree(c->d_i4_ctl);
  hipFree(c->d_i4_mask);
  hipHostFree(c->h_i4);
  hipFree(c->d_side_rows);
  hipFree(c->d_side_cnt);
  hipHostFree(c->h_side);
  hipFree(c->d_heads);
  hipFree(c->d_hmin);
  hipFree(c->d_gm);
  hipFree(c->d_gr_ctl);
  hipFree(c->d_gr_seg);
}

int ctx_prepare(Shard *s, Ctx *c, int32_t entries, bool need_mask) {
  HIPCHK(hipSetDevice(s->device));
  if (!c->ev0) {
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    HIPCHK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming | (blocking_wait() ? hipEventBlockingSync : 0)));
    HIPCHK(hipEventCreateWithFlags(&c->ev_scanned, hipEventDisableTiming));
    HIPCHK(hipMalloc(&c->d_query, (size_t)s->ld * sizeof(float)));
    HIPCHK(hipHostMalloc(&c->h_query, (size_t)s->ld * sizeof(float), hipHostMallocDefault));
    HIPCHK(hipMalloc(&c->d_big_count, 64));
    c->bytes += s->ld * 4;
  }
  int64_t tiles = s->cap / 64;
  if (tiles > c->tiles_cap) {
    hipFree(c->d_keys);
    hipFree(c->d_gmin);
    c->d_keys = nullptr;
    c->d_gmin = nullptr;
    HIPCHK(hipMalloc(&c->d_keys, (size_t)tiles * 64 * sizeof(uint32_t)));
    // (two minima per tile: the coarse int8 scan leaves its tiles' minima of lower sides behind the n_tiles upper ones)
    HIPCHK(hipMalloc(&c->d_gmin, (size_t)tiles * 2 * sizeof(uint32_t)));
    c->bytes += (tiles - c->tiles_cap) * 66 * 4;
    c->tiles_cap = tiles;
  }
  if (need_mask && tiles > c->mask_words) {
    hipFree(c->d_mask);
    hipHostFree(c->h_mask);
    c->d_mask = nullptr;
    c->h_mask = nullptr;
    HIPCHK(hipMalloc(&c->d_mask, (size_t)tiles * 8));
    HIPCHK(hipHostMalloc(&c->h_mask, (size_t)tiles * 8, hipHostMallocDefault));
    c->bytes += (tiles - c->mask_words) * 8;
    c->mask_words = tiles;
    c->mask_epoch = 0;
  }
  if (entries > c->entries_cap) {
    hipFree(c->d_block);
    hipHostFree(c->h_block);
    hipFree(c->d_cand);
    c->d_block = nullptr;
    c->h_block = nullptr;
    c->d_cand = nullptr;
    size_t bb = (size_t)tsh_candidate_block_bytes(entries);
    HIPCHK(hipMalloc(&c->d_block, bb));
    HIPCHK(hipHostMalloc(&c->h_block, bb, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_block_dev), c->h_block, 0));
    HIPCHK(hipMalloc(&c->d_cand, (size_t)entries * sizeof(uint32_t)));
    c->bytes += (int64_t)(bb + 4 * (size_t)entries);
    c->entries_cap = entries;
  }
  return TSH_OK;
}

Ctx *ctx_acquire(Shard *s, bool block) {
  std::unique_lock<std::mutex> lk(s->ctx_mu);
  for (;;) {
    if (!s->ctx_free.empty()) {
      Ctx *c = s->ctx_free.back();
      s->ctx_free.pop_back();
      return c;
    }
    if ((int)s->ctx_all.size() < MAX_CTX) {
      s->ctx_all.emplace_back(new Ctx());
      return s->ctx_all.back().get();
    }
    if (!block) return nullptr;
    s->ctx_cv.wait(lk);
  }
}
void ctx_release(Shard *s, Ctx *c) {
  if (s->dstreams) {  // whatever the device still books under this context's events is over (or given up)
    std::lock_guard<std::mutex> lk(*s->scan_mu);
    std::vector<DeviceStreams::ScanOut> &so = s->dstreams->scan_out;
    for (size_t i = 0; i < so.size();)
      if (so[i].owner == c) {
        s->dstreams->scans_out[so[i].which]--;
        so[i] = so.back();
        so.pop_back();
      } else {
        ++i;
      }
  }
  {
    std::lock_guard<std::mutex> lk(s->ctx_mu);
    s->ctx_free.push_back(c);
  }
  s->ctx_cv.notify_one();
}

// error band of the f32 ranking key (DESIGN.md "error model")
struct Band {
  float eps_rel = 0.f, delta_abs = 0.f;
  int force_all = 0;
};
Band compute_band(const Shard *s, const float *q) {
  Band b;
  if (s->safe_mode()) {
    b.force_all = 1;
    return b;
  }
  double qn2 = 0;
  for (int i = 0; i < s->dim; ++i) {
    float a = std::fabs(q[i]);
    if (!(a <= BIG_ABS)) {
      b.force_all = 1;  // inf / nan / huge query element
      return b;
    }
    qn2 += (double)q[i] * (double)q[i];
  }
  double qn = std::sqrt(qn2) * (1.0 + 1e-6);
  const double u2 = 1.1920928955078125e-07;  // 2^-23 = 2 * unit roundoff (safety factor 2)
  if (s->metric == TSH_METRIC_L2) {
    double eps = (4.0 * s->nch + 8.0) * u2;
    b.eps_rel = (float)(3.0 * eps);
    b.delta_abs = (float)((double)s->dim * 7.9e-31);  // d * 2^-100: underflow slack
  } else if (s->metric == TSH_METRIC_IP) {
    double gam = (4.0 * s->nch + 6.0) * u2;
    double delta = gam * qn * (double)s->max_norm * (1.0 + 1e-6) + (double)s->dim * 7.5e-37;
    b.delta_abs = (float)(2.0 * delta * 1.0001);
    if (!(b.delta_abs < 3.0e38f)) b.force_all = 1;
  } else {
    double gam = (4.0 * s->nch + 6.0) * u2;
    double delta = qn * (gam + 4.76837158203125e-07 /*2^-21*/) + (double)s->dim * 7.5e-37;
    b.delta_abs = (float)(2.0 * delta * 1.0001);
  }
  return b;
}

// d_mask: the caller's mask words on the device, or NULL; d_list: the rows to scan as a list of list_padded ids on the
// device, or NULL (the shard's tiles)
void fill_scan_args(const Shard *s, const Ctx *c, const uint64_t *d_mask, const uint32_t *d_list, int32_t list_padded, ScanArgsQ *aq) {
  ScanArgs *a = &aq->a;
  a->rows = s->d_rows;
  a->query = c->d_query;
  a->query_out = nullptr;
  a->inv_norm = s->d_inv_norm;
  a->live = s->d_live;
  a->mask = d_mask;
  a->keys = c->d_keys;
  a->gmin = c->d_gmin;
  a->ld = s->ld;
  a->n = s->rows;
  a->d4 = (int32_t)(s->ld / 4);
  a->n_tiles = d_list ? list_padded / 64 : (int32_t)((s->rows + 63) / 64);
  a->list = d_list;
  a->rows16 = nullptr;
  a->sqnorm = nullptr;
  a->inv_scale = a->w_alpha = a->w_beta = 0.f;
  a->pad_ = 0;
  a->scale8 = nullptr;
  a->w_s = 0.f;
  a->pad2_ = 0;
}

// slice the caller's GLOBAL keep mask into this shard's tile words (tsh_host_sync.h: no bit past the last row is kept)
inline void slice_mask(const Shard *s, const uint8_t *mask, uint64_t *out_words, int64_t n_words) {
  tsh::slice_mask(s->row_base, s->rows, mask, out_words, n_words);
}

// Which kernels answer one query on one shard (choose_route)
struct Route {
  bool use_list = false;  // the scan reads the mask's list of kept rows, not the shard's tiles
  int64_t n_exam = 0;     // rows (list: entries, padding included) the scan looks at
  bool exact = false;     // exact_scan_kernel + exact_select_kernel: the block is final, no f32 keys exist
  bool picked = false;    // ... + exact_pick_kernel instead of exact_select_kernel
  Band band;              // the f32 keys' error band (zero on the exact path)
  bool f16_eligible = false;  // the fp16 scan may run (the caller still owes the denial counter and rows16_ensure) ...
  int v_exp = 0;              // ... over a copy of this scale, its keys inside this band
  ScanF16Band fb;
  bool i8_eligible = false;  // the coarse int8 scan + the exact path over its survivors may run (the caller still owes
  ScanI8Band ib;             // the denial counter and rows8_ensure); `picked`: E2' behind it instead of E2
  bool i4_eligible = false;  // ... with the 4-bit pass in front of it (dense L2 only; the caller owes its denial counter,
  ScanI4Band i4b;            // rows4_ensure and the context's buffers)
};

// A selective caller mask as a list: local ids of the kept rows, ascending, padded with 0xFFFFFFFF to whole tiles of
// 64.  Made once per call (shard_search_blocks) and shared by the call's queries; nullptr = scan by tiles.
struct RowList {
  const uint32_t *ids = nullptr;    // on the host: every context of the call uploads it once ...
  const uint32_t *d_ids = nullptr;  // ... or resident on the device (a mask handle's, compacted there): read in place
  int32_t padded = 0;  // entries incl. padding (multiple of 64)
};

// A device buffer of the handles' parts that grows and never shrinks (BatchBuf's idiom, tsh_host_batch.inl.h).  The
// current device is the buffer's.  A failed allocation leaves d NULL and cap 0
template <typename T>
struct DevBuf {
  T *d = nullptr;
  int64_t cap = 0;  // entries
  // room for `want` entries: a buffer too small is replaced (never copied) by one of want + slack entries rounded up to
  // round_to, slack = want / 8 unless given.  *bytes follows what is held
  int reserve(int64_t want, int64_t round_to, int64_t *bytes = nullptr, int64_t slack = -1) {
    if (want <= cap) return TSH_OK;
    const int64_t held = cap;
    free();
    if (bytes) *bytes -= held * (int64_t)sizeof(T);
    const int64_t grown = round_up(want + (slack < 0 ? want / 8 : slack), round_to);
    HIPCHK(hipMalloc(&d, (size_t)grown * sizeof(T)));
    cap = grown;
    if (bytes) *bytes += grown * (int64_t)sizeof(T);
    return TSH_OK;
  }
  void free() {
    hipFree(d);
    d = nullptr;
    cap = 0;
  }
};

// ---- mask handles (tsh_mask_create, include/tostore_hip.h): one shard's part ------------------------------------
// The caller's bitmap sliced to this shard's rows, as the kernels read it (word t bit r = local row 64 t + r), on
// the host (the quarantined rows are matched against it there; the batched path places its sample window by it) and
// on the device (dense masked scans, the batched epilogue); and, when the mask is selective, the ascending list of
// its kept rows -- compacted on the device (tsh_mask.hip.h), never on the host.  Built for the rows the shard had at
// the time; a search that finds the shard grown rebuilds it first (current_part).
struct MaskPart {
  int device = 0;
  std::atomic<int64_t> built_rows{-1};  // rows of the shard the part was built for (-1: not built)
  int32_t n_tiles = 0;
  int64_t kept = 0;                // set bits (tombstones not subtracted)
  std::vector<uint64_t> h_words;   // n_tiles words
  std::vector<int32_t> pre;        // pre[t] = kept rows in words [0, t): n_tiles + 1 entries
  DevBuf<uint64_t> words;
  DevBuf<uint32_t> list;           // kept rows' local ids, ascending, padded with 0xFFFFFFFF to a multiple of 64
  int32_t list_padded = 0;         // 0: no list (the mask keeps too many rows for one to pay, or none)
  DevBuf<uint32_t> bsum;           // M1's per-workgroup counts + one word for M2's total
  int64_t bytes = 0;               // device bytes held
  void free_bufs() {
    words.free();
    list.free();
    bsum.free();
    bytes = 0;
  }
};
// the mask of a search, as the shard-level functions take it
struct MaskSrc {
  const uint8_t *bytes = nullptr;  // the caller's GLOBAL bitmap (pointer form: sliced, counted, listed per call) ...
  const MaskPart *part = nullptr;  // ... or this shard's part of a mask handle (resident)
  MaskSrc() {}
  MaskSrc(const uint8_t *b) : bytes(b) {}  // NOLINT: the pointer form converts where a mask is passed on
  explicit MaskSrc(const MaskPart *p) : part(p) {}
  explicit operator bool() const { return bytes != nullptr || part != nullptr; }
};
// ... and as one shard's scans read it: what resolve_mask makes of a MaskSrc, once per call
struct ShardMask {
  const uint64_t *words = nullptr;  // this shard's slice on the host (the caller's scratch, or a handle's part); NULL: no mask
  uint64_t epoch = 0;               // names a sliced pointer mask, so that a context uploads it once per call
  int64_t rows_est = 0;             // rows the scan will actually read (the mask's popcount, at least 1); 0: all of them
  RowList list;                     // a selective mask's kept rows
  const MaskPart *part = nullptr;   // a handle's: its device words and list are read in place, nothing is copied or uploaded
  bool listed() const { return list.ids || list.d_ids; }
};

// ---- groups handles (tsh_groups_create, include/tostore_hip.h): one shard's part ---------------------------------------
// The caller's group array sliced to this shard's rows on the device: entry r = the group of local row r, for the rows
// the shard had when the part was built (rows beyond the caller's array: -1).  A search that finds the shard grown, or
// the array changed by tsh_groups_set (built_rows = -1), rebuilds it first (current_part).
struct GroupPart {
  int device = 0;
  std::atomic<int64_t> built_rows{-1};
  DevBuf<int32_t> group;
  int32_t n_groups = 0;
  void free_bufs() { group.free(); }
};

// ---- attribute handles (tsh_attr_create, include/tostore_hip.h): one shard's part --------------------------------------
// The caller's column sliced to this shard's rows on the device: entry r = the value of local row r, for the rows the
// shard had when the part was built (rows beyond the caller's array: TSH_ATTR_NULL).  A mask made from the handle
// (tsh_mask_create_range) that finds the shard grown, or the array changed by tsh_attr_set (built_rows = -1), rebuilds
// it first (current_part).  8 B per row.
struct AttrPart {
  int device = 0;
  std::atomic<int64_t> built_rows{-1};
  DevBuf<int64_t> vals;
  void free_bufs() { vals.free(); }
};

// ---- tag handles (tsh_tags_create, include/tostore_hip.h): one shard's part --------------------------------------------
// The handle's normalised CSR sliced to this shard's rows on the device (tsh_tags_plan.h, tags_slice): rows + 1 32-bit
// offsets rebased to the slice's first value, the values, and the valid words (bit r of word t: local row 64 t + r
// exists in the column and is not NULL), for the rows the shard had when the part was built.  A mask made from the
// handle (tsh_mask_create_tags) that finds the shard grown, or the column changed by tsh_tags_set (built_rows = -1),
// rebuilds it first (current_part).  4 B per row + 8 B per value + 8 B per 64 rows.
struct TagsPart {
  int device = 0;
  std::atomic<int64_t> built_rows{-1};
  DevBuf<uint32_t> off;
  DevBuf<int64_t> vals;
  DevBuf<uint64_t> valid;
  void free_bufs() {
    off.free();
    vals.free();
    valid.free();
  }
};

// One query in flight on one context.  Its three kernels (scan, select,
// rerank) are enqueued back to back on the shard's single in-order pipeline
// stream with NO copy and NO cross-stream dependency between them: the query
// rides in the scan kernel's argument segment, the result block is stored
// straight into pinned host memory, completion is one event.
struct Job {
  Ctx *c = nullptr;
  int32_t k = 0, entries = 0;
  bool masked = false, user_mask = false;
  uint8_t *dev_target = nullptr;  // shard mode: caller's device block (header + entries land there)
  bool timed = false;             // ev0/ev1 bracket this job's scan kernel
  bool counted = false;           // contributes to Shard::inflight
  Route route;  // the kernels it was enqueued with; its band is also the fallback's own threshold.  (A list scan leaves
                // the context's keys / gmin in list order, route.n_exam of them)
  bool up_mask = false, up_list = false;  // staged in the context's pinned buffers: copied to the device in front of the scan
  const uint64_t *d_mask = nullptr;  // the caller's mask words on the device: the context's copy, or a mask handle's
  const uint32_t *d_list = nullptr;  // the scanned list on the device: the context's copy, or a mask handle's
  ExactSelArgs xsel{};     // the exact path: a pick whose cut bin was too full for the block is finished by
                           // exact_select_kernel on the same keys (these arguments), job_finish
  bool leave_overflow = false;  // shard mode under TSH_OPT_EXCHANGE_AHEAD: an exchange enqueued behind this job's kernels
                                // may be reading the device block when the host looks at it -- a block whose list
                                // overflowed is then NOT rewritten by the wide-band pass (a peer could gather a new
                                // header over old entries); it keeps FLAG_LIST_OVERFLOW, which every rank answers by
                                // redoing the group with larger blocks, not ahead
  bool no_i8 = false;  // enqueued as the redo of an int8 scan (JobReq::no_i8): a further redo stays off that route
  bool i4 = false;     // store == I8 and the 4-bit pass ran in front of the int8 scan, which then read rows behind its mask
  RowStore store = RowStore::F32;  // the copy of the rows its tile scan read (I8: survivors through the exact path).
                                   // A list overflow of an F16 / I8 scan is redone through another scan (redo_overflowed_scan),
  std::vector<float> redo_q;  // from this copy of the query, with this tag
  uint32_t tag = 0;
  ShardMask redo_mask;     // ... behind the same mask: a handle's part, or the context's own copy of a pointer mask's words
                           // (job_enqueue: the caller's slice may be gone when a ticket is waited for)
  hipStream_t last_stream = nullptr;  // where the job's last kernel was enqueued (ev_done rides on it)
  uint64_t enq_seq = 0;               // ... and its place in the device's enqueue order (DeviceStreams::enq_counter)
  std::vector<uint32_t> quar_sel;  // entries of c->h_quar that belong to this query's candidates
  // a cursor job (JobReq::after): its floor in the scan's key space (floored: the floor pass and the side re-rank run;
  // not in safe mode, not "from the start"), or no scan at all (after_skip: a +inf / NaN cursor, which only quarantined
  // rows can follow).  Redone once with a larger side list if that overflowed -- from redo_query / redo_mask
  bool has_after = false, floored = false, after_skip = false, after_redone = false;
  Cursor after;
  AfterFloor floor;
  int side_word = 0;  // which of the context's two count words this job counts in
  // a count job (JobReq::count): no select, no re-rank, no block.  windowed: the window pass and the side re-rank run
  // (tsh_count.hip.h; not in safe mode, where the job is a plain search whose wide-band pass hands every live row's exact
  // sums to the finaliser); after_skip: no row inside the model can count (CountWindow::skip), no scan runs.  A windowed
  // job leaves the rows it counted on the device in `certain` and a side list like a cursor job's, redone the same way
  bool counting = false, windowed = false;
  double count_thr = 0;
  CountWindow window;
  int64_t certain = 0;
  // a grouped job (JobReq::groups): the group passes run around select and re-rank (grouped; tsh_group.hip.h) and leave a
  // side list like a cursor job's, redone the same way -- or, in safe mode, a plain search job whose every live row
  // reaches the finaliser (grouping without grouped)
  bool grouping = false, grouped = false;
  const GroupPart *gpart = nullptr;
  // a grouped cursor search or a group count (JobReq::group_after; tsh_group_after_rule.h): grouped and floored, or grouped
  // and windowed -- G1, then the passes with the floor resp. the window pass in the places of G2 / G3 resp. select and
  // re-rank.  exact_all: the rule does not hold for this call (JobReq::exact_all): a plain search job whose every live
  // row reaches the finaliser, as in safe mode
  bool group_after = false, exact_all = false;
  // a grouped search with several rows per group (JobReq::group_rows, the rows per group; tsh_group_rows_rule.h): a grouped
  // job whose G3 gives way to the mark, member and pick passes (tsh_group_rows.hip.h).  rows_redone: it runs for the
  // second time, with larger lists or on the exact-all route
  int32_t group_rows = 0;
  bool rows_redone = false;
  // shard mode: the side rows' entries were appended to the caller's device block (A2', tsh_after.hip.h) -- a cursor job's
  // and a plain grouped job's (tsh_search_shard_after, tsh_search_shard_grouped); nothing of them reaches the host lists
  bool side_in_block() const { return dev_target && ((floored && !grouped) || (grouped && !floored && !windowed && group_rows == 0)); }
  const float *redo_query = nullptr;  // the caller's query (a ticket's own copy): valid until the job is finished
  std::vector<uint64_t> redo_words;   // a ticket's copy of a pointer mask's words (JobReq::mask_dies), else empty
};

void launch_select(const SelectArgs &se, int32_t n_tiles, hipStream_t st) {
  // (which of the three, and why: select_variant, tsh_select_plan.h)
  switch (select_variant(n_tiles, se.k, se.list != nullptr)) {
    case SEL_NT256_REGS: select_kernel<SEL_THREADS_SMALL, true><<<1, SEL_THREADS_SMALL, 0, st>>>(se); break;
    case SEL_NT1024_REGS: select_kernel<SEL_THREADS, true><<<1, SEL_THREADS, 0, st>>>(se); break;
    case SEL_NT1024_MEM: select_kernel<SEL_THREADS, false><<<1, SEL_THREADS, 0, st>>>(se); break;
  }
}

// host mode: the quarantined rows' sums go to the context's pinned h_quar (the host picks the query's: Job::quar_sel)
void launch_quarantine(Shard *s, Ctx *c, hipStream_t st) {
  QuarArgs qa{};
  qa.rows = s->d_rows;
  qa.Q = c->d_query;
  qa.list = s->d_quar;
  qa.out = c->h_quar_dev;
  qa.ld = s->ld;
  qa.ldq = s->ld;
  qa.row_base = s->row_base;
  qa.dim = s->dim;
  qa.cap = (int32_t)QUARANTINE_MAX;
  qa.metric = s->metric;
  quarantine_kernel<<<dim3((unsigned)((s->quar_ids.size() + 63) / 64), 1), 64, 0, st>>>(qa);
}
// shard mode: the quarantined rows go into the job's device block
void launch_quarantine_append(Shard *s, Ctx *c, Job *j, hipStream_t st) {
  QuarAppendArgs qa{};
  qa.rows = s->d_rows;
  qa.Q = c->d_query;
  qa.list = s->d_quar;
  qa.mask = j->user_mask ? j->d_mask : nullptr;
  qa.blocks = j->dev_target;
  qa.ld = s->ld;
  qa.ldq = s->ld;
  qa.row_base = s->row_base;
  qa.block_bytes = 0;
  qa.dim = s->dim;
  qa.entries = j->entries;
  qa.metric = s->metric;
  quarantine_append_kernel<<<dim3((unsigned)((s->quar_ids.size() + 63) / 64), 1), 64, 0, st>>>(qa);
}

int ctx_reserve_list(Ctx *c, int64_t padded) {
  if (padded <= c->list_cap) return TSH_OK;
  hipFree(c->d_list);
  hipHostFree(c->h_list);
  c->d_list = c->h_list = c->h_list_dev = nullptr;
  c->bytes -= c->list_cap * 4;
  c->list_cap = 0;
  c->list_epoch = 0;
  const int64_t want = round_up(padded + padded / 2, 4096);
  HIPCHK(hipMalloc(&c->d_list, (size_t)want * sizeof(uint32_t)));
  HIPCHK(hipHostMalloc(&c->h_list, (size_t)want * sizeof(uint32_t), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_list_dev), c->h_list, 0));
  c->list_cap = want;
  c->bytes += want * 4;
  return TSH_OK;
}

// the side list of a cursor job (tsh_after.hip.h): room for `want` undecided rows
int ctx_reserve_side(Ctx *c, int64_t want) {
  if (!c->d_side_cnt) {
    HIPCHK(hipMalloc(&c->d_side_cnt, 3 * sizeof(uint32_t)));
    c->side_dirty = true;
  }
  if (want <= c->side_cap) return TSH_OK;
  hipFree(c->d_side_rows);
  hipHostFree(c->h_side);
  c->d_side_rows = nullptr;
  c->h_side = c->h_side_dev = nullptr;
  c->bytes -= c->side_cap * 4;
  c->side_cap = 0;
  HIPCHK(hipMalloc(&c->d_side_rows, (size_t)want * sizeof(uint32_t)));
  HIPCHK(hipHostMalloc(&c->h_side, (size_t)(want + 1) * sizeof(BlockEntry), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_side_dev), c->h_side, 0));
  c->side_cap = want;
  c->bytes += want * 4;
  return TSH_OK;
}

// what a grouped job adds to its context (tsh_group.hip.h): the heads array and its minima, as many tiles as the context's
// keys have, and a head table of n_groups words
int ctx_reserve_group(Ctx *c, int64_t n_groups) {
  if (c->tiles_cap > c->heads_tiles) {
    hipFree(c->d_heads);
    hipFree(c->d_hmin);
    c->d_heads = c->d_hmin = nullptr;
    c->bytes -= c->heads_tiles * 65 * 4;
    c->heads_tiles = 0;
    HIPCHK(hipMalloc(&c->d_heads, (size_t)c->tiles_cap * 64 * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&c->d_hmin, (size_t)c->tiles_cap * sizeof(uint32_t)));
    c->heads_tiles = c->tiles_cap;
    c->bytes += c->heads_tiles * 65 * 4;
  }
  if (n_groups > c->gm_cap) {
    hipFree(c->d_gm);
    c->d_gm = nullptr;
    c->bytes -= c->gm_cap * 8;
    c->gm_cap = 0;
    const int64_t want = round_up(n_groups + n_groups / 8, 1024);
    HIPCHK(hipMalloc(&c->d_gm, (size_t)want * 8));
    c->gm_cap = want;
    c->bytes += want * 8;
  }
  return TSH_OK;
}

// what a grouped job with rows per group adds on top (tsh_group_rows.hip.h): `slots` slots and segment space for
// `seg_want` member rows
constexpr int64_t GROUP_ROWS_SEG_CAP = 8192;  // member rows a context's segments hold before a job is redone with more
int ctx_reserve_group_rows(Ctx *c, int64_t slots, int64_t seg_want) {
  if (slots > c->gr_slots) {
    hipFree(c->d_gr_ctl);
    c->d_gr_ctl = nullptr;
    c->bytes -= c->gr_slots * 12;
    c->gr_slots = 0;
    const int64_t want = round_up(slots, 256);
    HIPCHK(hipMalloc(&c->d_gr_ctl, (size_t)(GROUP_ROWS_CTL + 3 * want) * sizeof(uint32_t)));
    c->gr_slots = want;
    c->bytes += want * 12;
  }
  seg_want = std::max(seg_want, GROUP_ROWS_SEG_CAP);
  if (seg_want > c->gr_seg_cap) {
    hipFree(c->d_gr_seg);
    c->d_gr_seg = nullptr;
    c->bytes -= c->gr_seg_cap * 8;
    c->gr_seg_cap = 0;
    HIPCHK(hipMalloc(&c->d_gr_seg, (size_t)seg_want * 8));
    c->gr_seg_cap = seg_want;
    c->bytes += seg_want * 8;
  }
  return TSH_OK;
}

// A search with at most TSH_OPT_EXACT_SCAN_ROWS rows to look at takes the exact path (tsh_exact.hip.h); its block must
// have room for the k rows it will hold
bool exact_applies(const Shard *s, int64_t n_exam, int32_t k, int32_t entries) {
  return n_exam > 0 && n_exam <= std::min<int64_t>(s->exact_rows, EX_MAX_ROWS) && k <= entries;
}
// (list_mask_bits / popcount_words: tsh_host_sync.h -- pure host functions, tested on the CPU)
// A selective mask (a WHERE clause that keeps a few percent of the rows) is scanned as a LIST of row ids: scan_list_kernel
// gathers the kept rows, eight per wave, instead of walking tiles that are mostly dead (tsh_kernels.hip.h).  The list
// pays below one kept row in list_div (tools/r4_list_probe.sh); TSH_LIST_DIV=0 switches it off.  -> ids filled (padded
// with 0xFFFFFFFF to whole tiles) and true when the scan should use them.
inline int64_t mask_list_div() {
  static const int64_t v = probe_env("TSH_LIST_DIV") ? atoll(probe_env("TSH_LIST_DIV")) : 24;
  return v;
}
// does a search with this many kept rows scan them as a list?  (the rule of both forms of a mask: pointer and handle)
bool row_list_pays(const Shard *s, int64_t rows_kept, int32_t k, int32_t entries) {
  const int64_t list_div = mask_list_div();
  if (list_div <= 0 || s->rows < 4096 || rows_kept <= 0) return false;
  // few enough kept rows for the exact path (tsh_exact.hip.h): their list is all that search reads, at any row width
  // and any selectivity (a shard small enough for that path whole needs no list: it tests the mask row by row)
  const bool by_exact = !exact_applies(s, s->rows, k, entries) && exact_applies(s, round_up(rows_kept, 64), k, entries);
  return by_exact || (rows_kept * list_div <= s->rows && scan_list_supported(s->nch, s->ld));
}
bool build_row_list(const Shard *s, const uint64_t *mask_words, int32_t n_tiles, int64_t rows_kept, int32_t k, int32_t entries,
                    std::vector<uint32_t> *ids) {
  if (!mask_words || !row_list_pays(s, rows_kept, k, entries)) return false;
  // (mask_words come from slice_mask, which clears every bit at or past the shard's last row: the list names rows of
  // the shard only, and rows_kept -- their popcount -- is its exact length)
  ids->resize((size_t)round_up(rows_kept, 64) + 8);
  const size_t got = list_mask_bits(mask_words, n_tiles, rows_kept, ids->data());
  if (got == 0) return false;
  const size_t padded = (size_t)round_up((int64_t)got, 64);
  for (size_t i = got; i < padded; ++i) (*ids)[i] = 0xFFFFFFFFu;
  ids->resize(padded);
  return true;
}
// The per-call work on a search's mask, for one shard.  A handle's part was sliced, counted and listed when it was made:
// only whether its list pays for this k is left to ask.  A pointer mask is sliced into *words, counted (one pass per call:
// how long will each scan be?) and, when selective, listed into *ids -- the caller's scratch, which the result points into.
ShardMask resolve_mask(Shard *s, const MaskSrc &mask, int32_t k, int32_t entries, std::vector<uint64_t> *words, std::vector<uint32_t> *ids) {
  ShardMask m;
  if (const MaskPart *mp = mask.part) {
    m.part = mp;
    m.words = mp->h_words.data();
    m.rows_est = std::max<int64_t>(mp->kept, 1);
    if (mp->list_padded > 0 && row_list_pays(s, mp->kept, k, entries)) {
      m.list.d_ids = mp->list.d;
      m.list.padded = mp->list_padded;
    }
  } else if (mask.bytes) {
    const int32_t n_tiles = (int32_t)((s->rows + 63) / 64);
    if (words->size() < (size_t)n_tiles) words->resize((size_t)n_tiles);
    slice_mask(s, mask.bytes, words->data(), n_tiles);
    m.words = words->data();
    m.epoch = s->mask_epoch_src.fetch_add(1);
    m.rows_est = std::max<int64_t>(popcount_words(words->data(), (size_t)n_tiles), 1);
    if (build_row_list(s, words->data(), n_tiles, m.rows_est, k, entries, ids)) {
      m.list.ids = ids->data();
      m.list.padded = (int32_t)ids->size();
    }
  }
  return m;
}

int ctx_reserve_exact(Ctx *c, int64_t n) {
  if (n <= c->x_cap) return TSH_OK;
  hipFree(c->d_xkey);
  hipFree(c->d_xsum);
  c->d_xkey = nullptr;
  c->d_xsum = nullptr;
  c->bytes -= c->x_cap * 24;
  c->x_cap = 0;
  const int64_t want = std::min<int64_t>(round_up(n + n / 2, 1024), EX_MAX_ROWS);
  HIPCHK(hipMalloc(&c->d_xkey, (size_t)want * sizeof(uint64_t)));
  HIPCHK(hipMalloc(&c->d_xsum, (size_t)want * 2 * sizeof(double)));
  if (!c->d_xpick) {
    HIPCHK(hipMalloc(&c->d_xpick, (size_t)(1 + EX_MAX_ROWS / EX_R) * sizeof(uint64_t)));
    HIPCHK(hipMemset(c->d_xpick, 0, sizeof(uint64_t)));
    c->bytes += (1 + EX_MAX_ROWS / EX_R) * 8;
  }
  c->x_cap = want;
  c->bytes += want * 24;
  return TSH_OK;
}

// E1's arguments but for where the query is (a.query / a.query_out: the caller's); q: the query, zero-padded to ld;
// d_mask: the caller's mask words on the device, for entries by row, or NULL; d_list: the entries' rows, or NULL
void fill_exact_args(const Shard *s, const Ctx *c, const uint64_t *d_mask, const uint32_t *d_list, int64_t n_exam, const float *q, ExactArgsQ *xa) {
  ExactArgs *a = &xa->a;
  a->rows = s->d_rows;
  a->query = c->d_query;
  a->query_out = nullptr;
  a->live = s->d_live;
  a->mask = d_mask;
  a->list = d_list;
  a->list_out = nullptr;
  a->xkey = c->d_xkey;
  a->xsum = c->d_xsum;
  a->wmin = nullptr;
  a->sqrt_mag_a = s->metric == TSH_METRIC_COSINE ? std::sqrt(query_mag_a(q, s->dim)) : 0.0;
  a->ld = s->ld;
  a->n_rows = s->rows;
  a->n_entries = (int32_t)n_exam;
  a->dim = s->dim;
}

// a launch whose events, if any, ride on the kernel's own dispatch packet
#define TSH_LAUNCH_EV(kern, grid, block, st, start, stop, args)                                                      \
  do {                                                                                                               \
    if (start || stop) hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, st, start, stop, 0, args);            \
    else kern<<<grid, block, 0, st>>>(args);                                                                         \
  } while (0)
// E1 of a short search (tsh_exact.hip.h): one wave per eight entries, the events on the kernel's own packet
void launch_exact_scan(const ExactArgsQ &xa, int metric, hipStream_t st, const LaunchEv &ev) {
  const unsigned grid = (unsigned)((xa.a.n_entries + EX_R - 1) / EX_R);
  if (metric == TSH_METRIC_L2) TSH_LAUNCH_EV(exact_scan_kernel<METRIC_L2>, grid, 64, st, ev.start, ev.stop, xa);
  else if (metric == TSH_METRIC_IP) TSH_LAUNCH_EV(exact_scan_kernel<METRIC_IP>, grid, 64, st, ev.start, ev.stop, xa);
  else TSH_LAUNCH_EV(exact_scan_kernel<METRIC_COS>, grid, 64, st, ev.start, ev.stop, xa);
}

// ---- the fp16 scan's route (TSH_OPT_SCAN_F16) ---------------------------------------------------------------------
inline bool alloc_fault(int64_t bytes);      // tsh_host_batch.inl.h
inline bool device_has_room(int64_t bytes);
constexpr int64_t SCAN_F16_MIN_BYTES = 256ll << 20;  // the Infinity Cache: a row store below it is not HBM-bound

// Could a tile scan of this shard read the fp16 copy?  masked: behind a caller's mask, tombstones, quarantined rows or
// gaps -- TSH_OPT_SCAN_F16_MASKED decides for those, TSH_OPT_SCAN_F16 for dense scans and, at 0, for both.  (The shard's
// side of the decision: caller holds s->mu)
bool scan_f16_applies(const Shard *s, bool masked, int *v_exp) {
  const int mode = masked ? s->rows16.mode_masked : s->rows16.mode;
  if (s->rows16.mode == 0 || mode == 0 || s->rows16.denied || s->safe_mode()) return false;
  if (!scan_f16_supported(s->nch, s->dim)) return false;
  if (mode == 1 && s->rows * s->ld * 4 <= SCAN_F16_MIN_BYTES) return false;
  if (s->metric == TSH_METRIC_COSINE && !(s->min_norm > 0.f)) return false;  // (a zero row: no uniform cosine band)
  return scan_f16_exp(s->max_abs, v_exp);
}

// Brings a copy up to the shard's rows: allocation on first use (`bytes` for the row store's capacity), conversion of the
// rows past the watermark (all of them after a reset, or with `rebuild`) by convert(r0, r1) on `st`, waited for -- a scan
// on any stream may follow.  false: the copy does not fit on the device; the shard stays off it from now on (denied)
// instead of asking again with every query.  Caller holds row_copies_mu.
template <class Convert>
bool row_copy_ensure(Shard *s, RowCopy &c, int64_t bytes, bool rebuild, hipStream_t st, Convert convert) {
  if (c.denied) return false;
  if (c.d && c.cap == s->cap && !rebuild && c.valid == s->rows) return true;
  if (hipSetDevice(s->device) != hipSuccess) return false;
  if (!c.d || c.cap != s->cap) {
    c.release(s);
    if (alloc_fault(bytes) || !device_has_room(bytes) || hipMalloc(&c.d, (size_t)bytes) != hipSuccess) {
      (void)hipGetLastError();
      c.d = nullptr;
      c.denied = true;
      return false;
    }
    c.cap = s->cap;
    c.bytes = bytes;
    s->bytes += bytes;
  }
  if (rebuild) c.valid = 0;
  // whole tiles: the scan reads the last tile's rows past the shard's end (zeros in the f32 store) and drops them
  const int64_t r0 = c.valid, r1 = std::min(round_up(s->rows, 64), s->cap);
  convert(r0, r1);
  if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) {
    c.valid = 0;
    return false;
  }
  c.converted += s->rows - r0;
  c.valid = s->rows;
  return true;
}

// The fp16 copy, of scale 2^v_exp (another scale: every row again)
bool rows16_ensure(Shard *s, hipStream_t st, int v_exp) {
  std::lock_guard<std::mutex> lk(s->row_copies_mu);
  const bool rescale = s->rows16.exp != v_exp;
  s->rows16.exp = v_exp;
  return row_copy_ensure(s, s->rows16, s->cap * s->ld * 2, rescale, st, [&](int64_t r0, int64_t r1) {
    const int64_t groups = (r1 - r0) * s->ld / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((groups + 255) / 256, 8192));
    rows16_convert_kernel<<<grid, 256, 0, st>>>(s->d_rows, s->rows16.d, s->ld, r0, r1, std::ldexp(1.0f, v_exp));
  });
}

// The int8 copy and, behind its rows, their scales
bool rows8_ensure(Shard *s, hipStream_t st) {
  std::lock_guard<std::mutex> lk(s->row_copies_mu);
  return row_copy_ensure(s, s->rows8, s->cap * s->ld + s->cap * 4, false, st, [&](int64_t r0, int64_t r1) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((r1 - r0 + 3) / 4, 16384));
    rows8_convert_kernel<<<grid, 256, 0, st>>>(s->d_rows, s->rows8.d, rows8_scales(s->rows8, s->ld), s->ld, r0, r1);
  });
}

// Could a tile scan of this shard take the coarse int8 route?  masked: behind a caller's mask, tombstones, quarantined
// rows or gaps -- TSH_OPT_SCAN_I8_MASKED decides for those, TSH_OPT_SCAN_I8 for dense scans and, at 0, for both; an
// automatic masked route gives way to an fp16 masked route that was forced (TSH_OPT_SCAN_F16_MASKED = 2).  The exact path
// behind the scan needs a block of at least k entries.  (The shard's side of the decision: caller holds s->mu)
bool scan_i8_applies(const Shard *s, bool masked, int32_t k, int32_t entries) {
  const int mode = masked ? s->rows8.mode_masked : s->rows8.mode;
  if (s->rows8.mode == 0 || mode == 0 || s->rows8.denied || s->safe_mode()) return false;
  if (!masked && (!s->all_live || !s->quar_ids.empty())) return false;
  if (masked && mode == 1 && s->rows16.mode != 0 && s->rows16.mode_masked == 2) return false;
  if (!scan_i8_supported(s->nch) || k > entries || k > I8_LIST_CAP || s->rows <= 0) return false;
  if (mode == 1 && s->rows * s->ld * 4 <= SCAN_F16_MIN_BYTES) return false;
  if (s->metric == TSH_METRIC_COSINE && !(s->min_norm > 0.f)) return false;
  return true;
}

// The 4-bit plane and rho, from the int8 copy -- which the caller has just brought up to the shard's rows (rows8_ensure)
bool rows4_ensure(Shard *s, hipStream_t st) {
  std::lock_guard<std::mutex> lk(s->row_copies_mu);
  const int groups = scan_i4_groups(s->ld);
  if (!s->rows8.d || s->rows8.cap != s->cap || s->rows8.valid != s->rows) return false;
  return row_copy_ensure(s, s->rows4, s->cap * groups * 16 + s->cap * 4, false, st, [&](int64_t r0, int64_t r1) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((r1 - r0 + 3) / 4, 16384));
    rows4_convert_kernel<<<grid, 256, 0, st>>>(s->d_rows, static_cast<const uint8_t *>(s->rows8.d), rows8_scales(s->rows8, s->ld),
                                               static_cast<uint32_t *>(s->rows4.d), rows4_rho(s->rows4, groups), s->ld, s->dim, groups, r0, r1);
  });
}

// Could a scan that takes the coarse int8 route (scan_i8_applies said so) run the 4-bit pass in front of it?  Dense L2
// scans only: behind a mask, tombstones or gaps, and for inner product and cosine, the int8 scan runs alone.
bool scan_i4_applies(const Shard *s, bool masked) {
  const int mode = s->rows4.mode;
  if (mode == 0 || s->rows4.denied || masked || s->metric != TSH_METRIC_L2) return false;
  if (mode == 1 && s->rows * s->ld * 4 <= SCAN_I4_MIN_BYTES) return false;
  return true;
}

// the device buffers of the 4-bit pass: A's keys and minima, W's words, the control words and the host's total
int ctx_reserve_i4(Ctx *c, int64_t tiles) {
  if (!c->d_i4_ctl) {
    HIPCHK(hipMalloc(&c->d_i4_ctl, 16));
    HIPCHK(hipHostMalloc(&c->h_i4, 64, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_i4_dev), c->h_i4, 0));
    c->bytes += 16;
  }
  if (tiles > c->i4_tiles_cap) {
    hipFree(c->d_i4_keys);
    hipFree(c->d_i4_gmin);
    hipFree(c->d_i4_mask);
    c->d_i4_keys = c->d_i4_gmin = nullptr;
    c->d_i4_mask = nullptr;
    c->bytes -= c->i4_tiles_cap * (64 * 4 + 4 + 8);
    c->i4_tiles_cap = 0;
    HIPCHK(hipMalloc(&c->d_i4_keys, (size_t)tiles * 64 * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&c->d_i4_gmin, (size_t)tiles * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&c->d_i4_mask, (size_t)tiles * sizeof(uint64_t)));
    c->i4_tiles_cap = tiles;
    c->bytes += tiles * (64 * 4 + 4 + 8);
  }
  return TSH_OK;
}

// A's arguments; q: the staged query, ld floats (rides in the argument segment where it fits)
void fill_scan_i4_args(const Shard *s, const Ctx *c, const ScanI4Band &b, const float *q, ScanI4ArgsQ *aq) {
  ScanI4Args &a = aq->a;
  const int groups = scan_i4_groups(s->ld);
  a.plane = static_cast<const u32x4_i4 *>(s->rows4.d);
  a.query = s->ld <= SCAN_Q_INLINE ? nullptr : c->d_query;
  a.scale8 = rows8_scales(s->rows8, s->ld);
  a.rho = rows4_rho(s->rows4, groups);
  a.sqnorm = s->d_sqnorm;
  a.keys = c->d_i4_keys;
  a.gmin = c->d_i4_gmin;
  a.n = s->rows;
  a.n_tiles = (int32_t)((s->rows + 63) / 64);
  a.ld = (int32_t)s->ld;
  a.groups = groups;
  a.pad_ = 0;
  a.qbias = b.qbias;
  a.a_s = b.a_s;
  a.a_r = b.a_r;
  a.a_c = b.a_c;
  a.a_v = b.a_v;
  a.beta = b.beta;
  if (s->ld <= SCAN_Q_INLINE && q != aq->q) memcpy(aq->q, q, (size_t)s->ld * sizeof(float));
}

// A, T and W on st: afterwards c->d_i4_mask holds the survivors' words (their total: i4_total_kernel, launch_job_tail)
void launch_scan_i4(const ScanI4ArgsQ &aq, Ctx *c, int32_t k, hipStream_t st, hipEvent_t start) {
  const int32_t n_tiles = aq.a.n_tiles;
  const unsigned grid = (unsigned)((n_tiles + 3) / 4);
  const hipEvent_t none = nullptr;
  if (start) hipExtLaunchKernelGGL(scan_i4_kernel<4>, dim3(grid), dim3(256), 0, st, start, none, 0, aq);
  else scan_i4_kernel<4><<<grid, 256, 0, st>>>(aq);
  if (n_tiles <= SEL_VPT * SEL_THREADS) i4_tau_kernel<true><<<1, SEL_THREADS, 0, st>>>(c->d_i4_gmin, n_tiles, k, c->d_i4_ctl);
  else i4_tau_kernel<false><<<1, SEL_THREADS, 0, st>>>(c->d_i4_gmin, n_tiles, k, c->d_i4_ctl);
  i4_mask_kernel<<<grid, 256, 0, st>>>(c->d_i4_keys, n_tiles, c->d_i4_mask, c->d_i4_ctl);
}

// the int8 scan's arguments on top of the f32 scan's (fill_scan_args)
void fill_scan_i8_args(const Shard *s, const ScanI8Band &ib, ScanArgsQ *aq) {
  aq->a.rows16 = s->rows8.d;
  aq->a.scale8 = rows8_scales(s->rows8, s->ld);
  aq->a.sqnorm = s->d_sqnorm;
  aq->a.inv_scale = ib.qbias;
  aq->a.w_s = ib.a_s;
  aq->a.w_alpha = ib.a_v;
  aq->a.w_beta = ib.beta;
}

// the device buffers of the int8 scan's tail: the same for every shard size
int ctx_reserve_i8(Ctx *c) {
  if (!c->d_i8) {
    HIPCHK(hipMalloc(&c->d_i8, 16));  // [0] tau, [1] the survivors' total
    c->bytes += 16;
  }
  if (!c->d_i8_list) {
    HIPCHK(hipMalloc(&c->d_i8_list, (size_t)I8_LIST_CAP * sizeof(uint32_t)));
    c->bytes += I8_LIST_CAP * 4;
  }
  return TSH_OK;
}

// the fp16 scan's arguments on top of the f32 scan's (fill_scan_args) and the select's
void fill_scan_f16_args(const Shard *s, const ScanF16Band &fb, ScanArgsQ *aq, SelectArgs *se) {
  aq->a.rows16 = s->rows16.d;
  aq->a.sqnorm = s->d_sqnorm;
  aq->a.inv_scale = std::ldexp(1.0f, -s->rows16.exp);
  aq->a.w_alpha = fb.alpha;
  aq->a.w_beta = fb.beta;
  if (se) {
    se->eps_rel = 0.f;
    se->delta_abs = 2.0f * fb.w_max * 1.0001f;
    se->w_sq = s->metric == TSH_METRIC_COSINE ? nullptr : s->d_sqnorm;  // (cosine: the band is uniform)
    se->w_alpha = fb.alpha;
    se->w_beta = fb.beta;
  }
}

// The route of one query's scan on this shard, decided here for every caller and without side effects.  m: the search's
// mask (resolve_mask); masked: a mask or tombstones; q: the query (dim floats are read: zero-padded or not); no_f16:
// the redo of an fp16 scan.  Caller holds s->mu shared.
// after: a cursor job -- the f32 tile scan or the list scan, never the exact path or a reduced copy (tsh_after.hip.h)
Route choose_route(const Shard *s, const ShardMask &m, bool masked, int32_t k, int32_t entries, const float *q, bool no_f16,
                   bool no_i8 = false, bool after = false) {
  Route r;
  r.use_list = m.listed();
  if (after) {
    // (a list made for the exact path alone may be of a width scan_list_kernel does not serve: tiles behind the mask then)
    r.use_list = r.use_list && scan_list_supported(s->nch, s->ld);
    r.n_exam = r.use_list ? (int64_t)m.list.padded : s->rows;
    r.band = compute_band(s, q);
    return r;
  }
  // A search with only a few thousand rows to look at (a selective mask's list, a small index or shard) takes their
  // exact sums directly and selects among the exact distances: two dispatches instead of three, no f32 keys, no band
  // (tsh_exact.hip.h).  The block must have room for the k rows it will hold.
  r.n_exam = r.use_list ? (int64_t)m.list.padded : s->rows;
  r.exact = exact_applies(s, r.n_exam, k, entries);
  // the coarse int8 route: tile scans, dense or masked, inside the error model (TSH_OPT_SCAN_I8 = 2 resp.
  // TSH_OPT_SCAN_I8_MASKED = 2, the tests' settings, take it for shards the exact path would answer whole, too)
  if (!no_i8 && !r.use_list && (!r.exact || (masked ? s->rows8.mode_masked : s->rows8.mode) == 2) && scan_i8_applies(s, masked, k, entries) &&
      !compute_band(s, q).force_all) {
    r.ib = scan_i8_band(s->metric, s->dim, s->nch, q, s->max_norm, s->min_norm, s->max_abs);
    r.i8_eligible = true;
    if (r.exact && r.ib.ok) r.exact = false;  // (mode 2; a denial or a full device below leaves such a shard to its f32 scan)
    // E2' needs as many live waves as k; the survivors -- at least k rows, at the front of the list -- guarantee
    // ceil(k / EX_R) of them, and the host knows no more: the wide pick where that is enough, E2 otherwise.  Behind a
    // mask not even k rows need be alive (a tombstoned index of five rows, or of none): always E2, which writes
    // min(k, live rows) entries
    r.picked = !masked && s->exact_pick && (k + EX_R - 1) / EX_R >= k;
    if (r.ib.ok && scan_i4_applies(s, masked)) {
      r.i4b = scan_i4_band(s->dim, scan_i4_groups(s->ld), q, s->max_norm, s->max_abs);
      r.i4_eligible = r.i4b.ok;
    }
  }
  if (r.exact) {
    // E2' (the wide pick) bounds the k-th key by the k-th smallest wave minimum: it needs clearly more waves than k
    r.picked = s->exact_pick && (r.n_exam + EX_R - 1) / EX_R >= 2 * (int64_t)k;
    return r;
  }
  r.band = compute_band(s, q);
  // the fp16 route: tile scans of big shards, dense or masked, inside the error model on both sides
  r.f16_eligible = !no_f16 && !r.use_list && !r.band.force_all && scan_f16_applies(s, masked, &r.v_exp);
  if (r.f16_eligible) r.fb = scan_f16_band(s->metric, s->dim, s->nch, q, s->max_norm, s->min_norm, r.v_exp);
  return r;
}
// One query for job_enqueue
struct JobReq {
  JobReq(const float *q, int32_t k_, int32_t entries_) : query(q), k(k_), entries(entries_) {}
  const float *query;  // dim floats
  int32_t k, entries;
  ShardMask mask;
  uint8_t *dev_target = nullptr;  // shard mode: the caller's device block
  bool more_coming = false;       // the caller is about to submit more queries
  bool last_of_call = false;      // ... or this is the last of several
  uint32_t tag = 0;               // generation stamped into the block's header
  bool no_f16 = false;            // the redo of an fp16 scan whose list overflowed: f32 this time
  bool no_i8 = false;             // the redo of an int8 scan whose survivor list overflowed (with no_f16: f32)
  const Cursor *after = nullptr;  // a cursor search: only rows past it are wanted
  int64_t side_want = 0;          // ... redone after its side list overflowed: room for this many rows
  bool count = false;             // a count (tsh_search_count): how many rows pass count_thr and follow `after`, if given
  double count_thr = 0;           // ... its threshold (NaN: none)
  const GroupPart *groups = nullptr;  // a grouped search (tsh_search_grouped): this shard's part of the groups handle
  bool group_after = false;       // ... of tsh_search_grouped_after / tsh_search_grouped_count: `after` resp. `count` hold for GROUPS
  bool exact_all = false;         // ... whose rule does not hold for this call: every live row's exact sums for the finaliser
  int32_t group_rows = 0;         // ... of tsh_search_grouped_rows: this many rows of each group (0: a plain grouped search)
  int64_t seg_want = 0;           // ... redone after its member segments overflowed: room for this many rows
  bool rows_redone = false;       // ... redone at all (larger lists, or exact_all after its slots overflowed)
  bool mask_dies = false;         // ... enqueued for a ticket: a pointer mask's words and list are gone before the job is finished
};
// the arguments of a job's kernels (8 KiB: job_enqueue keeps them off the stack)
struct JobArgs {
  ScanArgsQ sa;
  ScanI4ArgsQ s4;  // (the 4-bit pass in front of an int8 scan: Job::i4)
  ExactArgsQ xa;
  SelectArgs se;
  RerankArgs ra;
};
// (RerankArgs, ExactSelArgs and ExactPickArgs below: in the order of their fields)
RerankArgs rerank_args(const Shard *s, const Ctx *c, const uint32_t *cand_rows, const uint32_t *count_ptr, BlockEntry *out, int32_t cap) {
  return RerankArgs{s->d_rows, c->d_query, cand_rows, count_ptr, out, s->ld, s->row_base, s->dim, cap, s->metric};
}
// E2' reads what E2 reads (xs), E1's wave minima and its own counter
ExactPickArgs exact_pick_args(const ExactSelArgs &xs, const Ctx *c) {
  return ExactPickArgs{xs.xkey, xs.xsum, xs.list, /*wmin*/ c->d_xpick + 1, /*ctr*/ reinterpret_cast<unsigned long long *>(c->d_xpick),
                       xs.hdr, xs.hdr_host, xs.out, xs.row_base, xs.shard_rows, xs.n_entries,
                       /*n_groups*/ (xs.n_entries + EX_R - 1) / EX_R, xs.k, xs.cap, xs.metric, xs.tag, xs.list_total, xs.list_cap};
}
// Reserves what the job's route needs in its context and stages the inputs on the host: the job's fields, mask and list in
// the context's pinned buffers where new to it, the query zero-padded at *qp (the scan's argument segment, or c->h_query)
int job_stage(Shard *s, Job *j, const JobReq &rq, JobArgs *ka, float **qp) {
  Ctx *c = j->c;
  const ShardMask &m = rq.mask;
  const Route &r = j->route;
  int rc = ctx_prepare(s, c, rq.entries, m.words != nullptr && !m.part);
  if (rc) return rc;
  const bool own_list = r.use_list && !m.list.d_ids;  // the context's copy of a host-made list
  if (own_list && (rc = ctx_reserve_list(c, m.list.padded))) return rc;
  if (r.exact && (rc = ctx_reserve_exact(c, r.n_exam))) return rc;
  j->d_mask = m.part ? m.part->words.d : c->d_mask;
  j->d_list = r.use_list ? (own_list ? c->d_list : m.list.d_ids) : nullptr;
  j->k = rq.k;
  j->entries = rq.entries;
  j->dev_target = rq.dev_target;
  j->quar_sel.clear();
  if (!s->quar_ids.empty()) {
    quarantine_select(s, m.words, &j->quar_sel);
    if (!j->quar_sel.empty() && !rq.dev_target && !c->h_quar) {
      HIPCHK(hipHostMalloc(&c->h_quar, QUARANTINE_MAX * sizeof(BlockEntry), hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&c->h_quar_dev), c->h_quar, 0));
    }
  }
  // (a list scan needs the mask words on the device only where quarantined rows are matched against them)
  j->up_mask = m.words && !m.part && c->mask_epoch != m.epoch && (!r.use_list || (!j->quar_sel.empty() && rq.dev_target));
  if (j->up_mask) {
    memcpy(c->h_mask, m.words, (size_t)((s->rows + 63) / 64) * 8);
    c->mask_epoch = m.epoch;
  }
  j->up_list = own_list && c->list_epoch != m.epoch;
  if (j->up_list) {
    memcpy(c->h_list, m.list.ids, (size_t)m.list.padded * sizeof(uint32_t));
    c->list_epoch = m.epoch;
  }
  float *q = *qp = s->ld <= SCAN_Q_INLINE ? (r.exact ? ka->xa.q : ka->sa.q) : c->h_query;
  memcpy(q, rq.query, (size_t)s->dim * sizeof(float));
  for (int64_t i = s->dim; i < s->ld; ++i) q[i] = 0.f;
  return TSH_OK;
}

// The arguments of the job's kernels: E1 and E2 (Job::xsel) of the exact path, or scan, select and re-rank.  q: the
// staged query (job_stage)
void fill_job_args(const Shard *s, Job *j, const JobReq &rq, const float *q, JobArgs *ka) {
  Ctx *c = j->c;
  const Route &r = j->route;
  const bool inline_q = s->ld <= SCAN_Q_INLINE;
  BlockHeader *hdr = reinterpret_cast<BlockHeader *>(rq.dev_target ? rq.dev_target : c->d_block);  // where the device header lives
  BlockHeader *hdr_host = reinterpret_cast<BlockHeader *>(c->h_block_dev);
  BlockEntry *out = reinterpret_cast<BlockEntry *>((rq.dev_target ? rq.dev_target : c->h_block_dev) + sizeof(BlockHeader));
  if (r.exact) {
    ExactArgs &a = ka->xa.a;
    fill_exact_args(s, c, j->user_mask && !r.use_list ? j->d_mask : nullptr, j->d_list, r.n_exam, q, &ka->xa);
    a.query = inline_q ? nullptr : c->d_query;
    // (only the quarantine kernels read the device copy of an inline query)
    a.query_out = inline_q && !j->quar_sel.empty() ? c->d_query : nullptr;
    if (j->up_list) {  // a new list: E1 reads it where it is (pinned host memory) and leaves the device copy -- a
      a.list = c->h_list_dev;  // DMA packet in front of the scan cost a lone masked query ~8 us before anything ran
      a.list_out = c->d_list;
    }
    if (r.picked) a.wmin = c->d_xpick + 1;
    j->xsel = ExactSelArgs{c->d_xkey, c->d_xsum, j->d_list, hdr, hdr_host, out, s->row_base, /*shard_rows*/ s->rows, a.n_entries,
                           rq.k, /*cap*/ rq.entries, s->metric, rq.tag};
    return;
  }
  fill_scan_args(s, c, j->user_mask ? j->d_mask : nullptr, j->d_list, r.use_list ? rq.mask.list.padded : 0, &ka->sa);
  if (inline_q) {
    ka->sa.a.query = nullptr;        // read q[] from the kernel-argument segment ...
    ka->sa.a.query_out = c->d_query;  // ... and leave a device copy for the rerank kernel
  }
  SelectArgs &se = ka->se = SelectArgs{};
  se.gmin = c->d_gmin;
  se.keys = c->d_keys;
  se.hdr = hdr;
  se.hdr_host = hdr_host;
  se.cand_rows = c->d_cand;
  se.n_tiles = ka->sa.a.n_tiles;
  se.list = j->d_list;
  se.tag = rq.tag;
  se.k = rq.k;
  se.cand_cap = rq.entries;
  se.eps_rel = r.band.eps_rel;
  se.delta_abs = r.band.delta_abs;
  se.force_all = r.band.force_all;
  se.metric = s->metric;
  se.row_base = s->row_base;
  se.shard_rows = s->rows;
  if (j->store == RowStore::F16) fill_scan_f16_args(s, r.fb, &ka->sa, &se);
  if (j->store == RowStore::I8) {
    // the coarse scan, then E1 + E2 / E2' over the survivor list: I8_LIST_CAP entries, the padding dead.  E1 reads the
    // query's device copy (the scan's workgroup 0 leaves it, or it was uploaded in front of the scan)
    fill_scan_i8_args(s, r.ib, &ka->sa);
    if (j->i4) {  // A, T, W, then the int8 scan as a masked one behind W's words
      fill_scan_i4_args(s, c, r.i4b, q, &ka->s4);
      ka->sa.a.mask = c->d_i4_mask;
    }
    fill_exact_args(s, c, nullptr, c->d_i8_list, I8_LIST_CAP, q, &ka->xa);
    if (r.picked) ka->xa.a.wmin = c->d_xpick + 1;
    j->xsel = ExactSelArgs{c->d_xkey, c->d_xsum, c->d_i8_list, hdr, hdr_host, out, s->row_base, /*shard_rows*/ s->rows, I8_LIST_CAP,
                           rq.k, /*cap*/ rq.entries, s->metric, rq.tag, /*list_total*/ c->d_i8 + 1, /*list_cap*/ (uint32_t)I8_LIST_CAP};
  }
  ka->ra = rerank_args(s, c, c->d_cand, &hdr->count, out, rq.entries);
}

// ---- on which streams a job's kernels run (all of it under the device's scan_mu) ------------------------------------
// The scan's stream; *which >= 0: one of the two scan streams, for a scan that alternates between them (small shards,
// big shards' scans with a large drain share), booked in DeviceStreams::scan_out once the scan is enqueued
hipStream_t pick_scan_stream(Shard *s, RowStore store, bool overlap, int64_t rows_est, int *which, bool i4 = false) {
  *which = -1;
  // Between two scans on one in-order stream the slots of the finished launch empty over one wave life and nothing
  // refills them: half a wave life per scan, a share
  //   tile_bytes x waves_per_CU x CUs / 2 / bytes_the_scan_moves
  // of the scan (tsh_scan_overlap.h).  Where that share is large -- every small shard, and a big shard's scans over the
  // int8 or fp16 copy, which read as few bytes as a quarter or half as many f32 rows -- consecutive scans alternate between
  // two streams and the next scan's workgroups fill in as the previous one drains.  The two scans then run side by side,
  // so each one's own duration roughly doubles; elsewhere one stream, where a scan's duration is its HBM time.
  // TSH_OPT_SCAN_STREAMS = 1 / 2 forces either.
  // (a selective row mask makes a big shard's scan just as short: count the rows it keeps)
  const int32_t n_tiles = (int32_t)((s->rows + 63) / 64);
  const int64_t tiles_read = rows_est > 0 ? std::min<int64_t>(n_tiles, (rows_est + 63) / 64) : n_tiles;
  // (two scan streams exist on a split device only: the scans' CUs are those the tails' mask leaves)
  // (a scan with the 4-bit pass in front: its threshold kernel is one workgroup, in order between the two passes --
  // whatever the shard's size the other stream's pass keeps the HBM busy meanwhile)
  const bool two = s->scan_streams == 2 ||
                   (s->scan_streams == 0 && (i4 || scan_two_streams(store, s->nch, s->ld, tiles_read, s->cus - TAIL_CUS)));
  if (!(overlap && two && s->scan_stream2)) return s->scan_stream;
  DeviceStreams *ds = s->dstreams;
  for (size_t i = 0; i < ds->scan_out.size();) {  // scans that have finished since the last look
    if (hipEventQuery(ds->scan_out[i].ev) != hipErrorNotReady) {
      ds->scans_out[ds->scan_out[i].which]--;
      ds->scan_out[i] = ds->scan_out.back();
      ds->scan_out.pop_back();
    } else {
      ++i;
    }
  }
  (void)hipGetLastError();  // (hipErrorNotReady is an answer, not an error)
  *which = ds->scans_out[0] != ds->scans_out[1] ? (ds->scans_out[1] < ds->scans_out[0] ? 1 : 0) : (int)(s->scan_seq++ & 1);
  return *which ? s->scan_stream2 : s->scan_stream;
}

// The stream of what follows the scan (enqueued on ps; `scanned` rides on its packet): ps itself, in order, or one of
// the tail queues on the reserved CUs, made to wait for the scan.  overlap: ... and this is not the last query of a call
int pick_tail_stream(Shard *s, const Route &r, bool overlap, int which, hipStream_t ps, hipEvent_t scanned, hipStream_t *out) {
  *out = ps;
  // (the last query of a call: nothing follows its scan on that stream, so its tail stays there -- in order, without
  // the ~10 us of a cross-stream event hand-off in front of the select, on the step every caller waits for)
  // (the exact path's select stays on its scan stream, in order behind its short scan, while the scan is short: no
  // cross-stream hand-off, and the two scan streams alternate whole queries -- 64-query calls on 10 k x 128: 20.6 -> 16.2 us
  // per query, 2 k x 768: 22 -> 16.7, 8 k x 768: 21 -> 18.4; from ~8 k rows of 768 on the tail queues win again: 16 k x
  // 768 23 against 25; tools/r5_x_inorder.sh)
#ifndef TSH_X_INORDER_MAX
#define TSH_X_INORDER_MAX 6500000
#endif
  // (round 6: behind the wide pick -- 5-6 us, one workgroup per 256 entries -- the tail queues' 16 CUs and their
  // cross-stream hand-off, ~10 us in front of the pick under load, never pay: 10 k x 768 in 64-query calls 18.5-23.9 ->
  // 15.8-19.2 us per query, same box, alternating, tools/r6_inorder_ab.sh)
  const bool x_inorder = r.exact && (r.picked || r.n_exam * s->ld <= (int64_t)TSH_X_INORDER_MAX);
  if (!overlap || x_inorder) return TSH_OK;
  // (one tail queue serialises select + re-rank of consecutive queries: ~40 us per query, which is what short
  // scans -- selective masks, small shards -- were then limited by)
  static const bool one_tail = probe_env("TSH_ONE_TAIL") != nullptr && probe_env("TSH_ONE_TAIL")[0] == '1';
  // (a small shard's two scan streams each have their tail queue: the scans of one stream end a scan's length
  // apart, longer than a tail, so no tail queues behind another -- alternating blindly put two tails of
  // near-simultaneous scan ends on one queue at the end of a call, 40 us in full view)
  if (which >= 0 && !one_tail && s->tail_stream2) *out = which ? s->tail_stream2 : s->tail_stream;
  else *out = (!one_tail && s->tail_stream2 && (s->tail_seq++ & 1)) ? s->tail_stream2 : s->tail_stream;
  HIPCHK(hipStreamWaitEvent(*out, scanned, 0));
  return TSH_OK;
}

// ---- which kernels run for a job ------------------------------------------------------------------------------------
// The first-pass kernel of a route, for searches and for the measurement hook alike: E1 over xa, or over sa the list
// scan or the tile scan of `store`.  masked: a mask or dead rows; rows_est: the mask's (ShardMask), 0 = none
void launch_route_scan(const Shard *s, const Route &r, RowStore store, bool masked, int64_t rows_est, const ScanArgsQ &sa,
                       const ExactArgsQ &xa, hipStream_t st, const LaunchEv &ev) {
  if (r.exact) return launch_exact_scan(xa, s->metric, st, ev);
  if (r.use_list) return launch_scan_list(sa, s->nch, s->metric, st, ev);
  const bool ml = masked && scan_mostly_live(rows_est > 0 ? rows_est : s->rows - s->deleted, s->rows);
  switch (store) {
    case RowStore::I8: launch_scan_i8(sa, s->nch, s->metric, masked, st, ev, ml); break;
    case RowStore::F16: launch_scan_f16(sa, s->nch, s->metric, masked, st, ev, ml); break;
    case RowStore::F32: launch_scan(sa, s->nch, s->metric, masked, st, ev, ml); break;
  }
}

// The copies of what is new to the context, then the route's scan, all on ps
// (short scans as ONE dispatch -- every workgroup scans its tiles, the one drawing the last ticket selects and
// re-ranks -- were built in round 2 and measured slower than these three launches: C1 45 vs 37 us per call,
// keep-1 % masks 11.8 k vs 23.8 k queries/s.  Removed in round 3)
int launch_job_scan(Shard *s, Job *j, const JobReq &rq, const JobArgs &ka, hipStream_t ps, const LaunchEv &ev) {
  Ctx *c = j->c;
  if (j->up_mask)
    HIPCHK(hipMemcpyAsync(c->d_mask, c->h_mask, (size_t)((s->rows + 63) / 64) * 8, hipMemcpyHostToDevice, ps));
  if (j->up_list && !j->route.exact)
    HIPCHK(hipMemcpyAsync(c->d_list, c->h_list, (size_t)rq.mask.list.padded * sizeof(uint32_t), hipMemcpyHostToDevice, ps));
  if (s->ld > SCAN_Q_INLINE)
    HIPCHK(hipMemcpyAsync(c->d_query, c->h_query, (size_t)s->ld * sizeof(float), hipMemcpyHostToDevice, ps));
  if (j->i4) {
    // the 4-bit pass, its threshold and its mask, then the int8 scan over the survivors in the scattered-mask grid: all in
    // order on this stream (the job's timing events bracket the four)
    launch_scan_i4(ka.s4, c, j->k, ps, ev.start);
    LaunchEv evb;
    evb.stop = ev.stop;
    launch_scan_i8(ka.sa, s->nch, s->metric, /*masked*/ true, ps, evb, /*mostly_live*/ false);
    return TSH_OK;
  }
  launch_route_scan(s, j->route, j->store, j->masked, rq.mask.rows_est, ka.sa, ka.xa, ps, ev);
  return TSH_OK;
}

// shard mode, a cursor job: the rows its floor pass could not decide go into the job's device block as well (A2',
// tsh_after.hip.h); `done`: an event to ride on the kernel's packet, or NULL
void launch_after_side_append(Shard *s, Ctx *c, Job *j, hipStream_t st, hipEvent_t done) {
  const uint32_t side_cap = (uint32_t)c->side_cap;
  const AfterSideAppendArgs sd{s->d_rows, c->d_query, c->d_side_rows, c->d_side_cnt + j->side_word, c->d_side_cnt + (j->side_word ^ 1),
                               &c->h_side_dev[0].id, j->dev_target, s->ld, s->row_base, s->dim, s->metric, side_cap, j->entries};
  const hipEvent_t none = nullptr;
  // (the grid of after_side_kernel: a page has a row or two to decide)
  TSH_LAUNCH_EV(after_side_append_kernel, side_cap > (uint32_t)AFTER_SIDE_CAP ? std::min(side_cap, 1024u) : 64u, 64, st, none, done, sd);
}

// What follows the scan, on ts: the exact path's pick or select, or select + re-rank; then the quarantined rows the
// mask keeps, if any.  The completion event rides on the last kernel's own dispatch packet unless more kernels follow
// (a separate hipEventRecord is one more runtime call and one more barrier packet per query)
// (short rows and lists, config C1: K2 + K4 as ONE dispatch, the selecting workgroup re-ranking its dozen
// candidates a lane each, was tried -- 17 us against 9 + 4.4 for the two launches: the lone workgroup waits out
// count -> candidate ids -> rows one after the other, which the second launch's ramp-up hides)
int launch_job_tail(Shard *s, Job *j, const JobArgs &ka, hipStream_t ts) {
  Ctx *c = j->c;
  const bool quar = !j->quar_sel.empty();
  const hipEvent_t none = nullptr, done = quar ? none : c->ev_done;
  const bool i8 = j->store == RowStore::I8;
  // (the 4-bit pass's survivors, counted for the host beside the tail: nothing on the scan streams waits for it)
  if (j->i4) i4_total_kernel<<<1, 1024, 0, ts>>>(c->d_i4_mask, ka.sa.a.n_tiles, c->h_i4_dev);
  if (i8) {
    // threshold, candidate tiles, the survivors' ascending list (capped and padded) and their total; E1 over the list
    const int32_t n_tiles = ka.sa.a.n_tiles;
    if (n_tiles <= SEL_VPT * SEL_THREADS) i8_list_kernel<true><<<1, SEL_THREADS, 0, ts>>>(c->d_gmin, c->d_keys, n_tiles, j->k, c->d_i8_list, c->d_i8);
    else i8_list_kernel<false><<<1, SEL_THREADS, 0, ts>>>(c->d_gmin, c->d_keys, n_tiles, j->k, c->d_i8_list, c->d_i8);
    launch_exact_scan(ka.xa, s->metric, ts, LaunchEv());
  }
  if (j->route.picked) {  // E2': one workgroup per 256 entries, a bound from E1's wave minima, no ranking below it
    const ExactPickArgs xp = exact_pick_args(j->xsel, c);
    TSH_LAUNCH_EV(exact_pick_kernel, (unsigned)((xp.n_entries + 255) / 256), 256, ts, none, done, xp);
  } else if (j->route.exact || i8) {
    TSH_LAUNCH_EV(exact_select_kernel, 1, 1024, ts, none, done, j->xsel);
  } else if (j->windowed && j->grouped) {
    // a group count: the head table cleared, every group's head found (G1); the window pass classifies the heads, counts
    // the groups certainly in the list and sends the rows of the groups it could not decide to the side list (GC); their
    // exact sums by the count jobs' side re-rank (C2) -- tsh_group.hip.h.  No select, no re-rank
    const GroupPart *gp = j->gpart;
    const int32_t n_tiles = ka.se.n_tiles;
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = c->d_side_cnt + j->side_word;
    const CountWindow &w = j->window;
    const GroupArgs ga{c->d_keys, c->d_gmin, j->d_list, gp->group.d, c->d_gm, nullptr, nullptr, gp->built_rows.load(), gp->n_groups, n_tiles};
    if (gp->n_groups > 0) HIPCHK(hipMemsetAsync(c->d_gm, 0xFF, (size_t)gp->n_groups * 8, ts));
    group_min_kernel<<<(unsigned)((n_tiles + 3) / 4), 256, 0, ts>>>(ga);
    const GroupCountArgs gc{ga, c->d_side_rows, side_count, c->d_side_cnt + 2, side_cap, w.in_lo, w.in_hi, w.out_lo, w.out_hi, ka.se.eps_rel, ka.se.delta_abs};
    group_count_window_kernel<<<(unsigned)((n_tiles + 4 * GROUP_COUNT_WAVE_TILES - 1) / (4 * GROUP_COUNT_WAVE_TILES)), 256, 0, ts>>>(gc);
    const CountSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->d_side_cnt + 2, c->h_side_dev,
                           s->ld, s->row_base, s->dim, s->metric, side_cap};
    TSH_LAUNCH_EV(count_side_kernel, std::min(side_cap, 1024u), 64, ts, none, done, sd);
  } else if (j->grouped && j->floored) {
    // a grouped cursor search: G1 as ever -- over all live rows, whatever the cursor --, then the heads pass and the side
    // pass with the cursor's floor keys (G2a, G3a) around the unchanged select and re-rank -- tsh_group.hip.h.  Both
    // passes draw places in the one side list through the job's one count word
    const GroupPart *gp = j->gpart;
    const int32_t n_tiles = ka.se.n_tiles;
    const unsigned tgrid = (unsigned)((n_tiles + 3) / 4);
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = c->d_side_cnt + j->side_word;
    const GroupArgs ga{c->d_keys, c->d_gmin, j->d_list, gp->group.d, c->d_gm, c->d_heads, c->d_hmin, gp->built_rows.load(), gp->n_groups, n_tiles};
    if (gp->n_groups > 0) HIPCHK(hipMemsetAsync(c->d_gm, 0xFF, (size_t)gp->n_groups * 8, ts));
    group_min_kernel<<<tgrid, 256, 0, ts>>>(ga);
    const GroupHeadsAfterArgs gh{ga, c->d_side_rows, side_count, side_cap, j->floor.lo, j->floor.hi};
    group_heads_after_kernel<<<tgrid, 256, 0, ts>>>(gh);
    launch_select(ka.se, n_tiles, ts);
    TSH_LAUNCH_EV(rerank_kernel, (unsigned)std::min(j->entries, 1024), 64, ts, none, none, ka.ra);
    const GroupSideAfterArgs gs{GroupSideArgs{ga, ka.se.hdr, c->d_side_rows, side_count, side_cap, ka.se.eps_rel, ka.se.delta_abs}, j->floor.lo, j->floor.hi};
    group_side_after_kernel<<<tgrid, 256, 0, ts>>>(gs);
    const AfterSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->h_side_dev, s->ld, s->row_base,
                           s->dim, s->metric, side_cap};
    TSH_LAUNCH_EV(after_side_kernel, side_cap > (uint32_t)AFTER_SIDE_CAP ? std::min(side_cap, 1024u) : 64u, 64, ts, none, done, sd);
  } else if (j->windowed) {
    // a count job: the window pass counts the rows certainly in the list (C1), the rows it could not decide get their
    // exact sums (C2) -- tsh_count.hip.h.  No select, no re-rank
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = c->d_side_cnt + j->side_word;
    const CountWindow &w = j->window;
    const CountWindowArgs wa{c->d_keys, c->d_gmin, j->d_list, c->d_side_rows, side_count, c->d_side_cnt + 2, ka.se.n_tiles, side_cap,
                             w.in_lo, w.in_hi, w.out_lo, w.out_hi};
    count_window_kernel<<<(unsigned)((ka.se.n_tiles + 4 * COUNT_WAVE_TILES - 1) / (4 * COUNT_WAVE_TILES)), 256, 0, ts>>>(wa);
    const CountSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->d_side_cnt + 2, c->h_side_dev,
                           s->ld, s->row_base, s->dim, s->metric, side_cap};
    // (the side re-rank's grid: one workgroup per row up to the re-rank's own 1024)
    TSH_LAUNCH_EV(count_side_kernel, std::min(side_cap, 1024u), 64, ts, none, done, sd);
  } else if (j->grouped && j->group_rows > 0) {
    // a grouped job with rows per group: G1, G2, select and re-rank as below; in G3's place the marked groups get their
    // slots (R1), their live rows are counted, given segments and written there (R2 - R4), and a workgroup per slot
    // sends the rows that may be among the group's m best to the side list (R5) -- tsh_group_rows.hip.h
    const GroupPart *gp = j->gpart;
    const int32_t n_tiles = ka.se.n_tiles;
    const unsigned tgrid = (unsigned)((n_tiles + 3) / 4);
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = c->d_side_cnt + j->side_word;
    const uint32_t slot_cap = (uint32_t)std::min<int64_t>(group_rows_slots(j->k), c->gr_slots);
    const GroupArgs ga{c->d_keys, c->d_gmin, j->d_list, gp->group.d, c->d_gm, c->d_heads, c->d_hmin, gp->built_rows.load(), gp->n_groups, n_tiles};
    if (gp->n_groups > 0) HIPCHK(hipMemsetAsync(c->d_gm, 0xFF, (size_t)gp->n_groups * 8, ts));
    // (the control words, cnt[] and cur[]; off[] is written before it is read)
    HIPCHK(hipMemsetAsync(c->d_gr_ctl, 0, (size_t)(GROUP_ROWS_CTL + 2 * c->gr_slots) * sizeof(uint32_t), ts));
    group_min_kernel<<<tgrid, 256, 0, ts>>>(ga);
    group_heads_kernel<<<tgrid, 256, 0, ts>>>(ga);
    launch_select(ka.se, n_tiles, ts);
    TSH_LAUNCH_EV(rerank_kernel, (unsigned)std::min(j->entries, 1024), 64, ts, none, none, ka.ra);
    uint32_t *const slots = c->d_gr_ctl + GROUP_ROWS_CTL;
    const GroupRowsArgs gr{ga, ka.se.hdr, c->d_gr_ctl, slots, slots + c->gr_slots, slots + 2 * c->gr_slots, c->d_gr_seg, slot_cap,
                           (uint32_t)std::min<int64_t>(c->gr_seg_cap, 0xFFFFFFFFll), (uint32_t)j->group_rows, c->d_side_rows, side_count, side_cap,
                           ka.se.eps_rel, ka.se.delta_abs, c->h_side_dev};
    group_rows_mark_kernel<<<tgrid, 256, 0, ts>>>(gr);
    group_rows_member_kernel<false><<<tgrid, 256, 0, ts>>>(gr);
    group_rows_alloc_kernel<<<(slot_cap + 255u) / 256u, 256, 0, ts>>>(gr);
    group_rows_member_kernel<true><<<tgrid, 256, 0, ts>>>(gr);
    group_rows_pick_kernel<<<slot_cap, 256, 0, ts>>>(gr);
    const AfterSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->h_side_dev, s->ld, s->row_base,
                           s->dim, s->metric, side_cap};
    TSH_LAUNCH_EV(after_side_kernel, side_cap > (uint32_t)AFTER_SIDE_CAP ? std::min(side_cap, 1024u) : 64u, 64, ts, none, done, sd);
  } else if (j->grouped) {
    // a grouped job: the head table cleared, every group's head found (G1), one head per group left for the select (G2);
    // behind the re-rank the rows that may still be their group's best (G3) get their exact sums by the cursor jobs' side
    // re-rank -- tsh_group.hip.h
    const GroupPart *gp = j->gpart;
    const int32_t n_tiles = ka.se.n_tiles;
    const unsigned tgrid = (unsigned)((n_tiles + 3) / 4);
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = c->d_side_cnt + j->side_word;
    const GroupArgs ga{c->d_keys, c->d_gmin, j->d_list, gp->group.d, c->d_gm, c->d_heads, c->d_hmin, gp->built_rows.load(), gp->n_groups, n_tiles};
    if (gp->n_groups > 0) HIPCHK(hipMemsetAsync(c->d_gm, 0xFF, (size_t)gp->n_groups * 8, ts));
    group_min_kernel<<<tgrid, 256, 0, ts>>>(ga);
    group_heads_kernel<<<tgrid, 256, 0, ts>>>(ga);
    launch_select(ka.se, n_tiles, ts);
    TSH_LAUNCH_EV(rerank_kernel, (unsigned)std::min(j->entries, 1024), 64, ts, none, none, ka.ra);
    const GroupSideArgs gs{ga, ka.se.hdr, c->d_side_rows, side_count, side_cap, ka.se.eps_rel, ka.se.delta_abs};
    group_side_kernel<<<tgrid, 256, 0, ts>>>(gs);
    if (j->dev_target) {
      // shard mode (tsh_search_shard_grouped): the side rows' entries go into the caller's device block behind the
      // re-rank's, by the cursor jobs' own append (in front of the quarantined rows' append: both draw places in the block)
      launch_after_side_append(s, c, j, ts, done);
    } else {
      const AfterSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->h_side_dev, s->ld, s->row_base,
                             s->dim, s->metric, side_cap};
      TSH_LAUNCH_EV(after_side_kernel, side_cap > (uint32_t)AFTER_SIDE_CAP ? std::min(side_cap, 1024u) : 64u, 64, ts, none, done, sd);
    }
  } else {
    // a cursor job: the floor pass takes the rows at or before the cursor out of the select's sight (A1), and the rows
    // it could not decide get their exact sums behind the re-rank (A2) -- tsh_after.hip.h
    const uint32_t side_cap = (uint32_t)c->side_cap;
    uint32_t *const side_count = j->floored ? c->d_side_cnt + j->side_word : nullptr;
    if (j->floored) {
      const AfterFloorArgs fa{c->d_keys, c->d_gmin, j->d_list, c->d_side_rows, side_count, ka.se.n_tiles, side_cap, j->floor.lo, j->floor.hi};
      after_floor_kernel<<<(unsigned)((ka.se.n_tiles + 3) / 4), 256, 0, ts>>>(fa);
    }
    launch_select(ka.se, ka.se.n_tiles, ts);
    TSH_LAUNCH_EV(rerank_kernel, (unsigned)std::min(j->entries, 1024), 64, ts, none, j->floored ? none : done, ka.ra);
    if (j->floored && j->dev_target) {
      launch_after_side_append(s, c, j, ts, done);  // (in front of the quarantined rows' append: both draw places in the block)
    } else if (j->floored) {
      const AfterSideArgs sd{s->d_rows, c->d_query, c->d_side_rows, side_count, c->d_side_cnt + (j->side_word ^ 1), c->h_side_dev, s->ld, s->row_base,
                             s->dim, s->metric, side_cap};
      // (a page has a row or two to decide: 64 workgroups stride over a full list of AFTER_SIDE_CAP ids; only a redo's
      // larger list gets the re-rank's own grid)
      TSH_LAUNCH_EV(after_side_kernel, side_cap > (uint32_t)AFTER_SIDE_CAP ? std::min(side_cap, 1024u) : 64u, 64, ts, none, done, sd);
    }
  }
  if (!quar) return TSH_OK;
  if (j->dev_target) launch_quarantine_append(s, c, j, ts);
  else launch_quarantine(s, c, ts);
  HIPCHK(hipEventRecord(c->ev_done, ts));
  return TSH_OK;
}

// A cursor job whose cursor no scanned row can follow (a +inf or NaN distance): an empty block, and the quarantined rows
// the mask keeps -- in shard mode both in the caller's device block.  q: the staged query (job_stage)
int enqueue_after_skip(Shard *s, Job *j, const JobReq &rq, const float *q) {
  Ctx *c = j->c;
  BlockHeader *h = reinterpret_cast<BlockHeader *>(c->h_block);
  memset(h, 0, sizeof *h);
  h->entries = (uint32_t)j->entries;
  h->k = (uint32_t)j->k;
  h->metric = (uint32_t)s->metric;
  h->row_base = s->row_base;
  h->shard_rows = s->rows;
  h->pad[1] = rq.tag;
  j->store = RowStore::F32;
  j->timed = j->counted = false;
  hipStream_t st = s->aux_stream;
  // (the pinned header is this job's until it is finished: the copy reads it in place)
  if (j->dev_target) HIPCHK(hipMemcpyAsync(j->dev_target, h, sizeof *h, hipMemcpyHostToDevice, st));
  if (!j->quar_sel.empty()) {
    if (q != c->h_query) memcpy(c->h_query, q, (size_t)s->ld * sizeof(float));
    HIPCHK(hipMemcpyAsync(c->d_query, c->h_query, (size_t)s->ld * sizeof(float), hipMemcpyHostToDevice, st));
    if (j->dev_target) {
      if (j->up_mask) {  // (no scan uploads the mask words the append matches the quarantined rows against)
        HIPCHK(hipMemcpyAsync(c->d_mask, c->h_mask, (size_t)((s->rows + 63) / 64) * 8, hipMemcpyHostToDevice, st));
        j->up_mask = false;
      }
      launch_quarantine_append(s, c, j, st);
    } else {
      launch_quarantine(s, c, st);
    }
  }
  // (what job_stage staged for a scan that does not run never reaches the device: the context's copies are not current)
  if (j->up_mask) c->mask_epoch = 0;
  if (j->up_list) c->list_epoch = 0;
  HIPCHK(hipEventRecord(c->ev_done, st));
  j->last_stream = st;
  return TSH_OK;
}

int job_enqueue(Shard *s, Job *j, const JobReq &rq) {
  Ctx *c = j->c;
  static thread_local JobArgs ka;  // ScanArgsQ, ExactArgsQ: 4 KiB each: keep them off the stack of deep callers
  j->user_mask = rq.mask.words != nullptr;
  j->masked = j->user_mask || !s->all_live;
  j->no_i8 = rq.no_i8;
  j->has_after = rq.after != nullptr;
  j->after_redone = rq.side_want > 0;
  if (rq.after) j->after = *rq.after;
  j->counting = rq.count;
  j->count_thr = rq.count_thr;
  j->certain = 0;
  j->grouping = rq.groups != nullptr;
  j->gpart = rq.groups;
  j->group_after = rq.group_after;
  j->exact_all = rq.exact_all;
  j->group_rows = rq.groups ? rq.group_rows : 0;
  j->rows_redone = rq.rows_redone;
  const Route &r = j->route =
      choose_route(s, rq.mask, j->masked, rq.k, rq.entries, rq.query, rq.no_f16, rq.no_i8, j->has_after || rq.count || j->grouping);
  // (the exact-all route of a grouped cursor search or group count: what safe mode runs -- no floor, no window, no group
  // passes below, and the wide-band pass hands every live row's exact sums to the finaliser)
  if (rq.exact_all) j->route.band.force_all = 1;
  // A cursor inside the error model gets its floor in the scan's key space (tsh_after_band.h); "from the start" has
  // none; a +inf or NaN cursor can only be followed by quarantined rows -- every row the scan offers has a finite
  // distance -- so no scan runs at all.  Safe mode: no floor, the finaliser filters.
  // A count inside the error model gets its window there (tsh_count_band.h), or no scan at all where no scanned row can
  // count.  Safe mode: a plain search job whose every live row reaches the finaliser with its exact sums.
  // A grouped search inside the error model gets its group passes (tsh_group.hip.h); safe mode: a plain search job.
  j->floored = j->after_skip = j->windowed = false;
  j->grouped = j->grouping && !r.band.force_all;
  if (rq.count) {
    if (!r.band.force_all) {
      j->window = count_window(s->metric, s->dim, r.band.eps_rel, r.band.delta_abs,
                               s->metric == TSH_METRIC_COSINE ? query_mag_a(rq.query, s->dim) : 0.0, j->has_after, j->after.dist, rq.count_thr);
      j->after_skip = j->window.skip;
      j->windowed = !j->window.skip;
    }
  } else if (j->has_after && !r.band.force_all) {
    if (!(j->after.dist < INFINITY)) {
      j->after_skip = true;
    } else {
      j->floor = after_floor(s->metric, s->dim, r.band.eps_rel, r.band.delta_abs,
                             s->metric == TSH_METRIC_COSINE ? query_mag_a(rq.query, s->dim) : 0.0, j->after.dist);
      j->floored = !j->floor.none();
    }
  }
  float *q;
  int rc = job_stage(s, j, rq, &ka, &q);
  if (rc) return rc;
  if (j->after_skip) {
    j->grouped = false;  // (a grouped cursor search or group count no scanned row can follow: no group passes, no side list)
    return enqueue_after_skip(s, j, rq, q);
  }
  if (j->grouped && (rc = ctx_reserve_group(c, rq.groups->n_groups))) return rc;
  const bool rows_job = j->grouped && j->group_rows > 0;
  if (rows_job && (rc = ctx_reserve_group_rows(c, group_rows_slots(rq.k), rq.seg_want))) return rc;
  // (a rows job sends on about m rows of each marked group: its side list starts with room for twice k * m of them, the
  // shard's rows at the most)
  const int64_t rows_side = !rows_job ? 0 : std::min<int64_t>(round_up(2 * (int64_t)rq.k * j->group_rows + AFTER_SIDE_CAP, 1024), round_up(s->rows, 1024));
  if (j->floored || j->windowed || j->grouped) {
    if ((rc = ctx_reserve_side(c, std::max<int64_t>(std::max<int64_t>(std::max<int64_t>(rq.side_want, rows_side), AFTER_SIDE_CAP), c->side_cap)))) return rc;
    if (c->side_dirty) {  // (a context's first cursor or count job, or one after a job that failed on its way)
      HIPCHK(hipMemsetAsync(c->d_side_cnt, 0, 3 * sizeof(uint32_t), s->aux_stream));
      HIPCHK(hipStreamSynchronize(s->aux_stream));
    }
    c->side_dirty = true;  // until this job is seen finished (job_finish)
    j->side_word = c->side_flip;
    c->side_flip ^= 1;
    // what a redo with a larger side list needs: the query, the tag and the mask, all by reference -- they outlive the
    // job (a synchronous call finishes its jobs before it returns; a ticket holds the query).  Only a ticket behind a
    // pointer mask (rq.mask_dies) must keep the words itself: the caller's slice is gone when it is waited for, and so
    // is the list made from it -- that redo walks tiles behind the copied words
    j->redo_query = rq.query;
    j->tag = rq.tag;
    j->redo_mask = rq.mask;
    if (rq.mask_dies && !rq.mask.part && rq.mask.words) {
      j->redo_mask.list = RowList();
      if (rq.mask.words != j->redo_words.data())
        j->redo_words.assign(rq.mask.words, rq.mask.words + (size_t)((s->rows + 63) / 64));
      j->redo_mask.words = j->redo_words.data();
    }
  }
  // (an eligible scan uses up a denial of its route, if any are left, whatever its band; a scan that takes the int8
  // route neither asks for the fp16 copy nor touches the fp16 route's denials)
  j->store = RowStore::F32;
  j->i4 = false;
  if (r.i8_eligible && !s->rows8.route.take_denial() && r.ib.ok && rows8_ensure(s, s->scan_stream)) {
    j->store = RowStore::I8;
    if ((rc = ctx_reserve_exact(c, I8_LIST_CAP)) || (rc = ctx_reserve_i8(c))) return rc;
    // (the 4-bit pass in front of it: an eligible scan uses up a denial of ITS route, if any are left)
    if (r.i4_eligible && !s->rows4.take_denial() && rows4_ensure(s, s->scan_stream)) {
      if ((rc = ctx_reserve_i4(c, s->cap / 64))) return rc;
      j->i4 = true;
    }
  } else {
    if (!r.exact) j->route.picked = false;
    if (r.f16_eligible && !s->rows16.route.take_denial() && r.fb.ok && rows16_ensure(s, s->scan_stream, r.v_exp)) j->store = RowStore::F16;
  }
  if (j->store != RowStore::F32) {  // what a redo needs (redo_overflowed_scan)
    j->redo_q.assign(rq.query, rq.query + s->dim);
    j->tag = rq.tag;
    // (no list: such a scan walks tiles, and so does its redo.  A pointer mask's words were staged in c->h_mask under
    // rq.mask.epoch -- by this job or an earlier one of the call -- and stay there while the job holds the context)
    j->redo_mask = ShardMask();
    j->redo_mask.words = rq.mask.part ? rq.mask.words : (rq.mask.words ? c->h_mask : nullptr);
    j->redo_mask.epoch = rq.mask.epoch;
    j->redo_mask.rows_est = rq.mask.rows_est;
    j->redo_mask.part = rq.mask.part;
  }
  fill_job_args(s, j, rq, q, &ka);
  if (j->grouped) {  // select and re-rank see one head per group
    ka.se.gmin = c->d_hmin;
    ka.se.keys = c->d_heads;
  }
  // with other queries already in flight -- or the caller about to submit more (the first query of a multi-query
  // call: left alone it kept its select + re-rank on the pipeline stream, in front of the call's third scan) -- the
  // tail moves to the reserved CUs; a lone query keeps everything in order on one stream (no hand-off latency)
  const bool overlap = (s->inflight.fetch_add(1) > 0 || rq.more_coming) && s->cu_split;
  j->counted = true;
  {
    std::lock_guard<std::mutex> lk(*s->scan_mu);
    int which;
    // (a first scan on the second stream needs no wait for the copy it reads: rows8_ensure / rows16_ensure above
    // converted on scan_stream and synchronised on the host before they returned -- row_copy_ensure)
    hipStream_t ps = pick_scan_stream(s, j->store, overlap, rq.mask.rows_est, &which, j->i4), ts;
    j->timed = (s->c_scans.load() & 3) == 0;  // sample every 4th scan with timing events
    LaunchEv ev;  // start / stop ride on the scan's own packet: no barrier packets between scans
    if (j->timed) {
      ev.start = c->ev0;
      ev.stop = c->ev1;
    } else if (overlap) {
      ev.stop = c->ev_scanned;
    }
    if ((rc = launch_job_scan(s, j, rq, ka, ps, ev))) return rc;
    if (which >= 0 && ev.stop) {
      s->dstreams->scan_out.push_back({c, ev.stop, which});
      s->dstreams->scans_out[which]++;
    }
    if ((rc = pick_tail_stream(s, r, overlap && !rq.last_of_call, which, ps, ev.stop, &ts))) return rc;
    j->last_stream = ts;
    j->enq_seq = ++s->dstreams->enq_counter;
    if ((rc = launch_job_tail(s, j, ka, ts))) return rc;
  }
  s->c_scans++;
  if (r.use_list) s->c_list_scans++;
  if (r.exact) s->c_exact_scans++;
  if (RowCopy *copy = s->row_copy(j->store)) copy->route.scans++;
  return TSH_OK;
}

// Wide-band path for a query whose K2 list overflowed (ties / degenerate data):
// whole-grid filter of this context's keys[] + f64 rerank of everything in the band.
// host copies of f2key / key2f / band_of (tsh_kernels.hip.h)
inline uint32_t h_f2key(float f) {
  if (f != f) return KEY_NAN;
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float h_key2f(uint32_t k) {
  uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline uint32_t h_band_of(uint32_t tau_key, float eps_rel, float delta_abs) {
  if (tau_key >= KEY_NAN) return KEY_NAN;
  float t = h_key2f(tau_key);
  if (t == INFINITY) return KEY_NAN;
  double w = (double)t + std::fabs((double)t) * (double)eps_rel + (double)delta_abs;
  float f = (float)w;
  if ((double)f < w) f = std::nextafter(f, INFINITY);
  if (!(f < INFINITY)) return KEY_NAN;
  return h_f2key(f);
}

int run_fallback(Shard *s, Job *j, uint32_t band_key, std::vector<BlockEntry> *spill) {
  Ctx *c = j->c;
  hipStream_t st = s->aux_stream;
  // (a list scan left its keys in list order: fewer keys, and the filter maps positions back to row ids)
  const int64_t n_keys = j->route.use_list ? j->route.n_exam : ((s->rows + 63) / 64) * 64;
  const uint32_t *list = j->route.use_list ? j->d_list : nullptr;
  if (s->cap > c->big_cap) {
    hipFree(c->d_big_rows);
    hipFree(c->d_big_entries);
    c->d_big_rows = nullptr;
    c->d_big_entries = nullptr;
    HIPCHK(hipMalloc(&c->d_big_rows, (size_t)s->cap * sizeof(uint32_t)));
    HIPCHK(hipMalloc(&c->d_big_entries, (size_t)s->cap * sizeof(BlockEntry)));
    c->bytes += (s->cap - c->big_cap) * 28;
    c->big_cap = s->cap;
  }
  int fgrid = (int)std::min<int64_t>((n_keys + 255) / 256, 4096);
  const Band &band = j->route.band;
  // (a grouped job: the wide band is taken over the heads -- one key per group -- as the select was)
  const uint32_t *const f_keys = j->grouped ? c->d_heads : c->d_keys, *const f_gmin = j->grouped ? c->d_hmin : c->d_gmin;
  if (band_key >= KEY_NAN && !band.force_all && j->k < n_keys) {
    // K2 could not bound the k-th key (k beyond its tile-minimum scheme, or fewer than k live tiles and a full
    // list): find the exact k-th smallest key with a 4-pass radix select over all keys -- 4 small kernels and
    // host round trips instead of an f64 rerank of every row (k = 2000 on 1 M rows: 0.9 ms instead of 9)
    if (!c->d_hist) HIPCHK(hipMalloc(&c->d_hist, 256 * sizeof(uint32_t)));
    uint32_t prefix = 0, hist[256];
    uint64_t remaining = (uint64_t)j->k;
    bool found = true;
    for (int shift = 24; shift >= 0 && found; shift -= 8) {
      HIPCHK(hipMemsetAsync(c->d_hist, 0, sizeof hist, st));
      radix_hist_kernel<<<fgrid, 256, 0, st>>>(f_keys, f_gmin, n_keys, prefix, shift, c->d_hist);
      HIPCHK(hipMemcpyAsync(hist, c->d_hist, sizeof hist, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      uint64_t cum = 0;
      int b = 0;
      for (; b < 256; ++b) {
        if (cum + hist[b] >= remaining) break;
        cum += hist[b];
      }
      if (b == 256) {
        found = false;  // fewer than k live keys: everything is a candidate
      } else {
        remaining -= cum;
        prefix |= (uint32_t)b << shift;
      }
    }
    if (found) band_key = h_band_of(prefix, band.eps_rel, band.delta_abs);
  }
  HIPCHK(hipMemsetAsync(c->d_big_count, 0, 4, st));
  filter_kernel<<<fgrid, 256, 0, st>>>(f_keys, f_gmin, n_keys, band_key, c->d_big_rows, c->d_big_count,
                                      (uint32_t)c->big_cap, list);
  uint32_t count = 0;
  HIPCHK(hipMemcpyAsync(&count, c->d_big_count, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const RerankArgs ra = rerank_args(s, c, c->d_big_rows, c->d_big_count, c->d_big_entries,
                                    (int32_t)std::min<int64_t>(c->big_cap, 0x7FFFFFFF));
  if (count > 0) {
    int rgrid = (int)std::min<uint32_t>(count, 16384u);
    rerank_kernel<<<rgrid, 64, 0, st>>>(ra);
  }
  BlockHeader *h = reinterpret_cast<BlockHeader *>(c->h_block);
  h->count = count;
  h->flags = count > (uint32_t)j->entries ? FLAG_LIST_OVERFLOW : 0u;
  HIPCHK(hipMemcpyAsync(j->dev_target ? j->dev_target : c->d_block, h, sizeof *h, hipMemcpyHostToDevice, st));
  uint32_t fit = std::min<uint32_t>(count, (uint32_t)j->entries);
  if (fit) {
    if (j->dev_target)
      HIPCHK(hipMemcpyAsync(j->dev_target + sizeof(BlockHeader), c->d_big_entries, (size_t)fit * sizeof(BlockEntry),
                            hipMemcpyDeviceToDevice, st));
    else
      HIPCHK(hipMemcpyAsync(c->h_block + sizeof(BlockHeader), c->d_big_entries, (size_t)fit * sizeof(BlockEntry),
                            hipMemcpyDeviceToHost, st));
  }
  if (spill && count > (uint32_t)j->entries) {
    spill->resize(count);
    HIPCHK(hipMemcpyAsync(spill->data(), c->d_big_entries, (size_t)count * sizeof(BlockEntry),
                          hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  s->c_fallbacks++;
  s->c_cands += count;
  return TSH_OK;
}

// A finished scan whose 4-bit pass ran (Job::i4): the survivors it left, and the deny rule -- the pass pays only while few
// rows survive it.  Two scans in a row above SCAN_I4_MAX_SHARE deny the route for deny_len eligible scans.  Scans that
// were already in flight when the denial fell (a pipelined call) are counted and otherwise ignored.  When a denial has
// run out (RowCopyI4::take_denial) and the scans after it are over the share again, the next denial is twice as long,
// up to SCAN_I4_DENY_CAP; a scan at or below the share ends that.
void scan_i4_account(Shard *s, Job *j) {
  RowCopyI4 &c4 = s->rows4;
  const int64_t kept = (int64_t)j->c->h_i4[0];
  j->i4 = false;
  c4.route.scans++;
  c4.survivors += kept;
  if (c4.route.denied.load() > 0) return;
  if ((double)kept <= SCAN_I4_MAX_SHARE * (double)s->rows) {
    c4.route.strikes.store(0);
    c4.probation.store(false);
    c4.deny_len.store(SCAN_ROUTE_DENIED_SCANS);
    return;
  }
  if (c4.route.strikes.fetch_add(1) + 1 < 2) return;
  c4.route.strikes.store(0);
  const int len = c4.probation.load() ? std::min(2 * c4.deny_len.load(), SCAN_I4_DENY_CAP) : SCAN_ROUTE_DENIED_SCANS;
  c4.deny_len.store(len);
  c4.probation.store(false);
  c4.route.denied.store(len);
  c4.denials++;
}

// A finished fp16 or int8 scan (j->store) whose list overflowed -- the fp16 scan's candidate list (crowded neighbours:
// ties, near-duplicates), the int8 scan's survivor list (the same, or fewer live tiles than k in a big shard) -- is NOT
// widened over its reduced keys: the query is redone through the f32 scan, from the job's saved query, tag and mask, and
// the f32 scan's own overflow handling follows in job_finish as ever.  Books the route's strike or denial.
int redo_overflowed_scan(Shard *s, Job *j) {
  Ctx *c = j->c;
  const bool i8 = j->store == RowStore::I8;
  ScanRouteState &rt = s->row_copy(j->store)->route;
  const BlockHeader *h = reinterpret_cast<const BlockHeader *>(c->h_block);
  if (!(h->flags & (i8 ? FLAG_I8_OVERFLOW : FLAG_LIST_OVERFLOW))) {
    rt.strikes.store(0);
    return TSH_OK;
  }
  if (j->leave_overflow && j->dev_target) return TSH_OK;  // (left as it is: see Job::leave_overflow)
  rt.redone++;
  if (rt.strikes.fetch_add(1) + 1 >= 2) {
    rt.strikes.store(0);
    rt.denied.store(SCAN_ROUTE_DENIED_SCANS);
  }
  const std::vector<float> q(j->redo_q);
  JobReq rq(q.data(), j->k, j->entries);
  rq.mask = j->redo_mask;  // the WHERE clause holds for the redo too
  rq.dev_target = j->dev_target;
  rq.last_of_call = true;
  rq.tag = j->tag;
  // (a masked int8 scan is redone through the fp16 masked scan where that applies; should THAT list overflow too, the f32
  // scan follows below.  A dense one goes straight to f32, as ever)
  rq.no_f16 = !(i8 && j->masked);
  rq.no_i8 = i8 || j->no_i8;
  int rc = job_enqueue(s, j, rq);
  if (j->counted) {
    s->inflight.fetch_sub(1);
    j->counted = false;
  }
  if (rc) return rc;
  HIPCHK(hipEventSynchronize(c->ev_done));
  HIPCHK(hipGetLastError());
  if (i8 && j->store == RowStore::F16) return redo_overflowed_scan(s, j);
  return TSH_OK;
}

// A finished cursor job whose floor pass (or count job whose window pass) found more undecided rows than its side list holds (ties by the thousand) is
// redone once with a list sized to the count it reported: the same scan over the same rows finds the same count.
int redo_after_side(Shard *s, Job *j) {
  Ctx *c = j->c;
  c->side_dirty = false;  // (finished: A2 left the context's other count word at zero)
  const int64_t n = c->h_side[0].id;
  // a job with rows per group that ran its device passes: the marked groups against its slots -- more, and it runs again on
  // the exact-all route --, the member rows against its segment space.  Segments that did not fit sent nothing on, so that
  // redo's side list gets room for every member: the pick sends on members only
  const bool rows_job = j->grouped && j->group_rows > 0;
  const int64_t marked = rows_job ? (int64_t)c->h_side[0].s0 : 0, members = rows_job ? (int64_t)c->h_side[0].s1 : 0;
  const bool slots_over = rows_job && marked > std::min<int64_t>(group_rows_slots(j->k), c->gr_slots);
  const bool seg_over = rows_job && !slots_over && members > c->gr_seg_cap;
  if (rows_job && !j->rows_redone) s->c_grows_marked += marked;
  if (n <= c->side_cap && !slots_over && !seg_over) return TSH_OK;
  if (j->after_redone || j->rows_redone)
    return set_err(TSH_E_HIP, "a cursor search's side list overflowed twice (%lld rows): internal error", (long long)n);
  (rows_job           ? s->c_grows_redone
   : j->group_after   ? s->c_gafter_redone
   : j->grouping      ? s->c_grouped_redone
   : j->counting      ? s->c_count_redone
                      : s->c_after_redone)++;
  const Cursor cur = j->after;
  JobReq rq(j->redo_query, j->k, j->entries);
  rq.mask = j->redo_mask;
  rq.mask_dies = !j->redo_words.empty() && j->redo_mask.words == j->redo_words.data();
  rq.dev_target = j->dev_target;  // (Job::leave_overflow stays with the job)
  rq.last_of_call = true;
  rq.tag = j->tag;
  rq.after = j->has_after ? &cur : nullptr;
  rq.count = j->counting;
  rq.count_thr = j->count_thr;
  rq.groups = j->gpart;
  rq.group_after = j->group_after;
  rq.exact_all = j->exact_all || slots_over;
  rq.group_rows = j->group_rows;
  rq.rows_redone = rows_job;
  rq.seg_want = seg_over ? round_up(members, 1024) : 0;
  rq.side_want = slots_over ? 0 : round_up(std::max(n, seg_over ? members : 0), 1024);
  int rc = job_enqueue(s, j, rq);
  if (j->counted) {
    s->inflight.fetch_sub(1);
    j->counted = false;
  }
  if (rc) return rc;
  HIPCHK(hipEventSynchronize(c->ev_done));
  HIPCHK(hipGetLastError());
  if (!(j->floored || j->windowed || j->grouped)) return TSH_OK;  // (redone on the exact-all route: no side list this time)
  return redo_after_side(s, j);
}

// Waits for a job; afterwards c->h_block / c->d_block hold the final block
// (and *spill every candidate when they did not fit); *extra gets the quarantined rows' entries.
int job_finish(Shard *s, Job *j, std::vector<BlockEntry> *spill, std::vector<BlockEntry> *extra) {
  Ctx *c = j->c;
  if (j->counted) {
    s->inflight.fetch_sub(1);
    j->counted = false;
  }
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipEventSynchronize(c->ev_done));
  HIPCHK(hipGetLastError());
  if (j->i4) scan_i4_account(s, j);
  if (j->store != RowStore::F32) {
    int rc = redo_overflowed_scan(s, j);
    if (rc) return rc;
  }
  if (j->floored || j->windowed || j->grouped) {
    int rc = redo_after_side(s, j);
    if (rc) return rc;
  }
  if (j->timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) {
      std::lock_guard<std::mutex> lk(s->ctx_mu);
      s->scan_us_sum += (double)ms * 1e3;
      s->scan_us_samples++;
    }
    j->timed = false;
  }
  BlockHeader *h = reinterpret_cast<BlockHeader *>(c->h_block);
  if (j->windowed) {  // (no kernel of a windowed count wrote the block: it is empty, the rows are in `certain` and the side list)
    memset(h, 0, sizeof *h);
    h->entries = (uint32_t)j->entries;
  }
#ifdef TSH_PROBES
  if (j->route.exact && probe_env("TSH_X2_TRACE"))
    fprintf(stderr, "[x2] keys %.2f select %.2f entries %.2f us, %u histogram rounds, %u ranked, %u out adds %.2f scan %.2f\n", h->tau_key * 0.01,
            h->band_key * 0.01, h->tiles_hit * 0.01, h->pad[2], h->pad[3], h->count, (h->pad[0] >> 16) * 0.01, (h->pad[0] & 0xFFFF) * 0.01);
#endif
  if ((h->flags & FLAG_LIST_OVERFLOW) && j->leave_overflow && j->dev_target) {
    s->c_cands += std::min(h->count, h->entries);  // (the block stays as it is: see Job::leave_overflow)
  } else if ((h->flags & FLAG_LIST_OVERFLOW) && (j->route.exact || j->store == RowStore::I8)) {
    // The wide pick emits every row up to its cut bin: ties by the hundred, or a k-th neighbour outside the histogram's
    // window, and the bin holds more rows than the block.  The keys and sums of all entries are still in the context:
    // exact_select_kernel ranks them and writes exactly min(k, live rows) entries -- into a block exact_applies sized for
    // k, so THAT cannot overflow (should the invariant ever slip: an error, never the wide-band pass, for which the
    // context holds no f32 keys).
    if (!j->route.picked) return set_err(TSH_E_HIP, "the exact path's block overflowed (%u of %u entries): internal error", h->count, h->entries);
    hipStream_t st = s->aux_stream;
    exact_select_kernel<<<1, 1024, 0, st>>>(j->xsel);
    if (!j->quar_sel.empty() && j->dev_target) launch_quarantine_append(s, c, j, st);  // (the block's count was rewritten)
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    s->c_pick_redone++;
    if (h->flags & FLAG_LIST_OVERFLOW)
      return set_err(TSH_E_HIP, "the exact path's block overflowed (%u of %u entries): internal error", h->count, h->entries);
    s->c_cands += h->count;
  } else if (h->flags & FLAG_LIST_OVERFLOW) {
    int rc = run_fallback(s, j, h->band_key, spill);  // keys[] of this query are still in the context
    if (rc) return rc;
    if (j->side_in_block() || (j->dev_target && !j->quar_sel.empty())) {  // the fallback rewrote the device block: append again
      if (j->side_in_block()) launch_after_side_append(s, c, j, s->aux_stream, nullptr);
      if (!j->quar_sel.empty()) launch_quarantine_append(s, c, j, s->aux_stream);
      HIPCHK(hipStreamSynchronize(s->aux_stream));
      HIPCHK(hipGetLastError());
    }
  } else {
    s->c_cands += h->count;
  }
  if (!j->quar_sel.empty() && !j->dev_target) {  // the quarantined rows join the candidates
    if (!extra) return set_err(TSH_E_BAD_ARG, "no room for the quarantined rows' entries");
    extra->clear();
    for (uint32_t i : j->quar_sel) extra->push_back(c->h_quar[i]);
  }
  if (j->group_after) {
    (j->counting ? s->c_gcount : s->c_gafter)++;
    if (j->route.band.force_all) s->c_gafter_all++;
  } else if (j->grouping && j->group_rows > 0) {
    s->c_grows++;
    if (!j->grouped) s->c_grows_all++;
  } else if (j->grouping) {
    s->c_grouped++;
    if (!j->grouped) s->c_grouped_nodev++;
  } else if (j->counting) {
    s->c_count++;
    if (!j->windowed) s->c_count_nowindow++;
  } else if (j->has_after) {
    s->c_after++;
    if (j->after_skip || (j->route.band.force_all && !j->after.from_start())) s->c_after_nofloor++;
  }
  if (j->side_in_block()) {  // (shard mode: the side rows' entries are in the device block already)
    (j->grouped ? s->c_grouped_side : s->c_after_side) += c->h_side[0].id;
  } else if (j->floored || j->windowed || j->grouped) {  // the rows the floor / window / side pass could not decide join the candidates too
    if (!extra) return set_err(TSH_E_BAD_ARG, "no room for the side list's entries");
    if (j->quar_sel.empty()) extra->clear();
    const uint32_t side_n = (uint32_t)c->h_side[0].id;
    extra->insert(extra->end(), c->h_side + 1, c->h_side + 1 + side_n);
    (j->group_rows > 0 ? s->c_grows_side
     : j->group_after  ? s->c_gafter_side
     : j->grouped      ? s->c_grouped_side
     : j->windowed     ? s->c_count_side
                       : s->c_after_side) += side_n;
    if (j->windowed) j->certain = (int64_t)c->h_side[0].s0;
  }
  s->c_searches++;
  return TSH_OK;
}

// An enqueued job that will not be finished (something else of its call failed): settled -- its kernels have run out and
// it no longer counts in Shard::inflight -- and then abandoned, its context back in the pool
inline void job_settle(Shard *s, Job *j) {
  if (!j->counted) return;
  hipEventSynchronize(j->c->ev_done);
  s->inflight.fetch_sub(1);
  j->counted = false;
}
inline void job_abandon(Shard *s, Job *j) {
  if (!j->c) return;
  job_settle(s, j);
  ctx_release(s, j->c);
  j->c = nullptr;
}

// One shard's candidates of one query, as the finaliser takes them: the spill if the wide-band pass made one, else the
// block's own entries, then the extra entries (quarantined rows, a side list) if there are any.  -> lists written
inline size_t shard_lists(const uint8_t *block, const std::vector<BlockEntry> *spill, const std::vector<BlockEntry> *extra,
                          EntryList out[2]) {
  size_t n = 0;
  out[n++] = spill && !spill->empty() ? EntryList{spill->data(), (uint32_t)spill->size()} : block_list(block);
  if (extra && !extra->empty()) out[n++] = EntryList{extra->data(), (uint32_t)extra->size()};
  return n;
}

struct SearchOut {
  uint8_t *h_blocks = nullptr;  // host mode: nq blocks (caller memory)
  std::vector<std::vector<BlockEntry>> *spill = nullptr;
  std::vector<std::vector<BlockEntry>> *extra = nullptr;  // per query: entries of the quarantined rows
  int32_t q_base = 0;  // batched path: this part's query 0 is (*extra)[q_base]
  uint8_t *d_blocks = nullptr;  // device mode
  hipStream_t user_stream = nullptr;
  // batched path, host mode: called as soon as the blocks of queries [q0, q1) have arrived from the GPU, while it
  // still re-ranks the next chunk; query q's block is at base + q * block bytes (the batch's own pinned buffer:
  // valid during the call only -- with a callback the blocks are NOT copied to h_blocks); skip[q] != 0 marks
  // queries the single-query path will redo (those do land in h_blocks)
  // (mag_a[q]: query_mag_a of query q, computed while the queries were prepared)
  std::function<void(int32_t q0, int32_t q1, const char *skip, const uint8_t *base, const double *mag_a)> on_chunk;
  // batched path, host mode: the caller takes FINAL results (threshold fin_thr applied, ordered, cut to k) -- the
  // device finalises whatever it can (rerank_final_kernel) and hands over ids / distances (k per query) and counts of
  // queries [q0, q1), indexed like the call's queries; what it cannot goes through on_chunk as before
  double fin_thr = std::nan("");
  std::function<void(int32_t q0, int32_t q1, const char *skip, const int64_t *ids, const double *dist, const int32_t *cnt)> on_final;
  // single-query pipeline, device mode (progressive shard search): called once query q's block is final in
  // d_blocks (its job finished on the host, fallback included), from whichever submitting thread ran it.  With it
  // set the submitting threads take the queries interleaved (q = t, t + T, ...), so blocks become final in order
  std::function<void(int32_t q)> on_done;
  // ... and once query q's kernels are all ENQUEUED: `done` is the event behind the last writer of its block
  // (`where`: the stream that event was recorded on -- kernels of one stream finish in order; `seq`: the job's place
  // in the order the device's streams were fed, which with two submitting threads is not the queries' order)
  std::function<void(int32_t q, hipEvent_t done, hipStream_t where, uint64_t seq)> on_enqueued;
  // single-query pipeline, host mode, ONE submitting thread (shard_search_blocks: scans long enough that the thread has
  // time to spare between two of them): called right after query q's job finished, with the context's own pinned block
  // and the query's spill and extra lists -- the caller finalises q while the GPU scans the next queries.  The block is
  // then NOT copied to h_blocks.  Calls that two threads submit do not use it: their blocks land in h_blocks as ever
  std::function<void(int32_t q, const uint8_t *block, const std::vector<BlockEntry> *spill, const std::vector<BlockEntry> *extra)> on_block;
  uint32_t tag = 0;  // generation stamped into the blocks' headers (BlockHeader.pad[1])
  bool leave_overflow = false;  // device mode: see Job::leave_overflow
  // single-query pipeline, host or device mode: a cursor per query (tsh_search_after, tsh_search_shard_after), or none
  Cursors after;
  // ... host mode, a count per query (tsh_search_count): count_out[q] = the rows of this shard that pass count_thr and
  // follow the query's cursor, if any.  No block leaves the shard (h_blocks NULL); spill / extra are needed
  int64_t *count_out = nullptr;
  double count_thr = 0;
  // ... host mode, a grouped search (tsh_search_grouped): this shard's part of the groups handle
  const GroupPart *groups = nullptr;
  // ... a grouped cursor search or a group count (tsh_search_grouped_after, tsh_search_grouped_count): `after` and
  // `count_out` hold for groups.  A group count leaves count_out[q] = the groups counted on the device only, and blocks,
  // spill and extra to the caller: groups may span shards, so the group-count step runs once over every shard's entries.
  // exact_all: JobReq::exact_all for every job of the call
  bool group_after = false, exact_all = false;
  // ... a grouped search with rows per group (tsh_search_grouped_rows): JobReq::group_rows for every job of the call
  int32_t group_rows = 0;
};

// One submitting thread's share of a multi-query call: queries [q0, q1) of the call, at most
// `depth` of them in flight on separate contexts so one query's select / rerank / copies hide
// behind the next query's scan.
int shard_search_slice(Shard *s, const float *queries, int32_t q0, int32_t q1, int32_t k, const ShardMask &mask,
                       int32_t entries, SearchOut *out, int depth, int32_t stride = 1, bool sole = false) {
  // (sole: this thread submits the whole call -- out->on_block, if set, takes the blocks)
  // this thread's queries: q0, q0 + stride, ... below q1 (cnt of them; i-th = q0 + i * stride)
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  const int32_t cnt = q1 > q0 ? (q1 - q0 + stride - 1) / stride : 0;
  depth = std::max(1, std::min(depth, std::min(cnt, MAX_CTX)));
  std::vector<Job> jobs((size_t)depth);
  int rc = TSH_OK;
  int32_t submitted = 0, finished = 0;
  auto release_all = [&]() {
    for (auto &j : jobs) job_abandon(s, &j);
  };
  while (finished < cnt) {
    while (submitted < cnt && submitted - finished < depth) {
      // wait for a context only while holding none: callers that each hold some and wait for
      // more would deadlock on the shard's fixed pool
      Ctx *c = ctx_acquire(s, submitted == finished);
      if (!c) break;
      Job &j = jobs[(size_t)(submitted % depth)];
      j.c = c;
      j.leave_overflow = out->leave_overflow;
      const int32_t q = q0 + submitted * stride;
      JobReq rq(queries + (size_t)q * s->dim, k, entries);
      rq.mask = mask;
      rq.dev_target = out->d_blocks ? out->d_blocks + (size_t)q * bb : nullptr;
      rq.more_coming = cnt > 1;
      rq.last_of_call = cnt > 1 && submitted == cnt - 1;
      rq.tag = out->tag;
      Cursor cur;
      rq.after = out->after.at(q, &cur);
      rq.count = out->count_out != nullptr;
      rq.count_thr = out->count_thr;
      rq.groups = out->groups;
      rq.group_after = out->group_after;
      rq.exact_all = out->exact_all;
      rq.group_rows = out->group_rows;
      rc = job_enqueue(s, &j, rq);
      if (rc) {
        release_all();
        return rc;
      }
      ++submitted;
      if (out->on_enqueued) out->on_enqueued(q, c->ev_done, j.last_stream, j.enq_seq);
    }
    Job &j = jobs[(size_t)(finished % depth)];
    const int32_t q = q0 + finished * stride;
    std::vector<BlockEntry> *sp = out->spill ? &(*out->spill)[(size_t)q] : nullptr;
    std::vector<BlockEntry> *ex = out->extra ? &(*out->extra)[(size_t)q] : nullptr;
    rc = job_finish(s, &j, sp, ex);
    if (rc) {
      release_all();
      return rc;
    }
    if (sole && out->on_block) out->on_block(q, j.c->h_block, sp, ex);
    else if (out->h_blocks) memcpy(out->h_blocks + (size_t)q * bb, j.c->h_block, bb);
    if (out->count_out && out->group_after) {
      out->count_out[q] = j.certain;
    } else if (out->count_out) {  // the rows counted on the device, and whatever reached the host with its exact sums
      EntryList two[2];
      const size_t n_lists = shard_lists(j.c->h_block, sp, ex, two);
      Cursor cur;
      out->count_out[q] = j.certain + count_entries(s->metric, s->dim, queries + (size_t)q * s->dim, out->count_thr, two, n_lists,
                                                    out->after.at(q, &cur));
    }
    ctx_release(s, j.c);
    j.c = nullptr;
    ++finished;
    if (out->on_done) out->on_done(q);
  }
  return TSH_OK;
}

// nq single-query searches.  Each query costs the host about seven runtime calls (three
// launches, events, a wait); on a small shard (a row range of a multi-GPU index) that is
// longer than the scan itself, so larger calls are submitted from a few threads at once.
// Caller holds s->mu shared.
int shard_search_blocks(Shard *s, const float *queries, int32_t nq, int32_t k, const MaskSrc &mask,
                        int32_t entries, SearchOut *out, int depth) {
  // (the calling thread's buffers, kept between calls: a lone masked query does not pay for two allocations)
  static thread_local std::vector<uint64_t> mask_words;
  static thread_local std::vector<uint32_t> list_ids;
  // (made here once for all queries of the call)
  const ShardMask m = resolve_mask(s, mask, k, entries, &mask_words, &list_ids);
  // short scans (small shards, selective masks) are bound by the submitting thread's ~25 us per query: two threads
  const int64_t scan_bytes = (m.rows_est > 0 ? m.rows_est : s->rows) * s->ld * 4;
  static const int forced_threads = probe_env("TSH_SUBMIT_THREADS") ? atoi(probe_env("TSH_SUBMIT_THREADS")) : 0;
  const int want = forced_threads > 0 ? forced_threads : (scan_bytes <= (160ll << 20) ? 2 : SUBMIT_THREADS);
  const int T = std::min(want, nq / 8);
  // (on_block only where one thread is the rule, not where a short call happens to get one: a thread that is the
  // bottleneck -- short scans -- has no time to finalise in)
  if (T <= 1) return shard_search_slice(s, queries, 0, nq, k, m, entries, out, depth, 1, /*sole*/ want <= 1);
  std::vector<int> rcs((size_t)T, TSH_OK);
  std::vector<std::string> errs((size_t)T);
  const int per_depth = std::max(2, depth / T);
  const bool interleave = (bool)out->on_done;  // a progressive search wants its blocks final in query order
  auto run = [&](int t) {
    const int32_t q0 = interleave ? t : (int32_t)((int64_t)nq * t / T);
    const int32_t q1 = interleave ? nq : (int32_t)((int64_t)nq * (t + 1) / T);
    rcs[(size_t)t] = shard_search_slice(s, queries, q0, q1, k, m, entries, out, per_depth, interleave ? T : 1);
    if (rcs[(size_t)t]) errs[(size_t)t] = g_err;
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; ++t) th.emplace_back(run, t);
  run(0);
  for (auto &x : th) x.join();
  for (int t = 0; t < T; ++t)
    if (rcs[(size_t)t]) {
      g_err = errs[(size_t)t];
      return rcs[(size_t)t];
    }
  return TSH_OK;
}

#include "tsh_host_batch.inl.h"  // batched (matrix-core) path, host side

}  // namespace

// ============================================================================
// an un-waited asynchronous search (tsh_search_submit): one job per shard; the
// shards stay share-locked until the wait so appends cannot move the rows
struct Ticket {
  int32_t k = 0, entries = 0;
  bool has_after = false;  // tsh_search_submit_after: the wait's finaliser filters by the cursor
  Cursor after;
  std::vector<float> query;
  std::vector<Job> jobs;
  std::vector<std::shared_lock<RwLock>> locks;
};

struct tsh_index {
  int dim = 0, metric = 0;
  int64_t rows_per_shard = 0;  // multi-device split (0: single shard)
  std::vector<std::unique_ptr<Shard>> shards;
  std::mutex mu;  // serialises append routing
  std::mutex tk_mu;
  std::vector<std::unique_ptr<Ticket>> tickets;
  std::atomic<int> tickets_open{0};  // submitted, not yet waited for: each holds one context per shard
  std::atomic<int32_t> batch_min_nq{1};  // 0 never, 1 by estimated cost, n >= 2: from n queries per call on
  std::vector<tsh_mask *> masks;  // live mask handles made for this index (guarded by g_mask_mu): orphaned by destroy
  std::vector<struct tsh_groups *> groups;  // ... and live groups handles, the same way
  std::vector<struct tsh_attr *> attrs;     // ... and live attribute handles
  std::vector<struct tsh_tags *> tags;      // ... and live tag handles
  std::unique_ptr<ShardWorkers> workers;  // multi-device handles: one persistent host thread per further shard
  // result-block buffers of multi-query calls, kept between calls: a fresh 6 MB allocation per call spends
  // ~0.3 ms in page faults when it is first written
  std::mutex pool_mu;
  std::vector<std::pair<size_t, std::unique_ptr<uint8_t[]>>> block_pool;
  std::unique_ptr<uint8_t[]> take_blocks(size_t bytes, size_t *cap) {
    std::lock_guard<std::mutex> lk(pool_mu);
    for (size_t i = 0; i < block_pool.size(); ++i)
      if (block_pool[i].first >= bytes) {
        *cap = block_pool[i].first;
        std::unique_ptr<uint8_t[]> p = std::move(block_pool[i].second);
        block_pool.erase(block_pool.begin() + (long)i);
        return p;
      }
    *cap = bytes;
    return std::unique_ptr<uint8_t[]>(new uint8_t[bytes]);
  }
  void give_blocks(std::unique_ptr<uint8_t[]> p, size_t cap) {
    std::lock_guard<std::mutex> lk(pool_mu);
    if (block_pool.size() < 4 && cap <= ((size_t)64 << 20)) block_pool.emplace_back(cap, std::move(p));
  }
};

namespace {

// Shared lock of a shard on behalf of a call on `idx`.  A handle with asynchronous tickets open passes a
// waiting writer (RwLock: queueing behind it would deadlock ticket holder, writer and this call).
inline std::shared_lock<RwLock> share(tsh_index *idx, Shard *s) {
  s->mu.lock_shared_gate(idx->tickets_open.load() > 0);
  return std::shared_lock<RwLock>(s->mu, std::adopt_lock);
}

int make_shard(int dim, int metric, int device, int64_t row_base, int64_t cap_rows,
               std::unique_ptr<Shard> *out) {
  std::unique_ptr<Shard> s(new Shard());
  s->device = device;
  s->dim = dim;
  s->metric = metric;
  s->ld = round_up(dim, 4);
  s->nch = pick_nch((int)(s->ld / 4));
  s->row_base = row_base;
  int rc = shard_init(s.get());
  if (rc) return rc;
  s->batch = new BatchCtx();
  s->batch2 = new BatchCtx();
  if (cap_rows > 0) {
    rc = shard_reserve(s.get(), cap_rows);
    if (rc) return rc;
  }
  *out = std::move(s);
  return TSH_OK;
}

void shard_destroy(Shard *s) {
  hipSetDevice(s->device);
  for (auto &c : s->ctx_all) ctx_free_all(c.get());
  for (BatchCtx **b : {&s->batch, &s->batch2})
    if (*b) {
      batch_free(*b);
      delete *b;
      *b = nullptr;
    }
  // (streams are the device's, not the shard's; the last shard on a device takes the CU-masked ones along)
  hipFree(s->d_rows);
  hipFree(s->d_inv_norm);
  hipFree(s->d_sqnorm);
  hipFree(s->d_live);
  hipFree(s->d_split);
  s->rows16.release(s);
  s->rows8.release(s);
  s->rows4.release(s);
  hipFree(s->d_perm);
  hipFree(s->d_psq);
  hipFree(s->d_hub);
  hipFree(s->d_hub_ids);
  hipFree(s->d_hub_sq);
  hipFree(s->d_stats);
  hipFree(s->d_tmp_u32);
  hipFree(s->d_del_ids);
  hipFree(s->d_quar);
  hipFree(s->d_irr);
  hipFree(s->d_facet);
  if (s->holds_streams) {
    s->holds_streams = false;
    device_streams_release(s->device);
  }
}

int check_create_args(int32_t dim, int32_t metric, int64_t cap, tsh_index **out) {
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (dim <= 0 || dim > MAX_DIM_SCAN)
    return set_err(TSH_E_BAD_ARG, "dim %d outside [1,%d]", dim, MAX_DIM_SCAN);
  if (metric < 0 || metric > 2) return set_err(TSH_E_BAD_ARG, "metric %d unknown", metric);
  if (cap < 0) return set_err(TSH_E_BAD_ARG, "capacity_rows < 0");
  if (device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return TSH_OK;
}

Shard *shard_for_row(tsh_index *idx, int64_t gid) {
  if (idx->shards.size() == 1) return idx->shards[0].get();
  int64_t g = idx->rows_per_shard > 0 ? gid / idx->rows_per_shard : 0;
  if (g >= (int64_t)idx->shards.size()) g = (int64_t)idx->shards.size() - 1;
  if (g < 0) g = 0;
  return idx->shards[(size_t)g].get();
}

int index_append(tsh_index *idx, int64_t first, int64_t n, const float *rows, bool dev) {
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (n < 0 || first < 0) return set_err(TSH_E_BAD_ARG, "negative row range");
  if (n == 0) return TSH_OK;
  if (!rows) return set_err(TSH_E_BAD_ARG, "rows is NULL");
  if (dev && idx->shards.size() > 1)
    return set_err(TSH_E_BAD_ARG, "append_device needs a single-device handle");
  std::lock_guard<std::mutex> lk(idx->mu);
  int64_t done = 0;
  while (done < n) {
    int64_t gid = first + done;
    Shard *s = shard_for_row(idx, gid);
    int64_t take = n - done;
    if (idx->shards.size() > 1 && s != idx->shards.back().get()) {
      int64_t end = s->row_base + idx->rows_per_shard;
      take = std::min(take, end - gid);
    }
    if (gid < s->row_base) return set_err(TSH_E_BAD_ARG, "row id %lld below shard base", (long long)gid);
    std::unique_lock<RwLock> xl(s->mu);
    int rc = shard_append(s, gid - s->row_base, take, rows + (size_t)done * idx->dim, dev);
    if (rc) return rc;
    done += take;
  }
  return TSH_OK;
}

}  // namespace

// ---- mask handles ---------------------------------------------------------------------------------------------
struct tsh_mask {
  tsh_index *idx = nullptr;   // nullptr: orphaned -- its index was destroyed first (parts freed then)
  std::vector<uint8_t> bits;  // the caller's GLOBAL bitmap (its own copy; zero-extended as the index grows)
  std::mutex mu;              // builds / rebuilds of the parts
  std::vector<std::unique_ptr<MaskPart>> parts;  // one per shard of the index
};

// ---- groups handles -------------------------------------------------------------------------------------------
struct tsh_groups {
  tsh_index *idx = nullptr;       // nullptr: orphaned -- its index was destroyed first (parts freed then)
  std::vector<int32_t> group_of;  // the caller's array by GLOBAL row id (its own copy: the finaliser reads it, 4 B per row)
  int32_t n_groups = 0;
  std::shared_mutex use_mu;  // searches: shared, for the whole call; tsh_groups_set: exclusive
  std::mutex mu;             // builds / rebuilds of the parts
  std::vector<std::unique_ptr<GroupPart>> parts;  // one per shard of the index
  // does a group have rows in the row ranges of two shards?  (groups_update_spans: set with the array -- by create, and by
  // tsh_groups_set, which marks every part for its rebuild -- and read by the grouped cursor searches and group counts,
  // whose per-shard rule does not hold then: tsh_group_after_rule.h)
  bool spans = false;
};

// ---- attribute handles ----------------------------------------------------------------------------------------
struct tsh_attr {
  tsh_index *idx = nullptr;     // nullptr: orphaned -- its index was destroyed first (parts freed then)
  std::vector<int64_t> values;  // the caller's column by GLOBAL row id (its own copy: the parts are sliced from it)
  std::shared_mutex use_mu;     // tsh_mask_create_range / _where: shared, for the whole call; tsh_attr_set: exclusive
  std::mutex mu;                // builds / rebuilds of the parts
  std::vector<std::unique_ptr<AttrPart>> parts;  // one per shard of the index
};

// ---- tag handles ------------------------------------------------------------------------------------------------------
struct tsh_tags {
  tsh_index *idx = nullptr;     // nullptr: orphaned -- its index was destroyed first (parts freed then)
  TagsColumn col;               // the caller's column by GLOBAL row id, normalised (tsh_tags_plan.h): the parts are sliced from it
  std::shared_mutex use_mu;     // tsh_mask_create_tags: shared, for the whole call; tsh_tags_set: exclusive
  std::mutex mu;                // builds / rebuilds of the parts
  std::vector<std::unique_ptr<TagsPart>> parts;  // one per shard of the index
};

namespace {

// Settles a mask's destroy against its index's (either may come first, from any thread): index -> masks lists, every
// mask's idx, and the parts' device buffers while an index frees them.  Held by tsh_mask_kept too, so an index cannot
// be destroyed under a count.
std::mutex g_mask_mu;

// ---- what the four handle kinds share: tsh_mask, tsh_groups, tsh_attr, tsh_tags ------------------------------------------
// Each has idx, mu and parts; a kind adds its part struct (with free_bufs), a build_part overload and a live_list overload.
template <class H>
using PartOf = typename decltype(H::parts)::value_type::element_type;

std::vector<tsh_mask *> &live_list(tsh_index *idx, const tsh_mask *) { return idx->masks; }
std::vector<tsh_groups *> &live_list(tsh_index *idx, const tsh_groups *) { return idx->groups; }
std::vector<tsh_attr *> &live_list(tsh_index *idx, const tsh_attr *) { return idx->attrs; }
std::vector<tsh_tags *> &live_list(tsh_index *idx, const tsh_tags *) { return idx->tags; }

int build_part(tsh_mask *m, MaskPart *p, Shard *s);
int build_part(tsh_groups *g, GroupPart *p, Shard *s);
int build_part(tsh_attr *a, AttrPart *p, Shard *s);
int build_part(tsh_tags *t, TagsPart *p, Shard *s);

// A part's device buffers go (built_rows with them: nothing reads it afterwards -- an orphan is refused by its idx ==
// nullptr before any part is read, and a failed create deletes the handle)
template <class P>
void part_free(P *p) {
  if (hipSetDevice(p->device) != hipSuccess) return;
  p->free_bufs();
  p->built_rows.store(-1);
}
// ... every part's, and the error text stays as it was
template <class H>
void free_parts(H *h) {
  const std::string keep = g_err;
  for (auto &p : h->parts) part_free(p.get());
  g_err = keep;
}

// Shard g's part of a handle, current for the rows the shard has; nullptr + *rc on failure.  Caller holds s->mu shared
// and, where the kind has one, h->use_mu shared.  A part built for other rows (the shard grew), or marked -1 by the
// kind's _set, is rebuilt under h->mu first.  Appends take the shard exclusively and _set takes the handle exclusively, so
// no search or kernel that reads the old buffers is running: whoever starts after either passes through here first
template <class H>
const PartOf<H> *current_part(H *h, size_t g, Shard *s, int *rc) {
  *rc = TSH_OK;
  PartOf<H> *p = h->parts[g].get();
  if (p->built_rows.load(std::memory_order_acquire) == s->rows) return p;
  std::lock_guard<std::mutex> lk(h->mu);
  if (p->built_rows.load(std::memory_order_acquire) != s->rows) {
    *rc = build_part(h, p, s);
    if (*rc) return nullptr;
  }
  return p;
}

// A new handle's parts: one for every shard of h->idx, each made by build(g, s, part) under h->mu and the shard's shared
// lock (a handle exists to take this work out of the searches).  On failure the parts are freed and g_err is build's
template <class H, class F>
int make_parts(H *h, F &&build) {
  tsh_index *idx = h->idx;
  for (size_t g = 0; g < idx->shards.size(); ++g) h->parts.emplace_back(new PartOf<H>());
  int rc = TSH_OK;
  {
    std::lock_guard<std::mutex> lk(h->mu);
    for (size_t g = 0; g < idx->shards.size() && rc == TSH_OK; ++g) {
      Shard *s = idx->shards[g].get();
      std::shared_lock<RwLock> sl = share(idx, s);
      rc = build(g, s, h->parts[g].get());
    }
  }
  if (rc) free_parts(h);
  return rc;
}
template <class H>
int make_parts(H *h) {
  return make_parts(h, [h](size_t, Shard *s, PartOf<H> *p) { return build_part(h, p, s); });
}

// The end of every create: the index learns of the handle, the caller gets it
template <class H>
int32_t register_handle(std::unique_ptr<H> &h, H **out) {
  {
    std::lock_guard<std::mutex> lk(g_mask_mu);
    live_list(h->idx, h.get()).push_back(h.get());
  }
  *out = h.release();
  return TSH_OK;
}

template <class H>
int32_t destroy_handle(H *h) {
  if (!h) return TSH_OK;
  {
    std::lock_guard<std::mutex> lk(g_mask_mu);
    if (tsh_index *idx = h->idx) {  // (an orphan's parts went with its index)
      auto &live = live_list(idx, h);
      live.erase(std::remove(live.begin(), live.end(), h), live.end());
      free_parts(h);
    }
  }
  delete h;
  return TSH_OK;
}

// tsh_index_destroy, g_mask_mu held: handles still alive are orphaned -- their device parts go now, the structs stay for
// their own destroy
template <class H>
void orphan_handles(std::vector<H *> &live) {
  for (H *h : live) {
    free_parts(h);
    h->idx = nullptr;
  }
  live.clear();
}

// tsh_groups_set, tsh_attr_set, tsh_tags_set behind their argument checks.  Locks: g_mask_mu (the index cannot be destroyed
// under the call), then idx->mu as an append does, then h->use_mu exclusive.  check() runs before the last two; change()
// alters the host copy under all three, and every part is marked for its rebuild by the next reader of each shard
template <class H, class C, class F>
int32_t set_column(H *h, const char *orphaned, int64_t n, C &&check, F &&change) {
  std::lock_guard<std::mutex> hold(g_mask_mu);
  tsh_index *idx = h->idx;
  if (!idx) return set_err(TSH_E_BAD_ARG, "%s", orphaned);
  int rc = check();
  if (rc) return rc;
  if (n == 0) return TSH_OK;
  std::lock_guard<std::mutex> lk(idx->mu);
  std::unique_lock<std::shared_mutex> xl(h->use_mu);
  rc = change();
  if (rc) return rc;
  for (auto &p : h->parts) p->built_rows.store(-1, std::memory_order_release);
  return TSH_OK;
}
inline int no_check() { return TSH_OK; }

// The second half of a part's build, whichever way its words were obtained (sliced from the handle's bitmap and uploaded:
// build_part; or written by a W kernel and copied back: mask_device_part): p->h_words and p->words.d hold the
// same n_tiles words (an upload may still be in flight on s->aux_stream; a copy back is done).  Counts them on the host once -- the
// batched path and the quarantined rows read words and prefix there -- and compacts a selective mask's list on the device
// (tsh_mask.hip.h).  Returns with the stream drained and the part current for `rows`.
int mask_finish_part(MaskPart *p, Shard *s, int64_t rows, int32_t n_tiles) {
  p->pre.assign((size_t)n_tiles + 1, 0);
  for (int32_t t = 0; t < n_tiles; ++t) p->pre[(size_t)t + 1] = p->pre[(size_t)t] + __builtin_popcountll(p->h_words[(size_t)t]);
  p->kept = p->pre[(size_t)n_tiles];
  p->n_tiles = n_tiles;
  p->list_padded = 0;
  hipStream_t st = s->aux_stream;
  // the list: wherever a search may scan the kept rows as one (row_list_pays: few enough for the exact path at any
  // k and row width, or fewer than one row in list_div) -- compacted on the device, in id order
  const int64_t padded = round_up(p->kept, 64);
  const int64_t list_div = mask_list_div();
  const bool want_list = p->kept > 0 && rows >= 4096 && list_div > 0 && padded < 0x7FFFFFC0ll &&
                         (padded <= EX_MAX_ROWS || p->kept * list_div <= rows);
  if (want_list) {
    const int32_t n_blocks = (n_tiles + MASK_BLOCK_WORDS - 1) / MASK_BLOCK_WORDS;
    int rc = p->bsum.reserve(n_blocks + 1, 64, &p->bytes, n_blocks / 8);
    if (rc) return rc;
    rc = p->list.reserve(padded, 1024, &p->bytes);
    if (rc) return rc;
    uint32_t *d_total = p->bsum.d + n_blocks;
    mask_block_count_kernel<<<n_blocks, MASK_BLOCK_WORDS, 0, st>>>(p->words.d, n_tiles, p->bsum.d);
    mask_compact_kernel<<<n_blocks, MASK_BLOCK_WORDS, 0, st>>>(p->words.d, n_tiles, p->bsum.d, p->list.d, d_total);
    if (padded > p->kept)
      HIPCHK(hipMemsetAsync(p->list.d + p->kept, 0xFF, (size_t)(padded - p->kept) * 4, st));
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, d_total, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    if ((int64_t)total != p->kept)  // (the host counted the same words: cannot differ)
      return set_err(TSH_E_HIP, "mask compaction listed %u rows, the mask keeps %lld", total, (long long)p->kept);
    p->list_padded = (int32_t)padded;
  } else {
    HIPCHK(hipStreamSynchronize(st));
  }
  p->built_rows.store(rows, std::memory_order_release);
  return TSH_OK;
}

// (Re)builds one shard's part for the rows the shard has now.  Caller holds s->mu shared (the rows cannot change) and
// m->mu.  The words are sliced from the handle's bitmap on the host and uploaded once; mask_finish_part does the rest.
int build_part(tsh_mask *m, MaskPart *p, Shard *s) {
  HIPCHK(hipSetDevice(s->device));
  p->device = s->device;
  const int64_t rows = s->rows;
  const int32_t n_tiles = (int32_t)((rows + 63) / 64);
  // bits at or beyond the caller's n_bytes are not kept: the handle's copy grows with zeros to what slice_mask reads
  const size_t need = (size_t)((s->row_base + rows + 7) / 8) + 1;
  if (m->bits.size() < need) m->bits.resize(need, 0);
  p->h_words.assign((size_t)n_tiles, 0);
  if (n_tiles > 0) slice_mask(s, m->bits.data(), p->h_words.data(), n_tiles);
  int rc = p->words.reserve(n_tiles, 64, &p->bytes);
  if (rc) return rc;
  if (n_tiles > 0)
    HIPCHK(hipMemcpyAsync(p->words.d, p->h_words.data(), (size_t)n_tiles * 8, hipMemcpyHostToDevice, s->aux_stream));
  return mask_finish_part(p, s, rows, n_tiles);
}

// The mask of a call, as the entries get it: the caller's global bitmap, or a mask handle, or neither
struct CallMask {
  const uint8_t *bytes = nullptr;
  tsh_mask *handle = nullptr;
};
// ... and what shard g's searches take of it: the handle's part for this shard -- resident, rebuilt here if the shard grew
// since -- else the pointer form.  Caller holds s->mu shared and has checked that the handle was made for this index
inline int call_mask_for_shard(const CallMask &m, size_t g, Shard *s, MaskSrc *out) {
  *out = MaskSrc(m.bytes);
  if (!m.handle) return TSH_OK;
  int rc = TSH_OK;
  const MaskPart *mp = current_part(m.handle, g, s, &rc);
  if (!mp) return rc;
  *out = MaskSrc(mp);
  return TSH_OK;
}

// (Re)builds one shard's part for the rows the shard has now: the slice of the handle's array, -1 beyond it.  Caller holds
// s->mu shared, g->use_mu (shared or exclusive) and g->mu
int build_part(tsh_groups *g, GroupPart *p, Shard *s) {
  HIPCHK(hipSetDevice(s->device));
  p->device = s->device;
  p->n_groups = g->n_groups;
  const int64_t rows = s->rows;
  int rc = p->group.reserve(rows, 1024);
  if (rc) return rc;
  if (rows > 0) {
    std::vector<int32_t> slice((size_t)rows, -1);
    const int64_t have = std::min<int64_t>(rows, std::max<int64_t>((int64_t)g->group_of.size() - s->row_base, 0));
    if (have > 0) memcpy(slice.data(), g->group_of.data() + s->row_base, (size_t)have * sizeof(int32_t));
    HIPCHK(hipMemcpyAsync(p->group.d, slice.data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, s->aux_stream));
    HIPCHK(hipStreamSynchronize(s->aux_stream));
  }
  p->built_rows.store(rows, std::memory_order_release);
  return TSH_OK;
}

// (Re)builds one shard's part for the rows the shard has now: the slice of the handle's column, TSH_ATTR_NULL beyond it.
// Caller holds s->mu shared, a->use_mu (shared or exclusive) and a->mu
int build_part(tsh_attr *a, AttrPart *p, Shard *s) {
  HIPCHK(hipSetDevice(s->device));
  p->device = s->device;
  const int64_t rows = s->rows;
  int rc = p->vals.reserve(rows, 1024);
  if (rc) return rc;
  if (rows > 0) {
    const int64_t have = std::min<int64_t>(rows, std::max<int64_t>((int64_t)a->values.size() - s->row_base, 0));
    // (the rows the column names go up from the handle's copy as they lie; only the rows beyond it need a staged NULL)
    if (have > 0)
      HIPCHK(hipMemcpyAsync(p->vals.d, a->values.data() + s->row_base, (size_t)have * sizeof(int64_t), hipMemcpyHostToDevice,
                            s->aux_stream));
    std::vector<int64_t> nulls((size_t)(rows - have), ATTR_NULL);
    if (rows > have)
      HIPCHK(hipMemcpyAsync(p->vals.d + have, nulls.data(), (size_t)(rows - have) * sizeof(int64_t), hipMemcpyHostToDevice,
                            s->aux_stream));
    HIPCHK(hipStreamSynchronize(s->aux_stream));
  }
  p->built_rows.store(rows, std::memory_order_release);
  return TSH_OK;
}

// (Re)builds one shard's part for the rows the shard has now: the slice of the handle's column (tags_slice: rebased
// offsets, the value span as it lies in the handle's copy, the valid words; rows beyond the column are empty spans with
// valid bit 0).  A slice of more than 2^31 - 1 values is refused before anything is allocated.  Caller holds s->mu
// shared, t->use_mu (shared or exclusive) and t->mu
int build_part(tsh_tags *t, TagsPart *p, Shard *s) {
  HIPCHK(hipSetDevice(s->device));
  p->device = s->device;
  const int64_t rows = s->rows;
  TagsSlice sl;
  try {
    if (const int e = tags_slice(t->col, s->row_base, rows, &sl)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for the offsets of %lld rows", (long long)rows);
  }
  const int64_t n_tiles = (int64_t)sl.valid.size();
  int rc = p->off.reserve(rows + 1, 1024, nullptr, rows / 8);
  if (rc == TSH_OK) rc = p->vals.reserve(sl.n_vals, 1024);
  if (rc == TSH_OK) rc = p->valid.reserve(n_tiles, 64);
  if (rc) return rc;
  hipStream_t st = s->aux_stream;
  HIPCHK(hipMemcpyAsync(p->off.d, sl.off.data(), (size_t)(rows + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  if (sl.n_vals > 0)
    HIPCHK(hipMemcpyAsync(p->vals.d, sl.vals, (size_t)sl.n_vals * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (n_tiles > 0)
    HIPCHK(hipMemcpyAsync(p->valid.d, sl.valid.data(), (size_t)n_tiles * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  p->built_rows.store(rows, std::memory_order_release);
  return TSH_OK;
}

// The words of a mask part obtained ON the device (tsh_where.hip.h, tsh_tags.hip.h): one launch over the shard's slice of
// the column(s), combined there with with's words if a handle is given, written straight into p->words.d and copied back
// once into p->h_words; mask_finish_part does the rest, as for an uploaded bitmap.  A term's set (n_set 8-byte entries;
// it outlives the synchronise below) goes up in one copy ahead of the launch, into the tail of the part's own word
// allocation -- the part is new, so the allocation is made here anyway: a call without a set stages nothing and allocates
// no more.  launch(st, rows, n_tiles, d_set, with's words or nullptr) enqueues the one kernel on st.  Caller holds s->mu
// shared, the new handle's mu and the columns' use_mu shared; the columns' parts are current for the shard's rows, and
// with's is made so here (n_tiles words, the bits at or past the last row 0)
template <class F>
int mask_device_part(MaskPart *p, Shard *s, tsh_mask *with, size_t g, const int64_t *set, int32_t n_set, F &&launch) {
  int rc = TSH_OK;
  const MaskPart *wp = with ? current_part(with, g, s, &rc) : nullptr;
  if (with && !wp) return rc;
  HIPCHK(hipSetDevice(s->device));
  p->device = s->device;
  const int64_t rows = s->rows;
  const int32_t n_tiles = (int32_t)((rows + 63) / 64);
  try {
    p->h_words.assign((size_t)n_tiles, 0);
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for %d mask words", n_tiles);
  }
  rc = p->words.reserve(n_tiles + (n_tiles > 0 ? n_set : 0), 64, &p->bytes);
  if (rc) return rc;
  if (n_tiles > 0) {
    hipStream_t st = s->aux_stream;
    int64_t *d_set = reinterpret_cast<int64_t *>(p->words.d + n_tiles);
    if (n_set > 0) HIPCHK(hipMemcpyAsync(d_set, set, (size_t)n_set * 8, hipMemcpyHostToDevice, st));
    launch(st, rows, n_tiles, d_set, wp ? wp->words.d : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p->h_words.data(), p->words.d, (size_t)n_tiles * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return mask_finish_part(p, s, rows, n_tiles);
}

// tsh_mask_create_range, _where and _tags behind their argument checks and their plan: the with check, the new handle,
// every shard's part by words(g, s, part) -- which fetches the columns' parts and ends in mask_device_part -- the handle's
// GLOBAL bitmap, registration.  cols: the column handles the words are made from.  They stay as they are until every part
// is made: their use_mu are held shared, taken in one order, by address -- two calls that name the same handles in
// opposite orders cannot hold one each while a _set waits between them -- and all given up before g_mask_mu is taken to
// register: a _set holds that one while it waits for these
template <class C, class F>
int32_t make_device_mask(tsh_index *idx, tsh_mask *with, tsh_mask **out, C *const *cols, int n_cols, F &&words) {
  if (with && with->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index (or its index was destroyed)");
  std::unique_ptr<tsh_mask> m(new tsh_mask());
  m->idx = idx;
  int rc = TSH_OK;
  {
    C *order[WHERE_MAX_COLUMNS];
    std::copy(cols, cols + n_cols, order);
    std::sort(order, order + n_cols, std::less<C *>());
    std::vector<std::shared_lock<std::shared_mutex>> use;
    use.reserve((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) use.emplace_back(order[c]->use_mu);
    rc = make_parts(m.get(), [&](size_t g, Shard *s, MaskPart *p) {
      int prc = words(g, s, p);
      if (prc) return prc;
      // the handle's GLOBAL bitmap, as a bitmap-made handle holds it: what a rebuild after an append slices (the rows it
      // keeps then are the rows it keeps now) and what tsh_mask_read copies
      try {
        const size_t need = (size_t)((s->row_base + s->rows + 7) / 8) + 1;
        if (m->bits.size() < need) m->bits.resize(need, 0);
      } catch (...) {
        return set_err(TSH_E_OOM, "no memory for the mask's bitmap");
      }
      if (s->rows > 0) unslice_mask(s->row_base, s->rows, p->h_words.data(), m->bits.data());
      return (int)TSH_OK;
    });
  }
  if (rc) return rc;
  return register_handle(m, out);
}

// tsh_groups::spans: one pass over the array against the shards' row ranges.  A multi-device index cuts its rows at
// multiples of rows_per_shard whatever the shards hold yet, so the answer changes with the array only, never with an
// append (a group that will span once rows named in the array arrive counts as spanning already: exact, only slower)
void groups_update_spans(tsh_groups *g) {
  g->spans = false;
  const tsh_index *idx = g->idx;
  if (!idx || idx->shards.size() < 2 || idx->rows_per_shard <= 0) return;
  const int64_t last = (int64_t)idx->shards.size() - 1;
  std::vector<int32_t> first((size_t)g->n_groups, -1);
  for (size_t i = 0; i < g->group_of.size(); ++i) {
    const int32_t gi = g->group_of[i];
    if (gi < 0 || gi >= g->n_groups) continue;
    const int32_t sh = (int32_t)std::min<int64_t>((int64_t)i / idx->rows_per_shard, last);
    if (first[(size_t)gi] < 0) first[(size_t)gi] = sh;
    else if (first[(size_t)gi] != sh) {
      g->spans = true;
      return;
    }
  }
}

// group ids of a caller's array: negative (ungrouped) or below n_groups
int check_group_ids(const int32_t *group_of, int64_t n, int32_t n_groups) {
  for (int64_t i = 0; i < n; ++i)
    if (group_of[i] >= n_groups) return set_err(TSH_E_BAD_ARG, "group_of[%lld] = %d is not below n_groups %d", (long long)i, group_of[i], n_groups);
  return TSH_OK;
}

// What the shard-level entries are asked (tsh_search_shard*, tsh_search_shard_begin*, the sharded search's windows, groups
// and retries): nq queries, the call's mask, a cursor per query or none, nq blocks of `entries` entries on the device.  A
// further per-query input is added here and in Cursors
struct ShardSearchReq {
  const float *queries = nullptr;
  int32_t nq = 0, k = 0, entries = 0;
  CallMask mask;
  Cursors after;
  uint8_t *d_blocks = nullptr;
  // a grouped call (tsh_search_shard_grouped and its kin): the groups handle made on this shard handle, or none.  Never
  // with cursors; k <= 0 is answered with empty blocks
  tsh_groups *groups = nullptr;
  // ... whose use_mu the caller holds shared for as long as the search runs (tsh_search_sharded_grouped: one lock for the
  // call's scans, retries and merges) -- it is not taken again here
  bool groups_held = false;
};
// What every grouped shard-level entry checks before it runs (tsh_search_grouped's argument errors)
inline int check_shard_groups(tsh_index *idx, const CallMask &m, const tsh_groups *groups) {
  if (m.bytes && m.handle) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!groups) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (groups->idx != idx) return set_err(TSH_E_BAD_ARG, "the groups handle was made for another index (or its index was destroyed)");
  return TSH_OK;
}
// ... and how a progressive one (shard_stream_begin) is to run
struct ShardStreamOpts {
  int32_t step = 0;            // matrix-core route: queries per batched call (0: all in one)
  bool copy_inputs = false;    // public entry points: the caller's arrays are consumed before begin returns
  uint32_t tag = 0;            // generation the blocks carry (BlockHeader.pad[1])
  OneWorker *exec = nullptr;   // the caller's persistent thread in place of the search's own (tsh_search_sharded: starting a
                               // thread costs a 20-query call on a 125 k-row shard 30-40 us before its first scan is enqueued)
  bool leave_overflow = false;  // the caller enqueues its exchange ahead of the blocks (Job::leave_overflow)
};

// fn(g) -> status, for every shard of the handle side by side: one shard inline, else the handle's workers.  -> the first
// failing shard's status, with that shard's error text in g_err
template <typename F>
int for_each_shard(tsh_index *idx, F fn) {
  const size_t ns = idx->shards.size();
  if (ns == 1) return fn((size_t)0);
  std::vector<int> rcs(ns, TSH_OK);
  std::vector<std::string> errs(ns);
  auto run = [&](size_t g) {
    rcs[g] = fn(g);
    if (rcs[g]) errs[g] = g_err;
  };
  const std::function<void(size_t)> frun = run;
  if (!idx->workers || !idx->workers->run(frun)) {  // the workers are busy with a concurrent call: own threads
    std::vector<std::thread> th;
    for (size_t g = 1; g < ns; ++g) th.emplace_back(run, g);
    run(0);
    for (auto &t : th) t.join();
  }
  for (size_t g = 0; g < ns; ++g)
    if (rcs[g]) {
      g_err = errs[g];
      return rcs[g];
    }
  return TSH_OK;
}

// nq empty blocks (an empty shard's contribution to a shard-level search), written to the device
int write_empty_blocks(Shard *s, int32_t nq, int32_t k, int32_t entries, uint32_t tag, uint8_t *d_blocks) {
  HIPCHK(hipSetDevice(s->device));
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  std::vector<uint8_t> z(bb * (size_t)nq, 0);
  for (int32_t q = 0; q < nq; ++q) {
    BlockHeader *h = reinterpret_cast<BlockHeader *>(z.data() + (size_t)q * bb);
    h->entries = (uint32_t)entries;
    h->k = (uint32_t)k;
    h->metric = (uint32_t)s->metric;
    h->row_base = s->row_base;
    h->pad[1] = tag;
  }
  HIPCHK(hipMemcpy(d_blocks, z.data(), z.size(), hipMemcpyHostToDevice));
  return TSH_OK;
}

// ---- facet counts (tsh_attr_facets, tsh_tags_facets; tsh_facet.hip.h, tsh_facet_plan.h) -------------------------------------
// What the two entries refuse on their arguments alone, in the header's order; no handle is dereferenced
int facet_check_args(tsh_index *idx, const void *col, const char *col_name, int32_t kind, const int64_t *keys, int64_t n_keys,
                     const int64_t *out_counts, const int64_t *out_rest, FacetKeys *k) {
  if (!out_rest) return set_err(TSH_E_BAD_ARG, "out_rest is NULL");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (!col) return set_err(TSH_E_BAD_ARG, "%s is NULL", col_name);
  try {
    if (const int e = facet_keys(kind, keys, n_keys, k)) return set_err(TSH_E_BAD_ARG, "%s", facet_plan_error(e));
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for the keys");
  }
  if (n_keys > 0 && !out_counts) return set_err(TSH_E_BAD_ARG, "out_counts is NULL with n_keys > 0");
  return TSH_OK;
}

// The call behind the argument checks, for either column kind H.  col->use_mu is held shared for the whole call (a _set
// waits for it, as for a mask maker); per shard, side by side: the shard's shared lock, the column's and the mask's part
// made current for the shard's rows, then -- under the shard's facet_mu -- the keys go up behind zeroed counters in the
// shard's scratch, launch(st, s, column part, mask words or nullptr, n_words, d_set, d_cnt) enqueues the one kernel on
// aux_stream and the |S| + 3 counters come back in one copy.  The device live bitmap has the quarantined rows' bits
// clear -- in safe mode too: the rows past QUARANTINE_MAX keep their bits and are counted on the device -- so the host adds
// the listed ones: quar(s, the mask's words on the host or nullptr, counters).  Then the sum over shards and the scatter
template <class H, class L, class Q>
int32_t facet_call(tsh_index *idx, H *col, tsh_mask *mask, const FacetKeys &k, int64_t *out_counts, int64_t *out_rest, L &&launch,
                   Q &&quar) {
  const size_t ns = idx->shards.size(), n_cnt = k.counters();
  const int32_t n_set = k.n();
  std::vector<std::vector<uint64_t>> cnt(ns);
  std::shared_lock<std::shared_mutex> use(col->use_mu);
  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    try {
      cnt[g].assign(n_cnt, 0);
    } catch (...) {
      return set_err(TSH_E_OOM, "no memory for %zu counters", n_cnt);
    }
    int prc = TSH_OK;
    const PartOf<H> *cp = current_part(col, g, s, &prc);
    if (!cp) return prc;
    const MaskPart *mp = mask ? current_part(mask, g, s, &prc) : nullptr;
    if (mask && !mp) return prc;
    HIPCHK(hipSetDevice(s->device));
    const int32_t n_words = (int32_t)((s->rows + 63) / 64);
    {
      std::lock_guard<std::mutex> lk(s->facet_mu);
      const int64_t need = (int64_t)n_cnt + n_set;
      if (s->facet_cap < need) {
        hipFree(s->d_facet);
        s->d_facet = nullptr;
        s->facet_cap = 0;
        const int64_t grown = round_up(need + need / 8, 1024);
        HIPCHK(hipMalloc(&s->d_facet, (size_t)grown * 8));
        s->facet_cap = grown;
      }
      hipStream_t st = s->aux_stream;
      unsigned long long *d_cnt = reinterpret_cast<unsigned long long *>(s->d_facet);
      int64_t *d_set = s->d_facet + n_cnt;
      HIPCHK(hipMemsetAsync(d_cnt, 0, n_cnt * 8, st));
      if (n_set > 0) HIPCHK(hipMemcpyAsync(d_set, k.set.data(), (size_t)n_set * 8, hipMemcpyHostToDevice, st));
      launch(st, s, cp, mp ? mp->words.d : nullptr, n_words, d_set, d_cnt);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(cnt[g].data(), d_cnt, n_cnt * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (!s->quar_ids.empty()) quar(s, mp ? mp->h_words.data() : nullptr, cnt[g].data());
    return TSH_OK;
  });
  if (rc) return rc;
  std::vector<uint64_t> all(n_cnt, 0);
  for (size_t g = 0; g < ns; ++g)
    if (!cnt[g].empty()) facet_add(all.data(), cnt[g].data(), n_cnt);
  facet_scatter(k, all.data(), out_counts, out_rest);
  return TSH_OK;
}

}  // namespace

extern "C" {

int32_t tsh_abi_version(void) { return TSH_ABI_VERSION; }

int32_t tsh_device_count(void) { return device_count_cached(); }

int32_t tsh_last_error(char *buf, int32_t len) {
  if (buf && len > 0) {
    size_t n = std::min<size_t>(g_err.size(), (size_t)len - 1);
    memcpy(buf, g_err.data(), n);
    buf[n] = 0;
  }
  return (int32_t)g_err.size();
}

int32_t tsh_index_create(int32_t dim, int32_t metric, int64_t capacity_rows, int32_t n_devices,
                         tsh_index **out) {
  int rc = check_create_args(dim, metric, capacity_rows, out);
  if (rc) return rc;
  // TSH_SHARDS_SHARE_DEVICES=1 (testing hook, obeyed only after TSH_OPT_TEST_HOOKS): shards of a multi-device
  // handle may share a physical device (shard g on device g % count), so the multi-shard code path -- append
  // routing, one host thread per shard, host merge -- can be exercised on a one-GPU box
  const char *share_env = test_env("TSH_SHARDS_SHARE_DEVICES");
  const bool share = share_env && share_env[0] == '1';
  if (n_devices < 1 || (!share && n_devices > device_count_cached()) || n_devices > 64)
    return set_err(TSH_E_BAD_ARG, "n_devices %d outside [1,%d]", n_devices, device_count_cached());
  std::unique_ptr<tsh_index> idx(new tsh_index());
  idx->dim = dim;
  idx->metric = metric;
  if (n_devices == 1) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    std::unique_ptr<Shard> s;
    rc = make_shard(dim, metric, dev, 0, capacity_rows, &s);
    if (rc) return rc;
    idx->shards.push_back(std::move(s));
  } else {
    if (capacity_rows <= 0)
      return set_err(TSH_E_BAD_ARG, "multi-device index needs capacity_rows to place the row ranges");
    idx->rows_per_shard = round_up((capacity_rows + n_devices - 1) / n_devices, 64);
    for (int g = 0; g < n_devices; ++g) {
      std::unique_ptr<Shard> s;
      rc = make_shard(dim, metric, g % device_count_cached(), (int64_t)g * idx->rows_per_shard,
                      idx->rows_per_shard, &s);
      if (rc) {
        for (auto &p : idx->shards) shard_destroy(p.get());
        return rc;
      }
      idx->shards.push_back(std::move(s));
    }
    idx->workers.reset(new ShardWorkers(n_devices));
  }
  *out = idx.release();
  return TSH_OK;
}

int32_t tsh_index_create_shard(int32_t dim, int32_t metric, int64_t capacity_rows, int32_t device_id,
                               int64_t row_base, tsh_index **out) {
  int rc = check_create_args(dim, metric, capacity_rows, out);
  if (rc) return rc;
  if (row_base < 0) return set_err(TSH_E_BAD_ARG, "row_base < 0");
  int dev = device_id;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= device_count_cached()) return set_err(TSH_E_BAD_ARG, "device %d not present", dev);
  std::unique_ptr<tsh_index> idx(new tsh_index());
  idx->dim = dim;
  idx->metric = metric;
  std::unique_ptr<Shard> s;
  rc = make_shard(dim, metric, dev, row_base, capacity_rows, &s);
  if (rc) return rc;
  idx->shards.push_back(std::move(s));
  *out = idx.release();
  return TSH_OK;
}

int32_t tsh_index_destroy(tsh_index *idx) {
  if (!idx) return TSH_OK;
  {
    std::lock_guard<std::mutex> lk(g_mask_mu);
    orphan_handles(idx->masks);
    orphan_handles(idx->groups);
    orphan_handles(idx->attrs);
    orphan_handles(idx->tags);
  }
  idx->workers.reset();  // joins the shard threads
  for (auto &s : idx->shards) {
    std::unique_lock<RwLock> xl(s->mu);
    shard_destroy(s.get());
  }
  delete idx;
  return TSH_OK;
}

int32_t tsh_index_append(tsh_index *idx, int64_t first_row_id, int64_t n_rows, const float *rows) {
  return index_append(idx, first_row_id, n_rows, rows, false);
}

int32_t tsh_index_append_device(tsh_index *idx, int64_t first_row_id, int64_t n_rows, const void *d_rows) {
  return index_append(idx, first_row_id, n_rows, static_cast<const float *>(d_rows), true);
}

int32_t tsh_index_set_deleted(tsh_index *idx, const int64_t *ids, int64_t n) {
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (n < 0) return set_err(TSH_E_BAD_ARG, "n < 0");
  if (n == 0) return TSH_OK;
  if (!ids) return set_err(TSH_E_BAD_ARG, "ids is NULL");
  for (auto &sp : idx->shards) {
    Shard *s = sp.get();
    std::unique_lock<RwLock> xl(s->mu);
    if (s->rows == 0) continue;
    HIPCHK(hipSetDevice(s->device));
    if (n > s->del_ids_cap) {  // kept between calls (deletes arrive in small batches, journal flush by journal flush)
      hipFree(s->d_del_ids);
      s->d_del_ids = nullptr;
      s->del_ids_cap = 0;
      const int64_t want = std::max<int64_t>(round_up(n, 1024), 4096);
      HIPCHK(hipMalloc(&s->d_del_ids, (size_t)want * sizeof(int64_t)));
      s->del_ids_cap = want;
    }
    int64_t *d_ids = s->d_del_ids;
    hipStream_t st = s->ingest_stream;
    hipError_t e = hipMemcpyAsync(d_ids, ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->d_tmp_u32, 0, 4, st);
    if (e == hipSuccess) {
      int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
      live_clear_ids_kernel<<<grid, 256, 0, st>>>(s->d_live, d_ids, n, s->row_base, s->rows, s->d_tmp_u32);
    }
    uint32_t cleared = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&cleared, s->d_tmp_u32, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_err(TSH_E_HIP, "set_deleted: %s", hipGetErrorString(e));
    s->deleted += cleared;
    if (cleared) s->all_live = false;
    if (!s->quar_ids.empty()) {  // a quarantined row's live bit is clear already: take it off the list
      size_t before = s->quar_ids.size();
      for (int64_t i = 0; i < n; ++i) {
        const int64_t r = ids[i] - s->row_base;
        if (r < 0 || r >= s->rows) continue;
        auto it = std::lower_bound(s->quar_ids.begin(), s->quar_ids.end(), (uint32_t)r);
        if (it != s->quar_ids.end() && *it == (uint32_t)r) s->quar_ids.erase(it);
      }
      if (s->quar_ids.size() != before) {
        s->deleted += (int64_t)(before - s->quar_ids.size());
        int rc = quarantine_upload(s);
        if (rc) return rc;
      }
    }
  }
  return TSH_OK;
}

int64_t tsh_index_size(tsh_index *idx) {
  if (!idx) return 0;
  int64_t m = 0;
  for (auto &s : idx->shards) {
    std::shared_lock<RwLock> sl = share(idx, s.get());
    if (s->rows > 0) m = std::max(m, s->row_base + s->rows);
  }
  return m;
}
int32_t tsh_index_dim(tsh_index *idx) { return idx ? idx->dim : 0; }
int32_t tsh_index_metric(tsh_index *idx) { return idx ? idx->metric : 0; }

int64_t tsh_candidate_block_bytes(int32_t entries) {
  return (int64_t)sizeof(BlockHeader) + (int64_t)std::max(entries, 0) * (int64_t)sizeof(BlockEntry);
}
int32_t tsh_default_block_entries(int32_t k) {
  return select_default_entries(k);
}

// after: a cursor per query (tsh_search_after), or none
static int32_t search_impl(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, const CallMask &mask,
                           int64_t *out_ids, double *out_dist, int32_t *out_count, Cursors after = Cursors()) {
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (mask.handle && mask.handle->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  if (k <= 0) return TSH_OK;  // reference: topK <= 0 yields an empty list
  if (!out_ids || !out_dist) return set_err(TSH_E_BAD_ARG, "out_ids / out_dist is NULL");

  const double t_in = now_us();
  size_t ns = idx->shards.size();
  int32_t entries = tsh_default_block_entries(k);
  size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  std::vector<std::unique_ptr<uint8_t[]>> blocks(ns);  // uninitialised: every block is written whole
  std::vector<size_t> block_caps(ns, 0);
  struct GiveBack {
    tsh_index *idx;
    std::vector<std::unique_ptr<uint8_t[]>> *b;
    std::vector<size_t> *c;
    ~GiveBack() {
      for (size_t g = 0; g < b->size(); ++g)
        if ((*b)[g]) idx->give_blocks(std::move((*b)[g]), (*c)[g]);
    }
  } give_back{idx, &blocks, &block_caps};
  std::vector<std::vector<std::vector<BlockEntry>>> spills(ns), extras(ns);
  std::vector<char> active(ns, 0);
  std::vector<char> finalized((size_t)nq, 0);  // done early by the batched path's chunk callback

  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    active[g] = 1;
    blocks[g] = idx->take_blocks(bb * (size_t)nq, &block_caps[g]);
    spills[g].resize((size_t)nq);
    extras[g].resize((size_t)nq);
    SearchOut so;
    so.h_blocks = blocks[g].get();
    so.spill = &spills[g];
    so.extra = &extras[g];
    so.after = after;
    if (ns == 1 && !after)  // batched path: finalise a chunk of queries while the GPU still works on the next one
      so.on_chunk = [&](int32_t q0, int32_t q1, const char *skip, const uint8_t *base, const double *mag_a) {
        parallel_for_range(q0, q1, [&](int32_t q) {
          if (skip[q]) return;
          EntryList two[2];
          const size_t n_lists = shard_lists(base + (size_t)q * bb, nullptr, &extras[0][(size_t)q], two);
          out_count[q] = finalize_query(idx->metric, idx->dim, queries + (size_t)q * idx->dim, k, thr, two,
                                        n_lists, out_ids + (size_t)q * k, out_dist + (size_t)q * k, mag_a + q);
          finalized[(size_t)q] = 1;
        });
      };
    if (ns == 1 && !after) {
      so.fin_thr = thr;
      so.on_final = [&](int32_t q0, int32_t q1, const char *skip, const int64_t *ids, const double *dist, const int32_t *cnt) {
        parallel_for_range(q0, q1, [&](int32_t q) {
          if (skip[q]) return;
          memcpy(out_ids + (size_t)q * k, ids + (size_t)q * k, (size_t)k * sizeof(int64_t));
          memcpy(out_dist + (size_t)q * k, dist + (size_t)q * k, (size_t)k * sizeof(double));
          out_count[q] = cnt[q];
          finalized[(size_t)q] = 1;
        });
      };
    }
    if (ns == 1)  // single-query pipeline, one submitting thread: query q is ordered and cut while the GPU scans q + 1 ...
      so.on_block = [&](int32_t q, const uint8_t *block, const std::vector<BlockEntry> *sp, const std::vector<BlockEntry> *ex) {
        EntryList two[2];
        const size_t n_lists = shard_lists(block, sp, ex, two);
        Cursor cur;
        out_count[q] = finalize_query(idx->metric, idx->dim, queries + (size_t)q * idx->dim, k, thr, two, n_lists,
                                      out_ids + (size_t)q * k, out_dist + (size_t)q * k, nullptr, after.at(q, &cur));
        finalized[(size_t)q] = 1;
      };
    MaskSrc ms;
    int mrc = call_mask_for_shard(mask, g, s, &ms);
    if (mrc) return mrc;
    // (cursor searches: the pipeline of single-query scans, never the batched path)
    return after ? shard_search_blocks(s, queries, nq, k, ms, entries, &so, PIPE_DEPTH)
                 : shard_search_any(s, s->batch, idx->batch_min_nq.load(), queries, nq, k, ms, entries, &so);
  });
  if (rc) return rc;
  const double t_shards = now_us();
  // (the batched path's chunk callback has usually done everything: waking the pool for nothing cost 30-50 us)
  const bool all_done = std::find(finalized.begin(), finalized.end(), (char)0) == finalized.end();
  if (!all_done) parallel_for(nq, [&](int32_t q) {
    if (finalized[(size_t)q]) return;
    std::vector<EntryList> lists;
    for (size_t g = 0; g < ns; ++g) {
      if (!active[g]) continue;
      EntryList two[2];
      const size_t n_lists = shard_lists(blocks[g].get() + (size_t)q * bb, &spills[g][(size_t)q], &extras[g][(size_t)q], two);
      lists.insert(lists.end(), two, two + n_lists);
    }
    Cursor cur;
    out_count[q] = finalize_query(idx->metric, idx->dim, queries + (size_t)q * idx->dim, k, thr, lists,
                                  out_ids + (size_t)q * k, out_dist + (size_t)q * k, after.at(q, &cur));
  });
  if (trace_batch() && nq >= 64)
    fprintf(stderr, "[tsh search] nq=%d shards %.0f us, finalize %.0f us\n", nq, t_shards - t_in, now_us() - t_shards);
  return TSH_OK;
}

int32_t tsh_search(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr,
                   const uint8_t *row_mask, int64_t *out_ids, double *out_dist, int32_t *out_count) {
  return search_impl(idx, queries, nq, k, thr, CallMask{row_mask, nullptr}, out_ids, out_dist, out_count);
}

int32_t tsh_search_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, tsh_mask *mask,
                          int64_t *out_ids, double *out_dist, int32_t *out_count) {
  return search_impl(idx, queries, nq, k, thr, CallMask{nullptr, mask}, out_ids, out_dist, out_count);
}

int32_t tsh_search_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, const uint8_t *row_mask,
                         tsh_mask *mask, const double *after_dist, const int64_t *after_id, int64_t *out_ids,
                         double *out_dist, int32_t *out_count) {
  if (row_mask && mask) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!after_dist || !after_id) return set_err(TSH_E_BAD_ARG, "after_dist / after_id is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return search_impl(idx, queries, nq, k, thr, CallMask{row_mask, mask}, out_ids, out_dist, out_count, Cursors{after_dist, after_id});
}

int32_t tsh_search_after_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = 0;
  for (auto &sp : idx->shards) {
    out[0] += sp->c_after.load();
    out[1] += sp->c_after_side.load();
    out[2] += sp->c_after_redone.load();
    out[3] += sp->c_after_nofloor.load();
  }
  return TSH_OK;
}

// ---- count: how many rows tsh_search_after's list holds ----------------------------------------------------------------
int32_t tsh_search_count(tsh_index *idx, const float *queries, int32_t nq, double thr, const uint8_t *row_mask, tsh_mask *mask_h,
                         const double *after_dist, const int64_t *after_id, int64_t *out_count) {
  if (row_mask && mask_h) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (half_cursor(after_dist, after_id)) return set_err(TSH_E_BAD_ARG, "after_dist / after_id: both or neither");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  const size_t ns = idx->shards.size();
  // (the block of a count job: used in safe mode only, where the job is a search for one row whose wide-band pass
  // spills every live row)
  const int32_t k = 1, entries = tsh_default_block_entries(k);
  std::vector<std::vector<int64_t>> counts(ns);
  std::vector<std::vector<std::vector<BlockEntry>>> spills(ns), extras(ns);
  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    counts[g].assign((size_t)nq, 0);
    spills[g].resize((size_t)nq);
    extras[g].resize((size_t)nq);
    SearchOut so;
    so.spill = &spills[g];
    so.extra = &extras[g];
    so.after = Cursors{after_dist, after_id};
    so.count_out = counts[g].data();
    so.count_thr = thr;
    MaskSrc ms;
    int mrc = call_mask_for_shard(CallMask{row_mask, mask_h}, g, s, &ms);
    if (mrc) return mrc;
    // (the pipeline of single-query scans, never the batched path)
    return shard_search_blocks(s, queries, nq, k, ms, entries, &so, PIPE_DEPTH);
  });
  if (rc) return rc;
  for (size_t g = 0; g < ns; ++g)
    for (size_t q = 0; q < counts[g].size(); ++q) out_count[q] += counts[g][q];
  return TSH_OK;
}

int32_t tsh_search_count_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = 0;
  for (auto &sp : idx->shards) {
    out[0] += sp->c_count.load();
    out[1] += sp->c_count_side.load();
    out[2] += sp->c_count_redone.load();
    out[3] += sp->c_count_nowindow.load();
  }
  return TSH_OK;
}

// ---- grouped search: the nearest row of each of the k nearest groups (tsh_group_rule.h) --------------------------------
// (the handle travels as void *, and create's out as the address of one: see the header)
int32_t tsh_groups_create(tsh_index *idx, const int32_t *group_of, int64_t n, int32_t n_groups, void *out_p) {
  tsh_groups **out = static_cast<tsh_groups **>(out_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (n_groups < 0 || n_groups > GROUP_MAX_GROUPS) return set_err(TSH_E_BAD_ARG, "n_groups %d outside [0, %d]", n_groups, GROUP_MAX_GROUPS);
  if (n < 0 || (n > 0 && !group_of)) return set_err(TSH_E_BAD_ARG, "group_of is NULL / n < 0");
  int rc = check_group_ids(group_of, n, n_groups);
  if (rc) return rc;
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  std::unique_ptr<tsh_groups> g(new tsh_groups());
  g->idx = idx;
  g->n_groups = n_groups;
  try {
    g->group_of.assign(group_of, group_of + n);
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for %lld group ids", (long long)n);
  }
  try {
    groups_update_spans(g.get());
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for %d groups' shards", n_groups);
  }
  rc = make_parts(g.get());
  if (rc) return rc;
  return register_handle(g, out);
}

int32_t tsh_groups_set(void *groups, int64_t first_row_id, int64_t n, const int32_t *group_of) {
  tsh_groups *g = static_cast<tsh_groups *>(groups);
  if (!g) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (first_row_id < 0 || n < 0 || (n > 0 && !group_of)) return set_err(TSH_E_BAD_ARG, "group_of is NULL / negative row range");
  return set_column(
      g, "the groups handle's index was destroyed", n, [&] { return check_group_ids(group_of, n, g->n_groups); },
      [&] {
        try {
          if ((int64_t)g->group_of.size() < first_row_id + n) g->group_of.resize((size_t)(first_row_id + n), -1);
        } catch (...) {
          return set_err(TSH_E_OOM, "no memory for %lld group ids", (long long)(first_row_id + n));
        }
        memcpy(g->group_of.data() + first_row_id, group_of, (size_t)n * sizeof(int32_t));
        try {
          groups_update_spans(g);
        } catch (...) {
          g->spans = true;  // (no memory for the pass: the exact-all route is always right)
        }
        return (int)TSH_OK;
      });
}

int32_t tsh_groups_destroy(void *groups_p) { return destroy_handle(static_cast<tsh_groups *>(groups_p)); }

int32_t tsh_search_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, const uint8_t *row_mask,
                           tsh_mask *mask_h, void *groups_p, int64_t *out_ids, double *out_dist, int32_t *out_group,
                           int32_t *out_count) {
  tsh_groups *groups = static_cast<tsh_groups *>(groups_p);
  if (row_mask && mask_h) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!groups) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (groups->idx != idx) return set_err(TSH_E_BAD_ARG, "the groups handle was made for another index (or its index was destroyed)");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  if (k <= 0) return TSH_OK;
  if (!out_ids || !out_dist) return set_err(TSH_E_BAD_ARG, "out_ids / out_dist is NULL");
  std::shared_lock<std::shared_mutex> use(groups->use_mu);  // the array stays as it is until the finaliser has read it
  const size_t ns = idx->shards.size();
  const int32_t entries = tsh_default_block_entries(k);
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  std::vector<std::unique_ptr<uint8_t[]>> blocks(ns);
  std::vector<std::vector<std::vector<BlockEntry>>> spills(ns), extras(ns);
  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    blocks[g].reset(new uint8_t[bb * (size_t)nq]);
    spills[g].resize((size_t)nq);
    extras[g].resize((size_t)nq);
    SearchOut so;
    so.h_blocks = blocks[g].get();
    so.spill = &spills[g];
    so.extra = &extras[g];
    int prc = TSH_OK;
    so.groups = current_part(groups, g, s, &prc);
    if (!so.groups) return prc;
    MaskSrc ms;
    int mrc = call_mask_for_shard(CallMask{row_mask, mask_h}, g, s, &ms);
    if (mrc) return mrc;
    // (the pipeline of single-query scans, never the batched path)
    return shard_search_blocks(s, queries, nq, k, ms, entries, &so, PIPE_DEPTH);
  });
  if (rc) return rc;
  // groups span shards: the finaliser's step runs once per query over every shard's entries
  const GroupTable table{groups->group_of.data(), (int64_t)groups->group_of.size()};
  parallel_for(nq, [&](int32_t q) {
    std::vector<EntryList> lists;
    for (size_t g = 0; g < ns; ++g) {
      if (!blocks[g]) continue;
      EntryList two[2];
      const size_t n_lists = shard_lists(blocks[g].get() + (size_t)q * bb, &spills[g][(size_t)q], &extras[g][(size_t)q], two);
      lists.insert(lists.end(), two, two + n_lists);
    }
    out_count[q] = finalize_grouped(idx->metric, idx->dim, queries + (size_t)q * idx->dim, k, thr, lists.data(), lists.size(), table,
                                    out_ids + (size_t)q * k, out_dist + (size_t)q * k, out_group ? out_group + (size_t)q * k : nullptr);
  });
  return TSH_OK;
}

int32_t tsh_search_grouped_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = 0;
  for (auto &sp : idx->shards) {
    out[0] += sp->c_grouped.load();
    out[1] += sp->c_grouped_side.load();
    out[2] += sp->c_grouped_redone.load();
    out[3] += sp->c_grouped_nodev.load();
  }
  return TSH_OK;
}

// ---- grouped cursor search and group count (tsh_group_after_rule.h) ------------------------------------------------------
namespace {

// Does this call take the exact-all route?  Groups with rows on several shards (the handle's flag), or a shard holding a
// live quarantined row (deleted ones are off the list: set_deleted), looked at under each shard's lock.  The shards' jobs
// look again under the lock they run under, so an append in between cannot slip a quarantined row past its own shard --
// and where groups stay inside a shard, its own shard is the only one such a row matters to
bool grouped_after_exact_all(tsh_index *idx, const tsh_groups *groups) {
  if (groups->spans) return true;
  for (auto &sp : idx->shards) {
    std::shared_lock<RwLock> sl = share(idx, sp.get());
    if (!sp->quar_ids.empty()) return true;
  }
  return false;
}

// The two entries' common body: count == false, a page of k groups per query past `after` (never empty); count == true,
// the number of groups per query past `after` (or all of them) into out_n.  One finaliser step per query over all shards
int grouped_after_impl(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, const uint8_t *row_mask, tsh_mask *mask_h,
                       tsh_groups *groups, Cursors after, bool count, int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_count,
                       int64_t *out_n) {
  std::shared_lock<std::shared_mutex> use(groups->use_mu);  // the array stays as it is until the finaliser has read it
  const size_t ns = idx->shards.size();
  const int32_t entries = tsh_default_block_entries(k);
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  const bool exact_all = grouped_after_exact_all(idx, groups);
  std::vector<std::unique_ptr<uint8_t[]>> blocks(ns);
  std::vector<std::vector<int64_t>> certain(ns);
  std::vector<std::vector<std::vector<BlockEntry>>> spills(ns), extras(ns);
  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    blocks[g].reset(new uint8_t[bb * (size_t)nq]);
    spills[g].resize((size_t)nq);
    extras[g].resize((size_t)nq);
    SearchOut so;
    so.h_blocks = blocks[g].get();
    so.spill = &spills[g];
    so.extra = &extras[g];
    so.after = after;
    so.group_after = true;
    so.exact_all = exact_all || !s->quar_ids.empty();
    if (count) {
      certain[g].assign((size_t)nq, 0);
      so.count_out = certain[g].data();
      so.count_thr = thr;
    }
    int prc = TSH_OK;
    so.groups = current_part(groups, g, s, &prc);
    if (!so.groups) return prc;
    MaskSrc ms;
    int mrc = call_mask_for_shard(CallMask{row_mask, mask_h}, g, s, &ms);
    if (mrc) return mrc;
    // (the pipeline of single-query scans, never the batched path)
    return shard_search_blocks(s, queries, nq, k, ms, entries, &so, PIPE_DEPTH);
  });
  if (rc) return rc;
  const GroupTable table{groups->group_of.data(), (int64_t)groups->group_of.size()};
  parallel_for(nq, [&](int32_t q) {
    std::vector<EntryList> lists;
    int64_t sure = 0;
    for (size_t g = 0; g < ns; ++g) {
      if (!blocks[g]) continue;
      EntryList two[2];
      const size_t n_lists = shard_lists(blocks[g].get() + (size_t)q * bb, &spills[g][(size_t)q], &extras[g][(size_t)q], two);
      lists.insert(lists.end(), two, two + n_lists);
      if (count) sure += certain[g][(size_t)q];
    }
    Cursor cur;
    const Cursor *c = after.at(q, &cur);
    const float *query = queries + (size_t)q * idx->dim;
    if (count)
      out_n[q] = sure + group_count_entries(idx->metric, idx->dim, query, thr, lists.data(), lists.size(), table, c);
    else
      out_count[q] = finalize_grouped_after(idx->metric, idx->dim, query, k, thr, lists.data(), lists.size(), table, *c, out_ids + (size_t)q * k,
                                            out_dist + (size_t)q * k, out_group ? out_group + (size_t)q * k : nullptr);
  });
  return TSH_OK;
}

}  // namespace

int32_t tsh_search_grouped_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double thr, const uint8_t *row_mask,
                                 tsh_mask *mask_h, void *groups_p, const double *after_dist, const int64_t *after_id, int64_t *out_ids,
                                 double *out_dist, int32_t *out_group, int32_t *out_count) {
  tsh_groups *groups = static_cast<tsh_groups *>(groups_p);
  if (row_mask && mask_h) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!groups) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (!after_dist || !after_id) return set_err(TSH_E_BAD_ARG, "after_dist / after_id is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (groups->idx != idx) return set_err(TSH_E_BAD_ARG, "the groups handle was made for another index (or its index was destroyed)");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  if (k <= 0) return TSH_OK;
  if (!out_ids || !out_dist) return set_err(TSH_E_BAD_ARG, "out_ids / out_dist is NULL");
  return grouped_after_impl(idx, queries, nq, k, thr, row_mask, mask_h, groups, Cursors{after_dist, after_id}, false, out_ids, out_dist, out_group,
                            out_count, nullptr);
}

int32_t tsh_search_grouped_count(tsh_index *idx, const float *queries, int32_t nq, double thr, const uint8_t *row_mask, tsh_mask *mask_h,
                                 void *groups_p, const double *after_dist, const int64_t *after_id, int64_t *out_count) {
  tsh_groups *groups = static_cast<tsh_groups *>(groups_p);
  if (row_mask && mask_h) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!groups) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (half_cursor(after_dist, after_id)) return set_err(TSH_E_BAD_ARG, "after_dist / after_id: both or neither");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (groups->idx != idx) return set_err(TSH_E_BAD_ARG, "the groups handle was made for another index (or its index was destroyed)");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  // (the block of a count job: used on the exact-all route only, where the job is a search for one row whose wide-band
  // pass spills every live row)
  return grouped_after_impl(idx, queries, nq, /*k*/ 1, thr, row_mask, mask_h, groups, Cursors{after_dist, after_id}, true, nullptr, nullptr, nullptr,
                            nullptr, out_count);
}

int32_t tsh_search_grouped_after_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = out[4] = 0;
  for (auto &sp : idx->shards) {
    out[0] += sp->c_gafter.load();
    out[1] += sp->c_gcount.load();
    out[2] += sp->c_gafter_side.load();
    out[3] += sp->c_gafter_redone.load();
    out[4] += sp->c_gafter_all.load();
  }
  return TSH_OK;
}

// ---- grouped search with several rows per group (tsh_group_rows_rule.h) ---------------------------------------------------
int32_t tsh_search_grouped_rows(tsh_index *idx, const float *queries, int32_t nq, int32_t k, int32_t m, double thr, const uint8_t *row_mask,
                                tsh_mask *mask_h, void *groups_p, int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_rows,
                                int32_t *out_count) {
  tsh_groups *groups = static_cast<tsh_groups *>(groups_p);
  if (row_mask && mask_h) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!groups) return set_err(TSH_E_BAD_ARG, "groups is NULL");
  if (m > GROUP_ROWS_MAX) return set_err(TSH_E_BAD_ARG, "rows_per_group %d outside [1, %d]", m, GROUP_ROWS_MAX);
  if (m <= 0 && k > 0) {  // (with k <= 0 or an empty index there is nothing to give rows of: the grouped search's trivial cases)
    bool any = !idx;
    for (size_t g = 0; idx && g < idx->shards.size(); ++g) {
      std::shared_lock<RwLock> sl = share(idx, idx->shards[g].get());
      any = any || idx->shards[g]->rows > 0;
    }
    if (any) return set_err(TSH_E_BAD_ARG, "rows_per_group %d outside [1, %d]", m, GROUP_ROWS_MAX);
  }
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (groups->idx != idx) return set_err(TSH_E_BAD_ARG, "the groups handle was made for another index (or its index was destroyed)");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (nq < 0) return set_err(TSH_E_BAD_ARG, "nq < 0");
  if (nq == 0) return TSH_OK;
  if (!queries || !out_count) return set_err(TSH_E_BAD_ARG, "queries / out_count is NULL");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  if (k <= 0 || m <= 0) return TSH_OK;
  if (!out_ids || !out_dist) return set_err(TSH_E_BAD_ARG, "out_ids / out_dist is NULL");
  std::shared_lock<std::shared_mutex> use(groups->use_mu);  // the array stays as it is until the finaliser has read it
  const size_t ns = idx->shards.size();
  const int32_t entries = tsh_default_block_entries(k);
  const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  const bool exact_all = grouped_after_exact_all(idx, groups);  // (the same two cases: tsh_group_rows_rule.h)
  std::vector<std::unique_ptr<uint8_t[]>> blocks(ns);
  std::vector<std::vector<std::vector<BlockEntry>>> spills(ns), extras(ns);
  int rc = for_each_shard(idx, [&](size_t g) -> int {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows == 0) return TSH_OK;
    blocks[g].reset(new uint8_t[bb * (size_t)nq]);
    spills[g].resize((size_t)nq);
    extras[g].resize((size_t)nq);
    SearchOut so;
    so.h_blocks = blocks[g].get();
    so.spill = &spills[g];
    so.extra = &extras[g];
    so.group_rows = m;
    so.exact_all = exact_all || !s->quar_ids.empty();
    int prc = TSH_OK;
    so.groups = current_part(groups, g, s, &prc);
    if (!so.groups) return prc;
    MaskSrc ms;
    int mrc = call_mask_for_shard(CallMask{row_mask, mask_h}, g, s, &ms);
    if (mrc) return mrc;
    // (the pipeline of single-query scans, never the batched path)
    return shard_search_blocks(s, queries, nq, k, ms, entries, &so, PIPE_DEPTH);
  });
  if (rc) return rc;
  // groups span shards: the finaliser's step runs once per query over every shard's entries
  const GroupTable table{groups->group_of.data(), (int64_t)groups->group_of.size()};
  const size_t km = (size_t)k * (size_t)m;
  parallel_for(nq, [&](int32_t q) {
    std::vector<EntryList> lists;
    for (size_t g = 0; g < ns; ++g) {
      if (!blocks[g]) continue;
      EntryList two[2];
      const size_t n_lists = shard_lists(blocks[g].get() + (size_t)q * bb, &spills[g][(size_t)q], &extras[g][(size_t)q], two);
      lists.insert(lists.end(), two, two + n_lists);
    }
    out_count[q] = finalize_grouped_rows(idx->metric, idx->dim, queries + (size_t)q * idx->dim, k, m, thr, lists.data(), lists.size(), table,
                                         out_ids + (size_t)q * km, out_dist + (size_t)q * km, out_group ? out_group + (size_t)q * k : nullptr,
                                         out_rows ? out_rows + (size_t)q * k : nullptr);
  });
  return TSH_OK;
}

int32_t tsh_search_grouped_rows_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = out[4] = 0;
  for (auto &sp : idx->shards) {
    out[0] += sp->c_grows.load();
    out[1] += sp->c_grows_marked.load();
    out[2] += sp->c_grows_side.load();
    out[3] += sp->c_grows_redone.load();
    out[4] += sp->c_grows_all.load();
  }
  return TSH_OK;
}

int32_t tsh_mask_create(tsh_index *idx, const uint8_t *bits, int64_t n_bytes, tsh_mask **out) {
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (n_bytes < 0 || (n_bytes > 0 && !bits)) return set_err(TSH_E_BAD_ARG, "bits is NULL / n_bytes < 0");
  std::unique_ptr<tsh_mask> m(new tsh_mask());
  m->idx = idx;
  try {
    m->bits.assign(bits, bits + n_bytes);
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for a %lld-byte mask", (long long)n_bytes);
  }
  if (const int rc = make_parts(m.get())) return rc;
  return register_handle(m, out);
}

int32_t tsh_mask_destroy(tsh_mask *mask) { return destroy_handle(mask); }

int64_t tsh_mask_kept(tsh_mask *mask) {
  if (!mask) return set_err(TSH_E_BAD_ARG, "mask is NULL");
  std::lock_guard<std::mutex> lk(g_mask_mu);
  tsh_index *idx = mask->idx;
  if (!idx) return set_err(TSH_E_BAD_ARG, "the mask's index was destroyed");
  int64_t kept = 0;
  for (size_t g = 0; g < idx->shards.size(); ++g) {
    Shard *s = idx->shards[g].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    int rc = TSH_OK;
    const MaskPart *p = current_part(mask, g, s, &rc);
    if (!p) return rc;
    kept += p->kept;
  }
  return kept;
}

// ---- attribute columns: a WHERE range term made into a mask handle on the device (tsh_where.hip.h) ----------------------
// (the attribute handle travels as void *, and create's out as the address of one: see the header)
int32_t tsh_attr_create(tsh_index *idx, const int64_t *values, int64_t n, void *out_p) {
  tsh_attr **out = static_cast<tsh_attr **>(out_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (n < 0 || (n > 0 && !values)) return set_err(TSH_E_BAD_ARG, "values is NULL / n < 0");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  std::unique_ptr<tsh_attr> a(new tsh_attr());
  a->idx = idx;
  try {
    a->values.assign(values, values + n);
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for %lld attribute values", (long long)n);
  }
  if (const int rc = make_parts(a.get())) return rc;
  return register_handle(a, out);
}

int32_t tsh_attr_set(void *attr, int64_t first_row_id, int64_t n, const int64_t *values) {
  tsh_attr *a = static_cast<tsh_attr *>(attr);
  if (!a) return set_err(TSH_E_BAD_ARG, "attr is NULL");
  if (first_row_id < 0 || n < 0 || (n > 0 && !values)) return set_err(TSH_E_BAD_ARG, "values is NULL / negative row range");
  return set_column(a, "the attribute handle's index was destroyed", n, no_check, [&] {
    try {
      if ((int64_t)a->values.size() < first_row_id + n) a->values.resize((size_t)(first_row_id + n), ATTR_NULL);
    } catch (...) {
      return set_err(TSH_E_OOM, "no memory for %lld attribute values", (long long)(first_row_id + n));
    }
    memcpy(a->values.data() + first_row_id, values, (size_t)n * sizeof(int64_t));
    return (int)TSH_OK;
  });
}

int32_t tsh_attr_destroy(void *attr) { return destroy_handle(static_cast<tsh_attr *>(attr)); }

int32_t tsh_mask_create_range(tsh_index *idx, void *attr_p, int64_t lo, int64_t hi, int32_t negate, tsh_mask *with,
                              int32_t combine, tsh_mask **out) {
  tsh_attr *attr = static_cast<tsh_attr *>(attr_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (combine != TSH_MASK_AND && combine != TSH_MASK_OR) return set_err(TSH_E_BAD_ARG, "combine %d is neither TSH_MASK_AND nor TSH_MASK_OR", combine);
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (!attr) return set_err(TSH_E_BAD_ARG, "attr is NULL");
  if (attr->idx != idx) return set_err(TSH_E_BAD_ARG, "the attribute handle was made for another index (or its index was destroyed)");
  return make_device_mask(idx, with, out, &attr, 1, [&](size_t g, Shard *s, MaskPart *p) {
    int rc = TSH_OK;
    const AttrPart *ap = current_part(attr, g, s, &rc);
    if (!ap) return rc;
    return mask_device_part(p, s, with, g, nullptr, 0, [&](hipStream_t st, int64_t rows, int32_t n_tiles, int64_t *, const uint64_t *d_with) {
      mask_range_kernel<<<where_grid(n_tiles), WHERE_BLOCK, 0, st>>>(ap->vals.d, rows, n_tiles, lo, hi, negate != 0 ? 1 : 0, d_with,
                                                                     combine, p->words.d);
    });
  });
}

// A whole WHERE clause in one launch and one finish per shard (tsh_where_plan.h plans it, W2 of tsh_where.hip.h runs it).
// make_device_mask as tsh_mask_create_range; what differs is the plan in front and one part per distinct column.
// Everything that can be refused is refused before any device work.  (terms travels as void *: see the header)
int32_t tsh_mask_create_where(tsh_index *idx, const void *terms_p, int32_t n_terms, tsh_mask *with, int32_t combine,
                              tsh_mask **out) {
  const tsh_where_term *terms = static_cast<const tsh_where_term *>(terms_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (combine != TSH_MASK_AND && combine != TSH_MASK_OR) return set_err(TSH_E_BAD_ARG, "combine %d is neither TSH_MASK_AND nor TSH_MASK_OR", combine);
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (!terms) return set_err(TSH_E_BAD_ARG, "terms is NULL");
  if (n_terms < 1 || n_terms > TSH_WHERE_MAX_TERMS) return set_err(TSH_E_BAD_ARG, "n_terms %d is not in 1 .. TSH_WHERE_MAX_TERMS", n_terms);
  WhereTermIn in[WHERE_MAX_TERMS];
  for (int32_t t = 0; t < n_terms; ++t) {
    if (terms[t].reserved != 0) return set_err(TSH_E_BAD_ARG, "term %d: reserved is not 0", t);
    in[t].column = terms[t].attr;
    in[t].lo = terms[t].lo;
    in[t].hi = terms[t].hi;
    in[t].set = terms[t].set;
    in[t].n_set = terms[t].n_set;
    in[t].kind = terms[t].kind;
    in[t].negate = terms[t].negate;
    in[t].clause = terms[t].clause;
  }
  WherePlan plan;
  try {
    if (const int e = where_plan(in, n_terms, &plan)) return set_err(TSH_E_BAD_ARG, "%s", where_plan_error(e));
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for the terms' sets");
  }
  tsh_attr *attrs[WHERE_MAX_COLUMNS];
  for (int c = 0; c < plan.n_cols; ++c) {
    attrs[c] = static_cast<tsh_attr *>(const_cast<void *>(plan.columns[c]));
    if (attrs[c]->idx != idx) return set_err(TSH_E_BAD_ARG, "the attribute handle was made for another index (or its index was destroyed)");
  }
  // (with is checked after the columns: a refusal make_device_mask makes ahead of any device work)
  const int32_t n_set = (int32_t)plan.set.size();
  return make_device_mask(idx, with, out, attrs, plan.n_cols, [&](size_t g, Shard *s, MaskPart *p) {
    int rc = TSH_OK;
    WhereArgs a{};
    for (int c = 0; c < plan.n_cols; ++c) {
      const AttrPart *ap = current_part(attrs[c], g, s, &rc);
      if (!ap) return rc;
      a.cols[c] = ap->vals.d;
    }
    memcpy(a.terms, plan.terms, sizeof(a.terms[0]) * (size_t)plan.n_terms);
    a.n_terms = plan.n_terms;
    a.n_cols = plan.n_cols;
    a.n_set = n_set;
    a.combine = combine;
    return mask_device_part(p, s, with, g, plan.set.data(), n_set, [&](hipStream_t st, int64_t rows, int32_t n_tiles, int64_t *d_set, const uint64_t *d_with) {
      mask_where_kernel<<<where_grid(n_tiles), WHERE_BLOCK, (size_t)n_set * 8, st>>>(a, rows, n_tiles, d_set, d_with, p->words.d);
    });
  });
}

// ---- tag columns: an array-valued WHERE term made into a mask handle on the device (tsh_tags.hip.h) ----------------------
// The attribute entries' shape; the column's normalisation, tsh_tags_set's splice, the slices and
// the term's set are tsh_tags_plan.h's.  (The tag handle travels as void *, and create's out as the address of one)
int32_t tsh_tags_create(tsh_index *idx, const int64_t *offsets, int64_t n, const int64_t *values, void *out_p) {
  tsh_tags **out = static_cast<tsh_tags **>(out_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (const int e = tags_check_csr(offsets, n, values)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  std::unique_ptr<tsh_tags> t(new tsh_tags());
  t->idx = idx;
  try {
    if (const int e = tags_normalise(offsets, n, values, &t->col)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for the tag lists of %lld rows", (long long)n);
  }
  // (a slice too large for the parts' 32-bit offsets is refused before any device work)
  for (size_t i = 0; i < idx->shards.size(); ++i) {
    Shard *s = idx->shards[i].get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (!tags_slice_fits(tags_slice_values(t->col, s->row_base, s->rows)))
      return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(TAGS_PLAN_SLICE_VALUES));
  }
  if (const int rc = make_parts(t.get())) return rc;
  return register_handle(t, out);
}

int32_t tsh_tags_set(void *tags, int64_t first_row_id, int64_t n, const int64_t *offsets, const int64_t *values) {
  tsh_tags *t = static_cast<tsh_tags *>(tags);
  if (!t) return set_err(TSH_E_BAD_ARG, "tags is NULL");
  if (first_row_id < 0) return set_err(TSH_E_BAD_ARG, "first_row_id < 0");
  if (const int e = tags_check_csr(offsets, n, values)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
  return set_column(t, "the tag handle's index was destroyed", n, no_check, [&] {
    try {
      if (const int e = tags_splice(&t->col, first_row_id, n, offsets, values)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
    } catch (...) {
      return set_err(TSH_E_OOM, "no memory for the tag lists of %lld rows", (long long)(first_row_id + n));
    }
    return (int)TSH_OK;
  });
}

int32_t tsh_tags_destroy(void *tags) { return destroy_handle(static_cast<tsh_tags *>(tags)); }

// make_device_mask as tsh_mask_create_range; what differs is the term's set in front (tags_query) and the part it
// reads.  Everything that can be refused on the arguments is refused before any device work
int32_t tsh_mask_create_tags(tsh_index *idx, void *tags_p, const int64_t *set, int64_t n_set, int32_t need, int32_t negate,
                             tsh_mask *with, int32_t combine, tsh_mask **out) {
  tsh_tags *tags = static_cast<tsh_tags *>(tags_p);
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (combine != TSH_MASK_AND && combine != TSH_MASK_OR) return set_err(TSH_E_BAD_ARG, "combine %d is neither TSH_MASK_AND nor TSH_MASK_OR", combine);
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (!tags) return set_err(TSH_E_BAD_ARG, "tags is NULL");
  TagsQuery q;
  try {
    if (const int e = tags_query(set, n_set, need, &q)) return set_err(TSH_E_BAD_ARG, "%s", tags_plan_error(e));
  } catch (...) {
    return set_err(TSH_E_OOM, "no memory for the term's set");
  }
  if (tags->idx != idx) return set_err(TSH_E_BAD_ARG, "the tag handle was made for another index (or its index was destroyed)");
  const int32_t n_q = (int32_t)q.set.size();
  return make_device_mask(idx, with, out, &tags, 1, [&](size_t g, Shard *s, MaskPart *p) {
    int rc = TSH_OK;
    const TagsPart *tp = current_part(tags, g, s, &rc);
    if (!tp) return rc;
    // (tp was built for the same rows: rows + 1 offsets, n_tiles valid words)
    return mask_device_part(p, s, with, g, q.set.data(), n_q, [&](hipStream_t st, int64_t rows, int32_t n_tiles, int64_t *d_set, const uint64_t *d_with) {
      mask_tags_kernel<<<where_grid(n_tiles), WHERE_BLOCK, (size_t)n_q * 8, st>>>(tp->off.d, tp->vals.d, tp->valid.d, rows, n_tiles, d_set, n_q,
                                                                                  (uint32_t)q.t, negate != 0 ? 1 : 0, d_with, combine, p->words.d);
    });
  });
}

// ---- facet counts: rows per value of an attribute or tag column, over the rows a search could return ----------------------
// facet_call does the work; what differs is the part a kernel reads and the column copy the quarantined rows are read from
int32_t tsh_attr_facets(tsh_index *idx, void *attr_p, tsh_mask *mask, int32_t kind, const int64_t *keys, int64_t n_keys,
                        int64_t *out_counts, int64_t *out_rest) {
  tsh_attr *attr = static_cast<tsh_attr *>(attr_p);
  FacetKeys k;
  if (const int rc = facet_check_args(idx, attr, "attr", kind, keys, n_keys, out_counts, out_rest, &k)) return rc;
  if (attr->idx != idx) return set_err(TSH_E_BAD_ARG, "the attribute handle was made for another index (or its index was destroyed)");
  if (mask && mask->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index (or its index was destroyed)");
  return facet_call(
      idx, attr, mask, k, out_counts, out_rest,
      [&](hipStream_t st, Shard *s, const AttrPart *ap, const uint64_t *d_mask, int32_t n_words, const int64_t *d_set,
          unsigned long long *d_cnt) {
        attr_facets_kernel<<<facet_grid(n_words), FACET_BLOCK, facet_lds_bytes(k.n()), st>>>(ap->vals.d, s->d_live, d_mask, s->rows, n_words,
                                                                                             d_set, k.n(), k.kind, d_cnt);
      },
      [&](const Shard *s, const uint64_t *mask_words, uint64_t *cnt) {
        facet_quar_attr(k, s->quar_ids.data(), s->quar_ids.size(), mask_words, attr->values.data(), (int64_t)attr->values.size(),
                        s->row_base, cnt);
      });
}

int32_t tsh_tags_facets(tsh_index *idx, void *tags_p, tsh_mask *mask, const int64_t *keys, int64_t n_keys, int64_t *out_counts,
                        int64_t *out_rest) {
  tsh_tags *tags = static_cast<tsh_tags *>(tags_p);
  FacetKeys k;
  if (const int rc = facet_check_args(idx, tags, "tags", FACET_VALUES, keys, n_keys, out_counts, out_rest, &k)) return rc;
  if (tags->idx != idx) return set_err(TSH_E_BAD_ARG, "the tag handle was made for another index (or its index was destroyed)");
  if (mask && mask->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index (or its index was destroyed)");
  return facet_call(
      idx, tags, mask, k, out_counts, out_rest,
      [&](hipStream_t st, Shard *s, const TagsPart *tp, const uint64_t *d_mask, int32_t n_words, const int64_t *d_set,
          unsigned long long *d_cnt) {
        // (tp was built for the same rows: rows + 1 offsets, n_words valid words)
        tags_facets_kernel<<<facet_grid(n_words), FACET_BLOCK, facet_lds_bytes(k.n()), st>>>(tp->off.d, tp->vals.d, tp->valid.d, s->d_live, d_mask,
                                                                                             s->rows, n_words, d_set, k.n(), d_cnt);
      },
      [&](const Shard *s, const uint64_t *mask_words, uint64_t *cnt) {
        facet_quar_tags(k, s->quar_ids.data(), s->quar_ids.size(), mask_words, tags->col, s->row_base, cnt);
      });
}

int32_t tsh_mask_read(tsh_mask *mask, uint8_t *out_bits, int64_t n_bytes) {
  if (!mask) return set_err(TSH_E_BAD_ARG, "mask is NULL");
  if (n_bytes < 0 || (n_bytes > 0 && !out_bits)) return set_err(TSH_E_BAD_ARG, "out_bits is NULL / n_bytes < 0");
  std::lock_guard<std::mutex> lk(g_mask_mu);
  if (!mask->idx) return set_err(TSH_E_BAD_ARG, "the mask's index was destroyed");
  std::lock_guard<std::mutex> ml(mask->mu);  // (a rebuild may be extending the bitmap)
  const size_t have = std::min<size_t>(mask->bits.size(), (size_t)n_bytes);
  if (have > 0) memcpy(out_bits, mask->bits.data(), have);
  if ((size_t)n_bytes > have) memset(out_bits + have, 0, (size_t)n_bytes - have);
  return TSH_OK;
}

// ---- asynchronous single-query searches ------------------------------------------
int32_t tsh_max_inflight(void) { return MAX_CTX; }

static int32_t submit_impl(tsh_index *idx, const float *query, int32_t k, const uint8_t *row_mask, tsh_mask *mask_h,
                           int32_t *out_ticket, const Cursor *after = nullptr) {
  if (!idx || !query || !out_ticket) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  if (k <= 0) return set_err(TSH_E_BAD_ARG, "k <= 0");
  if (mask_h && mask_h->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  *out_ticket = -1;
  std::unique_ptr<Ticket> t(new Ticket());
  t->k = k;
  t->entries = tsh_default_block_entries(k);
  t->query.assign(query, query + idx->dim);
  t->has_after = after != nullptr;
  if (after) t->after = *after;
  t->jobs.resize(idx->shards.size());
  t->locks.resize(idx->shards.size());
  int rc = TSH_OK;
  // The handle stays share-locked from submit to wait.  A caller that already has tickets open must not queue
  // behind a waiting append / delete (it would never reach the wait that lets the writer in): it is told to
  // drain its tickets first, which also keeps a caller that always has one open from starving the writer.
  const bool holding = idx->tickets_open.load() > 0;
  if (holding)
    for (auto &sp : idx->shards)
      if (sp->mu.writer_pending())
        return set_err(TSH_E_BUSY, "an append / delete is waiting for this handle's open asynchronous searches: "
                                   "wait for them, then submit again");
  for (size_t g = 0; g < idx->shards.size() && rc == TSH_OK; ++g) {
    Shard *s = idx->shards[g].get();
    s->mu.lock_shared_gate(holding);
    t->locks[g] = std::shared_lock<RwLock>(s->mu, std::adopt_lock);
    if (s->rows == 0) continue;
    // Contexts held by synchronous callers come back on their own, so wait for one -- unless the
    // un-waited tickets alone could hold them all: waiting would then never end for a caller that
    // submits before it waits
    Ctx *c = ctx_acquire(s, idx->tickets_open.load() < MAX_CTX);
    if (!c) {
      rc = set_err(TSH_E_BUSY, "%d asynchronous searches are already in flight on this handle", MAX_CTX);
      break;
    }
    t->jobs[g].c = c;
    std::vector<uint64_t> words;
    std::vector<uint32_t> list_ids;  // (job_enqueue copies what it keeps of either before it returns)
    MaskSrc src;
    rc = call_mask_for_shard(CallMask{row_mask, mask_h}, g, s, &src);
    if (rc) break;
    JobReq rq(t->query.data(), k, t->entries);  // (the ticket's copy: a cursor job may be redone from it at the wait)
    rq.mask = resolve_mask(s, src, k, t->entries, &words, &list_ids);
    rq.after = after;
    rq.mask_dies = true;
    rc = job_enqueue(s, &t->jobs[g], rq);
  }
  if (rc != TSH_OK) {
    std::string keep = g_err;
    for (size_t g = 0; g < idx->shards.size(); ++g) job_abandon(idx->shards[g].get(), &t->jobs[g]);
    g_err = keep;
    return rc;
  }
  std::lock_guard<std::mutex> lk(idx->tk_mu);
  int slot = -1;
  for (size_t i = 0; i < idx->tickets.size(); ++i)
    if (!idx->tickets[i]) {
      slot = (int)i;
      break;
    }
  if (slot < 0) {
    idx->tickets.emplace_back();
    slot = (int)idx->tickets.size() - 1;
  }
  idx->tickets[(size_t)slot] = std::move(t);
  idx->tickets_open.fetch_add(1);
  *out_ticket = slot;
  return TSH_OK;
}

int32_t tsh_search_submit(tsh_index *idx, const float *query, int32_t k, const uint8_t *row_mask, int32_t *out_ticket) {
  return submit_impl(idx, query, k, row_mask, nullptr, out_ticket);
}
int32_t tsh_search_submit_masked(tsh_index *idx, const float *query, int32_t k, tsh_mask *mask, int32_t *out_ticket) {
  return submit_impl(idx, query, k, nullptr, mask, out_ticket);
}

int32_t tsh_search_submit_after(tsh_index *idx, const float *query, int32_t k, const uint8_t *row_mask, tsh_mask *mask,
                                double after_dist, int64_t after_id, int32_t *out_ticket) {
  if (row_mask && mask) return set_err(TSH_E_BAD_ARG, "row_mask and mask are both given: at most one");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  Cursor cur;
  return submit_impl(idx, query, k, row_mask, mask, out_ticket, Cursors{&after_dist, &after_id}.at(0, &cur));
}

int32_t tsh_search_ready(tsh_index *idx, int32_t ticket) {
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  std::lock_guard<std::mutex> lk(idx->tk_mu);
  if (ticket < 0 || (size_t)ticket >= idx->tickets.size() || !idx->tickets[(size_t)ticket])
    return set_err(TSH_E_BAD_ARG, "unknown ticket %d", ticket);
  Ticket *t = idx->tickets[(size_t)ticket].get();
  for (size_t g = 0; g < idx->shards.size(); ++g) {
    if (!t->jobs[g].c) continue;
    if (hipSetDevice(idx->shards[g]->device) != hipSuccess) return set_err(TSH_E_HIP, "hipSetDevice failed");
    const hipError_t e = hipEventQuery(t->jobs[g].c->ev_done);
    if (e == hipErrorNotReady) return 0;
    if (e != hipSuccess) return set_err(TSH_E_HIP, "hipEventQuery failed: %s", hipGetErrorString(e));
  }
  return 1;
}

int32_t tsh_search_wait(tsh_index *idx, int32_t ticket, double thr, int64_t *out_ids, double *out_dist,
                        int32_t *out_count) {
  if (!idx || !out_ids || !out_dist || !out_count) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  std::unique_ptr<Ticket> t;
  {
    std::lock_guard<std::mutex> lk(idx->tk_mu);
    if (ticket < 0 || (size_t)ticket >= idx->tickets.size() || !idx->tickets[(size_t)ticket])
      return set_err(TSH_E_BAD_ARG, "unknown ticket %d", ticket);
    t = std::move(idx->tickets[(size_t)ticket]);
    idx->tickets_open.fetch_sub(1);
  }
  *out_count = 0;
  int rc = TSH_OK;
  std::vector<std::vector<BlockEntry>> spills(idx->shards.size()), extras(idx->shards.size());
  std::vector<EntryList> lists;
  for (size_t g = 0; g < idx->shards.size(); ++g) {
    Job &j = t->jobs[g];
    if (!j.c) continue;
    Shard *s = idx->shards[g].get();
    if (rc == TSH_OK) {
      rc = job_finish(s, &j, &spills[g], &extras[g]);
    } else {
      job_settle(s, &j);
    }
    if (rc == TSH_OK) {
      EntryList two[2];
      const size_t n_lists = shard_lists(j.c->h_block, &spills[g], &extras[g], two);
      lists.insert(lists.end(), two, two + n_lists);
    }
  }
  if (rc == TSH_OK)
    *out_count = finalize_query(idx->metric, idx->dim, t->query.data(), t->k, thr, lists, out_ids, out_dist,
                                t->has_after ? &t->after : nullptr);
  std::string keep = g_err;
  for (size_t g = 0; g < idx->shards.size(); ++g)  // (after the finaliser has read the blocks: they are the contexts')
    job_abandon(idx->shards[g].get(), &t->jobs[g]);
  g_err = keep;
  return rc;
}

namespace {
// tsh_search_shard and its kin; r.after: a cursor per query (tsh_search_shard_after), or none; r.mask: the caller's bitmap,
// or a mask handle in its place (tsh_search_shard_masked)
int32_t search_shard_impl(tsh_index *idx, const ShardSearchReq &r, void *stream) {
  if (!idx || idx->shards.size() != 1) return set_err(TSH_E_BAD_ARG, "needs a single-shard handle");
  if (r.mask.handle && r.mask.handle->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (r.nq <= 0 || !r.queries || !r.d_blocks || (r.k <= 0 && !r.groups) || r.entries < 1)
    return set_err(TSH_E_BAD_ARG, "bad nq / k / entries / pointers");
  Shard *s = idx->shards[0].get();
  // (a grouped call: the handle's array stays as it is while the shard's part of it is read)
  std::shared_lock<std::shared_mutex> use;
  if (r.groups && !r.groups_held) use = std::shared_lock<std::shared_mutex>(r.groups->use_mu);
  std::shared_lock<RwLock> sl = share(idx, s);
  // an empty shard contributes empty blocks, and so does a grouped call for no groups at all
  if (s->rows == 0 || r.k <= 0) return write_empty_blocks(s, r.nq, std::max(r.k, 0), r.entries, 0, r.d_blocks);
  MaskSrc ms;
  int rc = call_mask_for_shard(r.mask, 0, s, &ms);
  if (rc) return rc;
  SearchOut so;
  so.d_blocks = r.d_blocks;
  so.user_stream = static_cast<hipStream_t>(stream);
  so.after = r.after;
  if (r.groups && !(so.groups = current_part(r.groups, 0, s, &rc))) return rc;
  if (r.after || r.groups)  // a cursor call or a grouped call is never batched: every query is its own scan
    return shard_search_blocks(s, r.queries, r.nq, r.k, ms, r.entries, &so, PIPE_DEPTH);
  return shard_search_any(s, s->batch, idx->batch_min_nq.load(), r.queries, r.nq, r.k, ms, r.entries, &so);
}
}  // namespace

int32_t tsh_search_shard(tsh_index *idx, const float *queries, int32_t nq, int32_t k,
                         const uint8_t *row_mask, int32_t entries, void *d_out_blocks, void *stream) {
  return search_shard_impl(idx, ShardSearchReq{queries, nq, k, entries, {row_mask, nullptr}, {}, static_cast<uint8_t *>(d_out_blocks)}, stream);
}
int32_t tsh_search_shard_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                               const double *after_dist, const int64_t *after_id, int32_t entries, void *d_out_blocks, void *stream) {
  if (!after_dist || !after_id) return set_err(TSH_E_BAD_ARG, "after_dist / after_id is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return search_shard_impl(
      idx, ShardSearchReq{queries, nq, k, entries, {row_mask, nullptr}, {after_dist, after_id}, static_cast<uint8_t *>(d_out_blocks)}, stream);
}
int32_t tsh_search_shard_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, tsh_mask *mask,
                                const double *after_dist, const int64_t *after_id, int32_t entries, void *d_out_blocks, void *stream) {
  if (half_cursor(after_dist, after_id)) return set_err(TSH_E_BAD_ARG, "after_dist / after_id: both or neither");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return search_shard_impl(
      idx, ShardSearchReq{queries, nq, k, entries, {nullptr, mask}, {after_dist, after_id}, static_cast<uint8_t *>(d_out_blocks)}, stream);
}
int32_t tsh_search_shard_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask, tsh_mask *mask,
                                 void *groups, int32_t entries, void *d_out_blocks, void *stream) {
  tsh_groups *g = static_cast<tsh_groups *>(groups);
  int rc = check_shard_groups(idx, CallMask{row_mask, mask}, g);
  if (rc) return rc;
  return search_shard_impl(idx, ShardSearchReq{queries, nq, k, entries, {row_mask, mask}, {}, static_cast<uint8_t *>(d_out_blocks), g}, stream);
}

// ---- progressive shard search ---------------------------------------------------------------------------------
// tsh_search_shard answers when the LAST of its queries is done; a caller that exchanges the blocks group by group
// (tsh_search_sharded, sharded.py) then starts group g + 1's scans only after group g's have drained, and every
// group pays the fill and the drain of the scan pipeline (measured: ~45 us per group on a 125 k-row shard, a fifth of
// a ten-query group).  Here the scans of ALL nq queries run as ONE pipeline on a library thread -- group boundaries
// do not exist for the GPU -- and the caller is told how many LEADING queries' blocks are final.
struct tsh_shard_stream {
  tsh_index *idx = nullptr;
  ShardSearchReq req;  // (a mask handle is kept as it is, no bitmap is copied)
  ShardStreamOpts opt;
  std::vector<float> own_queries;  // opt.copy_inputs: req points into these
  std::vector<uint8_t> own_mask;
  std::vector<double> own_after_dist;
  std::vector<int64_t> own_after_id;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<char> done_q;  // single-query route: query q's block is final
  int32_t done = 0;          // leading queries whose blocks are final
  bool finished = false;     // the worker has returned
  std::atomic<int32_t> done_seen{0};  // copies of the two for a caller that polls before it sleeps
  std::atomic<bool> finished_seen{false};
  // single-query route: leading queries whose kernels are all enqueued, and the event behind each one's block
  // writer -- what a caller needs to order its own stream behind a group's blocks without waiting for them
  std::vector<char> enq_q;
  std::vector<hipEvent_t> ev_q;
  std::vector<hipStream_t> st_q;  // the stream ev_q[q] was recorded on
  std::vector<uint64_t> seq_q;    // ... and when (the device's enqueue order)
  int32_t enq = 0;
  std::atomic<int32_t> enq_seen{0};
  std::atomic<int> route{0};  // 0 not decided yet, 1 every query its own scan (events exist), 2 anything else
  int rc = TSH_OK;
  std::string err;
  double busy_us = 0;  // worker: first enqueue to last block
  std::thread th;      // the search's own thread (unless opt.exec)

  void publish(int32_t upto) {  // queries [0, upto) are final
    {
      std::lock_guard<std::mutex> lk(mu);
      done = std::max(done, upto);
      done_seen.store(done, std::memory_order_release);
    }
    cv.notify_all();
  }
  void mark_enqueued(int32_t q, hipEvent_t ev, hipStream_t where, uint64_t seq) {
    bool moved = false;
    {
      std::lock_guard<std::mutex> lk(mu);
      ev_q[(size_t)q] = ev;
      st_q[(size_t)q] = where;
      seq_q[(size_t)q] = seq;
      enq_q[(size_t)q] = 1;
      while (enq < req.nq && enq_q[(size_t)enq]) {
        ++enq;
        moved = true;
      }
      enq_seen.store(enq, std::memory_order_release);
    }
    if (moved) cv.notify_all();
  }
  void mark(int32_t q) {
    bool moved = false;
    {
      std::lock_guard<std::mutex> lk(mu);
      done_q[(size_t)q] = 1;
      while (done < req.nq && done_q[(size_t)done]) {
        ++done;
        moved = true;
      }
      done_seen.store(done, std::memory_order_release);
    }
    if (moved) cv.notify_all();
  }
  int body() {
    Shard *s = idx->shards[0].get();
    // (a grouped search: the handle's array stays as it is for as long as this thread reads the shard's part of it)
    std::shared_lock<std::shared_mutex> use;
    if (req.groups && !req.groups_held) use = std::shared_lock<std::shared_mutex>(req.groups->use_mu);
    std::shared_lock<RwLock> sl = share(idx, s);
    HIPCHK(hipSetDevice(s->device));
    if (!own_mask.empty()) {
      // _begin copied the mask for the rows the shard had THEN; rows appended between that look and this lock are
      // beyond the caller's mask: not kept (zero bits), and never read past the copy's end
      const size_t need = (size_t)((s->row_base + s->rows + 7) / 8);
      if (own_mask.size() < need) {
        own_mask.resize(need, 0);
        req.mask.bytes = own_mask.data();
      }
    }
    MaskSrc ms;
    int mrc = call_mask_for_shard(req.mask, 0, s, &ms);
    if (mrc) return mrc;
    const int32_t nq = req.nq, k = req.k, entries = req.entries;
    const size_t bb = (size_t)tsh_candidate_block_bytes(entries);
    if (s->rows == 0 || k <= 0) {  // an empty shard contributes empty blocks (k <= 0: a grouped search for no groups)
      route.store(2, std::memory_order_release);
      int erc = write_empty_blocks(s, nq, std::max(k, 0), entries, opt.tag, req.d_blocks);
      if (erc) return erc;
      publish(nq);
      return TSH_OK;
    }
    const int32_t min_nq = idx->batch_min_nq.load();
    const int32_t st = opt.step > 0 ? std::min(opt.step, nq) : nq;
    const GroupPart *gpart = nullptr;
    if (req.groups && !(gpart = current_part(req.groups, 0, s, &mrc))) return mrc;
    // (a cursor call or a grouped call is never batched, whatever step or the handle's batch threshold say)
    if (req.after || gpart || !shard_takes_batch(s, min_nq, st, k)) {  // one pipeline over all queries
      done_q.assign((size_t)nq, 0);
      enq_q.assign((size_t)nq, 0);
      ev_q.assign((size_t)nq, nullptr);
      st_q.assign((size_t)nq, nullptr);
      seq_q.assign((size_t)nq, 0);
      SearchOut so;
      so.d_blocks = req.d_blocks;
      so.tag = opt.tag;
      so.leave_overflow = opt.leave_overflow;
      so.after = req.after;
      so.groups = gpart;
      so.on_done = [this](int32_t q) { mark(q); };
      so.on_enqueued = [this](int32_t q, hipEvent_t ev, hipStream_t where, uint64_t seq) { mark_enqueued(q, ev, where, seq); };
      route.store(1, std::memory_order_release);
      cv.notify_all();
      return shard_search_blocks(s, req.queries, nq, k, ms, entries, &so, PIPE_DEPTH);
    }
    route.store(2, std::memory_order_release);
    cv.notify_all();
    // matrix-core route: a call per step (the batched path answers a call as a whole; the next step's call overlaps
    // the caller's work on this one as before)
    for (int32_t q0 = 0; q0 < nq; q0 += st) {
      const int32_t gq = std::min(st, nq - q0);
      SearchOut so;
      so.d_blocks = req.d_blocks + (size_t)q0 * bb;
      so.tag = opt.tag;  // (queries the batch hands back to the single-query path carry it at once)
      int r = shard_search_any(s, s->batch, min_nq, req.queries + (size_t)q0 * s->dim, gq, k, ms, entries, &so);
      if (r) return r;
      if (opt.tag) {  // the matrix-core path's blocks get their generation now (host-synchronised: they are final)
        stamp_tag_kernel<<<(unsigned)((gq + 63) / 64), 64, 0, s->aux_stream>>>(so.d_blocks, bb, gq, opt.tag);
        HIPCHK(hipStreamSynchronize(s->aux_stream));
      }
      publish(q0 + gq);
    }
    return TSH_OK;
  }
  void run() {
    const double t0 = now_us();
    int r = body();
    std::string e = r ? g_err : std::string();
    {
      std::lock_guard<std::mutex> lk(mu);
      rc = r;
      err = e;
      finished = true;
      busy_us = now_us() - t0;
      if (route.load() == 0) route.store(2);
      finished_seen.store(true, std::memory_order_release);
    }
    cv.notify_all();
  }
};

namespace {
int shard_stream_begin(tsh_index *idx, const ShardSearchReq &r, const ShardStreamOpts &opt, tsh_shard_stream **out) {
  if (!out) return set_err(TSH_E_BAD_ARG, "out is NULL");
  *out = nullptr;
  if (!idx || idx->shards.size() != 1) return set_err(TSH_E_BAD_ARG, "needs a single-shard handle");
  if (r.mask.handle && r.mask.handle->idx != idx) return set_err(TSH_E_BAD_ARG, "the mask handle was made for another index");
  if (r.nq <= 0 || !r.queries || !r.d_blocks || (r.k <= 0 && !r.groups) || r.entries < 1 || opt.step < 0)
    return set_err(TSH_E_BAD_ARG, "bad nq / k / entries / step / pointers");
  std::unique_ptr<tsh_shard_stream> st(new tsh_shard_stream());
  st->idx = idx;
  st->req = r;
  st->opt = opt;
  if (opt.copy_inputs) {
    Shard *s = idx->shards[0].get();
    st->own_queries.assign(r.queries, r.queries + (size_t)r.nq * (size_t)s->dim);
    st->req.queries = st->own_queries.data();
    if (r.after) {
      st->own_after_dist.assign(r.after.dist, r.after.dist + r.nq);
      st->own_after_id.assign(r.after.id, r.after.id + r.nq);
      st->req.after = Cursors{st->own_after_dist.data(), st->own_after_id.data()};
    }
    if (r.mask.bytes) {
      int64_t bits;
      {
        std::shared_lock<RwLock> sl = share(idx, s);
        bits = s->row_base + s->rows;  // the mask is global: one bit per row id below this shard's end
      }
      st->own_mask.assign(r.mask.bytes, r.mask.bytes + (size_t)((bits + 7) / 8));
      st->req.mask.bytes = st->own_mask.data();
    }
  }
  tsh_shard_stream *p = st.get();
  if (opt.exec) {
    opt.exec->post([p] { p->run(); });
  } else {
    try {
      st->th = std::thread([p] { p->run(); });
    } catch (...) {
      return set_err(TSH_E_OOM, "could not start the search thread");
    }
  }
  *out = st.release();
  return TSH_OK;
}

// Blocks until the kernels of the first min(want, nq) queries are all enqueued -- or it is clear they never will be
// one by one (matrix-core route, an empty shard, a failure).  -> the number of events written to `after` (at most
// `max`): the events behind the block writers of those queries that may still be running (a job further back than
// the pipeline is deep has been finished by the host); 0 = no stream order to be had, wait for _progress instead.
// (An event may meanwhile belong to a LATER query of the same pipeline -- its context was reused: waiting for it
// then waits a little longer than needed, never too short.)
int shard_stream_enqueued(tsh_shard_stream *st, int32_t want, hipEvent_t *after, int max) {
  want = std::min(want, st->req.nq);
  if (!blocking_wait()) {
    const double t_end = now_us() + 3000.0;
    while (st->enq_seen.load(std::memory_order_acquire) < want && st->route.load(std::memory_order_acquire) != 2 &&
           !st->finished_seen.load(std::memory_order_acquire) && now_us() < t_end)
      cpu_relax();
  }
  std::unique_lock<std::mutex> lk(st->mu);
  st->cv.wait(lk, [&] { return st->enq >= want || st->route.load() == 2 || st->finished; });
  if (st->route.load() != 1 || st->enq < want) return 0;
  // of the jobs that share a stream only the one enqueued LAST matters (a stream's kernels finish in order), so this
  // is two or three events, not eight: every wait is a packet the consumer's queue has to work through
  int n = 0;
  hipStream_t seen[MAX_CTX];
  uint64_t seen_seq[MAX_CTX];
  for (int32_t q = want - 1; q >= std::max(0, want - (int32_t)MAX_CTX); --q) {
    if (!st->ev_q[(size_t)q] || st->done_q[(size_t)q]) continue;
    int at = -1;
    for (int i = 0; i < n; ++i)
      if (seen[i] == st->st_q[(size_t)q]) at = i;
    if (at < 0) {
      if (n == max) continue;  // (cannot happen: max >= MAX_CTX jobs)
      at = n++;
      seen[at] = st->st_q[(size_t)q];
      seen_seq[at] = 0;
    }
    if (st->seq_q[(size_t)q] >= seen_seq[at]) {
      seen_seq[at] = st->seq_q[(size_t)q];
      after[at] = st->ev_q[(size_t)q];
    }
  }
  if (n == 0) after[n++] = st->ev_q[(size_t)(want - 1)];  // (all final already: any completed event will do)
  return n;
}

// blocks until min(want, nq) leading queries are final, or the search has ended; -> its status so far
int shard_stream_progress(tsh_shard_stream *st, int32_t want, int32_t *out_done) {
  want = std::min(want, st->req.nq);
  if (!blocking_wait()) {
    // the caller has nothing else to do and (blocking_wait: at least three CPUs per rank) a core to do it on: poll for
    // a few milliseconds before sleeping -- being woken through the condition variable costs 20-50 us, on the last
    // group of a call in full view
    const double t_end = now_us() + 3000.0;
    while (st->done_seen.load(std::memory_order_acquire) < want && !st->finished_seen.load(std::memory_order_acquire) &&
           now_us() < t_end)
      cpu_relax();
  }
  std::unique_lock<std::mutex> lk(st->mu);
  st->cv.wait(lk, [&] { return st->done >= want || st->finished; });
  if (out_done) *out_done = st->done;
  if (st->done >= want) return TSH_OK;  // (whatever happens to later queries)
  g_err = st->err;  // the search ended before it got there
  return st->rc != TSH_OK ? st->rc : set_err(TSH_E_HIP, "the shard search ended early");
}

int shard_stream_end(tsh_shard_stream *st, double *busy_us = nullptr) {
  if (st->opt.exec) st->opt.exec->wait();
  else if (st->th.joinable()) st->th.join();
  const int rc = st->rc;
  if (rc) g_err = st->err;
  if (busy_us) *busy_us = st->busy_us;
  delete st;
  return rc;
}
}  // namespace

// (the public entries: the caller's arrays are copied, the search runs on a thread of its own)
int32_t tsh_search_shard_begin(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                               int32_t entries, void *d_out_blocks, int32_t step, tsh_shard_stream **out) {
  return shard_stream_begin(idx, ShardSearchReq{queries, nq, k, entries, {row_mask, nullptr}, {}, static_cast<uint8_t *>(d_out_blocks)},
                            ShardStreamOpts{step, /*copy_inputs=*/true}, out);
}
int32_t tsh_search_shard_begin_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                                     const double *after_dist, const int64_t *after_id, int32_t entries, void *d_out_blocks,
                                     int32_t step, tsh_shard_stream **out) {
  if (out) *out = nullptr;
  if (!after_dist || !after_id) return set_err(TSH_E_BAD_ARG, "after_dist / after_id is NULL");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return shard_stream_begin(
      idx, ShardSearchReq{queries, nq, k, entries, {row_mask, nullptr}, {after_dist, after_id}, static_cast<uint8_t *>(d_out_blocks)},
      ShardStreamOpts{step, /*copy_inputs=*/true}, out);
}
int32_t tsh_search_shard_begin_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, tsh_mask *mask,
                                      const double *after_dist, const int64_t *after_id, int32_t entries, void *d_out_blocks,
                                      int32_t step, tsh_shard_stream **out) {
  if (out) *out = nullptr;
  if (half_cursor(after_dist, after_id)) return set_err(TSH_E_BAD_ARG, "after_dist / after_id: both or neither");
  if (!idx && device_count_cached() <= 0) return set_err(TSH_E_NO_DEVICE, "no HIP device available");
  return shard_stream_begin(
      idx, ShardSearchReq{queries, nq, k, entries, {nullptr, mask}, {after_dist, after_id}, static_cast<uint8_t *>(d_out_blocks)},
      ShardStreamOpts{step, /*copy_inputs=*/true}, out);
}
int32_t tsh_search_shard_begin_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask, tsh_mask *mask,
                                       void *groups, int32_t entries, void *d_out_blocks, int32_t step, tsh_shard_stream **out) {
  if (out) *out = nullptr;
  tsh_groups *g = static_cast<tsh_groups *>(groups);
  int rc = check_shard_groups(idx, CallMask{row_mask, mask}, g);
  if (rc) return rc;
  return shard_stream_begin(idx, ShardSearchReq{queries, nq, k, entries, {row_mask, mask}, {}, static_cast<uint8_t *>(d_out_blocks), g},
                            ShardStreamOpts{step, /*copy_inputs=*/true}, out);
}
int32_t tsh_search_shard_progress(tsh_shard_stream *st, int32_t want, int32_t *out_done) {
  if (!st) return set_err(TSH_E_BAD_ARG, "stream is NULL");
  return shard_stream_progress(st, want, out_done);
}
int32_t tsh_search_shard_end(tsh_shard_stream *st) {
  if (!st) return TSH_OK;
  return shard_stream_end(st);
}

namespace {
// tsh_merge_candidates; after: a cursor per query (tsh_merge_candidates_after), or none
int32_t merge_candidates_impl(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k, double thr,
                              Cursors after, const void *blocks, int32_t n_blocks,
                              int32_t entries, int64_t *out_ids, double *out_dist, int32_t *out_count, int32_t *needed_entries,
                              const GroupTable *table = nullptr, int32_t *out_group = nullptr) {
  if (metric < 0 || metric > 2 || dim <= 0 || nq < 0 || n_blocks < 0 || entries < 0)
    return set_err(TSH_E_BAD_ARG, "bad metric / dim / nq / n_blocks / entries");
  if (nq == 0) return TSH_OK;
  if (!queries || !blocks || !out_count) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  for (int32_t q = 0; q < nq; ++q) out_count[q] = 0;
  if (needed_entries) *needed_entries = entries;
  if (k <= 0) return TSH_OK;
  if (!out_ids || !out_dist) return set_err(TSH_E_BAD_ARG, "out_ids / out_dist is NULL");
  size_t bb = (size_t)tsh_candidate_block_bytes(entries);
  const uint8_t *base = static_cast<const uint8_t *>(blocks);
  uint32_t need = 0;
  for (int32_t b = 0; b < n_blocks; ++b)
    for (int32_t q = 0; q < nq; ++q) {
      const BlockHeader *h = reinterpret_cast<const BlockHeader *>(base + ((size_t)b * nq + q) * bb);
      if (h->entries != (uint32_t)entries)
        return set_err(TSH_E_FORMAT, "block %d/%d entries %u != %d", b, q, h->entries, entries);
      if (h->count > h->entries) need = std::max(need, h->count);
    }
  if (need) {
    if (needed_entries) *needed_entries = (int32_t)round_up(need, 64);
    return set_err(TSH_E_OVERFLOW, "a candidate block needs %u entries (have %d)", need, entries);
  }
  parallel_for(nq, [&](int32_t q) {
    std::vector<EntryList> lists;
    for (int32_t b = 0; b < n_blocks; ++b) lists.push_back(block_list(base + ((size_t)b * nq + q) * bb));  // (count <= entries: see above)
    if (table) {  // finalize_grouped over the union of the blocks' entries: the step a grouped search runs over several devices
      out_count[q] = finalize_grouped(metric, dim, queries + (size_t)q * dim, k, thr, lists.data(), lists.size(), *table,
                                      out_ids + (size_t)q * k, out_dist + (size_t)q * k, out_group ? out_group + (size_t)q * k : nullptr);
      return;
    }
    Cursor cur;
    out_count[q] = finalize_query(metric, dim, queries + (size_t)q * dim, k, thr, lists,
                                  out_ids + (size_t)q * k, out_dist + (size_t)q * k, after.at(q, &cur));
  });
  return TSH_OK;
}
}  // namespace

int32_t tsh_merge_candidates(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k,
                             double thr, const void *blocks, int32_t n_blocks, int32_t entries,
                             int64_t *out_ids, double *out_dist, int32_t *out_count,
                             int32_t *needed_entries) {
  return merge_candidates_impl(metric, dim, queries, nq, k, thr, Cursors(), blocks, n_blocks, entries, out_ids, out_dist,
                               out_count, needed_entries);
}
int32_t tsh_merge_candidates_after(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k, double thr,
                                   const double *after_dist, const int64_t *after_id, const void *blocks, int32_t n_blocks,
                                   int32_t entries, int64_t *out_ids, double *out_dist, int32_t *out_count,
                                   int32_t *needed_entries) {
  if (!after_dist || !after_id) return set_err(TSH_E_BAD_ARG, "after_dist / after_id is NULL");
  return merge_candidates_impl(metric, dim, queries, nq, k, thr, Cursors{after_dist, after_id}, blocks, n_blocks, entries, out_ids, out_dist,
                               out_count, needed_entries);
}
int32_t tsh_merge_candidates_grouped(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k, double thr,
                                     const int32_t *group_of, int64_t n_group_of, const void *blocks, int32_t n_blocks, int32_t entries,
                                     int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_count, int32_t *needed_entries) {
  if (n_group_of < 0 || (n_group_of > 0 && !group_of)) return set_err(TSH_E_BAD_ARG, "group_of is NULL / n_group_of < 0");
  const GroupTable table{group_of, n_group_of};
  return merge_candidates_impl(metric, dim, queries, nq, k, thr, Cursors(), blocks, n_blocks, entries, out_ids, out_dist, out_count,
                               needed_entries, &table, out_group);
}

int32_t tsh_get_counters(tsh_index *idx, tsh_counters *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  memset(out, 0, sizeof *out);
  for (auto &sp : idx->shards) {
    Shard *s = sp.get();
    std::shared_lock<RwLock> sl = share(idx, s);
    if (s->rows > 0) out->rows = std::max(out->rows, s->row_base + s->rows);
    out->deleted_rows += s->deleted;
    out->searches = std::max<int64_t>(out->searches, s->c_searches.load());
    out->scan_launches += s->c_scans.load();
    out->batch_launches += s->c_batches.load();
    out->fallback_searches += s->c_fallbacks.load();
    out->batch_plane_fallbacks += s->c_plane_fallbacks.load();
    out->batch_scan_fallbacks += s->c_scan_fallbacks.load();
    out->list_scans += s->c_list_scans.load();
    out->exact_scans += s->c_exact_scans.load();
    out->exact_redone += s->c_pick_redone.load();
    out->candidates_total += s->c_cands.load();
    int64_t b = s->bytes;
    {
      std::lock_guard<std::mutex> lk(s->ctx_mu);
      for (auto &c : s->ctx_all) b += c->bytes;
      out->scan_us_sum += s->scan_us_sum;
      out->scan_us_samples += s->scan_us_samples;
      out->batch_kernel_last = s->batch_kernel_last;
    }
    out->bytes_resident += b;
    if (s->safe_mode()) out->safe_mode = 1;
    out->quarantined_rows += (int32_t)s->quar_ids.size();
    out->device_id = s->device;
  }
  return TSH_OK;
}

// A measurement / probe entry's scaffold: the handle's one shard under its shared lock, a context prepared for the default
// block of k = 100 and given back when the entry returns, the query zero-padded in c->h_query and on its way to c->d_query
// on the aux stream (st)
struct ScanHook {
  Shard *s = nullptr;
  Ctx *c = nullptr;
  hipStream_t st = nullptr;
  std::shared_lock<RwLock> sl;
  ~ScanHook() {
    if (!c) return;
    if (st) (void)hipStreamSynchronize(st);  // (an entry that gave up: c->h_query is read until the upload is through)
    ctx_release(s, c);
  }
};
// args_ok: the entry's own arguments; need_mask: room for a caller's mask words in the context
int scan_hook_begin(ScanHook *h, tsh_index *idx, const float *query, bool args_ok, bool need_mask = false) {
  if (!idx || idx->shards.size() != 1 || !query || !args_ok) return set_err(TSH_E_BAD_ARG, "bad arguments");
  Shard *s = h->s = idx->shards[0].get();
  h->sl = share(idx, s);
  if (s->rows == 0) return set_err(TSH_E_BAD_ARG, "empty index");
  Ctx *c = h->c = ctx_acquire(s, true);
  int rc = ctx_prepare(s, c, tsh_default_block_entries(100), need_mask);
  if (rc) return rc;
  h->st = s->aux_stream;
  memcpy(c->h_query, query, (size_t)s->dim * sizeof(float));
  for (int64_t j = s->dim; j < s->ld; ++j) c->h_query[j] = 0.f;
  HIPCHK(hipMemcpyAsync(c->d_query, c->h_query, (size_t)s->ld * sizeof(float), hipMemcpyHostToDevice, h->st));
  return TSH_OK;
}
// What the hook's scan left in c->d_keys, waited for: every row's key as a float, NaN where the key is dead
int scan_hook_keys(const ScanHook &h, float *out_keys) {
  std::vector<uint32_t> keys((size_t)h.s->rows);
  HIPCHK(hipMemcpyAsync(keys.data(), h.c->d_keys, keys.size() * 4, hipMemcpyDeviceToHost, h.st));
  HIPCHK(hipStreamSynchronize(h.st));
  HIPCHK(hipGetLastError());
  for (size_t i = 0; i < keys.size(); ++i) out_keys[i] = keys[i] >= KEY_NAN ? std::nanf("") : h_key2f(keys[i]);
  return TSH_OK;
}

int32_t tsh_bench_scan(tsh_index *idx, const float *query, int32_t iters, const uint8_t *row_mask,
                       double *out_avg_us) {
  ScanHook h;
  int rc = scan_hook_begin(&h, idx, query, iters > 0 && out_avg_us, row_mask != nullptr);
  if (rc) return rc;
  Shard *s = h.s;
  Ctx *c = h.c;
  hipStream_t st = h.st;
  // A search's mask resolution, route (choose_route) and first-pass kernel (launch_route_scan), for k = 100 and its
  // default block -- EXCEPT the int8 route, which the hook never takes: where a search would scan the int8 copy, the hook
  // times the fp16 or f32 tile scan such a search falls back to (a denial, a full device).  Under TSH_OPT_SCAN_I8 = 2 that
  // is a tile scan even of a shard small enough for the exact path, which no search of it runs.  No denial is read or
  // used up, no route counter touched.
  const int32_t k = 100, entries = tsh_default_block_entries(k);
  std::vector<uint64_t> words;
  std::vector<uint32_t> list_ids;
  const ShardMask m = resolve_mask(s, MaskSrc(row_mask), k, entries, &words, &list_ids);
  const bool masked = m.words != nullptr || !s->all_live;
  const int32_t n_tiles = (int32_t)((s->rows + 63) / 64);
  if (m.words) {
    memcpy(c->h_mask, m.words, (size_t)n_tiles * 8);
    HIPCHK(hipMemcpyAsync(c->d_mask, c->h_mask, (size_t)n_tiles * 8, hipMemcpyHostToDevice, st));
    c->mask_epoch = 0;
  }
  const Route r = choose_route(s, m, masked, k, entries, c->h_query, false);
  if (r.use_list) {
    if ((rc = ctx_reserve_list(c, m.list.padded))) return rc;
    memcpy(c->h_list, m.list.ids, (size_t)m.list.padded * sizeof(uint32_t));
    c->list_epoch = 0;
    HIPCHK(hipMemcpyAsync(c->d_list, c->h_list, (size_t)m.list.padded * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  const uint32_t *d_list = r.use_list ? c->d_list : nullptr;
  static thread_local ScanArgsQ sa;
  static thread_local ExactArgsQ xa;
  RowStore store = RowStore::F32;
  if (r.exact) {  // (no wave minima: the scan alone is timed, nothing picks behind it)
    if ((rc = ctx_reserve_exact(c, r.n_exam))) return rc;
    fill_exact_args(s, c, m.words && !r.use_list ? c->d_mask : nullptr, d_list, r.n_exam, c->h_query, &xa);
  } else {
    fill_scan_args(s, c, m.words ? c->d_mask : nullptr, d_list, m.list.padded, &sa);
    if (r.f16_eligible && r.fb.ok && rows16_ensure(s, st, r.v_exp)) {
      store = RowStore::F16;
      fill_scan_f16_args(s, r.fb, &sa, nullptr);
    }
  }
  auto launch = [&]() { launch_route_scan(s, r, store, masked, m.rows_est, sa, xa, st, LaunchEv()); };
  launch();  // warm
  HIPCHK(hipEventRecord(c->ev0, st));
  for (int32_t i = 0; i < iters; ++i) launch();
  HIPCHK(hipEventRecord(c->ev1, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *out_avg_us = (double)ms * 1000.0 / iters;
  return TSH_OK;
}

int32_t tsh_index_set_option(tsh_index *idx, int32_t option, int64_t value) {
  if (option == TSH_OPT_EXCHANGE_AHEAD) {  // process-wide (idx is ignored)
    if (value != 0 && value != 1) return set_err(TSH_E_BAD_ARG, "exchange ahead: 0 or 1");
    exchange_ahead_flag().store(value != 0, std::memory_order_release);
    return TSH_OK;
  }
  if (option == TSH_OPT_TEST_HOOKS) {  // process-wide (idx is ignored): see test_env, tsh_host_sync.h
    if (value != 0 && value != TSH_TEST_HOOKS_MAGIC) return set_err(TSH_E_BAD_ARG, "test hooks: wrong magic");
    test_hooks_flag().store(value != 0, std::memory_order_release);
    return TSH_OK;
  }
  if (!idx) return set_err(TSH_E_BAD_ARG, "index is NULL");
  if (option == TSH_OPT_BATCH_MIN_NQ) {
    if (value < 0 || value > (1 << 20)) return set_err(TSH_E_BAD_ARG, "batch_min_nq out of range");
    idx->batch_min_nq = (int32_t)value;
    return TSH_OK;
  }
  // the per-shard options: id, lowest and highest value, what a value outside is told (%d: the highest), the store
  struct ShardOption {
    int32_t id;
    int64_t lo, hi;
    const char *msg;
    void (*set)(Shard *, int64_t);
  };
  static const ShardOption options[] = {
      {TSH_OPT_EXACT_SCAN_ROWS, 0, EX_MAX_ROWS, "exact scan rows: 0 .. %d", [](Shard *sh, int64_t v) { sh->exact_rows = (int)v; }},
      {TSH_OPT_BATCH_GROUP, 0, 1, "batch group: 0 or 1", [](Shard *sh, int64_t v) { sh->batch_group = v != 0; }},
      {TSH_OPT_BATCH_HUB, 0, 1, "batch hub: 0 or 1", [](Shard *sh, int64_t v) { sh->batch_hub = v != 0; }},
      {TSH_OPT_EXACT_SELECT, 0, 1, "exact select: 0 (one workgroup ranks k rows) or 1 (wide pick)",
       [](Shard *sh, int64_t v) { sh->exact_pick = v != 0; }},
      {TSH_OPT_SCAN_F16, 0, 2, "scan f16 must be 0 (never), 1 (auto: shards above 256 MiB) or 2 (every eligible dense scan)",
       [](Shard *sh, int64_t v) { sh->rows16.mode = (int)v; }},
      {TSH_OPT_SCAN_F16_MASKED, 0, 2, "scan f16 masked must be 0 (never), 1 (auto: shards above 256 MiB) or 2 (every eligible masked scan)",
       [](Shard *sh, int64_t v) { sh->rows16.mode_masked = (int)v; }},
      {TSH_OPT_SCAN_I8, 0, 2, "scan i8 must be 0 (never), 1 (auto: shards above 256 MiB) or 2 (every eligible scan)",
       [](Shard *sh, int64_t v) { sh->rows8.mode = (int)v; }},
      {TSH_OPT_SCAN_I8_MASKED, 0, 2, "scan i8 masked must be 0 (never), 1 (auto: shards above 256 MiB) or 2 (every eligible masked scan)",
       [](Shard *sh, int64_t v) { sh->rows8.mode_masked = (int)v; }},
      {TSH_OPT_SCAN_I4, 0, 2, "scan i4 must be 0 (never), 1 (auto: L2 shards above 256 MiB) or 2 (every eligible scan)",
       [](Shard *sh, int64_t v) { sh->rows4.mode = (int)v; }},
      {TSH_OPT_SCAN_STREAMS, 0, 2, "scan streams must be 0 (by the scan's drain share), 1 (one stream) or 2 (two whenever queries overlap)",
       [](Shard *sh, int64_t v) { sh->scan_streams = (int)v; }},
      {TSH_OPT_BATCH_KERNEL, 0, 3, "batch kernel must be 0 (f32 MFMA), 1 (bf16x3), 2 (f16) or 3 (auto)",
       [](Shard *sh, int64_t v) { sh->batch_kernel = (int)v; }},
  };
  for (const ShardOption &o : options) {
    if (o.id != option) continue;
    if (value < o.lo || value > o.hi) return set_err(TSH_E_BAD_ARG, o.msg, (int)o.hi);
    for (auto &sh : idx->shards) {
      std::unique_lock<RwLock> xl(sh->mu);
      o.set(sh.get(), value);
    }
    return TSH_OK;
  }
  return set_err(TSH_E_BAD_ARG, "unknown option %d", option);
}

int32_t tsh_bench_batch(tsh_index *idx, const float *queries, int32_t nq, int32_t k, int32_t iters,
                        double *out_avg_gemm_us, double *out_flops) {
  if (!idx || idx->shards.size() != 1 || !queries || nq <= 0 || k <= 0 || iters <= 0 || !out_avg_gemm_us)
    return set_err(TSH_E_BAD_ARG, "bad arguments");
  Shard *s = idx->shards[0].get();
  std::shared_lock<RwLock> sl = share(idx, s);
  if (s->rows == 0) return set_err(TSH_E_BAD_ARG, "empty index");
  if (s->safe_mode()) return set_err(TSH_E_BAD_ARG, "index is in safe mode: no batched path");
  int32_t entries = tsh_default_block_entries(k);
  std::vector<uint8_t> blocks((size_t)tsh_candidate_block_bytes(entries) * (size_t)nq);
  double acc = 0;
  for (int32_t i = 0; i < iters; ++i) {
    SearchOut so;
    so.h_blocks = blocks.data();
    // (the call tsh_search makes: results finalised on the device, lists as wide as that kernel takes -- with the
    // caller's 256-entry blocks an L2 corpus with varying norms overflowed here, and only here, and the overflows
    // talked the automatic kernel choice out of fp16 in the middle of a measurement)
    so.on_final = [](int32_t, int32_t, const char *, const int64_t *, const double *, const int32_t *) {};
    std::vector<int32_t> redo;
    s->batch->timed = true;  // (read under its mutex by the call below; measurement hooks are not run concurrently)
    int rc = shard_search_batch(s, s->batch, queries, nq, k, nullptr, entries, &so, &redo);
    s->batch->timed = false;
    if (rc) return rc;
    acc += s->batch->last_gemm_us;
  }
  *out_avg_gemm_us = acc / iters;
  if (out_flops) *out_flops = s->batch->last_flops;
  return TSH_OK;
}

// ---- probes of the pre-filter keys (tests/test_gpu_bands.py): what the kernels actually computed, next to the
// error bound the host claimed for it
int32_t tsh_probe_scan_keys(tsh_index *idx, const float *query, float *out_keys, float *out_eps_rel, float *out_delta_abs) {
  ScanHook h;
  int rc = scan_hook_begin(&h, idx, query, out_keys && out_eps_rel && out_delta_abs);
  if (rc) return rc;
  Shard *s = h.s;
  const Band band = compute_band(s, h.c->h_query);
  if (band.force_all) return set_err(TSH_E_BAD_ARG, "the query / index is outside the error model (no band)");
  static thread_local ScanArgsQ sa;
  fill_scan_args(s, h.c, nullptr, nullptr, 0, &sa);
  launch_scan(sa, s->nch, s->metric, /*masked*/ !s->all_live, h.st);
  if ((rc = scan_hook_keys(h, out_keys))) return rc;
  *out_eps_rel = band.eps_rel;
  *out_delta_abs = band.delta_abs;
  return TSH_OK;
}

// scans, queries redone through the f32 scan, rows converted, bytes of the copy: of one of the two copies, over the shards
int32_t row_copy_stats(tsh_index *idx, RowStore store, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  out[0] = out[1] = out[2] = out[3] = 0;
  for (auto &sp : idx->shards) {
    Shard *s = sp.get();
    std::shared_lock<RwLock> sl = share(idx, s);
    const RowCopy &c = *s->row_copy(store);
    out[0] += c.route.scans.load();
    out[1] += c.route.redone.load();
    out[2] += c.converted.load();
    std::lock_guard<std::mutex> lk(s->row_copies_mu);
    out[3] += c.bytes;
  }
  return TSH_OK;
}
int32_t tsh_scan_f16_stats(tsh_index *idx, int64_t *out) { return row_copy_stats(idx, RowStore::F16, out); }
int32_t tsh_scan_i8_stats(tsh_index *idx, int64_t *out) { return row_copy_stats(idx, RowStore::I8, out); }

// scans whose 4-bit pass ran, rows those passes left to the int8 scan, rows converted, bytes of the plane, times the route
// was denied, eligible scans a denial still covers: over the shards
int32_t tsh_scan_i4_stats(tsh_index *idx, int64_t *out) {
  if (!idx || !out) return set_err(TSH_E_BAD_ARG, "NULL pointer");
  for (int i = 0; i < 6; ++i) out[i] = 0;
  for (auto &sp : idx->shards) {
    Shard *s = sp.get();
    std::shared_lock<RwLock> sl = share(idx, s);
    const RowCopyI4 &c = s->rows4;
    out[0] += c.route.scans.load();
    out[1] += c.survivors.load();
    out[2] += c.converted.load();
    out[4] += c.denials.load();
    out[5] += std::max(0, c.route.denied.load());
    std::lock_guard<std::mutex> lk(s->row_copies_mu);
    out[3] += c.bytes;
  }
  return TSH_OK;
}

int32_t tsh_probe_scan_i4_keys(tsh_index *idx, const float *query, float *out_lower, float *out_upper) {
  ScanHook h;
  int rc = scan_hook_begin(&h, idx, query, out_lower && out_upper);
  if (rc) return rc;
  Shard *s = h.s;
  Ctx *c = h.c;
  hipStream_t st = h.st;
  const bool masked = !s->all_live || !s->quar_ids.empty();
  if (!scan_i8_applies(s, masked, 1, 1) || !scan_i4_applies(s, masked) || compute_band(s, c->h_query).force_all)
    return set_err(TSH_E_BAD_ARG, "no 4-bit scan for this index / query (TSH_OPT_SCAN_I8, TSH_OPT_SCAN_I4, metric, dead rows, row width, error model)");
  const ScanI4Band b = scan_i4_band(s->dim, scan_i4_groups(s->ld), c->h_query, s->max_norm, s->max_abs);
  if (!b.ok) return set_err(TSH_E_BAD_ARG, "the query is outside the 4-bit scan's error model");
  if (!rows8_ensure(s, st) || !rows4_ensure(s, st)) return set_err(TSH_E_OOM, "no room on the device for the 4-bit copy of the rows");
  if ((rc = ctx_reserve_i4(c, s->cap / 64))) return rc;
  static thread_local ScanI4ArgsQ sa;
  fill_scan_i4_args(s, c, b, c->h_query, &sa);
  // (the hook's helpers read the context's keys buffer: A writes there)
  sa.a.keys = c->d_keys;
  scan_i4_kernel<4><<<(unsigned)((sa.a.n_tiles + 3) / 4), 256, 0, st>>>(sa);
  if ((rc = scan_hook_keys(h, out_lower))) return rc;
  std::vector<float> w((size_t)s->rows);
  float *d_w = reinterpret_cast<float *>(c->d_keys);
  scan_i4_w_kernel<<<(unsigned)((s->rows + 255) / 256), 256, 0, st>>>(sa.a, d_w);
  HIPCHK(hipMemcpyAsync(w.data(), d_w, (size_t)s->rows * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  for (int64_t i = 0; i < s->rows; ++i) out_upper[i] = out_lower[i] + 2.0f * w[(size_t)i];
  return TSH_OK;
}

int32_t tsh_probe_scan_i8_keys(tsh_index *idx, const float *query, float *out_lower, float *out_upper) {
  ScanHook h;
  int rc = scan_hook_begin(&h, idx, query, out_lower && out_upper);
  if (rc) return rc;
  Shard *s = h.s;
  Ctx *c = h.c;
  hipStream_t st = h.st;
  const bool masked = !s->all_live || !s->quar_ids.empty();  // (dead rows: the keys of TSH_OPT_SCAN_I8_MASKED's route, NaN where a row is not live)
  if (!scan_i8_applies(s, masked, 1, 1) || compute_band(s, c->h_query).force_all)
    return set_err(TSH_E_BAD_ARG, "no int8 scan for this index / query (TSH_OPT_SCAN_I8, dead rows, row width, error model)");
  const ScanI8Band ib = scan_i8_band(s->metric, s->dim, s->nch, c->h_query, s->max_norm, s->min_norm, s->max_abs);
  if (!ib.ok) return set_err(TSH_E_BAD_ARG, "the query is outside the int8 scan's error model");
  if (!rows8_ensure(s, st)) return set_err(TSH_E_OOM, "no room on the device for the int8 copy of the rows");
  static thread_local ScanArgsQ sa;
  fill_scan_args(s, c, nullptr, nullptr, 0, &sa);
  fill_scan_i8_args(s, ib, &sa);
  // (a dead tile's keys stay as they were: the probe reads them all, so they start out dead)
  if (masked) HIPCHK(hipMemsetAsync(c->d_keys, 0xFF, (size_t)((s->rows + 63) / 64) * 64 * 4, st));
  launch_scan_i8(sa, s->nch, s->metric, masked, st);
  if ((rc = scan_hook_keys(h, out_lower))) return rc;
  // (the rows' bands, by the arithmetic the kernel forms them with -- into the keys buffer, free again once copied)
  std::vector<float> w((size_t)s->rows);
  float *d_w = reinterpret_cast<float *>(c->d_keys);
  scan_i8_w_kernel<<<(unsigned)((s->rows + 255) / 256), 256, 0, st>>>(s->d_sqnorm, s->metric == TSH_METRIC_COSINE ? s->d_inv_norm : nullptr,
                                                                     sa.a.scale8, s->rows, ib.a_s, ib.a_v, ib.beta, d_w);
  HIPCHK(hipMemcpyAsync(w.data(), d_w, (size_t)s->rows * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  // the upper side as the kernel forms it: (lower + w) + w would round twice -- the key itself is lower + w up to one
  // rounding, which the band's own slack (1.001) covers on either side
  for (int64_t i = 0; i < s->rows; ++i) out_upper[i] = out_lower[i] + 2.0f * w[(size_t)i];
  return TSH_OK;
}

int32_t tsh_probe_scan_f16_keys(tsh_index *idx, const float *query, float *out_keys, float *out_w) {
  ScanHook h;
  int rc = scan_hook_begin(&h, idx, query, out_keys && out_w);
  if (rc) return rc;
  Shard *s = h.s;
  Ctx *c = h.c;
  hipStream_t st = h.st;
  int v_exp = 0;
  const bool masked = !s->all_live;  // (dead rows: the keys of TSH_OPT_SCAN_F16_MASKED's route, NaN where a row is not live)
  if (!scan_f16_applies(s, masked, &v_exp) || compute_band(s, c->h_query).force_all)
    return set_err(TSH_E_BAD_ARG, "no fp16 scan for this index / query (TSH_OPT_SCAN_F16, TSH_OPT_SCAN_F16_MASKED, row width, error model)");
  const ScanF16Band fb = scan_f16_band(s->metric, s->dim, s->nch, c->h_query, s->max_norm, s->min_norm, v_exp);
  if (!fb.ok) return set_err(TSH_E_BAD_ARG, "the query is outside the fp16 scan's error model");
  if (!rows16_ensure(s, st, v_exp)) return set_err(TSH_E_OOM, "no room on the device for the fp16 copy of the rows");
  static thread_local ScanArgsQ sa;
  fill_scan_args(s, c, nullptr, nullptr, 0, &sa);
  fill_scan_f16_args(s, fb, &sa, nullptr);
  // (a dead tile's keys stay as they were: the probe reads them all, so they start out dead)
  if (masked) HIPCHK(hipMemsetAsync(c->d_keys, 0xFF, (size_t)((s->rows + 63) / 64) * 64 * 4, st));
  launch_scan_f16(sa, s->nch, s->metric, masked, st);
  if ((rc = scan_hook_keys(h, out_keys))) return rc;
  // (the rows' bands, by the function the kernel adds them with -- into the keys buffer, free again once copied)
  float *d_w = reinterpret_cast<float *>(c->d_keys);
  scan_f16_w_kernel<<<(unsigned)((s->rows + 255) / 256), 256, 0, st>>>(s->metric == TSH_METRIC_COSINE ? nullptr : s->d_sqnorm, s->rows,
                                                                      fb.alpha, fb.beta, d_w);
  HIPCHK(hipMemcpyAsync(out_w, d_w, (size_t)s->rows * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return TSH_OK;
}

int32_t tsh_probe_batch_keys(tsh_index *idx, const float *queries, int32_t nq, int32_t k, float *out_keys, float *out_delta2) {
  if (!idx || idx->shards.size() != 1 || !queries || nq <= 0 || k <= 0 || !out_keys || !out_delta2)
    return set_err(TSH_E_BAD_ARG, "bad arguments");
  Shard *s = idx->shards[0].get();
  std::shared_lock<RwLock> sl = share(idx, s);
  if (s->rows == 0 || s->safe_mode()) return set_err(TSH_E_BAD_ARG, "empty index, or safe mode: no batched path");
  if ((int64_t)nq * s->rows > (1ll << 28)) return set_err(TSH_E_BAD_ARG, "nq x rows too large for a dense key matrix");
  const int32_t entries = tsh_default_block_entries(k);
  std::vector<uint8_t> blocks((size_t)tsh_candidate_block_bytes(entries) * (size_t)nq);
  SearchOut so;
  so.h_blocks = blocks.data();
  std::vector<int32_t> redo;
  BatchCtx *b = s->batch;
  b->last_sample_force = 1;  // (read under b->mu by the call below; probes are not run concurrently)
  int rc = shard_search_batch(s, b, queries, nq, k, nullptr, entries, &so, &redo);
  b->last_sample_force = 0;
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(b->mu);
  if (b->last_sample != s->rows || b->last_nq != nq) return set_err(TSH_E_BUSY, "another batched call ran in between");
  HIPCHK(hipSetDevice(s->device));
  HIPCHK(hipMemcpy2D(out_keys, (size_t)s->rows * 4, b->dense.d, (size_t)b->last_sample * 4, (size_t)s->rows * 4, (size_t)nq,
                     hipMemcpyDeviceToHost));
  if (s->split_grouped && s->batch_kernel_last.load() == 2) {  // a norm-grouped plane: the keys came out by plane position
    std::vector<uint32_t> perm((size_t)s->rows);
    HIPCHK(hipMemcpy(perm.data(), s->d_perm, (size_t)s->rows * 4, hipMemcpyDeviceToHost));
    std::vector<float> byrow((size_t)s->rows);
    for (int32_t q = 0; q < nq; ++q) {
      float *kq = out_keys + (size_t)q * (size_t)s->rows;
      for (int64_t p2 = 0; p2 < s->rows; ++p2) byrow[perm[(size_t)p2]] = kq[p2];
      memcpy(kq, byrow.data(), (size_t)s->rows * 4);
    }
  }
  // one bound for every row of the query: the shared part + the per-row part at the longest row
  const QAux aux{b->qaux.h, (size_t)b->last_nq_pad};
  const float *d2 = aux.delta2(), *al = aux.alpha();
  for (int32_t q = 0; q < nq; ++q) {
    const double v = (double)d2[q] + 2.0 * (double)al[q] * (double)s->max_norm * (1.0 + 1e-6);
    out_delta2[q] = (float)v;
    if ((double)out_delta2[q] < v) out_delta2[q] = std::nextafter(out_delta2[q], INFINITY);
  }
  return TSH_OK;
}

int32_t tsh_probe_batch_row_band(tsh_index *idx, int32_t nq, float *out_alpha2, float *out_beta2) {
  if (!idx || idx->shards.size() != 1 || nq <= 0 || !out_alpha2 || !out_beta2) return set_err(TSH_E_BAD_ARG, "bad arguments");
  Shard *s = idx->shards[0].get();
  std::shared_lock<RwLock> sl = share(idx, s);
  BatchCtx *b = s->batch;
  std::lock_guard<std::mutex> lk(b->mu);
  if (b->last_nq != nq || !b->qaux.h) return set_err(TSH_E_BUSY, "no batched call of that many queries to report on");
  const QAux aux{b->qaux.h, (size_t)b->last_nq_pad};
  const float *d2 = aux.delta2(), *al = aux.alpha();
  for (int32_t q = 0; q < nq; ++q) {
    out_alpha2[q] = 2.f * al[q];
    out_beta2[q] = d2[q];
  }
  return TSH_OK;
}

}  // extern "C"

#include "tsh_host_coldstart.inl.h"  // raw-vector file loader, tsh_index_open_ngh
#include "tsh_host_pq.inl.h"         // tsh_pq_train, tsh_index_pq_encode
#include "tsh_host_comm.inl.h"       // tsh_comm_*, tsh_search_sharded (RCCL)
