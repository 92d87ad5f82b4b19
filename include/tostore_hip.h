/*
 * tostore_hip.h -- C-ABI of libtostore_hip.so: MI355X (gfx950) exhaustive kNN
 * behind ToStore's vectorSearch().
 *
 * The reference (tocreator/tostore v3.2.0, pure Dart) has no plugin/FFI hook
 * for vector search; the seam this library plugs into is the single call
 *   NghGraphEngine.search(...)   lib/src/core/ngh_graph_engine.dart:67-135
 * made from VectorIndexManager.vectorSearch
 *                                lib/src/core/vector_index_manager.dart:538-548
 * plus the data-feed seams listed per function below.  Conventions mirror the
 * reference's only existing FFI (lib/src/handler/system_ffi_helper.dart:21-55,
 * 219-262): int32 status returns with 0 = success, caller-allocated
 * out-params, no callbacks, every failure recoverable by falling back to the
 * Dart path.  The `dart:ffi` binding a maintainer would add is in
 * INTEGRATION.md and tostore_amd/dart/tostore_hip_bridge.dart.
 *
 * Ownership: the library owns only tsh_index handles and device memory.
 * Every host pointer is caller-allocated and caller-freed; inputs are fully
 * consumed before the call returns; no pointer is retained.
 * Threading: every entry point is thread-safe; searches on one handle may
 * run concurrently, append/delete/load take the handle exclusively.
 * Errors: <0 = error class below; text via tsh_last_error (thread-local).
 * The library never aborts, throws across the boundary, or falls back to a
 * CPU implementation: without a usable GPU every compute entry returns
 * TSH_E_NO_DEVICE.
 */
#ifndef TOSTORE_HIP_H
#define TOSTORE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: tsh_counters grew (fused_launches) and tsh_ngh_info grew (pages_absent, files_absent) after version 1 shipped; a
 * host built against the version-1 structs would be written past its buffers, so the number changed with them.
 * tsh_comm_create_host / tsh_comm_set_group and TSH_E_PEER came with version 2 as well. */
#define TSH_ABI_VERSION 5
/* 3: tsh_counters grew again (batch_plane_fallbacks, batch_scan_fallbacks); tsh_comm_get_timeline / tsh_comm_timeline
 * came with it.
 * 4: tsh_search_shard_begin / _progress / _end (the progressive shard search tsh_search_sharded is now built on);
 *    tsh_counters.list_scans, tsh_counters.exact_scans (the reserved slot of version 2), tsh_comm_timeline.pre_enqueue_us;
 *    TSH_OPT_EXCHANGE_AHEAD, TSH_OPT_EXACT_SCAN_ROWS, TSH_OPT_TEST_HOOKS.
 * 5: mask handles (tsh_mask_create / _destroy / _kept, tsh_search_masked, tsh_search_submit_masked): a WHERE row set
 *    that lives on the device across queries; tsh_index_open_ngh_shard (a rank cold-starts its own row range);
 *    tsh_ngh_info grew (row_base, row_end); tsh_comm_timeline's sampled fields are scaled by exchanges / timed
 *    exchanges instead of a constant.
 *    Additive since, same version: TSH_OPT_SCAN_F16, tsh_scan_f16_stats, tsh_probe_scan_f16_keys;
 *    TSH_OPT_SCAN_F16_MASKED; TSH_OPT_SCAN_I8, tsh_scan_i8_stats, tsh_probe_scan_i8_keys; TSH_OPT_SCAN_STREAMS;
 *    TSH_OPT_SCAN_I8_MASKED; TSH_OPT_SCAN_I4, tsh_scan_i4_stats, tsh_probe_scan_i4_keys; tsh_search_after, tsh_search_submit_after, tsh_search_after_stats;
 *    tsh_search_shard_after, tsh_search_shard_begin_after, tsh_merge_candidates_after, tsh_search_sharded_after;
 *    tsh_search_shard_masked, tsh_search_shard_begin_masked, tsh_search_sharded_masked;
 *    tsh_search_count, tsh_search_count_stats;
 *    tsh_groups_create, tsh_groups_set, tsh_groups_destroy, tsh_search_grouped, tsh_search_grouped_stats. */
/*    Additive since, same version, continued: tsh_search_grouped_after, tsh_search_grouped_count,
 *    tsh_search_grouped_after_stats. */
/*    Additive since, same version, continued: tsh_search_grouped_rows, tsh_search_grouped_rows_stats. */
/*    Additive since, same version, continued: tsh_attr_create, tsh_attr_set, tsh_attr_destroy, tsh_mask_create_range,
 *    tsh_mask_read. */
/*    Additive since, same version, continued: tsh_mask_create_where (tsh_where_term, TSH_TERM_*, TSH_WHERE_MAX_*). */
/*    Additive since, same version, continued: tsh_tags_create, tsh_tags_set, tsh_tags_destroy, tsh_mask_create_tags
 *    (TSH_TAGS_ALL, TSH_TAGS_ANY, TSH_TAGS_MAX_SET_VALUES). */
/*    Additive since, same version, continued: tsh_attr_facets, tsh_tags_facets
 *    (TSH_FACET_VALUES, TSH_FACET_EDGES, TSH_FACET_MAX_KEYS). */

/* status codes */
#define TSH_OK 0
#define TSH_E_BAD_ARG (-1)
#define TSH_E_DIM_MISMATCH (-2)
#define TSH_E_OOM (-3)
#define TSH_E_HIP (-4)
#define TSH_E_NO_DEVICE (-5)
#define TSH_E_OVERFLOW (-6) /* a candidate block was too small; retry with more entries */
#define TSH_E_IO (-7)
#define TSH_E_FORMAT (-8)
#define TSH_E_BUSY (-9) /* tsh_search_submit: tsh_max_inflight() asynchronous searches are already un-waited on the
                           handle, or an append / delete is waiting for the open ones: wait for them, then submit again */
#define TSH_E_RCCL (-10) /* librccl could not be loaded, or a collective failed */
#define TSH_E_PEER (-11) /* tsh_search_sharded: another rank of the collective failed (its own call returned the real
                            error); nothing was written on this rank.  The communicator stays usable. */

/* metric = enum order of VectorDistanceMetric, lib/src/model/table_schema.dart:2511-2531 */
#define TSH_METRIC_L2 0
#define TSH_METRIC_IP 1
#define TSH_METRIC_COSINE 2

typedef struct tsh_index tsh_index;

/* counters: replaces nothing in the reference (it has no tracing on this
 * path); feeds Logger-style diagnostics on the Dart side */
typedef struct tsh_counters {
  int64_t rows;              /* rows ever appended (= next row id) */
  int64_t deleted_rows;      /* tombstoned rows */
  int64_t searches;          /* queries answered */
  int64_t scan_launches;     /* single-query scan kernels launched */
  int64_t batch_launches;    /* batched (MFMA) passes launched */
  int64_t fallback_searches; /* queries that took the wide-band fallback */
  int64_t candidates_total;  /* rows re-ranked in f64 */
  int64_t bytes_resident;    /* device bytes held by this handle */
  int32_t safe_mode;         /* !=0: more than 1024 rows of one shard hold values outside the f32 error model
                                (see quarantined_rows); every search re-ranks all rows in f64 (exact, slow) */
  int32_t device_id;
  /* scan-kernel device time sampled with HIP events on the stream the kernel runs
   * on, inside real searches (every 4th query): sum of microseconds / samples.  The launch's own
   * duration: where consecutive scans alternate between two streams (TSH_OPT_SCAN_STREAMS) a scan runs
   * beside its neighbour and this is about twice its share of the HBM time */
  double scan_us_sum;
  int64_t scan_us_samples;
  int32_t batch_kernel_last; /* TSH_OPT_BATCH_KERNEL variant the last batched search ran (0/1/2; -1 none yet) */
  int32_t quarantined_rows;  /* live rows outside the f32 error model (non-finite or > 1e15 elements; cosine: norm
                                below 2^-50) that are kept out of the scan and re-ranked exactly on every search */
  int64_t exact_scans;       /* of scan_launches: searches with at most TSH_OPT_EXACT_SCAN_ROWS rows to look at (a
                                selective mask's list, a small index or shard), answered by the exact f64 sums of all of
                                them and a select among the exact distances -- two dispatches, no f32 keys, no band.
                                (The slot was "fused_launches", reserved and 0, before ABI 4.) */
  /* A batched call whose device allocations fail degrades instead of failing (results are identical on every path): */
  int64_t batch_plane_fallbacks; /* calls that could not allocate the fp16 / bf16x3 copy of the rows and scored
                                    their queries with the f32 MFMA kernel on the rows as stored (no copy needed) */
  int64_t batch_scan_fallbacks;  /* calls whose batch scratch could not be allocated either and that were answered by
                                    pipelined single-query scans */
  int64_t list_scans;            /* of scan_launches: scans of a selective row mask as a compacted list of row ids
                                    (scan_list_kernel) instead of a walk over the tiles */
  int64_t exact_redone;          /* of exact_scans: searches whose wide pick (TSH_OPT_EXACT_SELECT) met a cut bin too full
                                    for its block -- ties by the hundred, a k-th neighbour outside the key histogram's
                                    window -- and were finished by the one-workgroup select on the same keys (ABI 5) */
} tsh_counters;

int32_t tsh_abi_version(void);
/* number of usable HIP devices; 0 when none (never an error) */
int32_t tsh_device_count(void);
/* copies the calling thread's last error text (NUL-terminated, truncated to
 * len); returns the untruncated length */
int32_t tsh_last_error(char *buf, int32_t len);

/* Create an empty device index on the calling thread's current HIP device
 * (n_devices == 1) or row-range sharded over devices 0..n_devices-1.
 * Created lazily by the Dart side on the first vectorSearch / writeChanges of
 * an index (the reference loads nothing vector-related at open:
 * lib/src/core/data_store_impl.dart:822-846, vector_index_manager.dart:39-43).
 * dim/metric come from NghIndexMeta (lib/src/model/ngh_index_meta.dart:82-100).
 * 1 <= dim <= 4096 (a 16 KiB raw-vector page holds float32 vectors up to
 * dim 4073, lib/src/core/ngh_page.dart:575-579). */
int32_t tsh_index_create(int32_t dim, int32_t metric, int64_t capacity_rows,
                         int32_t n_devices, tsh_index **out);

/* One shard of a row-range partitioned corpus, for one-process-per-GPU
 * deployments: holds global rows [row_base, row_base + size) on device
 * `device_id` (-1 = current).  Ids reported by this handle are global. */
int32_t tsh_index_create_shard(int32_t dim, int32_t metric, int64_t capacity_rows,
                               int32_t device_id, int64_t row_base, tsh_index **out);

/* Replaces cache teardown: VectorIndexManager.clearCacheForTable/Index, dispose
 * (vector_index_manager.dart:1192-1216); also required after reorderByLocality
 * renumbers node ids (:932-1159). */
int32_t tsh_index_destroy(tsh_index *idx);

/* Append (or overwrite) rows [first_row_id, first_row_id + n_rows); `rows` is
 * row-major n_rows x dim float32, already converted exactly as the reference
 * stores them (f64 -> f32, truncate / zero-pad: core/compute/
 * vector_batch_prepare_compute.dart:79-86).  Mirrors NghGraphEngine.
 * _writeRawVector / insertBatch (ngh_graph_engine.dart:691-720, :297-403):
 * node ids are dense and monotonically assigned (:321).  Ids skipped by a gap
 * are treated as absent rows (never returned), like a missing raw-vector page
 * (ngh_graph_engine.dart:124-125).  Shard handles take GLOBAL ids. */
int32_t tsh_index_append(tsh_index *idx, int64_t first_row_id, int64_t n_rows,
                         const float *rows);
/* Same, from a device pointer on the handle's device (bulk loaders that
 * already hold the column in HBM).  The copy runs on a library stream: the
 * caller must have synchronised whatever produced d_rows before the call. */
int32_t tsh_index_append_device(tsh_index *idx, int64_t first_row_id, int64_t n_rows,
                                const void *d_rows);

/* Tombstones: mirrors NghGraphEngine.deleteBatch (ngh_graph_engine.dart:411-445),
 * which sets NghNodeFlags.deleted (ngh_page.dart:105-108) and leaves the raw
 * vector bytes in place.  Unlike the reference's beam search (which can leak
 * deleted rows from other pages, :230-232) deleted rows are never returned.
 * Unknown ids are ignored. */
int32_t tsh_index_set_deleted(tsh_index *idx, const int64_t *ids, int64_t n);

/* Cold load of one raw-vector partition file
 * <index>/ngh/rawvec/dir_N/pP.ngh (lib/src/core/path_manager.dart:318-324):
 * data pages 1..last of `page_size` bytes (page 0 is the partition meta page,
 * core/ngh_page.dart:29-98), each a 20-byte 'TPG2' header + CRC32
 * (core/btree_page.dart:132-234) + NghRawVectorPage payload
 * (core/ngh_page.dart:310-450; f64 / f32 / i8 elements converted to f32 exactly
 * as getVectorAsFloat32 does, :364-391).  `precision` is meta.json's
 * VectorPrecision index (0 f64, 1 f32, 2 i8) and fixes vectorsPerRawPage
 * (core/ngh_page.dart:575-579); data page p holds node ids
 * first_row_id + (p-1)*vectorsPerRawPage + slot (model/ngh_index_meta.dart:480-490).
 * Reader semantics follow readRawVectorPage (core/ngh_partition_manager.dart:239-295)
 * with ONE deliberate difference: where the reference makes up a page of zero
 * vectors (a page past the end of the file, :270-281) the ids stay ABSENT rows here --
 * the reference only meets such a slot if its graph walk reaches it, an exhaustive
 * scan would return those zero rows to every query.  A bad magic / type / CRC is an
 * error (the reference throws: core/btree_page.dart:215-233), and so is a page that
 * passes its CRC but does not decode as a raw-vector payload (ciphertext of an index
 * written with encryptVectorIndex): TSH_E_FORMAT, nothing appended from that page on.
 * Only ids < first_row_id + max_rows are loaded (meta.nextNodeId bounds them).
 * *out_rows = rows appended. */
int32_t tsh_index_load_rawvec_file(tsh_index *idx, const char *path, int32_t page_size,
                                   int32_t precision, int64_t first_row_id, int64_t max_rows,
                                   int64_t *out_rows);

/* What tsh_index_open_ngh found: the NghIndexMeta fields it used
 * (lib/src/model/ngh_index_meta.dart:359-408) and what it loaded. */
typedef struct tsh_ngh_info {
  int32_t dimensions;
  int32_t metric;    /* 0 l2, 1 innerProduct, 2 cosine */
  int32_t precision; /* 0 float64, 1 float32, 2 int8 (VectorPrecision order) */
  int32_t page_size;
  int32_t max_degree;
  int32_t reserved;
  int64_t next_node_id;
  int64_t total_vectors; /* meta.json's own count of live vectors */
  int64_t deleted_count; /* meta.json's own count of tombstones */
  int64_t max_partition_file_size;
  int64_t rows_loaded; /* node ids now resident */
  int64_t tombstones;  /* node ids whose graph slot carries NghNodeFlags.deleted */
  int64_t files_read;
  int64_t pages_absent; /* raw-vector pages below nextNodeId that are not on disk (file missing or shorter): their
                           node ids are ABSENT rows; a healthy index has 0 -- a caller may refuse the handle otherwise */
  int64_t files_absent; /* raw-vector partition files below nextNodeId that are missing altogether */
  int64_t row_base;     /* node ids [row_base, row_end) are what this handle was opened for: 0 and nextNodeId for */
  int64_t row_end;      /* tsh_index_open_ngh, the rank's range for tsh_index_open_ngh_shard (ABI 5) */
} tsh_ngh_info;

/* Cold start from an index directory written by the reference, without Dart
 * (SURVEY.md section 8f, N1): `<index>/ngh` as laid out by
 * lib/src/core/path_manager.dart:275-324.  Reads meta.json (jsonEncode of
 * NghIndexMeta.toJson, vector_index_manager.dart:623-634) for dimensions,
 * metric, precision, nextNodeId, page and partition-file sizes; creates the
 * handle; loads every raw-vector partition rawvec/dir_{p / max_entries_per_dir}/
 * p{p}.ngh with the addressing of ngh_index_meta.dart:480-490; then walks the
 * graph partitions and tombstones every node whose slot flags carry
 * NghNodeFlags.deleted (ngh_page.dart:105-108,198-213).  A missing graph file /
 * page reads as "no flags" exactly as in the reference; a missing raw-vector
 * file / page leaves its node ids ABSENT (never returned; counted in
 * info->pages_absent / files_absent -- see tsh_index_load_rawvec_file); a page
 * with a bad frame, type or CRC is TSH_E_FORMAT (the reference throws there,
 * btree_page.dart:215-233).  max_entries_per_dir <= 0 selects the reference
 * default of 500 (handler/common.dart:43).  Encrypted vector pages are not
 * supported (EncryptionConfig.encryptVectorIndex must be off): their payloads
 * pass the CRC but do not decode -> TSH_E_FORMAT.  info may be NULL. */
int32_t tsh_index_open_ngh(const char *ngh_dir, int32_t max_entries_per_dir, int32_t n_devices, tsh_index **out,
                           tsh_ngh_info *info);
/* Cold start of ONE row-range shard, for the one-process-per-GPU deployment tsh_search_sharded serves: rank `rank`
 * of `world` opens node ids [rank * per, min(nextNodeId, (rank + 1) * per)), per = ceil(nextNodeId / world), on
 * `device` (-1 = current) as a shard handle (tsh_index_create_shard: ids stay GLOBAL).  The addressing of
 * lib/src/model/ngh_index_meta.dart:480-490 makes that range a contiguous run of raw-vector partition files
 * (lib/src/core/path_manager.dart:275-324) and, inside the first and the last of them, of pages: only those files
 * are opened and only those pages read -- at BASELINE.json's C4 (10 M x 1536: 82 GB of pages) a rank of eight
 * reads its eighth.  A range that starts or ends inside a page takes that page's slots from / up to the boundary.
 * Tombstones come from the graph pages that hold the range's node ids (lib/src/core/ngh_page.dart:105-108,
 * 198-213), likewise only those.  Everything else -- meta.json, page checks, absent pages and files, errors -- is
 * tsh_index_open_ngh's; info (nullable) reports the census of THIS range (rows_loaded, tombstones, files_read,
 * pages_absent, files_absent) and the range itself (row_base, row_end).  W shards opened this way and merged
 * (tsh_merge_candidates / tsh_search_sharded) answer exactly what the whole-index handle answers. */
int32_t tsh_index_open_ngh_shard(const char *ngh_dir, int32_t max_entries_per_dir, int32_t device, int32_t world,
                                 int32_t rank, tsh_index **out, tsh_ngh_info *info);

/* Write-path helper: PQ-encode resident rows
 * [first_row_id, first_row_id + n_rows) against a trained codebook -- the
 * arithmetic of batchPqEncode (lib/src/core/compute_tasks.dart:2292-2326) ==
 * VectorQuantizer.encode (core/vector_quantizer.dart:357-368,461-483): per
 * sub-space the FIRST centroid with the smallest f64-accumulated squared
 * distance.  codebook: host, float32, layout centroids[(m*K + k)*subDim + d]
 * (vector_quantizer.dart:15), subDim = dim / subspaces; out_codes: host,
 * n_rows x subspaces bytes (one NghPqCodePage entry each, ngh_page.dart:232-300).
 * Codes are bit-exact with the reference. */
int32_t tsh_index_pq_encode(tsh_index *idx, int64_t first_row_id, int64_t n_rows, const float *codebook,
                            int32_t subspaces, int32_t centroids, uint8_t *out_codes);

/* Write-path helper (N4): train a PQ codebook the way the index manager's isolate
 * tasks do -- one trainPqSubspace per sub-space (lib/src/core/compute_tasks.dart:
 * 2135-2266, dispatched from core/vector_index_manager.dart:740-850 when >= 100
 * samples were collected; `iterations` is 10 there and centroids = min(256, n)).
 * samples: host, n x dim float32 (already _toFloat32'd, cosine rows normalised);
 * init_index: host, subspaces x centroids sample indices -- the values the
 * reference draws with Random(42 + subspaceIndex).nextInt(n), which stay on the
 * Dart side; out_codebook: host, layout centroids[(m*K + k)*subDim + d]
 * (vector_quantizer.dart:15).  Given the same init_index the codebook is
 * bit-identical to the reference's (mixed f32/f64 arithmetic restated, see
 * tsh_pq.hip.h).  Stateless: runs on `device`, needs no index handle. */
int32_t tsh_pq_train(int32_t device, const float *samples, int64_t n, int32_t dim, int32_t subspaces,
                     int32_t centroids, int32_t iterations, const int32_t *init_index, float *out_codebook);

int64_t tsh_index_size(tsh_index *idx); /* next row id (rows incl. tombstones) */
int32_t tsh_index_dim(tsh_index *idx);
int32_t tsh_index_metric(tsh_index *idx);

/* The drop-in for NghGraphEngine.search (ngh_graph_engine.dart:67-135) with
 * ef -> infinity: exact distances of EVERY live row, reference phase-3
 * semantics (:122-134): distance = sqrt(sum) for L2, -dot for IP,
 * 1 - cos for cosine, all in f64 accumulated left to right over f32 elements
 * (:908-946); rows with distance > distance_threshold dropped (NaN = none);
 * ascending by Dart double.compareTo, ties by row id; at most k per query.
 *   queries     nq x dim float32, prepared by the caller exactly as
 *               vector_index_manager.dart:514-520 does (_toFloat32, and
 *               _normalizeFloat32 for cosine)
 *   row_mask    nullable; ceil(size/8) bytes, bit i (LSB first) = 1 keeps row
 *               i (WHERE pre-filter; new capability).  Bytes read
 *               scale with the rows kept: a mask that keeps fewer than one row
 *               in 24 is compacted into a list of row ids once per call and
 *               scanned as a gather; a one-range mask (WHERE id BETWEEN ...)
 *               costs a batched call no more than a scattered one
 *   out_ids     nq x k      out_dist nq x k      out_count nq
 * nq == 1 (or small) streams the corpus once per query (HBM-bound kernel);
 * larger nq uses the batched matrix-core path, whose last steps (exact f64
 * re-rank, distance, threshold, order, cut) run on the device.  A device too
 * full for that path's buffers degrades the call (f32 matrix-core kernel on the
 * rows as stored, then pipelined scans: tsh_counters.batch_*_fallbacks) instead
 * of failing it.  Thread-safe;
 * two batched calls on one handle overlap (one prepares / copies out while the
 * GPU works on the other), further concurrent ones queue.  Empty index or
 * k <= 0 returns TSH_OK with counts 0 (the reference returns const []: :78). */
int32_t tsh_search(tsh_index *idx, const float *queries, int32_t nq, int32_t k,
                   double distance_threshold, const uint8_t *row_mask,
                   int64_t *out_ids, double *out_dist, int32_t *out_count);

/* ---- mask handles: a WHERE row set that lives on the device ------------------------------------------------------
 * tsh_search's row_mask pointer is consumed per call: the library slices the caller's bitmap, counts it and -- for a
 * selective one -- lists its rows, on the host, every time (three passes over 125 KB at 1 M rows: more than half of
 * a lone masked query's latency).  A row set that serves many queries -- the rows a WHERE clause keeps, mapped from
 * primary keys through the pk -> nodeId tree (lib/src/core/vector_index_manager.dart:1223-1378), or the complement
 * of a tombstone set (lib/src/core/ngh_page.dart:105-108) -- is made a HANDLE instead: the bitmap is uploaded once,
 * and when it is selective (few enough kept rows for the list scan or the exact path) compacted into the ascending
 * list of kept row ids ON THE DEVICE (popcount per 64-row word, a prefix over the words, one thread per word writing
 * its rows: the list never exists on the host).  Searches with the handle read both in place: no per-call copy, no
 * host pass.
 *   bits     GLOBAL keep bitmap, bit i (LSB first) = 1 keeps row id i, n_bytes bytes of it; rows at or beyond
 *            8 * n_bytes are NOT kept -- rows appended after the mask was made included (the handle re-slices its
 *            copy of the bitmap on the first search after an append; never the caller's memory again)
 *   rows tombstoned later are dropped as always (the kernels check the live bitmap), deleted rows never come back
 * A handle belongs to the index it was made for (any handle kind: whole index, several devices, a shard) and must be
 * destroyed before it; destroy it only after every ticket submitted with it has been waited for.  Thread-safe: any
 * number of searches may share one handle.  Results are identical to the pointer form's.
 * A handle that outlives its index is ORPHANED, not dangling: tsh_index_destroy frees the device parts of every handle
 * still made for it and detaches them; tsh_mask_kept then answers TSH_E_BAD_ARG, a search with it TSH_E_BAD_ARG (it
 * belongs to no index), and tsh_mask_destroy only frees the handle itself.  The two destroys may come in either order,
 * from any threads. */
typedef struct tsh_mask tsh_mask;
int32_t tsh_mask_create(tsh_index *idx, const uint8_t *bits, int64_t n_bytes, tsh_mask **out);
int32_t tsh_mask_destroy(tsh_mask *mask);
/* rows the mask keeps among the index's current row ids (tombstones not subtracted); < 0 = error */
int64_t tsh_mask_kept(tsh_mask *mask);
/* tsh_search / tsh_search_submit with the row set of a handle (mask may be NULL: no filter) */
int32_t tsh_search_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double distance_threshold,
                          tsh_mask *mask, int64_t *out_ids, double *out_dist, int32_t *out_count);
int32_t tsh_search_submit_masked(tsh_index *idx, const float *query, int32_t k, tsh_mask *mask, int32_t *out_ticket);

/* ---- attribute columns: a WHERE range made into a mask handle on the device (additive since ABI 5) ------------------
 * tsh_mask_create takes a bitmap the HOST made: for `tenant = 7` or `ts BETWEEN a AND b` the caller evaluates the
 * predicate row by row, maps primary keys to node ids (lib/src/core/vector_index_manager.dart:1223-1378), packs the
 * bitmap and hands it over, and the library slices, counts and uploads it again.  With a predicate per query (one
 * tenant each, a time window each) that is the whole cost of a lone filtered query.  An ATTRIBUTE handle keeps one
 * int64 column beside the rows on the device, by node id, 8 B per row; tsh_mask_create_range makes a mask handle from
 * one range term over it in one coalesced pass (tostore_amd/csrc/tsh_where.hip.h: a wave per 64 rows, its ballot is
 * the mask word), optionally combined with a handle that exists.  The bitmap never exists on the host first.  The
 * result is an ordinary tsh_mask: every entry that takes one works with it unchanged.
 *
 * tsh_attr_create: values[i] is the attribute of GLOBAL row id i; TSH_ATTR_NULL (INT64_MIN) says the row has no value,
 *   and rows at or beyond n read as NULL.  tsh_attr_set extends or overwrites [first_row_id, first_row_id + n): the
 *   append feed's companion (the column does not follow appends on its own).  Doubles and datetimes are stored by an
 *   order-preserving key (the bindings' f64_order_key: the value's bits b as int64, b if b >= 0 else
 *   b ^ 0x7FFFFFFFFFFFFFFF, NaNs made the positive quiet NaN first: double.compareTo's order, and never TSH_ATTR_NULL).
 * tsh_mask_create_range: row i of the index's current rows is kept iff  v[i] != NULL  and
 *   (lo <= v[i] <= hi) != (negate != 0),  the result and-ed (TSH_MASK_AND) or or-ed (TSH_MASK_OR) with W[i] when `with`
 *   is given -- W is with's bitmap, zero-extended to the current rows.  So a NULL row, or a row beyond the column, is
 *   kept by no term, negated or not (`with` under OR can still keep it); lo > hi is the empty range: nothing without
 *   negate, every non-NULL row with it.  The answer is exact: NumPy on the host is the specification.  Conjunctions,
 *   IN-lists and NOT are chains of calls (or one tsh_mask_create_where, below); each returns a new handle and the
 *   caller destroys the intermediates.  `with`
 *   may be any handle of the same index, made from a bitmap or from a range, and is left as it was.
 *   The handle is a SNAPSHOT: a later tsh_attr_set or tsh_attr_destroy does not change it, and rows appended later are
 *   not kept -- after a rebuild for a grown shard it keeps exactly the rows it kept before (the handle contract above).
 *   Tombstones and quarantined rows are treated as for any handle.
 *   TSH_E_BAD_ARG (each clears *out): a NULL idx, attr or out; combine neither TSH_MASK_AND nor TSH_MASK_OR, even with
 *   with == NULL; an attr or `with` made for another index, or orphaned.
 * tsh_mask_read: the handle's GLOBAL bitmap as it stands, for any handle however made: bit i (LSB first) = row id i,
 *   bytes past what the handle knows read 0.  (A bitmap-made handle answers with its copy of the caller's bits.)
 *   TSH_E_BAD_ARG: n_bytes < 0, a NULL out_bits with n_bytes > 0, an orphaned handle.
 * Lifetime: an attribute handle belongs to the index it was made for and works with any kind of handle -- a whole index,
 *   several devices (each shard holds its slice on its own device), a shard with global ids.  tsh_index_destroy
 *   orphans it: later use answers TSH_E_BAD_ARG, and tsh_attr_destroy then frees only the handle itself.  The two
 *   destroys may come in either order.
 * Threads: any number of tsh_mask_create_range calls may share one attribute handle.  tsh_attr_set takes the index lock
 *   the way an append does and waits for the calls that use the handle.
 * Cost, measured on 1 M x 768, L2, k = 100 ("Attribute columns"; profiles/mask_where_ab.json), medians by the
 *   host clock: making the handle takes 78 us for `x = c` keeping 1 % and 48 us for a range keeping 50 %, against 592
 *   and 554 us for the host route (NumPy compare, packbits, tsh_mask_create) and 55 and 24 us for tsh_mask_create
 *   alone from a bitmap that exists; a lone query including make and destroy takes 129 and 187 us against the host
 *   route's 650 and 698.  The range kernel runs 5.5 us; the copy of the words back to the host (the batched path and
 *   the quarantined rows read them there) is what the call costs over tsh_mask_create, and the list of a selective mask
 *   (M1 6.5 us + M2 5.2 us, tsh_mask.hip.h, with their synchronise) the 30 us between the two predicates.  M1 stayed a
 *   launch of its own: folding it into the range kernel would save under a tenth of the call.
 * The attribute handle is a tsh_attr * (typedef below) and travels as `void *`, tsh_attr_create's `out` -- the address
 *   of the caller's tsh_attr * -- too, exactly as a tsh_groups * does (see tsh_groups_create below).
 * Not here: string attributes (the bindings map them to int64 through a dictionary; multi-valued attributes are tag
 *   columns, tsh_tags_create below); a predicate evaluated inside the scan
 *   kernels without a handle; a column that follows appends on its own; collective (sharded) creation -- every rank
 *   makes its own handle from its own column, as with bitmaps. */
#define TSH_ATTR_NULL INT64_MIN
#define TSH_MASK_AND 0
#define TSH_MASK_OR 1
typedef struct tsh_attr tsh_attr;
int32_t tsh_attr_create(tsh_index *idx, const int64_t *values, int64_t n, void *out);
int32_t tsh_attr_set(void *attr, int64_t first_row_id, int64_t n, const int64_t *values);
int32_t tsh_attr_destroy(void *attr);
int32_t tsh_mask_create_range(tsh_index *idx, void *attr, int64_t lo, int64_t hi, int32_t negate, tsh_mask *with,
                              int32_t combine, tsh_mask **out);
int32_t tsh_mask_read(tsh_mask *mask, uint8_t *out_bits, int64_t n_bytes);

/* ---- a whole WHERE clause in one launch (additive since ABI 5) --------------------------------------------------------
 * A real WHERE is not one term: `tenant = 7 AND ts BETWEEN a AND b AND NOT flag = 1`, `category IN (3, 5, 8, 13, ...)`.
 * As a chain of tsh_mask_create_range calls every term, and every value of an IN-list, pays a whole call: a new handle
 * with its device buffers, a launch, the copy of the words back, the host prefix, the list kernels and their
 * synchronise, the un-slicing -- for handles nobody looks at.  tsh_mask_create_where evaluates the clause in ONE launch
 * and one finish per shard (W2 mask_where_kernel, tostore_amd/csrc/tsh_where.hip.h, planned by tsh_where_plan.h): each
 * distinct column is read once per row however many terms name it, and an IN-list is a sorted set in LDS that a lane
 * searches in at most 12 steps, not n equality terms.  The result is an ordinary tsh_mask.
 *
 * terms: n_terms tsh_where_term records (the array travels as `const void *`, as tsh_attr_create's out does).
 *   A term keeps row i iff  v[i] != TSH_ATTR_NULL  and  hit != (negate != 0),  v the term's column: for TSH_TERM_RANGE
 *   hit is lo <= v <= hi (set / n_set are not read, but must be well-formed); for TSH_TERM_IN hit is v in
 *   set[0, n_set) (lo / hi are not read).  Rows at or beyond the column read as NULL; a NULL row is kept by no term,
 *   negated or not.  The set's values come in any order, duplicates allowed; a TSH_ATTR_NULL among them is ignored;
 *   n_set == 0 is the empty set and lo > hi the empty range: nothing plain, every non-NULL row negated.  The library
 *   copies the sets: they need only live for the call.
 *   Terms of equal `clause` are OR-ed, and the clauses AND-ed; clause numbers start at 0 and never decrease or skip a
 *   number along the array.  If `with` is given the result is then and-ed / or-ed with its bitmap, zero-extended to the
 *   current rows, exactly as by tsh_mask_create_range; a call of one range term gives that entry's handle bit for bit.
 *   Limits: TSH_WHERE_MAX_TERMS terms, TSH_WHERE_MAX_COLUMNS distinct attribute handles, TSH_WHERE_MAX_SET_VALUES set
 *   values -- every IN term's own distinct non-NULL values, summed over the call.  Anything larger is written as
 *   chained calls through `with`.
 *   Snapshot, tsh_mask_read, rebuilds after appends, tombstones, quarantined rows, several devices and shard handles
 *   with global ids: as for a range-made handle.
 *   TSH_E_BAD_ARG (each clears *out, each answered before any device work): a NULL idx, terms or out; n_terms < 1 or
 *   > TSH_WHERE_MAX_TERMS; a NULL attr, or one made for another index, or orphaned; a `with` of another index; combine
 *   neither TSH_MASK_AND nor TSH_MASK_OR, even with with == NULL; a kind that is neither constant; reserved != 0;
 *   n_set < 0; a NULL set with n_set > 0; more than TSH_WHERE_MAX_COLUMNS distinct handles; more than
 *   TSH_WHERE_MAX_SET_VALUES set values; clause numbers out of order.
 * Threads: any number of calls may share attribute handles; a call takes every distinct handle's use lock shared, in
 *   the order of the handles' addresses, so two calls naming the same handles in opposite orders cannot deadlock against
 *   a waiting tsh_attr_set.
 * Cost, measured on 1 M x 768, L2, k = 100 ("A whole clause in one launch"; profiles/mask_where_terms_ab.json,
 *   written by tools/ab_mask_where_terms.py), medians by the host clock, the chain of tsh_mask_create_range calls with its
 *   intermediates destroyed against the one call: `tenant = 7 AND ts BETWEEN a AND b AND NOT flag = 1` (three calls) 241
 *   -> 88 us; `tenant IN (16 values)` (sixteen calls) 945 -> 58 us; `tenant IN (1024 values)` against the host route
 *   (NumPy isin, packbits, tsh_mask_create) 2552 -> 65 us.  A lone query including make and destroy: 292 -> 136, 1046 ->
 *   156 and 2709 -> 157 us.  The kernel runs 8.8 us on average over the three (W1 6.7); the call costs about one
 *   tsh_mask_create_range. */
#define TSH_TERM_RANGE 0
#define TSH_TERM_IN 1
#define TSH_WHERE_MAX_TERMS 32
#define TSH_WHERE_MAX_COLUMNS 8     /* distinct attribute handles in one call */
#define TSH_WHERE_MAX_SET_VALUES 4096 /* all IN terms of one call together, after the library's sort + dedupe */
typedef struct tsh_where_term {
  void *attr;         /* tsh_attr * of the same index */
  int64_t lo, hi;     /* TSH_TERM_RANGE */
  const int64_t *set; /* TSH_TERM_IN: n_set values, any order, duplicates allowed; may be NULL iff n_set == 0 */
  int64_t n_set;
  int32_t kind, negate;
  int32_t clause;     /* terms of equal clause are OR-ed; the clauses are AND-ed */
  int32_t reserved;   /* 0 */
} tsh_where_term;
int32_t tsh_mask_create_where(tsh_index *idx, const void *terms, int32_t n_terms, tsh_mask *with, int32_t combine,
                              tsh_mask **out);

/* ---- tag columns: an array-valued WHERE term made into a mask handle on the device (additive since ABI 5) -------------
 * The filter a vector table meets first is not scalar: `acl HAS ANY (the caller's 5 - 200 group ids)` differs for every
 * user and so for every query; `tags HAS ALL ('gpu', 'rocm')`, `NOT (labels HAS ANY (...))`.  The reference has the field
 * type (DataType.array, lib/src/model/table_schema.dart:1896) and would filter on the host
 * (lib/src/core/vector_index_manager.dart:1223-1378).  No attribute column can hold a row's set, so without this the caller
 * walks a ragged array per row per query, packs a bitmap and pays tsh_mask_create.  A TAG handle keeps the ragged column
 * beside the rows on the device as CSR, and tsh_mask_create_tags makes a mask handle from one HAS ANY / HAS ALL term over
 * it in one launch (T1 mask_tags_kernel, tostore_amd/csrc/tsh_tags.hip.h; the host side is tsh_tags_plan.h): a wave per
 * 64 rows streams those rows' values as ONE contiguous span, counts each row's matches against the term's sorted set in
 * LDS, and its ballot is the mask word.  The result is an ordinary tsh_mask.  It is not a new term kind of
 * tsh_mask_create_where: it composes with scalar clauses through `with`, as chained range calls do.
 *
 * tsh_tags_create: the column is CSR by GLOBAL row id: row i < n holds values[offsets[i] .. offsets[i + 1]); offsets has
 *   n + 1 entries, offsets[0] == 0, and never decreases (neither array is read when n == 0; values is not read when
 *   offsets[n] == 0).  The library keeps its own copy with every row's list sorted and deduplicated: a row is a SET.  A
 *   row whose list contains TSH_ATTR_NULL anywhere is a NULL row -- the field has no value -- and so is a row at or
 *   beyond n.  An empty list is a value, the empty set; it is NOT NULL.  Strings go in through the bindings' dictionary.
 * tsh_tags_set overwrites or extends rows [first_row_id, first_row_id + n); its offsets are relative to its own values,
 *   again from 0, and the lists may differ in length from those they replace.  Rows between the old end and first_row_id
 *   become NULL rows.  The append feed's companion: the column does not follow appends on its own.
 * tsh_mask_create_tags: let S be set[0, n_set) with duplicates and TSH_ATTR_NULL dropped, c_i = |row_i n S|, and the
 *   threshold t = |S| if need == TSH_TAGS_ALL, else need (TSH_TAGS_ANY is 1; any n >= 1 says "at least n distinct values
 *   of the set").  Row i of the index's current rows is kept iff it is not NULL and  (c_i >= t) != (negate != 0);  the
 *   result is then and-ed (TSH_MASK_AND) or or-ed (TSH_MASK_OR) with `with`'s bitmap, zero-extended to the current rows,
 *   exactly as by tsh_mask_create_range.  So HAS ALL of an empty S keeps every non-NULL row (t = 0) and HAS ANY of an
 *   empty S keeps none; need > |S| keeps none and, negated, every non-NULL row, empty-set rows included; a NULL row is
 *   kept by no term, negated or not.  The answer is exact: NumPy on the host is the specification.  The library copies
 *   the set: it need only live for the call.  One tag term per call; several are chained through `with`.
 *   Snapshot (a later tsh_tags_set or tsh_tags_destroy does not change the handle, rows appended later are not kept),
 *   tsh_mask_read, tsh_mask_kept, rebuilds after appends, tombstones, quarantined rows, several devices and shard handles
 *   with global ids: as for a range-made handle.
 * TSH_E_BAD_ARG (each clears *out, each answered before any device work): a NULL idx, tags or out; n < 0; NULL offsets
 *   with n > 0; offsets[0] != 0, or a decreasing offset; NULL values with offsets[n] > 0; first_row_id < 0; need < 0;
 *   n_set < 0, or a NULL set with n_set > 0; |S| > TSH_TAGS_MAX_SET_VALUES; combine neither TSH_MASK_AND nor TSH_MASK_OR,
 *   even with with == NULL; a tags or `with` handle of another index, or an orphaned one.  And: the device offsets are
 *   32-bit, so a shard's slice of the column may hold at most 2^31 - 1 values; the call that would build such a part
 *   (tsh_tags_create, or the tsh_mask_create_tags after a tsh_tags_set or an append) refuses it.
 * Lifetime: as an attribute handle's.  tsh_index_destroy orphans a live tag handle (later use answers TSH_E_BAD_ARG,
 *   tsh_tags_destroy then frees only the handle itself); the two destroys may come in either order.
 * Threads: any number of tsh_mask_create_tags calls may share one tag handle.  tsh_tags_set takes the index lock the way
 *   an append does and waits for the calls that use the handle.
 * Cost, measured on 1 M x 768, L2, k = 100 ("tag columns"; profiles/mask_tags_ab.json, written by
 *   tools/ab_mask_tags.py), us by the host clock, medians over five processes with their lowest and highest, the device
 *   route against the host route (NumPy isin over the flat values, bincount by owner, compare, packbits,
 *   tsh_mask_create).  An ACL-shaped column, 1 - 8 group ids per row out of 10 000 (4.5 M stored values): HAS ANY of 5
 *   values 90.7 (87.7 - 100.9) against 24 838 (24 502 - 28 053), of 64 values 94.3 against 22 549, of 1024 values 87.9
 *   against 23 101, HAS ALL of 2 values 61.8 against 30 053; a lone query including make and destroy 137.6, 171.7, 212.5
 *   and 115.4 against 24 967, 22 689, 23 328 and 30 182.  A tag-shaped column, 0 - 32 tags per row out of 1 000 (15.8 M
 *   stored values): HAS ANY of 5 values 78.4 (76.5 - 82.0) against 77 734 (76 590 - 77 947), of 64 values 87.1 against
 *   75 855, of all 1 000 values 132.8 against 89 369, HAS ALL of 2 values 104.1 against 46 683; a lone query 167.0,
 *   237.1, 332.7 and 152.4 against 77 915, 76 110, 89 657 and 46 790.  In every shape the device route's slowest process
 *   is faster than the host route's fastest.  The kernel itself, from a kernel trace in a run of its own: 9.4 - 32.0 us
 *   on the ACL-shaped column and 22.6 - 78.7 us on the tag-shaped one (it reads 8 B per stored value, 4 B per row of
 *   offsets and 8 B per 64 rows of valid bits, once; the longest is the term every stored value matches); the rest of
 *   the call is the tail every device-made handle pays (tsh_mask_create_range above).
 * The tag handle is a tsh_tags * (typedef below) and travels as `void *`, tsh_tags_create's `out` -- the address of the
 *   caller's tsh_tags * -- too, exactly as a tsh_attr * does.
 * Not here: tag terms inside tsh_mask_create_where's term table; more than one tag term per call; string values; a
 *   column that follows appends on its own; collective (sharded) creation -- every rank makes its own handle from the
 *   global CSR; a predicate evaluated inside the scan kernels without a handle. */
#define TSH_TAGS_ALL 0   /* need: every distinct non-NULL value of the set */
#define TSH_TAGS_ANY 1   /* need: at least one; any n >= 1 means "at least n distinct values of the set" */
#define TSH_TAGS_MAX_SET_VALUES 4096 /* the term's set, after the library's sort + dedupe */
typedef struct tsh_tags tsh_tags;
int32_t tsh_tags_create(tsh_index *idx, const int64_t *offsets, int64_t n, const int64_t *values, void *out);
int32_t tsh_tags_set(void *tags, int64_t first_row_id, int64_t n, const int64_t *offsets, const int64_t *values);
int32_t tsh_tags_destroy(void *tags);
int32_t tsh_mask_create_tags(tsh_index *idx, void *tags, const int64_t *set, int64_t n_set, int32_t need,
                             int32_t negate, tsh_mask *with, int32_t combine, tsh_mask **out);

/* ---- facet counts: rows per value of an attribute or tag column, on the device (additive since ABI 5) -----------------
 * A search screen that filters by the columns above also shows their facets: "Brand: A (312), B (207)", "Price: under 10
 * (1 204), 10 - 50 (3 310)", "tags: gpu (88), rocm (41)".  Without these entries a caller reads the mask back and walks the
 * column on the host, or makes one mask handle per value and pays a tsh_search_count each.  The column, the mask's words
 * and the live bitmap are on the device already; one launch per shard counts there (F1 attr_facets_kernel, F2
 * tags_facets_kernel, tostore_amd/csrc/tsh_facet.hip.h; the host side is tsh_facet_plan.h): a wave per 64 rows, each
 * lane's bucket found by a branch-free search of the keys in LDS, 32-bit counters in LDS, one 64-bit add per nonzero
 * counter and workgroup at the end.
 *
 * The population P -- the rows a search under `mask` could return: row ids 0 <= i < tsh_index_size that are present (not a
 *   gap, not an absent page), not tombstoned and, if `mask` is given, kept by it (rows beyond its bitmap are not kept;
 *   mask == NULL is no filter).  Quarantined rows (non-finite or huge elements) are in P: searches return them.  On a
 *   shard handle P is the shard's own rows under the GLOBAL mask and the GLOBAL column, and the caller adds the ranks'
 *   answers; a handle over several devices sums its shards itself.
 *   out_rest[2] == tsh_search_count(any finite query, threshold NaN, no cursor, the same mask).
 * tsh_attr_facets: v_i is the column's value of row i; rows beyond the column read as TSH_ATTR_NULL.
 *   TSH_FACET_VALUES: keys in any order, duplicates allowed; out_counts[j] = #{i in P : v_i == keys[j]} in the caller's
 *   order (a repeated key repeats its count; a TSH_ATTR_NULL among the keys matches nothing).
 *   TSH_FACET_EDGES: keys ascend strictly and keys[0] != TSH_ATTR_NULL; bucket j counts keys[j] <= v_i < keys[j + 1] and
 *   the last bucket v_i >= keys[n_keys - 1]: a value equal to an edge falls in the bucket that edge opens.
 *   out_rest[0] = "other", the rows of P with a non-NULL value in no bucket; out_rest[1] = the rows of P whose value is
 *   NULL; out_rest[2] = |P|.  The counts of the distinct keys + out_rest[0] + out_rest[1] == out_rest[2].  n_keys == 0 is
 *   legal: out_counts is not written, every non-NULL row is "other", keys and out_counts may be NULL.
 * tsh_tags_facets: a row is a set, NULL if its list holds TSH_ATTR_NULL or it lies beyond the column; an empty list is a
 *   value.  out_counts[j] = #{i in P : row i not NULL, keys[j] in row_i}; out_rest[0] = the non-NULL rows of P that hold
 *   none of the keys (empty sets included); out_rest[1] = the NULL rows of P; out_rest[2] = |P|.
 * The answer is exact: NumPy on the host is the specification; the adds are integer adds, so two runs agree bit for bit.
 *   The column is read as it stands when the call runs -- no handle is made, so there is no snapshot.  An empty index
 *   gives zeros.
 * TSH_E_BAD_ARG (each answered before any device work, nothing is written): a NULL idx, column or out_rest; n_keys < 0;
 *   NULL keys or out_counts with n_keys > 0; more than TSH_FACET_MAX_KEYS distinct non-NULL keys; a kind that is neither
 *   constant; edges that do not ascend strictly or start with TSH_ATTR_NULL; a column or mask made for another index, or
 *   an orphaned one.
 * Threads: any number of calls may share the handles; tsh_attr_set and tsh_tags_set wait for them, as they do for the
 *   mask makers.
 * Cost: DESIGN.md, "facet counts".
 * Not here: facets under a distance threshold; discovering the distinct values without keys (the bindings' dictionaries
 *   know them); more than TSH_FACET_MAX_KEYS keys in one call -- chain calls; a ticket form; collective (sharded) summing
 *   -- every rank answers for its rows. */
#define TSH_FACET_VALUES 0      /* bucket j: rows whose value == keys[j] */
#define TSH_FACET_EDGES  1      /* bucket j: keys[j] <= value < keys[j+1]; the last bucket: value >= keys[n_keys-1] */
#define TSH_FACET_MAX_KEYS 4096 /* distinct non-NULL keys of one call */
int32_t tsh_attr_facets(tsh_index *idx, void *attr, tsh_mask *mask, int32_t kind, const int64_t *keys, int64_t n_keys,
                        int64_t *out_counts, int64_t *out_rest);
int32_t tsh_tags_facets(tsh_index *idx, void *tags, tsh_mask *mask, const int64_t *keys, int64_t n_keys,
                        int64_t *out_counts, int64_t *out_rest);

/* Asynchronous form of a single-query tsh_search, for callers that keep several
 * independent queries in flight (the reference serves concurrent vectorSearch
 * calls from its isolate pool, lib/src/Interface/compute_native.dart:18-300): a
 * submitted query's select / re-rank / copies overlap the next query's corpus
 * scan.  At most tsh_max_inflight() un-waited tickets per handle (TSH_E_BUSY
 * beyond).  The handle is share-locked from submit to wait: appends and deletes
 * block until every ticket is waited.  Every ticket must be waited exactly once
 * before tsh_index_destroy.  Results are identical to tsh_search. */
int32_t tsh_max_inflight(void);
int32_t tsh_search_submit(tsh_index *idx, const float *query, int32_t k, const uint8_t *row_mask,
                          int32_t *out_ticket);
/* 1 = the ticket's kernels have finished (tsh_search_wait will not wait for the GPU), 0 = still running, < 0 =
 * error.  Never blocks: a single-threaded host (a Dart isolate, whose yield budget is 8 ms on clients and 50 ms on
 * servers: lib/src/model/data_store_config.dart:225-230, core/yield_controller.dart:110-169) submits, returns to
 * its event loop, and waits once this says 1. */
int32_t tsh_search_ready(tsh_index *idx, int32_t ticket);
int32_t tsh_search_wait(tsh_index *idx, int32_t ticket, double distance_threshold, int64_t *out_ids,
                        double *out_dist, int32_t *out_count);

/* ---- search after a cursor: the next k rows past (distance, id) (additive since ABI 5) ----------------------
 * Let L be the list tsh_search would return for the query with k = infinity, under the same mask, tombstones and
 * threshold: ordered by Dart double.compareTo on the distance (-0.0 before 0.0, NaN last), ties by row id
 * (ngh_graph_engine.dart:122-134).  tsh_search_after returns the first k entries of L that are strictly greater than
 * (after_dist[q], after_id[q]) in that order; the cursor need not name an existing row.  after_dist = -inf with any id
 * is "from the start" and equals tsh_search bit for bit.  The concatenation of successive pages, each started from the
 * last entry of the page before, is exactly L; a page shorter than k is the last one.  Each page costs one scan,
 * however deep it is: a pass over the scan's keys takes the rows at or before the cursor out of the select's sight,
 * and the few rows whose f32 key cannot tell are decided by their exact distances (tostore_amd/csrc/tsh_after.hip.h,
 * tsh_after_band.h).  "Everything within distance_threshold" is a loop of pages that ends at the first short page.
 * How long that list is, without walking it: tsh_search_count below.
 * row_mask / mask: at most one of the two forms of a WHERE row set, or neither.  after_dist / after_id: nq each.
 * Works on whole-index handles, handles over several devices and shard handles (global ids).  Several queries per
 * call run as the pipeline of single-query scans, never on the batched path.  TSH_E_BAD_ARG: both masks, a NULL
 * cursor array, a mask handle made for another index.  tsh_search_submit_after is the asynchronous form; its ticket is
 * waited for with tsh_search_wait.
 * tsh_search_after_stats, summed over the shards (a search counts once per shard, as tsh_counters.searches does; that
 * struct keeps its layout and counts cursor searches in searches and scan_launches like any other): out[0] = cursor
 * searches, out[1] = rows their floor passes could not decide and sent to the side list, out[2] = searches redone
 * because the side list overflowed (more than 1024 rows tied with the cursor), out[3] = searches answered without a
 * floor on the device (safe mode, where the finaliser filters; a +inf or NaN cursor, which only quarantined rows can
 * follow: no scan runs).
 * Sharded callers page with the *_after forms of the sharded entries below (tsh_search_shard_after,
 * tsh_search_shard_begin_after, tsh_merge_candidates_after, tsh_search_sharded_after): the cursor is GLOBAL, and the
 * order is total across shards, so the rows after it are the union of every shard's rows after it.  These calls count
 * in tsh_search_after_stats of the shard handle like any other cursor search. */
int32_t tsh_search_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double distance_threshold,
                         const uint8_t *row_mask, tsh_mask *mask, const double *after_dist, const int64_t *after_id,
                         int64_t *out_ids, double *out_dist, int32_t *out_count);
int32_t tsh_search_submit_after(tsh_index *idx, const float *query, int32_t k, const uint8_t *row_mask, tsh_mask *mask,
                                double after_dist, int64_t after_id, int32_t *out_ticket);
int32_t tsh_search_after_stats(tsh_index *idx, int64_t *out);

/* ---- count the rows a search would return (additive since ABI 5) --------------------------------------------------
 * out_count[q] is the number of entries in the list tsh_search_after would return for query q with k = infinity: the
 * row mask (pointer or handle, at most one), tombstones, gaps, quarantined rows, distance_threshold and cursor are the
 * same.  A row counts only if it passes the threshold as the finaliser applies it (dropped iff distance >
 * distance_threshold under IEEE >: a NaN threshold is none, a NaN distance passes any, -0.0 and +0.0 are one threshold)
 * and, with a cursor, only if it follows (after_dist[q], after_id[q]) strictly in (double.compareTo(distance), id)
 * order.  after_dist == after_id == NULL: no cursor, the list is tsh_search's; a cursor of -inf is "from the start";
 * exactly one NULL is TSH_E_BAD_ARG, as are both mask forms at once and a mask handle made for another index.  So after
 * any page, count(after = the page's last entry) is count(no cursor) minus the rows consumed so far; a caller shows
 * "4 312 results" beside the first page, sizes the buffers of a range loop, or finds a row's position in its list.
 * Cost: one scan, one pass over the scan's 4 B per row, and the exact distances of the few rows whose f32 key cannot
 * tell (tostore_amd/csrc/tsh_count.hip.h, tsh_count_band.h) -- no select, no re-rank, no candidate block; the output
 * is one integer however many rows qualify.  A count job takes the f32 tile scan or the list scan, never the exact path
 * or the fp16 / int8 copies; several queries per call run as the pipeline of single-query scans, never on the batched
 * path.  An empty index gives counts of 0.  Works on whole-index handles, on handles over several devices (the
 * library sums its shards' counts) and on shard handles: there the count covers the shard's own rows under a GLOBAL
 * mask and a GLOBAL cursor, and since the order is total across shards the caller adds the ranks' counts by whatever
 * transport it has.  tsh_counters keeps its layout and counts a count in searches and scan_launches like any other
 * search.  tsh_search_count_stats, summed over the shards (a count counts once per shard): */
int32_t tsh_search_count(tsh_index *idx, const float *queries, int32_t nq, double distance_threshold,
                         const uint8_t *row_mask, tsh_mask *mask,
                         const double *after_dist, const int64_t *after_id, int64_t *out_count);
/* out[0] count searches, out[1] rows sent to the side list, out[2] searches redone with a larger side list,
 * out[3] searches answered without a device window pass (safe mode; nothing for a key to decide) */
int32_t tsh_search_count_stats(tsh_index *idx, int64_t *out);

/* ---- grouped search: the nearest row of each of the k nearest groups (additive since ABI 5) -----------------------
 * The rows of a vector table are chunks of documents, frames of videos, variants of products; the answer wanted is
 * "the 10 nearest documents", each shown by its best chunk.  Let L be the list tsh_search would return for the query
 * with k = infinity: the same row mask (pointer or handle, at most one), tombstones, gaps, quarantined rows and
 * distance_threshold, ordered by Dart double.compareTo on the distance with ties by row id.  Every row belongs to a
 * group: its entry in the groups handle's array; a row whose entry is negative, or which lies beyond the array, is
 * UNGROUPED -- a group of its own.  G is L with every entry removed whose group occurred earlier in L, and
 * tsh_search_grouped returns the first k entries of G: ids and distances bit for bit those of L; out_group[i] (nullable)
 * is the entry's group, -1 for an ungrouped row; unused slots read id -1, distance NaN, group -1.  So with every row
 * ungrouped, or every row in a group of its own, the answer is tsh_search's; with all rows in one group it is L's first
 * entry; and a group is represented by its best row that SURVIVES mask, tombstones and threshold -- a group with no
 * surviving row does not appear.
 *
 * A groups handle holds the array: group_of[i] is the group of GLOBAL row id i, >= 0 and < n_groups, or negative.
 * tsh_groups_set extends or overwrites the entries [first_row_id, first_row_id + n): the append feed's companion.
 * Lifetime: a groups handle belongs to the index it was made for and works with any kind of handle -- a whole index,
 *   several devices (groups may span the shards: the finaliser's step runs once over all of them), a shard with global
 *   ids.  tsh_index_destroy orphans it, it is not left dangling: later use answers TSH_E_BAD_ARG, and
 *   tsh_groups_destroy then frees only the handle itself.  The two destroys may come in either order.
 * Threads: any number of searches may share one handle.  tsh_groups_set takes the index lock the way an append does
 *   and waits for the searches that use the handle.
 * Limits: n_groups <= 1 << 26 (every query context that runs a grouped search keeps 8 B per group on the device).
 *   TSH_E_BAD_ARG answers a larger table, an id at or above n_groups, both mask forms at once, a mask or groups handle
 *   made for another index, and a NULL `groups`.
 * Trivial cases: k <= 0 or an empty index returns TSH_OK with counts of 0.
 * Several queries per call run as the pipeline of single-query scans, never on the batched path.
 * A shard handle answers for its own rows; the ranks' answers merge by concatenating them, ordering, dropping repeated
 *   groups and cutting to k, which is exact: a winning group's best row is the best of its group on the rank that holds
 *   it, and fewer than k groups beat it there.
 * Cost: a grouped search takes the f32 tile scan or the list scan -- never the exact path, the fp16 / int8 copies or the
 *   batched path --, three passes over the scan's 4 B per row around the unchanged select and re-rank, and the exact
 *   distances of the few rows that are not their group's nearest by f32 key but may be exactly
 *   (tostore_amd/csrc/tsh_group.hip.h, tsh_group_rule.h).  On big shards, whose plain tsh_search reads the int8 copy
 *   (a quarter of the bytes), one grouped search therefore costs several plain searches -- measured on 1 M x 768, L2,
 *   64-query calls: 446 us per query against 118, a factor of 3.8, the ratio of the two scans' bytes; against the
 *   caller's loop of tsh_search_after pages until k groups were seen (984 us at k = 10, 1258 at k = 100, 2 to 4 pages) it
 *   is 0.45 resp. 0.35, and it costs what tsh_search_count costs ("Grouped search";
 *   profiles/search_grouped_ab.json).
 * A cursor, so that groups can be paged, and a count of groups: tsh_search_grouped_after and tsh_search_grouped_count,
 *   below.  More than one row per group: tsh_search_grouped_rows, below them.  Across row-range shards, one process
 *   per GPU: tsh_search_shard_grouped, tsh_merge_candidates_grouped and tsh_search_sharded_grouped, with the other
 *   sharded entries below.  The next step would bring, none of it here: a ticket form (tsh_search_submit_grouped).
 * tsh_counters keeps its layout; a grouped search counts in searches and scan_launches like any other search.
 * The handle is a tsh_groups * (typedef below).  In the prototypes it travels as `void *`, and tsh_groups_create's
 * `out` -- the address of the caller's tsh_groups * (a tsh_groups **) -- as `void *` too: the bindings' prototype tables
 * (tests/test_dart_bridge.py) know a closed list of C types, every opaque handle is a pointer to them anyway, and an
 * additive entry does not widen that list.  C callers pass their tsh_groups * and its address as they are. */
typedef struct tsh_groups tsh_groups;
int32_t tsh_groups_create(tsh_index *idx, const int32_t *group_of, int64_t n, int32_t n_groups, void *out);
int32_t tsh_groups_set(void *groups, int64_t first_row_id, int64_t n, const int32_t *group_of);
int32_t tsh_groups_destroy(void *groups);
int32_t tsh_search_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double distance_threshold,
                           const uint8_t *row_mask, tsh_mask *mask, void *groups, int64_t *out_ids,
                           double *out_dist, int32_t *out_group, int32_t *out_count);
/* out[0] grouped searches, out[1] rows sent to the side list, out[2] searches redone with a larger side list,
 * out[3] searches answered without the device group passes (safe mode); summed over the shards */
int32_t tsh_search_grouped_stats(tsh_index *idx, int64_t *out);

/* ---- grouped search behind a cursor, and a count of groups (additive since ABI 5) ------------------------------------
 * L and G as above: G is L with every entry removed whose group occurred earlier, under the same row mask (pointer or
 * handle, at most one), tombstones, gaps, quarantined rows and distance_threshold.
 *
 * tsh_search_grouped_after takes tsh_search_grouped's arguments and a cursor per query (after_dist / after_id, nq
 * each).  It returns the first k entries of G that follow (after_dist[q], after_id[q]) strictly, in tsh_search_after's
 * order (double.compareTo on the distance, ties by id).  A cursor of -inf is "from the start" and equals
 * tsh_search_grouped bit for bit.  Successive pages, each started from the last entry of the page before, concatenate
 * to exactly G; a page shorter than k is the last.  The cursor need not name an existing row.  A group whose best row
 * is at or before the cursor is consumed: none of its rows comes back, those past the cursor included -- which is what
 * tsh_search_after pages with the repeated groups dropped by the caller cannot give without remembering every group
 * shown.  Unused slots and out_group behave as in tsh_search_grouped.  A NULL cursor array is TSH_E_BAD_ARG; the other
 * argument errors and the trivial cases are the grouped search's.
 *
 * tsh_search_grouped_count: out_count[q] is the number of entries of G (k = infinity) that pass the threshold exactly
 * as the finaliser applies it (tsh_search_count's words) and, with a cursor, follow it.  after_dist == after_id == NULL:
 * no cursor; exactly one NULL is TSH_E_BAD_ARG.  After any page, count(after = the page's last entry) == count(no
 * cursor) - entries of G returned so far.
 *
 * How (tostore_amd/csrc/tsh_group_after_rule.h has the rules and their proof, tsh_group.hip.h the kernels): the head
 * table is built over all live rows, whatever the cursor; a group is classified by its head's f32 key against the
 * cursor's floor keys (resp. the count's window) -- certainly after the cursor: today's grouped rules; certainly before
 * it: consumed, none of its rows goes anywhere; undecided: the head and the group's rows within the head's band get
 * their exact distances and the finaliser decides.  Several queries per call run as the pipeline of single-query f32
 * tile scans or list scans, never the batched path, the fp16 / int8 copies or the exact path.  A +inf or NaN cursor runs
 * no scan (no scanned row follows it).
 *
 * The exact-all route.  The per-shard rule does not hold (a) for a handle over several devices whose groups have rows
 * in the row ranges of two shards -- one shard consumes a group while another offers one of its rows; found on the host
 * by one pass over the array whenever it is given or changed (tsh_groups_create, tsh_groups_set) -- and (b) while a
 * shard holds a live quarantined row: such rows are not in the head table, yet can be a group's best or consume it;
 * looked at per call under the shard locks.  Every shard's job of such a call then runs as safe mode does: no device
 * group passes, every live row's exact sums reach the finaliser, which then IS the specification.  This route is slow
 * -- the exact distance of every live row per query -- and exact.  The cheaper follow-up, not built here: flag the few
 * open groups (spanning, or holding a quarantined row) in the device copy of group_of, so that only their rows go to
 * the side list.
 *
 * Shard handles: the answer is for the shard's own rows, as if they were the whole index.  The ranks' merged pages
 * (concatenate, order, drop repeated groups, cut to k) are exact ONLY when no group has rows on two ranks: with a cursor,
 * a group consumed on one rank can reappear from another.  The tsh_search_shard* / tsh_search_sharded* forms stay out
 * of scope.
 *
 * tsh_search_grouped_after_stats, summed over the shards (a job counts once per shard): out[0] grouped cursor searches,
 * out[1] group counts, out[2] rows sent to the side list, out[3] jobs redone with a larger side list, out[4] jobs
 * answered by the exact-all route (safe mode's jobs included: they run the same way).  These jobs move NONE of
 * tsh_search_grouped_stats, tsh_search_after_stats and tsh_search_count_stats, which keep their meaning for their own
 * entries; tsh_counters counts them in searches and scan_launches like any other search.
 * Cost: a page costs one grouped search at any depth -- measured on 1 M x 768, L2, 64-query calls, per query: pages 1, 2
 * and 10 at 453.2 / 453.4 / 453.7 us (k = 10) and 453.9 / 454.0 / 454.2 us (k = 100) against 453.0 / 453.6 us of
 * tsh_search_grouped in the same run, and against 999 / 1237 / 1485 us (k = 10) of the caller's loop of tsh_search_after
 * pages with repeated groups dropped on the host, which grows with depth; a group count 469.9 us against 453.4 us of
 * tsh_search_count ("grouped search behind a cursor"; profiles/search_grouped_after_ab.json). */
int32_t tsh_search_grouped_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, double distance_threshold,
                                 const uint8_t *row_mask, tsh_mask *mask, void *groups,
                                 const double *after_dist, const int64_t *after_id, int64_t *out_ids,
                                 double *out_dist, int32_t *out_group, int32_t *out_count);
int32_t tsh_search_grouped_count(tsh_index *idx, const float *queries, int32_t nq, double distance_threshold,
                                 const uint8_t *row_mask, tsh_mask *mask, void *groups,
                                 const double *after_dist, const int64_t *after_id, int64_t *out_count);
int32_t tsh_search_grouped_after_stats(tsh_index *idx, int64_t *out);

/* ---- grouped search, several rows per group ------------------------------
 * tsh_search_grouped_rows: the rows_per_group nearest rows of each of the k nearest groups -- a document's best
 * passages, a video's best frames -- from the one scan of a grouped search.  L and G as above (L: tsh_search's list for
 * k = infinity under the same row mask, tombstones, gaps, quarantined rows and threshold; G: L without every entry whose
 * group occurred earlier).  The k winning groups are the groups of G's first k entries, in that order; for the i-th of
 * them the answer holds the first rows_per_group entries of L that belong to it, in L's order, ids and distances bit for
 * bit those of L.  An ungrouped row is a group of one row; a group with fewer surviving rows gives what it has; a row
 * that fails the threshold, the mask or the tombstones never appears, so the first row of every group is exactly what
 * tsh_search_grouped returns.  With rows_per_group = 1 the entry equals tsh_search_grouped bit for bit; with every row
 * in one group it equals tsh_search cut to rows_per_group.
 *
 * Slot (q, i, j) lives at (q * k + i) * rows_per_group + j of out_ids / out_dist; unused slots read id -1 and distance
 * NaN.  out_group / out_rows (nq x k, either may be NULL): the group (-1: ungrouped) and the rows it returned; an unused
 * group reads -1 and 0.  out_count (nq): the groups returned.  rows_per_group runs from 1 to 64 -- an interface limit --
 * and anything else is TSH_E_BAD_ARG, except that rows_per_group <= 0 together with k <= 0 or an empty index is the
 * grouped search's trivial case (TSH_OK, counts 0).  Every other argument error is tsh_search_grouped's: NULL groups,
 * both mask forms, a handle of another index or of a destroyed one.  At most one of row_mask / mask.
 *
 * How: a grouped job up to its re-rank.  The groups whose head key is at or below the band the select left contain every
 * winning group; they are marked, their live rows gathered, and of each the rows at or below band_of(the group's
 * rows_per_group-th smallest key) -- all rows of a smaller group -- get their exact sums beside the select's candidates
 * (tostore_amd/csrc/tsh_group_rows_rule.h has the proof, tsh_group_rows.hip.h the five passes).  No host round trip
 * inside a job; the finaliser runs once per query over all shards.  Several queries per call run as the pipeline of
 * single-query f32 tile scans or list scans, never the batched path, the fp16 / int8 copies or the exact path, as the
 * other grouped jobs do.
 *
 * The EXACT-ALL route, slow and exact (every live row's exact sums reach the finaliser, no device group passes), is
 * taken in the cases the grouped cursor search takes it in: a handle over several devices whose groups span two shards'
 * row ranges (a winning group's second row can lie on a shard where the group is not marked at all), a shard that holds a
 * live quarantined row (its group can win through a row the head table does not hold), and safe mode.  A job that marks
 * more groups than it has slots for (2 k + 64: no bound at all from the select, or heads tied at the k-th by the
 * hundred) runs again on that route; a job whose member or side lists overflow is redone once with lists sized from
 * the counts the first run left.
 *
 * tsh_search_grouped_rows_stats, summed over the shards (a job counts once per shard): out[0] searches, out[1] marked
 * groups, out[2] member rows sent on for exact sums, out[3] jobs redone with larger lists (or on the exact-all route
 * after their slots ran out), out[4] jobs answered by the exact-all route.  These jobs move NONE of the other *_stats;
 * tsh_counters keeps its layout and counts them in searches and scan_launches like any other search.
 *
 * Cost: the new passes read the 4 B key, the 4 B group id and one 8 B table word per row where the scan reads 3 KB --
 *   measured on 1 M x 768, L2, groups of 8 rows, 64-query calls, per query: 447.8 to 452.5 us at k = 10 for m = 1, 3 and
 *   10 (1.003 to 1.006 of tsh_search_grouped in the same process; 10.0 marked groups, 10 / 30 / 80 member rows per job),
 *   449.9 to 468.2 us at k = 100 (1.010 to 1.051; 100.4 marked groups, 100 / 301 / 803 member rows), against 445.1 to
 *   452.5 us for tsh_search_grouped, and against 1436 to 4149 us for the caller's loop of tsh_search_grouped and
 *   tsh_search_after pages, which after six pages of k m rows still missed 4 to 8 % of the rows at m = 3.  The five
 *   passes take 4.5 to 5.4 us each on an idle device ("several rows per group";
 *   profiles/search_grouped_rows_ab.json, profiles/search_grouped_rows_kernel_stats.txt).
 *
 * Out of scope: a cursor or a count with rows per group; a ticket form; the tsh_search_shard* / tsh_search_sharded*
 * entries (a shard handle answers for its own rows; merging ranks' answers is exact only when no group has rows on two
 * ranks); a cheaper handling of spanning or quarantined groups than the exact-all route. */
int32_t tsh_search_grouped_rows(tsh_index *idx, const float *queries, int32_t nq, int32_t k, int32_t rows_per_group,
                                double distance_threshold, const uint8_t *row_mask, tsh_mask *mask, void *groups,
                                int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_rows,
                                int32_t *out_count);
int32_t tsh_search_grouped_rows_stats(tsh_index *idx, int64_t *out);

/* ---- row-sharded deployments (one process per GPU) ----------------------
 * Each rank scans its shard and emits, per query, one fixed-size candidate
 * block into DEVICE memory; ranks all-gather the blocks (RCCL) and any rank
 * merges them on the host.  A block = 64-byte header + entries x 24 bytes
 * {int64 global id, f64 sum0, f64 sum1} holding the exact f64 accumulations
 * of ngh_graph_engine.dart:920-946 for every row that can be in the shard's
 * top k. */
int64_t tsh_candidate_block_bytes(int32_t entries);
int32_t tsh_default_block_entries(int32_t k);
/* d_out_blocks: device buffer of nq * tsh_candidate_block_bytes(entries) on the
 * handle's device; the kernels store the blocks into it directly and the call
 * returns after they completed (host-synchronised), so any stream may read it
 * next.  stream: reserved (pass NULL or the consumer's hipStream_t) -- a block is
 * final only once the HOST has seen its header (ties that overflow a block's
 * candidate list are redone by a wider pass the host starts), so completion
 * cannot be handed to a stream; a caller that wants to work on the first blocks
 * while the later ones are still being scanned uses the progressive form below.
 * row_mask is GLOBAL (bit = global row id).  Rows kept out of the scan (tsh_counters.quarantined_rows) are
 * appended to every block the mask lets them into; a block they do not fit in reports count > entries like any
 * other overflow, and tsh_merge_candidates answers TSH_E_OVERFLOW with the entry count to retry with. */
int32_t tsh_search_shard(tsh_index *idx, const float *queries, int32_t nq, int32_t k,
                         const uint8_t *row_mask, int32_t entries, void *d_out_blocks,
                         void *stream);
/* Progressive form of tsh_search_shard, for callers that exchange the blocks in
 * groups (tsh_search_sharded is built on it; tostore_amd/sharded.py can be): the
 * scans of ALL nq queries run as one pipeline on a library thread -- the GPU sees
 * no group boundaries, where group-by-group tsh_search_shard calls pay the fill and
 * drain of the scan pipeline per call (~45 us on a 125 k x 768 shard) -- and the
 * blocks become final in query order.
 *   _begin     starts the search and returns at once; queries / row_mask are copied
 *              (no pointer is retained), d_out_blocks must stay valid until _end.
 *              step: the caller's group size (queries it will ask for at a time);
 *              where a call of `step` queries would go to the matrix cores the
 *              search proceeds in calls of `step` queries, otherwise every query is
 *              its own scan.  0 = nq.
 *   _progress  blocks until the first min(want, nq) queries' blocks are final in
 *              d_out_blocks (host-synchronised: any stream may read them next) and
 *              returns TSH_OK, or until the search failed before it got there and
 *              returns its error; *out_done (nullable) = leading queries final.
 *   _end       waits for whatever still runs, frees the handle, returns the
 *              search's status.  Must be called exactly once per _begin.
 * Blocks, masks, overflow protocol: exactly tsh_search_shard's.  No reference
 * counterpart (the reference has no distributed compute). */
typedef struct tsh_shard_stream tsh_shard_stream;
int32_t tsh_search_shard_begin(tsh_index *idx, const float *queries, int32_t nq, int32_t k,
                               const uint8_t *row_mask, int32_t entries, void *d_out_blocks,
                               int32_t step, tsh_shard_stream **out);
int32_t tsh_search_shard_progress(tsh_shard_stream *stream, int32_t want, int32_t *out_done);
int32_t tsh_search_shard_end(tsh_shard_stream *stream);
/* Host-side merge of n_blocks x nq candidate blocks (layout [block][query]),
 * applying the final sqrt / negate / 1-cos, threshold, ordering and top-k cut.
 * Pure host code (no device needed).  Returns TSH_E_OVERFLOW if any block was
 * truncated: every rank sees the same headers, so all ranks retry with the
 * entry count written to *needed_entries. */
int32_t tsh_merge_candidates(int32_t metric, int32_t dim, const float *queries,
                             int32_t nq, int32_t k, double distance_threshold,
                             const void *blocks, int32_t n_blocks, int32_t entries,
                             int64_t *out_ids, double *out_dist, int32_t *out_count,
                             int32_t *needed_entries);
/* The sharded entries behind a cursor (tsh_search_after's semantics; additive since ABI 5).  after_dist / after_id: nq
 * each, the same GLOBAL cursor on every rank, like the queries; -inf is "from the start" and the merged answer equals
 * the cursor-less entries' bit for bit; a NULL cursor array is TSH_E_BAD_ARG.  Every shard emits a block of the rows
 * that can be among ITS first k past the cursor: the floor pass runs on the device as for tsh_search_after, and the few
 * rows whose f32 key cannot tell are appended to the query's device block with their exact sums (a block they do not
 * fit in reports count > entries: the usual overflow protocol).  tsh_merge_candidates_after drops what is at or before
 * the exact (distance, id), orders and cuts: pages concatenate to exactly the list the cursor-less merge would return
 * with k = infinity.  Blocks keep their layout; _progress and _end of the progressive form are the ones above.  A
 * cursor call is never batched, whatever step or TSH_OPT_BATCH_MIN_NQ say: every query is its own f32 tile scan or
 * list scan.  Safe mode runs no floor pass: its blocks are tsh_search_shard's and the merge filters.  A +inf or NaN
 * cursor launches no scan: only rows kept out of the scan can follow it. */
int32_t tsh_search_shard_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                               const double *after_dist, const int64_t *after_id, int32_t entries,
                               void *d_out_blocks, void *stream);
int32_t tsh_search_shard_begin_after(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                                     const double *after_dist, const int64_t *after_id, int32_t entries,
                                     void *d_out_blocks, int32_t step, tsh_shard_stream **out);
int32_t tsh_merge_candidates_after(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k,
                                   double distance_threshold, const double *after_dist, const int64_t *after_id,
                                   const void *blocks, int32_t n_blocks, int32_t entries, int64_t *out_ids,
                                   double *out_dist, int32_t *out_count, int32_t *needed_entries);
/* The sharded entries with a mask HANDLE (tsh_mask_create on the shard handle) in place of the row_mask pointer, and an
 * OPTIONAL cursor (additive since ABI 5).  The pointer entries slice, count and -- for a selective mask -- list the
 * caller's GLOBAL bitmap on the host in every call, on every rank, and the progressive form copies the bitmap up to the
 * shard's end first; these read the handle's device words and list in place: no per-call slice, count, list, upload or
 * bitmap copy happens anywhere in a handle call.
 *   mask        NULL = no filter: the call behaves as the pointer entry with row_mask == NULL.  Otherwise a handle made
 *               for `idx` (tsh_search_sharded_masked: for `shard`); a handle made for another index, or an orphaned
 *               one, is TSH_E_BAD_ARG.  The handle must outlive the call -- for _begin_masked the stream, up to _end:
 *               only the handle is kept, never a copy of a bitmap.
 *   after_dist / after_id   both NULL: no cursor (tsh_search_shard / _begin / tsh_search_sharded).  Both given: nq each,
 *               tsh_search_after's semantics (tsh_search_shard_after / _begin_after / tsh_search_sharded_after).
 *               Exactly one NULL is TSH_E_BAD_ARG.
 * The blocks, and the answer merged from them (tsh_merge_candidates / _after), are those of the pointer entry given the
 * bitmap the handle was made from, zero-extended to the shard's current end: rows appended after tsh_mask_create are
 * not kept, as in tsh_search_masked.  The shard's part of the handle is looked up under the shard's shared lock and
 * rebuilt there if the shard grew; the first scans, an overflow retry with larger blocks, a cursor job's side-list redo
 * and the batched path's listed and dense modes all read it.  Block layout, overflow protocol (count > entries,
 * TSH_E_OVERFLOW with the entry count to retry with), _progress / _end, the batched route and `step`, "a cursor call is
 * never batched", TSH_OPT_EXCHANGE_AHEAD ignored behind a cursor, failure protocol and timeline: the pointer entries'.
 * Every rank makes its own handle from the same GLOBAL bitmap; as with the pointer form, the library does not check
 * that the ranks agree.  In tsh_search_sharded_masked a bad handle is a LOCAL failure like a bad shard handle: the rank
 * stays in the collective and returns its own error, its peers return TSH_E_PEER, the communicator stays usable.
 * Measured on one MI355X (profiles/shard_mask_handle_ab.json, tools/ab_shard_mask_handle.py; one shard handle of
 * 1 M x 768 f32, L2, k = 100, medians, two processes): a lone query behind a keep-1 % mask 104.9 - 107.7 us per call
 * through tsh_search_shard, 33.9 - 34.6 us through tsh_search_shard_masked; a 64-query call behind a keep-50 % mask
 * 587 us by pointer, 493 us by handle. */
int32_t tsh_search_shard_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, tsh_mask *mask,
                                const double *after_dist, const int64_t *after_id, int32_t entries,
                                void *d_out_blocks, void *stream);
int32_t tsh_search_shard_begin_masked(tsh_index *idx, const float *queries, int32_t nq, int32_t k, tsh_mask *mask,
                                      const double *after_dist, const int64_t *after_id, int32_t entries,
                                      void *d_out_blocks, int32_t step, tsh_shard_stream **out);
/* The sharded entries of the plain grouped search (tsh_search_grouped's semantics: no cursor, one row per group; additive
 * since ABI 5; tsh_search_sharded_grouped is with the collective below).  The merged answer is bit for bit the one
 * tsh_search_grouped gives on one un-sharded index over the same rows, the same GLOBAL group_of array, the same mask,
 * tombstones and threshold.  Groups MAY have rows on any number of ranks.
 *   row_mask / mask   GLOBAL, at most one of them: the pointer form, or a handle under tsh_search_shard_masked's rules.
 *   groups      a handle made on THIS shard handle from the GLOBAL array (tsh_groups_create takes shard handles with
 *               global ids).  Every rank makes its own from the same array; as with masks, the library does not check
 *               that the ranks agree.  It travels as `void *`, as in tsh_search_grouped.
 * Blocks: layout and tsh_candidate_block_bytes are unchanged.  A grouped block holds, with their exact sums, the
 * select's candidates over the group HEADS (one row per group by f32 key), the SIDE rows (rows that are not their
 * group's head by f32 key but may be by exact distance) and the quarantined rows that the mask keeps.  No group id
 * travels in a block: the merge looks it up by global id.  A block the side rows do not fit in reports count > entries,
 * the usual overflow protocol.
 * tsh_merge_candidates_grouped is pure host code, no device: group_of / n_group_of is the same global array; an id at
 * or beyond it, or a negative entry, is ungrouped, as in the groups handle.  It is the grouped finaliser over the UNION
 * of all blocks' entries -- the step tsh_search_grouped runs over several devices: order by (distance, id), keep the
 * first entry of every group, cut to k.  Exact for groups that span ranks: every rank's block holds each of its groups'
 * exact best among the rows it may contribute (head and side rows), so the best entry of a group in the union is the
 * group's best overall, and a rank offers at least its k nearest groups, of which no more than k can precede the
 * answer's last.  out_group is nullable; unused slots read id -1, distance NaN, group -1.  A truncated block
 * (count > entries) answers TSH_E_OVERFLOW with *needed_entries, as in tsh_merge_candidates.
 * A grouped sharded call is never batched, whatever step or TSH_OPT_BATCH_MIN_NQ say: every query is its own f32 tile
 * scan or list scan, never the exact path or the fp16 / int8 copies, as for the other grouped jobs.  Safe mode runs no
 * device group passes: its blocks are tsh_search_shard's and the merge does the grouping.
 * Argument errors are tsh_search_grouped's (TSH_E_BAD_ARG): both mask forms at once, NULL `groups`, a groups or mask
 * handle of another index, an orphaned handle.  Trivial cases: with k <= 0 or an empty shard the shard still emits valid
 * empty blocks, so that an exchange is never short a block; they merge to counts of 0.
 * The groups handle is held shared while the search reads it -- the whole call, resp. the progressive search's thread
 * from _begin until its last block is final; the handle must outlive _end, like a mask handle.
 * tsh_search_grouped_stats on the shard handle counts these jobs (searches, side rows, redone, safe mode); no other
 * *_stats moves and tsh_counters keeps its layout.
 * Cost: a grouped shard search costs what tsh_search_grouped costs on the shard handle plus the side rows' append.
 *   Measured on one MI355X (profiles/shard_grouped_ab.json, tools/ab_shard_grouped.py; two ranks sharing the GPU, two
 *   shard handles of 500 k x 768 f32, L2, groups of 8 rows, 64-query calls over the host transport, us per query,
 *   medians): tsh_search_sharded_grouped 458.7 - 460.2 at k = 10 and 458.8 - 460.5 at k = 100, against 468.5 - 473.3 resp.
 *   531.5 - 538.3 for every rank's tsh_search_grouped plus a host gather and a NumPy merge -- not slower, which is all
 *   that is claimed; tsh_search_sharded on the same shards 12 - 13.4 (one batched pass over a reduced copy, where a
 *   grouped call is 64 f32 scans: DESIGN.md, "Grouped search", "Across shards").
 * Out of scope: a cursor, a count or several rows per group across ranks (a group consumed on one rank can reappear from
 * another, and a winning group's second row can lie on a rank where the group is not marked: both need a second
 * exchange); a ticket form; any change to the grouped kernels' rules; the fp16 / int8 copies for grouped jobs. */
int32_t tsh_search_shard_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k, const uint8_t *row_mask,
                                 tsh_mask *mask, void *groups, int32_t entries, void *d_out_blocks, void *stream);
int32_t tsh_search_shard_begin_grouped(tsh_index *idx, const float *queries, int32_t nq, int32_t k,
                                       const uint8_t *row_mask, tsh_mask *mask, void *groups, int32_t entries,
                                       void *d_out_blocks, int32_t step, tsh_shard_stream **out);
int32_t tsh_merge_candidates_grouped(int32_t metric, int32_t dim, const float *queries, int32_t nq, int32_t k,
                                     double distance_threshold, const int32_t *group_of, int64_t n_group_of,
                                     const void *blocks, int32_t n_blocks, int32_t entries, int64_t *out_ids,
                                     double *out_dist, int32_t *out_group, int32_t *out_count,
                                     int32_t *needed_entries);

/* ---- the same exchange from a host without torch (a Dart process per GPU) ------------------------------------
 * RCCL all-gather of the per-shard candidate blocks over xGMI + host merge, behind plain C.  librccl is loaded
 * with dlopen on first use.  One communicator per rank:
 *   rank 0:     tsh_comm_unique_id(id)  -> ship the 128 bytes to the other ranks (any channel the host has)
 *   every rank: tsh_comm_create(id, world, rank, device, &comm)      (collective: returns when all ranks called)
 *   every rank: tsh_search_sharded(shard, comm, queries, ...)        (collective: same queries / nq / k / threshold
 *               on every rank; identical answer on every rank -- the one tsh_search gives on one un-sharded
 *               index over the same rows)
 *   every rank: tsh_comm_destroy(comm)
 * Inside one call the queries travel in groups: this rank's scans of ALL the call's queries run as one pipeline
 * (tsh_search_shard_begin), and every group is all-gathered (device to device) and merged as soon as its blocks
 * are final, while the scans of the later groups go on.  Of every group each
 * rank copies back and merges only its own slice of the queries (world blocks per query); a second, small
 * all-gather hands every slice's final ids / distances to every rank.  (Groups of at most 128 blocks in all -- world x
 * queries -- are merged whole on every rank instead, and the second all-gather does not happen.)
 * Failures: a rank whose own part fails (bad handle, TSH_E_BUSY, a HIP error in its shard search, an allocation)
 * STAYS in the collective, contributes blocks that say so, and returns its error; the other ranks return
 * TSH_E_PEER; the communicator remains usable.  Only a failing all-gather / stream operation (TSH_E_RCCL,
 * TSH_E_HIP from the exchange itself) leaves the ranks out of step: destroy the communicator then.
 * row_mask is GLOBAL.  No reference counterpart (the reference has no distributed compute). */
typedef struct tsh_comm tsh_comm;
#define TSH_COMM_ID_BYTES 128
int32_t tsh_comm_unique_id(void *out_id);
int32_t tsh_comm_create(const void *id, int32_t world, int32_t rank, int32_t device, tsh_comm **out);
/* The same protocol over a transport the host brings (ranks on several nodes, a host without RCCL, tests with
 * several ranks on one GPU): `allgather(user, send, recv, bytes)` must place every rank's `bytes` at
 * recv + rank * bytes on every rank (host memory, synchronous; 0 = ok) -- the one callback in this ABI; it is
 * invoked on the thread that called tsh_search_sharded, never after that call returned.  The candidate blocks
 * then travel device -> host -> callback instead of device -> device. */
typedef int32_t (*tsh_allgather_fn)(void *user, const void *send, void *recv, int64_t bytes);
int32_t tsh_comm_create_host(int32_t world, int32_t rank, int32_t device, tsh_allgather_fn allgather, void *user,
                             tsh_comm **out);
int32_t tsh_comm_destroy(tsh_comm *comm);
int32_t tsh_comm_world(tsh_comm *comm);
/* queries per exchange of tsh_search_sharded; 0 (default) = the library's own schedule.  Calls of up to 128 queries that
 * the shards scan query by query (no rank batches -- TSH_OPT_BATCH_MIN_NQ = 0 on every handle -- or the cost model says
 * scans) go in SHRINKING groups (half of what is left each time, never below what hides an exchange behind the scans that
 * follow -- sized by the bytes a scan of the largest shard reads -- nor below four: 20 queries on 125 k x 768 shards as
 * 10 + 5 + 5), because only the LAST group's exchange is exposed; calls the shards answer on their matrix cores go as ONE
 * group (a group is one batched call per shard).  Beyond 128 queries: 256 per group, 512 from 1024 queries on.  What the
 * ranks know of each other (shard sizes, whether they batch) they tell each other whenever their buffers grow and on every
 * 64th call: a changed option takes that long to reach the schedule.  n > 0: uniform groups of n.  Same value on every rank. */
int32_t tsh_comm_set_group(tsh_comm *comm, int32_t queries_per_exchange);
int32_t tsh_search_sharded(tsh_index *shard, tsh_comm *comm, const float *queries, int32_t nq, int32_t k,
                           double distance_threshold, const uint8_t *row_mask, int64_t *out_ids, double *out_dist,
                           int32_t *out_count);
/* tsh_search_sharded behind a GLOBAL cursor per query (same arrays on every rank): identical answer on every rank -- the
 * one tsh_search_after gives on one un-sharded index over the same rows.  Groups follow the scan schedule above (the
 * shrinking groups), never the one-group batched schedule, on every rank alike and whatever any rank's
 * TSH_OPT_BATCH_MIN_NQ says.  A cursor call exchanges a group when its blocks are FINAL, whatever
 * TSH_OPT_EXCHANGE_AHEAD says: a search whose side list overflowed is redone by the host, so a block whose kernels are
 * enqueued is not yet the block that will be read.  Failure protocol and timeline: tsh_search_sharded's. */
int32_t tsh_search_sharded_after(tsh_index *shard, tsh_comm *comm, const float *queries, int32_t nq, int32_t k,
                                 double distance_threshold, const uint8_t *row_mask, const double *after_dist,
                                 const int64_t *after_id, int64_t *out_ids, double *out_dist, int32_t *out_count);
/* tsh_search_sharded / tsh_search_sharded_after with this rank's mask handle (see tsh_search_shard_masked above): mask
 * NULL = no filter, after_dist / after_id both NULL = no cursor.  Collective like the two; a bad handle on one rank
 * does not leave the ranks out of step. */
int32_t tsh_search_sharded_masked(tsh_index *shard, tsh_comm *comm, const float *queries, int32_t nq, int32_t k,
                                  double distance_threshold, tsh_mask *mask, const double *after_dist,
                                  const int64_t *after_id, int64_t *out_ids, double *out_dist, int32_t *out_count);
/* tsh_search_sharded for the plain grouped search (see tsh_search_shard_grouped above): identical answer on every rank --
 * the one tsh_search_grouped gives on one un-sharded index over the same rows and the same GLOBAL group_of array.
 * row_mask / mask: GLOBAL, at most one; groups: this rank's handle, made on `shard`.  Groups follow the scan schedule
 * (the shrinking groups) on every rank alike, and a group of queries is exchanged only when its blocks are FINAL,
 * whatever TSH_OPT_EXCHANGE_AHEAD says: a grouped job can be redone by the host, as a cursor job can.  Failure protocol
 * and timeline: tsh_search_sharded's.  A bad groups handle (NULL, another index's, orphaned), a bad mask handle or both
 * mask forms at once is a LOCAL failure: the rank stays in the collective and returns its own error, its peers return
 * TSH_E_PEER, the communicator stays usable.  Where only the slice owner merges and a second all-gather hands out ids
 * and distances, every rank fills out_group (nullable) by looking the ids up in its own handle's array: the wire
 * format of the result gather does not change. */
int32_t tsh_search_sharded_grouped(tsh_index *shard, tsh_comm *comm, const float *queries, int32_t nq, int32_t k,
                                   double distance_threshold, const uint8_t *row_mask, tsh_mask *mask, void *groups,
                                   int64_t *out_ids, double *out_dist, int32_t *out_group, int32_t *out_count);

/* Where the time of this rank's tsh_search_sharded calls went: sums over the calls since the communicator was made
 * (or since the last reset).  On the calling thread a call is, group after group,
 *   reserve | pre_enqueue | wait_scan | exchange_wait (= all-gather of the blocks + this rank's slice to the host) |
 *   merge | result_gather | copy_out        (+ retry_scan for groups redone with larger blocks)
 * so these eight add up to call_us but for loop overhead; scan_us runs beside them on the helper thread (group g + 1
 * is scanned while group g is exchanged), and gather_us + slice_d2h_us are the device-side split of exchange_wait_us.
 * A rank that waits for slower peers shows it in gather_us (the all-gather cannot finish before the last rank
 * joins); a rank whose own scans are the bottleneck shows it in wait_scan_us.  No reference counterpart. */
typedef struct tsh_comm_timeline {
  int64_t calls;   /* tsh_search_sharded calls that reached their exchange */
  int64_t queries; /* queries of those calls */
  int64_t groups;  /* exchanges (retried ones count again) */
  int64_t retries; /* groups redone with larger candidate blocks */
  int32_t world;
  int32_t rank;
  int32_t transport; /* 0 RCCL, 1 host callback, 2 a library named by TSH_RCCL_LIB (tests) */
  int32_t reserved;
  double call_us;          /* wall time inside the calls */
  double reserve_us;       /* buffers (+ the agreement all-gather when they grew) */
  double wait_scan_us;     /* calling thread blocked until this rank's scans of the group were done */
  double scan_us;          /* helper thread: tsh_search_shard of the groups (overlaps the previous group's exchange) */
  double exchange_wait_us; /* from issuing the block all-gather until this rank's slice is on the host */
  double gather_us;        /* the all-gather (RCCL: device time on the communicator's stream; every fourth exchange is
                              timed, the sum scaled by exchanges / timed exchanges) */
  double slice_d2h_us;     /* the slice's copy to the host (sampled likewise) */
  double merge_us;         /* host merge of the slice (threshold, order, cut) */
  double result_gather_us; /* every slice's results to every rank: H2D + all-gather + D2H */
  double copy_out_us;      /* into the caller's arrays */
  double retry_scan_us;    /* re-scans of overflowing groups, on the calling thread */
  double pre_enqueue_us;   /* RCCL transport: launching a group's all-gather + copy AHEAD of its blocks, behind a gate
                              the host opens when they are final (the launch's host cost hides behind the scans) */
} tsh_comm_timeline;
int32_t tsh_comm_get_timeline(tsh_comm *comm, tsh_comm_timeline *out, int32_t reset);

int32_t tsh_get_counters(tsh_index *idx, tsh_counters *out);

/* ---- measurement hooks (bench.py / profiles) -----------------------------
 * Average device time in microseconds of the scan kernel alone, measured with
 * HIP events on the library's own stream over `iters` launches of one query. */
int32_t tsh_bench_scan(tsh_index *idx, const float *query, int32_t iters,
                       const uint8_t *row_mask, double *out_avg_us);
/* One real batched search of nq queries, `iters` times: average device time of
 * the two matrix-core passes (sample + filtered) that together score every row
 * once, in microseconds (HIP events on the library's stream), and the
 * algorithmic flop count 2*nq*rows*dim they performed. */
int32_t tsh_bench_batch(tsh_index *idx, const float *queries, int32_t nq, int32_t k, int32_t iters,
                        double *out_avg_gemm_us, double *out_flops);

/* Probes of the pre-filter keys (tests only: tests/test_gpu_bands.py holds every key kernel to the error bound the
 * host claims for it, on rows built to err in one direction).  Single-shard handles.
 * tsh_probe_scan_keys: the single-query scan kernel's f32 ranking key of every row (NaN = row not live) and the
 * band the select step would apply: a row of the true top k has key <= tau * (1 + eps_rel) + delta_abs, where
 * eps_rel = 3 eps and delta_abs = 2 delta * 1.0001 for the per-key bounds |key - exact| <= eps * exact (L2) resp.
 * <= delta (inner product, cosine); exact = sum (q - v)^2, -q.v, -q.v / |v|.
 * tsh_probe_batch_keys: the batched key kernel's (TSH_OPT_BATCH_KERNEL) keys of every row for nq queries, row-major
 * nq x size, and per query 2 * 1.0001 * (the bound on |key - exact|); L2 keys are |q|^2 + |v|^2 - 2 q.v. */
int32_t tsh_probe_scan_keys(tsh_index *idx, const float *query, float *out_keys, float *out_eps_rel, float *out_delta_abs);
int32_t tsh_probe_batch_keys(tsh_index *idx, const float *queries, int32_t nq, int32_t k, float *out_keys,
                             float *out_delta2);
/* The band of the last tsh_probe_batch_keys call (same nq) row by row: the fp16 keys of an L2 / inner-product index are
 * known to alpha |v| + beta each -- the operand roundings act on the products, 2^-10 |q| |v| a row -- and the batched path
 * widens every row's key by its own band (a short row's far less than the longest row's).  out_alpha2[q] = 2 alpha_q,
 * out_beta2[q] = 2 * 1.0001 * beta_q: 2 |key - exact| <= out_alpha2[q] |v| + out_beta2[q] for every row v.  Key kernels
 * and metrics with one band for all rows report alpha = 0 and out_beta2 = out_delta2. */
int32_t tsh_probe_batch_row_band(tsh_index *idx, int32_t nq, float *out_alpha2, float *out_beta2);
/* tsh_probe_scan_f16_keys: the fp16 scan's (TSH_OPT_SCAN_F16) stored key of every row -- the UPPER side key + w of the
 * row's band -- and that band w: |out_keys[i] - out_w[i] - exact_i| <= out_w[i] with exact = |v|^2 - 2 q.v (L2: the
 * common |q|^2 is left out), -q.v, -q.v / |v|.  An error when the index or the query is not eligible for that scan.
 * On an index with dead rows (tombstones, quarantined rows, gaps: TSH_OPT_SCAN_F16_MASKED must allow the scan)
 * out_keys[i] is NaN for every row that is not live; out_w[i] is still the row's band.
 * tsh_probe_scan_keys keeps probing the f32 kernel. */
int32_t tsh_probe_scan_f16_keys(tsh_index *idx, const float *query, float *out_keys, float *out_w);
/* The fp16 scan's own counters (tsh_counters keeps its layout), summed over the shards: out[0] = scans launched over
 * the fp16 copy (dense and masked ones alike), out[1] = of those, queries whose candidate list overflowed and that were redone through the f32 scan,
 * out[2] = rows converted into the copy so far, out[3] = bytes of the copy resident now (part of bytes_resident). */
int32_t tsh_scan_f16_stats(tsh_index *idx, int64_t *out);
/* tsh_probe_scan_i8_keys: the int8 scan's (TSH_OPT_SCAN_I8, which must allow the scan) two sides of every row's
 * ranking key, out_lower[i] <= exact key of row i <= out_upper[i] being what its band claims (single-shard indexes;
 * rows floats each).  On an index with dead rows (tombstones, quarantined rows, gaps: TSH_OPT_SCAN_I8_MASKED must allow
 * the scan) both are NaN for every row that is not live.  For the band test. */
int32_t tsh_probe_scan_i8_keys(tsh_index *idx, const float *query, float *out_lower, float *out_upper);
/* tsh_scan_i8_stats: out[0] scans over the int8 copy (dense and masked ones alike), out[1] queries redone through
 * another scan (survivor list overflow), out[2] rows converted into the copy, out[3] device bytes the copy holds. */
int32_t tsh_scan_i8_stats(tsh_index *idx, int64_t *out);
/* tsh_probe_scan_i4_keys: the 4-bit first pass's (TSH_OPT_SCAN_I4 and TSH_OPT_SCAN_I8, which must both allow it: a dense
 * L2 index) two sides of every row's ranking key, out_lower[i] <= exact key of row i <= out_upper[i] being what its band
 * claims (single-shard indexes; rows floats each).  For the band test. */
int32_t tsh_probe_scan_i4_keys(tsh_index *idx, const float *query, float *out_lower, float *out_upper);
/* tsh_scan_i4_stats: out[0] scans whose 4-bit pass ran in front of the int8 scan, out[1] rows those passes left to the
 * int8 scan (their sum), out[2] rows converted into the 4-bit plane, out[3] device bytes the plane holds, out[4] times the
 * route was denied because too many rows survived, out[5] eligible scans a denial still covers. */
int32_t tsh_scan_i4_stats(tsh_index *idx, int64_t *out);

/* Tuning knobs (no reference counterpart).  TSH_OPT_BATCH_MIN_NQ: when tsh_search /
 * tsh_search_shard answer a multi-query call on the batched matrix-core path:
 * 0 = never; 1 (default) = whenever its estimated cost is below that of nq pipelined
 * single-query scans (on 1 M x 768 rows from two queries on, on 100 k rows from about
 * six); n >= 2 = from n queries per call on.  Results are identical either way. */
#define TSH_OPT_BATCH_MIN_NQ 1
/* TSH_OPT_BATCH_KERNEL: how the batched path forms its pre-filter keys (the f64
 * rerank decides, and each variant's band covers its own error, so results are
 * identical whichever runs):
 *   0  f32 MFMA on the rows as stored;
 *   1  bf16x3: each f32 operand split into bf16 hi + lo, three bf16 MFMAs per
 *      product (error 2^-15 |q||v| on top of the f32 accumulation bound);
 *      costs a second copy of the rows, 4 B per element;
 *   2  f16: operands rounded to fp16 after an exact power-of-two scaling (cosine
 *      rows normalised first), one f16 MFMA per product (error 2^-10 |q||v|);
 *      costs a copy of 2 B per element;
 *   3  (default) auto: f16 for cosine indexes, whose keys are scale-free, for
 *      inner-product indexes (a row's band is its own: alpha |v| + beta) and for L2
 *      indexes while the band's shared term, ~ c (1 + max|v|^2), stays small against
 *      the spacing of the shortest rows' keys (~ 0.1 min|v|): norms a factor 32 apart
 *      are served by f16, norms 2^-6 .. 2^6 by bf16x3; an index whose f16 candidate
 *      lists overflow all the same is moved to bf16x3 for its next 256 batched calls.
 * The copy is built by the first batched search and kept current across appends. */
#define TSH_OPT_BATCH_KERNEL 2
/* TSH_OPT_EXCHANGE_AHEAD (process-wide; idx is ignored and may be NULL; default 0): 1 = tsh_search_sharded over RCCL
 * launches a group's all-gather as soon as the group's scans are ENQUEUED, ordered on the communicator's stream behind
 * the events of the group's last block writers, instead of when the host has seen the blocks final -- the collective's
 * launch (tens of microseconds of host time) then hides behind the scans.  Blocks carry a generation
 * (their header's pad[1]) so that a block of an earlier call is never taken for an answer, and a block the host is
 * still going to redo (ties) asks for a retry like a truncated one.  Measured on one MI355X with 125 k x 768 shards it
 * LOSES 3-6 % (the early packets on the communicator's queue run late), hence off by default;
 * kept for hosts whose collectives are costlier to launch.  Same value on every rank.  tsh_search_sharded_after does not
 * look at it: a cursor search whose side list overflowed is redone by the host, so "enqueued" is not "final" there, and
 * its groups are exchanged when their blocks are final. */
#define TSH_OPT_EXCHANGE_AHEAD 3
/* TSH_OPT_EXACT_SCAN_ROWS (default and maximum 16384; 0 = never): a single-query search that has at most this many
 * rows to look at -- the kept rows of a selective row mask, or all rows of a small index or shard -- computes the exact
 * f64 sums of ALL of them in one launch (the re-rank's arithmetic, one wave per few rows) and selects the k smallest
 * exact distances in a second: the f32 pre-filter has nothing to spare there, and its three dependent dispatches
 * (scan, select, re-rank) are what such a search waits for.  Results are identical either way (the candidates are then
 * exactly the k winners); counted in tsh_counters.exact_scans. */
#define TSH_OPT_EXACT_SCAN_ROWS 4
/* TSH_OPT_EXACT_SELECT (default 1): what follows the exact scan of such a search.  1 = the wide pick: the scan leaves
 * every wave's smallest distance, the k-th smallest of those bounds the k-th distance from above, and one workgroup per
 * 256 rows emits every row at or below the bound -- the k winners plus a few rows that cannot win, no ranking on the
 * device (the finaliser orders and cuts as always); a bound that lets in more rows than the block holds (ties by the
 * hundred) is finished by the one-workgroup select, and searches with fewer than 16 k rows to look at take that select
 * directly.  0 = always the select (round 5: exactly min(k, live rows) entries, one compute unit, 9-17 us for 2 k-10 k
 * rows).  Results are identical. */
#define TSH_OPT_EXACT_SELECT 5
/* TSH_OPT_BATCH_HUB (default 0): 1 = batched searches of an L2 / inner-product index on fp16 keys also score the index's
 * HUB rows densely -- the 4096 rows whose norm alone puts them near every query: the shortest (L2) resp. the longest
 * (inner product), kept as a gathered fp16 copy -- and take the smaller of two thresholds: the sample's (an estimate,
 * verified) and the hub rows' k-th smallest key (a bound by construction).  Measured on one MI355X it thins the key
 * kernel's epilogue on corpora whose neighbours are their short rows (key passes - 3 to - 5 %) and costs the call as
 * much as it saves: off unless a host knows its corpus to be that kind.  Results are identical. */
#define TSH_OPT_BATCH_HUB 6
/* TSH_OPT_BATCH_GROUP (default 1): 1 = the fp16 copy of an L2 / inner-product index that batched searches score holds
 * its rows ordered by norm inside blocks of 8192 consecutive rows (the rows every query passes -- the short ones under
 * L2, the long ones under inner product -- then share a few tiles of the key kernel instead of slowing a quarter of
 * them down); 0 = in row order.  Results are identical either way; the copy is rebuilt by the next batched search
 * after a change. */
#define TSH_OPT_BATCH_GROUP 7
/* TSH_OPT_SCAN_F16 (default 1): whether a dense single-query scan -- no caller mask, no tombstones -- reads an fp16
 * copy of the rows instead of the rows themselves: half the HBM bytes per query.  0 = never; 1 = auto: shards whose row
 * store is larger than the 256 MiB Infinity Cache (below that a scan is not bandwidth-bound); 2 = every eligible
 * scan whatever the size (tests, A/B runs).  Eligible: rows of at least 256 elements, a multiple of 8, index and
 * query inside the error model.  The copy (2 B per element, scaled by a power of two) is built by the first such
 * search and kept current lazily: appended rows are converted in front of the next scan; an overwrite, a
 * reallocation or a change of the scale rebuild it.  A device too full for it scans f32.  Keys carry a per-row band
 * alpha |v| + beta; a query whose candidate list overflows on them is redone through the f32 scan, and two such queries
 * in a row move the index's next 256 eligible scans to f32.  Results are identical either way. */
#define TSH_OPT_SCAN_F16 8
/* TSH_OPT_SCAN_F16_MASKED (default 1): the same for single-query tile scans that are NOT dense -- behind a caller's row
 * mask (pointer or handle; masks selective enough for the list scan or the exact path keep those), tombstones,
 * quarantined rows or gaps of absent ids: only the live rows' halves are read, and a query redone through the f32 scan
 * keeps its mask.  0 = never; 1 = auto: shards whose row store is larger than 256 MiB; 2 = every eligible masked scan
 * whatever the size (tests, A/B runs).  TSH_OPT_SCAN_F16 = 0 switches both routes off; its value 2 does not force this
 * one.  Results are identical either way; the scans count in tsh_scan_f16_stats. */
#define TSH_OPT_SCAN_F16_MASKED 9
/* TSH_OPT_SCAN_I8 (default 1): whether a dense single-query scan -- no caller mask, no tombstones, no quarantined rows or
 * gaps -- runs as a COARSE first pass over an int8 copy of the rows (a quarter of the f32 bytes; a scale per row, built
 * lazily by the first such scan and kept current like the fp16 copy), whose survivors -- the rows whose proven lower
 * side is at or below the k-th smallest tile minimum of proven upper sides, at most 4096 of them -- are answered by the
 * exact scan + select.  0: never (the library then behaves exactly as without the option), 1: shards whose rows exceed
 * 256 MiB, 2: every eligible scan whatever the size (tests, A/B runs).  A survivor list that overflows is redone through
 * the f32 scan; two in a row keep the shard's next 256 eligible scans off the route.  Results are identical either way;
 * the scans count in tsh_scan_i8_stats. */
#define TSH_OPT_SCAN_I8 10
/* TSH_OPT_SCAN_STREAMS (default 0): on how many streams the single-query scans of overlapping queries (a multi-query
 * call, several tickets out) run.  On one in-order stream the compute units empty at the end of every scan and nothing
 * refills them until the next one starts: half a wave's life per scan, a share  tile bytes x waves per CU x CUs / 2 /
 * bytes the scan moves  of it.  0 = by that share: two streams for every scan of fewer than 6144 tiles (as ever) and for
 * bigger scans whose share is at least 4.5 % -- a big shard's scans over its int8 or fp16 copy; the f32 scan of 1 M x 768
 * rows (3 %) keeps one.  1 = always one stream; 2 = two streams whenever queries overlap (tests, A/B runs).  On two
 * streams consecutive scans run side by side: tsh_counters.scan_us_sum stays the sampled launch's OWN duration, which is
 * then about twice its share of the HBM time -- it is not rescaled.  Results are identical either way.
 * (Number 11 is not assigned: the suite pins it as an unknown id.) */
#define TSH_OPT_SCAN_STREAMS 12
/* TSH_OPT_SCAN_I8_MASKED (default 1; additive since ABI 5): the int8 coarse pass of TSH_OPT_SCAN_I8 for single-query tile
 * scans that are NOT dense -- behind a caller's row mask (pointer or handle; masks selective enough for the list scan or
 * the exact path keep those), tombstones, quarantined rows or gaps of absent ids: only the live rows' bytes are read,
 * dead tiles never count towards the threshold, and fewer live rows than k come back as exactly those.  0 = never; 1 =
 * auto: shards whose row store is larger than 256 MiB, unless the fp16 masked route was forced (TSH_OPT_SCAN_F16_MASKED =
 * 2: a forced value beats an automatic one); 2 = every eligible masked scan whatever the size (tests, A/B runs).
 * TSH_OPT_SCAN_I8 = 0 switches both int8 routes off; its value 2 does not force this one.  A survivor list that
 * overflows is redone behind the same mask through the fp16 masked scan where that applies, the f32 scan otherwise; two
 * in a row keep the shard's next 256 eligible scans off the int8 routes.  Results are identical either way; the scans
 * count in tsh_scan_i8_stats.  Measured on one MI355X, 1 M x 768, 64-query calls (profiles/scan_i8_masked_ab.json): one
 * tombstone 228.3 -> 123.7 us per query, a keep-50 % mask 123.9 -> 66.9 (pointer) and 123.2 -> 66.3 (handle) against the
 * fp16 masked scans, spread at most 2.5 %: hence 1 by default. */
#define TSH_OPT_SCAN_I8_MASKED 13
/* TSH_OPT_SCAN_I4 (default 1; additive since ABI 5): a 4-bit first pass in front of the coarse int8 scan of a dense L2
 * single-query scan.  It reads a plane of the int8 copy's high nibbles -- half a byte per element -- and one float per
 * row, bounds every row's key from below, and the int8 scan then reads only the rows whose lower bound does not exceed
 * the k-th smallest upper bound: on corpora whose norms differ about a tenth of the rows.  0 = never; 1 = auto: L2 shards
 * whose row store is larger than 1400 MiB (smaller ones lose: the pass has a fixed cost of three launches); 2 = every eligible scan whatever the size (tests, A/B runs).  It runs only
 * where the dense int8 route runs (TSH_OPT_SCAN_I8) and never behind a mask, tombstones, quarantined rows or gaps, for
 * cursor, count or grouped searches, or for inner product and cosine.  Two scans in a row that leave more than 32 % of the
 * rows to the int8 scan keep the shard's next 256 eligible scans on the plain int8 route; repeated denials double, up to
 * 65 536 scans (the plane -- half a byte per element -- stays resident meanwhile).  Results are identical either way; the scans count in tsh_scan_i4_stats.  Measured on one MI355X, 1 M x 768,
 * norms U(0.5, 2), k = 100 (profiles/scan_i4_bench_ab.json): a step of bench.py 0.1138 -> 0.0927 ms, five processes a side,
 * spreads 0.0006 and 0.0004 ms; unit-norm rows, where the pass prunes nothing and is denied after two scans: no difference.
 * The 32 % and the 1400 MiB are measured break-evens less their spreads (tools/ab_scan_i4.py, same file).  Hence 1 by default. */
#define TSH_OPT_SCAN_I4 14
/* TSH_OPT_TEST_HOOKS (process-wide; idx is ignored and may be NULL): value TSH_TEST_HOOKS_MAGIC switches the
 * library's TEST hooks on, 0 off.  Only then does it read the environment variables that change what it loads or make
 * it fail on purpose -- TSH_RCCL_LIB (a stand-in for librccl: tests/fake_rccl), TSH_TEST_FAIL_ALLOC_OVER (device
 * allocations fail), TSH_SHARDS_SHARE_DEVICES (several shards of one handle on one GPU).  Without the call those
 * variables change nothing: an embedded database must not be steerable through its environment.  Experiment
 * switches (kernel shapes, stream layouts) exist in probe builds only (-DTSH_PROBES).  A release build reads
 * LOCAL_WORLD_SIZE, TSH_BLOCKING_WAIT, TSH_HOST_THREADS (how the host side waits: DESIGN.md appendix B) and
 * TSH_TRACE_BATCH (stderr diagnostics), nothing else. */
#define TSH_OPT_TEST_HOOKS 1000
#define TSH_TEST_HOOKS_MAGIC 0x7465737468ll /* "testh" */
int32_t tsh_index_set_option(tsh_index *idx, int32_t option, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* TOSTORE_HIP_H */
