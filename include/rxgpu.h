/*
 * rxgpu — C-ABI of the MI355X (gfx950) engines behind Reindexer's float_vector / ft_fast index plugins.
 *
 * This header is the drop-in boundary: plain C types, caller-allocated outputs, int return codes
 * (0 = ok, negative = rxgpu_status), no C++/torch types.  Nothing in the reference knows this ABI; it is
 * what the GPU `Map` policy of HnswIndexBase<Map> (cpp_src/core/index/float_vector/hnsw_index.h:16-57) and
 * the GPU branch of Selector<IdCont>::mergeResults (cpp_src/core/ft/ft_fast/selecterimpl.h:611-628) bind.
 * Each entry point cites the reference interface it stands in for.  See INTEGRATION.md for the binding.
 *
 * Conventions
 *   - "row" = internal index of a vector inside one index (the reference's `idx` in bruteforce.cc / `tableint`
 *     in hnswalg.h).  Labels (FloatVectorId = rowId<<32 | arrayIdx) never cross this boundary: the host Map
 *     owns the row->label table exactly like the reference owns it inside its AoS rows (bruteforce.h:47-48).
 *   - Distances are "smaller is better": L2 -> squared distance, IP -> -dot, cosine -> -dot * inv_norm[row]
 *     (hnswlib.h:147-165,192-197).  They are bit-identical to the reference's AVX-512 path for every dim.
 *   - All functions are thread-safe for concurrent searches on one index (the reference's read path is
 *     re-entrant under the namespace shared lock); mutations require external exclusion (namespace write lock).
 *   - *_device variants take device pointers and a hipStream_t (as void*), enqueue work and return without
 *     synchronising; everything else synchronises before returning.
 */
#ifndef RXGPU_H
#define RXGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RXGPU_ABI_VERSION 2

typedef enum rxgpu_status {
	RXGPU_OK = 0,
	RXGPU_ERR_PARAMS = -3,    /* reindexer errParams (type_consts.h:139-148) */
	RXGPU_ERR_LOGIC = -4,     /* reindexer errLogic */
	RXGPU_ERR_NOMEM = -5,     /* std::runtime_error("Not enough memory ...") in bruteforce.cc:15,90 */
	RXGPU_ERR_DEVICE = -6,    /* HIP runtime failure; text in rxgpu_last_error() */
	RXGPU_ERR_NOTFOUND = -7,
	RXGPU_ERR_OVERFLOW = -8   /* caller-provided output buffer too small; required size reported */
} rxgpu_status;

typedef enum rxgpu_metric { RXGPU_METRIC_L2 = 0, RXGPU_METRIC_IP = 1, RXGPU_METRIC_COSINE = 2 } rxgpu_metric; /* core/enums.h:101 VectorMetric */

typedef struct rxgpu_index rxgpu_index; /* one float_vector index shard resident on one GPU */

/* Thread-local text of the last failure on the calling thread. */
const char* rxgpu_last_error(void);
int rxgpu_abi_version(void);
/* Number of visible HIP devices; <0 on runtime failure. */
int rxgpu_device_count(void);
/* Fills name with the gcnArchName of `device` ("gfx950:..."), mirrors the SIMD-level log line of hnsw_index.cc:25-44. */
int rxgpu_device_arch(int device, char* name, size_t cap);

/* ---------------------------------------------------------------------------------------------------------
 * Vector storage (device mirror of BruteforceSearch / HierarchicalNSW row storage)
 * ------------------------------------------------------------------------------------------------------- */

/* BruteforceSearch::BruteforceSearch(metric, dim, maxElements)  bruteforce.cc:11-18.
 * Allocates capacity * row_stride floats of HBM on `device` (row_stride = dim rounded up to 4 floats; ask rxgpu_index_row_stride rather than
 * compute it: RXGPU_ROW_ALIGN, an experiment of rxgpu_capi.hip that is no part of this ABI, enlarges it). */
int rxgpu_index_create(int metric, uint32_t dim, uint64_t capacity, int device, rxgpu_index** out);
void rxgpu_index_destroy(rxgpu_index* h);

/* The same index row-range SHARDED over several GPUs of this process (BASELINE configs[3]: the Map owns a device list; `devices` may
 * repeat a device — several shards on one GPU).  Shard s holds the global rows [s * shard_rows, (s + 1) * shard_rows), shard_rows =
 * ceil(capacity / n_devices) rounded up to 32.  The handle is used like any other with rxgpu_index_upload_rows (no holes: first_row <= count)
 * / move_row / truncate / count / capacity / device_bytes, rxgpu_search_knn, rxgpu_search_knn_subset, rxgpu_search_range,
 * rxgpu_search_range_subset and rxgpu_distances: rows in and out are GLOBAL rows, results are the single-device results bit for bit
 * (per-shard exact lists merged under (dist, global row), i.e. BruteforceSearch's scan order, bruteforce.cc:103-127), every shard's
 * kernels run concurrently on their own device.  The capacity is fixed (create a new index to grow); device-pointer entry points,
 * bitmap filters, SQ8, streaming sessions and profiling are single-device only and return RXGPU_ERR_LOGIC here.
 * HNSW over shards (SURVEY 8e "HNSW": "per-shard independent graphs + the same all-gather merge"): every shard holds the graph of ITS rows —
 * rows, graph, patches and delete marks go to the rxgpu_index_shard(h, s) handles (local row ids), each of which may hold any number of rows
 * up to rxgpu_index_shard_rows — and rxgpu_hnsw_search_knn / rxgpu_hnsw_search_range / rxgpu_hnsw_read_* on the sharded handle fan out:
 * every shard runs HierarchicalNSWImpl::SearchKnn (hnswalg.h:1988-2012) over its graph concurrently, the per-shard results stay in HBM and
 * meet in the same ncclAllGather + (dist, global row) merge as brute force (k <= 64; host merge above that or in host mode).  The merged
 * list of a query = the k best of the union of the per-shard results, sorted, rows GLOBAL (shard * shard_rows + local row). */
int rxgpu_index_create_sharded(int metric, uint32_t dim, uint64_t capacity, uint32_t n_devices, const int* devices, rxgpu_index** out);
uint32_t rxgpu_index_shard_count(const rxgpu_index* h);   /* 0 for an unsharded index */
uint64_t rxgpu_index_shard_rows(const rxgpu_index* h);
/* How SearchKnn's per-shard lists meet (north_star: "RCCL all-gather of per-shard top-k over xGMI"): 1 = on the devices — the index owns one
 * RCCL communicator over its distinct devices (ncclCommInitAll at creation), each search is the shards' scans, ONE ncclAllGather of
 * kk x 8 B x nq per shard on the shards' streams, the (dist, global row) merge kernel on the first device and one D2H copy; 0 = on the host
 * (RXGPU_SHARD_MERGE=host in the environment at creation: D2H per shard + host merge — also what range searches, pre-filtered searches and
 * kk > 64 use in either mode); -1 = not a sharded index.  RCCL is opened when the first sharded index asks for it (dlopen: a single-GPU
 * deployment does not need the library); if it is missing or the communicator cannot be built (no peer access, no /dev/shm, ...) the index is
 * still created, in host mode — one line on stderr, and rxgpu_index_shard_merge_note says why ("" in device mode). */
int rxgpu_index_shard_merge_mode(const rxgpu_index* h);
const char* rxgpu_index_shard_merge_note(const rxgpu_index* h);
uint32_t rxgpu_index_shard_ranks(const rxgpu_index* h);         /* RCCL ranks = distinct devices of the shard list (0 in host mode) */
uint64_t rxgpu_index_shard_collectives(const rxgpu_index* h);   /* all-gathers issued so far (tests / bench assert the path that ran) */
/* Shard s as an ordinary single-device index, for filling it in place (rxgpu_index_adopt_device_rows with memory of THAT device; the
 * sharded handle then takes the row counts over with rxgpu_index_shard_sync_count: full shards, then at most one partial, then empty). */
rxgpu_index* rxgpu_index_shard(rxgpu_index* h, uint32_t s);
int rxgpu_index_shard_sync_count(rxgpu_index* h);
/* One row back to the host (and its 1/|row| for cosine; out_inv_norm may be NULL): the cross-device half of a sharded swap-delete. */
int rxgpu_index_download_row(rxgpu_index* h, uint64_t row, float* out_row, float* out_inv_norm);

/* BruteforceSearch::ResizeIndex  bruteforce.cc:88-101 (contents preserved; shrinking below count is an error). */
int rxgpu_index_reserve(rxgpu_index* h, uint64_t capacity);

/* Device side of AddPointNoLock (bruteforce.cc:44-64): copy n host rows (packed [n][dim]) to rows
 * [first_row, first_row+n) and their 1/|row| coefficients (cosine only, may be NULL otherwise; the host computes
 * them exactly as DistCalculator::AddNorm does, hnswlib.h:80-92).  count becomes max(count, first_row+n). */
int rxgpu_index_upload_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const float* rows, const float* inv_norms);

/* Zero-copy alternative: adopt caller-owned device memory (e.g. a torch tensor) as the row storage.
 * d_rows: [n][row_stride] floats, row_stride >= dim, row_stride % 4 == 0, 16-byte aligned; d_inv_norms: [n] floats, or NULL
 * where the metric is not cosine.  RXGPU_ERR_PARAMS for a row_stride or a d_rows that breaks these rules and for cosine without d_inv_norms.
 * Only the first dim floats of a row are data.  The floats between dim and row_stride, and whatever lies in front of row 0 or behind row
 * n - 1 (of the rows and of the norms), are unspecified and never read as data: they may hold anything, NaN included, and no result
 * depends on them.  Row offsets are 64-bit: n * row_stride may exceed 2^32 floats (row_stride = 2^20 with n = 4160 is tested), n itself
 * stays below 2^32 - 1.  Every search entry point gives, over such storage, the counts, rows and distance bits it gives over an owned
 * index with the same rows (tests/test_gpu_row_layout.py).  A second adoption replaces the first and drops everything derived from it.
 * The caller keeps ownership and must keep the memory alive and unchanged while adopted; rxgpu_index_upload_rows, rxgpu_index_move_row and
 * rxgpu_index_reserve return RXGPU_ERR_LOGIC on adopted storage. */
int rxgpu_index_adopt_device_rows(rxgpu_index* h, const void* d_rows, uint64_t n, uint32_t row_stride, const void* d_inv_norms);

/* Device side of RemovePoint's swap-with-last (bruteforce.cc:70-86): copy row `from` over row `to` (incl. norm). */
int rxgpu_index_move_row(rxgpu_index* h, uint64_t from, uint64_t to);
/* Set the number of live rows (after a swap-delete, or Reset()). */
int rxgpu_index_truncate(rxgpu_index* h, uint64_t count);

uint64_t rxgpu_index_count(const rxgpu_index* h);
uint64_t rxgpu_index_capacity(const rxgpu_index* h);
uint32_t rxgpu_index_dim(const rxgpu_index* h);
uint32_t rxgpu_index_row_stride(const rxgpu_index* h);
int rxgpu_index_metric(const rxgpu_index* h);
int rxgpu_index_device(const rxgpu_index* h);
/* HBM bytes held by the index (AllocatedMemSize analogue, bruteforce.h:41-44). */
uint64_t rxgpu_index_device_bytes(const rxgpu_index* h);

/* ---------------------------------------------------------------------------------------------------------
 * Brute-force search (BruteforceSearch::SearchKnn / SearchRange)
 * ------------------------------------------------------------------------------------------------------- */

/* Exact top-kk of each of nq queries under the total order (dist, row) ascending — the order in which the
 * reference's (dist,label) max-heap evicts, with row standing in for label (bruteforce.cc:103-127).
 * queries: host [nq][dim] (cosine: already normalised by the caller, hnsw_index.cc:166-171).
 * out_dist/out_row: host [nq][kk]; out_count[q] = min(kk, count).
 * The GPU Map asks for kk = k+1 so it can detect a distance tie straddling the k-th boundary and replay the
 * reference's admission rule (strict `dist < worst`, bruteforce.cc:121) with rxgpu_search_range(inclusive = 1). */
int rxgpu_search_knn(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, float* out_dist, uint32_t* out_row,
					 uint32_t* out_count);

/* internal row -> row id (label >> 32, FloatVectorId::RowId) table kept beside the rows for consumers on the device: the hybrid fusion
 * translates the scan's rows there.  Rows [first_row, first_row + n); the table is sized by the index capacity.  The device pointer
 * (int32 [capacity]) or NULL when nothing was uploaded. */
int rxgpu_index_upload_row_ids(rxgpu_index* h, uint64_t first_row, uint64_t n, const int32_t* row_ids);
const void* rxgpu_index_row_ids_device(const rxgpu_index* h);
/* One host query searched with the result LEFT IN HBM (the hybrid query's KNN half): the search is enqueued on a stream of the
 * index and the call returns without waiting; *d_dist / *d_row ((dist, row) best first, *entries of them) and *d_count (device uint32)
 * are buffers of the index that hold this result until the CALLING THREAD's next resident search on it (every thread has buffers and a
 * stream of its own there); *stream is the stream it runs on — a consumer
 * (rxgpu_hybrid_fuse_resident) orders itself behind it on the device.  kk in [1, 128]. */
int rxgpu_search_knn_resident(rxgpu_index* h, const float* query, uint32_t kk, void** d_dist, void** d_row, void** d_count, void** stream,
							  uint32_t* entries);
/* Diagnostics: how many threads hold a resident context (stream + result buffers) on the index right now.  A thread that ends gives its
 * context back to the index's pool, so the number follows the LIVE searching threads, not every thread that ever searched. */
uint32_t rxgpu_index_resident_contexts(rxgpu_index* h);
/* Same, device-resident in/out on `stream` (hipStream_t); d_out_count may be NULL.  No synchronisation.
 * A single query (nq == 1) on an index of at least 1 GiB of f32 rows is served by default from a bf16 shadow of the rows (2 bytes per
 * element read instead of 4; the survivors of a rigorous rounding bound are re-scored by the exact f32 kernels: the same rows and distance
 * bits).  The shadow costs +2 bytes per element of HBM and is built by the first such call on the index (about one pass over the rows, as
 * the first call with two or more queries always did), then kept up to date by upload_rows / move_row / truncate; when it does not fit, or
 * a row has a NaN / infinite norm, the f32 scan serves the query as before.  RXGPU_SCAN_BF16 (environment, read per call): unset =
 * automatic, 0 = always the f32 paths, 1 = the pruned scan for up to 8 queries at any size; RXGPU_SCAN_BF16_MIN_BYTES moves the 1 GiB. */
int rxgpu_search_knn_device(rxgpu_index* h, const void* d_queries, uint32_t nq, uint32_t kk, void* d_out_dist, void* d_out_row,
							void* d_out_count, void* stream);
/* The decision above as a pure function (no device is touched): 1 when a call with nq queries on an index of rows x dim f32 rows takes the
 * bf16-pruned scan under the current environment.  shadow_available: the bf16 shadow fits in HBM; stats_finite: no row has a NaN or
 * infinite norm (both are facts the index learns on the device). */
int rxgpu_scan_policy(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite);
/* Which scan such a call takes: 0 the f32 paths, 1 the bf16-pruned scan, 2 the int8-pruned scan (no device is touched).  The int8 tier
 * refines a call the automatic mode accepts (RXGPU_SCAN_BF16 unset): a single query on an index of at least 1 GiB of f32 rows
 * (RXGPU_SCAN_I8_MIN_BYTES moves it) with 128 < dim <= 1024 is pruned over an int8 shadow of the rows (1 byte per element read, +1 byte per
 * element and +8 bytes per row of HBM, built by the first such call; the bf16 shadow is then not built for single queries) under a per-row
 * bound that is proven, not tuned: the same rows and distance bits.  RXGPU_SCAN_I8 (environment, read per call): unset = automatic, 0 = this
 * tier off, 1 = forced for up to 8 queries at any size; RXGPU_SCAN_BF16=0 and =1 both win over it.  shadow_available stands for the shadow of
 * either tier.  Tier 2 names the integer-shadow chain; rxgpu_scan_i6 names the shadow it reads. */
int rxgpu_scan_tier(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite);
/* 1 when such a call (whole index, no row list) reads the 6-bit shadow instead of the int8 one (no device is touched): the same chain, the
 * same bound and the same result bits from 0.75 bytes per element, behind a seed pass over a strided sample of the rows (+0.75 bytes per
 * element and +8 bytes per row of HBM, built by the first call that takes it; 128 < dim <= 1024).  RXGPU_SCAN_I6 (environment, read per
 * call): 0 = off, 1 = forced for up to 8 queries at any size, unset = automatic: a call the automatic rules give to tier 2, on an index of at
 * least 16 GiB of f32 rows (RXGPU_SCAN_I6_MIN_BYTES moves it).  RXGPU_SCAN_BF16 = 0 / 1 and RXGPU_SCAN_I8 = 0 / 1 win over
 * it: RXGPU_SCAN_I8=1 means the int8 shadow, exactly.  rxgpu_scan_tier does not know the variable and keeps its answers.  i6_available: the
 * 6-bit shadow fits in HBM (when it does not, the int8 shadow serves the call). */
int rxgpu_scan_i6(uint64_t rows, uint32_t dim, uint32_t nq, int i6_available, int stats_finite);
/* Candidates the last pruned single-query search through rxgpu_search_knn (or rxgpu_search_knn_subset / _bitmap / _lists) nominated for the exact re-score, and the capacity of their list
 * (count > cap: the list overflowed, or the query had no finite bound, and the exact scan answered).  A range call the int8 tier served
 * (rxgpu_scan_tier_range) records its candidates and the size of its list the same way.  Recorded only while profiling is enabled
 * (rxgpu_profile_enable). */
int rxgpu_index_last_candidates(const rxgpu_index* h, uint32_t* out_count, uint32_t* out_cap);
/* Test instrumentation: copies a named internal buffer of a single-device index to the host.  Reads only - nothing is built, invalidated or
 * changed.  *out_bytes is always set to the size needed; RXGPU_ERR_OVERFLOW when cap_bytes is smaller (out may be NULL then),
 * RXGPU_ERR_PARAMS for an unknown name or a sharded handle (inspect its rxgpu_index_shard handles), RXGPU_ERR_LOGIC when the buffer does
 * not exist (a shadow that is not built or is stale, no pruned call recorded, a name the tier or the metric does not have).
 * Derived data, for the count rows the index holds:
 *   "stats"      5 uint32: bits of max |x|^2, of max (|x| inv_norm)^2 (cosine), 1 once a non-finite row was seen, bits of max e^2 and of
 *                max (e inv_norm)^2 (cosine) of the int8 shadow
 *   "row_sq"     [count] float |x|^2 (L2 only)
 *   "codes_i8"   [count][dim rounded up to 256] int8 codes          "side_i8"  [count] float pairs {s_r, e_r}
 *   "rows_bf16"  [count][dim rounded up to 64] bf16 words, ROW-MAJOR whatever layout the shadow has on the device
 *   "codes_i6"   [count][dim rounded up to 256] bytes u = code + 32 (0 in the pad), ROW-MAJOR: de-tiled on the host          "side_i6"  as "side_i8"
 *   "stats_i6"   3 uint32: bits of max e^2 and of max (e inv_norm)^2 (cosine) of the 6-bit shadow, 1 once a non-finite e was seen
 * The last single-query search a pruned chain answered while profiling was enabled (recorded with rxgpu_index_last_candidates; the
 * snapshot is what that chain left in its buffers and is valid UNTIL THE NEXT CALL ON THE INDEX, which may reuse them):
 *   "pruned_values"     [n] float: the lower bound lo (int8 tier) or the approximate distance (bf16 tier) per row - per LIST POSITION when
 *                       the search ran over a row list (n = its entries)
 *   "pruned_margin", "pruned_q_sq"   1 float each: what knn_filter_approx adds to T; |q|^2
 *   "pruned_qinfo"      int8 tier: 2 floats {s_q, |q| rounded up}       "pruned_qplanes"  int8 tier: [2][dim rounded up to 256] int8 (h, then l)
 *   "pruned_top"        kk floats (the merged list of the pruning scan, ascending; its last entry is T) and 1 uint32, the entries it holds
 *   "pruned_cand_rows"  [min(candidates, capacity)] uint32 rows the filter nominated, in no particular order
 *   "pruned_emit_cnt"   int8 tier over every row, emitting scan: [4 x workgroups of the scan] uint32, the entries wavefront w emitted
 *   "pruned_emitted"    ... and [n] pairs {float lo, uint32 row}: the wavefronts' segments back to back (knn_emit_plan.h), segment w valid
 *                       up to its count, rows ascending
 *   "pruned_seed"       6-bit front: as "pruned_top", the merged list of the seed pass (its last entry is T_seed) */
int rxgpu_index_inspect(rxgpu_index* h, const char* what, void* out, uint64_t cap_bytes, uint64_t* out_bytes);
/* Test instrumentation: runs one merge kernel of the single-query KNN chains for one query over host arrays (copied to the device, the result
 * copied back; nothing is kept).  dist / row: the pairs; a row of 0xFFFFFFFF is an empty slot.  what =
 *   0  knn_merge_lists over n SORTED lists of kk entries each (dist, row: [n][kk], lists padded with empty slots); kk <= 128
 *   1  the candidate branch of knn_merge_final over n pairs in any order; kk <= 64
 *   2  the insertion fold (knn_merge) over the same n pairs; kk <= 64
 * out_dist / out_row: [kk], ascending by (distance, row) and padded with +inf / 0xFFFFFFFF; *out_count: the entries found.  *out_path: 1 when
 * a selection answered, 0 when an insertion merge did (always 0 for what = 2). */
int rxgpu_knn_merge_probe(int device, int what, const float* dist, const uint32_t* row, uint32_t n, uint32_t kk, float* out_dist, uint32_t* out_row,
						  uint32_t* out_count, int* out_path);

/* ---- Pre-filtered brute force: the caller side of `WHERE cond AND KNN(...)` -------------------
 * The reference evaluates such a query by taking the KNN result and filtering it on the host (selectLoop,
 * nsselecter.cc:841-875); only HNSW can stream more candidates (knn_streaming_index_iterator.cc).  Here the rows that
 * passed `cond` are handed to the scan, which then reads ONLY those rows: the result is exactly what
 * BruteforceSearch::SearchKnn (bruteforce.cc:103-127) returns over an index that holds just the allowed rows —
 * same distance bits, same (dist, row) order — and HBM traffic shrinks with the selectivity of the filter.
 *
 * rxgpu_search_knn_subset: row_ids = host [n_ids], strictly increasing internal rows (the shape of the selector's
 *   sorted IdSet, core/idset.h); best for selective filters (4 bytes per allowed row on the wire).
 * rxgpu_search_knn_bitmap: allowed_words = host [n_words >= ceil(count / 32)], bit (r % 32) of word r / 32 set = row r
 *   allowed (bits at and above `count` are ignored); expanded to the row list on the device; best for dense filters
 *   (count / 8 bytes on the wire).  *out_allowed (optional) = number of allowed rows.
 * Output layout as rxgpu_search_knn: host [nq][kk], out_count[q] = min(kk, allowed rows); any kk.
 * Errors: RXGPU_ERR_PARAMS for an unsorted / out-of-range list or a short bitmap.
 * Which scan serves them: the f32 gather scan (knn_scan_subset) unless rxgpu_scan_tier_subset() says 2 for the call; then the int8 shadow of
 * rxgpu_scan_tier is read for the listed rows (1 byte per element instead of 4) and the exact kernels re-score the survivors of its bound:
 * the same rows and distance bits.  The first such call on an index builds the shadow. */
int rxgpu_search_knn_subset(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* row_ids, uint64_t n_ids,
							float* out_dist, uint32_t* out_row, uint32_t* out_count);
int rxgpu_search_knn_bitmap(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* allowed_words,
							uint64_t n_words, float* out_dist, uint32_t* out_row, uint32_t* out_count, uint64_t* out_allowed);
/* Which scan a search over a row list takes (rxgpu_search_knn_subset / _bitmap / _subset_device / _lists and their per-shard calls): 0 the
 * f32 subset scan, 2 the int8-pruned subset scan (no device is touched; the bf16 tier has no subset form).  n_ids = entries of the list,
 * kk = min(kk, n_ids) of the call.  0 whenever RXGPU_SCAN_BF16 is 0 or 1, RXGPU_SCAN_I8 is 0, the shadow is not available, the dimension
 * is outside 128 < dim <= 1024, kk > 64 or the list is empty.  Otherwise RXGPU_SCAN_I8=1 forces 2 for up to 8 queries at any size, and the
 * automatic rule (RXGPU_SCAN_I8 unset) gives 2 for a single query on an index without a NaN / infinite row norm when the LISTED rows hold
 * at least RXGPU_SCAN_I8_SUBSET_MIN_BYTES of f32 data (n_ids * dim * 4): an index that only sees selective filters never builds the shadow.
 * The default of that variable is the maximum value until the crossover against the f32 subset scan is measured (never below 1 GiB then):
 * without the variable the automatic rule answers 0 and the tier is used only where RXGPU_SCAN_I8=1 forces it.  The environment is read
 * per call. */
int rxgpu_scan_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, int shadow_available, int stats_finite);

/* ---- IVF-Flat: faiss::IndexIVFFlat::search as IvfIndex drives it (ivf_index.cc:355-372) in ONE call ----------
 * rxgpu_index_set_lists: the inverted lists over this index's rows as CSR — list_off [nlist + 1] (list_off[0] = 0), list_rows
 *   [list_off[nlist]] internal rows (lists are disjoint); uploaded and kept until the next call.  Set them again after the rows change.
 * rxgpu_search_knn_lists: `coarse` = a flat index of the nlist centroids (same metric family, same device).  The nprobe nearest centroids
 *   are found on the device, their lists are marked in an allowed-rows bitmap, expanded to the ascending row list and scanned
 *   (rxgpu_search_knn_subset's kernels, the int8-pruned ones where rxgpu_scan_tier_subset says so) without a host round trip in between: same result as rxgpu_search_knn_subset over the union of
 *   the probed lists.  query = host [dim], already prepared for the metric (cosine: normalised).  Any nprobe (clamped to nlist): up to
 *   128 lists the coarse result never leaves HBM, wider probes fetch the nprobe list ids and send them back.  *out_scanned (optional)
 *   = rows in the probed lists.  Output as rxgpu_search_knn for nq = 1.
 * rxgpu_search_range_lists: IndexIVFFlat::range_search (ivf_index.cc:212-272 drives it) over the same device lists — probed lists ->
 *   row list on the device -> the range kernels of rxgpu_search_range_subset (the int8-pruned one where rxgpu_scan_tier_range says so
 *   for the rows of the probed lists); output, overflow protocol and ordering as rxgpu_search_range_subset.
 * rxgpu_search_knn_lists_batch: nq queries (host [nq][dim], prepared for the metric) in one call.  For every i, out_dist / out_row
 *   [i * kk ..], out_count[i] and out_scanned[i] (optional array) are what rxgpu_search_knn_lists(h, coarse, queries + i * dim, nprobe, kk,
 *   ...) writes for that query: the same rows, the same distance bits, the same (dist, row) order, out_count[i] = min(kk, rows in the
 *   probed lists).  The checks and codes are the single call's (a sharded handle, lists unset or stale: RXGPU_ERR_LOGIC); nq == 0, kk == 0
 *   or an empty index: RXGPU_OK with zero counts; nprobe is clamped to [1, nlist].  With the clamped nprobe <= 128 and kk <= 128 the
 *   queries go through DEVICE TRAINS on one stream, no host round trip inside a train: one upload, the coarse search for all of them
 *   (the chain of rxgpu_search_knn over the centroids), per query the running 64-entry chunk counts of its probed lists, one list scan
 *   (knn_scan_lists: grid (workgroups per query, queries); the lists are disjoint, so a query's candidates are the concatenation of
 *   its probed lists — no bitmap, no row list) and one merge, then one set of copies back and one wait.  A call is cut into several
 *   trains only where its device buffers would pass 256 MiB (RXGPU_IVF_BATCH_SCRATCH_BYTES, read per call, moves that); the launches
 *   this call adds to a train — chunk counts, scan, merge — do not depend on the number of queries.  Outside that envelope every query is
 *   answered by the single call's chain inside this call.
 * rxgpu_ivf_read_batch_stats: batch calls, their queries, device trains run and queries answered one by one, since the last call
 *   (any may be NULL).
 * rxgpu_ivf_batch_default: 1 where a caller with nq queries at hand should make the batch call (nq >= 2 inside the envelope), 0 where it
 *   should keep driving single calls — the rule of ivf_batch_plan.h that GpuIvfFlat::SearchBatch follows (no device is touched; nprobe
 *   = the clamped value). */
int rxgpu_index_set_lists(rxgpu_index* h, uint32_t nlist, const uint64_t* list_off, const uint32_t* list_rows);
int rxgpu_search_knn_lists(rxgpu_index* h, rxgpu_index* coarse, const float* query, uint32_t nprobe, uint32_t kk, float* out_dist,
						   uint32_t* out_row, uint32_t* out_count, uint64_t* out_scanned);
int rxgpu_search_range_lists(rxgpu_index* h, rxgpu_index* coarse, const float* query, uint32_t nprobe, float radius, int inclusive, float* out_dist,
							 uint32_t* out_row, uint64_t cap, uint64_t* out_total, uint64_t* out_scanned);
int rxgpu_search_knn_lists_batch(rxgpu_index* h, rxgpu_index* coarse, const float* queries, uint32_t nq, uint32_t nprobe, uint32_t kk, float* out_dist,
								 uint32_t* out_row, uint32_t* out_count, uint64_t* out_scanned);
int rxgpu_ivf_read_batch_stats(rxgpu_index* h, uint64_t* calls, uint64_t* queries, uint64_t* trains, uint64_t* queries_one_by_one);
int rxgpu_ivf_batch_default(uint32_t nq, uint32_t nprobe, uint32_t kk);

/* ---- IVF training from resident rows: the device half of IndexIVF::train / add_with_ids as IvfIndex drives them (ivf_index.cc:96-108,
 * 143-160; Level1Quantizer::train_q1 IndexIVF.cpp:43-88 -> Clustering::train_encoded Clustering.cpp:330-560) -------------------------
 * `coarse` = the flat index of the current centroids (nlist = its row count; same dimension, same device: else RXGPU_ERR_PARAMS, as the
 * list search answers).  No inverted lists are needed.  A row takes part as its PREPARED vector: row[j], on a cosine index
 * row[j] * (1 / |row|) with the stored reciprocal norm — one correctly rounded f32 multiply (IndexIVFFlat.cpp:54-75 through the engine's
 * normalisation).  The rows are read where they are (owned or adopted storage, any admitted stride, the first dim floats of a row only).
 * Row ids are checked on the host before anything is launched: an id >= count is RXGPU_ERR_PARAMS.  n == 0 is RXGPU_OK; a sharded handle
 * (either one) is RXGPU_ERR_LOGIC.  Both calls synchronise.  Rows with a NaN or an infinite component are outside the contract.
 * rxgpu_ivf_assign: out_list[i] = the nearest centroid of row_ids[i] (row_ids == NULL: of row first_row + i; with a list first_row is
 *   ignored; the list may be in any order and repeat rows) — the result of rxgpu_search_knn(coarse, prepared vector, k = 1), bit for
 *   bit and with its (dist, centroid) tie order: the same chain answers, over queries gathered on the device in chunks of a bounded
 *   scratch (64 MiB of prepared vectors; RXGPU_IVF_TRAIN_SCRATCH_BYTES, read per call, moves it).
 * rxgpu_ivf_kmeans_step: one iteration's assignment of the n listed rows (row_ids == NULL: rows 0 .. n - 1) and compute_centroids
 *   (Clustering.cpp:153-230) over it: per centroid c and component j ONE f32 chain  sum = +0; sum += p_i[j]  over the LIST POSITIONS i
 *   with assign[i] == c in ascending order (the position in the list, not the row number), then sum * (1 / float(count_c)), every
 *   operation a correctly rounded f32 one and nothing contracted; count_c == 0: the centroid's row is all zeros (split_clusters, the
 *   caller's, fills it).  out_centroids [nlist][dim], out_hassign [nlist] = float(count_c), out_assign [n] or NULL.  The reference counts
 *   with += 1.0f, which agrees with the integer count below 2^24 points: n >= 2^24 is RXGPU_ERR_PARAMS.
 * rxgpu_ivf_read_train_stats: rows assigned by the two calls, k-means steps, the device time of the calls' launches between two events
 *   and the part of it the sums kernel took, since the last call (any may be NULL). */
int rxgpu_ivf_assign(rxgpu_index* h, rxgpu_index* coarse, const uint32_t* row_ids, uint64_t first_row, uint64_t n, uint32_t* out_list);
int rxgpu_ivf_kmeans_step(rxgpu_index* h, rxgpu_index* coarse, const uint32_t* row_ids, uint64_t n, float* out_centroids, float* out_hassign,
						  uint32_t* out_assign);
int rxgpu_ivf_read_train_stats(rxgpu_index* h, uint64_t* rows_assigned, uint64_t* steps, double* kernel_ms, double* sums_ms);

/* Device-resident variant on `stream` (no synchronisation): d_row_ids = device [n_ids] uint32, 1 <= n_ids <= count,
 * kk in [1, 128]; d_out_count may be NULL.  The list is TRUSTED (strictly increasing, below count): an id beyond the
 * index would fault the device.  rxgpu_check_row_list_device() verifies a device list (synchronises `stream`).
 * Served by the scan rxgpu_scan_tier_subset names (the first int8-pruned call on an index builds the shadow and synchronises once). */
int rxgpu_search_knn_subset_device(rxgpu_index* h, const void* d_queries, uint32_t nq, uint32_t kk, const void* d_row_ids,
								   uint64_t n_ids, void* d_out_dist, void* d_out_row, void* d_out_count, void* stream);
int rxgpu_check_row_list_device(rxgpu_index* h, const void* d_row_ids, uint64_t n_ids, void* stream, int32_t* out_ok);

/* SearchRange over a row list (same list contract as rxgpu_search_knn_subset): every listed row with dist < radius (<= when
 * `inclusive`), sorted by (dist, row); *out_total = number of hits; RXGPU_ERR_OVERFLOW when it exceeds `cap` (call again with
 * cap >= *out_total).  Stands in for the list scan of faiss::IndexIVFFlat::range_search as the reference's IvfIndex calls it
 * (ivf_index.cc:212-272) — the probed inverted lists are the row list. */
/* Which kernel reads the rows: the f32 gather kernel (knn_range_subset) unless rxgpu_scan_tier_range(n_ids, dim, 1, ...) says 2; then the
 * int8 shadow is read for the listed rows and the exact kernel re-scores the rows its bound cannot exclude - the same total, rows and
 * distance bits (see rxgpu_search_range). */
int rxgpu_search_range_subset(rxgpu_index* h, const float* query, float radius, int inclusive, const uint32_t* row_ids, uint64_t n_ids,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total);

/* Multi-GPU merge step (no reference counterpart: the reference has no device notion).  d_gathered = the all-gather of every
 * rank's search output for one query batch: [world][2][nq][kk] 32-bit words — per rank the [nq][kk] distances followed by the
 * [nq][kk] shard-local rows (what rxgpu_search_knn_device writes when d_out_row == d_out_dist + nq*kk words).
 * Writes the global top-kk under (dist, global row = shard*shard_rows + local row): d_out_dist [nq][kk], d_out_row [nq][kk] u32.
 * Pure device work on `stream`, no synchronisation. */
int rxgpu_merge_shards_device(const void* d_gathered, uint32_t world, uint32_t nq, uint32_t kk, uint32_t shard_rows, void* d_out_dist,
							  void* d_out_row, void* d_out_count, void* stream);

/* BruteforceSearch::SearchRange (bruteforce.cc:129-143): every row with dist < radius (inclusive != 0: dist <= radius;
 * the inclusive form serves the tie replay above).  Rows are returned sorted by (dist,row); *out_total receives the
 * number of hits; at most cap are written; RXGPU_ERR_OVERFLOW if out_total > cap (call again with a larger buffer).
 *
 * Which kernel reads the rows: the f32 kernel (knn_range) unless rxgpu_scan_tier_range() says 2 for the call.  Then the int8 shadow of
 * rxgpu_scan_tier is scanned (1 byte per element instead of 4; the first such call on an index builds it): a row can be a hit only if the
 * lower bound of its distance is within the query's margin of the radius, those rows are collected in a candidate list of
 * min(rows, max(4096, 2 min(cap, rows))) entries, and the exact kernel re-scores them and applies the real test - the same *out_total, rows,
 * distance bits and overflow protocol.  More candidates than the list holds (a boundary zone that full, a radius of +inf), a query or an
 * index without a finite bound, or no room for the shadow: the f32 kernel answers the call. */
int rxgpu_search_range(rxgpu_index* h, const float* query, float radius, int inclusive, float* out_dist, uint32_t* out_row,
					   uint64_t cap, uint64_t* out_total);
/* Which kernel a range call takes (rxgpu_search_range, rxgpu_search_range_subset, rxgpu_search_range_lists and their per-shard calls): 0
 * the f32 range kernel, 2 the int8-pruned one (no device is touched; there is no bf16 form).  rows = the rows scanned: the index's, or the
 * entries of the list when `listed`.  0 whenever RXGPU_SCAN_BF16 is 0 or 1, RXGPU_SCAN_I8 is 0, the shadow is not available, the
 * dimension is outside 128 < dim <= 1024 or there are no rows.  Otherwise RXGPU_SCAN_I8=1 forces 2 at any size, and the automatic rule
 * (RXGPU_SCAN_I8 unset) gives 2 on an index without a NaN / infinite row norm when the scanned rows hold at least
 * RXGPU_SCAN_I8_RANGE_MIN_BYTES of f32 data (rows * dim * 4; default 16 GiB, the measured size from which the tier wins whatever the
 * number of hits, profiles/range_i8_ab.json) - and, for a list, at least RXGPU_SCAN_I8_SUBSET_MIN_BYTES as well, whose default is still
 * the maximum value: a list call takes the tier only where that variable or RXGPU_SCAN_I8=1 asks for it.  The environment is read per
 * call. */
int rxgpu_scan_tier_range(uint64_t rows, uint32_t dim, int listed, int shadow_available, int stats_finite);

/* Distances of one query against an explicit list of rows (DistCalculator::operator()(q,row,id), hnswlib.h:147-165);
 * used for exact re-scoring and by tests. */
int rxgpu_distances(rxgpu_index* h, const float* query, const uint32_t* rows, uint32_t n, float* out_dist);

/* ---------------------------------------------------------------------------------------------------------
 * HNSW search (HierarchicalNSWImpl<float>::SearchKnn, hnswalg.h:1988-2012) over a host-built graph
 * ------------------------------------------------------------------------------------------------------- */

/* Mirror the graph of an HNSW index into HBM.  The vectors are the index rows (rxgpu_index_upload_rows, internal id == row);
 * the graph is the flat form of HierarchicalNSWImpl's storage (hnswalg.h:216-240), built on the host by the GPU Map:
 *   links0     u32 [count][1 + max_m0]   slot 0 = neighbour count, then the level-0 links in stored order
 *   upper      u32 [upper_blocks][1 + M] per-level lists of the upper layers; node i owns its `level_i` blocks starting at
 *   upper_off  u64 [count + 1]           block upper_off[i] (level 1 first)
 *   deleted    u8  [count]               DELETE_MARK flags (hnswalg.h:1366-1374)
 * entry / maxlevel = enterpoint_node_ / maxlevel_; num_deleted selects the bare-bone search (hnswalg.h:1982).
 * Limits of the GPU engine: max_m0 <= 128 (M <= 64). */
int rxgpu_hnsw_attach_graph(rxgpu_index* h, const uint32_t* links0, const uint64_t* upper_off, const uint32_t* upper, uint64_t upper_blocks,
							const uint8_t* deleted, uint32_t M, uint32_t max_m0, int32_t maxlevel, uint32_t entry, uint64_t num_deleted);
/* In-place mirror of a host-side insert or update (addPoint / updatePoint, hnswalg.h:1472-1852, touch the new element and a few dozen
 * neighbours): instead of re-uploading the whole graph, the nodes whose lists changed are scattered into the resident arrays.  Call after
 * rxgpu_index_upload_rows for the new rows.  dirty_ids [n_dirty]: every node with a changed level-0 list, upper list or delete flag; new
 * nodes (id >= the attached node count) all listed, ascending; links0_rows [n_dirty][1 + max_m0]; deleted_flags [n_dirty]; levels [n_dirty]
 * = the node's level (upper blocks); upper_rows = those blocks concatenated in dirty order, (1 + M) words each.
 * RXGPU_ERR_OVERFLOW: the arrays allocated by the last attach cannot take the growth — attach the graph again. */
int rxgpu_hnsw_patch_graph(rxgpu_index* h, uint32_t n_dirty, const uint32_t* dirty_ids, const uint32_t* links0_rows, const uint8_t* deleted_flags,
						   const int32_t* levels, const uint32_t* upper_rows, int32_t maxlevel, uint32_t entry, uint64_t num_deleted);
/* MarkDelete mirror (hnswalg.h:1303-1339): refresh only the flags. */
int rxgpu_hnsw_update_deleted(rxgpu_index* h, const uint8_t* deleted, uint64_t num_deleted);

/* The level-0 graph built on the device in batches (addPoint's level-0 half, hnswalg.h:1694-1852, 977-1024, 1042-1180, for many rows at
 * once against the graph as it was before them — the form the reference accepts from its concurrent build).  Rows [first_row, first_row + n)
 * are uploaded (rxgpu_index_upload_rows) but not linked; first_row must equal the attached node count (>= 1).  Per row i: SearchKnn as
 * rxgpu_hnsw_search_knn defines it with k = ef = ef_construction over the nodes < first_row, the stored row as the query (cosine: the raw
 * row); the distances HnswGraph::distIds gives for i and the rows found; getNeighborsByHeuristic2 (M kept at most); the list of i in the
 * order mutuallyConnectNewElement writes it.  Per node t that received links: the new rows appended in ascending order while the list has
 * room, else ONE getNeighborsByHeuristic2 over its list and all the incoming rows (the reference: one per incoming link).  Afterwards the
 * attached node count is first_row + n; the upper lists of the new nodes follow through rxgpu_hnsw_patch_upper, before the next batch or
 * search.  Graphs without deleted nodes, M <= 64, ef_construction <= 256: RXGPU_ERR_PARAMS otherwise.  RXGPU_ERR_OVERFLOW: the level-0
 * array allocated by the last attach cannot take the rows — attach the graph again.  Synchronises. */
int rxgpu_hnsw_link_batch(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t ef_construction);
/* The upper lists only (addPoint's levels >= 1, hnswalg.h:1694-1852, built on the host): rxgpu_hnsw_patch_graph without level 0 and
 * delete flags.  ids [n_nodes]: every node whose upper lists changed; the nodes rxgpu_hnsw_link_batch added all listed, ascending (level 0
 * nodes too: levels[j] = 0); levels / upper_rows as for rxgpu_hnsw_patch_graph.  RXGPU_ERR_OVERFLOW: attach the graph again. */
int rxgpu_hnsw_patch_upper(rxgpu_index* h, uint32_t n_nodes, const uint32_t* ids, const int32_t* levels, const uint32_t* upper_rows, int32_t maxlevel,
						   uint32_t entry);
/* Level-0 lists [first_row, first_row + n) of the mirror, out [n][1 + max_m0] (mutuallyConnectNewElement's result, hnswalg.h:1042-1180). */
int rxgpu_hnsw_read_links0(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t* out);
/* rxgpu_hnsw_link_batch since the last call (hnswalg.h:1694-1852, 977-1024, 1042-1180 on the device): rows linked, batches, nodes whose
 * list was re-selected, nodes with more than 256 entries (finished by a second launch), and phase_ms [3] = search, select + pair grouping,
 * back-links (the search: wall clock of the call, which drains its stream; the others between events).  Any may be NULL. */
int rxgpu_hnsw_read_build_stats(rxgpu_index* h, uint64_t* rows, uint64_t* batches, uint64_t* reselected, uint64_t* past_cap, double* phase_ms);

/* Level 1 of the batch rxgpu_hnsw_link_batch linked last, built on the device under the same batch rule (addPoint's level-1 half for many
 * rows at once: the descent hnswalg.h:1762-1795, searchBaseLayer + getNeighborsByHeuristic2 977-1024 + mutuallyConnectNewElement 1042-1180
 * on level 1).  Called between rxgpu_hnsw_link_batch(first_row, n) and the patch of that batch: the attached node count is first_row + n,
 * the upper lists of the nodes >= first_row are not patched in yet, and the graph in front of the batch has a top level >= 1.  up_rows
 * [n_up]: EVERY row of the batch whose level is >= 1, ascending.  Per such row i: SearchKnn with k = ef = ef_construction over the nodes
 * < first_row with level 1 as the base layer — the greedy descent from the entry point through the levels >= 2, then the base-layer search
 * over the level-1 lists; this holds for rows of level >= 2 too, where addPoint would enter level 1 at the node its level-2 connect hands
 * down — then getNeighborsByHeuristic2 (M kept at most) and the list in the order mutuallyConnectNewElement writes it.  Per node t that
 * received links: the new rows appended ascending while its M slots have room, else ONE getNeighborsByHeuristic2 over its list and all the
 * incoming rows.  The lists of the older nodes are written into the mirror; those of up_rows wait on the device until
 * rxgpu_hnsw_patch_upper_from(first_level = 2) gives the new nodes their blocks.  Costs a dense level-1 array of (1 + M) * 4 bytes per row
 * of capacity until rxgpu_hnsw_release_build_view.  Errors — RXGPU_ERR_PARAMS: not the batch linked last, a row outside the batch or out of
 * order, a graph with deleted nodes, M > 64, ef_construction > 256; RXGPU_ERR_LOGIC: the batch is patched in already, level 1 of it is
 * linked already, the top level is 0, a sharded index.  Synchronises. */
int rxgpu_hnsw_link_batch_upper(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t n_up, const uint32_t* up_rows, uint32_t ef_construction);
/* rxgpu_hnsw_patch_upper with a first level (addPoint's levels >= first_level, hnswalg.h:1694-1852, built on the host).  first_level 1:
 * rxgpu_hnsw_patch_upper.  first_level 2: upper_rows holds the blocks of the levels >= 2 only (levels[j] - 1 blocks of a node of level
 * levels[j] >= 2, none otherwise); the new nodes get their levels[j] blocks as ever, their level-1 block is filled with what
 * rxgpu_hnsw_link_batch_upper built (RXGPU_ERR_LOGIC where it did not run over every new node of level >= 1), and the level 1 of the older
 * nodes is left as it is.  RXGPU_ERR_OVERFLOW: attach the graph again — rxgpu_hnsw_read_level still reads what the device built. */
int rxgpu_hnsw_patch_upper_from(rxgpu_index* h, int32_t first_level, uint32_t n_nodes, const uint32_t* ids, const int32_t* levels, const uint32_t* upper_rows,
								int32_t maxlevel, uint32_t entry);
/* The lists of one level >= 1 of the mirror (mutuallyConnectNewElement's result, hnswalg.h:1042-1180): out [n_ids][1 + M], an empty list
 * for a node that does not reach the level.  Between rxgpu_hnsw_link_batch_upper and the patch, level 1 of that batch's rows of level >= 1
 * is read from where it waits.  RXGPU_ERR_PARAMS: a node whose upper lists are not mirrored. */
int rxgpu_hnsw_read_level(rxgpu_index* h, int32_t level, uint64_t n_ids, const uint32_t* ids, uint32_t* out);
/* rxgpu_hnsw_link_batch_upper since the last call (hnswalg.h:1762-1852, 977-1024, 1042-1180 on level 1): rows linked, nodes whose list was
 * re-selected, nodes with more than 256 entries, phase_ms [3] = search, select + pair grouping, back-links.  Any may be NULL. */
int rxgpu_hnsw_read_build_upper_stats(rxgpu_index* h, uint64_t* rows, uint64_t* reselected, uint64_t* past_cap, double* phase_ms);
/* Frees the dense level-1 array of rxgpu_hnsw_link_batch_upper (the end of a build; the next call allocates it again).  RXGPU_ERR_LOGIC
 * while a batch's level-1 lists wait there for their patch (hnswalg.h:1042-1180 has no counterpart: the reference keeps lists in place). */
int rxgpu_hnsw_release_build_view(rxgpu_index* h);

/* SearchKnn for nq queries (host in/out).  ef == 0 means k*3/2 like the engine (hnswalg.h:1995); ef <= 4096
 * (RXGPU_ERR_PARAMS above that; from ef = 1025 on the candidate heap lives in global scratch instead of LDS).
 * Writes, per query, the members of the reference's top_candidates after trimming to k (UNORDERED: the Map pushes them into the
 * (dist,label) result heap exactly as hnswalg.h:2002-2010 does): out_dist/out_row [nq][k], out_count[q] <= k.
 * The traversal replays the reference's heaps step for step, so on the same graph the sets are identical. */
int rxgpu_hnsw_search_knn(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row,
						  uint32_t* out_count);
/* ONE query through the index's RESIDENT search kernel — the planner's call: HnswIndexBase::select issues one SearchKnn per query from as
 * many threads as there are connections (hnsw_index.cc:159-288; gtests/tests/unit/float_vector_index.cc:258-294 runs 16 of them).  The call
 * claims a slot of a mailbox in pinned host memory, stores the query and polls the answer; the kernel behind the mailbox is launched by
 * whichever caller finds none alive, serves every thread's requests side by side (one workgroup of four wavefronts per slot) and ends by
 * itself — when the index is about to change (every mutating entry point tells it), after RXGPU_HNSW_SERVER_IDLE_US (2000) without a
 * request, after RXGPU_HNSW_SERVER_LIFE_MS (50) in any case.  No launch, copy or completion signal lies on the path of a served query.
 * *served = 1: out_* hold what rxgpu_hnsw_search_knn returns for this query (the same device code runs the search).  *served = 0: this query
 * is not taken — every slot (RXGPU_HNSW_SERVER_SLOTS, 256) is busy, ef > 256 (224 on a graph with deleted nodes; up to 128 / 96 and above
 * that are served by two resident kernels of their own), a dimension other than
 * 128 / 512 / 768 / 1024 / 1536 (rxgpu_hnsw_distance_blocks names them), a profiled or sharded index, RXGPU_HNSW_SERVER=0, or the search needs the re-run tiers — and the caller uses
 * rxgpu_hnsw_search_knn, which tries the mailbox itself for nq == 1 and launches otherwise. */
int rxgpu_hnsw_search_knn_posted(rxgpu_index* h, const float* query, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row, uint32_t* out_count,
								 int32_t* served);
/* 64-float blocks of the fixed-dimension distance batch a search over rows of `dim` components takes (0: the generic batch).
 * sq8: over codes; deleted: the graph has deleted nodes.  *mailbox (may be NULL): 1 when the resident kernel serves that row format.
 * A pure function (no device is touched).  Floats: 128, 512, 768, 1024, 1536 -> dim / 64, mailbox 1, with or without deleted nodes; every
 * other size (384 among them) 0 / 0.  Codes: 128, 384, 512, 768, 1024, 1536 on a graph without deleted nodes, 128 and 768 with them. */
int rxgpu_hnsw_distance_blocks(uint32_t dim, int sq8, int deleted, int* mailbox);
/* The search kernels' own counters since the last read (reset by the call, like rxgpu_hnsw_read_stats): out4[0] = distance evaluations the
 * traversal used, [1] = hops, [2] = searches that started over on the reference's heaps inside the kernel, [3] = two 32-bit counts of the team
 * searches (small launches and the resident kernel): high half = hops that found their link block in LDS because it had come along with the
 * previous hop's rows; low half = distance trips of the look-ahead experiment (RXGPU_HNSW_SPEC=1, off by default; hnsw_search_core.hip.h). */
int rxgpu_hnsw_read_stats4(rxgpu_index* h, uint64_t* out4);
/* queries answered through the mailbox / resident kernels launched so far (instrumentation; 0 / 0 before the first such query) */
int rxgpu_hnsw_server_stats(rxgpu_index* h, uint64_t* served, uint64_t* generations);
/* ... and where their time went, summed over the queries answered so far: on the device (the search itself, by the kernel's wall clock) and at
 * the caller (from the store of the request until the answer was seen: the search + the mailbox + the caller's wake-up) — microseconds */
int rxgpu_hnsw_server_times(rxgpu_index* h, uint64_t* device_us, uint64_t* caller_us);

/* SQ8 graphs — HierarchicalNSWImpl<uint8_t> after HnswIndexBase::Quantize (hnsw_index.cc:626-660, hnswalg.h:353-420): the level-0 payload
 * is one byte per component plus the row's corrective offset, distances are DistCalculator<uint8_t>::operator() (hnswlib.h:147-165) over
 * L2SqrDistance<uint8_t> / InnerProductDistance<uint8_t> (tools/distances/l2_dist.cc:168-199, ip_dist.cc:163-192):
 *   alpha_2 * sum + corr(query) + corr(row)   (negated for IP / cosine, times 1/|row| for cosine), times the query's normCoef.
 * The summation order of the reference's AVX-512 form is part of the contract and is reproduced on the device (v_dot4_u32_u8 partial
 * sums re-associated into the 16 zmm lanes), so results are bit-identical to the quantised engine on the same graph.
 * codes [count][dim] u8, corr [count] (Quantizer::Quantize + CorrectiveOffsets, quantizer.h:93-124); count == the index row count.
 * Attach after rxgpu_hnsw_attach_graph / upload; the float rows of the index are not read by the SQ8 search. */
int rxgpu_hnsw_attach_sq8(rxgpu_index* h, const uint8_t* codes, const float* corr, uint64_t count, float alpha_2);
/* Rows [first_row, first_row + n) of the code table (first_row <= rows that have codes; first_row + n <= count): the device side of a point
 * added to or updated in a quantised graph (addPoint with a quantizer, hnswalg.h:1480-1495) — D + 4 bytes per row instead of the whole
 * table again.  The table is sized by the index capacity. */
int rxgpu_hnsw_upload_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const uint8_t* codes, const float* corr, float alpha_2);
/* Device side of Quantize / of points added to a quantised graph: codes + corrective offsets of rows [first_row, first_row + n) computed
 * ON THE DEVICE from the index's float rows (owned or adopted, at the index's row stride) with the caller's parameters (Sq8Params: minQ,
 * alpha, delta, alpha_2).  Same table, same range rules as rxgpu_hnsw_upload_sq8_rows (first_row <= rows that have codes,
 * first_row + n <= count; the table is sized by capacity): a hole or a range past count is RXGPU_ERR_PARAMS, n == 0 is RXGPU_OK, a sharded
 * handle is RXGPU_ERR_LOGIC (the shard handles take the call).  Result: byte for byte and bit for bit what Quantizer::quantize gives for
 * those rows under the index's metric (quantizer.h:93-124; inner product and cosine share a branch); an offset that comes out NaN — a row
 * with an infinite component — carries the reference platform's default NaN.  Rows with a NaN component are outside the contract (the
 * reference's float -> uint8 conversion is undefined for them): they get some code and some offset.  Synchronises. */
int rxgpu_hnsw_quantize_sq8(rxgpu_index* h, uint64_t first_row, uint64_t n, float min_q, float alpha, float delta, float alpha_2);
/* Test instrumentation: rows [first_row, first_row + n) of the code table and their corrective offsets back to the host (either may be
 * NULL).  Rows without codes: RXGPU_ERR_LOGIC. */
int rxgpu_hnsw_read_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, uint8_t* out_codes, float* out_corr);
/* Rows coded on the device (rxgpu_hnsw_quantize_sq8), launches and their device time since the last call (any may be NULL). */
int rxgpu_hnsw_read_sq8_quantize_stats(rxgpu_index* h, uint64_t* rows, uint64_t* launches, double* kernel_ms);
/* SearchKnn on the SQ8 graph.  The caller quantises the queries the way prepareData does (hnswalg.h:510-529): query_codes [nq][dim],
 * query_corr [nq], query_norm_coef [nq] (1 for L2 / IP, queryNormCoef for cosine, hnswalg.h:1855-1863).  Same outputs as
 * rxgpu_hnsw_search_knn. */
int rxgpu_hnsw_search_knn_sq8(rxgpu_index* h, const uint8_t* query_codes, const float* query_corr, const float* query_norm_coef, uint32_t nq,
							  uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row, uint32_t* out_count);
/* SearchKnn under an allowed-rows bitmap — `WHERE cond AND KNN(...)` on a graph index in ONE device call.  allowed_words = host
 * [n_words >= ceil(count / 32)], bit (r % 32) of word r / 32 set = node r may be returned (rxgpu_search_knn_bitmap's layout); bits at and
 * above the node count are ignored; one bitmap serves all nq queries.  The reference fork has no filter functor: its delete mark is how it
 * expresses a node that is traversed but not returned (hnswalg.h:1982 picks the branch by num_deleted, runLayer0Step :871-963 keeps a marked
 * node in candidate_set and out of top_candidates, MarkDelete :1303-1339 sets the mark).  So, per query, the call returns what
 * rxgpu_hnsw_search_knn (_sq8) returns on the same graph if every node with a clear bit also carried the delete mark, num_deleted counting
 * the nodes marked either way: ef == 0, the clamp of k and the outputs (unordered (dist, row), out_count[q] <= k) are the unfiltered call's.
 * *out_allowed (may be NULL) = set bits below the node count.  The kernels read the bitmap itself where they read the delete byte (N / 8
 * bytes per call in flight, uploaded once per call into the call's own context: concurrent calls bring their own filters).  A graph without
 * delete marks under a bitmap with every bit below the count set is answered by the unfiltered path (the reference's bare-bone branch).
 * RXGPU_ERR_PARAMS: allowed_words == NULL, n_words < ceil(count / 32), ef > 4096.  RXGPU_ERR_LOGIC: a sharded handle (its shard handles
 * take the call), no graph attached (no codes attached for _sq8).  nq == 0 or k == 0: RXGPU_OK, nothing written. */
int rxgpu_hnsw_search_knn_filtered(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, const uint32_t* allowed_words,
								   uint64_t n_words, float* out_dist, uint32_t* out_row, uint32_t* out_count, uint64_t* out_allowed);
int rxgpu_hnsw_search_knn_sq8_filtered(rxgpu_index* h, const uint8_t* query_codes, const float* query_corr, const float* query_norm_coef, uint32_t nq,
									   uint32_t k, uint32_t ef, const uint32_t* allowed_words, uint64_t n_words, float* out_dist, uint32_t* out_row,
									   uint32_t* out_count, uint64_t* out_allowed);
/* ONE quantised query through the index's RESIDENT search kernel over the SQ8 codes — rxgpu_hnsw_search_knn_posted for a quantised graph: the
 * same mailbox protocol, the same lifetime rules (idle / lifetime / every mutating entry point, the uploads of the code table among them, make
 * the kernel leave), one wavefront per slot.  The query travels as for rxgpu_hnsw_search_knn_sq8 with nq == 1: query_codes [dim], its
 * corrective offset and its normCoef.  *served = 1: out_* hold what rxgpu_hnsw_search_knn_sq8 returns for this query (the same device code
 * runs the search; a search that comes back flagged is answered by the launches' re-run tiers inside this call).  *served = 0: this query is
 * not taken — every slot is busy, ef > 256 (224 on a graph with deleted nodes), a dimension other than 128 / 384 / 512 / 768 / 1024 / 1536
 * (with deleted nodes: other than 128 / 768), no code table attached, a profiled or sharded index, RXGPU_HNSW_SERVER=0 or
 * RXGPU_HNSW_SERVER_SQ8=0 — and the caller uses rxgpu_hnsw_search_knn_sq8, which tries the mailbox itself for nq == 1 and launches otherwise. */
int rxgpu_hnsw_search_knn_sq8_posted(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t k, uint32_t ef,
									 float* out_dist, uint32_t* out_row, uint32_t* out_count, int32_t* served);
/* Counters accumulated since the last call (for the roofline accounting: bytes = evals*dim*4 + hops*(1+2M)*4). */
int rxgpu_hnsw_read_stats(rxgpu_index* h, uint64_t* distance_evals, uint64_t* hops);
/* Searches with ef <= 256 (<= 224 when the graph has deleted nodes) keep top_candidates + candidate_set (hnswalg.h:741-777) as one sorted
 * list in registers; a search in which EQUAL distances could change what the reference's binary heaps do (CompareByFirst,
 * hnswalg.h:581-585), or whose list runs out of registers, starts over on the kernel that replays those heaps.  Reads and resets the
 * number of such restarts.  RXGPU_HNSW_SORTED=0 in the environment keeps every search on the heap kernel. */
int rxgpu_hnsw_read_tie_reruns(rxgpu_index* h, uint64_t* reruns);
/* A search whose candidate_set (hnswalg.h:741-777, unbounded in the reference) outgrows the LDS area of its first pass is run again on the
 * heap kernel with the largest LDS heap (2048 entries) before the global-scratch tiers are tried.  Reads and resets the number of such
 * re-runs. */
int rxgpu_hnsw_read_lds_reruns(rxgpu_index* h, uint64_t* reruns);

/* HierarchicalNSW::SearchRange (hnswalg.h:2015-2070) with BOTH halves on the device: the ef-search, then the closure of its hits over the
 * level-0 links while dist < radius (a fresh visited set in which only the ef hits are marked; deleted neighbours skipped) in ONE launch.
 * Hits come back unordered ((dist, row), dist as the engine reports it: negated similarity for inner product / cosine).  cap too small:
 * RXGPU_ERR_OVERFLOW with *out_total = the hits counted so far (a lower bound) — retry with more room.  The _sq8 form runs over the
 * attached codes with the query as prepareData leaves it. */
int rxgpu_hnsw_search_range(rxgpu_index* h, const float* query, float radius, uint32_t ef, float* out_dist, uint32_t* out_row, uint64_t cap,
							uint64_t* out_total);
int rxgpu_hnsw_search_range_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, float radius, uint32_t ef,
								float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total);
/* Streaming (batched) KNN over the attached graph: HierarchicalNSWImpl::BeginStreamingSearch / ContinueStreamingSearch
 * (cpp_src/core/index/float_vector/hnswlib/hnswalg.h:1865-1975; interface hnsw_interface.h:18-45, 99-102).  The session owns its
 * Layer0SearchState (candidate_set, top_candidates, top_candidates_extras, visited set) in device memory.  query: [dim] floats, already
 * normalised for cosine (hnsw_index.cc:303-314); ef == 0 -> 100.  Every continue(batch) returns <= batch (dist, internal row) pairs,
 * worst first like emitStreamingBatch pops them, and *exhausted as the reference reports it.  The graph must not change during a
 * session (the reference requires an external read lock for the same reason). */
typedef struct rxgpu_hnsw_stream rxgpu_hnsw_stream;
int rxgpu_hnsw_stream_begin(rxgpu_index* h, const float* query, uint32_t ef, rxgpu_hnsw_stream** out);
/* The same session over the attached SQ8 codes (HierarchicalNSWImpl<uint8_t>): query codes + corrective offset + normCoef as for
 * rxgpu_hnsw_search_knn_sq8; rxgpu_hnsw_stream_continue / _end as above. */
int rxgpu_hnsw_stream_begin_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t ef, rxgpu_hnsw_stream** out);
int rxgpu_hnsw_stream_continue(rxgpu_hnsw_stream* s, uint32_t batch, float* out_dist, uint32_t* out_row, uint32_t* out_count, int32_t* exhausted);
void rxgpu_hnsw_stream_end(rxgpu_hnsw_stream* s);
/* `WHERE cond AND KNN(...)` over a session: the loop of StreamingKnnIndexIterator::Next (cpp_src/core/nsselecter/
 * knn_streaming_index_iterator.cc:36-110) for a filter that is a bitmap, in ONE device call (two launches at most) instead of a launch, two
 * synchronisations and three copies per Continue:
 *     calls = presented = accepted = 0;  batch = first_batch
 *     repeat:  B = continue(batch);  calls += 1;  presented += |B|;  accepted += rows of B whose bit is set
 *              stop if accepted >= needed or B.exhausted or calls >= max_calls
 *              batch = StreamingKnnEstimator::EstimateBatchSize(accepted, presented, needed)     (clamped to 100 .. 800)
 * allowed_words: one bit per internal row, bit (row & 31) of word row >> 5 (the rxgpu_search_knn_bitmap layout), n_words >=
 * ceil(count / 32) or RXGPU_ERR_PARAMS; bits at and above the node count are ignored; NULL = every row is allowed.  max_calls == 0 -> 1000
 * (kMaxContinueCalls).  needed == 0 or first_batch == 0: RXGPU_OK, nothing runs.
 * Out: the accepted (dist, row) pairs of every call, calls in order, the rows of a call in the order rxgpu_hnsw_stream_continue delivers
 * them; per call c its batch, the rows it delivered and out_call_end[c] = accepted rows through call c.  The cut at the needed-th row in
 * (dist, label) order is the caller's.  cap < rxgpu_hnsw_stream_collect_bound(count, needed, first_batch) = min(count, needed - 1 +
 * max(first_batch, 800)) or calls_cap < rxgpu_hnsw_stream_collect_calls_bound(...) = min(max_calls, count + 1): RXGPU_ERR_PARAMS — the room
 * is checked before anything runs, never found short at run time.  An empty graph: exhausted, 0 calls.  A graph that changed under the
 * session: RXGPU_ERR_LOGIC.  *out_launches (may be NULL): kernel launches the call took — 2 when the session's heaps outgrew LDS on the way.
 * out_pos (may be NULL): per accepted row its position in its call's batch, 0 = delivered first (the call's worst) — with out_call_emitted it
 * tells how many rows a consumer that walks the calls best first has been presented when it reaches a given accepted row.
 * Afterwards the session is in the state behind its last Continue and takes further continue / collect calls. */
int rxgpu_hnsw_stream_collect(rxgpu_hnsw_stream* s, const uint32_t* allowed_words, uint64_t n_words, uint32_t needed, uint32_t first_batch, uint32_t max_calls,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint32_t* out_call_batch, uint32_t* out_call_emitted, uint32_t* out_call_end,
							  uint32_t calls_cap, uint32_t* out_calls, uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted,
							  uint32_t* out_launches, uint32_t* out_pos);
/* rxgpu_hnsw_collect_knn / _sq8: rxgpu_hnsw_stream_begin(_sq8) + rxgpu_hnsw_stream_collect + rxgpu_hnsw_stream_end for one query in ONE call on a
 * search context leased from the index: the heaps, the visited set, the bitmap and the outputs live in context buffers that grow once and are
 * reused, so a call in steady state allocates nothing (a session's Begin makes six allocations); the descent and the collection are one
 * launch, a handover to the global heaps is the second.  Arguments and results as above (ef as for _begin); the results equal begin ->
 * collect -> end.  A sharded handle: RXGPU_ERR_LOGIC.  Thread-safe like the other searches (a context per call in flight). */
int rxgpu_hnsw_collect_knn(rxgpu_index* h, const float* query, uint32_t ef, const uint32_t* allowed_words, uint64_t n_words, uint32_t needed, uint32_t first_batch,
						   uint32_t max_calls, float* out_dist, uint32_t* out_row, uint64_t cap, uint32_t* out_call_batch, uint32_t* out_call_emitted,
						   uint32_t* out_call_end, uint32_t calls_cap, uint32_t* out_calls, uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted,
						   uint32_t* out_launches, uint32_t* out_pos);
int rxgpu_hnsw_collect_knn_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t ef, const uint32_t* allowed_words,
							   uint64_t n_words, uint32_t needed, uint32_t first_batch, uint32_t max_calls, float* out_dist, uint32_t* out_row, uint64_t cap,
							   uint32_t* out_call_batch, uint32_t* out_call_emitted, uint32_t* out_call_end, uint32_t calls_cap, uint32_t* out_calls,
							   uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted, uint32_t* out_launches, uint32_t* out_pos);
/* the rule's pieces (csrc/hnsw_stream_collect_plan.h), for callers that run the loop themselves or size the buffers */
uint32_t rxgpu_hnsw_stream_collect_batch(uint64_t accepted, uint64_t presented, uint64_t needed);
uint64_t rxgpu_hnsw_stream_collect_bound(uint64_t count, uint32_t needed, uint32_t first_batch);
uint64_t rxgpu_hnsw_stream_collect_calls_bound(uint64_t count, uint32_t needed, uint32_t first_batch, uint32_t max_calls);

/* ---------------------------------------------------------------------------------------------------------
 * ft_fast BM25 score accumulation (ft::Merger<..>::mergeSimple, cpp_src/core/ft/ft_fast/mergerimpl.h:194-250)
 * ------------------------------------------------------------------------------------------------------- */

typedef struct rxgpu_ft_index rxgpu_ft_index; /* device mirror of one ft_fast DataHolder: vdoc statistics + flattened postings */

/* FTConfig fields read by the merge (cpp_src/core/ft/config/ftconfig.h:118-124,151-220); per-field arrays have num_fields entries. */
typedef struct rxgpu_ft_config {
	double bm25_k1, bm25_b;                    /* Bm25Config: 2.0, 0.75 */
	double summation_ranks_by_fields_ratio;    /* 0.0 */
	double full_match_boost;                   /* 1.1; addFullMatchBoost (merger.h:100-109) is applied on the device (the word counts are resident) */
	int32_t min_rank;                          /* 5   (host) */
	uint32_t merge_limit;                      /* 20000 */
	uint32_t num_fields;
	const double *bm25_boost, *bm25_weight, *term_len_boost, *term_len_weight, *position_boost, *position_weight;
	double distance_boost, distance_weight;    /* 1.0, 0.5 (ftconfig.h:180-181); read by the multi-term merge only */
	int32_t bm25_type;                         /* FTConfig::Bm25Config::bm25Type (ftconfig.h:199-206; calculators in core/ft/bm25.h:8-68):
	                                              0 = rx (the default), 1 = classic, 2 = wordCount.  ABI 2. */
} rxgpu_ft_config;

/* FtDslOpts of the query term (cpp_src/core/ft/ftdsl.h:13-35).  At most 4096 sub-terms per term on the GPU engine. */
typedef struct rxgpu_ft_term_opts {
	float boost, term_len_boost;
	const float* field_boost;       /* FtDslFieldOpts::boost per field */
	const uint8_t* need_sum_rank;   /* FtDslFieldOpts::needSumRank per field (at most 8 set on the GPU engine) */
} rxgpu_ft_term_opts;

int rxgpu_ft_create(uint32_t num_fields, int device, rxgpu_ft_index** out);
void rxgpu_ft_destroy(rxgpu_ft_index* h);
/* The same index cut into DOCUMENT-RANGE shards over a device list (SURVEY 8e "BM25": "shard by doc-id range (each GPU holds the posting
 * fragments of its docs; idf uses global N and df ...); exchange = ... the uint16 pre-score histogram for the global threshold"): contiguous
 * runs of 8192-document ranges, one run per listed device (1..64 entries; a device may repeat).  rxgpu_ft_set_docs replicates the per-document
 * statistics and fixes the cut (call it BEFORE the words); rxgpu_ft_set_word / rxgpu_ft_set_word_positions hand every shard the postings of
 * its documents with the whole list's length as document frequency.  rxgpu_ft_merge_simple_raw / _terms_raw / _query_raw (without phrases)
 * run the ordinary launch train on every shard at once and exchange, between its kernels, what spans the shards — every shard's pre-score
 * histogram + mask popcount (the 2-phase gate and preselectMostRelevantDocs' threshold, mergerimpl.h:386-464, with the ties at the threshold
 * handed out in document order) and every shard's table of first-met documents per (sub-term row, range) (the merge slots of addDoc,
 * merger.h:161-180, and the cut at maxMergedDocs) — one all-gather each, stream-ordered between the shards' kernels with no host round trip:
 * an ncclAllGather over the listed devices (RCCL opened on demand; one communicator per index), a plain device copy when every shard lives on
 * one device; without RCCL on a multi-device node, or with RXGPU_SHARD_MERGE=host at creation, the pieces travel through the host
 * (rxgpu_ft_shard_exchange_mode 1 = on the devices, 0 = through the host).  The result is the single
 * index's, bit for bit, in merge order.  rxgpu_ft_merge_query2_raw's multi-word synonyms run there too (a synonym's mask, the term
 * counting and the removal of documents that hold only parts of it, mergerimpl.h:347-361 / 509-555, are decided per document, and a
 * document lies in one shard; the marked documents go after the union of the shards' slots), and so do phrases: PhraseMerger runs on every
 * shard over its fragments — a phrase is decided inside a document —, the rows of a phrase are numbered alike on every shard, the admission
 * cut of the whole index (at most merge_limit candidates of the first term in (row, document) order, phrasemerger.h:341) is settled between
 * the shards' admission passes, NumDocsMerged() in the 2-phase estimate is the sum.
 * rxgpu_ft_merge_query_areas_raw works there as well (a document's areas are built by the shard that holds it, at its global merge slot).
 * rxgpu_ft_merge_batch_raw runs its merges one after the other there.  Packed uploads (the host decodes, GpuFtMerger::SetWordsPacked) and
 * resident (hybrid) merges are single-device features: RXGPU_ERR_LOGIC here. */
int rxgpu_ft_create_sharded(uint32_t num_fields, uint32_t n_devices, const int* devices, rxgpu_ft_index** out);
uint32_t rxgpu_ft_shard_count(const rxgpu_ft_index* h);           /* 0 for an unsharded index */
/* The cut of a sharded index is fixed by the first rxgpu_ft_set_docs and kept while the shards hold words: an index that grows through
 * step commits (a larger total_docs, only the changed words uploaded again) keeps its fragments, the new document ranges go to the last
 * shard.  Ranges of the fullest shard / ranges of an even cut; 1.0 for an even cut or an unsharded index. */
double rxgpu_ft_shard_imbalance(const rxgpu_ft_index* h);
int rxgpu_ft_shard_exchange_mode(const rxgpu_ft_index* h);        /* 1 on the devices, 0 through the host, -1 not sharded */
uint64_t rxgpu_ft_shard_collectives(const rxgpu_ft_index* h);     /* all-gathers issued so far */
int rxgpu_ft_shard_ranges(const rxgpu_ft_index* h, uint32_t shard, uint32_t* range_begin, uint32_t* range_count);   /* the shard's run of 8192-document ranges */
/* Documents that hold the word over the WHOLE index (a sharded handle: the length of the whole list, not of a shard's fragment); 0 for a
 * word the index does not know (MaxVDocs of a sub-term: what the merge limits and the 2-phase estimate are computed from). */
int rxgpu_ft_word_df(rxgpu_ft_index* h, uint32_t word_id, uint64_t* out_df);
/* The DocsStatsGetter of IndexText (cpp_src/core/index/indextext/indextext.h:245-258): total_docs counts the empty sentinel
 * vdoc 0 ("first doc is always empty"); words_in_field [total_docs][num_fields] = VDoc::wordCounts_; avg_words [num_fields];
 * removed [total_docs] or NULL. */
int rxgpu_ft_set_docs(rxgpu_ft_index* h, uint64_t total_docs, const float* words_in_field, const float* avg_words, const uint8_t* removed);
/* Posting list of one dictionary word (IdRelVec / PackedIdRelVec, cpp_src/core/ft/idrelset.h:62-294) flattened to SoA: ascending
 * vdoc ids; per posting a run [ent_off[i], ent_off[i+1]) of (field, occurrences in that field, first position in that field),
 * fields ascending — exactly what calcTermRankImpl derives from IdRelType::Pos() (phrasemergerimpl.h:24-49). */
int rxgpu_ft_set_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* ent_off, const uint8_t* ent_field,
					  const uint32_t* ent_tf, const uint32_t* ent_first_pos);
/* Device half of Merger::mergeSimple for a Simple() query: nsub sub-terms (word_ids[], procs[], caller-sorted by proc desc like
 * SortSubterms), docsExcluded bitmap or NULL.  Writes the admitted documents IN MERGE ORDER with their rank (addFullMatchBoost applied,
 * merger.h:100-109) and field — before postProcessResults (merger.h:111-155), which the host merger applies to these <= merge_limit rows. */
int rxgpu_ft_merge_simple_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_term_opts* opts, uint32_t nsub,
							  const uint32_t* word_ids, const float* procs, const uint8_t* excluded, uint32_t* out_doc, float* out_proc,
							  uint8_t* out_field, uint64_t cap, uint64_t* out_n);
/* Posting list of one dictionary word WITH its positions, as the multi-term merge needs them (PositionsDistance,
 * cpp_src/core/ft/ft_fast/mergerimpl.h:20-37): per posting a run [pos_off[i], pos_off[i+1]) of PosType words
 * (cpp_src/core/ft/idrelset.h:14-32: pos | arrayIdx << 28 | field << 56), ascending like IdRelType::SortAndUnique leaves them.
 * The (field, tf, first position) entries of rxgpu_ft_set_word are derived from them, so the word serves both merges. */
int rxgpu_ft_set_word_positions(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* pos_off, const uint64_t* fpos);
/* Posting lists in the reference's own storage format, decoded ON THE DEVICE: `bytes` holds the PackedIdRelVec streams of
 * nwords dictionary words back to back (cpp_src/core/ft/idrelset.h:155-280; IdRelType::pack / unpack, idrelset.cc:8-139; varints
 * tools/varint.h:122-176), word w = bytes[byte_off[w] .. byte_off[w + 1]); array_found_pos[w] = PackedIdRelVec's offset (relative to the
 * word's first byte) from which elements carry array indexes (>= the stream length if none do).  Replaces, for these words, the host-side
 * flattening + rxgpu_ft_set_word_positions: documents, positions (PosType words), the (field, tf, first position) entries of
 * calcTermRankImpl (phrasemergerimpl.h:24-49) and the range index are produced by a kernel (one thread per word) into one device
 * allocation per call.  A malformed stream (truncated varint, ids not ascending, field >= num_fields) is RXGPU_ERR_PARAMS naming the word. */
int rxgpu_ft_set_words_packed(rxgpu_ft_index* h, uint32_t nwords, const uint32_t* word_ids, const uint64_t* byte_off, const uint8_t* bytes,
							  const uint64_t* array_found_pos);
/* The same with word w's stream at data[w] (len[w] bytes) — PackedIdRelVec::RawData() of every dictionary entry, where the engine keeps it:
 * the streams are gathered once, in launch order, into pinned staging memory and travel in one asynchronous copy. */
int rxgpu_ft_set_words_packed_ptrs(rxgpu_ft_index* h, uint32_t nwords, const uint32_t* word_ids, const uint8_t* const* data, const uint64_t* len,
								   const uint64_t* array_found_pos);
/* Wall time spent inside rxgpu_ft_set_words_packed / _ptrs since the last call (the commit-side cost at the C-ABI boundary). */
int rxgpu_ft_read_packed_wall(rxgpu_ft_index* h, double* wall_ms);
/* Device time of the two decode kernels of rxgpu_ft_set_words_packed (count pass, write pass), the stream bytes they read (each pass)
 * and the bytes of the arrays they produced (256-byte aligned slices included), since the last call. */
int rxgpu_ft_read_packed_stats(rxgpu_ft_index* h, double* count_ms, double* write_ms, uint64_t* bytes_in, uint64_t* bytes_out);
/* Reads a word's device arrays back (tests, diagnostics).  Sizes first (array pointers null), then the arrays the caller wants. */
int rxgpu_ft_get_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t* n, uint64_t* npos, uint64_t* nent, uint32_t* doc, uint32_t* pos_off, uint64_t* fpos,
					  uint32_t* ent_off, uint8_t* ent_field, uint32_t* ent_tf, uint32_t* ent_first_pos, uint32_t* n_ranges, uint32_t* range_off);

/* Device half of Merger::Merge for a query of nterms >= 2 terms without phrases / multi-word synonyms (mergerimpl.h:466-566):
 * buildRestrictingBitmask (:326-384), the 2-phase gate + preselectMostRelevantDocs (:386-464, 486-490) and mergeTerm (:107-192) for
 * every term that is not a NOT.  ops[t]: OpType 1 OR / 2 AND / 3 NOT (core/type_consts.h); opts[t]: the term's FtDslOpts; the
 * sub-terms of term t are word_ids/procs[sub_off[t] .. sub_off[t+1]) sorted by proc descending (SortSubterms).
 * Writes the merged documents IN MERGE ORDER with proc (addFullMatchBoost applied: canBeBoostedByFullMatch :527-531, merger.h:100-109),
 * field and MergerDocumentData::termsCounter (merger.h:24); the host merger applies postProcessResults (merger.h:111-155).
 * *out_preselected = 1 if the preselect phase ran.  cap >= min(merge_limit, total postings). */
int rxgpu_ft_merge_terms_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
							 const uint32_t* sub_off, const uint32_t* word_ids, const float* procs, const uint8_t* excluded, uint32_t* out_doc,
							 float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n, int32_t* out_preselected);
/* Device half of Merger::Merge for ANY query made of terms and phrases (QueryMergeData::queryParts, querymergedata.h:191-242; the
 * selecter builds them in selecterimpl.h:482-572): the arguments of rxgpu_ft_merge_terms_raw plus, per term, FtDslOpts::phraseNum and
 * FtDslOpts::distance (ftdsl.h:13-35) — consecutive terms with the same phrase_num >= 0 form one phrase (PhraseResults; its operator is
 * its first term's), phrase_num < 0 is a plain term; both arrays may be NULL (no phrases).  Every phrase goes through PhraseMerger::Merge
 * on the device first (phrasemergerimpl.h:161-329: preselectDocsContainingAllTerms, mergePhraseTerm with MergePositionsWithDist /
 * SwitchPositions, phrasemerger.h:24-55, 107-140), then the query parts are merged: mergeTerm for terms, mergePhrase (mergerimpl.h:39-90)
 * for phrases, the restricting bitmask / pre-scores with GetMergedDocsBitmask / ExcludeMergedDocsFromBitmask / GetMergedDocsScore
 * (phrasemerger.h:309-333).  A single plain term is the Simple() merge; an Empty() query writes nothing.  Multi-word synonyms
 * (QueryMergeData::synonyms) are not covered: such queries stay on the CPU merger.  Outputs as rxgpu_ft_merge_terms_raw;
 * cap >= min(merge_limit, total postings of all terms). */
int rxgpu_ft_merge_query_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
							 const int32_t* phrase_num, const int32_t* distance, const uint32_t* sub_off, const uint32_t* word_ids, const float* procs,
							 const uint8_t* excluded, uint32_t* out_doc, float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap,
							 uint64_t* out_n, int32_t* out_preselected);
/* The whole QueryMergeData (querymergedata.h:191-242) in one description: query parts (terms, phrases) AND multi-word synonyms.
 * Terms [0, nterms) make up the query parts exactly as in rxgpu_ft_merge_query_raw; terms [nterms, nterms + nsyn_terms) are the terms of the
 * nsyn multi-word synonyms (Synonym::Terms(), querymergedata.h:178-192), synonym s owning terms nterms + syn_term_off[s] .. nterms +
 * syn_term_off[s + 1]; every per-term array has nterms + nsyn_terms entries (phrase_num / distance of a synonym's term are ignored).
 * part_syn_off [nparts + 1] / part_syn: PhraseOrTerm::SynonymsIds() of every query part (nparts = the number of parts the terms form).
 * suppressed (may be NULL): SubtermResults::Suppressed() per sub-term — what QueryMergeData::SupressDuplicatesInSynonyms (:221-241) set.
 * The merge: buildRestrictingBitmask with the synonyms' masks (mergerimpl.h:347-361), their terms in the pre-scores (:393-397) and in the
 * 2-phase estimate (merger.h:251-255), mergeTerm for every synonym term behind the query parts with the term counting, the
 * containsFullMultiWordSynonym rule and the removal of documents that hold only parts of a synonym (:509-555).  A query without
 * synonyms is rxgpu_ft_merge_query_raw's. */
typedef struct rxgpu_ft_query {
	uint32_t nterms, nsyn_terms;
	const int32_t* ops;
	const rxgpu_ft_term_opts* opts;
	const int32_t* phrase_num;      /* may be NULL */
	const int32_t* distance;        /* may be NULL */
	const uint32_t* sub_off;        /* [nterms + nsyn_terms + 1] */
	const uint32_t* word_ids;
	const float* procs;
	const uint8_t* suppressed;      /* per sub-term, may be NULL */
	uint32_t nsyn;
	const uint32_t* syn_term_off;   /* [nsyn + 1] */
	const uint32_t* part_syn_off;   /* [nparts + 1], may be NULL when nsyn == 0 */
	const uint32_t* part_syn;
} rxgpu_ft_query;
int rxgpu_ft_merge_query2_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* query, const uint8_t* excluded, uint32_t* out_doc,
							  float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n, int32_t* out_preselected);
/* Merger<IdCont, MergeDataAreas<Area>, ..>::Merge — the merge behind highlight() / snippet() (merger.h:36-57 with kWithRegularAreas; addAreas
 * :196-204; AreasInDocument / AreasInField::Insert / Area::Concat, core/ft/areaholder.h:9-37, 56-155): the result of rxgpu_ft_merge_query2_raw
 * plus, per merged document i (merge order, like out_doc) and field f, the areas its postings left: out_area_cnt[i * num_fields + f] entries
 * of {start, end, arrayIdx} at out_areas[((i * num_fields + f) * max_areas_in_doc + j) * 3], in the order AreasInField::data_ holds them
 * BEFORE Commit() (the engine sorts and joins them when they are read).  max_areas_in_doc = FTConfig::maxAreasInDoc (default 5), >= 1.
 * out_area_cnt: cap * num_fields words; out_areas: cap * num_fields * max_areas_in_doc * 3 words.  Queries of plain terms (Simple() included;
 * the words need their positions); phrases, multi-word synonyms and MergeDataAreas<AreaDebug> return RXGPU_ERR_LOGIC: the CPU merger. */
int rxgpu_ft_merge_query_areas_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* query, const uint8_t* excluded, uint32_t max_areas_in_doc,
								   uint32_t* out_doc, float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n,
								   int32_t* out_preselected, uint32_t* out_area_cnt, uint32_t* out_areas);
/* nq queries (each as in rxgpu_ft_merge_query2_raw) over one index in ONE launch train: the kernels of the merge run with the query as the
 * second grid dimension, so the per-launch floors and the ramp of every grid are paid once per train and the device works on all the
 * queries' document ranges at a time — the form for a caller with several Merge() calls in hand (the hybrid path's query batch, T planner
 * threads behind one combiner).  Per query i: excluded[i] (the array or any entry may be NULL), the output arrays out_*[i] of `cap` entries
 * each, out_n[i], out_preselected[i] (may be NULL).  Results are those of nq single calls, bit for bit.  Queries with phrases or
 * multi-word synonyms (kernels of their own in front of the train) are run one by one inside the call; at most 64 queries share a train
 * (longer batches are cut). */
int rxgpu_ft_merge_batch_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nq, const rxgpu_ft_query* queries, const uint8_t* const* excluded,
							 uint32_t* const* out_doc, float* const* out_proc, uint8_t* const* out_field, uint16_t* const* out_terms_counter, uint64_t cap,
							 uint64_t* out_n, int32_t* out_preselected);
/* Launch trains run by rxgpu_ft_merge_batch_raw and the merges they carried, since the index was created. */
int rxgpu_ft_read_batch_stats(rxgpu_ft_index* h, uint64_t* trains, uint64_t* merges);
/* Two launch trains produce the same merge: the dense one (a workgroup per 8192-document range, per-document arrays in HBM between its
 * kernels) and the one for SPARSELY hit ranges (a wavefront per (query, range), bitmaps per sub-term in LDS, nothing per document in HBM;
 * eligible: plain terms whose fields share one positive boost, <= 16 sub-terms, Bm25Rx / TermCount, weights below 1).  By default the host
 * picks per query (eligible and postings on <= 30 % of the documents -> sparse).  mode: -1 that default, 0 always dense, 1 sparse whenever
 * eligible.  Process-wide; RXGPU_FT_TRAIN=dense|sparse presets it.  rxgpu_ft_read_train_stats: merges run by either since the last call. */
void rxgpu_ft_set_train_mode(int mode);
int rxgpu_ft_read_train_stats(rxgpu_ft_index* h, uint64_t* dense_merges, uint64_t* sparse_merges);
/* ---------------------------------------------------------------------------------------------------------
 * Hybrid rank fusion on the device: MergerRankedImpl + mergeRanked (cpp_src/core/nsselecter/selectiteratorcontainer.cc:
 * 1343-1423, 1454-1559), RanksHolder::InitRRFPositions (ranks_holder.h:61-76), RerankerRRF / RerankerLinear (core/sorting/reranker.h:11-39),
 * the Merged<desc> order (selectiteratorcontainer.cc:1258-1283: desc = rank descending, ties by DESCENDING id).
 * ------------------------------------------------------------------------------------------------------- */
typedef struct rxgpu_hybrid_params {
	int32_t kind;       /* 0 = RRF: params[0] = rank_const; 1 = linear: params = kKnn, knnDefault, kFt, ftDefault, c */
	int32_t is_union;   /* the two ranked conditions joined by OR (union) / AND (intersection), selectiteratorcontainer.cc:1473-1480 */
	int32_t desc;       /* 1: the normal rank() / RRF() ordering */
	int32_t reserved;
	double params[5];
} rxgpu_hybrid_params;
/* The merge of rxgpu_ft_merge_simple_raw / _terms_raw, but the result STAYS IN HBM (ft_finish's output; no export, no wait, the call
 * returns as soon as the train is enqueued) for rxgpu_hybrid_fuse_resident to read.
 * A resident merge opens a SESSION on the index that belongs to the calling thread and ends with that thread's rxgpu_hybrid_fuse_resident:
 * ordinary merges of other threads run on the handle's other lanes meanwhile, another thread's resident merge (or session-less fusion)
 * WAITS for the session to end.  A session that is not fused within 2 s is taken over; its owner's prepare / fuse then fail with
 * RXGPU_ERR_LOGIC — a resident result is never silently replaced by an empty or a foreign one. */
int rxgpu_ft_merge_simple_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_term_opts* opts, uint32_t nsub,
								   const uint32_t* word_ids, const float* procs, const uint8_t* excluded);
int rxgpu_ft_merge_terms_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
								  const uint32_t* sub_off, const uint32_t* word_ids, const float* procs, const uint8_t* excluded);
/* ... the same for rxgpu_ft_merge_query_raw's queries (phrases included).  *out_enqueued = 0 when the query is Empty(): there is then no
 * resident result and the fusion sees an empty FT side. */
int rxgpu_ft_merge_query_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
								  const int32_t* phrase_num, const int32_t* distance, const uint32_t* sub_off, const uint32_t* word_ids, const float* procs,
								  const uint8_t* excluded, int32_t* out_enqueued);
/* The resident form of rxgpu_ft_merge_query2_raw (terms, phrases AND multi-word synonyms, QueryMergeData::synonyms): Merger::Merge
 * (mergerimpl.h:466-566) left in HBM for rxgpu_hybrid_prepare_resident / rxgpu_hybrid_fuse_resident.  The documents Merge() removes because
 * they hold only parts of a synonym (mergerimpl.h:533-555) are skipped by the fusion kernels. */
int rxgpu_ft_merge_query2_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* query, const uint8_t* excluded, int32_t* out_enqueued);
/* The FT-only half of the fusion (postProcessResults, the documents' order among themselves, the rank-class tables), enqueued behind the
 * resident merge: it needs nothing from the KNN side, so a caller that enqueues it BEFORE it starts the KNN search has it run while the
 * scan streams the corpus, and only the short join is left on the query's critical path.  Optional — rxgpu_hybrid_fuse_resident
 * enqueues it itself when it was not called with the same min_rank / params / d_row_of_doc. */
int rxgpu_hybrid_prepare_resident(rxgpu_ft_index* h, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_row_of_doc);
/* Fuses the resident merge of `h` (postProcessResults — merger.h:111-140: proc < min_rank dropped, scaled to 0..255, uint8 — is applied on
 * the device) with a KNN result that lies in HBM as rxgpu_search_knn_device left it: d_knn_dist / d_knn_row best first, d_knn_count (device
 * uint32, or NULL) of knn_n entries valid, the first k taking part (ranks as the planner sees them: the distance for L2, its negation for
 * inner product / cosine, hnsw_index.cc:261-270).  knn_stream: the stream that search was enqueued on (the fusion waits for it on the
 * device) or NULL.  d_row_of_doc: int32 [total_docs], vdoc -> row id when texts and rows correspond 1:1 otherwise than by number, or NULL;
 * d_rowid_of_row: int32 [rows], internal row -> row id (label >> 32), or NULL = identity.  One list of (row id, fused rank) comes back,
 * ordered like Merged<desc>.  *out_flags bit 0: the k-th and (k+1)-th KNN distances are equal — the boundary tie is decided by labels on
 * the host (GpuBruteforceMap replays it), the caller should take that path.  cap >= merge_limit + k. */
int rxgpu_hybrid_fuse_resident(rxgpu_ft_index* h, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_knn_dist,
							   const void* d_knn_row, const void* d_knn_count, uint32_t knn_n, uint32_t k, void* knn_stream, const void* d_row_of_doc,
							   const void* d_rowid_of_row, int32_t* out_ids, float* out_ranks, uint64_t cap, uint64_t* out_n, uint32_t* out_flags);
/* Fusions run by rxgpu_hybrid_fuse_resident and the device time of their JOIN kernel — what is left on the critical path once both
 * halves are there (HIP events on the merger's stream) — since the last call. */
int rxgpu_hybrid_read_stats(rxgpu_ft_index* h, uint64_t* calls, double* kernel_ms, double* prepare_ms /* the overlapped FT-only kernel; may be NULL */);
/* The same kernel on host arrays: knn_ids / knn_ranks best first (at most 1024), ft_ids (unique, any order) with their uint8 ranks
 * (MergeInfo::normalizedProc).  cap >= n_knn + n_ft. */
int rxgpu_hybrid_fuse(int device, const rxgpu_hybrid_params* params, int metric, const int32_t* knn_ids, const float* knn_ranks, uint32_t n_knn,
					  const int32_t* ft_ids, const uint8_t* ft_ranks, uint32_t n_ft, int32_t* out_ids, float* out_ranks, uint64_t cap, uint64_t* out_n);

/* Postings scored / kernel milliseconds since the last call (roofline accounting: 20 B per posting). */
int rxgpu_ft_read_stats(rxgpu_ft_index* h, uint64_t* postings, double* kernel_ms);

/* ---------------------------------------------------------------------------------------------------------
 * Instrumentation (bench.py roofline leg): HIP-event timing of the dominant kernel on its own stream.
 * ------------------------------------------------------------------------------------------------------- */
int rxgpu_profile_enable(rxgpu_index* h, int on);
/* name: "scan" | "merge" | "range" ...; returns launches recorded since enable and their summed milliseconds. */
int rxgpu_profile_read(rxgpu_index* h, const char* name, uint64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* RXGPU_H */
