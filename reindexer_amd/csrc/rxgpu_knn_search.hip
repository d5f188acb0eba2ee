// The search entry points of the C-ABI (include/rxgpu.h) over float_vector rows: brute force on the host, the device and resident, pre-filtered
// by row list or bitmap, IVF, range, single distances, and the device-side helpers of the one-process-per-GPU deployment.  Contexts, index
// lifetime and the mutations are rxgpu_capi.hip; the chains these calls enqueue are rxgpu_knn_chains.hip.  Host-side plumbing only — all
// arithmetic is in the kernels.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/rxgpu.h"
#include "ivf_batch_plan.h"
#include "ivf_train_plan.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"
#include "shard_plan.h"   // check_row_list

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::enqueue_knn;
using rxgpu::enqueue_knn_fused;
using rxgpu::enqueue_knn_subset;
using rxgpu::ProfileScope;
using rxgpu::search_subset_host;
using rxgpu::set_error;

namespace {

// Scratch bound to a caller-owned stream: stream order makes reuse safe without synchronising.
rxgpu_search_ctx* stream_ctx(rxgpu_index* h, void* stream) {
	std::lock_guard<std::mutex> lk(h->mtx);
	auto it = h->stream_ctx.find(stream);
	if (it != h->stream_ctx.end()) return it->second;
	auto* c = new rxgpu_search_ctx();
	c->stream = static_cast<hipStream_t>(stream);
	c->own_stream = false;
	h->stream_ctx[stream] = c;
	return c;
}

// the row list of a pre-filtered call on the host (the plan's ordered rule over one shard)
int check_rows_host(const rxgpu_index* h, const uint32_t* row_ids, uint64_t n_ids, const char* who) {
	RX_CHECK(rxgpu::check_row_list(row_ids, n_ids, h->count, true) == rxgpu::kRowListOk, RXGPU_ERR_PARAMS,
			 std::string(who) + ": row_ids must be strictly increasing and below the row count");
	return RXGPU_OK;
}

// The allowed-rows bitmap in c->d_bitmap (one bit per row, enqueued on c->stream) -> the ascending row list in c->d_subset: tile counts, their
// total read back (*total; the stream is idle behind it), then — expand, and any row allowed — the expansion.  head() enqueues what still
// writes the bitmap; it runs inside the first of the two profile scopes filed under `slot`.
template <class Head>
int bitmap_to_row_list(rxgpu_index* h, rxgpu_search_ctx* c, const char* slot, bool expand, unsigned long long* total, Head&& head) {
	const uint32_t tiles = rxgpu::bitmap_tiles(h->count);
	if (int rc = c->d_tiles.ensure(size_t(2) * tiles * sizeof(uint32_t) + sizeof(unsigned long long)); rc) return rc;
	uint32_t* tile_scratch = static_cast<uint32_t*>(c->d_tiles.ptr);
	unsigned long long* d_total = reinterpret_cast<unsigned long long*>(tile_scratch + size_t(2) * tiles);   // 8-byte aligned: 2 * tiles words
	{
		ProfileScope ps(h, slot, c->stream);
		head();
		rxgpu::launch_bitmap_count(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, d_total, c->stream);
	}
	RX_HIP(hipGetLastError());
	*total = 0;
	RX_HIP(hipMemcpyAsync(total, d_total, sizeof(*total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	if (*total == 0 || !expand) return RXGPU_OK;
	if (int rc = c->d_subset.ensure(*total * sizeof(uint32_t)); rc) return rc;
	{
		ProfileScope ps(h, slot, c->stream);
		rxgpu::launch_bitmap_expand(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, static_cast<uint32_t*>(c->d_subset.ptr), *total,
									c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// The end of every range call once the stream is idle and the hit count known: the first min(total, cap) hits lie in c->d_out_dist /
// d_out_row in any order.  More hits than cap: *out_total says how many, nothing is written.  Else sorted by (dist, row).
int range_finish(rxgpu_search_ctx* c, unsigned long long total, float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total, const char* who) {
	*out_total = total;
	if (total > cap) {
		set_error(std::string(who) + ": output buffer too small");
		return RXGPU_ERR_OVERFLOW;
	}
	if (total == 0) return RXGPU_OK;
	std::vector<float> hd(total);
	std::vector<uint32_t> hr(total);
	RX_HIP(hipMemcpy(hd.data(), c->d_out_dist.ptr, total * sizeof(float), hipMemcpyDeviceToHost));
	RX_HIP(hipMemcpy(hr.data(), c->d_out_row.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
	rxgpu::sort_dist_row(hd, hr, out_dist, out_row);
	return RXGPU_OK;
}

// The tail of a range call, behind its launch: the hits were counted in c->d_out_count.
int range_tail(rxgpu_search_ctx* c, float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total, const char* who) {
	RX_HIP(hipGetLastError());
	unsigned long long total = 0;
	RX_HIP(hipMemcpyAsync(&total, c->d_out_count.ptr, sizeof(total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	return range_finish(c, total, out_dist, out_row, cap, out_total, who);
}

// One range search on the device, for both entry shapes: the query lies in c->d_queries; listed: the row list (n entries) lies in c->d_subset, else
// the n rows of the index are scanned.  Where rxgpu_scan_tier_range says so the int8 shadow serves the call (enqueue_range_pruned_i8): the
// candidate count comes back with the hit count in the tail's one synchronisation, and more candidates than the list holds (an overfull
// boundary zone, a radius of +inf, a query or an index without a finite bound) or no room for the shadow leave the call to the f32 kernel.
int range_on_device(rxgpu_index* h, rxgpu_search_ctx* c, bool listed, uint64_t n, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
					uint64_t* out_total, const char* who) {
	const uint32_t* d_ids = listed ? static_cast<const uint32_t*>(c->d_subset.ptr) : nullptr;
	const uint64_t dcap = std::min<uint64_t>(cap, n);
	if (int rc = c->d_out_dist.ensure(std::max<uint64_t>(dcap, 1) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(std::max<uint64_t>(dcap, 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_count.ensure(sizeof(unsigned long long)); rc) return rc;
	RX_HIP(hipMemsetAsync(c->d_out_count.ptr, 0, sizeof(unsigned long long), c->stream));
	if (rxgpu::scan_policy_tier_range(n, h->dim, listed, !h->i8_unavailable, true) == rxgpu::kTierI8) {
		if (int rc = rxgpu::ensure_row_stats(h, c->stream); rc) return rc;   // (automatic mode asks whether the row statistics are finite)
		if (rxgpu::scan_policy_tier_range(n, h->dim, listed, !h->i8_unavailable, h->stats_finite) == rxgpu::kTierI8) {
			uint32_t ccap = 0;
			const int rc = rxgpu::enqueue_range_pruned_i8(h, c, d_ids, n, radius, inclusive, cap, dcap, &ccap);
			if (rc == RXGPU_OK) {
				unsigned long long total = 0;
				uint32_t cand = 0;
				RX_HIP(hipMemcpyAsync(&total, c->d_out_count.ptr, sizeof(total), hipMemcpyDeviceToHost, c->stream));
				RX_HIP(hipMemcpyAsync(&cand, c->d_cand_cnt.ptr, sizeof(cand), hipMemcpyDeviceToHost, c->stream));
				RX_HIP(hipStreamSynchronize(c->stream));
				if (h->profiling) {   // rxgpu_index_last_candidates; the KNN chain rxgpu_index_inspect may have recorded is not this call's
					h->last_cand_count = cand;
					h->last_cand_cap = ccap;
					std::lock_guard<std::mutex> lk(h->mtx);
					h->last_pruned_ctx = nullptr;
				}
				if (cand <= ccap) return range_finish(c, total, out_dist, out_row, cap, out_total, who);
				// (the exact tail did nothing: the counter is still zero)
			} else if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) {
				return rc;
			}
		}
	}
	{
		ProfileScope ps(h, listed ? "range_subset" : "range", c->stream);
		if (listed) {
			rxgpu::launch_range_subset(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr), d_ids, n, h->stride, h->dim, radius,
									   inclusive, static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), dcap,
									   static_cast<unsigned long long*>(c->d_out_count.ptr), rxgpu::scan_grid_x(n, h->cus), c->stream);
		} else {
			rxgpu::launch_range(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr), n, h->stride, h->dim, radius, inclusive,
								static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), dcap,
								static_cast<unsigned long long*>(c->d_out_count.ptr), rxgpu::scan_grid_x(n, h->cus), c->stream);
		}
	}
	return range_tail(c, out_dist, out_row, cap, out_total, who);
}

}  // namespace

extern "C" {

int rxgpu_search_knn_device(rxgpu_index* h, const void* d_queries, uint32_t nq, uint32_t kk, void* d_out_dist, void* d_out_row,
							void* d_out_count, void* stream) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_search_knn_device: not available on a sharded index");
	RX_CHECK(nq > 0 && d_queries && d_out_dist && d_out_row, RXGPU_ERR_PARAMS, "rxgpu_search_knn_device: null argument");
	RX_CHECK(kk > 0 && kk <= uint32_t(rxgpu::kMaxFusedK), RXGPU_ERR_PARAMS, "rxgpu_search_knn_device: kk must be in [1, 64]");
	RX_CHECK(h->count > 0, RXGPU_ERR_PARAMS, "rxgpu_search_knn_device: index is empty");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = stream_ctx(h, stream);
	return enqueue_knn(h, c, static_cast<const float*>(d_queries), nq, kk, static_cast<float*>(d_out_dist),
					   static_cast<uint32_t*>(d_out_row), static_cast<uint32_t*>(d_out_count));
}

// One query, the result LEFT IN HBM: enqueued on the calling thread's resident stream, nothing waited for.  The buffers belong to the index
// and hold this result until the SAME THREAD's next resident search on it (other threads have buffers of their own); a consumer on another
// stream orders itself behind *stream.
int rxgpu_search_knn_resident(rxgpu_index* h, const float* query, uint32_t kk, void** d_dist, void** d_row, void** d_count, void** stream,
							  uint32_t* entries) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query && d_dist && d_row && d_count && stream && entries, RXGPU_ERR_PARAMS, "rxgpu_search_knn_resident: null argument");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_search_knn_resident: not available on a sharded index");
	RX_CHECK(kk >= 1 && kk <= uint32_t(rxgpu::kMaxFusedK2), RXGPU_ERR_PARAMS, "rxgpu_search_knn_resident: kk must be in [1, 128]");
	RX_CHECK(h->count > 0, RXGPU_ERR_PARAMS, "rxgpu_search_knn_resident: index is empty");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = nullptr;
	{   // this thread's resident context (created on its first resident search; searches of one thread are sequential)
		std::lock_guard<std::mutex> lk(h->resident_mtx);
		rxgpu_search_ctx*& slot = h->resident_ctx[std::this_thread::get_id()];
		if (!slot) {
			slot = acquire_ctx(h);
			if (slot) rxgpu::resident_thread_uses(h);
		}
		c = slot;
	}
	if (!c) return RXGPU_ERR_DEVICE;
	const uint32_t eff = uint32_t(std::min<uint64_t>(kk, h->count));
	const size_t qbytes = size_t(h->dim) * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	if (int rc = c->ensure_pinned(qbytes); rc) return rc;
	RX_HIP(hipStreamSynchronize(c->stream));   // the staging copy of the query before this one has been read (normally long ago)
	std::memcpy(c->h_pinned, query, qbytes);
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, c->h_pinned, qbytes, hipMemcpyHostToDevice, c->stream));
	if (int rc = c->d_out_dist.ensure(size_t(eff) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_count.ensure(sizeof(uint32_t)); rc) return rc;
	auto* run = eff <= uint32_t(rxgpu::kMaxFusedK) ? enqueue_knn : enqueue_knn_fused;
	if (int rc = run(h, c, static_cast<const float*>(c->d_queries.ptr), 1, eff, static_cast<float*>(c->d_out_dist.ptr),
					 static_cast<uint32_t*>(c->d_out_row.ptr), static_cast<uint32_t*>(c->d_out_count.ptr));
		rc)
		return rc;
	*d_dist = c->d_out_dist.ptr;
	*d_row = c->d_out_row.ptr;
	*d_count = c->d_out_count.ptr;
	*stream = c->stream;
	*entries = eff;
	return RXGPU_OK;
}

uint32_t rxgpu_index_resident_contexts(rxgpu_index* h) {
	if (!h || h->shard_set) return 0;
	std::lock_guard<std::mutex> lk(h->resident_mtx);
	return uint32_t(h->resident_ctx.size());
}

int rxgpu_search_knn(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, float* out_dist, uint32_t* out_row,
					 uint32_t* out_count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(queries && out_dist && out_row && out_count, RXGPU_ERR_PARAMS, "rxgpu_search_knn: null argument");
	if (nq == 0) return RXGPU_OK;
	if (h->count == 0 || kk == 0) {   // bruteforce.cc:106-108
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	if (h->shard_set) return rxgpu::sharded_search_knn_impl(h, queries, nq, kk, nullptr, 0, out_dist, out_row, out_count);
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	const uint32_t eff = uint32_t(std::min<uint64_t>(kk, h->count));
	const size_t qbytes = size_t(nq) * h->dim * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, queries, qbytes, hipMemcpyHostToDevice, c->stream));

	if (eff <= uint32_t(rxgpu::kMaxFusedK2)) {
		if (int rc = c->d_out_dist.ensure(size_t(nq) * eff * sizeof(float)); rc) return rc;
		if (int rc = c->d_out_row.ensure(size_t(nq) * eff * sizeof(uint32_t)); rc) return rc;
		if (int rc = c->d_out_count.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
		// kk <= 64: fused / batched / pruned dispatch; 64 < kk <= 128 (e.g. hybrid k = 100): the fused scan with two list entries per lane
		auto* run = eff <= uint32_t(rxgpu::kMaxFusedK) ? enqueue_knn : enqueue_knn_fused;
		c->pruned_cap = 0;   // set by a pruned chain
		c->keep_values = h->profiling && nq == 1;   // what copy_back_knn records (it clears the flag)
		if (int rc = run(h, c, static_cast<const float*>(c->d_queries.ptr), nq, eff, static_cast<float*>(c->d_out_dist.ptr),
						 static_cast<uint32_t*>(c->d_out_row.ptr), static_cast<uint32_t*>(c->d_out_count.ptr));
			rc) {
			c->keep_values = false;
			return rc;
		}
		return rxgpu::copy_back_knn(h, c, nq, kk, eff, out_dist, out_row, out_count);
	}

	// large-k path: distance pass + radix select per query, final (dist,row) sort of kk entries on the host
	if (int rc = c->d_misc.ensure(h->count * sizeof(float)); rc) return rc;
	if (int rc = c->d_select.ensure(rxgpu::select_scratch_bytes(h->count)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(eff) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	const uint32_t gridx = rxgpu::scan_grid_x(h->count, h->cus);
	std::vector<float> hd(eff);
	std::vector<uint32_t> hr(eff);
	for (uint32_t q = 0; q < nq; ++q) {
		{
			ProfileScope ps(h, "scan", c->stream);
			rxgpu::launch_all_distances(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr) + size_t(q) * h->dim,
										h->count, h->stride, h->dim, static_cast<float*>(c->d_misc.ptr), gridx, c->stream);
		}
		{
			ProfileScope ps(h, "select", c->stream);
			rxgpu::launch_select_smallest(static_cast<const float*>(c->d_misc.ptr), h->count, eff, c->d_select.ptr,
										  static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), c->stream);
		}
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpyAsync(hd.data(), c->d_out_dist.ptr, size_t(eff) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(hr.data(), c->d_out_row.ptr, size_t(eff) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
		rxgpu::sort_dist_row(hd, hr, out_dist + size_t(q) * kk, out_row + size_t(q) * kk);
		out_count[q] = eff;
	}
	return RXGPU_OK;
}

int rxgpu_search_knn_subset(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* row_ids, uint64_t n_ids,
							float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(queries && out_dist && out_row && out_count && (n_ids == 0 || row_ids), RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset: null argument");
	if (h->shard_set) {   // differs from the single-device branch below, and is kept: kk == 0 is refused here, and the row list's messages are the fan-out's
		if (nq == 0) return RXGPU_OK;
		RX_CHECK(kk >= 1, RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset: kk must be >= 1");
		if (n_ids == 0) {
			std::fill(out_count, out_count + nq, 0u);
			return RXGPU_OK;
		}
		return rxgpu::sharded_search_knn_impl(h, queries, nq, kk, row_ids, n_ids, out_dist, out_row, out_count);
	}
	if (nq == 0) return RXGPU_OK;
	if (int rc = check_rows_host(h, row_ids, n_ids, "rxgpu_search_knn_subset"); rc) return rc;
	if (n_ids == 0 || kk == 0) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_subset.ensure(n_ids * sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_subset.ptr, row_ids, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	return search_subset_host(h, c, queries, nq, kk, static_cast<const uint32_t*>(c->d_subset.ptr), n_ids, out_dist, out_row, out_count);
}

int rxgpu_search_knn_bitmap(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* allowed_words, uint64_t n_words,
							float* out_dist, uint32_t* out_row, uint32_t* out_count, uint64_t* out_allowed) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_search_knn_bitmap: not available on a sharded index");
	RX_CHECK(queries && out_dist && out_row && out_count && allowed_words, RXGPU_ERR_PARAMS, "rxgpu_search_knn_bitmap: null argument");
	const uint64_t need_words = (h->count + 31) / 32;
	RX_CHECK(n_words >= need_words, RXGPU_ERR_PARAMS, "rxgpu_search_knn_bitmap: the bitmap must cover every row (ceil(count / 32) words)");
	if (out_allowed) *out_allowed = 0;
	if (nq == 0) return RXGPU_OK;
	if (h->count == 0) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_bitmap.ensure(need_words * sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_bitmap.ptr, allowed_words, need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	unsigned long long total = 0;
	if (int rc = bitmap_to_row_list(h, c, "bitmap", kk != 0, &total, [] {}); rc) return rc;
	if (out_allowed) *out_allowed = total;
	if (total == 0 || kk == 0) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	return search_subset_host(h, c, queries, nq, kk, static_cast<const uint32_t*>(c->d_subset.ptr), total, out_dist, out_row, out_count);
}

int rxgpu_index_set_lists(rxgpu_index* h, uint32_t nlist, const uint64_t* list_off, const uint32_t* list_rows) {
	RX_CHECK(h && list_off && nlist > 0, RXGPU_ERR_PARAMS, "rxgpu_index_set_lists: null argument");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_index_set_lists: not available on a sharded index");
	RX_CHECK(list_off[0] == 0, RXGPU_ERR_PARAMS, "rxgpu_index_set_lists: offsets start at 0");
	for (uint32_t l = 0; l < nlist; ++l) RX_CHECK(list_off[l] <= list_off[l + 1], RXGPU_ERR_PARAMS, "rxgpu_index_set_lists: offsets must not decrease");
	const uint64_t total = list_off[nlist];
	RX_CHECK(total <= h->count && (total == 0 || list_rows), RXGPU_ERR_PARAMS, "rxgpu_index_set_lists: more listed rows than the index holds");
	for (uint64_t i = 0; i < total; ++i) RX_CHECK(list_rows[i] < h->count, RXGPU_ERR_PARAMS, "rxgpu_index_set_lists: row out of range");
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	if (h->d_list_off) (void)hipFree(h->d_list_off);
	if (h->d_list_rows) (void)hipFree(h->d_list_rows);
	h->d_list_off = nullptr;
	h->d_list_rows = nullptr;
	h->nlist = 0;
	RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_list_off), (size_t(nlist) + 1) * sizeof(uint64_t)));
	RX_HIP(hipMemcpy(h->d_list_off, list_off, (size_t(nlist) + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
	if (total) {
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_list_rows), total * sizeof(uint32_t)));
		RX_HIP(hipMemcpy(h->d_list_rows, list_rows, total * sizeof(uint32_t), hipMemcpyHostToDevice));
	}
	h->nlist = nlist;
	h->lists_rows = total;
	h->lists_count = h->count;
	h->lists_longest = 0;
	for (uint32_t l = 0; l < nlist; ++l) h->lists_longest = std::max<uint64_t>(h->lists_longest, list_off[l + 1] - list_off[l]);
	return RXGPU_OK;
}

namespace {
// The probed lists of one query as an ascending row list in c->d_subset, everything on the device: nprobe nearest centroids (the coarse
// quantiser's search; up to 128 lists its result never leaves HBM, wider probes fetch the list ids — nprobe words — and send them back),
// lists -> allowed-rows bitmap -> row list.  *total = rows to scan.
int ivf_probe_rows(rxgpu_index* h, rxgpu_index* coarse, rxgpu_search_ctx* c, const float* query, uint32_t nprobe, unsigned long long* total) {
	const size_t qbytes = size_t(h->dim) * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, qbytes, hipMemcpyHostToDevice, c->stream));
	const size_t o_lists = 0, o_dist = size_t(nprobe) * 4, o_cnt = o_dist + size_t(nprobe) * 4;
	if (int rc = c->d_ivf.ensure(o_cnt + 256); rc) return rc;
	char* ivf = static_cast<char*>(c->d_ivf.ptr);
	if (nprobe <= uint32_t(rxgpu::kMaxFusedK2)) {
		rxgpu_search_ctx* cc = stream_ctx(coarse, c->stream);
		auto* run = nprobe <= uint32_t(rxgpu::kMaxFusedK) ? enqueue_knn : enqueue_knn_fused;
		if (int rc = run(coarse, cc, static_cast<const float*>(c->d_queries.ptr), 1, nprobe, reinterpret_cast<float*>(ivf + o_dist),
						 reinterpret_cast<uint32_t*>(ivf + o_lists), reinterpret_cast<uint32_t*>(ivf + o_cnt));
			rc)
			return rc;
	} else {
		std::vector<float> cd(nprobe);
		std::vector<uint32_t> cl(nprobe);
		uint32_t cnt = 0;
		if (int rc = rxgpu_search_knn(coarse, query, 1, nprobe, cd.data(), cl.data(), &cnt); rc) return rc;
		RX_HIP(hipMemcpyAsync(ivf + o_lists, cl.data(), size_t(cnt) * 4, hipMemcpyHostToDevice, c->stream));
		RX_HIP(hipMemcpyAsync(ivf + o_cnt, &cnt, 4, hipMemcpyHostToDevice, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));   // cl / cnt live on this frame
	}
	const uint64_t need_words = (h->count + 31) / 32;
	if (int rc = c->d_bitmap.ensure(need_words * sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemsetAsync(c->d_bitmap.ptr, 0, need_words * sizeof(uint32_t), c->stream));
	return bitmap_to_row_list(h, c, "ivf_lists", true, total, [&] {
		rxgpu::launch_ivf_mark_lists(reinterpret_cast<const uint32_t*>(ivf + o_lists), reinterpret_cast<const uint32_t*>(ivf + o_cnt), nprobe, h->d_list_off,
									 h->d_list_rows, static_cast<uint32_t*>(c->d_bitmap.ptr), c->stream);
	});
}
int ivf_check(rxgpu_index* h, rxgpu_index* coarse, const char* who) {
	if (h->shard_set || coarse->shard_set) {
		set_error(std::string(who) + ": not available on a sharded index");
		return RXGPU_ERR_LOGIC;
	}
	RX_CHECK(h->nlist > 0 && h->lists_count == h->count, RXGPU_ERR_LOGIC, std::string(who) + ": inverted lists are not set / out of date");
	RX_CHECK(coarse->count == h->nlist && coarse->dim == h->dim && coarse->device == h->device, RXGPU_ERR_PARAMS,
			 std::string(who) + ": the coarse index must hold one centroid per list, same dimension, same device");
	return RXGPU_OK;
}
// ... and of the training calls, which run before there are lists: nlist is the coarse index's row count
int ivf_train_check(rxgpu_index* h, rxgpu_index* coarse, const char* who) {
	if (h->shard_set || coarse->shard_set) {
		set_error(std::string(who) + ": not available on a sharded index");
		return RXGPU_ERR_LOGIC;
	}
	RX_CHECK(coarse->count > 0 && coarse->count < 0xFFFFFFFFull && coarse->dim == h->dim && coarse->device == h->device, RXGPU_ERR_PARAMS,
			 std::string(who) + ": the coarse index must hold the centroids, same dimension, same device");
	return RXGPU_OK;
}

// An event pair on a stream: the device time of what a call enqueues between begin() and end() (read after the stream is idle).
struct IvfTimer {
	hipEvent_t a = nullptr, b = nullptr;
	~IvfTimer() {
		if (a) (void)hipEventDestroy(a);
		if (b) (void)hipEventDestroy(b);
	}
	hipError_t begin(hipStream_t s) {
		if (hipError_t e = hipEventCreate(&a); e != hipSuccess) return e;
		if (hipError_t e = hipEventCreate(&b); e != hipSuccess) return e;
		return hipEventRecord(a, s);
	}
	hipError_t end(hipStream_t s) { return hipEventRecord(b, s); }
	double ms() const {
		float v = 0.f;
		return hipEventElapsedTime(&v, a, b) == hipSuccess ? double(v) : 0.0;
	}
};

uint64_t ivf_gather_budget() {   // read per call (tests cut a small list into several chunks with it)
	const char* e = getenv("RXGPU_IVF_TRAIN_SCRATCH_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : rxgpu::kIvfGatherBudgetBytes;
}

// The row list of a training call on the host, before anything is launched: any order, repeats allowed, every id below the row count.
int ivf_check_ids(const rxgpu_index* h, const uint32_t* row_ids, uint64_t n, const char* who) {
	for (uint64_t i = 0; i < n; ++i) RX_CHECK(row_ids[i] < h->count, RXGPU_ERR_PARAMS, std::string(who) + ": row id out of range");
	return RXGPU_OK;
}

// Nearest centroid of n resident rows into c->d_out_row [n], all on c->stream: the rows listed in c->d_subset (listed) or rows [first_row,
// first_row + n).  The prepared vectors are gathered chunk by chunk (ivf_train_plan.h) into c->d_queries and searched by the chain that
// answers rxgpu_search_knn on the coarse index: the same bits, the same (dist, centroid) tie order.
int ivf_assign_enqueue(rxgpu_index* h, rxgpu_index* coarse, rxgpu_search_ctx* c, bool listed, uint64_t first_row, uint64_t n) {
	const uint64_t chunk_rows = rxgpu::ivf_gather_chunk_rows(n, h->dim, ivf_gather_budget());
	if (int rc = c->d_queries.ensure(chunk_rows * h->dim * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(n * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(chunk_rows * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_count.ensure(chunk_rows * sizeof(uint32_t)); rc) return rc;
	rxgpu_search_ctx* cc = stream_ctx(coarse, c->stream);
	const uint32_t* d_ids = listed ? static_cast<const uint32_t*>(c->d_subset.ptr) : nullptr;
	float* block = static_cast<float*>(c->d_queries.ptr);
	const uint64_t chunks = rxgpu::ivf_gather_chunks(n, chunk_rows);
	for (uint64_t i = 0; i < chunks; ++i) {
		const rxgpu::IvfChunk ch = rxgpu::ivf_gather_chunk(n, chunk_rows, i);
		{
			ProfileScope ps(h, "ivf_gather", c->stream);
			rxgpu::launch_ivf_gather(h->metric, h->d_rows, h->d_inv_norms, d_ids ? d_ids + ch.first : nullptr, first_row + ch.first, ch.rows, h->stride, h->dim, block,
									 h->cus, c->stream);
		}
		RX_HIP(hipGetLastError());
		if (int rc = enqueue_knn(coarse, cc, block, uint32_t(ch.rows), 1, static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr) + ch.first,
								 static_cast<uint32_t*>(c->d_out_count.ptr));
			rc)
			return rc;
	}
	return RXGPU_OK;
}
}  // namespace

int rxgpu_search_knn_lists(rxgpu_index* h, rxgpu_index* coarse, const float* query, uint32_t nprobe, uint32_t kk, float* out_dist,
						   uint32_t* out_row, uint32_t* out_count, uint64_t* out_scanned) {
	RX_CHECK(h && coarse && query && out_dist && out_row && out_count, RXGPU_ERR_PARAMS, "rxgpu_search_knn_lists: null argument");
	if (int rc = ivf_check(h, coarse, "rxgpu_search_knn_lists"); rc) return rc;
	if (out_scanned) *out_scanned = 0;
	*out_count = 0;
	if (h->count == 0 || kk == 0) return RXGPU_OK;
	nprobe = std::max<uint32_t>(1, std::min<uint32_t>(nprobe, h->nlist));
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	unsigned long long total = 0;
	if (int rc = ivf_probe_rows(h, coarse, c, query, nprobe, &total); rc) return rc;
	if (out_scanned) *out_scanned = total;
	if (total == 0) return RXGPU_OK;
	return search_subset_host(h, c, query, 1, kk, static_cast<const uint32_t*>(c->d_subset.ptr), total, out_dist, out_row, out_count);
}

namespace {
uint64_t ivf_batch_budget() {   // read per call (tests cut a call into several trains with it)
	const char* e = getenv("RXGPU_IVF_BATCH_SCRATCH_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : rxgpu::kIvfBatchScratchBytes;
}

// One device train over cq queries (host, prepared), all on c->stream: upload, coarse search, running chunk counts, list scan, merge, then one
// set of copies back through the context's pinned block and one wait.  Layout and gridx: ivf_batch_plan.h.
int ivf_batch_train(rxgpu_index* h, rxgpu_index* coarse, rxgpu_search_ctx* c, const float* queries, uint32_t cq, uint32_t nprobe, uint32_t kk, uint32_t gridx,
					float* out_dist, uint32_t* out_row, uint32_t* out_count, uint64_t* out_scanned) {
	const size_t qbytes = size_t(cq) * h->dim * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, queries, qbytes, hipMemcpyHostToDevice, c->stream));
	const rxgpu::IvfBatchScratch sc = rxgpu::ivf_batch_scratch(cq, nprobe);
	if (int rc = c->d_ivf.ensure(sc.bytes); rc) return rc;
	char* ivf = static_cast<char*>(c->d_ivf.ptr);
	uint32_t* probe = reinterpret_cast<uint32_t*>(ivf + sc.o_probe);
	uint32_t* pcnt = reinterpret_cast<uint32_t*>(ivf + sc.o_pcnt);
	uint32_t* cum = reinterpret_cast<uint32_t*>(ivf + sc.o_cum);
	unsigned long long* scanned = reinterpret_cast<unsigned long long*>(ivf + sc.o_scanned);
	const size_t part = size_t(cq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(cq) * kk * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(cq) * kk * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_count.ensure(size_t(cq) * sizeof(uint32_t)); rc) return rc;
	// the result's way back: [cq][kk] distances, [cq][kk] rows, [cq] rows probed, [cq] counts
	const size_t o_hrow = size_t(cq) * kk * sizeof(float), o_hscan = o_hrow + size_t(cq) * kk * sizeof(uint32_t), o_hcnt = o_hscan + size_t(cq) * sizeof(uint64_t);
	if (int rc = c->ensure_pinned(o_hcnt + size_t(cq) * sizeof(uint32_t)); rc) return rc;
	// 1. the coarse search: the chain that answers rxgpu_search_knn on the centroids, whatever nq (the single call's bits)
	rxgpu_search_ctx* cc = stream_ctx(coarse, c->stream);
	auto* run = nprobe <= uint32_t(rxgpu::kMaxFusedK) ? enqueue_knn : enqueue_knn_fused;
	if (int rc = run(coarse, cc, static_cast<const float*>(c->d_queries.ptr), cq, nprobe, reinterpret_cast<float*>(ivf + sc.o_pdist), probe, pcnt); rc) return rc;
	// 2. running chunk counts and rows probed
	{
		ProfileScope ps(h, "ivf_batch_offsets", c->stream);
		rxgpu::launch_ivf_batch_offsets(probe, pcnt, h->d_list_off, nprobe, cq, cum, scanned, c->stream);
	}
	// 3. the list scan, 4. the merge of its sorted partial lists
	rxgpu::ScanParams p{};
	p.rows = h->d_rows;
	p.inv_norms = h->d_inv_norms;
	p.queries = static_cast<const float*>(c->d_queries.ptr);
	p.stride = h->stride;
	p.dim = h->dim;
	p.kk = kk;
	p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	{
		ProfileScope ps(h, "scan_lists", c->stream);
		rxgpu::launch_scan_lists(h->metric, p, probe, cum, h->d_list_off, h->d_list_rows, nprobe, cq, gridx, c->stream);
	}
	{
		ProfileScope ps(h, "merge", c->stream);
		rxgpu::launch_merge_lists(p.part_dist, p.part_row, gridx, kk, cq, static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr),
								  static_cast<uint32_t*>(c->d_out_count.ptr), c->stream);
	}
	RX_HIP(hipGetLastError());
	char* hp = static_cast<char*>(c->h_pinned);
	RX_HIP(hipMemcpyAsync(hp, c->d_out_dist.ptr, o_hrow, hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipMemcpyAsync(hp + o_hrow, c->d_out_row.ptr, o_hscan - o_hrow, hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipMemcpyAsync(hp + o_hscan, scanned, o_hcnt - o_hscan, hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipMemcpyAsync(hp + o_hcnt, c->d_out_count.ptr, size_t(cq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	const float* hd = reinterpret_cast<const float*>(hp);
	const uint32_t* hr = reinterpret_cast<const uint32_t*>(hp + o_hrow);
	const uint64_t* hs = reinterpret_cast<const uint64_t*>(hp + o_hscan);
	const uint32_t* hc = reinterpret_cast<const uint32_t*>(hp + o_hcnt);
	for (uint32_t q = 0; q < cq; ++q) {   // what the single call writes: the first count entries
		const uint32_t n = std::min(hc[q], kk);
		std::memcpy(out_dist + size_t(q) * kk, hd + size_t(q) * kk, size_t(n) * sizeof(float));
		std::memcpy(out_row + size_t(q) * kk, hr + size_t(q) * kk, size_t(n) * sizeof(uint32_t));
		out_count[q] = n;
		if (out_scanned) out_scanned[q] = hs[q];
	}
	return RXGPU_OK;
}
}  // namespace

int rxgpu_search_knn_lists_batch(rxgpu_index* h, rxgpu_index* coarse, const float* queries, uint32_t nq, uint32_t nprobe, uint32_t kk, float* out_dist,
								 uint32_t* out_row, uint32_t* out_count, uint64_t* out_scanned) {
	RX_CHECK(h && coarse && (nq == 0 || (queries && out_dist && out_row && out_count)), RXGPU_ERR_PARAMS, "rxgpu_search_knn_lists_batch: null argument");
	if (int rc = ivf_check(h, coarse, "rxgpu_search_knn_lists_batch"); rc) return rc;
	if (nq == 0) return RXGPU_OK;
	std::fill(out_count, out_count + nq, 0u);
	if (out_scanned) std::fill(out_scanned, out_scanned + nq, uint64_t(0));
	if (h->count == 0 || kk == 0) return RXGPU_OK;
	nprobe = std::max<uint32_t>(1, std::min<uint32_t>(nprobe, h->nlist));
	uint64_t trains = 0, one_by_one = 0;
	int rc = RXGPU_OK;
	if (!rxgpu::ivf_batch_on_device(nprobe, kk)) {   // outside the envelope: the single call's chain per query, inside this call
		for (uint32_t q = 0; q < nq && rc == RXGPU_OK; ++q, ++one_by_one) {
			rc = rxgpu_search_knn_lists(h, coarse, queries + size_t(q) * h->dim, nprobe, kk, out_dist + size_t(q) * kk, out_row + size_t(q) * kk, out_count + q,
										out_scanned ? out_scanned + q : nullptr);
		}
	} else {
		DeviceGuard dg(h->device);
		rxgpu_search_ctx* c = acquire_ctx(h);
		if (!c) return RXGPU_ERR_DEVICE;
		CtxLease lease{h, c};
		const uint32_t gridx = rxgpu::ivf_batch_grid_x(nq, nprobe, h->nlist, h->lists_rows, h->lists_longest, uint32_t(h->cus));
		const uint32_t per = rxgpu::ivf_batch_train_queries(nq, h->dim, nprobe, kk, gridx, ivf_batch_budget());
		for (uint32_t q0 = 0; q0 < nq && rc == RXGPU_OK; q0 += per, ++trains) {
			rc = ivf_batch_train(h, coarse, c, queries + size_t(q0) * h->dim, std::min(per, nq - q0), nprobe, kk, gridx, out_dist + size_t(q0) * kk,
								 out_row + size_t(q0) * kk, out_count + q0, out_scanned ? out_scanned + q0 : nullptr);
		}
	}
	std::lock_guard<std::mutex> lk(h->mtx);
	h->ivf_batch_calls += 1;
	h->ivf_batch_queries += nq;
	h->ivf_batch_trains += trains;
	h->ivf_batch_one_by_one += one_by_one;
	return rc;
}

int rxgpu_ivf_batch_default(uint32_t nq, uint32_t nprobe, uint32_t kk) { return rxgpu::ivf_batch_default_on_device(nq, nprobe, kk) ? 1 : 0; }

int rxgpu_ivf_read_batch_stats(rxgpu_index* h, uint64_t* calls, uint64_t* queries, uint64_t* trains, uint64_t* queries_one_by_one) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	std::lock_guard<std::mutex> lk(h->mtx);
	if (calls) *calls = h->ivf_batch_calls;
	if (queries) *queries = h->ivf_batch_queries;
	if (trains) *trains = h->ivf_batch_trains;
	if (queries_one_by_one) *queries_one_by_one = h->ivf_batch_one_by_one;
	h->ivf_batch_calls = h->ivf_batch_queries = h->ivf_batch_trains = h->ivf_batch_one_by_one = 0;
	return RXGPU_OK;
}

int rxgpu_search_range_lists(rxgpu_index* h, rxgpu_index* coarse, const float* query, uint32_t nprobe, float radius, int inclusive, float* out_dist,
							 uint32_t* out_row, uint64_t cap, uint64_t* out_total, uint64_t* out_scanned) {
	RX_CHECK(h && coarse && query && out_total && (cap == 0 || (out_dist && out_row)), RXGPU_ERR_PARAMS, "rxgpu_search_range_lists: null argument");
	if (int rc = ivf_check(h, coarse, "rxgpu_search_range_lists"); rc) return rc;
	if (out_scanned) *out_scanned = 0;
	*out_total = 0;
	if (h->count == 0) return RXGPU_OK;
	nprobe = std::max<uint32_t>(1, std::min<uint32_t>(nprobe, h->nlist));
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	unsigned long long total = 0;
	if (int rc = ivf_probe_rows(h, coarse, c, query, nprobe, &total); rc) return rc;
	if (out_scanned) *out_scanned = total;
	if (total == 0) return RXGPU_OK;
	return range_on_device(h, c, true, total, radius, inclusive, out_dist, out_row, cap, out_total, "rxgpu_search_range_lists");
}

// add_with_ids' list assignment (and the closing one of train) for rows the index holds: gather + the coarse quantiser's k = 1 search, the
// answer back in one copy.
int rxgpu_ivf_assign(rxgpu_index* h, rxgpu_index* coarse, const uint32_t* row_ids, uint64_t first_row, uint64_t n, uint32_t* out_list) {
	RX_CHECK(h && coarse, RXGPU_ERR_PARAMS, "rxgpu_ivf_assign: null argument");
	if (int rc = ivf_train_check(h, coarse, "rxgpu_ivf_assign"); rc) return rc;
	if (n == 0) return RXGPU_OK;
	RX_CHECK(out_list, RXGPU_ERR_PARAMS, "rxgpu_ivf_assign: null argument");
	RX_CHECK(n < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "rxgpu_ivf_assign: too many rows");
	if (row_ids) {
		if (int rc = ivf_check_ids(h, row_ids, n, "rxgpu_ivf_assign"); rc) return rc;
	} else {
		RX_CHECK(first_row <= h->count && n <= h->count - first_row, RXGPU_ERR_PARAMS, "rxgpu_ivf_assign: the row range must stay below the row count");
	}
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (row_ids) {
		if (int rc = c->d_subset.ensure(n * sizeof(uint32_t)); rc) return rc;
		RX_HIP(hipMemcpyAsync(c->d_subset.ptr, row_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	}
	IvfTimer timer;
	RX_HIP(timer.begin(c->stream));
	if (int rc = ivf_assign_enqueue(h, coarse, c, row_ids != nullptr, row_ids ? 0 : first_row, n); rc) return rc;
	RX_HIP(timer.end(c->stream));
	RX_HIP(hipMemcpyAsync(out_list, c->d_out_row.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	std::lock_guard<std::mutex> lk(h->mtx);
	h->ivf_dev_rows += n;
	h->ivf_dev_ms += timer.ms();
	return RXGPU_OK;
}

// One k-means iteration's device half (Clustering.cpp:153-230 behind the assignment): the listed rows (or the first n) -> nearest centroid
// -> per-centroid segments in list order -> ordered sums x 1 / count.  split_clusters and the spherical renormalisation stay with the caller.
int rxgpu_ivf_kmeans_step(rxgpu_index* h, rxgpu_index* coarse, const uint32_t* row_ids, uint64_t n, float* out_centroids, float* out_hassign, uint32_t* out_assign) {
	RX_CHECK(h && coarse && out_centroids && out_hassign, RXGPU_ERR_PARAMS, "rxgpu_ivf_kmeans_step: null argument");
	if (int rc = ivf_train_check(h, coarse, "rxgpu_ivf_kmeans_step"); rc) return rc;
	RX_CHECK(rxgpu::ivf_train_points_ok(n), RXGPU_ERR_PARAMS, "rxgpu_ivf_kmeans_step: a step takes fewer than 2^24 points");
	const uint32_t nlist = uint32_t(coarse->count);
	if (n == 0) {
		std::fill(out_centroids, out_centroids + size_t(nlist) * h->dim, 0.f);
		std::fill(out_hassign, out_hassign + nlist, 0.f);
		return RXGPU_OK;
	}
	if (row_ids) {
		if (int rc = ivf_check_ids(h, row_ids, n, "rxgpu_ivf_kmeans_step"); rc) return rc;
	} else {
		RX_CHECK(n <= h->count, RXGPU_ERR_PARAMS, "rxgpu_ivf_kmeans_step: more points than the index holds rows");
	}
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	const rxgpu::IvfTrainScratch sc = rxgpu::ivf_train_scratch(n, nlist, h->dim);
	if (int rc = c->d_misc.ensure(sc.bytes); rc) return rc;
	char* base = static_cast<char*>(c->d_misc.ptr);
	uint32_t* table = reinterpret_cast<uint32_t*>(base + sc.o_table);
	uint32_t* seg_off = reinterpret_cast<uint32_t*>(base + sc.o_seg_off);
	uint32_t* seg_rows = reinterpret_cast<uint32_t*>(base + sc.o_seg_rows);
	float* centroids = reinterpret_cast<float*>(base + sc.o_centroids);
	float* hassign = reinterpret_cast<float*>(base + sc.o_hassign);
	uint32_t* flag = reinterpret_cast<uint32_t*>(base + sc.o_flag);
	if (row_ids) {
		if (int rc = c->d_subset.ensure(n * sizeof(uint32_t)); rc) return rc;
		RX_HIP(hipMemcpyAsync(c->d_subset.ptr, row_ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	}
	const uint32_t* d_ids = row_ids ? static_cast<const uint32_t*>(c->d_subset.ptr) : nullptr;
	IvfTimer timer, sums;
	RX_HIP(timer.begin(c->stream));
	if (int rc = ivf_assign_enqueue(h, coarse, c, row_ids != nullptr, 0, n); rc) return rc;
	const uint32_t* assign = static_cast<const uint32_t*>(c->d_out_row.ptr);
	RX_HIP(hipMemsetAsync(table, 0, sc.o_seg_off - sc.o_table, c->stream));
	RX_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
	{
		ProfileScope ps(h, "ivf_place", c->stream);
		rxgpu::launch_ivf_place(assign, d_ids, uint32_t(n), nlist, table, seg_off, seg_rows, hassign, flag, c->stream);
	}
	RX_HIP(hipGetLastError());
	RX_HIP(sums.begin(c->stream));
	{
		ProfileScope ps(h, "ivf_sums", c->stream);
		rxgpu::launch_ivf_centroid_sums(h->metric, h->d_rows, h->d_inv_norms, h->stride, h->dim, nlist, seg_off, seg_rows, centroids, c->stream);
	}
	RX_HIP(hipGetLastError());
	RX_HIP(sums.end(c->stream));
	RX_HIP(timer.end(c->stream));
	uint32_t bad = 0;
	RX_HIP(hipMemcpyAsync(out_centroids, centroids, size_t(nlist) * h->dim * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipMemcpyAsync(out_hassign, hassign, size_t(nlist) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	if (out_assign) RX_HIP(hipMemcpyAsync(out_assign, assign, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipMemcpyAsync(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	RX_CHECK(bad == 0, RXGPU_ERR_LOGIC, "rxgpu_ivf_kmeans_step: a point found no centroid (non-finite rows are outside the contract)");
	std::lock_guard<std::mutex> lk(h->mtx);
	h->ivf_dev_rows += n;
	h->ivf_dev_steps += 1;
	h->ivf_dev_ms += timer.ms();
	h->ivf_sums_ms += sums.ms();
	return RXGPU_OK;
}

int rxgpu_ivf_read_train_stats(rxgpu_index* h, uint64_t* rows_assigned, uint64_t* steps, double* kernel_ms, double* sums_ms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	std::lock_guard<std::mutex> lk(h->mtx);
	if (rows_assigned) *rows_assigned = h->ivf_dev_rows;
	if (steps) *steps = h->ivf_dev_steps;
	if (kernel_ms) *kernel_ms = h->ivf_dev_ms;
	if (sums_ms) *sums_ms = h->ivf_sums_ms;
	h->ivf_dev_rows = 0;
	h->ivf_dev_steps = 0;
	h->ivf_dev_ms = 0.0;
	h->ivf_sums_ms = 0.0;
	return RXGPU_OK;
}

int rxgpu_search_knn_subset_device(rxgpu_index* h, const void* d_queries, uint32_t nq, uint32_t kk, const void* d_row_ids, uint64_t n_ids,
								   void* d_out_dist, void* d_out_row, void* d_out_count, void* stream) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_search_knn_subset_device: not available on a sharded index");
	RX_CHECK(nq > 0 && d_queries && d_row_ids && d_out_dist && d_out_row, RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset_device: null argument");
	RX_CHECK(kk > 0 && kk <= uint32_t(rxgpu::kMaxFusedK2), RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset_device: kk must be in [1, 128]");
	RX_CHECK(n_ids > 0 && n_ids <= h->count, RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset_device: the row list must hold 1..count entries");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = stream_ctx(h, stream);
	return enqueue_knn_subset(h, c, static_cast<const float*>(d_queries), nq, kk, static_cast<const uint32_t*>(d_row_ids), n_ids,
							  static_cast<float*>(d_out_dist), static_cast<uint32_t*>(d_out_row), static_cast<uint32_t*>(d_out_count));
}

int rxgpu_check_row_list_device(rxgpu_index* h, const void* d_row_ids, uint64_t n_ids, void* stream, int32_t* out_ok) {
	RX_CHECK(h && out_ok && (n_ids == 0 || d_row_ids), RXGPU_ERR_PARAMS, "rxgpu_check_row_list_device: null argument");
	*out_ok = 1;
	if (n_ids == 0) return RXGPU_OK;
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = stream_ctx(h, stream);
	if (int rc = c->d_tiles.ensure(sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemsetAsync(c->d_tiles.ptr, 0, sizeof(uint32_t), c->stream));
	rxgpu::launch_check_row_list(static_cast<const uint32_t*>(d_row_ids), n_ids, h->count, static_cast<uint32_t*>(c->d_tiles.ptr), h->cus, c->stream);
	RX_HIP(hipGetLastError());
	uint32_t bad = 0;
	RX_HIP(hipMemcpyAsync(&bad, c->d_tiles.ptr, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	*out_ok = bad ? 0 : 1;
	return RXGPU_OK;
}

int rxgpu_merge_shards_device(const void* d_gathered, uint32_t world, uint32_t nq, uint32_t kk, uint32_t shard_rows, void* d_out_dist,
							  void* d_out_row, void* d_out_count, void* stream) {
	RX_CHECK(d_gathered && d_out_dist && d_out_row, RXGPU_ERR_PARAMS, "rxgpu_merge_shards_device: null argument");
	RX_CHECK(world >= 1 && nq >= 1 && kk >= 1 && kk <= uint32_t(rxgpu::kMaxFusedK), RXGPU_ERR_PARAMS, "rxgpu_merge_shards_device: bad shape");
	RX_CHECK(uint64_t(world) * shard_rows <= 0xFFFFFFFEull, RXGPU_ERR_PARAMS, "rxgpu_merge_shards_device: global rows must fit 32 bits");
	rxgpu::launch_merge_shards(static_cast<const uint32_t*>(d_gathered), world, nq, kk, shard_rows, static_cast<float*>(d_out_dist),
							   static_cast<uint32_t*>(d_out_row), static_cast<uint32_t*>(d_out_count), static_cast<hipStream_t>(stream));
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

int rxgpu_search_range(rxgpu_index* h, const float* query, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
					   uint64_t* out_total) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query && out_total && (cap == 0 || (out_dist && out_row)), RXGPU_ERR_PARAMS, "rxgpu_search_range: null argument");
	*out_total = 0;
	// (a sharded call that overflows leaves the first cap hits in the buffers, the tail below writes none: both are kept)
	if (h->shard_set) return rxgpu::sharded_search_range_impl(h, query, radius, inclusive, nullptr, 0, out_dist, out_row, cap, out_total);
	if (h->count == 0) return RXGPU_OK;   // bruteforce.cc:132-134
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_queries.ensure(h->dim * sizeof(float)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, h->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
	return range_on_device(h, c, false, h->count, radius, inclusive, out_dist, out_row, cap, out_total, "rxgpu_search_range");
}

int rxgpu_search_range_subset(rxgpu_index* h, const float* query, float radius, int inclusive, const uint32_t* row_ids, uint64_t n_ids,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query && out_total && (cap == 0 || (out_dist && out_row)) && (n_ids == 0 || row_ids), RXGPU_ERR_PARAMS,
			 "rxgpu_search_range_subset: null argument");
	*out_total = 0;
	if (h->shard_set) {   // (the fan-out checks the row list, with a message of its own)
		if (n_ids == 0) return RXGPU_OK;
		return rxgpu::sharded_search_range_impl(h, query, radius, inclusive, row_ids, n_ids, out_dist, out_row, cap, out_total);
	}
	if (int rc = check_rows_host(h, row_ids, n_ids, "rxgpu_search_range_subset"); rc) return rc;
	if (n_ids == 0) return RXGPU_OK;
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_queries.ensure(h->dim * sizeof(float)); rc) return rc;
	if (int rc = c->d_subset.ensure(n_ids * sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, h->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
	RX_HIP(hipMemcpyAsync(c->d_subset.ptr, row_ids, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	return range_on_device(h, c, true, n_ids, radius, inclusive, out_dist, out_row, cap, out_total, "rxgpu_search_range_subset");
}

int rxgpu_distances(rxgpu_index* h, const float* query, const uint32_t* rows, uint32_t n, float* out_dist) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query && (n == 0 || (rows && out_dist)), RXGPU_ERR_PARAMS, "rxgpu_distances: null argument");
	if (n == 0) return RXGPU_OK;
	if (h->shard_set) return rxgpu::sharded_distances(h, query, rows, n, out_dist);
	for (uint32_t i = 0; i < n; ++i) RX_CHECK(rows[i] < h->count, RXGPU_ERR_PARAMS, "rxgpu_distances: row out of range");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_queries.ensure(h->dim * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(n) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(n) * sizeof(float)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, h->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
	RX_HIP(hipMemcpyAsync(c->d_out_row.ptr, rows, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	{
		ProfileScope ps(h, "distances", c->stream);
		rxgpu::launch_distances(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr), h->stride, h->dim,
							static_cast<const uint32_t*>(c->d_out_row.ptr), n, static_cast<float*>(c->d_out_dist.ptr), c->stream);
	}
	RX_HIP(hipGetLastError());
	RX_HIP(hipMemcpyAsync(out_dist, c->d_out_dist.ptr, size_t(n) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	return RXGPU_OK;
}

}  // extern "C"
