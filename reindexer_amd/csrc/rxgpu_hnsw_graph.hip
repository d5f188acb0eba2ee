// C-ABI implementation (include/rxgpu.h), the HNSW host side: the graph mirror (attach, patch, update_deleted) and the SQ8 code table beside it
// (upload, attach, quantize on the device, read back).  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/rxgpu.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::set_error;

namespace {
// The code table of h with room for `rows` rows (the three entry points that write it come through here).  It is allocated for the index
// CAPACITY, like the float rows; where it has to grow — the first rows, or the index was reserved larger since — the rows that have codes
// are copied into the new one.  + 4 bytes: the word loads of the last row's last block stay inside the allocation whatever dim % 4 is.
// The caller has quiesced the resident kernel and holds the device.
int sq8_table_ensure(rxgpu_index* h, uint64_t rows, const char* who) {
	if (h->sq8_cap >= rows) return RXGPU_OK;
	const uint64_t cap = std::max<uint64_t>(h->capacity, h->count);
	RX_HIP(rxgpu::device_wait_all(h->device));
	uint8_t* nc = nullptr;
	float* nr = nullptr;
	RX_HIP(hipMalloc(reinterpret_cast<void**>(&nc), size_t(cap) * h->dim + 4));
	if (hipMalloc(reinterpret_cast<void**>(&nr), size_t(cap) * sizeof(float)) != hipSuccess) {
		(void)hipFree(nc);
		set_error(std::string(who) + ": not enough memory for the corrective offsets");
		return RXGPU_ERR_NOMEM;
	}
	if (h->sq8_n) {
		RX_HIP(hipMemcpy(nc, h->d_codes, size_t(h->sq8_n) * h->dim, hipMemcpyDeviceToDevice));
		RX_HIP(hipMemcpy(nr, h->d_corr, size_t(h->sq8_n) * sizeof(float), hipMemcpyDeviceToDevice));
	}
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_corr) (void)hipFree(h->d_corr);
	h->d_codes = nc;
	h->d_corr = nr;
	h->sq8_cap = cap;
	return RXGPU_OK;
}
}  // namespace

extern "C" {

/* ------------------------------------------------------------------------------------------------ graph mirror */

int rxgpu_hnsw_attach_graph(rxgpu_index* h, const uint32_t* links0, const uint64_t* upper_off, const uint32_t* upper, uint64_t upper_blocks,
							const uint8_t* deleted, uint32_t M, uint32_t max_m0, int32_t maxlevel, uint32_t entry, uint64_t num_deleted) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_attach_graph: a sharded index holds one graph per shard — attach to the rxgpu_index_shard(h, s) handles");
	const uint64_t n = h->count;
	RX_CHECK(n == 0 || (links0 && upper_off && deleted), RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: null argument");
	RX_CHECK(upper_blocks == 0 || upper, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: upper is null");
	RX_CHECK(M >= 1 && max_m0 <= uint32_t(rxgpu::kHnswMaxNeighbors) && M <= max_m0, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_attach_graph: the GPU engine supports M <= 64 (2*M <= 128)");
	RX_CHECK(n == 0 || entry < n, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: entry point out of range");
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	// allocated for the index CAPACITY (and with headroom for upper-level blocks), so that rxgpu_hnsw_patch_graph can grow the graph in place
	auto replace = [&](auto*& dst, const void* src, size_t bytes, size_t cap_bytes) -> int {
		if (dst) (void)hipFree(dst);
		dst = nullptr;
		if (cap_bytes == 0) return RXGPU_OK;
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&dst), cap_bytes));
		if (bytes) RX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
		return RXGPU_OK;
	};
	h->graph_attached = false;
	const uint64_t rows_cap = std::max<uint64_t>(std::max<uint64_t>(h->capacity, n), 1);
	// expected upper blocks of a full index: sum over levels of cap / M^level = cap / (M - 1); twice that (and at least what is there) as headroom
	uint64_t upper_cap = std::max<uint64_t>(2 * upper_blocks + 64, 2 * rows_cap / std::max<uint32_t>(M - 1, 1) + 64);
	// RXGPU_HNSW_UPPER_HEADROOM=<blocks> (read per attach; tests): that many blocks beyond the attached ones instead — the way to meet
	// RXGPU_ERR_OVERFLOW of the patch entry points, which the default headroom keeps out of reach
	if (const char* e = std::getenv("RXGPU_HNSW_UPPER_HEADROOM"); e && *e) {
		char* end = nullptr;
		const unsigned long long x = std::strtoull(e, &end, 10);
		if (end != e && *end == 0 && x > 0) upper_cap = upper_blocks + x;
	}
	const size_t row_bytes = (1 + size_t(max_m0)) * sizeof(uint32_t), blk_bytes = (1 + size_t(M)) * sizeof(uint32_t);
	if (int rc = replace(h->d_links0, links0, n * row_bytes, rows_cap * row_bytes); rc) return rc;
	if (int rc = replace(h->d_upper_off, upper_off, n ? (n + 1) * sizeof(uint64_t) : 0, (rows_cap + 1) * sizeof(uint64_t)); rc) return rc;
	if (int rc = replace(h->d_upper, upper, upper_blocks * blk_bytes, upper_cap * blk_bytes); rc) return rc;
	if (int rc = replace(h->d_deleted, deleted, n, rows_cap); rc) return rc;
	h->graph_rows_cap = rows_cap;
	h->graph_upper_cap = upper_cap;
	h->graph_upper_used = upper_blocks;
	if (!h->d_hnsw_stats) {
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_hnsw_stats), 8 * sizeof(unsigned long long)));   // evals, hops, in-kernel restarts, spare, [4..7] phase cycles (RXGPU_HNSW_PHASES builds)
		RX_HIP(hipMemset(h->d_hnsw_stats, 0, 8 * sizeof(unsigned long long)));
	}
	h->graph_n = n;
	h->graph_upper_nodes = n;
	h->build_upper_end = 0;   // level-1 lists of a build batch that were not patched in are gone with the arrays
	h->graph_M = M;
	h->graph_maxM0 = max_m0;
	h->graph_maxlevel = maxlevel;
	h->graph_entry = entry;
	h->graph_deleted = num_deleted;
	h->graph_attached = true;
	return RXGPU_OK;
}

int rxgpu_hnsw_patch_graph(rxgpu_index* h, uint32_t n_dirty, const uint32_t* dirty_ids, const uint32_t* links0_rows, const uint8_t* deleted_flags,
						   const int32_t* levels, const uint32_t* upper_rows, int32_t maxlevel, uint32_t entry, uint64_t num_deleted) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_graph: no graph attached");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	RX_CHECK(n_dirty == 0 || (dirty_ids && links0_rows && deleted_flags && levels), RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: null argument");
	const uint64_t n_new = h->count;   // the rows were uploaded first (rxgpu_index_upload_rows)
	RX_CHECK(n_new >= h->graph_n, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_graph: the index shrank under the graph");
	RX_CHECK(n_new == 0 || entry < n_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: entry point out of range");
	RX_CHECK(n_new <= h->graph_rows_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_patch_graph: the graph arrays were allocated for fewer rows (re-attach the graph)");
	// staging: ids, per-node upper placement, lists — one buffer, one upload, one scatter launch
	const uint32_t M = h->graph_M, max_m0 = h->graph_maxM0;
	const size_t stride0 = 1 + size_t(max_m0), stride = 1 + size_t(M);
	std::vector<uint64_t> upper_at(n_dirty);
	std::vector<uint32_t> upper_src(n_dirty);
	uint64_t used = h->graph_upper_used, staged_blocks = 0, next_new = h->graph_n;
	for (uint32_t j = 0; j < n_dirty; ++j) {
		RX_CHECK(dirty_ids[j] < n_new && levels[j] >= 0, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: node id / level out of range");
		upper_src[j] = uint32_t(staged_blocks);
		staged_blocks += uint64_t(levels[j]);
		if (dirty_ids[j] >= h->graph_n) {   // a new node: ids ascending, every one of them listed (its blocks are appended in id order)
			RX_CHECK(dirty_ids[j] == next_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: new nodes must be listed in ascending id order, none skipped");
			++next_new;
			upper_at[j] = used;
			used += uint64_t(levels[j]);
		} else {
			upper_at[j] = ~uint64_t(0);
		}
	}
	RX_CHECK(next_new == n_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: every new node must be listed");
	RX_CHECK(staged_blocks == 0 || upper_rows, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: upper_rows is null");
	RX_CHECK(used <= h->graph_upper_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_patch_graph: upper-level storage exhausted (re-attach the graph)");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	RX_HIP(rxgpu::device_wait_all(h->device));   // no search may be reading the lists while they change (the Map calls this under its writer lock)
	auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
	const size_t o_ids = 0, o_at = al(o_ids + size_t(n_dirty) * 4), o_src = al(o_at + size_t(n_dirty) * 8), o_lv = al(o_src + size_t(n_dirty) * 4),
				 o_l0 = al(o_lv + size_t(n_dirty) * 4), o_up = al(o_l0 + size_t(n_dirty) * stride0 * 4), o_del = al(o_up + staged_blocks * stride * 4),
				 total = al(o_del + n_dirty);
	if (n_dirty) {
		if (int rc = c->d_misc.ensure(total); rc) return rc;
		if (int rc = c->ensure_pinned(total); rc) return rc;
		char* hp = static_cast<char*>(c->h_pinned);
		std::memcpy(hp + o_ids, dirty_ids, size_t(n_dirty) * 4);
		std::memcpy(hp + o_at, upper_at.data(), size_t(n_dirty) * 8);
		std::memcpy(hp + o_src, upper_src.data(), size_t(n_dirty) * 4);
		std::memcpy(hp + o_lv, levels, size_t(n_dirty) * 4);
		std::memcpy(hp + o_l0, links0_rows, size_t(n_dirty) * stride0 * 4);
		if (staged_blocks) std::memcpy(hp + o_up, upper_rows, staged_blocks * stride * 4);
		std::memcpy(hp + o_del, deleted_flags, n_dirty);
		char* db = static_cast<char*>(c->d_misc.ptr);
		RX_HIP(hipMemcpyAsync(db, hp, total, hipMemcpyHostToDevice, c->stream));
		rxgpu::HnswPatch p{};
		p.ids = reinterpret_cast<const uint32_t*>(db + o_ids);
		p.upper_at = reinterpret_cast<const uint64_t*>(db + o_at);
		p.upper_src = reinterpret_cast<const uint32_t*>(db + o_src);
		p.levels = reinterpret_cast<const int32_t*>(db + o_lv);
		p.src_links0 = reinterpret_cast<const uint32_t*>(db + o_l0);
		p.src_upper = reinterpret_cast<const uint32_t*>(db + o_up);
		p.src_deleted = reinterpret_cast<const uint8_t*>(db + o_del);
		p.links0 = h->d_links0;
		p.upper_off = h->d_upper_off;
		p.upper = h->d_upper;
		p.deleted = h->d_deleted;
		p.M = M;
		p.maxM0 = max_m0;
		rxgpu::launch_hnsw_patch(p, n_dirty, c->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(c->stream));
	}
	h->graph_upper_used = used;
	h->graph_n = n_new;
	h->graph_upper_nodes = n_new;
	h->build_upper_end = 0;
	h->graph_maxlevel = maxlevel;
	h->graph_entry = entry;
	h->graph_deleted = num_deleted;
	return RXGPU_OK;
}

int rxgpu_hnsw_update_deleted(rxgpu_index* h, const uint8_t* deleted, uint64_t num_deleted) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_update_deleted: no graph attached");
	RX_CHECK(deleted || h->graph_n == 0, RXGPU_ERR_PARAMS, "rxgpu_hnsw_update_deleted: null argument");
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	if (h->graph_n) RX_HIP(hipMemcpy(h->d_deleted, deleted, h->graph_n, hipMemcpyHostToDevice));
	h->graph_deleted = num_deleted;
	return RXGPU_OK;
}

/* ------------------------------------------------------------------------------------------------ SQ8 code table */

// Rows [first_row, first_row + n) of the code table: the device side of a point added to / updated in a quantised graph (addPoint with a
// quantizer, hnswalg.h:1480-1495).  The table is allocated for the index CAPACITY (like the rows), so an upsert is a copy of its own D + 4
// bytes, not a re-upload of the table.
int rxgpu_hnsw_upload_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const uint8_t* codes, const float* corr, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_upload_sq8_rows: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(codes && corr, RXGPU_ERR_PARAMS, "rxgpu_hnsw_upload_sq8_rows: null argument");
	RX_CHECK(first_row <= h->sq8_n && first_row + n <= h->count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_upload_sq8_rows: rows follow the table without a hole and stay below count");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads what changes (or moves) here
	DeviceGuard dg(h->device);
	if (int rc = sq8_table_ensure(h, first_row + n, "rxgpu_hnsw_upload_sq8_rows"); rc) return rc;
	RX_HIP(hipMemcpy(h->d_codes + size_t(first_row) * h->dim, codes, size_t(n) * h->dim, hipMemcpyHostToDevice));
	RX_HIP(hipMemcpy(h->d_corr + first_row, corr, size_t(n) * sizeof(float), hipMemcpyHostToDevice));
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = std::max<uint64_t>(h->sq8_n, first_row + n);
	return RXGPU_OK;
}

int rxgpu_hnsw_attach_sq8(rxgpu_index* h, const uint8_t* codes, const float* corr, uint64_t count, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_attach_sq8: not available on a sharded index");
	RX_CHECK(count == h->count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_sq8: one code row per index row");
	RX_CHECK(count == 0 || (codes && corr), RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_sq8: null argument");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads the tables freed below
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_corr) (void)hipFree(h->d_corr);
	h->d_codes = nullptr;
	h->d_corr = nullptr;
	h->sq8_n = 0;
	h->sq8_cap = 0;
	if (count) {
		// a fresh table, sized by the index capacity: rows added later are patched in (rxgpu_hnsw_upload_sq8_rows / rxgpu_hnsw_quantize_sq8)
		if (int rc = sq8_table_ensure(h, count, "rxgpu_hnsw_attach_sq8"); rc) return rc;
		RX_HIP(hipMemcpy(h->d_codes, codes, size_t(count) * h->dim, hipMemcpyHostToDevice));
		RX_HIP(hipMemcpy(h->d_corr, corr, size_t(count) * sizeof(float), hipMemcpyHostToDevice));
	}
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = count;
	return RXGPU_OK;
}

// Quantizer::quantize where the rows are (hnsw_sq8_quantize.hip): what the Map used to compute on one host thread and upload — on the first
// Quantize, on every re-quantisation, after every bulk change — is one pass over rows the device already holds.
int rxgpu_hnsw_quantize_sq8(rxgpu_index* h, uint64_t first_row, uint64_t n, float min_q, float alpha, float delta, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_quantize_sq8: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(first_row <= h->sq8_n && first_row <= h->count && n <= h->count - first_row, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_quantize_sq8: rows follow the table without a hole and stay below count");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads what changes (or moves) here
	DeviceGuard dg(h->device);
	if (int rc = sq8_table_ensure(h, first_row + n, "rxgpu_hnsw_quantize_sq8"); rc) return rc;
	hipEvent_t a = nullptr, b = nullptr;
	RX_HIP(hipEventCreate(&a));
	if (hipError_t e = hipEventCreate(&b); e != hipSuccess) {
		(void)hipEventDestroy(a);
		RX_HIP(e);
	}
	float ms = 0.f;
	hipError_t e = hipEventRecord(a, nullptr);
	if (e == hipSuccess) {
		rxgpu::launch_hnsw_sq8_quantize(h->metric, h->d_rows, h->stride, h->dim, first_row, n, min_q, alpha, delta, h->d_codes, h->d_corr, nullptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipEventRecord(b, nullptr);
	if (e == hipSuccess) e = hipEventSynchronize(b);
	if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	RX_HIP(e);
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = std::min<uint64_t>(h->count, std::max<uint64_t>(h->sq8_n, first_row + n));   // codes behind a count that shrank since are no rows
	h->sq8_dev_rows += n;
	h->sq8_dev_launches += 1;
	h->sq8_dev_ms += double(ms);
	return RXGPU_OK;
}

int rxgpu_hnsw_read_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, uint8_t* out_codes, float* out_corr) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_sq8_rows: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(first_row <= h->sq8_n && n <= h->sq8_n - first_row, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_sq8_rows: rows without codes");
	rxgpu::hnsw_server_quiesce(h);   // a copy on the default stream would wait for the resident kernel's lifetime
	DeviceGuard dg(h->device);
	if (out_codes) RX_HIP(hipMemcpy(out_codes, h->d_codes + size_t(first_row) * h->dim, size_t(n) * h->dim, hipMemcpyDeviceToHost));
	if (out_corr) RX_HIP(hipMemcpy(out_corr, h->d_corr + first_row, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
	return RXGPU_OK;
}

int rxgpu_hnsw_read_sq8_quantize_stats(rxgpu_index* h, uint64_t* rows, uint64_t* launches, double* kernel_ms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (rows) *rows = h->sq8_dev_rows;
	if (launches) *launches = h->sq8_dev_launches;
	if (kernel_ms) *kernel_ms = h->sq8_dev_ms;
	h->sq8_dev_rows = 0;
	h->sq8_dev_launches = 0;
	h->sq8_dev_ms = 0.0;
	return RXGPU_OK;
}

}  // extern "C"
