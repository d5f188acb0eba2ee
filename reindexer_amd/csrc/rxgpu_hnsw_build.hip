// C-ABI implementation (include/rxgpu.h), the batched level-0 build of an HNSW graph: one batch of stored rows is searched against the
// graph before it (the search entry points' own code, results kept in HBM), given its lists (hnsw_build_select) and linked back
// (hnsw_build_backlink) — hnsw_build.hip.  What a batch is, and the layout of its scratch: hnsw_build_plan.h.  The upper levels are built
// on the host and arrive through rxgpu_hnsw_patch_upper — or, level 1, on the device under the same rule (rxgpu_hnsw_link_batch_upper):
// the level-1 lists are gathered into a dense view with the shape of a level-0 array (hnsw_build_upper.hip), the search runs over the
// handle with that view swapped in as its base layer, and the same selection and back-link kernels run on the view; the levels >= 2 then
// arrive through rxgpu_hnsw_patch_upper_from.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/rxgpu.h"
#include "hnsw_build.h"
#include "hnsw_build_plan.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::set_error;

namespace {

// an event pair on one stream; ms() after the stream was waited for
struct EventPair {
	hipEvent_t a = nullptr, b = nullptr;
	~EventPair() {
		if (a) (void)hipEventDestroy(a);
		if (b) (void)hipEventDestroy(b);
	}
	hipError_t create() {
		if (hipError_t e = hipEventCreate(&a); e != hipSuccess) return e;
		return hipEventCreate(&b);
	}
	double ms() const {
		float v = 0.f;
		return hipEventElapsedTime(&v, a, b) == hipSuccess ? double(v) : 0.0;
	}
};

// the areas of one batch's scratch (at sb) as the kernels take them; the caller fills in the graph and the batch
void scratch_args(rxgpu_index* h, const rxgpu::HnswBuildScratch& scr, char* sb, rxgpu::HnswBuildArgs& a) {
	a.pair_t = reinterpret_cast<uint32_t*>(sb + scr.o_pair_t);
	a.node_cnt = static_cast<uint32_t*>(h->build_nodes.ptr);
	a.node_seg = a.node_cnt + h->build_nodes_cap;
	a.touched = reinterpret_cast<uint32_t*>(sb + scr.o_touched);
	a.tcnt = reinterpret_cast<uint32_t*>(sb + scr.o_tcnt);
	a.tseg = reinterpret_cast<uint32_t*>(sb + scr.o_tseg);
	a.inc = reinterpret_cast<uint32_t*>(sb + scr.o_inc);
	a.over = reinterpret_cast<uint2*>(sb + scr.o_over);
	a.over_cap = uint32_t(scr.over_cap);
	a.big_id = reinterpret_cast<uint32_t*>(sb + scr.o_big_id);
	a.big_dist = reinterpret_cast<float*>(sb + scr.o_big_dist);
	a.big_pos = reinterpret_cast<uint32_t*>(sb + scr.o_big_pos);
	a.big_cap = uint32_t(scr.big_cap);
	a.counters = reinterpret_cast<uint32_t*>(sb + scr.o_counters);
}

// the two per-node words of the pair grouping, for the graph's row capacity, all zero
int ensure_build_nodes(rxgpu_index* h, const rxgpu::HnswBuildScratch& scr) {
	if (h->build_nodes_cap < h->graph_rows_cap) {
		if (int rc = h->build_nodes.ensure(scr.node_bytes); rc) return rc;
		RX_HIP(hipMemset(h->build_nodes.ptr, 0, scr.node_bytes));
		h->build_nodes_cap = h->graph_rows_cap;
	}
	return RXGPU_OK;
}

// Steps 4 and 5 of a batch on the lists a.links0 ([..][1 + a.maxM0]): the lists of the batch's rows, the pairs grouped by target, the
// back-links, and — never truncated — the second launch for the nodes past the kernel's cap.  Waits for the stream; counters [8] = kBuildCnt*.
int select_and_link_back(rxgpu_index* h, const rxgpu::HnswBuildArgs& a, const rxgpu::HnswBuildScratch& scr, hipStream_t st, const char* corrupt_msg,
						 const char* overflow_msg, uint32_t* counters, double* select_ms, double* back_ms) {
	EventPair select_ev, back_ev, big_ev;
	RX_HIP(select_ev.create());
	RX_HIP(back_ev.create());
	RX_HIP(big_ev.create());
	RX_HIP(hipEventRecord(select_ev.a, st));
	rxgpu::launch_hnsw_build_select(h->metric, a, st);
	rxgpu::launch_hnsw_build_group(a, st);
	RX_HIP(hipEventRecord(select_ev.b, st));
	RX_HIP(hipEventRecord(back_ev.a, st));
	rxgpu::launch_hnsw_build_backlink(h->metric, a, st);
	RX_HIP(hipEventRecord(back_ev.b, st));
	RX_HIP(hipGetLastError());
	RX_HIP(hipMemcpyAsync(counters, a.counters, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	RX_HIP(hipStreamSynchronize(st));
	RX_CHECK(counters[rxgpu::kBuildCntError] != 2, RXGPU_ERR_DEVICE, corrupt_msg);
	RX_CHECK(counters[rxgpu::kBuildCntError] == 0 && counters[rxgpu::kBuildCntOver] <= scr.over_cap, RXGPU_ERR_DEVICE, overflow_msg);
	*select_ms = select_ev.ms();
	*back_ms = back_ev.ms();
	if (counters[rxgpu::kBuildCntOver]) {   // never truncated: the nodes past the cap are finished by a second launch
		RX_HIP(hipEventRecord(big_ev.a, st));
		rxgpu::launch_hnsw_build_backlink_big(h->metric, a, counters[rxgpu::kBuildCntOver], st);
		RX_HIP(hipEventRecord(big_ev.b, st));
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpyAsync(counters, a.counters, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));   // (the re-selections of this launch count too)
		RX_HIP(hipStreamSynchronize(st));
		RX_CHECK(counters[rxgpu::kBuildCntError] == 0, RXGPU_ERR_DEVICE, corrupt_msg);
		*back_ms += big_ev.ms();
	}
	return RXGPU_OK;
}

// The level-1 lists as the graph's base layer for the length of one search: level 0 is the dense view (lists of M entries), the upper
// blocks begin one block later — so that the descent's address upper_off[cur] + level - 1 lands on the levels >= 2 — and the top level is
// one lower.  The graph counts the nodes in front of the batch, as the search does.
struct LevelOneAsBase {
	rxgpu_index* h;
	uint32_t* links0;
	uint32_t* upper;
	uint32_t max_m0;
	int maxlevel;
	uint64_t graph_n;
	LevelOneAsBase(rxgpu_index* h_, uint32_t* view, uint64_t nodes)
		: h(h_), links0(h_->d_links0), upper(h_->d_upper), max_m0(h_->graph_maxM0), maxlevel(h_->graph_maxlevel), graph_n(h_->graph_n) {
		h->d_links0 = view;
		h->d_upper = upper ? upper + (1 + size_t(h->graph_M)) : nullptr;
		h->graph_maxM0 = h->graph_M;
		h->graph_maxlevel = maxlevel - 1;
		h->graph_n = nodes;
	}
	~LevelOneAsBase() {
		h->d_links0 = links0;
		h->d_upper = upper;
		h->graph_maxM0 = max_m0;
		h->graph_maxlevel = maxlevel;
		h->graph_n = graph_n;
	}
};

rxgpu::HnswUpperView upper_view(rxgpu_index* h, uint64_t nodes) {
	rxgpu::HnswUpperView v{};
	v.view = static_cast<uint32_t*>(h->build_view.ptr);
	v.upper_off = h->d_upper_off;
	v.upper = h->d_upper;
	v.upper_used = h->graph_upper_used;
	v.nodes = uint32_t(nodes);
	v.M = h->graph_M;
	return v;
}

}  // namespace

extern "C" {

int rxgpu_hnsw_link_batch(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t ef_construction) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch: not available on a sharded index");
	RX_CHECK(h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch: no graph attached");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(first_row == h->graph_n && first_row >= 1, RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch: a batch starts at the attached node count (>= 1)");
	RX_CHECK(h->graph_upper_nodes == h->graph_n, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch: the upper lists of the batch before were not patched in (rxgpu_hnsw_patch_upper)");
	RX_CHECK(n <= h->count - std::min(h->count, first_row), RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch: the rows of the batch must be uploaded first");
	RX_CHECK(n <= rxgpu::kHnswBuildBatchCap * 4, RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch: at most 65536 rows a batch");
	const int path = rxgpu::hnsw_build_path(h->graph_deleted, h->graph_M, ef_construction, false);
	RX_CHECK(path == rxgpu::kHnswBuildDevice, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_link_batch: the device build takes graphs without deleted nodes, M <= 64 and efConstruction <= 256");
	RX_CHECK(first_row + n <= h->graph_rows_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_link_batch: the graph arrays were allocated for fewer rows (re-attach the graph)");
	RX_CHECK(h->metric != RXGPU_METRIC_COSINE || h->d_inv_norms, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch: cosine index without norms");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads the lists that change here
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	const uint32_t M = h->graph_M, max_m0 = h->graph_maxM0;
	const uint32_t k = uint32_t(std::min<uint64_t>(ef_construction, first_row));
	const bool pack = h->stride != h->dim;
	const rxgpu::HnswBuildScratch scr = rxgpu::hnsw_build_scratch(n, M, max_m0, k, h->dim, pack, h->graph_rows_cap);
	if (int rc = h->build_scratch.ensure(scr.bytes); rc) return rc;
	if (int rc = ensure_build_nodes(h, scr); rc) return rc;
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	hipStream_t st = c->stream;
	char* sb = static_cast<char*>(h->build_scratch.ptr);
	uint32_t* d_counters = reinterpret_cast<uint32_t*>(sb + scr.o_counters);
	RX_HIP(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint32_t), st));
	RX_HIP(hipMemsetAsync(h->d_deleted + first_row, 0, n, st));
	// step 3: the stored rows are the queries, where they are (packed first where the row stride is padded)
	const float* d_q = h->d_rows + first_row * h->stride;
	if (pack) {
		RX_HIP(hipMemcpy2DAsync(sb + scr.o_queries, size_t(h->dim) * 4, d_q, size_t(h->stride) * 4, size_t(h->dim) * 4, n, hipMemcpyDeviceToDevice, st));
		d_q = reinterpret_cast<const float*>(sb + scr.o_queries);
	}
	RX_HIP(hipStreamSynchronize(st));
	rxgpu::HnswSink sink{reinterpret_cast<uint32_t*>(sb + scr.o_cand_dist), reinterpret_cast<uint32_t*>(sb + scr.o_cand_row), k};
	const auto t0 = std::chrono::steady_clock::now();
	if (int rc = rxgpu::hnsw_search_rows_to_sink(h, d_q, uint32_t(n), k, ef_construction, first_row, sink); rc) return rc;   // (drains its stream)
	const double search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	// steps 4 and 5
	rxgpu::HnswBuildArgs a{};
	a.rows = h->d_rows;
	a.inv_norms = h->d_inv_norms;
	a.stride = h->stride;
	a.dim = h->dim;
	a.links0 = h->d_links0;
	a.M = M;
	a.maxM0 = max_m0;
	a.first = uint32_t(first_row);
	a.n = uint32_t(n);
	a.cand_row = sink.d_row;
	a.k = k;
	a.lds_rows = rxgpu::hnsw_build_select_lds(h->stride, M).kept_in_lds ? 1u : 0u;
	a.id_end = uint32_t(first_row + n);
	scratch_args(h, scr, sb, a);
	uint32_t counters[8] = {0};
	double select_ms = 0.0, back_ms = 0.0;
	if (int rc = select_and_link_back(h, a, scr, st, "rxgpu_hnsw_link_batch: a level-0 list names a node past the batch (corrupt graph)",
									  "rxgpu_hnsw_link_batch: the queue of nodes past the kernel's cap overflowed", counters, &select_ms, &back_ms);
		rc)
		return rc;
	h->graph_n = first_row + n;
	h->build_rows += n;
	h->build_batches += 1;
	h->build_reselected += counters[rxgpu::kBuildCntReselected];
	h->build_over += counters[rxgpu::kBuildCntOver];
	h->build_ms[0] += search_ms;
	h->build_ms[1] += select_ms;
	h->build_ms[2] += back_ms;
	return RXGPU_OK;
}

int rxgpu_hnsw_link_batch_upper(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t n_up, const uint32_t* up_rows, uint32_t ef_construction) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: not available on a sharded index");
	RX_CHECK(h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: no graph attached");
	RX_CHECK(n >= 1 && first_row >= 1 && h->graph_n == first_row + n, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_link_batch_upper: not the batch rxgpu_hnsw_link_batch linked last (level 0 of the batch comes first)");
	RX_CHECK(h->graph_upper_nodes == first_row, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: the upper lists of the batch are patched in already");
	RX_CHECK(h->build_upper_end != first_row + n, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: level 1 of the batch is linked already");
	RX_CHECK(h->graph_maxlevel >= 1, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: the graph in front of the batch has no level 1 (the host links such a batch)");
	RX_CHECK(n_up == 0 || up_rows, RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch_upper: null argument");
	for (uint32_t r = 0; r < n_up; ++r) {
		RX_CHECK(up_rows[r] >= first_row && up_rows[r] < first_row + n, RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch_upper: a row outside the batch");
		RX_CHECK(r == 0 || up_rows[r - 1] < up_rows[r], RXGPU_ERR_PARAMS, "rxgpu_hnsw_link_batch_upper: the rows must be ascending");
	}
	const int path = rxgpu::hnsw_build_path(h->graph_deleted, h->graph_M, ef_construction, false);
	RX_CHECK(path == rxgpu::kHnswBuildDevice, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_link_batch_upper: the device build takes graphs without deleted nodes, M <= 64 and efConstruction <= 256");
	RX_CHECK(h->metric != RXGPU_METRIC_COSINE || h->d_inv_norms, RXGPU_ERR_LOGIC, "rxgpu_hnsw_link_batch_upper: cosine index without norms");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads the lists that change here
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	const uint32_t M = h->graph_M;
	const uint32_t k = uint32_t(std::min<uint64_t>(ef_construction, first_row));
	const rxgpu::HnswBuildUpperScratch us = rxgpu::hnsw_build_upper_scratch(n_up, M, k, h->dim, h->graph_rows_cap);
	const rxgpu::HnswBuildScratch& scr = us.batch;
	if (int rc = h->build_scratch.ensure(us.bytes); rc) return rc;
	if (int rc = ensure_build_nodes(h, scr); rc) return rc;
	if (int rc = h->build_view.ensure(rxgpu::hnsw_build_upper_view_bytes(h->graph_rows_cap, M)); rc) return rc;
	if (n_up == 0) return RXGPU_OK;   // no row of level >= 1: no list changes
	h->build_upper_end = 0;
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	hipStream_t st = c->stream;
	char* sb = static_cast<char*>(h->build_scratch.ptr);
	uint32_t* d_counters = reinterpret_cast<uint32_t*>(sb + scr.o_counters);
	uint32_t* d_row_ids = reinterpret_cast<uint32_t*>(sb + us.o_row_ids);
	float* d_q = reinterpret_cast<float*>(sb + scr.o_queries);
	RX_HIP(hipMemsetAsync(d_counters, 0, 8 * sizeof(uint32_t), st));
	RX_HIP(hipMemcpyAsync(d_row_ids, up_rows, size_t(n_up) * 4, hipMemcpyHostToDevice, st));
	// the level-1 lists of the graph in front of the batch as a dense array, and the rows of U packed as queries
	const rxgpu::HnswUpperView view = upper_view(h, first_row);
	rxgpu::launch_hnsw_upper_view_gather(view, st);
	RX_HIP(hipMemsetAsync(view.view + first_row * (1 + size_t(M)), 0, n * (1 + size_t(M)) * sizeof(uint32_t), st));   // the batch's rows: empty until selected
	rxgpu::launch_hnsw_upper_pack_rows(h->d_rows, h->stride, h->dim, d_row_ids, n_up, d_q, st);
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(st));
	rxgpu::HnswSink sink{reinterpret_cast<uint32_t*>(sb + scr.o_cand_dist), reinterpret_cast<uint32_t*>(sb + scr.o_cand_row), k};
	const auto t0 = std::chrono::steady_clock::now();
	{
		LevelOneAsBase swapped(h, view.view, first_row);
		if (int rc = rxgpu::hnsw_search_rows_to_sink(h, d_q, n_up, k, ef_construction, first_row, sink); rc) return rc;   // (drains its stream)
	}
	const double search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	rxgpu::HnswBuildArgs a{};
	a.rows = h->d_rows;
	a.inv_norms = h->d_inv_norms;
	a.stride = h->stride;
	a.dim = h->dim;
	a.links0 = view.view;
	a.M = M;
	a.maxM0 = M;
	a.first = uint32_t(first_row);
	a.n = n_up;
	a.row_ids = d_row_ids;
	a.id_end = uint32_t(first_row + n);
	a.cand_row = sink.d_row;
	a.k = k;
	a.lds_rows = rxgpu::hnsw_build_select_lds(h->stride, M).kept_in_lds ? 1u : 0u;
	scratch_args(h, scr, sb, a);
	uint32_t counters[8] = {0};
	double select_ms = 0.0, back_ms = 0.0;
	if (int rc = select_and_link_back(h, a, scr, st, "rxgpu_hnsw_link_batch_upper: a level-1 list names a node past the batch (corrupt graph)",
									  "rxgpu_hnsw_link_batch_upper: the queue of nodes past the kernel's cap overflowed", counters, &select_ms, &back_ms);
		rc)
		return rc;
	// the lists of the older nodes that took links go back into their blocks; those of U stay in the view until rxgpu_hnsw_patch_upper_from
	// has given the new nodes their blocks
	rxgpu::launch_hnsw_upper_view_store(view, a.touched, d_counters, uint32_t(scr.pairs), st);
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(st));
	h->build_upper_end = first_row + n;
	h->build_upper_last = n_up;
	h->build_upper_rows += n_up;
	h->build_upper_reselected += counters[rxgpu::kBuildCntReselected];
	h->build_upper_over += counters[rxgpu::kBuildCntOver];
	h->build_upper_ms[0] += search_ms;
	h->build_upper_ms[1] += select_ms;
	h->build_upper_ms[2] += back_ms;
	return RXGPU_OK;
}

int rxgpu_hnsw_patch_upper(rxgpu_index* h, uint32_t n_nodes, const uint32_t* ids, const int32_t* levels, const uint32_t* upper_rows, int32_t maxlevel,
						   uint32_t entry) {
	return rxgpu_hnsw_patch_upper_from(h, 1, n_nodes, ids, levels, upper_rows, maxlevel, entry);
}

int rxgpu_hnsw_patch_upper_from(rxgpu_index* h, int32_t first_level, uint32_t n_nodes, const uint32_t* ids, const int32_t* levels, const uint32_t* upper_rows,
								int32_t maxlevel, uint32_t entry) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_upper: no graph attached");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_upper: not available on a sharded index");
	RX_CHECK(first_level == 1 || first_level == 2, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper_from: the first level is 1 or 2");
	RX_CHECK(n_nodes == 0 || (ids && levels), RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: null argument");
	RX_CHECK(h->graph_n == 0 || entry < h->graph_n, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: entry point out of range");
	rxgpu::hnsw_server_quiesce(h);
	const uint32_t M = h->graph_M;
	const size_t stride = 1 + size_t(M);
	const uint32_t skip = uint32_t(first_level - 1);   // blocks of a node in front of the first staged one
	std::vector<uint64_t> upper_at(n_nodes);
	std::vector<uint32_t> upper_src(n_nodes);
	std::vector<uint32_t> from_view;   // first_level 2: the new nodes of level >= 1, whose level-1 list the device built
	uint64_t used = h->graph_upper_used, staged_blocks = 0, next_new = h->graph_upper_nodes;
	for (uint32_t j = 0; j < n_nodes; ++j) {
		RX_CHECK(ids[j] < h->graph_n && levels[j] >= 0, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: node id / level out of range");
		upper_src[j] = uint32_t(staged_blocks);
		staged_blocks += uint64_t(levels[j]) > skip ? uint64_t(levels[j]) - skip : 0;
		if (ids[j] >= h->graph_upper_nodes) {   // a node of the batch: ids ascending, every one of them listed (its blocks are appended in id order)
			RX_CHECK(ids[j] == next_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: new nodes must be listed in ascending id order, none skipped");
			++next_new;
			upper_at[j] = used;
			used += uint64_t(levels[j]);
			if (skip && levels[j] >= 1) from_view.push_back(ids[j]);
		} else {
			upper_at[j] = ~uint64_t(0);
		}
	}
	RX_CHECK(next_new == h->graph_n, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: every node of the batch must be listed");
	RX_CHECK(from_view.empty() || (h->build_upper_end == h->graph_n && h->build_upper_last == from_view.size() && h->build_view.ptr), RXGPU_ERR_LOGIC,
			 "rxgpu_hnsw_patch_upper_from: level 1 of the batch's rows was not linked on the device (rxgpu_hnsw_link_batch_upper over every row of level >= 1)");
	RX_CHECK(staged_blocks == 0 || upper_rows, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_upper: upper_rows is null");
	RX_CHECK(used <= h->graph_upper_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_patch_upper: upper-level storage exhausted (re-attach the graph)");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	RX_HIP(rxgpu::device_wait_all(h->device));
	auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
	const size_t o_ids = 0, o_at = al(o_ids + size_t(n_nodes) * 4), o_src = al(o_at + size_t(n_nodes) * 8), o_lv = al(o_src + size_t(n_nodes) * 4),
				 o_up = al(o_lv + size_t(n_nodes) * 4), o_fv = al(o_up + staged_blocks * stride * 4), total = al(o_fv + from_view.size() * 4);
	if (n_nodes) {
		if (int rc = c->d_misc.ensure(total); rc) return rc;
		if (int rc = c->ensure_pinned(total); rc) return rc;
		char* hp = static_cast<char*>(c->h_pinned);
		std::memcpy(hp + o_ids, ids, size_t(n_nodes) * 4);
		std::memcpy(hp + o_at, upper_at.data(), size_t(n_nodes) * 8);
		std::memcpy(hp + o_src, upper_src.data(), size_t(n_nodes) * 4);
		std::memcpy(hp + o_lv, levels, size_t(n_nodes) * 4);
		if (staged_blocks) std::memcpy(hp + o_up, upper_rows, staged_blocks * stride * 4);
		if (!from_view.empty()) std::memcpy(hp + o_fv, from_view.data(), from_view.size() * 4);
		char* db = static_cast<char*>(c->d_misc.ptr);
		RX_HIP(hipMemcpyAsync(db, hp, total, hipMemcpyHostToDevice, c->stream));
		rxgpu::HnswUpperPatch p{};
		p.ids = reinterpret_cast<const uint32_t*>(db + o_ids);
		p.upper_at = reinterpret_cast<const uint64_t*>(db + o_at);
		p.upper_src = reinterpret_cast<const uint32_t*>(db + o_src);
		p.levels = reinterpret_cast<const int32_t*>(db + o_lv);
		p.src_upper = reinterpret_cast<const uint32_t*>(db + o_up);
		p.upper_off = h->d_upper_off;
		p.upper = h->d_upper;
		p.M = M;
		p.skip = skip;
		rxgpu::launch_hnsw_build_patch_upper(p, n_nodes, c->stream);
		if (!from_view.empty()) {   // the blocks of the new nodes exist now: their level-1 lists out of the view
			rxgpu::HnswUpperView v = upper_view(h, h->graph_n);
			v.upper_used = used;
			rxgpu::launch_hnsw_upper_view_store_ids(v, reinterpret_cast<const uint32_t*>(db + o_fv), uint32_t(from_view.size()), c->stream);
		}
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(c->stream));
	}
	h->build_upper_end = 0;
	h->graph_upper_used = used;
	h->graph_upper_nodes = h->graph_n;
	h->graph_maxlevel = maxlevel;
	h->graph_entry = entry;
	return RXGPU_OK;
}

int rxgpu_hnsw_read_links0(rxgpu_index* h, uint64_t first_row, uint64_t n, uint32_t* out) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_links0: no graph attached");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_links0: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(out, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_links0: null argument");
	RX_CHECK(first_row <= h->graph_n && n <= h->graph_n - first_row, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_links0: rows past the attached node count");
	rxgpu::hnsw_server_quiesce(h);   // a copy on the default stream would wait for the resident kernel's lifetime
	DeviceGuard dg(h->device);
	const size_t row_words = 1 + size_t(h->graph_maxM0);
	RX_HIP(hipMemcpy(out, h->d_links0 + first_row * row_words, n * row_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return RXGPU_OK;
}

int rxgpu_hnsw_read_level(rxgpu_index* h, int32_t level, uint64_t n_ids, const uint32_t* ids, uint32_t* out) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_level: no graph attached");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_level: not available on a sharded index");
	RX_CHECK(level >= 1, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_level: levels >= 1 (level 0: rxgpu_hnsw_read_links0)");
	if (n_ids == 0) return RXGPU_OK;
	RX_CHECK(ids && out, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_level: null argument");
	const uint64_t nodes = h->graph_upper_nodes;
	// between rxgpu_hnsw_link_batch_upper and the patch the level-1 lists of the batch's rows live in the view: readable from there
	const uint64_t view_end = level == 1 && h->build_upper_end > nodes && h->build_view.ptr ? h->build_upper_end : nodes;
	for (uint64_t j = 0; j < n_ids; ++j) RX_CHECK(ids[j] < view_end, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_level: a node whose upper lists are not mirrored");
	rxgpu::hnsw_server_quiesce(h);   // a copy on the default stream would wait for the resident kernel's lifetime
	DeviceGuard dg(h->device);
	const size_t stride = 1 + size_t(h->graph_M);
	std::vector<uint32_t> pending((view_end - nodes) * stride);
	if (!pending.empty())
		RX_HIP(hipMemcpy(pending.data(), static_cast<const uint32_t*>(h->build_view.ptr) + nodes * stride, pending.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	std::vector<uint64_t> off(nodes + 1);
	RX_HIP(hipMemcpy(off.data(), h->d_upper_off, nodes * sizeof(uint64_t), hipMemcpyDeviceToHost));
	off[nodes] = h->graph_upper_used;
	std::vector<uint32_t> upper(h->graph_upper_used * stride);
	if (!upper.empty()) RX_HIP(hipMemcpy(upper.data(), h->d_upper, upper.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	for (uint64_t j = 0; j < n_ids; ++j) {
		uint32_t* dst = out + j * stride;
		if (ids[j] >= nodes) {
			std::memcpy(dst, pending.data() + (ids[j] - nodes) * stride, stride * sizeof(uint32_t));
			continue;
		}
		const uint64_t at = off[ids[j]], end = off[ids[j] + 1];
		if (end > at && uint64_t(level) <= end - at && at + uint64_t(level) <= h->graph_upper_used) {
			std::memcpy(dst, upper.data() + (at + uint64_t(level) - 1) * stride, stride * sizeof(uint32_t));
		} else {
			std::memset(dst, 0, stride * sizeof(uint32_t));   // the node does not reach the level: an empty list
		}
	}
	return RXGPU_OK;
}

int rxgpu_hnsw_release_build_view(rxgpu_index* h) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(h->build_upper_end == 0, RXGPU_ERR_LOGIC, "rxgpu_hnsw_release_build_view: the view holds level-1 lists that are not patched in yet");
	if (!h->build_view.ptr) return RXGPU_OK;
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	h->build_view.release();
	return RXGPU_OK;
}

int rxgpu_hnsw_read_build_upper_stats(rxgpu_index* h, uint64_t* rows, uint64_t* reselected, uint64_t* past_cap, double* phase_ms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (rows) *rows = h->build_upper_rows;
	if (reselected) *reselected = h->build_upper_reselected;
	if (past_cap) *past_cap = h->build_upper_over;
	if (phase_ms) std::copy(h->build_upper_ms, h->build_upper_ms + 3, phase_ms);
	h->build_upper_rows = h->build_upper_reselected = h->build_upper_over = 0;
	std::fill(h->build_upper_ms, h->build_upper_ms + 3, 0.0);
	return RXGPU_OK;
}

int rxgpu_hnsw_read_build_stats(rxgpu_index* h, uint64_t* rows, uint64_t* batches, uint64_t* reselected, uint64_t* past_cap, double* phase_ms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (rows) *rows = h->build_rows;
	if (batches) *batches = h->build_batches;
	if (reselected) *reselected = h->build_reselected;
	if (past_cap) *past_cap = h->build_over;
	if (phase_ms) std::copy(h->build_ms, h->build_ms + 3, phase_ms);
	h->build_rows = h->build_batches = h->build_reselected = h->build_over = 0;
	std::fill(h->build_ms, h->build_ms + 3, 0.0);
	return RXGPU_OK;
}

}  // extern "C"
