// C-ABI implementation (include/rxgpu.h): the error slot, retired buffers, search contexts, index storage in HBM and its mutations,
// instrumentation.  The search entry points are rxgpu_knn_search.hip.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/rxgpu.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace rxgpu

using rxgpu::set_error;

namespace rxgpu {
// hipFree / hipHostFree wait for the whole device — and a resident search kernel (rxgpu_hnsw_server.hip) stays on it for up to its lifetime:
// a scratch buffer that grew on some thread's launch path stalled that thread for tens of milliseconds (measured: T = 16 planner threads over
// 10M rows, 7 of 1024 queries took the launches, the leg lasted 73 ms instead of 47).  While such a kernel may be alive, buffers that are
// replaced are retired instead and freed at the next point that waits for the device anyway (a mutation, a quiesce, index destruction),
// or when 256 MB have piled up.
std::atomic<int> g_resident_kernels{0};
namespace {
std::mutex g_retired_mtx;
std::vector<std::pair<void*, bool>> g_retired;   // (pointer, host memory?)
size_t g_retired_bytes = 0;
}  // namespace
void drain_retired() {
	std::vector<std::pair<void*, bool>> take;
	{
		std::lock_guard<std::mutex> lk(g_retired_mtx);
		take.swap(g_retired);
		g_retired_bytes = 0;
	}
	for (const auto& e : take) {
		if (e.second) {
			(void)hipHostFree(e.first);
		} else {
			(void)hipFree(e.first);
		}
	}
}
void free_or_retire(void* ptr, size_t bytes, bool host) {
	if (!ptr) return;
	if (g_resident_kernels.load(std::memory_order_acquire) <= 0) {
		if (host) {
			(void)hipHostFree(ptr);
		} else {
			(void)hipFree(ptr);
		}
		return;
	}
	bool drain = false;
	{
		std::lock_guard<std::mutex> lk(g_retired_mtx);
		g_retired.emplace_back(ptr, host);
		g_retired_bytes += bytes;
		drain = g_retired_bytes > (size_t(256) << 20);
	}
	if (drain) drain_retired();
}
// hipDeviceSynchronize for a device that may hold resident search kernels: they are told to leave first — the wait would otherwise last
// until their idle / lifetime limit
hipError_t device_wait_all(int device) {
	hnsw_servers_pause_device(device);
	const hipError_t e = hipDeviceSynchronize();
	drain_retired();
	return e;
}
}  // namespace rxgpu

int rxgpu_devbuf::ensure(size_t need) {
	if (need <= bytes) return RXGPU_OK;
	rxgpu::free_or_retire(ptr, bytes, false);
	ptr = nullptr;
	bytes = 0;
	const size_t want = std::max<size_t>(need, 4096);
	RX_HIP(hipMalloc(&ptr, want));
	bytes = want;
	// RXGPU_DEBUG_FILL=<byte>: every fresh scratch buffer is filled with it (a read before the first write then shows, whatever the allocator returned)
	static const int fill = [] {
		const char* e = std::getenv("RXGPU_DEBUG_FILL");
		return e ? int(std::strtol(e, nullptr, 0)) & 0xFF : -1;
	}();
	if (fill >= 0) RX_HIP(hipMemset(ptr, fill, want));
	return RXGPU_OK;
}
void rxgpu_devbuf::release() {
	rxgpu::free_or_retire(ptr, bytes, false);
	ptr = nullptr;
	bytes = 0;
}
int rxgpu_search_ctx::ensure_pinned(size_t need) {
	if (need <= h_pinned_bytes) return RXGPU_OK;
	rxgpu::free_or_retire(h_pinned, h_pinned_bytes, true);
	h_pinned = nullptr;
	h_pinned_bytes = 0;
	const size_t want = std::max<size_t>(need, 1 << 16);
	RX_HIP(hipHostMalloc(&h_pinned, want, hipHostMallocDefault));
	h_pinned_bytes = want;
	return RXGPU_OK;
}
int rxgpu_search_ctx::ensure_aux() {
	if (aux_stream) return RXGPU_OK;
	RX_HIP(hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking));
	RX_HIP(hipStreamCreateWithFlags(&aux2_stream, hipStreamNonBlocking));
	RX_HIP(hipEventCreateWithFlags(&split_done, hipEventDisableTiming));
	RX_HIP(hipEventCreateWithFlags(&aux_done, hipEventDisableTiming));
	RX_HIP(hipEventCreateWithFlags(&main_done, hipEventDisableTiming));
	return RXGPU_OK;
}
void rxgpu_search_ctx::release() {
	if (aux_done) (void)hipEventDestroy(aux_done);
	if (main_done) (void)hipEventDestroy(main_done);
	if (split_done) (void)hipEventDestroy(split_done);
	if (aux_stream) (void)hipStreamDestroy(aux_stream);
	if (aux2_stream) (void)hipStreamDestroy(aux2_stream);
	aux_done = main_done = split_done = nullptr;
	aux_stream = aux2_stream = nullptr;
	d_queries.release();
	d_part_dist.release();
	d_part_row.release();
	d_out_dist.release();
	d_out_row.release();
	d_out_count.release();
	d_misc.release();
	d_select.release();
	d_qpad.release();
	d_qstats.release();
	d_dense.release();
	d_cand_row.release();
	d_cand_dist.release();
	d_cand_cnt.release();
	d_visited.release();
	d_helper.release();
	d_helper_bits.release();
	d_ivf.release();
	d_gcand_d.release();
	d_redo.release();
	d_allowed.release();
	d_top.release();
	d_qplanes.release();
	d_emit.release();
	d_emit_cnt.release();
	d_seed.release();
	d_subset.release();
	d_bitmap.release();
	d_tiles.release();
	if (h_pinned) (void)hipHostFree(h_pinned);
	h_pinned = nullptr;
	if (own_stream && stream) (void)hipStreamDestroy(stream);
	stream = nullptr;
}

namespace rxgpu {
// Check out a scratch context with its own stream (host-synchronous searches).
rxgpu_search_ctx* acquire_ctx(rxgpu_index* h) {
	{
		std::lock_guard<std::mutex> lk(h->mtx);
		if (!h->free_ctx.empty()) {
			auto* c = h->free_ctx.back();
			h->free_ctx.pop_back();
			return c;
		}
	}
	auto* c = new rxgpu_search_ctx();
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
		delete c;
		set_error("hipStreamCreateWithFlags failed");
		return nullptr;
	}
	c->own_stream = true;
	return c;
}
void release_ctx(rxgpu_index* h, rxgpu_search_ctx* c) {
	std::lock_guard<std::mutex> lk(h->mtx);
	h->free_ctx.push_back(c);
}
ProfileScope::ProfileScope(rxgpu_index* h_, const char* n, hipStream_t s_) : h(h_), name(n), s(s_) {
	if (!h->profiling) return;
	if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
		a = b = nullptr;
		return;
	}
	(void)hipEventRecord(a, s);
}
ProfileScope::~ProfileScope() {
	if (!a) return;
	(void)hipEventRecord(b, s);
	std::lock_guard<std::mutex> lk(h->mtx);
	h->profile[name].events.emplace_back(a, b);
}
}  // namespace rxgpu

using rxgpu::DeviceGuard;
using rxgpu::release_ctx;

namespace {

// Resident contexts are per calling thread (rxgpu_search_knn_resident).  Planner threads come and go: a thread that ends hands the contexts it
// held back to the pools of the indexes that still exist — looked up by serial number, never through a pointer the thread kept — so short-lived
// threads neither pile up streams + device buffers until rxgpu_index_destroy nor leave their context to a later thread that got the same id.
std::mutex g_live_mtx;
std::map<uint64_t, rxgpu_index*> g_live_indexes;
std::atomic<uint64_t> g_index_serial{0};
struct ResidentThread {
	std::vector<uint64_t> used;
	~ResidentThread() {
		std::lock_guard<std::mutex> live(g_live_mtx);
		for (uint64_t serial : used) {
			auto it = g_live_indexes.find(serial);
			if (it == g_live_indexes.end()) continue;
			rxgpu_index* h = it->second;
			rxgpu_search_ctx* c = nullptr;
			{
				std::lock_guard<std::mutex> lk(h->resident_mtx);
				auto slot = h->resident_ctx.find(std::this_thread::get_id());
				if (slot == h->resident_ctx.end()) continue;
				c = slot->second;
				h->resident_ctx.erase(slot);
			}
			if (c) release_ctx(h, c);   // its stream orders the next user's work behind whatever this thread left running
		}
	}
};
thread_local ResidentThread t_resident;
void register_live_index(rxgpu_index* h) {
	std::lock_guard<std::mutex> live(g_live_mtx);
	h->serial = ++g_index_serial;
	g_live_indexes[h->serial] = h;
}
void unregister_live_index(rxgpu_index* h) {
	std::lock_guard<std::mutex> live(g_live_mtx);
	g_live_indexes.erase(h->serial);
}

}  // namespace

namespace rxgpu {
void resident_thread_uses(rxgpu_index* h) { t_resident.used.push_back(h->serial); }
}  // namespace rxgpu

extern "C" {

const char* rxgpu_last_error(void) { return rxgpu::g_err.c_str(); }
int rxgpu_abi_version(void) { return RXGPU_ABI_VERSION; }

int rxgpu_scan_policy(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite) {
	return rxgpu::scan_policy_pruned(rows, dim, nq, shadow_available != 0, stats_finite != 0) ? 1 : 0;
}

int rxgpu_scan_tier(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite) {
	return int(rxgpu::scan_policy_tier(rows, dim, nq, shadow_available != 0, shadow_available != 0, stats_finite != 0));
}

int rxgpu_scan_i6(uint64_t rows, uint32_t dim, uint32_t nq, int i6_available, int stats_finite) {
	return rxgpu::scan_policy_i6(rows, dim, nq, i6_available != 0, stats_finite != 0) ? 1 : 0;
}

int rxgpu_scan_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, int shadow_available, int stats_finite) {
	return int(rxgpu::scan_policy_tier_subset(n_ids, dim, nq, kk, shadow_available != 0, stats_finite != 0));
}

int rxgpu_scan_tier_range(uint64_t rows, uint32_t dim, int listed, int shadow_available, int stats_finite) {
	return int(rxgpu::scan_policy_tier_range(rows, dim, listed != 0, shadow_available != 0, stats_finite != 0));
}

int rxgpu_index_last_candidates(const rxgpu_index* h, uint32_t* out_count, uint32_t* out_cap) {
	RX_CHECK(h && out_count && out_cap, RXGPU_ERR_PARAMS, "rxgpu_index_last_candidates: null argument");
	*out_count = h->last_cand_count.load();
	*out_cap = h->last_cand_cap.load();
	return RXGPU_OK;
}

int rxgpu_index_inspect(rxgpu_index* h, const char* what, void* out, uint64_t cap_bytes, uint64_t* out_bytes) {
	RX_CHECK(h && what && out_bytes, RXGPU_ERR_PARAMS, "rxgpu_index_inspect: null argument");
	*out_bytes = 0;
	RX_CHECK(!h->shard_set, RXGPU_ERR_PARAMS, "rxgpu_index_inspect: single-device indexes only (inspect the rxgpu_index_shard handles)");
	DeviceGuard dg(h->device);
	return rxgpu::inspect_index(h, what, out, cap_bytes, out_bytes);
}

int rxgpu_knn_merge_probe(int device, int what, const float* dist, const uint32_t* row, uint32_t n, uint32_t kk, float* out_dist, uint32_t* out_row,
						  uint32_t* out_count, int* out_path) {
	RX_CHECK(out_dist && out_row && out_count && out_path && (n == 0 || (dist && row)), RXGPU_ERR_PARAMS, "rxgpu_knn_merge_probe: null argument");
	RX_CHECK(what >= 0 && what <= 2, RXGPU_ERR_PARAMS, "rxgpu_knn_merge_probe: unknown kernel");
	RX_CHECK(kk >= 1 && kk <= uint32_t(what == 0 ? rxgpu::kMaxFusedK2 : rxgpu::kMaxFusedK), RXGPU_ERR_PARAMS, "rxgpu_knn_merge_probe: kk out of range");
	const uint64_t pairs = what == 0 ? uint64_t(n) * kk : n;
	RX_CHECK(pairs <= (1u << 24), RXGPU_ERR_PARAMS, "rxgpu_knn_merge_probe: too many pairs");
	DeviceGuard dg(device);
	RX_CHECK(dg.ok, RXGPU_ERR_DEVICE, "rxgpu_knn_merge_probe: no such device");
	// one allocation: the pairs, the result, {count, path, candidate count}
	const size_t in_words = size_t(std::max<uint64_t>(pairs, 1));
	uint32_t* d = nullptr;
	RX_HIP(hipMalloc(reinterpret_cast<void**>(&d), (2 * in_words + 2 * kk + 3) * sizeof(uint32_t)));
	float* d_dist = reinterpret_cast<float*>(d);
	uint32_t* d_row = d + in_words;
	float* d_od = reinterpret_cast<float*>(d_row + in_words);
	uint32_t* d_or = d_row + in_words + kk;
	uint32_t* d_tail = d_or + kk;   // [0] count, [1] path, [2] n
	const uint32_t tail[3] = {0, 0, n};
	hipError_t e = hipMemcpy(d_tail, tail, sizeof(tail), hipMemcpyHostToDevice);
	if (e == hipSuccess && pairs) e = hipMemcpy(d_dist, dist, pairs * sizeof(float), hipMemcpyHostToDevice);
	if (e == hipSuccess && pairs) e = hipMemcpy(d_row, row, pairs * sizeof(uint32_t), hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		if (what == 0) {
			rxgpu::launch_merge_lists(d_dist, d_row, n, kk, 1, d_od, d_or, d_tail, nullptr, nullptr, 0, d_tail + 1);
		} else if (what == 1) {   // cand_cnt = cap = n: the candidate branch
			rxgpu::launch_merge_final(d_dist, d_row, d_tail + 2, n, nullptr, nullptr, 0, kk, 1, d_od, d_or, d_tail, nullptr, d_tail + 1);
		} else {
			rxgpu::launch_merge(d_dist, d_row, n, kk, 1, d_od, d_or, d_tail, nullptr, 0, nullptr);
		}
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipDeviceSynchronize();
	uint32_t back[2] = {0, 0};
	if (e == hipSuccess) e = hipMemcpy(out_dist, d_od, kk * sizeof(float), hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(out_row, d_or, kk * sizeof(uint32_t), hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(back, d_tail, sizeof(back), hipMemcpyDeviceToHost);
	(void)hipFree(d);
	RX_HIP(e);
	*out_count = back[0];
	*out_path = int(back[1]);
	return RXGPU_OK;
}

int rxgpu_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) {
		set_error("hipGetDeviceCount failed");
		return RXGPU_ERR_DEVICE;
	}
	return n;
}

int rxgpu_device_arch(int device, char* name, size_t cap) {
	hipDeviceProp_t prop;
	RX_HIP(hipGetDeviceProperties(&prop, device));
	std::snprintf(name, cap, "%s", prop.gcnArchName);
	return RXGPU_OK;
}

int rxgpu_index_create(int metric, uint32_t dim, uint64_t capacity, int device, rxgpu_index** out) {
	RX_CHECK(out, RXGPU_ERR_PARAMS, "rxgpu_index_create: out is null");
	RX_CHECK(metric >= 0 && metric <= 2, RXGPU_ERR_PARAMS, "rxgpu_index_create: unknown metric");
	RX_CHECK(dim > 0 && dim <= 65535, RXGPU_ERR_PARAMS, "rxgpu_index_create: dimension must be in [1, 65535]");
	RX_CHECK(capacity < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "rxgpu_index_create: capacity must fit 32-bit rows");
	int ndev = 0;
	RX_HIP(hipGetDeviceCount(&ndev));
	RX_CHECK(device >= 0 && device < ndev, RXGPU_ERR_PARAMS, "rxgpu_index_create: no such device");
	DeviceGuard dg(device);
	RX_CHECK(dg.ok, RXGPU_ERR_DEVICE, "rxgpu_index_create: hipSetDevice failed");
	hipDeviceProp_t prop;
	RX_HIP(hipGetDeviceProperties(&prop, device));
	auto* h = new rxgpu_index();
	h->metric = metric;
	h->dim = dim;
	h->stride = (dim + 3u) & ~3u;
	if (const char* e = std::getenv("RXGPU_ROW_ALIGN")) {   // experiment: rows start on multiples of so many bytes (a 3 KB row then lies in ONE 4 KB page)
		const uint32_t align = uint32_t(std::max(0, atoi(e)));
		if (align >= 16u && (align & (align - 1u)) == 0u) h->stride = uint32_t(((uint64_t(h->stride) * 4u + align - 1u) & ~uint64_t(align - 1u)) / 4u);
	}
	h->device = device;
	h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	*out = h;
	if (capacity) {
		if (int rc = rxgpu_index_reserve(h, capacity); rc) {
			delete h;
			*out = nullptr;
			return rc;
		}
	}
	register_live_index(h);
	return RXGPU_OK;
}

void rxgpu_index_destroy(rxgpu_index* h) {
	if (!h) return;
	if (h->shard_set) {
		rxgpu::sharded_destroy(h);
		delete h;
		return;
	}
	unregister_live_index(h);   // from here on an ending thread leaves this index alone
	DeviceGuard dg(h->device);
	(void)rxgpu::device_wait_all(h->device);
	rxgpu::hnsw_server_destroy(h);
	for (auto& kv : h->resident_ctx) h->free_ctx.push_back(kv.second);
	for (auto* c : h->free_ctx) {
		c->release();
		delete c;
	}
	for (auto& kv : h->stream_ctx) {
		kv.second->release();
		delete kv.second;
	}
	for (auto& kv : h->profile) {
		for (auto& ev : kv.second.events) {
			(void)hipEventDestroy(ev.first);
			(void)hipEventDestroy(ev.second);
		}
	}
	if (!h->adopted) {
		if (h->d_rows) (void)hipFree(h->d_rows);
		if (h->d_inv_norms) (void)hipFree(h->d_inv_norms);
	}
	rxgpu::derived_free(h);
	if (h->d_row_ids) (void)hipFree(h->d_row_ids);
	if (h->d_links0) (void)hipFree(h->d_links0);
	if (h->d_upper_off) (void)hipFree(h->d_upper_off);
	if (h->d_upper) (void)hipFree(h->d_upper);
	if (h->d_deleted) (void)hipFree(h->d_deleted);
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_list_off) (void)hipFree(h->d_list_off);
	if (h->d_list_rows) (void)hipFree(h->d_list_rows);
	if (h->d_corr) (void)hipFree(h->d_corr);
	if (h->d_hnsw_stats) (void)hipFree(h->d_hnsw_stats);
	h->build_scratch.release();
	h->build_nodes.release();
	h->build_view.release();
	delete h;
}

int rxgpu_index_reserve(rxgpu_index* h, uint64_t capacity) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (h->shard_set) {
		if (capacity == h->capacity) return RXGPU_OK;
		set_error("rxgpu_index_reserve: the capacity of a sharded index is fixed (create a new one)");
		return RXGPU_ERR_LOGIC;
	}
	RX_CHECK(!h->adopted, RXGPU_ERR_LOGIC, "rxgpu_index_reserve: storage is adopted (caller-owned)");
	RX_CHECK(capacity >= h->count, RXGPU_ERR_PARAMS, "Cannot resize, max element is less than the current number of elements");
	RX_CHECK(capacity < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "capacity must fit 32-bit rows");
	if (capacity == h->capacity) return RXGPU_OK;
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	DeviceGuard dg(h->device);
	float* nrows = nullptr;
	float* nnorm = nullptr;
	if (capacity) {
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&nrows), capacity * h->stride * sizeof(float)));
		if (h->metric == RXGPU_METRIC_COSINE) {
			hipError_t e = hipMalloc(reinterpret_cast<void**>(&nnorm), capacity * sizeof(float));
			if (e != hipSuccess) {
				(void)hipFree(nrows);
				set_error("Not enough memory: failed to allocate norm coefficients");
				return RXGPU_ERR_NOMEM;
			}
		}
		if (h->count) {
			RX_HIP(hipMemcpy(nrows, h->d_rows, h->count * h->stride * sizeof(float), hipMemcpyDeviceToDevice));
			if (nnorm) RX_HIP(hipMemcpy(nnorm, h->d_inv_norms, h->count * sizeof(float), hipMemcpyDeviceToDevice));
		}
	}
	if (h->d_rows) (void)hipFree(h->d_rows);
	if (h->d_inv_norms) (void)hipFree(h->d_inv_norms);
	h->d_rows = nrows;
	h->d_inv_norms = nnorm;
	h->capacity = capacity;
	return RXGPU_OK;
}

int rxgpu_index_upload_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const float* rows, const float* inv_norms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (h->shard_set) return rxgpu::sharded_upload_rows(h, first_row, n, rows, inv_norms);
	RX_CHECK(!h->adopted, RXGPU_ERR_LOGIC, "rxgpu_index_upload_rows: storage is adopted (caller-owned)");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(rows, RXGPU_ERR_PARAMS, "rxgpu_index_upload_rows: rows is null");
	RX_CHECK(first_row + n <= h->capacity, RXGPU_ERR_PARAMS, "The number of elements exceeds the specified limit");
	RX_CHECK(h->metric != RXGPU_METRIC_COSINE || inv_norms, RXGPU_ERR_PARAMS, "cosine index requires inv_norms");
	DeviceGuard dg(h->device);
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	float* dst = h->d_rows + first_row * h->stride;
	if (h->stride == h->dim) {
		RX_HIP(hipMemcpy(dst, rows, n * h->dim * sizeof(float), hipMemcpyHostToDevice));
	} else {
		RX_HIP(hipMemcpy2D(dst, h->stride * sizeof(float), rows, h->dim * sizeof(float), h->dim * sizeof(float), n, hipMemcpyHostToDevice));
	}
	if (h->metric == RXGPU_METRIC_COSINE) {
		RX_HIP(hipMemcpy(h->d_inv_norms + first_row, inv_norms, n * sizeof(float), hipMemcpyHostToDevice));
	}
	h->count = std::max(h->count, first_row + n);
	return rxgpu::derived_follow_upload(h, first_row, n);
}

int rxgpu_index_adopt_device_rows(rxgpu_index* h, const void* d_rows, uint64_t n, uint32_t row_stride, const void* d_inv_norms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_index_adopt_device_rows: not available on a sharded index");
	RX_CHECK(d_rows || n == 0, RXGPU_ERR_PARAMS, "rxgpu_index_adopt_device_rows: d_rows is null");
	RX_CHECK(row_stride >= h->dim && row_stride % 4 == 0, RXGPU_ERR_PARAMS, "row_stride must be >= dim and a multiple of 4 floats");
	RX_CHECK((reinterpret_cast<uintptr_t>(d_rows) & 15) == 0, RXGPU_ERR_PARAMS, "d_rows must be 16-byte aligned");
	RX_CHECK(n < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "n must fit 32-bit rows");
	RX_CHECK(h->metric != RXGPU_METRIC_COSINE || d_inv_norms || n == 0, RXGPU_ERR_PARAMS, "cosine index requires d_inv_norms");
	DeviceGuard dg(h->device);
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	if (!h->adopted) {
		if (h->d_rows) (void)hipFree(h->d_rows);
		if (h->d_inv_norms) (void)hipFree(h->d_inv_norms);
	}
	h->adopted = true;
	h->d_rows = const_cast<float*>(static_cast<const float*>(d_rows));
	h->d_inv_norms = const_cast<float*>(static_cast<const float*>(d_inv_norms));
	h->stride = row_stride;
	h->capacity = n;
	h->count = n;
	rxgpu::derived_invalidate(h);
	return RXGPU_OK;
}

int rxgpu_index_move_row(rxgpu_index* h, uint64_t from, uint64_t to) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (h->shard_set) return rxgpu::sharded_move_row(h, from, to);
	RX_CHECK(!h->adopted, RXGPU_ERR_LOGIC, "rxgpu_index_move_row: storage is adopted (caller-owned)");
	RX_CHECK(from < h->count && to < h->count, RXGPU_ERR_PARAMS, "rxgpu_index_move_row: row out of range");
	if (from == to) return RXGPU_OK;
	DeviceGuard dg(h->device);
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	RX_HIP(hipMemcpy(h->d_rows + to * h->stride, h->d_rows + from * h->stride, h->stride * sizeof(float), hipMemcpyDeviceToDevice));
	if (h->d_inv_norms) RX_HIP(hipMemcpy(h->d_inv_norms + to, h->d_inv_norms + from, sizeof(float), hipMemcpyDeviceToDevice));
	return rxgpu::derived_follow_move(h, from, to);
}

int rxgpu_index_download_row(rxgpu_index* h, uint64_t row, float* out_row, float* out_inv_norm) {
	RX_CHECK(h && out_row, RXGPU_ERR_PARAMS, "rxgpu_index_download_row: null argument");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_index_download_row: single-device indexes only");
	RX_CHECK(row < h->count, RXGPU_ERR_PARAMS, "rxgpu_index_download_row: row out of range");
	DeviceGuard dg(h->device);
	RX_HIP(hipMemcpy(out_row, h->d_rows + row * h->stride, h->dim * sizeof(float), hipMemcpyDeviceToHost));
	if (out_inv_norm) {
		*out_inv_norm = 1.0f;
		if (h->d_inv_norms) RX_HIP(hipMemcpy(out_inv_norm, h->d_inv_norms + row, sizeof(float), hipMemcpyDeviceToHost));
	}
	return RXGPU_OK;
}

int rxgpu_index_truncate(rxgpu_index* h, uint64_t count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (h->shard_set) return rxgpu::sharded_truncate(h, count);
	RX_CHECK(count <= h->capacity, RXGPU_ERR_PARAMS, "rxgpu_index_truncate: count exceeds capacity");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	// shrinking keeps the statistics (upper bounds stay upper bounds) and the shadow (rows past count are never read)
	if (count > h->count) rxgpu::derived_invalidate(h);
	if (count < h->count) {   // (the 6-bit shadow shares tiles between rows: the rows left behind in the last tile go back to zero)
		DeviceGuard dg(h->device);
		if (int rc = rxgpu::derived_follow_truncate(h, count); rc) return rc;
	}
	h->count = count;
	return RXGPU_OK;
}

uint64_t rxgpu_index_count(const rxgpu_index* h) { return h ? h->count : 0; }
uint64_t rxgpu_index_capacity(const rxgpu_index* h) { return h ? h->capacity : 0; }
uint32_t rxgpu_index_dim(const rxgpu_index* h) { return h ? h->dim : 0; }
uint32_t rxgpu_index_row_stride(const rxgpu_index* h) { return h ? h->stride : 0; }
int rxgpu_index_metric(const rxgpu_index* h) { return h ? h->metric : -1; }
int rxgpu_index_device(const rxgpu_index* h) { return h ? h->device : -1; }
uint64_t rxgpu_index_device_bytes(const rxgpu_index* h) {
	if (!h) return 0;
	if (h->shard_set) return rxgpu::sharded_device_bytes(h);
	return h->capacity * h->stride * sizeof(float) + (h->d_inv_norms ? h->capacity * sizeof(float) : 0);
}

// internal row -> row id table for consumers on the device (the hybrid fusion maps the scan's rows to the planner's row ids there)
int rxgpu_index_upload_row_ids(rxgpu_index* h, uint64_t first_row, uint64_t n, const int32_t* row_ids) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_index_upload_row_ids: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(row_ids && first_row + n <= h->capacity, RXGPU_ERR_PARAMS, "rxgpu_index_upload_row_ids: rows out of range");
	DeviceGuard dg(h->device);
	if (h->row_ids_cap < h->capacity) {
		int32_t* grown = nullptr;
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&grown), h->capacity * sizeof(int32_t)));
		if (h->d_row_ids) {
			(void)hipMemcpy(grown, h->d_row_ids, h->row_ids_cap * sizeof(int32_t), hipMemcpyDeviceToDevice);
			(void)hipFree(h->d_row_ids);
		}
		h->d_row_ids = grown;
		h->row_ids_cap = h->capacity;
	}
	RX_HIP(hipMemcpy(h->d_row_ids + first_row, row_ids, n * sizeof(int32_t), hipMemcpyHostToDevice));
	return RXGPU_OK;
}
const void* rxgpu_index_row_ids_device(const rxgpu_index* h) { return h && !h->shard_set ? h->d_row_ids : nullptr; }

int rxgpu_profile_enable(rxgpu_index* h, int on) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_profile_enable: not available on a sharded index");
	std::lock_guard<std::mutex> lk(h->mtx);
	for (auto& kv : h->profile) {
		for (auto& ev : kv.second.events) {
			(void)hipEventDestroy(ev.first);
			(void)hipEventDestroy(ev.second);
		}
	}
	h->profile.clear();
	h->profiling = on != 0;
	return RXGPU_OK;
}

int rxgpu_profile_read(rxgpu_index* h, const char* name, uint64_t* launches, double* total_ms) {
	RX_CHECK(h && name && launches && total_ms, RXGPU_ERR_PARAMS, "rxgpu_profile_read: null argument");
	*launches = 0;
	*total_ms = 0.0;
	std::lock_guard<std::mutex> lk(h->mtx);
	auto it = h->profile.find(name);
	if (it == h->profile.end()) return RXGPU_OK;
	DeviceGuard dg(h->device);
	for (auto& ev : it->second.events) {
		RX_HIP(hipEventSynchronize(ev.second));
		float ms = 0.f;
		RX_HIP(hipEventElapsedTime(&ms, ev.first, ev.second));
		*total_ms += ms;
		++*launches;
	}
	return RXGPU_OK;
}

}  // extern "C"
