// C-ABI implementation (include/rxgpu.h): index storage in HBM, search entry points, instrumentation.
// Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../../include/rxgpu.h"
#include "knn_i8_quant.h"
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
	d_top.release();
	d_qplanes.release();
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

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::ProfileScope;
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

// Enqueue scan + merge for nq device-resident queries; results land in d_out_* (device).
int enqueue_knn_fused(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
					  uint32_t* d_out_row, uint32_t* d_out_count) {
	const uint32_t gridx = rxgpu::scan_grid_x(h->count, h->cus);
	const size_t part = size_t(nq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	rxgpu::ScanParams p{};
	p.rows = h->d_rows;
	p.inv_norms = h->d_inv_norms;
	p.queries = d_queries;
	p.n = h->count;
	p.stride = h->stride;
	p.dim = h->dim;
	p.kk = kk;
	p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	{
		ProfileScope ps(h, "scan", c->stream);
		rxgpu::launch_scan(h->metric, p, nq, gridx, c->stream);
	}
	{
		ProfileScope ps(h, "merge", c->stream);
		rxgpu::launch_merge_lists(p.part_dist, p.part_row, gridx, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// ---- batched path (nq >= 2): MFMA candidate generation + exact re-score, see knn_batched.hip ----------------------
constexpr uint32_t kBatchSampleRows = 32768;
constexpr uint32_t kBatchSampleRowsBf16 = 131072;   // the sample pass is cheap on the bf16 pipe; a tighter threshold pays for the wider margin

static int batch_min_queries() {
	static const int v = [] {
		const char* e = getenv("RXGPU_BATCH_MIN");
		return e ? atoi(e) : 2;
	}();
	return v;
}

// The statistics words back on the host (h->mtx held): are the maxima finite and has no NaN row been seen?  Only then does the rounding
// bound of a pruned scan mean anything; the automatic scan policy (enqueue_knn) keeps such an index on the f32 scan.  Words 3 and 4 (the
// int8 shadow's residual maxima, knn_scan_i8.hip) report a non-finite value through word 2.
constexpr size_t kStatsWords = 5;
int read_stats_finite(rxgpu_index* h, hipStream_t s) {
	unsigned int w[3] = {0, 0, 0};
	RX_HIP(hipMemcpyAsync(w, h->d_stats, sizeof(w), hipMemcpyDeviceToHost, s));
	RX_HIP(hipStreamSynchronize(s));
	float a, b;
	std::memcpy(&a, &w[0], sizeof(a));
	std::memcpy(&b, &w[1], sizeof(b));
	h->stats_finite = std::isfinite(a) && std::isfinite(b) && w[2] == 0;
	return RXGPU_OK;
}

// Per-row statistics are cached on the index; recomputed (synchronously, under the index mutex) after any mutation.
int ensure_row_stats(rxgpu_index* h, hipStream_t s) {
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->stats_valid) return RXGPU_OK;
	if (!h->d_stats) RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_stats), kStatsWords * sizeof(unsigned int)));
	if (h->metric == RXGPU_METRIC_L2 && h->row_sq_capacity < h->count) {
		if (h->d_row_sq) (void)hipFree(h->d_row_sq);
		h->d_row_sq = nullptr;
		h->row_sq_capacity = 0;
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_row_sq), std::max<uint64_t>(h->capacity, h->count) * sizeof(float)));
		h->row_sq_capacity = std::max<uint64_t>(h->capacity, h->count);
	}
	RX_HIP(hipMemsetAsync(h->d_stats, 0, kStatsWords * sizeof(unsigned int), s));
	h->i8_valid = false;   // its two words were cleared with the rest: the shadow's next build folds them in again
	rxgpu::launch_row_stats(h->d_rows, h->d_inv_norms, h->count, h->stride, h->dim, h->metric == RXGPU_METRIC_L2 ? h->d_row_sq : nullptr,
							h->d_stats, h->cus, s);
	RX_HIP(hipGetLastError());
	if (int rc = read_stats_finite(h, s); rc) return rc;   // synchronises the stream
	h->stats_valid = true;
	return RXGPU_OK;
}

// bf16 shadow of the rows for the nomination GEMM: 2 bytes per element on top of the 4-byte rows (HBM is 288 GB: 10M x 768 costs 15.4 GB);
// rebuilt lazily after any mutation, like the row statistics.
int ensure_bf16_shadow(rxgpu_index* h, hipStream_t s) {
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->bf16_valid) return RXGPU_OK;
	const uint32_t ld = (h->dim + 63u) & ~63u;
	const uint64_t need = (std::max<uint64_t>(h->capacity, h->count) + rxgpu::kShadowTileRows - 1) / rxgpu::kShadowTileRows * rxgpu::kShadowTileRows;   // whole tiles
	if (h->bf16_capacity < need) {
		if (h->d_rows_bf16) (void)hipFree(h->d_rows_bf16);
		h->d_rows_bf16 = nullptr;
		h->bf16_capacity = 0;
		const char* e = getenv("RXGPU_SHADOW_BLOCKED");
		h->bf16_blocked = !(e && atoi(e) == 0);
		if (hipMalloc(reinterpret_cast<void**>(&h->d_rows_bf16), need * ld * sizeof(uint16_t)) != hipSuccess) {
			(void)hipGetLastError();   // not an error of the search: the caller falls back to the f32 rows
			h->d_rows_bf16 = nullptr;
			h->bf16_unavailable = true;
			return RXGPU_ERR_NOMEM;
		}
		h->bf16_capacity = need;
	}
	rxgpu::launch_to_bf16(h->d_rows, h->count, h->stride, h->dim, h->d_rows_bf16, ld, h->cus, s, 0, h->bf16_blocked);
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(s));
	h->bf16_valid = true;
	return RXGPU_OK;
}

// int8 shadow of the rows for the pruning pass of a single query (knn_scan_i8.hip): 1 byte per element + 8 bytes per row on top of the 4-byte
// rows; built lazily behind the row statistics (it folds two more maxima into their words) and kept in step by the mutations like the bf16 shadow.
int ensure_i8_shadow(rxgpu_index* h, hipStream_t s) {
	if (int rc = ensure_row_stats(h, s); rc) return rc;
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->i8_valid) return RXGPU_OK;
	const uint32_t ld8 = rxgpu::i8_ld(h->dim);
	const uint64_t need = std::max<uint64_t>(h->capacity, h->count);
	if (h->i8_capacity < need) {
		if (h->d_codes_i8) (void)hipFree(h->d_codes_i8);
		if (h->d_side_i8) (void)hipFree(h->d_side_i8);
		h->d_codes_i8 = nullptr;
		h->d_side_i8 = nullptr;
		h->i8_capacity = 0;
		if (hipMalloc(reinterpret_cast<void**>(&h->d_codes_i8), need * ld8) != hipSuccess ||
			hipMalloc(reinterpret_cast<void**>(&h->d_side_i8), need * sizeof(float2)) != hipSuccess) {
			(void)hipGetLastError();   // not an error of the search: the caller takes the bf16 tier
			if (h->d_codes_i8) (void)hipFree(h->d_codes_i8);
			h->d_codes_i8 = nullptr;
			h->d_side_i8 = nullptr;
			h->i8_unavailable = true;
			return RXGPU_ERR_NOMEM;
		}
		h->i8_capacity = need;
	}
	rxgpu::launch_i8_build(h->d_rows, h->d_inv_norms, h->count, h->stride, h->dim, h->d_codes_i8, h->d_side_i8, ld8, h->d_stats, h->cus, s);
	RX_HIP(hipGetLastError());
	if (int rc = read_stats_finite(h, s); rc) return rc;   // synchronises the stream
	h->i8_valid = true;
	return RXGPU_OK;
}

static int batch_bf16_min_queries() {   // read per call (tests and A/B runs switch it)
	const char* e = getenv("RXGPU_BATCH_BF16_MIN");   // 0 disables the bf16 nomination path
	return e ? atoi(e) : 2;   // measured at 10M x 768: 4.8-5.0 ms per batch for 8..256 queries against 6.2-10.6 ms on the f32 rows
}

// Every batch (2..256 queries at a time): nomination on the bf16 MFMA pipe over the bf16 shadow (knn_batched_bf16.hip), then the same exact tail.
int enqueue_knn_batched_bf16(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t q0, uint32_t cq, uint32_t kk,
							 float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_bf16_shadow(h, c->stream); rc) return rc;
	const uint32_t mt = cq <= 128 ? 128 : 256;   // query-tile width of the nomination kernel
	const uint32_t ld = (h->dim + 63u) & ~63u;
	const uint32_t q_stride = ld;   // the f32 copy for the exact re-score shares the padded stride
	const uint64_t ns = std::min<uint64_t>(h->count, kBatchSampleRowsBf16);
	// nominations per query ~ kk * n / ns, times ~3 for the bf16 margin; 10x headroom, overflow falls back to the exact scan
	uint64_t cap64 = std::max<uint64_t>(4096, 10 * uint64_t(kk) * ((h->count + ns - 1) / ns));
	cap64 = std::min<uint64_t>(cap64, std::max<uint64_t>(h->count, 64));
	const uint32_t cap = uint32_t((cap64 + 63) & ~63ull);
	if (int rc = c->d_qpad.ensure(size_t(mt) * q_stride * (sizeof(float) + sizeof(uint16_t))); rc) return rc;
	if (int rc = c->d_qstats.ensure(size_t(3) * mt * sizeof(float)); rc) return rc;
	if (int rc = c->d_dense.ensure(size_t(mt) * ns * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_row.ensure(size_t(mt) * cap * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_dist.ensure(size_t(mt) * cap * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(size_t(mt) * sizeof(uint32_t)); rc) return rc;
	float* qpad = static_cast<float*>(c->d_qpad.ptr);
	uint16_t* qbf = reinterpret_cast<uint16_t*>(qpad + size_t(mt) * q_stride);
	float* q_sq = static_cast<float*>(c->d_qstats.ptr);
	float* margin = q_sq + mt;
	float* thr = q_sq + 2 * mt;
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	c->pruned_cap = cap;
	RX_HIP(hipMemsetAsync(qpad, 0, size_t(mt) * q_stride * sizeof(float), c->stream));
	RX_HIP(hipMemcpy2DAsync(qpad, q_stride * sizeof(float), d_queries + size_t(q0) * h->dim, h->dim * sizeof(float), h->dim * sizeof(float), cq,
							hipMemcpyDeviceToDevice, c->stream));
	RX_HIP(hipMemsetAsync(cand_cnt, 0, size_t(mt) * sizeof(uint32_t), c->stream));
	rxgpu::launch_to_bf16(qpad, mt, q_stride, q_stride, qbf, ld, h->cus, c->stream);
	rxgpu::launch_query_stats(h->metric, qpad, cq, mt, q_stride, h->dim, h->d_stats, q_sq, margin, true, c->stream);

	rxgpu::GemmBf16Params g{};
	g.rows = h->d_rows_bf16;
	g.blocked = (h->bf16_blocked ? 1u : 0u) | ((getenv("RXGPU_GEMM_PRIO") && atoi(getenv("RXGPU_GEMM_PRIO"))) ? 2u : 0u);   // bit 1: s_setprio around the MFMA bursts (A/B)
	g.queries = qbf;
	g.inv_norms = h->d_inv_norms;
	g.row_sq = h->d_row_sq;
	g.q_sq = q_sq;
	g.ld = ld;
	g.nq = cq;
	auto grid_for = [&](uint64_t rows) { return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((rows + 255) / 256, uint64_t(h->cus)))); };
	g.n = ns;
	g.row_step = uint32_t(std::max<uint64_t>(1, h->count / ns));   // strided sample: representative whatever the insertion order
	g.dense = static_cast<float*>(c->d_dense.ptr);
	{
		ProfileScope ps(h, "gemm_sample", c->stream);
		RX_HIP(rxgpu::launch_gemm_bf16(h->metric, rxgpu::kGemmDense, int(mt), g, grid_for(ns), c->stream));
	}
	rxgpu::launch_sample_threshold(g.dense, ns, cq, mt, kk, margin, thr, c->stream);
	g.n = h->count;
	g.row_step = 1;
	g.dense = nullptr;
	g.thr = thr;
	g.cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
	g.cand_cnt = cand_cnt;
	g.cap = cap;
	{
		ProfileScope ps(h, "gemm", c->stream);
		RX_HIP(rxgpu::launch_gemm_bf16(h->metric, rxgpu::kGemmFilter, int(mt), g, grid_for(h->count), c->stream));
	}
	{
		ProfileScope ps(h, "rescore", c->stream);
		rxgpu::launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, q_stride, h->stride, h->dim, cq, cap, cand_cnt, g.cand_row,
							  static_cast<float*>(c->d_cand_dist.ptr), c->stream);
	}
	rxgpu::launch_merge(static_cast<float*>(c->d_cand_dist.ptr), g.cand_row, cap, kk, cq, d_out_dist + size_t(q0) * kk, d_out_row + size_t(q0) * kk,
						d_out_count ? d_out_count + q0 : nullptr, nullptr, 0, c->stream);
	{   // overflow fallback, gated on device
		const uint32_t gridx = rxgpu::scan_grid_x(h->count, h->cus);
		const size_t part = size_t(cq) * gridx * kk;
		if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
		if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
		rxgpu::ScanParams p{};
		p.rows = h->d_rows;
		p.inv_norms = h->d_inv_norms;
		p.queries = d_queries + size_t(q0) * h->dim;
		p.n = h->count;
		p.stride = h->stride;
		p.dim = h->dim;
		p.kk = kk;
		p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
		p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
		p.gate_cnt = cand_cnt;
		p.gate_cap = cap;
		ProfileScope ps(h, "fallback_scan", c->stream);
		rxgpu::launch_scan(h->metric, p, cq, gridx, c->stream);
		rxgpu::launch_merge(p.part_dist, p.part_row, gridx * kk, kk, cq, d_out_dist + size_t(q0) * kk, d_out_row + size_t(q0) * kk,
							d_out_count ? d_out_count + q0 : nullptr, cand_cnt, cap, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

int enqueue_knn_batched(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
						uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_row_stats(h, c->stream); rc) return rc;
	const uint32_t q_stride = (h->dim + 31u) & ~31u;
	const uint64_t ns = std::min<uint64_t>(h->count, kBatchSampleRows);
	// expected nominations per query ~ kk * n / ns (plus the eps margin); 4x headroom, overflow falls back to the exact scan
	uint64_t cap64 = std::max<uint64_t>(4096, 4 * uint64_t(kk) * ((h->count + ns - 1) / ns));
	cap64 = std::min<uint64_t>(cap64, std::max<uint64_t>(h->count, 64));
	const uint32_t cap = uint32_t((cap64 + 63) & ~63ull);
	for (uint32_t q0 = 0; q0 < nq; q0 += 256) {
		const uint32_t cq = std::min<uint32_t>(256, nq - q0);
		if (batch_bf16_min_queries() > 0 && int(cq) >= batch_bf16_min_queries() && !h->bf16_unavailable) {
			const int rc = enqueue_knn_batched_bf16(h, c, d_queries, q0, cq, kk, d_out_dist, d_out_row, d_out_count);
			if (rc == RXGPU_OK) continue;
			if (!(rc == RXGPU_ERR_NOMEM && h->bf16_unavailable)) return rc;   // no room for the shadow: f32 nomination below
		}
		const int mt = cq <= 32 ? 32 : cq <= 64 ? 64 : cq <= 128 ? 128 : 256;
		if (int rc = c->d_qpad.ensure(size_t(mt) * q_stride * sizeof(float)); rc) return rc;
		if (int rc = c->d_qstats.ensure(size_t(3) * mt * sizeof(float)); rc) return rc;
		if (int rc = c->d_dense.ensure(size_t(mt) * ns * sizeof(float)); rc) return rc;
		if (int rc = c->d_cand_row.ensure(size_t(mt) * cap * sizeof(uint32_t)); rc) return rc;
		if (int rc = c->d_cand_dist.ensure(size_t(mt) * cap * sizeof(float)); rc) return rc;
		if (int rc = c->d_cand_cnt.ensure(size_t(mt) * sizeof(uint32_t)); rc) return rc;
		float* qpad = static_cast<float*>(c->d_qpad.ptr);
		float* q_sq = static_cast<float*>(c->d_qstats.ptr);
		float* margin = q_sq + mt;
		float* thr = q_sq + 2 * mt;
		uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	c->pruned_cap = cap;
		RX_HIP(hipMemsetAsync(qpad, 0, size_t(mt) * q_stride * sizeof(float), c->stream));
		RX_HIP(hipMemcpy2DAsync(qpad, q_stride * sizeof(float), d_queries + size_t(q0) * h->dim, h->dim * sizeof(float),
								h->dim * sizeof(float), cq, hipMemcpyDeviceToDevice, c->stream));
		RX_HIP(hipMemsetAsync(cand_cnt, 0, size_t(mt) * sizeof(uint32_t), c->stream));
		rxgpu::launch_query_stats(h->metric, qpad, cq, mt, q_stride, h->dim, h->d_stats, q_sq, margin, false, c->stream);

		rxgpu::GemmParams g{};
		g.rows = h->d_rows;
		g.inv_norms = h->d_inv_norms;
		g.row_sq = h->d_row_sq;
		g.queries = qpad;
		g.q_sq = q_sq;
		g.stride = h->stride;
		g.dim = h->dim;
		g.nq = cq;
		g.q_stride = q_stride;
		const uint32_t wg_per_cu = uint32_t(std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / rxgpu::gemm_lds_bytes(mt))));
		auto grid_for = [&](uint64_t rows) {
			const uint64_t tiles = (rows + 127) / 128;
			return uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(tiles, uint64_t(h->cus) * wg_per_cu)));
		};
		// 2. sample (strided: representative whatever the insertion order)
		g.n = ns;
		g.row_step = uint32_t(std::max<uint64_t>(1, h->count / ns));
		g.dense = static_cast<float*>(c->d_dense.ptr);
		{
			ProfileScope ps(h, "gemm_sample", c->stream);
			RX_HIP(rxgpu::launch_gemm(h->metric, mt, rxgpu::kGemmDense, g, grid_for(ns), c->stream));
		}
		// 3. thresholds
		rxgpu::launch_sample_threshold(g.dense, ns, cq, mt, kk, margin, thr, c->stream);
		// 4. filter pass over the whole corpus
		g.n = h->count;
		g.row_step = 1;
		g.dense = nullptr;
		g.thr = thr;
		g.cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
		g.cand_cnt = cand_cnt;
		g.cap = cap;
		{
			ProfileScope ps(h, "gemm", c->stream);
			RX_HIP(rxgpu::launch_gemm(h->metric, mt, rxgpu::kGemmFilter, g, grid_for(h->count), c->stream));
		}
		// 5. exact re-score, 6. exact top-kk
		{
			ProfileScope ps(h, "rescore", c->stream);
			rxgpu::launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, q_stride, h->stride, h->dim, cq, cap, cand_cnt, g.cand_row,
								  static_cast<float*>(c->d_cand_dist.ptr), c->stream);
		}
		rxgpu::launch_merge(static_cast<float*>(c->d_cand_dist.ptr), g.cand_row, cap, kk, cq, d_out_dist + size_t(q0) * kk,
							d_out_row + size_t(q0) * kk, d_out_count ? d_out_count + q0 : nullptr, nullptr, 0, c->stream);
		// overflow fallback, gated on device: exact fused scan only for queries with cand_cnt > cap
		{
			const uint32_t gridx = rxgpu::scan_grid_x(h->count, h->cus);
			const size_t part = size_t(cq) * gridx * kk;
			if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
			if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
			rxgpu::ScanParams p{};
			p.rows = h->d_rows;
			p.inv_norms = h->d_inv_norms;
			p.queries = d_queries + size_t(q0) * h->dim;
			p.n = h->count;
			p.stride = h->stride;
			p.dim = h->dim;
			p.kk = kk;
			p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
			p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
			p.gate_cnt = cand_cnt;
			p.gate_cap = cap;
			ProfileScope ps(h, "fallback_scan", c->stream);
			rxgpu::launch_scan(h->metric, p, cq, gridx, c->stream);
			rxgpu::launch_merge(p.part_dist, p.part_row, gridx * kk, kk, cq, d_out_dist + size_t(q0) * kk, d_out_row + size_t(q0) * kk,
								d_out_count ? d_out_count + q0 : nullptr, cand_cnt, cap, c->stream);
		}
		RX_HIP(hipGetLastError());
	}
	return RXGPU_OK;
}

// bf16-pruned scan for one .. a few queries: 2 bytes per element from HBM instead of 4, exact result (knn_scan.hip).
// RXGPU_SCAN_BF16, read per call (a process can switch it for A/B runs): 1 = forced on (up to kPrunedMaxQueries queries, any size), 0 = forced
// off (the f32 paths, always), unset = automatic: single queries on indexes of at least kPrunedAutoMinBytes of f32 rows.
enum ScanBf16Mode { kScanBf16Off = 0, kScanBf16On = 1, kScanBf16Auto = 2 };
static ScanBf16Mode scan_bf16_mode() {
	const char* e = getenv("RXGPU_SCAN_BF16");
	if (!e || !*e) return kScanBf16Auto;
	return atoi(e) != 0 ? kScanBf16On : kScanBf16Off;
}
constexpr uint32_t kPrunedMaxQueries = 8;
// Automatic mode: the pruned path pays a fixed tail per query (filter, re-score, two merges, the gated scan) and saves half the streaming; it
// also costs +2 bytes per element of HBM.  Never below 1 GiB (small indexes keep the f32 kernel and their footprint); measured crossover in
// profiles/scan_policy_crossover.json.  RXGPU_SCAN_BF16_MIN_BYTES overrides it (tests exercise the decision on small corpora).
constexpr uint64_t kPrunedAutoMinBytes = 1ull << 30;
static uint64_t pruned_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_BF16_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedAutoMinBytes;
}
// The int8 tier (knn_scan_i8.hip) refines a call the automatic mode above already accepts.  RXGPU_SCAN_I8, read per call: 0 = this tier off,
// 1 = forced at any size (up to kPrunedMaxQueries queries; for tests and A/B), unset = automatic: indexes of at least kPrunedI8AutoMinBytes of
// f32 rows.  RXGPU_SCAN_BF16=0 (the f32 paths, always) and =1 (the bf16 tier, exactly) both win over it.
// kPrunedI8AutoMinBytes: the measured crossover against the bf16 tier (and the f32 scan) is 0.6 GB of f32 rows at 768 dims
// (profiles/scan_i8_crossover.json), rounded up to a power of two and never below 1 GiB, like kPrunedAutoMinBytes.  RXGPU_SCAN_I8_MIN_BYTES
// overrides it.
constexpr uint64_t kPrunedI8AutoMinBytes = 1ull << 30;
static ScanBf16Mode scan_i8_mode() {
	const char* e = getenv("RXGPU_SCAN_I8");
	if (!e || !*e) return kScanBf16Auto;
	return atoi(e) != 0 ? kScanBf16On : kScanBf16Off;
}
static uint64_t pruned_i8_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I8_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI8AutoMinBytes;
}
enum ScanTier { kTierF32 = 0, kTierBf16 = 1, kTierI8 = 2 };
// The whole decision, without a device: which scan does a call with nq queries on rows x dim f32 rows take?
static ScanTier scan_policy_tier(uint64_t rows, uint32_t dim, uint32_t nq, bool bf16_available, bool i8_available, bool stats_finite) {
	const ScanBf16Mode mode = scan_bf16_mode();
	if (mode == kScanBf16Off) return kTierF32;
	const ScanBf16Mode i8 = scan_i8_mode();
	const bool i8_can = mode == kScanBf16Auto && i8 != kScanBf16Off && i8_available && rxgpu::i8_dim_supported(dim);
	if (i8_can && i8 == kScanBf16On && nq <= kPrunedMaxQueries) return kTierI8;
	if (!bf16_available || !rxgpu::scan_bf16_supported((dim + 63u) & ~63u)) return kTierF32;
	if (mode == kScanBf16On) return nq <= kPrunedMaxQueries ? kTierBf16 : kTierF32;
	if (!(nq == 1 && stats_finite && rows * dim * sizeof(float) >= pruned_auto_min_bytes())) return kTierF32;
	return i8_can && rows * dim * sizeof(float) >= pruned_i8_auto_min_bytes() ? kTierI8 : kTierBf16;
}
// ... does it take a pruned scan at all?
static bool scan_policy_pruned(uint64_t rows, uint32_t dim, uint32_t nq, bool shadow_available, bool stats_finite) {
	return scan_policy_tier(rows, dim, nq, shadow_available, shadow_available, stats_finite) != kTierF32;
}
// The same decision for a search over a ROW LIST (enqueue_knn_subset: pre-filtered search, IVF, their per-shard calls): the f32 subset scan or the
// int8-pruned one (knn_scan_i8_subset; the bf16 tier has no subset form, so RXGPU_SCAN_BF16=1, "the bf16 tier, exactly", keeps the f32 scan).
// kk is min(kk, n_ids); the pruned chain keeps one list entry per lane, so kk in 65..128 stays on the f32 subset scan.  The automatic rule
// counts the f32 bytes of the LISTED rows, not of the index: small lists keep their kernel and an index that only sees selective filters never
// builds the shadow.  kPrunedI8SubsetAutoMinBytes is meant to be the measured crossover against the f32 subset scan (tools/bench_prefilter_i8.py),
// rounded up to a power of two and never below 1 GiB.  That crossover has NOT been measured yet, so the default is the
// maximum value: the tier is forced-only (RXGPU_SCAN_I8=1) or opted into with RXGPU_SCAN_I8_SUBSET_MIN_BYTES, which overrides the default.
constexpr uint64_t kPrunedI8SubsetAutoMinBytes = ~0ull;
static uint64_t pruned_i8_subset_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I8_SUBSET_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI8SubsetAutoMinBytes;
}
static ScanTier scan_policy_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, bool i8_available, bool stats_finite) {
	if (scan_bf16_mode() != kScanBf16Auto) return kTierF32;
	const ScanBf16Mode i8 = scan_i8_mode();
	if (i8 == kScanBf16Off || !i8_available || !rxgpu::i8_dim_supported(dim) || kk > uint32_t(rxgpu::kMaxFusedK) || n_ids == 0) return kTierF32;
	if (i8 == kScanBf16On) return nq <= kPrunedMaxQueries ? kTierI8 : kTierF32;   // without a finite bound the gate answers, as in the unfiltered tier
	return nq == 1 && stats_finite && n_ids * dim * sizeof(float) >= pruned_i8_subset_auto_min_bytes() ? kTierI8 : kTierF32;
}
constexpr uint32_t kPrunedCap = 4096;

int enqueue_knn_pruned(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
					   uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_row_stats(h, c->stream); rc) return rc;
	if (int rc = ensure_bf16_shadow(h, c->stream); rc) return rc;
	const uint32_t ld = (h->dim + 63u) & ~63u;
	const uint32_t gridx = rxgpu::scan_bf16_grid_x(h->count, h->cus);   // the bf16 scan's grid
	const uint32_t gridx_exact = rxgpu::scan_grid_x(h->count, h->cus);   // the gated f32 scan's
	const uint32_t grid_max = std::max(gridx, gridx_exact);
	const uint32_t cap = uint32_t(std::min<uint64_t>(kPrunedCap, std::max<uint64_t>(64, (h->count + 63) & ~63ull)));
	if (int rc = c->d_qpad.ensure(size_t(nq) * ld * sizeof(float)); rc) return rc;
	if (int rc = c->d_qstats.ensure(size_t(2) * nq * sizeof(float)); rc) return rc;
	if (int rc = c->d_dense.ensure(size_t(nq) * h->count * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_dist.ensure(size_t(nq) * grid_max * kk * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(nq) * grid_max * kk * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_top.ensure(size_t(nq) * (2 * kk + 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_row.ensure(size_t(nq) * cap * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_dist.ensure(size_t(nq) * cap * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
	float* qpad = static_cast<float*>(c->d_qpad.ptr);
	float* q_sq = static_cast<float*>(c->d_qstats.ptr);
	float* margin = q_sq + nq;
	float* top_dist = static_cast<float*>(c->d_top.ptr);
	uint32_t* top_row = reinterpret_cast<uint32_t*>(top_dist + size_t(nq) * kk);
	uint32_t* top_cnt = top_row + size_t(nq) * kk;
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	c->pruned_cap = cap;
	// one launch: padded copy of the query, |q|^2, margin, cand_cnt = 0 (cap + 1 for a query without a finite bound: the gated exact scan answers it)
	rxgpu::launch_query_prep(h->metric, d_queries, nq, h->dim, qpad, ld, h->d_stats, q_sq, margin, cand_cnt, cap, c->stream);
	rxgpu::ScanBf16Params p{};
	p.sp.inv_norms = h->d_inv_norms;
	p.sp.n = h->count;
	p.sp.kk = kk;
	p.sp.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.sp.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	p.rows16 = h->d_rows_bf16;
	p.blocked = h->bf16_blocked ? 1u : 0u;
	p.queries32 = qpad;
	p.row_sq = h->d_row_sq;
	p.q_sq = q_sq;
	p.ld = ld;
	p.approx = static_cast<float*>(c->d_dense.ptr);
	{
		ProfileScope ps(h, "scan_bf16", c->stream);
		rxgpu::launch_scan_bf16(h->metric, p, nq, gridx, c->stream);
	}
	// (the scan leaves sorted lists like the f32 scan: the list merge, 4 us against 28 for the insertion merge in the kernel trace of the headline)
	rxgpu::launch_merge_lists(p.sp.part_dist, p.sp.part_row, gridx, kk, nq, top_dist, top_row, top_cnt, c->stream);
	{
		ProfileScope ps(h, "filter_approx", c->stream);
		rxgpu::launch_filter_approx(p.approx, h->count, top_dist, top_cnt, kk, margin, static_cast<uint32_t*>(c->d_cand_row.ptr), cand_cnt, cap, nq,
									h->cus, c->stream);
	}
	{
		ProfileScope ps(h, "rescore", c->stream);
		rxgpu::launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, ld, h->stride, h->dim, nq, cap, cand_cnt,
							  static_cast<uint32_t*>(c->d_cand_row.ptr), static_cast<float*>(c->d_cand_dist.ptr), c->stream);
	}
	rxgpu::launch_merge(static_cast<float*>(c->d_cand_dist.ptr), static_cast<uint32_t*>(c->d_cand_row.ptr), cap, kk, nq, d_out_dist, d_out_row,
						d_out_count, nullptr, 0, c->stream);
	{   // more rows inside the bound than the list holds (massive ties), or no finite bound: the f32 path's own scan + merge, gated on device
		rxgpu::ScanParams e{};
		e.rows = h->d_rows;
		e.inv_norms = h->d_inv_norms;
		e.queries = d_queries;
		e.n = h->count;
		e.stride = h->stride;
		e.dim = h->dim;
		e.kk = kk;
		e.part_dist = p.sp.part_dist;
		e.part_row = p.sp.part_row;
		e.gate_cnt = cand_cnt;
		e.gate_cap = cap;
		ProfileScope ps(h, "fallback_scan", c->stream);
		rxgpu::launch_scan(h->metric, e, nq, gridx_exact, c->stream);
		rxgpu::launch_merge_lists(e.part_dist, e.part_row, gridx_exact, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream, cand_cnt, cap);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// The int8 tier of the same chain: knn_query_prep_i8 and knn_scan_i8 in front, per-row LOWER bounds where the bf16 chain keeps approximate
// distances, everything behind the scan as above (same buffers, same cap).
int enqueue_knn_pruned_i8(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
						  uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_i8_shadow(h, c->stream); rc) return rc;   // (the row statistics first)
	const uint32_t ld8 = rxgpu::i8_ld(h->dim);
	const uint32_t gridx = rxgpu::scan_i8_grid_x(h->count, h->cus);
	const uint32_t gridx_exact = rxgpu::scan_grid_x(h->count, h->cus);   // the gated f32 scan's
	const uint32_t grid_max = std::max(gridx, gridx_exact);
	const uint32_t cap = uint32_t(std::min<uint64_t>(kPrunedCap, std::max<uint64_t>(64, (h->count + 63) & ~63ull)));
	if (int rc = c->d_qpad.ensure(size_t(nq) * ld8 * sizeof(float)); rc) return rc;
	if (int rc = c->d_qplanes.ensure(size_t(nq) * 2 * ld8); rc) return rc;
	if (int rc = c->d_qstats.ensure(size_t(4) * nq * sizeof(float)); rc) return rc;
	if (int rc = c->d_dense.ensure(size_t(nq) * h->count * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_dist.ensure(size_t(nq) * grid_max * kk * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(nq) * grid_max * kk * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_top.ensure(size_t(nq) * (2 * kk + 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_row.ensure(size_t(nq) * cap * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_dist.ensure(size_t(nq) * cap * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
	float* qpad = static_cast<float*>(c->d_qpad.ptr);
	float2* qinfo = static_cast<float2*>(c->d_qstats.ptr);   // [nq] pairs, then [nq] |q|^2, [nq] margins
	float* q_sq = reinterpret_cast<float*>(qinfo + nq);
	float* margin = q_sq + nq;
	float* top_dist = static_cast<float*>(c->d_top.ptr);
	uint32_t* top_row = reinterpret_cast<uint32_t*>(top_dist + size_t(nq) * kk);
	uint32_t* top_cnt = top_row + size_t(nq) * kk;
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	c->pruned_cap = cap;
	rxgpu::launch_query_prep_i8(h->metric, d_queries, nq, h->dim, qpad, static_cast<int8_t*>(c->d_qplanes.ptr), ld8, h->d_stats, q_sq, margin, qinfo,
								cand_cnt, cap, c->stream);
	rxgpu::ScanI8Params p{};
	p.sp.inv_norms = h->d_inv_norms;
	p.sp.n = h->count;
	p.sp.kk = kk;
	p.sp.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.sp.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	p.codes = h->d_codes_i8;
	p.side = h->d_side_i8;
	p.planes = static_cast<const int8_t*>(c->d_qplanes.ptr);
	p.qinfo = qinfo;
	p.row_sq = h->d_row_sq;
	p.q_sq = q_sq;
	p.ld8 = ld8;
	p.lower = static_cast<float*>(c->d_dense.ptr);
	{
		ProfileScope ps(h, "scan_i8", c->stream);
		rxgpu::launch_scan_i8(h->metric, p, nq, gridx, c->stream);
	}
	rxgpu::launch_merge_lists(p.sp.part_dist, p.sp.part_row, gridx, kk, nq, top_dist, top_row, top_cnt, c->stream);
	{
		ProfileScope ps(h, "filter_approx", c->stream);
		rxgpu::launch_filter_approx(p.lower, h->count, top_dist, top_cnt, kk, margin, static_cast<uint32_t*>(c->d_cand_row.ptr), cand_cnt, cap, nq,
									h->cus, c->stream);
	}
	{
		ProfileScope ps(h, "rescore", c->stream);
		rxgpu::launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, ld8, h->stride, h->dim, nq, cap, cand_cnt,
							  static_cast<uint32_t*>(c->d_cand_row.ptr), static_cast<float*>(c->d_cand_dist.ptr), c->stream);
	}
	rxgpu::launch_merge(static_cast<float*>(c->d_cand_dist.ptr), static_cast<uint32_t*>(c->d_cand_row.ptr), cap, kk, nq, d_out_dist, d_out_row,
						d_out_count, nullptr, 0, c->stream);
	{   // more rows inside the bound than the list holds (massive ties), or no finite bound: the f32 path's own scan + merge, gated on device
		rxgpu::ScanParams e{};
		e.rows = h->d_rows;
		e.inv_norms = h->d_inv_norms;
		e.queries = d_queries;
		e.n = h->count;
		e.stride = h->stride;
		e.dim = h->dim;
		e.kk = kk;
		e.part_dist = p.sp.part_dist;
		e.part_row = p.sp.part_row;
		e.gate_cnt = cand_cnt;
		e.gate_cap = cap;
		ProfileScope ps(h, "fallback_scan", c->stream);
		rxgpu::launch_scan(h->metric, e, nq, gridx_exact, c->stream);
		rxgpu::launch_merge_lists(e.part_dist, e.part_row, gridx_exact, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream, cand_cnt, cap);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// The int8 tier over a row list: enqueue_knn_pruned_i8 with the gather form of the scan.  Lower bounds are kept per LIST POSITION ([nq][n_ids]);
// the candidate filter maps position -> row, so the re-score and the merges see real rows.  The margin comes from index-wide maxima and is
// therefore sound for any subset of the rows.  Behind the gate: the f32 subset scan, which is what answers this call off the tier.
int enqueue_knn_pruned_i8_subset(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
								 uint64_t n_ids, float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_i8_shadow(h, c->stream); rc) return rc;   // (the row statistics first)
	const uint32_t ld8 = rxgpu::i8_ld(h->dim);
	const uint32_t gridx = rxgpu::scan_i8_subset_grid_x(n_ids, h->cus);
	const uint32_t gridx_exact = rxgpu::subset_grid_x(n_ids, h->dim, kk, h->cus);   // the gated f32 subset scan's
	const uint32_t grid_max = std::max(gridx, gridx_exact);
	const uint32_t cap = uint32_t(std::min<uint64_t>(kPrunedCap, std::max<uint64_t>(64, (n_ids + 63) & ~63ull)));
	if (int rc = c->d_qpad.ensure(size_t(nq) * ld8 * sizeof(float)); rc) return rc;
	if (int rc = c->d_qplanes.ensure(size_t(nq) * 2 * ld8); rc) return rc;
	if (int rc = c->d_qstats.ensure(size_t(4) * nq * sizeof(float)); rc) return rc;
	if (int rc = c->d_dense.ensure(size_t(nq) * n_ids * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_dist.ensure(size_t(nq) * grid_max * kk * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(nq) * grid_max * kk * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_top.ensure(size_t(nq) * (2 * kk + 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_row.ensure(size_t(nq) * cap * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_dist.ensure(size_t(nq) * cap * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
	float* qpad = static_cast<float*>(c->d_qpad.ptr);
	float2* qinfo = static_cast<float2*>(c->d_qstats.ptr);   // [nq] pairs, then [nq] |q|^2, [nq] margins
	float* q_sq = reinterpret_cast<float*>(qinfo + nq);
	float* margin = q_sq + nq;
	float* top_dist = static_cast<float*>(c->d_top.ptr);
	uint32_t* top_row = reinterpret_cast<uint32_t*>(top_dist + size_t(nq) * kk);
	uint32_t* top_cnt = top_row + size_t(nq) * kk;
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	c->pruned_cap = cap;
	rxgpu::launch_query_prep_i8(h->metric, d_queries, nq, h->dim, qpad, static_cast<int8_t*>(c->d_qplanes.ptr), ld8, h->d_stats, q_sq, margin, qinfo,
								cand_cnt, cap, c->stream);
	rxgpu::ScanI8Params p{};
	p.sp.inv_norms = h->d_inv_norms;
	p.sp.n = n_ids;
	p.sp.kk = kk;
	p.sp.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.sp.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	p.codes = h->d_codes_i8;
	p.side = h->d_side_i8;
	p.planes = static_cast<const int8_t*>(c->d_qplanes.ptr);
	p.qinfo = qinfo;
	p.row_sq = h->d_row_sq;
	p.q_sq = q_sq;
	p.ld8 = ld8;
	p.lower = static_cast<float*>(c->d_dense.ptr);
	{
		ProfileScope ps(h, "scan_i8_subset", c->stream);
		rxgpu::launch_scan_i8_subset(h->metric, p, d_ids, nq, gridx, h->cus, c->stream);
	}
	rxgpu::launch_merge_lists(p.sp.part_dist, p.sp.part_row, gridx, kk, nq, top_dist, top_row, top_cnt, c->stream);
	{
		ProfileScope ps(h, "filter_approx", c->stream);
		rxgpu::launch_filter_approx(p.lower, n_ids, top_dist, top_cnt, kk, margin, static_cast<uint32_t*>(c->d_cand_row.ptr), cand_cnt, cap, nq, h->cus,
									c->stream, d_ids);
	}
	{
		ProfileScope ps(h, "rescore", c->stream);
		rxgpu::launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, ld8, h->stride, h->dim, nq, cap, cand_cnt,
							  static_cast<uint32_t*>(c->d_cand_row.ptr), static_cast<float*>(c->d_cand_dist.ptr), c->stream);
	}
	rxgpu::launch_merge(static_cast<float*>(c->d_cand_dist.ptr), static_cast<uint32_t*>(c->d_cand_row.ptr), cap, kk, nq, d_out_dist, d_out_row,
						d_out_count, nullptr, 0, c->stream);
	{   // more listed rows inside the bound than the list holds, or no finite bound: the f32 subset scan + its merge, gated on device
		rxgpu::ScanParams e{};
		e.rows = h->d_rows;
		e.inv_norms = h->d_inv_norms;
		e.queries = d_queries;
		e.n = n_ids;
		e.stride = h->stride;
		e.dim = h->dim;
		e.kk = kk;
		e.part_dist = p.sp.part_dist;
		e.part_row = p.sp.part_row;
		e.gate_cnt = cand_cnt;
		e.gate_cap = cap;
		// While profiling, the slot counts the calls whose gate OPENED for one of the queries (the counts are read back first, which synchronises
		// the stream): a call the pruned chain answered leaves it at 0, like "scan_subset".
		bool opened = false;
		if (h->profiling) {
			std::vector<uint32_t> cnt(nq);
			RX_HIP(hipMemcpyAsync(cnt.data(), cand_cnt, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
			RX_HIP(hipStreamSynchronize(c->stream));
			opened = std::any_of(cnt.begin(), cnt.end(), [&](uint32_t v) { return v > cap; });
		}
		auto fallback = [&] {
			rxgpu::launch_scan_subset(h->metric, e, d_ids, nq, gridx_exact, h->cus, c->stream);
			rxgpu::launch_merge_lists(e.part_dist, e.part_row, gridx_exact, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream, cand_cnt, cap);
		};
		if (opened) {
			ProfileScope ps(h, "fallback_scan", c->stream);
			fallback();
		} else {
			fallback();
		}
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// Pre-filtered search, kk <= kMaxFusedK2: gather-scan over the row list + the usual merge (rows in the lists are real rows, so the
// merge and everything downstream is unchanged).  Where scan_policy_tier_subset says so, the int8-pruned chain above answers instead.
int enqueue_knn_subset(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
					   uint64_t n_ids, float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	// (the device entry point may pass kk > n_ids; the chain runs with kk itself, so a kk above one entry per lane stays off the tier whatever the list)
	const uint32_t eff = kk <= uint32_t(rxgpu::kMaxFusedK) ? uint32_t(std::min<uint64_t>(kk, n_ids)) : kk;
	if (scan_policy_tier_subset(n_ids, h->dim, nq, eff, !h->i8_unavailable, true) == kTierI8) {
		if (int rc = ensure_row_stats(h, c->stream); rc) return rc;   // (automatic mode asks whether the row statistics are finite)
		if (scan_policy_tier_subset(n_ids, h->dim, nq, eff, !h->i8_unavailable, h->stats_finite) == kTierI8) {
			const int rc = enqueue_knn_pruned_i8_subset(h, c, d_queries, nq, kk, d_ids, n_ids, d_out_dist, d_out_row, d_out_count);
			if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) return rc;   // no room for the int8 shadow: the f32 subset scan below
		}
	}
	const uint32_t gridx = rxgpu::subset_grid_x(n_ids, h->dim, kk, h->cus);
	const size_t part = size_t(nq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	rxgpu::ScanParams p{};
	p.rows = h->d_rows;
	p.inv_norms = h->d_inv_norms;
	p.queries = d_queries;
	p.n = n_ids;
	p.stride = h->stride;
	p.dim = h->dim;
	p.kk = kk;
	p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	{
		ProfileScope ps(h, "scan_subset", c->stream);
		rxgpu::launch_scan_subset(h->metric, p, d_ids, nq, gridx, h->cus, c->stream);
	}
	{
		ProfileScope ps(h, "merge", c->stream);
		rxgpu::launch_merge_lists(p.part_dist, p.part_row, gridx, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// Host-facing tail shared by rxgpu_search_knn_subset / _bitmap: queries on the host, the row list already in HBM.
int search_subset_host(rxgpu_index* h, rxgpu_search_ctx* c, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
					   uint64_t n_ids, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	const uint32_t eff = uint32_t(std::min<uint64_t>(kk, n_ids));
	const size_t qbytes = size_t(nq) * h->dim * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, queries, qbytes, hipMemcpyHostToDevice, c->stream));
	if (eff <= uint32_t(rxgpu::kMaxFusedK2)) {
		if (int rc = c->d_out_dist.ensure(size_t(nq) * eff * sizeof(float)); rc) return rc;
		if (int rc = c->d_out_row.ensure(size_t(nq) * eff * sizeof(uint32_t)); rc) return rc;
		if (int rc = c->d_out_count.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
		c->pruned_cap = 0;   // set by a pruned chain
		if (int rc = enqueue_knn_subset(h, c, static_cast<const float*>(c->d_queries.ptr), nq, eff, d_ids, n_ids,
										static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr),
										static_cast<uint32_t*>(c->d_out_count.ptr));
			rc)
			return rc;
		RX_HIP(hipMemcpy2DAsync(out_dist, kk * sizeof(float), c->d_out_dist.ptr, eff * sizeof(float), eff * sizeof(float), nq,
								hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpy2DAsync(out_row, kk * sizeof(uint32_t), c->d_out_row.ptr, eff * sizeof(uint32_t), eff * sizeof(uint32_t), nq,
								hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(out_count, c->d_out_count.ptr, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
		if (h->profiling && nq == 1 && c->pruned_cap) {   // rxgpu_index_last_candidates, as rxgpu_search_knn records it
			uint32_t cnt = 0;
			RX_HIP(hipMemcpy(&cnt, c->d_cand_cnt.ptr, sizeof(cnt), hipMemcpyDeviceToHost));
			h->last_cand_count = cnt;
			h->last_cand_cap = c->pruned_cap;
		}
		return RXGPU_OK;
	}
	// large k: distances of the listed rows + radix select over (dist, position); positions -> rows; final sort of eff entries on the host
	RX_CHECK(n_ids <= (1ull << 28), RXGPU_ERR_PARAMS, "pre-filtered search with k > 128: the row list must not exceed 2^28 entries");
	if (int rc = c->d_misc.ensure(n_ids * sizeof(float)); rc) return rc;
	if (int rc = c->d_select.ensure(rxgpu::select_scratch_bytes(n_ids)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(eff) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	std::vector<float> hd(eff);
	std::vector<uint32_t> hr(eff), order(eff);
	for (uint32_t q = 0; q < nq; ++q) {
		{
			ProfileScope ps(h, "scan_subset", c->stream);
			rxgpu::launch_distances(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr) + size_t(q) * h->dim,
									h->stride, h->dim, d_ids, uint32_t(n_ids), static_cast<float*>(c->d_misc.ptr), c->stream);
		}
		rxgpu::launch_select_smallest(static_cast<const float*>(c->d_misc.ptr), n_ids, eff, c->d_select.ptr, static_cast<float*>(c->d_out_dist.ptr),
									  static_cast<uint32_t*>(c->d_out_row.ptr), c->stream);
		rxgpu::launch_gather_u32(d_ids, static_cast<const uint32_t*>(c->d_out_row.ptr), eff, static_cast<uint32_t*>(c->d_part_row.ptr), c->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpyAsync(hd.data(), c->d_out_dist.ptr, size_t(eff) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(hr.data(), c->d_part_row.ptr, size_t(eff) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
		std::iota(order.begin(), order.end(), 0u);
		std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hd[a] < hd[b] || (!(hd[b] < hd[a]) && hr[a] < hr[b]); });
		for (uint32_t i = 0; i < eff; ++i) {
			out_dist[size_t(q) * kk + i] = hd[order[i]];
			out_row[size_t(q) * kk + i] = hr[order[i]];
		}
		out_count[q] = eff;
	}
	return RXGPU_OK;
}

int enqueue_knn(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
				uint32_t* d_out_row, uint32_t* d_out_count) {
	// (automatic mode asks whether the row statistics are finite: compute them first where everything else already says yes)
	if (scan_bf16_mode() == kScanBf16Auto && scan_policy_tier(h->count, h->dim, nq, !h->bf16_unavailable, !h->i8_unavailable, true) != kTierF32) {
		if (int rc = ensure_row_stats(h, c->stream); rc) return rc;
	}
	if (scan_policy_tier(h->count, h->dim, nq, !h->bf16_unavailable, !h->i8_unavailable, h->stats_finite) == kTierI8) {
		const int rc = enqueue_knn_pruned_i8(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
		if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) return rc;   // no room for the int8 shadow: the bf16 tier below
	}
	if (scan_policy_tier(h->count, h->dim, nq, !h->bf16_unavailable, !h->i8_unavailable, h->stats_finite) == kTierBf16) {
		const int rc = enqueue_knn_pruned(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
		if (!(rc == RXGPU_ERR_NOMEM && h->bf16_unavailable)) return rc;
	}
	if (int(nq) >= batch_min_queries() && nq >= 2) return enqueue_knn_batched(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
	return enqueue_knn_fused(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
}

}  // namespace

extern "C" {

const char* rxgpu_last_error(void) { return rxgpu::g_err.c_str(); }
int rxgpu_abi_version(void) { return RXGPU_ABI_VERSION; }

int rxgpu_scan_policy(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite) {
	return scan_policy_pruned(rows, dim, nq, shadow_available != 0, stats_finite != 0) ? 1 : 0;
}

int rxgpu_scan_tier(uint64_t rows, uint32_t dim, uint32_t nq, int shadow_available, int stats_finite) {
	return int(scan_policy_tier(rows, dim, nq, shadow_available != 0, shadow_available != 0, stats_finite != 0));
}

int rxgpu_scan_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, int shadow_available, int stats_finite) {
	return int(scan_policy_tier_subset(n_ids, dim, nq, kk, shadow_available != 0, stats_finite != 0));
}

int rxgpu_index_last_candidates(const rxgpu_index* h, uint32_t* out_count, uint32_t* out_cap) {
	RX_CHECK(h && out_count && out_cap, RXGPU_ERR_PARAMS, "rxgpu_index_last_candidates: null argument");
	*out_count = h->last_cand_count.load();
	*out_cap = h->last_cand_cap.load();
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
	if (h->d_row_sq) (void)hipFree(h->d_row_sq);
	if (h->d_row_ids) (void)hipFree(h->d_row_ids);
	if (h->d_rows_bf16) (void)hipFree(h->d_rows_bf16);
	if (h->d_codes_i8) (void)hipFree(h->d_codes_i8);
	if (h->d_side_i8) (void)hipFree(h->d_side_i8);
	if (h->d_stats) (void)hipFree(h->d_stats);
	if (h->d_links0) (void)hipFree(h->d_links0);
	if (h->d_upper_off) (void)hipFree(h->d_upper_off);
	if (h->d_upper) (void)hipFree(h->d_upper);
	if (h->d_deleted) (void)hipFree(h->d_deleted);
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_list_off) (void)hipFree(h->d_list_off);
	if (h->d_list_rows) (void)hipFree(h->d_list_rows);
	if (h->d_corr) (void)hipFree(h->d_corr);
	if (h->d_hnsw_stats) (void)hipFree(h->d_hnsw_stats);
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
	// Derived data follows the mutation incrementally (a full recompute streams the whole corpus: 4 ms per 10M x 768 rows).  The row
	// statistics are maxima entering an error BOUND, so folding the new rows in (and never shrinking on deletes) keeps them valid.
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->stats_valid) {
		if (h->metric == RXGPU_METRIC_L2 && h->row_sq_capacity < first_row + n) {
			h->stats_valid = false;
		} else {
			rxgpu::launch_row_stats(dst, h->d_inv_norms ? h->d_inv_norms + first_row : nullptr, n, h->stride, h->dim,
									h->metric == RXGPU_METRIC_L2 ? h->d_row_sq + first_row : nullptr, h->d_stats, h->cus, nullptr);
			if (int rc = read_stats_finite(h, nullptr); rc) return rc;   // maxima never shrink: an index that has held a non-finite row stays on the f32 scan
		}
	}
	if (h->bf16_valid) {
		if (h->bf16_capacity < first_row + n) {
			h->bf16_valid = false;
		} else {
			const uint32_t ld = (h->dim + 63u) & ~63u;
			rxgpu::launch_to_bf16(dst, n, h->stride, h->dim, h->d_rows_bf16, ld, h->cus, nullptr, first_row, h->bf16_blocked);
		}
	}
	if (h->i8_valid) {
		if (h->i8_capacity < first_row + n || !h->stats_valid) {
			h->i8_valid = false;
		} else {   // re-quantise the range; its residual maxima join the statistics words
			const uint32_t ld8 = rxgpu::i8_ld(h->dim);
			rxgpu::launch_i8_build(dst, h->d_inv_norms ? h->d_inv_norms + first_row : nullptr, n, h->stride, h->dim, h->d_codes_i8 + first_row * ld8,
								   h->d_side_i8 + first_row, ld8, h->d_stats, h->cus, nullptr);
			if (int rc = read_stats_finite(h, nullptr); rc) return rc;
		}
	}
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(nullptr));
	return RXGPU_OK;
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
	h->stats_valid = false;
	h->bf16_valid = false;
	h->i8_valid = false;
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
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->stats_valid && h->metric == RXGPU_METRIC_L2) {
		RX_HIP(hipMemcpy(h->d_row_sq + to, h->d_row_sq + from, sizeof(float), hipMemcpyDeviceToDevice));
	}
	if (h->bf16_valid) {
		const uint32_t ld = (h->dim + 63u) & ~63u;
		rxgpu::launch_shadow_move(h->d_rows_bf16, ld, from, to, h->bf16_blocked, nullptr);
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(nullptr));
	}
	if (h->i8_valid) {
		const uint32_t ld8 = rxgpu::i8_ld(h->dim);
		RX_HIP(hipMemcpy(h->d_codes_i8 + to * ld8, h->d_codes_i8 + from * ld8, ld8, hipMemcpyDeviceToDevice));
		RX_HIP(hipMemcpy(h->d_side_i8 + to, h->d_side_i8 + from, sizeof(float2), hipMemcpyDeviceToDevice));
	}
	return RXGPU_OK;
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
	if (count > h->count) {
		h->stats_valid = false;
		h->bf16_valid = false;
		h->i8_valid = false;
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
			if (slot) t_resident.used.push_back(h->serial);
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
	if (h->shard_set) {
		if (nq == 0) return RXGPU_OK;
		if (h->count == 0 || kk == 0) {   // bruteforce.cc:106-108, as on a single device
			std::fill(out_count, out_count + nq, 0u);
			return RXGPU_OK;
		}
		return rxgpu::sharded_search_knn_impl(h, queries, nq, kk, nullptr, 0, out_dist, out_row, out_count);
	}
	if (nq == 0) return RXGPU_OK;
	if (h->count == 0 || kk == 0) {   // bruteforce.cc:106-108
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
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
		if (int rc = run(h, c, static_cast<const float*>(c->d_queries.ptr), nq, eff, static_cast<float*>(c->d_out_dist.ptr),
						 static_cast<uint32_t*>(c->d_out_row.ptr), static_cast<uint32_t*>(c->d_out_count.ptr));
			rc)
			return rc;
		if (eff == kk) {
			RX_HIP(hipMemcpyAsync(out_dist, c->d_out_dist.ptr, size_t(nq) * eff * sizeof(float), hipMemcpyDeviceToHost, c->stream));
			RX_HIP(hipMemcpyAsync(out_row, c->d_out_row.ptr, size_t(nq) * eff * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		} else {
			RX_HIP(hipMemcpy2DAsync(out_dist, kk * sizeof(float), c->d_out_dist.ptr, eff * sizeof(float), eff * sizeof(float), nq,
									hipMemcpyDeviceToHost, c->stream));
			RX_HIP(hipMemcpy2DAsync(out_row, kk * sizeof(uint32_t), c->d_out_row.ptr, eff * sizeof(uint32_t), eff * sizeof(uint32_t), nq,
									hipMemcpyDeviceToHost, c->stream));
		}
		RX_HIP(hipMemcpyAsync(out_count, c->d_out_count.ptr, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
		if (h->profiling && nq == 1 && c->pruned_cap) {   // rxgpu_index_last_candidates: what the pruned chain of this call nominated
			uint32_t cnt = 0;
			RX_HIP(hipMemcpy(&cnt, c->d_cand_cnt.ptr, sizeof(cnt), hipMemcpyDeviceToHost));
			h->last_cand_count = cnt;
			h->last_cand_cap = c->pruned_cap;
		}
		return RXGPU_OK;
	}

	// large-k path: distance pass + radix select per query, final (dist,row) sort of kk entries on the host
	if (int rc = c->d_misc.ensure(h->count * sizeof(float)); rc) return rc;
	if (int rc = c->d_select.ensure(rxgpu::select_scratch_bytes(h->count)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(eff) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	const uint32_t gridx = rxgpu::scan_grid_x(h->count, h->cus);
	std::vector<float> hd(eff);
	std::vector<uint32_t> hr(eff), order(eff);
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
		std::iota(order.begin(), order.end(), 0u);
		std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
			return hd[a] < hd[b] || (!(hd[b] < hd[a]) && hr[a] < hr[b]);
		});
		for (uint32_t i = 0; i < eff; ++i) {
			out_dist[size_t(q) * kk + i] = hd[order[i]];
			out_row[size_t(q) * kk + i] = hr[order[i]];
		}
		out_count[q] = eff;
	}
	return RXGPU_OK;
}

int rxgpu_search_knn_subset(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* row_ids, uint64_t n_ids,
							float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(queries && out_dist && out_row && out_count && (n_ids == 0 || row_ids), RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset: null argument");
	if (h->shard_set) {
		if (nq == 0) return RXGPU_OK;
		RX_CHECK(kk >= 1, RXGPU_ERR_PARAMS, "rxgpu_search_knn_subset: kk must be >= 1");
		if (n_ids == 0) {
			std::fill(out_count, out_count + nq, 0u);
			return RXGPU_OK;
		}
		return rxgpu::sharded_search_knn_impl(h, queries, nq, kk, row_ids, n_ids, out_dist, out_row, out_count);
	}
	if (nq == 0) return RXGPU_OK;
	for (uint64_t i = 0; i < n_ids; ++i) {
		RX_CHECK(row_ids[i] < h->count && (i == 0 || row_ids[i - 1] < row_ids[i]), RXGPU_ERR_PARAMS,
				 "rxgpu_search_knn_subset: row_ids must be strictly increasing and below the row count");
	}
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
	const uint32_t tiles = rxgpu::bitmap_tiles(h->count);
	if (int rc = c->d_bitmap.ensure(need_words * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_tiles.ensure(size_t(2) * tiles * sizeof(uint32_t) + sizeof(unsigned long long)); rc) return rc;
	uint32_t* tile_scratch = static_cast<uint32_t*>(c->d_tiles.ptr);
	unsigned long long* d_total = reinterpret_cast<unsigned long long*>(tile_scratch + size_t(2) * tiles);   // 8-byte aligned: 2 * tiles words
	RX_HIP(hipMemcpyAsync(c->d_bitmap.ptr, allowed_words, need_words * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	{
		ProfileScope ps(h, "bitmap", c->stream);
		rxgpu::launch_bitmap_count(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, d_total, c->stream);
	}
	RX_HIP(hipGetLastError());
	unsigned long long total = 0;
	RX_HIP(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	if (out_allowed) *out_allowed = total;
	if (total == 0 || kk == 0) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	if (int rc = c->d_subset.ensure(total * sizeof(uint32_t)); rc) return rc;
	{
		ProfileScope ps(h, "bitmap", c->stream);
		rxgpu::launch_bitmap_expand(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, static_cast<uint32_t*>(c->d_subset.ptr),
									total, c->stream);
	}
	RX_HIP(hipGetLastError());
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
	return RXGPU_OK;
}

namespace {
// The probed lists of one query as an ascending row list in c->d_subset, everything on the device: nprobe nearest centroids (the coarse
// quantiser's search; up to 128 lists its result never leaves HBM, wider probes fetch the list ids — nprobe words — and send them back),
// lists -> allowed-rows bitmap -> row list.  *total = rows to scan.
int ivf_probe_rows(rxgpu_index* h, rxgpu_index* coarse, rxgpu_search_ctx* c, const float* query, uint32_t nprobe, unsigned long long* total, const char* who) {
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
	const uint32_t tiles = rxgpu::bitmap_tiles(h->count);
	if (int rc = c->d_bitmap.ensure(need_words * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_tiles.ensure(size_t(2) * tiles * sizeof(uint32_t) + sizeof(unsigned long long)); rc) return rc;
	uint32_t* tile_scratch = static_cast<uint32_t*>(c->d_tiles.ptr);
	unsigned long long* d_total = reinterpret_cast<unsigned long long*>(tile_scratch + size_t(2) * tiles);
	RX_HIP(hipMemsetAsync(c->d_bitmap.ptr, 0, need_words * sizeof(uint32_t), c->stream));
	{
		ProfileScope ps(h, "ivf_lists", c->stream);
		rxgpu::launch_ivf_mark_lists(reinterpret_cast<const uint32_t*>(ivf + o_lists), reinterpret_cast<const uint32_t*>(ivf + o_cnt), nprobe, h->d_list_off,
									 h->d_list_rows, static_cast<uint32_t*>(c->d_bitmap.ptr), c->stream);
		rxgpu::launch_bitmap_count(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, d_total, c->stream);
	}
	RX_HIP(hipGetLastError());
	*total = 0;
	RX_HIP(hipMemcpyAsync(total, d_total, sizeof(*total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	if (*total == 0) return RXGPU_OK;
	if (int rc = c->d_subset.ensure(*total * sizeof(uint32_t)); rc) return rc;
	{
		ProfileScope ps(h, "ivf_lists", c->stream);
		rxgpu::launch_bitmap_expand(static_cast<const uint32_t*>(c->d_bitmap.ptr), h->count, tile_scratch, static_cast<uint32_t*>(c->d_subset.ptr), *total,
									c->stream);
	}
	RX_HIP(hipGetLastError());
	(void)who;
	return RXGPU_OK;
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
	if (int rc = ivf_probe_rows(h, coarse, c, query, nprobe, &total, "rxgpu_search_knn_lists"); rc) return rc;
	if (out_scanned) *out_scanned = total;
	if (total == 0) return RXGPU_OK;
	return search_subset_host(h, c, query, 1, kk, static_cast<const uint32_t*>(c->d_subset.ptr), total, out_dist, out_row, out_count);
}

namespace {
// range search over a row list that lies in c->d_subset (query in c->d_queries): the tail of rxgpu_search_range_subset
int range_subset_on_device(rxgpu_index* h, rxgpu_search_ctx* c, uint64_t n_ids, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
						   uint64_t* out_total, const char* who) {
	const uint64_t dcap = std::min<uint64_t>(cap, n_ids);
	if (int rc = c->d_out_dist.ensure(std::max<uint64_t>(dcap, 1) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(std::max<uint64_t>(dcap, 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_count.ensure(sizeof(unsigned long long)); rc) return rc;
	RX_HIP(hipMemsetAsync(c->d_out_count.ptr, 0, sizeof(unsigned long long), c->stream));
	{
		ProfileScope ps(h, "range_subset", c->stream);
		rxgpu::launch_range_subset(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr),
								   static_cast<const uint32_t*>(c->d_subset.ptr), n_ids, h->stride, h->dim, radius, inclusive,
								   static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), dcap,
								   static_cast<unsigned long long*>(c->d_out_count.ptr), rxgpu::scan_grid_x(n_ids, h->cus), c->stream);
	}
	RX_HIP(hipGetLastError());
	unsigned long long total = 0;
	RX_HIP(hipMemcpyAsync(&total, c->d_out_count.ptr, sizeof(total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	*out_total = total;
	if (total > cap) {
		set_error(std::string(who) + ": output buffer too small");
		return RXGPU_ERR_OVERFLOW;
	}
	if (total == 0) return RXGPU_OK;
	std::vector<float> hd(total);
	std::vector<uint32_t> hr(total), order(total);
	RX_HIP(hipMemcpy(hd.data(), c->d_out_dist.ptr, total * sizeof(float), hipMemcpyDeviceToHost));
	RX_HIP(hipMemcpy(hr.data(), c->d_out_row.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hd[a] < hd[b] || (!(hd[b] < hd[a]) && hr[a] < hr[b]); });
	for (uint64_t i = 0; i < total; ++i) {
		out_dist[i] = hd[order[i]];
		out_row[i] = hr[order[i]];
	}
	return RXGPU_OK;
}
}  // namespace

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
	if (int rc = ivf_probe_rows(h, coarse, c, query, nprobe, &total, "rxgpu_search_range_lists"); rc) return rc;
	if (out_scanned) *out_scanned = total;
	if (total == 0) return RXGPU_OK;
	return range_subset_on_device(h, c, total, radius, inclusive, out_dist, out_row, cap, out_total, "rxgpu_search_range_lists");
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
	if (h->shard_set) {
		*out_total = 0;
		return rxgpu::sharded_search_range_impl(h, query, radius, inclusive, nullptr, 0, out_dist, out_row, cap, out_total);
	}
	*out_total = 0;
	if (h->count == 0) return RXGPU_OK;   // bruteforce.cc:132-134
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	const uint64_t dcap = std::min<uint64_t>(cap, h->count);
	if (int rc = c->d_queries.ensure(h->dim * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(std::max<uint64_t>(dcap, 1) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(std::max<uint64_t>(dcap, 1) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_out_count.ensure(sizeof(unsigned long long)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, h->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
	RX_HIP(hipMemsetAsync(c->d_out_count.ptr, 0, sizeof(unsigned long long), c->stream));
	{
		ProfileScope ps(h, "range", c->stream);
		rxgpu::launch_range(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr), h->count, h->stride, h->dim,
							radius, inclusive, static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), dcap,
							static_cast<unsigned long long*>(c->d_out_count.ptr), rxgpu::scan_grid_x(h->count, h->cus), c->stream);
	}
	RX_HIP(hipGetLastError());
	unsigned long long total = 0;
	RX_HIP(hipMemcpyAsync(&total, c->d_out_count.ptr, sizeof(total), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	*out_total = total;
	if (total > cap) {
		set_error("rxgpu_search_range: output buffer too small");
		return RXGPU_ERR_OVERFLOW;
	}
	if (total == 0) return RXGPU_OK;
	std::vector<float> hd(total);
	std::vector<uint32_t> hr(total), order(total);
	RX_HIP(hipMemcpy(hd.data(), c->d_out_dist.ptr, total * sizeof(float), hipMemcpyDeviceToHost));
	RX_HIP(hipMemcpy(hr.data(), c->d_out_row.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hd[a] < hd[b] || (!(hd[b] < hd[a]) && hr[a] < hr[b]); });
	for (uint64_t i = 0; i < total; ++i) {
		out_dist[i] = hd[order[i]];
		out_row[i] = hr[order[i]];
	}
	return RXGPU_OK;
}

int rxgpu_search_range_subset(rxgpu_index* h, const float* query, float radius, int inclusive, const uint32_t* row_ids, uint64_t n_ids,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query && out_total && (cap == 0 || (out_dist && out_row)) && (n_ids == 0 || row_ids), RXGPU_ERR_PARAMS,
			 "rxgpu_search_range_subset: null argument");
	if (h->shard_set) {
		*out_total = 0;
		if (n_ids == 0) return RXGPU_OK;
		return rxgpu::sharded_search_range_impl(h, query, radius, inclusive, row_ids, n_ids, out_dist, out_row, cap, out_total);
	}
	*out_total = 0;
	for (uint64_t i = 0; i < n_ids; ++i) {
		RX_CHECK(row_ids[i] < h->count && (i == 0 || row_ids[i - 1] < row_ids[i]), RXGPU_ERR_PARAMS,
				 "rxgpu_search_range_subset: row_ids must be strictly increasing and below the row count");
	}
	if (n_ids == 0) return RXGPU_OK;
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	if (int rc = c->d_queries.ensure(h->dim * sizeof(float)); rc) return rc;
	if (int rc = c->d_subset.ensure(n_ids * sizeof(uint32_t)); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, query, h->dim * sizeof(float), hipMemcpyHostToDevice, c->stream));
	RX_HIP(hipMemcpyAsync(c->d_subset.ptr, row_ids, n_ids * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	return range_subset_on_device(h, c, n_ids, radius, inclusive, out_dist, out_row, cap, out_total, "rxgpu_search_range_subset");
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
