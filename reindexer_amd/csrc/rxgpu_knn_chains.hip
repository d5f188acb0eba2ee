// The host-side chains of brute-force KNN: which scan a call takes (the policy), and the launches of each chain — fused f32 scan, batched
// nomination (f32 / bf16 GEMM) with its exact tail, the pruned chains (bf16 / int8 / int8 over a row list / 6-bit) with theirs, the pre-filtered
// scan.  Called by the entry points of rxgpu_knn_search.hip through rxgpu_internal.h.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cstdlib>

#include "../../include/rxgpu.h"
#include "knn_emit_plan.h"
#include "knn_i6_quant.h"
#include "knn_i8_quant.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"
#include "shard_plan.h"   // dist_row_less

namespace rxgpu {
namespace {

// The one place that fills ScanParams: n rows (the index's, or the entries of a row list), kk, and the context's part buffers, which the
// caller has ensured for its grid.  With d_queries, the f32 scan's: rows and queries as well, and optionally the gate (the scan runs only for
// queries with gate_cnt[q] > gate_cap: the exact scan behind a nomination).  Without, the part a pruning scan over a shadow reads (it has
// queries and rows of its own): the other fields stay zero.
ScanParams scan_params(const rxgpu_index* h, const rxgpu_search_ctx* c, const float* d_queries, uint64_t n, uint32_t kk,
					   const uint32_t* gate_cnt = nullptr, uint32_t gate_cap = 0) {
	ScanParams p{};
	p.inv_norms = h->d_inv_norms;
	p.n = n;
	p.kk = kk;
	p.part_dist = static_cast<float*>(c->d_part_dist.ptr);
	p.part_row = static_cast<uint32_t*>(c->d_part_row.ptr);
	if (d_queries) {
		p.rows = h->d_rows;
		p.queries = d_queries;
		p.stride = h->stride;
		p.dim = h->dim;
		p.gate_cnt = gate_cnt;
		p.gate_cap = gate_cap;
	}
	return p;
}

}  // namespace

// Enqueue scan + merge for nq device-resident queries; results land in d_out_* (device).
int enqueue_knn_fused(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
					  uint32_t* d_out_row, uint32_t* d_out_count) {
	const uint32_t gridx = scan_grid_x(h->count, h->cus);
	const size_t part = size_t(nq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	const ScanParams p = scan_params(h, c, d_queries, h->count, kk);
	{
		ProfileScope ps(h, "scan", c->stream);
		launch_scan(h->metric, p, nq, gridx, c->stream);
	}
	{
		ProfileScope ps(h, "merge", c->stream);
		launch_merge_lists(p.part_dist, p.part_row, gridx, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

namespace {

// ---- batched path (nq >= 2): MFMA candidate generation + exact re-score, see knn_batched.hip ----------------------
constexpr uint32_t kBatchSampleRows = 32768;
constexpr uint32_t kBatchSampleRowsBf16 = 131072;   // the sample pass is cheap on the bf16 pipe; a tighter threshold pays for the wider margin

int batch_min_queries() {
	static const int v = [] {
		const char* e = getenv("RXGPU_BATCH_MIN");
		return e ? atoi(e) : 2;
	}();
	return v;
}

int batch_bf16_min_queries() {   // read per call (tests and A/B runs switch it)
	const char* e = getenv("RXGPU_BATCH_BF16_MIN");   // 0 disables the bf16 nomination path
	return e ? atoi(e) : 2;   // measured at 10M x 768: 4.8-5.0 ms per batch for 8..256 queries against 6.2-10.6 ms on the f32 rows
}

// Candidate capacity per query of a nomination over a sample of ns rows: expected nominations ~ kk * n / ns (plus the margin) times the
// headroom; overflow falls back to the exact scan.
uint32_t batched_cap(const rxgpu_index* h, uint32_t kk, uint64_t ns, uint32_t headroom) {
	uint64_t cap64 = std::max<uint64_t>(4096, headroom * uint64_t(kk) * ((h->count + ns - 1) / ns));
	cap64 = std::min<uint64_t>(cap64, std::max<uint64_t>(h->count, 64));
	return uint32_t((cap64 + 63) & ~63ull);
}

// The exact tail behind both nomination forms, over the cq queries of one chunk (d_queries, d_out_* at the chunk's first query): re-score
// of the nominated rows (d_cand_row, counted in d_cand_cnt) against the padded queries, top-kk, and for the queries whose nominations
// overflowed cap the exact fused scan, gated on the device.  The part buffers are ensured here, behind the nomination launches: nothing
// enqueued earlier uses them.
int enqueue_batched_tail(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t cq, uint32_t kk, const float* qpad, uint32_t q_stride,
						 uint32_t cap, float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	uint32_t* cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
	float* cand_dist = static_cast<float*>(c->d_cand_dist.ptr);
	{
		ProfileScope ps(h, "rescore", c->stream);
		launch_rescore(h->metric, h->d_rows, h->d_inv_norms, qpad, q_stride, h->stride, h->dim, cq, cap, cand_cnt, cand_row, cand_dist, c->stream);
	}
	launch_merge(cand_dist, cand_row, cap, kk, cq, d_out_dist, d_out_row, d_out_count, nullptr, 0, c->stream);
	const uint32_t gridx = scan_grid_x(h->count, h->cus);
	const size_t part = size_t(cq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	const ScanParams p = scan_params(h, c, d_queries, h->count, kk, cand_cnt, cap);
	{
		ProfileScope ps(h, "fallback_scan", c->stream);
		launch_scan(h->metric, p, cq, gridx, c->stream);
		launch_merge(p.part_dist, p.part_row, gridx * kk, kk, cq, d_out_dist, d_out_row, d_out_count, cand_cnt, cap, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// Every batch (2..256 queries at a time): nomination on the bf16 MFMA pipe over the bf16 shadow (knn_batched_bf16.hip), then the exact tail.
int enqueue_knn_batched_bf16(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t q0, uint32_t cq, uint32_t kk,
							 float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_bf16_shadow(h, c->stream); rc) return rc;
	const uint32_t mt = cq <= 128 ? 128 : 256;   // query-tile width of the nomination kernel
	const uint32_t ld = (h->dim + 63u) & ~63u;
	const uint32_t q_stride = ld;   // the f32 copy for the exact re-score shares the padded stride
	const uint64_t ns = std::min<uint64_t>(h->count, kBatchSampleRowsBf16);
	const uint32_t cap = batched_cap(h, kk, ns, 10);   // (the bf16 margin nominates ~3 times as many)
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
	launch_to_bf16(qpad, mt, q_stride, q_stride, qbf, ld, h->cus, c->stream);
	launch_query_stats(h->metric, qpad, cq, mt, q_stride, h->dim, h->d_stats, q_sq, margin, true, c->stream);

	GemmBf16Params g{};
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
		RX_HIP(launch_gemm_bf16(h->metric, kGemmDense, int(mt), g, grid_for(ns), c->stream));
	}
	launch_sample_threshold(g.dense, ns, cq, mt, kk, margin, thr, c->stream);
	g.n = h->count;
	g.row_step = 1;
	g.dense = nullptr;
	g.thr = thr;
	g.cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
	g.cand_cnt = cand_cnt;
	g.cap = cap;
	{
		ProfileScope ps(h, "gemm", c->stream);
		RX_HIP(launch_gemm_bf16(h->metric, kGemmFilter, int(mt), g, grid_for(h->count), c->stream));
	}
	return enqueue_batched_tail(h, c, d_queries + size_t(q0) * h->dim, cq, kk, qpad, q_stride, cap, d_out_dist + size_t(q0) * kk,
								d_out_row + size_t(q0) * kk, d_out_count ? d_out_count + q0 : nullptr);
}

int enqueue_knn_batched(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
						uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = ensure_row_stats(h, c->stream); rc) return rc;
	const uint32_t q_stride = (h->dim + 31u) & ~31u;
	const uint64_t ns = std::min<uint64_t>(h->count, kBatchSampleRows);
	const uint32_t cap = batched_cap(h, kk, ns, 4);
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
		launch_query_stats(h->metric, qpad, cq, mt, q_stride, h->dim, h->d_stats, q_sq, margin, false, c->stream);

		GemmParams g{};
		g.rows = h->d_rows;
		g.inv_norms = h->d_inv_norms;
		g.row_sq = h->d_row_sq;
		g.queries = qpad;
		g.q_sq = q_sq;
		g.stride = h->stride;
		g.dim = h->dim;
		g.nq = cq;
		g.q_stride = q_stride;
		const uint32_t wg_per_cu = uint32_t(std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / gemm_lds_bytes(mt))));
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
			RX_HIP(launch_gemm(h->metric, mt, kGemmDense, g, grid_for(ns), c->stream));
		}
		// 3. thresholds
		launch_sample_threshold(g.dense, ns, cq, mt, kk, margin, thr, c->stream);
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
			RX_HIP(launch_gemm(h->metric, mt, kGemmFilter, g, grid_for(h->count), c->stream));
		}
		// 5. exact re-score, 6. exact top-kk, overflow fallback
		if (int rc = enqueue_batched_tail(h, c, d_queries + size_t(q0) * h->dim, cq, kk, qpad, q_stride, cap, d_out_dist + size_t(q0) * kk,
										  d_out_row + size_t(q0) * kk, d_out_count ? d_out_count + q0 : nullptr);
			rc)
			return rc;
	}
	return RXGPU_OK;
}

// ---- which scan a call takes ----------------------------------------------------------------------------------------
// bf16-pruned scan for one .. a few queries: 2 bytes per element from HBM instead of 4, exact result (the chain: header of knn_scan_bf16 in knn_scan.hip; its filter and merges: knn_filter.hip, knn_merge.hip).
// RXGPU_SCAN_BF16, read per call (a process can switch it for A/B runs): 1 = forced on (up to kPrunedMaxQueries queries, any size), 0 = forced
// off (the f32 paths, always), unset = automatic: single queries on indexes of at least kPrunedAutoMinBytes of f32 rows.
enum ScanBf16Mode { kScanBf16Off = 0, kScanBf16On = 1, kScanBf16Auto = 2 };
ScanBf16Mode scan_bf16_mode() {
	const char* e = getenv("RXGPU_SCAN_BF16");
	if (!e || !*e) return kScanBf16Auto;
	return atoi(e) != 0 ? kScanBf16On : kScanBf16Off;
}
constexpr uint32_t kPrunedMaxQueries = 8;
// Automatic mode: the pruned path pays a fixed tail per query (filter, re-score, two merges, the gated scan) and saves half the streaming; it
// also costs +2 bytes per element of HBM.  Never below 1 GiB (small indexes keep the f32 kernel and their footprint); measured crossover in
// profiles/scan_policy_crossover.json.  RXGPU_SCAN_BF16_MIN_BYTES overrides it (tests exercise the decision on small corpora).
constexpr uint64_t kPrunedAutoMinBytes = 1ull << 30;
uint64_t pruned_auto_min_bytes() {
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
ScanBf16Mode scan_i8_mode() {
	const char* e = getenv("RXGPU_SCAN_I8");
	if (!e || !*e) return kScanBf16Auto;
	return atoi(e) != 0 ? kScanBf16On : kScanBf16Off;
}
uint64_t pruned_i8_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I8_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI8AutoMinBytes;
}
// The same decision for a search over a ROW LIST (scan_policy_tier_subset).  kPrunedI8SubsetAutoMinBytes is meant to be the measured
// crossover against the f32 subset scan (tools/bench_prefilter_i8.py), rounded up to a power of two and never below 1 GiB.  That crossover
// has NOT been measured yet, so the default is the maximum value: the tier is forced-only (RXGPU_SCAN_I8=1) or opted into
// with RXGPU_SCAN_I8_SUBSET_MIN_BYTES, which overrides the default.
constexpr uint64_t kPrunedI8SubsetAutoMinBytes = ~0ull;
uint64_t pruned_i8_subset_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I8_SUBSET_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI8SubsetAutoMinBytes;
}
// ... and for a RANGE call (scan_policy_tier_range).  kPrunedI8RangeAutoMinBytes is the measured crossover against the f32 range kernel
// (tools/bench_range_i8.py, profiles/range_i8_ab.json: 10M .. 350k x 768, radii of 10 / 1 000 / 100 000 hits and the tie replay), rounded up to
// a power of two and never below 1 GiB.  The tier wins every shape beyond the spread from 15.4 GB of f32 rows on (1.19 against 8.24 ms per
// call at 10M x 768, 10 hits); below that it still wins the small results at every size measured (0.13 against 0.35 ms at 1 GiB) but only
// ties at 100 000 hits, where the host-side sort of the hits is the call.  The rule asks for every shape: 2^34.  RXGPU_SCAN_I8_RANGE_MIN_BYTES
// overrides it.
constexpr uint64_t kPrunedI8RangeAutoMinBytes = 1ull << 34;
uint64_t pruned_i8_range_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I8_RANGE_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI8RangeAutoMinBytes;
}

// The 6-bit front (knn_scan_i6.hip) refines a call of the int8 tier: the same chain reads a 6-bit shadow (0.75 bytes per element) behind a seed
// pass.  RXGPU_SCAN_I6, read per call: 0 = off, 1 = forced at any size (up to kPrunedMaxQueries queries; for tests and A/B), unset = automatic:
// a call the automatic rules above give to the int8 tier, on an index of at least kPrunedI6AutoMinBytes of f32 rows.  RXGPU_SCAN_BF16=0 / =1 and
// RXGPU_SCAN_I8=0 / =1 win over it as documented above: RXGPU_SCAN_I8=1 means the int8 front, exactly.
// kPrunedI6AutoMinBytes: the measured crossover against the int8 front and every other series (tools/scan_policy_crossover.py, series i6;
// profiles/scan_i6_crossover.json: at 768 dims the front loses up to 6.1 GB of f32 rows - its seed pass, its merge and a tail over thousands of
// candidates cost about 65 us - and wins beyond the spread from 12.3 GB on), rounded up to a power of two and never below 1 GiB: 2^34.  The
// automatic mode is on because the headline A/B shows the gain beyond both spreads (profiles/scan_i6_headline_ab.json).
// RXGPU_SCAN_I6_MIN_BYTES overrides it.
constexpr uint64_t kPrunedI6AutoMinBytes = 1ull << 34;
ScanBf16Mode scan_i6_mode() {
	const char* e = getenv("RXGPU_SCAN_I6");
	if (!e || !*e) return kScanBf16Auto;
	return atoi(e) != 0 ? kScanBf16On : kScanBf16Off;
}
uint64_t pruned_i6_auto_min_bytes() {
	const char* e = getenv("RXGPU_SCAN_I6_MIN_BYTES");
	return e && *e ? strtoull(e, nullptr, 10) : kPrunedI6AutoMinBytes;
}

}  // namespace

// The whole decision, without a device: which scan does a call with nq queries on rows x dim f32 rows take?
ScanTier scan_policy_tier(uint64_t rows, uint32_t dim, uint32_t nq, bool bf16_available, bool i8_available, bool stats_finite) {
	const ScanBf16Mode mode = scan_bf16_mode();
	if (mode == kScanBf16Off) return kTierF32;
	const ScanBf16Mode i8 = scan_i8_mode();
	const bool i8_can = mode == kScanBf16Auto && i8 != kScanBf16Off && i8_available && i8_dim_supported(dim);
	if (i8_can && i8 == kScanBf16On && nq <= kPrunedMaxQueries) return kTierI8;
	if (!bf16_available || !scan_bf16_supported((dim + 63u) & ~63u)) return kTierF32;
	if (mode == kScanBf16On) return nq <= kPrunedMaxQueries ? kTierBf16 : kTierF32;
	if (!(nq == 1 && stats_finite && rows * dim * sizeof(float) >= pruned_auto_min_bytes())) return kTierF32;
	return i8_can && rows * dim * sizeof(float) >= pruned_i8_auto_min_bytes() ? kTierI8 : kTierBf16;
}
// Does such a call read the 6-bit shadow?  A refinement inside the int8 tier: scan_policy_tier does not know RXGPU_SCAN_I6 and keeps its
// answers; the forced mode takes a call at any size, as RXGPU_SCAN_I8=1 does.
bool scan_policy_i6(uint64_t rows, uint32_t dim, uint32_t nq, bool i6_available, bool stats_finite) {
	const ScanBf16Mode mode = scan_i6_mode();
	if (mode == kScanBf16Off || !i6_available || !i6_dim_supported(dim)) return false;
	if (scan_bf16_mode() != kScanBf16Auto || scan_i8_mode() != kScanBf16Auto) return false;
	if (mode == kScanBf16On) return nq <= kPrunedMaxQueries;
	if (scan_policy_tier(rows, dim, nq, true, true, stats_finite) != kTierI8) return false;
	return rows * dim * sizeof(float) >= pruned_i6_auto_min_bytes();
}
// ... does it take a pruned scan at all?
bool scan_policy_pruned(uint64_t rows, uint32_t dim, uint32_t nq, bool shadow_available, bool stats_finite) {
	return scan_policy_tier(rows, dim, nq, shadow_available, shadow_available, stats_finite) != kTierF32;
}
// The same decision for a search over a ROW LIST (enqueue_knn_subset: pre-filtered search, IVF, their per-shard calls): the f32 subset scan or the
// int8-pruned one (knn_scan_i8_subset; the bf16 tier has no subset form, so RXGPU_SCAN_BF16=1, "the bf16 tier, exactly", keeps the f32 scan).
// kk is min(kk, n_ids); the pruned chain keeps one list entry per lane, so kk in 65..128 stays on the f32 subset scan.  The automatic rule
// counts the f32 bytes of the LISTED rows, not of the index: small lists keep their kernel and an index that only sees selective filters never
// builds the shadow.
ScanTier scan_policy_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, bool i8_available, bool stats_finite) {
	if (scan_bf16_mode() != kScanBf16Auto) return kTierF32;
	const ScanBf16Mode i8 = scan_i8_mode();
	if (i8 == kScanBf16Off || !i8_available || !i8_dim_supported(dim) || kk > uint32_t(kMaxFusedK) || n_ids == 0) return kTierF32;
	if (i8 == kScanBf16On) return nq <= kPrunedMaxQueries ? kTierI8 : kTierF32;   // without a finite bound the gate answers, as in the unfiltered tier
	return nq == 1 && stats_finite && n_ids * dim * sizeof(float) >= pruned_i8_subset_auto_min_bytes() ? kTierI8 : kTierF32;
}

// The same decision for a RANGE call (one query; rxgpu_search_range, _subset, _lists and their per-shard calls): the f32 range kernel or the
// int8-pruned one (knn_range_i8 / knn_range_i8_subset).  rows: the rows scanned, the index's or the entries of the list.  There is no bf16
// form, so RXGPU_SCAN_BF16=1 keeps the f32 kernel like =0.  The automatic rule counts the f32 bytes of the scanned rows against
// RXGPU_SCAN_I8_RANGE_MIN_BYTES, and a list call against RXGPU_SCAN_I8_SUBSET_MIN_BYTES as well, like a KNN search over a list.
ScanTier scan_policy_tier_range(uint64_t rows, uint32_t dim, bool list, bool i8_available, bool stats_finite) {
	if (scan_bf16_mode() != kScanBf16Auto) return kTierF32;
	const ScanBf16Mode i8 = scan_i8_mode();
	if (i8 == kScanBf16Off || !i8_available || !i8_dim_supported(dim) || rows == 0) return kTierF32;
	if (i8 == kScanBf16On) return kTierI8;   // without a finite bound the f32 kernel answers behind the scan
	const uint64_t bytes = rows * dim * sizeof(float);
	if (!stats_finite || bytes < pruned_i8_range_auto_min_bytes()) return kTierF32;
	return list && bytes < pruned_i8_subset_auto_min_bytes() ? kTierF32 : kTierI8;
}

namespace {

// ---- the pruned chains (one .. kPrunedMaxQueries queries) --------------------------------------------------------------
// A cheap scan over a shadow of the rows leaves a value per row (an approximate distance, or a lower bound) and approximate top lists; the
// rows that can still belong to the result are filtered out of the values, re-scored exactly and merged.  Queries with more such rows than
// the candidate list holds (massive ties), or without a finite bound, are answered by the exact f32 scan behind a gate on the device.
constexpr uint32_t kPrunedCap = 4096;
uint32_t pruned_cap(uint64_t n, uint32_t most = kPrunedCap) { return uint32_t(std::min<uint64_t>(most, std::max<uint64_t>(64, (n + 63) & ~63ull))); }
// RXGPU_SCAN_I8_EMIT, read per call (A/B runs inside one process): 0 = the int8 scan stores a value per row and knn_filter_approx reads them
// all back (the sequence before the scan emitted); else / unset = the scan emits, knn_filter_emitted reads what it emitted.
bool scan_i8_emits() {
	const char* e = getenv("RXGPU_SCAN_I8_EMIT");
	return !(e && *e && atoi(e) == 0);
}

// What the chain carves out of the context's buffers for its front.
struct PrunedBufs {
	float* qpad;          // [nq][ld] zero-padded f32 queries (the re-score reads them too)
	float* qstats;        // [nq][qstats_floats - 2] whatever else the front keeps per query
	float* q_sq;          // [nq]
	float* margin;        // [nq]
	float* values;        // [nq][n] the scan's value per row (list position); an emitting front writes it only where keep is set
	uint32_t* cand_cnt;   // [nq]
	uint32_t cap;
	// an emitting front (PrunedFront::emits): the rows the scan emitted, and whether it keeps a value per row as well
	EmitEntry* emit;      // [nq][n]
	uint32_t* emit_cnt;   // [nq][wavefronts of the scan's grid]
	bool keep;
};
// The front of a pruned chain: the only place where the tiers differ.
struct PrunedFront {
	int (*ensure_shadow)(rxgpu_index* h, hipStream_t s);   // the derived data the front reads
	uint32_t ld;              // padded query stride (floats)
	uint32_t qstats_floats;   // d_qstats floats per query: |q|^2 and the margin, behind whatever the front adds
	bool planes;              // d_qplanes is needed
	// Which filter form the scan feeds.  false: a value per row in b.values, knn_filter_approx reads all of them.  true: the scan emits the rows
	// that can still be candidates (knn_emit_plan.h), knn_filter_emitted reads those; b.values is written only for a recording call (b.keep).
	bool emits;
	bool many_candidates;     // an emitting front whose filter leaves thousands of rows: knn_filter_emitted_wide
	uint64_t n;               // rows scanned: the index's, or the entries of ids
	const uint32_t* ids;      // the row list (null: every row); decides the exact scan behind the gate as well
	uint32_t cap;             // candidates the list holds per query (a multiple of 64)
	uint32_t gridx;           // the pruning scan's grid ...
	uint32_t gridx_exact;     // ... and the gated exact scan's (scan_grid_x, or subset_grid_x over a row list)
	const char* scan_slot;    // profile slot of the pruning scan
	// An optional pass in front of the scan, under a profile slot of its own (the 6-bit front's seed pass and its merge).  It may use the part
	// buffers: the scan overwrites them afterwards.
	const char* seed_slot;
	void (*seed)(rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b);
	// The profile slot of the gated exact scan: false = filed for every call.  true = while profiling, the slot counts the calls whose gate
	// OPENED for one of the queries (the counts are read back first, which synchronises the stream): a call the pruned chain answered
	// leaves it at 0, like "scan_subset".
	bool fallback_slot_when_opened;
	// one launch: padded copy of the query, |q|^2, margin, cand_cnt = 0 (cap + 1 for a query without a finite bound: the gated exact scan answers it)
	void (*prep)(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, const PrunedFront& f, const PrunedBufs& b);
	// the pruning scan: sp (n, kk, inv_norms, part buffers) is filled in; leaves b.values and a sorted list of kk entries per workgroup
	void (*scan)(rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b);
};

int enqueue_knn_pruned_chain(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const PrunedFront& f,
							 float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	if (int rc = f.ensure_shadow(h, c->stream); rc) return rc;
	const uint32_t grid_max = std::max(f.gridx, f.gridx_exact);
	const uint32_t cap = f.cap;
	if (int rc = c->d_qpad.ensure(size_t(nq) * f.ld * sizeof(float)); rc) return rc;
	if (f.planes) {
		if (int rc = c->d_qplanes.ensure(size_t(nq) * 2 * f.ld); rc) return rc;
	}
	if (int rc = c->d_qstats.ensure(size_t(f.qstats_floats) * nq * sizeof(float)); rc) return rc;
	const bool keep = !f.emits || c->keep_values;
	if (keep) {
		if (int rc = c->d_dense.ensure(size_t(nq) * f.n * sizeof(float)); rc) return rc;
	}
	if (f.emits) {
		if (int rc = c->d_emit.ensure(emit_buffer_bytes(f.n, nq)); rc) return rc;
		if (int rc = c->d_emit_cnt.ensure(emit_count_bytes(f.gridx, nq)); rc) return rc;
	}
	if (int rc = c->d_part_dist.ensure(size_t(nq) * grid_max * kk * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(nq) * grid_max * kk * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_top.ensure(size_t(nq) * (2 * kk + 1) * sizeof(uint32_t)); rc) return rc;
	if (f.seed) {
		if (int rc = c->d_seed.ensure(size_t(nq) * (2 * kk + 1) * sizeof(uint32_t)); rc) return rc;
	}
	if (int rc = c->d_cand_row.ensure(size_t(nq) * cap * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_dist.ensure(size_t(nq) * cap * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
	PrunedBufs b{};
	b.qpad = static_cast<float*>(c->d_qpad.ptr);
	b.qstats = static_cast<float*>(c->d_qstats.ptr);
	b.q_sq = b.qstats + size_t(f.qstats_floats - 2) * nq;
	b.margin = b.q_sq + nq;
	b.values = static_cast<float*>(c->d_dense.ptr);
	b.cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	b.cap = cap;
	b.emit = static_cast<EmitEntry*>(c->d_emit.ptr);
	b.emit_cnt = static_cast<uint32_t*>(c->d_emit_cnt.ptr);
	b.keep = keep;
	float* top_dist = static_cast<float*>(c->d_top.ptr);
	uint32_t* top_row = reinterpret_cast<uint32_t*>(top_dist + size_t(nq) * kk);
	uint32_t* top_cnt = top_row + size_t(nq) * kk;
	uint32_t* cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
	float* cand_dist = static_cast<float*>(c->d_cand_dist.ptr);
	c->pruned_cap = cap;
	c->pruned_n = f.n;
	c->pruned_kk = kk;
	c->pruned_ld = f.ld;
	c->pruned_i8 = f.planes;
	c->pruned_i6 = f.seed != nullptr;
	c->pruned_emit_gridx = f.emits ? f.gridx : 0;
	f.prep(h, c, d_queries, nq, f, b);
	const ScanParams e = scan_params(h, c, d_queries, f.n, kk, b.cand_cnt, cap);   // the exact scan behind the gate
	if (f.seed) {
		ProfileScope ps(h, f.seed_slot, c->stream);
		f.seed(h, c, nq, scan_params(h, c, nullptr, f.n, kk), f, b);
	}
	{
		ProfileScope ps(h, f.scan_slot, c->stream);
		f.scan(h, c, nq, scan_params(h, c, nullptr, f.n, kk), f, b);
	}
	// (the scan leaves sorted lists like the f32 scan: the list merge, 4 us against 28 for the insertion merge in the kernel trace of the headline)
	launch_merge_lists(e.part_dist, e.part_row, f.gridx, kk, nq, top_dist, top_row, top_cnt, c->stream);
	{
		ProfileScope ps(h, "filter_approx", c->stream);
		if (f.emits && f.many_candidates) {
			launch_filter_emitted_wide(b.emit, b.emit_cnt, emit_plan(f.n, f.gridx), top_dist, top_cnt, kk, b.margin, cand_row, b.cand_cnt, cap, nq, h->cus, c->stream);
		} else if (f.emits) {
			launch_filter_emitted(b.emit, b.emit_cnt, emit_plan(f.n, f.gridx), top_dist, top_cnt, kk, b.margin, cand_row, b.cand_cnt, cap, nq, h->cus, c->stream);
		} else {
			launch_filter_approx(b.values, f.n, top_dist, top_cnt, kk, b.margin, cand_row, b.cand_cnt, cap, nq, h->cus, c->stream, f.ids);
		}
	}
	{
		ProfileScope ps(h, "rescore", c->stream);
		launch_rescore(h->metric, h->d_rows, h->d_inv_norms, b.qpad, f.ld, h->stride, h->dim, nq, cap, b.cand_cnt, cand_row, cand_dist, c->stream);
	}
	{   // more rows inside the bound than the list holds (massive ties), or no finite bound: the f32 path's own scan, gated on device
		bool file_slot = !f.fallback_slot_when_opened;
		if (f.fallback_slot_when_opened && h->profiling) {
			std::vector<uint32_t> cnt(nq);
			RX_HIP(hipMemcpyAsync(cnt.data(), b.cand_cnt, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
			RX_HIP(hipStreamSynchronize(c->stream));
			file_slot = std::any_of(cnt.begin(), cnt.end(), [&](uint32_t v) { return v > cap; });
		}
		auto fallback = [&] {
			if (f.ids) {
				launch_scan_subset(h->metric, e, f.ids, nq, f.gridx_exact, h->cus, c->stream);
			} else {
				launch_scan(h->metric, e, nq, f.gridx_exact, c->stream);
			}
		};
		if (file_slot) {
			ProfileScope ps(h, "fallback_scan", c->stream);
			fallback();
		} else {
			fallback();
		}
	}
	// one merge: the re-scored candidates of a query the pruned chain answers, the exact scan's lists of a query whose gate opened
	launch_merge_final(cand_dist, cand_row, b.cand_cnt, cap, e.part_dist, e.part_row, f.gridx_exact, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream);
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// The bf16 tier: knn_query_prep and knn_scan_bf16 in front, approximate distances per row.
int enqueue_knn_pruned(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist,
					   uint32_t* d_out_row, uint32_t* d_out_count) {
	PrunedFront f{};
	f.ensure_shadow = [](rxgpu_index* h, hipStream_t s) {
		if (int rc = ensure_row_stats(h, s); rc) return rc;
		return ensure_bf16_shadow(h, s);
	};
	f.ld = (h->dim + 63u) & ~63u;
	f.qstats_floats = 2;
	f.n = h->count;
	f.cap = pruned_cap(f.n);
	f.gridx = scan_bf16_grid_x(h->count, h->cus);
	f.gridx_exact = scan_grid_x(h->count, h->cus);
	f.scan_slot = "scan_bf16";
	f.prep = [](rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, const PrunedFront& f, const PrunedBufs& b) {
		launch_query_prep(h->metric, d_queries, nq, h->dim, b.qpad, f.ld, h->d_stats, b.q_sq, b.margin, b.cand_cnt, b.cap, c->stream);
	};
	f.scan = [](rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b) {
		ScanBf16Params p{};
		p.sp = sp;
		p.rows16 = h->d_rows_bf16;
		p.blocked = h->bf16_blocked ? 1u : 0u;
		p.queries32 = b.qpad;
		p.row_sq = h->d_row_sq;
		p.q_sq = b.q_sq;
		p.ld = f.ld;
		p.approx = b.values;
		launch_scan_bf16(h->metric, p, nq, f.gridx, c->stream);
	};
	return enqueue_knn_pruned_chain(h, c, d_queries, nq, kk, f, d_out_dist, d_out_row, d_out_count);
}

// The int8 tier: knn_query_prep_i8 and knn_scan_i8 in front, per-row LOWER bounds where the bf16 chain keeps approximate distances.  Over
// a row list (d_ids): the gather form of the scan.  Lower bounds are then kept per LIST POSITION ([nq][n_ids]); the candidate filter maps
// position -> row, so the re-score and the merges see real rows.  The margin comes from index-wide maxima and is therefore sound for any
// subset of the rows.  Behind the gate of that form: the f32 subset scan, which is what answers the call off the tier.
int enqueue_knn_pruned_i8(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
						  uint64_t n_ids, float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	PrunedFront f{};
	f.ensure_shadow = ensure_i8_shadow;   // (the row statistics first)
	f.ld = i8_ld(h->dim);
	f.qstats_floats = 4;   // [nq] {s_q, |q|} pairs, then [nq] |q|^2, [nq] margins
	f.planes = true;
	f.n = d_ids ? n_ids : h->count;
	f.ids = d_ids;
	f.cap = pruned_cap(f.n);
	f.emits = !d_ids && scan_i8_emits();   // (the gather form keeps a value per list position)
	f.gridx = d_ids ? scan_i8_subset_grid_x(n_ids, h->cus) : scan_i8_grid_x(h->count, h->cus);
	f.gridx_exact = d_ids ? subset_grid_x(n_ids, h->dim, kk, h->cus) : scan_grid_x(h->count, h->cus);
	f.scan_slot = d_ids ? "scan_i8_subset" : "scan_i8";
	f.fallback_slot_when_opened = d_ids != nullptr;
	f.prep = [](rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, const PrunedFront& f, const PrunedBufs& b) {
		launch_query_prep_i8(h->metric, d_queries, nq, h->dim, b.qpad, static_cast<int8_t*>(c->d_qplanes.ptr), f.ld, h->d_stats, b.q_sq, b.margin,
							 reinterpret_cast<float2*>(b.qstats), b.cand_cnt, b.cap, c->stream);
	};
	f.scan = [](rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b) {
		ScanI8Params p{};
		p.sp = sp;
		p.codes = h->d_codes_i8;
		p.side = h->d_side_i8;
		p.planes = static_cast<const int8_t*>(c->d_qplanes.ptr);
		p.qinfo = reinterpret_cast<const float2*>(b.qstats);
		p.row_sq = h->d_row_sq;
		p.q_sq = b.q_sq;
		p.ld8 = f.ld;
		p.lower = b.values;
		if (f.ids) {
			launch_scan_i8_subset(h->metric, p, f.ids, nq, f.gridx, h->cus, c->stream);
		} else if (f.emits) {
			ScanI8Emit e{};
			e.margin = b.margin;
			e.emit = b.emit;
			e.emit_cnt = b.emit_cnt;
			e.plan = emit_plan(f.n, f.gridx);
			launch_scan_i8(h->metric, p, nq, f.gridx, c->stream, &e, b.keep);
		} else {
			launch_scan_i8(h->metric, p, nq, f.gridx, c->stream);
		}
	};
	return enqueue_knn_pruned_chain(h, c, d_queries, nq, kk, f, d_out_dist, d_out_row, d_out_count);
}

// The 6-bit front of the int8 tier (knn_scan_i6.hip; whole index only): the int8 prep with the 6-bit residual maxima, a seed pass over a strided
// sample whose merged list gives the scan a tight emission threshold from its first row, and the emitting scan.  The per-row window is four
// times the int8 one, so the filter leaves thousands of candidates where the int8 front leaves tens: the list holds
// kPrunedCapI6.  RXGPU_SCAN_I6_CAP lowers it (tests of the overflow gate).
constexpr uint32_t kPrunedCapI6 = 65536;
ScanI6Params scan_i6_params(rxgpu_index* h, rxgpu_search_ctx* c, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b) {
	ScanI6Params p{};
	p.sp = sp;
	p.codes = h->d_codes_i6;
	p.side = h->d_side_i6;
	p.planes = static_cast<const int8_t*>(c->d_qplanes.ptr);
	p.qinfo = reinterpret_cast<const float2*>(b.qstats);
	p.row_sq = h->d_row_sq;
	p.q_sq = b.q_sq;
	p.ld6 = f.ld;
	p.set_step = 1;
	p.lower = b.values;
	return p;
}
int enqueue_knn_pruned_i6(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist, uint32_t* d_out_row,
						  uint32_t* d_out_count) {
	PrunedFront f{};
	f.ensure_shadow = ensure_i6_shadow;   // (the row statistics first)
	f.ld = i6_ld(h->dim);
	f.qstats_floats = 4;   // as the int8 front
	f.planes = true;
	f.n = h->count;
	f.cap = pruned_cap(f.n, kPrunedCapI6);
	if (const char* e = getenv("RXGPU_SCAN_I6_CAP"); e && *e) f.cap = std::min(f.cap, pruned_cap(f.n, uint32_t(std::max(64, atoi(e)) + 63) & ~63u));
	f.emits = true;
	f.many_candidates = true;
	f.gridx = scan_i6_grid_x(h->count, 1, h->cus);
	f.gridx_exact = scan_grid_x(h->count, h->cus);
	f.scan_slot = "scan_i6";
	f.seed_slot = "seed_i6";
	f.prep = [](rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, const PrunedFront& f, const PrunedBufs& b) {
		launch_query_prep_i8(h->metric, d_queries, nq, h->dim, b.qpad, static_cast<int8_t*>(c->d_qplanes.ptr), f.ld, h->d_stats, b.q_sq, b.margin,
							 reinterpret_cast<float2*>(b.qstats), b.cand_cnt, b.cap, c->stream, h->d_stats_i6);
	};
	f.seed = [](rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b) {
		ScanI6Params p = scan_i6_params(h, c, sp, f, b);
		p.set_step = scan_i6_seed_step(f.n);
		const uint32_t gridx = scan_i6_grid_x(f.n, p.set_step, h->cus);   // (<= f.gridx: the part buffers hold it)
		launch_scan_i6(h->metric, p, nq, gridx, c->stream, nullptr, false);
		float* seed_dist = static_cast<float*>(c->d_seed.ptr);
		uint32_t* seed_row = reinterpret_cast<uint32_t*>(seed_dist + size_t(nq) * sp.kk);
		launch_merge_lists(sp.part_dist, sp.part_row, gridx, sp.kk, nq, seed_dist, seed_row, seed_row + size_t(nq) * sp.kk, c->stream);
	};
	f.scan = [](rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, const ScanParams& sp, const PrunedFront& f, const PrunedBufs& b) {
		ScanI6Params p = scan_i6_params(h, c, sp, f, b);
		p.seed_dist = static_cast<const float*>(c->d_seed.ptr);
		p.seed_cnt = reinterpret_cast<const uint32_t*>(p.seed_dist + 2 * size_t(nq) * sp.kk);
		ScanI8Emit e{};
		e.margin = b.margin;
		e.emit = b.emit;
		e.emit_cnt = b.emit_cnt;
		e.plan = emit_plan(f.n, f.gridx);
		launch_scan_i6(h->metric, p, nq, f.gridx, c->stream, &e, b.keep);
	};
	return enqueue_knn_pruned_chain(h, c, d_queries, nq, kk, f, d_out_dist, d_out_row, d_out_count);
}

}  // namespace

// Range search from the int8 shadow (declared in rxgpu_internal.h; the entry points and the f32 kernel behind it: rxgpu_knn_search.hip).  The
// candidate list is sized from the caller's cap, never from a guess about the hits: min(n, max(kPrunedCap, 2 min(cap, n))), so a call whose
// hits fit the caller's buffer fits the list too unless the boundary zone holds as many rows again as the buffer.
int enqueue_range_pruned_i8(rxgpu_index* h, rxgpu_search_ctx* c, const uint32_t* d_ids, uint64_t n, float radius, int inclusive, uint64_t cap, uint64_t dcap,
							uint32_t* ccap_out) {
	if (int rc = ensure_i8_shadow(h, c->stream); rc) return rc;
	const uint32_t ccap = uint32_t(std::min<uint64_t>(n, std::max<uint64_t>(kPrunedCap, 2 * std::min<uint64_t>(cap, n))));
	const uint32_t ld = i8_ld(h->dim);
	if (int rc = c->d_qpad.ensure(size_t(ld) * sizeof(float)); rc) return rc;
	if (int rc = c->d_qplanes.ensure(size_t(2) * ld); rc) return rc;
	if (int rc = c->d_qstats.ensure(4 * sizeof(float)); rc) return rc;
	if (int rc = c->d_cand_row.ensure(size_t(ccap) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_cand_cnt.ensure(sizeof(uint32_t)); rc) return rc;
	float* qstats = static_cast<float*>(c->d_qstats.ptr);   // {s_q, |q|^}, |q|^2, margin: the layout of the KNN chain's front
	float* q_sq = qstats + 2;
	float* margin = qstats + 3;
	uint32_t* cand_cnt = static_cast<uint32_t*>(c->d_cand_cnt.ptr);
	uint32_t* cand_row = static_cast<uint32_t*>(c->d_cand_row.ptr);
	const float* query = static_cast<const float*>(c->d_queries.ptr);
	launch_query_prep_i8(h->metric, query, 1, h->dim, static_cast<float*>(c->d_qpad.ptr), static_cast<int8_t*>(c->d_qplanes.ptr), ld, h->d_stats, q_sq, margin,
						 reinterpret_cast<float2*>(qstats), cand_cnt, ccap, c->stream);
	{
		ProfileScope ps(h, d_ids ? "range_i8_subset" : "range_i8", c->stream);
		ScanI8Params p{};
		p.sp.inv_norms = h->d_inv_norms;
		p.sp.n = n;
		p.codes = h->d_codes_i8;
		p.side = h->d_side_i8;
		p.planes = static_cast<const int8_t*>(c->d_qplanes.ptr);
		p.qinfo = reinterpret_cast<const float2*>(qstats);
		p.row_sq = h->d_row_sq;
		p.q_sq = q_sq;
		p.ld8 = ld;
		RangeI8Cand rc{};
		rc.radius = radius;
		rc.margin = margin;
		rc.cand_cnt = cand_cnt;
		rc.cand_row = cand_row;
		rc.ccap = ccap;
		launch_range_i8(h->metric, p, rc, d_ids, h->cus, c->stream);
	}
	{
		ProfileScope ps(h, "range_rescore", c->stream);
		launch_range_rescore(h->metric, h->d_rows, h->d_inv_norms, query, cand_cnt, cand_row, ccap, h->stride, h->dim, radius, inclusive,
							 static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr), dcap,
							 static_cast<unsigned long long*>(c->d_out_count.ptr), scan_grid_x(ccap, h->cus), c->stream);
	}
	RX_HIP(hipGetLastError());
	*ccap_out = ccap;
	return RXGPU_OK;
}

// Pre-filtered search, kk <= kMaxFusedK2: gather-scan over the row list + the usual merge (rows in the lists are real rows, so the
// merge and everything downstream is unchanged).  Where scan_policy_tier_subset says so, the int8-pruned chain above answers instead.
int enqueue_knn_subset(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
					   uint64_t n_ids, float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count) {
	// (the device entry point may pass kk > n_ids; the chain runs with kk itself, so a kk above one entry per lane stays off the tier whatever the list)
	const uint32_t eff = kk <= uint32_t(kMaxFusedK) ? uint32_t(std::min<uint64_t>(kk, n_ids)) : kk;
	if (scan_policy_tier_subset(n_ids, h->dim, nq, eff, !h->i8_unavailable, true) == kTierI8) {
		if (int rc = ensure_row_stats(h, c->stream); rc) return rc;   // (automatic mode asks whether the row statistics are finite)
		if (scan_policy_tier_subset(n_ids, h->dim, nq, eff, !h->i8_unavailable, h->stats_finite) == kTierI8) {
			const int rc = enqueue_knn_pruned_i8(h, c, d_queries, nq, kk, d_ids, n_ids, d_out_dist, d_out_row, d_out_count);
			if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) return rc;   // no room for the int8 shadow: the f32 subset scan below
		}
	}
	const uint32_t gridx = subset_grid_x(n_ids, h->dim, kk, h->cus);
	const size_t part = size_t(nq) * gridx * kk;
	if (int rc = c->d_part_dist.ensure(part * sizeof(float)); rc) return rc;
	if (int rc = c->d_part_row.ensure(part * sizeof(uint32_t)); rc) return rc;
	const ScanParams p = scan_params(h, c, d_queries, n_ids, kk);
	{
		ProfileScope ps(h, "scan_subset", c->stream);
		launch_scan_subset(h->metric, p, d_ids, nq, gridx, h->cus, c->stream);
	}
	{
		ProfileScope ps(h, "merge", c->stream);
		launch_merge_lists(p.part_dist, p.part_row, gridx, kk, nq, d_out_dist, d_out_row, d_out_count, c->stream);
	}
	RX_HIP(hipGetLastError());
	return RXGPU_OK;
}

// The result of an enqueue_knn* call ([nq][eff] in c->d_out_*) into the caller's [nq][kk] arrays: copies, the wait for the stream, and
// while profiling what the pruned chain of a single query nominated (rxgpu_index_last_candidates).
int copy_back_knn(rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, uint32_t kk, uint32_t eff, float* out_dist, uint32_t* out_row,
				  uint32_t* out_count) {
	if (eff == kk) {
		RX_HIP(hipMemcpyAsync(out_dist, c->d_out_dist.ptr, size_t(nq) * eff * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(out_row, c->d_out_row.ptr, size_t(nq) * eff * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	} else {
		RX_HIP(hipMemcpy2DAsync(out_dist, kk * sizeof(float), c->d_out_dist.ptr, eff * sizeof(float), eff * sizeof(float), nq, hipMemcpyDeviceToHost,
								c->stream));
		RX_HIP(hipMemcpy2DAsync(out_row, kk * sizeof(uint32_t), c->d_out_row.ptr, eff * sizeof(uint32_t), eff * sizeof(uint32_t), nq,
								hipMemcpyDeviceToHost, c->stream));
	}
	RX_HIP(hipMemcpyAsync(out_count, c->d_out_count.ptr, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	const bool kept = c->keep_values;
	c->keep_values = false;
	if (h->profiling && nq == 1 && c->pruned_cap && (kept || !c->pruned_emit_gridx)) {
		uint32_t cnt = 0;
		RX_HIP(hipMemcpy(&cnt, c->d_cand_cnt.ptr, sizeof(cnt), hipMemcpyDeviceToHost));
		h->last_cand_count = cnt;
		h->last_cand_cap = c->pruned_cap;
		// rxgpu_index_inspect reads the chain's buffers out of this context later.  The exact scan behind the gate writes the part buffers
		// and the result only (launch_scan / launch_scan_subset, launch_merge_final), never d_dense, d_emit, d_emit_cnt, d_top, d_qstats, d_qplanes or d_cand_row.
		std::lock_guard<std::mutex> lk(h->mtx);
		h->last_pruned_ctx = c;
		h->last_pruned_n = c->pruned_n;
		h->last_pruned_kk = c->pruned_kk;
		h->last_pruned_ld = c->pruned_ld;
		h->last_pruned_i8 = c->pruned_i8;
		h->last_pruned_i6 = c->pruned_i6;
		h->last_pruned_emit_gridx = c->pruned_emit_gridx;
	} else if (h->profiling) {   // another chain answered: whatever context it ran in may be the recorded one
		std::lock_guard<std::mutex> lk(h->mtx);
		h->last_pruned_ctx = nullptr;
	}
	return RXGPU_OK;
}

// The selected entries of a large k, or the hits of a range call (any order), sorted by (dist, row) into the caller's arrays: the one
// comparator of every host-side sort, dist_row_less — a strict weak order with NaN distances too (they sort last).
void sort_dist_row(const std::vector<float>& hd, const std::vector<uint32_t>& hr, float* out_dist, uint32_t* out_row) {
	std::vector<std::pair<float, uint32_t>> all(hd.size());
	for (size_t i = 0; i < all.size(); ++i) all[i] = {hd[i], hr[i]};
	std::sort(all.begin(), all.end(), dist_row_less);
	for (size_t i = 0; i < all.size(); ++i) {
		out_dist[i] = all[i].first;
		out_row[i] = all[i].second;
	}
}

// Host-facing tail shared by rxgpu_search_knn_subset / _bitmap / _lists: queries on the host, the row list already in HBM.
int search_subset_host(rxgpu_index* h, rxgpu_search_ctx* c, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids,
					   uint64_t n_ids, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	const uint32_t eff = uint32_t(std::min<uint64_t>(kk, n_ids));
	const size_t qbytes = size_t(nq) * h->dim * sizeof(float);
	if (int rc = c->d_queries.ensure(qbytes); rc) return rc;
	RX_HIP(hipMemcpyAsync(c->d_queries.ptr, queries, qbytes, hipMemcpyHostToDevice, c->stream));
	if (eff <= uint32_t(kMaxFusedK2)) {
		if (int rc = c->d_out_dist.ensure(size_t(nq) * eff * sizeof(float)); rc) return rc;
		if (int rc = c->d_out_row.ensure(size_t(nq) * eff * sizeof(uint32_t)); rc) return rc;
		if (int rc = c->d_out_count.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
		c->pruned_cap = 0;   // set by a pruned chain
		c->keep_values = h->profiling && nq == 1;   // what copy_back_knn records (it clears the flag)
		if (int rc = enqueue_knn_subset(h, c, static_cast<const float*>(c->d_queries.ptr), nq, eff, d_ids, n_ids,
										static_cast<float*>(c->d_out_dist.ptr), static_cast<uint32_t*>(c->d_out_row.ptr),
										static_cast<uint32_t*>(c->d_out_count.ptr));
			rc) {
			c->keep_values = false;
			return rc;
		}
		return copy_back_knn(h, c, nq, kk, eff, out_dist, out_row, out_count);
	}
	// large k: distances of the listed rows + radix select over (dist, position); positions -> rows; final sort of eff entries on the host
	RX_CHECK(n_ids <= (1ull << 28), RXGPU_ERR_PARAMS, "pre-filtered search with k > 128: the row list must not exceed 2^28 entries");
	if (int rc = c->d_misc.ensure(n_ids * sizeof(float)); rc) return rc;
	if (int rc = c->d_select.ensure(select_scratch_bytes(n_ids)); rc) return rc;
	if (int rc = c->d_out_dist.ensure(size_t(eff) * sizeof(float)); rc) return rc;
	if (int rc = c->d_out_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	if (int rc = c->d_part_row.ensure(size_t(eff) * sizeof(uint32_t)); rc) return rc;
	std::vector<float> hd(eff);
	std::vector<uint32_t> hr(eff);
	for (uint32_t q = 0; q < nq; ++q) {
		{
			ProfileScope ps(h, "scan_subset", c->stream);
			launch_distances(h->metric, h->d_rows, h->d_inv_norms, static_cast<const float*>(c->d_queries.ptr) + size_t(q) * h->dim, h->stride, h->dim,
							 d_ids, uint32_t(n_ids), static_cast<float*>(c->d_misc.ptr), c->stream);
		}
		launch_select_smallest(static_cast<const float*>(c->d_misc.ptr), n_ids, eff, c->d_select.ptr, static_cast<float*>(c->d_out_dist.ptr),
							   static_cast<uint32_t*>(c->d_out_row.ptr), c->stream);
		launch_gather_u32(d_ids, static_cast<const uint32_t*>(c->d_out_row.ptr), eff, static_cast<uint32_t*>(c->d_part_row.ptr), c->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpyAsync(hd.data(), c->d_out_dist.ptr, size_t(eff) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(hr.data(), c->d_part_row.ptr, size_t(eff) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
		sort_dist_row(hd, hr, out_dist + size_t(q) * kk, out_row + size_t(q) * kk);
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
	if (scan_policy_i6(h->count, h->dim, nq, !h->i6_unavailable, true) && h->count) {
		if (int rc = ensure_row_stats(h, c->stream); rc) return rc;
		if (scan_policy_i6(h->count, h->dim, nq, !h->i6_unavailable, h->stats_finite)) {
			int rc = enqueue_knn_pruned_i6(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
			if (!(rc == RXGPU_ERR_NOMEM && h->i6_unavailable)) return rc;
			// no room for the 6-bit shadow: the int8 front (which the forced mode takes at any size, like RXGPU_SCAN_I8=1), then the tiers below
			if (!h->i8_unavailable) {
				rc = enqueue_knn_pruned_i8(h, c, d_queries, nq, kk, nullptr, 0, d_out_dist, d_out_row, d_out_count);
				if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) return rc;
			}
		}
	}
	if (scan_policy_tier(h->count, h->dim, nq, !h->bf16_unavailable, !h->i8_unavailable, h->stats_finite) == kTierI8) {
		const int rc = enqueue_knn_pruned_i8(h, c, d_queries, nq, kk, nullptr, 0, d_out_dist, d_out_row, d_out_count);
		if (!(rc == RXGPU_ERR_NOMEM && h->i8_unavailable)) return rc;   // no room for the int8 shadow: the bf16 tier below
	}
	if (scan_policy_tier(h->count, h->dim, nq, !h->bf16_unavailable, !h->i8_unavailable, h->stats_finite) == kTierBf16) {
		const int rc = enqueue_knn_pruned(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
		if (!(rc == RXGPU_ERR_NOMEM && h->bf16_unavailable)) return rc;
	}
	if (int(nq) >= batch_min_queries() && nq >= 2) return enqueue_knn_batched(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
	return enqueue_knn_fused(h, c, d_queries, nq, kk, d_out_dist, d_out_row, d_out_count);
}

}  // namespace rxgpu
