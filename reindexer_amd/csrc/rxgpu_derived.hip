// Data derived from the rows of an index: the row statistics, the bf16 shadow, the int8 shadow and the 6-bit shadow.  Built lazily by the search chains
// (ensure_*), kept in step by the mutations of rxgpu_capi.hip through the derived_* calls below.  Host-side plumbing only.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/rxgpu.h"
#include "knn_i6_quant.h"
#include "knn_i8_quant.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {
namespace {

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

uint32_t bf16_ld(const rxgpu_index* h) { return (h->dim + 63u) & ~63u; }

}  // namespace

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
	launch_row_stats(h->d_rows, h->d_inv_norms, h->count, h->stride, h->dim, h->metric == RXGPU_METRIC_L2 ? h->d_row_sq : nullptr, h->d_stats, h->cus, s);
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
	const uint32_t ld = bf16_ld(h);
	const uint64_t need = (std::max<uint64_t>(h->capacity, h->count) + kShadowTileRows - 1) / kShadowTileRows * kShadowTileRows;   // whole tiles
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
	launch_to_bf16(h->d_rows, h->count, h->stride, h->dim, h->d_rows_bf16, ld, h->cus, s, 0, h->bf16_blocked);
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
	const uint32_t ld8 = i8_ld(h->dim);
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
	launch_i8_build(h->d_rows, h->d_inv_norms, h->count, h->stride, h->dim, h->d_codes_i8, h->d_side_i8, ld8, h->d_stats, h->cus, s);
	RX_HIP(hipGetLastError());
	if (int rc = read_stats_finite(h, s); rc) return rc;   // synchronises the stream
	h->i8_valid = true;
	return RXGPU_OK;
}

// 6-bit shadow of the rows for the 6-bit front of the int8-pruned chain (knn_scan_i6.hip): 0.75 bytes per element + 8 bytes per row, in tiles of
// four rows (knn_i6_quant.h); its residual maxima have three words of their own (kStatsI6Words), so the int8 words keep their meaning.  Built
// lazily behind the row statistics and kept in step by the mutations like the int8 shadow.  A fresh allocation is zeroed: the rows past the
// end of the index in the last tile are zero.
constexpr size_t kStatsI6Words = 3;
int ensure_i6_shadow(rxgpu_index* h, hipStream_t s) {
	if (int rc = ensure_row_stats(h, s); rc) return rc;
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->i6_valid) return RXGPU_OK;
	const uint32_t ld6 = i6_ld(h->dim);
	const uint64_t need = std::max<uint64_t>(h->capacity, h->count);
	if (h->i6_capacity < need) {
		if (h->d_codes_i6) (void)hipFree(h->d_codes_i6);
		if (h->d_side_i6) (void)hipFree(h->d_side_i6);
		h->d_codes_i6 = nullptr;
		h->d_side_i6 = nullptr;
		h->i6_capacity = 0;
		if (hipMalloc(reinterpret_cast<void**>(&h->d_codes_i6), i6_shadow_bytes(need, ld6)) != hipSuccess ||
			hipMalloc(reinterpret_cast<void**>(&h->d_side_i6), need * sizeof(float2)) != hipSuccess) {
			(void)hipGetLastError();   // not an error of the search: the caller takes the int8 front
			if (h->d_codes_i6) (void)hipFree(h->d_codes_i6);
			h->d_codes_i6 = nullptr;
			h->d_side_i6 = nullptr;
			h->i6_unavailable = true;
			return RXGPU_ERR_NOMEM;
		}
		h->i6_capacity = need;
		RX_HIP(hipMemsetAsync(h->d_codes_i6, 0, i6_shadow_bytes(need, ld6), s));
	}
	if (!h->d_stats_i6) RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_stats_i6), kStatsI6Words * sizeof(unsigned int)));
	RX_HIP(hipMemsetAsync(h->d_stats_i6, 0, kStatsI6Words * sizeof(unsigned int), s));
	launch_i6_build(h->d_rows, h->d_inv_norms, 0, h->count, h->stride, h->dim, h->d_codes_i6, h->d_side_i6, ld6, h->d_stats_i6, h->cus, s);
	for (uint64_t row = h->count; row < i6_tiles(h->count) * kI6TileRows; ++row) launch_i6_copy_row(h->d_codes_i6, ld6, ~0ull, row, s);   // (a rebuild over a longer one)
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(s));
	h->i6_valid = true;
	return RXGPU_OK;
}

void derived_invalidate(rxgpu_index* h) {
	h->stats_valid = false;
	h->bf16_valid = false;
	h->i8_valid = false;
	h->i6_valid = false;
}

// The index shrinks to `count` rows: the shadows keep their rows (those past the end are never read); the 6-bit shadow's last tile goes back
// to zero past the end, as a fresh build leaves it.
int derived_follow_truncate(rxgpu_index* h, uint64_t count) {
	std::lock_guard<std::mutex> lk(h->mtx);
	if (!h->i6_valid) return RXGPU_OK;
	const uint64_t end = std::min<uint64_t>(i6_tiles(count) * kI6TileRows, h->i6_capacity);
	for (uint64_t row = count; row < end; ++row) launch_i6_copy_row(h->d_codes_i6, i6_ld(h->dim), ~0ull, row, nullptr);
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(nullptr));
	return RXGPU_OK;
}

// Derived data follows the mutation incrementally (a full recompute streams the whole corpus: 4 ms per 10M x 768 rows).  The row
// statistics are maxima entering an error BOUND, so folding the new rows in (and never shrinking on deletes) keeps them valid.
int derived_follow_upload(rxgpu_index* h, uint64_t first_row, uint64_t n) {
	const float* rows = h->d_rows + first_row * h->stride;
	const float* inv_norms = h->d_inv_norms ? h->d_inv_norms + first_row : nullptr;
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->stats_valid) {
		if (h->metric == RXGPU_METRIC_L2 && h->row_sq_capacity < first_row + n) {
			h->stats_valid = false;
		} else {
			launch_row_stats(rows, inv_norms, n, h->stride, h->dim, h->metric == RXGPU_METRIC_L2 ? h->d_row_sq + first_row : nullptr, h->d_stats, h->cus,
							 nullptr);
			if (int rc = read_stats_finite(h, nullptr); rc) return rc;   // maxima never shrink: an index that has held a non-finite row stays on the f32 scan
		}
	}
	if (h->bf16_valid) {
		if (h->bf16_capacity < first_row + n) {
			h->bf16_valid = false;
		} else {
			launch_to_bf16(rows, n, h->stride, h->dim, h->d_rows_bf16, bf16_ld(h), h->cus, nullptr, first_row, h->bf16_blocked);
		}
	}
	if (h->i8_valid) {
		if (h->i8_capacity < first_row + n || !h->stats_valid) {
			h->i8_valid = false;
		} else {   // re-quantise the range; its residual maxima join the statistics words
			const uint32_t ld8 = i8_ld(h->dim);
			launch_i8_build(rows, inv_norms, n, h->stride, h->dim, h->d_codes_i8 + first_row * ld8, h->d_side_i8 + first_row, ld8, h->d_stats, h->cus, nullptr);
			if (int rc = read_stats_finite(h, nullptr); rc) return rc;
		}
	}
	if (h->i6_valid) {
		if (h->i6_capacity < first_row + n || !h->stats_valid) {
			h->i6_valid = false;
		} else {   // re-quantise the range; its residual maxima join the shadow's own statistics words
			launch_i6_build(h->d_rows, h->d_inv_norms, first_row, n, h->stride, h->dim, h->d_codes_i6, h->d_side_i6, i6_ld(h->dim), h->d_stats_i6, h->cus, nullptr);
		}
	}
	RX_HIP(hipGetLastError());
	RX_HIP(hipStreamSynchronize(nullptr));
	return RXGPU_OK;
}

int derived_follow_move(rxgpu_index* h, uint64_t from, uint64_t to) {
	std::lock_guard<std::mutex> lk(h->mtx);
	if (h->stats_valid && h->metric == RXGPU_METRIC_L2) {
		RX_HIP(hipMemcpy(h->d_row_sq + to, h->d_row_sq + from, sizeof(float), hipMemcpyDeviceToDevice));
	}
	if (h->bf16_valid) {
		launch_shadow_move(h->d_rows_bf16, bf16_ld(h), from, to, h->bf16_blocked, nullptr);
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(nullptr));
	}
	if (h->i8_valid) {
		const uint32_t ld8 = i8_ld(h->dim);
		RX_HIP(hipMemcpy(h->d_codes_i8 + to * ld8, h->d_codes_i8 + from * ld8, ld8, hipMemcpyDeviceToDevice));
		RX_HIP(hipMemcpy(h->d_side_i8 + to, h->d_side_i8 + from, sizeof(float2), hipMemcpyDeviceToDevice));
	}
	if (h->i6_valid) {   // (a row's bytes inside its tile are its own)
		launch_i6_copy_row(h->d_codes_i6, i6_ld(h->dim), from, to, nullptr);
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpy(h->d_side_i6 + to, h->d_side_i6 + from, sizeof(float2), hipMemcpyDeviceToDevice));
	}
	return RXGPU_OK;
}

// rxgpu_index_inspect: a named internal buffer copied to the host, for tests.  Reads only: nothing is built, invalidated or changed, so a
// buffer that was never built (or is stale) is RXGPU_ERR_LOGIC.  The index-level names cover the `count` rows the index holds; the
// pruned_* names are the buffers of the context the last recorded pruned call ran in (copy_back_knn), as that chain left them.
int inspect_index(rxgpu_index* h, const char* what, void* out, uint64_t cap_bytes, uint64_t* out_bytes) {
	const std::string name(what);
	std::lock_guard<std::mutex> lk(h->mtx);
	// pieces [device pointer, bytes] of the answer, in order
	struct Piece {
		const void* src;
		uint64_t bytes;
	};
	std::vector<Piece> pieces;
	bool deblock = false, detile = false;
	auto missing = [&](const char* why) {
		set_error(std::string("rxgpu_index_inspect: ") + what + ": " + why);
		return RXGPU_ERR_LOGIC;
	};
	const uint64_t n = h->count;
	if (name == "stats") {
		if (!h->stats_valid || !h->d_stats) return missing("the row statistics are not built");
		pieces.push_back({h->d_stats, kStatsWords * sizeof(unsigned int)});
	} else if (name == "row_sq") {
		if (h->metric != RXGPU_METRIC_L2 || !h->stats_valid || !h->d_row_sq) return missing("no |x|^2 per row (L2 with row statistics only)");
		pieces.push_back({h->d_row_sq, n * sizeof(float)});
	} else if (name == "codes_i8" || name == "side_i8") {
		if (!h->i8_valid) return missing("the int8 shadow is not built");
		if (name == "codes_i8") {
			pieces.push_back({h->d_codes_i8, n * i8_ld(h->dim)});
		} else {
			pieces.push_back({h->d_side_i8, n * sizeof(float2)});
		}
	} else if (name == "codes_i6" || name == "side_i6" || name == "stats_i6") {
		if (!h->i6_valid) return missing("the 6-bit shadow is not built");
		if (name == "codes_i6") {   // de-tiled on the host below: [count][ld6] bytes of u
			detile = true;
			pieces.push_back({h->d_codes_i6, n * i6_ld(h->dim)});
		} else if (name == "side_i6") {
			pieces.push_back({h->d_side_i6, n * sizeof(float2)});
		} else {
			pieces.push_back({h->d_stats_i6, kStatsI6Words * sizeof(unsigned int)});
		}
	} else if (name == "rows_bf16") {
		if (!h->bf16_valid) return missing("the bf16 shadow is not built");
		deblock = h->bf16_blocked;
		pieces.push_back({h->d_rows_bf16, n * bf16_ld(h) * sizeof(uint16_t)});
	} else if (name.rfind("pruned_", 0) == 0) {
		const rxgpu_search_ctx* c = h->last_pruned_ctx;
		const uint32_t kk = h->last_pruned_kk;
		const bool i8 = h->last_pruned_i8;
		const float* qstats = c ? static_cast<const float*>(c->d_qstats.ptr) : nullptr;   // one query: [{s_q, |q|^}] |q|^2, margin
		const float* q_sq = qstats ? qstats + (i8 ? 2 : 0) : nullptr;
		const char* known[] = {"pruned_values", "pruned_margin", "pruned_q_sq", "pruned_qinfo", "pruned_qplanes", "pruned_top", "pruned_cand_rows",
								   "pruned_emit_cnt", "pruned_emitted", "pruned_seed"};
		if (std::find_if(std::begin(known), std::end(known), [&](const char* k) { return name == k; }) == std::end(known)) {
			set_error(std::string("rxgpu_index_inspect: unknown buffer ") + what);
			return RXGPU_ERR_PARAMS;
		}
		if (!c) return missing("no pruned single-query call is recorded (profiling on, one query, a pruned chain)");
		if (name == "pruned_values") {
			pieces.push_back({c->d_dense.ptr, h->last_pruned_n * sizeof(float)});
		} else if (name == "pruned_margin") {
			pieces.push_back({q_sq + 1, sizeof(float)});
		} else if (name == "pruned_q_sq") {
			pieces.push_back({q_sq, sizeof(float)});
		} else if (name == "pruned_qinfo") {
			if (!i8) return missing("the bf16 tier keeps no {s_q, |q|^} pair");
			pieces.push_back({qstats, 2 * sizeof(float)});
		} else if (name == "pruned_qplanes") {
			if (!i8) return missing("the bf16 tier keeps no query planes");
			pieces.push_back({c->d_qplanes.ptr, 2ull * h->last_pruned_ld});
		} else if (name == "pruned_emit_cnt" || name == "pruned_emitted") {   // what the emitting int8 scan left (knn_emit_plan.h), one query
			if (!h->last_pruned_emit_gridx) return missing("the recorded call's scan emitted nothing (the bf16 tier, a row list, RXGPU_SCAN_I8_EMIT=0)");
			if (name == "pruned_emit_cnt") {   // [wavefronts of the grid] entries per segment
				pieces.push_back({c->d_emit_cnt.ptr, emit_count_bytes(h->last_pruned_emit_gridx, 1)});
			} else {   // [n] {lo, row} pairs: the segments back to back, each valid up to its count
				pieces.push_back({c->d_emit.ptr, emit_buffer_bytes(h->last_pruned_n, 1)});
			}
		} else if (name == "pruned_seed") {   // d_seed of one query, as "pruned_top": [kk] values and the count of the seed pass's merged list
			if (!h->last_pruned_i6) return missing("the recorded call did not take the 6-bit front");
			const float* seed = static_cast<const float*>(c->d_seed.ptr);
			pieces.push_back({seed, kk * sizeof(float)});
			pieces.push_back({seed + 2 * size_t(kk), sizeof(uint32_t)});
		} else if (name == "pruned_top") {   // d_top of one query: [kk] values, [kk] rows, the count
			const float* top = static_cast<const float*>(c->d_top.ptr);
			pieces.push_back({top, kk * sizeof(float)});
			pieces.push_back({top + 2 * size_t(kk), sizeof(uint32_t)});
		} else {
			pieces.push_back({c->d_cand_row.ptr, uint64_t(std::min(h->last_cand_count.load(), h->last_cand_cap.load())) * sizeof(uint32_t)});
		}
	} else {
		set_error(std::string("rxgpu_index_inspect: unknown buffer ") + what);
		return RXGPU_ERR_PARAMS;
	}
	uint64_t need = 0;
	for (const Piece& p : pieces) need += p.bytes;
	*out_bytes = need;
	if (cap_bytes < need || (need && !out)) {
		set_error(std::string("rxgpu_index_inspect: ") + what + " needs " + std::to_string(need) + " bytes");
		return RXGPU_ERR_OVERFLOW;
	}
	if (!need) return RXGPU_OK;
	if (detile) {   // whole tiles to the host, then row by row (knn_i6_quant.h)
		const uint32_t ld6 = i6_ld(h->dim);
		std::vector<uint8_t> raw(i6_shadow_bytes(n, ld6));
		RX_HIP(hipMemcpy(raw.data(), h->d_codes_i6, raw.size(), hipMemcpyDeviceToHost));
		for (uint64_t r = 0; r < n; ++r) i6_load_row(raw.data(), r, ld6, static_cast<uint8_t*>(out) + r * ld6);
		return RXGPU_OK;
	}
	if (deblock) {   // the tile-blocked shadow ([tile of 256 rows][32-element k-block][row][32]) back to [count][ld]: whole tiles to the host, then a loop
		const uint32_t ld = bf16_ld(h);
		const uint64_t tiles = (n + kShadowTileRows - 1) / kShadowTileRows;
		std::vector<uint16_t> raw(tiles * kShadowTileRows * ld);
		RX_HIP(hipMemcpy(raw.data(), h->d_rows_bf16, raw.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
		uint16_t* dst = static_cast<uint16_t*>(out);
		for (uint64_t r = 0; r < n; ++r) {
			const uint64_t base = shadow_elem_base(r, ld, true);
			for (uint32_t k = 0; k < ld; ++k) dst[r * ld + k] = raw[base + uint64_t(k / 32) * shadow_stage_step(true) + k % 32];
		}
		return RXGPU_OK;
	}
	char* dst = static_cast<char*>(out);
	for (const Piece& p : pieces) {
		RX_HIP(hipMemcpy(dst, p.src, p.bytes, hipMemcpyDeviceToHost));
		dst += p.bytes;
	}
	return RXGPU_OK;
}

void derived_free(rxgpu_index* h) {
	if (h->d_row_sq) (void)hipFree(h->d_row_sq);
	if (h->d_rows_bf16) (void)hipFree(h->d_rows_bf16);
	if (h->d_codes_i8) (void)hipFree(h->d_codes_i8);
	if (h->d_side_i8) (void)hipFree(h->d_side_i8);
	if (h->d_codes_i6) (void)hipFree(h->d_codes_i6);
	if (h->d_side_i6) (void)hipFree(h->d_side_i6);
	if (h->d_stats_i6) (void)hipFree(h->d_stats_i6);
	if (h->d_stats) (void)hipFree(h->d_stats);
}

}  // namespace rxgpu
