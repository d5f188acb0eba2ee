// int8-pruned scan (the default for a single query on a large index whose dimension it serves, see scan_policy_tier in rxgpu_knn_chains.hip;
// RXGPU_SCAN_I8=1 / 0 force it on / off): ONE byte per element from HBM instead of four, the SAME result bits.
//   0. knn_query_prep_i8  (knn_batched.hip) padded f32 copy of the query, its two int8 planes, |q|^2, {s_q, |q|^}, the margin, cand_cnt = 0 — or
//                         cap + 1 for a query (or an index) without a finite bound, which steps 3-4 then leave to the gated exact scan
//   1. knn_scan_i8        per row the exact integer S_r = dot(t, c_r) from the int8 shadow, d~ and its window [lo_r, up_r]; up_r is folded into
//                         the per-wave top-kk like a distance of the f32 scan; {lo_r, r} is EMITTED into the wavefront's segment
//                         (knn_emit_plan.h) when lo_r is within the margin of the wavefront's own running threshold, a superset of step 3's rows
//                         (RXGPU_SCAN_I8_EMIT=0, and the gather form: lo_r of every row is stored instead, [n] floats)
//   2. knn_merge_lists    -> T, the kk-th smallest upper bound
//   3. knn_filter_emitted the emitted rows with lo_r <= T + margin (knn_filter_approx over the stored values in the store-all sequence)
//   4. knn_rescore, the gated exact scan, knn_merge_final   EXACT distances of those rows, exact top-kk by (dist, row)
// The arithmetic, the bound and the soundness argument are in knn_i8_quant.h; nothing here rounds before the integer sum is complete.
//
// Mapping.  One 16-lane group owns FOUR consecutive rows per step: lane m loads the 16-byte chunks m, m + 16, ... of each (ld8 / 256 per row;
// 256 contiguous bytes per group and load, 12 loads per lane and step at 768 dims), double-buffered in registers like knn_scan_fixed.  The two
// query planes of a lane's chunks stay in registers for the whole kernel.  The four integer sums of a group are reduced over its 16 lanes
// with a transposing butterfly (4 cross-lane steps instead of 16) that leaves the sum of row j in the lanes with m % 4 == j; lanes m < 4 then
// own one row each: they have loaded its {s_r, e_r} pair (and |x|^2 or inv_norm) along with the codes, emit (or store) lo and offer up.  Rows are in
// increasing order over the lanes of a wavefront and over its steps.
#include <algorithm>
#include <cstdlib>

#include "knn_emit_plan.h"
#include "knn_i8_quant.h"
#include "knn_kernels.hip.h"
#include "knn_scan_common.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kI8RowsPerGroup = 4;
constexpr uint64_t kI8RowsPerWave = 4 * kI8RowsPerGroup;   // rows per wavefront step

__device__ __forceinline__ int i8_dot16(const u32x4& a, const u32x4& b, int acc) {
	acc = __builtin_amdgcn_sdot4(int(a.x), int(b.x), acc, false);
	acc = __builtin_amdgcn_sdot4(int(a.y), int(b.y), acc, false);
	acc = __builtin_amdgcn_sdot4(int(a.z), int(b.z), acc, false);
	acc = __builtin_amdgcn_sdot4(int(a.w), int(b.w), acc, false);
	return acc;
}

static_assert(kI8RowsPerWave == kEmitRowsPerSet && kScanWaves == int(kEmitWavesPerBlock), "knn_emit_plan.h lays the segments out for this mapping");

// NC8 = ld8 / 256: chunks per lane per row (768 -> 3)
// kEmit: instead of leaving lo of every row for knn_filter_approx to read back, the wavefront appends {lo, row} of the rows that can still be
// candidates to its own segment of e.emit (knn_emit_plan.h).  The threshold the filter needs is T, the kk-th smallest up of ALL rows; thr_d of
// the wavefront's own top-kk is the kk-th smallest up of a subset, hence >= T (+inf until the list is full), and f32 addition is monotone, so
// lo <= thr_d + margin holds wherever lo <= T + margin does: the emitted rows are a superset of the candidates, and knn_filter_emitted, which
// holds them against the final T, leaves exactly the set knn_filter_approx finds.  Wave-local: ballot, prefix popcount, a running count in a
// wave-uniform register; no atomics, entries in ascending row order.  A NaN lo or a margin that is not finite emits nothing (the prep has
// set cand_cnt = cap + 1 for such a query: the gated exact scan answers).
// kKeep: lo of every row goes to p.lower as well (a call that records for rxgpu_index_inspect, and the RXGPU_SCAN_I8_EMIT=0 sequence).
template <int kMetric, int NC8, bool kEmit, bool kKeep>
__global__ __launch_bounds__(kScanThreads) void knn_scan_i8(ScanI8Params p, ScanI8Emit e) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.y;
	u32x4 qh[NC8], ql[NC8];
	{
		const u32x4* ph = reinterpret_cast<const u32x4*>(p.planes + size_t(qi) * 2 * p.ld8);
#pragma unroll
		for (int t = 0; t < NC8; ++t) {
			qh[t] = ph[m + 16 * t];
			ql[t] = ph[16 * NC8 + m + 16 * t];
		}
	}
	const float2 qinfo = p.qinfo[qi];   // {s_q, |q| rounded up}
	float qq = 0.f;
	if constexpr (kMetric == kL2) qq = p.q_sq[qi];
	WaveTopK top;
	top.init(p.sp.kk);
	float* lower = p.lower + size_t(qi) * p.sp.n;
	const uint64_t n = p.sp.n;
	const uint64_t nsets = (n + kI8RowsPerWave - 1) / kI8RowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;
	float margin = 0.f;
	EmitEntry* seg = nullptr;
	uint32_t emitted = 0;   // wave-uniform
	if constexpr (kEmit) {
		margin = e.margin[qi];
		seg = e.emit + size_t(qi) * n + emit_segment_offset(e.plan, first);
	}

	struct Buf {
		u32x4 x[kI8RowsPerGroup * NC8];
		float2 side;
		float aux;
	};
	auto issue = [&](Buf& b, uint64_t set) {
		const uint64_t sc = set < nsets ? set : nsets - 1;   // past the end: re-read the last set (never reduced)
		const uint64_t r0 = sc * kI8RowsPerWave + uint64_t(g) * kI8RowsPerGroup;
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			uint64_t row = r0 + j;
			row = row < n ? row : n - 1;
			const u32x4* src = reinterpret_cast<const u32x4*>(p.codes + row * p.ld8) + m;
#pragma unroll
			for (int t = 0; t < NC8; ++t) b.x[j * NC8 + t] = __builtin_nontemporal_load(src + 16 * t);
		}
		uint64_t mine = r0 + (m & 3);
		mine = mine < n ? mine : n - 1;
		b.side = p.side[mine];
		if constexpr (kMetric == kL2) b.aux = p.row_sq[mine];
		if constexpr (kMetric == kCos) b.aux = p.sp.inv_norms[mine];
		if constexpr (kMetric == kIP) b.aux = 0.f;
	};
	auto reduce = [&](const Buf& b, uint64_t set) {
		if (set >= nsets) return;   // wave-uniform
		int v[kI8RowsPerGroup];
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			int hs = 0, ls = 0;
#pragma unroll
			for (int t = 0; t < NC8; ++t) {
				hs = i8_dot16(qh[t], b.x[j * NC8 + t], hs);
				ls = i8_dot16(ql[t], b.x[j * NC8 + t], ls);
			}
			v[j] = hs * 128 + ls;   // this lane's share of dot(t, c): exact (|S| < 2^31, knn_i8_quant.h)
		}
		// transposing butterfly over the group's 16 lanes: afterwards lane m holds the complete sum of row m % 4
		const bool b0 = (m & 1) != 0, b1 = (m & 2) != 0;
		const int a0 = (b0 ? v[1] : v[0]) + __shfl_xor(b0 ? v[0] : v[1], 1);
		const int a1 = (b0 ? v[3] : v[2]) + __shfl_xor(b0 ? v[2] : v[3], 1);
		int s = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
		s += __shfl_xor(s, 4);
		s += __shfl_xor(s, 8);
		const uint64_t row = set * kI8RowsPerWave + uint64_t(g) * kI8RowsPerGroup + (m & 3);
		const bool valid = row < n && m < kI8RowsPerGroup;
		float lo, up;
		i8_bounds(kMetric, i8_ip(qinfo.x, b.side.x, s), qinfo.y, b.side.y, qq, b.aux, lo, up);
		if constexpr (kKeep) {
			if (valid) lower[row] = lo;
		}
		if constexpr (kEmit) {   // against the threshold BEFORE this step's rows are offered
			const float bound = top.thr_d + margin;
			const bool em = valid && margin < __builtin_inff() && lo <= bound;
			const uint64_t emask = __ballot(em);
			if (em) {
				EmitEntry ent;
				ent.lo = lo;
				ent.row = uint32_t(row);
				seg[emitted + uint32_t(__popcll(emask & ((1ull << lane) - 1)))] = ent;
			}
			emitted += uint32_t(__popcll(emask));
		}
		const bool pass = valid && (top.filled < top.kk || up < top.thr_d);
		uint64_t pm = __ballot(pass);
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(up, src);
			const uint32_t i = __shfl(uint32_t(row), src);
			if (top.admits(d, i)) top.insert(d, i, lane);
		}
	};
	if (first < nsets) {
		Buf xa, xb;
		issue(xa, first);
		for (uint64_t set = first; set < nsets; set += 2 * nwaves) {
			issue(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xa, set);
			__builtin_amdgcn_sched_barrier(0);
			issue(xa, set + 2 * nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
		}
	}
	if constexpr (kEmit) {   // every wavefront of the grid, the idle ones too: the filter reads all nwaves counts
		if (lane == 0) e.emit_cnt[size_t(qi) * nwaves + first] = emitted;
	}
	block_merge_and_store(top, p.sp, lane, wave);
}

// ---- the gather form: the same pass over the rows of a list (pre-filtered search and IVF; enqueue_knn_pruned_i8 with a row list in rxgpu_knn_chains.hip).
// `ids` are strictly increasing internal rows, p.sp.n of them, trusted exactly as knn_scan_subset (knn_scan.hip) trusts them.  The arithmetic, the
// lane mapping and the window are knn_scan_i8's (kept apart from it: that kernel is the headline's and stays as measured); what differs is where
// a row comes from and where its lower bound goes: lo is stored at the LIST POSITION (p.lower is [nq][n_ids], so the store stays coalesced and
// knn_filter_approx maps position -> row), the upper bound is offered with the real row.
// kChunked (long lists): a wavefront owns chunks of 64 consecutive entries = 4 steps of 16; ONE coalesced load brings a chunk's ids (lane l:
// entry l), a step's ids are fetched with cross-lane reads, so the id -> address hop is off the per-step path and the code-row loads stay
// double-buffered across chunk boundaries, as in knn_scan_subset.  !kChunked (short lists): one set of 16 entries per wavefront step, 4x
// more wavefronts in flight, no double buffer.  Entries past the end of the list are clamped to its last entry and never reduced, stored or offered.
constexpr uint64_t kI8SubsetChunk = 64;
template <int kMetric, int NC8, bool kChunked>
__global__ __launch_bounds__(kScanThreads) void knn_scan_i8_subset(ScanI8Params p, const uint32_t* __restrict__ ids) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.y;
	u32x4 qh[NC8], ql[NC8];
	{
		const u32x4* ph = reinterpret_cast<const u32x4*>(p.planes + size_t(qi) * 2 * p.ld8);
#pragma unroll
		for (int t = 0; t < NC8; ++t) {
			qh[t] = ph[m + 16 * t];
			ql[t] = ph[16 * NC8 + m + 16 * t];
		}
	}
	const float2 qinfo = p.qinfo[qi];
	float qq = 0.f;
	if constexpr (kMetric == kL2) qq = p.q_sq[qi];
	WaveTopK top;
	top.init(p.sp.kk);
	const uint64_t n = p.sp.n;   // list entries
	float* lower = p.lower + size_t(qi) * n;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;

	struct Buf {
		u32x4 x[kI8RowsPerGroup * NC8];
		float2 side;
		float aux;
		uint32_t row;   // the row of entry (m & 3) of this group's four
	};
	// idv: the ids of the step's 16 entries in lanes e0 .. e0 + 15
	auto issue = [&](Buf& b, uint32_t idv, int e0) {
		const int l0 = e0 + g * kI8RowsPerGroup;
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			const uint64_t row = __shfl(idv, l0 + j);
			const u32x4* src = reinterpret_cast<const u32x4*>(p.codes + row * p.ld8) + m;
#pragma unroll
			for (int t = 0; t < NC8; ++t) b.x[j * NC8 + t] = __builtin_nontemporal_load(src + 16 * t);
		}
		b.row = __shfl(idv, l0 + (m & 3));
		b.side = p.side[b.row];
		if constexpr (kMetric == kL2) b.aux = p.row_sq[b.row];
		if constexpr (kMetric == kCos) b.aux = p.sp.inv_norms[b.row];
		if constexpr (kMetric == kIP) b.aux = 0.f;
	};
	// base: list position of the step's first entry
	auto reduce = [&](const Buf& b, uint64_t base) {
		if (base >= n) return;   // wave-uniform
		int v[kI8RowsPerGroup];
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			int hs = 0, ls = 0;
#pragma unroll
			for (int t = 0; t < NC8; ++t) {
				hs = i8_dot16(qh[t], b.x[j * NC8 + t], hs);
				ls = i8_dot16(ql[t], b.x[j * NC8 + t], ls);
			}
			v[j] = hs * 128 + ls;
		}
		const bool b0 = (m & 1) != 0, b1 = (m & 2) != 0;   // knn_scan_i8's transposing butterfly
		const int a0 = (b0 ? v[1] : v[0]) + __shfl_xor(b0 ? v[0] : v[1], 1);
		const int a1 = (b0 ? v[3] : v[2]) + __shfl_xor(b0 ? v[2] : v[3], 1);
		int s = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
		s += __shfl_xor(s, 4);
		s += __shfl_xor(s, 8);
		const uint64_t pos = base + uint64_t(g) * kI8RowsPerGroup + (m & 3);
		const bool valid = pos < n && m < kI8RowsPerGroup;
		float lo, up;
		i8_bounds(kMetric, i8_ip(qinfo.x, b.side.x, s), qinfo.y, b.side.y, qq, b.aux, lo, up);
		if (valid) lower[pos] = lo;
		const bool pass = valid && (top.filled < top.kk || up < top.thr_d);
		uint64_t pm = __ballot(pass);
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(up, src);
			const uint32_t i = __shfl(b.row, src);
			if (top.admits(d, i)) top.insert(d, i, lane);
		}
	};
	if constexpr (kChunked) {
		constexpr int kSteps = int(kI8SubsetChunk / kI8RowsPerWave);   // 4
		const uint64_t nchunks = (n + kI8SubsetChunk - 1) / kI8SubsetChunk;
		auto load_ids = [&](uint64_t chunk) -> uint32_t {   // clamped: reading past the list re-reads its last entry
			const uint64_t cc = chunk < nchunks ? chunk : nchunks - 1;
			const uint64_t item = cc * kI8SubsetChunk + lane;
			return ids[item < n ? item : n - 1];
		};
		if (first < nchunks) {
			Buf xa, xb;
			uint32_t idc = load_ids(first);
			issue(xa, idc, 0);
			for (uint64_t chunk = first; chunk < nchunks; chunk += nwaves) {
				const uint32_t idn = load_ids(chunk + nwaves);   // in flight while this chunk's steps run
				const uint64_t base = chunk * kI8SubsetChunk;
#pragma unroll 1
				for (int t = 0; t < kSteps; t += 2) {
					issue(xb, idc, (t + 1) * int(kI8RowsPerWave));
					__builtin_amdgcn_sched_barrier(0);
					reduce(xa, base + uint64_t(t) * kI8RowsPerWave);
					__builtin_amdgcn_sched_barrier(0);
					// step t + 2 of this chunk, or step 0 of this wave's next chunk (harmless re-read after the last one)
					const bool next = t + 2 >= kSteps;
					issue(xa, next ? idn : idc, next ? 0 : (t + 2) * int(kI8RowsPerWave));
					__builtin_amdgcn_sched_barrier(0);
					reduce(xb, base + uint64_t(t + 1) * kI8RowsPerWave);
					__builtin_amdgcn_sched_barrier(0);
				}
				idc = idn;
			}
		}
	} else {
		const uint64_t nsets = (n + kI8RowsPerWave - 1) / kI8RowsPerWave;
		for (uint64_t set = first; set < nsets; set += nwaves) {
			const uint64_t item = set * kI8RowsPerWave + m;
			Buf xa;
			issue(xa, ids[item < n ? item : n - 1], 0);
			reduce(xa, set * kI8RowsPerWave);
		}
	}
	block_merge_and_store(top, p.sp, lane, wave);
}

// ---- the range forms (BruteforceSearch::SearchRange from the shadow; enqueue_range_pruned_i8 in rxgpu_knn_chains.hip): one query, no top lists.
// A row can be a hit of the exact kernels only if lo_r <= i8_range_bound(radius, margin) (knn_i8_quant.h); those rows are compacted into
// c.cand_row the way knn_range compacts its hits (ballot, one atomicAdd per wavefront step that has any, prefix popcount), and
// knn_range_rescore (knn_range.hip) holds them against the radius with the exact distance.  The counter counts past c.ccap: the host then
// hands the call to the f32 kernel.  Lane mapping, loads, double buffer and butterfly are knn_scan_i8's, kept apart from it (that kernel is
// the headline's and stays as measured); what is gone is everything the top lists needed.
template <int kMetric, int NC8>
__global__ __launch_bounds__(kScanThreads) void knn_range_i8(ScanI8Params p, RangeI8Cand c) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	u32x4 qh[NC8], ql[NC8];
	{
		const u32x4* ph = reinterpret_cast<const u32x4*>(p.planes);
#pragma unroll
		for (int t = 0; t < NC8; ++t) {
			qh[t] = ph[m + 16 * t];
			ql[t] = ph[16 * NC8 + m + 16 * t];
		}
	}
	const float2 qinfo = p.qinfo[0];   // {s_q, |q| rounded up}
	float qq = 0.f;
	if constexpr (kMetric == kL2) qq = p.q_sq[0];
	const float margin = c.margin[0];
	const float bound = i8_range_bound(c.radius, margin);   // wave-uniform
	const bool bounded = margin < __builtin_inff();
	const uint64_t n = p.sp.n;
	const uint64_t nsets = (n + kI8RowsPerWave - 1) / kI8RowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;

	struct Buf {
		u32x4 x[kI8RowsPerGroup * NC8];
		float2 side;
		float aux;
	};
	auto issue = [&](Buf& b, uint64_t set) {
		const uint64_t sc = set < nsets ? set : nsets - 1;   // past the end: re-read the last set (never reduced)
		const uint64_t r0 = sc * kI8RowsPerWave + uint64_t(g) * kI8RowsPerGroup;
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			uint64_t row = r0 + j;
			row = row < n ? row : n - 1;
			const u32x4* src = reinterpret_cast<const u32x4*>(p.codes + row * p.ld8) + m;
#pragma unroll
			for (int t = 0; t < NC8; ++t) b.x[j * NC8 + t] = __builtin_nontemporal_load(src + 16 * t);
		}
		uint64_t mine = r0 + (m & 3);
		mine = mine < n ? mine : n - 1;
		b.side = p.side[mine];
		if constexpr (kMetric == kL2) b.aux = p.row_sq[mine];
		if constexpr (kMetric == kCos) b.aux = p.sp.inv_norms[mine];
		if constexpr (kMetric == kIP) b.aux = 0.f;
	};
	auto reduce = [&](const Buf& b, uint64_t set) {
		if (set >= nsets) return;   // wave-uniform
		int v[kI8RowsPerGroup];
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			int hs = 0, ls = 0;
#pragma unroll
			for (int t = 0; t < NC8; ++t) {
				hs = i8_dot16(qh[t], b.x[j * NC8 + t], hs);
				ls = i8_dot16(ql[t], b.x[j * NC8 + t], ls);
			}
			v[j] = hs * 128 + ls;
		}
		const bool b0 = (m & 1) != 0, b1 = (m & 2) != 0;   // knn_scan_i8's transposing butterfly
		const int a0 = (b0 ? v[1] : v[0]) + __shfl_xor(b0 ? v[0] : v[1], 1);
		const int a1 = (b0 ? v[3] : v[2]) + __shfl_xor(b0 ? v[2] : v[3], 1);
		int s = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
		s += __shfl_xor(s, 4);
		s += __shfl_xor(s, 8);
		const uint64_t row = set * kI8RowsPerWave + uint64_t(g) * kI8RowsPerGroup + (m & 3);
		const bool valid = row < n && m < kI8RowsPerGroup;
		float lo, up;
		i8_bounds(kMetric, i8_ip(qinfo.x, b.side.x, s), qinfo.y, b.side.y, qq, b.aux, lo, up);
		const bool em = valid && bounded && lo <= bound;   // (a NaN lo or bound: no candidate)
		const uint64_t emask = __ballot(em);
		if (emask) {
			uint32_t base = 0;
			if (lane == 0) base = atomicAdd(c.cand_cnt, uint32_t(__popcll(emask)));
			base = __shfl(base, 0);
			if (em) {
				const uint64_t pos = uint64_t(base) + uint32_t(__popcll(emask & ((1ull << lane) - 1)));
				if (pos < c.ccap) c.cand_row[pos] = uint32_t(row);
			}
		}
	};
	if (first < nsets) {
		Buf xa, xb;
		issue(xa, first);
		for (uint64_t set = first; set < nsets; set += 2 * nwaves) {
			issue(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xa, set);
			__builtin_amdgcn_sched_barrier(0);
			issue(xa, set + 2 * nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
		}
	}
}

// The gather form over a strictly increasing row list (p.sp.n entries, trusted as knn_scan_i8_subset trusts them): one set of 16 entries per
// wavefront step, as that kernel's !kChunked form; the candidate written is the real row.  Entries past the end of the list are clamped to
// its last entry and never reduced or emitted.
template <int kMetric, int NC8>
__global__ __launch_bounds__(kScanThreads) void knn_range_i8_subset(ScanI8Params p, RangeI8Cand c, const uint32_t* __restrict__ ids) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	u32x4 qh[NC8], ql[NC8];
	{
		const u32x4* ph = reinterpret_cast<const u32x4*>(p.planes);
#pragma unroll
		for (int t = 0; t < NC8; ++t) {
			qh[t] = ph[m + 16 * t];
			ql[t] = ph[16 * NC8 + m + 16 * t];
		}
	}
	const float2 qinfo = p.qinfo[0];
	float qq = 0.f;
	if constexpr (kMetric == kL2) qq = p.q_sq[0];
	const float margin = c.margin[0];
	const float bound = i8_range_bound(c.radius, margin);
	const bool bounded = margin < __builtin_inff();
	const uint64_t n = p.sp.n;   // list entries
	const uint64_t nsets = (n + kI8RowsPerWave - 1) / kI8RowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	for (uint64_t set = uint64_t(blockIdx.x) * kScanWaves + wave; set < nsets; set += nwaves) {
		const uint64_t item = set * kI8RowsPerWave + m;
		const uint32_t idv = ids[item < n ? item : n - 1];   // the ids of the step's 16 entries in lanes 0 .. 15
		const int l0 = g * kI8RowsPerGroup;
		u32x4 x[kI8RowsPerGroup * NC8];
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			const uint64_t row = __shfl(idv, l0 + j);
			const u32x4* src = reinterpret_cast<const u32x4*>(p.codes + row * p.ld8) + m;
#pragma unroll
			for (int t = 0; t < NC8; ++t) x[j * NC8 + t] = __builtin_nontemporal_load(src + 16 * t);
		}
		const uint32_t mine = __shfl(idv, l0 + (m & 3));   // the row of entry (m & 3) of this group's four
		const float2 side = p.side[mine];
		float aux = 0.f;
		if constexpr (kMetric == kL2) aux = p.row_sq[mine];
		if constexpr (kMetric == kCos) aux = p.sp.inv_norms[mine];
		int v[kI8RowsPerGroup];
#pragma unroll
		for (int j = 0; j < kI8RowsPerGroup; ++j) {
			int hs = 0, ls = 0;
#pragma unroll
			for (int t = 0; t < NC8; ++t) {
				hs = i8_dot16(qh[t], x[j * NC8 + t], hs);
				ls = i8_dot16(ql[t], x[j * NC8 + t], ls);
			}
			v[j] = hs * 128 + ls;
		}
		const bool b0 = (m & 1) != 0, b1 = (m & 2) != 0;   // knn_scan_i8's transposing butterfly
		const int a0 = (b0 ? v[1] : v[0]) + __shfl_xor(b0 ? v[0] : v[1], 1);
		const int a1 = (b0 ? v[3] : v[2]) + __shfl_xor(b0 ? v[2] : v[3], 1);
		int s = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
		s += __shfl_xor(s, 4);
		s += __shfl_xor(s, 8);
		const uint64_t pos = set * kI8RowsPerWave + uint64_t(g) * kI8RowsPerGroup + (m & 3);
		const bool valid = pos < n && m < kI8RowsPerGroup;
		float lo, up;
		i8_bounds(kMetric, i8_ip(qinfo.x, side.x, s), qinfo.y, side.y, qq, aux, lo, up);
		const bool em = valid && bounded && lo <= bound;
		const uint64_t emask = __ballot(em);
		if (emask) {
			uint32_t base = 0;
			if (lane == 0) base = atomicAdd(c.cand_cnt, uint32_t(__popcll(emask)));
			base = __shfl(base, 0);
			if (em) {
				const uint64_t at = uint64_t(base) + uint32_t(__popcll(emask & ((1ull << lane) - 1)));
				if (at < c.ccap) c.cand_row[at] = mine;
			}
		}
	}
}

// ---- the shadow: codes [n][ld8] (zero pad) and the side pair {s_r, e_r} per row, from the f32 rows (16-byte aligned, stride a multiple of 4
// floats, as the index keeps them).  One 16-lane group per row, lane m quantises the 16-element chunks m, m + 16, ... (read twice: the scale
// first); the residual is an fp64 sum over the codes as stored.  Folds max e^2 into stats[3], max
// (e inv_norm)^2 into stats[4] (cosine) and a non-finite e into stats[2], next to the words of knn_row_stats.
__global__ __launch_bounds__(256) void knn_i8_build(const float* rows, const float* inv_norms, uint64_t n, uint32_t stride, uint32_t dim, int8_t* codes,
													 float2* side, uint32_t ld8, unsigned int* stats) {
	const int lane = threadIdx.x & 63, m = lane & 15;
	const uint64_t ngroups = uint64_t(gridDim.x) * (blockDim.x / kGroup);
	const uint64_t gid = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 4;
	const uint64_t rounds = (n + ngroups - 1) / ngroups;
	const uint32_t nc = ld8 / 256;
	float me = 0.f, mec = 0.f;
	bool bad = false;
	for (uint64_t it = 0; it < rounds; ++it) {   // uniform trip count: every lane takes part in the shuffles
		const uint64_t row = it * ngroups + gid;
		const bool ok = row < n;
		const float* r = rows + (ok ? row : n - 1) * stride;
		float mx = 0.f;
		for (uint32_t t = 0; t < nc; ++t) {
			const uint32_t i0 = (m + 16 * t) * 16;
#pragma unroll
			for (uint32_t e = 0; e < 16; e += 4) {
				if (i0 + e >= dim) continue;
				const float4 v = *reinterpret_cast<const float4*>(r + i0 + e);   // stride is a multiple of 4 floats: in the row's storage
				const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (uint32_t c = 0; c < 4; ++c) {
					if (i0 + e + c < dim) mx = fmaxf(mx, fabsf(x[c]));
				}
			}
		}
		mx = fmaxf(mx, __shfl_xor(mx, 1));
		mx = fmaxf(mx, __shfl_xor(mx, 2));
		mx = fmaxf(mx, __shfl_xor(mx, 4));
		mx = fmaxf(mx, __shfl_xor(mx, 8));
		const float s = i8_scale(mx, kI8CodeMax);
		double r64 = 0.0;
		for (uint32_t t = 0; t < nc; ++t) {
			const uint32_t i0 = (m + 16 * t) * 16;
			uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
			for (uint32_t e = 0; e < 16; e += 4) {
				if (i0 + e >= dim) continue;
				const float4 v = *reinterpret_cast<const float4*>(r + i0 + e);
				const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k) {
					if (i0 + e + k >= dim) continue;
					const int c = i8_quantize(x[k], s, kI8CodeMax);
					const double d = i8_residual(x[k], s, c);
					r64 += d * d;
					w[e >> 2] |= (uint32_t(c) & 0xFFu) << (8 * k);
				}
			}
			if (ok) {
				u32x4 o;
				o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
				*reinterpret_cast<u32x4*>(codes + row * ld8 + i0) = o;
			}
		}
		r64 += __shfl_xor(r64, 1);
		r64 += __shfl_xor(r64, 2);
		r64 += __shfl_xor(r64, 4);
		r64 += __shfl_xor(r64, 8);
		if (ok) {
			const float e = i8_norm_up(r64);
			if (m == 0) side[row] = make_float2(s, e);
			me = fmaxf(me, e * e);
			bad |= !(e * e < __builtin_inff());
			if (inv_norms) {
				const float ei = e * inv_norms[row];
				mec = fmaxf(mec, ei * ei);
				bad |= !(ei * ei < __builtin_inff());
			}
		}
	}
	const bool any_bad = __ballot(bad) != 0;
	for (int o = 32; o; o >>= 1) {
		me = fmaxf(me, __shfl_xor(me, o));
		mec = fmaxf(mec, __shfl_xor(mec, o));
	}
	if (lane == 0) {   // non-negative floats order like their bit patterns
		atomicMax(&stats[3], __float_as_uint(me));
		atomicMax(&stats[4], __float_as_uint(mec));
		if (any_bad) atomicMax(&stats[2], 1u);
	}
}

// ------------------------------------------------------------------------------------------ launchers

// rows / inv_norms / codes / side point at the first row of the range
void launch_i8_build(const float* rows, const float* inv_norms, uint64_t n, uint32_t stride, uint32_t dim, int8_t* codes, float2* side, uint32_t ld8,
					 unsigned int* stats, int cus, hipStream_t s) {
	if (!n) return;
	const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n + 15) / 16, uint64_t(cus) * 8));
	hipLaunchKernelGGL(knn_i8_build, dim3(uint32_t(blocks)), dim3(256), 0, s, rows, inv_norms, n, stride, dim, codes, side, ld8, stats);
}

// Load depth: two buffers of 4 rows per group = 2 x 12 KB per wavefront at 768 dims, 96 KiB per buffer set and CU at 2 workgroups per CU (what
// knn_scan_bf16_blk keeps in flight).  RXGPU_SCAN_I8_WG_PER_CU overrides it (read per call: A/B runs inside one process).
constexpr int kScanI8WgPerCu = 2;
static int scan_i8_wg_per_cu() {
	int wg = kScanI8WgPerCu;
	if (const char* e = getenv("RXGPU_SCAN_I8_WG_PER_CU")) wg = atoi(e);
	return wg < 1 ? 1 : wg > 8 ? 8 : wg;
}
uint32_t scan_i8_grid_x(uint64_t n, int cus) {
	const int wg = scan_i8_wg_per_cu();
	const uint64_t nsets = (n + kI8RowsPerWave - 1) / kI8RowsPerWave;
	const uint64_t want = (nsets + kScanWaves - 1) / kScanWaves;
	const uint64_t cap = uint64_t(cus) * wg;
	return uint32_t(want < cap ? (want ? want : 1) : cap);
}

// The gather form: short lists go to the one-set-per-step kernel (4x more wavefronts in flight), long ones to the chunked, double-buffered
// one; the same rule as subset_use_chunked of the f32 kernels (knn_scan.hip), over this scan's own workgroups-per-CU figure.
static bool scan_i8_subset_chunked(uint64_t n_ids, int cus) {
	return n_ids >= 2 * uint64_t(cus) * scan_i8_wg_per_cu() * kScanWaves * kI8SubsetChunk;
}
uint32_t scan_i8_subset_grid_x(uint64_t n_ids, int cus) {
	const uint64_t per_wave = scan_i8_subset_chunked(n_ids, cus) ? kI8SubsetChunk : kI8RowsPerWave;
	const uint64_t units = (n_ids + per_wave - 1) / per_wave;
	const uint64_t want = (units + kScanWaves - 1) / kScanWaves;
	const uint64_t cap = uint64_t(cus) * scan_i8_wg_per_cu();
	return uint32_t(want < cap ? (want ? want : 1) : cap);
}

template <int kMetric, bool kEmit, bool kKeep>
static void launch_scan_i8_metric(const ScanI8Params& p, const ScanI8Emit& e, dim3 grid, hipStream_t s) {
	switch (p.ld8 / 256) {
		case 1: hipLaunchKernelGGL((knn_scan_i8<kMetric, 1, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		case 2: hipLaunchKernelGGL((knn_scan_i8<kMetric, 2, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		case 3: hipLaunchKernelGGL((knn_scan_i8<kMetric, 3, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		default: hipLaunchKernelGGL((knn_scan_i8<kMetric, 4, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
	}
}
template <bool kEmit, bool kKeep>
static void launch_scan_i8_form(int metric, const ScanI8Params& p, const ScanI8Emit& e, dim3 grid, hipStream_t s) {
	switch (metric) {
		case kL2: launch_scan_i8_metric<kL2, kEmit, kKeep>(p, e, grid, s); break;
		case kIP: launch_scan_i8_metric<kIP, kEmit, kKeep>(p, e, grid, s); break;
		default: launch_scan_i8_metric<kCos, kEmit, kKeep>(p, e, grid, s); break;
	}
}
// p.ld8 must be i8_ld(dim) of a dimension with i8_dim_supported(dim).  emit null: the store-all form (p.lower gets lo of every row, nothing is
// emitted); else e->plan must be emit_plan(p.sp.n, gridx), and keep says whether p.lower is written as well.
void launch_scan_i8(int metric, const ScanI8Params& p, uint32_t nq, uint32_t gridx, hipStream_t s, const ScanI8Emit* emit, bool keep) {
	const dim3 grid(gridx, nq);
	if (!emit) {
		launch_scan_i8_form<false, true>(metric, p, ScanI8Emit{}, grid, s);
	} else if (keep) {
		launch_scan_i8_form<true, true>(metric, p, *emit, grid, s);
	} else {
		launch_scan_i8_form<true, false>(metric, p, *emit, grid, s);
	}
}

template <int kMetric, bool kChunked>
static void launch_scan_i8_subset_metric(const ScanI8Params& p, const uint32_t* ids, dim3 grid, hipStream_t s) {
	switch (p.ld8 / 256) {
		case 1: hipLaunchKernelGGL((knn_scan_i8_subset<kMetric, 1, kChunked>), grid, dim3(kScanThreads), 0, s, p, ids); break;
		case 2: hipLaunchKernelGGL((knn_scan_i8_subset<kMetric, 2, kChunked>), grid, dim3(kScanThreads), 0, s, p, ids); break;
		case 3: hipLaunchKernelGGL((knn_scan_i8_subset<kMetric, 3, kChunked>), grid, dim3(kScanThreads), 0, s, p, ids); break;
		default: hipLaunchKernelGGL((knn_scan_i8_subset<kMetric, 4, kChunked>), grid, dim3(kScanThreads), 0, s, p, ids); break;
	}
}
template <bool kChunked>
static void launch_scan_i8_subset_form(int metric, const ScanI8Params& p, const uint32_t* ids, dim3 grid, hipStream_t s) {
	switch (metric) {
		case kL2: launch_scan_i8_subset_metric<kL2, kChunked>(p, ids, grid, s); break;
		case kIP: launch_scan_i8_subset_metric<kIP, kChunked>(p, ids, grid, s); break;
		default: launch_scan_i8_subset_metric<kCos, kChunked>(p, ids, grid, s); break;
	}
}
// p.sp.n = number of list entries (>= 1); gridx MUST come from scan_i8_subset_grid_x (it selects the kernel together with this function)
void launch_scan_i8_subset(int metric, const ScanI8Params& p, const uint32_t* ids, uint32_t nq, uint32_t gridx, int cus, hipStream_t s) {
	const dim3 grid(gridx, nq);
	if (scan_i8_subset_chunked(p.sp.n, cus)) {
		launch_scan_i8_subset_form<true>(metric, p, ids, grid, s);
	} else {
		launch_scan_i8_subset_form<false>(metric, p, ids, grid, s);
	}
}

template <int kMetric>
static void launch_range_i8_metric(const ScanI8Params& p, const RangeI8Cand& c, const uint32_t* ids, dim3 grid, hipStream_t s) {
	if (ids) {
		switch (p.ld8 / 256) {
			case 1: hipLaunchKernelGGL((knn_range_i8_subset<kMetric, 1>), grid, dim3(kScanThreads), 0, s, p, c, ids); break;
			case 2: hipLaunchKernelGGL((knn_range_i8_subset<kMetric, 2>), grid, dim3(kScanThreads), 0, s, p, c, ids); break;
			case 3: hipLaunchKernelGGL((knn_range_i8_subset<kMetric, 3>), grid, dim3(kScanThreads), 0, s, p, c, ids); break;
			default: hipLaunchKernelGGL((knn_range_i8_subset<kMetric, 4>), grid, dim3(kScanThreads), 0, s, p, c, ids); break;
		}
		return;
	}
	switch (p.ld8 / 256) {
		case 1: hipLaunchKernelGGL((knn_range_i8<kMetric, 1>), grid, dim3(kScanThreads), 0, s, p, c); break;
		case 2: hipLaunchKernelGGL((knn_range_i8<kMetric, 2>), grid, dim3(kScanThreads), 0, s, p, c); break;
		case 3: hipLaunchKernelGGL((knn_range_i8<kMetric, 3>), grid, dim3(kScanThreads), 0, s, p, c); break;
		default: hipLaunchKernelGGL((knn_range_i8<kMetric, 4>), grid, dim3(kScanThreads), 0, s, p, c); break;
	}
}
// The range forms, one query: p.sp.n rows (ids null) or list entries (>= 1), p.ld8 as for launch_scan_i8; p.lower and the part buffers are not
// touched.  The grid is sized here: scan_i8_grid_x for the whole index, one set of 16 entries per wavefront step over a list.
void launch_range_i8(int metric, const ScanI8Params& p, const RangeI8Cand& c, const uint32_t* ids, int cus, hipStream_t s) {
	uint32_t gridx = scan_i8_grid_x(p.sp.n, cus);
	if (ids) {
		const uint64_t nsets = (p.sp.n + kI8RowsPerWave - 1) / kI8RowsPerWave;
		const uint64_t want = (nsets + kScanWaves - 1) / kScanWaves;
		const uint64_t cap = uint64_t(cus) * scan_i8_wg_per_cu();   // as scan_i8_subset_grid_x sizes the one-set-per-step form
		gridx = uint32_t(want < cap ? (want ? want : 1) : cap);
	}
	const dim3 grid(gridx);
	switch (metric) {
		case kL2: launch_range_i8_metric<kL2>(p, c, ids, grid, s); break;
		case kIP: launch_range_i8_metric<kIP>(p, c, ids, grid, s); break;
		default: launch_range_i8_metric<kCos>(p, c, ids, grid, s); break;
	}
}

}  // namespace rxgpu
