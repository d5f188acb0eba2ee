// Streaming brute-force scans with a fused wavefront top-k (gfx950): f32 over every row or a row list, bf16 over the shadow.  What follows a
// scan is in knn_merge.hip (top-k merges), knn_filter.hip (candidate filters of the pruned chains) and knn_range.hip (range, distances).
// See knn_kernels.hip.h for the arithmetic contract.  Reference being replaced:
// cpp_src/core/index/float_vector/hnswlib/bruteforce.cc:103-143.
#include <type_traits>

#include "knn_kernels.hip.h"
#include "knn_scan_common.hip.h"
#include "rxgpu_internal.h"

#include <cstdlib>

namespace rxgpu {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Rows of this wave's step -> candidate insertion.  `dist` is replicated over each 16-lane group.
template <typename TK>
__device__ __forceinline__ void consider_quad(TK& top, float dist, uint32_t row, bool valid, int lane) {
	// Rows arrive in increasing index order within a wave, so a tie with the current worst never enters:
	// strict `<` is exactly the reference's admission test (bruteforce.cc:121).
	const bool pass = valid && (top.filled < top.kk || dist < top.thr_d);
	uint64_t pm = __ballot(pass) & 0x0001000100010001ull;   // one representative lane per group
	while (pm) {
		const int src = __builtin_ctzll(pm);
		pm &= pm - 1;
		const float d = __shfl(dist, src);
		const uint32_t i = __shfl(row, src);
		if (top.admits(d, i)) top.insert(d, i, lane);
	}
}

// dim == 64*NB.  Per step a wavefront streams 4 rows (NB 16-byte loads per lane, all issued back to back).
//   kQLds     : query fragment read from LDS each step (frees NB*4 VGPRs) instead of living in registers
//   kPrefetch : the loads of step i+1 are in flight while step i is reduced (double-buffered registers)
//   kNT       : non-temporal row loads
template <int kMetric, int NB, bool kQLds, bool kPrefetch, bool kNT, typename TK = WaveTopK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_fixed(ScanParams p) {
	__shared__ float4 s_q[kQLds ? NB * 16 : 1];
	if (p.gate_cnt && p.gate_cnt[blockIdx.y] <= p.gate_cap) return;
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float4* qg = reinterpret_cast<const float4*>(p.queries + size_t(blockIdx.y) * p.dim);
	float4 q[kQLds ? 1 : NB];
	if constexpr (kQLds) {
		for (int i = threadIdx.x; i < NB * 16; i += kScanThreads) s_q[i] = qg[i];
		__syncthreads();
	} else {
#pragma unroll
		for (int t = 0; t < NB; ++t) q[t] = qg[16 * t + m];
	}

	TK top;
	top.init(p.kk);

	const uint64_t nquads = (p.n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;

	auto issue = [&](float4 (&x)[NB], uint64_t quad) {
		const uint64_t qc = quad < nquads ? quad : nquads - 1;
		uint64_t row = qc * kRowsPerWave + g;
		row = row < p.n ? row : p.n - 1;
		const float4* rp = reinterpret_cast<const float4*>(p.rows + row * p.stride) + m;
#pragma unroll
		for (int t = 0; t < NB; ++t) x[t] = load_row4<kNT>(rp + 16 * t);
	};
	auto reduce = [&](const float4 (&x)[NB], uint64_t quad) {
		float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int t = 0; t < NB; ++t) {
			if constexpr (kQLds) {
				chain_step<kMetric>(acc, s_q[16 * t + m], x[t]);
			} else {
				chain_step<kMetric>(acc, q[t], x[t]);
			}
		}
		const uint64_t row = quad * kRowsPerWave + g;
		const bool valid = quad < nquads && row < p.n;
		const float sum = fold_chains<false>(acc, nullptr, nullptr, 0, m) + 0.0f;
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, valid ? row : p.n - 1);
		consider_quad(top, dist, uint32_t(row), valid, lane);
	};

	if (first < nquads) {
		if constexpr (kPrefetch) {
			float4 xa[NB], xb[NB];
			issue(xa, first);
			for (uint64_t quad = first; quad < nquads; quad += 2 * nwaves) {
				issue(xb, quad + nwaves);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xa, quad);
				__builtin_amdgcn_sched_barrier(0);
				issue(xa, quad + 2 * nwaves);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xb, quad + nwaves);
				__builtin_amdgcn_sched_barrier(0);
			}
		} else {
			float4 x[NB];
			for (uint64_t quad = first; quad < nquads; quad += nwaves) {
				issue(x, quad);
				__builtin_amdgcn_sched_barrier(0);
				reduce(x, quad);
				__builtin_amdgcn_sched_barrier(0);
			}
		}
	}
	block_merge_and_store(top, p, lane, wave);
}

// Any dim (tails included); query read through the caches.
template <int kMetric, typename TK = WaveTopK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_generic(ScanParams p) {
	if (p.gate_cnt && p.gate_cnt[blockIdx.y] <= p.gate_cap) return;
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float* q = p.queries + size_t(blockIdx.y) * p.dim;
	TK top;
	top.init(p.kk);
	const uint64_t nquads = (p.n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	for (uint64_t quad = uint64_t(blockIdx.x) * kScanWaves + wave; quad < nquads; quad += nwaves) {
		const uint64_t row = quad * kRowsPerWave + g;
		const bool valid = row < p.n;
		const uint64_t rowc = valid ? row : p.n - 1;
		const float sum = group_distance_generic<kMetric>(p.rows + rowc * p.stride, q, p.dim, m);
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, rowc);
		consider_quad(top, dist, uint32_t(row), valid, lane);
	}
	block_merge_and_store(top, p, lane, wave);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Pre-filtered scan: only the rows listed in `ids` (strictly increasing internal row numbers, p.n of them) compete.  This is the
// caller side of `WHERE cond AND KNN(...)` (the reference post-filters on the host, nsselecter.cc:841-875): HBM traffic is
// ids (4 B) + one row per ALLOWED row, so a 5 % filter reads 5 % of the corpus.  Distances are the same per-row arithmetic as
// knn_scan_fixed and the (dist,row) list order is unchanged, hence the result is the unfiltered engine's result over the sub-corpus.
//
// A wavefront owns chunks of 64 consecutive list entries (chunk c of wave w = first + c * nwaves): ONE coalesced 256-byte load brings the
// ids of 16 steps (lane l: step l / 4, group l % 4; a step's id is fetched with a cross-lane read), so the dependent id -> row address
// hop is off the per-step path and the row loads keep the double-buffered issue order of knn_scan_fixed across chunk boundaries.
template <int kMetric, int NB, typename TK = WaveTopK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_subset(ScanParams p, const uint32_t* __restrict__ ids) {
	if (p.gate_cnt && p.gate_cnt[blockIdx.y] <= p.gate_cap) return;
	__shared__ float4 s_q[NB * 16];
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float4* qg = reinterpret_cast<const float4*>(p.queries + size_t(blockIdx.y) * p.dim);
	for (int i = threadIdx.x; i < NB * 16; i += kScanThreads) s_q[i] = qg[i];
	__syncthreads();

	TK top;
	top.init(p.kk);

	constexpr int kChunk = 64, kSteps = kChunk / kRowsPerWave;
	const uint64_t nchunks = (p.n + kChunk - 1) / kChunk;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;

	auto load_ids = [&](uint64_t chunk) -> uint32_t {   // clamped: reading past the list re-reads its last entry
		const uint64_t cc = chunk < nchunks ? chunk : nchunks - 1;
		const uint64_t item = cc * kChunk + lane;
		return ids[item < p.n ? item : p.n - 1];
	};
	auto issue = [&](float4 (&x)[NB], uint32_t row) {
		const float4* rp = reinterpret_cast<const float4*>(p.rows + uint64_t(row) * p.stride) + m;
#pragma unroll
		for (int t = 0; t < NB; ++t) x[t] = load_row4<true>(rp + 16 * t);
	};
	auto reduce = [&](const float4 (&x)[NB], uint64_t item, uint32_t row) {
		float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int t = 0; t < NB; ++t) chain_step<kMetric>(acc, s_q[16 * t + m], x[t]);
		const float sum = fold_chains<false>(acc, nullptr, nullptr, 0, m) + 0.0f;
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, row);
		consider_quad(top, dist, row, item < p.n, lane);
	};

	if (first < nchunks) {
		float4 xa[NB], xb[NB];
		uint32_t idc = load_ids(first);
		issue(xa, __shfl(idc, g));
		for (uint64_t chunk = first; chunk < nchunks; chunk += nwaves) {
			const uint32_t idn = load_ids(chunk + nwaves);   // in flight while this chunk's 16 steps run
			const uint64_t base = chunk * kChunk + g;
#pragma unroll 1
			for (int t = 0; t < kSteps; t += 2) {
				const uint32_t ra = __shfl(idc, t * kRowsPerWave + g);
				const uint32_t rb = __shfl(idc, (t + 1) * kRowsPerWave + g);
				issue(xb, rb);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xa, base + uint64_t(t) * kRowsPerWave, ra);
				__builtin_amdgcn_sched_barrier(0);
				// step t + 2 of this chunk, or step 0 of this wave's next chunk (harmless re-read after the last one)
				const uint32_t rn = t + 2 < kSteps ? __shfl(idc, (t + 2) * kRowsPerWave + g) : __shfl(idn, g);
				issue(xa, rn);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xb, base + uint64_t(t + 1) * kRowsPerWave, rb);
				__builtin_amdgcn_sched_barrier(0);
			}
			idc = idn;
		}
	}
	block_merge_and_store(top, p, lane, wave);
}

// Any dim: one list entry per 16-lane group and step.
template <int kMetric, typename TK = WaveTopK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_subset_generic(ScanParams p, const uint32_t* __restrict__ ids) {
	if (p.gate_cnt && p.gate_cnt[blockIdx.y] <= p.gate_cap) return;
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float* q = p.queries + size_t(blockIdx.y) * p.dim;
	TK top;
	top.init(p.kk);
	const uint64_t nquads = (p.n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	for (uint64_t quad = uint64_t(blockIdx.x) * kScanWaves + wave; quad < nquads; quad += nwaves) {
		const uint64_t item = quad * kRowsPerWave + g;
		const bool valid = item < p.n;
		const uint32_t row = ids[valid ? item : p.n - 1];
		const float sum = group_distance_generic<kMetric>(p.rows + uint64_t(row) * p.stride, q, p.dim, m);
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, row);
		consider_quad(top, dist, row, valid, lane);
	}
	block_merge_and_store(top, p, lane, wave);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// bf16-pruned scan (a single query on a large index where the int8 tier of knn_scan_i8.hip does not apply, see scan_policy_tier in
// rxgpu_knn_chains.hip; RXGPU_SCAN_BF16=1 / 0 force it on / off): half the HBM bytes per query, the SAME result bits.
//   0. knn_query_prep     (knn_batched.hip) padded copy of the query, |q|^2, the margin 2 eps, cand_cnt = 0 — or cap + 1 for a query without a
//                         finite bound, which steps 3-4 then leave to the gated exact scan
//   1. knn_scan_bf16      approximate distance d~ of every row from the bf16 shadow (2 bytes per element), stored ([n] floats) and folded
//                         into the per-wave top-kk exactly like the f32 scan
//   2. knn_merge_lists    (knn_merge.hip) -> d~_(kk), the kk-th best approximate distance (the scan leaves sorted per-workgroup lists)
//   3. knn_filter_approx  (knn_filter.hip) rows with d~ <= d~_(kk) + 2 eps  (eps = the rigorous bf16 bound of knn_query_stats<.., true>)
//   4. knn_rescore, the gated exact scan, knn_merge_final   EXACT distances of those few dozen rows, exact top-kk by (dist, row)
// Soundness: a row r of the true top-kk has d~_r <= d_r + eps <= D_kk + eps, and D_kk <= kk-th smallest of (d~ + eps) = d~_(kk) + eps.
// One 16-lane group owns a row: lane m loads the 16-byte chunks m, m + 16, ... (8 bf16 each; 256 contiguous bytes per group per load),
// widens them to f32 (exact) and runs four fmaf chains against the f32 query fragment it keeps in registers.
template <int NC>
__device__ __forceinline__ float bf16_group_dot(const u32x4 (&x)[NC], const float (&q)[NC * 8]) {
	float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
	for (int t = 0; t < NC; ++t) {
		a0 = __builtin_fmaf(q[8 * t + 0], __uint_as_float(x[t].x << 16), a0);
		a1 = __builtin_fmaf(q[8 * t + 1], __uint_as_float(x[t].x & 0xFFFF0000u), a1);
		a2 = __builtin_fmaf(q[8 * t + 2], __uint_as_float(x[t].y << 16), a2);
		a3 = __builtin_fmaf(q[8 * t + 3], __uint_as_float(x[t].y & 0xFFFF0000u), a3);
		a0 = __builtin_fmaf(q[8 * t + 4], __uint_as_float(x[t].z << 16), a0);
		a1 = __builtin_fmaf(q[8 * t + 5], __uint_as_float(x[t].z & 0xFFFF0000u), a1);
		a2 = __builtin_fmaf(q[8 * t + 6], __uint_as_float(x[t].w << 16), a2);
		a3 = __builtin_fmaf(q[8 * t + 7], __uint_as_float(x[t].w & 0xFFFF0000u), a3);
	}
	float s = (a0 + a2) + (a1 + a3);
	s += __shfl_xor(s, 8);
	s += __shfl_xor(s, 4);
	s += __shfl_xor(s, 2);
	s += __shfl_xor(s, 1);
	return s;
}

// NC = ld / 128: chunks per lane per row (768 -> 6)
template <int kMetric, int NC>
__global__ __launch_bounds__(kScanThreads) void knn_scan_bf16(ScanBf16Params p) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.y;
	float q[NC * 8];
	{
		const float4* qg = reinterpret_cast<const float4*>(p.queries32 + size_t(qi) * p.ld);
#pragma unroll
		for (int t = 0; t < NC; ++t) {
			const float4 lo = qg[2 * (m + 16 * t)], hi = qg[2 * (m + 16 * t) + 1];
			q[8 * t + 0] = lo.x; q[8 * t + 1] = lo.y; q[8 * t + 2] = lo.z; q[8 * t + 3] = lo.w;
			q[8 * t + 4] = hi.x; q[8 * t + 5] = hi.y; q[8 * t + 6] = hi.z; q[8 * t + 7] = hi.w;
		}
	}
	float q_term = 0.f;
	if constexpr (kMetric == kL2) q_term = p.q_sq[qi];
	WaveTopK top;
	top.init(p.sp.kk);
	float* approx = p.approx + size_t(qi) * p.sp.n;
	const uint64_t n = p.sp.n;
	const uint64_t nquads = (n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;
	auto issue = [&](u32x4 (&x)[NC], uint64_t quad) {
		uint64_t row = quad * kRowsPerWave + g;
		if (row >= n) row = n - 1;
		// chunk m + 16 t of the row = k-block (m >> 2) + 4 t, 16-byte piece m & 3 of it; in the tile-blocked shadow the four 16-lane groups
		// of a wavefront (four consecutive rows) read 256 contiguous bytes per k-block, as they read 256 contiguous bytes per row otherwise
		const bool blocked = p.blocked != 0;
		const u32x4* src = reinterpret_cast<const u32x4*>(p.rows16 + shadow_elem_base(row, p.ld, blocked) + uint64_t(m >> 2) * shadow_stage_step(blocked) + (m & 3) * 8);
		const uint32_t tstep = shadow_stage_step(blocked) / 2;   // four k-blocks further on, in 16-byte units
#pragma unroll
		for (int t = 0; t < NC; ++t) x[t] = __builtin_nontemporal_load(src + size_t(tstep) * t);
	};
	auto reduce = [&](const u32x4 (&x)[NC], uint64_t quad) {
		if (quad >= nquads) return;
		const uint64_t row = quad * kRowsPerWave + g;
		const bool valid = row < n;
		const uint64_t rowc = valid ? row : n - 1;
		const float sum = bf16_group_dot<NC>(x, q);
		float dist;
		if constexpr (kMetric == kL2) {
			dist = (q_term + p.row_sq[rowc]) - 2.0f * sum;
		} else if constexpr (kMetric == kIP) {
			dist = -sum;
		} else {
			dist = -sum * p.sp.inv_norms[rowc];
		}
		if (valid && m == 0) approx[row] = dist;
		consider_quad(top, dist, uint32_t(row), valid, lane);
	};
	if (first < nquads) {
		u32x4 xa[NC], xb[NC];
		issue(xa, first);
		for (uint64_t quad = first; quad < nquads; quad += 2 * nwaves) {
			issue(xb, quad + nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xa, quad);
			__builtin_amdgcn_sched_barrier(0);
			issue(xa, quad + 2 * nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xb, quad + nwaves);
			__builtin_amdgcn_sched_barrier(0);
		}
	}
	block_merge_and_store(top, p.sp, lane, wave);
}

// The same pass over the TILE-BLOCKED shadow ([tile of 256 rows][32-element k-block][row][32], knn_kernels.hip.h).  There a row's k-blocks lie
// 16 KB apart, and what is contiguous is a k-block of CONSECUTIVE rows: a wavefront therefore takes 16 rows at a time — lane 4 r + c owns
// 16-byte piece c of every k-block of row r — so that one load instruction reads 16 rows x 64 B = 1 KB in one piece (the 16-lane-per-row
// mapping above reads 256 B pieces from this layout: 2.54 ms against 2.46 on the row-major shadow at 10M x 768).  The query fragment a lane
// needs changes with the k-block: it comes from LDS (four distinct 32-byte addresses per wavefront and k-block: broadcast reads).  The
// k-blocks of a row travel in four groups of NC (the register budget of the double-buffered loads), partial sums carried between them.
template <int kMetric, int NC>
__global__ __launch_bounds__(kScanThreads) void knn_scan_bf16_blk(ScanBf16Params p) {
	__shared__ __attribute__((aligned(16))) float s_q[NC * 128];   // [k-block][piece][8]
	const int lane = threadIdx.x & 63, c = lane & 3, r = lane >> 2;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.y;
	for (int i = threadIdx.x; i < NC * 128 / 4; i += kScanThreads) {
		reinterpret_cast<float4*>(s_q)[i] = reinterpret_cast<const float4*>(p.queries32 + size_t(qi) * p.ld)[i];   // ld = NC * 128 floats, k-major already
	}
	__syncthreads();
	float q_term = 0.f;
	if constexpr (kMetric == kL2) q_term = p.q_sq[qi];
	WaveTopK top;
	top.init(p.sp.kk);
	float* approx = p.approx + size_t(qi) * p.sp.n;
	const uint64_t n = p.sp.n;
	constexpr uint64_t kRows = 16;
	const uint64_t nsets = (n + kRows - 1) / kRows;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;
	// unit u = (row set, k-block group): set = first + (u / 4) * nwaves, group = u % 4
	const uint64_t my_sets = first < nsets ? (nsets - first + nwaves - 1) / nwaves : 0;
	const uint64_t units = my_sets * 4;
	auto issue = [&](u32x4 (&x)[NC], uint64_t u) {
		if (u >= units) return;
		const uint64_t set = first + (u >> 2) * nwaves;
		const uint32_t grp = uint32_t(u & 3);
		uint64_t row = set * kRows + r;
		if (row >= n) row = n - 1;
		const u32x4* src = reinterpret_cast<const u32x4*>(p.rows16 + shadow_elem_base(row, p.ld, true) + uint64_t(grp) * NC * kShadowStageElems + c * 8);
#pragma unroll
		for (int t = 0; t < NC; ++t) x[t] = __builtin_nontemporal_load(src + size_t(t) * (kShadowStageElems / 8));
	};
	float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
	auto reduce = [&](const u32x4 (&x)[NC], uint64_t u) {
		if (u >= units) return;
		const uint32_t grp = uint32_t(u & 3);
#pragma unroll
		for (int t = 0; t < NC; ++t) {
			const float4 qa = *reinterpret_cast<const float4*>(&s_q[((grp * NC + t) * 4 + c) * 8]);
			const float4 qb = *reinterpret_cast<const float4*>(&s_q[((grp * NC + t) * 4 + c) * 8 + 4]);
			a0 = __builtin_fmaf(qa.x, __uint_as_float(x[t].x << 16), a0);
			a1 = __builtin_fmaf(qa.y, __uint_as_float(x[t].x & 0xFFFF0000u), a1);
			a2 = __builtin_fmaf(qa.z, __uint_as_float(x[t].y << 16), a2);
			a3 = __builtin_fmaf(qa.w, __uint_as_float(x[t].y & 0xFFFF0000u), a3);
			a0 = __builtin_fmaf(qb.x, __uint_as_float(x[t].z << 16), a0);
			a1 = __builtin_fmaf(qb.y, __uint_as_float(x[t].z & 0xFFFF0000u), a1);
			a2 = __builtin_fmaf(qb.z, __uint_as_float(x[t].w << 16), a2);
			a3 = __builtin_fmaf(qb.w, __uint_as_float(x[t].w & 0xFFFF0000u), a3);
			if (t & 1) __builtin_amdgcn_sched_barrier(0);   // two k-blocks of query fragment in registers at a time, not all NC (142 VGPRs: 3 waves per SIMD)
		}
		if (grp != 3) return;   // uniform
		float sum = (a0 + a2) + (a1 + a3);
		a0 = a1 = a2 = a3 = 0.f;
		sum += __shfl_xor(sum, 2);
		sum += __shfl_xor(sum, 1);
		const uint64_t set = first + (u >> 2) * nwaves;
		const uint64_t row = set * kRows + r;
		const bool valid = row < n;
		const uint64_t rowc = valid ? row : n - 1;
		float dist;
		if constexpr (kMetric == kL2) {
			dist = (q_term + p.row_sq[rowc]) - 2.0f * sum;
		} else if constexpr (kMetric == kIP) {
			dist = -sum;
		} else {
			dist = -sum * p.sp.inv_norms[rowc];
		}
		if (valid && c == 0) approx[row] = dist;
		// rows in increasing order within the wavefront: lane group r holds row set * 16 + r (consider_quad's rule, one lane per 4-lane group)
		const bool pass = valid && (top.filled < top.kk || dist < top.thr_d);
		uint64_t pm = __ballot(pass) & 0x1111111111111111ull;
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(dist, src);
			const uint32_t i = __shfl(uint32_t(row), src);
			if (top.admits(d, i)) top.insert(d, i, lane);
		}
	};
	if (units) {
		u32x4 xa[NC], xb[NC];
		issue(xa, 0);
		for (uint64_t u = 0; u < units; u += 2) {
			issue(xb, u + 1);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xa, u);
			__builtin_amdgcn_sched_barrier(0);
			issue(xa, u + 2);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xb, u + 1);
			__builtin_amdgcn_sched_barrier(0);
		}
	}
	block_merge_and_store(top, p.sp, lane, wave);
}

// ------------------------------------------------------------------------------------------ launchers

// Tuning knobs (read once): RXGPU_SCAN_QLDS, RXGPU_SCAN_PREFETCH, RXGPU_SCAN_NT, RXGPU_SCAN_WG_PER_CU.
struct ScanTuning {
	int qlds = 1, prefetch = 1, nt = 1, wg_per_cu = 2;   // measured best on MI355X (profiles/r1_tune_ip768.jsonl)
	ScanTuning() {
		if (const char* e = getenv("RXGPU_SCAN_QLDS")) qlds = atoi(e);
		if (const char* e = getenv("RXGPU_SCAN_PREFETCH")) prefetch = atoi(e);
		if (const char* e = getenv("RXGPU_SCAN_NT")) nt = atoi(e);
		if (const char* e = getenv("RXGPU_SCAN_WG_PER_CU")) wg_per_cu = atoi(e);
		if (wg_per_cu < 1) wg_per_cu = 1;
	}
};
constexpr int kScanBf16WgPerCu = 2;   // 2 / 3 / 4 measured at 10M x 768: 2.393 / 2.402 / 2.461 ms per query (profiles/scan_bf16_grid_ab.json)
static const ScanTuning& tuning() {
	static ScanTuning t;
	static const bool dynamic = getenv("RXGPU_TUNE_DYNAMIC") != nullptr;   // tools/tune_scan.py: re-read on every launch
	if (dynamic) t = ScanTuning();
	return t;
}

template <int kMetric, int NB>
static void launch_scan_fixed(const ScanParams& p, dim3 grid, hipStream_t s) {
	const ScanTuning& t = tuning();
	const int v = (t.qlds ? 4 : 0) | (t.prefetch ? 2 : 0) | (t.nt ? 1 : 0);
	const dim3 blk(kScanThreads);
	switch (v) {
		case 0: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, false, false, false>), grid, blk, 0, s, p); break;
		case 1: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, false, false, true>), grid, blk, 0, s, p); break;
		case 2: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, false, true, false>), grid, blk, 0, s, p); break;
		case 3: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, false, true, true>), grid, blk, 0, s, p); break;
		case 4: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, true, false, false>), grid, blk, 0, s, p); break;
		case 5: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, true, false, true>), grid, blk, 0, s, p); break;
		case 6: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, true, true, false>), grid, blk, 0, s, p); break;
		default: hipLaunchKernelGGL((knn_scan_fixed<kMetric, NB, true, true, true>), grid, blk, 0, s, p); break;
	}
}

template <int kMetric>
static void launch_scan_metric_wide(const ScanParams& p, dim3 grid, hipStream_t s) {
	const dim3 blk(kScanThreads);
	switch (p.dim) {
		case 128: hipLaunchKernelGGL((knn_scan_fixed<kMetric, 2, true, true, true, WaveTopK2>), grid, blk, 0, s, p); return;
		case 256: hipLaunchKernelGGL((knn_scan_fixed<kMetric, 4, true, true, true, WaveTopK2>), grid, blk, 0, s, p); return;
		case 512: hipLaunchKernelGGL((knn_scan_fixed<kMetric, 8, true, true, true, WaveTopK2>), grid, blk, 0, s, p); return;
		case 768: hipLaunchKernelGGL((knn_scan_fixed<kMetric, 12, true, true, true, WaveTopK2>), grid, blk, 0, s, p); return;
		case 1024: hipLaunchKernelGGL((knn_scan_fixed<kMetric, 16, true, true, true, WaveTopK2>), grid, blk, 0, s, p); return;
		default: hipLaunchKernelGGL((knn_scan_generic<kMetric, WaveTopK2>), grid, blk, 0, s, p);
	}
}

template <int kMetric>
static void launch_scan_metric(const ScanParams& p, dim3 grid, hipStream_t s) {
	if (p.kk > uint32_t(kMaxFusedK)) {
		launch_scan_metric_wide<kMetric>(p, grid, s);
		return;
	}
	switch (p.dim) {
		case 64: launch_scan_fixed<kMetric, 1>(p, grid, s); return;
		case 128: launch_scan_fixed<kMetric, 2>(p, grid, s); return;
		case 256: launch_scan_fixed<kMetric, 4>(p, grid, s); return;
		case 384: launch_scan_fixed<kMetric, 6>(p, grid, s); return;
		case 512: launch_scan_fixed<kMetric, 8>(p, grid, s); return;
		case 768: launch_scan_fixed<kMetric, 12>(p, grid, s); return;
		case 1024: launch_scan_fixed<kMetric, 16>(p, grid, s); return;
		default: hipLaunchKernelGGL((knn_scan_generic<kMetric>), grid, dim3(kScanThreads), 0, s, p);
	}
}

uint32_t scan_grid_x(uint64_t n, int cus) {
	const uint64_t nquads = (n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t want = (nquads + kScanWaves - 1) / kScanWaves;
	const uint64_t cap = uint64_t(cus) * tuning().wg_per_cu;
	return uint32_t(want < cap ? (want ? want : 1) : cap);
}

// The bf16 scans keep half the bytes in flight per workgroup (two 6 KB load buffers per wavefront at 768 dims, against 12 KB): their grid has
// its own workgroups-per-CU figure.  RXGPU_SCAN_BF16_WG_PER_CU overrides it (read per call: A/B runs inside one process).
uint32_t scan_bf16_grid_x(uint64_t n, int cus) {
	int wg = kScanBf16WgPerCu;
	if (const char* e = getenv("RXGPU_SCAN_BF16_WG_PER_CU")) wg = atoi(e);
	wg = wg < 1 ? 1 : wg > 8 ? 8 : wg;
	const uint64_t nquads = (n + kRowsPerWave - 1) / kRowsPerWave;   // small corpora: scan_grid_x's rule
	const uint64_t want = (nquads + kScanWaves - 1) / kScanWaves;
	const uint64_t cap = uint64_t(cus) * wg;
	return uint32_t(want < cap ? (want ? want : 1) : cap);
}

void launch_scan(int metric, const ScanParams& p, uint32_t nq, uint32_t gridx, hipStream_t s) {
	const dim3 grid(gridx, nq);
	switch (metric) {
		case kL2: launch_scan_metric<kL2>(p, grid, s); break;
		case kIP: launch_scan_metric<kIP>(p, grid, s); break;
		default: launch_scan_metric<kCos>(p, grid, s); break;
	}
}

// ---- pre-filtered scan ----
constexpr uint64_t kSubsetChunk = 64;   // list entries per wavefront chunk of knn_scan_subset

static bool subset_fixed_dim(uint32_t dim, uint32_t kk) {
	if (kk > uint32_t(kMaxFusedK)) return dim == 512 || dim == 768;
	return dim == 128 || dim == 256 || dim == 512 || dim == 768 || dim == 1024;
}
// short lists go to the one-quad-per-step kernel (16x more wavefronts in flight); long ones to the chunked, double-buffered one
static bool subset_use_chunked(uint64_t n_ids, uint32_t dim, uint32_t kk, int cus) {
	const uint64_t waves = uint64_t(cus) * tuning().wg_per_cu * kScanWaves;
	return subset_fixed_dim(dim, kk) && n_ids >= 2 * waves * kSubsetChunk;
}
uint32_t subset_grid_x(uint64_t n_ids, uint32_t dim, uint32_t kk, int cus) {
	if (!subset_use_chunked(n_ids, dim, kk, cus)) return scan_grid_x(n_ids, cus);
	const uint64_t nchunks = (n_ids + kSubsetChunk - 1) / kSubsetChunk;
	const uint64_t want = (nchunks + kScanWaves - 1) / kScanWaves;
	const uint64_t cap = uint64_t(cus) * tuning().wg_per_cu;
	return uint32_t(want < cap ? want : cap);
}

template <int kMetric, typename TK>
static void launch_scan_subset_tk(const ScanParams& p, const uint32_t* ids, bool chunked, dim3 grid, hipStream_t s) {
	const dim3 blk(kScanThreads);
	if (chunked) {
		switch (p.dim) {
			case 128: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_subset<kMetric, 2, TK>), grid, blk, 0, s, p, ids); return; } break;
			case 256: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_subset<kMetric, 4, TK>), grid, blk, 0, s, p, ids); return; } break;
			case 512: hipLaunchKernelGGL((knn_scan_subset<kMetric, 8, TK>), grid, blk, 0, s, p, ids); return;
			case 768: hipLaunchKernelGGL((knn_scan_subset<kMetric, 12, TK>), grid, blk, 0, s, p, ids); return;
			case 1024: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_subset<kMetric, 16, TK>), grid, blk, 0, s, p, ids); return; } break;
			default: break;
		}
	}
	hipLaunchKernelGGL((knn_scan_subset_generic<kMetric, TK>), grid, blk, 0, s, p, ids);
}
template <int kMetric>
static void launch_scan_subset_metric(const ScanParams& p, const uint32_t* ids, bool chunked, dim3 grid, hipStream_t s) {
	if (p.kk > uint32_t(kMaxFusedK)) {
		launch_scan_subset_tk<kMetric, WaveTopK2>(p, ids, chunked, grid, s);
	} else {
		launch_scan_subset_tk<kMetric, WaveTopK>(p, ids, chunked, grid, s);
	}
}
// p.n = number of list entries; gridx MUST come from subset_grid_x (it selects the kernel together with this function)
void launch_scan_subset(int metric, const ScanParams& p, const uint32_t* ids, uint32_t nq, uint32_t gridx, int cus, hipStream_t s) {
	const dim3 grid(gridx, nq);
	const bool chunked = subset_use_chunked(p.n, p.dim, p.kk, cus);
	switch (metric) {
		case kL2: launch_scan_subset_metric<kL2>(p, ids, chunked, grid, s); break;
		case kIP: launch_scan_subset_metric<kIP>(p, ids, chunked, grid, s); break;
		default: launch_scan_subset_metric<kCos>(p, ids, chunked, grid, s); break;
	}
}

template <int kMetric>
static bool launch_scan_bf16_metric(const ScanBf16Params& p, dim3 grid, hipStream_t s) {
	if (p.blocked) {   // the tile-blocked shadow: 16 rows per wavefront
		switch (p.ld / 128) {
			case 1: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 1>), grid, dim3(kScanThreads), 0, s, p); return true;
			case 2: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 2>), grid, dim3(kScanThreads), 0, s, p); return true;
			case 3: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 3>), grid, dim3(kScanThreads), 0, s, p); return true;
			case 4: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 4>), grid, dim3(kScanThreads), 0, s, p); return true;
			case 6: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 6>), grid, dim3(kScanThreads), 0, s, p); return true;
			case 8: hipLaunchKernelGGL((knn_scan_bf16_blk<kMetric, 8>), grid, dim3(kScanThreads), 0, s, p); return true;
			default: return false;
		}
	}
	switch (p.ld / 128) {   // ld is a multiple of 64; the per-lane chunk count must be whole (ld % 128 == 0)
		case 1: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 1>), grid, dim3(kScanThreads), 0, s, p); return true;
		case 2: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 2>), grid, dim3(kScanThreads), 0, s, p); return true;
		case 3: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 3>), grid, dim3(kScanThreads), 0, s, p); return true;
		case 4: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 4>), grid, dim3(kScanThreads), 0, s, p); return true;
		case 6: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 6>), grid, dim3(kScanThreads), 0, s, p); return true;
		case 8: hipLaunchKernelGGL((knn_scan_bf16<kMetric, 8>), grid, dim3(kScanThreads), 0, s, p); return true;
		default: return false;
	}
}
bool scan_bf16_supported(uint32_t ld) {
	const uint32_t nc = ld / 128;
	return ld % 128 == 0 && (nc == 1 || nc == 2 || nc == 3 || nc == 4 || nc == 6 || nc == 8);
}
void launch_scan_bf16(int metric, const ScanBf16Params& p, uint32_t nq, uint32_t gridx, hipStream_t s) {
	const dim3 grid(gridx, nq);
	switch (metric) {
		case kL2: launch_scan_bf16_metric<kL2>(p, grid, s); break;
		case kIP: launch_scan_bf16_metric<kIP>(p, grid, s); break;
		default: launch_scan_bf16_metric<kCos>(p, grid, s); break;
	}
}

}  // namespace rxgpu
