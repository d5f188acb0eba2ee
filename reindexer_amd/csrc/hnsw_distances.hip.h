// The distance batches of the HNSW search: rows whose ids sit in LDS against one query, every distance the bits of the reference's.
// Included by hnsw_search_core.hip.h.
#pragma once
#include "knn_kernels.hip.h"

namespace rxgpu {

// Distances of `cnt` rows (ids in LDS) to the query, 4 rows per step; every lane participates in every step.
template <int kMetric>
__device__ __forceinline__ void batch_distances(const HnswParams& p, const float* q, const uint32_t* ids, int cnt, float* dists, int lane) {
	const int m = lane & 15, g = lane >> 4;
	for (int base = 0; base < cnt; base += kRowsPerWave) {
		const int idx = base + g;
		const bool ok = idx < cnt;
		const uint64_t row = ids[ok ? idx : base];
		const float sum = group_distance_generic<kMetric>(p.rows + row * p.stride, q, p.dim, m);
		const float dist = 1.0f * metric_epilogue<kMetric>(sum, p.inv_norms, row);   // normCoef == 1 (hnswalg.h:1855-1863)
		if (ok && m == 0) dists[idx] = dist;
	}
}

// dim == 64*NB, SQ8: 16-byte loads.  Lane m of the row's 16-lane group reads bytes [256 i + 16 m, + 16) of load i: block 4 i + (m >> 2),
// bytes 16 (m & 3) .. + 16 of it, i.e. the element pairs of reference lanes j = 8 (m & 1) + p, p = 0 .. 7 (pair p = halfword p of the 16
// bytes) — in the low half of the block for (m & 3) < 2, in the high half above; both halves feed the same reference lane.  Eight integer
// accumulators a lane, over all blocks (the reference's lanes accumulate over all blocks too); a transpose-reduction over the eight lanes
// of equal parity (xor 2, 4, 8: 7 exchanges) leaves reference lane j's sum on lane (j >> 3) + 2 ((j >> 2) & 1) + 4 ((j >> 1) & 1) + 8 (j & 1),
// and the 16 sums are then added as floats in the reference's order j = 0 .. 15.  L2: (a - b)^2 = a^2 - 2ab + b^2 per pair, exact in
// uint32; the query's b^2 share (qq) is computed once a search.  The query words and qq live in registers for the whole search.
template <int kMetric, int NB>
__device__ __forceinline__ void batch_distances_sq8_fixed(const HnswParams& p, const uint4 (&qw)[(NB + 3) / 4], const uint32_t (&qq)[8], float qcorr,
														  float qnorm, const uint32_t* ids, int cnt, float* dists, int lane) {
	constexpr int L = (NB + 3) / 4;
	const int m = lane & 15, g = lane >> 4;
	const int group_base = lane & ~15;
	for (int base = 0; base < cnt; base += kRowsPerWave) {
		const int idx = base + g;
		const bool ok = idx < cnt;
		const uint64_t row = ids[ok ? idx : base];
		const uint4* r = reinterpret_cast<const uint4*>(p.codes + row * uint64_t(64 * NB));
		uint4 a[L];
#pragma unroll
		for (int i = 0; i < L; ++i) {
			if (256 * i + 256 <= 64 * NB || 256 * i + 16 * m < 64 * NB) {
				a[i] = r[16 * i + m];
			} else {
				a[i] = make_uint4(0u, 0u, 0u, 0u);
			}
		}
		uint32_t ab[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, aa[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
		for (int i = 0; i < L; ++i) {
			const uint32_t aw[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
			const uint32_t bw[4] = {qw[i].x, qw[i].y, qw[i].z, qw[i].w};
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				const uint32_t lo = aw[c] & 0x0000FFFFu, hi = aw[c] & 0xFFFF0000u;
				ab[2 * c] = __builtin_amdgcn_udot4(lo, bw[c], ab[2 * c], false);
				ab[2 * c + 1] = __builtin_amdgcn_udot4(hi, bw[c], ab[2 * c + 1], false);
				if constexpr (kMetric == kL2) {
					aa[2 * c] = __builtin_amdgcn_udot4(lo, aw[c], aa[2 * c], false);
					aa[2 * c + 1] = __builtin_amdgcn_udot4(hi, aw[c], aa[2 * c + 1], false);
				}
			}
		}
		uint32_t s8[8];
#pragma unroll
		for (int q = 0; q < 8; ++q) s8[q] = kMetric == kL2 ? aa[q] + qq[q] - 2u * ab[q] : ab[q];
		const bool up1 = (m & 2) != 0, up2 = (m & 4) != 0, up3 = (m & 8) != 0;
		uint32_t t4[4], t2[2];
#pragma unroll
		for (int q = 0; q < 4; ++q) t4[q] = (up1 ? s8[q + 4] : s8[q]) + uint32_t(__shfl_xor(int(up1 ? s8[q] : s8[q + 4]), 2, 64));
#pragma unroll
		for (int q = 0; q < 2; ++q) t2[q] = (up2 ? t4[q + 2] : t4[q]) + uint32_t(__shfl_xor(int(up2 ? t4[q] : t4[q + 2]), 4, 64));
		const uint32_t mine = (up3 ? t2[1] : t2[0]) + uint32_t(__shfl_xor(int(up3 ? t2[0] : t2[1]), 8, 64));
		float result = 0.f;
#pragma unroll
		for (int j = 0; j < 16; ++j) {   // result += (float)lane[j], j = 0 .. 15
			const int holder = (j >> 3) + 2 * ((j >> 2) & 1) + 4 * ((j >> 1) & 1) + 8 * (j & 1);
			result += float(uint32_t(__shfl(int(mine), group_base + holder, 64)));
		}
		result = result + 0.f;   // + (float)tail, tail == 0: dim is a multiple of 64 (x + 0.f == x for every x the sum can take)
		float dist;
		if constexpr (kMetric == kL2) {
			dist = p.alpha2 * result + qcorr + p.corr[row];
		} else {
			dist = -(p.alpha2 * result + qcorr + p.corr[row]);
			if constexpr (kMetric == kCos) dist *= p.inv_norms[row];
		}
		dist = qnorm * dist;
		if (ok && m == 0) dists[idx] = dist;
	}
}

// dim == 64*NB: the query fragment lives in registers and the NB 16-byte loads of EIGHT rows (two per 16-lane group) are
// issued before the first reduction — one HBM round trip per 8 neighbours instead of three per 4.
// kQLds: the query fragment is re-read from LDS (ds_read_b128) instead of living in NB*4 VGPRs — 48 fewer registers at D = 768, which is
// what lets four of these wavefronts (instead of two) share a SIMD: the search is latency-bound, occupancy is throughput.
template <int kMetric, int NB, bool kQLds, bool kTwoSets>
__device__ __forceinline__ void batch_distances_fixed(const HnswParams& p, const float4 (&q)[kQLds ? 1 : NB], const float4* qlds, const uint32_t* ids,
													  int cnt, float* dists, int lane) {
	const int m = lane & 15, g = lane >> 4;
	auto Q = [&](int t) -> float4 {
		if constexpr (kQLds) {
			return qlds[16 * t + m];
		} else {
			return q[t];
		}
	};
	for (int base = 0; base < cnt; base += (kTwoSets ? 2 : 1) * kRowsPerWave) {
		const int ia = base + g, ib = base + kRowsPerWave + g;
		const bool oka = ia < cnt, okb = ib < cnt;
		const uint64_t ra = ids[oka ? ia : base], rb = ids[okb ? ib : base];
		const float4* pa = reinterpret_cast<const float4*>(p.rows + ra * p.stride) + m;
		const float4* pb = reinterpret_cast<const float4*>(p.rows + rb * p.stride) + m;
		float4 xa[NB], xb[NB];
#pragma unroll
		for (int t = 0; t < NB; ++t) xa[t] = pa[16 * t];
		const bool second = kTwoSets && base + kRowsPerWave < cnt;   // wave-uniform; one row set per trip keeps the D = 768 kernel at 4+ waves per SIMD
		if (second) {
#pragma unroll
			for (int t = 0; t < NB; ++t) xb[t] = pb[16 * t];
		}
		// cosine: 1 / |row| of the epilogue travels WITH the rows — read behind the scheduling barrier it was a dependent round trip of its
		// own at the end of every distance trip
		float inva = 1.0f, invb = 1.0f;
		if constexpr (kMetric == kCos) {
			inva = p.inv_norms[ra];
			if (second) invb = p.inv_norms[rb];
		}
		__builtin_amdgcn_sched_barrier(0);
		float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int t = 0; t < NB; ++t) chain_step<kMetric>(acc, Q(t), xa[t]);
		const float da = 1.0f * metric_epilogue<kMetric>(fold_chains<false>(acc, nullptr, nullptr, 0, m) + 0.0f, &inva, 0);
		if (oka && m == 0) dists[ia] = da;
		if (second) {
			acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
			for (int t = 0; t < NB; ++t) chain_step<kMetric>(acc, Q(t), xb[t]);
			const float db = 1.0f * metric_epilogue<kMetric>(fold_chains<false>(acc, nullptr, nullptr, 0, m) + 0.0f, &invb, 0);
			if (okb && m == 0) dists[ib] = db;
		}
	}
}

// dim == 64*NB, NB > 12 (1024 and 1536 floats): a whole row set of NB float4 a lane (96 VGPRs at NB = 24) does not fit beside the search's
// own state, so the NB loads of a row are cut into chunks of kChunk and the loads of chunk c + 1 are issued before chunk c is reduced: two
// chunks of a row set are in flight or in registers at any time.  The ONE accumulator runs through the chunks in block order —
// acc = chain_step(acc, Q(t), x[t]) for t = 0 .. NB - 1, the sequence batch_distances_fixed and the generic batch compute — and is folded once.
// The latency, team and resident forms (one or two wavefronts per SIMD anyway) take two row sets in chunks of 8: 128 VGPRs of rows, 2 and 3 chunks.
// The throughput form takes one set in chunks of 4 (32 VGPRs of rows, 4 and 6 chunks): 87 - 99 VGPRs in all, where chunks of 8 came to
// 131 - 141 and, held to 128 by __launch_bounds__, spilled.  The query fragment is always read from LDS.
template <int kMetric, int NB, bool kTwoSets, int kChunk = 8>
__device__ __forceinline__ void batch_distances_wide(const HnswParams& p, const float4* qlds, const uint32_t* ids, int cnt, float* dists, int lane) {
	static_assert(NB > kChunk && NB % kChunk == 0, "whole chunks, at least two");
	constexpr int kChunks = NB / kChunk;
	const int m = lane & 15, g = lane >> 4;
	for (int base = 0; base < cnt; base += (kTwoSets ? 2 : 1) * kRowsPerWave) {
		const int ia = base + g, ib = base + kRowsPerWave + g;
		const bool oka = ia < cnt, okb = ib < cnt;
		const uint64_t ra = ids[oka ? ia : base], rb = ids[okb ? ib : base];
		const float4* pa = reinterpret_cast<const float4*>(p.rows + ra * p.stride) + m;
		const float4* pb = reinterpret_cast<const float4*>(p.rows + rb * p.stride) + m;
		const bool second = kTwoSets && base + kRowsPerWave < cnt;   // wave-uniform
		float4 xa[2][kChunk], xb[2][kChunk];
#pragma unroll
		for (int t = 0; t < kChunk; ++t) xa[0][t] = pa[16 * t];
		if (second) {
#pragma unroll
			for (int t = 0; t < kChunk; ++t) xb[0][t] = pb[16 * t];
		}
		float inva = 1.0f, invb = 1.0f;   // cosine: 1 / |row| travels with the first chunk (see batch_distances_fixed)
		if constexpr (kMetric == kCos) {
			inva = p.inv_norms[ra];
			if (second) invb = p.inv_norms[rb];
		}
		float4 acca = make_float4(0.f, 0.f, 0.f, 0.f), accb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int c = 0; c < kChunks; ++c) {
			if (c + 1 < kChunks) {   // the next chunk's loads go out before this chunk is reduced
#pragma unroll
				for (int t = 0; t < kChunk; ++t) xa[(c + 1) & 1][t] = pa[16 * (kChunk * (c + 1) + t)];
				if (second) {
#pragma unroll
					for (int t = 0; t < kChunk; ++t) xb[(c + 1) & 1][t] = pb[16 * (kChunk * (c + 1) + t)];
				}
			}
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int t = 0; t < kChunk; ++t) chain_step<kMetric>(acca, qlds[16 * (kChunk * c + t) + m], xa[c & 1][t]);
			if (second) {
#pragma unroll
				for (int t = 0; t < kChunk; ++t) chain_step<kMetric>(accb, qlds[16 * (kChunk * c + t) + m], xb[c & 1][t]);
			}
			__builtin_amdgcn_sched_barrier(0);
		}
		const float da = 1.0f * metric_epilogue<kMetric>(fold_chains<false>(acca, nullptr, nullptr, 0, m) + 0.0f, &inva, 0);
		if (oka && m == 0) dists[ia] = da;
		if (second) {
			const float db = 1.0f * metric_epilogue<kMetric>(fold_chains<false>(accb, nullptr, nullptr, 0, m) + 0.0f, &invb, 0);
			if (okb && m == 0) dists[ib] = db;
		}
	}
}

}  // namespace rxgpu
