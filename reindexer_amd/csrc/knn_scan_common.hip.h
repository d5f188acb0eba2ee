// What the streaming scan kernels of knn_scan.hip, knn_scan_i8.hip and knn_scan_i6.hip share: the workgroup shape and the epilogue that folds
// the per-wavefront top-kk lists into the workgroup's sorted partial list, one overload per list type.
#pragma once

#include "knn_kernels.hip.h"

namespace rxgpu {

constexpr int kScanThreads = 256;                    // 4 wavefronts per workgroup, one per SIMD
constexpr int kScanWaves = kScanThreads / kWave;

// Workgroup epilogue of every scan kernel: fold the per-wave lists into one and store it.
__device__ __forceinline__ void block_merge_and_store(WaveTopK& top, const ScanParams& p, int lane, int wave) {
	__shared__ float s_d[kScanWaves][kMaxFusedK];
	__shared__ uint32_t s_i[kScanWaves][kMaxFusedK];
	s_d[wave][lane] = top.bd;
	s_i[wave][lane] = top.bi;
	__syncthreads();
	if (wave != 0) return;
	for (int w = 1; w < kScanWaves; ++w) {
		const float cd = s_d[w][lane];
		const uint32_t ci = s_i[w][lane];
		// lists are sorted: once one entry is rejected the rest of that list is too
		uint64_t pm = __ballot(ci != kInvalidRow && lane < int(top.kk));
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(cd, src);
			const uint32_t i = __shfl(ci, src);
			if (!top.admits(d, i)) break;
			top.insert(d, i, lane);
		}
	}
	if (lane < int(top.kk)) {
		const size_t o = (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * top.kk + lane;
		p.part_dist[o] = top.bd;
		p.part_row[o] = top.bi;
	}
}

// ... for the two-entries-per-lane list (64 < kk <= 128)
__device__ __forceinline__ void block_merge_and_store(WaveTopK2& top, const ScanParams& p, int lane, int wave) {
	__shared__ float s_d[kScanWaves][kMaxFusedK2];
	__shared__ uint32_t s_i[kScanWaves][kMaxFusedK2];
	s_d[wave][lane] = top.d0;
	s_i[wave][lane] = top.i0;
	s_d[wave][64 + lane] = top.d1;
	s_i[wave][64 + lane] = top.i1;
	__syncthreads();
	if (wave != 0) return;
	for (int w = 1; w < kScanWaves; ++w) {
		for (uint32_t e = 0; e < top.kk; ++e) {   // sorted: once one entry is rejected the rest of that list is too
			const float d = s_d[w][e];
			const uint32_t i = s_i[w][e];
			if (i == kInvalidRow || !top.admits(d, i)) break;
			top.insert(d, i, lane);
		}
	}
	const size_t o = (size_t(blockIdx.y) * gridDim.x + blockIdx.x) * top.kk;
	if (lane < int(top.kk)) {
		p.part_dist[o + lane] = top.d0;
		p.part_row[o + lane] = top.i0;
	}
	if (64 + lane < int(top.kk)) {
		p.part_dist[o + 64 + lane] = top.d1;
		p.part_row[o + 64 + lane] = top.i1;
	}
}

}  // namespace rxgpu
