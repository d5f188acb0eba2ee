// Range search and explicit-row distances over the f32 rows (gfx950): every row, a row list, or the candidates an int8 range scan left.
// One body, range_body, for the three range kernels: only where an item's row number comes from differs.  See knn_kernels.hip.h for the
// arithmetic contract.  Reference being replaced: cpp_src/core/index/float_vector/hnswlib/bruteforce.cc:129-143.
#include "knn_kernels.hip.h"
#include "knn_scan_common.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

// BruteforceSearch::SearchRange (bruteforce.cc:129-143): compact every row with dist < radius (or <=).
struct RangeParams {
	const float* rows;
	const float* inv_norms;
	const float* query;
	uint64_t n;
	uint32_t stride, dim;
	float radius;
	int inclusive;
	float* out_dist;
	uint32_t* out_row;
	uint64_t cap;
	unsigned long long* counter;
};

// Items 0 .. n - 1, one 16-lane group per item and step; row_of(item) is the item's row.  The distance (group_distance_generic and
// metric_epilogue over p.query), the test against p.radius and the counter protocol (p.counter counts every hit, the first p.cap are
// written) are the same for every caller: that is what makes the int8 range tier's exact tail return what knn_range returns.
template <int kMetric, typename RowOf>
__device__ __forceinline__ void range_body(const RangeParams& p, uint64_t n, RowOf row_of) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
	const uint64_t nquads = (n + kRowsPerWave - 1) / kRowsPerWave;
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	for (uint64_t quad = uint64_t(blockIdx.x) * kScanWaves + wave; quad < nquads; quad += nwaves) {
		const uint64_t item = quad * kRowsPerWave + g;
		const bool valid = item < n;
		const uint64_t row = row_of(valid ? item : n - 1);
		const float sum = group_distance_generic<kMetric>(p.rows + row * p.stride, p.query, p.dim, m);
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, row);
		const bool hit = valid && m == 0 && (p.inclusive ? dist <= p.radius : dist < p.radius);
		const uint64_t hm = __ballot(hit);
		if (hm) {
			unsigned long long basePos = 0;
			if (lane == 0) basePos = atomicAdd(p.counter, (unsigned long long)__popcll(hm));
			basePos = __shfl(basePos, 0);
			if (hit) {
				const uint64_t pos = basePos + __popcll(hm & ((1ull << lane) - 1));
				if (pos < p.cap) {
					p.out_dist[pos] = dist;
					p.out_row[pos] = uint32_t(row);
				}
			}
		}
	}
}

template <int kMetric>
__global__ __launch_bounds__(kScanThreads) void knn_range(RangeParams p) {
	range_body<kMetric>(p, p.n, [](uint64_t item) { return item; });
}

// SearchRange restricted to a row list (the list scan of an IVF range query, ivf_index.cc:212-272; p.n = list entries)
template <int kMetric>
__global__ __launch_bounds__(kScanThreads) void knn_range_subset(RangeParams p, const uint32_t* __restrict__ ids) {
	range_body<kMetric>(p, p.n, [ids](uint64_t item) -> uint64_t { return ids[item]; });
}

// The exact tail of the int8 range forms (knn_range_i8 / knn_range_i8_subset in knn_scan_i8.hip): knn_range_subset over the candidate rows,
// their number read on the device.  More candidates than the list holds (or no finite bound: the query prep left ccap + 1): nothing is done,
// the host launches the f32 kernel.
template <int kMetric>
__global__ __launch_bounds__(kScanThreads) void knn_range_rescore(RangeParams p, const uint32_t* __restrict__ cand_cnt, const uint32_t* __restrict__ cand_row,
																   uint32_t ccap) {
	const uint32_t have = *cand_cnt;
	if (have > ccap || have == 0) return;
	range_body<kMetric>(p, have, [cand_row](uint64_t item) -> uint64_t { return cand_row[item]; });
}

// DistCalculator::operator()(q,row,id) for an explicit row list: one 16-lane group per row.
template <int kMetric>
__global__ __launch_bounds__(256) void knn_distances(const float* rows, const float* inv_norms, const float* query, uint32_t stride,
													uint32_t dim, const uint32_t* ids, uint32_t n, float* out) {
	const int lane = threadIdx.x & 63, m = lane & 15;
	const uint32_t item = blockIdx.x * (256u / kGroup) + (threadIdx.x >> 4);   // 16 rows a block: no 32-bit thread-index product (n up to 2^32 - 1)
	const uint32_t itemc = item < n ? item : n - 1;
	const uint64_t row = ids[itemc];
	const float sum = group_distance_generic<kMetric>(rows + row * stride, query, dim, m);
	const float dist = metric_epilogue<kMetric>(sum, inv_norms, row);
	if (item < n && m == 0) out[item] = dist;
}

// ------------------------------------------------------------------------------------------ launchers

void launch_range(int metric, const float* rows, const float* inv_norms, const float* query, uint64_t n, uint32_t stride, uint32_t dim,
				  float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap, unsigned long long* counter,
				  uint32_t gridx, hipStream_t s) {
	RangeParams p{rows, inv_norms, query, n, stride, dim, radius, inclusive, out_dist, out_row, cap, counter};
	switch (metric) {
		case kL2: hipLaunchKernelGGL((knn_range<kL2>), dim3(gridx), dim3(kScanThreads), 0, s, p); break;
		case kIP: hipLaunchKernelGGL((knn_range<kIP>), dim3(gridx), dim3(kScanThreads), 0, s, p); break;
		default: hipLaunchKernelGGL((knn_range<kCos>), dim3(gridx), dim3(kScanThreads), 0, s, p); break;
	}
}

void launch_range_subset(int metric, const float* rows, const float* inv_norms, const float* query, const uint32_t* ids, uint64_t n_ids,
						 uint32_t stride, uint32_t dim, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
						 unsigned long long* counter, uint32_t gridx, hipStream_t s) {
	RangeParams p{rows, inv_norms, query, n_ids, stride, dim, radius, inclusive, out_dist, out_row, cap, counter};
	switch (metric) {
		case kL2: hipLaunchKernelGGL((knn_range_subset<kL2>), dim3(gridx), dim3(kScanThreads), 0, s, p, ids); break;
		case kIP: hipLaunchKernelGGL((knn_range_subset<kIP>), dim3(gridx), dim3(kScanThreads), 0, s, p, ids); break;
		default: hipLaunchKernelGGL((knn_range_subset<kCos>), dim3(gridx), dim3(kScanThreads), 0, s, p, ids); break;
	}
}

// cand_cnt / cand_row / ccap: what knn_range_i8 left; the grid covers ccap candidates
void launch_range_rescore(int metric, const float* rows, const float* inv_norms, const float* query, const uint32_t* cand_cnt, const uint32_t* cand_row,
						  uint32_t ccap, uint32_t stride, uint32_t dim, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
						  unsigned long long* counter, uint32_t gridx, hipStream_t s) {
	RangeParams p{rows, inv_norms, query, 0, stride, dim, radius, inclusive, out_dist, out_row, cap, counter};
	switch (metric) {
		case kL2: hipLaunchKernelGGL((knn_range_rescore<kL2>), dim3(gridx), dim3(kScanThreads), 0, s, p, cand_cnt, cand_row, ccap); break;
		case kIP: hipLaunchKernelGGL((knn_range_rescore<kIP>), dim3(gridx), dim3(kScanThreads), 0, s, p, cand_cnt, cand_row, ccap); break;
		default: hipLaunchKernelGGL((knn_range_rescore<kCos>), dim3(gridx), dim3(kScanThreads), 0, s, p, cand_cnt, cand_row, ccap); break;
	}
}

void launch_distances(int metric, const float* rows, const float* inv_norms, const float* query, uint32_t stride, uint32_t dim,
					  const uint32_t* ids, uint32_t n, float* out, hipStream_t s) {
	const uint32_t blocks = uint32_t((uint64_t(n) * kGroup + 255) / 256);   // 64-bit product: n * 16 wraps from 2^28 rows on
	switch (metric) {
		case kL2: hipLaunchKernelGGL((knn_distances<kL2>), dim3(blocks), dim3(256), 0, s, rows, inv_norms, query, stride, dim, ids, n, out); break;
		case kIP: hipLaunchKernelGGL((knn_distances<kIP>), dim3(blocks), dim3(256), 0, s, rows, inv_norms, query, stride, dim, ids, n, out); break;
		default: hipLaunchKernelGGL((knn_distances<kCos>), dim3(blocks), dim3(256), 0, s, rows, inv_norms, query, stride, dim, ids, n, out); break;
	}
}

}  // namespace rxgpu
