// Level 1 of the batched HNSW build on the device (gfx950): the level-1 lists of the graph — blocks of 1 + M words inside each node's run of
// upper blocks — gathered into a dense array [nodes][1 + M] that has the shape of a level-0 array.  On that view the search kernels
// (hnsw_search.hip) and the selection and back-link kernels of hnsw_build.hip run unchanged, with links0 = view and maxM0 = M; what they
// leave there goes back into the blocks.  The rule: hnsw_build_plan.h and DESIGN §8 (3).
//
//   hnsw_upper_view_gather     view row i = the level-1 block of node i, an empty list where i has level 0
//   hnsw_upper_view_store      the view rows of the nodes a batch touched, back into their blocks
//   hnsw_upper_view_store_ids  the view rows of the batch's own rows, once their blocks exist (rxgpu_hnsw_patch_upper_from)
//   hnsw_upper_pack_rows       the stored rows of the batch's level >= 1 nodes packed as queries
//
// Plain copies: one 64-lane group per list, no arithmetic, every index checked against the node count before it is used.
#include <hip/hip_runtime.h>

#include "hnsw_build.h"

namespace rxgpu {

namespace {

constexpr uint32_t kViewThreads = 256;   // 4 lists per workgroup, 64 lanes each (M <= 64: one pass)

// blocks of node i: [upper_off[i], the next node's first block); the last node's end where the used blocks end
__device__ __forceinline__ uint64_t node_blocks(const HnswUpperView& v, uint32_t i, uint64_t& at) {
	at = v.upper_off[i];
	const uint64_t end = i + 1u < v.nodes ? v.upper_off[i + 1u] : v.upper_used;
	return end > at ? end - at : 0;
}

__global__ __launch_bounds__(kViewThreads) void hnsw_upper_view_gather(HnswUpperView v) {
	const uint32_t i = blockIdx.x * (kViewThreads / 64u) + threadIdx.x / 64u, lane = threadIdx.x & 63u;
	if (i >= v.nodes) return;
	const uint32_t stride = 1u + v.M;
	uint64_t at = 0;
	const bool has = node_blocks(v, i, at) != 0;
	for (uint32_t w = lane; w < stride; w += 64u) v.view[uint64_t(i) * stride + w] = has ? v.upper[at * stride + w] : 0u;
}

__device__ __forceinline__ void store_row(const HnswUpperView& v, uint32_t id, uint32_t lane) {
	if (id >= v.nodes) return;
	const uint32_t stride = 1u + v.M;
	uint64_t at = 0;
	if (node_blocks(v, id, at) == 0) return;   // a node of level 0 has no list to take the row
	for (uint32_t w = lane; w < stride; w += 64u) v.upper[at * stride + w] = v.view[uint64_t(id) * stride + w];
}

__global__ __launch_bounds__(kViewThreads) void hnsw_upper_view_store(HnswUpperView v, const uint32_t* touched, const uint32_t* counters, uint32_t max_touched) {
	const uint32_t j = blockIdx.x * (kViewThreads / 64u) + threadIdx.x / 64u;
	if (j >= min(counters[kBuildCntTouched], max_touched)) return;
	store_row(v, touched[j], threadIdx.x & 63u);
}

__global__ __launch_bounds__(kViewThreads) void hnsw_upper_view_store_ids(HnswUpperView v, const uint32_t* ids, uint32_t n) {
	const uint32_t j = blockIdx.x * (kViewThreads / 64u) + threadIdx.x / 64u;
	if (j >= n) return;
	store_row(v, ids[j], threadIdx.x & 63u);
}

__global__ __launch_bounds__(kViewThreads) void hnsw_upper_pack_rows(const float* rows, uint32_t stride, uint32_t dim, const uint32_t* ids, uint32_t n, float* out) {
	const uint32_t r = blockIdx.x;
	if (r >= n) return;
	const float* src = rows + uint64_t(ids[r]) * stride;
	for (uint32_t c = threadIdx.x; c < dim; c += kViewThreads) out[uint64_t(r) * dim + c] = src[c];
}

inline uint32_t groups(uint32_t lists) { return (lists + kViewThreads / 64u - 1u) / (kViewThreads / 64u); }

}  // namespace

void launch_hnsw_upper_view_gather(const HnswUpperView& v, hipStream_t s) {
	if (v.nodes) hipLaunchKernelGGL(hnsw_upper_view_gather, dim3(groups(v.nodes)), dim3(kViewThreads), 0, s, v);
}

void launch_hnsw_upper_view_store(const HnswUpperView& v, const uint32_t* touched, const uint32_t* counters, uint32_t max_touched, hipStream_t s) {
	if (max_touched) hipLaunchKernelGGL(hnsw_upper_view_store, dim3(groups(max_touched)), dim3(kViewThreads), 0, s, v, touched, counters, max_touched);
}

void launch_hnsw_upper_view_store_ids(const HnswUpperView& v, const uint32_t* ids, uint32_t n, hipStream_t s) {
	if (n) hipLaunchKernelGGL(hnsw_upper_view_store_ids, dim3(groups(n)), dim3(kViewThreads), 0, s, v, ids, n);
}

void launch_hnsw_upper_pack_rows(const float* rows, uint32_t stride, uint32_t dim, const uint32_t* ids, uint32_t n, float* out, hipStream_t s) {
	if (n) hipLaunchKernelGGL(hnsw_upper_pack_rows, dim3(n), dim3(kViewThreads), 0, s, rows, stride, dim, ids, n, out);
}

}  // namespace rxgpu
