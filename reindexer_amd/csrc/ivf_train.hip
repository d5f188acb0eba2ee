// IVF training where the rows live: the device half of faiss::Clustering::train_encoded as GpuIvfFlat::Train restates it (Clustering.cpp:
// 153-230 compute_centroids; IndexIVFFlat.cpp:54-75 for the cosine preparation) and of add_with_ids' list assignment, over rows an index
// already holds in HBM.  Three pieces; the layout decisions are ivf_train_plan.h, the host side is rxgpu_ivf_assign / rxgpu_ivf_kmeans_step.
//
//   ivf_gather            the PREPARED vectors of list positions (or of a row range) as a packed [n][dim] block: row[j], for cosine
//                         row[j] * (1 / |row|) — one correctly rounded f32 multiply, what NormalizeCopyVector and Train compute.  The block is
//                         what the coarse quantiser's exact k = 1 search (enqueue_knn) reads as device queries.
//   ivf_place_count /     a STABLE placement of the positions into per-centroid segments (ivf_train_plan.h): integer atomics count, prefixes
//   _prefix / _offsets /  give bases, a workgroup ranks 256 positions at a time.  No order is left to an atomic cursor: a segment lists its
//   _place                members' rows in list order.
//   ivf_centroid_sums     what the reference fixes per (centroid c, component j) is ONE f32 chain over the members in list order,
//                             sum = +0;  sum = sum + p_i[j]  (i ascending over the list positions with assign[i] == c);  sum * (1 / float(count))
//                         with p_i rounded to f32 before the add.  Chains of different (c, j) are independent, so: one wavefront per (centroid,
//                         64 columns), lane j carries the chain of column col0 + j, and the members' 256-byte row slices are loaded
//                         kIvfSumLoadsInFlight ahead of the dependent adds (their addresses are known from the segment).  The kernel is
//                         latency-bound per wavefront and lives on occupancy: nlist * ceil(dim / 64) wavefronts.  No float atomics.
// No contraction (explicit __fmul_rn / __fadd_rn on top of the build's -ffp-contract=off: the cosine multiply must not fuse into the add),
// denormals kept.  Vector loads and stores only.
#include <algorithm>

#include "ivf_train_plan.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

namespace {
constexpr int kIvfThreads = 256;
constexpr uint32_t kIvfNoCentroid = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t ivf_row_of(const uint32_t* __restrict__ ids, uint64_t first_row, uint64_t i) {
	return ids ? ids[i] : uint32_t(first_row + i);
}
}  // namespace

// one wavefront per position, lanes across the columns; kVec: dim % 4 == 0, so source (rows are 16-byte aligned at any admitted stride) and
// destination rows both start on 16 bytes
template <bool kCosine, bool kVec>
__global__ __launch_bounds__(kIvfThreads) void ivf_gather(const float* __restrict__ rows, const float* __restrict__ inv_norms, const uint32_t* __restrict__ ids,
														   uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim, float* __restrict__ out) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t waves = uint64_t(gridDim.x) * (kIvfThreads / 64);
	for (uint64_t i = uint64_t(blockIdx.x) * (kIvfThreads / 64) + (threadIdx.x >> 6); i < n; i += waves) {
		const uint32_t r = ivf_row_of(ids, first_row, i);
		const float* __restrict__ src = rows + uint64_t(r) * stride;
		float* __restrict__ dst = out + i * dim;
		float k = 1.f;
		if (kCosine) k = inv_norms[r];
		if (kVec) {
			for (uint32_t j = lane * 4u; j < dim; j += 256u) {
				float4 v = *reinterpret_cast<const float4*>(src + j);
				if (kCosine) v = make_float4(__fmul_rn(v.x, k), __fmul_rn(v.y, k), __fmul_rn(v.z, k), __fmul_rn(v.w, k));
				*reinterpret_cast<float4*>(dst + j) = v;
			}
		} else {
			for (uint32_t j = lane; j < dim; j += 64u) {
				float v = src[j];
				if (kCosine) v = __fmul_rn(v, k);
				dst[j] = v;
			}
		}
	}
}

// workgroup b counts the positions of its span per centroid into row b of the table (zeroed by the host); a position without a centroid
// (the search found none) is left out and flagged
__global__ __launch_bounds__(kIvfThreads) void ivf_place_count(const uint32_t* __restrict__ assign, uint32_t n, uint32_t nlist, uint32_t span,
																uint32_t* __restrict__ table, uint32_t* __restrict__ flag) {
	const uint32_t b = blockIdx.x;
	const uint32_t begin = b * span;
	const uint32_t end = min(n, begin + span);
	for (uint32_t i = begin + threadIdx.x; i < end; i += kIvfThreads) {
		const uint32_t a = assign[i];
		if (a < nlist) {
			atomicAdd(&table[ivf_place_table_index(b, a, nlist)], 1u);
		} else {
			atomicOr(flag, 1u);
		}
	}
}

// thread c: the column of centroid c becomes its exclusive prefix over the spans; counts[c] = the column's total
__global__ __launch_bounds__(kIvfThreads) void ivf_place_prefix(uint32_t* __restrict__ table, uint32_t blocks, uint32_t nlist, uint32_t* __restrict__ counts) {
	const uint32_t c = blockIdx.x * kIvfThreads + threadIdx.x;
	if (c >= nlist) return;
	uint32_t run = 0;
	for (uint32_t b = 0; b < blocks; ++b) {
		const uint64_t t = ivf_place_table_index(b, c, nlist);
		const uint32_t v = table[t];
		table[t] = run;
		run += v;
	}
	counts[c] = run;
}

// ONE workgroup: seg_off = exclusive prefix of the counts it finds in seg_off[1 ..] (seg_off[c + 1] = count of c on entry), hassign = float(count)
__global__ __launch_bounds__(kIvfThreads) void ivf_place_offsets(uint32_t* __restrict__ seg_off, uint32_t nlist, float* __restrict__ hassign) {
	__shared__ uint32_t s_scan[kIvfThreads];
	__shared__ uint32_t s_carry;
	const uint32_t t = threadIdx.x;
	if (t == 0) s_carry = 0;
	__syncthreads();
	for (uint32_t c0 = 0; c0 < nlist; c0 += kIvfThreads) {
		const uint32_t c = c0 + t;
		const uint32_t v = c < nlist ? seg_off[c + 1] : 0u;
		s_scan[t] = v;
		__syncthreads();
		for (uint32_t d = 1; d < kIvfThreads; d <<= 1) {   // inclusive scan of the 256 counts
			const uint32_t add = t >= d ? s_scan[t - d] : 0u;
			__syncthreads();
			s_scan[t] += add;
			__syncthreads();
		}
		const uint32_t carry = s_carry;
		if (c < nlist) {
			seg_off[c + 1] = carry + s_scan[t];
			hassign[c] = float(v);   // exact: a step takes fewer than 2^24 points
		}
		__syncthreads();
		if (t == kIvfThreads - 1) s_carry = carry + s_scan[t];
		__syncthreads();
	}
	if (t == 0) seg_off[0] = 0;
}

// workgroup b walks its span 256 positions at a time, in order: a position's rank among the tile's earlier positions of its centroid + the
// (span, centroid) base, which the tile's last position of the centroid then moves on.  seg_rows receives the ROW of the position.
__global__ __launch_bounds__(kIvfThreads) void ivf_place(const uint32_t* __restrict__ assign, const uint32_t* __restrict__ ids, uint32_t n, uint32_t nlist, uint32_t span,
														  uint32_t* table, const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ seg_rows) {
	__shared__ uint32_t s_key[kIvfPlaceTile];
	const uint32_t b = blockIdx.x;
	const uint32_t t = threadIdx.x;
	const uint32_t begin = b * span;
	const uint32_t end = min(n, begin + span);
	for (uint32_t i0 = begin; i0 < end; i0 += kIvfPlaceTile) {
		const uint32_t i = i0 + t;
		uint32_t key = kIvfNoCentroid;
		if (i < end) {
			key = assign[i];
			if (key >= nlist) key = kIvfNoCentroid;
		}
		s_key[t] = key;
		__syncthreads();
		uint32_t before = 0, total = 0;
		if (key != kIvfNoCentroid) {
			for (uint32_t j = 0; j < kIvfPlaceTile; ++j) {   // every lane reads the same word: a broadcast
				const uint32_t same = s_key[j] == key ? 1u : 0u;
				total += same;
				before += j < t ? same : 0u;
			}
		}
		uint32_t base = 0;
		if (key != kIvfNoCentroid) base = table[ivf_place_table_index(b, key, nlist)];
		__syncthreads();   // every base of this tile is read before one of them moves
		if (key != kIvfNoCentroid) {
			seg_rows[ivf_place_slot(seg_off[key], base, before)] = ivf_row_of(ids, 0, i);
			if (before + 1 == total) table[ivf_place_table_index(b, key, nlist)] = base + total;
		}
		__threadfence_block();
		__syncthreads();   // the moved bases are visible to the next tile; s_key is free again
	}
}

template <bool kCosine>
__global__ __launch_bounds__(kIvfThreads) void ivf_centroid_sums(const float* __restrict__ rows, const float* __restrict__ inv_norms, uint32_t stride, uint32_t dim,
																 uint32_t nlist, const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ seg_rows,
																 float* __restrict__ centroids) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t w = uint64_t(blockIdx.x) * kIvfSumWavesPerBlock + uint32_t(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
	if (w >= ivf_sum_waves(nlist, dim)) return;
	const IvfSumUnit u = ivf_sum_unit(w, dim);
	const bool active = lane < u.cols;
	const uint32_t col = u.col0 + (active ? lane : 0u);   // an idle lane of the last tile walks column col0 along and stores nothing
	const uint32_t beg = seg_off[u.centroid];
	const uint32_t cnt = seg_off[u.centroid + 1] - beg;
	float sum = 0.f;
	for (uint32_t g = 0; g < cnt; g += 64u) {
		// the next 64 members: lane l holds member g + l's row (and 1 / |row|); the walk below broadcasts them one by one.  Lanes behind the
		// last member repeat it: every load of a batch has a valid address and needs no branch, only the adds know where the segment ends.
		const uint32_t left = min(64u, cnt - g);
		const uint32_t my_row = seg_rows[beg + g + min(lane, left - 1u)];
		float my_k = 1.f;
		if (kCosine) my_k = inv_norms[my_row];
		for (uint32_t m = 0; m < left; m += kIvfSumLoadsInFlight) {
			float v[kIvfSumLoadsInFlight];
#pragma unroll
			for (uint32_t e = 0; e < kIvfSumLoadsInFlight; ++e) {   // the row slices of a batch of members, all issued before the first add waits
				const uint32_t r = uint32_t(__builtin_amdgcn_readlane(int(my_row), int(m + e)));
				v[e] = rows[uint64_t(r) * stride + col];
			}
			if (m + kIvfSumLoadsInFlight <= left) {
#pragma unroll
				for (uint32_t e = 0; e < kIvfSumLoadsInFlight; ++e) {
					float p = v[e];
					if (kCosine) p = __fmul_rn(p, __uint_as_float(uint32_t(__builtin_amdgcn_readlane(int(__float_as_uint(my_k)), int(m + e)))));
					sum = __fadd_rn(sum, p);
				}
			} else {
#pragma unroll
				for (uint32_t e = 0; e < kIvfSumLoadsInFlight; ++e) {
					if (m + e < left) {   // wave-uniform
						float p = v[e];
						if (kCosine) p = __fmul_rn(p, __uint_as_float(uint32_t(__builtin_amdgcn_readlane(int(__float_as_uint(my_k)), int(m + e)))));
						sum = __fadd_rn(sum, p);
					}
				}
			}
		}
	}
	// x 1 / count, both correctly rounded (compute_centroids: norm = 1 / hassign[c]; c[j] *= norm); an empty centroid stays all zeros
	if (active) centroids[uint64_t(u.centroid) * dim + col] = cnt ? __fmul_rn(sum, __fdiv_rn(1.0f, float(cnt))) : 0.f;
}

void launch_ivf_gather(int metric, const float* rows, const float* inv_norms, const uint32_t* ids, uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim,
					   float* out, int cus, hipStream_t s) {
	if (n == 0) return;
	const uint64_t want = (n + kIvfThreads / 64 - 1) / (kIvfThreads / 64);
	const uint32_t grid = uint32_t(std::min<uint64_t>(want, uint64_t(cus) * 32));
	const bool cosine = metric == kCos;
	const bool vec = (dim & 3u) == 0;
	if (cosine) {
		if (vec) hipLaunchKernelGGL((ivf_gather<true, true>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, ids, first_row, n, stride, dim, out);
		else hipLaunchKernelGGL((ivf_gather<true, false>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, ids, first_row, n, stride, dim, out);
	} else {
		if (vec) hipLaunchKernelGGL((ivf_gather<false, true>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, ids, first_row, n, stride, dim, out);
		else hipLaunchKernelGGL((ivf_gather<false, false>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, ids, first_row, n, stride, dim, out);
	}
}

// assign [n] -> seg_off [nlist + 1], seg_rows [n] (the members' rows; ids null: position i is row i), hassign [nlist]; table: [blocks][nlist]
// as ivf_place_shape(n, nlist) says.  The caller has zeroed table and flag on s.
void launch_ivf_place(const uint32_t* assign, const uint32_t* ids, uint32_t n, uint32_t nlist, uint32_t* table, uint32_t* seg_off, uint32_t* seg_rows, float* hassign,
					  uint32_t* flag, hipStream_t s) {
	const IvfPlaceShape sh = ivf_place_shape(n, nlist);
	const uint32_t cgrid = (nlist + kIvfThreads - 1) / kIvfThreads;
	if (sh.blocks) hipLaunchKernelGGL(ivf_place_count, dim3(sh.blocks), dim3(kIvfThreads), 0, s, assign, n, nlist, sh.span, table, flag);
	hipLaunchKernelGGL(ivf_place_prefix, dim3(cgrid), dim3(kIvfThreads), 0, s, table, sh.blocks, nlist, seg_off + 1);
	hipLaunchKernelGGL(ivf_place_offsets, dim3(1), dim3(kIvfThreads), 0, s, seg_off, nlist, hassign);
	if (sh.blocks) hipLaunchKernelGGL(ivf_place, dim3(sh.blocks), dim3(kIvfThreads), 0, s, assign, ids, n, nlist, sh.span, table, seg_off, seg_rows);
}

void launch_ivf_centroid_sums(int metric, const float* rows, const float* inv_norms, uint32_t stride, uint32_t dim, uint32_t nlist, const uint32_t* seg_off,
							  const uint32_t* seg_rows, float* centroids, hipStream_t s) {
	const uint32_t grid = uint32_t(ivf_sum_blocks(nlist, dim));
	if (metric == kCos) {
		hipLaunchKernelGGL((ivf_centroid_sums<true>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, stride, dim, nlist, seg_off, seg_rows, centroids);
	} else {
		hipLaunchKernelGGL((ivf_centroid_sums<false>), dim3(grid), dim3(kIvfThreads), 0, s, rows, inv_norms, stride, dim, nlist, seg_off, seg_rows, centroids);
	}
}

}  // namespace rxgpu
