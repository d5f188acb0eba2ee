// SQ8 codes and corrective offsets of stored rows, computed where the rows live: hnswlib::Quantizer::quantize
// (cpp_src/core/index/float_vector/scalar_quantization/quantizer.h:93-124) for rows [first_row, first_row + n) of an index, bit for bit.
//
// What the reference fixes and what it leaves open:
//   per element  c = (v - minQ) / alpha (correctly rounded division), clamped to [0, 255] by the reference's two comparisons and truncated;
//                err = v - (alpha * code + minQ); a `res` term and a `shift` term, each a function of (v, code) alone
//   per row      res and shift are each ONE f32 chain over i = 0 .. dim - 1 — the order of the additions is the contract, not who computes the terms
// So the terms are computed with the lanes ACROSS the columns (16 lanes x float4 per row: the loads of a wavefront are four 256-byte runs, the
// four codes of a lane leave as one word), written to LDS, and then one lane per row and per chain adds them up in column order.  No
// contraction (-ffp-contract=off), no reassociation, denormals kept (-fno-gpu-flush-denormals-to-zero): the host's expressions, shape for shape.
//
// Tile: 64 rows x 64 columns per workgroup of 256.  Two term planes of [64][65] floats (33 KiB: four workgroups a CU).  The pad makes the
// chain's read — lane r at dword 65 r + c — hit 32 distinct banks per half-wave; the term writes (lane j of a row at dwords 4 j .. 4 j + 3)
// are 2-way conflicted, eight writes against some 600 arithmetic instructions a pass.
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

namespace {
constexpr int kSq8Threads = 256;
constexpr int kSq8TileRows = 64;
constexpr int kSq8TileCols = 64;
constexpr int kSq8Ld = kSq8TileCols + 1;
constexpr int kSq8RowsPerPass = kSq8Threads / (kSq8TileCols / 4);   // 16: a wavefront covers 4 rows x 64 columns with one float4 a lane
constexpr float kSq8Range = 255.f;

// one element: its code and its two terms (Quantizer::quantize's loop body without the two accumulations)
template <bool kIsL2>
__device__ __forceinline__ uint32_t sq8_element(float val, float min_q, float alpha, float& t_res, float& t_shift) {
	float c = (val - min_q) / alpha;
	c = c < 0.f ? 0.f : (c > kSq8Range ? kSq8Range : c);
	const uint8_t code = uint8_t(c);   // truncates
	const float err = val - (alpha * float(code) + min_q);
	if (kIsL2) {
		t_res = (2 * alpha * float(code) + err) * err;
		t_shift = 2.f * alpha * err * float(code);   // shift -= this
	} else {
		t_res = alpha * float(code) + err;
		t_shift = alpha * err * float(code);   // shift += this
	}
	return code;
}
}  // namespace

template <bool kIsL2>
__global__ __launch_bounds__(kSq8Threads) void hnsw_sq8_quantize(const float* __restrict__ rows, uint32_t stride, uint32_t dim, uint64_t first_row,
																 uint64_t n, float min_q, float alpha, float delta, uint8_t* __restrict__ codes,
																 float* __restrict__ corr) {
	__shared__ float s_res[kSq8TileRows * kSq8Ld];
	__shared__ float s_shift[kSq8TileRows * kSq8Ld];
	__shared__ float s_shift_sum[kSq8TileRows];
	const uint32_t t = threadIdx.x;
	const uint32_t quad = t & 15u;            // which float4 of the 64-column chunk
	const uint32_t prow = t >> 4;             // row within a pass of 16
	const uint64_t tile_row = uint64_t(blockIdx.x) * kSq8TileRows;   // relative to first_row
	const bool words = (dim & 3u) == 0;       // every code row starts on a word boundary: the four codes of a lane leave as one store
	// the chains: thread r < 64 carries res of row r, thread 64 + r carries shift of row r
	const uint32_t chain_row = t & 63u;
	float acc = 0.f;

	for (uint32_t c0 = 0; c0 < dim; c0 += kSq8TileCols) {
		const uint32_t col = c0 + quad * 4u;
#pragma unroll
		for (int pass = 0; pass < kSq8TileRows / kSq8RowsPerPass; ++pass) {
			const uint32_t r = uint32_t(pass) * kSq8RowsPerPass + prow;
			const uint64_t rel = tile_row + r;
			const bool live = rel < n && col < dim;
			float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
			// stride % 4 == 0, stride >= round4(dim) and the rows are 16-byte aligned: the float4 at a live column stays inside its row
			if (live) v = *reinterpret_cast<const float4*>(rows + (first_row + rel) * stride + col);
			const float in[4] = {v.x, v.y, v.z, v.w};
			uint32_t packed = 0;
			float* const pr = s_res + r * kSq8Ld + quad * 4u;
			float* const ps = s_shift + r * kSq8Ld + quad * 4u;
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				// what lies behind dim in the row's last float4 is padding (anything, NaN included): not data
				const float val = (live && col + e < dim) ? in[e] : 0.f;
				float tr, ts;
				const uint32_t code = sq8_element<kIsL2>(val, min_q, alpha, tr, ts);
				packed |= code << (8 * e);
				pr[e] = tr;
				ps[e] = ts;
			}
			if (live) {
				uint8_t* const out = codes + (first_row + rel) * dim + col;
				if (words) {
					*reinterpret_cast<uint32_t*>(out) = packed;
				} else {
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						if (col + e < dim) out[e] = uint8_t(packed >> (8 * e));
					}
				}
			}
		}
		__syncthreads();
		if (t < 2 * kSq8TileRows) {
			const float* const terms = (t < kSq8TileRows ? s_res : s_shift) + chain_row * kSq8Ld;
			const uint32_t cols = min(uint32_t(kSq8TileCols), dim - c0);
			if (kIsL2 && t >= kSq8TileRows) {
				for (uint32_t c = 0; c < cols; ++c) acc -= terms[c];
			} else {
				for (uint32_t c = 0; c < cols; ++c) acc += terms[c];
			}
		}
		__syncthreads();
	}
	if (t >= kSq8TileRows && t < 2 * kSq8TileRows) s_shift_sum[chain_row] = acc;
	__syncthreads();
	if (t < kSq8TileRows && tile_row + t < n) {
		float res = acc;
		if (!kIsL2) {
			res *= min_q;
			res += delta;
		}
		res += s_shift_sum[t];
		// a row with an infinite component ends in inf - inf or 0 * inf: x86 hands out the negative default NaN where this device hands out the
		// positive one.  No NaN goes in (the contract), so every NaN here is such a generated one: give it the reference's bits.
		if (res != res) res = __uint_as_float(0xFFC00000u);
		corr[first_row + tile_row + t] = res;
	}
}

void launch_hnsw_sq8_quantize(int metric, const float* rows, uint32_t stride, uint32_t dim, uint64_t first_row, uint64_t n, float min_q, float alpha,
							  float delta, uint8_t* codes, float* corr, hipStream_t s) {
	const uint32_t grid = uint32_t((n + kSq8TileRows - 1) / kSq8TileRows);
	if (metric == kL2) {
		hipLaunchKernelGGL((hnsw_sq8_quantize<true>), dim3(grid), dim3(kSq8Threads), 0, s, rows, stride, dim, first_row, n, min_q, alpha, delta, codes, corr);
	} else {
		hipLaunchKernelGGL((hnsw_sq8_quantize<false>), dim3(grid), dim3(kSq8Threads), 0, s, rows, stride, dim, first_row, n, min_q, alpha, delta, codes, corr);
	}
}

}  // namespace rxgpu
