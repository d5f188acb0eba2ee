// The candidate filters of the pruned single-query chains (rxgpu_knn_chains.hip; gfx950): what a pruning scan left -> the rows the exact tail
// re-scores.  Three forms of one test, `value <= thr`: over a value per row (knn_filter_approx, behind knn_scan_bf16 and the value-per-row form
// of knn_scan_i8), over the entries an emitting scan left (knn_filter_emitted behind knn_scan_i8, knn_filter_emitted_wide behind
// knn_scan_i6).  A chain is exact only if its filter uses the threshold its scan was bounded against: filter_threshold is that threshold.
#include <algorithm>

#include "knn_emit_plan.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

// The threshold of query qi: the kk-th best approximate distance of the merged top list (+inf while the list holds fewer than kk) plus the
// query's margin.  False: the query has no finite bound (its query prep has set cand_cnt = cap + 1 and, in the emitting chains, nothing was
// emitted): the filter does nothing and the gated exact scan answers the query.
__device__ __forceinline__ bool filter_threshold(const float* top_dist, const uint32_t* top_count, uint32_t kk, const float* margin, uint32_t qi, float& thr) {
	if (!(margin[qi] < __builtin_inff())) return false;
	thr = (top_count[qi] >= kk ? top_dist[size_t(qi) * kk + kk - 1] : __builtin_inff()) + margin[qi];
	return true;
}

// rows whose approximate distance is within the bound of the kk-th best approximate distance -> candidate list of the query
__global__ __launch_bounds__(256) void knn_filter_approx(const float* approx, uint64_t n, const float* top_dist, const uint32_t* top_count, uint32_t kk,
														 const float* margin, uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap,
														 const uint32_t* __restrict__ ids) {
	const uint32_t qi = blockIdx.y;
	const int lane = threadIdx.x & 63;
	float thr;
	if (!filter_threshold(top_dist, top_count, kk, margin, qi, thr)) return;
	const float* a = approx + size_t(qi) * n;
	const uint64_t span = uint64_t(gridDim.x) * blockDim.x;
	for (uint64_t base = uint64_t(blockIdx.x) * blockDim.x; base < n; base += span) {   // wave-uniform trip count
		const uint64_t row = base + threadIdx.x;
		const bool pass = row < n && a[row] <= thr;
		const uint64_t pm = __ballot(pass);
		if (!pm) continue;
		uint32_t pos0 = 0;
		if (lane == __builtin_ctzll(pm)) pos0 = atomicAdd(&cand_cnt[qi], uint32_t(__popcll(pm)));
		pos0 = __shfl(pos0, __builtin_ctzll(pm));
		const uint32_t pos = pos0 + uint32_t(__popcll(pm & ((1ull << lane) - 1)));
		if (pass && pos < cap) cand_row[size_t(qi) * cap + pos] = ids ? ids[row] : uint32_t(row);   // a row list: position -> row
	}
}

// knn_filter_approx over what knn_scan_i8 emitted (knn_emit_plan.h) instead of a value per row: the same early return, the same threshold, the
// same append.  Workgroups stride over the wavefronts' segments and read emit_cnt[w] entries of each; an entry stays when lo <= thr.  The
// emitted rows are a superset of {lo <= thr} (knn_scan_i8), so the candidate set is the one knn_filter_approx finds over all rows.
__global__ __launch_bounds__(256) void knn_filter_emitted(const EmitEntry* emit, const uint32_t* emit_cnt, EmitPlan plan, const float* top_dist,
														  const uint32_t* top_count, uint32_t kk, const float* margin, uint32_t* cand_row,
														  uint32_t* cand_cnt, uint32_t cap) {
	const uint32_t qi = blockIdx.y;
	const int lane = threadIdx.x & 63;
	float thr;
	if (!filter_threshold(top_dist, top_count, kk, margin, qi, thr)) return;
	const EmitEntry* all = emit + size_t(qi) * plan.n;
	const uint32_t* counts = emit_cnt + size_t(qi) * plan.nwaves;
	for (uint64_t w = blockIdx.x; w < plan.nwaves; w += gridDim.x) {
		const uint64_t room = emit_rows_of(plan, w);
		uint64_t cnt = counts[w];
		cnt = cnt < room ? cnt : room;   // (a count is never above its segment; nothing may read past it whatever the buffer holds)
		const EmitEntry* seg = all + emit_segment_offset(plan, w);
		for (uint64_t base = 0; base < cnt; base += blockDim.x) {   // workgroup-uniform trip count
			const uint64_t at = base + threadIdx.x;
			EmitEntry ent;
			ent.lo = __builtin_inff();
			ent.row = kInvalidRow;
			if (at < cnt) ent = seg[at];
			const bool pass = at < cnt && ent.lo <= thr;
			const uint64_t pm = __ballot(pass);
			if (!pm) continue;
			uint32_t pos0 = 0;
			if (lane == __builtin_ctzll(pm)) pos0 = atomicAdd(&cand_cnt[qi], uint32_t(__popcll(pm)));
			pos0 = __shfl(pos0, __builtin_ctzll(pm));
			const uint32_t pos = pos0 + uint32_t(__popcll(pm & ((1ull << lane) - 1)));
			if (pass && pos < cap) cand_row[size_t(qi) * cap + pos] = ent.row;
		}
	}
}

// knn_filter_emitted for a front that leaves thousands of candidates (knn_scan_i6): the same early return, threshold and test, so the same
// candidate SET (their order in the list differs; nothing reads it as ordered).  That kernel reserves list positions with one atomic per
// wavefront and chunk of 64 entries that has a candidate; with 4 % of the emitted entries passing nearly every chunk has one, and 6 000
// atomics on one word are 60 us at 10M rows.  Here a workgroup strides over the segments twice: it counts what passes, reserves its positions
// with ONE atomic, and writes on the second walk (the entries are in the cache by then).  A wavefront takes the same 64 entries of every
// chunk in both walks, so its positions follow from the four wavefront counts alone.
__global__ __launch_bounds__(256) void knn_filter_emitted_wide(const EmitEntry* emit, const uint32_t* emit_cnt, EmitPlan plan, const float* top_dist,
																const uint32_t* top_count, uint32_t kk, const float* margin, uint32_t* cand_row,
																uint32_t* cand_cnt, uint32_t cap) {
	__shared__ uint32_t s_cnt[4];
	__shared__ uint32_t s_base;
	const uint32_t qi = blockIdx.y;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	float thr;
	if (!filter_threshold(top_dist, top_count, kk, margin, qi, thr)) return;
	const EmitEntry* all = emit + size_t(qi) * plan.n;
	const uint32_t* counts = emit_cnt + size_t(qi) * plan.nwaves;
	uint32_t mine = 0, at0 = 0;   // wave-uniform: what this wavefront's entries pass; the list position of its next candidate
	for (int walk = 0; walk < 2; ++walk) {
		for (uint64_t w = blockIdx.x; w < plan.nwaves; w += gridDim.x) {
			const uint64_t room = emit_rows_of(plan, w);
			uint64_t cnt = counts[w];
			cnt = cnt < room ? cnt : room;   // (a count is never above its segment; nothing may read past it whatever the buffer holds)
			const EmitEntry* seg = all + emit_segment_offset(plan, w);
			for (uint64_t base = uint64_t(wave) * 64; base < cnt; base += 256) {
				const uint64_t at = base + lane;
				EmitEntry ent;
				ent.lo = __builtin_inff();
				ent.row = kInvalidRow;
				if (at < cnt) ent = seg[at];
				const bool pass = at < cnt && ent.lo <= thr;
				const uint64_t pm = __ballot(pass);
				if (walk == 0) {
					mine += uint32_t(__popcll(pm));
				} else {
					const uint32_t pos = at0 + uint32_t(__popcll(pm & ((1ull << lane) - 1)));
					if (pass && pos < cap) cand_row[size_t(qi) * cap + pos] = ent.row;
					at0 += uint32_t(__popcll(pm));
				}
			}
		}
		if (walk == 0) {
			if (lane == 0) s_cnt[wave] = mine;
			__syncthreads();
			if (threadIdx.x == 0) {
				const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
				s_base = total ? atomicAdd(&cand_cnt[qi], total) : 0u;
			}
			__syncthreads();
			at0 = s_base;
			for (int v = 0; v < wave; ++v) at0 += s_cnt[v];
		}
	}
}

// ------------------------------------------------------------------------------------------ launchers

void launch_filter_approx(const float* approx, uint64_t n, const float* top_dist, const uint32_t* top_count, uint32_t kk, const float* margin,
						  uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus, hipStream_t s, const uint32_t* ids) {
	const uint32_t gx = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, uint64_t(cus) * 8)));
	hipLaunchKernelGGL(knn_filter_approx, dim3(gx, nq), dim3(256), 0, s, approx, n, top_dist, top_count, kk, margin, cand_row, cand_cnt, cap, ids);
}

void launch_filter_emitted(const EmitEntry* emit, const uint32_t* emit_cnt, const EmitPlan& plan, const float* top_dist, const uint32_t* top_count, uint32_t kk,
						   const float* margin, uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus, hipStream_t s) {
	const uint32_t gx = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(plan.nwaves, uint64_t(cus) * 8)));
	hipLaunchKernelGGL(knn_filter_emitted, dim3(gx, nq), dim3(256), 0, s, emit, emit_cnt, plan, top_dist, top_count, kk, margin, cand_row, cand_cnt, cap);
}

void launch_filter_emitted_wide(const EmitEntry* emit, const uint32_t* emit_cnt, const EmitPlan& plan, const float* top_dist, const uint32_t* top_count,
								uint32_t kk, const float* margin, uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus, hipStream_t s) {
	const uint32_t gx = uint32_t(std::max<uint64_t>(1, std::min<uint64_t>(plan.nwaves, uint64_t(cus))));
	hipLaunchKernelGGL(knn_filter_emitted_wide, dim3(gx, nq), dim3(256), 0, s, emit, emit_cnt, plan, top_dist, top_count, kk, margin, cand_row, cand_cnt, cap);
}

}  // namespace rxgpu
