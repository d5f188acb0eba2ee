// What travels around the ft_fast merge trains: the plan in (ft_import, ft_import_pieces), the packed result out (ft_export), and the three
// per-query facts document-range shards exchange between the pieces of the dense train (ft_shard_*).  Copy and sum kernels only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "rxgpu_internal.h"
#include "ft_replay.hip.h"

namespace rxgpu {

// The packed result (header + four arrays, ~11 B per merged document) leaves through a copy kernel writing 16-byte words straight into
// the caller's pinned host buffer: a hipMemcpyAsync of the same 220 KB took ~40 us from enqueue to completion (copy-engine start-up),
// a third of the merge.  Only the header and the first numDocs entries of every array are written.
__global__ __launch_bounds__(256) void ft_export(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	if (!p.host_out) return;
	const uint32_t n = p.out_header[0] < p.max_merged ? p.out_header[0] : p.max_merged;
	const uint4* src = reinterpret_cast<const uint4*>(p.out_header);
	uint4* dst = reinterpret_cast<uint4*>(p.host_out);
	// region r of the packed layout: [start, start + bytes actually used), in 16-byte words
	const size_t a16 = 16, m4 = (size_t(p.max_merged) * 4 + 255) & ~size_t(255), m2 = (size_t(p.max_merged) * 2 + 255) & ~size_t(255);
	const size_t starts[5] = {0, 256, 256 + m4, 256 + 2 * m4, 256 + 2 * m4 + m2};
	const size_t used[5] = {a16, size_t(n) * 4, size_t(n) * 4, size_t(n) * 2, size_t(n)};
	const size_t gtid = size_t(blockIdx.x) * blockDim.x + threadIdx.x, gsize = size_t(gridDim.x) * blockDim.x;
#pragma unroll
	for (int r = 0; r < 5; ++r) {
		const size_t w0 = starts[r] / 16, w1 = (starts[r] + used[r] + 15) / 16;
		for (size_t w = w0 + gtid; w < w1; w += gsize) dst[w] = src[w];
	}
}

// The plan (sub-term and term descriptors, grid entries, per-field parameters: a few KB) comes in the same way: one small workgroup
// reads it from the pinned staging buffer and writes it where the kernels expect it — no copy-engine transfer in front of the train.
__global__ __launch_bounds__(256) void ft_import(const uint4* host_plan, uint4* dev_plan, uint32_t n16) {
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < n16; w += gridDim.x * blockDim.x) dev_plan[w] = host_plan[w];
}
// the plans of a batch (and the FtPlan array itself) from their pinned staging buffers into HBM in ONE launch: blockIdx.y = piece
__global__ __launch_bounds__(256) void ft_import_pieces(FtImportBatch b) {
	const uint32_t j = blockIdx.y;
	const uint4* src = reinterpret_cast<const uint4*>(b.src[j]);
	uint4* dst = reinterpret_cast<uint4*>(b.dst[j]);
	for (uint32_t w = blockIdx.x * blockDim.x + threadIdx.x; w < b.n16[j]; w += gridDim.x * blockDim.x) dst[w] = src[w];
}
hipError_t launch_ft_import_batch(const FtImportBatch& b, hipStream_t st) {
	if (b.n) hipLaunchKernelGGL(ft_import_pieces, dim3(4, b.n), dim3(256), 0, st, b);
	return hipGetLastError();
}
hipError_t launch_ft_import(const void* host_plan, void* dev_plan, size_t bytes, hipStream_t st) {
	const uint32_t n16 = uint32_t((bytes + 15) / 16);
	hipLaunchKernelGGL(ft_import, dim3((n16 + 255) / 256 < 16 ? (n16 + 255) / 256 : 16), dim3(256), 0, st, reinterpret_cast<const uint4*>(host_plan),
					   reinterpret_cast<uint4*>(dev_plan), n16);
	return hipGetLastError();
}

// the results' way out (after the merge's timing bracket: the roofline of the merge kernels does not include the transfer)
hipError_t launch_ft_export(const FtPlan* plans, const FtPlan* host_plans, uint32_t nq, hipStream_t st) {
	bool any = false;
	for (uint32_t q = 0; q < nq; ++q) any = any || host_plans[q].host_out;
	if (any) hipLaunchKernelGGL(ft_export, dim3(nq > 4 ? 16 : 64, nq), dim3(256), 0, st, plans);
	return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------- document-range shards: what travels between the kernels
// One shard's pre-score histogram, its kFtHistCopies copies added up (fine counters, then the chunk counters), and the popcount of its
// mask words behind them: what the all-gather carries.
__global__ __launch_bounds__(256) void ft_shard_fold(const FtPlan* plans, uint32_t* dst) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < kFtFoldWords; i += gridDim.x * 256) {
		uint32_t v = 0;
		if (i < kFtHistStride) {
			if (p.hist) {
#pragma unroll
				for (uint32_t k = 0; k < kFtHistCopies; ++k) v += p.hist[size_t(k) * kFtHistStride + i];
			}
		} else if (i == kFtHistStride) {
			v = p.sync[kFtSyncPop];
		}
		dst[i] = v;
	}
}
// ... and back: copy 0 of the histogram = the sum over the shards (the other copies zero), the popcount = the sum: ft_preselect_on and
// ft_pick_threshold then decide on the WHOLE index, every shard alike.  pos[s] = where shard s lies in the gathered buffer.
__global__ __launch_bounds__(256) void ft_shard_hist_combine(const FtPlan* plans, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i <= kFtHistStride; i += gridDim.x * 256) {
		uint32_t v = 0;
		for (uint32_t sh = 0; sh < n_shards; ++sh) v += gathered[size_t(pos[sh]) * kFtFoldWords + i];
		if (i < kFtHistStride) {
			if (p.hist) {
				p.hist[i] = v;
#pragma unroll
				for (uint32_t k = 1; k < kFtHistCopies; ++k) p.hist[size_t(k) * kFtHistStride + i] = 0u;
			}
		} else {
			p.sync[kFtSyncPop] = v;
		}
	}
}
// the table of ft_adders: every shard filled its own columns (the rest zero) — the sum is the table of the whole index
__global__ __launch_bounds__(256) void ft_shard_table_sum(uint32_t* table, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards, uint64_t n, uint64_t stride) {
	for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256) {
		uint32_t v = 0;
		for (uint32_t sh = 0; sh < n_shards; ++sh) v += gathered[size_t(pos[sh]) * stride + i];
		table[i] = v;
	}
}
void launch_ft_shard_fold(const FtPlan* plan, uint32_t* dst, hipStream_t st) { hipLaunchKernelGGL(ft_shard_fold, dim3(64), dim3(256), 0, st, plan, dst); }
void launch_ft_shard_hist_combine(const FtPlan* plan, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards, hipStream_t st) {
	hipLaunchKernelGGL(ft_shard_hist_combine, dim3(64), dim3(256), 0, st, plan, gathered, pos, n_shards);
}
void launch_ft_shard_table_sum(uint32_t* table, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards, uint64_t n, uint64_t stride, hipStream_t st) {
	if (!n) return;
	hipLaunchKernelGGL(ft_shard_table_sum, dim3(uint32_t(std::min<uint64_t>(256, (n + 255) / 256))), dim3(256), 0, st, table, gathered, pos, n_shards, n, stride);
}

}  // namespace rxgpu
