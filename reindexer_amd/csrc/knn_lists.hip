// IVF-Flat list scan for a batch of queries (gfx950): the hot kernel of rxgpu_search_knn_lists_batch and the small kernel in front of it.
//   ivf_batch_offsets  per query the running chunk counts of its probed lists ([nprobe + 1], ivf_batch_plan.h) and the rows probed
//   knn_scan_lists     grid (gridx, nq): workgroup (x, y) scans its share of the 64-entry chunks of query y's CONCATENATED probed lists and
//                      leaves a sorted partial top-kk, as every scan of knn_scan.hip does; knn_merge_lists (knn_merge.hip) follows
// The inverted lists are disjoint, so a query's candidates are the concatenation of its probed lists: no bitmap, no row-list union.  The
// top-kk under (dist, row) does not depend on the order in which candidates are met, and a row's distance is the arithmetic of
// knn_scan_subset / knn_scan_subset_generic unchanged (a 16-lane group owns a row; chain_step, fold_chains, metric_epilogue), hence the
// result is rxgpu_search_knn_lists's, bit for bit.  No atomics; the only stores are the partial lists.
#include <type_traits>

#include "ivf_batch_plan.h"
#include "knn_kernels.hip.h"
#include "knn_scan_common.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

static_assert(kIvfBatchMaxProbe == uint32_t(kMaxFusedK2) && kIvfBatchMaxKk == uint32_t(kMaxFusedK2), "the envelope is the widest fused top list");
static_assert(kIvfBatchWaves == uint32_t(kScanWaves) && kIvfBatchChunk == uint32_t(kWave), "a chunk is one entry per lane of a wavefront");

// what the scan reads of the lists, next to ScanParams (rows, queries, kk, the partial lists)
struct ListsParams {
	const uint32_t* probe;       // [nq][nprobe] list ids of the coarse search (entries past a query's count are never read)
	const uint32_t* cum;         // [nq][nprobe + 1] running chunk counts
	const uint64_t* list_off;    // [nlist + 1]
	const uint32_t* list_rows;   // rows of the lists back to back
	uint32_t nprobe;
};

// ---- running chunk counts: one wavefront per query, lane l owns probe slots l and 64 + l
constexpr int kOffsetsThreads = 256;
__global__ __launch_bounds__(kOffsetsThreads) void ivf_batch_offsets(const uint32_t* __restrict__ probe, const uint32_t* __restrict__ probe_cnt,
																	   const uint64_t* __restrict__ list_off, uint32_t nprobe, uint32_t nq,
																	   uint32_t* __restrict__ cum, unsigned long long* __restrict__ scanned) {
	const int lane = threadIdx.x & 63;
	const uint32_t q = blockIdx.x * (kOffsetsThreads / kWave) + (threadIdx.x >> 6);
	if (q >= nq) return;   // wavefront-uniform
	uint32_t cnt = probe_cnt[q];
	cnt = cnt < nprobe ? cnt : nprobe;
	uint32_t ch[2];
	unsigned long long rows = 0;
#pragma unroll
	for (int h = 0; h < 2; ++h) {
		const uint32_t s = uint32_t(h) * 64 + lane;
		ch[h] = 0;
		if (s < cnt) {
			const uint32_t l = probe[size_t(q) * nprobe + s];
			const uint64_t len = list_off[l + 1] - list_off[l];
			ch[h] = ivf_batch_list_chunks(len);
			rows += len;
		}
	}
	// inclusive prefix over the 64 lanes of each half; the second half starts at the first half's total
	uint32_t in0 = ch[0], in1 = ch[1];
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const uint32_t u0 = __shfl_up(in0, o), u1 = __shfl_up(in1, o);
		if (lane >= o) {
			in0 += u0;
			in1 += u1;
		}
	}
	const uint32_t half = __shfl(in0, 63);
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) rows += __shfl_xor(rows, o);
	uint32_t* out = cum + size_t(q) * (nprobe + 1);
	if (lane == 0) {
		out[0] = 0;
		scanned[q] = rows;
	}
	if (uint32_t(lane) < nprobe) out[1 + lane] = in0;
	if (64u + lane < nprobe) out[65 + lane] = half + in1;
}

// Rows of this wave's step -> candidate insertion, for rows that arrive in ANY order (consider_quad of knn_scan.hip counts on ascending rows:
// there a tie with the current worst never enters; here an equal distance with a smaller row does, so the pre-test lets equal distances through
// and admits() decides by (dist, row)).  `dist` is replicated over each 16-lane group.
template <typename TK>
__device__ __forceinline__ void consider_quad_any_order(TK& top, float dist, uint32_t row, bool valid, int lane) {
	const bool pass = valid && (top.filled < top.kk || dist <= top.thr_d);
	uint64_t pm = __ballot(pass) & 0x0001000100010001ull;   // one representative lane per group
	while (pm) {
		const int src = __builtin_ctzll(pm);
		pm &= pm - 1;
		const float d = __shfl(dist, src);
		const uint32_t i = __shfl(row, src);
		if (top.admits(d, i)) top.insert(d, i, lane);
	}
}

// the query's probed lists in LDS: running chunk counts, and per slot with chunks the list's first entry and its length
struct ListsLds {
	uint32_t cum[kIvfBatchMaxProbe + 1];
	uint32_t len[kIvfBatchMaxProbe];
	uint64_t base[kIvfBatchMaxProbe];
};
__device__ __forceinline__ void load_lists(ListsLds& s, const ListsParams& lp, uint32_t q) {
	const uint32_t* cum = lp.cum + size_t(q) * (lp.nprobe + 1);
	for (uint32_t t = threadIdx.x; t <= lp.nprobe; t += kScanThreads) s.cum[t] = cum[t];
	for (uint32_t t = threadIdx.x; t < lp.nprobe; t += kScanThreads) {
		uint64_t b = 0;
		uint32_t n = 0;
		if (cum[t + 1] != cum[t]) {   // a slot without chunks (an empty list, a slot past the query's count) is never mapped to: its id is not read
			const uint32_t l = lp.probe[size_t(q) * lp.nprobe + t];
			b = lp.list_off[l];
			n = uint32_t(lp.list_off[l + 1] - b);
		}
		s.base[t] = b;
		s.len[t] = n;
	}
	__syncthreads();
}
// one chunk of the concatenation: its ids (one per lane, entries past the list's end re-read the list's last) and the entries it holds
struct ChunkIds {
	uint32_t id;
	uint32_t left;   // entries of the list from the chunk's first on (>= 1); the chunk holds min(left, 64)
};
__device__ __forceinline__ ChunkIds load_chunk(const ListsLds& s, const ListsParams& lp, uint32_t chunk, uint32_t nchunks, int lane) {
	const uint32_t cc = chunk < nchunks ? chunk : nchunks - 1;   // clamped: reading past the end re-reads the last chunk
	const IvfBatchChunkAt at = ivf_batch_chunk_at(s.cum, lp.nprobe, cc);
	const uint32_t len = s.len[at.slot];
	const uint32_t item = at.offset + uint32_t(lane);
	ChunkIds c;
	c.id = lp.list_rows[s.base[at.slot] + (item < len ? item : len - 1)];
	c.left = len - at.offset;
	return c;
}

// dim == 64 * NB: query block in LDS, double-buffered row loads (knn_scan_subset's step order across chunk boundaries)
template <int kMetric, int NB, typename TK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_lists(ScanParams p, ListsParams lp) {
	__shared__ float4 s_q[NB * 16];
	__shared__ ListsLds s_l;
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float4* qg = reinterpret_cast<const float4*>(p.queries + size_t(blockIdx.y) * p.dim);
	for (int i = threadIdx.x; i < NB * 16; i += kScanThreads) s_q[i] = qg[i];
	load_lists(s_l, lp, blockIdx.y);   // (ends with the barrier)

	TK top;
	top.init(p.kk);

	constexpr int kSteps = int(kIvfBatchChunk) / kRowsPerWave;
	const uint32_t nchunks = s_l.cum[lp.nprobe];
	const uint32_t nwaves = gridDim.x * kScanWaves;
	const uint32_t first = blockIdx.x * kScanWaves + wave;

	auto issue = [&](float4 (&x)[NB], uint32_t row) {
		const float4* rp = reinterpret_cast<const float4*>(p.rows + uint64_t(row) * p.stride) + m;
#pragma unroll
		for (int t = 0; t < NB; ++t) x[t] = load_row4<true>(rp + 16 * t);
	};
	auto reduce = [&](const float4 (&x)[NB], bool valid, uint32_t row) {
		float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
		for (int t = 0; t < NB; ++t) chain_step<kMetric>(acc, s_q[16 * t + m], x[t]);
		const float sum = fold_chains<false>(acc, nullptr, nullptr, 0, m) + 0.0f;
		const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, row);
		consider_quad_any_order(top, dist, row, valid, lane);
	};

	if (first < nchunks) {
		float4 xa[NB], xb[NB];
		ChunkIds cur = load_chunk(s_l, lp, first, nchunks, lane);
		issue(xa, __shfl(cur.id, g));
		for (uint32_t chunk = first; chunk < nchunks; chunk += nwaves) {
			const ChunkIds nxt = load_chunk(s_l, lp, chunk + nwaves, nchunks, lane);   // in flight while this chunk's steps run
			const int steps = cur.left >= kIvfBatchChunk ? kSteps : int((cur.left + kRowsPerWave - 1) / kRowsPerWave);   // a short list ends early
#pragma unroll 1
			for (int t = 0; t < steps; t += 2) {
				const uint32_t ra = __shfl(cur.id, t * kRowsPerWave + g);
				const uint32_t rb = __shfl(cur.id, ((t + 1) & (kSteps - 1)) * kRowsPerWave + g);
				issue(xb, rb);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xa, uint32_t(t * kRowsPerWave + g) < cur.left, ra);
				__builtin_amdgcn_sched_barrier(0);
				// step t + 2 of this chunk, or step 0 of this wave's next chunk (harmless re-read after the last one)
				const uint32_t rn = t + 2 < steps ? __shfl(cur.id, (t + 2) * kRowsPerWave + g) : __shfl(nxt.id, g);
				issue(xa, rn);
				__builtin_amdgcn_sched_barrier(0);
				reduce(xb, t + 1 < steps && uint32_t((t + 1) * kRowsPerWave + g) < cur.left, rb);
				__builtin_amdgcn_sched_barrier(0);
			}
			cur = nxt;
		}
	}
	block_merge_and_store(top, p, lane, wave);   // a workgroup without a chunk stores an empty list: the merge reads every slot
}

// Any dim: one list entry per 16-lane group and step, the query read through the caches
template <int kMetric, typename TK>
__global__ __launch_bounds__(kScanThreads) void knn_scan_lists_generic(ScanParams p, ListsParams lp) {
	__shared__ ListsLds s_l;
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const float* q = p.queries + size_t(blockIdx.y) * p.dim;
	load_lists(s_l, lp, blockIdx.y);
	TK top;
	top.init(p.kk);
	constexpr int kSteps = int(kIvfBatchChunk) / kRowsPerWave;
	const uint32_t nchunks = s_l.cum[lp.nprobe];
	const uint32_t nwaves = gridDim.x * kScanWaves;
	for (uint32_t chunk = blockIdx.x * kScanWaves + wave; chunk < nchunks; chunk += nwaves) {
		const ChunkIds cur = load_chunk(s_l, lp, chunk, nchunks, lane);
		const int steps = cur.left >= kIvfBatchChunk ? kSteps : int((cur.left + kRowsPerWave - 1) / kRowsPerWave);
#pragma unroll 1
		for (int t = 0; t < steps; ++t) {
			const uint32_t row = __shfl(cur.id, t * kRowsPerWave + g);   // clamped inside the list: a real row
			const float sum = group_distance_generic<kMetric>(p.rows + uint64_t(row) * p.stride, q, p.dim, m);
			const float dist = metric_epilogue<kMetric>(sum, p.inv_norms, row);
			consider_quad_any_order(top, dist, row, uint32_t(t * kRowsPerWave + g) < cur.left, lane);
		}
	}
	block_merge_and_store(top, p, lane, wave);
}

// ------------------------------------------------------------------------------------------ launchers

void launch_ivf_batch_offsets(const uint32_t* probe, const uint32_t* probe_cnt, const uint64_t* list_off, uint32_t nprobe, uint32_t nq, uint32_t* cum,
							  unsigned long long* scanned, hipStream_t s) {
	const uint32_t per = kOffsetsThreads / kWave;
	hipLaunchKernelGGL(ivf_batch_offsets, dim3((nq + per - 1) / per), dim3(kOffsetsThreads), 0, s, probe, probe_cnt, list_off, nprobe, nq, cum, scanned);
}

// the dimensions launch_scan_subset (knn_scan.hip) gives to its fixed kernel take the fixed form here, every other the generic one
template <int kMetric, typename TK>
static void launch_scan_lists_tk(const ScanParams& p, const ListsParams& lp, dim3 grid, hipStream_t s) {
	const dim3 blk(kScanThreads);
	switch (p.dim) {
		case 128: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_lists<kMetric, 2, TK>), grid, blk, 0, s, p, lp); return; } break;
		case 256: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_lists<kMetric, 4, TK>), grid, blk, 0, s, p, lp); return; } break;
		case 512: hipLaunchKernelGGL((knn_scan_lists<kMetric, 8, TK>), grid, blk, 0, s, p, lp); return;
		case 768: hipLaunchKernelGGL((knn_scan_lists<kMetric, 12, TK>), grid, blk, 0, s, p, lp); return;
		case 1024: if constexpr (std::is_same_v<TK, WaveTopK>) { hipLaunchKernelGGL((knn_scan_lists<kMetric, 16, TK>), grid, blk, 0, s, p, lp); return; } break;
		default: break;
	}
	hipLaunchKernelGGL((knn_scan_lists_generic<kMetric, TK>), grid, blk, 0, s, p, lp);
}
template <int kMetric>
static void launch_scan_lists_metric(const ScanParams& p, const ListsParams& lp, dim3 grid, hipStream_t s) {
	if (ivf_batch_wide_list(p.kk)) {
		launch_scan_lists_tk<kMetric, WaveTopK2>(p, lp, grid, s);
	} else {
		launch_scan_lists_tk<kMetric, WaveTopK>(p, lp, grid, s);
	}
}
// p: rows, inv_norms, queries [nq][dim], stride, dim, kk <= 128, part_dist / part_row [nq][gridx][kk] (p.n unused); 1 <= nprobe <= 128
void launch_scan_lists(int metric, const ScanParams& p, const uint32_t* probe, const uint32_t* cum, const uint64_t* list_off, const uint32_t* list_rows,
					   uint32_t nprobe, uint32_t nq, uint32_t gridx, hipStream_t s) {
	const ListsParams lp{probe, cum, list_off, list_rows, nprobe};
	const dim3 grid(gridx, nq);
	switch (metric) {
		case kL2: launch_scan_lists_metric<kL2>(p, lp, grid, s); break;
		case kIP: launch_scan_lists_metric<kIP>(p, lp, grid, s); break;
		default: launch_scan_lists_metric<kCos>(p, lp, grid, s); break;
	}
}

}  // namespace rxgpu
