// The batched level-0 build of an HNSW graph on the device (gfx950): what HierarchicalNSWImpl::addPoint does with the result of its
// construction search on level 0 — getNeighborsByHeuristic2 (hnswalg.h:977-1024) and mutuallyConnectNewElement (hnswalg.h:1042-1180) as
// host/hnsw_graph.cc restates them (selectNeighbors, connect) — for a whole batch of new rows at once.  The candidates come from the
// search kernels (hnsw_search.hip) over the graph as it was before the batch; the rule the batch follows is in hnsw_build_plan.h and DESIGN §8.
//
//   hnsw_build_select    one wavefront per new row i: distIds(i, c) of its candidates, selectNeighbors(C_i, M), the list of i in the order
//                        connect() writes it, and one (target, i) pair per link, counted per target
//   hnsw_build_segments  a segment of `inc` per touched target            } the pairs grouped by target
//   hnsw_build_scatter   the pairs into their segments                     }
//   hnsw_build_backlink  one wavefront per touched target t: its list + the incoming rows — appended (ascending) while they fit, else
//                        selectNeighbors(cur U inc, maxM0) on distIds(x, t), written as connect() writes a re-selected list
//
// Bits: a distance is the 64-chain sum of knn_kernels.hip.h (a 16-lane group owns a row) with HnswGraph::distIds' epilogue — 1.0f * s + 0 + 0,
// negated for inner product / cosine, cosine multiplied by the stored 1 / |v| of the FIRST argument and then of the second.  The sum itself
// does not depend on the argument order (squares of differences, commutative products), the two multiplications do.
// Order: selectNeighbors pops its candidates by ascending distance, the larger id first among equal distances (std::less on (-dist, id)); the
// written order is what a max-heap on the distance alone (ResultHeap<Pair, ByFirst>, host/rx_types.h) pops after the kept entries were
// pushed in the order they were kept — one lane replays that heap, sift for sift.
//
// Every loop is bounded by a count known at launch (k <= 256 candidates, lists of at most maxM0 <= 128 entries, the entries of a target:
// its incoming rows, counted before the launch); no workgroup waits for another.
#include <hip/hip_runtime.h>

#include "hnsw_build.h"
#include "hnsw_build_plan.h"
#include "knn_kernels.hip.h"

namespace rxgpu {

namespace {

constexpr int kBuildThreads = 64;            // one wavefront per workgroup
constexpr uint32_t kBuildMaxList = 128;      // maxM0 <= 128

struct BuildLds {
	uint32_t id[kHnswBuildEntries];
	float dist[kHnswBuildEntries];
	uint32_t order[kHnswBuildEntries];       // order[w] = the entry walked w-th
	uint32_t kept_id[kBuildMaxList];
	float kept_d[kBuildMaxList];
	uint32_t heap_id[kBuildMaxList];
	float heap_d[kBuildMaxList];
};
static_assert(sizeof(BuildLds) == hnsw_build_fixed_lds_bytes(), "hnsw_build_plan.h counts these arrays");

// HnswGraph::distIds(first, second) from the chains' sum
template <int kMetric>
__device__ __forceinline__ float dist_ids(const HnswBuildArgs& a, float sum, uint32_t first, uint32_t second) {
	if constexpr (kMetric == kL2) {
		return 1.0f * sum + 0.0f + 0.0f;
	} else {
		float d = -(1.0f * sum + 0.0f + 0.0f);
		if constexpr (kMetric == kCos) {
			d *= a.inv_norms[first];
			d *= a.inv_norms[second];
		}
		return d;
	}
}

// dist[e] = distIds(base, ids[e]) (kBaseFirst) or distIds(ids[e], base), four entries a step.  Every lane runs every step: the folds
// exchange between the 16 lanes of a group.
template <int kMetric, bool kBaseFirst>
__device__ __forceinline__ void entry_distances(const HnswBuildArgs& a, const float* base_row, uint32_t base, const uint32_t* ids, float* dist, uint32_t n_e,
												int lane) {
	const int m = lane & 15, g = lane >> 4;
	for (uint32_t e0 = 0; e0 < n_e; e0 += kRowsPerWave) {
		const uint32_t e = e0 + uint32_t(g);
		const bool ok = e < n_e;
		const uint32_t id = ids[ok ? e : e0];
		const float sum = group_distance_generic<kMetric>(a.rows + uint64_t(id) * a.stride, base_row, a.dim, m);
		const float d = kBaseFirst ? dist_ids<kMetric>(a, sum, base, id) : dist_ids<kMetric>(a, sum, id, base);
		if (ok && m == 0) dist[e] = d;
	}
}

// The order selectNeighbors walks the entries in: ascending distance, the larger id first among equal distances.  Ids are distinct, so the
// rank of an entry is the number of entries in front of it.  (Distances that do not order — NaN, outside the contract — can give two
// entries one rank: every slot holds a valid entry all the same.)
__device__ __forceinline__ void walk_order(const uint32_t* ids, const float* dist, uint32_t* order, uint32_t n_e, int lane) {
	for (uint32_t e = lane; e < n_e; e += kBuildThreads) order[e] = e;
	__syncthreads();
	for (uint32_t e = lane; e < n_e; e += kBuildThreads) {
		const float de = dist[e];
		const uint32_t ie = ids[e];
		uint32_t rank = 0;
		for (uint32_t f = 0; f < n_e; ++f) {
			const float df = dist[f];
			rank += (df < de || (!(de < df) && ids[f] > ie)) ? 1u : 0u;
		}
		order[rank] = e;
	}
	__syncthreads();
}

// selectNeighbors(entries, limit): everything when there are fewer than `limit`; else closest first, an entry is kept unless some kept s has
// distIds(s, c) < its own distance, until `limit` are kept.  Returns the number kept (kept_id / kept_d in the order they were kept).
// kLdsRows: the kept rows are copied into lds_rows (slot 1 + index; slot 0 is the caller's) and read from there.
template <int kMetric, bool kLdsRows>
__device__ __forceinline__ uint32_t select_walk(const HnswBuildArgs& a, const uint32_t* ids, const float* dist, const uint32_t* order, uint32_t n_e,
												uint32_t limit, uint32_t* kept_id, float* kept_d, float* lds_rows, int lane) {
	if (n_e < limit) {
		for (uint32_t w = lane; w < n_e; w += kBuildThreads) {
			const uint32_t e = order[w];
			kept_id[w] = ids[e];
			kept_d[w] = dist[e];
		}
		__syncthreads();
		return n_e;
	}
	const int m = lane & 15, g = lane >> 4;
	uint32_t kept_n = 0;
	for (uint32_t w = 0; w < n_e && kept_n < limit; ++w) {
		const uint32_t e = order[w];
		const uint32_t c = ids[e];
		const float dc = dist[e];
		const float* c_row = a.rows + uint64_t(c) * a.stride;
		bool good = true;
		for (uint32_t s0 = 0; s0 < kept_n; s0 += kRowsPerWave) {
			const uint32_t s = s0 + uint32_t(g);
			const bool ok = s < kept_n;
			const uint32_t si = ok ? s : s0;
			const uint32_t sid = kept_id[si];
			const float* s_row = kLdsRows ? lds_rows + size_t(1 + si) * a.stride : a.rows + uint64_t(sid) * a.stride;
			const float sum = group_distance_generic<kMetric>(s_row, c_row, a.dim, m);
			const float d = dist_ids<kMetric>(a, sum, sid, c);
			if (__ballot(ok && d < dc) != 0) {
				good = false;
				break;
			}
		}
		if (good) {
			if constexpr (kLdsRows) {
				float4* dst = reinterpret_cast<float4*>(lds_rows + size_t(1 + kept_n) * a.stride);
				const float4* src = reinterpret_cast<const float4*>(c_row);
				for (uint32_t q = lane; q < a.stride / 4; q += kBuildThreads) dst[q] = src[q];
			}
			if (lane == 0) {
				kept_id[kept_n] = c;
				kept_d[kept_n] = dc;
			}
			++kept_n;
			__syncthreads();
		}
	}
	return kept_n;
}

// The order connect() writes a list in: the kept entries pushed into ResultHeap<Pair, ByFirst> one after the other, then popped.  One lane;
// the result replaces kept_id[0 .. kept_n).
__device__ __forceinline__ void heap_order(uint32_t* kept_id, const float* kept_d, uint32_t kept_n, uint32_t* hid, float* hd) {
	uint32_t n = 0;
	for (uint32_t j = 0; j < kept_n; ++j) {   // emplace: bubbleUp
		uint32_t i = n++;
		hd[i] = kept_d[j];
		hid[i] = kept_id[j];
		while (i) {
			const uint32_t up = (i - 1) >> 1;
			if (!(hd[up] < hd[i])) break;
			const float td = hd[up];
			const uint32_t ti = hid[up];
			hd[up] = hd[i];
			hid[up] = hid[i];
			hd[i] = td;
			hid[i] = ti;
			i = up;
		}
	}
	uint32_t out = 0;
	while (n) {   // top, pop: sinkDown
		kept_id[out++] = hid[0];
		--n;
		hd[0] = hd[n];
		hid[0] = hid[n];
		uint32_t i = 0;
		for (;;) {
			uint32_t big = i;
			const uint32_t l = 2 * i + 1, r = l + 1;
			if (l < n && hd[big] < hd[l]) big = l;
			if (r < n && hd[big] < hd[r]) big = r;
			if (big == i) break;
			const float td = hd[big];
			const uint32_t ti = hid[big];
			hd[big] = hd[i];
			hid[big] = hid[i];
			hd[i] = td;
			hid[i] = ti;
			i = big;
		}
	}
}

// a list row: count, the links, unused slots 0
__device__ __forceinline__ void write_list(uint32_t* row, const uint32_t* links, uint32_t count, uint32_t max_m0, int lane) {
	for (uint32_t w = lane; w < 1 + max_m0; w += kBuildThreads) row[w] = w == 0 ? count : (w - 1 < count ? links[w - 1] : 0u);
}

template <int kMetric, bool kLdsRows>
__global__ __launch_bounds__(kBuildThreads) void hnsw_build_select(HnswBuildArgs a) {
	__shared__ BuildLds L;
	extern __shared__ float4 build_rows4[];
	float* lds_rows = reinterpret_cast<float*>(build_rows4);
	const int lane = threadIdx.x;
	const uint32_t r = blockIdx.x;
	const uint32_t i = a.row_ids ? a.row_ids[r] : a.first + r;
	// the candidates the search left: nodes of the graph before the batch
	const uint32_t k = min(a.k, kHnswBuildEntries);
	uint32_t n_c = 0;
	for (uint32_t c0 = 0; c0 < k; c0 += kBuildThreads) {
		const uint32_t c = c0 + lane;
		const uint32_t id = c < k ? a.cand_row[uint64_t(r) * a.k + c] : kInvalidRow;
		const bool ok = id < a.first;
		const uint64_t mask = __ballot(ok);
		if (ok) L.id[n_c + __popcll(mask & ((1ull << lane) - 1ull))] = id;
		n_c += __popcll(mask);
	}
	const float* base_row = a.rows + uint64_t(i) * a.stride;
	if constexpr (kLdsRows) {
		const float4* src = reinterpret_cast<const float4*>(base_row);
		for (uint32_t q = lane; q < a.stride / 4; q += kBuildThreads) build_rows4[q] = src[q];
		base_row = lds_rows;
	}
	__syncthreads();
	entry_distances<kMetric, true>(a, base_row, i, L.id, L.dist, n_c, lane);
	__syncthreads();
	walk_order(L.id, L.dist, L.order, n_c, lane);
	const uint32_t kept_n = select_walk<kMetric, kLdsRows>(a, L.id, L.dist, L.order, n_c, a.M, L.kept_id, L.kept_d, lds_rows, lane);
	__syncthreads();
	if (lane == 0) heap_order(L.kept_id, L.kept_d, kept_n, L.heap_id, L.heap_d);
	__syncthreads();
	write_list(a.links0 + uint64_t(i) * (1 + a.maxM0), L.kept_id, kept_n, a.maxM0, lane);
	// one pair per link; the first pair of a target puts it on the list of touched nodes
	for (uint32_t j = lane; j < a.M; j += kBuildThreads) {
		const uint32_t t = j < kept_n ? L.kept_id[j] : kInvalidRow;
		a.pair_t[uint64_t(r) * a.M + j] = t;
		if (t != kInvalidRow) {
			if (atomicAdd(&a.node_cnt[t], 1u) == 0u) a.touched[atomicAdd(&a.counters[kBuildCntTouched], 1u)] = t;
		}
	}
}

__global__ __launch_bounds__(256) void hnsw_build_segments(HnswBuildArgs a) {
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= a.counters[kBuildCntTouched]) return;
	const uint32_t t = a.touched[j];
	const uint32_t c = a.node_cnt[t];
	const uint32_t seg = atomicAdd(&a.counters[kBuildCntInc], c);
	a.tcnt[j] = c;
	a.tseg[j] = seg;
	a.node_seg[t] = seg;
}

// ... and counts node_cnt back down to zero: the array is clean for the next batch
__global__ __launch_bounds__(256) void hnsw_build_scatter(HnswBuildArgs a) {
	const uint64_t p = uint64_t(blockIdx.x) * 256u + threadIdx.x;
	if (p >= uint64_t(a.n) * a.M) return;
	const uint32_t t = a.pair_t[p];
	if (t == kInvalidRow) return;
	const uint32_t left = atomicSub(&a.node_cnt[t], 1u);
	const uint32_t r = uint32_t(p / a.M);
	a.inc[a.node_seg[t] + left - 1u] = a.row_ids ? a.row_ids[r] : a.first + r;
}

// kBig: the second launch, workgroup o finishes the o-th node the first one queued; its entries are ordered in the big arrays
template <int kMetric, bool kBig>
__global__ __launch_bounds__(kBuildThreads) void hnsw_build_backlink(HnswBuildArgs a) {
	__shared__ BuildLds L;
	const int lane = threadIdx.x;
	uint32_t j = blockIdx.x, big_off = 0;
	if constexpr (kBig) {
		const uint2 o = a.over[blockIdx.x];
		j = o.x;
		big_off = o.y;
	} else {
		if (j >= a.counters[kBuildCntTouched]) return;
	}
	const uint32_t t = a.touched[j], c = a.tcnt[j], seg = a.tseg[j];
	uint32_t* row = a.links0 + uint64_t(t) * (1 + a.maxM0);
	const uint32_t m0 = min(row[0], a.maxM0);
	if (m0 + c <= a.maxM0) {   // room for every incoming row: appended, ascending
		if constexpr (!kBig) {
			for (uint32_t e = lane; e < c; e += kBuildThreads) L.id[e] = a.inc[seg + e];
			__syncthreads();
			for (uint32_t e = lane; e < c; e += kBuildThreads) {
				const uint32_t ie = L.id[e];
				uint32_t rank = 0;
				for (uint32_t f = 0; f < c; ++f) rank += L.id[f] < ie ? 1u : 0u;
				row[1 + m0 + rank] = ie;
			}
			if (lane == 0) row[0] = m0 + c;
		}
		return;
	}
	const uint32_t n_e = m0 + c;
	if constexpr (!kBig) {
		if (n_e > kHnswBuildEntries) {   // more than this wavefront orders in LDS: queued for the second launch, the list untouched
			if (lane == 0) {
				const uint32_t o = atomicAdd(&a.counters[kBuildCntOver], 1u);
				const uint32_t off = atomicAdd(&a.counters[kBuildCntBig], n_e);
				if (o < a.over_cap && uint64_t(off) + n_e <= a.big_cap) {
					a.over[o] = make_uint2(j, off);
				} else {
					atomicExch(&a.counters[kBuildCntError], 1u);
				}
			}
			return;
		}
	}
	uint32_t* ids = kBig ? a.big_id + big_off : L.id;
	float* dist = kBig ? a.big_dist + big_off : L.dist;
	uint32_t* order = kBig ? a.big_pos + big_off : L.order;
	// An id past the batch can only come from a corrupt list: it is reported (the call fails) and, so that nothing is read out of bounds
	// on the way there, replaced by the batch's last row.
	const uint32_t last = a.id_end - 1u;
	for (uint32_t e = lane; e < n_e; e += kBuildThreads) {
		uint32_t id = e < m0 ? row[1 + e] : a.inc[seg + e - m0];
		if (id > last) {
			atomicExch(&a.counters[kBuildCntError], 2u);
			id = last;
		}
		ids[e] = id;
	}
	if (lane == 0) atomicAdd(&a.counters[kBuildCntReselected], 1u);
	__syncthreads();
	entry_distances<kMetric, false>(a, a.rows + uint64_t(t) * a.stride, t, ids, dist, n_e, lane);
	__syncthreads();
	walk_order(ids, dist, order, n_e, lane);
	const uint32_t kept_n = select_walk<kMetric, false>(a, ids, dist, order, n_e, a.maxM0, L.kept_id, L.kept_d, nullptr, lane);
	__syncthreads();
	if (lane == 0) heap_order(L.kept_id, L.kept_d, kept_n, L.heap_id, L.heap_d);
	__syncthreads();
	write_list(row, L.kept_id, kept_n, a.maxM0, lane);
}

__global__ __launch_bounds__(64) void hnsw_build_patch_upper(HnswUpperPatch p) {
	const uint32_t j = blockIdx.x, lane = threadIdx.x;
	const uint32_t id = p.ids[j];
	const uint32_t stride = 1 + p.M;
	uint64_t at = p.upper_at[j];
	if (at == ~uint64_t(0)) {
		at = p.upper_off[id];
	} else if (lane == 0) {
		p.upper_off[id] = at;
	}
	const uint32_t lv = uint32_t(p.levels[j]);
	const uint32_t words = lv > p.skip ? (lv - p.skip) * stride : 0u;   // the staged blocks are the levels past `skip`
	for (uint32_t w = lane; w < words; w += 64) p.upper[(at + p.skip) * stride + w] = p.src_upper[uint64_t(p.upper_src[j]) * stride + w];
}

template <bool kLdsRows>
void launch_select(int metric, const HnswBuildArgs& a, size_t lds, hipStream_t s) {
	if (metric == kL2) {
		hipLaunchKernelGGL((hnsw_build_select<kL2, kLdsRows>), dim3(a.n), dim3(kBuildThreads), lds, s, a);
	} else if (metric == kIP) {
		hipLaunchKernelGGL((hnsw_build_select<kIP, kLdsRows>), dim3(a.n), dim3(kBuildThreads), lds, s, a);
	} else {
		hipLaunchKernelGGL((hnsw_build_select<kCos, kLdsRows>), dim3(a.n), dim3(kBuildThreads), lds, s, a);
	}
}

template <bool kBig>
void launch_backlink(int metric, const HnswBuildArgs& a, uint32_t grid, hipStream_t s) {
	if (metric == kL2) {
		hipLaunchKernelGGL((hnsw_build_backlink<kL2, kBig>), dim3(grid), dim3(kBuildThreads), 0, s, a);
	} else if (metric == kIP) {
		hipLaunchKernelGGL((hnsw_build_backlink<kIP, kBig>), dim3(grid), dim3(kBuildThreads), 0, s, a);
	} else {
		hipLaunchKernelGGL((hnsw_build_backlink<kCos, kBig>), dim3(grid), dim3(kBuildThreads), 0, s, a);
	}
}

}  // namespace

void launch_hnsw_build_select(int metric, const HnswBuildArgs& a, hipStream_t s) {
	if (a.n == 0) return;
	if (a.lds_rows) {
		launch_select<true>(metric, a, size_t(a.M + 1) * a.stride * sizeof(float), s);
	} else {
		launch_select<false>(metric, a, 0, s);
	}
}

void launch_hnsw_build_group(const HnswBuildArgs& a, hipStream_t s) {
	const uint64_t pairs = uint64_t(a.n) * a.M;
	if (pairs == 0) return;
	const uint32_t grid = uint32_t((pairs + 255) / 256);
	hipLaunchKernelGGL(hnsw_build_segments, dim3(grid), dim3(256), 0, s, a);
	hipLaunchKernelGGL(hnsw_build_scatter, dim3(grid), dim3(256), 0, s, a);
}

void launch_hnsw_build_backlink(int metric, const HnswBuildArgs& a, hipStream_t s) {
	const uint64_t pairs = uint64_t(a.n) * a.M;   // an upper bound of the touched nodes: the count itself stays on the device
	if (pairs) launch_backlink<false>(metric, a, uint32_t(pairs), s);
}

void launch_hnsw_build_backlink_big(int metric, const HnswBuildArgs& a, uint32_t n_over, hipStream_t s) {
	if (n_over) launch_backlink<true>(metric, a, n_over, s);
}

void launch_hnsw_build_patch_upper(const HnswUpperPatch& p, uint32_t n_nodes, hipStream_t s) {
	if (n_nodes) hipLaunchKernelGGL(hnsw_build_patch_upper, dim3(n_nodes), dim3(64), 0, s, p);
}

}  // namespace rxgpu
