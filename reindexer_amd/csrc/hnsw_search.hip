// HNSW search on gfx950: one wavefront per query, traversal IDENTICAL to the reference's.
//
// Replaces (cpp_src/core/index/float_vector/hnswlib/hnswalg.h): getLayer0EntryPoint :799-827, initLayer0SearchState :829-858,
// layer0ShouldStopBeforePop :860-869, runLayer0Step :871-963 (non-streaming), searchBaseLayerST :966-975, SearchKnn :1988-2012.
//
// Why the result can be *equal*, not just "recall-close": every distance is bit-identical to the CPU engine's
// (knn_kernels.hip.h), the graph is the same flat graph, and the two working heaps (PriorityQueue + CompareByFirst,
// priority_queue.h:7-152 / hnswalg.h:581-585) are replayed with the reference's sift mechanics, so ties break the same way.
// The best-first search is sequential per query; parallelism comes from
//   * lanes: the <=2M neighbours of the popped node are fetched/visited-tested one per lane, their distances computed
//     4 rows at a time (16 lanes per row, 16-byte loads), and
//   * queries: thousands of independent wavefronts in flight — the kernel is bound by random 3 KB row gathers from HBM.
// Per query state: candidate heap + result heap in LDS (heap updates by lane 0 in neighbour order), visited bitset in HBM
// (one atomicOr per neighbour is both the test and the mark).  A query whose candidate heap outgrows LDS is flagged and
// re-run with the heap in a global scratch (still on the GPU) — never on the CPU.
// Graphs without deleted nodes, ef <= 256, start differently: both queues as ONE sorted list in registers (HnswSortedList, hnsw_sorted_list.hip.h), and
// only a search in which equal distances could change what the reference's heaps do starts over on the heaps, inside the same kernel.


#include "hnsw_dispatch.hip.h"
#include "hnsw_search_core.hip.h"

namespace rxgpu {

template <int kMetric, int NB, int kSorted, bool kDel, int kTeam>
__global__ __launch_bounds__(64 * kTeam) void hnsw_team_kernel(HnswParams p) {
	__shared__ HnswTeamBox box;
	const uint32_t slot = blockIdx.x;
	if (threadIdx.x < 64) {
		hnsw_search_one<kMetric, false, NB, true, false, kSorted, kDel, kTeam>(p, slot, p.only ? p.only[slot] : slot, &box);
		if (threadIdx.x == 0) box.cnt = -1;
		__syncthreads();
	} else {
		hnsw_team_serve<kMetric, NB, kTeam>(p, &box);
	}
}

// (wavefronts per SIMD asked for: five of the D = 768 headline form, four of every throughput form over rows of 1024 and 1536 floats — the
// chunked distance batch leaves the registers for it, and without the bound the allocation lands a few registers above 128)
template <int kMetric, bool kGlobalCand, int NB, bool kLatency, bool kSq8 = false, int kSorted = 0, bool kDel = false>
__global__ __launch_bounds__(64, (kSorted == 2 && !kDel && !kLatency && !kSq8 && NB == 12) ? 5 : (!kLatency && !kSq8 && NB > 12) ? 4 : 1) void hnsw_search_kernel(HnswParams p) {
	const uint32_t slot = blockIdx.x;
	hnsw_search_one<kMetric, kGlobalCand, NB, kLatency, kSq8, kSorted, kDel>(p, slot, p.only ? p.only[slot] : slot);
	if (p.helper_n) {   // a batch with helper workgroups: this search has ended, and what it queued for them is visible
		__threadfence();
		if (threadIdx.x == 0) atomicAdd(p.helper_n + 2, 1u);
	}
}

// Helper workgroups of a batch: workgroup w serves entries w, w + G, ... of the overflow queue until the stop word is set (a 4-byte memset
// behind the batch's last launch) and its next entry does not exist.  Every search runs on the heap kernel's code with the largest LDS heap
// and the workgroup's own bitset (zeroed here); a search that overflows again keeps kHnswOverflow for the host's global-heap tiers.  A
// wall-clock limit remains as the last resort; the end of the batch itself is a count of finished searches in device memory (HnswHelper::
// finished), which needs no memset or signal to get through a queue the helper may share.
template <int kMetric, int NB, bool kSq8>
__global__ __launch_bounds__(64) void hnsw_helper_kernel(HnswParams p, HnswHelper hq) {
	const uint32_t w = blockIdx.x, G = gridDim.x;
	const int lane = threadIdx.x;
	const unsigned long long t0 = wall_clock64();
	uint4* bits = reinterpret_cast<uint4*>(p.visited + size_t(w) * p.visited_words);
	for (uint32_t s = w; s < hq.cap; s += G) {
		uint32_t id1 = 0;
		for (;;) {
			id1 = __hip_atomic_load(&hq.ids[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
			if (id1) break;
			if (__hip_atomic_load(hq.stop, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) ||
				__hip_atomic_load(hq.finished, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= hq.expected) {   // the batch is over: the queue is final
				const uint32_t n = __hip_atomic_load(hq.n, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
				if (s >= n) return;
				id1 = __hip_atomic_load(&hq.ids[s], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
				if (id1) break;
			}
			if (wall_clock64() - t0 > hq.ticks_limit) return;
			__builtin_amdgcn_s_sleep(100);
		}
		id1 = uint32_t(__builtin_amdgcn_readfirstlane(int(id1)));
		for (uint64_t i = lane; i < p.visited_words / 4; i += 64) bits[i] = make_uint4(0u, 0u, 0u, 0u);   // (visited_words is padded to 4)
		__threadfence();
		__syncthreads();
		hnsw_search_one<kMetric, false, NB, (NB > 8 && !kSq8), kSq8, 0, false>(p, w, id1 - 1u);
		__syncthreads();
	}
}

// From a pick to the instantiation (hnsw_kernel_pick.h states which ones exist: nothing outside that set is compiled, and a pick outside it
// launches nothing).
static bool dispatch_hnsw_search(int metric, const HnswKernelPick& k, const HnswParams& p, uint32_t blocks, hipStream_t s) {
	return with_metric(metric, [&](auto m) {
		return with_int<0, 2, 6, 8, 12, 16, 24>(k.nb, [&](auto nb) {
			return with_int<0, 2, 3, 4>(k.sorted, [&](auto sorted) {
				return with_bool(k.del, [&](auto del) {
					constexpr int M = decltype(m)::value, NB = decltype(nb)::value, S = decltype(sorted)::value;
					constexpr bool D = decltype(del)::value;
					if (k.family == kHnswTeam) {
						if constexpr (hnsw_team_kernel_exists(NB, S, D)) return hnsw_launch<&hnsw_team_kernel<M, NB, S, D, 4>>(k, blocks, s, p);
						return false;
					}
					return with_bool(k.global_cand, [&](auto global_cand) {
						return with_bool(k.latency, [&](auto latency) {
							return with_bool(k.sq8, [&](auto sq8) {
								constexpr bool G = decltype(global_cand)::value, L = decltype(latency)::value, Q = decltype(sq8)::value;
								if constexpr (hnsw_search_kernel_exists(G, NB, L, Q, S, D)) return hnsw_launch<&hnsw_search_kernel<M, G, NB, L, Q, S, D>>(k, blocks, s, p);
								return false;
							});
						});
					});
				});
			});
		});
	});
}

void launch_hnsw_search(int metric, const HnswParams& p, uint32_t blocks, bool global_cand, hipStream_t s) {
	const HnswKernelPick k = pick_hnsw_search(hnsw_pick_input(p, blocks, global_cand));
	if (!dispatch_hnsw_search(metric, k, hnsw_patched(p, k), blocks, s)) hnsw_no_kernel("search", metric, k);
}

// the helper workgroups of a batch (hnsw_helper_kernel): p = the batch's parameters with the helpers' own visited bitsets, the largest LDS
// heap, no `only` list, no overflow queue of their own
void launch_hnsw_helper(int metric, const HnswParams& p, const HnswHelper& hq, uint32_t groups, hipStream_t s) {
	const HnswKernelPick k = pick_hnsw_helper(hnsw_pick_input(p, groups, false));
	const HnswParams pk = hnsw_patched(p, k);
	const bool launched = with_metric(metric, [&](auto m) {
		return with_int<0, 2, 12, 16, 24>(k.nb, [&](auto nb) {
			return with_bool(k.sq8, [&](auto sq8) {
				constexpr int M = decltype(m)::value, NB = decltype(nb)::value;
				constexpr bool Q = decltype(sq8)::value;
				if constexpr (hnsw_helper_kernel_exists(NB, Q)) return hnsw_launch<&hnsw_helper_kernel<M, NB, Q>>(k, groups, s, pk, hq);
				return false;
			});
		});
	});
	if (!launched) hnsw_no_kernel("helper", metric, k);
}


// SearchRange's second half on the device (hnswalg.h:2030-2064): the closure of the ef-search's hits under "neighbour on level 0, not
// deleted, dist < radius".  The result is a SET (the reference's radius_queue order does not change it), so the expansion runs level by
// level: one workgroup of 16 wavefronts, every wavefront takes frontier nodes — the node's list block in one round, test-and-mark on a
// fresh visited bitset (atomicOr; the reference starts a new visited list too: only the ef hits are marked), distances of the fresh
// neighbours 4 rows per step — and appends what lies inside the radius to the result and to the next frontier.
constexpr int kRangeThreads = 1024;
constexpr int kRangeWaves = kRangeThreads / 64;

template <int kMetric>
__global__ __launch_bounds__(kRangeThreads) void hnsw_range_kernel(HnswParams p, HnswRange r) {
	__shared__ uint32_t nb_id[kRangeWaves][kHnswMaxNeighbors];
	__shared__ float nb_d[kRangeWaves][kHnswMaxNeighbors];
	__shared__ uint32_t s_na, s_nb;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const bool sq8 = p.codes != nullptr;
	uint32_t* fa = r.frontier;
	uint32_t* fb = r.frontier + r.cap;
	if (tid == 0) {
		s_na = 0;
		s_nb = 0;
	}
	__syncthreads();
	// the ef hits: all marked visited, those inside the radius are results and the first frontier
	for (uint32_t i = tid; i < r.seed_n; i += kRangeThreads) {
		const uint32_t id = r.seed_row[i];
		const float d = r.seed_dist[i];
		atomicOr(&r.visited[id >> 5], 1u << (id & 31));
		if (d < r.radius) {
			const unsigned long long pos = atomicAdd(r.total, 1ull);
			if (pos < r.cap) {
				r.out_dist[pos] = d;
				r.out_row[pos] = id;
				fa[atomicAdd(&s_na, 1u)] = id;
			}
		}
	}
	__syncthreads();
	for (;;) {
		const uint32_t na = s_na;
		if (na == 0) break;
		for (uint32_t i = wave; i < na; i += kRangeWaves) {
			const uint32_t node = fa[i];
			const uint32_t* ll = p.links0 + size_t(node) * (1 + p.maxM0);
			int nfresh = 0, cnt = 0;
			for (int base = 0; base <= int(p.maxM0); base += 64) {
				const int w = base + lane;
				const uint32_t word = w <= int(p.maxM0) ? ll[w] : 0u;
				if (base == 0) cnt = int(__builtin_amdgcn_readfirstlane(word));
				if (base > cnt) break;   // uniform
				const int j = w - 1;
				bool fresh = false;
				if (j >= 0 && j < cnt && (p.bare || !p.deleted[word])) {   // IsMarkedDeleted first: a deleted neighbour is not even marked
					const uint32_t bit = 1u << (word & 31);
					fresh = !(atomicOr(&r.visited[word >> 5], bit) & bit);
				}
				const uint64_t fm = __ballot(fresh);
				if (fresh) nb_id[wave][nfresh + __popcll(fm & ((1ull << lane) - 1))] = word;
				nfresh += __popcll(fm);
			}
			__builtin_amdgcn_wave_barrier();
			if (sq8) {
				batch_distances_sq8<kMetric>(p, p.qcodes, p.qcorr[0], p.qnorm[0], nb_id[wave], nfresh, nb_d[wave], lane);
			} else {
				batch_distances<kMetric>(p, p.queries, nb_id[wave], nfresh, nb_d[wave], lane);
			}
			__builtin_amdgcn_wave_barrier();
			for (int j = lane; j < nfresh; j += 64) {
				const float d = nb_d[wave][j];
				if (d < r.radius) {
					const unsigned long long pos = atomicAdd(r.total, 1ull);
					if (pos < r.cap) {
						r.out_dist[pos] = d;
						r.out_row[pos] = nb_id[wave][j];
						fb[atomicAdd(&s_nb, 1u)] = nb_id[wave][j];   // at most cap entries ever enter a frontier: one per stored result
					}
				}
			}
			__builtin_amdgcn_wave_barrier();
		}
		__syncthreads();
		if (tid == 0) {
			s_na = s_nb;
			s_nb = 0;
		}
		uint32_t* t = fa;
		fa = fb;
		fb = t;
		__syncthreads();
	}
}

void launch_hnsw_range(int metric, const HnswParams& p, const HnswRange& r, hipStream_t s) {
	switch (metric) {
		case kL2: hipLaunchKernelGGL(hnsw_range_kernel<kL2>, dim3(1), dim3(kRangeThreads), 0, s, p, r); break;
		case kIP: hipLaunchKernelGGL(hnsw_range_kernel<kIP>, dim3(1), dim3(kRangeThreads), 0, s, p, r); break;
		default: hipLaunchKernelGGL(hnsw_range_kernel<kCos>, dim3(1), dim3(kRangeThreads), 0, s, p, r); break;
	}
}

// rxgpu_hnsw_patch_graph: a host insert (addPoint / updatePoint, hnswalg.h:1472-1852) rewrites the lists of the new element and of a few
// dozen neighbours; their staged copies are scattered into the resident graph instead of re-uploading all of it.
__global__ __launch_bounds__(64) void hnsw_patch_kernel(HnswPatch p) {
	const uint32_t j = blockIdx.x, lane = threadIdx.x;
	const uint32_t id = p.ids[j];
	const uint32_t stride0 = 1 + p.maxM0, stride = 1 + p.M;
	for (uint32_t w = lane; w < stride0; w += 64) p.links0[uint64_t(id) * stride0 + w] = p.src_links0[uint64_t(j) * stride0 + w];
	uint64_t at = p.upper_at[j];
	if (at == ~uint64_t(0)) {
		at = p.upper_off[id];
	} else if (lane == 0) {
		p.upper_off[id] = at;
	}
	const uint32_t words = uint32_t(p.levels[j]) * stride;
	for (uint32_t w = lane; w < words; w += 64) p.upper[at * stride + w] = p.src_upper[uint64_t(p.upper_src[j]) * stride + w];
	if (lane == 0) p.deleted[id] = p.src_deleted[j];
}

void launch_hnsw_patch(const HnswPatch& p, uint32_t n_dirty, hipStream_t s) {
	if (n_dirty) hipLaunchKernelGGL(hnsw_patch_kernel, dim3(n_dirty), dim3(64), 0, s, p);
}

}  // namespace rxgpu
