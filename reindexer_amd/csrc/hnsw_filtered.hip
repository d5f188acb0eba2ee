// HNSW search under an allowed-rows bitmap (`WHERE cond AND KNN(...)` on a graph index): the search of hnsw_search.hip with every node
// whose bit is clear hidden the way a deleted node is.
//
// The reference fork has no filter functor: its delete mark is the one way it expresses a node that is traversed but not returned
// (hnswalg.h:1982 picks the branch, runLayer0Step :871-963 keeps such a node in candidate_set and out of top_candidates, MarkDelete
// :1303-1339 sets the mark).  A filtered search is therefore DEFINED as the reference's SearchKnn after MarkDelete of every row that fails
// the condition, and computed as that: hnsw_search_one (hnsw_search_core.hip.h) with kFilter reads the call's bitmap in the four places
// that read the delete mark — the bit itself, one per node (N / 8 bytes per call in flight), never expanded into a byte array.
//
// A family of its own, in a unit of its own: the unfiltered kernels keep their names, their instantiation sets and their machine code.
// Instantiated: heaps in LDS and with global candidates, the lists with deleted nodes at 2 / 3 / 4 entries a lane; floats and codes with
// the generic distance batch and the fixed ones for 128 and 768 components; the four-wavefront team for floats at 128 and 768 (the
// planner's call is one query).  No resident form, no helper workgroups, no range closure, no streaming form.
#include "hnsw_dispatch.hip.h"
#include "hnsw_search_core.hip.h"

namespace rxgpu {

template <int kMetric, int NB, int kSorted>
__global__ __launch_bounds__(256) void hnsw_filtered_team_kernel(HnswFilteredParams p) {
	__shared__ HnswTeamBox box;
	const uint32_t slot = blockIdx.x;
	if (threadIdx.x < 64) {
		hnsw_search_one<kMetric, false, NB, true, false, kSorted, true, 4, true>(p, slot, p.only ? p.only[slot] : slot, &box);
		if (threadIdx.x == 0) box.cnt = -1;
		__syncthreads();
	} else {
		hnsw_team_serve<kMetric, NB, 4>(p, &box);
	}
}

// kSorted == 0: the heaps (deleted and hidden nodes are theirs to handle: p.bare is 0 in every filtered call); else the list with deleted nodes
template <int kMetric, bool kGlobalCand, int NB, bool kSq8, int kSorted>
__global__ __launch_bounds__(64) void hnsw_filtered_kernel(HnswFilteredParams p) {
	const uint32_t slot = blockIdx.x;
	hnsw_search_one<kMetric, kGlobalCand, NB, false, kSq8, kSorted, (kSorted > 0), 1, true>(p, slot, p.only ? p.only[slot] : slot);
}

static bool dispatch_hnsw_filtered(int metric, const HnswKernelPick& k, const HnswFilteredParams& p, uint32_t blocks, hipStream_t s) {
	return with_metric(metric, [&](auto m) {
		return with_int<0, 2, 12>(k.nb, [&](auto nb) {
			return with_int<0, 2, 3, 4>(k.sorted, [&](auto sorted) {
				constexpr int M = decltype(m)::value, NB = decltype(nb)::value, S = decltype(sorted)::value;
				if (k.del != (S > 0) || k.latency != (k.family == kHnswFilteredTeam)) return false;
				if (k.family == kHnswFilteredTeam) {
					if constexpr (hnsw_filtered_kernel_exists(true, false, NB, false, S, S > 0)) {
						if (k.sq8 || k.global_cand || k.team != 4) return false;
						return hnsw_launch<&hnsw_filtered_team_kernel<M, NB, S>>(k, blocks, s, p);
					}
					return false;
				}
				return with_bool(k.global_cand, [&](auto global_cand) {
					return with_bool(k.sq8, [&](auto sq8) {
						constexpr bool G = decltype(global_cand)::value, Q = decltype(sq8)::value;
						if constexpr (hnsw_filtered_kernel_exists(false, G, NB, Q, S, S > 0)) return hnsw_launch<&hnsw_filtered_kernel<M, G, NB, Q, S>>(k, blocks, s, p);
						return false;
					});
				});
			});
		});
	});
}

void launch_hnsw_filtered(int metric, const HnswFilteredParams& p, uint32_t blocks, bool global_cand, hipStream_t s) {
	HnswPickInput in = hnsw_pick_input(p, blocks, global_cand);
	in.filtered = true;
	const HnswKernelPick k = pick_hnsw_search(in);
	HnswFilteredParams pk = p;
	static_cast<HnswParams&>(pk) = hnsw_patched(p, k);
	const bool ours = (k.family == kHnswFiltered || k.family == kHnswFilteredTeam) && p.allowed != nullptr && p.bare == 0;
	if (!ours || !dispatch_hnsw_filtered(metric, k, pk, blocks, s)) hnsw_no_kernel("filtered", metric, k);
}

}  // namespace rxgpu
