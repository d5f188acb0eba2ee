// The visited sets of the HNSW search: a bitset over the nodes or a hash set sized by ef, in HBM or in LDS.  Included by
// hnsw_search_core.hip.h.
#pragma once
#include "knn_kernels.hip.h"

namespace rxgpu {

// "Seen before?" of the reference's visited list (vl_type tags, hnswalg.h:904-931), as test-and-set.  Bitset: one atomicOr.  Hash set
// (HnswParams::vis_hash_log2): linear probing with compare-and-swap on node + 1; the neighbours a wavefront tests together are distinct
// nodes, two lanes can only meet on an EMPTY slot and the CAS settles that.  The table is at most half full (the callers check), so a probe
// sequence ends.  Its 32 KB stay in the L2 / Infinity Cache for the life of the search, where a bitset over 10M nodes (1.25 MB per
// search, 6 GB for the searches in flight) sends every test to HBM.
__device__ __forceinline__ bool hnsw_visit(uint32_t* visited, uint32_t hash_log2, uint32_t id) {
	if (hash_log2 == 0) {
		const uint32_t bit = 1u << (id & 31);
		return !(atomicOr(&visited[id >> 5], bit) & bit);
	}
	const uint32_t mask = (1u << hash_log2) - 1u, key = id + 1u;
	uint32_t h = (id * 2654435761u) >> (32u - hash_log2);
	for (;;) {
		const uint32_t old = atomicCAS(&visited[h], 0u, key);
		if (old == 0u) return true;
		if (old == key) return false;
		h = (h + 1u) & mask;
	}
}

// the latency form may keep the hash set in LDS (HnswParams::vis_lds): same probing, a ds_cmpst_rtn instead of a global atomic.  (Its own
// function, without the bitset branch: sharing hnsw_visit let the compiler merge the two bitset paths into ONE flat_atomic_or.)
__device__ __forceinline__ bool hnsw_visit_lds(uint32_t* table, uint32_t hash_log2, uint32_t id) {
	const uint32_t mask = (1u << hash_log2) - 1u, key = id + 1u;
	uint32_t h = (id * 2654435761u) >> (32u - hash_log2);
	for (;;) {
		const uint32_t old = atomicCAS(&table[h], 0u, key);
		if (old == 0u) return true;
		if (old == key) return false;
		h = (h + 1u) & mask;
	}
}
// "seen before?" WITHOUT the mark (the speculative distance batch of a team search looks ahead at a candidate's neighbours, but only the
// expansion itself may mark them)
__device__ __forceinline__ bool hnsw_seen(const uint32_t* visited, uint32_t hash_log2, uint32_t id) {
	if (hash_log2 == 0) return ((__hip_atomic_load(&visited[id >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (id & 31)) & 1u) != 0u;
	const uint32_t mask = (1u << hash_log2) - 1u, key = id + 1u;
	uint32_t h = (id * 2654435761u) >> (32u - hash_log2);
	for (;;) {
		const uint32_t v = __hip_atomic_load(&visited[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (v == key) return true;
		if (v == 0u) return false;
		h = (h + 1u) & mask;
	}
}
__device__ __forceinline__ bool hnsw_seen_lds(const uint32_t* table, uint32_t hash_log2, uint32_t id) {
	const uint32_t mask = (1u << hash_log2) - 1u, key = id + 1u;
	uint32_t h = (id * 2654435761u) >> (32u - hash_log2);
	for (;;) {
		const uint32_t v = table[h];
		if (v == key) return true;
		if (v == 0u) return false;
		h = (h + 1u) & mask;
	}
}
template <bool kLds>
__device__ __forceinline__ bool hnsw_visit_sel(uint32_t* visited, uint32_t* lds_vis, bool use_lds, uint32_t hash_log2, uint32_t id) {
	if constexpr (kLds) {
		if (use_lds) return hnsw_visit_lds(lds_vis, hash_log2, id);
	}
	return hnsw_visit(visited, hash_log2, id);
}

}  // namespace rxgpu
