// The kernel choice of a filtered HNSW search (reindexer_amd/csrc/hnsw_kernel_pick.h: HnswPickInput::filtered, pick_hnsw_filtered,
// hnsw_filtered_kernel_exists) compiled for the host: tests/test_hnsw_filtered_pick.py pins its rules on the CPU.  Test infrastructure only —
// nothing in the product links this.
#include <cstdint>

#include "hnsw_kernel_pick.h"

extern "C" {

// in: the fields of HnswPickInput in declaration order (`filtered` last); out: the pick, one 64-bit word a field in the order of FIELDS in the
// test, then whether the instantiation exists in its family's set
void hnsw_filtered_pick_cpu(const uint32_t* in, uint64_t* out) {
	rxgpu::HnswPickInput i{};
	i.dim = in[0];
	i.ef = in[1];
	i.ef_cap = in[2];
	i.lds_cand_cap = in[3];
	i.sorted = in[4] != 0;
	i.bare = in[5] != 0;
	i.sq8 = in[6] != 0;
	i.team = in[7];
	i.team_max = in[8];
	i.vis_lds = in[9];
	i.vis_lds_log2 = in[10];
	i.vis_hash_log2 = in[11];
	i.has_visited = in[12] != 0;
	i.sq8_query = in[13] != 0;
	i.nbl = in[14];
	i.spec = in[15];
	i.maxM0 = in[16];
	i.blocks = in[17];
	i.global_cand = in[18] != 0;
	i.filtered = in[19] != 0;
	const rxgpu::HnswKernelPick k = rxgpu::pick_hnsw_search(i);
	bool exists = false;
	switch (k.family) {
		case rxgpu::kHnswSearch: exists = rxgpu::hnsw_search_kernel_exists(k.global_cand, k.nb, k.latency, k.sq8, k.sorted, k.del); break;
		case rxgpu::kHnswTeam: exists = rxgpu::hnsw_team_kernel_exists(k.nb, k.sorted, k.del) && k.team == 4; break;
		case rxgpu::kHnswFiltered: exists = rxgpu::hnsw_filtered_kernel_exists(false, k.global_cand, k.nb, k.sq8, k.sorted, k.del) && !k.latency && k.team == 1; break;
		case rxgpu::kHnswFilteredTeam:
			exists = rxgpu::hnsw_filtered_kernel_exists(true, k.global_cand, k.nb, k.sq8, k.sorted, k.del) && k.latency && k.team == 4;
			break;
		default: break;
	}
	const uint64_t v[] = {uint64_t(k.family), uint64_t(k.nb), uint64_t(k.sorted), k.del, k.latency, k.sq8, k.global_cand, uint64_t(k.team), k.threads,
						  k.lds_bytes, k.vis_lds, k.vis_hash_log2, k.nbl_off, k.spec_off, k.needs_raised_lds, k.served, exists};
	for (uint64_t x : v) *out++ = x;
}

// the instantiation set of hnsw_filtered.hip as the pick header states it
int hnsw_filtered_exists_cpu(int team, int global_cand, int nb, int sq8, int sorted, int del) {
	return rxgpu::hnsw_filtered_kernel_exists(team != 0, global_cand != 0, nb, sq8 != 0, sorted, del != 0) ? 1 : 0;
}
}
