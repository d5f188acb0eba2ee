// The kernel choice of an HNSW search (reindexer_amd/csrc/hnsw_kernel_pick.h) compiled for the host: tests/test_hnsw_kernel_pick.py pins its
// rules on the CPU.  Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "hnsw_kernel_pick.h"

extern "C" {

// in: the fields of HnswPickInput in declaration order; which: 0 = search, 1 = helper, 2 = server; out: the pick, one 64-bit word a field in
// the order of FIELDS in the test, then whether the instantiation exists
void hnsw_pick_cpu(int which, const uint32_t* in, uint64_t* out) {
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
	const rxgpu::HnswKernelPick k = which == 0 ? rxgpu::pick_hnsw_search(i) : which == 1 ? rxgpu::pick_hnsw_helper(i) : rxgpu::pick_hnsw_server(i);
	bool exists = false;
	switch (k.family) {
		case rxgpu::kHnswSearch: exists = rxgpu::hnsw_search_kernel_exists(k.global_cand, k.nb, k.latency, k.sq8, k.sorted, k.del); break;
		case rxgpu::kHnswTeam: exists = rxgpu::hnsw_team_kernel_exists(k.nb, k.sorted, k.del) && k.team == 4; break;
		case rxgpu::kHnswHelper: exists = rxgpu::hnsw_helper_kernel_exists(k.nb, k.sq8); break;
		default: exists = rxgpu::hnsw_server_kernel_exists(k.nb, k.sq8, k.sorted, k.del) && (k.family == rxgpu::kHnswServerWide) == (!k.sq8 && k.nb > 12); break;
	}
	const uint64_t v[] = {uint64_t(k.family), uint64_t(k.nb), uint64_t(k.sorted), k.del, k.latency, k.sq8, k.global_cand, uint64_t(k.team), k.threads,
						  k.lds_bytes, k.vis_lds, k.vis_hash_log2, k.nbl_off, k.spec_off, k.needs_raised_lds, k.served, exists};
	for (uint64_t x : v) *out++ = x;
}

// the byte offsets of the dynamic LDS the kernels and the launchers share: candidate heap, query fragment, visited set
void hnsw_lds_layout_cpu(uint32_t ef_cap, uint32_t lds_cand_cap, int global_cand, int nb, int sq8, uint64_t* out) {
	const rxgpu::HnswLdsLayout l = rxgpu::hnsw_lds_layout(ef_cap, lds_cand_cap, global_cand != 0, nb, sq8 != 0);
	out[0] = l.cand_off();
	out[1] = l.query_off();
	out[2] = l.visited_off();
}

// the constants the pick shares with the kernels
void hnsw_pick_constants(uint32_t* out) {
	out[0] = rxgpu::kHnswNblBytes;
	out[1] = rxgpu::kHnswSpecBytes;
	out[2] = uint32_t(rxgpu::kHnswNblRows);
	out[3] = rxgpu::kHnswSpecLog2;
}
}
