// The decisions of level 1 of the batched HNSW build on the device (reindexer_amd/csrc/hnsw_build_plan.h) compiled for the host:
// tests/test_hnsw_build_upper_plan.py pins its rules on the CPU.  Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "hnsw_build_plan.h"

extern "C" {

// RXGPU_HNSW_BUILD_UPPER as the environment sets it: 1 = device
int hnsw_build_upper_plan_variable() { return rxgpu::read_hnsw_build_upper_device() ? 1 : 0; }
int hnsw_build_upper_plan_on_device(int upper_device, int path, int top_level_before, uint64_t upper_rows) {
	return rxgpu::hnsw_build_upper_on_device(upper_device != 0, path, top_level_before, upper_rows) ? 1 : 0;
}
uint64_t hnsw_build_upper_plan_view_bytes(uint64_t nodes_cap, uint32_t M) { return rxgpu::hnsw_build_upper_view_bytes(nodes_cap, M); }
// out = the 18 words of the batch scratch in hnsw_build_plan_scratch's order (tests/cpp/hnsw_build_plan_cpu.cc), then {o_row_ids, bytes}
void hnsw_build_upper_plan_scratch(uint64_t up_rows, uint32_t M, uint32_t k, uint32_t dim, uint64_t nodes_cap, uint64_t* out) {
	const rxgpu::HnswBuildUpperScratch u = rxgpu::hnsw_build_upper_scratch(up_rows, M, k, dim, nodes_cap);
	const rxgpu::HnswBuildScratch& s = u.batch;
	const uint64_t v[20] = {s.pairs,	s.o_cand_dist, s.o_cand_row, s.o_queries,  s.o_pair_t,	 s.o_inc,	  s.o_touched, s.o_tcnt,	 s.o_tseg,	  s.over_cap,
							s.big_cap,	s.o_over,	   s.o_big_id,	 s.o_big_dist, s.o_big_pos, s.o_counters, s.bytes,	   s.node_bytes, u.o_row_ids, u.bytes};
	for (int i = 0; i < 20; ++i) out[i] = v[i];
}

}  // extern "C"
