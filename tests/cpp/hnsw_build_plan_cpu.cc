// The decisions of the batched HNSW build on the device (reindexer_amd/csrc/hnsw_build_plan.h) compiled for the host:
// tests/test_hnsw_build_plan.py pins its rules on the CPU.  Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "hnsw_build_plan.h"

extern "C" {

// out = {seed, ratio, batch_cap} as the environment sets them
void hnsw_build_plan_knobs(uint64_t* out) {
	const rxgpu::HnswBuildKnobs k = rxgpu::read_hnsw_build_knobs();
	out[0] = k.seed;
	out[1] = k.ratio;
	out[2] = k.batch_cap;
}
uint64_t hnsw_build_plan_seed_rows(uint64_t linked, uint64_t n) { return rxgpu::hnsw_build_seed_rows(linked, n, rxgpu::read_hnsw_build_knobs()); }
uint64_t hnsw_build_plan_batch_rows(uint64_t a, uint64_t n) { return rxgpu::hnsw_build_batch_rows(a, n, rxgpu::read_hnsw_build_knobs()); }
int hnsw_build_plan_path(uint64_t deleted, uint32_t M, uint32_t efc, int sharded) { return rxgpu::hnsw_build_path(deleted, M, efc, sharded != 0); }
// out = {fixed bytes, row bytes, kept in LDS}
void hnsw_build_plan_lds(uint32_t row_stride, uint32_t M, uint32_t* out) {
	const rxgpu::HnswBuildLds l = rxgpu::hnsw_build_select_lds(row_stride, M);
	out[0] = l.fixed_bytes;
	out[1] = l.rows_bytes;
	out[2] = l.kept_in_lds ? 1 : 0;
}
// out = {pairs, o_cand_dist, o_cand_row, o_queries, o_pair_t, o_inc, o_touched, o_tcnt, o_tseg, over_cap, big_cap, o_over, o_big_id, o_big_dist,
//        o_big_pos, o_counters, bytes, node_bytes}
void hnsw_build_plan_scratch(uint64_t rows, uint32_t M, uint32_t max_m0, uint32_t k, uint32_t dim, int pack, uint64_t nodes_cap, uint64_t* out) {
	const rxgpu::HnswBuildScratch s = rxgpu::hnsw_build_scratch(rows, M, max_m0, k, dim, pack != 0, nodes_cap);
	const uint64_t v[18] = {s.pairs, s.o_cand_dist, s.o_cand_row, s.o_queries, s.o_pair_t, s.o_inc, s.o_touched, s.o_tcnt, s.o_tseg, s.over_cap, s.big_cap,
							s.o_over, s.o_big_id, s.o_big_dist, s.o_big_pos, s.o_counters, s.bytes, s.node_bytes};
	for (int i = 0; i < 18; ++i) out[i] = v[i];
}

}  // extern "C"
