// The decisions of IVF training on the device (reindexer_amd/csrc/ivf_train_plan.h) compiled for the host: tests/test_ivf_train_plan.py pins
// its rules on the CPU.  Test infrastructure only — nothing in the product links this.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ivf_train_plan.h"

extern "C" {

int ivf_plan_points_ok(uint64_t n) { return rxgpu::ivf_train_points_ok(n) ? 1 : 0; }
uint64_t ivf_plan_default_budget() { return rxgpu::kIvfGatherBudgetBytes; }
uint64_t ivf_plan_chunk_rows(uint64_t n, uint32_t dim, uint64_t budget) { return rxgpu::ivf_gather_chunk_rows(n, dim, budget); }
uint64_t ivf_plan_chunks(uint64_t n, uint64_t chunk_rows) { return rxgpu::ivf_gather_chunks(n, chunk_rows); }
// out = {first, rows}
void ivf_plan_chunk(uint64_t n, uint64_t chunk_rows, uint64_t i, uint64_t* out) {
	const rxgpu::IvfChunk c = rxgpu::ivf_gather_chunk(n, chunk_rows, i);
	out[0] = c.first;
	out[1] = c.rows;
}
// out = {blocks, span}
void ivf_plan_place_shape(uint64_t n, uint64_t nlist, uint32_t* out) {
	const rxgpu::IvfPlaceShape s = rxgpu::ivf_place_shape(n, nlist);
	out[0] = s.blocks;
	out[1] = s.span;
}
// seg_off [nlist + 1], order [n]
void ivf_plan_place(const uint32_t* assign, uint32_t n, uint32_t nlist, uint32_t* seg_off, uint32_t* order) {
	const rxgpu::IvfPlaceShape s = rxgpu::ivf_place_shape(n, nlist);
	std::vector<uint32_t> table(std::size_t(s.blocks) * nlist + 1);
	rxgpu::ivf_place_host(assign, n, nlist, table.data(), seg_off, order);
}
uint32_t ivf_plan_sum_tiles(uint32_t dim) { return rxgpu::ivf_sum_tiles(dim); }
uint64_t ivf_plan_sum_waves(uint64_t nlist, uint32_t dim) { return rxgpu::ivf_sum_waves(nlist, dim); }
uint64_t ivf_plan_sum_blocks(uint64_t nlist, uint32_t dim) { return rxgpu::ivf_sum_blocks(nlist, dim); }
// out = {centroid, col0, cols}
void ivf_plan_sum_unit(uint64_t w, uint32_t dim, uint32_t* out) {
	const rxgpu::IvfSumUnit u = rxgpu::ivf_sum_unit(w, dim);
	out[0] = u.centroid;
	out[1] = u.col0;
	out[2] = u.cols;
}
// out = {o_table, o_seg_off, o_seg_rows, o_centroids, o_hassign, o_flag, bytes}
void ivf_plan_scratch(uint64_t n, uint64_t nlist, uint32_t dim, uint64_t* out) {
	const rxgpu::IvfTrainScratch s = rxgpu::ivf_train_scratch(n, nlist, dim);
	const uint64_t v[7] = {s.o_table, s.o_seg_off, s.o_seg_rows, s.o_centroids, s.o_hassign, s.o_flag, s.bytes};
	for (int i = 0; i < 7; ++i) out[i] = v[i];
}

}  // extern "C"
