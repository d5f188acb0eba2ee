// The decisions of a batched IVF list search (reindexer_amd/csrc/ivf_batch_plan.h) compiled for the host: tests/test_ivf_batch_plan.py pins
// its rules on the CPU.  Test infrastructure only — nothing in the product links this.  Built with -DIVF_BATCH_PLAN_MAIN it is a stand-alone
// program that walks the chunk rule over a few list shapes (what a sanitizer build runs).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "ivf_batch_plan.h"

extern "C" {

int ivfb_on_device(uint32_t nprobe, uint32_t kk) { return rxgpu::ivf_batch_on_device(nprobe, kk) ? 1 : 0; }
int ivfb_wide_list(uint32_t kk) { return rxgpu::ivf_batch_wide_list(kk) ? 1 : 0; }
int ivfb_default_on_device(uint32_t nq, uint32_t nprobe, uint32_t kk) { return rxgpu::ivf_batch_default_on_device(nq, nprobe, kk) ? 1 : 0; }
uint32_t ivfb_list_chunks(uint64_t rows) { return rxgpu::ivf_batch_list_chunks(rows); }
// out = {slot, offset}
void ivfb_chunk_at(const uint32_t* cum, uint32_t nprobe, uint32_t chunk, uint32_t* out) {
	const rxgpu::IvfBatchChunkAt at = rxgpu::ivf_batch_chunk_at(cum, nprobe, chunk);
	out[0] = at.slot;
	out[1] = at.offset;
}
uint32_t ivfb_grid_x(uint32_t nq, uint32_t nprobe, uint32_t nlist, uint64_t rows_listed, uint64_t longest, uint32_t cus) {
	return rxgpu::ivf_batch_grid_x(nq, nprobe, nlist, rows_listed, longest, cus);
}
uint32_t ivfb_max_grid_x() { return rxgpu::kIvfBatchMaxGridX; }
uint64_t ivfb_default_budget() { return rxgpu::kIvfBatchScratchBytes; }
uint64_t ivfb_query_bytes(uint32_t dim, uint32_t nprobe, uint32_t kk, uint32_t gridx) { return rxgpu::ivf_batch_query_bytes(dim, nprobe, kk, gridx); }
uint32_t ivfb_train_queries(uint32_t nq, uint32_t dim, uint32_t nprobe, uint32_t kk, uint32_t gridx, uint64_t budget) {
	return rxgpu::ivf_batch_train_queries(nq, dim, nprobe, kk, gridx, budget);
}
uint32_t ivfb_trains(uint32_t nq, uint32_t train_queries) { return rxgpu::ivf_batch_trains(nq, train_queries); }
// out = {o_probe, o_pdist, o_pcnt, o_cum, o_scanned, bytes}
void ivfb_scratch(uint64_t q, uint32_t nprobe, uint64_t* out) {
	const rxgpu::IvfBatchScratch s = rxgpu::ivf_batch_scratch(q, nprobe);
	const uint64_t v[6] = {s.o_probe, s.o_pdist, s.o_pcnt, s.o_cum, s.o_scanned, s.bytes};
	for (int i = 0; i < 6; ++i) out[i] = v[i];
}

}  // extern "C"

#if defined(IVF_BATCH_PLAN_MAIN)
#include <cstdio>
// every entry of every list exactly once, no chunk across two lists; 0 = ok
static int walk(const std::vector<uint64_t>& len) {
	const uint32_t nprobe = uint32_t(len.size());
	std::vector<uint32_t> cum(nprobe + 1, 0);
	for (uint32_t s = 0; s < nprobe; ++s) cum[s + 1] = cum[s] + rxgpu::ivf_batch_list_chunks(len[s]);
	std::vector<std::vector<int>> seen(nprobe);
	for (uint32_t s = 0; s < nprobe; ++s) seen[s].assign(len[s], 0);
	for (uint32_t c = 0; c < cum[nprobe]; ++c) {
		const rxgpu::IvfBatchChunkAt at = rxgpu::ivf_batch_chunk_at(cum.data(), nprobe, c);
		if (at.slot >= nprobe || at.offset >= len[at.slot]) return 1;
		for (uint64_t i = at.offset; i < at.offset + rxgpu::kIvfBatchChunk && i < len[at.slot]; ++i) ++seen[at.slot][i];
	}
	for (const auto& v : seen)
		for (int n : v)
			if (n != 1) return 2;
	return 0;
}
int main() {
	const std::vector<std::vector<uint64_t>> shapes = {{1}, {0, 1, 0}, {63, 64, 65}, {0, 0, 5000, 1, 64, 0}, std::vector<uint64_t>(128, 77), {0}};
	for (const auto& s : shapes) {
		if (const int rc = walk(s)) {
			std::printf("chunk walk failed: %d\n", rc);
			return 1;
		}
	}
	std::printf("ok\n");
	return 0;
}
#endif
