// The launch policy of an HNSW search (reindexer_amd/csrc/hnsw_launch_plan.h) compiled for the host: tests/test_hnsw_launch_plan.py pins
// its rules on the CPU.  The hooks are read from the process environment, as the library reads them.  Test infrastructure only — nothing
// in the product links this.
#include <cstdint>

#include "hnsw_launch_plan.h"

extern "C" {

// every field of the plan as one 64-bit word, in the order of kFields in the test
void hnsw_plan_cpu(uint64_t count, uint32_t dim, int bare, uint32_t nq, uint32_t k, uint32_t ef, int sq8, int to_host, uint64_t visited_avail_bytes,
				   uint64_t* out) {
	const rxgpu::HnswLaunchPlan p = rxgpu::plan_hnsw_search(count, dim, bare != 0, nq, k, ef, sq8 != 0, to_host != 0, visited_avail_bytes, rxgpu::read_hnsw_knobs());
	const uint64_t v[] = {p.big_ef,      p.words,        p.max_slots,  p.vis_hash_log2, p.vis_lds_log2,      p.vis_words,     p.vis_slots, p.first_zero_bytes,
						  p.split_upload, p.split_parts,  p.part_q,     p.o_qcorr,       p.o_qnorm,           p.staged,        p.zero_copy, p.st_corr,
						  p.st_norm,     p.st_count,     p.st_dist,    p.st_row,        p.st_end,            p.prefetch_links, p.team,     p.team_max,
						  p.nbl,         p.spec,         p.lds_cand_cap, p.ef_cap,      p.use_sorted,        p.sorted_mode,   p.sorted_restart_cap, p.helper_wanted,
						  p.tier_cap[0], p.tier_cap[1],  p.force_global_tiers};
	for (uint64_t x : v) *out++ = x;
}

int hnsw_knobs_names_a_kernel() { return rxgpu::read_hnsw_knobs().names_a_kernel ? 1 : 0; }

// the five constants the policy shares with the kernels
void hnsw_plan_constants(int* out) {
	out[0] = rxgpu::kHnswMaxEf;
	out[1] = rxgpu::kHnswLdsCandEf;
	out[2] = rxgpu::kHnswCandLds;
	out[3] = rxgpu::kHnswSortedMaxEf;
	out[4] = rxgpu::kHnswSortedMaxEfDel;
}
}
