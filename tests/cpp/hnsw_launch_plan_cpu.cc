// The launch policy of an HNSW search (reindexer_amd/csrc/hnsw_launch_plan.h) and its re-run ladder (hnsw_rerun_plan.h) compiled for the
// host: tests/test_hnsw_launch_plan.py and tests/test_hnsw_rerun_plan.py pin their rules on the CPU.  The hooks are read from the process
// environment, as the library reads them.  Test infrastructure only — nothing in the product links this.
#include <cstdint>
#include <cstring>

#include "hnsw_rerun_plan.h"

extern "C" {

// every field of the plan as one 64-bit word, in the order of kFields in the test
void hnsw_plan_filtered_cpu(uint64_t count, uint32_t dim, int bare, uint32_t nq, uint32_t k, uint32_t ef, int sq8, int to_host, uint64_t visited_avail_bytes,
							int filtered, uint64_t* out) {
	const rxgpu::HnswLaunchPlan p =
		rxgpu::plan_hnsw_search(count, dim, bare != 0, nq, k, ef, sq8 != 0, to_host != 0, visited_avail_bytes, rxgpu::read_hnsw_knobs(), filtered != 0);
	const uint64_t v[] = {p.big_ef,      p.words,        p.max_slots,  p.vis_hash_log2, p.vis_lds_log2,      p.vis_words,     p.vis_slots, p.first_zero_bytes,
						  p.split_upload, p.split_parts,  p.part_q,     p.o_qcorr,       p.o_qnorm,           p.staged,        p.zero_copy, p.st_corr,
						  p.st_norm,     p.st_count,     p.st_dist,    p.st_row,        p.st_end,            p.prefetch_links, p.team,     p.team_max,
						  p.nbl,         p.spec,         p.lds_cand_cap, p.ef_cap,      p.use_sorted,        p.sorted_mode,   p.sorted_restart_cap, p.helper_wanted,
						  p.tier_cap[0], p.tier_cap[1],  p.force_global_tiers};
	for (uint64_t x : v) *out++ = x;
}
// ... of a call without a bitmap
void hnsw_plan_cpu(uint64_t count, uint32_t dim, int bare, uint32_t nq, uint32_t k, uint32_t ef, int sq8, int to_host, uint64_t visited_avail_bytes,
				   uint64_t* out) {
	hnsw_plan_filtered_cpu(count, dim, bare, nq, k, ef, sq8, to_host, visited_avail_bytes, 0, out);
}

// The re-run ladder of one call, with this function in the device's place: rounds[r][nq] are the counts the host sees at the ladder's r-th
// question (r = 0: behind the first pass).  Every step it hands out goes to steps[] as 9 words — rung, number of ids, slots, 1 if the
// profile name is "hnsw_ties" and 0 if it is "hnsw_redo", vis_hash_log2, visited_words, lds_cand_cap, vis_lds_log2, gcand_cap — and its ids
// behind the ids of the steps before it.  totals: tie_reruns, lds_reruns, 1 if the ladder ended in its overflow error, ids written.  Returns
// the number of steps, or -1: the ladder asked more often than `n_rounds`, or the output arrays are too small.
int hnsw_rerun_cpu(uint64_t count, uint32_t dim, int bare, uint32_t nq, uint32_t k, uint32_t ef, uint64_t visited_avail_bytes, int filtered,
				   uint32_t helper_entries, const uint32_t* rounds, uint32_t n_rounds, uint64_t* steps, uint32_t steps_cap, uint32_t* ids, uint32_t ids_cap,
				   uint64_t* totals) {
	const rxgpu::HnswLaunchPlan pl = rxgpu::plan_hnsw_search(count, dim, bare != 0, nq, k, ef, false, true, visited_avail_bytes, rxgpu::read_hnsw_knobs(), filtered != 0);
	rxgpu::HnswRerunLadder ladder(pl, nq, helper_entries);
	uint32_t n_steps = 0, n_ids = 0;
	for (uint32_t r = 0;; ++r) {
		if (r >= n_rounds) return -1;
		const rxgpu::HnswRerunStep* s = ladder.next(rounds + size_t(r) * nq);
		if (!s) break;
		if (n_steps >= steps_cap || s->ids.size() > ids_cap - n_ids) return -1;
		const bool ties = std::strcmp(s->profile_name, "hnsw_ties") == 0;
		if (!ties && std::strcmp(s->profile_name, "hnsw_redo") != 0) return -1;
		const uint64_t v[9] = {uint64_t(s->rung), s->ids.size(), s->slots, ties, s->vis_hash_log2, s->visited_words, s->lds_cand_cap, s->vis_lds_log2, s->gcand_cap};
		std::memcpy(steps + size_t(n_steps++) * 9, v, sizeof(v));
		for (uint32_t q : s->ids) ids[n_ids++] = q;
	}
	totals[0] = ladder.tie_reruns;
	totals[1] = ladder.lds_reruns;
	totals[2] = ladder.overflowed();
	totals[3] = n_ids;
	return int(n_steps);
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
// the two flags a search leaves in place of a count, and the helper queue's capacity
void hnsw_rerun_constants(uint32_t* out) {
	out[0] = rxgpu::kHnswTie;
	out[1] = rxgpu::kHnswOverflow;
	out[2] = rxgpu::kHnswHelperQueueCap;
}
}
