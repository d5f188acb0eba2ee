// The launch policy of an HNSW search (rxgpu_hnsw_search.hip: hnsw_search_impl) as a pure function of the call's shape and the RXGPU_HNSW_*
// hooks: what the executor stages, zeroes, splits and launches follows from the plan alone.  No HIP in here — the file compiles for the host
// on its own (tests/cpp/hnsw_launch_plan_cpu.cc, tests/test_hnsw_launch_plan.py).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <unistd.h>   // environ

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace rxgpu {

constexpr int kHnswMaxEf = 4096;        // result-heap capacity in LDS (above kHnswLdsCandEf the candidate heap lives in global scratch)
constexpr int kHnswLdsCandEf = 1024;    // largest ef whose candidate heap is tried in LDS first
constexpr int kHnswCandLds = 2048;      // candidate-heap capacity in LDS
constexpr int kHnswSortedMaxEf = 256;            // largest ef the sorted-list search holds in registers (4 entries a lane)
constexpr int kHnswSortedMaxEfDel = 224;         // ... for a graph with deleted nodes: 32 entries of room for the deleted candidates in reach
// what a search leaves in its out_count instead of a count when the host has to run it again (hnsw_rerun_plan.h)
constexpr uint32_t kHnswOverflow = 0xFFFFFFFFu;
constexpr uint32_t kHnswTie = 0xFFFFFFFEu;        // sorted-list search met equal keys: re-run on the heap kernel

// The A/B and test hooks of the HNSW search (RXGPU_HNSW_*), read in ONE pass over the environment per call — a dozen getenv() lookups each
// walked the whole environment, on the path of every single-query SearchKnn.  (Still the process environment: tests flip the hooks between
// calls.  Not safe against a concurrent setenv, like getenv itself.)
struct HnswKnobs {
	const char* visited = nullptr;       // RXGPU_HNSW_VISITED = bitset | hash
	int visited_log2 = -1;               // RXGPU_HNSW_VISITED_LOG2
	int visited_lds = -1;                // RXGPU_HNSW_VISITED_LDS
	int split_upload = -1;               // RXGPU_HNSW_SPLIT_UPLOAD
	int prefetch = -1;                   // RXGPU_HNSW_PREFETCH
	int lds_cand_cap = -1;               // RXGPU_HNSW_LDS_CAND_CAP
	int helper = -1;                     // RXGPU_HNSW_HELPER
	int restart_cand = -1;               // RXGPU_HNSW_RESTART_CAND
	int sorted = -1;                     // RXGPU_HNSW_SORTED
	int gcand_cap = -1;                  // RXGPU_HNSW_GCAND_CAP
	int team = -1;                       // RXGPU_HNSW_TEAM: wavefronts per search of a small launch (1 = off)
	int team_max = -1;                   // RXGPU_HNSW_TEAM_MAX: searches per launch up to which the team form is used
	int zero_copy = -1;                  // RXGPU_HNSW_ZERO_COPY = 0: small calls copy their queries / results like large ones
	int nbl = -1;                        // RXGPU_HNSW_NBL = 1: team searches fetch the link blocks of a hop's rows along with the rows (an experiment, off by default)
	int spec = -1;                       // RXGPU_HNSW_SPEC = 1: team searches also evaluate the next candidate's neighbours in the hop's distance trip (an experiment, off by default)
	int server = -1;                     // RXGPU_HNSW_SERVER = 0: single queries take a launch each (no resident kernel)
	int server_sq8 = -1;                 // RXGPU_HNSW_SERVER_SQ8 = 0: single queries over SQ8 codes take a launch each (the float mailbox stays; A/B)
	int server_slots = -1, server_idle_us = -1, server_life_ms = -1;   // RXGPU_HNSW_SERVER_SLOTS / _IDLE_US / _LIFE_MS
	bool names_a_kernel = false;         // a hook that picks a kernel form is set: the resident kernel (one form) stands aside
};
inline HnswKnobs read_hnsw_knobs() {
	HnswKnobs k;
	static const char kPrefix[] = "RXGPU_HNSW_";
	for (char** e = environ; e && *e; ++e) {
		const char* s = *e;
		if (s[0] != 'R' || std::strncmp(s, kPrefix, sizeof(kPrefix) - 1) != 0) continue;
		const char* name = s + sizeof(kPrefix) - 1;
		const char* eq = std::strchr(name, '=');
		if (!eq) continue;
		const size_t n = size_t(eq - name);
		const char* val = eq + 1;
		auto is = [&](const char* want) { return std::strlen(want) == n && std::strncmp(name, want, n) == 0; };
		if (is("VISITED")) k.visited = val;
		else if (is("VISITED_LOG2")) k.visited_log2 = atoi(val);
		else if (is("VISITED_LDS")) k.visited_lds = atoi(val);
		else if (is("SPLIT_UPLOAD")) k.split_upload = atoi(val);
		else if (is("PREFETCH")) k.prefetch = atoi(val);
		else if (is("LDS_CAND_CAP")) k.lds_cand_cap = atoi(val);
		else if (is("HELPER")) k.helper = atoi(val);
		else if (is("RESTART_CAND")) k.restart_cand = atoi(val);
		else if (is("SORTED")) k.sorted = atoi(val);
		else if (is("GCAND_CAP")) k.gcand_cap = atoi(val);
		else if (is("TEAM")) k.team = atoi(val);
		else if (is("TEAM_MAX")) k.team_max = atoi(val);
		else if (is("ZERO_COPY")) k.zero_copy = atoi(val);
		else if (is("SPEC")) k.spec = atoi(val);
		else if (is("NBL")) k.nbl = atoi(val);
		else if (is("SERVER")) k.server = atoi(val);
		else if (is("SERVER_SQ8")) k.server_sq8 = atoi(val);
		else if (is("SERVER_SLOTS")) k.server_slots = atoi(val);
		else if (is("SERVER_IDLE_US")) k.server_idle_us = atoi(val);
		else if (is("SERVER_LIFE_MS")) k.server_life_ms = atoi(val);
		else continue;
		if (!is("SERVER") && !is("SERVER_SQ8") && !is("SERVER_SLOTS") && !is("SERVER_IDLE_US") && !is("SERVER_LIFE_MS") && !is("SPLIT_UPLOAD") && !is("HELPER") && !is("SPEC") && !is("NBL")) k.names_a_kernel = true;
	}
	return k;
}

// Everything hnsw_search_impl decides before it touches the device.  Byte offsets are into the context's query buffer (o_*) and its pinned
// staging buffer (st_*).
struct HnswLaunchPlan {
	bool big_ef;                   // ef > kHnswLdsCandEf: no first pass, every query goes to the global-heap tiers
	uint64_t words;                // words of one bitset over the nodes
	uint64_t max_slots;            // bitsets (= searches) one launch of a re-run tier may hold
	uint32_t vis_hash_log2;        // first pass and tie re-runs: 0 = bitset, else log2 of the hash set's words (in HBM)
	uint32_t vis_lds_log2;         // ... of the same set in LDS for a handful of searches (0: off)
	uint64_t vis_words, vis_slots; // per search of the first pass / searches per launch of it
	size_t first_zero_bytes;       // bitsets of the first launch zeroed on the second stream in front of the query upload (0: by the launch's own memset)
	bool split_upload;
	uint32_t split_parts, part_q;  // part_q: queries uploaded in front of the first launch = queries per part
	size_t o_qcorr, o_qnorm;
	bool staged, zero_copy;
	size_t st_corr, st_norm, st_count, st_dist, st_row, st_end;
	uint32_t prefetch_links, team, team_max, nbl, spec;
	uint32_t lds_cand_cap, ef_cap;
	bool use_sorted;
	uint32_t sorted_mode, sorted_restart_cap;
	bool helper_wanted;
	uint64_t tier_cap[2];
	bool force_global_tiers;       // RXGPU_HNSW_LDS_CAND_CAP is set: overflowing searches skip the LDS re-run
};

// count / dim / bare: the index (rows, floats or codes per row, no deleted nodes); nq / k / ef: the call, k and ef already defaulted and
// checked; visited_avail_bytes: free HBM + what the context's visited buffer already holds (small calls pass the latter alone).
// filtered: the call brings an allowed-rows bitmap — never bare (the caller passes bare = false), and no helper workgroups: the filtered
// family has none.
inline HnswLaunchPlan plan_hnsw_search(uint64_t count, uint32_t dim, bool bare, uint32_t nq, uint32_t k, uint32_t ef, bool sq8, bool to_host,
									   uint64_t visited_avail_bytes, const HnswKnobs& knobs, bool filtered = false) {
	HnswLaunchPlan pl{};
	// ef > 1024: the result heap alone takes the LDS budget of a search — the candidate heap goes to global scratch from the start
	const bool big_ef = pl.big_ef = ef > uint32_t(kHnswLdsCandEf);
	const uint64_t words = pl.words = (count + 31) / 32;
	// visited bitsets are the memory hog (N / 8 bytes per resident search): a launch gets an eighth of the free HBM for them, between 2 and
	// 16 GiB.  (A fixed 2 GiB held a 10M-node index to 1717 searches per launch — fewer than the chip keeps resident.)
	// (a handful of searches never comes near the budget: no driver call on the path of a single-query SearchKnn)
	const uint64_t visited_budget = std::min<uint64_t>(16ull << 30, std::max<uint64_t>(2ull << 30, visited_avail_bytes / 8));
	const uint64_t max_slots = pl.max_slots = std::max<uint64_t>(1, std::min<uint64_t>(32768, visited_budget / (words * 4)));
	// The visited set of the first pass (and of the tie re-runs) is a HASH SET sized by ef, zeroed by the search itself — not a bitset over
	// the nodes zeroed by a memset: 2^k words >= 64 ef (8192 words = 32 KB at ef = 128; a search may fill half: 4096 nodes, against the
	// 850 - 2300 it tests at 1M - 10M rows) instead of N / 8 bytes (1.25 MB per search at 10M rows: 20 GB of memset in front of a 16 384-query
	// launch).  Searches that would outgrow it come back as kHnswOverflow and take the global-heap re-run, which keeps the bitset.
	// Graphs so small that the bitset is the smaller of the two keep it.  RXGPU_HNSW_VISITED=bitset: the former path (A/B, tests).
	pl.vis_hash_log2 = 12;
	while ((1ull << pl.vis_hash_log2) < 64ull * ef && pl.vis_hash_log2 < 18) ++pl.vis_hash_log2;
	if (knobs.visited_log2 >= 0) pl.vis_hash_log2 = uint32_t(std::min(20, std::max(6, knobs.visited_log2)));   // test hook: force overflows
	// a handful of searches (the latency form of the kernel, at most two workgroups per CU): the same hash set in LDS, whatever the rule
	// below picks for batches — the launcher decides (pick_hnsw_search, hnsw_kernel_pick.h).  RXGPU_HNSW_VISITED_LDS=0: off (A/B)
	pl.vis_lds_log2 = pl.vis_hash_log2;
	if (knobs.visited_lds == 0) pl.vis_lds_log2 = 0;
	if (knobs.visited) pl.vis_lds_log2 = 0;   // an explicit choice of the global form (A/B, tests) stands for every launch
	{
		const char* e = knobs.visited;   // "bitset" / "hash": force one of the two (A/B, tests on small graphs)
		const bool force_hash = e && std::strcmp(e, "hash") == 0;
		// Which one by default: the hash set costs a second dependent trip on the hops where a lane's first slot is taken (measured at 1M x 768,
		// ef = 128, same box and graph: 1.28 - 1.33 M q/s against 1.43 - 1.46 M on the bitset, profiles/rd4f_hnsw_visited_ab.txt); the bitset
		// costs its memset (N / 8 bytes per query) and, once the bitsets of the searches in flight outgrow the Infinity Cache, an HBM round trip per
		// test.  The hash set takes over where one search's bitset is 16 x its hash set or more (4.2 M nodes at ef = 128).
		if ((e && std::strcmp(e, "bitset") == 0) || (!force_hash && (16ull << pl.vis_hash_log2) > words)) pl.vis_hash_log2 = 0;
		// in HBM the set gets twice the words (a quarter full at most): fewer second probes — 10M x 768, one graph and box, 16 384 queries:
		// 2^13 words 469 k q/s kernels only, 2^14 498 k, 2^15 497 k, 2^16 483 k, bitset 472 k (profiles/rd4j_hnsw_10m_*.json)
		if (pl.vis_hash_log2 && knobs.visited_log2 < 0 && pl.vis_hash_log2 < 18) pl.vis_hash_log2 += 1;
	}
	const uint64_t vis_words = pl.vis_words = pl.vis_hash_log2 ? (1ull << pl.vis_hash_log2) : words;   // per search of the first pass
	const uint64_t vis_slots = pl.vis_slots = pl.vis_hash_log2 ? std::max<uint64_t>(1, std::min<uint64_t>(32768, visited_budget / (vis_words * 4))) : max_slots;
	// SQ8 queries: [codes, padded to 4 bytes][corr][normCoef] in the one query buffer
	const size_t qelem = sq8 ? sizeof(uint8_t) : sizeof(float);
	const size_t qbytes = size_t(nq) * dim * qelem;
	pl.o_qcorr = (qbytes + 255) & ~size_t(255);
	pl.o_qnorm = pl.o_qcorr + ((size_t(nq) * 4 + 255) & ~size_t(255));
	// the bitsets of the first launch (N / 8 bytes per search: 2 GB for 16 384 searches over 1M nodes) are zeroed on a second stream and
	// enqueued BEFORE the upload of the query block (a copy from pageable memory keeps this thread until it is staged): the two overlap,
	// the launch waits for both
	if (!big_ef && !pl.vis_hash_log2) {
		const uint32_t cq = uint32_t(std::min<uint64_t>(vis_slots, nq));
		const size_t zero_bytes = size_t(cq) * words * 4;
		if (zero_bytes >= (size_t(8) << 20)) pl.first_zero_bytes = zero_bytes;
	}
	// A large batch in ONE launch is searched in two halves on two streams: the upload of the second half of the query block (a copy from
	// pageable memory keeps this thread until it is staged) runs while the first half's searches have started; the halves overlap on the
	// device like the workgroups of one launch.  RXGPU_HNSW_SPLIT_UPLOAD=0: one upload, one launch.
	// Round 6: four parts from 2048 queries on (the first launch waits for a quarter of the block, three quarters of the upload run under
	// searches), the parts alternating between the two streams; RXGPU_HNSW_SPLIT_UPLOAD = n: that many parts (0 / 1: one upload, one launch).
	pl.split_upload = !big_ef && nq >= 2048 && uint64_t(nq) <= vis_slots;
	pl.split_parts = 4;
	if (knobs.split_upload >= 0) {
		pl.split_upload = pl.split_upload && knobs.split_upload > 1;
		pl.split_parts = uint32_t(std::min(16, std::max(2, knobs.split_upload)));
	}
	pl.part_q = pl.split_upload ? (nq + pl.split_parts - 1) / pl.split_parts : nq;
	// Small calls — the Map's single queries and its coalesced batches — move their queries and results through the context's PINNED buffer.
	// A copy between pageable memory and the device goes through the runtime's own staging, one call after the other whatever their
	// streams: T planner threads then queue up in the copies on both sides of a 0.5 ms kernel.  (Large batches keep the direct copies:
	// they are the bandwidth case, and the two-halves upload overlaps them with the searches.)
	const size_t up_bytes = (size_t(nq) * dim * qelem + 15) & ~size_t(15);
	pl.st_corr = up_bytes;
	pl.st_norm = pl.st_corr + size_t(nq) * 4;
	pl.st_count = pl.st_norm + size_t(nq) * 4;
	pl.st_dist = pl.st_count + size_t(nq) * 4;
	pl.st_row = pl.st_dist + size_t(nq) * k * 4;
	pl.st_end = pl.st_row + size_t(nq) * k * 4;
	pl.staged = !pl.split_upload && pl.st_end <= (size_t(1) << 20);
	// The Map's single queries and its small coalesced batches do not copy at all: the kernel reads the queries from the pinned buffer (once,
	// into LDS or registers) and writes counts and lists there — a call is ONE launch and one wait instead of a launch between four copies
	// (each an enqueue of its own on the path of a 0.5 ms search).  RXGPU_HNSW_ZERO_COPY=0: the copies (A/B).
	pl.zero_copy = pl.staged && to_host && !sq8 && nq <= 64 && knobs.zero_copy != 0;
	pl.prefetch_links = 1;
	if (knobs.prefetch >= 0) pl.prefetch_links = knobs.prefetch ? 1u : 0u;   // A/B hook
	// a handful of searches on the chip: four wavefronts share a search's distance batches (RXGPU_HNSW_TEAM=1: off, RXGPU_HNSW_TEAM_MAX: up to
	// how many searches per launch)
	pl.team = knobs.team >= 0 ? uint32_t(knobs.team) : 4u;
	pl.team_max = knobs.team_max >= 0 ? uint32_t(knobs.team_max) : 256u;
	pl.nbl = knobs.nbl > 0 ? 1u : 0u;
	pl.spec = knobs.spec > 0 ? 1u : 0u;   // off by default: measured slower at 1M x 768 (profiles/rd6sp_single.json), see hnsw_search_core.hip.h
	pl.ef_cap = (ef + 63u) & ~63u;
	// typical candidate heaps stay within a few x ef.  Measured at 1M x 768, ef = 128: 512 entries overflow for a handful of queries and the
	// global-heap re-run costs more than the extra occupancy brings (1.07 M q/s at 1024 against 0.43 M at 512 and 0.86 M at 768)
	pl.lds_cand_cap = ef <= 256 ? 1024u : uint32_t(kHnswCandLds);
	if (knobs.lds_cand_cap >= 0) {   // test hook: force the global-heap re-run
		pl.lds_cand_cap = std::min<uint32_t>(uint32_t(kHnswCandLds), uint32_t(std::max(1, knobs.lds_cand_cap)));
	}
	pl.force_global_tiers = knobs.lds_cand_cap >= 0;   // (the hook forces the global tiers)
	// Graphs without deleted nodes, ef <= 256: both queues as one sorted list in registers (hnsw_search.hip).  A query that meets equal
	// distances there comes back as kHnswTie and takes the heap kernel, whose sift order is the reference's.
	pl.use_sorted = ef <= uint32_t(bare ? kHnswSortedMaxEf : kHnswSortedMaxEfDel);
	pl.sorted_mode = 1;
	// candidate-heap entries a restarted search gets in LDS.  Measured at 1M x 768, ef = 128, 16 384 queries, ~90 restarts (profiles/
	// rd3p_restart_caps.txt, one graph, one box): 384 entries (8 KB per workgroup, 19 per CU) -> one restart overflows and the global-heap
	// launch it needs costs 2.9 ms; 600 (10 KB, 16 per CU) 11.96 ms in all; 780 12.10; 1024 12.25; no in-kernel restart (0: the tie queries
	// come back to this function and get a launch of their own) 9.92 + 2.53 = 12.46 ms.
	pl.sorted_restart_cap = 600;
	// Round 4: with helper workgroups beside the batch (below) an overflowing restart is no longer a launch behind the batch, and the area
	// can shrink to what lets a CU hold 20 searches instead of 15 (LDS per workgroup 10.3 -> 7.6 KB): first pass of 16 384 queries at
	// 1M x 768 11.9 -> 10.5 ms (profiles/rd4k_hnsw_1m_restart_caps.txt; without the helpers the one restart that overflows costs 2.5 ms).
	const bool helper_wanted = pl.helper_wanted = nq >= 2048 && !big_ef && knobs.helper != 0 && !filtered;
	// ... where a batch lasts long against one heap search: the overflowing searches now run beside the batch, but one that is queued late
	// still sticks out by its own length (2.5 ms at 1M x 768, where the whole batch takes 10: 1.29 M q/s with the copies at 600 entries
	// against 1.16 - 1.22 M at 256 although the first pass alone runs at 1.57 - 1.70 M; at 10M x 768: 495 k -> 586 k q/s,
	// profiles/rd4l_hnsw_*.json).  Same size rule as the hash set.
	if (helper_wanted && ef <= 128 && (16ull << 13) <= words) pl.sorted_restart_cap = 256;
	if (knobs.restart_cand >= 0) pl.sorted_restart_cap = std::min<uint32_t>(uint32_t(kHnswCandLds), uint32_t(knobs.restart_cand));
	if (knobs.sorted >= 0) {   // A/B and test hook: 0 = heaps only, 2 = list shifts through ds_bpermute instead of DPP
		pl.sorted_mode = uint32_t(knobs.sorted);
		pl.use_sorted = pl.use_sorted && pl.sorted_mode != 0;
	}
	// Re-runs with the candidate heap in global scratch, in two tiers: 64 K entries first (0.5 MB per search: hundreds of re-runs share one
	// launch), one entry per node — the bound that cannot overflow — only for what outgrows that.  (With the full bound from the start a
	// 10M-node index allows 13 searches per launch: 39 overflowing queries out of 16 384 cost a quarter of the whole batch.)
	pl.tier_cap[0] = std::min<uint64_t>(count + 1, 65536);
	pl.tier_cap[1] = count + 1;
	if (knobs.gcand_cap >= 0) pl.tier_cap[0] = std::min<uint64_t>(count + 1, uint64_t(std::max(1, knobs.gcand_cap)));   // test hook
	return pl;
}

}  // namespace rxgpu
