// Which kernel an HNSW search gets, with how many threads, how much dynamic LDS and at which offsets — as pure functions of the call's shape.
// hnsw_search.hip and hnsw_server.hip compute a pick, copy its patch fields into the launch's HnswParams and hand it to ONE dispatcher each
// (hnsw_dispatch.hip.h), which turns the runtime fields into template arguments; hnsw_lds_layout states the dynamic-LDS areas the launchers size
// and the kernels carve up.  No HIP in here — the file compiles for the host on its own (tests/cpp/hnsw_kernel_pick_cpu.cc, tests/test_hnsw_kernel_pick.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "hnsw_distance_blocks.h"

namespace rxgpu {

constexpr uint32_t kHnswSpecLog2 = 11;   // speculative team search: 2048-entry direct-mapped table of distances computed ahead of time
constexpr uint32_t kHnswSpecBytes = (2u << kHnswSpecLog2) * 4 + (128 + 3 * 64) * 4;   // table + two link blocks + the trip's id / distance / destination arrays
constexpr int kHnswNblRows = 32;             // team searches: link blocks fetched along with a hop's rows (one 64-word slot each)
constexpr uint32_t kHnswNblBytes = kHnswNblRows * 64 * 4;
constexpr size_t kHnswLdsPlain = size_t(60) << 10;     // dynamic LDS a launch gets without an attribute (kept under the 64 KB limit)
constexpr size_t kHnswLdsRaised = size_t(150) << 10;   // a handful of workgroups, one per CU: each may take most of the CU's 160 KB (the launcher raises the kernel's limit)

// The dynamic LDS of a search, areas in order: [ef_cap] result heap (dist, id), then [lds_cand_cap] candidate heap (dist, id) — none when it
// lives in global scratch —, then the query fragment of a fixed-dimension float search (nb * 16 float4; 16-byte aligned: every part is a
// multiple of 64 entries), then the visited hash set of the forms that keep it in LDS.  The three sized areas in their own elements (8-byte
// heap entries, float4): the kernels step from one area to the next with typed pointers, the launchers ask for the byte offsets.
struct HnswLdsLayout {
	uint32_t top, cand;   // heap entries
	uint32_t query;       // float4
	constexpr size_t cand_off() const { return size_t(top) * 8; }
	constexpr size_t query_off() const { return (size_t(top) + cand) * 8; }
	constexpr size_t visited_off() const { return query_off() + size_t(query) * 16; }
};
constexpr HnswLdsLayout hnsw_lds_layout(uint32_t ef_cap, uint32_t lds_cand_cap, bool global_cand, int nb, bool sq8) {
	return HnswLdsLayout{ef_cap, global_cand ? 0 : lds_cand_cap, uint32_t(sq8 ? 0 : nb * 16)};
}

// the call: the fields of HnswParams (knn_kernels.hip.h) and of the launch that decide
struct HnswPickInput {
	uint32_t dim, ef, ef_cap, lds_cand_cap;
	bool sorted, bare, sq8;
	uint32_t team, team_max;
	uint32_t vis_lds, vis_lds_log2, vis_hash_log2;   // vis_lds / vis_hash_log2: what the caller set (the pick passes them on or overrides them)
	bool has_visited;                                // server: a visited buffer in HBM
	bool sq8_query;                                  // server over codes: corrective offsets and the mailbox's codes / corr / normCoef arrays are there
	uint32_t nbl, spec, maxM0;
	uint32_t blocks;                                 // searches of the launch / groups of helpers / slots of the mailbox
	bool global_cand;
	bool filtered = false;                           // the call brings an allowed-rows bitmap (HnswFilteredParams): the kernels of hnsw_filtered.hip
};

enum HnswKernelFamily : int { kHnswSearch = 0, kHnswTeam, kHnswHelper, kHnswServer, kHnswServerWide, kHnswServerSq8, kHnswFiltered, kHnswFilteredTeam };

struct HnswKernelPick {
	HnswKernelFamily family;
	int nb, sorted;      // template arguments NB and kSorted
	bool del, latency, sq8, global_cand;
	int team;            // wavefronts per search (kTeam)
	uint32_t threads;
	size_t lds_bytes;
	uint32_t vis_lds, vis_hash_log2, nbl_off, spec_off;   // what the launcher patches into HnswParams
	bool needs_raised_lds;                                // lds_bytes > kHnswLdsPlain: the kernel's limit goes up to kHnswLdsRaised first
	bool served;                                          // server: false = this call has no resident form
};

// both queues as one sorted list in registers.  Without deleted nodes: 2 entries a lane up to ef = 128, 4 up to 256; with deleted nodes the
// list also holds the deleted candidates in reach: 2 entries a lane up to ef = 96, 3 up to 160, 4 up to 224 (kHnswSortedMaxEfDel)
constexpr int hnsw_sorted_slots(uint32_t ef, bool bare) { return bare ? (ef > 128u ? 4 : 2) : (ef <= 96u ? 2 : ef <= 160u ? 3 : 4); }

// the link-block area (RXGPU_HNSW_NBL) and the look-ahead area (RXGPU_HNSW_SPEC) of a team behind `at` bytes, where they stay under kHnswLdsRaised
constexpr size_t hnsw_team_areas(const HnswPickInput& in, size_t at, HnswKernelPick& k) {
	if (in.nbl && !in.spec && in.maxM0 < 64u && at + kHnswNblBytes <= kHnswLdsRaised) {   // the link blocks of a hop's rows come along with the rows (hnsw_team_serve)
		k.nbl_off = uint32_t(at);
		at += kHnswNblBytes;
	}
	if (in.spec && !k.del && in.maxM0 < 64u && at + kHnswSpecBytes <= kHnswLdsRaised) {   // distances of the next candidate's neighbours ride along (hnsw_search_core.hip.h)
		k.spec_off = uint32_t(at);
		at += kHnswSpecBytes;
	}
	return at;
}

constexpr HnswKernelPick hnsw_pick_start(const HnswPickInput& in, HnswKernelFamily family) {
	HnswKernelPick k{};
	k.family = family;
	k.team = 1;
	k.threads = 64;
	k.vis_lds = in.vis_lds;
	k.vis_hash_log2 = in.vis_hash_log2;
	k.served = true;
	return k;
}
constexpr HnswKernelPick hnsw_pick_end(HnswKernelPick k, size_t lds) {
	k.lds_bytes = lds;
	k.needs_raised_lds = lds > kHnswLdsPlain;
	return k;
}

// launch_hnsw_filtered: a search under an allowed-rows bitmap (hnsw_filtered_kernel, or hnsw_filtered_team_kernel for a handful of floats
// searches).  Hidden nodes are traversed like deleted ones, so the pick is never bare: the list with deleted nodes up to ef = 224
// (kHnswSortedMaxEfDel), the heaps above that and in every re-run with global candidates.  The family has the fixed distance batches for
// 128 and 768 components only (other fixed sizes take the generic batch: same bits), no latency form outside the team, no link-block or
// look-ahead area, and neither helpers nor a resident form (the launch plan and hnsw_search_impl leave both out).
constexpr int hnsw_filtered_blocks(uint32_t dim) { return dim == 128u ? 2 : dim == 768u ? 12 : 0; }
constexpr HnswKernelPick pick_hnsw_filtered(const HnswPickInput& in) {
	HnswKernelPick k = hnsw_pick_start(in, kHnswFiltered);
	k.sq8 = in.sq8;
	k.global_cand = in.global_cand;
	k.vis_lds = 0;
	if (in.sorted && !in.global_cand && in.ef <= 224u) {
		k.sorted = hnsw_sorted_slots(in.ef, false);
		k.del = true;
	}
	k.nb = hnsw_filtered_blocks(in.dim);
	size_t lds = hnsw_lds_layout(in.ef_cap, in.lds_cand_cap, in.global_cand, k.nb, in.sq8).visited_off();
	if (!in.sq8 && k.nb > 0 && k.sorted > 0 && in.team > 1u && in.blocks <= in.team_max) {   // the planner's call is one query: four wavefronts per search
		k.family = kHnswFilteredTeam;
		k.latency = true;
		k.team = 4;
		k.threads = 256;
		if (in.vis_lds_log2) {   // the visited set in LDS, by the rule of the unfiltered team (pick_hnsw_search)
			uint32_t lg = in.vis_lds_log2;
			if (lg >= 12u && lg < 14u) lg += 1u;
			if ((size_t(4) << lg) <= (64u << 10)) {
				k.vis_lds = 1;
				k.vis_hash_log2 = lg;
				lds += size_t(4) << lg;
			}
		}
	}
	return hnsw_pick_end(k, lds);
}

// launch_hnsw_search: hnsw_search_kernel, or hnsw_team_kernel for a handful of searches
constexpr HnswKernelPick pick_hnsw_search(const HnswPickInput& in) {
	if (in.filtered) return pick_hnsw_filtered(in);
	HnswKernelPick k = hnsw_pick_start(in, kHnswSearch);
	k.sq8 = in.sq8;
	k.global_cand = in.global_cand;
	if (in.sorted && !in.global_cand) {
		k.sorted = hnsw_sorted_slots(in.ef, in.bare);
		k.del = !in.bare;
	}
	k.nb = hnsw_distance_blocks(in.dim, in.sq8, k.del);   // (the heaps handle deleted nodes themselves: one list of sizes)
	size_t lds = hnsw_lds_layout(in.ef_cap, in.lds_cand_cap, in.global_cand, k.nb, in.sq8).visited_off();
	if (in.sq8) return hnsw_pick_end(k, lds);
	// a handful of searches (the Map's single queries and small coalesced batches): four wavefronts per search (hnsw_team_kernel)
	if (k.nb > 0 && k.sorted > 0 && in.team > 1u && in.blocks <= in.team_max) {
		k.family = kHnswTeam;
		k.latency = true;
		k.team = 4;
		k.threads = 256;
		// the visited set in LDS, one size up from what the caller allows where that stays within 64 KB (a handful of workgroups: each may take
		// a large part of its CU's 160 KB): at 10M x 768, ef = 128, 0.7 % of the searches mark more than the 4096 nodes a 32 KB set holds, and
		// every one of them costs a re-run launch with a bitset behind the batch
		if (in.vis_lds_log2) {
			uint32_t lg = in.vis_lds_log2;
			if (lg >= 12u && lg < 14u) lg += 1u;   // (smaller sizes are the tests' way of forcing the re-run tiers: left as asked)
			if ((size_t(4) << lg) <= (64u << 10)) {
				k.vis_lds = 1;
				k.vis_hash_log2 = lg;
				lds += size_t(4) << lg;
			}
		}
		lds = hnsw_team_areas(in, lds, k);   // (its own statement: the areas' offsets land in k before k is copied)
		return hnsw_pick_end(k, lds);
	}
	// no more searches than the chip holds of this form (3 per SIMD; at 1536 floats the two row sets in flight leave one wavefront per SIMD): spend registers on fewer round trips
	k.latency = k.nb > 8 && in.blocks <= (k.nb > 16 ? 1024u : 3072u);
	// at most two searches per CU and a set of up to 32 KB: the visited set moves into LDS (dynamic LDS stays under the 64 KB a launch gets
	// without an attribute)
	if (k.latency && !in.global_cand && in.vis_lds_log2 && in.blocks <= 512u && (size_t(4) << in.vis_lds_log2) <= (32u << 10) &&
		lds + (size_t(4) << in.vis_lds_log2) <= kHnswLdsPlain) {
		k.vis_lds = 1;
		k.vis_hash_log2 = in.vis_lds_log2;
		lds += size_t(4) << in.vis_lds_log2;
	}
	return hnsw_pick_end(k, lds);
}

// launch_hnsw_helper: the helper workgroups of a batch run the heap search with the largest LDS heap.  Codes: the two sizes every SQ8 graph
// has a fixed form for; floats: 512 has no helper instantiation of its own (the generic batch)
constexpr HnswKernelPick pick_hnsw_helper(const HnswPickInput& in) {
	HnswKernelPick k = hnsw_pick_start(in, kHnswHelper);
	k.sq8 = in.sq8;
	k.nb = in.sq8 ? hnsw_distance_blocks(in.dim, true, true) : hnsw_distance_blocks(in.dim, false, false);
	if (!in.sq8 && k.nb == 8) k.nb = 0;
	k.latency = k.nb > 8 && !in.sq8;
	return hnsw_pick_end(k, hnsw_lds_layout(in.ef_cap, in.lds_cand_cap, false, k.nb, in.sq8).visited_off());
}

// launch_hnsw_server.  Two classes of resident kernel (an index may have one of each per row format, serving a mailbox of its own): ef <= 128
// (96 with deleted nodes) — lists of two entries a lane, the visited set in LDS — and ef <= 256 (224) — four entries a lane, the visited hash
// set of a slot in HBM.  ef_cap says which: 128 or 256.  The resident kernel exists for the embedding sizes with a fixed-dimension distance
// batch; everything else keeps the launches (served = false).
// Dynamic LDS of a float workgroup: heaps + query fragment + visited set, then (what fits) the link-block area and the look-ahead area.  Over
// codes a slot is one wavefront: heaps and visited set, no query fragment (the codes live in registers).
constexpr HnswKernelPick pick_hnsw_server(const HnswPickInput& in) {
	HnswKernelPick k = hnsw_pick_start(in, kHnswServer);
	const size_t vis = in.vis_lds_log2 ? (size_t(4) << in.vis_lds_log2) : 0;
	k.del = !in.bare;
	k.latency = true;
	k.sorted = in.ef_cap > 128u ? 4 : 2;   // the second mailbox of an index: lists of four entries a lane
	// (the float layout over dim / 64 blocks is also what the gate below measures, whatever the row format)
	const size_t lds = hnsw_team_areas(in, hnsw_lds_layout(in.ef_cap, in.lds_cand_cap, false, int(in.dim / 64u), false).visited_off() + vis, k);
	k = hnsw_pick_end(k, lds);
	k.served = in.sorted && k.lds_bytes <= kHnswLdsRaised &&
			   (in.ef_cap <= 128u ? (in.vis_lds && in.vis_lds_log2 <= 14u) : (!in.vis_lds && !in.vis_lds_log2 && in.has_visited && in.vis_hash_log2 >= 14u));
	k.nb = hnsw_distance_blocks(in.dim, in.sq8, k.del);
	if (k.nb == 0) k.served = false;
	if (in.sq8) {
		k.family = kHnswServerSq8;
		k.sq8 = true;
		k.nbl_off = k.spec_off = 0u;
		if (!in.sq8_query) k.served = false;
		return hnsw_pick_end(k, hnsw_lds_layout(in.ef_cap, in.lds_cand_cap, false, k.nb, true).visited_off() + vis);
	}
	k.family = k.nb > 12 ? kHnswServerWide : kHnswServer;   // rows of 1024 and 1536 floats are read in chunks
	k.team = 4;
	k.threads = 256;
	return k;
}

// The instantiations that exist: the dispatchers guard with these (`if constexpr`), so a pick outside the set is a host error, never another kernel.
constexpr bool hnsw_sorted_form_exists(int sorted, bool del) { return sorted == 2 || sorted == 4 || (del && sorted == 3); }
constexpr bool hnsw_float_nb(int nb) { return nb == 0 || nb == 2 || nb == 8 || nb == 12 || nb == 16 || nb == 24; }
constexpr bool hnsw_sq8_nb(int nb, bool del) { return nb == 0 || nb == 2 || nb == 12 || (!del && (nb == 6 || nb == 8 || nb == 16 || nb == 24)); }
constexpr bool hnsw_search_kernel_exists(bool global_cand, int nb, bool latency, bool sq8, int sorted, bool del) {
	if (sorted == 0 ? del : (global_cand || !hnsw_sorted_form_exists(sorted, del))) return false;
	return sq8 ? (!latency && hnsw_sq8_nb(nb, del)) : (hnsw_float_nb(nb) && (!latency || nb > 8));
}
constexpr bool hnsw_team_kernel_exists(int nb, int sorted, bool del) { return nb > 0 && hnsw_float_nb(nb) && hnsw_sorted_form_exists(sorted, del); }
// hnsw_filtered.hip: heaps in LDS and with global candidates, the three lists with deleted nodes; floats and codes with the generic batch and
// the fixed ones for 128 and 768 components; the team for floats at those two sizes on the lists
constexpr bool hnsw_filtered_kernel_exists(bool team, bool global_cand, int nb, bool sq8, int sorted, bool del) {
	if (nb != 0 && nb != 2 && nb != 12) return false;
	if (team) return !sq8 && nb > 0 && !global_cand && del && sorted >= 2 && sorted <= 4;
	return sorted == 0 ? !del : (del && !global_cand && sorted >= 2 && sorted <= 4);
}
constexpr bool hnsw_helper_kernel_exists(int nb, bool sq8) { return sq8 ? hnsw_sq8_nb(nb, true) : (hnsw_float_nb(nb) && nb != 8); }
constexpr bool hnsw_server_kernel_exists(int nb, bool sq8, int sorted, bool del) {
	return nb > 0 && (sorted == 2 || sorted == 4) && (sq8 ? hnsw_sq8_nb(nb, del) : hnsw_float_nb(nb));
}

}  // namespace rxgpu
