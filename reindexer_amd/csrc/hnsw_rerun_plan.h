// The re-run ladder of an HNSW search (rxgpu_hnsw_search.hip: hnsw_search_impl): which searches of a batch run again after the first pass,
// on which rung and with which parameters, until every flagged one has come back as the reference's.  Decided from the plan and the counts
// on the host alone; the executor (HnswCall::rerun) carries a step out and asks again.  No HIP in here — the file compiles for the host on
// its own (tests/cpp/hnsw_launch_plan_cpu.cc, tests/test_hnsw_rerun_plan.py).
#pragma once

#include <utility>
#include <vector>

#include "hnsw_launch_plan.h"

namespace rxgpu {

constexpr uint32_t kHnswHelperQueueCap = 4096;   // entries of a batch's overflow queue (HelperBatch); what is appended beyond them is not run by the helpers

enum HnswRung : int {
	kHnswRungTies = 0,     // equal keys met in the sorted list: the same queries through the reference's heaps (candidate heap in LDS)
	kHnswRungLdsMax = 1,   // a candidate heap outgrew its LDS area: once more on the heap kernel with the largest LDS heap there is and a bitset
	kHnswRungGlobal0 = 2,  // the heap in global scratch, HnswLaunchPlan::tier_cap[0] entries a search
	kHnswRungGlobal1 = 3,  // ... one entry per node: the bound that cannot overflow
};

// One launch train of the ladder: the searches `ids` of the batch once more, `slots` of them per launch.
struct HnswRerunStep {
	std::vector<uint32_t> ids;   // ascending
	HnswRung rung;
	uint64_t slots;
	const char* profile_name;
	// what the rung sets in the call's shared HnswParams (every other field stays the call's).  visited_words is the size of one search's
	// visited set — a hash set the search zeroes itself (vis_hash_log2 != 0) or a bitset the executor zeroes; gcand_cap != 0: the candidate
	// heaps live in global scratch, that many entries each.
	uint32_t vis_hash_log2;
	uint64_t visited_words;
	uint32_t lds_cand_cap, vis_lds_log2;
	uint64_t gcand_cap;
};

class HnswRerunLadder {
public:
	// helper_entries: what the batch's searches appended to the helpers' overflow queue (0 without helpers), as the device counted them
	HnswRerunLadder(const HnswLaunchPlan& pl, uint32_t nq, uint32_t helper_entries)
		: pl_(pl), nq_(nq), helper_queued_(std::min(helper_entries, kHnswHelperQueueCap)), at_(pl.big_ef ? kBigEf : kFirstPassDone) {}

	// what the call adds to the index's hnsw_tie_reruns / hnsw_lds_reruns
	uint64_t tie_reruns = 0, lds_reruns = 0;

	// counts[nq]: the call's out_count as the host sees it now — behind the first pass, then behind the step handed out last.  The next
	// step (owned by the ladder, valid until the next call), or nullptr: nothing is left to run.
	const HnswRerunStep* next(const uint32_t* counts) {
		switch (at_) {
		case kFirstPassDone: {
			lds_reruns += helper_queued_;
			at_ = kDone;
			bool clean = true;
			for (uint32_t q = 0; q < nq_; ++q) {
				if (counts[q] == kHnswTie) step_.ids.push_back(q);
				clean = clean && counts[q] != kHnswTie && counts[q] != kHnswOverflow;
			}
			if (clean) return nullptr;
			at_ = kCollectOverflows;
			if (!step_.ids.empty()) {   // a tie re-run never goes through the list: first-pass visited set, the plan's heap area
				tie_reruns += step_.ids.size();
				return emit({{}, kHnswRungTies, pl_.vis_slots, "hnsw_ties", pl_.vis_hash_log2, pl_.vis_words, pl_.lds_cand_cap, pl_.vis_lds_log2, 0});
			}
		}
			[[fallthrough]];
		case kCollectOverflows: {   // (a tie query that overflowed on the heaps is among them)
			step_.ids.clear();
			for (uint32_t q = 0; q < nq_; ++q) {
				if (counts[q] == kHnswOverflow) step_.ids.push_back(q);
			}
			// 600 entries for a search that started over inside the sorted-list kernel, 1024 for the heap kernel's first pass: the largest LDS
			// heap before the global-heap tiers (a search that filled its hash set lands here too).  A search with its heap in global scratch
			// takes 5 - 7 ms at 10M x 768 (profiles/rd4i_hnsw_10m_*.json: ONE such query was a fifth of a 16 384-query batch), one in LDS about 1 ms.
			const uint32_t first_cap = pl_.use_sorted ? pl_.sorted_restart_cap : pl_.lds_cand_cap;
			if (!step_.ids.empty() && first_cap < uint32_t(kHnswCandLds) && !pl_.force_global_tiers) {
				at_ = kLdsMaxDone;
				return emit({{}, kHnswRungLdsMax, pl_.max_slots, "hnsw_redo", 0, pl_.words, uint32_t(kHnswCandLds), 0, 0});
			}
			return global_tier(0);   // (the ids are the flagged ones already)
		}
		case kLdsMaxDone:   // searches the helpers had queued but not finished were among the ids again: counted once
			lds_reruns += step_.ids.size() > helper_queued_ ? step_.ids.size() - helper_queued_ : 0;
			keep_overflowing(counts);
			return global_tier(0);
		case kBigEf:   // no first pass: every query starts with its heap in global scratch
			step_.ids.resize(nq_);
			for (uint32_t q = 0; q < nq_; ++q) step_.ids[q] = q;
			return global_tier(0);
		case kGlobal0:   // (tier 0 ran)
			keep_overflowing(counts);
			return global_tier(1);
		case kGlobal1:
			keep_overflowing(counts);
			at_ = kDone;
			return nullptr;
		case kDone: break;
		}
		return nullptr;
	}
	// behind the last step: a search is still flagged — a candidate heap of one entry per node overflowed
	bool overflowed() const { return at_ == kDone && !step_.ids.empty(); }

private:
	enum At { kFirstPassDone, kCollectOverflows, kLdsMaxDone, kBigEf, kGlobal0, kGlobal1, kDone };

	const HnswRerunStep* emit(HnswRerunStep s) {   // (s.ids is empty: the ids collected so far stay the ladder's)
		s.ids.swap(step_.ids);
		step_ = std::move(s);
		return &step_;
	}
	// the step's ids that are still flagged stay (in order)
	void keep_overflowing(const uint32_t* counts) {
		step_.ids.erase(std::remove_if(step_.ids.begin(), step_.ids.end(), [counts](uint32_t q) { return counts[q] != kHnswOverflow; }), step_.ids.end());
	}
	// tier t over the step's ids: a bitset, the plan's LDS parameters, tier_cap[t] heap entries a search in global scratch — at most 1 GiB of
	// them per launch.  No second tier where both have one entry per node.
	const HnswRerunStep* global_tier(int t) {
		at_ = kDone;
		if (step_.ids.empty() || (t == 1 && pl_.tier_cap[1] == pl_.tier_cap[0])) return nullptr;
		at_ = t == 0 ? kGlobal0 : kGlobal1;
		const uint64_t slots = std::max<uint64_t>(1, std::min<uint64_t>(pl_.max_slots, (1ull << 30) / (pl_.tier_cap[t] * 8)));
		return emit({{}, t == 0 ? kHnswRungGlobal0 : kHnswRungGlobal1, slots, "hnsw_redo", 0, pl_.words, pl_.lds_cand_cap, pl_.vis_lds_log2, pl_.tier_cap[t]});
	}

	const HnswLaunchPlan& pl_;
	uint32_t nq_, helper_queued_;
	At at_;
	HnswRerunStep step_{};
};

}  // namespace rxgpu
