// The sorted list of the HNSW search: both of the reference's queues as ONE list in registers, spread over the lanes of a wavefront
// (HnswSortedList; HnswSortedListDel for graphs with deleted nodes).  Included by hnsw_search_core.hip.h.
#pragma once
#include "knn_kernels.hip.h"

namespace rxgpu {

// --- The fast path of a search over a graph without deleted nodes: BOTH queues as one sorted list spread over the lanes ---
// In a bare-bone search (hnswalg.h:873-876, 932-960) every candidate is pushed into top_candidates together with its push into
// candidate_set, so the live part of candidate_set is "the members of top_candidates that were not expanded yet": what top_candidates
// evicted lies at or above lowerBound for good, and popping it ends the search like an empty candidate_set does (at: see below).  One list of <= ef
// entries sorted by distance plus one "expanded" bit per entry therefore carries the whole Layer0SearchState: entry 64 s + l lives in
// slot s of lane l, an insertion is one ballot + one lane shift (wave_shr DPP) instead of two binary-heap sifts by one lane, the pop is a
// scalar find-first-zero.
// Equal distances.  With CompareByFirst heaps the reference's choice among EQUAL keys is whatever libstdc++'s sift loops leave on top,
// which a sorted list cannot know.  Where that choice cannot matter the list goes on; where it can, the search is flagged and starts
// over on the heaps (the code below the list's branch in hnsw_search_kernel; kHnswTie and a launch of its own if the launcher gave the
// workgroup no heap area):
//   * the popped candidate's key d equals the next unexpanded one's (which of the two the reference expands first is its heap's
//     secret) AND lowerBound has come down to d by the time every candidate with a key <= d is expanded.  While lowerBound stays above
//     d the order is immaterial: each node of key <= d that gets evaluated is admitted (key < lowerBound) and expanded before anything
//     farther, so both orders expand the same closure — "evaluated nodes of key <= d, and what their lists reach" —, top_candidates
//     is the ef smallest keys of the same evaluated set, and lowerBound in the other order is never below its value at the end of this
//     one (fewer keys seen, larger ef-th smallest).  The check is made when the first key > d is popped, or when the list runs dry;
//   * the popped key, or lowerBound when the list runs dry, equals the key of the last node that went OUTSIDE the list with a key equal
//     to lowerBound — evicted next to an equal maximum, or refused admission at dist == lowerBound: an evicted entry is still in the
//     reference's candidate_set, alive (dist > lowerBound is false) and due for expansion, and in another order of equal pops a refused
//     node is one that got in.  (Keys outside the list never lie below lowerBound, and lowerBound only falls: the last such key is the
//     only one that can still equal it.)
//   * entries k - 1 and k of the final list are equal (SearchKnn's trim to k pops one of them);
//   * a key is not finite.
// Everything else depends on keys alone: top_candidates is the multiset of the ef smallest keys seen, an eviction among equal maxima
// changes neither lowerBound nor candidate_set, and an equal key met in the middle of the list has no consequence until one of the
// events above.  (Flagging every equal key met on insertion re-ran 31 % of the queries of a 1M x 768 corpus: with 128 keys in a narrow
// band of float32 values a search of ~400 insertions meets one more often than not.)
__device__ __forceinline__ uint32_t wave_shr1(uint32_t x) {   // lane l <- lane l - 1 (lane 0 keeps its value)
	return uint32_t(__builtin_amdgcn_update_dpp(int(x), int(x), 0x138 /* wave_shr:1 */, 0xF, 0xF, false));
}
__device__ __forceinline__ float lane_value(float v, int l) { return __uint_as_float(uint32_t(__builtin_amdgcn_readlane(int(__float_as_uint(v)), l))); }
// The per-slot state of a list as VECTOR values, not arrays: an array member keeps the whole struct in scratch memory as soon as a loop
// over it is not unrolled before LLVM's SROA pass runs (seen for S = 3 and 4: 100 bytes of scratch per lane, every access a memory op).
template <int S>
struct HnswVec {
	typedef float f __attribute__((ext_vector_type(S)));
	typedef uint32_t u __attribute__((ext_vector_type(S)));
	typedef uint64_t m __attribute__((ext_vector_type(S)));
};
// entries >= pos move up by one (the last one falls off the registers), (nd, nid) lands at pos
template <int S>
__device__ __forceinline__ void sorted_shift_in(typename HnswVec<S>::f& d, typename HnswVec<S>::u& id, int pos, float nd, uint32_t nid, bool dpp, int lane) {
#pragma unroll
	for (int s = S - 1; s >= 0; --s) {
		if (pos >= 64 * (s + 1)) continue;   // uniform: the slot lies below the insertion point
		const int g = 64 * s + lane;
		float up_d;
		uint32_t up_i;
		if (dpp) {
			up_d = __uint_as_float(wave_shr1(__float_as_uint(d[s])));
			up_i = wave_shr1(id[s]);
		} else {   // RXGPU_HNSW_SORTED=2: the same shift through the LDS crossbar (ds_bpermute)
			up_d = __shfl_up(d[s], 1, 64);
			up_i = __shfl_up(id[s], 1, 64);
		}
		if (s > 0) {
			const float carry_d = lane_value(d[s > 0 ? s - 1 : 0], 63);
			const uint32_t carry_i = uint32_t(__builtin_amdgcn_readlane(int(id[s > 0 ? s - 1 : 0]), 63));
			if (lane == 0) {
				up_d = carry_d;
				up_i = carry_i;
			}
		}
		d[s] = g < pos ? d[s] : (g == pos ? nd : up_d);
		id[s] = g < pos ? id[s] : (g == pos ? nid : up_i);
	}
}
// the same for a wave-uniform bit per entry
template <int S>
__device__ __forceinline__ void mask_shift_in(typename HnswVec<S>::m& m, int pos, bool bit) {
#pragma unroll
	for (int s = S - 1; s >= 0; --s) {
		if (pos >= 64 * (s + 1)) continue;
		if (pos < 64 * s) {
			m[s] = (m[s] << 1) | (m[s > 0 ? s - 1 : 0] >> 63);
		} else {
			const uint64_t below = (1ull << (pos - 64 * s)) - 1ull;
			m[s] = (m[s] & below) | ((m[s] & ~below) << 1) | (uint64_t(bit) << (pos - 64 * s));
		}
	}
}
// (Two structs that repeat init, key_at, first_open and pop line for line, on purpose: with the shared part in one CRTP base — the same
// statements — 345 of the 399 kernels that hold a list came out as different machine code, tools/compare_kernel_isa.py.)
template <int S>
struct HnswSortedList {
	typename HnswVec<S>::f d;
	typename HnswVec<S>::u id;
	typename HnswVec<S>::m done;   // wave-uniform: bit l of word s = entry 64 s + l is expanded (or empty)
	int n;
	float lower;        // lowerBound: the largest key while the list is filling, entry ef - 1 afterwards
	float outside;      // key of the last node evicted, or refused at dist == lowerBound (NaN before the first: equal to nothing)
	float pend;         // largest key at which a pop met an equal unexpanded key and the verdict is still open
	bool pending;
	bool tie;
	bool dpp;

	__device__ __forceinline__ void init(bool use_dpp) {
		dpp = use_dpp;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			d[s] = __builtin_inff();
			id[s] = 0u;
			done[s] = ~0ull;
		}
		n = 0;
		lower = 3.402823466e+38f;
		outside = __builtin_nanf("");
		pend = 0.f;
		pending = false;
		tie = false;
	}
	// every candidate of key <= pend is expanded now: the order among the equal ones was immaterial iff lowerBound is still above pend
	// (a list that is not full admits everything, whatever lowerBound says)
	__device__ __forceinline__ void settle(int ef) {
		if (pending && n == ef && !(lower > pend)) tie = true;
		pending = false;
	}
	// key of entry e (wave-uniform e)
	__device__ __forceinline__ float key_at(int e) const {
		float v = d[0];
#pragma unroll
		for (int s = 1; s < S; ++s) v = (e >> 6) == s ? d[s] : v;
		return lane_value(v, e & 63);
	}
	// (nd, nid) wave-uniform; the caller has checked n < ef || lower > nd
	__device__ __forceinline__ void insert(float nd, uint32_t nid, int ef, int lane) {
		int pos = 0;
#pragma unroll
		for (int s = 0; s < S; ++s) pos += __popcll(__ballot(d[s] < nd));
		tie = tie || !(nd < __builtin_inff());
		if (n == ef) outside = lower;   // the list is full: its last entry leaves
		sorted_shift_in<S>(d, id, pos, nd, nid, dpp, lane);
		mask_shift_in<S>(done, pos, false);   // bit pos: 0 = not expanded
		if (n < ef) {
			++n;
		} else {
#pragma unroll
			for (int s = 0; s < S; ++s) {   // the evicted maximum sits at index ef now (if the registers reach that far): an empty entry again
				const bool here = (ef >> 6) == s;
				d[s] = (here && lane == (ef & 63)) ? __builtin_inff() : d[s];
				done[s] |= here ? 1ull << (ef & 63) : 0ull;
			}
		}
		lower = key_at(n - 1);
	}
	// the interface the kernel shares with HnswSortedListDel: members of top_candidates held, insertion with a delete mark (none here)
	__device__ __forceinline__ int held() const { return n; }
	__device__ __forceinline__ void insert(float nd, uint32_t nid, bool, int ef, int lane) { insert(nd, nid, ef, lane); }
	// first entry that was not expanded yet, -1 if none (selects over static slot numbers, no early exit: the arrays must stay in registers)
	__device__ __forceinline__ int first_open() const {
		int e = -1;
#pragma unroll
		for (int s = S - 1; s >= 0; --s) {
			const uint64_t o = ~done[s];
			e = o ? 64 * s + __builtin_ctzll(o) : e;
		}
		return e;
	}
	// the first unexpanded entry behind entry `after`, -1 if none
	__device__ __forceinline__ int next_open(int after) const {
		int e = -1;
#pragma unroll
		for (int s = S - 1; s >= 0; --s) {
			uint64_t o = ~done[s];
			if ((after >> 6) == s) o = (after & 63) == 63 ? 0ull : (o & (~0ull << ((after & 63) + 1)));
			if ((after >> 6) > s) o = 0ull;
			e = o ? 64 * s + __builtin_ctzll(o) : e;
		}
		return e;
	}
	// candidate_set.top() + pop(): the nearest entry that was not expanded yet
	__device__ __forceinline__ bool pop(uint32_t& node, float& dist, int ef) {
		const int e = first_open();
		if (e < 0) {
			settle(ef);
			return false;
		}
		uint32_t iv = id[0];
#pragma unroll
		for (int s = 1; s < S; ++s) iv = (e >> 6) == s ? id[s] : iv;
		dist = key_at(e);
		node = uint32_t(__builtin_amdgcn_readlane(int(iv), e & 63));
		if (pending && dist > pend) settle(ef);
#pragma unroll
		for (int s = 0; s < S; ++s) done[s] |= (e >> 6) == s ? 1ull << (e & 63) : 0ull;
		const int next = first_open();
		tie = tie || dist == outside;
		if (next >= 0 && key_at(next) == dist) {
			pend = pending ? fmaxf(pend, dist) : dist;
			pending = true;
		}
		return true;
	}
};

// The same list for a graph WITH deleted nodes (hnswalg.h:882-893, 943-957): a deleted node is a candidate like any other but never a
// member of top_candidates, lowerBound follows the LIVE entries only, the search stops on a far candidate only once ef live entries are
// held, and a deleted entry point enters candidate_set at FLT_MAX (initLayer0SearchState :853-856).  The list holds live and deleted
// entries in one order; `del` marks the deleted ones, `live` counts the others.  Once ef live entries are held everything behind the
// last of them is dead — deleted entries above lowerBound, the live entry a new one evicts — and leaves the list; `outside` takes the
// smallest key that leaves.  The equal-key rules are the bare list's, with "full" meaning live == ef; a list that runs out of registers
// (many deleted nodes in reach) flags the search like an equal key does.  tests/test_hnsw_sorted_model.py holds the Python restatement
// of both lists and runs it against the two-heap oracle.
template <int S>
struct HnswSortedListDel {
	static constexpr int kCap = 64 * S;
	typename HnswVec<S>::f d;
	typename HnswVec<S>::u id;
	typename HnswVec<S>::m done;   // wave-uniform: expanded (or empty)
	typename HnswVec<S>::m del;    // wave-uniform: the entry is a deleted node (0 for empty slots)
	int n, live;
	float lower, outside, pend;
	bool pending, tie, dpp;

	__device__ __forceinline__ void init(bool use_dpp) {
		dpp = use_dpp;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			d[s] = __builtin_inff();
			id[s] = 0u;
			done[s] = ~0ull;
			del[s] = 0ull;
		}
		n = live = 0;
		lower = 3.402823466e+38f;
		outside = __builtin_nanf("");
		pend = 0.f;
		pending = false;
		tie = false;
	}
	__device__ __forceinline__ float key_at(int e) const {
		float v = d[0];
#pragma unroll
		for (int s = 1; s < S; ++s) v = (e >> 6) == s ? d[s] : v;
		return lane_value(v, e & 63);
	}
	// bits of word s that belong to entries < count
	static __device__ __forceinline__ uint64_t below_count(int s, int count) {
		const int c = count - 64 * s;
		return c <= 0 ? 0ull : (c >= 64 ? ~0ull : ((1ull << c) - 1ull));
	}
	__device__ __forceinline__ int last_live() const {
		int e = -1;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			const uint64_t m = ~del[s] & below_count(s, n);
			e = m ? 64 * s + 63 - __builtin_clzll(m) : e;
		}
		return e;
	}
	__device__ __forceinline__ int held() const { return live; }
	__device__ __forceinline__ void settle(int ef) {
		if (pending && live == ef && !(lower > pend)) tie = true;
		pending = false;
	}
	// (nd, nid, isdel) wave-uniform; the caller has checked live < ef || lower > nd
	__device__ __forceinline__ void insert(float nd, uint32_t nid, bool isdel, int ef, int lane) {
		tie = tie || !(nd < __builtin_inff());
		const bool full = live == ef;
		if (n == kCap && !(full && !isdel)) {   // no register left for one more entry: the heaps take the search over
			tie = true;
			return;
		}
		int pos = 0;
#pragma unroll
		for (int s = 0; s < S; ++s) pos += __popcll(__ballot(d[s] < nd));
		const float old_lower = lower;
		sorted_shift_in<S>(d, id, pos, nd, nid, dpp, lane);
		mask_shift_in<S>(done, pos, false);
		mask_shift_in<S>(del, pos, isdel);
		const bool fell_off = n == kCap;   // only with a full top and a live newcomer: the entry that fell off was the largest live one
		if (!fell_off) ++n;
		if (!isdel) {
			if (!full) {
				++live;
			} else if (fell_off) {
				outside = old_lower;
			} else {   // the largest live entry leaves top_candidates: from here on it is one of the dead behind the last live entry
				const int gone = last_live();
				outside = key_at(gone);
#pragma unroll
				for (int s = 0; s < S; ++s) del[s] |= (gone >> 6) == s ? 1ull << (gone & 63) : 0ull;
			}
			if (live == ef) {   // everything behind the last live entry is dead now
				const int keep = last_live() + 1;
				if (keep < n) {
					outside = key_at(keep);   // the smallest key that leaves
#pragma unroll
					for (int s = 0; s < S; ++s) {
						const uint64_t stay = below_count(s, keep);
						d[s] = (64 * s + lane) >= keep ? __builtin_inff() : d[s];
						done[s] |= ~stay;
						del[s] &= stay;
					}
					n = keep;
				}
			}
		}
		if (live > 0) lower = key_at(last_live());
	}
	__device__ __forceinline__ int first_open() const {
		int e = -1;
#pragma unroll
		for (int s = S - 1; s >= 0; --s) {
			const uint64_t o = ~done[s];
			e = o ? 64 * s + __builtin_ctzll(o) : e;
		}
		return e;
	}
	__device__ __forceinline__ bool pop(uint32_t& node, float& dist, int ef) {
		const int e = first_open();
		if (e < 0) {
			settle(ef);
			return false;
		}
		uint32_t iv = id[0];
#pragma unroll
		for (int s = 1; s < S; ++s) iv = (e >> 6) == s ? id[s] : iv;
		dist = key_at(e);
		node = uint32_t(__builtin_amdgcn_readlane(int(iv), e & 63));
		if (pending && dist > pend) settle(ef);
#pragma unroll
		for (int s = 0; s < S; ++s) done[s] |= (e >> 6) == s ? 1ull << (e & 63) : 0ull;
		const int next = first_open();
		tie = tie || dist == outside;
		if (next >= 0 && key_at(next) == dist) {
			pend = pending ? fmaxf(pend, dist) : dist;
			pending = true;
		}
		return true;
	}
	// index of the r-th live entry (r < live)
	__device__ __forceinline__ int live_at(int r) const {
		int e = -1, seen = 0;
#pragma unroll
		for (int s = 0; s < S; ++s) {
			uint64_t m = ~del[s] & below_count(s, n);
			const int c = __popcll(m);
			if (e < 0 && r < seen + c) {
				for (int i = seen; i < r; ++i) m &= m - 1;   // drop the r - seen lowest set bits (wave-uniform loop)
				e = 64 * s + __builtin_ctzll(m);
			}
			seen += c;
		}
		return e;
	}
};

// The node of the nearest entry that is not expanded yet (what pop() would return next if nothing nearer is inserted before), or
// 0xFFFFFFFF: the search prefetches that node's link block while the current hop's distances are computed.
template <typename List, int S>
__device__ __forceinline__ uint32_t hnsw_peek_open(const List& list) {
	const int e = list.first_open();
	if (e < 0) return 0xFFFFFFFFu;
	uint32_t iv = list.id[0];
#pragma unroll
	for (int s = 1; s < S; ++s) iv = (e >> 6) == s ? list.id[s] : iv;
	return uint32_t(__builtin_amdgcn_readlane(int(iv), e & 63));
}

// the node of list entry e (wave-uniform e >= 0)
template <typename List, int S>
__device__ __forceinline__ uint32_t hnsw_node_at(const List& list, int e) {
	uint32_t iv = list.id[0];
#pragma unroll
	for (int s = 1; s < S; ++s) iv = (e >> 6) == s ? list.id[s] : iv;
	return uint32_t(__builtin_amdgcn_readlane(int(iv), e & 63));
}

}  // namespace rxgpu
