// The last kernel of the dense ft_fast train (ft_merge.hip tells the whole story): slots, entry rows and the per-document replay of one
// document range, the zeroed tables handed back to the next merge, and the result header.  The kernel at the end of this file reads as the
// list of its phases; each phase is a function above it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rxgpu_internal.h"
#include "knn_kernels.hip.h"
#include "ft_rank.hip.h"
#include "ft_scan.hip.h"
#include "ft_replay.hip.h"

namespace rxgpu {

__device__ __forceinline__ void ft_replay_step(FtPlanK& p, FtReplayState& st, uint32_t row, float r, uint8_t fld, uint32_t i, const uint64_t* const* s_fpos,
											   const uint32_t* const* s_pos_off, const uint32_t* s_qp, uint32_t sl, float& max_term_rank) {
	uint32_t qp = 0;
	FtPosList pos;
	if (!p.simple || p.max_areas) ft_replay_locate(p, row, i, s_fpos, s_pos_off, s_qp, qp, pos.ptr, pos.n);
	if (p.max_areas && __float_as_uint(r) != kFtSuppressedRank) ft_areas_of_posting(p, sl, pos.ptr, pos.n, r, max_term_rank);
	ft_replay_apply(p, st, r, fld, qp, pos);
}
// the document's row of the entry table, walked in sub-term order
__device__ __forceinline__ void ft_replay_doc(FtPlanK& p, uint32_t sl, uint32_t doc, const uint64_t* const* s_fpos, const uint32_t* const* s_pos_off,
											  const uint32_t* s_qp) {
	FtReplayState st;
	float max_term_rank = 0.f;   // AreasInDocument::maxTermRank_
	// Most documents meet ONE sub-term, a few two or three, out of many: each lane first collects WHICH of its rows are occupied (rank
	// loads, 64 rows per mask word) and then walks only those, in row order = the order mergeTerm met the postings.
	for (uint32_t row0 = 0; row0 < p.n_rows; row0 += 64) {
		unsigned long long occupied = 0;
		const uint32_t rows_here = p.n_rows - row0 < 64 ? p.n_rows - row0 : 64;
		for (uint32_t j0 = 0; j0 < rows_here; j0 += 8) {
			float ahead[8];
#pragma unroll
			for (uint32_t j = 0; j < 8; ++j) ahead[j] = j0 + j < rows_here ? p.e_rank[uint64_t(row0 + j0 + j) * p.max_merged + sl] : 0.0f;
#pragma unroll
			for (uint32_t j = 0; j < 8; ++j) occupied |= (unsigned long long)(ahead[j] != 0.0f) << (j0 + j);
		}
		while (occupied) {
			const uint32_t row = row0 + uint32_t(__ffsll((long long)occupied) - 1);
			occupied &= occupied - 1;
			const uint64_t cell = uint64_t(row) * p.max_merged + sl;
			ft_replay_step(p, st, row, p.e_rank[cell], p.e_field[cell], (p.simple && !p.max_areas) ? 0u : p.e_idx[cell], s_fpos, s_pos_off, s_qp, sl, max_term_rank);
		}
	}
	ft_replay_finish(p, st, sl, doc);
}

// The phases are forceinline functions over one struct of workgroup-uniform facts.  This is not the machine code of the one-function
// kernel it replaces (118 -> 126 VGPRs, 288 fewer lines, occupancy 4 and no scratch as before; tests/test_ft_kernel_resources.py holds
// the last two): on their own, ft_finish_compact() in place of the spelled-out rule and FtFinishLds::table() in place of the literal
// pointer choice each renumbered the whole kernel already, so the decomposition was accepted on timing — profiles/ft_units_ab.json, inside
// the parent's run-to-run spread on every leg.
//
// What the phases of ft_finish share: the workgroup's LDS and the facts that are uniform over it
struct FtFinishWg {
	uint32_t* lds;                       // the dynamic block, carved as FtFinishLds says (ft_merge_plan.h)
	const uint64_t* const* s_fpos;       // [kFtReplayRows] replay descriptors of the merged rows ...
	const uint32_t* const* s_pos_off;
	const uint32_t* s_qp;                // ... ft_row_qpw
	uint32_t* s_nadd;                    // a counter: keys of the sorted layout, then the documents a sparse bucket replays
	uint32_t (*s_red)[kFtFinishRows];    // [4][kFtFinishRows] per-wavefront partial sums
	uint32_t* s_rowbase;                 // [kFtFinishRows] slot of the first document of (row, this range) when own_bases
	uint32_t tid, range, d_begin;
	bool own_bases;                      // the table of ft_adders is small: every workgroup sums what lies in front of its own entries
	bool few_rows;                       // the compact layout
	uint4* rec;                          // the range's bucket of records ...
	uint32_t nw;                         // ... and their number; 0 when the mergeLimit cut leaves the range nothing to do
};
__device__ __forceinline__ uint32_t ft_finish_base(FtPlanK& p, const FtFinishWg& c, uint32_t row) {
	return c.own_bases ? c.s_rowbase[row] : p.adders[uint64_t(row) * p.n_ranges + c.range];
}

// ---- row bases (own_bases): tv = the thread's entries of ft_adders' table, fetched with everything else up front; the table goes into the
// LDS area that is idle until the slots are set up.  base(row) = every entry of the rows before it + this row's entries left of the range:
// one wavefront per row adds up (row total, part left of the range).  (Loops that consumed each load before issuing the next paid a memory
// round trip per row or per column chunk: 7-10 us; testing every entry against every row's position in registers: 9 us of VALU work.)
__device__ __forceinline__ void ft_finish_own_bases(FtPlanK& p, const FtFinishWg& c, const uint32_t (&tv)[kFtRangeDocs / 256]) {
	const uint32_t tid = c.tid;
	uint32_t* s_table = c.lds + FtFinishLds::table(c.few_rows);
	if (c.own_bases) {
		const uint32_t total = p.n_rows * p.n_ranges;
#pragma unroll
		for (uint32_t k = 0; k < kFtRangeDocs / 256; ++k) {
			if (k * 256 + tid < total) s_table[k * 256 + tid] = tv[k];
		}
	}
	__syncthreads();
	if (c.own_bases) {
		const uint32_t lane = tid & 63;
		for (uint32_t r = tid >> 6; r < p.n_rows; r += 4) {
			uint32_t rs = 0, ps = 0;
			for (uint32_t col = lane; col < p.n_ranges; col += 64) {
				const uint32_t x = s_table[r * p.n_ranges + col];
				rs += x;
				ps += col < c.range ? x : 0u;
			}
			rs = wave_sum(rs);
			ps = wave_sum(ps);
			if (lane == 0) {
				c.s_red[0][r] = rs;
				c.s_red[1][r] = ps;
			}
		}
	}
	__syncthreads();
	if (c.own_bases && tid == 0) {
		uint32_t before_rows = 0;
		for (uint32_t r = 0; r < p.n_rows; ++r) {
			c.s_rowbase[r] = before_rows + c.s_red[1][r];
			before_rows += c.s_red[0][r];
		}
	}
	__syncthreads();
}

// ---- the mergeLimit cut (addDoc until maxMergedDocs): slots ascend with (row, range), so when even the first slot of every row of this
// range lies at or beyond the limit none of its documents is merged — a whole-corpus single-term merge adds its 20 000 documents in
// the first dozen ranges, and the other six hundred have nothing to sort, scatter or replay
__device__ __forceinline__ bool ft_finish_reaches(FtPlanK& p, const FtFinishWg& c) {
	bool reaches = false;
	for (uint32_t r = c.tid; r < p.n_rows; r += 256) reaches = reaches || ft_finish_base(p, c, r) < p.max_merged;
	return __syncthreads_or(reaches ? 1 : 0) != 0;
}

// ---- slots, up to kFtBitmapRows merged sub-terms: no sort.  s_slot[doc] = first row, then the slot (16 bits: max_merged < 65535, a slot at
// or beyond it means "never merged" and is stored as 0xFFFF); one bitmap of the range's documents per row marks the first
// postings, a prefix over the bitmap words gives every one its rank inside (row, range)
__device__ __forceinline__ void ft_finish_slots_by_bitmaps(FtPlanK& p, const FtFinishWg& c) {
	const uint32_t tid = c.tid;
	uint32_t* s_slot = c.lds + FtFinishLds::slot;   // [kFtRangeDocs] halves
	uint32_t* s_bits = c.lds + FtFinishLds::bits;   // [kFtBitmapRows][256]
	uint32_t* s_pref = c.lds + FtFinishLds::pref;   // [kFtBitmapRows][256]
	// (the table of ft_adders lay here: dead since the barrier behind the row bases)
	for (uint32_t w = tid; w < kFtRangeDocs / 2; w += 256) s_slot[w] = 0xFFFFFFFFu;
	for (uint32_t w = tid; w < FtFinishLds::kBitmapWords; w += 256) s_bits[w] = 0;
	__syncthreads();
	FT_STAMP(p, 33);
	// the range's first postings; the record remembers that it adds its document
	ft_first_postings(c.rec, c.nw, s_slot, tid, [&] { FT_STAMP(p, 34); }, [&](uint32_t e, const uint4& r, uint32_t row, uint32_t dl) {
		atomicOr(&s_bits[row * (kFtRangeDocs / 32) + (dl >> 5)], 1u << (dl & 31));
		c.rec[e].w = r.w | 0x80000000u;
	});
	__syncthreads();
	FT_STAMP(p, 35);
	{   // exclusive prefix of the popcounts along every bitmap: thread t owns word t
		uint32_t cnt[kFtBitmapRows], incl[kFtBitmapRows];
#pragma unroll
		for (uint32_t r = 0; r < kFtBitmapRows; ++r) {
			cnt[r] = r < p.n_rows ? __popc(s_bits[r * (kFtRangeDocs / 32) + tid]) : 0u;
			incl[r] = wave_inclusive_scan(cnt[r], int(tid & 63));
			if ((tid & 63) == 63) c.s_red[tid >> 6][r] = incl[r];
		}
		__syncthreads();
#pragma unroll
		for (uint32_t r = 0; r < kFtBitmapRows; ++r) {
			uint32_t excl = incl[r] - cnt[r];
			for (uint32_t w = 0; w < (tid >> 6); ++w) excl += c.s_red[w][r];
			s_pref[r * (kFtRangeDocs / 32) + tid] = excl;
		}
	}
	__syncthreads();
	FT_STAMP(p, 36);
	for (uint32_t e = tid; e < c.nw; e += 256) {   // first posting -> slot of its document
		const uint4 r = c.rec[e];
		if (!(r.w >> 31)) continue;
		const uint32_t row = r.w & 0xFFFFu, dl = r.x & (kFtRangeDocs - 1);
		const uint32_t word = row * (kFtRangeDocs / 32) + (dl >> 5);
		const uint32_t rank = s_pref[word] + __popc(s_bits[word] & ((1u << (dl & 31)) - 1u));
		const uint32_t slot = ft_finish_base(p, c, row) + rank;
		lds_set_u16(s_slot, dl, slot < 0xFFFFu ? slot : 0xFFFFu);   // every document with an unsuppressed record has exactly one first posting (the others keep 0xFFFF: never merged)
		if (slot < p.max_merged) p.out_doc[slot] = c.d_begin + dl;
	}
	__syncthreads();
	FT_STAMP(p, 37);
}

// ---- slots, many sub-terms: 16-bit document table + a sorted list of (row, document) keys
__device__ __forceinline__ void ft_finish_slots_by_sort(FtPlanK& p, const FtFinishWg& c) {
	const uint32_t tid = c.tid;
	uint32_t* s_tab = c.lds + FtFinishLds::tab;     // [kFtRangeDocs] halves
	uint32_t* s_keys = c.lds + FtFinishLds::keys;   // [kFtRangeDocs]
	for (uint32_t w = tid; w < kFtRangeDocs / 2; w += 256) s_tab[w] = 0xFFFFFFFFu;
	__syncthreads();
	FT_STAMP(p, 33);
	// the range's first postings: key (row, document); the record remembers that it adds
	ft_first_postings(c.rec, c.nw, s_tab, tid, [&] { FT_STAMP(p, 34); }, [&](uint32_t e, const uint4& r, uint32_t row, uint32_t dl) {
		s_keys[atomicAdd(c.s_nadd, 1u)] = (row << kFtRangeShift) | dl;
		c.rec[e].w = r.w | 0x80000000u;
	});
	__syncthreads();
	FT_STAMP(p, 35);
	const uint32_t A = *c.s_nadd;   // <= kFtRangeDocs: one per document
	uint32_t N = 2;
	while (N < A) N <<= 1;
	for (uint32_t q = A + tid; q < N; q += 256) s_keys[q] = 0xFFFFFFFFu;
	__syncthreads();
	for (uint32_t k = 2; k <= N; k <<= 1) {   // bitonic sort, ascending
		for (uint32_t j = k >> 1; j > 0; j >>= 1) {
			for (uint32_t t = tid; t < N / 2; t += 256) {
				const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
				const uint32_t x = s_keys[i], y = s_keys[l];
				if ((x > y) == ((i & k) == 0)) {
					s_keys[i] = y;
					s_keys[l] = x;
				}
			}
			__syncthreads();
		}
	}
	FT_STAMP(p, 36);
	// rank inside the row = position - first position of the row (binary search); parked in the document table, whose first-row
	// entries are no longer needed
	for (uint32_t q = tid; q < A; q += 256) {
		const uint32_t key = s_keys[q], first_of_row = key & ~(kFtRangeDocs - 1);
		uint32_t lo = 0, hi = q;   // lower bound of first_of_row in [0, q]
		while (lo < hi) {
			const uint32_t mid = (lo + hi) >> 1;
			if (s_keys[mid] < first_of_row) {
				lo = mid + 1;
			} else {
				hi = mid;
			}
		}
		lds_set_u16(s_tab, key & (kFtRangeDocs - 1), q - lo);
	}
	__syncthreads();
	FT_STAMP(p, 37);
	for (uint32_t q = tid; q < A; q += 256) {   // key -> slot; document -> its position in the list
		const uint32_t key = s_keys[q], row = key >> kFtRangeShift, dl = key & (kFtRangeDocs - 1);
		const uint32_t slot = ft_finish_base(p, c, row) + lds_get_u16(s_tab, dl);
		s_keys[q] = slot;
		lds_set_u16(s_tab, dl, q);
		if (slot < p.max_merged) p.out_doc[slot] = c.d_begin + dl;
	}
	__syncthreads();
}

// the merge slot of document `dl` of the range, in either layout (a document whose only records are a suppressed sub-term's has no first
// posting: slot 0xFFFFFFFF = never merged)
__device__ __forceinline__ uint32_t ft_finish_slot_of(const FtFinishWg& c, uint32_t dl) {
	if (c.few_rows) {
		const uint32_t v = lds_get_u16(c.lds + FtFinishLds::slot, dl);
		return v == 0xFFFFu ? 0xFFFFFFFFu : v;
	}
	const uint32_t at = lds_get_u16(c.lds + FtFinishLds::tab, dl);
	return at == 0xFFFFu ? 0xFFFFFFFFu : (c.lds + FtFinishLds::keys)[at];
}

// ---- replay of a sparse bucket (the usual one after a preselect: a few hundred records): the records go into LDS and the thread of every
// first posting collects its document's other postings from there — no entry rows in global memory, i.e. no scatter, no gather
// chain in front of the position loads, nothing to hand back zeroed.  A document with more than kFtSparsePostings postings
// sends the whole range down the general path: returns true when the general path has to redo the range.
__device__ __forceinline__ bool ft_finish_replay_sparse(FtPlanK& p, const FtFinishWg& c) {
	const uint32_t tid = c.tid, nw = c.nw, d_begin = c.d_begin;
	// behind the slots of the bitmap layout; in the sorted layout the list of slots is no longer than the bucket, i.e. ends in front
	uint32_t* sparse_base = c.lds + FtFinishLds::sparse(c.few_rows);
	uint4* s_rec = reinterpret_cast<uint4*>(sparse_base + FtFinishLds::sparse_rec);   // [kFtSparseRecords]; .x = document in the range | next record << 13
	uint32_t* s_head = sparse_base + FtFinishLds::sparse_head;   // [kHeads] first record of the documents with these low bits
	constexpr uint32_t kHeads = kFtSparseHeads, kNil = 1023;
	uint16_t* s_todo = reinterpret_cast<uint16_t*>(sparse_base + FtFinishLds::sparse_todo);   // [kFtSparseRecords] the first postings of the documents to replay
	for (uint32_t w = tid; w < kHeads; w += 256) s_head[w] = kNil;
	if (tid == 0) *c.s_nadd = 0;
	__syncthreads();
	for (uint32_t e = tid; e < nw; e += 256) {   // the documents' records chained through the copy; one thread per document to replay
		uint4 r = c.rec[e];
		const uint32_t dl = r.x & (kFtRangeDocs - 1);
		r.x = dl | (atomicExch(&s_head[dl & (kHeads - 1)], e) << kFtRangeShift);
		s_rec[e] = r;
		if ((r.w >> 31) && ft_finish_slot_of(c, dl) < p.max_merged) s_todo[atomicAdd(c.s_nadd, 1u)] = uint16_t(e);
	}
	__syncthreads();
	FT_STAMP(p, 38);
	const uint32_t todo = *c.s_nadd;
	const FtTermCfg& t0 = p.terms[0];
	const bool one_field = t0.num_fields == 1;
	int over = 0;
	for (uint32_t q = tid; q < todo; q += 256) {
		const uint32_t dl = s_rec[s_todo[q]].x & (kFtRangeDocs - 1);
		float words0 = 0.f;
		if (one_field) words0 = t0.words[d_begin + dl];   // in flight during the walk
		// the document's postings: keys (sub-term row, record) collected along the chain, ordered by a sorting network
		uint32_t key[kFtSparsePostings];
#pragma unroll
		for (uint32_t k = 0; k < kFtSparsePostings; ++k) key[k] = 0xFFFFFFFFu;
		uint32_t cnt = 0;
		for (uint32_t j = s_head[dl & (kHeads - 1)]; j != kNil;) {
			const uint4 o = s_rec[j];
			if ((o.x & (kFtRangeDocs - 1)) == dl) {
				const uint32_t v = ((o.w & 0xFFFFu) << 16) | j;
#pragma unroll
				for (uint32_t k = 0; k < kFtSparsePostings; ++k) key[k] = cnt == k ? v : key[k];
				++cnt;
			}
			j = o.x >> kFtRangeShift;
		}
		if (cnt > kFtSparsePostings) {
			over = 1;
			continue;
		}
#define RX_CSWAP(a, b)                                \
	{                                                 \
		const uint32_t lo = key[a] < key[b] ? key[a] : key[b]; \
		const uint32_t hi = key[a] < key[b] ? key[b] : key[a]; \
		key[a] = lo;                                  \
		key[b] = hi;                                  \
	}
		static_assert(kFtSparsePostings == 6, "the network below orders six keys");
		RX_CSWAP(0, 5) RX_CSWAP(1, 3) RX_CSWAP(2, 4) RX_CSWAP(1, 2) RX_CSWAP(3, 4) RX_CSWAP(0, 3) RX_CSWAP(2, 5) RX_CSWAP(0, 1) RX_CSWAP(2, 3)
		RX_CSWAP(4, 5) RX_CSWAP(1, 2) RX_CSWAP(3, 4)
#undef RX_CSWAP
		// everything the walk will read is requested first: the position ranges of all the postings are in flight together
		float pr[kFtSparsePostings];
		uint8_t pf[kFtSparsePostings];
		uint32_t pq[kFtSparsePostings];
		const uint64_t* pp[kFtSparsePostings];
		uint32_t pn[kFtSparsePostings];
#pragma unroll
		for (uint32_t k = 0; k < kFtSparsePostings; ++k) {   // in sub-term order = the order mergeTerm met the postings
			pr[k] = 0.f;
			pf[k] = 0;
			pq[k] = 0;
			pp[k] = nullptr;
			pn[k] = 0;
			if (k >= cnt) continue;
			const uint4 o = s_rec[key[k] & 0xFFFFu];
			pr[k] = __uint_as_float(o.z);
			pf[k] = uint8_t((o.w >> 16) & 0xFFu);
			if (!p.simple || p.max_areas) ft_replay_locate(p, key[k] >> 16, o.y, c.s_fpos, c.s_pos_off, c.s_qp, pq[k], pp[k], pn[k]);
		}
		if (p.max_areas) {   // MergeDataAreas: the document's areas from its postings in merge order (before the ranks: independent of them)
			float max_term_rank = 0.f;
			const uint32_t sl_a = ft_finish_slot_of(c, dl);
#pragma unroll
			for (uint32_t k = 0; k < kFtSparsePostings; ++k) {
				if (k < cnt && __float_as_uint(pr[k]) != kFtSuppressedRank) ft_areas_of_posting(p, sl_a, pp[k], pn[k], pr[k], max_term_rank);
			}
		}
		uint32_t longest = 0;
#pragma unroll
		for (uint32_t k = 0; k < kFtSparsePostings; ++k) longest = pn[k] > longest ? pn[k] : longest;
		if (cnt > 1 && longest <= 4) {
			// ... and so are the positions (up to four per posting, the usual case): the walk, which compares the lists of two
			// consecutive terms at a time, then runs on registers instead of paying one memory round trip per posting
			FtPosRegs lists[kFtSparsePostings];
#pragma unroll
			for (uint32_t k = 0; k < kFtSparsePostings; ++k) {
				lists[k].n = pn[k];
#pragma unroll
				for (uint32_t i = 0; i < 4; ++i) lists[k].v[i] = i < pn[k] ? pp[k][i] : 0ull;
			}
			FtReplayStateT<FtPosRegs> st;
#pragma unroll
			for (uint32_t k = 0; k < kFtSparsePostings; ++k) {
				if (k < cnt) ft_replay_apply(p, st, pr[k], pf[k], pq[k], lists[k]);
			}
			ft_replay_finish(p, st, ft_finish_slot_of(c, dl), d_begin + dl, one_field, words0);
		} else {
			FtReplayState st;
#pragma unroll
			for (uint32_t k = 0; k < kFtSparsePostings; ++k) {
				FtPosList pos;
				pos.ptr = pp[k];
				pos.n = pn[k];
				if (k < cnt) ft_replay_apply(p, st, pr[k], pf[k], pq[k], pos);
			}
			ft_replay_finish(p, st, ft_finish_slot_of(c, dl), d_begin + dl, one_field, words0);
		}
	}
	return __syncthreads_or(over) != 0;   // a document with more postings than the network orders
}

// ---- the general replay: every posting of a merged document into the document's row of the entry table (column = its sub-term), the
// documents replayed from there, and the rows handed back ZEROED: the occupancy test of the next merge relies on it
__device__ __forceinline__ void ft_finish_replay_general(FtPlanK& p, const FtFinishWg& c) {
	const uint32_t tid = c.tid, nw = c.nw;
	FT_STAMP(p, 38);
	for (uint32_t e = tid; e < nw; e += 256) {
		const uint4 r = c.rec[e];
		const uint32_t sl = ft_finish_slot_of(c, r.x & (kFtRangeDocs - 1));
		if (sl >= p.max_merged) continue;   // met after the limit was hit: never added
		const uint64_t cell = uint64_t(r.w & 0xFFFFu) * p.max_merged + sl;
		p.e_rank[cell] = __uint_as_float(r.z);
		p.e_idx[cell] = r.y;
		p.e_field[cell] = uint8_t((r.w >> 16) & 0xFFu);
	}
	__syncthreads();   // the rows are read back by this workgroup only
	FT_STAMP(p, 39);
	for (uint32_t e = tid; e < nw; e += 256) {
		const uint4 r = c.rec[e];
		if (!(r.w >> 31)) continue;
		const uint32_t sl = ft_finish_slot_of(c, r.x & (kFtRangeDocs - 1));
		if (sl < p.max_merged) ft_replay_doc(p, sl, r.x, c.s_fpos, c.s_pos_off, c.s_qp);
	}
	__syncthreads();
	for (uint32_t e = tid; e < nw; e += 256) {
		const uint4 r = c.rec[e];
		const uint32_t sl = ft_finish_slot_of(c, r.x & (kFtRangeDocs - 1));
		if (sl < p.max_merged) p.e_rank[uint64_t(r.w & 0xFFFFu) * p.max_merged + sl] = 0.0f;
	}
}

// ---- the last workgroup of the grid writes the result header and leaves the synchronisation words clean for the next merge
__device__ __forceinline__ void ft_finish_publish(FtPlanK& p, const FtFinishWg& c) {
	const uint32_t tid = c.tid;
	if (c.own_bases) {   // the number of merged documents = the whole table, cut at maxMergedDocs (ft_slot_bases did not run)
		const uint64_t total = uint64_t(p.n_rows) * p.n_ranges;
		uint32_t sum = 0;
		for (uint64_t j = tid; j < total; j += 256) sum += p.adders[j];
		sum = wave_sum(sum);
		if ((tid & 63) == 0) c.s_red[tid >> 6][0] = sum;
		__syncthreads();
		if (tid == 0) {
			const uint32_t all = c.s_red[0][0] + c.s_red[1][0] + c.s_red[2][0] + c.s_red[3][0];
			p.sync[kFtSyncNumDocs] = all < p.max_merged ? all : p.max_merged;
		}
	}
	if (tid == 0) {
		p.out_header[0] = p.sync[kFtSyncNumDocs];
		p.out_header[1] = p.sync[kFtSyncError];
		p.out_header[2] = ft_preselect_on(p) ? 1u : 0u;
		p.out_header[3] = 0;
	}
	__syncthreads();
	if (tid < kFtSyncWords) p.sync[tid] = 0;
}

// Slots, entry rows and the per-document replay of one document range.  Dynamic LDS (FtFinishLds, ft_merge_plan.h): the 16-bit document
// table (first row, then the position in the sorted key list) followed by the key list of the range's first postings ((row << 13 |
// document), then the slot); or, in the compact layout, 16-bit slots and per-row bitmaps.
__global__ __launch_bounds__(256) void ft_finish(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	extern __shared__ uint32_t ft_finish_lds[];
	__shared__ const uint64_t* s_fpos[kFtReplayRows];
	__shared__ const uint32_t* s_pos_off[kFtReplayRows];
	__shared__ uint32_t s_qp[kFtReplayRows];   // ft_row_qpw
	__shared__ uint32_t s_nadd, s_last;
	__shared__ uint32_t s_red[4][kFtFinishRows], s_rowbase[kFtFinishRows];
	const uint32_t tid = threadIdx.x, range = blockIdx.x + p.range_begin;
	FtFinishWg c{ft_finish_lds, s_fpos, s_pos_off, s_qp, &s_nadd, s_red, s_rowbase, tid, range, range << kFtRangeShift, ft_own_bases(p), ft_finish_compact(p), nullptr, 0u};
	FT_STAMP(p, 32);
	// everything the workgroup fetches unconditionally is issued together: record count and bucket offset, the replay descriptors, and
	// (own_bases) the whole table of ft_adders
	const uint32_t n = p.bucket_cnt[range];
	const uint32_t bucket_off = p.bucket_off[range];
	uint32_t tv[kFtRangeDocs / 256];
	if (c.own_bases) {
		const uint32_t total = p.n_rows * p.n_ranges;
#pragma unroll
		for (uint32_t k = 0; k < kFtRangeDocs / 256; ++k) tv[k] = k * 256 + tid < total ? p.adders[k * 256 + tid] : 0u;
	}
	for (uint32_t row = tid; row < p.n_rows && row < kFtReplayRows; row += 256) {   // two dependent loads per row, once per workgroup
		const FtPosSubterm& s = p.subs[p.merge_grid[row].sub];
		s_fpos[row] = s.fpos;
		s_pos_off[row] = s.pos_off;
		s_qp[row] = ft_row_qpw(s);
	}
	if (n) {
		if (tid == 0) s_nadd = 0;
		ft_finish_own_bases(p, c, tv);
		c.nw = ft_finish_reaches(p, c) ? n : 0u;
		c.rec = p.b_rec + bucket_off;
		if (c.few_rows) {
			ft_finish_slots_by_bitmaps(p, c);
		} else {
			ft_finish_slots_by_sort(p, c);
		}
		if (c.nw > kFtSparseRecords || ft_finish_replay_sparse(p, c)) ft_finish_replay_general(p, c);
	}
	// ---- leave the shared tables clean for the next merge; the last workgroup writes the result header
	__syncthreads();
	FT_STAMP(p, 40);
	if (tid == 0) {
		if (n) p.bucket_cnt[range] = 0;
		// no release: the last workgroup reads nothing the others wrote in this kernel (header values come from the kernels before)
		s_last = atomicAdd(&p.sync[kFtSyncDoneFinish], 1u) == gridDim.x - 1 ? 1u : 0u;
	}
	__syncthreads();
	FT_STAMP(p, 41);
	if (s_last) ft_finish_publish(p, c);
}

// grid.y = query; lds_bytes: FtFinishLds::bytes when any query of the batch needs the sorted layout, bytes_few otherwise (ft_train_launch)
hipError_t launch_ft_finish(const FtPlan* plans, uint32_t ranges, uint32_t nq, size_t lds_bytes, hipStream_t st) {
	static std::atomic<uint64_t> raised{0};
	if (hipError_t e = raise_dynamic_lds_once(raised, reinterpret_cast<const void*>(&ft_finish), FtFinishLds::bytes); e != hipSuccess) return e;
	hipLaunchKernelGGL(ft_finish, dim3(ranges, nq), dim3(256), lds_bytes, st, plans);
	return hipSuccess;
}

}  // namespace rxgpu
