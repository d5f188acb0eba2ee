// The document-side front of the dense ft_fast train (ft_merge.hip tells the whole story): the restricting bitmask with its synonym half,
// the pre-score with its histogram, and the preselect's cut at the threshold score.  One workgroup per range of kFtRangeDocs documents.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rxgpu_internal.h"
#include "knn_kernels.hip.h"
#include "ft_rank.hip.h"
#include "ft_scan.hip.h"
#include "ft_replay.hip.h"

namespace rxgpu {

// buildRestrictingBitmask's synonym half (mergerimpl.h:347-361): for every AND part with multi-word synonyms, the documents that hold EVERY
// term of ONE of its synonyms (calcTermBitmask per term :252-274: any occurrence with a relevant field; AccumulateAnd over the synonym's
// terms; OR over the part's synonyms).  One workgroup per range of kFtRangeDocs documents, bitmaps in LDS; runs in front of ft_ranges only
// when the query has such parts.
__global__ __launch_bounds__(256) void ft_syn_masks(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	constexpr uint32_t kWords = kFtRangeDocs / 32;
	__shared__ uint32_t s_or[kWords], s_and[kWords], s_tmp[kWords];
	const uint32_t tid = threadIdx.x, range = blockIdx.x;
	const uint64_t d_begin = uint64_t(range) * kFtRangeDocs;
	for (uint32_t j = 0; j < p.n_syn_jobs; ++j) {
		const FtSynMaskJob job = p.syn_jobs[j];
		for (uint32_t w = tid; w < kWords; w += 256) s_or[w] = 0;
		for (uint32_t k = job.syn_begin; k < job.syn_end; ++k) {
			const FtSynonym syn = p.syns[p.job_syns[k]];
			for (uint32_t w = tid; w < kWords; w += 256) s_and[w] = 0xFFFFFFFFu;
			for (uint32_t t = syn.term_begin; t < syn.term_end; ++t) {
				const FtTermCfg& term = p.terms[t];
				for (uint32_t w = tid; w < kWords; w += 256) s_tmp[w] = 0;
				__syncthreads();
				for (uint32_t si = term.sub_begin; si < term.sub_end; ++si) {
					const FtPosSubterm& sub = p.subs[si];
					const uint32_t lo = ft_seg_lo(sub, range);
					const uint32_t hi = ft_seg_hi(sub, range);
					for (uint32_t i = lo + tid; i < hi; i += 256) {
						bool rel = term.all_pos_boost != 0;
						if (!rel) {   // checkFieldsRelevance (phrasemergerimpl.h:93-125)
							for (uint32_t e = sub.ent_off[i], e1 = sub.ent_off[i + 1]; e < e1 && !rel; ++e) rel = term.field_boost[sub.ent_field[e]] != 0.0f;
						}
						if (rel) {
							const uint32_t local = uint32_t(sub.doc[i] - d_begin);
							atomicOr(&s_tmp[local >> 5], 1u << (local & 31));
						}
					}
				}
				__syncthreads();
				for (uint32_t w = tid; w < kWords; w += 256) s_and[w] &= s_tmp[w];
			}
			__syncthreads();
			if (syn.term_end > syn.term_begin) {   // (AccumulateAnd over no term leaves an empty mask: nothing to OR)
				for (uint32_t w = tid; w < kWords; w += 256) s_or[w] |= s_and[w];
			}
			__syncthreads();
		}
		for (uint32_t w = tid; w < kWords; w += 256) {
			const uint64_t gw = d_begin / 32 + w;
			if (gw < p.nwords) job.out[gw] = s_or[w];
		}
		__syncthreads();
	}
}

// One workgroup per range of kFtRangeDocs documents; everything below lives in LDS until the range's mask words / scores are written.
//   restrictingMask_ = ~docsExcluded_ (mergerimpl.h:328-330; bits past total_docs stay 0 so that the popcount is exact)
//   AND term   calcTermBitmask (:252-274): any occurrence with a relevant field (checkFieldsRelevance, phrasemergerimpl.h:93-125); mask &= it
//   NOT term   excludeTermFromBitmask (:276-287)
//   pre-score  calcTermScores (:289-324) for every term that is not a NOT, when the host half of the 2-phase gate held: the first sub-term
//              (SortSubterms order) with a positive field boost adds min(proc16, 65535 / 4), saturating at 65535; then (:416-423) documents
//              outside the mask / removed score 0 and the rest is histogrammed
constexpr uint32_t kFtRangeSubs = 128;   // sub-terms whose segment, list pointer and proc are staged in LDS (more: read from HBM)
constexpr uint32_t kFtHistRep = 8;       // counters per key of the LDS score histogram (on distinct banks)
// LDS per workgroup ~30 KB -> 5 workgroups per CU.  The kernel is a chain of dependent phases (range index, posting stage, terms behind
// barriers, mask, scores, histogram): with Q queries in one grid its throughput is the number of workgroups a CU holds.  (512 staged
// sub-terms and 16 counters per key cost 48.6 KB = 3 per CU; queries with more than 128 sub-terms read the rest of their plan from HBM.)
constexpr uint32_t kFtStageBlocks = 32;  // 256-posting blocks of the range prefetched into registers (one posting per thread and block)
// the kernel's tail (defined behind it): masked scores out, their histogram
__device__ __forceinline__ void ft_ranges_histogram(FtPlanK& p, uint32_t tid, uint32_t range, uint64_t d_begin, uint32_t docs_here, const uint32_t (&rm8)[kFtRangeDocs / 4 / 256],
													 const uint32_t* s_mask, uint16_t* s_score, uint32_t* s_keys, uint32_t* s_rep);
__global__ __launch_bounds__(256, 5) void ft_ranges(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	constexpr uint32_t kWords = kFtRangeDocs / 32;
	__shared__ uint32_t s_mask[kWords], s_term[kWords];
	__shared__ uint16_t s_score[kFtRangeDocs];
	__shared__ uint32_t s_keys[256], s_part[4];
	__shared__ uint32_t s_lo[kFtRangeSubs], s_hi[kFtRangeSubs], s_blk0[kFtRangeSubs + 1];
	__shared__ const uint32_t* s_docptr[kFtRangeSubs];
	__shared__ float s_proc[kFtRangeSubs];
	struct BlockInfo {            // one 256-posting block of a staged sub-term's segment
		const uint32_t* first;    // &doc[lo + 256 k]
		uint32_t count;           // postings in the block (1..256)
		uint32_t pad;
	};
	__shared__ __attribute__((aligned(16))) BlockInfo s_binfo[kFtStageBlocks];
	__shared__ __attribute__((aligned(16))) uint32_t s_rep[256 * kFtHistRep];   // score histogram: kFtHistRep counters per key (after the term pass)
	// During the term pass the same space holds one byte per document: the number (+1) of the last term that scored it.  "Already scored in
	// this term" is then a plain byte compare — documents are unique inside a sub-term and sub-terms sit behind barriers, so no two threads
	// touch one byte — where a bit set took an LDS atomic with return per posting: at 6400 postings per range and three ranges per CU the
	// atomics alone were ~10 us of this kernel.
	uint8_t* s_scored = reinterpret_cast<uint8_t*>(s_rep);   // [kFtRangeDocs]
	static_assert(sizeof(s_rep) >= kFtRangeDocs, "one byte per document fits the counter space");
	const uint32_t tid = threadIdx.x, range = blockIdx.x + p.range_begin;   // (a document-range shard runs its own ranges only)
	FT_STAMP(p, 0);
	const uint64_t d_begin = uint64_t(range) * kFtRangeDocs;
	const uint32_t docs_here = uint32_t(p.total_docs - d_begin < kFtRangeDocs ? p.total_docs - d_begin : kFtRangeDocs);
	for (uint32_t w = tid; w < kWords; w += 256) {
		const uint32_t d0 = w * 32;
		uint32_t bits = 0;
		if (d0 < docs_here) {
			const uint32_t cnt = docs_here - d0 < 32 ? docs_here - d0 : 32;
			if (!p.excluded) {
				bits = cnt == 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u);
			} else {
				for (uint32_t b = 0; b < cnt; ++b) bits |= (p.excluded[d_begin + d0 + b] ? 0u : 1u) << b;
			}
		}
		s_mask[w] = bits;
	}
	if (p.prescore) {
		for (uint32_t i = tid; i < kFtRangeDocs / 2; i += 256) reinterpret_cast<uint32_t*>(s_score)[i] = 0;
		for (uint32_t i = tid; i < kFtRangeDocs / 4; i += 256) reinterpret_cast<uint32_t*>(s_scored)[i] = 0;
		s_keys[tid] = 0;   // a score of 0 is never inserted
	}
	// this range's segment [lo, hi) of every posting list, fetched up front (two dependent loads each, all in flight together); the merged
	// postings in front of the range = where its bucket of surviving postings starts (ft_rank_all)
	uint32_t before = 0;
	for (uint32_t si = tid; si < p.n_subs; si += 256) {
		const FtPosSubterm& s = p.subs[si];
		const uint32_t lo = ft_seg_lo(s, range);
		if (si < kFtRangeSubs) {
			s_lo[si] = lo;
			s_hi[si] = ft_seg_hi(s, range);
			s_docptr[si] = s.doc;
			s_proc[si] = s.proc;
		}
		if (s.qp != 0) before += lo;   // NOT terms are not merged
	}
	before = wave_sum(before);
	if ((tid & 63) == 0) s_part[tid >> 6] = before;
	__syncthreads();
	if (tid == 0) p.bucket_off[range] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
	__syncthreads();   // s_part is reused below
	FT_STAMP(p, 1);
	const uint32_t nterms = p.simple ? 0u : p.nterms;
	const uint32_t ns = nterms ? (p.n_subs < kFtRangeSubs ? p.n_subs : kFtRangeSubs) : 0u;
	// ---- the staged segments cut into blocks of 256 postings (a block never spans two sub-terms); the first kFtStageBlocks blocks are
	// fetched NOW into registers — one posting per thread and block, every load independent of the others — and the terms below run out
	// of registers.  Which sub-term a block belongs to is a wave-uniform fact: the term loop tests it with scalar compares.  (History:
	// walking the sub-terms one after the other, each behind its own load round trips, took 23 us of this kernel's 40 for a 3 x 3 query;
	// a flat layout with a per-posting owner search spent 6 us in VALU compares — a wave64 operation costs four cycles — plus an LDS stage.)
	if (ns) {
		const uint32_t a = 2 * tid, b = 2 * tid + 1;
		const uint32_t na = a < ns ? (s_hi[a] - s_lo[a] + 255) / 256 : 0u, nb = b < ns ? (s_hi[b] - s_lo[b] + 255) / 256 : 0u;
		const uint32_t incl = wave_inclusive_scan(na + nb, int(tid & 63));
		if ((tid & 63) == 63) s_part[tid >> 6] = incl;
		__syncthreads();
		uint32_t excl = incl - (na + nb);
		for (uint32_t w = 0; w < (tid >> 6); ++w) excl += s_part[w];
		if (a < ns) s_blk0[a] = excl;
		if (b < ns) s_blk0[b] = excl + na;
		if (b + 1 == ns) {   // the thread that holds the last staged sub-term also writes the end marker
			s_blk0[ns] = excl + na + nb;
		} else if (a + 1 == ns) {
			s_blk0[ns] = excl + na;
		}
		for (uint32_t which = 0; which < 2; ++which) {   // block descriptors of this thread's two sub-terms
			const uint32_t si = which ? b : a, nblk = which ? nb : na, b0 = which ? excl + na : excl;
			if (si >= ns) continue;
			for (uint32_t k = 0; k < nblk && b0 + k < kFtStageBlocks; ++k) {
				const uint32_t first = s_lo[si] + 256 * k;
				s_binfo[b0 + k] = BlockInfo{s_docptr[si] + first, s_hi[si] - first < 256u ? s_hi[si] - first : 256u, 0u};
			}
		}
		__syncthreads();
	}
	FT_STAMP(p, 7);
	const uint32_t total_blocks = ns ? s_blk0[ns] : 0u;
	const uint32_t n_staged = total_blocks < kFtStageBlocks ? total_blocks : kFtStageBlocks;
	uint32_t dd[kFtStageBlocks];   // local document id of the thread's posting in block q, or 0xFFFFFFFF
	{
		uint32_t raw[kFtStageBlocks];
		bool have[kFtStageBlocks];
#pragma unroll
		for (uint32_t q = 0; q < kFtStageBlocks; ++q) {
			const uint4 info = *reinterpret_cast<const uint4*>(&s_binfo[q]);   // uniform address: one broadcast read, all 32 of them independent
			const uint32_t* first = reinterpret_cast<const uint32_t*>((uint64_t(info.y) << 32) | info.x);
			have[q] = q < n_staged && tid < info.z;
			raw[q] = have[q] ? first[tid] : 0u;
		}
#pragma unroll
		for (uint32_t q = 0; q < kFtStageBlocks; ++q) dd[q] = have[q] ? raw[q] - uint32_t(d_begin) : 0xFFFFFFFFu;
	}
	FT_STAMP(p, 6);
	// the removed flags of the thread's documents (four per word), wanted after the terms: requested now, in flight behind the term pass
	constexpr uint32_t kSteps = kFtRangeDocs / 4 / 256;   // 8 steps of four documents per thread
	uint32_t rm8[kSteps];
#pragma unroll
	for (uint32_t j = 0; j < kSteps; ++j) {
		const uint32_t l0 = (j * 256 + tid) * 4;
		rm8[j] = (p.prescore && p.removed && l0 < docs_here) ? *reinterpret_cast<const uint32_t*>(p.removed + d_begin + l0) : 0u;   // reads past the end stay inside the allocation
	}
	for (uint32_t t = 0; t < nterms; ++t) {
		const FtTermCfg& term = p.terms[t];
		const int op = term.op;
		const bool want_score = p.prescore && op != 3;
		if (op == 1 && !want_score) continue;   // an OR term only matters to the pre-score
		for (uint32_t w = tid; w < kWords; w += 256) s_term[w] = 0;
		const uint32_t epoch = (t % 255u) + 1u;   // byte tag of this term (the bytes start at 0: set with the scores above)
		if (t && t % 255u == 0) {   // the tags wrap: no stale one may survive
			for (uint32_t w = tid; w < kFtRangeDocs / 4; w += 256) reinterpret_cast<uint32_t*>(s_scored)[w] = 0;
		}
		__syncthreads();
		// the term's configuration in registers: `term` lives in global memory, and a load per posting sat on the critical path
		const bool all_pos_boost = term.all_pos_boost != 0, same_boost = term.same_boost != 0;
		const float boost0 = term.field_boost[0], opts_boost = term.opts_boost;
		// a phrase part (its rows come from ft_phrase.hip): every document counts (GetMergedDocsBitmask, phrasemerger.h:309-317) and scores
		// CalcProc16 without the 65535 / 4 cap of a term (GetMergedDocsScore, :326-333)
		const bool is_phrase = term.phrase != 0;
		const uint32_t phrase16 = term.phrase_proc16;
		const bool need_entries = (op == 2 && !all_pos_boost) || (want_score && !same_boost);
		auto visit = [&](const FtPosSubterm& s, float sproc, uint32_t i, uint32_t local) {
			const uint32_t bit = 1u << (local & 31);
			if (op == 3) {
				atomicAnd(&s_mask[local >> 5], ~bit);
				return;
			}
			bool rel = all_pos_boost;
			float mb = boost0;
			if (need_entries) {   // maxFieldsBoost (phrasemergerimpl.h:127-160) / relevance of the occurrence
				mb = 0.0f;
				rel = false;
				for (uint32_t e = s.ent_off[i], e1 = s.ent_off[i + 1]; e < e1; ++e) {
					const float fb = term.field_boost[s.ent_field[e]];
					mb = fmaxf(mb, fb);
					rel = rel || fb != 0.0f;
				}
				if (same_boost) mb = boost0;
				if (all_pos_boost) rel = true;
			}
			if (op == 2 && rel) atomicOr(&s_term[local >> 5], bit);
			if (want_score && mb > 0.0f) {
				// termMask: documents are unique inside a sub-term and earlier sub-terms are behind a barrier, so the first one wins
				if (s_scored[local] != epoch) {
					s_scored[local] = uint8_t(epoch);
					const float proc = sproc * mb * opts_boost;
					uint32_t p16 = uint32_t(int32_t(proc)) & 0xFFFFu;   // static_cast<uint16_t>(float) as x86 evaluates it
					p16 = p16 < 65535u / 4 ? p16 : 65535u / 4;
					if (is_phrase) p16 = phrase16;
					const uint32_t cur = s_score[local];
					p16 = p16 < 65535u - cur ? p16 : 65535u - cur;
					s_score[local] = uint16_t(cur + p16);
				}
			}
		};
		// sub-terms in SortSubterms order behind barriers ("the first one holding the document wins")
		const uint32_t sub_begin = term.sub_begin, sub_end = term.sub_end;
		for (uint32_t si = sub_begin; si < sub_end; ++si) {
			const FtPosSubterm& s = p.subs[si];
			uint32_t lo, hi, from_global;
			float sproc;
			if (si < ns) {
				lo = s_lo[si];
				hi = s_hi[si];
				sproc = s_proc[si];
				const uint32_t b0 = s_blk0[si], b1raw = s_blk0[si + 1];
				const uint32_t b1 = b1raw < n_staged ? b1raw : n_staged;   // staged blocks of this sub-term: [b0, b1)
				const bool fast = !(op == 3 || need_entries);
				const float proc = sproc * boost0 * opts_boost;
				uint32_t p16c = uint32_t(int32_t(proc)) & 0xFFFFu;   // static_cast<uint16_t>(float) as x86 evaluates it
				p16c = p16c < 65535u / 4 ? p16c : 65535u / 4;
				if (is_phrase) p16c = phrase16;
				const bool scoring = want_score && boost0 > 0.0f;
#pragma unroll
				for (uint32_t g = 0; g < kFtStageBlocks; g += 4) {
					if (g + 4 <= b0 || g >= b1) continue;   // uniform: none of the four blocks is this sub-term's
					bool ok[4];
					uint32_t loc[4], tag[4];
#pragma unroll
					for (uint32_t q = 0; q < 4; ++q) {
						ok[q] = g + q >= b0 && g + q < b1 && dd[g + q] != 0xFFFFFFFFu;
						loc[q] = ok[q] ? dd[g + q] : 0u;
					}
					if (!fast) {
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q) {
							if (ok[q]) visit(s, sproc, lo + 256 * (g + q - b0) + tid, loc[q]);
						}
						continue;
					}
					// the common case (no per-entry field test), four postings per thread: their LDS atomics and score updates are
					// independent chains that overlap
					if (op == 2) {   // all_pos_boost: every occurrence is relevant
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q) {
							if (ok[q]) atomicOr(&s_term[loc[q] >> 5], 1u << (loc[q] & 31));
						}
					}
					if (scoring) {
						// Reads without a condition (a lane without a posting reads document 0 and drops the result): under `if (ok)` each
						// of them became its own exec-masked block with its own lgkmcnt(0), i.e. eight LDS round trips in a row per
						// group instead of two.  The four documents of a thread are distinct, and so are those of different threads
						// (one sub-term), so every read may precede every write.
						uint32_t cur[4];
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q) tag[q] = s_scored[loc[q]];
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q) cur[q] = s_score[loc[q]];
#pragma unroll
						for (uint32_t q = 0; q < 4; ++q) {
							if (!ok[q] || tag[q] == epoch) continue;   // (an earlier sub-term of the term holds the document)
							const uint32_t add = p16c < 65535u - cur[q] ? p16c : 65535u - cur[q];
							s_scored[loc[q]] = uint8_t(epoch);
							s_score[loc[q]] = uint16_t(cur[q] + add);
						}
					}
				}
				from_global = lo + 256 * (b1 > b0 ? b1 - b0 : 0u);   // what did not fit the stage
				if (from_global > hi) from_global = hi;
			} else {
				lo = ft_seg_lo(s, range);
				hi = ft_seg_hi(s, range);
				sproc = s.proc;
				from_global = lo;
			}
			for (uint32_t base = from_global; base < hi; base += 4 * 256) {
				uint32_t idx[4], d4[4];
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					idx[q] = base + uint32_t(q) * 256 + tid;
					d4[q] = idx[q] < hi ? s.doc[idx[q]] : 0u;
				}
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					if (idx[q] < hi) visit(s, sproc, idx[q], uint32_t(d4[q] - d_begin));
				}
			}
			__syncthreads();   // the next sub-term of the term sees this one's documents
		}
		if (op == 2) {   // restrictingMask_ &= termMask (an AND term without postings empties the range)
			const uint32_t* syn_mask = term.syn_mask;   // termMask |= synMask of the part's multi-word synonyms (mergerimpl.h:347-361), ft_syn_masks
			for (uint32_t w = tid; w < kWords; w += 256) {
				const uint64_t gw = d_begin / 32 + w;
				s_mask[w] &= s_term[w] | ((syn_mask && gw < p.nwords) ? syn_mask[gw] : 0u);
			}
			__syncthreads();
		}
		FT_STAMP(p, 11 + (t < 4 ? t : 4));
	}
	FT_STAMP(p, 2);
	// ---- the range's mask words + their popcount (the device half of the 2-phase gate).  The global stores come last: a barrier behind
	// them would wait for their acknowledgement
	uint32_t c = 0;
	for (uint32_t w = tid; w < kWords; w += 256) {
		if (d_begin / 32 + w < p.nwords) c += __popc(s_mask[w]);
	}
	c = wave_sum(c);
	if ((tid & 63) == 0) s_part[tid >> 6] = c;
	__syncthreads();
	if (tid == 0) {
		const uint32_t tot = s_part[0] + s_part[1] + s_part[2] + s_part[3];
		if (tot) atomicAdd(&p.sync[kFtSyncPop], tot);
	}
	for (uint32_t w = tid; w < kWords; w += 256) {
		const uint64_t gw = d_begin / 32 + w;
		if (gw < p.nwords) p.mask[gw] = s_mask[w];
	}
	FT_STAMP(p, 3);
	if (p.prescore) ft_ranges_histogram(p, tid, range, d_begin, docs_here, rm8, s_mask, s_score, s_keys, s_rep);
}

// ---- the tail of ft_ranges when pre-scores are collected, as a function of its own.  (It changes the kernel's machine code — 87 VGPRs, occupancy
// 5 and no scratch as before — and was accepted on timing: profiles/ft_units_ab.json.)  Scores: masked-out / removed documents score 0 (mergerimpl.h:416-423);
// histogram of the rest through a small LDS hash table.
// Few distinct scores occur (a handful of proc values and their sums), so plain counters would take 64-way same-address atomics from
// every wavefront: each key gets kFtHistRep counters on different banks (the posting stage is free by now), lane l adds to counter l % kFtHistRep
__device__ __forceinline__ void ft_ranges_histogram(FtPlanK& p, uint32_t tid, uint32_t range, uint64_t d_begin, uint32_t docs_here, const uint32_t (&rm8)[kFtRangeDocs / 4 / 256],
													 const uint32_t* s_mask, uint16_t* s_score, uint32_t* s_keys, uint32_t* s_rep) {
	constexpr uint32_t kWords = kFtRangeDocs / 32, kSteps = kFtRangeDocs / 4 / 256;
	uint32_t* hist_copy = p.hist + size_t(range % kFtHistCopies) * kFtHistStride;
	for (uint32_t i = tid; i < 256 * kFtHistRep; i += 256) s_rep[i] = 0;
	__syncthreads();
	// masked scores first (eight 8-byte LDS reads, the global stores; the masked value goes back into the LDS copy), then the counting
	// loop — deliberately NOT unrolled: with the probe loop inlined 32 times this phase was 8400 instructions and, at three wavefronts
	// per SIMD, took 6 us on instruction issue alone
#pragma unroll
	for (uint32_t j = 0; j < kSteps; ++j) {
		const uint32_t l0 = (j * 256 + tid) * 4;
		const uint32_t mw = s_mask[(l0 >> 5) & (kWords - 1)];
		const uint2 four = *reinterpret_cast<const uint2*>(&s_score[l0]);
		const uint32_t raw[4] = {four.x & 0xFFFFu, four.x >> 16, four.y & 0xFFFFu, four.y >> 16};
		uint32_t sc[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const bool in = l0 + k < docs_here && ((mw >> ((l0 + k) & 31)) & 1u) && !((rm8[j] >> (8 * k)) & 0xFFu);
			sc[k] = in ? raw[k] : 0u;
		}
		const uint2 packed = make_uint2(sc[0] | (sc[1] << 16), sc[2] | (sc[3] << 16));
		*reinterpret_cast<uint2*>(&s_score[l0]) = packed;   // this thread's own four documents
		if (l0 < docs_here) *reinterpret_cast<uint2*>(p.score + d_begin + l0) = packed;   // the array is padded to whole mask words
	}
#pragma unroll 1
	for (uint32_t j = 0; j < kSteps; ++j) {
		const uint32_t l0 = (j * 256 + tid) * 4;
		const uint2 four = *reinterpret_cast<const uint2*>(&s_score[l0]);
		const uint32_t sc[4] = {four.x & 0xFFFFu, four.x >> 16, four.y & 0xFFFFu, four.y >> 16};
		uint32_t h[4], cur[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			h[k] = (sc[k] * 2654435761u) >> 24;
			cur[k] = sc[k] ? s_keys[h[k]] : 0u;
		}
		uint32_t slow = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			if (!sc[k]) continue;
			if (cur[k] == sc[k]) {   // the key is there already (after the first few documents of the range it always is)
				atomicAdd(&s_rep[h[k] * kFtHistRep + (tid & (kFtHistRep - 1))], 1u);
			} else {
				slow |= 1u << k;
			}
		}
		while (slow) {   // a new key, or a slot taken by another one: probe
			const int k = __ffs(int(slow)) - 1;
			slow &= slow - 1;
			const uint32_t v = k == 0 ? sc[0] : k == 1 ? sc[1] : k == 2 ? sc[2] : sc[3];
			uint32_t hh = k == 0 ? h[0] : k == 1 ? h[1] : k == 2 ? h[2] : h[3];
			int probes = 0;
			for (; probes < 256; ++probes, hh = (hh + 1) & 255u) {
				uint32_t c = s_keys[hh];
				if (c != v) {
					if (c != 0u) continue;
					c = atomicCAS(&s_keys[hh], 0u, v);
					if (c != 0u && c != v) continue;
				}
				atomicAdd(&s_rep[hh * kFtHistRep + (tid & (kFtHistRep - 1))], 1u);
				break;
			}
			if (probes == 256) {   // more than 256 distinct scores in one range (a register-side count of the common values was slower: 15 us)
				atomicAdd(&hist_copy[v], 1u);
				atomicAdd(&hist_copy[65536 + (v >> 6)], 1u);
			}
		}
	}
	__syncthreads();
	FT_STAMP(p, 4);
	const uint32_t key = s_keys[tid];
	uint32_t total = 0;
	if (key) {
#pragma unroll
		for (uint32_t r = 0; r < kFtHistRep; ++r) total += s_rep[tid * kFtHistRep + r];
		atomicAdd(&hist_copy[key], total);
	}
	// the chunk totals: the keys of one chunk are combined inside the workgroup first — every workgroup holds the same few scores, and
	// same-address device atomics from 600 workgroups on two or three chunk counters took 24 us when each key added on its own
	__syncthreads();   // the replicated counters have been read: their space becomes the chunk table
	uint32_t* s_ck = s_rep;          // [256] chunk + 1 (0 = free)
	uint32_t* s_cc = s_rep + 256;    // [256] documents
	s_ck[tid] = 0;
	s_cc[tid] = 0;
	__syncthreads();
	if (key) {
		const uint32_t ck = (key >> 6) + 1;
		uint32_t h = (ck * 2654435761u) >> 24;
		for (int probes = 0; probes < 256; ++probes, h = (h + 1) & 255u) {   // at most 256 keys: a free slot always turns up
			uint32_t cur = s_ck[h];
			if (cur != ck) {
				if (cur != 0u) continue;
				cur = atomicCAS(&s_ck[h], 0u, ck);
				if (cur != 0u && cur != ck) continue;
			}
			atomicAdd(&s_cc[h], total);
			break;
		}
	}
	__syncthreads();
	if (s_ck[tid]) atomicAdd(&hist_copy[65536 + s_ck[tid] - 1], s_cc[tid]);
	FT_STAMP(p, 5);
}


// mergerimpl.h:448-462: kFtApplyWords mask words per thread (the ordered prefix chain is as long as the grid: fewer, fatter workgroups);
// ties at minScore are kept in document order up to minScoreDocs
__global__ __launch_bounds__(256) void ft_preselect_apply(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	if (!ft_preselect_on(p)) return;
	const uint32_t ticket = grab_ticket(p.sync + kFtSyncPreTicket);
	// a document-range shard walks its own mask words (tickets = document order inside the shard); nwords_end bounds the last workgroup
	const uint64_t word_begin = uint64_t(p.range_begin) * (kFtRangeDocs / 32);
	const uint64_t nwords_end = p.range_count ? min(p.nwords, word_begin + uint64_t(p.range_count) * (kFtRangeDocs / 32)) : p.nwords;
	const uint64_t w0 = word_begin + (uint64_t(ticket) * 256 + threadIdx.x) * kFtApplyWords;
	uint32_t min_score, min_docs;
	ft_pick_threshold(p, &min_score, &min_docs);
	if (p.shard_hist) {   // the ties the shards in front of this one keep at the threshold score (document order = shard order): taken off the quota
		uint32_t used = 0;
		for (uint32_t sh = 0; sh < p.shard_index; ++sh) used += p.shard_hist[size_t(p.shard_pos[sh]) * kFtFoldWords + min_score];
		min_docs = min_docs > used ? min_docs - used : 0u;
	}
	uint32_t bits[kFtApplyWords], gt[kFtApplyWords], tie[kFtApplyWords];
	uint32_t ties = 0;
#pragma unroll
	for (int j = 0; j < kFtApplyWords; ++j) {
		bits[j] = gt[j] = tie[j] = 0;
		const uint64_t w = w0 + j;
		if (w >= nwords_end) continue;
		bits[j] = p.mask[w];
		// the 32 scores of the word as four 16-byte loads (the score array is padded to a whole word); only masked-in documents count
		const uint4* s4 = reinterpret_cast<const uint4*>(p.score + w * 32);
		uint4 v[4];
#pragma unroll
		for (int q = 0; q < 4; ++q) v[q] = s4[q];
		const uint32_t half[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
								   v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
#pragma unroll
		for (int q = 0; q < 16; ++q) {
			const uint32_t lo = half[q] & 0xFFFFu, hi = half[q] >> 16;
			gt[j] |= (uint32_t(lo > min_score) << (2 * q)) | (uint32_t(hi > min_score) << (2 * q + 1));
			tie[j] |= (uint32_t(lo == min_score) << (2 * q)) | (uint32_t(hi == min_score) << (2 * q + 1));
		}
		gt[j] &= bits[j];
		tie[j] &= bits[j];
		ties += __popc(tie[j]);
	}
	uint32_t grand;
	const uint32_t excl = ordered_prefix(ties, ticket, p.lookback_pre, p.sync + kFtSyncError, &grand);
	uint32_t allowed = min_docs > excl ? min_docs - excl : 0;
#pragma unroll
	for (int j = 0; j < kFtApplyWords; ++j) {
		if (w0 + j >= nwords_end) continue;
		uint32_t keep = gt[j], tj = tie[j];
		while (tj && allowed) {
			const uint32_t low = tj & (0u - tj);
			keep |= low;
			tj ^= low;
			--allowed;
		}
		if (keep != bits[j]) p.mask[w0 + j] = keep;
	}
}

void launch_ft_syn_masks(const FtPlan* plans, uint32_t ranges, hipStream_t st) { hipLaunchKernelGGL(ft_syn_masks, dim3(ranges, 1), dim3(256), 0, st, plans); }
void launch_ft_ranges(const FtPlan* plans, uint32_t ranges, uint32_t nq, hipStream_t st) { hipLaunchKernelGGL(ft_ranges, dim3(ranges, nq), dim3(256), 0, st, plans); }
void launch_ft_preselect_apply(const FtPlan* plans, uint32_t blocks, uint32_t nq, hipStream_t st) {
	hipLaunchKernelGGL(ft_preselect_apply, dim3(blocks, nq), dim3(256), 0, st, plans);
}

}  // namespace rxgpu
