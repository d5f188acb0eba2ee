// Admission of the dense ft_fast train (ft_merge.hip tells the whole story): every eligible posting ranked and bucketed by document range
// (ft_rank_all), the documents first met per (sub-term row, range) counted (ft_adders), and that table turned into the slot bases
// (ft_slot_bases, when ft_finish does not sum them itself).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rxgpu_internal.h"
#include "knn_kernels.hip.h"
#include "ft_rank.hip.h"
#include "ft_scan.hip.h"
#include "ft_replay.hip.h"

namespace rxgpu {

// ---------------------------------------------------------------------------------------------- mergeTerm / mergeSimple
// calcTermRank of every eligible posting of the query (restrictingMask_, DocRemoved); the postings that rank non-zero leave as 16-byte
// records in the bucket of their document range.
// The gathers of one posting form a dependent chain (doc -> mask word -> removed flag | entries -> words in field).  The cheap half
// (document, mask bit, removed flag) is streamed for kFtRankTiles x 1024 postings per workgroup, four postings per thread and tile with
// every stage issued for all of them before anything is consumed; the survivors are COMPACTED in LDS and the expensive half
// (calcTermRank, five dependent gathers) then runs once over the compact list, one posting per lane.  After a preselect ~1 % of the
// postings survive: evaluated in place, nearly every wavefront held one and paid the chain up to four times in a row (once per
// item slot) — 38 us for 3.9 M postings; a first attempt with fatter threads made that 64 us.
__global__ __launch_bounds__(256) void ft_rank_all(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	if (blockIdx.x * kFtRankTiles >= p.merge_blocks) return;   // the grid is the widest query's
	__shared__ uint32_t s_cnt;
	__shared__ uint16_t s_item[kFtRankTiles * kFtBlockPostings];   // tile << 10 | thread << 2 | slot
	__shared__ uint32_t s_doc[kFtRankTiles * kFtBlockPostings];
	__shared__ uint32_t s_sub[kFtRankTiles], s_base[kFtRankTiles];
	// the tiles' sub-term and term descriptors, copied once: calcTermRank reads a dozen of their fields per posting, and from global
	// memory every first touch was one more round trip in front of the entry gathers
	__shared__ FtPosSubterm s_subd[kFtRankTiles];
	__shared__ FtTermCfg s_termd[kFtRankTiles];
	static_assert(sizeof(FtPosSubterm) % 4 == 0 && sizeof(FtTermCfg) % 4 == 0, "descriptors are copied word by word");
	FT_STAMP(p, 16);
	if (threadIdx.x == 0) s_cnt = 0;
	{
		const uint32_t g = threadIdx.x >> 7, l = threadIdx.x & 127;   // 128 threads per tile: binary search by all (broadcast loads), copy by words
		static_assert(kFtRankTiles == 2, "two tiles, 128 threads each");
		const uint32_t tile = blockIdx.x * kFtRankTiles + g;
		if (tile < p.merge_blocks) {
			const FtGridEntry ge = grid_entry(p.merge_grid, p.n_merge_entries, tile);
			if (l == 0) {
				s_sub[g] = ge.sub;
				s_base[g] = ge.block_base;
			}
			const uint32_t* src_s = reinterpret_cast<const uint32_t*>(p.subs + ge.sub);
			if (l < sizeof(FtPosSubterm) / 4) reinterpret_cast<uint32_t*>(&s_subd[g])[l] = src_s[l];
			const uint32_t term = p.subs[ge.sub].term;
			const uint32_t* src_t = reinterpret_cast<const uint32_t*>(p.terms + term);
			if (l < sizeof(FtTermCfg) / 4) reinterpret_cast<uint32_t*>(&s_termd[g])[l] = src_t[l];
		}
	}
	__syncthreads();
	uint32_t docs[kFtRankTiles][kFtPassItems];
	bool live[kFtRankTiles][kFtPassItems];
#pragma unroll
	for (int g = 0; g < kFtRankTiles; ++g) {
		const uint32_t tile = blockIdx.x * kFtRankTiles + g;
#pragma unroll
		for (int k = 0; k < kFtPassItems; ++k) {
			live[g][k] = false;
			docs[g][k] = 0;
		}
		if (tile >= p.merge_blocks) continue;
		const FtPosSubterm& s = s_subd[g];
		const uint64_t i0 = uint64_t(tile - s_base[g]) * kFtBlockPostings + uint64_t(threadIdx.x) * kFtPassItems;
		if (i0 < s.n) load_docs(s, i0, docs[g], live[g]);
	}
	{
		uint32_t mw[kFtRankTiles][kFtPassItems];
#pragma unroll
		for (int g = 0; g < kFtRankTiles; ++g) {
#pragma unroll
			for (int k = 0; k < kFtPassItems; ++k) mw[g][k] = live[g][k] ? p.mask[docs[g][k] >> 5] : 0u;
		}
#pragma unroll
		for (int g = 0; g < kFtRankTiles; ++g) {
#pragma unroll
			for (int k = 0; k < kFtPassItems; ++k) live[g][k] = live[g][k] && ((mw[g][k] >> (docs[g][k] & 31)) & 1u);   // restrictingMask_
		}
	}
	if (p.removed && p.check_removed && !ft_preselect_on(p)) {   // needToCheckRemoved_ is false once the preselect has run (mergerimpl.h:463)
		uint8_t rm[kFtRankTiles][kFtPassItems];
#pragma unroll
		for (int g = 0; g < kFtRankTiles; ++g) {
#pragma unroll
			for (int k = 0; k < kFtPassItems; ++k) rm[g][k] = live[g][k] ? p.removed[docs[g][k]] : uint8_t(0);
		}
#pragma unroll
		for (int g = 0; g < kFtRankTiles; ++g) {
#pragma unroll
			for (int k = 0; k < kFtPassItems; ++k) live[g][k] = live[g][k] && !rm[g][k];
		}
	}
#pragma unroll
	for (int g = 0; g < kFtRankTiles; ++g) {
#pragma unroll
		for (int k = 0; k < kFtPassItems; ++k) {
			if (!live[g][k]) continue;
			const uint32_t at = atomicAdd(&s_cnt, 1u);
			s_item[at] = uint16_t((uint32_t(g) << 10) | (threadIdx.x << 2) | uint32_t(k));
			s_doc[at] = docs[g][k];
		}
	}
	__syncthreads();
	FT_STAMP(p, 17);
	const uint32_t cnt = s_cnt;
	const int lane = threadIdx.x & 63;
	// Two postings per thread and step when more than one step is due (dense merges rank every posting of the tile): the two
	// calcTermRank gather chains are independent and overlap.  Uniform trip count: the wavefront votes below.
	const uint32_t per_step = cnt > 256 ? 512u : 256u;
	for (uint32_t e0 = 0; e0 < cnt; e0 += per_step) {
		bool want[2] = {false, false};
		uint32_t d[2] = {0, 0}, row[2] = {0, 0}, idx[2] = {0, 0};
		float rank[2] = {0.0f, 0.0f};
		uint8_t field[2] = {0, 0};
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const uint32_t e = e0 + uint32_t(u) * 256 + threadIdx.x;
			if ((u == 0 || per_step == 512) && e < cnt) {
				const uint32_t item = s_item[e], g = item >> 10, local = item & 1023u;
				const uint32_t tile = blockIdx.x * kFtRankTiles + g;
				const FtPosSubterm& s = s_subd[g];
				const FtTermCfg& t = s_termd[g];
				const uint64_t i = uint64_t(tile - s_base[g]) * kFtBlockPostings + local;
				d[u] = s_doc[e];
				if (s.suppressed) {   // mergerimpl.h:144-151: no rank; the record only counts the term for a document that is merged already
					rank[u] = __uint_as_float(kFtSuppressedRank);
					field[u] = 0;
				} else if (s.pre_rank) {   // a phrase row: mergePhrase takes the PhraseMerger's rank and field as they are (mergerimpl.h:46-62)
					rank[u] = s.pre_rank[i];
					field[u] = s.pre_field[i];
				} else {
					rank[u] = ft_term_rank(t, s, s.ent_off[i], s.ent_off[i + 1], d[u], &field[u]);
				}
				want[u] = rank[u] != 0.0f;
				row[u] = s.row;
				idx[u] = uint32_t(i);
			}
		}
		// one device atomic per (wavefront, document range): neighbouring postings share a range, whole-corpus merges would otherwise
		// hammer a few hundred counters with millions of same-address atomics
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const uint32_t rg = d[u] >> kFtRangeShift;
			unsigned long long pending = __ballot(want[u]);
			while (pending) {
				const int leader = __ffsll((long long)pending) - 1;
				const uint32_t lrg = uint32_t(__shfl(int(rg), leader, 64));
				const bool mine = want[u] && rg == lrg;
				const unsigned long long same = __ballot(mine);
				uint32_t base = 0;
				if (lane == leader) base = atomicAdd(&p.bucket_cnt[lrg], uint32_t(__popcll(same)));
				base = uint32_t(__shfl(int(base), leader, 64));
				if (mine) {
					const uint32_t pos = base + uint32_t(__popcll(same & ((1ull << lane) - 1ull)));
					p.b_rec[uint64_t(p.bucket_off[lrg]) + pos] = make_uint4(d[u], idx[u], __float_as_uint(rank[u]), row[u] | (uint32_t(field[u]) << 16));
					want[u] = false;
				}
				pending &= ~same;
			}
		}
	}
	FT_STAMP(p, 18);
}

// addDoc order (merger.h:161-180), document side.  One workgroup per range: the row (sub-term) of every document's first surviving
// posting, counted per (row, range); the LAST workgroup to finish replaces the table by its exclusive prefix in row-major order — the merge
// slot of the first document of every (row, range) — and publishes the number of merged documents.  Also hands the next kernels / the next
// merge their zeroed tables (entry rows, histogram, look-back words).
constexpr uint32_t kFtAdderRowsLds = 1024;
__global__ __launch_bounds__(256) void ft_adders(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	__shared__ uint32_t s_tab[kFtRangeDocs / 2];   // first row of every document of the range, 16 bits each
	__shared__ uint32_t s_rowcnt[kFtAdderRowsLds];
	const uint32_t tid = threadIdx.x, range = blockIdx.x + p.range_begin;
	FT_STAMP(p, 24);
	if (p.prescore) {   // ft_preselect_apply was the last reader of the histograms and of the look-back words
		const uint64_t gtid = uint64_t(blockIdx.x) * blockDim.x + tid, gsize = uint64_t(gridDim.x) * blockDim.x;
		fill_words(p.hist, uint64_t(kFtHistCopies) * kFtHistStride, 0u, gtid, gsize);
		fill_words(reinterpret_cast<uint32_t*>(p.lookback_pre), ft_apply_blocks(p.nwords) * 2, 0u, gtid, gsize);
	}
	const uint32_t n = p.bucket_cnt[range];
	const bool lds_rows = p.n_rows <= kFtAdderRowsLds;
	for (uint32_t w = tid; w < kFtRangeDocs / 2; w += 256) s_tab[w] = 0xFFFFFFFFu;
	for (uint32_t r = tid; r < p.n_rows; r += 256) {
		if (lds_rows) {
			s_rowcnt[r] = 0;
		} else {
			p.adders[uint64_t(r) * p.n_ranges + range] = 0;   // this workgroup owns the column
		}
	}
	__syncthreads();
	FT_STAMP(p, 25);
	const uint4* rec = p.b_rec + p.bucket_off[range];
	// (the shared pass tests "first row" before "suppressed", where this kernel had it the other way round: other machine code, same result;
	// timed in profiles/ft_units_ab.json)
	ft_first_postings(rec, n, s_tab, tid, [&] { FT_STAMP(p, 26); }, [&](uint32_t, const uint4&, uint32_t row, uint32_t) {
		if (lds_rows) {
			atomicAdd(&s_rowcnt[row], 1u);
		} else {
			atomicAdd(&p.adders[uint64_t(row) * p.n_ranges + range], 1u);
		}
	});
	__syncthreads();
	if (lds_rows) {
		for (uint32_t r = tid; r < p.n_rows; r += 256) p.adders[uint64_t(r) * p.n_ranges + range] = s_rowcnt[r];
	}
	FT_STAMP(p, 27);
}

// The table of ft_adders -> its exclusive prefix in row-major order = the merge slot of the first document of every (row, range), and the
// number of merged documents (ft_own_bases, ft_merge_plan.h: small tables are summed by ft_finish instead).  One workgroup, behind a
// kernel boundary: an in-kernel hand-over (every workgroup releasing at agent scope before an arrival counter) cost 29 us — each release
// writes back the dirty lines of its XCD's L2.
// Tiles of 2048 entries: eight consecutive loads per thread in flight, one workgroup scan, eight stores.
__global__ __launch_bounds__(256) void ft_slot_bases(const FtPlan* plans) {
	FtPlanK& p = FT_PLAN_OF_QUERY(plans);
	if (!p.sparse && ft_own_bases(p)) return;   // this query's ft_finish sums the small table itself (the sparse train always comes here)
	__shared__ uint32_t s_part[4];
	const uint32_t tid = threadIdx.x;
	const uint64_t total = uint64_t(p.n_rows) * p.n_ranges;
	uint32_t carry = 0;
	for (uint64_t base = 0; base < total; base += 256 * 8) {
		const uint64_t j0 = base + uint64_t(tid) * 8;
		uint32_t v[8];
#pragma unroll
		for (int k = 0; k < 8; ++k) v[k] = j0 + k < total ? p.adders[j0 + k] : 0u;
		uint32_t local = 0;
#pragma unroll
		for (int k = 0; k < 8; ++k) local += v[k];
		const uint32_t incl = wave_inclusive_scan(local, int(tid & 63));
		if ((tid & 63) == 63) s_part[tid >> 6] = incl;
		__syncthreads();
		uint32_t running = carry + incl - local;
		for (uint32_t w = 0; w < (tid >> 6); ++w) running += s_part[w];
		carry += s_part[0] + s_part[1] + s_part[2] + s_part[3];
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			if (j0 + k < total) p.adders[j0 + k] = running;
			running += v[k];
		}
		__syncthreads();   // s_part is rewritten by the next tile
	}
	if (tid == 0) p.sync[kFtSyncNumDocs] = carry < p.max_merged ? carry : p.max_merged;
}

void launch_ft_rank_all(const FtPlan* plans, uint32_t blocks, uint32_t nq, hipStream_t st) { hipLaunchKernelGGL(ft_rank_all, dim3(blocks, nq), dim3(256), 0, st, plans); }
void launch_ft_adders(const FtPlan* plans, uint32_t ranges, uint32_t nq, hipStream_t st) { hipLaunchKernelGGL(ft_adders, dim3(ranges, nq), dim3(256), 0, st, plans); }
void launch_ft_slot_bases(const FtPlan* plans, uint32_t nq, hipStream_t st) { hipLaunchKernelGGL(ft_slot_bases, dim3(1, nq), dim3(256), 0, st, plans); }

}  // namespace rxgpu
