// Top-k merge kernels (gfx950): what the scans, the re-score and the shards leave -> the sorted top-kk of a query.  One insertion merge
// (merge_by_insertion, the definition of the result, NaN distances included) and the selections that answer without serial insertions
// wherever they can (merge_lists over sorted lists, merge_select over unsorted candidates).
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

constexpr int kMergeThreads = 512;
constexpr int kMergeWaves = kMergeThreads / kWave;
constexpr int kMergeAhead = 8;                       // candidate chunks whose loads a merge wavefront keeps in flight

// ---- the cross-wave steps of the insertion merge, one set per list type: a wavefront's sorted list into LDS (merge_list_store), a stored list
// offered to wavefront 0's (merge_list_offer), the result out to HBM (merge_list_write).  s_d / s_i hold kMergeListCap words per wavefront,
// `at` is the first word of the list in question.  (The scans' epilogue, block_merge_and_store in knn_scan_common.hip.h, spells the same
// steps out once more: sharing them there changed the scan kernels' instruction streams.)
template <typename TK>
constexpr int kMergeListCap = kMaxFusedK;
template <>
constexpr int kMergeListCap<WaveTopK2> = kMaxFusedK2;

// one entry per lane
__device__ __forceinline__ void merge_list_store(const WaveTopK& top, float* s_d, uint32_t* s_i, int at, int lane) {
	s_d[at + lane] = top.bd;
	s_i[at + lane] = top.bi;
}
// Lists are sorted and invalid entries sit only at their end: a list is walked from its head and left at the first entry that is not admitted.
// Here it is read into the lanes once and offered from there.
__device__ __forceinline__ void merge_list_offer(WaveTopK& top, const float* s_d, const uint32_t* s_i, int at, int lane) {
	const float cd = s_d[at + lane];
	const uint32_t ci = s_i[at + lane];
	uint64_t pm = __ballot(ci != kInvalidRow && lane < int(top.kk));
	while (pm) {
		const int src = __builtin_ctzll(pm);
		pm &= pm - 1;
		const float d = __shfl(cd, src);
		const uint32_t i = __shfl(ci, src);
		if (!top.admits(d, i)) break;
		top.insert(d, i, lane);
	}
}
__device__ __forceinline__ void merge_list_write(const WaveTopK& top, float* dist, uint32_t* row, size_t o, int lane) {
	if (lane < int(top.kk)) {
		dist[o + lane] = top.bd;
		row[o + lane] = top.bi;
	}
}
// two entries per lane (64 < kk <= 128): a stored list is walked in LDS
__device__ __forceinline__ void merge_list_store(const WaveTopK2& top, float* s_d, uint32_t* s_i, int at, int lane) {
	s_d[at + lane] = top.d0;
	s_i[at + lane] = top.i0;
	s_d[at + 64 + lane] = top.d1;
	s_i[at + 64 + lane] = top.i1;
}
__device__ __forceinline__ void merge_list_offer(WaveTopK2& top, const float* s_d, const uint32_t* s_i, int at, int lane) {
	for (uint32_t e = 0; e < top.kk; ++e) {
		const float d = s_d[at + e];
		const uint32_t i = s_i[at + e];
		if (i == kInvalidRow || !top.admits(d, i)) break;
		top.insert(d, i, lane);
	}
}
__device__ __forceinline__ void merge_list_write(const WaveTopK2& top, float* dist, uint32_t* row, size_t o, int lane) {
	if (lane < int(top.kk)) {
		dist[o + lane] = top.d0;
		row[o + lane] = top.i0;
	}
	if (64 + lane < int(top.kk)) {
		dist[o + 64 + lane] = top.d1;
		row[o + 64 + lane] = top.i1;
	}
}

// The insertion merge: fold `total` candidate (dist,row) pairs at part_*[base ..] (invalid rows skipped) into the sorted top-kk of query
// blockIdx.x, by all kMergeThreads threads.  Every wavefront folds its share into a list of its own, then wavefront 0 folds those lists in
// wavefront order.  s_d / s_i: [kMergeWaves][kMergeListCap<TK>] words of LDS each.
template <typename TK>
__device__ __forceinline__ void merge_by_insertion(const float* part_dist, const uint32_t* part_row, size_t base, uint32_t total, uint32_t kk, float* out_dist,
												   uint32_t* out_row, uint32_t* out_count, float* s_d, uint32_t* s_i) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	TK top;
	top.init(kk);
	// kMergeAhead chunks of 64 candidates per trip, all their loads issued together: one chunk per trip left every trip behind its own
	// memory round trip (~2 us each: 0.27 ms for the 512 x 101 partial entries of a k = 100 search, against 0.03 ms of list work)
	for (uint32_t c0 = wave * kWave; c0 < total; c0 += kMergeThreads * kMergeAhead) {
		float cd[kMergeAhead];
		uint32_t ci[kMergeAhead];
#pragma unroll
		for (int u = 0; u < kMergeAhead; ++u) {
			const uint32_t c = c0 + uint32_t(u) * kMergeThreads + lane;
			cd[u] = __builtin_inff();
			ci[u] = kInvalidRow;
			if (c < total) {
				cd[u] = part_dist[base + c];
				ci[u] = part_row[base + c];
			}
		}
#pragma unroll
		for (int u = 0; u < kMergeAhead; ++u) {
			uint64_t pm = __ballot(ci[u] != kInvalidRow && top.admits(cd[u], ci[u]));
			while (pm) {
				const int src = __builtin_ctzll(pm);
				pm &= pm - 1;
				const float d = __shfl(cd[u], src);
				const uint32_t i = __shfl(ci[u], src);
				if (top.admits(d, i)) top.insert(d, i, lane);
			}
		}
	}
	constexpr int kCap = kMergeListCap<TK>;
	merge_list_store(top, s_d, s_i, wave * kCap, lane);
	__syncthreads();
	if (wave != 0) return;
	for (int w = 1; w < kMergeWaves; ++w) merge_list_offer(top, s_d, s_i, w * kCap, lane);
	merge_list_write(top, out_dist, out_row, size_t(blockIdx.x) * kk, lane);
	if (lane == 0 && out_count) out_count[blockIdx.x] = top.filled;
}

// One workgroup per query: merge_by_insertion over the query's `total` pairs, in any order (the batched path: its re-scored candidates, and
// behind the gate the exact scan's lists).  kk <= kMaxFusedK.
__global__ __launch_bounds__(kMergeThreads) void knn_merge(const float* part_dist, const uint32_t* part_row, uint32_t total,
															uint32_t kk, float* out_dist, uint32_t* out_row, uint32_t* out_count,
															const uint32_t* gate_cnt, uint32_t gate_cap) {
	__shared__ float s_d[kMergeWaves * kMaxFusedK];
	__shared__ uint32_t s_i[kMergeWaves * kMaxFusedK];
	if (gate_cnt && gate_cnt[blockIdx.x] <= gate_cap) return;
	merge_by_insertion<WaveTopK>(part_dist, part_row, size_t(blockIdx.x) * total, total, kk, out_dist, out_row, out_count, s_d, s_i);
}

// ---- merge of SORTED partial lists (what the scans leave: gridDim.x lists of kk entries per query), without serial insertions.
// Folding ~500 lists through a wavefront-wide sorted list costs an insertion (a chain of cross-lane operations, ~0.4 us) for every
// candidate that beats the running kk-th — ~650 of them at k = 100: 0.25 ms behind a 1.5 ms scan.  The lists are sorted, so:
//   1. the kk-th smallest list HEAD bounds the kk-th best overall (the heads are kk real candidates at or below it);
//   2. only entries at or below that bound can be in the result: every list is walked from its head while it stays below — for rows
//      spread evenly over the partitions that is ~1.1 kk entries in total;
//   3. those candidates are sorted in LDS (bitonic, (distance, row) keys) and the first kk written.
// Exact for any data; when the bound lets more than kMergeCandMax entries through (masses of equal distances) or there are fewer lists
// than kk, the insertion merge runs instead (same kernel, workgroup-uniform branch).
constexpr uint32_t kMergeHeadsMax = 4096, kMergeCandMax = 2048;
__device__ __forceinline__ unsigned long long merge_pair_key(float d, uint32_t row) {
	uint32_t b = __float_as_uint(d);
	if (b == 0x80000000u) b = 0;   // -0.0 == +0.0 for pair_lt: the row decides
	b ^= (b >> 31) ? 0xFFFFFFFFu : 0x80000000u;
	return (static_cast<unsigned long long>(b) << 32) | row;
}
// ascending bitonic sort of n = 2^m (key, payload) pairs in LDS by all kMergeThreads threads
__device__ __forceinline__ void merge_bitonic(unsigned long long* key, float* val, uint32_t n) {
	for (uint32_t k = 2; k <= n; k <<= 1) {
		for (uint32_t j = k >> 1; j > 0; j >>= 1) {
			for (uint32_t t = threadIdx.x; t < n / 2; t += kMergeThreads) {
				const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
				const unsigned long long x = key[i], y = key[l];
				if ((x > y) == ((i & k) == 0)) {
					key[i] = y;
					key[l] = x;
					const float vx = val[i];
					val[i] = val[l];
					val[l] = vx;
				}
			}
			__syncthreads();
		}
	}
}
// The bound of both selections below is the kk-th smallest of a few hundred group heads, and sorting them all in LDS to read one entry costs 45
// barrier stages at 512 heads.  Instead every wavefront sorts its 64 heads in registers (no LDS, no barrier) and leaves the first min(kk, 64):
// the kk-th smallest overall is among those.  For kk = 11 and 512 heads that is 88 keys, and the one of rank kk - 1 is found by counting.
constexpr uint32_t kMergeRankMax = 256;   // up to this many keys are ranked by counting over LDS (n reads per thread, one barrier); more: bitonic
// ascending sort of one key per lane across the wavefront: lane i ends with the i-th smallest
__device__ __forceinline__ unsigned long long merge_wave_sort(unsigned long long k, int lane) {
	for (int size = 2; size <= kWave; size <<= 1) {
		for (int j = size >> 1; j > 0; j >>= 1) {
			const unsigned long long o = __shfl_xor(k, j);
			const bool take_min = ((lane & size) == 0) == ((lane & j) == 0);
			k = (k < o) == take_min ? k : o;
		}
	}
	return k;
}
// rank of entry i among key[0 .. n): the number of smaller keys, equal keys (pads; the same row handed in twice) in index order
__device__ __forceinline__ uint32_t merge_rank(const unsigned long long* key, uint32_t n, uint32_t i) {
	const unsigned long long mine = key[i];
	uint32_t rank = 0;
	for (uint32_t j = 0; j < n; ++j) {
		const unsigned long long k = key[j];
		rank += (k < mine || (k == mine && j < i)) ? 1u : 0u;
	}
	return rank;
}
// *bound = the key of rank kk - 1 among key[0 .. m) (m <= kMergeRankMax, kk <= m; pads are ~0, so ~0 when fewer than kk keys are real).
// `bound` is a word of LDS outside key[0 .. m); ends with a barrier.
__device__ __forceinline__ void merge_kth_key(const unsigned long long* key, uint32_t m, uint32_t kk, unsigned long long* bound) {
	__syncthreads();
	if (threadIdx.x < m && merge_rank(key, m, threadIdx.x) == kk - 1) *bound = key[threadIdx.x];
	__syncthreads();
}
// The n <= kMergeCandMax collected (key, distance) pairs in LDS, unique keys -> the first kk in key order, padded with +inf / kInvalidRow, and
// the count.  Every thread has passed a barrier since the pairs were written.
__device__ __forceinline__ void merge_write_sorted(unsigned long long* s_key, float* s_val, uint32_t n, uint32_t kk, float* out_dist, uint32_t* out_row,
												   uint32_t* out_count) {
	const uint32_t tid = threadIdx.x, cnt = n < kk ? n : kk;
	const size_t o = size_t(blockIdx.x) * kk;
	if (tid == 0 && out_count) out_count[blockIdx.x] = cnt;
	if (n <= kMergeRankMax) {   // an entry's place is the number of smaller keys
		if (tid < n) {
			const uint32_t rank = merge_rank(s_key, n, tid);
			if (rank < kk) {
				out_dist[o + rank] = s_val[tid];
				out_row[o + rank] = uint32_t(s_key[tid]);
			}
		}
		for (uint32_t q = cnt + tid; q < kk; q += kMergeThreads) {
			out_dist[o + q] = __builtin_inff();
			out_row[o + q] = kInvalidRow;
		}
		return;
	}
	uint32_t n2 = 64;
	while (n2 < n) n2 <<= 1;
	for (uint32_t q = n + tid; q < n2; q += kMergeThreads) {
		s_key[q] = ~0ull;
		s_val[q] = 0.f;
	}
	__syncthreads();
	merge_bitonic(s_key, s_val, n2);
	for (uint32_t q = tid; q < kk; q += kMergeThreads) {
		out_dist[o + q] = q < cnt ? s_val[q] : __builtin_inff();
		out_row[o + q] = q < cnt ? uint32_t(s_key[q]) : kInvalidRow;
	}
}

constexpr uint32_t kMergeWalkAhead = 4;   // entries of a list whose loads the walk issues together, ahead of the comparison
// the merge of query blockIdx.x; s_key / s_val: [kMergeHeadsMax], s_n: one word of LDS.  Returns true when the selection answered, false when
// the insertion merge did (workgroup-uniform).
template <typename TK>
__device__ __forceinline__ bool merge_lists(const float* part_dist, const uint32_t* part_row, uint32_t nlists, uint32_t kk, float* out_dist, uint32_t* out_row,
											uint32_t* out_count, unsigned long long* s_key, float* s_val, uint32_t* s_np) {
	uint32_t& s_n = *s_np;
	const uint32_t tid = threadIdx.x, total = nlists * kk;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const size_t base = size_t(blockIdx.x) * total;
	bool serial = nlists < kk || nlists > kMergeHeadsMax;
	if (!serial) {
		// a head: row and distance loaded together (the slot exists whether or not the list holds an entry)
		auto head = [&](uint32_t l) {
			unsigned long long k = ~0ull;
			if (l < nlists) {
				const uint32_t r = part_row[base + size_t(l) * kk];
				const float d = part_dist[base + size_t(l) * kk];
				if (r != kInvalidRow) k = merge_pair_key(d, r);
			}
			return k;
		};
		const uint32_t runs = (nlists + kWave - 1) / kWave, per_run = kk < uint32_t(kWave) ? kk : uint32_t(kWave);
		unsigned long long bound;
		if (tid == 0) s_n = 0;
		if (nlists <= 2 * kMergeThreads && runs * per_run <= kMergeRankMax) {   // workgroup-uniform
			unsigned long long h0 = head(tid), h1 = head(kMergeThreads + tid);
			h0 = merge_wave_sort(h0, lane);
			if (runs > uint32_t(kMergeWaves)) h1 = merge_wave_sort(h1, lane);
			if (uint32_t(lane) < per_run) {
				if (uint32_t(wave) < runs) s_key[wave * per_run + lane] = h0;
				if (uint32_t(kMergeWaves + wave) < runs) s_key[(kMergeWaves + wave) * per_run + lane] = h1;
			}
			merge_kth_key(s_key, runs * per_run, kk, &s_key[kMergeRankMax]);
			bound = s_key[kMergeRankMax];
		} else {
			uint32_t n1 = 64;
			while (n1 < nlists) n1 <<= 1;
			for (uint32_t l = tid; l < n1; l += kMergeThreads) {
				s_key[l] = head(l);
				s_val[l] = 0.f;
			}
			__syncthreads();
			merge_bitonic(s_key, s_val, n1);
			bound = s_key[kk - 1];
		}
		// bound = ~0: fewer than kk non-empty lists — everything valid is a candidate
		__syncthreads();
		// (the candidates overwrite the heads: every thread has read the bound)
		for (uint32_t l = tid; l < nlists; l += kMergeThreads) {
			const size_t at = base + size_t(l) * kk;
			bool more = true;
			for (uint32_t e0 = 0; e0 < kk && more; e0 += kMergeWalkAhead) {
				uint32_t r[kMergeWalkAhead];
				float d[kMergeWalkAhead];
#pragma unroll
				for (uint32_t u = 0; u < kMergeWalkAhead; ++u) {
					r[u] = kInvalidRow;
					d[u] = __builtin_inff();
					if (e0 + u < kk) {
						r[u] = part_row[at + e0 + u];
						d[u] = part_dist[at + e0 + u];
					}
				}
#pragma unroll
				for (uint32_t u = 0; u < kMergeWalkAhead; ++u) {
					const unsigned long long k = merge_pair_key(d[u], r[u]);
					more = more && r[u] != kInvalidRow && k <= bound;
					if (more) {
						const uint32_t pos = atomicAdd(&s_n, 1u);
						if (pos < kMergeCandMax) {
							s_key[pos] = k;
							s_val[pos] = d[u];
						}
					}
				}
			}
		}
		__syncthreads();
		const uint32_t n = s_n;
		serial = n > kMergeCandMax;
		if (!serial) {
			merge_write_sorted(s_key, s_val, n, kk, out_dist, out_row, out_count);
			return true;
		}
		__syncthreads();
	}
	// the insertion merge over the same lists (LDS reused for the wavefronts' lists)
	merge_by_insertion<TK>(part_dist, part_row, base, total, kk, out_dist, out_row, out_count, s_val, reinterpret_cast<uint32_t*>(s_key));
	return false;
}

// path (optional, test instrumentation): [query] 1 = the selection answered, 0 = the insertion merge
template <typename TK>
__global__ __launch_bounds__(kMergeThreads) void knn_merge_lists(const float* part_dist, const uint32_t* part_row, uint32_t nlists, uint32_t kk,
																  float* out_dist, uint32_t* out_row, uint32_t* out_count, const uint32_t* gate_cnt,
																  uint32_t gate_cap, uint32_t* path) {
	__shared__ unsigned long long s_key[kMergeHeadsMax];
	__shared__ float s_val[kMergeHeadsMax];
	__shared__ uint32_t s_n;
	if (gate_cnt && gate_cnt[blockIdx.x] <= gate_cap) return;   // workgroup-uniform (knn_merge's gate)
	const bool fast = merge_lists<TK>(part_dist, part_row, nlists, kk, out_dist, out_row, out_count, s_key, s_val, &s_n);
	if (path && threadIdx.x == 0) path[blockIdx.x] = fast ? 1u : 0u;
}

// The re-scored candidates of a pruned chain -> the exact top-kk without serial insertions: the rule of merge_lists for UNSORTED groups.  Thread
// t owns candidates t, t + kMergeThreads, ...; its smallest key is the head of that group, the kk-th smallest head bounds the kk-th best
// overall, and a second walk (the candidates are in L2 by then) collects every key at or below the bound: for candidates in list order little
// more than kk.  Up to kMergeThreads candidates need no heads: all of them are collected.  Returns false, workgroup-uniform and with nothing
// written, when merge_by_insertion has to answer: a NaN distance (pair_lt is no order over NaN, so its answer is the definition), fewer than kk
// non-empty groups (no bound), more than kMergeCandMax entries collected (masses of equal distances).  kk <= 64.
__device__ __forceinline__ bool merge_select(const float* cand_dist, const uint32_t* cand_row, size_t base, uint32_t cnt, uint32_t kk, float* out_dist,
											 uint32_t* out_row, uint32_t* out_count, unsigned long long* s_key, float* s_val, uint32_t* s_np) {
	uint32_t& s_n = *s_np;
	const uint32_t tid = threadIdx.x;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// one trip of a walk: kMergeAhead candidates of this thread, their loads issued together
	auto walk = [&](auto&& each) {
		for (uint32_t c0 = tid; c0 < cnt; c0 += kMergeThreads * kMergeAhead) {
			float cd[kMergeAhead];
			uint32_t ci[kMergeAhead];
#pragma unroll
			for (int u = 0; u < kMergeAhead; ++u) {
				const uint32_t c = c0 + uint32_t(u) * kMergeThreads;
				cd[u] = __builtin_inff();
				ci[u] = kInvalidRow;
				if (c < cnt) {
					cd[u] = cand_dist[base + c];
					ci[u] = cand_row[base + c];
				}
			}
#pragma unroll
			for (int u = 0; u < kMergeAhead; ++u) {
				if (ci[u] != kInvalidRow) each(cd[u], ci[u]);
			}
		}
	};
	uint32_t& s_nan = *reinterpret_cast<uint32_t*>(&s_val[kMergeHeadsMax - 1]);   // (a word neither the heads nor the collected entries reach)
	if (tid == 0) {
		s_n = 0;
		s_nan = 0;
	}
	__syncthreads();
	unsigned long long bound = ~0ull;
	bool nan = false;
	if (cnt > uint32_t(kMergeThreads)) {   // workgroup-uniform
		unsigned long long h = ~0ull;
		walk([&](float d, uint32_t r) {
			nan |= d != d;
			const unsigned long long k = merge_pair_key(d, r);
			h = k < h ? k : h;
		});
		h = merge_wave_sort(h, lane);
		if (uint32_t(lane) < kk) s_key[uint32_t(wave) * kk + lane] = h;
		if (nan) s_nan = 1;
		__syncthreads();
		if (s_nan) return false;
		const uint32_t m = uint32_t(kMergeWaves) * kk;   // <= 512 keys
		if (m <= kMergeRankMax) {
			merge_kth_key(s_key, m, kk, &s_key[kMergeRankMax]);
			bound = s_key[kMergeRankMax];
		} else {
			if (tid >= m) s_key[tid] = ~0ull;   // kk = 33 .. 64: 264 .. 512 keys, padded to the 512 the sort takes
			s_val[tid] = 0.f;
			__syncthreads();
			merge_bitonic(s_key, s_val, kMergeThreads);
			bound = s_key[kk - 1];
		}
		if (bound == ~0ull) return false;
		__syncthreads();   // (the candidates overwrite the heads: every thread has read the bound)
	}
	walk([&](float d, uint32_t r) {
		nan |= d != d;
		const unsigned long long k = merge_pair_key(d, r);
		if (k <= bound) {
			const uint32_t pos = atomicAdd(&s_n, 1u);
			if (pos < kMergeCandMax) {
				s_key[pos] = k;
				s_val[pos] = d;
			}
		}
	});
	if (nan) s_nan = 1;
	__syncthreads();
	if (s_nan) return false;
	const uint32_t n = s_n;
	if (n > kMergeCandMax) return false;
	merge_write_sorted(s_key, s_val, n, kk, out_dist, out_row, out_count);
	return true;
}

// The one merge at the end of a pruned chain (rxgpu_knn_chains.hip), one workgroup per query.  Gate closed (cand_cnt <= cap): the pruned chain
// answers — merge_select over the cand_cnt re-scored candidates (kk <= 64), merge_by_insertion where that declines.  Gate open: the exact scan behind the gate has
// run — merge_lists over its lists.  path (optional, test instrumentation): [query] 1 = a selection answered, 0 = an insertion merge.
template <typename TK>
__global__ __launch_bounds__(kMergeThreads) void knn_merge_final(const float* cand_dist, const uint32_t* cand_row, const uint32_t* cand_cnt, uint32_t cap,
																  const float* part_dist, const uint32_t* part_row, uint32_t nlists, uint32_t kk,
																  float* out_dist, uint32_t* out_row, uint32_t* out_count, uint32_t* path) {
	__shared__ unsigned long long s_key[kMergeHeadsMax];
	__shared__ float s_val[kMergeHeadsMax];
	__shared__ uint32_t s_n;
	const uint32_t cnt = cand_cnt[blockIdx.x];   // workgroup-uniform
	bool fast;
	if (cnt <= cap) {
		fast = merge_select(cand_dist, cand_row, size_t(blockIdx.x) * cap, cnt, kk, out_dist, out_row, out_count, s_key, s_val, &s_n);
		if (!fast) {
			__syncthreads();   // (the wavefronts' lists reuse the LDS of the selection)
			merge_by_insertion<WaveTopK>(cand_dist, cand_row, size_t(blockIdx.x) * cap, cnt, kk, out_dist, out_row, out_count, s_val, reinterpret_cast<uint32_t*>(s_key));
		}
	} else {
		fast = merge_lists<TK>(part_dist, part_row, nlists, kk, out_dist, out_row, out_count, s_key, s_val, &s_n);
	}
	if (path && threadIdx.x == 0) path[blockIdx.x] = fast ? 1u : 0u;
}

// Multi-GPU: fold the all-gathered per-shard lists of one query batch into the global top-kk.
// gathered: [world][2][nq][kk] 32-bit words — per shard the [nq][kk] distances followed by the [nq][kk] shard-local rows (what
// the scan writes when d_out_row == d_out_dist + nq*kk).  Global row = shard * shard_rows + local row; order = (dist, global row).
// slot_base (in-process RCCL path, rxgpu_sharded.hip): the global row base of every gathered position (rank-major, several shards per
// device, padded positions = kInvalidRow and skipped); null: position w is shard w.
// sorted = 0: the lists are UNORDERED sets (the per-shard HNSW results, members of top_candidates): every entry is offered.
__global__ __launch_bounds__(64) void knn_merge_shards(const uint32_t* gathered, uint32_t world, uint32_t nq, uint32_t kk, uint32_t shard_rows,
														const uint32_t* slot_base, float* out_dist, uint32_t* out_row, uint32_t* out_count, uint32_t sorted) {
	const int lane = threadIdx.x;
	const uint32_t q = blockIdx.x;
	WaveTopK top;
	top.init(kk);
	for (uint32_t w = 0; w < world; ++w) {
		const uint32_t* rec = gathered + size_t(w) * 2 * nq * kk + size_t(q) * kk;
		const uint32_t base = slot_base ? slot_base[w] : w * shard_rows;
		if (base == kInvalidRow) continue;
		float cd = __builtin_inff();
		uint32_t ci = kInvalidRow;
		if (lane < int(kk)) {
			cd = __uint_as_float(rec[lane]);
			const uint32_t local = rec[size_t(nq) * kk + lane];
			if (local != kInvalidRow) ci = base + local;
		}
		uint64_t pm = __ballot(ci != kInvalidRow);
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(cd, src);
			const uint32_t i = __shfl(ci, src);
			if (!top.admits(d, i)) {
				if (sorted) break;   // each shard list is sorted
				continue;
			}
			top.insert(d, i, lane);
		}
	}
	if (lane < int(kk)) {
		out_dist[size_t(q) * kk + lane] = top.bd;
		out_row[size_t(q) * kk + lane] = top.bi;
	}
	if (lane == 0 && out_count) out_count[q] = top.filled;
}

// Sharded HNSW: one shard's search result ([nq][k] distances, [nq][k] local rows, [nq] counts <= k) into its slot of the exchange's send
// buffer — [nq][kk] distances | [nq][kk] rows, entries past a query's count = (+inf, kInvalidRow), which knn_merge_shards skips.
__global__ __launch_bounds__(256) void knn_pack_lists(const float* dist, const uint32_t* row, const uint32_t* count, uint32_t nq, uint32_t k, uint32_t kk,
													   uint32_t* dst_dist, uint32_t* dst_row) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nq * kk) return;
	const uint32_t q = i / kk, j = i % kk;
	const bool have = j < k && j < count[q];
	dst_dist[i] = have ? __float_as_uint(dist[size_t(q) * k + j]) : 0x7F800000u;
	dst_row[i] = have ? row[size_t(q) * k + j] : kInvalidRow;
}

// ------------------------------------------------------------------------------------------ launchers

// Precondition: kk <= kMaxFusedK (one entry per lane).  The callers are the batched tail, which enqueue_knn reaches only with kk <= kMaxFusedK,
// and rxgpu_knn_merge_probe, which refuses more; wider lists are sorted lists and go through launch_merge_lists.
void launch_merge(const float* part_dist, const uint32_t* part_row, uint32_t total_per_query, uint32_t kk, uint32_t nq, float* out_dist,
				  uint32_t* out_row, uint32_t* out_count, const uint32_t* gate_cnt, uint32_t gate_cap, hipStream_t s) {
	hipLaunchKernelGGL(knn_merge, dim3(nq), dim3(kMergeThreads), 0, s, part_dist, part_row, total_per_query, kk, out_dist, out_row, out_count,
					   gate_cnt, gate_cap);
}

// the partial results are SORTED lists of kk entries (nlists per query): knn_merge_lists
void launch_merge_lists(const float* part_dist, const uint32_t* part_row, uint32_t nlists, uint32_t kk, uint32_t nq, float* out_dist, uint32_t* out_row,
						uint32_t* out_count, hipStream_t s, const uint32_t* gate_cnt, uint32_t gate_cap, uint32_t* path) {
	if (kk > uint32_t(kMaxFusedK)) {
		hipLaunchKernelGGL((knn_merge_lists<WaveTopK2>), dim3(nq), dim3(kMergeThreads), 0, s, part_dist, part_row, nlists, kk, out_dist, out_row, out_count,
						   gate_cnt, gate_cap, path);
	} else {
		hipLaunchKernelGGL((knn_merge_lists<WaveTopK>), dim3(nq), dim3(kMergeThreads), 0, s, part_dist, part_row, nlists, kk, out_dist, out_row, out_count,
						   gate_cnt, gate_cap, path);
	}
}

// the end of a pruned chain: the candidates (cand_cnt <= cap) or the exact scan's nlists sorted lists (knn_merge_final)
void launch_merge_final(const float* cand_dist, const uint32_t* cand_row, const uint32_t* cand_cnt, uint32_t cap, const float* part_dist,
						const uint32_t* part_row, uint32_t nlists, uint32_t kk, uint32_t nq, float* out_dist, uint32_t* out_row, uint32_t* out_count,
						hipStream_t s, uint32_t* path) {
	if (kk > uint32_t(kMaxFusedK)) {   // (the pruned chains keep kk <= 64: the candidate branch holds one entry per lane)
		hipLaunchKernelGGL((knn_merge_final<WaveTopK2>), dim3(nq), dim3(kMergeThreads), 0, s, cand_dist, cand_row, cand_cnt, cap, part_dist, part_row, nlists, kk,
						   out_dist, out_row, out_count, path);
	} else {
		hipLaunchKernelGGL((knn_merge_final<WaveTopK>), dim3(nq), dim3(kMergeThreads), 0, s, cand_dist, cand_row, cand_cnt, cap, part_dist, part_row, nlists, kk,
						   out_dist, out_row, out_count, path);
	}
}

void launch_merge_shards(const uint32_t* gathered, uint32_t world, uint32_t nq, uint32_t kk, uint32_t shard_rows, float* out_dist,
						 uint32_t* out_row, uint32_t* out_count, hipStream_t s, const uint32_t* slot_base, bool sorted) {
	hipLaunchKernelGGL(knn_merge_shards, dim3(nq), dim3(64), 0, s, gathered, world, nq, kk, shard_rows, slot_base, out_dist, out_row, out_count, sorted ? 1u : 0u);
}

void launch_pack_lists(const float* dist, const uint32_t* row, const uint32_t* count, uint32_t nq, uint32_t k, uint32_t kk, uint32_t* dst_dist, uint32_t* dst_row,
					   hipStream_t s) {
	const uint32_t total = nq * kk;
	if (!total) return;
	hipLaunchKernelGGL(knn_pack_lists, dim3((total + 255) / 256), dim3(256), 0, s, dist, row, count, nq, k, kk, dst_dist, dst_row);
}

}  // namespace rxgpu
