// Small device helpers shared by the ft_fast kernels (the units of the dense train, ft_sparse.hip, ft_phrase.hip): wavefront scans, the
// ordered prefix over all workgroups of a launch (decoupled look-back in ticket order), a list's segment of a document range, the posting
// loads and fills of the posting-side kernels, and 16-bit cells in LDS words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rxgpu_internal.h"

namespace rxgpu {
namespace {

constexpr unsigned long long kLbPrefix = 1ull << 63;
constexpr unsigned long long kLbAggregate = 1ull << 62;

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, int lane) {
#pragma unroll
	for (int off = 1; off < 64; off <<= 1) {
		const uint32_t o = __shfl_up(v, off, 64);
		if (lane >= off) v += o;
	}
	return v;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
	return v;
}

// Exclusive prefix of `count` over ALL threads of ALL workgroups in ticket order (256 threads per workgroup).
// lookback[] is zeroed before the launch; *grand_incl = inclusive total up to and including this workgroup.
__device__ inline uint32_t ordered_prefix(uint32_t count, uint32_t ticket, unsigned long long* lookback, uint32_t* error_flag, uint32_t* grand_incl) {
	__shared__ uint32_t s_wave_tot[4];
	__shared__ uint32_t s_block_excl;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const uint32_t incl = wave_inclusive_scan(count, lane);
	if (lane == 63) s_wave_tot[wave] = incl;
	__syncthreads();
	uint32_t before = 0;
	for (int w = 0; w < wave; ++w) before += s_wave_tot[w];
	const uint32_t block_total = s_wave_tot[0] + s_wave_tot[1] + s_wave_tot[2] + s_wave_tot[3];
	if (wave == 0) {
		if (lane == 0) {
			__hip_atomic_store(&lookback[ticket], (ticket == 0 ? kLbPrefix : kLbAggregate) | block_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
		uint32_t excl = 0;
		long long j = (long long)ticket - 1;   // nearest predecessor
		while (j >= 0) {
			const long long idx = j - lane;
			unsigned long long st = 0;
			if (idx >= 0) {
				uint32_t spins = 0;
				do {
					st = __hip_atomic_load(&lookback[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					if (st) break;
					__builtin_amdgcn_s_sleep(1);
					if ((++spins & 1023u) == 0 &&
						(spins > (1u << 24) || __hip_atomic_load(error_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
						__hip_atomic_store(error_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // never hang the GPU: bail out, the host reports it
						st = kLbPrefix;
						break;
					}
				} while (true);
			}
			const unsigned long long pm = __ballot(idx >= 0 && (st & kLbPrefix));
			const int first = pm ? __ffsll((long long)pm) - 1 : 63;
			excl += wave_sum((idx >= 0 && lane <= first) ? uint32_t(st & 0xFFFFFFFFull) : 0u);
			if (pm) break;
			j -= 64;
		}
		if (lane == 0) {
			if (ticket != 0) __hip_atomic_store(&lookback[ticket], kLbPrefix | (unsigned long long)(excl + block_total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			s_block_excl = excl;
		}
	}
	__syncthreads();
	const uint32_t be = s_block_excl;
	*grand_incl = be + block_total;
	__syncthreads();   // the shared words are reused by the caller's next call
	return be + before + (incl - count);
}

__device__ __forceinline__ uint32_t grab_ticket(uint32_t* ticket) {
	__shared__ uint32_t s_ticket;
	if (threadIdx.x == 0) s_ticket = atomicAdd(ticket, 1u);
	__syncthreads();
	return s_ticket;
}

// block of a posting-side grid -> its sub-term (every entry owns at least one block; entries ascend by block_base)
__device__ __forceinline__ FtGridEntry grid_entry(const FtGridEntry* g, uint32_t n, uint32_t block) {
	uint32_t lo = 0, hi = n - 1;
	while (lo < hi) {
		const uint32_t mid = (lo + hi + 1) >> 1;
		if (g[mid].block_base <= block) {
			lo = mid;
		} else {
			hi = mid - 1;
		}
	}
	return g[lo];
}

// A posting list's segment [lo, hi) of document range `range` (FtPosSubterm / FtPlan::SpSub: range_off[k] = first posting with
// doc >= k * kFtRangeDocs; ranges past the index of the list are empty at its end)
template <typename Sub>
__device__ __forceinline__ uint32_t ft_seg_lo(const Sub& s, uint32_t range) { return range < s.n_ranges ? s.range_off[range] : uint32_t(s.n); }
template <typename Sub>
__device__ __forceinline__ uint32_t ft_seg_hi(const Sub& s, uint32_t range) { return range + 1 < s.n_ranges ? s.range_off[range + 1] : uint32_t(s.n); }

// The doc ids of a thread's kFtPassItems consecutive postings (one 16-byte load away from the tail)
__device__ __forceinline__ void load_docs(const FtPosSubterm& s, uint64_t i0, uint32_t (&docs)[kFtPassItems], bool (&live)[kFtPassItems]) {
	static_assert(kFtPassItems == 4, "the vector load reads four document ids");
	if (i0 + kFtPassItems <= s.n) {
		const uint4 v = *reinterpret_cast<const uint4*>(s.doc + i0);   // i0 % 4 == 0 and the list is 256-byte aligned
		docs[0] = v.x;
		docs[1] = v.y;
		docs[2] = v.z;
		docs[3] = v.w;
#pragma unroll
		for (int k = 0; k < kFtPassItems; ++k) live[k] = true;
	} else {
#pragma unroll
		for (int k = 0; k < kFtPassItems; ++k) {
			live[k] = i0 + k < s.n;
			docs[k] = live[k] ? s.doc[i0 + k] : 0u;
		}
	}
}

__device__ __forceinline__ void fill_words(uint32_t* ptr, uint64_t n, uint32_t value, uint64_t gtid, uint64_t gsize) {
	if (!ptr || !n) return;
	const uint64_t n4 = n / 4;
	uint4* p4 = reinterpret_cast<uint4*>(ptr);   // every scratch region starts on a 256-byte boundary
	const uint4 v = make_uint4(value, value, value, value);
	for (uint64_t i = gtid; i < n4; i += gsize) p4[i] = v;
	for (uint64_t i = n4 * 4 + gtid; i < n; i += gsize) ptr[i] = value;
}

// 16-bit minimum in an LDS table of packed halves (there are no 16-bit LDS atomics; contention is one posting per (document, sub-term))
__device__ __forceinline__ void lds_min_u16(uint32_t* words, uint32_t idx, uint32_t v) {
	uint32_t* w = words + (idx >> 1);
	const uint32_t sh = (idx & 1u) * 16u;
	uint32_t old = *w;
	while (((old >> sh) & 0xFFFFu) > v) {
		const uint32_t nw = (old & ~(0xFFFFu << sh)) | (v << sh);
		const uint32_t prev = atomicCAS(w, old, nw);
		if (prev == old) break;
		old = prev;
	}
}
__device__ __forceinline__ uint32_t lds_get_u16(const uint32_t* words, uint32_t idx) { return (words[idx >> 1] >> ((idx & 1u) * 16u)) & 0xFFFFu; }
__device__ __forceinline__ void lds_set_u16(uint32_t* words, uint32_t idx, uint32_t v) {   // plain store of one half (ds_write_b16)
	reinterpret_cast<uint16_t*>(words)[idx] = uint16_t(v);
}

// The first posting of every document of one range among the `n` records of its bucket ({doc, posting, rank bits, row | field << 16}, in any
// order): the 16-bit minimum of the rows per document into `tab` (kFtRangeDocs halves, preset to 0xFFFF), then, behind a barrier, every
// record is read again and first(e, record, row, document in the range) runs for the one that holds its document's minimum — a document
// has one posting per row, so exactly one record adds it.  A suppressed sub-term's records never add a document (mergerimpl.h:144-151).
// between(): the caller's phase stamp.  All 256 threads of the workgroup call this.
template <typename Between, typename First>
__device__ __forceinline__ void ft_first_postings(const uint4* rec, uint32_t n, uint32_t* tab, uint32_t tid, Between&& between, First&& first) {
	for (uint32_t e = tid; e < n; e += 256) {
		const uint4 r = rec[e];
		if (r.z != kFtSuppressedRank) lds_min_u16(tab, r.x & (kFtRangeDocs - 1), r.w & 0xFFFFu);
	}
	__syncthreads();
	between();
	for (uint32_t e = tid; e < n; e += 256) {
		const uint4 r = rec[e];
		const uint32_t row = r.w & 0xFFFFu, dl = r.x & (kFtRangeDocs - 1);
		if (lds_get_u16(tab, dl) != row || r.z == kFtSuppressedRank) continue;
		first(e, r, row, dl);
	}
}

}  // namespace
}  // namespace rxgpu
