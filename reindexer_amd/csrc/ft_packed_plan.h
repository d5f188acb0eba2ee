// The decisions of ONE packed upload (rxgpu_ft_set_words_packed_ptrs, rxgpu_ft_packed.hip), without HIP: everything the call works out from
// the streams' lengths before its first launch — launch order, offsets, pieces, staging layout, chunks, gather threads — and, once the
// counting pass has told how much every word decodes to, the layout of the pool.  Arithmetic on lengths only: no byte of a stream is read here,
// so tests/test_ft_packed_plan.py pins it on the CPU (tests/cpp/ft_packed_plan_cpu.cc).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "ft_merge_plan.h"
#include "ft_packed_decode.h"

namespace rxgpu {

struct FtPackedPlan {
	uint32_t nwords = 0;
	std::vector<uint32_t> order;        // launch position -> the caller's word
	std::vector<uint64_t> off, afp;     // launch order: (start, end) of every stream in the staging buffer; array_found_pos
	uint64_t total_bytes = 0;
	uint32_t nsegs = 0;                 // pieces of kFtPackedSegBytes (the wavefront kernels only, else 0) ...
	std::vector<uint32_t> seg_first;    // ... [nwords + 1]: the first piece of every word
	// pinned staging, mirrored on the device: [streams + 16 zero bytes | (start, end) pairs | array_found_pos | piece -> word | seg_first]
	size_t o_off = 0, o_afp = 0, o_sw = 0, o_sf = 0, in_bytes = 0;
	std::vector<uint32_t> chunk_first;  // [nchunks + 1]: the streams travel in chunks of whole words
	unsigned nthr = 1;                  // threads of the gather
	uint64_t len_of(uint32_t k) const { return off[2 * size_t(k) + 1] - off[2 * size_t(k)]; }
	uint32_t nchunks() const { return uint32_t(chunk_first.size() - 1); }
	void fill_seg_word(uint32_t* sw) const {   // the piece -> word table, [nsegs]
		for (uint32_t k = 0; k < nwords; ++k) std::fill(sw + seg_first[k], sw + seg_first[k + 1], k);
	}
	// the words [k, e) of chunk c that gather thread t moves
	void gather_range(uint32_t c, unsigned t, uint32_t& k, uint32_t& e) const {
		const uint32_t k0 = chunk_first[c], kn = chunk_first[c + 1] - k0;
		k = k0 + uint32_t(uint64_t(kn) * t / nthr);
		e = k0 + uint32_t(uint64_t(kn) * (t + 1) / nthr);
	}
};

// `wave`: one wavefront per word (pieces and checkpoints), else the one-thread-per-word kernels.  chunk_target: bytes after which a chunk
// is closed; ~0: one chunk.
inline FtPlanError ft_packed_plan(uint32_t nwords, const uint64_t* len, const uint64_t* array_found_pos, bool wave, uint64_t chunk_target, FtPackedPlan& p) {
	p = FtPackedPlan{};
	p.nwords = nwords;
	// wavefronts of similar work: the words are launched longest first (a wavefront lasts as long as its longest stream).  A bucket sort by
	// the length's power of two is enough for that — O(n); a comparison sort of a 100 000-word dictionary cost 8 ms of the call.
	p.order.resize(nwords);
	auto bucket_of = [&](uint32_t w) { return len[w] ? 64 - uint32_t(__builtin_clzll(len[w])) : 0u; };   // 0 .. 64
	uint32_t start[66] = {0};
	for (uint32_t w = 0; w < nwords; ++w) start[64 - bucket_of(w) + 1] += 1;
	for (int b = 0; b < 65; ++b) start[b + 1] += start[b];
	for (uint32_t w = 0; w < nwords; ++w) p.order[start[64 - bucket_of(w)]++] = w;
	p.off.resize(size_t(nwords) * 2);
	p.afp.resize(nwords);
	for (uint32_t k = 0; k < nwords; ++k) {
		p.off[2 * size_t(k)] = p.total_bytes;
		p.total_bytes += len[p.order[k]];
		p.off[2 * size_t(k) + 1] = p.total_bytes;
		p.afp[k] = array_found_pos[p.order[k]];
	}
	// pieces: the counting pass leaves a checkpoint in each, the writing pass runs one wavefront per piece
	if (wave) {
		p.seg_first.assign(size_t(nwords) + 1, 0);
		for (uint32_t k = 0; k < nwords; ++k) {
			const uint64_t pieces = std::max<uint64_t>(1, (p.len_of(k) + kFtPackedSegBytes - 1) / kFtPackedSegBytes);
			if (!(p.seg_first[k] + pieces < 0xFFFFFFFFull)) return FtPlanError{RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed: too many stream bytes in one call"};
			p.seg_first[k + 1] = uint32_t(p.seg_first[k] + pieces);
		}
		p.nsegs = p.seg_first[nwords];
	}
	p.o_off = ft_align256(size_t(p.total_bytes) + 16);
	p.o_afp = p.o_off + ft_align256(size_t(nwords) * 16);
	p.o_sw = p.o_afp + ft_align256(size_t(nwords) * 8);
	p.o_sf = p.o_sw + ft_align256(size_t(p.nsegs) * 4);
	p.in_bytes = p.o_sf + ft_align256((size_t(nwords) + 1) * 4);
	p.chunk_first.push_back(0);
	uint64_t acc = 0;
	for (uint32_t k = 0; k < nwords; ++k) {
		acc += p.len_of(k);
		if (acc >= chunk_target && k + 1 < nwords) {
			p.chunk_first.push_back(k + 1);
			acc = 0;
		}
	}
	p.chunk_first.push_back(nwords);
	// the gather: one pass over the streams by a few threads (100 000 pieces of a few hundred bytes: one thread moves ~7 GB/s of them)
	p.nthr = p.total_bytes > (8u << 20) ? 4u : 1u;
	return FtPlanError{};
}

// One pool for the whole call, every array of every word on a 256-byte boundary (the kernels read document ids 16 bytes at a time): the
// offsets of a word's eight arrays in the order they are carved.  A word without postings takes nothing.
struct FtPackedSlices {
	size_t doc = 0, pos_off = 0, fpos = 0, ent_off = 0, ent_field = 0, ent_tf = 0, ent_first = 0, range_off = 0;
	uint32_t n_ranges = 0;   // last_doc / kFtRangeDocs + 2
};
inline size_t ft_packed_pool(const FtPackedCounts* counts, uint32_t nwords, std::vector<FtPackedSlices>& sl) {
	FtCarver cv;
	sl.assign(nwords, FtPackedSlices{});
	for (uint32_t k = 0; k < nwords; ++k) {
		const FtPackedCounts& c = counts[k];
		if (!c.n) continue;
		FtPackedSlices& s = sl[k];
		s.doc = cv.take(size_t(c.n) * 4);
		s.pos_off = cv.take((size_t(c.n) + 1) * 4);
		s.fpos = cv.take(size_t(c.npos) * 8);
		s.ent_off = cv.take((size_t(c.n) + 1) * 4);
		s.ent_field = cv.take(size_t(c.nent));
		s.ent_tf = cv.take(size_t(c.nent) * 4);
		s.ent_first = cv.take(size_t(c.nent) * 4);
		s.n_ranges = c.last_doc / kFtRangeDocs + 2;
		s.range_off = cv.take(size_t(s.n_ranges) * 4);
	}
	return cv.off;
}

}  // namespace rxgpu
