// The decisions of one packed upload (reindexer_amd/csrc/ft_packed_plan.h) compiled for the host: tests/test_ft_packed_plan.py pins its rules
// on the CPU, tests/test_gpu_ft_routes.py holds the device path's pool against it.  Test infrastructure only — nothing in the product links this.
#include <cstdint>
#include <cstring>
#include <vector>

#include "ft_packed_plan.h"

extern "C" {

struct FtPackedPlanCpuOut {
	int32_t code;
	char msg[252];
	uint64_t scalars[8];     // total_bytes, nsegs, o_off, o_afp, o_sw, o_sf, in_bytes, nthr
	uint32_t nchunks, pad;
	uint32_t* order;         // [nwords]
	uint64_t* off;           // [nwords][2]
	uint64_t* afp;           // [nwords]
	uint32_t* seg_first;     // [nwords + 1]; untouched when the plan has no pieces
	uint32_t* seg_word;      // [nsegs]; may be null (the overflow cases: lengths only)
	uint32_t* chunk_first;   // [nwords + 1] at most
	uint32_t* gather;        // [nchunks][nthr][2]; may be null
};

// chunk_target: bytes, ~0 for none
int ft_packed_plan_cpu(uint32_t nwords, const uint64_t* len, const uint64_t* array_found_pos, int wave, uint64_t chunk_target, FtPackedPlanCpuOut* out) {
	rxgpu::FtPackedPlan p;
	const rxgpu::FtPlanError e = rxgpu::ft_packed_plan(nwords, len, array_found_pos, wave != 0, chunk_target, p);
	out->code = e.code;
	std::memset(out->msg, 0, sizeof(out->msg));
	std::strncpy(out->msg, e.msg.c_str(), sizeof(out->msg) - 1);
	if (e) return e.code;
	const uint64_t scalars[8] = {p.total_bytes, p.nsegs, p.o_off, p.o_afp, p.o_sw, p.o_sf, p.in_bytes, p.nthr};
	std::memcpy(out->scalars, scalars, sizeof(scalars));
	out->nchunks = p.nchunks();
	std::memcpy(out->order, p.order.data(), p.order.size() * 4);
	std::memcpy(out->off, p.off.data(), p.off.size() * 8);
	std::memcpy(out->afp, p.afp.data(), p.afp.size() * 8);
	if (!p.seg_first.empty()) std::memcpy(out->seg_first, p.seg_first.data(), p.seg_first.size() * 4);
	if (out->seg_word && p.nsegs) p.fill_seg_word(out->seg_word);
	std::memcpy(out->chunk_first, p.chunk_first.data(), p.chunk_first.size() * 4);
	for (uint32_t c = 0; out->gather && c < p.nchunks(); ++c) {
		for (unsigned t = 0; t < p.nthr; ++t) p.gather_range(c, t, out->gather[(size_t(c) * p.nthr + t) * 2], out->gather[(size_t(c) * p.nthr + t) * 2 + 1]);
	}
	return 0;
}

// counts: [nwords][4] n, npos, nent, last_doc.  slices: [nwords][8] offsets in carving order, n_ranges: [nwords]; both may be null.  Returns the pool's bytes.
uint64_t ft_packed_pool_cpu(uint32_t nwords, const uint32_t* counts, uint64_t* slices, uint32_t* n_ranges) {
	std::vector<rxgpu::FtPackedCounts> c(nwords);
	for (uint32_t k = 0; k < nwords; ++k) {
		c[k].n = counts[4 * k];
		c[k].npos = counts[4 * k + 1];
		c[k].nent = counts[4 * k + 2];
		c[k].last_doc = counts[4 * k + 3];
	}
	std::vector<rxgpu::FtPackedSlices> sl;
	const uint64_t bytes = rxgpu::ft_packed_pool(c.data(), nwords, sl);
	for (uint32_t k = 0; k < nwords; ++k) {
		const uint64_t s[8] = {sl[k].doc, sl[k].pos_off, sl[k].fpos, sl[k].ent_off, sl[k].ent_field, sl[k].ent_tf, sl[k].ent_first, sl[k].range_off};
		if (slices) std::memcpy(slices + 8 * size_t(k), s, sizeof(s));
		if (n_ranges) n_ranges[k] = sl[k].n_ranges;
	}
	return bytes;
}

uint32_t ft_packed_seg_bytes() { return rxgpu::kFtPackedSegBytes; }

}  // extern "C"
