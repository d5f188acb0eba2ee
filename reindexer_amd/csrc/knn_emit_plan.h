// Where the int8-pruned scan (knn_scan_i8.hip) puts the rows it emits, without HIP.  The scan's grid is gridx workgroups of kEmitWavesPerBlock
// wavefronts; wavefront w owns the sets w, w + nwaves, ... of kEmitRowsPerSet consecutive rows.  While it scans, a wavefront appends an 8-byte
// {lo, row} entry for every row whose lower bound can still matter, into a segment of its own: segments lie back to back in wavefront order,
// each exactly as large as the rows its wavefront scans, so emission can never overflow and needs no overflow path.  knn_filter_emitted
// (knn_filter.hip) then reads emit_cnt[w] entries of every segment.  Arithmetic on counts only — tests/test_knn_emit_plan.py pins it on the
// CPU (tests/cpp/knn_emit_plan_cpu.cc); the kernels take an EmitPlan by value, so nothing divides on the device.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RX_EMIT_HD __host__ __device__
#else
#define RX_EMIT_HD
#endif

namespace rxgpu {

constexpr uint64_t kEmitRowsPerSet = 16;        // rows per wavefront step (kI8RowsPerWave)
constexpr uint64_t kEmitWavesPerBlock = 4;      // kScanWaves

struct EmitEntry {   // one emitted row: its lower bound and itself
	float lo;
	uint32_t row;
};

struct EmitPlan {
	uint64_t n;        // rows scanned
	uint64_t nwaves;   // wavefronts of the grid
	uint64_t nsets;    // ceil(n / kEmitRowsPerSet)
	uint64_t q, r;     // nsets = q * nwaves + r: wavefronts below r own q + 1 sets, the others q
	uint64_t short_by; // rows the last set lacks (0..15)
	uint64_t last_w;   // the wavefront that owns the last set (n > 0)
};

RX_EMIT_HD inline uint64_t emit_wavefronts(uint64_t gridx) { return gridx * kEmitWavesPerBlock; }

RX_EMIT_HD inline EmitPlan emit_plan(uint64_t n, uint64_t gridx) {
	EmitPlan p{};
	p.n = n;
	p.nwaves = emit_wavefronts(gridx);
	p.nsets = (n + kEmitRowsPerSet - 1) / kEmitRowsPerSet;
	p.q = p.nwaves ? p.nsets / p.nwaves : 0;
	p.r = p.nwaves ? p.nsets % p.nwaves : 0;
	p.short_by = p.nsets * kEmitRowsPerSet - n;
	p.last_w = p.nsets && p.nwaves ? (p.nsets - 1) % p.nwaves : 0;
	return p;
}

// sets wavefront w scans
RX_EMIT_HD inline uint64_t emit_sets_of(const EmitPlan& p, uint64_t w) { return p.q + (w < p.r ? 1 : 0); }
// rows wavefront w scans = the capacity of its segment in entries
RX_EMIT_HD inline uint64_t emit_rows_of(const EmitPlan& p, uint64_t w) {
	return emit_sets_of(p, w) * kEmitRowsPerSet - (p.nsets && w == p.last_w ? p.short_by : 0);
}
// first entry of wavefront w's segment
RX_EMIT_HD inline uint64_t emit_segment_offset(const EmitPlan& p, uint64_t w) {
	const uint64_t sets_before = w * p.q + (w < p.r ? w : p.r);
	return sets_before * kEmitRowsPerSet - (p.nsets && w > p.last_w ? p.short_by : 0);
}
// the two context buffers, per call of nq queries: segments of a query cover n entries, one count per wavefront
RX_EMIT_HD inline uint64_t emit_buffer_bytes(uint64_t n, uint64_t nq) { return nq * n * uint64_t(sizeof(EmitEntry)); }
RX_EMIT_HD inline uint64_t emit_count_bytes(uint64_t gridx, uint64_t nq) { return nq * emit_wavefronts(gridx) * uint64_t(sizeof(uint32_t)); }

}  // namespace rxgpu
