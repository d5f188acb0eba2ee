// The segment layout of the emitting int8 scan (reindexer_amd/csrc/knn_emit_plan.h) checked on the host, stand-alone: tests/test_knn_emit_plan.py
// builds and runs it.  Every expectation is a restatement of the rule, by brute force: the sets are dealt to the wavefronts one by one and the
// rows counted.  Test infrastructure only — nothing in the product links this.
//   knn_emit_plan_cpu [max_n]      exit status 0: every check held
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_emit_plan.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                         \
	do {                                         \
		if (!(cond)) {                           \
			if (failures++ < 20) {               \
				std::printf("FAILED %s: ", #cond); \
				std::printf(__VA_ARGS__);        \
				std::printf("\n");               \
			}                                    \
		}                                        \
	} while (0)

// scan_i8_grid_x (knn_scan_i8.hip) restated: a workgroup per 4 sets of 16 rows, at most wg per CU
uint64_t grid_x(uint64_t n, uint64_t cus, uint64_t wg) {
	const uint64_t nsets = (n + 15) / 16, want = (nsets + 3) / 4, cap = cus * wg;
	return want < cap ? (want ? want : 1) : cap;
}

void check_layout(uint64_t n, uint64_t gridx) {
	const rxgpu::EmitPlan p = rxgpu::emit_plan(n, gridx);
	const uint64_t nwaves = gridx * 4, nsets = (n + 15) / 16;
	CHECK(p.nwaves == nwaves && p.nsets == nsets && p.n == n, "n=%llu gridx=%llu", (unsigned long long)n, (unsigned long long)gridx);
	CHECK(rxgpu::emit_wavefronts(gridx) == nwaves, "gridx=%llu", (unsigned long long)gridx);
	// deal the sets: wavefront w scans the sets w, w + nwaves, ..., the last set of all holds what is left of n
	std::vector<uint64_t> sets(nwaves, 0), rows(nwaves, 0);
	for (uint64_t s = 0; s < nsets; ++s) {
		sets[s % nwaves] += 1;
		rows[s % nwaves] += s + 1 < nsets ? 16 : n - 16 * s;
	}
	uint64_t at = 0;   // segments back to back in wavefront order: disjoint, and together exactly n entries
	for (uint64_t w = 0; w < nwaves; ++w) {
		CHECK(rxgpu::emit_sets_of(p, w) == sets[w], "n=%llu gridx=%llu w=%llu", (unsigned long long)n, (unsigned long long)gridx, (unsigned long long)w);
		CHECK(rxgpu::emit_rows_of(p, w) == rows[w], "n=%llu gridx=%llu w=%llu: %llu != %llu", (unsigned long long)n, (unsigned long long)gridx,
			  (unsigned long long)w, (unsigned long long)rxgpu::emit_rows_of(p, w), (unsigned long long)rows[w]);
		CHECK(rxgpu::emit_segment_offset(p, w) == at, "n=%llu gridx=%llu w=%llu: %llu != %llu", (unsigned long long)n, (unsigned long long)gridx,
			  (unsigned long long)w, (unsigned long long)rxgpu::emit_segment_offset(p, w), (unsigned long long)at);
		at += rows[w];
	}
	CHECK(at == n, "n=%llu gridx=%llu", (unsigned long long)n, (unsigned long long)gridx);
}

}  // namespace

int main(int argc, char** argv) {
	const uint64_t max_n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 70000;
	static_assert(sizeof(rxgpu::EmitEntry) == 8, "one 8-byte store per emitted row");
	for (uint64_t n = 1; n <= max_n; ++n) {
		for (uint64_t wg : {1, 2, 8}) check_layout(n, grid_x(n, 256, wg));
	}
	check_layout(40003, 256);   // every wavefront loops
	check_layout(5, 7);         // most wavefronts idle: empty segments at offset n
	// sizes in 64 bits: n = 2^32 - 1 rows, the largest grid, 8 queries
	const uint64_t big = 0xFFFFFFFFull, gx = grid_x(big, 256, 8);
	const rxgpu::EmitPlan p = rxgpu::emit_plan(big, gx);
	const uint64_t nwaves = gx * 4;
	CHECK(gx == 2048 && p.nsets == (1ull << 28), "gx=%llu", (unsigned long long)gx);
	CHECK(rxgpu::emit_buffer_bytes(big, 1) == 8 * big && rxgpu::emit_buffer_bytes(big, 8) == 64 * big, "buffer bytes");
	CHECK(rxgpu::emit_count_bytes(gx, 8) == 8 * nwaves * 4, "count bytes");
	uint64_t total = 0, prev_end = 0;
	for (uint64_t w = 0; w < nwaves; ++w) {
		const uint64_t sets = (p.nsets - w + nwaves - 1) / nwaves;   // sets w, w + nwaves, ... below nsets
		const uint64_t rows = sets * 16 - ((p.nsets - 1) % nwaves == w ? 1 : 0);   // 2^32 - 1 rows: the last set lacks one
		CHECK(rxgpu::emit_rows_of(p, w) == rows, "big w=%llu", (unsigned long long)w);
		CHECK(rxgpu::emit_segment_offset(p, w) == prev_end, "big w=%llu", (unsigned long long)w);
		prev_end += rows;
		total += rows;
	}
	CHECK(total == big && prev_end > (1ull << 31), "big total");
	std::printf("knn_emit_plan_cpu: %s (n up to %llu, %d failures)\n", failures ? "FAILED" : "ok", (unsigned long long)max_n, failures);
	return failures ? 1 : 0;
}
