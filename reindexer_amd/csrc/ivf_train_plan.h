// The decisions of IVF training on the device (ivf_train.hip, rxgpu_ivf_assign / rxgpu_ivf_kmeans_step) that need no device, without HIP:
//   * how many training points one pass may take (the 2^24 rule),
//   * how the gathered block of prepared vectors is cut into chunks against a scratch budget,
//   * how the positions of a training list are placed into per-centroid segments IN LIST ORDER (block spans, the table of per-block
//     counts, the segment offsets, a position's slot) — the ordered sums of compute_centroids (Clustering.cpp:153-230) walk these segments,
//   * which (centroid, column tile) a wavefront of the sums kernel owns,
//   * where everything lies in the one scratch buffer of a k-means step.
// Arithmetic on counts only: tests/test_ivf_train_plan.py pins it on the CPU (tests/cpp/ivf_train_plan_cpu.cc); the kernels call the same
// inline functions, so the layout the host sizes is the layout the device walks.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RX_IVF_HD __host__ __device__
#else
#define RX_IVF_HD
#endif

namespace rxgpu {

// compute_centroids counts a centroid's points with `hassign[c] += 1.0f`; the device counts integers and converts.  The two agree while a
// count stays below 2^24 (the first integer a float cannot hold is 2^24 + 1), so a step takes fewer points than that.
constexpr uint64_t kIvfTrainMaxPoints = 1ull << 24;
RX_IVF_HD inline bool ivf_train_points_ok(uint64_t n) { return n < kIvfTrainMaxPoints; }

// ---- the gathered block: prepared vectors [chunk][dim] f32 that the coarse quantiser's k = 1 search reads as device queries
constexpr uint64_t kIvfGatherBudgetBytes = 64ull << 20;   // default scratch budget of the block (RXGPU_IVF_TRAIN_SCRATCH_BYTES overrides it)
constexpr uint64_t kIvfGatherQuantum = 256;               // a chunk is whole query tiles of the batched search

// rows per chunk: as many whole quanta as the budget holds, one quantum at least (a budget below one quantum is exceeded by that one
// quantum), never more than n
RX_IVF_HD inline uint64_t ivf_gather_chunk_rows(uint64_t n, uint32_t dim, uint64_t budget_bytes) {
	const uint64_t row_bytes = uint64_t(dim ? dim : 1) * sizeof(float);
	uint64_t rows = budget_bytes / row_bytes / kIvfGatherQuantum * kIvfGatherQuantum;
	if (rows < kIvfGatherQuantum) rows = kIvfGatherQuantum;
	return rows < n ? rows : n;
}
RX_IVF_HD inline uint64_t ivf_gather_chunks(uint64_t n, uint64_t chunk_rows) { return chunk_rows ? (n + chunk_rows - 1) / chunk_rows : 0; }
struct IvfChunk {
	uint64_t first, rows;   // list positions [first, first + rows)
};
RX_IVF_HD inline IvfChunk ivf_gather_chunk(uint64_t n, uint64_t chunk_rows, uint64_t i) {
	const uint64_t first = i * chunk_rows;
	const uint64_t left = n - first;
	return IvfChunk{first, left < chunk_rows ? left : chunk_rows};
}

// ---- stable placement: position i of the list goes to slot seg_off[a] + (positions j < i with assign[j] == a), a = assign[i]
// The list is cut into `blocks` spans of `span` consecutive positions (a multiple of the tile a workgroup ranks at a time); workgroup b
// counts its span per centroid into row b of a table [blocks][nlist]; a column-wise exclusive prefix of the table gives every (span,
// centroid) its base inside the centroid's segment, the column totals are the counts, their exclusive prefix the segment offsets.
constexpr uint32_t kIvfPlaceTile = 256;                 // positions ranked at a time = threads of a placing workgroup
constexpr uint64_t kIvfPlaceTableWords = 4ull << 20;    // the table stays below 16 MiB ...
constexpr uint32_t kIvfPlaceMaxBlocks = 512;            // ... and the column prefix below 512 steps
struct IvfPlaceShape {
	uint32_t blocks;   // spans = workgroups (0: n == 0)
	uint32_t span;     // positions per span
};
RX_IVF_HD inline IvfPlaceShape ivf_place_shape(uint64_t n, uint64_t nlist) {
	if (n == 0) return IvfPlaceShape{0, kIvfPlaceTile};
	uint64_t max_blocks = kIvfPlaceTableWords / (nlist ? nlist : 1);
	if (max_blocks < 1) max_blocks = 1;
	if (max_blocks > kIvfPlaceMaxBlocks) max_blocks = kIvfPlaceMaxBlocks;
	const uint64_t tiles = (n + kIvfPlaceTile - 1) / kIvfPlaceTile;
	const uint64_t tiles_per_block = (tiles + max_blocks - 1) / max_blocks;
	const uint64_t span = tiles_per_block * kIvfPlaceTile;
	return IvfPlaceShape{uint32_t((n + span - 1) / span), uint32_t(span)};
}
// table entry of (span b, centroid c): centroids are contiguous, so the column prefix reads coalesced
RX_IVF_HD inline uint64_t ivf_place_table_index(uint32_t b, uint32_t c, uint32_t nlist) { return uint64_t(b) * nlist + c; }
// slot of a position: segment offset of its centroid + base of its span there + its rank among the span's earlier positions of the centroid
RX_IVF_HD inline uint32_t ivf_place_slot(uint32_t seg_off, uint32_t span_base, uint32_t rank_in_span) { return seg_off + span_base + rank_in_span; }

// The whole placement on the host, step for step what the kernels do (counts per span, column prefix, segment offsets, slots).
// assign[i] >= nlist marks a position without a centroid: it is left out (the device flags the call instead).  table: [blocks * nlist]
// scratch; seg_off [nlist + 1]; order [n] receives the positions, segment after segment.
inline void ivf_place_host(const uint32_t* assign, uint32_t n, uint32_t nlist, uint32_t* table, uint32_t* seg_off, uint32_t* order) {
	const IvfPlaceShape sh = ivf_place_shape(n, nlist);
	for (uint64_t i = 0; i < uint64_t(sh.blocks) * nlist; ++i) table[i] = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if (assign[i] < nlist) ++table[ivf_place_table_index(i / sh.span, assign[i], nlist)];
	}
	seg_off[0] = 0;
	for (uint32_t c = 0; c < nlist; ++c) {
		uint32_t run = 0;
		for (uint32_t b = 0; b < sh.blocks; ++b) {
			const uint64_t t = ivf_place_table_index(b, c, nlist);
			const uint32_t v = table[t];
			table[t] = run;
			run += v;
		}
		seg_off[c + 1] = seg_off[c] + run;
	}
	for (uint32_t i = 0; i < n; ++i) {   // ascending positions: the running base of a (span, centroid) is the rank
		if (assign[i] >= nlist) continue;
		const uint64_t t = ivf_place_table_index(i / sh.span, assign[i], nlist);
		order[ivf_place_slot(seg_off[assign[i]], table[t], 0)] = i;
		++table[t];
	}
}

// ---- the ordered sums: one wavefront per (centroid, tile of 64 columns), lane j holds the running sum of column col0 + j
constexpr uint32_t kIvfSumTileCols = 64;
constexpr uint32_t kIvfSumWavesPerBlock = 4;
constexpr uint32_t kIvfSumLoadsInFlight = 32;   // members whose row slices a wavefront loads ahead of the dependent adds
RX_IVF_HD inline uint32_t ivf_sum_tiles(uint32_t dim) { return (dim + kIvfSumTileCols - 1) / kIvfSumTileCols; }
RX_IVF_HD inline uint64_t ivf_sum_waves(uint64_t nlist, uint32_t dim) { return nlist * ivf_sum_tiles(dim); }
RX_IVF_HD inline uint64_t ivf_sum_blocks(uint64_t nlist, uint32_t dim) { return (ivf_sum_waves(nlist, dim) + kIvfSumWavesPerBlock - 1) / kIvfSumWavesPerBlock; }
struct IvfSumUnit {
	uint32_t centroid, col0, cols;   // columns [col0, col0 + cols), 1 <= cols <= 64
};
// wavefront w of the grid: the tiles of one centroid are neighbours, so a member's row is read by neighbouring wavefronts at about the same time
RX_IVF_HD inline IvfSumUnit ivf_sum_unit(uint64_t w, uint32_t dim) {
	const uint32_t tiles = ivf_sum_tiles(dim);
	const uint32_t tile = uint32_t(w % tiles);
	const uint32_t col0 = tile * kIvfSumTileCols;
	const uint32_t left = dim - col0;
	return IvfSumUnit{uint32_t(w / tiles), col0, left < kIvfSumTileCols ? left : kIvfSumTileCols};
}
// ---- the scratch of one k-means step, one allocation: every part starts on a 256-byte boundary
struct IvfTrainScratch {
	uint64_t o_table;       // u32 [blocks][nlist]   per-span counts, then bases
	uint64_t o_seg_off;     // u32 [nlist + 1]
	uint64_t o_seg_rows;    // u32 [n]               the members' ROW numbers, segment after segment, list order inside a segment
	uint64_t o_centroids;   // f32 [nlist][dim]
	uint64_t o_hassign;     // f32 [nlist]
	uint64_t o_flag;        // u32 [1]               positions without a centroid
	uint64_t bytes;
};
RX_IVF_HD inline uint64_t ivf_align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }
RX_IVF_HD inline IvfTrainScratch ivf_train_scratch(uint64_t n, uint64_t nlist, uint32_t dim) {
	const IvfPlaceShape sh = ivf_place_shape(n, nlist);
	IvfTrainScratch s{};
	s.o_table = 0;
	s.o_seg_off = ivf_align256(s.o_table + uint64_t(sh.blocks) * nlist * 4);
	s.o_seg_rows = ivf_align256(s.o_seg_off + (nlist + 1) * 4);
	s.o_centroids = ivf_align256(s.o_seg_rows + n * 4);
	s.o_hassign = ivf_align256(s.o_centroids + nlist * dim * 4);
	s.o_flag = ivf_align256(s.o_hassign + nlist * 4);
	s.bytes = ivf_align256(s.o_flag + 4);
	return s;
}

}  // namespace rxgpu
