// The decisions of the batched level-0 build of an HNSW graph on the device (hnsw_build.hip, rxgpu_hnsw_build.hip, host/gpu_hnsw_map.cc) as
// pure functions: the batch schedule, which builds take the device path at all, what the selection kernel keeps in LDS, and the layout of the
// scratch the pair grouping uses.  No HIP in here — the file compiles for the host on its own (tests/cpp/hnsw_build_plan_cpu.cc,
// tests/test_hnsw_build_plan.py).
//
// The batch rule (known difference (3)): nodes [0, L) are linked; a batch [a, b) with a = L and
//   b - a = min(max(a / ratio, kHnswBuildMinBatch), cap, n - a)
// is searched against the graph of the nodes < a, so the rows of one batch do not see each other.  While L < seed the rows go in one by
// one through the sequential builder.  Level 1 of a batch follows the same rule one level up where RXGPU_HNSW_BUILD_UPPER=device says so
// (the second half of this file).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <string_view>

namespace rxgpu {

constexpr uint64_t kHnswBuildSeed = 1024;        // RXGPU_HNSW_BUILD_SEED: nodes the sequential builder links before the first batch
constexpr uint64_t kHnswBuildRatio = 16;         // RXGPU_HNSW_BUILD_RATIO: a batch is at most 1 / ratio of the graph it searches ...
constexpr uint64_t kHnswBuildMinBatch = 64;      // ... but never below this
constexpr uint64_t kHnswBuildBatchCap = 16384;   // RXGPU_HNSW_BUILD_BATCH: rows per batch at most
constexpr uint32_t kHnswBuildMaxM = 64;          // the device path takes M <= 64 (lists of 2 M <= 128 entries) ...
constexpr uint32_t kHnswBuildMaxEfc = 256;       // ... and efConstruction <= 256: the candidates of a row fit the selection kernel's arrays
constexpr uint32_t kHnswBuildEntries = 256;      // entries (candidates; current links + incoming rows) one wavefront orders in LDS
constexpr uint32_t kHnswBuildLdsBudget = 64 * 1024;   // static + dynamic LDS of one selection workgroup

struct HnswBuildKnobs {
	uint64_t seed = kHnswBuildSeed, ratio = kHnswBuildRatio, batch_cap = kHnswBuildBatchCap;
};
// the three hooks, read per call (tests flip them between calls); anything unparsable or zero keeps the default
inline HnswBuildKnobs read_hnsw_build_knobs() {
	HnswBuildKnobs k;
	auto take = [](const char* name, uint64_t& v) {
		const char* e = std::getenv(name);
		if (!e || !*e) return;
		char* end = nullptr;
		const unsigned long long x = std::strtoull(e, &end, 10);
		if (end != e && *end == 0 && x > 0) v = x;
	};
	take("RXGPU_HNSW_BUILD_SEED", k.seed);
	take("RXGPU_HNSW_BUILD_RATIO", k.ratio);
	take("RXGPU_HNSW_BUILD_BATCH", k.batch_cap);
	return k;
}

// Rows the sequential builder still has to insert when `linked` nodes are linked and `n` rows are stored: up to the seed size.
inline uint64_t hnsw_build_seed_rows(uint64_t linked, uint64_t n, const HnswBuildKnobs& k) {
	const uint64_t seed = std::max<uint64_t>(k.seed, 1);   // the first node has nothing to search
	if (linked >= seed || linked >= n) return 0;
	return std::min(seed, n) - linked;
}
// Rows of the batch that starts at node a (a >= 1) of n stored rows; 0: nothing is pending.
inline uint64_t hnsw_build_batch_rows(uint64_t a, uint64_t n, const HnswBuildKnobs& k) {
	if (a >= n) return 0;
	const uint64_t by_ratio = std::max<uint64_t>(a / std::max<uint64_t>(k.ratio, 1), kHnswBuildMinBatch);
	return std::min(std::min(by_ratio, std::max<uint64_t>(k.batch_cap, 1)), n - a);
}

// Which builds the device path takes: graphs without deleted nodes, M <= 64, efConstruction <= 256, one device.  Anything else keeps the
// host insertions (and the statistics say so).
enum HnswBuildPath : int { kHnswBuildDevice = 0, kHnswBuildHostDeleted = 1, kHnswBuildHostM = 2, kHnswBuildHostEfc = 3, kHnswBuildHostSharded = 4 };
inline int hnsw_build_path(uint64_t deleted_nodes, uint32_t M, uint32_t ef_construction, bool sharded) {
	if (sharded) return kHnswBuildHostSharded;
	if (deleted_nodes != 0) return kHnswBuildHostDeleted;
	if (M == 0 || M > kHnswBuildMaxM) return kHnswBuildHostM;
	if (ef_construction == 0 || ef_construction > kHnswBuildMaxEfc) return kHnswBuildHostEfc;
	return kHnswBuildDevice;
}

// LDS of one hnsw_build_select workgroup (one wavefront, one new row): the fixed arrays — ids, distances and order of the candidates, the
// kept entries and the heap that fixes their written order — and, where they fit beside them, the new row and the rows kept so far
// ((1 + M) rows of row_stride floats).  Past the budget the rows are read from L2 instead.
struct HnswBuildLds {
	uint32_t fixed_bytes;   // the static arrays
	uint32_t rows_bytes;    // dynamic: (1 + M) * row_stride * 4 when kept_in_lds, else 0
	bool kept_in_lds;
};
constexpr uint32_t hnsw_build_fixed_lds_bytes() {
	// cand id / dist / sorted position: 3 x 256 words; kept id / dist: 2 x 128; heap id / dist: 2 x 128
	return (3 * kHnswBuildEntries + 4 * 128) * 4;
}
inline HnswBuildLds hnsw_build_select_lds(uint32_t row_stride, uint32_t M) {
	HnswBuildLds l{};
	l.fixed_bytes = hnsw_build_fixed_lds_bytes();
	const uint64_t rows = (uint64_t(M) + 1) * row_stride * 4;
	l.kept_in_lds = uint64_t(l.fixed_bytes) + rows <= kHnswBuildLdsBudget;
	l.rows_bytes = l.kept_in_lds ? uint32_t(rows) : 0;
	return l;
}

// Scratch of one batch of `rows` new rows (M links each at most, k candidates each) over a graph allocated for `nodes_cap` nodes.  Byte
// offsets, every area 256-byte aligned.  Two areas are per NODE and live as long as the graph arrays (node_cnt is all zero between
// batches: the grouping leaves it so); the others are per batch.
struct HnswBuildScratch {
	uint64_t pairs;          // rows * M: upper bound of the (target, new row) pairs of a batch = of the targets touched
	uint64_t o_cand_dist, o_cand_row;   // [rows][k] the searches' lists (HnswSink)
	uint64_t o_queries;      // [rows][dim] the new rows packed (only where the row stride is padded)
	uint64_t o_pair_t;       // [pairs] target of pair slot (row, j), kInvalidRow: unused
	uint64_t o_inc;          // [pairs] new rows grouped by target
	uint64_t o_touched;      // [pairs] the targets touched, in the order they were first met
	uint64_t o_tcnt, o_tseg; // [pairs] incoming rows / first entry in inc, by position in `touched`
	// A node past the kernel's cap holds more than kHnswBuildEntries - maxM0 >= 128 incoming rows, so a batch has at most pairs / 128 of them
	// and their entries (current links + incoming rows) number fewer than 2 * pairs: the second launch orders them in these arrays.
	uint64_t over_cap;       // entries of `over`
	uint64_t big_cap;        // entries of each big array
	uint64_t o_over;         // [over_cap] {position in `touched`, first entry in the big arrays}
	uint64_t o_big_id, o_big_dist, o_big_pos;   // [big_cap]
	uint64_t o_counters;     // 8 words: touched, entries of inc handed out, re-selected, past the cap, big entries handed out
	uint64_t bytes;
	uint64_t node_bytes;     // node_cnt [nodes_cap] + node_seg [nodes_cap]
};
inline HnswBuildScratch hnsw_build_scratch(uint64_t rows, uint32_t M, uint32_t max_m0, uint32_t k, uint32_t dim, bool pack_queries, uint64_t nodes_cap) {
	HnswBuildScratch s{};
	uint64_t at = 0;
	auto take = [&at](uint64_t bytes) {
		const uint64_t o = at;
		at = (at + bytes + 255) & ~uint64_t(255);
		return o;
	};
	s.pairs = rows * M;
	s.o_cand_dist = take(rows * k * 4);
	s.o_cand_row = take(rows * k * 4);
	s.o_queries = take(pack_queries ? rows * dim * 4 : 0);
	s.o_pair_t = take(s.pairs * 4);
	s.o_inc = take(s.pairs * 4);
	s.o_touched = take(s.pairs * 4);
	s.o_tcnt = take(s.pairs * 4);
	s.o_tseg = take(s.pairs * 4);
	s.over_cap = s.pairs / (kHnswBuildEntries - max_m0) + 1;
	s.big_cap = s.pairs + s.over_cap * max_m0;
	s.o_over = take(s.over_cap * 8);
	s.o_big_id = take(s.big_cap * 4);
	s.o_big_dist = take(s.big_cap * 4);
	s.o_big_pos = take(s.big_cap * 4);
	s.o_counters = take(8 * 4);
	s.bytes = at;
	s.node_bytes = nodes_cap * 8;
	return s;
}

// ---------------------------------------------------------------------------------------------------------------- level 1 of a batch
// The same rule one level up: U, the rows of the batch with level >= 1, are searched over the level-1 lists of the graph in
// front of the batch — reached by the greedy descent from its entry point through its levels >= 2 — given lists of M links at most and
// linked back with limit M.  Levels >= 2, the entry point and the top level stay on the host.

// RXGPU_HNSW_BUILD_UPPER, read per call: "device" moves level 1 of a batch to the device, "host" / unset / anything else keeps it on the
// host.  It only means something under RXGPU_HNSW_BUILD=device.
inline bool read_hnsw_build_upper_device() {
	const char* e = std::getenv("RXGPU_HNSW_BUILD_UPPER");
	return e && std::string_view(e) == "device";
}

// Whether level 1 of a batch goes to the device: the batch's level 0 does (path), the graph in front of it has a level-1 node to start
// from (its top level is >= 1; the top level only grows, so within a flush a "no" can only come in front of the first "yes"), and the
// batch holds a row of level >= 1.
inline bool hnsw_build_upper_on_device(bool upper_device, int path, int top_level_before, uint64_t upper_rows) {
	return upper_device && path == kHnswBuildDevice && top_level_before >= 1 && upper_rows > 0;
}

// Bytes of the dense level-1 view [nodes_cap][1 + M]: the level-1 lists as a level-0 array, so that the search, selection and back-link
// kernels run on level 1 as they are.
inline uint64_t hnsw_build_upper_view_bytes(uint64_t nodes_cap, uint32_t M) { return nodes_cap * (1 + uint64_t(M)) * 4; }

// Scratch of the level-1 step of one batch with `up_rows` rows in U: the batch scratch for up_rows rows whose lists hold M entries, and
// behind it (256-byte aligned like every area) the ids of U.  The queries are always packed: U is not contiguous.
struct HnswBuildUpperScratch {
	HnswBuildScratch batch;   // hnsw_build_scratch(up_rows, M, M, k, dim, true, nodes_cap)
	uint64_t o_row_ids;       // [up_rows]
	uint64_t bytes;
};
inline HnswBuildUpperScratch hnsw_build_upper_scratch(uint64_t up_rows, uint32_t M, uint32_t k, uint32_t dim, uint64_t nodes_cap) {
	HnswBuildUpperScratch s{};
	s.batch = hnsw_build_scratch(up_rows, M, M, k, dim, true, nodes_cap);
	s.o_row_ids = s.batch.bytes;
	s.bytes = (s.o_row_ids + up_rows * 4 + 255) & ~uint64_t(255);
	return s;
}

}  // namespace rxgpu
