// What the kernels of the batched level-0 build (hnsw_build.hip) take: one batch of new rows [first, first + n) of an index whose nodes
// < first are linked.  Layout and sizes of the scratch: hnsw_build_plan.h (HnswBuildScratch).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rxgpu {

// (kBuildCntError: 0 none, 1 the queue of nodes past the cap overflowed, 2 a list named a node past the batch)
enum : uint32_t { kBuildCntTouched = 0, kBuildCntInc = 1, kBuildCntReselected = 2, kBuildCntOver = 3, kBuildCntBig = 4, kBuildCntError = 5 };

struct HnswBuildArgs {
	const float* rows;          // [..][stride]
	const float* inv_norms;     // cosine: 1 / |row|
	uint32_t stride, dim;
	uint32_t* links0;           // [..][1 + maxM0]
	uint32_t M, maxM0;
	uint32_t first, n;          // the batch
	const uint32_t* cand_row;   // [n][k] what the search found for row first + r (kInvalidRow past its count)
	uint32_t k;
	uint32_t lds_rows;          // hnsw_build_select: the new row and the kept rows live in the dynamic LDS ((1 + M) * stride floats)
	uint32_t* pair_t;           // [n * M]
	uint32_t* node_cnt;         // [nodes] incoming rows of a node; zero outside a batch
	uint32_t* node_seg;         // [nodes] first entry of a touched node in inc
	uint32_t* touched;          // [n * M]
	uint32_t* tcnt;
	uint32_t* tseg;
	uint32_t* inc;              // [n * M]
	uint2* over;                // [over_cap]
	uint32_t over_cap;
	uint32_t* big_id;           // [big_cap]
	float* big_dist;
	uint32_t* big_pos;
	uint32_t big_cap;
	uint32_t* counters;         // [8], kBuildCnt*
};

// step 4: one wavefront per new row — its list, and the (target, row) pairs it creates, counted per target
void launch_hnsw_build_select(int metric, const HnswBuildArgs& a, hipStream_t s);
// pair grouping: a segment of inc per touched node, then the pairs into their segments (leaves node_cnt zero again)
void launch_hnsw_build_group(const HnswBuildArgs& a, hipStream_t s);
// step 5: one wavefront per touched node; nodes with more than kHnswBuildEntries entries are queued in `over` ...
void launch_hnsw_build_backlink(int metric, const HnswBuildArgs& a, hipStream_t s);
// ... and finished by this launch (n_over = counters[kBuildCntOver] read back), which orders their entries in the big arrays
void launch_hnsw_build_backlink_big(int metric, const HnswBuildArgs& a, uint32_t n_over, hipStream_t s);

// step 6's mirror: the upper lists of n_nodes nodes into the resident arrays (HnswPatch without level 0 and delete marks)
struct HnswUpperPatch {
	const uint32_t* ids;
	const uint64_t* upper_at;    // new nodes: first block, assigned by the host; old nodes: ~0 = where they are
	const uint32_t* upper_src;
	const int32_t* levels;
	const uint32_t* src_upper;
	uint64_t* upper_off;
	uint32_t* upper;
	uint32_t M;
};
void launch_hnsw_build_patch_upper(const HnswUpperPatch& p, uint32_t n_nodes, hipStream_t s);

}  // namespace rxgpu
