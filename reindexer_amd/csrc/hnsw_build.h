// What the kernels of the batched build (hnsw_build.hip; level 1: hnsw_build_upper.hip) take: one batch of new rows [first, first + n) of an
// index whose nodes < first are linked.  Layout and sizes of the scratch: hnsw_build_plan.h (HnswBuildScratch).
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
	uint32_t first, n;          // the batch: its candidates are nodes < first, it has n rows
	const uint32_t* row_ids;    // [n] the rows of the batch, ascending (level 1: the batch's rows of level >= 1); null: row r is first + r
	uint32_t id_end;            // every id a list may name is below this: first + n for a contiguous batch
	const uint32_t* cand_row;   // [n][k] what the search found for row r (kInvalidRow past its count)
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
	uint32_t skip;               // levels of a node in front of the first staged one: 0, or 1 where level 1 was built on the device
};
void launch_hnsw_build_patch_upper(const HnswUpperPatch& p, uint32_t n_nodes, hipStream_t s);

// Level 1 of a batch (hnsw_build_upper.hip): the level-1 lists as a dense array view [..][1 + M], on which the kernels above run with
// links0 = view and maxM0 = M.
struct HnswUpperView {
	uint32_t* view;              // [..][1 + M]
	const uint64_t* upper_off;   // first block of a node; a node's blocks end where the next node's begin
	uint32_t* upper;             // [blocks][1 + M]
	uint64_t upper_used;         // blocks in use: where the blocks of node `nodes - 1` end
	uint32_t nodes;              // the nodes the blocks of which exist
	uint32_t M;
};
// view row i = the level-1 block of node i, or an empty list where it has none, for every i < nodes
void launch_hnsw_upper_view_gather(const HnswUpperView& v, hipStream_t s);
// the view rows of the touched nodes (touched [counters[kBuildCntTouched]], all < nodes) back into their level-1 blocks
void launch_hnsw_upper_view_store(const HnswUpperView& v, const uint32_t* touched, const uint32_t* counters, uint32_t max_touched, hipStream_t s);
// the view rows of ids [n] (nodes whose blocks exist by now) into their level-1 blocks
void launch_hnsw_upper_view_store_ids(const HnswUpperView& v, const uint32_t* ids, uint32_t n, hipStream_t s);
// out [n][dim] = rows[ids[r]][0 .. dim): the stored rows of a batch's level >= 1 nodes packed as queries
void launch_hnsw_upper_pack_rows(const float* rows, uint32_t stride, uint32_t dim, const uint32_t* ids, uint32_t n, float* out, hipStream_t s);

}  // namespace rxgpu
