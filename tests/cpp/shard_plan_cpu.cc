// The decisions of a row-range sharded index (reindexer_amd/csrc/shard_plan.h) compiled for the host: tests/test_shard_plan.py pins its rules
// on the CPU, tests/test_gpu_sharded_routes.py holds the device path's layout against it.  Test infrastructure only — nothing in the product links this.
#include <cstdint>
#include <cstring>
#include <vector>

#include "shard_plan.h"

extern "C" {

uint64_t shard_plan_rows(uint64_t capacity, uint32_t n_shards) { return rxgpu::shard_rows_for(capacity, n_shards); }
uint64_t shard_plan_local_count(uint64_t shard_rows, uint32_t s, uint64_t count) { return rxgpu::ShardCut{shard_rows}.local_count(s, count); }
// out = {shard, local row}
void shard_plan_locate(uint64_t shard_rows, uint64_t row, uint64_t* out) {
	const rxgpu::ShardCut cut{shard_rows};
	out[0] = cut.shard_of(row);
	out[1] = cut.local(row);
}
// ab = {a, b}; returns 1 when the range touches the shard
int shard_plan_piece(uint64_t shard_rows, uint32_t s, uint64_t first, uint64_t n, uint64_t* ab) { return rxgpu::ShardCut{shard_rows}.piece(s, first, n, ab[0], ab[1]) ? 1 : 0; }
// returns 1 + *total, or 0: not a prefix
int shard_plan_prefix(const uint64_t* counts, uint32_t n_shards, uint64_t shard_rows, uint64_t* total) { return rxgpu::shard_prefix_total(counts, n_shards, shard_rows, *total) ? 1 : 0; }

// head = {nranks, slots}; rank_dev [n] at most, shard_rank / shard_slot / pos [n], base [nranks * slots] (n * n at most)
void shard_plan_layout(const int* devices, uint32_t n, uint64_t shard_rows, uint32_t invalid_row, uint32_t* head, int* rank_dev, uint32_t* shard_rank, uint32_t* shard_slot,
					   uint32_t* pos, uint32_t* base) {
	const rxgpu::RankLayout l = rxgpu::rank_layout(devices, n, shard_rows, invalid_row);
	head[0] = l.nranks;
	head[1] = l.slots;
	std::memcpy(rank_dev, l.rank_dev.data(), l.rank_dev.size() * sizeof(int));
	std::memcpy(shard_rank, l.shard_rank.data(), l.shard_rank.size() * 4);
	std::memcpy(shard_slot, l.shard_slot.data(), l.shard_slot.size() * 4);
	std::memcpy(pos, l.pos.data(), l.pos.size() * 4);
	std::memcpy(base, l.base.data(), l.base.size() * 4);
}

// Returns the rule (0 ok, 1 not increasing, 2 out of range), *at = the first offending index.  ok: sizes [n_shards]; local / where [n_ids]
// hold the shards' lists back to back (where: the unordered form only, else untouched).
int shard_plan_split(const uint32_t* ids, uint64_t n_ids, uint64_t count, uint64_t shard_rows, uint32_t n_shards, int ordered, uint64_t* at, uint64_t* sizes, uint32_t* local,
					 uint32_t* where) {
	const rxgpu::RowSplit sp = rxgpu::split_row_list(ids, n_ids, count, shard_rows, n_shards, ordered != 0);
	*at = sp.at;
	if (sp.rule != rxgpu::kRowListOk) return sp.rule;
	for (uint32_t s = 0; s < n_shards; ++s) {
		sizes[s] = sp.local[s].size();
		std::memcpy(local, sp.local[s].data(), sp.local[s].size() * 4);
		local += sp.local[s].size();
		if (!ordered) {
			std::memcpy(where, sp.where[s].data(), sp.where[s].size() * 4);
			where += sp.where[s].size();
		}
	}
	return 0;
}
int shard_plan_check_rows(const uint32_t* ids, uint64_t n_ids, uint64_t count, int ordered, uint64_t* at) { return rxgpu::check_row_list(ids, n_ids, count, ordered != 0, at); }

// out = {qbytes, list_words, local_bytes, gathered_bytes, out_bytes, o_dist, o_row, o_count, pinned_knn, pinned_hnsw}
void shard_plan_exchange_shape(uint32_t nq, uint32_t kk, uint32_t nranks, uint32_t slots, uint32_t dim, uint64_t* out) {
	const rxgpu::ExchangeShape e = rxgpu::exchange_shape(nq, kk, nranks, slots, dim);
	const uint64_t v[10] = {e.qbytes, e.list_words, e.local_bytes, e.gathered_bytes, e.out_bytes, e.o_dist, e.o_row, e.o_count, e.pinned_knn(), e.pinned_hnsw()};
	std::memcpy(out, v, sizeof(v));
}
// out = {brute force takes the exchange, HNSW takes it, hole}
void shard_plan_routes(const int* devices, uint32_t n_shards, const uint64_t* counts, int has_exchange, int has_row_list, uint32_t kk, uint32_t max_fused_k, int* out) {
	out[0] = rxgpu::knn_takes_exchange(has_exchange != 0, has_row_list != 0, kk, max_fused_k, counts, n_shards);
	out[1] = rxgpu::hnsw_takes_exchange(has_exchange != 0, kk, max_fused_k);
	out[2] = rxgpu::exchange_hole(rxgpu::rank_layout(devices, n_shards), counts, n_shards);
}

int shard_plan_less(float da, uint32_t ra, float db, uint32_t rb) { return rxgpu::dist_row_less({da, ra}, {db, rb}) ? 1 : 0; }

// shard s: dist / row at [off[s], ...) of the flat arrays, count [s][nq], stride[s]
void shard_plan_merge_topk(uint32_t n_shards, const float* dist, const uint32_t* row, const uint64_t* off, const uint32_t* count, const uint64_t* stride, uint64_t shard_rows,
						   uint32_t nq, uint32_t k, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	std::vector<const float*> pd(n_shards);
	std::vector<const uint32_t*> pr(n_shards), pc(n_shards);
	std::vector<size_t> st(n_shards);
	for (uint32_t s = 0; s < n_shards; ++s) {
		pd[s] = dist + off[s];
		pr[s] = row + off[s];
		pc[s] = count + size_t(s) * nq;
		st[s] = size_t(stride[s]);
	}
	rxgpu::merge_shard_topk(rxgpu::ShardLists{pd.data(), pr.data(), pc.data(), st.data()}, n_shards, shard_rows, nq, k, out_dist, out_row, out_count);
}
// shard s: total[s] hits at [off[s], ...); concat != 0: shard after shard, else sorted.  Returns the number of hits.
uint64_t shard_plan_merge_ranges(uint32_t n_shards, const float* dist, const uint32_t* row, const uint64_t* off, const uint64_t* total, uint64_t shard_rows, uint64_t cap,
								 int concat, float* out_dist, uint32_t* out_row) {
	std::vector<const float*> pd(n_shards);
	std::vector<const uint32_t*> pr(n_shards);
	for (uint32_t s = 0; s < n_shards; ++s) {
		pd[s] = dist + off[s];
		pr[s] = row + off[s];
	}
	return (concat ? rxgpu::concat_shard_ranges : rxgpu::merge_shard_ranges)(pd.data(), pr.data(), total, n_shards, shard_rows, cap, out_dist, out_row);
}

uint64_t shard_plan_range_want(int hnsw, uint64_t cap, uint64_t want, uint64_t reported) {
	return hnsw ? rxgpu::hnsw_range_want(cap, want, reported) : rxgpu::range_want(cap, want, reported);
}
int shard_plan_range_attempts(int hnsw) { return hnsw ? rxgpu::kHnswRangeAttempts : rxgpu::kRangeAttempts; }

}  // extern "C"
