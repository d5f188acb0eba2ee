// The decisions of a row-range sharded index (rxgpu_sharded.hip; the rank layout also serves rxgpu_ft_sharded.hip), without HIP: how the rows
// are cut, which RCCL rank and slot a shard takes, how a row list splits at the shard boundaries, how large the exchange's buffers are and
// which calls go through it, how the per-shard answers merge under (dist, global row), and how a range fan-out grows its buffers.  Arithmetic
// on counts and lists only, so tests/test_shard_plan.py pins it on the CPU (tests/cpp/shard_plan_cpu.cc) for layouts no one-GPU box ever
// sees.  Constants that live in HIP headers (kInvalidRow, kMaxFusedK) come in as arguments.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace rxgpu {

// ---- the row cut: shard s holds the global rows [s * shard_rows, (s + 1) * shard_rows)
inline uint64_t shard_rows_for(uint64_t capacity, uint32_t n_shards) {
	return ((capacity + n_shards - 1) / n_shards + 31) & ~uint64_t(31);   // whole bitmap words per shard
}
struct ShardCut {
	uint64_t shard_rows = 0;
	size_t shard_of(uint64_t row) const { return size_t(row / shard_rows); }
	uint64_t base(size_t s) const { return uint64_t(s) * shard_rows; }
	uint64_t local(uint64_t row) const { return row - base(shard_of(row)); }
	// rows of shard s when the whole index holds `count` (with count = capacity: the shard's capacity, 0 past the end)
	uint64_t local_count(size_t s, uint64_t count) const { return count > base(s) ? std::min<uint64_t>(count - base(s), shard_rows) : 0; }
	// the part [a, b) of the global rows [first, first + n) that falls into shard s; false: none
	bool piece(size_t s, uint64_t first, uint64_t n, uint64_t& a, uint64_t& b) const {
		a = std::max(first, base(s));
		b = std::min(first + n, base(s) + shard_rows);
		return a < b;
	}
};
// Shards filled directly must hold a prefix of the global rows: full shards, then at most one partial, then empty ones.  false: they do not.
inline bool shard_prefix_total(const uint64_t* counts, size_t n_shards, uint64_t shard_rows, uint64_t& total) {
	total = 0;
	bool ended = false;
	for (size_t s = 0; s < n_shards; ++s) {
		if (counts[s] > shard_rows || (ended && counts[s])) return false;
		ended = ended || counts[s] < shard_rows;
		total += counts[s];
	}
	return true;
}

// ---- the exchange's ranks: one per DISTINCT device, in first-seen order; a device that holds several shards sends them as `slots`
// consecutive pieces, devices with fewer shards pad.  pos[s] = where shard s lies in a gathered buffer; base[p] = the global row base of
// the shard at gathered position p, invalid_row at padded positions (the merge kernel skips those).
struct RankLayout {
	uint32_t nranks = 0, slots = 0;
	std::vector<int> rank_dev;
	std::vector<uint32_t> shard_rank, shard_slot, pos, base;
	size_t positions() const { return size_t(nranks) * slots; }
};
inline RankLayout rank_layout(const int* devices, uint32_t n_shards, uint64_t shard_rows = 0, uint32_t invalid_row = 0xFFFFFFFFu) {
	RankLayout l;
	std::vector<uint32_t> per_rank;
	for (uint32_t s = 0; s < n_shards; ++s) {
		uint32_t r = 0;
		while (r < l.rank_dev.size() && l.rank_dev[r] != devices[s]) ++r;
		if (r == l.rank_dev.size()) {
			l.rank_dev.push_back(devices[s]);
			per_rank.push_back(0);
		}
		l.shard_rank.push_back(r);
		l.shard_slot.push_back(per_rank[r]++);
	}
	l.nranks = uint32_t(l.rank_dev.size());
	l.slots = n_shards ? *std::max_element(per_rank.begin(), per_rank.end()) : 0;
	l.base.assign(l.positions(), invalid_row);
	for (uint32_t s = 0; s < n_shards; ++s) {
		l.pos.push_back(l.shard_rank[s] * l.slots + l.shard_slot[s]);
		l.base[l.pos[s]] = uint32_t(s * shard_rows);
	}
	return l;
}

// ---- a list of global rows split at the shard boundaries: local[s] = the rows of shard s minus its base, in list order.  ordered: the
// list must ascend strictly (the pre-filtered searches); else any order with repeats (rxgpu_distances), and where[s][j] = the list position
// local[s][j] came from.  rule != kRowListOk: ids[at] is the first entry that broke it (the caller words the message).
enum RowListRule : int { kRowListOk = 0, kRowListNotIncreasing = 1, kRowListOutOfRange = 2 };
inline RowListRule row_list_rule(const uint32_t* ids, uint64_t i, uint64_t count, bool ordered) {
	if (ordered && i && ids[i] <= ids[i - 1]) return kRowListNotIncreasing;
	return ids[i] >= count ? kRowListOutOfRange : kRowListOk;
}
inline RowListRule check_row_list(const uint32_t* ids, uint64_t n_ids, uint64_t count, bool ordered, uint64_t* at = nullptr) {
	for (uint64_t i = 0; i < n_ids; ++i) {
		if (const RowListRule r = row_list_rule(ids, i, count, ordered); r != kRowListOk) {
			if (at) *at = i;
			return r;
		}
	}
	return kRowListOk;
}
struct RowSplit {
	RowListRule rule = kRowListOk;
	uint64_t at = 0;
	std::vector<std::vector<uint32_t>> local, where;
};
inline RowSplit split_row_list(const uint32_t* ids, uint64_t n_ids, uint64_t count, uint64_t shard_rows, size_t n_shards, bool ordered) {
	RowSplit sp;
	sp.local.resize(n_shards);
	sp.where.resize(n_shards);
	const ShardCut cut{shard_rows};
	for (uint64_t i = 0; i < n_ids; ++i) {
		if ((sp.rule = row_list_rule(ids, i, count, ordered)) != kRowListOk) {
			sp.at = i;
			return sp;
		}
		const size_t s = cut.shard_of(ids[i]);
		sp.local[s].push_back(uint32_t(ids[i] - cut.base(s)));
		if (!ordered) sp.where[s].push_back(uint32_t(i));
	}
	return sp;
}

// ---- one exchange of nq x kk lists.  A shard's piece is [nq][kk] distance bits | [nq][kk] rows (list_words 32-bit words); rank 0's d_out
// and the pinned buffer hold [nq][kk] distances | [nq][kk] global rows | [nq] counts at the word offsets o_dist / o_row / o_count.
struct ExchangeShape {
	size_t qbytes = 0, list_words = 0, local_bytes = 0, gathered_bytes = 0, out_bytes = 0;
	size_t o_dist = 0, o_row = 0, o_count = 0;
	size_t pinned_knn() const { return std::max(qbytes, out_bytes); }   // the queries on the way in, the merged lists on the way out
	size_t pinned_hnsw() const { return out_bytes; }                    // the shards' searches upload their queries themselves
};
inline ExchangeShape exchange_shape(uint32_t nq, uint32_t kk, uint32_t nranks, uint32_t slots, uint32_t dim) {
	ExchangeShape e;
	e.qbytes = size_t(nq) * dim * sizeof(float);
	e.list_words = size_t(2) * nq * kk;
	e.local_bytes = e.list_words * slots * sizeof(uint32_t);
	e.gathered_bytes = e.local_bytes * nranks;
	e.o_row = size_t(nq) * kk;
	e.o_count = size_t(2) * nq * kk;
	e.out_bytes = (e.o_count + nq) * sizeof(uint32_t);
	return e;
}
// Brute force goes through the exchange iff there is one, the call has no row list, the lists fit the fused scan and every shard holds
// 0 or >= kk rows (a shard with fewer rows than kk returns a shorter list: the host path pads it).
inline bool knn_takes_exchange(bool has_exchange, bool has_row_list, uint32_t kk, uint32_t max_fused_k, const uint64_t* counts, size_t n_shards) {
	if (!has_exchange || has_row_list || kk > max_fused_k) return false;
	for (size_t s = 0; s < n_shards; ++s) {
		if (counts[s] != 0 && counts[s] < kk) return false;
	}
	return true;
}
inline bool hnsw_takes_exchange(bool has_exchange, uint32_t k, uint32_t max_fused_k) { return has_exchange && k <= max_fused_k; }
// Some piece of the send buffers gets no list: padded positions are skipped by their base, EMPTY shards need invalid lists (the 0xFF fill).
inline bool exchange_hole(const RankLayout& l, const uint64_t* counts, size_t n_shards) {
	bool hole = l.positions() != n_shards;
	for (size_t s = 0; s < n_shards; ++s) hole = hole || counts[s] == 0;
	return hole;
}

// ---- host merges under (dist, GLOBAL row), global row = s * shard_rows + local row: the single-device order
// a strict weak order even when a distance is NaN (NaN sorts last; +0 and -0 are one distance)
inline bool dist_row_less(const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) {
	const bool an = a.first != a.first, bn = b.first != b.first;
	if (an != bn) return bn;
	if (!an && a.first != b.first) return a.first < b.first;
	return a.second < b.second;
}
// The per-shard lists of one fan-out: shard s wrote count[s][q] entries of query q at dist[s] / row[s] + q * stride[s].
struct ShardLists {
	const float* const* dist;
	const uint32_t* const* row;
	const uint32_t* const* count;
	const size_t* stride;
};
// The k best of the union, per query, into [nq][k] arrays; out_count[q] = entries written.
inline void merge_shard_topk(const ShardLists& in, size_t n_shards, uint64_t shard_rows, uint32_t nq, uint32_t k, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	std::vector<std::pair<float, uint32_t>> all;
	for (uint32_t q = 0; q < nq; ++q) {
		all.clear();
		for (size_t s = 0; s < n_shards; ++s) {
			const size_t o = size_t(q) * in.stride[s];
			for (uint32_t j = 0; j < in.count[s][q]; ++j) all.emplace_back(in.dist[s][o + j], uint32_t(in.row[s][o + j] + s * shard_rows));
		}
		const size_t take = std::min<size_t>(k, all.size());
		std::partial_sort(all.begin(), all.begin() + take, all.end(), dist_row_less);
		for (size_t j = 0; j < take; ++j) {
			out_dist[size_t(q) * k + j] = all[j].first;
			out_row[size_t(q) * k + j] = all[j].second;
		}
		out_count[q] = uint32_t(take);
	}
}
// Range hits of every shard (total[s] entries each), sorted / shard after shard as they came: returns the number of hits and writes the
// first min(hits, cap) of them.
inline uint64_t merge_shard_ranges(const float* const* dist, const uint32_t* const* row, const uint64_t* total, size_t n_shards, uint64_t shard_rows, uint64_t cap,
								   float* out_dist, uint32_t* out_row) {
	std::vector<std::pair<float, uint32_t>> all;
	for (size_t s = 0; s < n_shards; ++s) {
		for (uint64_t j = 0; j < total[s]; ++j) all.emplace_back(dist[s][j], uint32_t(row[s][j] + s * shard_rows));
	}
	std::sort(all.begin(), all.end(), dist_row_less);
	for (size_t j = 0; j < all.size() && j < cap; ++j) {
		out_dist[j] = all[j].first;
		out_row[j] = all[j].second;
	}
	return all.size();
}
inline uint64_t concat_shard_ranges(const float* const* dist, const uint32_t* const* row, const uint64_t* total, size_t n_shards, uint64_t shard_rows, uint64_t cap,
									float* out_dist, uint32_t* out_row) {
	uint64_t n = 0;
	for (size_t s = 0; s < n_shards; ++s) {
		for (uint64_t j = 0; j < total[s]; ++j, ++n) {
			if (n < cap) {
				out_dist[n] = dist[s][j];
				out_row[n] = uint32_t(row[s][j] + s * shard_rows);
			}
		}
	}
	return n;
}

// ---- the buffer a shard's range search is given: `want` of the attempt before (0: this is the first) and the hits that attempt reported.
// Brute force reports the exact number, so the second attempt fits; an HNSW overflow reports a lower bound: grow until the closure fits.
constexpr int kRangeAttempts = 2, kHnswRangeAttempts = 8;
inline uint64_t range_want(uint64_t cap, uint64_t want, uint64_t reported) { return want ? reported : std::max<uint64_t>(cap, 64); }
inline uint64_t hnsw_range_want(uint64_t cap, uint64_t want, uint64_t reported) { return want ? std::max<uint64_t>(want * 4, reported * 2) : std::max<uint64_t>(cap, 256); }

}  // namespace rxgpu
