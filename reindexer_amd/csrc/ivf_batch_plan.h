// The decisions of a batched IVF-Flat list search (rxgpu_search_knn_lists_batch, knn_lists.hip) that need no device, without HIP:
//   * the envelope: which calls the device train answers and which go query by query through rxgpu_search_knn_lists,
//   * how the queries of a call are cut into trains against a scratch budget,
//   * gridx, the workgroups per query of knn_scan_lists, from what the host knows without asking the device,
//   * the rule that maps a virtual 64-entry chunk of a query's concatenated probed lists to (probe slot, offset inside the list),
//   * where everything lies in the one scratch buffer of a train.
// Arithmetic on counts only: tests/test_ivf_batch_plan.py pins it on the CPU (tests/cpp/ivf_batch_plan_cpu.cc); the kernels and the launcher
// call the same inline functions, so the layout the host sizes is the layout the device walks.
//
// Which shapes take the train by default: every shape inside the envelope.  profiles/ivf_batch_ab.json (tools/bench_ivf.py --batch-ab) holds
// the A/B against the four host threads at 1M x 768, nlist 1024: 256 and 4096 queries at nprobe 1 / 16 / 64, the train faster in all six
// (2.3x at nprobe 64 to 18x at nprobe 1), so ivf_batch_default_on_device below keeps no shape on the old path; a shape measured slower gets
// its rule there.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RX_IVFB_HD __host__ __device__
#else
#define RX_IVFB_HD
#endif

namespace rxgpu {

// ---- the envelope.  The coarse search leaves up to 128 list ids per query in HBM (kMaxFusedK2, the widest fused top list), and the scan keeps
// up to 128 entries per wavefront (WaveTopK2).  nprobe is the clamped value: 1 <= nprobe <= nlist.
constexpr uint32_t kIvfBatchMaxProbe = 128;
constexpr uint32_t kIvfBatchMaxKk = 128;
RX_IVFB_HD inline bool ivf_batch_on_device(uint32_t nprobe, uint32_t kk) { return nprobe >= 1 && nprobe <= kIvfBatchMaxProbe && kk >= 1 && kk <= kIvfBatchMaxKk; }
// which list type the scan runs with: one entry per lane up to 64, two above
RX_IVFB_HD inline bool ivf_batch_wide_list(uint32_t kk) { return kk > 64; }
// The default inside the envelope (the engine's SearchBatch asks; RXGPU_IVF_BATCH=threads overrides it): the train, for every shape.
RX_IVFB_HD inline bool ivf_batch_default_on_device(uint32_t nq, uint32_t nprobe, uint32_t kk) { return nq >= 2 && ivf_batch_on_device(nprobe, kk); }

// ---- chunks: a list of L rows is ceil(L / 64) chunks of 64 consecutive entries, a chunk never spans two lists
constexpr uint32_t kIvfBatchChunk = 64;
RX_IVFB_HD inline uint32_t ivf_batch_list_chunks(uint64_t rows) { return uint32_t((rows + kIvfBatchChunk - 1) / kIvfBatchChunk); }
struct IvfBatchChunkAt {
	uint32_t slot;     // probe slot (position of the list in the query's coarse result)
	uint32_t offset;   // first entry of the chunk inside that list
};
// cum [nprobe + 1]: cum[s] = chunks of the probe slots in front of s (cum[0] = 0, cum[nprobe] = the query's chunks).  chunk < cum[nprobe].
// The slot is the LAST one whose running count is <= chunk: slots of empty lists (equal neighbours) are stepped over.
RX_IVFB_HD inline IvfBatchChunkAt ivf_batch_chunk_at(const uint32_t* cum, uint32_t nprobe, uint32_t chunk) {
	uint32_t lo = 0, hi = nprobe;
	while (hi - lo > 1) {
		const uint32_t mid = (lo + hi) >> 1;
		if (cum[mid] <= chunk) {
			lo = mid;
		} else {
			hi = mid;
		}
	}
	return IvfBatchChunkAt{lo, (chunk - cum[lo]) * kIvfBatchChunk};
}

// ---- gridx: workgroups (of four wavefronts) per query.  The host knows nprobe, nlist, the rows listed and the longest list, not which lists a
// query probes.  A query is expected to hold nprobe average lists; it never holds more chunks than nprobe longest lists, nor more than every
// listed row in as many lists.  A workgroup should find kIvfBatchChunksPerWave chunks per wavefront where the batch alone fills the machine
// (nq >= 2 workgroups per CU); a small batch spreads each query over more workgroups, down to one chunk per wavefront.
constexpr uint32_t kIvfBatchWaves = 4;
constexpr uint32_t kIvfBatchChunksPerWave = 8;
constexpr uint32_t kIvfBatchWgPerCu = 2;
constexpr uint32_t kIvfBatchMaxGridX = 256;
RX_IVFB_HD inline uint32_t ivf_batch_grid_x(uint32_t nq, uint32_t nprobe, uint32_t nlist, uint64_t rows_listed, uint64_t longest_list, uint32_t cus) {
	if (nq == 0 || nlist == 0) return 1;
	const uint64_t avg_rows = (rows_listed + nlist - 1) / nlist;
	const uint64_t expect = uint64_t(nprobe) * ivf_batch_list_chunks(avg_rows);
	uint64_t most = uint64_t(nprobe) * ivf_batch_list_chunks(longest_list);
	const uint64_t all = ivf_batch_list_chunks(rows_listed) + nprobe;
	if (most > all) most = all;
	const uint64_t by_work = (expect + uint64_t(kIvfBatchWaves) * kIvfBatchChunksPerWave - 1) / (uint64_t(kIvfBatchWaves) * kIvfBatchChunksPerWave);
	const uint64_t fill = (uint64_t(cus ? cus : 1) * kIvfBatchWgPerCu + nq - 1) / nq;
	uint64_t g = by_work > fill ? by_work : fill;
	const uint64_t one_each = (most + kIvfBatchWaves - 1) / kIvfBatchWaves;   // more workgroups than this find no chunk for any query
	if (g > one_each) g = one_each;
	if (g > kIvfBatchMaxGridX) g = kIvfBatchMaxGridX;
	return uint32_t(g ? g : 1);
}

// ---- the scratch of one train, one allocation: every part starts on a 256-byte boundary.  The partial lists [q][gridx][kk] and the result
// [q][kk] lie in the search context's part and out buffers; their bytes count against the budget all the same.
struct IvfBatchScratch {
	uint64_t o_probe;      // u32 [q][nprobe]       the coarse search's list ids
	uint64_t o_pdist;      // f32 [q][nprobe]       ... and distances (unused behind it)
	uint64_t o_pcnt;       // u32 [q]               lists found per query
	uint64_t o_cum;        // u32 [q][nprobe + 1]   running chunk counts
	uint64_t o_scanned;    // u64 [q]               rows in the probed lists
	uint64_t bytes;
};
RX_IVFB_HD inline uint64_t ivf_batch_align256(uint64_t v) { return (v + 255) & ~uint64_t(255); }
RX_IVFB_HD inline IvfBatchScratch ivf_batch_scratch(uint64_t q, uint32_t nprobe) {
	IvfBatchScratch s{};
	s.o_probe = 0;
	s.o_pdist = ivf_batch_align256(s.o_probe + q * nprobe * 4);
	s.o_pcnt = ivf_batch_align256(s.o_pdist + q * nprobe * 4);
	s.o_cum = ivf_batch_align256(s.o_pcnt + q * 4);
	s.o_scanned = ivf_batch_align256(s.o_cum + q * (uint64_t(nprobe) + 1) * 4);
	s.bytes = ivf_batch_align256(s.o_scanned + q * 8);
	return s;
}

// ---- trains: the queries of a call in chunks whose device buffers stay within a budget (RXGPU_IVF_BATCH_SCRATCH_BYTES, read per call)
constexpr uint64_t kIvfBatchScratchBytes = 256ull << 20;
constexpr uint32_t kIvfBatchMaxTrainQueries = 32768;   // grid.y of the scan
// what one query takes: its vector, its partial lists, its result, its share of the scratch above
RX_IVFB_HD inline uint64_t ivf_batch_query_bytes(uint32_t dim, uint32_t nprobe, uint32_t kk, uint32_t gridx) {
	return uint64_t(dim) * 4 + uint64_t(gridx) * kk * 8 + uint64_t(kk) * 8 + 4 + uint64_t(nprobe) * 8 + 4 + (uint64_t(nprobe) + 1) * 4 + 8;
}
// queries per train: as many as the budget holds, one at least (a budget below one query is exceeded by that one query), never more than nq
RX_IVFB_HD inline uint32_t ivf_batch_train_queries(uint32_t nq, uint32_t dim, uint32_t nprobe, uint32_t kk, uint32_t gridx, uint64_t budget_bytes) {
	uint64_t q = budget_bytes / ivf_batch_query_bytes(dim, nprobe, kk, gridx);
	if (q < 1) q = 1;
	if (q > kIvfBatchMaxTrainQueries) q = kIvfBatchMaxTrainQueries;
	return q < nq ? uint32_t(q) : nq;
}
RX_IVFB_HD inline uint32_t ivf_batch_trains(uint32_t nq, uint32_t train_queries) { return train_queries ? (nq + train_queries - 1) / train_queries : 0; }

}  // namespace rxgpu
