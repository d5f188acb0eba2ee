// The rule under which a streaming HNSW session is collected under an allowed-rows bitmap, without HIP: StreamingKnnIndexIterator::Next
// (cpp_src/core/nsselecter/knn_streaming_index_iterator.cc:36-110) with StreamingKnnEstimator::EstimateBatchSize
// (knn_streaming_estimator.h:26-38), for a filter that is a bitmap and an index that is not an array.
//
//   calls = presented = accepted = 0;  batch = first_batch
//   repeat:
//       B = ContinueStreamingSearch(session, batch);  calls += 1
//       presented += |B|;  accepted += rows of B whose bit is set
//       stop if accepted >= needed or B.exhausted or calls >= max_calls
//       batch = clamp(size_t(double(presented) / max(1, accepted) * (needed - accepted)), 100, 800)
//
// The loop reads per-batch counts only.  The device loop (hnsw_stream_collect.hip), the Map's host loop (RXGPU_HNSW_COLLECT=host,
// gpu_hnsw_map.cc) and the tests (tests/cpp/hnsw_stream_collect_plan_cpu.cc) all take it from here.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RX_COLLECT_HD __host__ __device__
#else
#define RX_COLLECT_HD
#endif

namespace rxgpu {

constexpr uint32_t kCollectMinBatch = 100;    // StreamingKnnEstimator::kMinEfBatch
constexpr uint32_t kCollectMaxBatch = 800;    // StreamingKnnEstimator::kMaxEfBatch
constexpr uint32_t kCollectMaxCalls = 1000;   // StreamingKnnIndexIterator::kMaxContinueCalls, the default of max_calls

// EstimateBatchSize(accepted, presented, needed).  The product is clamped as a double: above 800 the reference's conversion to size_t
// is followed by the same clamp, and where that conversion would not be defined (a product of 2^64 and more) this stays 800.
RX_COLLECT_HD inline uint32_t collect_batch(uint64_t accepted, uint64_t presented, uint64_t needed) {
	const uint64_t remaining = accepted >= needed ? 1 : needed - accepted;
	const double amplification = double(presented) / double(accepted ? accepted : 1);
	const double value = amplification * double(remaining);
	if (!(value < double(kCollectMaxBatch))) return kCollectMaxBatch;
	const uint64_t v = uint64_t(value);
	return v < kCollectMinBatch ? kCollectMinBatch : uint32_t(v);
}

// behind a call: is it the last one?
RX_COLLECT_HD inline bool collect_stop(uint64_t accepted, uint64_t needed, bool exhausted, uint64_t calls, uint64_t max_calls) {
	return accepted >= needed || exhausted || calls >= max_calls;
}

// the largest batch a collection can ask for
RX_COLLECT_HD inline uint64_t collect_max_batch(uint64_t first_batch) { return first_batch > kCollectMaxBatch ? first_batch : uint64_t(kCollectMaxBatch); }

// Accepted rows a collection can deliver: every call but the last leaves fewer than `needed` accepted, the last adds at most its batch,
// and no node is delivered twice.
RX_COLLECT_HD inline uint64_t collect_out_bound(uint64_t count, uint64_t needed, uint64_t first_batch) {
	if (needed == 0 || first_batch == 0) return 0;
	const uint64_t mb = collect_max_batch(first_batch);
	const uint64_t room = needed - 1 > ~uint64_t(0) - mb ? ~uint64_t(0) : needed - 1 + mb;
	return count < room ? count : room;
}

// Calls a collection can make: a call that delivers nothing reports the session exhausted (an empty top_candidates behind the step loop
// means an empty candidate_set and empty extras), so every call but the last delivers a node of its own.
RX_COLLECT_HD inline uint64_t collect_calls_bound(uint64_t count, uint64_t needed, uint64_t first_batch, uint64_t max_calls) {
	if (needed == 0 || first_batch == 0) return 0;
	const uint64_t by_rows = count + 1;
	return max_calls < by_rows ? max_calls : by_rows;
}

}  // namespace rxgpu
