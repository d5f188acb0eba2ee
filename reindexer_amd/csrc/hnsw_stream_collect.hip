// A streaming HNSW session collected under an allowed-rows bitmap in one launch: the loop of StreamingKnnIndexIterator::Next
// (cpp_src/core/nsselecter/knn_streaming_index_iterator.cc:36-110) with StreamingKnnEstimator::EstimateBatchSize
// (knn_streaming_estimator.h:26-38) — csrc/hnsw_stream_collect_plan.h — around the body of ContinueStreamingSearch
// (hnsw_stream_core.hip.h), on the device next to the heaps.
//
// One workgroup of 64 lanes per session, as in hnsw_stream.hip.  Per call of the loop: mergeExtras, the step loop and emitStreamingBatch
// by the shared body (the batch lands in a scratch: LDS behind the heaps, or the session's output arrays in the global variant), then all
// 64 lanes test the bitmap for the delivered rows and append the accepted ones to the output in delivery order (ballot + popcount) with their position in the call's batch, and
// the counters and the next batch follow from the plan header.  No round trip between the calls; LDS-staged heaps stay staged over the
// whole collection and are written back once, at its end or at a handover.
//
// mode: kCollectFresh = a collection on a begun session; kCollectBegin = the descent and initLayer0SearchState first (the one-shot call:
// descent and collection are one launch); kCollectResume = continued after kStreamNeedGlobal.
//
// A step that would outgrow the LDS heaps (kStreamLdsCand / kStreamLdsExt) stops the launch at that step boundary: the heaps are staged
// out, the loop's state (calls, presented, accepted, the batch of the call that was running) goes into HnswStreamState and the status is
// kStreamNeedGlobal; the host launches the global variant once with resume set — at most two launches per collection.
//
// Every loop is bounded: the step loop by N pops (a node enters candidate_set once), the calls by max_calls (checked here), the emit and
// the compaction by the batch.
#include "hnsw_stream_collect_plan.h"
#include "hnsw_stream_core.hip.h"

namespace rxgpu {

namespace {
constexpr int kCollectLdsEmit = kStreamLdsTop;   // rows one call can deliver while the heaps are in LDS (the batch is at most top_candidates' room)
constexpr size_t kCollectLdsBytes = kStreamLdsBytes + size_t(kCollectLdsEmit) * 8;
}  // namespace

template <int kMetric, bool kLds>
__global__ __launch_bounds__(64) void hnsw_stream_collect_kernel(HnswParams p, HnswStream s, HnswStreamCollect c, int mode) {
	extern __shared__ __attribute__((aligned(16))) unsigned char stream_lds[];
	__shared__ uint32_t nb_id[kHnswMaxNeighbors];
	__shared__ float nb_d[kHnswMaxNeighbors];
	__shared__ uint32_t s_cur;
	__shared__ int s_flag;
	__shared__ int s_n[3];
	__shared__ uint32_t s_emitted, s_exhausted;
	const int lane = threadIdx.x;
	const float* q = s.query;
	HnswStreamState* st = s.state;
	const StreamShared sh{nb_id, nb_d, &s_cur, &s_flag, s_n};
	if (mode == kCollectBegin) {   // the one-shot call: BeginStreamingSearch in front of the collection, in the same launch
		stream_begin<kMetric>(p, s, q, st, sh, lane);
		__syncthreads();
	}
	const bool resume = mode == kCollectResume;
	RX_STREAM_HEAPS(h);
	stream_attach<kLds>(h, s, st, stream_lds, lane);
	// the batch of a call: behind the staged heaps, or the session's output arrays (sized for the largest batch by the host)
	float* em_d = kLds ? reinterpret_cast<float*>(stream_lds + kStreamLdsBytes) : s.out_dist;
	uint32_t* em_r = kLds ? reinterpret_cast<uint32_t*>(stream_lds + kStreamLdsBytes) + kCollectLdsEmit : s.out_row;

	// the loop's state, the same in every lane
	uint32_t calls = resume ? st->calls : 0u, presented = resume ? st->presented : 0u, accepted = resume ? st->accepted : 0u;
	uint32_t batch = resume ? st->batch : c.first_batch;
	bool in_call = resume && st->in_call;
	uint32_t status = kStreamOk, emitted = 0, exhausted_last = resume ? st->exhausted : 0u;

	while (calls < c.max_calls) {
		const int ef = int(s.ef > batch ? s.ef : batch);   // state.ef = max(state.ef, batchSize), hnswalg.h:1960-1961
		if (lane == 0) s_flag = int(in_call ? kStreamOk : stream_merge_extras(h, ef));
		__syncthreads();
		status = uint32_t(s_flag);
		__syncthreads();
		if (status != kStreamOk) break;
		in_call = true;
		if (stream_steps<kMetric, kLds>(p, s, q, h, ef, sh, lane) == 2) {
			status = kStreamNeedGlobal;
			break;
		}
		if (lane == 0) {
			uint32_t exhausted = 0;
			s_emitted = stream_emit(h, batch, em_d, em_r, &exhausted);
			s_exhausted = exhausted;
		}
		__syncthreads();
		in_call = false;
		emitted = s_emitted;
		const bool exhausted = s_exhausted != 0;
		// the delivered rows under the bitmap, accepted ones appended in delivery order
		for (uint32_t base = 0; base < emitted; base += 64) {
			const uint32_t j = base + uint32_t(lane);
			bool ok = false;
			uint32_t row = 0;
			float dist = 0.f;
			if (j < emitted) {
				row = em_r[j];
				dist = em_d[j];
				ok = !c.allowed || ((c.allowed[row >> 5] >> (row & 31)) & 1u);
			}
			const uint64_t m = __ballot(ok);
			const uint32_t at = accepted + uint32_t(__popcll(m & ((1ull << lane) - 1)));
			if (ok && at < c.cap) {
				c.out_dist[at] = dist;
				c.out_row[at] = row;
				c.out_pos[at] = j;
			}
			accepted += uint32_t(__popcll(m));
		}
		presented += emitted;
		if (lane == 0 && calls < c.calls_cap) {
			c.call_batch[calls] = batch;
			c.call_emitted[calls] = emitted;
			c.call_end[calls] = accepted;
		}
		++calls;
		__syncthreads();   // the scratch is read: the next call's emit may overwrite it
		exhausted_last = exhausted ? 1u : 0u;
		if (collect_stop(accepted, c.needed, exhausted, calls, c.max_calls)) break;
		batch = collect_batch(accepted, presented, c.needed);
	}

	if (lane == 0) {
		st->out_count = emitted;
		st->exhausted = exhausted_last;
		st->status = status;
		st->calls = calls;
		st->presented = presented;
		st->accepted = accepted;
		st->batch = batch;
		st->in_call = status == kStreamNeedGlobal ? 1u : 0u;
	}
	stream_detach<kLds>(h, s, st, sh, lane);
}

void launch_hnsw_stream_collect(int metric, const HnswParams& p, const HnswStream& s, const HnswStreamCollect& c, int mode, bool lds, hipStream_t st) {
	const size_t lds_bytes = lds ? kCollectLdsBytes : 0;
#define RX_COLLECT(M, L)                                                                                                             \
	do {                                                                                                                             \
		static std::atomic<uint64_t> raised{0};                                                                                      \
		if (L) (void)raise_dynamic_lds_once(raised, reinterpret_cast<const void*>(&hnsw_stream_collect_kernel<M, L>), lds_bytes);     \
		hipLaunchKernelGGL((hnsw_stream_collect_kernel<M, L>), dim3(1), dim3(64), lds_bytes, st, p, s, c, mode);                      \
	} while (0)
	if (lds) {
		switch (metric) {
			case kL2: RX_COLLECT(kL2, true); break;
			case kIP: RX_COLLECT(kIP, true); break;
			default: RX_COLLECT(kCos, true); break;
		}
	} else {
		switch (metric) {
			case kL2: RX_COLLECT(kL2, false); break;
			case kIP: RX_COLLECT(kIP, false); break;
			default: RX_COLLECT(kCos, false); break;
		}
	}
#undef RX_COLLECT
}

}  // namespace rxgpu
