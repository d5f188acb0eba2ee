// HNSW streaming (batched) KNN on gfx950: BeginStreamingSearch / ContinueStreamingSearch
// (cpp_src/core/index/float_vector/hnswlib/hnswalg.h:1865-1975) with the streaming branches of initLayer0SearchState (:846-850),
// layer0ShouldStopBeforePop (:865-868), runLayer0Step (:882-893, 939-940), mergeExtrasIntoTopCandidates (:1893-1926) and
// emitStreamingBatch (:1928-1945).
//
// A session is a resumable best-first enumeration: every evaluated node goes into candidate_set, nodes enter top_candidates when
// they are POPPED, nodes pushed out of a full top_candidates are parked in top_candidates_extras, and each Continue(batch) runs
// with ef = max(ef, batch), then hands out the `batch` best of top_candidates.  One wavefront drives one session; the three
// heaps (PriorityQueue + CompareByFirst, replayed with the reference's sift mechanics so ties break identically) persist in the
// session's device memory between calls.  While they fit they are staged in LDS for the duration of a call (heap updates are
// dependent single-lane accesses: ~100 ns in LDS against ~1 us in HBM); a call that would outgrow LDS stops at a step boundary
// with status kStreamNeedGlobal and is resumed by the all-global variant — never on the CPU.
#include "hnsw_stream_core.hip.h"

namespace rxgpu {

// mode: kStreamBegin = descent + initLayer0SearchState; kStreamContinue = one ContinueStreamingSearch; kStreamResume = the same call
// continued after kStreamNeedGlobal (no second mergeExtras).  kLds: heaps staged in LDS for this call.
template <int kMetric, bool kLds>
__global__ __launch_bounds__(64) void hnsw_stream_kernel(HnswParams p, HnswStream s, uint32_t batch, int mode) {
	extern __shared__ __attribute__((aligned(16))) unsigned char stream_lds[];
	__shared__ uint32_t nb_id[kHnswMaxNeighbors];
	__shared__ float nb_d[kHnswMaxNeighbors];
	__shared__ uint32_t s_cur;
	__shared__ int s_flag;
	__shared__ int s_n[3];
	const int lane = threadIdx.x;
	const float* q = s.query;
	HnswStreamState* st = s.state;

	const StreamShared sh{nb_id, nb_d, &s_cur, &s_flag, s_n};
	if (mode == kStreamBegin) {   // getLayer0EntryPoint + initLayer0SearchState, streaming
		stream_begin<kMetric>(p, s, q, st, sh, lane);
		return;
	}

	// ---- heaps: LDS staging or the session's global arrays
	RX_STREAM_HEAPS(h);
	stream_attach<kLds>(h, s, st, stream_lds, lane);
	const int ef = int(s.ef > batch ? s.ef : batch);   // state.ef = max(state.ef, batchSize), hnswalg.h:1960-1961
	uint32_t status = kStreamOk;

	if (mode == kStreamContinue && lane == 0) status = stream_merge_extras(h, ef);
	if (lane == 0) s_flag = int(status);
	__syncthreads();
	status = uint32_t(s_flag);
	__syncthreads();

	bool finished = false;
	if (status == kStreamOk) {
		const int flag = stream_steps<kMetric, kLds>(p, s, q, h, ef, sh, lane);
		finished = flag == 1;
		if (flag == 2) status = kStreamNeedGlobal;
	}

	if (lane == 0) {
		uint32_t emitted = 0;
		if (finished) {
			uint32_t exhausted = 0;
			emitted = stream_emit(h, batch, s.out_dist, s.out_row, &exhausted);
			st->exhausted = exhausted;
		}
		st->out_count = emitted;
		st->status = status;
	}
	stream_detach<kLds>(h, s, st, sh, lane);
}

void launch_hnsw_stream(int metric, const HnswParams& p, const HnswStream& s, uint32_t batch, int mode, bool lds, hipStream_t st) {
	const size_t lds_bytes = lds ? kStreamLdsBytes : 0;
#define RX_STREAM(M, L)                                                                                                      \
	do {                                                                                                                     \
		static std::atomic<uint64_t> raised{0};                                                                              \
		if (L) (void)raise_dynamic_lds_once(raised, reinterpret_cast<const void*>(&hnsw_stream_kernel<M, L>), lds_bytes);     \
		hipLaunchKernelGGL((hnsw_stream_kernel<M, L>), dim3(1), dim3(64), lds_bytes, st, p, s, batch, mode);                  \
	} while (0)
	if (lds) {
		switch (metric) {
			case kL2: RX_STREAM(kL2, true); break;
			case kIP: RX_STREAM(kIP, true); break;
			default: RX_STREAM(kCos, true); break;
		}
	} else {
		switch (metric) {
			case kL2: RX_STREAM(kL2, false); break;
			case kIP: RX_STREAM(kIP, false); break;
			default: RX_STREAM(kCos, false); break;
		}
	}
#undef RX_STREAM
}

}  // namespace rxgpu
