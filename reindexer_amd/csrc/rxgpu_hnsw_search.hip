// C-ABI implementation (include/rxgpu.h), the HNSW host side: SearchKnn — plain, posted, over SQ8 codes, under an allowed-rows bitmap, into a
// sink — and the search counters.  What a search launches is decided in hnsw_launch_plan.h, what runs again behind the first pass in
// hnsw_rerun_plan.h (no HIP, tested on the CPU), and carried out here; the resident kernel behind single queries is rxgpu_hnsw_server.hip.
// Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/rxgpu.h"
#include "hnsw_rerun_plan.h"
#include "rxgpu_hnsw_internal.h"

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::ProfileScope;
using rxgpu::set_error;

namespace {

using rxgpu::default_k_ef;
using rxgpu::fill_hnsw_params;
using rxgpu::fill_sq8_params;
using rxgpu::HnswKnobs;
using rxgpu::HnswLaunchPlan;
using rxgpu::HnswRequest;

// 1: the index's resident kernel answered; 0: it does not take this query (the caller launches); 2: it ran the search and the search came back
// flagged (the launches' re-run tiers answer it); otherwise an error code.  qcorr != nullptr: `query` are SQ8 codes, through the mailbox over codes.
int hnsw_try_server(rxgpu_index* h, const HnswKnobs& knobs, const void* query, const float* qcorr, const float* qnorm, uint32_t k, uint32_t ef,
					float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	if (knobs.server == 0 || knobs.names_a_kernel) return 0;
	if (qcorr && knobs.server_sq8 == 0) return 0;
	rxgpu::HnswServerConfig cfg;
	if (knobs.server_slots > 0) cfg.slots = uint32_t(knobs.server_slots);
	if (knobs.server_idle_us > 0) cfg.idle_us = uint32_t(knobs.server_idle_us);
	if (knobs.server_life_ms > 0) cfg.life_ms = uint32_t(knobs.server_life_ms);
	cfg.spec = knobs.spec > 0;
	cfg.nbl = knobs.nbl > 0;
	if (qcorr) return rxgpu::hnsw_server_search_sq8(h, cfg, static_cast<const uint8_t*>(query), *qcorr, *qnorm, k, ef, out_dist, out_row, out_count);
	return rxgpu::hnsw_server_search(h, cfg, static_cast<const float*>(query), k, ef, out_dist, out_row, out_count);
}

// The device-side search counters [first, first + n) of the index (d_hnsw_stats: evals, hops, in-kernel restarts, distance trips of the
// speculative team searches), taken: the device is waited for, the counters are copied out and cleared.
int take_hnsw_stats(rxgpu_index* h, uint32_t first, uint32_t n, unsigned long long* v) {
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	RX_HIP(hipMemcpy(v, h->d_hnsw_stats + first, n * sizeof(*v), hipMemcpyDeviceToHost));
	RX_HIP(hipMemset(h->d_hnsw_stats + first, 0, n * sizeof(*v)));
	return RXGPU_OK;
}
// out[0 .. n) = the sum over the shards' graphs of what read(shard, values) yields
template <class Read>
int sum_over_shards(rxgpu_index* h, uint32_t n, uint64_t* out, Read read) {
	std::fill(out, out + n, uint64_t(0));
	for (uint32_t s = 0; s < rxgpu_index_shard_count(h); ++s) {
		uint64_t v[2] = {0, 0};
		if (int rc = read(rxgpu_index_shard(h, s), v); rc) return rc;
		for (uint32_t i = 0; i < n; ++i) out[i] += v[i];
	}
	return RXGPU_OK;
}

// Helper workgroups beside a large batch (hnsw_helper_kernel, second stream): a search that overflows its LDS heap area is queued and
// runs with the largest LDS heap while the batch is still going, instead of as a launch of its own behind it.  RXGPU_HNSW_HELPER=0: off.
// ONE batch at a time has helpers, and only a batch that is one chunk.  A helper polls until ITS batch is over; HIP streams share a
// few hardware queues, so with two callers at it helper A can sit in front of batch B's kernels while helper B sits in front of
// batch A's — each waits for a batch that cannot start, until the helpers' wall-clock bail-out (seconds: four threads with 2300-query
// batches measured 3 s calls, tests/test_gpu_hnsw_visited.py).  With a single set of helpers in flight nothing that spins ever waits
// for work queued behind another spinner; the callers that come second run their overflowing searches behind their batch, as batches
// below 2048 queries always do.  (The same inside one call: the kernels of a second chunk would queue up behind its own helpers.)
std::atomic<bool> g_helpers_in_flight{false};
struct HelperBatch {
	static constexpr uint32_t kGroups = 64, kCap = rxgpu::kHnswHelperQueueCap;
	bool held = false;              // this call has the helpers (until the object goes: HnswCall::first_pass)
	uint32_t* hq_words = nullptr;   // [0] entries appended, [1] stop, [2] searches of the batch that have ended, [16 ..] ids
	uint32_t n = 0;                 // entries appended, once the batch's stream has been waited for
	~HelperBatch() {
		if (held) g_helpers_in_flight.store(false, std::memory_order_release);
	}
	// takes the helpers if nobody has them, and empties the overflow queue in front of the batch
	int begin(rxgpu_search_ctx* c, uint64_t words) {
		bool expected = false;
		held = g_helpers_in_flight.compare_exchange_strong(expected, true, std::memory_order_acq_rel);
		if (!held) return RXGPU_OK;
		const uint64_t words4 = (words + 3) & ~uint64_t(3);
		const size_t hq_bytes = (size_t(kCap) + 16) * 4;
		if (int rc = c->ensure_aux(); rc) return rc;
		if (int rc = c->d_helper.ensure(hq_bytes); rc) return rc;
		if (int rc = c->d_helper_bits.ensure(size_t(kGroups) * words4 * 4); rc) return rc;
		hq_words = static_cast<uint32_t*>(c->d_helper.ptr);
		RX_HIP(hipMemsetAsync(hq_words, 0, hq_bytes, c->aux_stream));
		RX_HIP(hipEventRecord(c->main_done, c->aux_stream));      // the queue is empty before the first search of the batch can append to it
		RX_HIP(hipStreamWaitEvent(c->stream, c->main_done, 0));
		return RXGPU_OK;
	}
	// The helpers spin until the batch says stop, so they are enqueued BEHIND the batch's launches: HIP streams share a few
	// hardware queues, and a helper that reached a queue in front of the batch kernel it waits for would hold that queue until its
	// wall-clock bail-out.  Launched last, the worst case is the serial one — helpers behind the batch on one queue find the stop flag and
	// only drain what was queued; on separate queues they run beside the batch as intended.
	int launch(rxgpu_index* h, rxgpu_search_ctx* c, const rxgpu::HnswParams& batch, const void* d_q) {   // batch: what the batch's launches share
		const uint64_t words4 = (batch.visited_words + 3) & ~uint64_t(3);
		rxgpu::HnswParams ph = batch;
		ph.queries = static_cast<const float*>(d_q);
		ph.visited = static_cast<uint32_t*>(c->d_helper_bits.ptr);
		ph.visited_words = words4;
		ph.vis_hash_log2 = 0;
		ph.vis_lds_log2 = 0;
		ph.lds_cand_cap = uint32_t(rxgpu::kHnswCandLds);
		ph.sorted = 0;
		rxgpu::HnswHelper hq{hq_words, hq_words + 16, hq_words + 1, hq_words + 2, batch.nq, kCap, 100000000ull};   // (last resort: gives up after 1 s)
		rxgpu::launch_hnsw_helper(h->metric, ph, hq, kGroups, c->aux_stream);
		RX_HIP(hipGetLastError());
		return RXGPU_OK;
	}
	// the batch is over: tell the helpers, take their results with the batch's
	int finish(rxgpu_search_ctx* c) {
		RX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(hq_words + 1), 1, 1, c->stream));
		RX_HIP(hipEventRecord(c->aux_done, c->aux_stream));
		RX_HIP(hipStreamWaitEvent(c->stream, c->aux_done, 0));
		RX_HIP(hipMemcpyAsync(&n, hq_words, sizeof(n), hipMemcpyDeviceToHost, c->stream));
		return RXGPU_OK;
	}
};

// One call of hnsw_search_impl behind its plan: where its queries and results live, and the moves its passes share.
struct HnswCall {
	rxgpu_index* h;
	rxgpu_search_ctx* c;
	const HnswLaunchPlan& pl;
	const HnswRequest& rq;       // k and ef defaulted
	const uint32_t nq = rq.nq, k = rq.k;
	const bool sq8 = rq.qcorr != nullptr;
	size_t row_bytes = 0;        // of one query
	rxgpu::HnswParams p{};       // what every launch of the call shares
	const void* d_q = nullptr;   // where the kernels read the queries
	const uint32_t* allowed = nullptr;   // a call under an allowed-rows bitmap: the bitmap in this call's context (HBM), beside p in every launch
	// where counts and lists arrive on the host: the caller's arrays, or the pinned staging buffer
	uint32_t* dl_count = nullptr;
	float* dl_dist = nullptr;
	uint32_t* dl_row = nullptr;
	bool lists_on_host = false;  // the lists travelled with the counts of the first pass, and no re-run has changed them since
	// Output and query buffers, the early zeroing, the staging buffer, the first upload (the bitmap with it), and the parameters every launch shares.
	int stage_and_upload() {
		row_bytes = size_t(h->dim) * (sq8 ? sizeof(uint8_t) : sizeof(float));
		if (!rq.dev_q) {   // (queries in HBM are read where they are)
			if (int rc = c->d_queries.ensure(sq8 ? pl.o_qnorm + size_t(nq) * 4 : size_t(nq) * row_bytes); rc) return rc;
		}
		if (int rc = c->d_out_dist.ensure(size_t(nq) * k * sizeof(float)); rc) return rc;
		if (int rc = c->d_out_row.ensure(size_t(nq) * k * sizeof(uint32_t)); rc) return rc;
		if (int rc = c->d_out_count.ensure(size_t(nq) * sizeof(uint32_t)); rc) return rc;
		if (pl.first_zero_bytes) {   // (HnswLaunchPlan: on the second stream, in front of the upload; the first launch waits for aux_done)
			if (int rc = c->d_visited.ensure(pl.first_zero_bytes); rc) return rc;
			if (int rc = c->ensure_aux(); rc) return rc;
			RX_HIP(hipMemsetAsync(c->d_visited.ptr, 0, pl.first_zero_bytes, c->aux_stream));
			RX_HIP(hipEventRecord(c->aux_done, c->aux_stream));
		}
		if (pl.split_upload) {
			if (int rc = c->ensure_aux(); rc) return rc;
		}
		const void* up_queries = rq.queries;
		const float *up_qcorr = rq.qcorr, *up_qnorm = rq.qnorm;
		dl_count = rq.out_count;
		dl_dist = rq.out_dist;
		dl_row = rq.out_row;
		char* zc_dev = nullptr;   // the pinned buffer as the device sees it
		if (pl.staged) {
			if (int rc = c->ensure_pinned(pl.st_end); rc) return rc;
			char* hp = static_cast<char*>(c->h_pinned);
			if (pl.zero_copy) {
				void* dv = nullptr;
				RX_HIP(hipHostGetDevicePointer(&dv, hp, 0));
				zc_dev = static_cast<char*>(dv);
			}
			if (!rq.dev_q) {
				std::memcpy(hp, rq.queries, size_t(nq) * row_bytes);
				up_queries = hp;
			}
			if (sq8) {
				std::memcpy(hp + pl.st_corr, rq.qcorr, size_t(nq) * 4);
				std::memcpy(hp + pl.st_norm, rq.qnorm, size_t(nq) * 4);
				up_qcorr = reinterpret_cast<const float*>(hp + pl.st_corr);
				up_qnorm = reinterpret_cast<const float*>(hp + pl.st_norm);
			}
			dl_count = reinterpret_cast<uint32_t*>(hp + pl.st_count);
			dl_dist = reinterpret_cast<float*>(hp + pl.st_dist);
			dl_row = reinterpret_cast<uint32_t*>(hp + pl.st_row);
		}
		d_q = rq.dev_q ? rq.queries : pl.zero_copy ? static_cast<void*>(zc_dev) : c->d_queries.ptr;
		if (!pl.zero_copy && !rq.dev_q) RX_HIP(hipMemcpyAsync(c->d_queries.ptr, up_queries, size_t(pl.part_q) * row_bytes, hipMemcpyHostToDevice, c->stream));
		if (sq8) {
			char* qb = static_cast<char*>(c->d_queries.ptr);
			RX_HIP(hipMemcpyAsync(qb + pl.o_qcorr, up_qcorr, size_t(nq) * 4, hipMemcpyHostToDevice, c->stream));
			RX_HIP(hipMemcpyAsync(qb + pl.o_qnorm, up_qnorm, size_t(nq) * 4, hipMemcpyHostToDevice, c->stream));
			fill_sq8_params(h, p);
			p.qcodes = reinterpret_cast<const uint8_t*>(qb);
			p.qcorr = reinterpret_cast<const float*>(qb + pl.o_qcorr);
			p.qnorm = reinterpret_cast<const float*>(qb + pl.o_qnorm);
		}
		fill_hnsw_params(h, p);
		p.nq = nq;
		p.k = k;
		p.ef = rq.ef;
		p.visited_words = pl.words;
		p.vis_lds_log2 = pl.vis_lds_log2;
		p.prefetch_links = pl.prefetch_links;
		p.team = pl.team;
		p.team_max = pl.team_max;
		p.nbl = pl.nbl;
		p.spec = pl.spec;
		p.out_dist = pl.zero_copy ? reinterpret_cast<float*>(zc_dev + pl.st_dist) : static_cast<float*>(c->d_out_dist.ptr);
		p.out_row = pl.zero_copy ? reinterpret_cast<uint32_t*>(zc_dev + pl.st_row) : static_cast<uint32_t*>(c->d_out_row.ptr);
		p.out_count = pl.zero_copy ? reinterpret_cast<uint32_t*>(zc_dev + pl.st_count) : static_cast<uint32_t*>(c->d_out_count.ptr);
		p.stats = h->d_hnsw_stats;
		p.ef_cap = pl.ef_cap;
		p.lds_cand_cap = pl.lds_cand_cap;
		if (rq.allowed) {   // the bitmap, once, into this call's context: launch() hands it to the first pass and every re-run tier
			const size_t bytes = size_t((h->count + 31) / 32) * sizeof(uint32_t);
			if (int rc = c->d_allowed.ensure(bytes); rc) return rc;
			RX_HIP(hipMemcpyAsync(c->d_allowed.ptr, rq.allowed, bytes, hipMemcpyHostToDevice, c->stream));
			allowed = static_cast<const uint32_t*>(c->d_allowed.ptr);
			p.bare = 0;   // hidden nodes are traversed like deleted ones (hnswalg.h:1982: the branch with deleted nodes)
		}
		return RXGPU_OK;
	}

	// counts / lists back to the host (nothing to do when the kernels wrote them there), and the wait behind a small launch: polled — the
	// wake-up out of hipStreamSynchronize alone is tens of microseconds
	int fetch_counts() {
		if (!pl.zero_copy) RX_HIP(hipMemcpyAsync(dl_count, c->d_out_count.ptr, size_t(nq) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		return RXGPU_OK;
	}
	int fetch_lists() {
		if (!pl.zero_copy) {
			RX_HIP(hipMemcpyAsync(dl_dist, c->d_out_dist.ptr, size_t(nq) * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
			RX_HIP(hipMemcpyAsync(dl_row, c->d_out_row.ptr, size_t(nq) * k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		}
		return RXGPU_OK;
	}
	int wait_stream() {
		if (nq <= 256) {
			const auto t0 = std::chrono::steady_clock::now();
			hipError_t q = hipStreamQuery(c->stream);
			while (q == hipErrorNotReady && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < 4000.0) q = hipStreamQuery(c->stream);
			if (q != hipErrorNotReady) {
				RX_HIP(q);
				return RXGPU_OK;
			}
		}
		RX_HIP(hipStreamSynchronize(c->stream));
		return RXGPU_OK;
	}
	int done_host() {   // (behind the last hipStreamSynchronize) what was staged goes to the caller's arrays
		if (pl.staged) {
			std::memcpy(rq.out_count, dl_count, size_t(nq) * 4);
			if (!rq.sink) {
				std::memcpy(rq.out_dist, dl_dist, size_t(nq) * k * 4);
				std::memcpy(rq.out_row, dl_row, size_t(nq) * k * 4);
			}
		}
		return RXGPU_OK;
	}
	int to_sink() {   // the finished lists into the exchange's send buffer (sharded HNSW), on this search's stream, drained
		rxgpu::launch_pack_lists(p.out_dist, p.out_row, p.out_count, nq, k, rq.sink->kk, rq.sink->d_dist, rq.sink->d_row, c->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(c->stream));
		return done_host();   // (the counts)
	}

	// searches [qa, qa + cnt) of the batch on stream st (slot = index inside this launch's visited block)
	void launch_part(uint32_t qa, uint32_t cnt, uint32_t slot0, hipStream_t st, const HelperBatch& helpers) {
		rxgpu::HnswParams pc = p;
		pc.vis_hash_log2 = pl.vis_hash_log2;
		pc.visited_words = pl.vis_words;
		pc.queries = reinterpret_cast<const float*>(static_cast<const char*>(d_q) + size_t(qa) * row_bytes);
		if (sq8) {
			pc.qcodes = p.qcodes + size_t(qa) * h->dim;
			pc.qcorr = p.qcorr + qa;
			pc.qnorm = p.qnorm + qa;
		}
		pc.visited = static_cast<uint32_t*>(c->d_visited.ptr) + size_t(slot0) * pl.vis_words;
		pc.out_dist = p.out_dist + size_t(qa) * k;
		pc.out_row = p.out_row + size_t(qa) * k;
		pc.out_count = p.out_count + qa;
		if (helpers.held) {
			pc.helper_n = helpers.hq_words;
			pc.helper_ids = helpers.hq_words + 16;
			pc.helper_cap = HelperBatch::kCap;
			pc.q_base = qa;
		}
		if (pl.use_sorted) {   // the list lives in registers; LDS holds only the heap area of a search that starts over (equal keys that matter)
			pc.sorted = pl.sorted_mode;
			pc.lds_cand_cap = pl.sorted_restart_cap;
			if (pl.sorted_restart_cap == 0) pc.ef_cap = 0;
		}
		launch(pc, cnt, false, st);
	}
	// every launch of the call, first pass and re-run tiers alike: a call under a bitmap takes the filtered family and nothing else
	void launch(const rxgpu::HnswParams& pc, uint32_t cnt, bool global_cand, hipStream_t st) {
		if (allowed) {
			rxgpu::HnswFilteredParams pf{};
			static_cast<rxgpu::HnswParams&>(pf) = pc;
			pf.allowed = allowed;
			rxgpu::launch_hnsw_filtered(h->metric, pf, cnt, global_cand, st);
		} else {
			rxgpu::launch_hnsw_search(h->metric, pc, cnt, global_cand, st);
		}
	}

	// Every query once, in launches of vis_slots searches; counts (and lists) are on the host when it returns, and in *helper_entries what
	// the searches appended to the helpers' overflow queue (0 for a batch without helpers).  The helpers are this call's for as long as the
	// pass lasts: they have left when its stream has been waited for.
	int first_pass(uint32_t* helper_entries) {
		HelperBatch helpers;
		if (pl.helper_wanted && uint64_t(nq) <= pl.vis_slots) {
			if (int rc = helpers.begin(c, pl.words); rc) return rc;
		}
		bool helpers_launched = false;
		for (uint32_t q0 = 0; q0 < nq; q0 += uint32_t(pl.vis_slots)) {
			const uint32_t cq = uint32_t(std::min<uint64_t>(pl.vis_slots, nq - q0));
			if (int rc = c->d_visited.ensure(size_t(cq) * pl.vis_words * 4); rc) return rc;
			if (!pl.vis_hash_log2) {
				const size_t zero_bytes = size_t(cq) * pl.words * 4;
				if (q0 == 0 && pl.first_zero_bytes) {
					RX_HIP(hipStreamWaitEvent(c->stream, c->aux_done, 0));
				} else {   // (a later chunk of the same call reuses the buffer behind the chunk before it)
					RX_HIP(hipMemsetAsync(c->d_visited.ptr, 0, zero_bytes, c->stream));
				}
			}
			ProfileScope ps(h, "hnsw", c->stream);   // (with two halves: until the main stream has waited for the second one)
			if (pl.split_upload) {
				hipStream_t sb = c->aux2_stream;
				// whatever the first half waits for — zeroed bitsets, the empty overflow queue, the SQ8 query terms — the second half waits for too
				RX_HIP(hipEventRecord(c->split_done, c->stream));
				RX_HIP(hipStreamWaitEvent(sb, c->split_done, 0));
				launch_part(0, pl.part_q, 0, c->stream, helpers);
				for (uint32_t qa = pl.part_q, part = 1; qa < nq; qa += pl.part_q, ++part) {
					const uint32_t cnt = std::min(pl.part_q, nq - qa);
					hipStream_t st = (part & 1u) ? sb : c->stream;
					const size_t off = size_t(qa) * row_bytes;
					if (!rq.dev_q) RX_HIP(hipMemcpyAsync(static_cast<char*>(c->d_queries.ptr) + off, static_cast<const char*>(rq.queries) + off, size_t(cnt) * row_bytes, hipMemcpyHostToDevice, st));
					launch_part(qa, cnt, qa, st, helpers);
				}
				RX_HIP(hipEventRecord(c->split_done, sb));
				RX_HIP(hipStreamWaitEvent(c->stream, c->split_done, 0));
			} else {
				launch_part(q0, cq, 0, c->stream, helpers);
			}
			if (helpers.held && !helpers_launched) {   // behind the first chunk's launches (all of them, for a batch that fits one chunk)
				if (int rc = helpers.launch(h, c, p, d_q); rc) return rc;
				helpers_launched = true;
			}
		}
		RX_HIP(hipGetLastError());
		if (helpers.held) {
			if (int rc = helpers.finish(c); rc) return rc;
		}
		// counts and results travel together: a batch without re-runs (the common case for a handful of queries) is done after ONE wait
		if (int rc = fetch_counts(); rc) return rc;
		if (!rq.sink) {
			if (int rc = fetch_lists(); rc) return rc;
			lists_on_host = true;
		}
		if (int rc = wait_stream(); rc) return rc;
		*helper_entries = helpers.n;
		return RXGPU_OK;
	}

	// One step of the re-run ladder (hnsw_rerun_plan.h): the searches step.ids of the batch once more, step.slots of them per launch, with the
	// call's parameters and what the rung sets in them; their new counts are on the host when it returns.
	int rerun(const rxgpu::HnswRerunStep& step) {
		rxgpu::HnswParams tier = p;
		tier.vis_hash_log2 = step.vis_hash_log2;
		tier.visited_words = step.visited_words;
		tier.lds_cand_cap = step.lds_cand_cap;
		tier.vis_lds_log2 = step.vis_lds_log2;
		tier.gcand_cap = step.gcand_cap;
		const std::vector<uint32_t>& ids = step.ids;
		const bool global_cand = tier.gcand_cap != 0;
		lists_on_host = false;
		if (int rc = c->d_redo.ensure(ids.size() * sizeof(uint32_t)); rc) return rc;
		RX_HIP(hipMemcpyAsync(c->d_redo.ptr, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		for (size_t r0 = 0; r0 < ids.size(); r0 += step.slots) {
			const uint32_t cq = uint32_t(std::min<uint64_t>(step.slots, ids.size() - r0));
			if (int rc = c->d_visited.ensure(size_t(cq) * tier.visited_words * 4); rc) return rc;
			if (global_cand) {
				if (int rc = c->d_gcand_d.ensure(size_t(cq) * tier.gcand_cap * sizeof(uint2)); rc) return rc;
			}
			if (!tier.vis_hash_log2) RX_HIP(hipMemsetAsync(c->d_visited.ptr, 0, size_t(cq) * tier.visited_words * 4, c->stream));
			rxgpu::HnswParams pc = tier;
			pc.queries = static_cast<const float*>(d_q);
			pc.visited = static_cast<uint32_t*>(c->d_visited.ptr);
			pc.only = static_cast<const uint32_t*>(c->d_redo.ptr) + r0;
			if (global_cand) pc.gcand = static_cast<uint2*>(c->d_gcand_d.ptr);
			ProfileScope ps(h, step.profile_name, c->stream);
			launch(pc, cq, global_cand, c->stream);
		}
		RX_HIP(hipGetLastError());
		if (int rc = fetch_counts(); rc) return rc;
		RX_HIP(hipStreamSynchronize(c->stream));
		return RXGPU_OK;
	}
	// the lists: packed into the sink, or to the caller — once more behind a re-run (and for a call that had no first pass)
	int finish() {
		if (rq.sink) return to_sink();
		if (!lists_on_host) {
			if (int rc = fetch_lists(); rc) return rc;
			RX_HIP(hipStreamSynchronize(c->stream));
		}
		return done_host();
	}
};

}  // namespace

namespace rxgpu {

int hnsw_search_impl(rxgpu_index* h, const HnswRequest& request) {
	// 1. validate and normalise
	HnswRequest rq = request;
	const bool to_host = rq.sink == nullptr;
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_sq8: not available on a sharded index");
	RX_CHECK(rq.queries && rq.out_count && (rq.sink || (rq.out_dist && rq.out_row)), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: null argument");
	if (rq.nq == 0) return RXGPU_OK;
	if (h->count == 0 || rq.k == 0) {   // hnswalg.h:1989-1991
		RX_CHECK(to_host, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn: an empty shard has no list to send");
		std::fill(rq.out_count, rq.out_count + rq.nq, 0u);
		return RXGPU_OK;
	}
	RX_CHECK(h->graph_attached && h->graph_n == h->count, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn: graph is not attached / out of date");
	default_k_ef(h, rq.k, rq.ef);
	RX_CHECK(rq.ef <= uint32_t(rxgpu::kHnswMaxEf), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: ef must be <= 4096 on the GPU engine");
	const HnswKnobs knobs = rxgpu::read_hnsw_knobs();
	// 2. ONE query, the planner's call: through the mailbox of the index's resident kernel (rxgpu_hnsw_server.hip) — no launch on the path
	if (rq.nq == 1 && to_host && rq.try_server && !rq.allowed) {
		const int served = hnsw_try_server(h, knobs, rq.queries, rq.qcorr, rq.qnorm, rq.k, rq.ef, rq.out_dist, rq.out_row, rq.out_count);
		if (served == 1) return RXGPU_OK;
		if (served != 0 && served != 2) return served;   // (2: the search ran there and came back flagged — the tiers below answer it)
	}
	// 3. a context of its own
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	// 4. the plan (a handful of searches never comes near the visited budget: no driver call on the path of a single-query SearchKnn)
	size_t free_b = 0, total_b = 0;
	if (rq.nq > 256 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
	const HnswLaunchPlan pl = rxgpu::plan_hnsw_search(h->count, h->dim, h->graph_deleted == 0 && !rq.allowed, rq.nq, rq.k, rq.ef, rq.qcorr != nullptr, to_host,
													  uint64_t(free_b) + c->d_visited.bytes, knobs, rq.allowed != nullptr);
	// 5. staging and the first upload
	HnswCall call{h, c, pl, rq};
	if (int rc = call.stage_and_upload(); rc) return rc;
	// 6. the first pass (ef > 1024 has none: the ladder starts every query on its global tiers)
	uint32_t helper_entries = 0;
	if (!pl.big_ef) {
		if (int rc = call.first_pass(&helper_entries); rc) return rc;
	}
	// 7. the re-runs, as long as the counts on the host ask for one
	rxgpu::HnswRerunLadder ladder(pl, rq.nq, helper_entries);
	int rc = RXGPU_OK;
	for (const rxgpu::HnswRerunStep* step; !rc && (step = ladder.next(call.dl_count)) != nullptr;) rc = call.rerun(*step);
	h->hnsw_lds_reruns += ladder.lds_reruns;
	if (ladder.tie_reruns) h->hnsw_tie_reruns += ladder.tie_reruns;
	if (rc) return rc;
	RX_CHECK(!ladder.overflowed(), RXGPU_ERR_DEVICE, "rxgpu_hnsw_search_knn: a candidate heap of one entry per node overflowed");
	// 8. the lists: to the caller, or packed into the sink
	return call.finish();
}

int hnsw_search_to_sink(rxgpu_index* shard, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, const HnswSink& sink) {
	std::vector<uint32_t> counts(nq);
	RX_CHECK(!qcorr || (shard->d_codes && shard->sq8_n == shard->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_sq8: SQ8 codes are not attached / out of date on a shard");
	HnswRequest rq;
	rq.queries = queries, rq.qcorr = qcorr, rq.qnorm = qnorm, rq.nq = nq, rq.k = k, rq.ef = ef;
	rq.out_count = counts.data(), rq.sink = &sink;
	return hnsw_search_impl(shard, rq);
}
// The construction searches of one build batch (rxgpu_hnsw_build.hip): the queries are nq packed float rows in HBM, the graph is the one of
// the first `nodes` rows — the rows behind them are stored but not linked yet, so for the length of the call the index counts `nodes` rows.
// The caller holds the index exclusively (a build batch changes the lists the searches read).
int hnsw_search_rows_to_sink(rxgpu_index* h, const float* d_queries, uint32_t nq, uint32_t k, uint32_t ef, uint64_t nodes, const HnswSink& sink) {
	struct CountAs {
		rxgpu_index* h;
		uint64_t keep;
		~CountAs() { h->count = keep; }
	} restore{h, h->count};
	h->count = nodes;
	std::vector<uint32_t> counts(nq);
	HnswRequest rq;
	rq.queries = d_queries, rq.dev_q = true, rq.nq = nq, rq.k = k, rq.ef = ef;
	rq.out_count = counts.data(), rq.sink = &sink, rq.try_server = false;
	return hnsw_search_impl(h, rq);
}
}  // namespace rxgpu

extern "C" {

/* ------------------------------------------------------------------------------------------------ SearchKnn */

namespace {
// one body for both row formats (qcorr == nullptr: float rows), behind the callers' argument checks
int hnsw_posted_impl(rxgpu_index* h, const void* query, const float* qcorr, const float* qnorm, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row,
					 uint32_t* out_count, int32_t* served) {
	*served = 0;
	if (h->shard_set || h->count == 0 || k == 0 || !h->graph_attached || h->graph_n != h->count) return RXGPU_OK;   // the launching call says what is wrong
	if (qcorr && (!h->d_codes || h->sq8_n != h->count)) return RXGPU_OK;
	default_k_ef(h, k, ef);
	const int rc = hnsw_try_server(h, rxgpu::read_hnsw_knobs(), query, qcorr, qnorm, k, ef, out_dist, out_row, out_count);
	if (rc == 1) {
		*served = 1;
		return RXGPU_OK;
	}
	if (rc == 2) {   // the mailbox took it and the search needs the re-run tiers: answered here by the launches, not offered to the mailbox again
		HnswRequest rq;
		rq.queries = query, rq.qcorr = qcorr, rq.qnorm = qnorm, rq.nq = 1, rq.k = k, rq.ef = ef;
		rq.out_dist = out_dist, rq.out_row = out_row, rq.out_count = out_count;
		rq.try_server = false;
		const int r2 = hnsw_search_impl(h, rq);
		if (r2 == RXGPU_OK) *served = 1;
		return r2;
	}
	return rc;
}
}  // namespace

int rxgpu_hnsw_distance_blocks(uint32_t dim, int sq8, int deleted, int* mailbox) {
	if (mailbox) *mailbox = rxgpu::hnsw_mailbox_serves(dim, sq8 != 0, deleted != 0) ? 1 : 0;
	return rxgpu::hnsw_distance_blocks(dim, sq8 != 0, deleted != 0);
}

int rxgpu_hnsw_search_knn_posted(rxgpu_index* h, const float* query, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row, uint32_t* out_count,
								 int32_t* served) {
	RX_CHECK(h && query && out_dist && out_row && out_count && served, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_posted: null argument");
	return hnsw_posted_impl(h, query, nullptr, nullptr, k, ef, out_dist, out_row, out_count, served);
}

int rxgpu_hnsw_search_knn_sq8_posted(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t k, uint32_t ef,
									 float* out_dist, uint32_t* out_row, uint32_t* out_count, int32_t* served) {
	RX_CHECK(h && query_codes && out_dist && out_row && out_count && served, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_sq8_posted: null argument");
	return hnsw_posted_impl(h, query_codes, &query_corr, &query_norm_coef, k, ef, out_dist, out_row, out_count, served);
}

int rxgpu_hnsw_server_times(rxgpu_index* h, uint64_t* device_us, uint64_t* caller_us) {
	RX_CHECK(h && device_us && caller_us, RXGPU_ERR_PARAMS, "rxgpu_hnsw_server_times: null argument");
	rxgpu::hnsw_server_times(h, device_us, caller_us);
	return RXGPU_OK;
}

int rxgpu_hnsw_server_stats(rxgpu_index* h, uint64_t* served, uint64_t* generations) {
	RX_CHECK(h && served && generations, RXGPU_ERR_PARAMS, "rxgpu_hnsw_server_stats: null argument");
	rxgpu::hnsw_server_counters(h, served, generations);
	return RXGPU_OK;
}

int rxgpu_hnsw_search_knn(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row,
						  uint32_t* out_count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(queries, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: null argument");
	if (h->shard_set) {   // SURVEY 8(e) "HNSW": a graph per shard, the per-shard results meet in the same all-gather + merge as brute force
		RX_CHECK(out_dist && out_row && out_count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: null argument");
		return rxgpu::sharded_hnsw_search_knn(h, queries, nullptr, nullptr, nq, k, ef, out_dist, out_row, out_count);
	}
	HnswRequest rq;
	rq.queries = queries, rq.nq = nq, rq.k = k, rq.ef = ef;
	rq.out_dist = out_dist, rq.out_row = out_row, rq.out_count = out_count;
	return hnsw_search_impl(h, rq);
}

int rxgpu_hnsw_search_knn_sq8(rxgpu_index* h, const uint8_t* query_codes, const float* query_corr, const float* query_norm_coef, uint32_t nq,
							  uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(query_codes && query_corr && query_norm_coef, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_sq8: null argument");
	if (h->shard_set) {   // every shard searches the code table attached to ITS handle (rxgpu_hnsw_attach_sq8 on rxgpu_index_shard(h, s)); same exchange
		RX_CHECK(out_dist && out_row && out_count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_sq8: null argument");
		for (uint32_t s = 0; s < rxgpu_index_shard_count(h); ++s) {
			const rxgpu_index* sh = rxgpu_index_shard(h, s);
			RX_CHECK(sh->count == 0 || (sh->d_codes && sh->sq8_n == sh->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_sq8: SQ8 codes are not attached / out of date on a shard");
		}
		return rxgpu::sharded_hnsw_search_knn(h, query_codes, query_corr, query_norm_coef, nq, k, ef, out_dist, out_row, out_count);
	}
	RX_CHECK(h->count == 0 || (h->d_codes && h->sq8_n == h->count), RXGPU_ERR_LOGIC,
			 "rxgpu_hnsw_search_knn_sq8: SQ8 codes are not attached / out of date");
	HnswRequest rq;
	rq.queries = query_codes, rq.qcorr = query_corr, rq.qnorm = query_norm_coef, rq.nq = nq, rq.k = k, rq.ef = ef;
	rq.out_dist = out_dist, rq.out_row = out_row, rq.out_count = out_count;
	return hnsw_search_impl(h, rq);
}

/* SearchKnn under an allowed-rows bitmap: the reference has no filter functor, so the result is defined through its delete mark — hnswalg.h:1982
 * (num_deleted picks the branch), :871-963 (runLayer0Step keeps a marked node in candidate_set and out of top_candidates), :1303-1339
 * (MarkDelete).  One body for floats and codes. */
static int hnsw_filtered_entry(rxgpu_index* h, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k,
							   uint32_t ef, const uint32_t* allowed_words, uint64_t n_words, float* out_dist, uint32_t* out_row, uint32_t* out_count,
							   uint64_t* out_allowed) {
	const bool sq8 = qcorr != nullptr;
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_filtered: not available on a sharded index (its shard handles take the call)");
	RX_CHECK(queries && (!sq8 || qnorm), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_filtered: null argument");
	RX_CHECK(allowed_words, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_filtered: null bitmap");
	const uint64_t words = (h->count + 31) / 32;
	RX_CHECK(n_words >= words, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_filtered: the bitmap is shorter than ceil(count / 32) words");
	RX_CHECK(ef <= uint32_t(rxgpu::kHnswMaxEf), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_filtered: ef must be <= 4096 on the GPU engine");
	RX_CHECK(h->count == 0 || (h->graph_attached && h->graph_n == h->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_filtered: graph is not attached / out of date");
	RX_CHECK(!sq8 || h->count == 0 || (h->d_codes && h->sq8_n == h->count), RXGPU_ERR_LOGIC,
			 "rxgpu_hnsw_search_knn_sq8_filtered: SQ8 codes are not attached / out of date");
	if (nq == 0 || k == 0) return RXGPU_OK;
	RX_CHECK(out_count && out_dist && out_row, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_filtered: null argument");
	uint64_t set = 0;   // bits below the node count
	for (uint64_t w = 0; w < words; ++w) {
		uint32_t v = allowed_words[w];
		if (w == words - 1 && (h->count & 31u)) v &= (1u << (h->count & 31u)) - 1u;
		set += uint64_t(__builtin_popcount(v));
	}
	if (out_allowed) *out_allowed = set;
	HnswRequest rq;
	rq.queries = queries, rq.qcorr = qcorr, rq.qnorm = qnorm, rq.nq = nq, rq.k = k, rq.ef = ef;
	rq.out_dist = out_dist, rq.out_row = out_row, rq.out_count = out_count;
	// nothing hidden at all: the reference would take its bare-bone branch — the unfiltered path answers, and nothing else
	if (h->graph_deleted != 0 || set != h->count) {
		rq.allowed = allowed_words;
		rq.try_server = false;
	}
	return hnsw_search_impl(h, rq);
}

int rxgpu_hnsw_search_knn_filtered(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, const uint32_t* allowed_words,
								   uint64_t n_words, float* out_dist, uint32_t* out_row, uint32_t* out_count, uint64_t* out_allowed) {
	return hnsw_filtered_entry(h, queries, nullptr, nullptr, nq, k, ef, allowed_words, n_words, out_dist, out_row, out_count, out_allowed);
}

int rxgpu_hnsw_search_knn_sq8_filtered(rxgpu_index* h, const uint8_t* query_codes, const float* query_corr, const float* query_norm_coef, uint32_t nq,
									   uint32_t k, uint32_t ef, const uint32_t* allowed_words, uint64_t n_words, float* out_dist, uint32_t* out_row,
									   uint32_t* out_count, uint64_t* out_allowed) {
	RX_CHECK(query_corr, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn_sq8_filtered: null argument");
	return hnsw_filtered_entry(h, query_codes, query_corr, query_norm_coef, nq, k, ef, allowed_words, n_words, out_dist, out_row, out_count, out_allowed);
}

/* ------------------------------------------------------------------------------------------------ counters */

int rxgpu_hnsw_read_stats(rxgpu_index* h, uint64_t* distance_evals, uint64_t* hops) {
	RX_CHECK(h && distance_evals && hops, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_stats: null argument");
	*distance_evals = 0;
	*hops = 0;
	if (h->shard_set) {
		uint64_t sum[2] = {0, 0};
		const int rc = sum_over_shards(h, 2, sum, [](rxgpu_index* sh, uint64_t* v) { return rxgpu_hnsw_read_stats(sh, &v[0], &v[1]); });
		*distance_evals = sum[0];
		*hops = sum[1];
		return rc;
	}
	if (!h->d_hnsw_stats) return RXGPU_OK;
	unsigned long long v[4] = {0, 0, 0, 0};   // evals, hops, in-kernel restarts, distance trips of the speculative team searches
	if (int rc = take_hnsw_stats(h, 0, 4, v); rc) return rc;
	*distance_evals = v[0];
	*hops = v[1];
	if (std::getenv("RXGPU_HNSW_TRIPS")) std::fprintf(stderr, "[rxgpu hnsw] hops %llu evals %llu restarts %llu speculative-search distance trips %llu\n", v[1], v[0], v[2], v[3]);
	if (std::getenv("RXGPU_HNSW_PHASES")) {   // a library built with -DRXGPU_HNSW_PHASES: shader cycles of the sorted-list search by phase
		DeviceGuard dg(h->device);
		unsigned long long ph[4] = {0, 0, 0, 0};
		RX_HIP(hipMemcpy(ph, h->d_hnsw_stats + 4, sizeof(ph), hipMemcpyDeviceToHost));
		RX_HIP(hipMemset(h->d_hnsw_stats + 4, 0, sizeof(ph)));
		std::fprintf(stderr, "[rxgpu hnsw phases] hops %llu evals %llu | cycles: pop+links+visited %llu  distances %llu  inserts %llu  layer0 total %llu\n", v[1], v[0], ph[0],
					 ph[1], ph[2], ph[3]);
	}
	return RXGPU_OK;
}

int rxgpu_hnsw_read_stats4(rxgpu_index* h, uint64_t* out4) {
	RX_CHECK(h && out4, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_stats4: null argument");
	out4[0] = out4[1] = out4[2] = out4[3] = 0;
	if (h->shard_set || !h->d_hnsw_stats) return RXGPU_OK;
	unsigned long long v[4] = {0, 0, 0, 0};
	if (int rc = take_hnsw_stats(h, 0, 4, v); rc) return rc;
	for (int i = 0; i < 4; ++i) out4[i] = v[i];
	return RXGPU_OK;
}

int rxgpu_hnsw_read_lds_reruns(rxgpu_index* h, uint64_t* reruns) {
	RX_CHECK(h && reruns, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_lds_reruns: null argument");
	if (h->shard_set) return sum_over_shards(h, 1, reruns, [](rxgpu_index* sh, uint64_t* v) { return rxgpu_hnsw_read_lds_reruns(sh, v); });
	*reruns = h->hnsw_lds_reruns.exchange(0);
	return RXGPU_OK;
}

int rxgpu_hnsw_read_tie_reruns(rxgpu_index* h, uint64_t* reruns) {
	RX_CHECK(h && reruns, RXGPU_ERR_PARAMS, "rxgpu_hnsw_read_tie_reruns: null argument");
	if (h->shard_set) return sum_over_shards(h, 1, reruns, [](rxgpu_index* sh, uint64_t* v) { return rxgpu_hnsw_read_tie_reruns(sh, v); });
	*reruns = h->hnsw_tie_reruns.exchange(0);   // queries this library re-ran in a launch of their own ...
	if (h->d_hnsw_stats) {                      // ... and searches that started over on the heaps inside the sorted-list kernel
		unsigned long long v = 0;
		if (int rc = take_hnsw_stats(h, 2, 1, &v); rc) return rc;
		*reruns += v;
	}
	return RXGPU_OK;
}

}  // extern "C"
