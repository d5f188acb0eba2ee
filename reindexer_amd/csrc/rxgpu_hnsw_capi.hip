// C-ABI implementation (include/rxgpu.h), the HNSW host side: the graph mirror and its SQ8 code table, SearchKnn / SearchRange, streaming
// sessions, the search counters.  What a search launches is decided in hnsw_launch_plan.h (no HIP, tested on the CPU) and carried out here;
// the resident kernel behind single queries is rxgpu_hnsw_server.hip.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/rxgpu.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::ProfileScope;
using rxgpu::set_error;

// A streaming KNN session (rxgpu_hnsw_stream_begin)
struct rxgpu_hnsw_stream {
	rxgpu_index* owner = nullptr;
	uint64_t graph_n = 0;
	uint32_t ef = 0;
	hipStream_t stream = nullptr;
	rxgpu_devbuf d_query, d_visited, d_cand, d_top, d_ext, d_state, d_out;
	uint32_t out_cap = 0;
	rxgpu::HnswStreamState host_state{};
	bool empty_graph = false;
	bool sq8 = false;          // the session runs over the SQ8 codes: d_query holds the query's codes
	float qcorr = 0.f, qnorm = 1.f;
};

namespace {

using rxgpu::HnswKnobs;
using rxgpu::HnswLaunchPlan;

// k and ef of a search as the reference defaults them: no more results than rows, ef = 1.5 k where the caller leaves it open, at least 1
void default_k_ef(const rxgpu_index* h, uint32_t& k, uint32_t& ef) {
	k = uint32_t(std::min<uint64_t>(k, h->count));
	if (!ef) ef = k * 3 / 2;                                        // hnswalg.h:1995
	if (!ef) ef = 1;
}

// The graph as the kernels see it: the one place that writes these fields (searches, range searches, streaming sessions) ...
void fill_hnsw_params(const rxgpu_index* h, rxgpu::HnswParams& p) {
	p.rows = h->d_rows;
	p.inv_norms = h->d_inv_norms;
	p.links0 = h->d_links0;
	p.upper_off = h->d_upper_off;
	p.upper = h->d_upper;
	p.deleted = h->d_deleted;
	p.n = h->count;
	p.stride = h->stride;
	p.dim = h->dim;
	p.M = h->graph_M;
	p.maxM0 = h->graph_maxM0;
	p.maxlevel = h->graph_maxlevel;
	p.entry = h->graph_entry;
	p.bare = h->graph_deleted == 0;
}
// ... and the SQ8 code table, for a search over the codes
void fill_sq8_params(const rxgpu_index* h, rxgpu::HnswParams& p) {
	p.codes = h->d_codes;
	p.corr = h->d_corr;
	p.alpha2 = h->sq8_alpha2;
}

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
	static constexpr uint32_t kGroups = 64, kCap = 4096;
	bool held = false;              // this call has the helpers (until the object goes)
	uint32_t* hq_words = nullptr;   // [0] entries appended, [1] stop, [2] searches of the batch that have ended, [16 ..] ids
	uint32_t n = 0;                 // entries appended, once the batch's stream has been waited for
	~HelperBatch() {
		if (held) g_helpers_in_flight.store(false, std::memory_order_release);
	}
	uint32_t queued() const { return std::min<uint32_t>(n, kCap); }
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
	uint32_t nq, k;
	bool sq8;
	const void* queries;         // the caller's block
	float* out_dist;
	uint32_t* out_row;
	uint32_t* out_count;
	const rxgpu::HnswSink* sink;
	bool dev_q = false;          // the queries are float rows in HBM already ([nq][dim]): read where they are, nothing is uploaded
	size_t row_bytes = 0;        // of one query
	rxgpu::HnswParams p{};       // what every launch of the call shares
	const void* d_q = nullptr;   // where the kernels read the queries
	const uint32_t* allowed = nullptr;   // a call under an allowed-rows bitmap: the bitmap in this call's context (HBM), beside p in every launch
	// where counts and lists arrive on the host: the caller's arrays, or the pinned staging buffer
	uint32_t* dl_count = nullptr;
	float* dl_dist = nullptr;
	uint32_t* dl_row = nullptr;
	// Output and query buffers, the early zeroing, the staging buffer, the first upload, and the parameters every launch shares.
	int stage_and_upload(const float* qcorr, const float* qnorm, uint32_t ef) {
		row_bytes = size_t(h->dim) * (sq8 ? sizeof(uint8_t) : sizeof(float));
		if (!dev_q) {   // (queries in HBM are read where they are)
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
		const void* up_queries = queries;
		const float *up_qcorr = qcorr, *up_qnorm = qnorm;
		dl_count = out_count;
		dl_dist = out_dist;
		dl_row = out_row;
		char* zc_dev = nullptr;   // the pinned buffer as the device sees it
		if (pl.staged) {
			if (int rc = c->ensure_pinned(pl.st_end); rc) return rc;
			char* hp = static_cast<char*>(c->h_pinned);
			if (pl.zero_copy) {
				void* dv = nullptr;
				RX_HIP(hipHostGetDevicePointer(&dv, hp, 0));
				zc_dev = static_cast<char*>(dv);
			}
			if (!dev_q) {
				std::memcpy(hp, queries, size_t(nq) * row_bytes);
				up_queries = hp;
			}
			if (sq8) {
				std::memcpy(hp + pl.st_corr, qcorr, size_t(nq) * 4);
				std::memcpy(hp + pl.st_norm, qnorm, size_t(nq) * 4);
				up_qcorr = reinterpret_cast<const float*>(hp + pl.st_corr);
				up_qnorm = reinterpret_cast<const float*>(hp + pl.st_norm);
			}
			dl_count = reinterpret_cast<uint32_t*>(hp + pl.st_count);
			dl_dist = reinterpret_cast<float*>(hp + pl.st_dist);
			dl_row = reinterpret_cast<uint32_t*>(hp + pl.st_row);
		}
		d_q = dev_q ? queries : pl.zero_copy ? static_cast<void*>(zc_dev) : c->d_queries.ptr;
		if (!pl.zero_copy && !dev_q) RX_HIP(hipMemcpyAsync(c->d_queries.ptr, up_queries, size_t(pl.part_q) * row_bytes, hipMemcpyHostToDevice, c->stream));
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
		p.ef = ef;
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
			std::memcpy(out_count, dl_count, size_t(nq) * 4);
			if (!sink) {
				std::memcpy(out_dist, dl_dist, size_t(nq) * k * 4);
				std::memcpy(out_row, dl_row, size_t(nq) * k * 4);
			}
		}
		return RXGPU_OK;
	}
	int to_sink() {   // the finished lists into the exchange's send buffer (sharded HNSW), on this search's stream, drained
		rxgpu::launch_pack_lists(p.out_dist, p.out_row, p.out_count, nq, k, sink->kk, sink->d_dist, sink->d_row, c->stream);
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

	// Every query once, in launches of vis_slots searches; counts (and lists) are on the host when it returns.
	int first_pass(HelperBatch& helpers) {
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
					if (!dev_q) RX_HIP(hipMemcpyAsync(static_cast<char*>(c->d_queries.ptr) + off, static_cast<const char*>(queries) + off, size_t(cnt) * row_bytes, hipMemcpyHostToDevice, st));
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
		if (!sink) {
			if (int rc = fetch_lists(); rc) return rc;
		}
		return wait_stream();
	}

	// One re-run launch train: the searches `ids` of the batch once more with the parameters of `tier`, `slots` of them per launch; their new
	// counts are on the host when it returns.  tier.visited_words is the size of one search's visited set — a hash set the search zeroes itself
	// (tier.vis_hash_log2 != 0) or a bitset zeroed here; tier.gcand_cap != 0: the candidate heaps live in global scratch, that many entries each.
	int rerun(const std::vector<uint32_t>& ids, uint64_t slots, const char* profile_name, const rxgpu::HnswParams& tier) {
		const bool global_cand = tier.gcand_cap != 0;
		if (int rc = c->d_redo.ensure(ids.size() * sizeof(uint32_t)); rc) return rc;
		RX_HIP(hipMemcpyAsync(c->d_redo.ptr, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
		for (size_t r0 = 0; r0 < ids.size(); r0 += slots) {
			const uint32_t cq = uint32_t(std::min<uint64_t>(slots, ids.size() - r0));
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
			ProfileScope ps(h, profile_name, c->stream);
			launch(pc, cq, global_cand, c->stream);
		}
		RX_HIP(hipGetLastError());
		if (int rc = fetch_counts(); rc) return rc;
		RX_HIP(hipStreamSynchronize(c->stream));
		return RXGPU_OK;
	}
	int finish() { return sink ? to_sink() : done_host(); }
};

// One body for both row formats: `queries` are float rows (qcorr == nullptr) or SQ8 codes with their corrective offsets and normCoefs.
// sink (sharded HNSW, rxgpu_sharded.hip): the result lists stay in HBM — packed into the shard's slot of the exchange's send buffer
// ([nq][kk] distances | [nq][kk] local rows, invalid entries past a query's count) instead of travelling to the host; only the counts
// come back (the re-run tiers are driven by them).  The stream is drained before the call returns.
int hnsw_search_impl(rxgpu_index* h, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist,
					 uint32_t* out_row, uint32_t* out_count, const rxgpu::HnswSink* sink = nullptr, bool try_server = true, bool dev_q = false,
					 const uint32_t* allowed = nullptr) {
	// 1. validate and normalise
	const bool sq8 = qcorr != nullptr;
	const bool to_host = sink == nullptr;
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_sq8: not available on a sharded index");
	RX_CHECK(queries && out_count && (sink || (out_dist && out_row)), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: null argument");
	if (nq == 0) return RXGPU_OK;
	if (h->count == 0 || k == 0) {   // hnswalg.h:1989-1991
		RX_CHECK(to_host, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn: an empty shard has no list to send");
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	RX_CHECK(h->graph_attached && h->graph_n == h->count, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn: graph is not attached / out of date");
	default_k_ef(h, k, ef);
	RX_CHECK(ef <= uint32_t(rxgpu::kHnswMaxEf), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_knn: ef must be <= 4096 on the GPU engine");
	const HnswKnobs knobs = rxgpu::read_hnsw_knobs();
	// 2. ONE query, the planner's call: through the mailbox of the index's resident kernel (rxgpu_hnsw_server.hip) — no launch on the path
	if (nq == 1 && to_host && try_server && !allowed) {
		const int served = hnsw_try_server(h, knobs, queries, qcorr, qnorm, k, ef, out_dist, out_row, out_count);
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
	if (nq > 256 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
	const HnswLaunchPlan pl = rxgpu::plan_hnsw_search(h->count, h->dim, h->graph_deleted == 0 && !allowed, nq, k, ef, sq8, to_host,
													  uint64_t(free_b) + c->d_visited.bytes, knobs, allowed != nullptr);
	// 5. staging and the first upload
	HnswCall call{h, c, pl, nq, k, sq8, queries, out_dist, out_row, out_count, sink, dev_q};
	if (int rc = call.stage_and_upload(qcorr, qnorm, ef); rc) return rc;
	if (allowed) {   // the bitmap, once, into this call's context: HnswCall::launch hands it to the first pass and every re-run tier
		const size_t bytes = size_t((h->count + 31) / 32) * sizeof(uint32_t);
		if (int rc = c->d_allowed.ensure(bytes); rc) return rc;
		RX_HIP(hipMemcpyAsync(c->d_allowed.ptr, allowed, bytes, hipMemcpyHostToDevice, c->stream));
		call.allowed = static_cast<const uint32_t*>(c->d_allowed.ptr);
		call.p.bare = 0;   // hidden nodes are traversed like deleted ones (hnswalg.h:1982: the branch with deleted nodes)
	}
	const uint32_t* const counts = call.dl_count;
	std::vector<uint32_t> redo;
	if (pl.big_ef) {
		redo.resize(nq);
		for (uint32_t q = 0; q < nq; ++q) redo[q] = q;
	} else {
		// 6. the first pass
		HelperBatch helpers;
		if (int rc = call.first_pass(helpers); rc) return rc;
		const uint32_t helper_queued = helpers.queued();
		h->hnsw_lds_reruns += helper_queued;
		std::vector<uint32_t> ties;
		bool clean = true;
		for (uint32_t q = 0; q < nq; ++q) {
			if (counts[q] == rxgpu::kHnswTie) ties.push_back(q);
			clean = clean && counts[q] != rxgpu::kHnswTie && counts[q] != rxgpu::kHnswOverflow;
		}
		if (clean) return call.finish();
		// 7. the re-runs that keep the candidate heap in LDS
		if (!ties.empty()) {   // equal keys met in the sorted list: the same queries through the reference's heaps (candidate heap in LDS)
			h->hnsw_tie_reruns += ties.size();
			rxgpu::HnswParams tier = call.p;
			tier.vis_hash_log2 = pl.vis_hash_log2;
			tier.visited_words = pl.vis_words;
			if (int rc = call.rerun(ties, pl.vis_slots, "hnsw_ties", tier); rc) return rc;
		}
		// Queries whose candidate heap outgrew its LDS area — 600 entries for a search that started over inside the sorted-list kernel, 1024 for
		// the heap kernel's first pass: once more on the heap kernel with the largest LDS heap there is and a bitset (a search that filled
		// its hash set lands here too), before the global-heap tiers.  A search with its heap in global scratch takes 5 - 7 ms at 10M x 768
		// (profiles/rd4i_hnsw_10m_*.json: ONE such query was a fifth of a 16 384-query batch), one in LDS about 1 ms.
		std::vector<uint32_t> over;
		for (uint32_t q = 0; q < nq; ++q) {
			if (counts[q] == rxgpu::kHnswOverflow) over.push_back(q);
		}
		const uint32_t first_cap = pl.use_sorted ? pl.sorted_restart_cap : pl.lds_cand_cap;
		if (!over.empty() && first_cap < uint32_t(rxgpu::kHnswCandLds) && !pl.force_global_tiers) {
			rxgpu::HnswParams tier = call.p;
			tier.lds_cand_cap = uint32_t(rxgpu::kHnswCandLds);
			tier.vis_lds_log2 = 0;   // (a search that filled its hash set is among these)
			if (int rc = call.rerun(over, pl.max_slots, "hnsw_redo", tier); rc) return rc;
			// searches the helpers had queued but not finished are in `over` again: counted once
			h->hnsw_lds_reruns += over.size() > helper_queued ? over.size() - helper_queued : 0;
		}
		// ... and what still does not fit: re-run with the heap in global scratch (bounded by one entry per node)
		for (const uint32_t q : over) {
			if (counts[q] == rxgpu::kHnswOverflow) redo.push_back(q);
		}
	}
	// ... and the two tiers with the heap in global scratch (HnswLaunchPlan::tier_cap)
	for (int t = 0; t < 2 && !redo.empty(); ++t) {
		if (t == 1 && pl.tier_cap[1] == pl.tier_cap[0]) break;
		rxgpu::HnswParams tier = call.p;
		tier.gcand_cap = pl.tier_cap[t];
		const uint64_t redo_slots = std::max<uint64_t>(1, std::min<uint64_t>(pl.max_slots, (1ull << 30) / (pl.tier_cap[t] * 8)));
		if (int rc = call.rerun(redo, redo_slots, "hnsw_redo", tier); rc) return rc;
		std::vector<uint32_t> again;
		for (const uint32_t q : redo) {
			if (counts[q] == rxgpu::kHnswOverflow) again.push_back(q);
		}
		redo.swap(again);
	}
	RX_CHECK(redo.empty(), RXGPU_ERR_DEVICE, "rxgpu_hnsw_search_knn: a candidate heap of one entry per node overflowed");
	// 8. the lists: to the caller, or packed into the sink
	if (!to_host) return call.to_sink();
	if (int rc = call.fetch_lists(); rc) return rc;
	RX_HIP(hipStreamSynchronize(c->stream));
	return call.done_host();
}

// ---------------------------------------------------------------------------------------------- SearchRange, expansion on the device
// hnswalg.h:2015-2070: ef-search (the kernels above), then the closure over level-0 links while dist < radius — hnsw_range_kernel, one
// launch whatever the depth of the expansion.  cap too small: RXGPU_ERR_OVERFLOW with *out_total = hits counted so far (a lower bound: the
// expansion stops growing where it cannot store) — the caller retries with more room.
int hnsw_range_impl(rxgpu_index* h, const void* query, const float* qcorr, const float* qnorm, float radius, uint32_t ef, float* out_dist,
						   uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	const bool sq8 = qcorr != nullptr;
	RX_CHECK(h && query && out_total, RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_range: null argument");
	*out_total = 0;
	RX_CHECK(cap == 0 || (out_dist && out_row), RXGPU_ERR_PARAMS, "rxgpu_hnsw_search_range: null argument");
	if (h->count == 0) return RXGPU_OK;
	const uint32_t ef_eff = ef ? ef : 1;
	const uint32_t kk = uint32_t(std::min<uint64_t>(ef_eff, h->count));
	std::vector<float> sd(kk);
	std::vector<uint32_t> sr(kk);
	uint32_t sc = 0;
	if (int rc = hnsw_search_impl(h, query, qcorr, qnorm, 1, kk, ef_eff, sd.data(), sr.data(), &sc); rc) return rc;
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	const uint64_t words = (h->count + 31) / 32;
	const uint64_t room = std::max<uint64_t>(cap, 1);
	const size_t qelem = sq8 ? 1 : 4;
	size_t carve = 0;
	auto take = [&carve](size_t bytes) {
		const size_t at = carve;
		carve = (carve + bytes + 255) & ~size_t(255);
		return at;
	};
	const size_t o_q = take(size_t(h->dim) * qelem + 16), o_qc = take(8), o_sd = take(size_t(kk) * 4), o_sr = take(size_t(kk) * 4),
				 o_front = take(size_t(2) * room * 4), o_total = take(8);
	if (int rc = c->d_misc.ensure(carve); rc) return rc;
	if (int rc = c->d_visited.ensure(words * 4); rc) return rc;
	if (int rc = c->d_out_dist.ensure(room * 4); rc) return rc;
	if (int rc = c->d_out_row.ensure(room * 4); rc) return rc;
	char* mb = static_cast<char*>(c->d_misc.ptr);
	RX_HIP(hipMemcpyAsync(mb + o_q, query, size_t(h->dim) * qelem, hipMemcpyHostToDevice, c->stream));
	if (sq8) {
		const float qc[2] = {*qcorr, *qnorm};
		RX_HIP(hipMemcpyAsync(mb + o_qc, qc, 8, hipMemcpyHostToDevice, c->stream));
	}
	if (sc) {
		RX_HIP(hipMemcpyAsync(mb + o_sd, sd.data(), size_t(sc) * 4, hipMemcpyHostToDevice, c->stream));
		RX_HIP(hipMemcpyAsync(mb + o_sr, sr.data(), size_t(sc) * 4, hipMemcpyHostToDevice, c->stream));
	}
	RX_HIP(hipMemsetAsync(mb + o_total, 0, 8, c->stream));
	RX_HIP(hipMemsetAsync(c->d_visited.ptr, 0, words * 4, c->stream));
	rxgpu::HnswParams p{};
	fill_hnsw_params(h, p);
	p.queries = reinterpret_cast<const float*>(mb + o_q);
	if (sq8) {
		fill_sq8_params(h, p);
		p.qcodes = reinterpret_cast<const uint8_t*>(mb + o_q);
		p.qcorr = reinterpret_cast<const float*>(mb + o_qc);
		p.qnorm = reinterpret_cast<const float*>(mb + o_qc) + 1;
	}
	rxgpu::HnswRange r{};
	r.seed_dist = reinterpret_cast<const float*>(mb + o_sd);
	r.seed_row = reinterpret_cast<const uint32_t*>(mb + o_sr);
	r.seed_n = sc;
	r.radius = radius;
	r.visited = static_cast<uint32_t*>(c->d_visited.ptr);
	r.frontier = reinterpret_cast<uint32_t*>(mb + o_front);
	r.out_dist = static_cast<float*>(c->d_out_dist.ptr);
	r.out_row = static_cast<uint32_t*>(c->d_out_row.ptr);
	r.total = reinterpret_cast<unsigned long long*>(mb + o_total);
	r.cap = cap;
	{
		ProfileScope ps(h, "hnsw_range", c->stream);
		rxgpu::launch_hnsw_range(h->metric, p, r, c->stream);
	}
	RX_HIP(hipGetLastError());
	unsigned long long total = 0;
	RX_HIP(hipMemcpyAsync(&total, mb + o_total, 8, hipMemcpyDeviceToHost, c->stream));
	RX_HIP(hipStreamSynchronize(c->stream));
	*out_total = total;
	const uint64_t have = std::min<uint64_t>(total, cap);
	if (have) {
		RX_HIP(hipMemcpyAsync(out_dist, c->d_out_dist.ptr, have * 4, hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipMemcpyAsync(out_row, c->d_out_row.ptr, have * 4, hipMemcpyDeviceToHost, c->stream));
		RX_HIP(hipStreamSynchronize(c->stream));
	}
	RX_CHECK(total <= cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_search_range: more hits than the output buffer holds");
	return RXGPU_OK;
}

void fill_stream(const rxgpu_hnsw_stream* s, rxgpu::HnswStream& d) {
	const uint64_t cap = s->graph_n;
	d.query = static_cast<const float*>(s->d_query.ptr);
	d.qcodes = s->sq8 ? static_cast<const uint8_t*>(s->d_query.ptr) : nullptr;
	d.qcorr = s->qcorr;
	d.qnorm = s->qnorm;
	d.visited = static_cast<uint32_t*>(s->d_visited.ptr);
	d.cand_d = static_cast<float*>(s->d_cand.ptr);
	d.cand_i = reinterpret_cast<uint32_t*>(d.cand_d + cap);
	d.top_d = static_cast<float*>(s->d_top.ptr);
	d.top_i = reinterpret_cast<uint32_t*>(d.top_d + 2 * cap);
	d.ext_d = static_cast<float*>(s->d_ext.ptr);
	d.ext_i = reinterpret_cast<uint32_t*>(d.ext_d + 2 * cap);
	d.cap = uint32_t(cap);
	d.ef = s->ef;
	d.state = static_cast<rxgpu::HnswStreamState*>(s->d_state.ptr);
	d.out_dist = static_cast<float*>(s->d_out.ptr);
	d.out_row = reinterpret_cast<uint32_t*>(d.out_dist + s->out_cap);
}

int hnsw_stream_begin_impl(rxgpu_index* h, const void* query, bool sq8, float qcorr, float qnorm, uint32_t ef, rxgpu_hnsw_stream** out) {
	RX_CHECK(h && query && out, RXGPU_ERR_PARAMS, "rxgpu_hnsw_stream_begin: null argument");
	*out = nullptr;
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_stream_begin: streaming sessions are per graph — not available on a sharded index");
	RX_CHECK(!sq8 || h->count == 0 || (h->d_codes && h->sq8_n == h->count), RXGPU_ERR_LOGIC,
			 "rxgpu_hnsw_stream_begin_sq8: SQ8 codes are not attached / out of date");
	DeviceGuard dg(h->device);
	auto* s = new rxgpu_hnsw_stream();
	s->owner = h;
	s->ef = ef ? ef : 100;   // kDefaultStreamingEf (hnswalg.h:1867)
	s->sq8 = sq8;
	s->qcorr = qcorr;
	s->qnorm = qnorm;
	s->graph_n = h->count;
	if (h->count == 0) {     // hnswalg.h:1880-1882: an empty graph yields a session that is exhausted at once
		s->empty_graph = true;
		*out = s;
		return RXGPU_OK;
	}
	struct Guard {
		rxgpu_hnsw_stream* s;
		~Guard() {
			if (s) rxgpu_hnsw_stream_end(s);
		}
	} guard{s};
	RX_CHECK(h->graph_attached && h->graph_n == h->count, RXGPU_ERR_LOGIC, "rxgpu_hnsw_stream_begin: graph is not attached / out of date");
	RX_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
	const uint64_t cap = h->count, words = (h->count + 31) / 32;
	const size_t qbytes = size_t(h->dim) * (sq8 ? 1 : 4);
	if (int rc = s->d_query.ensure(size_t(h->dim) * 4); rc) return rc;
	if (int rc = s->d_visited.ensure(words * 4); rc) return rc;
	if (int rc = s->d_cand.ensure(cap * 8); rc) return rc;
	if (int rc = s->d_top.ensure(cap * 16); rc) return rc;
	if (int rc = s->d_ext.ensure(cap * 16); rc) return rc;
	if (int rc = s->d_state.ensure(sizeof(rxgpu::HnswStreamState)); rc) return rc;
	RX_HIP(hipMemcpyAsync(s->d_query.ptr, query, qbytes, hipMemcpyHostToDevice, s->stream));
	RX_HIP(hipMemsetAsync(s->d_visited.ptr, 0, words * 4, s->stream));
	rxgpu::HnswParams p{};
	fill_hnsw_params(h, p);
	if (s->sq8) fill_sq8_params(h, p);
	rxgpu::HnswStream d{};
	fill_stream(s, d);
	rxgpu::launch_hnsw_stream(h->metric, p, d, 0, rxgpu::kStreamBegin, false, s->stream);
	RX_HIP(hipGetLastError());
	RX_HIP(hipMemcpyAsync(&s->host_state, s->d_state.ptr, sizeof(s->host_state), hipMemcpyDeviceToHost, s->stream));
	RX_HIP(hipStreamSynchronize(s->stream));
	guard.s = nullptr;
	*out = s;
	return RXGPU_OK;
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

}  // namespace

namespace rxgpu {
int hnsw_search_to_sink(rxgpu_index* shard, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, const HnswSink& sink) {
	std::vector<uint32_t> counts(nq);
	RX_CHECK(!qcorr || (shard->d_codes && shard->sq8_n == shard->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_knn_sq8: SQ8 codes are not attached / out of date on a shard");
	return hnsw_search_impl(shard, queries, qcorr, qnorm, nq, k, ef, nullptr, nullptr, counts.data(), &sink);
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
	return hnsw_search_impl(h, d_queries, nullptr, nullptr, nq, k, ef, nullptr, nullptr, counts.data(), &sink, false, true);
}
}  // namespace rxgpu

extern "C" {

/* ------------------------------------------------------------------------------------------------ graph mirror, SQ8 code table */

int rxgpu_hnsw_attach_graph(rxgpu_index* h, const uint32_t* links0, const uint64_t* upper_off, const uint32_t* upper, uint64_t upper_blocks,
							const uint8_t* deleted, uint32_t M, uint32_t max_m0, int32_t maxlevel, uint32_t entry, uint64_t num_deleted) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_attach_graph: a sharded index holds one graph per shard — attach to the rxgpu_index_shard(h, s) handles");
	const uint64_t n = h->count;
	RX_CHECK(n == 0 || (links0 && upper_off && deleted), RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: null argument");
	RX_CHECK(upper_blocks == 0 || upper, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: upper is null");
	RX_CHECK(M >= 1 && max_m0 <= uint32_t(rxgpu::kHnswMaxNeighbors) && M <= max_m0, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_attach_graph: the GPU engine supports M <= 64 (2*M <= 128)");
	RX_CHECK(n == 0 || entry < n, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_graph: entry point out of range");
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	// allocated for the index CAPACITY (and with headroom for upper-level blocks), so that rxgpu_hnsw_patch_graph can grow the graph in place
	auto replace = [&](auto*& dst, const void* src, size_t bytes, size_t cap_bytes) -> int {
		if (dst) (void)hipFree(dst);
		dst = nullptr;
		if (cap_bytes == 0) return RXGPU_OK;
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&dst), cap_bytes));
		if (bytes) RX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
		return RXGPU_OK;
	};
	h->graph_attached = false;
	const uint64_t rows_cap = std::max<uint64_t>(std::max<uint64_t>(h->capacity, n), 1);
	// expected upper blocks of a full index: sum over levels of cap / M^level = cap / (M - 1); twice that (and at least what is there) as headroom
	uint64_t upper_cap = std::max<uint64_t>(2 * upper_blocks + 64, 2 * rows_cap / std::max<uint32_t>(M - 1, 1) + 64);
	// RXGPU_HNSW_UPPER_HEADROOM=<blocks> (read per attach; tests): that many blocks beyond the attached ones instead — the way to meet
	// RXGPU_ERR_OVERFLOW of the patch entry points, which the default headroom keeps out of reach
	if (const char* e = std::getenv("RXGPU_HNSW_UPPER_HEADROOM"); e && *e) {
		char* end = nullptr;
		const unsigned long long x = std::strtoull(e, &end, 10);
		if (end != e && *end == 0 && x > 0) upper_cap = upper_blocks + x;
	}
	const size_t row_bytes = (1 + size_t(max_m0)) * sizeof(uint32_t), blk_bytes = (1 + size_t(M)) * sizeof(uint32_t);
	if (int rc = replace(h->d_links0, links0, n * row_bytes, rows_cap * row_bytes); rc) return rc;
	if (int rc = replace(h->d_upper_off, upper_off, n ? (n + 1) * sizeof(uint64_t) : 0, (rows_cap + 1) * sizeof(uint64_t)); rc) return rc;
	if (int rc = replace(h->d_upper, upper, upper_blocks * blk_bytes, upper_cap * blk_bytes); rc) return rc;
	if (int rc = replace(h->d_deleted, deleted, n, rows_cap); rc) return rc;
	h->graph_rows_cap = rows_cap;
	h->graph_upper_cap = upper_cap;
	h->graph_upper_used = upper_blocks;
	if (!h->d_hnsw_stats) {
		RX_HIP(hipMalloc(reinterpret_cast<void**>(&h->d_hnsw_stats), 8 * sizeof(unsigned long long)));   // evals, hops, in-kernel restarts, spare, [4..7] phase cycles (RXGPU_HNSW_PHASES builds)
		RX_HIP(hipMemset(h->d_hnsw_stats, 0, 8 * sizeof(unsigned long long)));
	}
	h->graph_n = n;
	h->graph_upper_nodes = n;
	h->build_upper_end = 0;   // level-1 lists of a build batch that were not patched in are gone with the arrays
	h->graph_M = M;
	h->graph_maxM0 = max_m0;
	h->graph_maxlevel = maxlevel;
	h->graph_entry = entry;
	h->graph_deleted = num_deleted;
	h->graph_attached = true;
	return RXGPU_OK;
}

int rxgpu_hnsw_patch_graph(rxgpu_index* h, uint32_t n_dirty, const uint32_t* dirty_ids, const uint32_t* links0_rows, const uint8_t* deleted_flags,
						   const int32_t* levels, const uint32_t* upper_rows, int32_t maxlevel, uint32_t entry, uint64_t num_deleted) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_graph: no graph attached");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel reads what changes here
	RX_CHECK(n_dirty == 0 || (dirty_ids && links0_rows && deleted_flags && levels), RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: null argument");
	const uint64_t n_new = h->count;   // the rows were uploaded first (rxgpu_index_upload_rows)
	RX_CHECK(n_new >= h->graph_n, RXGPU_ERR_LOGIC, "rxgpu_hnsw_patch_graph: the index shrank under the graph");
	RX_CHECK(n_new == 0 || entry < n_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: entry point out of range");
	RX_CHECK(n_new <= h->graph_rows_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_patch_graph: the graph arrays were allocated for fewer rows (re-attach the graph)");
	// staging: ids, per-node upper placement, lists — one buffer, one upload, one scatter launch
	const uint32_t M = h->graph_M, max_m0 = h->graph_maxM0;
	const size_t stride0 = 1 + size_t(max_m0), stride = 1 + size_t(M);
	std::vector<uint64_t> upper_at(n_dirty);
	std::vector<uint32_t> upper_src(n_dirty);
	uint64_t used = h->graph_upper_used, staged_blocks = 0, next_new = h->graph_n;
	for (uint32_t j = 0; j < n_dirty; ++j) {
		RX_CHECK(dirty_ids[j] < n_new && levels[j] >= 0, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: node id / level out of range");
		upper_src[j] = uint32_t(staged_blocks);
		staged_blocks += uint64_t(levels[j]);
		if (dirty_ids[j] >= h->graph_n) {   // a new node: ids ascending, every one of them listed (its blocks are appended in id order)
			RX_CHECK(dirty_ids[j] == next_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: new nodes must be listed in ascending id order, none skipped");
			++next_new;
			upper_at[j] = used;
			used += uint64_t(levels[j]);
		} else {
			upper_at[j] = ~uint64_t(0);
		}
	}
	RX_CHECK(next_new == n_new, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: every new node must be listed");
	RX_CHECK(staged_blocks == 0 || upper_rows, RXGPU_ERR_PARAMS, "rxgpu_hnsw_patch_graph: upper_rows is null");
	RX_CHECK(used <= h->graph_upper_cap, RXGPU_ERR_OVERFLOW, "rxgpu_hnsw_patch_graph: upper-level storage exhausted (re-attach the graph)");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	RX_HIP(rxgpu::device_wait_all(h->device));   // no search may be reading the lists while they change (the Map calls this under its writer lock)
	auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
	const size_t o_ids = 0, o_at = al(o_ids + size_t(n_dirty) * 4), o_src = al(o_at + size_t(n_dirty) * 8), o_lv = al(o_src + size_t(n_dirty) * 4),
				 o_l0 = al(o_lv + size_t(n_dirty) * 4), o_up = al(o_l0 + size_t(n_dirty) * stride0 * 4), o_del = al(o_up + staged_blocks * stride * 4),
				 total = al(o_del + n_dirty);
	if (n_dirty) {
		if (int rc = c->d_misc.ensure(total); rc) return rc;
		if (int rc = c->ensure_pinned(total); rc) return rc;
		char* hp = static_cast<char*>(c->h_pinned);
		std::memcpy(hp + o_ids, dirty_ids, size_t(n_dirty) * 4);
		std::memcpy(hp + o_at, upper_at.data(), size_t(n_dirty) * 8);
		std::memcpy(hp + o_src, upper_src.data(), size_t(n_dirty) * 4);
		std::memcpy(hp + o_lv, levels, size_t(n_dirty) * 4);
		std::memcpy(hp + o_l0, links0_rows, size_t(n_dirty) * stride0 * 4);
		if (staged_blocks) std::memcpy(hp + o_up, upper_rows, staged_blocks * stride * 4);
		std::memcpy(hp + o_del, deleted_flags, n_dirty);
		char* db = static_cast<char*>(c->d_misc.ptr);
		RX_HIP(hipMemcpyAsync(db, hp, total, hipMemcpyHostToDevice, c->stream));
		rxgpu::HnswPatch p{};
		p.ids = reinterpret_cast<const uint32_t*>(db + o_ids);
		p.upper_at = reinterpret_cast<const uint64_t*>(db + o_at);
		p.upper_src = reinterpret_cast<const uint32_t*>(db + o_src);
		p.levels = reinterpret_cast<const int32_t*>(db + o_lv);
		p.src_links0 = reinterpret_cast<const uint32_t*>(db + o_l0);
		p.src_upper = reinterpret_cast<const uint32_t*>(db + o_up);
		p.src_deleted = reinterpret_cast<const uint8_t*>(db + o_del);
		p.links0 = h->d_links0;
		p.upper_off = h->d_upper_off;
		p.upper = h->d_upper;
		p.deleted = h->d_deleted;
		p.M = M;
		p.maxM0 = max_m0;
		rxgpu::launch_hnsw_patch(p, n_dirty, c->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipStreamSynchronize(c->stream));
	}
	h->graph_upper_used = used;
	h->graph_n = n_new;
	h->graph_upper_nodes = n_new;
	h->build_upper_end = 0;
	h->graph_maxlevel = maxlevel;
	h->graph_entry = entry;
	h->graph_deleted = num_deleted;
	return RXGPU_OK;
}

int rxgpu_hnsw_update_deleted(rxgpu_index* h, const uint8_t* deleted, uint64_t num_deleted) {
	RX_CHECK(h && h->graph_attached, RXGPU_ERR_LOGIC, "rxgpu_hnsw_update_deleted: no graph attached");
	RX_CHECK(deleted || h->graph_n == 0, RXGPU_ERR_PARAMS, "rxgpu_hnsw_update_deleted: null argument");
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	if (h->graph_n) RX_HIP(hipMemcpy(h->d_deleted, deleted, h->graph_n, hipMemcpyHostToDevice));
	h->graph_deleted = num_deleted;
	return RXGPU_OK;
}

namespace {
// The code table of h with room for `rows` rows (the three entry points that write it come through here).  It is allocated for the index
// CAPACITY, like the float rows; where it has to grow — the first rows, or the index was reserved larger since — the rows that have codes
// are copied into the new one.  + 4 bytes: the word loads of the last row's last block stay inside the allocation whatever dim % 4 is.
// The caller has quiesced the resident kernel and holds the device.
int sq8_table_ensure(rxgpu_index* h, uint64_t rows, const char* who) {
	if (h->sq8_cap >= rows) return RXGPU_OK;
	const uint64_t cap = std::max<uint64_t>(h->capacity, h->count);
	RX_HIP(rxgpu::device_wait_all(h->device));
	uint8_t* nc = nullptr;
	float* nr = nullptr;
	RX_HIP(hipMalloc(reinterpret_cast<void**>(&nc), size_t(cap) * h->dim + 4));
	if (hipMalloc(reinterpret_cast<void**>(&nr), size_t(cap) * sizeof(float)) != hipSuccess) {
		(void)hipFree(nc);
		set_error(std::string(who) + ": not enough memory for the corrective offsets");
		return RXGPU_ERR_NOMEM;
	}
	if (h->sq8_n) {
		RX_HIP(hipMemcpy(nc, h->d_codes, size_t(h->sq8_n) * h->dim, hipMemcpyDeviceToDevice));
		RX_HIP(hipMemcpy(nr, h->d_corr, size_t(h->sq8_n) * sizeof(float), hipMemcpyDeviceToDevice));
	}
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_corr) (void)hipFree(h->d_corr);
	h->d_codes = nc;
	h->d_corr = nr;
	h->sq8_cap = cap;
	return RXGPU_OK;
}
}  // namespace

// Rows [first_row, first_row + n) of the code table: the device side of a point added to / updated in a quantised graph (addPoint with a
// quantizer, hnswalg.h:1480-1495).  The table is allocated for the index CAPACITY (like the rows), so an upsert is a copy of its own D + 4
// bytes, not a re-upload of the table.
int rxgpu_hnsw_upload_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const uint8_t* codes, const float* corr, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_upload_sq8_rows: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(codes && corr, RXGPU_ERR_PARAMS, "rxgpu_hnsw_upload_sq8_rows: null argument");
	RX_CHECK(first_row <= h->sq8_n && first_row + n <= h->count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_upload_sq8_rows: rows follow the table without a hole and stay below count");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads what changes (or moves) here
	DeviceGuard dg(h->device);
	if (int rc = sq8_table_ensure(h, first_row + n, "rxgpu_hnsw_upload_sq8_rows"); rc) return rc;
	RX_HIP(hipMemcpy(h->d_codes + size_t(first_row) * h->dim, codes, size_t(n) * h->dim, hipMemcpyHostToDevice));
	RX_HIP(hipMemcpy(h->d_corr + first_row, corr, size_t(n) * sizeof(float), hipMemcpyHostToDevice));
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = std::max<uint64_t>(h->sq8_n, first_row + n);
	return RXGPU_OK;
}

int rxgpu_hnsw_attach_sq8(rxgpu_index* h, const uint8_t* codes, const float* corr, uint64_t count, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_attach_sq8: not available on a sharded index");
	RX_CHECK(count == h->count, RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_sq8: one code row per index row");
	RX_CHECK(count == 0 || (codes && corr), RXGPU_ERR_PARAMS, "rxgpu_hnsw_attach_sq8: null argument");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads the tables freed below
	DeviceGuard dg(h->device);
	RX_HIP(rxgpu::device_wait_all(h->device));
	if (h->d_codes) (void)hipFree(h->d_codes);
	if (h->d_corr) (void)hipFree(h->d_corr);
	h->d_codes = nullptr;
	h->d_corr = nullptr;
	h->sq8_n = 0;
	h->sq8_cap = 0;
	if (count) {
		// a fresh table, sized by the index capacity: rows added later are patched in (rxgpu_hnsw_upload_sq8_rows / rxgpu_hnsw_quantize_sq8)
		if (int rc = sq8_table_ensure(h, count, "rxgpu_hnsw_attach_sq8"); rc) return rc;
		RX_HIP(hipMemcpy(h->d_codes, codes, size_t(count) * h->dim, hipMemcpyHostToDevice));
		RX_HIP(hipMemcpy(h->d_corr, corr, size_t(count) * sizeof(float), hipMemcpyHostToDevice));
	}
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = count;
	return RXGPU_OK;
}

// Quantizer::quantize where the rows are (hnsw_sq8_quantize.hip): what the Map used to compute on one host thread and upload — on the first
// Quantize, on every re-quantisation, after every bulk change — is one pass over rows the device already holds.
int rxgpu_hnsw_quantize_sq8(rxgpu_index* h, uint64_t first_row, uint64_t n, float min_q, float alpha, float delta, float alpha_2) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_quantize_sq8: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(first_row <= h->sq8_n && first_row <= h->count && n <= h->count - first_row, RXGPU_ERR_PARAMS,
			 "rxgpu_hnsw_quantize_sq8: rows follow the table without a hole and stay below count");
	rxgpu::hnsw_server_quiesce(h);   // the resident search kernel over the codes reads what changes (or moves) here
	DeviceGuard dg(h->device);
	if (int rc = sq8_table_ensure(h, first_row + n, "rxgpu_hnsw_quantize_sq8"); rc) return rc;
	hipEvent_t a = nullptr, b = nullptr;
	RX_HIP(hipEventCreate(&a));
	if (hipError_t e = hipEventCreate(&b); e != hipSuccess) {
		(void)hipEventDestroy(a);
		RX_HIP(e);
	}
	float ms = 0.f;
	hipError_t e = hipEventRecord(a, nullptr);
	if (e == hipSuccess) {
		rxgpu::launch_hnsw_sq8_quantize(h->metric, h->d_rows, h->stride, h->dim, first_row, n, min_q, alpha, delta, h->d_codes, h->d_corr, nullptr);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipEventRecord(b, nullptr);
	if (e == hipSuccess) e = hipEventSynchronize(b);
	if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	RX_HIP(e);
	h->sq8_alpha2 = alpha_2;
	h->sq8_n = std::min<uint64_t>(h->count, std::max<uint64_t>(h->sq8_n, first_row + n));   // codes behind a count that shrank since are no rows
	h->sq8_dev_rows += n;
	h->sq8_dev_launches += 1;
	h->sq8_dev_ms += double(ms);
	return RXGPU_OK;
}

int rxgpu_hnsw_read_sq8_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, uint8_t* out_codes, float* out_corr) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_sq8_rows: not available on a sharded index");
	if (n == 0) return RXGPU_OK;
	RX_CHECK(first_row <= h->sq8_n && n <= h->sq8_n - first_row, RXGPU_ERR_LOGIC, "rxgpu_hnsw_read_sq8_rows: rows without codes");
	rxgpu::hnsw_server_quiesce(h);   // a copy on the default stream would wait for the resident kernel's lifetime
	DeviceGuard dg(h->device);
	if (out_codes) RX_HIP(hipMemcpy(out_codes, h->d_codes + size_t(first_row) * h->dim, size_t(n) * h->dim, hipMemcpyDeviceToHost));
	if (out_corr) RX_HIP(hipMemcpy(out_corr, h->d_corr + first_row, size_t(n) * sizeof(float), hipMemcpyDeviceToHost));
	return RXGPU_OK;
}

int rxgpu_hnsw_read_sq8_quantize_stats(rxgpu_index* h, uint64_t* rows, uint64_t* launches, double* kernel_ms) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (rows) *rows = h->sq8_dev_rows;
	if (launches) *launches = h->sq8_dev_launches;
	if (kernel_ms) *kernel_ms = h->sq8_dev_ms;
	h->sq8_dev_rows = 0;
	h->sq8_dev_launches = 0;
	h->sq8_dev_ms = 0.0;
	return RXGPU_OK;
}

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
		const int r2 = hnsw_search_impl(h, query, qcorr, qnorm, 1, k, ef, out_dist, out_row, out_count, nullptr, false);
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
	return hnsw_search_impl(h, queries, nullptr, nullptr, nq, k, ef, out_dist, out_row, out_count);
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
	return hnsw_search_impl(h, query_codes, query_corr, query_norm_coef, nq, k, ef, out_dist, out_row, out_count);
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
	// nothing hidden at all: the reference would take its bare-bone branch — the unfiltered path answers, and nothing else
	if (h->graph_deleted == 0 && set == h->count) return hnsw_search_impl(h, queries, qcorr, qnorm, nq, k, ef, out_dist, out_row, out_count);
	return hnsw_search_impl(h, queries, qcorr, qnorm, nq, k, ef, out_dist, out_row, out_count, nullptr, false, false, allowed_words);
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

/* ------------------------------------------------------------------------------------------------ SearchRange */

int rxgpu_hnsw_search_range(rxgpu_index* h, const float* query, float radius, uint32_t ef, float* out_dist, uint32_t* out_row, uint64_t cap,
							uint64_t* out_total) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	if (h->shard_set) return rxgpu::sharded_hnsw_search_range(h, query, radius, ef, out_dist, out_row, cap, out_total);
	RX_CHECK(h->count == 0 || (h->graph_attached && h->graph_n == h->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_range: graph is not attached / out of date");
	return hnsw_range_impl(h, query, nullptr, nullptr, radius, ef, out_dist, out_row, cap, out_total);
}

int rxgpu_hnsw_search_range_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, float radius, uint32_t ef,
								float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null index");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_range_sq8: not available on a sharded index");
	RX_CHECK(h->count == 0 || (h->graph_attached && h->graph_n == h->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_range_sq8: graph is not attached / out of date");
	RX_CHECK(h->count == 0 || (h->d_codes && h->sq8_n == h->count), RXGPU_ERR_LOGIC, "rxgpu_hnsw_search_range_sq8: SQ8 codes are not attached / out of date");
	return hnsw_range_impl(h, query_codes, &query_corr, &query_norm_coef, radius, ef, out_dist, out_row, cap, out_total);
}

/* ------------------------------------------------------------------------------------------------ streaming KNN sessions */

void rxgpu_hnsw_stream_end(rxgpu_hnsw_stream* s) {
	if (!s) return;
	DeviceGuard dg(s->owner->device);
	if (s->stream) {
		(void)hipStreamSynchronize(s->stream);
		(void)hipStreamDestroy(s->stream);
	}
	for (rxgpu_devbuf* b : {&s->d_query, &s->d_visited, &s->d_cand, &s->d_top, &s->d_ext, &s->d_state, &s->d_out}) b->release();
	delete s;
}

int rxgpu_hnsw_stream_begin(rxgpu_index* h, const float* query, uint32_t ef, rxgpu_hnsw_stream** out) {
	return hnsw_stream_begin_impl(h, query, false, 0.f, 1.f, ef, out);
}

// The same session over a quantised graph (HierarchicalNSWImpl<uint8_t>): the query as prepareData leaves it (codes + corrective offset),
// every distance scaled by its normCoef — BeginStreamingSearch / ContinueStreamingSearch (hnswalg.h:1865-1975) instantiated for uint8_t.
int rxgpu_hnsw_stream_begin_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t ef, rxgpu_hnsw_stream** out) {
	return hnsw_stream_begin_impl(h, query_codes, true, query_corr, query_norm_coef, ef, out);
}

int rxgpu_hnsw_stream_continue(rxgpu_hnsw_stream* s, uint32_t batch, float* out_dist, uint32_t* out_row, uint32_t* out_count, int32_t* exhausted) {
	RX_CHECK(s && out_count && exhausted, RXGPU_ERR_PARAMS, "rxgpu_hnsw_stream_continue: null argument");
	*out_count = 0;
	*exhausted = 0;
	if (batch == 0) return RXGPU_OK;   // hnswalg.h:1956-1958
	if (s->empty_graph) {
		*exhausted = 1;
		return RXGPU_OK;
	}
	RX_CHECK(out_dist && out_row, RXGPU_ERR_PARAMS, "rxgpu_hnsw_stream_continue: null argument");
	rxgpu_index* h = s->owner;
	// the whole session must run under the caller's read lock (hnsw_interface.h:99): a mutated graph invalidates it
	RX_CHECK(h->graph_attached && h->graph_n == s->graph_n && h->count == s->graph_n, RXGPU_ERR_LOGIC,
			 "rxgpu_hnsw_stream_continue: the graph changed under the session");
	DeviceGuard dg(h->device);
	const uint32_t out_need = uint32_t(std::min<uint64_t>(batch, s->graph_n));
	if (out_need > s->out_cap) {
		if (int rc = s->d_out.ensure(size_t(out_need) * 8); rc) return rc;
		s->out_cap = out_need;
	}
	rxgpu::HnswParams p{};
	fill_hnsw_params(h, p);
	if (s->sq8) fill_sq8_params(h, p);
	rxgpu::HnswStream d{};
	fill_stream(s, d);
	const rxgpu::HnswStreamState& hs = s->host_state;
	const uint32_t ef_eff = std::max(s->ef, batch);
	bool lds = ef_eff <= uint32_t(rxgpu::kStreamLdsTop) && uint32_t(hs.top_n) <= uint32_t(rxgpu::kStreamLdsTop) &&
			   uint32_t(hs.ext_n) <= uint32_t(rxgpu::kStreamLdsExt) && uint32_t(hs.cand_n) + h->graph_maxM0 <= uint32_t(rxgpu::kStreamLdsCand);
	if (getenv("RXGPU_HNSW_STREAM_GLOBAL")) lds = false;   // test hook: run every call with the heaps in HBM
	int mode = rxgpu::kStreamContinue;
	for (int attempt = 0; attempt < 2; ++attempt) {
		ProfileScope ps(h, lds ? "hnsw_stream" : "hnsw_stream_global", s->stream);
		rxgpu::launch_hnsw_stream(h->metric, p, d, batch, mode, lds, s->stream);
		RX_HIP(hipGetLastError());
		RX_HIP(hipMemcpyAsync(&s->host_state, s->d_state.ptr, sizeof(s->host_state), hipMemcpyDeviceToHost, s->stream));
		RX_HIP(hipStreamSynchronize(s->stream));
		if (s->host_state.status != rxgpu::kStreamNeedGlobal) break;
		RX_CHECK(lds, RXGPU_ERR_DEVICE, "rxgpu_hnsw_stream_continue: global-heap pass asked for more room");
		lds = false;                       // outgrew LDS at a step boundary: same call, heaps in HBM, no second mergeExtras
		mode = rxgpu::kStreamResume;
	}
	RX_CHECK(s->host_state.status == rxgpu::kStreamOk, RXGPU_ERR_DEVICE, "rxgpu_hnsw_stream_continue: device-side session error");
	const uint32_t n = s->host_state.out_count;
	if (n) {
		RX_HIP(hipMemcpyAsync(out_dist, d.out_dist, size_t(n) * 4, hipMemcpyDeviceToHost, s->stream));
		RX_HIP(hipMemcpyAsync(out_row, d.out_row, size_t(n) * 4, hipMemcpyDeviceToHost, s->stream));
		RX_HIP(hipStreamSynchronize(s->stream));
	}
	*out_count = n;
	*exhausted = s->host_state.exhausted ? 1 : 0;
	return RXGPU_OK;
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
