// What the units of the HNSW host path share — rxgpu_hnsw_graph.hip (graph mirror, SQ8 code table), rxgpu_hnsw_search.hip (SearchKnn, the
// search counters), rxgpu_hnsw_sessions.hip (SearchRange, streaming sessions) — and nothing else.  What other units call is in rxgpu_internal.h.
#pragma once

#include <algorithm>

#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

// One call of hnsw_search_impl.  `queries` are float rows (qcorr == nullptr) or SQ8 codes with their corrective offsets and normCoefs.
struct HnswRequest {
	const void* queries = nullptr;
	const float* qcorr = nullptr;
	const float* qnorm = nullptr;
	uint32_t nq = 0, k = 0, ef = 0;
	float* out_dist = nullptr;
	uint32_t* out_row = nullptr;
	uint32_t* out_count = nullptr;
	// sharded HNSW (rxgpu_sharded.hip): the result lists stay in HBM — packed into the shard's slot of the exchange's send buffer
	// ([nq][kk] distances | [nq][kk] local rows, invalid entries past a query's count) instead of travelling to the host; only the counts
	// come back (the re-run tiers are driven by them)
	const HnswSink* sink = nullptr;
	bool try_server = true;              // a single query is offered to the mailbox of the index's resident kernel first
	bool dev_q = false;                  // the queries are float rows in HBM already ([nq][dim]): read where they are, nothing is uploaded
	const uint32_t* allowed = nullptr;   // the call's allowed-rows bitmap (host, ceil(count / 32) words), null: none
};
// One body for both row formats and every caller.  The stream is drained before the call returns.
int hnsw_search_impl(::rxgpu_index* h, const HnswRequest& rq);

// k and ef of a search as the reference defaults them: no more results than rows, ef = 1.5 k where the caller leaves it open, at least 1
inline void default_k_ef(const ::rxgpu_index* h, uint32_t& k, uint32_t& ef) {
	k = uint32_t(std::min<uint64_t>(k, h->count));
	if (!ef) ef = k * 3 / 2;                                        // hnswalg.h:1995
	if (!ef) ef = 1;
}

// The graph as the kernels see it: the one place that writes these fields (searches, range searches, streaming sessions) ...
inline void fill_hnsw_params(const ::rxgpu_index* h, HnswParams& p) {
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
inline void fill_sq8_params(const ::rxgpu_index* h, HnswParams& p) {
	p.codes = h->d_codes;
	p.corr = h->d_corr;
	p.alpha2 = h->sq8_alpha2;
}

}  // namespace rxgpu
