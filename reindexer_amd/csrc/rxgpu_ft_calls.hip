// The merge entry points of the C-ABI (rxgpu_ft_merge_*_raw, rxgpu_ft_merge_*_resident): what they share, then the calls; a merge itself is
// rxgpu_ft_merge.hip's.  rxgpu_ft_merge_batch_raw runs Q plain merges as ONE launch train.
#include <algorithm>
#include <cstring>

#include "rxgpu_ft_internal.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

namespace {
// ---------------------------------------------------------------------------------------------------- what the entry points share
// The common head of a merge call: the configuration fits the index, the index has its documents
int check_merge_head(const rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const char* who) {
	RX_CHECK(cfg->num_fields == h->num_fields, RXGPU_ERR_PARAMS, std::string(who) + ": field count mismatch");
	RX_CHECK(h->total_docs > 0, RXGPU_ERR_LOGIC, std::string(who) + ": rxgpu_ft_set_docs was not called");
	return RXGPU_OK;
}

// The terms of a query given as arrays; the classification is QueryMergeData::Empty() / Simple() (querymergedata.h:208; ft_merge_plan.h)
int query_terms(const char* who, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts, const int32_t* phrase_num, const int32_t* distance,
				const uint32_t* sub_off, const uint32_t* word_ids, const float* procs, std::vector<QueryTermIn>& terms, bool* empty, bool* simple) {
	*empty = true;
	*simple = false;
	if (nterms == 0) return RXGPU_OK;
	RX_CHECK(ops && opts && sub_off, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	RX_CHECK(nterms < 0x7FFF, RXGPU_ERR_PARAMS, std::string(who) + ": too many terms");
	RX_CHECK(sub_off[nterms] == 0 || (word_ids && procs), RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	terms.resize(nterms);
	for (uint32_t t = 0; t < nterms; ++t) {
		RX_CHECK(ops[t] >= 1 && ops[t] <= 3, RXGPU_ERR_PARAMS, std::string(who) + ": op must be 1 (OR), 2 (AND) or 3 (NOT)");
		terms[t] = QueryTermIn{ops[t], &opts[t], sub_off[t], sub_off[t + 1], phrase_num ? phrase_num[t] : -1, distance ? distance[t] : 1};
	}
	const rxgpu::FtQueryClass c = rxgpu::ft_classify_query(terms.data(), nterms);
	*empty = c.empty;
	*simple = c.simple;
	return RXGPU_OK;
}

// An rxgpu_ft_query as run_merge takes it: the parts' terms, then — unless the query is Empty(), which looks at the parts only — the
// synonyms' terms with their tables
struct ParsedQuery {
	std::vector<QueryTermIn> terms;
	SynonymsIn syn;
	bool empty = false, simple = false;
	const SynonymsIn* synonyms() const { return syn.nsyn ? &syn : nullptr; }
	MergeQuery merge_query(const rxgpu_ft_config* cfg, const rxgpu_ft_query* q, const uint8_t* excluded, const char* who) const {
		MergeQuery mq;
		mq.cfg = cfg;
		mq.simple = simple;
		mq.terms = &terms;
		mq.word_ids = q->word_ids;
		mq.procs = q->procs;
		mq.excluded = excluded;
		mq.synonyms = synonyms();
		mq.who = who;
		return mq;
	}
};
int parse_query(const char* who, const rxgpu_ft_query* q, ParsedQuery& out) {
	if (int rc = query_terms(who, q->nterms, q->ops, q->opts, q->phrase_num, q->distance, q->sub_off, q->word_ids, q->procs, out.terms, &out.empty, &out.simple); rc) return rc;
	if (out.empty || !q->nsyn) return RXGPU_OK;
	RX_CHECK(q->syn_term_off && q->part_syn_off, RXGPU_ERR_PARAMS, std::string(who) + ": null synonym tables");
	for (uint32_t k = 0; k < q->nsyn_terms; ++k) {
		const uint32_t t = q->nterms + k;
		RX_CHECK(q->ops[t] >= 1 && q->ops[t] <= 3, RXGPU_ERR_PARAMS, std::string(who) + ": op must be 1 (OR), 2 (AND) or 3 (NOT)");
		out.terms.push_back(QueryTermIn{q->ops[t], &q->opts[t], q->sub_off[t], q->sub_off[t + 1], -1, 1});
	}
	out.syn.nsyn = q->nsyn;
	out.syn.first_term = q->nterms;
	out.syn.syn_term_off = q->syn_term_off;
	out.syn.part_syn_off = q->part_syn_off;
	out.syn.part_syn = q->part_syn;
	out.syn.suppressed = q->suppressed;
	out.simple = false;
	return RXGPU_OK;
}

// A resident call on the handle: its lock, this thread's session, the dictionary, the device; the result of the merge before is forgotten
struct ResidentCall {
	std::unique_lock<std::mutex> lk;
	std::shared_lock<std::shared_mutex> dict_lk;
	rxgpu::DeviceGuard dg;
	static std::unique_lock<std::mutex> open(rxgpu_ft_index* h) {
		std::unique_lock<std::mutex> l(h->mtx);
		open_resident_session(h, l);
		return l;
	}
	explicit ResidentCall(rxgpu_ft_index* h) : lk(open(h)), dict_lk(h->dict_mtx), dg(h->device) {
		h->res_cap = 0;
		h->prep_done = false;
	}
};
int run_resident(rxgpu_ft_index* h, const MergeQuery& q) {
	uint64_t n = 0;
	MergeOut out;
	out.n = &n;
	return run_merge(h, q, out, true);
}

}  // namespace

extern "C" {

int rxgpu_ft_merge_simple_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_term_opts* opts, uint32_t nsub,
							  const uint32_t* word_ids, const float* procs, const uint8_t* excluded, uint32_t* out_doc, float* out_proc,
							  uint8_t* out_field, uint64_t cap, uint64_t* out_n) {
	const char* who = "rxgpu_ft_merge_simple_raw";
	RX_CHECK(h && cfg && opts && out_n, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_simple_raw: null argument");
	*out_n = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	if (nsub == 0) return RXGPU_OK;
	RX_CHECK(word_ids && procs && opts->field_boost && opts->need_sum_rank, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_simple_raw: null argument");
	LaneLock ll;
	if (int rc = checkout_lane(h, ll); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	const std::vector<QueryTermIn> terms{QueryTermIn{1, opts, 0, nsub}};
	return run_merge(ll.lane, MergeQuery{cfg, true, &terms, word_ids, procs, excluded, nullptr, nullptr, who}, MergeOut{out_doc, out_proc, out_field, nullptr, cap, out_n, nullptr});
}

int rxgpu_ft_merge_terms_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
							 const uint32_t* sub_off, const uint32_t* word_ids, const float* procs, const uint8_t* excluded, uint32_t* out_doc,
							 float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n, int32_t* out_preselected) {
	const char* who = "rxgpu_ft_merge_terms_raw";
	RX_CHECK(h && cfg && out_n, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: null argument");
	*out_n = 0;
	if (out_preselected) *out_preselected = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	// QueryMergeData::Empty() (querymergedata.h:208)
	if (nterms == 0) return RXGPU_OK;
	RX_CHECK(ops && opts && sub_off, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: null argument");
	for (uint32_t t = 0; t < nterms; ++t) RX_CHECK(ops[t] >= 1 && ops[t] <= 3, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: op must be 1 (OR), 2 (AND) or 3 (NOT)");
	if (nterms == 1 && ops[0] == 3) return RXGPU_OK;
	RX_CHECK(nterms >= 2, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: a single-term query is Simple(): use rxgpu_ft_merge_simple_raw");
	RX_CHECK(nterms < 0xFFFF, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: too many terms");
	RX_CHECK(sub_off[nterms] == 0 || (word_ids && procs), RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_raw: null argument");
	LaneLock ll;
	if (int rc = checkout_lane(h, ll); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	std::vector<QueryTermIn> terms(nterms);
	for (uint32_t t = 0; t < nterms; ++t) terms[t] = QueryTermIn{ops[t], &opts[t], sub_off[t], sub_off[t + 1]};
	return run_merge(ll.lane, MergeQuery{cfg, false, &terms, word_ids, procs, excluded, nullptr, nullptr, who},
					 MergeOut{out_doc, out_proc, out_field, out_terms_counter, cap, out_n, out_preselected});
}

int rxgpu_ft_merge_query_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
							 const int32_t* phrase_num, const int32_t* distance, const uint32_t* sub_off, const uint32_t* word_ids, const float* procs,
							 const uint8_t* excluded, uint32_t* out_doc, float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap,
							 uint64_t* out_n, int32_t* out_preselected) {
	const char* who = "rxgpu_ft_merge_query_raw";
	RX_CHECK(h && cfg && out_n, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*out_n = 0;
	if (out_preselected) *out_preselected = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	std::vector<QueryTermIn> terms;
	bool empty = false, simple = false;
	if (int rc = query_terms(who, nterms, ops, opts, phrase_num, distance, sub_off, word_ids, procs, terms, &empty, &simple); rc) return rc;
	if (empty) return RXGPU_OK;
	LaneLock ll;
	if (int rc = checkout_lane(h, ll); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	return run_merge(ll.lane, MergeQuery{cfg, simple, &terms, word_ids, procs, excluded, nullptr, nullptr, who},
					 MergeOut{out_doc, out_proc, out_field, out_terms_counter, cap, out_n, out_preselected});
}

int rxgpu_ft_merge_query2_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* q, const uint8_t* excluded, uint32_t* out_doc, float* out_proc,
							  uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n, int32_t* out_preselected) {
	const char* who = "rxgpu_ft_merge_query2_raw";
	RX_CHECK(h && cfg && q && out_n, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*out_n = 0;
	if (out_preselected) *out_preselected = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	RX_CHECK(q->nsyn > 0 || q->nsyn_terms == 0, RXGPU_ERR_PARAMS, std::string(who) + ": synonym terms without synonyms");
	ParsedQuery pq;
	if (int rc = parse_query(who, q, pq); rc) return rc;
	if (pq.empty) return RXGPU_OK;   // QueryMergeData::Empty() looks at the query parts only
	LaneLock ll;
	if (int rc = checkout_lane(h, ll); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	return run_merge(ll.lane, pq.merge_query(cfg, q, excluded, who), MergeOut{out_doc, out_proc, out_field, out_terms_counter, cap, out_n, out_preselected});
}

// Merger<IdCont, MergeDataAreas<Area>, ...>::Merge (merger.h:36-57 with kWithRegularAreas): the merge of rxgpu_ft_merge_query2_raw plus, per merged
// document and field, the areas its postings left — what highlight() / snippet() read.
int rxgpu_ft_merge_query_areas_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* q, const uint8_t* excluded, uint32_t max_areas_in_doc,
								   uint32_t* out_doc, float* out_proc, uint8_t* out_field, uint16_t* out_terms_counter, uint64_t cap, uint64_t* out_n,
								   int32_t* out_preselected, uint32_t* out_area_cnt, uint32_t* out_areas) {
	const char* who = "rxgpu_ft_merge_query_areas_raw";
	RX_CHECK(h && cfg && q && out_n && out_area_cnt && out_areas, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*out_n = 0;
	if (out_preselected) *out_preselected = 0;
	RX_CHECK(max_areas_in_doc >= 1 && max_areas_in_doc <= 4096, RXGPU_ERR_PARAMS, std::string(who) + ": max_areas_in_doc must be in [1, 4096] (FTConfig::maxAreasInDoc; unlimited areas stay on the CPU merger)");
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	RX_CHECK(q->nsyn == 0 && q->nsyn_terms == 0, RXGPU_ERR_LOGIC, std::string(who) + ": areas are built for queries without multi-word synonyms");
	ParsedQuery pq;
	if (int rc = parse_query(who, q, pq); rc) return rc;
	if (pq.empty) return RXGPU_OK;
	LaneLock ll;
	if (int rc = checkout_lane(h, ll); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	const AreasOut ao{max_areas_in_doc, out_area_cnt, out_areas};
	MergeQuery mq = pq.merge_query(cfg, q, excluded, who);
	mq.areas = &ao;
	return run_merge(ll.lane, mq, MergeOut{out_doc, out_proc, out_field, out_terms_counter, cap, out_n, out_preselected});
}

// Q queries over one index in ONE launch train (ft_merge.hip: grid.y = query).  The launch floors and the ramp of every kernel's grid are
// paid once per train instead of once per merge, and the device sees Q x the work at a time: what a planner with several FT queries in
// hand (or the hybrid path with its batch of queries) calls instead of Q single merges.
int rxgpu_ft_merge_batch_raw(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nq, const rxgpu_ft_query* queries, const uint8_t* const* excluded,
							 uint32_t* const* out_doc, float* const* out_proc, uint8_t* const* out_field, uint16_t* const* out_terms_counter, uint64_t cap,
							 uint64_t* out_n, int32_t* out_preselected) {
	const char* who = "rxgpu_ft_merge_batch_raw";
	RX_CHECK(h && cfg && out_n && (nq == 0 || (queries && out_doc && out_proc && out_field && out_terms_counter)), RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	for (uint32_t i = 0; i < nq; ++i) {
		out_n[i] = 0;
		if (out_preselected) out_preselected[i] = 0;
	}
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	auto out_of = [&](uint32_t i) { return MergeOut{out_doc[i], out_proc[i], out_field[i], out_terms_counter[i], cap, &out_n[i], out_preselected ? &out_preselected[i] : nullptr}; };
	// queries with phrases or multi-word synonyms have kernels of their own in front of the train (ft_phrase.hip, ft_syn_masks): one by one
	std::vector<uint32_t> batched;
	for (uint32_t i = 0; i < nq; ++i) {
		const rxgpu_ft_query& q = queries[i];
		bool plain = q.nsyn == 0 && q.nsyn_terms == 0;
		for (uint32_t t = 0; plain && q.phrase_num && t < q.nterms; ++t) plain = q.phrase_num[t] < 0;
		if (plain && !h->shard_set) {   // (a sharded index: every shard's handle runs one train and its exchanges at a time — the merges one by one)
			batched.push_back(i);
			continue;
		}
		const MergeOut o = out_of(i);
		if (int rc = rxgpu_ft_merge_query2_raw(h, cfg, &q, excluded ? excluded[i] : nullptr, o.doc, o.proc, o.field, o.terms_counter, cap, o.n, o.preselected); rc) return rc;
	}
	if (batched.empty()) return RXGPU_OK;
	std::lock_guard<std::mutex> batch_lk(h->batch_mtx);
	std::shared_lock<std::shared_mutex> dict_lk(h->dict_mtx);
	rxgpu::DeviceGuard dg(h->device);
	if (!h->batch_stream) RX_HIP(hipStreamCreateWithFlags(&h->batch_stream, hipStreamNonBlocking));
	if (!h->ev_ba) {
		RX_HIP(hipEventCreate(&h->ev_ba));
		RX_HIP(hipEventCreate(&h->ev_bb));
	}
	constexpr size_t kPlansBytes = (size_t(rxgpu::kFtBatchMax) * sizeof(rxgpu::FtPlan) + 255) & ~size_t(255);
	if (!h->h_batch_plans) RX_HIP(hipHostMalloc(&h->h_batch_plans, kPlansBytes, hipHostMallocDefault));
	if (int rc = h->d_batch_plans.ensure(kPlansBytes); rc) return rc;
	void* plans_dev_view = nullptr;
	RX_HIP(hipHostGetDevicePointer(&plans_dev_view, h->h_batch_plans, 0));
	hipStream_t st = h->batch_stream;
	for (size_t c0 = 0; c0 < batched.size(); c0 += rxgpu::kFtBatchMax) {
		const size_t c1 = std::min(batched.size(), c0 + rxgpu::kFtBatchMax);
		std::vector<MergeJob> jobs;
		std::vector<rxgpu_ft_index*> job_lane;
		std::vector<uint32_t> job_query;
		std::vector<rxgpu::FtPlan> host_plans;
		rxgpu::FtImportBatch pieces{};
		uint64_t postings = 0;
		for (size_t c = c0; c < c1; ++c) {
			const uint32_t i = batched[c];
			const rxgpu_ft_query& q = queries[i];
			ParsedQuery pq;   // (plain: no synonyms)
			if (int rc = parse_query(who, &q, pq); rc) return rc;
			if (pq.empty) continue;
			const size_t k = jobs.size();
			while (h->batch_lanes.size() <= k) {   // a scratch set per query of the train; the whole train runs on batch_stream
				std::unique_ptr<rxgpu_ft_index> lane;
				if (int rc = make_lane(h, false, lane); rc) return rc;
				h->batch_lanes.push_back(std::move(lane));
			}
			rxgpu_ft_index* lane = h->batch_lanes[k].get();
			lane_adopt_docs(lane, h);
			MergeJob job;
			if (int rc = prepare_merge(lane, st, pq.merge_query(cfg, &q, excluded ? excluded[i] : nullptr, who), false, OutRoom{out_of(i).complete(pq.simple), cap}, job, false); rc) {
				return rc;
			}
			if (job.empty) continue;
			pieces.src[k] = job.hp_dev;
			pieces.dst[k] = job.dev_base;
			pieces.n16[k] = uint32_t(job.plan_bytes / 16);
			postings += job.merged_postings;
			host_plans.push_back(job.p);
			jobs.push_back(job);
			job_lane.push_back(lane);
			job_query.push_back(i);
		}
		const uint32_t B = uint32_t(jobs.size());
		if (!B) continue;
		// the sparse train's queries in front, the dense train's behind: each train is launched over its own run of plans
		std::stable_sort(host_plans.begin(), host_plans.end(), [](const rxgpu::FtPlan& a, const rxgpu::FtPlan& b) {
			const int ka = a.sparse ? (a.prescore ? 0 : 1) : 2, kb = b.sparse ? (b.prescore ? 0 : 1) : 2;   // (the sparse train runs the preselecting queries as one run)
			return ka < kb;
		});
		uint32_t n_sparse = 0;
		while (n_sparse < B && host_plans[n_sparse].sparse) ++n_sparse;
		std::memcpy(h->h_batch_plans, host_plans.data(), size_t(B) * sizeof(rxgpu::FtPlan));
		pieces.src[B] = plans_dev_view;
		pieces.dst[B] = h->d_batch_plans.ptr;
		pieces.n16[B] = uint32_t((size_t(B) * sizeof(rxgpu::FtPlan) + 15) / 16);
		pieces.n = B + 1;
		const rxgpu::FtPlan* d_plans = static_cast<const rxgpu::FtPlan*>(h->d_batch_plans.ptr);
		for (rxgpu_ft_index* lane : job_lane) lane->clean_dirty = true;   // until the train has run to its end
		RX_HIP(rxgpu::launch_ft_import_batch(pieces, st));
		RX_HIP(hipEventRecord(h->ev_ba, st));
		RX_HIP(rxgpu::launch_ft_merge_sparse(d_plans, host_plans.data(), n_sparse, st));
		RX_HIP(rxgpu::launch_ft_merge(d_plans + n_sparse, host_plans.data() + n_sparse, B - n_sparse, st));
		RX_HIP(hipEventRecord(h->ev_bb, st));
		h->trains_sparse += n_sparse;
		h->trains_dense += B - n_sparse;
		RX_HIP(rxgpu::launch_ft_export(d_plans, host_plans.data(), B, st));
		if (int rc = wait_stream_polled(st); rc) return rc;
		float ms = 0.f;
		(void)hipEventElapsedTime(&ms, h->ev_ba, h->ev_bb);
		h->stat_postings += postings;
		h->stat_ms += ms;
		h->batch_trains += 1;
		h->batch_merges += B;
		for (uint32_t k = 0; k < B; ++k) {
			if (int rc = collect_merge(job_lane[k], jobs[k], out_of(job_query[k]), who); rc) return rc;
		}
	}
	return RXGPU_OK;
}

void rxgpu_ft_set_train_mode(int mode) { ft_train_mode()->store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }
int rxgpu_ft_read_train_stats(rxgpu_ft_index* h, uint64_t* dense_merges, uint64_t* sparse_merges) {
	RX_CHECK(h && dense_merges && sparse_merges, RXGPU_ERR_PARAMS, "rxgpu_ft_read_train_stats: null argument");
	*dense_merges = h->trains_dense.exchange(0);
	*sparse_merges = h->trains_sparse.exchange(0);
	return RXGPU_OK;
}
int rxgpu_ft_read_batch_stats(rxgpu_ft_index* h, uint64_t* trains, uint64_t* merges) {
	RX_CHECK(h && trains && merges, RXGPU_ERR_PARAMS, "rxgpu_ft_read_batch_stats: null argument");
	std::lock_guard<std::mutex> lk(h->batch_mtx);
	*trains = h->batch_trains;
	*merges = h->batch_merges;
	return RXGPU_OK;
}

int rxgpu_ft_merge_query_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
								  const int32_t* phrase_num, const int32_t* distance, const uint32_t* sub_off, const uint32_t* word_ids, const float* procs,
								  const uint8_t* excluded, int32_t* out_enqueued) {
	const char* who = "rxgpu_ft_merge_query_resident";
	RX_CHECK(h && cfg && out_enqueued, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*out_enqueued = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	std::vector<QueryTermIn> terms;
	bool empty = false, simple = false;
	if (int rc = query_terms(who, nterms, ops, opts, phrase_num, distance, sub_off, word_ids, procs, terms, &empty, &simple); rc) return rc;
	ResidentCall call(h);
	if (empty) return finish_pending(h, who);   // nothing is merged: the fusion sees an empty FT side
	if (int rc = run_resident(h, MergeQuery{cfg, simple, &terms, word_ids, procs, excluded, nullptr, nullptr, who}); rc) return rc;
	*out_enqueued = h->res_pending ? 1 : 0;
	return RXGPU_OK;
}

// ... and the resident form of rxgpu_ft_merge_query2_raw: multi-word synonyms included.  The documents that hold only parts of a synonym
// stay in the result with their 0xFFFF mark; the fusion kernels treat them as absent (HybridFuseArgs::ft_terms).
int rxgpu_ft_merge_query2_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_query* q, const uint8_t* excluded, int32_t* out_enqueued) {
	const char* who = "rxgpu_ft_merge_query2_resident";
	RX_CHECK(h && cfg && q && out_enqueued, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*out_enqueued = 0;
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	RX_CHECK(q->nsyn > 0 || q->nsyn_terms == 0, RXGPU_ERR_PARAMS, std::string(who) + ": synonym terms without synonyms");
	ParsedQuery pq;
	if (int rc = parse_query(who, q, pq); rc) return rc;
	ResidentCall call(h);
	if (pq.empty) return finish_pending(h, who);   // nothing is merged: the fusion sees an empty FT side
	if (int rc = run_resident(h, pq.merge_query(cfg, q, excluded, who)); rc) return rc;
	*out_enqueued = h->res_pending ? 1 : 0;
	return RXGPU_OK;
}

// ---------------------------------------------------------------------------------------------------- hybrid: merges that stay in HBM + the fusion
int rxgpu_ft_merge_simple_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const rxgpu_ft_term_opts* opts, uint32_t nsub,
								   const uint32_t* word_ids, const float* procs, const uint8_t* excluded) {
	const char* who = "rxgpu_ft_merge_simple_resident";
	RX_CHECK(h && cfg && opts, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_simple_resident: null argument");
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	RX_CHECK(nsub > 0 && word_ids && procs && opts->field_boost && opts->need_sum_rank, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_simple_resident: null argument");
	ResidentCall call(h);
	const std::vector<QueryTermIn> terms{QueryTermIn{1, opts, 0, nsub}};
	return run_resident(h, MergeQuery{cfg, true, &terms, word_ids, procs, excluded, nullptr, nullptr, who});
}

int rxgpu_ft_merge_terms_resident(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, uint32_t nterms, const int32_t* ops, const rxgpu_ft_term_opts* opts,
								  const uint32_t* sub_off, const uint32_t* word_ids, const float* procs, const uint8_t* excluded) {
	const char* who = "rxgpu_ft_merge_terms_resident";
	RX_CHECK(h && cfg && ops && opts && sub_off, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_resident: null argument");
	if (int rc = check_merge_head(h, cfg, who); rc) return rc;
	RX_CHECK(nterms >= 2 && nterms < 0xFFFF, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_resident: 2 or more terms (one term: rxgpu_ft_merge_simple_resident)");
	for (uint32_t t = 0; t < nterms; ++t) RX_CHECK(ops[t] >= 1 && ops[t] <= 3, RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_resident: op must be 1 (OR), 2 (AND) or 3 (NOT)");
	RX_CHECK(sub_off[nterms] == 0 || (word_ids && procs), RXGPU_ERR_PARAMS, "rxgpu_ft_merge_terms_resident: null argument");
	ResidentCall call(h);
	std::vector<QueryTermIn> terms(nterms);
	for (uint32_t t = 0; t < nterms; ++t) terms[t] = QueryTermIn{ops[t], &opts[t], sub_off[t], sub_off[t + 1]};
	return run_resident(h, MergeQuery{cfg, false, &terms, word_ids, procs, excluded, nullptr, nullptr, who});
}

}  // extern "C"
