// One BM25 merge on one lane = one launch train: ft_merge_plan.h decides, this unit gathers the facts, stages the plan, launches and
// collects.  Also the resident session a hybrid query keeps between its merge and its fusion (rxgpu_hybrid.hip).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rxgpu_ft_internal.h"
#include "ft_rank.hip.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

// ---------------------------------------------------------------------------------------------------- one merge = one launch train
namespace {
// the calculator's IDF per sub-term (bm25.h): totalDocCount = totalNumDocs - 1 ("first doc is always empty"), matchedDocCount = |postings|
double subterm_idf(int bm25_type, uint64_t total_docs, uint64_t n) {
	const double td = double(total_docs - 1), md = double(n);
	if (bm25_type == rxgpu::kFtBm25WordCount) return 0.0;                            // TermCount::GetIDF
	if (bm25_type == rxgpu::kFtBm25Classic) return std::log(td / (md + 1)) + 1;      // Bm25Classic::IDF
	double f = n ? std::log((td - md + 1) / md) / std::log(1 + td) : 0.2;            // Bm25Rx::IDF, saturated at 0.2
	if (f < 0.2) f = 0.2;
	return f;
}
}  // namespace

namespace rxgpu {

// a refusal of the plan (ft_merge_plan.h) as the C-ABI reports it
int plan_error(const rxgpu::FtPlanError& e) {
	set_error(e.msg);
	return e.code;
}
void fill_term_cfg(rxgpu::FtTermCfg& tc, const rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const QueryTermIn& qt, bool same, bool all_pos) {
	tc.num_fields = h->num_fields;
	tc.bm25_type = cfg->bm25_type;
	tc.words = h->d_words;
	tc.avg_words = h->d_avg;
	tc.k1 = cfg->bm25_k1;
	tc.b = cfg->bm25_b;
	tc.summation_ratio = cfg->summation_ranks_by_fields_ratio;
	tc.opts_boost = qt.opts->boost;
	tc.term_len_boost_in = qt.opts->term_len_boost;
	tc.op = qt.op;
	tc.same_boost = same ? 1 : 0;
	tc.all_pos_boost = all_pos ? 1 : 0;
}
// the per-field FTConfig parameters as floats (bound() takes float arguments): 6 x nf
void stage_field_cfg(float* fc, const rxgpu_ft_config* cfg, uint32_t nf) {
	for (uint32_t f = 0; f < nf; ++f) {
		fc[0 * nf + f] = float(cfg->bm25_boost[f]);
		fc[1 * nf + f] = float(cfg->bm25_weight[f]);
		fc[2 * nf + f] = float(cfg->term_len_boost[f]);
		fc[3 * nf + f] = float(cfg->term_len_weight[f]);
		fc[4 * nf + f] = float(cfg->position_boost[f]);
		fc[5 * nf + f] = float(cfg->position_weight[f]);
	}
}
void point_term_cfg(rxgpu::FtTermCfg& tc, const float* d_fc, const float* d_field_boost, const uint8_t* d_need_sum, uint32_t nf) {
	tc.field_boost = d_field_boost;
	tc.need_sum_rank = d_need_sum;
	tc.bm25_boost = d_fc + 0 * nf;
	tc.bm25_weight = d_fc + 1 * nf;
	tc.term_len_boost = d_fc + 2 * nf;
	tc.term_len_weight = d_fc + 3 * nf;
	tc.position_boost = d_fc + 4 * nf;
	tc.position_weight = d_fc + 5 * nf;
}
rxgpu::FtPosSubterm word_subterm(const rxgpu_ft_word& w, int bm25_type, uint64_t N, float proc) {
	rxgpu::FtPosSubterm ft{};
	ft.n = w.n;
	ft.doc = w.doc;
	ft.ent_off = w.ent_off;
	ft.ent_field = w.ent_field;
	ft.ent_tf = w.ent_tf;
	ft.ent_first_pos = w.ent_first_pos;
	ft.pos_off = w.pos_off;
	ft.fpos = w.fpos;
	ft.idf = subterm_idf(bm25_type, N, word_df(w));
	ft.proc = proc;
	ft.range_off = w.range_off;
	ft.n_ranges = w.n_ranges;
	return ft;
}

}  // namespace rxgpu

namespace {
constexpr std::chrono::milliseconds kResidentPatience{2000};
// what THIS thread believes about its resident session (one text index at a time per thread: HybridQueryResident runs its steps in a row)
thread_local const rxgpu_ft_index* tl_res_handle = nullptr;
thread_local uint64_t tl_res_generation = 0;
}  // namespace

namespace rxgpu {

// `lk` holds h->mtx.  Waits until no OTHER thread's session is open (bounded), then opens one for the caller.
void open_resident_session(rxgpu_ft_index* h, std::unique_lock<std::mutex>& lk) {
	const auto me = std::this_thread::get_id();
	if (h->res_session && h->res_owner != me) {
		(void)h->res_cv.wait_for(lk, kResidentPatience, [&] { return !h->res_session; });   // timed out: the session is taken over below
	}
	h->res_session = true;
	h->res_owner = me;
	h->res_generation += 1;
	tl_res_handle = h;
	tl_res_generation = h->res_generation;
}
// `lk` holds h->mtx.  RXGPU_OK when the caller may use the lane for the prepare / fuse step: it owns the open session, or it never opened one
// (a query whose FT side merged nothing) and nobody else's is open (waited for, bounded).
int check_resident_session(rxgpu_ft_index* h, std::unique_lock<std::mutex>& lk, const char* who) {
	const auto me = std::this_thread::get_id();
	if (tl_res_handle == h && tl_res_generation != 0) {
		if (!(h->res_session && h->res_owner == me && h->res_generation == tl_res_generation)) {
			tl_res_generation = 0;
			set_error(std::string(who) + ": this thread's resident merge was replaced by another caller's (its session was not fused within 2 s)");
			return RXGPU_ERR_LOGIC;
		}
		return RXGPU_OK;
	}
	if (h->res_session && h->res_owner != me) {
		if (!h->res_cv.wait_for(lk, kResidentPatience, [&] { return !h->res_session; })) {
			set_error(std::string(who) + ": another caller's resident merge is parked on this index");
			return RXGPU_ERR_LOGIC;
		}
	}
	// a fusion without a resident merge in front (the query's FT side merged nothing): a session of its own with an empty FT side, so that
	// nobody else's prepare lands between this caller's prepare and its fuse
	if (!h->res_session) {
		h->res_pending = false;
		h->res_cap = 0;
		h->prep_done = false;
	}
	h->res_session = true;
	h->res_owner = me;
	h->res_generation += 1;
	tl_res_handle = h;
	tl_res_generation = h->res_generation;
	return RXGPU_OK;
}
void close_resident_session(rxgpu_ft_index* h) {
	if (h->res_session && h->res_owner == std::this_thread::get_id()) {
		h->res_session = false;
		h->res_cv.notify_all();
	}
	if (tl_res_handle == h) tl_res_generation = 0;
}

// The header of a packed result (FtOutLayout): the look-back word and the count
int check_result_header(const uint32_t* hdr, uint64_t max_merged, const char* who) {
	RX_CHECK(hdr[1] == 0, RXGPU_ERR_DEVICE, std::string(who) + ": ordered look-back timed out on the device");
	RX_CHECK(hdr[0] <= max_merged, RXGPU_ERR_DEVICE, std::string(who) + ": corrupt result header");
	return RXGPU_OK;
}

// A merge is ~0.1 ms of device time: poll for its end instead of sleeping in hipStreamSynchronize (the wake-up alone is tens of
// microseconds); anything that takes longer than a few milliseconds falls back to the blocking wait
int wait_stream_polled(hipStream_t st) {
	using clk = std::chrono::steady_clock;
	const auto t_poll = clk::now();
	hipError_t q = hipStreamQuery(st);
	while (q == hipErrorNotReady && std::chrono::duration<double, std::micro>(clk::now() - t_poll).count() < 3000.0) q = hipStreamQuery(st);
	if (q == hipErrorNotReady) {
		RX_HIP(hipStreamSynchronize(st));
	} else {
		RX_HIP(q);
	}
	return RXGPU_OK;
}

// The header of a resident merge that has ended: the look-back word, the kernel time, the kept-clean state.  (Its capacity may be gone by
// now — a later resident call resets res_cap — so the count is not checked here.)
int settle_resident_merge(rxgpu_ft_index* h, const char* who) {
	uint32_t hdr[4] = {0, 0, 0, 0};
	RX_HIP(hipMemcpy(hdr, h->d_out.ptr, sizeof(hdr), hipMemcpyDeviceToHost));
	float ms = 0.f;
	if (h->ev_a && hipEventElapsedTime(&ms, h->ev_a, h->ev_b) == hipSuccess) h->stat_ms += ms;
	if (int rc = check_result_header(hdr, UINT64_MAX, who); rc) return rc;
	h->clean_dirty = false;
	return RXGPU_OK;
}
// A resident merge was enqueued and nobody looked at its header yet: wait for it and settle it.
int finish_pending(rxgpu_ft_index* h, const char* who) {
	if (!h->res_pending) return RXGPU_OK;
	h->res_pending = false;
	RX_HIP(hipStreamSynchronize(h->stream));
	return settle_resident_merge(h, who);
}

// Which launch train runs a merge: -1 the host decides per query (ft_sparse_eligible + a density test), 0 always the dense train
// (ft_merge.hip), 1 the sparse train (ft_sparse.hip) whenever the query is eligible.  RXGPU_FT_TRAIN=dense|sparse presets it, read once;
// rxgpu_ft_set_train_mode changes it (tests, benchmarks).
std::atomic<int>* ft_train_mode() {
	static std::atomic<int> mode{[] {
		const char* e = std::getenv("RXGPU_FT_TRAIN");
		if (e && std::strcmp(e, "dense") == 0) return 0;
		if (e && std::strcmp(e, "sparse") == 0) return 1;
		return -1;
	}()};
	return &mode;
}

}  // namespace rxgpu

namespace {
// ---------------------------------------------------------------------------------------------------- the first half of a merge
// Three steps: gather the facts (the one look at the dictionary), let ft_merge_plan.h decide, execute — scratch, the plan staged in the lane's
// pinned buffer (FtPlan included, behind the tables it points into) and the copy kernel that takes it to HBM.  Everything is enqueued on one
// stream: the lane's own for a single merge, the batch stream when Q lanes' merges go into one train.
static_assert(rxgpu::kFtPlanBm25Classic == rxgpu::kFtBm25Classic, "ft_merge_plan.h and ft_rank.hip.h name the same calculator");

constexpr rxgpu::FtStructSizes kStructSizes{sizeof(rxgpu::FtPosSubterm), sizeof(rxgpu::FtTermCfg), sizeof(rxgpu::FtSynMaskJob), sizeof(rxgpu::FtPlan), sizeof(uint4)};

// One merge between its query and its MergeJob
struct MergePrep {
	std::vector<rxgpu::FtSubFact> subs;
	rxgpu::FtMergeFacts facts;
	rxgpu::FtMergePlan plan;
	std::vector<PhraseRows> phrase_rows;   // per part; filled for the phrase parts
	size_t n_phrases = 0;
	const uint8_t* d_excluded = nullptr;
	const uint32_t* d_excluded_bits = nullptr;
};
struct PhraseView {   // what ft_plan_rows reads of the phrases
	const std::vector<PhraseRows>& pr;
	uint64_t admitted(uint32_t pi) const { return pr[pi].admitted; }
	uint32_t n_rows(uint32_t pi) const { return uint32_t(pr[pi].rows.size()); }
	uint64_t row_n(uint32_t pi, uint32_t r) const { return pr[pi].rows[r].n; }
};

// Step 1: the facts.  The dictionary is looked up once per sub-term; an unknown word is a fact too (the plan reports it in its turn).
void gather_facts(const rxgpu_ft_index* h, const MergeQuery& q, bool resident, OutRoom room, MergePrep& mp) {
	const std::vector<QueryTermIn>& terms = *q.terms;
	const auto& dict = h->dict();
	uint32_t n_subs = 0;   // (sized by the largest range, whatever the order of the caller's offsets)
	for (const QueryTermIn& qt : terms) n_subs = std::max(n_subs, qt.sub_end);
	mp.subs.assign(n_subs, rxgpu::FtSubFact{});
	for (const QueryTermIn& qt : terms) {
		for (uint32_t si = qt.sub_begin; si < qt.sub_end; ++si) {
			const auto it = dict.find(q.word_ids[si]);
			if (it == dict.end()) continue;
			const rxgpu_ft_word& w = it->second;
			mp.subs[si] = rxgpu::FtSubFact{w.n, word_df(w), w.last_doc, true, w.fpos != nullptr, &w};
		}
	}
	rxgpu::FtMergeFacts& f = mp.facts;
	f.terms = terms.data();
	f.nterms = uint32_t(terms.size());
	f.synonyms = q.synonyms;
	f.subs = mp.subs.data();
	f.procs = q.procs;
	f.cfg = q.cfg;
	f.num_fields = h->num_fields;
	f.h_avg = h->h_avg.data();
	f.n_avg = uint32_t(h->h_avg.size());
	f.total_docs = h->total_docs;
	f.sh_total = h->sh_total;
	f.train_mode = ft_train_mode()->load(std::memory_order_relaxed);
	f.simple = q.simple;
	f.resident = resident;
	f.max_areas = q.max_areas();
	f.have_outs = room.have_outs;
	f.cap = room.cap;
	f.who = q.who;
}

// docsExcluded of the merge: one byte per document, or (the sparse train) one bit
int upload_excluded(rxgpu_ft_index* h, hipStream_t st, const uint8_t* excluded, MergePrep& mp) {
	const uint64_t N = h->total_docs;
	if (excluded && mp.plan.sparse) {
		std::vector<uint32_t> bits((N + 31) / 32, 0u);
		for (uint64_t d = 0; d < N; ++d) bits[d >> 5] |= (excluded[d] ? 1u : 0u) << (d & 31);
		if (int rc = h->d_excl.ensure(bits.size() * 4); rc) return rc;
		RX_HIP(hipMemcpyAsync(h->d_excl.ptr, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, st));   // (pageable source: the copy is staged before the call returns)
		mp.d_excluded_bits = static_cast<const uint32_t*>(h->d_excl.ptr);
	} else if (excluded) {
		if (int rc = h->d_excl.ensure(N); rc) return rc;
		RX_HIP(hipMemcpyAsync(h->d_excl.ptr, excluded, N, hipMemcpyHostToDevice, st));
		mp.d_excluded = static_cast<const uint8_t*>(h->d_excl.ptr);
	}
	return RXGPU_OK;
}

// Facts, the plan's first half, docsExcluded: what every kind of preparation starts with.  mp.plan.empty: nothing is merged.
int begin_merge(rxgpu_ft_index* h, hipStream_t st, const MergeQuery& q, bool resident, OutRoom room, MergePrep& mp) {
	gather_facts(h, q, resident, room, mp);
	if (rxgpu::FtPlanError e = rxgpu::ft_plan_volume(mp.facts, mp.plan); e) return plan_error(e);
	if (mp.plan.empty) return RXGPU_OK;
	return upload_excluded(h, st, q.excluded, mp);
}

// Phrases first (Merger::init, merger.h:73-81): every PhraseMerger runs before the query parts are looked at
int run_query_phrases(rxgpu_ft_index* h, const MergeQuery& q, MergePrep& mp, bool first_half_only) {
	mp.n_phrases = 0;
	if (!mp.plan.any_phrase) return RXGPU_OK;   // (phrase_rows is read for phrase parts only)
	mp.phrase_rows.assign(mp.plan.nparts, PhraseRows{});
	for (uint32_t pi = 0; pi < mp.plan.nparts; ++pi) {
		if (!mp.plan.parts[pi].phrase) continue;
		if (int rc = run_phrase(h, q.cfg, *q.terms, mp.plan.parts[pi], q.word_ids, q.procs, mp.d_excluded, mp.n_phrases++, mp.phrase_rows[pi], q.who, first_half_only); rc) return rc;
	}
	return RXGPU_OK;
}

// The tables of the plan region, staged in pinned memory `hp`; device addresses are those of `base` (the lane's state buffer)
void stage_plan_tables(rxgpu_ft_index* h, const MergeQuery& q, const MergePrep& mp, char* hp, char* base) {
	const rxgpu::FtMergePlan& pl = mp.plan;
	const rxgpu::FtStateLayout& L = pl.state;
	const rxgpu_ft_config* cfg = q.cfg;
	const std::vector<QueryTermIn>& terms = *q.terms;
	const uint32_t nf = h->num_fields, nparts = pl.nparts;
	std::memset(hp, 0, L.plan_bytes);
	auto* subs = reinterpret_cast<rxgpu::FtPosSubterm*>(hp + L.plan_subs.off);
	for (size_t i = 0; i < pl.rows.size(); ++i) {
		const rxgpu::FtRow& r = pl.rows[i];
		rxgpu::FtPosSubterm ft = r.phrase ? mp.phrase_rows[r.term].rows[r.src]
										  : word_subterm(*static_cast<const rxgpu_ft_word*>(mp.subs[r.src].source), cfg->bm25_type, h->total_docs, q.procs[r.src]);
		ft.term = r.term;
		ft.qp = r.qp;
		ft.prev_term_qp = r.prev_term_qp;
		ft.ord_in_term = r.ord_in_term;
		ft.row = r.row;
		ft.suppressed = r.suppressed;
		subs[i] = ft;
	}
	float* fc = reinterpret_cast<float*>(hp + L.plan_fc.off);
	uint8_t* need_sum = reinterpret_cast<uint8_t*>(fc + L.cfg_floats);
	const float* d_fc = reinterpret_cast<const float*>(base + L.plan_fc.off);
	const uint8_t* d_need_sum = reinterpret_cast<const uint8_t*>(d_fc + L.cfg_floats);
	stage_field_cfg(fc, cfg, nf);
	auto* tcfg = reinterpret_cast<rxgpu::FtTermCfg*>(hp + L.plan_terms.off);
	for (uint32_t ti = 0; ti < uint32_t(pl.terms.size()); ++ti) {   // the query parts (a phrase is one part: its first term's), then the synonyms' terms
		const rxgpu::FtPlanTerm& pt = pl.terms[ti];
		const QueryTermIn& qt = ti < nparts ? terms[pl.parts[ti].t_begin] : terms[pl.npart_terms + (ti - nparts)];
		rxgpu::FtTermCfg& tc = tcfg[ti];
		fill_term_cfg(tc, h, cfg, qt, pt.same_boost, pt.all_pos_boost);
		tc.op = pt.op;
		tc.sub_begin = pt.sub_begin;
		tc.sub_end = pt.sub_end;
		if (pt.phrase) {   // its rows carry rank and field, every document counts for the masks, the pre-score adds CalcProc16
			tc.opts_boost = 1.0f;
			tc.phrase = 1;
			tc.phrase_proc16 = mp.phrase_rows[ti].proc16;
		}
		for (uint32_t f = 0; f < nf; ++f) {   // a phrase part: ones (its rows are ranked already; ft_ranges reads field_boost[0] > 0)
			fc[size_t(6 + ti) * nf + f] = pt.phrase ? 1.0f : qt.opts->field_boost[f];
			need_sum[size_t(ti) * nf + f] = pt.phrase ? uint8_t(0) : qt.opts->need_sum_rank[f];
		}
		point_term_cfg(tc, d_fc, d_fc + size_t(6 + ti) * nf, d_need_sum + size_t(ti) * nf, nf);
	}
	auto* jobs = reinterpret_cast<rxgpu::FtSynMaskJob*>(hp + L.plan_jobs.off);
	for (size_t j = 0; j < pl.jobs.size(); ++j) {
		jobs[j].syn_begin = pl.jobs[j].syn_begin;
		jobs[j].syn_end = pl.jobs[j].syn_end;
		jobs[j].out = reinterpret_cast<uint32_t*>(base + L.synmask.off) + j * pl.nwords;
		tcfg[pl.jobs[j].part].syn_mask = jobs[j].out;
	}
	if (!pl.syns.empty()) std::memcpy(hp + L.plan_syns.off, pl.syns.data(), pl.syns.size() * sizeof(rxgpu::FtSynonym));
	if (!pl.job_syns.empty()) std::memcpy(hp + L.plan_jsyn.off, pl.job_syns.data(), pl.job_syns.size() * 4);
	if (!pl.merge_grid.empty()) std::memcpy(hp + L.plan_mgrid.off, pl.merge_grid.data(), pl.merge_grid.size() * sizeof(rxgpu::FtGridEntry));
}

// FtPlan: the plan's numbers and the addresses of its regions in the lane's buffers
void fill_ft_plan(const rxgpu_ft_index* h, const MergeQuery& q, const MergePrep& mp, const char* hp, void* hp_dev, rxgpu::FtPlan& p) {
	const rxgpu::FtMergePlan& pl = mp.plan;
	const rxgpu::FtStateLayout& L = pl.state;
	const rxgpu::FtCleanLayout& C = pl.clean;
	const rxgpu_ft_config* cfg = q.cfg;
	char* base = static_cast<char*>(h->d_state.ptr);
	char* cbase = static_cast<char*>(h->d_clean.ptr);
	char* ob = static_cast<char*>(h->d_out.ptr);
	const bool prescore = pl.prescore;
	p = rxgpu::FtPlan{};
	p.subs = reinterpret_cast<const rxgpu::FtPosSubterm*>(base + L.plan_subs.off);
	p.terms = reinterpret_cast<const rxgpu::FtTermCfg*>(base + L.plan_terms.off);
	p.merge_grid = reinterpret_cast<const rxgpu::FtGridEntry*>(base + L.plan_mgrid.off);
	p.n_merge_entries = uint32_t(pl.merge_grid.size());
	p.merge_blocks = uint32_t(pl.merge_blocks);
	p.nterms = uint32_t(pl.terms.size());
	p.n_parts = pl.nparts;
	p.n_part_qp = pl.n_part_qp;
	p.syns = reinterpret_cast<const rxgpu::FtSynonym*>(base + L.plan_syns.off);
	p.n_syn = pl.nsyn;
	p.syn_jobs = reinterpret_cast<const rxgpu::FtSynMaskJob*>(base + L.plan_jobs.off);
	p.job_syns = reinterpret_cast<const uint32_t*>(base + L.plan_jsyn.off);
	p.n_syn_jobs = uint32_t(pl.jobs.size());
	p.query_len = pl.query_len;
	p.n_rows = pl.n_rows;
	p.n_subs = uint32_t(pl.rows.size());
	p.total_docs = h->total_docs;
	p.nwords = pl.nwords;
	p.max_merged = uint32_t(pl.max_merged);
	p.merge_limit = cfg->merge_limit;
	p.simple = q.simple ? 1 : 0;
	p.prescore = prescore ? 1 : 0;
	p.check_removed = 1;
	p.distance_weight = float(cfg->distance_weight);
	p.distance_boost = float(cfg->distance_boost);
	p.full_match_boost = cfg->full_match_boost;
	p.removed = h->d_removed;
	p.excluded = mp.d_excluded;
	p.mask = reinterpret_cast<uint32_t*>(base + L.mask.off);
	p.score = prescore ? reinterpret_cast<uint16_t*>(base + L.score.off) : nullptr;
	p.hist = prescore ? reinterpret_cast<uint32_t*>(cbase + C.hist.off) : nullptr;
	p.lookback_pre = prescore ? reinterpret_cast<unsigned long long*>(cbase + C.lb_pre.off) : nullptr;
	p.b_rec = reinterpret_cast<uint4*>(base + L.brec.off);
	p.bucket_off = reinterpret_cast<uint32_t*>(base + L.boff.off);
	p.bucket_cnt = reinterpret_cast<uint32_t*>(cbase + C.bcnt.off);
	p.adders = reinterpret_cast<uint32_t*>(base + L.adders.off);
	p.n_ranges = pl.n_ranges;
	p.e_rank = reinterpret_cast<float*>(cbase + C.erank.off);
	p.e_idx = reinterpret_cast<uint32_t*>(base + L.eidx.off);
	p.e_field = reinterpret_cast<uint8_t*>(base + L.efield.off);
	p.sync = reinterpret_cast<uint32_t*>(cbase + C.sync.off);
	static const char* const stamps_env = std::getenv("RXGPU_FT_STAMPS");   // (a debugging hook: read once, not once per merge)
	p.dbg = stamps_env ? reinterpret_cast<unsigned long long*>(cbase + C.dbg.off) : nullptr;
	p.dbg_block = stamps_env ? uint32_t(std::atoi(stamps_env)) : 0;
	p.out_header = reinterpret_cast<uint32_t*>(ob + pl.out.header);
	p.host_out = hp_dev;
	p.out_doc = reinterpret_cast<uint32_t*>(ob + pl.out.doc);
	p.out_proc = reinterpret_cast<float*>(ob + pl.out.proc);
	p.out_terms_counter = reinterpret_cast<uint16_t*>(ob + pl.out.terms_counter);
	p.out_field = reinterpret_cast<uint8_t*>(ob + pl.out.field);
	p.sparse = pl.sparse ? 1 : 0;
	p.removed_bits = h->d_removed_bits;
	p.excluded_bits = mp.d_excluded_bits;
	p.lb_units = reinterpret_cast<unsigned long long*>(cbase + C.lb_units.off);
	if (pl.sparse) {
		p.t_doc = reinterpret_cast<uint32_t*>(base + L.tdoc.off);
		p.t_pos = reinterpret_cast<uint32_t*>(base + L.tpos.off);
		p.t_idx = reinterpret_cast<uint32_t*>(base + L.tidx.off);
		const auto* subs = reinterpret_cast<const rxgpu::FtPosSubterm*>(hp + L.plan_subs.off);
		for (size_t si = 0; si < pl.rows.size(); ++si) {   // what the unit kernels read of a sub-term, and its attribute word (ft_sparse.hip)
			p.sp_sub[si].doc = subs[si].doc;
			p.sp_sub[si].range_off = subs[si].range_off;
			p.sp_sub[si].n = uint32_t(subs[si].n);
			p.sp_sub[si].n_ranges = subs[si].n_ranges;
			p.sp_sub[si].attr = pl.rows[si].attr;
		}
		p.sp_empty_and = pl.sp_empty_and ? 1 : 0;
	}
}

// Step 3: the plan on the device.  `phrases_given`: the rows came from the sharded layer (a shard never runs a query's phrases on its own).
int execute_plan(rxgpu_ft_index* h, hipStream_t st, const MergeQuery& q, const MergePrep& mp, bool resident, bool phrases_given, MergeJob& job, bool import_now) {
	const rxgpu::FtMergePlan& pl = mp.plan;
	const char* who = q.who;
	const size_t M = size_t(pl.max_merged);
	// ---- device scratch (one buffer each for the state and for the packed result)
	if (int rc = h->d_state.ensure(pl.state.bytes); rc) return rc;
	char* base = static_cast<char*>(h->d_state.ptr);
	if (h->clean_docs != h->total_docs || h->d_clean.bytes < pl.clean.bytes) {
		if (int rc = h->d_clean.ensure(pl.clean.bytes); rc) return rc;
		h->clean_docs = h->total_docs;
		h->clean_dirty = true;
	}
	if (int rc = h->d_out.ensure(pl.out.bytes); rc) return rc;
	// ---- host staging of the plan (pinned), one upload
	if (int rc = h->ensure_pinned(std::max(pl.state.plan_bytes, pl.out.bytes)); rc) return rc;
	char* hp = static_cast<char*>(h->h_pinned);
	stage_plan_tables(h, q, mp, hp, base);
	if (h->clean_dirty) {
		RX_HIP(hipMemsetAsync(h->d_clean.ptr, 0, h->d_clean.bytes, st));
		h->clean_dirty = false;
	}
	void* hp_dev = nullptr;   // the pinned staging buffer as the device sees it
	RX_HIP(hipHostGetDevicePointer(&hp_dev, hp, 0));
	rxgpu::FtPlan& p = job.p;
	fill_ft_plan(h, q, mp, hp, hp_dev, p);
	if (h->sh_total > 1) {   // a document-range shard: its own ranges, the facts that span the shards arrive between the kernels
		// (multi-word synonyms are fine: their masks, term counts and the "only parts of a synonym" marks are facts of ONE document, and a
		// document lies in one shard — ft_syn_masks sees this shard's fragments, the caller drops the marked documents after the union)
		RX_CHECK(!resident, RXGPU_ERR_LOGIC, std::string(who) + ": a sharded ft index merges into the caller's lists (no resident results)");
		RX_CHECK(mp.n_phrases == 0 || phrases_given, RXGPU_ERR_LOGIC, std::string(who) + ": a shard's phrases are run by the sharded layer");
		p.range_begin = h->sh_range_begin;
		p.range_count = h->sh_range_count;
		p.shard_index = h->sh_index;
		p.n_shards = h->sh_total;
		p.shard_hist = pl.prescore ? h->sh_hist : nullptr;
		p.shard_pos = h->sh_pos;
		RX_HIP(hipMemsetAsync(p.adders, 0, std::max<size_t>(1, size_t(pl.n_rows) * pl.n_ranges) * 4, st));   // the other shards' columns
		RX_HIP(hipMemsetAsync(p.out_doc, 0xFF, M * 4, st));                                                    // slots another shard fills stay marked
	}
	if (q.max_areas()) {
		job.area_hdr_bytes = pl.area_hdr_bytes;
		job.area_bytes = pl.area_bytes;
		if (int rc = h->d_areas.ensure(job.area_hdr_bytes + job.area_bytes); rc) return rc;
		RX_HIP(hipMemsetAsync(h->d_areas.ptr, 0, job.area_hdr_bytes, st));
		p.max_areas = q.max_areas();
		p.area_fields = h->num_fields;
		p.area_hdr = static_cast<uint32_t*>(h->d_areas.ptr);
		p.out_areas = reinterpret_cast<uint32_t*>(static_cast<char*>(h->d_areas.ptr) + job.area_hdr_bytes);
	}
	std::memcpy(hp + pl.state.plan_self.off, &p, sizeof(p));
	job.d_plan = reinterpret_cast<const rxgpu::FtPlan*>(base + pl.state.plan_self.off);
	job.dev_base = base;
	job.max_merged = pl.max_merged;
	job.merged_postings = pl.merged_postings;
	job.plan_bytes = pl.state.plan_bytes;
	job.hp_dev = hp_dev;
	job.nsyn = pl.nsyn;
	if (import_now) RX_HIP(rxgpu::launch_ft_import(hp_dev, base, pl.state.plan_bytes, st));   // plan_bytes is a multiple of 256
	return RXGPU_OK;
}

double us_since(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count(); }

// Rows, limits and layouts of a merge whose phrases have run, then the execution.  `given`: the phrases' rows as the sharded layer settled them.
int plan_and_execute(rxgpu_ft_index* h, hipStream_t st, const MergeQuery& q, MergePrep& mp, bool resident, bool phrases_given, MergeJob& job, bool import_now,
					 std::chrono::steady_clock::time_point t_begin) {
	for (uint32_t pi = 0; pi < mp.plan.nparts; ++pi) {   // (statistics: counted whether or not the checks below let the merge run)
		if (mp.plan.parts[pi].phrase) h->stat_postings += mp.phrase_rows[pi].postings;
	}
	if (rxgpu::FtPlanError e = rxgpu::ft_plan_rows(mp.facts, PhraseView{mp.phrase_rows}, kStructSizes, mp.plan); e) return plan_error(e);
	h->trace_us[0] += us_since(t_begin);
	const auto t_stage = std::chrono::steady_clock::now();
	if (int rc = execute_plan(h, st, q, mp, resident, phrases_given, job, import_now); rc) return rc;
	h->trace_us[1] += us_since(t_stage);
	return RXGPU_OK;
}

}  // namespace

namespace rxgpu {

// A whole merge prepared on `st`: the query's phrases run here.  job.empty: nothing is merged.
int prepare_merge(rxgpu_ft_index* h, hipStream_t st, const MergeQuery& q, bool resident, OutRoom room, MergeJob& job, bool import_now) {
	const auto t_begin = std::chrono::steady_clock::now();
	MergePrep mp;
	if (int rc = begin_merge(h, st, q, resident, room, mp); rc) return rc;
	job.empty = mp.plan.empty;
	if (job.empty) return RXGPU_OK;
	if (int rc = run_query_phrases(h, q, mp, false); rc) return rc;
	return plan_and_execute(h, st, q, mp, resident, false, job, import_now, t_begin);
}

// A document-range shard, first visit: the query's phrases through their admission pass only — the sharded layer settles the admission cut of
// the whole index before any shard goes on (finish_phrase).  *empty: nothing is merged, alike on every shard.
int prepare_shard_phrases(rxgpu_ft_index* h, const MergeQuery& q, std::vector<PhraseRows>& phrases, bool* empty) {
	MergePrep mp;
	if (int rc = begin_merge(h, h->stream, q, false, OutRoom{true, q.cfg->merge_limit}, mp); rc) return rc;
	*empty = mp.plan.empty;
	if (mp.plan.empty) return RXGPU_OK;
	if (int rc = run_query_phrases(h, q, mp, true); rc) return rc;
	phrases = std::move(mp.phrase_rows);
	return RXGPU_OK;
}

// A document-range shard, the merge itself.  `phrases`: the rows of the query's phrases, `admitted` holding the sum over the shards (the 2-phase
// estimate is a fact of the whole index); null: the query has none.
int prepare_shard_merge(rxgpu_ft_index* h, const MergeQuery& q, const std::vector<PhraseRows>* phrases, MergeJob& job) {
	if (!phrases) return prepare_merge(h, h->stream, q, false, OutRoom{true, q.cfg->merge_limit}, job, true);
	const auto t_begin = std::chrono::steady_clock::now();
	MergePrep mp;
	if (int rc = begin_merge(h, h->stream, q, false, OutRoom{true, q.cfg->merge_limit}, mp); rc) return rc;
	job.empty = mp.plan.empty;
	if (job.empty) return RXGPU_OK;
	RX_CHECK(phrases->size() == mp.plan.nparts, RXGPU_ERR_LOGIC, std::string(q.who) + ": phrase rows of another query");
	mp.phrase_rows = *phrases;
	for (const QueryPartIn& part : mp.plan.parts) mp.n_phrases += part.phrase ? 1 : 0;
	return plan_and_execute(h, h->stream, q, mp, false, true, job, true, t_begin);
}

// Second half: the merged documents out of the lane's pinned staging buffer (ft_export wrote them there; the stream has been waited for).
int collect_merge(rxgpu_ft_index* h, const MergeJob& job, const MergeOut& out, const char* who) {
	const char* hp = static_cast<const char*>(h->h_pinned);
	const rxgpu::FtOutLayout ol = rxgpu::ft_out_layout(job.max_merged);
	const uint32_t* hdr = reinterpret_cast<const uint32_t*>(hp + ol.header);
	if (int rc = check_result_header(hdr, job.max_merged, who); rc) return rc;
	const uint64_t n = hdr[0];
	h->clean_dirty = false;   // the merge ran to its end: ft_adders / ft_finish handed the tables back zeroed
	uint64_t kept = n;
	if (n && job.nsyn) {   // the documents that hold only parts of a multi-word synonym go (mergerimpl.h:533-555): the rest keeps its order
		const uint32_t* sd = reinterpret_cast<const uint32_t*>(hp + ol.doc);
		const float* sp = reinterpret_cast<const float*>(hp + ol.proc);
		const uint16_t* st_ = reinterpret_cast<const uint16_t*>(hp + ol.terms_counter);
		const uint8_t* sf = reinterpret_cast<const uint8_t*>(hp + ol.field);
		kept = 0;
		for (uint64_t i = 0; i < n; ++i) {
			if (st_[i] == 0xFFFFu) continue;
			out.doc[kept] = sd[i];
			out.proc[kept] = sp[i];
			if (out.terms_counter) out.terms_counter[kept] = st_[i];
			out.field[kept] = sf[i];
			++kept;
		}
	} else if (n) {
		std::memcpy(out.doc, hp + ol.doc, n * 4);
		std::memcpy(out.proc, hp + ol.proc, n * 4);
		if (out.terms_counter) std::memcpy(out.terms_counter, hp + ol.terms_counter, n * 2);
		std::memcpy(out.field, hp + ol.field, n);
	}
	*out.n = kept;
	if (out.preselected) *out.preselected = hdr[2] ? 1 : 0;
	return RXGPU_OK;
}

}  // namespace rxgpu

namespace {
// RXGPU_FT_STAMPS: the phase stamps of the merge that just ended, summed into the lane
int read_stamps(rxgpu_ft_index* h, const rxgpu::FtPlan& p) {
	unsigned long long raw[64];
	RX_HIP(hipMemcpy(raw, p.dbg, sizeof(raw), hipMemcpyDeviceToHost));
	RX_HIP(hipMemset(p.dbg, 0, sizeof(raw)));
	const int groups[][2] = {{0, 16}, {16, 24}, {24, 32}, {32, 48}};
	for (const auto& g : groups) {
		for (int k = g[0]; k < g[1]; ++k) {
			if (raw[k] && raw[g[0]]) h->stamps[k] += double(raw[k] - raw[g[0]]) * 0.01;   // 100 MHz -> us
		}
	}
	return RXGPU_OK;
}
}  // namespace

namespace rxgpu {

// One merge on lane `h` (locked by the caller) into the caller's lists, or — resident — left in HBM for the hybrid fusion.
int run_merge(rxgpu_ft_index* h, const MergeQuery& q, const MergeOut& out, bool resident) {
	using clk = std::chrono::steady_clock;
	const char* who = q.who;
	if (h->shard_set) {   // document-range shards: the same train on every shard, two exchanges between its pieces
		RX_CHECK(!resident, RXGPU_ERR_LOGIC, std::string(who) + ": a sharded ft index merges into the caller's lists (no resident results)");
		RX_CHECK(out.complete(q.simple), RXGPU_ERR_OVERFLOW, std::string(who) + ": output buffers too small");
		return run_merge_sharded(h, q, out);
	}
	if (int rc = finish_pending(h, who); rc) return rc;
	hipStream_t st = h->stream;
	MergeJob job;
	if (int rc = prepare_merge(h, st, q, resident, OutRoom{out.complete(q.simple), out.cap}, job, true); rc) return rc;
	if (job.empty) return RXGPU_OK;
	const rxgpu::FtPlan& p = job.p;
	const auto t_launch = clk::now();
	if (!h->ev_a) {
		RX_HIP(hipEventCreate(&h->ev_a));
		RX_HIP(hipEventCreate(&h->ev_b));
	}
	// from here on an error return leaves the kept-clean tables in an unknown state: the next merge clears them first
	h->clean_dirty = true;
	RX_HIP(hipEventRecord(h->ev_a, st));
	if (p.sparse) {
		RX_HIP(rxgpu::launch_ft_merge_sparse(job.d_plan, &job.p, 1, st));
	} else {
		RX_HIP(rxgpu::launch_ft_merge(job.d_plan, &job.p, 1, st));
	}
	RX_HIP(hipEventRecord(h->ev_b, st));
	(h->root ? h->root : h)->trains_dense += p.sparse ? 0 : 1;
	(h->root ? h->root : h)->trains_sparse += p.sparse ? 1 : 0;
	if (resident) {   // the result stays where ft_finish wrote it (d_out): the fusion kernel reads it there, nothing travels
		h->res_pending = true;
		h->res_has_syn = job.nsyn != 0;   // the fusion skips the documents ft_finish marked (they hold only parts of a synonym)
		h->prep_done = false;
		h->res_cap = uint32_t(job.max_merged);
		h->stat_postings += job.merged_postings;
		h->trace_us[2] += us_since(t_launch);
		h->trace_us[5] += 1;
		return RXGPU_OK;
	}
	RX_HIP(rxgpu::launch_ft_export(job.d_plan, &job.p, 1, st));
	const AreasOut* areas = q.areas;
	std::vector<uint32_t> area_hdr;
	if (areas) {   // {held, insertions} per (document, field) and the areas, as the replay left them (the wait below covers the copies)
		area_hdr.resize(size_t(job.max_merged) * h->num_fields * 2);
		RX_HIP(hipMemcpyAsync(area_hdr.data(), p.area_hdr, area_hdr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		RX_HIP(hipMemcpyAsync(areas->areas, p.out_areas, job.area_bytes, hipMemcpyDeviceToHost, st));
	}
	h->trace_us[2] += us_since(t_launch);
	const auto t_wait = clk::now();
	// (the result is already on its way: ft_export, the last kernel of the train, writes it into the pinned staging buffer)
	if (int rc = wait_stream_polled(st); rc) return rc;
	if (p.dbg) {
		if (int rc = read_stamps(h, p); rc) return rc;
	}
	h->trace_us[3] += us_since(t_wait);
	const auto t_unpack = clk::now();
	float ms = 0.f;
	(void)hipEventElapsedTime(&ms, h->ev_a, h->ev_b);
	h->stat_postings += job.merged_postings;
	h->stat_ms += ms;
	if (int rc = collect_merge(h, job, out, who); rc) return rc;
	if (areas) {
		RX_HIP(hipStreamSynchronize(st));   // (the polling above may have ended on the export kernel: the two copies behind it too, now)
		const size_t nf = h->num_fields;
		for (uint64_t i = 0; i < *out.n; ++i) {
			for (size_t f = 0; f < nf; ++f) areas->cnt[i * nf + f] = area_hdr[(i * nf + f) * 2];
		}
	}
	h->trace_us[4] += us_since(t_unpack);
	h->trace_us[5] += 1;
	return RXGPU_OK;
}

}  // namespace rxgpu
