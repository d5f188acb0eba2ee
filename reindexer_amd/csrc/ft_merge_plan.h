// The decisions of ONE BM25 merge, without HIP: what prepare_merge (rxgpu_ft_merge.hip) decides before it touches the device — the query
// parts, the volume and the 2-phase gate's host half, the launch train, the table of merged sub-term rows with its grid, the synonym mask
// jobs, the layouts of the three device buffers and every engine limit that is a fact of the query alone.  Inputs are plain facts (the
// caller looks the words up in the dictionary and says what it found), so the rules compile with a host compiler and are pinned on the CPU
// (tests/cpp/ft_merge_plan_cpu.cc, tests/test_ft_merge_plan.py).  The counterpart of hnsw_launch_plan.h for the FT path.
//
// Errors come back as (code, message) pairs, in the order the checks fire: callers and tests see the first one.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rxgpu.h"

#if defined(__HIPCC__)
#define RX_FT_HD __host__ __device__
#else
#define RX_FT_HD
#endif

namespace rxgpu {

constexpr int kFtPassItems = 4;            // postings per thread in the posting-side kernels
constexpr uint32_t kFtRangeDocs = 8192;    // documents per workgroup of the document-range kernel (ft_ranges); multiple of 32
constexpr int kFtBlockPostings = 256 * kFtPassItems;
inline uint32_t ft_pass_blocks(uint64_t n) { return uint32_t((n + kFtBlockPostings - 1) / kFtBlockPostings); }
constexpr int kFtApplyWords = 4;           // mask words per thread in ft_preselect_apply
// workgroups of ft_preselect_apply over `nwords` mask words = the words of its look-back chain (FtCleanLayout::lb_pre, zeroed by ft_adders)
RX_FT_HD inline uint64_t ft_apply_blocks(uint64_t nwords) { return (nwords + 256 * kFtApplyWords - 1) / (256 * kFtApplyWords); }
constexpr int kFtRankTiles = 2;            // tiles of kFtBlockPostings postings per workgroup of ft_rank_all
constexpr uint32_t kFtSparseSubs = 16;     // sub-terms (NOT terms' included) a sparse merge holds bitmaps for
constexpr uint32_t kFtHistCopies = 8, kFtHistStride = 65536 + 1024;
constexpr uint32_t kFtSyncWords = 16;      // the kFtSync* words of a merge (rxgpu_internal.h names them)
constexpr uint32_t kFtBatchMax = 64;       // merges in one launch train (rxgpu_ft_merge_batch_raw)
constexpr int kFtPlanBm25Classic = 1;      // rxgpu_ft_config::bm25_type of Bm25Classic (ft_rank.hip.h: kFtBm25Classic)

struct FtGridEntry {           // block range of one sub-term in a posting-side grid (blocks of kFtBlockPostings postings)
	uint32_t block_base;
	uint32_t sub;              // index into FtPlan::subs
};
// Multi-word synonyms (QueryMergeData::synonyms, querymergedata.h:178-192): their terms follow the query parts in FtPlan::terms (op = OR for
// the pre-score pass: calcTermScores counts them like any term, mergerimpl.h:393-397, and they never restrict on their own)
struct FtSynonym {
	uint32_t term_begin, term_end;   // its terms in FtPlan::terms
	uint32_t end_qp;                 // qp of its last term (every term takes a qp, NOT terms too: mergerimpl.h:511-514)
	uint32_t nterms;                 // Synonym::NumTerms()
};

inline size_t ft_align256(size_t v) { return (v + 255) & ~size_t(255); }
// A region of a carved buffer
struct FtRegion {
	size_t off = 0, bytes = 0;
};
// Carves regions out of one growable device buffer; every region starts on a 256-byte boundary
struct FtCarver {
	size_t off = 0;
	size_t take(size_t bytes) {
		const size_t at = off;
		off = ft_align256(off + bytes);
		return at;
	}
	FtRegion region(size_t bytes) { return FtRegion{take(bytes), bytes}; }
};

// ---------------------------------------------------------------------------------------------------------------------- the inputs
struct QueryTermIn {
	int32_t op;
	const rxgpu_ft_term_opts* opts;
	uint32_t sub_begin, sub_end;
	int32_t phrase_num = -1;   // FtDslOpts::phraseNum: consecutive terms with the same number >= 0 are one phrase (selecterimpl.h:482-572)
	int32_t distance = 1;      // FtDslOpts::distance (the phrase's terms)
};
// multi-word synonyms of a query (rxgpu_ft_query): their terms are terms[first_term ..] of run_merge's list
struct SynonymsIn {
	uint32_t nsyn = 0, first_term = 0;
	const uint32_t* syn_term_off = nullptr;   // [nsyn + 1], relative to first_term
	const uint32_t* part_syn_off = nullptr;   // [nparts + 1]
	const uint32_t* part_syn = nullptr;
	const uint8_t* suppressed = nullptr;      // per sub-term
};
// a query part (PhraseOrTerm, querymergedata.h:145-176): one plain term or the terms [t_begin, t_end) of one phrase
struct QueryPartIn {
	bool phrase;
	uint32_t t_begin, t_end;
};
// what the dictionary holds of one sub-term's word
struct FtSubFact {
	uint64_t n = 0;              // postings of the list on this handle (a document-range shard: of its fragment)
	uint64_t df = 0;             // document frequency over the whole index (word_df)
	uint32_t last_doc = 0;       // largest document id of the list
	bool found = false;          // the dictionary knows the word id
	bool has_positions = false;  // uploaded with its positions (rxgpu_ft_set_word_positions / _packed)
	const void* source = nullptr;   // the caller's own (its dictionary entry); the plan never looks at it
};
struct FtMergeFacts {
	const QueryTermIn* terms = nullptr;   // the query parts' terms, then the synonyms' terms
	uint32_t nterms = 0;
	const SynonymsIn* synonyms = nullptr;
	const FtSubFact* subs = nullptr;      // per sub-term of the caller's list
	const float* procs = nullptr;
	const rxgpu_ft_config* cfg = nullptr;
	uint32_t num_fields = 0;
	const float* h_avg = nullptr;         // avg_words as uploaded, [n_avg]
	uint32_t n_avg = 0;
	uint64_t total_docs = 0;
	uint32_t sh_total = 0;                // document-range shards of the index this handle is one of (0 / 1: unsharded)
	int train_mode = -1;                  // -1 the plan decides, 0 always dense, 1 sparse whenever eligible
	bool simple = false, resident = false;
	uint32_t max_areas = 0;
	bool have_outs = true;                // the caller's output lists are all there ...
	uint64_t cap = 0;                     // ... with room for `cap` documents
	const char* who = "";
};
// sizes of the device structs the plan region holds (rxgpu_internal.h; HIP types, so the executor names them)
struct FtStructSizes {
	size_t subterm = 0, term_cfg = 0, syn_job = 0, plan = 0, record = 16;
};

struct FtPlanError {
	int code = RXGPU_OK;
	std::string msg;
	explicit operator bool() const { return code != RXGPU_OK; }
};
#define RX_PLAN_CHECK(cond, err, text)                               \
	do {                                                             \
		if (!(cond)) return FtPlanError{err, std::string(who) + text}; \
	} while (0)

// ---------------------------------------------------------------------------------------------------------------------- the plan
// One kept sub-term (a word with postings somewhere in the index, or a row of a phrase) in FtPlan::subs order
struct FtRow {
	uint32_t term = 0;          // -> FtPlan::terms: the part, or nparts + the synonym term
	uint32_t src = 0;           // the sub-term `si` of the caller's list; a phrase row: its index among the phrase's rows
	uint32_t row = 0;           // index among the merged (non-NOT) rows; 0 for a NOT term's
	uint32_t attr = 0;          // the sparse train's attribute word (FtPlan::SpSub::attr); 0 on the dense train
	uint16_t qp = 0, prev_term_qp = 0, ord_in_term = 0;
	uint8_t suppressed = 0, phrase = 0;
};
struct FtPlanTerm {             // one entry of FtPlan::terms
	uint32_t sub_begin = 0, sub_end = 0;
	int32_t op = 1;
	bool same_boost = true, all_pos_boost = true, phrase = false;
};
struct FtSynJob {               // an AND part whose term mask takes its synonyms' masks in (ft_syn_masks)
	uint32_t part, syn_begin, syn_end;   // into job_syns
};
struct FtStateLayout {          // d_state: the plan region (uploaded in one copy), then the per-merge tables
	FtRegion plan_subs, plan_terms, plan_mgrid, plan_fc, plan_syns, plan_jobs, plan_jsyn, plan_self;
	size_t cfg_floats = 0, plan_bytes = 0;
	FtRegion mask, synmask, score, brec, boff, adders, eidx, efield, tdoc, tpos, tidx;
	size_t bytes = 0;
};
struct FtCleanLayout {          // d_clean: the tables every merge finds zeroed and leaves zeroed
	FtRegion hist, lb_pre, bcnt, sync, dbg, lb_units, erank;
	size_t bytes = 0;
};
// The packed result: header (4 x u32: numDocs, error flag, preselected, 0), then doc / proc / terms_counter / field over max_merged
struct FtOutLayout {
	size_t header = 0, doc = 0, proc = 0, terms_counter = 0, field = 0, bytes = 0;
};
inline FtOutLayout ft_out_layout(uint64_t max_merged) {
	const size_t M = size_t(max_merged);
	FtOutLayout o;
	o.doc = ft_align256(16);
	o.proc = o.doc + ft_align256(M * 4);
	o.terms_counter = o.proc + ft_align256(M * 4);
	o.field = o.terms_counter + ft_align256(M * 2);
	o.bytes = o.field + ft_align256(M);
	return o;
}

struct FtMergePlan {
	// ---- ft_plan_volume
	std::vector<QueryPartIn> parts;
	std::vector<uint64_t> term_postings;   // MaxVDocs per term (the whole index's)
	uint32_t nparts = 0, npart_terms = 0, nsyn = 0, nsyn_terms = 0;
	uint64_t total_vids = 0, max_merged = 0;
	bool empty = false;                    // min(mergeLimit, totalORVids) == 0: nothing is merged
	bool any_phrase = false, sparse = false;
	size_t n_subs_kept = 0;
	uint64_t local_postings = 0;
	// ---- ft_plan_rows
	uint64_t est_or = 0, est_and = UINT64_MAX;
	bool prescore = false;
	uint32_t query_len = 0;
	std::vector<FtRow> rows;
	std::vector<FtPlanTerm> terms;         // [nparts + nsyn_terms]
	std::vector<FtGridEntry> merge_grid;
	uint64_t merge_blocks = 0, merged_postings = 0;
	uint32_t n_rows = 0, n_part_qp = 0;
	std::vector<FtSynonym> syns;
	std::vector<FtSynJob> jobs;
	std::vector<uint32_t> job_syns;
	bool sp_empty_and = false;
	uint64_t nwords = 0;
	uint32_t n_ranges = 0;
	FtStateLayout state;
	FtCleanLayout clean;
	FtOutLayout out;
	size_t area_hdr_bytes = 0, area_bytes = 0;   // MergeDataAreas: the two regions of d_areas
};

// ---------------------------------------------------------------------------------------------------------------------- the rules
// The query parts (selecterimpl.h:482-572): consecutive terms with the same phraseNum >= 0 are one phrase
inline void ft_query_parts(const QueryTermIn* terms, uint32_t nterms, std::vector<QueryPartIn>& parts) {
	parts.clear();
	for (uint32_t t = 0; t < nterms;) {
		if (terms[t].phrase_num < 0) {
			parts.push_back({false, t, t + 1});
			++t;
			continue;
		}
		uint32_t e = t + 1;
		while (e < nterms && terms[e].phrase_num == terms[t].phrase_num) ++e;
		parts.push_back({true, t, e});
		t = e;
	}
}
// QueryMergeData::Empty() / Simple() (querymergedata.h:208) over the parts' terms, without building the parts
struct FtQueryClass {
	uint32_t nparts = 0;
	bool empty = true, simple = false;
};
inline FtQueryClass ft_classify_query(const QueryTermIn* terms, uint32_t nterms) {
	FtQueryClass c;
	for (uint32_t t = 0; t < nterms; ++t) {
		if (terms[t].phrase_num < 0 || t == 0 || terms[t - 1].phrase_num != terms[t].phrase_num) ++c.nparts;
	}
	if (nterms == 0) return c;
	c.empty = c.nparts == 1 && terms[0].op == 3;
	c.simple = c.nparts == 1 && terms[0].op != 3 && terms[0].phrase_num < 0;
	return c;
}

// FtDslOpts of a term as the kernels want it
inline FtPlanError ft_check_term_opts(const QueryTermIn& qt, uint32_t nf, const char* who, bool& same, bool& all_pos) {
	RX_PLAN_CHECK(qt.opts->field_boost && qt.opts->need_sum_rank, RXGPU_ERR_PARAMS, ": null term options");
	uint32_t nsum = 0;
	same = true;
	all_pos = true;
	for (uint32_t f = 0; f < nf; ++f) {
		nsum += qt.opts->need_sum_rank[f] ? 1 : 0;
		same = same && qt.opts->field_boost[f] == qt.opts->field_boost[0];
		all_pos = all_pos && qt.opts->field_boost[f] != 0.0f;
	}
	RX_PLAN_CHECK(nsum <= 8, RXGPU_ERR_PARAMS, ": more than 8 fields with needSumRank (GPU engine limit)");
	RX_PLAN_CHECK(qt.sub_end - qt.sub_begin <= 4096, RXGPU_ERR_PARAMS, ": more than 4096 sub-terms in one term (GPU engine limit)");
	return {};
}
// what every sub-term of a merged term must satisfy, whatever kind of term it belongs to (a phrase's, a plain one, a synonym's)
inline FtPlanError ft_check_subterm(const QueryTermIn& qt, uint32_t si, const FtSubFact& w, const float* procs, bool need_positions, const char* who) {
	RX_PLAN_CHECK(!need_positions || w.n == 0 || w.has_positions, RXGPU_ERR_LOGIC, ": the word was uploaded without positions (rxgpu_ft_set_word_positions)");
	RX_PLAN_CHECK(si == qt.sub_begin || procs[si] <= procs[si - 1], RXGPU_ERR_PARAMS, ": sub-terms must be sorted by proc, descending (SortSubterms)");
	return {};
}

// The sparse train (ft_sparse.hip) derives every per-document fact from one bitmap per sub-term and ranks a document only once its merge slot
// is known.  That is the reference's merge exactly when
//   * the query is made of plain terms (no phrase rows, no multi-word synonyms, no areas) with at most kFtSparseSubs sub-terms,
//   * every field of every merged term has the same positive boost — calcTermBitmask / calcTermScores then never look at an occurrence's
//     fields (mergerimpl.h:252-324: allFieldsHaveSameBoost; checkFieldsRelevance is true for every occurrence),
//   * calcTermRank cannot return 0 for any posting, so that "added by its first posting with a non-zero rank" (merger.h:161-180) is "added
//     by its first posting": Bm25Rx / TermCount (positive, finite for avg_words > 0), every weight below 1 and every boost >= 0, which
//     bounds each factor of phrasemergerimpl.h:51-63 from below by (1 - weight) > 0; the product's lower bound must stay a normal float.
inline bool ft_sparse_eligible(const FtMergeFacts& f, size_t n_subs, size_t n_phrases) {
	const rxgpu_ft_config* cfg = f.cfg;
	const uint32_t nsyn = f.synonyms ? f.synonyms->nsyn : 0;
	if (f.sh_total > 1 || n_phrases || nsyn || f.max_areas) return false;
	if (n_subs == 0 || n_subs > kFtSparseSubs || f.nterms > 32) return false;
	if (cfg->bm25_type == kFtPlanBm25Classic) return false;   // TF = count / wordsInDoc: a field without words makes the rank NaN, which is never admitted
	if (!(cfg->bm25_k1 >= 0.0) || !(cfg->bm25_b >= 0.0 && cfg->bm25_b <= 1.0) || !(cfg->summation_ranks_by_fields_ratio >= 0.0)) return false;
	const uint32_t nf = f.num_fields;
	if (f.n_avg != nf) return false;
	double floor_fields = 1.0;   // lower bound of norm * termLenBoost * positionRank over the fields
	for (uint32_t k = 0; k < nf; ++k) {
		if (!(f.h_avg[k] > 0.0f) || !std::isfinite(f.h_avg[k])) return false;
		const double w[3] = {cfg->bm25_weight[k], cfg->term_len_weight[k], cfg->position_weight[k]};
		const double b[3] = {cfg->bm25_boost[k], cfg->term_len_boost[k], cfg->position_boost[k]};
		double fl = 1.0;
		for (int j = 0; j < 3; ++j) {
			if (!(w[j] >= 0.0 && w[j] <= 0.999) || !(b[j] >= 0.0) || !std::isfinite(b[j])) return false;
			fl *= 1.0 - w[j];
		}
		floor_fields = std::min(floor_fields, fl);
	}
	for (uint32_t t = 0; t < f.nterms; ++t) {
		const QueryTermIn& qt = f.terms[t];
		if (qt.phrase_num >= 0) return false;
		if (qt.op == 3) continue;   // a NOT term only clears mask bits, whatever its options (excludeTermFromBitmask, mergerimpl.h:276-287)
		const float fb = qt.opts->field_boost[0];
		if (!(fb > 0.0f) || !std::isfinite(fb)) return false;
		for (uint32_t k = 1; k < nf; ++k) {
			if (qt.opts->field_boost[k] != fb) return false;
		}
		if (!(qt.opts->boost > 0.0f) || !std::isfinite(qt.opts->boost) || !(qt.opts->term_len_boost >= 0.0f) || !std::isfinite(qt.opts->term_len_boost)) return false;
		for (uint32_t si = qt.sub_begin; si < qt.sub_end; ++si) {
			if (!(f.procs[si] > 0.0f) || !std::isfinite(f.procs[si])) return false;
			if (double(fb) * floor_fields * double(qt.opts->boost) * double(f.procs[si]) < 1e-30) return false;
		}
	}
	return true;
}

// Parts, volume, train: everything that is decided before the query's phrases run.  p.empty: nothing is merged (and nothing else is set).
inline FtPlanError ft_plan_volume(const FtMergeFacts& f, FtMergePlan& p) {
	const char* who = f.who;
	const rxgpu_ft_config* cfg = f.cfg;
	const SynonymsIn* synonyms = f.synonyms;
	const uint64_t N = f.total_docs;
	p.nsyn = synonyms ? synonyms->nsyn : 0;
	p.npart_terms = p.nsyn ? synonyms->first_term : f.nterms;
	p.nsyn_terms = f.nterms - p.npart_terms;
	RX_PLAN_CHECK(cfg->bm25_type >= 0 && cfg->bm25_type <= 2, RXGPU_ERR_PARAMS, ": bm25_type must be 0 (rx), 1 (classic) or 2 (wordCount)");
	ft_query_parts(f.terms, p.npart_terms, p.parts);
	const uint32_t nparts = p.nparts = uint32_t(p.parts.size());
	RX_PLAN_CHECK(nparts < 0x7FFF, RXGPU_ERR_PARAMS, ": too many query parts");
	RX_PLAN_CHECK(!f.simple || (nparts == 1 && !p.parts[0].phrase && !p.nsyn), RXGPU_ERR_LOGIC, ": a phrase is not a Simple() query");
	if (p.nsyn) {
		RX_PLAN_CHECK(synonyms->syn_term_off && synonyms->part_syn_off && synonyms->syn_term_off[0] == 0 && synonyms->syn_term_off[p.nsyn] == p.nsyn_terms &&
						  synonyms->part_syn_off[0] == 0,
					  RXGPU_ERR_PARAMS, ": inconsistent synonym tables");
		for (uint32_t k = 0; k < synonyms->part_syn_off[nparts]; ++k) {
			RX_PLAN_CHECK(synonyms->part_syn && synonyms->part_syn[k] < p.nsyn, RXGPU_ERR_PARAMS, ": synonym id out of range");
		}
	}
	p.term_postings.assign(f.nterms, 0);
	p.total_vids = 0;
	p.n_subs_kept = 0;
	p.local_postings = 0;
	for (uint32_t t = 0; t < f.nterms; ++t) {
		const QueryTermIn& qt = f.terms[t];
		for (uint32_t si = qt.sub_begin; si < qt.sub_end; ++si) {
			const FtSubFact& w = f.subs[si];
			RX_PLAN_CHECK(w.found, RXGPU_ERR_NOTFOUND, ": unknown word id");
			// the kernels index words_in_field[doc * fields + f] and an (N + 31) / 32-word mask by document: a list reaching past the
			// documents rxgpu_ft_set_docs described would read and write out of bounds (set_docs may follow the words, so it is checked here)
			RX_PLAN_CHECK(w.n == 0 || w.last_doc < N, RXGPU_ERR_PARAMS, ": a posting list holds a document id >= total_docs (rxgpu_ft_set_docs)");
			p.term_postings[t] += w.df;   // (a document-range shard: the whole index's count — limits and gates are global facts)
			if (w.df) {
				++p.n_subs_kept;
				p.local_postings += w.n;
			}
		}
		p.total_vids += p.term_postings[t];   // totalORVids: MaxVDocs of every term, whatever its operator and inside phrases too (selecterimpl.h:546)
	}
	RX_PLAN_CHECK(p.total_vids < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, ": more than 2^32 postings in one merge");
	p.max_merged = std::min<uint64_t>(cfg->merge_limit, p.total_vids);   // Merge(): min(mergeLimit, totalORVids)
	p.empty = p.max_merged == 0;
	if (p.empty) return {};
	RX_PLAN_CHECK(f.resident || (f.cap >= p.max_merged && f.have_outs), RXGPU_ERR_OVERFLOW, ": output buffers too small");
	p.any_phrase = false;
	for (const QueryPartIn& part : p.parts) p.any_phrase = p.any_phrase || part.phrase;
	// the launch train: the sparse one for eligible queries whose postings lie on a fraction of the documents (or on request)
	p.sparse = false;
	if (f.train_mode != 0 && ft_sparse_eligible(f, p.n_subs_kept, p.any_phrase ? 1 : 0)) {
		p.sparse = f.train_mode == 1 || p.local_postings * 10 <= N * 3;   // dense queries keep the dense train (posting-parallel ranking, per-range workgroups)
	}
	return {};
}

// The three device buffers of a merge whose rows are known
inline void ft_plan_layouts(const FtMergeFacts& f, const FtStructSizes& sz, FtMergePlan& p) {
	const uint32_t nf = f.num_fields;
	const uint64_t N = f.total_docs, nwords = p.nwords = (N + 31) / 32;
	const size_t M = size_t(p.max_merged);
	const uint32_t n_rows = p.n_rows, n_ranges = p.n_ranges = uint32_t((N + kFtRangeDocs - 1) / kFtRangeDocs);
	const uint32_t nplan_terms = p.nparts + p.nsyn_terms;
	const bool sparse = p.sparse;
	FtStateLayout& s = p.state;
	FtCarver cv;
	s.plan_subs = cv.region(std::max<size_t>(1, p.rows.size()) * sz.subterm);
	s.plan_terms = cv.region(size_t(nplan_terms) * sz.term_cfg);
	s.plan_mgrid = cv.region(std::max<size_t>(1, p.merge_grid.size()) * sizeof(FtGridEntry));
	s.cfg_floats = size_t(6) * nf + size_t(nplan_terms) * nf;
	s.plan_fc = cv.region(s.cfg_floats * sizeof(float) + size_t(nplan_terms) * nf);
	s.plan_syns = cv.region(std::max<size_t>(1, p.syns.size()) * sizeof(FtSynonym));
	s.plan_jobs = cv.region(std::max<size_t>(1, p.jobs.size()) * sz.syn_job);
	s.plan_jsyn = cv.region(std::max<size_t>(1, p.job_syns.size()) * 4);
	s.plan_self = cv.region(sz.plan);   // the FtPlan itself: the kernels read it from HBM (a batch of one)
	s.plan_bytes = cv.off;              // everything above is uploaded in one copy
	// (a sparse merge keeps nothing per document or per posting in HBM: ft_sparse.hip)
	s.mask = cv.region(sparse ? 0 : nwords * 4);
	s.synmask = cv.region(p.jobs.size() * nwords * 4);
	s.score = cv.region(p.prescore && !sparse ? nwords * 32 * 2 : 0);   // padded to whole mask words (ft_preselect_apply reads 32 scores at a time)
	s.brec = cv.region(sparse ? 0 : size_t(p.merged_postings) * sz.record);
	s.boff = cv.region(size_t(n_ranges) * 4);
	s.adders = cv.region(std::max<size_t>(1, size_t(n_rows) * n_ranges) * 4);
	s.eidx = cv.region(sparse ? 0 : size_t(n_rows) * M * 4);
	s.efield = cv.region(sparse ? 0 : size_t(n_rows) * M);
	s.tdoc = cv.region(sparse ? M * 4 : 0);
	s.tpos = cv.region(sparse ? M * 4 : 0);
	s.tidx = cv.region(sparse ? M * std::max<size_t>(1, n_rows) * 4 : 0);
	s.bytes = cv.off;
	// the kept-clean tables: sized by the corpus only, so that they stay where they are from merge to merge
	FtCleanLayout& c = p.clean;
	FtCarver cc;
	c.hist = cc.region(size_t(kFtHistCopies) * kFtHistStride * 4);   // copies of (fine + coarse)
	c.lb_pre = cc.region(ft_apply_blocks(nwords) * 8);
	c.bcnt = cc.region(size_t(n_ranges) * 4);
	c.sync = cc.region(kFtSyncWords * 4);
	c.dbg = cc.region(64 * 8);
	c.lb_units = cc.region(size_t(n_ranges) * 8);
	c.erank = cc.region(sparse ? 0 : size_t(n_rows) * M * 4);   // last: the regions before it never move when a query needs more rows
	c.bytes = cc.off;
	p.out = ft_out_layout(p.max_merged);
	p.area_hdr_bytes = p.area_bytes = 0;
	if (f.max_areas) {
		p.area_hdr_bytes = ft_align256(M * nf * 2 * sizeof(uint32_t));
		p.area_bytes = M * nf * size_t(f.max_areas) * 3 * sizeof(uint32_t);
	}
}

// Gate, rows, limits, layouts: everything behind the phrases.  `phrases` tells what ft_phrase.hip made of the phrase parts:
//   phrases.admitted(pi)   PhraseMerger::NumDocsMerged() (a document-range shard: the sum over the shards)
//   phrases.n_rows(pi)     rows of the phrase,  phrases.row_n(pi, r)   documents of row r
template <typename PhraseView>
FtPlanError ft_plan_rows(const FtMergeFacts& f, const PhraseView& phrases, const FtStructSizes& sz, FtMergePlan& p) {
	const char* who = f.who;
	const rxgpu_ft_config* cfg = f.cfg;
	const SynonymsIn* synonyms = f.synonyms;
	const uint64_t N = f.total_docs;
	const uint32_t nparts = p.nparts, nsyn = p.nsyn, npart_terms = p.npart_terms;

	// 2-phase gate, host half (estimateNumDocsInMerge, merger.h:239-267; mergerimpl.h:486-490)
	p.est_or = 0;
	p.est_and = UINT64_MAX;
	p.query_len = 0;
	for (uint32_t pi = 0; pi < nparts; ++pi) {
		const QueryPartIn& part = p.parts[pi];
		p.query_len += part.t_end - part.t_begin;
		const int32_t op = f.terms[part.t_begin].op;   // PhraseResults::Op(): its first term's
		if (op == 3) continue;
		uint64_t num_docs = part.phrase ? phrases.admitted(pi) : p.term_postings[part.t_begin];
		if (nsyn) {   // + the first term of every synonym of the part (merger.h:251-255)
			for (uint32_t k = synonyms->part_syn_off[pi]; k < synonyms->part_syn_off[pi + 1]; ++k) {
				const uint32_t sy = synonyms->part_syn[k];
				if (synonyms->syn_term_off[sy + 1] > synonyms->syn_term_off[sy]) num_docs += p.term_postings[npart_terms + synonyms->syn_term_off[sy]];
			}
		}
		if (op == 2) {
			p.est_and = std::min(p.est_and, num_docs);
		} else {
			p.est_or += num_docs;
		}
	}
	p.prescore = !f.simple && std::min(std::min(p.est_or, p.est_and), N) > cfg->merge_limit && N > cfg->merge_limit;

	// ---- the rows: phrase rows, plain sub-terms and the synonyms' sub-terms go through one door
	p.rows.clear();
	p.merge_grid.clear();
	p.terms.assign(nparts + p.nsyn_terms, FtPlanTerm{});
	p.merge_blocks = p.merged_postings = 0;
	uint16_t qp = 0, last_term_qp = 0;
	auto add_row = [&](FtRow r, int32_t op, uint64_t n) {
		r.qp = op == 3 ? 0 : qp;
		if (op != 3) {   // mergeTerm returns at once for a NOT term (mergerimpl.h:110-112)
			r.row = uint32_t(p.merge_grid.size());
			p.merge_grid.push_back({uint32_t(p.merge_blocks), uint32_t(p.rows.size())});
			p.merge_blocks += ft_pass_blocks(n);
			p.merged_postings += n;
		}
		p.rows.push_back(r);
	};
	// the words of one plain or synonym term `qt` as entry `ti` of FtPlan::terms
	auto word_rows = [&](uint32_t ti, const QueryTermIn& qt, bool need_positions, const uint8_t* suppressed) -> FtPlanError {
		for (uint32_t si = qt.sub_begin; si < qt.sub_end; ++si) {
			const FtSubFact& w = f.subs[si];
			if (FtPlanError e = ft_check_subterm(qt, si, w, f.procs, need_positions, who); e) return e;
			if (!w.df) continue;   // (a shard keeps the row of a word it holds no posting of: rows are numbered alike on every shard)
			FtRow r;
			r.term = ti;
			r.src = si;
			r.ord_in_term = uint16_t(si - qt.sub_begin);
			r.suppressed = suppressed && suppressed[si] ? 1 : 0;
			add_row(r, qt.op, w.n);
		}
		return {};
	};
	for (uint32_t pi = 0; pi < nparts; ++pi) {
		const QueryPartIn& part = p.parts[pi];
		const QueryTermIn& qt = f.terms[part.t_begin];
		FtPlanTerm& tc = p.terms[pi];
		tc.op = qt.op;
		tc.sub_begin = uint32_t(p.rows.size());
		if (part.phrase) {
			// the phrase as one part: its rows carry rank and field, every document counts for the masks, the pre-score adds CalcProc16
			tc.phrase = true;
			if (qt.op != 3) ++qp;
			for (uint32_t k = 0, n = phrases.n_rows(pi); k < n; ++k) {
				FtRow r;
				r.term = pi;
				r.src = k;
				r.phrase = 1;
				r.prev_term_qp = last_term_qp;
				r.ord_in_term = uint16_t(p.rows.size() - tc.sub_begin);
				add_row(r, qt.op, phrases.row_n(pi, k));
			}
		} else {
			if (FtPlanError e = ft_check_term_opts(qt, f.num_fields, who, tc.same_boost, tc.all_pos_boost); e) return e;
			if (qt.op != 3) last_term_qp = ++qp;
			if (FtPlanError e = word_rows(pi, qt, !f.simple, nullptr); e) return e;
		}
		tc.sub_end = uint32_t(p.rows.size());
	}
	// ---- the multi-word synonyms' terms behind the parts (mergerimpl.h:509-514): plain mergeTerm calls, every term takes a qp
	p.n_part_qp = qp;
	p.syns.assign(nsyn, FtSynonym{});
	for (uint32_t sy = 0; sy < nsyn; ++sy) {
		p.syns[sy].term_begin = nparts + synonyms->syn_term_off[sy];
		p.syns[sy].term_end = nparts + synonyms->syn_term_off[sy + 1];
		p.syns[sy].nterms = synonyms->syn_term_off[sy + 1] - synonyms->syn_term_off[sy];
		for (uint32_t k = synonyms->syn_term_off[sy]; k < synonyms->syn_term_off[sy + 1]; ++k) {
			const QueryTermIn& qt = f.terms[npart_terms + k];
			FtPlanTerm& tc = p.terms[nparts + k];
			if (FtPlanError e = ft_check_term_opts(qt, f.num_fields, who, tc.same_boost, tc.all_pos_boost); e) return e;
			tc.op = 1;   // for ft_ranges: scored like any term (calcTermScores, mergerimpl.h:393-397), never a restriction of its own
			tc.sub_begin = uint32_t(p.rows.size());
			RX_PLAN_CHECK(qp < 0x7FFE, RXGPU_ERR_PARAMS, ": too many query terms");
			++qp;
			if (FtPlanError e = word_rows(nparts + k, qt, true, synonyms->suppressed); e) return e;
			tc.sub_end = uint32_t(p.rows.size());
		}
		p.syns[sy].end_qp = qp;
	}
	// the AND parts whose term mask takes their synonyms' masks in (ft_syn_masks)
	p.jobs.clear();
	p.job_syns.clear();
	for (uint32_t pi = 0; pi < nparts && nsyn; ++pi) {
		if (f.terms[p.parts[pi].t_begin].op != 2 || synonyms->part_syn_off[pi + 1] == synonyms->part_syn_off[pi]) continue;
		FtSynJob job{pi, uint32_t(p.job_syns.size()), 0};
		for (uint32_t k = synonyms->part_syn_off[pi]; k < synonyms->part_syn_off[pi + 1]; ++k) p.job_syns.push_back(synonyms->part_syn[k]);
		job.syn_end = uint32_t(p.job_syns.size());
		p.jobs.push_back(job);
	}
	RX_PLAN_CHECK(p.merge_blocks * kFtBlockPostings < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, ": more than 2^32 (padded) postings in one merge");
	p.n_rows = uint32_t(p.merge_grid.size());
	RX_PLAN_CHECK(p.n_rows < 0xFFFFu, RXGPU_ERR_PARAMS, ": more than 65534 merged sub-terms in one query (GPU engine limit)");
	if (f.max_areas) {   // MergeDataAreas<Area>: plain terms only (a phrase's areas come out of the PhraseMerger's position chains, phrasemerger.h:147-181)
		RX_PLAN_CHECK(!f.resident && !nsyn, RXGPU_ERR_LOGIC, ": areas are built for queries of plain terms (no multi-word synonyms, no resident form)");
		for (const QueryPartIn& part : p.parts) RX_PLAN_CHECK(!part.phrase, RXGPU_ERR_LOGIC, ": a phrase's areas stay on the CPU merger");
		for (const FtRow& r : p.rows) {
			RX_PLAN_CHECK(f.subs[r.src].n == 0 || f.subs[r.src].has_positions, RXGPU_ERR_LOGIC, ": areas need the words' positions (rxgpu_ft_set_word_positions)");
		}
	}
	p.sp_empty_and = false;
	if (p.sparse) {   // (eligible: plain terms only, so a row's term is its part and its source a word)
		for (size_t i = 0; i < p.rows.size(); ++i) {
			FtRow& r = p.rows[i];
			const FtPlanTerm& tc = p.terms[r.term];
			const QueryTermIn& qt = f.terms[p.parts[r.term].t_begin];
			// calcTermScores (mergerimpl.h:312-315): every field has the same boost, so maxBoostFromFields is field 0's
			const float proc = f.procs[r.src] * qt.opts->field_boost[0] * qt.opts->boost;
			uint32_t p16 = uint32_t(int32_t(proc)) & 0xFFFFu;   // static_cast<uint16_t>(float) as x86 evaluates it
			p16 = std::min<uint32_t>(p16, 65535u / 4);
			r.attr = p16 | (r.row << 20);
			if (i == tc.sub_begin) r.attr |= 1u << 16;
			if (tc.op == 2) r.attr |= 1u << 17;
			if (tc.op == 3) r.attr |= 1u << 18;
		}
		for (uint32_t pi = 0; pi < nparts && !f.simple; ++pi) {   // an AND term without postings empties the mask (buildRestrictingBitmask)
			if (p.terms[pi].op == 2 && p.terms[pi].sub_begin == p.terms[pi].sub_end) p.sp_empty_and = true;
		}
	}
	ft_plan_layouts(f, sz, p);
	return {};
}

// a query without phrases
struct FtNoPhrases {
	uint64_t admitted(uint32_t) const { return 0; }
	uint32_t n_rows(uint32_t) const { return 0; }
	uint64_t row_n(uint32_t, uint32_t) const { return 0; }
};

#undef RX_PLAN_CHECK

// ---------------------------------------------------------------------------------------------------------------------- the dense train
// The merge slot of the first document of (row, range) = the entries of ft_adders' table in front of it, in row-major order.  Up to
// kFtFinishRows merged sub-terms (and 8192 entries) the table is small and every workgroup of ft_finish adds up its own bases (one pass, all
// rows at once); larger queries run ft_slot_bases, which turns the table into its prefix.
constexpr uint32_t kFtFinishRows = 16;
constexpr uint32_t kFtSparseRecords = 768;   // buckets up to this size are replayed from an LDS copy of their records
constexpr uint32_t kFtSparsePostings = 6;    // ... if no document of theirs has more postings than this
constexpr uint32_t kFtSparseHeads = 512;     // chain heads of that copy (by the low bits of the document)
constexpr uint32_t kFtBitmapRows = 8;        // up to this many merged sub-terms ft_finish ranks the first postings with per-row bitmaps instead of a sort
template <typename Plan>
RX_FT_HD inline bool ft_own_bases(const Plan& p) { return p.n_rows <= kFtFinishRows && uint64_t(p.n_rows) * p.n_ranges <= kFtRangeDocs; }
// ft_finish's compact layout (16-bit slots, 32 KB of LDS, 4 workgroups per CU): up to kFtBitmapRows merged sub-terms and mergeLimit below 65535
template <typename Plan>
RX_FT_HD inline bool ft_finish_compact(const Plan& p) { return p.n_rows <= kFtBitmapRows && p.max_merged < 0xFFFFu; }

// ft_finish's dynamic LDS, in 32-bit words from its start.  One block, carved twice: the sorted layout (document table + key list) and the
// compact one (slots + per-row bitmaps + their prefixes); the table of ft_adders lies at the start of the key list / of the block while the
// row bases are summed, and the sparse-bucket replay overlays what the slots leave idle.
struct FtFinishLds {
	static constexpr uint32_t kBitmapWords = kFtBitmapRows * (kFtRangeDocs / 32);
	// sorted layout
	static constexpr uint32_t tab = 0;                                   // [kFtRangeDocs] halves: first row of every document, then its position in the key list
	static constexpr uint32_t keys = tab + kFtRangeDocs / 2;             // [kFtRangeDocs] (row << 13 | document) of the first postings, then their slots
	static constexpr uint32_t words = keys + kFtRangeDocs;
	// compact layout
	static constexpr uint32_t slot = 0;                                  // [kFtRangeDocs] halves: first row, then the slot
	static constexpr uint32_t bits = slot + kFtRangeDocs / 2;            // [kFtBitmapRows][256]
	static constexpr uint32_t pref = bits + kBitmapWords;                // [kFtBitmapRows][256]
	static constexpr uint32_t words_few = pref + kBitmapWords;
	// the table of ft_adders while the bases are summed (ft_own_bases: at most kFtRangeDocs entries)
	RX_FT_HD static constexpr uint32_t table(bool compact) { return compact ? 0u : keys; }
	// sparse-bucket overlay: behind the 16-bit slots / inside the idle tail of the key list (its slots are no more than the bucket's records)
	RX_FT_HD static constexpr uint32_t sparse(bool compact) { return compact ? bits : kFtRangeDocs; }
	static constexpr uint32_t sparse_rec = 0;                                     // [kFtSparseRecords] uint4
	static constexpr uint32_t sparse_head = sparse_rec + kFtSparseRecords * 4;    // [kFtSparseHeads]
	static constexpr uint32_t sparse_todo = sparse_head + kFtSparseHeads;         // [kFtSparseRecords] halves
	static constexpr uint32_t sparse_words = sparse_todo + kFtSparseRecords / 2;
	static constexpr size_t bytes = size_t(words) * 4, bytes_few = size_t(words_few) * 4;
};
static_assert(FtFinishLds::bytes == 48 * 1024 && FtFinishLds::bytes_few == 32 * 1024, "ft_finish: 48 KB, 32 KB in the compact layout");
static_assert(FtFinishLds::table(false) + kFtRangeDocs <= FtFinishLds::words && FtFinishLds::table(true) + kFtRangeDocs <= FtFinishLds::words_few,
			  "the table of ft_adders fits both layouts");
static_assert(FtFinishLds::keys + kFtSparseRecords <= FtFinishLds::sparse(false), "the slots of a sparse bucket end in front of its overlay");
static_assert(FtFinishLds::sparse(false) + FtFinishLds::sparse_words <= FtFinishLds::words &&
				  FtFinishLds::sparse(true) + FtFinishLds::sparse_words <= FtFinishLds::words_few,
			  "the sparse-bucket overlay fits both layouts");
static_assert(kFtSparseRecords <= 1023, "a record index and the end marker fit ten bits");

// What the dense train launches for Q merges over one index (grid.y = query): a grid of 0 means the kernel is not launched.
//   * a document-range shard (range_count != 0, Q == 1) runs its own ranges and mask words only,
//   * phase < 0 launches the whole train, 0 / 1 / 2 the piece a sharded merge exchanges between,
//   * one grid serves the batch: the widest query sets ft_rank_all's, any query that needs ft_preselect_apply / ft_slot_bases / ft_finish's
//     large layout sets it for all (the kernels return at once for the queries that do not).
struct FtTrainLaunch {
	uint32_t nq = 0;
	uint32_t syn_grid = 0;       // ft_syn_masks (a query with multi-word synonyms runs alone: the caller's rule)
	uint32_t ranges_grid = 0;    // ft_ranges
	uint32_t apply_blocks = 0;   // ft_preselect_apply
	uint32_t rank_blocks = 0;    // ft_rank_all
	uint32_t adders_grid = 0;    // ft_adders
	uint32_t bases_grid = 0;     // ft_slot_bases (one workgroup per query)
	uint32_t finish_grid = 0;    // ft_finish ...
	size_t finish_lds = 0;       // ... and its dynamic LDS
};
template <typename Plan>
inline FtTrainLaunch ft_train_launch(const Plan* host_plans, uint32_t nq, int phase) {
	FtTrainLaunch t;
	t.nq = nq;
	if (!nq) return t;
	uint32_t rank_blocks = 0;
	bool any_pre = false, any_bases = false, any_large = false;
	for (uint32_t q = 0; q < nq; ++q) {
		const Plan& p = host_plans[q];
		any_large = any_large || !ft_finish_compact(p);
		rank_blocks = std::max(rank_blocks, (uint32_t(p.merge_blocks) + kFtRankTiles - 1) / kFtRankTiles);
		any_pre = any_pre || (!p.simple && p.prescore);
		any_bases = any_bases || !ft_own_bases(p);
	}
	const Plan& p0 = host_plans[0];
	const uint32_t ranges = p0.range_count ? p0.range_count : p0.n_ranges;
	const uint64_t words = p0.range_count ? uint64_t(p0.range_count) * (kFtRangeDocs / 32) : p0.nwords;
	if (phase < 0 || phase == 0) {
		t.syn_grid = p0.n_syn_jobs ? p0.n_ranges : 0u;
		t.ranges_grid = ranges;
	}
	if (phase < 0 || phase == 1) {
		t.apply_blocks = any_pre ? uint32_t(ft_apply_blocks(words)) : 0u;
		t.rank_blocks = rank_blocks;
		t.adders_grid = ranges;
	}
	if (phase < 0 || phase == 2) {
		t.bases_grid = any_bases ? 1u : 0u;
		t.finish_grid = ranges;
		t.finish_lds = any_large ? FtFinishLds::bytes : FtFinishLds::bytes_few;
	}
	return t;
}

}  // namespace rxgpu
