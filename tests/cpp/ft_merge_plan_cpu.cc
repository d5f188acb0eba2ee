// The decisions of one BM25 merge (reindexer_amd/csrc/ft_merge_plan.h) compiled for the host: tests/test_ft_merge_plan.py pins its rules on
// the CPU.  Test infrastructure only — nothing in the product links this.
#include <cstdint>
#include <cstring>
#include <vector>

#include "ft_merge_plan.h"

extern "C" {

// the query, the dictionary's facts and the handle's facts as flat arrays (the field order is FtPlanCpuIn's in the test)
struct FtPlanCpuIn {
	uint32_t nterms, num_fields;
	const int32_t* ops;
	const int32_t* phrase_num;
	const uint32_t* sub_off;          // [nterms + 1]
	const float* boost;               // [nterms] FtDslOpts::boost
	const float* term_len_boost;      // [nterms]
	const float* field_boost;         // [nterms][num_fields]; null: the terms' options hold null arrays
	const uint8_t* need_sum;          // [nterms][num_fields]
	uint32_t nsyn, first_term;
	const uint32_t* syn_term_off;
	const uint32_t* part_syn_off;
	const uint32_t* part_syn;
	const uint8_t* suppressed;
	const uint64_t* sub_n;            // per sub-term
	const uint64_t* sub_df;
	const uint32_t* sub_last_doc;
	const uint8_t* sub_found;
	const uint8_t* sub_has_pos;
	const float* procs;
	uint32_t merge_limit;
	int32_t bm25_type;
	double k1, b, ratio;
	const double* field_cfg;          // [6][num_fields]: bm25 boost, bm25 weight, term_len boost, term_len weight, position boost, position weight
	const float* h_avg;
	uint32_t n_avg, sh_total;
	uint64_t total_docs;
	int32_t train_mode, simple, resident, have_outs;
	uint32_t max_areas, pad;
	uint64_t cap;
	const uint64_t* phrase_admitted;  // per part
	const uint32_t* phrase_row_off;   // [nparts + 1] into phrase_row_n
	const uint64_t* phrase_row_n;
	uint64_t sizes[5];                // FtStructSizes: subterm, term_cfg, syn_job, plan, record
};
struct FtPlanCpuOut {
	int32_t code;
	char msg[252];
	uint64_t* scalars;        // kScalars in the test
	uint32_t* parts;          // [nparts][3] phrase, t_begin, t_end
	uint64_t* term_postings;  // [nterms]
	uint32_t* rows;           // [n][9] term, src, row, attr, qp, prev_term_qp, ord_in_term, suppressed, phrase
	uint32_t* terms;          // [n][6] sub_begin, sub_end, op, same_boost, all_pos_boost, phrase
	uint32_t* grid;           // [n][2] block_base, sub
	uint32_t* syns;           // [n][4] term_begin, term_end, end_qp, nterms
	uint32_t* jobs;           // [n][3] part, syn_begin, syn_end
	uint32_t* job_syns;
	uint64_t* regions;        // [26][2] (off, bytes): the state layout's regions in declaration order, then the clean layout's
	uint32_t cap_rows;        // rows / grid entries the arrays above hold
};

namespace {
struct PhraseArrays {
	const FtPlanCpuIn& in;
	uint64_t admitted(uint32_t pi) const { return in.phrase_admitted ? in.phrase_admitted[pi] : 0; }
	uint32_t n_rows(uint32_t pi) const { return in.phrase_row_off ? in.phrase_row_off[pi + 1] - in.phrase_row_off[pi] : 0; }
	uint64_t row_n(uint32_t pi, uint32_t r) const { return in.phrase_row_n[in.phrase_row_off[pi] + r]; }
};
int fail(const rxgpu::FtPlanError& e, FtPlanCpuOut* out) {
	out->code = e.code;
	std::strncpy(out->msg, e.msg.c_str(), sizeof(out->msg) - 1);
	return e.code;
}
}  // namespace

int ft_merge_plan_cpu(const FtPlanCpuIn* in, FtPlanCpuOut* out) {
	const uint32_t nf = in->num_fields;
	std::vector<rxgpu_ft_term_opts> opts(in->nterms);
	std::vector<rxgpu::QueryTermIn> terms(in->nterms);
	for (uint32_t t = 0; t < in->nterms; ++t) {
		opts[t].boost = in->boost[t];
		opts[t].term_len_boost = in->term_len_boost[t];
		opts[t].field_boost = in->field_boost ? in->field_boost + size_t(t) * nf : nullptr;
		opts[t].need_sum_rank = in->field_boost ? in->need_sum + size_t(t) * nf : nullptr;
		terms[t] = rxgpu::QueryTermIn{in->ops[t], &opts[t], in->sub_off[t], in->sub_off[t + 1], in->phrase_num[t], 1};
	}
	const uint32_t nsubs = in->nterms ? in->sub_off[in->nterms] : 0;
	std::vector<rxgpu::FtSubFact> subs(nsubs);
	for (uint32_t s = 0; s < nsubs; ++s) subs[s] = rxgpu::FtSubFact{in->sub_n[s], in->sub_df[s], in->sub_last_doc[s], in->sub_found[s] != 0, in->sub_has_pos[s] != 0, nullptr};
	rxgpu::SynonymsIn syn;
	syn.nsyn = in->nsyn;
	syn.first_term = in->first_term;
	syn.syn_term_off = in->syn_term_off;
	syn.part_syn_off = in->part_syn_off;
	syn.part_syn = in->part_syn;
	syn.suppressed = in->suppressed;
	rxgpu_ft_config cfg{};
	cfg.bm25_k1 = in->k1;
	cfg.bm25_b = in->b;
	cfg.summation_ranks_by_fields_ratio = in->ratio;
	cfg.merge_limit = in->merge_limit;
	cfg.num_fields = nf;
	cfg.bm25_type = in->bm25_type;
	cfg.bm25_boost = in->field_cfg + 0 * nf;
	cfg.bm25_weight = in->field_cfg + 1 * nf;
	cfg.term_len_boost = in->field_cfg + 2 * nf;
	cfg.term_len_weight = in->field_cfg + 3 * nf;
	cfg.position_boost = in->field_cfg + 4 * nf;
	cfg.position_weight = in->field_cfg + 5 * nf;
	rxgpu::FtMergeFacts f;
	f.terms = terms.data();
	f.nterms = in->nterms;
	f.synonyms = in->nsyn ? &syn : nullptr;
	f.subs = subs.data();
	f.procs = in->procs;
	f.cfg = &cfg;
	f.num_fields = nf;
	f.h_avg = in->h_avg;
	f.n_avg = in->n_avg;
	f.total_docs = in->total_docs;
	f.sh_total = in->sh_total;
	f.train_mode = in->train_mode;
	f.simple = in->simple != 0;
	f.resident = in->resident != 0;
	f.max_areas = in->max_areas;
	f.have_outs = in->have_outs != 0;
	f.cap = in->cap;
	f.who = "plan";
	out->code = 0;
	out->msg[0] = 0;
	rxgpu::FtMergePlan p;
	if (rxgpu::FtPlanError e = rxgpu::ft_plan_volume(f, p); e) return fail(e, out);
	uint64_t* sc = out->scalars;
	sc[0] = p.nparts;
	sc[1] = p.total_vids;
	sc[2] = p.max_merged;
	sc[3] = p.empty;
	sc[4] = p.any_phrase;
	sc[5] = p.sparse;
	for (uint32_t i = 0; i < p.nparts; ++i) {
		out->parts[3 * i] = p.parts[i].phrase;
		out->parts[3 * i + 1] = p.parts[i].t_begin;
		out->parts[3 * i + 2] = p.parts[i].t_end;
	}
	for (uint32_t t = 0; t < in->nterms; ++t) out->term_postings[t] = p.term_postings[t];
	if (p.empty) return 0;
	const rxgpu::FtStructSizes sz{size_t(in->sizes[0]), size_t(in->sizes[1]), size_t(in->sizes[2]), size_t(in->sizes[3]), size_t(in->sizes[4])};
	if (rxgpu::FtPlanError e = rxgpu::ft_plan_rows(f, PhraseArrays{*in}, sz, p); e) return fail(e, out);
	const uint64_t more[] = {p.est_or,     p.est_and,         p.prescore,   p.query_len,       p.rows.size(),  p.terms.size(),      p.merge_grid.size(),
							 p.merge_blocks, p.merged_postings, p.n_rows,     p.n_part_qp,       p.syns.size(),  p.jobs.size(),       p.job_syns.size(),
							 p.sp_empty_and, p.nwords,          p.n_ranges,   p.state.cfg_floats, p.state.plan_bytes, p.state.bytes,  p.clean.bytes,
							 p.out.header,  p.out.doc,         p.out.proc,   p.out.terms_counter, p.out.field, p.out.bytes,         p.area_hdr_bytes,
							 p.area_bytes};
	for (size_t i = 0; i < sizeof(more) / sizeof(more[0]); ++i) sc[6 + i] = more[i];
	for (size_t i = 0; i < p.rows.size() && i < out->cap_rows; ++i) {
		const rxgpu::FtRow& r = p.rows[i];
		const uint32_t v[9] = {r.term, r.src, r.row, r.attr, r.qp, r.prev_term_qp, r.ord_in_term, r.suppressed, r.phrase};
		std::memcpy(out->rows + 9 * i, v, sizeof(v));
	}
	for (size_t i = 0; i < p.terms.size() && i < out->cap_rows; ++i) {
		const rxgpu::FtPlanTerm& t = p.terms[i];
		const uint32_t v[6] = {t.sub_begin, t.sub_end, uint32_t(t.op), t.same_boost, t.all_pos_boost, t.phrase};
		std::memcpy(out->terms + 6 * i, v, sizeof(v));
	}
	for (size_t i = 0; i < p.merge_grid.size() && i < out->cap_rows; ++i) {
		out->grid[2 * i] = p.merge_grid[i].block_base;
		out->grid[2 * i + 1] = p.merge_grid[i].sub;
	}
	for (size_t i = 0; i < p.syns.size() && i < out->cap_rows; ++i) {
		const uint32_t v[4] = {p.syns[i].term_begin, p.syns[i].term_end, p.syns[i].end_qp, p.syns[i].nterms};
		std::memcpy(out->syns + 4 * i, v, sizeof(v));
	}
	for (size_t i = 0; i < p.jobs.size() && i < out->cap_rows; ++i) {
		const uint32_t v[3] = {p.jobs[i].part, p.jobs[i].syn_begin, p.jobs[i].syn_end};
		std::memcpy(out->jobs + 3 * i, v, sizeof(v));
	}
	for (size_t i = 0; i < p.job_syns.size() && i < out->cap_rows; ++i) out->job_syns[i] = p.job_syns[i];
	const rxgpu::FtStateLayout& s = p.state;
	const rxgpu::FtCleanLayout& c = p.clean;
	const rxgpu::FtRegion regs[] = {s.plan_subs, s.plan_terms, s.plan_mgrid, s.plan_fc, s.plan_syns, s.plan_jobs, s.plan_jsyn, s.plan_self, s.mask,  s.synmask, s.score, s.brec, s.boff,
									s.adders,    s.eidx,       s.efield,     s.tdoc,    s.tpos,      s.tidx,      c.hist,      c.lb_pre,    c.bcnt, c.sync,    c.dbg,   c.lb_units, c.erank};
	for (size_t i = 0; i < sizeof(regs) / sizeof(regs[0]); ++i) {
		out->regions[2 * i] = regs[i].off;
		out->regions[2 * i + 1] = regs[i].bytes;
	}
	return 0;
}

// QueryMergeData::Empty() / Simple() of the parts' terms: out = {nparts, empty, simple}
void ft_classify_cpu(uint32_t nterms, const int32_t* ops, const int32_t* phrase_num, uint32_t* out) {
	std::vector<rxgpu::QueryTermIn> terms(nterms);
	for (uint32_t t = 0; t < nterms; ++t) terms[t] = rxgpu::QueryTermIn{ops[t], nullptr, 0, 0, phrase_num[t], 1};
	const rxgpu::FtQueryClass c = rxgpu::ft_classify_query(terms.data(), nterms);
	out[0] = c.nparts;
	out[1] = c.empty;
	out[2] = c.simple;
}

void ft_out_layout_cpu(uint64_t max_merged, uint64_t* out) {
	const rxgpu::FtOutLayout o = rxgpu::ft_out_layout(max_merged);
	const uint64_t v[6] = {o.header, o.doc, o.proc, o.terms_counter, o.field, o.bytes};
	std::memcpy(out, v, sizeof(v));
}

// What the dense train launches (ft_train_launch) for nq host plans given as rows of nine facts:
//   n_rows, max_merged, merge_blocks, simple, prescore, n_ranges, range_count, nwords, n_syn_jobs
// out = {syn_grid, ranges_grid, apply_blocks, rank_blocks, adders_grid, bases_grid, finish_grid, finish_lds}
void ft_train_launch_cpu(const uint64_t* facts, uint32_t nq, int32_t phase, uint64_t* out) {
	struct Plan {
		uint32_t n_rows, max_merged, merge_blocks;
		uint8_t simple, prescore;
		uint32_t n_ranges, range_count;
		uint64_t nwords;
		uint32_t n_syn_jobs;
	};
	std::vector<Plan> plans(nq);
	for (uint32_t q = 0; q < nq; ++q) {
		const uint64_t* f = facts + 9 * size_t(q);
		plans[q] = Plan{uint32_t(f[0]), uint32_t(f[1]), uint32_t(f[2]), uint8_t(f[3]), uint8_t(f[4]), uint32_t(f[5]), uint32_t(f[6]), f[7], uint32_t(f[8])};
	}
	const rxgpu::FtTrainLaunch t = rxgpu::ft_train_launch(plans.data(), nq, phase);
	const uint64_t v[8] = {t.syn_grid, t.ranges_grid, t.apply_blocks, t.rank_blocks, t.adders_grid, t.bases_grid, t.finish_grid, t.finish_lds};
	std::memcpy(out, v, sizeof(v));
}

// ft_finish's dynamic LDS as the kernel carves it, in words: the sorted layout, the compact one, the sparse-bucket overlay in both
void ft_finish_lds_cpu(uint32_t* out) {
	using L = rxgpu::FtFinishLds;
	const uint32_t v[14] = {L::tab,           L::keys,          L::words,      L::slot,        L::bits,        L::pref,         L::words_few,
							L::table(false),  L::table(true),   L::sparse(false), L::sparse(true), L::sparse_head, L::sparse_todo, L::sparse_words};
	std::memcpy(out, v, sizeof(v));
}

uint64_t ft_apply_blocks_cpu(uint64_t nwords) { return rxgpu::ft_apply_blocks(nwords); }

// the constants of the dense train's launch rules
void ft_train_constants(uint32_t* out) {
	const uint32_t v[7] = {uint32_t(rxgpu::kFtApplyWords), uint32_t(rxgpu::kFtRankTiles), rxgpu::kFtFinishRows,  rxgpu::kFtBitmapRows,
						   rxgpu::kFtSparseRecords,        rxgpu::kFtSparsePostings,      rxgpu::kFtSparseHeads};
	std::memcpy(out, v, sizeof(v));
}

// the constants the decisions share with the kernels
void ft_plan_constants(uint32_t* out) {
	const uint32_t v[9] = {uint32_t(rxgpu::kFtBlockPostings), uint32_t(rxgpu::kFtPassItems), rxgpu::kFtRangeDocs, rxgpu::kFtSparseSubs, rxgpu::kFtHistCopies,
						   rxgpu::kFtHistStride,              rxgpu::kFtSyncWords,           rxgpu::kFtBatchMax,  rxgpu::ft_pass_blocks(1025)};
	std::memcpy(out, v, sizeof(v));
}
}
