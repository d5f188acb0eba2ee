// One phrase of a query through ft_phrase.hip: the rows the main merge (rxgpu_ft_merge.hip) reads instead of words.
#include <algorithm>
#include <cstring>

#include "rxgpu_ft_internal.h"

namespace rxgpu {

// a row of a phrase no document of this shard holds
static FtPosSubterm empty_row(const float* procs, uint32_t si) {
	FtPosSubterm row{};
	row.proc = procs[si];
	row.phrase = 1;
	return row;
}

// The rest of a phrase behind its admission: the admitted documents term by term (ft_phrase_docs), the packed rows (ft_phrase_pack).
// c.admitted may have been LOWERED by the sharded layer (the cut of the whole index fell inside or before this shard's documents): the
// admitted documents are a prefix of the slots, so the count on the device is simply overwritten.
int finish_phrase(rxgpu_ft_index* h, const float* procs, PhraseCtx& c, PhraseRows& out, const char* who) {
	rxgpu::FtPhrasePlan& p = c.p;
	const uint32_t admitted = c.admitted, n_rows0 = c.n_rows0, n_ranges = c.n_ranges;
	const uint64_t sum_caps = c.sum_caps;
	const size_t phrase_index = c.phrase_index;
	const bool shard = c.shard;
	const std::vector<uint32_t>&row_sub = c.row_sub, &shard_row_sub = c.shard_row_sub;
	const std::vector<int32_t>& shard_row_grid = c.shard_row_grid;
	hipStream_t st = h->stream;
	char* hp = static_cast<char*>(h->h_pinned);
	out.admitted = admitted;
	if (shard) RX_HIP(hipMemcpyAsync(p.sync + 2, &c.admitted, 4, hipMemcpyHostToDevice, st));   // (c outlives the copy: the waits below)

	// ---- workspace + packed rows, sized by what the admission found
	const size_t pad = rxgpu::kFtPhraseRowPad;
	const size_t cap_entries = size_t(admitted) + (size_t(n_rows0) + 1) * pad;
	rxgpu::FtCarver cb;
	const size_t o_ws = cb.take(std::max<uint64_t>(1, 2 * sum_caps) * 8);
	const size_t o_rcnt = cb.take(size_t(n_rows0) * 4), o_rbase = cb.take(size_t(n_rows0) * 4);
	const size_t o_odoc = cb.take(cap_entries * 4), o_orank = cb.take(cap_entries * 4), o_ofield = cb.take(cap_entries), o_opoff = cb.take(cap_entries * 4);
	const size_t o_ofpos = cb.take(std::max<uint64_t>(1, sum_caps) * 8);
	const size_t o_orange = cb.take(size_t(n_rows0) * (n_ranges + 1) * 4);
	const size_t o_hdr = cb.take((size_t(4) + n_rows0) * 4);
	rxgpu_devbuf& db = h->d_phrase_b[phrase_index];
	if (int rc = db.ensure(cb.off); rc) return rc;
	char* bb = static_cast<char*>(db.ptr);
	p.ws = reinterpret_cast<uint64_t*>(bb + o_ws);
	p.row_cnt = reinterpret_cast<uint32_t*>(bb + o_rcnt);
	p.row_base = reinterpret_cast<uint32_t*>(bb + o_rbase);
	p.out_doc = reinterpret_cast<uint32_t*>(bb + o_odoc);
	p.out_rank = reinterpret_cast<float*>(bb + o_orank);
	p.out_field = reinterpret_cast<uint8_t*>(bb + o_ofield);
	p.out_pos_off = reinterpret_cast<uint32_t*>(bb + o_opoff);
	p.out_fpos = reinterpret_cast<uint64_t*>(bb + o_ofpos);
	p.out_range_off = reinterpret_cast<uint32_t*>(bb + o_orange);
	p.out_header = reinterpret_cast<uint32_t*>(bb + o_hdr);
	RX_HIP(rxgpu::launch_ft_phrase_docs(p, admitted, st));
	RX_HIP(rxgpu::launch_ft_phrase_pack(p, st));
	RX_HIP(hipEventRecord(h->ev_phb, st));
	RX_HIP(hipMemcpyAsync(hp, p.out_header, (size_t(4) + n_rows0) * 4, hipMemcpyDeviceToHost, st));
	RX_HIP(hipStreamSynchronize(st));
	float ms = 0.f;
	if (hipEventElapsedTime(&ms, h->ev_pha, h->ev_phb) == hipSuccess) h->stat_ms += ms;
	const uint32_t* hdr = reinterpret_cast<const uint32_t*>(hp);
	RX_CHECK(hdr[0] == admitted && hdr[2] <= admitted, RXGPU_ERR_DEVICE, std::string(who) + ": corrupt phrase header");
	size_t row_base = 0;
	std::vector<rxgpu::FtPosSubterm> packed(n_rows0);   // by grid row; n == 0: the row came out empty
	for (uint32_t r = 0; r < n_rows0; ++r) {
		const uint32_t cnt = hdr[4 + r];
		if (cnt) {
			rxgpu::FtPosSubterm row{};
			row.n = cnt;
			row.doc = p.out_doc + row_base;
			row.pos_off = p.out_pos_off + row_base;
			row.fpos = p.out_fpos;
			row.pre_rank = p.out_rank + row_base;
			row.pre_field = p.out_field + row_base;
			row.proc = procs[row_sub[r]];
			row.range_off = p.out_range_off + size_t(r) * (n_ranges + 1);
			row.n_ranges = n_ranges;
			row.phrase = 1;
			packed[r] = row;
			if (!shard) out.rows.push_back(row);
		}
		row_base += (size_t(cnt) + 1 + pad - 1) / pad * pad;
	}
	for (size_t j = 0; j < shard_row_sub.size(); ++j) {   // a shard: every row of the index, the empty ones included
		const int32_t g = shard_row_grid[j];
		out.rows.push_back(g >= 0 && packed[size_t(g)].n ? packed[size_t(g)] : empty_row(procs, shard_row_sub[j]));
	}
	return RXGPU_OK;
}

int run_phrase(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const std::vector<QueryTermIn>& terms, const QueryPartIn& part, const uint32_t* word_ids,
			   const float* procs, const uint8_t* d_excluded, size_t phrase_index, PhraseRows& out, const char* who, bool first_half_only) {
	const uint32_t nf = h->num_fields, T = part.t_end - part.t_begin;
	const uint64_t N = h->total_docs;
	const int bm25_type = cfg->bm25_type;
	std::vector<rxgpu::FtPosSubterm> subs;
	std::vector<rxgpu::FtTermCfg> tcfg(T);
	std::vector<int32_t> distance(T);
	std::vector<rxgpu::FtGridEntry> grid;
	std::vector<uint32_t> row_sub;   // first term: position of the row's sub-term in the caller's list
	uint64_t grid_blocks = 0, term0_vdocs = 0, term0_df = 0;
	long long sum_proc = 0;
	// A document-range shard: the rows of the phrase are numbered alike on every shard — one per sub-term of the first term that
	// holds postings ANYWHERE in the index (word_df), with or without postings in this shard's documents — because the sharded layer adds the
	// shards' [rows][ranges] tables up.  shard_row_grid: the row's entry in `grid`, -1 when this shard holds none of its postings.
	const bool shard = h->sh_total > 1;
	std::vector<uint32_t> shard_row_sub;
	std::vector<int32_t> shard_row_grid;
	for (uint32_t k = 0; k < T; ++k) {
		const QueryTermIn& qt = terms[part.t_begin + k];
		bool same, all_pos;
		if (rxgpu::FtPlanError e = rxgpu::ft_check_term_opts(qt, nf, who, same, all_pos); e) return plan_error(e);
		fill_term_cfg(tcfg[k], h, cfg, qt, same, all_pos);
		distance[k] = qt.distance;
		tcfg[k].sub_begin = uint32_t(subs.size());
		if (qt.sub_end > qt.sub_begin) sum_proc = (long long)(float(sum_proc) + procs[qt.sub_begin]);   // CalcProc16: long long += float, term by term
		for (uint32_t si = qt.sub_begin; si < qt.sub_end; ++si) {
			const rxgpu_ft_word& w = h->dict().find(word_ids[si])->second;
			RX_CHECK(w.n == 0 || w.fpos, RXGPU_ERR_LOGIC, std::string(who) + ": the word was uploaded without positions (rxgpu_ft_set_word_positions)");
			RX_CHECK(si == qt.sub_begin || procs[si] <= procs[si - 1], RXGPU_ERR_PARAMS,
					 std::string(who) + ": sub-terms must be sorted by proc, descending (SortSubterms)");
			if (k == 0) {
				term0_vdocs += w.n;
				term0_df += word_df(w);
				if (shard && word_df(w)) {
					shard_row_sub.push_back(si);
					shard_row_grid.push_back(w.n ? int32_t(grid.size()) : -1);
				}
			}
			out.postings += w.n;
			if (!w.n) continue;
			rxgpu::FtPosSubterm ft = word_subterm(w, bm25_type, N, procs[si]);
			ft.term = k;
			ft.ord_in_term = uint16_t(si - qt.sub_begin);
			if (k == 0) {
				grid.push_back({uint32_t(grid_blocks), uint32_t(subs.size())});
				grid_blocks += rxgpu::ft_pass_blocks(w.n);
				row_sub.push_back(si);
			}
			subs.push_back(ft);
		}
		tcfg[k].sub_end = uint32_t(subs.size());
	}
	RX_CHECK(sum_proc >= 0 && sum_proc < 65535, RXGPU_ERR_PARAMS, std::string(who) + ": the procs of a phrase's terms add up to 65535 or more");
	out.proc16 = uint32_t(sum_proc);
	const uint32_t n_rows0 = uint32_t(grid.size());
	(void)term0_df;   // (the admission cut of the whole index — phrasemerger.h:341 — is settled by the sharded layer between the two halves)
	const uint64_t max_merged = std::min<uint64_t>(cfg->merge_limit, term0_vdocs);   // phrasemerger.h:341
	if (!n_rows0 || !max_merged) {   // the first term matched nothing (here): no document (of this shard) holds the phrase
		for (const uint32_t si : shard_row_sub) out.rows.push_back(empty_row(procs, si));
		return RXGPU_OK;
	}
	RX_CHECK(grid_blocks * rxgpu::kFtBlockPostings < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, std::string(who) + ": more than 2^32 (padded) postings in one phrase term");
	const uint32_t n_ranges = uint32_t((N + rxgpu::kFtRangeDocs - 1) / rxgpu::kFtRangeDocs);
	const size_t M = size_t(max_merged);

	if (h->d_phrase_a.size() <= phrase_index) {
		h->d_phrase_a.resize(phrase_index + 1);
		h->d_phrase_b.resize(phrase_index + 1);
	}
	rxgpu::FtCarver ca;
	const size_t o_subs = ca.take(subs.size() * sizeof(rxgpu::FtPosSubterm));
	const size_t o_terms = ca.take(size_t(T) * sizeof(rxgpu::FtTermCfg));
	const size_t o_dist = ca.take(size_t(T) * 4);
	const size_t o_grid = ca.take(grid.size() * sizeof(rxgpu::FtGridEntry));
	const size_t cfg_floats = size_t(6) * nf + size_t(T) * nf;
	const size_t o_fc = ca.take(cfg_floats * 4 + size_t(T) * nf);
	const size_t plan_bytes = ca.off;
	const size_t o_zero = ca.off;
	const size_t o_lb = ca.take(size_t(grid_blocks) * 8);
	const size_t o_sync = ca.take(8 * 4);
	const size_t zero_bytes = ca.off - o_zero;
	const size_t o_sdoc = ca.take(M * 4), o_srow = ca.take(M * 4), o_scap = ca.take(M * 4), o_sproc = ca.take(M * 4), o_sfield = ca.take(M);
	const size_t o_spos = ca.take(M * 8), o_snpos = ca.take(M * 4);
	rxgpu_devbuf& da = h->d_phrase_a[phrase_index];
	if (int rc = da.ensure(ca.off); rc) return rc;
	char* base = static_cast<char*>(da.ptr);
	if (int rc = h->ensure_pinned(std::max<size_t>(plan_bytes, (size_t(8) + n_rows0) * 4 + 256)); rc) return rc;
	char* hp = static_cast<char*>(h->h_pinned);
	std::memset(hp, 0, plan_bytes);
	float* fc = reinterpret_cast<float*>(hp + o_fc);
	uint8_t* need_sum = reinterpret_cast<uint8_t*>(fc + cfg_floats);
	const float* d_fc = reinterpret_cast<const float*>(base + o_fc);
	const uint8_t* d_need_sum = reinterpret_cast<const uint8_t*>(d_fc + cfg_floats);
	stage_field_cfg(fc, cfg, nf);
	for (uint32_t k = 0; k < T; ++k) {
		const QueryTermIn& qt = terms[part.t_begin + k];
		for (uint32_t f = 0; f < nf; ++f) {
			fc[size_t(6 + k) * nf + f] = qt.opts->field_boost[f];
			need_sum[size_t(k) * nf + f] = qt.opts->need_sum_rank[f];
		}
		point_term_cfg(tcfg[k], d_fc, d_fc + size_t(6 + k) * nf, d_need_sum + size_t(k) * nf, nf);
	}
	std::memcpy(hp + o_subs, subs.data(), subs.size() * sizeof(rxgpu::FtPosSubterm));
	std::memcpy(hp + o_terms, tcfg.data(), tcfg.size() * sizeof(rxgpu::FtTermCfg));
	std::memcpy(hp + o_dist, distance.data(), distance.size() * 4);
	std::memcpy(hp + o_grid, grid.data(), grid.size() * sizeof(rxgpu::FtGridEntry));
	hipStream_t st = h->stream;
	RX_HIP(hipMemcpyAsync(base, hp, plan_bytes, hipMemcpyHostToDevice, st));
	RX_HIP(hipMemsetAsync(base + o_zero, 0, zero_bytes, st));

	rxgpu::FtPhrasePlan p{};
	p.subs = reinterpret_cast<const rxgpu::FtPosSubterm*>(base + o_subs);
	p.terms = reinterpret_cast<const rxgpu::FtTermCfg*>(base + o_terms);
	p.distance = reinterpret_cast<const int32_t*>(base + o_dist);
	p.grid = reinterpret_cast<const rxgpu::FtGridEntry*>(base + o_grid);
	p.nterms = T;
	p.n_grid = n_rows0;
	p.grid_blocks = uint32_t(grid_blocks);
	p.n_rows0 = n_rows0;
	p.max_merged = uint32_t(max_merged);
	p.n_ranges = n_ranges;
	p.total_docs = N;
	p.distance_weight = float(cfg->distance_weight);
	p.distance_boost = float(cfg->distance_boost);
	p.removed = h->d_removed;
	p.excluded = d_excluded;
	p.lookback = reinterpret_cast<unsigned long long*>(base + o_lb);
	p.sync = reinterpret_cast<uint32_t*>(base + o_sync);
	p.slot_doc = reinterpret_cast<uint32_t*>(base + o_sdoc);
	p.slot_row = reinterpret_cast<uint32_t*>(base + o_srow);
	p.slot_cap = reinterpret_cast<uint32_t*>(base + o_scap);
	p.slot_proc = reinterpret_cast<float*>(base + o_sproc);
	p.slot_field = reinterpret_cast<uint8_t*>(base + o_sfield);
	p.slot_pos = reinterpret_cast<uint64_t*>(base + o_spos);
	p.slot_npos = reinterpret_cast<uint32_t*>(base + o_snpos);
	if (!h->ev_pha) {
		RX_HIP(hipEventCreate(&h->ev_pha));
		RX_HIP(hipEventCreate(&h->ev_phb));
	}
	RX_HIP(hipEventRecord(h->ev_pha, st));
	RX_HIP(rxgpu::launch_ft_phrase_admit(p, st));
	RX_HIP(hipMemcpyAsync(hp, p.sync, 8 * 4, hipMemcpyDeviceToHost, st));
	RX_HIP(hipStreamSynchronize(st));
	const uint32_t* sy = reinterpret_cast<const uint32_t*>(hp);
	RX_CHECK(sy[1] == 0, RXGPU_ERR_DEVICE, std::string(who) + ": ordered look-back timed out on the device (phrase admission)");
	const uint32_t admitted = sy[2];
	const uint64_t sum_caps = uint64_t(sy[4]) | (uint64_t(sy[5]) << 32);
	RX_CHECK(admitted <= max_merged, RXGPU_ERR_DEVICE, std::string(who) + ": corrupt phrase admission count");
	RX_CHECK(sum_caps < (1ull << 31), RXGPU_ERR_PARAMS, std::string(who) + ": more than 2^31 positions in the documents of one phrase (GPU engine limit)");
	out.admitted = admitted;
	auto ctx = std::make_shared<PhraseCtx>();
	ctx->p = p;
	ctx->row_sub = row_sub;
	ctx->shard_row_sub = shard_row_sub;
	ctx->shard_row_grid = shard_row_grid;
	ctx->n_rows0 = n_rows0;
	ctx->n_ranges = n_ranges;
	ctx->admitted = admitted;
	ctx->sum_caps = sum_caps;
	ctx->phrase_index = phrase_index;
	ctx->shard = shard;
	if (first_half_only) {   // what this shard admitted, row by row (slot order IS (row, document) order): the sharded layer's cut needs it
		std::vector<uint32_t> slot_row(admitted);
		if (admitted) RX_HIP(hipMemcpy(slot_row.data(), p.slot_row, size_t(admitted) * 4, hipMemcpyDeviceToHost));
		std::vector<uint32_t> by_grid(n_rows0, 0);
		for (const uint32_t r : slot_row) {
			RX_CHECK(r < n_rows0, RXGPU_ERR_DEVICE, std::string(who) + ": corrupt phrase admission rows");
			++by_grid[r];
		}
		ctx->row_admitted.assign(shard_row_sub.size(), 0);
		for (size_t j = 0; j < shard_row_sub.size(); ++j) {
			if (shard_row_grid[j] >= 0) ctx->row_admitted[j] = by_grid[size_t(shard_row_grid[j])];
		}
		out.pending = std::move(ctx);
		return RXGPU_OK;
	}
	return finish_phrase(h, procs, *ctx, out, who);
}

}  // namespace rxgpu
