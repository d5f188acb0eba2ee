// Document-range shards of an ft_fast index (rxgpu_ft_create_sharded; the layout and the exchange: rxgpu_ft_internal.h, above
// rxgpu_ft_shard_set): the sharded handle's side of the dictionary calls and one merge over all shards.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rxgpu_ft_internal.h"
#include "ft_phrase_cut.h"
#include "shard_plan.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

namespace {
// Piece `k` (0 histograms, 1 tables) of every shard -> every rank's receive buffer.  Every shard's producer has been enqueued on its own
// stream and wrote bytes (a multiple of 4) at send_ptr(k, s); consumers enqueued afterwards on the shards' streams read recv_ptr(k, s).
int ft_shards_gather(rxgpu_ft_shard_set* ss, int k, size_t bytes) {
	const size_t S = ss->shards.size();
	for (size_t s = 0; s < S; ++s) {
		RX_HIP(hipSetDevice(ss->devices[s]));
		RX_HIP(hipEventRecord(ss->ev_shard[s], ss->shards[s]->stream));
	}
	for (uint32_t r = 0; r < ss->nranks; ++r) {
		RX_HIP(hipSetDevice(ss->rank_dev[r]));
		for (size_t s = 0; s < S; ++s) {
			if (ss->shard_rank[s] == r) RX_HIP(hipStreamWaitEvent(ss->rstream[r], ss->ev_shard[s], 0));
		}
	}
	if (ss->cs) {
		const rxgpu::RcclApi& api = rxgpu::rccl_api();
		std::lock_guard<std::mutex> lk(ss->cs->mtx);
		ncclResult_t nr = api.ncclGroupStart();
		for (uint32_t r = 0; r < ss->nranks && nr == ncclSuccess; ++r) {
			nr = api.ncclAllGather(ss->d_send[k][r].ptr, ss->d_recv[k][r].ptr, bytes / 4 * ss->slots, ncclUint32, ss->cs->comms[r], ss->rstream[r]);
		}
		const ncclResult_t ne = api.ncclGroupEnd();
		if (nr == ncclSuccess) nr = ne;
		if (nr != ncclSuccess) {
			set_error(std::string("sharded ft index: ncclAllGather: ") + api.ncclGetErrorString(nr));
			return RXGPU_ERR_DEVICE;
		}
		++ss->collectives;
	} else if (!ss->host_exchange && ss->nranks == 1) {
		// every shard lives on ONE device: the all-gather of a single rank is a copy on that device's exchange stream (no communicator is made
		// for one rank; with several devices the branch above runs — the same call pattern as the float_vector shards' exchange)
		RX_HIP(hipSetDevice(ss->rank_dev[0]));
		RX_HIP(hipMemcpyAsync(ss->d_recv[k][0].ptr, ss->d_send[k][0].ptr, bytes * ss->slots, hipMemcpyDeviceToDevice, ss->rstream[0]));
		++ss->collectives;
	} else {   // asked for, or no RCCL on this node: the same pieces through the host
		std::vector<char> all(size_t(ss->nranks) * ss->slots * bytes);
		for (uint32_t r = 0; r < ss->nranks; ++r) {
			RX_HIP(hipSetDevice(ss->rank_dev[r]));
			RX_HIP(hipMemcpyAsync(all.data() + size_t(r) * ss->slots * bytes, ss->d_send[k][r].ptr, ss->slots * bytes, hipMemcpyDeviceToHost, ss->rstream[r]));
		}
		for (uint32_t r = 0; r < ss->nranks; ++r) {
			RX_HIP(hipSetDevice(ss->rank_dev[r]));
			RX_HIP(hipStreamSynchronize(ss->rstream[r]));
		}
		for (uint32_t r = 0; r < ss->nranks; ++r) {
			RX_HIP(hipSetDevice(ss->rank_dev[r]));
			RX_HIP(hipMemcpyAsync(ss->d_recv[k][r].ptr, all.data(), all.size(), hipMemcpyHostToDevice, ss->rstream[r]));
			RX_HIP(hipStreamSynchronize(ss->rstream[r]));   // (`all` goes out of scope)
		}
	}
	for (uint32_t r = 0; r < ss->nranks; ++r) {
		RX_HIP(hipSetDevice(ss->rank_dev[r]));
		RX_HIP(hipEventRecord(ss->ev_rank[r], ss->rstream[r]));
	}
	for (size_t s = 0; s < S; ++s) {
		RX_HIP(hipSetDevice(ss->devices[s]));
		RX_HIP(hipStreamWaitEvent(ss->shards[s]->stream, ss->ev_rank[ss->shard_rank[s]], 0));
	}
	return RXGPU_OK;
}

int ft_shards_buffers(rxgpu_ft_shard_set* ss, int k, size_t bytes) {
	for (uint32_t r = 0; r < ss->nranks; ++r) {
		RX_HIP(hipSetDevice(ss->rank_dev[r]));
		const bool grow = ss->d_send[k][r].bytes < bytes * ss->slots;
		if (int rc = ss->d_send[k][r].ensure(bytes * ss->slots); rc) return rc;
		if (int rc = ss->d_recv[k][r].ensure(bytes * ss->slots * ss->nranks); rc) return rc;
		if (grow) RX_HIP(hipMemset(ss->d_send[k][r].ptr, 0, ss->d_send[k][r].bytes));   // padded slots (a device with fewer shards) stay zero
	}
	return RXGPU_OK;
}
inline char* ft_send_ptr(rxgpu_ft_shard_set* ss, int k, size_t s, size_t bytes) {
	return static_cast<char*>(ss->d_send[k][ss->shard_rank[s]].ptr) + size_t(ss->shard_slot[s]) * bytes;
}
}  // namespace

namespace rxgpu {

// ---- the sharded handle's side of the dictionary calls (the merge itself: run_merge_sharded)
int ft_shards_set_docs(rxgpu_ft_index* h, uint64_t total_docs, const float* words_in_field, const float* avg_words, const uint8_t* removed) {
	rxgpu_ft_shard_set* ss = h->shard_set;
	std::lock_guard<std::mutex> lk(h->mtx);
	const uint32_t S = uint32_t(ss->shards.size());
	const uint32_t n_ranges = uint32_t((total_docs + rxgpu::kFtRangeDocs - 1) / rxgpu::kFtRangeDocs);
	// The cut: shard s starts at range s * per.  It is fixed by the first rxgpu_ft_set_docs and KEPT while any shard holds words — the index
	// grows through step commits (IndexText::commitFulltextImpl calls this with a larger totalDocs and re-uploads only the changed words),
	// and the fragments already on the shards must stay where the cut put them: new ranges go to the last shard, an even cut comes back
	// with the next index built from scratch (rxgpu_ft_shard_imbalance tells the caller when that is worth it).
	bool holds_words = false;
	for (rxgpu_ft_index* sh : ss->shards) holds_words = holds_words || !sh->words.empty();
	if (!ss->per || !holds_words) ss->per = std::max<uint32_t>(1, (n_ranges + S - 1) / S);
	const uint32_t per = ss->per;
	for (uint32_t s = 0; s < S; ++s) {
		rxgpu_ft_index* sh = ss->shards[s];
		if (int rc = rxgpu_ft_set_docs(sh, total_docs, words_in_field, avg_words, removed); rc) return rc;   // replicated: a few bytes per document
		sh->sh_index = s;
		sh->sh_total = S;
		sh->sh_range_begin = std::min(s * per, n_ranges);
		sh->sh_range_count = s + 1 == S ? n_ranges - sh->sh_range_begin : std::min(per, n_ranges - sh->sh_range_begin);
	}
	ss->n_ranges = n_ranges;
	h->total_docs = total_docs;
	return RXGPU_OK;
}

// One dictionary word: every shard takes the postings of ITS documents (ids stay global) and the whole list's length as document frequency.
// Either the flat form (ent_*) or the positions form (pos_off / fpos).
int ft_shards_set_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* ent_off, const uint8_t* ent_field,
					   const uint32_t* ent_tf, const uint32_t* ent_first_pos, const uint32_t* pos_off, const uint64_t* fpos) {
	rxgpu_ft_shard_set* ss = h->shard_set;
	std::lock_guard<std::mutex> lk(h->mtx);
	RX_CHECK(ss->n_ranges > 0, RXGPU_ERR_LOGIC, "a sharded ft index cuts its posting lists at the document ranges: call rxgpu_ft_set_docs first");
	for (uint64_t i = 1; i < n; ++i) RX_CHECK(doc[i] > doc[i - 1], RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: document ids must ascend strictly");
	RX_CHECK(n == 0 || doc[n - 1] < h->total_docs, RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: a posting list holds a document id >= total_docs (rxgpu_ft_set_docs)");
	for (rxgpu_ft_index* sh : ss->shards) {
		const uint64_t d_lo = uint64_t(sh->sh_range_begin) * rxgpu::kFtRangeDocs, d_hi = d_lo + uint64_t(sh->sh_range_count) * rxgpu::kFtRangeDocs;
		const uint64_t a = uint64_t(std::lower_bound(doc, doc + n, d_lo, [](uint32_t x, uint64_t v) { return uint64_t(x) < v; }) - doc);
		const uint64_t b = uint64_t(std::lower_bound(doc, doc + n, d_hi, [](uint32_t x, uint64_t v) { return uint64_t(x) < v; }) - doc);
		const uint64_t m = b - a;
		int rc;
		if (pos_off) {
			std::vector<uint32_t> po(m + 1);
			for (uint64_t i = 0; i <= m; ++i) po[i] = pos_off[a + i] - pos_off[a];
			rc = rxgpu_ft_set_word_positions(sh, word_id, m, m ? doc + a : nullptr, po.data(), m ? fpos + pos_off[a] : nullptr);
		} else {
			std::vector<uint32_t> eo(m + 1);
			for (uint64_t i = 0; i <= m; ++i) eo[i] = ent_off[a + i] - ent_off[a];
			const uint32_t e0 = m ? ent_off[a] : 0;
			rc = rxgpu_ft_set_word(sh, word_id, m, m ? doc + a : nullptr, eo.data(), ent_field + e0, ent_tf + e0, ent_first_pos + e0);
		}
		if (rc) return rc;
		std::lock_guard<std::mutex> slk(sh->mtx);
		std::unique_lock<std::shared_mutex> dict_lk(sh->dict_mtx);
		sh->words[word_id].df = n;   // (an empty fragment keeps its entry: the word's row exists on every shard)
	}
	return RXGPU_OK;
}

void ft_shards_destroy(rxgpu_ft_shard_set* ss) {
	if (!ss) return;
	for (rxgpu_ft_index* sh : ss->shards) rxgpu_ft_destroy(sh);
	for (uint32_t r = 0; r < ss->nranks; ++r) {
		(void)hipSetDevice(ss->rank_dev[r]);
		if (r < ss->rstream.size() && ss->rstream[r]) (void)hipStreamDestroy(ss->rstream[r]);
		if (r < ss->ev_rank.size() && ss->ev_rank[r]) (void)hipEventDestroy(ss->ev_rank[r]);
		if (r < ss->d_pos.size() && ss->d_pos[r]) (void)hipFree(ss->d_pos[r]);
		for (int k = 0; k < 2; ++k) {
			if (r < ss->d_send[k].size()) ss->d_send[k][r].release();
			if (r < ss->d_recv[k].size()) ss->d_recv[k][r].release();
		}
	}
	for (size_t s = 0; s < ss->ev_shard.size(); ++s) {
		if (ss->ev_shard[s]) {
			(void)hipSetDevice(ss->devices[s]);
			(void)hipEventDestroy(ss->ev_shard[s]);
		}
	}
	delete ss;
}

// One merge over all shards (the caller holds the sharded handle's mutex): the ordinary launch train in its three pieces, the two exchanges
// between them, every shard's packed result, the slot-wise union.
int run_merge_sharded(rxgpu_ft_index* parent, const MergeQuery& q, const MergeOut& out) {
	rxgpu_ft_shard_set* ss = parent->shard_set;
	const rxgpu_ft_config* cfg = q.cfg;
	const std::vector<QueryTermIn>& terms = *q.terms;
	const float* procs = q.procs;
	const AreasOut* areas = q.areas;
	const char* who = q.who;
	const uint32_t max_areas = q.max_areas();
	uint32_t* out_doc = out.doc;
	float* out_proc = out.proc;
	uint8_t* out_field = out.field;
	uint16_t* out_terms_counter = out.terms_counter;
	const size_t S = ss->shards.size();
	RX_CHECK(ss->n_ranges > 0, RXGPU_ERR_LOGIC, std::string(who) + ": rxgpu_ft_set_docs was not called");
	int prev_dev = -1;
	(void)hipGetDevice(&prev_dev);
	struct Restore {
		int d;
		~Restore() { if (d >= 0) (void)hipSetDevice(d); }
	} restore{prev_dev};
	// exchange buffers first: the plans carry pointers into them
	const size_t fold_bytes = size_t(rxgpu::kFtFoldWords) * 4;
	const size_t nsubs = terms.empty() ? 0 : terms.back().sub_end;
	const size_t table_stride = std::max<size_t>(1, nsubs) * ss->n_ranges;   // >= rows x ranges of the plan (every sub-term is at most one row)
	if (int rc = ft_shards_buffers(ss, 0, fold_bytes); rc) return rc;
	if (int rc = ft_shards_buffers(ss, 1, table_stride * 4); rc) return rc;
	std::vector<MergeJob> jobs(S);
	std::vector<std::unique_lock<std::mutex>> locks;
	std::vector<std::shared_lock<std::shared_mutex>> dicts;
	std::vector<bool> active(S, false);
	bool empty = false;
	for (size_t s = 0; s < S; ++s) {
		locks.emplace_back(ss->shards[s]->mtx);
		dicts.emplace_back(ss->shards[s]->dict_mtx);
	}
	// Phrases first, on every shard (Merger::init, merger.h:73-81): a phrase is decided inside a document, so every shard runs PhraseMerger over
	// its own fragments; what spans the shards is NumDocsMerged() — the 2-phase estimate takes the sum — and the numbering of the phrase's rows.
	bool any_phrase = false;
	for (const QueryTermIn& t : terms) any_phrase = any_phrase || t.phrase_num >= 0;
	std::vector<std::vector<PhraseRows>> phrases(S);
	if (any_phrase) {
		for (size_t s = 0; s < S; ++s) {
			RX_HIP(hipSetDevice(ss->devices[s]));
			bool nothing = false;
			if (int rc = prepare_shard_phrases(ss->shards[s], q, phrases[s], &nothing); rc) return rc;
			if (nothing) return RXGPU_OK;   // min(mergeLimit, totalORVids) == 0: alike on every shard
		}
		// the admission cut of the whole index (phrasemerger.h:341): the first mergeLimit candidates in (row, document) order — row by row,
		// inside a row shard after shard (a shard's documents lie before the next one's).  What a shard keeps is a prefix of its own slots.
		for (size_t pi = 0; pi < phrases[0].size(); ++pi) {
			size_t n_rows = 0;
			bool any_pending = false;
			for (size_t s = 0; s < S; ++s) {
				RX_CHECK(phrases[s].size() == phrases[0].size(), RXGPU_ERR_LOGIC, std::string(who) + ": the shards disagree on the parts of the query");
				const PhraseRows& pr = phrases[s][pi];
				const size_t r = pr.pending ? pr.pending->row_admitted.size() : pr.rows.size();
				RX_CHECK(s == 0 || r == n_rows, RXGPU_ERR_LOGIC, std::string(who) + ": the shards disagree on the rows of a phrase");
				n_rows = r;
				any_pending = any_pending || pr.pending;
			}
			if (!any_pending) continue;
			std::vector<std::vector<uint32_t>> counts(S);
			for (size_t s = 0; s < S; ++s) {
				if (phrases[s][pi].pending) counts[s] = phrases[s][pi].pending->row_admitted;
			}
			const std::vector<uint64_t> keep = rxgpu::ft_shard_phrase_cut(counts, n_rows, cfg->merge_limit);
			for (size_t s = 0; s < S; ++s) {
				PhraseRows& pr = phrases[s][pi];
				if (!pr.pending) continue;
				pr.pending->admitted = uint32_t(std::min<uint64_t>(pr.pending->admitted, keep[s]));
				RX_HIP(hipSetDevice(ss->devices[s]));
				if (int rc = finish_phrase(ss->shards[s], procs, *pr.pending, pr, who); rc) return rc;
				pr.pending.reset();
			}
		}
		for (size_t pi = 0; pi < phrases[0].size(); ++pi) {
			uint64_t admitted = 0;
			for (size_t s = 0; s < S; ++s) {
				RX_CHECK(phrases[s].size() == phrases[0].size() && phrases[s][pi].rows.size() == phrases[0][pi].rows.size(), RXGPU_ERR_LOGIC,
						 std::string(who) + ": the shards disagree on the rows of a phrase");
				admitted += phrases[s][pi].admitted;
			}
			for (size_t s = 0; s < S; ++s) phrases[s][pi].admitted = uint32_t(std::min<uint64_t>(admitted, 0xFFFFFFFFull));
		}
	}
	for (size_t s = 0; s < S; ++s) {
		rxgpu_ft_index* sh = ss->shards[s];
		RX_HIP(hipSetDevice(ss->devices[s]));
		active[s] = sh->sh_range_count != 0;
		sh->sh_hist = static_cast<const uint32_t*>(ss->d_recv[0][ss->shard_rank[s]].ptr);
		sh->sh_pos = ss->d_pos[ss->shard_rank[s]];
		if (int rc = prepare_shard_merge(sh, q, any_phrase ? &phrases[s] : nullptr, jobs[s]); rc) return rc;
		empty = empty || jobs[s].empty;
		sh->clean_dirty = !jobs[s].empty;   // an error return from here on leaves the kept-clean tables in an unknown state
	}
	if (empty) return RXGPU_OK;   // min(mergeLimit, totalORVids) == 0 — decided on the whole index's counts, alike on every shard
	const uint64_t M = jobs[0].max_merged;
	RX_CHECK(out.cap >= M, RXGPU_ERR_OVERFLOW, std::string(who) + ": output buffers too small");
	const bool prescore = jobs[0].p.prescore != 0;
	auto phase = [&](int ph) -> int {
		for (size_t s = 0; s < S; ++s) {
			if (!active[s]) continue;
			RX_HIP(hipSetDevice(ss->devices[s]));
			RX_HIP(rxgpu::launch_ft_merge_phase(jobs[s].d_plan, &jobs[s].p, 1, ph, ss->shards[s]->stream));
		}
		return RXGPU_OK;
	};
	if (int rc = phase(0); rc) return rc;
	if (prescore) {   // the histogram + popcount of every shard -> the sums; gate, threshold and tie quota are the whole index's
		for (size_t s = 0; s < S; ++s) {
			RX_HIP(hipSetDevice(ss->devices[s]));
			uint32_t* dst = reinterpret_cast<uint32_t*>(ft_send_ptr(ss, 0, s, fold_bytes));
			if (active[s]) {
				rxgpu::launch_ft_shard_fold(jobs[s].d_plan, dst, ss->shards[s]->stream);
			} else {
				RX_HIP(hipMemsetAsync(dst, 0, fold_bytes, ss->shards[s]->stream));
			}
		}
		if (int rc = ft_shards_gather(ss, 0, fold_bytes); rc) return rc;
		for (size_t s = 0; s < S; ++s) {
			if (!active[s]) continue;
			RX_HIP(hipSetDevice(ss->devices[s]));
			rxgpu::launch_ft_shard_hist_combine(jobs[s].d_plan, static_cast<const uint32_t*>(ss->d_recv[0][ss->shard_rank[s]].ptr), ss->d_pos[ss->shard_rank[s]],
												uint32_t(S), ss->shards[s]->stream);
		}
	}
	if (int rc = phase(1); rc) return rc;
	{   // the adder tables: every shard's own columns -> the table of the whole index
		const size_t n_table = size_t(jobs[0].p.n_rows) * jobs[0].p.n_ranges;
		for (size_t s = 0; s < S; ++s) {
			RX_HIP(hipSetDevice(ss->devices[s]));
			char* dst = ft_send_ptr(ss, 1, s, table_stride * 4);
			if (active[s] && n_table) {
				RX_HIP(hipMemcpyAsync(dst, jobs[s].p.adders, n_table * 4, hipMemcpyDeviceToDevice, ss->shards[s]->stream));
			} else {
				RX_HIP(hipMemsetAsync(dst, 0, std::max<size_t>(4, n_table * 4), ss->shards[s]->stream));
			}
		}
		if (int rc = ft_shards_gather(ss, 1, table_stride * 4); rc) return rc;
		for (size_t s = 0; s < S; ++s) {
			if (!active[s]) continue;
			RX_HIP(hipSetDevice(ss->devices[s]));
			rxgpu::launch_ft_shard_table_sum(jobs[s].p.adders, static_cast<const uint32_t*>(ss->d_recv[1][ss->shard_rank[s]].ptr), ss->d_pos[ss->shard_rank[s]], uint32_t(S),
											 n_table, table_stride, ss->shards[s]->stream);
		}
	}
	if (int rc = phase(2); rc) return rc;
	for (size_t s = 0; s < S; ++s) {
		if (!active[s]) continue;
		RX_HIP(hipSetDevice(ss->devices[s]));
		RX_HIP(rxgpu::launch_ft_export(jobs[s].d_plan, &jobs[s].p, 1, ss->shards[s]->stream));
	}
	// MergeDataAreas: {held, insertions} per (merge slot, field) and the areas as every shard's replay left them — a document's areas are
	// built where the document lies, at its GLOBAL merge slot, so the caller's arrays are the slot-wise union too
	const size_t nf = parent->num_fields;
	std::vector<std::vector<uint32_t>> area_hdr(areas ? S : 0), area_data(areas ? S : 0);
	for (size_t s = 0; s < S && areas; ++s) {
		if (!active[s]) continue;
		RX_HIP(hipSetDevice(ss->devices[s]));
		area_hdr[s].resize(size_t(M) * nf * 2);
		area_data[s].resize(jobs[s].area_bytes / sizeof(uint32_t));
		RX_HIP(hipMemcpyAsync(area_hdr[s].data(), jobs[s].p.area_hdr, area_hdr[s].size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ss->shards[s]->stream));
		RX_HIP(hipMemcpyAsync(area_data[s].data(), jobs[s].p.out_areas, jobs[s].area_bytes, hipMemcpyDeviceToHost, ss->shards[s]->stream));
	}
	for (size_t s = 0; s < S; ++s) {
		RX_HIP(hipSetDevice(ss->devices[s]));
		RX_HIP(hipStreamSynchronize(ss->shards[s]->stream));
	}
	++ss->merges;
	// ---- the slot-wise union: every merge slot was written by exactly one shard (the others left their 0xFFFFFFFF mark)
	uint64_t n = 0;
	bool have_n = false;
	int32_t presel = 0;
	for (size_t s = 0; s < S; ++s) {
		if (!active[s]) continue;
		const uint32_t* hdr = static_cast<const uint32_t*>(ss->shards[s]->h_pinned);
		if (int rc = check_result_header(hdr, UINT64_MAX, who); rc) return rc;   // the look-back word; the count once the shards agree on it
		RX_CHECK(!have_n || hdr[0] == n, RXGPU_ERR_DEVICE, std::string(who) + ": the shards disagree on the number of merged documents");
		n = hdr[0];
		have_n = true;
		presel = presel || hdr[2];
		ss->shards[s]->clean_dirty = false;
		ss->shards[s]->stat_postings += jobs[s].merged_postings;
	}
	RX_CHECK(n <= M, RXGPU_ERR_DEVICE, std::string(who) + ": corrupt result header");
	std::vector<uint8_t> filled(n, 0);
	const rxgpu::FtOutLayout ol = rxgpu::ft_out_layout(M);
	for (size_t s = 0; s < S; ++s) {
		if (!active[s]) continue;
		const char* hp = static_cast<const char*>(ss->shards[s]->h_pinned);
		const uint32_t* sd = reinterpret_cast<const uint32_t*>(hp + ol.doc);
		const float* sp = reinterpret_cast<const float*>(hp + ol.proc);
		const uint16_t* st_ = reinterpret_cast<const uint16_t*>(hp + ol.terms_counter);
		const uint8_t* sf = reinterpret_cast<const uint8_t*>(hp + ol.field);
		for (uint64_t i = 0; i < n; ++i) {
			if (sd[i] == 0xFFFFFFFFu) continue;
			RX_CHECK(!filled[i], RXGPU_ERR_DEVICE, std::string(who) + ": two shards wrote one merge slot");
			filled[i] = 1;
			out_doc[i] = sd[i];
			out_proc[i] = sp[i];
			if (out_terms_counter) out_terms_counter[i] = st_[i];
			out_field[i] = sf[i];
			if (areas) {
				const size_t per_doc = nf * size_t(max_areas) * 3;
				for (size_t f = 0; f < nf; ++f) areas->cnt[i * nf + f] = area_hdr[s][(i * nf + f) * 2];
				std::memcpy(areas->areas + i * per_doc, area_data[s].data() + i * per_doc, per_doc * sizeof(uint32_t));
			}
		}
	}
	for (uint64_t i = 0; i < n; ++i) RX_CHECK(filled[i], RXGPU_ERR_DEVICE, std::string(who) + ": a merge slot no shard wrote");
	if (n && jobs[0].nsyn && out_terms_counter) {   // the documents that hold only parts of a multi-word synonym go (mergerimpl.h:533-555), as in collect_merge
		uint64_t kept = 0;
		for (uint64_t i = 0; i < n; ++i) {
			if (out_terms_counter[i] == 0xFFFFu) continue;
			out_doc[kept] = out_doc[i];
			out_proc[kept] = out_proc[i];
			out_terms_counter[kept] = out_terms_counter[i];
			out_field[kept] = out_field[i];
			++kept;
		}
		n = kept;
	}
	*out.n = n;
	if (out.preselected) *out.preselected = presel;
	return RXGPU_OK;
}

}  // namespace rxgpu

extern "C" {

int rxgpu_ft_create_sharded(uint32_t num_fields, uint32_t n_devices, const int* devices, rxgpu_ft_index** out) {
	RX_CHECK(out && devices && n_devices >= 1 && n_devices <= 64, RXGPU_ERR_PARAMS, "rxgpu_ft_create_sharded: bad arguments (1..64 devices)");
	*out = nullptr;
	int prev = -1;
	(void)hipGetDevice(&prev);
	rxgpu_ft_index* h = nullptr;
	if (int rc = rxgpu_ft_create(num_fields, devices[0], &h); rc) return rc;   // the handle the caller holds: no dictionary of its own
	auto* ss = new rxgpu_ft_shard_set();
	h->shard_set = ss;
	auto fail = [&](int rc) {
		const std::string msg = rxgpu_last_error();
		rxgpu_ft_destroy(h);
		if (prev >= 0) (void)hipSetDevice(prev);
		set_error(msg);
		return rc;
	};
	for (uint32_t s = 0; s < n_devices; ++s) {
		rxgpu_ft_index* sh = nullptr;
		if (int rc = rxgpu_ft_create(num_fields, devices[s], &sh); rc) return fail(rc);
		ss->shards.push_back(sh);
		ss->devices.push_back(devices[s]);
	}
	const rxgpu::RankLayout lay = rxgpu::rank_layout(devices, n_devices);   // shard_plan.h: the layout of the float_vector shards' exchange
	ss->nranks = lay.nranks;
	ss->slots = lay.slots;
	ss->rank_dev = lay.rank_dev;
	ss->shard_rank = lay.shard_rank;
	ss->shard_slot = lay.shard_slot;
	ss->pos = lay.pos;
	ss->rstream.assign(ss->nranks, nullptr);
	ss->ev_rank.assign(ss->nranks, nullptr);
	ss->d_pos.assign(ss->nranks, nullptr);
	ss->ev_shard.assign(n_devices, nullptr);
	for (int k = 0; k < 2; ++k) {
		ss->d_send[k].resize(ss->nranks);
		ss->d_recv[k].resize(ss->nranks);
	}
	for (uint32_t r = 0; r < ss->nranks; ++r) {
		hipError_t e = hipSetDevice(ss->rank_dev[r]);
		if (e == hipSuccess) e = hipStreamCreateWithFlags(&ss->rstream[r], hipStreamNonBlocking);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&ss->ev_rank[r], hipEventDisableTiming);
		if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&ss->d_pos[r]), ss->pos.size() * sizeof(uint32_t));
		if (e == hipSuccess) e = hipMemcpy(ss->d_pos[r], ss->pos.data(), ss->pos.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
		if (e != hipSuccess) {
			set_error(std::string("rxgpu_ft_create_sharded: device ") + std::to_string(ss->rank_dev[r]) + ": " + hipGetErrorString(e));
			return fail(RXGPU_ERR_DEVICE);
		}
	}
	for (uint32_t s = 0; s < n_devices; ++s) {
		hipError_t e = hipSetDevice(devices[s]);
		if (e == hipSuccess) e = hipEventCreateWithFlags(&ss->ev_shard[s], hipEventDisableTiming);
		if (e != hipSuccess) {
			set_error(std::string("rxgpu_ft_create_sharded: ") + hipGetErrorString(e));
			return fail(RXGPU_ERR_DEVICE);
		}
	}
	// the exchange: RXGPU_SHARD_MERGE=host -> through the host; one device -> copies on that device; several devices -> one RCCL
	// communicator over them (opened on demand; missing / failing: through the host, one line on stderr)
	const char* mode = getenv("RXGPU_SHARD_MERGE");
	if (mode && std::strcmp(mode, "host") == 0) {
		ss->host_exchange = true;
		ss->note = "RXGPU_SHARD_MERGE=host";
	} else if (ss->nranks > 1) {
		ss->cs = rxgpu::rccl_comm_set(ss->rank_dev, &ss->note);
		if (!ss->cs) {
			ss->host_exchange = true;
			fprintf(stderr, "rxgpu: sharded ft index over %u device slot(s): %s — the shards' histograms and tables travel through the host\n", n_devices, ss->note.c_str());
		}
	}
	if (prev >= 0) (void)hipSetDevice(prev);
	*out = h;
	return RXGPU_OK;
}
uint32_t rxgpu_ft_shard_count(const rxgpu_ft_index* h) { return h && h->shard_set ? uint32_t(h->shard_set->shards.size()) : 0; }
// ranges of the fullest shard / ranges of an even cut (1.0: even; an index that grew by step commits piles its new ranges on the last shard)
double rxgpu_ft_shard_imbalance(const rxgpu_ft_index* h) {
	if (!h || !h->shard_set || !h->shard_set->n_ranges) return 1.0;
	const rxgpu_ft_shard_set* ss = h->shard_set;
	uint32_t most = 0;
	for (const rxgpu_ft_index* sh : ss->shards) most = std::max(most, sh->sh_range_count);
	const double even = double(ss->n_ranges) / double(ss->shards.size());
	return even > 0 ? std::max(1.0, double(most) / std::max(1.0, even)) : 1.0;
}
int rxgpu_ft_shard_exchange_mode(const rxgpu_ft_index* h) { return h && h->shard_set ? (h->shard_set->host_exchange ? 0 : 1) : -1; }
uint64_t rxgpu_ft_shard_collectives(const rxgpu_ft_index* h) { return h && h->shard_set ? h->shard_set->collectives : 0; }
int rxgpu_ft_shard_ranges(const rxgpu_ft_index* h, uint32_t shard, uint32_t* range_begin, uint32_t* range_count) {
	RX_CHECK(h && h->shard_set && shard < h->shard_set->shards.size() && range_begin && range_count, RXGPU_ERR_PARAMS, "rxgpu_ft_shard_ranges: bad arguments");
	*range_begin = h->shard_set->shards[shard]->sh_range_begin;
	*range_count = h->shard_set->shards[shard]->sh_range_count;
	return RXGPU_OK;
}

}  // extern "C"
