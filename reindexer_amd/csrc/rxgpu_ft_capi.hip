// C-ABI of the BM25 merge (include/rxgpu.h, rxgpu_ft_*): the device mirror of the ft_fast posting lists — lifetime of an index, its lanes, the
// dictionary calls.  The merges: rxgpu_ft_merge.hip (one merge), rxgpu_ft_calls.hip (the entry points); the other units: rxgpu_ft_internal.h.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rxgpu_ft_internal.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

namespace {
void release_lane(rxgpu_ft_index* h) {   // what a lane owns: stream, scratch, staging, events
	for (rxgpu_devbuf* b : {&h->d_state, &h->d_out, &h->d_clean, &h->d_fuse, &h->d_excl, &h->d_areas, &h->d_pk_in, &h->d_pk_cnt, &h->d_pk_segs, &h->d_pk_outs}) b->release();
	for (rxgpu_devbuf& b : h->d_phrase_a) b.release();
	for (rxgpu_devbuf& b : h->d_phrase_b) b.release();
	for (hipEvent_t e : {h->ev_knn, h->ev_fa, h->ev_fb, h->ev_pa, h->ev_pb, h->ev_pha, h->ev_phb}) {
		if (e) (void)hipEventDestroy(e);
	}
	for (hipStream_t& ps : h->pk_streams) {
		if (ps) (void)hipStreamDestroy(ps);
		ps = nullptr;
	}
	if (h->h_pinned) (void)hipHostFree(h->h_pinned);
	if (h->ev_a) (void)hipEventDestroy(h->ev_a);
	if (h->ev_b) (void)hipEventDestroy(h->ev_b);
	if (h->stream) (void)hipStreamDestroy(h->stream);
}

constexpr uint32_t kFtMaxLanes = 16;
uint32_t ft_lane_limit() {
	static const uint32_t v = [] {
		const char* e = std::getenv("RXGPU_FT_LANES");
		const long n = e && *e ? std::atol(e) : 4;
		return uint32_t(n < 1 ? 1 : (n > long(kFtMaxLanes) ? long(kFtMaxLanes) : n));
	}();
	return v;
}
}  // namespace

namespace rxgpu {

int make_lane(rxgpu_ft_index* h, bool stream, std::unique_ptr<rxgpu_ft_index>& out) {
	auto lane = std::make_unique<rxgpu_ft_index>();
	lane->device = h->device;
	lane->num_fields = h->num_fields;
	lane->root = h;
	if (stream) {
		rxgpu::DeviceGuard dg(h->device);
		if (hipStreamCreateWithFlags(&lane->stream, hipStreamNonBlocking) != hipSuccess) {
			set_error("hipStreamCreateWithFlags failed");
			return RXGPU_ERR_DEVICE;
		}
	}
	out = std::move(lane);
	return RXGPU_OK;
}
void lane_adopt_docs(rxgpu_ft_index* l, const rxgpu_ft_index* h) {
	l->total_docs = h->total_docs;
	l->d_words = h->d_words;
	l->d_avg = h->d_avg;
	l->d_removed = h->d_removed;
	l->d_removed_bits = h->d_removed_bits;
	l->h_avg = h->h_avg;
}

int checkout_lane(rxgpu_ft_index* h, LaneLock& out) {
	if (h->shard_set) {   // a sharded index runs one merge at a time: every shard's handle is busy with it
		out.lane = h;
		out.lk = std::unique_lock<std::mutex>(h->mtx);
		out.dict = std::shared_lock<std::shared_mutex>(h->dict_mtx);
		return RXGPU_OK;
	}
	auto take = [&](rxgpu_ft_index* l, std::unique_lock<std::mutex>&& lk) {
		out.lane = l;
		out.lk = std::move(lk);
		out.dict = std::shared_lock<std::shared_mutex>(h->dict_mtx);
		if (l != h) lane_adopt_docs(l, h);
	};
	{
		std::unique_lock<std::mutex> lk(h->mtx, std::try_to_lock);
		if (lk.owns_lock() && !h->res_session) {   // (a resident merge parked on the handle: ordinary merges take the other lanes)
			take(h, std::move(lk));
			return RXGPU_OK;
		}
	}
	std::vector<rxgpu_ft_index*> have;
	{
		std::lock_guard<std::mutex> g(h->lanes_mtx);
		for (auto& l : h->lanes) have.push_back(l.get());
	}
	for (rxgpu_ft_index* l : have) {
		std::unique_lock<std::mutex> lk(l->mtx, std::try_to_lock);
		if (lk.owns_lock()) {
			take(l, std::move(lk));
			return RXGPU_OK;
		}
	}
	if (have.size() + 1 < std::max<uint32_t>(ft_lane_limit(), 2)) {   // (at least one lane besides the handle: a parked resident merge keeps the handle busy)
		std::unique_ptr<rxgpu_ft_index> lane;
		if (int rc = make_lane(h, true, lane); rc) return rc;
		rxgpu_ft_index* l = lane.get();
		std::unique_lock<std::mutex> lk(l->mtx);
		{
			std::lock_guard<std::mutex> g(h->lanes_mtx);
			h->lanes.push_back(std::move(lane));
		}
		take(l, std::move(lk));
		return RXGPU_OK;
	}
	uint32_t turn = h->next_lane.fetch_add(1) % uint32_t(have.size() + 1);
	if (turn == 0) {
		std::unique_lock<std::mutex> lk(h->mtx);
		if (!h->res_session) {
			take(h, std::move(lk));
			return RXGPU_OK;
		}
		turn = 1;   // (have is not empty: the branch above makes a second lane before anyone queues)
	}
	rxgpu_ft_index* l = have[turn - 1];
	take(l, std::unique_lock<std::mutex>(l->mtx));
	return RXGPU_OK;
}

}  // namespace rxgpu

extern "C" {

int rxgpu_ft_create(uint32_t num_fields, int device, rxgpu_ft_index** out) {
	RX_CHECK(out, RXGPU_ERR_PARAMS, "rxgpu_ft_create: out is null");
	RX_CHECK(num_fields >= 1 && num_fields <= 63, RXGPU_ERR_PARAMS, "rxgpu_ft_create: 1..63 fields (kMaxFtCompositeFields)");
	int ndev = 0;
	RX_HIP(hipGetDeviceCount(&ndev));
	RX_CHECK(device >= 0 && device < ndev, RXGPU_ERR_PARAMS, "rxgpu_ft_create: no such device");
	rxgpu::DeviceGuard dg(device);
	auto* h = new rxgpu_ft_index();
	h->device = device;
	h->num_fields = num_fields;
	if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
		delete h;
		set_error("hipStreamCreateWithFlags failed");
		return RXGPU_ERR_DEVICE;
	}
	*out = h;
	return RXGPU_OK;
}

void rxgpu_ft_destroy(rxgpu_ft_index* h) {
	if (!h) return;
	if (h->shard_set) {
		rxgpu::DeviceGuard dgs(h->device);
		ft_shards_destroy(h->shard_set);
		h->shard_set = nullptr;
	}
	rxgpu::DeviceGuard dg(h->device);
	(void)rxgpu::device_wait_all(h->device);
	for (auto& kv : h->words) kv.second.release();
	for (void* p : {static_cast<void*>(h->d_words), static_cast<void*>(h->d_avg), static_cast<void*>(h->d_removed), static_cast<void*>(h->d_removed_bits)}) {
		if (p) (void)hipFree(p);
	}
	for (auto& l : h->lanes) release_lane(l.get());
	for (auto& l : h->batch_lanes) release_lane(l.get());
	h->d_batch_plans.release();
	if (h->h_batch_plans) (void)hipHostFree(h->h_batch_plans);
	if (h->ev_ba) (void)hipEventDestroy(h->ev_ba);
	if (h->ev_bb) (void)hipEventDestroy(h->ev_bb);
	if (h->batch_stream) (void)hipStreamDestroy(h->batch_stream);
	release_lane(h);
	delete h;
}

int rxgpu_ft_set_docs(rxgpu_ft_index* h, uint64_t total_docs, const float* words_in_field, const float* avg_words, const uint8_t* removed) {
	RX_CHECK(h && words_in_field && avg_words, RXGPU_ERR_PARAMS, "rxgpu_ft_set_docs: null argument");
	RX_CHECK(total_docs >= 1 && total_docs < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "rxgpu_ft_set_docs: total_docs out of range");
	if (h->shard_set) return ft_shards_set_docs(h, total_docs, words_in_field, avg_words, removed);
	std::lock_guard<std::mutex> lk(h->mtx);
	std::unique_lock<std::shared_mutex> dict_lk(h->dict_mtx);   // no merge on any lane reads the dictionary meanwhile
	rxgpu::DeviceGuard dg(h->device);
	RX_HIP(hipStreamSynchronize(h->stream));
	if (int rc = upload(h->d_words, words_in_field, total_docs * h->num_fields); rc) return rc;
	if (int rc = upload(h->d_avg, avg_words, h->num_fields); rc) return rc;
	bool any_removed = false;
	if (removed) {
		if (int rc = upload(h->d_removed, removed, total_docs); rc) return rc;
		std::vector<uint32_t> bits((total_docs + 31) / 32, 0u);
		for (uint64_t d = 0; d < total_docs; ++d) {
			if (removed[d]) {
				bits[d >> 5] |= 1u << (d & 31);
				any_removed = true;
			}
		}
		if (any_removed) {
			if (int rc = upload(h->d_removed_bits, bits.data(), bits.size()); rc) return rc;
		}
	} else {
		if (h->d_removed) (void)hipFree(h->d_removed);
		h->d_removed = nullptr;
	}
	if (!any_removed && h->d_removed_bits) {
		(void)hipFree(h->d_removed_bits);
		h->d_removed_bits = nullptr;
	}
	h->h_avg.assign(avg_words, avg_words + h->num_fields);
	h->total_docs = total_docs;
	return RXGPU_OK;
}

int rxgpu_ft_set_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* ent_off, const uint8_t* ent_field,
					  const uint32_t* ent_tf, const uint32_t* ent_first_pos) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null ft index");
	RX_CHECK(n == 0 || (doc && ent_off && ent_field && ent_tf && ent_first_pos), RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: null argument");
	if (h->shard_set) return ft_shards_set_word(h, word_id, n, doc, ent_off, ent_field, ent_tf, ent_first_pos, nullptr, nullptr);
	std::lock_guard<std::mutex> lk(h->mtx);
	std::unique_lock<std::shared_mutex> dict_lk(h->dict_mtx);   // no merge on any lane reads the dictionary meanwhile
	rxgpu::DeviceGuard dg(h->device);
	RX_HIP(hipStreamSynchronize(h->stream));
	rxgpu_ft_word& w = h->words[word_id];
	w.release();
	if (n == 0) return RXGPU_OK;
	const uint64_t nent = ent_off[n];
	if (int rc = upload(w.doc, doc, n); rc) return rc;
	if (int rc = upload(w.ent_off, ent_off, n + 1); rc) return rc;
	if (int rc = upload(w.ent_field, ent_field, nent); rc) return rc;
	if (int rc = upload(w.ent_tf, ent_tf, nent); rc) return rc;
	if (int rc = upload(w.ent_first_pos, ent_first_pos, nent); rc) return rc;
	{   // range index over the (ascending) document ids: range k starts at the first posting with doc >= k * kFtRangeDocs; the last entry is n
		RX_CHECK(n < 0xFFFFFFFFull, RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: posting list too long");
		const uint32_t n_ranges = uint32_t(doc[n - 1] / rxgpu::kFtRangeDocs) + 2;
		std::vector<uint32_t> ro(n_ranges);
		uint64_t i = 0;
		for (uint32_t k = 0; k < n_ranges; ++k) {
			const uint64_t first_doc = uint64_t(k) * rxgpu::kFtRangeDocs;
			while (i < n && doc[i] < first_doc) {
				RX_CHECK(i == 0 || doc[i] > doc[i - 1], RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: document ids must ascend strictly");
				++i;
			}
			ro[k] = uint32_t(i);
		}
		for (; i < n; ++i) RX_CHECK(i == 0 || doc[i] > doc[i - 1], RXGPU_ERR_PARAMS, "rxgpu_ft_set_word: document ids must ascend strictly");
		if (int rc = upload(w.range_off, ro.data(), ro.size()); rc) return rc;
		w.n_ranges = n_ranges;
	}
	w.n = n;
	w.nent = nent;
	w.last_doc = doc[n - 1];
	return RXGPU_OK;
}

int rxgpu_ft_set_word_positions(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* pos_off, const uint64_t* fpos) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null ft index");
	RX_CHECK(n == 0 || (doc && pos_off && fpos), RXGPU_ERR_PARAMS, "rxgpu_ft_set_word_positions: null argument");
	if (h->shard_set) return ft_shards_set_word(h, word_id, n, doc, nullptr, nullptr, nullptr, nullptr, pos_off, fpos);
	// derive the (field, tf, first position) entries calcTermRankImpl groups out of IdRelType::Pos() (phrasemergerimpl.h:24-49)
	std::vector<uint32_t> ent_off(n + 1, 0), ent_tf, ent_first;
	std::vector<uint8_t> ent_field;
	for (uint64_t i = 0; i < n; ++i) {
		ent_off[i] = uint32_t(ent_field.size());
		RX_CHECK(pos_off[i + 1] > pos_off[i], RXGPU_ERR_PARAMS, "rxgpu_ft_set_word_positions: a posting without positions");
		for (uint32_t a = pos_off[i]; a < pos_off[i + 1];) {
			const uint32_t f = uint32_t(fpos[a] >> 56);
			RX_CHECK(f < h->num_fields, RXGPU_ERR_PARAMS, "rxgpu_ft_set_word_positions: field out of range");
			uint32_t b = a + 1;
			while (b < pos_off[i + 1] && uint32_t(fpos[b] >> 56) == f) ++b;
			ent_field.push_back(uint8_t(f));
			ent_tf.push_back(b - a);
			ent_first.push_back(uint32_t(fpos[a] & ((1u << 28) - 1)));
			a = b;
		}
	}
	ent_off[n] = uint32_t(ent_field.size());
	if (int rc = rxgpu_ft_set_word(h, word_id, n, doc, ent_off.data(), ent_field.data(), ent_tf.data(), ent_first.data()); rc) return rc;
	if (n == 0) return RXGPU_OK;
	std::lock_guard<std::mutex> lk(h->mtx);
	std::unique_lock<std::shared_mutex> dict_lk(h->dict_mtx);
	rxgpu::DeviceGuard dg(h->device);
	rxgpu_ft_word& w = h->words[word_id];
	if (int rc = upload(w.pos_off, pos_off, n + 1); rc) return rc;
	if (int rc = upload(w.fpos, fpos, size_t(pos_off[n])); rc) return rc;
	return RXGPU_OK;
}

int rxgpu_ft_word_df(rxgpu_ft_index* h, uint32_t word_id, uint64_t* out_df) {
	RX_CHECK(h && out_df, RXGPU_ERR_PARAMS, "rxgpu_ft_word_df: null argument");
	*out_df = 0;
	rxgpu_ft_index* src = h;
	if (h->shard_set) {   // every shard keeps the word's entry with the whole list's length
		if (h->shard_set->shards.empty()) return RXGPU_OK;
		src = h->shard_set->shards[0];
	}
	std::shared_lock<std::shared_mutex> dict_lk(src->dict_mtx);
	const auto it = src->words.find(word_id);
	if (it != src->words.end()) *out_df = word_df(it->second);
	return RXGPU_OK;
}

int rxgpu_ft_get_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t* n, uint64_t* npos, uint64_t* nent, uint32_t* doc, uint32_t* pos_off, uint64_t* fpos,
					  uint32_t* ent_off, uint8_t* ent_field, uint32_t* ent_tf, uint32_t* ent_first_pos, uint32_t* n_ranges, uint32_t* range_off) {
	RX_CHECK(h && n && npos && nent && n_ranges, RXGPU_ERR_PARAMS, "rxgpu_ft_get_word: null argument");
	std::lock_guard<std::mutex> lk(h->mtx);
	std::shared_lock<std::shared_mutex> dict_lk(h->dict_mtx);
	rxgpu::DeviceGuard dg(h->device);
	RX_HIP(hipStreamSynchronize(h->stream));
	const auto it = h->words.find(word_id);
	RX_CHECK(it != h->words.end(), RXGPU_ERR_PARAMS, "rxgpu_ft_get_word: unknown word");
	const rxgpu_ft_word& w = it->second;
	*n = w.n;
	*nent = w.nent;
	*n_ranges = w.n_ranges;
	*npos = 0;
	if (!w.n) return RXGPU_OK;
	if (w.pos_off) {
		uint32_t last = 0;
		RX_HIP(hipMemcpy(&last, w.pos_off + w.n, 4, hipMemcpyDeviceToHost));
		*npos = last;
	}
	auto down = [](void* dst, const void* src, size_t bytes) -> int {
		if (dst && src && bytes) RX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
		return RXGPU_OK;
	};
	if (int rc = down(doc, w.doc, w.n * 4); rc) return rc;
	if (int rc = down(pos_off, w.pos_off, (w.n + 1) * 4); rc) return rc;
	if (int rc = down(fpos, w.fpos, size_t(*npos) * 8); rc) return rc;
	if (int rc = down(ent_off, w.ent_off, (w.n + 1) * 4); rc) return rc;
	if (int rc = down(ent_field, w.ent_field, w.nent); rc) return rc;
	if (int rc = down(ent_tf, w.ent_tf, w.nent * 4); rc) return rc;
	if (int rc = down(ent_first_pos, w.ent_first_pos, w.nent * 4); rc) return rc;
	if (int rc = down(range_off, w.range_off, size_t(w.n_ranges) * 4); rc) return rc;
	return RXGPU_OK;
}

int rxgpu_ft_read_stats(rxgpu_ft_index* h, uint64_t* postings, double* kernel_ms) {
	RX_CHECK(h && postings && kernel_ms, RXGPU_ERR_PARAMS, "rxgpu_ft_read_stats: null argument");
	std::lock_guard<std::mutex> lk(h->mtx);
	{   // the lanes' merges count too
		std::vector<rxgpu_ft_index*> have;
		{
			std::lock_guard<std::mutex> g(h->lanes_mtx);
			for (auto& l : h->lanes) have.push_back(l.get());
		}
		for (rxgpu_ft_index* l : have) {
			std::lock_guard<std::mutex> ll(l->mtx);
			h->stat_postings += l->stat_postings;
			h->stat_ms += l->stat_ms;
			for (int k = 0; k < 6; ++k) h->trace_us[k] += l->trace_us[k];
			for (int k = 0; k < 64; ++k) h->stamps[k] += l->stamps[k];
			l->stat_postings = 0;
			l->stat_ms = 0.0;
			for (double& v : l->trace_us) v = 0;
			for (double& v : l->stamps) v = 0;
		}
	}
	*postings = h->stat_postings;
	*kernel_ms = h->stat_ms;
	if (const char* e = std::getenv("RXGPU_FT_TRACE"); e && e[0] == '1' && h->trace_us[5] > 0) {
		const double m = h->trace_us[5];
		std::fprintf(stderr, "[rxgpu ft trace] per merge (us): plan %.1f  stage+upload %.1f  launches %.1f  wait+download %.1f  unpack %.1f  (kernels %.1f)\n",
					 h->trace_us[0] / m, h->trace_us[1] / m, h->trace_us[2] / m, h->trace_us[3] / m, h->trace_us[4] / m, h->stat_ms * 1e3 / m);
		if (std::getenv("RXGPU_FT_STAMPS")) {
			auto line = [&](const char* name, int a, int b) {
				std::fprintf(stderr, "[rxgpu ft stamps] %-12s", name);
				for (int k = a; k < b; ++k) std::fprintf(stderr, " %d:%.1f", k, h->stamps[k] / m);
				std::fprintf(stderr, "\n");
			};
			line("ft_ranges", 0, 16);
			line("ft_rank_all", 16, 19);
			line("ft_adders", 24, 32);
			line("ft_finish", 32, 42);
			for (double& v : h->stamps) v = 0;
		}
		for (double& v : h->trace_us) v = 0;
	}
	h->stat_postings = 0;
	h->stat_ms = 0.0;
	return RXGPU_OK;
}

}  // extern "C"
