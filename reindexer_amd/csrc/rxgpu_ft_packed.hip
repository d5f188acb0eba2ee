// Packed uploads (rxgpu_ft_set_words_packed*): posting lists as the reference stores them, decoded on the device (ft_packed.hip).  What the
// call decides from the streams' lengths is ft_packed_plan.h's; this unit executes it.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "rxgpu_ft_internal.h"
#include "ft_packed_plan.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

extern "C" {

int rxgpu_ft_set_words_packed(rxgpu_ft_index* h, uint32_t nwords, const uint32_t* word_ids, const uint64_t* byte_off, const uint8_t* bytes,
							  const uint64_t* array_found_pos) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null ft index");
	if (nwords == 0) return RXGPU_OK;
	RX_CHECK(word_ids && byte_off && array_found_pos, RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed: null argument");
	RX_CHECK(byte_off[0] == 0, RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed: byte_off[0] must be 0");
	for (uint32_t w = 0; w < nwords; ++w) RX_CHECK(byte_off[w + 1] >= byte_off[w], RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed: byte_off must not descend");
	RX_CHECK(byte_off[nwords] == 0 || bytes, RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed: null argument");
	std::vector<const uint8_t*> data(nwords);
	std::vector<uint64_t> len(nwords);
	for (uint32_t w = 0; w < nwords; ++w) {
		data[w] = bytes + byte_off[w];
		len[w] = byte_off[w + 1] - byte_off[w];
	}
	return rxgpu_ft_set_words_packed_ptrs(h, nwords, word_ids, data.data(), len.data(), array_found_pos);
}

// The same with every word's stream where the caller keeps it (PackedIdRelVec::RawData() of each dictionary entry — separate allocations):
// the streams are gathered ONCE, in launch order, straight into the pinned staging buffer, and travel in one asynchronous copy.
int rxgpu_ft_set_words_packed_ptrs(rxgpu_ft_index* h, uint32_t nwords, const uint32_t* word_ids, const uint8_t* const* data, const uint64_t* len,
								   const uint64_t* array_found_pos) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "null ft index");
	if (nwords == 0) return RXGPU_OK;
	RX_CHECK(word_ids && data && len && array_found_pos, RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed_ptrs: null argument");
	const auto t_call = std::chrono::steady_clock::now();
	struct WallClock {
		rxgpu_ft_index* h;
		std::chrono::steady_clock::time_point t0;
		~WallClock() { h->packed_wall_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
	};
	for (uint32_t w = 0; w < nwords; ++w) RX_CHECK(len[w] == 0 || data[w], RXGPU_ERR_PARAMS, "rxgpu_ft_set_words_packed_ptrs: null stream");
	std::lock_guard<std::mutex> lk(h->mtx);
	WallClock wall{h, t_call};
	std::unique_lock<std::shared_mutex> dict_lk(h->dict_mtx);   // no merge on any lane reads the dictionary meanwhile
	rxgpu::DeviceGuard dg(h->device);
	RX_HIP(hipStreamSynchronize(h->stream));

	// ---- 1. plan (ft_packed_plan.h): launch order, offsets, pieces, staging layout, chunks, gather threads
	// one wavefront per word (ft_packed_wave); RXGPU_FT_PACKED_THREAD=1: the one-thread-per-word kernels of round 2 (cross-check, comparison)
	const bool wave = std::getenv("RXGPU_FT_PACKED_THREAD") == nullptr;
	// The streams may travel in chunks of whole words (launch order: the longest words first) so that the gather of chunk c + 1, the copy of
	// chunk c and the counting pass over chunk c - 1 overlap.  Measured on the 100 000-word dictionary of tools/bench_ft_packed.py: 49.8 ms
	// per call with 8 MB chunks against 34.6 ms in one piece (profiles/rd4k_ft_packed_chunked.json, rd4h_ft_packed.json) — a chunk's
	// counting pass lasts as long as its longest stream, and the longest streams are what travels first.  One piece is the default;
	// RXGPU_FT_PACKED_CHUNK_MB=<n> cuts.
	uint64_t chunk_target = ~0ull;
	if (const char* e = std::getenv("RXGPU_FT_PACKED_CHUNK_MB")) {
		if (std::atol(e) > 0) chunk_target = uint64_t(std::atol(e)) << 20;
	}
	rxgpu::FtPackedPlan pl;
	if (rxgpu::FtPlanError e = rxgpu::ft_packed_plan(nwords, len, array_found_pos, wave, chunk_target, pl); e) {
		set_error(e.msg);
		return e.code;
	}
	const std::vector<uint32_t>& order = pl.order;
	const uint32_t nchunks = pl.nchunks();
	const unsigned nthr = pl.nthr;

	// ---- 2. stage: scratch of the call (streams, offsets, counts, pieces, slices) lives in buffers the index keeps and grows — no hipMalloc /
	// hipFree pair, each a device synchronisation, per call.  Everything but the streams travels first (one copy).
	if (int rc = h->d_pk_in.ensure(pl.in_bytes); rc) return rc;
	if (int rc = h->ensure_pinned(pl.in_bytes); rc) return rc;
	uint8_t* hp = static_cast<uint8_t*>(h->h_pinned);
	std::memcpy(hp + pl.o_off, pl.off.data(), size_t(nwords) * 16);
	std::memcpy(hp + pl.o_afp, pl.afp.data(), size_t(nwords) * 8);
	if (wave) {
		pl.fill_seg_word(reinterpret_cast<uint32_t*>(hp + pl.o_sw));
		std::memcpy(hp + pl.o_sf, pl.seg_first.data(), (size_t(nwords) + 1) * 4);
	}
	uint8_t* d_bytes = static_cast<uint8_t*>(h->d_pk_in.ptr);
	uint64_t* d_off = reinterpret_cast<uint64_t*>(d_bytes + pl.o_off);
	uint64_t* d_afp = reinterpret_cast<uint64_t*>(d_bytes + pl.o_afp);
	RX_HIP(hipMemcpyAsync(d_bytes + pl.o_off, hp + pl.o_off, pl.in_bytes - pl.o_off, hipMemcpyHostToDevice, h->stream));
	if (int rc = h->d_pk_cnt.ensure(size_t(nwords) * sizeof(rxgpu::FtPackedCounts)); rc) return rc;
	rxgpu::FtPackedCounts* d_counts = static_cast<rxgpu::FtPackedCounts*>(h->d_pk_cnt.ptr);
	rxgpu::FtPackedSegs segs{};
	if (wave) {
		if (int rc = h->d_pk_segs.ensure(size_t(pl.nsegs) * sizeof(rxgpu::FtPackedCheckpoint)); rc) return rc;
		RX_HIP(hipMemsetAsync(h->d_pk_segs.ptr, 0xFF, size_t(pl.nsegs) * sizeof(rxgpu::FtPackedCheckpoint), h->stream));
		segs.seg_word = reinterpret_cast<const uint32_t*>(d_bytes + pl.o_sw);
		segs.seg_first = reinterpret_cast<const uint32_t*>(d_bytes + pl.o_sf);
		segs.cps = static_cast<rxgpu::FtPackedCheckpoint*>(h->d_pk_segs.ptr);
		segs.nsegs = pl.nsegs;
	}

	// ---- 3. gather and count per chunk: the gather threads move the streams chunk by chunk; the calling thread sends a chunk on its way as
	// soon as every worker is through with it
	std::vector<std::atomic<uint32_t>> chunk_done(nchunks);
	for (auto& c : chunk_done) c.store(0, std::memory_order_relaxed);
	auto gather = [&](unsigned t) {
		for (uint32_t c = 0; c < nchunks; ++c) {
			uint32_t k, e;
			for (pl.gather_range(c, t, k, e); k < e; ++k) {
				const uint64_t n = pl.len_of(k);
				if (n) std::memcpy(hp + pl.off[2 * size_t(k)], data[order[k]], size_t(n));
			}
			chunk_done[c].fetch_add(1, std::memory_order_release);
		}
	};
	std::memset(hp + pl.total_bytes, 0, 16);
	std::vector<std::thread> gatherers;
	struct Joiner {
		std::vector<std::thread>& threads;
		~Joiner() {
			for (std::thread& t : threads) t.join();
		}
	} joiner{gatherers};
	if (nthr > 1) {
		for (unsigned t = 0; t < nthr; ++t) gatherers.emplace_back(gather, t);
	}
	// The counting pass of a chunk needs only that chunk's bytes, and lasts as long as the chunk's longest stream (a serial walk): on ONE
	// stream the chunks' kernels ran one behind the other and the pass took 34 ms instead of 6.  They run on four streams, each behind
	// its chunk's copy, and overlap like the wavefronts of a single launch do.
	for (hipStream_t& ps : h->pk_streams) {
		if (!ps) RX_HIP(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
	}
	EventPair ev_count, ev_write;
	if (int rc = ev_count.create(); rc) return rc;
	if (int rc = ev_write.create(); rc) return rc;
	struct EventList {
		std::vector<hipEvent_t> v;
		~EventList() {
			for (hipEvent_t e : v) (void)hipEventDestroy(e);
		}
		int add(hipEvent_t* out) {
			hipEvent_t e = nullptr;
			RX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
			v.push_back(e);
			*out = e;
			return RXGPU_OK;
		}
	} chunk_events;
	std::vector<hipEvent_t> counted(nchunks, nullptr);
	RX_HIP(hipEventRecord(ev_count.a, h->stream));   // (behind the setup copies: the pass is timed from here to its last kernel, uploads included)
	for (uint32_t c = 0; c < nchunks; ++c) {
		if (nthr > 1) {
			while (chunk_done[c].load(std::memory_order_acquire) < nthr) std::this_thread::yield();
		} else if (c == 0) {
			gather(0);   // small calls: everything at once on this thread
		}
		const uint32_t k0 = pl.chunk_first[c], k1 = pl.chunk_first[c + 1];
		const uint64_t b0 = pl.off[2 * size_t(k0)], b1 = pl.off[2 * size_t(k1 - 1) + 1] + (c + 1 == nchunks ? 16 : 0);
		if (b1 > b0) RX_HIP(hipMemcpyAsync(d_bytes + b0, hp + b0, size_t(b1 - b0), hipMemcpyHostToDevice, h->stream));
		hipEvent_t landed = nullptr;
		if (int rc = chunk_events.add(&landed); rc) return rc;
		RX_HIP(hipEventRecord(landed, h->stream));
		hipStream_t ks = h->pk_streams[c % 4];
		RX_HIP(hipStreamWaitEvent(ks, landed, 0));
		if (wave) {
			RX_HIP(rxgpu::launch_ft_packed_count(d_bytes, d_off, d_afp, nwords, h->num_fields, d_counts, &segs, ks, k0, k1 - k0));
		} else if (c + 1 == nchunks) {   // the thread-per-word kernels: one launch over all words
			RX_HIP(rxgpu::launch_ft_packed_count(d_bytes, d_off, d_afp, nwords, h->num_fields, d_counts, nullptr, ks, 0, nwords));
		}
		if (int rc = chunk_events.add(&counted[c]); rc) return rc;
		RX_HIP(hipEventRecord(counted[c], ks));
	}
	for (uint32_t c = 0; c < nchunks; ++c) RX_HIP(hipStreamWaitEvent(h->stream, counted[c], 0));
	RX_HIP(hipEventRecord(ev_count.b, h->stream));
	std::vector<rxgpu::FtPackedCounts> counts(nwords);
	RX_HIP(hipMemcpyAsync(counts.data(), d_counts, size_t(nwords) * sizeof(rxgpu::FtPackedCounts), hipMemcpyDeviceToHost, h->stream));
	RX_HIP(hipStreamSynchronize(h->stream));

	// ---- 4. check counts
	auto status_text = [](uint32_t st) {
		switch (st) {
			case rxgpu::kFtPackedTruncated: return "truncated varint stream";
			case rxgpu::kFtPackedDocOrder: return "document ids must ascend strictly";
			case rxgpu::kFtPackedField: return "field out of range";
			default: return "posting list too long";
		}
	};
	for (uint32_t k = 0; k < nwords; ++k) {
		RX_CHECK(counts[k].status == rxgpu::kFtPackedOk, RXGPU_ERR_PARAMS,
				 std::string("rxgpu_ft_set_words_packed: word ") + std::to_string(word_ids[order[k]]) + ": " + status_text(counts[k].status));
	}

	// ---- 5. carve pool: one allocation for the whole batch (ft_packed_plan.h lays it out)
	std::vector<rxgpu::FtPackedSlices> sl;
	const size_t pool_bytes = rxgpu::ft_packed_pool(counts.data(), nwords, sl);
	std::vector<rxgpu::FtPackedOut> outs(nwords);
	std::shared_ptr<void> pool;
	char* base = nullptr;
	if (pool_bytes) {
		void* raw = nullptr;
		RX_HIP(hipMalloc(&raw, pool_bytes));
		const int device = h->device;
		pool = std::shared_ptr<void>(raw, [device](void* q) {
			rxgpu::DeviceGuard g(device);
			(void)hipFree(q);
		});
		base = static_cast<char*>(raw);
	}
	for (uint32_t k = 0; k < nwords; ++k) {
		if (!counts[k].n) continue;
		outs[k].doc = reinterpret_cast<uint32_t*>(base + sl[k].doc);
		outs[k].pos_off = reinterpret_cast<uint32_t*>(base + sl[k].pos_off);
		outs[k].fpos = reinterpret_cast<uint64_t*>(base + sl[k].fpos);
		outs[k].ent_off = reinterpret_cast<uint32_t*>(base + sl[k].ent_off);
		outs[k].ent_field = reinterpret_cast<uint8_t*>(base + sl[k].ent_field);
		outs[k].ent_tf = reinterpret_cast<uint32_t*>(base + sl[k].ent_tf);
		outs[k].ent_first_pos = reinterpret_cast<uint32_t*>(base + sl[k].ent_first);
		outs[k].range_off = reinterpret_cast<uint32_t*>(base + sl[k].range_off);
		outs[k].n_ranges = sl[k].n_ranges;
	}

	// ---- 6. write
	if (int rc = h->d_pk_outs.ensure(size_t(nwords) * sizeof(rxgpu::FtPackedOut)); rc) return rc;
	RX_HIP(hipMemcpyAsync(h->d_pk_outs.ptr, outs.data(), size_t(nwords) * sizeof(rxgpu::FtPackedOut), hipMemcpyHostToDevice, h->stream));
	RX_HIP(hipEventRecord(ev_write.a, h->stream));
	RX_HIP(rxgpu::launch_ft_packed_write(d_bytes, d_off, d_afp, nwords, h->num_fields, static_cast<const rxgpu::FtPackedOut*>(h->d_pk_outs.ptr), d_counts, wave ? &segs : nullptr, h->stream));
	RX_HIP(hipEventRecord(ev_write.b, h->stream));
	std::vector<rxgpu::FtPackedCounts> again(nwords);
	RX_HIP(hipMemcpyAsync(again.data(), d_counts, size_t(nwords) * sizeof(rxgpu::FtPackedCounts), hipMemcpyDeviceToHost, h->stream));

	// ---- 7. adopt into the dictionary while the write pass runs (100 000 map insertions are a fifth of this call); should the pass disagree
	// with the counting pass below — an internal error — the words of the call are left empty
	h->words.reserve(h->words.size() + nwords);
	for (uint32_t k = 0; k < nwords; ++k) {
		rxgpu_ft_word& w = h->words[word_ids[order[k]]];
		w.release();
		const rxgpu::FtPackedCounts& c = counts[k];
		if (!c.n) continue;
		w.n = c.n;
		w.nent = c.nent;
		w.last_doc = c.last_doc;
		w.doc = outs[k].doc;
		w.ent_off = outs[k].ent_off;
		w.ent_field = outs[k].ent_field;
		w.ent_tf = outs[k].ent_tf;
		w.ent_first_pos = outs[k].ent_first_pos;
		w.pos_off = outs[k].pos_off;
		w.fpos = outs[k].fpos;
		w.range_off = outs[k].range_off;
		w.n_ranges = outs[k].n_ranges;
		w.pool = pool;
	}

	// ---- 8. verify and account
	const hipError_t waited = hipStreamSynchronize(h->stream);
	bool agree = waited == hipSuccess;
	for (uint32_t k = 0; k < nwords && agree; ++k) {
		agree = again[k].status == rxgpu::kFtPackedOk && again[k].n == counts[k].n && again[k].npos == counts[k].npos && again[k].nent == counts[k].nent;
	}
	if (!agree) {
		for (uint32_t k = 0; k < nwords; ++k) h->words[word_ids[order[k]]].release();
		RX_HIP(waited);
		RX_CHECK(false, RXGPU_ERR_DEVICE, "rxgpu_ft_set_words_packed: the write pass disagrees with the counting pass");
	}
	h->packed_count_ms += ev_count.elapsed_ms();
	h->packed_write_ms += ev_write.elapsed_ms();
	h->packed_bytes_in += pl.total_bytes;
	h->packed_bytes_out += pool_bytes;
	return RXGPU_OK;
}

int rxgpu_ft_read_packed_stats(rxgpu_ft_index* h, double* count_ms, double* write_ms, uint64_t* bytes_in, uint64_t* bytes_out) {
	RX_CHECK(h && count_ms && write_ms && bytes_in && bytes_out, RXGPU_ERR_PARAMS, "rxgpu_ft_read_packed_stats: null argument");
	std::lock_guard<std::mutex> lk(h->mtx);
	*count_ms = h->packed_count_ms;
	*write_ms = h->packed_write_ms;
	*bytes_in = h->packed_bytes_in;
	*bytes_out = h->packed_bytes_out;
	h->packed_count_ms = h->packed_write_ms = 0.0;
	h->packed_bytes_in = h->packed_bytes_out = 0;
	return RXGPU_OK;
}

int rxgpu_ft_read_packed_wall(rxgpu_ft_index* h, double* wall_ms) {
	RX_CHECK(h && wall_ms, RXGPU_ERR_PARAMS, "rxgpu_ft_read_packed_wall: null argument");
	std::lock_guard<std::mutex> lk(h->mtx);
	*wall_ms = h->packed_wall_ms;
	h->packed_wall_ms = 0.0;
	return RXGPU_OK;
}

}  // extern "C"
