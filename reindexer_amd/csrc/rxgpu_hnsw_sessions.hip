// C-ABI implementation (include/rxgpu.h), the HNSW host side: SearchRange (an ef-search through hnsw_search_impl, then the expansion on the
// device) and the streaming KNN sessions.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cstdlib>
#include <functional>
#include <string>

#include "../../include/rxgpu.h"
#include "hnsw_stream_collect_plan.h"
#include "rxgpu_hnsw_internal.h"

using rxgpu::acquire_ctx;
using rxgpu::CtxLease;
using rxgpu::DeviceGuard;
using rxgpu::fill_hnsw_params;
using rxgpu::fill_sq8_params;
using rxgpu::ProfileScope;
using rxgpu::set_error;

// A streaming KNN session (rxgpu_hnsw_stream_begin)
struct rxgpu_hnsw_stream {
	rxgpu_index* owner = nullptr;
	uint64_t graph_n = 0;
	uint32_t ef = 0;
	hipStream_t stream = nullptr;
	rxgpu_devbuf d_query, d_visited, d_cand, d_top, d_ext, d_state, d_out;
	rxgpu_devbuf d_allowed, d_collect;   // rxgpu_hnsw_stream_collect: the call's bitmap; its accepted rows and per-call records
	uint32_t out_cap = 0;
	rxgpu::HnswStreamState host_state{};
	bool empty_graph = false;
	bool sq8 = false;          // the session runs over the SQ8 codes: d_query holds the query's codes
	float qcorr = 0.f, qnorm = 1.f;
};

namespace {

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
	rxgpu::HnswRequest seed;
	seed.queries = query, seed.qcorr = qcorr, seed.qnorm = qnorm, seed.nq = 1, seed.k = kk, seed.ef = ef_eff;
	seed.out_dist = sd.data(), seed.out_row = sr.data(), seed.out_count = &sc;
	if (int rc = rxgpu::hnsw_search_impl(h, seed); rc) return rc;
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

// ---------------------------------------------------------------------------------------------- a collection under an allowed-rows bitmap
struct CollectOut {   // where a collection's results go (the C-ABI's output arguments)
	float* dist;
	uint32_t* row;
	uint32_t* pos;   // may be null
	uint64_t cap;
	uint32_t *call_batch, *call_emitted, *call_end;
	uint32_t calls_cap;
	uint32_t* calls;
	uint64_t *presented, *accepted;
	int32_t* exhausted;
	uint32_t* launches;   // may be null
};
struct CollectRun {   // what a collection runs on: a session's own buffers, or a leased context's
	rxgpu_index* h;
	uint64_t graph_n;
	bool empty_graph, sq8;
	uint32_t ef;
	hipStream_t stream;
	rxgpu::HnswStreamState* host_state;
	rxgpu_devbuf *d_allowed, *d_collect;
	int mode;                                                  // kCollectFresh: a begun session; kCollectBegin: the descent first, in the same launch
	std::function<int(rxgpu::HnswStream&, uint32_t)> fill;     // the device view of the heaps, with an emit scratch of so many rows
	std::function<int()> before_launch;                        // optional: uploads and memsets of the one-shot call
};

int collect_impl(CollectRun& r, const uint32_t* allowed_words, uint64_t n_words, uint32_t needed, uint32_t first_batch, uint32_t max_calls, const CollectOut& o,
				 const char* who) {
	RX_CHECK(o.calls && o.presented && o.accepted && o.exhausted, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	*o.calls = 0;
	*o.presented = 0;
	*o.accepted = 0;
	*o.exhausted = 0;
	if (o.launches) *o.launches = 0;
	if (needed == 0 || first_batch == 0) return RXGPU_OK;
	if (r.empty_graph) {
		*o.exhausted = 1;
		return RXGPU_OK;
	}
	if (max_calls == 0) max_calls = rxgpu::kCollectMaxCalls;
	rxgpu_index* h = r.h;
	RX_CHECK(h->graph_attached && h->graph_n == r.graph_n && h->count == r.graph_n, RXGPU_ERR_LOGIC, std::string(who) + ": the graph changed under the session");
	const uint64_t words = (r.graph_n + 31) / 32;
	RX_CHECK(!allowed_words || n_words >= words, RXGPU_ERR_PARAMS, std::string(who) + ": the bitmap is shorter than the graph");
	const uint64_t out_bound = rxgpu::collect_out_bound(r.graph_n, needed, first_batch);
	const uint64_t calls_bound = rxgpu::collect_calls_bound(r.graph_n, needed, first_batch, max_calls);
	RX_CHECK(o.cap >= out_bound && o.dist && o.row, RXGPU_ERR_PARAMS, std::string(who) + ": the output holds fewer rows than a collection can deliver");
	RX_CHECK(o.calls_cap >= calls_bound && o.call_batch && o.call_emitted && o.call_end, RXGPU_ERR_PARAMS,
			 std::string(who) + ": the per-call records hold fewer calls than a collection can make");
	DeviceGuard dg(h->device);
	const uint32_t out_need = uint32_t(std::min<uint64_t>(rxgpu::collect_max_batch(first_batch), r.graph_n));
	rxgpu::HnswStream d{};
	if (int rc = r.fill(d, out_need); rc) return rc;
	const size_t o_dist = 0, o_row = size_t(out_bound) * 4, o_pos = size_t(out_bound) * 8, o_calls = size_t(out_bound) * 12;
	if (int rc = r.d_collect->ensure(o_calls + size_t(calls_bound) * 12); rc) return rc;
	if (allowed_words) {   // uploaded once per call
		if (int rc = r.d_allowed->ensure(words * 4); rc) return rc;
		RX_HIP(hipMemcpyAsync(r.d_allowed->ptr, allowed_words, words * 4, hipMemcpyHostToDevice, r.stream));
	}
	if (r.before_launch) {
		if (int rc = r.before_launch(); rc) return rc;
	}
	rxgpu::HnswParams p{};
	fill_hnsw_params(h, p);
	if (r.sq8) fill_sq8_params(h, p);
	char* cb = static_cast<char*>(r.d_collect->ptr);
	rxgpu::HnswStreamCollect c{};
	c.allowed = allowed_words ? static_cast<const uint32_t*>(r.d_allowed->ptr) : nullptr;
	c.needed = needed, c.first_batch = first_batch, c.max_calls = max_calls;
	c.out_dist = reinterpret_cast<float*>(cb + o_dist);
	c.out_row = reinterpret_cast<uint32_t*>(cb + o_row);
	c.out_pos = reinterpret_cast<uint32_t*>(cb + o_pos);
	c.cap = uint32_t(out_bound);
	c.call_batch = reinterpret_cast<uint32_t*>(cb + o_calls);
	c.call_emitted = c.call_batch + calls_bound;
	c.call_end = c.call_emitted + calls_bound;
	c.calls_cap = uint32_t(calls_bound);
	rxgpu::HnswStreamState& hs = *r.host_state;
	// LDS form: the largest ef and the largest batch of the collection fit top_candidates' area, and the heaps fit now (a session that begins
	// in this launch holds its entry point only)
	const bool fresh = r.mode == rxgpu::kCollectBegin;
	const uint32_t top_n = fresh ? 0u : uint32_t(hs.top_n), ext_n = fresh ? 0u : uint32_t(hs.ext_n), cand_n = fresh ? 1u : uint32_t(hs.cand_n);
	bool lds = std::max<uint64_t>(r.ef, rxgpu::collect_max_batch(first_batch)) <= uint64_t(rxgpu::kStreamLdsTop) && top_n <= uint32_t(rxgpu::kStreamLdsTop) &&
			   ext_n <= uint32_t(rxgpu::kStreamLdsExt) && cand_n + h->graph_maxM0 <= uint32_t(rxgpu::kStreamLdsCand);
	if (getenv("RXGPU_HNSW_STREAM_GLOBAL")) lds = false;   // test hook: the whole collection with the heaps in HBM
	int mode = r.mode;
	uint32_t launches = 0;
	for (int attempt = 0; attempt < 2; ++attempt) {
		ProfileScope ps(h, lds ? "hnsw_stream_collect" : "hnsw_stream_collect_global", r.stream);
		rxgpu::launch_hnsw_stream_collect(h->metric, p, d, c, mode, lds, r.stream);
		RX_HIP(hipGetLastError());
		++launches;
		RX_HIP(hipMemcpyAsync(&hs, d.state, sizeof(hs), hipMemcpyDeviceToHost, r.stream));
		RX_HIP(hipStreamSynchronize(r.stream));
		if (hs.status != rxgpu::kStreamNeedGlobal) break;
		RX_CHECK(lds, RXGPU_ERR_DEVICE, std::string(who) + ": global-heap pass asked for more room");
		lds = false;   // outgrew LDS at a step boundary: the same collection, heaps in HBM, from the call it stopped in
		mode = rxgpu::kCollectResume;
	}
	if (o.launches) *o.launches = launches;
	RX_CHECK(hs.status == rxgpu::kStreamOk, RXGPU_ERR_DEVICE, std::string(who) + ": device-side session error");
	const uint32_t calls = hs.calls, accepted = hs.accepted;
	RX_CHECK(calls <= calls_bound && accepted <= out_bound, RXGPU_ERR_DEVICE, std::string(who) + ": the collection left its bounds");
	if (calls) {
		RX_HIP(hipMemcpyAsync(o.call_batch, c.call_batch, size_t(calls) * 4, hipMemcpyDeviceToHost, r.stream));
		RX_HIP(hipMemcpyAsync(o.call_emitted, c.call_emitted, size_t(calls) * 4, hipMemcpyDeviceToHost, r.stream));
		RX_HIP(hipMemcpyAsync(o.call_end, c.call_end, size_t(calls) * 4, hipMemcpyDeviceToHost, r.stream));
	}
	if (accepted) {
		RX_HIP(hipMemcpyAsync(o.dist, c.out_dist, size_t(accepted) * 4, hipMemcpyDeviceToHost, r.stream));
		RX_HIP(hipMemcpyAsync(o.row, c.out_row, size_t(accepted) * 4, hipMemcpyDeviceToHost, r.stream));
		if (o.pos) RX_HIP(hipMemcpyAsync(o.pos, c.out_pos, size_t(accepted) * 4, hipMemcpyDeviceToHost, r.stream));
	}
	RX_HIP(hipStreamSynchronize(r.stream));
	*o.calls = calls;
	*o.presented = hs.presented;
	*o.accepted = accepted;
	*o.exhausted = hs.exhausted ? 1 : 0;
	return RXGPU_OK;
}

// BeginStreamingSearch + the collection for one query on a leased search context: the heaps (40 bytes a node), the visited set, the bitmap and
// the outputs live in context buffers that grow once and are reused, so a call in steady state allocates nothing; the descent and the
// collection are one launch, a handover to the global heaps is the second.
int collect_knn_impl(rxgpu_index* h, const void* query, bool sq8, float qcorr, float qnorm, uint32_t ef, const uint32_t* allowed_words, uint64_t n_words,
					 uint32_t needed, uint32_t first_batch, uint32_t max_calls, const CollectOut& o, const char* who) {
	RX_CHECK(h && query, RXGPU_ERR_PARAMS, std::string(who) + ": null argument");
	RX_CHECK(!h->shard_set, RXGPU_ERR_LOGIC, std::string(who) + ": streaming sessions are per graph — not available on a sharded index");
	RX_CHECK(h->count == 0 || (h->graph_attached && h->graph_n == h->count), RXGPU_ERR_LOGIC, std::string(who) + ": graph is not attached / out of date");
	RX_CHECK(!sq8 || h->count == 0 || (h->d_codes && h->sq8_n == h->count), RXGPU_ERR_LOGIC, std::string(who) + ": SQ8 codes are not attached / out of date");
	DeviceGuard dg(h->device);
	rxgpu_search_ctx* c = acquire_ctx(h);
	if (!c) return RXGPU_ERR_DEVICE;
	CtxLease lease{h, c};
	const uint64_t n = h->count, words = (n + 31) / 32;
	rxgpu::HnswStreamState host_state{};
	CollectRun r{};
	r.h = h, r.graph_n = n, r.empty_graph = n == 0, r.sq8 = sq8, r.ef = ef ? ef : 100, r.stream = c->stream;   // kDefaultStreamingEf (hnswalg.h:1867)
	r.host_state = &host_state, r.d_allowed = &c->d_allowed, r.d_collect = &c->d_out_dist;
	r.mode = rxgpu::kCollectBegin;
	const size_t qbytes = size_t(h->dim) * (sq8 ? 1 : 4);
	size_t o_state = 0, o_scratch = 0;
	r.fill = [&](rxgpu::HnswStream& d, uint32_t out_need) -> int {
		o_state = (size_t(h->dim) * 4 + 255) & ~size_t(255);
		o_scratch = o_state + 256;
		if (int rc = c->d_misc.ensure(o_scratch + size_t(out_need) * 8); rc) return rc;
		if (int rc = c->d_visited.ensure(words * 4); rc) return rc;
		if (int rc = c->d_gcand_d.ensure(size_t(n) * 40); rc) return rc;
		char* mb = static_cast<char*>(c->d_misc.ptr);
		d.query = reinterpret_cast<const float*>(mb);
		d.qcodes = sq8 ? reinterpret_cast<const uint8_t*>(mb) : nullptr;
		d.qcorr = qcorr;
		d.qnorm = qnorm;
		d.visited = static_cast<uint32_t*>(c->d_visited.ptr);
		d.cand_d = static_cast<float*>(c->d_gcand_d.ptr);
		d.cand_i = reinterpret_cast<uint32_t*>(d.cand_d + n);
		d.top_d = d.cand_d + 2 * n;
		d.top_i = reinterpret_cast<uint32_t*>(d.top_d + 2 * n);
		d.ext_d = d.top_d + 4 * n;
		d.ext_i = reinterpret_cast<uint32_t*>(d.ext_d + 2 * n);
		d.cap = uint32_t(n);
		d.ef = r.ef;
		d.state = reinterpret_cast<rxgpu::HnswStreamState*>(mb + o_state);
		d.out_dist = reinterpret_cast<float*>(mb + o_scratch);
		d.out_row = reinterpret_cast<uint32_t*>(d.out_dist + out_need);
		return RXGPU_OK;
	};
	r.before_launch = [&]() -> int {
		RX_HIP(hipMemcpyAsync(c->d_misc.ptr, query, qbytes, hipMemcpyHostToDevice, c->stream));
		RX_HIP(hipMemsetAsync(c->d_visited.ptr, 0, words * 4, c->stream));
		return RXGPU_OK;
	};
	static_assert(sizeof(rxgpu::HnswStreamState) <= 256, "the state's slot in the context's scratch");
	return collect_impl(r, allowed_words, n_words, needed, first_batch, max_calls, o, who);
}

}  // namespace

extern "C" {

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
	for (rxgpu_devbuf* b : {&s->d_query, &s->d_visited, &s->d_cand, &s->d_top, &s->d_ext, &s->d_state, &s->d_out, &s->d_allowed, &s->d_collect}) b->release();
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

uint32_t rxgpu_hnsw_stream_collect_batch(uint64_t accepted, uint64_t presented, uint64_t needed) { return rxgpu::collect_batch(accepted, presented, needed); }

uint64_t rxgpu_hnsw_stream_collect_bound(uint64_t count, uint32_t needed, uint32_t first_batch) { return rxgpu::collect_out_bound(count, needed, first_batch); }

uint64_t rxgpu_hnsw_stream_collect_calls_bound(uint64_t count, uint32_t needed, uint32_t first_batch, uint32_t max_calls) {
	return rxgpu::collect_calls_bound(count, needed, first_batch, max_calls ? max_calls : rxgpu::kCollectMaxCalls);
}

// The loop of csrc/hnsw_stream_collect_plan.h over the session, on the device (hnsw_stream_collect.hip): one launch, or two when the
// session's heaps outgrow LDS on the way.
int rxgpu_hnsw_stream_collect(rxgpu_hnsw_stream* s, const uint32_t* allowed_words, uint64_t n_words, uint32_t needed, uint32_t first_batch, uint32_t max_calls,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint32_t* out_call_batch, uint32_t* out_call_emitted, uint32_t* out_call_end,
							  uint32_t calls_cap, uint32_t* out_calls, uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted,
							  uint32_t* out_launches, uint32_t* out_pos) {
	RX_CHECK(s, RXGPU_ERR_PARAMS, "rxgpu_hnsw_stream_collect: null argument");
	CollectOut o{out_dist, out_row, out_pos, cap, out_call_batch, out_call_emitted, out_call_end, calls_cap, out_calls, out_presented, out_accepted, out_exhausted,
				 out_launches};
	CollectRun r{};
	r.h = s->owner, r.graph_n = s->graph_n, r.empty_graph = s->empty_graph, r.sq8 = s->sq8, r.ef = s->ef, r.stream = s->stream;
	r.host_state = &s->host_state, r.d_allowed = &s->d_allowed, r.d_collect = &s->d_collect;
	r.mode = rxgpu::kCollectFresh;
	r.fill = [s](rxgpu::HnswStream& d, uint32_t out_need) -> int {
		if (out_need > s->out_cap) {   // a call delivers at most its batch, and never more than the graph holds: the global variant's emit scratch
			if (int rc = s->d_out.ensure(size_t(out_need) * 8); rc) return rc;
			s->out_cap = out_need;
		}
		fill_stream(s, d);
		return RXGPU_OK;
	};
	return collect_impl(r, allowed_words, n_words, needed, first_batch, max_calls, o, "rxgpu_hnsw_stream_collect");
}

/* Begin + collect for one query on a leased search context: nothing is allocated in steady state, the descent and the collection are one launch */
int rxgpu_hnsw_collect_knn(rxgpu_index* h, const float* query, uint32_t ef, const uint32_t* allowed_words, uint64_t n_words, uint32_t needed, uint32_t first_batch,
						   uint32_t max_calls, float* out_dist, uint32_t* out_row, uint64_t cap, uint32_t* out_call_batch, uint32_t* out_call_emitted,
						   uint32_t* out_call_end, uint32_t calls_cap, uint32_t* out_calls, uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted,
						   uint32_t* out_launches, uint32_t* out_pos) {
	CollectOut o{out_dist, out_row, out_pos, cap, out_call_batch, out_call_emitted, out_call_end, calls_cap, out_calls, out_presented, out_accepted, out_exhausted,
				 out_launches};
	return collect_knn_impl(h, query, false, 0.f, 1.f, ef, allowed_words, n_words, needed, first_batch, max_calls, o, "rxgpu_hnsw_collect_knn");
}

int rxgpu_hnsw_collect_knn_sq8(rxgpu_index* h, const uint8_t* query_codes, float query_corr, float query_norm_coef, uint32_t ef, const uint32_t* allowed_words,
							   uint64_t n_words, uint32_t needed, uint32_t first_batch, uint32_t max_calls, float* out_dist, uint32_t* out_row, uint64_t cap,
							   uint32_t* out_call_batch, uint32_t* out_call_emitted, uint32_t* out_call_end, uint32_t calls_cap, uint32_t* out_calls,
							   uint64_t* out_presented, uint64_t* out_accepted, int32_t* out_exhausted, uint32_t* out_launches, uint32_t* out_pos) {
	CollectOut o{out_dist, out_row, out_pos, cap, out_call_batch, out_call_emitted, out_call_end, calls_cap, out_calls, out_presented, out_accepted, out_exhausted,
				 out_launches};
	return collect_knn_impl(h, query_codes, true, query_corr, query_norm_coef, ef, allowed_words, n_words, needed, first_batch, max_calls, o,
							"rxgpu_hnsw_collect_knn_sq8");
}

}  // extern "C"
