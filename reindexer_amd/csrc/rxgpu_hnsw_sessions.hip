// C-ABI implementation (include/rxgpu.h), the HNSW host side: SearchRange (an ef-search through hnsw_search_impl, then the expansion on the
// device) and the streaming KNN sessions.  Host-side plumbing only — all arithmetic is in the kernels.
#include <algorithm>
#include <cstdlib>

#include "../../include/rxgpu.h"
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
	for (rxgpu_devbuf* b : {&s->d_query, &s->d_visited, &s->d_cand, &s->d_top, &s->d_ext, &s->d_state, &s->d_out}) b->release();
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

}  // extern "C"
