// Hybrid queries (rxgpu_hybrid_*): the fusion of a KNN list with the BM25 merge that rxgpu_ft_merge_*_resident left in HBM (hybrid_fuse.hip).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rxgpu_ft_internal.h"

using namespace rxgpu;   // the cross-unit types and functions: rxgpu_ft_internal.h

namespace {
int check_hybrid_params(const rxgpu_hybrid_params* p, const char* who) {
	RX_CHECK(p, RXGPU_ERR_PARAMS, std::string(who) + ": null parameters");
	RX_CHECK(p->kind == 0 || p->kind == 1, RXGPU_ERR_PARAMS, std::string(who) + ": kind must be 0 (RRF) or 1 (linear)");
	return RXGPU_OK;
}
void fill_reranker(rxgpu::HybridFuseArgs& a, const rxgpu_hybrid_params* p, int metric) {
	a.kind = p->kind;
	a.is_union = p->is_union ? 1 : 0;
	a.desc = p->desc ? 1 : 0;
	for (int i = 0; i < 5; ++i) a.params[i] = p->params[i];
	a.metric_l2 = metric == RXGPU_METRIC_L2 ? 1 : 0;
}
}  // namespace

namespace {
// the FT-side arguments of the two fusion kernels for the resident merge of `h` (M = its max_merged; 0: no resident merge)
int fuse_ft_args(rxgpu_ft_index* h, uint32_t M, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_row_of_doc,
				 rxgpu::HybridFuseArgs& a) {
	const size_t key_bytes = rxgpu::ft_align256(size_t(2) * std::max<uint32_t>(M, 1) * 4), cls_bytes = rxgpu::ft_align256(size_t(2) * std::max<uint32_t>(M, 1) * 2);
	if (int rc = h->d_fuse.ensure(key_bytes + cls_bytes + rxgpu::ft_align256(sizeof(rxgpu::HybridFuseState))); rc) return rc;
	char* ob = static_cast<char*>(h->d_out.ptr);
	if (M) {   // the packed layout run_merge gave d_out for max_merged = M
		const rxgpu::FtOutLayout ol = rxgpu::ft_out_layout(M);
		a.ft_count_ptr = reinterpret_cast<const uint32_t*>(ob + ol.header);
		a.ft_doc = reinterpret_cast<const uint32_t*>(ob + ol.doc);
		a.ft_proc = reinterpret_cast<const float*>(ob + ol.proc);
		if (h->res_has_syn) a.ft_terms = reinterpret_cast<const uint16_t*>(ob + ol.terms_counter);
	}
	a.ft_n = 0;
	a.ft_cap = M;
	a.min_rank = float(min_rank);
	a.row_of_doc = static_cast<const int32_t*>(d_row_of_doc);
	fill_reranker(a, params, metric);
	a.scratch_key = static_cast<uint32_t*>(h->d_fuse.ptr);
	a.scratch_cls = reinterpret_cast<uint16_t*>(static_cast<char*>(h->d_fuse.ptr) + key_bytes);
	a.state = reinterpret_cast<rxgpu::HybridFuseState*>(static_cast<char*>(h->d_fuse.ptr) + key_bytes + cls_bytes);
	return RXGPU_OK;
}
void prep_signature(int32_t min_rank, const rxgpu_hybrid_params* p, const void* d_row_of_doc, double sig[8]) {
	sig[0] = min_rank;
	sig[1] = p->kind * 4 + (p->desc ? 2 : 0);
	for (int i = 0; i < 5; ++i) sig[2 + i] = p->params[i];
	sig[7] = double(reinterpret_cast<uintptr_t>(d_row_of_doc));
}
int enqueue_prepare(rxgpu_ft_index* h, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_row_of_doc) {
	const uint32_t M = h->res_pending ? h->res_cap : 0;
	rxgpu::HybridFuseArgs a{};
	if (int rc = fuse_ft_args(h, M, min_rank, params, metric, d_row_of_doc, a); rc) return rc;
	if (!h->ev_pa) {
		RX_HIP(hipEventCreate(&h->ev_pa));
		RX_HIP(hipEventCreate(&h->ev_pb));
	}
	RX_HIP(hipEventRecord(h->ev_pa, h->stream));
	RX_HIP(rxgpu::launch_hybrid_prepare(a, h->stream));
	RX_HIP(hipEventRecord(h->ev_pb, h->stream));
	h->prep_timed = true;
	prep_signature(min_rank, params, d_row_of_doc, h->prep_sig);
	h->prep_done = true;
	return RXGPU_OK;
}
}  // namespace

extern "C" {

// The FT-only half of the fusion (postProcessResults, id order, class / group tables), enqueued behind the resident merge so that it
// runs while the KNN search is still streaming the corpus.  Optional: rxgpu_hybrid_fuse_resident enqueues it itself when it was not.
int rxgpu_hybrid_prepare_resident(rxgpu_ft_index* h, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_row_of_doc) {
	RX_CHECK(h, RXGPU_ERR_PARAMS, "rxgpu_hybrid_prepare_resident: null argument");
	if (int rc = check_hybrid_params(params, "rxgpu_hybrid_prepare_resident"); rc) return rc;
	std::unique_lock<std::mutex> lk(h->mtx);
	if (int rc = check_resident_session(h, lk, "rxgpu_hybrid_prepare_resident"); rc) return rc;
	rxgpu::DeviceGuard dg(h->device);
	return enqueue_prepare(h, min_rank, params, metric, d_row_of_doc);
}

int rxgpu_hybrid_fuse_resident(rxgpu_ft_index* h, int32_t min_rank, const rxgpu_hybrid_params* params, int metric, const void* d_knn_dist,
							   const void* d_knn_row, const void* d_knn_count, uint32_t knn_n, uint32_t k, void* knn_stream, const void* d_row_of_doc,
							   const void* d_rowid_of_row, int32_t* out_ids, float* out_ranks, uint64_t cap, uint64_t* out_n, uint32_t* out_flags) {
	RX_CHECK(h && out_n, RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse_resident: null argument");
	*out_n = 0;
	if (out_flags) *out_flags = 0;
	if (int rc = check_hybrid_params(params, "rxgpu_hybrid_fuse_resident"); rc) return rc;
	RX_CHECK(k <= uint32_t(rxgpu::kMaxFuseKnn) && k <= knn_n, RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse_resident: k must be <= 1024 and <= the entries of the KNN list");
	RX_CHECK(knn_n == 0 || (d_knn_dist && d_knn_row), RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse_resident: null KNN list");
	std::unique_lock<std::mutex> lk(h->mtx);
	if (int rc = check_resident_session(h, lk, "rxgpu_hybrid_fuse_resident"); rc) return rc;
	struct SessionEnd {   // whatever happens below, this thread's session ends with its fusion
		rxgpu_ft_index* h;
		~SessionEnd() { close_resident_session(h); }
	} session_end{h};
	rxgpu::DeviceGuard dg(h->device);
	const uint32_t M = h->res_pending ? h->res_cap : 0;   // no resident merge: an empty FT side (the merge found nothing to do)
	const size_t out_cap = size_t(M) + k;
	RX_CHECK(cap >= out_cap && (out_cap == 0 || (out_ids && out_ranks)), RXGPU_ERR_OVERFLOW, "rxgpu_hybrid_fuse_resident: output buffers too small");
	{   // the FT-only half, unless the caller had it enqueued already (for exactly these parameters)
		double sig[8];
		prep_signature(min_rank, params, d_row_of_doc, sig);
		if (!h->prep_done || std::memcmp(sig, h->prep_sig, sizeof(sig)) != 0) {
			if (int rc = enqueue_prepare(h, min_rank, params, metric, d_row_of_doc); rc) return rc;
		}
	}
	// the result leaves through the pinned staging buffer: the kernel's stores go straight to host memory, no copy-engine start-up
	const size_t o_ids = 256, o_ranks = o_ids + rxgpu::ft_align256(out_cap * 4), stage = o_ranks + rxgpu::ft_align256(out_cap * 4);
	if (int rc = h->ensure_pinned(stage); rc) return rc;
	char* hp = static_cast<char*>(h->h_pinned);
	void* hp_dev = nullptr;
	RX_HIP(hipHostGetDevicePointer(&hp_dev, hp, 0));
	char* hd = static_cast<char*>(hp_dev);
	hipStream_t st = h->stream;
	if (knn_stream) {   // the KNN search ran on the caller's stream: the join waits for it on the device, the host does not
		if (!h->ev_knn) RX_HIP(hipEventCreateWithFlags(&h->ev_knn, hipEventDisableTiming));
		RX_HIP(hipEventRecord(h->ev_knn, static_cast<hipStream_t>(knn_stream)));
		RX_HIP(hipStreamWaitEvent(st, h->ev_knn, 0));
	}
	rxgpu::HybridFuseArgs a{};
	if (int rc = fuse_ft_args(h, M, min_rank, params, metric, d_row_of_doc, a); rc) return rc;
	a.knn_dist = static_cast<const float*>(d_knn_dist);
	a.knn_row = static_cast<const uint32_t*>(d_knn_row);
	a.knn_count_ptr = static_cast<const uint32_t*>(d_knn_count);
	a.knn_n = knn_n;
	a.k = k;
	a.knn_negate = metric == RXGPU_METRIC_L2 ? 0 : 1;
	a.rowid_of_row = static_cast<const int32_t*>(d_rowid_of_row);
	a.out_header = reinterpret_cast<uint32_t*>(hd);
	a.out_ids = reinterpret_cast<int32_t*>(hd + o_ids);
	a.out_ranks = reinterpret_cast<float*>(hd + o_ranks);
	static const bool stamps = std::getenv("RXGPU_FUSE_STAMPS") != nullptr;
	if (stamps) a.dbg = reinterpret_cast<unsigned long long*>(hd + 64);   // inside the 256-byte header region of the staging buffer
	if (!h->ev_fa) {
		RX_HIP(hipEventCreate(&h->ev_fa));
		RX_HIP(hipEventCreate(&h->ev_fb));
	}
	RX_HIP(hipEventRecord(h->ev_fa, st));
	RX_HIP(rxgpu::launch_hybrid_join(a, st));
	RX_HIP(hipEventRecord(h->ev_fb, st));
	h->prep_done = false;
	if (int rc = wait_stream_polled(st); rc) return rc;
	// the merge in front of the fusion has ended too: settle its state without another wait
	if (h->res_pending) {
		h->res_pending = false;
		if (int rc = settle_resident_merge(h, "rxgpu_hybrid_fuse_resident"); rc) return rc;
	}
	{
		float fms = 0.f;
		if (hipEventElapsedTime(&fms, h->ev_fa, h->ev_fb) == hipSuccess) {
			h->fuse_ms += fms;
			h->fuse_calls += 1;
		}
		if (h->prep_timed && hipEventElapsedTime(&fms, h->ev_pa, h->ev_pb) == hipSuccess) h->prep_ms += fms;
		h->prep_timed = false;
	}
	if (stamps) {
		const unsigned long long* raw = reinterpret_cast<const unsigned long long*>(hp + 64);
		for (int k2 = 1; k2 < 8; ++k2) h->fuse_stamps[k2] += raw[k2] >= raw[0] ? double(raw[k2] - raw[0]) * 0.01 : 0.0;   // 100 MHz -> us
	}
	const uint32_t* hdr = reinterpret_cast<const uint32_t*>(hp);
	const uint64_t n = hdr[0];
	RX_CHECK(n <= out_cap, RXGPU_ERR_DEVICE, "rxgpu_hybrid_fuse_resident: corrupt result header");
	if (n) {
		std::memcpy(out_ids, hp + o_ids, n * 4);
		std::memcpy(out_ranks, hp + o_ranks, n * 4);
	}
	*out_n = n;
	if (out_flags) *out_flags = hdr[1];
	return RXGPU_OK;
}

int rxgpu_hybrid_read_stats(rxgpu_ft_index* h, uint64_t* calls, double* kernel_ms, double* prepare_ms) {
	RX_CHECK(h && calls && kernel_ms, RXGPU_ERR_PARAMS, "rxgpu_hybrid_read_stats: null argument");
	std::lock_guard<std::mutex> lk(h->mtx);
	*calls = h->fuse_calls;
	*kernel_ms = h->fuse_ms;
	if (prepare_ms) *prepare_ms = h->prep_ms;
	h->prep_ms = 0.0;
	if (std::getenv("RXGPU_FUSE_STAMPS") && h->fuse_calls) {
		std::fprintf(stderr, "[rxgpu fuse stamps] us since kernel start:");
		for (int k = 1; k < 8; ++k) {
			std::fprintf(stderr, " %d:%.1f", k, h->fuse_stamps[k] / double(h->fuse_calls));
			h->fuse_stamps[k] = 0;
		}
		std::fprintf(stderr, "\n");
	}
	h->fuse_calls = 0;
	h->fuse_ms = 0.0;
	return RXGPU_OK;
}

// The same kernel on host arrays (tests, callers whose two halves are already on the host): everything is staged, fused, brought back.
int rxgpu_hybrid_fuse(int device, const rxgpu_hybrid_params* params, int metric, const int32_t* knn_ids, const float* knn_ranks, uint32_t n_knn,
					  const int32_t* ft_ids, const uint8_t* ft_ranks, uint32_t n_ft, int32_t* out_ids, float* out_ranks, uint64_t cap, uint64_t* out_n) {
	RX_CHECK(out_n, RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse: null argument");
	*out_n = 0;
	if (int rc = check_hybrid_params(params, "rxgpu_hybrid_fuse"); rc) return rc;
	RX_CHECK(n_knn <= uint32_t(rxgpu::kMaxFuseKnn), RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse: at most 1024 KNN entries");
	RX_CHECK((n_knn == 0 || (knn_ids && knn_ranks)) && (n_ft == 0 || (ft_ids && ft_ranks)), RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse: null argument");
	RX_CHECK(cap >= uint64_t(n_knn) + n_ft && (cap == 0 || (out_ids && out_ranks)), RXGPU_ERR_OVERFLOW, "rxgpu_hybrid_fuse: output buffers too small");
	int ndev = 0;
	RX_HIP(hipGetDeviceCount(&ndev));
	RX_CHECK(device >= 0 && device < ndev, RXGPU_ERR_PARAMS, "rxgpu_hybrid_fuse: no such device");
	rxgpu::DeviceGuard dg(device);
	const size_t nf = std::max<uint32_t>(n_ft, 1), nk = std::max<uint32_t>(n_knn, 1), no = size_t(n_ft) + n_knn + 1;
	rxgpu::FtCarver cv;
	const size_t o_fid = cv.take(nf * 4), o_fr = cv.take(nf), o_kid = cv.take(nk * 4), o_kr = cv.take(nk * 4), o_key = cv.take(2 * nf * 4),
				 o_cls = cv.take(2 * nf * 2), o_hdr = cv.take(16), o_oid = cv.take(no * 4), o_or = cv.take(no * 4),
				 o_state = cv.take(sizeof(rxgpu::HybridFuseState));
	rxgpu_devbuf buf;
	if (int rc = buf.ensure(cv.off); rc) return rc;
	struct BufRelease {
		rxgpu_devbuf& b;
		~BufRelease() { b.release(); }
	} buf_release{buf};
	char* d = static_cast<char*>(buf.ptr);
	if (n_ft) {
		RX_HIP(hipMemcpy(d + o_fid, ft_ids, size_t(n_ft) * 4, hipMemcpyHostToDevice));
		RX_HIP(hipMemcpy(d + o_fr, ft_ranks, n_ft, hipMemcpyHostToDevice));
	}
	if (n_knn) {
		RX_HIP(hipMemcpy(d + o_kid, knn_ids, size_t(n_knn) * 4, hipMemcpyHostToDevice));
		RX_HIP(hipMemcpy(d + o_kr, knn_ranks, size_t(n_knn) * 4, hipMemcpyHostToDevice));
	}
	rxgpu::HybridFuseArgs a{};
	a.ft_doc = reinterpret_cast<const uint32_t*>(d + o_fid);
	a.ft_rank_u8 = reinterpret_cast<const uint8_t*>(d + o_fr);
	a.ft_n = n_ft;
	a.ft_cap = uint32_t(nf);
	a.knn_dist = reinterpret_cast<const float*>(d + o_kr);   // ranks as the planner holds them: no sign change
	a.knn_row = reinterpret_cast<const uint32_t*>(d + o_kid);
	a.knn_n = n_knn;
	a.k = n_knn;
	a.knn_negate = 0;
	fill_reranker(a, params, metric);
	a.out_header = reinterpret_cast<uint32_t*>(d + o_hdr);
	a.out_ids = reinterpret_cast<int32_t*>(d + o_oid);
	a.out_ranks = reinterpret_cast<float*>(d + o_or);
	a.scratch_key = reinterpret_cast<uint32_t*>(d + o_key);
	a.scratch_cls = reinterpret_cast<uint16_t*>(d + o_cls);
	a.state = reinterpret_cast<rxgpu::HybridFuseState*>(d + o_state);
	RX_HIP(rxgpu::launch_hybrid_prepare(a, nullptr));
	RX_HIP(rxgpu::launch_hybrid_join(a, nullptr));
	RX_HIP(hipStreamSynchronize(nullptr));   // (the two launches above; not a device-wide wait — resident search kernels may be alive)
	uint32_t hdr[4];
	RX_HIP(hipMemcpy(hdr, d + o_hdr, sizeof(hdr), hipMemcpyDeviceToHost));
	const uint64_t n = hdr[0];
	RX_CHECK(n <= uint64_t(n_knn) + n_ft, RXGPU_ERR_DEVICE, "rxgpu_hybrid_fuse: corrupt result header");
	if (n) {
		RX_HIP(hipMemcpy(out_ids, d + o_oid, n * 4, hipMemcpyDeviceToHost));
		RX_HIP(hipMemcpy(out_ranks, d + o_or, n * 4, hipMemcpyDeviceToHost));
	}
	*out_n = n;
	return RXGPU_OK;
}

}  // extern "C"
