// Row-range sharding of one float_vector index over several GPUs of THIS process (BASELINE configs[3] behind the C++ seam: the Map owns a
// device list).  Every shard is an ordinary rxgpu_index on its own device; a search fans the query out, every shard runs the kernels of
// rxgpu_search_* on its rows, and the per-shard answers (kk x 8 B per query) are merged under the reference's order — (dist, GLOBAL row),
// global row = shard * shard_rows + local row, which is the scan order of BruteforceSearch::SearchKnn (bruteforce.cc:103-127) because shard
// s holds the rows [s * shard_rows, (s + 1) * shard_rows).
//
// SearchKnn (kk <= 64, the planner's case) exchanges the lists over RCCL: the index keeps ONE communicator over its distinct devices
// (ncclCommInitAll), every device's scans write their sorted lists straight into that device's send buffer, one ncclAllGather per query
// batch (inside ncclGroupStart/End, on the shards' streams: kk x 8 B x nq per shard over xGMI), knn_merge_shards on device 0, ONE D2H copy.
// One host thread enqueues everything; nothing is merged on the host.  RXGPU_SHARD_MERGE=host keeps the former path (a worker thread per
// shard, D2H per shard, host merge), which also serves range searches, pre-filtered searches, kk > 64 and shards holding fewer than kk rows.
// The one-process-per-GPU deployment (torch.distributed over the same RCCL) is reindexer_amd/sharded.py.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include "rccl_dyn.h"   // <rccl/rccl.h> for types and prototypes only: the library is opened at the first sharded index (rxgpu_rccl.hip)

#include "../../include/rxgpu.h"
#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"
#include "shard_plan.h"   // every decision below: row cut, rank layout, row-list split, exchange shape and routes, host merges, retry sizes

using rxgpu::set_error;

namespace rxgpu {

// A small pool of worker threads per shard (the shard's device stays current on them) behind one job queue: fan-outs of concurrent
// callers queue up per shard and overlap — the single-device entry points are re-entrant (a search context and stream per call) — so
// no lock is held across a fan-out.  Searches share `call_mtx`, mutations take it exclusively (the reference's namespace lock above us
// does the same; this one only protects direct C-ABI callers).
struct ShardWorker {
	static constexpr unsigned kThreads = 4;
	std::vector<std::thread> threads;
	std::mutex mtx;
	std::condition_variable cv;
	std::deque<std::function<void()>> jobs;
	bool stop = false;

	void run() {
		std::unique_lock<std::mutex> lk(mtx);
		for (;;) {
			cv.wait(lk, [&] { return !jobs.empty() || stop; });
			if (jobs.empty()) return;   // stop requested and nothing left
			auto fn = std::move(jobs.front());
			jobs.pop_front();
			lk.unlock();
			fn();
			lk.lock();
		}
	}
	void post(std::function<void()> fn) {
		{
			std::lock_guard<std::mutex> lk(mtx);
			jobs.push_back(std::move(fn));
		}
		cv.notify_one();
	}
};

// Buffers and streams of one exchange in flight (per distinct device = RCCL rank); lanes are pooled so that concurrent callers overlap.
struct ExchangeLane {
	std::vector<hipStream_t> stream;
	std::vector<rxgpu_devbuf> d_queries, d_local, d_gathered;
	rxgpu_devbuf d_out;            // rank 0: [nq][kk] distances | [nq][kk] global rows | [nq] counts
	void* h_pinned = nullptr;      // queries on the way in, the merged lists on the way out
	size_t h_pinned_bytes = 0;
};

// The RCCL side of a sharded index: one rank per DISTINCT device; a device that holds several shards (the 1-GPU test box lists the same
// device several times) sends them as `slots` consecutive lists, devices with fewer shards pad (slot base = kInvalidRow, skipped by the merge).
struct ShardExchange {
	RankLayout lay;                    // ranks, slots and gathered positions of the shards (shard_plan.h)
	std::shared_ptr<RcclCommSet> cs;   // the process-wide communicators over lay.rank_dev (rccl_dyn.h)
	uint32_t* d_slot_base = nullptr;   // on rank_dev[0]: lay.base, the global row base of every gathered position
	std::mutex mtx;                    // lane pool
	std::vector<ExchangeLane*> free_lanes;
	std::atomic<uint64_t> collectives{0};
};

struct ShardSet {
	std::vector<rxgpu_index*> shards;
	std::vector<ShardWorker*> workers;
	ShardCut cut;                 // shard s holds the global rows [s * cut.shard_rows, (s + 1) * cut.shard_rows)
	std::shared_mutex call_mtx;   // shared: searches (any number of fan-outs in flight); exclusive: uploads, moves, truncation
	ShardExchange* xch = nullptr; // null: the host-merge path (RXGPU_SHARD_MERGE=host, or RCCL is not available: merge_note says why)
	std::string merge_note;
	std::vector<uint64_t> counts() const {   // rows every shard holds now
		std::vector<uint64_t> c;
		for (const rxgpu_index* sh : shards) c.push_back(rxgpu_index_count(sh));
		return c;
	}
};

namespace {

// completion latch of one fan-out (lives on the caller's stack)
struct FanOut {
	std::mutex m;
	std::condition_variable cv;
	size_t left;
	explicit FanOut(size_t n) : left(n) {}
	void arrive() {
		std::lock_guard<std::mutex> lk(m);
		if (--left == 0) cv.notify_all();
	}
	void wait() {
		std::unique_lock<std::mutex> lk(m);
		cv.wait(lk, [&] { return left == 0; });
	}
};

// runs fn on the worker pool of shard s and waits; an exception inside (bad_alloc while staging) becomes RXGPU_ERR_NOMEM
int run_on_shard(ShardSet* ss, size_t s, const std::function<int()>& fn, std::string& err) {
	int rc = RXGPU_OK;
	FanOut done(1);
	ss->workers[s]->post([&] {
		try {
			rc = fn();
			if (rc != RXGPU_OK) err = rxgpu_last_error();   // thread-local on the worker: carry it over
		} catch (const std::exception& e) {
			rc = RXGPU_ERR_NOMEM;
			err = e.what();
		}
		done.arrive();
	});
	done.wait();
	return rc;
}

// runs fn(s) for every shard concurrently; returns the first non-OK code (the message of that shard is kept)
int for_each_shard(ShardSet* ss, const std::function<int(size_t)>& fn) {
	const size_t n = ss->shards.size();
	std::vector<int> rc(n, RXGPU_OK);
	std::vector<std::string> err(n);
	FanOut done(n);
	for (size_t s = 0; s < n; ++s) {
		ss->workers[s]->post([&, s] {
			try {
				rc[s] = fn(s);
				if (rc[s] != RXGPU_OK) err[s] = rxgpu_last_error();
			} catch (const std::exception& e) {
				rc[s] = RXGPU_ERR_NOMEM;
				err[s] = e.what();
			}
			done.arrive();
		});
	}
	done.wait();
	for (size_t s = 0; s < n; ++s) {
		if (rc[s] != RXGPU_OK) {
			set_error("shard " + std::to_string(s) + ": " + err[s]);
			return rc[s];
		}
	}
	return RXGPU_OK;
}

}  // namespace


#define SH_HIP(expr)                                                                       \
	do {                                                                                   \
		hipError_t e__ = (expr);                                                           \
		if (e__ != hipSuccess) {                                                           \
			set_error(std::string(#expr) + ": " + hipGetErrorString(e__));                 \
			return e__ == hipErrorOutOfMemory ? RXGPU_ERR_NOMEM : RXGPU_ERR_DEVICE;        \
		}                                                                                  \
	} while (0)
#define SH_NCCL(expr)                                                                      \
	do {                                                                                   \
		ncclResult_t r__ = (expr);                                                         \
		if (r__ != ncclSuccess) {                                                          \
			set_error(std::string(#expr) + ": " + rccl_api().ncclGetErrorString(r__));     \
			return RXGPU_ERR_DEVICE;                                                       \
		}                                                                                  \
	} while (0)

namespace {

struct CurrentDevice {   // restores the caller's device
	int prev = -1;
	CurrentDevice() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
	~CurrentDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

void free_lane(ShardExchange* x, ExchangeLane* l) {
	for (uint32_t r = 0; r < x->lay.nranks; ++r) {
		(void)hipSetDevice(x->lay.rank_dev[r]);
		if (r < l->stream.size() && l->stream[r]) {
			(void)hipStreamSynchronize(l->stream[r]);
			(void)hipStreamDestroy(l->stream[r]);
		}
		if (r < l->d_queries.size()) l->d_queries[r].release();
		if (r < l->d_local.size()) l->d_local[r].release();
		if (r < l->d_gathered.size()) l->d_gathered[r].release();
	}
	(void)hipSetDevice(x->lay.rank_dev[0]);
	l->d_out.release();
	if (l->h_pinned) (void)hipHostFree(l->h_pinned);
	delete l;
}

int new_lane(ShardExchange* x, ExchangeLane** out) {
	auto* l = new ExchangeLane();
	l->stream.assign(x->lay.nranks, nullptr);
	l->d_queries.resize(x->lay.nranks);
	l->d_local.resize(x->lay.nranks);
	l->d_gathered.resize(x->lay.nranks);
	for (uint32_t r = 0; r < x->lay.nranks; ++r) {
		hipError_t e = hipSetDevice(x->lay.rank_dev[r]);
		if (e == hipSuccess) e = hipStreamCreateWithFlags(&l->stream[r], hipStreamNonBlocking);
		if (e != hipSuccess) {
			set_error(std::string("sharded exchange: stream on device ") + std::to_string(x->lay.rank_dev[r]) + ": " + hipGetErrorString(e));
			free_lane(x, l);
			return RXGPU_ERR_DEVICE;
		}
	}
	*out = l;
	return RXGPU_OK;
}

void exchange_destroy(ShardExchange* x) {
	if (!x) return;
	CurrentDevice cd;
	for (ExchangeLane* l : x->free_lanes) free_lane(x, l);
	if (x->d_slot_base) {
		(void)hipSetDevice(x->lay.rank_dev[0]);
		(void)hipFree(x->d_slot_base);
	}
	delete x;
}

// One communicator over the distinct devices of the shard list, and the position -> global row base table of the merge kernel.
int exchange_create(ShardSet* ss, uint32_t n_devices, const int* devices, ShardExchange** out) {
	auto* x = new ShardExchange();
	x->lay = rank_layout(devices, n_devices, ss->cut.shard_rows, kInvalidRow);
	CurrentDevice cd;
	std::string why;
	x->cs = rccl_comm_set(x->lay.rank_dev, &why);
	if (!x->cs) {
		set_error(why);
		delete x;
		return RXGPU_ERR_DEVICE;
	}
	const std::vector<uint32_t>& base = x->lay.base;
	hipError_t e = hipSetDevice(x->lay.rank_dev[0]);
	if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&x->d_slot_base), base.size() * sizeof(uint32_t));
	if (e == hipSuccess) e = hipMemcpy(x->d_slot_base, base.data(), base.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		set_error(std::string("rxgpu_index_create_sharded: slot table: ") + hipGetErrorString(e));
		exchange_destroy(x);
		return RXGPU_ERR_DEVICE;
	}
	*out = x;
	return RXGPU_OK;
}

// The second half of every exchange: the per-shard lists sit in d_local of their rank's device (on that rank's lane stream) -> ONE
// ncclAllGather per query batch -> knn_merge_shards on the first device -> one D2H copy of the merged lists.
int exchange_gather_merge(ShardSet* ss, ExchangeLane* l, const ExchangeShape& e, uint32_t nq, uint32_t kk, bool sorted, float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	ShardExchange* x = ss->xch;
	{
		std::lock_guard<std::mutex> lk(x->cs->mtx);
		const RcclApi& api = rccl_api();
		SH_NCCL(api.ncclGroupStart());
		for (uint32_t r = 0; r < x->lay.nranks; ++r) {
			const ncclResult_t nr = api.ncclAllGather(l->d_local[r].ptr, l->d_gathered[r].ptr, e.list_words * x->lay.slots, ncclUint32, x->cs->comms[r], l->stream[r]);
			if (nr != ncclSuccess) {
				(void)api.ncclGroupEnd();
				set_error(std::string("ncclAllGather: ") + api.ncclGetErrorString(nr));
				return RXGPU_ERR_DEVICE;
			}
		}
		SH_NCCL(api.ncclGroupEnd());
		x->collectives.fetch_add(1, std::memory_order_relaxed);
	}
	SH_HIP(hipSetDevice(x->lay.rank_dev[0]));
	if (int rc = l->d_out.ensure(e.out_bytes); rc) return rc;
	uint32_t* d_o = static_cast<uint32_t*>(l->d_out.ptr);
	float* d_od = reinterpret_cast<float*>(d_o + e.o_dist);
	uint32_t *d_or = d_o + e.o_row, *d_oc = d_o + e.o_count;
	launch_merge_shards(static_cast<const uint32_t*>(l->d_gathered[0].ptr), uint32_t(x->lay.positions()), nq, kk, 0, d_od, d_or, d_oc, l->stream[0], x->d_slot_base, sorted);
	SH_HIP(hipGetLastError());
	SH_HIP(hipMemcpyAsync(l->h_pinned, l->d_out.ptr, e.out_bytes, hipMemcpyDeviceToHost, l->stream[0]));
	for (uint32_t r = 0; r < x->lay.nranks; ++r) SH_HIP(hipStreamSynchronize(l->stream[r]));
	const auto* hp = static_cast<const uint32_t*>(l->h_pinned);
	std::memcpy(out_dist, hp + e.o_dist, size_t(nq) * kk * sizeof(float));
	std::memcpy(out_row, hp + e.o_row, size_t(nq) * kk * sizeof(uint32_t));
	std::memcpy(out_count, hp + e.o_count, size_t(nq) * sizeof(uint32_t));
	return RXGPU_OK;
}

int ensure_pinned(ExchangeLane* l, size_t pin) {
	if (l->h_pinned_bytes < pin) {
		if (l->h_pinned) (void)hipHostFree(l->h_pinned);
		l->h_pinned = nullptr;
		l->h_pinned_bytes = 0;
		SH_HIP(hipHostMalloc(&l->h_pinned, pin, hipHostMallocDefault));
		l->h_pinned_bytes = pin;
	}
	return RXGPU_OK;
}

// SearchKnn over every shard with the exchange on the devices.  The caller holds call_mtx shared and has checked the shape
// (knn_takes_exchange over lc, the rows every shard holds).
int exchange_search_knn(rxgpu_index* h, ShardSet* ss, ExchangeLane* l, const std::vector<uint64_t>& lc, const float* queries, uint32_t nq, uint32_t kk,
						float* out_dist, uint32_t* out_row, uint32_t* out_count) {
	ShardExchange* x = ss->xch;
	const ExchangeShape e = exchange_shape(nq, kk, x->lay.nranks, x->lay.slots, h->dim);
	if (int rc = ensure_pinned(l, e.pinned_knn()); rc) return rc;
	std::memcpy(l->h_pinned, queries, e.qbytes);
	const bool hole = exchange_hole(x->lay, lc.data(), lc.size());
	for (uint32_t r = 0; r < x->lay.nranks; ++r) {
		SH_HIP(hipSetDevice(x->lay.rank_dev[r]));
		if (int rc = l->d_queries[r].ensure(e.qbytes); rc) return rc;
		if (int rc = l->d_local[r].ensure(e.local_bytes); rc) return rc;
		if (int rc = l->d_gathered[r].ensure(e.gathered_bytes); rc) return rc;
		SH_HIP(hipMemcpyAsync(l->d_queries[r].ptr, l->h_pinned, e.qbytes, hipMemcpyHostToDevice, l->stream[r]));
		if (hole) SH_HIP(hipMemsetAsync(l->d_local[r].ptr, 0xFF, e.local_bytes, l->stream[r]));   // rows = kInvalidRow
		for (size_t s = 0; s < ss->shards.size(); ++s) {
			if (x->lay.shard_rank[s] != r || lc[s] == 0) continue;
			uint32_t* dst = static_cast<uint32_t*>(l->d_local[r].ptr) + e.list_words * x->lay.shard_slot[s];
			if (int rc = rxgpu_search_knn_device(ss->shards[s], l->d_queries[r].ptr, nq, kk, dst, dst + size_t(nq) * kk, nullptr, l->stream[r]); rc) return rc;
		}
	}
	return exchange_gather_merge(ss, l, e, nq, kk, true, out_dist, out_row, out_count);
}

// HNSW SearchKnn over every shard's own graph (SURVEY 8e "HNSW"): the searches run concurrently on the shards' worker threads — each is the
// single-device search with its re-run tiers, driven from the host by the counts alone — and leave their lists in HBM, packed into the
// shard's slot of the send buffer (HnswSink); then the same all-gather + merge as brute force (the lists are unordered sets: sorted = false).
int exchange_hnsw_search_knn(rxgpu_index* h, ShardSet* ss, ExchangeLane* l, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist,
							 uint32_t* out_row, uint32_t* out_count) {
	ShardExchange* x = ss->xch;
	const ExchangeShape e = exchange_shape(nq, k, x->lay.nranks, x->lay.slots, h->dim);
	if (int rc = ensure_pinned(l, e.pinned_hnsw()); rc) return rc;
	for (uint32_t r = 0; r < x->lay.nranks; ++r) {
		SH_HIP(hipSetDevice(x->lay.rank_dev[r]));
		if (int rc = l->d_local[r].ensure(e.local_bytes); rc) return rc;
		if (int rc = l->d_gathered[r].ensure(e.gathered_bytes); rc) return rc;
		SH_HIP(hipMemsetAsync(l->d_local[r].ptr, 0xFF, e.local_bytes, l->stream[r]));   // empty shards and padded slots: rows = kInvalidRow
		SH_HIP(hipStreamSynchronize(l->stream[r]));                                    // the searches write from their own streams
	}
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		if (rxgpu_index_count(ss->shards[s]) == 0) return RXGPU_OK;
		uint32_t* dst = static_cast<uint32_t*>(l->d_local[x->lay.shard_rank[s]].ptr) + e.list_words * x->lay.shard_slot[s];
		return hnsw_search_to_sink(ss->shards[s], queries, qcorr, qnorm, nq, k, ef, HnswSink{dst, dst + size_t(nq) * k, k});
	});
	if (rc != RXGPU_OK) return rc;
	return exchange_gather_merge(ss, l, e, nq, k, false, out_dist, out_row, out_count);
}

ExchangeLane* take_lane(ShardExchange* x) {
	std::lock_guard<std::mutex> pl(x->mtx);
	if (x->free_lanes.empty()) return nullptr;
	ExchangeLane* lane = x->free_lanes.back();
	x->free_lanes.pop_back();
	return lane;
}

void give_lane(ShardExchange* x, ExchangeLane* lane, int rc) {
	if (rc != RXGPU_OK) {   // streams may hold half an exchange: drain before the lane is reused
		for (uint32_t r = 0; r < x->lay.nranks; ++r) {
			(void)hipSetDevice(x->lay.rank_dev[r]);
			(void)hipStreamSynchronize(lane->stream[r]);
		}
	}
	std::lock_guard<std::mutex> pl(x->mtx);
	x->free_lanes.push_back(lane);
}

// fn(lane) on a lane of its own (a pooled one, or a new one), with the caller's device restored behind it
template <class Fn>
int on_lane(ShardExchange* x, Fn&& fn) {
	CurrentDevice cd;
	ExchangeLane* lane = take_lane(x);
	if (!lane) {
		if (int rc = new_lane(x, &lane); rc) return rc;
	}
	const int rc = fn(lane);
	give_lane(x, lane, rc);
	return rc;
}

// a vector per shard as the array of pointers the plan's merges take
template <class T>
std::vector<const T*> data_of(const std::vector<std::vector<T>>& v) {
	std::vector<const T*> p;
	for (const auto& e : v) p.push_back(e.data());
	return p;
}

}  // namespace

void sharded_destroy(rxgpu_index* h) {
	ShardSet* ss = h->shard_set;
	if (!ss) return;
	exchange_destroy(ss->xch);
	ss->xch = nullptr;
	for (ShardWorker* w : ss->workers) {
		{
			std::lock_guard<std::mutex> lk(w->mtx);
			w->stop = true;
			w->cv.notify_all();
		}
		for (std::thread& t : w->threads) {
			if (t.joinable()) t.join();
		}
		delete w;
	}
	for (rxgpu_index* s : ss->shards) rxgpu_index_destroy(s);
	delete ss;
	h->shard_set = nullptr;
}

uint64_t sharded_device_bytes(const rxgpu_index* h) {
	uint64_t b = 0;
	for (const rxgpu_index* s : h->shard_set->shards) b += rxgpu_index_device_bytes(s);
	return b;
}

int sharded_upload_rows(rxgpu_index* h, uint64_t first_row, uint64_t n, const float* rows, const float* inv_norms) {
	ShardSet* ss = h->shard_set;
	if (n == 0) return RXGPU_OK;
	if (!rows) {
		set_error("rxgpu_index_upload_rows: rows is null");
		return RXGPU_ERR_PARAMS;
	}
	if (first_row > h->count || first_row + n > h->capacity) {
		set_error(first_row > h->count ? "rxgpu_index_upload_rows: a sharded index is filled without holes (first_row <= count)"
									   : "The number of elements exceeds the specified limit");
		return RXGPU_ERR_PARAMS;
	}
	std::unique_lock<std::shared_mutex> lk(ss->call_mtx);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		uint64_t a, b;
		if (!ss->cut.piece(s, first_row, n, a, b)) return RXGPU_OK;
		return rxgpu_index_upload_rows(ss->shards[s], a - ss->cut.base(s), b - a, rows + (a - first_row) * h->dim, inv_norms ? inv_norms + (a - first_row) : nullptr);
	});
	if (rc == RXGPU_OK) h->count = std::max(h->count, first_row + n);
	return rc;
}

int sharded_truncate(rxgpu_index* h, uint64_t count) {
	ShardSet* ss = h->shard_set;
	if (count > h->count) {
		set_error("rxgpu_index_truncate: count exceeds the number of rows");
		return RXGPU_ERR_PARAMS;
	}
	std::unique_lock<std::shared_mutex> lk(ss->call_mtx);
	const int rc = for_each_shard(ss, [&](size_t s) -> int { return rxgpu_index_truncate(ss->shards[s], ss->cut.local_count(s, count)); });
	if (rc == RXGPU_OK) h->count = count;
	return rc;
}

// exact top-kk of every query under (dist, global row): through the exchange, or per-shard exact top-kk lists merged on the host
int sharded_search_knn_impl(rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* row_ids, uint64_t n_ids, float* out_dist,
							uint32_t* out_row, uint32_t* out_count) {
	ShardSet* ss = h->shard_set;
	const size_t ns = ss->shards.size();
	// a row list (pre-filtered search) is split at the shard boundaries; local ids = global - shard base
	const RowSplit sp = split_row_list(row_ids, row_ids ? n_ids : 0, h->count, ss->cut.shard_rows, ns, true);
	if (sp.rule != kRowListOk) {
		set_error(sp.rule == kRowListNotIncreasing ? "rxgpu_search_knn_subset: row ids must be strictly increasing" : "rxgpu_search_knn_subset: row id out of range");
		return RXGPU_ERR_PARAMS;
	}
	std::shared_lock<std::shared_mutex> lk(ss->call_mtx);
	const std::vector<uint64_t> lc = ss->counts();
	if (knn_takes_exchange(ss->xch != nullptr, row_ids != nullptr, kk, uint32_t(kMaxFusedK), lc.data(), ns)) {
		return on_lane(ss->xch, [&](ExchangeLane* lane) { return exchange_search_knn(h, ss, lane, lc, queries, nq, kk, out_dist, out_row, out_count); });
	}
	std::vector<std::vector<float>> sd(ns);
	std::vector<std::vector<uint32_t>> sr(ns), sc(ns);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		sd[s].assign(size_t(nq) * kk, 0.f);
		sr[s].assign(size_t(nq) * kk, 0u);
		sc[s].assign(nq, 0u);
		if (row_ids) {
			if (sp.local[s].empty()) return RXGPU_OK;
			return rxgpu_search_knn_subset(ss->shards[s], queries, nq, kk, sp.local[s].data(), sp.local[s].size(), sd[s].data(), sr[s].data(), sc[s].data());
		}
		if (lc[s] == 0) return RXGPU_OK;
		return rxgpu_search_knn(ss->shards[s], queries, nq, kk, sd[s].data(), sr[s].data(), sc[s].data());
	});
	if (rc != RXGPU_OK) return rc;
	const std::vector<size_t> stride(ns, kk);
	const auto pd = data_of(sd);
	const auto pr = data_of(sr), pc = data_of(sc);
	merge_shard_topk(ShardLists{pd.data(), pr.data(), pc.data(), stride.data()}, ns, ss->cut.shard_rows, nq, kk, out_dist, out_row, out_count);
	return RXGPU_OK;
}

int sharded_search_range_impl(rxgpu_index* h, const float* query, float radius, int inclusive, const uint32_t* row_ids, uint64_t n_ids, float* out_dist,
							  uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	ShardSet* ss = h->shard_set;
	const size_t ns = ss->shards.size();
	const RowSplit sp = split_row_list(row_ids, row_ids ? n_ids : 0, h->count, ss->cut.shard_rows, ns, true);
	if (sp.rule != kRowListOk) {
		set_error("rxgpu_search_range_subset: row ids must be strictly increasing and below count");
		return RXGPU_ERR_PARAMS;
	}
	std::vector<std::vector<float>> sd(ns);
	std::vector<std::vector<uint32_t>> sr(ns);
	std::vector<uint64_t> st(ns, 0);
	std::shared_lock<std::shared_mutex> lk(ss->call_mtx);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		uint64_t want = 0;
		for (int attempt = 0; attempt < kRangeAttempts; ++attempt) {   // a shard that overflows its buffer is asked again with the size it reported
			want = range_want(cap, want, st[s]);
			sd[s].resize(want);
			sr[s].resize(want);
			int r;
			if (row_ids) {
				if (sp.local[s].empty()) {
					st[s] = 0;
					return RXGPU_OK;
				}
				r = rxgpu_search_range_subset(ss->shards[s], query, radius, inclusive, sp.local[s].data(), sp.local[s].size(), sd[s].data(), sr[s].data(), want, &st[s]);
			} else {
				if (rxgpu_index_count(ss->shards[s]) == 0) {
					st[s] = 0;
					return RXGPU_OK;
				}
				r = rxgpu_search_range(ss->shards[s], query, radius, inclusive, sd[s].data(), sr[s].data(), want, &st[s]);
			}
			if (r != RXGPU_ERR_OVERFLOW) return r;
		}
		return RXGPU_ERR_OVERFLOW;
	});
	if (rc != RXGPU_OK) return rc;
	// (an overflow here leaves the first cap hits in the caller's buffers; a single-device index writes none — rxgpu_knn_search.hip)
	*out_total = merge_shard_ranges(data_of(sd).data(), data_of(sr).data(), st.data(), ns, ss->cut.shard_rows, cap, out_dist, out_row);
	if (*out_total > cap) {
		set_error("rxgpu_search_range: more hits than the output buffer holds");
		return RXGPU_ERR_OVERFLOW;
	}
	return RXGPU_OK;
}

// rxgpu_hnsw_search_knn on a sharded handle: every shard searches its own graph (attached through rxgpu_index_shard(h, s)); the merged list
// of a query = the k best of the union of the per-shard results under (dist, global row), global row = s * shard_rows + local row.
// out_count[q] <= k entries, sorted (a superset of the single-device contract, which leaves them unordered).
int sharded_hnsw_search_knn(rxgpu_index* h, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row,
							uint32_t* out_count) {
	ShardSet* ss = h->shard_set;
	const size_t ns = ss->shards.size();
	if (nq == 0) return RXGPU_OK;
	if (k == 0) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	std::shared_lock<std::shared_mutex> lk(ss->call_mtx);
	const std::vector<uint64_t> lc = ss->counts();
	if (std::all_of(lc.begin(), lc.end(), [](uint64_t c) { return c == 0; })) {
		std::fill(out_count, out_count + nq, 0u);
		return RXGPU_OK;
	}
	if (hnsw_takes_exchange(ss->xch != nullptr, k, uint32_t(kMaxFusedK))) {
		return on_lane(ss->xch, [&](ExchangeLane* lane) { return exchange_hnsw_search_knn(h, ss, lane, queries, qcorr, qnorm, nq, k, ef, out_dist, out_row, out_count); });
	}
	std::vector<std::vector<float>> sd(ns);
	std::vector<std::vector<uint32_t>> sr(ns), sc(ns);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		sd[s].assign(size_t(nq) * k, 0.f);
		sr[s].assign(size_t(nq) * k, 0u);
		sc[s].assign(nq, 0u);
		if (lc[s] == 0) return RXGPU_OK;
		if (qcorr) {
			return rxgpu_hnsw_search_knn_sq8(ss->shards[s], static_cast<const uint8_t*>(queries), qcorr, qnorm, nq, k, ef, sd[s].data(), sr[s].data(), sc[s].data());
		}
		return rxgpu_hnsw_search_knn(ss->shards[s], static_cast<const float*>(queries), nq, k, ef, sd[s].data(), sr[s].data(), sc[s].data());
	});
	if (rc != RXGPU_OK) return rc;
	// a shard's search clamps k to the points it holds and writes its lists with THAT stride (hnsw_search_impl: p.k = min(k, count))
	std::vector<size_t> stride(ns);
	for (size_t s = 0; s < ns; ++s) stride[s] = size_t(std::min<uint64_t>(k, lc[s]));
	const auto pd = data_of(sd);
	const auto pr = data_of(sr), pc = data_of(sc);
	merge_shard_topk(ShardLists{pd.data(), pr.data(), pc.data(), stride.data()}, ns, ss->cut.shard_rows, nq, k, out_dist, out_row, out_count);
	return RXGPU_OK;
}

// HierarchicalNSW::SearchRange over the shards' graphs: every shard's ef-search + closure (rxgpu_hnsw_search_range), hits concatenated with
// global rows (unordered, like the single-device call).  Overflow protocol as there: *out_total = hits counted so far.
int sharded_hnsw_search_range(rxgpu_index* h, const float* query, float radius, uint32_t ef, float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total) {
	ShardSet* ss = h->shard_set;
	const size_t ns = ss->shards.size();
	if (!query || !out_total || (cap && !(out_dist && out_row))) {
		set_error("rxgpu_hnsw_search_range: null argument");
		return RXGPU_ERR_PARAMS;
	}
	*out_total = 0;
	std::vector<std::vector<float>> sd(ns);
	std::vector<std::vector<uint32_t>> sr(ns);
	std::vector<uint64_t> st(ns, 0);
	std::shared_lock<std::shared_mutex> lk(ss->call_mtx);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		if (rxgpu_index_count(ss->shards[s]) == 0) return RXGPU_OK;
		uint64_t want = 0;
		for (int attempt = 0; attempt < kHnswRangeAttempts; ++attempt) {   // the count an overflow reports is a lower bound: grow until the closure fits
			want = hnsw_range_want(cap, want, st[s]);
			sd[s].resize(want);
			sr[s].resize(want);
			const int r = rxgpu_hnsw_search_range(ss->shards[s], query, radius, ef, sd[s].data(), sr[s].data(), want, &st[s]);
			if (r != RXGPU_ERR_OVERFLOW) return r;
		}
		return RXGPU_ERR_OVERFLOW;
	});
	if (rc != RXGPU_OK) return rc;
	*out_total = concat_shard_ranges(data_of(sd).data(), data_of(sr).data(), st.data(), ns, ss->cut.shard_rows, cap, out_dist, out_row);
	if (*out_total > cap) {
		set_error("rxgpu_hnsw_search_range: more hits than the output buffer holds");
		return RXGPU_ERR_OVERFLOW;
	}
	return RXGPU_OK;
}

int sharded_distances(rxgpu_index* h, const float* query, const uint32_t* rows, uint32_t n, float* out_dist) {
	ShardSet* ss = h->shard_set;
	const size_t ns = ss->shards.size();
	const RowSplit sp = split_row_list(rows, n, h->count, ss->cut.shard_rows, ns, false);
	if (sp.rule != kRowListOk) {
		set_error("rxgpu_distances: row out of range");
		return RXGPU_ERR_PARAMS;
	}
	std::vector<std::vector<float>> sd(ns);
	std::shared_lock<std::shared_mutex> lk(ss->call_mtx);
	const int rc = for_each_shard(ss, [&](size_t s) -> int {
		if (sp.local[s].empty()) return RXGPU_OK;
		sd[s].resize(sp.local[s].size());
		return rxgpu_distances(ss->shards[s], query, sp.local[s].data(), uint32_t(sp.local[s].size()), sd[s].data());
	});
	if (rc != RXGPU_OK) return rc;
	for (size_t s = 0; s < ns; ++s) {
		for (size_t j = 0; j < sp.where[s].size(); ++j) out_dist[sp.where[s][j]] = sd[s][j];
	}
	return RXGPU_OK;
}

// RemovePoint's swap-with-last across shards: the row travels through the host (two devices may be involved)
int sharded_move_row(rxgpu_index* h, uint64_t from, uint64_t to) {
	ShardSet* ss = h->shard_set;
	if (from >= h->count || to >= h->count) {
		set_error("rxgpu_index_move_row: row out of range");
		return RXGPU_ERR_PARAMS;
	}
	if (from == to) return RXGPU_OK;
	const size_t sf = ss->cut.shard_of(from), st = ss->cut.shard_of(to);
	std::unique_lock<std::shared_mutex> lk(ss->call_mtx);
	std::string err;
	int rc;
	if (sf == st) {
		rc = run_on_shard(ss, sf, [&] { return rxgpu_index_move_row(ss->shards[sf], ss->cut.local(from), ss->cut.local(to)); }, err);
	} else {
		std::vector<float> row(h->dim);
		float norm = 0.f;
		rc = run_on_shard(ss, sf, [&] { return rxgpu_index_download_row(ss->shards[sf], ss->cut.local(from), row.data(), &norm); }, err);
		if (rc == RXGPU_OK) {
			rc = run_on_shard(ss, st, [&] {
				return rxgpu_index_upload_rows(ss->shards[st], ss->cut.local(to), 1, row.data(), h->metric == RXGPU_METRIC_COSINE ? &norm : nullptr);
			}, err);
		}
	}
	if (rc != RXGPU_OK) set_error(err);
	return rc;
}

}  // namespace rxgpu

extern "C" {

int rxgpu_index_create_sharded(int metric, uint32_t dim, uint64_t capacity, uint32_t n_devices, const int* devices, rxgpu_index** out) {
	if (!out || !devices || n_devices == 0 || n_devices > 64) {
		set_error("rxgpu_index_create_sharded: bad arguments (1..64 devices)");
		return RXGPU_ERR_PARAMS;
	}
	if (capacity == 0 || capacity >= 0xFFFFFFFFull) {
		set_error("rxgpu_index_create_sharded: capacity must be in [1, 2^32)");
		return RXGPU_ERR_PARAMS;
	}
	*out = nullptr;
	auto* ss = new rxgpu::ShardSet();
	ss->cut.shard_rows = rxgpu::shard_rows_for(capacity, n_devices);
	auto* h = new rxgpu_index();
	h->metric = metric;
	h->dim = dim;
	h->stride = (dim + 3u) & ~3u;
	h->device = devices[0];
	h->capacity = capacity;
	h->shard_set = ss;
	for (uint32_t s = 0; s < n_devices; ++s) {
		rxgpu_index* sh = nullptr;
		const int rc = rxgpu_index_create(metric, dim, std::max<uint64_t>(ss->cut.local_count(s, capacity), 1), devices[s], &sh);
		if (rc != RXGPU_OK) {
			rxgpu::sharded_destroy(h);
			delete h;
			return rc;
		}
		ss->shards.push_back(sh);
		auto* w = new rxgpu::ShardWorker();
		for (unsigned t = 0; t < rxgpu::ShardWorker::kThreads; ++t) {
			w->threads.emplace_back([w, dev = devices[s]] {
				(void)hipSetDevice(dev);
				w->run();
			});
		}
		ss->workers.push_back(w);
	}
	const char* mode = getenv("RXGPU_SHARD_MERGE");
	if (mode && std::strcmp(mode, "host") == 0) {
		ss->merge_note = "RXGPU_SHARD_MERGE=host";
	} else if (rxgpu::exchange_create(ss, n_devices, devices, &ss->xch) != RXGPU_OK) {
		// no device-side exchange on this node: the index works on the host-merge path (same results); said once per index, and kept for
		// rxgpu_index_shard_merge_note
		ss->xch = nullptr;
		ss->merge_note = rxgpu_last_error();
		fprintf(stderr, "rxgpu: sharded index over %u device slot(s): %s — per-shard lists are merged on the host\n", n_devices, ss->merge_note.c_str());
	}
	*out = h;
	return RXGPU_OK;
}

int rxgpu_index_shard_merge_mode(const rxgpu_index* h) { return h && h->shard_set ? (h->shard_set->xch ? 1 : 0) : -1; }
const char* rxgpu_index_shard_merge_note(const rxgpu_index* h) { return h && h->shard_set ? h->shard_set->merge_note.c_str() : ""; }
uint32_t rxgpu_index_shard_ranks(const rxgpu_index* h) { return h && h->shard_set && h->shard_set->xch ? h->shard_set->xch->lay.nranks : 0; }
uint64_t rxgpu_index_shard_collectives(const rxgpu_index* h) {
	return h && h->shard_set && h->shard_set->xch ? h->shard_set->xch->collectives.load(std::memory_order_relaxed) : 0;
}
rxgpu_index* rxgpu_index_shard(rxgpu_index* h, uint32_t s) {
	return h && h->shard_set && s < h->shard_set->shards.size() ? h->shard_set->shards[s] : nullptr;
}
/* After the caller filled shards directly (rxgpu_index_adopt_device_rows on rxgpu_index_shard handles): count = rows held, which must
 * form a prefix of the global row space (every shard before the last non-empty one full). */
int rxgpu_index_shard_sync_count(rxgpu_index* h) {
	if (!h || !h->shard_set) {
		set_error("rxgpu_index_shard_sync_count: not a sharded index");
		return RXGPU_ERR_PARAMS;
	}
	rxgpu::ShardSet* ss = h->shard_set;
	std::unique_lock<std::shared_mutex> lk(ss->call_mtx);
	const std::vector<uint64_t> lc = ss->counts();
	uint64_t total = 0;
	if (!rxgpu::shard_prefix_total(lc.data(), lc.size(), ss->cut.shard_rows, total)) {
		set_error("rxgpu_index_shard_sync_count: shards must hold a prefix of the global rows (full shards, then at most one partial)");
		return RXGPU_ERR_PARAMS;
	}
	h->count = total;
	return RXGPU_OK;
}

uint32_t rxgpu_index_shard_count(const rxgpu_index* h) { return h && h->shard_set ? uint32_t(h->shard_set->shards.size()) : 0; }
uint64_t rxgpu_index_shard_rows(const rxgpu_index* h) { return h && h->shard_set ? h->shard_set->cut.shard_rows : 0; }


}  // extern "C"
