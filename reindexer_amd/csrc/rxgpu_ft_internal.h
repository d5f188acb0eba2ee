// What the host units of the BM25 merge share (rxgpu_ft_*.hip, rxgpu_hybrid.hip): the handles behind rxgpu_ft_index*, the types that travel
// between the units and the functions one unit calls in another.  Everything a single unit uses stays in that unit.
//   rxgpu_ft_capi.hip     lifetime, lanes, the dictionary calls          rxgpu_ft_packed.hip   packed uploads (ft_packed_plan.h decides)
//   rxgpu_ft_phrase.hip   one phrase through ft_phrase.hip              rxgpu_ft_merge.hip    one merge on one lane (ft_merge_plan.h decides)
//   rxgpu_ft_calls.hip    the merge entry points, the batch train       rxgpu_ft_sharded.hip  document-range shards
//   rxgpu_hybrid.hip      the fusion behind a resident merge
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/rxgpu.h"
#include "rccl_dyn.h"
#include "rxgpu_internal.h"

struct rxgpu_ft_word {
	uint64_t n = 0, nent = 0;
	uint32_t* doc = nullptr;
	uint32_t* ent_off = nullptr;
	uint8_t* ent_field = nullptr;
	uint32_t* ent_tf = nullptr;
	uint32_t* ent_first_pos = nullptr;
	uint32_t* pos_off = nullptr;   // only for words uploaded with their positions (multi-term merge)
	uint32_t* range_off = nullptr; // [n_ranges]: first posting with doc >= k * kFtRangeDocs (ft_ranges finds its segment of the list here)
	uint32_t n_ranges = 0;
	uint32_t last_doc = 0;         // largest document id of the list: checked against total_docs when a merge uses the word
	uint64_t df = 0;               // document-range shards: the word's document frequency over the WHOLE index (this list is a fragment); 0: n
	uint64_t* fpos = nullptr;
	std::shared_ptr<void> pool;    // set for words decoded on the device (rxgpu_ft_set_words_packed): the arrays are slices of one allocation
	void release() {
		if (!pool) {
			for (void* p : {static_cast<void*>(doc), static_cast<void*>(ent_off), static_cast<void*>(ent_field), static_cast<void*>(ent_tf),
							static_cast<void*>(ent_first_pos), static_cast<void*>(pos_off), static_cast<void*>(fpos), static_cast<void*>(range_off)}) {
				if (p) (void)hipFree(p);
			}
		}
		*this = rxgpu_ft_word{};
	}
};

struct rxgpu_ft_shard_set;
struct rxgpu_ft_index {
	int device = 0;
	uint32_t num_fields = 0;
	uint64_t total_docs = 0;
	// Document-range shards (rxgpu_ft_create_sharded, SURVEY 8e "BM25").  The handle the caller holds owns the shards (shard_set); a shard is
	// an ordinary index over the GLOBAL document space that merges its own ranges only (sh_*: set by the sharded layer around every merge).
	rxgpu_ft_shard_set* shard_set = nullptr;
	uint32_t sh_range_begin = 0, sh_range_count = 0, sh_index = 0, sh_total = 0;
	const uint32_t* sh_hist = nullptr;   // every shard's folded histogram as gathered on this shard's device
	const uint32_t* sh_pos = nullptr;    // shard -> position in the gathered buffers
	float* d_words = nullptr;
	float* d_avg = nullptr;
	uint8_t* d_removed = nullptr;
	uint32_t* d_removed_bits = nullptr;   // the same as one bit per document (the sparse train, ft_sparse.hip); null: no document is removed
	std::vector<float> h_avg;             // avg_words as uploaded (the sparse train's eligibility test reads it)
	std::atomic<uint64_t> trains_dense{0}, trains_sparse{0};   // merges by launch train (rxgpu_ft_read_train_stats)
	std::unordered_map<uint32_t, rxgpu_ft_word> words;
	std::mutex mtx;
	// Concurrent merges (several planner threads query one index at a time): extra LANES — own stream, scratch, staging, events — behind
	// the same dictionary.  A lane is a rxgpu_ft_index whose `root` points at the handle that owns words and statistics; the handle
	// itself is lane 0 and the only one the resident / hybrid calls use.  Merges hold dict_mtx shared, dictionary updates exclusively.
	rxgpu_ft_index* root = nullptr;
	std::vector<std::unique_ptr<rxgpu_ft_index>> lanes;
	std::mutex lanes_mtx;
	std::shared_mutex dict_mtx;
	std::atomic<uint32_t> next_lane{0};
	// Q merges in ONE launch train (rxgpu_ft_merge_batch_raw): a scratch set per query of the batch (lanes without a stream of their own: the
	// whole train runs on batch_stream), the Q FtPlan structs back to back in HBM + their pinned staging, events around the train
	std::vector<std::unique_ptr<rxgpu_ft_index>> batch_lanes;
	std::mutex batch_mtx;
	hipStream_t batch_stream = nullptr;
	rxgpu_devbuf d_batch_plans;
	void* h_batch_plans = nullptr;
	hipEvent_t ev_ba = nullptr, ev_bb = nullptr;
	uint64_t batch_trains = 0, batch_merges = 0;
	const std::unordered_map<uint32_t, rxgpu_ft_word>& dict() const { return root ? root->words : words; }
	hipStream_t stream = nullptr;
	rxgpu_devbuf d_state, d_out;   // per-merge scratch (plan + tables) and the packed result
	rxgpu_devbuf d_excl;           // docsExcluded of the running merge
	rxgpu_devbuf d_areas;          // MergeDataAreas: per merged document and field {held, insertions} + the areas themselves
	rxgpu_devbuf d_pk_in, d_pk_cnt, d_pk_segs, d_pk_outs;   // rxgpu_ft_set_words_packed: streams + offsets, counts, pieces, slices (kept and grown)
	hipStream_t pk_streams[4] = {nullptr, nullptr, nullptr, nullptr};   // ... and the streams its chunked counting pass runs on (created on first use)
	std::vector<rxgpu_devbuf> d_phrase_a, d_phrase_b;   // per phrase of a query: plan + admission slots, workspace + the packed rows
	hipEvent_t ev_pha = nullptr, ev_phb = nullptr;      // around the phrase kernels
	// tables every merge finds ZEROED and leaves zeroed (the kernel that reads one last clears it): pre-score histogram, look-back words of
	// the preselect, bucket counters, synchronisation words, the occupancy (rank) plane of the entry rows.  Cleared by the host only when (re)allocated or after a failed merge.
	rxgpu_devbuf d_clean;
	uint64_t clean_docs = 0;
	bool clean_dirty = true;
	void* h_pinned = nullptr;     // staging: plan upload / result download
	size_t h_pinned_bytes = 0;
	hipEvent_t ev_a = nullptr, ev_b = nullptr;
	int ensure_pinned(size_t need) {
		if (need <= h_pinned_bytes) return RXGPU_OK;
		if (h_pinned) (void)hipHostFree(h_pinned);
		h_pinned = nullptr;
		h_pinned_bytes = 0;
		const size_t want = need + need / 2 + 4096;
		if (hipHostMalloc(&h_pinned, want, hipHostMallocDefault) != hipSuccess) {
			rxgpu::set_error("hipHostMalloc failed");
			return RXGPU_ERR_NOMEM;
		}
		h_pinned_bytes = want;
		return RXGPU_OK;
	}
	// a merge left in HBM for the hybrid fusion (rxgpu_ft_merge_*_resident): no export, no wait; checked by finish_pending()
	// The steps of one hybrid query (resident merge, prepare, fuse) each take `mtx` on their own, so the result is guarded by a SESSION: opened
	// by the resident merge for the calling thread, closed by that thread's fusion.  While it is open ordinary merges keep off this lane
	// (checkout_lane), other threads' resident merges wait on res_cv; a session nobody fuses is taken over after kResidentPatience and its
	// owner's later calls fail with RXGPU_ERR_LOGIC (generation mismatch) instead of reading another query's result.
	bool res_session = false;
	std::thread::id res_owner;
	uint64_t res_generation = 0;
	std::condition_variable res_cv;
	bool res_pending = false;
	bool res_has_syn = false;   // the resident merge had multi-word synonyms: its terms counters carry the 0xFFFF marks of the removed documents
	uint32_t res_cap = 0;          // max_merged of that merge (the packed layout of d_out depends on it)
	bool prep_done = false;        // hybrid_prepare_kernel has been enqueued behind that merge (with prep_sig's reranker / min_rank)
	double prep_sig[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	rxgpu_devbuf d_fuse;           // fusion scratch: radix ping-pong keys / classes
	hipEvent_t ev_knn = nullptr;   // orders the fusion behind the KNN search's stream
	hipEvent_t ev_fa = nullptr, ev_fb = nullptr;   // around the join kernel (rxgpu_hybrid_read_stats)
	hipEvent_t ev_pa = nullptr, ev_pb = nullptr;   // around the prepare kernel
	bool prep_timed = false;
	double prep_ms = 0.0;
	uint64_t fuse_calls = 0;
	double fuse_ms = 0.0;
	double fuse_stamps[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // RXGPU_FUSE_STAMPS: summed phase stamps of the fusion kernel (us since its first)
	double packed_wall_ms = 0.0;                            // rxgpu_ft_set_words_packed*: wall time inside the calls (rxgpu_ft_read_packed_wall)
	double packed_count_ms = 0.0, packed_write_ms = 0.0;   // rxgpu_ft_set_words_packed: device time of the two decode kernels ...
	uint64_t packed_bytes_in = 0, packed_bytes_out = 0;    // ... the stream bytes they read and the array bytes they wrote
	uint64_t stat_postings = 0;
	double stat_ms = 0.0;
	double stamps[64] = {};   // RXGPU_FT_STAMPS: summed phase stamps (relative to the workgroup's first), see rxgpu_ft_read_stats
	double trace_us[6] = {0, 0, 0, 0, 0, 0};   // RXGPU_FT_TRACE: plan build, staging + upload, launches, wait + download, unpack, merges
};

// ---------------------------------------------------------------------------------------------- document-range shards (SURVEY 8e "BM25")
// "Shard by doc-id range (each GPU holds the posting fragments of its docs; idf uses global N and df ...); exchange = ... the uint16 pre-score
// histogram for the global threshold".  The index is cut into contiguous runs of 8192-document ranges, one run per listed device (a device
// may repeat).  Every shard is an ordinary rxgpu_ft_index over the GLOBAL document space — the per-document statistics are replicated (a
// few bytes per document), the posting lists, the bulk, are split: a shard holds the fragment of every list that falls into its documents,
// with the whole list's length as document frequency — and runs the ordinary kernels over its own ranges.  The merge algorithm is
// range-parallel with three per-query facts that span the ranges; between the kernels exactly those travel, over RCCL when the library is
// there (one all-gather each; rccl_dyn.h), on the streams, without a host round trip:
//   behind ft_ranges   every shard's folded pre-score histogram + the popcount of its mask words  (266 KB per shard)
//                      -> the 2-phase gate and preselectMostRelevantDocs' threshold (mergerimpl.h:386-464, 486-490) are decided on the sums,
//                         the ties kept at the threshold score are handed out in document order = shard order
//   behind ft_adders   every shard's table of documents first met per (sub-term row, range)      (rows x ranges x 4 B per shard)
//                      -> the sum is the table of the whole index: the merge slot of every document (addDoc order, merger.h:161-180) and the
//                         cut at maxMergedDocs are the single index's
// so every shard writes its documents at their GLOBAL merge slots, and the caller's list is the slot-wise union: the single handle's result,
// bit for bit (tests/test_gpu_ft_sharded.py).  postProcessResults' maximum (merger.h:111-155) is taken by the host merger over that list.
struct rxgpu_ft_shard_set {
	std::vector<rxgpu_ft_index*> shards;
	std::vector<int> devices;
	uint32_t n_ranges = 0;                  // of the whole index; 0: rxgpu_ft_set_docs has not run
	uint32_t per = 0;                       // ranges per shard of the current cut (the last shard also takes what lies behind S * per)
	// the exchange: one RCCL rank per DISTINCT device, a device's shards are `slots` consecutive pieces of its rank's buffers
	uint32_t nranks = 0, slots = 0;
	std::vector<int> rank_dev;
	std::vector<uint32_t> shard_rank, shard_slot, pos;   // pos[s] = rank * slots + slot: where shard s lies in a gathered buffer
	std::shared_ptr<rxgpu::RcclCommSet> cs; // the process-wide communicators over rank_dev when the shards span several devices (rccl_dyn.h); else null
	bool host_exchange = false;             // RXGPU_SHARD_MERGE=host, or several devices without RCCL (note says why): the pieces travel through the host
	std::string note;
	std::vector<hipStream_t> rstream;       // per rank
	std::vector<hipEvent_t> ev_shard, ev_rank;
	std::vector<uint32_t*> d_pos;           // per rank: pos[] on the device
	std::vector<rxgpu_devbuf> d_send[2], d_recv[2];   // per rank; [0] histograms, [1] adder tables
	uint64_t collectives = 0, merges = 0;
};

namespace rxgpu {

// HIP event pair that cannot leak on an early error return
struct EventPair {
	hipEvent_t a = nullptr, b = nullptr;
	int create() {
		RX_HIP(hipEventCreate(&a));
		RX_HIP(hipEventCreate(&b));
		return RXGPU_OK;
	}
	float elapsed_ms() const {
		float ms = 0.f;
		(void)hipEventElapsedTime(&ms, a, b);
		return ms;
	}
	~EventPair() {
		if (a) (void)hipEventDestroy(a);
		if (b) (void)hipEventDestroy(b);
	}
};
template <typename T>
int upload(T*& dst, const T* src, size_t count) {
	if (dst) (void)hipFree(dst);
	dst = nullptr;
	if (!count) return RXGPU_OK;
	RX_HIP(hipMalloc(reinterpret_cast<void**>(&dst), count * sizeof(T)));
	RX_HIP(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
	return RXGPU_OK;
}
inline uint64_t word_df(const rxgpu_ft_word& w) { return w.df ? w.df : w.n; }

// A free lane for one merge, locked; then the dictionary, shared.  The first free one of: the handle itself, the lanes made so far, a new
// lane (up to RXGPU_FT_LANES, default 4); all busy: wait for one in turn.
struct LaneLock {
	rxgpu_ft_index* lane = nullptr;
	std::unique_lock<std::mutex> lk;
	std::shared_lock<std::shared_mutex> dict;
};

// A phrase between its admission pass and the rest (a document-range shard: the sharded layer settles the admission cut of the WHOLE index —
// at most mergeLimit documents in (row, document) order, phrasemerger.h:341 — before any shard goes on; finish_phrase)
struct PhraseCtx {
	rxgpu::FtPhrasePlan p{};
	std::vector<uint32_t> row_sub, shard_row_sub;
	std::vector<int32_t> shard_row_grid;
	std::vector<uint32_t> row_admitted;   // by the row numbering all shards share: documents this shard admitted for that row
	uint32_t n_rows0 = 0, n_ranges = 0, admitted = 0;
	uint64_t sum_caps = 0;
	size_t phrase_index = 0;
	bool shard = false;
};
// One phrase through ft_phrase.hip: the rows the main merge reads instead of words
struct PhraseRows {
	std::vector<rxgpu::FtPosSubterm> rows;   // non-empty rows, first-term sub-term order; device arrays live in the handle's phrase buffers
	uint32_t admitted = 0;                   // PhraseMerger::NumDocsMerged()
	uint32_t proc16 = 0;                     // PhraseResults::CalcProc16
	uint64_t postings = 0;                   // postings of the phrase's words (statistics)
	std::shared_ptr<PhraseCtx> pending;      // admission ran, finish_phrase has not yet (run_phrase(..., first_half_only))
};

// MergeDataAreas<Area>: what the caller wants back besides the merged documents (rxgpu_ft_merge_query_areas_raw)
struct AreasOut {
	uint32_t max_areas = 0;      // FTConfig::maxAreasInDoc
	uint32_t* cnt = nullptr;     // [cap][num_fields]
	uint32_t* areas = nullptr;   // [cap][num_fields][max_areas][3]
};

// One merge between the building of its plan and the unpacking of its result.
struct MergeJob {
	rxgpu::FtPlan p{};
	const rxgpu::FtPlan* d_plan = nullptr;   // the plan where the kernels read it (HBM, behind the rest of the plan)
	void* dev_base = nullptr;                // where the staged plan goes (the lane's state buffer)
	uint64_t max_merged = 0, merged_postings = 0;
	size_t plan_bytes = 0;
	void* hp_dev = nullptr;                  // the lane's pinned staging buffer as the device sees it
	uint32_t nsyn = 0;
	bool empty = false;                      // min(mergeLimit, totalORVids) == 0: nothing is merged
	size_t area_hdr_bytes = 0, area_bytes = 0;   // MergeDataAreas: the two regions of the lane's d_areas
};

// Where a merge's documents go: the caller's lists (terms_counter may be null for a Simple() query; all null: a resident merge)
struct MergeOut {
	uint32_t* doc = nullptr;
	float* proc = nullptr;
	uint8_t* field = nullptr;
	uint16_t* terms_counter = nullptr;
	uint64_t cap = 0;
	uint64_t* n = nullptr;
	int32_t* preselected = nullptr;   // may be null
	bool complete(bool simple) const { return doc && proc && field && (simple || terms_counter); }
};
// One query as the merge functions take it
struct MergeQuery {
	const rxgpu_ft_config* cfg = nullptr;
	bool simple = false;
	const std::vector<QueryTermIn>* terms = nullptr;
	const uint32_t* word_ids = nullptr;
	const float* procs = nullptr;
	const uint8_t* excluded = nullptr;
	const SynonymsIn* synonyms = nullptr;
	const AreasOut* areas = nullptr;
	const char* who = "";
	uint32_t max_areas() const { return areas ? areas->max_areas : 0u; }
};

// room in the caller's lists, as the plan's overflow check wants it
struct OutRoom {
	bool have_outs;
	uint64_t cap;
};

// ---- rxgpu_ft_capi.hip: the lanes
int make_lane(rxgpu_ft_index* h, bool stream, std::unique_ptr<rxgpu_ft_index>& out);
void lane_adopt_docs(rxgpu_ft_index* l, const rxgpu_ft_index* h);
int checkout_lane(rxgpu_ft_index* h, LaneLock& out);

// ---- rxgpu_ft_sharded.hip: the sharded handle's side of the dictionary calls, its end, its merge
int ft_shards_set_docs(rxgpu_ft_index* h, uint64_t total_docs, const float* words_in_field, const float* avg_words, const uint8_t* removed);
int ft_shards_set_word(rxgpu_ft_index* h, uint32_t word_id, uint64_t n, const uint32_t* doc, const uint32_t* ent_off, const uint8_t* ent_field,
					   const uint32_t* ent_tf, const uint32_t* ent_first_pos, const uint32_t* pos_off, const uint64_t* fpos);
void ft_shards_destroy(rxgpu_ft_shard_set* ss);
int run_merge_sharded(rxgpu_ft_index* parent, const MergeQuery& q, const MergeOut& out);

// ---- rxgpu_ft_phrase.hip
int run_phrase(rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const std::vector<QueryTermIn>& terms, const QueryPartIn& part, const uint32_t* word_ids,
			   const float* procs, const uint8_t* d_excluded, size_t phrase_index, PhraseRows& out, const char* who, bool first_half_only = false);
int finish_phrase(rxgpu_ft_index* h, const float* procs, PhraseCtx& c, PhraseRows& out, const char* who);

// ---- rxgpu_ft_merge.hip: what a phrase stages like a merge does
int plan_error(const FtPlanError& e);
void fill_term_cfg(FtTermCfg& tc, const rxgpu_ft_index* h, const rxgpu_ft_config* cfg, const QueryTermIn& qt, bool same, bool all_pos);
void stage_field_cfg(float* fc, const rxgpu_ft_config* cfg, uint32_t nf);
void point_term_cfg(FtTermCfg& tc, const float* d_fc, const float* d_field_boost, const uint8_t* d_need_sum, uint32_t nf);
FtPosSubterm word_subterm(const rxgpu_ft_word& w, int bm25_type, uint64_t N, float proc);
// ... the resident session (the thread's view of it lives in that unit), results and waits
void open_resident_session(rxgpu_ft_index* h, std::unique_lock<std::mutex>& lk);
int check_resident_session(rxgpu_ft_index* h, std::unique_lock<std::mutex>& lk, const char* who);
void close_resident_session(rxgpu_ft_index* h);
int check_result_header(const uint32_t* hdr, uint64_t max_merged, const char* who);
int wait_stream_polled(hipStream_t st);
int settle_resident_merge(rxgpu_ft_index* h, const char* who);
int finish_pending(rxgpu_ft_index* h, const char* who);
std::atomic<int>* ft_train_mode();
// ... and the merge itself, whole or in the halves the batch train and the shards drive
int prepare_merge(rxgpu_ft_index* h, hipStream_t st, const MergeQuery& q, bool resident, OutRoom room, MergeJob& job, bool import_now);
int prepare_shard_phrases(rxgpu_ft_index* h, const MergeQuery& q, std::vector<PhraseRows>& phrases, bool* empty);
int prepare_shard_merge(rxgpu_ft_index* h, const MergeQuery& q, const std::vector<PhraseRows>* phrases, MergeJob& job);
int collect_merge(rxgpu_ft_index* h, const MergeJob& job, const MergeOut& out, const char* who);
int run_merge(rxgpu_ft_index* h, const MergeQuery& q, const MergeOut& out, bool resident = false);

}  // namespace rxgpu
