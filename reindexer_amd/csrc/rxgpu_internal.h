// Internal declarations shared by the C-ABI implementation and the kernel translation units.
#pragma once

#include <atomic>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <thread>
#include <mutex>
#include <string>
#include <vector>
#include "ft_packed_decode.h"
#include "ft_merge_plan.h"   // the FT constants the host decisions share with the kernels, FtGridEntry, FtSynonym

namespace rxgpu {

struct ScanParams;

// ---- knn_scan.hip: the streaming f32 scans (every row; a row list) and the bf16 scan over the shadow
uint32_t scan_grid_x(uint64_t n, int cus);
void launch_scan(int metric, const ScanParams& p, uint32_t nq, uint32_t gridx, hipStream_t s);
struct ScanBf16Params;
bool scan_bf16_supported(uint32_t ld);
uint32_t scan_bf16_grid_x(uint64_t n, int cus);
void launch_scan_bf16(int metric, const ScanBf16Params& p, uint32_t nq, uint32_t gridx, hipStream_t s);
// pre-filtered search: knn_scan_subset over a strictly increasing row list (knn_subset.hip below makes one from a bitmap)
uint32_t subset_grid_x(uint64_t n_ids, uint32_t dim, uint32_t kk, int cus);
void launch_scan_subset(int metric, const ScanParams& p, const uint32_t* ids, uint32_t nq, uint32_t gridx, int cus, hipStream_t s);

// ---- knn_scan_i8.hip, knn_scan_i6.hip: the pruning scans over the int8 and 6-bit shadows
struct ScanI8Params;   // int8-pruned scan (knn_scan_i8.hip; the query side: knn_query_prep_i8 in knn_batched.hip)
uint32_t scan_i8_grid_x(uint64_t n, int cus);
struct ScanI8Emit;     // its emitting form (knn_emit_plan.h): null = lo of every row into p.lower and nothing emitted; keep: p.lower is written as well
void launch_scan_i8(int metric, const ScanI8Params& p, uint32_t nq, uint32_t gridx, hipStream_t s, const ScanI8Emit* emit = nullptr, bool keep = true);
// the gather form over a row list: p.sp.n = list entries, p.lower [nq][n_ids] by list position; gridx MUST come from scan_i8_subset_grid_x
uint32_t scan_i8_subset_grid_x(uint64_t n_ids, int cus);
void launch_scan_i8_subset(int metric, const ScanI8Params& p, const uint32_t* ids, uint32_t nq, uint32_t gridx, int cus, hipStream_t s);
void launch_i8_build(const float* rows, const float* inv_norms, uint64_t n, uint32_t stride, uint32_t dim, int8_t* codes, float2* side, uint32_t ld8,
					 unsigned int* stats, int cus, hipStream_t s);   // every pointer at the first row of the range
// estats: the residual maxima the margin takes, {max e^2, max (e inv_norm)^2, non-finite flag}; null = the int8 shadow's (stats[3], stats[4]; its flag is stats[2])
void launch_query_prep_i8(int metric, const float* src, uint32_t nq, uint32_t dim, float* qpad, int8_t* planes, uint32_t ld8, const unsigned int* stats,
						  float* q_sq, float* margin, float2* qinfo, uint32_t* cand_cnt, uint32_t cap, hipStream_t s, const unsigned int* estats = nullptr);
// the 6-bit front of the int8-pruned chain (knn_scan_i6.hip, knn_i6_quant.h): seed pass (emit null) and full pass of one kernel
struct ScanI6Params;
uint32_t scan_i6_seed_step(uint64_t n);
uint32_t scan_i6_grid_x(uint64_t n, uint32_t set_step, int cus);
void launch_scan_i6(int metric, const ScanI6Params& p, uint32_t nq, uint32_t gridx, hipStream_t s, const ScanI8Emit* emit, bool keep);
void launch_i6_build(const float* rows, const float* inv_norms, uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim, uint8_t* codes, float2* side,
					 uint32_t ld6, unsigned int* stats6, int cus, hipStream_t s);   // every pointer at row 0 of the index
void launch_i6_copy_row(uint8_t* codes, uint32_t ld6, uint64_t from, uint64_t to, hipStream_t s);   // from == ~0: zeros over row `to`
// range search from the int8 shadow, one query: the pruning scan (ids null = every row, else p.sp.n list entries); its exact tail over the
// candidates it left is launch_range_rescore (knn_range.hip)
struct RangeI8Cand;
void launch_range_i8(int metric, const ScanI8Params& p, const RangeI8Cand& c, const uint32_t* ids, int cus, hipStream_t s);

// ---- knn_filter.hip: the candidate filters of the pruned chains, one threshold (top_dist[kk - 1] + margin; a query without a finite margin is left alone)
void launch_filter_approx(const float* approx, uint64_t n, const float* top_dist, const uint32_t* top_count, uint32_t kk, const float* margin,
						  uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus, hipStream_t s,
						  const uint32_t* ids = nullptr);   // ids: approx is indexed by list position and the candidates are ids[position]
struct EmitEntry;
struct EmitPlan;
void launch_filter_emitted(const EmitEntry* emit, const uint32_t* emit_cnt, const EmitPlan& plan, const float* top_dist, const uint32_t* top_count, uint32_t kk,
						   const float* margin, uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus,
						   hipStream_t s);   // launch_filter_approx over what knn_scan_i8 emitted
void launch_filter_emitted_wide(const EmitEntry* emit, const uint32_t* emit_cnt, const EmitPlan& plan, const float* top_dist, const uint32_t* top_count,
								uint32_t kk, const float* margin, uint32_t* cand_row, uint32_t* cand_cnt, uint32_t cap, uint32_t nq, int cus,
								hipStream_t s);   // the same candidate set with one atomic per workgroup: for the thousands of candidates behind knn_scan_i6

// ---- knn_merge.hip: the top-k merges
// the insertion merge over total_per_query unsorted pairs.  Precondition: kk <= kMaxFusedK (the batched tail is reached with no more,
// rxgpu_knn_merge_probe refuses more); sorted lists of any kk <= kMaxFusedK2 go through launch_merge_lists
void launch_merge(const float* part_dist, const uint32_t* part_row, uint32_t total_per_query, uint32_t kk, uint32_t nq, float* out_dist,
				  uint32_t* out_row, uint32_t* out_count, const uint32_t* gate_cnt, uint32_t gate_cap, hipStream_t s);
void launch_merge_lists(const float* part_dist, const uint32_t* part_row, uint32_t nlists, uint32_t kk, uint32_t nq, float* out_dist, uint32_t* out_row,
						uint32_t* out_count, hipStream_t s, const uint32_t* gate_cnt = nullptr, uint32_t gate_cap = 0,
						uint32_t* path = nullptr);   // the partial results are sorted lists of kk entries: no serial insertions; gated like launch_merge
// the one merge at the end of a pruned chain: per query the cand_cnt re-scored candidates (cand_cnt <= cap), else the exact scan's sorted lists
// path (both; rxgpu_knn_merge_probe): [nq] words, 1 where a selection answered the query, 0 where an insertion merge did
void launch_merge_final(const float* cand_dist, const uint32_t* cand_row, const uint32_t* cand_cnt, uint32_t cap, const float* part_dist,
						const uint32_t* part_row, uint32_t nlists, uint32_t kk, uint32_t nq, float* out_dist, uint32_t* out_row, uint32_t* out_count,
						hipStream_t s, uint32_t* path = nullptr);
void launch_merge_shards(const uint32_t* gathered, uint32_t world, uint32_t nq, uint32_t kk, uint32_t shard_rows, float* out_dist,
						 uint32_t* out_row, uint32_t* out_count, hipStream_t s, const uint32_t* slot_base = nullptr, bool sorted = true);
// one shard's HNSW result (unordered, counts <= k) into its [nq][kk] | [nq][kk] slot of the exchange's send buffer, padded with invalid entries
void launch_pack_lists(const float* dist, const uint32_t* row, const uint32_t* count, uint32_t nq, uint32_t k, uint32_t kk, uint32_t* dst_dist, uint32_t* dst_row,
					   hipStream_t s);

// ---- knn_range.hip: range search and explicit-row distances over the f32 rows (one body for the three range forms)
void launch_range(int metric, const float* rows, const float* inv_norms, const float* query, uint64_t n, uint32_t stride, uint32_t dim,
				  float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap, unsigned long long* counter,
				  uint32_t gridx, hipStream_t s);
void launch_range_subset(int metric, const float* rows, const float* inv_norms, const float* query, const uint32_t* ids, uint64_t n_ids,
						 uint32_t stride, uint32_t dim, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
						 unsigned long long* counter, uint32_t gridx, hipStream_t s);
void launch_distances(int metric, const float* rows, const float* inv_norms, const float* query, uint32_t stride, uint32_t dim,
					  const uint32_t* ids, uint32_t n, float* out, hipStream_t s);
// the exact tail of launch_range_i8 over the candidates it left: does nothing when there are more than ccap (or none)
void launch_range_rescore(int metric, const float* rows, const float* inv_norms, const float* query, const uint32_t* cand_cnt, const uint32_t* cand_row,
						  uint32_t ccap, uint32_t stride, uint32_t dim, float radius, int inclusive, float* out_dist, uint32_t* out_row, uint64_t cap,
						  unsigned long long* counter, uint32_t gridx, hipStream_t s);

// ---- knn_subset.hip: pre-filtered search, bitmap -> the row list launch_scan_subset walks
uint32_t bitmap_tiles(uint64_t n_rows);
void launch_bitmap_count(const uint32_t* words, uint64_t n_rows, uint32_t* tile_scratch, unsigned long long* total, hipStream_t s);
void launch_bitmap_expand(const uint32_t* words, uint64_t n_rows, const uint32_t* tile_scratch, uint32_t* out_rows, uint64_t cap, hipStream_t s);
void launch_ivf_mark_lists(const uint32_t* probe, const uint32_t* probe_cnt, uint32_t nprobe, const uint64_t* list_off, const uint32_t* list_rows,
						   uint32_t* bitmap, hipStream_t s);
void launch_gather_u32(const uint32_t* src, const uint32_t* idx, uint32_t n, uint32_t* out, hipStream_t s);
void launch_check_row_list(const uint32_t* ids, uint64_t n, uint64_t limit, uint32_t* bad, int cus, hipStream_t s);

// ---- knn_lists.hip: the list scan of a batched IVF search (layout and chunk rule: ivf_batch_plan.h)
void launch_ivf_batch_offsets(const uint32_t* probe, const uint32_t* probe_cnt, const uint64_t* list_off, uint32_t nprobe, uint32_t nq, uint32_t* cum,
							  unsigned long long* scanned, hipStream_t s);   // running chunk counts [nq][nprobe + 1] and rows probed [nq]
void launch_scan_lists(int metric, const ScanParams& p, const uint32_t* probe, const uint32_t* cum, const uint64_t* list_off, const uint32_t* list_rows,
					   uint32_t nprobe, uint32_t nq, uint32_t gridx, hipStream_t s);   // partial lists [nq][gridx][kk], every slot written

// IVF training on the device (ivf_train.hip; layout: ivf_train_plan.h).  ids: list positions -> rows in HBM, or null: position i is row first_row + i
void launch_ivf_gather(int metric, const float* rows, const float* inv_norms, const uint32_t* ids, uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim,
					   float* out, int cus, hipStream_t s);   // prepared vectors [n][dim]: row[j], cosine row[j] * inv_norms[row]
void launch_ivf_place(const uint32_t* assign, const uint32_t* ids, uint32_t n, uint32_t nlist, uint32_t* table, uint32_t* seg_off, uint32_t* seg_rows, float* hassign,
					  uint32_t* flag, hipStream_t s);   // stable per-centroid segments of the members' rows; table and flag zeroed by the caller
void launch_ivf_centroid_sums(int metric, const float* rows, const float* inv_norms, uint32_t stride, uint32_t dim, uint32_t nlist, const uint32_t* seg_off,
							  const uint32_t* seg_rows, float* centroids, hipStream_t s);   // compute_centroids' ordered sums x 1 / count

// Large-k path (k+1 > 64): distance pass + radix select (knn_select.hip).
void launch_all_distances(int metric, const float* rows, const float* inv_norms, const float* query, uint64_t n, uint32_t stride,
						  uint32_t dim, float* out_dist, uint32_t gridx, hipStream_t s);
size_t select_scratch_bytes(uint64_t n);
// Finds the kk smallest (dist,row) of d_dist[0..n) ; writes them UNSORTED to d_out_*; *d_out_n (device) = count (== min(kk,n)).
void launch_select_smallest(const float* d_dist, uint64_t n, uint32_t kk, void* d_scratch, float* d_out_dist, uint32_t* d_out_row,
							hipStream_t s);

// Batched (MFMA) path, knn_batched.hip
struct GemmParams;
size_t gemm_lds_bytes(int mt);
hipError_t launch_gemm(int metric, int mt, int mode, const GemmParams& p, uint32_t grid, hipStream_t s);
void launch_row_stats(const float* rows, const float* inv_norms, uint64_t n, uint32_t stride, uint32_t dim, float* row_sq,
					  unsigned int* stats, int cus, hipStream_t s);
void launch_query_stats(int metric, const float* queries, uint32_t nq, uint32_t mt, uint32_t q_stride, uint32_t dim, const unsigned int* stats,
						float* q_sq, float* margin, bool bf16, hipStream_t s);
void launch_query_prep(int metric, const float* src, uint32_t nq, uint32_t dim, float* qpad, uint32_t ld, const unsigned int* stats, float* q_sq,
					   float* margin, uint32_t* cand_cnt, uint32_t cap, hipStream_t s);   // the pruned scan's query side in one launch
struct GemmBf16Params;
hipError_t launch_gemm_bf16(int metric, int mode, int qt, const GemmBf16Params& p, uint32_t grid, hipStream_t s);
void launch_to_bf16(const float* src, uint64_t n, uint32_t stride, uint32_t dim, uint16_t* dst, uint32_t ld, int cus, hipStream_t s, uint64_t first_row = 0,
					bool blocked = false);   // dst = the shadow's base when first_row / blocked are given
void launch_shadow_move(uint16_t* shadow, uint32_t ld, uint64_t from, uint64_t to, bool blocked, hipStream_t s);
void launch_sample_threshold(const float* dense, uint64_t ns, uint32_t nq, uint32_t mt, uint32_t kk, const float* margin, float* thr,
							 hipStream_t s);
void launch_rescore(int metric, const float* rows, const float* inv_norms, const float* queries, uint32_t q_stride, uint32_t stride,
					uint32_t dim, uint32_t nq, uint32_t cap, const uint32_t* cand_cnt, uint32_t* cand_row, float* cand_dist, hipStream_t s);

// HNSW search (hnsw_search.hip)
struct HnswParams;
void launch_hnsw_search(int metric, const HnswParams& p, uint32_t blocks, bool global_cand, hipStream_t s);
// the same launch for a call under an allowed-rows bitmap (p.allowed set, p.bare 0): the kernels of hnsw_filtered.hip
struct HnswFilteredParams;
void launch_hnsw_filtered(int metric, const HnswFilteredParams& p, uint32_t blocks, bool global_cand, hipStream_t s);
struct HnswHelper;
void launch_hnsw_helper(int metric, const HnswParams& p, const HnswHelper& hq, uint32_t groups, hipStream_t s);
struct HnswServer;
// the resident search kernel (one workgroup per mailbox slot); false: this (metric, dim, list size, deleted nodes) has no resident form
bool launch_hnsw_server(int metric, const HnswParams& p, const HnswServer& sv, uint32_t slots, hipStream_t s);
size_t hnsw_server_lds_bytes(const HnswParams& p);
bool hnsw_server_sq8_serves(uint32_t dim, bool bare);   // the resident kernel over SQ8 codes exists for this embedding size
struct HnswPatch;
void launch_hnsw_patch(const HnswPatch& p, uint32_t n_dirty, hipStream_t s);
// Quantizer::quantize on the device (hnsw_sq8_quantize.hip): codes [..][dim] and corrective offsets of rows [first_row, first_row + n)
void launch_hnsw_sq8_quantize(int metric, const float* rows, uint32_t stride, uint32_t dim, uint64_t first_row, uint64_t n, float min_q, float alpha,
							  float delta, uint8_t* codes, float* corr, hipStream_t s);
struct HnswStream;
void launch_hnsw_stream(int metric, const HnswParams& p, const HnswStream& s, uint32_t batch, int mode, bool lds, hipStream_t st);
// a whole collection under an allowed-rows bitmap in one launch (hnsw_stream_collect.hip); mode: kCollectFresh / kCollectResume / kCollectBegin
struct HnswStreamCollect;
void launch_hnsw_stream_collect(int metric, const HnswParams& p, const HnswStream& s, const HnswStreamCollect& c, int mode, bool lds, hipStream_t st);
struct HnswRange;
void launch_hnsw_range(int metric, const HnswParams& p, const HnswRange& r, hipStream_t s);

// Hybrid FT + KNN rank fusion on the device (hybrid_fuse.hip)
constexpr int kMaxFuseKnn = 1024;      // KNN entries one fusion takes (k of the KNN condition)
// what hybrid_prepare_kernel leaves in HBM for hybrid_join_kernel, next to the FT documents in their final mutual order
struct HybridFuseState {
	uint32_t n_valid;            // documents that passed postProcessResults = entries of the prepared list
	uint32_t max_id;
	uint32_t result_in_second;   // which half of the scratch arrays holds the prepared list
	uint32_t pad;
	uint32_t cls_pos[256];       // RRF position of a rank class
	uint32_t cls_key[256];       // fused rank of an FT-only document of the class, as an order key (smaller = earlier)
	float cls_rank[256];         // ... and as the float that is returned
	uint32_t cls_group[256];     // classes with equal fused ranks share a group
	uint32_t grp_key[256];       // key of group g (0xFFFFFFFF: unused)
	uint32_t grp_start[260];     // first prepared position of group g; [256] = n_valid
};
struct HybridFuseArgs {
	// FT side.  Either the merge train's raw output (ft_doc + ft_proc: postProcessResults is applied here with min_rank) or documents with
	// their uint8 ranks (ft_doc + ft_rank_u8).  Ids unique, any order.  ft_count_ptr (device) overrides ft_n when set.
	const uint32_t* ft_doc;
	const float* ft_proc;
	const uint8_t* ft_rank_u8;
	const uint32_t* ft_count_ptr;
	const uint16_t* ft_terms;          // optional (raw merge output of a query with multi-word synonyms): 0xFFFF marks a document that holds only
	                                   // parts of a synonym — removed before postProcessResults (mergerimpl.h:533-555), i.e. absent here
	uint32_t ft_n, ft_cap;             // ft_cap: what the scratch arrays hold
	float min_rank;
	const int32_t* row_of_doc;         // vdoc -> row id (1:1), or null: the document number is the row id
	// KNN side: the search's (dist, row) list, best first
	const float* knn_dist;
	const uint32_t* knn_row;
	const uint32_t* knn_count_ptr;     // device count of valid entries, or null: knn_n
	uint32_t knn_n, k;                 // entries present / entries that take part (the list holds k + 1 when the caller checks boundary ties)
	int32_t knn_negate;                // IP / cosine: the planner's rank is -distance (hnsw_index.cc:261-270)
	int32_t metric_l2;                 // runs of equal KNN ranks: L2 ascends, IP / cosine descend
	const int32_t* rowid_of_row;       // internal row -> row id, or null: identity
	// reranker: kind 0 RRF (params[0] = rank_const), 1 linear (kKnn, knnDefault, kFt, ftDefault, c)
	int32_t kind, is_union, desc;
	double params[5];
	int32_t* out_ids;
	float* out_ranks;
	uint32_t* out_header;              // [0] count, [1] flags (1: distance tie at the k-th place), [2] head size, [3] tail size
	unsigned long long* dbg;           // phase stamps of the join kernel (100 MHz wall clock), 8 words, or null
	HybridFuseState* state;
	uint32_t* scratch_key;             // [2 * ft_cap]
	uint16_t* scratch_cls;             // [2 * ft_cap]
};
hipError_t launch_hybrid_prepare(const HybridFuseArgs& a, hipStream_t st);   // FT only: may run while the KNN search is still going
hipError_t launch_hybrid_join(const HybridFuseArgs& a, hipStream_t st);      // needs both halves

// ft_fast merge (ft_merge.hip and the units of its kernels): Merger::mergeSimple / mergeTerm + restricting bitmask + preselect, restated ORDER-FREE so that a whole
// query is a fixed number of launches (see the header of ft_merge.hip)
struct FtPosSubterm {
	uint64_t n;
	const uint32_t* doc;
	const uint32_t* ent_off;
	const uint8_t* ent_field;
	const uint32_t* ent_tf;
	const uint32_t* ent_first_pos;
	const uint32_t* pos_off;   // [n + 1]; null for words uploaded without positions (single-term merge only)
	const uint64_t* fpos;      // PosType words (idrelset.h:14-32): pos | arrayIdx << 28 | field << 56
	double idf;                // the calculator's IDF for this sub-term (bm25.h), computed on the host
	float proc;
	uint32_t term;             // query term index -> FtPlan::terms
	uint16_t qp;               // 1-based index among the terms that are not NOT (mergeTerm's qpIdx); 0 for a NOT term
	uint16_t ord_in_term;      // position inside its term (SortSubterms order)
	uint32_t row;              // row of the per-slot entry table = index among the merged (non-NOT, non-empty) sub-terms
	const uint32_t* range_off; // [n_ranges + 1]: first posting with doc >= k * kFtRangeDocs (built when the word is uploaded)
	uint32_t n_ranges;
	// A row of a merged PHRASE (ft_phrase.hip): the documents one sub-term of the phrase's first term added to the PhraseMerger, with their
	// phrase rank / field (what mergePhrase reads, mergerimpl.h:39-90) instead of entries; fpos = lastPhrasePositions.  Null for a word.
	const float* pre_rank;
	const uint8_t* pre_field;
	uint16_t prev_term_qp;     // phrase row: qp of the last plain term in front of the phrase (0: none) — the last switchToNextWord before it
	uint8_t phrase;            // 1: phrase row
	uint8_t suppressed;        // SubtermResults::Suppressed() (querymergedata.h:32, set by SupressDuplicatesInSynonyms :221-241): the sub-term of a
	                           // multi-word synonym is a word the query's own terms found already — its postings only count terms (mergerimpl.h:144-151)
};
constexpr uint32_t kFtSuppressedRank = 0x7FC00001u;   // rank bits of a suppressed sub-term's record (a NaN: never a rank, never 0)
// (qp, phrase flag, prev_term_qp) of a row as the replay carries it
__host__ __device__ inline uint32_t ft_row_qpw(const FtPosSubterm& s) { return uint32_t(s.qp) | (uint32_t(s.phrase) << 15) | (uint32_t(s.prev_term_qp) << 16); }
struct FtTermCfg {             // what calcTermRank reads: FTConfig + the FtDslOpts of ONE query term
	uint32_t num_fields;
	int32_t bm25_type;         // kFtBm25Rx / Classic / WordCount (ft_rank.hip.h)
	const float* words;
	const float* avg_words;
	double k1, b, summation_ratio;
	float opts_boost, term_len_boost_in;
	const float* field_boost;
	const uint8_t* need_sum_rank;
	const float *bm25_boost, *bm25_weight, *term_len_boost, *term_len_weight, *position_boost, *position_weight;
	int32_t op;                // 1 OR, 2 AND, 3 NOT
	uint32_t sub_begin, sub_end; // the term's (non-empty) sub-terms in FtPlan::subs, in SortSubterms order
	uint8_t same_boost;        // every field has the same boost (calcTermScores' shortcut)
	uint8_t all_pos_boost;     // every field has a non-zero boost (calcTermBitmask's shortcut)
	uint8_t phrase;            // the part is a phrase: its sub-terms are the rows ft_phrase.hip produced; field_boost = ones
	uint8_t pad0;
	uint32_t phrase_proc16;    // PhraseResults::CalcProc16 (querymergedata.h:117-127): what GetMergedDocsScore adds (phrasemerger.h:326-333)
	// an AND part with multi-word synonyms (PhraseOrTerm::SynonymsIds): the documents that hold EVERY term of one of them, as a bitmap over
	// the documents — OR-ed into the part's term mask before it restricts (buildRestrictingBitmask, mergerimpl.h:347-361); ft_syn_masks
	const uint32_t* syn_mask;
};
struct FtSynMaskJob {                // one AND part's synonym mask
	uint32_t syn_begin, syn_end;     // into FtPlan::job_syns
	uint32_t* out;                   // [nwords]
};
// (FtSynonym, FtGridEntry, kFtPassItems, kFtRangeDocs, kFtBlockPostings, ft_pass_blocks: ft_merge_plan.h)

// Everything one merge needs on the device.  Pointers into per-index scratch; scalar members by value (the struct travels as a kernel argument).
struct FtPlan {
	const FtPosSubterm* subs;
	const FtTermCfg* terms;
	const FtGridEntry* merge_grid;   // merged sub-terms in (term, sub-term) order
	uint32_t n_merge_entries, merge_blocks;
	uint32_t nterms, n_rows, n_subs;   // nterms = entries of `terms`: the query parts (a phrase is one part), then the synonyms' terms
	uint32_t n_parts;                  // queryParts.size()
	uint32_t n_part_qp;                // qp of the last merged query part: documents created behind it are the synonyms' (mergerimpl.h:510)
	const FtSynonym* syns;             // [n_syn]
	uint32_t n_syn;
	const FtSynMaskJob* syn_jobs;      // [n_syn_jobs] -> ft_syn_masks
	const uint32_t* job_syns;
	uint32_t n_syn_jobs;
	uint32_t query_len;                // QueryMergeData::QueryLength(): the terms inside phrases counted one by one (addFullMatchBoost)
	uint64_t total_docs, nwords;
	uint32_t max_merged, merge_limit;
	uint8_t simple;            // Merger::mergeSimple (one term): max over sub-terms, first maximum wins; no positions
	uint8_t prescore;          // the host-side half of the 2-phase gate held: pre-scores are collected, the device decides on popcount
	uint8_t check_removed;
	float distance_weight, distance_boost;
	double full_match_boost;   // FTConfig::fullMatchBoost, applied by ft_replay (addFullMatchBoost)
	const uint8_t* removed;
	const uint8_t* excluded;
	uint32_t* mask;            // restrictingMask_ [nwords]
	uint16_t* score;           // [total_docs]
	// pre-score histogram in kFtHistCopies interleaved copies (workgroup b of ft_ranges adds to copy b % kFtHistCopies; the reader sums them):
	// every workgroup holds the same handful of scores, and same-address device atomics are served one at a time.
	// Copy c = hist + c * kFtHistStride: [65536] documents per pre-score, then [1024] documents per chunk of 64 scores.
	uint32_t* hist;
	// admission (ft_rank_all -> ft_adders -> ft_finish): the eligible postings with a non-zero rank, bucketed by document range
	uint4* b_rec;              // [merged postings] records {doc, posting index, rank bits, row | field << 16}; bucket r starts at bucket_off[r]
	uint32_t* bucket_off;      // [n_ranges] = merged postings in front of the range (sum of the sub-terms' range offsets), written by ft_ranges
	uint32_t* bucket_cnt;      // [n_ranges] records in the bucket; kept zero between merges (ft_finish clears its own)
	uint32_t* adders;          // [n_rows][n_ranges]: documents first met in (sub-term row, range); then its exclusive prefix in place = slot bases
	uint32_t n_ranges;
	float* e_rank;             // per-slot entry table [n_rows][max_merged]: 0 = the document has no posting in that sub-term
	uint32_t* e_idx;
	uint8_t* e_field;
	unsigned long long* dbg;   // RXGPU_FT_STAMPS=<workgroup>: wall-clock stamps of that workgroup's phases (null otherwise)
	uint32_t dbg_block;
	uint32_t* sync;            // kFtSync* words; kept zero between merges (the last workgroup of ft_finish clears them)
	unsigned long long* lookback_pre;     // [ft_apply_blocks(nwords)] (ft_merge_plan.h): one word per workgroup of ft_preselect_apply
	// packed result: header (4 x u32: numDocs, error flag, preselected, 0) then doc[max_merged] u32, proc[max_merged] f32,
	// terms_counter[max_merged] u16, field[max_merged] u8 — one D2H copy
	uint32_t* out_header;
	void* host_out;            // device-visible address of the caller's pinned staging buffer: ft_export copies the used part of the result there
	uint32_t* out_doc;
	float* out_proc;
	uint16_t* out_terms_counter;
	uint8_t* out_field;
	// MergeDataAreas<Area> (merger.h:39-41, 182-204; areaholder.h:56-155): the highlight / snippet areas of every merged document, built by the
	// replay from the positions of the document's postings in merge order.  max_areas = FTConfig::maxAreasInDoc (> 0), 0: no areas.
	// area_hdr [max_merged][area_fields][2] = {entries held (AreasInField::data_.size()), insertions so far (index_)}, zeroed by the host in
	// front of the train; out_areas [max_merged][area_fields][max_areas][3] = {start, end, arrayIdx} in data_ order.
	uint32_t max_areas, area_fields;
	uint32_t* area_hdr;
	uint32_t* out_areas;
	// Document-range shards (SURVEY 8e "BM25", rxgpu_ft_sharded.hip): this handle merges the documents of the ranges [range_begin,
	// range_begin + range_count) only — its posting lists hold just those documents' fragments (global ids; idf from the global N / df) — and
	// the three per-query facts that span the shards travel between the kernels: the pre-score histogram + mask popcount (behind ft_ranges;
	// shard_hist = every shard's folded histogram, [n_shards][kFtFoldWords]: the sum is the threshold's input, the entries of the shards in
	// front give the tie quota already used at the threshold score), and the table of ft_adders (every shard fills its own columns, the
	// sum is the global table the slot bases come from).  range_count == 0: the whole index (unsharded).
	uint32_t range_begin, range_count;
	uint32_t shard_index, n_shards;
	const uint32_t* shard_hist;   // gathered layout: shard s at [shard_pos[s]][kFtFoldWords]
	const uint32_t* shard_pos;    // [n_shards]
	// The train for SPARSELY hit document ranges (ft_sparse.hip): one wavefront per (query, range), bitmaps of the range's documents per
	// sub-term in LDS, nothing per document in HBM.  sparse = 1: the host found the query eligible (ft_sparse_eligible, ft_merge_plan.h).
	uint8_t sparse;
	uint8_t sp_empty_and;         // an AND term without postings: no document passes the mask
	const uint32_t* removed_bits; // [nwords] DocRemoved as one bit per document (null: none removed); built by rxgpu_ft_set_docs
	const uint32_t* excluded_bits;// [nwords] docsExcluded of this merge as bits (null: none)
	unsigned long long* lb_units; // [n_ranges] look-back words of ft_sp_select's ordered tie count; kept zero between merges
	// the merged documents as ft_sp_select / ft_sp_place found them, one task each, replayed by ft_sp_replay:
	//   t_doc [max_merged] document; t_pos [max_merged] its slot | 1 << 31, or merge row << 24 | rank among the (row, range)'s documents;
	//   t_idx [max_merged][n_rows] posting index + 1 of the document in sub-term row r, 0: none
	uint32_t* t_doc;
	uint32_t* t_pos;
	uint32_t* t_idx;
	struct SpSub {                // what the unit kernels read of sub-term si (lane si loads entry si)
		const uint32_t* doc;
		const uint32_t* range_off;
		uint32_t n, n_ranges;
		uint32_t attr;            // proc16 | first sub-term of its term << 16 | AND term << 17 | NOT term << 18 | merge row << 20
		uint32_t pad;
	} sp_sub[16];
};
static_assert(sizeof(FtPlan::SpSub) == 32, "one 32-byte entry per lane");
constexpr uint32_t kFtFoldWords = 65536 + 1024 + 64;   // one shard's folded histogram (fine + chunk counters), [65536 + 1024] = its mask popcount
enum : uint32_t { kFtSyncError = 0, kFtSyncPop = 1, kFtSyncPreTicket = 4, kFtSyncNumDocs = 6, kFtSyncDoneFinish = 9,
				  // the sparse train: threshold score / documents kept at it / flags (bit 0 preselect on, bit 1 every tie is kept), the ticket of ft_sp_select
				  kFtSyncThrScore = 10, kFtSyncThrDocs = 11, kFtSyncThrFlags = 12, kFtSyncSpTicket = 13, kFtSyncTasks = 14 };   // (their count, kFtSyncWords: ft_merge_plan.h)
constexpr uint32_t kFtRangeShift = 13;     // log2(kFtRangeDocs)
static_assert((1u << kFtRangeShift) == kFtRangeDocs, "document ranges are powers of two");
// Q merges over one index in ONE train (grid.y = query; a single merge is a batch of one): the plans in HBM + their host copy
hipError_t launch_ft_merge(const FtPlan* plans, const FtPlan* host_plans, uint32_t nq, hipStream_t st);
// the same train in the three pieces a sharded merge exchanges between: 0 = [syn masks] + ft_ranges, 1 = [ft_preselect_apply] + ft_rank_all +
// ft_adders, 2 = [ft_slot_bases] + ft_finish
hipError_t launch_ft_merge_phase(const FtPlan* plans, const FtPlan* host_plans, uint32_t nq, int phase, hipStream_t st);
// the train for sparsely hit ranges (ft_sparse.hip) over nq plans that all have sparse = 1, those with prescore = 1 in front: ft_sp_scan,
// [ft_sp_threshold, ft_sp_select], ft_slot_bases, [ft_sp_place], ft_sp_replay
hipError_t launch_ft_merge_sparse(const FtPlan* plans, const FtPlan* host_plans, uint32_t nq, hipStream_t st);
// The kernels of the dense train, each launched from its own unit (the build has no relocatable device code); grid.y = query.  What the
// train launches is ft_train_launch's decision (ft_merge_plan.h), ft_merge.hip executes it.
void launch_ft_syn_masks(const FtPlan* plans, uint32_t ranges, hipStream_t st);                          // ft_ranges.hip
void launch_ft_ranges(const FtPlan* plans, uint32_t ranges, uint32_t nq, hipStream_t st);
void launch_ft_preselect_apply(const FtPlan* plans, uint32_t blocks, uint32_t nq, hipStream_t st);
void launch_ft_rank_all(const FtPlan* plans, uint32_t blocks, uint32_t nq, hipStream_t st);              // ft_admit.hip
void launch_ft_adders(const FtPlan* plans, uint32_t ranges, uint32_t nq, hipStream_t st);
void launch_ft_slot_bases(const FtPlan* plans, uint32_t nq, hipStream_t st);
hipError_t launch_ft_finish(const FtPlan* plans, uint32_t ranges, uint32_t nq, size_t lds_bytes, hipStream_t st);   // ft_finish.hip
void launch_ft_shard_fold(const FtPlan* plan, uint32_t* dst, hipStream_t st);                                            // hist copies + popcount -> dst [kFtFoldWords]
void launch_ft_shard_hist_combine(const FtPlan* plan, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards, hipStream_t st);   // gathered [..][kFtFoldWords]
void launch_ft_shard_table_sum(uint32_t* table, const uint32_t* gathered, const uint32_t* pos, uint32_t n_shards, uint64_t n, uint64_t stride, hipStream_t st);   // gathered [..][stride]
struct FtImportBatch {             // pieces of one batched upload (pinned staging -> HBM), 16-byte words
	const void* src[kFtBatchMax + 1];
	void* dst[kFtBatchMax + 1];
	uint32_t n16[kFtBatchMax + 1];
	uint32_t n;
};
hipError_t launch_ft_import_batch(const FtImportBatch& b, hipStream_t st);

// PhraseMerger::Merge (phrasemergerimpl.h:161-329) for ONE phrase, ft_phrase.hip.  Three launches: admission over the first term's
// postings (ordered prefix = mergeData_ order), one thread per admitted document through the terms, packing of the documents with a
// non-zero rank into one posting list per sub-term of the first term (the rows the main merge then treats like words).
struct FtPhrasePlan {
	const FtPosSubterm* subs;      // the sub-terms of the phrase's terms, term after term, SortSubterms order
	const FtTermCfg* terms;        // [nterms]: calcTermRank configuration, sub_begin / sub_end into subs
	const int32_t* distance;       // [nterms] FtDslOpts::distance of the term (MergeWithDist's dist)
	const FtGridEntry* grid;       // the first term's sub-terms in blocks of kFtBlockPostings postings
	uint32_t nterms, n_grid, grid_blocks, n_rows0;   // n_rows0: sub-terms of the first term
	uint32_t max_merged;           // min(mergeLimit, Term(0).MaxVDocs()) (phrasemerger.h:341-342)
	uint32_t n_ranges;
	uint64_t total_docs;
	float distance_weight, distance_boost;
	const uint8_t* removed;
	const uint8_t* excluded;
	unsigned long long* lookback;  // [grid_blocks], zero
	uint32_t* sync;                // [8], zero: 0 ticket, 1 error, 2 admitted, 3 alive, 4-5 sum of caps (u64), 6-7 workspace top (u64)
	uint32_t* slot_doc;            // [max_merged] per admitted document, mergeData_ order
	uint32_t* slot_row;            // sub-term of the first term that added it
	uint32_t* slot_cap;            // positions the document can carry from one term to the next
	float* slot_proc;
	uint8_t* slot_field;
	uint64_t* slot_pos;            // offset of lastPhrasePositions in the workspace
	uint32_t* slot_npos;
	uint64_t* ws;                  // position workspace (2 x sum of caps)
	// packed rows: row r = [row_base[r], row_base[r] + row_cnt[r]) of the arrays below; pos_off holds row_cnt + 1 entries per row
	uint32_t* row_cnt;             // [n_rows0]
	uint32_t* row_base;            // [n_rows0]
	uint32_t* out_doc;
	float* out_rank;
	uint8_t* out_field;
	uint32_t* out_pos_off;
	uint64_t* out_fpos;
	uint32_t* out_range_off;       // [n_rows0][n_ranges + 1]
	uint32_t* out_header;          // [4 + n_rows0] (pinned, device view): admitted, error, alive, positions, then row_cnt
};
constexpr uint32_t kFtPhraseRowPad = 64;   // entries: every packed row starts on a 256-byte boundary
hipError_t launch_ft_phrase_admit(const FtPhrasePlan& p, hipStream_t st);
hipError_t launch_ft_phrase_docs(const FtPhrasePlan& p, uint32_t admitted, hipStream_t st);
hipError_t launch_ft_phrase_pack(const FtPhrasePlan& p, hipStream_t st);
hipError_t launch_ft_export(const FtPlan* plans, const FtPlan* host_plans, uint32_t nq, hipStream_t st);
hipError_t launch_ft_import(const void* host_plan_device_view, void* dev_plan, size_t bytes, hipStream_t st);
// ft_packed.hip: PackedIdRelVec streams -> flat posting arrays, one thread per word (counting pass, then writing pass)
// pieces of the packed streams for the wavefront decoder (null: the one-thread-per-word kernels)
struct FtPackedSegs {
	const uint32_t* seg_word;    // [nsegs] word (launch order) of a piece
	const uint32_t* seg_first;   // [nwords + 1] first piece of a word
	FtPackedCheckpoint* cps;     // [nsegs], byte_off preset to ~0
	uint32_t nsegs;
};
hipError_t launch_ft_packed_count(const uint8_t* bytes, const uint64_t* byte_off, const uint64_t* array_found_pos, uint32_t nwords, uint32_t num_fields,
								   FtPackedCounts* counts, const FtPackedSegs* segs, hipStream_t st, uint32_t first_word, uint32_t word_count);
hipError_t launch_ft_packed_write(const uint8_t* bytes, const uint64_t* byte_off, const uint64_t* array_found_pos, uint32_t nwords, uint32_t num_fields,
								   const FtPackedOut* outs, FtPackedCounts* counts, const FtPackedSegs* segs, hipStream_t st);

void set_error(const std::string& msg);

}  // namespace rxgpu

// The early returns of the C-ABI functions (include/rxgpu.h for the codes): a failed HIP call, a failed precondition
#define RX_HIP(expr)                                                                                      \
	do {                                                                                                  \
		hipError_t e__ = (expr);                                                                          \
		if (e__ != hipSuccess) {                                                                          \
			::rxgpu::set_error(std::string(#expr) + ": " + hipGetErrorString(e__));                                \
			return e__ == hipErrorOutOfMemory ? RXGPU_ERR_NOMEM : RXGPU_ERR_DEVICE;                       \
		}                                                                                                 \
	} while (0)

#define RX_CHECK(cond, code, msg) \
	do {                          \
		if (!(cond)) {            \
			::rxgpu::set_error(msg);       \
			return code;          \
		}                         \
	} while (0)

// A growable device buffer.
struct rxgpu_devbuf {
	void* ptr = nullptr;
	size_t bytes = 0;
	int ensure(size_t need);
	void release();
};

// Per-search scratch: one is checked out per host-side search call (or bound to a caller stream).
struct rxgpu_search_ctx {
	hipStream_t stream = nullptr;
	bool own_stream = false;
	rxgpu_devbuf d_queries, d_part_dist, d_part_row, d_out_dist, d_out_row, d_out_count, d_misc, d_select;
	rxgpu_devbuf d_qpad, d_qstats, d_dense, d_cand_row, d_cand_dist, d_cand_cnt;   // batched path
	rxgpu_devbuf d_visited, d_gcand_d, d_redo;                                     // HNSW (d_gcand_d: (dist bits, id) entries)
	rxgpu_devbuf d_allowed;                                                        // HNSW: the allowed-rows bitmap of a filtered call (one per call in flight)
	rxgpu_devbuf d_helper, d_helper_bits;                                          // HNSW: overflow queue of a batch, bitsets of its helper workgroups
	rxgpu_devbuf d_top;                                                            // bf16- / int8-pruned scan: approximate top lists
	rxgpu_devbuf d_qplanes;                                                        // int8-pruned scan: the query's two int8 planes
	rxgpu_devbuf d_emit, d_emit_cnt;                                               // int8-pruned scan: the rows it emitted and their count per wavefront (knn_emit_plan.h)
	rxgpu_devbuf d_seed;                                                           // 6-bit front: the seed pass's merged list, laid out like d_top
	rxgpu_devbuf d_ivf;                                                            // IVF: the coarse search's lists, distances, count
	rxgpu_devbuf d_subset, d_bitmap, d_tiles;                                      // pre-filtered search: row list, allowed-rows bitmap, tile sums
	uint32_t pruned_cap = 0;   // candidate capacity of the pruned chain the current call enqueued (0: none) — rxgpu_index_last_candidates
	// ... and what else rxgpu_index_inspect needs to find that chain's buffers again (set with pruned_cap): rows or list entries scanned, kk,
	// the padded query stride, and the tier (int8: d_qplanes and the {s_q, |q|^} pair in front of d_qstats exist)
	uint64_t pruned_n = 0;
	uint32_t pruned_kk = 0, pruned_ld = 0;
	bool pruned_i8 = false;
	bool pruned_i6 = false;           // the 6-bit front ran: d_seed holds the seed pass's merged list
	uint32_t pruned_emit_gridx = 0;  // the grid of the int8 scan when it emitted (0: it stored a value per row and emitted nothing)
	// Set by a host entry point that ends in copy_back_knn, in front of the enqueue, when the call will be recorded for rxgpu_index_inspect
	// (profiling, one query); cleared by copy_back_knn.  The emitting int8 scan then keeps its value per row as well ("pruned_values").
	bool keep_values = false;
	void* h_pinned = nullptr;
	size_t h_pinned_bytes = 0;
	// second stream + events (created on first use): work that does not depend on the query upload — zeroing the visited bitsets of an
	// HNSW launch — runs beside it
	hipStream_t aux_stream = nullptr;
	hipStream_t aux2_stream = nullptr;   // second half of a large HNSW batch: its upload runs beside the first half's searches
	hipEvent_t split_done = nullptr;
	hipEvent_t aux_done = nullptr, main_done = nullptr;
	int ensure_aux();
	int ensure_pinned(size_t need);
	void release();
};

struct rxgpu_profile_slot {
	std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
};

struct rxgpu_index;
namespace rxgpu {
struct ShardSet;
void sharded_destroy(struct ::rxgpu_index* h);
uint64_t sharded_device_bytes(const struct ::rxgpu_index* h);
int sharded_upload_rows(struct ::rxgpu_index* h, uint64_t first_row, uint64_t n, const float* rows, const float* inv_norms);
int sharded_truncate(struct ::rxgpu_index* h, uint64_t count);
int sharded_move_row(struct ::rxgpu_index* h, uint64_t from, uint64_t to);
int sharded_search_knn_impl(struct ::rxgpu_index* h, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* row_ids, uint64_t n_ids, float* out_dist,
							uint32_t* out_row, uint32_t* out_count);
int sharded_search_range_impl(struct ::rxgpu_index* h, const float* query, float radius, int inclusive, const uint32_t* row_ids, uint64_t n_ids,
							  float* out_dist, uint32_t* out_row, uint64_t cap, uint64_t* out_total);
int sharded_distances(struct ::rxgpu_index* h, const float* query, const uint32_t* rows, uint32_t n, float* out_dist);
// Sharded HNSW: a graph per shard (attached through rxgpu_index_shard handles), SearchKnn fans out and meets in the exchange
struct HnswSink {
	uint32_t* d_dist;   // [nq][kk] distance bits   (device memory of the shard's GPU)
	uint32_t* d_row;    // [nq][kk] shard-local rows, kInvalidRow past a query's count
	uint32_t kk;
};
// queries: float rows, or (qcorr != null) SQ8 codes with their corrective offsets and normCoefs — the shard then searches its code table
int hnsw_search_to_sink(struct ::rxgpu_index* shard, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, const HnswSink& sink);
// nq packed float rows in HBM as queries over the graph of the first `nodes` rows (the construction searches of a build batch)
int hnsw_search_rows_to_sink(struct ::rxgpu_index* h, const float* d_queries, uint32_t nq, uint32_t k, uint32_t ef, uint64_t nodes, const HnswSink& sink);
int sharded_hnsw_search_knn(struct ::rxgpu_index* h, const void* queries, const float* qcorr, const float* qnorm, uint32_t nq, uint32_t k, uint32_t ef, float* out_dist,
							uint32_t* out_row, uint32_t* out_count);
int sharded_hnsw_search_range(struct ::rxgpu_index* h, const float* query, float radius, uint32_t ef, float* out_dist, uint32_t* out_row, uint64_t cap,
							  uint64_t* out_total);
}  // namespace rxgpu

namespace rxgpu {
// The resident HNSW search kernel of an index and its mailbox (rxgpu_hnsw_server.hip)
struct HnswServerState;
struct HnswServerConfig {
	uint32_t slots = 256;      // RXGPU_HNSW_SERVER_SLOTS: workgroups = requests in flight (one per CU of an MI355X; an idle slot looks at its mailbox word every ~7 us)
	uint32_t idle_us = 2000;   // RXGPU_HNSW_SERVER_IDLE_US: the kernel leaves after so long without a request
	bool nbl = false;          // RXGPU_HNSW_NBL=1: link blocks come along with a hop's rows (read when the mailbox is made; off by default)
	bool spec = false;         // RXGPU_HNSW_SPEC=1: look-ahead distance batches (read when the index's mailbox is made; off by default)
	uint32_t life_ms = 50;     // RXGPU_HNSW_SERVER_LIFE_MS: ... and after so long in any case (the next caller launches the next one)
};
// 1: served; 0: not served (the caller takes the launches); 2: the search ran there and came back flagged (the launching tiers answer it);
// any other value: an RXGPU error code (negative, as everywhere in the ABI), which the caller returns as it is
int hnsw_server_search(struct ::rxgpu_index* h, const HnswServerConfig& cfg, const float* query, uint32_t k, uint32_t ef, float* out_dist, uint32_t* out_row,
					   uint32_t* out_count);
// the same through the index's mailbox over SQ8 codes: the query as prepareData leaves it (dim codes, corrective offset) and its normCoef
int hnsw_server_search_sq8(struct ::rxgpu_index* h, const HnswServerConfig& cfg, const uint8_t* codes, float qcorr, float qnorm, uint32_t k, uint32_t ef,
						   float* out_dist, uint32_t* out_row, uint32_t* out_count);
void hnsw_server_quiesce(struct ::rxgpu_index* h);      // before the index changes: the resident kernel leaves, none is queued
void hnsw_server_destroy(struct ::rxgpu_index* h);
void hnsw_servers_pause_device(int device);             // before a device-wide wait: every index's resident kernel on that device leaves
extern std::atomic<int> g_resident_kernels;             // resident search kernels that may be alive: frees are deferred meanwhile (rxgpu_capi.hip)
void free_or_retire(void* ptr, size_t bytes, bool host);
void drain_retired();
hipError_t device_wait_all(int device);                 // hipDeviceSynchronize behind hnsw_servers_pause_device
void hnsw_server_times(const struct ::rxgpu_index* h, uint64_t* device_us, uint64_t* caller_us);
void hnsw_server_counters(const struct ::rxgpu_index* h, uint64_t* served, uint64_t* generations);
// The calling thread's device for a scope; what was current before comes back behind it.  ok: the switch worked (rxgpu_index_create asks).
struct DeviceGuard {
	int prev = -1;
	bool ok = true;
	explicit DeviceGuard(int dev) {
		if (hipGetDevice(&prev) != hipSuccess) prev = -1;
		if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
	}
	~DeviceGuard() {
		if (prev >= 0) (void)hipSetDevice(prev);
	}
};
}  // namespace rxgpu

struct rxgpu_index {
	rxgpu::ShardSet* shard_set = nullptr;   // non-null: a row-range sharded index (rxgpu_sharded.hip); the fields below describe the whole
	int metric = 0;
	uint32_t dim = 0;
	uint32_t stride = 0;     // floats per row in HBM
	uint64_t capacity = 0;   // rows allocated (owned storage only)
	uint64_t count = 0;
	int device = 0;
	int cus = 256;

	float* d_rows = nullptr;       // owned or adopted
	float* d_inv_norms = nullptr;  // cosine only
	bool adopted = false;

	// batched path: per-row |x|^2 (L2) and the maxima entering the rounding bound; recomputed lazily after mutations
	float* d_row_sq = nullptr;
	uint64_t row_sq_capacity = 0;
	unsigned int* d_stats = nullptr;
	bool stats_valid = false;
	std::atomic<bool> stats_finite{true};   // valid with stats_valid: no row has a NaN / infinite |x|^2 — what the pruning bound of the bf16 scan needs
	uint16_t* d_rows_bf16 = nullptr;   // bf16 shadow of the rows for the nomination GEMM (built lazily with the row statistics)
	uint64_t bf16_capacity = 0;
	bool bf16_blocked = true;   // layout of the shadow (knn_kernels.hip.h); RXGPU_SHADOW_BLOCKED=0 when the shadow is first built: row-major (A/B)
	bool bf16_valid = false;
	bool bf16_unavailable = false;     // the shadow did not fit in HBM: nominate on the f32 rows instead (still exact, still on the GPU)
	// int8 shadow of the rows for the pruning pass of a single query (knn_scan_i8.hip), built lazily and kept in step like the bf16 shadow
	int8_t* d_codes_i8 = nullptr;      // [i8_capacity][i8_ld(dim)]
	float2* d_side_i8 = nullptr;       // [i8_capacity] {scale, residual bound}
	uint64_t i8_capacity = 0;
	bool i8_valid = false;
	bool i8_unavailable = false;       // it did not fit in HBM: the call takes the bf16 tier
	// 6-bit shadow for the 6-bit front of the same chain (knn_scan_i6.hip): tiles of 4 rows (knn_i6_quant.h), its own side pairs and its own
	// statistics words {max e^2, max (e inv_norm)^2, non-finite}; built lazily and kept in step like the int8 shadow
	uint8_t* d_codes_i6 = nullptr;     // [i6_tiles(i6_capacity)] tiles
	float2* d_side_i6 = nullptr;       // [i6_capacity]
	unsigned int* d_stats_i6 = nullptr;
	uint64_t i6_capacity = 0;
	bool i6_valid = false;
	bool i6_unavailable = false;       // it did not fit in HBM: the call takes the int8 front
	std::atomic<uint32_t> last_cand_count{0}, last_cand_cap{0};   // rxgpu_index_last_candidates
	// rxgpu_index_inspect: the context the last profiled single-query pruned call ran in (idle in the pool since, so its buffers hold what the
	// chain left until the next call on the index takes it), with that call's sizes.  Guarded by mtx; null: none recorded.
	rxgpu_search_ctx* last_pruned_ctx = nullptr;
	uint64_t last_pruned_n = 0;
	uint32_t last_pruned_kk = 0, last_pruned_ld = 0;
	bool last_pruned_i8 = false;
	bool last_pruned_i6 = false;
	uint32_t last_pruned_emit_gridx = 0;

	// HNSW graph mirror (rxgpu_hnsw_attach_graph)
	uint32_t* d_links0 = nullptr;
	uint64_t* d_upper_off = nullptr;
	uint32_t* d_upper = nullptr;
	uint8_t* d_deleted = nullptr;
	// IVF: inverted lists over this index's rows as CSR (rxgpu_index_set_lists)
	uint64_t* d_list_off = nullptr;   // [nlist + 1]
	uint32_t* d_list_rows = nullptr;  // [lists_rows]
	uint32_t nlist = 0;
	uint64_t lists_rows = 0, lists_count = 0;   // rows listed; the index row count the lists were built for
	uint64_t lists_longest = 0;                 // rows of the longest list
	// rxgpu_search_knn_lists_batch since rxgpu_ivf_read_batch_stats: calls, queries, device trains, queries answered one by one (guarded by mtx)
	uint64_t ivf_batch_calls = 0, ivf_batch_queries = 0, ivf_batch_trains = 0, ivf_batch_one_by_one = 0;
	// SQ8 copy of the rows (rxgpu_hnsw_attach_sq8): codes [sq8_n][dim], stored corrective offsets, alpha^2
	uint8_t* d_codes = nullptr;
	float* d_corr = nullptr;
	float sq8_alpha2 = 0.f;
	uint64_t sq8_n = 0, sq8_cap = 0;   // rows with codes / rows the tables are allocated for
	uint64_t sq8_dev_rows = 0, sq8_dev_launches = 0;   // rxgpu_hnsw_quantize_sq8 since rxgpu_hnsw_read_sq8_quantize_stats: rows coded, launches,
	double sq8_dev_ms = 0.0;                           // and the kernel's time between two events
	// rxgpu_ivf_assign / rxgpu_ivf_kmeans_step since rxgpu_ivf_read_train_stats: rows assigned, steps, device time of the calls between two events,
	// and the part of it the sums kernel took
	uint64_t ivf_dev_rows = 0, ivf_dev_steps = 0;
	double ivf_dev_ms = 0.0, ivf_sums_ms = 0.0;
	uint64_t graph_n = 0, graph_deleted = 0;
	uint64_t graph_rows_cap = 0, graph_upper_cap = 0, graph_upper_used = 0;   // allocated level-0 rows / upper blocks (rxgpu_hnsw_patch_graph grows in place)
	uint32_t graph_M = 0, graph_maxM0 = 0;
	int graph_maxlevel = -1;
	uint32_t graph_entry = 0;
	bool graph_attached = false;
	// The batched level-0 build (rxgpu_hnsw_build.hip).  graph_upper_nodes: nodes whose upper lists are mirrored — graph_n, except between a
	// rxgpu_hnsw_link_batch and the rxgpu_hnsw_patch_upper that follows it.  build_nodes: the two per-node words of the pair grouping
	// (hnsw_build_plan.h), allocated with the first batch for the graph's row capacity and all zero between batches.
	uint64_t graph_upper_nodes = 0;
	rxgpu_devbuf build_scratch, build_nodes;
	uint64_t build_nodes_cap = 0;
	uint64_t build_rows = 0, build_batches = 0, build_reselected = 0, build_over = 0;   // since rxgpu_hnsw_read_build_stats
	double build_ms[3] = {0.0, 0.0, 0.0};                                                // search, select, back-link
	// Level 1 of a batch (rxgpu_hnsw_link_batch_upper).  build_view: the level-1 lists as a dense array [graph_rows_cap][1 + M], gathered
	// from the blocks for every batch; the rows of the batch's own nodes stay there until rxgpu_hnsw_patch_upper_from has given them
	// blocks.  build_upper_end: the end of the batch whose level 1 was linked last (0: none pending), build_upper_last: its rows.
	rxgpu_devbuf build_view;
	uint64_t build_upper_end = 0, build_upper_last = 0;
	uint64_t build_upper_rows = 0, build_upper_reselected = 0, build_upper_over = 0;     // since rxgpu_hnsw_read_build_upper_stats
	double build_upper_ms[3] = {0.0, 0.0, 0.0};
	unsigned long long* d_hnsw_stats = nullptr;
	// the resident search kernels' mailboxes, made at the first single query of the class: [0] floats, ef <= 128; [1] floats, ef <= 256;
	// [2] / [3] the same two over the SQ8 codes.  Written once under mtx (release), read without it (acquire).
	std::atomic<rxgpu::HnswServerState*> hnsw_server[4] = {{nullptr}, {nullptr}, {nullptr}, {nullptr}};
	bool hnsw_server_failed[4] = {false, false, false, false};
	std::atomic<uint64_t> hnsw_lds_reruns{0};   // searches whose candidate heap outgrew its first LDS area and were re-run with the largest one
	std::atomic<uint64_t> hnsw_tie_reruns{0};   // queries the sorted-list search handed to the heap kernel (equal distances met)

	std::mutex mtx;  // guards ctx pool + profile state
	std::vector<rxgpu_search_ctx*> free_ctx;
	std::map<void*, rxgpu_search_ctx*> stream_ctx;
	int32_t* d_row_ids = nullptr;   // internal row -> row id (label >> 32) for consumers on the device (hybrid fusion); null until uploaded
	uint64_t row_ids_cap = 0;
	// rxgpu_search_knn_resident: the result stays in the context's buffers for a consumer on the device.  One context per CALLING THREAD:
	// the list a thread left in HBM lives until that thread's next resident search, whatever other threads search meanwhile.
	// A thread that ends gives its context back to the pool (rxgpu_capi.hip: ResidentThread), found through `serial` in the table of live indexes.
	std::map<std::thread::id, rxgpu_search_ctx*> resident_ctx;
	std::mutex resident_mtx;
	uint64_t serial = 0;

	bool profiling = false;
	std::map<std::string, rxgpu_profile_slot> profile;
};

namespace rxgpu {
// Check out a scratch context with its own stream (host-synchronous searches), and hand it back (rxgpu_capi.hip).
rxgpu_search_ctx* acquire_ctx(rxgpu_index* h);
void release_ctx(rxgpu_index* h, rxgpu_search_ctx* c);
// the calling thread took a resident context of h (rxgpu_search_knn_resident): when the thread ends, the context goes back to h's pool
void resident_thread_uses(rxgpu_index* h);
// ... handed back when the scope ends
struct CtxLease {
	rxgpu_index* h;
	rxgpu_search_ctx* c;
	~CtxLease() { release_ctx(h, c); }
};
// While the index is profiling (rxgpu_profile_enable): an event pair around what the scope enqueues on s, filed under `name`.
struct ProfileScope {
	rxgpu_index* h;
	const char* name;
	hipStream_t s;
	hipEvent_t a = nullptr, b = nullptr;
	ProfileScope(rxgpu_index* h_, const char* n, hipStream_t s_);
	~ProfileScope();
};

// Data derived from the rows (rxgpu_derived.hip): row statistics, bf16 shadow, int8 shadow.  The chains build them lazily ...
int ensure_row_stats(rxgpu_index* h, hipStream_t s);
int ensure_bf16_shadow(rxgpu_index* h, hipStream_t s);   // RXGPU_ERR_NOMEM + h->bf16_unavailable: it does not fit, the caller takes the f32 rows
int ensure_i8_shadow(rxgpu_index* h, hipStream_t s);     // (the row statistics first)  RXGPU_ERR_NOMEM + h->i8_unavailable: the caller takes the bf16 tier
int ensure_i6_shadow(rxgpu_index* h, hipStream_t s);     // (the row statistics first)  RXGPU_ERR_NOMEM + h->i6_unavailable: the caller takes the int8 front
// ... and the mutations keep them in step
int derived_follow_truncate(rxgpu_index* h, uint64_t count);                    // the index shrinks to `count` rows (before h->count changes)
void derived_invalidate(rxgpu_index* h);                                       // the rows changed wholesale: everything is rebuilt at its next use
int derived_follow_upload(rxgpu_index* h, uint64_t first_row, uint64_t n);      // rows [first_row, first_row + n) were written
int derived_follow_move(rxgpu_index* h, uint64_t from, uint64_t to);            // row `from` was copied over row `to`
void derived_free(rxgpu_index* h);                                              // the index is being destroyed
// a named internal buffer copied to the host (rxgpu_index_inspect; test instrumentation, reads only)
int inspect_index(rxgpu_index* h, const char* what, void* out, uint64_t cap_bytes, uint64_t* out_bytes);

// The chains of brute-force KNN (rxgpu_knn_chains.hip), as far as the entry points call them.  nq device-resident queries, results in d_out_* (device).
int enqueue_knn(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist, uint32_t* d_out_row,
				uint32_t* d_out_count);   // kk <= kMaxFusedK: fused / batched / pruned, as the scan policy says
int enqueue_knn_fused(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, float* d_out_dist, uint32_t* d_out_row,
					  uint32_t* d_out_count);   // kk <= kMaxFusedK2
int enqueue_knn_subset(rxgpu_index* h, rxgpu_search_ctx* c, const float* d_queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids, uint64_t n_ids,
					   float* d_out_dist, uint32_t* d_out_row, uint32_t* d_out_count);   // over an ascending row list in HBM
int search_subset_host(rxgpu_index* h, rxgpu_search_ctx* c, const float* queries, uint32_t nq, uint32_t kk, const uint32_t* d_ids, uint64_t n_ids,
					   float* out_dist, uint32_t* out_row, uint32_t* out_count);   // ... queries and results on the host, any kk
int copy_back_knn(rxgpu_index* h, rxgpu_search_ctx* c, uint32_t nq, uint32_t kk, uint32_t eff, float* out_dist, uint32_t* out_row, uint32_t* out_count);
void sort_dist_row(const std::vector<float>& hd, const std::vector<uint32_t>& hr, float* out_dist, uint32_t* out_row);   // by dist_row_less (shard_plan.h)
// the scan policy, without a device (rxgpu_scan_policy, rxgpu_scan_tier, rxgpu_scan_tier_subset, rxgpu_scan_tier_range)
enum ScanTier { kTierF32 = 0, kTierBf16 = 1, kTierI8 = 2 };
bool scan_policy_pruned(uint64_t rows, uint32_t dim, uint32_t nq, bool shadow_available, bool stats_finite);
ScanTier scan_policy_tier(uint64_t rows, uint32_t dim, uint32_t nq, bool bf16_available, bool i8_available, bool stats_finite);
// does a whole-index call of nq queries read the 6-bit shadow (the 6-bit front of the kTierI8 chain)?  rxgpu_scan_i6
bool scan_policy_i6(uint64_t rows, uint32_t dim, uint32_t nq, bool i6_available, bool stats_finite);
ScanTier scan_policy_tier_subset(uint64_t n_ids, uint32_t dim, uint32_t nq, uint32_t kk, bool i8_available, bool stats_finite);
ScanTier scan_policy_tier_range(uint64_t rows, uint32_t dim, bool list, bool i8_available, bool stats_finite);   // rxgpu_scan_tier_range
// The int8 front of a range call whose query lies in c->d_queries (d_ids null: every row, else n list entries in HBM) and whose counter
// c->d_out_count is zero: query prep, pruning scan, exact tail into c->d_out_dist / d_out_row (dcap entries).  *ccap = the candidate list's
// size; the caller reads c->d_cand_cnt back with the hit count, and more candidates than *ccap mean the tail did nothing.
int enqueue_range_pruned_i8(rxgpu_index* h, rxgpu_search_ctx* c, const uint32_t* d_ids, uint64_t n, float radius, int inclusive, uint64_t cap, uint64_t dcap,
							uint32_t* ccap);
}  // namespace rxgpu
