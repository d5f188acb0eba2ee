// Device code shared by the HNSW search kernels (hnsw_search.hip: the launches; hnsw_server.hip: the resident form): the reference's two
// heaps and ONE search by one wavefront / one team (hnsw_search_one); the sorted list (hnsw_sorted_list.hip.h), the distance
// batches (hnsw_distances.hip.h) and the visited sets (hnsw_visited.hip.h) are files of their own.  See hnsw_search.hip for what is replaced
// and why the results are equal.
#pragma once
#include <type_traits>

#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"
#include "hnsw_distances.hip.h"
#include "hnsw_sorted_list.hip.h"
#include "hnsw_visited.hip.h"

namespace rxgpu {

// --- PriorityQueue<pair<float,tableint>, vector, CompareByFirst> restated on an array of (dist bits, id) pairs (executed by ONE lane) ---
// One 8-byte entry per element: a sift level is ONE dependent LDS round trip (both children, each one ds_read_b64, issued together)
// instead of three (two distances, then the winner's id) — the heap updates of lane 0 are the longest stretch of a hop.
__device__ __forceinline__ float hp_dist(uint2 e) { return __uint_as_float(e.x); }
__device__ __forceinline__ void hp_sift_up(uint2* h, int child) {
	const uint2 v = h[child];
	while (child > 0) {
		const int parent = (child - 1) / 2;
		const uint2 pe = h[parent];
		if (!(hp_dist(pe) < hp_dist(v))) break;
		h[child] = pe;
		child = parent;
	}
	h[child] = v;
}
__device__ __forceinline__ void hp_sift_down(uint2* h, int parent, int size) {
	const uint2 v = h[parent];
	for (;;) {
		const int left = parent * 2 + 1;
		if (left >= size) break;
		const int right = left + 1;
		const uint2 le = h[left];
		const uint2 re = h[right < size ? right : left];
		const bool take_right = right < size && hp_dist(le) < hp_dist(re);
		const uint2 be = take_right ? re : le;
		if (!(hp_dist(v) < hp_dist(be))) break;
		h[parent] = be;
		parent = take_right ? right : left;
	}
	h[parent] = v;
}
__device__ __forceinline__ void hp_emplace(uint2* h, int& n, float vd, uint32_t vi) {
	h[n] = make_uint2(__float_as_uint(vd), vi);
	++n;
	if (n >= 2) hp_sift_up(h, n - 1);
}
__device__ __forceinline__ void hp_pop(uint2* h, int& n) {
	if (n >= 2) {
		const uint2 t = h[0];
		h[0] = h[n - 1];
		h[n - 1] = t;
		if (n > 2) hp_sift_down(h, 0, n - 1);
	}
	--n;
}
__device__ __forceinline__ void hp_replace_top(uint2* h, int n, float vd, uint32_t vi) {
	h[0] = make_uint2(__float_as_uint(vd), vi);
	hp_sift_down(h, 0, n);
}

typedef __attribute__((address_space(3))) void hnsw_lds_void;

// kLatency: few queries in flight -> two row sets per distance trip (fewer dependent round trips per hop, 172 VGPRs at D = 768);
// otherwise one set (92 VGPRs: twice the resident searches).  D <= 512 always affords two.
// kSorted: 0 = the reference's two heaps, replayed by lane 0; S > 0 = HnswSortedList<S> (ef <= 64 S, no deleted nodes, heaps not in LDS at all)
// kDel (with kSorted): the graph has deleted nodes — HnswSortedListDel
// kFilter (hnsw_filtered.hip): the call brings a bitmap of the nodes it may return (HnswFilteredParams::allowed; p is then that struct's
// base); a node with a clear bit is hidden exactly as a deleted one is — read in the four places that read the delete mark (entry point on
// the list and on the heaps, the fresh neighbours' nb_del[] on either path), from the bitmap itself: one bit per node, never a byte array
// per call
// A search that leaves as kHnswOverflow also goes into the launch's overflow queue when there is one: a few helper workgroups launched
// beside the batch (hnsw_helper_kernel) pick it up and run it with the largest LDS heap WHILE the batch is still running — after the batch
// such a search is pure tail (one of 16 384 queries took 5 - 7 ms of a 32 ms batch at 10M x 768).
__device__ __forceinline__ void hnsw_enqueue_overflow(const HnswParams& p, uint32_t qi) {   // lane 0, behind the out_count store
	if (!p.helper_n) return;
	__threadfence();
	const uint32_t at = atomicAdd(p.helper_n, 1u);
	if (at < p.helper_cap) __hip_atomic_store(&p.helper_ids[at], p.q_base + qi + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// One search by one wavefront: slot = its scratch (visited set, global heap), qi = the query.  hnsw_search_kernel runs it once per
// workgroup, hnsw_helper_kernel in a loop over the overflow queue.
// A TEAM search (kTeam > 1 wavefronts per query, small launches): wavefront 0 runs the search below unchanged — list, visited set, link
// blocks — and the others only ever compute distances: at every distance batch the driver posts (ids, count) in the workgroup's box, all
// wavefronts meet at a barrier, each takes a slice of the rows (four rows a 16-lane group step, two sets a trip: 32 rows of 3 KB in flight
// per trip with four wavefronts instead of 8), and they meet again.  A hop's ~16 fresh neighbours are then ONE memory round trip instead of
// two or three — the search is a chain of ~140 dependent hops, and with a handful of queries on the chip nothing else hides them.  The
// driver's own LDS traffic is ordered wavefront-locally (HN_SYNC): the helpers do not take part in its barriers.
struct HnswTeamBox {
	const uint32_t* ids;
	float* dists;
	int cnt;     // < 0: the search is over
	int links;   // the ids are a hop's fresh neighbours: the other wavefronts also fetch their link blocks into the team's block area (p.nbl_off)
};
template <int kTeam>
__device__ __forceinline__ void hn_sync() {
	if constexpr (kTeam > 1) {
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
		__builtin_amdgcn_wave_barrier();
	} else {
		__syncthreads();
	}
}
// the rows wavefront `wave` of a team takes of a batch of cnt: [begin, begin + n), begin a multiple of 4
template <int kTeam>
__device__ __forceinline__ void team_slice(int cnt, int wave, int& begin, int& n) {
	const int per = (((cnt + kTeam - 1) / kTeam) + 3) & ~3;
	begin = wave * per;
	n = cnt - begin < per ? cnt - begin : per;
	if (n < 0) n = 0;
}
#define HN_SYNC() hn_sync<kTeam>()
// hidden from a filtered call's result: deleted, or not in the call's bitmap (p is the base of the kernel's HnswFilteredParams)
__device__ __forceinline__ bool hnsw_hidden(const HnswParams& p, uint32_t id) {
	const uint32_t* allowed = static_cast<const HnswFilteredParams&>(p).allowed;
	return p.deleted[id] != 0 || !((allowed[id >> 5] >> (id & 31)) & 1);
}
// (One function on purpose, for now: prologue, descent, layer 0 on the sorted list — with its look-ahead hop —, layer 0 on the heaps, store.
// Taking the descent, the insertion loop and the two stores out as __forceinline__ functions of their own, with the same statements, changed
// the machine code of every kernel that runs this — about a thousand lines of each — and so did one shared loop for the three "fetch a link
// block, test-and-mark, compact" sites; a full split over a shared state struct left one resident kernel spilling 8 VGPRs
// (tools/compare_kernel_isa.py, tests/test_hnsw_wide_rows_resources.py).  A split has to be measured on the device against this form, not
// assumed equal.)
template <int kMetric, bool kGlobalCand, int NB, bool kLatency, bool kSq8 = false, int kSorted = 0, bool kDel = false, int kTeam = 1, bool kFilter = false>
__device__ __forceinline__ void hnsw_search_one(const HnswParams& p, const uint32_t slot, const uint32_t qi, HnswTeamBox* box = nullptr) {
	static_assert(kTeam == 1 || (NB > 0 && !kSq8 && !kGlobalCand), "the team form serves the fixed-dimension float search with its heaps in LDS");
	static_assert(kSorted == 0 || !kGlobalCand, "the sorted-list search starts in LDS; its re-runs with a global heap are heap-kernel launches");
	static_assert(!kFilter || kSorted == 0 || kDel, "a filtered search hides nodes: its list is the one with deleted nodes");
	// dynamic LDS: [ef_cap] result heap (dist, id) then [lds_cand_cap] candidate heap (dist, id) — sized by the launcher so that
	// small-ef searches keep more wavefronts resident per CU.  (The areas of hnsw_lds_layout, spelled out: asking that function here, as
	// hnsw_team_serve does, moved the query loads of 45 SQ8 kernels — tools/compare_kernel_isa.py.)
	extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_lds[];
	uint2* top = reinterpret_cast<uint2*>(hnsw_lds);   // (dist bits, id) entries
	uint2* lcand = top + p.ef_cap;
	constexpr bool kQLds = NB > 0 && !kSq8;   // fixed dims: query fragment in LDS behind the heaps (16-byte aligned: every part is a multiple of 64 entries)
	float4* q_s = reinterpret_cast<float4*>(lcand + (kGlobalCand ? 0 : p.lds_cand_cap));
	uint32_t* lds_vis = reinterpret_cast<uint32_t*>(q_s + (kQLds ? NB * 16 : 0));   // [1 << vis_hash_log2] when p.vis_lds (latency form only)
	const bool vis_in_lds = kLatency && p.vis_lds != 0;
	__shared__ uint32_t nb_id[kHnswMaxNeighbors];
	__shared__ float nb_d[kHnswMaxNeighbors];
	__shared__ uint8_t nb_del[kHnswMaxNeighbors];
	__shared__ uint32_t s_cur;
	__shared__ int s_flag;
	__shared__ uint32_t s_pre[64];   // sorted-list search: the link block of the candidate next in line, fetched one hop ahead by LDS-DMA

	const int lane = threadIdx.x & 63;   // (a team's driver is wavefront 0)
	// the speculative team search (its hop below) keeps, at p.spec_off of the dynamic LDS: a direct-mapped table of distances computed ahead of
	// time (keys = node + 1, values), the link blocks of the two nearest open candidates, and the id / distance / destination arrays of a trip
	constexpr bool kSpecOk = kTeam > 1 && kSorted > 0 && !kDel && NB > 0 && !kSq8 && !kGlobalCand;
	constexpr uint32_t kSpecLog2 = kHnswSpecLog2;
	constexpr int kSpecRows = 8 * kTeam;   // rows of ONE distance trip of the team (two row sets of four rows a wavefront)
	uint32_t* spec_key = reinterpret_cast<uint32_t*>(hnsw_lds + p.spec_off);
	float* spec_val = reinterpret_cast<float*>(spec_key + (1u << kSpecLog2));
	uint32_t* spec_pre = spec_key + (2u << kSpecLog2);
	uint32_t* spec_id = spec_pre + 128;
	float* spec_d = reinterpret_cast<float*>(spec_id + 64);
	uint32_t* spec_dst = spec_id + 128;
	bool use_spec = false;
	if constexpr (kSpecOk) {
		use_spec = p.spec_off != 0u && p.maxM0 < 64u;
		if (use_spec) {
			for (uint32_t i = lane; i < (1u << kSpecLog2); i += 64) spec_key[i] = 0u;
		}
	}
	const float* q = p.queries + size_t(qi) * p.dim;
	uint32_t* visited = p.visited + size_t(slot) * p.visited_words;
	uint2* cand = kGlobalCand ? p.gcand + size_t(slot) * p.gcand_cap : lcand;
	const uint64_t cand_cap = kGlobalCand ? p.gcand_cap : uint64_t(p.lds_cand_cap);
	unsigned long long ndist = 0, hops = 0;
	float4 qreg[1];
	constexpr int kSqL = (kSq8 && NB > 0) ? (NB + 3) / 4 : 1;
	uint4 sq_q[kSqL];
	uint32_t sq_qq[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
	if constexpr (kSq8 && NB > 0) {
		const uint4* qp = reinterpret_cast<const uint4*>(p.qcodes + size_t(qi) * p.dim);
		const int m = lane & 15;
#pragma unroll
		for (int i = 0; i < kSqL; ++i) {
			sq_q[i] = (256 * i + 16 * m < 64 * NB) ? qp[16 * i + m] : make_uint4(0u, 0u, 0u, 0u);
			if constexpr (kMetric == kL2) {
				const uint32_t bw[4] = {sq_q[i].x, sq_q[i].y, sq_q[i].z, sq_q[i].w};
#pragma unroll
				for (int c = 0; c < 4; ++c) {
					sq_qq[2 * c] = __builtin_amdgcn_udot4(bw[c] & 0x0000FFFFu, bw[c], sq_qq[2 * c], false);
					sq_qq[2 * c + 1] = __builtin_amdgcn_udot4(bw[c] & 0xFFFF0000u, bw[c], sq_qq[2 * c + 1], false);
				}
			}
		}
	}
	// the query's corrective offset and normCoef, read ONCE: in the resident form they sit in the mailbox (pinned host memory) like the codes,
	// and a read per distance batch would be a trip across PCIe per hop
	float sq_qcorr = 0.f, sq_qnorm = 1.f;
	if constexpr (kSq8) {
		sq_qcorr = p.qcorr[qi];
		sq_qnorm = p.qnorm[qi];
	}
	if constexpr (NB > 0 && !kSq8) {
		const float4* qp = reinterpret_cast<const float4*>(q);
		for (int i = lane; i < NB * 16; i += 64) q_s[i] = qp[i];
		HN_SYNC();
	}
	int team_links = 0;   // (team searches) 1 while the batches are a hop's fresh neighbours, see HnswTeamBox::links
	auto distances = [&](const uint32_t* ids, int cnt, float* dists) {
		if constexpr (kSq8 && NB > 0) {
			batch_distances_sq8_fixed<kMetric, NB>(p, sq_q, sq_qq, sq_qcorr, sq_qnorm, ids, cnt, dists, lane);
		} else if constexpr (kSq8) {
			batch_distances_sq8<kMetric>(p, p.qcodes + size_t(qi) * p.dim, sq_qcorr, sq_qnorm, ids, cnt, dists, lane);
		} else if constexpr (NB > 0 && kTeam > 1) {
			box->ids = ids;
			box->dists = dists;
			box->cnt = cnt;
			box->links = team_links;
			__syncthreads();   // the whole team: the batch is posted (and everything the driver wrote to LDS before it is visible)
			int b0, n0;
			team_slice<kTeam>(cnt, 0, b0, n0);
			if constexpr (NB > 12) {
				batch_distances_wide<kMetric, NB, true>(p, q_s, ids + b0, n0, dists + b0, lane);
			} else {
				batch_distances_fixed<kMetric, NB, kQLds, true>(p, qreg, q_s, ids + b0, n0, dists + b0, lane);
			}
			__syncthreads();   // ... every slice is written
		} else if constexpr (NB > 12) {
			batch_distances_wide<kMetric, NB, kLatency, (kLatency ? 8 : 4)>(p, q_s, ids, cnt, dists, lane);
		} else if constexpr (NB > 0) {
			batch_distances_fixed<kMetric, NB, kQLds, (kLatency || NB <= 8)>(p, qreg, q_s, ids, cnt, dists, lane);
		} else {
			batch_distances<kMetric>(p, q, ids, cnt, dists, lane);
		}
	};

	const uint32_t vis_hash = p.vis_hash_log2;
	const unsigned long long vis_limit = vis_hash ? (1ull << (vis_hash - 1)) : ~0ull;   // entries the hash set may hold
	if (vis_hash) {   // the search zeroes its own (small) set: 16-byte stores, in flight during the descent through the upper levels
		if (vis_in_lds) {
			uint4* v4 = reinterpret_cast<uint4*>(lds_vis);
			for (uint32_t w = lane; w < (1u << vis_hash) / 4; w += 64) v4[w] = make_uint4(0u, 0u, 0u, 0u);
		} else {
			uint4* v4 = reinterpret_cast<uint4*>(visited);
			for (uint32_t w = lane; w < (1u << vis_hash) / 4; w += 64) v4[w] = make_uint4(0u, 0u, 0u, 0u);
		}
	}
	// ---- upper levels: greedy descent (getLayer0EntryPoint)
	uint32_t cur = p.entry;
	if (lane == 0) nb_id[0] = cur;
	HN_SYNC();
	distances(nb_id, 1, nb_d);
	HN_SYNC();
	float curdist = nb_d[0];
	ndist += 1;
	for (int level = p.maxlevel; level > 0; --level) {
		bool changed = true;
		while (changed) {
			HN_SYNC();
			const uint32_t* ll = p.upper + (p.upper_off[cur] + uint64_t(level - 1)) * (1 + p.M);
			const int cnt = int(ll[0]);
			for (int j = lane; j < cnt; j += 64) nb_id[j] = ll[1 + j];
			HN_SYNC();
			distances(nb_id, cnt, nb_d);
			HN_SYNC();
			ndist += cnt;
			changed = false;
			for (int i = 0; i < cnt; ++i) {   // uniform scalar-style scan (every lane computes the same thing)
				const float d = nb_d[i];
				if (d < curdist) {
					curdist = d;
					cur = nb_id[i];
					changed = true;
				}
			}
		}
	}

	const unsigned long long ndist_upper = ndist;
	if constexpr (kSorted > 0) {
		// ---- layer 0 on the sorted list
		using List = typename std::conditional<kDel, HnswSortedListDel<kSorted>, HnswSortedList<kSorted>>::type;
		List list;
		list.init(p.sorted == 1);
		const int ef = int(p.ef);
		bool ep_live;
		if constexpr (kFilter) {
			ep_live = !hnsw_hidden(p, cur);
		} else {
			ep_live = !kDel || !p.deleted[cur];
		}
		if (ep_live) {
			list.insert(curdist, cur, false, ef, lane);
			ndist += 1;   // the reference recomputes the entry distance here (same value)
		} else {
			list.insert(3.402823466e+38f, cur, true, ef, lane);   // a deleted entry point: candidate at FLT_MAX, lowerBound = FLT_MAX (:853-856)
		}
		if (vis_hash) {   // the zeroing stores have landed before the first test-and-set
			__threadfence();
			HN_SYNC();
		}
		if (lane == 0) (void)hnsw_visit_sel<kLatency>(visited, lds_vis, vis_in_lds, vis_hash, cur);
		// the link block of the candidate that is next in line, requested one hop ahead: it arrives while this hop's visited tests and row
		// gathers are in flight, and saves the next hop its first dependent round trip whenever no nearer candidate turned up meanwhile
		// (LDS-DMA: the block goes straight into s_pre, no register lives across the hop — the D = 768 kernel sits at its 96-VGPR budget)
		uint32_t pre_node = 0xFFFFFFFFu;
		uint32_t pre_tag0 = 0xFFFFFFFFu, pre_tag1 = 0xFFFFFFFFu;   // speculative team search: the nodes whose link blocks sit in spec_pre[0] / [1]
		unsigned long long spec_trips = 0;
		int nbl_rows = 0;                   // team searches: rows of the last hop whose link blocks sit in the team's block area
		unsigned long long nbl_hits = 0;
#ifdef RXGPU_HNSW_PHASES
		unsigned long long ph_a = 0, ph_b = 0, ph_c = 0, ph_t = __builtin_readcyclecounter(), ph_start = ph_t;
#define HN_PHASE(acc)                                              \
	do {                                                           \
		const unsigned long long now__ = __builtin_readcyclecounter(); \
		acc += now__ - ph_t;                                       \
		ph_t = now__;                                              \
	} while (0)
#else
#define HN_PHASE(acc) do { } while (0)
#endif
		for (;;) {
			if (ndist - ndist_upper + p.maxM0 > vis_limit) {   // the hash set would pass half full: this search goes to the bitset re-run
				if (lane == 0) {
					p.out_count[qi] = kHnswOverflow;
					hnsw_enqueue_overflow(p, qi);
				}
				return;
			}
			uint32_t node;
			float cdist;
			if (!list.pop(node, cdist, ef)) {   // candidate_set empty, or only dead entries left in it ...
				list.tie = list.tie || (list.held() == ef && list.lower == list.outside);   // ... of which the last one is still alive in the reference's
				break;
			}
			if (list.tie) break;                 // the rest of this search belongs to the heaps
			if (cdist > list.lower && (!kDel || list.held() == ef)) break;   // layer0ShouldStopBeforePop (never true for a member of a full list; kept for the form)
			hops += 1;
			int nfresh = 0;
			bool spec_hop = false;
			if constexpr (kSpecOk) spec_hop = use_spec;
			if (spec_hop) {
				if constexpr (kSpecOk) {
					// (RXGPU_HNSW_SPEC=1.  MEASURED, 1M x 768, ef = 128, one query at a time: 0.547 ms against 0.452 ms without it — only 23 % of the
					// hops run without a trip (the candidate expanded next is more often one this very hop inserted than the one in line before
					// it) and the bookkeeping below costs ~0.7 us a hop; profiles/rd6sp_single_1m.json.  Exact — fuzz and parity tests run it —
					// but off by default.)
					// ---- a hop of the SPECULATIVE team search.  The traversal is the reference's — pops, marks and insertions in its order, every
					// distance the same bits — but a distance need not be computed in the hop that uses it: d(query, row) does not change during a
					// search.  Each distance trip of the team (32 rows, four wavefronts) carries, next to the rows this hop must have, the unmarked
					// neighbours of the candidate NEXT in line, and their distances wait in a small direct-mapped table (spec_key / spec_val; a
					// collision only costs a re-evaluation).  When that candidate is popped — it is, unless this hop inserts something nearer, and
					// then it usually is a hop later — its rows are already there and the hop runs without a memory round trip.  The link blocks of
					// the two nearest open candidates are kept in LDS (two buffers, LDS-DMA), so the look-ahead has its list without a trip either.
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every link block requested so far has landed
					const int e1 = list.first_open();
					const uint32_t c1 = e1 >= 0 ? hnsw_node_at<List, kSorted>(list, e1) : 0xFFFFFFFFu;
					const int e2 = e1 >= 0 ? list.next_open(e1) : -1;
					const uint32_t c2 = e2 >= 0 ? hnsw_node_at<List, kSorted>(list, e2) : 0xFFFFFFFFu;
					const int nbuf = node == pre_tag0 ? 0 : (node == pre_tag1 ? 1 : -1);   // uniform
					int c1buf = c1 == 0xFFFFFFFFu ? -1 : (c1 == pre_tag0 ? 0 : (c1 == pre_tag1 ? 1 : -1));
					const uint32_t* ll = p.links0 + size_t(node) * (1 + p.maxM0);
					const uint32_t word = nbuf >= 0 ? spec_pre[64 * nbuf + lane] : (lane <= int(p.maxM0) ? ll[lane] : 0u);
					const uint32_t w1 = c1buf >= 0 ? spec_pre[64 * c1buf + lane] : 0u;
					const int cnt = int(__builtin_amdgcn_readfirstlane(word));
					const int cnt1 = int(__builtin_amdgcn_readfirstlane(w1));   // (both blocks are in registers: their buffers may be overwritten)
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					if (p.prefetch_links) {   // keep the blocks of the two nearest open candidates in LDS
						auto fetch = [&](int b, uint32_t nd) {
							const uint32_t* src = p.links0 + size_t(nd) * (1 + p.maxM0) + (lane <= int(p.maxM0) ? lane : int(p.maxM0));
							__builtin_amdgcn_global_load_lds(src, (hnsw_lds_void*)(spec_pre + 64 * b), 4, 0, 0);
							if (b == 0) {
								pre_tag0 = nd;
							} else {
								pre_tag1 = nd;
							}
						};
						int holds1 = c1buf;   // the buffer that holds (or is about to hold) c1's block
						if (c1 != 0xFFFFFFFFu && c1buf < 0) {
							holds1 = (c2 != 0xFFFFFFFFu && c2 == pre_tag0) ? 1 : 0;
							fetch(holds1, c1);
						}
						if (c2 != 0xFFFFFFFFu && holds1 >= 0 && c2 != pre_tag0 && c2 != pre_tag1) fetch(1 - holds1, c2);
					}
					// the popped node's neighbours: test-and-mark, in list order
					{
						const int j = lane - 1;
						bool fresh = false;
						if (j >= 0 && j < cnt) fresh = hnsw_visit_sel<kLatency>(visited, lds_vis, vis_in_lds, vis_hash, word);
						const uint64_t fm = __ballot(fresh);
						if (fresh) nb_id[__popcll(fm & ((1ull << lane) - 1))] = word;
						nfresh = __popcll(fm);
					}
					HN_SYNC();
					HN_PHASE(ph_a);
					// which of them were evaluated ahead of time
					int nmiss = 0;
					{
						const bool mine = lane < nfresh;
						const uint32_t id = mine ? nb_id[lane] : 0u;
						const uint32_t sl = (id * 2654435761u) >> (32u - kSpecLog2);
						const bool have = mine && spec_key[sl] == id + 1u;
						if (have) nb_d[lane] = spec_val[sl];
						const uint64_t mm = __ballot(mine && !have);
						if (mine && !have) {
							const int r = __popcll(mm & ((1ull << lane) - 1));
							spec_id[r] = id;
							spec_dst[r] = uint32_t(lane);
						}
						nmiss = __popcll(mm);
					}
					// ... and the look-ahead: neighbours of the next candidate that are neither marked nor evaluated yet, as far as the trip has room
					int total = nmiss;
					if (c1buf >= 0 && nmiss < kSpecRows) {
						const int j = lane - 1;
						bool want = false;
						if (j >= 0 && j < cnt1) {
							const bool seen = vis_in_lds ? hnsw_seen_lds(lds_vis, vis_hash, w1) : hnsw_seen(visited, vis_hash, w1);
							want = !seen && spec_key[(w1 * 2654435761u) >> (32u - kSpecLog2)] != w1 + 1u;
						}
						const uint64_t sm = __ballot(want);
						const int r = nmiss + __popcll(sm & ((1ull << lane) - 1));
						if (want && r < kSpecRows) {
							spec_id[r] = w1;
							spec_dst[r] = 0xFFFFFFFFu;
						}
						total = nmiss + __popcll(sm);
						total = total < kSpecRows ? total : kSpecRows;
					}
					HN_SYNC();
					if (total > 0) {
						distances(spec_id, total, spec_d);
						HN_SYNC();
						{
							const bool mine = lane < total;
							const float dv = mine ? spec_d[lane] : 0.f;
							const uint32_t dst = mine ? spec_dst[lane] : 0u;
							const bool ahead = mine && dst == 0xFFFFFFFFu;
							const uint32_t id = ahead ? spec_id[lane] : 0u;
							const uint32_t sl = (id * 2654435761u) >> (32u - kSpecLog2);
							if (mine && !ahead) nb_d[dst] = dv;
							// two look-ahead rows of one trip may share a table slot: the key decides which of them the slot keeps, and only that
							// lane writes the value (a key next to another row's value would be a wrong distance)
							if (ahead) spec_key[sl] = id + 1u;
							HN_SYNC();
							if (ahead && spec_key[sl] == id + 1u) spec_val[sl] = dv;
						}
						spec_trips += 1;
					}
					ndist += nfresh;
					HN_SYNC();
					HN_PHASE(ph_b);
				}
			} else {
				const uint32_t* ll = p.links0 + size_t(node) * (1 + p.maxM0);
				uint32_t first_word;
				uint64_t came_along = 0ull;   // (team searches) the popped node was one of the last hop's rows: its block came with them
				if constexpr (kTeam > 1) {
					if (nbl_rows > 0 && node != pre_node) came_along = __ballot(lane < nbl_rows && nb_id[lane] == node);   // nb_id still holds the last hop's rows
				}
				if (node == pre_node) {   // uniform: the block was requested a hop ago and has landed (every load issued since has been waited for)
					asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
					first_word = s_pre[lane];
				} else if (came_along) {
					first_word = reinterpret_cast<const uint32_t*>(hnsw_lds + p.nbl_off)[64 * __builtin_ctzll(came_along) + lane];
					nbl_hits += 1;
				} else {
					first_word = lane <= int(p.maxM0) ? ll[lane] : 0u;
				}
				int cnt = 0;
				for (int base = 0; base <= int(p.maxM0); base += 64) {
					const int w = base + lane;
					const uint32_t word = base == 0 ? first_word : (w <= int(p.maxM0) ? ll[w] : 0u);
					if (base == 0) {
						cnt = int(__builtin_amdgcn_readfirstlane(word));   // (s_pre has been read: the next request may overwrite it)
						pre_node = p.prefetch_links ? hnsw_peek_open<List, kSorted>(list) : 0xFFFFFFFFu;
						if (pre_node != 0xFFFFFFFFu) {
							const uint32_t* src = p.links0 + size_t(pre_node) * (1 + p.maxM0) + (lane <= int(p.maxM0) ? lane : int(p.maxM0));
							__builtin_amdgcn_global_load_lds(src, (hnsw_lds_void*)s_pre, 4, 0, 0);
						}
					}
					if (base > cnt) break;   // uniform
					const int j = w - 1;
					bool fresh = false;
					if (j >= 0 && j < cnt) fresh = hnsw_visit_sel<kLatency>(visited, lds_vis, vis_in_lds, vis_hash, word);
					const uint64_t fm = __ballot(fresh);
					if (fresh) nb_id[nfresh + __popcll(fm & ((1ull << lane) - 1))] = word;
					nfresh += __popcll(fm);
				}
				HN_SYNC();
				HN_PHASE(ph_a);
				if constexpr (kDel) {   // the delete marks travel while the distances are computed
					if constexpr (kFilter) {
						for (int j = lane; j < nfresh; j += 64) nb_del[j] = hnsw_hidden(p, nb_id[j]);
					} else {
						for (int j = lane; j < nfresh; j += 64) nb_del[j] = p.deleted[nb_id[j]];
					}
				}
				if constexpr (kTeam > 1) {
					team_links = (p.nbl_off != 0u && p.maxM0 < 64u) ? 1 : 0;
					nbl_rows = (team_links && nfresh > 0) ? (nfresh < kHnswNblRows ? nfresh : kHnswNblRows) : 0;
				}
				distances(nb_id, nfresh, nb_d);
				team_links = 0;
				ndist += nfresh;
				HN_SYNC();
				HN_PHASE(ph_b);
			}
			for (int base = 0; base < nfresh && !list.tie; base += 64) {   // runLayer0Step :932-960 in neighbour order; lane j carries neighbour base + j
				const int j = base + lane;
				const float dj = j < nfresh ? nb_d[j] : __builtin_inff();
				const uint32_t idj = j < nfresh ? nb_id[j] : 0u;
				const uint64_t delm = kDel ? __ballot(j < nfresh && nb_del[j] != 0) : 0ull;
				// lowerBound only falls while the list is full: what fails the test now fails it later in the loop as well
				uint64_t m = __ballot(j < nfresh && (list.held() < ef || list.lower > dj));
				if (list.held() == ef && __ballot(j < nfresh && dj == list.lower)) list.outside = list.lower;   // refused at dist == lowerBound
				while (m && !list.tie) {
					const int b = __builtin_ctzll(m);
					m &= m - 1;
					const float nd = lane_value(dj, b);
					if (list.held() < ef || list.lower > nd) {
						list.insert(nd, uint32_t(__builtin_amdgcn_readlane(int(idj), b)), ((delm >> b) & 1ull) != 0, ef, lane);
					} else if (nd == list.lower) {
						list.outside = nd;
					}
				}
			}
			HN_SYNC();
			HN_PHASE(ph_c);
		}
#ifdef RXGPU_HNSW_PHASES
		if (lane == 0 && p.stats) {
			atomicAdd(&p.stats[4], ph_a);
			atomicAdd(&p.stats[5], ph_b);
			atomicAdd(&p.stats[6], ph_c);
			atomicAdd(&p.stats[7], __builtin_readcyclecounter() - ph_start);
		}
#endif
		const int total = list.held();
		const int keep = total < int(p.k) ? total : int(p.k);   // SearchKnn :1998-2000: the k nearest of top_candidates
		if constexpr (!kDel) {
			if (!list.tie && total > keep && list.key_at(keep - 1) == list.key_at(keep)) list.tie = true;   // the trim pops one of two equal keys
		} else {
			if (!list.tie && total > keep && keep > 0 && list.key_at(list.live_at(keep - 1)) == list.key_at(list.live_at(keep))) list.tie = true;
		}
		if (!list.tie) {
			if constexpr (!kDel) {
#pragma unroll
				for (int s = 0; s < kSorted; ++s) {
					const int g = 64 * s + lane;
					if (g < keep) {
						p.out_dist[size_t(qi) * p.k + g] = list.d[s];
						p.out_row[size_t(qi) * p.k + g] = list.id[s];
					}
				}
			} else {
				int before = 0;   // live entries in the slots below
#pragma unroll
				for (int s = 0; s < kSorted; ++s) {
					const uint64_t lm = ~list.del[s] & List::below_count(s, list.n);
					const int r = before + __popcll(lm & ((1ull << lane) - 1ull));
					if (((lm >> lane) & 1ull) && r < keep) {
						p.out_dist[size_t(qi) * p.k + r] = list.d[s];
						p.out_row[size_t(qi) * p.k + r] = list.id[s];
					}
					before += __popcll(lm);
				}
			}
			if (lane == 0) {
				p.out_count[qi] = uint32_t(keep);
				if (p.stats) {
					atomicAdd(&p.stats[0], ndist);
					atomicAdd(&p.stats[1], hops);
					if (nbl_hits) atomicAdd(&p.stats[3], nbl_hits << 32);   // (high half: hops whose link block had come along with the previous hop's rows)
					if (spec_trips) atomicAdd(&p.stats[3], spec_trips);   // distance trips of the speculative team search (< hops: the rest ran on distances computed ahead)
				}
			}
			return;
		}
		// Equal keys that matter: this search starts over on the reference's heaps, here and now — while the rest of the batch keeps the
		// chip busy — instead of in a launch of its own after the batch (whose whole duration is the tail of ONE heap search).  The
		// launcher gives every workgroup a small heap area for that (lds_cand_cap entries; a search that outgrows it is flagged
		// kHnswOverflow and re-run with the global heap like any other); without one the query goes back to the host as kHnswTie.
		if (p.lds_cand_cap == 0) {
			if (lane == 0) p.out_count[qi] = kHnswTie;
			return;
		}
		if (vis_in_lds) {
			for (uint32_t w = lane; w < (1u << vis_hash); w += 64) lds_vis[w] = 0u;
		} else {
			for (uint64_t w = lane; w < p.visited_words; w += 64) visited[w] = 0u;
		}
		__threadfence();
		HN_SYNC();
		if (lane == 0 && p.stats) atomicAdd(&p.stats[2], 1ull);
		ndist = ndist_upper;
		hops = 0;
	}

	// ---- layer 0: initLayer0SearchState
	int top_n = 0, cand_n = 0;
	float lower;
	bool overflow = false;
	if (vis_hash) {   // the zeroing stores (kernel start, or the restart above) have landed before the first test-and-set
		__threadfence();
		HN_SYNC();
	}
	{
		bool ep_ok;
		if constexpr (kFilter) {
			ep_ok = !hnsw_hidden(p, cur);
		} else {
			ep_ok = p.bare || !p.deleted[cur];
		}
		if (lane == 0) {
			if (ep_ok) {
				hp_emplace(top, top_n, curdist, cur);
				hp_emplace(cand, cand_n, -curdist, cur);
			} else {
				hp_emplace(cand, cand_n, -3.402823466e+38f, cur);
			}
			(void)hnsw_visit_sel<kLatency>(visited, lds_vis, vis_in_lds, vis_hash, cur);
		}
		lower = ep_ok ? curdist : 3.402823466e+38f;
		if (ep_ok) ndist += 1;   // the reference recomputes the entry distance here (same value)
	}

	for (;;) {
		// layer0ShouldStopBeforePop + pop (lane 0), broadcast through LDS
		const bool vis_full = ndist - ndist_upper + p.maxM0 > vis_limit;   // uniform: the hash set would pass half full
		if (lane == 0) {
			int flag = 0;
			if (vis_full) overflow = true;
			if (cand_n == 0 || overflow) {
				flag = 1;
			} else {
				const uint2 best = cand[0];
				const float cdist = -hp_dist(best);
				if (p.bare ? (cdist > lower) : (cdist > lower && top_n >= int(p.ef))) {
					flag = 1;
				} else {
					s_cur = best.y;
					hp_pop(cand, cand_n);
				}
			}
			s_flag = flag;
		}
		HN_SYNC();
		if (s_flag) break;
		const uint32_t node = s_cur;
		hops += 1;
		// neighbours: the whole list block (count word + up to 2M ids) is fetched in ONE round — lane L reads word L of the block, so the
		// count arrives together with the ids instead of in front of them; atomicOr = visited test + mark
		const uint32_t* ll = p.links0 + size_t(node) * (1 + p.maxM0);
		int nfresh = 0;
		int cnt = 0;
		for (int base = 0; base <= int(p.maxM0); base += 64) {
			const int w = base + lane;   // word of the block; neighbour index j = w - 1
			const uint32_t word = w <= int(p.maxM0) ? ll[w] : 0u;
			if (base == 0) cnt = int(__builtin_amdgcn_readfirstlane(word));
			if (base > cnt) break;   // uniform
			const int j = w - 1;
			bool fresh = false;
			if (j >= 0 && j < cnt) fresh = hnsw_visit_sel<kLatency>(visited, lds_vis, vis_in_lds, vis_hash, word);
			const uint64_t fm = __ballot(fresh);
			if (fresh) nb_id[nfresh + __popcll(fm & ((1ull << lane) - 1))] = word;
			nfresh += __popcll(fm);
		}
		HN_SYNC();
		distances(nb_id, nfresh, nb_d);
		if constexpr (kFilter) {
			for (int j = lane; j < nfresh; j += 64) nb_del[j] = hnsw_hidden(p, nb_id[j]);
		} else if (!p.bare) {
			for (int j = lane; j < nfresh; j += 64) nb_del[j] = p.deleted[nb_id[j]];
		}
		ndist += nfresh;
		HN_SYNC();
		if (lane == 0) {   // sequential heap updates in neighbour order (runLayer0Step :932-960)
			for (int i = 0; i < nfresh; ++i) {
				const float d = nb_d[i];
				const uint32_t id = nb_id[i];
				if (top_n < int(p.ef) || lower > d) {
					if (uint64_t(cand_n) >= cand_cap) {
						overflow = true;
						break;
					}
					hp_emplace(cand, cand_n, -d, id);
					if (p.bare || !nb_del[i]) {
						if (top_n < int(p.ef)) {
							hp_emplace(top, top_n, d, id);
						} else {
							hp_replace_top(top, top_n, d, id);
						}
					}
					if (top_n) lower = hp_dist(top[0]);
				}
			}
		}
		HN_SYNC();
	}

	if (lane == 0) {
		if (overflow) {
			p.out_count[qi] = kHnswOverflow;
			if constexpr (!kGlobalCand) hnsw_enqueue_overflow(p, qi);
		} else {
			while (top_n > int(p.k)) hp_pop(top, top_n);   // SearchKnn :1998-2000
			for (int i = 0; i < top_n; ++i) {
				p.out_dist[size_t(qi) * p.k + i] = hp_dist(top[i]);
				p.out_row[size_t(qi) * p.k + i] = top[i].y;
			}
			p.out_count[qi] = uint32_t(top_n);
		}
		if (p.stats) {
			atomicAdd(&p.stats[0], ndist);
			atomicAdd(&p.stats[1], hops);
		}
	}
}

#undef HN_SYNC

// The other wavefronts of a team: distance batches until the driver says the search is over.
template <int kMetric, int NB, int kTeam>
__device__ __forceinline__ void hnsw_team_serve(const HnswParams& p, const HnswTeamBox* box) {
	extern __shared__ __attribute__((aligned(16))) unsigned char hnsw_lds[];
	const HnswLdsLayout at = hnsw_lds_layout(p.ef_cap, p.lds_cand_cap, false, NB, false);
	const float4* q_s = reinterpret_cast<const float4*>(reinterpret_cast<uint2*>(hnsw_lds) + at.top + at.cand);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	float4 qreg[1];
	for (;;) {
		__syncthreads();
		const int cnt = box->cnt;
		if (cnt < 0) return;
		int b0, n0;
		team_slice<kTeam>(cnt, wave, b0, n0);
		// (RXGPU_HNSW_NBL=1, an experiment that is OFF by default.)  The candidate expanded next is often one of the rows of THIS batch (a
		// neighbour that turns out nearer than everything in line), which the driver's one-hop-ahead prefetch cannot know.  So the link blocks of
		// the batch's rows come along with the rows and the next hop finds its block in LDS whichever row it pops.  MEASURED: 15 % of the hops
		// at 1M x 768 find their block this way, but the 16 extra 132-byte gathers a hop delay the row gathers behind them: one query 0.452 ->
		// 0.517 ms at 1M, 0.67 -> 1.05 ms at 10M rows, where every gather starts with a page walk and the walks are what a hop waits for
		// (profiles/rd6d_*_linkblocks.json).
		if (box->links && p.nbl_off) {
			uint32_t* nbl = reinterpret_cast<uint32_t*>(hnsw_lds + p.nbl_off);
			const int rows = cnt < kHnswNblRows ? cnt : kHnswNblRows;
			for (int j = wave - 1; j < rows; j += kTeam - 1) {
				const uint32_t* src = p.links0 + size_t(box->ids[j]) * (1 + p.maxM0) + (lane <= int(p.maxM0) ? lane : int(p.maxM0));
				__builtin_amdgcn_global_load_lds(src, (hnsw_lds_void*)(nbl + 64 * j), 4, 0, 0);
			}
		}
		if constexpr (NB > 12) {
			if (n0 > 0) batch_distances_wide<kMetric, NB, true>(p, q_s, box->ids + b0, n0, box->dists + b0, lane);
		} else {
			if (n0 > 0) batch_distances_fixed<kMetric, NB, true, true>(p, qreg, q_s, box->ids + b0, n0, box->dists + b0, lane);
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (a wavefront without rows of its own still has blocks in flight)
		__syncthreads();
	}
}
}  // namespace rxgpu
