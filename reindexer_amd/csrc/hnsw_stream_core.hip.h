// The body of one ContinueStreamingSearch (cpp_src/core/index/float_vector/hnswlib/hnswalg.h:1945-1975) on gfx950, shared by the kernel
// that runs one call per launch (hnsw_stream.hip) and the one that runs a whole collection under an allowed-rows bitmap
// (hnsw_stream_collect.hip): the heap primitives, the session's heaps in LDS or in the session's global arrays, mergeExtrasIntoTopCandidates
// (:1893-1926), the step loop (layer0ShouldStopBeforePop :865-868, runLayer0Step :882-893, 939-940) and emitStreamingBatch (:1928-1945).
//
// One wavefront drives one session.  Heap updates are dependent single-lane accesses: lane 0 executes them and lane 0 alone knows the
// heaps' sizes — the other lanes learn what they need through the workgroup's shared words (StreamShared).
#pragma once

#include "knn_kernels.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

namespace {

struct Heap {
	float* d;
	uint32_t* i;
	int n;
};
// PriorityQueue<pair<float,tableint>, vector, CompareByFirst> (priority_queue.h:7-152, hnswalg.h:581-585), executed by ONE lane
__device__ __forceinline__ void sh_sift_up(Heap& h, int child) {
	const float vd = h.d[child];
	const uint32_t vi = h.i[child];
	while (child > 0) {
		const int parent = (child - 1) / 2;
		if (!(h.d[parent] < vd)) break;
		h.d[child] = h.d[parent];
		h.i[child] = h.i[parent];
		child = parent;
	}
	h.d[child] = vd;
	h.i[child] = vi;
}
__device__ __forceinline__ void sh_sift_down(Heap& h, int parent, int size) {
	const float vd = h.d[parent];
	const uint32_t vi = h.i[parent];
	for (;;) {
		const int left = parent * 2 + 1;
		if (left >= size) break;
		int best = left;
		const int right = left + 1;
		if (right < size && h.d[left] < h.d[right]) best = right;
		if (!(vd < h.d[best])) break;
		h.d[parent] = h.d[best];
		h.i[parent] = h.i[best];
		parent = best;
	}
	h.d[parent] = vd;
	h.i[parent] = vi;
}
__device__ __forceinline__ void sh_emplace(Heap& h, float vd, uint32_t vi) {
	h.d[h.n] = vd;
	h.i[h.n] = vi;
	++h.n;
	if (h.n >= 2) sh_sift_up(h, h.n - 1);
}
__device__ __forceinline__ void sh_pop(Heap& h) {
	if (h.n >= 2) {
		const float td = h.d[0];
		const uint32_t ti = h.i[0];
		h.d[0] = h.d[h.n - 1];
		h.i[0] = h.i[h.n - 1];
		h.d[h.n - 1] = td;
		h.i[h.n - 1] = ti;
		if (h.n > 2) sh_sift_down(h, 0, h.n - 1);
	}
	--h.n;
}
__device__ __forceinline__ void sh_replace_top(Heap& h, float vd, uint32_t vi) {
	h.d[0] = vd;
	h.i[0] = vi;
	sh_sift_down(h, 0, h.n);
}

template <int kMetric>
__device__ __forceinline__ void stream_distances(const HnswParams& p, const HnswStream& s, const float* q, const uint32_t* ids, int cnt, float* dists,
												 int lane) {
	if (p.codes) {   // quantised graph (HierarchicalNSWImpl<uint8_t>): the same session over codes — wave-uniform branch
		batch_distances_sq8<kMetric>(p, s.qcodes, s.qcorr, s.qnorm, ids, cnt, dists, lane);
		return;
	}
	const int m = lane & 15, g = lane >> 4;
	for (int base = 0; base < cnt; base += kRowsPerWave) {
		const int idx = base + g;
		const bool ok = idx < cnt;
		const uint64_t row = ids[ok ? idx : base];
		const float sum = group_distance_generic<kMetric>(p.rows + row * p.stride, q, p.dim, m);
		const float dist = 1.0f * metric_epilogue<kMetric>(sum, p.inv_norms, row);
		if (ok && m == 0) dists[idx] = dist;
	}
}

constexpr size_t kStreamLdsBytes = size_t(2 * kStreamLdsTop + 2 * kStreamLdsExt + kStreamLdsCand) * 8;   // the staged heaps: 57 344 bytes

// the workgroup's shared words (declared by the kernel)
struct StreamShared {
	uint32_t* nb_id;   // [kHnswMaxNeighbors]
	float* nb_d;       // [kHnswMaxNeighbors]
	uint32_t* cur;
	int* flag;
	int* n;            // [3]
};

// The session's three heaps as one call sees them.  Sizes, selectors and the lower bound are lane 0's.  top / ext point at two Heaps each,
// locals of the kernel (RX_STREAM_HEAPS): they are the only part indexed by a selector, and kept apart everything else stays in registers.
struct StreamHeaps {
	Heap* top;
	Heap* ext;
	Heap cand;
	uint32_t tsel, esel;
	uint32_t cap_top, cap_ext, cap_cand;
	float lower;
};

// BeginStreamingSearch on the device (hnswalg.h:1865-1891): getLayer0EntryPoint (:799-827), then initLayer0SearchState with its streaming
// branch — the entry point only enters candidate_set.  The visited set is zeroed by the host.  Called by every lane; the state it leaves in
// *st and in the session's global arrays is visible to the workgroup behind the next __syncthreads.
template <int kMetric>
__device__ __forceinline__ void stream_begin(const HnswParams& p, const HnswStream& s, const float* q, HnswStreamState* st, const StreamShared& sh, int lane) {
	uint32_t cur = p.entry;
	if (lane == 0) sh.nb_id[0] = cur;
	__syncthreads();
	stream_distances<kMetric>(p, s, q, sh.nb_id, 1, sh.nb_d, lane);
	__syncthreads();
	float curdist = sh.nb_d[0];
	for (int level = p.maxlevel; level > 0; --level) {
		bool changed = true;
		while (changed) {
			__syncthreads();
			const uint32_t* ll = p.upper + (p.upper_off[cur] + uint64_t(level - 1)) * (1 + p.M);
			const int cnt = int(ll[0]);
			for (int j = lane; j < cnt; j += 64) sh.nb_id[j] = ll[1 + j];
			__syncthreads();
			stream_distances<kMetric>(p, s, q, sh.nb_id, cnt, sh.nb_d, lane);
			__syncthreads();
			changed = false;
			for (int i = 0; i < cnt; ++i) {
				const float d = sh.nb_d[i];
				if (d < curdist) {
					curdist = d;
					cur = sh.nb_id[i];
					changed = true;
				}
			}
		}
	}
	if (lane == 0) {
		const bool ep_ok = p.bare || !p.deleted[cur];
		const float lower = ep_ok ? curdist : 3.402823466e+38f;
		s.cand_d[0] = -lower;
		s.cand_i[0] = cur;
		s.visited[cur >> 5] |= 1u << (cur & 31);
		st->cand_n = 1;
		st->top_n = 0;
		st->ext_n = 0;
		st->lower = lower;
		st->top_sel = 0;
		st->ext_sel = 0;
		st->status = kStreamOk;
		st->out_count = 0;
		st->exhausted = 0;
	}
}

#define RX_STREAM_HEAPS(h)          \
	Heap h##_top[2], h##_ext[2];    \
	StreamHeaps h;                  \
	h.top = h##_top;                \
	h.ext = h##_ext

// kLds: the heaps are staged into `lds` (kStreamLdsBytes; the launcher guarantees the sizes fit) and the current ones land in slot 0; else
// they are the session's global arrays.
template <bool kLds>
__device__ __forceinline__ void stream_attach(StreamHeaps& h, const HnswStream& s, const HnswStreamState* st, unsigned char* lds, int lane) {
	h.cap_top = kLds ? uint32_t(kStreamLdsTop) : s.cap;
	h.cap_ext = kLds ? uint32_t(kStreamLdsExt) : s.cap;
	h.cap_cand = kLds ? uint32_t(kStreamLdsCand) : s.cap;
	h.tsel = st->top_sel;
	h.esel = st->ext_sel;
	if constexpr (kLds) {
		float* f = reinterpret_cast<float*>(lds);
		h.top[0] = Heap{f, reinterpret_cast<uint32_t*>(f + kStreamLdsTop), 0};
		f += 2 * kStreamLdsTop;
		h.top[1] = Heap{f, reinterpret_cast<uint32_t*>(f + kStreamLdsTop), 0};
		f += 2 * kStreamLdsTop;
		h.ext[0] = Heap{f, reinterpret_cast<uint32_t*>(f + kStreamLdsExt), 0};
		f += 2 * kStreamLdsExt;
		h.ext[1] = Heap{f, reinterpret_cast<uint32_t*>(f + kStreamLdsExt), 0};
		f += 2 * kStreamLdsExt;
		h.cand = Heap{f, reinterpret_cast<uint32_t*>(f + kStreamLdsCand), 0};
		const int tn = st->top_n, en = st->ext_n, cn = st->cand_n;
		const float* gtd = s.top_d + size_t(h.tsel) * s.cap;
		const uint32_t* gti = s.top_i + size_t(h.tsel) * s.cap;
		const float* ged = s.ext_d + size_t(h.esel) * s.cap;
		const uint32_t* gei = s.ext_i + size_t(h.esel) * s.cap;
		for (int j = lane; j < tn; j += 64) {
			h.top[0].d[j] = gtd[j];
			h.top[0].i[j] = gti[j];
		}
		for (int j = lane; j < en; j += 64) {
			h.ext[0].d[j] = ged[j];
			h.ext[0].i[j] = gei[j];
		}
		for (int j = lane; j < cn; j += 64) {
			h.cand.d[j] = s.cand_d[j];
			h.cand.i[j] = s.cand_i[j];
		}
		h.tsel = 0;
		h.esel = 0;
		h.top[0].n = tn;
		h.ext[0].n = en;
		h.cand.n = cn;
		__syncthreads();
	} else {
		for (int k = 0; k < 2; ++k) {
			h.top[k] = Heap{s.top_d + size_t(k) * s.cap, s.top_i + size_t(k) * s.cap, 0};
			h.ext[k] = Heap{s.ext_d + size_t(k) * s.cap, s.ext_i + size_t(k) * s.cap, 0};
		}
		h.cand = Heap{s.cand_d, s.cand_i, st->cand_n};
		h.top[h.tsel].n = st->top_n;
		h.ext[h.esel].n = st->ext_n;
	}
	h.lower = st->lower;
}

// mergeExtrasIntoTopCandidates (hnswalg.h:1893-1926), lane 0.  Returns the call's status.
__device__ __forceinline__ uint32_t stream_merge_extras(StreamHeaps& h, int ef) {
	uint32_t status = kStreamOk;
	Heap& T = h.top[h.tsel];
	if (!(T.n >= ef || h.ext[h.esel].n == 0)) {
		if (T.n) {
			Heap& te = h.ext[h.esel];
			Heap& ne = h.ext[h.esel ^ 1];
			ne.n = 0;
			const int need = ef - T.n;
			int delta = te.n > need ? te.n - need : 0;
			while (delta-- > 0) {
				sh_emplace(ne, te.d[0], te.i[0]);
				sh_pop(te);
			}
			while (te.n && T.n < ef) {
				sh_emplace(T, te.d[0], te.i[0]);
				sh_pop(te);
			}
			h.esel ^= 1;
		} else {
			// top_candidates = move(extras): the array (heap layout included) becomes the top heap
			Heap& E = h.ext[h.esel];
			if (uint32_t(E.n) > h.cap_top) {
				status = kStreamError;   // unreachable: the launcher stages in LDS only when kStreamLdsExt <= kStreamLdsTop holds the heap
			} else {
				for (int j = 0; j < E.n; ++j) {
					T.d[j] = E.d[j];
					T.i[j] = E.i[j];
				}
				T.n = E.n;
				E.n = 0;
				while (T.n > ef) {
					sh_emplace(E, T.d[0], T.i[0]);
					sh_pop(T);
				}
			}
		}
		if (T.n) h.lower = T.d[0];
	}
	return status;
}

// The step loop of a call with its ef: 1 = layer0ShouldStopBeforePop fired (the call emits next), 2 = (kLds) a step would outgrow the LDS
// heaps — stopped at a step boundary, the global variant resumes.  Every node enters candidate_set once (the visited test-and-set), so the
// loop ends after at most N pops.
template <int kMetric, bool kLds>
__device__ __forceinline__ int stream_steps(const HnswParams& p, const HnswStream& s, const float* q, StreamHeaps& h, int ef, const StreamShared& sh, int lane) {
	for (;;) {
		if (lane == 0) {
			Heap& T = h.top[h.tsel];
			int flag = 0;
			if (h.cand.n == 0) {
				flag = 1;
			} else {
				const float cdist = -h.cand.d[0];
				if (cdist > h.lower && T.n >= ef) {   // streaming: never the bare-bone shortcut (hnswalg.h:865-868)
					flag = 1;
				} else if (kLds && (uint32_t(h.cand.n) + p.maxM0 > h.cap_cand || uint32_t(h.ext[h.esel].n) + 1 > h.cap_ext)) {
					flag = 2;   // stop at a step boundary; the global variant resumes
				} else {
					const uint32_t id = h.cand.i[0];
					sh_pop(h.cand);
					if (p.bare || !p.deleted[id]) {   // hnswalg.h:882-893
						if (T.n < ef) {
							sh_emplace(T, cdist, id);
						} else if (h.lower > cdist) {
							const float od = T.d[0];
							const uint32_t oi = T.i[0];
							sh_replace_top(T, cdist, id);
							sh_emplace(h.ext[h.esel], od, oi);
						}
						h.lower = T.d[0];
					}
					*sh.cur = id;
				}
			}
			*sh.flag = flag;
		}
		__syncthreads();
		const int flag = *sh.flag;
		if (flag) return flag;
		const uint32_t node = *sh.cur;
		const uint32_t* ll = p.links0 + size_t(node) * (1 + p.maxM0);
		const int cnt = int(ll[0]);
		int nfresh = 0;
		for (int base = 0; base < cnt; base += 64) {
			const int j = base + lane;
			bool fresh = false;
			uint32_t id = 0;
			if (j < cnt) {
				id = ll[1 + j];
				const uint32_t bit = 1u << (id & 31);
				fresh = !(atomicOr(&s.visited[id >> 5], bit) & bit);
			}
			const uint64_t fm = __ballot(fresh);
			if (fresh) sh.nb_id[nfresh + __popcll(fm & ((1ull << lane) - 1))] = id;
			nfresh += __popcll(fm);
		}
		__syncthreads();
		stream_distances<kMetric>(p, s, q, sh.nb_id, nfresh, sh.nb_d, lane);
		__syncthreads();
		if (lane == 0) {
			for (int i = 0; i < nfresh; ++i) sh_emplace(h.cand, -sh.nb_d[i], sh.nb_id[i]);   // streaming: every evaluated node (hnswalg.h:939-940)
		}
		__syncthreads();
	}
}

// emitStreamingBatch (hnswalg.h:1928-1945), lane 0: the `batch` best of top_candidates leave in pop order into out_dist / out_row (room for
// min(batch, top_candidates) entries).  Returns how many; *exhausted as ContinueStreamingSearch reports it (:1973).
__device__ __forceinline__ uint32_t stream_emit(StreamHeaps& h, uint32_t batch, float* out_dist, uint32_t* out_row, uint32_t* exhausted) {
	uint32_t emitted = 0;
	Heap& A = h.top[h.tsel];
	Heap& B = h.top[h.tsel ^ 1];
	B.n = 0;
	while (A.n > int(batch)) {
		sh_emplace(B, A.d[0], A.i[0]);
		sh_pop(A);
	}
	while (A.n > 0) {
		out_dist[emitted] = A.d[0];
		out_row[emitted] = A.i[0];
		++emitted;
		sh_pop(A);
	}
	h.tsel ^= 1;
	*exhausted = (h.cand.n == 0 && h.top[h.tsel].n == 0 && h.ext[h.esel].n == 0) ? 1u : 0u;
	return emitted;
}

// The end of a launch: lane 0 records the heaps' sizes, selectors and the lower bound in the session's state; staged heaps are written back
// into slot 0 of the session's arrays.  Called by every lane.
template <bool kLds>
__device__ __forceinline__ void stream_detach(const StreamHeaps& h, const HnswStream& s, HnswStreamState* st, const StreamShared& sh, int lane) {
	if (lane == 0) {
		st->lower = h.lower;
		st->cand_n = h.cand.n;
		st->top_n = h.top[h.tsel].n;
		st->ext_n = h.ext[h.esel].n;
		if constexpr (!kLds) {
			st->top_sel = h.tsel;
			st->ext_sel = h.esel;
		} else {
			st->top_sel = 0;
			st->ext_sel = 0;
		}
		*sh.cur = h.tsel | (h.esel << 1);
		sh.n[0] = h.top[h.tsel].n;
		sh.n[1] = h.ext[h.esel].n;
		sh.n[2] = h.cand.n;
	}
	__syncthreads();
	if constexpr (kLds) {   // stage out into slot 0 of the session arrays
		const uint32_t sel = *sh.cur;
		const Heap& T = h.top[sel & 1];
		const Heap& E = h.ext[(sel >> 1) & 1];
		const int tn = sh.n[0], en = sh.n[1], cn = sh.n[2];
		for (int j = lane; j < tn; j += 64) {
			s.top_d[j] = T.d[j];
			s.top_i[j] = T.i[j];
		}
		for (int j = lane; j < en; j += 64) {
			s.ext_d[j] = E.d[j];
			s.ext_i[j] = E.i[j];
		}
		for (int j = lane; j < cn; j += 64) {
			s.cand_d[j] = h.cand.d[j];
			s.cand_i[j] = h.cand.i[j];
		}
	}
}

}  // namespace

}  // namespace rxgpu
