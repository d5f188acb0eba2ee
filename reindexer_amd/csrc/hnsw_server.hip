// The resident HNSW search kernel (protocol: HnswServer, knn_kernels.hip.h; host side: rxgpu_hnsw_server.hip).
#include "hnsw_dispatch.hip.h"
#include "hnsw_search_core.hip.h"

namespace rxgpu {

// The RESIDENT form of the team search (HnswServer, knn_kernels.hip.h): the kernel stays on the chip and workgroup w serves the requests
// planner threads post into slot w of a mailbox in pinned host memory.  The reference's concurrency is T threads with one SearchKnn each
// (float_vector_index.cc:258-294); as launches that is T kernels, T completion signals and — between them — a batcher with its wake-ups:
// 9.9 k q/s at T = 16 over 10M rows where the reference's 16 cores make 18.6 k, although one search is as fast as one core's.  Served from
// the mailbox a call costs what the search costs.
//   * one writer per word (host: post, req, query, stop; device: done, leaving, results), sequence numbers instead of flags: nothing is
//     ever reset, a word is either old or new;
//   * the kernel always ends by itself: workgroup 0 decides — the host's stop word (the index is about to change), no request for
//     idle_ticks, or life_ticks since the start — writes the generation number to `leaving` and raises the leave flag the other workgroups
//     poll in device memory.  No wait in here depends on another kernel or on the host making progress;
//   * the next generation is an ordinary launch on the SAME stream: it starts when this one is gone, so a slot has one server at a time and
//     a request posted while a generation leaves is simply the next one's first.
// Three kernels speak this protocol: hnsw_server_kernel (float rows of 128, 512, 768 components, a team of four wavefronts a slot),
// hnsw_server_wide_kernel (the same body over rows of 1024 and 1536 floats, read in chunks) and hnsw_server_sq8_kernel (SQ8 codes, one
// wavefront a slot).

// Lane 0 of a slot waits for the slot's next request or for the kernel's end and leaves the verdict in s_cmd: [0] 1 = a request, 2 = leave;
// [1] its sequence number; [2] k; [3] ef.  Shared by the two resident kernels below: the protocol is one.
__device__ __forceinline__ void server_await(const HnswServer& sv, uint32_t slot, uint32_t last, unsigned long long t_start, uint32_t* s_cmd) {
	uint32_t cmd = 0u, seq = last, quiet = 0u;
	while (!cmd) {
		seq = __hip_atomic_load(&sv.post[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		if (seq != last) {
			cmd = 1u;
			break;
		}
		const unsigned long long now = wall_clock64();
		if (slot == 0u) {
			const unsigned long long seen = __hip_atomic_load(&sv.dev[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			const unsigned long long since = seen > t_start ? seen : t_start;
			if (__hip_atomic_load(sv.stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u || now - t_start > sv.life_ticks ||
				(now > since && now - since > sv.idle_ticks)) {
				__hip_atomic_store(sv.leaving, sv.generation, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
				__hip_atomic_store(&sv.dev[0], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
				cmd = 2u;
			}
		} else if (__hip_atomic_load(&sv.dev[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull || now - t_start > 2ull * sv.life_ticks) {
			cmd = 2u;   // (twice the lifetime: workgroup 0 never came to decide — e.g. it was not resident yet; the kernel ends anyway)
		}
		// every look is a read across PCIe: close together while requests keep coming, ~7 us apart once the slot has been quiet for a while
		if (!cmd) {
			if (++quiet < 64u) {
				__builtin_amdgcn_s_sleep(24);
			} else {
				__builtin_amdgcn_s_sleep(127);
				__builtin_amdgcn_s_sleep(127);
			}
		}
	}
	if (cmd == 1u) {
		s_cmd[2] = __hip_atomic_load(&sv.req[2 * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		s_cmd[3] = __hip_atomic_load(&sv.req[2 * slot + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		(void)__hip_atomic_fetch_max(&sv.dev[1], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
	s_cmd[1] = seq;
	s_cmd[0] = cmd;
}
// the parameters of the search a slot runs for the request in s_cmd: k, ef, the slot's result arrays (its query: the caller)
__device__ __forceinline__ HnswParams server_slot_params(const HnswParams& p, const HnswServer& sv, uint32_t slot, const uint32_t* s_cmd) {
	HnswParams pl = p;
	pl.k = s_cmd[2];
	pl.ef = s_cmd[3];
	pl.out_dist = p.out_dist + size_t(slot) * sv.kcap;
	pl.out_row = p.out_row + size_t(slot) * sv.kcap;
	pl.out_count = p.out_count + slot;
	return pl;
}
// lane 0, behind the release fence over the slot's result stores: the answer
__device__ __forceinline__ void server_answer(const HnswServer& sv, uint32_t slot, uint32_t seq, unsigned long long t_search) {
	__hip_atomic_store(&sv.took[slot], uint32_t(wall_clock64() - t_search), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	__hip_atomic_store(&sv.done[slot], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The body of the resident float kernels (hnsw_server_kernel, and hnsw_server_wide_kernel for the rows served in chunks): one protocol, one code.
template <int kMetric, int NB, int kSorted, bool kDel, int kTeam>
__device__ __forceinline__ void hnsw_server_body(const HnswParams& p, const HnswServer& sv) {
	__shared__ HnswTeamBox box;
	__shared__ uint32_t s_cmd[4];
	const uint32_t slot = blockIdx.x;
	if (threadIdx.x >= 64) {   // the other wavefronts of the team: distance batches of every search until the workgroup leaves
		for (;;) {
			__syncthreads();
			if (s_cmd[0] == 2u) return;
			hnsw_team_serve<kMetric, NB, kTeam>(p, &box);
		}
	}
	const int lane = threadIdx.x;
	const unsigned long long t_start = wall_clock64();
	uint32_t last = __hip_atomic_load(&sv.done[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // the host keeps it across generations
	for (;;) {
		if (lane == 0) server_await(sv, slot, last, t_start, s_cmd);
		__syncthreads();
		if (s_cmd[0] == 2u) return;
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");   // the query the host wrote in front of the sequence number, not a cached line of the slot's last one
		const uint32_t seq = s_cmd[1];
		const unsigned long long t_search = wall_clock64();
		HnswParams pl = server_slot_params(p, sv, slot, s_cmd);
		pl.queries = p.queries + size_t(slot) * p.dim;
		hnsw_search_one<kMetric, false, NB, true, false, kSorted, kDel, kTeam>(pl, slot, 0u, &box);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // this wavefront's result stores are out before the sequence number
		if (lane == 0) {
			server_answer(sv, slot, seq, t_search);
			box.cnt = -1;
		}
		last = seq;
		__syncthreads();   // the team leaves hnsw_team_serve
	}
}
template <int kMetric, int NB, int kSorted, bool kDel, int kTeam>
__global__ __launch_bounds__(64 * kTeam) void hnsw_server_kernel(HnswParams p, HnswServer sv) {
	hnsw_server_body<kMetric, NB, kSorted, kDel, kTeam>(p, sv);
}
// rows of 1024 and 1536 floats (NB = 16, 24: batch_distances_wide)
template <int kMetric, int NB, int kSorted, bool kDel, int kTeam>
__global__ __launch_bounds__(64 * kTeam) void hnsw_server_wide_kernel(HnswParams p, HnswServer sv) {
	static_assert(NB > 12, "the narrower rows are hnsw_server_kernel's");
	hnsw_server_body<kMetric, NB, kSorted, kDel, kTeam>(p, sv);
}

// The same mailbox over the SQ8 codes of a quantised graph.  A slot is ONE wavefront (the team form serves float rows only: a 768-byte code row
// is a quarter of a float row's gather, and nobody has measured four wavefronts over it).  The slot's query is dim code bytes (padded to 16), one
// corrective offset and one normCoef; hnsw_search_one pulls all three into registers in its prologue and never looks at the mailbox again.
// Class 0 keeps the visited set in LDS (kLatency: the hash set behind the heaps, 2^14 words — what a launch of that ef gets in HBM).
template <int kMetric, int NB, int kSorted, bool kDel>
__global__ __launch_bounds__(64) void hnsw_server_sq8_kernel(HnswParams p, HnswServer sv) {
	static_assert(NB > 0, "the generic SQ8 form re-reads the query codes at every distance batch: not over a mailbox");
	__shared__ uint32_t s_cmd[4];
	const uint32_t slot = blockIdx.x;
	const int lane = threadIdx.x;
	const unsigned long long t_start = wall_clock64();
	uint32_t last = __hip_atomic_load(&sv.done[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	for (;;) {
		if (lane == 0) server_await(sv, slot, last, t_start, s_cmd);
		__syncthreads();
		if (s_cmd[0] == 2u) return;
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
		const uint32_t seq = s_cmd[1];
		const unsigned long long t_search = wall_clock64();
		HnswParams pl = server_slot_params(p, sv, slot, s_cmd);
		pl.qcodes = p.qcodes + size_t(slot) * hnsw_server_sq8_record(p.dim);
		pl.qcorr = p.qcorr + slot;
		pl.qnorm = p.qnorm + slot;
		hnsw_search_one<kMetric, false, NB, true, true, kSorted, kDel, 1>(pl, slot, 0u);
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
		if (lane == 0) server_answer(sv, slot, seq, t_search);
		last = seq;
		__syncthreads();   // s_cmd is read by every lane before lane 0 writes the next verdict
	}
}

// dynamic LDS of a float server workgroup (pick_hnsw_server: what its first gate measures, whatever the row format)
size_t hnsw_server_lds_bytes(const HnswParams& p) {
	HnswPickInput in = hnsw_pick_input(p, 0u, false);
	in.sq8 = false;
	return pick_hnsw_server(in).lds_bytes;
}
// the embedding sizes with a fixed-dimension SQ8 distance batch (hnsw_distance_blocks.h): six for a bare graph, two with deleted nodes
bool hnsw_server_sq8_serves(uint32_t dim, bool bare) {
	HnswPickInput in{};
	in.dim = dim;
	in.bare = bare;
	in.sq8 = true;
	return pick_hnsw_server(in).nb != 0;
}
// The resident kernel of a mailbox (pick_hnsw_server has the classes and the gates); false: this call has no resident form.
bool launch_hnsw_server(int metric, const HnswParams& p, const HnswServer& sv, uint32_t slots, hipStream_t s) {
	const HnswKernelPick k = pick_hnsw_server(hnsw_pick_input(p, slots, false));
	if (!k.served) return false;
	const HnswParams pk = hnsw_patched(p, k);
	const bool launched = with_metric(metric, [&](auto m) {
		return with_int<2, 6, 8, 12, 16, 24>(k.nb, [&](auto nb) {
			return with_int<2, 4>(k.sorted, [&](auto sorted) {
				return with_bool(k.del, [&](auto del) {
					constexpr int M = decltype(m)::value, NB = decltype(nb)::value, S = decltype(sorted)::value;
					constexpr bool D = decltype(del)::value;
					if (k.family == kHnswServerSq8) {
						if constexpr (hnsw_server_kernel_exists(NB, true, S, D)) return hnsw_launch<&hnsw_server_sq8_kernel<M, NB, S, D>>(k, slots, s, pk, sv);
						return false;
					}
					if constexpr (!hnsw_server_kernel_exists(NB, false, S, D)) {
						return false;
					} else if constexpr (NB > 12) {
						return hnsw_launch<&hnsw_server_wide_kernel<M, NB, S, D, 4>>(k, slots, s, pk, sv);
					} else {
						return hnsw_launch<&hnsw_server_kernel<M, NB, S, D, 4>>(k, slots, s, pk, sv);
					}
				});
			});
		});
	});
	if (!launched) hnsw_no_kernel("server", metric, k);
	return true;
}


}  // namespace rxgpu
