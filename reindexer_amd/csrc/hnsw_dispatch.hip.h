// From a pick (hnsw_kernel_pick.h) to a launch: the one mechanism that turns runtime values into template arguments, shared by
// hnsw_search.hip and hnsw_server.hip.  with_metric / with_int / with_bool call f with the value as a std::integral_constant and answer what
// f answered — false when the value is not in the list or f had no kernel for it, which the launchers treat as a host error.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "hnsw_kernel_pick.h"
#include "knn_kernels.hip.h"

namespace rxgpu {

template <int... kValues, class F>
inline bool with_int(int v, F&& f) {
	return ((v == kValues && f(std::integral_constant<int, kValues>{})) || ...);
}
template <class F>
inline bool with_bool(bool v, F&& f) {
	return v ? f(std::true_type{}) : f(std::false_type{});
}
template <class F>
inline bool with_metric(int metric, F&& f) {
	switch (metric) {
		case kL2: return f(std::integral_constant<int, kL2>{});
		case kIP: return f(std::integral_constant<int, kIP>{});
		default: return f(std::integral_constant<int, kCos>{});
	}
}

// what the pick functions read of a launch
inline HnswPickInput hnsw_pick_input(const HnswParams& p, uint32_t blocks, bool global_cand) {
	HnswPickInput in{};
	in.dim = p.dim;
	in.ef = p.ef;
	in.ef_cap = p.ef_cap;
	in.lds_cand_cap = p.lds_cand_cap;
	in.sorted = p.sorted != 0;
	in.bare = p.bare != 0;
	in.sq8 = p.codes != nullptr;
	in.team = p.team;
	in.team_max = p.team_max;
	in.vis_lds = p.vis_lds;
	in.vis_lds_log2 = p.vis_lds_log2;
	in.vis_hash_log2 = p.vis_hash_log2;
	in.has_visited = p.visited != nullptr;
	in.sq8_query = p.corr && p.qcodes && p.qcorr && p.qnorm;
	in.nbl = p.nbl;
	in.spec = p.spec;
	in.maxM0 = p.maxM0;
	in.blocks = blocks;
	in.global_cand = global_cand;
	return in;
}
// the launch's parameters: the caller's with the fields the pick decides
inline HnswParams hnsw_patched(const HnswParams& p, const HnswKernelPick& k) {
	HnswParams pk = p;
	pk.vis_lds = k.vis_lds;
	pk.vis_hash_log2 = k.vis_hash_log2;
	pk.nbl_off = k.nbl_off;
	pk.spec_off = k.spec_off;
	return pk;
}

// one launch of the instantiation kKernel as the pick sizes it (the record of the devices whose LDS limit was raised is per instantiation)
template <auto kKernel, class... Args>
inline bool hnsw_launch(const HnswKernelPick& k, uint32_t grid, hipStream_t s, const Args&... args) {
	static std::atomic<uint64_t> raised{0};
	if (k.needs_raised_lds) (void)raise_dynamic_lds_once(raised, reinterpret_cast<const void*>(kKernel), kHnswLdsRaised);
	hipLaunchKernelGGL(kKernel, dim3(grid), dim3(k.threads), k.lds_bytes, s, args...);
	return true;
}
// a pick outside the instantiated set is a bug in hnsw_kernel_pick.h: no other kernel stands in for it
[[noreturn]] inline void hnsw_no_kernel(const char* what, int metric, const HnswKernelPick& k) {
	std::fprintf(stderr, "rxgpu: no %s kernel for metric %d family %d nb %d sorted %d del %d latency %d sq8 %d global_cand %d\n", what, metric, int(k.family), k.nb,
				 k.sorted, int(k.del), int(k.latency), int(k.sq8), int(k.global_cand));
	std::abort();
}

}  // namespace rxgpu
