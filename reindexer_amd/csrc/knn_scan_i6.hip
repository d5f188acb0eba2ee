// The 6-bit front of the int8-pruned single-query chain (forced with RXGPU_SCAN_I6=1, automatic where scan_policy_i6 of rxgpu_knn_chains.hip
// says so): 0.75 bytes per element from HBM instead of one, the SAME result bits.  The chain is the int8 tier's (knn_scan_i8.hip) with two more
// launches in front of the scan:
//   0. knn_query_prep_i8   unchanged, with the margin taken from the 6-bit residual maxima
//   1. knn_scan_i6 (seed)  the first set of 16 rows of every set_step sets, about 65 536 rows: per-workgroup top-kk of up_r, nothing emitted
//   2. knn_merge_lists     -> T_seed, the kk-th smallest up_r of the sample (+inf with fewer than kk sampled rows)
//   3. knn_scan_i6         every row: S_r from the 6-bit shadow, the window [lo_r, up_r] of i8_bounds, up_r into the per-wave top-kk; {lo_r, r}
//                          is emitted when lo_r <= min(thr of the wavefront, T_seed) + margin
//   4. knn_merge_lists -> T, knn_filter_emitted_wide (knn_filter.hip: knn_filter_emitted's test with one atomic per workgroup), knn_rescore, the gated
//      exact scan, knn_merge_final: as behind knn_scan_i8
// Why the seed: with 6-bit codes the per-row window is four times as wide as the int8 one, and a wavefront's own running threshold stays loose
// for so long that it would emit in nearly every step; a store per step costs the scan its bandwidth.  T_seed is tight from the first row.
// Why it is sound: T (step 4) is the kk-th smallest up_r of ALL rows; the kk-th smallest of any subset - the wavefront's own rows so far, the
// sample - is >= T, f32 addition is monotone, so lo_r <= T + margin implies lo_r <= min(thr, T_seed) + margin: the emitted rows are a
// superset of the candidates whatever the sample holds.  Only their NUMBER depends on the sample, which is why it is strided over the index.
// Arithmetic, layout and the (inherited) bound: knn_i6_quant.h.  The mapping is knn_scan_i8's: a 16-lane group owns the tile of rows
// 4 g ... 4 g + 3 of a set of 16, three 16-byte loads per lane and 256-dimension chunk (9 per step at 768 dims against 12), double-buffered;
// the transposing butterfly, the per-wave top-kk, the segments of knn_emit_plan.h and block_merge_and_store are shared.  No atomics in the scan.
#include <algorithm>
#include <cstdlib>

#include "knn_emit_plan.h"
#include "knn_i6_quant.h"
#include "knn_kernels.hip.h"
#include "knn_scan_common.hip.h"
#include "rxgpu_internal.h"

namespace rxgpu {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kI6RowsPerGroup = int(kI6TileRows);
constexpr uint64_t kI6RowsPerWave = 4 * kI6RowsPerGroup;
static_assert(kI6RowsPerWave == kEmitRowsPerSet && kScanWaves == int(kEmitWavesPerBlock), "knn_emit_plan.h lays the segments out for this mapping");

// this lane's share of dot(t, u) for 16 codes of one row: words w0, w1 (nibbles) and z (2-bit plane), t = 128 h + l
__device__ __forceinline__ void i6_dot16(uint32_t w0, uint32_t w1, uint32_t z, const u32x4& qh, const u32x4& ql, int& hs, int& ls) {
	uint32_t c0, c1, c2, c3;
	i6_unpack16(w0, w1, z, c0, c1, c2, c3);
	hs = __builtin_amdgcn_sdot4(int(qh.x), int(c0), hs, false);
	ls = __builtin_amdgcn_sdot4(int(ql.x), int(c0), ls, false);
	hs = __builtin_amdgcn_sdot4(int(qh.y), int(c1), hs, false);
	ls = __builtin_amdgcn_sdot4(int(ql.y), int(c1), ls, false);
	hs = __builtin_amdgcn_sdot4(int(qh.z), int(c2), hs, false);
	ls = __builtin_amdgcn_sdot4(int(ql.z), int(c2), ls, false);
	hs = __builtin_amdgcn_sdot4(int(qh.w), int(c3), hs, false);
	ls = __builtin_amdgcn_sdot4(int(ql.w), int(c3), ls, false);
}

// NC = ld6 / 256.  kEmit: the full pass of a search (p.set_step == 1, e.plan = emit_plan(n, gridDim.x)); !kEmit: the seed pass, or a pass that only
// keeps.  kKeep: lo of every scanned row goes to p.lower as well (a recording call).
template <int kMetric, int NC, bool kEmit, bool kKeep>
__global__ __launch_bounds__(kScanThreads) void knn_scan_i6(ScanI6Params p, ScanI8Emit e) {
	const int lane = threadIdx.x & 63, m = lane & 15, g = lane >> 4;
	const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t qi = blockIdx.y;
	u32x4 qh[NC], ql[NC];
	int tsum = 0;   // sum(t) over the group's 16 lanes = over the whole (zero padded) query
	{
		const u32x4* ph = reinterpret_cast<const u32x4*>(p.planes + size_t(qi) * 2 * p.ld6);
		int hs = 0, ls = 0;
#pragma unroll
		for (int t = 0; t < NC; ++t) {
			qh[t] = ph[m + 16 * t];
			ql[t] = ph[16 * NC + m + 16 * t];
			const int one = 0x01010101;
			hs = __builtin_amdgcn_sdot4(int(qh[t].x), one, hs, false);
			hs = __builtin_amdgcn_sdot4(int(qh[t].y), one, hs, false);
			hs = __builtin_amdgcn_sdot4(int(qh[t].z), one, hs, false);
			hs = __builtin_amdgcn_sdot4(int(qh[t].w), one, hs, false);
			ls = __builtin_amdgcn_sdot4(int(ql[t].x), one, ls, false);
			ls = __builtin_amdgcn_sdot4(int(ql[t].y), one, ls, false);
			ls = __builtin_amdgcn_sdot4(int(ql[t].z), one, ls, false);
			ls = __builtin_amdgcn_sdot4(int(ql[t].w), one, ls, false);
		}
		tsum = hs * 128 + ls;
		tsum += __shfl_xor(tsum, 1);
		tsum += __shfl_xor(tsum, 2);
		tsum += __shfl_xor(tsum, 4);
		tsum += __shfl_xor(tsum, 8);
	}
	const float2 qinfo = p.qinfo[qi];   // {s_q, |q| rounded up}
	float qq = 0.f;
	if constexpr (kMetric == kL2) qq = p.q_sq[qi];
	WaveTopK top;
	top.init(p.sp.kk);
	float* lower = p.lower + size_t(qi) * p.sp.n;
	const uint64_t n = p.sp.n;
	const uint64_t step = p.set_step;
	const uint64_t nsets_all = (n + kI6RowsPerWave - 1) / kI6RowsPerWave;
	const uint64_t nsets = (nsets_all + step - 1) / step;   // sets this pass scans: set s is set s * step of the index
	const uint64_t ntiles = i6_tiles(n);
	const uint64_t tile_bytes = i6_tile_bytes(p.ld6);
	const uint64_t nwaves = uint64_t(gridDim.x) * kScanWaves;
	const uint64_t first = uint64_t(blockIdx.x) * kScanWaves + wave;
	float margin = 0.f, tseed = __builtin_inff();
	EmitEntry* seg = nullptr;
	uint32_t emitted = 0;   // wave-uniform
	if constexpr (kEmit) {
		margin = e.margin[qi];
		seg = e.emit + size_t(qi) * n + emit_segment_offset(e.plan, first);
		if (p.seed_cnt[qi] >= p.sp.kk) tseed = p.seed_dist[size_t(qi) * p.sp.kk + p.sp.kk - 1];
	}

	struct Buf {
		u32x4 x[3 * NC];
		float2 side;
		float aux;
	};
	auto issue = [&](Buf& b, uint64_t set) {
		const uint64_t sc = (set < nsets ? set : nsets - 1) * step;   // past the end: re-read the last set (never reduced)
		uint64_t tile = sc * 4 + uint64_t(g);
		tile = tile < ntiles ? tile : ntiles - 1;   // the last set may hold fewer than four tiles
		const u32x4* src = reinterpret_cast<const u32x4*>(p.codes + tile * tile_bytes) + m;
#pragma unroll
		for (int i = 0; i < 3 * NC; ++i) b.x[i] = __builtin_nontemporal_load(src + 16 * i);
		uint64_t mine = sc * kI6RowsPerWave + uint64_t(g) * kI6RowsPerGroup + (m & 3);
		mine = mine < n ? mine : n - 1;
		b.side = p.side[mine];
		if constexpr (kMetric == kL2) b.aux = p.row_sq[mine];
		if constexpr (kMetric == kCos) b.aux = p.sp.inv_norms[mine];
		if constexpr (kMetric == kIP) b.aux = 0.f;
	};
	auto reduce = [&](const Buf& b, uint64_t set) {
		if (set >= nsets) return;   // wave-uniform
		int v[kI6RowsPerGroup];
#pragma unroll
		for (int j = 0; j < kI6RowsPerGroup; ++j) {
			int hs = 0, ls = 0;
#pragma unroll
			for (int t = 0; t < NC; ++t) {
				const u32x4& nib = b.x[3 * t + (j >> 1)];
				const u32x4& two = b.x[3 * t + 2];
				const uint32_t w0 = (j & 1) ? nib.z : nib.x, w1 = (j & 1) ? nib.w : nib.y;
				const uint32_t z = j == 0 ? two.x : j == 1 ? two.y : j == 2 ? two.z : two.w;
				i6_dot16(w0, w1, z, qh[t], ql[t], hs, ls);
			}
			v[j] = hs * 128 + ls;   // this lane's share of dot(t, u): exact (knn_i6_quant.h)
		}
		// knn_scan_i8's transposing butterfly: afterwards lane m holds the complete sum of row m % 4
		const bool b0 = (m & 1) != 0, b1 = (m & 2) != 0;
		const int a0 = (b0 ? v[1] : v[0]) + __shfl_xor(b0 ? v[0] : v[1], 1);
		const int a1 = (b0 ? v[3] : v[2]) + __shfl_xor(b0 ? v[2] : v[3], 1);
		int s = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 2);
		s += __shfl_xor(s, 4);
		s += __shfl_xor(s, 8);
		const uint64_t row = set * step * kI6RowsPerWave + uint64_t(g) * kI6RowsPerGroup + (m & 3);
		const bool valid = row < n && m < kI6RowsPerGroup;
		float lo, up;
		i8_bounds(kMetric, i8_ip(qinfo.x, b.side.x, i6_sum(s, tsum)), qinfo.y, b.side.y, qq, b.aux, lo, up);
		if constexpr (kKeep) {
			if (valid) lower[row] = lo;
		}
		if constexpr (kEmit) {   // against the wavefront's threshold BEFORE this step's rows are offered
			const float bound = fminf(top.thr_d, tseed) + margin;
			const bool em = valid && margin < __builtin_inff() && lo <= bound;
			const uint64_t emask = __ballot(em);
			if (em) {
				EmitEntry ent;
				ent.lo = lo;
				ent.row = uint32_t(row);
				seg[emitted + uint32_t(__popcll(emask & ((1ull << lane) - 1)))] = ent;
			}
			emitted += uint32_t(__popcll(emask));
		}
		const bool pass = valid && (top.filled < top.kk || up < top.thr_d);
		uint64_t pm = __ballot(pass);
		while (pm) {
			const int src = __builtin_ctzll(pm);
			pm &= pm - 1;
			const float d = __shfl(up, src);
			const uint32_t i = __shfl(uint32_t(row), src);
			if (top.admits(d, i)) top.insert(d, i, lane);
		}
	};
	if (first < nsets) {
		Buf xa, xb;
		issue(xa, first);
		for (uint64_t set = first; set < nsets; set += 2 * nwaves) {
			issue(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xa, set);
			__builtin_amdgcn_sched_barrier(0);
			issue(xa, set + 2 * nwaves);
			__builtin_amdgcn_sched_barrier(0);
			reduce(xb, set + nwaves);
			__builtin_amdgcn_sched_barrier(0);
		}
	}
	if constexpr (kEmit) {   // every wavefront of the grid, the idle ones too: the filter reads all nwaves counts
		if (lane == 0) e.emit_cnt[size_t(qi) * nwaves + first] = emitted;
	}
	block_merge_and_store(top, p.sp, lane, wave);
}

// ---- the shadow: tiles (knn_i6_quant.h) and the side pair {s_r, e_r} per row, from the f32 rows.  knn_i8_build's shape: one 16-lane group per
// row, lane m quantises the 16-element chunks m, m + 16, ... (read twice: the scale first) and stores its three words of each; the residual is an
// fp64 sum over the codes as stored.  Rows first_row ... first_row + n - 1; every pointer at row 0 of the index.  Folds max e^2 into stats6[0], max
// (e inv_norm)^2 into stats6[1] (cosine) and a non-finite e into stats6[2].
__global__ __launch_bounds__(256) void knn_i6_build(const float* rows, const float* inv_norms, uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim,
													 uint8_t* codes, float2* side, uint32_t ld6, unsigned int* stats6) {
	const int lane = threadIdx.x & 63, m = lane & 15;
	const uint64_t ngroups = uint64_t(gridDim.x) * (blockDim.x / kGroup);
	const uint64_t gid = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 4;
	const uint64_t rounds = (n + ngroups - 1) / ngroups;
	const uint32_t nc = ld6 / 256;
	float me = 0.f, mec = 0.f;
	bool bad = false;
	for (uint64_t it = 0; it < rounds; ++it) {   // uniform trip count: every lane takes part in the shuffles
		const uint64_t at = it * ngroups + gid;
		const bool ok = at < n;
		const uint64_t row = first_row + (ok ? at : n - 1);
		const float* r = rows + row * stride;
		float mx = 0.f;
		for (uint32_t t = 0; t < nc; ++t) {
			const uint32_t i0 = (m + 16 * t) * 16;
#pragma unroll
			for (uint32_t e = 0; e < 16; e += 4) {
				if (i0 + e >= dim) continue;
				const float4 v = *reinterpret_cast<const float4*>(r + i0 + e);   // stride is a multiple of 4 floats: in the row's storage
				const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (uint32_t c = 0; c < 4; ++c) {
					if (i0 + e + c < dim) mx = fmaxf(mx, fabsf(x[c]));
				}
			}
		}
		mx = fmaxf(mx, __shfl_xor(mx, 1));
		mx = fmaxf(mx, __shfl_xor(mx, 2));
		mx = fmaxf(mx, __shfl_xor(mx, 4));
		mx = fmaxf(mx, __shfl_xor(mx, 8));
		const float s = i8_scale(mx, kI6CodeMax);
		double r64 = 0.0;
		for (uint32_t t = 0; t < nc; ++t) {
			const uint32_t i0 = (m + 16 * t) * 16;
			uint8_t u[16];
#pragma unroll
			for (uint32_t e = 0; e < 16; ++e) u[e] = 0;   // the pad
#pragma unroll
			for (uint32_t e = 0; e < 16; e += 4) {
				if (i0 + e >= dim) continue;
				const float4 v = *reinterpret_cast<const float4*>(r + i0 + e);
				const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
				for (uint32_t k = 0; k < 4; ++k) {
					if (i0 + e + k >= dim) continue;
					const int c = i8_quantize(x[k], s, kI6CodeMax);
					const double d = i8_residual(x[k], s, c);
					r64 += d * d;
					u[e + k] = uint8_t(c + kI6Bias);
				}
			}
			if (ok) {
				uint32_t w0, w1, z;
				i6_pack16(u, w0, w1, z);
				*reinterpret_cast<uint2*>(codes + i6_nib_offset(row, ld6, t, m)) = make_uint2(w0, w1);
				*reinterpret_cast<uint32_t*>(codes + i6_two_offset(row, ld6, t, m)) = z;
			}
		}
		r64 += __shfl_xor(r64, 1);
		r64 += __shfl_xor(r64, 2);
		r64 += __shfl_xor(r64, 4);
		r64 += __shfl_xor(r64, 8);
		if (ok) {
			const float e = i8_norm_up(r64);
			if (m == 0) side[row] = make_float2(s, e);
			me = fmaxf(me, e * e);
			bad |= !(e * e < __builtin_inff());
			if (inv_norms) {
				const float ei = e * inv_norms[row];
				mec = fmaxf(mec, ei * ei);
				bad |= !(ei * ei < __builtin_inff());
			}
		}
	}
	const bool any_bad = __ballot(bad) != 0;
	for (int o = 32; o; o >>= 1) {
		me = fmaxf(me, __shfl_xor(me, o));
		mec = fmaxf(mec, __shfl_xor(mec, o));
	}
	if (lane == 0) {   // non-negative floats order like their bit patterns
		atomicMax(&stats6[0], __float_as_uint(me));
		atomicMax(&stats6[1], __float_as_uint(mec));
		if (any_bad) atomicMax(&stats6[2], 1u);
	}
}

// A row's bytes inside its tile are its own: row `from` over row `to` (move_row), or zeros over row `to` (from == ~0: the rows a truncate leaves
// behind in the last tile).  One workgroup; thread i handles lane m = i % 16 of chunk i / 16.
__global__ __launch_bounds__(64) void knn_i6_copy_row(uint8_t* codes, uint32_t ld6, uint64_t from, uint64_t to) {
	const uint32_t t = threadIdx.x >> 4, m = threadIdx.x & 15;
	if (t >= ld6 / 256) return;
	uint2 w = make_uint2(0u, 0u);
	uint32_t z = 0;
	if (from != ~0ull) {
		w = *reinterpret_cast<const uint2*>(codes + i6_nib_offset(from, ld6, t, m));
		z = *reinterpret_cast<const uint32_t*>(codes + i6_two_offset(from, ld6, t, m));
	}
	*reinterpret_cast<uint2*>(codes + i6_nib_offset(to, ld6, t, m)) = w;
	*reinterpret_cast<uint32_t*>(codes + i6_two_offset(to, ld6, t, m)) = z;
}

// ------------------------------------------------------------------------------------------ launchers

void launch_i6_build(const float* rows, const float* inv_norms, uint64_t first_row, uint64_t n, uint32_t stride, uint32_t dim, uint8_t* codes, float2* side,
					 uint32_t ld6, unsigned int* stats6, int cus, hipStream_t s) {
	if (!n) return;
	const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n + 15) / 16, uint64_t(cus) * 8));
	hipLaunchKernelGGL(knn_i6_build, dim3(uint32_t(blocks)), dim3(256), 0, s, rows, inv_norms, first_row, n, stride, dim, codes, side, ld6, stats6);
}

void launch_i6_copy_row(uint8_t* codes, uint32_t ld6, uint64_t from, uint64_t to, hipStream_t s) {
	hipLaunchKernelGGL(knn_i6_copy_row, dim3(1), dim3(64), 0, s, codes, ld6, from, to);
}

// The sample of the seed pass: the first set of every scan_i6_seed_step(n) sets, at most kI6SeedSets of them (65 536 rows).
constexpr uint64_t kI6SeedSets = 4096;
uint32_t scan_i6_seed_step(uint64_t n) {
	const uint64_t nsets = (n + kI6RowsPerWave - 1) / kI6RowsPerWave;
	return uint32_t(std::max<uint64_t>(1, (nsets + kI6SeedSets - 1) / kI6SeedSets));
}
// The grid of a pass with that step (1: the full pass).  The load depth is the int8 scan's: RXGPU_SCAN_I8_WG_PER_CU sizes both.
uint32_t scan_i6_grid_x(uint64_t n, uint32_t set_step, int cus) {
	const uint64_t nsets_all = (n + kI6RowsPerWave - 1) / kI6RowsPerWave;
	const uint64_t nsets = (nsets_all + set_step - 1) / set_step;
	return scan_i8_grid_x(nsets * kI6RowsPerWave, cus);
}

template <int kMetric, bool kEmit, bool kKeep>
static void launch_scan_i6_metric(const ScanI6Params& p, const ScanI8Emit& e, dim3 grid, hipStream_t s) {
	switch (p.ld6 / 256) {
		case 1: hipLaunchKernelGGL((knn_scan_i6<kMetric, 1, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		case 2: hipLaunchKernelGGL((knn_scan_i6<kMetric, 2, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		case 3: hipLaunchKernelGGL((knn_scan_i6<kMetric, 3, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
		default: hipLaunchKernelGGL((knn_scan_i6<kMetric, 4, kEmit, kKeep>), grid, dim3(kScanThreads), 0, s, p, e); break;
	}
}
template <bool kEmit, bool kKeep>
static void launch_scan_i6_form(int metric, const ScanI6Params& p, const ScanI8Emit& e, dim3 grid, hipStream_t s) {
	switch (metric) {
		case kL2: launch_scan_i6_metric<kL2, kEmit, kKeep>(p, e, grid, s); break;
		case kIP: launch_scan_i6_metric<kIP, kEmit, kKeep>(p, e, grid, s); break;
		default: launch_scan_i6_metric<kCos, kEmit, kKeep>(p, e, grid, s); break;
	}
}
// p.ld6 must be i6_ld(dim) of a dimension with i6_dim_supported(dim); gridx = scan_i6_grid_x(p.sp.n, p.set_step, cus).  emit null: the seed pass
// (nothing emitted, nothing kept); else p.set_step must be 1 and e->plan emit_plan(p.sp.n, gridx), and keep says whether p.lower is written.
void launch_scan_i6(int metric, const ScanI6Params& p, uint32_t nq, uint32_t gridx, hipStream_t s, const ScanI8Emit* emit, bool keep) {
	const dim3 grid(gridx, nq);
	if (!emit) {
		launch_scan_i6_form<false, false>(metric, p, ScanI8Emit{}, grid, s);
	} else if (keep) {
		launch_scan_i6_form<true, true>(metric, p, *emit, grid, s);
	} else {
		launch_scan_i6_form<true, false>(metric, p, *emit, grid, s);
	}
}

}  // namespace rxgpu
