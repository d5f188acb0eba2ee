// Arithmetic of the int8 shadow tier of the single-query scan (knn_scan_i8.hip, knn_query_prep_i8 in knn_batched.hip), standard library
// only: the kernels and the host compile the same functions (tests/cpp/knn_i8_quant_cpu.cc pins them on the CPU).
//
// Row r is stored as codes c_i = clamp(rint(x_i / s_r), -127, 127) with s_r = max|x_i| / 127 and a side pair {s_r, e_r}, where e_r is the
// A-POSTERIORI residual norm: e_r >= |x_r - s_r c_r|_2, computed in fp64 from the codes that were stored and rounded up.  The query is
// quantised to 15 bits, t_i = rint(q_i / s_q), s_q = max|q_i| / 16256, carried as two byte planes t = 128 h + l (h in [-127, 127],
// l in [-64, 63]), with r_q >= |q - s_q t|_2 computed the same way.  The scan forms S_r = 128 dot(h, c_r) + dot(l, c_r) = dot(t, c_r) in
// int32: an EXACT integer whatever the order of the additions (|S| <= D * 127 * 16256 < 2^31 for D <= 1040), and
//     ip~ = fl(fl(s_q s_r) fl(S_r)).
//
// Bound (inner product).  With P = s_q s_r S_r as a real number:
//     q.x - P = q.(x - s_r c) + (q - s_q t).(s_r c)        =>   |q.x - P| <= |q| e_r + r_q |s_r c| <= |q| e_r + r_q (|x| + e_r)
//     |ip~ - P| <= ((1 + u)^3 - 1) |P| + 2^-118            (int -> float, two products; 2^-118 covers a product that underflows)
//     |P| <= |s_q t| |s_r c| <= (|q| + r_q)(|x| + e_r)
// so |q.x - ip~| <= E_r + G with
//     E_r = |q|^ e_r (1 + 4u) + 2^-118                      per row     (i8_bounds;  |q|^ = |q| rounded up)
//     G   = [r_q + 6u (|q|^ + r_q)] (max|x| + max e)        per query   (i8_margin_global; the maxima are sqrt of the statistics words, + 1 %
//                                                                        for the f32 arithmetic that produced them)
// L2:      d~ = (|q|^2 + |x_r|^2) - 2 ip~ : per row 2 E_r, per query 2 G; the f32 terms of f32_query_margin<L2> cover the decomposed form, its
//          f32 |q|^2 and |x|^2 and the reference's own summation, as they do for the f32 nomination GEMM.
// cosine:  d~ = -ip~ inv_r : per row E_r inv_r, per query G with the maxima of (|x| inv) and (e inv); the extra product is inside the 6u.
// The kernel stores lo_r = d~ - B_r and folds up_r = d~ + B_r (B_r the per-row term, both rounded outward by 4u of their operands) into its
// top-kk.  With T = the kk-th smallest up_r, delta = the f32 error of the exact kernels' own distances (half of f32_query_margin) and D_kk
// the kk-th best exact distance: kk rows have d <= up + G + delta <= T + G + delta, so D_kk <= T + G + delta, and every row of the true
// top-kk has lo_r <= d_r + G + delta <= T + 2 G + 2 delta.  knn_filter_approx therefore runs over the lo_r with margin = 2 delta + 2 G.
//
// Range search (knn_range_i8 in knn_scan_i8.hip, i8_range_bound below).  A row is a hit when the exact kernels' f32 distance d_r satisfies
// d_r < radius (or <=), so a hit has, as real numbers, lo_r <= d_r + G + delta <= radius + G + delta = radius + margin / 2: half of the
// margin the query prep writes is spare.  The kernel compares against t = fl(radius + margin), moved one float outward.  The f32 rounding of that
// sum cannot eat the spare half, however large |radius| is against the margin: lo_r is itself an f32 and rounding to nearest is monotone, so
// lo_r <= radius + margin / 2 <= radius + margin (margin >= 0) gives lo_r = fl(lo_r) <= fl(radius + margin) <= t.  (Where ulp(radius)
// exceeds the margin the sum rounds back to radius, and a float lo_r <= radius + margin / 2 < the float above radius is <= radius as well.)
// The outward step is not needed for this; it covers a sum evaluated in another rounding mode.  A NaN radius gives t = NaN, which no row
// passes, and the f32 kernel finds no hit either; a margin that is not finite means there is no bound: t = +inf, every row passes (the
// query prep has set cand_cnt = cap + 1 for such a query and the kernel emits nothing: the f32 kernel answers the call).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RX_I8_HD __host__ __device__
#else
#define RX_I8_HD
#endif

namespace rxgpu {

enum : int { kI8L2 = 0, kI8IP = 1, kI8Cos = 2 };   // the metric numbers of knn_kernels.hip.h

constexpr int kI8CodeMax = 127;
constexpr int kI8QueryMax = 16256;                     // 127 * 128: h stays within [-127, 127]
constexpr float kI8Floor = 3.1e-36f;                   // > 2^-118
constexpr float kI8U4 = 2.384185791015625e-07f;        // 2^-22 = 4u
constexpr float kI8U = 5.9604645e-08f;                 // 2^-24
constexpr float kI8MinScale = 1.17549435e-38f;         // smallest normal f32: a smaller scale is degenerate

// bytes of a code row: the dimension rounded up to 256 (16 lanes x 16 bytes).  The tier serves ld8 <= 1024 (int32 range of S) where a code row
// is shorter than the row of the bf16 shadow (2 bytes x the dimension rounded up to 64): up to 128 dims both are 256 bytes and the bf16 tier stays.
RX_I8_HD inline uint32_t i8_ld(uint32_t dim) { return (dim + 255u) & ~255u; }
RX_I8_HD inline bool i8_dim_supported(uint32_t dim) { return dim <= 1024 && i8_ld(dim) < 2u * ((dim + 63u) & ~63u); }

// a float >= v for v >= 0 (NaN stays NaN)
RX_I8_HD inline float i8_up(double v) {
	float f = float(v);
	if (double(f) < v) {
		uint32_t b;
		__builtin_memcpy(&b, &f, sizeof(b));
		++b;   // f >= 0 and finite here: the next float up (the largest finite one becomes +inf)
		__builtin_memcpy(&f, &b, sizeof(b));
	}
	return f;
}
// sqrt of an fp64 sum of squares, rounded up (2^-30 covers the fp64 summation of <= 2^20 terms and the root)
RX_I8_HD inline float i8_norm_up(double sumsq) { return i8_up(std::sqrt(sumsq) * (1.0 + 9.3132257461547852e-10)); }

// scale of a row (qmax = 127) or of a query (qmax = 16256); 0 = degenerate (zero, subnormal or not finite): codes are zero then and the
// row / query is carried by its residual alone
RX_I8_HD inline float i8_scale(float maxabs, int qmax) {
	const float s = maxabs / float(qmax);
	return (s >= kI8MinScale && s < HUGE_VALF) ? s : 0.0f;
}
RX_I8_HD inline int i8_quantize(float x, float s, int qmax) {
	if (!(s > 0.0f)) return 0;
	const float r = ::rintf(x / s);
	if (!(r == r)) return 0;   // a NaN element: its residual is NaN, which marks the index as not finite
	return r > float(qmax) ? qmax : r < -float(qmax) ? -qmax : int(r);
}
// x - s c as the residual sums take it (s c is exact in fp64)
RX_I8_HD inline double i8_residual(float x, float s, int c) { return double(x) - double(s) * double(c); }

// t = 128 h + l, h in [-127, 127], l in [-64, 63], for |t| <= 16256
RX_I8_HD inline void i8_split(int t, int& h, int& l) {
	h = (t + 64 + 128 * 128) / 128 - 128;   // floor((t + 64) / 128) on non-negative operands
	l = t - 128 * h;
}

// The per-query margin 2 eps_q of an f32 (kBf16 = false) or bf16 nomination from s = |q|^2 and the statistics words as floats:
// xmax2 = max |x|^2, xcmax2 = max (|x| inv_norm)^2 (cosine).
template <int kMetric, bool kBf16>
RX_I8_HD inline float f32_query_margin(float s, uint32_t dim, float xmax2, float xcmax2) {
	const float u = kI8U;
	// f32 accumulation: covers both summation trees (D-chain vs 64-chain + fold), 10% slack.  The bf16 MFMA adds 16 products per instruction in an
	// adder tree whose internal rounding mode is not documented: allow 2 ulp-halves per addition and the tree depth on top of the chain (4x)
	const float gamma = (kBf16 ? 4.4f : 1.1f) * float(dim + 64) * u;
	// rne_bf16 on q and x: |q~.x~ - q.x| <= ((1+2^-9)^2 - 1) sum|q_i x_i| <= 2^-8 (1 + 2^-10) |q||x|   (only the inner product is affected:
	// |q|^2 and |x|^2 of the L2 form come from the f32 data)
	const float gb = kBf16 ? 1.01f * 0.00390625f : 0.0f;
	float eps;
	if (kMetric == kI8L2) {
		// d = (qq + xx) - 2 ip: 2*gamma*|q||x| <= gamma*(qq+xx), plus the roundings of qq, xx and of the reference's own sum; bf16 adds 2*gb*|q||x|
		eps = 2.0f * gamma * (s + xmax2) + 2.0f * gb * ::sqrtf(s) * ::sqrtf(xmax2);
	} else if (kMetric == kI8IP) {
		eps = (gamma + gb) * ::sqrtf(s) * ::sqrtf(xmax2);
	} else {
		eps = (gamma + gb + 4.0f * u) * ::sqrtf(s) * ::sqrtf(xcmax2);
	}
	// bf16 MFMA may flush subnormal inputs: at most dim * 2^-126 * (|q| + max|x|), far below the 1e-30 floor added here
	return 2.0f * eps * 1.01f + (kBf16 ? 1e-30f : 1e-37f);
}

// G of the file header: the part of the int8 bound that does not depend on the row.  xmax2 / emax2 are the statistics words as floats
// (max |x|^2 and max e^2, or their cosine forms max (|x| inv)^2 and max (e inv)^2).
RX_I8_HD inline float i8_margin_global(int metric, float qn_up, float rq_up, float xmax2, float emax2) {
	const float m = 1.01f * (::sqrtf(xmax2) + ::sqrtf(emax2));
	const float coef = rq_up + 6.0f * kI8U * (qn_up + rq_up);
	const float g = coef * m * 1.01f;
	return metric == kI8L2 ? 2.0f * g : g;
}
// what knn_filter_approx adds to the kk-th smallest upper bound: 2 delta + 2 G, rounded up
template <int kMetric>
RX_I8_HD inline float i8_margin(float s, uint32_t dim, float qn_up, float rq_up, float xmax2, float xcmax2, float emax2, float ecmax2) {
	const float g = kMetric == kI8Cos ? i8_margin_global(kMetric, qn_up, rq_up, xcmax2, ecmax2) : i8_margin_global(kMetric, qn_up, rq_up, xmax2, emax2);
	return (f32_query_margin<kMetric, false>(s, dim, xmax2, xcmax2) + 2.0f * g) * 1.0001f;
}

// The threshold of a range scan: every row whose exact-kernel distance is <= radius has lo_r <= i8_range_bound(radius, margin), with margin
// = i8_margin of the query (the argument is in the file header).  NaN radius: NaN (no row passes); no finite margin: +inf (no bound).
RX_I8_HD inline float i8_range_bound(float radius, float margin) {
	if (!(radius == radius)) return radius;
	if (!(margin < HUGE_VALF)) return HUGE_VALF;
	float t = radius + margin;
	if (!(::fabsf(t) < HUGE_VALF)) return t;   // +-inf stays
	uint32_t b;
	__builtin_memcpy(&b, &t, sizeof(b));
	if (t > 0.0f) {
		++b;   // the next float up (the largest finite one becomes +inf)
	} else if (t < 0.0f) {
		--b;   // towards zero
	} else {
		b = 1u;   // +-0: the smallest positive subnormal
	}
	__builtin_memcpy(&t, &b, sizeof(b));
	return t;
}

RX_I8_HD inline float i8_ip(float s_q, float s_r, int32_t S) { return (s_q * s_r) * float(S); }

// d~ and its per-row window [lo, up] (rounded outward).  aux = |x_r|^2 (L2) or inv_norm_r (cosine); qq = |q|^2 in f32 (L2).
RX_I8_HD inline float i8_bounds(int metric, float ipf, float qn_up, float e_r, float qq, float aux, float& lo, float& up) {
	float E = qn_up * e_r;
	E = E + E * kI8U4 + kI8Floor;
	float d, B;
	if (metric == kI8L2) {
		d = (qq + aux) - 2.0f * ipf;
		B = 2.0f * E;
	} else if (metric == kI8IP) {
		d = -ipf;
		B = E;
	} else {
		d = -ipf * aux;
		B = E * ::fabsf(aux);
		B = B + B * kI8U4;
	}
	const float w = kI8U4 * (::fabsf(d) + B);
	lo = (d - B) - w;
	up = (d + B) + w;
	return d;
}

}  // namespace rxgpu
