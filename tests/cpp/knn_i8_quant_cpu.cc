// The arithmetic of the int8 shadow tier (reindexer_amd/csrc/knn_i8_quant.h) compiled for the host: tests/test_knn_i8_quant.py pins the
// quantisation, the residuals and the bound on the CPU, through the functions the kernels call, in the order the kernels call them.
// Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "knn_i8_quant.h"

extern "C" {

// one row as knn_i8_build stores it: codes[ld8] (zero pad), *scale, *resid (e_r)
void i8_cpu_quantize_row(const float* x, uint32_t dim, int8_t* codes, float* scale, float* resid) {
	float mx = 0.f;
	for (uint32_t i = 0; i < dim; ++i) mx = std::fmax(mx, std::fabs(x[i]));
	const float s = rxgpu::i8_scale(mx, rxgpu::kI8CodeMax);
	double r64 = 0.0;
	const uint32_t ld8 = rxgpu::i8_ld(dim);
	for (uint32_t i = 0; i < ld8; ++i) {
		int c = 0;
		if (i < dim) {
			c = rxgpu::i8_quantize(x[i], s, rxgpu::kI8CodeMax);
			const double d = rxgpu::i8_residual(x[i], s, c);
			r64 += d * d;
		}
		codes[i] = int8_t(c);
	}
	*scale = s;
	*resid = rxgpu::i8_norm_up(r64);
}

// the same for n rows: x[n][dim], codes[n][ld8], scale[n], resid[n]
void i8_cpu_quantize_rows(const float* x, uint64_t n, uint32_t dim, int8_t* codes, float* scale, float* resid) {
	const uint32_t ld8 = rxgpu::i8_ld(dim);
	for (uint64_t r = 0; r < n; ++r) i8_cpu_quantize_row(x + r * dim, dim, codes + r * ld8, scale + r, resid + r);
}

// one query as knn_query_prep_i8 leaves it: planes h[ld8], l[ld8], t[ld8]; info = {s_q, |q| rounded up, r_q, |q|^2 (f32 fmaf chain)}
void i8_cpu_quantize_query(const float* q, uint32_t dim, int8_t* h, int8_t* l, int32_t* t, float* info) {
	float mx = 0.f, s = 0.f;
	double s64 = 0.0;
	for (uint32_t i = 0; i < dim; ++i) {
		mx = std::fmax(mx, std::fabs(q[i]));
		s = std::fma(q[i], q[i], s);
		s64 += double(q[i]) * double(q[i]);
	}
	const float sq = rxgpu::i8_scale(mx, rxgpu::kI8QueryMax);
	double r64 = 0.0;
	const uint32_t ld8 = rxgpu::i8_ld(dim);
	for (uint32_t i = 0; i < ld8; ++i) {
		const float v = i < dim ? q[i] : 0.f;
		const int ti = rxgpu::i8_quantize(v, sq, rxgpu::kI8QueryMax);
		int hh, ll;
		rxgpu::i8_split(ti, hh, ll);
		h[i] = int8_t(hh);
		l[i] = int8_t(ll);
		t[i] = ti;
		const double d = rxgpu::i8_residual(v, sq, ti);
		r64 += d * d;
	}
	info[0] = sq;
	info[1] = rxgpu::i8_norm_up(s64);
	info[2] = rxgpu::i8_norm_up(r64);
	info[3] = s;
}

// S = 128 dot(h, c) + dot(l, c) in int32 as the scan forms it; returns 0 and sets *overflow when an int64 evaluation disagrees
int32_t i8_cpu_dot(const int8_t* h, const int8_t* l, const int8_t* c, uint32_t ld8, int* overflow) {
	int32_t hs = 0, ls = 0;
	int64_t wide = 0;
	for (uint32_t i = 0; i < ld8; ++i) {
		hs += int32_t(h[i]) * int32_t(c[i]);
		ls += int32_t(l[i]) * int32_t(c[i]);
		wide += (int64_t(h[i]) * 128 + int64_t(l[i])) * int64_t(c[i]);
	}
	const int64_t s = int64_t(hs) * 128 + int64_t(ls);
	*overflow = (s != wide || s > INT32_MAX || s < INT32_MIN) ? 1 : 0;
	return int32_t(s);
}

// d~, lo, up of one (query, row) pair: out = {d~, lo, up}
void i8_cpu_bounds(int metric, float s_q, float s_r, int32_t S, float qn_up, float e_r, float qq, float aux, float* out) {
	float lo, up;
	out[0] = rxgpu::i8_bounds(metric, rxgpu::i8_ip(s_q, s_r, S), qn_up, e_r, qq, aux, lo, up);
	out[1] = lo;
	out[2] = up;
}

// the same for n pairs: out[n][3]
void i8_cpu_bounds_many(int metric, uint64_t n, const float* s_q, const float* s_r, const int32_t* S, const float* qn_up, const float* e_r, const float* qq,
						const float* aux, float* out) {
	for (uint64_t i = 0; i < n; ++i) i8_cpu_bounds(metric, s_q[i], s_r[i], S[i], qn_up[i], e_r[i], qq[i], aux[i], out + 3 * i);
}

// {G (i8_margin_global), the whole margin of knn_filter_approx}; xmax2 .. ecmax2 are the statistics words as floats
void i8_cpu_margin(int metric, float s, uint32_t dim, float qn_up, float rq_up, float xmax2, float xcmax2, float emax2, float ecmax2, float* out) {
	const bool cosine = metric == rxgpu::kI8Cos;
	out[0] = rxgpu::i8_margin_global(metric, qn_up, rq_up, cosine ? xcmax2 : xmax2, cosine ? ecmax2 : emax2);
	out[1] = metric == rxgpu::kI8L2   ? rxgpu::i8_margin<rxgpu::kI8L2>(s, dim, qn_up, rq_up, xmax2, xcmax2, emax2, ecmax2)
			 : metric == rxgpu::kI8IP ? rxgpu::i8_margin<rxgpu::kI8IP>(s, dim, qn_up, rq_up, xmax2, xcmax2, emax2, ecmax2)
									  : rxgpu::i8_margin<rxgpu::kI8Cos>(s, dim, qn_up, rq_up, xmax2, xcmax2, emax2, ecmax2);
}

// the per-query margin of an f32 (bf16 = 0) or bf16 nomination, as knn_query_stats / knn_query_prep form it
float i8_cpu_f32_margin(int metric, int bf16, float s, uint32_t dim, float xmax2, float xcmax2) {
	using namespace rxgpu;
	if (bf16) {
		return metric == kI8L2 ? f32_query_margin<kI8L2, true>(s, dim, xmax2, xcmax2)
			   : metric == kI8IP ? f32_query_margin<kI8IP, true>(s, dim, xmax2, xcmax2)
								 : f32_query_margin<kI8Cos, true>(s, dim, xmax2, xcmax2);
	}
	return metric == kI8L2 ? f32_query_margin<kI8L2, false>(s, dim, xmax2, xcmax2)
		   : metric == kI8IP ? f32_query_margin<kI8IP, false>(s, dim, xmax2, xcmax2)
							 : f32_query_margin<kI8Cos, false>(s, dim, xmax2, xcmax2);
}

int i8_cpu_dim_supported(uint32_t dim) { return rxgpu::i8_dim_supported(dim) ? 1 : 0; }
uint32_t i8_cpu_ld(uint32_t dim) { return rxgpu::i8_ld(dim); }
}
