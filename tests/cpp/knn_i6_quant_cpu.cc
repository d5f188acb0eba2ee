// The arithmetic and the layout of the 6-bit shadow (reindexer_amd/csrc/knn_i6_quant.h) compiled for the host: tests/test_knn_i6_quant.py
// pins pack and unpack, the integer sum and the bound on the CPU, through the functions the kernels call.  Everything from the integer sum
// on is knn_i8_quant.h's and is reached through tests/cpp/knn_i8_quant_cpu.cc.  Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "knn_i6_quant.h"

extern "C" {

uint32_t i6_cpu_ld(uint32_t dim) { return rxgpu::i6_ld(dim); }
uint64_t i6_cpu_shadow_bytes(uint64_t rows, uint32_t ld6) { return rxgpu::i6_shadow_bytes(rows, ld6); }

// one row as knn_i6_build forms it: u[ld6] (zero pad), *scale, *resid (e_r)
void i6_cpu_quantize_row(const float* x, uint32_t dim, uint8_t* u, float* scale, float* resid) {
	float mx = 0.f;
	for (uint32_t i = 0; i < dim; ++i) mx = std::fmax(mx, std::fabs(x[i]));
	const float s = rxgpu::i8_scale(mx, rxgpu::kI6CodeMax);
	double r64 = 0.0;
	const uint32_t ld6 = rxgpu::i6_ld(dim);
	for (uint32_t i = 0; i < ld6; ++i) {
		u[i] = 0;
		if (i < dim) {
			u[i] = rxgpu::i6_code(x[i], s);
			const double d = rxgpu::i8_residual(x[i], s, int(u[i]) - rxgpu::kI6Bias);
			r64 += d * d;
		}
	}
	*scale = s;
	*resid = rxgpu::i8_norm_up(r64);
}
void i6_cpu_quantize_rows(const float* x, uint64_t n, uint32_t dim, uint8_t* u, float* scale, float* resid) {
	const uint32_t ld6 = rxgpu::i6_ld(dim);
	for (uint64_t r = 0; r < n; ++r) i6_cpu_quantize_row(x + r * dim, dim, u + r * ld6, scale + r, resid + r);
}

// n rows of row-major bytes u[n][ld6] into a tiled shadow (i6_cpu_shadow_bytes(n, ld6) bytes, zeroed first), and back
void i6_cpu_pack(const uint8_t* u, uint64_t n, uint32_t ld6, uint8_t* shadow) {
	std::memset(shadow, 0, rxgpu::i6_shadow_bytes(n, ld6));
	for (uint64_t r = 0; r < n; ++r) rxgpu::i6_store_row(shadow, r, ld6, u + r * ld6);
}
void i6_cpu_unpack(const uint8_t* shadow, uint64_t n, uint32_t ld6, uint8_t* u) {
	for (uint64_t r = 0; r < n; ++r) rxgpu::i6_load_row(shadow, r, ld6, u + r * ld6);
}

// S of row `row` of a tiled shadow as knn_scan_i6 forms it, in int32: per lane and chunk the unpacked words against the planes (byte by byte,
// what the 4-way dot instruction does), hs * 128 + ls per lane, the lanes summed, 32 sum(t) taken off.  *overflow: an int64 evaluation of
// any of the int32 quantities disagrees.
int32_t i6_cpu_sum(const int8_t* h, const int8_t* l, const uint8_t* shadow, uint64_t row, uint32_t ld6, int* overflow) {
	int64_t wide = 0, wide_t = 0;
	int32_t dot = 0, tsum = 0;
	for (uint32_t m = 0; m < 16; ++m) {
		int32_t hs = 0, ls = 0, ht = 0, lt = 0;
		for (uint32_t t = 0; t < ld6 / 256u; ++t) {
			uint32_t w[3], c[4];
			std::memcpy(w, shadow + rxgpu::i6_nib_offset(row, ld6, t, m), 8);
			std::memcpy(w + 2, shadow + rxgpu::i6_two_offset(row, ld6, t, m), 4);
			rxgpu::i6_unpack16(w[0], w[1], w[2], c[0], c[1], c[2], c[3]);
			for (uint32_t k = 0; k < 16; ++k) {
				const uint32_t i = (m + 16u * t) * 16u + k;
				const int32_t code = int32_t((c[k / 4] >> (8 * (k % 4))) & 0xFFu);
				hs += int32_t(h[i]) * code;
				ls += int32_t(l[i]) * code;
				ht += int32_t(h[i]);
				lt += int32_t(l[i]);
				wide += (int64_t(h[i]) * 128 + int64_t(l[i])) * int64_t(code);
				wide_t += int64_t(h[i]) * 128 + int64_t(l[i]);
			}
		}
		dot += hs * 128 + ls;
		tsum += ht * 128 + lt;
	}
	const int32_t s = rxgpu::i6_sum(dot, tsum);
	const int64_t want = wide - 32 * wide_t;
	*overflow = (int64_t(dot) != wide || int64_t(tsum) != wide_t || int64_t(s) != want) ? 1 : 0;
	return s;
}
}
