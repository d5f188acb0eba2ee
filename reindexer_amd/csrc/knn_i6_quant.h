// Arithmetic and layout of the 6-bit shadow front of the int8-pruned single-query scan (knn_scan_i6.hip), standard library only: the kernels
// and the host compile the same functions (tests/cpp/knn_i6_quant_cpu.cc pins them on the CPU).
//
// Row r is stored as codes c_i = clamp(rint(x_i / s_r), -31, 31) with s_r = max|x_i| / 31, kept as u_i = c_i + 32 in 6 bits, and the side
// pair {s_r, e_r} with e_r the a-posteriori residual norm exactly as the int8 shadow forms it: i8_scale / i8_quantize with qmax = 31,
// i8_residual and i8_norm_up of knn_i8_quant.h.  The query side is the int8 tier's, unchanged (knn_query_prep_i8: the planes t = 128 h + l,
// {s_q, |q|^}, r_q).  The scan forms
//     S_r = dot(t, u_r) - 32 sum(t)          over the real dimensions (the planes are zero in the pad, so the pad codes do not matter)
// Both terms are exact int32: |dot(t, u)| <= 1024 * 63 * 16256 < 2^31 and 32 |sum(t)| <= 32 * 1024 * 16256 < 2^31, and S_r = dot(t, c_r).
// From there on everything is knn_i8_quant.h's: i8_ip, i8_bounds, and i8_margin with the maxima of the 6-bit residuals (statistics words of
// their own: the int8 words keep their meaning).  THE SOUNDNESS ARGUMENT IS THAT HEADER'S, WORD FOR WORD: nothing in it depends on the number
// of code levels, only on e_r >= |x_r - s_r c_r| and on S_r being the exact integer dot(t, c_r).
//
// Layout: 0.75 bytes per element at ld6 = the dimension rounded up to 256.  Four consecutive rows share a TILE of 3 ld6 bytes.  A tile is cut
// into ld6 / 256 chunks of three 256-byte lines; line L of chunk t holds 16 bytes for each of the 16 lanes m of a group, and lane m owns the
// 16 codes of the dimensions (m + 16 t) 16 ... + 15 of each of the four rows:
//     line 0: row 0 {w0, w1}, row 1 {w0, w1}       line 1: rows 2 and 3 the same       line 2: z of rows 0, 1, 2, 3
// w0, w1 (nibble planes, u >> 2) and z (the 2-bit plane, u & 3) are 32-bit words; byte b of w0 holds codes b (low nibble) and 4 + b (high), of
// w1 codes 8 + b and 12 + b, and byte b of z holds codes b, 4 + b, 8 + b, 12 + b in its bit pairs.  So the bytes of codes 4 k ... 4 k + 3, in order,
// are ((w >> 4 (k & 1)) & 0x0F0F0F0F) << 2 | (z >> 2 k) & 0x03030303: the query planes need no permutation.  Every byte of a tile belongs to
// one row; pad codes and the rows past the end of the index in the last tile are zero bytes.
#pragma once

#include "knn_i8_quant.h"

namespace rxgpu {

constexpr int kI6CodeMax = 31;
constexpr int kI6Bias = 32;
constexpr uint32_t kI6TileRows = 4;

RX_I8_HD inline uint32_t i6_ld(uint32_t dim) { return i8_ld(dim); }
RX_I8_HD inline bool i6_dim_supported(uint32_t dim) { return i8_dim_supported(dim); }
RX_I8_HD inline uint64_t i6_tile_bytes(uint32_t ld6) { return uint64_t(ld6) * 3u; }
RX_I8_HD inline uint64_t i6_tiles(uint64_t rows) { return (rows + kI6TileRows - 1) / kI6TileRows; }
RX_I8_HD inline uint64_t i6_shadow_bytes(uint64_t rows, uint32_t ld6) { return i6_tiles(rows) * i6_tile_bytes(ld6); }
// where lane m's words of row `row` and chunk t start: the 8 bytes {w0, w1} and the 4 bytes z
RX_I8_HD inline uint64_t i6_nib_offset(uint64_t row, uint32_t ld6, uint32_t t, uint32_t m) {
	const uint32_t j = uint32_t(row % kI6TileRows);
	return (row / kI6TileRows) * i6_tile_bytes(ld6) + (uint64_t(t * 3u + (j >> 1)) * 16u + m) * 16u + (j & 1u) * 8u;
}
RX_I8_HD inline uint64_t i6_two_offset(uint64_t row, uint32_t ld6, uint32_t t, uint32_t m) {
	const uint32_t j = uint32_t(row % kI6TileRows);
	return (row / kI6TileRows) * i6_tile_bytes(ld6) + (uint64_t(t * 3u + 2u) * 16u + m) * 16u + j * 4u;
}

// 16 biased codes (0 .. 63) -> the three words of a lane, and back to four words of four bytes each
RX_I8_HD inline void i6_pack16(const uint8_t* u, uint32_t& w0, uint32_t& w1, uint32_t& z) {
	w0 = w1 = z = 0;
	for (uint32_t b = 0; b < 4; ++b) {
		w0 |= (uint32_t(u[b] >> 2) | uint32_t(u[4 + b] >> 2) << 4) << (8 * b);
		w1 |= (uint32_t(u[8 + b] >> 2) | uint32_t(u[12 + b] >> 2) << 4) << (8 * b);
		z |= (uint32_t(u[b] & 3) | uint32_t(u[4 + b] & 3) << 2 | uint32_t(u[8 + b] & 3) << 4 | uint32_t(u[12 + b] & 3) << 6) << (8 * b);
	}
}
RX_I8_HD inline void i6_unpack16(uint32_t w0, uint32_t w1, uint32_t z, uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
	c0 = ((w0 << 2) & 0x3C3C3C3Cu) | (z & 0x03030303u);
	c1 = ((w0 >> 2) & 0x3C3C3C3Cu) | ((z >> 2) & 0x03030303u);
	c2 = ((w1 << 2) & 0x3C3C3C3Cu) | ((z >> 4) & 0x03030303u);
	c3 = ((w1 >> 2) & 0x3C3C3C3Cu) | ((z >> 6) & 0x03030303u);
}

// the biased code of element x of a row with scale s (a pad element is stored as 0, not through this)
RX_I8_HD inline uint8_t i6_code(float x, float s) { return uint8_t(i8_quantize(x, s, kI6CodeMax) + kI6Bias); }

// S_r from dot(t, u_r) and sum(t)
RX_I8_HD inline int32_t i6_sum(int32_t dot_tu, int32_t sum_t) { return dot_tu - kI6Bias * sum_t; }

// Host side: one row of a tiled shadow <-> ld6 row-major bytes of u (the builder's packing and rxgpu_index_inspect's "codes_i6").
inline void i6_store_row(uint8_t* shadow, uint64_t row, uint32_t ld6, const uint8_t* u) {
	for (uint32_t t = 0; t < ld6 / 256u; ++t) {
		for (uint32_t m = 0; m < 16u; ++m) {
			uint32_t w[3];
			i6_pack16(u + (m + 16u * t) * 16u, w[0], w[1], w[2]);
			std::memcpy(shadow + i6_nib_offset(row, ld6, t, m), w, 8);
			std::memcpy(shadow + i6_two_offset(row, ld6, t, m), w + 2, 4);
		}
	}
}
inline void i6_load_row(const uint8_t* shadow, uint64_t row, uint32_t ld6, uint8_t* u) {
	for (uint32_t t = 0; t < ld6 / 256u; ++t) {
		for (uint32_t m = 0; m < 16u; ++m) {
			uint32_t w[3], c[4];
			std::memcpy(w, shadow + i6_nib_offset(row, ld6, t, m), 8);
			std::memcpy(w + 2, shadow + i6_two_offset(row, ld6, t, m), 4);
			i6_unpack16(w[0], w[1], w[2], c[0], c[1], c[2], c[3]);
			std::memcpy(u + (m + 16u * t) * 16u, c, 16);   // (little endian: byte b of c[k] is code 4 k + b)
		}
	}
}

}  // namespace rxgpu
