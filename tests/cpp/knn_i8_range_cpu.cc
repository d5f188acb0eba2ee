// The range bound of the int8 shadow tier (i8_range_bound in reindexer_amd/csrc/knn_i8_quant.h) compiled for the host:
// tests/test_knn_i8_range.py holds it against the lower bounds and the f32 distances of the adversarial corpus, through the function the
// kernels call.  Test infrastructure only — nothing in the product links this.
#include <cstdint>

#include "knn_i8_quant.h"

extern "C" {

float i8_range_cpu_bound(float radius, float margin) { return rxgpu::i8_range_bound(radius, margin); }

// the same for n (radius, margin) pairs
void i8_range_cpu_bound_many(uint64_t n, const float* radius, const float* margin, float* out) {
	for (uint64_t i = 0; i < n; ++i) out[i] = rxgpu::i8_range_bound(radius[i], margin[i]);
}
}
