// The rule of a collected streaming session (reindexer_amd/csrc/hnsw_stream_collect_plan.h) checked on the host, stand-alone:
// tests/test_hnsw_stream_collect_plan.py builds and runs it, once plain and once under -fsanitize=address,undefined.
//   hnsw_stream_collect_plan_cpu check          the estimate against a restatement in integers and (built with -DRX_WITH_REFERENCE and the
//                                               reference tree on the include path) against StreamingKnnEstimator::EstimateBatchSize itself,
//                                               over a grid of accepted <= 2000, presented <= 800 000, needed <= 2000; the stop test and
//                                               the bounds by brute force.  Exit status 0: every check held.
//   hnsw_stream_collect_plan_cpu table FILE     the recorded table's points (a text file of "accepted presented needed" lines) -> one batch
//                                               per line on stdout
// Test infrastructure only — nothing in the product links this.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hnsw_stream_collect_plan.h"
#if defined(RX_WITH_REFERENCE)
#include "core/nsselecter/knn_streaming_estimator.h"
#endif

namespace {

int failures = 0;
#define CHECK(cond, ...)                         \
	do {                                         \
		if (!(cond)) {                           \
			if (failures++ < 20) {               \
				std::printf("FAILED %s: ", #cond); \
				std::printf(__VA_ARGS__);        \
				std::printf("\n");               \
			}                                    \
		}                                        \
	} while (0)

std::vector<uint64_t> grid(uint64_t top, std::initializer_list<uint64_t> extra) {
	std::vector<uint64_t> v;
	for (uint64_t x = 0; x <= 40 && x <= top; ++x) v.push_back(x);
	for (uint64_t x = 41; x <= top; x = x + x / 7 + 1) v.push_back(x);
	for (uint64_t x : extra) {
		if (x <= top) v.push_back(x);
	}
	v.push_back(top);
	return v;
}

int check() {
	const auto acc = grid(2000, {99, 100, 101, 799, 800, 801, 1999});
	const auto need = grid(2000, {99, 100, 101, 150, 799, 800, 801, 1999});
	const auto pres = grid(800000, {99, 100, 101, 799, 800, 801, 2988, 3000, 79999, 80000, 799999});
	uint64_t points = 0;
	for (uint64_t a : acc) {
		for (uint64_t n : need) {
			for (uint64_t p : pres) {
				const uint32_t got = rxgpu::collect_batch(a, p, n);
				CHECK(got >= 100 && got <= 800, "a=%llu p=%llu n=%llu: %u", (unsigned long long)a, (unsigned long long)p, (unsigned long long)n, got);
#if defined(RX_WITH_REFERENCE)
				const size_t want = reindexer::StreamingKnnEstimator::EstimateBatchSize(size_t(a), size_t(p), size_t(n));
				CHECK(got == want, "a=%llu p=%llu n=%llu: %u != reference %zu", (unsigned long long)a, (unsigned long long)p, (unsigned long long)n, got, want);
#endif
				// where the quotient is exact in integers the estimate is that integer, clamped
				const uint64_t rem = a >= n ? 1 : n - a, den = a ? a : 1;
				if (p % den == 0) {
					const uint64_t v = p / den * rem, want_i = v < 100 ? 100 : v > 800 ? 800 : v;
					CHECK(got == want_i, "a=%llu p=%llu n=%llu: %u != %llu", (unsigned long long)a, (unsigned long long)p, (unsigned long long)n, got,
						  (unsigned long long)want_i);
				}
				++points;
			}
		}
	}
	// values no product of the grid reaches: the clamp happens before the conversion
	CHECK(rxgpu::collect_batch(0, ~uint64_t(0), ~uint64_t(0)) == 800, "2^128");
	CHECK(rxgpu::collect_batch(1, 0, 10) == 100, "nothing presented");
	// the stop test
	for (uint64_t a = 0; a < 4; ++a) {
		for (uint64_t n = 1; n < 4; ++n) {
			for (int ex = 0; ex < 2; ++ex) {
				for (uint64_t c = 1; c < 4; ++c) {
					for (uint64_t mc = 1; mc < 4; ++mc) {
						CHECK(rxgpu::collect_stop(a, n, ex != 0, c, mc) == (a >= n || ex || c >= mc), "stop a=%llu n=%llu", (unsigned long long)a, (unsigned long long)n);
					}
				}
			}
		}
	}
	// the bounds: every collection the rule allows stays inside them — the worst case by brute force: needed - 1 accepted, then a full batch
	for (uint64_t count : {0ull, 1ull, 5ull, 100ull, 899ull, 900ull, 3000ull, 1ull << 32}) {
		for (uint64_t n : {0ull, 1ull, 10ull, 150ull, 100000ull}) {
			for (uint64_t fb : {0ull, 1ull, 16ull, 100ull, 800ull, 801ull, 1200ull}) {
				const uint64_t got = rxgpu::collect_out_bound(count, n, fb);
				if (n == 0 || fb == 0) {
					CHECK(got == 0 && rxgpu::collect_calls_bound(count, n, fb, 1000) == 0, "nothing runs");
					continue;
				}
				const uint64_t mb = fb > 800 ? fb : 800, worst = n - 1 + mb;
				CHECK(got == (count < worst ? count : worst), "count=%llu n=%llu fb=%llu: %llu", (unsigned long long)count, (unsigned long long)n,
					  (unsigned long long)fb, (unsigned long long)got);
				CHECK(rxgpu::collect_max_batch(fb) == mb, "fb=%llu", (unsigned long long)fb);
				for (uint64_t mc : {1ull, 2ull, 1000ull, 1ull << 40}) {
					const uint64_t cb = rxgpu::collect_calls_bound(count, n, fb, mc);
					CHECK(cb == (mc < count + 1 ? mc : count + 1), "calls count=%llu mc=%llu: %llu", (unsigned long long)count, (unsigned long long)mc, (unsigned long long)cb);
				}
			}
		}
	}
	CHECK(rxgpu::collect_out_bound(~uint64_t(0), ~uint64_t(0), 100) == ~uint64_t(0), "saturates");
	std::printf("hnsw_stream_collect_plan_cpu: %s (%llu grid points%s, %d failures)\n", failures ? "FAILED" : "ok", (unsigned long long)points,
#if defined(RX_WITH_REFERENCE)
				", against the reference's estimator",
#else
				"",
#endif
				failures);
	return failures ? 1 : 0;
}

int table(const char* path) {
	std::FILE* f = std::fopen(path, "r");
	if (!f) return 2;
	unsigned long long a, p, n;
	while (std::fscanf(f, "%llu %llu %llu", &a, &p, &n) == 3) std::printf("%u\n", rxgpu::collect_batch(a, p, n));
	std::fclose(f);
	return 0;
}

#if defined(RX_WITH_REFERENCE)
// the same points through the reference's estimator: what tests/golden/make_stream_collect_batches.py records
int reftable(const char* path) {
	std::FILE* f = std::fopen(path, "r");
	if (!f) return 2;
	unsigned long long a, p, n;
	while (std::fscanf(f, "%llu %llu %llu", &a, &p, &n) == 3) {
		std::printf("%zu\n", reindexer::StreamingKnnEstimator::EstimateBatchSize(size_t(a), size_t(p), size_t(n)));
	}
	std::fclose(f);
	return 0;
}
#endif

}  // namespace

int main(int argc, char** argv) {
	if (argc >= 3 && !std::strcmp(argv[1], "table")) return table(argv[2]);
#if defined(RX_WITH_REFERENCE)
	if (argc >= 3 && !std::strcmp(argv[1], "reftable")) return reftable(argv[2]);
#endif
	return check();
}
