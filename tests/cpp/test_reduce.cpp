// spsamd_reduce through the plain C ABI on a hand-written 3 x 3 matrix: every op and post-operation against answers written
// out below, the capacity query, and result == NULL.  Prints OK on success.
#include <spsparse_amd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

static int failures = 0;

static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

static void expect(const char *what, int op, int post, size_t n, const int32_t *gi, const double *gv, size_t wn, const int32_t *wi, const double *wv)
{
	if (n != wn) { std::printf("FAIL %s op %d post %d: %zu entries, want %zu\n", what, op, post, n, wn); ++failures; return; }
	for (size_t k = 0; k < wn; ++k)
		if ((gi && gi[k] != wi[k]) || std::memcmp(&gv[k], &wv[k], 8) != 0) {
			std::printf("FAIL %s op %d post %d [%zu]: (%d, %.17g) vs (%d, %.17g)\n", what, op, post, k, gi ? gi[k] : -1, gv[k], wi[k], wv[k]);
			++failures;
		}
}

int main()
{
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	// row 0: (0,0) 4     (0,2) -3
	// row 1: (1,0) 2                      (no diagonal entry)
	// row 2: (2,2) 0.25  (2,1) -1         (stored in this order: a trusted operand keeps it)
	const int32_t i0[5] = {0, 0, 1, 2, 2}, i1[5] = {0, 2, 0, 2, 1};
	const double v[5] = {4.0, -3.0, 2.0, 0.25, -1.0};
	const spsamd_coo A = {i0, i1, v, 5, 3, 3, 0, SPSAMD_MEM_HOST};
	const double dnan = with_bits(0xFFF8000000000000ull);
	const int32_t all[3] = {0, 1, 2}, dg[2] = {0, 2};
	// [op - 1][post][entry]
	const double want[6][4][3] = {
		/* SUM     */ {{1.0, 2.0, -0.75}, {1.0, 0.5, -1.3333333333333333}, {1.0, 1.4142135623730951, dnan}, {1.0, 0.70710678118654746, dnan}},
		/* SUM_ABS */ {{7.0, 2.0, 1.25}, {0.14285714285714285, 0.5, 0.8}, {2.6457513110645907, 1.4142135623730951, 1.1180339887498949},
		               {0.37796447300922720, 0.70710678118654746, 0.89442719099991586}},
		/* SUM_SQ  */ {{25.0, 4.0, 1.0625}, {0.04, 0.25, 0.94117647058823528}, {5.0, 2.0, 1.0307764064044151}, {0.2, 0.5, 0.97014250014533188}},
		/* MAX_ABS */ {{4.0, 2.0, 1.0}, {0.25, 0.5, 1.0}, {2.0, 1.4142135623730951, 1.0}, {0.5, 0.70710678118654746, 1.0}},
		/* COUNT   */ {{2.0, 1.0, 2.0}, {0.5, 1.0, 0.5}, {1.4142135623730951, 1.0, 1.4142135623730951}, {0.70710678118654746, 1.0, 0.70710678118654746}},
		/* DIAG    */ {{4.0, 0.25, 0.0}, {0.25, 4.0, 0.0}, {2.0, 0.5, 0.0}, {0.5, 2.0, 0.0}},        // rows 0 and 2 only
	};
	for (int op = SPSAMD_REDUCE_SUM; op <= SPSAMD_REDUCE_DIAG; ++op)
		for (int post = SPSAMD_POST_NONE; post <= SPSAMD_POST_RSQRT; ++post) {
			const bool diag = op == SPSAMD_REDUCE_DIAG;
			int32_t gi[3] = {-3, -3, -3};
			double gv[3] = {-7.5, -7.5, -7.5};
			size_t n = 99;
			spsamd_result res;
			int rc = spsamd_reduce(ctx, &A, '.', op, post, SPSAMD_ADD, 0, gi, gv, 3, SPSAMD_MEM_HOST, &n, &res);
			if (rc != SPSAMD_OK) { std::printf("FAIL op %d post %d: rc %d %s\n", op, post, rc, spsamd_last_error(ctx)); ++failures; continue; }
			expect("sparse", op, post, n, gi, gv, diag ? 2 : 3, diag ? dg : all, want[op - 1][post]);
			if (res.shape0 != 3 || res.shape1 != 0 || res.nnz != n || res.nnz_a != 5) { std::printf("FAIL result of op %d\n", op); ++failures; }
			// the dense form, result == NULL: the row without a contributing tuple holds +0.0
			double gd[3] = {-7.5, -7.5, -7.5};
			rc = spsamd_reduce(ctx, &A, '.', op, post, SPSAMD_ADD, 0, nullptr, gd, 3, SPSAMD_MEM_HOST, &n, nullptr);
			const double dd[3] = {want[5][post][0], 0.0, want[5][post][1]};
			if (rc != SPSAMD_OK) { std::printf("FAIL dense op %d post %d: rc %d\n", op, post, rc); ++failures; continue; }
			expect("dense", op, post, 3, nullptr, gd, 3, all, diag ? dd : want[op - 1][post]);
			if (n != (diag ? 2u : 3u)) { std::printf("FAIL dense count of op %d: %zu\n", op, n); ++failures; }
		}
	{   // column sums: the same call with 'T' (the raw operand is consolidated by columns)
		const spsamd_coo R = {i0, i1, v, 5, 3, 3, -1, SPSAMD_MEM_HOST};
		int32_t gi[3]; double gv[3]; size_t n = 0;
		const double w[3] = {6.0, -1.0, -2.75};
		if (spsamd_reduce(ctx, &R, 'T', SPSAMD_REDUCE_SUM, SPSAMD_POST_NONE, SPSAMD_ADD, 0, gi, gv, 3, SPSAMD_MEM_HOST, &n, nullptr) != SPSAMD_OK) { std::printf("FAIL 'T'\n"); ++failures; }
		else expect("column sums", 1, 0, n, gi, gv, 3, all, w);
	}
	{   // the capacity query: ECAPACITY, the count, nothing written
		int32_t gi[3] = {-3, -3, -3};
		double gv[3] = {-7.5, -7.5, -7.5};
		size_t n = 99;
		int rc = spsamd_reduce(ctx, &A, '.', SPSAMD_REDUCE_DIAG, SPSAMD_POST_NONE, SPSAMD_ADD, 0, gi, gv, 0, SPSAMD_MEM_HOST, &n, nullptr);
		if (rc != SPSAMD_ECAPACITY || n != 2 || gi[0] != -3 || gv[0] != -7.5) { std::printf("FAIL capacity query: rc %d n %zu\n", rc, n); ++failures; }
		rc = spsamd_reduce(ctx, &A, '.', SPSAMD_REDUCE_SUM, SPSAMD_POST_NONE, SPSAMD_ADD, 0, gi, gv, 2, SPSAMD_MEM_HOST, &n, nullptr);
		if (rc != SPSAMD_ECAPACITY || n != 3 || gi[0] != -3 || gv[0] != -7.5) { std::printf("FAIL capacity 2: rc %d n %zu\n", rc, n); ++failures; }
		rc = spsamd_reduce(ctx, &A, '.', SPSAMD_REDUCE_SUM, SPSAMD_POST_NONE, SPSAMD_ADD, 0, nullptr, gv, 2, SPSAMD_MEM_HOST, &n, nullptr);
		if (rc != SPSAMD_ECAPACITY || gv[0] != -7.5) { std::printf("FAIL dense capacity: rc %d\n", rc); ++failures; }
		rc = spsamd_reduce(ctx, &A, '.', 0, SPSAMD_POST_NONE, SPSAMD_ADD, 0, gi, gv, 3, SPSAMD_MEM_HOST, &n, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL unknown op: rc %d\n", rc); ++failures; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
