// spsamd_emult through the plain C ABI on a hand-written 4 x 4 pair: TIMES, FIRST and FIRST | COMPLEMENT against answers written
// out below (fetched through spsamd_result_fetch), and the error codes.  Prints OK on success.
#include <spsparse_amd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

struct Tup { int32_t i, j; double v; };

static int collect(void *user, const int32_t *i, const int32_t *j, const double *v, size_t n)
{
	auto *out = (std::vector<Tup> *)user;
	for (size_t k = 0; k < n; ++k) out->push_back(Tup{i[k], j[k], v[k]});
	return 0;
}

static void expect(spsamd_ctx *ctx, const char *what, int rc, const spsamd_result &res, const std::vector<Tup> &want, uint64_t nnz_b)
{
	if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; return; }
	std::vector<Tup> got;
	if (spsamd_result_fetch(ctx, &res, collect, &got) != SPSAMD_OK) { std::printf("FAIL %s: fetch\n", what); ++failures; return; }
	if (res.shape0 != 4 || res.shape1 != 4 || res.nnz != want.size() || res.nnz_a != 6 || res.nnz_b != nnz_b) {
		std::printf("FAIL %s: result fields (nnz %llu nnz_a %llu nnz_b %llu)\n", what, (unsigned long long)res.nnz,
			(unsigned long long)res.nnz_a, (unsigned long long)res.nnz_b);
		++failures;
	}
	if (got.size() != want.size()) { std::printf("FAIL %s: %zu tuples, want %zu\n", what, got.size(), want.size()); ++failures; return; }
	for (size_t k = 0; k < want.size(); ++k)
		if (got[k].i != want[k].i || got[k].j != want[k].j || std::memcmp(&got[k].v, &want[k].v, 8) != 0) {
			std::printf("FAIL %s [%zu]: (%d, %d, %.17g) vs (%d, %d, %.17g)\n", what, k, got[k].i, got[k].j, got[k].v, want[k].i, want[k].j, want[k].v);
			++failures;
		}
}

static void refused(spsamd_ctx *ctx, const char *what, int rc, int want)
{
	if (rc != want || !spsamd_last_error(ctx)[0]) { std::printf("FAIL %s: rc %d, want %d\n", what, rc, want); ++failures; }
}

int main()
{
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	// A, in row-major order and saying so:   (0,0) 2   (0,2) -3   (1,1) 4   (2,0) 0.5   (2,3) 8   (3,3) -1
	const int32_t a0[6] = {0, 0, 1, 2, 2, 3}, a1[6] = {0, 2, 1, 0, 3, 3};
	const double av[6] = {2.0, -3.0, 4.0, 0.5, 8.0, -1.0};
	const spsamd_coo A = {a0, a1, av, 6, 4, 4, 0, SPSAMD_MEM_HOST};
	// B, the same way, its key (0,2) twice:  (0,2) 10  (0,2) 100  (1,0) 7  (1,1) 0.25  (2,3) -2  (3,0) 1
	const int32_t b0[6] = {0, 0, 1, 1, 2, 3}, b1[6] = {2, 2, 0, 1, 3, 0};
	const double bv[6] = {10.0, 100.0, 7.0, 0.25, -2.0, 1.0};
	const spsamd_coo B = {b0, b1, bv, 6, 4, 4, 0, SPSAMD_MEM_HOST};
	spsamd_coo Bkeys = B;
	Bkeys.val = nullptr;                                        // FIRST never reads B's values
	spsamd_result res;
	for (long path = 0; path <= 3; ++path) {
		if (spsamd_ctx_set_tuning(ctx, "emult_path", path) != SPSAMD_OK) { std::printf("FAIL knob\n"); ++failures; }
		// (alpha * a) * b with the FIRST (0,2) of B
		int rc = spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 2.0, &A, '.', &B, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res);
		expect(ctx, "TIMES", rc, res, {{0, 2, -60.0}, {1, 1, 2.0}, {2, 3, -32.0}}, 6);
		rc = spsamd_emult(ctx, SPSAMD_EMULT_FIRST, 0, 2.0, &A, '.', &Bkeys, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res);
		expect(ctx, "FIRST", rc, res, {{0, 2, -3.0}, {1, 1, 4.0}, {2, 3, 8.0}}, 5);
		rc = spsamd_emult(ctx, SPSAMD_EMULT_FIRST, SPSAMD_EMULT_COMPLEMENT, 2.0, &A, '.', &Bkeys, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res);
		expect(ctx, "FIRST | COMPLEMENT", rc, res, {{0, 0, 2.0}, {2, 0, 0.5}, {3, 3, -1.0}}, 5);
		if ((path == 1 && res.products != 0) || (path >= 2 && res.products == 0)) { std::printf("FAIL products of path %ld\n", path); ++failures; }
	}
	spsamd_ctx_set_tuning(ctx, "emult_path", 0);
	refused(ctx, "unknown op", spsamd_emult(ctx, 0, 0, 1.0, &A, '.', &B, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "unknown flag", spsamd_emult(ctx, SPSAMD_EMULT_FIRST, 2, 1.0, &A, '.', &B, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "COMPLEMENT with TIMES", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, SPSAMD_EMULT_COMPLEMENT, 1.0, &A, '.', &B, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "NULL A", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 1.0, nullptr, '.', &B, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "NULL val under TIMES", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 1.0, &A, '.', &Bkeys, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "bad policy", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 1.0, &A, '.', &B, '.', 3, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EINVAL);
	refused(ctx, "bad sink", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 1.0, &A, '.', &B, '.', SPSAMD_ADD, 0, 7, 0, &res), SPSAMD_EINVAL);
	spsamd_coo W = B;
	W.shape1 = 5;
	refused(ctx, "shapes", spsamd_emult(ctx, SPSAMD_EMULT_TIMES, 0, 1.0, &A, '.', &W, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &res), SPSAMD_EDIM);
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
