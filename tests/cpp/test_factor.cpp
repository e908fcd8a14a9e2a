// spsamd_factor_ilu0 through the plain C ABI against the row-wise loop written out in C++ (compiled with -ffp-contract=off:
// g++ emits mulsd, subsd and divsd as written, so a NaN carries the bits real x86-64 hardware gives it).  A Laplace 32^3
// from spsamd_gen_laplace3d and a symmetrised R-MAT scale 14 (spsamd_gen_rmat, then spsamd_add of A and A^T, then of a
// diagonal), both built on the device; then the application U^-1 L^-1 b by two spsamd_solve_tri calls chained from the
// factor through a prepared handle.  Prints OK on success.
#include <spsparse_amd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int hipMalloc(void **ptr, size_t bytes);     // the runtime the library is linked against: device arrays for the generators
extern "C" int hipFree(void *ptr);

static int failures = 0;

static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

struct Tuples { std::vector<int32_t> i, j; std::vector<double> v; };

struct Counters { uint64_t lookups = 0, updates = 0; int64_t zero_pivot = -1, missing_diag = -1; };

// the loop of the header over row-major, strictly ascending tuples; f in place of S.v
static Counters ilu0_loop(Tuples &S, int n)
{
	Counters c;
	std::vector<size_t> beg(n + 1, 0), dpos(n, SIZE_MAX), ustart(n);
	for (size_t t = 0; t < S.v.size(); ++t) ++beg[S.i[t] + 1];
	for (int i = 0; i < n; ++i) beg[i + 1] += beg[i];
	for (int i = 0; i < n; ++i) {
		size_t u = beg[i];
		while (u < beg[i + 1] && S.j[u] < i) ++u;
		if (u < beg[i + 1] && S.j[u] == i) dpos[i] = u++;
		ustart[i] = u;
	}
	double *f = S.v.data();
	for (int i = 0; i < n; ++i) {
		for (size_t t = beg[i]; t < beg[i + 1] && S.j[t] < i; ++t) {
			const int k = S.j[t];
			const double p = dpos[k] != SIZE_MAX ? f[dpos[k]] : 0.0;
			f[t] = f[t] / p;
			size_t u = t + 1;
			for (size_t s = ustart[k]; s < beg[k + 1]; ++s) {
				++c.lookups;
				while (u < beg[i + 1] && S.j[u] < S.j[s]) ++u;
				if (u < beg[i + 1] && S.j[u] == S.j[s]) { const double prod = f[t] * f[s]; f[u] = f[u] - prod; ++c.updates; }
			}
		}
		if (dpos[i] == SIZE_MAX) { if (c.missing_diag < 0) c.missing_diag = i; if (c.zero_pivot < 0) c.zero_pivot = i; }
		else if (f[dpos[i]] == 0.0 && c.zero_pivot < 0) c.zero_pivot = i;
	}
	return c;
}

// L y = b (unit diagonal), then U x = y: the loop of spsamd_solve_tri over F
static void apply_loop(const Tuples &F, int n, const double *b, double *x, int nrhs)
{
	std::vector<size_t> beg(n + 1, 0);
	for (size_t t = 0; t < F.v.size(); ++t) ++beg[F.i[t] + 1];
	for (int i = 0; i < n; ++i) beg[i + 1] += beg[i];
	std::vector<double> y((size_t)n * nrhs);
	for (int r = 0; r < nrhs; ++r) {
		for (int i = 0; i < n; ++i) {
			double acc = b[(size_t)i * nrhs + r];
			for (size_t t = beg[i]; t < beg[i + 1]; ++t)
				if (F.j[t] < i) { const double p = F.v[t] * y[(size_t)F.j[t] * nrhs + r]; acc = acc - p; }
			y[(size_t)i * nrhs + r] = acc;
		}
		for (int i = n - 1; i >= 0; --i) {
			double acc = y[(size_t)i * nrhs + r], d = 0.0;
			for (size_t t = beg[i]; t < beg[i + 1]; ++t) {
				if (F.j[t] == i) d = d + F.v[t];
				else if (F.j[t] > i) { const double p = F.v[t] * x[(size_t)F.j[t] * nrhs + r]; acc = acc - p; }
			}
			x[(size_t)i * nrhs + r] = acc / d;
		}
	}
}

static bool to_host(spsamd_ctx *ctx, const spsamd_result &res, Tuples *out)
{
	out->i.resize(res.nnz); out->j.resize(res.nnz); out->v.resize(res.nnz);
	return spsamd_memcpy(ctx, out->i.data(), res.idx0, res.nnz * 4) == SPSAMD_OK && spsamd_memcpy(ctx, out->j.data(), res.idx1, res.nnz * 4) == SPSAMD_OK &&
		spsamd_memcpy(ctx, out->v.data(), res.val, res.nnz * 8) == SPSAMD_OK;
}

// factor `A` (a device operand whose tuples `S` holds), compare with the loop, then apply F to two right-hand sides
static void run_case(spsamd_ctx *ctx, const char *what, const spsamd_coo &A, Tuples &S, int n)
{
	spsamd_factor_stats st;
	spsamd_result res;
	int rc = spsamd_factor_ilu0(ctx, &A, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &st, &res);
	if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; return; }
	const Counters c = ilu0_loop(S, n);
	Tuples F;
	if (!to_host(ctx, res, &F) || F.v.size() != S.v.size()) { std::printf("FAIL %s: %zu tuples, want %zu\n", what, F.v.size(), S.v.size()); ++failures; return; }
	size_t bad = 0, first = 0;
	for (size_t t = F.v.size(); t-- > 0;)
		if (F.i[t] != S.i[t] || F.j[t] != S.j[t] || bits_of(F.v[t]) != bits_of(S.v[t])) { ++bad; first = t; }
	if (bad) {
		std::printf("FAIL %s: %zu tuples differ, first at %zu: (%d, %d, %.17g) vs (%d, %d, %.17g)\n", what, bad, first, F.i[first], F.j[first], F.v[first],
			S.i[first], S.j[first], S.v[first]);
		++failures;
	}
	if (st.lookups != c.lookups || st.updates != c.updates || st.zero_pivot != c.zero_pivot || st.missing_diag != c.missing_diag || res.products != c.lookups) {
		std::printf("FAIL %s: counters %llu %llu %lld %lld, want %llu %llu %lld %lld\n", what, (unsigned long long)st.lookups, (unsigned long long)st.updates,
			(long long)st.zero_pivot, (long long)st.missing_diag, (unsigned long long)c.lookups, (unsigned long long)c.updates, (long long)c.zero_pivot, (long long)c.missing_diag);
		++failures;
	}
	std::printf("%s: n %d tuples %zu levels %llu lookups %llu updates %llu launches %llu\n", what, n, S.v.size(), (unsigned long long)st.levels,
		(unsigned long long)st.lookups, (unsigned long long)st.updates, (unsigned long long)st.launches);
	// the application, chained: F as a device operand, prepared once, two solves per right-hand-side block
	const spsamd_coo Fop = {res.idx0, res.idx1, res.val, (size_t)res.nnz, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};
	spsamd_operand *h = nullptr;
	rc = spsamd_operand_prepare(ctx, &Fop, '.', SPSAMD_AS_A, SPSAMD_ADD, 0, &h);
	spsamd_coo Fh;
	if (rc != SPSAMD_OK || spsamd_operand_as_coo(h, &Fh) != SPSAMD_OK) { std::printf("FAIL %s: prepare rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; return; }
	const int nrhs = 2;
	std::vector<double> b((size_t)n * nrhs), y(b.size()), x(b.size()), want(b.size());
	for (size_t k = 0; k < b.size(); ++k) b[k] = 1.0 + 0.001 * (double)(k % 977) - 0.5 * (double)(k % 3);
	rc = spsamd_solve_tri(ctx, &Fh, '.', SPSAMD_TRI_LOWER, SPSAMD_DIAG_UNIT, b.data(), nrhs, y.data(), nrhs, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
	if (rc == SPSAMD_OK)
		rc = spsamd_solve_tri(ctx, &Fh, '.', SPSAMD_TRI_UPPER, SPSAMD_DIAG_NONUNIT, y.data(), nrhs, x.data(), nrhs, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
	if (rc != SPSAMD_OK) { std::printf("FAIL %s: solve rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; }
	else {
		apply_loop(S, n, b.data(), want.data(), nrhs);
		size_t badx = 0;
		for (size_t k = 0; k < x.size(); ++k) if (bits_of(x[k]) != bits_of(want[k])) ++badx;
		if (badx) { std::printf("FAIL %s: %zu values of U^-1 L^-1 b differ\n", what, badx); ++failures; }
	}
	spsamd_operand_destroy(h);
}

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "--abi-only")) { std::printf("OK\n"); return 0; }
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	{   // Laplace 32^3
		const uint64_t N = 32, n = N * N * N, m = 7 * n - 6 * N * N;
		void *d0 = nullptr, *d1 = nullptr, *dv = nullptr;
		if (hipMalloc(&d0, m * 4) || hipMalloc(&d1, m * 4) || hipMalloc(&dv, m * 8)) { std::printf("FAIL hipMalloc\n"); return 1; }
		int rc = spsamd_gen_laplace3d(ctx, N, (int32_t *)d0, (int32_t *)d1, (double *)dv);
		if (rc != SPSAMD_OK) { std::printf("FAIL gen_laplace3d rc %d\n", rc); return 1; }
		const spsamd_coo A = {(const int32_t *)d0, (const int32_t *)d1, (const double *)dv, (size_t)m, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};
		Tuples S;
		S.i.resize(m); S.j.resize(m); S.v.resize(m);
		if (spsamd_memcpy(ctx, S.i.data(), d0, m * 4) || spsamd_memcpy(ctx, S.j.data(), d1, m * 4) || spsamd_memcpy(ctx, S.v.data(), dv, m * 8)) { std::printf("FAIL memcpy\n"); return 1; }
		run_case(ctx, "laplace 32^3", A, S, (int)n);
		hipFree(d0); hipFree(d1); hipFree(dv);
	}
	{   // R-MAT scale 14, edge factor 8: A + A^T (duplicates added), then + 4096 I
		const int scale = 14, ef = 8;
		const uint64_t n = 1ull << scale, m = (uint64_t)ef * n;
		void *d0 = nullptr, *d1 = nullptr, *dv = nullptr;
		if (hipMalloc(&d0, m * 4) || hipMalloc(&d1, m * 4) || hipMalloc(&dv, m * 8)) { std::printf("FAIL hipMalloc\n"); return 1; }
		int rc = spsamd_gen_rmat(ctx, scale, ef, 3, 0, m, (int32_t *)d0, (int32_t *)d1, (double *)dv);
		if (rc != SPSAMD_OK) { std::printf("FAIL gen_rmat rc %d\n", rc); return 1; }
		const spsamd_coo A = {(const int32_t *)d0, (const int32_t *)d1, (const double *)dv, (size_t)m, (size_t)n, (size_t)n, -1, SPSAMD_MEM_DEVICE};
		spsamd_result sym, shifted;
		rc = spsamd_add(ctx, 1.0, &A, '.', 1.0, &A, 'T', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &sym);
		if (rc != SPSAMD_OK) { std::printf("FAIL add rc %d %s\n", rc, spsamd_last_error(ctx)); return 1; }
		std::vector<int32_t> di(n);
		std::vector<double> dd(n, 4096.0);
		for (uint64_t k = 0; k < n; ++k) di[k] = (int32_t)k;
		const spsamd_coo symop = {sym.idx0, sym.idx1, sym.val, (size_t)sym.nnz, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};
		const spsamd_coo D = {di.data(), di.data(), dd.data(), (size_t)n, (size_t)n, (size_t)n, 0, SPSAMD_MEM_HOST};
		rc = spsamd_add(ctx, 1.0, &symop, '.', 1.0, &D, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &shifted);
		if (rc != SPSAMD_OK) { std::printf("FAIL add of the diagonal rc %d %s\n", rc, spsamd_last_error(ctx)); return 1; }
		Tuples S;
		if (!to_host(ctx, shifted, &S)) { std::printf("FAIL memcpy\n"); return 1; }
		const spsamd_coo op = {shifted.idx0, shifted.idx1, shifted.val, (size_t)shifted.nnz, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};
		run_case(ctx, "rmat 14", op, S, (int)n);
		hipFree(d0); hipFree(d1); hipFree(dv);
	}
	{   // refusals
		int32_t i0[3] = {0, 1, 1}, i1[3] = {0, 1, 1};
		double v[3] = {1, 2, 3};
		const spsamd_coo dup = {i0, i1, v, 3, 2, 2, 0, SPSAMD_MEM_HOST}, wide = {i0, i1, v, 3, 2, 3, -1, SPSAMD_MEM_HOST};
		spsamd_result res;
		int rc = spsamd_factor_ilu0(ctx, &dup, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, nullptr, &res);
		if (rc != SPSAMD_EINVAL || !std::strstr(spsamd_last_error(ctx), "position 2")) { std::printf("FAIL duplicate key: rc %d %s\n", rc, spsamd_last_error(ctx)); ++failures; }
		rc = spsamd_factor_ilu0(ctx, &wide, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, nullptr, &res);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL not square: rc %d\n", rc); ++failures; }
		rc = spsamd_factor_ilu0(ctx, &dup, '.', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL null result: rc %d\n", rc); ++failures; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
