// spsamd_solve_tri through the plain C ABI against the substitution loop written out in C++: g++ emits mulsd, addsd, subsd
// and divsd as written, so the NaN a result carries here is the one real x86-64 hardware gives it.  A trusted 6 x 6 operand
// with both triangles, duplicates, an explicit zero, a missing diagonal and NaNs of several payloads; both triangles, both
// diagonals, both transposes; then one Gauss-Seidel sweep chained from spsamd_multiply_dense.  Prints OK on success.
#include <spsparse_amd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }
static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

struct Tuples { std::vector<int32_t> i, j; std::vector<double> v; };

// the loop of the header over the tuples in storage order (row-major: the rows ascend), `nrhs` right-hand sides
static void solve_loop(const Tuples &S, int n, int uplo, int diag, const double *B, int ldb, double *X, int ldx, int nrhs)
{
	for (int r = 0; r < nrhs; ++r)
		for (int s = 0; s < n; ++s) {
			const int i = uplo == SPSAMD_TRI_UPPER ? n - 1 - s : s;
			volatile double acc = B[i * ldb + r], d = 0.0;
			for (size_t t = 0; t < S.v.size(); ++t) {
				if (S.i[t] != i) continue;
				const int j = S.j[t];
				if (j == i) { if (diag == SPSAMD_DIAG_NONUNIT) d = d + S.v[t]; continue; }
				if ((j < i) != (uplo == SPSAMD_TRI_LOWER)) continue;
				volatile double p = S.v[t] * X[j * ldx + r];
				acc = acc - p;
			}
			X[i * ldx + r] = diag == SPSAMD_DIAG_UNIT ? (double)acc : acc / d;
		}
}

static void compare(const char *what, const double *got, const double *want, int n, int ld, int nrhs)
{
	for (int i = 0; i < n; ++i)
		for (int r = 0; r < ld; ++r)
			if (bits_of(got[i * ld + r]) != bits_of(want[i * ld + r])) {
				std::printf("FAIL %s [%d, %d]%s: %.17g (%016llx) vs %.17g (%016llx)\n", what, i, r, r >= nrhs ? " (padding)" : "", got[i * ld + r],
					(unsigned long long)bits_of(got[i * ld + r]), want[i * ld + r], (unsigned long long)bits_of(want[i * ld + r]));
				++failures;
			}
}

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "--abi-only")) { std::printf("OK\n"); return 0; }
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	const double qa = with_bits(0x7FF80000DEADBEEFull), qb = with_bits(0xFFF8000000000123ull), sn = with_bits(0x7FF0000000000001ull);
	const int n = 6;
	// stored by rows, the columns of a row in no order; row 3 has no diagonal, (4, 4) is stored twice, (5, 2) is an explicit zero
	Tuples S;
	S.i = {0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 5};
	S.j = {0, 3, 1, 0, 5, 1, 2, 0, 4, 0, 2, 5, 4, 1, 4, 3, 5, 2, 0, 4, 1};
	S.v = {2.0, 0.5, -4.0, 1.5, qa, 0.25, 0.5, -1.0, 3.0, 1.0, qb, -2.0, 1.0, sn, 0.5, 0.125, -0.0, 0.0, 7.0, -3.0, 1.0 / 3.0};
	const spsamd_coo A = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), (size_t)n, (size_t)n, 0, SPSAMD_MEM_HOST};
	Tuples St;                                  // op(A) under 'T', as the call takes a raw operand: consolidated by columns
	for (int c = 0; c < n; ++c)
		for (int r = 0; r < n; ++r) {
			bool have = false; double acc = 0.0;
			for (size_t t = 0; t < S.v.size(); ++t)
				if (S.j[t] == c && S.i[t] == r && S.v[t] != 0.0) { acc = have ? acc + S.v[t] : S.v[t]; have = true; }
			if (have) { St.i.push_back(c); St.j.push_back(r); St.v.push_back(acc); }
		}
	const spsamd_coo Araw = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), (size_t)n, (size_t)n, -1, SPSAMD_MEM_HOST};
	const int nrhs = 3, ld = 4;
	double B[n * ld];
	for (int i = 0; i < n; ++i)
		for (int r = 0; r < ld; ++r) B[i * ld + r] = r < nrhs ? (i + 1) * (r == 1 ? -0.75 : 1.0) + 0.1 * r : -7.5;
	B[2 * ld + 2] = qb;
	for (int uplo = 0; uplo < 2; ++uplo)
		for (int diag = 0; diag < 2; ++diag)
			for (int tr = 0; tr < 2; ++tr) {
				char what[64];
				std::snprintf(what, sizeof what, "uplo %d diag %d %s", uplo, diag, tr ? "'T'" : "'.'");
				double X[n * ld], W[n * ld];
				for (int k = 0; k < n * ld; ++k) X[k] = W[k] = -7.5;
				solve_loop(tr ? St : S, n, uplo, diag, B, ld, W, ld, nrhs);
				spsamd_solve_stats st;
				spsamd_result res;
				const int rc = spsamd_solve_tri(ctx, tr ? &Araw : &A, tr ? 'T' : '.', uplo, diag, B, ld, X, ld, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, &st, &res);
				if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; continue; }
				compare(what, X, W, n, ld, nrhs);
				if (res.shape0 != (uint64_t)n || res.shape1 != (uint64_t)n || res.nnz_a != (tr ? St.v.size() : S.v.size())) { std::printf("FAIL result of %s\n", what); ++failures; }
				if (!tr && uplo == SPSAMD_TRI_LOWER && st.zero_pivot != (diag ? -1 : 3)) { std::printf("FAIL zero pivot of %s: %lld\n", what, (long long)st.zero_pivot); ++failures; }
				if (!tr && uplo == SPSAMD_TRI_UPPER && st.zero_pivot != (diag ? -1 : 3)) { std::printf("FAIL zero pivot of %s: %lld\n", what, (long long)st.zero_pivot); ++failures; }
			}
	{   // in place, stats and result NULL
		double X[n * ld], W[n * ld];
		for (int k = 0; k < n * ld; ++k) { X[k] = B[k]; W[k] = -7.5; }
		solve_loop(S, n, SPSAMD_TRI_LOWER, SPSAMD_DIAG_NONUNIT, B, ld, W, ld, nrhs);
		const int rc = spsamd_solve_tri(ctx, &A, '.', SPSAMD_TRI_LOWER, SPSAMD_DIAG_NONUNIT, X, ld, X, ld, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_OK) { std::printf("FAIL in place: rc %d %s\n", rc, spsamd_last_error(ctx)); ++failures; }
		else compare("in place", X, W, n, ld, nrhs);
	}
	{   // one Gauss-Seidel sweep on a diagonally dominant 5 x 5 matrix: r = b - M x through multiply_dense, x += (D + L)^-1 r
		const int m = 5;
		Tuples M;
		for (int i = 0; i < m; ++i)
			for (int j = 0; j < m; ++j)
				if (i == j || (i + 2 * j) % 3 == 0) { M.i.push_back(i); M.j.push_back(j); M.v.push_back(i == j ? 4.0 + 0.1 * i : 1.0 / (3 + i + j)); }
		const spsamd_coo Mc = {M.i.data(), M.j.data(), M.v.data(), M.v.size(), (size_t)m, (size_t)m, 0, SPSAMD_MEM_HOST};
		double b[m], x[m], xm[m], r[m], wr[m], dx[m], wdx[m];
		for (int i = 0; i < m; ++i) { b[i] = 1.0 + 0.3 * i; x[i] = 0.1 * (i - 2); xm[i] = -x[i]; r[i] = wr[i] = b[i]; }
		for (size_t t = 0; t < M.v.size(); ++t) { volatile double p = M.v[t] * xm[M.j[t]]; wr[M.i[t]] = wr[M.i[t]] + p; }
		int rc = spsamd_multiply_dense(ctx, &Mc, '.', xm, 1, r, 1, 1, SPSAMD_MEM_HOST, SPSAMD_ADD, 0);
		if (rc != SPSAMD_OK) { std::printf("FAIL multiply_dense: rc %d\n", rc); ++failures; }
		compare("residual", r, wr, m, 1, 1);
		solve_loop(M, m, SPSAMD_TRI_LOWER, SPSAMD_DIAG_NONUNIT, wr, 1, wdx, 1, 1);
		spsamd_solve_stats st;
		rc = spsamd_solve_tri(ctx, &Mc, '.', SPSAMD_TRI_LOWER, SPSAMD_DIAG_NONUNIT, r, 1, dx, 1, 1, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, &st, nullptr);
		if (rc != SPSAMD_OK) { std::printf("FAIL sweep: rc %d %s\n", rc, spsamd_last_error(ctx)); ++failures; }
		compare("sweep", dx, wdx, m, 1, 1);
		if (st.zero_pivot != -1 || st.levels < 2) { std::printf("FAIL sweep stats\n"); ++failures; }
		// the sweep reduces the residual of this dominant matrix
		double before = 0, after = 0;
		for (int i = 0; i < m; ++i) { x[i] += dx[i]; before += wr[i] * wr[i]; }
		for (int i = 0; i < m; ++i) { double s = b[i]; for (size_t t = 0; t < M.v.size(); ++t) if (M.i[t] == i) s -= M.v[t] * x[M.j[t]]; after += s * s; }
		if (!(after < 0.25 * before)) { std::printf("FAIL the sweep did not reduce the residual: %g -> %g\n", before, after); ++failures; }
	}
	{   // errors: X untouched
		double X[n * ld];
		for (int k = 0; k < n * ld; ++k) X[k] = -7.5;
		int rc = spsamd_solve_tri(ctx, &A, '.', 2, 0, B, ld, X, ld, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL bad uplo: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_tri(ctx, &A, '.', 0, 0, B, 2, X, ld, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL ldb < nrhs: rc %d\n", rc); ++failures; }
		const spsamd_coo R = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), 6, 7, 0, SPSAMD_MEM_HOST};
		rc = spsamd_solve_tri(ctx, &R, '.', 0, 0, B, ld, X, ld, nrhs, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL not square: rc %d\n", rc); ++failures; }
		for (int k = 0; k < n * ld; ++k) if (X[k] != -7.5) { std::printf("FAIL an error wrote X\n"); ++failures; break; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
