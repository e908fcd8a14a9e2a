// spsamd_solve_gmres through the plain C ABI against the loop of the header written out in C++ and compiled by g++ with
// -ffp-contract=off: mulsd, addsd, subsd, divsd and sqrtsd as written, the fold in its fixed shape.  An upwind 1-D
// convection-diffusion operator of order 2500 (three chunks, two levels of the fold) with a right-hand side of mixed
// magnitudes under restart 7; no preconditioner, Jacobi, and the LU factors of the unperturbed stencil as M; then a 6 x 6
// operand with a NaN; then the refusals.  Prints OK on success.
#include <spsparse_amd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;

static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

struct Tuples { std::vector<int32_t> i, j; std::vector<double> v; };

static double fold(std::vector<double> t)
{
	for (;;) {
		const size_t m = t.size();
		if (m == 0) return 0.0;
		const size_t c = (m + 1023) / 1024;
		std::vector<double> out(c);
		for (size_t g = 0; g < c; ++g) {
			volatile double a[64];
			for (int l = 0; l < 64; ++l) {
				a[l] = 0.0;
				for (int k = 0; k < 16; ++k) {
					const size_t e = 1024 * g + 64 * k + l;
					if (e < m) a[l] = a[l] + t[e];
				}
			}
			for (int s = 32; s >= 1; s >>= 1)
				for (int l = 0; l < s; ++l) a[l] = a[l] + a[l + s];
			out[g] = a[0];
		}
		if (c == 1) return out[0];
		t = out;
	}
}

static double dot(const std::vector<double> &u, const std::vector<double> &w)
{
	std::vector<double> t(u.size());
	for (size_t e = 0; e < u.size(); ++e) { volatile double p = u[e] * w[e]; t[e] = p; }
	return fold(t);
}

// S row-major: the rows ascend
static std::vector<double> apply(const Tuples &S, int n, const std::vector<double> &p)
{
	std::vector<double> q(n, 0.0);
	for (size_t t = 0; t < S.v.size(); ++t) { volatile double pr = S.v[t] * p[S.j[t]]; q[S.i[t]] = q[S.i[t]] + pr; }
	return q;
}

static std::vector<double> precondition(int precond, const Tuples &S, const Tuples &F, int n, const std::vector<double> &r)
{
	if (precond == SPSAMD_PRECOND_NONE) return r;
	std::vector<double> z(n);
	if (precond == SPSAMD_PRECOND_JACOBI) {
		std::vector<double> d(n, 0.0);
		for (size_t t = 0; t < S.v.size(); ++t) if (S.i[t] == S.j[t]) d[S.i[t]] = d[S.i[t]] + S.v[t];
		for (int i = 0; i < n; ++i) z[i] = r[i] / d[i];
		return z;
	}
	std::vector<size_t> beg(n + 1, 0);
	for (size_t t = 0; t < F.v.size(); ++t) ++beg[F.i[t] + 1];
	for (int i = 0; i < n; ++i) beg[i + 1] += beg[i];
	for (int i = 0; i < n; ++i) {                                    // LOWER | UNIT
		volatile double acc = r[i];
		for (size_t t = beg[i]; t < beg[i + 1]; ++t) if (F.j[t] < i) { volatile double p = F.v[t] * z[F.j[t]]; acc = acc - p; }
		z[i] = acc;
	}
	for (int i = n - 1; i >= 0; --i) {                               // UPPER | NONUNIT, in place
		volatile double acc = z[i], d = 0.0;
		for (size_t t = beg[i]; t < beg[i + 1]; ++t) {
			if (F.j[t] == i) d = d + F.v[t];
			else if (F.j[t] > i) { volatile double p = F.v[t] * z[F.j[t]]; acc = acc - p; }
		}
		z[i] = acc / d;
	}
	return z;
}

static bool usable(double v) { return std::isfinite(v) && v != 0.0; }

struct Outcome { std::vector<double> x, hist; uint64_t k, cycles; int reason; double bb, rr0, rr; };

static Outcome gmres_loop(const Tuples &S, int n, int precond, const Tuples &F, const std::vector<double> &b, std::vector<double> x,
	double tol, uint64_t max_iter, uint32_t m)
{
	Outcome o;
	volatile double tol2 = tol * tol;
	o.bb = dot(b, b);
	volatile double thresh = tol2 * o.bb;
	std::vector<double> r(n), q = apply(S, n, x);
	for (int e = 0; e < n; ++e) r[e] = b[e] - q[e];
	double rr = dot(r, r);
	o.rr0 = rr; o.k = 0; o.cycles = 0; o.hist.push_back(rr);
	for (;;) {
		if (rr <= thresh) { o.reason = SPSAMD_PCG_CONVERGED; break; }
		if (o.k == max_iter) { o.reason = SPSAMD_PCG_MAXITER; break; }
		if (!usable(rr)) { o.reason = SPSAMD_PCG_BREAKDOWN; break; }
		++o.cycles;
		volatile double beta = std::sqrt(rr);
		std::vector<std::vector<double>> V(1, std::vector<double>(n));
		for (int e = 0; e < n; ++e) V[0][e] = r[e] / beta;
		std::vector<double> g(m + 1, 0.0), c(m, 0.0), s(m, 0.0), h(m + 1, 0.0), d(m + 1, 0.0), R((size_t)m * m, 0.0);
		g[0] = beta;
		uint32_t j = 0;
		bool broken = false;
		for (;;) {
			std::vector<double> w = apply(S, n, precondition(precond, S, F, n, V[j]));
			for (uint32_t i = 0; i <= j; ++i) h[i] = dot(V[i], w);
			for (uint32_t i = 0; i <= j; ++i)
				for (int e = 0; e < n; ++e) { volatile double p = h[i] * V[i][e]; w[e] = w[e] - p; }
			for (uint32_t i = 0; i <= j; ++i) d[i] = dot(V[i], w);
			for (uint32_t i = 0; i <= j; ++i) {
				for (int e = 0; e < n; ++e) { volatile double p = d[i] * V[i][e]; w[e] = w[e] - p; }
				volatile double hs = h[i] + d[i];
				h[i] = hs;
			}
			const double ww = dot(w, w);
			volatile double hn = std::sqrt(ww);
			for (uint32_t i = 0; i < j; ++i) {
				volatile double a0 = c[i] * h[i], a1 = s[i] * h[i + 1], t = a0 + a1;
				volatile double b0 = c[i] * h[i + 1], b1 = s[i] * h[i], u = b0 - b1;
				h[i + 1] = u; h[i] = t;
			}
			volatile double hh = h[j] * h[j], nn = hn * hn, sum = hh + nn, den = std::sqrt(sum);
			if (!usable(den)) { broken = true; break; }
			volatile double cj = h[j] / den, sj = hn / den;
			c[j] = cj; s[j] = sj;
			for (uint32_t i = 0; i < j; ++i) R[(size_t)i * m + j] = h[i];
			R[(size_t)j * m + j] = den;
			volatile double sg = sj * g[j], cg = cj * g[j];
			g[j + 1] = -sg; g[j] = cg;
			++o.k; ++j;
			volatile double gg = g[j] * g[j];
			const double est = gg;
			o.hist.push_back(est);
			if (est <= thresh || j == m || o.k == max_iter || !usable(ww)) {
				if (!std::isfinite(ww)) broken = true;
				break;
			}
			V.push_back(std::vector<double>(n));
			for (int e = 0; e < n; ++e) V[j][e] = w[e] / hn;
		}
		if (j > 0) {
			std::vector<double> y(j);
			for (int i = (int)j - 1; i >= 0; --i) {
				volatile double a = g[i];
				for (uint32_t l = i + 1; l < j; ++l) { volatile double p = R[(size_t)i * m + l] * y[l]; a = a - p; }
				y[i] = a / R[(size_t)i * m + i];
			}
			std::vector<double> u(n, 0.0);
			for (uint32_t i = 0; i < j; ++i)
				for (int e = 0; e < n; ++e) { volatile double p = y[i] * V[i][e]; u[e] = u[e] + p; }
			const std::vector<double> z = precondition(precond, S, F, n, u);
			for (int e = 0; e < n; ++e) x[e] = x[e] + z[e];
			q = apply(S, n, x);
			for (int e = 0; e < n; ++e) r[e] = b[e] - q[e];
			rr = dot(r, r);
			o.hist[o.k] = rr;
		}
		if (broken) { o.reason = SPSAMD_PCG_BREAKDOWN; break; }
	}
	o.x = x; o.rr = rr;
	return o;
}

static void same(const char *what, const char *name, const double *got, const double *want, size_t n)
{
	for (size_t i = 0; i < n; ++i)
		if (bits_of(got[i]) != bits_of(want[i])) {
			std::printf("FAIL %s: %s[%zu] %.17g (%016llx) vs %.17g (%016llx)\n", what, name, i, got[i], (unsigned long long)bits_of(got[i]),
				want[i], (unsigned long long)bits_of(want[i]));
			++failures;
			return;
		}
}

static void run(spsamd_ctx *ctx, const char *what, const Tuples &S, int n, int precond, const Tuples &F, const std::vector<double> &b,
	const std::vector<double> &x0, double tol, uint64_t max_iter, uint32_t restart)
{
	const Outcome w = gmres_loop(S, n, precond, F, b, x0, tol, max_iter, restart);
	const spsamd_coo A = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), (size_t)n, (size_t)n, 0, SPSAMD_MEM_HOST};
	const spsamd_coo M = {F.i.data(), F.j.data(), F.v.data(), F.v.size(), (size_t)n, (size_t)n, 0, SPSAMD_MEM_HOST};
	std::vector<double> x = x0, hist(max_iter + 1, -7.5);
	spsamd_pcg_stats st;
	spsamd_result res;
	const int rc = spsamd_solve_gmres(ctx, &A, '.', precond, precond == SPSAMD_PRECOND_LU ? &M : nullptr, '.', b.data(), x.data(),
		SPSAMD_MEM_HOST, tol, max_iter, restart, hist.data(), hist.size(), SPSAMD_ADD, 0, &st, &res);
	if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; return; }
	if (st.iterations != w.k || st.reason != w.reason || st.readbacks != w.cycles + 1) {
		std::printf("FAIL %s: stopped at %llu for %d after %llu cycles, want %llu for %d after %llu\n", what, (unsigned long long)st.iterations,
			st.reason, (unsigned long long)st.readbacks - 1, (unsigned long long)w.k, w.reason, (unsigned long long)w.cycles);
		++failures;
		return;
	}
	same(what, "x", x.data(), w.x.data(), n);
	same(what, "hist", hist.data(), w.hist.data(), w.hist.size());
	const double got3[3] = {st.bb, st.rr0, st.rr}, want3[3] = {w.bb, w.rr0, w.rr};
	same(what, "bb, rr0, rr", got3, want3, 3);
	if (res.shape0 != (uint64_t)n || res.nnz_a != S.v.size()) { std::printf("FAIL result of %s\n", what); ++failures; }
	std::printf("%s: %llu steps, %llu cycles, reason %d\n", what, (unsigned long long)st.iterations, (unsigned long long)w.cycles, st.reason);
}

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "--abi-only")) { std::printf("OK\n"); return 0; }
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	{
		const int n = 2500;
		Tuples S, F;
		std::vector<double> u(n), b(n), x0(n, 0.0);
		uint64_t s = 12345;
		const double cv = 1.5;                                       // upwind: the sub-diagonal carries the convection
		for (int i = 0; i < n; ++i) {
			if (i) { S.i.push_back(i); S.j.push_back(i - 1); S.v.push_back(-1.0 - cv); }
			S.i.push_back(i); S.j.push_back(i); S.v.push_back(2.0 + cv + 0.001 * (i % 7));
			if (i + 1 < n) { S.i.push_back(i); S.j.push_back(i + 1); S.v.push_back(-1.0); }
			s = s * 6364136223846793005ull + 1442695040888963407ull;
			b[i] = std::ldexp((double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.25, (int)((s >> 3) % 40) - 20);
		}
		for (int i = 0; i < n; ++i) {                                // the LU of the stencil without the 0.001 (i % 7): close to S, not its factor
			const double d = 2.0 + cv;
			if (i) { const double l = (-1.0 - cv) / u[i - 1]; F.i.push_back(i); F.j.push_back(i - 1); F.v.push_back(l); u[i] = d - l * -1.0; }
			else u[i] = d;
			F.i.push_back(i); F.j.push_back(i); F.v.push_back(u[i]);
			if (i + 1 < n) { F.i.push_back(i); F.j.push_back(i + 1); F.v.push_back(-1.0); }
		}
		run(ctx, "convdiff1d, none", S, n, SPSAMD_PRECOND_NONE, F, b, x0, 1e-6, 30, 7);
		run(ctx, "convdiff1d, jacobi", S, n, SPSAMD_PRECOND_JACOBI, F, b, x0, 1e-6, 30, 7);
		run(ctx, "convdiff1d, lu", S, n, SPSAMD_PRECOND_LU, F, b, x0, 1e-6, 30, 7);
		for (int i = 0; i < n; ++i) x0[i] = 0.001 * (i % 11) - 0.004;
		run(ctx, "convdiff1d, jacobi, x0", S, n, SPSAMD_PRECOND_JACOBI, F, b, x0, 0.0, 10, 7);
	}
	{
		const int n = 6;
		Tuples S, F;
		for (int i = 0; i < n; ++i)
			for (int j = 0; j < n; ++j)
				if (i == j || (i + j) % 3 == 0) { S.i.push_back(i); S.j.push_back(j); S.v.push_back(i == j ? 4.0 + 0.25 * i : 1.0 / (2 + i + j)); }
		F = S;
		std::vector<double> b = {1.0, -2.0, 0.5, 3.0, -0.75, 0.125}, x0(n, 0.0);
		for (int pc = 0; pc < 3; ++pc) run(ctx, "6 x 6", S, n, pc, F, b, x0, 1e-12, 20, 7);
		S.v[3] = with_bits(0x7FF80000DEADBEEFull);
		for (int pc = 0; pc < 3; ++pc) run(ctx, "6 x 6 with a NaN", S, n, pc, F, b, x0, 1e-12, 20, 7);
		// the refusals: x untouched
		const spsamd_coo A = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), (size_t)n, (size_t)n, 0, SPSAMD_MEM_HOST};
		const spsamd_coo R = {S.i.data(), S.j.data(), S.v.data(), S.v.size(), 6, 7, 0, SPSAMD_MEM_HOST};
		std::vector<double> x(n, -7.5);
		int rc = spsamd_solve_gmres(ctx, &A, '.', 0, nullptr, '.', b.data(), x.data(), SPSAMD_MEM_HOST, -1.0, 5, 7, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL negative tol: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_gmres(ctx, &A, '.', SPSAMD_PRECOND_LU, nullptr, '.', b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, 7, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL LU without M: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_gmres(ctx, &R, '.', 0, nullptr, '.', b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, 7, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL not square: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_gmres(ctx, &A, '.', 0, nullptr, '.', b.data(), b.data(), SPSAMD_MEM_HOST, 1e-8, 5, 7, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL x == b: rc %d\n", rc); ++failures; }
		for (uint32_t bad : {0u, (uint32_t)SPSAMD_GMRES_MAX_RESTART + 1}) {
			rc = spsamd_solve_gmres(ctx, &A, '.', 0, nullptr, '.', b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, bad, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
			if (rc != SPSAMD_EINVAL) { std::printf("FAIL restart %u: rc %d\n", bad, rc); ++failures; }
		}
		for (int k = 0; k < n; ++k) if (x[k] != -7.5) { std::printf("FAIL an error wrote x\n"); ++failures; break; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
