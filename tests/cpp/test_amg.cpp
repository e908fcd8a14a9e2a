// spsamd_amg_apply and spsamd_solve_pcg_amg through the plain C ABI against the loops of the header written out in C++ and
// compiled by g++ with -ffp-contract=off.  A 1-D Laplacian of order 2500 with integer entries, pairwise aggregates, three
// levels (2500 / 1250 / 625; the Galerkin sums are exact), the tentative prolongator passed as P with '.' and as R with 'T';
// V(1,1) and V(2,1) with 3 coarse sweeps and omega = 2/3; then the refusals.  Prints OK on success.
#include <spsparse_amd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

static int failures = 0;

static uint64_t bits_of(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

struct Tuples { std::vector<int32_t> i, j; std::vector<double> v; };
struct Level { int n; Tuples S, P, R; std::vector<double> d; };

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

// X row-major: the rows ascend
static std::vector<double> apply(const Tuples &X, int nrow, const std::vector<double> &v)
{
	std::vector<double> q(nrow, 0.0);
	for (size_t t = 0; t < X.v.size(); ++t) { volatile double pr = X.v[t] * v[X.j[t]]; q[X.i[t]] = q[X.i[t]] + pr; }
	return q;
}

static std::vector<double> smooth(const Level &L, const std::vector<double> &b, const std::vector<double> &x, double omega, bool first)
{
	std::vector<double> out(L.n);
	if (first) {
		for (int i = 0; i < L.n; ++i) { volatile double t = b[i] / L.d[i]; out[i] = omega * t; }
		return out;
	}
	const std::vector<double> q = apply(L.S, L.n, x);
	for (int i = 0; i < L.n; ++i) {
		volatile double r = b[i] - q[i];
		volatile double t = r / L.d[i];
		volatile double u = omega * t;
		out[i] = x[i] + u;
	}
	return out;
}

static std::vector<double> cycle(const std::vector<Level> &lv, const spsamd_amg_params &p, size_t l, const std::vector<double> &b)
{
	const Level &L = lv[l];
	std::vector<double> x(L.n, 0.0);
	const bool last = l + 1 == lv.size();
	for (uint32_t s = 0; s < (last ? p.coarse : p.pre); ++s) x = smooth(L, b, x, p.omega, s == 0);
	if (last) return x;
	std::vector<double> r = b;
	if (p.pre) {
		const std::vector<double> q = apply(L.S, L.n, x);
		for (int i = 0; i < L.n; ++i) r[i] = b[i] - q[i];
	}
	const std::vector<double> e = cycle(lv, p, l + 1, apply(L.R, lv[l + 1].n, r)), c = apply(L.P, L.n, e);
	for (int i = 0; i < L.n; ++i) x[i] = x[i] + c[i];
	for (uint32_t s = 0; s < p.post; ++s) x = smooth(L, b, x, p.omega, false);
	return x;
}

static bool usable(double v) { return std::isfinite(v) && v != 0.0; }

struct Outcome { std::vector<double> x, hist; uint64_t k; int reason; double bb, rr0, rr; };

static Outcome pcg_loop(const std::vector<Level> &lv, const spsamd_amg_params &prm, const std::vector<double> &b, std::vector<double> x,
	double tol, uint64_t max_iter)
{
	const Tuples &S = lv[0].S;
	const int n = lv[0].n;
	Outcome o;
	volatile double tol2 = tol * tol;
	o.bb = dot(b, b);
	volatile double thresh = tol2 * o.bb;
	std::vector<double> r(n), p(n), q = apply(S, n, x);
	for (int i = 0; i < n; ++i) r[i] = b[i] - q[i];
	double rr = dot(r, r), rz = 0.0;
	o.rr0 = rr; o.k = 0; o.hist.push_back(rr);
	for (;;) {
		if (rr <= thresh) { o.reason = SPSAMD_PCG_CONVERGED; break; }
		if (o.k == max_iter) { o.reason = SPSAMD_PCG_MAXITER; break; }
		const std::vector<double> z = cycle(lv, prm, 0, r);
		const double rz1 = dot(r, z);
		if (o.k == 0) p = z;
		else {
			volatile double beta = rz1 / rz;
			for (int i = 0; i < n; ++i) { volatile double t = beta * p[i]; p[i] = z[i] + t; }
		}
		rz = rz1;
		if (!usable(rz)) { o.reason = SPSAMD_PCG_BREAKDOWN; break; }
		q = apply(S, n, p);
		const double pq = dot(p, q);
		if (!usable(pq)) { o.reason = SPSAMD_PCG_BREAKDOWN; break; }
		volatile double alpha = rz / pq;
		for (int i = 0; i < n; ++i) {
			volatile double t = alpha * p[i]; x[i] = x[i] + t;
			volatile double u = alpha * q[i]; r[i] = r[i] - u;
		}
		rr = dot(r, r); ++o.k; o.hist.push_back(rr);
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

static spsamd_coo host(const Tuples &X, size_t s0, size_t s1) { return spsamd_coo{X.i.data(), X.j.data(), X.v.data(), X.v.size(), s0, s1, 0, SPSAMD_MEM_HOST}; }

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "--abi-only")) {
		spsamd_amg_stats st;
		spsamd_amg_level lv = {nullptr, '.', nullptr, '.', nullptr, '.'};
		spsamd_amg_params p = {1, 1, 4, 2.0 / 3.0};
		int (*f)(spsamd_ctx *, const spsamd_amg_level *, size_t, const spsamd_amg_params *, const double *, double *, int, int, int,
			spsamd_amg_stats *, spsamd_result *) = spsamd_amg_apply;
		(void)st; (void)lv; (void)p; (void)f;
		static_assert(sizeof(st.rows) == 32 * 8 && sizeof(st.nnz) == 32 * 8, "32 levels");
		// no context: both calls refuse without touching anything
		if (spsamd_amg_apply(nullptr, &lv, 1, &p, nullptr, nullptr, SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr) != SPSAMD_EINVAL) return 1;
		if (spsamd_solve_pcg_amg(nullptr, &lv, 1, &p, nullptr, nullptr, SPSAMD_MEM_HOST, 1e-8, 1, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr, nullptr) != SPSAMD_EINVAL) return 1;
		std::printf("OK\n");
		return 0;
	}
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }

	// ---- the hierarchy: pairwise aggregates, P^T S P summed exactly (integers)
	std::vector<Level> lv(3);
	{
		int n = 2500;
		Tuples S;
		for (int i = 0; i < n; ++i) {
			if (i) { S.i.push_back(i); S.j.push_back(i - 1); S.v.push_back(-1.0); }
			S.i.push_back(i); S.j.push_back(i); S.v.push_back(2.0 + (i % 3));
			if (i + 1 < n) { S.i.push_back(i); S.j.push_back(i + 1); S.v.push_back(-1.0); }
		}
		for (size_t l = 0; l < lv.size(); ++l) {
			Level &L = lv[l];
			L.n = n; L.S = S;
			L.d.assign(n, 0.0);
			for (size_t t = 0; t < S.v.size(); ++t) if (S.i[t] == S.j[t]) L.d[S.i[t]] = L.d[S.i[t]] + S.v[t];
			if (l + 1 == lv.size()) break;
			const int nc = (n + 1) / 2;
			for (int i = 0; i < n; ++i) { L.P.i.push_back(i); L.P.j.push_back(i / 2); L.P.v.push_back(1.0); }
			for (int i = 0; i < n; ++i) { L.R.i.push_back(i / 2); L.R.j.push_back(i); L.R.v.push_back(1.0); }   // P^T, row-major
			std::map<std::pair<int, int>, double> acc;
			for (size_t t = 0; t < S.v.size(); ++t) acc[{S.i[t] / 2, S.j[t] / 2}] += S.v[t];
			Tuples C;
			for (const auto &kv : acc) if (kv.second != 0.0) { C.i.push_back(kv.first.first); C.j.push_back(kv.first.second); C.v.push_back(kv.second); }
			S = C; n = nc;
		}
	}
	std::vector<spsamd_coo> A(3), P(2);
	std::vector<spsamd_amg_level> lev(3);
	for (size_t l = 0; l < 3; ++l) {
		A[l] = host(lv[l].S, lv[l].n, lv[l].n);
		if (l < 2) P[l] = host(lv[l].P, lv[l].n, lv[l + 1].n);
		lev[l] = spsamd_amg_level{&A[l], '.', l < 2 ? &P[l] : nullptr, '.', l < 2 ? &P[l] : nullptr, l < 2 ? 'T' : '.'};
	}
	const int n = lv[0].n;
	std::vector<double> b(n), x0(n, 0.0);
	uint64_t s = 12345;
	for (int i = 0; i < n; ++i) {
		s = s * 6364136223846793005ull + 1442695040888963407ull;
		b[i] = std::ldexp((double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.25, (int)((s >> 3) % 40) - 20);
	}

	const spsamd_amg_params params[2] = {{1, 1, 3, 2.0 / 3.0}, {2, 1, 3, 2.0 / 3.0}};
	for (int k = 0; k < 2; ++k) {
		const spsamd_amg_params &prm = params[k];
		char what[64];
		std::snprintf(what, sizeof what, "laplace1d V(%u,%u)", prm.pre, prm.post);
		// one cycle
		{
			const std::vector<double> w = cycle(lv, prm, 0, b);
			std::vector<double> x(n, -7.5);
			spsamd_amg_stats ast;
			spsamd_result res;
			const int rc = spsamd_amg_apply(ctx, lev.data(), 3, &prm, b.data(), x.data(), SPSAMD_MEM_HOST, SPSAMD_ADD, 0, &ast, &res);
			if (rc != SPSAMD_OK) { std::printf("FAIL %s: amg_apply rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; continue; }
			same(what, "cycle", x.data(), w.data(), n);
			if (ast.levels != 3 || ast.rows[0] != 2500 || ast.rows[1] != 1250 || ast.rows[2] != 625 || ast.nnz[0] != lv[0].S.v.size() ||
				ast.fused_levels != 1 || ast.launches_per_cycle == 0 || res.shape0 != (uint64_t)n || res.nnz_a != lv[0].S.v.size()) {
				std::printf("FAIL %s: stats\n", what); ++failures;
			}
		}
		// the loop
		const Outcome w = pcg_loop(lv, prm, b, x0, 1e-6, 30);
		std::vector<double> x = x0, hist(31, -7.5);
		spsamd_pcg_stats st;
		spsamd_amg_stats ast;
		spsamd_result res;
		const int rc = spsamd_solve_pcg_amg(ctx, lev.data(), 3, &prm, b.data(), x.data(), SPSAMD_MEM_HOST, 1e-6, 30, hist.data(), hist.size(),
			SPSAMD_ADD, 0, &st, &ast, &res);
		if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; continue; }
		if (st.iterations != w.k || st.reason != w.reason) {
			std::printf("FAIL %s: stopped at %llu for %d, want %llu for %d\n", what, (unsigned long long)st.iterations, st.reason, (unsigned long long)w.k, w.reason);
			++failures;
			continue;
		}
		same(what, "x", x.data(), w.x.data(), n);
		same(what, "hist", hist.data(), w.hist.data(), w.hist.size());
		const double got3[3] = {st.bb, st.rr0, st.rr}, want3[3] = {w.bb, w.rr0, w.rr};
		same(what, "bb, rr0, rr", got3, want3, 3);
		if (ast.levels != 3 || res.shape0 != (uint64_t)n || res.nnz_a != lv[0].S.v.size()) { std::printf("FAIL result of %s\n", what); ++failures; }
		std::printf("%s: %llu iterations, reason %d\n", what, (unsigned long long)st.iterations, st.reason);
	}

	// ---- the refusals: x untouched
	{
		std::vector<double> x(n, -7.5);
		const spsamd_amg_params prm = params[0];
		spsamd_amg_params bad = prm;
		bad.omega = std::nan("");
		int rc = spsamd_amg_apply(ctx, lev.data(), 3, &bad, b.data(), x.data(), SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL omega NaN: rc %d\n", rc); ++failures; }
		rc = spsamd_amg_apply(ctx, lev.data(), 0, &prm, b.data(), x.data(), SPSAMD_MEM_HOST, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL nlevels 0: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_pcg_amg(ctx, lev.data(), 2, &prm, b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL P on the last level: rc %d\n", rc); ++failures; }
		std::vector<spsamd_amg_level> skip = {lev[0], lev[2]};
		rc = spsamd_solve_pcg_amg(ctx, skip.data(), 2, &prm, b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr, nullptr);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL shapes that do not chain: rc %d\n", rc); ++failures; }
		rc = spsamd_solve_pcg(ctx, &A[0], '.', 3, nullptr, '.', b.data(), x.data(), SPSAMD_MEM_HOST, 1e-8, 5, nullptr, 0, SPSAMD_ADD, 0, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL solve_pcg took precond 3: rc %d\n", rc); ++failures; }
		for (int k = 0; k < n; ++k) if (x[k] != -7.5) { std::printf("FAIL an error wrote x\n"); ++failures; break; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
