// spsparse_amd::multiply_sampled (the sampled dense-dense product over the C ABI) on a small case: duplicates, an explicit
// zero, a NaN payload, 0 * Inf, both transposes, alpha and beta, an in-place update of M's values and an index out of
// bounds.  Prints OK on success.
#include <spsparse_amd/multiply.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

using Mat = spsparse_amd::VectorCooMatrix<int, double>;

static int failures = 0;

static void expect(const char *what, const double *got, const double *want, int n)
{
	for (int k = 0; k < n; ++k)
		if (std::memcmp(&got[k], &want[k], sizeof(double)) != 0) {
			std::printf("FAIL %s [%d]: %.17g vs %.17g\n", what, k, got[k], want[k]);
			++failures;
		}
}

static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

int main()
{
	Mat M({3, 4});
	M.add({2, 1}, 2.0);
	M.add({0, 3}, -1.0);
	M.add({2, 1}, 0.5);            // duplicate of the first tuple: its own output
	M.add({1, 2}, 0.0);            // explicit zero
	// P: 3 rows of k = 2 (ldp 3), Q: 4 rows of k = 2 (ldq 2)
	const double P[9] = {1.0, 2.0, -7.0, 3.0, 4.0, -7.0, 5.0, 6.0, -7.0};
	const double Q[8] = {1.0, 1.0, 10.0, 100.0, INFINITY, 0.0, 0.5, 0.25};
	double out[4];
	spsparse_amd::multiply_sampled(M, P, 3, Q, 2, 2, out);
	// (2,1): 5*10 + 6*100; (0,3): 1*0.5 + 2*0.25; (1,2): 3*Inf + 4*0 = Inf
	const double plain[4] = {650.0, 1.0, 650.0, INFINITY};
	expect("plain", out, plain, 4);

	spsparse_amd::multiply_sampled(M, P, 3, Q, 2, 2, out, 2.0, -1.0);
	const double scaled[4] = {1298.0, 3.0, 1299.5, INFINITY};
	expect("alpha/beta", out, scaled, 4);

	// a NaN payload in P (left operand of the first product) survives
	double Pn[9];
	std::memcpy(Pn, P, sizeof P);
	Pn[6] = with_bits(0x7FF8000000000123ull);
	spsparse_amd::multiply_sampled(M, Pn, 3, Q, 2, 2, out);
	const double nanrow[4] = {with_bits(0x7FF8000000000123ull), 1.0, with_bits(0x7FF8000000000123ull), INFINITY};
	expect("NaN payload", out, nanrow, 4);

	// 0 * Inf: the x86 default NaN
	double Pz[9];
	std::memcpy(Pz, P, sizeof P);
	Pz[3] = 0.0;
	spsparse_amd::multiply_sampled(M, Pz, 3, Q, 2, 2, out);
	const double dflt = with_bits(0xFFF8000000000000ull);
	expect("0 * Inf", out + 3, &dflt, 1);

	// transpose: P has cols(M) = 4 rows, Q rows(M) = 3 rows (k = 1)
	const double Pt[4] = {1.0, 2.0, 3.0, 4.0}, Qt[3] = {10.0, 20.0, 30.0};
	spsparse_amd::multiply_sampled(M, Pt, 1, Qt, 1, 1, out, 1.0, 0.0, true);
	const double tr[4] = {60.0, 40.0, 60.0, 60.0};
	expect("transpose", out, tr, 4);

	// in place: M's values become alpha * d + beta * v
	spsparse_amd::multiply_sampled(M, Pt, 1, Qt, 1, 1, &M.val(0), -1.0, 1.0, true);
	const double inplace[4] = {-58.0, -41.0, -59.5, -60.0};
	expect("in place", &M.val(0), inplace, 4);

	// an index out of bounds reaches the error hook
	Mat bad({2, 2});
	bad.add({1, 0}, 1.0);
	bad.index(0, 0) = 5;
	bool raised = false;
	try { spsparse_amd::multiply_sampled(bad, P, 3, Q, 2, 2, out); } catch (const spsparse_amd::Exception &) { raised = true; }
	if (!raised) { std::printf("FAIL out of bounds did not raise\n"); ++failures; }

	if (failures) return 1;
	std::printf("OK\n");
	return 0;
}
