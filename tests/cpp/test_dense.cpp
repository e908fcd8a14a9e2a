// spsparse_amd::multiply_dense (multiply_dense.hpp:11-35 restated over the C ABI) on a small case: duplicates, an
// explicit zero times Inf, both transposes, the three policies and handle_nan.  Prints OK on success.
#include <spsparse_amd/multiply.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

using Mat = spsparse_amd::VectorCooMatrix<int, double>;
using spsparse_amd::DuplicatePolicy;

static int failures = 0;

static void expect(const char *what, const double *got, const double *want, int n)
{
	for (int k = 0; k < n; ++k)
		if (std::memcmp(&got[k], &want[k], sizeof(double)) != 0) {
			std::printf("FAIL %s [%d]: %.17g vs %.17g\n", what, k, got[k], want[k]);
			++failures;
		}
}

int main()
{
	Mat M({3, 4});
	M.add({2, 1}, 2.0);
	M.add({0, 3}, -1.0);
	M.add({2, 1}, 0.5);            // duplicate of the first tuple
	M.add({0, 0}, 4.0);
	M.add({1, 2}, 0.0);            // explicit zero: 0 * Inf = NaN
	const double x[4] = {1.0, 10.0, INFINITY, 100.0};

	double y[3] = {1.0, 2.0, 3.0};
	spsparse_amd::multiply_dense(M, x, y);
	const double add[3] = {1.0 - 100.0 + 4.0, NAN, 3.0 + 20.0 + 5.0};
	expect("ADD", y, add, 1); expect("ADD", y + 2, add + 2, 1);
	if (!std::isnan(y[1])) { std::printf("FAIL ADD [1]: %g is not NaN\n", y[1]); ++failures; }

	double y2[3] = {1.0, 2.0, 3.0};
	spsparse_amd::multiply_dense(M, x, y2, true);               // handle_nan: the NaN product is skipped
	const double hn[3] = {-95.0, 2.0, 28.0};
	expect("handle_nan", y2, hn, 3);

	double y3[3] = {NAN, 2.0, 3.0};
	spsparse_amd::multiply_dense(M, x, y3, true, false, DuplicatePolicy::REPLACE);
	const double rep[3] = {4.0, 2.0, 5.0};
	expect("REPLACE", y3, rep, 3);

	double y4[3] = {NAN, 2.0, 3.0};
	spsparse_amd::multiply_dense(M, x, y4, true, false, DuplicatePolicy::LEAVE_ALONE);
	if (!std::isnan(y4[0]) || y4[1] != 2.0 || y4[2] != 5.0) { std::printf("FAIL LEAVE_ALONE\n"); ++failures; }

	// transpose: y (4 entries) (op)= M^T x (3 entries)
	const double xt[3] = {1.0, 2.0, 3.0};
	double yt[4] = {0.0, 0.0, 0.0, 0.0};
	spsparse_amd::multiply_dense(M, xt, yt, false, true);
	const double tr[4] = {4.0, 2.0 * 3.0 + 0.5 * 3.0, 0.0, -1.0};
	expect("transpose", yt, tr, 4);

	// an index out of bounds reaches the error hook
	Mat bad({2, 2});
	bad.add({1, 0}, 1.0);
	bad.index(0, 0) = 5;
	bool raised = false;
	try { spsparse_amd::multiply_dense(bad, xt, yt); } catch (const spsparse_amd::Exception &) { raised = true; }
	if (!raised) { std::printf("FAIL out of bounds did not raise\n"); ++failures; }

	if (failures) return 1;
	std::printf("OK\n");
	return 0;
}
