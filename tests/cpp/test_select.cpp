// spsparse_amd::select (the C++ mirror of spsamd_select) on a hand-written 6 x 6 matrix, once per predicate: the kept tuples
// arrive in row-major order with their values untouched (a NaN payload and a -0.0 included).  Prints OK on success.
#include <spsparse_amd/multiply.hpp>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using Mat = spsparse_amd::VectorCooMatrix<int, double>;

static int failures = 0;

static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

struct Tup { int i, j; double v; };

static void expect(const char *what, Mat const &got, std::vector<Tup> const &want)
{
	if (got.size() != want.size()) { std::printf("FAIL %s: %zu tuples, want %zu\n", what, got.size(), want.size()); ++failures; return; }
	for (size_t k = 0; k < want.size(); ++k)
		if (got.index(0, k) != want[k].i || got.index(1, k) != want[k].j || std::memcmp(&got.val(k), &want[k].v, 8) != 0) {
			std::printf("FAIL %s [%zu]: (%d, %d, %.17g) vs (%d, %d, %.17g)\n", what, k, got.index(0, k), got.index(1, k), got.val(k),
				want[k].i, want[k].j, want[k].v);
			++failures;
		}
}

int main()
{
	const double nan = with_bits(0x7FF80000DEADBEEFull);
	// row 0: (0,0) 4   (0,3) -1   (0,5) 0.5
	// row 1: (1,1) -2  (1,2) 2
	// row 2: (2,0) nan (2,2) 8    (2,4) -8
	// row 4: (4,3) 1e-3
	// row 5: (5,0) 3   (5,5) -6
	Mat A({6, 6});
	A.add({5, 5}, -6.0); A.add({0, 3}, -1.0); A.add({2, 0}, nan); A.add({1, 2}, 2.0); A.add({0, 0}, 4.0); A.add({2, 4}, -8.0);
	A.add({4, 3}, 1e-3); A.add({1, 1}, -2.0); A.add({5, 0}, 3.0); A.add({2, 2}, 8.0); A.add({0, 5}, 0.5);

	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_TRIL, -1);
	  expect("TRIL(-1)", R, {{2, 0, nan}, {4, 3, 1e-3}, {5, 0, 3.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_TRIU, 1);
	  expect("TRIU(1)", R, {{0, 3, -1.0}, {0, 5, 0.5}, {1, 2, 2.0}, {2, 4, -8.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_DIAG, 0);
	  expect("DIAG(0)", R, {{0, 0, 4.0}, {1, 1, -2.0}, {2, 2, 8.0}, {5, 5, -6.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_OFFDIAG, 0);
	  expect("OFFDIAG(0)", R, {{0, 3, -1.0}, {0, 5, 0.5}, {1, 2, 2.0}, {2, 0, nan}, {2, 4, -8.0}, {4, 3, 1e-3}, {5, 0, 3.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_ABS_GE, 0, 3.0);
	  expect("ABS_GE(3)", R, {{0, 0, 4.0}, {2, 0, nan}, {2, 2, 8.0}, {2, 4, -8.0}, {5, 0, 3.0}, {5, 5, -6.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_ROW_REL, 0, 0.25);
	  expect("ROW_REL(0.25)", R, {{0, 0, 4.0}, {0, 3, -1.0}, {1, 1, -2.0}, {1, 2, 2.0}, {2, 0, nan}, {2, 2, 8.0}, {2, 4, -8.0}, {4, 3, 1e-3}, {5, 0, 3.0}, {5, 5, -6.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_ROW_TOPK, 1);          // the NaN is its row's largest; ties go to the lower column
	  expect("ROW_TOPK(1)", R, {{0, 0, 4.0}, {1, 1, -2.0}, {2, 0, nan}, {4, 3, 1e-3}, {5, 5, -6.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, '.', SPSAMD_SELECT_ROW_TOPK, 2, 0.0, SPSAMD_SELECT_COMPLEMENT);
	  expect("ROW_TOPK(2) complement", R, {{0, 5, 0.5}, {2, 4, -8.0}}); }
	{ Mat R({1, 1}); spsparse_amd::select(R, A, 'T', SPSAMD_SELECT_ROW_TOPK, 1);          // the largest of every column, as rows of A^T
	  expect("ROW_TOPK(1) of A^T", R, {{0, 2, nan}, {1, 1, -2.0}, {2, 2, 8.0}, {3, 0, -1.0}, {4, 2, -8.0}, {5, 5, -6.0}});
	  if (R.shape[0] != 6 || R.shape[1] != 6) { std::printf("FAIL shape\n"); ++failures; } }

	// a -0.0 in an operand that carries its sort order stays, bit for bit
	Mat Z({2, 2});
	Z.add({0, 0}, -0.0); Z.add({1, 0}, 1.0);
	Z.set_sorted(spsparse_amd::ROW_MAJOR);
	{ Mat R({1, 1}); spsparse_amd::select(R, Z, '.', SPSAMD_SELECT_ABS_GE, 0, 0.0);
	  expect("-0.0 kept", R, {{0, 0, -0.0}, {1, 0, 1.0}}); }

	// a bad predicate reaches the error hook
	bool raised = false;
	try { Mat R({1, 1}); spsparse_amd::select(R, A, '.', 99); } catch (const spsparse_amd::Exception &) { raised = true; }
	if (!raised) { std::printf("FAIL bad predicate did not raise\n"); ++failures; }

	if (failures) return 1;
	std::printf("OK\n");
	return 0;
}
