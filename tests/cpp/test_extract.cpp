// spsparse_amd::extract (the C++ mirror of spsamd_extract) on a hand-written 5 x 5 matrix -- unordered and repeated lists,
// ALL on either side, the transpose, an empty list -- and a permutation round trip: extract(extract(A, p, p), q, q) with
// q the inverse of p is consolidate(A).  Values arrive bit for bit (a NaN payload and a -0.0 included).  Prints OK on success.
#include <spsparse_amd/multiply.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using Mat = spsparse_amd::VectorCooMatrix<int, double>;

static int failures = 0;

static double with_bits(uint64_t b) { double x; std::memcpy(&x, &b, 8); return x; }

struct Tup { int i, j; double v; };

static void expect(const char *what, Mat const &got, std::vector<Tup> const &want, size_t s0, size_t s1)
{
	if (got.shape[0] != s0 || got.shape[1] != s1) { std::printf("FAIL %s: shape %zu x %zu, want %zu x %zu\n", what, (size_t)got.shape[0], (size_t)got.shape[1], s0, s1); ++failures; }
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
	//        c0    c1    c2    c3    c4
	// r0     4     .     .     -1    .
	// r1     .     -2    2     .     .
	// r2     nan   .     8     .     -8
	// r3     .     .     .     .     .
	// r4     3     .     .     1e-3  -6
	Mat A({5, 5});
	A.add({4, 4}, -6.0); A.add({0, 3}, -1.0); A.add({2, 0}, nan); A.add({1, 2}, 2.0); A.add({0, 0}, 4.0); A.add({2, 4}, -8.0);
	A.add({4, 3}, 1e-3); A.add({1, 1}, -2.0); A.add({4, 0}, 3.0); A.add({2, 2}, 8.0);

	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', std::vector<int>{2, 0}, std::vector<int>{0, 2, 4});
	  expect("A([2 0], [0 2 4])", R, {{0, 0, nan}, {0, 1, 8.0}, {0, 2, -8.0}, {1, 0, 4.0}}, 2, 3); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', std::vector<int>{4, 4, 3}, std::vector<int>{3, 0, 0});      // repeats, an empty row
	  expect("A([4 4 3], [3 0 0])", R, {{0, 0, 1e-3}, {0, 1, 3.0}, {0, 2, 3.0}, {1, 0, 1e-3}, {1, 1, 3.0}, {1, 2, 3.0}}, 3, 3); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', spsparse_amd::all, std::vector<int>{4, 1});
	  expect("A(:, [4 1])", R, {{1, 1, -2.0}, {2, 0, -8.0}, {4, 0, -6.0}}, 5, 2); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', std::vector<int>{1, 2}, spsparse_amd::all);
	  expect("A([1 2], :)", R, {{0, 1, -2.0}, {0, 2, 2.0}, {1, 0, nan}, {1, 2, 8.0}, {1, 4, -8.0}}, 2, 5); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, 'T', std::vector<int>{0, 3}, std::vector<int>{4, 2, 0});         // rows of A^T are columns of A
	  expect("A^T([0 3], [4 2 0])", R, {{0, 0, 3.0}, {0, 1, nan}, {0, 2, 4.0}, {1, 0, 1e-3}, {1, 2, -1.0}}, 2, 3); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', std::vector<int>{}, spsparse_amd::all);
	  expect("A([], :)", R, {}, 0, 5); }
	{ Mat R({1, 1}); spsparse_amd::extract(R, A, '.', spsparse_amd::all, spsparse_amd::all);
	  expect("A(:, :)", R, {{0, 0, 4.0}, {0, 3, -1.0}, {1, 1, -2.0}, {1, 2, 2.0}, {2, 0, nan}, {2, 2, 8.0}, {2, 4, -8.0}, {4, 0, 3.0}, {4, 3, 1e-3}, {4, 4, -6.0}}, 5, 5); }

	// a -0.0 and duplicate keys in an operand that carries its sort order stay, in storage order
	Mat Z({2, 2});
	Z.add({0, 1}, -0.0); Z.add({0, 0}, 1.0); Z.add({0, 1}, 2.0); Z.add({1, 0}, 5.0);
	Z.set_sorted(spsparse_amd::ROW_MAJOR);
	{ Mat R({1, 1}); spsparse_amd::extract(R, Z, '.', std::vector<int>{0}, std::vector<int>{1, 0});
	  expect("trusted duplicates", R, {{0, 0, -0.0}, {0, 0, 2.0}, {0, 1, 1.0}}, 1, 2); }

	// permutation round trip on a 200 x 200 matrix with duplicate keys (consolidated by ADD on the way in)
	{
		const int n = 200;
		Mat B({(size_t)n, (size_t)n});
		uint64_t s = 12345;
		auto next = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); };
		for (int k = 0; k < 3000; ++k) { const int i = (int)(next() % n), j = (int)(next() % n); B.add({i, j}, 0.25 + (double)(next() % 1000)); }
		std::vector<int> p(n), q(n);
		for (int k = 0; k < n; ++k) p[k] = k;
		for (int k = n - 1; k > 0; --k) { const int j = (int)(next() % (uint32_t)(k + 1)); std::swap(p[k], p[j]); }
		for (int k = 0; k < n; ++k) q[p[k]] = k;
		Mat P({1, 1}), Back({1, 1}), C({1, 1});
		spsparse_amd::extract(P, B, '.', p, p);
		spsparse_amd::extract(Back, P, '.', q, q);
		spsparse_amd::extract(C, B, '.', spsparse_amd::all, spsparse_amd::all);    // consolidate(B), through the same intake
		Mat D(B);
		D.consolidate(spsparse_amd::ROW_MAJOR);
		std::vector<Tup> want;
		for (size_t k = 0; k < D.size(); ++k) want.push_back({D.index(0, k), D.index(1, k), D.val(k)});
		expect("extract(extract(B, p, p), q, q)", Back, want, n, n);
		expect("extract(B, :, :)", C, want, n, n);
		if (P.size() != D.size()) { std::printf("FAIL permuted size\n"); ++failures; }
	}

	// an index out of range reaches the error hook, with its position
	bool raised = false;
	try { Mat R({1, 1}); spsparse_amd::extract(R, A, '.', std::vector<int>{0, 5}, spsparse_amd::all); }
	catch (const spsparse_amd::Exception &) { raised = std::strstr(spsamd_last_error(spsparse_amd::default_context().get()), "rows[1]") != nullptr; }
	if (!raised) { std::printf("FAIL out-of-range row did not raise with its position\n"); ++failures; }

	if (failures) return 1;
	std::printf("OK\n");
	return 0;
}
