// spsparse_amd::multiply through spsamd_multiply_stream (stream_block_tuples != 0) against the same call without it.
//
//   test_stream --abi-only   CPU: the template compiles with stream_block_tuples set, links, and the streamed path fails
//                            loudly without a GPU (the error hook is called, nothing is delivered)
//   test_stream              GPU: random products, both transposes, scale vectors and policies, at several budgets:
//                            the streamed accumulator holds the same tuples as the plain one, bit for bit (SINK_ORDERED)
//   test_stream --stream A.bin BUDGET OUT
//                            GPU: A*A of the square matrix in A.bin (n, nnz, then int32 i[], int32 j[], double v[]) streamed
//                            with stream_block_tuples = BUDGET into an accumulator that stores nothing: count, index hash and
//                            strict (i, j) order on stdout, per-row counts, index hashes and value sums to OUT.{nnz,hash,sum}
//   test_stream --digest A.bin OUT
//                            GPU: the same product through the digest sink with SINK_ROWSTATS, the same outputs
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include <spsparse_amd/multiply.hpp>

using namespace spsparse_amd;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

typedef VectorCooMatrix<int, double> Mat;
typedef VectorCooVector<int, double> Vec;

static std::string last_message;
static int errors_seen = 0;
static void recording_handler(int, const char *format, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, format);
	std::vsnprintf(buf, sizeof buf, format, ap);
	va_end(ap);
	last_message = buf;
	++errors_seen;
}

static Mat random_mat(std::mt19937_64 &g, size_t m, size_t n, size_t nnz)
{
	Mat A({m, n});
	std::uniform_int_distribution<int> ri(0, (int)m - 1), rj(0, (int)n - 1);
	std::uniform_real_distribution<double> rv(-1.0, 1.0);
	for (size_t q = 0; q < nnz; ++q) A.add({ri(g), rj(g)}, rv(g));
	return A;
}

static bool same(Mat const &X, Mat const &Y)
{
	if (X.size() != Y.size() || X.shape[0] != Y.shape[0] || X.shape[1] != Y.shape[1]) return false;
	for (size_t q = 0; q < X.size(); ++q) {
		if (X.index(0, q) != Y.index(0, q) || X.index(1, q) != Y.index(1, q)) return false;
		uint64_t a, b;
		double va = X.val(q), vb = Y.val(q);
		std::memcpy(&a, &va, 8); std::memcpy(&b, &vb, 8);
		if (a != b) return false;
	}
	return true;
}

static uint64_t mix64(uint32_t i, uint32_t j)          // the digest sink's index hash
{
	uint64_t x = (((uint64_t)i << 32) | (uint64_t)j) * 0x9E3779B97F4A7C15ull;
	return x ^ (x >> 29);
}

// An Accumulator (set_shape + add) that keeps per-row statistics only: a product larger than the device streams through it.
struct DigestAcc {
	typedef int index_type;
	typedef double val_type;
	static const int rank = 2;
	std::vector<int64_t> row_nnz;
	std::vector<uint64_t> row_hash;
	std::vector<double> row_sum;
	uint64_t count = 0, hash = 0;
	int64_t last = -1;
	bool ordered = true;
	void set_shape(std::array<size_t, 2> const &s) { row_nnz.assign(s[0], 0); row_hash.assign(s[0], 0); row_sum.assign(s[0], 0.0); }
	void add(std::array<int, 2> const &ix, double v)
	{
		const int64_t key = ((int64_t)ix[0] << 32) | (int64_t)(uint32_t)ix[1];
		if (key <= last) ordered = false;
		last = key;
		const uint64_t h = mix64((uint32_t)ix[0], (uint32_t)ix[1]);
		++count; hash += h;
		row_nnz[ix[0]] += 1; row_hash[ix[0]] += h; row_sum[ix[0]] += v;
	}
};

static bool read_square(const char *path, Mat &A)
{
	FILE *f = std::fopen(path, "rb");
	if (!f) return false;
	uint64_t hdr[2];
	bool ok = std::fread(hdr, 8, 2, f) == 2;
	std::vector<int32_t> i(hdr[1]), j(hdr[1]);
	std::vector<double> v(hdr[1]);
	ok = ok && std::fread(i.data(), 4, hdr[1], f) == hdr[1] && std::fread(j.data(), 4, hdr[1], f) == hdr[1] && std::fread(v.data(), 8, hdr[1], f) == hdr[1];
	std::fclose(f);
	if (!ok) return false;
	A = Mat({(size_t)hdr[0], (size_t)hdr[0]});
	const int32_t *cols[2] = {i.data(), j.data()};
	A.add_tuples(cols, v.data(), hdr[1]);
	return true;
}

template <class T>
static bool write_array(const std::string &path, const std::vector<T> &x)
{
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f) return false;
	const bool ok = std::fwrite(x.data(), sizeof(T), x.size(), f) == x.size();
	return std::fclose(f) == 0 && ok;
}

static int big_product(int argc, char **argv)
{
	const bool streamed = std::strcmp(argv[1], "--stream") == 0;
	if (argc != (streamed ? 5 : 4)) { std::printf("usage: test_stream --stream A.bin BUDGET OUT | --digest A.bin OUT\n"); return 2; }
	Mat A;
	if (!read_square(argv[2], A)) { std::printf("cannot read %s\n", argv[2]); return 2; }
	const std::string out = argv[streamed ? 4 : 3];
	const auto t0 = std::chrono::steady_clock::now();
	DigestAcc acc;
	if (streamed) {
		stream_block_tuples = (size_t)std::strtoull(argv[3], nullptr, 10);
		multiply(acc, 1.0, (Vec *)nullptr, A, '.', (Vec *)nullptr, A, '.', (Vec *)nullptr);
		stream_block_tuples = 0;
		if (errors_seen) { std::printf("FAILED: %s\n", last_message.c_str()); return 1; }
	} else {
		spsamd_ctx *ctx = default_context().get();
		spsamd_coo a = detail::as_coo(A);
		spsamd_result res;
		int rc = spsamd_multiply(ctx, 1.0, nullptr, &a, '.', nullptr, &a, '.', nullptr, SPSAMD_ADD, 0, SPSAMD_SINK_DIGEST,
			SPSAMD_SINK_ROWSTATS | SPSAMD_SINK_EXACT_PATTERN, &res);
		if (rc) { std::printf("FAILED: %s\n", spsamd_last_error(ctx)); return 1; }
		acc.set_shape({A.shape[0], A.shape[1]});
		rc = spsamd_memcpy(ctx, acc.row_nnz.data(), res.row_nnz, A.shape[0] * 8);
		rc = rc ? rc : spsamd_memcpy(ctx, acc.row_hash.data(), res.row_hash, A.shape[0] * 8);
		rc = rc ? rc : spsamd_memcpy(ctx, acc.row_sum.data(), res.row_sum, A.shape[0] * 8);
		if (rc) { std::printf("FAILED: %s\n", spsamd_last_error(ctx)); return 1; }
		acc.count = res.nnz; acc.hash = res.hash;
	}
	const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	if (!write_array(out + ".nnz", acc.row_nnz) || !write_array(out + ".hash", acc.row_hash) || !write_array(out + ".sum", acc.row_sum)) {
		std::printf("cannot write %s.*\n", out.c_str());
		return 2;
	}
	std::printf("count %llu hash %llu ordered %d seconds %.1f\n", (unsigned long long)acc.count, (unsigned long long)acc.hash,
		acc.ordered ? 1 : 0, s);
	return 0;
}

int main(int argc, char **argv)
{
	spsparse_error = &recording_handler;
	if (argc > 1 && (std::strcmp(argv[1], "--stream") == 0 || std::strcmp(argv[1], "--digest") == 0)) return big_product(argc, argv);
	if (argc > 1 && std::strcmp(argv[1], "--abi-only") == 0) {
		Mat A({3, 4}), B({4, 2}), C;
		A.add({0, 1}, 2.0); B.add({1, 1}, 3.0);
		stream_block_tuples = 64;
		multiply(C, 1.0, (Vec *)nullptr, A, '.', (Vec *)nullptr, B, '.', (Vec *)nullptr);
		const bool loud = errors_seen > 0 && C.size() == 0;
		std::printf("streamed multiply without a device: %s (%s)\n", loud ? "fails loudly" : "DID NOT FAIL", last_message.c_str());
		return loud ? 0 : 1;
	}
	multiply_flags = SPSAMD_SINK_ORDERED;
	std::mt19937_64 g(12345);
	long tuples = 0;
	for (int trial = 0; trial < 40; ++trial) {
		const size_t m = 1 + g() % 300, k = 1 + g() % 200, n = 1 + g() % 5000;
		const char tA = trial % 2 ? 'T' : '.', tB = trial % 3 ? '.' : 'T';
		Mat A = tA == 'T' ? random_mat(g, k, m, 1 + g() % 3000) : random_mat(g, m, k, 1 + g() % 3000);
		Mat B = tB == 'T' ? random_mat(g, n, k, 1 + g() % 20000) : random_mat(g, k, n, 1 + g() % 20000);
		Vec si({m});
		for (size_t r = 0; r < m; r += 2) si.add({(int)r}, 0.5 + (double)r);
		const DuplicatePolicy pol = trial % 3 == 0 ? DuplicatePolicy::ADD : (trial % 3 == 1 ? DuplicatePolicy::REPLACE : DuplicatePolicy::LEAVE_ALONE);
		Mat plain;
		stream_block_tuples = 0;
		multiply(plain, 2.0, trial % 4 ? &si : nullptr, A, tA, (Vec *)nullptr, B, tB, (Vec *)nullptr, pol);
		for (size_t budget : {size_t(5000), size_t(20000), size_t(1) << 40}) {
			Mat s2;
			stream_block_tuples = budget;
			errors_seen = 0;
			multiply(s2, 2.0, trial % 4 ? &si : nullptr, A, tA, (Vec *)nullptr, B, tB, (Vec *)nullptr, pol);
			if (errors_seen) {
				// the only refusal allowed here: a row that can produce more tuples than the budget
				CHECK(last_message.find("smallest budget") != std::string::npos);
				continue;
			}
			CHECK(same(plain, s2));
		}
		tuples += (long)plain.size();
	}
	stream_block_tuples = 0;
	std::printf("streamed = plain on 40 products, %ld tuples\n", tuples);
	CHECK(tuples > 10000);
	std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
	return failures ? 1 : 0;
}
