// spsamd_color through the plain C ABI against the greedy loop of the header written out in C++: a Laplace 32^3 from
// spsamd_gen_laplace3d and a symmetrised R-MAT scale 12 (spsamd_gen_rmat, then spsamd_add of A and A^T, chained), both built
// on the device; both orders, with and without SPSAMD_COLOR_SYMMETRIC, host and device buffers.  Prints OK on success.
#include <spsparse_amd.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <utility>
#include <vector>

extern "C" int hipMalloc(void **ptr, size_t bytes);     // the runtime the library is linked against: device arrays for the generators
extern "C" int hipFree(void *ptr);

static int failures = 0;

static uint32_t hash32(uint32_t v, uint32_t seed)
{
	uint32_t h = v + seed * 0x9E3779B9u;
	h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
	return h;
}

struct Want { std::vector<int32_t> color, perm, ptr; uint64_t ncolors = 0, rounds = 0, adjacency = 0, max_degree = 0; };

// the loop of the header over the keys (i, j) of an n x n pattern, symmetrised
static Want greedy_loop(const std::vector<int32_t> &ki, const std::vector<int32_t> &kj, int n, int order, uint32_t seed)
{
	std::vector<std::pair<int32_t, int32_t>> e;
	for (size_t t = 0; t < ki.size(); ++t)
		if (ki[t] != kj[t]) { e.emplace_back(ki[t], kj[t]); e.emplace_back(kj[t], ki[t]); }
	std::sort(e.begin(), e.end());
	e.erase(std::unique(e.begin(), e.end()), e.end());
	std::vector<size_t> beg(n + 1, 0);
	for (auto &p : e) ++beg[p.first + 1];
	for (int i = 0; i < n; ++i) beg[i + 1] += beg[i];
	Want w;
	w.adjacency = e.size();
	std::vector<uint64_t> key(n);
	for (int v = 0; v < n; ++v) {
		const uint64_t deg = beg[v + 1] - beg[v];
		w.max_degree = std::max(w.max_degree, deg);
		key[v] = (order == SPSAMD_COLOR_ORDER_DEGREE ? deg << 32 : 0) | hash32((uint32_t)v, seed);
	}
	std::vector<int32_t> visit(n);
	std::iota(visit.begin(), visit.end(), 0);
	std::sort(visit.begin(), visit.end(), [&](int32_t a, int32_t b) { return key[a] > key[b]; });
	w.color.assign(n, -1);
	std::vector<int64_t> round(n, 0);
	std::vector<char> held;
	for (int32_t v : visit) {
		held.assign(beg[v + 1] - beg[v] + 1, 0);
		int64_t r = 0;
		for (size_t t = beg[v]; t < beg[v + 1]; ++t) {
			const int32_t u = e[t].second;
			if (w.color[u] >= 0 && (size_t)w.color[u] < held.size()) held[w.color[u]] = 1;
			if (key[u] > key[v]) r = std::max(r, round[u] + 1);
		}
		int32_t c = 0;
		while (held[c]) ++c;
		w.color[v] = c;
		round[v] = r;
		w.ncolors = std::max<uint64_t>(w.ncolors, (uint64_t)c + 1);
		w.rounds = std::max<uint64_t>(w.rounds, (uint64_t)r + 1);
	}
	w.perm.resize(n);
	std::iota(w.perm.begin(), w.perm.end(), 0);
	std::stable_sort(w.perm.begin(), w.perm.end(), [&](int32_t a, int32_t b) { return w.color[a] < w.color[b]; });
	w.ptr.assign(w.ncolors + 1, 0);
	for (int v = 0; v < n; ++v) ++w.ptr[w.color[v] + 1];
	for (uint64_t c = 0; c < w.ncolors; ++c) w.ptr[c + 1] += w.ptr[c];
	return w;
}

static void run_case(spsamd_ctx *ctx, const char *what, const spsamd_coo &A, const std::vector<int32_t> &ki, const std::vector<int32_t> &kj, int n)
{
	void *dc = nullptr, *dp = nullptr, *dq = nullptr;
	if (hipMalloc(&dc, (size_t)n * 4) || hipMalloc(&dp, (size_t)n * 4) || hipMalloc(&dq, ((size_t)n + 1) * 4)) { std::printf("FAIL hipMalloc\n"); ++failures; return; }
	for (int order = 0; order < 2; ++order) {
		const uint32_t seed = 17;
		const Want w = greedy_loop(ki, kj, n, order, seed);
		for (int variant = 0; variant < 3; ++variant) {                 // host buffers; host with the flag; device buffers
			const int flags = variant == 1 ? SPSAMD_COLOR_SYMMETRIC : 0, mem = variant == 2 ? SPSAMD_MEM_DEVICE : SPSAMD_MEM_HOST;
			std::vector<int32_t> color(n, -5), perm(n, -5), ptr(n + 1, -5);
			size_t nc = 0;
			spsamd_color_stats st;
			int rc = spsamd_color(ctx, &A, '.', order, seed, flags, mem == SPSAMD_MEM_DEVICE ? (int32_t *)dc : color.data(),
				mem == SPSAMD_MEM_DEVICE ? (int32_t *)dp : perm.data(), mem == SPSAMD_MEM_DEVICE ? (int32_t *)dq : ptr.data(), (size_t)n + 1, mem, &nc, &st, nullptr);
			if (rc != SPSAMD_OK) { std::printf("FAIL %s: rc %d %s\n", what, rc, spsamd_last_error(ctx)); ++failures; continue; }
			if (mem == SPSAMD_MEM_DEVICE && (spsamd_memcpy(ctx, color.data(), dc, (size_t)n * 4) || spsamd_memcpy(ctx, perm.data(), dp, (size_t)n * 4) ||
				spsamd_memcpy(ctx, ptr.data(), dq, (nc + 1) * 4))) { std::printf("FAIL %s: memcpy\n", what); ++failures; continue; }
			ptr.resize(nc + 1);
			if (nc != w.ncolors || st.ncolors != w.ncolors || st.rounds != w.rounds || st.adjacency != w.adjacency || st.max_degree != w.max_degree || st.conflicts != 0) {
				std::printf("FAIL %s order %d variant %d: colours %zu rounds %llu adjacency %llu max degree %llu conflicts %llu, want %llu %llu %llu %llu 0\n", what, order,
					variant, nc, (unsigned long long)st.rounds, (unsigned long long)st.adjacency, (unsigned long long)st.max_degree, (unsigned long long)st.conflicts,
					(unsigned long long)w.ncolors, (unsigned long long)w.rounds, (unsigned long long)w.adjacency, (unsigned long long)w.max_degree);
				++failures;
			}
			if (color != w.color || perm != w.perm || ptr != w.ptr) {
				size_t bad = 0;
				for (int v = 0; v < n; ++v) bad += color[v] != w.color[v];
				std::printf("FAIL %s order %d variant %d: %zu colours differ; perm %s, color_ptr %s\n", what, order, variant, bad, perm == w.perm ? "equal" : "differs",
					ptr == w.ptr ? "equal" : "differs");
				++failures;
			}
			if (variant == 0)
				std::printf("%s order %d: n %d colours %zu rounds %llu launches %llu fused rounds %llu\n", what, order, n, nc, (unsigned long long)st.rounds,
					(unsigned long long)st.launches, (unsigned long long)st.fused_rounds);
		}
	}
	hipFree(dc); hipFree(dp); hipFree(dq);
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
		const spsamd_coo A = {(const int32_t *)d0, (const int32_t *)d1, nullptr, (size_t)m, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};     // val is never read
		std::vector<int32_t> ki(m), kj(m);
		if (spsamd_memcpy(ctx, ki.data(), d0, m * 4) || spsamd_memcpy(ctx, kj.data(), d1, m * 4)) { std::printf("FAIL memcpy\n"); return 1; }
		run_case(ctx, "laplace 32^3", A, ki, kj, (int)n);
		hipFree(d0); hipFree(d1); hipFree(dv);
	}
	{   // R-MAT scale 12, edge factor 8: A + A^T, read in place as a chained result
		const int scale = 12, ef = 8;
		const uint64_t n = 1ull << scale, m = (uint64_t)ef * n;
		void *d0 = nullptr, *d1 = nullptr, *dv = nullptr;
		if (hipMalloc(&d0, m * 4) || hipMalloc(&d1, m * 4) || hipMalloc(&dv, m * 8)) { std::printf("FAIL hipMalloc\n"); return 1; }
		int rc = spsamd_gen_rmat(ctx, scale, ef, 3, 0, m, (int32_t *)d0, (int32_t *)d1, (double *)dv);
		if (rc != SPSAMD_OK) { std::printf("FAIL gen_rmat rc %d\n", rc); return 1; }
		const spsamd_coo A = {(const int32_t *)d0, (const int32_t *)d1, (const double *)dv, (size_t)m, (size_t)n, (size_t)n, -1, SPSAMD_MEM_DEVICE};
		spsamd_result sym;
		rc = spsamd_add(ctx, 1.0, &A, '.', 1.0, &A, 'T', SPSAMD_ADD, 0, SPSAMD_SINK_COO, 0, &sym);
		if (rc != SPSAMD_OK) { std::printf("FAIL add rc %d %s\n", rc, spsamd_last_error(ctx)); return 1; }
		std::vector<int32_t> ki(sym.nnz), kj(sym.nnz);
		if (spsamd_memcpy(ctx, ki.data(), sym.idx0, sym.nnz * 4) || spsamd_memcpy(ctx, kj.data(), sym.idx1, sym.nnz * 4)) { std::printf("FAIL memcpy\n"); return 1; }
		const spsamd_coo op = {sym.idx0, sym.idx1, sym.val, (size_t)sym.nnz, (size_t)n, (size_t)n, 0, SPSAMD_MEM_DEVICE};
		run_case(ctx, "rmat 12", op, ki, kj, (int)n);
		hipFree(d0); hipFree(d1); hipFree(dv);
	}
	{   // refusals
		int32_t i0[3] = {0, 1, 1}, i1[3] = {1, 0, 1}, color[3], ptr[4];
		const spsamd_coo tri = {i0, i1, nullptr, 3, 2, 2, 0, SPSAMD_MEM_HOST}, wide = {i0, i1, nullptr, 3, 2, 3, -1, SPSAMD_MEM_HOST};
		size_t nc = 0;
		int rc = spsamd_color(ctx, &wide, '.', 0, 0, 0, color, nullptr, nullptr, 0, SPSAMD_MEM_HOST, &nc, nullptr, nullptr);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL not square: rc %d\n", rc); ++failures; }
		rc = spsamd_color(ctx, &tri, '.', 0, 0, 0, nullptr, nullptr, nullptr, 0, SPSAMD_MEM_HOST, &nc, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL null color: rc %d\n", rc); ++failures; }
		rc = spsamd_color(ctx, &tri, '.', 0, 0, 0, color, nullptr, ptr, 2, SPSAMD_MEM_HOST, &nc, nullptr, nullptr);
		if (rc != SPSAMD_ECAPACITY || nc != 2) { std::printf("FAIL capacity: rc %d colours %zu\n", rc, nc); ++failures; }
		rc = spsamd_color(ctx, &tri, '.', 0, 0, 0, color, nullptr, ptr, 3, SPSAMD_MEM_HOST, &nc, nullptr, nullptr);
		if (rc != SPSAMD_OK || nc != 2 || color[0] == color[1] || ptr[0] != 0 || ptr[1] != 1 || ptr[2] != 2) { std::printf("FAIL two vertices: rc %d\n", rc); ++failures; }
	}
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
