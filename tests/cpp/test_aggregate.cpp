// spsamd_aggregate through the plain C ABI against the loop of the header written out in C++: three dozen random patterns of
// up to 200 vertices, symmetric and not, host operands, both orders, with and without SPSAMD_AGG_SYMMETRIC, host and device
// buffers; then the refusals.  Prints OK on success.
#include <spsparse_amd.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <set>
#include <utility>
#include <vector>

extern "C" int hipMalloc(void **ptr, size_t bytes);     // the runtime the library is linked against: the device buffers
extern "C" int hipFree(void *ptr);

static int failures = 0;

static uint32_t hash32(uint32_t v, uint32_t seed)
{
	uint32_t h = v + seed * 0x9E3779B9u;
	h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
	return h;
}

static uint64_t next_random(uint64_t &s)
{
	s += 0x9E3779B97F4A7C15ull;
	uint64_t z = s;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

struct Want { std::vector<int32_t> agg, members, ptr; uint64_t naggregates = 0, ring1 = 0, ring2 = 0, adjacency = 0, max_degree = 0, asymmetric = 0; };

// the loop of the header over the keys (i, j) of an n x n pattern, symmetrised
static Want serial_loop(const std::vector<int32_t> &ki, const std::vector<int32_t> &kj, int n, int order, uint32_t seed)
{
	std::set<std::pair<int32_t, int32_t>> have;
	for (size_t t = 0; t < ki.size(); ++t) have.emplace(ki[t], kj[t]);
	Want w;
	std::vector<std::set<int32_t>> nb(n);
	for (auto &p : have)
		if (p.first != p.second) {
			nb[p.first].insert(p.second); nb[p.second].insert(p.first);
			if (!have.count({p.second, p.first})) ++w.asymmetric;
		}
	std::vector<uint64_t> key(n);
	for (int v = 0; v < n; ++v) {
		const uint64_t deg = nb[v].size();
		w.adjacency += deg;
		w.max_degree = std::max(w.max_degree, deg);
		key[v] = (order == SPSAMD_AGG_ORDER_DEGREE ? deg << 32 : 0) | hash32((uint32_t)v, seed);
	}
	std::vector<int32_t> visit(n);
	std::iota(visit.begin(), visit.end(), 0);
	std::sort(visit.begin(), visit.end(), [&](int32_t a, int32_t b) { return key[a] > key[b]; });
	std::vector<char> root(n, 0);
	for (int32_t v : visit) {
		bool near = false;                                              // a root within distance 2 of v
		for (int32_t x : nb[v]) {
			near = near || root[x];
			for (int32_t u : nb[x]) near = near || (u != v && root[u]);
		}
		root[v] = !near;
	}
	std::vector<int32_t> id(n, 0), ring(n, 2);
	for (int v = 0; v < n; ++v) { id[v] = (int32_t)w.naggregates; w.naggregates += root[v]; }
	w.agg.assign(n, -1);
	for (int v = 0; v < n; ++v) {
		if (root[v]) { w.agg[v] = id[v]; ring[v] = 0; continue; }
		for (int32_t r : nb[v]) if (root[r]) { w.agg[v] = id[r]; ring[v] = 1; }
	}
	for (int v = 0; v < n; ++v) {
		if (ring[v] != 2) continue;
		int32_t best = -1;
		for (int32_t x : nb[v]) if (ring[x] == 1 && (best < 0 || key[x] > key[best])) best = x;
		w.agg[v] = best < 0 ? -1 : w.agg[best];
	}
	for (int v = 0; v < n; ++v) { w.ring1 += ring[v] == 1; w.ring2 += ring[v] == 2; }
	w.members.resize(n);
	std::iota(w.members.begin(), w.members.end(), 0);
	std::stable_sort(w.members.begin(), w.members.end(), [&](int32_t a, int32_t b) {
		return std::make_pair(w.agg[a], ring[a]) < std::make_pair(w.agg[b], ring[b]); });
	w.ptr.assign(w.naggregates + 1, 0);
	for (int v = 0; v < n; ++v) ++w.ptr[w.agg[v] + 1];
	for (uint64_t a = 0; a < w.naggregates; ++a) w.ptr[a + 1] += w.ptr[a];
	return w;
}

constexpr int MAX_N = 200;
static void *da = nullptr, *dm = nullptr, *dq = nullptr;                 // the device buffers, for MAX_N vertices

static void run_case(spsamd_ctx *ctx, int trial, const spsamd_coo &A, const std::vector<int32_t> &ki, const std::vector<int32_t> &kj, int n, uint32_t seed)
{
	for (int order = 0; order < 2; ++order) {
		const Want w = serial_loop(ki, kj, n, order, seed);
		for (int variant = 0; variant < 3; ++variant) {                 // host buffers; host with the flag; device buffers
			const int flags = variant == 1 ? SPSAMD_AGG_SYMMETRIC : 0, mem = variant == 2 ? SPSAMD_MEM_DEVICE : SPSAMD_MEM_HOST;
			std::vector<int32_t> agg(n, -5), members(n, -5), ptr(n + 1, -5);
			size_t na = 0;
			spsamd_aggregate_stats st;
			int rc = spsamd_aggregate(ctx, &A, '.', order, seed, flags, mem == SPSAMD_MEM_DEVICE ? (int32_t *)da : agg.data(),
				mem == SPSAMD_MEM_DEVICE ? (int32_t *)dm : members.data(), mem == SPSAMD_MEM_DEVICE ? (int32_t *)dq : ptr.data(), (size_t)n + 1, mem, &na, &st, nullptr);
			if (flags && w.asymmetric) {                                   // the promise is false: refused, the count reported, nothing written
				if (rc != SPSAMD_EINVAL || st.asymmetric != w.asymmetric || agg != std::vector<int32_t>(n, -5) || ptr != std::vector<int32_t>(n + 1, -5)) {
					std::printf("FAIL trial %d order %d: a false promise: rc %d asymmetric %llu, want %llu\n", trial, order, rc, (unsigned long long)st.asymmetric,
						(unsigned long long)w.asymmetric);
					++failures;
				}
				continue;
			}
			if (rc != SPSAMD_OK) { std::printf("FAIL trial %d: rc %d %s\n", trial, rc, spsamd_last_error(ctx)); ++failures; continue; }
			if (mem == SPSAMD_MEM_DEVICE && (spsamd_memcpy(ctx, agg.data(), da, (size_t)n * 4) || spsamd_memcpy(ctx, members.data(), dm, (size_t)n * 4) ||
				spsamd_memcpy(ctx, ptr.data(), dq, (na + 1) * 4))) { std::printf("FAIL trial %d: memcpy\n", trial); ++failures; continue; }
			ptr.resize(na + 1);
			uint64_t mx = 0, mn = ~0ull;
			for (size_t a = 0; a + 1 < w.ptr.size(); ++a) { mx = std::max<uint64_t>(mx, w.ptr[a + 1] - w.ptr[a]); mn = std::min<uint64_t>(mn, w.ptr[a + 1] - w.ptr[a]); }
			if (na != w.naggregates || st.naggregates != w.naggregates || st.ring1 != w.ring1 || st.ring2 != w.ring2 || st.adjacency != w.adjacency ||
				st.max_degree != w.max_degree || st.max_size != mx || st.min_size != mn || st.asymmetric != 0 || st.rounds == 0 || st.rows_thread + st.rows_wave != (uint64_t)n) {
				std::printf("FAIL trial %d order %d variant %d: aggregates %zu rings %llu %llu adjacency %llu max degree %llu sizes %llu %llu, want %llu %llu %llu %llu %llu %llu %llu\n",
					trial, order, variant, na, (unsigned long long)st.ring1, (unsigned long long)st.ring2, (unsigned long long)st.adjacency, (unsigned long long)st.max_degree,
					(unsigned long long)st.max_size, (unsigned long long)st.min_size, (unsigned long long)w.naggregates, (unsigned long long)w.ring1, (unsigned long long)w.ring2,
					(unsigned long long)w.adjacency, (unsigned long long)w.max_degree, (unsigned long long)mx, (unsigned long long)mn);
				++failures;
			}
			if (agg != w.agg || members != w.members || ptr != w.ptr) {
				size_t bad = 0;
				for (int v = 0; v < n; ++v) bad += agg[v] != w.agg[v];
				std::printf("FAIL trial %d order %d variant %d: %zu ids differ; members %s, agg_ptr %s\n", trial, order, variant, bad, members == w.members ? "equal" : "differs",
					ptr == w.ptr ? "equal" : "differs");
				++failures;
			}
		}
	}
}

int main(int argc, char **argv)
{
	if (argc > 1 && !std::strcmp(argv[1], "--abi-only")) {
		static_assert(sizeof(spsamd_aggregate_stats) == 13 * 8 + 3 * 4 + 4, "thirteen counters and three times");
		std::printf("OK\n");
		return 0;
	}
	const auto t0 = std::chrono::steady_clock::now();
	auto seconds = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
	spsamd_ctx *ctx = nullptr;
	if (spsamd_ctx_create(&ctx, -1, nullptr) != SPSAMD_OK) { std::printf("FAIL no context\n"); return 1; }
	if (hipMalloc(&da, MAX_N * 4) || hipMalloc(&dm, MAX_N * 4) || hipMalloc(&dq, (MAX_N + 1) * 4)) { std::printf("FAIL hipMalloc\n"); return 1; }
	std::printf("context and buffers after %.2f s\n", seconds());
	uint64_t rs = 2402;
	for (int trial = 0; trial < 36; ++trial) {
		const int n = trial ? 1 + (int)(next_random(rs) % MAX_N) : MAX_N;  // (the largest first: the workspace grows once)
		const bool symmetric = trial % 3 != 0;
		const size_t m = (size_t)(next_random(rs) % (3 * (uint64_t)n + 1));
		std::vector<int32_t> ki, kj;
		for (size_t t = 0; t < m; ++t) {
			const int32_t i = (int32_t)(next_random(rs) % n), j = (int32_t)(next_random(rs) % n);
			ki.push_back(i); kj.push_back(j);
			if (symmetric) { ki.push_back(j); kj.push_back(i); }
		}
		const spsamd_coo A = {ki.data(), kj.data(), nullptr, ki.size(), (size_t)n, (size_t)n, -1, SPSAMD_MEM_HOST};          // val is never read
		run_case(ctx, trial, A, ki, kj, n, (uint32_t)next_random(rs));
	}
	std::printf("patterns after %.2f s\n", seconds());
	{   // refusals
		int32_t i0[4] = {0, 1, 1, 2}, i1[4] = {1, 0, 2, 1}, agg[3], ptr[4];
		const spsamd_coo path = {i0, i1, nullptr, 4, 3, 3, 0, SPSAMD_MEM_HOST}, wide = {i0, i1, nullptr, 4, 3, 4, -1, SPSAMD_MEM_HOST},
			directed = {i0, i1, nullptr, 3, 3, 3, 0, SPSAMD_MEM_HOST};
		size_t na = 0;
		int rc = spsamd_aggregate(ctx, &wide, '.', 0, 0, 0, agg, nullptr, nullptr, 0, SPSAMD_MEM_HOST, &na, nullptr, nullptr);
		if (rc != SPSAMD_EDIM) { std::printf("FAIL not square: rc %d\n", rc); ++failures; }
		rc = spsamd_aggregate(ctx, &path, '.', 0, 0, 0, nullptr, nullptr, nullptr, 0, SPSAMD_MEM_HOST, &na, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL null agg: rc %d\n", rc); ++failures; }
		rc = spsamd_aggregate(ctx, &directed, '.', 0, 0, SPSAMD_AGG_SYMMETRIC, agg, nullptr, nullptr, 0, SPSAMD_MEM_HOST, &na, nullptr, nullptr);
		if (rc != SPSAMD_EINVAL) { std::printf("FAIL a false promise: rc %d\n", rc); ++failures; }
		rc = spsamd_aggregate(ctx, &path, '.', 0, 0, 0, agg, nullptr, ptr, 1, SPSAMD_MEM_HOST, &na, nullptr, nullptr);
		if (rc != SPSAMD_ECAPACITY || na != 1) { std::printf("FAIL capacity: rc %d aggregates %zu\n", rc, na); ++failures; }
		rc = spsamd_aggregate(ctx, &path, '.', 0, 0, SPSAMD_AGG_SYMMETRIC, agg, nullptr, ptr, 2, SPSAMD_MEM_HOST, &na, nullptr, nullptr);
		if (rc != SPSAMD_OK || na != 1 || agg[0] || agg[1] || agg[2] || ptr[0] != 0 || ptr[1] != 3) { std::printf("FAIL path of three: rc %d\n", rc); ++failures; }
	}
	hipFree(da); hipFree(dm); hipFree(dq);
	spsamd_ctx_destroy(ctx);
	if (failures) { std::printf("%d failures\n", failures); return 1; }
	std::printf("OK\n");
	return 0;
}
