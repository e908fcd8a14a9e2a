// devutil.h -- wave64 / workgroup helpers shared by the kernels (gfx950: wavefront = 64).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spsamd {

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ unsigned wave_id() { return threadIdx.x >> 6; }
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << lane_id()) - 1ull; }

// Inclusive scan across the 64 lanes of a wave (generic: LDS-crossbar shuffles).
template <class T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		T o = __shfl_up(v, d, 64);
		if ((int)lane_id() >= d) v += o;
	}
	return v;
}

// uint32 inclusive scan with DPP row shifts and row broadcasts (gfx9 family): six
// VALU adds instead of six dependent ds_bpermute round trips.
__device__ __forceinline__ uint32_t wave_inclusive_scan_u32(uint32_t v)
{
	int x = (int)v;
	x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);      // row_shr:1
	x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);      // row_shr:2
	x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);      // row_shr:4
	x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);      // row_shr:8
	x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true);      // row_bcast:15 -> rows 1 and 3
	x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, true);      // row_bcast:31 -> rows 2 and 3
	return (uint32_t)x;
}

// Inclusive scan inside aligned groups of S lanes (S = 8, 16, 32, 64), DPP only.
// s = lane index inside the group.
template <int S>
__device__ __forceinline__ uint32_t group_inclusive_scan_u32(uint32_t v, unsigned s)
{
	int x = (int)v, t;
	t = __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true); if (s >= 1) x += t;      // row_shr:1 (rows of 16 lanes)
	t = __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true); if (s >= 2) x += t;
	t = __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true); if (s >= 4) x += t;
	if (S >= 16) { t = __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true); if (s >= 8) x += t; }
	if (S >= 32) { t = __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, true); if (s >= 16) x += t; }   // row_bcast:15
	if (S >= 64) { t = __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, true); if (s >= 32) x += t; }   // row_bcast:31
	return (uint32_t)x;
}

template <class T>
__device__ __forceinline__ T wave_reduce_sum(T v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}

// Exclusive scan across a workgroup of NT threads (NT multiple of 64, <= 1024).
// scratch: NT/64 + 1 entries of T in LDS.  Returns the exclusive prefix of v;
// *total (if non-null) receives the workgroup sum.  Contains three barriers.
template <class T, int NT>
__device__ __forceinline__ T block_exclusive_scan(T v, T *scratch, T *total)
{
	constexpr int NW = NT / 64;
	T inc = wave_inclusive_scan(v);
	if (lane_id() == 63) scratch[wave_id()] = inc;
	__syncthreads();
	if (threadIdx.x == 0) {
		T run = 0;
#pragma unroll
		for (int w = 0; w < NW; ++w) { T t = scratch[w]; scratch[w] = run; run += t; }
		scratch[NW] = run;
	}
	__syncthreads();
	T base = scratch[wave_id()];
	T tot = scratch[NW];
	__syncthreads();            // scratch may be reused right away
	if (total) *total = tot;
	return base + inc - v;
}

// mag(x): the bits of x with the sign cleared, compared as an unsigned integer where no floating-point comparison may decide
__device__ __forceinline__ uint64_t mag_of(double v) { return (uint64_t)__double_as_longlong(v) & 0x7FFFFFFFFFFFFFFFull; }

// ---- order-preserving compaction over wave tiles, lists claimed from a counter ----------------
// A new operation calls these, it does not copy them.  Every lane of the wave must call them (they ballot).

constexpr int WAVE_TILE_ROUNDS = 8;
constexpr int WAVE_TILE = 64 * WAVE_TILE_ROUNDS;   // elements a wave of a count / compact pass takes: 8 rounds of 64

// How many i of [base, min(base + WAVE_TILE, n)) have keep(i).  keep is called for i < n only (it may store per element).
template <class Keep>
__device__ __forceinline__ uint32_t wave_tile_count(uint64_t base, uint64_t n, Keep keep)
{
	uint32_t cnt = 0;
#pragma unroll
	for (int r = 0; r < WAVE_TILE_ROUNDS; ++r) {
		const uint64_t i = base + (uint64_t)r * 64 + lane_id();
		cnt += (uint32_t)__popcll(__ballot(i < n && keep(i)));
	}
	return cnt;
}

// store(i, p) for every i of the wave-uniform range [a0, a1) with keep(i), p = o, o + 1, ... in the order of i: `o` is the
// scanned count of what the waves before this one keep.  No atomic: the output is in input order.  The range may be empty
// or longer than a tile.  A whole tile's eight rounds are unrolled, so that their loads are issued together; what is left
// of the range goes round by round, so a short range (the merge path hands out half tiles) pays for the rounds it has.
template <class Keep, class Store>
__device__ __forceinline__ void wave_range_compact(uint64_t a0, uint64_t a1, uint32_t o, Keep keep, Store store)
{
	auto round = [&](uint64_t base) {
		const uint64_t i = base + lane_id();
		const bool k = i < a1 && keep(i);
		const uint64_t m = __ballot(k);
		if (k) store(i, o + (uint32_t)__popcll(m & lanemask_lt()));
		o += (uint32_t)__popcll(m);
	};
	uint64_t base = a0;
	for (; base + WAVE_TILE <= a1; base += WAVE_TILE) {                // uniform
#pragma unroll
		for (int r = 0; r < WAVE_TILE_ROUNDS; ++r) round(base + (uint64_t)r * 64);
	}
	for (; base < a1; base += 64) round(base);                         // uniform
}

// Appends the lanes with `pred` to the list that *counter counts and returns each one's slot (a lane without `pred` gets a
// number that means nothing): one atomic per wave, none when no lane has it.  The list ends up in no particular order.
__device__ __forceinline__ uint32_t wave_claim(uint32_t *counter, bool pred)
{
	const uint64_t m = __ballot(pred);
	if (!m) return 0;                                                  // uniform
	uint32_t at = 0;
	if (lane_id() == 0) at = atomicAdd(counter, (uint32_t)__popcll(m));
	at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
	return at + (uint32_t)__popcll(m & lanemask_lt());
}

// ---- the graph operations (k_color.hip, k_aggregate.hip) ------------------------------------------------------------

// h(v) of the header: the visiting order of spsamd_color and spsamd_aggregate
__device__ __forceinline__ uint32_t col_hash(uint32_t v, uint32_t seed)
{
	uint32_t h = v + seed * 0x9E3779B9u;
	h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
	return h;
}

// first position of [b, e) whose neighbour is >= j
__device__ __forceinline__ uint32_t col_lower_bound(const int32_t *adj, uint32_t b, uint32_t e, int32_t j)
{
	while (b < e) {
		const uint32_t m = b + ((e - b) >> 1);
		if (adj[m] < j) b = m + 1; else e = m;
	}
	return b;
}

__device__ __forceinline__ int32_t wave_reduce_max(int32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
	return v;
}

// Index hash of the digest sink: one 64-bit multiply and a fold of (i, j).
// Same arithmetic as orc_mix64 in the test oracle.
__host__ __device__ __forceinline__ uint64_t mix64(uint32_t i, uint32_t j)
{
	uint64_t x = (((uint64_t)i << 32) | (uint64_t)j) * 0x9E3779B97F4A7C15ull;
	return x ^ (x >> 29);
}

} // namespace spsamd
