// bank_layout.h -- where a column lands in the LDS arrays of k_dense and k_bm_tiles.
//
// Both kernels take their LDS addresses from low column bits, and the bits of real column indices are not fair coins
// (R-MAT without vertex scrambling: every bit is set with probability 0.24; strides and blocks elsewhere), so a few banks
// take most of the traffic.  The remaps below are bijections that spread such indices over the banks and cost no LDS
// operation; uniform indices stay uniform.  Chosen with scripts/bank_skew.py.  Plain C++: host programs include this too.
#pragma once
#include <stdint.h>
#include "workload_common.h"

namespace spsamd {

// ---- k_dense: slot s of the window accumulator lives at s ^ dense_swz(s >> 6).  The value depends on the 64-slot group
// alone and is below 64: a permutation inside every group (any window size), and one group read by 64 consecutive lanes
// is still 64 consecutive slots.  The group's bits reach all six low bits through the product's carries.
SPS_HD uint32_t dense_swz(uint32_t group) { return ((group * 181u) >> 3) & 63u; }
SPS_HD uint32_t dense_phys(uint32_t slot) { return slot ^ dense_swz(slot >> 6); }

// ---- k_bm_tiles: a column relative to the cell's first, rel < 2^17, is known inside the cell by a key: the low 14 bits
// of rel * K (K odd: a bijection modulo 2^14; KINV its inverse) under rel's bits 14..16.  Bit b < 14 of the key mixes bits
// 0..b of rel; the banks come from bits 5..11.  The top bits stay: a key falls into the same 256 bitmap words -- one wave's
// share of the scan and of the cleaning -- as its column, so the waves beyond a cell's column range still find nothing to do.
// Both factors of either product are below 2^24: the 24-bit multiply applies, and a bit-field insert does the rest.
constexpr uint32_t TILE_KEY_BITS = 17, TILE_KEY_MASK = (1u << TILE_KEY_BITS) - 1u;
constexpr uint32_t TILE_KEY_LOW_BITS = 14, TILE_KEY_LOW = (1u << TILE_KEY_LOW_BITS) - 1u;
constexpr uint32_t TILE_KEY_K = 40503u, TILE_KEY_KINV = 96135u;
static_assert(((TILE_KEY_K * TILE_KEY_KINV) & TILE_KEY_MASK) == 1u, "inverse modulo 2^17, hence modulo 2^14");

SPS_HD uint32_t bank_mul24(uint32_t x, uint32_t k)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __umul24(x, k);
#else
	return x * k;
#endif
}
SPS_HD uint32_t tile_key(uint32_t rel) { return rel ^ ((rel ^ bank_mul24(rel, TILE_KEY_K)) & TILE_KEY_LOW); }
SPS_HD uint32_t tile_rel(uint32_t key) { return key ^ ((key ^ bank_mul24(key, TILE_KEY_KINV)) & TILE_KEY_LOW); }

} // namespace spsamd
