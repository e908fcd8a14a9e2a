// k_extract.hip -- the submatrix op(A)(I, J) by row and column lists (spsamd_extract, include/spsparse_amd.h).
//
// S = op(A) as consolidate_operand() hands it over (row-major; consolidated, or trusted as stored), with a dense row
// pointer.  Output row r holds, for every tuple (I[r], j, v) of S at position p and every output column c with J[c] == j,
// one tuple (r, c, v), in (c, p) order.  No value is computed: every value keeps its bits.
//
// Device path:
//   1. k_ext_check validates I and J (first entry out of range, strictly ascending?, a repeated index?) and builds J's
//      column map on the way: an int32 inverse over cols(op(A)) (new column or -1), or -- when J repeats an index -- a CSR
//      of J by source column (radix_sort_pairs on J[c], payload c: the output columns ascend per source column).
//   2. count: n_r = sum of mult(col) over the tuples of source row I[r].  Source rows of at most 64 tuples: k_ext_short, a
//      wave per 64 consecutive output rows, their tuples packed a lane each (the owning row by a search over the wave's 64
//      row ends), counted by ballots.  Longer rows: k_ext_rows, a wave per row, beyond 4096 tuples a workgroup per row.
//      scan_exclusive_u32_i64 turns the counts into offsets.
//   3. emit: the same kernels again, storing (r, map[col], v) at off[r] + the tuple's rank in its row (ballot + popcount;
//      a wave scan where a column is named more than once).  No atomic touches the output.  Where J is ascending (or ALL)
//      and S is column-ordered inside its rows, that is the result (the in-order path).
//   4. otherwise every output row of two or more tuples is brought into (c, p) order by a stable sort on c, by class of n_r:
//      k_ext_sort_light (n_r <= 64: a wave per row, or a group of 8 / 16 / 32 lanes per short row; rank by compare-all), k_ext_sort_mid
//      (n_r <= 4096: a workgroup per row, keys c << 12 | position in LDS, bitonic network, values gathered by the sorted
//      position), heavy (one radix_sort_pairs over the remaining rows' tuples on (heavy row << bits(ncols) | c), gather).
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace spsamd {

constexpr int EXT_SHORT_MAX = 64;              // longest source row of the packed kernel / output row of the light sort
constexpr int EXT_MID_MAX = 4096;              // longest source row a wave takes / output row of the mid sort (32 KiB of LDS keys)
constexpr int EXT_LONG_NT = 64;
constexpr int EXT_HUGE_NT = 1024;
constexpr int EXT_MID_NT = 256;

enum { EXT_MAP_ALL = 0, EXT_MAP_INVERSE = 1, EXT_MAP_CSR = 2 };

struct ExtMap {
	const int32_t *inv;                        // INVERSE: output column of a source column, or -1
	const uint32_t *jptr;                      // CSR: pointer per source column ...
	const uint32_t *jout;                      // ... into the output columns, ascending per source column
};

// how many output columns name source column `col`; `first`: the output column (ALL, INVERSE) or where they start in jout
template <int MAP>
__device__ __forceinline__ uint32_t ext_mult(const ExtMap &m, int32_t col, uint32_t &first)
{
	if (MAP == EXT_MAP_ALL) { first = (uint32_t)col; return 1u; }
	if (MAP == EXT_MAP_INVERSE) { const int32_t c = m.inv[col]; first = (uint32_t)c; return c >= 0 ? 1u : 0u; }
	const uint32_t b = m.jptr[col];
	first = b;
	return m.jptr[col + 1] - b;
}

template <int MAP>
__device__ __forceinline__ void ext_store(const ExtMap &m, uint32_t pos, uint32_t mult, uint32_t first, int32_t r, double v,
	int32_t *__restrict__ orow, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	if (MAP != EXT_MAP_CSR) {
		if (mult) { orow[pos] = r; ocol[pos] = (int32_t)first; oval[pos] = v; }
		return;
	}
	for (uint32_t q = 0; q < mult; ++q) { orow[pos + q] = r; ocol[pos + q] = (int32_t)m.jout[first + q]; oval[pos + q] = v; }
}

__device__ __forceinline__ uint64_t bits_below(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ uint32_t clamp_u32(uint64_t x) { return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x; }

// One list: w[0] = ~(first position out of [0, dim)) (0: none), w[1] = an entry is not above its predecessor, w[2] = an
// index occurs twice (only looked for where `inv` is given: inv[x] = position, claimed once).
__global__ void __launch_bounds__(256) k_ext_check(const int32_t *__restrict__ list, uint32_t n, uint64_t dim, int32_t *inv, uint32_t *w)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false, desc = false, rep = false;
	if (i < n) {
		const int32_t x = list[i];
		bad = x < 0 || (uint64_t)x >= dim;
		desc = i > 0 && list[i - 1] >= x;
		if (!bad && inv) rep = atomicCAS(&inv[x], -1, (int32_t)i) != -1;
	}
	const uint64_t mb = __ballot(bad), md = __ballot(desc), mr = __ballot(rep);
	if (lane_id() == 0) {
		if (mb) atomicMax(&w[0], ~(i + (uint32_t)(__ffsll((unsigned long long)mb) - 1)));
		if (md) atomicOr(&w[1], 1u);
		if (mr) atomicOr(&w[2], 1u);
	}
}

__global__ void __launch_bounds__(256) k_ext_list_keys(const int32_t *__restrict__ list, uint32_t n, uint64_t *__restrict__ keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = (uint64_t)(uint32_t)list[i];
}

__global__ void __launch_bounds__(256) k_ext_low32(const uint64_t *__restrict__ keys, uint32_t n, int32_t *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = (int32_t)(uint32_t)keys[i];
}

// the output rows whose source row is too long for the packed kernel: w[0] of them up to EXT_MID_MAX tuples, w[1] beyond
// (an entry of I out of range is skipped: the call is refused once the check's words are read)
__global__ void __launch_bounds__(256) k_ext_src_classify(const int32_t *__restrict__ I, uint64_t nR, uint64_t nrowS,
	const uint32_t *__restrict__ ptr, uint32_t *w, uint32_t *__restrict__ long_list, uint32_t *__restrict__ huge_list)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t len = 0;
	if (r < nR) {
		const int64_t src = I ? (int64_t)I[r] : (int64_t)r;
		if (src >= 0 && (uint64_t)src < nrowS) len = ptr[src + 1] - ptr[src];
	}
	const int cls = len <= (uint32_t)EXT_SHORT_MAX ? -1 : len <= (uint32_t)EXT_MID_MAX ? 0 : 1;
#pragma unroll
	for (int q = 0; q < 2; ++q) {
		const uint32_t slot = wave_claim(&w[q], cls == q);
		if (cls == q) (q == 0 ? long_list : huge_list)[slot] = (uint32_t)r;
	}
}

struct ExtArgs {
	const int32_t *I;                          // null: output row r is source row r
	uint64_t nR;
	const uint32_t *ptr;                       // dense row pointer of S
	const int32_t *col;
	const double *val;
	ExtMap map;
	uint32_t *cnt;                             // count pass: n_r
	const int64_t *off;                        // emit pass: first output position of row r
	int32_t *orow, *ocol;
	double *oval;
};

// Source rows of at most EXT_SHORT_MAX tuples: a wave takes 64 consecutive output rows (a lane each for the bookkeeping) and
// walks their tuples packed, 64 at a time, a lane each.
template <int MAP, bool EMIT>
__global__ void __launch_bounds__(256) k_ext_short(ExtArgs a)
{
	__shared__ uint32_t s_end[4][64];
	const uint32_t w = wave_id(), lane = lane_id();
	const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + w) * 64, r = r0 + lane;
	uint32_t beg = 0, len = 0;
	bool mine = false;
	if (r < a.nR) {
		const uint32_t src = a.I ? (uint32_t)a.I[r] : (uint32_t)r;
		beg = a.ptr[src];
		len = a.ptr[src + 1] - beg;
		mine = len <= (uint32_t)EXT_SHORT_MAX;
		if (!mine) len = 0;                                        // served by k_ext_rows
	}
	const uint32_t end = wave_inclusive_scan_u32(len), start = end - len;
	s_end[w][lane] = end;
	__syncthreads();
	const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)end, 63);
	uint64_t run = 0;                                              // outputs of this lane's row so far
	const uint32_t myoff = EMIT && r < a.nR ? (uint32_t)a.off[r] : 0u;
	for (uint32_t base = 0; base < total; base += 64) {           // uniform
		const uint32_t slot = base + lane;
		const bool act = slot < total;
		uint32_t k = 0;                                            // the row of this slot: how many rows end at or before it
		if (act) {
#pragma unroll
			for (uint32_t step = 32; step; step >>= 1) if (s_end[w][k + step - 1] <= slot) k += step;
		}
		const uint32_t kstart = (uint32_t)__shfl((int)start, (int)k, 64), kbeg = (uint32_t)__shfl((int)beg, (int)k, 64);
		uint32_t mult = 0, first = 0;
		double v = 0;
		if (act) {
			const uint32_t t = kbeg + (slot - kstart);
			mult = ext_mult<MAP>(a.map, a.col[t], first);
			if (EMIT && mult) v = a.val[t];
		}
		// [lo, hi): the lanes of this chunk that hold this lane's own row; rs: the first lane of the slot's row
		const int lo = (int)std::min<int64_t>(std::max<int64_t>((int64_t)start - base, 0), 64);
		const int hi = (int)std::min<int64_t>(std::max<int64_t>((int64_t)end - base, 0), 64);
		const int rs = (int)std::max<int64_t>((int64_t)kstart - base, 0);
		uint64_t own, before;
		if (MAP != EXT_MAP_CSR) {
			const uint64_t m = __ballot(mult != 0);
			own = (uint64_t)__popcll(m & bits_below(hi) & ~bits_below(lo));
			before = (uint64_t)__popcll(m & lanemask_lt() & ~bits_below(rs));
		} else {
			const unsigned long long incl = wave_inclusive_scan<unsigned long long>((unsigned long long)mult);
			const unsigned long long at_hi = __shfl(incl, hi > 0 ? hi - 1 : 0, 64), at_lo = __shfl(incl, lo > 0 ? lo - 1 : 0, 64);
			const unsigned long long at_rs = __shfl(incl, rs > 0 ? rs - 1 : 0, 64);
			own = hi > lo ? at_hi - (lo > 0 ? at_lo : 0ull) : 0ull;
			before = incl - mult - (rs > 0 ? at_rs : 0ull);
		}
		if (EMIT) {
			const uint32_t kpos = (uint32_t)__shfl((int)(myoff + (uint32_t)run), (int)k, 64);
			if (act) ext_store<MAP>(a.map, kpos + (uint32_t)before, mult, first, (int32_t)(r0 + k), v, a.orow, a.ocol, a.oval);
		}
		run += own;
	}
	if (!EMIT && mine) a.cnt[r] = clamp_u32(run);
}

// Longer source rows: a workgroup of NT threads per listed output row (NT = 64: a wave)
template <int MAP, bool EMIT, int NT>
__global__ void __launch_bounds__(NT) k_ext_rows(ExtArgs a, const uint32_t *__restrict__ list)
{
	constexpr int NW = NT / 64;
	__shared__ unsigned long long s_w[2][NW];
	const uint32_t r = list[blockIdx.x];
	const uint32_t src = a.I ? (uint32_t)a.I[r] : r;
	const uint32_t beg = a.ptr[src], n = a.ptr[src + 1] - beg;
	const uint32_t off = EMIT ? (uint32_t)a.off[r] : 0u;
	uint64_t run = 0;
	int buf = 0;
	for (uint32_t base = 0; base < n; base += NT, buf ^= 1) {      // uniform
		const uint32_t i = base + threadIdx.x;
		const bool act = i < n;
		uint32_t mult = 0, first = 0;
		double v = 0;
		if (act) {
			mult = ext_mult<MAP>(a.map, a.col[beg + i], first);
			if (EMIT && mult) v = a.val[beg + i];
		}
		uint64_t excl, wtot;
		if (MAP != EXT_MAP_CSR) {
			const uint64_t m = __ballot(mult != 0);
			excl = (uint64_t)__popcll(m & lanemask_lt());
			wtot = (uint64_t)__popcll(m);
		} else {
			const unsigned long long incl = wave_inclusive_scan<unsigned long long>((unsigned long long)mult);
			excl = incl - mult;
			wtot = __shfl(incl, 63, 64);
		}
		uint64_t before = 0, tot = wtot;
		if (NW > 1) {
			if (lane_id() == 0) s_w[buf][wave_id()] = wtot;
			__syncthreads();
			tot = 0;
#pragma unroll
			for (int q = 0; q < NW; ++q) { const uint64_t t = s_w[buf][q]; before += (uint32_t)q < wave_id() ? t : 0ull; tot += t; }
		}
		if (EMIT && act) ext_store<MAP>(a.map, off + (uint32_t)(run + before + excl), mult, first, (int32_t)r, v, a.orow, a.ocol, a.oval);
		run += tot;
	}
	if (!EMIT && threadIdx.x == 0) a.cnt[r] = clamp_u32(run);
}

// ---------------------------------------------------------------- ordering the output rows (the permuted path)

// class of an output row of n >= 2 tuples: 0 light, 1 mid, 2 heavy (extract_path 2 / 3 / 4 forces a class wherever it can hold the row)
__device__ __forceinline__ int ext_class(uint32_t n, int path)
{
	if (path <= 2 && n <= (uint32_t)EXT_SHORT_MAX) return 0;
	if (path <= 3 && n <= (uint32_t)EXT_MID_MAX) return 1;
	return 2;
}

// w[0..2] rows per class, w[3..5] their tuples; the mid and heavy rows are listed (in no particular order), the heavy ones
// with their lengths.  Grid-stride: a wave keeps its light rows' counts in registers and adds them once at the end (one
// atomic per wave of 64 rows on two words took 6 ms for the 1.7e7 rows of a stencil matrix).
__global__ void __launch_bounds__(256) k_ext_classify(const uint32_t *__restrict__ cnt, uint64_t nR, int path, uint32_t *w,
	uint32_t *__restrict__ mid_list, uint32_t *__restrict__ heavy_list, uint32_t *__restrict__ heavy_len)
{
	uint32_t lrows = 0, ltup = 0;
	for (uint64_t r0 = (uint64_t)blockIdx.x * 256 + wave_id() * 64; r0 < nR; r0 += (uint64_t)gridDim.x * 256) {   // uniform
		const uint64_t r = r0 + lane_id();
		uint32_t n = 0;
		if (r < nR) n = cnt[r];
		const int cls = n >= 2 ? ext_class(n, path) : -1;
#pragma unroll
		for (int q = 0; q < 3; ++q) {
			const bool in = cls == q;
			const uint64_t m = __ballot(in);
			if (!m) continue;                                      // uniform
			const uint32_t tup = wave_reduce_sum<uint32_t>(in ? n : 0u);
			if (q == 0) { lrows += (uint32_t)__popcll(m); ltup += tup; continue; }
			const uint32_t slot = wave_claim(&w[q], in);
			if (lane_id() == 0) atomicAdd(&w[3 + q], tup);
			if (in && q == 1) mid_list[slot] = (uint32_t)r;
			if (in && q == 2) { heavy_list[slot] = (uint32_t)r; heavy_len[slot] = n; }
		}
	}
	if (lane_id() == 0 && lrows) { atomicAdd(&w[0], lrows); atomicAdd(&w[3], ltup); }
}

// Light rows: a wave takes 64 consecutive output rows and serves those of its class, a tuple per lane.  The place of a tuple
// is the number of tuples of a smaller column, or of the same column and emitted before it.  Rows of at most G = 8, 16 or 32
// tuples go 64 / G at a time, each in an aligned group of G lanes that exchange their columns by ds_bpermute (most light rows
// are short: a stencil's rows one at a time left 59 of 64 lanes idle); longer rows one at a time, by readlane broadcasts.
template <int G>
__device__ __forceinline__ void ext_sort_groups(uint64_t todo, uint32_t beg, uint32_t len, int32_t *ocol, double *oval)
{
	constexpr int NG = 64 / G;
	const int grp = (int)lane_id() / G, sub = (int)lane_id() % G;
	while (todo) {                                                 // uniform
		int mine = -1;                                             // the row of this lane's group: the next NG rows of `todo`
#pragma unroll
		for (int g = 0; g < NG; ++g) {
			const int l = todo ? __ffsll((unsigned long long)todo) - 1 : -1;
			if (todo) todo &= todo - 1ull;
			if (g == grp) mine = l;
		}
		const uint32_t b = (uint32_t)__shfl((int)beg, mine < 0 ? 0 : mine, 64);
		uint32_t n = (uint32_t)__shfl((int)len, mine < 0 ? 0 : mine, 64);
		if (mine < 0) n = 0;
		const bool have = (uint32_t)sub < n;
		int32_t c = 0;
		double v = 0;
		if (have) { c = ocol[b + sub]; v = oval[b + sub]; }
		uint32_t rank = 0;
#pragma unroll
		for (int j = 0; j < G; ++j) {
			const int32_t cj = __shfl(c, grp * G + j, 64);
			rank += ((uint32_t)j < n && (cj < c || (cj == c && j < sub))) ? 1u : 0u;
		}
		if (have) { ocol[b + rank] = c; oval[b + rank] = v; }      // (every lane's loads are done: one wave, program order)
	}
}

__global__ void __launch_bounds__(256) k_ext_sort_light(const uint32_t *__restrict__ cnt, const int64_t *__restrict__ off, uint64_t nR,
	int path, int32_t *ocol, double *oval)
{
	const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave_id()) * 64;
	if (r0 >= nR) return;
	const uint64_t r = r0 + lane_id();
	uint32_t beg = 0, len = 0;
	if (r < nR) { beg = (uint32_t)off[r]; len = cnt[r]; }
	const bool sel = len >= 2 && ext_class(len, path) == 0;
	ext_sort_groups<8>(__ballot(sel && len <= 8), beg, len, ocol, oval);
	ext_sort_groups<16>(__ballot(sel && len > 8 && len <= 16), beg, len, ocol, oval);
	ext_sort_groups<32>(__ballot(sel && len > 16 && len <= 32), beg, len, ocol, oval);
	uint64_t todo = __ballot(sel && len > 32);
	while (todo) {                                                 // uniform
		const int l = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
		todo &= todo - 1ull;
		const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)beg, l), n = (uint32_t)__builtin_amdgcn_readlane((int)len, l);
		const bool have = lane_id() < n;
		int32_t c = 0;
		double v = 0;
		if (have) { c = ocol[b + lane_id()]; v = oval[b + lane_id()]; }
		uint32_t rank = 0;
		for (uint32_t j = 0; j < n; ++j) {
			const int32_t cj = __builtin_amdgcn_readlane(c, (int)j);
			rank += (cj < c || (cj == c && j < lane_id())) ? 1u : 0u;
		}
		if (have) { ocol[b + rank] = c; oval[b + rank] = v; }
	}
}

// Mid rows: a workgroup per row; the keys column << 12 | emitted position sort in LDS (bitonic network over the next power of
// two, padded with all-ones keys), then every thread gathers its values by the sorted position before anyone stores.
__global__ void __launch_bounds__(EXT_MID_NT) k_ext_sort_mid(const uint32_t *__restrict__ list, const uint32_t *__restrict__ cnt,
	const int64_t *__restrict__ off, int32_t *ocol, double *oval)
{
	__shared__ uint64_t s_key[EXT_MID_MAX];
	const uint32_t r = list[blockIdx.x];
	const uint32_t b = (uint32_t)off[r], n = cnt[r];               // 2 <= n <= EXT_MID_MAX (ext_class)
	uint32_t P = 64;
	while (P < n) P <<= 1;
	for (uint32_t i = threadIdx.x; i < P; i += EXT_MID_NT)
		s_key[i] = i < n ? ((uint64_t)(uint32_t)ocol[b + i] << 12) | i : ~0ull;
	__syncthreads();
	for (uint32_t k = 2; k <= P; k <<= 1)
		for (uint32_t j = k >> 1; j > 0; j >>= 1) {
			for (uint32_t t = threadIdx.x; t < P / 2; t += EXT_MID_NT) {
				const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
				const uint64_t x = s_key[i], y = s_key[p];
				const bool up = (i & k) == 0;
				if ((x > y) == up) { s_key[i] = y; s_key[p] = x; }
			}
			__syncthreads();
		}
	double v[EXT_MID_MAX / EXT_MID_NT];
#pragma unroll
	for (int q = 0; q < EXT_MID_MAX / EXT_MID_NT; ++q) {
		const uint32_t i = threadIdx.x + (uint32_t)q * EXT_MID_NT;
		v[q] = i < n ? oval[b + (uint32_t)(s_key[i] & 4095u)] : 0.0;
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < EXT_MID_MAX / EXT_MID_NT; ++q) {
		const uint32_t i = threadIdx.x + (uint32_t)q * EXT_MID_NT;
		if (i < n) { oval[b + i] = v[q]; ocol[b + i] = (int32_t)(s_key[i] >> 12); }
	}
}

// Heavy rows: tuple i of listed row h is slot hoff[h] + i: its key (h << col_bits | column) and its place in the output
__global__ void __launch_bounds__(256) k_ext_heavy_keys(const uint32_t *__restrict__ list, const uint32_t *__restrict__ hoff,
	const uint32_t *__restrict__ cnt, const int64_t *__restrict__ off, const int32_t *__restrict__ ocol, int col_bits,
	uint64_t *__restrict__ keys, uint32_t *__restrict__ pos0)
{
	const uint32_t h = blockIdx.x, r = list[h];
	const uint32_t b = (uint32_t)off[r], n = cnt[r], s = hoff[h];
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		keys[s + i] = ((uint64_t)h << col_bits) | (uint64_t)(uint32_t)ocol[b + i];
		pos0[s + i] = b + i;
	}
}

// sorted slot i holds the tuple emitted at pos0[perm[i]] and belongs at pos0[i] (the sort keeps the rows in list order)
__global__ void __launch_bounds__(256) k_ext_heavy_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm,
	const uint32_t *__restrict__ pos0, const double *__restrict__ oval, uint32_t n, int col_bits, int32_t *__restrict__ tc, double *__restrict__ tv)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	tc[i] = (int32_t)(keys[i] & ((uint64_t(1) << col_bits) - 1));
	tv[i] = oval[pos0[perm[i]]];
}

__global__ void __launch_bounds__(256) k_ext_heavy_scatter(const int32_t *__restrict__ tc, const double *__restrict__ tv,
	const uint32_t *__restrict__ pos0, uint32_t n, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	ocol[pos0[i]] = tc[i];
	oval[pos0[i]] = tv[i];
}

template <int MAP, bool EMIT>
static void launch_kernels(spsamd_ctx *c, const ExtArgs &a, const uint32_t *long_list, uint32_t nlong, const uint32_t *huge_list, uint32_t nhuge)
{
	hipStream_t st = c->stream;
	k_ext_short<MAP, EMIT><<<dim3(grid_for(a.nR, 256)), dim3(256), 0, st>>>(a);
	SPS_LAUNCH_CHECK();
	if (nlong) { k_ext_rows<MAP, EMIT, EXT_LONG_NT><<<dim3(nlong), dim3(EXT_LONG_NT), 0, st>>>(a, long_list); SPS_LAUNCH_CHECK(); }
	if (nhuge) { k_ext_rows<MAP, EMIT, EXT_HUGE_NT><<<dim3(nhuge), dim3(EXT_HUGE_NT), 0, st>>>(a, huge_list); SPS_LAUNCH_CHECK(); }
}

template <bool EMIT>
static void launch_pass(spsamd_ctx *c, int map, const ExtArgs &a, const uint32_t *long_list, uint32_t nlong, const uint32_t *huge_list, uint32_t nhuge)
{
	if (map == EXT_MAP_ALL) launch_kernels<EXT_MAP_ALL, EMIT>(c, a, long_list, nlong, huge_list, nhuge);
	else if (map == EXT_MAP_INVERSE) launch_kernels<EXT_MAP_INVERSE, EMIT>(c, a, long_list, nlong, huge_list, nhuge);
	else launch_kernels<EXT_MAP_CSR, EMIT>(c, a, long_list, nlong, huge_list, nhuge);
}

// an index list must live where index_mem says: a device pointer handed in as host memory (or the reverse) would fault
static void check_list_pointer(const int32_t *p, int index_mem, const char *name)
{
	hipPointerAttribute_t at;
	int type = -1;                                                 // plain host memory: unknown to the runtime
	if (hipPointerGetAttributes(&at, p) == hipSuccess) type = (int)at.type;
	else (void)hipGetLastError();
	if (type == (int)hipMemoryTypeManaged) return;
	const bool device = type == (int)hipMemoryTypeDevice;
	if (device != (index_mem == SPSAMD_MEM_DEVICE))
		throw Error{SPSAMD_EINVAL, std::string(name) + (device ? " is a device pointer but index_mem says host" : " is not a device pointer but index_mem says device")};
}

void extract_tuples(spsamd_ctx *c, const spsamd_coo *A, char transpose, const int32_t *rows, size_t nrows, const int32_t *cols,
	size_t ncols, int index_mem, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	check_sink_args(duplicate_policy, sink_kind);
	if (index_mem != SPSAMD_MEM_HOST && index_mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "index_mem must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	if ((rows && nrows >= (size_t(1) << 31)) || (cols && ncols >= (size_t(1) << 31))) throw Error{SPSAMD_EINVAL, "an index list of 2^31 or more entries"};
	SPS_HIP(hipSetDevice(c->device));
	if (rows && nrows) check_list_pointer(rows, index_mem, "rows");
	if (cols && ncols) check_list_pointer(cols, index_mem, "cols");
	std::memset(res, 0, sizeof(*res));
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {A->shape0, A->shape1};
	const uint64_t nrowS = shape[lead], ncolS = shape[1 - lead];
	const uint64_t nR = rows ? nrows : nrowS, nC = cols ? ncols : ncolS;
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	const int path = c->tune.extract_path;
	res->shape0 = permute ? nC : nR;
	res->shape1 = permute ? nR : nC;

	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	if (coo) {
		const spsamd_coo *ops[1] = {A};
		pick_output_set(c, ops, 1);
		if (index_mem == SPSAMD_MEM_DEVICE && ((rows && nrows && c->out[c->cur_out].holds(rows)) || (cols && ncols && c->out[c->cur_out].holds(cols))))
			throw Error{SPSAMD_EINVAL, "an index list lies in the output set this call is about to write: copy it out first (spsamd_memcpy)"};
	}
	// is S known to be column-ordered inside its rows?  Consolidated here, chained or prepared: yes; trusted as stored: looked at
	const OperandView view = operand_view(c, A);
	const bool trusted = !(view.prep && view.prep->lead == lead) && view.coo.nnz > 0 && view.coo.sort0 == lead &&
		!(view.coo.mem == SPSAMD_MEM_DEVICE_VERIFIED || is_own_result(c, view.coo));
	ConMat S;
	Prepared *prep = nullptr;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S, &prep);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	const uint32_t n = S.nnz;
	res->nnz_a = n;

	// the lists: checked whatever the operand holds
	const int32_t *dI = rows ? to_device(c, rows, nR, index_mem) : nullptr;
	const int32_t *dJ = cols ? to_device(c, cols, nC, index_mem) : nullptr;
	uint32_t *w = get_zeroed<uint32_t>(c, 16);                     // [0..2] I, [3..5] J (k_ext_check), [6..7] source classes, [8..13] output classes
	int32_t *inv = nullptr;
	if (dI && nR) { k_ext_check<<<dim3(grid_for(nR)), dim3(256), 0, st>>>(dI, (uint32_t)nR, nrowS, nullptr, w); SPS_LAUNCH_CHECK(); }
	if (dJ && nC) {
		inv = c->arena.get<int32_t>(ncolS ? ncolS : 1);
		fill_u32(c, (uint32_t *)inv, 0xFFFFFFFFu, ncolS);
		k_ext_check<<<dim3(grid_for(nC)), dim3(256), 0, st>>>(dJ, (uint32_t)nC, ncolS, inv, w + 3);
		SPS_LAUNCH_CHECK();
	}
	const bool work = n && nR && nC;
	const uint32_t *ptr = nullptr;
	uint32_t *long_list = nullptr, *huge_list = nullptr;
	if (work) {
		ptr = prep && prep->rowptr ? prep->rowptr : dense_rowptr(c, S, 0);
		long_list = c->arena.get<uint32_t>(nR + 1); huge_list = c->arena.get<uint32_t>(nR + 1);
		k_ext_src_classify<<<dim3(grid_for(nR)), dim3(256), 0, st>>>(dI, nR, nrowS, ptr, w + 6, long_list, huge_list);
		SPS_LAUNCH_CHECK();
	}
	uint32_t h[8];
	{ WordList wl; for (int q = 0; q < 8; ++q) wl.add(w + q); read_back_words(c, wl, h); }
	for (int q = 0; q < 2; ++q)
		if (h[3 * q]) {
			char buf[160];
			std::snprintf(buf, sizeof buf, "%s[%u] is outside [0, %llu), the %s of op(A)", q ? "cols" : "rows", ~h[3 * q],
				(unsigned long long)(q ? ncolS : nrowS), q ? "columns" : "rows");
			throw Error{SPSAMD_EINVAL, buf};
		}
	if (!work) return;
	const bool j_ascending = !dJ || !h[4], j_repeats = dJ && h[5];
	const uint32_t nlong = h[6], nhuge = h[7];
	bool s_ordered = true;
	if (trusted && path == 0 && j_ascending) s_ordered = !(inspect_operand(c, S.row, S.col, S.val, n, nrowS, ncolS) & 32u);
	const bool in_order = path == 0 && j_ascending && s_ordered;

	ExtArgs a;
	std::memset(&a, 0, sizeof a);
	a.I = dI; a.nR = nR; a.ptr = ptr; a.col = S.col; a.val = S.val;
	int map = !dJ ? EXT_MAP_ALL : EXT_MAP_INVERSE;
	a.map.inv = inv;
	if (j_repeats) {                                               // J as a CSR by source column
		map = EXT_MAP_CSR;
		PairSort sort(c, nC);
		k_ext_list_keys<<<dim3(grid_for(nC)), dim3(256), 0, st>>>(dJ, (uint32_t)nC, sort.keys);
		SPS_LAUNCH_CHECK();
		sort.run(bits_of(ncolS));
		ConMat jm;
		jm.row = c->arena.get<int32_t>(nC); jm.nnz = (uint32_t)nC; jm.nrow = ncolS;
		k_ext_low32<<<dim3(grid_for(nC)), dim3(256), 0, st>>>(sort.keys, (uint32_t)nC, jm.row);
		SPS_LAUNCH_CHECK();
		a.map.jptr = dense_rowptr(c, jm, 0);
		a.map.jout = sort.perm;
	}

	// count, scan
	a.cnt = c->arena.get<uint32_t>(nR + 1);
	int64_t *off = c->arena.get<int64_t>(nR + 1);
	launch_pass<false>(c, map, a, long_list, nlong, huge_list, nhuge);
	scan_exclusive_u32_i64(c, a.cnt, off, nR);
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));
	const int64_t total64 = read_back(c, off + nR);
	if (total64 >= (int64_t(1) << 31)) {
		char buf[160];
		// (a single row beyond 2^32 - 1 tuples is counted as that many: the sum is then a lower bound)
		std::snprintf(buf, sizeof buf, "the result would hold %lld tuples: 2^31 or more (an index is named too many times)", (long long)total64);
		throw Error{SPSAMD_EINVAL, buf};
	}
	const uint32_t total = (uint32_t)total64;

	// emit
	const CooOut o = coo ? coo_output(c, total) : scratch_output(c, total);
	a.off = off; a.orow = o.row; a.ocol = o.col; a.oval = o.val;
	if (total) launch_pass<true>(c, map, a, long_list, nlong, huge_list, nhuge);

	// order the rows
	if (total && !in_order) {
		const size_t cap = (size_t)std::min<uint64_t>(nR, (uint64_t)total / 2 + 1);
		uint32_t *mid_list = c->arena.get<uint32_t>(cap + 1), *heavy_list = c->arena.get<uint32_t>(cap + 1), *heavy_len = c->arena.get<uint32_t>(cap + 1);
		k_ext_classify<<<dim3(std::min(grid_for(nR), 2048u)), dim3(256), 0, st>>>(a.cnt, nR, path, w + 8, mid_list, heavy_list, heavy_len);
		SPS_LAUNCH_CHECK();
		uint32_t g[6];
		{ WordList wl; for (int q = 0; q < 6; ++q) wl.add(w + 8 + q); read_back_words(c, wl, g); }
		const uint32_t nl = g[0], nm = g[1], nh = g[2], th = g[5];
		res->rows_light = nl; res->rows_mid = nm; res->rows_heavy = nh;
		res->tuples_light = g[3]; res->tuples_mid = g[4]; res->tuples_heavy = th;
		if (nl) { k_ext_sort_light<<<dim3(grid_for(nR, 256)), dim3(256), 0, st>>>(a.cnt, off, nR, path, o.col, o.val); SPS_LAUNCH_CHECK(); }
		if (nm) { k_ext_sort_mid<<<dim3(nm), dim3(EXT_MID_NT), 0, st>>>(mid_list, a.cnt, off, o.col, o.val); SPS_LAUNCH_CHECK(); }
		if (nh) {
			uint32_t *hoff = c->arena.get<uint32_t>((size_t)nh + 1);
			scan_exclusive_u32_u32(c, heavy_len, hoff, nh);
			const int cb = bits_of(nC);
			PairSort sort(c, th);
			uint32_t *pos0 = c->arena.get<uint32_t>(th);
			k_ext_heavy_keys<<<dim3(nh), dim3(256), 0, st>>>(heavy_list, hoff, a.cnt, off, o.col, cb, sort.keys, pos0);
			SPS_LAUNCH_CHECK();
			sort.run(cb + bits_of(nh));
			int32_t *tc = c->arena.get<int32_t>(th);
			double *tv = c->arena.get<double>(th);
			k_ext_heavy_gather<<<dim3(grid_for(th)), dim3(256), 0, st>>>(sort.keys, sort.perm, pos0, o.val, th, cb, tc, tv);
			SPS_LAUNCH_CHECK();
			k_ext_heavy_scatter<<<dim3(grid_for(th)), dim3(256), 0, st>>>(tc, tv, pos0, th, o.col, o.val);
			SPS_LAUNCH_CHECK();
		}
	}
	// row-major, every row in (c, p) order (read permuted: sorted by {1, 0}), indices checked
	deliver_stored(c, res, o, total, nR, coo, permute, sink_flags);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
}

} // namespace spsamd
