// k_select.hip -- keep the tuples of op(A) that a predicate names (spsamd_select, include/spsparse_amd.h).
//
// S = op(A) as consolidate_operand() hands it over (row-major; consolidated, or trusted as stored).  The result is a
// subsequence of S: no value is computed, so every kept value keeps its bits.
//
// Device path:
//   1. one byte per tuple of S, keep[t]:
//        TRIL .. ABS_GE   k_sel_flag: one streaming pass over the indices (or the values) that also counts;
//        ROW_REL          k_sel_rowmax (segmented integer max of mag over the non-NaN entries of each row), then k_sel_flag;
//        ROW_TOPK         rows with at most k tuples keep everything; the others go by length to
//                           k_sel_topk_light  n <= 64: a wave per row, rank by compare-all (readlane broadcast of every key),
//                           k_sel_topk_mid    n <= 4096: a workgroup per row, keys in LDS, MSD radix select of the k-th key,
//                           k_sel_topk_heavy  beyond: the same select, keys re-read from memory for every digit,
//                         then k_sel_count counts the bytes;
//   2. the shared compaction over wave tiles (devutil.h): k_sel_compact stores the kept tuples in S's order.
// mag(x) = the bits of x with the sign cleared, compared as an unsigned integer; no floating-point comparison decides.
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace spsamd {

constexpr int SEL_LIGHT_MAX = 64;              // longest row of the light class (one tuple per lane)
constexpr int SEL_MID_MAX = 4096;              // longest row of the mid class (keys in 32 KiB of LDS)
constexpr int SEL_MID_NT = 256;
constexpr int SEL_HEAVY_NT = 1024;
constexpr uint64_t SEL_INF = 0x7FF0000000000000ull;

struct SelArgs {
	const int32_t *row, *col;
	const double *val;
	uint32_t n;
	long long d;                               // structural predicates: the diagonal
	unsigned long long tmag;                   // ABS_GE: mag(theta)
	double theta;                              // ROW_REL
	const unsigned long long *rowmax;          // ROW_REL: mag of the largest non-NaN |v| per row
	int flip;                                  // COMPLEMENT
};

// keep[t] and the number of kept tuples per tile: the predicate is the `keep` of wave_tile_count, and stores its byte
template <int PRED>
__global__ void __launch_bounds__(256) k_sel_flag(SelArgs a, uint8_t *__restrict__ keep, uint32_t *__restrict__ tile_count)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	const uint64_t base = (uint64_t)tile * WAVE_TILE;
	if (base >= a.n) return;
	const uint32_t cnt = wave_tile_count(base, a.n, [&](uint64_t i) {
		bool k;
		if (PRED <= SPSAMD_SELECT_OFFDIAG) {
			const long long diff = (long long)a.col[i] - (long long)a.row[i];
			k = PRED == SPSAMD_SELECT_TRIL ? diff <= a.d : PRED == SPSAMD_SELECT_TRIU ? diff >= a.d :
				PRED == SPSAMD_SELECT_DIAG ? diff == a.d : diff != a.d;
		} else if (PRED == SPSAMD_SELECT_ABS_GE) k = mag_of(a.val[i]) >= a.tmag;
		else {
			const double t = a.theta * __longlong_as_double((long long)a.rowmax[a.row[i]]);
			k = mag_of(a.val[i]) >= mag_of(t);
		}
		k = k != (a.flip != 0);
		keep[i] = k ? 1 : 0;
		return k;
	});
	if (lane_id() == 0) tile_count[tile] = cnt;
}

__global__ void __launch_bounds__(256) k_sel_count(const uint8_t *__restrict__ keep, uint32_t n, uint32_t *__restrict__ tile_count)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	const uint64_t base = (uint64_t)tile * WAVE_TILE;
	if (base >= n) return;
	const uint32_t cnt = wave_tile_count(base, n, [&](uint64_t i) { return keep[i] != 0; });
	if (lane_id() == 0) tile_count[tile] = cnt;
}

__global__ void __launch_bounds__(256) k_sel_compact(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
	const double *__restrict__ val, uint32_t n, const uint8_t *__restrict__ keep, const uint32_t *__restrict__ tile_off,
	int32_t *__restrict__ orow, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	const uint64_t base = (uint64_t)tile * WAVE_TILE;
	if (base >= n) return;
	wave_range_compact(base, std::min<uint64_t>(base + WAVE_TILE, n), tile_off[tile], [&](uint64_t i) { return keep[i] != 0; },
		[&](uint64_t i, uint32_t p) { orow[p] = row[i]; ocol[p] = col[i]; oval[p] = val[i]; });
}

// rowmax[r] = max of mag(v) over the non-NaN entries of row r (the array starts at 0): a segmented max scan across the wave
// (the rows of S are runs), one atomic per run and wave.  An integer max: exact in any order.
__global__ void __launch_bounds__(256) k_sel_rowmax(const int32_t *__restrict__ row, const double *__restrict__ val, uint32_t n,
	unsigned long long *rowmax)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	int r = -1;
	unsigned long long m = 0;
	if (i < n) {
		r = row[i];
		const uint64_t x = mag_of(val[i]);
		if (x <= SEL_INF) m = x;
	}
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long om = __shfl_up(m, d, 64);
		const int orr = __shfl_up(r, d, 64);
		if ((int)lane_id() >= d && orr == r && om > m) m = om;
	}
	const int next = __shfl_down(r, 1, 64);
	if (i < n && (lane_id() == 63 || next != r) && m) atomicMax(&rowmax[r], m);
}

// ---------------------------------------------------------------- ROW_TOPK

// class of a row of n > k tuples: 0 light, 1 mid, 2 heavy (select_path forces a class wherever it can hold the row)
__device__ __forceinline__ int sel_class(uint32_t n, int path)
{
	if (path <= 1 && n <= (uint32_t)SEL_LIGHT_MAX) return 0;
	if (path <= 2 && n <= (uint32_t)SEL_MID_MAX) return 1;
	return 2;
}

// cnt[0..2] rows per class, cnt[3..5] their tuples; the mid and heavy rows are listed (in no particular order: every row
// is decided on its own)
__global__ void __launch_bounds__(256) k_sel_classify(const uint32_t *__restrict__ ptr, uint64_t nrow, uint32_t k, int path,
	uint32_t *cnt, uint32_t *__restrict__ mid_list, uint32_t *__restrict__ heavy_list)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t n = 0;
	if (r < nrow) n = ptr[r + 1] - ptr[r];
	const int cls = n > k ? sel_class(n, path) : -1;
#pragma unroll
	for (int q = 0; q < 3; ++q) {
		const bool in = cls == q;
		if (!__ballot(in)) continue;                               // uniform
		const uint32_t slot = wave_claim(&cnt[q], in);
		const uint32_t tup = wave_reduce_sum<uint32_t>(in ? n : 0u);
		if (lane_id() == 0) atomicAdd(&cnt[3 + q], tup);
		if (in && q > 0) (q == 1 ? mid_list : heavy_list)[slot] = (uint32_t)r;
	}
}

// Light rows: a wave takes 64 consecutive rows and serves those of its class one after the other, a tuple per lane.  The rank
// of a tuple in (mag descending, position ascending) is the number of tuples that come before it: every key is broadcast
// once (v_readlane) and compared by all lanes.
__global__ void __launch_bounds__(256) k_sel_topk_light(const uint32_t *__restrict__ ptr, uint64_t nrow, const double *__restrict__ val,
	uint32_t k, int path, int flip, uint8_t *__restrict__ keep)
{
	const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + wave_id()) * 64;
	if (r0 >= nrow) return;
	const uint64_t r = r0 + lane_id();
	uint32_t beg = 0, len = 0;
	if (r < nrow) { beg = ptr[r]; len = ptr[r + 1] - beg; }
	uint64_t todo = __ballot(len > k && sel_class(len, path) == 0);
	while (todo) {                                                 // uniform
		const int l = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
		todo &= todo - 1ull;
		const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)beg, l), n = (uint32_t)__builtin_amdgcn_readlane((int)len, l);
		const bool have = lane_id() < n;
		uint64_t key = 0;
		if (have) key = mag_of(val[b + lane_id()]);
		const int lo = (int)(uint32_t)key, hi = (int)(uint32_t)(key >> 32);
		uint32_t rank = 0;
		for (uint32_t j = 0; j < n; ++j) {
			const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, (int)j) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, (int)j);
			rank += (kj > key || (kj == key && j < lane_id())) ? 1u : 0u;
		}
		if (have) keep[b + lane_id()] = ((rank < k) != (flip != 0)) ? 1 : 0;
	}
}

// hist[digit] += 1 for every active lane, one LDS atomic per distinct digit of the wave (the top digits of doubles of one
// scale are all the same: 64 lanes on one counter would serialise).  Every lane of the wave must call it.
__device__ __forceinline__ void sel_hist_add(uint32_t *hist, uint32_t digit, bool active)
{
	uint64_t peers = __ballot(active);
#pragma unroll
	for (int b = 0; b < 8; ++b) {
		const bool bit = (digit >> b) & 1u;
		const uint64_t m = __ballot(active && bit);
		peers &= bit ? m : ~m;
	}
	if (active && (peers & lanemask_lt()) == 0) atomicAdd(&hist[digit], (uint32_t)__popcll(peers));
}

struct SelShared {
	uint32_t hist[256];
	uint32_t scan[SEL_HEAVY_NT / 64 + 1];
	uint32_t sel[3];
	uint32_t ties[2][SEL_HEAVY_NT / 64];
	unsigned long long tau;
};

// One row of n > k tuples by a workgroup of NT threads; key_at(i) = mag of its i-th tuple.  MSD radix select over the eight
// bytes of the key (the top bit is clear) for tau, the k-th key in descending order: per digit a histogram of the keys that
// share the digits found so far, a scan from the top bucket down, and the bucket that holds rank k; it stops when that bucket
// holds a single key or the digits run out.  Then one pass in storage order: a tuple stays if its key is above tau, or equals
// it and fewer than `q` equal keys precede it (q = k minus the keys above tau).
template <int NT, class KeyAt>
__device__ __forceinline__ void sel_row(KeyAt key_at, uint32_t n, uint32_t k, int flip, uint8_t *__restrict__ keep, SelShared &s)
{
	constexpr int NW = NT / 64;
	const uint32_t tid = threadIdx.x;
	uint64_t tau = ~0ull;                                          // k == 0: nothing is at or above it
	uint32_t q = 0;
	bool all_ties = true;
	if (k > 0) {
		uint64_t prefix = 0;
		uint32_t kk = k, cnt = 0;
		int shift = 56;
		for (;; shift -= 8) {
			for (uint32_t t = tid; t < 256; t += NT) s.hist[t] = 0;
			__syncthreads();
			for (uint32_t base = 0; base < n; base += NT) {        // uniform trip count
				const uint32_t i = base + tid;
				bool act = i < n;
				const uint64_t key = act ? key_at(i) : 0;
				if (shift < 56) act = act && (key >> (shift + 8)) == (prefix >> (shift + 8));
				sel_hist_add(s.hist, (uint32_t)(key >> shift) & 255u, act);
			}
			__syncthreads();
			const uint32_t c = tid < 256 ? s.hist[255 - tid] : 0u;     // buckets from the top down
			const uint32_t above = block_exclusive_scan<uint32_t, NT>(c, s.scan, nullptr);
			if (tid < 256 && above < kk && kk <= above + c) { s.sel[0] = 255 - tid; s.sel[1] = kk - above; s.sel[2] = c; }
			__syncthreads();
			prefix |= (uint64_t)s.sel[0] << shift;
			kk = s.sel[1]; cnt = s.sel[2];
			__syncthreads();
			if (cnt == 1 || shift == 0) break;
		}
		if (shift > 0) {                                           // the bucket's one key
			for (uint32_t i = tid; i < n; i += NT) {
				const uint64_t key = key_at(i);
				if ((key >> shift) == (prefix >> shift)) s.tau = key;
			}
			__syncthreads();
			prefix = s.tau;
		}
		tau = prefix; q = kk;
		all_ties = q == cnt;                                       // every key equal to tau stays: no order to establish
	}
	const bool fl = flip != 0;
	if (all_ties) {
		for (uint32_t i = tid; i < n; i += NT) keep[i] = ((key_at(i) >= tau) != fl) ? 1 : 0;
		return;
	}
	uint32_t run = 0;                                              // keys equal to tau before this chunk
	int buf = 0;
	for (uint32_t base = 0; base < n; base += NT, buf ^= 1) {
		const uint32_t i = base + tid;
		const bool act = i < n;
		const uint64_t key = act ? key_at(i) : 0;
		const bool tie = act && key == tau;
		const uint64_t m = __ballot(tie);
		if (lane_id() == 0) s.ties[buf][wave_id()] = (uint32_t)__popcll(m);
		__syncthreads();
		uint32_t before = run, tot = 0;
#pragma unroll
		for (int w = 0; w < NW; ++w) { const uint32_t t = s.ties[buf][w]; before += (uint32_t)w < wave_id() ? t : 0u; tot += t; }
		run += tot;
		if (act) keep[i] = ((key > tau || (tie && before + (uint32_t)__popcll(m & lanemask_lt()) < q)) != fl) ? 1 : 0;
	}
}

__global__ void __launch_bounds__(SEL_MID_NT) k_sel_topk_mid(const uint32_t *__restrict__ list, const uint32_t *__restrict__ ptr,
	const double *__restrict__ val, uint32_t k, int flip, uint8_t *__restrict__ keep)
{
	__shared__ uint64_t s_key[SEL_MID_MAX];
	__shared__ SelShared s;
	const uint32_t r = list[blockIdx.x];
	const uint32_t beg = ptr[r], n = ptr[r + 1] - beg;             // n <= SEL_MID_MAX (sel_class)
	for (uint32_t i = threadIdx.x; i < n; i += SEL_MID_NT) s_key[i] = mag_of(val[beg + i]);
	__syncthreads();
	sel_row<SEL_MID_NT>([&](uint32_t i) { return s_key[i]; }, n, k, flip, keep + beg, s);
}

__global__ void __launch_bounds__(SEL_HEAVY_NT) k_sel_topk_heavy(const uint32_t *__restrict__ list, const uint32_t *__restrict__ ptr,
	const double *__restrict__ val, uint32_t k, int flip, uint8_t *__restrict__ keep)
{
	__shared__ SelShared s;
	const uint32_t r = list[blockIdx.x];
	const uint32_t beg = ptr[r], n = ptr[r + 1] - beg;
	const double *v = val + beg;
	sel_row<SEL_HEAVY_NT>([&](uint32_t i) { return mag_of(v[i]); }, n, k, flip, keep + beg, s);
}

template <int PRED>
static void launch_flag(spsamd_ctx *c, const SelArgs &a, uint32_t ntiles, uint8_t *keep, uint32_t *tile_count)
{
	k_sel_flag<PRED><<<dim3(grid_for(ntiles, 4)), dim3(256), 0, c->stream>>>(a, keep, tile_count);
	SPS_LAUNCH_CHECK();
}

void select_tuples(spsamd_ctx *c, const spsamd_coo *A, char transpose, int predicate, int64_t iparam, double dparam,
	int select_flags, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (predicate < SPSAMD_SELECT_TRIL || predicate > SPSAMD_SELECT_ROW_TOPK) throw Error{SPSAMD_EINVAL, "unknown select predicate"};
	if (select_flags & ~SPSAMD_SELECT_COMPLEMENT) throw Error{SPSAMD_EINVAL, "unknown select_flags"};
	check_sink_args(duplicate_policy, sink_kind);
	if ((predicate == SPSAMD_SELECT_ABS_GE || predicate == SPSAMD_SELECT_ROW_REL) && !(dparam >= 0))
		throw Error{SPSAMD_EINVAL, "theta of a value predicate must be >= 0 and not NaN"};
	if (predicate == SPSAMD_SELECT_ROW_TOPK && iparam < 0) throw Error{SPSAMD_EINVAL, "k of ROW_TOPK must be >= 0"};
	std::memset(res, 0, sizeof(*res));
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {A->shape0, A->shape1};
	const uint64_t nrow = shape[lead], ncol = shape[1 - lead];
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	const int flip = (select_flags & SPSAMD_SELECT_COMPLEMENT) ? 1 : 0;
	res->shape0 = permute ? ncol : nrow;
	res->shape1 = permute ? nrow : ncol;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	if (coo) { const spsamd_coo *ops[1] = {A}; pick_output_set(c, ops, 1); }
	ConMat S;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	const uint32_t n = S.nnz;
	res->nnz_a = n;
	if (n == 0) return;

	const uint32_t ntiles = (uint32_t)(((uint64_t)n + WAVE_TILE - 1) / WAVE_TILE);
	uint8_t *keep = c->arena.get<uint8_t>((size_t)n + 8);
	uint32_t *tile_count = c->arena.get<uint32_t>((size_t)ntiles + 1), *tile_off = c->arena.get<uint32_t>((size_t)ntiles + 1);
	SelArgs a;
	a.row = S.row; a.col = S.col; a.val = S.val; a.n = n; a.d = (long long)iparam; a.theta = dparam; a.rowmax = nullptr; a.flip = flip;
	{ uint64_t b; std::memcpy(&b, &dparam, 8); a.tmag = b & 0x7FFFFFFFFFFFFFFFull; }
	switch (predicate) {
	case SPSAMD_SELECT_TRIL: launch_flag<SPSAMD_SELECT_TRIL>(c, a, ntiles, keep, tile_count); break;
	case SPSAMD_SELECT_TRIU: launch_flag<SPSAMD_SELECT_TRIU>(c, a, ntiles, keep, tile_count); break;
	case SPSAMD_SELECT_DIAG: launch_flag<SPSAMD_SELECT_DIAG>(c, a, ntiles, keep, tile_count); break;
	case SPSAMD_SELECT_OFFDIAG: launch_flag<SPSAMD_SELECT_OFFDIAG>(c, a, ntiles, keep, tile_count); break;
	case SPSAMD_SELECT_ABS_GE: launch_flag<SPSAMD_SELECT_ABS_GE>(c, a, ntiles, keep, tile_count); break;
	case SPSAMD_SELECT_ROW_REL: {
		unsigned long long *rowmax = c->arena.get<unsigned long long>(nrow ? nrow : 1);
		fill_zero(c, rowmax, nrow * sizeof(unsigned long long));
		k_sel_rowmax<<<dim3(grid_for(n)), dim3(256), 0, st>>>(S.row, S.val, n, rowmax);
		SPS_LAUNCH_CHECK();
		a.rowmax = rowmax;
		launch_flag<SPSAMD_SELECT_ROW_REL>(c, a, ntiles, keep, tile_count);
		break;
	}
	default: {
		const uint32_t k = (uint32_t)std::min<int64_t>(iparam, 0x7FFFFFFF);
		const int path = c->tune.select_path;
		const uint32_t *ptr = dense_rowptr(c, S, 0);
		SPS_HIP(hipMemsetAsync(keep, flip ? 0 : 1, n, st));              // rows of at most k tuples stay whole
		const size_t cap = (size_t)std::min<uint64_t>(nrow, n);
		uint32_t *cnt = c->arena.get<uint32_t>(8), *mid_list = c->arena.get<uint32_t>(cap + 1), *heavy_list = c->arena.get<uint32_t>(cap + 1);
		fill_zero(c, cnt, 8 * sizeof(uint32_t));
		k_sel_classify<<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(ptr, nrow, k, path, cnt, mid_list, heavy_list);
		SPS_LAUNCH_CHECK();
		uint32_t *h = (uint32_t *)c->host_staging(8 * sizeof(uint32_t));
		SPS_HIP(hipMemcpyAsync(h, cnt, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
		const uint32_t nl = h[0], nm = h[1], nh = h[2];
		res->rows_light = nl; res->rows_mid = nm; res->rows_heavy = nh;
		res->tuples_light = h[3]; res->tuples_mid = h[4]; res->tuples_heavy = h[5];
		if (nl) { k_sel_topk_light<<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(ptr, nrow, S.val, k, path, flip, keep); SPS_LAUNCH_CHECK(); }
		if (nm) { k_sel_topk_mid<<<dim3(nm), dim3(SEL_MID_NT), 0, st>>>(mid_list, ptr, S.val, k, flip, keep); SPS_LAUNCH_CHECK(); }
		if (nh) { k_sel_topk_heavy<<<dim3(nh), dim3(SEL_HEAVY_NT), 0, st>>>(heavy_list, ptr, S.val, k, flip, keep); SPS_LAUNCH_CHECK(); }
		k_sel_count<<<dim3(grid_for(ntiles, 4)), dim3(256), 0, st>>>(keep, n, tile_count);
		SPS_LAUNCH_CHECK();
		break;
	}
	}
	uint32_t total;
	const CooOut o = counted_output(c, tile_count, tile_off, ntiles, coo, &total);
	if (total) {
		k_sel_compact<<<dim3(grid_for(ntiles, 4)), dim3(256), 0, st>>>(S.row, S.col, S.val, n, keep, tile_off, o.row, o.col, o.val);
		SPS_LAUNCH_CHECK();
	}
	// a subsequence of S: in op(A)'s row order (read permuted: sorted by {1, 0}), indices checked
	deliver_stored(c, res, o, total, nrow, coo, permute, sink_flags);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_CONSOLIDATED], c->ev[EV_END]));
}

} // namespace spsamd
