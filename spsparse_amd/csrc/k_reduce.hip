// k_reduce.hip -- row reductions of op(A) into a vector (spsamd_reduce, include/spsparse_amd.h).
//
// S = op(A) as consolidate_operand() hands it over (row-major; consolidated, or trusted as stored).  r_i is a SERIAL fold over
// the tuples of row i in S's order -- every add and multiply rounded on its own, a NaN result with x86's bits (x86fp.h) -- so
// no tree sum: a lane owns a row and walks it front to back, and the kernels' work is feeding 64 such chains per wave with
// coalesced loads.
//
// Device path:
//   1. k_red_classify counts the non-empty rows by class (short: at most RED_LIGHT_MAX tuples; long: the others) and, for the
//      long rows, by length bin (2^(b-1) < len <= 2^b); a second launch lists the long rows bin by bin, longest first.
//   2. k_red_short: a wave takes 64 consecutive rows.  Their tuples are one contiguous span of S: it is walked in chunks of
//      RED_SPAN values, loaded packed and coalesced into the wave's LDS; each lane then folds the part of its own row that lies
//      in the chunk.  A chunk starts at the first tuple still to be folded, so the long rows between short ones are jumped
//      over.  The same kernel is correct for rows of any length (reduce_path 1).
//   3. k_red_long: a wave takes 64 listed rows of similar length.  Per step every row contributes one chunk of RED_CHUNK
//      consecutive values, loaded by half a wave (256 contiguous bytes) into a padded [row][RED_CHUNK + 1] LDS tile; each lane
//      folds its row's chunk while the next step's loads are in flight (they are issued into registers ahead of the adds).
//   4. both kernels apply the post-operation and store dense: out_val itself (dense form, device memory) or a workspace
//      array.  The sparse form runs one more pass over the ROWS: k_red_tile_count, a scan, k_red_compact (the shared
//      compaction over wave tiles, devutil.h).
// COUNT reads the row pointer only (k_red_rowcount).  MAX_ABS goes through the same two kernels with an integer max on mag.
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

constexpr int RED_LIGHT_MAX = 64;              // longest row of the short class
constexpr int RED_SPAN = 512;                  // values a wave of k_red_short stages per step (8 per lane)
constexpr int RED_CHUNK = 32;                  // values per row and step of k_red_long
constexpr uint64_t RED_INF = 0x7FF0000000000000ull;

struct RedArgs {
	const uint32_t *ptr;                       // dense row pointer of S
	const int32_t *col;                        // DIAG only
	const double *val;
	uint64_t nrow;
	int path, post;
	double *dval;                              // post(r_i) per row, +0.0 where nothing contributes
	uint8_t *has;                              // DIAG: does the row have a diagonal tuple
	uint32_t *nz;                              // DIAG: the number of such rows
};

// the LDS of these kernels is private to a wave, whose DS operations execute in order: only the compiler has to be held
__device__ __forceinline__ void wave_lds_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one step of the fold; the accumulator is the left operand
template <int OP>
__device__ __forceinline__ double red_step(double acc, double v, bool on_diag, bool &has)
{
	if (OP == SPSAMD_REDUCE_SUM) return ref_add(acc, v);
	if (OP == SPSAMD_REDUCE_SUM_ABS) return ref_add(acc, __longlong_as_double((long long)mag_of(v)));
	if (OP == SPSAMD_REDUCE_SUM_SQ) return ref_add(acc, ref_mul(v, v));
	if (OP == SPSAMD_REDUCE_MAX_ABS) {
		const uint64_t x = mag_of(v);
		return (x <= RED_INF && x > (uint64_t)__double_as_longlong(acc)) ? __longlong_as_double((long long)x) : acc;
	}
	if (on_diag) { has = true; return ref_add(acc, v); }
	return acc;
}

__device__ __forceinline__ double red_recip(double r) { return r != r ? quiet(r) : __ddiv_rn(1.0, r); }
__device__ __forceinline__ double red_sqrt(double r) { return ref_sqrt(r); }
__device__ __forceinline__ double red_post(double r, int post)
{
	if (post == SPSAMD_POST_RECIP) return red_recip(r);
	if (post == SPSAMD_POST_SQRT) return red_sqrt(r);
	if (post == SPSAMD_POST_RSQRT) return red_recip(red_sqrt(r));
	return r;
}

// what a row kernel leaves for row r (every lane of the wave calls it)
template <int OP>
__device__ __forceinline__ void red_store(const RedArgs &a, uint64_t r, bool store, bool has, double acc)
{
	if (store) {
		a.dval[r] = has ? red_post(acc, a.post) : 0.0;
		if (OP == SPSAMD_REDUCE_DIAG) a.has[r] = has ? 1 : 0;
	}
	if (OP == SPSAMD_REDUCE_DIAG) {
		const uint64_t m = __ballot(store && has);
		if (m && lane_id() == 0) atomicAdd(a.nz, (uint32_t)__popcll(m));
	}
}

__device__ __forceinline__ bool red_is_long(uint32_t n, int path) { return n > 0 && (path == 2 || (path == 0 && n > (uint32_t)RED_LIGHT_MAX)); }
__device__ __forceinline__ int red_bin(uint32_t n) { return n <= 1 ? 0 : 32 - __clz((int)(n - 1)); }      // 2^(b-1) < n <= 2^b

// FILL = false: cnt[0] short rows, cnt[1] long rows, cnt[2] / cnt[3] their tuples, bins[b] long rows per length bin.
// FILL = true: bins[] holds each bin's cursor into `list`; the long rows are listed (inside a bin in no particular order).
template <bool FILL>
__global__ void __launch_bounds__(256) k_red_classify(const uint32_t *__restrict__ ptr, uint64_t nrow, int path, uint32_t *cnt,
	uint32_t *bins, uint32_t *__restrict__ list)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t n = 0;
	if (r < nrow) n = ptr[r + 1] - ptr[r];
	const bool lng = red_is_long(n, path);
	if (!FILL) {
		const bool sht = n > 0 && !lng;
		const uint64_t ms = __ballot(sht), ml = __ballot(lng);
		if (ms) {                                                  // uniform
			const uint32_t t = wave_reduce_sum<uint32_t>(sht ? n : 0u);
			if (lane_id() == 0) { atomicAdd(&cnt[0], (uint32_t)__popcll(ms)); atomicAdd(&cnt[2], t); }
		}
		if (ml) {
			const uint32_t t = wave_reduce_sum<uint32_t>(lng ? n : 0u);
			if (lane_id() == 0) { atomicAdd(&cnt[1], (uint32_t)__popcll(ml)); atomicAdd(&cnt[3], t); }
		}
	}
	const int b = red_bin(n);
	uint64_t todo = __ballot(lng);
	while (todo) {                                                 // uniform
		const int l = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)todo) - 1);
		const int bb = __builtin_amdgcn_readlane(b, l);
		const bool in = lng && b == bb;
		todo &= ~__ballot(in);
		const uint32_t slot = wave_claim(&bins[bb], in);           // (FILL = false: counted only)
		if (FILL && in) list[slot] = (uint32_t)r;
	}
}

// bins[b] = the rows in longer bins: the list starts with the longest rows
__global__ void __launch_bounds__(64) k_red_binscan(uint32_t *bins)
{
	const uint32_t lane = lane_id();
	const uint32_t v = lane < 32 ? bins[31 - lane] : 0u;
	const uint32_t incl = wave_inclusive_scan_u32(v);
	if (lane < 32) bins[31 - lane] = incl - v;
}

// Short rows (and, under reduce_path 1, every row): see the head of the file.
template <int OP>
__global__ void __launch_bounds__(256) k_red_short(RedArgs a)
{
	constexpr bool DIAG = OP == SPSAMD_REDUCE_DIAG;
	__shared__ double s_val[4][RED_SPAN];
	__shared__ int32_t s_col[4][DIAG ? RED_SPAN : 1];
	const uint32_t w = wave_id(), lane = lane_id();
	const uint64_t r0 = ((uint64_t)blockIdx.x * 4 + w) * 64;
	if (r0 >= a.nrow) return;                                      // (no workgroup barrier below)
	const uint64_t r = r0 + lane;
	const bool inrange = r < a.nrow;
	uint32_t beg = 0, end = 0;
	if (inrange) { beg = a.ptr[r]; end = a.ptr[r + 1]; }
	const uint32_t len = end - beg;
	const bool mine = len > 0 && !red_is_long(len, a.path);        // (a long row is k_red_long's)
	double acc = 0.0;
	bool has = false;
	const uint64_t mm = __ballot(mine);
	if (mm) {                                                      // uniform
		const uint32_t span_end = (uint32_t)__builtin_amdgcn_readlane((int)end, __builtin_amdgcn_readfirstlane(63 - __clzll((long long)mm)));
		uint32_t pos = beg;                                        // the next tuple of this lane's row
		for (;;) {
			const uint64_t m = __ballot(mine && pos < end);
			if (!m) break;                                         // uniform
			// the rows ascend with the lane: the first unfinished lane holds the lowest position still to be folded
			const uint32_t cb = (uint32_t)__builtin_amdgcn_readlane((int)pos, __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1));
			const uint32_t cend = std::min(cb + (uint32_t)RED_SPAN, span_end);
			// (every load is issued before the first LDS store; a slot past the chunk's end repeats its last tuple: cend > cb)
			double lv[RED_SPAN / 64];
			int32_t lc[DIAG ? RED_SPAN / 64 : 1];
#pragma unroll
			for (int k = 0; k < RED_SPAN / 64; ++k) {
				const uint32_t i = std::min(cb + (uint32_t)k * 64 + lane, cend - 1);
				lv[k] = a.val[i];
				if (DIAG) lc[DIAG ? k : 0] = a.col[i];
			}
#pragma unroll
			for (int k = 0; k < RED_SPAN / 64; ++k) {
				s_val[w][k * 64 + lane] = lv[k];
				if (DIAG) s_col[w][k * 64 + lane] = lc[DIAG ? k : 0];
			}
			wave_lds_sync();
			const uint32_t stop = std::min(end, cend);
			if (mine) {
				for (; pos < stop; ++pos) {
					const bool d = DIAG && s_col[w][DIAG ? pos - cb : 0] == (int32_t)r;
					acc = red_step<OP>(acc, s_val[w][pos - cb], d, has);
				}
			}
			wave_lds_sync();
		}
	}
	if (!DIAG) has = mine;
	red_store<OP>(a, r, inrange && (mine || len == 0), has, acc);
}

// Long rows (and, under reduce_path 2, every non-empty row): see the head of the file.
template <int OP>
__global__ void __launch_bounds__(64) k_red_long(RedArgs a, const uint32_t *__restrict__ list, uint32_t nlist)
{
	constexpr bool DIAG = OP == SPSAMD_REDUCE_DIAG;
	constexpr int NI = RED_CHUNK;                                  // load rounds per step: two rows each, 32 lanes per row
	static_assert(RED_CHUNK == 32, "half a wave loads one row's chunk");
	__shared__ double s_val[64][RED_CHUNK + 1];
	__shared__ int32_t s_col[DIAG ? 64 : 1][RED_CHUNK + 1];
	const uint32_t lane = lane_id();
	const uint32_t e = blockIdx.x * 64 + lane;
	uint32_t r = 0, beg = 0, len = 0;
	if (e < nlist) { r = list[e]; beg = a.ptr[r]; len = a.ptr[r + 1] - beg; }
	uint32_t maxlen = len;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) maxlen = std::max(maxlen, (uint32_t)__shfl_xor((int)maxlen, d, 64));
	const uint32_t nsteps = (maxlen + RED_CHUNK - 1) / RED_CHUNK;
	// round i of a step: this lane loads value `o` of the chunk of the wave's row 2 * i + (lane >> 5)
	const uint32_t o = lane & 31u, half = lane >> 5;
	uint32_t qpos[NI], qlen[NI];
#pragma unroll
	for (int i = 0; i < NI; ++i) {
		qpos[i] = (uint32_t)__shfl((int)beg, 2 * i + (int)half, 64) + o;
		qlen[i] = (uint32_t)__shfl((int)len, 2 * i + (int)half, 64);
	}
	double pv[NI] = {};                                            // (a slot past its row's end is stored to the tile, never folded)
	int32_t pc[DIAG ? NI : 1] = {};
	auto load = [&](uint32_t step) {
#pragma unroll
		for (int i = 0; i < NI; ++i) {
			const uint32_t at = step * RED_CHUNK + o;
			if (at < qlen[i]) {
				pv[i] = a.val[qpos[i] + step * RED_CHUNK];
				if (DIAG) pc[DIAG ? i : 0] = a.col[qpos[i] + step * RED_CHUNK];
			}
		}
	};
	double acc = 0.0;
	bool has = false;
	if (nsteps) load(0);
	for (uint32_t step = 0; step < nsteps; ++step) {               // uniform
#pragma unroll
		for (int i = 0; i < NI; ++i) {
			s_val[2 * i + half][o] = pv[i];
			if (DIAG) s_col[DIAG ? 2 * i + half : 0][o] = pc[DIAG ? i : 0];
		}
		wave_lds_sync();
		if (step + 1 < nsteps) load(step + 1);                     // in flight during the adds
		const uint32_t done = step * RED_CHUNK;
		const uint32_t cnt = len > done ? std::min(len - done, (uint32_t)RED_CHUNK) : 0u;
		for (uint32_t k = 0; k < cnt; ++k) {
			const bool d = DIAG && s_col[DIAG ? lane : 0][k] == (int32_t)r;
			acc = red_step<OP>(acc, s_val[lane][k], d, has);
		}
		wave_lds_sync();
	}
	if (!DIAG) has = len > 0;
	red_store<OP>(a, r, e < nlist, has, acc);
}

// COUNT: the row pointer alone
__global__ void __launch_bounds__(256) k_red_rowcount(RedArgs a)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= a.nrow) return;
	const uint32_t n = a.ptr[r + 1] - a.ptr[r];
	a.dval[r] = n ? red_post((double)n, a.post) : 0.0;
}

__device__ __forceinline__ bool red_present(const uint32_t *ptr, const uint8_t *has, uint64_t r) { return has ? has[r] != 0 : ptr[r + 1] > ptr[r]; }

__global__ void __launch_bounds__(256) k_red_tile_count(const uint32_t *__restrict__ ptr, const uint8_t *__restrict__ has, uint64_t nrow,
	uint32_t *__restrict__ tile_count)
{
	const uint64_t tile = (uint64_t)blockIdx.x * 4 + wave_id();
	const uint64_t base = tile * WAVE_TILE;
	if (base >= nrow) return;
	const uint32_t cnt = wave_tile_count(base, nrow, [&](uint64_t r) { return red_present(ptr, has, r); });
	if (lane_id() == 0) tile_count[tile] = cnt;
}

__global__ void __launch_bounds__(256) k_red_compact(const uint32_t *__restrict__ ptr, const uint8_t *__restrict__ has, uint64_t nrow,
	const double *__restrict__ dval, const uint32_t *__restrict__ tile_off, int32_t *__restrict__ oidx, double *__restrict__ oval)
{
	const uint64_t tile = (uint64_t)blockIdx.x * 4 + wave_id();
	const uint64_t base = tile * WAVE_TILE;
	if (base >= nrow) return;
	wave_range_compact(base, std::min<uint64_t>(base + WAVE_TILE, nrow), tile_off[tile], [&](uint64_t r) { return red_present(ptr, has, r); },
		[&](uint64_t r, uint32_t at) { oidx[at] = (int32_t)r; oval[at] = dval[r]; });
}

template <int OP>
static void launch_short(spsamd_ctx *c, const RedArgs &a)
{
	k_red_short<OP><<<dim3(grid_for(a.nrow, 256)), dim3(256), 0, c->stream>>>(a);
	SPS_LAUNCH_CHECK();
}

template <int OP>
static void launch_long(spsamd_ctx *c, const RedArgs &a, const uint32_t *list, uint32_t nlist)
{
	k_red_long<OP><<<dim3(grid_for(nlist, 64)), dim3(64), 0, c->stream>>>(a, list, nlist);
	SPS_LAUNCH_CHECK();
}

static void run_short(spsamd_ctx *c, int op, const RedArgs &a)
{
	switch (op) {
	case SPSAMD_REDUCE_SUM: launch_short<SPSAMD_REDUCE_SUM>(c, a); break;
	case SPSAMD_REDUCE_SUM_ABS: launch_short<SPSAMD_REDUCE_SUM_ABS>(c, a); break;
	case SPSAMD_REDUCE_SUM_SQ: launch_short<SPSAMD_REDUCE_SUM_SQ>(c, a); break;
	case SPSAMD_REDUCE_MAX_ABS: launch_short<SPSAMD_REDUCE_MAX_ABS>(c, a); break;
	default: launch_short<SPSAMD_REDUCE_DIAG>(c, a); break;
	}
}

static void run_long(spsamd_ctx *c, int op, const RedArgs &a, const uint32_t *list, uint32_t nlist)
{
	switch (op) {
	case SPSAMD_REDUCE_SUM: launch_long<SPSAMD_REDUCE_SUM>(c, a, list, nlist); break;
	case SPSAMD_REDUCE_SUM_ABS: launch_long<SPSAMD_REDUCE_SUM_ABS>(c, a, list, nlist); break;
	case SPSAMD_REDUCE_SUM_SQ: launch_long<SPSAMD_REDUCE_SUM_SQ>(c, a, list, nlist); break;
	case SPSAMD_REDUCE_MAX_ABS: launch_long<SPSAMD_REDUCE_MAX_ABS>(c, a, list, nlist); break;
	default: launch_long<SPSAMD_REDUCE_DIAG>(c, a, list, nlist); break;
	}
}

bool ranges_overlap(const void *p, uint64_t np, const void *q, uint64_t nq)
{
	return p && q && np && nq && (const char *)p < (const char *)q + nq && (const char *)q < (const char *)p + np;
}

bool in_output_sets(const spsamd_ctx *c, const void *p, uint64_t bytes)
{
	if (!p || !bytes) return false;
	for (const auto &s : c->out) if (s.holds(p) || s.holds((const char *)p + bytes - 1)) return true;
	return false;
}

// The folds of reduce_rows in two steps, shared with reduce_diag_dense.  ctr: 40 zeroed words ([0..3] the classes, [4] DIAG's
// rows, [8..39] the bins).  Step one counts the rows by class, folds the short rows (under reduce_path 2 there are none:
// the dense result and DIAG's marks are zeroed instead) unless the caller defers that until it has seen the counters, and
// brings the first eight counters to h.
static void fold_short_rows(spsamd_ctx *c, int op, const RedArgs &a, uint32_t *ctr, uint32_t *h, bool zero_dense, bool defer_short)
{
	hipStream_t st = c->stream;
	k_red_classify<false><<<dim3(grid_for(a.nrow)), dim3(256), 0, st>>>(a.ptr, a.nrow, a.path, ctr, ctr + 8, nullptr);
	SPS_LAUNCH_CHECK();
	if (a.path == 2) {
		if (zero_dense) fill_zero(c, a.dval, a.nrow * sizeof(double));
		if (op == SPSAMD_REDUCE_DIAG) fill_zero(c, a.has, a.nrow);
	} else if (!defer_short) run_short(c, op, a);
	SPS_HIP(hipMemcpyAsync(h, ctr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipStreamSynchronize(st));
}

// Step two: the nlong (= h[1]) long rows listed bin by bin, longest first, and folded.
static void fold_long_rows(spsamd_ctx *c, int op, const RedArgs &a, uint32_t *ctr, uint32_t nlong)
{
	if (!nlong) return;
	hipStream_t st = c->stream;
	uint32_t *list = c->arena.get<uint32_t>((size_t)nlong + 1);
	k_red_binscan<<<dim3(1), dim3(64), 0, st>>>(ctr + 8);
	SPS_LAUNCH_CHECK();
	k_red_classify<true><<<dim3(grid_for(a.nrow)), dim3(256), 0, st>>>(a.ptr, a.nrow, a.path, ctr, ctr + 8, list);
	SPS_LAUNCH_CHECK();
	run_long(c, op, a, list, nlong);
}

// (declared in internal.h: spsamd_solve_pcg's Jacobi preconditioner) the DIAG fold of a taken operand, dense, by the two
// steps above: d[i] = +0.0 and then every diagonal tuple of row i added in S's order
void reduce_diag_dense(spsamd_ctx *c, const uint32_t *ptr, const int32_t *col, const double *val, uint64_t nrow, double *d)
{
	RedArgs a;
	a.ptr = ptr; a.col = col; a.val = val; a.nrow = nrow; a.post = SPSAMD_POST_NONE;
	a.path = c->tune.reduce_path == 1 || c->tune.reduce_path == 2 ? c->tune.reduce_path : 0;
	a.dval = d;
	a.has = c->arena.get<uint8_t>(nrow + 8);
	uint32_t *ctr = get_zeroed<uint32_t>(c, 40);
	a.nz = ctr + 4;
	uint32_t *h = (uint32_t *)c->host_staging(8 * sizeof(uint32_t));
	fold_short_rows(c, SPSAMD_REDUCE_DIAG, a, ctr, h, true, false);
	fold_long_rows(c, SPSAMD_REDUCE_DIAG, a, ctr, h[1]);
}

int reduce_rows(spsamd_ctx *c, const spsamd_coo *A, char transpose, int op, int post, int duplicate_policy, int zero_nan,
	int32_t *out_idx, double *out_val, size_t capacity, int mem, size_t *out_nnz, spsamd_result *res)
{
	if (op < SPSAMD_REDUCE_SUM || op > SPSAMD_REDUCE_DIAG) throw Error{SPSAMD_EINVAL, "unknown reduce op"};
	if (post < SPSAMD_POST_NONE || post > SPSAMD_POST_RSQRT) throw Error{SPSAMD_EINVAL, "unknown post-operation"};
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of the output must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {A->shape0, A->shape1};
	const uint64_t nrow = shape[lead];
	const bool sparse = out_idx != nullptr, diag = op == SPSAMD_REDUCE_DIAG;
	{
		const OperandView view = operand_view(c, A);
		const uint64_t n = view.coo.nnz;
		const uint64_t ibytes = sparse ? (uint64_t)capacity * 4 : 0, vbytes = (sparse ? (uint64_t)capacity : nrow) * 8;
		if (ranges_overlap(out_idx, ibytes, out_val, vbytes)) throw Error{SPSAMD_EINVAL, "out_idx and out_val overlap"};
		const void *arr[3] = {view.coo.idx0, view.coo.idx1, view.coo.val};
		for (int k = 0; k < 3; ++k)
			if (ranges_overlap(out_idx, ibytes, arr[k], n * (k == 2 ? 8 : 4)) || ranges_overlap(out_val, vbytes, arr[k], n * (k == 2 ? 8 : 4)))
				throw Error{SPSAMD_EINVAL, "an output buffer overlaps A's arrays"};
		if (mem == SPSAMD_MEM_DEVICE && (in_output_sets(c, out_idx, ibytes) || in_output_sets(c, out_val, vbytes)))
			throw Error{SPSAMD_EINVAL, "an output buffer lies in an output set of the context"};
	}
	std::memset(res, 0, sizeof(*res));
	res->shape0 = nrow;
	if (!sparse && capacity < nrow) {
		*out_nnz = nrow;
		c->last_error = "out_val is too small for the dense form: it needs one entry per row of op(A)";
		return SPSAMD_ECAPACITY;
	}

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	ConMat S;
	Prepared *hp = nullptr;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S, &hp);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	const uint32_t n = S.nnz;
	res->nnz_a = n;
	*out_nnz = 0;
	if (n == 0 || nrow == 0) {
		if (!sparse && nrow) {
			if (mem == SPSAMD_MEM_HOST) std::memset(out_val, 0, nrow * sizeof(double));
			else { fill_zero(c, out_val, nrow * sizeof(double)); SPS_HIP(hipStreamSynchronize(st)); }
		}
		return SPSAMD_OK;
	}

	const uint32_t *ptr;
	if (hp) { prepared_row_structure(c, hp); ptr = hp->rowptr; }
	else ptr = dense_rowptr(c, S, 0);
	const int path = c->tune.reduce_path == 1 || c->tune.reduce_path == 2 ? c->tune.reduce_path : 0;
	const bool direct = !sparse && mem == SPSAMD_MEM_DEVICE;           // the kernels store into out_val itself
	RedArgs a;
	a.ptr = ptr; a.col = S.col; a.val = S.val; a.nrow = nrow; a.path = path; a.post = post;
	a.dval = direct ? out_val : c->arena.get<double>(nrow);
	a.has = diag ? c->arena.get<uint8_t>(nrow + 8) : nullptr;
	uint32_t *ctr = get_zeroed<uint32_t>(c, 40);                      // [0..3] the classes, [4] DIAG's rows, [8..39] the bins
	a.nz = ctr + 4;
	uint32_t *h = (uint32_t *)c->host_staging(8 * sizeof(uint32_t));
	auto read_counters = [&]() {
		SPS_HIP(hipMemcpyAsync(h, ctr, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
	};
	auto too_small = [&](uint64_t count) {
		*out_nnz = count;
		c->last_error = "the output buffers are too small: *out_nnz holds the number of entries";
		return SPSAMD_ECAPACITY;
	};

	uint64_t count = 0;
	if (op == SPSAMD_REDUCE_COUNT) {
		k_red_classify<false><<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(ptr, nrow, path, ctr, ctr + 8, nullptr);
		SPS_LAUNCH_CHECK();
		k_red_rowcount<<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(a);
		SPS_LAUNCH_CHECK();
		read_counters();
		count = (uint64_t)h[0] + h[1];
		if (sparse && capacity < count) return too_small(count);
	} else {
		// the size of a sparse result is known before any fold, except DIAG's; elsewhere the short rows' kernel runs
		// while the host waits for the counters
		const bool early = sparse && !diag;
		fold_short_rows(c, op, a, ctr, h, !sparse, early);
		count = (uint64_t)h[0] + h[1];
		if (early && capacity < count) return too_small(count);
		if (path != 2 && early) run_short(c, op, a);
		const uint32_t nlong = h[1];
		res->rows_light = h[0]; res->rows_heavy = nlong;
		res->tuples_light = h[2]; res->tuples_heavy = h[3];
		fold_long_rows(c, op, a, ctr, nlong);
		if (diag) {
			count = read_back(c, a.nz);
			if (sparse && capacity < count) return too_small(count);
		}
	}

	if (sparse && count) {
		const uint32_t ntiles = (uint32_t)((nrow + WAVE_TILE - 1) / WAVE_TILE);
		uint32_t *tile_count = c->arena.get<uint32_t>((size_t)ntiles + 1), *tile_off = c->arena.get<uint32_t>((size_t)ntiles + 1);
		k_red_tile_count<<<dim3(grid_for(ntiles, 4)), dim3(256), 0, st>>>(ptr, a.has, nrow, tile_count);
		SPS_LAUNCH_CHECK();
		scan_exclusive_u32_u32(c, tile_count, tile_off, ntiles);
		const bool dev = mem == SPSAMD_MEM_DEVICE;
		int32_t *oi = dev ? out_idx : c->arena.get<int32_t>(count);
		double *ov = dev ? out_val : c->arena.get<double>(count);
		k_red_compact<<<dim3(grid_for(ntiles, 4)), dim3(256), 0, st>>>(ptr, a.has, nrow, a.dval, tile_off, oi, ov);
		SPS_LAUNCH_CHECK();
		if (!dev) {
			SPS_HIP(hipMemcpyAsync(out_idx, oi, count * sizeof(int32_t), hipMemcpyDeviceToHost, st));
			SPS_HIP(hipMemcpyAsync(out_val, ov, count * sizeof(double), hipMemcpyDeviceToHost, st));
		}
	} else if (!sparse && !direct)
		SPS_HIP(hipMemcpyAsync(out_val, a.dval, nrow * sizeof(double), hipMemcpyDeviceToHost, st));
	*out_nnz = count;
	res->nnz = count;
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_CONSOLIDATED], c->ev[EV_END]));
	return SPSAMD_OK;
}

} // namespace spsamd
