// k_factor.hip -- F = ILU(0) of op(A) on its own pattern by level schedule (spsamd_factor_ilu0, include/spsparse_amd.h;
// DESIGN.md section 21).
//
// S = op(A) as consolidate_operand() hands it over (row-major; consolidated, or trusted as stored), checked here to ascend
// strictly in its (row, col) key.  The result has S's keys and the values of the row-wise loop of the header: row i takes
// its lower tuples (i, k) in ascending k, divides by row k's pivot and subtracts f_t * f_s from the tuple (i, j) for every
// tuple (k, j) right of row k's diagonal that row i stores.  Every value is ONE serial chain -- its updates in ascending k,
// then one division if it is a lower tuple -- so what is parallel is the rows whose named rows are final (the levels of
// solve_tri's LOWER triangle: analyse(), k_solve.hip) and, inside one k, the distinct j.
//
// Row pass (per call, functions of the pattern; thread per tuple or row): the strict-ordering check, each row's diagonal
// position and the start of its upper part, its work w_i (lookups), and the pivots of the rows without a lower tuple.
// Numeric phase, in place on the result's value array F, level by level from level 1 on (level 0 has no lower tuple):
//   own launches  k_fac_serial (a thread per row: rows of at most serial_work lookups) and, where the level has a row of
//                 more work, k_fac_wave (a wave per row, the row's columns and values in LDS) and, where it has a row longer
//                 than the LDS copy, k_fac_block (a workgroup per row, the row's values stay in F)
//   fused run     a maximal run of consecutive thin levels of serial-class rows: ONE launch of ONE workgroup, k_fac_fused,
//                 which walks the levels with __syncthreads() between them
// No kernel here waits on a value another workgroup writes in the same launch: every dependency between workgroups is a
// kernel boundary, every dependency inside a workgroup a barrier.  F is read and written by the same kernel, so nothing
// below marks it __restrict__ or reads it through a non-coherent path.
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace spsamd {

constexpr uint32_t FAC_FUSE_ROWS = SOLVE_FUSE_ROWS;   // default of the factor_fuse_rows knob
constexpr uint32_t FAC_SERIAL_WORK = 64;              // default of factor_serial_work: the most lookups of a serial-class row
constexpr uint32_t FAC_LDS_ROW = 256;                 // default of factor_lds_row: the longest row of the wave kernel's LDS copy
constexpr uint32_t FAC_LDS_ROW_MAX = 4096;            // ... and the most the knob may ask for (48 KiB of LDS)
constexpr int FAC_BLOCK_NT = 256;                     // threads of k_fac_block's workgroup
constexpr uint32_t FAC_NONE = 0xFFFFFFFFu;            // dpos of a row that stores no diagonal

// acc[]: the counters of one call
enum { FAC_UPDATES = 0, FAC_ZERO_PIVOT = 1, FAC_BAD = 2, FAC_LOOKUPS = 3, FAC_MISSING = 4, FAC_ROWS = 5 /* + class - 1 */, FAC_ACC = 8 };

struct FacArgs {
	const uint32_t *ptr;                       // dense row pointer of S
	const int32_t *col;
	double *F;                                 // the result's values: S's on entry
	const uint32_t *dpos, *ustart, *work;      // per row: the diagonal's position (FAC_NONE: none), the first tuple right of it, the lookups (saturated)
	const uint32_t *rows, *level_ptr;          // the schedule
	unsigned long long *acc;
	uint32_t serial_work, lds_row;
	int rowk;                                  // the factor_row knob
};

// first position of [b, e) whose column is >= j (columns ascending)
__device__ __forceinline__ uint32_t fac_lower_bound(const int32_t *col, uint32_t b, uint32_t e, int32_t j)
{
	while (b < e) {
		const uint32_t m = b + ((e - b) >> 1);
		if (col[m] < j) b = m + 1; else e = m;
	}
	return b;
}

// where row i's lower tuples end
__device__ __forceinline__ uint32_t fac_low_end(const FacArgs &a, uint32_t i)
{
	const uint32_t d = a.dpos[i];
	return d != FAC_NONE ? d : a.ustart[i];
}

// 0: no lower tuple (nothing to do) | 1 serial | 2 wave | 3 block
__device__ __forceinline__ int fac_class(uint32_t nlow, uint32_t len, uint32_t work, uint32_t serial_work, uint32_t lds_row, int rowk)
{
	if (nlow == 0) return 0;
	if (rowk == 1) return 1;
	if (rowk == 3) return 3;
	if (rowk == 0 && work <= serial_work) return 1;
	return len <= lds_row ? 2 : 3;
}

__device__ __forceinline__ int fac_class_of(const FacArgs &a, uint32_t i)
{
	const uint32_t b = a.ptr[i];
	return fac_class(fac_low_end(a, i) - b, a.ptr[i + 1] - b, a.work[i], a.serial_work, a.lds_row, a.rowk);
}

__device__ __forceinline__ double fac_pivot(const FacArgs &a, uint32_t k)
{
	const uint32_t d = a.dpos[k];
	return d != FAC_NONE ? a.F[d] : 0.0;
}

// ---------------------------------------------------------------- row pass

// the first position whose (row, col) key does not exceed the key in front of it
__global__ void __launch_bounds__(256) k_fac_check(const int32_t *__restrict__ row, const int32_t *__restrict__ col, uint32_t n,
	unsigned long long *acc)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
	if (t >= n) return;
	const uint64_t k0 = (uint64_t)(uint32_t)row[t - 1] << 32 | (uint32_t)col[t - 1], k1 = (uint64_t)(uint32_t)row[t] << 32 | (uint32_t)col[t];
	if (k1 <= k0) atomicMin(&acc[FAC_BAD], (unsigned long long)t);
}

__global__ void __launch_bounds__(256) k_fac_rows(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, uint64_t n,
	uint32_t *__restrict__ dpos, uint32_t *__restrict__ ustart)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t e = ptr[i + 1], p = fac_lower_bound(col, ptr[i], e, (int32_t)i);
	const bool has = p < e && col[p] == (int32_t)i;
	dpos[i] = has ? p : FAC_NONE;
	ustart[i] = has ? p + 1 : p;
}

// Per row its lookups; the totals; the rows by kernel class; the missing diagonals; the pivots that are final already
// (the rows without a lower tuple, and every row without a diagonal).
__global__ void __launch_bounds__(256) k_fac_work(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col,
	const double *__restrict__ val, uint64_t n, const uint32_t *__restrict__ dpos, const uint32_t *__restrict__ ustart,
	uint32_t *__restrict__ work, unsigned long long *acc, uint32_t serial_work, uint32_t lds_row, int rowk)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = i < n;
	unsigned long long w = 0;
	int cl = 0;
	if (in) {
		const uint32_t b = ptr[i], d = dpos[i], le = d != FAC_NONE ? d : ustart[i];
		for (uint32_t t = b; t < le; ++t) { const uint32_t k = (uint32_t)col[t]; w += ptr[k + 1] - ustart[k]; }
		const uint32_t ws = (uint32_t)std::min<unsigned long long>(w, 0xFFFFFFFFull);
		work[i] = ws;
		cl = fac_class(le - b, ptr[i + 1] - b, ws, serial_work, lds_row, rowk);
		if (d == FAC_NONE) { atomicMin(&acc[FAC_MISSING], (unsigned long long)i); atomicMin(&acc[FAC_ZERO_PIVOT], (unsigned long long)i); }
		else if (le == b && val[d] == 0.0) atomicMin(&acc[FAC_ZERO_PIVOT], (unsigned long long)i);
	}
	const unsigned long long tot = wave_reduce_sum<unsigned long long>(w);
	const uint64_t m1 = __ballot(cl == 1), m2 = __ballot(cl == 2), m3 = __ballot(cl == 3);
	if (lane_id() == 0) {
		if (tot) atomicAdd(&acc[FAC_LOOKUPS], tot);
		if (m1) atomicAdd(&acc[FAC_ROWS + 0], (unsigned long long)__popcll(m1));
		if (m2) atomicAdd(&acc[FAC_ROWS + 1], (unsigned long long)__popcll(m2));
		if (m3) atomicAdd(&acc[FAC_ROWS + 2], (unsigned long long)__popcll(m3));
	}
}

// each level's largest row work: entry p of the schedule's row list finds its level in the levels' bounds
__global__ void __launch_bounds__(256) k_fac_levwork(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ level_ptr,
	uint32_t levels, uint64_t n, const uint32_t *__restrict__ work, uint32_t *levwork)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const uint32_t w = work[rows[p]];
	if (w == 0) return;
	uint32_t lo = 0, hi = levels;                                  // the last level whose bound is <= p
	while (hi - lo > 1) {
		const uint32_t m = lo + ((hi - lo) >> 1);
		if (level_ptr[m] <= p) lo = m; else hi = m;
	}
	atomicMax(&levwork[lo], w);
}

// ---------------------------------------------------------------- numeric phase

__device__ __forceinline__ void fac_count_updates(const FacArgs &a, uint32_t upd)
{
	const uint32_t tot = wave_reduce_sum<uint32_t>(upd);
	if (lane_id() == 0 && tot) atomicAdd(&a.acc[FAC_UPDATES], (unsigned long long)tot);
}

__device__ __forceinline__ void fac_check_pivot(const FacArgs &a, uint32_t i, double p)
{
	if (p == 0.0) atomicMin(&a.acc[FAC_ZERO_PIVOT], (unsigned long long)i);
}

// row i by one thread: for each lower k ascending the division, then a merge walk of row k's upper part and the rest of
// row i (both ascend).  Returns the updates.
__device__ __forceinline__ uint32_t fac_row_serial(const FacArgs &a, uint32_t i)
{
	const uint32_t b = a.ptr[i], e = a.ptr[i + 1], le = fac_low_end(a, i);
	if (le == b) return 0;
	uint32_t upd = 0;
	for (uint32_t t = b; t < le; ++t) {
		const uint32_t k = (uint32_t)a.col[t];
		const double f = ref_div(a.F[t], fac_pivot(a, k));
		a.F[t] = f;
		const uint32_t ke = a.ptr[k + 1];
		uint32_t u = t + 1;
		for (uint32_t s = a.ustart[k]; s < ke && u < e; ++s) {
			const int32_t j = a.col[s];
			while (u < e && a.col[u] < j) ++u;
			if (u < e && a.col[u] == j) { a.F[u] = ref_sub(a.F[u], ref_mul(f, a.F[s])); ++upd; ++u; }
		}
	}
	const uint32_t d = a.dpos[i];
	if (d != FAC_NONE) fac_check_pivot(a, i, a.F[d]);
	return upd;
}

// ---- serial: one thread per entry of the row list [lo, hi); the rows of another class are left to their kernels
__global__ void __launch_bounds__(256) k_fac_serial(FacArgs a, uint32_t lo, uint32_t hi)
{
	const uint64_t p = (uint64_t)lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t upd = 0;
	if (p < hi) {
		const uint32_t row = a.rows[p];
		if (fac_class_of(a, row) == 1) upd = fac_row_serial(a, row);
	}
	fac_count_updates(a, upd);
}

// ---- fused run: the levels [l0, l1), one workgroup, a barrier between two levels
__global__ void __launch_bounds__(SOLVE_NT) k_fac_fused(FacArgs a, uint32_t l0, uint32_t l1)
{
	uint32_t lo = a.level_ptr[l0], upd = 0;
	for (uint32_t l = l0; l < l1; ++l) {                           // uniform
		const uint32_t hi = a.level_ptr[l + 1];
		for (uint32_t p = lo + threadIdx.x; p < hi; p += SOLVE_NT) upd += fac_row_serial(a, a.rows[p]);
		lo = hi;
		__syncthreads();                                           // this level's rows are final, and visible to the workgroup
	}
	fac_count_updates(a, upd);
}

// ---- wave: one wave per listed row, the row's columns and values in LDS (lds_row doubles, then lds_row columns); k runs
// sequentially, the lanes stride over row k's upper tuples and look each j up in the LDS columns
__global__ void __launch_bounds__(64) k_fac_wave(FacArgs a, uint32_t lo)
{
	extern __shared__ double s_fac[];
	const uint32_t row = a.rows[lo + blockIdx.x];
	if (fac_class_of(a, row) != 2) return;                         // uniform
	double *sval = s_fac;
	int32_t *scol = (int32_t *)(s_fac + a.lds_row);
	const uint32_t b = a.ptr[row], len = a.ptr[row + 1] - b, nlow = fac_low_end(a, row) - b, lane = lane_id();
	for (uint32_t q = lane; q < len; q += 64) { scol[q] = a.col[b + q]; sval[q] = a.F[b + q]; }
	uint32_t upd = 0;
	for (uint32_t tt = 0; tt < nlow; ++tt) {                       // uniform
		__syncthreads();                                           // one wave: the LDS writes of the previous k (and the staging) before this k's reads
		const uint32_t k = (uint32_t)scol[tt];
		const double f = ref_div(sval[tt], fac_pivot(a, k));        // every lane the same division (sval[tt] has its last update: they come from smaller k)
		if (lane == 0) a.F[b + tt] = f;                            // (nobody reads a lower tuple of row i again)
		const uint32_t ke = a.ptr[k + 1];
		for (uint32_t s = a.ustart[k] + lane; s < ke; s += 64) {
			const int32_t j = a.col[s];                            // distinct j across the lanes: no two write one value
			const uint32_t u = fac_lower_bound(scol, tt + 1, len, j);
			if (u < len && scol[u] == j) { sval[u] = ref_sub(sval[u], ref_mul(f, a.F[s])); ++upd; }
		}
	}
	__syncthreads();
	for (uint32_t q = nlow + lane; q < len; q += 64) a.F[b + q] = sval[q];
	const uint32_t d = a.dpos[row];
	if (lane == 0 && d != FAC_NONE) fac_check_pivot(a, row, sval[d - b]);
	fac_count_updates(a, upd);
}

// ---- block: one workgroup per listed row, the row's values stay in F; all threads stride over row k's upper tuples, a
// barrier between two k (plain stores, workgroup barrier: the visibility rule of the fused runs)
__global__ void __launch_bounds__(FAC_BLOCK_NT) k_fac_block(FacArgs a, uint32_t lo)
{
	__shared__ double s_f;
	const uint32_t row = a.rows[lo + blockIdx.x];
	if (fac_class_of(a, row) != 3) return;                         // uniform
	const uint32_t b = a.ptr[row], e = a.ptr[row + 1], le = fac_low_end(a, row);
	uint32_t upd = 0;
	for (uint32_t t = b; t < le; ++t) {                            // uniform
		__syncthreads();                                           // the previous k's updates are complete; s_f is free
		const uint32_t k = (uint32_t)a.col[t];
		if (threadIdx.x == 0) { const double f = ref_div(a.F[t], fac_pivot(a, k)); a.F[t] = f; s_f = f; }
		__syncthreads();
		const double f = s_f;
		const uint32_t ke = a.ptr[k + 1];
		for (uint32_t s = a.ustart[k] + threadIdx.x; s < ke; s += FAC_BLOCK_NT) {
			const int32_t j = a.col[s];
			const uint32_t u = fac_lower_bound(a.col, t + 1, e, j);
			if (u < e && a.col[u] == j) { a.F[u] = ref_sub(a.F[u], ref_mul(f, a.F[s])); ++upd; }
		}
	}
	__syncthreads();
	const uint32_t d = a.dpos[row];
	if (threadIdx.x == 0 && d != FAC_NONE) fac_check_pivot(a, row, a.F[d]);
	fac_count_updates(a, upd);
}

// ---------------------------------------------------------------- host

void factor_ilu0(spsamd_ctx *c, const spsamd_coo *A, char transpose, int duplicate_policy, int zero_nan, int sink_kind,
	int sink_flags, spsamd_factor_stats *stats, spsamd_result *res)
{
	check_sink_args(duplicate_policy, sink_kind);
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {A->shape0, A->shape1};
	const uint64_t N = shape[lead];
	if (shape[0] != shape[1]) throw Error{SPSAMD_EDIM, "op(A) must be square for a factorisation"};
	if (operand_view(c, A).coo.nnz >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "operand has 2^31 or more tuples"};
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	std::memset(res, 0, sizeof(*res));
	if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->zero_pivot = stats->missing_diag = -1; }
	res->shape0 = res->shape1 = N;

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
	const spsamd_coo *ops[1] = {A};
	if (n == 0) {                                                    // every row misses its diagonal; one level of N rows
		if (coo) pick_output_set(c, ops, 1);
		if (stats && N) { stats->levels = 1; stats->max_level_rows = N; stats->zero_pivot = stats->missing_diag = 0; }
		deliver_stored(c, res, coo ? coo_output(c, 0) : scratch_output(c, 0), 0, N, coo, permute, sink_flags);
		SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
		return;
	}

	// ---- row pass
	TriView t;
	if (hp) { prepared_row_structure(c, hp); t.ptr = hp->rowptr; }
	else { S.nrow = N; t.ptr = dense_rowptr(c, S, 0); }
	t.col = S.col; t.val = S.val; t.n = N; t.upper = 0; t.unit = 0;
	const int path = c->tune.factor_path == 1 || c->tune.factor_path == 2 ? c->tune.factor_path : 0;
	const int rowk = c->tune.factor_row >= 1 && c->tune.factor_row <= 3 ? c->tune.factor_row : 0;
	const uint32_t fuse_rows = c->tune.factor_fuse_rows > 0 ? (uint32_t)c->tune.factor_fuse_rows : FAC_FUSE_ROWS;
	const uint32_t serial_work = c->tune.factor_serial_work > 0 ? (uint32_t)c->tune.factor_serial_work : FAC_SERIAL_WORK;
	const uint32_t lds_row = c->tune.factor_lds_row > 0 ? std::min<uint32_t>((uint32_t)c->tune.factor_lds_row, FAC_LDS_ROW_MAX) : FAC_LDS_ROW;
	unsigned long long *acc = c->arena.get<unsigned long long>(FAC_ACC);
	uint32_t *dpos = c->arena.get<uint32_t>(N), *ustart = c->arena.get<uint32_t>(N), *work = c->arena.get<uint32_t>(N);
	fill_zero(c, acc, FAC_ACC * sizeof(unsigned long long));
	SPS_HIP(hipMemsetAsync(acc + FAC_ZERO_PIVOT, 0xFF, 2 * sizeof(unsigned long long), st));       // (and FAC_BAD behind it)
	SPS_HIP(hipMemsetAsync(acc + FAC_MISSING, 0xFF, sizeof(unsigned long long), st));
	if (n > 1) { k_fac_check<<<dim3(grid_for(n - 1)), dim3(256), 0, st>>>(S.row, S.col, n, acc); SPS_LAUNCH_CHECK(); }
	k_fac_rows<<<dim3(grid_for(N)), dim3(256), 0, st>>>(t.ptr, S.col, N, dpos, ustart);
	SPS_LAUNCH_CHECK();
	k_fac_work<<<dim3(grid_for(N)), dim3(256), 0, st>>>(t.ptr, S.col, S.val, N, dpos, ustart, work, acc, serial_work, lds_row, rowk);
	SPS_LAUNCH_CHECK();
	unsigned long long hacc[FAC_ACC];
	{
		unsigned long long *h = (unsigned long long *)c->host_staging(FAC_ACC * sizeof(unsigned long long));
		SPS_HIP(hipMemcpyAsync(h, acc, FAC_ACC * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
		std::memcpy(hacc, h, sizeof hacc);
	}
	if (hacc[FAC_BAD] != ~0ull) {
		char buf[200];
		std::snprintf(buf, sizeof buf, "the tuples of op(A) must ascend strictly in their (row, col) key: the key at position %llu "
			"does not exceed the one before it", hacc[FAC_BAD]);
		throw Error{SPSAMD_EINVAL, buf};
	}

	// ---- schedule: the levels of the LOWER triangle, kept in a handle beside solve_tri's
	SolveSchedule local;
	SolveSchedule *s = hp && hp->owns ? &hp->solve[SPSAMD_TRI_LOWER][SPSAMD_DIAG_NONUNIT] : &local;
	const bool reused = s->built;
	uint64_t peel[2] = {0, 0};
	if (!reused) {
		try { analyse(c, t, s == &local ? nullptr : hp, s, peel); }
		catch (...) { *s = SolveSchedule(); throw; }
	}
	if (!s->have_work) {
		uint32_t *levwork = get_zeroed<uint32_t>(c, s->levels);
		k_fac_levwork<<<dim3(grid_for(N)), dim3(256), 0, st>>>(s->rows, s->level_ptr, s->levels, N, work, levwork);
		SPS_LAUNCH_CHECK();
		s->h_level_work.resize(s->levels);
		SPS_HIP(hipMemcpyAsync(s->h_level_work.data(), levwork, (size_t)s->levels * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
		s->have_work = true;
	}
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));

	// ---- the result: S's keys, its values to be factored in place
	if (coo) pick_output_set(c, ops, 1);
	CooOut o;
	if (coo) {
		o = coo_output(c, n);
		SPS_HIP(hipMemcpyAsync(o.row, S.row, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
		SPS_HIP(hipMemcpyAsync(o.col, S.col, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
	} else o = CooOut{S.row, S.col, c->arena.get<double>((size_t)n + 1)};
	SPS_HIP(hipMemcpyAsync(o.val, S.val, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));

	FacArgs a;
	a.ptr = t.ptr; a.col = S.col; a.F = o.val; a.dpos = dpos; a.ustart = ustart; a.work = work;
	a.rows = s->rows; a.level_ptr = s->level_ptr; a.acc = acc;
	a.serial_work = serial_work; a.lds_row = lds_row; a.rowk = rowk;
	const uint32_t *lp = s->h_level_ptr.data(), *lmax = s->h_level_max.data(), *lwork = s->h_level_work.data();
	auto all_serial = [&](uint32_t l) { return rowk == 1 || (rowk == 0 && lwork[l] <= serial_work); };
	auto thin = [&](uint32_t l) { return path != 1 && all_serial(l) && (path == 2 || lp[l + 1] - lp[l] <= fuse_rows); };
	const size_t wave_lds = (size_t)lds_row * (sizeof(double) + sizeof(int32_t));
	uint64_t launches = 0, fused = 0;
	for (uint32_t l = 1; l < s->levels;) {
		if (thin(l)) {
			uint32_t e = l + 1;
			while (e < s->levels && thin(e)) ++e;
			k_fac_fused<<<dim3(1), dim3(SOLVE_NT), 0, st>>>(a, l, e);
			SPS_LAUNCH_CHECK();
			++launches; fused += e - l;
			l = e;
			continue;
		}
		const uint32_t lo = lp[l], hi = lp[l + 1];
		const bool serial_only = all_serial(l);
		if (rowk <= 1) {
			k_fac_serial<<<dim3(grid_for(hi - lo)), dim3(256), 0, st>>>(a, lo, hi);
			SPS_LAUNCH_CHECK();
			++launches;
		}
		if (!serial_only && rowk != 3) {
			k_fac_wave<<<dim3(hi - lo), dim3(64), wave_lds, st>>>(a, lo);
			SPS_LAUNCH_CHECK();
			++launches;
		}
		if (!serial_only && (rowk == 3 || lmax[l] > lds_row)) {
			k_fac_block<<<dim3(hi - lo), dim3(FAC_BLOCK_NT), 0, st>>>(a, lo);
			SPS_LAUNCH_CHECK();
			++launches;
		}
		++l;
	}
	{                                                                // (before the sink tail, which stages words of its own)
		unsigned long long *h = (unsigned long long *)c->host_staging(2 * sizeof(unsigned long long));
		SPS_HIP(hipMemcpyAsync(h, acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
		std::memcpy(hacc, h, 2 * sizeof(unsigned long long));
	}
	res->products = hacc[FAC_LOOKUPS];
	// S's own order and keys: row-major, every key once, indices checked (read permuted: sorted by {1, 0})
	deliver_stored(c, res, o, n, N, coo, permute, sink_flags);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	if (stats) {
		stats->levels = s->levels; stats->max_level_rows = s->max_level_rows;
		stats->launches = launches; stats->fused_levels = fused;
		stats->lookups = hacc[FAC_LOOKUPS]; stats->updates = hacc[FAC_UPDATES];
		stats->zero_pivot = hacc[FAC_ZERO_PIVOT] == ~0ull ? -1 : (int64_t)hacc[FAC_ZERO_PIVOT];
		stats->missing_diag = hacc[FAC_MISSING] == ~0ull ? -1 : (int64_t)hacc[FAC_MISSING];
		stats->rows_serial = hacc[FAC_ROWS + 0]; stats->rows_wave = hacc[FAC_ROWS + 1]; stats->rows_block = hacc[FAC_ROWS + 2];
		stats->analysis_reused = reused ? 1u : 0u;
		stats->ms_analysis = res->ms_symbolic; stats->ms_factor = res->ms_numeric;
	}
}

} // namespace spsamd
