// k_solve.hip -- T * X = B for a triangle T of op(A) by level schedule (spsamd_solve_tri, include/spsparse_amd.h;
// DESIGN.md section 20).
//
// S = op(A) as consolidate_operand() hands it over (row-major; consolidated, or trusted as stored).  Of row i the tuples on
// the other side of the diagonal are skipped (under DIAG_UNIT the diagonal too); every entry of X is then ONE serial chain
// in S's order -- acc - v * x rounded twice per off-diagonal tuple, d + v per diagonal tuple, one division at the end, a NaN
// result with x86's bits (x86fp.h) -- so what is parallel is the set of (row, rhs) chains whose inputs are complete.
//
// Analysis (the schedule; kept in a prepared handle per (uplo, diag)):
//   1. k_tri_init: per row its used off-diagonal tuples (the in-degree), the diagonal fold (zero pivot), the used tuples;
//      the rows without a dependency are the first frontier.
//   2. the used off-diagonal tuples keyed by column, one PairSort: a column-ordered view in which a finished row finds its
//      dependants.
//   3. the peel: a frontier's rows get the level, decrement their dependants, and those that reach zero are the next
//      frontier (wave_claim).  A wide frontier is one launch of k_peel_wide (the host looks at the frontier size every
//      PEEL_BATCH launches, not every level); a frontier of at most PEEL_THIN_MAX rows is taken by k_peel_thin, ONE workgroup
//      that walks level after level with a barrier between them until the frontier is empty or wide again.
//   4. one stable sort of the rows by level (ascending rows inside a level), the levels' bounds, each level's longest row.
// Numeric phase, level by level in the order of the schedule:
//   own launch   k_solve_serial (a thread per (row, rhs): rows of at most long_min tuples) and, where the level has a longer
//                row, k_solve_lanes / k_solve_fold (a wave per row; the shapes of k_spmm.hip)
//   fused run    a maximal run of consecutive thin levels of short rows: ONE launch of ONE workgroup, k_solve_fused, which
//                walks the levels with __syncthreads() between them
// No kernel here waits on a value another workgroup writes in the same launch: every dependency between workgroups is a
// kernel boundary, every dependency inside k_solve_fused / k_peel_thin a workgroup barrier.  X is read and written by the same
// kernel, so nothing below marks it __restrict__ or reads it through a non-coherent path.
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

constexpr uint64_t SOLVE_FUSE_WORK = 2048;     // ... under which a thin level also has at most this many (row, rhs) pairs: two strides of the workgroup
constexpr uint32_t PEEL_THIN_MAX = 2048;       // frontier rows up to which the peel stays inside one workgroup
constexpr int PEEL_BATCH = 16;                 // wide frontiers: launches between two looks at the frontier size
constexpr int SOLVE_FOLD_RHS = 16;             // right-hand sides per pass of k_solve_fold (LDS: 16 x 65 doubles)

// 0: skipped (the other triangle; the diagonal under UNIT) | 1: off-diagonal, used | 2: diagonal, used
__device__ __forceinline__ int tri_class(int32_t i, int32_t j, int upper, int unit)
{
	if (j == i) return unit ? 0 : 2;
	return (j < i) != (upper != 0) ? 1 : 0;
}

// ---------------------------------------------------------------- analysis

// acc[0]: used tuples; acc[1]: the smallest row whose diagonal folds to +-0.0 (all ones: none)
__global__ void __launch_bounds__(256) k_tri_init(TriView t, uint32_t *__restrict__ indeg, unsigned long long *acc,
	uint32_t *__restrict__ front, uint32_t *fcount)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = i < t.n;
	uint32_t off = 0, used = 0;
	bool zero = false;
	if (in) {
		double d = 0.0;
		const uint32_t e = t.ptr[i + 1];
		for (uint32_t k = t.ptr[i]; k < e; ++k) {
			const int cl = tri_class((int32_t)i, t.col[k], t.upper, t.unit);
			if (cl == 1) ++off;
			else if (cl == 2) { d = ref_add(d, t.val[k]); ++used; }
		}
		used += off;
		indeg[i] = off;
		zero = !t.unit && d == 0.0;
	}
	const bool free_row = in && off == 0;
	const uint32_t slot = wave_claim(fcount, free_row);
	if (free_row) front[slot] = (uint32_t)i;
	const uint32_t tot = wave_reduce_sum<uint32_t>(used);
	if (lane_id() == 0 && tot) atomicAdd(&acc[0], (unsigned long long)tot);
	if (zero) atomicMin(&acc[1], (unsigned long long)i);
}

// the used off-diagonal tuples of row i, from uoff[i] on: the column as sort key, the row beside it
__global__ void __launch_bounds__(256) k_tri_deps(TriView t, const uint32_t *__restrict__ uoff, uint64_t *__restrict__ keys,
	uint32_t *__restrict__ urow)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= t.n) return;
	uint32_t o = uoff[i];
	const uint32_t e = t.ptr[i + 1];
	for (uint32_t k = t.ptr[i]; k < e; ++k) {
		const int32_t j = t.col[k];
		if (tri_class((int32_t)i, j, t.upper, t.unit) == 1) { keys[o] = (uint64_t)(uint32_t)j; urow[o] = (uint32_t)i; ++o; }
	}
}

// sorted by column: the dependant of entry k and its column as dense_rowptr reads it
__global__ void __launch_bounds__(256) k_tri_depgather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm,
	const uint32_t *__restrict__ urow, uint32_t m, uint32_t *__restrict__ dep, int32_t *__restrict__ scol)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= m) return;
	dep[k] = urow[perm[k]];
	scol[k] = (int32_t)keys[k];
}

// One level of a wide frontier.  fin / *cin: the frontier; fout / *cout: the next one (unordered); *czero: the counter of
// the level after that (nobody reads it in this launch).
__global__ void __launch_bounds__(256) k_peel_wide(const uint32_t *__restrict__ cptr, const uint32_t *__restrict__ dep, uint32_t *indeg,
	uint32_t *__restrict__ level, uint32_t L, const uint32_t *__restrict__ fin, const uint32_t *__restrict__ cin,
	uint32_t *__restrict__ fout, uint32_t *cout, uint32_t *czero, uint32_t *nlev)
{
	const uint32_t n = *cin;
	if (blockIdx.x == 0 && threadIdx.x == 0) { *czero = 0; if (n) *nlev = L + 1; }
	const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += stride) {      // uniform in the workgroup
		const uint64_t e = base + threadIdx.x;
		uint32_t k = 0, ke = 0;
		if (e < n) { const uint32_t r = fin[e]; level[r] = L; k = cptr[r]; ke = cptr[r + 1]; }
		while (__ballot(k < ke)) {                                 // uniform in the wave (wave_claim ballots)
			bool ready = false;
			uint32_t d = 0;
			if (k < ke) { d = dep[k]; ready = atomicSub(&indeg[d], 1u) == 1u; ++k; }
			const uint32_t slot = wave_claim(cout, ready);
			if (ready) fout[slot] = d;
		}
	}
}

// Thin frontiers: one workgroup walks the levels from L on until the frontier is empty or has more than PEEL_THIN_MAX rows.
// f[0] holds the frontier of *cin rows on entry.  On exit st[0] = the level reached, st[1] = which of f[0] / f[1] holds the
// frontier now, st[2] = its size; cnt3[0] = that size, cnt3[1] = cnt3[2] = 0 (the wide kernel's three counters, restarted).
__global__ void __launch_bounds__(SOLVE_NT) k_peel_thin(const uint32_t *__restrict__ cptr, const uint32_t *__restrict__ dep, uint32_t *indeg,
	uint32_t *__restrict__ level, uint32_t L, uint32_t *f0, uint32_t *f1, const uint32_t *cin, uint32_t *cnt3, uint32_t *st, uint32_t *nlev)
{
	__shared__ uint32_t s_cnt[3];
	uint32_t n = *cin;
	if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
	__syncthreads();
	uint32_t *fin = f0, *fout = f1;
	uint32_t which = 0, it = 0;
	const uint32_t L0 = L;
	while (n != 0 && n <= PEEL_THIN_MAX) {                          // uniform
		uint32_t *next = &s_cnt[it % 3];
		for (uint32_t e = threadIdx.x; e < n; e += SOLVE_NT) {
			const uint32_t r = fin[e];
			level[r] = L;
			const uint32_t ke = cptr[r + 1];
			for (uint32_t k = cptr[r]; k < ke; ++k) {
				const uint32_t d = dep[k];
				if (atomicSub(&indeg[d], 1u) == 1u) fout[atomicAdd(next, 1u)] = d;
			}
		}
		__syncthreads();                                           // the next frontier is complete, and visible to the workgroup
		n = *next;
		if (threadIdx.x == 0) s_cnt[(it + 2) % 3] = 0;             // the counter of the level after the next: last read before this barrier
		uint32_t *t = fin; fin = fout; fout = t;
		which ^= 1u; ++it; ++L;
	}
	if (threadIdx.x == 0) {
		st[0] = L; st[1] = which; st[2] = n;
		cnt3[0] = n; cnt3[1] = 0; cnt3[2] = 0;
		if (L > L0) *nlev = L;
	}
}

__global__ void __launch_bounds__(256) k_level_keys(const uint32_t *__restrict__ level, uint64_t n, uint64_t *__restrict__ keys)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = level[i];
}

// the sorted levels as dense_rowptr reads them, and each level's longest row
__global__ void __launch_bounds__(256) k_level_sorted(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rows,
	const uint32_t *__restrict__ ptr, uint64_t n, int32_t *__restrict__ slev, uint32_t *levmax)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = p < n;
	uint32_t lev = 0, len = 0;
	if (in) { lev = (uint32_t)keys[p]; slev[p] = (int32_t)lev; const uint32_t r = rows[p]; len = ptr[r + 1] - ptr[r]; }
	// neighbours in the list mostly share a level: one atomic for the wave then
	const uint64_t act = __ballot(in);
	if (!act) return;                                              // uniform
	const uint32_t lev0 = (uint32_t)__builtin_amdgcn_readlane((int)lev, __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)act) - 1));
	if (__ballot(in && lev != lev0) == 0) {                        // uniform
		uint32_t mx = len;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) mx = std::max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
		if (lane_id() == 0 && mx) atomicMax(&levmax[lev0], mx);
	} else if (in && len) atomicMax(&levmax[lev], len);
}

// ---------------------------------------------------------------- numeric phase

struct SolveArgs {
	TriView t;
	const uint32_t *rows, *level_ptr;          // the schedule
	const double *B;                           // (may be X: in place)
	uint64_t ldb;
	double *X;
	uint64_t ldx;
	uint32_t nrhs, long_min;
};

__device__ __forceinline__ double solve_finish(double acc, double d, int unit) { return unit ? acc : ref_div(acc, d); }

// the chain of (row, rhs r), front to back
__device__ __forceinline__ void solve_one(const SolveArgs &a, uint32_t row, uint32_t r)
{
	const uint32_t e = a.t.ptr[row + 1];
	double acc = a.B[(uint64_t)row * a.ldb + r], d = 0.0;
	for (uint32_t k = a.t.ptr[row]; k < e; ++k) {
		const int32_t j = a.t.col[k];
		const int cl = tri_class((int32_t)row, j, a.t.upper, a.t.unit);
		if (cl == 1) acc = ref_sub(acc, ref_mul(a.t.val[k], a.X[(uint64_t)(uint32_t)j * a.ldx + r]));
		else if (cl == 2) d = ref_add(d, a.t.val[k]);
	}
	a.X[(uint64_t)row * a.ldx + r] = solve_finish(acc, d, a.t.unit);
}

// ---- serial: one thread per (row, rhs) of list entries [lo, hi), rhs fastest; rows of more than long_min tuples are left
// to the wave kernels
__global__ void __launch_bounds__(256) k_solve_serial(SolveArgs a, uint32_t lo, uint32_t hi)
{
	const uint64_t total = (uint64_t)(hi - lo) * a.nrhs;
	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t q = t / a.nrhs;
		const uint32_t row = a.rows[lo + q], r = (uint32_t)(t - q * a.nrhs);
		if (a.t.ptr[row + 1] - a.t.ptr[row] > a.long_min) continue;
		solve_one(a, row, r);
	}
}

// ---- fused run: the levels [l0, l1), one workgroup, a barrier between two levels
__global__ void __launch_bounds__(SOLVE_NT) k_solve_fused(SolveArgs a, uint32_t l0, uint32_t l1)
{
	uint32_t lo = a.level_ptr[l0];
	for (uint32_t l = l0; l < l1; ++l) {                           // uniform
		const uint32_t hi = a.level_ptr[l + 1];
		const uint64_t total = (uint64_t)(hi - lo) * a.nrhs;
		for (uint64_t t = threadIdx.x; t < total; t += SOLVE_NT) {
			const uint64_t q = t / a.nrhs;
			solve_one(a, a.rows[lo + q], (uint32_t)(t - q * a.nrhs));
		}
		lo = hi;
		__syncthreads();                                           // this level's X is complete, and visible to the workgroup
	}
}

// ---- lanes: one wave per listed row, lane = right-hand side, tuples read wave-uniform
__global__ void __launch_bounds__(64) k_solve_lanes(SolveArgs a, uint32_t lo)
{
	const uint32_t row = a.rows[lo + blockIdx.x];
	const uint32_t b = a.t.ptr[row], e = a.t.ptr[row + 1];
	if (e - b <= a.long_min) return;
	for (uint32_t rb = 0; rb < a.nrhs; rb += 64) {
		const uint32_t r = rb + lane_id();
		const bool on = r < a.nrhs;
		double acc = on ? a.B[(uint64_t)row * a.ldb + r] : 0.0, d = 0.0;
		for (uint32_t k = b; k < e; ++k) {
			const int32_t j = a.t.col[k];                              // wave-uniform
			const int cl = tri_class((int32_t)row, j, a.t.upper, a.t.unit);
			if (cl == 1) {
				const double x = on ? a.X[(uint64_t)(uint32_t)j * a.ldx + r] : 0.0;
				acc = ref_sub(acc, ref_mul(a.t.val[k], x));
			} else if (cl == 2) d = ref_add(d, a.t.val[k]);
		}
		if (on) a.X[(uint64_t)row * a.ldx + r] = solve_finish(acc, d, a.t.unit);
	}
}

// ---- fold: one wave per listed row, the products of 64 tuples at a time across the lanes into LDS, then one ordered fold
// per right-hand side by one lane each
__global__ void __launch_bounds__(64) k_solve_fold(SolveArgs a, uint32_t lo)
{
	__shared__ double prod[SOLVE_FOLD_RHS][65];                    // [rhs][tuple]; a diagonal tuple's value in prod[0]
	__shared__ uint8_t cls[64];
	const uint32_t row = a.rows[lo + blockIdx.x];
	const uint32_t b = a.t.ptr[row], e = a.t.ptr[row + 1];
	if (e - b <= a.long_min) return;
	const uint32_t lane = lane_id();
	for (uint32_t rb = 0; rb < a.nrhs; rb += SOLVE_FOLD_RHS) {
		const uint32_t nr = std::min((uint32_t)SOLVE_FOLD_RHS, a.nrhs - rb);
		double acc = lane < nr ? a.B[(uint64_t)row * a.ldb + rb + lane] : 0.0, d = 0.0;
		for (uint32_t k0 = b; k0 < e; k0 += 64) {
			const uint32_t cnt = std::min(64u, e - k0);
			if (lane < cnt) {
				const int32_t j = a.t.col[k0 + lane];
				const int cl = tri_class((int32_t)row, j, a.t.upper, a.t.unit);
				cls[lane] = (uint8_t)cl;
				if (cl) {
					const double v = a.t.val[k0 + lane];
					if (cl == 2) prod[0][lane] = v;
					else {
						const double *xr = a.X + (uint64_t)(uint32_t)j * a.ldx + rb;
						for (uint32_t q = 0; q < nr; ++q) prod[q][lane] = ref_mul(v, xr[q]);
					}
				}
			}
			__syncthreads();
			if (lane < nr) {
				for (uint32_t q = 0; q < cnt; ++q) {
					const int cl = cls[q];
					if (cl == 1) acc = ref_sub(acc, prod[lane][q]);
					else if (cl == 2) d = ref_add(d, prod[0][q]);
				}
			}
			__syncthreads();
		}
		if (lane < nr) a.X[(uint64_t)row * a.ldx + rb + lane] = solve_finish(acc, d, a.t.unit);
	}
}

// ---------------------------------------------------------------- host

// (declared in internal.h: spsamd_factor_ilu0 schedules by the LOWER triangle's levels as well)
void analyse(spsamd_ctx *c, const TriView &t, Prepared *hp, SolveSchedule *s, uint64_t peel[2])
{
	hipStream_t st = c->stream;
	const uint64_t N = t.n;
	uint32_t *indeg = c->arena.get<uint32_t>(N + 1), *uoff = c->arena.get<uint32_t>(N + 1);
	uint32_t *f[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)};
	uint32_t *level = c->arena.get<uint32_t>(N);
	unsigned long long *acc = c->arena.get<unsigned long long>(2);
	uint32_t *ctr = get_zeroed<uint32_t>(c, 8);                      // [0..2] the frontier counters, [3] the levels, [4..6] k_peel_thin's report
	uint32_t *cnt3 = ctr, *nlev = ctr + 3, *state = ctr + 4;
	fill_zero(c, acc, sizeof(unsigned long long));
	SPS_HIP(hipMemsetAsync(acc + 1, 0xFF, sizeof(unsigned long long), st));
	k_tri_init<<<dim3(grid_for(N)), dim3(256), 0, st>>>(t, indeg, acc, f[0], &cnt3[0]);
	SPS_LAUNCH_CHECK();
	scan_exclusive_u32_u32(c, indeg, uoff, N);
	const uint32_t m = read_back(c, uoff + N);                       // the used off-diagonal tuples

	if (m == 0) {                                                    // no dependency anywhere: one level
		fill_zero(c, level, N * sizeof(uint32_t));
		fill_u32(c, nlev, 1u, 1);
	} else {
		PairSort sort(c, m);
		uint32_t *urow = c->arena.get<uint32_t>(m), *dep = c->arena.get<uint32_t>(m);
		int32_t *scol = c->arena.get<int32_t>(m);
		k_tri_deps<<<dim3(grid_for(N)), dim3(256), 0, st>>>(t, uoff, sort.keys, urow);
		SPS_LAUNCH_CHECK();
		sort.run(bits_of(N));
		k_tri_depgather<<<dim3(grid_for(m)), dim3(256), 0, st>>>(sort.keys, sort.perm, urow, m, dep, scol);
		SPS_LAUNCH_CHECK();
		ConMat cols;
		cols.row = scol; cols.nnz = m; cols.nrow = N;
		const uint32_t *cptr = dense_rowptr(c, cols, 0u);

		uint32_t L = 0;
		int cur = 0, ci = 0;                                         // f[cur] / cnt3[ci]: the frontier of level L
		const unsigned wide_grid = (unsigned)c->num_cu * 8;
		for (;;) {
			const uint32_t n = read_back(c, &cnt3[ci]);
			if (n == 0) break;
			if (n <= PEEL_THIN_MAX) {
				k_peel_thin<<<dim3(1), dim3(SOLVE_NT), 0, st>>>(cptr, dep, indeg, level, L, f[cur], f[cur ^ 1], &cnt3[ci], cnt3, state, nlev);
				SPS_LAUNCH_CHECK();
				++peel[0];
				uint32_t *h = (uint32_t *)c->host_staging(4 * sizeof(uint32_t));
				SPS_HIP(hipMemcpyAsync(h, state, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
				SPS_HIP(hipStreamSynchronize(st));
				L = h[0]; cur ^= (int)h[1]; ci = 0;
				if (h[2] == 0) break;
			}
			for (int b = 0; b < PEEL_BATCH; ++b) {
				k_peel_wide<<<dim3(wide_grid), dim3(256), 0, st>>>(cptr, dep, indeg, level, L, f[cur], &cnt3[ci], f[cur ^ 1],
					&cnt3[(ci + 1) % 3], &cnt3[(ci + 2) % 3], nlev);
				SPS_LAUNCH_CHECK();
				++peel[1];
				++L; cur ^= 1; ci = (ci + 1) % 3;
			}
		}
	}

	uint32_t *h = (uint32_t *)c->host_staging(8 * sizeof(uint32_t));
	SPS_HIP(hipMemcpyAsync(h, nlev, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipMemcpyAsync(h + 2, acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipStreamSynchronize(st));
	const uint32_t levels = h[0];
	unsigned long long hacc[2];
	std::memcpy(hacc, h + 2, sizeof hacc);
	s->levels = levels;
	s->tuples_used = hacc[0];
	s->zero_pivot = hacc[1] == ~0ull ? -1 : (int64_t)hacc[1];

	// the rows by level, ascending inside a level; the levels' bounds; each level's longest row
	PairSort byl(c, N);
	k_level_keys<<<dim3(grid_for(N)), dim3(256), 0, st>>>(level, N, byl.keys);
	SPS_LAUNCH_CHECK();
	byl.run(bits_of(levels));
	int32_t *slev = c->arena.get<int32_t>(N);
	uint32_t *levmax = get_zeroed<uint32_t>(c, levels);
	k_level_sorted<<<dim3(grid_for(N)), dim3(256), 0, st>>>(byl.keys, byl.perm, t.ptr, N, slev, levmax);
	SPS_LAUNCH_CHECK();
	ConMat lv;
	lv.row = slev; lv.nnz = (uint32_t)N; lv.nrow = levels;
	uint32_t *level_ptr = dense_rowptr(c, lv, 0u);
	s->rows = byl.perm;
	s->level_ptr = level_ptr;
	if (hp) {                                                        // a handle keeps its own copy (the workspace's is gone after this call)
		// (a block of its own, not carved from the handle's slab: spsamd_operand_bytes grows by exactly this schedule)
		const size_t rbytes = (N * sizeof(uint32_t) + 255) & ~size_t(255), bytes = rbytes + ((size_t)levels + 1) * sizeof(uint32_t);
		void *blk = nullptr;
		if (hipMalloc(&blk, bytes) != hipSuccess) { (void)hipGetLastError(); throw Error{SPSAMD_ENOMEM, "hipMalloc of a solve schedule failed"}; }
		hp->owned.push_back(blk);
		hp->owned_bytes += bytes;
		s->rows = (uint32_t *)blk;
		s->level_ptr = (uint32_t *)((char *)blk + rbytes);
		SPS_HIP(hipMemcpyAsync(s->rows, byl.perm, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
		SPS_HIP(hipMemcpyAsync(s->level_ptr, level_ptr, ((size_t)levels + 1) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
	}
	s->h_level_ptr.resize((size_t)levels + 1);
	s->h_level_max.resize(levels);
	SPS_HIP(hipMemcpyAsync(s->h_level_ptr.data(), level_ptr, ((size_t)levels + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipMemcpyAsync(s->h_level_max.data(), levmax, (size_t)levels * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipStreamSynchronize(st));
	s->max_level_rows = 0;
	for (uint32_t l = 0; l < levels; ++l) s->max_level_rows = std::max(s->max_level_rows, s->h_level_ptr[l + 1] - s->h_level_ptr[l]);
	s->built = true;
}

// (declared in internal.h: spsamd_solve_pcg applies a factor's two triangles every iteration on schedules it got once)
uint64_t solve_levels(spsamd_ctx *c, const TriView &t, const SolveSchedule &s, const double *B, uint64_t ldb, double *X,
	uint64_t ldx, uint32_t nrhs, uint64_t *fused_levels)
{
	hipStream_t st = c->stream;
	SolveArgs a;
	a.t = t; a.rows = s.rows; a.level_ptr = s.level_ptr; a.nrhs = nrhs;
	a.B = B; a.ldb = ldb; a.X = X; a.ldx = ldx;
	const int path = c->tune.solve_path == 1 || c->tune.solve_path == 2 ? c->tune.solve_path : 0;
	const int rowk = c->tune.solve_row >= 1 && c->tune.solve_row <= 3 ? c->tune.solve_row : 0;
	// serial rows: up to long_min tuples (0 in a forced wave kernel: only the empty rows are serial)
	a.long_min = rowk == 1 ? 0xFFFFFFFFu : rowk >= 2 ? 0u : c->tune.spmm_long_min > 0 ? (uint32_t)c->tune.spmm_long_min : 64u;
	const bool lanes = rowk == 2 || (rowk == 0 && nrhs >= 16);
	// (a set knob is taken as given; the default also bounds a thin level's work, which grows with nrhs)
	const uint32_t fuse_rows = c->tune.solve_fuse_rows > 0 ? (uint32_t)c->tune.solve_fuse_rows
		: (uint32_t)std::min<uint64_t>(SOLVE_FUSE_ROWS, std::max<uint64_t>(SOLVE_FUSE_WORK / nrhs, 1));
	const uint32_t *lp = s.h_level_ptr.data(), *lmax = s.h_level_max.data();
	auto thin = [&](uint32_t l) { return path != 1 && lmax[l] <= a.long_min && (path == 2 || lp[l + 1] - lp[l] <= fuse_rows); };
	uint64_t launches = 0, fused = 0;
	for (uint32_t l = 0; l < s.levels;) {
		if (thin(l)) {
			uint32_t e = l + 1;
			while (e < s.levels && thin(e)) ++e;
			k_solve_fused<<<dim3(1), dim3(SOLVE_NT), 0, st>>>(a, l, e);
			SPS_LAUNCH_CHECK();
			++launches; fused += e - l;
			l = e;
			continue;
		}
		const uint32_t lo = lp[l], hi = lp[l + 1];
		const uint64_t total = (uint64_t)(hi - lo) * nrhs;
		k_solve_serial<<<dim3((unsigned)std::min<uint64_t>(grid_for(total), (uint64_t)c->num_cu * 64)), dim3(256), 0, st>>>(a, lo, hi);
		SPS_LAUNCH_CHECK();
		++launches;
		if (lmax[l] > a.long_min) {
			if (lanes) k_solve_lanes<<<dim3(hi - lo), dim3(64), 0, st>>>(a, lo);
			else k_solve_fold<<<dim3(hi - lo), dim3(64), 0, st>>>(a, lo);
			SPS_LAUNCH_CHECK();
			++launches;
		}
		++l;
	}
	if (fused_levels) *fused_levels = fused;
	return launches;
}

int solve_tri(spsamd_ctx *c, const spsamd_coo *A, char transpose, int uplo, int diag, const double *B, size_t ldb, double *X,
	size_t ldx, size_t nrhs, int mem, int duplicate_policy, int zero_nan, spsamd_solve_stats *stats, spsamd_result *res)
{
	if (uplo != SPSAMD_TRI_LOWER && uplo != SPSAMD_TRI_UPPER) throw Error{SPSAMD_EINVAL, "uplo must be SPSAMD_TRI_LOWER or SPSAMD_TRI_UPPER"};
	if (diag != SPSAMD_DIAG_NONUNIT && diag != SPSAMD_DIAG_UNIT) throw Error{SPSAMD_EINVAL, "diag must be SPSAMD_DIAG_NONUNIT or SPSAMD_DIAG_UNIT"};
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of B and X must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	if (ldb < nrhs || ldx < nrhs) throw Error{SPSAMD_EINVAL, "leading dimension of B or X smaller than nrhs"};
	if (nrhs > 0xFFFFFFFFull) throw Error{SPSAMD_EINVAL, "nrhs exceeds 2^32 - 1"};
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {A->shape0, A->shape1};
	const uint64_t N = shape[lead];
	if (shape[0] != shape[1]) throw Error{SPSAMD_EDIM, "op(A) must be square for a triangular solve"};
	if (nrhs && N && (!B || !X)) throw Error{SPSAMD_EINVAL, "null B or X"};
	const bool in_place = X == B;
	{
		const OperandView view = operand_view(c, A);
		const uint64_t n = view.coo.nnz;
		if (n >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "operand has 2^31 or more tuples"};
		const uint64_t bbytes = N && nrhs ? ((N - 1) * ldb + nrhs) * sizeof(double) : 0;
		const uint64_t xbytes = N && nrhs ? ((N - 1) * ldx + nrhs) * sizeof(double) : 0;
		if (in_place ? (bbytes && ldx != ldb) : ranges_overlap(X, xbytes, B, bbytes))
			throw Error{SPSAMD_EINVAL, "X and B overlap (in place: X == B with ldx == ldb)"};
		const void *arr[3] = {view.coo.idx0, view.coo.idx1, view.coo.val};
		for (int k = 0; k < 3; ++k)
			if (ranges_overlap(X, xbytes, arr[k], n * (k == 2 ? 8 : 4))) throw Error{SPSAMD_EINVAL, "X overlaps A's arrays"};
		if (mem == SPSAMD_MEM_DEVICE && xbytes)
			for (const auto &s : c->out)
				if (s.holds(X) || s.holds((const char *)X + xbytes - 1)) throw Error{SPSAMD_EINVAL, "X lies in an output set of the context"};
	}
	std::memset(res, 0, sizeof(*res));
	if (stats) { std::memset(stats, 0, sizeof(*stats)); stats->zero_pivot = -1; }
	res->shape0 = res->shape1 = N;
	if (!nrhs || !N) return SPSAMD_OK;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	ConMat S;
	Prepared *hp = nullptr;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S, &hp);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	res->nnz_a = S.nnz;

	TriView t;
	if (hp) { prepared_row_structure(c, hp); t.ptr = hp->rowptr; }
	else { S.nrow = N; t.ptr = dense_rowptr(c, S, 0); }
	t.col = S.col; t.val = S.val; t.n = N; t.upper = uplo == SPSAMD_TRI_UPPER; t.unit = diag == SPSAMD_DIAG_UNIT;

	SolveSchedule local;
	SolveSchedule *s = hp && hp->owns ? &hp->solve[uplo][diag] : &local;
	const bool reused = s->built;
	uint64_t peel[2] = {0, 0};
	if (!reused) {
		try { analyse(c, t, s == &local ? nullptr : hp, s, peel); }
		catch (...) { *s = SolveSchedule(); throw; }
	}
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));

	const double *db = B;
	double *dx = X;
	uint64_t dldb = ldb, dldx = ldx;
	if (mem == SPSAMD_MEM_HOST) {                                        // one packed device copy, solved in place
		double *tx = c->arena.get<double>(N * nrhs);
		SPS_HIP(hipMemcpy2DAsync(tx, nrhs * sizeof(double), B, ldb * sizeof(double), nrhs * sizeof(double), N, hipMemcpyHostToDevice, st));
		db = tx; dx = tx; dldb = dldx = nrhs;
	}
	uint64_t fused = 0;
	const uint64_t launches = solve_levels(c, t, *s, db, dldb, dx, dldx, (uint32_t)nrhs, &fused);
	if (mem == SPSAMD_MEM_HOST)
		SPS_HIP(hipMemcpy2DAsync(X, ldx * sizeof(double), dx, nrhs * sizeof(double), nrhs * sizeof(double), N, hipMemcpyDeviceToHost, st));
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	if (stats) {
		stats->levels = s->levels; stats->max_level_rows = s->max_level_rows;
		stats->launches = launches; stats->fused_levels = fused;
		stats->tuples_used = s->tuples_used; stats->zero_pivot = s->zero_pivot;
		stats->analysis_reused = reused ? 1u : 0u;
		stats->peel_thin_launches = peel[0]; stats->peel_wide_launches = peel[1];
		stats->ms_analysis = res->ms_symbolic; stats->ms_solve = res->ms_numeric;
	}
	return SPSAMD_OK;
}

} // namespace spsamd
