// k_amg.hip -- one multigrid V-cycle over the caller's levels, and that cycle as the preconditioner of the conjugate
// gradient loop of k_krylov.hip (spsamd_amg_apply, spsamd_solve_pcg_amg, include/spsparse_amd.h).
//
// Every level operand is taken by consolidate_operand() like S of spsamd_solve_pcg (row-major; consolidated, or trusted as
// stored).  Every returned bit is defined by the loop of the header: a row of an operand is ONE serial chain from +0.0 in the
// operand's order wherever it runs, and the smoother's omega * ((b - q) / d) is three operations rounded one by one
// (x86fp.h).  Three places walk a row:
//   a lane of a level kernel      k_amg_smooth, k_amg_residual, k_amg_restrict, k_amg_prolong: a row per lane straight off
//                                 ptr / col / val, the vector operation of the step in the same pass
//   the wave kernel of k_spmm.hip rows above spmm_long_min (listed once, at set-up): the level kernel stores +0.0 for such
//                                 a row, the wave kernel adds the chain to it, k_amg_long finishes the row's vector operation
//   a thread of the fused tail    k_amg_tail: one workgroup walks the thin levels down and up, threads stride over the rows,
//                                 a workgroup barrier between any write of a vector and its next read
// A cycle is planned once per call: every buffer comes from the workspace at set-up, the x buffers of a level ping-pong (no
// lane reads what another wrote in the launch), and which of the two holds a level's result follows from the sweep counts.
// The cycle kernels write level scratch and the cycle's result only and read no PcgState: after the stop of the loop z is
// scratch (k_krylov.hip).
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <vector>

namespace spsamd {

constexpr int AMG_NT = 256;
constexpr int AMG_TAIL_NT = 1024;              // the one workgroup of the fused tail

// acc = +0.0;  acc = acc + val * v_j over row i's tuples in the operand's order
__device__ __forceinline__ double amg_chain(const uint32_t *ptr, const int32_t *col, const double *val, uint64_t i, const double *v)
{
	double acc = 0.0;
	for (uint32_t k = ptr[i], e = ptr[i + 1]; k < e; ++k) acc = ref_add(acc, ref_mul(val[k], v[(uint32_t)col[k]]));
	return acc;
}

// x'_i of smooth(): x_i + omega * ((b_i - q_i) / d_i)
__device__ __forceinline__ double amg_relax(double x, double b, double q, double d, double omega)
{
	return ref_add(x, ref_mul(omega, ref_div(ref_sub(b, q), d)));
}

// ---------------------------------------------------------------- the level kernels

__global__ void __launch_bounds__(AMG_NT) k_amg_smooth0(const double *__restrict__ b, const double *__restrict__ d, double *__restrict__ x,
	uint64_t n, double omega)
{
	const uint64_t i = (uint64_t)blockIdx.x * AMG_NT + threadIdx.x;
	if (i < n) x[i] = ref_mul(omega, ref_div(b[i], d[i]));
}

// xn = smooth(b, x).  A row above long_min: q_i = +0.0, and xn_i is left to k_amg_long.
__global__ void __launch_bounds__(AMG_NT) k_amg_smooth(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ b, const double *__restrict__ d, const double *__restrict__ x, double *__restrict__ xn, double *__restrict__ q,
	uint64_t n, double omega, uint32_t long_min)
{
	const uint64_t i = (uint64_t)blockIdx.x * AMG_NT + threadIdx.x;
	if (i >= n) return;
	if (ptr[i + 1] - ptr[i] > long_min) { q[i] = 0.0; return; }
	xn[i] = amg_relax(x[i], b[i], amg_chain(ptr, col, val, i, x), d[i], omega);
}

// r = b - S x.  A row above long_min: r_i = +0.0 (the wave kernel adds q_i there, k_amg_long turns it into b_i - q_i).
__global__ void __launch_bounds__(AMG_NT) k_amg_residual(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ b, const double *__restrict__ x, double *__restrict__ r, uint64_t n, uint32_t long_min)
{
	const uint64_t i = (uint64_t)blockIdx.x * AMG_NT + threadIdx.x;
	if (i >= n) return;
	if (ptr[i + 1] - ptr[i] > long_min) { r[i] = 0.0; return; }
	r[i] = ref_sub(b[i], amg_chain(ptr, col, val, i, x));
}

// bc = R r, a lane per coarse row (R's columns are bounded by the fine order at the intake).  A row above long_min: +0.0,
// and the wave kernel adds the chain.
__global__ void __launch_bounds__(AMG_NT) k_amg_restrict(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ r, double *__restrict__ bc, uint64_t nc, uint32_t long_min)
{
	const uint64_t i = (uint64_t)blockIdx.x * AMG_NT + threadIdx.x;
	if (i >= nc) return;
	bc[i] = ptr[i + 1] - ptr[i] > long_min ? 0.0 : amg_chain(ptr, col, val, i, r);
}

// x_i = x_i + (P e)_i, a lane per fine row; ZERO: x is +0.0 (no sweep has written it).  A row above long_min: q_i = +0.0,
// and x_i is left to k_amg_long.
template <bool ZERO>
__global__ void __launch_bounds__(AMG_NT) k_amg_prolong(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ e, double *__restrict__ x, double *__restrict__ q, uint64_t n, uint32_t long_min)
{
	const uint64_t i = (uint64_t)blockIdx.x * AMG_NT + threadIdx.x;
	if (i >= n) return;
	if (ptr[i + 1] - ptr[i] > long_min) { q[i] = 0.0; return; }
	x[i] = ref_add(ZERO ? 0.0 : x[i], amg_chain(ptr, col, val, i, e));
}

// The vector operation of a step for the listed rows, whose chains the wave kernel has put into q
enum { LONG_SMOOTH = 0, LONG_RESIDUAL = 1, LONG_PROLONG = 2, LONG_PROLONG_ZERO = 3 };
template <int WHAT>
__global__ void __launch_bounds__(AMG_NT) k_amg_long(const uint32_t *__restrict__ list, const uint32_t *__restrict__ count, const double *b,
	const double *d, const double *x, double *out, const double *q, double omega)
{
	const uint32_t t = blockIdx.x * AMG_NT + threadIdx.x;
	if (t >= *count) return;
	const uint32_t i = list[t];
	if (WHAT == LONG_SMOOTH) out[i] = amg_relax(x[i], b[i], q[i], d[i], omega);
	else if (WHAT == LONG_RESIDUAL) out[i] = ref_sub(b[i], q[i]);              // (out is q)
	else out[i] = ref_add(WHAT == LONG_PROLONG_ZERO ? 0.0 : x[i], q[i]);      // (out is x)
}

// ---------------------------------------------------------------- the fused tail

// One level as the tail reads it.  x0 is the buffer the level's first sweep (or, without one, its first write) fills.
struct AmgDesc {
	const uint32_t *aptr, *pptr, *rptr;
	const int32_t *acol, *pcol, *rcol;
	const double *aval, *pval, *rval;
	const double *b, *d;             // (the tail writes the b of every level but its first)
	double *x0, *x1, *r;
	uint64_t n;
};

// sweeps s = 0 .. count - 1 from x = +0.0 (count >= 1): where the result is
__device__ double *tail_sweeps0(const AmgDesc *L, uint32_t count, double omega)
{
	const uint64_t n = L->n;
	double *cur = L->x0;
	for (uint64_t i = threadIdx.x; i < n; i += AMG_TAIL_NT) cur[i] = ref_mul(omega, ref_div(L->b[i], L->d[i]));
	__syncthreads();
	for (uint32_t s = 1; s < count; ++s) {                                   // uniform
		double *nxt = cur == L->x0 ? L->x1 : L->x0;
		for (uint64_t i = threadIdx.x; i < n; i += AMG_TAIL_NT)
			nxt[i] = amg_relax(cur[i], L->b[i], amg_chain(L->aptr, L->acol, L->aval, i, cur), L->d[i], omega);
		__syncthreads();
		cur = nxt;
	}
	return cur;
}

// cycle(first, .) over desc[first .. last]: b of level `first` is given, the result is in the buffer amg_final() names
__global__ void __launch_bounds__(AMG_TAIL_NT) k_amg_tail(const AmgDesc *desc, uint32_t first, uint32_t last, uint32_t pre, uint32_t post,
	uint32_t coarse, double omega)
{
	for (uint32_t l = first; l < last; ++l) {                                // down; uniform
		const AmgDesc *L = desc + l, *C = L + 1;
		const double *rs = L->b;
		if (pre) {
			const double *cur = tail_sweeps0(L, pre, omega);
			for (uint64_t i = threadIdx.x; i < L->n; i += AMG_TAIL_NT) L->r[i] = ref_sub(L->b[i], amg_chain(L->aptr, L->acol, L->aval, i, cur));
			__syncthreads();
			rs = L->r;
		}
		double *bc = const_cast<double *>(C->b);
		for (uint64_t i = threadIdx.x; i < C->n; i += AMG_TAIL_NT) bc[i] = amg_chain(L->rptr, L->rcol, L->rval, i, rs);
		__syncthreads();
	}
	const double *e;
	{
		const AmgDesc *L = desc + last;
		if (coarse) e = tail_sweeps0(L, coarse, omega);
		else {
			for (uint64_t i = threadIdx.x; i < L->n; i += AMG_TAIL_NT) L->x0[i] = 0.0;
			__syncthreads();
			e = L->x0;
		}
	}
	for (uint32_t l = last; l-- > first;) {                                  // up; uniform
		const AmgDesc *L = desc + l;
		double *cur = pre == 0 || ((pre - 1) & 1u) == 0 ? L->x0 : L->x1;
		for (uint64_t i = threadIdx.x; i < L->n; i += AMG_TAIL_NT)
			cur[i] = ref_add(pre ? cur[i] : 0.0, amg_chain(L->pptr, L->pcol, L->pval, i, e));
		__syncthreads();
		for (uint32_t s = 0; s < post; ++s) {
			double *nxt = cur == L->x0 ? L->x1 : L->x0;
			for (uint64_t i = threadIdx.x; i < L->n; i += AMG_TAIL_NT)
				nxt[i] = amg_relax(cur[i], L->b[i], amg_chain(L->aptr, L->acol, L->aval, i, cur), L->d[i], omega);
			__syncthreads();
			cur = nxt;
		}
		e = cur;
	}
}

// ---------------------------------------------------------------- host

namespace {

struct AmgLevel {
	RowOperator A, P, R;
	uint64_t n = 0;
	const double *b = nullptr;
	double *x0 = nullptr, *x1 = nullptr, *r = nullptr, *d = nullptr;
};

// The cycle of one call: set up once, then run() as often as the loop asks
struct AmgCycle : PcgPrecond {
	spsamd_ctx *c = nullptr;
	const spsamd_amg_level *in = nullptr;
	uint32_t L = 0, tail = 0;                  // levels; the first level of the fused tail (L: there is none)
	spsamd_amg_params prm = {};
	int policy = 0, zero_nan = 0;
	std::vector<AmgLevel> lv;
	std::vector<AmgDesc> hdesc;
	AmgDesc *desc = nullptr;
	std::vector<std::function<void()>> steps;  // one entry per launch or fill of a cycle
	spsamd_amg_stats st = {};

	// how often the result of level l changes buffers after its first write, and where it ends up
	uint32_t switches(uint32_t l) const { return l == L - 1 ? (prm.coarse ? prm.coarse - 1 : 0) : (prm.pre ? prm.pre - 1 : 0) + prm.post; }
	double *result(uint32_t l) const { return switches(l) & 1u ? lv[l].x1 : lv[l].x0; }

	void take(const spsamd_coo *X, char tr, bool long_rows, RowOperator *op)
	{
		const int lead = tr == 'T' ? 1 : 0;
		ConMat S;
		Prepared *hp = nullptr;
		consolidate_operand(c, X, lead, lead, policy, zero_nan, &S, &hp);
		const uint64_t shape[2] = {X->shape0, X->shape1};
		row_operator(c, S, hp, shape[lead], shape[1 - lead], long_rows, op);
	}

	// S0: levels[0].A as the caller has taken it already, or null.  b -> x of the cycle: device vectors of n_0 entries.
	void build(const RowOperator *S0, const double *b, double *x)
	{
		lv.resize(L);
		const uint32_t rows_max = c->tune.amg_fuse_rows > 0 ? (uint32_t)c->tune.amg_fuse_rows : AMG_FUSE_ROWS;
		tail = L;
		if (c->tune.amg_path == 2) tail = 0;
		else if (c->tune.amg_path != 1)
			while (tail > 0 && in[tail - 1].A->shape0 <= rows_max) --tail;
		for (uint32_t l = 0; l < L; ++l) {
			AmgLevel &v = lv[l];
			const bool wave = l < tail;                                        // the tail walks every row itself
			v.n = in[l].A->shape0;
			if (l == 0 && S0) v.A = *S0;
			else take(in[l].A, in[l].transpose_A, wave, &v.A);
			if (l + 1 < L) {
				take(in[l].P, in[l].transpose_P, wave, &v.P);
				take(in[l].R, in[l].transpose_R, wave, &v.R);
			}
			const uint64_t na = v.n ? v.n : 1;
			v.d = c->arena.get<double>(na);
			if (v.n && v.A.nnz) reduce_diag_dense(c, v.A.ptr, v.A.col, v.A.val, v.n, v.d);
			else fill_zero(c, v.d, na * sizeof(double));
			v.x0 = l == 0 ? x : c->arena.get<double>(na);
			v.x1 = c->arena.get<double>(na);
			v.r = c->arena.get<double>(na);
			v.b = l == 0 ? b : c->arena.get<double>(na);
			st.rows[l] = v.n; st.nnz[l] = v.A.nnz;
			if (wave) st.long_rows += (uint64_t)v.A.nlong + v.P.nlong + v.R.nlong;
		}
		if (switches(0) & 1u) std::swap(lv[0].x0, lv[0].x1);                   // level 0's result is x
		uint64_t total = 0;
		for (uint32_t l = 0; l < L; ++l) total += st.nnz[l];
		st.levels = L; st.fused_levels = L - tail;
		st.operator_complexity = st.nnz[0] ? (double)total / (double)st.nnz[0] : 0.0;
		if (tail < L) {
			hdesc.resize(L);
			for (uint32_t l = 0; l < L; ++l) {
				const AmgLevel &v = lv[l];
				hdesc[l] = AmgDesc{v.A.ptr, v.P.ptr, v.R.ptr, v.A.col, v.P.col, v.R.col, v.A.val, v.P.val, v.R.val, v.b, v.d, v.x0, v.x1, v.r, v.n};
			}
			desc = c->arena.get<AmgDesc>(L);
			SPS_HIP(hipMemcpyAsync(desc, hdesc.data(), L * sizeof(AmgDesc), hipMemcpyHostToDevice, c->stream));
		}
		plan();
		st.launches_per_cycle = steps.size();
	}

	// ---- the steps of a level outside the tail (nothing here runs before run())
	void long_chain(const RowOperator &op, const double *in_v, double *q)
	{
		spsamd_ctx *cc = c;
		steps.push_back([=] { spmm_long_rows(cc, op.m, op.list, op.count, in_v, 1, q, 1, 1); });
	}
	template <int WHAT> void long_finish(const RowOperator &op, const double *b, const double *d, const double *x, double *out, const double *q)
	{
		hipStream_t s = c->stream;
		const double omega = prm.omega;
		steps.push_back([=] {
			k_amg_long<WHAT><<<dim3(grid_for(op.nlong, AMG_NT)), dim3(AMG_NT), 0, s>>>(op.list, op.count, b, d, x, out, q, omega);
			SPS_LAUNCH_CHECK();
		});
	}
	// x = +0.0 and `count` sweeps: where the result is
	double *sweeps0(const AmgLevel &v, uint32_t count)
	{
		hipStream_t s = c->stream;
		const double omega = prm.omega;
		const uint64_t n = v.n;
		double *cur = v.x0;
		const double *b = v.b, *d = v.d;
		if (!count) {
			spsamd_ctx *cc = c;
			steps.push_back([=] { fill_zero(cc, cur, n * sizeof(double)); });
			return cur;
		}
		steps.push_back([=] {
			k_amg_smooth0<<<dim3(grid_for(n, AMG_NT)), dim3(AMG_NT), 0, s>>>(b, d, cur, n, omega);
			SPS_LAUNCH_CHECK();
		});
		for (uint32_t k = 1; k < count; ++k) cur = sweep(v, cur);
		return cur;
	}
	double *sweep(const AmgLevel &v, double *cur)
	{
		hipStream_t s = c->stream;
		const double omega = prm.omega;
		const RowOperator A = v.A;
		const uint64_t n = v.n;
		double *nxt = cur == v.x0 ? v.x1 : v.x0, *q = v.r;
		const double *b = v.b, *d = v.d;
		steps.push_back([=] {
			k_amg_smooth<<<dim3(grid_for(n, AMG_NT)), dim3(AMG_NT), 0, s>>>(A.ptr, A.col, A.val, b, d, cur, nxt, q, n, omega, A.long_min);
			SPS_LAUNCH_CHECK();
		});
		if (A.nlong) {
			long_chain(A, cur, q);
			long_finish<LONG_SMOOTH>(A, b, d, cur, nxt, q);
		}
		return nxt;
	}

	void plan()
	{
		hipStream_t s = c->stream;
		const uint32_t top = std::min(tail, L - 1);                            // the levels below `top` go down and up here
		for (uint32_t l = 0; l < top; ++l) {
			const AmgLevel &v = lv[l], &w = lv[l + 1];
			const double *rs = v.b;
			if (v.n && prm.pre) {
				const double *cur = sweeps0(v, prm.pre), *b = v.b;
				double *r = v.r;
				const RowOperator A = v.A;
				const uint64_t n = v.n;
				steps.push_back([=] {
					k_amg_residual<<<dim3(grid_for(n, AMG_NT)), dim3(AMG_NT), 0, s>>>(A.ptr, A.col, A.val, b, cur, r, n, A.long_min);
					SPS_LAUNCH_CHECK();
				});
				if (A.nlong) {
					long_chain(A, cur, r);
					long_finish<LONG_RESIDUAL>(A, b, nullptr, nullptr, r, r);
				}
				rs = r;
			}
			if (w.n) {
				const RowOperator R = v.R;
				double *bc = const_cast<double *>(w.b);
				const uint64_t nc = w.n;
				steps.push_back([=] {
					k_amg_restrict<<<dim3(grid_for(nc, AMG_NT)), dim3(AMG_NT), 0, s>>>(R.ptr, R.col, R.val, rs, bc, nc, R.long_min);
					SPS_LAUNCH_CHECK();
				});
				if (R.nlong) long_chain(R, rs, bc);
			}
		}
		if (tail < L) {
			const AmgDesc *dd = desc;
			const uint32_t first = tail, last = L - 1;
			const spsamd_amg_params p = prm;
			if (lv[first].n)
				steps.push_back([=] {
					k_amg_tail<<<dim3(1), dim3(AMG_TAIL_NT), 0, s>>>(dd, first, last, p.pre, p.post, p.coarse, p.omega);
					SPS_LAUNCH_CHECK();
				});
		} else if (lv[L - 1].n) sweeps0(lv[L - 1], prm.coarse);
		for (uint32_t l = top; l-- > 0;) {
			const AmgLevel &v = lv[l];
			if (!v.n) continue;
			const double *e = result(l + 1);
			const RowOperator P = v.P;
			const uint64_t n = v.n;
			double *cur = prm.pre == 0 || ((prm.pre - 1) & 1u) == 0 ? v.x0 : v.x1, *q = v.r;
			const bool zero = prm.pre == 0;
			steps.push_back([=] {
				if (zero) k_amg_prolong<true><<<dim3(grid_for(n, AMG_NT)), dim3(AMG_NT), 0, s>>>(P.ptr, P.col, P.val, e, cur, q, n, P.long_min);
				else k_amg_prolong<false><<<dim3(grid_for(n, AMG_NT)), dim3(AMG_NT), 0, s>>>(P.ptr, P.col, P.val, e, cur, q, n, P.long_min);
				SPS_LAUNCH_CHECK();
			});
			if (P.nlong) {
				long_chain(P, e, q);
				if (zero) long_finish<LONG_PROLONG_ZERO>(P, nullptr, nullptr, cur, cur, q);
				else long_finish<LONG_PROLONG>(P, nullptr, nullptr, cur, cur, q);
			}
			for (uint32_t k = 0; k < prm.post; ++k) cur = sweep(v, cur);
		}
	}

	uint64_t run()
	{
		for (auto &f : steps) f();
		return steps.size();
	}

	// ---- the hook of the conjugate gradient loop
	void setup(spsamd_ctx *, const RowOperator &S, const double *r, double *z) override { build(&S, r, z); }
	uint64_t apply() override { return run(); }
};

// What both entry points refuse before any work; returns n_0
uint64_t amg_check(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params, const double *b,
	double *x, int mem, int duplicate_policy)
{
	if (!levels || !params) throw Error{SPSAMD_EINVAL, "null levels or params"};
	if (nlevels < 1 || nlevels > (size_t)AMG_MAX_LEVELS) throw Error{SPSAMD_EINVAL, "nlevels must be 1 .. 32"};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of b and x must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	if (params->omega - params->omega != 0.0) throw Error{SPSAMD_EINVAL, "omega must be finite"};
	for (size_t l = 0; l < nlevels; ++l) {
		const spsamd_amg_level &v = levels[l];
		const std::string at = " (level " + std::to_string(l) + ")";
		if (!v.A) throw Error{SPSAMD_EINVAL, "null level operator" + at};
		const bool last = l + 1 == nlevels;
		if (last ? (v.P || v.R) : (!v.P || !v.R)) throw Error{SPSAMD_EINVAL, (last ? "P and R must be NULL on the last level" : "P and R are needed below the last level") + at};
	}
	for (size_t l = 0; l < nlevels; ++l) {
		const spsamd_amg_level &v = levels[l];
		const std::string at = " (level " + std::to_string(l) + ")";
		if (v.A->shape0 != v.A->shape1) throw Error{SPSAMD_EDIM, "op(A) must be square" + at};
		if (l + 1 == nlevels) break;
		const uint64_t n = v.A->shape0, nc = levels[l + 1].A->shape0;
		const bool tp = v.transpose_P == 'T', tr = v.transpose_R == 'T';
		if ((tp ? v.P->shape1 : v.P->shape0) != n || (tp ? v.P->shape0 : v.P->shape1) != nc) throw Error{SPSAMD_EDIM, "op(P) must be n_l x n_{l+1}" + at};
		if ((tr ? v.R->shape1 : v.R->shape0) != nc || (tr ? v.R->shape0 : v.R->shape1) != n) throw Error{SPSAMD_EDIM, "op(R) must be n_{l+1} x n_l" + at};
	}
	const uint64_t n = levels[0].A->shape0, vbytes = n * sizeof(double);
	if (n && (!b || !x)) throw Error{SPSAMD_EINVAL, "null b or x"};
	if (ranges_overlap(x, vbytes, b, vbytes)) throw Error{SPSAMD_EINVAL, "x and b overlap"};
	for (size_t l = 0; l < nlevels; ++l) {
		check_vector_overlap(c, levels[l].A, "A", x, vbytes);
		if (levels[l].P) check_vector_overlap(c, levels[l].P, "P", x, vbytes);
		if (levels[l].R) check_vector_overlap(c, levels[l].R, "R", x, vbytes);
	}
	if (mem == SPSAMD_MEM_DEVICE && in_output_sets(c, x, vbytes)) throw Error{SPSAMD_EINVAL, "x lies in an output set of the context"};
	return n;
}

void amg_init(AmgCycle &cy, spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params,
	int duplicate_policy, int zero_nan)
{
	cy.c = c; cy.in = levels; cy.L = (uint32_t)nlevels; cy.prm = *params; cy.policy = duplicate_policy; cy.zero_nan = zero_nan;
}

} // namespace

int amg_apply(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params, const double *b,
	double *x, int mem, int duplicate_policy, int zero_nan, spsamd_amg_stats *stats, spsamd_result *res)
{
	const uint64_t n = amg_check(c, levels, nlevels, params, b, x, mem, duplicate_policy);
	std::memset(res, 0, sizeof(*res));
	if (stats) std::memset(stats, 0, sizeof(*stats));
	res->shape0 = res->shape1 = n;
	if (!n) return SPSAMD_OK;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	AmgCycle cy;
	amg_init(cy, c, levels, nlevels, params, duplicate_policy, zero_nan);
	const double *db = to_device(c, b, n, mem);
	double *dx = mem == SPSAMD_MEM_HOST ? c->arena.get<double>(n) : x;
	cy.build(nullptr, db, dx);
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));
	cy.run();
	if (mem == SPSAMD_MEM_HOST) SPS_HIP(hipMemcpyAsync(x, dx, n * sizeof(double), hipMemcpyDeviceToHost, st));
	finish_call(c, res);
	res->nnz_a = cy.st.nnz[0];
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_BEGIN], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	if (stats) {
		*stats = cy.st;
		stats->ms_setup = res->ms_symbolic; stats->ms_cycle = res->ms_numeric;
	}
	return SPSAMD_OK;
}

int solve_pcg_amg(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params, const double *b,
	double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity, int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats, spsamd_amg_stats *astats, spsamd_result *res)
{
	amg_check(c, levels, nlevels, params, b, x, mem, duplicate_policy);
	if (astats) std::memset(astats, 0, sizeof(*astats));
	AmgCycle cy;
	amg_init(cy, c, levels, nlevels, params, duplicate_policy, zero_nan);
	const int rc = pcg_solve(c, levels[0].A, levels[0].transpose_A, PCG_PRECOND_HOOK, nullptr, '.', b, x, mem, tol, max_iter, hist_host,
		hist_capacity, duplicate_policy, zero_nan, stats, res, &cy);
	if (astats && cy.st.levels) *astats = cy.st;
	return rc;
}

} // namespace spsamd
