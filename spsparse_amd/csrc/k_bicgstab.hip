// k_bicgstab.hip -- A x = b for an unsymmetric A by right-preconditioned BiCGStab, the whole loop on the device
// (spsamd_solve_bicgstab, include/spsparse_amd.h).
//
// The shape is k_krylov.hip's: S = op(A) and F = op(M) as consolidate_operand() hands them over, every returned bit defined
// by the loop of the header, every dot product in the one reduction shape of krylov_dev.h (a wave per chunk of 1024
// elements, no LDS and no barrier at level 0).  An iteration has five dots in four groups, and each group rides in the
// kernel that produces its vector:
//     v = A y          with the partials of dot(rhat, v)              k_bicg_spmv<1>     then k_bicg_finish<RV>: alpha
//     s = r - alpha v  with the partials of dot(s, s)                 k_bicg_half        then <SS>: the half-step decision
//     t = A z          with the partials of dot(t, s) and dot(t, t)   k_bicg_spmv<2>     then <TS_TT>: omega
//     x, r             with the partials of dot(r, r), dot(rhat, r)   k_bicg_update<0>   then <RR_RHO>: k, hist, stops, beta
// Two dots of one pass go to two partial arrays and are folded one after the other by the one workgroup of the finish
// kernel.  Rows above spmm_long_min are left to k_spmm.hip's wave kernel as in k_krylov.hip, and k_bicg_dot_rows redoes the
// partials -- of both arrays behind the second SpMV -- of the chunks that hold one.
//
// The state word (BicgState, a PcgState with omega and ss) has one value more than the loop of k_krylov.hip: BICG_HALF, from
// the SS finish that takes the half-step exit until the RR_RHO finish of the same iteration.  In it k_bicg_update does
// x = x + alpha y and nothing else, the RR_RHO finish sets rr = ss, k, hist and CONVERGED, and every other kernel is idle.
// Every kernel of this file that writes x, r, p, k, the history or a scalar reads the state first and does nothing unless
// it is RUNNING (or HALF, for those two).  y, z, v, s and t are scratch after the stop.  No kernel reads what another
// workgroup wrote in the same launch.
#include "krylov_dev.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

constexpr int32_t BICG_HALF = -2;              // BicgState::state between the half-step decision and the x update that goes with it

struct BicgState : PcgState {                  // (rz holds rho; pq is not used)
	double omega, ss;
};

// chunk_partial for two folds of one pass: term(e, &t0, &t1) gives element e's term of each
template <class Term>
__device__ __forceinline__ void chunk_partial2(uint64_t g, uint64_t n, Term term, double *a0, double *a1)
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
	double t0[PCG_CHUNK / 64], t1[PCG_CHUNK / 64];
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k) {
		const uint64_t e = base + (uint64_t)k * 64;
		t0[k] = t1[k] = 0.0;
		if (e < n) term(e, &t0[k], &t1[k]);
	}
	double a = 0.0, b = 0.0;
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k)
		if (base + (uint64_t)k * 64 < n) { a = ref_add(a, t0[k]); b = ref_add(b, t1[k]); }
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		const double oa = __shfl_down(a, s, 64), ob = __shfl_down(b, s, 64);
		if (lane_id() < (unsigned)s) { a = ref_add(a, oa); b = ref_add(b, ob); }
	}
	*a0 = a; *a1 = b;
}

// ---------------------------------------------------------------- level 0: the vector kernels

__global__ void __launch_bounds__(PCG_NT) k_bicg_dot(const double *u, const double *w, uint64_t n, double *__restrict__ part, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	const double a = chunk_partial(g, n, [&](uint64_t e) { return ref_mul(u[e], w[e]); });
	if (lane_id() == 0) part[g] = a;
}

// r = b - q (the set-up's residual), and the partials of dot(r, r)
template <bool DOT>
__global__ void __launch_bounds__(PCG_NT) k_bicg_residual(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r,
	uint64_t n, double *__restrict__ part)
{
	uint64_t g;
	if (!my_chunk(n, &g)) return;
	const double a = chunk_partial(g, n, [&](uint64_t e) { const double v = ref_sub(b[e], q[e]); r[e] = v; return DOT ? ref_mul(v, v) : 0.0; });
	if (DOT && lane_id() == 0) part[g] = a;
}

// out = in / d (y = p / d and z = s / d: no dot follows either)
__global__ void __launch_bounds__(PCG_NT) k_bicg_jacobi(const double *__restrict__ in, const double *__restrict__ d, double *__restrict__ out,
	uint64_t n, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	(void)chunk_partial(g, n, [&](uint64_t e) { out[e] = ref_div(in[e], d[e]); return 0.0; });
}

// row i's serial chain over S; +0.0 for a row of more than long_min tuples (k_spmm.hip's wave kernel adds its chain in the
// next launch)
__device__ __forceinline__ double bicg_row(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ in, uint64_t i, uint32_t long_min)
{
	double acc = 0.0;
	const uint32_t b = ptr[i], e = ptr[i + 1];
	if (e - b <= long_min)
		for (uint32_t k = b; k < e; ++k) acc = ref_add(acc, ref_mul(val[k], in[(uint32_t)col[k]]));
	return acc;
}

// out = S in.  NDOT 1: and the partials of dot(u, out) (v = A y with rhat) | 2: of dot(out, u) and dot(out, out) (t = A z
// with s).  A lane walks the 16 rows 64 apart that the fold gives it.  u may be `in` (z is s without a preconditioner).
template <int NDOT>
__global__ void __launch_bounds__(PCG_NT) k_bicg_spmv(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *in, double *__restrict__ out, uint64_t n, uint32_t long_min, const double *u, double *__restrict__ part0,
	double *__restrict__ part1, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	if (NDOT == 2) {
		double a0, a1;
		chunk_partial2(g, n, [&](uint64_t i, double *t0, double *t1) {
			const double acc = bicg_row(ptr, col, val, in, i, long_min);
			out[i] = acc;
			*t0 = ref_mul(acc, u[i]); *t1 = ref_mul(acc, acc);
		}, &a0, &a1);
		if (lane_id() == 0) { part0[g] = a0; part1[g] = a1; }
	} else {
		const double a = chunk_partial(g, n, [&](uint64_t i) {
			const double acc = bicg_row(ptr, col, val, in, i, long_min);
			out[i] = acc;
			return NDOT ? ref_mul(u[i], acc) : 0.0;
		});
		if (NDOT && lane_id() == 0) part0[g] = a;
	}
}

// The partials of dot(u0, w0) -- and of dot(u1, w1) where u1 is given -- for the chunks that hold a listed row, a wave per
// listed row (two rows of one chunk store the same value twice)
__global__ void __launch_bounds__(64) k_bicg_dot_rows(const double *u0, const double *w0, double *part0, const double *u1, const double *w1,
	double *part1, uint64_t n, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count, const PcgState *st)
{
	if (stopped(st)) return;
	const uint32_t m = *count;
	for (uint32_t r = blockIdx.x; r < m; r += gridDim.x) {               // uniform
		const uint64_t g = list[r] / PCG_CHUNK;
		const double a = chunk_partial(g, n, [&](uint64_t e) { return ref_mul(u0[e], w0[e]); });
		if (lane_id() == 0) part0[g] = a;
		if (u1) {
			const double b = chunk_partial(g, n, [&](uint64_t e) { return ref_mul(u1[e], w1[e]); });
			if (lane_id() == 0) part1[g] = b;
		}
	}
}

// p = r (k == 0), else p = r + beta (p - omega v).  No fold here, so nothing fixes which lane owns which element: VEC takes
// two neighbouring elements per thread in 16-byte loads and stores (r, v and p 16-byte aligned), the odd last element alone.
__device__ __forceinline__ double bicg_dir(double r, double p, double v, double beta, double omega)
{
	return ref_add(r, ref_mul(beta, ref_sub(p, ref_mul(omega, v))));
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_bicg_direction(const double *__restrict__ r, const double *__restrict__ v, double *__restrict__ p,
	uint64_t n, const BicgState *st)
{
	if (stopped(st)) return;
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool first = st->k == 0;
	const double beta = st->beta, omega = st->omega;
	if (VEC) {
		const uint64_t e = 2 * t;
		if (e + 1 < n) {
			const double2 rr = *reinterpret_cast<const double2 *>(r + e);
			double2 pp = rr;
			if (!first) {
				const double2 vv = *reinterpret_cast<const double2 *>(v + e);
				pp = *reinterpret_cast<const double2 *>(p + e);
				pp.x = bicg_dir(rr.x, pp.x, vv.x, beta, omega);
				pp.y = bicg_dir(rr.y, pp.y, vv.y, beta, omega);
			}
			*reinterpret_cast<double2 *>(p + e) = pp;
		} else if (e < n) p[e] = first ? r[e] : bicg_dir(r[e], p[e], v[e], beta, omega);
	} else if (t < n) p[t] = first ? r[t] : bicg_dir(r[t], p[t], v[t], beta, omega);
}

// s = r - alpha v, and the partials of dot(s, s)
template <bool DOT>
__global__ void __launch_bounds__(PCG_NT) k_bicg_half(const double *__restrict__ r, const double *__restrict__ v, double *__restrict__ s,
	uint64_t n, double *__restrict__ part, const BicgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	const double alpha = st->alpha;
	const double a = chunk_partial(g, n, [&](uint64_t e) { const double w = ref_sub(r[e], ref_mul(alpha, v[e])); s[e] = w; return DOT ? ref_mul(w, w) : 0.0; });
	if (DOT && lane_id() == 0) part[g] = a;
}

// WHAT 0: x = (x + alpha y) + omega z, r = s - omega t and the partials of dot(r, r) and dot(rhat, r) | 1: x alone |
// 2: r alone.  After a taken half-step exit (BICG_HALF) WHAT 0 and 1 do x = x + alpha y and nothing else, WHAT 2 nothing.
// y may be p and z may be s (no preconditioner): both are only read.
template <int WHAT>
__global__ void __launch_bounds__(PCG_NT) k_bicg_update(double *__restrict__ x, const double *y, const double *z, double *__restrict__ r,
	const double *s, const double *__restrict__ t, const double *__restrict__ rhat, uint64_t n, double *__restrict__ part0,
	double *__restrict__ part1, const BicgState *st)
{
	uint64_t g;
	const int32_t state = st->state;
	if ((state != PCG_RUNNING && (state != BICG_HALF || WHAT == 2)) || !my_chunk(n, &g)) return;   // (the state: uniform)
	const double alpha = st->alpha, omega = st->omega;
	if (state == BICG_HALF) {
		(void)chunk_partial(g, n, [&](uint64_t e) { x[e] = ref_add(x[e], ref_mul(alpha, y[e])); return 0.0; });
		return;
	}
	if (WHAT == 1) {
		(void)chunk_partial(g, n, [&](uint64_t e) { x[e] = ref_add(ref_add(x[e], ref_mul(alpha, y[e])), ref_mul(omega, z[e])); return 0.0; });
	} else if (WHAT == 2) {
		(void)chunk_partial(g, n, [&](uint64_t e) { r[e] = ref_sub(s[e], ref_mul(omega, t[e])); return 0.0; });
	} else {
		double a0, a1;
		chunk_partial2(g, n, [&](uint64_t e, double *t0, double *t1) {
			x[e] = ref_add(ref_add(x[e], ref_mul(alpha, y[e])), ref_mul(omega, z[e]));
			const double w = ref_sub(s[e], ref_mul(omega, t[e]));
			r[e] = w;
			*t0 = ref_mul(w, w); *t1 = ref_mul(rhat[e], w);
		}, &a0, &a1);
		if (lane_id() == 0) { part0[g] = a0; part1[g] = a1; }
	}
}

__global__ void k_bicg_init(BicgState *st, unsigned long long max_iter, unsigned long long hist_cap)
{
	BicgState s = {};
	s.max_iter = max_iter; s.hist_cap = hist_cap; s.state = PCG_RUNNING;
	*st = s;
}

// ---------------------------------------------------------------- levels 1 and up, the scalars, the stop tests

enum { BFIN_BB = 0, BFIN_RR0 = 1, BFIN_RV = 2, BFIN_SS = 3, BFIN_TS_TT = 4, BFIN_RR_RHO = 5 };

// k_pcg_finish's design: one workgroup, a wave per chunk of partials, a barrier per level, then thread 0.  TS_TT and RR_RHO
// fold part0, then part1 (each into an LDS word of its own: a fast wave may finish the second fold's only chunk while a slow
// one still reads the first fold's value).
template <int KIND>
__global__ void __launch_bounds__(PCG_FINISH_NT) k_bicg_finish(const double *part0, const double *part1, uint64_t c0, double *b0, double *b1,
	BicgState *st, double *__restrict__ hist, double tol2)
{
	__shared__ double s_out[2];
	const int32_t state = st->state;
	__syncthreads();                                                 // every thread has read the state before thread 0 may set it
	if (KIND == BFIN_RR_RHO && state == BICG_HALF) {                 // uniform: the half-step exit, after its x update
		if (threadIdx.x != 0) return;
		const unsigned long long k = st->k + 1;
		st->k = k; st->rr = st->ss;
		if (k < st->hist_cap) hist[k] = st->ss;
		st->state = SPSAMD_PCG_CONVERGED;
		return;
	}
	if (KIND >= BFIN_RV && state != PCG_RUNNING) return;             // uniform
	const double v = c0 == 1 ? part0[0] : block_fold(part0, c0, b0, b1, &s_out[0]);
	double w = 0.0;
	if (KIND == BFIN_TS_TT || KIND == BFIN_RR_RHO) w = c0 == 1 ? part1[0] : block_fold(part1, c0, b0, b1, &s_out[1]);
	if (threadIdx.x != 0) return;
	if (KIND == BFIN_BB) { st->bb = v; st->thresh = ref_mul(tol2, v); return; }
	if (KIND == BFIN_RV) {
		if (!pcg_usable(v)) st->state = SPSAMD_PCG_BREAKDOWN;
		else st->alpha = ref_div(st->rz, v);
		return;
	}
	if (KIND == BFIN_SS) {
		st->ss = v;
		if (v <= st->thresh) st->state = BICG_HALF;                  // (a NaN compares false)
		return;
	}
	if (KIND == BFIN_TS_TT) {                                        // v = ts, w = tt
		if (!pcg_usable(w)) st->state = SPSAMD_PCG_BREAKDOWN;
		else st->omega = ref_div(v, w);
		return;
	}
	// the end of an iteration (v = rr, w = rho') or of the set-up (v = rr0 = rho'), and the stop tests of the loop's top
	unsigned long long k = 0;
	double rho1 = v;
	if (KIND == BFIN_RR0) st->rr0 = v;
	else { k = st->k + 1; st->k = k; rho1 = w; }
	st->rr = v;
	if (k < st->hist_cap) hist[k] = v;
	if (v <= st->thresh) st->state = SPSAMD_PCG_CONVERGED;               // (a NaN compares false)
	else if (k == st->max_iter) st->state = SPSAMD_PCG_MAXITER;
	else if (!pcg_usable(rho1)) st->state = SPSAMD_PCG_BREAKDOWN;
	else if (KIND == BFIN_RR_RHO && !pcg_usable(st->omega)) st->state = SPSAMD_PCG_BREAKDOWN;
	else {
		if (KIND == BFIN_RR_RHO) st->beta = ref_mul(ref_div(rho1, st->rz), ref_div(st->alpha, st->omega));
		st->rz = rho1;
	}
}

// ---------------------------------------------------------------- host

namespace {

struct Bicg {
	spsamd_ctx *c;
	uint64_t n, c0;
	bool unfused;
	double *part0, *part1, *b0, *b1, *hist;
	BicgState *st;
	uint64_t launches = 0;
	unsigned chunk_grid() const { return (unsigned)((c0 + PCG_NT / 64 - 1) / (PCG_NT / 64)); }

	void dot(const double *u, const double *w, double *part, const PcgState *pred)
	{
		k_bicg_dot<<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(u, w, n, part, pred);
		SPS_LAUNCH_CHECK();
		++launches;
	}
	template <int KIND> void finish(double tol2 = 0.0)
	{
		k_bicg_finish<KIND><<<dim3(1), dim3(PCG_FINISH_NT), 0, c->stream>>>(part0, part1, c0, b0, b1, st, hist, tol2);
		SPS_LAUNCH_CHECK();
		++launches;
	}
};

} // namespace

// out = S in.  ndot 1: + the partials of dot(u, out) in part0 | 2: of dot(out, u) in part0 and dot(out, out) in part1.
// Nothing is allocated here: it runs twice per iteration.
static void bicg_spmv(Bicg &k, const RowOperator &op, const double *in, double *out, int ndot, const double *u, const PcgState *pred)
{
	spsamd_ctx *c = k.c;
	const int fused = k.unfused ? 0 : ndot;
	const dim3 grid(k.chunk_grid()), nt(PCG_NT);
	if (fused == 2) k_bicg_spmv<2><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, k.n, op.long_min, u, k.part0, k.part1, pred);
	else if (fused == 1) k_bicg_spmv<1><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, k.n, op.long_min, u, k.part0, k.part1, pred);
	else k_bicg_spmv<0><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, k.n, op.long_min, u, k.part0, k.part1, pred);
	SPS_LAUNCH_CHECK();
	++k.launches;
	if (op.nlong) {
		spmm_long_rows(c, op.m, op.list, op.count, in, 1, out, 1, 1);
		++k.launches;
	}
	if (!ndot) return;
	const double *u0 = ndot == 1 ? u : out, *w0 = ndot == 1 ? out : u;
	if (!fused || op.nlong > k.c0) {                                     // (more long rows than chunks: every chunk once instead)
		k.dot(u0, w0, k.part0, pred);
		if (ndot == 2) k.dot(out, out, k.part1, pred);
	} else if (op.nlong) {
		k_bicg_dot_rows<<<dim3(std::min<unsigned>(op.nlong, (unsigned)c->num_cu * 8)), dim3(64), 0, c->stream>>>(u0, w0, k.part0,
			ndot == 2 ? out : nullptr, out, k.part1, k.n, op.list, op.count, pred);
		SPS_LAUNCH_CHECK();
		++k.launches;
	}
}

int solve_bicgstab(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	// ---- the checks of spsamd_solve_pcg, in its order
	if (precond < SPSAMD_PRECOND_NONE || precond > SPSAMD_PRECOND_LU) throw Error{SPSAMD_EINVAL, "precond must be SPSAMD_PRECOND_NONE, _JACOBI or _LU"};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of b and x must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	if (!(tol >= 0.0) || tol - tol != 0.0) throw Error{SPSAMD_EINVAL, "tol must be finite and not negative"};
	if ((precond == SPSAMD_PRECOND_LU) != (M != nullptr)) throw Error{SPSAMD_EINVAL, "M goes with SPSAMD_PRECOND_LU, and only with it"};
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	const int lead = transpose == 'T' ? 1 : 0, lead_m = transpose_M == 'T' ? 1 : 0;
	const uint64_t n = A->shape0;
	if (A->shape0 != A->shape1) throw Error{SPSAMD_EDIM, "op(A) must be square"};
	if (M && (M->shape0 != M->shape1 || M->shape0 != n)) throw Error{SPSAMD_EDIM, "op(M) must be square and of op(A)'s order"};
	if (n && (!b || !x)) throw Error{SPSAMD_EINVAL, "null b or x"};
	const uint64_t vbytes = n * sizeof(double);
	if (ranges_overlap(x, vbytes, b, vbytes)) throw Error{SPSAMD_EINVAL, "x and b overlap"};
	check_vector_overlap(c, A, "A", x, vbytes);
	if (M) check_vector_overlap(c, M, "M", x, vbytes);
	if (mem == SPSAMD_MEM_DEVICE && in_output_sets(c, x, vbytes)) throw Error{SPSAMD_EINVAL, "x lies in an output set of the context"};

	std::memset(res, 0, sizeof(*res));
	if (stats) std::memset(stats, 0, sizeof(*stats));
	res->shape0 = res->shape1 = n;
	if (!n) {                                                        // every dot is the fold of nothing: rr = +0.0 <= thresh
		if (hist_host && hist_capacity) hist_host[0] = 0.0;
		return SPSAMD_OK;
	}

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	ConMat S, F;
	Prepared *hpa = nullptr, *hpm = nullptr;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S, &hpa);
	if (M) consolidate_operand(c, M, lead_m, lead_m, duplicate_policy, zero_nan, &F, &hpm);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	res->nnz_a = S.nnz;
	res->nnz_b = M ? F.nnz : 0;

	Bicg k;
	k.c = c; k.n = n; k.c0 = (n + PCG_CHUNK - 1) / PCG_CHUNK; k.unfused = c->tune.pcg_fuse == 1;
	const uint64_t c1 = (k.c0 + PCG_CHUNK - 1) / PCG_CHUNK;
	k.part0 = c->arena.get<double>(k.c0); k.part1 = c->arena.get<double>(k.c0);
	k.b0 = c->arena.get<double>(c1); k.b1 = c->arena.get<double>(c1);
	k.st = c->arena.get<BicgState>(1);
	const uint64_t hcap = !hist_host ? 0 : std::min<uint64_t>(hist_capacity, max_iter == ~0ull ? max_iter : max_iter + 1);
	k.hist = hcap ? c->arena.get<double>(hcap) : nullptr;

	// ---- the operator: S's row pointer; the long rows' list and the packed rows of k_spmm.hip only where there is a long row
	RowOperator op;
	row_operator(c, S, hpa, n, n, true, &op);

	// ---- the preconditioner
	double *diag = nullptr;
	RowOperator fop;
	TriView tl = {}, tu = {};
	SolveSchedule local[2], *sched[2] = {nullptr, nullptr};
	uint32_t analyses = 0;
	if (precond == SPSAMD_PRECOND_JACOBI) {
		diag = c->arena.get<double>(n);
		if (S.nnz) reduce_diag_dense(c, op.ptr, S.col, S.val, n, diag);
		else fill_zero(c, diag, vbytes);
	} else if (precond == SPSAMD_PRECOND_LU) {
		row_operator(c, F, hpm, n, n, false, &fop);                      // (F's row pointer; the solves walk its rows themselves)
		tl.ptr = fop.ptr;
		tl.col = F.col; tl.val = F.val; tl.n = n; tl.upper = 0; tl.unit = 1;
		tu = tl; tu.upper = 1; tu.unit = 0;
		const TriView *tv[2] = {&tl, &tu};
		for (int s = 0; s < 2; ++s) {
			const bool kept = hpm && hpm->owns;
			sched[s] = kept ? &hpm->solve[s == 0 ? SPSAMD_TRI_LOWER : SPSAMD_TRI_UPPER][s == 0 ? SPSAMD_DIAG_UNIT : SPSAMD_DIAG_NONUNIT] : &local[s];
			if (sched[s]->built) continue;
			uint64_t peel[2] = {0, 0};
			try { analyse(c, *tv[s], kept ? hpm : nullptr, sched[s], peel); }
			catch (...) { *sched[s] = SolveSchedule(); throw; }
			++analyses;
		}
	}

	// ---- the vectors
	const double *db = to_device(c, b, n, mem);
	double *dx = x;
	if (mem == SPSAMD_MEM_HOST) { dx = c->arena.get<double>(n); SPS_HIP(hipMemcpyAsync(dx, x, vbytes, hipMemcpyHostToDevice, st)); }
	double *r = c->arena.get<double>(n), *rhat = c->arena.get<double>(n), *p = c->arena.get<double>(n), *v = c->arena.get<double>(n);
	double *s = c->arena.get<double>(n), *t = c->arena.get<double>(n);
	double *y = precond == SPSAMD_PRECOND_NONE ? p : c->arena.get<double>(n);
	double *z = precond == SPSAMD_PRECOND_NONE ? s : c->arena.get<double>(n);
	const bool vec = (((uintptr_t)r | (uintptr_t)v | (uintptr_t)p) & 15u) == 0;
	const dim3 grid(k.chunk_grid()), nt(PCG_NT);

	// ---- bb, thresh; r = b - A x, rhat, rr0, hist[0], the stop tests before the first iteration
	k_bicg_init<<<dim3(1), dim3(1), 0, st>>>(k.st, max_iter, hcap);
	SPS_LAUNCH_CHECK();
	k.dot(db, db, k.part0, nullptr);
	k.finish<BFIN_BB>(tol * tol);
	bicg_spmv(k, op, dx, v, 0, nullptr, nullptr);
	if (k.unfused) {
		k_bicg_residual<false><<<grid, nt, 0, st>>>(db, v, r, n, k.part0);
		SPS_LAUNCH_CHECK();
		k.dot(r, r, k.part0, nullptr);
	} else {
		k_bicg_residual<true><<<grid, nt, 0, st>>>(db, v, r, n, k.part0);
		SPS_LAUNCH_CHECK();
	}
	SPS_HIP(hipMemcpyAsync(rhat, r, vbytes, hipMemcpyDeviceToDevice, st));
	k.finish<BFIN_RR0>();
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));

	// ---- the iterations, pcg_check_every of them between two reads of the state
	const uint64_t every = c->tune.pcg_check_every > 0 ? (uint64_t)c->tune.pcg_check_every : (uint64_t)PCG_CHECK_EVERY;
	k.launches = 0;
	uint64_t readbacks = 0, enqueued = 0;
	BicgState hs;
	auto precondition = [&](const double *in, double *out) {             // out = M^-1 in (nothing to do without a preconditioner)
		if (precond == SPSAMD_PRECOND_JACOBI) {
			k_bicg_jacobi<<<grid, nt, 0, st>>>(in, diag, out, n, k.st);
			SPS_LAUNCH_CHECK();
			++k.launches;
		} else if (precond == SPSAMD_PRECOND_LU) {
			k.launches += solve_levels(c, tl, *sched[0], in, 1, out, 1, 1, nullptr);
			k.launches += solve_levels(c, tu, *sched[1], out, 1, out, 1, 1, nullptr);
		}
	};
	for (;;) {
		hs = read_back(c, k.st);
		++readbacks;
		if (hs.state != PCG_RUNNING) break;
		const uint64_t batch = std::min<uint64_t>(every, max_iter - enqueued);   // (RUNNING: k < max_iter, and k <= enqueued)
		for (uint64_t it = 0; it < batch; ++it) {
			// p = r + beta (p - omega v)
			if (vec) k_bicg_direction<true><<<dim3(grid_for((n + 1) / 2)), dim3(256), 0, st>>>(r, v, p, n, k.st);
			else k_bicg_direction<false><<<dim3(grid_for(n)), dim3(256), 0, st>>>(r, v, p, n, k.st);
			SPS_LAUNCH_CHECK();
			++k.launches;
			// y = M^-1 p, v = A y, rv = dot(rhat, v), alpha
			precondition(p, y);
			bicg_spmv(k, op, y, v, 1, rhat, k.st);
			k.finish<BFIN_RV>();
			// s = r - alpha v, ss = dot(s, s), the half-step decision
			if (k.unfused) {
				k_bicg_half<false><<<grid, nt, 0, st>>>(r, v, s, n, k.part0, k.st);
				SPS_LAUNCH_CHECK();
				++k.launches;
				k.dot(s, s, k.part0, k.st);
			} else {
				k_bicg_half<true><<<grid, nt, 0, st>>>(r, v, s, n, k.part0, k.st);
				SPS_LAUNCH_CHECK();
				++k.launches;
			}
			k.finish<BFIN_SS>();
			// z = M^-1 s, t = A z, ts = dot(t, s), tt = dot(t, t), omega
			precondition(s, z);
			bicg_spmv(k, op, z, t, 2, s, k.st);
			k.finish<BFIN_TS_TT>();
			// x = (x + alpha y) + omega z, r = s - omega t, rr, rho', k, hist, the stop tests, beta
			if (k.unfused) {
				k_bicg_update<1><<<grid, nt, 0, st>>>(dx, y, z, r, s, t, rhat, n, k.part0, k.part1, k.st);
				SPS_LAUNCH_CHECK();
				k_bicg_update<2><<<grid, nt, 0, st>>>(dx, y, z, r, s, t, rhat, n, k.part0, k.part1, k.st);
				SPS_LAUNCH_CHECK();
				k.launches += 2;
				k.dot(r, r, k.part0, k.st);
				k.dot(rhat, r, k.part1, k.st);
			} else {
				k_bicg_update<0><<<grid, nt, 0, st>>>(dx, y, z, r, s, t, rhat, n, k.part0, k.part1, k.st);
				SPS_LAUNCH_CHECK();
				++k.launches;
			}
			k.finish<BFIN_RR_RHO>();
		}
		enqueued += batch;
	}

	if (mem == SPSAMD_MEM_HOST) SPS_HIP(hipMemcpyAsync(x, dx, vbytes, hipMemcpyDeviceToHost, st));
	const uint64_t nh = std::min<uint64_t>(hs.k + 1, hcap);
	if (nh) SPS_HIP(hipMemcpyAsync(hist_host, k.hist, nh * sizeof(double), hipMemcpyDeviceToHost, st));
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	if (stats) {
		stats->iterations = hs.k; stats->reason = hs.state;
		stats->bb = hs.bb; stats->rr0 = hs.rr0; stats->rr = hs.rr;
		stats->launches = k.launches; stats->readbacks = readbacks; stats->analyses = analyses;
		stats->ms_setup = res->ms_consolidate + res->ms_symbolic; stats->ms_iterate = res->ms_numeric;
	}
	return SPSAMD_OK;
}

} // namespace spsamd
