// k_bicgstab.hip -- A x = b for an unsymmetric A by right-preconditioned BiCGStab, the whole loop on the device
// (spsamd_solve_bicgstab, include/spsparse_amd.h).
//
// The shape is k_krylov.hip's, and so is the frame of the call (KrylovCall, krylov_dev.h): the checks, S = op(A) and
// F = op(M) as consolidate_operand() hands them over, the workspace, the preconditioner, the read-back loop and the tail, and
// the vector kernels both loops use (k_pcg_dot, _residual, _jacobi, _spmv, _dot_rows, _init).  Every returned bit is defined
// by the loop of the header, every dot product in the one reduction shape of krylov_dev.h (a wave per chunk of 1024
// elements, no LDS and no barrier at level 0).  An iteration has five dots in four groups, and each group rides in the
// kernel that produces its vector:
//     v = A y          with the partials of dot(rhat, v)              k_pcg_spmv<1>      then k_bicg_finish<RV>: alpha
//     s = r - alpha v  with the partials of dot(s, s)                 k_bicg_half        then <SS>: the half-step decision
//     t = A z          with the partials of dot(t, s) and dot(t, t)   k_pcg_spmv<2>      then <TS_TT>: omega
//     x, r             with the partials of dot(r, r), dot(rhat, r)   k_bicg_update<0>   then <RR_RHO>: k, hist, stops, beta
// Two dots of one pass go to two partial arrays and are folded one after the other by the one workgroup of the finish
// kernel.  Rows above spmm_long_min are left to k_spmm.hip's wave kernel as in k_krylov.hip, and k_pcg_dot_rows redoes the
// partials -- of both arrays behind the second SpMV -- of the chunks that hold one.
//
// The state word (BicgState, a PcgState with omega and ss) has one value more than the loop of k_krylov.hip: BICG_HALF, from
// the SS finish that takes the half-step exit until the RR_RHO finish of the same iteration.  In it k_bicg_update does
// x = x + alpha y and nothing else, the RR_RHO finish sets rr = ss, k, hist and CONVERGED, and every other kernel is idle
// (the shared kernels among them: to stopped() HALF is not RUNNING).  Every kernel of this file that writes x, r, p, k, the
// history or a scalar reads the state first and does nothing unless it is RUNNING (or HALF, for those two).  y, z, v, s
// and t are scratch after the stop.  No kernel reads what another workgroup wrote in the same launch.
#include "krylov_dev.h"

namespace spsamd {

constexpr int32_t BICG_HALF = -2;              // BicgState::state between the half-step decision and the x update that goes with it

struct BicgState : PcgState {                  // (rz holds rho; pq is not used)
	double omega, ss;
};

// ---------------------------------------------------------------- level 0: the vector kernels of this loop alone

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

template <int KIND> static void bicg_finish(KrylovCall &k, double tol2 = 0.0)
{
	k_bicg_finish<KIND><<<dim3(1), dim3(PCG_FINISH_NT), 0, k.c->stream>>>(k.part0, k.part1, k.c0, k.b0, k.b1, static_cast<BicgState *>(k.st), k.hist, tol2);
	SPS_LAUNCH_CHECK();
	++k.launches;
}

int solve_bicgstab(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (precond < SPSAMD_PRECOND_NONE || precond > SPSAMD_PRECOND_LU) throw Error{SPSAMD_EINVAL, "precond must be SPSAMD_PRECOND_NONE, _JACOBI or _LU"};
	KrylovCall k;
	if (!k.open(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity, duplicate_policy, zero_nan,
			stats, res, 2, sizeof(BicgState), nullptr)) return SPSAMD_OK;
	const uint64_t n = k.n;
	hipStream_t st = c->stream;
	const BicgState *bs = static_cast<const BicgState *>(k.st);
	double *r = c->arena.get<double>(n), *rhat = c->arena.get<double>(n), *p = c->arena.get<double>(n), *v = c->arena.get<double>(n);
	double *s = c->arena.get<double>(n), *t = c->arena.get<double>(n);
	double *y = precond == SPSAMD_PRECOND_NONE ? p : c->arena.get<double>(n);
	double *z = precond == SPSAMD_PRECOND_NONE ? s : c->arena.get<double>(n);
	const bool vec = (((uintptr_t)r | (uintptr_t)v | (uintptr_t)p) & 15u) == 0;
	const dim3 grid(k.chunk_grid()), nt(PCG_NT);

	// ---- bb, thresh; r = b - A x, rhat, rr0, hist[0], the stop tests before the first iteration
	k.dot(k.db, k.db, k.part0, nullptr);
	bicg_finish<BFIN_BB>(k, tol * tol);
	k.spmv(k.dx, v, 0, nullptr, nullptr);
	k.residual(k.db, v, r);
	SPS_HIP(hipMemcpyAsync(rhat, r, n * sizeof(double), hipMemcpyDeviceToDevice, st));
	bicg_finish<BFIN_RR0>(k);

	const PcgState hs = k.iterate([&] {
		// p = r + beta (p - omega v)
		if (vec) k_bicg_direction<true><<<dim3(grid_for((n + 1) / 2)), dim3(256), 0, st>>>(r, v, p, n, bs);
		else k_bicg_direction<false><<<dim3(grid_for(n)), dim3(256), 0, st>>>(r, v, p, n, bs);
		SPS_LAUNCH_CHECK();
		++k.launches;
		// y = M^-1 p, v = A y, rv = dot(rhat, v), alpha
		k.precondition(p, y, nullptr);
		k.spmv(y, v, 1, rhat, bs);
		bicg_finish<BFIN_RV>(k);
		// s = r - alpha v, ss = dot(s, s), the half-step decision
		if (k.unfused) k_bicg_half<false><<<grid, nt, 0, st>>>(r, v, s, n, k.part0, bs);
		else k_bicg_half<true><<<grid, nt, 0, st>>>(r, v, s, n, k.part0, bs);
		SPS_LAUNCH_CHECK();
		++k.launches;
		if (k.unfused) k.dot(s, s, k.part0, bs);
		bicg_finish<BFIN_SS>(k);
		// z = M^-1 s, t = A z, ts = dot(t, s), tt = dot(t, t), omega
		k.precondition(s, z, nullptr);
		k.spmv(z, t, 2, s, bs);
		bicg_finish<BFIN_TS_TT>(k);
		// x = (x + alpha y) + omega z, r = s - omega t, rr, rho', k, hist, the stop tests, beta
		if (k.unfused) {
			k_bicg_update<1><<<grid, nt, 0, st>>>(k.dx, y, z, r, s, t, rhat, n, k.part0, k.part1, bs);
			SPS_LAUNCH_CHECK();
			k_bicg_update<2><<<grid, nt, 0, st>>>(k.dx, y, z, r, s, t, rhat, n, k.part0, k.part1, bs);
			SPS_LAUNCH_CHECK();
			k.launches += 2;
			k.dot(r, r, k.part0, bs);
			k.dot(rhat, r, k.part1, bs);
		} else {
			k_bicg_update<0><<<grid, nt, 0, st>>>(k.dx, y, z, r, s, t, rhat, n, k.part0, k.part1, bs);
			SPS_LAUNCH_CHECK();
			++k.launches;
		}
		bicg_finish<BFIN_RR_RHO>(k);
	});
	return k.close(hs);
}

} // namespace spsamd
