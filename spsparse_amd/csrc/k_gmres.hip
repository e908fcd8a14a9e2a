// k_gmres.hip -- A x = b for an unsymmetric A by right-preconditioned restarted GMRES(m), the whole loop on the device
// (spsamd_solve_gmres, include/spsparse_amd.h).
//
// The frame of the call is KrylovCall's (krylov_dev.h), as for k_krylov.hip and k_bicgstab.hip: the checks, S = op(A) and
// F = op(M), the workspace, the preconditioner, the read-back loop, the tail, and the vector kernels k_pcg_dot, _spmv,
// _residual and _jacobi.  Every returned bit is defined by the loop of the header, every dot product in the one reduction
// shape of krylov_dev.h.  What this loop adds is the orthogonalisation of one vector w against the block v_0 .. v_j, classical
// Gram-Schmidt done twice.  An Arnoldi step at inner index j is
//     z = M^-1 v_j, w = A z                                              the frame's precondition and spmv
//     the partials of dot(v_i, w), i = 0 .. j, in one pass over V        k_gmres_project     (w in registers)
//     h_i = their folds, a workgroup a vector                            k_gmres_fold<0>
//     w = w - h_i v_i, i ascending                                       k_gmres_subtract<0> (w in registers)
//     the same three with d_i; h_i = h_i + d_i; the partials of ww       k_gmres_project, _fold<1>, _subtract<1>
//     ww, hn, the rotations, den, c_j, s_j, R's column, g, k, j, hist,   k_gmres_hess        (one workgroup)
//     the end-of-cycle decision
//     v_{j+1} = w / hn                                                   k_gmres_scale<0>
// and under gmres_path 1 every dot is the frame's k_pcg_dot with a k_gmres_fold of one workgroup, every w = w - coef v_i a
// k_gmres_subtract over the one vector: the same arithmetic in the launches that composing the existing kernels gives.
//
// The state (GmresState, a PcgState with hn, j and `broken`; g, c, s, h, d, y and R beside it in device memory) has one
// value more than RUNNING: GMRES_CYCLE_END, from the k_gmres_hess that ends a cycle to the k_gmres_backsub of that cycle's
// end.  A cycle may end at any step, so the host cannot know j: every step kernel reads j and the state word, and between
// two reads of the state the host enqueues one whole cycle, min(m, max_iter - k) steps for the k it read (a cycle may end on
// the estimate with the true rr above the threshold, and the loop goes on: k is then behind what was enqueued) and one cycle
// end.  A cycle that
// began RUNNING ends within those steps (j == m, k == max_iter, the estimate, or a breakdown), so step kernels behind the
// end are idle (to them, and to the frame's kernels, CYCLE_END is not RUNNING) and the cycle end runs once:
//     y by back substitution; the state back to RUNNING (j > 0), or BREAKDOWN with x untouched (j == 0)     k_gmres_backsub
//     u = sum y_i v_i, or x = x + u at once without a preconditioner                                        k_gmres_combine
//     z = M^-1 u, x = x + z                                                       the frame's precondition, k_gmres_addx
//     q = A x, r = b - q with the partials of dot(r, r)                           the frame's spmv and residual
//     rr, hist[k] = rr, BREAKDOWN if broken, else the stop tests of the cycle's top, beta, g_0, j = 0       k_gmres_finish
//     v_0 = r / beta                                                                                        k_gmres_scale<1>
// w, z and V are scratch after the stop.  No kernel reads what another workgroup wrote in the same launch.
#include "krylov_dev.h"

namespace spsamd {

constexpr int32_t GMRES_CYCLE_END = -2;        // GmresState::state from the hess that ends a cycle to that cycle's back substitution
constexpr int GM_T = PCG_CHUNK / 64;           // elements of a chunk a lane holds

struct GmresState : PcgState {                 // (beta holds sqrt(rr) of the cycle's top; rz, pq and alpha are not used)
	double hn;                                 // sqrt(ww) of the last step
	unsigned long long j;                      // the inner index: v_0 .. v_j are stored
	int32_t broken, pad2;                      // the cycle in progress ends in BREAKDOWN
};

// The scalars of a cycle in device memory: g[m + 1], c[m], s[m], h[m + 1], d[m + 1], y[m], and R[i * m + l] (row i, column l)
struct GmresArrays {
	double *g, *c, *s, *h, *d, *y, *R;
};

__device__ __forceinline__ double flip_sign(double a) { return __longlong_as_double(__double_as_longlong(a) ^ (long long)0x8000000000000000ull); }

// a lane's 16 elements of chunk g of t (+0.0 at or past n)
__device__ __forceinline__ void load_chunk(const double *__restrict__ t, uint64_t g, uint64_t n, double (&out)[GM_T])
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
#pragma unroll
	for (int k = 0; k < GM_T; ++k) {
		const uint64_t e = base + (uint64_t)k * 64;
		out[k] = e < n ? t[e] : 0.0;
	}
}

__device__ __forceinline__ void store_chunk(double *__restrict__ t, uint64_t g, uint64_t n, const double (&in)[GM_T])
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
#pragma unroll
	for (int k = 0; k < GM_T; ++k) {
		const uint64_t e = base + (uint64_t)k * 64;
		if (e < n) t[e] = in[k];
	}
}

// ---------------------------------------------------------------- level 0: the block kernels

// part[i c0 + g] = the partial of chunk g of dot(v_i, w), i = 0 .. j: w stays in registers, and v_{i+1}'s loads are issued
// before v_i's butterfly
__global__ void __launch_bounds__(PCG_NT) k_gmres_project(const double *__restrict__ V, const double *__restrict__ w, uint64_t n, uint64_t c0,
	double *__restrict__ part, const GmresState *gs)
{
	uint64_t g;
	if (stopped(gs) || !my_chunk(n, &g)) return;
	const uint64_t j = gs->j;
	double wr[GM_T], cur[GM_T], nxt[GM_T];
	load_chunk(w, g, n, wr);
	load_chunk(V, g, n, cur);
	for (uint64_t i = 0; i <= j; ++i) {                                  // uniform
		if (i < j) load_chunk(V + (i + 1) * n, g, n, nxt);
#pragma unroll
		for (int k = 0; k < GM_T; ++k) cur[k] = ref_mul(cur[k], wr[k]);
		const double a = chunk_partial_regs(g, n, cur);
		if (lane_id() == 0) part[i * c0 + g] = a;
		if (i < j) {
#pragma unroll
			for (int k = 0; k < GM_T; ++k) cur[k] = nxt[k];
		}
	}
}

// (PASS ? d : h)[i] = fold of part[(i - i0) stride .. + c0), i = i0 + blockIdx.x, for i <= j: a workgroup a vector, each with
// level buffers of its own (fb: 2 c1 doubles a workgroup).  The block path folds all j + 1 arrays in one launch (i0 = 0,
// stride = c0), gmres_path 1 one array a launch (stride 0).
template <int PASS>
__global__ void __launch_bounds__(PCG_FINISH_NT) k_gmres_fold(const double *part, uint64_t c0, uint64_t stride, uint64_t i0, double *fb,
	uint64_t c1, GmresArrays a, const GmresState *gs)
{
	__shared__ double s_out;
	const uint64_t i = i0 + blockIdx.x;
	if (stopped(gs) || i > gs->j) return;                                // uniform
	const double *p = part + (uint64_t)blockIdx.x * stride;
	double *b0 = fb + (uint64_t)blockIdx.x * 2 * c1;
	const double v = c0 == 1 ? p[0] : block_fold(p, c0, b0, b0 + c1, &s_out);
	if (threadIdx.x == 0) (PASS ? a.d : a.h)[i] = v;
}

// w = w - coef_i v_i for i = lo .. min(hi, j) ascending, coef = PASS ? d : h, w in registers and stored once.  PASS 1 also
// does h_i = h_i + d_i for those i (lane 0 of chunk 0: no other workgroup reads h here) and, where partw is given, leaves the
// partials of dot(w, w).
template <int PASS>
__global__ void __launch_bounds__(PCG_NT) k_gmres_subtract(const double *__restrict__ V, double *__restrict__ w, uint64_t n, uint64_t lo,
	uint64_t hi, double *__restrict__ partw, GmresArrays a, const GmresState *gs)
{
	uint64_t g;
	if (stopped(gs) || !my_chunk(n, &g)) return;
	hi = min((unsigned long long)hi, gs->j);
	if (lo > hi) return;
	const double *coef = PASS ? a.d : a.h;
	double wr[GM_T], cur[GM_T], nxt[GM_T];
	load_chunk(w, g, n, wr);
	load_chunk(V + lo * n, g, n, cur);
	for (uint64_t i = lo; i <= hi; ++i) {                                // uniform
		if (i < hi) load_chunk(V + (i + 1) * n, g, n, nxt);
		const double ci = coef[i];
#pragma unroll
		for (int k = 0; k < GM_T; ++k) wr[k] = ref_sub(wr[k], ref_mul(ci, cur[k]));
		if (i < hi) {
#pragma unroll
			for (int k = 0; k < GM_T; ++k) cur[k] = nxt[k];
		}
	}
	store_chunk(w, g, n, wr);
	if (PASS && partw) {
#pragma unroll
		for (int k = 0; k < GM_T; ++k) cur[k] = ref_mul(wr[k], wr[k]);
		const double p = chunk_partial_regs(g, n, cur);
		if (lane_id() == 0) partw[g] = p;
	}
	if (PASS && g == 0 && lane_id() == 0)
		for (uint64_t i = lo; i <= hi; ++i) a.h[i] = ref_add(a.h[i], a.d[i]);
}

// FIRST 0: v_j = w / hn (the j the step's k_gmres_hess left) | 1: v_0 = r / beta
template <int FIRST>
__global__ void __launch_bounds__(PCG_NT) k_gmres_scale(const double *__restrict__ src, double *__restrict__ V, uint64_t n, const GmresState *gs)
{
	uint64_t g;
	if (stopped(gs) || !my_chunk(n, &g)) return;
	const double div = FIRST ? gs->beta : gs->hn;
	double *dst = V + (FIRST ? 0 : gs->j) * n;
	double t[GM_T];
	load_chunk(src, g, n, t);
#pragma unroll
	for (int k = 0; k < GM_T; ++k) t[k] = ref_div(t[k], div);
	store_chunk(dst, g, n, t);
}

// u = sum over i < j ascending of y_i v_i from +0.0, u in registers.  DIRECT: x = x + u | else out = u
template <bool DIRECT>
__global__ void __launch_bounds__(PCG_NT) k_gmres_combine(const double *__restrict__ V, double *__restrict__ out, uint64_t n, GmresArrays a,
	const GmresState *gs)
{
	uint64_t g;
	if (stopped(gs) || !my_chunk(n, &g)) return;
	const uint64_t j = gs->j;
	double u[GM_T], cur[GM_T], nxt[GM_T];
#pragma unroll
	for (int k = 0; k < GM_T; ++k) u[k] = 0.0;
	load_chunk(V, g, n, cur);
	for (uint64_t i = 0; i < j; ++i) {                                   // uniform (j >= 1)
		if (i + 1 < j) load_chunk(V + (i + 1) * n, g, n, nxt);
		const double yi = a.y[i];
#pragma unroll
		for (int k = 0; k < GM_T; ++k) u[k] = ref_add(u[k], ref_mul(yi, cur[k]));
		if (i + 1 < j) {
#pragma unroll
			for (int k = 0; k < GM_T; ++k) cur[k] = nxt[k];
		}
	}
	if (DIRECT) {
		load_chunk(out, g, n, cur);
#pragma unroll
		for (int k = 0; k < GM_T; ++k) u[k] = ref_add(cur[k], u[k]);
	}
	store_chunk(out, g, n, u);
}

// x = x + z
__global__ void __launch_bounds__(PCG_NT) k_gmres_addx(double *__restrict__ x, const double *__restrict__ z, uint64_t n, const GmresState *gs)
{
	uint64_t g;
	if (stopped(gs) || !my_chunk(n, &g)) return;
	double xr[GM_T], zr[GM_T];
	load_chunk(x, g, n, xr);
	load_chunk(z, g, n, zr);
#pragma unroll
	for (int k = 0; k < GM_T; ++k) xr[k] = ref_add(xr[k], zr[k]);
	store_chunk(x, g, n, xr);
}

// ---------------------------------------------------------------- levels 1 and up, the scalars, the decisions

// The end of a step: ww from its partials, then thread 0 (the loop of the header from `hn = sqrt(ww)` to the end-of-cycle test)
__global__ void __launch_bounds__(PCG_FINISH_NT) k_gmres_hess(const double *partw, uint64_t c0, double *b0, double *b1, GmresArrays a, uint32_t m,
	double *__restrict__ hist, GmresState *gs)
{
	__shared__ double s_out;
	const int32_t state = gs->state;
	__syncthreads();                                                 // every thread has read the state before thread 0 may set it
	if (state != PCG_RUNNING) return;                                // uniform
	const double ww = c0 == 1 ? partw[0] : block_fold(partw, c0, b0, b1, &s_out);
	if (threadIdx.x != 0) return;
	const uint64_t j = gs->j;
	const double hn = ref_sqrt(ww);
	double hi = a.h[0];
	for (uint64_t i = 0; i < j; ++i) {
		const double ci = a.c[i], si = a.s[i], h1 = a.h[i + 1];
		const double t = ref_add(ref_mul(ci, hi), ref_mul(si, h1));
		const double u = ref_sub(ref_mul(ci, h1), ref_mul(si, hi));
		a.R[i * m + j] = t;                                              // (read only if this step counts)
		hi = u;
	}
	const double den = ref_sqrt(ref_add(ref_mul(hi, hi), ref_mul(hn, hn)));
	if (!pcg_usable(den)) { gs->broken = 1; gs->state = GMRES_CYCLE_END; return; }   // the step is discarded: k and j stay
	const double cj = ref_div(hi, den), sj = ref_div(hn, den), gj = a.g[j];
	a.c[j] = cj; a.s[j] = sj; a.R[j * m + j] = den;
	const double g1 = flip_sign(ref_mul(sj, gj));
	a.g[j + 1] = g1; a.g[j] = ref_mul(cj, gj);
	const unsigned long long k = gs->k + 1;
	const double est = ref_mul(g1, g1);
	gs->k = k; gs->j = j + 1; gs->hn = hn;
	if (k < gs->hist_cap) hist[k] = est;
	if (est <= gs->thresh || j + 1 == m || k == gs->max_iter || !pcg_usable(ww)) {     // (a NaN compares false)
		if (ww != ww || mag_of(ww) == 0x7FF0000000000000ull) gs->broken = 1;
		gs->state = GMRES_CYCLE_END;
	}
}

// The cycle end's first kernel, one wave.  j == 0 (the first step broke down): BREAKDOWN, x untouched.  Else y from
// R y = g by rows from the last: a row's products by the lanes, its chain l ascending by lane 0; then RUNNING again, for
// the kernels of the cycle end.
__global__ void __launch_bounds__(64) k_gmres_backsub(GmresArrays a, uint32_t m, GmresState *gs)
{
	__shared__ double s_y[SPSAMD_GMRES_MAX_RESTART], s_p[SPSAMD_GMRES_MAX_RESTART];
	if (gs->state != GMRES_CYCLE_END) return;                            // uniform
	const int j = (int)gs->j;
	if (j == 0) { if (threadIdx.x == 0) gs->state = SPSAMD_PCG_BREAKDOWN; return; }
	for (int i = j - 1; i >= 0; --i) {
		for (int l = i + 1 + (int)threadIdx.x; l < j; l += 64) s_p[l] = ref_mul(a.R[(uint64_t)i * m + l], s_y[l]);
		__syncthreads();
		if (threadIdx.x == 0) {
			double acc = a.g[i];
			for (int l = i + 1; l < j; ++l) acc = ref_sub(acc, s_p[l]);
			acc = ref_div(acc, a.R[(uint64_t)i * m + i]);
			s_y[i] = acc; a.y[i] = acc;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) gs->state = PCG_RUNNING;
}

enum { GFIN_BB = 0, GFIN_TOP0 = 1, GFIN_TOP = 2 };

// BB: bb and thresh | TOP0: the set-up's rr0, hist[0] | TOP: a cycle end's rr, hist[k] = rr and BREAKDOWN where the cycle broke
// down; then (TOP0, TOP) the stop tests of the cycle's top, beta, g_0 and j = 0
template <int KIND>
__global__ void __launch_bounds__(PCG_FINISH_NT) k_gmres_finish(const double *part, uint64_t c0, double *b0, double *b1, GmresArrays a,
	double *__restrict__ hist, double tol2, GmresState *gs)
{
	__shared__ double s_out;
	const int32_t state = gs->state;
	__syncthreads();                                                 // every thread has read the state before thread 0 may set it
	if (KIND == GFIN_TOP && state != PCG_RUNNING) return;            // uniform
	const double v = c0 == 1 ? part[0] : block_fold(part, c0, b0, b1, &s_out);
	if (threadIdx.x != 0) return;
	if (KIND == GFIN_BB) { gs->bb = v; gs->thresh = ref_mul(tol2, v); return; }
	const unsigned long long k = KIND == GFIN_TOP0 ? 0 : gs->k;
	if (KIND == GFIN_TOP0) gs->rr0 = v;
	gs->rr = v;
	if (k < gs->hist_cap) hist[k] = v;
	if (KIND == GFIN_TOP && gs->broken) gs->state = SPSAMD_PCG_BREAKDOWN;
	else if (v <= gs->thresh) gs->state = SPSAMD_PCG_CONVERGED;          // (a NaN compares false)
	else if (k == gs->max_iter) gs->state = SPSAMD_PCG_MAXITER;
	else if (!pcg_usable(v)) gs->state = SPSAMD_PCG_BREAKDOWN;
	else {
		const double beta = ref_sqrt(v);
		gs->beta = beta; a.g[0] = beta; gs->j = 0;
	}
}

// ---------------------------------------------------------------- host

int solve_gmres(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, uint32_t restart, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (precond < SPSAMD_PRECOND_NONE || precond > SPSAMD_PRECOND_LU) throw Error{SPSAMD_EINVAL, "precond must be SPSAMD_PRECOND_NONE, _JACOBI or _LU"};
	if (restart == 0 || restart > SPSAMD_GMRES_MAX_RESTART) throw Error{SPSAMD_EINVAL, "restart must be 1 .. SPSAMD_GMRES_MAX_RESTART"};
	KrylovCall k;
	if (!k.open(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity, duplicate_policy, zero_nan,
			stats, res, 1, sizeof(GmresState), nullptr)) return SPSAMD_OK;
	const bool single = c->tune.gmres_path == 1;                         // every dot and every subtraction a launch of its own
	k.unfused = single;                                                  // (pcg_fuse is not this call's knob)
	const uint64_t n = k.n, c0 = k.c0, c1 = (c0 + PCG_CHUNK - 1) / PCG_CHUNK, m = restart;
	hipStream_t st = c->stream;
	GmresState *gs = static_cast<GmresState *>(k.st);
	const bool pre = precond != SPSAMD_PRECOND_NONE;

	// ---- the workspace of the loop: nothing is allocated after this
	GmresArrays a;
	a.g = c->arena.get<double>(m + 1); a.c = c->arena.get<double>(m); a.s = c->arena.get<double>(m);
	a.h = c->arena.get<double>(m + 1); a.d = c->arena.get<double>(m + 1); a.y = c->arena.get<double>(m);
	a.R = c->arena.get<double>(m * m);
	double *V = c->arena.get<double>(m * n), *w = c->arena.get<double>(n), *r = c->arena.get<double>(n);
	double *zb = pre ? c->arena.get<double>(n) : nullptr;
	double *bpart = single ? k.part0 : c->arena.get<double>(m * c0);     // a step orthogonalises against m vectors at the most
	double *fb = c->arena.get<double>((single ? 1 : m) * 2 * c1);
	const dim3 grid(k.chunk_grid()), nt(PCG_NT), one(1), fnt(PCG_FINISH_NT);

	// ---- bb, thresh; r = b - A x, rr0, hist[0], the stop tests of the first cycle's top, v_0
	k.dot(k.db, k.db, k.part0, nullptr);
	k_gmres_finish<GFIN_BB><<<one, fnt, 0, st>>>(k.part0, c0, k.b0, k.b1, a, k.hist, tol * tol, gs);
	SPS_LAUNCH_CHECK();
	k.spmv(k.dx, w, 0, nullptr, nullptr);
	k.residual(k.db, w, r);
	k_gmres_finish<GFIN_TOP0><<<one, fnt, 0, st>>>(k.part0, c0, k.b0, k.b1, a, k.hist, 0.0, gs);
	SPS_LAUNCH_CHECK();
	k_gmres_scale<1><<<grid, nt, 0, st>>>(r, V, n, gs);
	SPS_LAUNCH_CHECK();

	const PcgState hs = k.iterate(m, [&](uint64_t s) {
		// ---- one Arnoldi step; where it runs at all, j == s
		const double *vj = V + s * n, *z = vj;
		if (pre) { k.precondition(vj, zb, nullptr); z = zb; }
		k.spmv(z, w, 0, nullptr, gs);
		for (int pass = 0; pass < 2; ++pass) {
			if (single) {
				for (uint64_t i = 0; i <= s; ++i) {
					k.dot(V + i * n, w, k.part0, gs);
					if (pass) k_gmres_fold<1><<<one, fnt, 0, st>>>(k.part0, c0, 0, i, fb, c1, a, gs);
					else k_gmres_fold<0><<<one, fnt, 0, st>>>(k.part0, c0, 0, i, fb, c1, a, gs);
					SPS_LAUNCH_CHECK();
					++k.launches;
				}
				for (uint64_t i = 0; i <= s; ++i) {
					if (pass) k_gmres_subtract<1><<<grid, nt, 0, st>>>(V, w, n, i, i, nullptr, a, gs);
					else k_gmres_subtract<0><<<grid, nt, 0, st>>>(V, w, n, i, i, nullptr, a, gs);
					SPS_LAUNCH_CHECK();
					++k.launches;
				}
			} else {
				k_gmres_project<<<grid, nt, 0, st>>>(V, w, n, c0, bpart, gs);
				SPS_LAUNCH_CHECK();
				if (pass) k_gmres_fold<1><<<dim3((unsigned)s + 1), fnt, 0, st>>>(bpart, c0, c0, 0, fb, c1, a, gs);
				else k_gmres_fold<0><<<dim3((unsigned)s + 1), fnt, 0, st>>>(bpart, c0, c0, 0, fb, c1, a, gs);
				SPS_LAUNCH_CHECK();
				if (pass) k_gmres_subtract<1><<<grid, nt, 0, st>>>(V, w, n, 0, s, k.part0, a, gs);
				else k_gmres_subtract<0><<<grid, nt, 0, st>>>(V, w, n, 0, s, nullptr, a, gs);
				SPS_LAUNCH_CHECK();
				k.launches += 3;
			}
		}
		if (single) k.dot(w, w, k.part0, gs);
		k_gmres_hess<<<one, fnt, 0, st>>>(k.part0, c0, k.b0, k.b1, a, (uint32_t)m, k.hist, gs);
		SPS_LAUNCH_CHECK();
		k_gmres_scale<0><<<grid, nt, 0, st>>>(w, V, n, gs);
		SPS_LAUNCH_CHECK();
		k.launches += 2;
	}, [&] {
		// ---- the cycle end: y, x = x + M^-1 (V y), the true residual, the decisions of the next cycle's top, v_0
		k_gmres_backsub<<<one, dim3(64), 0, st>>>(a, (uint32_t)m, gs);
		SPS_LAUNCH_CHECK();
		if (pre) {
			k_gmres_combine<false><<<grid, nt, 0, st>>>(V, w, n, a, gs);
			SPS_LAUNCH_CHECK();
			k.precondition(w, zb, nullptr);
			k_gmres_addx<<<grid, nt, 0, st>>>(k.dx, zb, n, gs);
			SPS_LAUNCH_CHECK();
			++k.launches;
		} else {
			k_gmres_combine<true><<<grid, nt, 0, st>>>(V, k.dx, n, a, gs);
			SPS_LAUNCH_CHECK();
		}
		k.spmv(k.dx, w, 0, nullptr, gs);
		k.residual(k.db, w, r);
		k_gmres_finish<GFIN_TOP><<<one, fnt, 0, st>>>(k.part0, c0, k.b0, k.b1, a, k.hist, 0.0, gs);
		SPS_LAUNCH_CHECK();
		k_gmres_scale<1><<<grid, nt, 0, st>>>(r, V, n, gs);
		SPS_LAUNCH_CHECK();
		k.launches += 5;                                                 // backsub, combine, residual, finish, scale
	});
	return k.close(hs);
}

} // namespace spsamd
