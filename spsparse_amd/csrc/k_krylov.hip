// k_krylov.hip -- A x = b by preconditioned conjugate gradients, the whole loop on the device (spsamd_solve_pcg,
// include/spsparse_amd.h).
//
// S = op(A) and F = op(M) as consolidate_operand() hands them over (row-major; consolidated, or trusted as stored).  Every
// returned bit is defined by the loop of the header: products and sums rounded one by one (x86fp.h), the operator and the
// preconditioner as serial chains in S's / F's order, and every dot product in ONE reduction shape, whatever the launch
// geometry:
//     level 0   chunk g = elements [1024 g, 1024 g + 1024): lane l adds t[1024 g + 64 k + l], k = 0 .. 15, to +0.0 in that
//               order; then a butterfly over the lanes (s = 32 .. 1: a_l = a_l + a_{l+s}); the partial is a_0
//     level 1+  the same over the partials, until one value is left
// A wave owns a chunk, so level 0 needs no LDS and no barrier: 16 coalesced loads per lane and six shuffles.  The kernels
// that produce a vector in chunk order (the Jacobi division, the serial SpMV, the x / r update, the residual) produce the
// level-0 partials of the dot that follows in the same pass; behind the level-scheduled solves of k_solve.hip k_pcg_dot runs
// alone.  Rows above spmm_long_min are left to k_spmm.hip's wave kernel (their list is made once per call); the fused SpMV
// still covers every short row, and k_pcg_dot_rows then redoes the partials of the few chunks that hold a long row.
// Levels 1 and up, the scalar that depends on the dot and the stop tests are one workgroup, k_pcg_finish.
//
// The scalars, k, the history and the state word live in device memory (PcgState).  The host enqueues pcg_check_every
// iterations and reads the state once; every kernel of this file that writes x, r, p, k, the history or a scalar reads the
// state first and does nothing unless it is RUNNING.  q and z are scratch of the loop and may be overwritten after the stop
// (k_spmm.hip and k_solve.hip know nothing of the state); nothing returned depends on them.  No kernel reads what another
// workgroup wrote in the same launch: every dependency between workgroups is a kernel boundary.
//
// The preconditioner step is also a hook (PcgPrecond, internal.h): spsamd_solve_pcg_amg runs this loop with the multigrid
// cycle of k_amg.hip as z = M^-1 r, under the rule of the solves -- it writes its own scratch and z, and reads no state.
//
// This file also holds what every Krylov loop of the library shares (k_bicgstab.hip is the other one): the vector kernels
// k_pcg_dot, _residual, _jacobi, _spmv, _dot_rows and _init, and the members of the frame that alone launches them
// (KrylovCall, krylov_dev.h) -- the argument checks, the operands, the workspace, the preconditioner's data, the read-back
// loop and the tail of a call.  A loop keeps its direction, update and finish kernels, its state struct and its body.
#include "krylov_dev.h"

#include <cstring>

namespace spsamd {

// ---------------------------------------------------------------- level 0: the vector kernels of every loop

__global__ void __launch_bounds__(PCG_NT) k_pcg_dot(const double *u, const double *w, uint64_t n, double *__restrict__ part, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	const double a = chunk_partial(g, n, [&](uint64_t e) { return ref_mul(u[e], w[e]); });
	if (lane_id() == 0) part[g] = a;
}

// r = b - q (the set-up's residual), and the partials of dot(r, r)
template <bool DOT>
__global__ void __launch_bounds__(PCG_NT) k_pcg_residual(const double *__restrict__ b, const double *__restrict__ q, double *__restrict__ r,
	uint64_t n, double *__restrict__ part)
{
	uint64_t g;
	if (!my_chunk(n, &g)) return;
	const double a = chunk_partial(g, n, [&](uint64_t e) { const double v = ref_sub(b[e], q[e]); r[e] = v; return DOT ? ref_mul(v, v) : 0.0; });
	if (DOT && lane_id() == 0) part[g] = a;
}

// out = in / d, and the partials of dot(in, out)
template <bool DOT>
__global__ void __launch_bounds__(PCG_NT) k_pcg_jacobi(const double *__restrict__ in, const double *__restrict__ d, double *__restrict__ out,
	uint64_t n, double *__restrict__ part, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	const double a = chunk_partial(g, n, [&](uint64_t e) { const double re = in[e], v = ref_div(re, d[e]); out[e] = v; return DOT ? ref_mul(re, v) : 0.0; });
	if (DOT && lane_id() == 0) part[g] = a;
}

// out = S in by row_chain.  NDOT 1: and the partials of dot(u, out) | 2: of dot(out, u) and dot(out, out).  The partial of a
// chunk that holds a long row is redone once the wave kernel has added that row's chain (k_pcg_dot_rows).  A lane walks the
// 16 rows 64 apart that the fold gives it.  u may be `in`.
template <int NDOT>
__global__ void __launch_bounds__(PCG_NT) k_pcg_spmv(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *in, double *__restrict__ out, uint64_t n, uint32_t long_min, const double *u, double *__restrict__ part0,
	double *__restrict__ part1, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	if (NDOT == 2) {
		double a0, a1;
		chunk_partial2(g, n, [&](uint64_t i, double *t0, double *t1) {
			const double acc = row_chain(ptr, col, val, in, i, long_min);
			out[i] = acc;
			*t0 = ref_mul(acc, u[i]); *t1 = ref_mul(acc, acc);
		}, &a0, &a1);
		if (lane_id() == 0) { part0[g] = a0; part1[g] = a1; }
	} else {
		const double a = chunk_partial(g, n, [&](uint64_t i) {
			const double acc = row_chain(ptr, col, val, in, i, long_min);
			out[i] = acc;
			return NDOT ? ref_mul(u[i], acc) : 0.0;
		});
		if (NDOT && lane_id() == 0) part0[g] = a;
	}
}

// The partials of dot(u0, w0) -- and of dot(u1, w1) where u1 is given -- for the chunks that hold a listed row, a wave per
// listed row (two rows of one chunk store the same value twice)
__global__ void __launch_bounds__(64) k_pcg_dot_rows(const double *u0, const double *w0, double *part0, const double *u1, const double *w1,
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

// A loop's state struct of `words` 8-byte words, a PcgState first: all +0.0 / 0 but these three
__global__ void k_pcg_init(PcgState *st, uint32_t words, unsigned long long max_iter, unsigned long long hist_cap)
{
	for (uint32_t w = 0; w < words; ++w) reinterpret_cast<unsigned long long *>(st)[w] = 0;
	st->max_iter = max_iter; st->hist_cap = hist_cap; st->state = PCG_RUNNING;
}

// ---------------------------------------------------------------- the loop's own vector kernels

// p = z (k == 0), else p = z + beta p.  No fold here, so nothing fixes which lane owns which element: VEC takes two
// neighbouring elements per thread in 16-byte loads and stores (z and p 16-byte aligned), the odd last element alone.
template <bool VEC>
__global__ void __launch_bounds__(256) k_pcg_direction(const double *__restrict__ z, double *__restrict__ p, uint64_t n, const PcgState *st)
{
	if (stopped(st)) return;
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool first = st->k == 0;
	const double beta = st->beta;
	if (VEC) {
		const uint64_t e = 2 * t;
		if (e + 1 < n) {
			const double2 zz = *reinterpret_cast<const double2 *>(z + e);
			double2 pp = zz;
			if (!first) {
				pp = *reinterpret_cast<const double2 *>(p + e);
				pp.x = ref_add(zz.x, ref_mul(beta, pp.x));
				pp.y = ref_add(zz.y, ref_mul(beta, pp.y));
			}
			*reinterpret_cast<double2 *>(p + e) = pp;
		} else if (e < n) p[e] = first ? z[e] : ref_add(z[e], ref_mul(beta, p[e]));
	} else if (t < n) p[t] = first ? z[t] : ref_add(z[t], ref_mul(beta, p[t]));
}

// WHAT 0: x += alpha p, r -= alpha q and the partials of dot(r, r) | 1: x += alpha p alone | 2: r -= alpha q alone
template <int WHAT>
__global__ void __launch_bounds__(PCG_NT) k_pcg_update(double *__restrict__ x, const double *__restrict__ p, double *__restrict__ r,
	const double *__restrict__ q, uint64_t n, double *__restrict__ part, const PcgState *st)
{
	uint64_t g;
	if (stopped(st) || !my_chunk(n, &g)) return;
	const double alpha = st->alpha;
	const double a = chunk_partial(g, n, [&](uint64_t e) {
		if (WHAT != 2) x[e] = ref_add(x[e], ref_mul(alpha, p[e]));
		if (WHAT == 1) return 0.0;
		const double v = ref_sub(r[e], ref_mul(alpha, q[e]));
		r[e] = v;
		return WHAT == 0 ? ref_mul(v, v) : 0.0;
	});
	if (WHAT == 0 && lane_id() == 0) part[g] = a;
}

// ---------------------------------------------------------------- levels 1 and up, the scalars, the stop tests

enum { FIN_BB = 0, FIN_RR0 = 1, FIN_RZ = 2, FIN_PQ = 3, FIN_RR = 4 };

// part == nullptr (FIN_RZ under PRECOND_NONE): z is r, and dot(r, z) has the bits of rr
template <int KIND>
__global__ void __launch_bounds__(PCG_FINISH_NT) k_pcg_finish(const double *part, uint64_t c0, double *b0, double *b1, PcgState *st,
	double *__restrict__ hist, double tol2)
{
	__shared__ double s_out;
	const bool idle = KIND >= FIN_RZ && st->state != PCG_RUNNING;
	__syncthreads();                                                 // every thread has read the state before thread 0 may set it
	if (idle) return;                                                // uniform
	double v = 0.0;
	if (part) v = c0 == 0 ? 0.0 : c0 == 1 ? part[0] : block_fold(part, c0, b0, b1, &s_out);
	if (threadIdx.x != 0) return;
	if (KIND == FIN_BB) { st->bb = v; st->thresh = ref_mul(tol2, v); return; }
	if (KIND == FIN_RZ) {
		const double rz = part ? v : st->rr;
		if (st->k != 0) st->beta = ref_div(rz, st->rz);
		st->rz = rz;
		if (!pcg_usable(rz)) st->state = SPSAMD_PCG_BREAKDOWN;
		return;
	}
	if (KIND == FIN_PQ) {
		st->pq = v;
		if (!pcg_usable(v)) st->state = SPSAMD_PCG_BREAKDOWN;
		else st->alpha = ref_div(st->rz, v);
		return;
	}
	unsigned long long k = 0;
	if (KIND == FIN_RR0) st->rr0 = v;
	else { k = st->k + 1; st->k = k; }
	st->rr = v;
	if (k < st->hist_cap) hist[k] = v;
	if (v <= st->thresh) st->state = SPSAMD_PCG_CONVERGED;               // (a NaN compares false)
	else if (k == st->max_iter) st->state = SPSAMD_PCG_MAXITER;
}

// ---------------------------------------------------------------- host: the frame

// (declared in internal.h) S, taken by consolidate_operand, with what its serial chains need
void row_operator(spsamd_ctx *c, ConMat &S, Prepared *hp, uint64_t nrow, uint64_t ncol, bool long_rows, RowOperator *out)
{
	RowOperator &op = *out;
	op.nrow = nrow; op.ncol = ncol; op.nnz = S.nnz;
	if (hp) { prepared_row_structure(c, hp); op.ptr = hp->rowptr; }
	else if (!S.nnz) op.ptr = get_zeroed<uint32_t>(c, nrow + 1);
	else { S.nrow = nrow; op.ptr = dense_rowptr(c, S, 0); }
	op.col = S.col; op.val = S.val;
	if (S.nnz && long_rows) {
		const int path = c->tune.spmm_path;
		op.long_min = path == 1 ? 0xFFFFFFFFu : path >= 2 ? 0u : c->tune.spmm_long_min > 0 ? (uint32_t)c->tune.spmm_long_min : 64u;
		uint32_t *list = nullptr, *count = nullptr;
		if (path != 1) op.nlong = spmm_long_list(c, op.ptr, nrow, op.long_min, &list, &count);
		if (op.nlong) {
			op.list = list; op.count = count;
			op.m.rowptr = op.ptr; op.m.nrow = nrow; op.m.ncol = ncol; op.m.nnz = S.nnz;
			if (hp) op.m.tup = prepared_btup(c, hp);
			else { BTup *t = c->arena.get<BTup>(S.nnz); pack_tuples(c, S.col, S.val, S.nnz, t); op.m.tup = t; }
		}
	}
}

void check_vector_overlap(spsamd_ctx *c, const spsamd_coo *X, const char *name, const double *x, uint64_t bytes)
{
	const OperandView view = operand_view(c, X);
	const uint64_t n = view.coo.nnz;
	if (n >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, std::string(name) + " has 2^31 or more tuples"};
	const void *arr[3] = {view.coo.idx0, view.coo.idx1, view.coo.val};
	for (int k = 0; k < 3; ++k)
		if (ranges_overlap(x, bytes, arr[k], n * (k == 2 ? 8 : 4))) throw Error{SPSAMD_EINVAL, std::string("x overlaps the arrays of ") + name};
}

bool KrylovCall::open(spsamd_ctx *ctx, const spsamd_coo *A, char transpose, int pre, const spsamd_coo *M, char transpose_M, const double *b,
	double *xx, int mm, double tol, uint64_t maxit, double *hh, size_t hist_capacity, int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *ss, spsamd_result *rr, int nparts, size_t state_bytes, PcgPrecond *hk)
{
	c = ctx; precond = pre; x = xx; mem = mm; max_iter = maxit; hist_host = hh; stats = ss; res = rr; hook = hk;
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of b and x must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	if (!(tol >= 0.0) || tol - tol != 0.0) throw Error{SPSAMD_EINVAL, "tol must be finite and not negative"};
	if ((precond == SPSAMD_PRECOND_LU) != (M != nullptr)) throw Error{SPSAMD_EINVAL, "M goes with SPSAMD_PRECOND_LU, and only with it"};
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	const int lead = transpose == 'T' ? 1 : 0, lead_m = transpose_M == 'T' ? 1 : 0;
	n = A->shape0;
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
		return false;
	}

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], c->stream));
	ConMat S, F;
	Prepared *hpa = nullptr, *hpm = nullptr;
	consolidate_operand(c, A, lead, lead, duplicate_policy, zero_nan, &S, &hpa);
	if (M) consolidate_operand(c, M, lead_m, lead_m, duplicate_policy, zero_nan, &F, &hpm);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], c->stream));
	res->nnz_a = S.nnz;
	res->nnz_b = M ? F.nnz : 0;

	// ---- the workspace of the frame (this order fixes workspace_bytes)
	c0 = (n + PCG_CHUNK - 1) / PCG_CHUNK; unfused = c->tune.pcg_fuse == 1;
	const uint64_t c1 = (c0 + PCG_CHUNK - 1) / PCG_CHUNK;
	part0 = c->arena.get<double>(c0);
	if (nparts == 2) part1 = c->arena.get<double>(c0);
	b0 = c->arena.get<double>(c1); b1 = c->arena.get<double>(c1);
	st = (PcgState *)c->arena.alloc(state_bytes);
	hcap = !hist_host ? 0 : std::min<uint64_t>(hist_capacity, max_iter == ~0ull ? max_iter : max_iter + 1);
	hist = hcap ? c->arena.get<double>(hcap) : nullptr;

	// ---- the operator: S's row pointer; the long rows' list and the packed rows of k_spmm.hip only where there is a long row
	row_operator(c, S, hpa, n, n, true, &op);

	// ---- the preconditioner
	if (precond == SPSAMD_PRECOND_JACOBI) {
		diag = c->arena.get<double>(n);
		if (S.nnz) reduce_diag_dense(c, op.ptr, S.col, S.val, n, diag);
		else fill_zero(c, diag, vbytes);
	} else if (precond == SPSAMD_PRECOND_LU) {
		RowOperator fop;
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

	// ---- b and x; the state
	db = to_device(c, b, n, mem);
	dx = x;
	if (mem == SPSAMD_MEM_HOST) { dx = c->arena.get<double>(n); SPS_HIP(hipMemcpyAsync(dx, x, vbytes, hipMemcpyHostToDevice, c->stream)); }
	k_pcg_init<<<dim3(1), dim3(1), 0, c->stream>>>(st, (uint32_t)(state_bytes / 8), max_iter, hcap);
	SPS_LAUNCH_CHECK();
	return true;
}

void KrylovCall::dot(const double *u, const double *w, double *part, const PcgState *pred)
{
	k_pcg_dot<<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(u, w, n, part, pred);
	SPS_LAUNCH_CHECK();
	++launches;
}

// Nothing is allocated here: it runs in every iteration.
void KrylovCall::spmv(const double *in, double *out, int ndot, const double *u, const PcgState *pred)
{
	const int fused = unfused ? 0 : ndot;
	const dim3 grid(chunk_grid()), nt(PCG_NT);
	if (fused == 2) k_pcg_spmv<2><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, n, op.long_min, u, part0, part1, pred);
	else if (fused == 1) k_pcg_spmv<1><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, n, op.long_min, u, part0, part1, pred);
	else k_pcg_spmv<0><<<grid, nt, 0, c->stream>>>(op.ptr, op.col, op.val, in, out, n, op.long_min, u, part0, part1, pred);
	SPS_LAUNCH_CHECK();
	++launches;
	if (op.nlong) {
		spmm_long_rows(c, op.m, op.list, op.count, in, 1, out, 1, 1);
		++launches;
	}
	if (!ndot) return;
	const double *u0 = ndot == 1 ? u : out, *w0 = ndot == 1 ? out : u;
	if (!fused || op.nlong > c0) {                                       // (more long rows than chunks: every chunk once instead)
		dot(u0, w0, part0, pred);
		if (ndot == 2) dot(out, out, part1, pred);
	} else if (op.nlong) {
		k_pcg_dot_rows<<<dim3(std::min<unsigned>(op.nlong, (unsigned)c->num_cu * 8)), dim3(64), 0, c->stream>>>(u0, w0, part0,
			ndot == 2 ? out : nullptr, out, part1, n, op.list, op.count, pred);
		SPS_LAUNCH_CHECK();
		++launches;
	}
}

void KrylovCall::residual(const double *b, const double *q, double *r)
{
	if (unfused) k_pcg_residual<false><<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(b, q, r, n, part0);
	else k_pcg_residual<true><<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(b, q, r, n, part0);
	SPS_LAUNCH_CHECK();
	if (unfused) dot(r, r, part0, nullptr);
}

void KrylovCall::precondition(const double *in, double *out, double *part)
{
	if (precond == SPSAMD_PRECOND_JACOBI) {
		const bool fused = part && !unfused;                             // the dot rides in the division
		if (fused) k_pcg_jacobi<true><<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(in, diag, out, n, part, st);
		else k_pcg_jacobi<false><<<dim3(chunk_grid()), dim3(PCG_NT), 0, c->stream>>>(in, diag, out, n, part, st);
		SPS_LAUNCH_CHECK();
		++launches;
		if (fused) return;
	} else if (precond == SPSAMD_PRECOND_LU) {
		launches += solve_levels(c, tl, *sched[0], in, 1, out, 1, 1, nullptr);
		launches += solve_levels(c, tu, *sched[1], out, 1, out, 1, 1, nullptr);
	} else if (hook) launches += hook->apply();
	else return;
	if (part) dot(in, out, part, st);
}

int KrylovCall::close(const PcgState &hs)
{
	if (mem == SPSAMD_MEM_HOST) SPS_HIP(hipMemcpyAsync(x, dx, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	const uint64_t nh = std::min<uint64_t>(hs.k + 1, hcap);
	if (nh) SPS_HIP(hipMemcpyAsync(hist_host, hist, nh * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	if (stats) {
		stats->iterations = hs.k; stats->reason = hs.state;
		stats->bb = hs.bb; stats->rr0 = hs.rr0; stats->rr = hs.rr;
		stats->launches = launches; stats->readbacks = readbacks; stats->analyses = analyses;
		stats->ms_setup = res->ms_consolidate + res->ms_symbolic; stats->ms_iterate = res->ms_numeric;
	}
	return SPSAMD_OK;
}

// ---------------------------------------------------------------- host: conjugate gradients

template <int KIND> static void pcg_finish(KrylovCall &k, bool have_part, double tol2 = 0.0)
{
	k_pcg_finish<KIND><<<dim3(1), dim3(PCG_FINISH_NT), 0, k.c->stream>>>(have_part ? k.part0 : nullptr, k.c0, k.b0, k.b1, k.st, k.hist, tol2);
	SPS_LAUNCH_CHECK();
	++k.launches;
}

// The loop of both entry points.  `hook`: a preconditioner of the caller's own (spsamd_solve_pcg_amg); precond is then
// PCG_PRECOND_HOOK and M null.
int pcg_solve(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res, PcgPrecond *hook)
{
	KrylovCall k;
	if (!k.open(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity, duplicate_policy, zero_nan,
			stats, res, 1, sizeof(PcgState), hook)) return SPSAMD_OK;
	const uint64_t n = k.n;
	hipStream_t st = c->stream;
	double *r = c->arena.get<double>(n), *p = c->arena.get<double>(n), *q = c->arena.get<double>(n);
	double *z = precond == SPSAMD_PRECOND_NONE ? r : c->arena.get<double>(n);
	const bool vec = (((uintptr_t)z | (uintptr_t)p) & 15u) == 0;
	const dim3 grid(k.chunk_grid()), nt(PCG_NT);
	if (hook) hook->setup(c, k.op, r, z);

	// ---- bb, thresh; r = b - A x, rr0, hist[0], the stop tests before the first iteration
	k.dot(k.db, k.db, k.part0, nullptr);
	pcg_finish<FIN_BB>(k, true, tol * tol);
	k.spmv(k.dx, q, 0, nullptr, nullptr);
	k.residual(k.db, q, r);
	pcg_finish<FIN_RR0>(k, true);

	const PcgState hs = k.iterate([&] {
		// z = M^-1 r, rz' = dot(r, z), beta, rz
		k.precondition(r, z, k.part0);
		pcg_finish<FIN_RZ>(k, precond != SPSAMD_PRECOND_NONE);
		if (vec) k_pcg_direction<true><<<dim3(grid_for((n + 1) / 2)), dim3(256), 0, st>>>(z, p, n, k.st);
		else k_pcg_direction<false><<<dim3(grid_for(n)), dim3(256), 0, st>>>(z, p, n, k.st);
		SPS_LAUNCH_CHECK();
		++k.launches;
		// q = A p, pq = dot(p, q), alpha
		k.spmv(p, q, 1, p, k.st);
		pcg_finish<FIN_PQ>(k, true);
		// x += alpha p, r -= alpha q, rr = dot(r, r), k, hist, the stop tests
		if (k.unfused) {
			k_pcg_update<1><<<grid, nt, 0, st>>>(k.dx, p, r, q, n, k.part0, k.st);
			SPS_LAUNCH_CHECK();
			k_pcg_update<2><<<grid, nt, 0, st>>>(k.dx, p, r, q, n, k.part0, k.st);
			SPS_LAUNCH_CHECK();
			k.launches += 2;
			k.dot(r, r, k.part0, k.st);
		} else {
			k_pcg_update<0><<<grid, nt, 0, st>>>(k.dx, p, r, q, n, k.part0, k.st);
			SPS_LAUNCH_CHECK();
			++k.launches;
		}
		pcg_finish<FIN_RR>(k, true);
	});
	return k.close(hs);
}

int solve_pcg(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (precond < SPSAMD_PRECOND_NONE || precond > SPSAMD_PRECOND_LU) throw Error{SPSAMD_EINVAL, "precond must be SPSAMD_PRECOND_NONE, _JACOBI or _LU"};
	return pcg_solve(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity, duplicate_policy,
		zero_nan, stats, res, nullptr);
}

} // namespace spsamd
