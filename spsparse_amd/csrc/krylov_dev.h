// krylov_dev.h -- what the device loops of k_krylov.hip (conjugate gradients), k_bicgstab.hip (BiCGStab) and k_gmres.hip
// (restarted GMRES) share: the state
// word and the scalars of a loop in device memory, the one reduction shape of every dot product (the fold of
// include/spsparse_amd.h), a row's serial chain, and the frame of a call (KrylovCall; its members
// and the vector kernels they launch are k_krylov.hip's).  HIP only.
#pragma once

#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>

namespace spsamd {

constexpr int PCG_CHUNK = 1024;                // elements of a level-0 chunk: 16 per lane of one wave
constexpr int PCG_NT = 256;                    // four waves, a chunk each
constexpr int PCG_FINISH_NT = 1024;            // the one workgroup of a finish kernel
constexpr int32_t PCG_RUNNING = -1;            // PcgState::state; from 0 on: SPSAMD_PCG_*

struct PcgState {
	double bb, thresh, rr0, rr, rz, pq, alpha, beta;
	unsigned long long k, max_iter, hist_cap;
	int32_t state, pad;
};

__device__ __forceinline__ bool pcg_usable(double v) { return v == v && mag_of(v) != 0x7FF0000000000000ull && v != 0.0; }

// The partial of chunk g of t[0 .. n) from the 16 terms a lane holds in registers (t[k]: element 1024 g + 64 k + lane; those
// at or past n are not read): valid in lane 0.  Every lane of the wave calls it.
__device__ __forceinline__ double chunk_partial_regs(uint64_t g, uint64_t n, const double (&t)[PCG_CHUNK / 64])
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
	double a = 0.0;
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k)
		if (base + (uint64_t)k * 64 < n) a = ref_add(a, t[k]);
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		const double o = __shfl_down(a, s, 64);
		if (lane_id() < (unsigned)s) a = ref_add(a, o);              // a_l is the left operand
	}
	return a;
}

// The partial of chunk g of t[0 .. n), t[e] = term(e) (called once per element of the chunk, by the lane that owns it):
// valid in lane 0.  Every lane of the wave calls it.
template <class Term>
__device__ __forceinline__ double chunk_partial(uint64_t g, uint64_t n, Term term)
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
	double t[PCG_CHUNK / 64];
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k) {
		const uint64_t e = base + (uint64_t)k * 64;
		t[k] = e < n ? term(e) : 0.0;
	}
	return chunk_partial_regs(g, n, t);
}

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

// row i's serial chain over S; +0.0 for a row of more than long_min tuples (k_spmm.hip's wave kernel adds its chain in the
// next launch)
__device__ __forceinline__ double row_chain(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ col, const double *__restrict__ val,
	const double *__restrict__ in, uint64_t i, uint32_t long_min)
{
	double acc = 0.0;
	const uint32_t b = ptr[i], e = ptr[i + 1];
	if (e - b <= long_min)
		for (uint32_t k = b; k < e; ++k) acc = ref_add(acc, ref_mul(val[k], in[(uint32_t)col[k]]));
	return acc;
}

// the chunk of this wave, or false past the last one
__device__ __forceinline__ bool my_chunk(uint64_t n, uint64_t *g)
{
	*g = (uint64_t)blockIdx.x * (PCG_NT / 64) + wave_id();
	return *g * PCG_CHUNK < n;
}

__device__ __forceinline__ bool stopped(const PcgState *st) { return st && st->state != PCG_RUNNING; }

// fold(part, c0) for c0 >= 2 by the whole workgroup: a wave per chunk, a barrier between two levels; b0 / b1 take the
// levels' partials in turn (ceil(c0 / 1024) entries each).  The value comes back in every thread.
__device__ inline double block_fold(const double *part, uint64_t m, double *b0, double *b1, double *s_out)
{
	const double *src = part;
	double *dst = b0;
	for (;;) {                                                       // uniform
		const uint64_t c = (m + PCG_CHUNK - 1) / PCG_CHUNK;
		for (uint64_t g = wave_id(); g < c; g += PCG_FINISH_NT / 64) {
			const double a = chunk_partial(g, m, [&](uint64_t e) { return src[e]; });
			if (lane_id() == 0) { if (c == 1) *s_out = a; else dst[g] = a; }
		}
		__syncthreads();                                             // this level's partials are complete, and visible to the workgroup
		if (c == 1) break;
		src = dst; dst = dst == b0 ? b1 : b0; m = c;
	}
	return *s_out;
}

// ---------------------------------------------------------------- the frame of a call (members: k_krylov.hip)

// What solve_pcg, solve_pcg_amg, solve_bicgstab and solve_gmres do alike around their iteration bodies.  A loop open()s the call, takes
// its own vectors (then hook->setup), enqueues its set-up with dot / spmv / residual and its own finish kernels, hands its
// iteration body to iterate() and close()s.  Every launch of an iteration goes through a member or bumps `launches`.
struct KrylovCall {
	spsamd_ctx *c = nullptr;
	uint64_t n = 0, c0 = 0;                    // the order; the level-0 chunks of a vector
	bool unfused = false;                      // pcg_fuse 1: every vector operation and every dot a launch of its own
	int precond = 0;
	double *part0 = nullptr, *part1 = nullptr; // level-0 partials (part1 under nparts 2)
	double *b0 = nullptr, *b1 = nullptr;       // block_fold's levels
	double *hist = nullptr;
	PcgState *st = nullptr;                    // the loop's state struct: a PcgState, or one derived from it
	RowOperator op;                            // S
	const double *db = nullptr;                // b and x on the device
	double *dx = nullptr;
	uint64_t launches = 0;

	// The checks (but the range of precond), the zeroing of res / stats, both operands, the workspace of the frame, S's
	// row_operator, the preconditioner's data, b and x on the device, the state's init.  False: n == 0, the call is over.
	bool open(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M, const double *b,
		double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity, int duplicate_policy, int zero_nan,
		spsamd_pcg_stats *stats, spsamd_result *res, int nparts, size_t state_bytes, PcgPrecond *hook);
	// the partials of dot(u, w)
	void dot(const double *u, const double *w, double *part, const PcgState *pred);
	// out = S in.  ndot 1: + the partials of dot(u, out) in part0 | 2: of dot(out, u) in part0 and dot(out, out) in part1
	void spmv(const double *in, double *out, int ndot, const double *u, const PcgState *pred);
	// r = b - q, and the partials of dot(r, r) in part0 (the set-up: no state is read)
	void residual(const double *b, const double *q, double *r);
	// out = M^-1 in (the hook: on the pair of its setup), and where `part` is given the partials of dot(in, out).
	// Nothing is launched without a preconditioner.
	void precondition(const double *in, double *out, double *part);
	// the three event times and stats, x and the history back with the caller
	int close(const PcgState &hs);

	unsigned chunk_grid() const { return (unsigned)((c0 + PCG_NT / 64 - 1) / (PCG_NT / 64)); }

	// The end of the set-up; then `one()` enqueues an iteration, pcg_check_every of them between two reads of the state
	template <class Body> PcgState iterate(Body one)
	{
		const uint64_t every = c->tune.pcg_check_every > 0 ? (uint64_t)c->tune.pcg_check_every : (uint64_t)PCG_CHECK_EVERY;
		return iterate(every, [&](uint64_t) { one(); }, [] {});
	}

	// The same with the batch given: between two reads of the state `every` iterations at the most, one(it) the it-th of its
	// batch, and end() once behind them (a loop whose iterations come in groups: a restart cycle and its end).  The batch is
	// sized from the k that was read: a loop whose every enqueued iteration counts while it is RUNNING (PCG, BiCGStab) has
	// k == the iterations enqueued so far, and one whose group may end early and go on (GMRES) still never enqueues past
	// max_iter and never waits on an empty batch.
	template <class Body, class End> PcgState iterate(uint64_t every, Body one, End end)
	{
		SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], c->stream));
		launches = 0;
		for (;;) {
			const PcgState hs = read_back(c, st);
			++readbacks;
			if (hs.state != PCG_RUNNING) return hs;
			const uint64_t batch = std::min<uint64_t>(every, max_iter - hs.k);       // (RUNNING: k < max_iter)
			for (uint64_t it = 0; it < batch; ++it) one(it);
			end();
		}
	}

	// ---- what only the members use
	double *diag = nullptr;                    // Jacobi
	TriView tl = {}, tu = {};                  // LU: F's triangles and their schedules
	SolveSchedule local[2], *sched[2] = {nullptr, nullptr};
	PcgPrecond *hook = nullptr;
	uint64_t max_iter = 0, hcap = 0, readbacks = 0;
	uint32_t analyses = 0;
	int mem = 0;
	double *x = nullptr, *hist_host = nullptr; // the caller's
	spsamd_pcg_stats *stats = nullptr;
	spsamd_result *res = nullptr;
};

} // namespace spsamd
