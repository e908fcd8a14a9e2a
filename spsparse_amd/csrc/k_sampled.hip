// k_sampled.hip -- the sampled dense-dense product (SDDMM): for every tuple t = (i, j, v) of op(M), in storage order,
//     d = +0.0;  for r = 0 .. k-1:  d = d + P[i*ldp + r] * Q[j*ldq + r]       (serial, ascending r)
//     out[t] = alpha * d  (+ beta * v  when beta != 0)
// with the x86-64 NaN rule of x86fp.h on every product and sum, and no FMA (the build has -ffp-contract=off).  Tuples are
// independent: each one's k terms are folded by ONE lane in ascending r, so any grouping of tuples gives the same bits, and
// every output is written exactly once (no atomics).
//
// Kernel shapes:
//   lane   one lane per tuple, its P and Q rows streamed straight into registers (16-byte loads where the rows are 16-byte
//          aligned): small k, and every k where neighbouring tuples read nearby rows
//   slab   one wave per 64 tuples; the 64 P rows and 64 Q rows are staged through LDS in slabs of 16 values (one 128-byte
//          line per row, loaded coalesced), then each lane folds its own tuple's slab serially, the running sum kept in a
//          register across slabs: larger k on random columns, unbounded by LDS
// Auto picks by k and by a probe of M's storage order (auto_slab below).
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>

namespace spsamd {

struct SampledArgs {
	const int32_t *row;         // rows(op(M)) index of each tuple: the row of P
	const int32_t *col;         // cols(op(M)) index of each tuple: the row of Q
	const double *val;          // M's values (read only where beta != 0); may be `out` itself
	uint32_t nnz;
	const double *P;
	uint64_t ldp;
	const double *Q;
	uint64_t ldq;
	uint32_t k;
	double alpha, beta;
	double *out;
};

// o = alpha * d, then + beta * v; the tuple's v is read before its slot is written (out may be M's value array)
__device__ __forceinline__ void finish(const SampledArgs &a, double d, uint32_t t)
{
	double o = ref_mul(a.alpha, d);
	if (a.beta != 0) o = ref_add(o, ref_mul(a.beta, a.val[t]));
	a.out[t] = o;
}

// ---- lane: one lane per tuple ----------------------------------------------------------------------------------------
// VEC = 2: P, Q, ldp and ldq keep every row 16-byte aligned
template <int VEC>
__global__ void __launch_bounds__(256) k_sampled_lane(SampledArgs a)
{
	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.nnz; t += (uint64_t)gridDim.x * blockDim.x) {
		const double *p = a.P + (uint64_t)(uint32_t)a.row[t] * a.ldp;
		const double *q = a.Q + (uint64_t)(uint32_t)a.col[t] * a.ldq;
		double d = 0.0;
		uint32_t r = 0;
		if (VEC == 2) {
#pragma unroll 4
			for (; r + 2 <= a.k; r += 2) {
				const double2 x = *(const double2 *)(p + r), y = *(const double2 *)(q + r);
				d = ref_add(d, ref_mul(x.x, y.x));
				d = ref_add(d, ref_mul(x.y, y.y));
			}
		}
#pragma unroll 4
		for (; r < a.k; ++r) d = ref_add(d, ref_mul(p[r], q[r]));
		finish(a, d, (uint32_t)t);
	}
}

// ---- slab: one wave per 64 tuples, rows staged through LDS ----------------------------------------------------------
constexpr uint32_t SLAB = 16;                     // values of r per slab: one 128-byte line of a row
constexpr uint32_t SLAB_LD = SLAB + 1;            // LDS row stride in doubles: lane l's row starts at bank 34 l mod 64, so
                                                  // the fold's ds_read_b64 (lanes 0-31, then 32-63) hits every bank once

// Rows [0, 64) of this group's slab [r0, r0 + w) of one operand into img (row-major, SLAB_LD apart).  VEC = 2: lane = piece
// (16 bytes) lane % 8 of rows lane / 8 + 8 s; VEC = 1: 8-byte piece lane % 16 of rows lane / 16 + 4 s.  A row past the last
// tuple, or values past w, are not loaded (their slots are never folded into a result that is kept).
template <int VEC>
__device__ __forceinline__ void load_slab(const double *__restrict__ base, const uint64_t *__restrict__ off, uint32_t cnt,
	uint32_t r0, uint32_t w, double *img)
{
	constexpr uint32_t PIECES = SLAB / VEC, ROWS_PER = 64 / PIECES;
	const uint32_t piece = threadIdx.x % PIECES, e = piece * VEC;
#pragma unroll
	for (uint32_t s = 0; s < 64 / ROWS_PER; ++s) {
		const uint32_t rw = threadIdx.x / PIECES + ROWS_PER * s;
		if (rw >= cnt || e >= w) continue;
		const double *src = base + off[rw] + r0 + e;
		double *dst = img + rw * SLAB_LD + e;
		if (VEC == 2 && e + 1 < w) {
			const double2 x = *(const double2 *)src;
			dst[0] = x.x; dst[1] = x.y;
		} else {
			dst[0] = src[0];
		}
	}
}

template <int VEC>
__global__ void __launch_bounds__(64) k_sampled_slab(SampledArgs a)
{
	__shared__ double sp[64 * SLAB_LD], sq[64 * SLAB_LD];
	__shared__ uint64_t op[64], oq[64];             // element offsets of the group's P and Q rows
	const unsigned lane = threadIdx.x;
	const uint32_t groups = (a.nnz + 63) / 64;
	for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
		const uint32_t t0 = g * 64, cnt = min(64u, a.nnz - t0), t = t0 + lane;
		if (lane < cnt) {
			op[lane] = (uint64_t)(uint32_t)a.row[t] * a.ldp;
			oq[lane] = (uint64_t)(uint32_t)a.col[t] * a.ldq;
		}
		__syncthreads();
		double d = 0.0;
		for (uint32_t r0 = 0; r0 < a.k; r0 += SLAB) {
			const uint32_t w = min(SLAB, a.k - r0);
			load_slab<VEC>(a.P, op, cnt, r0, w, sp);
			load_slab<VEC>(a.Q, oq, cnt, r0, w, sq);
			__syncthreads();
			const double *x = sp + lane * SLAB_LD, *y = sq + lane * SLAB_LD;
			if (w == SLAB) {
				double u[SLAB], v[SLAB];
#pragma unroll
				for (uint32_t r = 0; r < SLAB; ++r) { u[r] = x[r]; v[r] = y[r]; }
#pragma unroll
				for (uint32_t r = 0; r < SLAB; ++r) d = ref_add(d, ref_mul(u[r], v[r]));
			} else {
				for (uint32_t r = 0; r < w; ++r) d = ref_add(d, ref_mul(x[r], y[r]));
			}
			__syncthreads();                            // the image is refilled by the next slab (or the next group's offsets)
		}
		if (lane < cnt) finish(a, d, t);
	}
}

// ---- auto: which kernel ----------------------------------------------------------------------------------------------
// The lane kernel's gathers are served from L2 when the 64 tuples of a wave read nearby Q rows (a stencil), and it wins
// there at every k; on random columns (R-MAT) the slab kernel's coalesced loads win from k = 12 (rows unsorted) or 32 (rows
// sorted, P rows shared by neighbouring lanes).  DESIGN.md section 13 has the sweep.
constexpr uint32_t PROBE_MIN_K = 12;              // below: the lane kernel, no probe
constexpr uint32_t SLAB_MIN_K_SORTED = 32;        // non-local columns, rows in order: the slab kernel from here
constexpr uint32_t PROBE_GROUPS = 1024;           // groups of 64 consecutive tuples sampled evenly over M

// counts[0]: sampled groups whose column span is at most ncol / 16; counts[1]: sampled groups whose rows descend somewhere
__global__ void k_sampled_probe(const int32_t *__restrict__ row, const int32_t *__restrict__ col, uint32_t nnz, uint32_t S,
	uint64_t ncol, uint32_t *counts)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= S) return;
	const uint32_t groups = (nnz + 63) / 64;
	const uint32_t b = (uint32_t)((uint64_t)s * groups / S) * 64, e = min(nnz, b + 64);
	int32_t lo = col[b], hi = lo, prev = row[b];
	bool desc = false;
	for (uint32_t t = b + 1; t < e; ++t) {
		const int32_t c = col[t], r = row[t];
		lo = min(lo, c); hi = max(hi, c);
		desc |= r < prev;
		prev = r;
	}
	if ((uint64_t)(hi - lo) * 16 <= ncol) atomicAdd(&counts[0], 1u);
	if (desc) atomicAdd(&counts[1], 1u);
}

static bool auto_slab(spsamd_ctx *c, const SampledArgs &a, uint64_t ncol)
{
	if (a.k < PROBE_MIN_K) return false;
	const uint32_t groups = (a.nnz + 63) / 64, S = std::min(groups, PROBE_GROUPS);
	uint32_t *counts = c->arena.get<uint32_t>(2);
	fill_zero(c, counts, 2 * sizeof(uint32_t));
	k_sampled_probe<<<dim3(grid_for(S)), dim3(256), 0, c->stream>>>(a.row, a.col, a.nnz, S, ncol, counts);
	SPS_LAUNCH_CHECK();
	const uint64_t both = read_back(c, (const uint64_t *)counts);
	const uint32_t local = (uint32_t)both, descending = (uint32_t)(both >> 32);
	if (2 * local >= S) return false;                                  // mostly local columns: the lane kernel
	return 2 * descending >= S || a.k >= SLAB_MIN_K_SORTED;
}

static void launch_sampled(spsamd_ctx *c, const SampledArgs &a, uint64_t ncol)
{
	const int path = c->tune.sampled_path;
	const bool vec2 = a.ldp % 2 == 0 && a.ldq % 2 == 0 && (uintptr_t)a.P % 16 == 0 && (uintptr_t)a.Q % 16 == 0;
	const bool slab = path == 2 || (path == 0 && auto_slab(c, a, ncol));
	if (slab) {
		const unsigned groups = (a.nnz + 63) / 64;
		const unsigned grid = std::min<unsigned>(groups, (unsigned)c->num_cu * 32);
		if (vec2) k_sampled_slab<2><<<dim3(grid), dim3(64), 0, c->stream>>>(a);
		else k_sampled_slab<1><<<dim3(grid), dim3(64), 0, c->stream>>>(a);
	} else {
		const unsigned grid = std::min<unsigned>(grid_for(a.nnz), (unsigned)c->num_cu * 32);
		if (vec2) k_sampled_lane<2><<<dim3(grid), dim3(256), 0, c->stream>>>(a);
		else k_sampled_lane<1><<<dim3(grid), dim3(256), 0, c->stream>>>(a);
	}
	SPS_LAUNCH_CHECK();
}

// ---- host driver -----------------------------------------------------------------------------------------------------

// Do the byte ranges [a, a + na) and [b, b + nb) share a byte?
static bool overlaps(const void *a, uint64_t na, const void *b, uint64_t nb)
{
	return a && b && na && nb && (const char *)a < (const char *)b + nb && (const char *)b < (const char *)a + na;
}

void multiply_sampled(spsamd_ctx *c, const spsamd_coo *M, char transpose, const double *P, size_t ldp, const double *Q,
	size_t ldq, size_t k, double alpha, double beta, double *out, int mem)
{
	if (!M) throw Error{SPSAMD_EINVAL, "null matrix"};
	const int lead = transpose == 'T' ? 1 : 0;
	const uint64_t shape[2] = {M->shape0, M->shape1};
	const uint64_t nrow = shape[lead], ncol = shape[1 - lead];        // rows of P, rows of Q
	if (ldp < k || ldq < k) throw Error{SPSAMD_EINVAL, "leading dimension of P or Q smaller than k"};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of P, Q and out must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	// (the kernels count r in 32 bits and step it by up to SLAB: k < 2^31 keeps r + SLAB from wrapping)
	if (k >= (size_t(1) << 31)) throw Error{SPSAMD_EINVAL, "k is 2^31 or more"};
	// the tuples: a prepared operand's consolidated ones (its lead's order), else M's arrays as stored
	const OperandView view = operand_view(c, M);
	const Prepared *prep = view.prep;
	const int32_t *i0 = view.coo.idx0, *i1 = view.coo.idx1;
	const double *v = view.coo.val;
	const size_t n = view.coo.nnz;
	const int mmem = view.coo.mem;
	check_operand(view.coo, OPERAND_PLAIN_MEM);                        // a bad mem is refused even where M is empty; val: below
	if (n == 0) return;
	if (k && (!P || !Q)) throw Error{SPSAMD_EINVAL, "null P or Q"};
	if (!out) throw Error{SPSAMD_EINVAL, "null out"};
	if (beta != 0 && !v) throw Error{SPSAMD_EINVAL, "beta != 0 reads M's values, and M->val is null"};
	// the bytes each array spans: rows - 1 full leading dimensions and k values
	const uint64_t obytes = n * sizeof(double);
	const uint64_t pbytes = nrow && k ? ((nrow - 1) * ldp + k) * sizeof(double) : 0;
	const uint64_t qbytes = ncol && k ? ((ncol - 1) * ldq + k) * sizeof(double) : 0;
	if (overlaps(out, obytes, P, pbytes) || overlaps(out, obytes, Q, qbytes)) throw Error{SPSAMD_EINVAL, "out overlaps P or Q"};
	if (overlaps(out, obytes, i0, n * 4) || overlaps(out, obytes, i1, n * 4)) throw Error{SPSAMD_EINVAL, "out overlaps M's index arrays"};
	if (overlaps(out, obytes, v, obytes) && (out != v || prep)) throw Error{SPSAMD_EINVAL, "out overlaps M's values without being them"};

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	// a SINK_COO result of this context handed back in: valid indices
	const bool own_result = prep || is_own_result(c, *M);
	const int32_t *d0 = to_device(c, i0, n, mmem), *d1 = to_device(c, i1, n, mmem);
	const double *dv = beta != 0 ? to_device(c, v, n, mmem) : nullptr;
	SampledArgs a;
	a.row = lead == 0 ? d0 : d1; a.col = lead == 0 ? d1 : d0;
	a.val = dv; a.nnz = (uint32_t)n;
	a.k = (uint32_t)k; a.alpha = alpha; a.beta = beta;
	a.P = P; a.ldp = ldp; a.Q = Q; a.ldq = ldq; a.out = out;
	if (mem == SPSAMD_MEM_HOST) {                                       // packed device copies, k values per row
		double *tp = c->arena.get<double>(k ? nrow * k : 1), *tq = c->arena.get<double>(k ? ncol * k : 1);
		if (k) {
			SPS_HIP(hipMemcpy2DAsync(tp, k * sizeof(double), P, ldp * sizeof(double), k * sizeof(double), nrow, hipMemcpyHostToDevice, c->stream));
			SPS_HIP(hipMemcpy2DAsync(tq, k * sizeof(double), Q, ldq * sizeof(double), k * sizeof(double), ncol, hipMemcpyHostToDevice, c->stream));
		}
		a.P = tp; a.Q = tq; a.ldp = a.ldq = k;
		a.out = c->arena.get<double>(n);
	}
	if (!own_result) {
		// k_inspect reads a value per tuple: M's, or (beta == 0, M->val possibly null) the device output array's current bytes
		const uint32_t f = inspect_operand(c, a.row, a.col, dv ? dv : a.out, n, nrow, ncol);
		if (f & 1u) throw Error{SPSAMD_EINVAL, "Sparse index out of bounds (VectorCooArray::add would reject it, VectorCooArray.hpp:246-262)"};
	}
	launch_sampled(c, a, ncol);
	if (mem == SPSAMD_MEM_HOST)
		SPS_HIP(hipMemcpyAsync(out, a.out, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	SPS_HIP(hipStreamSynchronize(c->stream));
}

} // namespace spsamd
