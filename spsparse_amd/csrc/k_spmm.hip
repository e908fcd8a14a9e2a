// k_spmm.hip -- Y (op)= op(M) * X for dense X with nrhs right-hand sides: the reference's multiply(M, x, y, handle_nan,
// transpose) (multiply_dense.hpp:11-35, compiled out there) with y a DenseAccum (accum.hpp:110-140).
//
// The reference walks M's tuples in storage order and applies, per right-hand side r,
//     p = v * X[j, r];  if (handle_nan && !isfinite(p)) skip;  Y[i, r] (op)= p
// Every entry of Y is bit-identical to that loop here:
//   - the tuples are put in order of the OUTPUT row by a stable sort (storage order inside a row), so each (row, rhs) is one
//     serial chain of adds in storage order -- no tree reduction, no FMA (the build has -ffp-contract=off);
//   - a NaN result takes the bits x86-64 SSE gives it (the reference's build): the left operand's NaN, quieted, if it is
//     one, else the right operand's, else the default NaN 0xFFF8000000000000 (0 * Inf, Inf - Inf).  The left operand is
//     `val` in `val * x` and the accumulated entry in `oval += val`.
//
// Kernel shapes (DESIGN.md "Applying an operator to dense vectors"):
//   serial   one thread per (row, rhs), rhs fastest: the rows of up to `long_min` tuples
//   lanes    one wave per row, lanes across the right-hand sides, tuples read wave-uniform: long rows, nrhs >= 16
//   fold     one wave per row, 64 products at a time across the lanes into LDS, then one ordered fold per rhs by one
//            lane each: long rows, nrhs < 16
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

namespace spsamd {

// One step of DenseAccum::add (accum.hpp:124-135) on the entry y with the product p.
template <int POLICY, bool HNAN>
__device__ __forceinline__ void accum(double &y, double p)
{
	if (HNAN && !isfinite(p)) return;                              // multiply_dense.hpp:19-20
	if (POLICY == SPSAMD_ADD) { const double s = y + p; y = s != s ? x86_nan(y, p) : s; }
	else if (POLICY == SPSAMD_REPLACE) y = p;
	else if (!(y != y)) y = p;                                      // LEAVE_ALONE as accum.hpp:128-130 spells it
}

__device__ __forceinline__ double tup_val(const BTup &t) { return __hiloint2double((int)t.vhi, (int)t.vlo); }

// ---- serial: one thread per (row, rhs) ---------------------------------------------------------------------------
template <int POLICY, bool HNAN>
__global__ void __launch_bounds__(256) k_spmm_serial(const uint32_t *__restrict__ rowptr, const BTup *__restrict__ tup, uint64_t nrow,
	const double *__restrict__ X, uint64_t ldx, double *__restrict__ Y, uint64_t ldy, uint32_t nrhs, uint32_t long_min)
{
	const uint64_t total = nrow * nrhs;
	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint64_t row = t / nrhs, r = t - row * nrhs;
		const uint32_t b = rowptr[row], e = rowptr[row + 1];
		if (b == e || e - b > long_min) continue;                   // empty: Y keeps its value; long: the wave kernels
		double *yp = Y + row * ldy + r;
		double y = *yp;
		const double *xr = X + r;
#pragma unroll 4
		for (uint32_t k = b; k < e; ++k) {
			const BTup tp = tup[k];
			accum<POLICY, HNAN>(y, ref_mul(tup_val(tp), xr[(uint64_t)(uint32_t)tp.col * ldx]));
		}
		*yp = y;
	}
}

// Rows with more than long_min tuples (long_min = 0: every non-empty row), appended in any order: each is one work item.
__global__ void k_spmm_long_rows(const uint32_t *__restrict__ rowptr, uint64_t nrow, uint32_t long_min, uint32_t *list, uint32_t *count)
{
	const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool is_long = row < nrow && rowptr[row + 1] - rowptr[row] > long_min;
	const uint32_t slot = wave_claim(count, is_long);
	if (is_long) list[slot] = (uint32_t)row;
}

// ---- lanes: one wave per long row, lane = right-hand side ---------------------------------------------------------
template <int POLICY, bool HNAN>
__global__ void __launch_bounds__(64) k_spmm_lanes(const uint32_t *__restrict__ rowptr, const BTup *__restrict__ tup,
	const uint32_t *__restrict__ list, const uint32_t *__restrict__ count,
	const double *__restrict__ X, uint64_t ldx, double *__restrict__ Y, uint64_t ldy, uint32_t nrhs)
{
	const uint32_t n = *count;
	for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
		const uint64_t row = list[w];
		const uint32_t b = rowptr[row], e = rowptr[row + 1];
		for (uint32_t rb = 0; rb < nrhs; rb += 64) {
			const uint32_t r = rb + lane_id();
			const bool on = r < nrhs;
			double *yp = Y + row * ldy + r;
			double y = on ? *yp : 0.0;
			const double *xr = X + r;
#pragma unroll 4
			for (uint32_t k = b; k < e; ++k) {
				const BTup tp = tup[k];                                // wave-uniform
				const double x = on ? xr[(uint64_t)(uint32_t)tp.col * ldx] : 0.0;
				accum<POLICY, HNAN>(y, ref_mul(tup_val(tp), x));
			}
			if (on) *yp = y;
		}
	}
}

// ---- fold: one wave per long row, products 64 at a time, ordered fold per rhs ------------------------------------
constexpr int FOLD_RHS = 16;                      // right-hand sides per pass over the row (LDS: FOLD_RHS x 65 doubles)

template <int POLICY, bool HNAN>
__global__ void __launch_bounds__(64) k_spmm_fold(const uint32_t *__restrict__ rowptr, const BTup *__restrict__ tup,
	const uint32_t *__restrict__ list, const uint32_t *__restrict__ count,
	const double *__restrict__ X, uint64_t ldx, double *__restrict__ Y, uint64_t ldy, uint32_t nrhs)
{
	__shared__ double prod[FOLD_RHS][65];                          // [rhs][product]; 65: the fold's column walk spreads over the banks
	const uint32_t n = *count;
	const unsigned lane = lane_id();
	for (uint32_t w = blockIdx.x; w < n; w += gridDim.x) {
		const uint64_t row = list[w];
		const uint32_t b = rowptr[row], e = rowptr[row + 1];
		for (uint32_t rb = 0; rb < nrhs; rb += FOLD_RHS) {
			const uint32_t nr = min((uint32_t)FOLD_RHS, nrhs - rb);
			double *yp = Y + row * ldy + rb + lane;
			double y = lane < nr ? *yp : 0.0;
			for (uint32_t k0 = b; k0 < e; k0 += 64) {
				const uint32_t cnt = min(64u, e - k0);
				if (lane < cnt) {
					const BTup tp = tup[k0 + lane];
					const double v = tup_val(tp);
					const double *xr = X + (uint64_t)(uint32_t)tp.col * ldx + rb;
					for (uint32_t q = 0; q < nr; ++q) prod[q][lane] = ref_mul(v, xr[q]);
				}
				__syncthreads();
				if (lane < nr) {
					// eight LDS reads in flight ahead of the adds: the chain then waits on the adds, not on each read
					uint32_t q = 0;
					for (; q + 8 <= cnt; q += 8) {
						double p[8];
#pragma unroll
						for (int u = 0; u < 8; ++u) p[u] = prod[lane][q + u];
#pragma unroll
						for (int u = 0; u < 8; ++u) accum<POLICY, HNAN>(y, p[u]);
					}
					for (; q < cnt; ++q) accum<POLICY, HNAN>(y, prod[lane][q]);
				}
				__syncthreads();
			}
			if (lane < nr) *yp = y;
		}
	}
}

template <int POLICY, bool HNAN>
static void launch_spmm(spsamd_ctx *c, const DenseOperand &m, const double *X, uint64_t ldx, double *Y, uint64_t ldy, uint32_t nrhs)
{
	hipStream_t st = c->stream;
	const int path = c->tune.spmm_path;
	// serial rows: up to long_min tuples (0 in a forced wave path: no row is serial)
	const uint32_t long_min = path == 1 ? 0xFFFFFFFFu : path >= 2 ? 0u : c->tune.spmm_long_min > 0 ? (uint32_t)c->tune.spmm_long_min : 64u;
	if (path != 2 && path != 3) {
		const uint64_t total = m.nrow * nrhs;
		const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(total), (uint64_t)c->num_cu * 64);
		k_spmm_serial<POLICY, HNAN><<<dim3(grid), dim3(256), 0, st>>>(m.rowptr, m.tup, m.nrow, X, ldx, Y, ldy, nrhs, long_min);
		SPS_LAUNCH_CHECK();
	}
	if (path == 1) return;
	uint32_t *count = c->arena.get<uint32_t>(1), *list = c->arena.get<uint32_t>(m.nrow ? m.nrow : 1);
	fill_zero(c, count, sizeof(uint32_t));
	k_spmm_long_rows<<<dim3(grid_for(m.nrow)), dim3(256), 0, st>>>(m.rowptr, m.nrow, long_min, list, count);
	SPS_LAUNCH_CHECK();
	// persistent waves over the list (its length stays on the device)
	const unsigned waves = (unsigned)c->num_cu * 8;
	const bool lanes = path == 2 || (path == 0 && nrhs >= 16);
	if (lanes) k_spmm_lanes<POLICY, HNAN><<<dim3(waves), dim3(64), 0, st>>>(m.rowptr, m.tup, list, count, X, ldx, Y, ldy, nrhs);
	else k_spmm_fold<POLICY, HNAN><<<dim3(waves), dim3(64), 0, st>>>(m.rowptr, m.tup, list, count, X, ldx, Y, ldy, nrhs);
	SPS_LAUNCH_CHECK();
}

void spmm_dense(spsamd_ctx *c, const DenseOperand &m, const double *X, uint64_t ldx, double *Y, uint64_t ldy, uint32_t nrhs,
	int policy, bool handle_nan)
{
	if (!m.nnz || !nrhs) return;
#define SPMM_CASE(P)                                                                          \
	if (policy == P) {                                                                        \
		if (handle_nan) launch_spmm<P, true>(c, m, X, ldx, Y, ldy, nrhs);                       \
		else launch_spmm<P, false>(c, m, X, ldx, Y, ldy, nrhs);                                 \
		return;                                                                               \
	}
	SPMM_CASE(SPSAMD_ADD)
	SPMM_CASE(SPSAMD_REPLACE)
	SPMM_CASE(SPSAMD_LEAVE_ALONE)
#undef SPMM_CASE
	throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
}

// ---- the tuples of op(M) in order of the output row ----------------------------------------------------------------

__global__ void k_pack_rows(const int32_t *__restrict__ minor, const double *__restrict__ val, uint32_t n, BTup *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const double v = val[i];
	BTup t; t.col = minor[i]; t.vlo = (uint32_t)__double2loint(v); t.vhi = (uint32_t)__double2hiint(v);
	out[i] = t;
}

// (declared in internal.h: spsamd_solve_pcg packs an operand it took itself)
void pack_tuples(spsamd_ctx *c, const int32_t *minor, const double *val, uint32_t n, BTup *out)
{
	if (!n) return;
	k_pack_rows<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(minor, val, n, out);
	SPS_LAUNCH_CHECK();
}

// (declared in internal.h) launch_spmm's two halves of the long rows for a caller that applies one operand many times: the
// list once ...
uint32_t spmm_long_list(spsamd_ctx *c, const uint32_t *rowptr, uint64_t nrow, uint32_t long_min, uint32_t **list, uint32_t **count)
{
	*count = get_zeroed<uint32_t>(c, 1);
	*list = c->arena.get<uint32_t>(nrow ? nrow : 1);
	k_spmm_long_rows<<<dim3(grid_for(nrow)), dim3(256), 0, c->stream>>>(rowptr, nrow, long_min, *list, *count);
	SPS_LAUNCH_CHECK();
	return read_back(c, *count);
}

// ... and the wave kernel over it per application (ADD, handle_nan off): one launch, nothing allocated
void spmm_long_rows(spsamd_ctx *c, const DenseOperand &m, const uint32_t *list, const uint32_t *count, const double *X, uint64_t ldx,
	double *Y, uint64_t ldy, uint32_t nrhs)
{
	const unsigned waves = (unsigned)c->num_cu * 8;
	const bool lanes = c->tune.spmm_path == 2 || (c->tune.spmm_path == 0 && nrhs >= 16);
	if (lanes) k_spmm_lanes<SPSAMD_ADD, false><<<dim3(waves), dim3(64), 0, c->stream>>>(m.rowptr, m.tup, list, count, X, ldx, Y, ldy, nrhs);
	else k_spmm_fold<SPSAMD_ADD, false><<<dim3(waves), dim3(64), 0, c->stream>>>(m.rowptr, m.tup, list, count, X, ldx, Y, ldy, nrhs);
	SPS_LAUNCH_CHECK();
}

__global__ void k_row_keys(const int32_t *__restrict__ major, uint32_t n, uint64_t *__restrict__ keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = (uint64_t)(uint32_t)major[i];
}

// tuple i of the ordered copy is tuple perm[i] of the storage
__global__ void k_gather_rows(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm, const int32_t *__restrict__ minor,
	const double *__restrict__ val, uint32_t n, int32_t *__restrict__ row, BTup *__restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = perm[i];
	const double v = val[s];
	BTup t; t.col = minor[s]; t.vlo = (uint32_t)__double2loint(v); t.vhi = (uint32_t)__double2hiint(v);
	out[i] = t;
	row[i] = (int32_t)keys[i];
}

void dense_operand(spsamd_ctx *c, const spsamd_coo *M, int lead, DenseOperand *out)
{
	const uint64_t shape[2] = {M->shape0, M->shape1};
	out->nrow = shape[lead]; out->ncol = shape[1 - lead];
	out->nnz = 0; out->rowptr = nullptr; out->tup = nullptr; out->sorted = false;
	const OperandView view = operand_view(c, M);
	if (view.prep && view.prep->lead == lead) {
		// consolidated by the output row already: its packed tuples and dense row pointer (both kept in the handle)
		Prepared *p = view.prep;
		out->nnz = p->m.nnz;
		if (!out->nnz) return;
		prepared_row_structure(c, p);
		out->rowptr = p->rowptr;
		out->tup = prepared_btup(c, p);
		return;
	}
	M = &view.coo;                                                     // (prepared the other way round: its tuples as stored)
	const size_t n = M->nnz;
	if (n == 0) return;
	check_operand(*M, OPERAND_VALUES);                                 // (mem was never checked here: whatever is not HOST is read as device memory)
	out->nnz = (uint32_t)n;
	// a SINK_COO result of this context handed back in: valid indices, ascending rows (by sort0)
	const bool own_result = is_own_result(c, *M);
	const int32_t *d0 = to_device(c, M->idx0, n, M->mem);
	const int32_t *d1 = to_device(c, M->idx1, n, M->mem);
	const double *dv = to_device(c, M->val, n, M->mem);
	const int32_t *major = lead == 0 ? d0 : d1, *minor = lead == 0 ? d1 : d0;
	bool ordered = own_result && M->sort0 == lead;
	if (!own_result) {
		const uint32_t f = inspect_operand(c, major, minor, dv, n, out->nrow, out->ncol);
		if (f & 1u) throw Error{SPSAMD_EINVAL, "Sparse index out of bounds (VectorCooArray::add would reject it, VectorCooArray.hpp:246-262)"};
		ordered = !(f & 16u);                                          // the output row never descends: storage order is row order
	}
	BTup *tup = c->arena.get<BTup>(n);
	ConMat rows;
	rows.nnz = (uint32_t)n; rows.nrow = out->nrow; rows.ncol = out->ncol;
	if (ordered) {
		k_pack_rows<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(minor, dv, (uint32_t)n, tup);
		SPS_LAUNCH_CHECK();
		rows.row = const_cast<int32_t *>(major);
	} else {
		// one stable radix pass set keyed on the output row alone, storage position as payload
		PairSort sort(c, n);
		k_row_keys<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(major, (uint32_t)n, sort.keys);
		SPS_LAUNCH_CHECK();
		sort.run(bits_of(out->nrow));
		int32_t *srow = c->arena.get<int32_t>(n);
		k_gather_rows<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(sort.keys, sort.perm, minor, dv, (uint32_t)n, srow, tup);
		SPS_LAUNCH_CHECK();
		rows.row = srow;
		out->sorted = true;
	}
	out->rowptr = dense_rowptr(c, rows, 0u);
	out->tup = tup;
}

} // namespace spsamd
