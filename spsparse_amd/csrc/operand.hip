// operand.hip -- operand intake (internal.h): what every entry point settles about a spsamd_coo before its own work
// starts -- which arrays hold its tuples, whether they may be trusted without the inspection pass, the argument checks --
// and the frame of a product.  Each rule is written here once; what an operation does after intake is in its own file.
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cstdio>

namespace spsamd {

OperandView operand_view(spsamd_ctx *c, const spsamd_coo *X)
{
	OperandView v;
	v.coo = *X;
	if (X->mem != SPSAMD_MEM_PREPARED) return v;
	// a prepared operand (spsamd_operand_prepare; idx0 carries the handle): consolidated once, by the lead it was prepared
	// for.  Used the other way round ('T' now, '.' then) its tuples are an ordinary device operand sorted by the other dimension.
	Prepared *p = (Prepared *)const_cast<int32_t *>(X->idx0);
	if (!p || p->ctx != c) throw Error{SPSAMD_EINVAL, "a prepared operand belongs to the context that prepared it"};
	v.prep = p;
	v.coo.idx0 = p->lead == 0 ? p->m.row : p->m.col; v.coo.idx1 = p->lead == 0 ? p->m.col : p->m.row; v.coo.val = p->m.val;
	v.coo.nnz = p->m.nnz; v.coo.sort0 = p->lead; v.coo.mem = SPSAMD_MEM_DEVICE;
	return v;
}

uint64_t operand_tuples(const spsamd_coo *X)
{
	if (X->mem == SPSAMD_MEM_PREPARED) return X->idx0 ? ((const Prepared *)X->idx0)->m.nnz : 0;
	return X->nnz;
}

void check_operand(const spsamd_coo &X, int flags)
{
	if ((flags & OPERAND_PLAIN_MEM) && X.mem != SPSAMD_MEM_HOST && X.mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "bad mem of an operand"};
	if (X.nnz == 0) return;
	if (X.nnz >= (size_t(1) << 31))
		throw Error{SPSAMD_EINVAL, "operand has 2^31 or more tuples (the reference's int positions cap it too, algorithm.hpp:419)"};
	if (!X.idx0 || !X.idx1 || ((flags & OPERAND_VALUES) && !X.val)) throw Error{SPSAMD_EINVAL, "operand with nnz > 0 has a null array"};
	if (X.shape0 > (uint64_t(1) << 31) || X.shape1 > (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "shape exceeds the int32 index range"};
}

bool is_own_result(const spsamd_ctx *c, const spsamd_coo &X)
{
	if (X.mem != SPSAMD_MEM_DEVICE) return false;
	for (const auto &o : c->own)
		if (o.sort0 >= 0 && o.sort0 == X.sort0 && o.d0 == X.idx0 && o.d1 == X.idx1 && o.v == X.val && o.nnz == X.nnz &&
			o.shape0 == X.shape0 && o.shape1 == X.shape1) return true;
	return false;
}

int bits_of(uint64_t dim)
{
	int b = 0;
	while (b < 63 && (uint64_t(1) << b) < dim) ++b;
	return b;
}

__global__ void __launch_bounds__(256) k_build_keys(const int32_t *__restrict__ major, const int32_t *__restrict__ minor, uint32_t n,
	int minor_bits, uint64_t *__restrict__ keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = ((uint64_t)(uint32_t)major[i] << minor_bits) | (uint64_t)(uint32_t)minor[i];
}

__global__ void __launch_bounds__(256) k_gather_sorted(SortedKeys sk,
	const double *__restrict__ val, uint32_t n, int minor_bits, int32_t *__restrict__ row, int32_t *__restrict__ col,
	double *__restrict__ oval)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = sk.key(i);
	const double v = val[sk.pos(i)];                       // (before the stores: nothing says they do not alias the position array)
	row[i] = (int32_t)(k >> minor_bits);
	col[i] = (int32_t)(k & ((uint64_t(1) << minor_bits) - 1));
	oval[i] = v;
}

// (n < 2^31 tuples: check_operand)
void build_keys(spsamd_ctx *c, const int32_t *major, const int32_t *minor, size_t n, int minor_bits, uint64_t *keys)
{
	k_build_keys<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(major, minor, (uint32_t)n, minor_bits, keys);
	SPS_LAUNCH_CHECK();
}

void gather_sorted(spsamd_ctx *c, const SortedKeys &sk, const double *val, size_t n, int minor_bits,
	int32_t *row, int32_t *col, double *oval)
{
	k_gather_sorted<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(sk, val, (uint32_t)n, minor_bits, row, col, oval);
	SPS_LAUNCH_CHECK();
}

PlainStream plain_stream(spsamd_ctx *c, const spsamd_coo &X, int lead)
{
	check_operand(X, OPERAND_VALUES | OPERAND_PLAIN_MEM);
	const size_t n = X.nnz;
	const uint64_t shape[2] = {X.shape0, X.shape1};
	PlainStream s;
	s.own_result = is_own_result(c, X);
	const int32_t *d0 = to_device(c, X.idx0, n, X.mem), *d1 = to_device(c, X.idx1, n, X.mem);
	s.val = to_device(c, X.val, n, X.mem);
	s.major = lead == 0 ? d0 : d1; s.minor = lead == 0 ? d1 : d0;
	if (s.own_result) return s;
	s.flags = inspect_operand(c, s.major, s.minor, s.val, n, shape[lead], shape[1 - lead]);
	if (s.flags & 1u) throw Error{SPSAMD_EINVAL, "Sparse index out of bounds (VectorCooArray::add would reject it, VectorCooArray.hpp:246-262)"};
	if (X.sort0 == lead && (s.flags & 32u))
		throw Error{SPSAMD_EINVAL, "operand claims sort_order but its (row, col) keys are not in that order (set_sorted() on unsorted tuples?)"};
	return s;
}

// ---------------------------------------------------------------- structural keys (a mask M, emult's pattern operand)

// bit0: an index out of bounds; bit1: the (row, col) key descends somewhere; bit2: a key repeats its predecessor
__global__ void __launch_bounds__(256) k_mask_inspect(const int32_t *__restrict__ r, const int32_t *__restrict__ c, size_t n,
	uint64_t nrow, uint64_t ncol, uint32_t *flags)
{
	uint32_t f = 0;
	for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
		const int32_t x = r[t], y = c[t];
		if (x < 0 || (uint64_t)x >= nrow || y < 0 || (uint64_t)y >= ncol) f |= 1u;
		if (t > 0) {
			const int32_t px = r[t - 1], py = c[t - 1];
			if (px > x || (px == x && py > y)) f |= 2u;
			if (px == x && py == y) f |= 4u;
		}
	}
	uint32_t wf = 0;
	for (uint32_t b = 1u; b <= 4u; b <<= 1) if (__ballot(f & b)) wf |= b;
	if (lane_id() == 0 && wf) atomicOr(flags, wf);
}

__global__ void __launch_bounds__(256) k_mask_first(const uint64_t *__restrict__ keys, uint32_t n, uint8_t *__restrict__ first)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < n) first[t] = t == 0 || keys[t] != keys[t - 1];
}

__global__ void __launch_bounds__(256) k_mask_unique(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ first,
	const uint32_t *__restrict__ off, uint32_t n, int cbits, int32_t *__restrict__ mi, int32_t *__restrict__ mj)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n || !first[t]) return;
	const uint64_t k = keys[t];
	mi[off[t]] = (int32_t)(k >> cbits);
	mj[off[t]] = (int32_t)(k & ((uint64_t(1) << cbits) - 1));
}

void mask_keys(spsamd_ctx *c, const spsamd_coo *M, int lead, uint64_t nrow, uint64_t ncol, MaskKeys *out)
{
	*out = MaskKeys();
	const OperandView view = operand_view(c, M);
	if (view.prep && view.prep->lead == lead) { out->i = view.prep->m.row; out->j = view.prep->m.col; out->n = view.prep->m.nnz; out->prep = view.prep; return; }     // consolidated in op()'s row order
	const spsamd_coo &X = view.coo;                  // (prepared for the other transpose: its consolidated tuples, sorted the other way)
	const size_t n = X.nnz;
	if (n == 0) return;
	check_operand(X, OPERAND_PLAIN_MEM);             // only M's keys are read: val may be null
	const int32_t *d0 = to_device(c, X.idx0, n, X.mem), *d1 = to_device(c, X.idx1, n, X.mem);
	const int32_t *r = lead == 0 ? d0 : d1, *cc = lead == 0 ? d1 : d0;
	uint32_t *flags = c->arena.get<uint32_t>(1);
	fill_zero(c, flags, sizeof(uint32_t));
	k_mask_inspect<<<dim3(std::min(grid_for(n, 1024), 2048u)), dim3(256), 0, c->stream>>>(r, cc, n, nrow, ncol, flags);
	SPS_LAUNCH_CHECK();
	const uint32_t f = read_back(c, flags);
	if (f & 1u) throw Error{SPSAMD_EINVAL, "pattern operand: index out of bounds"};
	if (X.sort0 == lead && (f & 2u))
		throw Error{SPSAMD_EINVAL, "pattern operand claims op()'s row order but its (row, col) keys are not in that order"};
	if (!(f & 6u)) { out->i = r; out->j = cc; out->n = (uint32_t)n; return; }      // in order, no repeats: read in place
	const int cb = bits_of(ncol), rb = bits_of(nrow);
	const uint64_t *keys;
	if (f & 2u) {
		PairSort sort(c, n);
		build_keys(c, r, cc, n, cb, sort.keys);
		sort.run(cb + rb);
		keys = sort.keys;
	} else {                                         // in order with repeats: the keys as they stand
		uint64_t *k = c->arena.get<uint64_t>(n);
		build_keys(c, r, cc, n, cb, k);
		keys = k;
	}
	uint8_t *first = c->arena.get<uint8_t>(n);
	uint32_t *off = c->arena.get<uint32_t>(n + 1);
	k_mask_first<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(keys, (uint32_t)n, first);
	SPS_LAUNCH_CHECK();
	scan_exclusive_u8_u32(c, first, off, n);
	const uint32_t nu = read_back(c, off + n);
	int32_t *mi = c->arena.get<int32_t>(nu), *mj = c->arena.get<int32_t>(nu);
	k_mask_unique<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(keys, first, off, (uint32_t)n, cb, mi, mj);
	SPS_LAUNCH_CHECK();
	out->i = mi; out->j = mj; out->n = nu;
}

ProductFrame::ProductFrame(const spsamd_coo *A, char transpose_A, const spsamd_coo *B, char transpose_B, bool permute)
{
	a0 = transpose_A == 'T' ? 1 : 0; a1 = 1 - a0;
	bk = transpose_B == 'T' ? 1 : 0; bj = 1 - bk;
	const uint64_t ashape[2] = {A->shape0, A->shape1}, bshape[2] = {B->shape0, B->shape1};
	nrow = ashape[a0]; inner = ashape[a1]; inner_b = bshape[bk]; ncol = bshape[bj];
	shape0 = permute ? ncol : nrow;
	shape1 = permute ? nrow : ncol;
}

void ProductFrame::check_inner(const char *what) const
{
	if (inner == inner_b) return;
	char buf[160];
	std::snprintf(buf, sizeof buf, "Inner dimensions for A (%ld) and %s (%ld) must match!", (long)inner, what, (long)inner_b);
	throw Error{SPSAMD_EDIM, buf};
}

bool product_is_empty(double C, const spsamd_vec *scalei, const spsamd_coo *A, const spsamd_vec *scalej, const spsamd_coo *B,
	const spsamd_vec *scalek)
{
	return C == 0 || (scalei && scalei->nnz == 0) || A->nnz == 0 || (scalej && scalej->nnz == 0) || B->nnz == 0 ||
		(scalek && scalek->nnz == 0);
}

} // namespace spsamd
