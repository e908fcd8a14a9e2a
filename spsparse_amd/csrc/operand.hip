// operand.hip -- operand intake (internal.h): what every entry point settles about a spsamd_coo before its own work
// starts -- which arrays hold its tuples, whether they may be trusted without the inspection pass, the argument checks --
// and the frame of a product.  Each rule is written here once; what an operation does after intake is in its own file.
#include "internal.h"

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

__global__ void __launch_bounds__(256) k_gather_sorted(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm,
	const double *__restrict__ val, uint32_t n, int minor_bits, int32_t *__restrict__ row, int32_t *__restrict__ col,
	double *__restrict__ oval)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = keys[i];
	row[i] = (int32_t)(k >> minor_bits);
	col[i] = (int32_t)(k & ((uint64_t(1) << minor_bits) - 1));
	oval[i] = val[perm[i]];
}

// (n < 2^31 tuples: check_operand)
void build_keys(spsamd_ctx *c, const int32_t *major, const int32_t *minor, size_t n, int minor_bits, uint64_t *keys)
{
	k_build_keys<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(major, minor, (uint32_t)n, minor_bits, keys);
	SPS_LAUNCH_CHECK();
}

void gather_sorted(spsamd_ctx *c, const uint64_t *keys, const uint32_t *perm, const double *val, size_t n, int minor_bits,
	int32_t *row, int32_t *col, double *oval)
{
	k_gather_sorted<<<dim3(grid_for(n)), dim3(256), 0, c->stream>>>(keys, perm, val, (uint32_t)n, minor_bits, row, col, oval);
	SPS_LAUNCH_CHECK();
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
