// sink.hip -- the sink tail (internal.h): which output set of the context a result may overwrite, how a SINK_COO result is
// handed over and remembered as the context's own, the DIGEST of stored tuples, the row statistics, the end of a call.
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

void check_sink_args(int duplicate_policy, int sink_kind)
{
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	if (sink_kind != SPSAMD_SINK_COO && sink_kind != SPSAMD_SINK_DIGEST) throw Error{SPSAMD_EINVAL, "bad sink_kind"};
}

bool output_set_aliased(const spsamd_ctx *c, int s, const spsamd_coo *const *operands, int n)
{
	for (int k = 0; k < n; ++k) {
		const spsamd_coo *X = operands[k];
		if (X && X->mem == SPSAMD_MEM_DEVICE && (c->out[s].holds(X->idx0) || c->out[s].holds(X->idx1) || c->out[s].holds(X->val))) return true;
	}
	return false;
}

void pick_output_set(spsamd_ctx *c, const spsamd_coo *const *operands, int n)
{
	if (!output_set_aliased(c, c->cur_out, operands, n)) return;
	if (output_set_aliased(c, c->cur_out ^ 1, operands, n))
		throw Error{SPSAMD_EINVAL, "both result buffers of this context are operands of the call: copy one of them out first (spsamd_memcpy)"};
	c->cur_out ^= 1;
}

CooOut grow_output(OutSet &o, size_t total)
{
	o.i.ensure(total * 4); o.j.ensure(total * 4); o.v.ensure(total * 8);
	return CooOut{(int32_t *)o.i.p, (int32_t *)o.j.p, (double *)o.v.p};
}

CooOut coo_output(spsamd_ctx *c, size_t total)
{
	c->own[c->cur_out].sort0 = -1;                                     // that set is about to be overwritten
	return grow_output(c->out[c->cur_out], total + 1);
}

CooOut scratch_output(spsamd_ctx *c, size_t total)
{
	int32_t *row = c->arena.get<int32_t>(total + 1), *col = c->arena.get<int32_t>(total + 1);
	return CooOut{row, col, c->arena.get<double>(total + 1)};
}

CooOut counted_output(spsamd_ctx *c, const uint32_t *counts, uint32_t *offs, size_t n, bool coo, uint32_t *total)
{
	scan_exclusive_u32_u32(c, counts, offs, n);
	*total = read_back(c, offs + n);
	return coo ? coo_output(c, *total) : scratch_output(c, *total);
}

void publish_coo(spsamd_ctx *c, spsamd_result *res, const int32_t *orow, const int32_t *ocol, const double *oval, uint64_t total, bool permute)
{
	res->nnz = total;
	res->idx0 = permute ? ocol : orow; res->idx1 = permute ? orow : ocol; res->val = oval;
	auto &w = c->own[c->cur_out];
	w.d0 = res->idx0; w.d1 = res->idx1; w.v = oval; w.nnz = total;
	w.shape0 = res->shape0; w.shape1 = res->shape1; w.sort0 = permute ? 1 : 0;
}

RowStats rowstats_begin(spsamd_ctx *c, uint64_t nrow, size_t slack, spsamd_result *res)
{
	c->rowstat_n.ensure(nrow * sizeof(long long) + slack);
	c->rowstat_s.ensure(nrow * sizeof(double) + slack);
	c->rowstat_h.ensure(nrow * sizeof(unsigned long long) + slack);
	fill_zero(c, c->rowstat_n.p, nrow * sizeof(long long));
	fill_zero(c, c->rowstat_s.p, nrow * sizeof(double));
	fill_zero(c, c->rowstat_h.p, nrow * sizeof(unsigned long long));
	const RowStats rs{(long long *)c->rowstat_n.p, (double *)c->rowstat_s.p, (unsigned long long *)c->rowstat_h.p};
	res->row_nnz = (const int64_t *)rs.nnz; res->row_sum = rs.sum; res->row_hash = (const uint64_t *)rs.hash;
	return rs;
}

// DIGEST sink over the stored tuples: index hash, sum (and the per-row statistics under ROWSTATS)
__global__ void __launch_bounds__(256) k_digest_stored(const int32_t *__restrict__ row, const int32_t *__restrict__ col,
	const double *__restrict__ val, uint32_t n, unsigned long long *hash, double *sum,
	long long *row_nnz, double *row_sum, unsigned long long *row_hash)
{
	unsigned long long h = 0;
	double s = 0;
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		const unsigned long long x = mix64((uint32_t)row[t], (uint32_t)col[t]);
		h += x; s += val[t];
		if (row_nnz) { atomicAdd((unsigned long long *)&row_nnz[row[t]], 1ull); atomicAdd(&row_sum[row[t]], val[t]); atomicAdd(&row_hash[row[t]], x); }
	}
	h = wave_reduce_sum(h); s = wave_reduce_sum(s);
	if (lane_id() == 0) { atomicAdd(hash, h); atomicAdd(sum, s); }
}

void digest_stored(spsamd_ctx *c, spsamd_result *res, const int32_t *orow, const int32_t *ocol, const double *oval, uint32_t total,
	uint64_t nrow, int sink_flags)
{
	hipStream_t st = c->stream;
	unsigned long long *hs = c->arena.get<unsigned long long>(2);
	fill_zero(c, hs, 2 * sizeof(unsigned long long));
	RowStats rs;
	if (sink_flags & SPSAMD_SINK_ROWSTATS) rs = rowstats_begin(c, nrow, 8, res);
	if (total) {
		k_digest_stored<<<dim3(std::min(grid_for(total), 2048u)), dim3(256), 0, st>>>(orow, ocol, oval, total, hs, (double *)(hs + 1), rs.nnz, rs.sum, rs.hash);
		SPS_LAUNCH_CHECK();
	}
	unsigned long long *h = (unsigned long long *)c->host_staging(2 * sizeof(unsigned long long));
	SPS_HIP(hipMemcpyAsync(h, hs, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	SPS_HIP(hipStreamSynchronize(st));
	res->hash = h[0];
	std::memcpy(&res->sum, &h[1], sizeof(double));
}

void finish_call(spsamd_ctx *c, spsamd_result *res)
{
	SPS_HIP(hipEventRecord(c->ev[EV_END], c->stream));
	SPS_HIP(hipEventSynchronize(c->ev[EV_END]));
	SPS_HIP(hipEventElapsedTime(&res->ms_total, c->ev[EV_BEGIN], c->ev[EV_END]));
	res->workspace_bytes = c->arena.call_used;
}

void deliver_stored(spsamd_ctx *c, spsamd_result *res, const CooOut &o, uint32_t total, uint64_t nrow, bool coo, bool permute, int sink_flags)
{
	res->nnz = total;
	if (coo) publish_coo(c, res, o.row, o.col, o.val, total, permute);
	else digest_stored(c, res, o.row, o.col, o.val, total, nrow, sink_flags);
	finish_call(c, res);
}

} // namespace spsamd
