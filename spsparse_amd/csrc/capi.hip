// capi.hip -- the extern "C" boundary declared in include/spsparse_amd.h.
// Argument handling mirrors spsparse::multiply (multiply_sparse.hpp:152-248):
// shape first (:169), inner-dimension check (:172-174), short-circuits
// (:178-184), consolidation of both operands (:187-188), then the product.
#include "internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <exception>
#include <vector>

using namespace spsamd;

// (a streamed multiply's callback runs while the call still works on the context: every entry point refuses it)
#define API_GUARD(ctx, ...)                                                         \
	if ((ctx)->busy) { (ctx)->last_error = "context busy: a streamed multiply is delivering on it"; return SPSAMD_EINVAL; } \
	try { __VA_ARGS__ }                                                             \
	catch (const spsamd::Error &e) { (ctx)->last_error = e.msg; return e.code; }    \
	catch (const std::bad_alloc &) { (ctx)->last_error = "host allocation failed"; return SPSAMD_ENOMEM; } \
	catch (const std::exception &e) { (ctx)->last_error = e.what(); return SPSAMD_EINVAL; }

extern "C" const char *spsamd_version(void) { return "spsparse_amd 0.2 (gfx950)"; }

extern "C" int spsamd_ctx_create(spsamd_ctx **out, int device, void *hip_stream)
{
	if (!out) return SPSAMD_EINVAL;
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { (void)hipGetLastError(); return SPSAMD_ENODEVICE; }
	if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return SPSAMD_ENODEVICE; }
	if (device >= ndev) return SPSAMD_ENODEVICE;
	if (hipSetDevice(device) != hipSuccess) return SPSAMD_ENODEVICE;
	spsamd_ctx *c = new (std::nothrow) spsamd_ctx();
	if (!c) return SPSAMD_ENOMEM;
	c->device = device;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
	if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->own_stream = false; }
	else {
		if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SPSAMD_EHIP; }
		c->own_stream = true;
	}
	// (from here on a failure hands the context to spsamd_ctx_destroy, which releases whatever exists already)
	for (auto &e : c->ev) if (hipEventCreate(&e) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	for (auto &e : c->ev2) if (hipEventCreate(&e) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	for (auto &e : c->ev_side) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	if (hipStreamCreateWithFlags(&c->side2, hipStreamNonBlocking) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	for (auto &e : c->ev_side2) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { spsamd_ctx_destroy(c); return SPSAMD_EHIP; }
	// developer knobs: the environment is consulted here and nowhere else
	static const char *const knobs[] = {"window", "cell_cap", "dense_min", "no_tiles", "xcd", "emit_path", "light_path", "no_wmajor", "direct_min", "tiles_v1", "long_cap", "long_dense_min", "few_max", "index_budget_mb", "trace", "light_two_pass", "spmm_path", "spmm_long_min", "add_path", "masked_path", "sampled_path", "select_path", "extract_path", "reduce_path", "emult_path", "tile_walk", "solve_path", "solve_row", "solve_fuse_rows", "factor_path", "factor_row", "factor_fuse_rows", "factor_serial_work", "factor_lds_row", "color_path", "color_row", "color_fuse_rows", "color_wave_deg", "agg_path", "agg_row", "agg_fuse_rows", "agg_wave_deg", "agg_per_rows", "pcg_check_every", "pcg_fuse", "amg_path", "amg_fuse_rows", "gmres_path"};
	static const char *const envs[] = {"SPSAMD_W", "SPSAMD_CELL_CAP", "SPSAMD_DENSE_MIN", "SPSAMD_NO_TILES", "SPSAMD_XCD", "SPSAMD_EMIT_PATH", "SPSAMD_LIGHT_PATH", "SPSAMD_NO_WMAJOR", "SPSAMD_DIRECT_MIN", "SPSAMD_TILES_V1", "SPSAMD_LONG_CAP", "SPSAMD_LONG_DENSE_MIN", "SPSAMD_FEW_MAX", "SPSAMD_INDEX_BUDGET_MB", "SPSAMD_TRACE", "SPSAMD_LIGHT_TWO_PASS", "SPSAMD_SPMM_PATH", "SPSAMD_SPMM_LONG_MIN", "SPSAMD_ADD_PATH", "SPSAMD_MASKED_PATH", "SPSAMD_SAMPLED_PATH", "SPSAMD_SELECT_PATH", "SPSAMD_EXTRACT_PATH", "SPSAMD_REDUCE_PATH", "SPSAMD_EMULT_PATH", "SPSAMD_TILE_WALK", "SPSAMD_SOLVE_PATH", "SPSAMD_SOLVE_ROW", "SPSAMD_SOLVE_FUSE_ROWS", "SPSAMD_FACTOR_PATH", "SPSAMD_FACTOR_ROW", "SPSAMD_FACTOR_FUSE_ROWS", "SPSAMD_FACTOR_SERIAL_WORK", "SPSAMD_FACTOR_LDS_ROW", "SPSAMD_COLOR_PATH", "SPSAMD_COLOR_ROW", "SPSAMD_COLOR_FUSE_ROWS", "SPSAMD_COLOR_WAVE_DEG", "SPSAMD_AGG_PATH", "SPSAMD_AGG_ROW", "SPSAMD_AGG_FUSE_ROWS", "SPSAMD_AGG_WAVE_DEG", "SPSAMD_AGG_PER_ROWS", "SPSAMD_PCG_CHECK_EVERY", "SPSAMD_PCG_FUSE", "SPSAMD_AMG_PATH", "SPSAMD_AMG_FUSE_ROWS", "SPSAMD_GMRES_PATH"};
	static_assert(sizeof knobs / sizeof knobs[0] == sizeof envs / sizeof envs[0], "one environment variable per knob");
	for (size_t k = 0; k < sizeof knobs / sizeof knobs[0]; ++k)
		if (const char *e = getenv(envs[k])) (void)spsamd_ctx_set_tuning(c, knobs[k], atol(e));
#ifdef SPSAMD_ABLATIONS
	if (const char *e = getenv("SPSAMD_DBG")) c->tune.dbg = atoi(e);
#endif
	*out = c;
	return SPSAMD_OK;
}

extern "C" int spsamd_ctx_set_tuning(spsamd_ctx *c, const char *name, long value)
{
	if (!c || !name) return SPSAMD_EINVAL;
	if (c->busy) { c->last_error = "context busy: a streamed multiply is delivering on it"; return SPSAMD_EINVAL; }
	struct { const char *n; int *p; } tab[] = {
		{"window", &c->tune.window}, {"cell_cap", &c->tune.cell_cap}, {"dense_min", &c->tune.dense_min},
		{"no_tiles", &c->tune.no_tiles}, {"xcd", &c->tune.xcd}, {"emit_path", &c->tune.emit_path},
		{"light_path", &c->tune.light_path}, {"no_wmajor", &c->tune.no_wmajor}, {"direct_min", &c->tune.direct_min}, {"tiles_v1", &c->tune.tiles_v1}, {"long_cap", &c->tune.long_cap}, {"long_dense_min", &c->tune.long_dense_min}, {"few_max", &c->tune.few_max}, {"index_budget_mb", &c->tune.index_budget_mb}, {"trace", &c->tune.trace}, {"light_two_pass", &c->tune.light_two_pass},
		{"spmm_path", &c->tune.spmm_path}, {"spmm_long_min", &c->tune.spmm_long_min}, {"add_path", &c->tune.add_path},
		{"masked_path", &c->tune.masked_path}, {"sampled_path", &c->tune.sampled_path}, {"select_path", &c->tune.select_path},
		{"extract_path", &c->tune.extract_path}, {"reduce_path", &c->tune.reduce_path}, {"emult_path", &c->tune.emult_path},
		{"tile_walk", &c->tune.tile_walk}, {"solve_path", &c->tune.solve_path}, {"solve_row", &c->tune.solve_row},
		{"solve_fuse_rows", &c->tune.solve_fuse_rows}, {"factor_path", &c->tune.factor_path}, {"factor_row", &c->tune.factor_row},
		{"factor_fuse_rows", &c->tune.factor_fuse_rows}, {"factor_serial_work", &c->tune.factor_serial_work},
		{"factor_lds_row", &c->tune.factor_lds_row}, {"color_path", &c->tune.color_path}, {"color_row", &c->tune.color_row},
		{"color_fuse_rows", &c->tune.color_fuse_rows}, {"color_wave_deg", &c->tune.color_wave_deg},
		{"agg_path", &c->tune.agg_path}, {"agg_row", &c->tune.agg_row}, {"agg_fuse_rows", &c->tune.agg_fuse_rows},
		{"agg_wave_deg", &c->tune.agg_wave_deg}, {"agg_per_rows", &c->tune.agg_per_rows},
		{"pcg_check_every", &c->tune.pcg_check_every}, {"pcg_fuse", &c->tune.pcg_fuse},
		{"gmres_path", &c->tune.gmres_path}, {"amg_path", &c->tune.amg_path}, {"amg_fuse_rows", &c->tune.amg_fuse_rows},
	};
	for (auto &t : tab) if (!std::strcmp(t.n, name)) { *t.p = (int)value; return SPSAMD_OK; }
	c->last_error = std::string("unknown tuning knob: ") + name;
	return SPSAMD_EINVAL;
}

extern "C" void spsamd_ctx_destroy(spsamd_ctx *c)
{
	if (!c) return;
	(void)hipSetDevice(c->device);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	if (c->side) (void)hipStreamSynchronize(c->side);
	if (c->side2) (void)hipStreamSynchronize(c->side2);
	c->arena.release();
	c->out[0].release(); c->out[1].release();
	c->rowstat_n.release(); c->rowstat_s.release(); c->rowstat_h.release();
	if (c->pinned) (void)hipHostFree(c->pinned);
	if (c->stream_pinned) (void)hipHostFree(c->stream_pinned);
	for (auto &e : c->ev) if (e) (void)hipEventDestroy(e);
	for (auto &e : c->ev2) if (e) (void)hipEventDestroy(e);
	for (auto &e : c->ev_side) if (e) (void)hipEventDestroy(e);
	for (auto &e : c->ev_side2) if (e) (void)hipEventDestroy(e);
	if (c->side) (void)hipStreamDestroy(c->side);
	if (c->side2) (void)hipStreamDestroy(c->side2);
	if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
	delete c;
}

extern "C" const char *spsamd_last_error(const spsamd_ctx *c) { return c ? c->last_error.c_str() : "null context"; }

extern "C" int spsamd_ctx_reserve(spsamd_ctx *c, size_t workspace_bytes, size_t output_tuples)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		SPS_HIP(hipSetDevice(c->device));
		if (workspace_bytes) c->arena.reserve(workspace_bytes);
		if (output_tuples) {
			OutSet &o = c->out[c->cur_out];
			o.i.ensure(output_tuples * sizeof(int32_t));
			o.j.ensure(output_tuples * sizeof(int32_t));
			o.v.ensure(output_tuples * sizeof(double));
		}
		return SPSAMD_OK;
	)
}

bool spsamd::same_operand(const spsamd_coo *a, const spsamd_coo *b)
{
	return a->idx0 == b->idx0 && a->idx1 == b->idx1 && a->val == b->val && a->nnz == b->nnz &&
		a->shape0 == b->shape0 && a->shape1 == b->shape1 && a->sort0 == b->sort0 && a->mem == b->mem;
}

// Shared body of the MM and MV entry points.  `what` names the right operand in
// the inner-dimension message ("B" or "V", multiply_sparse.hpp:173,299).
int spsamd::multiply_body(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res, const char *what, bool arena_ready, const OperandParts *parts, bool b_rank1)
{
	check_sink_args(duplicate_policy, sink_kind);
	std::memset(res, 0, sizeof(*res));
	const bool permute = (sink_flags & SPSAMD_SINK_PERMUTE) && sink_kind == SPSAMD_SINK_COO;
	const ProductFrame f(A, transpose_A, B, transpose_B, permute);
	const int a0 = f.a0, bk = f.bk, bj = f.bj;
	res->shape0 = f.shape0; res->shape1 = f.shape1;
	f.check_inner(what);
	if (product_is_empty(C, scalei, A, scalej, B, scalek)) return SPSAMD_OK;

	SPS_HIP(hipSetDevice(c->device));
	if (!arena_ready) c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	// (also for the digest sink: a product by column blocks, spgemm_column_blocks, goes through the COO buffers)
	{ const spsamd_coo *ops[2] = {A, B}; pick_output_set(c, ops, 2); }
	MultiplyArgs a;
	a.C = C; a.sink_kind = sink_kind; a.sink_flags = sink_flags;
	if (parts) { a.pa = parts->pa; a.pb = parts->pb; a.b_ready = parts->b_ready; a.static_walk = true; }
	Prepared *hp = nullptr;
	consolidate_operand(c, A, a0, a0, duplicate_policy, zero_nan, &a.A, &hp);      // :187
	if (hp) a.pa = hp;
	// A*A: one consolidation serves both -- except under zero_nan, where the NaNs dropped from B are those
	// of the leading run of the reference's column-major sequence (:168), not of A's row-major one
	// (a prepared operand is taken as it was prepared, like any operand that carries the wanted sort order)
	if (a0 == bk && same_operand(A, B) && (!zero_nan || hp)) { a.B = a.A; if (a.pa) a.pb = a.pa; }
	// (MV's V: Consolidate<VecT>(&V, {0}), :313 -- the reference's order is V's own, so a V that carries it is taken as stored)
	else { consolidate_operand(c, B, bk, b_rank1 ? bk : bj, duplicate_policy, zero_nan, &a.B, &hp); if (hp) a.pb = hp; }  // :188
	if (sink_kind == SPSAMD_SINK_COO) c->own[c->cur_out].sort0 = -1;           // that set is about to be overwritten
	upload_scale(c, scalei, f.nrow, "scalei", &a.si);
	upload_scale(c, scalej, f.inner, "scalej", &a.sj);
	upload_scale(c, scalek, f.ncol, "scalek", &a.sk);
	spgemm(c, a, res);
	// (spgemm grew the output set itself and stored there; no tuples: nothing to hand over, and nothing to swap)
	if (sink_kind == SPSAMD_SINK_COO && res->idx0 && res->idx1) publish_coo(c, res, res->idx0, res->idx1, res->val, res->nnz, permute);
	finish_call(c, res);
	if (res->nnz_a && res->nnz_b) {
		SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	}
	return SPSAMD_OK;
}

extern "C" int spsamd_multiply(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !B || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		return multiply_body(c, C, scalei, A, transpose_A, scalej, B, transpose_B, scalek, duplicate_policy, zero_nan,
			sink_kind, sink_flags, res, "B", false);
	)
}

// The product delivered in row blocks while it is computed (k_stream.hip)
extern "C" int spsamd_multiply_stream(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_flags, size_t block_tuples, spsamd_chunk_fn cb, void *user,
	spsamd_result *res, spsamd_stream_stats *stats)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !B || !res || !cb) throw Error{SPSAMD_EINVAL, "null operand, callback or result"};
		struct Busy { spsamd_ctx *c; Busy(spsamd_ctx *x) : c(x) { c->busy = true; } ~Busy() { c->busy = false; } } busy{c};
		return multiply_stream(c, C, scalei, A, transpose_A, scalej, B, transpose_B, scalek, duplicate_policy, zero_nan,
			sink_flags, block_tuples, cb, user, res, stats);
	)
}

// C = alpha * op(A) + beta * op(B): consolidate() of the concatenated, scaled tuples (k_add.hip)
extern "C" int spsamd_add(spsamd_ctx *c, double alpha, const spsamd_coo *A, char transpose_A,
	double beta, const spsamd_coo *B, char transpose_B, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !B || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		add_matrices(c, alpha, A, transpose_A, beta, B, transpose_B, duplicate_policy, zero_nan, sink_kind, sink_flags, res);
		return SPSAMD_OK;
	)
}

// op(A) * op(B) on the pattern of M: the reference's inner-product loop run over M's keys only (k_masked.hip)
extern "C" int spsamd_multiply_masked(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, const spsamd_coo *M,
	int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !B || !M || !res) throw Error{SPSAMD_EINVAL, "null operand, mask or result"};
		multiply_masked(c, C, scalei, A, transpose_A, scalej, B, transpose_B, scalek, M, duplicate_policy, zero_nan,
			sink_kind, sink_flags, res);
		return SPSAMD_OK;
	)
}

// Matrix x sparse vector (multiply_sparse.hpp:281-365): V is the one-column
// matrix (idx, 0) of shape (V.shape0, 1); consolidating it row-major is
// Consolidate<VecT>(&V, {0}) (:313).  The result's idx1 is all zero.
extern "C" int spsamd_multiply_mv(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_vec *V,
	int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !V || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		spsamd_coo Vm;
		Vm.nnz = V->nnz; Vm.shape0 = V->shape0; Vm.shape1 = 1;
		Vm.sort0 = V->sort0 == 0 ? 0 : -1;
		Vm.mem = SPSAMD_MEM_DEVICE;
		Vm.idx0 = nullptr; Vm.idx1 = nullptr; Vm.val = nullptr;
		if (V->nnz) {
			if (!V->idx || !V->val) throw Error{SPSAMD_EINVAL, "vector with nnz > 0 has a null array"};
			int32_t *vi = c->arena.get<int32_t>(V->nnz), *vz = c->arena.get<int32_t>(V->nnz);
			double *vv = c->arena.get<double>(V->nnz);
			hipMemcpyKind kind = V->mem == SPSAMD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
			SPS_HIP(hipMemcpyAsync(vi, V->idx, V->nnz * sizeof(int32_t), kind, c->stream));
			SPS_HIP(hipMemcpyAsync(vv, V->val, V->nnz * sizeof(double), kind, c->stream));
			fill_zero(c, vz, V->nnz * sizeof(int32_t));
			Vm.idx0 = vi; Vm.idx1 = vz; Vm.val = vv;
		}
		int rc = multiply_body(c, C, scalei, A, transpose_A, scalej, &Vm, '.', nullptr, duplicate_policy, zero_nan,
			sink_kind, sink_flags & ~SPSAMD_SINK_PERMUTE, res, "V", true, nullptr, true);     // a rank-1 result has nothing to permute
		res->shape1 = 0;                              // rank-1 result: ret.set_shape({rows}) (:295)
		res->idx1 = nullptr;                          // ... with one index array: nothing to copy for a second one
		return rc;
	)
}

// ---- prepared operands -------------------------------------------------------------------------------------
// The reference keeps what it derives from an operand: an array that carries the wanted sort_order is not consolidated
// again (Consolidate<>, algorithm.hpp:360) and its row structure is computed once and cached in the object
// (VectorCooArray::dim_beginnings, VectorCooArray.hpp:325-335).  spsamd_operand is that object on the device.

struct spsamd_operand {
	spsamd::Prepared p;
	uint64_t shape0 = 0, shape1 = 0;
};

extern "C" int spsamd_operand_prepare(spsamd_ctx *c, const spsamd_coo *X, char transpose, int role, int duplicate_policy, int zero_nan,
	spsamd_operand **out)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!X || !out) throw Error{SPSAMD_EINVAL, "null operand or result"};
		*out = nullptr;
		if (role != SPSAMD_AS_A && role != SPSAMD_AS_B && role != (SPSAMD_AS_A | SPSAMD_AS_B)) throw Error{SPSAMD_EINVAL, "bad role"};
		if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
		if (X->mem == SPSAMD_MEM_PREPARED) throw Error{SPSAMD_EINVAL, "the operand is a prepared one already"};
		if (zero_nan && role == (SPSAMD_AS_A | SPSAMD_AS_B))
			throw Error{SPSAMD_EINVAL, "under zero_nan the two sides of a product drop different NaNs (multiply_sparse.hpp:167-168): prepare one operand per side"};
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		// the leading dimension multiply consolidates this side by, and the one the REFERENCE's own sequence leads with
		// (they differ for B: multiply_sparse.hpp:168)
		const int lead = transpose == 'T' ? 1 : 0;
		const int ref_lead = (role & SPSAMD_AS_A) ? lead : 1 - lead;
		ConMat m;
		consolidate_operand(c, X, lead, ref_lead, duplicate_policy, zero_nan, &m);
		spsamd_operand *h = new spsamd_operand();
		struct Guard { spsamd_operand *h; ~Guard() { if (h) { h->p.release(); delete h; } } } guard{h};
		h->shape0 = X->shape0; h->shape1 = X->shape1;
		Prepared &p = h->p;
		p.ctx = c; p.owns = true; p.lead = lead;
		p.m = m;
		const size_t n = m.nnz;
		// All of the handle's memory is taken NOW, in one piece: tuples, packed tuples, row list, row pointer -- and, for a right
		// operand with long rows, the column-window indices the first product with a heavy row will build.  (Measured on cfg2:
		// taken later and separately, after the context's workspace exists, the same arrays make the kernels that gather from
		// them at random -- the hash cells of the long rows -- 2.3x slower; presumably the fragments the driver then finds are
		// smaller.)  Not for operands whose indices would be out of proportion: a stencil matrix has no heavy rows and
		// millions of columns.
		size_t want = (n + 64) * (16 + 12 + 8) + (m.nrow + 66) * 4 + 65536;
		uint32_t maxlen = 0;
		if (n) {
			Prepared view;                                              // (the consolidated tuples still sit in the workspace)
			view.ctx = c; view.m = m;
			prepared_row_structure(c, &view);
			maxlen = view.maxlen;
		}
		if ((role & SPSAMD_AS_B) && maxlen > 64) {
			const uint64_t W = m.ncol > (uint64_t(1) << 21) ? 16384 : 8192, nwin = (m.ncol + W - 1) / W, nwp = (nwin + 7) & ~7ull, nrowb = m.nrow + 1;
			const uint64_t nbw = (((nwin + 31) >> 5) + 3) & ~3ull;        // (the window-occupancy words, heavy_b_index)
			const uint64_t idx = nrowb * (nwin + 1) * 4 + nrowb * nwp * 2 + nrowb * nbw * 4 + (nrowb * nwin + 1) * 4 + (n + 8) * 12 + 8192;
			size_t freeb = 0, totalb = 0;
			if (idx <= 64 * (uint64_t)n * 16 && hipMemGetInfo(&freeb, &totalb) == hipSuccess && idx + want < freeb / 2) want += idx;
		}
		p.reserve(want);
		p.m.row = p.get<int32_t>(n ? n : 1); p.m.col = p.get<int32_t>(n ? n : 1); p.m.val = p.get<double>(n ? n : 1);
		if (n) {
			SPS_HIP(hipMemcpyAsync(p.m.row, m.row, n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
			SPS_HIP(hipMemcpyAsync(p.m.col, m.col, n * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
			SPS_HIP(hipMemcpyAsync(p.m.val, m.val, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
		}
		prepared_row_structure(c, &p);                                  // the row pointer and the longest row (every product asks for them)
		SPS_HIP(hipStreamSynchronize(c->stream));
		guard.h = nullptr;
		*out = h;
		return SPSAMD_OK;
	)
}

extern "C" int spsamd_operand_as_coo(const spsamd_operand *h, spsamd_coo *out)
{
	if (!h || !out) return SPSAMD_EINVAL;
	out->idx0 = (const int32_t *)h; out->idx1 = nullptr; out->val = nullptr;
	out->nnz = h->p.m.nnz; out->shape0 = h->shape0; out->shape1 = h->shape1;
	out->sort0 = h->p.lead; out->mem = SPSAMD_MEM_PREPARED;
	return SPSAMD_OK;
}

extern "C" uint64_t spsamd_operand_bytes(const spsamd_operand *h) { return h ? h->p.owned_bytes : 0; }

extern "C" void spsamd_operand_destroy(spsamd_operand *h)
{
	if (!h) return;
	if (h->p.ctx) { (void)hipSetDevice(h->p.ctx->device); (void)hipStreamSynchronize(h->p.ctx->stream); if (h->p.ctx->side) (void)hipStreamSynchronize(h->p.ctx->side); }
	h->p.release();
	delete h;
}

extern "C" int spsamd_result_fetch(spsamd_ctx *c, const spsamd_result *res, spsamd_chunk_fn cb, void *user)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!res || !cb) throw Error{SPSAMD_EINVAL, "null result or callback"};
		if (res->nnz == 0) return SPSAMD_OK;
		if (!res->idx0 || !res->val) throw Error{SPSAMD_EINVAL, "result has no COO tuples (DIGEST sink?)"};
		SPS_HIP(hipSetDevice(c->device));
		// chunks of 2^20 tuples through two pinned staging buffers: the copy of chunk k+1 runs while the
		// callback consumes chunk k (the callback, one ret.add() per tuple upstream, is the slow side)
		const size_t chunk = size_t(1) << 20;
		char *h = (char *)c->host_staging(2 * chunk * 16);
		hipEvent_t ev[2] = {c->ev[EV_FETCH0], c->ev[EV_FETCH1]};
		auto issue = [&](uint64_t o, int b) {
			size_t n = (size_t)std::min<uint64_t>(chunk, res->nnz - o);
			char *hb = h + (size_t)b * chunk * 16;
			SPS_HIP(hipMemcpyAsync(hb, res->idx0 + o, n * 4, hipMemcpyDeviceToHost, c->stream));
			if (res->idx1) SPS_HIP(hipMemcpyAsync(hb + chunk * 4, res->idx1 + o, n * 4, hipMemcpyDeviceToHost, c->stream));
			SPS_HIP(hipMemcpyAsync(hb + chunk * 8, res->val + o, n * 8, hipMemcpyDeviceToHost, c->stream));
			SPS_HIP(hipEventRecord(ev[b], c->stream));
		};
		issue(0, 0);
		int b = 0;
		for (uint64_t o = 0; o < res->nnz; o += chunk, b ^= 1) {
			size_t n = (size_t)std::min<uint64_t>(chunk, res->nnz - o);
			if (o + chunk < res->nnz) issue(o + chunk, b ^ 1);
			SPS_HIP(hipEventSynchronize(ev[b]));
			char *hb = h + (size_t)b * chunk * 16;
			int rc = cb(user, (int32_t *)hb, res->idx1 ? (int32_t *)(hb + chunk * 4) : nullptr, (double *)(hb + chunk * 8), n);
			if (rc) { SPS_HIP(hipStreamSynchronize(c->stream)); return rc; }
		}
		return SPSAMD_OK;
	)
}

__global__ void k_scatter_dense(const int32_t *i, const int32_t *j, const double *v, uint64_t n, double *dense, size_t ld, int policy)
{
	uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (; t < n; t += stride) {
		double *p = dense + (size_t)i[t] * ld + (size_t)j[t];      // (i, j) is unique inside one result
		if (policy == SPSAMD_ADD) *p += v[t];
		else if (policy == SPSAMD_REPLACE) *p = v[t];
		else if (!(*p != *p)) *p = v[t];                          // LEAVE_ALONE exactly as accum.hpp:128-130 spells it: `if (!std::isnan(oval)) oval = val`
	}
}

extern "C" int spsamd_result_scatter_dense(spsamd_ctx *c, const spsamd_result *res, double *dense, size_t ld, int policy)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!res || (res->nnz && (!dense || !res->idx0 || !res->idx1 || !res->val))) throw Error{SPSAMD_EINVAL, "null result, matrix or no COO tuples"};
		if (policy < 0 || policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
		if (ld < res->shape1) throw Error{SPSAMD_EINVAL, "leading dimension smaller than the result's column count"};
		if (res->nnz == 0) return SPSAMD_OK;
		SPS_HIP(hipSetDevice(c->device));
		unsigned grid = (unsigned)std::min<uint64_t>((res->nnz + 255) / 256, 8192);
		k_scatter_dense<<<dim3(grid), dim3(256), 0, c->stream>>>(res->idx0, res->idx1, res->val, res->nnz, dense, ld, policy);
		SPS_LAUNCH_CHECK();
		SPS_HIP(hipStreamSynchronize(c->stream));
		return SPSAMD_OK;
	)
}

// Y (op)= op(M) * X (multiply_dense.hpp:11-35; y a DenseAccum, accum.hpp:110-140).  Workspace only: neither output set of
// the context is written, so a SINK_COO result stays fetchable and may itself be M.
extern "C" int spsamd_multiply_dense(spsamd_ctx *c, const spsamd_coo *M, char transpose, const double *X, size_t ldx,
	double *Y, size_t ldy, size_t nrhs, int mem, int policy, int handle_nan)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!M) throw Error{SPSAMD_EINVAL, "null matrix"};
		const int lead = transpose == 'T' ? 1 : 0;
		const uint64_t shape[2] = {M->shape0, M->shape1};
		const uint64_t nrow = shape[lead], ncol = shape[1 - lead];      // rows(op(M)) = rows of Y, cols(op(M)) = rows of X
		if (nrhs && (nrow || ncol) && (!X || !Y)) throw Error{SPSAMD_EINVAL, "null X or Y"};
		if (ldx < nrhs || ldy < nrhs) throw Error{SPSAMD_EINVAL, "leading dimension of X or Y smaller than nrhs"};
		if (policy < 0 || policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
		if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of X and Y must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
		if (nrhs > 0xFFFFFFFFull) throw Error{SPSAMD_EINVAL, "nrhs exceeds 2^32 - 1"};
		// the bytes each array spans: rows - 1 full leading dimensions and nrhs values
		const uint64_t xbytes = ncol && nrhs ? ((ncol - 1) * ldx + nrhs) * sizeof(double) : 0;
		const uint64_t ybytes = nrow && nrhs ? ((nrow - 1) * ldy + nrhs) * sizeof(double) : 0;
		if (xbytes && ybytes && (const char *)X < (const char *)Y + ybytes && (const char *)Y < (const char *)X + xbytes)
			throw Error{SPSAMD_EINVAL, "X and Y overlap"};
		// (the unchecked count: a null prepared handle is an empty M here, as it always was; dense_operand checks the handle)
		if (!nrhs || operand_tuples(M) == 0) return SPSAMD_OK;
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		DenseOperand m;
		dense_operand(c, M, lead, &m);
		if (!m.nnz) return SPSAMD_OK;
		const double *dX = X;
		double *dY = Y;
		uint64_t dldx = ldx, dldy = ldy;
		if (mem == SPSAMD_MEM_HOST) {                                  // packed device copies, nrhs values per row
			double *tx = c->arena.get<double>(ncol * nrhs), *ty = c->arena.get<double>(nrow * nrhs);
			SPS_HIP(hipMemcpy2DAsync(tx, nrhs * sizeof(double), X, ldx * sizeof(double), nrhs * sizeof(double), ncol, hipMemcpyHostToDevice, c->stream));
			SPS_HIP(hipMemcpy2DAsync(ty, nrhs * sizeof(double), Y, ldy * sizeof(double), nrhs * sizeof(double), nrow, hipMemcpyHostToDevice, c->stream));
			dX = tx; dY = ty; dldx = dldy = nrhs;
		}
		spmm_dense(c, m, dX, dldx, dY, dldy, (uint32_t)nrhs, policy, handle_nan != 0);
		if (mem == SPSAMD_MEM_HOST)
			SPS_HIP(hipMemcpy2DAsync(Y, ldy * sizeof(double), dY, nrhs * sizeof(double), nrhs * sizeof(double), nrow, hipMemcpyDeviceToHost, c->stream));
		SPS_HIP(hipStreamSynchronize(c->stream));
		return SPSAMD_OK;
	)
}

// out[t] = alpha * (P_i . Q_j) (+ beta * v) over op(M)'s tuples in storage order (k_sampled.hip).  Workspace only, like
// multiply_dense: neither output set is written, so a SINK_COO result stays fetchable and may itself be M.
extern "C" int spsamd_multiply_sampled(spsamd_ctx *c, const spsamd_coo *M, char transpose, const double *P, size_t ldp,
	const double *Q, size_t ldq, size_t k, double alpha, double beta, double *out, int mem)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		multiply_sampled(c, M, transpose, P, ldp, Q, ldq, k, alpha, beta, out, mem);
		return SPSAMD_OK;
	)
}

// The tuples of op(A) that a predicate keeps, in op(A)'s order, values untouched (k_select.hip)
extern "C" int spsamd_select(spsamd_ctx *c, const spsamd_coo *A, char transpose, int predicate, int64_t iparam, double dparam,
	int select_flags, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		select_tuples(c, A, transpose, predicate, iparam, dparam, select_flags, duplicate_policy, zero_nan, sink_kind, sink_flags, res);
		return SPSAMD_OK;
	)
}

// The submatrix op(A)(I, J) by row and column lists, values untouched (k_extract.hip)
extern "C" int spsamd_extract(spsamd_ctx *c, const spsamd_coo *A, char transpose, const int32_t *rows, size_t nrows,
	const int32_t *cols, size_t ncols, int index_mem, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags,
	spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		extract_tuples(c, A, transpose, rows, nrows, cols, ncols, index_mem, duplicate_policy, zero_nan, sink_kind, sink_flags, res);
		return SPSAMD_OK;
	)
}

// post(fold over each row of op(A)) as a sparse or dense vector in the caller's buffers (k_reduce.hip).  Workspace only, like
// multiply_dense: neither output set is written, so a SINK_COO result stays fetchable and may itself be A.
extern "C" int spsamd_reduce(spsamd_ctx *c, const spsamd_coo *A, char transpose, int op, int post, int duplicate_policy, int zero_nan,
	int32_t *out_idx, double *out_val, size_t capacity, int mem, size_t *out_nnz, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !out_val || !out_nnz) throw Error{SPSAMD_EINVAL, "null operand, out_val or out_nnz"};
		spsamd_result local;
		return reduce_rows(c, A, transpose, op, post, duplicate_policy, zero_nan, out_idx, out_val, capacity, mem, out_nnz,
			res ? res : &local);
	)
}

// op(A) o op(B) over the intersection of the two patterns, op(A) on or off op(B)'s pattern (k_emult.hip)
extern "C" int spsamd_emult(spsamd_ctx *c, int op, int emult_flags, double alpha, const spsamd_coo *A, char transpose_A,
	const spsamd_coo *B, char transpose_B, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !B || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		emult_matrices(c, op, emult_flags, alpha, A, transpose_A, B, transpose_B, duplicate_policy, zero_nan, sink_kind, sink_flags, res);
		return SPSAMD_OK;
	)
}

// T * X = B for a triangle of op(A), by level schedule (k_solve.hip).  Workspace only, like multiply_dense: neither output
// set is written, so a SINK_COO result stays fetchable and may itself be A.
extern "C" int spsamd_solve_tri(spsamd_ctx *c, const spsamd_coo *A, char transpose, int uplo, int diag, const double *B, size_t ldb,
	double *X, size_t ldx, size_t nrhs, int mem, int duplicate_policy, int zero_nan, spsamd_solve_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A) throw Error{SPSAMD_EINVAL, "null operand"};
		spsamd_result local;
		return solve_tri(c, A, transpose, uplo, diag, B, ldb, X, ldx, nrhs, mem, duplicate_policy, zero_nan, stats, res ? res : &local);
	)
}

// F = ILU(0) of op(A) on its own pattern, by the LOWER triangle's level schedule (k_factor.hip)
extern "C" int spsamd_factor_ilu0(spsamd_ctx *c, const spsamd_coo *A, char transpose, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_factor_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !res) throw Error{SPSAMD_EINVAL, "null operand or result"};
		factor_ilu0(c, A, transpose, duplicate_policy, zero_nan, sink_kind, sink_flags, stats, res);
		return SPSAMD_OK;
	)
}

// A greedy multi-colour ordering of op(A)'s graph (k_color.hip).  Workspace only, like spsamd_reduce: neither output set is
// written, so a SINK_COO result stays fetchable and may itself be A.
extern "C" int spsamd_color(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int color_flags,
	int32_t *color, int32_t *perm, int32_t *color_ptr, size_t ptr_capacity, int mem, size_t *out_ncolors,
	spsamd_color_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !color || !out_ncolors) throw Error{SPSAMD_EINVAL, "null operand, color or out_ncolors"};
		spsamd_result local;
		return color_graph(c, A, transpose, order, seed, color_flags, color, perm, color_ptr, ptr_capacity, mem, out_ncolors,
			stats, res ? res : &local);
	)
}

// The MIS(2) aggregates of op(A)'s graph (k_aggregate.hip).  Workspace only, like spsamd_color.
extern "C" int spsamd_aggregate(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int agg_flags,
	int32_t *agg, int32_t *members, int32_t *agg_ptr, size_t ptr_capacity, int mem, size_t *out_naggregates,
	spsamd_aggregate_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !agg || !out_naggregates) throw Error{SPSAMD_EINVAL, "null operand, agg or out_naggregates"};
		spsamd_result local;
		return aggregate_graph(c, A, transpose, order, seed, agg_flags, agg, members, agg_ptr, ptr_capacity, mem, out_naggregates,
			stats, res ? res : &local);
	)
}

// op(A) x = b by preconditioned conjugate gradients, the loop on the device (k_krylov.hip).  Workspace only, like
// spsamd_solve_tri: neither output set is written, so A and M may be the SINK_COO results of the two sets.
extern "C" int spsamd_solve_pcg(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A) throw Error{SPSAMD_EINVAL, "null operand"};
		spsamd_result local;
		return solve_pcg(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity,
			duplicate_policy, zero_nan, stats, res ? res : &local);
	)
}

// op(A) x = b by right-preconditioned BiCGStab, the loop on the device (k_bicgstab.hip).  Workspace only, like
// spsamd_solve_pcg.
extern "C" int spsamd_solve_bicgstab(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A) throw Error{SPSAMD_EINVAL, "null operand"};
		spsamd_result local;
		return solve_bicgstab(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, hist_host, hist_capacity,
			duplicate_policy, zero_nan, stats, res ? res : &local);
	)
}

// op(A) x = b by right-preconditioned restarted GMRES(restart), the loop on the device (k_gmres.hip).  Workspace only, like
// spsamd_solve_pcg.
extern "C" int spsamd_solve_gmres(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, uint32_t restart, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A) throw Error{SPSAMD_EINVAL, "null operand"};
		spsamd_result local;
		return solve_gmres(c, A, transpose, precond, M, transpose_M, b, x, mem, tol, max_iter, restart, hist_host, hist_capacity,
			duplicate_policy, zero_nan, stats, res ? res : &local);
	)
}

// x = cycle(0, b): one multigrid cycle over the caller's levels (k_amg.hip).  Workspace only.
extern "C" int spsamd_amg_apply(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params,
	const double *b, double *x, int mem, int duplicate_policy, int zero_nan, spsamd_amg_stats *stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		spsamd_result local;
		return amg_apply(c, levels, nlevels, params, b, x, mem, duplicate_policy, zero_nan, stats, res ? res : &local);
	)
}

// levels[0].A x = b by the loop of spsamd_solve_pcg with z = cycle(0, r) (k_krylov.hip, k_amg.hip).  Workspace only.
extern "C" int spsamd_solve_pcg_amg(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_amg_stats *amg_stats, spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		spsamd_result local;
		return solve_pcg_amg(c, levels, nlevels, params, b, x, mem, tol, max_iter, hist_host, hist_capacity, duplicate_policy,
			zero_nan, stats, amg_stats, res ? res : &local);
	)
}

extern "C" int spsamd_memcpy(spsamd_ctx *c, void *dst, const void *src, size_t bytes)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (bytes && (!dst || !src)) throw Error{SPSAMD_EINVAL, "null pointer"};
		SPS_HIP(hipSetDevice(c->device));
		SPS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, c->stream));
		SPS_HIP(hipStreamSynchronize(c->stream));
		return SPSAMD_OK;
	)
}

extern "C" int spsamd_consolidate(spsamd_ctx *c, const spsamd_coo *A, int so0, int duplicate_policy, int zero_nan,
	spsamd_result *res)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !res || (so0 != 0 && so0 != 1)) throw Error{SPSAMD_EINVAL, "bad argument"};
		if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
		// (the stand-alone algorithms read an operand's arrays themselves: a prepared one as the device COO it holds)
		const OperandView view = operand_view(c, A);
		A = &view.coo;
		std::memset(res, 0, sizeof(*res));
		res->shape0 = A->shape0; res->shape1 = A->shape1;
		if (A->nnz == 0) return SPSAMD_OK;
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		spsamd_coo X = *A;
		X.sort0 = -1;                         // the stand-alone algorithm always runs (algorithm.hpp:251)
		ConMat m;
		consolidate_operand(c, &X, so0, so0, duplicate_policy, zero_nan, &m);
		size_t n = m.nnz;
		const spsamd_coo *ops[1] = {A};
		pick_output_set(c, ops, 1);
		const CooOut o = coo_output(c, n);
		SPS_HIP(hipMemcpyAsync(o.row, m.row, n * 4, hipMemcpyDeviceToDevice, c->stream));
		SPS_HIP(hipMemcpyAsync(o.col, m.col, n * 4, hipMemcpyDeviceToDevice, c->stream));
		SPS_HIP(hipMemcpyAsync(o.val, m.val, n * 8, hipMemcpyDeviceToDevice, c->stream));
		SPS_HIP(hipStreamSynchronize(c->stream));
		res->nnz_a = n;
		// m.row is the leading (sorted) dimension: so0 == 1 is the permuted reading, which puts the dimensions back in place
		publish_coo(c, res, o.row, o.col, o.val, n, so0 == 1);
		return SPSAMD_OK;
	)
}

extern "C" int spsamd_sorted_permutation(spsamd_ctx *c, const spsamd_coo *A, int so0, uint64_t *perm_host)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || (so0 != 0 && so0 != 1) || (A->nnz && !perm_host)) throw Error{SPSAMD_EINVAL, "bad argument"};
		if (A->nnz == 0) return SPSAMD_OK;
		const OperandView view = operand_view(c, A);
		A = &view.coo;
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		uint32_t *perm = sorted_permutation(c, A, so0);
		std::vector<uint32_t> h(A->nnz);
		SPS_HIP(hipMemcpyAsync(h.data(), perm, A->nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		SPS_HIP(hipStreamSynchronize(c->stream));
		for (size_t i = 0; i < A->nnz; ++i) perm_host[i] = h[i];
		return SPSAMD_OK;
	)
}

extern "C" int spsamd_dim_beginnings(spsamd_ctx *c, const spsamd_coo *A, int so0, uint64_t *beg_host, size_t *count)
{
	if (!c) return SPSAMD_EINVAL;
	API_GUARD(c,
		if (!A || !count || (so0 != 0 && so0 != 1)) throw Error{SPSAMD_EINVAL, "bad argument"};
		const OperandView view = operand_view(c, A);
		A = &view.coo;
		if (A->sort0 != so0) throw Error{SPSAMD_EINVAL, "dim_beginnings() required the VectorCooArray is sorted first."};
		*count = 0;
		if (A->nnz == 0) return SPSAMD_OK;                         // algorithm.hpp:89
		if (!beg_host) throw Error{SPSAMD_EINVAL, "null output"};
		SPS_HIP(hipSetDevice(c->device));
		c->arena.reset();
		ConMat m;
		consolidate_operand(c, A, so0, so0, SPSAMD_ADD, 0, &m);         // trusted as is (sort0 == so0): upload only
		RowList rl;
		dim_beginnings(c, m, &rl);
		std::vector<uint32_t> h((size_t)rl.nrows + 1);
		SPS_HIP(hipMemcpyAsync(h.data(), rl.beg, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
		SPS_HIP(hipStreamSynchronize(c->stream));
		for (size_t i = 0; i < h.size(); ++i) beg_host[i] = h[i];
		*count = h.size();
		return SPSAMD_OK;
	)
}
