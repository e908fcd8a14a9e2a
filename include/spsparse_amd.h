/*
 * spsparse_amd.h -- C ABI of the MI355X SpGEMM behind spsparse::multiply().
 *
 * This is the drop-in boundary.  The reference has no FFI today: its boundary
 * is the header-only template spsparse::multiply()
 * (slib/spsparse/multiply_sparse.hpp:138-164).  include/spsparse_amd/multiply.hpp
 * is that template re-stated on top of the entry points below; INTEGRATION.md
 * shows the lines a spsparse maintainer would add to bind them.
 *
 * Conventions
 *   - plain pointers and sizes, no C++ or torch types; never throws.
 *   - every entry point returns 0 or a negative SPSAMD_E* code; the text of the
 *     last error of a context is at spsamd_last_error().  The C++ shim forwards
 *     it to (*spsparse_error)(-1, "%s", msg) (spsparse.hpp:47,54).
 *   - indices int32, values double: the only instantiation the reference tests
 *     (tests/test_multiply_sparse.cpp:90-91).  Counts and offsets are 64 bit:
 *     nnz(C) exceeds 2^31 on BASELINE cfg2.
 *   - operands are borrowed for the duration of a call and never modified
 *     (multiply_sparse.hpp:143,146 take const&).
 *   - one context = one device + one HIP stream + one workspace; calls on
 *     different contexts may run concurrently from different host threads.
 *   - there is no CPU fallback: every compute entry point needs the GPU.
 *
 * Limits (each is an SPSAMD_EINVAL / SPSAMD_ENOMEM with a message, never a wrong result)
 *   - indices int32, fewer than 2^31 tuples per operand (like the reference's int positions,
 *     algorithm.hpp:419); one output row may hold at most 2^32-1 scalar products.
 *   - rows with more than 4096 scalar products ("heavy" rows) are cut along column windows of 8192
 *     columns (16384 above 2^21 columns), at most 2048 of them.  A product with a heavy row and more than
 *     2^25 columns in op(B) is multiplied by column blocks of op(B), 2^25 columns at a time (same result,
 *     slower: every block repeats the work on A and a COO result is assembled by one more pass).
 *   - the heavy-row path keeps dense indices of rows(op(B)) x windows entries in the workspace (10 bytes per
 *     row and window: 1.4 GB for a 2^20-square matrix, 43 GB at 2^23).  Where they would not fit the device the
 *     product also goes by column blocks, narrow enough for them to fit; SPSAMD_ENOMEM only if one window's
 *     share does not.
 *
 * Applying a matrix to dense vectors
 *   spsamd_multiply_dense is the reference's multiply(M, x, y, handle_nan, transpose) (multiply_dense.hpp:11-35, compiled
 *   out there) into a DenseAccum (accum.hpp:110-140), for nrhs right-hand sides at once.  Every entry of Y is
 *   bit-identical to the reference's loop over M's tuples in storage order (duplicates and explicit zeros included).
 */
#ifndef SPSPARSE_AMD_H
#define SPSPARSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define SPSAMD_OK            0
#define SPSAMD_EDIM        (-1)   /* inner dimensions differ (multiply_sparse.hpp:172-174) */
#define SPSAMD_EINVAL      (-2)   /* bad argument (null pointer, index out of bounds, unsorted scale vector ...) */
#define SPSAMD_EHIP        (-3)   /* HIP runtime error (message carries hipGetErrorString) */
#define SPSAMD_ENOMEM      (-4)   /* device or host allocation failed */
#define SPSAMD_ECAPACITY   (-5)   /* caller-supplied output buffer too small */
#define SPSAMD_ENODEVICE   (-6)   /* no usable gfx950 device */
#define SPSAMD_EPEER       (-7)   /* multi-GPU step: another rank of the communicator reported an error (nothing was multiplied) */

/* spsparse::DuplicatePolicy (spsparse.hpp:25-26), same enumerator order */
#define SPSAMD_LEAVE_ALONE 0
#define SPSAMD_ADD         1
#define SPSAMD_REPLACE     2

/* where the pointers of an operand live */
#define SPSAMD_MEM_HOST    0
#define SPSAMD_MEM_DEVICE  1

typedef struct spsamd_ctx spsamd_ctx;

/*
 * A COO matrix as VectorCooArray<int,double,2> stores it
 * (VectorCooArray.hpp:17,22-23,35): one index vector per dimension, one value
 * vector, shape, and sort_order[0] (-1 = unsorted / edit mode, 0 = consolidated
 * row major {0,1}, 1 = consolidated column major {1,0}).  A matching
 * sort order is trusted like Consolidate<> does (algorithm.hpp:360).
 */
typedef struct {
	const int32_t *idx0;
	const int32_t *idx1;
	const double *val;
	size_t nnz;
	size_t shape0, shape1;
	int sort0;
	int mem;             /* SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE */
} spsamd_coo;

/*
 * A sparse vector (VectorCooArray<int,double,1>): the three diagonal scale
 * operands and the right-hand side of the matrix-vector multiply.  Scale
 * vectors must be strictly ascending in idx: the reference joins them as
 * stored and silently mis-computes otherwise (multiply_sparse.hpp:83-85,
 * 223-226) -- this library rejects them (SPSAMD_EINVAL).
 */
typedef struct {
	const int32_t *idx;
	const double *val;
	size_t nnz;
	size_t shape0;
	int sort0;           /* only read for the MV right-hand side */
	int mem;
} spsamd_vec;

/* ---- sinks: the device side of the Accumulator concept (accum.hpp:12-24) ---- */

#define SPSAMD_SINK_COO       1   /* row-major sorted (i, j, v) tuples in device memory */
#define SPSAMD_SINK_DIGEST    2   /* count + sum + index hash only (ScalarAccumulator analogue, accum.hpp:158-167) */

/* sink flags */
#define SPSAMD_SINK_ROWSTATS  1   /* DIGEST: also fill row_nnz / row_sum / row_hash (length = rows of op(A)) */
#define SPSAMD_SINK_PERMUTE   4   /* COO, matrix result: emit (j, i, v) -- idx0 holds the column, idx1 the row, shape
                                   * swapped (PermuteAccum with perm {1,0}, accum.hpp:73-101; the tuples stay in
                                   * the order of C's rows, i.e. column-major for the permuted array) */
#define SPSAMD_SINK_EXACT_PATTERN 8 /* the reference's INDEX SET at arrival-order speed: a sum that could be exactly
                                   * zero in the reference's ascending-k order but not in arrival order (or the reverse) --
                                   * |sum| within the rounding bound of its cell -- is re-evaluated in ascending k and that
                                   * value decides (multiply_sparse.hpp:238) and is emitted; all other values stay within
                                   * rounding (1e-12 relative) of the reference's */
#define SPSAMD_SINK_ORDERED   2   /* every sum accumulated in ascending k like the reference's loop
                                   * (multiply_sparse.hpp:219-236): bit-identical values and zero drops on
                                   * any input, several times slower on rows with more than 64 products */

/*
 * Result of one multiply.  For SINK_COO the three arrays live in one of the
 * context's two output buffers (device memory) and stay valid until the next
 * SINK_COO multiply / consolidate or spsamd_ctx_destroy on that context;
 * tuples are in ascending (i, j), each (i, j) at most once, exact zeros dropped
 * (multiply_sparse.hpp:238).
 * Chaining: the arrays may be handed straight back as a SPSAMD_MEM_DEVICE,
 * sort0 = 0 operand of the NEXT call on the same context (T = R*A, then
 * C = T*R^T): that call reads them in place and writes its own result to the
 * other buffer, so no copy and no re-consolidation of T takes place; T stays
 * valid until the call after that.
 */
typedef struct {
	uint64_t shape0, shape1;      /* ret.set_shape(), multiply_sparse.hpp:169 */
	uint64_t nnz;                 /* tuples emitted */
	uint64_t products;            /* P = sum over A tuples of the B row length */
	uint64_t nnz_a, nnz_b;        /* consolidated operand sizes */
	double sum;                   /* DIGEST: sum of emitted values */
	uint64_t hash;                /* DIGEST: sum of mix64(i, j) mod 2^64 */
	const int32_t *idx0;          /* COO: device pointers */
	const int32_t *idx1;
	const double *val;
	const int64_t *row_nnz;       /* DIGEST|ROWSTATS: device pointers */
	const double *row_sum;
	/* timing of the device pipeline stages, milliseconds (HIP events) */
	float ms_consolidate, ms_symbolic, ms_numeric, ms_total;
	/* numeric kernels by row class (P_r = products of the output row):
	 * light P_r <= 64, mid <= 4096, heavy above */
	float ms_light, ms_mid, ms_heavy;
	float ms_dense;               /* part of ms_heavy spent in the dense-window kernel */
	uint32_t window;              /* column-window width the heavy rows were cut with (8192 / 16384; 0 = no heavy row) */
	uint64_t cells_hash, cells_dense;   /* heavy rows are cut into cells: LDS-hash cells and dense-window cells */
	uint64_t products_dense;            /* products of the dense-window cells (part of products_heavy) */
	uint64_t workspace_bytes;           /* device workspace this call carved from the context's arena */
	uint64_t rows_light, rows_mid, rows_heavy;
	uint64_t products_light, products_mid, products_heavy;
	uint64_t tuples_light, tuples_mid, tuples_heavy;      /* A tuples in the rows of each class */
	/* the heavy rows' hash-class cells by kernel: tiles (rows with <= 256 A tuples: hash / bitmap tiles), direct tiles
	 * (off by default: 0); the rest of ms_heavy - ms_dense is the windowed k_hash of the longer rows */
	float ms_tiles, ms_direct;
	uint64_t products_tiles, products_direct;
	const uint64_t *row_hash;     /* DIGEST|ROWSTATS: per row the sum of mix64(i, j) over its tuples (device pointer) */
} spsamd_result;

/* ---- context ---- */

/* device < 0: current device.  stream: a hipStream_t to run on, or NULL to
 * create a private one.  Fails with SPSAMD_ENODEVICE without a GPU. */
int spsamd_ctx_create(spsamd_ctx **out, int device, void *hip_stream);
void spsamd_ctx_destroy(spsamd_ctx *ctx);
const char *spsamd_last_error(const spsamd_ctx *ctx);
/* pre-size the workspace (bytes); optional, it grows on demand otherwise */
int spsamd_ctx_reserve(spsamd_ctx *ctx, size_t workspace_bytes, size_t output_tuples);
const char *spsamd_version(void);
/* Developer knobs (value 0 = default).  They select between equivalent kernels / cell sizes: the result of a
 * multiply is the same for every setting (tests/test_gpu_parity.py forces each in turn).
 *   window          8192 | 16384      column-window width of the heavy rows (default: 16384 when ncol > 2^21)
 *   cell_cap        64..4096          grouping target of the hash cells (2048)
 *   dense_min       64..4096          a window above this many products is a dense cell (3072 with bitmap tiles, else 2048)
 *   long_dense_min  > 0               the same for rows of more than 256 A tuples (1024 at 8192-column windows)
 *   long_cap        > 0               grouping target of those rows' hash cells (cell_cap)
 *   few_max         1..16 | -1        mid rows (65 .. 4096 products) of at most this many A tuples run in k_few, which holds a
 *                                     row's B segments in registers and requests the next row's B tuples a row ahead (8);
 *                                     -1: none, every mid row in k_hash.  ORDERED and EXACT_PATTERN calls: always none
 *   direct_min      > 0               a window of a tile row above this is a direct cell (off: >= dense_min)
 *   tiles_v1        1 | 2 | 3         hash tiles r01 | hash tiles v2 | bitmap-rank tiles (default: chosen per call)
 *   no_tiles, no_wmajor               1: no tiles | no window-major copy of B
 *   xcd                               0: one cell list for all XCDs | 1: static XCD parts (experiment) | 2: dense cells claimed from XCD parts (default)
 *   tile_walk       1                 the heavy rows' tiles dealt with a static grid stride (default: claimed from a counter)
 *   emit_path       1 | 2             COO order of a hash cell: LDS radix sort | bitonic network (default: by cell width)
 *   light_path      1                 binned light kernels even where every row is light
 *   light_two_pass  1                 all-light COO sink: count, scan, store (two compute passes) instead of one pass + gather
 *   trace           1                 the symbolic phase prints its choices (tile scheme, cell counts) to stderr
 *   index_budget_mb > 0               cap of the heavy rows' window indices (default: 80 % of the free device memory);
 *                                     beyond it the product goes by column blocks of op(B)
 *   spmm_path       1 | 2 | 3         multiply_dense: every row through the serial (thread per row and rhs) | lanes (wave per
 *                                     row, lanes across rhs) | fold (wave per row, ordered fold) kernel (default: by row length)
 *   spmm_long_min   > 0               multiply_dense: rows of more tuples than this go to a wave kernel (64)
 *   add_path        1                 add: sort every operand, ignoring sort0, chained results and preparation (default:
 *                                     an operand already in op()'s row-major order is read in place)
 *   masked_path     1 | 2 | 3         multiply_masked: every mask key through the entry kernel (lane per key) | the row kernel
 *                                     wherever A_i fits its LDS copy (4096 tuples; the other keys: entry) | the wave kernel
 *                                     (wave per key) (default: by the lengths of A_i and B_j)
 *   sampled_path    1 | 2             multiply_sampled: every tuple through the lane kernel (lane per tuple, rows read into
 *                                     registers) | the slab kernel (wave per 64 tuples, rows staged through LDS in slabs of
 *                                     16 values) (default: by k and a sampled probe of M's column locality and row
 *                                     order)
 *   select_path     1 | 2 | 3         select, ROW_TOPK: every row of more than k tuples through the light (a wave per row,
 *                                     rows of at most 64 tuples) | mid (a workgroup per row, keys in LDS, at most 4096 tuples) |
 *                                     heavy (a workgroup per row, keys re-read from memory) kernel wherever that kernel can
 *                                     hold the row; a row too long for the forced class falls to the next one (default: by
 *                                     row length)
 *   extract_path    1 | 2 | 3 | 4     extract: 1 every output row through the permuted path (emit, then order), even where the
 *                                     in-order path applies; 2 | 3 | 4 the same, with every output row of two or more tuples
 *                                     through the light (a wave per row, at most 64 tuples) | mid (a workgroup per row, keys
 *                                     in LDS, at most 4096 tuples) | heavy (one radix sort over all such rows) ordering kernel
 *                                     wherever that kernel can hold the row; a row too long for the forced class falls to the
 *                                     next one (default: in order where J ascends and S is column-ordered, else by row
 *                                     length)
 *   reduce_path     1 | 2             reduce: every row through the short rows' kernel (a wave per 64 consecutive rows, their
 *                                     tuples staged packed through LDS; correct for any length) | the long rows' kernel (a
 *                                     wave per 64 listed rows, a padded LDS tile of 32 values per row and step) (default:
 *                                     rows of at most 64 tuples short, the others long)
 *   emult_path      1 | 2 | 3         emult: 1 the merge of the two key streams | 2 every tuple of op(A) looks its key up in op(B)
 *                                     (inside the row where B is a prepared handle, else over the whole stream) | 3 every key of
 *                                     op(B) looks up its run in op(A) (default: the cheapest by a byte model, DESIGN.md
 *                                     section 17)
 *   solve_path      1 | 2             solve_tri: 1 every level of the schedule in a launch of its own | 2 every level whose rows
 *                                     are all short through the fused runs (one workgroup walking consecutive levels), whatever
 *                                     its width (default: levels of at most solve_fuse_rows rows fuse)
 *   solve_row       1 | 2 | 3         solve_tri: every row through the serial (thread per row and rhs) | lanes (wave per row,
 *                                     lanes across rhs) | fold (wave per row, ordered fold) kernel (default: rows of at most
 *                                     spmm_long_min tuples serial, the others lanes from 16 right-hand sides on, else fold)
 *   solve_fuse_rows > 0               solve_tri: the widest level that still counts as thin (default: 256 rows, and at most
 *                                     2048 (row, rhs) pairs; a set value is taken as given)
 *   factor_path     1 | 2             factor_ilu0: 1 every level of the schedule in launches of its own | 2 every level whose
 *                                     rows are all serial-class through the fused runs, whatever its width (default: such
 *                                     levels of at most factor_fuse_rows rows fuse)
 *   factor_row      1 | 2 | 3         factor_ilu0: every row with a lower tuple through the serial (a thread per row) | wave (a
 *                                     wave per row, the row staged in LDS) | block (a workgroup per row, the row in memory)
 *                                     kernel wherever that kernel can hold the row; a row too long for the wave kernel's LDS
 *                                     copy falls to the block kernel (default: by the row's work and length)
 *   factor_fuse_rows > 0              factor_ilu0: the widest level that still counts as thin (256 rows)
 *   factor_serial_work > 0            factor_ilu0: rows of at most this many lookups are serial-class (64)
 *   factor_lds_row  1..4096           factor_ilu0: the longest row (tuples) of the wave kernel's LDS copy (256)
 *   pcg_check_every > 0               solve_pcg, solve_bicgstab: iterations enqueued between two reads of the device state (8, DESIGN.md
 *                                     section 23)
 *   pcg_fuse        1                 solve_pcg, solve_bicgstab: every vector operation and every dot product in a launch of its own
 *                                     (default: a dot's first level rides in the kernel that produces its vector)
 *   gmres_path      1                 solve_gmres: every dot product through the frame's dot kernel with a fold of its own, and every
 *                                     w = w - coef * v a launch of its own (default: the block kernels)
 *   amg_path        1 | 2             amg_apply, solve_pcg_amg: 1 every level of the cycle in launches of its own | 2 the whole
 *                                     hierarchy in the one launch of the fused tail, whatever its levels' orders (default: the
 *                                     levels from the first one on from which none has more than amg_fuse_rows rows)
 *   amg_fuse_rows   > 0               amg_apply, solve_pcg_amg: the largest order of a level of the fused tail (1024)
 * The environment variables of the same purpose (SPSAMD_W ...) are read once, inside spsamd_ctx_create; nothing reads
 * the environment later.  Unknown names: SPSAMD_EINVAL. */
int spsamd_ctx_set_tuning(spsamd_ctx *ctx, const char *name, long value);

/*
 * ret = C * diag(scalei) * op(A) * diag(scalej) * op(B) * diag(scalek)
 * -- spsparse::multiply, matrix x matrix (multiply_sparse.hpp:152-248).
 * Argument order and meaning follow the reference; scale pointers may be NULL;
 * only the exact character 'T' transposes (multiply_sparse.hpp:167-168).
 * Operands may be host or device resident (per-operand `mem`).  The result
 * goes to the device sink named by sink_kind; host callers then use
 * spsamd_result_fetch() to stream it out in order.
 */
int spsamd_multiply(spsamd_ctx *ctx, double C,
	const spsamd_vec *scalei,
	const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej,
	const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags,
	spsamd_result *result);

/*
 * ret = C * diag(scalei) * op(A) * diag(scalej) * V
 * -- spsparse::multiply, matrix x sparse vector (multiply_sparse.hpp:281-365).
 * V is consolidated with sort order {0} (:313); a V with sort0 == 0 is taken
 * as stored, also under zero_nan (Consolidate<>, algorithm.hpp:360).  The result is rank 1:
 * result->idx0 holds the row indices, idx1 is NULL (spsamd_result_fetch then
 * passes j = NULL to the callback), shape1 is 0.
 */
int spsamd_multiply_mv(spsamd_ctx *ctx, double C,
	const spsamd_vec *scalei,
	const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej,
	const spsamd_vec *V,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags,
	spsamd_result *result);

/*
 * Host delivery of the last SINK_COO result of ctx: calls cb(user, i, j, v, n)
 * with consecutive chunks (host pointers, valid during the call) in ascending
 * (i, j) order -- the shim's callback loops ret.add({i,j}, v)
 * (multiply_sparse.hpp:242).  A non-zero return of cb stops the delivery and
 * is returned.
 */
typedef int (*spsamd_chunk_fn)(void *user, const int32_t *i, const int32_t *j,
	const double *v, size_t n);
int spsamd_result_fetch(spsamd_ctx *ctx, const spsamd_result *result,
	spsamd_chunk_fn cb, void *user);

/*
 * DenseAccum (accum.hpp:110-140) on the device: apply the tuples of a SINK_COO
 * result to a row-major dense matrix in device memory,
 *     dense[i * ld + j]  (op)=  v        per duplicate_policy
 * ADD sums into the existing entry, REPLACE overwrites it.  LEAVE_ALONE does what
 * the reference's code does, on both sides of the boundary (this entry point and the
 * host mirror in spsparse_amd/multiply.hpp): `if (!std::isnan(oval)) oval = val`
 * (accum.hpp:128-130) -- the entry is overwritten unless it holds a NaN.  SURVEY
 * Appendix A.12 notes that this looks inverted against the policy's documented
 * meaning (spsparse.hpp:19-23); a drop-in keeps the behaviour callers get today.
 */
int spsamd_result_scatter_dense(spsamd_ctx *ctx, const spsamd_result *result, double *dense_device, size_t ld,
	int duplicate_policy);

/*
 * Y (op)= op(M) * X  -- multiply_dense.hpp:11-35 (compiled out in the reference), y a DenseAccum (accum.hpp:110-140),
 * nrhs right-hand sides at once.  For each right-hand side r, over M's tuples (i, j, v) IN STORAGE ORDER ((j, i) with 'T'):
 *     p = v * X[j*ldx + r];   if (handle_nan && (isnan(p) || isinf(p))) skip;
 *     Y[i*ldy + r]:  ADD  Y += p   |   REPLACE  Y = p   |   LEAVE_ALONE  if (!isnan(Y)) Y = p   (accum.hpp:124-135)
 * Every entry of Y is bit-identical to that loop: the adds into one entry run in storage order, products and sums are
 * rounded separately (no FMA), and a NaN result has the bits x86-64 gives it (the left operand's NaN, quieted, else the
 * right one's, else 0xFFF8000000000000).  Y is never zeroed: an entry that receives no product keeps its value.  M is NOT
 * consolidated -- duplicates and explicit zeros each contribute (0 * Inf = NaN) -- except a prepared operand
 * (SPSAMD_MEM_PREPARED), which is taken as its consolidated tuples the way Consolidate<> takes a sorted array: preparing
 * merges duplicates and drops zeros, and so can change Y.
 *   X      cols(op(M)) rows of nrhs values, row-major: X[j*ldx + r]
 *   Y      rows(op(M)) rows, Y[i*ldy + r], read and written (the ldy - nrhs values after each row's are not touched)
 *   mem    SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE, for X and Y together (M has its own `mem`)
 * SPSAMD_EINVAL: M NULL, X or Y NULL while nrhs > 0 and M has a non-empty dimension, ldx or ldy < nrhs, a policy outside
 * 0..2, a bad mem, an index of M out of bounds, X and Y overlapping.  nrhs == 0 or an empty M: 0, Y untouched.
 * Returns when Y holds the result.  The workspace comes from the context's arena; neither output buffer is written, so a
 * SINK_COO result stays valid and fetchable across the call and can itself be M.
 */
int spsamd_multiply_dense(spsamd_ctx *ctx,
	const spsamd_coo *M, char transpose,
	const double *X, size_t ldx,
	double *Y, size_t ldy,
	size_t nrhs, int mem,
	int duplicate_policy, int handle_nan);

/*
 * The sampled dense-dense product (SDDMM): for every tuple of M, the dot product of a row of P with a row of Q -- the
 * dense-factor form of spsamd_multiply_masked.  For each tuple t of M IN STORAGE ORDER, as (i, j, v) -- (j, i, v) when
 * transpose is the character 'T':
 *     d = +0.0;   for r = 0 .. k-1:  d = d + P[i*ldp + r] * Q[j*ldq + r]      (serially, in ascending r)
 *     o = alpha * d;   if (beta != 0)  o = o + beta * v;                      (beta == 0: v is never read)
 *     out[t] = o
 * Every out[t] is bit-identical to that loop: products and sums are rounded separately (no FMA), there is no tree or
 * split sum over r, and a NaN result has the bits x86-64 gives it (the left operand's NaN, quieted, else the right one's,
 * else 0xFFF8000000000000; the left operand is the one written on the left above), as in spsamd_multiply_dense.
 *   P      rows(op(M)) rows of k values, row-major: P[i*ldp + r], ldp >= k
 *   Q      cols(op(M)) rows of k values, row-major: Q[j*ldq + r], ldq >= k
 *   out    one value per tuple of M, aligned with M's arrays (out[t] belongs to M's tuple t): M is NOT consolidated --
 *          duplicates and explicit zeros each get their own output.  out == M->val is allowed (an in-place update of M's
 *          values: each tuple's v is read before its slot is written).
 *   mem    SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE, for P, Q and out together (M has its own `mem`)
 * Gradient: for Y = op(M) * X (spsamd_multiply_dense) and G = dL/dY, the gradient of L with respect to M's values is this
 * product with P = G, Q = X, alpha = 1, beta = 0.
 * A prepared operand (SPSAMD_MEM_PREPARED) stands for its consolidated tuples, in the order spsamd_consolidate gives them
 * for the transpose it was prepared with; out is aligned with those.  A SINK_COO result of this context may be M (read in
 * place, its indices trusted); neither output set of the context is written, so it stays fetchable.
 * SPSAMD_EINVAL, with out not written: M NULL; P or Q NULL while k > 0 and M has tuples; out NULL while M has tuples;
 * M->val NULL while beta != 0; ldp < k or ldq < k; a bad mem; an index of M out of bounds; out overlapping P, Q or M's index
 * arrays; out overlapping M->val without being equal to it (or overlapping a prepared operand's arrays); M with 2^31 or
 * more tuples; a dimension of M above 2^31; k >= 2^31.  An empty M: 0, nothing touched.  k == 0: out[t] = alpha * 0 (+ beta * v); P and Q are not read.
 * Index arithmetic is 64-bit (rows * ld may exceed 2^32 values).  Returns when out holds the result.
 */
int spsamd_multiply_sampled(spsamd_ctx *ctx,
	const spsamd_coo *M, char transpose,
	const double *P, size_t ldp,
	const double *Q, size_t ldq,
	size_t k, double alpha, double beta,
	double *out, int mem);

/*
 * ret = alpha * op(A) + beta * op(B)  -- sparse addition (rocSPARSE / cuSPARSE csrgeam).  The result is exactly what
 *     VectorCooArray T;
 *     for (i, j, v) in op(A), in storage order:  T.add({i, j}, alpha * v);
 *     for (i, j, v) in op(B), in storage order:  T.add({i, j}, beta * v);
 *     consolidate(ret, T, {0, 1}, duplicate_policy, zero_nan);          (algorithm.hpp:251-319)
 * produces, bit for bit, NaN payloads included:
 *   - op(X) swaps the two indices exactly when its flag is the character 'T'.
 *   - the stable sort puts all of A's tuples of a key before B's; inside one operand a key's tuples keep storage order.
 *   - every scaled value is alpha * v (also for alpha == 1 or 0: 0 * Inf is a NaN and survives); a NaN product or sum has
 *     the bits x86-64 gives it, as in spsamd_multiply_dense.
 *   - consolidate()'s quirks hold over the merged sequence: zeros (and under zero_nan NaNs) before its first kept entry are
 *     dropped, after it only exact zeros (+-0); the rest is folded left to right by the policy (ADD: serial acc += v,
 *     REPLACE: the last, LEAVE_ALONE: the first); a sum that cancels to 0.0 is emitted.
 *   - sort0 and preparation only let the call skip a sort, they never change the result.  An operand whose sort0 names
 *     op()'s row order while its (row, col) keys of op() are not in that order is rejected (SPSAMD_EINVAL).  A prepared
 *     operand stands for its consolidated tuples.
 * The shape of op(A) must equal that of op(B) (SPSAMD_EDIM); the result has that shape.  SPSAMD_EINVAL: nnz(A) + nnz(B)
 * >= 2^31, an index out of bounds, a policy outside 0..2, a null pointer, both output buffers of the context operands
 * of the call.  Sinks as for spsamd_multiply: SINK_COO (row-major tuples in the context's output set, chainable as a
 * MEM_DEVICE sort0 = 0 operand -- sort0 = 1 with SINK_PERMUTE -- and fetchable), SINK_DIGEST (+ ROWSTATS); SINK_ORDERED
 * and SINK_EXACT_PATTERN are accepted and change nothing.  result: nnz, shape, nnz_a / nnz_b (input tuples),
 * ms_consolidate (the operands' sorts; 0 when none ran), ms_total, workspace_bytes.  Returns when the result is complete.
 */
int spsamd_add(spsamd_ctx *ctx,
	double alpha, const spsamd_coo *A, char transpose_A,
	double beta, const spsamd_coo *B, char transpose_B,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags,
	spsamd_result *result);

/*
 * ret = the tuples of op(A) that a predicate keeps  -- dropping entries (rocSPARSE / cuSPARSE prune_csr2csr, GraphBLAS
 * GrB_select).  No value is computed: the result is a subsequence of op(A)'s tuples.
 *   - Operand.  op(A) (indices swapped exactly when transpose is the character 'T') is taken the way spsamd_multiply takes
 *     its left operand, with duplicate_policy and zero_nan: a raw operand is consolidated by op()'s rows (stable sort,
 *     leading-run rule, zero drop, duplicates folded by the policy); an operand whose sort0 names op()'s row order is
 *     trusted as stored (duplicates, zeros and the order inside a row included) and rejected (SPSAMD_EINVAL) if its leading
 *     index descends; a SINK_COO result of this context and a prepared handle of the same transpose are read in place; a
 *     prepared handle of the other transpose is re-sorted.  Host and device operands.  Call the resulting sequence S.  The
 *     result is a SUBSEQUENCE of S: order kept, values bit for bit untouched (NaN payloads, signalling NaNs, -0.0 included).
 *   - mag(x) is the 64-bit pattern of x with the sign bit cleared, compared as an unsigned integer.  For non-NaN values that
 *     is the order of |x|; every NaN ranks above +Inf (by payload).  All three value predicates compare through it, so a NaN
 *     entry is never dropped by a value predicate and counts as the largest in a top-k.  No floating-point comparison
 *     decides an entry's fate.
 *   - TRIL / TRIU / DIAG / OFFDIAG use j - i in 64-bit arithmetic on op(A)'s indices; d = iparam may be any int64.
 *   - ABS_GE: theta = dparam must be >= 0 and not NaN (+Inf allowed: only Inf and NaN entries stay).
 *   - ROW_REL: m_i is the largest |v| over the non-NaN entries of row i of S (+0.0 when there are none); the threshold
 *     t_i = theta * m_i is one rounded double multiply (0 * Inf gives a NaN threshold: then only NaN entries whose mag is at
 *     or above it pass -- the rule above, nothing special-cased).  theta >= 0, not NaN.  theta = 0 with finite rows keeps S.
 *   - ROW_TOPK: k = iparam >= 0.  Within a row of S the tuples are ranked by (mag descending, position in S ascending);
 *     those of rank < k are kept.  In a consolidated row positions ascend with the column, so ties at the k-th magnitude
 *     go to the lowest columns; for a trusted operand the order is the stored one.  k = 0: empty result; a row of at most
 *     k tuples is kept whole.  Column-wise top-k is transpose = 'T' plus SPSAMD_SINK_PERMUTE.
 *   - SPSAMD_SELECT_COMPLEMENT inverts the decision per tuple, for every predicate (top-k: the tuples of rank >= k).
 *     For any input, predicate and parameters, select and its complement partition S.
 * Sinks as for spsamd_add: SINK_COO (tuples in the context's output set, fetchable, usable with
 * spsamd_result_scatter_dense, chainable as a MEM_DEVICE sort0 = 0 operand -- sort0 = 1 with SINK_PERMUTE), SINK_DIGEST
 * (+ ROWSTATS over rows(op(A)): row_nnz is the number of kept tuples per row); SINK_ORDERED and SINK_EXACT_PATTERN are
 * accepted and change nothing.  The operand may be the context's current output set (filtering a product in a chain):
 * the result goes to the other set.
 * result: shape, nnz, nnz_a (= |S|), ms_consolidate, ms_numeric, ms_total, workspace_bytes; for ROW_TOPK also
 * rows_light / rows_mid / rows_heavy and tuples_light / tuples_mid / tuples_heavy: the rows of S with more than k tuples,
 * and their tuples, by the kernel class that served them (rows of at most k tuples are in none).  Everything else 0 / NULL.
 * SPSAMD_EINVAL: A or result NULL, an unknown predicate, select_flags or sink, a policy outside 0..2, theta < 0 or NaN,
 * k < 0, an index out of bounds, 2^31 or more tuples.  An empty A: an empty result of op(A)'s shape.  Returns when the
 * result is complete.
 */
#define SPSAMD_SELECT_TRIL     1   /* keep (i, j) with  j - i <= d          d = iparam (int64, any sign)            */
#define SPSAMD_SELECT_TRIU     2   /*                   j - i >= d                                                  */
#define SPSAMD_SELECT_DIAG     3   /*                   j - i == d                                                  */
#define SPSAMD_SELECT_OFFDIAG  4   /*                   j - i != d                                                  */
#define SPSAMD_SELECT_ABS_GE   5   /* keep v with  mag(v) >= mag(theta)            theta = dparam                   */
#define SPSAMD_SELECT_ROW_REL  6   /* keep v with  mag(v) >= mag(theta * m_i)      m_i: the row's largest non-NaN |v| */
#define SPSAMD_SELECT_ROW_TOPK 7   /* keep the k first tuples of each row in the order (mag descending, position ascending)  k = iparam */
#define SPSAMD_SELECT_COMPLEMENT 1 /* select_flags: keep exactly the tuples the predicate would drop                */

int spsamd_select(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int predicate, int64_t iparam, double dparam, int select_flags,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *result);

/*
 * ret = op(A)(I, J), the submatrix (or reordering) of op(A) by a row list I and a column list J  -- GraphBLAS GrB_extract:
 * A_FC / A_CC of a C/F splitting, a Schwarz subdomain A(I, I), an induced subgraph, P*A*P^T for a permutation, a row block.
 * No value is computed.
 *   - Operand.  op(A) is taken exactly as spsamd_select takes it (above), with duplicate_policy and zero_nan: a raw operand
 *     is consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as stored and rejected
 *     (SPSAMD_EINVAL) if its leading index descends; a SINK_COO result of this context and a prepared handle of the same
 *     transpose are read in place.  Host and device operands.  Call the resulting sequence S.
 *   - Lists.  rows holds nrows indices into rows(op(A)), cols holds ncols indices into cols(op(A)); both live where
 *     index_mem says (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE).  SPSAMD_EXTRACT_ALL (NULL) stands for every index of that
 *     dimension, ascending (GrB_ALL); its count is ignored.  A list may be in any order and may name an index more than
 *     once: a row named twice is delivered twice, a column named m times multiplies that column's tuples by m.
 *   - Result.  Shape nrows x ncols.  For every output row r, output column c and tuple (I[r], J[c], v) of S at position p it
 *     holds one tuple (r, c, v), and no other; the order is (r, c, p) ascending.  v keeps its bits (NaN payloads,
 *     signalling NaNs, -0.0, the explicit zeros of a trusted operand): no value is computed, no floating-point comparison
 *     is made.  For a consolidated S the result has every key once, row-major; for a trusted S with duplicate keys or
 *     unordered rows the duplicates of a key follow each other in storage order.
 * Sinks as for spsamd_select: SINK_COO (fetchable, usable with spsamd_result_scatter_dense, chainable as a MEM_DEVICE
 * sort0 = 0 operand -- sort0 = 1 with SINK_PERMUTE, which swaps the index arrays and the shape), SINK_DIGEST (+ ROWSTATS
 * over the nrows output rows); SINK_ORDERED and SINK_EXACT_PATTERN are accepted and change nothing.  The operand may live
 * in the context's current output set: the result goes to the other set.
 * result: shape, nnz, nnz_a (= |S|), ms_consolidate, ms_symbolic (list checks, column map, count, scan), ms_numeric (emit and
 * ordering), ms_total, workspace_bytes; rows_light / rows_mid / rows_heavy and tuples_light / tuples_mid / tuples_heavy: the
 * output rows of two or more tuples, and their tuples, by the ordering kernel class that served them -- all 0 on the in-order
 * path (J ALL or strictly ascending and S column-ordered inside its rows), where nothing needs ordering.  Everything else
 * 0 / NULL.
 * SPSAMD_EINVAL, with a message and nothing written: A or result NULL; index_mem neither HOST nor DEVICE, or a list
 * pointer that is not of that kind; an entry of rows outside [0, rows(op(A))) or of cols outside [0, cols(op(A))) (the
 * message names the first such position); nrows or ncols >= 2^31; a policy outside 0..2; an unknown sink; an index of A out
 * of bounds; a result of 2^31 or more tuples (possible only with repeated indices; the message names the count); a device
 * list that lies in the output set about to be written.  nrows == 0, ncols == 0 or an empty S: an empty result of shape
 * nrows x ncols.  Returns when the result is complete.
 */
#define SPSAMD_EXTRACT_ALL NULL   /* rows / cols == NULL: every index of that dimension, ascending (GrB_ALL) */
int spsamd_extract(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	const int32_t *rows, size_t nrows,      /* I: nrows indices into rows(op(A)); NULL: all rows (nrows ignored) */
	const int32_t *cols, size_t ncols,      /* J: ncols indices into cols(op(A)); NULL: all columns (ncols ignored) */
	int index_mem,                          /* SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE, for rows and cols together */
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *result);

/*
 * v = post(reduce(op(A)))  -- a matrix reduced to a vector along its rows (GraphBLAS GrB_reduce to a vector; column
 * reductions are transpose = 'T'): row sums, 1- and 2-norms, the largest magnitude, the tuple count and the diagonal, with an
 * optional reciprocal / square root, straight into caller-owned memory -- device memory included, so that a chained product
 * is scaled (spsamd_multiply's scalei / scalej / scalek with mem = SPSAMD_MEM_DEVICE) without a trip to the host.
 *   - Operand.  op(A) is taken exactly as spsamd_select takes it (above), with duplicate_policy and zero_nan: a raw operand
 *     is consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as stored (duplicates, zeros
 *     and the order inside a row included) and rejected (SPSAMD_EINVAL) if its leading index descends; a SINK_COO result of
 *     this context and a prepared handle of the same transpose are read in place.  Host and device operands.  Call the
 *     resulting sequence S.
 *   - Rows.  The contributing tuples of row i are all its tuples in S -- for SPSAMD_REDUCE_DIAG only those with column i.  A
 *     row appears in the result if and only if it has at least one contributing tuple.
 *   - Value.  r_i is the fold written beside each constant below over the contributing tuples IN S's ORDER, serially: every
 *     add and multiply is rounded on its own (no FMA, no tree or split sum), and a NaN result has the bits x86-64 gives it
 *     (the left operand's NaN, quieted, else the right one's, else 0xFFF8000000000000; the accumulator is the left operand),
 *     as in spsamd_multiply_dense.  MAX_ABS is the largest |v| over the non-NaN tuples, compared through mag like
 *     spsamd_select does, +0.0 when there is none: bit for bit the m_i of SPSAMD_SELECT_ROW_REL.  COUNT is exact (a row
 *     holds fewer than 2^31 tuples).  The emitted value is post(r_i): RECIP = 1.0 / r and SQRT = sqrt(r) are the correctly
 *     rounded IEEE operations, RSQRT is SQRT followed by RECIP (two roundings); a NaN result has x86's bits (1.0 / NaN and
 *     sqrt(NaN): the operand quieted; sqrt(r < 0): 0xFFF8000000000000; sqrt(-0.0) = -0.0).
 *   - No entry is dropped for its value: zeros, infinities and NaNs are emitted.  NOTE for scale vectors: spsamd_multiply
 *     treats a zero scale entry like a missing one (isnone, multiply_sparse.hpp:195,211) and skips that row, column or k.
 *   - Output, caller-owned; mem says where out_idx and out_val live (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE).
 *       sparse form (out_idx != NULL): the entries (i, post(r_i)), i strictly ascending -- a valid spsamd_vec of shape0 =
 *         rows(op(A)), ready to be a scale vector.  *out_nnz gets their number.  capacity < that number: nothing is written,
 *         *out_nnz gets the number needed and the call returns SPSAMD_ECAPACITY (capacity = 0 is the size query).
 *       dense form (out_idx == NULL): out_val[i] for every row of op(A) -- what spsamd_multiply_dense and
 *         spsamd_multiply_sampled consume; rows without a contributing tuple get +0.0 (no post-operation applied to them).
 *         *out_nnz is still the number of rows with one.  capacity < rows(op(A)): SPSAMD_ECAPACITY, nothing written,
 *         *out_nnz = rows(op(A)).
 *     Neither output set of the context is written: a SINK_COO result may be A and stays valid and fetchable.
 *   - result (may be NULL): shape0 = rows(op(A)), shape1 = 0, nnz = the count, nnz_a = |S|, ms_consolidate, ms_numeric,
 *     ms_total, workspace_bytes; rows_light / rows_heavy and tuples_light / tuples_heavy: the non-empty rows of S, and their
 *     tuples, by the kernel that served them (the short rows' and the long rows' kernel; all 0 for COUNT, which reads the row
 *     pointer only).  Everything else 0 / NULL.  `Nothing written` below and above means the output
 *     buffers: on SPSAMD_ECAPACITY result is zeroed with shape0 set, and the sparse form has filled nnz_a too (its count
 *     is known only after the intake; the dense form is refused before it).  On another error result is unspecified.
 * SPSAMD_EINVAL, with a message and nothing written: A, out_val or out_nnz NULL; an unknown op or post; a policy outside
 * 0..2; a bad mem; an index of A out of bounds; a false sort0; 2^31 or more tuples; out_idx / out_val overlapping each
 * other or A's arrays, or, for device buffers, lying in either output set of the context.  An empty S: 0 with count 0 (the
 * dense form is then filled with +0.0).  Returns when the output is complete.
 */
#define SPSAMD_REDUCE_SUM      1   /* acc = +0.0;  acc = acc + v                       */
#define SPSAMD_REDUCE_SUM_ABS  2   /* acc = +0.0;  acc = acc + |v|   (sign bit cleared) */
#define SPSAMD_REDUCE_SUM_SQ   3   /* acc = +0.0;  acc = acc + v * v (two roundings)    */
#define SPSAMD_REDUCE_MAX_ABS  4   /* spsamd_select ROW_REL's m_i                       */
#define SPSAMD_REDUCE_COUNT    5   /* the number of tuples, as a double                 */
#define SPSAMD_REDUCE_DIAG     6   /* SUM over the row's tuples with col == row only    */

#define SPSAMD_POST_NONE   0
#define SPSAMD_POST_RECIP  1       /* 1.0 / r            */
#define SPSAMD_POST_SQRT   2       /* sqrt(r)            */
#define SPSAMD_POST_RSQRT  3       /* 1.0 / sqrt(r): two rounded operations */

int spsamd_reduce(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int op, int post, int duplicate_policy, int zero_nan,
	int32_t *out_idx, double *out_val, size_t capacity, int mem,
	size_t *out_nnz, spsamd_result *result /* may be NULL */);

/*
 * ret = op(A) o op(B) over the intersection of the two patterns, or op(A) restricted to / taken off op(B)'s pattern  --
 * GraphBLAS GrB_eWiseMult and its structural relatives: the strength of connection A o A^T, a Galerkin product kept on a
 * prescribed stencil, a frontier minus the visited set.
 *   - Operand A.  op(A) is taken exactly as spsamd_select takes it (above), with duplicate_policy and zero_nan: a raw operand
 *     is consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as stored; a SINK_COO result
 *     of this context and a prepared handle of the same transpose are read in place.  Call the resulting sequence S_A.
 *   - Trusted operands must ascend.  An operand trusted as stored must be non-descending in its full (row, col) key of op()
 *     (equal keys allowed); otherwise SPSAMD_EINVAL, the rule of spsamd_add.  A SINK_COO result of this context handed back
 *     in is NOT inspected (as in spsamd_add): a product, sum or consolidation ascends by construction, but a select, extract
 *     or emult result is a subsequence of its own operand, so one made from a trusted operand whose columns descend inside
 *     a row must not be chained into this call or spsamd_add -- its matches would be missed silently (never out of bounds).
 *   - Operand B under TIMES is taken like A, giving S_B.  The partner of a tuple of S_A with key (i, j) is the FIRST tuple of
 *     S_B with that key.
 *   - Operand B under FIRST (with or without COMPLEMENT) is structural, exactly like M in spsamd_multiply_masked: B->val is
 *     never read and may be NULL, duplicate keys count once, explicit zeros count, a false sort0 is rejected.
 *   - Result.  For every tuple (i, j, a) of S_A at position p whose key is a key of B (under COMPLEMENT: is NOT a key of B)
 *     the result holds one tuple, and no other; the order is (i, j, p) ascending, so the result is a subsequence of S_A.
 *       TIMES   v = (alpha * a) * b: two rounded multiplies, left to right, a NaN result with the bits x86-64 gives it (the
 *               left operand's NaN, quieted, else the right one's, else 0xFFF8000000000000), as in spsamd_add.  alpha is
 *               applied even when it is 1 or 0.
 *       FIRST   v = a, bits untouched (NaN payloads, signalling NaNs, -0.0); alpha is not read.
 *     Nothing is dropped by value: a product that is 0.0 or NaN is emitted; the pattern depends on keys only.  For any
 *     input, FIRST and FIRST | COMPLEMENT partition S_A.
 * op(A) and op(B) must have equal shape (SPSAMD_EDIM); the result has that shape.  Sinks as for spsamd_select: SINK_COO
 * (fetchable, usable with spsamd_result_scatter_dense, chainable as a MEM_DEVICE sort0 = 0 operand -- sort0 = 1 with
 * SINK_PERMUTE), SINK_DIGEST (+ ROWSTATS); SINK_ORDERED and SINK_EXACT_PATTERN are accepted and change nothing.  An operand
 * may live in the context's current output set: the result goes to the other set.  The same struct on both sides with equal
 * transposes is legal (A o A).
 * result: shape, nnz, nnz_a (= |S_A|), nnz_b (|S_B|; B's unique keys when B is structural), products (the probe tuples
 * searched: 0 when the merge path ran, see the emult_path knob), ms_consolidate, ms_numeric, ms_total, workspace_bytes.
 * Everything else 0 / NULL.
 * SPSAMD_EINVAL, with a message and nothing written: A, B or result NULL; an unknown op or flag; COMPLEMENT with TIMES; a
 * policy outside 0..2; an unknown sink; an index out of bounds; 2^31 or more tuples in either operand; a NULL val where it
 * is read; both output sets of the context being operands of the call.  An empty A: an empty result (B is still checked).  An
 * empty B: an empty result, under COMPLEMENT S_A.  Returns when the result is complete.
 */
#define SPSAMD_EMULT_TIMES 1  /* v = (alpha * a) * b: two rounded multiplies, left to right, x86 NaN bits (ref_mul of x86fp.h) */
#define SPSAMD_EMULT_FIRST 2  /* v = a, bits untouched; B is structural */
#define SPSAMD_EMULT_COMPLEMENT 1  /* emult_flags, FIRST only: keep the tuples of op(A) whose key is NOT a key of op(B) */

int spsamd_emult(spsamd_ctx *ctx, int op, int emult_flags,
	double alpha, const spsamd_coo *A, char transpose_A,
	const spsamd_coo *B, char transpose_B,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *result);

/*
 * Solve T * X = B for X, T the `uplo` triangle of op(A): a sparse triangular solve with nrhs right-hand sides by level
 * schedule (the counterpart of rocSPARSE / cuSPARSE csrsv and csrsm).  With it a Gauss-Seidel or SOR
 * sweep ((D + L)^-1 r: LOWER on the whole matrix, no select in front) and an ILU / IC application (LOWER | UNIT, then UPPER)
 * stay in this library.
 *   - Operand.  op(A) is taken exactly as spsamd_select takes it, with duplicate_policy and zero_nan: a raw operand is
 *     consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as stored (duplicates and
 *     explicit zeros included); a SINK_COO result of this context and a prepared handle of the same transpose are read in
 *     place.  Call the resulting sequence S.  op(A) must be square (SPSAMD_EDIM); n is its order.
 *   - Used triangle (rocSPARSE's fill-mode rule).  Under LOWER the tuples with j > i, under UPPER those with j < i, are
 *     skipped and their values never read; under DIAG_UNIT the tuples with j == i are skipped as well.
 *   - Every bit of X is defined by this loop, run for each right-hand side r over the rows in ascending i (LOWER) or
 *     descending i (UPPER):
 *         acc = B[i * ldb + r];  d = +0.0
 *         for each used tuple (i, j, v) of row i, in S's order:
 *             if j == i:  d = d + v                        (the fold of spsamd_reduce's DIAG)
 *             else:       acc = acc - v * X[j * ldx + r]   (the product rounded, then the subtraction rounded: no FMA)
 *         X[i * ldx + r] = UNIT ? acc : acc / d            (a true IEEE division, not a multiplication by a reciprocal)
 *     A NaN result carries the bits x86-64 gives it (mulsd, addsd, subsd, divsd): the left operand's NaN quieted, else the
 *     right one's, else 0xFFF8000000000000.  A missing or zero diagonal is no error: d stays +-0.0 and the division gives
 *     what IEEE gives; a row without a used tuple gives B / +0.0 (B under UNIT).
 *   - B and X are row-major like multiply_dense's arrays: n rows of nrhs values, ldb, ldx >= nrhs, the ld - nrhs trailing
 *     values of a row never touched; `mem` (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE) holds for both.  X == B with ldx == ldb
 *     solves in place; any other overlap of X with B or with A's arrays, and a device X inside an output set of the
 *     context, are SPSAMD_EINVAL.  Neither output set is written: a SINK_COO result stays valid and can be A.
 *   - The schedule: level(i) = 0 for a row without a used off-diagonal tuple, else 1 + the largest level of the rows its
 *     used off-diagonal tuples name (by pattern: explicit zeros count).  The rows of a level are solved together; a run of
 *     consecutive thin levels is one launch of one workgroup.  A prepared handle of the same transpose keeps the schedule
 *     of each (uplo, diag) it was solved with (spsamd_operand_bytes grows once); any other operand is analysed per call.
 * stats (may be NULL): see the struct.  result (may be NULL): shape0 = shape1 = n, nnz_a = |S|, ms_consolidate, ms_symbolic
 * (the analysis), ms_numeric, ms_total, workspace_bytes; everything else 0 / NULL.
 * SPSAMD_EINVAL, with a message and X untouched: A NULL; B or X NULL while nrhs > 0 and n > 0; uplo or diag out of range;
 * ldb or ldx < nrhs; a bad mem or policy; an index out of bounds; a false sort0; 2^31 or more tuples.  nrhs == 0 or n == 0
 * returns 0 with nothing touched.  Returns when X is complete.
 */
#define SPSAMD_TRI_LOWER 0
#define SPSAMD_TRI_UPPER 1
#define SPSAMD_DIAG_NONUNIT 0
#define SPSAMD_DIAG_UNIT 1
typedef struct {
	uint64_t levels, max_level_rows;  /* of the schedule */
	uint64_t launches;                /* kernel launches of the numeric phase of this call */
	uint64_t fused_levels;            /* levels served inside a fused run */
	uint64_t tuples_used;             /* tuples of S in the used triangle, diagonal included unless UNIT */
	int64_t  zero_pivot;              /* smallest row with d_i == +-0.0 (NONUNIT only), else -1 */
	uint32_t analysis_reused;         /* 1: the schedule came from a prepared handle */
	float ms_analysis, ms_solve;
	uint64_t peel_thin_launches;      /* the analysis of this call: launches of the one-workgroup peel (thin frontiers) ... */
	uint64_t peel_wide_launches;      /* ... and of the level-per-launch peel, those that found an empty frontier included;
	                                     both 0 when analysis_reused is 1 or no off-diagonal tuple is used */
} spsamd_solve_stats;

int spsamd_solve_tri(spsamd_ctx *ctx, const spsamd_coo *A, char transpose, int uplo, int diag,
	const double *B, size_t ldb, double *X, size_t ldx, size_t nrhs, int mem,
	int duplicate_policy, int zero_nan,
	spsamd_solve_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * ret = F, the incomplete LU factorisation of op(A) on its own pattern, ILU(0), by level schedule (the counterpart of
 * rocSPARSE / cuSPARSE csrilu0, as spsamd_solve_tri is of csrsv).  F holds L strictly below the
 * diagonal (its unit diagonal is implied) and U on and above it, so the application U^-1 L^-1 r is
 * spsamd_solve_tri(F, LOWER, UNIT), then spsamd_solve_tri(F, UPPER, NONUNIT).
 *   - Operand.  op(A) is taken exactly as spsamd_select takes it, with duplicate_policy and zero_nan: a raw operand is
 *     consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as stored; a SINK_COO result of
 *     this context and a prepared handle of the same transpose are read in place.  Call the resulting sequence S.  op(A)
 *     must be square (SPSAMD_EDIM); n is its order.
 *   - S must be strictly ascending in its (row, col) key: no duplicate key, columns ascending inside a row.  This is checked
 *     on the device for every kind of operand, chained results included (a select of a trusted operand may descend inside a
 *     row).  A violation is SPSAMD_EINVAL; the message names the first offending position, and nothing is written.  Explicit
 *     zeros of a trusted operand are pattern.
 *   - Result.  S's keys, all of them, in S's order, with the values f this loop defines:
 *         f_t = value of tuple t of S, for every t
 *         for i = 0 .. n-1:
 *           for each tuple t = (i, k) of row i with k < i, in ascending k:
 *               f_t = f_t / p_k           p_k: f of row k's diagonal tuple (final, since k < i); +0.0 if row k stores none
 *               for each tuple s = (k, j) of row k with j > k:
 *                   if row i stores a tuple u = (i, j):   f_u = f_u - f_t * f_s
 *     The product is rounded, then the subtraction (no FMA); the division is a true IEEE division, not a multiplication by
 *     a reciprocal; a NaN result carries the bits x86-64 gives it (mulsd, subsd, divsd: the left operand's NaN quieted, else
 *     the right one's, else 0xFFF8000000000000; f_t is the left operand of the product).  Every f_u is one serial chain -- its
 *     updates in ascending k, then (for j < i) one division -- so every value is defined bit for bit.  Nothing is dropped by
 *     value: an f of 0.0, Inf or NaN is stored.  A missing or zero pivot is no error: the division gives what IEEE gives.
 *   - The schedule is that of spsamd_solve_tri's LOWER triangle (off-diagonal tuples by pattern).  A prepared handle of the
 *     same transpose uses and keeps the LOWER / NONUNIT schedule, so a factorisation after a Gauss-Seidel solve on the same
 *     handle, or the reverse, analyses nothing (spsamd_operand_bytes grows once).  Level 0 (the rows without a lower tuple)
 *     has no work: it is never launched, and not counted in fused_levels.
 * Sinks as for spsamd_emult: SINK_COO (fetchable, chainable as a MEM_DEVICE sort0 = 0 operand -- sort0 = 1 with
 * SINK_PERMUTE), SINK_DIGEST (+ ROWSTATS); SINK_ORDERED and SINK_EXACT_PATTERN are accepted and change nothing.  The operand
 * may live in the context's current output set: F goes to the other set.
 * stats (may be NULL): see the struct.  result: shape, nnz (= |S|), nnz_a (= |S|), products (= lookups), ms_consolidate,
 * ms_symbolic (the row pass and the analysis), ms_numeric, ms_total, workspace_bytes; everything else 0 / NULL.
 * SPSAMD_EINVAL, with a message and nothing written: A or result NULL; a bad policy or sink; an index out of bounds; a false
 * sort0; 2^31 or more tuples; the ordering rule above.  n == 0 or an empty S: an empty result of op(A)'s shape.  Returns
 * when the result is complete.
 */
typedef struct {
	uint64_t levels, max_level_rows;  /* of the schedule */
	uint64_t launches;                /* kernel launches of the numeric phase of this call */
	uint64_t fused_levels;            /* levels (from level 1 on) served inside a fused run */
	uint64_t lookups;                 /* sum over the lower tuples (i, k) of the tuples of row k right of its diagonal: the work */
	uint64_t updates;                 /* the lookups that found a tuple in row i: the subtractions performed */
	int64_t  zero_pivot;              /* smallest row whose final p_i is +-0.0, a row without a stored diagonal included (a NaN
	                                     pivot is not one), else -1 */
	int64_t  missing_diag;            /* smallest row that stores no diagonal, else -1 */
	uint64_t rows_serial, rows_wave, rows_block;   /* rows with at least one lower tuple, by the kernel that served them */
	uint32_t analysis_reused;         /* 1: the schedule came from a prepared handle */
	float ms_analysis, ms_factor;
} spsamd_factor_stats;

int spsamd_factor_ilu0(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int duplicate_policy, int zero_nan, int sink_kind, int sink_flags,
	spsamd_factor_stats *stats /* may be NULL */, spsamd_result *result);

/*
 * A greedy multi-colour ordering of op(A)'s graph by independent sets.  Rows of one colour share
 * no tuple, so P*A*P^T for the permutation `perm` has at most `ncolors` levels in spsamd_solve_tri's and
 * spsamd_factor_ilu0's schedules; the colour classes also serve multi-colour Gauss-Seidel and coarsening.
 *   - Operand.  op(A) is structural, taken exactly as spsamd_multiply_masked takes M: val is never read and may be NULL,
 *     duplicate keys count once, explicit zeros count; host, device, a chained SINK_COO result of this context (read in
 *     place) and a prepared handle are accepted; sort0 only lets the call skip the sort, and a false one is rejected.
 *     There is no duplicate_policy / zero_nan: a colouring of a superset of a pattern is proper for the pattern.  op(A)
 *     must be square (SPSAMD_EDIM); n is its order, K its sorted unique key set.
 *   - Graph.  N(i) = { j != i : (i, j) in K or (j, i) in K }; under SPSAMD_COLOR_SYMMETRIC the caller states that the
 *     pattern is symmetric and N(i) = { j != i : (i, j) in K } -- row i alone, no symmetrisation pass.  deg(i) = |N(i)|.
 *     Without the flag the graph of A^T is the graph of A: `transpose` changes nothing in the output.
 *   - Order.  key(v) = (order == SPSAMD_COLOR_ORDER_DEGREE ? deg(v) : 0) << 32 | h(v), with 32-bit wrapping arithmetic in
 *         h = v + seed * 0x9E3779B9;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *     u precedes v when key(u) > key(v).  Every step of h is invertible, so h is a bijection of the index and keys never tie.
 *   - Every output is defined by this loop:
 *         color[v] = -1 for all v
 *         for v in descending key:   color[v] = the smallest c >= 0 that no u in N(v) with color[u] >= 0 holds
 *         round(v) = 0 if no u in N(v) precedes v, else 1 + max round(u) over those u
 *     An isolated vertex gets colour 0.  ncolors = 1 + the largest colour (0 for n = 0), rounds = 1 + the largest round
 *     (0 for n = 0), adjacency = the sum of deg.  The device runs the loop as a Jones-Plassmann sweep, synchronous in
 *     rounds -- vertex v is coloured in round(v) -- which returns exactly the loop's colours: all of these are functions
 *     of K, order, seed and the flag only, never of timing or of a tuning knob.
 *   - color (required) gets n colours.  perm (may be NULL) gets the n vertices ascending in (colour, index): the list to
 *     hand to spsamd_extract as both rows and cols for P*A*P^T, new index r being old vertex perm[r].  color_ptr (may be
 *     NULL) gets ncolors + 1 entries: color_ptr[c] is the first position of colour c in perm, color_ptr[ncolors] = n.
 *     The buffers are the caller's; `mem` (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE) holds for all three.  color_ptr with
 *     ptr_capacity < ncolors + 1: nothing is written, *out_ncolors gets the count and the call returns SPSAMD_ECAPACITY;
 *     a capacity of n + 1 always suffices.
 *   - conflicts = the keys (i, j) of K with i != j and color[i] == color[j], counted after the sweep.  Always 0 without the
 *     flag; with it, non-zero exactly where a false promise of symmetry mattered -- the call still succeeds.
 * Workspace only, like spsamd_reduce: neither output set of the context is written, so a chained result stays valid and
 * can be A.  SPSAMD_EINVAL, with a message and nothing written: A, color or out_ncolors NULL; an order, flag or mem
 * outside the above; buffers that overlap each other or A's arrays; a device buffer inside an output set of the context;
 * an index out of bounds; a false sort0; 2^31 or more tuples.  n == 0 returns 0 with *out_ncolors = 0.
 * stats (may be NULL): see the struct.  result (may be NULL): shape, nnz_a (= |K|), ms_consolidate (the intake of K),
 * ms_symbolic (the adjacency), ms_numeric (the sweep, perm and delivery), ms_total, workspace_bytes; everything else
 * 0 / NULL.  Returns when the buffers are complete.
 */
#define SPSAMD_COLOR_ORDER_HASH    0   /* visit by hashed index */
#define SPSAMD_COLOR_ORDER_DEGREE  1   /* largest degree first, hash among equal degrees */
#define SPSAMD_COLOR_SYMMETRIC     1   /* color_flags: the caller states that the pattern is symmetric */

typedef struct {
	uint64_t ncolors, rounds;         /* of the colouring */
	uint64_t adjacency, max_degree;   /* the sum and the largest of deg */
	uint64_t conflicts;               /* see above */
	uint64_t launches;                /* round-kernel launches of the sweep of this call (a fused run is one) */
	uint64_t fused_rounds;            /* rounds served inside the fused run: the tail of the sweep, one workgroup */
	uint64_t rows_thread, rows_wave;  /* vertices of degree >= 1 by the kernel class that coloured them */
	float ms_adjacency, ms_color;
} spsamd_color_stats;

int spsamd_color(spsamd_ctx *ctx, const spsamd_coo *A, char transpose, int order, uint32_t seed, int color_flags,
	int32_t *color, int32_t *perm, int32_t *color_ptr, size_t ptr_capacity, int mem,
	size_t *out_ncolors, spsamd_color_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * MIS(2) aggregation of op(A)'s graph: the coarsening step of aggregation multigrid.  A distance-2
 * maximal independent set is chosen in the order of spsamd_color's key, and an aggregate is grown around every root.
 *   - Operand.  op(A) is structural, taken exactly as spsamd_color takes it: val is never read and may be NULL, duplicate
 *     keys count once, explicit zeros count; host, device, a chained SINK_COO result of this context (read in place) and a
 *     prepared handle are accepted; sort0 only lets the call skip the sort, and a false one is rejected.  op(A) must be
 *     square (SPSAMD_EDIM); n is its order, K its sorted unique key set.  Strength filtering is not part of this call:
 *     run spsamd_select or spsamd_emult first and chain the result.
 *   - Graph.  N(i) = { j != i : (i, j) in K or (j, i) in K }.  Under SPSAMD_AGG_SYMMETRIC the caller states that the pattern
 *     is symmetric and N(i) is row i alone, without a symmetrisation pass; the promise is checked: asymmetric = the number
 *     of keys (i, j) of K with i != j and (j, i) not in K, and if it is not 0 the call returns SPSAMD_EINVAL with a message
 *     and writes no buffer (a distance-2 set on a directed pattern has no definition worth pinning).  deg(i) = |N(i)|,
 *     N[v] = N(v) + {v}.  u is WITHIN DISTANCE 2 of v when u != v and u is in N[w] for some w in N[v].
 *   - Order.  key(v) = (order == SPSAMD_AGG_ORDER_DEGREE ? deg(v) : 0) << 32 | h(v), h and the seed mixing exactly
 *     spsamd_color's.  u precedes v when key(u) > key(v); keys never tie.
 *   - Every output is defined by this loop:
 *         root[v] = 0 for all v
 *         for v in descending key:   root[v] = 1 unless some u within distance 2 of v has root[u] = 1
 *         id(r) = the number of roots with index < r                 (roots numbered in ascending vertex index)
 *         ring 0:  a root v:                            agg[v] = id(v)
 *         ring 1:  a non-root v with a root r in N(v):  agg[v] = id(r)    (r is unique: two roots in N(v) would lie within distance 2)
 *         ring 2:  every other v:                       agg[v] = agg[w], w the ring-1 vertex of N(v) with the largest key
 *                                                       (one exists: the set is maximal, so a root lies at distance exactly 2)
 *     An isolated vertex is a root and an aggregate of its own.  naggregates = the number of roots (0 for n = 0); ring1 and
 *     ring2 count the vertices of those rings.
 *   - rounds is defined by the synchronous form the device runs:
 *         state[v] = UNDECIDED for all v;  t = 0
 *         while some v is UNDECIDED:
 *             for every UNDECIDED v, all from the states at the start of the round:
 *                 if a ROOT lies within distance 2 of v:                         v becomes OUT
 *                 elif key(v) > key(u) for every UNDECIDED u within distance 2:  v becomes ROOT
 *             t += 1
 *         rounds = t
 *     whose roots are exactly the loop's (DESIGN.md section 24 has the proof).  All of the above are functions of K, order,
 *     seed and the flag only, never of timing or of a tuning knob.
 *   - agg (required) gets n aggregate ids.  members (may be NULL) gets the n vertices ascending in (aggregate, ring, index):
 *     members[agg_ptr[a]] is the root of aggregate a, its ring 1 follows, then its ring 2.  agg_ptr (may be NULL) gets
 *     naggregates + 1 bounds into members.  The buffers are the caller's; `mem` (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE) holds
 *     for all three.  agg_ptr with ptr_capacity < naggregates + 1: nothing is written, *out_naggregates gets the count and
 *     the call returns SPSAMD_ECAPACITY; a capacity of n + 1 always suffices.
 *   - The tentative prolongator P (n x naggregates) is the spsamd_coo { idx0 = 0 .. n - 1, idx1 = agg, val = 1.0, sort0 = 0 }:
 *     sorted, one tuple per row, to be trusted as it stands; the Galerkin operator is P^T (A P) by two spsamd_multiply calls.
 * Workspace only, like spsamd_color: neither output set of the context is written, so a chained result stays valid and
 * can be A.  SPSAMD_EINVAL, with a message and nothing written: A, agg or out_naggregates NULL; an order, flag or mem
 * outside the above; buffers that overlap each other or A's arrays; a device buffer inside an output set of the context;
 * an index out of bounds; a false sort0; 2^31 or more tuples; a false promise of symmetry.  n == 0 returns 0 with
 * *out_naggregates = 0.  stats (may be NULL): see the struct.  result (may be NULL): the fields spsamd_color fills, with
 * ms_numeric the sweep and the assignment together.  Returns when the buffers are complete.
 */
#define SPSAMD_AGG_ORDER_HASH    0   /* visit by hashed index */
#define SPSAMD_AGG_ORDER_DEGREE  1   /* largest degree first, hash among equal degrees */
#define SPSAMD_AGG_SYMMETRIC     1   /* agg_flags: the caller states that the pattern is symmetric (checked) */

typedef struct {
	uint64_t naggregates, rounds;     /* of the aggregation */
	uint64_t ring1, ring2;            /* vertices adjacent to their root, and at distance 2 of it */
	uint64_t max_size, min_size;      /* the largest and smallest aggregate (agg_ptr's differences), 0 for n = 0 */
	uint64_t adjacency, max_degree;   /* the sum and the largest of deg */
	uint64_t asymmetric;              /* see above; counted under the flag only, else 0 */
	uint64_t launches;                /* spread and decide launches of the sweep of this call (a fused run is one) */
	uint64_t fused_rounds;            /* rounds served inside the fused run: the tail of the sweep, one workgroup */
	uint64_t rows_thread, rows_wave;  /* vertices by the kernel class that walks their row (degree 0: always thread) */
	float ms_adjacency, ms_sweep, ms_assign;
} spsamd_aggregate_stats;

int spsamd_aggregate(spsamd_ctx *ctx, const spsamd_coo *A, char transpose, int order, uint32_t seed, int agg_flags,
	int32_t *agg, int32_t *members, int32_t *agg_ptr, size_t ptr_capacity, int mem,
	size_t *out_naggregates, spsamd_aggregate_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * Solve op(A) x = b by preconditioned conjugate gradients, one right-hand side, the whole loop on the device (DESIGN.md
 * section 23).  It is what the preconditioner stack is for: spsamd_factor_ilu0's result (after spsamd_color + spsamd_extract
 * or not) is M, spsamd_solve_tri's level schedules are built at most once per call, the scalars never visit the host.
 *   - Operands.  op(A) and op(M) are taken exactly as spsamd_solve_tri takes its operand, duplicate_policy and zero_nan
 *     included: a raw operand is consolidated by op()'s rows; an operand whose sort0 names op()'s row order is trusted as
 *     stored; a SINK_COO result of this context and a prepared handle of the same transpose are read in place.  Call the
 *     resulting sequences S (of A) and F (of M).  Both must be square and of one order n (SPSAMD_EDIM).  M is given under
 *     SPSAMD_PRECOND_LU and only then.
 *   - b and x are n doubles in `mem` (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE, for both).  x holds x0 on entry and the iterate
 *     at the stop on return.  x may not overlap b, A's or M's arrays, nor lie in an output set of the context (SPSAMD_EINVAL).
 *     Neither output set is written: A is usually a chained result and M the spsamd_factor_ilu0 result in the other set.
 *   - Every value returned -- x, hist, iterations, reason, bb, rr0, rr -- is defined by the loop below, bit for bit.
 *     Products and sums are rounded separately (no FMA), divisions are true IEEE divisions, and a NaN result carries the
 *     bits x86-64 gives it (the left operand's NaN quieted, else the right one's, else 0xFFF8000000000000).
 *       dot(u, w):  t[e] = u[e] * w[e] for e < n;  return fold(t, n)            (the fold of nothing is +0.0)
 *       fold(t, m): for each chunk g of 1024 consecutive elements (the last may be short):
 *                      for lane l = 0 .. 63:  a_l = +0.0;  for k = 0 .. 15:  e = 1024 g + 64 k + l;  if e < m:  a_l = a_l + t[e]
 *                      for s = 32, 16, 8, 4, 2, 1:  for l < s:  a_l = a_l + a_{l+s}       (a_l is the left operand)
 *                      t'[g] = a_0
 *                   with c = ceil(m / 1024) chunks:  c == 1 ? t'[0] : fold(t', c)
 *       q = A p:    q_i = acc after  acc = +0.0;  acc = acc + v * p_j  over row i's tuples (i, j, v) of S in S's order
 *                   (spsamd_multiply_dense with ADD into +0.0, handle_nan off)
 *       z = M^-1 r: NONE  z = r  |  JACOBI  z_i = r_i / d_i, d the DIAG fold of spsamd_reduce over S (+0.0 without a
 *                   diagonal tuple)  |  LU  the loops of spsamd_solve_tri on F: LOWER | UNIT on r, then UPPER | NONUNIT
 *       usable(v):  v is finite and not +-0.0
 *
 *       bb = dot(b, b);  thresh = (tol * tol) * bb
 *       q = A x;  r_i = b_i - q_i;  rr = dot(r, r);  k = 0;  hist[0] = rr;  rr0 = rr
 *       loop:
 *           if rr <= thresh:   stop CONVERGED          (a NaN compares false)
 *           if k == max_iter:  stop MAXITER
 *           z = M^-1 r;  rz' = dot(r, z)
 *           if k == 0:  p = z          else:  beta = rz' / rz;  p_i = z_i + beta * p_i
 *           rz = rz'
 *           if not usable(rz):  stop BREAKDOWN
 *           q = A p;  pq = dot(p, q)
 *           if not usable(pq):  stop BREAKDOWN
 *           alpha = rz / pq
 *           x_i = x_i + alpha * p_i;   r_i = r_i - alpha * q_i
 *           rr = dot(r, r);  k = k + 1;  hist[k] = rr
 *     At a stop x is the iterate after k iterations.  hist_host (host memory, may be NULL) gets hist[k] for
 *     k <= min(iterations, hist_capacity - 1).  The stop is relative: sqrt(rr) <= tol * sqrt(bb), on the recursive residual.
 *   - The host enqueues pcg_check_every iterations (knob, default 8), then reads the device state once.  Every kernel that
 *     writes x, r, p, k, hist or a scalar reads the state first and does nothing after the stop, so the knob changes
 *     launches and readbacks, never a returned bit; so does pcg_fuse (0: the dots' first level is fused into the kernels
 *     that produce the vectors | 1: every vector operation and every dot a launch of its own).
 * stats (may be NULL): see the struct.  result (may be NULL): shape0 = shape1 = n, nnz_a = |S|, nnz_b = |F|, ms_consolidate
 * (the intake of A and M), ms_symbolic (row forms, diagonal, schedules, bb and the first residual), ms_numeric (the
 * iterations), ms_total, workspace_bytes; everything else 0 / NULL.
 * SPSAMD_EINVAL, with a message and x untouched: A NULL; b or x NULL while n > 0; tol negative, NaN or Inf; M non-NULL
 * without PRECOND_LU or NULL with it; precond, mem or a policy out of range; the overlaps above; an index out of bounds; a
 * false sort0; 2^31 or more tuples.  n == 0 returns 0 with iterations = 0, reason = CONVERGED and hist[0] = +0.0.  Returns
 * when x is complete.
 */
#define SPSAMD_PRECOND_NONE   0   /* z = r */
#define SPSAMD_PRECOND_JACOBI 1   /* z_i = r_i / d_i, d the DIAG fold of spsamd_reduce over S (a true division) */
#define SPSAMD_PRECOND_LU     2   /* z = solve_tri(F, UPPER, NONUNIT, solve_tri(F, LOWER, UNIT, r)); F = the operand M */

#define SPSAMD_PCG_CONVERGED  0
#define SPSAMD_PCG_MAXITER    1
#define SPSAMD_PCG_BREAKDOWN  2

typedef struct {
	uint64_t iterations;       /* k at the stop */
	int32_t  reason;           /* SPSAMD_PCG_* */
	double   bb, rr0, rr;      /* dot(b,b), dot(r,r) before the first and after the last iteration */
	uint64_t launches;         /* kernel launches (and fills) of the iteration phase, those enqueued after the stop included */
	uint64_t readbacks;        /* host reads of the device state during the iteration phase */
	uint32_t analyses;         /* level schedules built by this call (0 .. 2) */
	float ms_setup, ms_iterate;
} spsamd_pcg_stats;

int spsamd_solve_pcg(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int precond, const spsamd_coo *M /* PRECOND_LU only, else NULL */, char transpose_M,
	const double *b, double *x /* in: x0, out: the iterate at the stop */, int mem,
	double tol, uint64_t max_iter,
	double *hist_host /* may be NULL */, size_t hist_capacity,
	int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * Solve op(A) x = b for an unsymmetric op(A) by right-preconditioned BiCGStab with rhat = r0, one right-hand side, the whole
 * loop on the device.  Everything around the loop is spsamd_solve_pcg's and is not restated: the
 * operands and their intake (S of A, F of M), b, x and mem, the overlap rules, the three preconditioners, dot, fold,
 * q = A p, M^-1, usable, the NaN and rounding rules, hist_host, stats (the same struct and SPSAMD_PCG_* reasons), result,
 * the SPSAMD_EINVAL / SPSAMD_EDIM cases with x untouched, n == 0, and the meaning of the knobs pcg_check_every and pcg_fuse.
 * Every value returned -- x, hist, iterations, reason, bb, rr0, rr -- is defined by this loop, bit for bit:
 *
 *       bb = dot(b, b);  thresh = (tol * tol) * bb
 *       q = A x;  r_i = b_i - q_i;  rhat = r;  rr = dot(r, r);  rho' = rr;  k = 0;  hist[0] = rr;  rr0 = rr
 *       loop:
 *           if rr <= thresh:                  stop CONVERGED          (a NaN compares false)
 *           if k == max_iter:                 stop MAXITER
 *           if not usable(rho'):              stop BREAKDOWN
 *           if k == 0:  p = r
 *           else:       if not usable(omega): stop BREAKDOWN
 *                       beta = (rho' / rho) * (alpha / omega);   p_i = r_i + beta * (p_i - omega * v_i)
 *           rho = rho'
 *           y = M^-1 p;  v = A y;  rv = dot(rhat, v)
 *           if not usable(rv):                stop BREAKDOWN
 *           alpha = rho / rv
 *           s_i = r_i - alpha * v_i;  ss = dot(s, s)
 *           if ss <= thresh:                  x_i = x_i + alpha * y_i;  rr = ss;  k = k + 1;  hist[k] = rr;  stop CONVERGED
 *           z = M^-1 s;  t = A z;  ts = dot(t, s);  tt = dot(t, t)
 *           if not usable(tt):                stop BREAKDOWN
 *           omega = ts / tt
 *           x_i = (x_i + alpha * y_i) + omega * z_i;   r_i = s_i - omega * t_i
 *           rr = dot(r, r);  rho' = dot(rhat, r);  k = k + 1;  hist[k] = rr
 *
 *   - At k = 0 dot(rhat, r) is dot(r, r) term for term: rho' has the bits of rr0 and is not computed.
 *   - At a BREAKDOWN inside an iteration x, rr and k are those after k whole iterations.
 *   - The half-step exit is part of the definition: a system solved exactly at the half step (a diagonal A under Jacobi, at
 *     k = 1) would otherwise end in 0 / 0.  An iteration that ends there counts as one, and applies M^-1 and A once.
 *   - Under SPSAMD_PRECOND_NONE y is p and z is s.
 * Returns when x is complete.
 */
int spsamd_solve_bicgstab(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int precond, const spsamd_coo *M /* PRECOND_LU only, else NULL */, char transpose_M,
	const double *b, double *x /* in: x0, out: the iterate at the stop */, int mem,
	double tol, uint64_t max_iter,
	double *hist_host /* may be NULL */, size_t hist_capacity,
	int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * Solve op(A) x = b for an unsymmetric op(A) by right-preconditioned restarted GMRES(m), m = restart, one right-hand side,
 * the whole loop on the device.  Everything around the loop is spsamd_solve_pcg's and is not restated:
 * the operands and their intake (S of A, F of M), b, x and mem, the overlap rules, the three preconditioners, dot, fold,
 * q = A p, M^-1, usable, the NaN and rounding rules (no FMA, true divisions), hist_host, stats (the same struct and
 * SPSAMD_PCG_* reasons), result, the SPSAMD_EINVAL / SPSAMD_EDIM cases with x untouched, and n == 0.  One more
 * SPSAMD_EINVAL: restart == 0 or restart > SPSAMD_GMRES_MAX_RESTART.  stats->iterations counts Arnoldi steps, and
 * stats->readbacks - 1 is the number of cycles.  Square roots are correctly rounded IEEE square roots with spsamd_reduce's
 * rules for a NaN, a negative operand and -0.0.  The Arnoldi step is classical Gram-Schmidt done twice, the Hessenberg
 * matrix is kept triangular by Givens rotations.  Every value returned -- x, hist, iterations, reason, bb, rr0, rr -- is
 * defined by this loop, bit for bit; every product, sum and difference is rounded on its own:
 *
 *       bb = dot(b, b);  thresh = (tol * tol) * bb
 *       q = A x;  r_e = b_e - q_e;  rr = dot(r, r);  k = 0;  hist[0] = rr;  rr0 = rr
 *       cycle:
 *           if rr <= thresh:        stop CONVERGED        (a NaN compares false)
 *           if k == max_iter:       stop MAXITER
 *           if not usable(rr):      stop BREAKDOWN
 *           beta = sqrt(rr);  v_0 = r / beta (element by element);  g_0 = beta;  j = 0;  broken = false
 *           step:
 *               z = M^-1 v_j;  w = A z
 *               for i = 0..j:  h_i = dot(v_i, w)                      (all on the same w: classical Gram-Schmidt)
 *               for i = 0..j ascending:  w_e = w_e - h_i * v_i[e]
 *               for i = 0..j:  d_i = dot(v_i, w)                      (the second pass)
 *               for i = 0..j ascending:  w_e = w_e - d_i * v_i[e];   h_i = h_i + d_i
 *               ww = dot(w, w);  hn = sqrt(ww)
 *               for i = 0..j-1:  t = c_i*h_i + s_i*h_{i+1};  h_{i+1} = c_i*h_{i+1} - s_i*h_i;  h_i = t
 *               den = sqrt(h_j*h_j + hn*hn)
 *               if not usable(den):  broken = true;  goto end     (the step is discarded: k and j stay)
 *               c_j = h_j / den;  s_j = hn / den;  R[i][j] = h_i for i < j;  R[j][j] = den
 *               g_{j+1} = -(s_j * g_j);  g_j = c_j * g_j
 *               k = k + 1;  j = j + 1;  est = g_j * g_j;  hist[k] = est
 *               if est <= thresh or j == m or k == max_iter or not usable(ww):
 *                   if ww is NaN or Inf:  broken = true
 *                   goto end
 *               v_j = w / hn (element by element);  goto step
 *           end:
 *               if j > 0:
 *                   for i = j-1 .. 0:  a = g_i;  for l = i+1 .. j-1 ascending:  a = a - R[i][l]*y_l;   y_i = a / R[i][i]
 *                   u_e = +0.0;  for i = 0..j-1 ascending:  u_e = u_e + y_i * v_i[e]
 *                   z = M^-1 u;  x_e = x_e + z_e
 *                   q = A x;  r_e = b_e - q_e;  rr = dot(r, r);  hist[k] = rr       (the true value replaces the estimate)
 *               if broken:  stop BREAKDOWN
 *               goto cycle
 *
 *   - CONVERGED is only ever decided on dot(b - A x, b - A x) of the returned x.
 *   - hist[k] inside a cycle is the Givens estimate of the squared residual norm; at a cycle's last step it is the true value.
 *   - Stagnation (a cycle that does not lower rr) ends in MAXITER.
 *   - Under SPSAMD_PRECOND_NONE z is its input, with no copy.
 *   - An exactly solved system (ww == 0) ends its cycle through est == 0 <= thresh.
 *   - The negation of g_{j+1} flips the sign bit, of a NaN too.
 *   - Between two reads of the device state the host enqueues one whole cycle: min(m, max_iter - k) steps and one cycle
 *     end.  Step kernels after an in-cycle end are idle, the cycle-end kernels run once.  The knobs pcg_check_every and
 *     pcg_fuse are not read by this call; gmres_path changes launches, never a returned bit.
 *   - The workspace holds the m basis vectors v_0 .. v_{m-1} and up to three more vectors of n doubles beside the frame's;
 *     SPSAMD_ENOMEM where that does not fit.  Nothing is allocated inside the loop.
 * Returns when x is complete.
 */
#define SPSAMD_GMRES_MAX_RESTART 256
int spsamd_solve_gmres(spsamd_ctx *ctx, const spsamd_coo *A, char transpose,
	int precond, const spsamd_coo *M /* PRECOND_LU only, else NULL */, char transpose_M,
	const double *b, double *x /* in: x0, out: the iterate at the stop */, int mem,
	double tol, uint64_t max_iter, uint32_t restart,
	double *hist_host /* may be NULL */, size_t hist_capacity,
	int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats /* may be NULL */, spsamd_result *result /* may be NULL */);

/*
 * One multigrid V-cycle over a hierarchy of the caller's, on the device, and spsamd_solve_pcg's loop with that cycle as its
 * preconditioner.  The set-up pieces are public calls of their own: spsamd_aggregate and its
 * tentative prolongator P, the Galerkin operator P^T (A P) by two spsamd_multiply calls; a smoothed P comes from
 * spsamd_add, spsamd_reduce and spsamd_multiply and goes through here unchanged.
 *   - Levels.  levels[l], l = 0 .. nlevels - 1 (1 <= nlevels <= 32), holds the level operator op(A_l), n_l x n_l, and below
 *     the last level the prolongation op(P_l), n_l x n_{l+1}, and the restriction op(R_l), n_{l+1} x n_l; on the last level
 *     P and R are NULL.  P and R are separate operands: the tentative prolongator is passed twice, as P with '.' and as R
 *     with 'T'.  The cycle is defined for any operands of these shapes.  A SYMMETRIC preconditioner -- what conjugate
 *     gradients need -- is the caller's responsibility: R_l = P_l^T and pre == post.
 *   - Every operand is taken exactly as spsamd_solve_pcg takes A, duplicate_policy and zero_nan included: a raw operand is
 *     consolidated by op()'s rows, an operand whose sort0 names op()'s row order is trusted, a SINK_COO result of this
 *     context and a prepared handle of the same transpose are read in place.  Call the sequences S_l, P_l, R_l.  The call
 *     keeps nothing: prepared handles make the intake free.  Neither output set of the context is written.
 *   - Every returned bit is defined by this loop.  Products, sums and divisions are each rounded once, with no FMA; a NaN
 *     result carries the bits x86-64 gives it (the rules of spsamd_solve_pcg above).
 *       d_l            = the DIAG fold of spsamd_reduce over S_l (+0.0 without a diagonal tuple)
 *       apply(X, v)_i  = acc after  acc = +0.0;  acc = acc + val * v_j  over row i's tuples (i, j, val) of X in X's order
 *       smooth0(l, b)  : x_i = omega * (b_i / d_i)
 *       smooth(l, b, x): q = apply(S_l, x);  x'_i = x_i + omega * ((b_i - q_i) / d_i)    for all i from the old x (Jacobi)
 *
 *       cycle(l, b):
 *           if l == nlevels - 1:
 *               x = +0.0;  sweep s = 0 .. coarse-1:  x = (s == 0 ? smooth0(l, b) : smooth(l, b, x));  return x
 *           x = +0.0;      sweep s = 0 .. pre-1:     x = (s == 0 ? smooth0(l, b) : smooth(l, b, x))
 *           r = (pre == 0 ? b : b - apply(S_l, x))                   (r_i = b_i - q_i)
 *           e = cycle(l + 1, apply(R_l, r))
 *           x_i = x_i + apply(P_l, e)_i
 *           sweep s = 0 .. post-1:  x = smooth(l, b, x)
 *           return x
 *     Nothing is checked for a zero or a missing diagonal: the infinities and NaNs go where IEEE sends them (and the loop of
 *     conjugate gradients then stops with BREAKDOWN).  A level below the first may have order 0: the correction of the level
 *     above is then a vector of +0.0 (which is still added: a -0.0 becomes +0.0).
 *   - spsamd_amg_apply:  x = cycle(0, b).  b and x are n_0 doubles in `mem` (SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE, for both);
 *     x is written only.
 *   - spsamd_solve_pcg_amg: the loop of spsamd_solve_pcg's header with A = levels[0].A (and its transpose flag) and
 *     z = cycle(0, r): the same fold, stop reasons, hist, stats, and the same meaning of pcg_check_every and pcg_fuse.
 *   - The levels from the first one on from which no level has more than amg_fuse_rows rows (knob, default 1024) are the
 *     fused tail: one launch of one workgroup walks them down and up.  amg_path = 1 turns the tail off, amg_path = 2 makes
 *     the whole hierarchy the tail.  Rows above spmm_long_min of a level outside the tail go to the wave kernel of
 *     spsamd_multiply_dense.  Every row is one serial chain in the operand's order on every path: no knob changes a
 *     returned bit.  Nothing is allocated inside a cycle; workspace_bytes does not depend on the iteration count.
 * amg_stats (may be NULL): see the struct.  result (may be NULL): as spsamd_solve_pcg fills it (nnz_a = |S_0|, nnz_b = 0);
 * for spsamd_amg_apply shape0 = shape1 = n_0, nnz_a = |S_0|, ms_symbolic (the intake and set-up), ms_numeric (the cycle),
 * ms_total, workspace_bytes.
 * SPSAMD_EINVAL, with a message and x untouched: levels, params or a level's A NULL; b or x NULL while n_0 > 0; nlevels
 * outside 1 .. 32; P or R missing below the last level, or present on it; omega not finite; and, applied to every operand,
 * the overlap, mem, policy, tol and 2^31 rules of spsamd_solve_pcg.  SPSAMD_EDIM: a level operator that is not square, or
 * P / R shapes that do not chain n_l -> n_{l+1}.  n_0 == 0 returns as spsamd_solve_pcg does.  Returns when x is complete.
 */
typedef struct {
	const spsamd_coo *A; char transpose_A;   /* level operator, op(A_l): n_l x n_l                              */
	const spsamd_coo *P; char transpose_P;   /* prolongation,  op(P_l): n_l x n_{l+1};  NULL on the last level  */
	const spsamd_coo *R; char transpose_R;   /* restriction,   op(R_l): n_{l+1} x n_l;  NULL on the last level  */
} spsamd_amg_level;

typedef struct { uint32_t pre, post, coarse; double omega; } spsamd_amg_params;

typedef struct {
	uint32_t levels;              /* nlevels */
	uint32_t fused_levels;        /* levels served inside the fused tail */
	uint64_t launches_per_cycle;  /* kernel launches (and fills) one cycle enqueues */
	uint64_t rows[32], nnz[32];   /* n_l and |S_l| */
	double operator_complexity;   /* sum of |S_l| over |S_0| (0 where S_0 is empty) */
	uint64_t long_rows;           /* rows sent to the wave kernel, over the operands of all levels outside the tail */
	float ms_setup, ms_cycle;     /* spsamd_amg_apply only */
} spsamd_amg_stats;

int spsamd_amg_apply(spsamd_ctx *ctx, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params,
	const double *b, double *x /* out */, int mem, int duplicate_policy, int zero_nan,
	spsamd_amg_stats *amg_stats /* may be NULL */, spsamd_result *result /* may be NULL */);

int spsamd_solve_pcg_amg(spsamd_ctx *ctx, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params,
	const double *b, double *x /* in: x0, out: the iterate at the stop */, int mem,
	double tol, uint64_t max_iter,
	double *hist_host /* may be NULL */, size_t hist_capacity,
	int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats /* may be NULL */, spsamd_amg_stats *amg_stats /* may be NULL */,
	spsamd_result *result /* may be NULL */);

/*
 * ret = (C * diag(scalei) * op(A) * diag(scalej) * op(B) * diag(scalek)) restricted to the keys of M  -- a masked product
 * (SDDMM-style sampling of a sparse product: (L*L) o L counts triangles).  The result is exactly those tuples of
 *     spsparse::multiply(ret, C, scalei, A, transpose_A, scalej, B, transpose_B, scalek, duplicate_policy, zero_nan)
 * whose key (i, j) is a key of M, in ascending (i, j), bit for bit (NaN payloads included) -- the reference being the
 * inner-product loop of multiply_sparse.hpp:192-243 (the test oracle's orc_multiply_mm / orc_multiply_mm_rowwise), run
 * over M's keys only:
 *   - op(A) is consolidated by rows, op(B) by its columns (:187-188), with duplicate_policy and zero_nan.
 *   - a row, column or k whose scale entry is missing or zero (isnone) is skipped (:195, :211, the join3 over scalej).
 *   - sum starts at 0 and adds the products of the matched k in ascending k, serially, no FMA: a * b, or (a * sj) * b under
 *     scalej; a NaN product or sum has the bits x86-64 gives it.
 *   - the tuple is emitted when the PRE-scale sum is not 0 (:238): a NaN sum is emitted, and so is a sum that the scales
 *     then turn into 0.0.  Its value is sum * C * a_scale * b_scale, left to right (a missing scale vector counts 1).
 *   - C == 0, an empty scale vector, an empty operand (:178-184) or an empty M: an empty result of the product's shape.
 * M is structural: its shape must be rows(op(A)) x cols(op(B)) (SPSAMD_EDIM otherwise; M has no transpose flag, it is
 * given in C's orientation); M->val is never read and may be NULL; duplicate keys count once and explicit zeros count.  M
 * may be host, device, a chained SINK_COO result of this context, or prepared (SPSAMD_MEM_PREPARED: its consolidated
 * tuples; prepared for 'T', it is read as a device operand sorted the other way).  sort0 == 0 only lets the call skip the
 * sort: keys that are not actually ascending are rejected.  SPSAMD_EINVAL: M NULL, an index of M out of bounds, a false
 * sort0 == 0, nnz(M) >= 2^31, a policy outside 0..2, both output buffers of the context operands of the call (A, B and M
 * count), and every check spsamd_multiply makes.
 * Sinks: SINK_COO (row-major tuples in the context's output set, fetchable, usable with spsamd_result_scatter_dense,
 * chainable as a MEM_DEVICE sort0 = 0 operand -- sort0 = 1 with SINK_PERMUTE, which swaps the index arrays), SINK_DIGEST
 * (+ ROWSTATS over rows(op(A))); SINK_ORDERED and SINK_EXACT_PATTERN are accepted and change nothing.
 * result: shape, nnz, nnz_a / nnz_b (the consolidated operands), products (the matched and summed k over all evaluated
 * keys), ms_consolidate, ms_numeric, ms_total, workspace_bytes; the other fields are 0.  Returns when the result is
 * complete.  The work is proportional to the keys of M and the lengths of their rows of op(A) and columns of op(B), not to
 * the whole product.
 */
int spsamd_multiply_masked(spsamd_ctx *ctx, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, const spsamd_coo *M,
	int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *result);

/*
 * The product of spsamd_multiply, delivered to the host in row blocks while it is computed: the whole of C never sits in
 * device memory at once, so a product larger than the device can still reach a host accumulator.
 *   Tuples  cb receives consecutive chunks, each of at least one tuple, in ascending (i, j) order over the whole product.
 *           Concatenated they are what spsamd_multiply(..., SPSAMD_SINK_COO, sink_flags) followed by
 *           spsamd_result_fetch delivers: bit for bit (NaN payloads included) under SPSAMD_SINK_ORDERED; under
 *           SINK_EXACT_PATTERN and flags 0 by the same rules as spsamd_multiply with those flags.  SINK_PERMUTE gives
 *           (j, i, v) in C's row order; SINK_ROWSTATS is refused (SPSAMD_EINVAL).  The callback contract is
 *           spsamd_result_fetch's: host pointers valid during the call, j never NULL.  A non-zero return stops the
 *           delivery; the call returns that value once no work of the call is still running on the device.  cb is called
 *           on the calling thread.
 *   Blocks  Over the consolidated op(A) and op(B) (after the policy and zero_nan), P_r = the sum of len_op(B)(k) over the
 *           tuples (r, k) of op(A), and bound_r = min(P_r, cols(op(B))) (scale vectors ignored: still an upper bound of
 *           the row's tuples).  The blocks are the maximal runs of consecutive rows (from row 0, empty rows included)
 *           whose bounds sum to at most block_tuples: a block ends where the next row would take the sum over it.
 *           stats->blocks is their count.  A bound_r > block_tuples fails with SPSAMD_ECAPACITY before anything is
 *           delivered; the message names the smallest budget that works (the largest bound_r).
 *           block_tuples == 0: SPSAMD_STREAM_DEFAULT_BLOCK (2^30 tuples, 16 GiB per block output set).
 *   Memory  At most two blocks' outputs exist at once, each sized to its block's bound sum at 16 bytes per tuple:
 *           device_output_bytes <= 2 * 16 * block_tuples plus the rounding of six allocations to 256 bytes, whatever
 *           nnz(C) is.  The workspace (context arena) and the operands' derived structures come on top, as for
 *           spsamd_multiply.  Pinned host staging: two chunks of at most 2^22 tuples, 128 MiB, kept by the context.
 *   Errors  Every check spsamd_multiply makes (SPSAMD_EDIM, an index out of bounds, an unsorted scale vector, a bad
 *           policy) fails before cb is first called.  A failure after chunks were delivered returns its code, and the
 *           context stays usable.
 *   Context Neither output set of the context is written: a chained operand (an earlier SINK_COO result) is read in
 *           place and keeps its tuples; treat any other SINK_COO result of the context as invalid after the call.
 *           Any call on the same context from inside cb (spsamd_ctx_set_tuning included) returns SPSAMD_EINVAL
 *           ("context busy").  Prepared operands (SPSAMD_MEM_PREPARED) are accepted; a handle the call uses must outlive
 *           it (spsamd_operand_destroy on it from inside cb is undefined).
 *   Columns A product spsamd_multiply would compute by column blocks of op(B) (a row of more than 4096 products and
 *           more than 2^25 columns, or window indices over the budget -- index_budget_mb) is refused with
 *           SPSAMD_EINVAL before any delivery.  The test is conservative: it uses P_r without the scale vectors.
 * result gets the totals: shape, nnz, products, nnz_a / nnz_b, rows / products / tuples / cells by class, the stage times
 * summed over the blocks, ms_consolidate, ms_total (the call's device time), workspace_bytes; idx0, idx1 and val are NULL.
 * stats (may be NULL) gets the figures of the blocking.
 */
#define SPSAMD_STREAM_DEFAULT_BLOCK ((size_t)1 << 30)
typedef struct {
	uint64_t blocks;              /* row blocks the product was cut into */
	uint64_t block_tuples;        /* the budget in effect (after the default was applied) */
	uint64_t max_block_nnz;       /* largest block actually produced */
	uint64_t device_output_bytes; /* peak device bytes held for block outputs during the call */
	float ms_device;              /* sum of the blocks' device times (HIP events) */
	float ms_callback;            /* host time spent inside cb */
	float ms_wall;                /* whole call */
} spsamd_stream_stats;

int spsamd_multiply_stream(spsamd_ctx *ctx, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_flags, size_t block_tuples,
	spsamd_chunk_fn cb, void *user,
	spsamd_result *result, spsamd_stream_stats *stats);

/* Copy `bytes` between host and/or device memory of this context's device
 * (e.g. result->row_nnz to the host, result->idx0 into a caller's device
 * buffer), ordered after everything queued on the context's stream; returns
 * when the copy is complete. */
int spsamd_memcpy(spsamd_ctx *ctx, void *dst, const void *src, size_t bytes);

/*
 * Stand-alone consolidate (algorithm.hpp:251-319) of a COO matrix on the
 * device: stable sort by sort_order {so0, 1-so0}, zeros dropped, duplicates
 * merged by policy.  Output tuples land in the context's output buffer
 * (result->idx0/idx1/val, nnz); fetch them with spsamd_result_fetch.
 */
int spsamd_consolidate(spsamd_ctx *ctx, const spsamd_coo *A, int so0,
	int duplicate_policy, int zero_nan, spsamd_result *result);

/*
 * sorted_permutation (algorithm.hpp:411-427): the stable permutation that sorts
 * the tuples of A by sort_order {so0, 1-so0}; perm_host receives A->nnz entries.
 * Pinned by tests/test_array.cpp:67-79.
 */
int spsamd_sorted_permutation(spsamd_ctx *ctx, const spsamd_coo *A, int so0, uint64_t *perm_host);

/*
 * dim_beginnings (algorithm.hpp:74-118): offsets at which the leading sorted
 * index changes, plus the end sentinel -- only non-empty rows appear.  A must
 * carry sort0 == so0 (the reference raises "dim_beginnings() required the
 * VectorCooArray is sorted first." otherwise, algorithm.hpp:82-84).
 * beginnings_host needs room for nnz + 1 entries; *count receives the number
 * written (0 for an empty array).  Pinned by tests/test_array.cpp:146-166.
 */
int spsamd_dim_beginnings(spsamd_ctx *ctx, const spsamd_coo *A, int so0, uint64_t *beginnings_host, size_t *count);

/* ---- prepared operands ----
 * What a multiply derives from an operand before it starts -- the consolidated tuples, the row structure, the
 * (col, val)-interleaved copy and, for products with heavy rows, the column-window indices of the right operand -- kept
 * in device memory so that it is derived ONCE for an operand that takes part in many products.  The reference does the
 * same on the host: an array that carries the wanted sort_order is not consolidated again (Consolidate<>,
 * algorithm.hpp:360) and its row structure is cached inside the object (VectorCooArray.hpp:325-335).
 *   role       SPSAMD_AS_A, SPSAMD_AS_B or both: the side(s) of multiply the operand will stand on
 *   transpose  the transpose flag it will be passed with
 *   duplicate_policy, zero_nan: as for multiply; they are applied HERE, once (a multiply takes a prepared operand as it
 *              is, the way Consolidate<> takes a sorted one)
 * spsamd_operand_as_coo fills a spsamd_coo (mem = SPSAMD_MEM_PREPARED) that is accepted wherever an operand is; results
 * are identical to those of the plain operand.  A handle belongs to the context that prepared it and is immutable; the
 * structures only heavy rows need are built by the first multiply that needs them and stay (not re-entrant on one
 * handle from two threads, like the reference's lazy cache).  Used with the other transpose flag than it was prepared
 * for, the handle is read as an ordinary device operand sorted the other way (and consolidated by that call). */
#define SPSAMD_MEM_PREPARED 2
#define SPSAMD_AS_A 1
#define SPSAMD_AS_B 2
typedef struct spsamd_operand spsamd_operand;
int spsamd_operand_prepare(spsamd_ctx *ctx, const spsamd_coo *X, char transpose, int role, int duplicate_policy, int zero_nan,
	spsamd_operand **out);
int spsamd_operand_as_coo(const spsamd_operand *op, spsamd_coo *out);
uint64_t spsamd_operand_bytes(const spsamd_operand *op);     /* device memory the handle holds right now */
void spsamd_operand_destroy(spsamd_operand *op);

/* ---- multi-GPU: op(A) sharded by contiguous row blocks, one rank per GPU ----
 * The reference has no counterpart.  Output row i depends only on row i of op(A) and the op(B) rows
 * {k : op(A)(i,k) != 0} (the reference's own loop structure, multiply_sparse.hpp:192): every rank multiplies its row
 * block of op(A) with the panel of op(B) rows it needs, fetched with ONE exchange step (grouped ncclSend / ncclRecv over
 * RCCL: the all-to-allv of needed B row panels); C stays row partitioned, there is no reduction.
 */
typedef struct spsamd_dist spsamd_dist;

/* Optional transport replacing the built-in RCCL one (tests: gloo / MPI through host memory).  All-to-allv of
 * device buffers: send[p] (sendbytes[p] bytes) goes to rank p, recvbytes[p] bytes from rank p arrive in recv[p].
 * The buffers are complete when it is called and must be complete when it returns.  A step calls it several times
 * (once per kind of payload); every rank makes the same sequence of calls. */
typedef int (*spsamd_alltoallv_fn)(void *user, const void *const *send, const size_t *sendbytes,
	void *const *recv, const size_t *recvbytes, int world, void *hip_stream);

typedef struct {
	uint64_t block_nnz_a;         /* consolidated tuples of this rank's A block */
	uint64_t panel_tuples;        /* tuples of the B panel this rank multiplied with */
	uint64_t remote_tuples;       /* ... of which received from other ranks */
	uint64_t sent_tuples;         /* tuples this rank sent to other ranks */
	float ms_exchange;            /* consolidation of the blocks + both exchange rounds up to the issue of the panel transfer
	                               * (HIP events; the transfer itself overlaps the product's symbolic phase) */
	float pad_;
} spsamd_dist_stats;

/* 128 bytes identifying a new RCCL communicator (ncclGetUniqueId): call on one rank, hand to all (MPI, a file,
 * torch.distributed ...), then spsamd_dist_create(..., unique_id, ...) on every rank. */
int spsamd_dist_unique_id(char id[128]);
/* One of: unique_id (the library creates its communicator with ncclCommInitRank), nccl_comm (an ncclComm_t of
 * the caller, borrowed), or transport (+ transport_user).  ctx: this rank's context (its device and stream).
 * At most 64 ranks. */
int spsamd_dist_create(spsamd_dist **out, spsamd_ctx *ctx, int rank, int world, const char *unique_id,
	void *nccl_comm, spsamd_alltoallv_fn transport, void *transport_user);
void spsamd_dist_destroy(spsamd_dist *d);
/*
 * One step: this rank's rows of  C * diag(scalei) * op(A) * diag(scalej) * op(B) * diag(scalek)  -- the arguments of
 * spsparse::multiply (multiply_sparse.hpp:138-150) with the two matrices given block-wise:
 *   A_block  the tuples of A that belong to this rank's rows of op(A) -- raw COO with GLOBAL indices, shape = the whole
 *            matrix's, in their original relative order (which rows a rank owns is the caller's choice: any partition).
 *   B_block  the tuples of B whose op(B) ROW -- the inner index: idx0 without 'T', idx1 with it -- lies in
 *            [b_bounds[rank], b_bounds[rank+1]); or NULL where B is A with the same transpose flag and the A blocks
 *            are cut at b_bounds too (A * A: the own A block then is the own B block).
 *   b_bounds world + 1 ascending boundaries of op(B)'s distribution over the inner dimension (0 .. inner), the same on
 *            every rank.
 *   scale vectors: whole, the same on every rank.  zero_nan: the NaNs dropped are those of the leading run of the WHOLE
 *            matrix' sorted sequence, as in the reference (algorithm.hpp:272-275): the ranks agree on it first.
 * The result is this rank's rows of C in the sink of its context (digest: add the counts / hashes / sums of all ranks;
 * COO: tuples with global indices, chainable as the A_block of the next step: T = R*A, then C = T*R^T).
 * Collective: every rank of the communicator must call it, with the same shapes, bounds, flags and policies.  A rank
 * whose own operands are bad (index out of bounds, a B_block tuple outside its bounds ...) still takes part in the first
 * exchange round, which carries every rank's status: then EVERY rank returns an error -- its own, or SPSAMD_EPEER -- and
 * the communicator stays usable.  A failure after that round (out of memory, a HIP / RCCL error) cannot be agreed on any
 * more: the communicator refuses further steps (SPSAMD_EPEER); destroy it and create a new one.
 */
int spsamd_dist_multiply(spsamd_dist *d, double C,
	const spsamd_vec *scalei,
	const spsamd_coo *A_block, char transpose_A,
	const spsamd_vec *scalej,
	const spsamd_coo *B_block, char transpose_B,
	const spsamd_vec *scalek,
	const uint64_t *b_bounds,
	int duplicate_policy, int zero_nan, int sink_kind, int sink_flags,
	spsamd_result *result, spsamd_dist_stats *stats);

/* ---- synthetic operands generated on the device (bench / tests) ----
 * Bit-identical to spsparse_amd/workloads.py.  Outputs are device arrays
 * owned by the caller (capacity >= the generator's tuple count). */
int spsamd_gen_rmat(spsamd_ctx *ctx, int scale, int edge_factor, uint64_t seed,
	uint64_t first_edge, uint64_t n_edges, int32_t *idx0, int32_t *idx1, double *val);
int spsamd_gen_random_rows(spsamd_ctx *ctx, uint64_t n, uint64_t per_row, uint64_t seed,
	uint64_t stream_base, int32_t *idx0, int32_t *idx1, double *val);
/* 5-point Poisson on an N x N grid: writes 5N^2-4N tuples, row-major sorted */
int spsamd_gen_poisson2d(spsamd_ctx *ctx, uint64_t N, int32_t *idx0, int32_t *idx1, double *val);
/* 7-point Laplacian on an N^3 grid: writes 7N^3-6N^2 tuples, row-major sorted */
int spsamd_gen_laplace3d(spsamd_ctx *ctx, uint64_t N, int32_t *idx0, int32_t *idx1, double *val);
/* 2x2x2 piecewise-constant aggregation, (N/2)^3 x N^3: writes N^3 tuples */
int spsamd_gen_aggregation3d(spsamd_ctx *ctx, uint64_t N, int32_t *idx0, int32_t *idx1, double *val);

#ifdef __cplusplus
}
#endif
#endif
