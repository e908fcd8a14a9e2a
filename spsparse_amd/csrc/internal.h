// internal.h -- shared declarations of the spsparse_amd HIP library (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

#include "../../include/spsparse_amd.h"

namespace spsamd {

// ---------------------------------------------------------------- errors

struct Error {
	int code;
	std::string msg;
};

#define SPS_HIP(call)                                                              \
	do {                                                                           \
		hipError_t e_ = (call);                                                    \
		if (e_ != hipSuccess)                                                      \
			throw ::spsamd::Error{SPSAMD_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)}; \
	} while (0)

#define SPS_LAUNCH_CHECK() SPS_HIP(hipGetLastError())

// ---------------------------------------------------------------- workspace

// Bump allocator over device slabs.  A multiply carves everything it needs
// from here; if the first slab was too small extra slabs are chained and the
// arena is re-made as one slab of the high-water size at the next reset, so a
// steady-state call does no hipMalloc.
struct Arena {
	struct Slab { char *p; size_t cap; size_t used; };
	std::vector<Slab> slabs;
	size_t high_water = 0;
	size_t call_used = 0;

	void *alloc(size_t bytes);
	// Stack discipline inside a call: everything allocated after mark() is given back by rewind().
	struct Mark { size_t nslabs, used, call_used; };
	Mark mark() const { return Mark{slabs.size(), slabs.empty() ? 0 : slabs.back().used, call_used}; }
	void rewind(const Mark &m);
	void reset();          // start of a call
	void release();        // free everything
	void reserve(size_t bytes);
	template <class T> T *get(size_t n) { return (T *)alloc(n * sizeof(T)); }
};

// Grow-only device buffer (the context's output buffer, host staging).
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	void ensure(size_t bytes);
	void release();
	bool holds(const void *q) const { return p && q && (const char *)q >= (const char *)p && (const char *)q < (const char *)p + cap; }
};

// One set of SINK_COO / consolidate output arrays.  A context has two: a result handed back as a
// device operand of the next call (T = R*A, then C = T*R^T: accum.hpp:73-101's use case) is read
// in place while the new result goes to the other set.
struct OutSet {
	DevBuf i, j, v;
	bool holds(const void *q) const { return i.holds(q) || j.holds(q) || v.holds(q); }
	void release() { i.release(); j.release(); v.release(); }
};

// Developer knobs of one context.  Read from the environment ONCE, at spsamd_ctx_create (one SPSAMD_* variable per knob:
// the `knobs` / `envs` table there, capi.hip), or set through spsamd_ctx_set_tuning; results are identical for every setting.
struct Tuning {
	int window = 0;              // 0: chosen from the column count; 8192 / 16384
	int cell_cap = 0;            // 0: default grouping target of the hash cells
	int dense_min = 0;           // 0: default threshold above which a window becomes a dense cell
	int no_tiles = 0;
	int xcd = 2;                     // 0: one list for all XCDs | 1: every cell list in eight static parts (experiment, slower) | 2: the dense cells' list in eight parts, claimed
	int emit_path = 0;           // 0 auto | 1 no bitmap rank | 2 bitonic only
	int light_path = 0;          // 0 auto | 1 generic k_light only
	int light_two_pass = 0;      // 1: the all-light COO sink counts, scans and stores (two compute passes) instead of one pass + gather
	int no_wmajor = 0;           // 1: dense cells read the row-major B through bwin (no window-major copy)
	int tiles_v1 = 0;            // tile kernel of the hash-class cells: 0 auto, 1 first generation, 2 hash tiles v2, 3 bitmap rank
	int long_cap = 0;            // 0: cell_cap; grouping target of the hash cells of rows too long for tiles (<= 4096)
	int long_dense_min = 0;      // 0: default (1024 with 8192-column windows, else dense_min); dense threshold of the rows too long for tiles
	int few_max = 0;             // 0: default (8); mid rows of at most this many A tuples (<= 16) run in k_few | -1: none, every mid row in k_hash
	int direct_min = 0;          // 0: default; products above which one window of a tile row becomes a direct cell (>= dense_min: never)
	int trace = 0;               // 1: the symbolic phase prints its choices to stderr
	int index_budget_mb = 0;     // 0: 80 % of the free device memory; cap (MB) of the heavy rows' window indices, beyond which the product goes by column blocks
	int spmm_path = 0;           // multiply_dense: 0 auto | 1 serial kernel for every row | 2 lanes kernel for every row | 3 fold kernel for every row
	int spmm_long_min = 0;       // multiply_dense, auto: rows of more tuples than this go to a wave kernel (0: 64)
	int add_path = 0;            // add: 0 auto | 1 sort every operand (ignore sort0, chained results and preparation)
	int masked_path = 0;         // multiply_masked: 0 auto | 1 entry kernel for every key | 2 row kernel wherever A_i fits LDS | 3 wave kernel for every key
	int sampled_path = 0;        // multiply_sampled: 0 auto | 1 lane kernel for every tuple | 2 slab kernel for every tuple (auto: by k and a probe of M's order)
	int select_path = 0;         // select, ROW_TOPK: 0 by row length | 1 light | 2 mid | 3 heavy kernel for every row it can hold
	int extract_path = 0;        // extract: 0 auto | 1 every row through the permuted path | 2 light | 3 mid | 4 heavy ordering kernel for every row it can hold
	int reduce_path = 0;         // reduce: 0 by row length | 1 every row through the short rows' kernel | 2 every row through the long rows' kernel
	int tile_walk = 0;           // tiles of the heavy rows: 0 claimed from a counter | 1 the static grid-stride walk
	int emult_path = 0;          // emult: 0 by a byte model | 1 merge | 2 every tuple of op(A) probes op(B) | 3 every key of op(B) probes op(A)
	int solve_path = 0;          // solve_tri: 0 thin levels fuse | 1 every level a launch of its own | 2 every level of short rows fuses, whatever its width
	int solve_row = 0;           // solve_tri: 0 by row length (spmm_long_min) | 1 serial | 2 lanes | 3 fold kernel for every row
	int solve_fuse_rows = 0;     // solve_tri: the widest level that still counts as thin (0: 256 rows and 2048 (row, rhs) pairs)
	int factor_path = 0;         // factor_ilu0: 0 thin levels fuse | 1 every level in launches of its own | 2 every level of serial-class rows fuses, whatever its width
	int factor_row = 0;          // factor_ilu0: 0 by the row's work and length | 1 serial | 2 wave | 3 block kernel for every row it can hold
	int factor_fuse_rows = 0;    // factor_ilu0: the widest level that still counts as thin (0: 256)
	int factor_serial_work = 0;  // factor_ilu0: the most lookups of a serial-class row (0: 64)
	int factor_lds_row = 0;      // factor_ilu0: the longest row of the wave kernel's LDS copy (0: 256; at most 4096)
	int color_path = 0;          // color: 0 the thin tail of the sweep fuses | 1 every round in launches of its own | 2 every round fuses, whatever its width
	int color_row = 0;           // color: 0 by degree | 1 thread | 2 wave kernel for every vertex
	int color_fuse_rows = 0;     // color: the widest worklist that still counts as thin (0: 1024)
	int color_wave_deg = 0;      // color: the largest degree of a thread-class vertex (0: 16)
	int agg_path = 0;            // aggregate: 0 the thin tail of the sweep fuses | 1 every round in launches of its own | 2 every round fuses, whatever its width
	int agg_row = 0;             // aggregate: 0 by degree | 1 thread | 2 wave kernel for every vertex of degree >= 1
	int agg_fuse_rows = 0;       // aggregate: the longest worklist that still counts as thin (0: 1024)
	int agg_wave_deg = 0;        // aggregate: the largest degree of a thread-class vertex (0: 32)
	int agg_per_rows = 0;        // aggregate: the shortest list whose thread kernels take four entries a thread (0: 1024 for every CU)
	int pcg_check_every = 0;     // solve_pcg: iterations enqueued between two reads of the device state (0: 8)
	int pcg_fuse = 0;            // solve_pcg: 0 dots fused into the kernels that produce their vectors | 1 every vector operation and every dot a launch of its own
	int gmres_path = 0;          // solve_gmres: 0 the block kernels of k_gmres.hip | 1 every dot through the frame's dot and every w -= coef v a launch of its own
	int amg_path = 0;            // amg cycle: 0 the thin tail of the hierarchy is one launch | 1 every level in launches of its own | 2 the whole hierarchy is the tail, whatever its levels' orders
	int amg_fuse_rows = 0;       // amg cycle: the largest order of a level that still counts as thin (0: 1024)
#ifdef SPSAMD_ABLATIONS
	int dbg = 0;
#endif
};
}

struct spsamd_ctx {
	int device = 0;
	spsamd::Tuning tune;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	spsamd::Arena arena;
	spsamd::OutSet out[2];                   // SINK_COO results (see OutSet)
	int cur_out = 0;
	// what each output set holds right now, where this library wrote it and knows it to be consolidated by `sort0` with
	// valid indices: handed back as an operand (T = R*A, then C = T*R^T) it is taken as it is, without the inspection pass
	struct OwnResult { const int32_t *d0 = nullptr, *d1 = nullptr; const double *v = nullptr; uint64_t nnz = 0, shape0 = 0, shape1 = 0; int sort0 = -1; } own[2];
	spsamd::DevBuf rowstat_n, rowstat_s, rowstat_h;     // DIGEST row statistics
	void *pinned = nullptr;                  // host staging for small readbacks / fetch
	size_t pinned_cap = 0;
	std::string last_error;
	hipEvent_t ev[10] = {};                  // timing marks of a call, by Ev (below)
	hipEvent_t ev2[3] = {};                  // around the tile launches of the heavy rows, by Ev2
	hipStream_t side = nullptr;              // second stream: the window-major copy of B is built on it beside the rest of the symbolic phase
	hipEvent_t ev_side[2] = {};              // [0] main -> side (inputs ready), [1] side -> main (copy built: waited for just before the dense cells)
	hipStream_t side2 = nullptr;             // third stream: the cell lists are sorted on it beside the light and mid rows' kernels
	hipEvent_t ev_side2[2] = {};             // [0] main -> side2 (cells emitted), [1] side2 -> main (lists sorted: waited for before the heavy rows' kernels)
	bool wm_pending = false, sort_pending = false;   // work of this call still running on side / side2 that the main stream has not waited for yet
	void join_side(bool wm, bool sort);      // make the main stream wait for it (no-op where nothing is pending)
	int num_cu = 256;
	void *host_staging(size_t bytes);
	bool busy = false;                       // a streamed multiply is delivering: every entry point refuses the context
	void *stream_pinned = nullptr;           // the streamed multiply's two chunk buffers (host staging of its own)
	size_t stream_pinned_cap = 0;
};

namespace spsamd {

// While one of these lives, c->stream is a side stream of the context, so that every helper launches there: `which` 0
// the second stream (ev_side, wm_pending), 1 the third (ev_side2, sort_pending).  On entry the side stream waits for the
// fork event [0] -- recorded on the main stream here (`record_fork`), or earlier by the caller -- and the pending flag is
// set; on every way out, an exception included, c->stream is the main stream again and the join event [1] is recorded
// behind what was launched, for spsamd_ctx::join_side.  Nothing else assigns c->stream after spsamd_ctx_create.
struct SideScope {
	SideScope(spsamd_ctx *c, int which, bool record_fork);
	~SideScope();
	SideScope(const SideScope &) = delete;
	SideScope &operator=(const SideScope &) = delete;
private:
	spsamd_ctx *c;
	hipStream_t main, side;
	hipEvent_t join;
};

// What each event of spsamd_ctx::ev marks for the multiply.  The stand-alone operations share 0, 1 and 7 and reuse 2 and
// 3 for stages of their own: k_masked.hip for the begin and end of its numeric kernels, k_stream.hip 2 for its set-up done.
enum Ev {
	EV_NONE = -1,           // (no event: spgemm.hip's launch_pass)
	EV_BEGIN = 0,           // the call begins
	EV_CONSOLIDATED = 1,    // operands consolidated: the symbolic phase begins
	EV_SYMBOLIC = 2,        // symbolic phase done: the numeric phase begins
	EV_N0 = 3,              // numeric marks.  DIGEST: before the light rows | COO: before the COUNT pass
	EV_N1 = 4,              //   DIGEST: light rows done | COO: output grown, before the STORE pass | all rows light: kernels done
	EV_N2 = 5,              //   DIGEST: mid rows done | COO: light and mid rows stored
	EV_N3 = 6,              //   the heavy rows' hash cells done (COO: stored)
	EV_END = 7,             // the call ends (finish_call)
	EV_N4 = 8,              //   the heavy rows' dense cells done (COO: stored)
	EV_FETCH0 = EV_N4, EV_FETCH1 = 9 };     // spsamd_result_fetch, between calls: its two chunks in flight
enum Ev2 { EV2_TILES_BEGIN = 0, EV2_TILES_END = 1, EV2_DIRECT_END = 2 };   // the tiles, then the direct tiles

// ---------------------------------------------------------------- primitives (prims.hip)

// out[i] = sum_{j<i} in[j], out[n] = total (out has n+1 entries).
void scan_exclusive_u32_i64(spsamd_ctx *c, const uint32_t *in, int64_t *out, size_t n);
void scan_exclusive_u32_u32(spsamd_ctx *c, const uint32_t *in, uint32_t *out, size_t n);
void scan_exclusive_u8_u32(spsamd_ctx *c, const uint8_t *in, uint32_t *out, size_t n);
void scan_exclusive_u64_u64(spsamd_ctx *c, const unsigned long long *in, unsigned long long *out, size_t n);

// The same for up to SCAN_BATCH_MAX arrays of one length in three launches (blockIdx.y = array): the symbolic phase
// scans a dozen per-row counters of the heavy rows, and a launch is worth more than the work at that size.
constexpr int SCAN_BATCH_MAX = 12;
struct ScanBatch { const uint32_t *in[SCAN_BATCH_MAX]; uint32_t *out[SCAN_BATCH_MAX]; int count = 0;
	void add(const uint32_t *i, uint32_t *o) { in[count] = i; out[count] = o; ++count; } };
void scan_exclusive_u32_batch(spsamd_ctx *c, const ScanBatch &b, size_t n);

// One device-to-host round trip for a list of 32-bit words scattered over device memory (host[i] = *p[i]).
constexpr int WORD_LIST_MAX = 40;
struct WordList { const uint32_t *p[WORD_LIST_MAX]; int count = 0;
	int add(const void *q) { p[count] = (const uint32_t *)q; return count++; }
	int add64(const void *q) { const int at = add(q); add((const uint32_t *)q + 1); return at; } };
void read_back_words(spsamd_ctx *c, const WordList &w, uint32_t *host);

// The frame of every sort by key: the two key and two payload buffers out of the workspace (allocated by the constructor:
// keys, keys, payloads, payloads, n entries each), the caller's keys in `keys`, then run(): a stable LSD radix sort on key
// bits [low_bit, key_bits) (a caller whose input is already in the order of the low bits skips their passes).  The
// payload is the storage position, so what comes out is the sorted keys and the stable permutation that sorts them.
//
// The one-word form, for a caller that names its key width to the constructor and whose keys are short enough to share a
// 64-bit word with the position (word_key_bits + bits_of(n) <= 64; index_bits >= 0 says that it was taken): the words are
// key << index_bits | position, the sort goes over the key's bits alone -- 8 bytes per item and pass instead of 12 -- and
// there are no payload buffers: sorted() hands both forms to the kernels that read the result.  run_indices() is run() for
// the key major << minor_bits | minor of an operand's tuples: its first pass reads the two index arrays and puts the key (or
// the word) together itself, so nobody fills `keys`.
struct SortedKeys {
	const uint64_t *w;       // two arrays: the keys | one word: key << ibits | position
	const uint32_t *perm;    // two arrays: the positions | one word: null
	int ibits;               // 0 with two arrays
	__device__ __forceinline__ uint64_t key(size_t i) const { return w[i] >> ibits; }
	__device__ __forceinline__ uint32_t pos(size_t i) const { return perm ? perm[i] : (uint32_t)(w[i] & ((uint64_t(1) << ibits) - 1)); }
};

struct PairSort {
	uint64_t *keys;          // before run(): the n keys to fill | after: the keys, sorted
	uint32_t *perm;          // after run(): perm[i] = the input position of sorted key i (null in the one-word form)
	int index_bits;          // >= 0: the one-word form and the position's width
	PairSort(spsamd_ctx *c, size_t n, int word_key_bits = -1);
	void run(int key_bits, int low_bit = 0);
	void run_indices(const int32_t *major, const int32_t *minor, int minor_bits, int key_bits, int low_bit = 0);
	SortedKeys sorted() const { return SortedKeys{keys, perm, index_bits < 0 ? 0 : index_bits}; }
private:
	uint64_t *spare_keys;    // the other pair of buffers
	uint32_t *spare_pay;
	void sort_from(const void *first, int key_bits, int low_bit);   // first: a KeySrc of prims.hip or null
	spsamd_ctx *c;
	size_t n;
};

void fill_u32(spsamd_ctx *c, uint32_t *p, uint32_t v, size_t n);
void fill_zero(spsamd_ctx *c, void *p, size_t bytes);
template <class T> T *get_zeroed(spsamd_ctx *c, size_t n) { T *p = c->arena.get<T>(n); fill_zero(c, p, n * sizeof(T)); return p; }   // workspace memory

template <class T>
T read_back(spsamd_ctx *c, const T *dev)
{
	T *h = (T *)c->host_staging(sizeof(T));
	SPS_HIP(hipMemcpyAsync(h, dev, sizeof(T), hipMemcpyDeviceToHost, c->stream));
	SPS_HIP(hipStreamSynchronize(c->stream));
	return *h;
}

inline unsigned grid_for(size_t n, unsigned bs = 256) { return (unsigned)((n + bs - 1) / bs); }

// Internal value of spsamd_coo::mem (never part of the public ABI): device arrays this library produced itself and
// knows to be consolidated with valid indices -- consolidate_operand takes them as they are, without the inspection pass.
#define SPSAMD_MEM_DEVICE_VERIFIED 3

// ---------------------------------------------------------------- operand intake (operand.hip)
// What every entry point settles about an operand before its own work starts.  These return facts; what an operation
// does with them (consolidate, sort without merging, pack rows, make unique keys, only inspect) stays in its own file.

struct Prepared;

// Any operand as a plain one.  SPSAMD_MEM_PREPARED: the handle is checked (non-null, prepared by `c`) and `coo` holds its
// consolidated tuples as stored (idx0 / idx1 by its lead, sort0 = its lead, device memory; the shape is X's), `prep` the
// handle.  Host and device operands: `coo` is *X, `prep` null.  Either way coo.nnz is the operand's tuple count.
struct OperandView { spsamd_coo coo; Prepared *prep = nullptr; };
OperandView operand_view(spsamd_ctx *c, const spsamd_coo *X);
// The tuple count alone, nothing checked (a null handle counts as empty): for the short circuits that run before intake.
uint64_t operand_tuples(const spsamd_coo *X);

// The argument checks of a plain operand, all SPSAMD_EINVAL: mem (under OPERAND_PLAIN_MEM), then, where it has tuples,
// 2^31 or more of them, a null array (val counts under OPERAND_VALUES), a dimension beyond the int32 index range.
enum { OPERAND_VALUES = 1,        // the caller reads X.val
       OPERAND_PLAIN_MEM = 2 };   // mem must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE (the multiply's intake also takes _VERIFIED)
void check_operand(const spsamd_coo &X, int flags);

// Is the device operand X a result this context wrote itself and still holds (c->own): consolidated by X.sort0, indices valid?
bool is_own_result(const spsamd_ctx *c, const spsamd_coo &X);

// Upload if host: p itself for device memory (or n == 0), else a copy in the workspace.
template <class T>
const T *to_device(spsamd_ctx *c, const T *p, size_t n, int mem)
{
	if (mem != SPSAMD_MEM_HOST || n == 0) return p;
	T *d = c->arena.get<T>(n);
	SPS_HIP(hipMemcpyAsync(d, p, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
	return d;
}

// A plain operand (host or device, X.nnz > 0) as a stream of op()'s tuples for the calls that merge or search sorted streams
// (add, emult): the argument checks, the arrays on the device in op()'s orientation (lead = 1 for 'T') and, unless it is a
// result this context wrote itself, the inspection flags (inspect_operand).  SPSAMD_EINVAL: an index out of bounds; a sort0
// that names op()'s row order over (row, col) keys that descend somewhere (equal keys are allowed).
struct PlainStream {
	const int32_t *major = nullptr, *minor = nullptr;
	const double *val = nullptr;
	uint32_t flags = 0;           // inspect_operand's; 0 for an own result
	bool own_result = false;
};
PlainStream plain_stream(spsamd_ctx *c, const spsamd_coo &X, int lead);

// A structural operand (multiply_masked's M, emult's pattern operand): the keys of op(M) in row-major order, each once --
// workspace memory, or M's own arrays where they already are that (`prep`: the handle of the same transpose they belong
// to).  Only the indices are read (val may be null); duplicate keys count once, explicit zeros count; an index out of
// bounds and a sort0 that names op()'s row order over keys that descend are SPSAMD_EINVAL.  lead = 1 for 'T'; nrow x ncol
// is op(M)'s shape.
struct MaskKeys {
	const int32_t *i = nullptr, *j = nullptr;
	uint32_t n = 0;
	Prepared *prep = nullptr;
};
void mask_keys(spsamd_ctx *c, const spsamd_coo *M, int lead, uint64_t nrow, uint64_t ncol, MaskKeys *out);

int bits_of(uint64_t dim);        // bits needed to hold indices 0 .. dim-1
// keys[i] = major[i] << minor_bits | minor[i]: the sort key of radix_sort_pairs (payload: the storage position) ...
void build_keys(spsamd_ctx *c, const int32_t *major, const int32_t *minor, size_t n, int minor_bits, uint64_t *keys);
// ... and tuple i of the sorted operand: its indices out of sorted key i, its value from the storage position beside it
void gather_sorted(spsamd_ctx *c, const SortedKeys &sk, const double *val, size_t n, int minor_bits,
	int32_t *row, int32_t *col, double *oval);

// The frame of a product op(A) * op(B) (multiply_sparse.hpp:167-169): op(A) rows = A.shape[a0]; op(B) is read by ROWS
// (inner index first), its columns are B.shape[bj].
struct ProductFrame {
	int a0, a1, bk, bj;
	uint64_t nrow, inner, ncol;   // rows(op(A)), its columns, cols(op(B))
	uint64_t inner_b;             // rows(op(B)): must equal `inner`
	uint64_t shape0, shape1;      // the result's shape (nrow x ncol, the other way round under `permute`)
	ProductFrame(const spsamd_coo *A, char transpose_A, const spsamd_coo *B, char transpose_B, bool permute);
	void check_inner(const char *what) const;   // SPSAMD_EDIM (:172-174); `what` names the right operand, "B" or "V" (:173,299)
};
// The reference's short circuits (:178-184): the product is empty whatever the operands hold.
bool product_is_empty(double C, const spsamd_vec *scalei, const spsamd_coo *A, const spsamd_vec *scalej, const spsamd_coo *B,
	const spsamd_vec *scalek);

// ---------------------------------------------------------------- consolidated operand (consolidate.hip)

// op(X) in row-major consolidated form on the device.
struct ConMat {
	int32_t *row = nullptr;     // leading (row of op(X)) index per tuple
	int32_t *col = nullptr;     // minor index per tuple
	double *val = nullptr;
	uint32_t nnz = 0;
	uint64_t nrow = 0, ncol = 0;
};

// (spsamd_coo::mem == SPSAMD_MEM_PREPARED: idx0 carries the spsamd_operand handle, whose first member is its Prepared record)

// Upload (if host) + consolidate `X` by sort order {lead, 1-lead} into `out`
// (arena memory).  A prepared operand whose lead matches yields its handle in *prep (otherwise null).  Mirrors Consolidate<> (algorithm.hpp:353-369): an operand
// whose sort0 == lead is used as is.
// `ref_lead` is the leading dimension of the order the REFERENCE consolidates this operand in
// (it differs from `lead` for B: multiply_sparse.hpp:168); it decides which NaNs zero_nan drops.
void consolidate_operand(spsamd_ctx *c, const spsamd_coo *X, int lead, int ref_lead, int duplicate_policy,
	int zero_nan, ConMat *out, Prepared **prep = nullptr, const unsigned long long *global_first_key = nullptr);
// (global_first_key: the distributed step's -- device word holding the smallest reference-order key of a kept tuple over ALL
// ranks' blocks; under zero_nan the NaNs below it are the leading run the reference drops, algorithm.hpp:272-275)

// Distributed step under zero_nan: smallest reference-order key of a tuple of X (DEVICE arrays) that is neither 0 nor NaN
// -> *out_dev (all ones: none).  Same key as consolidate_operand's own first-kept search.
void first_kept_key_raw(spsamd_ctx *c, const spsamd_coo *Xdev, int lead, int ref_lead, unsigned long long *out_dev);

// Inspection flags of tuples (major, minor, val) on the device (k_inspect): bit0 an index out of [0, nrow) x [0, ncol),
// bit4 the major index descends somewhere, bit5 the (major, minor) key descends somewhere; the other bits are
// consolidate_operand's own.
uint32_t inspect_operand(spsamd_ctx *c, const int32_t *major, const int32_t *minor, const double *val, size_t n,
	uint64_t nrow, uint64_t ncol);

// Row boundaries of a consolidated operand: dim_beginnings (algorithm.hpp:74-118):
// beg[r] for each non-empty row + sentinel, and the row ids.
struct RowList {
	uint32_t *beg = nullptr;    // nrows + 1 entries
	int32_t *id = nullptr;      // nrows entries
	uint32_t nrows = 0;
};
void dim_beginnings(spsamd_ctx *c, const ConMat &m, RowList *out);
// The same from m's dense row pointer (row r holds tuples iff ptr[r + 1] > ptr[r]): three passes over nrow entries
// instead of nnz.
void dim_beginnings(spsamd_ctx *c, const ConMat &m, const uint32_t *ptr, RowList *out);

// Stable permutation sorting X by {lead, 1-lead} (device array of X->nnz uint32, arena memory).
uint32_t *sorted_permutation(spsamd_ctx *c, const spsamd_coo *X, int lead);

// Dense row pointer over all `nrow + extra` rows (extra trailing empty rows); `into`: the array to fill (nrow + 1 + extra
// entries) or null for arena memory.
uint32_t *dense_rowptr(spsamd_ctx *c, const ConMat &m, uint32_t extra, uint32_t *into = nullptr);

// One B tuple as the numeric kernels read it: column and value side by side (12 bytes), so
// a short B segment sits in one or two cache lines instead of two partial lines of separate
// col[] / val[] arrays.  Same bytes per product as the SoA form (12 B).
struct __attribute__((packed, aligned(4))) BTup { int32_t col; uint32_t vlo, vhi; };

// What a multiply derives from a consolidated operand before it can start, kept so that it is derived once: the reference
// keeps an operand's row structure across calls as well (the lazy dim_beginnings cache, VectorCooArray.hpp:325-335) and
// skips the consolidation of an operand that carries the wanted sort order (algorithm.hpp:360).  Either a VIEW for the
// duration of one call (pieces in the context's arena; the distributed step hands its panel's row pointer in this way) or a
// prepared-operand HANDLE of the C ABI (spsamd_operand_prepare: pieces in device memory of their own, built on first use).
// The level schedule of one (uplo, diag) triangle of an operand (k_solve.hip): the rows listed level
// by level (ascending inside a level), the levels' bounds in that list and, for the host that plans the launches, copies of
// the bounds and of each level's longest row.
struct SolveSchedule {
	bool built = false;
	uint32_t levels = 0, max_level_rows = 0;
	uint64_t tuples_used = 0;
	int64_t zero_pivot = -1;
	uint32_t *level_ptr = nullptr;    // device: levels + 1 entries
	uint32_t *rows = nullptr;         // device: one entry per row of op(A)
	std::vector<uint32_t> h_level_ptr, h_level_max;
	// spsamd_factor_ilu0 on the LOWER / NONUNIT schedule (k_factor.hip): each level's largest row work (lookups, saturated)
	bool have_work = false;
	std::vector<uint32_t> h_level_work;
};

struct Prepared {
	spsamd_ctx *ctx = nullptr;
	ConMat m;                         // op(X), consolidated, row-major
	int lead = 0;                     // the stored dimension that is m.row
	bool owns = false;                // handle: the pieces live in device memory of the handle's own until release()
	std::vector<void *> owned;        // its slabs (few and large: a handle's arrays are gathered from at random like the workspace's,
	uint64_t owned_bytes = 0;         // and many small allocations cost the numeric kernels 5 % in address translation)
	char *slab = nullptr;             // the slab being carved
	size_t slab_left = 0;
	void reserve(size_t bytes);       // make the next `bytes` of alloc() calls come out of one slab
	// both roles
	uint32_t *rowptr = nullptr;       // dense row pointer over nrow + 1 rows (the last one an empty sentinel): nrow + 2 entries
	uint32_t maxlen = 0;              // longest row
	bool have_maxlen = false;
	// left operand
	RowList rl;                       // dim_beginnings (algorithm.hpp:74-118)
	bool have_rl = false;
	// right operand
	BTup *btup = nullptr;             // (col, val) interleaved, nnz + 4 entries
	int W = 0;                        // column-window width of the heavy-row indices below (0: not built)
	uint32_t nwin = 0, nwp = 0;
	uint64_t nrowb = 0;
	uint32_t *bwin = nullptr;         // [nrowb][nwin + 1] first tuple of row k with column >= w * W
	uint16_t *wcnt = nullptr;         // [nrowb][nwp]      tuples of row k in window w
	uint32_t *bocc = nullptr;         // [nrowb][nbw]      bit w: row k has a tuple in window w (nbw words, a multiple of four)
	uint32_t nbw = 0;
	uint32_t *wptr = nullptr;         // [nwin][nrowb] + 1 window-major copy: CSR pointer per window ...
	BTup *btw = nullptr;              // ... and its tuples
	// triangular solves
	SolveSchedule solve[2][2];        // [uplo][diag], each built by the first solve that needs it (handles only)
	void *alloc(size_t bytes);        // arena memory of the current call (view) or device memory of the handle's own
	template <class T> T *get(size_t n) { return (T *)alloc(n * sizeof(T)); }
	void release();
};

// ---------------------------------------------------------------- multiply (spgemm.hip and the k_*.hip kernel files)

struct ScaleDev {
	bool present = false;
	int32_t *pos = nullptr;     // dense: position in the vector or -1
	const double *val = nullptr; // device copy of the values
	uint64_t dim = 0;
};

void upload_scale(spsamd_ctx *c, const spsamd_vec *s, uint64_t dim, const char *name, ScaleDev *out);

struct MultiplyArgs {
	double C;
	ScaleDev si, sj, sk;
	ConMat A, B;
	int sink_kind, sink_flags;
	Prepared *pa = nullptr, *pb = nullptr;   // derived structures of A / B that already exist (or are kept once built): may be null
	hipEvent_t b_ready = nullptr;            // the TUPLES of B arrive on another stream (the distributed step's panel): wait for this
	                                         // event before the first kernel that reads them; its row pointer (pb->rowptr) is valid at once
	OutSet *out = nullptr;                   // SINK_COO: the arrays the tuples go to (null: the context's current output set)
	bool static_walk = false;                // the distributed step's block product: its tiles keep the static walk
};
void spgemm(spsamd_ctx *c, MultiplyArgs &a, spsamd_result *res);
void prepared_row_structure(spsamd_ctx *c, Prepared *p);      // its dense row pointer and longest row, now (spgemm.hip)
BTup *prepared_btup(spsamd_ctx *c, Prepared *p);               // its packed (col, val) tuples, built on first use (spgemm.hip)

// Shared body of the MM and MV entry points (capi.hip); `arena_ready`: the caller has reset the workspace
// and may hold operands in it (the distributed step does); `parts`: records of derived structures the caller already
// has for A / B (the distributed step: its panel's row pointer, and the event that says the panel's tuples have arrived);
// `b_rank1`: B stands for a rank-1 array (MV's V as a k x 1 matrix), which the reference consolidates by its own order {0}.
struct OperandParts { Prepared *pa = nullptr, *pb = nullptr; hipEvent_t b_ready = nullptr; };
int multiply_body(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res, const char *what, bool arena_ready, const OperandParts *parts = nullptr, bool b_rank1 = false);

// ---------------------------------------------------------------- streamed product (k_stream.hip)

// spsamd_multiply_stream after its null checks
int multiply_stream(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_flags, size_t block_tuples, spsamd_chunk_fn cb, void *user,
	spsamd_result *res, spsamd_stream_stats *stats);

// ---------------------------------------------------------------- dense right-hand sides (k_spmm.hip)

// op(M)'s tuples in order of the output row (storage order inside a row) with a dense row pointer: workspace memory, or
// the pieces of a prepared operand of the same transpose
struct DenseOperand {
	const uint32_t *rowptr = nullptr;   // nrow + 1 entries (at least)
	const BTup *tup = nullptr;
	uint64_t nrow = 0, ncol = 0;        // rows(op(M)), cols(op(M))
	uint32_t nnz = 0;
	bool sorted = false;                // the stable sort ran (the storage order was not row order)
};
// Checks the indices (SPSAMD_EINVAL) and orders the tuples; lead = 1 for 'T'.
void dense_operand(spsamd_ctx *c, const spsamd_coo *M, int lead, DenseOperand *out);
// Y[i * ldy + r] (op)= op(M)(i, j) * X[j * ldx + r] in storage order, X and Y device memory
void spmm_dense(spsamd_ctx *c, const DenseOperand &m, const double *X, uint64_t ldx, double *Y, uint64_t ldy, uint32_t nrhs,
	int policy, bool handle_nan);
// out[t] = (minor[t], val[t]) packed, for a caller that has op(M)'s tuples in row order already
void pack_tuples(spsamd_ctx *c, const int32_t *minor, const double *val, uint32_t n, BTup *out);
// The long rows' half of spmm_dense for a caller that applies one operand many times (spsamd_solve_pcg): the rows of more
// than long_min tuples listed once (workspace memory; returns how many) ...
uint32_t spmm_long_list(spsamd_ctx *c, const uint32_t *rowptr, uint64_t nrow, uint32_t long_min, uint32_t **list, uint32_t **count);
// ... and Y[i] += op(M)(i, j) * X[j] in storage order for the listed rows alone (ADD, handle_nan off): one launch of the wave
// kernel spmm_dense would choose, nothing allocated
void spmm_long_rows(spsamd_ctx *c, const DenseOperand &m, const uint32_t *list, const uint32_t *count, const double *X, uint64_t ldx,
	double *Y, uint64_t ldy, uint32_t nrhs);

// ---------------------------------------------------------------- sparse addition (k_add.hip)

// op(X) on the device, ordered by (row, col), storage order inside a key: one side of a merge
struct AddStream {
	const int32_t *row = nullptr, *col = nullptr;
	const double *val = nullptr;
	uint32_t n = 0;
};
constexpr int ADD_NT = 256;                    // lanes per tile
constexpr int ADD_IPT = 8;                     // merged items per lane
constexpr int ADD_TILE = ADD_NT * ADD_IPT;     // merged items per tile
// Merge-path split of the merged sequence of a and b (64-bit keys row << 32 | col, ties: a first) into `ntiles` tiles of
// ADD_TILE items: split[t] = how many of a's tuples lie in the first min(t * ADD_TILE, a.n + b.n) items (ntiles + 1 entries).
// Shared by add and emult.
void merge_partition(spsamd_ctx *c, const AddStream &a, const AddStream &b, uint32_t ntiles, uint32_t *split);

// C = alpha * op(A) + beta * op(B) into the sink: spsamd_add after its null checks
void add_matrices(spsamd_ctx *c, double alpha, const spsamd_coo *A, char transpose_A, double beta, const spsamd_coo *B,
	char transpose_B, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res);

// ---------------------------------------------------------------- masked product (k_masked.hip)

// op(A) * op(B) on the pattern of M: spsamd_multiply_masked after its null checks
void multiply_masked(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, const spsamd_coo *M, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res);

// ---------------------------------------------------------------- sampled dense-dense product (k_sampled.hip)

// out[t] = alpha * (P_i . Q_j) (+ beta * v) for every tuple (i, j, v) of op(M): spsamd_multiply_sampled after the context check
void multiply_sampled(spsamd_ctx *c, const spsamd_coo *M, char transpose, const double *P, size_t ldp, const double *Q,
	size_t ldq, size_t k, double alpha, double beta, double *out, int mem);

// ---------------------------------------------------------------- dropping entries (k_select.hip)

// the tuples of op(A) a predicate keeps, into the sink: spsamd_select after its null checks
void select_tuples(spsamd_ctx *c, const spsamd_coo *A, char transpose, int predicate, int64_t iparam, double dparam,
	int select_flags, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res);

// ---------------------------------------------------------------- submatrix by index lists (k_extract.hip)

// op(A)(I, J) into the sink: spsamd_extract after its null checks (rows / cols null: every index of that dimension)
void extract_tuples(spsamd_ctx *c, const spsamd_coo *A, char transpose, const int32_t *rows, size_t nrows, const int32_t *cols,
	size_t ncols, int index_mem, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res);

// ---------------------------------------------------------------- reduction to a vector (k_reduce.hip)

// post(fold of op(A)'s rows) into the caller's buffers: spsamd_reduce after its null checks.  Returns SPSAMD_OK, or
// SPSAMD_ECAPACITY with *out_nnz = the entries needed and the context's last error set (nothing written).
int reduce_rows(spsamd_ctx *c, const spsamd_coo *A, char transpose, int op, int post, int duplicate_policy, int zero_nan,
	int32_t *out_idx, double *out_val, size_t capacity, int mem, size_t *out_nnz, spsamd_result *res);

// The checks of caller-owned output buffers (reduce, solve_tri, color; defined in k_reduce.hip): do two byte ranges overlap (a null or empty one never does);
// does a device range touch an output set of the context?
bool ranges_overlap(const void *p, uint64_t np, const void *q, uint64_t nq);
bool in_output_sets(const spsamd_ctx *c, const void *p, uint64_t bytes);
// The DIAG fold (post NONE, dense form) of an operand already taken: ptr / col / val are S's dense row pointer and tuples,
// d gets nrow values in device memory, +0.0 where a row stores no diagonal.  Workspace of the current call; nrow > 0.
void reduce_diag_dense(spsamd_ctx *c, const uint32_t *ptr, const int32_t *col, const double *val, uint64_t nrow, double *d);

// ---------------------------------------------------------------- sparse triangular solve (k_solve.hip)

// T * X = B for the `uplo` triangle of op(A): spsamd_solve_tri after the context check
int solve_tri(spsamd_ctx *c, const spsamd_coo *A, char transpose, int uplo, int diag, const double *B, size_t ldb, double *X,
	size_t ldx, size_t nrhs, int mem, int duplicate_policy, int zero_nan, spsamd_solve_stats *stats, spsamd_result *res);

// One triangle of S as the analysis and the solve kernels read it
struct TriView {
	const uint32_t *ptr;                       // dense row pointer of S
	const int32_t *col;
	const double *val;
	uint64_t n;                                // order of op(A)
	int upper, unit;
};
// The schedule of the `uplo` / `diag` triangle of S into `s`: device arrays in workspace memory, or in the handle's own
// when `hp` is given.  peel[0] / peel[1]: the k_peel_thin / k_peel_wide launches issued (those that find an empty frontier too).
void analyse(spsamd_ctx *c, const TriView &t, Prepared *hp, SolveSchedule *s, uint64_t peel[2]);
// The numeric phase alone, on a schedule of t's triangle: T * X = B over device arrays (X may be B).  Returns the launches
// issued; *fused_levels (may be null) the levels served inside fused runs.
uint64_t solve_levels(spsamd_ctx *c, const TriView &t, const SolveSchedule &s, const double *B, uint64_t ldb, double *X,
	uint64_t ldx, uint32_t nrhs, uint64_t *fused_levels);
constexpr int SOLVE_NT = 1024;                 // threads of the one workgroup of a fused run (k_solve_fused, k_fac_fused) and of k_peel_thin
constexpr uint32_t SOLVE_FUSE_ROWS = 256;      // default of the solve_fuse_rows knob: the flat end of the measured sweep

// ---------------------------------------------------------------- Krylov loops (k_krylov.hip, k_bicgstab.hip, k_gmres.hip)
// All three loops, and solve_pcg_amg through pcg_solve, run inside one frame, KrylovCall (krylov_dev.h, HIP only): it owns the
// argument checks and their order, the operands, the workspace order, the preconditioner's data with the schedule rollback,
// the vector kernels, the read-back loop, what counts as a launch, and the tail.  A loop supplies its state struct, its own
// vectors, its direction / update / finish kernels and the body of an iteration.

// A x = b by preconditioned conjugate gradients, the loop of the header: spsamd_solve_pcg after the context check
int solve_pcg(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res);
constexpr int PCG_CHECK_EVERY = 8;             // default of the pcg_check_every knob: the measured sweep is flat from 4 on, and 8 bounds the work after the stop

// An operand taken by consolidate_operand with what its serial chains need: S for the loop's SpMV, and every level operand
// of the multigrid cycle (k_amg.hip)
struct RowOperator {
	const uint32_t *ptr = nullptr;   // dense row pointer, nrow + 1 entries
	const int32_t *col = nullptr;
	const double *val = nullptr;
	uint64_t nrow = 0, ncol = 0;
	uint32_t nnz = 0;
	uint32_t long_min = 0xFFFFFFFFu; // rows of more tuples go to the wave kernel of k_spmm.hip
	uint32_t nlong = 0;              // how many there are; then: their list and its length on the device, the packed tuples in m
	const uint32_t *list = nullptr, *count = nullptr;
	DenseOperand m;
};
// S's row pointer; under `long_rows` the long rows' list and the packed rows of k_spmm.hip where there is a long row
void row_operator(spsamd_ctx *c, ConMat &S, Prepared *hp, uint64_t nrow, uint64_t ncol, bool long_rows, RowOperator *out);
// SPSAMD_EINVAL where X has 2^31 or more tuples or the vector x overlaps one of its arrays
void check_vector_overlap(spsamd_ctx *c, const spsamd_coo *X, const char *name, const double *x, uint64_t bytes);

// The preconditioner step of the frame as a hook.  setup() runs once, after S is taken and the loop's vectors exist: it
// takes everything it needs out of the workspace then.  apply() enqueues z = M^-1 r on those two vectors and returns the
// launches it issued; it allocates nothing, reads no PcgState and writes nothing but its own scratch and z.
struct PcgPrecond {
	virtual void setup(spsamd_ctx *c, const RowOperator &S, const double *r, double *z) = 0;
	virtual uint64_t apply() = 0;
	virtual ~PcgPrecond() {}
};
constexpr int PCG_PRECOND_HOOK = 3;            // pcg_solve's precond under a hook (never a value of the public ABI)
// solve_pcg's loop with z = M^-1 r left to `hook` (precond PCG_PRECOND_HOOK, M null), or solve_pcg itself (hook null)
int pcg_solve(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res, PcgPrecond *hook);

// A x = b for an unsymmetric A by BiCGStab, the loop of the header: spsamd_solve_bicgstab after the context check
int solve_bicgstab(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res);

// A x = b for an unsymmetric A by restarted GMRES(m), the loop of the header: spsamd_solve_gmres after the context check
int solve_gmres(spsamd_ctx *c, const spsamd_coo *A, char transpose, int precond, const spsamd_coo *M, char transpose_M,
	const double *b, double *x, int mem, double tol, uint64_t max_iter, uint32_t restart, double *hist_host, size_t hist_capacity,
	int duplicate_policy, int zero_nan, spsamd_pcg_stats *stats, spsamd_result *res);

// ---------------------------------------------------------------- aggregation multigrid cycle (k_amg.hip)

// x = cycle(0, b): spsamd_amg_apply after the context check
int amg_apply(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params, const double *b,
	double *x, int mem, int duplicate_policy, int zero_nan, spsamd_amg_stats *stats, spsamd_result *res);
// the loop of solve_pcg with z = cycle(0, r): spsamd_solve_pcg_amg after the context check
int solve_pcg_amg(spsamd_ctx *c, const spsamd_amg_level *levels, size_t nlevels, const spsamd_amg_params *params, const double *b,
	double *x, int mem, double tol, uint64_t max_iter, double *hist_host, size_t hist_capacity, int duplicate_policy, int zero_nan,
	spsamd_pcg_stats *stats, spsamd_amg_stats *astats, spsamd_result *res);
constexpr uint32_t AMG_FUSE_ROWS = 1024;       // default of the amg_fuse_rows knob
constexpr int AMG_MAX_LEVELS = 32;

// ---------------------------------------------------------------- ILU(0) factorisation (k_factor.hip)

// F = ILU(0) of op(A) into the sink: spsamd_factor_ilu0 after its null checks
void factor_ilu0(spsamd_ctx *c, const spsamd_coo *A, char transpose, int duplicate_policy, int zero_nan, int sink_kind,
	int sink_flags, spsamd_factor_stats *stats, spsamd_result *res);

// ---------------------------------------------------------------- multi-colour ordering (k_color.hip)

// the greedy colouring of op(A)'s graph into the caller's buffers: spsamd_color after its null checks.  Returns SPSAMD_OK,
// or SPSAMD_ECAPACITY with *out_ncolors = the colours and the context's last error set (nothing written).
int color_graph(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int color_flags, int32_t *color,
	int32_t *perm, int32_t *color_ptr, size_t ptr_capacity, int mem, size_t *out_ncolors, spsamd_color_stats *stats,
	spsamd_result *res);

// The two parts of the colouring that spsamd_aggregate runs too: one copy, in k_color.hip.
// The graph of the key set K of an n x n operand as rows: K symmetrised, made unique and stripped of its diagonal, or
// (`symmetric`) K's own rows, which may name the vertex itself.  Workspace memory, or K's and its handle's own arrays.
struct GraphRows { const uint32_t *ptr; const int32_t *adj; };
GraphRows graph_adjacency(spsamd_ctx *c, const MaskKeys &K, uint64_t N, bool symmetric);
// Per vertex its degree (the row without the vertex itself); the worklists of round 0 by class (thread: deg <= wave_deg, or
// what rowk says), their lengths in ctr[0] and ctr[1]; the totals in acc[GRAPH_*].  A vertex of degree 0 gets color 0 and
// is on no list, or (`list_isolated`) color -1 and a place on the thread-class list; every other vertex gets color -1.
enum { GRAPH_ADJ = 0, GRAPH_MAXDEG = 1, GRAPH_ROWS_T = 2, GRAPH_ROWS_W = 3, GRAPH_ACC = 4 };
void graph_classes(spsamd_ctx *c, const GraphRows &g, uint64_t N, uint32_t *deg, int32_t *color, uint32_t *list_t, uint32_t *list_w,
	uint32_t *ctr, unsigned long long *acc, uint32_t wave_deg, int rowk, int list_isolated);
// The output tail: `sort` holds one key of key_bits bits per vertex; a stable sort, so the vertices come out ascending in
// (key, index), into `list` (may be null; `kind` says where the caller's buffers live); under `bounds` the nbuckets + 1
// bounds of the buckets key >> shift in that list, every one of which must occur, into workspace memory (returned) and
// `list_ptr` (may be null).
uint32_t *order_by_key(spsamd_ctx *c, PairSort &sort, uint64_t N, int key_bits, int shift, uint64_t nbuckets, bool bounds,
	int32_t *list, int32_t *list_ptr, hipMemcpyKind kind);

// The frame of a graph call: what spsamd_color and spsamd_aggregate do around their sweeps, once.
// An operation names its messages, knobs and counters (GraphOp); its orders and its one flag have spsamd_color's values.
static_assert(SPSAMD_AGG_ORDER_HASH == SPSAMD_COLOR_ORDER_HASH && SPSAMD_AGG_ORDER_DEGREE == SPSAMD_COLOR_ORDER_DEGREE &&
	SPSAMD_AGG_SYMMETRIC == SPSAMD_COLOR_SYMMETRIC, "GraphCall::open checks one set of values");
struct GraphOp {
	const char *bad_order, *bad_flags, *not_square, *overlap, *too_small;      // the refusals' messages
	int Tuning::*path, Tuning::*row, Tuning::*fuse_rows, Tuning::*wave_deg;    // its four knobs, and the defaults of the last two
	uint32_t fuse_rows_default, wave_deg_default;
	int acc_len, nlists;                       // its acc[] slots; its worklists per parity: 2, or 4 (two (thread, wave) pairs)
};
struct GraphTotals { uint64_t adjacency, max_degree, launches, fused_rounds, rows_wave; float ms_adjacency; };   // the stats both structs hold
struct GraphCall {
	spsamd_ctx *c;
	const GraphOp *op;
	int32_t *ids_out = nullptr, *list_out = nullptr, *ptr_out = nullptr;   // the caller's: per-vertex ids, the ordered list, its bounds
	size_t ptr_capacity = 0, *out_count = nullptr;
	spsamd_result *res = nullptr;
	hipMemcpyKind kind = hipMemcpyDeviceToHost;                            // towards the caller's buffers
	uint64_t N = 0;                                                        // from here on: what open() leaves
	bool symmetric = false;
	MaskKeys K; GraphRows g{};
	int path = 0, rowk = 0;
	uint32_t fuse_rows = 0, wave_deg = 0;
	unsigned long long *acc = nullptr;         // op->acc_len counters, zeroed
	uint32_t *ctr = nullptr, *deg = nullptr;   // ctr[nlists * parity + list]: the lengths of the worklists, zeroed
	int32_t *ids = nullptr;
	uint32_t *h = nullptr;                     // host staging of op->acc_len * 8 bytes
	uint64_t launches = 0, rounds = 0;         // what sweep() counts
	bool fused = false;
	// Everything from the first argument check to the first workspace arrays: the refusals in their order, res and the
	// `stats_bytes` of `stats` (may be null) zeroed, the keys taken, *out_count zeroed after that, the adjacency, the knobs,
	// then acc, ctr, deg and ids out of the workspace in this order.  False: the call is over (no vertex) and returns *rc.
	bool open(const spsamd_coo *A, char transpose, int order, int flags, int mem, void *stats, size_t stats_bytes, int *rc);
	void read_counts(int par, uint32_t *cnt);  // cnt[nlists] = the lists' lengths at a parity: one copy, one synchronisation
	// The host loop over the parities from the round-0 counts in cnt[nlists].  round(par, cnt) enqueues one round and returns its
	// launches; fuse(par, cnt) enqueues the fused run of the rest: under path 2, or (path 0) once every (thread, wave) pair
	// of lists holds at most fuse_rows.  Nothing is zeroed here: the operations' kernels do that.
	template <class Round, class Fuse> void sweep(uint32_t *cnt, Round round, Fuse fuse)
	{
		for (int par = 0; cnt[0] || cnt[1]; par ^= 1) {
			bool thin = path != 1;
			for (int k = 0; k < op->nlists; k += 2) thin = thin && (path == 2 || (uint64_t)cnt[k] + cnt[k + 1] <= fuse_rows);
			if (thin) { fuse(par, cnt); ++launches; fused = true; break; }
			launches += round(par, cnt);
			++rounds;
			read_counts(par ^ 1, cnt);
		}
	}
	// *out_count = count; false, with the context's last error set, where ptr_out cannot hold count + 1 bounds.  The caller
	// returns SPSAMD_ECAPACITY then, without close(): nothing has been written.
	bool fits(uint64_t count);
	void deliver() { SPS_HIP(hipMemcpyAsync(ids_out, ids, N * sizeof(int32_t), kind, c->stream)); }
	// finish_call and res's three times; `hacc`: acc as read back, whose slot `fused_slot` counts the fused run's rounds
	GraphTotals close(const unsigned long long *hacc, int fused_slot);
};

// ---------------------------------------------------------------- MIS(2) aggregation (k_aggregate.hip)

// the aggregates of op(A)'s graph into the caller's buffers: spsamd_aggregate after its null checks.  Returns SPSAMD_OK,
// or SPSAMD_ECAPACITY with *out_naggregates = the aggregates and the context's last error set (nothing written).
int aggregate_graph(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int agg_flags, int32_t *agg,
	int32_t *members, int32_t *agg_ptr, size_t ptr_capacity, int mem, size_t *out_naggregates, spsamd_aggregate_stats *stats,
	spsamd_result *res);

// ---------------------------------------------------------------- element-wise product and pattern restriction (k_emult.hip)

// op(A) o op(B) (TIMES), op(A) on (FIRST) or off (FIRST | COMPLEMENT) op(B)'s pattern into the sink: spsamd_emult after
// its null checks
void emult_matrices(spsamd_ctx *c, int op, int emult_flags, double alpha, const spsamd_coo *A, char transpose_A,
	const spsamd_coo *B, char transpose_B, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res);

// The same operand struct twice (A * A): one consolidation can serve both sides (capi.hip).
bool same_operand(const spsamd_coo *a, const spsamd_coo *b);

// ---------------------------------------------------------------- sink tail (sink.hip)
// How an operation hands its result over.  A new operation calls these (and the intake above), it does not copy them.

// What every entry point with a sink refuses first: "bad duplicate_policy", "bad sink_kind" (SPSAMD_EINVAL).
void check_sink_args(int duplicate_policy, int sink_kind);
// Select the output set the next result is written to: the current one unless a device operand lives in it.
void pick_output_set(spsamd_ctx *c, const spsamd_coo *const *operands, int n);
// Does output set `s` of the context hold an array of one of the device operands?
bool output_set_aliased(const spsamd_ctx *c, int s, const spsamd_coo *const *operands, int n);

struct CooOut { int32_t *row, *col; double *val; };
// An output set grown to `total` tuples: the one way its three arrays are asked for.
CooOut grow_output(OutSet &o, size_t total);
// The current output set, about to be overwritten (its entry of c->own is dropped), grown to `total` + 1 tuples.
CooOut coo_output(spsamd_ctx *c, size_t total);
// Workspace arrays for `total` tuples: where the DIGEST sink of an operation that stores its tuples first keeps them.
CooOut scratch_output(spsamd_ctx *c, size_t total);
// The frame between a count pass and its store pass: offs = exclusive scan of counts (n + 1 entries), *total = offs[n] read
// back, and the output for that many tuples: coo_output, or scratch_output for the DIGEST sink.
CooOut counted_output(spsamd_ctx *c, const uint32_t *counts, uint32_t *offs, size_t n, bool coo, uint32_t *total);
// SINK_COO: fill res (nnz, idx0, idx1, val; its shape is set already) and register the tuples in c->own -- row-major sorted,
// every (i, j) once, indices valid: consolidated by sort order {0, 1}.  `permute` (PermuteAccum {1,0}): the same tuples
// with res->idx0 / idx1 swapped, which read that way are consolidated by {1, 0}.
void publish_coo(spsamd_ctx *c, spsamd_result *res, const int32_t *orow, const int32_t *ocol, const double *oval, uint64_t total, bool permute);
// DIGEST | ROWSTATS: the context's three per-row arrays (tuple count, value sum, index hash), zeroed and attached to res.
// `slack`: bytes each buffer is asked for beyond its nrow entries.
struct RowStats { long long *nnz = nullptr; double *sum = nullptr; unsigned long long *hash = nullptr; };
RowStats rowstats_begin(spsamd_ctx *c, uint64_t nrow, size_t slack, spsamd_result *res);
// SINK_DIGEST over stored tuples: the row statistics if sink_flags asks, index hash and value sum into res.
void digest_stored(spsamd_ctx *c, spsamd_result *res, const int32_t *orow, const int32_t *ocol, const double *oval, uint32_t total,
	uint64_t nrow, int sink_flags);
// The end of a call: EV_END recorded and waited for, ms_total (from EV_BEGIN) and workspace_bytes filled.
void finish_call(spsamd_ctx *c, spsamd_result *res);
// The tail of an operation whose `total` tuples are stored in `o` (rows of [0, nrow)): res->nnz, publish_coo or
// digest_stored, finish_call.  The ms_* fields other than ms_total stay with the caller: which events they span differs.
void deliver_stored(spsamd_ctx *c, spsamd_result *res, const CooOut &o, uint32_t total, uint64_t nrow, bool coo, bool permute, int sink_flags);

} // namespace spsamd
