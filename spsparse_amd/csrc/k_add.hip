// k_add.hip -- C = alpha * op(A) + beta * op(B) by a merge of two sorted streams (spsamd_add, include/spsparse_amd.h).
//
// The result is the reference's consolidate() (algorithm.hpp:251-319) of the concatenation
//     for (i, j, v) in op(A), in storage order:  T.add({i, j}, alpha * v);
//     for (i, j, v) in op(B), in storage order:  T.add({i, j}, beta * v);
// sorted by {0, 1}.  The stable sort of that concatenation is the merge of the two operands each sorted stably on its own,
// with A's tuples first on equal keys; so nothing is merged before the merge (folding B's duplicates before A's are added
// would change the rounding).
//
// Device path:
//   1. each operand as a stream sorted by (row, col) of op(): read in place where its stored order already is that order
//      (found by the inspection pass, a chained result of this context, a prepared handle of the same transpose), else
//      one stable radix sort with the storage position as payload and one gather of the values;
//   2. k_add_partition: merge-path split of the merged sequence into tiles of ADD_TILE items (ties: A first) -- fixed
//      tiles of the merged sequence, whatever the row lengths;
//   3. k_add_merge<count>: per tile, both slices staged in LDS, each lane merges ADD_IPT items; the lane that holds the
//      first item of a key group walks the whole group (A's run of the key, then B's, past the tile's end from global
//      memory) and says whether any item of it is kept; a scan of the per-tile counts gives each tile its output offset;
//   4. k_add_merge<write>: the same walk, now folding the kept items by the policy, and one tuple per group stored.
// Every scaled value and every sum of a NaN result has the bits x86-64 gives it (x86fp.h).
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

namespace spsamd {

// The first tuple of the merged sequence that consolidate() keeps whatever zero_nan says (neither 0 nor NaN after
// scaling), as its position in merge order (key, stream, index): under zero_nan the NaNs before it are the leading
// run the reference drops (algorithm.hpp:272-275).  key = ~0: there is none, every NaN is dropped.
struct FirstKept {
	unsigned long long key;
	uint32_t src, idx;
};

__device__ __forceinline__ uint64_t add_key(const int32_t *row, const int32_t *col, uint32_t i)
{
	return ((uint64_t)(uint32_t)row[i] << 32) | (uint64_t)(uint32_t)col[i];
}

__device__ __forceinline__ bool before_first(uint64_t key, uint32_t src, uint32_t idx, const FirstKept &f)
{
	return key < f.key || (key == f.key && (src < f.src || (src == f.src && idx < f.idx)));
}

// First index of a stream whose scaled value is kept whatever zero_nan says.  The stream is sorted, so the first index is
// also the first in merge order.  A lane's first hit in its grid-stride walk is its smallest: it stops there.
__global__ void __launch_bounds__(256) k_add_first_idx(const double *__restrict__ val, uint32_t n, double scale, uint32_t *out)
{
	uint32_t best = 0xFFFFFFFFu;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const double v = ref_mul(scale, val[i]);
		if (v != 0 && v == v) { best = i; break; }
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, d, 64));
	if (lane_id() == 0 && best != 0xFFFFFFFFu) atomicMin(out, best);
}

__global__ void k_add_first_pick(AddStream a, AddStream b, const uint32_t *idx, FirstKept *out)
{
	const uint32_t ia = idx[0], ib = idx[1];
	const uint64_t ka = ia != 0xFFFFFFFFu ? add_key(a.row, a.col, ia) : ~0ull;
	const uint64_t kb = ib != 0xFFFFFFFFu ? add_key(b.row, b.col, ib) : ~0ull;
	FirstKept f;
	if (ia == 0xFFFFFFFFu && ib == 0xFFFFFFFFu) { f.key = ~0ull; f.src = 2; f.idx = 0; }
	else if (ia != 0xFFFFFFFFu && (ib == 0xFFFFFFFFu || ka <= kb)) { f.key = ka; f.src = 0; f.idx = ia; }
	else { f.key = kb; f.src = 1; f.idx = ib; }
	*out = f;
}

// split[t] = how many of A's tuples lie in the first min(t * ADD_TILE, na + nb) items of the merged sequence
__global__ void __launch_bounds__(256) k_add_partition(AddStream a, AddStream b, uint32_t ntiles, uint32_t *split)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t > ntiles) return;
	const uint64_t d = std::min<uint64_t>((uint64_t)t * ADD_TILE, (uint64_t)a.n + b.n);
	uint32_t lo = d > b.n ? (uint32_t)(d - b.n) : 0u, hi = (uint32_t)std::min<uint64_t>(d, a.n);
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (add_key(a.row, a.col, mid) <= add_key(b.row, b.col, (uint32_t)(d - 1 - mid))) lo = mid + 1;
		else hi = mid;
	}
	split[t] = lo;
}

void merge_partition(spsamd_ctx *c, const AddStream &a, const AddStream &b, uint32_t ntiles, uint32_t *split)
{
	k_add_partition<<<dim3(grid_for((size_t)ntiles + 1)), dim3(256), 0, c->stream>>>(a, b, ntiles, split);
	SPS_LAUNCH_CHECK();
}

constexpr int ADD_COUNT = -1;                  // MODE of the count pass; the write pass's MODE is the duplicate policy

// One tile of the merged sequence.  Count pass: tile_count[tile] = tuples the tile emits.  Write pass: stores them from
// tile_off[tile] on.
template <int MODE>
__global__ void __launch_bounds__(ADD_NT) k_add_merge(AddStream a, AddStream b, double alpha, double beta, int zero_nan,
	const FirstKept *__restrict__ first, const uint32_t *__restrict__ split, uint32_t *__restrict__ tile_count,
	const uint32_t *__restrict__ tile_off, int32_t *__restrict__ orow, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	__shared__ uint64_t s_key[ADD_TILE];
	__shared__ double s_val[ADD_TILE];
	__shared__ uint64_t s_last[ADD_NT];
	__shared__ uint32_t s_scan[ADD_NT / 64 + 1];
	const uint32_t tile = blockIdx.x;
	const uint64_t n = (uint64_t)a.n + b.n;
	const uint64_t d0 = (uint64_t)tile * ADD_TILE, d1 = std::min<uint64_t>(d0 + ADD_TILE, n);
	const uint32_t ia0 = split[tile], ia1 = split[tile + 1];
	const uint32_t ib0 = (uint32_t)(d0 - ia0), ib1 = (uint32_t)(d1 - ia1);
	const uint32_t la = ia1 - ia0, len = (uint32_t)(d1 - d0), lb = len - la;
	// A's slice at [0, la), B's at [la, len)
	for (uint32_t k = threadIdx.x; k < len; k += ADD_NT) {
		if (k < la) { s_key[k] = add_key(a.row, a.col, ia0 + k); s_val[k] = a.val[ia0 + k]; }
		else { const uint32_t g = ib0 + (k - la); s_key[k] = add_key(b.row, b.col, g); s_val[k] = b.val[g]; }
	}
	FirstKept fk = {~0ull, 2u, 0u};
	if (zero_nan) fk = *first;
	__syncthreads();

	// this lane's items: merged positions [diag, diag + ADD_IPT) of the tile
	const uint32_t diag = std::min<uint32_t>(threadIdx.x * ADD_IPT, len);
	uint32_t lo = diag > lb ? diag - lb : 0u, hi = std::min(diag, la);
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (s_key[mid] <= s_key[la + diag - 1 - mid]) lo = mid + 1;
		else hi = mid;
	}
	uint32_t ia = lo, ib = diag - lo;
	uint64_t key[ADD_IPT];
	uint32_t cur_a[ADD_IPT], cur_b[ADD_IPT];               // the two cursors before the item was taken
	const uint32_t nit = std::min<uint32_t>(ADD_IPT, len - diag);
#pragma unroll
	for (int k = 0; k < ADD_IPT; ++k) {
		cur_a[k] = ia; cur_b[k] = ib;
		key[k] = ~0ull;
		if ((uint32_t)k < nit) {
			const bool take_a = ia < la && (ib >= lb || s_key[ia] <= s_key[la + ib]);
			key[k] = take_a ? s_key[ia] : s_key[la + ib];
			ia += take_a; ib += !take_a;
		}
	}
	if (nit) s_last[threadIdx.x] = key[nit - 1];
	__syncthreads();
	uint64_t prev = ~0ull;                                   // key of the item before this lane's first (~0: none)
	if (threadIdx.x > 0) prev = s_last[threadIdx.x - 1];
	else if (ia0 > 0 || ib0 > 0) {
		const uint64_t pa = ia0 > 0 ? add_key(a.row, a.col, ia0 - 1) : 0ull, pb = ib0 > 0 ? add_key(b.row, b.col, ib0 - 1) : 0ull;
		prev = std::max(pa, pb);
	}

	// Walk the group of every item that opens one: A's run of its key from the A cursor, then B's from the B cursor (an
	// item taken from B has no A tuple of its key left).  Items inside the slices come from LDS, the rest from memory.
	uint32_t emit = 0;
	double acc[ADD_IPT];
	bool out[ADD_IPT];
#pragma unroll
	for (int k = 0; k < ADD_IPT; ++k) {
		out[k] = false; acc[k] = 0.0;
		if ((uint32_t)k >= nit) continue;
		const uint64_t K = key[k];
		const bool head = K != (k == 0 ? prev : key[k - 1]);
		if (!head) continue;
		bool any = false;
		double s = 0.0;
		bool done = false;
		// one item of the group: scale, drop, fold (algorithm.hpp:284-310)
		auto item = [&](double raw, double scale, uint32_t src, uint32_t g) {
			const double v = ref_mul(scale, raw);
			if (v == 0) return;
			if (v != v && zero_nan && before_first(K, src, g, fk)) return;
			if (!any) { s = v; any = true; if (MODE == ADD_COUNT || MODE == SPSAMD_LEAVE_ALONE) done = true; }
			else if (MODE == SPSAMD_ADD) s = ref_add(s, v);
			else if (MODE == SPSAMD_REPLACE) s = v;
		};
		auto run = [&](const AddStream &st, uint32_t g, uint32_t g_lds_end, uint32_t g_lds_begin, uint32_t lds_base, double scale, uint32_t src) {
			for (; g < g_lds_end && !done; ++g) {
				const uint32_t q = lds_base + (g - g_lds_begin);
				if (s_key[q] != K) return;
				item(s_val[q], scale, src, g);
			}
			while (g < st.n && !done) {                          // past the slice: four items per round trip
				uint64_t kq[4]; double vq[4];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					kq[u] = ~0ull; vq[u] = 0.0;
					if (g + u < st.n) { kq[u] = add_key(st.row, st.col, g + u); vq[u] = st.val[g + u]; }
				}
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					if (kq[u] != K) return;
					if (!done) item(vq[u], scale, src, g + u);
				}
				g += 4;
			}
		};
		run(a, ia0 + cur_a[k], ia1, ia0, 0u, alpha, 0u);
		if (!done) run(b, ib0 + cur_b[k], ib1, ib0, la, beta, 1u);
		if (any) { out[k] = true; acc[k] = s; ++emit; }
	}

	if (MODE == ADD_COUNT) {
		uint32_t tot = 0;
		(void)block_exclusive_scan<uint32_t, ADD_NT>(emit, s_scan, &tot);
		if (threadIdx.x == 0) tile_count[tile] = tot;
		return;
	}
	uint32_t o = tile_off[tile] + block_exclusive_scan<uint32_t, ADD_NT>(emit, s_scan, nullptr);
#pragma unroll
	for (int k = 0; k < ADD_IPT; ++k) {
		if (!out[k]) continue;
		orow[o] = (int32_t)(key[k] >> 32);
		ocol[o] = (int32_t)(uint32_t)key[k];
		oval[o] = acc[k];
		++o;
	}
}

// op(X) as a sorted stream; *sorted: a sort ran.  lead = 1 for 'T'.
static void add_stream(spsamd_ctx *c, const spsamd_coo *X, int lead, bool force_sort, AddStream *out, bool *sorted)
{
	*out = AddStream();
	// a prepared handle of the same transpose is the stream; of the other, its consolidated tuples as stored
	const OperandView view = operand_view(c, X);
	if (view.prep && view.prep->lead == lead && !force_sort) { const ConMat &m = view.prep->m; out->row = m.row; out->col = m.col; out->val = m.val; out->n = m.nnz; return; }
	X = &view.coo;
	const size_t n = X->nnz;
	if (n == 0) return;
	const uint64_t shape[2] = {X->shape0, X->shape1};
	const PlainStream ps = plain_stream(c, *X, lead);
	const int32_t *major = ps.major, *minor = ps.minor;
	const double *dv = ps.val;
	// a SINK_COO result of this context handed back in is in the order its sort0 names; anything else: as inspected
	const bool ordered = ps.own_result ? X->sort0 == lead : !(ps.flags & 32u);
	// strictly in (minor, major) order -- a row-major matrix used with 'T': the stable passes over the major digits alone
	// leave equal majors in storage order, which is minor order (as consolidate_operand does)
	const int low_bit = !ps.own_result && !(ps.flags & 4u) ? -1 : 0;
	if (ordered && !force_sort) { out->row = major; out->col = minor; out->val = dv; out->n = (uint32_t)n; return; }
	// one stable radix sort on (major, minor), storage position as payload; the indices come back out of the sorted keys,
	// so only the value is gathered from storage
	const int mb = bits_of(shape[1 - lead]), Mb = bits_of(shape[lead]);
	PairSort sort(c, n);
	build_keys(c, major, minor, n, mb, sort.keys);
	sort.run(mb + Mb, low_bit < 0 ? mb : 0);
	int32_t *row = c->arena.get<int32_t>(n), *col = c->arena.get<int32_t>(n);
	double *val = c->arena.get<double>(n);
	gather_sorted(c, sort.sorted(), dv, n, mb, row, col, val);
	out->row = row; out->col = col; out->val = val; out->n = (uint32_t)n;
	*sorted = true;
}

template <int MODE>
static void launch_merge(spsamd_ctx *c, uint32_t ntiles, const AddStream &a, const AddStream &b, double alpha, double beta,
	int zero_nan, const FirstKept *first, const uint32_t *split, uint32_t *tile_count, const uint32_t *tile_off,
	int32_t *orow, int32_t *ocol, double *oval)
{
	k_add_merge<MODE><<<dim3(ntiles), dim3(ADD_NT), 0, c->stream>>>(a, b, alpha, beta, zero_nan, first, split, tile_count, tile_off, orow, ocol, oval);
	SPS_LAUNCH_CHECK();
}

void add_matrices(spsamd_ctx *c, double alpha, const spsamd_coo *A, char transpose_A, double beta, const spsamd_coo *B,
	char transpose_B, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	check_sink_args(duplicate_policy, sink_kind);
	std::memset(res, 0, sizeof(*res));
	const int la = transpose_A == 'T' ? 1 : 0, lb = transpose_B == 'T' ? 1 : 0;
	const uint64_t ash[2] = {A->shape0, A->shape1}, bsh[2] = {B->shape0, B->shape1};
	const uint64_t nrow = ash[la], ncol = ash[1 - la];
	if (nrow != bsh[lb] || ncol != bsh[1 - lb]) {
		char buf[200];
		std::snprintf(buf, sizeof buf, "Shapes of op(A) (%llu x %llu) and op(B) (%llu x %llu) must match!", (unsigned long long)nrow,
			(unsigned long long)ncol, (unsigned long long)bsh[lb], (unsigned long long)bsh[1 - lb]);
		throw Error{SPSAMD_EDIM, buf};
	}
	const uint64_t na = operand_view(c, A).coo.nnz, nb = operand_view(c, B).coo.nnz;
	if (na + nb >= (uint64_t(1) << 31))
		throw Error{SPSAMD_EINVAL, "nnz(A) + nnz(B) is 2^31 or more: the result would not be a legal operand"};
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	res->shape0 = permute ? ncol : nrow;
	res->shape1 = permute ? nrow : ncol;
	res->nnz_a = na; res->nnz_b = nb;
	if (na + nb == 0) return;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	if (coo) { const spsamd_coo *ops[2] = {A, B}; pick_output_set(c, ops, 2); }
	const bool force_sort = c->tune.add_path == 1;
	AddStream sa, sb;
	bool sorted_a = false, sorted_b = false;
	add_stream(c, A, la, force_sort, &sa, &sorted_a);
	add_stream(c, B, lb, force_sort, &sb, &sorted_b);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));

	const uint64_t n = (uint64_t)sa.n + sb.n;
	const uint32_t ntiles = (uint32_t)((n + ADD_TILE - 1) / ADD_TILE);
	FirstKept *first = nullptr;
	if (zero_nan) {
		uint32_t *idx = c->arena.get<uint32_t>(2);
		first = c->arena.get<FirstKept>(1);
		fill_u32(c, idx, 0xFFFFFFFFu, 2);
		if (sa.n) { k_add_first_idx<<<dim3(std::min(grid_for(sa.n), 1024u)), dim3(256), 0, st>>>(sa.val, sa.n, alpha, idx); SPS_LAUNCH_CHECK(); }
		if (sb.n) { k_add_first_idx<<<dim3(std::min(grid_for(sb.n), 1024u)), dim3(256), 0, st>>>(sb.val, sb.n, beta, idx + 1); SPS_LAUNCH_CHECK(); }
		k_add_first_pick<<<dim3(1), dim3(1), 0, st>>>(sa, sb, idx, first);
		SPS_LAUNCH_CHECK();
	}
	uint32_t *split = c->arena.get<uint32_t>((size_t)ntiles + 1);
	uint32_t *tile_count = c->arena.get<uint32_t>((size_t)ntiles + 1), *tile_off = c->arena.get<uint32_t>((size_t)ntiles + 1);
	merge_partition(c, sa, sb, ntiles, split);
	launch_merge<ADD_COUNT>(c, ntiles, sa, sb, alpha, beta, zero_nan, first, split, tile_count, nullptr, nullptr, nullptr, nullptr);
	uint32_t total;
	const CooOut o = counted_output(c, tile_count, tile_off, ntiles, coo, &total);
	switch (duplicate_policy) {
	case SPSAMD_ADD: launch_merge<SPSAMD_ADD>(c, ntiles, sa, sb, alpha, beta, zero_nan, first, split, nullptr, tile_off, o.row, o.col, o.val); break;
	case SPSAMD_REPLACE: launch_merge<SPSAMD_REPLACE>(c, ntiles, sa, sb, alpha, beta, zero_nan, first, split, nullptr, tile_off, o.row, o.col, o.val); break;
	default: launch_merge<SPSAMD_LEAVE_ALONE>(c, ntiles, sa, sb, alpha, beta, zero_nan, first, split, nullptr, tile_off, o.row, o.col, o.val); break;
	}
	deliver_stored(c, res, o, total, nrow, coo, permute, sink_flags);
	if (sorted_a || sorted_b) SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
}

} // namespace spsamd
