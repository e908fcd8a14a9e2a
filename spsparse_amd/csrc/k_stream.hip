// k_stream.hip -- spsamd_multiply_stream: the product cut into blocks of whole rows of op(A), each computed by the ordinary
// pipeline (spgemm_once) into one of two device output sets while the other set's block is copied to the host and handed
// to the callback.  The reference's loop makes the rows of C independent (multiply_sparse.hpp:192): a block of rows is a
// product of its own, and their outputs, one after the other, are C's tuples in order.
//
// Once per call: consolidation of both operands, the scale vectors, B's derived structures (row pointer, packed tuples and --
// where a row may be heavy -- the column-window index; the window-major copy is built by the first block with a heavy row
// and kept), the per-row bounds, their scan (prims.hip's, 64 bits in and out: this file has no scan kernel of its own) and
// the block boundaries.  Per block: the numeric pipeline on a row slice of A.
//
// Threads: a worker thread computes the blocks in order (the pipeline synchronises with the host between its stages); the
// calling thread copies each finished block to pinned staging on a copy stream of its own, chunk by chunk, and calls the
// callback.  Block k + 2 reuses block k's output set once the calling thread has copied block k out.
#include "spgemm_host.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace spsamd {

// ====================================================================== per-row bounds

// length of the op(B) row each tuple of op(A) selects
__global__ void k_stream_tuple_len(const int32_t *acol, const uint32_t *bptr, uint32_t n, uint32_t *len)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e < n) { const int32_t k = acol[e]; len[e] = bptr[k + 1] - bptr[k]; }
}

struct BoundStats { unsigned long long max_bound, max_p, heavy; };

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
	return v;
}

// P_r = pref[aptr[r+1]] - pref[aptr[r]] (products of row r), bound_r = min(P_r, ncol); the largest bound, the largest P_r and
// the rows with P_r above the mid class (the heavy rows a block may meet)
__global__ void k_stream_row_bound(const uint32_t *aptr, const int64_t *pref, uint64_t nrow, uint64_t ncol,
	unsigned long long *bound, BoundStats *bs)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long p = 0, b = 0, h = 0;
	if (r < nrow) {
		p = (unsigned long long)(pref[aptr[r + 1]] - pref[aptr[r]]);
		b = p < ncol ? p : ncol;
		h = p > MID_MAX ? 1ull : 0ull;
		bound[r] = b;
	}
	b = wave_max_u64(b); p = wave_max_u64(p); h = wave_reduce_sum(h);
	if (lane_id() == 0) {
		if (b > *(volatile unsigned long long *)&bs->max_bound) atomicMax(&bs->max_bound, b);
		if (p > *(volatile unsigned long long *)&bs->max_p) atomicMax(&bs->max_p, p);
		if (h) atomicAdd(&bs->heavy, h);
	}
}

// ====================================================================== block boundaries

// next[r]: the end of a block that starts at row r -- the largest e in (r, n] with S[e] - S[r] <= budget (S the exclusive scan
// of the bounds; every bound is <= budget, so e > r)
__global__ void k_stream_next(const unsigned long long *S, uint64_t n, unsigned long long budget, uint32_t *next)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n) return;
	const unsigned long long s = S[r];
	const unsigned long long lim = s + budget < s ? ~0ull : s + budget;
	uint64_t lo = r + 1, hi = n;
	while (lo < hi) {
		const uint64_t mid = (lo + hi + 1) >> 1;
		if (S[mid] <= lim) lo = mid; else hi = mid - 1;
	}
	next[r] = (uint32_t)lo;
}

// the chain of blocks from row 0: first row, first tuple of op(A) and bound sum of each (one thread: a dependent load per block)
__global__ void k_stream_walk(const uint32_t *next, const unsigned long long *S, const uint32_t *aptr, uint64_t n,
	uint32_t *brow, uint32_t *btup, unsigned long long *bsum, unsigned long long *count)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	uint64_t b = 0, k = 0;
	while (b < n) {
		const uint64_t e = next[b];
		brow[k] = (uint32_t)b; btup[k] = aptr[b]; bsum[k] = S[e] - S[b];
		++k; b = e;
	}
	brow[k] = (uint32_t)n; btup[k] = aptr[n]; bsum[k] = 0;
	*count = k;
}

// ====================================================================== driver

static void alloc_exact(DevBuf &d, size_t bytes)
{
	bytes = (std::max<size_t>(bytes, 1) + 255) / 256 * 256;
	hipError_t e = hipMalloc(&d.p, bytes);
	if (e != hipSuccess) {
		(void)hipGetLastError();
		d.p = nullptr; d.cap = 0;
		throw Error{SPSAMD_ENOMEM, "hipMalloc of " + std::to_string(bytes) + " bytes for a block's output failed: " + hipGetErrorString(e)};
	}
	d.cap = bytes;
}

static void add_totals(spsamd_result &acc, const spsamd_result &rs)
{
	acc.nnz += rs.nnz; acc.products += rs.products;
	acc.rows_light += rs.rows_light; acc.rows_mid += rs.rows_mid; acc.rows_heavy += rs.rows_heavy;
	acc.products_light += rs.products_light; acc.products_mid += rs.products_mid; acc.products_heavy += rs.products_heavy;
	acc.tuples_light += rs.tuples_light; acc.tuples_mid += rs.tuples_mid; acc.tuples_heavy += rs.tuples_heavy;
	acc.products_dense += rs.products_dense; acc.products_tiles += rs.products_tiles; acc.products_direct += rs.products_direct;
	acc.cells_hash += rs.cells_hash; acc.cells_dense += rs.cells_dense; acc.window = std::max(acc.window, rs.window);
	acc.ms_symbolic += rs.ms_symbolic; acc.ms_numeric += rs.ms_numeric; acc.ms_light += rs.ms_light; acc.ms_mid += rs.ms_mid;
	acc.ms_heavy += rs.ms_heavy; acc.ms_dense += rs.ms_dense; acc.ms_tiles += rs.ms_tiles; acc.ms_direct += rs.ms_direct;
}

constexpr size_t STREAM_CHUNK = size_t(1) << 22;       // tuples per host chunk: two pinned chunks of 64 MiB

int multiply_stream(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, int duplicate_policy, int zero_nan,
	int sink_flags, size_t block_tuples, spsamd_chunk_fn cb, void *user,
	spsamd_result *res, spsamd_stream_stats *stats)
{
	using Clock = std::chrono::steady_clock;
	const Clock::time_point t_call = Clock::now();
	auto ms_since = [](Clock::time_point t) { return std::chrono::duration<float, std::milli>(Clock::now() - t).count(); };
	if (duplicate_policy < 0 || duplicate_policy > 2) throw Error{SPSAMD_EINVAL, "bad duplicate_policy"};
	if (sink_flags & SPSAMD_SINK_ROWSTATS) throw Error{SPSAMD_EINVAL, "SINK_ROWSTATS belongs to the digest sink: the streamed product delivers tuples"};
	std::memset(res, 0, sizeof(*res));
	spsamd_stream_stats st{};
	st.block_tuples = block_tuples ? (uint64_t)block_tuples : (uint64_t)SPSAMD_STREAM_DEFAULT_BLOCK;
	if (stats) *stats = st;
	const unsigned long long budget = st.block_tuples;
	// shape, inner dimension and short-circuits exactly as spsamd_multiply (multiply_sparse.hpp:167-184)
	const bool permute = (sink_flags & SPSAMD_SINK_PERMUTE) != 0;
	const ProductFrame f(A, transpose_A, B, transpose_B, permute);
	const int a0 = f.a0, bk = f.bk, bj = f.bj;
	res->shape0 = f.shape0; res->shape1 = f.shape1;
	f.check_inner("B");
	auto finish = [&](int rc) { st.ms_wall = ms_since(t_call); if (stats) *stats = st; return rc; };
	if (product_is_empty(C, scalei, A, scalej, B, scalek)) return finish(SPSAMD_OK);
	// the same refusal as spsamd_multiply's, although this call writes neither output set
	const spsamd_coo *ops[2] = {A, B};
	if (output_set_aliased(c, 0, ops, 2) && output_set_aliased(c, 1, ops, 2))
		throw Error{SPSAMD_EINVAL, "both result buffers of this context are operands of the call: copy one of them out first (spsamd_memcpy)"};

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t s0 = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], s0));
	MultiplyArgs a;
	a.C = C; a.sink_kind = SPSAMD_SINK_COO; a.sink_flags = sink_flags & (SPSAMD_SINK_ORDERED | SPSAMD_SINK_EXACT_PATTERN);
	Prepared *hpa = nullptr, *hpb = nullptr;
	consolidate_operand(c, A, a0, a0, duplicate_policy, zero_nan, &a.A, &hpa);
	if (a0 == bk && same_operand(A, B) && (!zero_nan || hpa)) { a.B = a.A; hpb = hpa; }
	else consolidate_operand(c, B, bk, bj, duplicate_policy, zero_nan, &a.B, &hpb);
	upload_scale(c, scalei, f.nrow, "scalei", &a.si);
	upload_scale(c, scalej, f.inner, "scalej", &a.sj);
	upload_scale(c, scalek, f.ncol, "scalek", &a.sk);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], s0));
	const ConMat Am = a.A, Bm = a.B;
	res->nnz_a = Am.nnz; res->nnz_b = Bm.nnz;
	if (Am.nnz == 0 || Bm.nnz == 0) {
		SPS_HIP(hipStreamSynchronize(s0));
		res->ms_consolidate = res->ms_total = elapsed(c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]);
		return finish(SPSAMD_OK);
	}

	// ---- op(B)'s derived structures, once for all blocks: a prepared operand's own, or a record of this call's
	struct OwnB { Prepared p; ~OwnB() { p.release(); } } own_b;
	own_b.p.ctx = c; own_b.p.owns = true; own_b.p.m = Bm; own_b.p.lead = bk;
	Prepared *pb = hpb;
	if (!pb) {
		own_b.p.reserve(((size_t)Bm.nnz + 64) * (12 + 4) + (Bm.nrow + 66) * 4 + 65536);
		pb = &own_b.p;
		prepared_row_structure(c, pb);
	}
	prepared_btup(c, pb);
	const uint32_t *bptr = pb->rowptr;

	// ---- per-row bounds, their scan, the blocks
	const uint64_t n = Am.nrow;
	uint32_t *len = c->arena.get<uint32_t>(Am.nnz);
	int64_t *pref = c->arena.get<int64_t>((size_t)Am.nnz + 1);
	k_stream_tuple_len<<<dim3(grid_for(Am.nnz)), dim3(256), 0, s0>>>(Am.col, bptr, Am.nnz, len);
	SPS_LAUNCH_CHECK();
	scan_exclusive_u32_i64(c, len, pref, Am.nnz);
	const uint32_t *aptr = dense_rowptr(c, Am, 0);
	unsigned long long *bound = c->arena.get<unsigned long long>(n);
	BoundStats *bs = c->arena.get<BoundStats>(1);
	fill_zero(c, bs, sizeof(BoundStats));
	k_stream_row_bound<<<dim3(grid_for(n)), dim3(256), 0, s0>>>(aptr, pref, n, Bm.ncol, bound, bs);
	SPS_LAUNCH_CHECK();
	const BoundStats hb = read_back(c, bs);
	res->ms_consolidate = elapsed(c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]);
	if (hb.max_bound > budget) {
		char buf[200];
		std::snprintf(buf, sizeof buf, "a row of op(A) can produce %llu tuples, more than block_tuples = %llu: the smallest budget that works is %llu",
			hb.max_bound, budget, hb.max_bound);
		throw Error{SPSAMD_ECAPACITY, buf};
	}
	unsigned long long *S = c->arena.get<unsigned long long>(n + 1);
	scan_exclusive_u64_u64(c, bound, S, n);                 // S[n] = the sum of all bounds
	uint32_t *next = c->arena.get<uint32_t>(n);
	k_stream_next<<<dim3(grid_for(n)), dim3(256), 0, s0>>>(S, n, budget, next);
	SPS_LAUNCH_CHECK();
	uint32_t *brow = c->arena.get<uint32_t>(n + 1), *btup = c->arena.get<uint32_t>(n + 1);
	unsigned long long *bsum = c->arena.get<unsigned long long>(n + 1), *bcount = c->arena.get<unsigned long long>(1);
	k_stream_walk<<<dim3(1), dim3(64), 0, s0>>>(next, S, aptr, n, brow, btup, bsum, bcount);
	SPS_LAUNCH_CHECK();
	const uint64_t nb = read_back(c, bcount);
	std::vector<uint32_t> htup(nb + 1);
	std::vector<unsigned long long> hsum(nb + 1);
	SPS_HIP(hipMemcpyAsync(htup.data(), btup, (nb + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s0));
	SPS_HIP(hipMemcpyAsync(hsum.data(), bsum, (nb + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s0));
	SPS_HIP(hipStreamSynchronize(s0));
	st.blocks = nb;
	const uint64_t maxblk = *std::max_element(hsum.begin(), hsum.end());

	// ---- two output sets of the largest block's bound, pinned staging, the copy stream
	struct Sets { OutSet s[2]; ~Sets() { s[0].release(); s[1].release(); } } sets;
	for (int q = 0; q < (nb > 1 ? 2 : 1); ++q) {
		alloc_exact(sets.s[q].i, maxblk * sizeof(int32_t));
		alloc_exact(sets.s[q].j, maxblk * sizeof(int32_t));
		alloc_exact(sets.s[q].v, maxblk * sizeof(double));
	}
	const size_t chunk = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(STREAM_CHUNK, maxblk));
	if (2 * chunk * 16 > c->stream_pinned_cap) {
		if (c->stream_pinned) (void)hipHostFree(c->stream_pinned);
		c->stream_pinned = nullptr; c->stream_pinned_cap = 0;
		hipError_t e = hipHostMalloc(&c->stream_pinned, 2 * chunk * 16, hipHostMallocDefault);
		if (e != hipSuccess) { (void)hipGetLastError(); c->stream_pinned = nullptr; throw Error{SPSAMD_ENOMEM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e)}; }
		c->stream_pinned_cap = 2 * chunk * 16;
	}
	char *pinned = (char *)c->stream_pinned;
	if (hb.max_p > MID_MAX) {
		// the column-window index the heavy rows need, now -- after the output sets, so that its budget (80 % of the free memory)
		// counts them -- and before delivery: a product that would go by column blocks is refused here
		try { (void)heavy_b_index(c, Bm, bptr, 1u, hb.heavy, pb); }
		catch (const TooWide &) {
			throw Error{SPSAMD_EINVAL, "the product would go by column blocks of op(B) (a row of more than 4096 products and more than 2^25 "
				"columns, or window indices over the budget): not supported by the streamed product"};
		}
	}
	struct Copy {
		hipStream_t s = nullptr; hipEvent_t ev[2] = {}, tb[2] = {};
		~Copy() {
			if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
			for (auto e : ev) if (e) (void)hipEventDestroy(e);
			for (auto e : tb) if (e) (void)hipEventDestroy(e);
		}
	} cp;
	SPS_HIP(hipStreamCreateWithFlags(&cp.s, hipStreamNonBlocking));
	for (auto &e : cp.ev) SPS_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
	for (auto &e : cp.tb) SPS_HIP(hipEventCreate(&e));
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], s0));
	SPS_HIP(hipEventSynchronize(c->ev[EV_SYMBOLIC]));
	const float ms_setup = elapsed(c->ev[EV_BEGIN], c->ev[EV_SYMBOLIC]);           // consolidation, B's structures, bounds and blocks

	// ---- the worker computes the blocks; this thread delivers them
	struct Done { uint64_t nnz = 0; const int32_t *i = nullptr, *j = nullptr; const double *v = nullptr; };
	std::vector<Done> done(nb);
	std::mutex mu;
	std::condition_variable cv;
	int64_t ready = -1, freed = -1;
	bool stop = false, failed = false;
	int err_code = 0;
	std::string err_msg;
	spsamd_result acc{};
	float ms_dev = 0;
	uint64_t ws_peak = c->arena.call_used;
	const Arena::Mark base = c->arena.mark();
	auto fail = [&](int code, std::string msg) {
		std::lock_guard<std::mutex> lk(mu);
		failed = true; err_code = code; err_msg = std::move(msg);
		cv.notify_all();
	};
	std::thread worker([&] {
		try {
			SPS_HIP(hipSetDevice(c->device));
			for (uint64_t k = 0; k < nb; ++k) {
				{
					std::unique_lock<std::mutex> lk(mu);
					cv.wait(lk, [&] { return stop || (int64_t)k - 2 <= freed; });
					if (stop) return;
				}
				MultiplyArgs as = a;
				as.pa = nullptr; as.pb = pb; as.out = &sets.s[k & 1];
				const uint32_t t0 = htup[k], t1 = htup[k + 1];
				as.A.row = Am.row + t0; as.A.col = Am.col + t0; as.A.val = Am.val + t0; as.A.nnz = t1 - t0;
				spsamd_result rs{};
				SPS_HIP(hipEventRecord(cp.tb[0], c->stream));
				if (as.A.nnz) spgemm_once(c, as, &rs);
				SPS_HIP(hipEventRecord(cp.tb[1], c->stream));
				SPS_HIP(hipEventSynchronize(cp.tb[1]));
				ms_dev += elapsed(cp.tb[0], cp.tb[1]);
				ws_peak = std::max<uint64_t>(ws_peak, c->arena.call_used);
				c->arena.rewind(base);
				add_totals(acc, rs);
				std::lock_guard<std::mutex> lk(mu);
				done[k] = Done{rs.nnz, rs.idx0, rs.idx1, rs.val};
				ready = (int64_t)k;
				cv.notify_all();
			}
		}
		catch (const TooWide &) { fail(SPSAMD_EINVAL, "a block would go by column blocks of op(B): not supported by the streamed product"); }
		catch (const Error &e) { fail(e.code, e.msg); }
		catch (const std::bad_alloc &) { fail(SPSAMD_ENOMEM, "host allocation failed"); }
		catch (const std::exception &e) { fail(SPSAMD_EINVAL, e.what()); }
	});
	struct Join {
		std::thread &t; std::mutex &mu; std::condition_variable &cv; bool &stop;
		~Join() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); if (t.joinable()) t.join(); }
	} join{worker, mu, cv, stop};

	int rc = 0;
	float ms_cb = 0;
	int buf = 0;
	for (uint64_t k = 0; k < nb && !rc; ++k) {
		Done d;
		{
			std::unique_lock<std::mutex> lk(mu);
			cv.wait(lk, [&] { return ready >= (int64_t)k || failed; });
			if (ready < (int64_t)k) break;
			d = done[k];
		}
		st.max_block_nnz = std::max<uint64_t>(st.max_block_nnz, d.nnz);
		auto issue = [&](uint64_t o, int b) {
			const size_t m = (size_t)std::min<uint64_t>(chunk, d.nnz - o);
			char *hb = pinned + (size_t)b * chunk * 16;
			SPS_HIP(hipMemcpyAsync(hb, d.i + o, m * 4, hipMemcpyDeviceToHost, cp.s));
			SPS_HIP(hipMemcpyAsync(hb + chunk * 4, d.j + o, m * 4, hipMemcpyDeviceToHost, cp.s));
			SPS_HIP(hipMemcpyAsync(hb + chunk * 8, d.v + o, m * 8, hipMemcpyDeviceToHost, cp.s));
			SPS_HIP(hipEventRecord(cp.ev[b], cp.s));
		};
		if (d.nnz) issue(0, buf);
		for (uint64_t o = 0; o < d.nnz; o += chunk, buf ^= 1) {
			const size_t m = (size_t)std::min<uint64_t>(chunk, d.nnz - o);
			if (o + chunk < d.nnz) issue(o + chunk, buf ^ 1);
			SPS_HIP(hipEventSynchronize(cp.ev[buf]));
			const char *hb = pinned + (size_t)buf * chunk * 16;
			const int32_t *hi = (const int32_t *)hb, *hj = (const int32_t *)(hb + chunk * 4);
			const Clock::time_point t_cb = Clock::now();
			rc = permute ? cb(user, hj, hi, (const double *)(hb + chunk * 8), m) : cb(user, hi, hj, (const double *)(hb + chunk * 8), m);
			ms_cb += ms_since(t_cb);
			if (rc) break;
		}
		SPS_HIP(hipStreamSynchronize(cp.s));
		std::lock_guard<std::mutex> lk(mu);
		freed = (int64_t)k;
		cv.notify_all();
	}
	{ std::lock_guard<std::mutex> lk(mu); stop = true; }
	cv.notify_all();
	worker.join();
	SPS_HIP(hipStreamSynchronize(cp.s));
	SPS_HIP(hipStreamSynchronize(c->stream));
	for (int q = 0; q < 2; ++q) st.device_output_bytes += sets.s[q].i.cap + sets.s[q].j.cap + sets.s[q].v.cap;
	st.ms_device = ms_dev;
	st.ms_callback = ms_cb;
	if (rc) return finish(rc);
	if (failed) { finish(0); throw Error{err_code, err_msg}; }
	const spsamd_result keep = *res;
	*res = acc;
	res->shape0 = keep.shape0; res->shape1 = keep.shape1;
	res->nnz_a = keep.nnz_a; res->nnz_b = keep.nnz_b;
	res->ms_consolidate = keep.ms_consolidate;
	res->ms_total = ms_setup + ms_dev;
	res->workspace_bytes = ws_peak;
	return finish(SPSAMD_OK);
}

} // namespace spsamd
