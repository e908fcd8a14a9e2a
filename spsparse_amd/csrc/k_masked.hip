// k_masked.hip -- C = op(A) * op(B) on a given pattern M only (spsamd_multiply_masked, include/spsparse_amd.h).
//
// The reference's loop (multiply_sparse.hpp:192-243) runs over the rows i of op(A) and, inside each, over the columns j
// of op(B) (op(B) consolidated by columns, :168); for each pair it joins the two sorted lists in ascending k and sums
// `a * b` (`a * sj * b` under scalej) serially from 0.  A masked product is that loop run over the pairs (i, j) of M
// only, so every value below is the reference's own, bit for bit: every kernel sums the matched products of a key in
// ascending k, one after the other, with the x86 NaN rules of x86fp.h (no tree reduction anywhere).
//
// Device path:
//   1. op(A) consolidated by rows, op(B) by its columns (the reference's Acon / Bcon), a dense row pointer over each;
//   2. M's keys row-major and duplicate-free (checked in place when already in order, else one radix sort), and M's
//      dense row pointer;
//   3. k_masked_rows / k_masked_classify: every key whose A row or B column is empty, or whose row or column scale is
//      missing or zero, is dropped; the rest go to one of three kernels by cost (la = |A_i|, lb = |B_j|):
//        entry  one lane per key: both lists in registers when short, else walks the shorter and gallops the longer;
//        row    one workgroup per mask row: A_i staged in LDS once, one lane per key (only when forced, masked_path = 2);
//        wave   one wave per key where both lists are long: 64 consecutive elements of the shorter list per step, each
//               lane searches the longer one, the matches go to LDS in k order (ballot + mbcnt) and lane 0 folds them;
//   4. sum and emit flag (sum != 0, NaN kept: :238) per key, then the COO sink compacts, the DIGEST sink reduces.
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

namespace spsamd {

// Class thresholds
constexpr uint32_t MASK_ROW_CAP = 4096;        // longest A_i the row kernel stages: 48 KiB of LDS, three workgroups per CU
constexpr uint32_t MASK_WAVE_MIN = 32;         // auto: a key goes to the wave kernel when both lists are at least this long
// (auto sends no row to the row kernel: measured slower than the entry kernel on both benchmark workloads; masked_path = 2
// forces it)

enum : uint8_t { MCLS_NONE = 0, MCLS_ENTRY = 1, MCLS_ROW = 2, MCLS_WAVE = 3 };

// What every evaluation kernel reads
struct MaskedArgs {
	const uint32_t *arp;            // op(A): row pointer over rows(op(A)) + 1
	const int32_t *acol;            //        k of each tuple, ascending inside a row
	const double *aval;
	const uint32_t *brp;            // op(B) by columns: pointer over cols(op(B)) + 1
	const int32_t *bcol;            //        k of each tuple, ascending inside a column
	const double *bval;
	const int32_t *mi, *mj;         // M's keys, row-major, each once
	const int32_t *sj_pos;          // scalej: dense position per k or -1 (null: no scalej)
	const double *sj_val;
	double *sum;                    // per key
	uint8_t *emit;                  // per key: the reference emits it (sum != 0)
	unsigned long long *products;   // matched and summed terms, all keys
};

// One term of the join: (a * sj) * b under scalej (multiply_sparse.hpp:228), a * b without (:235).  false: k is not in
// scalej (the join3 skips it).
__device__ __forceinline__ bool masked_term(const MaskedArgs &g, int32_t k, double a, double b, double *p)
{
	if (g.sj_pos) {
		const int32_t q = g.sj_pos[k];
		if (q < 0) return false;
		*p = ref_mul(ref_mul(a, g.sj_val[q]), b);
	} else *p = ref_mul(a, b);
	return true;
}

// First position in [lo, hi) whose key is >= k, galloping from lo (the cursor only moves forward)
__device__ __forceinline__ uint32_t gallop(const int32_t *key, uint32_t lo, uint32_t hi, int32_t k)
{
	if (lo >= hi || key[lo] >= k) return lo;
	uint32_t step = 1;
	while (lo + step < hi && key[lo + step] < k) { lo += step; step <<= 1; }
	uint32_t l = lo + 1, h = min(lo + step, hi);              // key[lo] < k: the answer lies in (lo, h]
	while (l < h) { const uint32_t m = (l + h) >> 1; if (key[m] < k) l = m + 1; else h = m; }
	return l;
}

__device__ __forceinline__ uint32_t lower_bound_i32(const int32_t *key, uint32_t lo, uint32_t hi, int32_t k)
{
	while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (key[m] < k) lo = m + 1; else hi = m; }
	return lo;
}

// Serial ascending-k sum of one key: walk the shorter list, gallop through the longer one.  A's list may be a copy in
// LDS (ak / av from position 0).
__device__ __forceinline__ double masked_serial(const MaskedArgs &g, const int32_t *ak, const double *av, uint32_t a0, uint32_t a1,
	uint32_t b0, uint32_t b1, unsigned long long *cnt)
{
	double sum = 0.0;
	double p;
	if (a1 - a0 <= b1 - b0) {
		uint32_t q = b0;
		for (uint32_t e = a0; e < a1 && q < b1; ++e) {
			const int32_t k = ak[e];
			q = gallop(g.bcol, q, b1, k);
			if (q < b1 && g.bcol[q] == k && masked_term(g, k, av[e], g.bval[q], &p)) { sum = ref_add(sum, p); ++*cnt; }
		}
	} else {
		uint32_t q = a0;
		for (uint32_t f = b0; f < b1 && q < a1; ++f) {
			const int32_t k = g.bcol[f];
			q = gallop(ak, q, a1, k);
			if (q < a1 && ak[q] == k && masked_term(g, k, av[q], g.bval[f], &p)) { sum = ref_add(sum, p); ++*cnt; }
		}
	}
	return sum;
}

__device__ __forceinline__ void flush_products(const MaskedArgs &g, unsigned long long cnt)
{
	cnt = wave_reduce_sum(cnt);
	if (lane_id() == 0 && cnt) atomicAdd(g.products, cnt);
}

// Both lists short (at most MASK_SHORT tuples): all loads issued at once, the join done in registers (no dependent
// gallop loads).  A's elements in ascending k, each matched against all of B's: the terms still arrive in ascending k.
constexpr uint32_t MASK_SHORT = 8;

__device__ __forceinline__ double masked_short(const MaskedArgs &g, uint32_t a0, uint32_t la, uint32_t b0, uint32_t lb,
	unsigned long long *cnt)
{
	int32_t ka[MASK_SHORT], kb[MASK_SHORT];
	double va[MASK_SHORT], vb[MASK_SHORT];
#pragma unroll
	for (uint32_t e = 0; e < MASK_SHORT; ++e) {
		ka[e] = e < la ? g.acol[a0 + e] : -1;
		va[e] = e < la ? g.aval[a0 + e] : 0.0;
		kb[e] = e < lb ? g.bcol[b0 + e] : -2;
		vb[e] = e < lb ? g.bval[b0 + e] : 0.0;
	}
	double sum = 0.0, p;
#pragma unroll
	for (uint32_t e = 0; e < MASK_SHORT; ++e) {
		bool hit = false;
		double b = 0.0;
#pragma unroll
		for (uint32_t f = 0; f < MASK_SHORT; ++f)
			if (kb[f] == ka[e]) { hit = true; b = vb[f]; }
		if (hit && masked_term(g, ka[e], va[e], b, &p)) { sum = ref_add(sum, p); ++*cnt; }
	}
	return sum;
}

// entry: one lane per key of the list.  The list is in key order, so the keys of one mask row sit in adjacent lanes and
// share A_i's cache lines.
__global__ void __launch_bounds__(256) k_masked_entry(MaskedArgs g, const uint32_t *__restrict__ list, uint32_t n)
{
	unsigned long long cnt = 0;
	// (a grid stride: the product counter takes one atomic per wave of the launch -- one per wave of KEYS serialised 1.3 M
	// atomics on one address, 13 ms of Poisson 4096^2)
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
		const uint32_t key = list[t];
		const int32_t i = g.mi[key], j = g.mj[key];
		const uint32_t a0 = g.arp[i], a1 = g.arp[i + 1], b0 = g.brp[j], b1 = g.brp[j + 1];
		const double s = a1 - a0 <= MASK_SHORT && b1 - b0 <= MASK_SHORT ? masked_short(g, a0, a1 - a0, b0, b1 - b0, &cnt)
			: masked_serial(g, g.acol, g.aval, a0, a1, b0, b1, &cnt);
		g.sum[key] = s;
		g.emit[key] = s != 0;                                           // NaN: emitted (multiply_sparse.hpp:238)
	}
	flush_products(g, cnt);
}

// row: one workgroup per mask row of the list; A_i (at most MASK_ROW_CAP tuples) staged in LDS, one lane per key of the
// row that the classification gave this kernel.
__global__ void __launch_bounds__(256) k_masked_row(MaskedArgs g, const int32_t *__restrict__ rows, uint32_t nrows,
	const uint32_t *__restrict__ mrp, const uint8_t *__restrict__ cls)
{
	__shared__ int32_t s_k[MASK_ROW_CAP];
	__shared__ double s_a[MASK_ROW_CAP];
	unsigned long long cnt = 0;
	for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {            // (a grid stride: the launch stays far below 2^32 lanes)
		const int32_t i = rows[r];
		const uint32_t a0 = g.arp[i], la = min(g.arp[i + 1] - a0, MASK_ROW_CAP);      // (the classification keeps la <= the cap)
		__syncthreads();                                                  // the previous row's copy is no longer read
		for (uint32_t e = threadIdx.x; e < la; e += blockDim.x) { s_k[e] = g.acol[a0 + e]; s_a[e] = g.aval[a0 + e]; }
		__syncthreads();
		const uint32_t t1 = mrp[i + 1];
		for (uint32_t t = mrp[i] + threadIdx.x; t < t1; t += blockDim.x) {
			if (cls[t] != MCLS_ROW) continue;
			const int32_t j = g.mj[t];
			const double s = masked_serial(g, s_k, s_a, 0, la, g.brp[j], g.brp[j + 1], &cnt);
			g.sum[t] = s;
			g.emit[t] = s != 0;
		}
	}
	flush_products(g, cnt);
}

// wave: one wave per key of the list.  Step by step, 64 consecutive elements of the shorter list, one per lane; each lane
// binary-searches the longer list from where the previous step ended.  The matched products of the step are placed in
// LDS in lane order -- ascending k -- and lane 0 folds them into the sum left to right.
__global__ void __launch_bounds__(256) k_masked_wave(MaskedArgs g, const uint32_t *__restrict__ list, uint32_t n)
{
	__shared__ double s_p[4][64];
	const unsigned lane = lane_id(), wv = wave_id();
	unsigned long long total = 0;                                       // (uniform: summed popcounts)
	for (uint32_t w = blockIdx.x * 4 + wv; w < n; w += gridDim.x * 4) {    // (whole waves, no barrier: a grid stride)
	const uint32_t key = list[w];
	const int32_t i = g.mi[key], j = g.mj[key];
	const uint32_t a0 = g.arp[i], a1 = g.arp[i + 1], b0 = g.brp[j], b1 = g.brp[j + 1];
	const bool a_short = a1 - a0 <= b1 - b0;
	const int32_t *sk = a_short ? g.acol : g.bcol, *lk = a_short ? g.bcol : g.acol;
	const uint32_t s0 = a_short ? a0 : b0, s1 = a_short ? a1 : b1;
	const uint32_t l1 = a_short ? b1 : a1;
	uint32_t llo = a_short ? b0 : a0;
	double sum = 0.0;
	unsigned long long cnt = 0;
	for (uint32_t base = s0; base < s1 && llo < l1; base += 64) {
		const uint32_t e = base + lane;
		const bool ok = e < s1;
		const int32_t k = ok ? sk[e] : INT_MAX;
		const uint32_t pos = ok ? lower_bound_i32(lk, llo, l1, k) : l1;
		double p = 0.0;
		bool hit = ok && pos < l1 && lk[pos] == k;
		if (hit) hit = a_short ? masked_term(g, k, g.aval[e], g.bval[pos], &p) : masked_term(g, k, g.aval[pos], g.bval[e], &p);
		const uint64_t m = __ballot(hit);
		if (hit) s_p[wv][__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = p;
		__builtin_amdgcn_wave_barrier();
		const uint32_t nm = (uint32_t)__popcll(m);
		if (lane == 0)
			for (uint32_t q = 0; q < nm; ++q) sum = ref_add(sum, s_p[wv][q]);
		__builtin_amdgcn_wave_barrier();
		cnt += nm;
		// the next step's keys are above this step's last: its search starts at that key's position
		const int last = (int)min(63u, s1 - 1 - base);
		llo = (uint32_t)__builtin_amdgcn_readlane((int)pos, last);
	}
	if (lane == 0) {
		g.sum[key] = sum;
		g.emit[key] = sum != 0;
	}
	total += cnt;
	}
	if (lane == 0 && total) atomicAdd(g.products, total);
}

__device__ __forceinline__ bool scale_allowed(const int32_t *pos, const double *val, int32_t x)
{
	if (!pos) return true;
	const int32_t q = pos[x];
	return q >= 0 && val[q] != 0;                                       // missing or isnone: skipped (:195, :211)
}

// Which mask rows go to the row kernel
__global__ void __launch_bounds__(256) k_masked_rows(const uint32_t *__restrict__ mrp, const uint32_t *__restrict__ arp, uint64_t nrow,
	const int32_t *si_pos, const double *si_val, int path, uint8_t *__restrict__ rowflag)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= nrow) return;
	const uint32_t nk = mrp[i + 1] - mrp[i], la = arp[i + 1] - arp[i];
	bool ok = nk > 0 && la > 0 && la <= MASK_ROW_CAP && scale_allowed(si_pos, si_val, (int32_t)i);
	if (path != 2) ok = false;                                          // (auto: no row class)
	rowflag[i] = ok;
}

__global__ void __launch_bounds__(256) k_masked_classify(const int32_t *__restrict__ mi, const int32_t *__restrict__ mj, uint32_t nm,
	const uint32_t *__restrict__ arp, const uint32_t *__restrict__ brp, const int32_t *si_pos, const double *si_val,
	const int32_t *sk_pos, const double *sk_val, const uint8_t *__restrict__ rowflag, int path,
	uint8_t *__restrict__ cls, uint8_t *__restrict__ f_entry, uint8_t *__restrict__ f_wave)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nm) return;
	const int32_t i = mi[t], j = mj[t];
	const uint32_t la = arp[i + 1] - arp[i], lb = brp[j + 1] - brp[j];
	uint8_t c;
	if (la == 0 || lb == 0 || !scale_allowed(si_pos, si_val, i) || !scale_allowed(sk_pos, sk_val, j)) c = MCLS_NONE;
	else if (path == 3) c = MCLS_WAVE;
	else if (path == 1) c = MCLS_ENTRY;
	else if (path == 2) c = rowflag[i] ? MCLS_ROW : MCLS_ENTRY;
	else if (min(la, lb) >= MASK_WAVE_MIN) c = MCLS_WAVE;
	else c = rowflag[i] ? MCLS_ROW : MCLS_ENTRY;
	cls[t] = c;
	f_entry[t] = c == MCLS_ENTRY;
	f_wave[t] = c == MCLS_WAVE;
}

__global__ void __launch_bounds__(256) k_masked_lists(const uint8_t *__restrict__ f_entry, const uint8_t *__restrict__ f_wave,
	const uint32_t *__restrict__ off_entry, const uint32_t *__restrict__ off_wave, uint32_t nm,
	uint32_t *__restrict__ list_entry, uint32_t *__restrict__ list_wave)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nm) return;
	if (f_entry[t]) list_entry[off_entry[t]] = t;
	if (f_wave[t]) list_wave[off_wave[t]] = t;
}

__global__ void __launch_bounds__(256) k_masked_rowlist(const uint8_t *__restrict__ rowflag, const uint32_t *__restrict__ off, uint64_t nrow,
	int32_t *__restrict__ rows)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < nrow && rowflag[i]) rows[off[i]] = (int32_t)i;
}

// The emitted value: sum * C * a_scale * b_scale, left to right (multiply_sparse.hpp:242; a missing scale vector is 1)
__device__ __forceinline__ double masked_value(double s, double C, const int32_t *si_pos, const double *si_val,
	const int32_t *sk_pos, const double *sk_val, int32_t i, int32_t j)
{
	const double as = si_pos ? si_val[si_pos[i]] : 1.0, bs = sk_pos ? sk_val[sk_pos[j]] : 1.0;
	return ref_mul(ref_mul(ref_mul(s, C), as), bs);
}

__global__ void __launch_bounds__(256) k_masked_compact(const int32_t *__restrict__ mi, const int32_t *__restrict__ mj,
	const double *__restrict__ sum, const uint8_t *__restrict__ emit, const uint32_t *__restrict__ off, uint32_t nm, double C,
	const int32_t *si_pos, const double *si_val, const int32_t *sk_pos, const double *sk_val,
	int32_t *__restrict__ orow, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= nm || !emit[t]) return;
	const uint32_t o = off[t];
	const int32_t i = mi[t], j = mj[t];
	orow[o] = i; ocol[o] = j;
	oval[o] = masked_value(sum[t], C, si_pos, si_val, sk_pos, sk_val, i, j);
}

// DIGEST sink over the emitted keys: count, index hash, sum (and the per-row statistics under ROWSTATS)
__global__ void __launch_bounds__(256) k_masked_digest(const int32_t *__restrict__ mi, const int32_t *__restrict__ mj,
	const double *__restrict__ sum, const uint8_t *__restrict__ emit, uint32_t nm, double C,
	const int32_t *si_pos, const double *si_val, const int32_t *sk_pos, const double *sk_val,
	unsigned long long *acc, long long *row_nnz, double *row_sum, unsigned long long *row_hash)
{
	unsigned long long n = 0, h = 0;
	double s = 0;
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < nm; t += gridDim.x * blockDim.x) {
		if (!emit[t]) continue;
		const int32_t i = mi[t], j = mj[t];
		const double v = masked_value(sum[t], C, si_pos, si_val, sk_pos, sk_val, i, j);
		const unsigned long long x = mix64((uint32_t)i, (uint32_t)j);
		++n; h += x; s += v;
		if (row_nnz) { atomicAdd((unsigned long long *)&row_nnz[i], 1ull); atomicAdd(&row_sum[i], v); atomicAdd(&row_hash[i], x); }
	}
	n = wave_reduce_sum(n); h = wave_reduce_sum(h); s = wave_reduce_sum(s);
	if (lane_id() == 0) { atomicAdd(&acc[0], n); atomicAdd(&acc[1], h); atomicAdd((double *)&acc[2], s); }
}

void multiply_masked(spsamd_ctx *c, double C,
	const spsamd_vec *scalei, const spsamd_coo *A, char transpose_A,
	const spsamd_vec *scalej, const spsamd_coo *B, char transpose_B,
	const spsamd_vec *scalek, const spsamd_coo *M, int duplicate_policy, int zero_nan,
	int sink_kind, int sink_flags, spsamd_result *res)
{
	check_sink_args(duplicate_policy, sink_kind);
	std::memset(res, 0, sizeof(*res));
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	// op(A) by rows, op(B) by its columns (the reference's Bcon)
	const ProductFrame f(A, transpose_A, B, transpose_B, permute);
	const uint64_t nrow = f.nrow, ncol = f.ncol;
	res->shape0 = f.shape0; res->shape1 = f.shape1;
	f.check_inner("B");
	if (M->shape0 != nrow || M->shape1 != ncol) {
		char buf[200];
		std::snprintf(buf, sizeof buf, "Shape of M (%llu x %llu) must be that of op(A) * op(B) (%llu x %llu)",
			(unsigned long long)M->shape0, (unsigned long long)M->shape1, (unsigned long long)nrow, (unsigned long long)ncol);
		throw Error{SPSAMD_EDIM, buf};
	}
	// (the unchecked count, as this call always took it: a null prepared handle is an empty mask here, where add's intake
	// throws, and a handle of another context fails only once mask_keys reads it)
	const uint64_t nm_in = operand_tuples(M);
	if (nm_in >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "nnz(M) is 2^31 or more"};
	if (product_is_empty(C, scalei, A, scalej, B, scalek) || nm_in == 0) return;      // and an empty mask

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	{ const spsamd_coo *ops[3] = {A, B, M}; pick_output_set(c, ops, 3); }
	ConMat ca, cb;
	consolidate_operand(c, A, f.a0, f.a0, duplicate_policy, zero_nan, &ca);       // :187
	consolidate_operand(c, B, f.bj, f.bj, duplicate_policy, zero_nan, &cb);       // :188, by the columns of op(B)
	res->nnz_a = ca.nnz; res->nnz_b = cb.nnz;
	const uint32_t *arp = dense_rowptr(c, ca, 0), *brp = dense_rowptr(c, cb, 0);
	ScaleDev si, sj, sk;
	upload_scale(c, scalei, nrow, "scalei", &si);
	upload_scale(c, scalej, f.inner, "scalej", &sj);
	upload_scale(c, scalek, ncol, "scalek", &sk);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	MaskKeys mk;
	mask_keys(c, M, 0, nrow, ncol, &mk);
	const uint32_t nm = mk.n;
	ConMat mcon;
	mcon.row = const_cast<int32_t *>(mk.i); mcon.col = const_cast<int32_t *>(mk.j); mcon.nnz = nm; mcon.nrow = nrow; mcon.ncol = ncol;
	const uint32_t *mrp = dense_rowptr(c, mcon, 0);

	// classes
	const int path = c->tune.masked_path;
	if (path < 0 || path > 3) throw Error{SPSAMD_EINVAL, "masked_path must be 0 (auto), 1 (entry), 2 (row) or 3 (wave)"};
	uint8_t *rowflag = c->arena.get<uint8_t>(nrow ? nrow : 1), *cls = c->arena.get<uint8_t>(nm + 1);
	uint8_t *f_entry = c->arena.get<uint8_t>(nm + 1), *f_wave = c->arena.get<uint8_t>(nm + 1), *emit = c->arena.get<uint8_t>(nm + 1);
	uint32_t *off_entry = c->arena.get<uint32_t>(nm + 1), *off_wave = c->arena.get<uint32_t>(nm + 1), *off_row = c->arena.get<uint32_t>(nrow + 1);
	double *sums = c->arena.get<double>(nm + 1);
	unsigned long long *acc = c->arena.get<unsigned long long>(4);           // products, then the digest's count, hash, sum
	fill_zero(c, acc, 4 * sizeof(unsigned long long));
	fill_zero(c, emit, nm + 1);
	const int32_t *si_pos = si.present ? si.pos : nullptr, *sk_pos = sk.present ? sk.pos : nullptr;
	if (nrow) { k_masked_rows<<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(mrp, arp, nrow, si_pos, si.val, path, rowflag); SPS_LAUNCH_CHECK(); }
	if (nm) {
		k_masked_classify<<<dim3(grid_for(nm)), dim3(256), 0, st>>>(mk.i, mk.j, nm, arp, brp, si_pos, si.val, sk_pos, sk.val, rowflag, path,
			cls, f_entry, f_wave);
		SPS_LAUNCH_CHECK();
	}
	scan_exclusive_u8_u32(c, f_entry, off_entry, nm);
	scan_exclusive_u8_u32(c, f_wave, off_wave, nm);
	scan_exclusive_u8_u32(c, rowflag, off_row, nrow);
	WordList wl;
	wl.add(off_entry + nm); wl.add(off_wave + nm); wl.add(off_row + nrow);
	uint32_t cnt[3];
	read_back_words(c, wl, cnt);
	const uint32_t n_entry = cnt[0], n_wave = cnt[1], n_row = cnt[2];
	uint32_t *list_entry = c->arena.get<uint32_t>(n_entry + 1), *list_wave = c->arena.get<uint32_t>(n_wave + 1);
	int32_t *rows = c->arena.get<int32_t>(n_row + 1);
	if (nm) { k_masked_lists<<<dim3(grid_for(nm)), dim3(256), 0, st>>>(f_entry, f_wave, off_entry, off_wave, nm, list_entry, list_wave); SPS_LAUNCH_CHECK(); }
	if (n_row) { k_masked_rowlist<<<dim3(grid_for(nrow)), dim3(256), 0, st>>>(rowflag, off_row, nrow, rows); SPS_LAUNCH_CHECK(); }

	// evaluation: one launch per class
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));
	MaskedArgs g;
	g.arp = arp; g.acol = ca.col; g.aval = ca.val;
	g.brp = brp; g.bcol = cb.col; g.bval = cb.val;
	g.mi = mk.i; g.mj = mk.j;
	g.sj_pos = sj.present ? sj.pos : nullptr; g.sj_val = sj.val;
	g.sum = sums; g.emit = emit; g.products = acc;
	const unsigned cap = (unsigned)c->num_cu * 32u;                    // workgroups of the grid-stride launches
	if (n_entry) { k_masked_entry<<<dim3(std::min(grid_for(n_entry), cap)), dim3(256), 0, st>>>(g, list_entry, n_entry); SPS_LAUNCH_CHECK(); }
	if (n_row) { k_masked_row<<<dim3(std::min(n_row, cap)), dim3(256), 0, st>>>(g, rows, n_row, mrp, cls); SPS_LAUNCH_CHECK(); }
	if (n_wave) { k_masked_wave<<<dim3(std::min(grid_for(n_wave, 4), cap)), dim3(256), 0, st>>>(g, list_wave, n_wave); SPS_LAUNCH_CHECK(); }
	SPS_HIP(hipEventRecord(c->ev[EV_N0], st));

	// sinks
	if (coo) {
		uint32_t *off = c->arena.get<uint32_t>(nm + 1);
		scan_exclusive_u8_u32(c, emit, off, nm);
		WordList w2;
		w2.add(off + nm); w2.add64(acc);
		uint32_t h[3];
		read_back_words(c, w2, h);
		const uint32_t total = h[0];
		res->products = (uint64_t)h[1] | ((uint64_t)h[2] << 32);
		const CooOut o = coo_output(c, total);
		if (total) {
			k_masked_compact<<<dim3(grid_for(nm)), dim3(256), 0, st>>>(mk.i, mk.j, sums, emit, off, nm, C, si_pos, si.val, sk_pos, sk.val,
				o.row, o.col, o.val);
			SPS_LAUNCH_CHECK();
		}
		publish_coo(c, res, o.row, o.col, o.val, total, permute);
	} else {
		RowStats rs;
		if (sink_flags & SPSAMD_SINK_ROWSTATS) rs = rowstats_begin(c, nrow, 8, res);      // (8 bytes of slack, as this sink always asked for)
		if (nm) {
			k_masked_digest<<<dim3(std::min(grid_for(nm), 2048u)), dim3(256), 0, st>>>(mk.i, mk.j, sums, emit, nm, C, si_pos, si.val, sk_pos,
				sk.val, acc + 1, rs.nnz, rs.sum, rs.hash);
			SPS_LAUNCH_CHECK();
		}
		unsigned long long *h = (unsigned long long *)c->host_staging(4 * sizeof(unsigned long long));
		SPS_HIP(hipMemcpyAsync(h, acc, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
		SPS_HIP(hipStreamSynchronize(st));
		res->products = h[0];
		res->nnz = h[1];
		res->hash = h[2];
		std::memcpy(&res->sum, &h[3], sizeof(double));
	}
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_N0]));
}

} // namespace spsamd
