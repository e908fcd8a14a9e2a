// k_emult.hip -- op(A) o op(B) over the intersection of two patterns, and op(A) on or off op(B)'s pattern (spsamd_emult,
// include/spsparse_amd.h; GraphBLAS eWiseMult and its two structural relatives).
//
// S_A = op(A) as spsamd_select takes it; S_B the same under TIMES, op(B)'s unique keys (the shared intake's mask_keys) under
// FIRST.  Both ascend in the 64-bit key row << 32 | col (a trusted operand is checked for it).  The result is a subsequence
// of S_A: the tuples whose key is (FIRST | COMPLEMENT: is not) a key of B; under TIMES the value is (alpha * a) * b with b the
// FIRST tuple of S_B of that key, under FIRST a's bits.
//
// Device path.  Every path answers one question per position of S_A -- B's position, or a miss:
//   1. merge    the shared merge-path split (k_add.hip: tiles of ADD_TILE merged items, A first on equal keys); k_em_merge
//               stages the tile's two key slices in LDS, each lane merges ADD_IPT items.  With A first on ties, the B cursor
//               of a lane that takes an A tuple stands on the first B tuple whose key is not smaller: a hit if that key is
//               equal, and that tuple is the first of its key.  A cursor past the tile's B slice reads the one key that
//               follows the slice from memory, so a run of equal A keys that straddles tiles still names the same B tuple.
//               The lane writes one 4-byte word per A tuple (B's position or all ones), the wave its count of kept tuples
//               and where its A range starts.  The keys are read once; no value is touched.
//   2. probe A  k_em_probe_a: every tuple of S_A finds the lower bound of its key in S_B -- inside the row where B is a
//               prepared handle (its row pointer exists), over the whole stream on the 64-bit key where it is not.
//   3. probe B  k_em_probe_b: every first-of-key tuple of S_B finds the lower bound and the run length of its key in S_A.
//               Without COMPLEMENT the run lengths are scanned and k_em_emit_runs stores the runs: no array of nnz(A)
//               entries exists.  Under COMPLEMENT the probe writes its position over the run in a word array preset to
//               all ones, and the flag tail below runs over S_A.
//   flag tail   the shared compaction over wave tiles (devutil.h): the per-wave counts are scanned; k_em_compact reads each
//               word and, for a kept tuple, a (and b under TIMES) and stores (i, j, v) in S_A's order.
// Every product has the bits x86-64 gives it (x86fp.h).
#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace spsamd {

constexpr uint32_t EM_MISS = 0xFFFFFFFFu;      // the word of an A tuple whose key is no key of B
// Auto choice: the fraction of a probe's search steps charged one 64-byte line of memory traffic (measured 0.29 on the
// lopsided benchmark workload: DESIGN.md section 17, profiles/emult/)
constexpr double EM_PROBE_MISS = 0.25;

__device__ __forceinline__ uint64_t em_key(const int32_t *row, const int32_t *col, uint32_t i)
{
	return ((uint64_t)(uint32_t)row[i] << 32) | (uint64_t)(uint32_t)col[i];
}

// First position of s whose key is >= K: inside row K >> 32 where a dense row pointer exists, else over the whole stream
__device__ __forceinline__ uint32_t em_lower_bound(const AddStream &s, const uint32_t *__restrict__ rp, uint64_t K)
{
	uint32_t lo = 0, hi = s.n;
	if (rp) {
		const uint32_t r = (uint32_t)(K >> 32);
		const int32_t cK = (int32_t)(uint32_t)K;
		lo = rp[r]; hi = rp[r + 1];
		while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (s.col[m] < cK) lo = m + 1; else hi = m; }
		return lo;
	}
	while (lo < hi) { const uint32_t m = lo + ((hi - lo) >> 1); if (em_key(s.row, s.col, m) < K) lo = m + 1; else hi = m; }
	return lo;
}

// The end of the run of key K that starts at `lo` (key[lo] == K; keys ascend): gallop, then bisect
__device__ __forceinline__ uint32_t em_run_end(const AddStream &s, uint32_t lo, uint64_t K)
{
	uint32_t p = lo, step = 1;
	while ((uint64_t)p + step < s.n && em_key(s.row, s.col, p + step) == K) { p += step; step <<= 1; }
	uint32_t l = p + 1, h = (uint32_t)std::min<uint64_t>((uint64_t)p + step, s.n);       // key[p] == K: the end lies in (p, h]
	while (l < h) { const uint32_t m = l + ((h - l) >> 1); if (em_key(s.row, s.col, m) == K) l = m + 1; else h = m; }
	return l;
}

// ---------------------------------------------------------------- path 1: merge

// One tile of the merged sequence: hit[] for the tile's A tuples; per wave, where its A range starts (bounds[4 * tile + wave])
// and how many of its A tuples are kept (hits, under `flip` misses).
__global__ void __launch_bounds__(ADD_NT) k_em_merge(AddStream a, AddStream b, const uint32_t *__restrict__ split, uint32_t ntiles, int flip,
	uint32_t *__restrict__ hit, uint32_t *__restrict__ bounds, uint32_t *__restrict__ wave_count)
{
	__shared__ uint64_t s_key[ADD_TILE];
	const uint32_t tile = blockIdx.x;
	const uint64_t n = (uint64_t)a.n + b.n;
	const uint64_t d0 = (uint64_t)tile * ADD_TILE, d1 = std::min<uint64_t>(d0 + ADD_TILE, n);
	const uint32_t ia0 = split[tile], ia1 = split[tile + 1];
	const uint32_t ib0 = (uint32_t)(d0 - ia0), ib1 = (uint32_t)(d1 - ia1);
	const uint32_t la = ia1 - ia0, len = (uint32_t)(d1 - d0), lb = len - la;
	// A's slice at [0, la), B's at [la, len)
	for (uint32_t k = threadIdx.x; k < len; k += ADD_NT)
		s_key[k] = k < la ? em_key(a.row, a.col, ia0 + k) : em_key(b.row, b.col, ib0 + (k - la));
	// the B key that follows the slice (all ones: none; no real key has its top bit set)
	const uint64_t next_b = ib1 < b.n ? em_key(b.row, b.col, ib1) : ~0ull;
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
	const uint32_t first_a = ia0 + ia;
	const uint32_t nit = std::min<uint32_t>(ADD_IPT, len - diag);
	uint32_t kept = 0;
#pragma unroll
	for (int k = 0; k < ADD_IPT; ++k) {
		if ((uint32_t)k >= nit) continue;
		const uint64_t kb = ib < lb ? s_key[la + ib] : next_b;
		const uint64_t ka = ia < la ? s_key[ia] : ~0ull;
		if (ia < la && (ib >= lb || ka <= kb)) {                 // A first on equal keys: the partition's rule
			const bool h = ka == kb;
			hit[ia0 + ia] = h ? ib0 + ib : EM_MISS;
			kept += h != (flip != 0);
			++ia;
		} else ++ib;
	}
	kept = wave_reduce_sum<uint32_t>(kept);
	if (lane_id() == 0) {
		const uint32_t w = tile * (ADD_NT / 64) + wave_id();         // the wave tile of k_em_compact that stores this range
		bounds[w] = first_a;
		wave_count[w] = kept;
		if (tile == ntiles - 1 && wave_id() == 0) bounds[ntiles * (ADD_NT / 64)] = a.n;
	}
}

// ---------------------------------------------------------------- path 2: every tuple of S_A probes S_B

// (wave_tile_count of devutil.h with the probe as its `keep`, spelled out: that helper unrolls all eight rounds, and this
// loop stays as it was tuned, two binary searches in flight per lane)
__global__ void __launch_bounds__(256) k_em_probe_a(AddStream a, AddStream b, const uint32_t *__restrict__ brp, int flip,
	uint32_t *__restrict__ hit, uint32_t *__restrict__ tile_count)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	const uint64_t base = (uint64_t)tile * WAVE_TILE;
	if (base >= a.n) return;
	uint32_t cnt = 0;
#pragma unroll 2
	for (int r = 0; r < WAVE_TILE_ROUNDS; ++r) {
		const uint64_t i = base + (uint64_t)r * 64 + lane_id();
		bool k = false;
		if (i < a.n) {
			const uint64_t K = em_key(a.row, a.col, (uint32_t)i);
			const uint32_t p = em_lower_bound(b, brp, K);
			const bool h = p < b.n && em_key(b.row, b.col, p) == K;
			hit[i] = h ? p : EM_MISS;
			k = h != (flip != 0);
		}
		cnt += (uint32_t)__popcll(__ballot(k));
	}
	if (lane_id() == 0) tile_count[tile] = cnt;
}

// ---------------------------------------------------------------- path 3: every first-of-key tuple of S_B probes S_A

// run_lo[t], run_len[t] of B tuple t's key in S_A (length 0: not the first of its key, or no such key in A).  MARK: the run's
// words of hit[] get t.
template <bool MARK>
__global__ void __launch_bounds__(256) k_em_probe_b(AddStream b, AddStream a, const uint32_t *__restrict__ arp,
	uint32_t *__restrict__ run_lo, uint32_t *__restrict__ run_len, uint32_t *__restrict__ hit)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= b.n) return;
	const uint64_t K = em_key(b.row, b.col, t);
	uint32_t lo = 0, len = 0;
	if (t == 0 || em_key(b.row, b.col, t - 1) != K) {
		lo = em_lower_bound(a, arp, K);
		if (lo < a.n && em_key(a.row, a.col, lo) == K) len = em_run_end(a, lo, K) - lo;
	}
	if (MARK) { for (uint32_t q = 0; q < len; ++q) hit[lo + q] = t; }
	else { run_lo[t] = lo; run_len[t] = len; }
}

template <int OP>
__device__ __forceinline__ double em_value(double av, const double *__restrict__ bval, uint32_t bpos, double alpha)
{
	if (OP == SPSAMD_EMULT_TIMES) return ref_mul(ref_mul(alpha, av), bval[bpos]);
	return av;
}

template <int OP>
__global__ void __launch_bounds__(256) k_em_emit_runs(AddStream a, AddStream b, double alpha, const uint32_t *__restrict__ run_lo,
	const uint32_t *__restrict__ run_len, const uint32_t *__restrict__ off, int32_t *__restrict__ orow, int32_t *__restrict__ ocol,
	double *__restrict__ oval)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= b.n) return;
	const uint32_t len = run_len[t];
	if (!len) return;
	const uint32_t lo = run_lo[t], o = off[t];
	for (uint32_t q = 0; q < len; ++q) {
		orow[o + q] = a.row[lo + q]; ocol[o + q] = a.col[lo + q];
		oval[o + q] = em_value<OP>(a.val[lo + q], b.val, t, alpha);
	}
}

// ---------------------------------------------------------------- the flag tail

// kept tuples per fixed tile of WAVE_TILE words (the paths whose probe does not count: 3 under COMPLEMENT, an empty B)
__global__ void __launch_bounds__(256) k_em_count(const uint32_t *__restrict__ hit, uint32_t n, int flip, uint32_t *__restrict__ tile_count)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	const uint64_t base = (uint64_t)tile * WAVE_TILE;
	if (base >= n) return;
	const uint32_t cnt = wave_tile_count(base, n, [&](uint64_t i) { return (hit[i] != EM_MISS) != (flip != 0); });
	if (lane_id() == 0) tile_count[tile] = cnt;
}

// A wave per tile: the A range [bounds[tile], bounds[tile + 1]) (null: fixed tiles of WAVE_TILE), stored from tile_off[tile] on
template <int OP>
__global__ void __launch_bounds__(256) k_em_compact(AddStream a, const double *__restrict__ bval, double alpha,
	const uint32_t *__restrict__ hit, const uint32_t *__restrict__ bounds, const uint32_t *__restrict__ tile_off, uint32_t ntiles, int flip,
	int32_t *__restrict__ orow, int32_t *__restrict__ ocol, double *__restrict__ oval)
{
	const uint32_t tile = blockIdx.x * 4 + wave_id();
	if (tile >= ntiles) return;
	uint32_t a0, a1;
	if (bounds) { a0 = bounds[tile]; a1 = bounds[tile + 1]; }
	else { a0 = tile * (uint32_t)WAVE_TILE; a1 = (uint32_t)std::min<uint64_t>((uint64_t)a0 + WAVE_TILE, a.n); }
	a0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a0); a1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)a1);
	wave_range_compact(a0, a1, tile_off[tile], [&](uint64_t i) { return (hit[i] != EM_MISS) != (flip != 0); },
		[&](uint64_t i, uint32_t p) {
			orow[p] = a.row[i]; ocol[p] = a.col[i];
			oval[p] = em_value<OP>(a.val[i], bval, hit[i], alpha);
		});
}

// ---------------------------------------------------------------- driver

// op(X) as spsamd_select takes it, plus this call's rule for a trusted operand: its (row, col) keys must not descend
static void em_operand(spsamd_ctx *c, const spsamd_coo *X, int lead, int duplicate_policy, int zero_nan, ConMat *S, Prepared **prep)
{
	*prep = nullptr;
	const OperandView view = operand_view(c, X);
	const spsamd_coo &P = view.coo;
	const bool handle = view.prep && view.prep->lead == lead;
	if (handle || P.nnz == 0 || P.sort0 != lead || is_own_result(c, P)) {
		consolidate_operand(c, X, lead, lead, duplicate_policy, zero_nan, S, prep);
		return;
	}
	// trusted as stored (duplicates, zeros included): the shared intake inspects it, for the bounds and for the order of the
	// full key
	const PlainStream ps = plain_stream(c, P, lead);
	const size_t n = P.nnz;
	const uint64_t shape[2] = {P.shape0, P.shape1};
	const int32_t *major = ps.major, *minor = ps.minor;
	const double *dv = ps.val;
	S->row = const_cast<int32_t *>(major); S->col = const_cast<int32_t *>(minor); S->val = const_cast<double *>(dv);
	S->nnz = (uint32_t)n; S->nrow = shape[lead]; S->ncol = shape[1 - lead];
}

// The byte model of the auto choice: merge streams 8 B of keys per tuple of both operands and writes and reads one word per
// A tuple; a probe reads its own key (and the word traffic where it has any) and pays one 64-byte line for the fraction
// EM_PROBE_MISS of its search steps.
static int em_choose(uint64_t na, uint64_t nb, bool flip, bool a_rows, bool b_rows, uint64_t nrow)
{
	auto steps = [&](uint64_t n, bool rows) {
		const double per = rows ? (double)n / (double)std::max<uint64_t>(1, std::min<uint64_t>(nrow, n)) : (double)n;
		return std::log2(1.0 + per) + (rows ? 1.0 : 0.0);
	};
	const double m1 = 8.0 * (double)(na + nb) + 8.0 * (double)na;
	const double m2 = 16.0 * (double)na + 64.0 * EM_PROBE_MISS * (double)na * steps(nb, b_rows);
	const double m3 = 8.0 * (double)nb + 64.0 * EM_PROBE_MISS * (double)nb * steps(na, a_rows) + (flip ? 12.0 * (double)na : 0.0);
	if (m3 < m1 && m3 <= m2) return 3;
	return m2 < m1 ? 2 : 1;
}

template <int OP>
static void em_tail(spsamd_ctx *c, const AddStream &a, const double *bval, double alpha, const uint32_t *hit, const uint32_t *bounds,
	const uint32_t *tile_off, uint32_t nwt, int flip, const CooOut &o)
{
	k_em_compact<OP><<<dim3(grid_for(nwt, 4)), dim3(256), 0, c->stream>>>(a, bval, alpha, hit, bounds, tile_off, nwt, flip, o.row, o.col, o.val);
	SPS_LAUNCH_CHECK();
}

void emult_matrices(spsamd_ctx *c, int op, int emult_flags, double alpha, const spsamd_coo *A, char transpose_A,
	const spsamd_coo *B, char transpose_B, int duplicate_policy, int zero_nan, int sink_kind, int sink_flags, spsamd_result *res)
{
	if (op != SPSAMD_EMULT_TIMES && op != SPSAMD_EMULT_FIRST) throw Error{SPSAMD_EINVAL, "unknown emult op"};
	if (emult_flags & ~SPSAMD_EMULT_COMPLEMENT) throw Error{SPSAMD_EINVAL, "unknown emult_flags"};
	const int flip = (emult_flags & SPSAMD_EMULT_COMPLEMENT) ? 1 : 0;
	if (flip && op != SPSAMD_EMULT_FIRST) throw Error{SPSAMD_EINVAL, "SPSAMD_EMULT_COMPLEMENT goes with SPSAMD_EMULT_FIRST only"};
	check_sink_args(duplicate_policy, sink_kind);
	const int path = c->tune.emult_path;
	if (path < 0 || path > 3) throw Error{SPSAMD_EINVAL, "emult_path must be 0 (auto), 1 (merge), 2 (probe A in B) or 3 (probe B in A)"};
	const int la = transpose_A == 'T' ? 1 : 0, lb = transpose_B == 'T' ? 1 : 0;
	const uint64_t ash[2] = {A->shape0, A->shape1}, bsh[2] = {B->shape0, B->shape1};
	const uint64_t nrow = ash[la], ncol = ash[1 - la];
	if (nrow != bsh[lb] || ncol != bsh[1 - lb]) {
		char buf[200];
		std::snprintf(buf, sizeof buf, "Shapes of op(A) (%llu x %llu) and op(B) (%llu x %llu) must match!", (unsigned long long)nrow,
			(unsigned long long)ncol, (unsigned long long)bsh[lb], (unsigned long long)bsh[1 - lb]);
		throw Error{SPSAMD_EDIM, buf};
	}
	const uint64_t na_in = operand_view(c, A).coo.nnz, nb_in = operand_view(c, B).coo.nnz;      // (and the handles checked)
	if (na_in >= (uint64_t(1) << 31) || nb_in >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "an operand has 2^31 or more tuples"};
	const bool times = op == SPSAMD_EMULT_TIMES;
	const bool coo = sink_kind == SPSAMD_SINK_COO;
	const bool permute = coo && (sink_flags & SPSAMD_SINK_PERMUTE);
	const spsamd_coo *ops[2] = {A, B};
	// both output sets operands of the call: refused before anything is written, an empty operand or not
	if (coo && output_set_aliased(c, 0, ops, 2) && output_set_aliased(c, 1, ops, 2))
		throw Error{SPSAMD_EINVAL, "both result buffers of this context are operands of the call: copy one of them out first (spsamd_memcpy)"};
	std::memset(res, 0, sizeof(*res));
	res->shape0 = permute ? ncol : nrow;
	res->shape1 = permute ? nrow : ncol;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	if (coo) pick_output_set(c, ops, 2);
	ConMat SA, SBm;
	Prepared *pa = nullptr, *pb = nullptr;
	em_operand(c, A, la, duplicate_policy, zero_nan, &SA, &pa);
	AddStream sa, sb;
	sa.row = SA.row; sa.col = SA.col; sa.val = SA.val; sa.n = SA.nnz;
	if (times) {
		if (la == lb && same_operand(A, B)) { SBm = SA; pb = pa; }         // A o A: one intake serves both sides
		else em_operand(c, B, lb, duplicate_policy, zero_nan, &SBm, &pb);
		sb.row = SBm.row; sb.col = SBm.col; sb.val = SBm.val; sb.n = SBm.nnz;
	} else {
		MaskKeys mk;
		mask_keys(c, B, lb, nrow, ncol, &mk);
		sb.row = mk.i; sb.col = mk.j; sb.val = nullptr; sb.n = mk.n; pb = mk.prep;
	}
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	const uint32_t na = sa.n, nb = sb.n;
	res->nnz_a = na; res->nnz_b = nb;
	const uint32_t *arp = pa ? pa->rowptr : nullptr, *brp = pb ? pb->rowptr : nullptr;

	uint32_t total = 0;
	CooOut o = {nullptr, nullptr, nullptr};
	if (na && (nb || flip)) {
		int p = path ? path : em_choose(na, nb, flip != 0, arp != nullptr, brp != nullptr, nrow);
		if (nb == 0) p = 3;                                                // no probe runs: every word stays a miss
		if (p == 3 && !flip) {
			// run lengths per tuple of S_B, scanned: nothing of nnz(A) entries
			uint32_t *run_lo = c->arena.get<uint32_t>(nb), *run_len = c->arena.get<uint32_t>((size_t)nb + 1), *off = c->arena.get<uint32_t>((size_t)nb + 1);
			k_em_probe_b<false><<<dim3(grid_for(nb)), dim3(256), 0, st>>>(sb, sa, arp, run_lo, run_len, nullptr);
			SPS_LAUNCH_CHECK();
			o = counted_output(c, run_len, off, nb, coo, &total);
			if (total) {
				if (times) k_em_emit_runs<SPSAMD_EMULT_TIMES><<<dim3(grid_for(nb)), dim3(256), 0, st>>>(sa, sb, alpha, run_lo, run_len, off, o.row, o.col, o.val);
				else k_em_emit_runs<SPSAMD_EMULT_FIRST><<<dim3(grid_for(nb)), dim3(256), 0, st>>>(sa, sb, alpha, run_lo, run_len, off, o.row, o.col, o.val);
				SPS_LAUNCH_CHECK();
			}
			res->products = nb;
		} else {
			uint32_t *hit = c->arena.get<uint32_t>((size_t)na + 1);
			uint32_t nwt = (uint32_t)(((uint64_t)na + WAVE_TILE - 1) / WAVE_TILE);       // wave tiles of the flag tail
			const uint32_t *bounds = nullptr;
			uint32_t *tile_count = nullptr;
			if (p == 1) {
				const uint64_t n = (uint64_t)na + nb;
				const uint32_t ntiles = (uint32_t)((n + ADD_TILE - 1) / ADD_TILE);
				nwt = ntiles * (ADD_NT / 64);
				uint32_t *split = c->arena.get<uint32_t>((size_t)ntiles + 1), *bnd = c->arena.get<uint32_t>((size_t)nwt + 1);
				tile_count = c->arena.get<uint32_t>((size_t)nwt + 1);
				merge_partition(c, sa, sb, ntiles, split);
				k_em_merge<<<dim3(ntiles), dim3(ADD_NT), 0, st>>>(sa, sb, split, ntiles, flip, hit, bnd, tile_count);
				SPS_LAUNCH_CHECK();
				bounds = bnd;
			} else if (p == 2) {
				tile_count = c->arena.get<uint32_t>((size_t)nwt + 1);
				k_em_probe_a<<<dim3(grid_for(nwt, 4)), dim3(256), 0, st>>>(sa, sb, brp, flip, hit, tile_count);
				SPS_LAUNCH_CHECK();
				res->products = na;
			} else {
				tile_count = c->arena.get<uint32_t>((size_t)nwt + 1);
				fill_u32(c, hit, EM_MISS, na);
				if (nb) {
					k_em_probe_b<true><<<dim3(grid_for(nb)), dim3(256), 0, st>>>(sb, sa, arp, nullptr, nullptr, hit);
					SPS_LAUNCH_CHECK();
				}
				k_em_count<<<dim3(grid_for(nwt, 4)), dim3(256), 0, st>>>(hit, na, flip, tile_count);
				SPS_LAUNCH_CHECK();
				res->products = nb;
			}
			uint32_t *tile_off = c->arena.get<uint32_t>((size_t)nwt + 1);
			o = counted_output(c, tile_count, tile_off, nwt, coo, &total);
			if (total) {
				if (times) em_tail<SPSAMD_EMULT_TIMES>(c, sa, sb.val, alpha, hit, bounds, tile_off, nwt, flip, o);
				else em_tail<SPSAMD_EMULT_FIRST>(c, sa, sb.val, alpha, hit, bounds, tile_off, nwt, flip, o);
			}
		}
	} else o = coo ? coo_output(c, 0) : scratch_output(c, 0);
	// a subsequence of S_A: in op(A)'s row order (read permuted: sorted by {1, 0}), indices checked
	deliver_stored(c, res, o, total, nrow, coo, permute, sink_flags);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_CONSOLIDATED], c->ev[EV_END]));
}

} // namespace spsamd
