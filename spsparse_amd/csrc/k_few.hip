// k_few.hip -- the LDS hash accumulator for cells whose row has few A tuples (at most FEW_LMAX = 16): k_few<T, NT, MODE>.
// The mid rows with at most `few_max` A tuples run here (bins BIN_FEW ..; the others stay on k_hash).
//
// Such a cell is the union of a few long, contiguous B segments (R-MAT scale 20: 2.3 A tuples per mid row, a median segment
// of 220 tuples).  k_hash spends on it what a chunk of NT A tuples costs -- expand_load, expand_batch, three LDS lookups per
// product -- and asks for the B tuples only behind those barriers, with nothing of the next cell in flight.  Here
//   * a cell's segments (first B tuple, length, A value) live in lanes 0 .. 15 of EVERY wave, read from elo / elen / aval by
//     A position (no load depends on another), and the exclusive product prefix is a DPP scan: no LDS, no barrier;
//   * thread t takes products t, t + NT, ...; the segment of product p is the last one whose prefix is <= p, found by a
//     uniform loop over the cell's A tuples (v_readlane + compare + select): a wave reads consecutive tuples of a segment;
//   * the loop over the cells is a software pipeline, branch-free and clamped like k_hash's: the record of cell i+3
//     (CellPend), the segments of cell i+2 and ALL B tuples of cell i+1 are requested at the top of cell i, before its
//     insertions -- ceil(T / 2 / NT) tuples per thread wait in registers while cell i is accumulated and emitted;
//   * two barriers per cell outside hash_emit: insertions complete, table clean.  The count of occupied slots is two
//     counters taken in turn, as in k_hash_tiles2 (k_tiles.hip).
// Insertion and emission are spgemm_hash.h's: hash_slot, the probe loop of hash_products, hash_emit.
#include "spgemm_host.h"
#include "spgemm_hash.h"

namespace spsamd {

// A cell's segments as every wave holds them: lane l < La has segment l (len 0 in the lanes behind); prods = their sum
struct FewSegs { uint32_t lo, len; double a; };

// ... of the cell with A tuples [beg, end): three independent loads per lane (lanes behind the cell re-read its first tuple)
__device__ __forceinline__ FewSegs few_segs_load(const RowMeta &m, uint32_t beg, uint32_t end)
{
	const uint32_t e = beg + (lane_id() & (FEW_LMAX - 1u));
	const bool act = lane_id() < FEW_LMAX && e < end;
	const uint32_t ec = act ? e : beg;
	FewSegs s;
	s.lo = m.elo[ec];
	const uint32_t len = m.elen[ec];
	s.a = m.aval[ec];
	s.len = act ? len : 0u;
	return s;
}

// The B tuples of a cell, U per thread, as they wait in registers: slot u is product u * NT + tid (a slot past the last
// product re-reads the cell's first tuple and is masked by `prods`)
template <int U> struct FewB { BTup t[U]; double a[U]; uint32_t prods; };

template <int U, int NT>
__device__ __forceinline__ void few_request(FewB<U> &b, const RowMeta &m, const FewSegs &s, const Cell &rec, uint32_t cap)
{
	const uint32_t inc = wave_inclusive_scan_u32(s.len);
	const uint32_t La = min(rec.end - rec.beg, FEW_LMAX);
	uint32_t prods = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
	if (rec.prods > cap || rec.end - rec.beg > FEW_LMAX) prods = 0; // never (k_few flags it): the cell is skipped as a whole
	const uint32_t pref = inc - s.len;
	uint32_t p[U], off[U];
#pragma unroll
	for (int u = 0; u < U; ++u) {
		const uint32_t q = (uint32_t)u * NT + threadIdx.x;
		p[u] = q < prods ? q : 0u;
		off[u] = 0u; b.a[u] = 0.0;
	}
	for (uint32_t g = 0; g < La; ++g) {                             // uniform; prefixes ascend, so the last segment with prefix <= p wins
		const uint32_t ps = (uint32_t)__builtin_amdgcn_readlane((int)pref, (int)g);
		const uint32_t rel = (uint32_t)__builtin_amdgcn_readlane((int)s.lo, (int)g) - ps;
		const double as = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s.a), (int)g), __builtin_amdgcn_readlane(__double2loint(s.a), (int)g));
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const bool in = ps <= p[u];
			off[u] = in ? rel : off[u];
			b.a[u] = in ? as : b.a[u];
		}
	}
#pragma unroll
	for (int u = 0; u < U; ++u) b.t[u] = m.btup[off[u] + p[u]];
	b.prods = prods;
}

template <int T, int NT, int MODE>
__global__ __launch_bounds__(NT) void k_few(const Cell *cells, uint32_t ncell, RowMeta m, EmitParams ep, SinkParams sk)
{
	constexpr int U = (T / 2 + NT - 1) / NT;
	__shared__ int32_t h_key[T];
	__shared__ double h_val[MODE == MODE_COUNT ? 1 : T];
	__shared__ uint16_t occ[T / 2];
	__shared__ uint64_t s_sort[MODE == MODE_STORE ? T / 2 : 1];
	__shared__ uint16_t s_cnt[MODE == MODE_STORE ? 16 * ((T / 2 + NT - 1) / NT) * (NT / 64) : 1];
	__shared__ uint32_t scr32[NT / 64 + 1];
	__shared__ uint32_t s_nocc[2];           // occupied slots of a cell: two counters taken in turn (below)
	__shared__ unsigned long long s_u64[2 * (NT / 64)];
	__shared__ double s_f64[NT / 64];

	const unsigned tid = threadIdx.x, lane = lane_id();
	for (int q = tid; q < T; q += NT) { h_key[q] = -1; if (MODE != MODE_COUNT) h_val[q] = 0.0; }
	if (tid < 2) s_nocc[tid] = 0;
	__syncthreads();
	DigestAcc dacc{0, 0, 0.0};                                      // DIGEST, whole launch
	uint32_t oflip = 0;

	// The pipeline's state at the top of cell i: rec0 and b0 (its B tuples, requested a cell ago), rec1 and seg1 (cell i+1,
	// its segments read a cell ago), rec2 (cell i+2), pend3 (the record of cell i+3 in flight).  Indices past the
	// workgroup's last cell are clamped to it: what they read is valid and never used.
	const uint32_t stride = gridDim.x, first = blockIdx.x, clast = ncell - 1u;     // (grid <= ncell: every workgroup has a cell)
	const uint32_t zlane = cell_pend_zero();
	Cell rec0 = cells[min(first, clast)], rec1 = cells[min(first + stride, clast)], rec2 = cells[min(first + 2u * stride, clast)];
	CellPend pend3 = cell_pend_load(cells, min(first + 3u * stride, clast), zlane);
	FewSegs seg1 = few_segs_load(m, rec1.beg, rec1.end), seg2 = few_segs_load(m, rec2.beg, rec2.end);
	FewB<U> b0;
	few_request<U, NT>(b0, m, few_segs_load(m, rec0.beg, rec0.end), rec0, (uint32_t)(T / 2));
	for (uint32_t ci = first; ci < ncell; ci += stride) {
		const Cell cell = rec0;
		// Never: the bin bounds the cell (T / 2 products fit the tables) and the routing its A tuples.  If the host's lists ever
		// broke either promise the cell is skipped as a whole -- few_request asked for no product of it -- and the error word
		// makes the multiply fail instead of returning a wrong product.
		if ((cell.prods > (uint32_t)(T / 2) || cell.end - cell.beg > FEW_LMAX) && tid == 0) atomicOr(sk.err, 1u);
		// ---- the top of the cell: every B tuple of the next one, the segments of the one after, the record of the third
		FewB<U> b1;
		few_request<U, NT>(b1, m, seg1, rec1, (uint32_t)(T / 2));
		rec0 = rec1; rec1 = rec2; seg1 = seg2;
		rec2 = cell_from_pend(pend3);
		seg2 = few_segs_load(m, rec2.beg, rec2.end);
		pend3 = cell_pend_load(cells, min(ci + 4u * stride, clast), zlane);

		// ---- this cell's products -> table (the probe loop and the wave-aggregated append of hash_products)
		{
			uint32_t slot_of[U]; uint64_t newmask[U]; uint32_t nnew = 0;
#pragma unroll
			for (int u = 0; u < U; ++u) {
				bool isnew = false;
				uint32_t h = 0;
				if ((uint32_t)u * NT + tid < b0.prods) {
					const int32_t col = b0.t[u].col;
					h = hash_slot<T>(col);
					for (;;) {
						int32_t old = atomicCAS(&h_key[h], -1, col);
						if (old == -1) { isnew = true; break; }
						if (old == col) break;
						if constexpr ((T & (T - 1)) == 0) h = (h + 1) & (T - 1);
						else h = h + 1 == (uint32_t)T ? 0u : h + 1;
					}
					if (MODE != MODE_COUNT) atomicAdd(&h_val[h], b0.a[u] * btup_val(b0.t[u]));
				}
				slot_of[u] = h;
				newmask[u] = __ballot(isnew);
				nnew += (uint32_t)__popcll(newmask[u]);
			}
			if (nnew) {                                                 // uniform: one LDS fetch-add per wave and cell
				uint32_t base = 0;
				if (lane == 0) base = lds_add_rtn_u32(&s_nocc[oflip], nnew);
				base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
				for (int u = 0; u < U; ++u) {
					if ((newmask[u] >> lane) & 1ull) occ[base + __popcll(newmask[u] & lanemask_lt())] = (uint16_t)slot_of[u];
					base += (uint32_t)__popcll(newmask[u]);
				}
			}
		}
		lds_barrier();                                              // the cell's products are in the table
		const uint32_t nocc = s_nocc[oflip];
		// the previous cell's count: every wave read it before that cell's last barrier; the next cell adds to it behind this one's
		if (tid == 0) s_nocc[oflip ^ 1u] = 0;
		oflip ^= 1u;
		hash_emit<T, NT, MODE, false>(nocc, cell.rowid, cell.seg, ep, sk, h_key, h_val, occ, s_sort, scr32, dacc, s_cnt, 0, ep.ncolbits, m, cell.beg, cell.end, -1.0);
		lds_barrier();                                              // the table is clean
		b0 = b1;
	}
	if (MODE == MODE_DIGEST) digest_flush<NT>(sk.digest, dacc.cnt, dacc.hash, dacc.sum, s_u64, s_f64);
}

template <int T, int NT, int MODE>
static void launch_few(spsamd_ctx *c, const Cell *cells, uint32_t ncell, const RowMeta &m, const EmitParams &ep, const SinkParams &sk)
{
	if (!ncell) return;
	const unsigned grid = std::min<unsigned>(ncell, (unsigned)(c->num_cu * resident_per_cu<&k_few<T, NT, MODE>>(NT)));
	k_few<T, NT, MODE><<<dim3(grid), dim3(NT), 0, c->stream>>>(cells, ncell, m, ep, sk);
	SPS_LAUNCH_CHECK();
}

// The mid rows with at most few_max A tuples, by the mid rows' table classes
template <int MODE>
void launch_mid_few(spsamd_ctx *c, const Bins &b, const MidCells &mc, const RowMeta &m, const EmitParams &ep, const SinkParams &sk)
{
	launch_few<1024, 256, MODE>(c, mc.few[0], b.count[BIN_FEW], m, ep, sk);
	launch_few<4096, 512, MODE>(c, mc.few[1], b.count[BIN_FEW + 1], m, ep, sk);
	launch_few<8192, 1024, MODE>(c, mc.few[2], b.count[BIN_FEW + 2], m, ep, sk);   // 104 KB of LDS and more: one workgroup per CU, so make it 16 waves (512 threads: 1.26 ms against 0.95 on R-MAT scale 20)
}

template void launch_mid_few<MODE_COUNT>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_mid_few<MODE_STORE>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_mid_few<MODE_DIGEST>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);

} // namespace spsamd
