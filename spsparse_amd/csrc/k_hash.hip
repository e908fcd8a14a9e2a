// k_hash.hip -- the LDS hash accumulator: k_hash<T,NT> (mid rows; hash cells of heavy rows too long for a tile) and the
// first-generation hash tiles k_hash_tiles (the ORDERED mode runs on them).
#include "spgemm_host.h"
#include "spgemm_hash.h"

namespace spsamd {

// The window-occupancy words of op(B) (bocc, k_bwin_scan): does row k hold a tuple in the cell's windows [wa, wb)?  A hash
// cell of a long row visits every A tuple of its row, and for three tuples in four (R-MAT scale 20) the cell's windows of that B
// row are empty: the 16 MB table answers from the L2 / Infinity Cache what a pair of random lines of the 541 MB bwin would.
// wa < wb are uniform: the masks are scalar, and a range makes one step unless it crosses a group of 128 windows.  The load
// and the test are apart so that a word read ahead stays in flight until the test.
__device__ __forceinline__ uint4 bocc_load(const uint32_t *bocc, uint32_t nbw, uint32_t k, uint32_t g)
{
	return reinterpret_cast<const uint4 *>(bocc + (uint64_t)k * nbw)[g];
}
__device__ __forceinline__ uint32_t bocc_word_mask(uint32_t lo, uint32_t hi, uint32_t base)       // bits [lo, hi) of a group, word at `base`
{
	const uint32_t a = lo > base ? min(lo - base, 32u) : 0u, b = hi > base ? min(hi - base, 32u) : 0u;
	return (uint32_t)(((1ull << b) - 1ull) & ~((1ull << a) - 1ull));
}
__device__ __forceinline__ uint32_t bocc_test(const uint4 &x, uint32_t g, uint32_t wa, uint32_t wb)
{
	const uint32_t b0 = g << 7, lo = max(wa, b0) - b0, hi = min(wb, b0 + 128u) - b0;
	return (x.x & bocc_word_mask(lo, hi, 0)) | (x.y & bocc_word_mask(lo, hi, 32)) | (x.z & bocc_word_mask(lo, hi, 64)) | (x.w & bocc_word_mask(lo, hi, 96));
}
// ... the groups after `g0`, the one that holds wa (none for most cells)
__device__ __forceinline__ uint32_t bocc_rest(const uint32_t *bocc, uint32_t nbw, uint32_t k, uint32_t g0, uint32_t wa, uint32_t wb)
{
	uint32_t bits = 0;
	for (uint32_t g = g0 + 1u; g <= (wb - 1u) >> 7; ++g) bits |= bocc_test(bocc_load(bocc, nbw, k, g), g, wa, wb);
	return bits;
}

// Steps of 64 A tuples a wave scans ahead per round in the long rows' cells: as many as the survivors' ring has room for -- in
// STORE it lies over s_sort (T / 2 entries), otherwise the 512-thread classes must keep two workgroups on a CU.
constexpr int long_steps(int T, int MODE) { return T == 1024 ? (MODE == MODE_STORE ? 1 : 3) : (T == 3072 ? 2 : (T == 4096 ? 3 : 4)); }

template <int T, int NT, int MODE, bool WINDOWED, bool PAT>
__global__ __launch_bounds__(NT) void k_hash(const Cell *cells, uint32_t ncell, const uint32_t *xb, RowMeta m,
	const uint32_t *bwin, uint32_t nwin1, EmitParams ep, SinkParams sk, const uint32_t *bocc, uint32_t nbw)
{
	__shared__ int32_t h_key[T];
	__shared__ double h_val[MODE == MODE_COUNT ? 1 : T];
	__shared__ uint16_t occ[T / 2];
	__shared__ uint64_t s_sort[MODE == MODE_STORE ? sort_slots(T) : 1];
	__shared__ uint16_t s_cnt[MODE == MODE_STORE ? 16 * ((T / 2 + NT - 1) / NT) * (NT / 64) : 1];
	__shared__ Expand<NT, T / 2> X;
	__shared__ uint32_t scr32[NT / 64 + 1];
	__shared__ uint32_t s_nocc;
	__shared__ PatCell s_pat;
	__shared__ unsigned long long s_u64[2 * (NT / 64)];
	__shared__ double s_f64[NT / 64];
	__shared__ uint2 s_queue[WINDOWED && MODE != MODE_STORE ? NT * (long_steps(T, MODE) + 1) : 1];      // WINDOWED: the survivors' ring
	__shared__ uint32_t s_qcnt[2][NT / 64];

	const unsigned tid = threadIdx.x;
	for (int q = tid; q < T; q += NT) { h_key[q] = -1; if (MODE != MODE_COUNT) h_val[q] = 0.0; }
	PatAcc pat; pat_init(pat);
	if (tid == 0) pat_reset(&s_pat);
	DigestAcc dacc{0, 0, 0.0};                                      // DIGEST, whole launch
	uint32_t flip = 0;

	const CellWalk walk = cell_walk(xb, ncell);
	const uint32_t stride = walk.stride, cend = walk.end;
	const bool any_cell = walk.first < cend;
	const uint32_t clast = any_cell ? cend - 1 : 0;
	const uint32_t zlane = cell_pend_zero();                        // (records read ahead stay in flight in vector registers: CellPend)
	Cell rec1 = cells[min(walk.first, clast)];
	CellPend pend2 = cell_pend_load(cells, min(walk.first + stride, clast), zlane);
	if constexpr (!WINDOWED) {
	// Software pipeline over the cells of this workgroup: the record of cell i+2, the A tuples of
	// cell i+1 and then its B segment bounds are loaded while cell i is processed (the barriers
	// inside are LDS-only, so these loads stay in flight).
	// The prefetches are branch-free (indices clamped to valid cells / tuples, results masked
	// afterwards): a load inside a conditional is waited for at the join, which would serialise it.
	uint32_t nlo, nlen; double na;
	{
		const uint32_t e = rec1.beg + tid;
		const bool act = e < rec1.end;
		const uint32_t ec = act ? e : rec1.beg;
		const int32_t k = m.acol[ec];
		const uint32_t lo = m.bptr[k], hi = m.bptr[k + 1];
		na = m.aval[ec];
		nlo = lo; nlen = act ? hi - lo : 0u;
	}
	for (uint32_t ci = walk.first; ci < cend; ci += stride) {
		const Cell cell = rec1;
		const uint32_t beg = cell.beg, end = cell.end, seg = cell.seg;
		const int32_t rowid = cell.rowid;
		const uint32_t lo0 = nlo, len0 = nlen; const double a0 = na;
		// stage A / B of the pipeline
		rec1 = cell_from_pend(pend2);
		pend2 = cell_pend_load(cells, min(ci + 2 * stride, clast), zlane);
		const uint32_t ne = rec1.beg + tid;
		const bool nact = (ci + stride < cend) && ne < rec1.end;
		const uint32_t nec = ne < rec1.end ? ne : rec1.beg;
		const int32_t nk = m.acol[nec];
		na = m.aval[nec];
		// Never: the class bounds the cell (T/2 products fit the LDS tables).  If the host's cell lists ever broke
		// that promise the cell is skipped as a whole -- the pipeline state below stays consistent -- and the error
		// word makes the multiply fail instead of returning a wrong product.
		const bool oversize = cell.prods > (uint32_t)(T / 2);
		if (oversize && tid == 0) atomicOr(sk.err, 1u);
		lds_barrier();                                              // previous cell fully emitted, its s_nocc read
		if (tid == 0) s_nocc = 0;

		for (uint32_t chunk = beg; chunk < (oversize ? beg : end); chunk += NT) {
			uint32_t lo = lo0, len = len0; double a = a0;
			if (chunk != beg) {
				uint32_t e = chunk + tid;
				lo = 0; len = 0; a = 0;
				if (e < end) {
					int32_t k = m.acol[e];
					lo = m.bptr[k]; len = m.bptr[k + 1] - lo;
					a = m.aval[e];
				}
			}
			uint32_t total, nzc, ex;
			expand_load(X, lo, len, a, &total, &nzc, flip, &ex);
			if (total == 0) continue;
			if (!ABL(ep, 4)) expand_batch(X, 0, total, nzc);
			if (ABL(ep, 1)) total = 0;
			if (ep.ordered) hash_products_ordered<T, NT, T / 2, MODE>(X, 0, nzc, m, h_key, h_val, occ, &s_nocc);
			else hash_products<T, NT, T / 2, MODE, PAT>(X, 0, total, 0, m, h_key, h_val, occ, &s_nocc, pat);
			lds_barrier();
		}
		if (PAT) pat_publish(pat, &s_pat);                   // (complete at the barrier below)
		// stage C of the pipeline: B segment bounds of the next cell's first chunk
		{
			const uint32_t lo = m.bptr[nk], hi = m.bptr[nk + 1];
			nlo = lo; nlen = nact ? hi - lo : 0u;
		}
		lds_barrier();
		uint32_t nocc = s_nocc;
		if (ABL(ep, 2)) nocc = 0;
		const double pthr = PAT ? pat_threshold(&s_pat, end - beg) : -1.0;
		hash_emit<T, NT, MODE, PAT>(nocc, rowid, seg, ep, sk, h_key, h_val, occ, s_sort, scr32, dacc, s_cnt, 0, ep.ncolbits, m, beg, end, pthr);
		if (PAT) { lds_barrier(); if (tid == 0) pat_reset(&s_pat); }     // (the next cell's barrier orders the reset)
	}
	} else {
	// WINDOWED: the hash cells of rows too long for a tile.  A cell visits every A tuple of its row, and three in four of them
	// (R-MAT scale 20) select a B segment that is empty in the cell's windows.  So the cell does not spend a chunk -- segment
	// bounds from bwin, expand_load, expand_batch, the products, a barrier each -- per NT A tuples of the row: each wave SCANS
	// ahead over the row, U = long_steps(T, MODE) steps of 64 tuples at a time, reading the tuples' columns and op(B)'s occupancy words only
	// (branch-free, all steps in flight), and appends the survivors by ballot rank to a queue of (A position, k) in LDS, in
	// ascending A position: wave w takes the w-th run of U * 64 tuples of a round.  A CHUNK is the next NT survivors:
	// bounds and A values are fetched for those alone.  hash_products_ordered and the EXACT_PATTERN bookkeeping see the
	// tuples in the order they always did, less those that contribute nothing to either.  The queue is a ring of
	// NT * (U + 1) entries: a round is scanned only while fewer than NT survivors wait.  (STORE: the ring lies over
	// s_sort, which only hash_emit uses, a barrier away on either side.)
	// The hand-over to the next cell reads ahead the columns of that cell's first round (and the cell record after it).
	constexpr int NW = NT / 64, U = long_steps(T, MODE);
	constexpr uint32_t QCAP = (uint32_t)NT * (U + 1);
	static_assert(MODE != MODE_STORE || QCAP <= (uint32_t)(T / 2), "the ring fits s_sort");
	uint2 *const queue = MODE == MODE_STORE ? reinterpret_cast<uint2 *>(s_sort) : s_queue;
	const uint32_t lane = lane_id(), wv = wave_id();
	const uint32_t mypos = (wv * U) * 64u + lane;                   // this thread's first tuple in a round
	uint32_t qflip = 0;
	int32_t nk[U];
#pragma unroll
	for (int u = 0; u < U; ++u) { const uint32_t e = rec1.beg + mypos + u * 64u; nk[u] = m.acol[e < rec1.end ? e : rec1.beg]; }
	for (uint32_t ci = walk.first; ci < cend; ci += stride) {
		const Cell cell = rec1;
		const uint32_t beg = cell.beg, end = cell.end, wa = cell.wa, wb = cell.wb, seg = cell.seg, g0 = wa >> 7;
		const int32_t rowid = cell.rowid;
		int32_t k0[U];
#pragma unroll
		for (int u = 0; u < U; ++u) k0[u] = nk[u];
		rec1 = cell_from_pend(pend2);
		pend2 = cell_pend_load(cells, min(ci + 2 * stride, clast), zlane);
#pragma unroll
		for (int u = 0; u < U; ++u) { const uint32_t e = rec1.beg + mypos + u * 64u; nk[u] = m.acol[e < rec1.end ? e : rec1.beg]; }
		// Never (see above): an oversize cell is skipped as a whole, the read-ahead state stays consistent
		const bool oversize = cell.prods > (uint32_t)(T / 2);
		if (oversize && tid == 0) atomicOr(sk.err, 1u);
		lds_barrier();                                              // previous cell fully emitted, its s_nocc read
		if (tid == 0) s_nocc = 0;

		const uint32_t stop = oversize ? beg : end;
		uint32_t pos = beg, qh = 0, qt = 0, qn = 0;                 // ring: head, tail (both < QCAP), entries waiting -- all uniform
		while (pos < stop || qn) {
			if (pos < stop && qn < (uint32_t)NT) {
				// ---- scan a round: NT * U A tuples from pos
				int32_t kk[U]; uint4 x[U];
				if (pos == beg) {
#pragma unroll
					for (int u = 0; u < U; ++u) kk[u] = k0[u];
				} else {
#pragma unroll
					for (int u = 0; u < U; ++u) { const uint32_t e = pos + mypos + u * 64u; kk[u] = m.acol[e < end ? e : beg]; }
				}
#pragma unroll
				for (int u = 0; u < U; ++u) x[u] = bocc_load(bocc, nbw, (uint32_t)kk[u], g0);
				unsigned long long bm[U]; uint32_t wt = 0;
#pragma unroll
				for (int u = 0; u < U; ++u) {
					const uint32_t bits = bocc_test(x[u], g0, wa, wb) | bocc_rest(bocc, nbw, (uint32_t)kk[u], g0, wa, wb);
					bm[u] = __ballot(pos + mypos + u * 64u < end && bits != 0u);
					wt += (uint32_t)__popcll(bm[u]);
				}
				if (lane == 0) s_qcnt[qflip][wv] = wt;
				lds_barrier();
				uint32_t off = qt, tot = 0;
#pragma unroll
				for (int w = 0; w < NW; ++w) { const uint32_t c = s_qcnt[qflip][w]; if (w < (int)wv) off += c; tot += c; }
				qflip ^= 1u;
				tot = (uint32_t)__builtin_amdgcn_readfirstlane((int)tot);       // (the ring's counters stay scalar)
#pragma unroll
				for (int u = 0; u < U; ++u) {
					if ((bm[u] >> lane) & 1ull) {
						uint32_t idx = off + (uint32_t)__popcll(bm[u] & lanemask_lt());
						if (idx >= QCAP) idx -= QCAP;
						queue[idx] = make_uint2(pos + mypos + u * 64u, (uint32_t)kk[u]);
					}
					off += (uint32_t)__popcll(bm[u]);
				}
				qt += tot; if (qt >= QCAP) qt -= QCAP;
				qn += tot;
				pos += (uint32_t)NT * U;
				lds_barrier();                                          // the entries are visible
				continue;
			}
			// ---- a chunk: the next NT survivors (fewer at the row's end)
			const uint32_t n = min(qn, (uint32_t)NT);
			uint32_t lo = 0, len = 0; double a = 0;
			if (tid < n) {
				uint32_t idx = qh + tid;
				if (idx >= QCAP) idx -= QCAP;
				const uint2 q = queue[idx];
				const uint32_t *bw = bwin + (uint64_t)q.y * nwin1;
				lo = bw[wa]; len = bw[wb] - lo;
				a = m.aval[q.x];
			}
			qh += n; if (qh >= QCAP) qh -= QCAP;
			qn -= n;
			uint32_t total, nzc, ex;
			expand_load(X, lo, len, a, &total, &nzc, flip, &ex);     // (its barrier: the entries are read before a round overwrites them)
			if (total == 0) continue;
			if (!ABL(ep, 4)) expand_batch(X, 0, total, nzc);
			if (ABL(ep, 1)) total = 0;
			if (ep.ordered) hash_products_ordered<T, NT, T / 2, MODE>(X, 0, nzc, m, h_key, h_val, occ, &s_nocc);
			else hash_products<T, NT, T / 2, MODE, PAT>(X, 0, total, 0, m, h_key, h_val, occ, &s_nocc, pat);
			lds_barrier();
		}
		if (PAT) pat_publish(pat, &s_pat);                   // (complete at the barrier below)
		lds_barrier();
		uint32_t nocc = s_nocc;
		if (ABL(ep, 2)) nocc = 0;
		const uint32_t colbase = wa << ep.wshift, colbits = ep.wshift + (wb - wa > 1 ? 32 - __builtin_clz(wb - wa - 1) : 0);
		const double pthr = PAT ? pat_threshold(&s_pat, end - beg) : -1.0;
		hash_emit<T, NT, MODE, PAT>(nocc, rowid, seg, ep, sk, h_key, h_val, occ, s_sort, scr32, dacc, s_cnt, colbase, colbits, m, beg, end, pthr);
		if (PAT) { lds_barrier(); if (tid == 0) pat_reset(&s_pat); }     // (the next cell's barrier orders the reset)
	}
	}
	if (MODE == MODE_DIGEST) digest_flush<NT>(sk.digest, dacc.cnt, dacc.hash, dacc.sum, s_u64, s_f64);
}

template <int MODE>
__global__ __launch_bounds__(TILE_NT) void k_hash_tiles(const Tile *tiles, uint32_t ntile, const TCell *tcells, RowMeta m,
	const uint32_t *bwin, uint32_t nwin1, EmitParams ep, SinkParams sk)
{
	constexpr int NT = TILE_NT, T = TILE_T;
	__shared__ int32_t h_key[T];
	__shared__ double h_val[MODE == MODE_COUNT ? 1 : T];
	__shared__ uint16_t occ[T / 2];
	__shared__ uint64_t s_sort[MODE == MODE_STORE ? T / 2 : 1];
	__shared__ uint16_t s_cnt[MODE == MODE_STORE ? 16 * ((T / 2 + NT - 1) / NT) * (NT / 64) : 1];
	constexpr int PB = MODE == MODE_STORE ? TILE_PB_STORE : TILE_PB;
	__shared__ Expand<NT, PB> X;
	__shared__ uint32_t scr32[NT / 64 + 1];
	__shared__ uint32_t s_nocc;
	__shared__ PatCell s_pat;
	__shared__ uint32_t cellP[TILE_MAXCELLS + 1];
	__shared__ unsigned long long s_u64[2 * (NT / 64)];
	__shared__ double s_f64[NT / 64];

	const unsigned tid = threadIdx.x;
	for (int q = tid; q < T; q += NT) { h_key[q] = -1; if (MODE != MODE_COUNT) h_val[q] = 0.0; }
	PatAcc pat; pat_init(pat);
	if (tid == 0) pat_reset(&s_pat);
	DigestAcc dacc{0, 0, 0.0};
	uint32_t flip = 0;
	STAMP_BEGIN();
	TileWalk<BoundsRowMajor, false> walk;
	for (walk.begin(tiles, ntile, tcells, m.acol, m.aval, BoundsRowMajor{bwin, nwin1}); walk.more(); walk.next()) {
		const TileTake t = walk.take();
		const Tile &tile = t.tile;
		const uint32_t myc = tid >> t.lsh, myei = tid & ((1u << t.lsh) - 1u);

		STAMP_COUNT(8);
		STAMP(0);
		lds_barrier();                                              // previous tile fully emitted
		STAMP(1);
		uint32_t total, nzc, ex;
		expand_load(X, t.lo, t.len, t.a, &total, &nzc, flip, &ex);
		if (myei == 0 && myc < tile.ncells) cellP[myc] = ex;       // first product of each cell
		if (tid == 0) { cellP[tile.ncells] = total; s_nocc = 0; }
		// segment ids of the cells of this tile: thread (c, 0) holds cell c's
		const uint32_t seg_of_mine = t.seg;
		STAMP(2);
		if (total) expand_batch(X, 0, total, nzc);
		else lds_barrier();
		STAMP(3);
		walk.expanded();
		for (uint32_t c = 0; c < tile.ncells; ++c) {
			STAMP_COUNT(9);
			STAMP(0);
			const uint32_t p0 = cellP[c], p1 = cellP[c + 1];
			if (ep.ordered) {
				// the cell's products [p0, p1) are whole segments (a segment belongs to one cell)
				const uint32_t q0 = expand_lookup(X, p0, 0), q1 = expand_lookup(X, p1 - 1, 0) + 1;
				hash_products_ordered<T, NT, PB, MODE>(X, q0, q1, m, h_key, h_val, occ, &s_nocc);
			} else if (ep.pattern) hash_products<T, NT, PB, MODE, true>(X, p0, p1, 0, m, h_key, h_val, occ, &s_nocc, pat);
			else hash_products<T, NT, PB, MODE, false>(X, p0, p1, 0, m, h_key, h_val, occ, &s_nocc, pat);
			if (ep.pattern) pat_publish(pat, &s_pat);
			STAMP(4);
			lds_barrier();
			STAMP(5);
			const uint32_t nocc = s_nocc;
			// the cell's output segment id lives in thread (c, 0): broadcast through LDS
			if (myc == c && myei == 0) scr32[NT / 64] = seg_of_mine;
			lds_barrier();
			const uint32_t seg = scr32[NT / 64];
			if (tid == 0) s_nocc = 0;
			uint32_t colbase = 0, colbits = 0;
			if (MODE == MODE_STORE) {
				const TCell tcc = tcells[tile.first + c];                  // uniform
				colbase = (uint32_t)tcc.wa << ep.wshift;
				colbits = ep.wshift + (tcc.wb - tcc.wa > 1 ? 32 - __builtin_clz((uint32_t)(tcc.wb - tcc.wa) - 1u) : 0);
			}
			STAMP(6);
			const double pthr = ep.pattern ? pat_threshold(&s_pat, tile.end - tile.beg) : -1.0;
			if (ep.pattern) hash_emit<T, NT, MODE, true>(nocc, tile.rowid, seg, ep, sk, h_key, h_val, occ, s_sort, scr32, dacc, s_cnt, colbase, colbits, m, tile.beg, tile.end, pthr);
			else hash_emit<T, NT, MODE, false>(nocc, tile.rowid, seg, ep, sk, h_key, h_val, occ, s_sort, scr32, dacc, s_cnt, colbase, colbits, m, tile.beg, tile.end, pthr);
			STAMP(7);
			if (ep.pattern) { lds_barrier(); if (tid == 0) pat_reset(&s_pat); }
			lds_barrier();
		}
	}
	STAMP_FLUSH();
	if (MODE == MODE_DIGEST) digest_flush<NT>(sk.digest, dacc.cnt, dacc.hash, dacc.sum, s_u64, s_f64);
}

template <int T, int NT, int MODE, bool WINDOWED>
static void launch_hash(spsamd_ctx *c, const Cell *cells, uint32_t ncell, const uint32_t *xb, const RowMeta &m, const uint32_t *bwin,
	uint32_t nwin1, const EmitParams &ep, const SinkParams &sk, const uint32_t *bocc = nullptr, uint32_t nbw = 0)
{
	if (!ncell) return;
	unsigned grid = std::min<unsigned>(ncell, (unsigned)(c->num_cu * resident_per_cu<&k_hash<T, NT, MODE, WINDOWED, false>>(NT)));
	if (grid >= 64) grid &= ~7u;               // multiple of 8: the XCD-aware walk
	if (ep.pattern) k_hash<T, NT, MODE, WINDOWED, true><<<dim3(grid), dim3(NT), 0, c->stream>>>(cells, ncell, xb, m, bwin, nwin1, ep, sk, bocc, nbw);
	else k_hash<T, NT, MODE, WINDOWED, false><<<dim3(grid), dim3(NT), 0, c->stream>>>(cells, ncell, xb, m, bwin, nwin1, ep, sk, bocc, nbw);
	SPS_LAUNCH_CHECK();
}

template <int MODE>
void launch_mid(spsamd_ctx *c, const Bins &b, const MidCells &mc, const RowMeta &m, const EmitParams &ep, const SinkParams &sk)
{
	launch_hash<1024, 256, MODE, false>(c, mc.cells[0], b.count[5], nullptr, m, nullptr, 0, ep, sk);
	launch_hash<4096, 512, MODE, false>(c, mc.cells[1], b.count[6], nullptr, m, nullptr, 0, ep, sk);
	launch_hash<8192, 512, MODE, false>(c, mc.cells[2], b.count[7], nullptr, m, nullptr, 0, ep, sk);   // 115 KB of LDS: one workgroup per CU, so make it 8 waves
}

template <int MODE>
void launch_hash_windowed(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk)
{
	launch_hash<1024, 256, MODE, true>(c, hv.cells[0], hv.ncell[0], hv.xb[0], m, hv.bwin, hv.nwin1, ep, sk, hv.bocc, hv.nbw);
	launch_hash<3072, 512, MODE, true>(c, hv.cells[1], hv.ncell[1], hv.xb[1], m, hv.bwin, hv.nwin1, ep, sk, hv.bocc, hv.nbw);
	launch_hash<4096, 512, MODE, true>(c, hv.cells[2], hv.ncell[2], hv.xb[2], m, hv.bwin, hv.nwin1, ep, sk, hv.bocc, hv.nbw);
	launch_hash<8192, 512, MODE, true>(c, hv.cells[3], hv.ncell[3], hv.xb[3], m, hv.bwin, hv.nwin1, ep, sk, hv.bocc, hv.nbw);
}

template <int MODE>
void launch_tiles_v1(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk)
{
	const unsigned grid = std::min<unsigned>(hv.ntile, (unsigned)(c->num_cu * resident_per_cu<&k_hash_tiles<MODE>>(TILE_NT)));
	const SinkParams &sks = stamps_sink(c, sk, grid);
	k_hash_tiles<MODE><<<dim3(grid), dim3(TILE_NT), 0, c->stream>>>(hv.tb.tiles, hv.ntile, hv.tb.tcells, m, hv.bwin, hv.nwin1, ep, sks);
	SPS_LAUNCH_CHECK();
	static const char *const nm[10] = {"pre", "Bwait", "expand_load", "expand_batch", "products", "Bwait2", "segbcast", "emit", "tiles", "cells"};
	stamps_report(c, sks, grid, "k_hash_tiles", nm, 10);
}

template void launch_mid<MODE_COUNT>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_mid<MODE_STORE>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_mid<MODE_DIGEST>(spsamd_ctx *, const Bins &, const MidCells &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_hash_windowed<MODE_COUNT>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_hash_windowed<MODE_STORE>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_hash_windowed<MODE_DIGEST>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_tiles_v1<MODE_COUNT>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_tiles_v1<MODE_STORE>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);
template void launch_tiles_v1<MODE_DIGEST>(spsamd_ctx *, const Heavy &, const RowMeta &, const EmitParams &, const SinkParams &);

#ifdef SPSAMD_ABLATIONS
void set_ablation_word(spsamd_ctx *c, int word)
{
	SPS_HIP(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_abl), &word, sizeof(int), 0, hipMemcpyHostToDevice, c->stream));
	SPS_HIP(hipStreamSynchronize(c->stream));
}
#endif

} // namespace spsamd
