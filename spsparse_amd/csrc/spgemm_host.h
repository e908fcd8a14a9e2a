// spgemm_host.h -- host-side structures of the multiply path and the launchers its translation units export
#pragma once
#include "spgemm_dev.h"

namespace spsamd {

struct Bins {
	uint32_t count[NBIN];
	uint32_t off[NBIN + 1];
	uint32_t *rows;
};

struct MidCells { Cell *cells[3] = {nullptr, nullptr, nullptr}; Cell *few[3] = {nullptr, nullptr, nullptr}; };   // by table class: k_hash's rows, k_few's (bins BIN_FEW ..)

// Thrown by heavy_prepare: op(B) has more column windows than the heavy-row path indexes, or its window indices would not
// fit the device -- spgemm() then multiplies by column blocks of `width` columns (spgemm_column_blocks).
struct TooWide { uint64_t width; };
constexpr uint64_t COLBLK = (uint64_t)2048 << 14;                   // 2048 windows of 16384 columns: 2^25

struct Heavy {
	uint32_t n = 0;                  // heavy rows
	uint64_t tuples = 0;             // ... and their A tuples
	uint32_t *rows = nullptr;
	uint32_t *bwin = nullptr;
	uint32_t *bocc = nullptr;        // window-occupancy words of op(B)'s rows (the long rows' hash cells test them before bwin)
	uint32_t nbw = 0;
	uint32_t nwin = 0, nwin1 = 0;
	uint32_t *winprod = nullptr;
	uint32_t ncell[NCLS] = {};
	Cell *cells[NCLS] = {};
	CellBases cnt{}, base{};
	uint32_t *xb[NCLS] = {};         // XCD part boundaries per class
	int W = 8192;
	uint32_t cell_cap = CELL_CAP_DEFAULT, dense_min = DENSE_MIN_DEFAULT;
	TileBases tb{};                  // hash tiles
	uint32_t ntile = 0, ntcell = 0;
	TileBases tb2{};                 // direct tiles (k_direct_tiles)
	uint32_t ntile2 = 0, ntcell2 = 0;
	uint32_t direct_min = 0;
	int tiles2 = 0;
	uint32_t *tile_ctr = nullptr;    // claim counters of the tile launches, zeroed with the grouping's counters: [0] COUNT or DIGEST, [1] STORE (null: static walk)
	uint32_t span_cap = 0;
	uint32_t alt_cap = 0, alt_span = 0;
	unsigned long long *alt_cells = nullptr;
	uint32_t long_cap = 0, long_dense_min = 0;
	bool coo = false;                // the tiles also serve a STORE launch
	unsigned long long clsprod[NCLS + 2] = {};
	uint32_t *wptr = nullptr;        // window-major copy of B (dense cells): row pointer per window ...
	BTup *btw = nullptr;             // ... and tuples
	uint64_t nrowb = 0;
	uint32_t nnzb = 0;

	// 32-bit byte offsets into B's tuples suffice (fetch_piece): always, short of 3.5e8 tuples
	uint32_t narrow() const { return ((uint64_t)nnzb + DENSE_SLACK) * 12u < (uint64_t(1) << 32) ? 1u : 0u; }
	// the claim counter of a tile launch (one zeroed counter per launch of a call; null: static walk)
	template <int MODE> uint32_t *tile_claim() const { return tile_ctr ? tile_ctr + (MODE == MODE_STORE ? 1 : 0) : nullptr; }
};

static inline TileKinds tile_kinds(const Heavy &hv)
{
	TileKinds tk{{hv.tb, hv.tb2}, hv.direct_min, hv.span_cap, hv.long_cap, hv.long_dense_min,
		hv.tiles2 == 0 ? (uint32_t)BM_MAXOUT : (uint32_t)(TILE_T / 2), hv.alt_cap, hv.alt_span, hv.alt_cells};
	return tk;
}

static inline float elapsed(hipEvent_t a, hipEvent_t b)
{
	float ms = 0;
	SPS_HIP(hipEventElapsedTime(&ms, a, b));
	return ms;
}

// Resident workgroups per CU of KERNEL at nt threads and no dynamic LDS (asked once per kernel)
template <auto KERNEL>
static inline int resident_per_cu(int nt)
{
	static int per_cu = 0;
	if (!per_cu) {
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, KERNEL, nt, 0) != hipSuccess || nb < 1) nb = 1;
		per_cu = nb;
	}
	return per_cu;
}

// Diagnostic builds (-DSPSAMD_STAMPS): the kernels that keep per-phase cycle counters (STAMP, spgemm_dev.h) are launched with
// stamps_sink's copy of their sink, which has a zeroed block of STAMP_COLS counters per workgroup; stamps_report, behind the
// launch, prints the means over the workgroups of the first ncol columns under their names, and with nmax > 0 the largest
// sum of one workgroup's first nmax columns (its total).  In every other build: the sink itself, and nothing.
#ifdef SPSAMD_STAMPS
static inline SinkParams stamps_sink(spsamd_ctx *c, const SinkParams &sk, unsigned grid)
{
	SinkParams sk2 = sk;
	sk2.stamps = c->arena.get<unsigned long long>((size_t)grid * STAMP_COLS);
	fill_zero(c, sk2.stamps, (size_t)grid * STAMP_COLS * sizeof(unsigned long long));
	return sk2;
}
static inline void stamps_report(spsamd_ctx *c, const SinkParams &sk2, unsigned grid, const char *kernel, const char *const *nm, int ncol, int nmax = 0)
{
	std::vector<unsigned long long> h((size_t)grid * STAMP_COLS);
	SPS_HIP(hipMemcpyAsync(h.data(), sk2.stamps, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
	SPS_HIP(hipStreamSynchronize(c->stream));
	double sum[STAMP_COLS] = {}, mx = 0;
	for (unsigned g = 0; g < grid; ++g) {
		double t = 0;
		for (int i = 0; i < STAMP_COLS; ++i) { sum[i] += (double)h[(size_t)g * STAMP_COLS + i]; if (i < nmax) t += (double)h[(size_t)g * STAMP_COLS + i]; }
		mx = std::max(mx, t);
	}
	fprintf(stderr, "%s stamps (mean cycles per workgroup, grid %u", kernel, grid);
	if (nmax) fprintf(stderr, "; max total %.3g", mx);
	fprintf(stderr, "):");
	for (int i = 0; i < ncol; ++i) fprintf(stderr, " %s %.4g", nm[i], sum[i] / grid);
	fprintf(stderr, "\n");
}
#else
static inline const SinkParams &stamps_sink(spsamd_ctx *, const SinkParams &sk, unsigned) { return sk; }
static inline void stamps_report(spsamd_ctx *, const SinkParams &, unsigned, const char *, const char *const *, int, int = 0) { }
#endif

// ---- launchers (explicitly instantiated for MODE_COUNT / MODE_STORE / MODE_DIGEST in the file named)
template <int MODE> void launch_light(spsamd_ctx *c, const Bins &b, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);             // k_light.hip
template <int MODE> void launch_light_direct_s(spsamd_ctx *c, uint32_t maxp, uint32_t nrow, const uint32_t *aptr, const int32_t *acol, const double *aval,
	const uint32_t *bptr, const ConMat &B, bool k64, const EmitParams &ep, const SinkParams &sk, unsigned long long *pc);                         // k_light.hip
void launch_light_gather(spsamd_ctx *c, uint32_t nrow, uint32_t S, const uint32_t *cnt, const int64_t *off,
	const int32_t *si, const int32_t *sj, const double *sv, int32_t *oi, int32_t *oj, double *ov);                                                    // k_light.hip
template <int MODE> void launch_mid(spsamd_ctx *c, const Bins &b, const MidCells &mc, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);  // k_hash.hip
template <int MODE> void launch_mid_few(spsamd_ctx *c, const Bins &b, const MidCells &mc, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);  // k_few.hip
template <int MODE> void launch_hash_windowed(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);  // k_hash.hip
template <int MODE> void launch_tiles_v1(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);       // k_hash.hip
template <int MODE> void launch_tiles_bm(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);       // k_tiles.hip
template <int MODE> void launch_tiles_hash2(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);    // k_tiles.hip
template <int MODE> void launch_tiles_direct(spsamd_ctx *c, const Heavy &hv, const RowMeta &m, const EmitParams &ep, const SinkParams &sk);   // k_tiles.hip
template <int MODE> void launch_heavy_dense(spsamd_ctx *c, const Heavy &hv, const RowMeta &m0, const EmitParams &ep, const SinkParams &sk);   // k_dense.hip

// ---- the heavy rows' symbolic phase (symbolic_heavy.hip)
int heavy_b_index(spsamd_ctx *c, const ConMat &B, const uint32_t *bptr, uint32_t extra, uint64_t nheavy, Prepared *pb);
void heavy_prepare(spsamd_ctx *c, Heavy &hv, const Bins &bins, const RowMeta &m, const ConMat &B, const uint32_t *bptr,
	uint32_t extra, uint32_t *nseg, bool ordered, bool pattern, Prepared *pb);
void heavy_cells(spsamd_ctx *c, Heavy &hv, const RowMeta &m, const uint32_t *segbase);
void heavy_sort_lists(spsamd_ctx *c, Heavy &hv);

// ---- one multiply in one pass (spgemm.hip).  Also the streamed product's row slice: a.A holds a run of whole rows of op(A) (its tuple
// arrays offset, nrow unchanged); the COO result goes to a.out.  Never by column blocks: a product that would need them throws TooWide.
void spgemm_once(spsamd_ctx *c, MultiplyArgs &a, spsamd_result *res);

#ifdef SPSAMD_ABLATIONS
void set_ablation_word(spsamd_ctx *c, int word);          // k_hash.hip (the only unit that reads it through ABLG)
#endif

#define SPSAMD_INSTANTIATE_MODES(decl_macro) decl_macro(MODE_COUNT) decl_macro(MODE_STORE) decl_macro(MODE_DIGEST)

} // namespace spsamd
