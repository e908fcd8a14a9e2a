// k_aggregate.hip -- MIS(2) aggregation of op(A)'s graph (spsamd_aggregate, include/spsparse_amd.h).
//
// K, the graph and key(v) are spsamd_color's, and so is the code that builds them: graph_adjacency, graph_classes and
// order_by_key of k_color.hip.  Under SPSAMD_AGG_SYMMETRIC the rows are K's own and k_agg_asym checks the promise first.
//
// Sweep.  One 64-bit word per vertex: 0 OUT, key + 1 UNDECIDED, all ones ROOT -- so the largest word of a set says at once
// whether it holds a root and, if not, which undecided vertex comes first.  A round is two walks of the adjacency:
//   spread   for w on the spread list, T1[w] = the largest word of N[w]
//   decide   for v on the undecided list, T2 = the largest T1 of N[v], which is the largest word within distance 2 of v or at
//            v itself: all ones, a root is in range and v goes OUT; v's own word, v becomes a ROOT; else v waits.
// Spread reads words and writes T1, decide reads T1 and its own word and writes its own word, and the two are launches of
// their own (phases between workgroup barriers in the fused run): no kernel reads what another workgroup wrote in the same
// launch.  w stays on the spread list while N[w] holds an undecided vertex and no root: only undecided vertices of N[w]
// read T1[w], and a root in N[w] puts all of them OUT in the round that sees it.  Both lists only shrink; once both are
// thin the rest of the sweep is ONE launch of ONE workgroup, k_agg_fused (k_col_fused's scheme).  The lists are appended
// to through counters, so their order varies from run to run; nothing that is returned depends on it.
//
// Assignment.  The root flags are scanned into ids; k_agg_ring1 gives every root its id and every neighbour of a root the
// root's; k_agg_ring2, a launch of its own because it reads ring 1's ids, gives every other vertex the aggregate of its
// ring-1 neighbour with the largest key.  Then the tail with key agg << 2 | ring, and the sizes off the bounds.
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

constexpr uint32_t AGG_FUSE_ROWS = 1024;              // default of the agg_fuse_rows knob
constexpr uint32_t AGG_WAVE_DEG = 32;                 // default of agg_wave_deg: the largest degree of a thread-class vertex (the measured sweep)
constexpr int AGG_NT = SOLVE_NT;                      // threads of k_agg_fused's one workgroup
constexpr uint64_t AGG_ROOT = ~0ull;
constexpr uint32_t AGG_RING_LONG = 64;                // the ring kernels: a row longer than this is walked by the whole wave

// acc[]: the counters of one call, after graph_classes' four.  AGG_MINSZ holds 2^32 - 1 - the smallest size, so that zeroed
// memory is its neutral element.
enum { AGG_ASYM = GRAPH_ACC, AGG_FUSED = 5, AGG_RING1 = 6, AGG_RING2 = 7, AGG_MAXSZ = 8, AGG_MINSZ = 9, AGG_ACC = 10 };

struct AggArgs {
	const uint32_t *ptr;                       // row pointer of the adjacency
	const int32_t *adj;                        // the neighbours, ascending inside a row; with the flag the row may name v itself
	uint64_t *word;                            // 0 OUT | key + 1 UNDECIDED | all ones ROOT
	uint64_t *t1;                              // the largest word of N[w], as of the last spread that had w on its list
	unsigned long long *acc;
};

__device__ __forceinline__ uint64_t wave_reduce_max_u64(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint64_t)__shfl_xor((unsigned long long)v, d, 64));
	return v;
}

__device__ __forceinline__ bool agg_undecided(uint64_t word) { return word - 1 < AGG_ROOT - 1; }

// every vertex starts UNDECIDED
__global__ void __launch_bounds__(256) k_agg_words(const uint32_t *__restrict__ deg, uint64_t n, uint32_t seed, int by_degree, uint64_t *__restrict__ word)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n) word[v] = ((by_degree ? (uint64_t)deg[v] << 32 : 0ull) | col_hash((uint32_t)v, seed)) + 1;
}

// the keys (i, j) of K off the diagonal without their reverse: row j of K is searched for i
__global__ void __launch_bounds__(256) k_agg_asym(const int32_t *__restrict__ ki, const int32_t *__restrict__ kj, uint32_t n,
	const uint32_t *__restrict__ kptr, unsigned long long *acc)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false;
	if (t < n) {
		const int32_t i = ki[t], j = kj[t];
		if (i != j) {
			const uint32_t e = kptr[j + 1], p = col_lower_bound(kj, kptr[j], e, i);
			bad = p == e || kj[p] != i;
		}
	}
	const uint64_t m = __ballot(bad);
	if (lane_id() == 0 && m) atomicAdd(&acc[AGG_ASYM], (unsigned long long)__popcll(m));
}

// ---------------------------------------------------------------- sweep

// T1[w] by one thread; does w stay on the spread list?  The walk ends at the first root.
__device__ __forceinline__ bool agg_spread_thread(const AggArgs &a, uint32_t w)
{
	uint64_t m = a.word[w];
	bool und = agg_undecided(m);
	const uint32_t e = a.ptr[w + 1];
	for (uint32_t t = a.ptr[w]; t < e && m != AGG_ROOT; ++t) {
		const uint64_t x = a.word[a.adj[t]];
		und |= agg_undecided(x);
		m = max(m, x);
	}
	a.t1[w] = m;
	return und && m != AGG_ROOT;
}

// The same by one wave (every lane gets the answer): the lanes stride the row 64 neighbours at a time.
__device__ __forceinline__ bool agg_spread_wave(const AggArgs &a, uint32_t w)
{
	const uint32_t b = a.ptr[w], e = a.ptr[w + 1], lane = lane_id();
	uint64_t m = a.word[w];
	bool und = agg_undecided(m);
	for (uint32_t t0 = b; t0 < e; t0 += 64) {                          // uniform
		const uint32_t t = t0 + lane;
		if (t < e) {
			const uint64_t x = a.word[a.adj[t]];
			und |= agg_undecided(x);
			m = max(m, x);
		}
		if (__ballot(m == AGG_ROOT)) { m = AGG_ROOT; break; }           // uniform
	}
	m = wave_reduce_max_u64(m);
	if (lane == 0) a.t1[w] = m;
	return __ballot(und) != 0 && m != AGG_ROOT;
}

// T2 of v by one thread, and v's new word (its old one: v waits)
__device__ __forceinline__ uint64_t agg_decide_thread(const AggArgs &a, uint32_t v, uint64_t own)
{
	uint64_t m = a.t1[v];
	const uint32_t e = a.ptr[v + 1];
	for (uint32_t t = a.ptr[v]; t < e && m != AGG_ROOT; ++t) m = max(m, a.t1[a.adj[t]]);
	return m == AGG_ROOT ? 0 : m == own ? AGG_ROOT : own;
}

__device__ __forceinline__ uint64_t agg_decide_wave(const AggArgs &a, uint32_t v, uint64_t own)
{
	const uint32_t b = a.ptr[v], e = a.ptr[v + 1], lane = lane_id();
	uint64_t m = a.t1[v];
	for (uint32_t t0 = b; t0 < e; t0 += 64) {                          // uniform
		const uint32_t t = t0 + lane;
		if (t < e) m = max(m, a.t1[a.adj[t]]);
		if (__ballot(m == AGG_ROOT)) { m = AGG_ROOT; break; }           // uniform
	}
	m = wave_reduce_max_u64(m);
	return m == AGG_ROOT ? 0 : m == own ? AGG_ROOT : own;
}

// The thread kernels take PER list entries per thread, a block's entries 256 apart, and append what stays with ONE atomic per
// wave for all of them (wave_claim's scheme over PER ballots).  PER = AGG_PER on a list long enough to give every CU a
// workgroup that way (the agg_per_rows knob: on a list of that many entries): a list of 16.8 M vertices is 65 k atomics on its counter instead of 262 k, which at some 90
// same-address atomics per microsecond was two thirds of a wide round.  On a shorter list the atomics are few and four
// rows in a row per thread only lengthen the kernel (R-MAT 16: 1.8 ms against 1.5): PER = 1.
constexpr int AGG_PER = 4;
template <int PER>
__device__ __forceinline__ void agg_append(uint32_t *counter, uint32_t *__restrict__ next, const uint32_t (&v)[PER], const bool (&keep)[PER])
{
	uint64_t m[PER];
	uint32_t total = 0;
#pragma unroll
	for (int k = 0; k < PER; ++k) { m[k] = __ballot(keep[k]); total += (uint32_t)__popcll(m[k]); }
	if (!total) return;                                                // uniform
	uint32_t at = 0;
	if (lane_id() == 0) at = atomicAdd(counter, total);
	at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		if (keep[k]) next[at + (uint32_t)__popcll(m[k] & lanemask_lt())] = v[k];
		at += (uint32_t)__popcll(m[k]);
	}
}

template <int PER>
__global__ void __launch_bounds__(256) k_agg_spread_thread(AggArgs a, const uint32_t *__restrict__ list, uint32_t cnt, uint32_t *__restrict__ next,
	uint32_t *ctr_next)
{
	uint32_t w[PER];
	bool keep[PER];
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const uint64_t p = ((uint64_t)blockIdx.x * PER + k) * blockDim.x + threadIdx.x;
		w[k] = 0; keep[k] = false;
		if (p < cnt) { w[k] = list[p]; keep[k] = agg_spread_thread(a, w[k]); }
	}
	agg_append<PER>(ctr_next, next, w, keep);
}

__global__ void __launch_bounds__(256) k_agg_spread_wave(AggArgs a, const uint32_t *__restrict__ list, uint32_t cnt, uint32_t *__restrict__ next,
	uint32_t *ctr_next)
{
	const uint64_t p = (uint64_t)blockIdx.x * 4 + wave_id();
	if (p >= cnt) return;                                              // uniform
	const uint32_t w = list[p];
	if (agg_spread_wave(a, w) && lane_id() == 0) next[atomicAdd(ctr_next, 1u)] = w;
}

// ctr_zero: the four counters of the lists this round read, which the round after this one appends to
template <int PER>
__global__ void __launch_bounds__(256) k_agg_decide_thread(AggArgs a, const uint32_t *__restrict__ list, uint32_t cnt, uint32_t *__restrict__ next,
	uint32_t *ctr_next, uint32_t *ctr_zero)
{
	if (blockIdx.x == 0 && threadIdx.x < 4) ctr_zero[threadIdx.x] = 0;
	uint32_t v[PER];
	bool keep[PER];
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const uint64_t p = ((uint64_t)blockIdx.x * PER + k) * blockDim.x + threadIdx.x;
		v[k] = 0; keep[k] = false;
		if (p < cnt) {
			v[k] = list[p];
			const uint64_t own = a.word[v[k]], nw = agg_decide_thread(a, v[k], own);
			keep[k] = nw == own;
			if (!keep[k]) a.word[v[k]] = nw;
		}
	}
	agg_append<PER>(ctr_next, next, v, keep);
}

__global__ void __launch_bounds__(256) k_agg_decide_wave(AggArgs a, const uint32_t *__restrict__ list, uint32_t cnt, uint32_t *__restrict__ next,
	uint32_t *ctr_next, uint32_t *ctr_zero)
{
	if (blockIdx.x == 0 && threadIdx.x < 4) ctr_zero[threadIdx.x] = 0;
	const uint64_t p = (uint64_t)blockIdx.x * 4 + wave_id();
	if (p >= cnt) return;                                              // uniform
	const uint32_t v = list[p];
	const uint64_t own = a.word[v], nw = agg_decide_wave(a, v, own);
	if (lane_id() == 0) {
		if (nw == own) next[atomicAdd(ctr_next, 1u)] = v;
		else a.word[v] = nw;
	}
}

// ---- fused run: every remaining round, one workgroup; the threads stride the thread-class lists, the sixteen waves the
// wave-class ones.  A round spreads (words read, T1 written), a barrier, decides (T1 read, words written), a barrier.
// s_n[r % 3] counts the four lists that round r appends to: [0] [1] undecided, [2] [3] spread, thread- and wave-class.  It
// is zeroed in round r - 1 before that round's first barrier (s_n[0] ahead of the loop), and was last read between round
// r - 3's second barrier and round r - 2's first.
__global__ void __launch_bounds__(AGG_NT) k_agg_fused(AggArgs a, uint32_t *ut0, uint32_t *ut1, uint32_t cnt_ut, uint32_t *uw0, uint32_t *uw1,
	uint32_t cnt_uw, uint32_t *st0, uint32_t *st1, uint32_t cnt_st, uint32_t *sw0, uint32_t *sw1, uint32_t cnt_sw)
{
	__shared__ uint32_t s_n[3][4];
	if (threadIdx.x < 4) s_n[0][threadIdx.x] = 0;
	__syncthreads();
	uint32_t r = 0;
	while (cnt_ut | cnt_uw) {                                          // uniform
		uint32_t *ctr = s_n[r % 3];
		if (threadIdx.x < 4) s_n[(r + 1) % 3][threadIdx.x] = 0;
		for (uint32_t base = 0; base < cnt_st; base += AGG_NT) {       // uniform
			const uint32_t p = base + threadIdx.x;
			uint32_t w = 0;
			bool keep = false;
			if (p < cnt_st) { w = st0[p]; keep = agg_spread_thread(a, w); }
			const uint32_t s = wave_claim(ctr + 2, keep);
			if (keep) st1[s] = w;
		}
		for (uint32_t p = wave_id(); p < cnt_sw; p += AGG_NT / 64) {   // uniform in the wave
			const uint32_t w = sw0[p];
			if (agg_spread_wave(a, w) && lane_id() == 0) sw1[atomicAdd(ctr + 3, 1u)] = w;
		}
		__syncthreads();                                               // T1 is this round's, and visible to the workgroup
		for (uint32_t base = 0; base < cnt_ut; base += AGG_NT) {       // uniform
			const uint32_t p = base + threadIdx.x;
			uint32_t v = 0;
			bool keep = false;
			if (p < cnt_ut) {
				v = ut0[p];
				const uint64_t own = a.word[v], nw = agg_decide_thread(a, v, own);
				keep = nw == own;
				if (!keep) a.word[v] = nw;
			}
			const uint32_t s = wave_claim(ctr, keep);
			if (keep) ut1[s] = v;
		}
		for (uint32_t p = wave_id(); p < cnt_uw; p += AGG_NT / 64) {   // uniform in the wave
			const uint32_t v = uw0[p];
			const uint64_t own = a.word[v], nw = agg_decide_wave(a, v, own);
			if (lane_id() == 0) {
				if (nw == own) uw1[atomicAdd(ctr + 1, 1u)] = v;
				else a.word[v] = nw;
			}
		}
		__syncthreads();                                               // this round's words are final, and visible to the workgroup
		cnt_ut = ctr[0]; cnt_uw = ctr[1]; cnt_st = ctr[2]; cnt_sw = ctr[3];
		uint32_t *x = ut0; ut0 = ut1; ut1 = x;
		x = uw0; uw0 = uw1; uw1 = x;
		x = st0; st0 = st1; st1 = x;
		x = sw0; sw0 = sw1; sw1 = x;
		++r;
	}
	if (threadIdx.x == 0) a.acc[AGG_FUSED] = r;
}

// ---------------------------------------------------------------- assignment

__global__ void __launch_bounds__(256) k_agg_flags(const uint64_t *__restrict__ word, uint64_t n, uint8_t *__restrict__ root)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n) root[v] = word[v] == AGG_ROOT;
}

struct RingArgs {
	const uint32_t *ptr;
	const int32_t *adj;
	const uint32_t *deg;
	const uint8_t *root;                       // the flags
	const uint32_t *id;                        // their exclusive scan
	int32_t *agg;
	uint8_t *ring;
	unsigned long long *acc;
	uint64_t n;
	uint32_t seed;
	int by_degree;
};

// Both ring kernels: a thread per vertex for the short rows, then the wave takes its long rows one by one, the lanes
// striding the row (no lists: every vertex is looked at once).

// Rings 0 and 1: a root takes its id, a vertex with a root in its row the root's; everybody else is ring 2 and has -1 for now.
__global__ void __launch_bounds__(256) k_agg_ring1(RingArgs a)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool in = v < a.n;
	uint32_t b = 0, e = 0;
	int32_t g = -1;
	bool isroot = false;
	if (in) {
		b = a.ptr[v]; e = a.ptr[v + 1];
		isroot = a.root[v] != 0;
		if (isroot) g = (int32_t)a.id[v];
	}
	const bool walk = in && !isroot;
	const bool longrow = walk && e - b > AGG_RING_LONG;
	if (walk && !longrow)
		for (uint32_t t = b; t < e; ++t) {
			const uint32_t u = (uint32_t)a.adj[t];
			if (a.root[u]) { g = (int32_t)a.id[u]; break; }
		}
	for (uint64_t todo = __ballot(longrow); todo; todo &= todo - 1) {      // uniform
		const int src = __ffsll((unsigned long long)todo) - 1;
		const uint32_t rb = __shfl(b, src, 64), re = __shfl(e, src, 64);
		int32_t found = -1;
		for (uint32_t t0 = rb; t0 < re; t0 += 64) {                    // uniform
			const uint32_t t = t0 + lane_id();
			if (t < re) {
				const uint32_t u = (uint32_t)a.adj[t];
				if (a.root[u]) found = (int32_t)a.id[u];
			}
			if (__ballot(found >= 0)) break;                           // uniform
		}
		found = wave_reduce_max(found);                                // (one root at most)
		if ((int)lane_id() == src) g = found;
	}
	const int ring = isroot ? 0 : g >= 0 ? 1 : 2;
	if (in) { a.agg[v] = g; a.ring[v] = (uint8_t)ring; }
	const uint64_t m1 = __ballot(in && ring == 1), m2 = __ballot(in && ring == 2);
	if (lane_id() == 0) {
		if (m1) atomicAdd(&a.acc[AGG_RING1], (unsigned long long)__popcll(m1));
		if (m2) atomicAdd(&a.acc[AGG_RING2], (unsigned long long)__popcll(m2));
	}
}

__device__ __forceinline__ uint64_t ring_key(const RingArgs &a, uint32_t w)
{
	return ((a.by_degree ? (uint64_t)a.deg[w] << 32 : 0ull) | col_hash(w, a.seed)) + 1;
}

// Ring 2: the aggregate of the ring-1 neighbour with the largest key.  It reads the ids of ring-1 vertices and writes those
// of ring-2 vertices, which no thread of this launch reads.
__global__ void __launch_bounds__(256) k_agg_ring2(RingArgs a)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const bool walk = v < a.n && a.ring[v] == 2;
	uint32_t b = 0, e = 0;
	if (walk) { b = a.ptr[v]; e = a.ptr[v + 1]; }
	const bool longrow = walk && e - b > AGG_RING_LONG;
	uint64_t best = 0;
	int32_t g = -1;
	if (walk && !longrow)
		for (uint32_t t = b; t < e; ++t) {
			const uint32_t w = (uint32_t)a.adj[t];
			if (a.ring[w] != 1) continue;
			const uint64_t k = ring_key(a, w);
			if (k > best) { best = k; g = a.agg[w]; }
		}
	for (uint64_t todo = __ballot(longrow); todo; todo &= todo - 1) {      // uniform
		const int src = __ffsll((unsigned long long)todo) - 1;
		const uint32_t rb = __shfl(b, src, 64), re = __shfl(e, src, 64);
		uint64_t lbest = 0;
		int32_t lg = -1;
		for (uint32_t t = rb + lane_id(); t < re; t += 64) {
			const uint32_t w = (uint32_t)a.adj[t];
			if (a.ring[w] != 1) continue;
			const uint64_t k = ring_key(a, w);
			if (k > lbest) { lbest = k; lg = a.agg[w]; }
		}
		const uint64_t wbest = wave_reduce_max_u64(lbest);
		const uint64_t holder = __ballot(lbest == wbest);              // (keys never tie: one lane, unless no lane found any)
		const int32_t wg = __shfl(lg, __ffsll((unsigned long long)holder) - 1, 64);
		if ((int)lane_id() == src) g = wg;
	}
	if (walk) a.agg[v] = g;
}

// the sort keys of members and agg_ptr
__global__ void __launch_bounds__(256) k_agg_keys(const int32_t *__restrict__ agg, const uint8_t *__restrict__ ring, uint64_t n, uint64_t *__restrict__ keys)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n) keys[v] = (uint64_t)(uint32_t)agg[v] << 2 | ring[v];
}

// the largest and the smallest difference of the bounds
__global__ void __launch_bounds__(256) k_agg_sizes(const uint32_t *__restrict__ aptr, uint64_t nagg, unsigned long long *acc)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t mx = 0, mn = 0;                                               // (mn: 2^32 - 1 - size)
	if (p < nagg) { const uint32_t d = aptr[p + 1] - aptr[p]; mx = d; mn = 0xFFFFFFFFu - d; }
	mx = wave_reduce_max_u64(mx); mn = wave_reduce_max_u64(mn);
	if (lane_id() == 0) {
		atomicMax(&acc[AGG_MAXSZ], (unsigned long long)mx);
		atomicMax(&acc[AGG_MINSZ], (unsigned long long)mn);
	}
}

// ---------------------------------------------------------------- host

// The call runs inside GraphCall (internal.h, k_color.hip); here are the lists, the two launch bodies and the assignment.
// Four lists a parity: [4 * parity + list] of ctr is undecided thread, wave; spread thread, wave.
static const GraphOp AGG_OP = {"unknown aggregation order", "unknown agg_flags", "op(A) must be square for an aggregation",
	"agg, members and agg_ptr overlap", "agg_ptr is too small: it needs one entry per aggregate and one more; *out_naggregates holds the aggregates",
	&Tuning::agg_path, &Tuning::agg_row, &Tuning::agg_fuse_rows, &Tuning::agg_wave_deg, AGG_FUSE_ROWS, AGG_WAVE_DEG, AGG_ACC, 4};

int aggregate_graph(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int agg_flags, int32_t *agg,
	int32_t *members, int32_t *agg_ptr, size_t ptr_capacity, int mem, size_t *out_naggregates, spsamd_aggregate_stats *stats,
	spsamd_result *res)
{
	GraphCall gc{c, &AGG_OP, agg, members, agg_ptr, ptr_capacity, out_naggregates, res};
	int rc;
	if (!gc.open(A, transpose, order, agg_flags, mem, stats, sizeof(*stats), &rc)) return rc;
	hipStream_t st = c->stream;
	const uint64_t N = gc.N; const MaskKeys &K = gc.K; const GraphRows &g = gc.g;
	unsigned long long *acc = gc.acc; uint32_t *ctr = gc.ctr, *deg = gc.deg;
	int32_t *ids = gc.ids;                                              // the aggregate ids (until then: what graph_classes calls colours)

	// ---- the lists, and the promise checked
	uint64_t *word = c->arena.get<uint64_t>(N), *t1 = c->arena.get<uint64_t>(N);
	uint32_t *ut[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)}, *uw[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)};
	uint32_t *sl[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)}, *sw[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)};
	graph_classes(c, g, N, deg, ids, ut[0], uw[0], ctr, acc, gc.wave_deg, gc.rowk, 1);
	if (gc.symmetric && K.n) { k_agg_asym<<<dim3(grid_for(K.n)), dim3(256), 0, st>>>(K.i, K.j, K.n, g.ptr, acc); SPS_LAUNCH_CHECK(); }
	k_agg_words<<<dim3(grid_for(N)), dim3(256), 0, st>>>(deg, N, seed, order == SPSAMD_AGG_ORDER_DEGREE, word);
	SPS_LAUNCH_CHECK();
	uint32_t cnt0[4];
	{                                                                  // the round-0 lists' lengths and the asymmetric keys in one trip
		WordList wl;
		wl.add(ctr); wl.add(ctr + 1);
		const int at = wl.add64(&acc[AGG_ASYM]);
		uint32_t hw[4];
		read_back_words(c, wl, hw);
		cnt0[0] = cnt0[2] = hw[0]; cnt0[1] = cnt0[3] = hw[1];
		const uint64_t asym = (uint64_t)hw[at + 1] << 32 | hw[at];
		if (asym) {
			if (stats) stats->asymmetric = asym;
			throw Error{SPSAMD_EINVAL, "SPSAMD_AGG_SYMMETRIC: the pattern is not symmetric (" + std::to_string(asym) + " keys without their reverse)"};
		}
	}
	// the spread lists of round 0 are the undecided ones: every vertex
	if (cnt0[0]) SPS_HIP(hipMemcpyAsync(sl[0], ut[0], (size_t)cnt0[0] * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
	if (cnt0[1]) SPS_HIP(hipMemcpyAsync(sw[0], uw[0], (size_t)cnt0[1] * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));

	// ---- sweep
	AggArgs a;
	a.ptr = g.ptr; a.adj = g.adj; a.word = word; a.t1 = t1; a.acc = acc;
	const uint32_t per_min = c->tune.agg_per_rows > 0 ? (uint32_t)c->tune.agg_per_rows : (uint32_t)std::max(c->num_cu, 1) * 256u * AGG_PER;
	gc.sweep(cnt0,
		[&](int par, const uint32_t *cnt) {
			const int nx = par ^ 1;
			uint32_t *cn = ctr + 4 * nx, *cz = ctr + 4 * par;
			uint64_t launches = 0;
			if (cnt[2] >= per_min) { k_agg_spread_thread<AGG_PER><<<dim3(grid_for(cnt[2], 256 * AGG_PER)), dim3(256), 0, st>>>(a, sl[par], cnt[2], sl[nx], cn + 2); SPS_LAUNCH_CHECK(); ++launches; }
			else if (cnt[2]) { k_agg_spread_thread<1><<<dim3(grid_for(cnt[2])), dim3(256), 0, st>>>(a, sl[par], cnt[2], sl[nx], cn + 2); SPS_LAUNCH_CHECK(); ++launches; }
			if (cnt[3]) { k_agg_spread_wave<<<dim3(grid_for(cnt[3], 4)), dim3(256), 0, st>>>(a, sw[par], cnt[3], sw[nx], cn + 3); SPS_LAUNCH_CHECK(); ++launches; }
			if (cnt[0] >= per_min) { k_agg_decide_thread<AGG_PER><<<dim3(grid_for(cnt[0], 256 * AGG_PER)), dim3(256), 0, st>>>(a, ut[par], cnt[0], ut[nx], cn, cz); SPS_LAUNCH_CHECK(); ++launches; }
			else if (cnt[0]) { k_agg_decide_thread<1><<<dim3(grid_for(cnt[0])), dim3(256), 0, st>>>(a, ut[par], cnt[0], ut[nx], cn, cz); SPS_LAUNCH_CHECK(); ++launches; }
			if (cnt[1]) { k_agg_decide_wave<<<dim3(grid_for(cnt[1], 4)), dim3(256), 0, st>>>(a, uw[par], cnt[1], uw[nx], cn + 1, cz); SPS_LAUNCH_CHECK(); ++launches; }
			return launches;
		},
		[&](int par, const uint32_t *cnt) {
			const int nx = par ^ 1;
			k_agg_fused<<<dim3(1), dim3(AGG_NT), 0, st>>>(a, ut[par], ut[nx], cnt[0], uw[par], uw[nx], cnt[1], sl[par], sl[nx], cnt[2],
				sw[par], sw[nx], cnt[3]);
			SPS_LAUNCH_CHECK();
		});
	SPS_HIP(hipEventRecord(c->ev[EV_N0], st));

	// ---- assignment
	uint8_t *root = c->arena.get<uint8_t>(N), *ring = c->arena.get<uint8_t>(N);
	uint32_t *rid = c->arena.get<uint32_t>(N + 1);
	k_agg_flags<<<dim3(grid_for(N)), dim3(256), 0, st>>>(word, N, root);
	SPS_LAUNCH_CHECK();
	scan_exclusive_u8_u32(c, root, rid, N);
	const uint64_t nagg = read_back(c, rid + N);
	if (!gc.fits(nagg)) return SPSAMD_ECAPACITY;
	RingArgs ra;
	ra.ptr = g.ptr; ra.adj = g.adj; ra.deg = deg; ra.root = root; ra.id = rid; ra.agg = ids; ra.ring = ring; ra.acc = acc; ra.n = N;
	ra.seed = seed; ra.by_degree = order == SPSAMD_AGG_ORDER_DEGREE;
	k_agg_ring1<<<dim3(grid_for(N)), dim3(256), 0, st>>>(ra);
	SPS_LAUNCH_CHECK();
	k_agg_ring2<<<dim3(grid_for(N)), dim3(256), 0, st>>>(ra);
	SPS_LAUNCH_CHECK();

	// ---- members, agg_ptr, the sizes and delivery
	if (members || agg_ptr || stats) {
		PairSort sort(c, N);
		k_agg_keys<<<dim3(grid_for(N)), dim3(256), 0, st>>>(ids, ring, N, sort.keys);
		SPS_LAUNCH_CHECK();
		const uint32_t *aptr = order_by_key(c, sort, N, bits_of(nagg) + 2, 2, nagg, true, members, agg_ptr, gc.kind);   // stable: ascending index inside a ring
		k_agg_sizes<<<dim3(grid_for(nagg)), dim3(256), 0, st>>>(aptr, nagg, acc);
		SPS_LAUNCH_CHECK();
	}
	gc.deliver();
	const unsigned long long *hacc = (const unsigned long long *)gc.h;    // (there once close() has waited for the stream)
	SPS_HIP(hipMemcpyAsync(gc.h, acc, AGG_ACC * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
	const GraphTotals t = gc.close(hacc, AGG_FUSED);
	if (stats) {
		stats->naggregates = nagg; stats->rounds = gc.rounds + t.fused_rounds;
		stats->ring1 = hacc[AGG_RING1]; stats->ring2 = hacc[AGG_RING2];
		stats->max_size = hacc[AGG_MAXSZ]; stats->min_size = 0xFFFFFFFFull - hacc[AGG_MINSZ];
		stats->adjacency = t.adjacency; stats->max_degree = t.max_degree; stats->asymmetric = 0;
		stats->launches = t.launches; stats->fused_rounds = t.fused_rounds;
		stats->rows_wave = t.rows_wave; stats->rows_thread = N - t.rows_wave;
		stats->ms_adjacency = t.ms_adjacency;
		SPS_HIP(hipEventElapsedTime(&stats->ms_sweep, c->ev[EV_SYMBOLIC], c->ev[EV_N0]));
		SPS_HIP(hipEventElapsedTime(&stats->ms_assign, c->ev[EV_N0], c->ev[EV_END]));
	}
	return SPSAMD_OK;
}

} // namespace spsamd
