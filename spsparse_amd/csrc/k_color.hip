// k_color.hip -- a greedy multi-colour ordering of op(A)'s graph by independent sets (spsamd_color, include/spsparse_amd.h;
// DESIGN.md section 22).
//
// K = the sorted unique keys of op(A) as mask_keys() hands them over.  The graph is K symmetrised without its diagonal, or
// K's own rows under SPSAMD_COLOR_SYMMETRIC.  Every output is defined by the serial loop of the header: the vertices in
// descending key(v) = deg << 32 | hash (or the hash alone), each taking the smallest colour no coloured neighbour holds.
// What is parallel is a Jones-Plassmann sweep with first-fit colours, synchronous in rounds: a vertex is coloured in round r
// exactly when every neighbour that precedes it was coloured before round r.  At that moment its coloured neighbours are
// exactly the neighbours that precede it -- a later neighbour waits for the vertex itself -- so first fit sees what the
// serial loop sees, and the round a vertex is coloured in is round(v) of the header.  (Under the flag the rows need not be
// symmetric: first fit then counts the coloured neighbours that precede the vertex, and only those: col_holds.)
//
// Adjacency (per call): with the flag the row pointer over K; without it the keys (i, j) and (j, i) of K, sorted, made
// unique and stripped of the diagonal, then the row pointer.  k_col_init: deg, the isolated vertices' colour 0 (without the flag), the two
// worklists (thread-class and wave-class vertices), the degree sum and maximum.
// Sweep: a round is k_col_thread over the thread-class worklist (a thread per vertex, the forbidden colours in a 64-bit
// mask over a window of 64 colours), k_col_wave over the wave-class one (a wave per vertex, the lanes stride the row, the
// masks OR-reduced over the wave), then k_col_commit, which stores the winners' pending colours and appends the others to
// the next worklists.  The round kernels read committed colours only and write pending ones; winners of one round are never
// adjacent.  The worklist only shrinks: once it is thin it stays so, and the rest of the sweep is ONE launch of ONE
// workgroup, k_col_fused, with __syncthreads() between the phases of a round (plain stores, workgroup barrier: k_fac_fused's
// visibility rule).  No kernel here waits on a value another workgroup writes in the same launch.  A waiting vertex
// remembers where in its row it stopped (wait[]), so the waiting costs one walk of the row, however many rounds it takes.
// The worklists are appended to through a counter, so their order varies from run to run; nothing that is returned depends
// on it.
#include "internal.h"
#include "devutil.h"

#include <algorithm>
#include <cstring>

namespace spsamd {

constexpr uint32_t COL_FUSE_ROWS = 1024;              // default of the color_fuse_rows knob: one vertex per thread of the fused run
constexpr uint32_t COL_WAVE_DEG = 16;                 // default of color_wave_deg: the largest degree of a thread-class vertex
constexpr int COL_NT = SOLVE_NT;                      // threads of k_col_fused's one workgroup

// acc[]: the counters of one call
enum { COL_NCOLORS = GRAPH_ACC, COL_CONFLICTS = 5, COL_FUSED = 6, COL_ACC = 8 };   // (after graph_classes' four)

struct ColArgs {
	const uint32_t *ptr;                       // row pointer of the adjacency
	const int32_t *adj;                        // the neighbours, ascending inside a row; with the flag the row may name v itself
	const uint32_t *deg;
	int32_t *color;                            // committed colours (-1: none yet)
	int32_t *pending;                          // what the round kernels decide (-1: the vertex waits)
	uint32_t *wait;                            // where in its row a waiting vertex looks next (col_row_thread)
	unsigned long long *acc;
	uint32_t seed;
	int by_degree;
	int directed;                              // the rows are taken on the caller's word (SPSAMD_COLOR_SYMMETRIC): see col_holds
};

__device__ __forceinline__ uint64_t col_key(const ColArgs &a, uint32_t v)
{
	return (a.by_degree ? (uint64_t)a.deg[v] << 32 : 0ull) | col_hash(v, a.seed);
}

// Does the coloured neighbour u of v forbid its colour?  In a symmetric graph every coloured neighbour of a winner precedes
// it (a later one waits for the winner itself).  Rows taken on the caller's word may name a later vertex that never saw v and
// is coloured already; the serial loop has not reached it when it colours v, so it does not count.
__device__ __forceinline__ bool col_holds(const ColArgs &a, uint32_t u, uint64_t kv)
{
	return !a.directed || col_key(a, u) > kv;
}

__device__ __forceinline__ uint64_t wave_reduce_or(uint64_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
	return v;
}

// ---------------------------------------------------------------- adjacency

// the keys (i, j) and (j, i) of every key of K
__global__ void __launch_bounds__(256) k_col_sym_keys(const int32_t *__restrict__ ki, const int32_t *__restrict__ kj, uint32_t n, int bits,
	uint64_t *__restrict__ keys)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n) return;
	const uint64_t i = (uint32_t)ki[t], j = (uint32_t)kj[t];
	keys[2 * t] = i << bits | j;
	keys[2 * t + 1] = j << bits | i;
}

// 1 where a sorted key is the first of its value and off the diagonal
__global__ void __launch_bounds__(256) k_col_first(const uint64_t *__restrict__ keys, uint64_t m, int bits, uint8_t *__restrict__ first)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= m) return;
	const uint64_t k = keys[t];
	first[t] = (t == 0 || k != keys[t - 1]) && (k >> bits) != (k & ((uint64_t(1) << bits) - 1));
}

__global__ void __launch_bounds__(256) k_col_unique(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ first,
	const uint32_t *__restrict__ off, uint64_t m, int bits, int32_t *__restrict__ ai, int32_t *__restrict__ aj)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= m || !first[t]) return;
	const uint64_t k = keys[t];
	ai[off[t]] = (int32_t)(k >> bits);
	aj[off[t]] = (int32_t)(k & ((uint64_t(1) << bits) - 1));
}

// 0: isolated | 1 thread | 2 wave
__device__ __forceinline__ int col_class(uint32_t deg, uint32_t wave_deg, int rowk)
{
	if (deg == 0) return 0;
	if (rowk) return rowk;
	return deg <= wave_deg ? 1 : 2;
}

// Per vertex its degree (the row without v itself) and, for an isolated one, colour 0; the worklists of round 0; the totals.
// `directed`: an isolated vertex may still be named by a row, whose vertex has to see it coloured in round 0 and not before:
// it goes on the thread-class worklist instead.
constexpr int COL_INIT_PER = 8;                       // vertices per thread of k_col_init: the totals cost one set of atomics per wave
__global__ void __launch_bounds__(256) k_col_init(const uint32_t *__restrict__ ptr, const int32_t *__restrict__ adj, uint64_t n,
	uint32_t *__restrict__ deg, int32_t *__restrict__ color, uint32_t *__restrict__ list_t, uint32_t *__restrict__ list_w, uint32_t *ctr,
	unsigned long long *acc, uint32_t wave_deg, int rowk, int directed)
{
	unsigned long long tot = 0;
	uint32_t md = 0, n1 = 0, n2 = 0;
	for (int k = 0; k < COL_INIT_PER; ++k) {                           // uniform
		const uint64_t i = ((uint64_t)blockIdx.x * COL_INIT_PER + k) * blockDim.x + threadIdx.x;
		uint32_t d = 0;
		if (i < n) {
			const uint32_t b = ptr[i], e = ptr[i + 1];
			d = e - b;
			if (d) {
				const uint32_t p = col_lower_bound(adj, b, e, (int32_t)i);
				if (p < e && adj[p] == (int32_t)i) --d;
			}
			deg[i] = d;
			color[i] = d || directed ? -1 : 0;
		}
		const int cl = col_class(d, wave_deg, rowk);
		const bool on_t = cl == 1 || (directed && i < n && d == 0);
		const uint32_t st = wave_claim(ctr, on_t);
		if (on_t) list_t[st] = (uint32_t)i;
		const uint32_t sw = wave_claim(ctr + 1, cl == 2);
		if (cl == 2) list_w[sw] = (uint32_t)i;
		tot += d;
		md = max(md, d);
		n1 += (uint32_t)__popcll(__ballot(cl == 1)); n2 += (uint32_t)__popcll(__ballot(cl == 2));
	}
	tot = wave_reduce_sum<unsigned long long>(tot);
	const int32_t wmd = wave_reduce_max((int32_t)std::min<uint32_t>(md, 0x7FFFFFFFu));
	if (lane_id() == 0 && tot) {
		atomicAdd(&acc[GRAPH_ADJ], tot);
		atomicMax(&acc[GRAPH_MAXDEG], (unsigned long long)wmd);
		if (n1) atomicAdd(&acc[GRAPH_ROWS_T], (unsigned long long)n1);
		if (n2) atomicAdd(&acc[GRAPH_ROWS_W], (unsigned long long)n2);
	}
}

// ---------------------------------------------------------------- sweep

// Vertex v by one thread: -1 if an uncoloured neighbour precedes it, else its first-fit colour.  wait[v] is where the last
// look stopped: the neighbours in front of it were coloured, or later than v, then, and stay so -- so a vertex that waits
// R rounds pays one walk of its row for the waiting, not R.  The forbidden colours of the window [base, base + 64) are a
// mask in registers; a full window moves the base up and walks the row again.  A first look collects window 0 on its way.
__device__ __forceinline__ int32_t col_row_thread(const ColArgs &a, uint32_t v)
{
	const uint32_t b = a.ptr[v], e = a.ptr[v + 1], w0 = a.wait[v];
	const uint64_t kv = col_key(a, v);
	uint64_t mask = 0;
	for (uint32_t t = b + w0; t < e; ++t) {
		const uint32_t u = (uint32_t)a.adj[t];
		if (u == v) continue;
		const int32_t cu = a.color[u];
		if (cu < 0) {
			if (col_key(a, u) > kv) { if (t - b != w0) a.wait[v] = t - b; return -1; }
		} else if (w0 == 0 && cu < 64 && col_holds(a, u, kv)) mask |= 1ull << cu;
	}
	int32_t base = 0;
	if (w0) { base = -64; mask = ~0ull; }                              // a resumed look has no mask yet: window 0 is walked below
	while (mask == ~0ull) {
		base += 64;
		mask = 0;
		for (uint32_t t = b; t < e; ++t) {
			const uint32_t u = (uint32_t)a.adj[t];
			const uint32_t w = (uint32_t)(a.color[u] - base);          // (an uncoloured neighbour: far outside the window)
			if (u != v && w < 64u && col_holds(a, u, kv)) mask |= 1ull << w;
		}
	}
	return base + (__ffsll((unsigned long long)~mask) - 1);
}

// The same by one wave (every lane gets the answer): the lanes stride the row 64 neighbours at a time, the look stops at
// the first chunk with a neighbour to wait for, the masks are OR-reduced.
__device__ __forceinline__ int32_t col_row_wave(const ColArgs &a, uint32_t v)
{
	const uint32_t b = a.ptr[v], e = a.ptr[v + 1], lane = lane_id(), w0 = a.wait[v];
	const uint64_t kv = col_key(a, v);
	uint64_t mask = 0;
	for (uint32_t t0 = b + w0; t0 < e; t0 += 64) {                     // uniform
		const uint32_t t = t0 + lane;
		bool lose = false;
		if (t < e) {
			const uint32_t u = (uint32_t)a.adj[t];
			const int32_t cu = u == v ? 0x7FFFFFFF : a.color[u];
			if (cu < 0) lose = col_key(a, u) > kv;
			else if (w0 == 0 && cu < 64 && col_holds(a, u, kv)) mask |= 1ull << cu;
		}
		const uint64_t m = __ballot(lose);
		if (m) {                                                       // uniform
			const uint32_t at = t0 - b + (uint32_t)__ffsll((unsigned long long)m) - 1;
			if (lane == 0 && at != w0) a.wait[v] = at;
			return -1;
		}
	}
	int32_t base = 0;
	mask = w0 ? ~0ull : wave_reduce_or(mask);
	if (w0) base = -64;
	while (mask == ~0ull) {                                            // uniform
		base += 64;
		mask = 0;
		for (uint32_t t = b + lane; t < e; t += 64) {
			const uint32_t u = (uint32_t)a.adj[t];
			const uint32_t w = (uint32_t)(a.color[u] - base);
			if (u != v && w < 64u && col_holds(a, u, kv)) mask |= 1ull << w;
		}
		mask = wave_reduce_or(mask);
	}
	return base + (__ffsll((unsigned long long)~mask) - 1);
}

__global__ void __launch_bounds__(256) k_col_thread(ColArgs a, const uint32_t *__restrict__ list, uint32_t cnt)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= cnt) return;
	const uint32_t v = list[p];
	a.pending[v] = col_row_thread(a, v);
}

__global__ void __launch_bounds__(256) k_col_wave(ColArgs a, const uint32_t *__restrict__ list, uint32_t cnt)
{
	const uint64_t p = (uint64_t)blockIdx.x * 4 + wave_id();
	if (p >= cnt) return;                                              // uniform
	const uint32_t v = list[p];
	const int32_t cv = col_row_wave(a, v);
	if (lane_id() == 0) a.pending[v] = cv;
}

// the largest colour count seen so far (the plain read spares most waves the atomic: the word only grows)
__device__ __forceinline__ void col_note_colors(const ColArgs &a, int32_t mc)
{
	mc = wave_reduce_max(mc);
	if (lane_id() == 0 && mc >= 0 && (unsigned long long)mc + 1 > a.acc[COL_NCOLORS]) atomicMax(&a.acc[COL_NCOLORS], (unsigned long long)mc + 1);
}

// The end of a round: a winner's pending colour becomes its colour, everybody else goes to the next worklist of its class.
// ctr_zero: the counters of the lists this round read, which the round after this one appends to.
__global__ void __launch_bounds__(256) k_col_commit(ColArgs a, const uint32_t *__restrict__ list_t, uint32_t cnt_t,
	const uint32_t *__restrict__ list_w, uint32_t cnt_w, uint32_t *__restrict__ next_t, uint32_t *__restrict__ next_w, uint32_t *ctr_next,
	uint32_t *ctr_zero)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p == 0) { ctr_zero[0] = 0; ctr_zero[1] = 0; }
	const bool in = p < (uint64_t)cnt_t + cnt_w, isw = p >= cnt_t;
	uint32_t v = 0;
	int32_t cv = -1;
	if (in) {
		v = isw ? list_w[p - cnt_t] : list_t[p];
		cv = a.pending[v];
		if (cv >= 0) a.color[v] = cv;
	}
	const bool keep = in && cv < 0;
	const uint32_t st = wave_claim(ctr_next, keep && !isw);
	if (keep && !isw) next_t[st] = v;
	const uint32_t sw = wave_claim(ctr_next + 1, keep && isw);
	if (keep && isw) next_w[sw] = v;
	col_note_colors(a, cv);
}

// one list's part of a fused round's commit: every thread of the workgroup calls it
__device__ __forceinline__ int32_t col_fused_commit(const ColArgs &a, const uint32_t *cur, uint32_t cnt, uint32_t *nxt, uint32_t *ctr, int32_t mc)
{
	for (uint32_t base = 0; base < cnt; base += COL_NT) {              // uniform
		const uint32_t p = base + threadIdx.x;
		const bool in = p < cnt;
		uint32_t v = 0;
		int32_t cv = -1;
		if (in) {
			v = cur[p];
			cv = a.pending[v];
			if (cv >= 0) { a.color[v] = cv; mc = max(mc, cv); }
		}
		const bool keep = in && cv < 0;
		const uint32_t s = wave_claim(ctr, keep);
		if (keep) nxt[s] = v;
	}
	return mc;
}

// ---- fused run: every remaining round, one workgroup; the threads stride the thread-class worklist, the sixteen waves the
// wave-class one.  A round decides (committed colours are read, pending ones written), a barrier, commits and compacts
// (pending read, colours written), a barrier.  s_n[r % 3] counts the two lists that round r appends to: it is zeroed before
// round r's first barrier, and was last read before round r - 2's.
__global__ void __launch_bounds__(COL_NT) k_col_fused(ColArgs a, uint32_t *t0, uint32_t *t1, uint32_t cnt_t, uint32_t *w0, uint32_t *w1,
	uint32_t cnt_w)
{
	__shared__ uint32_t s_n[3][2];
	uint32_t *cur_t = t0, *nxt_t = t1, *cur_w = w0, *nxt_w = w1;
	uint32_t r = 0;
	int32_t mc = -1;
	while (cnt_t | cnt_w) {                                            // uniform
		uint32_t *ctr = s_n[r % 3];
		if (threadIdx.x < 2) ctr[threadIdx.x] = 0;
		for (uint32_t p = threadIdx.x; p < cnt_t; p += COL_NT) { const uint32_t v = cur_t[p]; a.pending[v] = col_row_thread(a, v); }
		for (uint32_t p = wave_id(); p < cnt_w; p += COL_NT / 64) {    // uniform in the wave
			const uint32_t v = cur_w[p];
			const int32_t cv = col_row_wave(a, v);
			if (lane_id() == 0) a.pending[v] = cv;
		}
		__syncthreads();
		mc = col_fused_commit(a, cur_t, cnt_t, nxt_t, ctr, mc);
		mc = col_fused_commit(a, cur_w, cnt_w, nxt_w, ctr + 1, mc);
		__syncthreads();                                               // this round's colours are final, and visible to the workgroup
		cnt_t = ctr[0]; cnt_w = ctr[1];
		uint32_t *x = cur_t; cur_t = nxt_t; nxt_t = x;
		x = cur_w; cur_w = nxt_w; nxt_w = x;
		++r;
	}
	col_note_colors(a, mc);
	if (threadIdx.x == 0) a.acc[COL_FUSED] = r;
}

// ---------------------------------------------------------------- outputs

// the keys of K off the diagonal whose two ends hold one colour
__global__ void __launch_bounds__(256) k_col_conflicts(const int32_t *__restrict__ ki, const int32_t *__restrict__ kj, uint32_t n,
	const int32_t *__restrict__ color, unsigned long long *acc)
{
	const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false;
	if (t < n) { const int32_t i = ki[t], j = kj[t]; bad = i != j && color[i] == color[j]; }
	const uint64_t m = __ballot(bad);
	if (lane_id() == 0 && m) atomicAdd(&acc[COL_CONFLICTS], (unsigned long long)__popcll(m));
}

// the sort keys of perm and color_ptr
__global__ void __launch_bounds__(256) k_col_keys(const int32_t *__restrict__ color, uint64_t n, uint64_t *__restrict__ keys)
{
	const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (v < n) keys[v] = (uint32_t)color[v];
}

// The bounds of the buckets key >> shift in the sorted keys: every bucket below nbuckets occurs (a vertex takes colour c only
// past holders of 0 .. c - 1; every aggregate holds its root).
__global__ void __launch_bounds__(256) k_col_bounds(const uint64_t *__restrict__ keys, uint64_t n, uint64_t nbuckets, int shift, uint32_t *__restrict__ cptr)
{
	const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= n) return;
	const uint64_t k = keys[p] >> shift;
	if (k < nbuckets && (p == 0 || keys[p - 1] >> shift != k)) cptr[k] = (uint32_t)p;
	if (p == n - 1) cptr[nbuckets] = (uint32_t)n;
}

// ---------------------------------------------------------------- host

// The parts spsamd_aggregate runs too (k_aggregate.hip; declared in internal.h).

GraphRows graph_adjacency(spsamd_ctx *c, const MaskKeys &K, uint64_t N, bool symmetric)
{
	hipStream_t st = c->stream;
	const uint32_t *ptr;
	const int32_t *adj;
	if (symmetric) {
		if (K.prep) { prepared_row_structure(c, K.prep); ptr = K.prep->rowptr; }
		else {
			ConMat m;
			m.row = const_cast<int32_t *>(K.i); m.nnz = K.n; m.nrow = N;
			ptr = dense_rowptr(c, m, 0);
		}
		adj = K.j;
	} else {
		ConMat m;
		m.nrow = N;
		if (K.n) {
			const int bits = bits_of(N);
			const uint64_t total = 2 * (uint64_t)K.n;                  // (< 2^32: K.n < 2^31)
			PairSort sort(c, total);
			k_col_sym_keys<<<dim3(grid_for(K.n)), dim3(256), 0, st>>>(K.i, K.j, K.n, bits, sort.keys);
			SPS_LAUNCH_CHECK();
			sort.run(2 * bits);
			uint8_t *first = c->arena.get<uint8_t>(total);
			uint32_t *off = c->arena.get<uint32_t>(total + 1);
			k_col_first<<<dim3(grid_for(total)), dim3(256), 0, st>>>(sort.keys, total, bits, first);
			SPS_LAUNCH_CHECK();
			scan_exclusive_u8_u32(c, first, off, total);
			const uint32_t nu = read_back(c, off + total);
			if (nu) {
				m.row = c->arena.get<int32_t>(nu); m.col = c->arena.get<int32_t>(nu); m.nnz = nu;
				k_col_unique<<<dim3(grid_for(total)), dim3(256), 0, st>>>(sort.keys, first, off, total, bits, m.row, m.col);
				SPS_LAUNCH_CHECK();
			}
		}
		ptr = dense_rowptr(c, m, 0);
		adj = m.col;
	}
	return GraphRows{ptr, adj};
}

void graph_classes(spsamd_ctx *c, const GraphRows &g, uint64_t N, uint32_t *deg, int32_t *color, uint32_t *list_t, uint32_t *list_w,
	uint32_t *ctr, unsigned long long *acc, uint32_t wave_deg, int rowk, int list_isolated)
{
	k_col_init<<<dim3(grid_for(N, 256 * COL_INIT_PER)), dim3(256), 0, c->stream>>>(g.ptr, g.adj, N, deg, color, list_t, list_w, ctr, acc, wave_deg, rowk, list_isolated);
	SPS_LAUNCH_CHECK();
}

uint32_t *order_by_key(spsamd_ctx *c, PairSort &sort, uint64_t N, int key_bits, int shift, uint64_t nbuckets, bool bounds,
	int32_t *list, int32_t *list_ptr, hipMemcpyKind kind)
{
	hipStream_t st = c->stream;
	sort.run(key_bits);
	uint32_t *cptr = nullptr;
	if (bounds) {
		cptr = c->arena.get<uint32_t>(nbuckets + 1);
		k_col_bounds<<<dim3(grid_for(N)), dim3(256), 0, st>>>(sort.keys, N, nbuckets, shift, cptr);
		SPS_LAUNCH_CHECK();
		if (list_ptr) SPS_HIP(hipMemcpyAsync(list_ptr, cptr, (nbuckets + 1) * sizeof(uint32_t), kind, st));
	}
	if (list) SPS_HIP(hipMemcpyAsync(list, sort.perm, N * sizeof(uint32_t), kind, st));
	return cptr;
}

// ---- the frame of a graph call (GraphCall, internal.h)

bool GraphCall::open(const spsamd_coo *A, char transpose, int order, int flags, int mem, void *stats, size_t stats_bytes, int *rc)
{
	if (order != SPSAMD_COLOR_ORDER_HASH && order != SPSAMD_COLOR_ORDER_DEGREE) throw Error{SPSAMD_EINVAL, op->bad_order};
	if (flags & ~SPSAMD_COLOR_SYMMETRIC) throw Error{SPSAMD_EINVAL, op->bad_flags};
	if (mem != SPSAMD_MEM_HOST && mem != SPSAMD_MEM_DEVICE) throw Error{SPSAMD_EINVAL, "mem of the output must be SPSAMD_MEM_HOST or SPSAMD_MEM_DEVICE"};
	const int lead = transpose == 'T' ? 1 : 0;
	N = A->shape0;
	if (A->shape0 != A->shape1) throw Error{SPSAMD_EDIM, op->not_square};
	if (N >= (uint64_t(1) << 31)) throw Error{SPSAMD_EINVAL, "shape exceeds the int32 index range"};
	symmetric = (flags & SPSAMD_COLOR_SYMMETRIC) != 0;
	kind = mem == SPSAMD_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
	{
		const OperandView view = operand_view(c, A);
		const uint64_t n = view.coo.nnz;
		const void *buf[3] = {ids_out, list_out, ptr_out};
		const uint64_t bytes[3] = {N * 4, N * 4, (uint64_t)ptr_capacity * 4};
		for (int p = 0; p < 3; ++p)
			for (int q = p + 1; q < 3; ++q)
				if (ranges_overlap(buf[p], bytes[p], buf[q], bytes[q])) throw Error{SPSAMD_EINVAL, op->overlap};
		const void *arr[3] = {view.coo.idx0, view.coo.idx1, view.coo.val};
		for (int p = 0; p < 3; ++p)
			for (int k = 0; k < 3; ++k)
				if (ranges_overlap(buf[p], bytes[p], arr[k], n * (k == 2 ? 8 : 4))) throw Error{SPSAMD_EINVAL, "an output buffer overlaps A's arrays"};
		if (mem == SPSAMD_MEM_DEVICE)
			for (int p = 0; p < 3; ++p)
				if (in_output_sets(c, buf[p], bytes[p])) throw Error{SPSAMD_EINVAL, "an output buffer lies in an output set of the context"};
	}
	std::memset(res, 0, sizeof(*res));
	if (stats) std::memset(stats, 0, stats_bytes);
	res->shape0 = res->shape1 = N;

	SPS_HIP(hipSetDevice(c->device));
	c->arena.reset();
	hipStream_t st = c->stream;
	SPS_HIP(hipEventRecord(c->ev[EV_BEGIN], st));
	mask_keys(c, A, lead, N, N, &K);
	SPS_HIP(hipEventRecord(c->ev[EV_CONSOLIDATED], st));
	res->nnz_a = K.n;
	*out_count = 0;
	if (N == 0) {                                                      // no vertex, nothing to count: ptr_out is the one entry 0
		*rc = fits(0) ? SPSAMD_OK : SPSAMD_ECAPACITY;
		if (*rc != SPSAMD_OK || !ptr_out) return false;
		if (mem == SPSAMD_MEM_HOST) ptr_out[0] = 0;
		else { fill_zero(c, ptr_out, sizeof(int32_t)); SPS_HIP(hipStreamSynchronize(st)); }
		return false;
	}
	g = graph_adjacency(c, K, N, symmetric);
	const int kp = c->tune.*op->path, kr = c->tune.*op->row, kf = c->tune.*op->fuse_rows, kw = c->tune.*op->wave_deg;
	path = kp == 1 || kp == 2 ? kp : 0;
	rowk = kr == 1 || kr == 2 ? kr : 0;
	fuse_rows = kf > 0 ? (uint32_t)kf : op->fuse_rows_default;
	wave_deg = kw > 0 ? (uint32_t)kw : op->wave_deg_default;
	acc = get_zeroed<unsigned long long>(c, op->acc_len);
	ctr = get_zeroed<uint32_t>(c, 2 * op->nlists);
	deg = c->arena.get<uint32_t>(N);
	ids = c->arena.get<int32_t>(N);
	h = (uint32_t *)c->host_staging(op->acc_len * sizeof(unsigned long long));
	return true;
}

void GraphCall::read_counts(int par, uint32_t *cnt)
{
	SPS_HIP(hipMemcpyAsync(h, ctr + op->nlists * par, op->nlists * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	SPS_HIP(hipStreamSynchronize(c->stream));
	std::memcpy(cnt, h, op->nlists * sizeof(uint32_t));
}

bool GraphCall::fits(uint64_t count)
{
	*out_count = count;
	if (!ptr_out || ptr_capacity >= count + 1) return true;
	c->last_error = op->too_small;
	return false;
}

GraphTotals GraphCall::close(const unsigned long long *hacc, int fused_slot)
{
	finish_call(c, res);
	SPS_HIP(hipEventElapsedTime(&res->ms_consolidate, c->ev[EV_BEGIN], c->ev[EV_CONSOLIDATED]));
	SPS_HIP(hipEventElapsedTime(&res->ms_symbolic, c->ev[EV_CONSOLIDATED], c->ev[EV_SYMBOLIC]));
	SPS_HIP(hipEventElapsedTime(&res->ms_numeric, c->ev[EV_SYMBOLIC], c->ev[EV_END]));
	return GraphTotals{hacc[GRAPH_ADJ], hacc[GRAPH_MAXDEG], launches, fused ? hacc[fused_slot] : 0, hacc[GRAPH_ROWS_W], res->ms_symbolic};
}

static const GraphOp COL_OP = {"unknown colouring order", "unknown color_flags", "op(A) must be square for a colouring",
	"color, perm and color_ptr overlap", "color_ptr is too small: it needs one entry per colour and one more; *out_ncolors holds the colours",
	&Tuning::color_path, &Tuning::color_row, &Tuning::color_fuse_rows, &Tuning::color_wave_deg, COL_FUSE_ROWS, COL_WAVE_DEG, COL_ACC, 2};

int color_graph(spsamd_ctx *c, const spsamd_coo *A, char transpose, int order, uint32_t seed, int color_flags, int32_t *color,
	int32_t *perm, int32_t *color_ptr, size_t ptr_capacity, int mem, size_t *out_ncolors, spsamd_color_stats *stats,
	spsamd_result *res)
{
	GraphCall gc{c, &COL_OP, color, perm, color_ptr, ptr_capacity, out_ncolors, res};
	int rc;
	if (!gc.open(A, transpose, order, color_flags, mem, stats, sizeof(*stats), &rc)) return rc;
	hipStream_t st = c->stream;
	const uint64_t N = gc.N; const MaskKeys &K = gc.K;
	int32_t *col = gc.ids, *pending = c->arena.get<int32_t>(N);
	uint32_t *wait = get_zeroed<uint32_t>(c, N);
	uint32_t *list_t[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)};
	uint32_t *list_w[2] = {c->arena.get<uint32_t>(N), c->arena.get<uint32_t>(N)};
	graph_classes(c, gc.g, N, gc.deg, col, list_t[0], list_w[0], gc.ctr, gc.acc, gc.wave_deg, gc.rowk, gc.symmetric);
	SPS_HIP(hipEventRecord(c->ev[EV_SYMBOLIC], st));
	uint32_t cnt0[2];
	gc.read_counts(0, cnt0);

	// ---- sweep
	ColArgs a;
	a.ptr = gc.g.ptr; a.adj = gc.g.adj; a.deg = gc.deg; a.color = col; a.pending = pending; a.wait = wait; a.acc = gc.acc; a.seed = seed;
	a.by_degree = order == SPSAMD_COLOR_ORDER_DEGREE; a.directed = gc.symmetric;
	gc.sweep(cnt0,
		[&](int par, const uint32_t *cnt) {
			uint64_t launches = 0;                                     // (the commit is not counted: it is the round's bookkeeping)
			if (cnt[0]) { k_col_thread<<<dim3(grid_for(cnt[0])), dim3(256), 0, st>>>(a, list_t[par], cnt[0]); SPS_LAUNCH_CHECK(); ++launches; }
			if (cnt[1]) { k_col_wave<<<dim3(grid_for(cnt[1], 4)), dim3(256), 0, st>>>(a, list_w[par], cnt[1]); SPS_LAUNCH_CHECK(); ++launches; }
			k_col_commit<<<dim3(grid_for((size_t)cnt[0] + cnt[1])), dim3(256), 0, st>>>(a, list_t[par], cnt[0], list_w[par], cnt[1],
				list_t[par ^ 1], list_w[par ^ 1], gc.ctr + 2 * (par ^ 1), gc.ctr + 2 * par);
			SPS_LAUNCH_CHECK();
			return launches;
		},
		[&](int par, const uint32_t *cnt) {
			k_col_fused<<<dim3(1), dim3(COL_NT), 0, st>>>(a, list_t[par], list_t[par ^ 1], cnt[0], list_w[par], list_w[par ^ 1], cnt[1]);
			SPS_LAUNCH_CHECK();
		});
	if (K.n) { k_col_conflicts<<<dim3(grid_for(K.n)), dim3(256), 0, st>>>(K.i, K.j, K.n, col, gc.acc); SPS_LAUNCH_CHECK(); }
	unsigned long long hacc[COL_ACC];
	SPS_HIP(hipMemcpyAsync(gc.h, gc.acc, sizeof hacc, hipMemcpyDeviceToHost, st));
	SPS_HIP(hipStreamSynchronize(st));
	std::memcpy(hacc, gc.h, sizeof hacc);
	const uint64_t ncolors = std::max<uint64_t>(hacc[COL_NCOLORS], 1);  // (the isolated vertices hold colour 0 ...)
	if (!gc.fits(ncolors)) return SPSAMD_ECAPACITY;

	// ---- perm, color_ptr and delivery
	if (perm || color_ptr) {
		PairSort sort(c, N);
		k_col_keys<<<dim3(grid_for(N)), dim3(256), 0, st>>>(col, N, sort.keys);
		SPS_LAUNCH_CHECK();
		order_by_key(c, sort, N, bits_of(ncolors), 0, ncolors, color_ptr != nullptr, perm, color_ptr, gc.kind);   // stable: ascending index inside a colour
	}
	gc.deliver();
	const GraphTotals t = gc.close(hacc, COL_FUSED);
	if (stats) {
		stats->ncolors = ncolors; stats->rounds = std::max<uint64_t>(gc.rounds + t.fused_rounds, 1);   // (... and are round 0)
		stats->adjacency = t.adjacency; stats->max_degree = t.max_degree; stats->conflicts = hacc[COL_CONFLICTS];
		stats->launches = t.launches; stats->fused_rounds = t.fused_rounds;
		stats->rows_thread = hacc[GRAPH_ROWS_T]; stats->rows_wave = t.rows_wave;
		stats->ms_adjacency = t.ms_adjacency; stats->ms_color = res->ms_numeric;
	}
	return SPSAMD_OK;
}

} // namespace spsamd
