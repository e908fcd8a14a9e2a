// krylov_dev.h -- what the device loops of k_krylov.hip (conjugate gradients) and k_bicgstab.hip (BiCGStab) share: the state
// word and the scalars of a loop in device memory, and the one reduction shape of every dot product (the fold of
// include/spsparse_amd.h).  Device code only; included after devutil.h and x86fp.h.
#pragma once

#include "internal.h"
#include "devutil.h"
#include "x86fp.h"

namespace spsamd {

constexpr int PCG_CHUNK = 1024;                // elements of a level-0 chunk: 16 per lane of one wave
constexpr int PCG_NT = 256;                    // four waves, a chunk each
constexpr int PCG_FINISH_NT = 1024;            // the one workgroup of a finish kernel
constexpr int32_t PCG_RUNNING = -1;            // PcgState::state; from 0 on: SPSAMD_PCG_*

struct PcgState {
	double bb, thresh, rr0, rr, rz, pq, alpha, beta;
	unsigned long long k, max_iter, hist_cap;
	int32_t state, pad;
};

__device__ __forceinline__ bool pcg_usable(double v) { return v == v && mag_of(v) != 0x7FF0000000000000ull && v != 0.0; }

// The partial of chunk g of t[0 .. n), t[e] = term(e) (called once per element of the chunk, by the lane that owns it):
// valid in lane 0.  Every lane of the wave calls it.
template <class Term>
__device__ __forceinline__ double chunk_partial(uint64_t g, uint64_t n, Term term)
{
	const uint64_t base = g * PCG_CHUNK + lane_id();
	double t[PCG_CHUNK / 64];
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k) {
		const uint64_t e = base + (uint64_t)k * 64;
		t[k] = e < n ? term(e) : 0.0;
	}
	double a = 0.0;
#pragma unroll
	for (int k = 0; k < PCG_CHUNK / 64; ++k)
		if (base + (uint64_t)k * 64 < n) a = ref_add(a, t[k]);
#pragma unroll
	for (int s = 32; s >= 1; s >>= 1) {
		const double o = __shfl_down(a, s, 64);
		if (lane_id() < (unsigned)s) a = ref_add(a, o);              // a_l is the left operand
	}
	return a;
}

// the chunk of this wave, or false past the last one
__device__ __forceinline__ bool my_chunk(uint64_t n, uint64_t *g)
{
	*g = (uint64_t)blockIdx.x * (PCG_NT / 64) + wave_id();
	return *g * PCG_CHUNK < n;
}

__device__ __forceinline__ bool stopped(const PcgState *st) { return st && st->state != PCG_RUNNING; }

// fold(part, c0) for c0 >= 2 by the whole workgroup: a wave per chunk, a barrier between two levels; b0 / b1 take the
// levels' partials in turn (ceil(c0 / 1024) entries each).  The value comes back in every thread.
__device__ inline double block_fold(const double *part, uint64_t m, double *b0, double *b1, double *s_out)
{
	const double *src = part;
	double *dst = b0;
	for (;;) {                                                       // uniform
		const uint64_t c = (m + PCG_CHUNK - 1) / PCG_CHUNK;
		for (uint64_t g = wave_id(); g < c; g += PCG_FINISH_NT / 64) {
			const double a = chunk_partial(g, m, [&](uint64_t e) { return src[e]; });
			if (lane_id() == 0) { if (c == 1) *s_out = a; else dst[g] = a; }
		}
		__syncthreads();                                             // this level's partials are complete, and visible to the workgroup
		if (c == 1) break;
		src = dst; dst = dst == b0 ? b1 : b0; m = c;
	}
	return *s_out;
}

} // namespace spsamd
