// x86fp.h -- double arithmetic whose NaN results carry the bits x86-64 SSE gives them (the reference's build).
// The GPU returns its own default NaN; an x86-64 mulsd / addsd returns the left operand's NaN, quieted, if it is one,
// else the right operand's, else the default NaN 0xFFF8000000000000 (0 * Inf, Inf - Inf).  Used by multiply_dense
// (k_spmm.hip) and add (k_add.hip); DESIGN.md §9.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spsamd {

constexpr uint64_t X86_DEFAULT_NAN = 0xFFF8000000000000ull;

__device__ __forceinline__ double quiet(double a)
{
	return __longlong_as_double(__double_as_longlong(a) | 0x0008000000000000ll);
}

// The NaN an x86-64 SSE mulsd / addsd returns for operands (a, b) when its result is a NaN.
__device__ __forceinline__ double x86_nan(double a, double b)
{
	return a != a ? quiet(a) : b != b ? quiet(b) : __longlong_as_double((long long)X86_DEFAULT_NAN);
}

__device__ __forceinline__ double ref_mul(double a, double b)
{
	double r = a * b;
	return r != r ? x86_nan(a, b) : r;
}

__device__ __forceinline__ double ref_add(double a, double b)
{
	double r = a + b;
	return r != r ? x86_nan(a, b) : r;
}

// subsd: a - b, never a + (-b) -- the negation would flip the sign bit of a NaN b that the result then carries
__device__ __forceinline__ double ref_sub(double a, double b)
{
	double r = a - b;
	return r != r ? x86_nan(a, b) : r;
}

// divsd: a true IEEE division (0 / 0 and Inf / Inf give the default NaN)
__device__ __forceinline__ double ref_div(double a, double b)
{
	double r = __ddiv_rn(a, b);
	return r != r ? x86_nan(a, b) : r;
}

// sqrtsd: the correctly rounded square root (a NaN operand quieted; a < 0: the default NaN; sqrt(-0.0) = -0.0)
__device__ __forceinline__ double ref_sqrt(double a)
{
	if (a != a) return quiet(a);
	if (a < 0.0) return __longlong_as_double((long long)X86_DEFAULT_NAN);
	return __dsqrt_rn(a);
}

} // namespace spsamd
