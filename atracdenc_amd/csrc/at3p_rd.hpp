// RATE-DISTORTION WORD LENGTHS (include/at3phip.h, R1-R5): what the host function at3phip_host_allocate_rd and the two kernels
// k_at3p_write_adaptive_with<WriteParamsRd>, <WriteParamsTonalRd> (at3p_alloc.hpp; instantiated in at3p_rd.hip) share. Everything
// here is integer arithmetic or single double operations that are exact or rounded once: no libm, nothing to contract.
#pragma once
#include <cstdint>

#include "at3p_write.hpp"

namespace at3p {

// R3: the scan's range. kRdJMax: the smallest j at which every unit picks 0 whatever its spectrum and its costs (the header derives
// it); kRdJMin: below it lambda no longer decides a pick on any of the project's signals. 100 values: 25 per wavefront.
constexpr int kRdJMin = -30, kRdJMax = 69, kRdJCount = kRdJMax - kRdJMin + 1;
static_assert(kRdJCount % 4 == 0, "the four wavefronts share the scan evenly");

// the parameter types of the rate-distortion instantiations: the fixed writer's, marked (as WriteParamsSparse in at3p_alloc.hpp),
// with atrac3p_mant_tab, which the writers' tables hold only inverted, in the kernel's arguments
#include "at3p_mant.inc"
struct WriteParamsRd : WriteParams { float mant[8]; };
struct WriteParamsTonalRd : WriteParamsTonal { float mant[8]; };
template <typename P> struct alloc_is_rd { static constexpr bool value = false; };
template <> struct alloc_is_rd<WriteParamsRd> { static constexpr bool value = true; };
template <> struct alloc_is_rd<WriteParamsTonalRd> { static constexpr bool value = true; };

__host__ __device__ inline double rd_pow2(int n) { return __builtin_bit_cast(double, (uint64_t)(1023 + n) << 52); }   // -1022 <= n <= 1023

// R1: one line's squared error at 2^-40, truncated, as (uint64)(d * 0x1p40f) gives it; d: the float square, below 1 (|v| < 1 and the
// mantissa's value lies within half a step of it). A float-to-64-bit conversion expands to a sequence with an FMA in it, so the
// product t < 2^40 is split into two exact 32-bit conversions: t * 2^-16 truncates to hi < 2^24, and t - hi * 2^16 = t mod 2^16 is
// a multiple of t's last place below 2^16, so the subtraction is exact.
__host__ __device__ inline uint64_t rd_dist_u(float d)
{
    if (!(d == d)) return 0;   // NaN (R5)
    const float t = d * 0x1p40f;
    const uint32_t hi = (uint32_t)(t * 0x1p-16f);
    const uint32_t lo = (uint32_t)(t - (float)hi * 0x1p16f);
    return ((uint64_t)hi << 16) + lo;
}

// G[i] and D = (double)S * G[sfi]: S < 2^50, so both halves convert exactly and their sum is exact
__host__ __device__ inline double rd_g(float scale) { return (double)scale * (double)scale; }
__host__ __device__ inline double rd_d(uint64_t S, double g) { return ((double)(uint32_t)(S >> 32) * 0x1p32 + (double)(uint32_t)S) * g; }

// R2: lambda_j = 2^40 G[j mod 3] 4^floor(j / 3); scale: ScaleTable's first three entries
__host__ __device__ inline double rd_lambda(int j, const float* scale)
{
    const int q = j >= 0 ? j / 3 : -((2 - j) / 3), r = j - 3 * q;
    return rd_g(scale[r]) * rd_pow2(40 + 2 * q);
}

// R2: pick - the w in 0..7 with the smallest D[w] + lambda * (B[w] + (w > 0 ? 3 : 0)), the smaller w on a tie; B[0] counts as 0
__host__ __device__ inline int rd_pick(const double* D, const uint16_t* B, double lambda)
{
    int best = 0;
    double least = D[0];
    for (int w = 1; w < 8; ++w) {
        const double rate = lambda * (double)((int)B[w] + 3);
        const double cost = D[w] + rate;
        if (cost < least) {
            least = cost;
            best = w;
        }
    }
    return best;
}

}  // namespace at3p
