// MASKING-WEIGHTED WORD LENGTHS (include/at3phip.h, M1-M7): what the host function at3phip_host_allocate_psy and the two kernels
// k_at3p_write_adaptive_with<WriteParamsPsy>, <WriteParamsTonalPsy> (at3p_alloc.hpp; instantiated in at3p_psy.hip) share. As in
// at3p_rd.hpp everything is integer arithmetic or single double operations rounded once: no libm, nothing to contract.
#pragma once
#include <cstdint>

#include "at3p_rd.hpp"

namespace at3p {

// M2, M3: the highest threshold index and the largest offset
constexpr int kPsyMuHi = 73, kPsyMaxOffset = 32;

#include "at3p_psy.inc"

// the parameter types of the masking-weighted instantiations: the rate-distortion ones with the two tables of M2 in the kernel's
// arguments (1056 bytes; the kernel copies them to LDS, where each lane indexes them on its own)
struct PsyTables {
    alignas(4) uint8_t spread[32][32];
    alignas(4) uint8_t ath[32];
};
struct WriteParamsPsy : WriteParamsRd { PsyTables psy; };
struct WriteParamsTonalPsy : WriteParamsTonalRd { PsyTables psy; };
template <> struct alloc_is_rd<WriteParamsPsy> { static constexpr bool value = true; };
template <> struct alloc_is_rd<WriteParamsTonalPsy> { static constexpr bool value = true; };
template <typename P> struct alloc_is_psy { static constexpr bool value = false; };
template <> struct alloc_is_psy<WriteParamsPsy> { static constexpr bool value = true; };
template <> struct alloc_is_psy<WriteParamsTonalPsy> { static constexpr bool value = true; };

// M2: the largest i in 0..kPsyMuHi with lambda_i <= th, for th >= lambda_0. lambda_i rises with i (G[0] < G[1] < G[2] < 4 G[0]), so
// the bisection finds what the definition's walk finds. scale: ScaleTable's first three entries.
__host__ __device__ inline int psy_mu(double th, const float* scale)
{
    int lo = 0, hi = kPsyMuHi;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rd_lambda(mid, scale) <= th) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace at3p
