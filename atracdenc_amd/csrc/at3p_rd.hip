// RATE-DISTORTION WORD LENGTHS (include/at3phip.h): the rate-distortion instantiations of the adaptive ATRAC3plus writer
// (at3p_alloc.hpp, at3p_rd.hpp), their launch, and at3phip_host_allocate_rd. A translation unit of its own for the reason
// at3p_sparse.hip is one: the instantiations share device functions with the other four writer kernels, and compiled next to them
// they change the code the compiler makes for those. at3phip.hip finds the launch as a weak symbol; a build without this file
// refuses AT3PHIP_ALLOC_RD and has no at3phip_host_allocate_rd, the symbol by which a host detects the flag.
#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_alloc.hpp"
#include "at3p_rd.hpp"

namespace at3p {

constexpr auto k_at3p_write_adaptive_rd = k_at3p_write_adaptive_with<WriteParamsRd>;
constexpr auto k_at3p_write_adaptive_tonal_rd = k_at3p_write_adaptive_with<WriteParamsTonalRd>;

__attribute__((visibility("default"))) void launch_write_adaptive_rd(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    launch_write_adaptive_as<WriteParamsRd, WriteParamsTonalRd>(wp, frame_bytes, on);
}

}  // namespace at3p

extern "C" int at3phip_host_allocate_rd(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int32_t channels, int32_t tail_bits,
                                        int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k, int32_t* chose_rd)
{
    if (const int rc = at3p::host_allocate_rd_args(sfi, bits, dist, channels, tail_bits, frame_bytes, wl_out, n_units, j, k, chose_rd)) return rc;
    int n = 0, js = 0, ks = 0, rd = 0;
    at3p::host_allocate_rd(sfi, bits, dist, nullptr, channels, tail_bits, 8 * frame_bytes - 3, wl_out, &n, &js, &ks, &rd);
    *n_units = n;
    *j = js;
    *k = ks;
    *chose_rd = rd;
    return AT3HIP_OK;
}
