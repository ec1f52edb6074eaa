// The adaptive ATRAC3plus frame writer's kernels (at3p_alloc.hpp) and at3phip_host_allocate (include/at3phip.h, ADAPTIVE WORD
// LENGTHS). A translation unit of its own: the kernels share device functions with the fixed writer's, and compiled next to them
// they change the code the compiler makes for those.
#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_alloc.hpp"

namespace at3p {

// The two unflagged instantiations by name, without records first and ahead of the launch: this fixes the order in which they are
// instantiated, which the unit's device code depends on (the launch template alone names the one with records first). at3p_sparse.hip
// and at3p_rd.hip name theirs in the same way.
constexpr auto k_at3p_write_adaptive = k_at3p_write_adaptive_with<WriteParams>;
constexpr auto k_at3p_write_adaptive_tonal = k_at3p_write_adaptive_with<WriteParamsTonal>;

__attribute__((visibility("default"))) void launch_write_adaptive(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    launch_write_adaptive_as<WriteParams, WriteParamsTonal>(wp, frame_bytes, on);
}

}  // namespace at3p

extern "C" int at3phip_host_allocate_sized(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes,
                                           uint8_t* wl_out, int32_t* n_units, int32_t* t, int32_t* k)
{
    return at3p::host_allocate_checked(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, t, k, false);
}

extern "C" int at3phip_host_allocate(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, uint8_t* wl_out, int32_t* n_units,
                                     int32_t* t, int32_t* k)
{
    return at3phip_host_allocate_sized(sfi, bits, channels, tail_bits, AT3PHIP_FRAME_BYTES, wl_out, n_units, t, k);
}
