// The adaptive ATRAC3plus frame writer's kernels (at3p_alloc.hpp) and at3phip_host_allocate (include/at3phip.h, ADAPTIVE WORD
// LENGTHS). A translation unit of its own: the kernels share device functions with the fixed writer's, and compiled next to them
// they change the code the compiler makes for those.
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_alloc.hpp"

namespace at3p {

namespace {
#include "at3p_tone_vlc.inc"
}

// the two unflagged instantiations under the names they are launched by
constexpr auto k_at3p_write_adaptive = k_at3p_write_adaptive_with<WriteParams>;
constexpr auto k_at3p_write_adaptive_tonal = k_at3p_write_adaptive_with<WriteParamsTonal>;

// wp: the fixed writer's parameters as at3phip.hip's launch_write fills them; wp.tonal null: the writer without records. The
// word-length code tables and the frame size travel in the kernel's arguments: nothing is allocated or uploaded for the adaptive
// path. wp.out is [n_items][frame_bytes].
__attribute__((visibility("default"))) void launch_write_adaptive(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    if (wp.tonal) {
        AdaptiveParams<WriteParamsTonal> ap;
        static_cast<WriteParamsTonal&>(ap) = wp;
        memcpy(ap.tone_vlc, AT3P_TONE_BANDS_VLC, sizeof(ap.tone_vlc));
        memcpy(ap.wl_vlc, AT3P_WL_VLC, sizeof(ap.wl_vlc));
        ap.frame_bytes = frame_bytes;
        hipLaunchKernelGGL(k_at3p_write_adaptive_tonal, dim3((unsigned)wp.n_items), dim3(256), 0, on, ap);
    } else {
        AdaptiveParams<WriteParams> ap;
        static_cast<WriteParams&>(ap) = static_cast<const WriteParams&>(wp);
        memcpy(ap.wl_vlc, AT3P_WL_VLC, sizeof(ap.wl_vlc));
        ap.frame_bytes = frame_bytes;
        hipLaunchKernelGGL(k_at3p_write_adaptive, dim3((unsigned)wp.n_items), dim3(256), 0, on, ap);
    }
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
