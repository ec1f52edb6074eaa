// SPARSE WORD LENGTHS (include/at3phip.h): the sparse instantiations of the adaptive ATRAC3plus writer (at3p_alloc.hpp) and of the
// decoder's unpack kernel (at3p_decode.hpp), their launches, and at3phip_host_allocate_sparse. A translation unit of its own for the
// reason at3p_alloc.hip is one: the instantiations share device functions with the unflagged kernels, and compiled next to them they
// change the code the compiler makes for those. at3phip.hip finds the launches as weak symbols; a build without this file refuses
// AT3PHIP_ALLOC_SPARSE and AT3PHIP_DECODE_SPARSE.
#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_alloc.hpp"
#include "at3p_tables.hpp"
#define AT3P_DECODE_UNPACK_ONLY
#include "at3p_decode.hpp"

namespace at3p {

constexpr auto k_at3p_write_adaptive_sparse = k_at3p_write_adaptive_with<WriteParamsSparse>;
constexpr auto k_at3p_write_adaptive_tonal_sparse = k_at3p_write_adaptive_with<WriteParamsTonalSparse>;
constexpr auto k_at3pd_unpack_sparse = k_at3pd_unpack_sparse_with<false>;
constexpr auto k_at3pd_unpack_sparse_sized = k_at3pd_unpack_sparse_with<true>;

__attribute__((visibility("default"))) void launch_write_adaptive_sparse(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    launch_write_adaptive_as<WriteParamsSparse, WriteParamsTonalSparse>(wp, frame_bytes, on);
}

__attribute__((visibility("default"))) void launch_unpack_sparse(const DecUnpackParams& up, bool sized, dim3 grid, hipStream_t on)
{
    if (sized) hipLaunchKernelGGL(k_at3pd_unpack_sparse_sized, grid, dim3(kDecUnpackThreads), 0, on, up);
    else hipLaunchKernelGGL(k_at3pd_unpack_sparse, grid, dim3(kDecUnpackThreads), 0, on, up);
}

}  // namespace at3p

extern "C" int at3phip_host_allocate_sparse(const uint8_t* sfi, const uint16_t* bits, int32_t channels, int32_t tail_bits, int32_t frame_bytes,
                                            uint8_t* wl_out, int32_t* n_units, int32_t* t, int32_t* k)
{
    return at3p::host_allocate_checked(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, t, k, true);
}
