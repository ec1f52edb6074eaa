// Input PCM of the kernels that first touch a call's samples, as float32 or as 16-bit integers (the *_short / *_s16 entry
// points of include/). A 16-bit sample s becomes (float)s * 0x1p-15f, which is exact and equals s / 32768.0f: the rule of
// at3hip_encode_s16. The 16-bit form widens in the load: no float copy of the input is written to memory.
//
// A row of 16-bit samples that starts 4-byte aligned is read as 32-bit sample pairs (one dword per load, the wanted half
// selected afterwards); the last sample of a row of odd length, and every sample of a row that is only 2-byte aligned (a mono
// stream behind an odd number of samples, a caller's pointer with int16_t alignment), is read on its own, so that no load
// reaches past the row.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace at3 {

// may `row` be read as 32-bit pairs? (wave-uniform wherever the row is)
__device__ __forceinline__ bool pcm_pairs(const float*) { return false; }
__device__ __forceinline__ bool pcm_pairs(const int16_t* row) { return ((uintptr_t)row & 3u) == 0; }

// sample i of a row of n samples
__device__ __forceinline__ float pcm_at(const float* row, size_t i, size_t, bool) { return row[i]; }
__device__ __forceinline__ float pcm_at(const int16_t* row, size_t i, size_t n, bool pairs)
{
    int v;
    if (pairs && (i | 1) < n) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(row)[i >> 1];
        v = (int16_t)((i & 1) ? (w >> 16) : (w & 0xffffu));
    } else {
        v = row[i];
    }
    return (float)v * 0x1p-15f;
}

}  // namespace at3
