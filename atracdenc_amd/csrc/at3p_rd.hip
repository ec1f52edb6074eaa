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

// R2-R4 on the host. dist: S [channels][32][8]. Returns Bits of the allocation written.
static int host_allocate_rd(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int channels, int tail_bits, int size_bits, uint8_t* wl_out,
                            int* n_units, int* j_out, int* k_out, int* chose_rd)
{
    double D[2][32][8] = {};
    uint16_t B[2][32][8] = {};
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu)
            for (int w = 0; w < 8; ++w) {
                D[ch][qu][w] = rd_d(dist[(ch * 32 + qu) * 8 + w], rd_g(AT3P_SCALE[sfi[ch * 32 + qu]]));
                B[ch][qu][w] = w ? bits[(ch * 32 + qu) * 8 + w] : 0;   // (entry 0 is not read)
            }
    int wl[2][32] = {};
    int N = 1, took = 0;
    auto form = [&](int j, int k) {   // R(j, k) into wl and N; took: the units that took the j - 1 value
        const double lam = rd_lambda(j, AT3P_SCALE), lam_up = rd_lambda(j - 1, AT3P_SCALE);
        int top = -1;
        took = 0;
        for (int qu = 0, left = k; qu < 32; ++qu)
            for (int ch = 0; ch < channels; ++ch) {
                const int w0 = rd_pick(D[ch][qu], B[ch][qu], lam), up = rd_pick(D[ch][qu], B[ch][qu], lam_up);
                wl[ch][qu] = w0;
                if (left > 0 && up > w0) {
                    wl[ch][qu] = up;
                    --left;
                    ++took;
                }
                if (wl[ch][qu]) top = qu;
            }
        N = host_sparse_close(wl, top);
    };
    auto count = [&]() { return host_alloc_bits(wl, N, bits, channels, tail_bits); };
    int js = kRdJMax + 1, ks = 0;
    for (int j = kRdJMax; j >= kRdJMin; --j) {   // every j: the smallest that fits
        form(j, 0);
        if (count() <= size_bits) js = j;
    }
    if (js > kRdJMax) js = kRdJMax;               // nothing fits (a caller's table only)
    for (int k = 0; k <= kAllocKMax; ++k) {       // every k: the largest that fits
        form(js, k);
        if (count() <= size_bits) ks = k;
    }
    form(js, ks);
    // R4: against the sparse allocation A(t*, k*)
    uint8_t wl_a[64] = {};
    int n_a = 0, t_a = 0, k_a = 0;
    const int bits_a = host_allocate(sfi, bits, channels, tail_bits, size_bits, wl_a, &n_a, &t_a, &k_a, true);
    double sum_r = 0.0, sum_a = 0.0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            sum_r += D[ch][qu][wl[ch][qu]];
            sum_a += D[ch][qu][wl_a[ch * 32 + qu]];
        }
    *j_out = js;
    *k_out = took;   // k* as reported (A5)
    *chose_rd = sum_r <= sum_a;
    if (*chose_rd) {
        for (int ch = 0; ch < channels; ++ch)
            for (int qu = 0; qu < 32; ++qu) wl_out[ch * 32 + qu] = (uint8_t)wl[ch][qu];
        *n_units = N;
        return count();
    }
    memcpy(wl_out, wl_a, (size_t)channels * 32);
    *n_units = n_a;
    return bits_a;
}

}  // namespace at3p

extern "C" int at3phip_host_allocate_rd(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int32_t channels, int32_t tail_bits,
                                        int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k, int32_t* chose_rd)
{
    if (!dist || !chose_rd) return AT3HIP_EINVAL;
    if (const int rc = at3p::host_allocate_args(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, j, k)) return rc;
    for (int i = 0; i < 256 * channels; ++i)
        if (dist[i] > (1ull << 47)) return AT3HIP_EINVAL;   // 128 lines of at most 2^40 each
    int n = 0, js = 0, ks = 0, rd = 0;
    at3p::host_allocate_rd(sfi, bits, dist, channels, tail_bits, 8 * frame_bytes - 3, wl_out, &n, &js, &ks, &rd);
    *n_units = n;
    *j = js;
    *k = ks;
    *chose_rd = rd;
    return AT3HIP_OK;
}
