// MASKING-WEIGHTED WORD LENGTHS (include/at3phip.h): the masking-weighted instantiations of the adaptive ATRAC3plus writer
// (at3p_alloc.hpp, at3p_psy.hpp), their launch, and at3phip_host_allocate_psy. A translation unit of its own for the reason
// at3p_rd.hip is one: compiled next to the other six writer kernels these two change the code the compiler makes for those.
// at3phip.hip finds the launch as a weak symbol; a build without this file refuses AT3PHIP_ALLOC_PSY and has no
// at3phip_host_allocate_psy, the symbol by which a host detects the flag.
#include <hip/hip_runtime.h>

#include "../../include/at3phip.h"
#include "at3p_alloc.hpp"
#include "at3p_psy.hpp"

namespace at3p {

constexpr auto k_at3p_write_adaptive_psy = k_at3p_write_adaptive_with<WriteParamsPsy>;
constexpr auto k_at3p_write_adaptive_tonal_psy = k_at3p_write_adaptive_with<WriteParamsTonalPsy>;

__attribute__((visibility("default"))) void launch_write_adaptive_psy(const WriteParamsTonal& wp, int32_t frame_bytes, hipStream_t on)
{
    launch_write_adaptive_as<WriteParamsPsy, WriteParamsTonalPsy>(wp, frame_bytes, on);
}

// M1-M3 on the host: the offsets from D's first column. dist: S [channels][32][8].
static void host_psy_offsets(const uint8_t* sfi, const uint64_t* dist, int channels, int (&o)[2][32])
{
    int mu[2][32] = {}, mu_min = kPsyMuHi + 1;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            double th = rd_lambda(AT3P_PSY_ATH[qu], AT3P_SCALE);
            for (int m = 0; m < 32; ++m) {
                const int s = AT3P_PSY_SPREAD[m][qu];
                if (s > 63) continue;
                const double cast = rd_d(dist[(ch * 32 + m) * 8], rd_g(AT3P_SCALE[sfi[ch * 32 + m]])) * rd_g(AT3P_SCALE[63 - s]);   // M1: D[ch][m][0]
                if (cast > th) th = cast;
            }
            mu[ch][qu] = psy_mu(th, AT3P_SCALE);
            if (dist[(ch * 32 + qu) * 8] > 0 && mu[ch][qu] < mu_min) mu_min = mu[ch][qu];
        }
    for (int ch = 0; ch < 2; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            const bool live = ch < channels && dist[(ch * 32 + qu) * 8] > 0;
            const int d = live ? mu[ch][qu] - mu_min : 0;
            o[ch][qu] = d < kPsyMaxOffset ? d : kPsyMaxOffset;
        }
}

}  // namespace at3p

extern "C" int at3phip_host_allocate_psy(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const uint8_t* offsets_in, int32_t channels,
                                         int32_t tail_bits, int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k,
                                         int32_t* chose_psy, uint8_t* offsets_out)
{
    if (const int rc = at3p::host_allocate_rd_args(sfi, bits, dist, channels, tail_bits, frame_bytes, wl_out, n_units, j, k, chose_psy)) return rc;
    int o[2][32] = {};
    if (offsets_in) {
        for (int i = 0; i < 32 * channels; ++i) {
            if (offsets_in[i] > at3p::kPsyMaxOffset) return AT3HIP_EINVAL;
            o[i >> 5][i & 31] = offsets_in[i];
        }
    } else {
        at3p::host_psy_offsets(sfi, dist, channels, o);
    }
    if (offsets_out)
        for (int i = 0; i < 32 * channels; ++i) offsets_out[i] = (uint8_t)o[i >> 5][i & 31];
    int n = 0, js = 0, ks = 0, psy = 0;
    at3p::host_allocate_rd(sfi, bits, dist, o, channels, tail_bits, 8 * frame_bytes - 3, wl_out, &n, &js, &ks, &psy);
    *n_units = n;
    *j = js;
    *k = ks;
    *chose_psy = psy;
    return AT3HIP_OK;
}
