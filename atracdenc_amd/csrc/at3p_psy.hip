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

// M1-M3 on the host: the offsets from D's first column. D [2][32][8], live from dist.
static void host_psy_offsets(const double (&D)[2][32][8], const uint64_t* dist, int channels, int (&o)[2][32])
{
    int mu[2][32] = {}, mu_min = kPsyMuHi + 1;
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            double th = rd_lambda(AT3P_PSY_ATH[qu], AT3P_SCALE);
            for (int m = 0; m < 32; ++m) {
                const int s = AT3P_PSY_SPREAD[m][qu];
                if (s > 63) continue;
                const double cast = D[ch][m][0] * rd_g(AT3P_SCALE[63 - s]);
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

// M1-M6 on the host. dist: S [channels][32][8]; offsets_in: null, or the offsets to use. Returns Bits of the allocation written.
static int host_allocate_psy(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const uint8_t* offsets_in, int channels, int tail_bits,
                             int size_bits, uint8_t* wl_out, int* n_units, int* j_out, int* k_out, int* chose_psy, uint8_t* offsets_out)
{
    double D[2][32][8] = {};
    uint16_t B[2][32][8] = {};
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu)
            for (int w = 0; w < 8; ++w) {
                D[ch][qu][w] = rd_d(dist[(ch * 32 + qu) * 8 + w], rd_g(AT3P_SCALE[sfi[ch * 32 + qu]]));
                B[ch][qu][w] = w ? bits[(ch * 32 + qu) * 8 + w] : 0;   // (entry 0 is not read)
            }
    int o[2][32] = {}, O = 0;
    if (offsets_in) {
        for (int ch = 0; ch < channels; ++ch)
            for (int qu = 0; qu < 32; ++qu) o[ch][qu] = offsets_in[ch * 32 + qu];
    } else {
        host_psy_offsets(D, dist, channels, o);
    }
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            if (o[ch][qu] > O) O = o[ch][qu];
            if (offsets_out) offsets_out[ch * 32 + qu] = (uint8_t)o[ch][qu];
        }
    int wl[2][32] = {};
    int N = 1, took = 0;
    auto form = [&](int j, int k) {   // P(j, k) into wl and N; took: the units that took the j - 1 value
        int top = -1;
        took = 0;
        for (int qu = 0, left = k; qu < 32; ++qu)
            for (int ch = 0; ch < channels; ++ch) {
                const int w0 = rd_pick(D[ch][qu], B[ch][qu], rd_lambda(j + o[ch][qu], AT3P_SCALE));
                const int up = rd_pick(D[ch][qu], B[ch][qu], rd_lambda(j - 1 + o[ch][qu], AT3P_SCALE));
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
    for (int j = kRdJMax; j >= kRdJMin - O; --j) {   // M5: every j, the smallest that fits
        form(j, 0);
        if (count() <= size_bits) js = j;
    }
    if (js > kRdJMax) js = kRdJMax;                   // nothing fits (a caller's table only)
    for (int k = 0; k <= kAllocKMax; ++k) {           // every k: the largest that fits
        form(js, k);
        if (count() <= size_bits) ks = k;
    }
    form(js, ks);
    // M6: against the sparse allocation A(t*, k*)
    uint8_t wl_a[64] = {};
    int n_a = 0, t_a = 0, k_a = 0;
    const int bits_a = host_allocate(sfi, bits, channels, tail_bits, size_bits, wl_a, &n_a, &t_a, &k_a, true);
    double sum_p = 0.0, sum_a = 0.0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const double g = rd_g(AT3P_SCALE[63 - o[ch][qu]]);
            sum_p += D[ch][qu][wl[ch][qu]] * g;
            sum_a += D[ch][qu][wl_a[ch * 32 + qu]] * g;
        }
    *j_out = js;
    *k_out = took;   // k* as reported (A5)
    *chose_psy = sum_p <= sum_a;
    if (*chose_psy) {
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

extern "C" int at3phip_host_allocate_psy(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const uint8_t* offsets_in, int32_t channels,
                                         int32_t tail_bits, int32_t frame_bytes, uint8_t* wl_out, int32_t* n_units, int32_t* j, int32_t* k,
                                         int32_t* chose_psy, uint8_t* offsets_out)
{
    if (!dist || !chose_psy) return AT3HIP_EINVAL;
    if (const int rc = at3p::host_allocate_args(sfi, bits, channels, tail_bits, frame_bytes, wl_out, n_units, j, k)) return rc;
    for (int i = 0; i < 256 * channels; ++i)
        if (dist[i] > (1ull << 47)) return AT3HIP_EINVAL;   // 128 lines of at most 2^40 each
    if (offsets_in)
        for (int i = 0; i < 32 * channels; ++i)
            if (offsets_in[i] > at3p::kPsyMaxOffset) return AT3HIP_EINVAL;
    int n = 0, js = 0, ks = 0, psy = 0;
    at3p::host_allocate_psy(sfi, bits, dist, offsets_in, channels, tail_bits, 8 * frame_bytes - 3, wl_out, &n, &js, &ks, &psy, offsets_out);
    *n_units = n;
    *j = js;
    *k = ks;
    *chose_psy = psy;
    return AT3HIP_OK;
}
