// ff_atrac3p_generate_tones for one band, as the ATRAC3plus decoder's step 4b runs it (include/at3phip.h, TONAL BLOCKS) and as the
// tone analysis' step 8 subtracts it (FINDING TONES, G5): the envelope a record's band gets from its own points and the record
// before's, which regions are synthesised and Hann-windowed, and one sample of a region. One copy for k_at3pd_synth
// (at3p_decode.hpp) and k_at3p_tone_find / k_at3p_tone_sub (at3p_gha.hpp).
#pragma once
#include "at3_common.hpp"

namespace at3p {

// One band of a frame's tonal block. sp / ep are the envelope's start / stop point + 1, 0 when absent (pend_env's start_pos -1 /
// stop_pos 32), so that a zeroed record is a frame without a tonal block.
struct TonalBand {
    uint8_t nw, start_index, sp, ep;
};

struct DecpEnv {
    int hs, s, he, e;   // has_start_point, start_pos, has_stop_point, stop_pos
};

// curr_env of record k's band (nx) from its pend_env and record k-1's (nw), as ff_atrac3p_generate_tones reconstructs it
__device__ __forceinline__ DecpEnv decp_curr_env(TonalBand nx, TonalBand nw)
{
    const int nx_start = (int)nx.sp - 1, nx_stop = nx.ep ? (int)nx.ep - 1 : 32;
    DecpEnv r;
    if (nx.sp && nx_start < nx_stop) {
        r.hs = 1;
        r.s = nx_start + 32;
    } else if (nw.sp) {
        r.hs = 1;
        r.s = (int)nw.sp - 1;
    } else {
        r.hs = 0;
        r.s = 0;
    }
    if (nw.ep && (int)nw.ep - 1 >= r.s) {
        r.he = 1;
        r.e = (int)nw.ep - 1;
    } else if (nx.ep) {
        r.he = 1;
        r.e = nx_stop + 32;
    } else {
        r.he = 0;
        r.e = 64;
    }
    return r;
}

// What generate_tones does for one band: region 1 = record k-1's waves at reg_offset 128, region 2 = record k's at 0.
struct DecpToneJob {
    int active;          // the function runs for this band
    int n1, i1, n2, i2;  // waves synthesised (0 = the region stays zero) and the first wave's index
    int h1, h2;          // the Hann multiplies of the two regions
    DecpEnv e1, e2;
};

// nx, nw, pv: the band in records k, k-1, k-2; present: record k or k-1 has a tonal block
__device__ __forceinline__ DecpToneJob decp_tone_job(TonalBand nx, TonalBand nw, TonalBand pv, bool present)
{
    DecpToneJob j;
    j.active = present && (nx.nw || nw.nw);
    j.e2 = decp_curr_env(nx, nw);
    j.e1 = decp_curr_env(nw, pv);   // what the function stored for record k-1 when frame k-1 ran (it ran: nw.nw != 0)
    const int reg1 = j.e1.e < 32 ? 0 : 1, reg2 = j.e2.s >= 32 ? 0 : 1;
    j.n1 = nw.nw && reg1 ? nw.nw : 0;
    j.n2 = nx.nw && reg2 ? nx.nw : 0;
    j.i1 = nw.start_index;
    j.i2 = nx.start_index;
    if (nw.nw && nx.nw && reg1 && reg2) {
        j.h1 = 1;
        j.h2 = 1;
    } else {
        j.h1 = nw.nw && !j.e1.he;
        j.h2 = nx.nw && !j.e2.hs;
    }
    return j;
}

// waves_synth's sample i of a region: the waves in order, each out += sine_table[pos] * amp in double, then the envelope.
// Tables: anything with the decoder's sine[2048], hann[256] and amp_sf[64] (DecToneTables, ToneFindTables). kEnv = false: the
// caller knows that no record of the stream holds a point (the ungated tone analysis), and the envelope is not looked at.
template <bool kEnv = true, typename Tables>
__device__ __forceinline__ float decp_waves(const Tables* TT, const uint32_t* wave, int n, const DecpEnv& e, int reg, int i)
{
    float v = 0.0f;
    for (int w = 0; w < n; ++w) {
        const uint32_t wv = wave[w];
        const int inc = (int)(wv & 1023u), sf = (int)((wv >> 10) & 63u), ph = (int)((wv >> 16) & 31u);
        const double amp = (double)TT->amp_sf[sf];
        const int pos = ((ph << 6) + (i - (reg ^ 128)) * inc) & 2047;   // (pos0 + i * inc) & 2047
        v = (float)((double)v + (double)TT->sine[pos] * amp);
    }
    if (kEnv && e.hs) {
        const int pos = (e.s << 2) - reg;
        if (pos > 0 && pos <= 128) {
            if (i < pos) v = 0.0f;
            else if (i < pos + 4 && (!e.he || e.s != e.e)) v = v * TT->hann[32 * (i - pos)];
        }
    }
    if (kEnv && e.he) {
        const int pos = ((e.e + 1) << 2) - reg;
        if (pos > 0 && pos <= 128) {
            if (i >= pos) v = 0.0f;
            else if (i >= pos - 4) v = v * TT->hann[32 * (pos - 1 - i)];
        }
    }
    return v;
}

}  // namespace at3p
