// The body of the ATRAC3plus decoder's unpack kernel, included by at3p_decode.hpp once per parse: DECP_UNPACK_KERNEL names the
// kernel template, DECP_UNPACK_SPARSE is decp_parse's kSparse. Text inclusion and not a device function both kernels call: through
// such a function (forced inline, its LDS inside or handed in) the compiler makes other code for the unflagged kernels than it made
// before there was a second parse, and those stay instruction for instruction what they were.
// kSized: the frame size is the parameter block's; otherwise it is 2048 and every limit folds to the constant it was before
// frames had a size (the parse is one lane's serial code, and a limit held in a register instead of an immediate costs it 2 %).
template <bool kSized>
__global__ __launch_bounds__(kDecUnpackThreads) void DECP_UNPACK_KERNEL(DecUnpackParams p)
{
    constexpr int NT = kDecUnpackThreads;
    __shared__ uint32_t s_w[512 + 2];                              // the frame, big-endian words, two zero words behind
    __shared__ __attribute__((aligned(16))) float s_spec[2][2048];   // the dequantised spectra
    __shared__ __attribute__((aligned(16))) cpx s_f[32 * 64];       // the 16 x C 64-point FFTs
    __shared__ uint8_t s_wl[2][32], s_sf[2][32], s_tab[2][32];
    __shared__ uint16_t s_win[2];
    __shared__ int s_reason;
    __shared__ TonalRec s_tone;

    const DecTables* T = p.T;
    const int f = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, C = p.nch;
    // s_w holds the largest frame; the words behind this frame's are zero and no read reaches them (the reader's limit)
    const int frame_bytes = kSized ? p.frame_bytes : 2048, n_words = frame_bytes >> 2;
    const uint8_t* frame = p.frames + ((size_t)s * p.n_frames + f) * (size_t)frame_bytes;
    for (int i = tid; i < 512 + 2; i += NT) {   // byte loads: a caller's device buffer need not be word-aligned
        uint32_t w = 0;
        if (i < n_words)
            for (int k = 0; k < 4; ++k) w = (w << 8) | frame[4 * i + k];
        s_w[i] = w;
    }
    for (int i = tid; i < 2 * 2048; i += NT) (&s_spec[0][0])[i] = 0.0f;
    if (tid < 2) s_win[tid] = 0;
    for (int i = tid; i < kTonalWords; i += NT) ((uint32_t*)&s_tone)[i] = 0u;
    __syncthreads();
    if (tid == 0) {
        MsbReader b(s_w, 8 * frame_bytes);
        const int why = decp_parse<DECP_UNPACK_SPARSE>(b, T, C, &s_spec[0][0], s_wl, s_sf, s_tab, s_win, p.tone_vlc, p.tones ? &s_tone : nullptr);
        s_reason = why;
        if (why) atomicAdd(&p.rejected[why - 1], 1ull);
    }
    __syncthreads();
    const bool rejected = s_reason != kRpOk;
    if (tid < C) p.flags[decp_rec(f + 2, s, tid, p.n_streams, C)] = rejected ? (uint16_t)0 : s_win[tid];
    {   // the frame's tonal record; none for a rejected frame
        uint32_t* rec = (uint32_t*)decp_tonal_rec(p.tonal, f, s, p.n_streams);
        for (int i = tid; i < kTonalWords; i += NT) rec[i] = rejected ? 0u : ((const uint32_t*)&s_tone)[i];
    }
    // TMIDCT<256> pre-rotation per subband (odd subbands: SwapArray folded into the index), into the FFT's leaf order; a
    // rejected frame has a zero spectrum
    const float* cs = T->cs256;
    for (int j = tid; j < C * 1024; j += NT) {
        const int ch = j >> 10, band = (j >> 6) & 15, k2 = j & 63, n = 2 * k2;
        const int a = band & 1 ? 127 - n : n, bb = band & 1 ? n : 127 - n;
        const float* sp = &s_spec[ch][band * 128];
        const float r0 = rejected ? 0.0f : sp[a];
        const float i0 = rejected ? 0.0f : sp[bb];
        s_f[(ch * 16 + band) * 64 + at3::fft_leaf_pos<64>(k2)] = at3::midct_pre(r0, i0, cs[n], cs[n + 1]);
    }
    __syncthreads();
    at3::fft_lds<64, false>(s_f, 64, 16 * C, T->tw64, tid, NT);
    // post-rotation (mdct.h): the whole Buf[256] of each subband
    for (int j = tid; j < C * 1024; j += NT) {
        const int ch = j >> 10, band = (j >> 6) & 15, k2 = j & 63, n = 2 * k2;
        float r1, i1;
        at3::midct_post(s_f[j], cs[n], cs[n + 1], r1, i1);
        float* o = p.raw + decp_rec(f + 2, s, ch, p.n_streams, C) * 4096 + band * 256;
        at3::midct_unfold<64>(n, r1, i1, [&](int x, float v) { o[x] = v; });
    }
}
