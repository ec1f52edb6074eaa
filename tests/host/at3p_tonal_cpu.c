/* TEST INFRASTRUCTURE ONLY - the entry points of the C restatement of the ATRAC3plus decoder with tonal blocks (include/at3phip.h,
 * TONAL BLOCKS) at 2048 bytes, and the encoder's ApplyFilter. The tonal block's syntax, step 4b and the frame loop are
 * tests/host/at3p_decode_cpu.c's, included here; a stream of this file keeps frame n - 1's record beside that file's state. Compiled
 * by the tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
#include "at3p_decode_cpu.c"

typedef struct {
    at3pd_stream base;
    trec prev;   /* frame n-1's record with the curr_env step 4b gave it */
} at3pt_stream;

size_t at3pt_state_bytes(void) { return sizeof(at3pt_stream); }
void at3pt_reset(void* state)
{
    init_tables();
    init_tone_tables();
    memset(state, 0, sizeof(at3pt_stream));
}

/* frames [n][2048] -> pcm [n][2048][C] float32 with tonal blocks (tones = 1) or as the decoder without the flag; rejected [6] */
void at3pt_decode(void* state, int C, const uint8_t* frames, int n_frames, float* pcm, uint64_t* rejected, int tones)
{
    at3pt_stream* st = (at3pt_stream*)state;
    decode_frames(&st->base, &st->prev, C, frames, 2048, n_frames, pcm, rejected, NULL, tones, 0);
}

/* steps 1-2 with tonal blocks for the golden generator: specs [C][2048], win [C] and the record as flat ints:
 * present, then per (ch, band) nw, start_index, has_start, start, has_stop, stop, then freq[48], amp_sf[48], phase[48] */
int at3pt_unpack_frame(const uint8_t* frame, int C, float* specs, uint16_t* win, int32_t* rec)
{
    trec r;
    at3pd_fields f;
    const int why = unpack(frame, 2048, C, specs, win, &r, &f, 0);
    int k = 0;
    rec[k++] = r.present;
    for (int ch = 0; ch < 2; ++ch)
        for (int b = 0; b < 16; ++b) {
            const tband* t = &r.band[ch][b];
            rec[k++] = t->nw; rec[k++] = t->start_index;
            rec[k++] = t->pend.has_start; rec[k++] = t->pend.start; rec[k++] = t->pend.has_stop; rec[k++] = t->pend.stop;
        }
    for (int i = 0; i < 48; ++i) rec[k++] = r.freq[i];
    for (int i = 0; i < 48; ++i) rec[k++] = r.amp_sf[i];
    for (int i = 0; i < 48; ++i) rec[k++] = r.phase[i];
    return why;
}

/* the encoder's ApplyFilter for the round-trip test: per call one frame's subband samples sub [C][2048] (rewritten) and its
 * record, flattened as at3pt_unpack_frame writes it; state: at3pt_filter_bytes() bytes, zeroed at start */
size_t at3pt_filter_bytes(void) { return sizeof(trec); }
void at3pt_apply_filter(void* state, int C, const int32_t* rec, float* sub)
{
    trec* prev = (trec*)state;
    trec cur;
    init_tone_tables();
    memset(&cur, 0, sizeof(cur));
    int k = 0;
    cur.present = rec[k++];
    for (int ch = 0; ch < 2; ++ch)
        for (int b = 0; b < 16; ++b) {
            tband* t = &cur.band[ch][b];
            t->nw = rec[k++]; t->start_index = rec[k++];
            t->pend.has_start = rec[k++]; t->pend.start = rec[k++]; t->pend.has_stop = rec[k++]; t->pend.stop = rec[k++];
        }
    for (int i = 0; i < 48; ++i) cur.freq[i] = rec[k++];
    for (int i = 0; i < 48; ++i) cur.amp_sf[i] = rec[k++];
    for (int i = 0; i < 48; ++i) cur.phase[i] = rec[k++];
    for (int ch = 0; ch < C; ++ch)
        if (cur.present || prev->present)
            for (int sb = 0; sb < 16; ++sb)
                if (cur.band[ch][sb].nw || prev->band[ch][sb].nw) generate_tones(prev, &cur, ch, sb, sub + ch * 2048 + sb * 128, 1);
    *prev = cur;
}

void at3pt_tone_tables(float* sine, float* hann, float* amp_sf)
{
    init_tone_tables();
    memcpy(sine, TT.sine, sizeof(TT.sine));
    memcpy(hann, TT.hann, sizeof(TT.hann));
    memcpy(amp_sf, TT.amp_sf, sizeof(TT.amp_sf));
}
