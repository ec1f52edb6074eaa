/* TEST INFRASTRUCTURE: the CPU side of the float-domain tests as a stand-alone program, so that it can be built with
 * -fsanitize=address,undefined,float-cast-overflow and run as a child process (nothing sanitized is loaded into Python).
 *
 *     float_domain_main FILE
 *
 * FILE is written by tests/test_float_domain_cpu.py from tests/float_domain_lib.py's pattern table:
 *     int32 n_patterns, int32 n_blocks (12), int32 meter_samples (52920)
 *     per pattern: char name[16], float pcm[n_blocks][1024][2], float meter[meter_samples][2]
 * Every pattern goes through every CPU definition a GPU engine is compared with: the three encoder oracles (oracle/*.c) in
 * the settings of tests/test_float_domain_gpu.py, tests/host/resample_cpu.c, tests/host/loudness_cpu.c, tests/host/limiter_cpu.c
 * (both detectors, six pairs of gain and ceiling) and tests/host/at3p_gha_cpu.c (every flag combination). Each run is
 * made twice and must give the same bytes (a read of uninitialised memory that no sanitizer of this build sees shows as
 * a difference). Exit status 0 and no sanitizer report is a pass; the program itself reports only nondeterminism. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/at3phip.h"
#include "../../oracle/at3_oracle.h"

int at1o_encode(const float* pcm, int nch, int n_blocks, int window_auto, int window_mask, int bfu_idx_const, uint8_t* out,
                float* tap_specs, int32_t* tap_masks, float* tap_loud);
void at3po_pqf_analyse(const float* in, int n_frames, float* out);
void at3po_mdct(const float* bands, const uint16_t* win_flags, int n_frames, float* specs);
int at3po_write_frames(const float* specs, const uint16_t* win_flags, int channels, int n_frames, uint8_t* out, void* info);

typedef struct rs_stream rs_stream;
rs_stream* rs_create(int in, int out, int channels);
void rs_destroy(rs_stream* s);
int64_t rs_process(rs_stream* s, const float* in, int64_t n_in, float* out);
int64_t rs_flush(rs_stream* s, float* out);

typedef struct ld_result {
    double integrated, momentary_max, short_term_max;
    float sample_peak[2], true_peak[2];
    int64_t n_samples;
    int32_t n_hops, n_blocks_kept;
} ld_result;
void ld_hops(const float* x, int64_t T, int C, double* z);
void ld_measure(const float* x, int64_t T, int C, int true_peak, ld_result* r);

void ld_tp_table(float* out);
void lim_run(const float* x, int64_t T, int C, float g, float c, const float* hp, float* y, int64_t* S_out, double* r_out,
             int64_t* stats);

size_t at3pg_state_bytes(void);
void at3pg_reset(void* state);
void at3pg_analyse(void* state, int C, const float* bands, int n, at3phip_tonal_block* blocks, float* residual, uint32_t flags,
                   int8_t* intervals, int32_t* found);

enum { kBlock = 1024, kMaxBlocks = 64 };

static int failures = 0;

static void* xmalloc(size_t n)
{
    void* p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return p;
}

/* the bytes of two runs; a NaN's payload is part of the comparison (the same program on the same input) */
static void same(const char* pat, const char* what, const void* a, const void* b, size_t n)
{
    if (memcmp(a, b, n) != 0) {
        fprintf(stderr, "%s: %s differs between two runs\n", pat, what);
        ++failures;
    }
}

static void channel_of(const float* pcm2, size_t n, int nch, float* out)
{
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < nch; ++c) out[i * nch + c] = pcm2[2 * i + c];
}

static void run_at3(const char* pat, const float* pcm2, int nb)
{
    static const int rows[5][4] = {{132300, 0, 0, 2}, {132300, 1, 1, 2}, {66150, 0, 0, 2}, {66150, 1, 1, 2}, {66150, 0, 0, 1}};
    float* pcm = xmalloc(sizeof(float) * nb * kBlock * 2);
    unsigned char* out[2];
    for (int k = 0; k < 2; ++k) out[k] = xmalloc((size_t)nb * 1024);
    for (int r = 0; r < 5; ++r) {
        const int nch = rows[r][3];
        channel_of(pcm2, (size_t)nb * kBlock, nch, pcm);
        int n[2], fsz[2];
        for (int k = 0; k < 2; ++k) {
            memset(out[k], 0, (size_t)nb * 1024);
            n[k] = at3o_encode(rows[r][0], nch, rows[r][1], rows[r][2], 0, pcm, nb, out[k], &fsz[k], NULL);
        }
        if (n[0] != nb - 1 || n[1] != n[0] || fsz[0] != fsz[1]) { fprintf(stderr, "%s: at3o_encode returned %d, %d\n", pat, n[0], n[1]); ++failures; continue; }
        same(pat, "ATRAC3 frames", out[0], out[1], (size_t)n[0] * fsz[0]);
    }
    free(pcm); free(out[0]); free(out[1]);
}

static void run_at1(const char* pat, const float* pcm2, int nb)
{
    static const int modes[2][2] = {{1, 0}, {0, 7}};   /* auto, short: (window_auto, window_mask) */
    const int n1 = 2 * nb;
    float* pcm = xmalloc(sizeof(float) * n1 * 512 * 2);
    uint8_t* out[2];
    float* loud[2];
    float* specs = xmalloc(sizeof(float) * n1 * 2 * 512);
    int32_t* masks = xmalloc(sizeof(int32_t) * n1 * 2);
    for (int k = 0; k < 2; ++k) { out[k] = xmalloc((size_t)n1 * 2 * 212); loud[k] = xmalloc(sizeof(float) * n1); }
    for (int m = 0; m < 2; ++m)
        for (int nch = 1; nch <= 2; ++nch) {
            channel_of(pcm2, (size_t)n1 * 512, nch, pcm);
            for (int k = 0; k < 2; ++k) {
                const int n = at1o_encode(pcm, nch, n1, modes[m][0], modes[m][1], 0, out[k], specs, masks, loud[k]);
                if (n != n1 * nch * 212) { fprintf(stderr, "%s: at1o_encode returned %d\n", pat, n); ++failures; }
            }
            same(pat, "ATRAC1 sound units", out[0], out[1], (size_t)n1 * nch * 212);
            same(pat, "ATRAC1 loudness", loud[0], loud[1], sizeof(float) * n1);
        }
    free(pcm); free(specs); free(masks);
    for (int k = 0; k < 2; ++k) { free(out[k]); free(loud[k]); }
}

static void run_at3p(const char* pat, const float* pcm2, int nb)
{
    const int nf = nb / 2;
    float* x = xmalloc(sizeof(float) * nf * 2048);
    float* bands = xmalloc(sizeof(float) * nf * 2048);
    float* specs = xmalloc(sizeof(float) * nf * 2 * 2048);
    float* one = xmalloc(sizeof(float) * nf * 2048);
    uint8_t* out[2];
    for (int k = 0; k < 2; ++k) out[k] = xmalloc((size_t)nf * 2048);
    for (int nch = 1; nch <= 2; ++nch) {
        for (int k = 0; k < 2; ++k) {
            for (int c = 0; c < nch; ++c) {
                for (int i = 0; i < nf * 2048; ++i) x[i] = pcm2[2 * i + c];
                at3po_pqf_analyse(x, nf, bands);
                for (int i = 0; i < nf * 2048; ++i) bands[i] = (float)((double)bands[i] / (32768.0 / 1.122018));
                at3po_mdct(bands, NULL, nf, one);
                for (int f = 0; f < nf; ++f) memcpy(specs + ((size_t)f * nch + c) * 2048, one + (size_t)f * 2048, sizeof(float) * 2048);
            }
            const int n = at3po_write_frames(specs, NULL, nch, nf, out[k], NULL);
            if (n != nf) { fprintf(stderr, "%s: at3po_write_frames returned %d\n", pat, n); ++failures; }
        }
        same(pat, "ATRAC3plus frames", out[0], out[1], (size_t)nf * 2048);
    }
    free(x); free(bands); free(specs); free(one); free(out[0]); free(out[1]);
}

static void run_resample(const char* pat, const float* pcm2)
{
    static const int pairs[2][2] = {{48000, 44100}, {44100, 48000}};
    enum { T = 3001, kFirst = 2048, kMaxOut = 2 * T };
    float* x = xmalloc(sizeof(float) * T * 2);
    float* out[2];
    for (int k = 0; k < 2; ++k) out[k] = xmalloc(sizeof(float) * kMaxOut * 2);
    for (int p = 0; p < 2; ++p)
        for (int nch = 1; nch <= 2; ++nch) {
            channel_of(pcm2 + 2 * kFirst, T, nch, x);
            int64_t n[2];
            for (int k = 0; k < 2; ++k) {
                rs_stream* s = rs_create(pairs[p][0], pairs[p][1], nch);
                if (!s) { fprintf(stderr, "rs_create failed\n"); exit(2); }
                n[k] = rs_process(s, x, T, out[k]);
                n[k] += rs_flush(s, out[k] + n[k] * nch);
                rs_destroy(s);
            }
            if (n[0] != n[1] || n[0] > kMaxOut) { fprintf(stderr, "%s: resampler output counts %lld, %lld\n", pat, (long long)n[0], (long long)n[1]); ++failures; continue; }
            same(pat, "resampled samples", out[0], out[1], sizeof(float) * (size_t)n[0] * nch);
        }
    free(x); free(out[0]); free(out[1]);
}

static void run_meter(const char* pat, const float* meter2, int T)
{
    float* x = xmalloc(sizeof(float) * T * 2);
    double* z[2];
    for (int k = 0; k < 2; ++k) z[k] = xmalloc(sizeof(double) * (T / 4410 + 1) * 2);
    for (int nch = 1; nch <= 2; ++nch) {
        channel_of(meter2, (size_t)T, nch, x);
        ld_result r[2];
        for (int k = 0; k < 2; ++k) {
            memset(&r[k], 0, sizeof(r[k]));
            ld_hops(x, T, nch, z[k]);
            ld_measure(x, T, nch, 1, &r[k]);
        }
        same(pat, "hop sums", z[0], z[1], sizeof(double) * (size_t)(T / 4410) * nch);
        same(pat, "meter result", &r[0], &r[1], sizeof(ld_result));
    }
    free(x); free(z[0]); free(z[1]);
}

/* tests/host/limiter_cpu.c on the first 6000 samples, both detectors, float_domain_lib.LIMITER_PAIRS */
static void run_limiter(const char* pat, const float* pcm2)
{
    enum { T = 6000 };
    const float ceil1 = 0.8912509381337456f, tiny = 1.4e-45f, big = 3.4028234663852886e38f;   /* -1 dBFS, the smallest subnormal, FLT_MAX */
    const float pairs[6][2] = {{0.0f, ceil1}, {2.0f, ceil1}, {big, ceil1}, {2.0f, tiny}, {2.0f, big}, {tiny, ceil1}};
    static float hp[4 * 144];
    ld_tp_table(hp);
    float* x = xmalloc(sizeof(float) * T * 2);
    float* y[2];
    for (int k = 0; k < 2; ++k) y[k] = xmalloc(sizeof(float) * T * 2);
    for (int nch = 1; nch <= 2; ++nch) {
        channel_of(pcm2, T, nch, x);
        for (int tp = 0; tp < 2; ++tp)
            for (int p = 0; p < 6; ++p) {
                int64_t stats[2][2];
                for (int k = 0; k < 2; ++k) {
                    memset(y[k], 0xA5, sizeof(float) * T * 2);
                    lim_run(x, T, nch, pairs[p][0], pairs[p][1], tp ? hp : NULL, y[k], NULL, NULL, stats[k]);
                }
                same(pat, "limited samples", y[0], y[1], sizeof(float) * T * nch);
                same(pat, "limiter statistics", stats[0], stats[1], sizeof(stats[0]));
            }
    }
    free(x); free(y[0]); free(y[1]);
}

/* tests/host/at3p_gha_cpu.c on the oracle's subbands of the 6 frames, every combination of the two flags */
static void run_tones(const char* pat, const float* pcm2, int nb)
{
    const int nf = nb / 2;
    float* x = xmalloc(sizeof(float) * nf * 2048);
    float* one = xmalloc(sizeof(float) * nf * 2048);
    float* bands = xmalloc(sizeof(float) * nf * 2 * 2048);
    void* state = xmalloc(at3pg_state_bytes());
    at3phip_tonal_block* blocks[2];
    float* resid[2];
    for (int k = 0; k < 2; ++k) {
        blocks[k] = xmalloc(sizeof(at3phip_tonal_block) * nf);
        resid[k] = xmalloc(sizeof(float) * nf * 2 * 2048);
    }
    for (int nch = 1; nch <= 2; ++nch) {
        for (int c = 0; c < nch; ++c) {
            for (int i = 0; i < nf * 2048; ++i) x[i] = pcm2[2 * i + c];
            at3po_pqf_analyse(x, nf, one);
            for (int f = 0; f < nf; ++f) memcpy(bands + ((size_t)f * nch + c) * 2048, one + (size_t)f * 2048, sizeof(float) * 2048);
        }
        for (uint32_t flags = 0; flags < 4; ++flags) {
            const uint32_t fl = ((flags & 1) ? AT3PHIP_TONES_GATED : 0) | ((flags & 2) ? AT3PHIP_TONES_SHARED : 0);
            for (int k = 0; k < 2; ++k) {
                memset(blocks[k], 0, sizeof(at3phip_tonal_block) * nf);
                memset(resid[k], 0xA5, sizeof(float) * nf * 2 * 2048);
                at3pg_reset(state);
                at3pg_analyse(state, nch, bands, nf, blocks[k], resid[k], fl, NULL, NULL);
            }
            same(pat, "tonal records", blocks[0], blocks[1], sizeof(at3phip_tonal_block) * nf);
            same(pat, "tone residuals", resid[0], resid[1], sizeof(float) * nf * nch * 2048);
        }
    }
    free(x); free(one); free(bands); free(state);
    for (int k = 0; k < 2; ++k) { free(blocks[k]); free(resid[k]); }
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[3];
    if (fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] < 1 || hdr[1] < 6 || hdr[1] > kMaxBlocks || (hdr[1] & 1) || hdr[2] < 4410 || hdr[2] > (1 << 20)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int nb = hdr[1], T = hdr[2];
    const size_t n_pcm = (size_t)nb * kBlock * 2, n_meter = (size_t)T * 2;
    float* pcm = xmalloc(sizeof(float) * n_pcm);
    float* meter = xmalloc(sizeof(float) * n_meter);
    for (int p = 0; p < hdr[0]; ++p) {
        char name[17] = {0};
        if (fread(name, 1, 16, f) != 16 || fread(pcm, sizeof(float), n_pcm, f) != n_pcm || fread(meter, sizeof(float), n_meter, f) != n_meter) {
            fprintf(stderr, "short file at pattern %d\n", p);
            return 2;
        }
        run_at3(name, pcm, nb);
        run_at1(name, pcm, nb);
        run_at3p(name, pcm, nb);
        run_resample(name, pcm);
        run_meter(name, meter, T);
        run_limiter(name, pcm);
        run_tones(name, pcm, nb);
        printf("%s done\n", name);
    }
    free(pcm); free(meter);
    fclose(f);
    if (failures) { fprintf(stderr, "%d comparisons failed\n", failures); return 1; }
    printf("FLOAT DOMAIN OK: %d patterns\n", hdr[0]);
    return 0;
}
