/* C restatement of the look-ahead limiter's definition (include/at3hip_loudness.h, "The look-ahead limiter"), TEST
 * INFRASTRUCTURE: one stream at a time over the whole signal, plain loops, the naive window minimum and the naive sum. The
 * converter's table is the one tests/host/loudness_cpu.c restates (ld_tp_table; the caller passes it in). Built with
 * gcc -O2 -ffp-contract=off -fno-fast-math (tests/limiter_lib.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LA 220                        /* A: look-ahead */
#define LH 2205                       /* H: hold */
#define ONE30 (1u << 30)
#define FULL ((int64_t)(LA + 1) << 30)
#define TP_L 4
#define TP_K 144

static uint32_t mag(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return u & 0x7fffffffu;
}

static float unmag(uint32_t u)
{
    float v;
    memcpy(&v, &u, 4);
    return v;
}

static float sample(const float* x, int64_t T, int C, int64_t n, int c) { return (n < 0 || n >= T) ? 0.0f : x[n * C + c]; }

/* step 1: m[n], 0 <= n < T */
static float detector(const float* x, int64_t T, int C, int64_t n, const float* hp)
{
    uint32_t m = 0;
    for (int c = 0; c < C; ++c) {
        if (mag(sample(x, T, C, n, c)) > m) m = mag(sample(x, T, C, n, c));
        if (!hp) continue;
        for (int p = 0; p < TP_L; ++p) {
            float acc = 0.0f;
            for (int k = 0; k < TP_K; ++k) acc = fmaf(hp[p * TP_K + k], sample(x, T, C, n + k - (TP_K / 2 - 1), c), acc);
            if (mag(acc) > m) m = mag(acc);
        }
    }
    return unmag(m);
}

/* step 2 */
static uint32_t required(float g, float c, float m, double* r_out)
{
    double e = (double)g * (double)m;
    double r = e > (double)c ? (double)c / e : 1.0;
    if (r_out) *r_out = r;
    return (uint32_t)(r * 1073741824.0);
}

static uint32_t q_at(const uint32_t* q, int64_t T, int64_t n) { return (n < 0 || n >= T) ? ONE30 : q[n]; }

static uint32_t w_at(const uint32_t* q, int64_t T, int64_t n)
{
    uint32_t w = ONE30;
    for (int64_t j = n - LH; j <= n + LA; ++j)
        if (q_at(q, T, j) < w) w = q_at(q, T, j);
    return w;
}

/* (double) -> float toward zero, for d >= 0 */
static float to_float_rz(double d)
{
    float f = (float)d;
    if ((double)f > d) f = unmag(mag(f) - 1);
    return f;
}

/* x [T][C] -> y [T][C]; hp: the converter's table [4][144] for the true-peak detector, or NULL for the sample detector.
 * S_out [T] (int64) and r_out [T] (double) may be NULL. stats: {min S, count of S < FULL}. */
void lim_run(const float* x, int64_t T, int C, float g, float c, const float* hp, float* y, int64_t* S_out, double* r_out,
             int64_t* stats)
{
    uint32_t* q = malloc(sizeof(uint32_t) * (T ? T : 1));
    uint32_t* w = malloc(sizeof(uint32_t) * (T + LA + 1));   /* w[n - LA .. n] of every n < T: index j + LA */
    for (int64_t n = 0; n < T; ++n) q[n] = required(g, c, detector(x, T, C, n, hp), r_out ? &r_out[n] : NULL);
    for (int64_t j = -LA; j < T; ++j) w[j + LA] = w_at(q, T, j);
    stats[0] = FULL;
    stats[1] = 0;
    for (int64_t n = 0; n < T; ++n) {
        int64_t S = 0;
        for (int64_t j = n - LA; j <= n; ++j) S += (int64_t)w[j + LA];
        if (S_out) S_out[n] = S;
        if (S < stats[0]) stats[0] = S;
        if (S < FULL) ++stats[1];
        float s = to_float_rz((double)S / (double)FULL);
        for (int ch = 0; ch < C; ++ch) {
            float t = (x[n * C + ch] * g) * s;
            y[n * C + ch] = t > c ? c : (t < -c ? -c : t);
        }
    }
    free(q);
    free(w);
}
