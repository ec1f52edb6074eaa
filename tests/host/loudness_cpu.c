/* C restatement of the loudness meter's definition (include/at3hip_loudness.h), TEST INFRASTRUCTURE: the K-weighting chain with
 * its restart per hop, the peaks (the 44100 -> 176400 converter of include/at3hip_resample.h restated once more for the true
 * peak), the gating and the gain, one stream at a time over the whole signal. Built with gcc -O2 -ffp-contract=off
 * -fno-fast-math (tests/loudness_lib.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HOP 4410

/* {b0, b1, b2, a1, a2} */
static const double kStage1[5] = {1.5308412300503478, -2.6509799951547297, 1.169079079921587, -1.6636551132560204, 0.7125954280732254};
static const double kStage2[5] = {1.0, -2.0, 1.0, -1.989169673629796, 0.9891990357870393};

void ld_coeffs(double* out)
{
    memcpy(out, kStage1, sizeof(kStage1));
    memcpy(out + 5, kStage2, sizeof(kStage2));
}

typedef struct biquad {
    double s1, s2;
} biquad;

static double step(biquad* f, const double* k, double x)
{
    double y = k[0] * x + f->s1;
    f->s1 = (k[1] * x - k[3] * y) + f->s2;
    f->s2 = k[2] * x - k[4] * y;
    return y;
}

/* x [T][C] -> z [T / 4410][C]; warm = the hops of warm-up before each hop (the definition: 2) */
static void hops_warm(const float* x, int64_t T, int C, double* z, int warm)
{
    int64_t H = T / HOP;
    for (int64_t j = 0; j < H; ++j)
        for (int c = 0; c < C; ++c) {
            biquad f1 = {0.0, 0.0}, f2 = {0.0, 0.0};
            int64_t start = HOP * (j > warm ? j - warm : 0);
            double acc = 0.0;
            for (int64_t n = start; n < HOP * (j + 1); ++n) {
                double y2 = step(&f2, kStage2, step(&f1, kStage1, (double)x[n * C + c]));
                if (n >= HOP * j) acc = acc + y2 * y2;
            }
            z[j * C + c] = acc;
        }
}

void ld_hops(const float* x, int64_t T, int C, double* z) { hops_warm(x, T, C, z, 2); }
void ld_hops_warm(const float* x, int64_t T, int C, double* z, int warm) { hops_warm(x, T, C, z, warm); }

/* the same sums from a filter that is never restarted (what the definition approximates) */
void ld_hops_continuous(const float* x, int64_t T, int C, double* z)
{
    int64_t H = T / HOP;
    for (int c = 0; c < C; ++c) {
        biquad f1 = {0.0, 0.0}, f2 = {0.0, 0.0};
        for (int64_t j = 0; j < H; ++j) {
            double acc = 0.0;
            for (int64_t n = HOP * j; n < HOP * (j + 1); ++n) {
                double y2 = step(&f2, kStage2, step(&f1, kStage1, (double)x[n * C + c]));
                acc = acc + y2 * y2;
            }
            z[j * C + c] = acc;
        }
    }
}

/* magnitudes are compared as the float's bits without the sign */
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

void ld_sample_peak(const float* x, int64_t T, int C, float* out)
{
    out[0] = out[1] = 0.0f;
    for (int c = 0; c < C; ++c) {
        uint32_t m = 0;
        for (int64_t n = 0; n < T; ++n)
            if (mag(x[n * C + c]) > m) m = mag(x[n * C + c]);
        out[c] = unmag(m);
    }
}

/* ---- the 44100 -> 176400 table of at3hip_resample.h: L = 4, M = 1, K = 144, fc = 0.47675 ---- */
#define TP_L 4
#define TP_K 144

static double i0(double x)
{
    double q = (x / 2) * (x / 2), t = 1.0, s = 0.0;
    s += t;
    for (int m = 1; m < 40; ++m) {
        t = t * q / ((double)m * m);
        s += t;
    }
    return s;
}

static double G(double d, double fc, double beta, int half)
{
    double x = 2 * fc * d;
    double sinc = (x == 0.0) ? 1.0 : sin(M_PI * x) / (M_PI * x);
    double r = d / half;
    double w = 1 - r * r;
    if (w < 0) w = 0;
    return 2 * fc * sinc * i0(beta * sqrt(w)) / i0(beta);
}

void ld_tp_table(float* hp)
{
    double fc = 0.47675 * 44100 / 44100, beta = 0.1102 * (100.0 - 8.7);
    int half = TP_K / 2;
    for (int p = 0; p < TP_L; ++p)
        for (int k = 0; k < TP_K; ++k) hp[p * TP_K + k] = (float)G((double)(k - (half - 1)) - (double)p / TP_L, fc, beta, half);
}

/* the larger of the sample peak and the largest |u| over all 4T outputs of the converter (zeros before and past the signal) */
void ld_true_peak(const float* x, int64_t T, int C, float* out)
{
    float hp[TP_L * TP_K];
    ld_tp_table(hp);
    ld_sample_peak(x, T, C, out);
    for (int c = 0; c < C; ++c) {
        uint32_t m = mag(out[c]);
        for (int64_t n = 0; n < TP_L * T; ++n) {
            int64_t i = n / TP_L, p = n % TP_L;
            float acc = 0.0f;
            for (int k = 0; k < TP_K; ++k) {
                int64_t a = i + k - (TP_K / 2 - 1);
                acc = fmaf(hp[p * TP_K + k], (a < 0 || a >= T) ? 0.0f : x[a * C + c], acc);
            }
            if (mag(acc) > m) m = mag(acc);
        }
        out[c] = unmag(m);
    }
}

/* ---- gating and gain ---- */
typedef struct ld_result {
    double integrated, momentary_max, short_term_max;
    float sample_peak[2], true_peak[2];
    int64_t n_samples;
    int32_t n_hops, n_blocks_kept;
} ld_result;

static double lufs(double p) { return -0.691 + 10.0 * log10(p); }

/* relative = 0 disables the relative gate (used to show that a test exercises it) */
void ld_gate_opt(const double* z, int32_t H, int32_t C, ld_result* r, int relative)
{
    r->n_hops = H;
    r->n_blocks_kept = 0;
    r->integrated = r->momentary_max = r->short_term_max = -HUGE_VAL;
    int nb = H - 3;
    if (nb > 0) {
        double* P = malloc(sizeof(double) * nb);
        double* l = malloc(sizeof(double) * nb);
        for (int b = 0; b < nb; ++b) {
            double sum = 0.0;
            for (int c = 0; c < C; ++c) {
                double t = ((z[b * C + c] + z[(b + 1) * C + c]) + z[(b + 2) * C + c]) + z[(b + 3) * C + c];
                sum = c == 0 ? t : sum + t;
            }
            P[b] = sum / 17640.0;
            l[b] = lufs(P[b]);
            if (l[b] > r->momentary_max) r->momentary_max = l[b];
        }
        double sum = 0.0;
        int n = 0;
        for (int b = 0; b < nb; ++b)
            if (l[b] > -70.0) {
                sum = sum + P[b];
                ++n;
            }
        if (n > 0) {
            double rel = relative ? lufs(sum / (double)n) - 10.0 : -HUGE_VAL;
            sum = 0.0;
            n = 0;
            for (int b = 0; b < nb; ++b)
                if (l[b] > -70.0 && l[b] > rel) {
                    sum = sum + P[b];
                    ++n;
                }
            if (n > 0) {
                r->integrated = lufs(sum / (double)n);
                r->n_blocks_kept = n;
            }
        }
        free(P);
        free(l);
    }
    for (int b = 0; b + 30 <= H; ++b) {
        double sum = 0.0;
        for (int c = 0; c < C; ++c) {
            double t = z[b * C + c];
            for (int k = 1; k < 30; ++k) t = t + z[(b + k) * C + c];
            sum = c == 0 ? t : sum + t;
        }
        double v = lufs(sum / 132300.0);
        if (v > r->short_term_max) r->short_term_max = v;
    }
}

void ld_gate(const double* z, int32_t H, int32_t C, ld_result* r) { ld_gate_opt(z, H, C, r, 1); }

float ld_gain(const ld_result* r, double target, double ceiling_db)
{
    int measured = r->true_peak[0] != 0.0f || r->true_peak[1] != 0.0f;
    const float* pk = measured ? r->true_peak : r->sample_peak;
    double peak = (double)(pk[0] > pk[1] ? pk[0] : pk[1]);
    if (r->integrated == -HUGE_VAL || peak == 0.0) return 1.0f;
    double a = pow(10.0, (target - r->integrated) / 20.0);
    double b = pow(10.0, ceiling_db / 20.0) / peak;
    return (float)(a < b ? a : b);
}

/* the whole meter over one stream x [T][C] */
void ld_measure(const float* x, int64_t T, int C, int true_peak, ld_result* r)
{
    int64_t H = T / HOP;
    double* z = malloc(sizeof(double) * (H ? H : 1) * C);
    ld_hops(x, T, C, z);
    ld_gate(z, (int32_t)H, C, r);
    free(z);
    r->n_samples = T;
    ld_sample_peak(x, T, C, r->sample_peak);
    r->true_peak[0] = r->true_peak[1] = 0.0f;
    if (true_peak) ld_true_peak(x, T, C, r->true_peak);
}
