/* C restatement of the sample-rate converter's definition (include/at3hip_resample.h), TEST INFRASTRUCTURE: the table, the
 * fmaf chain per output, and the streaming and flush rules, one stream and channel count at a time. Built with
 * gcc -O2 -ffp-contract=off -fno-fast-math (tests/resample_lib.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static const int kRates[] = {8000, 11025, 16000, 22050, 24000, 32000, 48000, 88200, 96000, 176400, 192000};

static int rate_ok(int hz)
{
    for (unsigned i = 0; i < sizeof(kRates) / sizeof(kRates[0]); ++i)
        if (kRates[i] == hz) return 1;
    return 0;
}

static int gcd(int a, int b)
{
    while (b) {
        int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

/* (L, M, K) of a pair; -1 for an unsupported one */
int rs_shape(int in, int out, int32_t* L, int32_t* M, int32_t* K)
{
    if (!((in == 44100 && rate_ok(out)) || (out == 44100 && rate_ok(in)))) return -1;
    int g = gcd(in, out), f_lo = in < out ? in : out;
    *L = out / g;
    *M = in / g;
    *K = 2 * (int)((72ll * in + f_lo - 1) / f_lo);   /* 2 ceil(72 in / f_lo) */
    return 0;
}

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

/* hp[L][K] */
int rs_table(int in, int out, float* hp)
{
    int32_t L, M, K;
    if (rs_shape(in, out, &L, &M, &K)) return -1;
    int f_lo = in < out ? in : out;
    double fc = 0.47675 * f_lo / in, beta = 0.1102 * (100.0 - 8.7);
    int half = K / 2;
    for (int p = 0; p < L; ++p)
        for (int k = 0; k < K; ++k) hp[(size_t)p * K + k] = (float)G((double)(k - (half - 1)) - (double)p / L, fc, beta, half);
    return 0;
}

/* One stream: every input sample kept (the restatement favours plainness over memory). */
typedef struct rs_stream {
    int32_t L, M, K, C;
    float* hp;
    float* x;          /* [cap][C] */
    int64_t T, cap;    /* samples received, capacity */
    int64_t n_out;     /* outputs emitted */
} rs_stream;

rs_stream* rs_create(int in, int out, int channels)
{
    rs_stream* s = calloc(1, sizeof(rs_stream));
    if (rs_shape(in, out, &s->L, &s->M, &s->K)) {
        free(s);
        return NULL;
    }
    s->C = channels;
    s->hp = malloc(sizeof(float) * s->L * s->K);
    rs_table(in, out, s->hp);
    return s;
}

void rs_destroy(rs_stream* s)
{
    if (!s) return;
    free(s->hp);
    free(s->x);
    free(s);
}

void rs_reset(rs_stream* s)
{
    s->T = 0;
    s->n_out = 0;
}

static float xin(const rs_stream* s, int64_t a, int c)
{
    return (a < 0 || a >= s->T) ? 0.0f : s->x[a * s->C + c];
}

/* outputs [s->n_out, n_end) into out [..][C] */
static int64_t emit(rs_stream* s, int64_t n_end, float* out)
{
    int64_t count = 0, half = s->K / 2;
    for (int64_t n = s->n_out; n < n_end; ++n, ++count) {
        int64_t i = n * s->M / s->L, p = n * s->M % s->L;
        for (int c = 0; c < s->C; ++c) {
            float acc = 0.0f;
            for (int k = 0; k < s->K; ++k) acc = fmaf(s->hp[p * s->K + k], xin(s, i + k - (half - 1), c), acc);
            out[count * s->C + c] = acc;
        }
    }
    s->n_out = n_end > s->n_out ? n_end : s->n_out;
    return count;
}

/* outputs whose i is below a: #{n : n M < a L} */
static int64_t below(const rs_stream* s, int64_t a) { return a <= 0 ? 0 : (a * s->L + s->M - 1) / s->M; }

/* in [n_in][C]; returns the outputs written to out */
int64_t rs_process(rs_stream* s, const float* in, int64_t n_in, float* out)
{
    if (s->T + n_in > s->cap) {
        int64_t cap = (s->T + n_in) * 2 + 16;
        s->x = realloc(s->x, sizeof(float) * cap * s->C);
        s->cap = cap;
    }
    memcpy(s->x + s->T * s->C, in, sizeof(float) * n_in * s->C);
    s->T += n_in;
    return emit(s, below(s, s->T - s->K / 2), out);   /* i + K/2 <= T - 1 */
}

int64_t rs_flush(rs_stream* s, float* out)
{
    int64_t n = emit(s, below(s, s->T), out);
    rs_reset(s);
    return n;
}
