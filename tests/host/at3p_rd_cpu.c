/* TEST INFRASTRUCTURE ONLY - CPU restatement of the ATRAC3plus adaptive writer with RATE-DISTORTION WORD LENGTHS (include/at3phip.h,
 * R1-R5) and with MASKING-WEIGHTED WORD LENGTHS (M1-M7), which are the former with an offset o per unit: lambda shifted by it, the scan
 * reaching down by the largest, the guard's sums weighted. A1, A2, A4s, the frame's layout (A6s) and the decoder are
 * tests/host/at3p_writer_cpu.c's, included here as that file includes its predecessors; R1-R4 and M1-M6, the distortion table, the
 * thresholds and offsets, the candidates, the two scans and the guard, are written out here in plain scalar C from the header's text,
 * with the two integer tables of atracdenc_amd/csrc/at3p_psy.inc. o == NULL is R throughout.
 * Compiled by the tests with gcc -O2 -fPIC -ffp-contract=off -fno-fast-math. */
#include "at3p_writer_cpu.c"
#include "../../atracdenc_amd/csrc/at3p_psy.inc"

#define J_MIN (-30)
#define J_MAX 69
#define MU_HI 73
#define O_MAX 32

/* R1: S[ch][qu][w], from A1's scaled values (values [channels][2048]) */
static void rd_dist_table(const float* values, int channels, uint64_t* dist)
{
    int mant[128];
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            const int start = kQuStart[qu], n = kSpecsPerBlock[qu];
            const float* v = values + ch * 2048 + start;
            for (int w = 0; w < 8; ++w) {
                if (w) quantise(v, n, w, mant);
                else memset(mant, 0, sizeof(mant));
                uint64_t S = 0;
                for (int i = 0; i < n; ++i) {
                    const float q = (float)mant[i] * AT3P_MANT[w];
                    const float e = v[i] - q;
                    const float d = e * e;
                    if (d == d) S += (uint64_t)(d * 0x1p40f);   /* NaN: u = 0 */
                }
                dist[(ch * 32 + qu) * 8 + w] = S;
            }
        }
}

/* A1 + A2 + R1 of one frame */
int at3prd_tables(const float* specs, int channels, uint8_t* sfi, uint16_t* bits, uint8_t* tab, uint64_t* dist, float* values_out)
{
    float values[2 * 2048];
    if (at3pw_cost_table(specs, channels, sfi, bits, tab, values) != 0) return -1;
    rd_dist_table(values, channels, dist);
    if (values_out) memcpy(values_out, values, sizeof(float) * 2048 * (size_t)channels);
    return 0;
}

static double rd_G(int i) { return (double)AT3P_SCALE[i] * (double)AT3P_SCALE[i]; }

/* R2: lambda_j = 2^40 G[j mod 3] 4^floor(j / 3) */
static double rd_lam(int j)
{
    int q = j / 3, r = j % 3;
    if (r < 0) {
        r += 3;
        q -= 1;
    }
    return ldexp(rd_G(r), 40 + 2 * q);   /* (exact: a power of two) */
}

static int rd_pick_w(const uint64_t* S, const uint16_t* B, int sfi, int j)
{
    const double lam = rd_lam(j), G = rd_G(sfi);
    int best = 0;
    double least = 0;
    for (int w = 0; w < 8; ++w) {
        const double D = (double)S[w] * G;
        const double rate = lam * (double)(w ? B[w] + 3 : 0);
        const double cost = D + rate;
        if (w == 0 || cost < least) {
            least = cost;
            best = w;
        }
    }
    return best;
}

/* M1-M3: mu [channels][32] and the offsets o [2][32]; returns O */
static int psy_offsets(const uint8_t* sfi, const uint64_t* dist, int channels, uint8_t o[2][32], int32_t mu_out[2][32])
{
    int mu[2][32], mu_min = 0, any = 0, O = 0;
    memset(mu, 0, sizeof(mu));
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            double Th = rd_lam(AT3P_PSY_ATH[qu]);
            for (int m = 0; m < 32; ++m) {
                if (AT3P_PSY_SPREAD[m][qu] > 63) continue;
                const double E = (double)dist[(ch * 32 + m) * 8] * rd_G(sfi[ch * 32 + m]);   /* M1: D[ch][m][0] */
                const double cast = E * rd_G(63 - AT3P_PSY_SPREAD[m][qu]);
                if (cast > Th) Th = cast;
            }
            int i = MU_HI;
            while (i > 0 && !(rd_lam(i) <= Th)) --i;   /* the largest i with lambda_i <= Th */
            mu[ch][qu] = i;
            if (dist[(ch * 32 + qu) * 8] > 0 && (!any || i < mu_min)) {
                mu_min = i;
                any = 1;
            }
        }
    memset(o, 0, 64);
    for (int ch = 0; ch < channels; ++ch)
        for (int qu = 0; qu < 32; ++qu) {
            if (dist[(ch * 32 + qu) * 8] > 0) o[ch][qu] = (uint8_t)(mu[ch][qu] - mu_min > O_MAX ? O_MAX : mu[ch][qu] - mu_min);
            if (o[ch][qu] > O) O = o[ch][qu];
        }
    if (mu_out) memcpy(mu_out, mu, sizeof(mu));
    return O;
}

/* R2, M4: the candidate R(j, k) or P(j, k); returns N, and in *took how many units took the j - 1 value */
static int rd_candidate(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, int channels, uint8_t (*o)[32], int j, int k, uint8_t wl[2][32],
                        int* took)
{
    memset(wl, 0, 64);
    int taken = 0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const int u = ch * 32 + qu, ju = j + (o ? o[ch][qu] : 0);
            const int w0 = rd_pick_w(dist + u * 8, bits + u * 8, sfi[u], ju), up = rd_pick_w(dist + u * 8, bits + u * 8, sfi[u], ju - 1);
            wl[ch][qu] = (uint8_t)w0;
            if (up > w0 && taken < k) {
                wl[ch][qu] = (uint8_t)up;
                ++taken;
            }
        }
    if (took) *took = taken;
    return close_sparse(wl, channels);
}

/* R4: T(X); M6: Tw(X), each term weighted by G[63 - o] */
static double rd_total(const uint8_t* sfi, const uint64_t* dist, int channels, uint8_t (*o)[32], uint8_t wl[2][32])
{
    double T = 0.0;
    for (int qu = 0; qu < 32; ++qu)
        for (int ch = 0; ch < channels; ++ch) {
            const double D = (double)dist[(ch * 32 + qu) * 8 + wl[ch][qu]] * rd_G(sfi[ch * 32 + qu]);
            if (o) {
                const double term = D * rd_G(63 - o[ch][qu]);
                T += term;
            } else {
                T += D;
            }
        }
    return T;
}

typedef struct {
    int32_t j, k, num_quant_units, bits;   /* j*, k* of R3 / M5; N and Bits of the allocation written */
    int32_t chose, t, k_sparse, O;         /* R4 / M6: 1 = R(j*, k*) or P(j*, k*), 0 = A(t*, k*); t*, k* of the sparse allocation; M3's O */
    double T, T_sparse;                    /* T of R4, Tw of M6 */
    uint8_t o[2][32];                      /* M3's offsets */
    int32_t mu[2][32];                     /* M2's indices (zero when the offsets were given) */
    frame_alloc used;
} at3prd_frame_info;                       /* O, o and mu are zero for R */

/* R2-R4 or M1-M6 on the tables against the budget 8 * frame_bytes - 3. offsets_in (optional) [channels][32]: P with these in place of
 * M1-M3's; else psy: P with M1-M3's; else R. Returns Bits of the allocation written. rec (optional): everything but num_quant_units,
 * bits and used is filled. */
int at3prd_allocate(const uint8_t* sfi, const uint16_t* bits, const uint64_t* dist, const uint8_t* offsets_in, int psy, int channels, int tail_bits,
                    int frame_bytes, uint8_t* wl_out, int32_t* n_units, void* rec)
{
    const int size_bits = 8 * frame_bytes - 3;
    uint8_t wl[2][32], wa[2][32], offs[2][32];
    uint8_t (*o)[32] = offsets_in || psy ? offs : NULL;
    int32_t mu[2][32];
    int O = 0;
    memset(mu, 0, sizeof(mu));
    memset(offs, 0, sizeof(offs));
    if (offsets_in) {
        memcpy(offs, offsets_in, (size_t)channels * 32);
        for (int i = 0; i < 32 * channels; ++i)
            if (offsets_in[i] > O) O = offsets_in[i];
    } else if (psy) {
        O = psy_offsets(sfi, dist, channels, offs, mu);
    }
    int js = J_MAX, ks = 0;
    for (int j = J_MIN - O; j <= J_MAX; ++j) {
        const int N = rd_candidate(sfi, bits, dist, channels, o, j, 0, wl, NULL);
        if (alloc_bits(bits, channels, tail_bits, wl, N, 1) <= size_bits) {
            js = j;
            break;
        }
    }
    for (int k = 0; k <= K_MAX; ++k) {
        const int N = rd_candidate(sfi, bits, dist, channels, o, js, k, wl, NULL);
        if (alloc_bits(bits, channels, tail_bits, wl, N, 1) <= size_bits) ks = k;
    }
    int N = rd_candidate(sfi, bits, dist, channels, o, js, ks, wl, &ks);
    int32_t Na, ta, ka;
    memset(wa, 0, sizeof(wa));
    at3pw_allocate(sfi, bits, channels, tail_bits, frame_bytes, 1, &wa[0][0], &Na, &ta, &ka);
    if (channels == 1) memset(wa[1], 0, 32);
    const double Tr = rd_total(sfi, dist, channels, o, wl), Ta = rd_total(sfi, dist, channels, o, wa);
    const int chose = Tr <= Ta;
    if (!chose) {
        memcpy(wl, wa, sizeof(wl));
        N = Na;
    }
    memcpy(wl_out, wl, (size_t)channels * 32);
    *n_units = N;
    if (rec) {
        at3prd_frame_info* r = (at3prd_frame_info*)rec;
        r->j = js;
        r->k = ks;
        r->chose = chose;
        r->t = ta;
        r->k_sparse = ka;
        r->O = O;
        r->T = Tr;
        r->T_sparse = Ta;
        memcpy(r->o, offs, sizeof(r->o));
        memcpy(r->mu, mu, sizeof(r->mu));
    }
    return alloc_bits(bits, channels, tail_bits, wl, N, 1);
}

/* A1, A2, R1, then R2-R4 or M1-M6 of one frame: the allocation of R4 or M6, then the frame (A6s) */
static void rd_write_frame(const float* specs, int channels, int frame_bytes, int psy, const uint8_t* tail, int tail_bits, uint8_t* out,
                           at3prd_frame_info* info)
{
    uint8_t sfi[2][32], tab[2][32][8], wl[2][32];
    uint16_t bits[2][32][8];
    uint64_t dist[2][32][8];
    float values[2][2048];
    at3prd_frame_info rec;
    memset(sfi, 0, sizeof(sfi));
    memset(tab, 0, sizeof(tab));
    memset(bits, 0, sizeof(bits));
    memset(dist, 0, sizeof(dist));
    memset(wl, 0, sizeof(wl));
    memset(&rec, 0, sizeof(rec));
    at3prd_tables(specs, channels, &sfi[0][0], &bits[0][0][0], &tab[0][0][0], &dist[0][0][0], &values[0][0]);
    int32_t N;
    rec.bits = at3prd_allocate(&sfi[0][0], &bits[0][0][0], &dist[0][0][0], NULL, psy, channels, tail_bits, frame_bytes, &wl[0][0], &N, &rec);
    rec.num_quant_units = N;
    if (channels == 1) memset(wl[1], 0, 32);
    emit_frame(out, frame_bytes, channels, 1, sfi, tab, wl, N, values, tail, tail_bits, &rec.used);
    if (info) *info = rec;
}

/* specs [n_frames][channels][2048], tails [n_frames][TAIL_BYTES], tail_bits [n_frames] -> out [n_frames][frame_bytes]; info optional */
int at3prd_write_frames(const float* specs, int channels, int n_frames, int frame_bytes, int psy, const uint8_t* tails, const int32_t* tail_bits,
                        uint8_t* out, void* info)
{
    if (channels < 1 || channels > 2 || frame_bytes < 8 || frame_bytes > MAX_FRAME_SZ || frame_bytes % 8) return -1;
    for (int f = 0; f < n_frames; ++f) {
        if (tail_bits[f] < 0 || tail_bits[f] > TAIL_BYTES * 8) return -1;
        rd_write_frame(specs + (size_t)f * channels * 2048, channels, frame_bytes, psy, tails + (size_t)f * TAIL_BYTES, tail_bits[f],
                       out + (size_t)f * frame_bytes, info ? (at3prd_frame_info*)info + f : NULL);
    }
    return n_frames;
}
int at3prd_frame_info_size(void) { return (int)sizeof(at3prd_frame_info); }
int at3prd_j_min(void) { return J_MIN; }
int at3prd_j_max(void) { return J_MAX; }
