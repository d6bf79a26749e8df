/* Check behind recip_rn / div_by_recip / share_window (dgen_amd/csrc/dgen_hip.hip):
 * the tiered bills' period shares u_p / U formed from one reciprocal of U.
 *
 *   y  = seed ~ 1/U (the hardware reciprocal: 24-26 good bits)
 *   3 x { e = fma(-U, y, 1); y = fma(y, e, y); }      -> y = RN(1/U)
 *   q0 = u * y;  r = fma(-U, q0, u);  q = fma(r, y, q0) -> q = RN(u/U)
 *
 * The functions below restate the device code with fma(); the seed is a
 * parameter, so the check runs over the documented error of the hardware's
 * reciprocal: 1/U cut to 24, 25 and 26 significant bits, and that value one
 * unit of its last kept bit down and up (9 seeds).  Inside the window the
 * result must equal u / U bit for bit; outside it the helper must decline
 * (the caller then divides).  Prints the number of mismatches, the number of
 * window mistakes and the number of pairs checked; "0 0 N" is the pass. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#define PREG 4

static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

/* the device's share_window, test for test */
static int share_window(double U, const double* u) {
    uint32_t hmax = (uint32_t)(bits(U) >> 32);
    int emin = 0;
    for (int p = 0; p < PREG; p++) {
        const uint32_t h = (uint32_t)(bits(u[p]) >> 32);
        int e = 0;
        if (u[p] == u[p] && !isinf(u[p])) (void)frexp(u[p], &e);   /* v_frexp_exp_i32_f64: 0 for 0, inf, nan */
        if (h > hmax) hmax = h;
        if (e < emin) emin = e;
    }
    return U >= 0x1p-256 && hmax < 0x4FF00000u && emin >= -255 && (uint32_t)bits(U) != 0xFFFFFFFFu;
}

static double recip_rn(double U, double seed) {
    double y = seed;
    for (int k = 0; k < 3; k++) {
        const double e = fma(-U, y, 1.0);
        y = fma(y, e, y);
    }
    return y;
}

static double div_by_recip(double u, double U, double y) {
    const double q0 = u * y;
    const double r = fma(-U, q0, u);
    return fma(r, y, q0);
}

/* 1/U cut to `keep` significant bits, moved d units of the last kept bit */
static double seed_of(double U, int keep, int d) {
    const uint64_t b = bits(1.0 / U);
    const int drop = 53 - keep;
    uint64_t m = (b >> drop) + (uint64_t)(int64_t)d;   /* a carry into the exponent is the next binade */
    return from_bits(m << drop);
}

static uint64_t rng_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void) {   /* splitmix64 */
    uint64_t z = (rng_s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double mk(int e, uint64_t mant) { return from_bits(((uint64_t)(e + 1023) << 52) | (mant & 0xFFFFFFFFFFFFFull)); }

static long bad = 0, wbad = 0, total = 0;

/* one pair with one seed: in the window the helper equals u / U, and the
 * window says what the caller expects of it */
static void pair1(double u, double U, int keep, int d, int want_fast) {
    double uu[PREG] = {u, 0.0, 0.0, 0.0};
    const int fast = share_window(U, uu);
    total++;
    if (want_fast >= 0 && fast != want_fast) wbad++;
    if (!fast) return;                       /* the caller divides */
    const double q = div_by_recip(u, U, recip_rn(U, seed_of(U, keep, d)));
    if (bits(q) != bits(u / U)) bad++;
}
static void pair(double u, double U, int want_fast) {
    for (int keep = 24; keep <= 26; keep++)
        for (int d = -1; d <= 1; d++) pair1(u, U, keep, d, want_fast);
}

int main(int argc, char** argv) {
    long nrand = 36000000;
    if (argc > 1) sscanf(argv[1], "%ld", &nrand);
    const uint64_t ONES = 0xFFFFFFFFFFFFFull;

    /* random pairs over the whole accepted band; the seed rotates */
    for (long i = 0; i < nrand; i++) {
        const uint64_t a = rnd(), b = rnd(), c = rnd();
        const int eU = (int)(a % 512) - 256;                     /* 2^-256 <= U < 2^256 */
        double U = mk(eU, b);
        if ((uint32_t)bits(U) == 0xFFFFFFFFu) U = mk(eU, b ^ 1);
        double u;
        switch ((a >> 16) & 7) {
        case 0: case 1: case 2: case 3:                           /* a share of U */
            u = U * ((double)(c >> 11) * 0x1p-53);
            break;
        case 4: case 5: {                                         /* any exponent of the band at or below U's */
            const int eu = -256 + (int)((c >> 52) % (uint64_t)(eU + 257));
            u = mk(eu, c);
            if (u > U) u = U;
            break;
        }
        case 6:                                                   /* within a few ulps below U */
            u = from_bits(bits(U) - (c & 7));
            break;
        default:                                                  /* anywhere in the band (u may exceed U) */
            u = mk((int)((c >> 52) % 512) - 256, c);
            break;
        }
        if (u != 0.0 && u < 0x1p-256) u = 0.0;
        const int k = (int)((a >> 32) % 9);
        pair1(u, U, 24 + k / 3, k % 3 - 1, 1);
    }

    /* u = 0, u = U, u one ulp below U; significands of all ones but one bit,
     * powers of two, and their neighbours, at every exponent of the band */
    for (int e = -256; e < 256; e++) {
        const uint64_t ms[] = {0, 1, 2, ONES - 1, ONES - 2, ONES ^ (1ull << 51), ONES ^ (1ull << 32),
                               ONES ^ (1ull << 31), 0x8000000000000ull, 0x7FFFFFFFFFFFFull, 0xFFFFF00000000ull,
                               0x00000FFFFFFFEull, rnd() & ~1ull, rnd() | 0x100000000ull};
        for (unsigned j = 0; j < sizeof ms / sizeof *ms; j++) {
            const double U = mk(e, ms[j]);
            if ((uint32_t)bits(U) == 0xFFFFFFFFu) continue;
            pair(0.0, U, 1);
            pair(U, U, 1);
            if (bits(U) - 1 >= bits(0x1p-256)) pair(from_bits(bits(U) - 1), U, 1);
            pair(mk(e, 0) > U ? U : mk(e, 0), U, 1);
            pair(mk(-256, ms[j]) > U ? U : mk(-256, ms[j]), U, 1);           /* the smallest accepted u's */
            pair(mk(-256, 0), U, 1);
            pair(mk(255, ONES), U, 1);                                       /* the largest accepted u */
            for (int k = 0; k < 8; k++) {
                const double u = U * ((double)(rnd() >> 11) * 0x1p-53);
                pair(u != 0.0 && u < 0x1p-256 ? 0.0 : u, U, 1);
            }
        }
        /* significand of all ones (the reciprocal theorem's exception) and
         * every other U whose low word is all ones: the helper declines */
        pair(mk(e, 0x123), mk(e, ONES), 0);
        pair(0.0, mk(e, ONES), 0);
        pair(mk(e, 0), mk(e, 0xABCDEFFFFFFFFull), 0);
    }

    /* the edges of the window, inside */
    pair(0x1p-256, 0x1p-256, 1);
    pair(0.0, 0x1p-256, 1);
    pair(0x1p-256, mk(255, ONES - 1), 1);
    pair(mk(255, ONES - 1), mk(255, ONES - 1), 1);
    pair(mk(255, ONES), 0x1p-256, 1);
    /* just outside: the helper declines */
    pair(0.0, from_bits(bits(0x1p-256) - 2), 0);                 /* U below the band */
    pair(0x1p-300, 0x1p-257, 0);
    pair(1.0, 0x1p256, 0);                                       /* U above the band */
    pair(1.0, 0x1p1023, 0);
    pair(from_bits(bits(0x1p-256) - 1), 1.0, 0);                 /* a non-zero u below the band */
    pair(0x1p-1000, 1.0, 0);
    pair(0x1p-1022, 1.0, 0);
    pair(0x1p-1074, 1.0, 0);                                     /* subnormal u */
    pair(from_bits(0x00000000FFFFFFFFull), 1.0, 0);              /* subnormal, high word 0 */
    pair(0x1p256, 1.0, 0);                                       /* u above the band */
    pair(-0.0, 1.0, 0);                                          /* signed zero: u / U is -0 */
    pair(-1.0, 2.0, 0);
    pair(INFINITY, 1.0, 0);
    pair(NAN, 1.0, 0);
    pair(1.0, 0.0, 0);
    pair(1.0, -1.0, 0);
    pair(1.0, INFINITY, 0);
    pair(1.0, NAN, 0);
    pair(0.0, 0x1p-1060, 0);

    /* the other registers of a month count too: one bad u declines for all */
    {
        double uu[PREG] = {1.0, 0.5, 0x1p-300, 0.0};
        total++;
        if (share_window(2.0, uu)) wbad++;
        uu[2] = 0x1p-256;
        total++;
        if (!share_window(2.0, uu)) wbad++;
        uu[3] = -0.0;
        total++;
        if (share_window(2.0, uu)) wbad++;
    }

    printf("%ld %ld %ld\n", bad, wbad, total);
    return bad || wbad ? 1 : 0;
}
