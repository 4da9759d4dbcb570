/* One K = 7, rate-1/2 Viterbi decode of an SBAS frame buffer (1512 symbols -> 750 bits) as DESIGN.md 3.5 defines it,
 * plain single-thread C: the host cost tools/fec_time.py compares the device decoder with.  Not part of the library.
 *   gcc -O2 -o fec_ref tools/fec_ref.c && ./fec_ref [decodes]      prints "<ns per decode> <checksum>" */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#define WIN  1512
#define NDEC 750

static int parity(unsigned x) { return __builtin_popcount(x) & 1; }

static void decode(const signed char *fbits, unsigned polyA, unsigned polyB, unsigned char *out)
{
    static uint64_t dec[WIN / 2];
    uint32_t m[64], mn[64];
    unsigned eA0[64], eB0[64], eA1[64], eB1[64];    /* expected symbols of the two branches into state s */
    for (unsigned s = 0; s < 64; s++) {
        m[s] = s ? 63 : 0;
        eA0[s] = 255u * parity(s & polyA);
        eB0[s] = 255u * parity(s & polyB);
        eA1[s] = 255u * parity((s | 64) & polyA);
        eB1[s] = 255u * parity((s | 64) & polyB);
    }
    for (int t = 0; t < WIN / 2; t++) {
        const unsigned ra = fbits[2 * t] == 1 ? 0 : 255, rb = fbits[2 * t + 1] == 1 ? 0 : 255;
        uint64_t word = 0;
        for (unsigned s = 0; s < 64; s++) {
            const uint32_t m0 = m[s >> 1] + (eA0[s] ^ ra) + (eB0[s] ^ rb);
            const uint32_t m1 = m[(s >> 1) + 32] + (eA1[s] ^ ra) + (eB1[s] ^ rb);
            const int d = (int32_t)(m0 - m1) > 0;
            mn[s] = d ? m1 : m0;
            word |= (uint64_t)d << s;
        }
        dec[t] = word;
        for (int s = 0; s < 64; s++) m[s] = mn[s];
    }
    unsigned st = 0;
    for (int i = 0; i < (NDEC + 7) / 8; i++) out[i] = 0;
    for (int t = WIN / 2 - 1; t >= 0; t--) {
        if (t < NDEC) out[t >> 3] |= (unsigned char)((st & 1) << (7 - (t & 7)));
        st = (st >> 1) | ((unsigned)((dec[t] >> st) & 1) << 5);
    }
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 400;
    static signed char sym[WIN + 4096];
    unsigned char out[96];
    unsigned seed = 12345, sum = 0;
    for (int i = 0; i < WIN + 4096; i++) {
        seed = seed * 1664525u + 1013904223u;
        sym[i] = (seed >> 16) & 1 ? 1 : -1;
    }
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int k = 0; k < n; k++) {
        decode(sym + (k & 4095), 0x6d, 0x4f, out);
        sum += out[k % 94];
    }
    clock_gettime(CLOCK_MONOTONIC, &b);
    printf("%.1f %u\n", ((b.tv_sec - a.tv_sec) * 1e9 + (b.tv_nsec - a.tv_nsec)) / n, sum);
    return 0;
}
