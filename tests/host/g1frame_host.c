/* Stand-alone driver of gnsscorr_g1frame_replay for tests/test_g1frame_host.py: compiled together with csrc/sdr_g1.c
 * alone (no device library), usually under -fsanitize=address,undefined.
 *   g1frame_host <file> <cnt0> <piece> [<zero_ephcnt_at_row>]
 * <file> holds one signed byte per log row, the row's navbit; buffloc of a row is 1000 * cnt.  The rows are replayed in
 * pieces of <piece> rows, each piece from a heap block of exactly its size; a piece that begins at row
 * <zero_ephcnt_at_row> is preceded by the caller's ephcnt = 0.  After every piece one line with every state field. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gnsscorr.h"

static void show(const gnsscorr_g1frame_t *s, long row)
{
    printf("%ld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %llu %llu %.17g %.17g ", row, s->polarity, s->flagsyncf,
           s->flagtow, s->flagdec, s->id, s->ephcnt, s->s1cnt, s->tk[0], s->tk[1], s->tk[2], s->nt, s->slot, s->n4, s->iode,
           s->update, s->week, (unsigned long long)s->firstsf, (unsigned long long)s->firstsfcnt, s->firstsftow, s->tow_gpst);
    for (int i = 0; i < 11; i++) printf("%02x", s->str[i]);
    printf(" ");
    for (int i = 0; i < 200; i++) putchar(s->fbits[i] > 0 ? '+' : s->fbits[i] < 0 ? '-' : '0');
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    const unsigned long long cnt0 = strtoull(argv[2], NULL, 10);
    const long piece = atol(argv[3]), zero_at = argc > 4 ? atol(argv[4]) : -1;
    if (piece < 1) return 2;
    fseek(fp, 0, SEEK_END);
    const long n = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    signed char *bits = (signed char *)malloc((size_t)n + 1);
    if (!bits || fread(bits, 1, (size_t)n, fp) != (size_t)n) return 2;
    fclose(fp);

    gnsscorr_g1frame_t st, same;
    memset(&st, 0, sizeof(st));
    /* the error paths touch nothing */
    memset(&same, 0x5a, sizeof(same));
    gnsscorr_trklog_t one;
    memset(&one, 0, sizeof(one));
    if (gnsscorr_g1frame_replay(NULL, &one, 1, 0) != GNSSCORR_EINVAL || gnsscorr_g1frame_replay(&same, NULL, 1, 0) != GNSSCORR_EINVAL ||
        gnsscorr_g1frame_replay(&same, &one, -1, 0) != GNSSCORR_EINVAL)
        return 3;
    for (size_t i = 0; i < sizeof(same); i++)
        if (((unsigned char *)&same)[i] != 0x5a) return 3;
    if (gnsscorr_g1frame_replay(&st, &one, 0, 0) != GNSSCORR_OK) return 3;

    for (long r0 = 0; r0 < n; r0 += piece) {
        const long m = n - r0 < piece ? n - r0 : piece;
        gnsscorr_trklog_t *log = (gnsscorr_trklog_t *)calloc((size_t)m, sizeof(*log));
        if (!log) return 2;
        for (long i = 0; i < m; i++) {
            log[i].navbit = bits[r0 + i];
            log[i].buffloc = 1000ull * (cnt0 + (unsigned long long)(r0 + i));
        }
        if (r0 == zero_at) st.ephcnt = 0;
        if (gnsscorr_g1frame_replay(&st, log, (int)m, cnt0 + (unsigned long long)r0) != GNSSCORR_OK) return 4;
        free(log);
        show(&st, r0 + m);
    }
    free(bits);
    return 0;
}
