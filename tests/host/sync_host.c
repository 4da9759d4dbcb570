/* Stand-alone driver of gnsscorr_sync_* for tests/test_sync_host.py: compiled together with csrc/sdr_sync.c alone (no
 * device library), also under -fsanitize=address,undefined.
 *   sync_host <script>
 * The script holds one operation per line; doubles are C99 hexadecimal floats:
 *   create <nch> <outms>
 *   chan <ch> <nsamp> <ctime> <ti>
 *   push <ch> <flagdec> <week> <firstsf> <firstsfcnt> <n>      followed by n lines  <tow> <remcout> <L> <D> <S> <codei> <cntout> <snr>
 *   detach <ch>
 *   flush
 * Every push hands the library a heap block of exactly its rows.  After every operation: "rc <code>", then the epoch rows
 * fetched (three at a time, through a heap block of exactly three) as "<ch> <week> <tow> <P> <L> <D> <S> <sampref>". */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gnsscorr.h"

static int drain(gnsscorr_sync_t *st)
{
    for (;;) {
        gnsscorr_epochobs_t *o = (gnsscorr_epochobs_t *)malloc(3 * sizeof(*o));
        if (!o) return 2;
        const int k = gnsscorr_sync_fetch(st, o, 3);
        for (int i = 0; i < k; i++)
            printf("%d %d %a %a %a %a %a %llu\n", o[i].ch, o[i].week, o[i].tow, o[i].P, o[i].L, o[i].D, o[i].S,
                   (unsigned long long)o[i].sampref);
        free(o);
        if (k < 0) return 4;
        if (k < 3) return 0;
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *fp = fopen(argv[1], "r");
    if (!fp) return 2;
    gnsscorr_sync_t *st = NULL;
    char op[16];

    /* the refusals that need no state, and those that must leave a state as it was */
    gnsscorr_syncframe_t fr0;
    gnsscorr_obsrow_t row0;
    memset(&fr0, 0, sizeof(fr0));
    memset(&row0, 0, sizeof(row0));
    if (gnsscorr_sync_create(NULL, 1, 10) != GNSSCORR_EINVAL || gnsscorr_sync_create(&st, 0, 10) != GNSSCORR_EINVAL ||
        gnsscorr_sync_create(&st, 1, 0) != GNSSCORR_EINVAL || st != NULL)
        return 3;
    if (gnsscorr_sync_channel(NULL, 0, 1, 1e-3, 1e-6) != GNSSCORR_EINVAL || gnsscorr_sync_push(NULL, 0, &fr0, &row0, 1) != GNSSCORR_EINVAL ||
        gnsscorr_sync_detach(NULL, 0) != GNSSCORR_EINVAL || gnsscorr_sync_flush(NULL) != GNSSCORR_EINVAL ||
        gnsscorr_sync_fetch(NULL, NULL, 0) != GNSSCORR_EINVAL)
        return 3;
    gnsscorr_sync_destroy(NULL);

    while (fscanf(fp, "%15s", op) == 1) {
        int rc = GNSSCORR_OK;
        if (!strcmp(op, "create")) {
            int nch, outms;
            if (fscanf(fp, "%d %d", &nch, &outms) != 2) return 2;
            gnsscorr_sync_destroy(st);
            st = NULL;
            rc = gnsscorr_sync_create(&st, nch, outms);
        } else if (!strcmp(op, "chan")) {
            int ch, nsamp;
            double ctime, ti;
            if (fscanf(fp, "%d %d %la %la", &ch, &nsamp, &ctime, &ti) != 4) return 2;
            rc = gnsscorr_sync_channel(st, ch, nsamp, ctime, ti);
        } else if (!strcmp(op, "push")) {
            int ch, n;
            unsigned long long sf, sfcnt;
            gnsscorr_syncframe_t fr;
            memset(&fr, 0, sizeof(fr));
            if (fscanf(fp, "%d %d %d %llu %llu %d", &ch, &fr.flagdec, &fr.week, &sf, &sfcnt, &n) != 6 || n < 0) return 2;
            fr.firstsf = sf;
            fr.firstsfcnt = sfcnt;
            gnsscorr_obsrow_t *rows = (gnsscorr_obsrow_t *)calloc((size_t)n, sizeof(*rows));
            if (n && !rows) return 2;
            for (int i = 0; i < n; i++) {
                unsigned long long codei, cntout;
                if (fscanf(fp, "%la %la %la %la %la %llu %llu %d", &rows[i].tow, &rows[i].remcout, &rows[i].L, &rows[i].D, &rows[i].S,
                           &codei, &cntout, &rows[i].snr) != 8)
                    return 2;
                rows[i].codei = codei;
                rows[i].cntout = cntout;
            }
            gnsscorr_syncframe_t *frp = (gnsscorr_syncframe_t *)malloc(sizeof(fr));
            if (!frp) return 2;
            *frp = fr;
            rc = gnsscorr_sync_push(st, ch, frp, n ? rows : &row0, n);
            free(frp);
            free(rows);
        } else if (!strcmp(op, "detach")) {
            int ch;
            if (fscanf(fp, "%d", &ch) != 1) return 2;
            rc = gnsscorr_sync_detach(st, ch);
        } else if (!strcmp(op, "flush")) {
            rc = gnsscorr_sync_flush(st);
        } else
            return 2;
        printf("rc %d\n", rc);
        if (rc && !gnsscorr_sync_last_error()[0]) return 3;
        if (st) {
            const int d = drain(st);
            if (d) return d;
        }
    }
    fclose(fp);
    gnsscorr_sync_destroy(st);
    return 0;
}
