/* Stand-alone driver of gnsscorr_rxnav_* for tests/test_rxnav_host.py: compiled together with csrc/sdr_rxnav.c,
 * sdr_host.c, sdr_g1.c and sdr_sync.c (no device library; the six device entry points sdr_host.c refers to are stubs
 * here that answer an error), once plain and once under -fsanitize=address,undefined.
 *   rxnav_host <script>
 * The script, one command per line (doubles as C99 hex floats):
 *   create <nch> <outms> <hold_steps>     followed by nch lines: ctype nsamp loopms f_sf f_if foffset ctime ti oldremcode
 *   week <ch> <week>
 *   feed <stride>                         followed by nch lines: ndone cnt_after tracking, each followed by its ndone rows:
 *                                         carrfreq codefreq remcode remcarr buffloc currnsamp flagloopfilter flagsync navbit II0
 *   flush | fetch | status | frame <ch> | destroy
 * Every command prints "rc <code>"; a feed then prints the rows it made ("row <ch> ..."), fetch the epochs ("epo ..."),
 * status one line per channel ("st ..."), frame the state's bytes in hex ("fr <ch> <hex>").  The arrays of a feed are heap
 * blocks of exactly nch * stride elements.  Before the script the error paths run on objects of their own. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gnsscorr.h"

/* the device entry points csrc/sdr_host.c refers to: none of them is reached from here */
void gc_compat_forget(void *sdr) { (void)sdr; }
gnsscorr_ctx *gnsscorr_default_ctx(void) { return NULL; }
const char *gnsscorr_last_error(void) { return "no device library"; }
int gnsscorr_ring_create(gnsscorr_ctx *ctx, int ftype, int dtype, uint64_t ringlen, void *devmem)
{
    (void)ctx; (void)ftype; (void)dtype; (void)ringlen; (void)devmem;
    return GNSSCORR_EHIP;
}
int gnsscorr_ring_push(gnsscorr_ctx *ctx, int ftype, const void *host, uint64_t nsamp)
{
    (void)ctx; (void)ftype; (void)host; (void)nsamp;
    return GNSSCORR_EHIP;
}
int gnsscorr_fec_run(gnsscorr_ctx *ctx, const signed char *sym, int nch, int nsym, int pos0, int npos, int stride, int win,
                     int ndec, int polyA, int polyB, unsigned char *out, int rowbytes)
{
    (void)ctx; (void)sym; (void)nch; (void)nsym; (void)pos0; (void)npos; (void)stride; (void)win; (void)ndec; (void)polyA;
    (void)polyB; (void)out; (void)rowbytes;
    return GNSSCORR_EHIP;
}

#define CT_L1CA 1
#define CT_SBAS 27
#define CT_G1   20

static gnsscorr_rxnavch_t chan_of(int ctype, double f_sf)
{
    gnsscorr_rxnavch_t c;
    memset(&c, 0, sizeof(c));
    c.ctype = ctype;
    c.nsamp = 4092;
    c.loopms = 10;
    c.f_sf = f_sf;
    c.ctime = 1e-3;
    c.ti = 1.0 / f_sf;
    return c;
}

static int same_status(gnsscorr_rxnav_t *nv, const gnsscorr_rxnavstat_t *before, int nch)
{
    gnsscorr_rxnavstat_t now[4];
    if (gnsscorr_rxnav_status(nv, now) != GNSSCORR_OK) return 0;
    return memcmp(now, before, sizeof(now[0]) * (size_t)nch) == 0;
}

/* the refusals, each on state of its own; returns 0 when every one answers as the header says */
static int error_paths(void)
{
    gnsscorr_rxnav_t *nv = NULL;
    gnsscorr_rxnavch_t ch[2] = {chan_of(CT_L1CA, 4.092e6), chan_of(CT_SBAS, 4.092e6)};
    if (gnsscorr_rxnav_create(NULL, 2, ch, 10, 0) != GNSSCORR_EINVAL || gnsscorr_rxnav_create(&nv, 0, ch, 10, 0) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_create(&nv, 2, NULL, 10, 0) != GNSSCORR_EINVAL || gnsscorr_rxnav_create(&nv, 2, ch, 10, -1) != GNSSCORR_EINVAL)
        return 1;
    ch[1].ctype = 5;                                            /* a code type outside the three */
    if (gnsscorr_rxnav_create(&nv, 2, ch, 10, 0) != GNSSCORR_EINVAL || nv) return 2;
    ch[1] = chan_of(CT_G1, 4.0e6);                              /* another ti: the sync's refusal, with its message */
    if (gnsscorr_rxnav_create(&nv, 2, ch, 10, 0) != GNSSCORR_EINVAL || nv || !strstr(gnsscorr_rxnav_last_error(), gnsscorr_sync_last_error()))
        return 3;
    if (gnsscorr_rxnav_create(&nv, 2, ch, 0, 0) != GNSSCORR_EINVAL || nv) return 4;      /* outms */
    ch[1] = chan_of(CT_SBAS, 4.092e6);
    if (gnsscorr_rxnav_create(&nv, 2, ch, 10, 1) != GNSSCORR_OK || !nv) return 5;
    const int stride = 40;
    gnsscorr_trklog_t *log = calloc(2 * (size_t)stride, sizeof(*log));
    double *ii = calloc(2 * (size_t)stride, sizeof(*ii));
    if (!log || !ii) return 6;
    for (int k = 0; k < 2; k++)
        for (int p = 0; p < stride; p++) {
            log[k * stride + p].buffloc = 1000 + 4092ull * (unsigned)p + (unsigned)k;
            log[k * stride + p].currnsamp = 4092;
            log[k * stride + p].codefreq = 1.023e6;
            log[k * stride + p].flagloopfilter = p % 10 == 9 ? 2 : 0;
        }
    int ndone[2] = {40, 0}, tracking[2] = {1, 1};
    uint64_t cnt[2] = {40, 0};
    gnsscorr_rxnavstat_t st[4];
    memset(st, 0, sizeof(st));
    /* an SBAS channel without a context, NULL pointers, bad counts: nothing touched */
    if (gnsscorr_rxnav_status(nv, st) != GNSSCORR_OK) return 7;
    if (gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_EINVAL || !same_status(nv, st, 2)) return 8;
    gnsscorr_rxnav_destroy(nv);
    nv = NULL;
    ch[1] = chan_of(CT_G1, 4.092e6);
    if (gnsscorr_rxnav_create(&nv, 2, ch, 10, 1) != GNSSCORR_OK) return 9;
    if (gnsscorr_rxnav_feed(NULL, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, NULL, ii, stride, ndone, cnt, tracking) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, log, NULL, stride, ndone, cnt, tracking) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, NULL, cnt, tracking) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, NULL, tracking) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, NULL) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_feed(nv, NULL, log, ii, stride - 1, ndone, cnt, tracking) != GNSSCORR_EINVAL)
        return 10;
    ndone[1] = -1;
    if (gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_EINVAL) return 11;
    ndone[1] = 0;
    if (gnsscorr_rxnav_status(nv, st) != GNSSCORR_OK || st[0].cnt != 0 || st[0].nrows != 0) return 12;
    if (gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_OK) return 13;
    if (gnsscorr_rxnav_status(nv, st) != GNSSCORR_OK || st[0].cnt != 40 || st[0].nrows != 4 || !st[0].attached) return 14;
    /* a gap in cnt: GNSSCORR_ESTATE naming the channel, every state as it was */
    cnt[0] = 90;
    if (gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_ESTATE || !same_status(nv, st, 2) ||
        !strstr(gnsscorr_rxnav_last_error(), "channel 0"))
        return 15;
    /* a wrong size, a channel out of range */
    gnsscorr_frame_t fr;
    gnsscorr_g1frame_t g1;
    if (gnsscorr_rxnav_frame(nv, 0, &fr, sizeof(fr) - 1) != GNSSCORR_EINVAL || gnsscorr_rxnav_frame(nv, 0, &g1, sizeof(g1)) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_frame(nv, 2, &fr, sizeof(fr)) != GNSSCORR_EINVAL || gnsscorr_rxnav_frame(nv, 0, &fr, sizeof(fr)) != GNSSCORR_OK ||
        gnsscorr_rxnav_frame(nv, 1, &g1, sizeof(g1)) != GNSSCORR_OK)
        return 16;
    if (gnsscorr_rxnav_week(nv, 1, 2262) != GNSSCORR_EINVAL || gnsscorr_rxnav_week(nv, -1, 2262) != GNSSCORR_EINVAL ||
        gnsscorr_rxnav_week(nv, 0, 2262) != GNSSCORR_OK)
        return 17;
    gnsscorr_obsrow_t rows[4];
    if (gnsscorr_rxnav_rows(nv, 0, rows, 2) != 2 || gnsscorr_rxnav_rows(nv, 0, rows, 4) != 4 || gnsscorr_rxnav_rows(nv, 1, rows, 4) != 0 ||
        gnsscorr_rxnav_rows(nv, 2, rows, 4) != GNSSCORR_EINVAL || rows[3].cntout != 39)
        return 18;
    /* tracking 0 zeroes, detaches and counts one reset; hold_steps 1 detaches channel 0 after one starved feed */
    tracking[0] = 0;
    ndone[0] = 0;
    cnt[0] = 40;
    if (gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking) != GNSSCORR_OK || gnsscorr_rxnav_status(nv, st) != GNSSCORR_OK ||
        st[0].resets != 1 || st[0].attached || st[0].nrows != 0)
        return 19;
    gnsscorr_epochobs_t epo[1];
    if (gnsscorr_rxnav_flush(nv) != GNSSCORR_OK || gnsscorr_rxnav_fetch(nv, epo, 1) != 0) return 20;
    gnsscorr_rxnav_destroy(nv);
    gnsscorr_rxnav_destroy(NULL);
    free(log);
    free(ii);
    return 0;
}

static void hex(const void *p, size_t n)
{
    for (size_t i = 0; i < n; i++) printf("%02x", ((const unsigned char *)p)[i]);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    const int bad = error_paths();
    if (bad) {
        fprintf(stderr, "error path %d: %s\n", bad, gnsscorr_rxnav_last_error());
        return 3;
    }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) return 2;
    gnsscorr_rxnav_t *nv = NULL;
    int nch = 0, ctype[64];
    char cmd[32];
    while (fscanf(fp, "%31s", cmd) == 1) {
        if (!strcmp(cmd, "create")) {
            int outms, hold;
            if (fscanf(fp, "%d %d %d", &nch, &outms, &hold) != 3 || nch < 1 || nch > 64) return 2;
            gnsscorr_rxnavch_t *ch = calloc((size_t)nch, sizeof(*ch));
            if (!ch) return 2;
            for (int k = 0; k < nch; k++) {
                if (fscanf(fp, "%d %d %d %la %la %la %la %la %la", &ch[k].ctype, &ch[k].nsamp, &ch[k].loopms, &ch[k].f_sf, &ch[k].f_if,
                           &ch[k].foffset, &ch[k].ctime, &ch[k].ti, &ch[k].oldremcode) != 9)
                    return 2;
                ctype[k] = ch[k].ctype;
            }
            printf("rc %d\n", gnsscorr_rxnav_create(&nv, nch, ch, outms, hold));
            free(ch);
        } else if (!strcmp(cmd, "week")) {
            int k, w;
            if (fscanf(fp, "%d %d", &k, &w) != 2) return 2;
            printf("rc %d\n", gnsscorr_rxnav_week(nv, k, w));
        } else if (!strcmp(cmd, "feed")) {
            int stride;
            if (fscanf(fp, "%d", &stride) != 1 || stride < 1) return 2;
            gnsscorr_trklog_t *log = calloc((size_t)nch * (size_t)stride, sizeof(*log));
            double *ii = calloc((size_t)nch * (size_t)stride, sizeof(*ii));
            int *ndone = calloc((size_t)nch, sizeof(int)), *tracking = calloc((size_t)nch, sizeof(int));
            uint64_t *cnt = calloc((size_t)nch, sizeof(*cnt));
            if (!log || !ii || !ndone || !tracking || !cnt) return 2;
            for (int k = 0; k < nch; k++) {
                unsigned long long c;
                if (fscanf(fp, "%d %llu %d", &ndone[k], &c, &tracking[k]) != 3 || ndone[k] > stride) return 2;
                cnt[k] = c;
                for (int p = 0; p < ndone[k]; p++) {
                    gnsscorr_trklog_t *r = &log[(size_t)k * (size_t)stride + (size_t)p];
                    unsigned long long b;
                    if (fscanf(fp, "%la %la %la %la %llu %d %d %d %d %la", &r->carrfreq, &r->codefreq, &r->remcode, &r->remcarr, &b,
                               &r->currnsamp, &r->flagloopfilter, &r->flagsync, &r->navbit, &ii[(size_t)k * (size_t)stride + (size_t)p]) != 10)
                        return 2;
                    r->buffloc = b;
                }
            }
            printf("rc %d\n", gnsscorr_rxnav_feed(nv, NULL, log, ii, stride, ndone, cnt, tracking));
            for (int k = 0; k < nch; k++) {
                gnsscorr_obsrow_t *rows = calloc((size_t)stride, sizeof(*rows));
                if (!rows) return 2;
                const int n = gnsscorr_rxnav_rows(nv, k, rows, stride);
                for (int i = 0; i < n; i++)
                    printf("row %d %a %a %a %a %a %llu %llu %d\n", k, rows[i].tow, rows[i].remcout, rows[i].L, rows[i].D, rows[i].S,
                           (unsigned long long)rows[i].codei, (unsigned long long)rows[i].cntout, rows[i].snr);
                free(rows);
            }
            free(log); free(ii); free(ndone); free(tracking); free(cnt);
        } else if (!strcmp(cmd, "flush")) {
            printf("rc %d\n", gnsscorr_rxnav_flush(nv));
        } else if (!strcmp(cmd, "fetch")) {
            gnsscorr_epochobs_t e[64];
            int m, rc = 0;
            while ((m = gnsscorr_rxnav_fetch(nv, e, 64)) > 0)
                for (int i = 0; i < m; i++)
                    printf("epo %d %d %a %a %a %a %a %llu\n", e[i].ch, e[i].week, e[i].tow, e[i].P, e[i].L, e[i].D, e[i].S,
                           (unsigned long long)e[i].sampref);
            if (m < 0) rc = m;
            printf("rc %d\n", rc);
        } else if (!strcmp(cmd, "status")) {
            gnsscorr_rxnavstat_t *st = calloc((size_t)nch, sizeof(*st));
            if (!st) return 2;
            printf("rc %d\n", gnsscorr_rxnav_status(nv, st));
            for (int k = 0; k < nch; k++)
                printf("st %d %d %d %d %d %d %d %d %llu %llu %llu %llu %a %a\n", st[k].ctype, st[k].attached, st[k].flagsyncf, st[k].flagdec,
                       st[k].polarity, st[k].week, st[k].id, st[k].resets, (unsigned long long)st[k].cnt, (unsigned long long)st[k].firstsf,
                       (unsigned long long)st[k].firstsfcnt, (unsigned long long)st[k].nrows, st[k].firstsftow, st[k].tow);
            free(st);
        } else if (!strcmp(cmd, "frame")) {
            int k;
            if (fscanf(fp, "%d", &k) != 1 || k < 0 || k >= nch) return 2;
            const size_t size = ctype[k] == CT_L1CA ? sizeof(gnsscorr_frame_t) : ctype[k] == CT_G1 ? sizeof(gnsscorr_g1frame_t) : sizeof(gnsscorr_sbasframe_t);
            void *s = malloc(size);
            if (!s) return 2;
            printf("rc %d\n", gnsscorr_rxnav_frame(nv, k, s, size));
            printf("fr %d ", k);
            hex(s, size);
            printf("\n");
            free(s);
        } else if (!strcmp(cmd, "destroy")) {
            gnsscorr_rxnav_destroy(nv);
            nv = NULL;
            printf("rc 0\n");
        } else {
            return 2;
        }
    }
    fclose(fp);
    gnsscorr_rxnav_destroy(nv);
    return 0;
}
