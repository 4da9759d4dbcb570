/*
 * sdr_sync.c -- observation epochs: what the body of syncthread()'s loop does (ref src/sdrsync.c:49-121) with interp1()
 * and uint64todouble() (ref src/sdrcmn.c:505-565), replayed over the rows gnsscorr_obs_replay gives each channel.  One
 * row per channel and loopms periods: scalar host work (DESIGN.md sections 3.8 and 7).  Plain C with no device and no
 * dependence on the rest of the library: a stand-alone program can compile and link this file alone
 * (tests/host/sync_host.c does).  Each function cites the reference routine whose behaviour it reproduces
 * ("ref <file>:<line>"); the reference's quirks that are kept are lettered as in DESIGN.md section 3.8.
 */
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gnsscorr.h"

#define NH        GNSSCORR_OBSHIST
#define CLIGHT    299792458.0           /* ref src/sdr.h:107 */
#define WEEKSEC   (3600 * 24 * 7)       /* ref src/sdrsync.c:66 */

typedef struct {
    gnsscorr_obsrow_t row;
    gnsscorr_syncframe_t fr;
} sync_item_t;

typedef struct {
    int      configured, attached, eligible;
    int      nsamp;                     /* ref sdrch_t.nsamp / .ctime / .ti */
    double   ctime, ti;
    /* ref sdrtrk_t.tow / .codei / .cntout / .remcout / .L / .D, newest first, and S[0] */
    double   tow[NH], remcout[NH], L[NH], D[NH], S0;
    uint64_t codei[NH], cntout[NH];
    /* of the row consumed last: ref sdreph_t.week_gpst, sdrnav_t.firstsf / .firstsfcnt */
    int      week;
    uint64_t firstsf, firstsfcnt;
    /* rows that wait: q[head .. head + len) */
    sync_item_t *q;
    int      head, len, cap;
    int      have_last;
    uint64_t lastcodei;                 /* codei of the row pushed last */
} sync_chan_t;

struct gnsscorr_sync {
    int      nch, outms;
    double   reftow;                    /* of the pass before (ref src/sdrsync.c:65) */
    int     *ind;                       /* [nch], by position in the eligible list: quirk (a) */
    int     *isat;                      /* [nch] scratch: the eligible list */
    sync_chan_t *chan;
    gnsscorr_epochobs_t *out;           /* epochs not fetched yet: out[ohead .. ohead + olen) */
    size_t   ohead, olen, ocap;
};

static _Thread_local char g_sync_err[160] = "";

static int sync_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_sync_err, sizeof(g_sync_err), fmt, ap);
    va_end(ap);
    return code;
}

const char *gnsscorr_sync_last_error(void) { return g_sync_err; }

/* interp1() for the n = 80 this file calls it with (ref src/sdrcmn.c:505-552), quirk (e): abscissae that descend from
 * first to last are reversed, whatever lies between; t at or outside the second / last-but-one abscissa takes the three
 * points of that end, otherwise a bisection on "t < xx[i-1]" brackets t and the neighbour on the nearer side joins; then
 * the Lagrange polynomial through the three points, factor by factor in the reference's order.  Unfilled history
 * elements are abscissae like any other; equal abscissae among the three points divide by zero and the result is
 * whatever IEEE arithmetic gives.
 * Bounds, for any x: the bisection runs only when xx[1] < t < xx[n-2].  Its last step on the all-left path tests xx[1]
 * and moves k, its last step on the all-right path tests xx[n-2] and moves m, so 2 <= k, m = k + 1 <= n - 1 (1-based),
 * and the three indices stay within 0 .. n-1. */
static double sync_interp1(const double *x, const double *y, double t)
{
    double xx[NH], yy[NH];
    int k, m;
    if (x[0] > x[NH - 1]) {
        for (int j = 0; j < NH; j++) {
            xx[j] = x[NH - 1 - j];
            yy[j] = y[NH - 1 - j];
        }
    } else {
        memcpy(xx, x, sizeof(xx));
        memcpy(yy, y, sizeof(yy));
    }
    if (t <= xx[1]) {
        k = 0;
        m = 2;
    } else if (t >= xx[NH - 2]) {
        k = NH - 3;
        m = NH - 1;
    } else {
        k = 1;
        m = NH;
        while (m - k != 1) {
            const int i = (k + m) / 2;
            if (t < xx[i - 1]) m = i;
            else k = i;
        }
        k -= 1;
        m -= 1;
        if (fabs(t - xx[k]) < fabs(t - xx[m])) k -= 1;
        else m += 1;
    }
    double z = 0.0;
    for (int i = k; i <= m; i++) {
        double s = 1.0;
        for (int j = k; j <= m; j++)
            if (j != i) s = s * (t - xx[j]) / (xx[i] - xx[j]);
        z = z + s * yy[i];
    }
    return z;
}

/* double to int64 as x86-64's cvttsd2si does it: towards zero, and 0x8000000000000000 for what does not fit.  C leaves
 * the reference's (uint64_t) of a negative product undefined (ref src/sdrsync.c:102-103); DESIGN.md section 3.8. */
static uint64_t sync_toint64(double v)
{
    if (!(v > -9223372036854775808.0 && v < 9223372036854775808.0)) return (uint64_t)1 << 63;
    return (uint64_t)(int64_t)v;
}

static int sync_reserve_out(gnsscorr_sync_t *st, size_t more)
{
    if (st->olen == 0) st->ohead = 0;
    if (st->ohead + st->olen + more <= st->ocap) return GNSSCORR_OK;
    if (st->ohead) {
        memmove(st->out, st->out + st->ohead, st->olen * sizeof(*st->out));
        st->ohead = 0;
        if (st->olen + more <= st->ocap) return GNSSCORR_OK;
    }
    size_t cap = st->ocap ? st->ocap : 64;
    while (cap < st->olen + more) cap *= 2;
    gnsscorr_epochobs_t *p = (gnsscorr_epochobs_t *)realloc(st->out, cap * sizeof(*p));
    if (!p) return sync_fail(GNSSCORR_ENOMEM, "gnsscorr_sync: no memory for %zu epoch rows", cap);
    st->out = p;
    st->ocap = cap;
    return GNSSCORR_OK;
}

/* one pass of ref src/sdrsync.c:53-121 over the histories; the caller has reserved nch output rows */
static void sync_poll(gnsscorr_sync_t *st)
{
    int nsat = 0;
    for (int i = 0; i < st->nch; i++)           /* ref :54-60 */
        if (st->chan[i].eligible) st->isat[nsat++] = i;
    const double oldreftow = st->reftow;        /* ref :65-70 */
    double reftow = WEEKSEC;
    for (int i = 0; i < nsat; i++)
        if (st->chan[st->isat[i]].tow[0] < reftow) reftow = st->chan[st->isat[i]].tow[0];
    st->reftow = reftow;
    if (nsat == 0 || oldreftow == reftow) return;       /* ref :72 */
    const double ms = reftow * 1000;
    if (!(ms > -2147483649.0)) return;          /* (int) is not defined there; reftow <= 604800 bounds the other side */
    if ((int)ms % st->outms != 0) return;       /* quirk (b): the truncation drops products just below an integer */
    for (int i = 0; i < nsat; i++) {            /* ref :76-86, quirk (a): ind[] is by position and keeps its value */
        const sync_chan_t *c = &st->chan[st->isat[i]];
        for (int j = 0; j < NH; j++)
            if (fabs(c->tow[j] - reftow) < 1E-4) {
                st->ind[i] = j;
                break;
            }
    }
    uint64_t mincodei = UINT64_MAX;             /* ref :89-98: the nearest satellite */
    int refi = 0;
    for (int i = 0; i < nsat; i++) {
        const sync_chan_t *c = &st->chan[st->isat[i]];
        if (c->codei[st->ind[i]] < mincodei) {
            refi = i;
            mincodei = c->codei[st->ind[i]];
        }
    }
    const sync_chan_t *r = &st->chan[st->isat[refi]];   /* ref :100-105 */
    const uint64_t diffcnt = r->cntout[st->ind[refi]] - r->firstsfcnt;
    const uint64_t sampref = r->firstsf + sync_toint64(r->nsamp * (-GNSSCORR_PTIMING / (1000 * r->ctime) + diffcnt));
    const uint64_t sampbase = r->codei[NH - 1] - (uint64_t)(10 * r->nsamp);     /* quirk (c): codei[79] of a short history is 0 */
    const double samprefd = (double)(sampref - sampbase);
    for (int i = 0; i < nsat; i++) {            /* ref :108-121 */
        const sync_chan_t *c = &st->chan[st->isat[i]];
        gnsscorr_epochobs_t *o = &st->out[st->ohead + st->olen++];
        double codeid[NH];
        memset(o, 0, sizeof(*o));
        o->ch = st->isat[i];
        o->week = c->week;
        o->tow = reftow + (double)(GNSSCORR_PTIMING) / 1000;
        o->P = CLIGHT * c->ti * ((double)(c->codei[st->ind[i]] - sampref) - c->remcout[st->ind[i]]);
        for (int k = 0; k < NH; k++) codeid[k] = (double)(c->codei[k] - sampbase);      /* uint64todouble() */
        o->L = sync_interp1(codeid, c->L, samprefd);
        o->D = sync_interp1(codeid, c->D, samprefd);
        o->S = c->S0;                           /* quirk (d): the newest S, not the one at ind */
        o->sampref = sampref;
    }
}

/* the row a channel's thread appends (setobsdata(), ref src/sdrtrk.c:163-173), then the poll that sees it */
static void sync_consume(gnsscorr_sync_t *st, int ch)
{
    sync_chan_t *c = &st->chan[ch];
    const sync_item_t *it = &c->q[c->head];
    memmove(c->tow + 1, c->tow, sizeof(double) * (NH - 1));
    memmove(c->remcout + 1, c->remcout, sizeof(double) * (NH - 1));
    memmove(c->L + 1, c->L, sizeof(double) * (NH - 1));
    memmove(c->D + 1, c->D, sizeof(double) * (NH - 1));
    memmove(c->codei + 1, c->codei, sizeof(uint64_t) * (NH - 1));
    memmove(c->cntout + 1, c->cntout, sizeof(uint64_t) * (NH - 1));
    c->tow[0] = it->row.tow;
    c->remcout[0] = it->row.remcout;
    c->L[0] = it->row.L;
    c->D[0] = it->row.D;
    c->codei[0] = it->row.codei;
    c->cntout[0] = it->row.cntout;
    if (it->row.snr) c->S0 = it->row.S;
    c->week = it->fr.week;
    c->firstsf = it->fr.firstsf;
    c->firstsfcnt = it->fr.firstsfcnt;
    c->eligible = it->fr.flagdec && it->fr.week != 0 && it->row.cntout >= it->fr.firstsfcnt;
    c->head++;
    if (--c->len == 0) c->head = 0;
    sync_poll(st);
}

/* the waiting row with the smallest codei, the lower channel on ties; -1: none.  *starved: the first attached channel
 * with nothing waiting, or -1 */
static int sync_next(const gnsscorr_sync_t *st, int *starved)
{
    int best = -1;
    *starved = -1;
    for (int i = 0; i < st->nch; i++) {
        const sync_chan_t *c = &st->chan[i];
        if (!c->attached) continue;
        if (c->len == 0) {
            if (*starved < 0) *starved = i;
            continue;
        }
        if (best < 0 || c->q[c->head].row.codei < st->chan[best].q[st->chan[best].head].row.codei) best = i;
    }
    return best;
}

static int sync_drain(gnsscorr_sync_t *st, int all)
{
    for (;;) {
        int starved;
        const int ch = sync_next(st, &starved);
        if (ch < 0 || (!all && starved >= 0)) return GNSSCORR_OK;
        const int rc = sync_reserve_out(st, (size_t)st->nch);
        if (rc) return rc;                      /* the rows stay where they wait */
        sync_consume(st, ch);
    }
}

static void sync_clear(sync_chan_t *c)
{
    sync_item_t *q = c->q;
    const int cap = c->cap, configured = c->configured, nsamp = c->nsamp;
    const double ctime = c->ctime, ti = c->ti;
    memset(c, 0, sizeof(*c));
    c->q = q;
    c->cap = cap;
    c->configured = configured;
    c->nsamp = nsamp;
    c->ctime = ctime;
    c->ti = ti;
}

int gnsscorr_sync_create(gnsscorr_sync_t **pst, int nch, int outms)
{
    if (!pst || nch <= 0 || outms <= 0) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_create: NULL, nch %d or outms %d", nch, outms);
    gnsscorr_sync_t *st = (gnsscorr_sync_t *)calloc(1, sizeof(*st));
    if (st) {
        st->ind = (int *)calloc((size_t)nch, sizeof(int));
        st->isat = (int *)calloc((size_t)nch, sizeof(int));
        st->chan = (sync_chan_t *)calloc((size_t)nch, sizeof(sync_chan_t));
    }
    if (!st || !st->ind || !st->isat || !st->chan) {
        gnsscorr_sync_destroy(st);
        return sync_fail(GNSSCORR_ENOMEM, "gnsscorr_sync_create: no memory for %d channels", nch);
    }
    st->nch = nch;
    st->outms = outms;
    *pst = st;
    return GNSSCORR_OK;
}

void gnsscorr_sync_destroy(gnsscorr_sync_t *st)
{
    if (!st) return;
    if (st->chan)
        for (int i = 0; i < st->nch; i++) free(st->chan[i].q);
    free(st->chan);
    free(st->ind);
    free(st->isat);
    free(st->out);
    free(st);
}

int gnsscorr_sync_channel(gnsscorr_sync_t *st, int ch, int nsamp, double ctime, double ti)
{
    if (!st) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_channel: NULL");
    if (ch < 0 || ch >= st->nch) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_channel: channel %d of %d", ch, st->nch);
    if (nsamp <= 0 || !(ctime > 0 && ctime < INFINITY) || !(ti > 0 && ti < INFINITY))
        return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_channel: channel %d: nsamp %d, ctime %g, ti %g", ch, nsamp, ctime, ti);
    for (int i = 0; i < st->nch; i++)
        if (i != ch && st->chan[i].configured && st->chan[i].ti != ti)
            return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_channel: channel %d: ti %.17g, channel %d has %.17g", ch, ti, i,
                             st->chan[i].ti);
    sync_chan_t *c = &st->chan[ch];
    sync_clear(c);
    c->configured = 1;
    c->attached = 1;
    c->nsamp = nsamp;
    c->ctime = ctime;
    c->ti = ti;
    return GNSSCORR_OK;
}

int gnsscorr_sync_push(gnsscorr_sync_t *st, int ch, const gnsscorr_syncframe_t *fr, const gnsscorr_obsrow_t *rows, int n)
{
    if (!st || !fr || (n > 0 && !rows) || n < 0) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_push: NULL or n %d", n);
    if (ch < 0 || ch >= st->nch) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_push: channel %d of %d", ch, st->nch);
    sync_chan_t *c = &st->chan[ch];
    if (!c->configured) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_push: channel %d before gnsscorr_sync_channel", ch);
    if (n == 0) return GNSSCORR_OK;
    for (int k = 0; k < n; k++) {
        const int have = k > 0 || c->have_last;
        const uint64_t last = k > 0 ? rows[k - 1].codei : c->lastcodei;
        if (have && rows[k].codei <= last)
            return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_push: channel %d row %d: codei %llu is not above %llu", ch, k,
                             (unsigned long long)rows[k].codei, (unsigned long long)last);
    }
    if (n > GNSSCORR_SYNCQCAP - c->len) {
        int starved;
        sync_next(st, &starved);
        if (starved >= 0 && starved != ch)
            return sync_fail(GNSSCORR_ESTATE, "gnsscorr_sync_push: channel %d: %d rows wait and %d more pass the cap of %d: channel "
                             "%d holds the others back (push its rows or detach it)", ch, c->len, n, GNSSCORR_SYNCQCAP, starved);
        return sync_fail(GNSSCORR_ESTATE, "gnsscorr_sync_push: channel %d: %d rows wait and %d more pass the cap of %d", ch,
                         c->len, n, GNSSCORR_SYNCQCAP);
    }
    if (c->head + c->len + n > c->cap) {
        if (c->head) {
            memmove(c->q, c->q + c->head, (size_t)c->len * sizeof(*c->q));
            c->head = 0;
        }
        if (c->len + n > c->cap) {
            int cap = c->cap ? c->cap : 64;
            while (cap < c->len + n) cap *= 2;
            sync_item_t *q = (sync_item_t *)realloc(c->q, (size_t)cap * sizeof(*q));
            if (!q) return sync_fail(GNSSCORR_ENOMEM, "gnsscorr_sync_push: channel %d: no memory for %d rows", ch, cap);
            c->q = q;
            c->cap = cap;
        }
    }
    for (int k = 0; k < n; k++) {
        sync_item_t *it = &c->q[c->head + c->len + k];
        it->row = rows[k];
        it->fr = *fr;
    }
    c->len += n;
    c->lastcodei = rows[n - 1].codei;
    c->have_last = 1;
    c->attached = 1;
    return sync_drain(st, 0);
}

int gnsscorr_sync_detach(gnsscorr_sync_t *st, int ch)
{
    if (!st) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_detach: NULL");
    if (ch < 0 || ch >= st->nch) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_detach: channel %d of %d", ch, st->nch);
    sync_clear(&st->chan[ch]);                  /* the queue, the history, the eligibility; ind[] and reftow stay: quirk (a) */
    return sync_drain(st, 0);                   /* it no longer holds the others back */
}

int gnsscorr_sync_flush(gnsscorr_sync_t *st)
{
    if (!st) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_flush: NULL");
    return sync_drain(st, 1);
}

int gnsscorr_sync_fetch(gnsscorr_sync_t *st, gnsscorr_epochobs_t *out, int max_out)
{
    if (!st || max_out < 0 || (max_out > 0 && !out)) return sync_fail(GNSSCORR_EINVAL, "gnsscorr_sync_fetch: NULL or max_out %d", max_out);
    const size_t n = st->olen < (size_t)max_out ? st->olen : (size_t)max_out;
    if (n) memcpy(out, st->out + st->ohead, n * sizeof(*out));
    st->ohead += n;
    st->olen -= n;
    return (int)n;
}
