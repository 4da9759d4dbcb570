/*
 * sdr_rxnav.c -- frames, observables and epochs behind every step of the receiver: the loop a caller of
 * gnsscorr_rx_step / gnsscorr_trk_run_loop writes around the step's rows, once, with its
 * rules named.  One nav state per channel -- the frame state of the channel's code type and the
 * observables' state -- plus one gnsscorr_sync_t.  Plain host code: the only device work is what
 * gnsscorr_sbasframe_replay does for an SBAS channel.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdr_compat.h"
#include "../../include/gnsscorr.h"

typedef struct {
    gnsscorr_rxnavch_t cfg;
    union {
        gnsscorr_frame_t     ca;
        gnsscorr_sbasframe_t sb;
        gnsscorr_g1frame_t   g1;
    } fr;
    gnsscorr_obs_t ob;
    int      attached, resets, week;    /* week: gnsscorr_rxnav_week's (L1 C/A only) */
    int      fed;                       /* a feed has passed over the channel: cnt is valid */
    int      held;                      /* rows were fed since the last reset */
    int      starved;                   /* consecutive starved feeds (rule 6) */
    uint64_t cnt, nrows;
    double   tow;
    gnsscorr_obsrow_t *rows;            /* the rows the last feed made */
    int      nlast, cap;
} rxnav_chan_t;

struct gnsscorr_rxnav {
    int nch, hold_steps;
    gnsscorr_sync_t *sync;
    rxnav_chan_t *chan;
};

static _Thread_local char g_rxnav_err[256] = "";

static int rxnav_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_rxnav_err, sizeof(g_rxnav_err), fmt, ap);
    va_end(ap);
    return code;
}

/* an error of gnsscorr_sync_*, with its message */
static int rxnav_sync_fail(int code, const char *who, int ch)
{
    return rxnav_fail(code, "%s: channel %d: %s", who, ch, gnsscorr_sync_last_error());
}

const char *gnsscorr_rxnav_last_error(void) { return g_rxnav_err; }

static size_t frame_size(int ctype)
{
    return ctype == CTYPE_L1CA ? sizeof(gnsscorr_frame_t) : ctype == CTYPE_G1 ? sizeof(gnsscorr_g1frame_t) : sizeof(gnsscorr_sbasframe_t);
}

/* the frame fields every code type's state has, by name */
typedef struct {
    int flagsyncf, flagdec, polarity, week, id;
    uint64_t firstsf, firstsfcnt;
    double firstsftow;
} rxnav_fields_t;

static rxnav_fields_t frame_fields(const rxnav_chan_t *c)
{
    rxnav_fields_t f;
    if (c->cfg.ctype == CTYPE_L1CA) {
        const gnsscorr_frame_t *s = &c->fr.ca;
        f = (rxnav_fields_t){s->flagsyncf, s->flagdec, s->polarity, c->week, s->sfid, s->firstsf, s->firstsfcnt, s->firstsftow};
    } else if (c->cfg.ctype == CTYPE_G1) {
        const gnsscorr_g1frame_t *s = &c->fr.g1;
        f = (rxnav_fields_t){s->flagsyncf, s->flagdec, s->polarity, s->week, s->id, s->firstsf, s->firstsfcnt, s->firstsftow};
    } else {
        const gnsscorr_sbasframe_t *s = &c->fr.sb;
        f = (rxnav_fields_t){s->flagsyncf, s->flagdec, s->polarity, s->week, s->id, s->firstsf, s->firstsfcnt, s->firstsftow};
    }
    return f;
}

/* the observables' state with its constants and nothing running */
static void obs_init(rxnav_chan_t *c, double oldremcode)
{
    memset(&c->ob, 0, sizeof(c->ob));
    c->ob.f_sf = c->cfg.f_sf;
    c->ob.f_if = c->cfg.f_if;
    c->ob.foffset = c->cfg.foffset;
    c->ob.ctime = c->cfg.ctime;
    c->ob.loopms = c->cfg.loopms;
    c->ob.oldremcode = oldremcode;
}

/* rule 1 */
static void chan_reset(gnsscorr_rxnav_t *nv, int k)
{
    rxnav_chan_t *c = &nv->chan[k];
    memset(&c->fr, 0, sizeof(c->fr));
    obs_init(c, 0.0);
    c->nrows = 0;
    c->tow = 0.0;
    c->starved = 0;
    if (c->held) c->resets++;
    c->held = 0;
    gnsscorr_sync_detach(nv->sync, k);
    c->attached = 0;
}

int gnsscorr_rxnav_create(gnsscorr_rxnav_t **pnv, int nch, const gnsscorr_rxnavch_t *ch, int outms, int hold_steps)
{
    if (!pnv || !ch || nch <= 0 || hold_steps < 0)
        return rxnav_fail(GNSSCORR_EINVAL, "rxnav_create: bad arguments (nch %d, hold_steps %d)", nch, hold_steps);
    for (int k = 0; k < nch; k++)
        if (ch[k].ctype != CTYPE_L1CA && ch[k].ctype != CTYPE_L1SBAS && ch[k].ctype != CTYPE_G1)
            return rxnav_fail(GNSSCORR_EINVAL, "rxnav_create: channel %d: code type %d (L1 C/A, L1 SBAS or G1)", k, ch[k].ctype);
    gnsscorr_rxnav_t *nv = calloc(1, sizeof(*nv));
    if (!nv) return rxnav_fail(GNSSCORR_ENOMEM, "rxnav_create: out of memory");
    nv->nch = nch;
    nv->hold_steps = hold_steps;
    nv->chan = calloc((size_t)nch, sizeof(*nv->chan));
    if (!nv->chan) {
        free(nv);
        return rxnav_fail(GNSSCORR_ENOMEM, "rxnav_create: out of memory");
    }
    int rc = gnsscorr_sync_create(&nv->sync, nch, outms);
    if (rc) {
        nv->sync = NULL;
        gnsscorr_rxnav_destroy(nv);
        return rxnav_fail(rc, "rxnav_create: %s", gnsscorr_sync_last_error());
    }
    for (int k = 0; k < nch; k++) {
        rxnav_chan_t *c = &nv->chan[k];
        c->cfg = ch[k];
        obs_init(c, ch[k].oldremcode);
        /* declared, and detached until it delivers */
        rc = gnsscorr_sync_channel(nv->sync, k, ch[k].nsamp, ch[k].ctime, ch[k].ti);
        if (!rc) rc = gnsscorr_sync_detach(nv->sync, k);
        if (rc) {
            gnsscorr_rxnav_destroy(nv);
            return rxnav_sync_fail(rc, "rxnav_create", k);
        }
    }
    *pnv = nv;
    return GNSSCORR_OK;
}

void gnsscorr_rxnav_destroy(gnsscorr_rxnav_t *nv)
{
    if (!nv) return;
    if (nv->chan)
        for (int k = 0; k < nv->nch; k++) free(nv->chan[k].rows);
    free(nv->chan);
    if (nv->sync) gnsscorr_sync_destroy(nv->sync);
    free(nv);
}

int gnsscorr_rxnav_week(gnsscorr_rxnav_t *nv, int ch, int week)
{
    if (!nv || ch < 0 || ch >= nv->nch) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_week: channel %d of %d", ch, nv ? nv->nch : 0);
    if (nv->chan[ch].cfg.ctype != CTYPE_L1CA)
        return rxnav_fail(GNSSCORR_EINVAL, "rxnav_week: channel %d takes its week from its frame state", ch);
    nv->chan[ch].week = week;
    return GNSSCORR_OK;
}

int gnsscorr_rxnav_feed(gnsscorr_rxnav_t *nv, gnsscorr_ctx *ctx, const gnsscorr_trklog_t *log, const double *II0,
                        int stride, const int *ndone, const uint64_t *cnt_after, const int *tracking)
{
    if (!nv || !log || !II0 || !ndone || !cnt_after || !tracking) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_feed: null argument");
    /* validation: nothing is touched before every channel has passed */
    int any = 0;
    for (int k = 0; k < nv->nch; k++) {
        const rxnav_chan_t *c = &nv->chan[k];
        if (ndone[k] < 0 || stride < ndone[k])
            return rxnav_fail(GNSSCORR_EINVAL, "rxnav_feed: channel %d: %d rows with a stride of %d", k, ndone[k], stride);
        if (cnt_after[k] < (uint64_t)ndone[k])
            return rxnav_fail(GNSSCORR_EINVAL, "rxnav_feed: channel %d: cnt %llu behind %d rows", k, (unsigned long long)cnt_after[k], ndone[k]);
        if (c->cfg.ctype == CTYPE_L1SBAS && !ctx)
            return rxnav_fail(GNSSCORR_EINVAL, "rxnav_feed: channel %d is SBAS: its Viterbi decodes need the context", k);
        if (ndone[k] > 0) any++;
    }
    for (int k = 0; k < nv->nch; k++) {
        const rxnav_chan_t *c = &nv->chan[k];
        const uint64_t cnt0 = cnt_after[k] - (uint64_t)ndone[k];
        if (ndone[k] > 0 && c->fed && cnt0 != 0 && cnt0 != c->cnt)
            return rxnav_fail(GNSSCORR_ESTATE, "rxnav_feed: channel %d: rows from cnt %llu on, the feed before ended at %llu "
                              "(a step's rows were skipped)", k, (unsigned long long)cnt0, (unsigned long long)c->cnt);
    }
    for (int k = 0; k < nv->nch; k++) {
        rxnav_chan_t *c = &nv->chan[k];
        const int n = ndone[k];
        const uint64_t cnt0 = cnt_after[k] - (uint64_t)n;
        const gnsscorr_trklog_t *rows = log + (size_t)k * stride;
        const double *ii = II0 + (size_t)k * stride;
        /* 1. reset */
        if (!tracking[k] || (n > 0 && cnt0 == 0 && c->held)) chan_reset(nv, k);
        c->fed = 1;
        c->cnt = cnt_after[k];
        c->nlast = 0;
        if (n > 0 && tracking[k]) {
            /* 2. frame replay */
            int rc;
            if (c->cfg.ctype == CTYPE_L1CA) rc = gnsscorr_frame_replay(&c->fr.ca, rows, n, cnt0);
            else if (c->cfg.ctype == CTYPE_G1) rc = gnsscorr_g1frame_replay(&c->fr.g1, rows, n, cnt0);
            else rc = gnsscorr_sbasframe_replay(ctx, &c->fr.sb, rows, n, cnt0, NULL, 0);
            c->held = 1;
            if (rc) return rxnav_fail(rc, "rxnav_feed: channel %d: frame replay failed (%d)", k, rc);
            /* 3. frame fields, before the piece that raised flagdec */
            const rxnav_fields_t f = frame_fields(c);
            if (f.flagdec) {
                c->ob.flagsyncf = f.flagsyncf;
                c->ob.polarity = f.polarity;
                c->ob.firstsftow = f.firstsftow;
                c->ob.firstsfcnt = f.firstsfcnt;
            }
            /* 4. observables */
            if (c->cap < n) {
                gnsscorr_obsrow_t *p = realloc(c->rows, sizeof(*p) * (size_t)n);
                if (!p) return rxnav_fail(GNSSCORR_ENOMEM, "rxnav_feed: channel %d: out of memory", k);
                c->rows = p;
                c->cap = n;
            }
            const int nobs = gnsscorr_obs_replay(&c->ob, rows, ii, n, cnt0, c->rows, c->cap);
            if (nobs < 0) return rxnav_fail(nobs, "rxnav_feed: channel %d: observables replay failed (%d)", k, nobs);
            c->nlast = nobs;
            c->nrows += (uint64_t)nobs;
            if (nobs > 0) c->tow = c->rows[nobs - 1].tow;
            /* 5. push */
            if (nobs > 0) {
                const gnsscorr_syncframe_t sf = {f.flagdec, f.week, f.firstsf, f.firstsfcnt};
                rc = gnsscorr_sync_push(nv->sync, k, &sf, c->rows, nobs);
                if (rc) return rxnav_sync_fail(rc, "rxnav_feed", k);
                c->attached = 1;
            }
        }
        /* 6. starvation */
        if (n == 0 && tracking[k] && c->attached && any > 0) {
            c->starved++;
            if (nv->hold_steps > 0 && c->starved >= nv->hold_steps) {
                gnsscorr_sync_detach(nv->sync, k);
                c->attached = 0;
                c->starved = 0;
            }
        } else {
            c->starved = 0;
        }
    }
    return GNSSCORR_OK;
}

int gnsscorr_rxnav_flush(gnsscorr_rxnav_t *nv)
{
    if (!nv) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_flush: null");
    const int rc = gnsscorr_sync_flush(nv->sync);
    return rc ? rxnav_fail(rc, "rxnav_flush: %s", gnsscorr_sync_last_error()) : rc;
}

int gnsscorr_rxnav_fetch(gnsscorr_rxnav_t *nv, gnsscorr_epochobs_t *out, int max_out)
{
    if (!nv) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_fetch: null");
    const int rc = gnsscorr_sync_fetch(nv->sync, out, max_out);
    return rc < 0 ? rxnav_fail(rc, "rxnav_fetch: %s", gnsscorr_sync_last_error()) : rc;
}

int gnsscorr_rxnav_status(gnsscorr_rxnav_t *nv, gnsscorr_rxnavstat_t *st)
{
    if (!nv || !st) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_status: null argument");
    for (int k = 0; k < nv->nch; k++) {
        const rxnav_chan_t *c = &nv->chan[k];
        const rxnav_fields_t f = frame_fields(c);
        memset(&st[k], 0, sizeof(st[k]));
        st[k].ctype = c->cfg.ctype;
        st[k].attached = c->attached;
        st[k].flagsyncf = f.flagsyncf;
        st[k].flagdec = f.flagdec;
        st[k].polarity = f.polarity;
        st[k].week = f.week;
        st[k].id = f.id;
        st[k].resets = c->resets;
        st[k].cnt = c->cnt;
        st[k].firstsf = f.firstsf;
        st[k].firstsfcnt = f.firstsfcnt;
        st[k].nrows = c->nrows;
        st[k].firstsftow = f.firstsftow;
        st[k].tow = c->tow;
    }
    return GNSSCORR_OK;
}

int gnsscorr_rxnav_frame(gnsscorr_rxnav_t *nv, int ch, void *state, size_t size)
{
    if (!nv || !state || ch < 0 || ch >= nv->nch) return rxnav_fail(GNSSCORR_EINVAL, "rxnav_frame: channel %d of %d", ch, nv ? nv->nch : 0);
    const rxnav_chan_t *c = &nv->chan[ch];
    if (size != frame_size(c->cfg.ctype))
        return rxnav_fail(GNSSCORR_EINVAL, "rxnav_frame: channel %d: %zu bytes, its frame state has %zu", ch, size, frame_size(c->cfg.ctype));
    memcpy(state, &c->fr, size);
    return GNSSCORR_OK;
}

int gnsscorr_rxnav_rows(gnsscorr_rxnav_t *nv, int ch, gnsscorr_obsrow_t *rows, int max_rows)
{
    if (!nv || ch < 0 || ch >= nv->nch || max_rows < 0 || (!rows && max_rows))
        return rxnav_fail(GNSSCORR_EINVAL, "rxnav_rows: channel %d of %d, room for %d rows", ch, nv ? nv->nch : 0, max_rows);
    const rxnav_chan_t *c = &nv->chan[ch];
    const int n = c->nlast < max_rows ? c->nlast : max_rows;
    if (n) memcpy(rows, c->rows, sizeof(*rows) * (size_t)n);
    return n;
}
