// gnsscorr_rx.hip -- the receiver schedule: sdrthread()'s per-channel state machine (ref src/sdrmain.c:247-316) on the
// batched engine.  A channel searches (sdracquisition(), retried after a pause) until it is acquired, then tracks one
// code period after the other.  The states live on the host, which needs them to size the launches; the work they
// select runs on the device: the due channels' search as one list (gnsscorr_acq.hip), the hand-over of the acquired
// ones into the closed loop (acq_to_loop_kernel), and the closed loop itself, in which a channel that is not tracking
// is handed a write position of 0 and so plans nothing (trk_step_tail_kernel, ref src/sdrtrk.c:26-30).  The way back,
// TRACK -> SEARCH, which the reference lacks, is the lock monitor's (gnsscorr_lock.hip): it runs behind the closed loop
// of a step, and the next step reads its verdicts.  In front of it, bit synchronisation by symbol energy
// (gnsscorr_bsync.hip) presets flagsync / synci of a tracking channel on the device, for the next step's first period.
// Behind both, the correlation monitor (gnsscorr_cfm.hip) sums every tap over whole nav bits and tests the shape of the
// correlation function; it reports only.
//
// The reference sleeps ACQSLEEP = 2000 ms of wall time after a failed search (ref src/sdracq.c:57-60).  Here the pause
// is counted on the sample clock -- retry_ms * 1e-3 * f_sf samples of the channel's ring from the write position of
// the failed search -- so that the schedule depends on the input alone.
#include <vector>

#include "gnsscorr_stage.h"

#define GC_ACQSLEEP 2000        // ms, ref src/sdr.h (ACQSLEEP)

// ref src/sdracq.c:24-26; a channel that compensates code Doppler looks `back` samples further (shifts
// beyond a code period are the search's to refuse)
static uint64_t rx_first_try(const gnsscorr_ctx *ctx, int ch)
{
    const GcChan &c = ctx->hchan[ch];
    std::vector<int32_t> s;
    int back = 0;
    if (ctx->hfcf[ch] != 0.0 && gc_acq_shifts(ctx, ch, s, &back) != GNSSCORR_OK) back = 0;
    return (uint64_t)(c.intg + 1) * (uint64_t)c.nsamp + (uint64_t)back;
}

extern "C" int gnsscorr_rx_start(gnsscorr_ctx *ctx, int retry_ms)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    if (!ctx->nch) return gc_fail(GNSSCORR_ESTATE, "rx_start: no channels set");
    for (int i = 0; i < ctx->nch; i++)
        if (!ctx->loop.isset[i])
            return gc_fail(GNSSCORR_ESTATE, "rx_start: channel %d has no loop constants (gnsscorr_loop_set)", i);
    GcRx &rx = ctx->rx;
    ctx->nav.off();             // the nav driver's states belong to the schedule that ends here (gnsscorr_rx_nav_start comes after)
    rx.retry_ms = retry_ms > 0 ? retry_ms : GC_ACQSLEEP;
    gnsscorr_rxstat_t z;
    memset(&z, 0, sizeof(z));
    rx.st.assign(ctx->nch, z);
    // the lock monitor is off for all; a launch of an earlier schedule is waited for and its verdicts dropped
    if (ctx->lock_pending) GC_HIP(hipEventSynchronize(ctx->ev_lock));
    ctx->lock_pending = false;
    rx.losses.assign(ctx->nch, 0);
    rx.lock_listed.clear();
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(rx.lock.start(ctx));
    // so are bit synchronisation, whose applied counts start over with its states, and the correlation monitor
    GC_TRY(rx.bsync.start(ctx));
    if (rx.dbsync_applied) GC_HIP(hipMemsetAsync(rx.dbsync_applied, 0, sizeof(int) * ctx->nch, ctx->stream));
    GC_TRY(rx.cfm.start(ctx));
    for (int i = 0; i < ctx->nch; i++) {
        rx.st[i].state = GNSSCORR_CH_SEARCH;
        rx.st[i].next_try = rx_first_try(ctx, i);
    }
    rx.on = true;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_rx_set(gnsscorr_ctx *ctx, int ch, int state)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_set: no gnsscorr_rx_start yet");
    if (ch < 0 || ch >= ctx->nch) return gc_fail(GNSSCORR_EINVAL, "rx_set: channel %d of %d", ch, ctx->nch);
    gnsscorr_rxstat_t &s = ctx->rx.st[ch];
    if (state == GNSSCORR_CH_IDLE) {
        s.state = GNSSCORR_CH_IDLE;
    } else if (state == GNSSCORR_CH_SEARCH) {
        std::lock_guard<std::mutex> lk(ctx->mtx);
        s.state = GNSSCORR_CH_SEARCH;
        s.next_try = ctx->ring[ctx->hdesc[ch].ftype - 1].wrpos;
    } else {
        return gc_fail(GNSSCORR_EINVAL, "rx_set: state %d (a channel starts tracking through acquisition only)", state);
    }
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_rx_step(gnsscorr_ctx *ctx, int max_periods)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_step: no gnsscorr_rx_start yet");
    if (max_periods <= 0) return gc_fail(GNSSCORR_EINVAL, "rx_step: max_periods %d", max_periods);
    GC_HIP(hipSetDevice(ctx->device));
    GcRx &rx = ctx->rx;
    const int nch = ctx->nch;
    uint64_t wpr[2];
    {
        std::lock_guard<std::mutex> lk(ctx->mtx);
        wpr[0] = ctx->ring[0].wrpos;
        wpr[1] = ctx->ring[1].wrpos;
    }
    // 0. the verdicts of the monitor launch behind the previous step's closed loop: a TRACK channel it declared lost is
    //    due at this step's write position.  Words of channels that are no longer TRACK (parked or re-armed since) are
    //    ignored.
    if (ctx->lock_pending) {
        GC_HIP(hipEventSynchronize(ctx->ev_lock));
        ctx->lock_pending = false;
        for (int i : rx.lock_listed) {
            if (!rx.lock_lost[i] || rx.st[i].state != GNSSCORR_CH_TRACK) continue;
            rx.st[i].state = GNSSCORR_CH_SEARCH;
            rx.st[i].next_try = wpr[ctx->hdesc[i].ftype - 1];
            rx.losses[i]++;
        }
    }
    // 1. the channels whose search is due, as one list
    std::vector<int> due;
    for (int i = 0; i < nch; i++) {
        const uint64_t wp = wpr[ctx->hdesc[i].ftype - 1];
        if (rx.st[i].state == GNSSCORR_CH_SEARCH && wp >= rx.st[i].next_try && wp >= rx_first_try(ctx, i)) due.push_back(i);
    }
    if (!due.empty()) {
        int rc = gc_acq_run_list(ctx, wpr, due.data(), (int)due.size());
        if (rc) return rc;
        rc = gc_loop_take_state(ctx);
        if (rc) return rc;
        rc = gc_acq_handover(ctx, false);
        if (rc) return rc;
        // 2. the outcome: the schedule needs the acquired flags
        std::vector<gnsscorr_acqres_t> res(nch);
        rc = gnsscorr_acq_fetch(ctx, res.data());
        if (rc) return rc;
        for (int i : due) {
            gnsscorr_rxstat_t &s = rx.st[i];
            const uint64_t wp = wpr[ctx->hdesc[i].ftype - 1];
            s.attempts++;
            s.acq = res[i];
            s.acq_wrpos = wp;
            if (res[i].flagacq) s.state = GNSSCORR_CH_TRACK;
            else s.next_try = wp + (uint64_t)((double)rx.retry_ms * 1e-3 * ctx->hdesc[i].f_sf);
        }
    }
    // 3. the closed loop for the tracking channels, those acquired above included
    std::vector<uint64_t> wp(nch);
    for (int i = 0; i < nch; i++) wp[i] = rx.st[i].state == GNSSCORR_CH_TRACK ? wpr[ctx->hdesc[i].ftype - 1] : 0;
    int rc = gc_trk_run_loop(ctx, max_periods, wp.data());
    // 3b. bit synchronisation by symbol energy over the periods just tracked: a decision presets flagsync / synci in the
    //     device's loop state, which the next step's first period sees; nothing waits for it here
    if (!rc && rx.bsync.on) rc = gc_rx_bsync_launch(ctx, max_periods);
    // 4. the lock monitor over the periods just tracked, behind the loop's last tail; nothing waits for it here
    if (!rc && rx.lock.on) rc = gc_rx_lock_launch(ctx, max_periods);
    // 5. the correlation monitor over the same periods: it reports only (gnsscorr_rx_cfm_status), so no step reads it
    if (!rc && rx.cfm.on) rc = gc_rx_cfm_launch(ctx, max_periods);
    return rc;
}

extern "C" int gnsscorr_rx_status(gnsscorr_ctx *ctx, gnsscorr_rxstat_t *st)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_status: no gnsscorr_rx_start yet");
    if (!st) return gc_fail(GNSSCORR_EINVAL, "rx_status: null status array");
    GC_HIP(hipSetDevice(ctx->device));
    const int nch = ctx->nch;
    // sdrthread's cnt of every channel: one column of the device's loop states, behind whatever the stream still runs
    std::vector<uint64_t> cnt(nch);
    GC_TRY(gc_loop_column(ctx, offsetof(gnsscorr_loop_t, cnt), sizeof(uint64_t), 0, nch, cnt.data()));
    for (int i = 0; i < nch; i++) {
        st[i] = ctx->rx.st[i];
        st[i].cnt = cnt[i];
    }
    return GNSSCORR_OK;
}

// ---- frames, observables and epochs behind every step: the context's driver of csrc/sdr_rxnav.c -----------------------
static int nav_fail(int rc) { return gc_fail(rc, "%s", gnsscorr_rxnav_last_error()); }

extern "C" int gnsscorr_rx_nav_start(gnsscorr_ctx *ctx, int outms, int hold_steps)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    if (!ctx->nch) return gc_fail(GNSSCORR_ESTATE, "rx_nav_start: no channels set");
    const int nch = ctx->nch;
    for (int i = 0; i < nch; i++)
        if (!ctx->loop.isset[i])
            return gc_fail(GNSSCORR_ESTATE, "rx_nav_start: channel %d has no loop constants (gnsscorr_loop_set)", i);
    if (ctx->rx.on)
        for (int i = 0; i < nch; i++)
            if (ctx->rx.st[i].attempts > 0)
                return gc_fail(GNSSCORR_ESTATE, "rx_nav_start: the schedule has stepped (channel %d was searched): start the "
                               "nav driver before the first gnsscorr_rx_step", i);
    // the constants: the channel table, loopms of the loop constants, the remcode the first row's oldremcode is
    std::vector<gnsscorr_loop_t> lp(nch);
    std::vector<gnsscorr_trkstate_t> ts(nch);
    GC_TRY(gnsscorr_loop_get(ctx, 0, nch, lp.data()));
    GC_TRY(gnsscorr_trk_get_state(ctx, 0, nch, ts.data()));
    std::vector<gnsscorr_rxnavch_t> ch(nch);
    for (int i = 0; i < nch; i++) {
        const gnsscorr_chan_t &c = ctx->hdesc[i];
        memset(&ch[i], 0, sizeof(ch[i]));
        ch[i].ctype = c.ctype;
        ch[i].nsamp = c.nsamp;
        ch[i].loopms = lp[i].loopms;
        ch[i].f_sf = c.f_sf;
        ch[i].f_if = c.f_if;
        ch[i].foffset = c.foffset;
        ch[i].ctime = c.ctime;
        ch[i].ti = c.ti;
        ch[i].oldremcode = ts[i].remcode;
    }
    gnsscorr_rxnav_t *nv = nullptr;
    const int rc = gnsscorr_rxnav_create(&nv, nch, ch.data(), outms, hold_steps);
    if (rc) return nav_fail(rc);            // (a driver that was running stays)
    ctx->nav.off();
    ctx->nav.nv = nv;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_rx_nav_stop(gnsscorr_ctx *ctx)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    if (!ctx->nav.nv) return gc_fail(GNSSCORR_ESTATE, "rx_nav_stop: no gnsscorr_rx_nav_start yet");
    ctx->nav.off();
    return GNSSCORR_OK;
}

extern "C" gnsscorr_rxnav_t *gnsscorr_rx_nav(gnsscorr_ctx *ctx) { return ctx ? ctx->nav.nv : nullptr; }

extern "C" int gnsscorr_rx_nav_step(gnsscorr_ctx *ctx, int max_periods)
{
    if (!ctx || !ctx->nav.nv) return gc_fail(GNSSCORR_ESTATE, "rx_nav_step: no gnsscorr_rx_nav_start yet");
    GC_TRY(ctx->rx.on ? gnsscorr_rx_step(ctx, max_periods) : gnsscorr_trk_run_loop(ctx, max_periods));
    GcNav &nav = ctx->nav;
    const int nch = ctx->nch;
    const size_t units = (size_t)nch * max_periods;
    if (nav.log.size() < units) {
        nav.log.resize(units);
        nav.ii0.resize(units);
    }
    nav.ndone.resize(nch);
    nav.tracking.resize(nch);
    nav.cnt.resize(nch);
    // the step's rows and the prompt column; sdrthread's cnt and the state behind the step
    GC_TRY(gnsscorr_trk_fetch_log(ctx, nav.log.data(), nav.ndone.data()));
    GC_TRY(gnsscorr_trk_fetch_prompt(ctx, nav.ii0.data(), nullptr));
    if (ctx->rx.on) {
        nav.st.resize(nch);
        GC_TRY(gnsscorr_rx_status(ctx, nav.st.data()));
        for (int i = 0; i < nch; i++) {
            nav.cnt[i] = nav.st[i].cnt;
            nav.tracking[i] = nav.st[i].state == GNSSCORR_CH_TRACK;
        }
    } else {
        GC_TRY(gc_loop_column(ctx, offsetof(gnsscorr_loop_t, cnt), sizeof(uint64_t), 0, nch, nav.cnt.data()));
        for (int i = 0; i < nch; i++) nav.tracking[i] = 1;
    }
    const int rc = gnsscorr_rxnav_feed(nav.nv, ctx, nav.log.data(), nav.ii0.data(), max_periods, nav.ndone.data(), nav.cnt.data(),
                                       nav.tracking.data());
    return rc ? nav_fail(rc) : GNSSCORR_OK;
}
