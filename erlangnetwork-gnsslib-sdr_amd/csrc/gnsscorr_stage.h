// gnsscorr_stage.h -- what the schedule's per-channel stages behind the closed loop share: the lock
// monitor (gnsscorr_lock.hip), bit synchronisation by symbol energy (gnsscorr_bsync.hip) and the correlation monitor
// (gnsscorr_cfm.hip).  Their kernels walk the rows of a run differently and stay apart; around the walks there is one
// rows view with its decode and two builders, one staging path for gnsscorr_{lock,bsync,cfm}_run, the operations of the
// stage record GcStage (gnsscorr_ctx.h), and the read of one column of the device's loop states.
#pragma once

#include <cstddef>

#include "gnsscorr_ctx.h"

// The rows of a run as a stage kernel sees them, by value.  chlist: the channels of the launch (nullptr: channel = list
// index), nlist of them.  I / Q: element ch * ch_stride + e * row_stride (+ t) is the prompt sum (tap t) of row e.
// log: [channel][nper] the rows' flagsync / navbit.  ndone: [channel] rows of the run, at most nper.  rate / cnt: byte
// pointers to channel 0's value and the byte stride to the next channel's; cnt_after: the value is the cnt behind the
// run (cnt0 = cnt - ndone), else cnt0.
struct GcRowsView {
    const int *chlist;
    int nlist;
    const char *rate;
    size_t rate_stride;
    const double *I, *Q;
    size_t ch_stride, row_stride;
    const gnsscorr_trklog_t *log;
    int nper;
    const int *ndone;
    const char *cnt;
    size_t cnt_stride;
    int cnt_after;
};

// One list entry of a view.  have: the entry exists (else ch = rt = nd = cnt0 = 0 and the pointers are channel 0's,
// never to be read).  rt: the channel's rate; nd: its rows, 0 .. nper; cnt0: the cnt of row 0.
struct GcRows {
    bool have;
    int ch, rt, nd;
    unsigned long long cnt0;
    const double *pI, *pQ;
    const gnsscorr_trklog_t *plog;
};

// Integer and pointer work only: the kernels keep their own returns and their own "off" conditions.
__device__ __forceinline__ GcRows gc_rows(const GcRowsView &v, int li)
{
    GcRows r;
    r.have = li < v.nlist;
    r.ch = r.have ? (v.chlist ? v.chlist[li] : li) : 0;
    // read without a branch (channel 0's values stand in where there is no entry: in bounds, and dropped below), so that
    // the loads a kernel adds for its own prm and st are in flight beside these and not behind them
    const int rt = *reinterpret_cast<const int *>(v.rate + (size_t)r.ch * v.rate_stride);
    const int nd = min(max(v.ndone[r.ch], 0), v.nper);
    unsigned long long cnt0 = *reinterpret_cast<const unsigned long long *>(v.cnt + (size_t)r.ch * v.cnt_stride);
    if (v.cnt_after) cnt0 -= (unsigned long long)nd;
    r.rt = r.have ? rt : 0;
    r.nd = r.have ? nd : 0;
    r.cnt0 = r.have ? cnt0 : 0;
    r.pI = v.I + (size_t)r.ch * v.ch_stride;
    r.pQ = v.Q + (size_t)r.ch * v.ch_stride;
    r.plog = v.log + (size_t)r.ch * (size_t)v.nper;
    return r;
}

// The rows the last gc_trk_run_loop of nperiod periods left, for the n channels of a mapped list.
static inline GcRowsView gc_rows_of_run(const gnsscorr_ctx *ctx, const int *dlist, int n, int nperiod)
{
    const char *loop = (const char *)ctx->loop.dloop.p;
    // trk.II is the correlator's QQ (ref src/sdrtrk.c:42): gnsscorr_trk_fetch's II rows are dcorrQ
    return {dlist, n, loop + offsetof(gnsscorr_loop_t, rate), sizeof(gnsscorr_loop_t), ctx->out.dcorrQ.p, ctx->out.dcorrI.p,
            (size_t)nperiod * ctx->ntap, (size_t)ctx->ntap, ctx->loop.dlog.p, nperiod, ctx->loop.ddone.p,
            loop + offsetof(gnsscorr_loop_t, cnt), sizeof(gnsscorr_loop_t), 1};
}

// One column of the device's loop states, channels ch0 .. ch0+nch-1, behind whatever the stream still runs: the field
// at byte `offset`, `size` bytes each, into dst.  Waits for it.
static inline int gc_loop_column(gnsscorr_ctx *ctx, size_t offset, size_t size, int ch0, int nch, void *dst)
{
    GC_HIP(hipMemcpy2DAsync(dst, size, (const char *)(ctx->loop.dloop.p + ch0) + offset, sizeof(gnsscorr_loop_t), size, nch,
                            hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

// gnsscorr_{lock,bsync,cfm}_run behind their argument checks: the host arrays of nch channels and nper rows (vals
// doubles per row in I and Q) go to the context's staging buffer as one blob in one transfer -- prm, rate, ndone, cnt0,
// st, I, Q, log, each 16-byte aligned -- launch(rows, dprm, dst) queues the kernel on the context's stream, and st comes
// back.  Holds the context's lock and waits for the stream, so the one buffer serves all three.
template <class Prm, class St, class Launch>
static int gc_stage_run(gnsscorr_ctx *ctx, const Prm *prm, const int *rate, St *st, const double *I, const double *Q,
                        const gnsscorr_trklog_t *log, const int *ndone, const uint64_t *cnt0, int nch, int nper, int vals,
                        Launch launch)
{
    std::lock_guard<std::mutex> lk(ctx->mtx);
    GC_HIP(hipSetDevice(ctx->device));
    const size_t units = (size_t)nch * nper;
    const void *src[8] = {prm, rate, ndone, cnt0, st, I, Q, log};
    const size_t len[8] = {sizeof(Prm) * nch, sizeof(int) * nch, sizeof(int) * nch, sizeof(uint64_t) * nch, sizeof(St) * nch,
                           sizeof(double) * units * vals, sizeof(double) * units * vals, sizeof(gnsscorr_trklog_t) * units};
    size_t o[9] = {0};
    for (int i = 0; i < 8; i++) o[i + 1] = (o[i] + len[i] + 15) & ~(size_t)15;
    std::vector<unsigned char> blob(o[8], 0);
    for (int i = 0; i < 8; i++) memcpy(&blob[o[i]], src[i], len[i]);
    GC_RESERVE(ctx, ctx->dstage, o[8]);
    unsigned char *d = ctx->dstage;
    GC_HIP(hipMemcpyAsync(d, blob.data(), o[8], hipMemcpyHostToDevice, ctx->stream));
    const GcRowsView rows = {nullptr, nch, (const char *)(d + o[1]), sizeof(int), (const double *)(d + o[5]), (const double *)(d + o[6]),
                             (size_t)nper * vals, (size_t)vals, (const gnsscorr_trklog_t *)(d + o[7]), nper, (const int *)(d + o[2]),
                             (const char *)(d + o[3]), sizeof(uint64_t), 0};
    launch(rows, (const Prm *)(d + o[0]), (St *)(d + o[4]));
    GC_HIP(hipGetLastError());
    GC_HIP(hipMemcpyAsync(blob.data(), d + o[4], len[4], hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(st, blob.data(), len[4]);
    return GNSSCORR_OK;
}

// ---- GcStage (gnsscorr_ctx.h) ------------------------------------------------------------------------------------------
static inline bool gc_prm_on(const gnsscorr_lockprm_t &p) { return p.kbits != 0; }
static inline bool gc_prm_on(const gnsscorr_bsyncprm_t &p) { return p.nsym != 0; }
static inline bool gc_prm_on(const gnsscorr_cfmprm_t &p) { return p.kbits != 0; }

// gnsscorr_rx_*_set behind "the schedule is on": p (all zero: off) for channels ch0 .. ch0+nch-1.  check(who, p, rate,
// channel) is the stage's own, run per channel with the channel's nav bit length when p is on.  A state buffer made
// here is zeroed whole, so a channel never named reads as zeros; otherwise only the named channels' states are.
template <class Prm, class St>
template <class Check>
int GcStage<Prm, St>::set(gnsscorr_ctx *ctx, const char *who, int ch0, int nch, const Prm &p, Check check)
{
    if (ch0 < 0 || nch < 0 || ch0 > ctx->nch - nch)     // (compared without forming ch0 + nch, which can overflow)
        return gc_fail(GNSSCORR_EINVAL, "%s: channels %d..%d of %d", who, ch0, (int)((unsigned)ch0 + nch - 1u), ctx->nch);
    if (nch == 0) return GNSSCORR_OK;
    GC_HIP(hipSetDevice(ctx->device));
    if (gc_prm_on(p)) {
        std::vector<int> rate(nch);
        GC_TRY(gc_loop_column(ctx, offsetof(gnsscorr_loop_t, rate), sizeof(int), ch0, nch, rate.data()));
        for (int i = 0; i < nch; i++) GC_TRY(check(who, p, rate[i], ch0 + i));
    }
    const bool fresh = !dst;
    GC_RESERVE(ctx, dprm, ctx->nch);
    GC_RESERVE(ctx, dst, ctx->nch);
    GC_TRY(list.reserve(ctx->nch, hipHostMallocMapped));
    for (int i = 0; i < nch; i++) prm[ch0 + i] = p;
    on = 0;
    for (const Prm &q : prm) on += gc_prm_on(q);
    // behind whatever the stream still runs (a launch of the last step included; the lock monitor's verdicts stay to be read)
    GC_HIP(hipStreamSynchronize(ctx->stream));
    GC_HIP(hipMemcpy(dprm.p, prm.data(), sizeof(Prm) * ctx->nch, hipMemcpyHostToDevice));
    if (fresh) GC_HIP(hipMemset(dst.p, 0, sizeof(St) * ctx->nch));
    else GC_HIP(hipMemset(dst.p + ch0, 0, sizeof(St) * nch));
    return GNSSCORR_OK;
}

// gnsscorr_rx_*_status: zeros when the stage has never been on, else the copy queued behind the stream (the caller waits)
template <class Prm, class St>
int GcStage<Prm, St>::status(gnsscorr_ctx *ctx, St *out) const
{
    if (dst) GC_HIP(hipMemcpyAsync(out, dst, sizeof(St) * ctx->nch, hipMemcpyDeviceToHost, ctx->stream));
    else memset(out, 0, sizeof(St) * ctx->nch);
    return GNSSCORR_OK;
}

// gnsscorr_rx_start (the device is set): off for all, and the states start over, behind a launch of an earlier schedule
template <class Prm, class St>
int GcStage<Prm, St>::start(gnsscorr_ctx *ctx)
{
    Prm off;
    memset(&off, 0, sizeof(off));
    prm.assign(ctx->nch, off);
    on = 0;
    if (dst) GC_HIP(hipMemsetAsync(dst, 0, sizeof(St) * ctx->nch, ctx->stream));
    return GNSSCORR_OK;
}

// The TRACK channels that have the stage on, into the mapped list; returns how many.  Rewriting the list is safe
// because the kernel that read it last is over.  Lock monitor: the previous launch's event has been waited for in step
// 0 of gnsscorr_rx_step.  Bit synchronisation and the correlation monitor: the closed loop of this step drained the
// stream before its first launch.
template <class Prm, class St>
int GcStage<Prm, St>::fill(const std::vector<gnsscorr_rxstat_t> &rxst)
{
    int n = 0;
    for (size_t i = 0; i < prm.size(); i++)
        if (gc_prm_on(prm[i]) && rxst[i].state == GNSSCORR_CH_TRACK) list[n++] = (int)i;
    return n;
}
