// gnsscorr_lock.hip -- the lock monitor for gfx950 (MI355X): the TRACK -> SEARCH edge of the receiver schedule
// (gnsscorr_rx.hip), which the reference does not have -- once flagacq is set it is never cleared (ref
// src/sdrmain.c:247-316), so a channel whose satellite sets, or that was acquired on noise, tracks noise to the end.
//
// The detector (every arithmetic statement one IEEE double operation, sums in period order, npsum in
// bit order), per channel over the rows e < ndone of one closed-loop run, cnt = cnt0 + e:
//   cnt == 0               the state is zeroed (first period after a hand-over)
//   lost                   sticky: nothing more is read
//   flagsync[e] == 0       reason 1 if sync_periods > 0 and cnt + 1 >= sync_periods; the row counts for nothing else
//   otherwise              while a bit is open, sI += I, sQ += Q, w += I*I + Q*Q, n += 1; a row with navbit != 0 closes
//                          the bit: a whole one (open, n == rate) gives np = (sI^2 + sQ^2) / w (0 when w is not > 0),
//                          kbits of them a window mean mu = npsum / kbits, nbad consecutive windows with mu < mu_min
//                          reason 2; the row then opens the next bit with empty sums
//
//   rx_lock   one wavefront per channel, GC_LOCK_WAVES channels per workgroup, the rows in chunks of 64 (lane = row).
//             Per chunk: the prompt sums go to the wavefront's LDS slice; a ballot of "synchronised and navbit != 0"
//             gives the chunk's bit ends, a ballot of the reason-1 condition and a find-first its earliest such row,
//             behind which the chunk counts for nothing.  The lane that owns a bit end sums its bit's rows from LDS in
//             period order (at most rate of them: a bit with another count is dropped unsummed), the chunk's first bit
//             continuing from the partial sums the state carries.  The closed bits are then walked in order for the
//             window logic.  The walk runs on wave-uniform values in every lane -- what lane 0 alone would compute --
//             so that the state needs no broadcast back: a bit's np comes to all lanes by one cross-lane read.  Last,
//             the rows behind the chunk's last bit end are summed into the carried partial sums, the same way.
//             No atomics, no scratch; the order of every sum is the period order whatever the chunking or the cut of
//             the stream into calls, so the states are bit-identical from run to run and from cut to cut.
#include <algorithm>
#include <vector>

#include "gnsscorr_ctx.h"

#define GC_LOCK_WAVES 4                         // channels per workgroup

namespace {

struct GcLockLds {
    double I[2][64], Q[2][64];                  // the chunk's prompt sums, two chunks deep
};

__device__ __forceinline__ unsigned long long lock_below(int p)    // bits 0 .. p-1, 0 <= p <= 64
{
    return p >= 64 ? ~0ULL : ((1ULL << p) - 1ULL);
}

// sI, sQ, w continued over the rows `rows` (a mask of the chunk's lanes) of the LDS copy, in period order
__device__ __forceinline__ void lock_sum(const double *li, const double *lq, unsigned long long rows, double &sI,
                                         double &sQ, double &w)
{
    while (rows) {
        const int j = __builtin_ctzll(rows);
        rows &= rows - 1ULL;
        const double x = li[j], y = lq[j];
        sI = __dadd_rn(sI, x);
        sQ = __dadd_rn(sQ, y);
        w = __dadd_rn(w, __dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y)));
    }
}

// chlist: the channels of the launch (nullptr: channel = list index), nlist of them.  I / Q: element
// ch * ch_stride + e * row_stride is the prompt sum of row e.  rate / cnt: byte pointers to channel 0's value and the
// byte stride to the next channel's; cnt_after: the value is the cnt behind the run (cnt0 = cnt - ndone), else cnt0.
// lostw: nullptr, or a word per channel: 1 when this launch declared the channel lost, else 0.
// grid ceil(nlist / GC_LOCK_WAVES), GC_LOCK_WAVES * 64 lanes.
__global__ __launch_bounds__(GC_LOCK_WAVES * 64) void rx_lock_kernel(
    const int *__restrict__ chlist, int nlist, const gnsscorr_lockprm_t *__restrict__ prm, const char *__restrict__ rate,
    size_t rate_stride, gnsscorr_lock_t *__restrict__ st, const double *__restrict__ I, const double *__restrict__ Q,
    size_t ch_stride, size_t row_stride, const gnsscorr_trklog_t *__restrict__ log, int nper,
    const int *__restrict__ ndone, const char *__restrict__ cnt, size_t cnt_stride, int cnt_after,
    unsigned *__restrict__ lostw)
{
    __shared__ GcLockLds lds[GC_LOCK_WAVES];
    __shared__ int rows_of[GC_LOCK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GcLockLds &L = lds[wave];
    const int li = blockIdx.x * GC_LOCK_WAVES + wave;
    const bool have = li < nlist;
    const int ch = have ? (chlist ? chlist[li] : li) : 0;
    gnsscorr_lockprm_t p = {0, 0, 0, 0, 0.0};
    gnsscorr_lock_t s = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int rt = 0, nd = 0;
    unsigned long long cnt0 = 0;
    if (have) {
        p = prm[ch];
        s = st[ch];
        rt = *reinterpret_cast<const int *>(rate + (size_t)ch * rate_stride);
        nd = min(max(ndone[ch], 0), nper);
        cnt0 = *reinterpret_cast<const unsigned long long *>(cnt + (size_t)ch * cnt_stride);
        if (cnt_after) cnt0 -= (unsigned long long)nd;
        if (p.kbits <= 0) nd = 0;                                           // the channel's monitor is off
    }
    // every wavefront of the workgroup walks as many chunks as its longest channel has: every one reaches every barrier
    if (lane == 0) rows_of[wave] = nd;
    __syncthreads();
    int most = 0;
    for (int i = 0; i < GC_LOCK_WAVES; i++) most = max(most, rows_of[i]);
    const int nchunk = (most + 63) >> 6;

    if (nd > 0 && cnt0 == 0) s = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0};    // row 0 is the period with cnt == 0
    bool live = nd > 0 && !s.lost;
    unsigned newly = 0;
    const double *pI = I + (size_t)ch * ch_stride, *pQ = Q + (size_t)ch * ch_stride;
    const gnsscorr_trklog_t *plog = log + (size_t)ch * (size_t)nper;

    for (int c = 0; c < nchunk; c++) {
        const int base = c << 6, e = base + lane, b = c & 1;
        const bool valid = live && e < nd;
        double vi = 0.0, vq = 0.0;
        int fs = 0, nb = 0;
        if (valid) {
            vi = pI[(size_t)e * row_stride];
            vq = pQ[(size_t)e * row_stride];
            fs = plog[e].flagsync;
            nb = plog[e].navbit;
        }
        L.I[b][lane] = vi;
        L.Q[b][lane] = vq;
        __syncthreads();
        if (!live) continue;
        // reason 1: the earliest unsynchronised row at or behind the time limit; rows from there on count for nothing
        const bool late = valid && fs == 0 && p.sync_periods > 0 &&
                          cnt0 + (unsigned long long)e + 1ULL >= (unsigned long long)p.sync_periods;
        const unsigned long long m1 = __ballot(late);
        const int p1 = m1 ? __builtin_ctzll(m1) : 64;
        const unsigned long long act = __ballot(valid && fs != 0) & lock_below(p1);         // rows that count
        const unsigned long long ends = __ballot(valid && fs != 0 && nb != 0) & lock_below(p1);
        // the owner of a bit end: its bit's rows are those that count behind the bit end before it
        double np = 0.0;
        int whole = 0;
        if ((ends >> lane) & 1ULL) {
            const unsigned long long before = ends & lock_below(lane);
            const int q = before ? 63 - __builtin_clzll(before) : -1;
            const unsigned long long rows = act & lock_below(lane + 1) & ~lock_below(q + 1);
            const int n = __popcll(rows) + (q < 0 ? s.n : 0);
            const int open = q < 0 ? s.open : 1;
            if (open && n == rt) {
                double sI = q < 0 ? s.sI : 0.0, sQ = q < 0 ? s.sQ : 0.0, w = q < 0 ? s.w : 0.0;
                lock_sum(L.I[b], L.Q[b], rows, sI, sQ, w);
                whole = 1;
                np = w > 0.0 ? __ddiv_rn(__dadd_rn(__dmul_rn(sI, sI), __dmul_rn(sQ, sQ)), w) : 0.0;
            }
        }
        // the closed bits in order: the window logic, on wave-uniform values
        int p2 = 64;
        for (unsigned long long m = ends; m;) {
            const int j = __builtin_ctzll(m);
            m &= m - 1ULL;
            const int whole_j = __shfl(whole, j, 64);
            const double np_j = __shfl(np, j, 64);
            if (!whole_j) continue;
            s.npsum = __dadd_rn(s.npsum, np_j);
            s.k++;
            if (s.k != p.kbits) continue;
            const double mu = __ddiv_rn(s.npsum, (double)p.kbits);
            s.mu_last = mu;
            s.windows++;
            s.nbad = mu < p.mu_min ? s.nbad + 1 : 0;
            s.k = 0;
            s.npsum = 0.0;
            if (s.nbad >= p.nbad) {
                s.lost = 1;
                s.reason = 2;
                s.lost_cnt = cnt0 + (unsigned long long)(base + j);
                p2 = j;
                break;
            }
        }
        if (p2 < 64) {                                                      // the losing row has opened the next bit
            s.open = 1;
            s.n = 0;
            s.sI = s.sQ = s.w = 0.0;
            live = false;
            newly = 1;
            continue;
        }
        // the rows behind the chunk's last bit end: the partial sums the next chunk (or call) continues from
        const int qlast = ends ? 63 - __builtin_clzll(ends) : -1;
        if (qlast >= 0) {
            s.open = 1;
            s.n = 0;
            s.sI = s.sQ = s.w = 0.0;
        }
        if (s.open) {
            const unsigned long long rows = act & ~lock_below(qlast + 1);
            s.n += __popcll(rows);
            lock_sum(L.I[b], L.Q[b], rows, s.sI, s.sQ, s.w);
        }
        if (p1 < 64) {
            s.lost = 1;
            s.reason = 1;
            s.lost_cnt = cnt0 + (unsigned long long)(base + p1);
            live = false;
            newly = 1;
        }
    }
    if (have && lane == 0) {
        st[ch] = s;
        if (lostw) lostw[ch] = newly;
    }
}

int lock_check_prm(const char *who, const gnsscorr_lockprm_t &p, int rate, int ch)
{
    if (rate < 2 || rate > 20) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: rate %d (2..20)", who, ch, rate);
    if (p.kbits < 1 || p.kbits > 4096) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: kbits %d (1..4096)", who, ch, p.kbits);
    if (p.nbad < 1) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: nbad %d (at least 1)", who, ch, p.nbad);
    if (p.sync_periods < 0) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: sync_periods %d (0: no limit)", who, ch, p.sync_periods);
    if (!(p.mu_min > 0.0 && p.mu_min <= (double)rate))
        return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: mu_min %g (above 0, at most the rate %d)", who, ch, p.mu_min, rate);
    return GNSSCORR_OK;
}

size_t lock_align(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace

extern "C" int gnsscorr_lock_run(gnsscorr_ctx *ctx, const gnsscorr_lockprm_t *prm, const int *rate, gnsscorr_lock_t *st,
                                 const double *I, const double *Q, const gnsscorr_trklog_t *log, const int *ndone,
                                 const uint64_t *cnt0, int nch, int nper)
{
    if (!ctx || !prm || !rate || !st || !I || !Q || !log || !ndone || !cnt0) return gc_fail(GNSSCORR_EINVAL, "lock_run: null argument");
    if (nch < 0 || nper < 1) return gc_fail(GNSSCORR_EINVAL, "lock_run: nch %d, nper %d", nch, nper);
    for (int i = 0; i < nch; i++) {
        int rc = lock_check_prm("lock_run", prm[i], rate[i], i);
        if (rc) return rc;
        if (ndone[i] < 0 || ndone[i] > nper) return gc_fail(GNSSCORR_EINVAL, "lock_run: channel %d: ndone %d of %d rows", i, ndone[i], nper);
    }
    if (nch == 0) return GNSSCORR_OK;
    std::lock_guard<std::mutex> lk(ctx->mtx);
    GC_HIP(hipSetDevice(ctx->device));
    // one staging buffer, one transfer: prm, rate, ndone, cnt0, st, I, Q, log
    const size_t units = (size_t)nch * nper;
    const size_t o_prm = 0, o_rate = lock_align(o_prm + sizeof(gnsscorr_lockprm_t) * nch), o_nd = lock_align(o_rate + sizeof(int) * nch),
                 o_cnt = lock_align(o_nd + sizeof(int) * nch), o_st = lock_align(o_cnt + sizeof(uint64_t) * nch),
                 o_I = lock_align(o_st + sizeof(gnsscorr_lock_t) * nch), o_Q = lock_align(o_I + sizeof(double) * units),
                 o_log = lock_align(o_Q + sizeof(double) * units), total = lock_align(o_log + sizeof(gnsscorr_trklog_t) * units);
    std::vector<unsigned char> blob(total, 0);
    memcpy(&blob[o_prm], prm, sizeof(gnsscorr_lockprm_t) * nch);
    memcpy(&blob[o_rate], rate, sizeof(int) * nch);
    memcpy(&blob[o_nd], ndone, sizeof(int) * nch);
    memcpy(&blob[o_cnt], cnt0, sizeof(uint64_t) * nch);
    memcpy(&blob[o_st], st, sizeof(gnsscorr_lock_t) * nch);
    memcpy(&blob[o_I], I, sizeof(double) * units);
    memcpy(&blob[o_Q], Q, sizeof(double) * units);
    memcpy(&blob[o_log], log, sizeof(gnsscorr_trklog_t) * units);
    GC_RESERVE(ctx, ctx->dlock_stage, total);
    unsigned char *d = ctx->dlock_stage;
    GC_HIP(hipMemcpyAsync(d, blob.data(), total, hipMemcpyHostToDevice, ctx->stream));
    {
        GcTimed t(ctx, "rx_lock");
        hipLaunchKernelGGL(rx_lock_kernel, dim3((nch + GC_LOCK_WAVES - 1) / GC_LOCK_WAVES), dim3(GC_LOCK_WAVES * 64), 0, ctx->stream,
                           (const int *)nullptr, nch, (const gnsscorr_lockprm_t *)(d + o_prm), (const char *)(d + o_rate), sizeof(int),
                           (gnsscorr_lock_t *)(d + o_st), (const double *)(d + o_I), (const double *)(d + o_Q), (size_t)nper, (size_t)1,
                           (const gnsscorr_trklog_t *)(d + o_log), nper, (const int *)(d + o_nd), (const char *)(d + o_cnt),
                           sizeof(uint64_t), 0, (unsigned *)nullptr);
    }
    GC_HIP(hipGetLastError());
    std::vector<gnsscorr_lock_t> out(nch);
    GC_HIP(hipMemcpyAsync(out.data(), d + o_st, sizeof(gnsscorr_lock_t) * nch, hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(st, out.data(), sizeof(gnsscorr_lock_t) * nch);
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_rx_lock_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_lockprm_t *prm)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_lock_set: no gnsscorr_rx_start yet");
    if (ch0 < 0 || nch < 0 || ch0 + nch > ctx->nch) return gc_fail(GNSSCORR_EINVAL, "rx_lock_set: channels %d..%d of %d", ch0, ch0 + nch - 1, ctx->nch);
    if (nch == 0) return GNSSCORR_OK;
    GC_HIP(hipSetDevice(ctx->device));
    GcRx &rx = ctx->rx;
    gnsscorr_lockprm_t p = {0, 0, 0, 0, 0.0};
    if (prm && prm->kbits != 0) {
        p = *prm;
        p.pad = 0;
        // the channels' nav bit lengths: one column of the device's loop states
        std::vector<int> rate(nch);
        GC_HIP(hipMemcpy2DAsync(rate.data(), sizeof(int), (const char *)(ctx->loop.dloop.p + ch0) + offsetof(gnsscorr_loop_t, rate),
                                sizeof(gnsscorr_loop_t), sizeof(int), nch, hipMemcpyDeviceToHost, ctx->stream));
        GC_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < nch; i++) {
            int rc = lock_check_prm("rx_lock_set", p, rate[i], ch0 + i);
            if (rc) return rc;
        }
    }
    GC_RESERVE(ctx, rx.dlockprm, ctx->nch);
    GC_RESERVE(ctx, rx.dlock, ctx->nch);
    { int rc = rx.lock_list.reserve(ctx->nch, hipHostMallocMapped); if (rc) return rc; }
    { int rc = rx.lock_lost.reserve(ctx->nch, hipHostMallocMapped); if (rc) return rc; }
    GC_TRY(ctx->ev_lock.make());
    for (int i = 0; i < nch; i++) rx.lockprm[ch0 + i] = p;
    rx.lock_on = 0;
    for (int i = 0; i < ctx->nch; i++) rx.lock_on += rx.lockprm[i].kbits != 0;
    // behind whatever the stream still runs (a monitor launch of the last step included: its verdicts stay to be read)
    GC_HIP(hipStreamSynchronize(ctx->stream));
    GC_HIP(hipMemcpy(rx.dlockprm.p, rx.lockprm.data(), sizeof(gnsscorr_lockprm_t) * ctx->nch, hipMemcpyHostToDevice));
    GC_HIP(hipMemset(rx.dlock.p + ch0, 0, sizeof(gnsscorr_lock_t) * nch));
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_rx_lock_status(gnsscorr_ctx *ctx, gnsscorr_lock_t *st, int *losses)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_lock_status: no gnsscorr_rx_start yet");
    GC_HIP(hipSetDevice(ctx->device));
    const int nch = ctx->nch;
    if (st) {
        if (ctx->rx.dlock) GC_HIP(hipMemcpyAsync(st, ctx->rx.dlock, sizeof(gnsscorr_lock_t) * nch, hipMemcpyDeviceToHost, ctx->stream));
        else memset(st, 0, sizeof(gnsscorr_lock_t) * nch);                  // the monitor has never been on
    }
    GC_HIP(hipStreamSynchronize(ctx->stream));
    if (losses) for (int i = 0; i < nch; i++) losses[i] = ctx->rx.losses[i];
    return GNSSCORR_OK;
}

int gc_rx_lock_launch(gnsscorr_ctx *ctx, int nperiod)
{
    GcRx &rx = ctx->rx;
    rx.lock_listed.clear();
    for (int i = 0; i < ctx->nch; i++)
        if (rx.lockprm[i].kbits != 0 && rx.st[i].state == GNSSCORR_CH_TRACK) rx.lock_listed.push_back(i);
    const int n = (int)rx.lock_listed.size();
    if (!n) return GNSSCORR_OK;
    // the previous launch's event has been waited for (step 0): the kernel that read the list is over
    for (int i = 0; i < n; i++) {
        rx.lock_list[i] = rx.lock_listed[i];
        rx.lock_lost[rx.lock_listed[i]] = 0;
    }
    {
        GcTimed t(ctx, "rx_lock");
        // trk.II is the correlator's QQ (ref src/sdrtrk.c:42): gnsscorr_trk_fetch's II rows are dcorrQ
        hipLaunchKernelGGL(rx_lock_kernel, dim3((n + GC_LOCK_WAVES - 1) / GC_LOCK_WAVES), dim3(GC_LOCK_WAVES * 64), 0, ctx->stream,
                           (const int *)rx.lock_list.dev, n, (const gnsscorr_lockprm_t *)rx.dlockprm.p,
                           (const char *)ctx->loop.dloop.p + offsetof(gnsscorr_loop_t, rate), sizeof(gnsscorr_loop_t), rx.dlock.p,
                           (const double *)ctx->out.dcorrQ.p, (const double *)ctx->out.dcorrI.p, (size_t)nperiod * ctx->ntap, (size_t)ctx->ntap,
                           (const gnsscorr_trklog_t *)ctx->loop.dlog.p, nperiod, (const int *)ctx->loop.ddone.p,
                           (const char *)ctx->loop.dloop.p + offsetof(gnsscorr_loop_t, cnt), sizeof(gnsscorr_loop_t), 1,
                           rx.lock_lost.dev);
    }
    GC_HIP(hipGetLastError());
    GC_HIP(hipEventRecord(ctx->ev_lock, ctx->stream));
    ctx->lock_pending = true;
    return GNSSCORR_OK;
}
