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

#include "gnsscorr_stage.h"

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

// v: the rows (GcRowsView, gnsscorr_stage.h).  lostw: nullptr, or a word per channel: 1 when this launch declared the
// channel lost, else 0.  grid ceil(nlist / GC_LOCK_WAVES), GC_LOCK_WAVES * 64 lanes.
__global__ __launch_bounds__(GC_LOCK_WAVES * 64) void rx_lock_kernel(const GcRowsView v, const gnsscorr_lockprm_t *__restrict__ prm,
                                                                     gnsscorr_lock_t *__restrict__ st, unsigned *__restrict__ lostw)
{
    __shared__ GcLockLds lds[GC_LOCK_WAVES];
    __shared__ int rows_of[GC_LOCK_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GcLockLds &L = lds[wave];
    const GcRows r = gc_rows(v, blockIdx.x * GC_LOCK_WAVES + wave);
    const bool have = r.have;
    const int ch = r.ch, rt = r.rt;
    const unsigned long long cnt0 = r.cnt0;
    gnsscorr_lockprm_t p = {0, 0, 0, 0, 0.0};
    gnsscorr_lock_t s = {0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int nd = r.nd;
    if (have) {
        p = prm[ch];
        s = st[ch];
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
    const double *pI = r.pI, *pQ = r.pQ;
    const gnsscorr_trklog_t *plog = r.plog;
    const size_t row_stride = v.row_stride;

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

void lock_launch(gnsscorr_ctx *ctx, const GcRowsView &rows, const gnsscorr_lockprm_t *prm, gnsscorr_lock_t *st, unsigned *lostw)
{
    GcTimed t(ctx, "rx_lock");
    hipLaunchKernelGGL(rx_lock_kernel, dim3((rows.nlist + GC_LOCK_WAVES - 1) / GC_LOCK_WAVES), dim3(GC_LOCK_WAVES * 64), 0, ctx->stream,
                       rows, prm, st, lostw);
}

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
    return gc_stage_run(ctx, prm, rate, st, I, Q, log, ndone, cnt0, nch, nper, 1,
                        [&](const GcRowsView &rows, const gnsscorr_lockprm_t *dprm, gnsscorr_lock_t *dst) { lock_launch(ctx, rows, dprm, dst, nullptr); });
}

extern "C" int gnsscorr_rx_lock_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_lockprm_t *prm)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_lock_set: no gnsscorr_rx_start yet");
    GC_HIP(hipSetDevice(ctx->device));
    GcRx &rx = ctx->rx;
    // the monitor's own, before it can be on: the verdict words and the end of a launch
    GC_TRY(rx.lock_lost.reserve(ctx->nch, hipHostMallocMapped));
    GC_TRY(ctx->ev_lock.make());
    gnsscorr_lockprm_t p = {0, 0, 0, 0, 0.0};
    if (prm && prm->kbits != 0) {
        p = *prm;
        p.pad = 0;
    }
    return rx.lock.set(ctx, "rx_lock_set", ch0, nch, p, lock_check_prm);
}

extern "C" int gnsscorr_rx_lock_status(gnsscorr_ctx *ctx, gnsscorr_lock_t *st, int *losses)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_lock_status: no gnsscorr_rx_start yet");
    GC_HIP(hipSetDevice(ctx->device));
    if (st) GC_TRY(ctx->rx.lock.status(ctx, st));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    if (losses) for (int i = 0; i < ctx->nch; i++) losses[i] = ctx->rx.losses[i];
    return GNSSCORR_OK;
}

int gc_rx_lock_launch(gnsscorr_ctx *ctx, int nperiod)
{
    GcRx &rx = ctx->rx;
    const int n = rx.lock.fill(rx.st);
    rx.lock_listed.assign(rx.lock.list.p, rx.lock.list.p + n);
    if (!n) return GNSSCORR_OK;
    for (int i : rx.lock_listed) rx.lock_lost[i] = 0;
    lock_launch(ctx, gc_rows_of_run(ctx, rx.lock.list.dev, n, nperiod), rx.lock.dprm, rx.lock.dst, rx.lock_lost.dev);
    GC_HIP(hipGetLastError());
    GC_HIP(hipEventRecord(ctx->ev_lock, ctx->stream));
    ctx->lock_pending = true;
    return GNSSCORR_OK;
}
