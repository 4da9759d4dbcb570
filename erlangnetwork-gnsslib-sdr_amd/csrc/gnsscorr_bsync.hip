// gnsscorr_bsync.hip -- bit synchronisation by symbol energy for gfx950 (MI355X): a preset of flagsync / synci from the
// first tracked periods of a channel, in front of the reference's checksync() (nav_checksync, gnsscorr_loop.hip), which
// starts only after cnt > 2000 and whose shift-register branch takes the first `rate` prompts of one sign for a symbol.
//
// The detector (include/gnsscorr.h; every arithmetic statement one IEEE double operation, sums in period
// order), per channel over the rows e < ndone of one closed-loop run, c = cnt0 + e, R = the channel's rate:
//   1. c == 0              the state is zeroed (first period behind a hand-over)
//   2. done != 0           sticky: nothing more is read
//   3. flagsync[e] != 0    done = 3: the loop synchronised by its own rule, or was preset
//   4. c < start_cnt       the row does not count
//   5. first counted row   armed = 1, a0 = c
//   6. offsets o < R       if fill[o] > 0 or c mod R == o: sI[o] += I, sQ[o] += Q, fill[o]++; at fill[o] == R the symbol
//                          closes: E[o] += sI[o]^2 + sQ[o]^2, sums and fill cleared
//   7. L = c - a0 + 1      when (L + 1) mod R == 0 every offset has closed n = (L + 1)/R - 1 symbols; at n >= 1 and
//                          n mod nsym == 0 a test: o* = argmax E (lowest index), h = (o* + R/2) mod R, pass when
//                          E[o*] > 0 and E[o*] >= gate * E[h]: done = 1, synci = (o* + R - 1) mod R; else done = 2 once
//                          n >= nsym_max
//
//   rx_bsync  one wavefront per channel, GC_BSYNC_WAVES channels per workgroup, the rows in chunks of 64 through the
//             wavefront's LDS slice (lane = row while staging).  Lane o < R owns offset o: E, sI, sQ and fill of its
//             offset stay in its registers while every lane walks the chunk's rows from LDS in period order, all lanes
//             reading one address, the next row's read in flight.  A ballot of the rows' flagsync gives the row at
//             which rule 3 ends the walk; the rows in front of start_cnt are skipped at once; cnt mod R and rule 7's
//             (L + 1) mod R and (L + 1) / R are carried from row to row, so a row costs no division.  The test of rule 7
//             gathers the R energies by cross-lane reads and runs on wave-uniform values in every lane, so the scalar
//             part of the state needs no broadcast back.  No atomics, no scratch; the order of every sum is the period
//             order whatever the chunking or the cut of the stream into calls, so the states are bit-identical from run
//             to run and from cut to cut.  In the schedule the same kernel presets the loop state of a channel it
//             decided in this launch.
#include <algorithm>
#include <vector>

#include "gnsscorr_stage.h"

#define GC_BSYNC_WAVES 4                        // channels per workgroup
#define GC_BSYNC_MAXRATE 20                     // gnsscorr_bsync_t's arrays, gnsscorr_loop_t.bitsync[]

namespace {

struct GcBsyncLds {
    double I[2][64], Q[2][64];                  // the chunk's prompt sums, two chunks deep
};

// v: the rows (GcRowsView, gnsscorr_stage.h).  loop: nullptr, or the loop states [channel]: a channel decided in this
// launch (done 0 -> 1) whose flagsync is still 0 gets flagsync = 1 and synci, and applied[channel] goes up by one.
// grid ceil(nlist / GC_BSYNC_WAVES), GC_BSYNC_WAVES * 64 lanes.
__global__ __launch_bounds__(GC_BSYNC_WAVES * 64) void rx_bsync_kernel(const GcRowsView v, const gnsscorr_bsyncprm_t *__restrict__ prm,
                                                                       gnsscorr_bsync_t *__restrict__ st, gnsscorr_loop_t *loop,
                                                                       int *__restrict__ applied)
{
    GC_FP_STRICT                                // plain operators below, one IEEE operation each: no product is fused into a sum
    __shared__ GcBsyncLds lds[GC_BSYNC_WAVES];
    __shared__ int rows_of[GC_BSYNC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GcBsyncLds &L = lds[wave];
    const GcRows r = gc_rows(v, blockIdx.x * GC_BSYNC_WAVES + wave);
    const bool have = r.have;
    const int ch = r.ch, rt = have ? r.rt : 2;  // (a wavefront without a channel still divides by its rate)
    const unsigned long long cnt0 = r.cnt0;
    const bool own = lane < GC_BSYNC_MAXRATE;   // the lane holds an element of the state's arrays
    gnsscorr_bsyncprm_t p = {0, 0, 0, 0, 0.0};
    int nd = r.nd;
    // the state: the arrays by lane, the rest wave-uniform
    double E = 0.0, sI = 0.0, sQ = 0.0, ratio_last = 0.0;
    unsigned long long a0 = 0, decided_cnt = 0;
    int fill = 0, armed = 0, n = 0, tests = 0, done = 0, best = 0, synci = 0;
    if (have) {
        p = prm[ch];
        if (p.nsym <= 0 || rt < 2 || rt > GC_BSYNC_MAXRATE) nd = 0;         // the channel's detector is off
        const gnsscorr_bsync_t &s = st[ch];
        if (own) {
            E = s.E[lane];
            sI = s.sI[lane];
            sQ = s.sQ[lane];
            fill = s.fill[lane];
        }
        ratio_last = s.ratio_last;
        a0 = s.a0;
        decided_cnt = s.decided_cnt;
        armed = s.armed; n = s.n; tests = s.tests; done = s.done; best = s.best; synci = s.synci;
    }
    // every wavefront of the workgroup walks as many chunks as its longest channel has: every one reaches every barrier
    if (lane == 0) rows_of[wave] = nd;
    __syncthreads();
    int most = 0;
    for (int i = 0; i < GC_BSYNC_WAVES; i++) most = max(most, rows_of[i]);
    const int nchunk = (most + 63) >> 6;

    if (nd > 0 && cnt0 == 0) {                                              // rule 1: row 0 is the period with cnt == 0
        E = sI = sQ = ratio_last = 0.0;
        a0 = decided_cnt = 0;
        fill = armed = n = tests = done = best = synci = 0;
    }
    bool live = nd > 0 && !done;                                            // rule 2
    int newly = 0;
    int phase = (int)(cnt0 % (unsigned long long)rt);                      // c mod R, carried from row to row
    const double *pI = r.pI, *pQ = r.pQ;
    const gnsscorr_trklog_t *plog = r.plog;
    const size_t row_stride = v.row_stride;

    for (int k = 0; k < nchunk; k++) {
        const int base = k << 6, e = base + lane, b = k & 1;
        const bool valid = live && e < nd;
        double vi = 0.0, vq = 0.0;
        int fs = 0;
        if (valid) {
            vi = pI[(size_t)e * row_stride];
            vq = pQ[(size_t)e * row_stride];
            fs = plog[e].flagsync;
        }
        L.I[b][lane] = vi;
        L.Q[b][lane] = vq;
        __syncthreads();
        if (!live) continue;
        const int nrows = min(64, nd - base);
        // rule 3: the chunk's first synchronised row, in front of which the walk ends
        const unsigned long long m3 = __ballot(valid && fs != 0);
        const int p3 = m3 ? __builtin_ctzll(m3) : 64;
        const int jend = min(nrows, p3);
        const unsigned long long cb = cnt0 + (unsigned long long)base;     // c of the chunk's row 0
        // rule 4: the rows in front of start_cnt only advance c mod R
        int j = 0;
        if (cb < (unsigned long long)p.start_cnt) {
            const unsigned long long gap = (unsigned long long)p.start_cnt - cb;
            j = gap < (unsigned long long)jend ? (int)gap : jend;
            phase = (phase + j) % rt;
        }
        if (j < jend) {
            if (!armed) {                                                   // rule 5
                armed = 1;
                a0 = cb + (unsigned long long)j;
            }
            // rule 7's L + 1 of row j as (L + 1) mod R and (L + 1) / R, carried from row to row
            const unsigned len1 = (unsigned)(cb + (unsigned long long)j - a0) + 2u;
            int lm = (int)(len1 % (unsigned)rt), lq = (int)(len1 / (unsigned)rt);
            double x = L.I[b][j], y = L.Q[b][j];
            for (; j < jend; j++) {
                const double xn = L.I[b][(j + 1) & 63], yn = L.Q[b][(j + 1) & 63];      // the next row, in flight
                if (lane < rt && (fill > 0 || phase == lane)) {             // rule 6: lane o is offset o
                    sI = sI + x;
                    sQ = sQ + y;
                    fill++;
                    if (fill == rt) {
                        const double ii = sI * sI, qq = sQ * sQ;
                        E = E + (ii + qq);
                        sI = sQ = 0.0;
                        fill = 0;
                    }
                }
                if (lm == 0) {                                              // rule 7: (L + 1) mod R == 0
                    n = lq - 1;
                    if (n >= 1 && n % p.nsym == 0) {
                        double eb = __shfl(E, 0, 64);
                        int ob = 0;
                        for (int o = 1; o < rt; o++) {
                            const double eo = __shfl(E, o, 64);
                            if (eo > eb) {
                                eb = eo;
                                ob = o;
                            }
                        }
                        int h = ob + rt / 2;
                        if (h >= rt) h -= rt;
                        const double eh = __shfl(E, h, 64);
                        tests++;
                        ratio_last = eh > 0.0 ? eb / eh : 0.0;
                        if (eb > 0.0 && eb >= p.gate * eh) {
                            done = 1;
                            best = ob;
                            synci = ob == 0 ? rt - 1 : ob - 1;
                            decided_cnt = cb + (unsigned long long)j;
                            newly = 1;
                        } else if (n >= p.nsym_max) {
                            done = 2;
                        }
                        if (done) {
                            live = false;
                            break;
                        }
                    }
                }
                if (++lm == rt) {
                    lm = 0;
                    lq++;
                }
                phase = phase + 1 == rt ? 0 : phase + 1;
                x = xn;
                y = yn;
            }
        }
        if (live && p3 < nrows) {                                           // the walk reached the synchronised row
            done = 3;
            live = false;
        }
    }
    if (!have || nd <= 0) return;                                           // (every barrier is behind)
    gnsscorr_bsync_t &s = st[ch];
    if (own) {
        s.E[lane] = E;
        s.sI[lane] = sI;
        s.sQ[lane] = sQ;
        s.fill[lane] = fill;
    }
    if (lane == 0) {
        s.ratio_last = ratio_last;
        s.a0 = a0;
        s.decided_cnt = decided_cnt;
        s.armed = armed; s.n = n; s.tests = tests; s.done = done; s.best = best; s.synci = synci;
        if (newly && loop) {
            gnsscorr_loop_t *lp = loop + ch;
            if (lp->flagsync == 0) {
                lp->flagsync = 1;
                lp->synci = synci;
                applied[ch] += 1;
            }
        }
    }
}

int bsync_check_prm(const char *who, const gnsscorr_bsyncprm_t &p, int rate, int ch)
{
    if (rate < 2 || rate > GC_BSYNC_MAXRATE) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: rate %d (2..20)", who, ch, rate);
    if (p.start_cnt < 0) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: start_cnt %d (at least 0)", who, ch, p.start_cnt);
    if (p.nsym_max < 1 || p.nsym_max > 4096)
        return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: nsym_max %d (1..4096)", who, ch, p.nsym_max);
    if (p.nsym < 1 || p.nsym > p.nsym_max)
        return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: nsym %d (1..nsym_max %d)", who, ch, p.nsym, p.nsym_max);
    if (!(p.gate >= 1.0)) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: gate %g (at least 1)", who, ch, p.gate);
    return GNSSCORR_OK;
}

void bsync_launch(gnsscorr_ctx *ctx, const GcRowsView &rows, const gnsscorr_bsyncprm_t *prm, gnsscorr_bsync_t *st, gnsscorr_loop_t *loop,
                  int *applied)
{
    GcTimed t(ctx, "rx_bsync");
    hipLaunchKernelGGL(rx_bsync_kernel, dim3((rows.nlist + GC_BSYNC_WAVES - 1) / GC_BSYNC_WAVES), dim3(GC_BSYNC_WAVES * 64), 0, ctx->stream,
                       rows, prm, st, loop, applied);
}

}  // namespace

extern "C" int gnsscorr_bsync_run(gnsscorr_ctx *ctx, const gnsscorr_bsyncprm_t *prm, const int *rate, gnsscorr_bsync_t *st,
                                  const double *I, const double *Q, const gnsscorr_trklog_t *log, const int *ndone,
                                  const uint64_t *cnt0, int nch, int nper)
{
    if (!ctx || !prm || !rate || !st || !I || !Q || !log || !ndone || !cnt0) return gc_fail(GNSSCORR_EINVAL, "bsync_run: null argument");
    if (nch < 0 || nper < 1) return gc_fail(GNSSCORR_EINVAL, "bsync_run: nch %d, nper %d", nch, nper);
    for (int i = 0; i < nch; i++) {
        if (prm[i].nsym != 0) {
            int rc = bsync_check_prm("bsync_run", prm[i], rate[i], i);
            if (rc) return rc;
        }
        if (ndone[i] < 0 || ndone[i] > nper) return gc_fail(GNSSCORR_EINVAL, "bsync_run: channel %d: ndone %d of %d rows", i, ndone[i], nper);
    }
    if (nch == 0) return GNSSCORR_OK;
    return gc_stage_run(ctx, prm, rate, st, I, Q, log, ndone, cnt0, nch, nper, 1,
                        [&](const GcRowsView &rows, const gnsscorr_bsyncprm_t *dprm, gnsscorr_bsync_t *dst) {
                            bsync_launch(ctx, rows, dprm, dst, nullptr, nullptr);
                        });
}

extern "C" int gnsscorr_rx_bsync_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_bsyncprm_t *prm)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_bsync_set: no gnsscorr_rx_start yet");
    GC_HIP(hipSetDevice(ctx->device));
    GcRx &rx = ctx->rx;
    // the detector's own, before it can be on: the applied counts, which no kernel has seen when they are made
    if (!rx.dbsync_applied) {
        GC_RESERVE(ctx, rx.dbsync_applied, ctx->nch);
        GC_HIP(hipMemset(rx.dbsync_applied.p, 0, sizeof(int) * ctx->nch));
    }
    gnsscorr_bsyncprm_t p = {0, 0, 0, 0, 0.0};
    if (prm && prm->nsym != 0) {
        p = *prm;
        p.pad = 0;
    }
    return rx.bsync.set(ctx, "rx_bsync_set", ch0, nch, p, bsync_check_prm);
}

extern "C" int gnsscorr_rx_bsync_status(gnsscorr_ctx *ctx, gnsscorr_bsync_t *st, int *applied)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_bsync_status: no gnsscorr_rx_start yet");
    GC_HIP(hipSetDevice(ctx->device));
    const int nch = ctx->nch;
    if (st) GC_TRY(ctx->rx.bsync.status(ctx, st));
    if (applied) {
        if (ctx->rx.dbsync_applied) GC_HIP(hipMemcpyAsync(applied, ctx->rx.dbsync_applied, sizeof(int) * nch, hipMemcpyDeviceToHost, ctx->stream));
        else memset(applied, 0, sizeof(int) * nch);                         // the detector has never been on
    }
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

int gc_rx_bsync_launch(gnsscorr_ctx *ctx, int nperiod)
{
    GcRx &rx = ctx->rx;
    const int n = rx.bsync.fill(rx.st);
    if (!n) return GNSSCORR_OK;
    bsync_launch(ctx, gc_rows_of_run(ctx, rx.bsync.list.dev, n, nperiod), rx.bsync.dprm, rx.bsync.dst, ctx->loop.dloop, rx.dbsync_applied);
    GC_HIP(hipGetLastError());
    return GNSSCORR_OK;
}
