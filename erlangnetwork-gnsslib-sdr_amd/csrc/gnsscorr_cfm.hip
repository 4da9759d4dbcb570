// gnsscorr_cfm.hip -- the correlation monitor for gfx950 (MI355X): every tap of a tracking channel summed over whole nav
// bits, wiped of the data bit and added up over windows of kbits bits, and the early-minus-late and early-plus-late
// tests of signal quality monitoring on each window (multipath, spoofing).  The engine computes up to 33 taps per
// channel and period; the loops read three of them and the reference plots the rest.  The monitor reports and never
// acts: it writes no loop, tracking or schedule state.
//
// The monitor (include/gnsscorr.h; every arithmetic statement one IEEE double operation, sums in period
// order, window sums in bit order), per channel over the rows e < ndone of one closed-loop run, c = cnt0 + e,
// R = the channel's rate, T = 1 + 2 corrn taps {P, E1, L1, E2, L2, ...}:
//   c == 0                 the state is zeroed (first period behind a hand-over)
//   flagsync[e] == 0       the row counts for nothing
//   otherwise              while a bit is open, sI[t] += I_t, sQ[t] += Q_t for t < T, n += 1.  A row with navbit != 0
//                          closes the bit: a whole one (open, n == R) counts (bits += 1) and, behind the first skip_bits
//                          of them, goes into the window with d = the decided bit: aI[t] += d sI[t], aQ[t] += d sQ[t],
//                          aP[t] += sI[t]^2 + sQ[t]^2, k += 1.  At k == kbits the window closes: cfI / cfQ / cfP are the
//                          sums, P = cfI[0], delta[j-1] = (cfI[2j-1] - cfI[2j]) / P and ratio[j-1] = (cfI[2j-1] +
//                          cfI[2j]) / P for j <= corrn when P > 0, else 0; the window is bad when P is not > 0 or a
//                          pair j <= npair has |delta - dref| > dtol or |ratio - rref| > rtol (worst_pair: the first);
//                          nbad consecutive bad windows raise alarm, a good one clears it.  The row then opens the next
//                          bit with empty sums.
//
//   rx_cfm    one wavefront per listed channel, GC_CFM_WAVES channels per workgroup, the rows in chunks of 64.  Lane
//             t < 33 owns element t of the state's arrays -- sI, sQ, aI, aQ, aP, cfI, cfQ, cfP stay in its registers for
//             the whole launch -- and lane j - 1 < 16 owns delta / ratio / dref / rref of pair j.  Per chunk lane = row
//             reads the row's flagsync and navbit, and three ballots (synchronised, bit end, bit positive) turn them
//             into wave-uniform masks: the bit, skip and window logic then runs on scalar values in every lane, so the
//             scalar part of the state needs no broadcast back, and no row control passes through memory again (no
//             LDS, no barrier).  The data rows are read GC_CFM_ROWS at a time, all their loads in flight before the
//             first is added: a row's T doubles are consecutive, lane t reads element t.  A group of rows without a
//             synchronised one is not read at all, so a channel costs nothing before bit synchronisation.  A window's
//             close gathers the pair's taps by cross-lane reads (lanes 2j-1, 2j and 0) and the verdict by one ballot.
//             No atomics, no scratch; the order of every sum is the period order whatever the chunking or the cut of
//             the stream into calls, so the states are bit-identical from run to run and from cut to cut.
#include <algorithm>
#include <cmath>
#include <vector>

#include "gnsscorr_stage.h"

#define GC_CFM_WAVES 4                          // channels per workgroup
#define GC_CFM_ROWS 8                           // data rows in flight (divides 64)
#define GC_CFM_MAXPAIR 16                       // gnsscorr_cfm_t's delta / ratio, gnsscorr_cfmprm_t's dref / rref

namespace {

// v: the rows (GcRowsView, gnsscorr_stage.h), tap t of a row at + t; ntap = 1 + 2 corrn <= row_stride.
// grid ceil(nlist / GC_CFM_WAVES), GC_CFM_WAVES * 64 lanes.
__global__ __launch_bounds__(GC_CFM_WAVES * 64) void rx_cfm_kernel(const GcRowsView v, const gnsscorr_cfmprm_t *__restrict__ prm,
                                                                   gnsscorr_cfm_t *__restrict__ st, int ntap)
{
    GC_FP_STRICT                                // plain operators below, one IEEE operation each: no product is fused into a sum
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GcRows r = gc_rows(v, blockIdx.x * GC_CFM_WAVES + wave);
    if (!r.have) return;                                                    // (the kernel has no barrier)
    const int ch = r.ch, rt = r.rt, nd = r.nd;
    const unsigned long long cnt0 = r.cnt0;
    const gnsscorr_cfmprm_t &p = prm[ch];
    const int kbits = p.kbits, skip_bits = p.skip_bits, nbad_max = p.nbad, npair = p.npair;
    const double dtol = p.dtol, rtol = p.rtol;
    if (nd <= 0 || kbits <= 0 || rt < 2 || ntap < 3 || ntap > GNSSCORR_MAXTAPS) return;    // nothing to read, or the monitor is off
    const int corrn = (ntap - 1) >> 1;
    const bool own = lane < GNSSCORR_MAXTAPS;   // the lane holds an element of the state's tap arrays
    const bool tap = lane < ntap;               // ... of a tap the channel has
    const bool pair = lane < GC_CFM_MAXPAIR;    // ... and delta / ratio of pair lane + 1
    gnsscorr_cfm_t &s = st[ch];
    // the state: the arrays by lane, the rest wave-uniform
    double sI = 0.0, sQ = 0.0, aI = 0.0, aQ = 0.0, aP = 0.0, cfI = 0.0, cfQ = 0.0, cfP = 0.0, delta = 0.0, ratio = 0.0;
    double dref = 0.0, rref = 0.0;
    unsigned long long win_cnt = 0;
    int open = 0, n = 0, k = 0, bits = 0, nbad = 0, alarm = 0, alarms = 0, windows = 0, worst = 0;
    if (pair) {
        dref = p.dref[lane];
        rref = p.rref[lane];
    }
    if (cnt0 != 0) {                                                        // else row 0 is the period with cnt == 0
        if (own) {
            sI = s.sI[lane]; sQ = s.sQ[lane];
            aI = s.aI[lane]; aQ = s.aQ[lane]; aP = s.aP[lane];
            cfI = s.cfI[lane]; cfQ = s.cfQ[lane]; cfP = s.cfP[lane];
        }
        if (pair) {
            delta = s.delta[lane];
            ratio = s.ratio[lane];
        }
        win_cnt = s.win_cnt;
        open = s.open; n = s.n; k = s.k; bits = s.bits; nbad = s.nbad; alarm = s.alarm; alarms = s.alarms;
        windows = s.windows; worst = s.worst_pair;
    }
    const double *pI = r.pI + lane, *pQ = r.pQ + lane;
    const gnsscorr_trklog_t *plog = r.plog;
    const size_t row_stride = v.row_stride;

    for (int base = 0; base < nd; base += 64) {
        const int e = base + lane;
        int fs = 0, nb = 0;
        if (e < nd) {
            fs = plog[e].flagsync;
            nb = plog[e].navbit;
        }
        const unsigned long long mfs = __ballot(fs != 0);                   // the rows that count
        if (!mfs) continue;
        const unsigned long long mend = __ballot(fs != 0 && nb != 0), mpos = __ballot(nb > 0);
        for (int g = 0; g < 64; g += GC_CFM_ROWS) {
            const unsigned gm = (unsigned)(mfs >> g) & ((1u << GC_CFM_ROWS) - 1u);
            if (!gm) continue;
            // the group's rows, every load issued before the first sum (rows behind the run re-read its last row)
            double xi[GC_CFM_ROWS], xq[GC_CFM_ROWS];
#pragma unroll
            for (int r = 0; r < GC_CFM_ROWS; r++) xi[r] = xq[r] = 0.0;
            if (tap) {
#pragma unroll
                for (int r = 0; r < GC_CFM_ROWS; r++) {
                    const size_t row = (size_t)min(base + g + r, nd - 1) * row_stride;
                    xi[r] = pI[row];
                    xq[r] = pQ[row];
                }
            }
#pragma unroll
            for (int r = 0; r < GC_CFM_ROWS; r++) {
                if (!((gm >> r) & 1u)) continue;
                const int j = g + r;
                if (open) {
                    if (tap) {
                        sI = sI + xi[r];
                        sQ = sQ + xq[r];
                    }
                    n++;
                }
                if (!((mend >> j) & 1ULL)) continue;
                if (open && n == rt) {                                      // a whole bit
                    bits++;
                    if (bits > skip_bits) {
                        const double d = ((mpos >> j) & 1ULL) ? 1.0 : -1.0;
                        if (tap) {
                            const double wi = d * sI, wq = d * sQ, ii = sI * sI, qq = sQ * sQ;
                            aI = aI + wi;
                            aQ = aQ + wq;
                            aP = aP + (ii + qq);
                        }
                        k++;
                        if (k == kbits) {                                   // the window closes
                            cfI = aI;
                            cfQ = aQ;
                            cfP = aP;
                            win_cnt = cnt0 + (unsigned long long)(base + j);
                            windows++;
                            const double P = __shfl(cfI, 0, 64);
                            const double ce = __shfl(cfI, (2 * lane + 1) & 63, 64), cl = __shfl(cfI, (2 * lane + 2) & 63, 64);
                            const bool pos = P > 0.0;
                            if (pos && lane < corrn) {
                                const double dm = ce - cl, sm = ce + cl;
                                delta = dm / P;
                                ratio = sm / P;
                            } else {
                                delta = ratio = 0.0;
                            }
                            const double dd = delta - dref, dr = ratio - rref;
                            const unsigned long long mf = __ballot(lane < npair && (fabs(dd) > dtol || fabs(dr) > rtol));
                            worst = mf ? __builtin_ctzll(mf) + 1 : 0;
                            nbad = (!pos || mf) ? nbad + 1 : 0;
                            alarm = nbad >= nbad_max ? 1 : 0;
                            alarms += alarm;
                            aI = aQ = aP = 0.0;
                            k = 0;
                        }
                    }
                }
                open = 1;
                n = 0;
                sI = sQ = 0.0;
            }
        }
    }
    if (own) {
        s.sI[lane] = sI; s.sQ[lane] = sQ;
        s.aI[lane] = aI; s.aQ[lane] = aQ; s.aP[lane] = aP;
        s.cfI[lane] = cfI; s.cfQ[lane] = cfQ; s.cfP[lane] = cfP;
    }
    if (pair) {
        s.delta[lane] = delta;
        s.ratio[lane] = ratio;
    }
    if (lane == 0) {
        s.win_cnt = win_cnt;
        s.open = open; s.n = n; s.k = k; s.bits = bits; s.nbad = nbad; s.alarm = alarm; s.alarms = alarms;
        s.windows = windows; s.worst_pair = worst; s.pad = 0;
    }
}

int cfm_check_prm(const char *who, const gnsscorr_cfmprm_t &p, int rate, int corrn, int ch)
{
    if (rate < 2 || rate > 20) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: rate %d (2..20)", who, ch, rate);
    if (p.kbits < 1 || p.kbits > 4096) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: kbits %d (1..4096)", who, ch, p.kbits);
    if (p.skip_bits < 0) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: skip_bits %d (at least 0)", who, ch, p.skip_bits);
    if (p.nbad < 1) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: nbad %d (at least 1)", who, ch, p.nbad);
    if (p.npair < 1 || p.npair > corrn) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: npair %d (1..corrn %d)", who, ch, p.npair, corrn);
    if (!(p.dtol > 0.0)) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: dtol %g (above 0)", who, ch, p.dtol);
    if (!(p.rtol > 0.0)) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: rtol %g (above 0)", who, ch, p.rtol);
    for (int j = 0; j < GC_CFM_MAXPAIR; j++) {
        if (!std::isfinite(p.dref[j])) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: dref[%d] %g (finite)", who, ch, j, p.dref[j]);
        if (!std::isfinite(p.rref[j])) return gc_fail(GNSSCORR_EINVAL, "%s: channel %d: rref[%d] %g (finite)", who, ch, j, p.rref[j]);
    }
    return GNSSCORR_OK;
}

void cfm_launch(gnsscorr_ctx *ctx, const GcRowsView &rows, const gnsscorr_cfmprm_t *prm, gnsscorr_cfm_t *st, int ntap)
{
    GcTimed t(ctx, "rx_cfm");
    hipLaunchKernelGGL(rx_cfm_kernel, dim3((rows.nlist + GC_CFM_WAVES - 1) / GC_CFM_WAVES), dim3(GC_CFM_WAVES * 64), 0, ctx->stream,
                       rows, prm, st, ntap);
}

}  // namespace

extern "C" int gnsscorr_cfm_run(gnsscorr_ctx *ctx, const gnsscorr_cfmprm_t *prm, const int *rate, int corrn, gnsscorr_cfm_t *st,
                                const double *II, const double *QQ, const gnsscorr_trklog_t *log, const int *ndone,
                                const uint64_t *cnt0, int nch, int nper)
{
    if (!ctx || !prm || !rate || !st || !II || !QQ || !log || !ndone || !cnt0) return gc_fail(GNSSCORR_EINVAL, "cfm_run: null argument");
    if (nch < 0 || nper < 1) return gc_fail(GNSSCORR_EINVAL, "cfm_run: nch %d, nper %d", nch, nper);
    if (corrn < 1 || 1 + 2 * corrn > GNSSCORR_MAXTAPS) return gc_fail(GNSSCORR_EINVAL, "cfm_run: corrn %d (1..16)", corrn);
    for (int i = 0; i < nch; i++) {
        if (prm[i].kbits != 0) {
            int rc = cfm_check_prm("cfm_run", prm[i], rate[i], corrn, i);
            if (rc) return rc;
        }
        if (ndone[i] < 0 || ndone[i] > nper) return gc_fail(GNSSCORR_EINVAL, "cfm_run: channel %d: ndone %d of %d rows", i, ndone[i], nper);
    }
    if (nch == 0) return GNSSCORR_OK;
    const int ntap = 1 + 2 * corrn;
    return gc_stage_run(ctx, prm, rate, st, II, QQ, log, ndone, cnt0, nch, nper, ntap,
                        [&](const GcRowsView &rows, const gnsscorr_cfmprm_t *dprm, gnsscorr_cfm_t *dst) { cfm_launch(ctx, rows, dprm, dst, ntap); });
}

extern "C" int gnsscorr_rx_cfm_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_cfmprm_t *prm)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_cfm_set: no gnsscorr_rx_start yet");
    gnsscorr_cfmprm_t p;
    memset(&p, 0, sizeof(p));
    if (prm && prm->kbits != 0) p = *prm;
    const int corrn = (ctx->ntap - 1) / 2;
    return ctx->rx.cfm.set(ctx, "rx_cfm_set", ch0, nch, p, [corrn](const char *who, const gnsscorr_cfmprm_t &q, int rate, int ch) {
        return cfm_check_prm(who, q, rate, corrn, ch);
    });
}

extern "C" int gnsscorr_rx_cfm_status(gnsscorr_ctx *ctx, gnsscorr_cfm_t *st)
{
    if (!ctx || !ctx->rx.on) return gc_fail(GNSSCORR_ESTATE, "rx_cfm_status: no gnsscorr_rx_start yet");
    if (!st) return gc_fail(GNSSCORR_EINVAL, "rx_cfm_status: null argument");
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(ctx->rx.cfm.status(ctx, st));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

int gc_rx_cfm_launch(gnsscorr_ctx *ctx, int nperiod)
{
    GcRx &rx = ctx->rx;
    const int n = rx.cfm.fill(rx.st);
    if (!n) return GNSSCORR_OK;
    cfm_launch(ctx, gc_rows_of_run(ctx, rx.cfm.list.dev, n, nperiod), rx.cfm.dprm, rx.cfm.dst, ctx->ntap);
    GC_HIP(hipGetLastError());
    return GNSSCORR_OK;
}
