// gnsscorr_loop.hip -- closed-loop tracking on the device, in steps.  gfx950 (MI355X).
//
// What sdrthread() does around sdrtracking() (ref src/sdrmain.c:264-312): correlate one code period, let
// sdrnavigation() look at the prompt sum (bit synchronisation and bit decision, ref src/sdrnav.c:15-36,198-282),
// accumulate (cumsumcorr, ref src/sdrtrk.c:64-76), run pll()/dll() (ref src/sdrtrk.c:95-150) -- every period until
// the nav bit is synchronised, afterwards whenever checkbit() raises swloop (every loopms periods counted from the
// bit edge) -- and clear the sums after a filter update.
//
// The frequencies only change at a filter update, so the periods between two updates of a channel (its "filter
// interval": 1 period before bit sync, up to loopms after) are open-loop work: they are planned in one go and
// correlated side by side.  A run is a chain of launch pairs on one stream, no host round trip:
//
//   trk_step_tail  one workgroup of eight wavefronts per channel: closes the interval the previous correlator launch
//                  produced (partial sums -> II/QQ, sdrnavigation's bit sync / bit decision, cumsumcorr, pll/dll where
//                  due, log rows) and plans the next one: the exact NCO chains of gnsscorr_nco.h on two wavefronts, then
//                  every (period, NCO) piece table as a task from a queue all wavefronts serve, then unit constants
//                  and rounds, written for the correlator.
//   trk_step_corr  (channel, period of the interval, quarter) -> one 256-lane workgroup running ps_unit
//                  (gnsscorr_ps.h) on four rounds of 1024 IQ samples, one per wavefront; int32 partial sums per workgroup.
//
// Round 2 ran all of this in ONE workgroup per channel, period by period (32 of 256 CUs busy, 35 us per period).
#include <cstdlib>
#include <type_traits>

// the shaped code step inline: its emitter then lives in registers (handed by reference to an out-of-line function it
// sits in scratch memory, and every piece costs a few scratch round trips: 20 000 clocks per period instead of 8 000)
#define GC_CODE_PERIOD_INLINE
#include "gnsscorr_internal.h"
#include "gnsscorr_ps.h"
#include "gnsscorr_ctx.h"       // the host driver below the kernels

#ifdef GC_TAIL_PROF     // (tools/debug: shader-clock stamps of channel 0's tail wavefront, summed over the launches)
__device__ unsigned long long gc_tail_prof[16];
__shared__ unsigned long long tprev_;       // (thread 0's last stamp: the phases are functions of their own)
#define GC_TSTART() do { if (threadIdx.x == 0) tprev_ = __builtin_readcyclecounter(); } while (0)
#define GC_TSTAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long t_ = __builtin_readcyclecounter(); \
        gc_tail_prof[i] += t_ - tprev_; tprev_ = t_; } } while (0)
extern "C" int gnsscorr_debug_tail_prof(unsigned long long *dst, int reset)
{
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(gc_tail_prof), sizeof(unsigned long long) * 16) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(gc_tail_prof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#else
#define GC_TSTART() do { } while (0)
#define GC_TSTAMP(i) do { } while (0)
#endif

namespace {

// ref src/sdrtrk.c:95-126 (IP = sumI[0], QP = sumQ[0] after the II/QQ swap of :42)
__device__ __forceinline__ void loop_pll(gnsscorr_loop_t *L, GcTrkState &st, int prm, double dt)
{
    GC_FP_STRICT
    const double PI = 3.1415926535897932;
    const double IP = L->sumI[0], QP = L->sumQ[0], oldIP = L->oldsumI[0], oldQP = L->oldsumQ[0];
    double carrErr;
    if (IP > 0) carrErr = atan2(QP, IP) / PI;
    else carrErr = atan2(-QP, -IP) / PI;
    const double f1 = (IP == 0) ? PI / 2 : atan(QP / IP);
    const double f2 = (oldIP == 0) ? PI / 2 : atan(oldQP / oldIP);
    double freqErr = f1 - f2;
    if (freqErr > PI / 2) freqErr = PI - freqErr;
    if (freqErr < -PI / 2) freqErr = -PI - freqErr;
    L->carrNco += L->pllaw[prm] * (carrErr - L->carrErr) + L->pllw2[prm] * dt * carrErr + L->fllw[prm] * dt * freqErr;
    st.carrfreq = L->acqfreq + L->carrNco;
    L->carrErr = carrErr;
    L->freqErr = freqErr;
}

// ref src/sdrtrk.c:135-150
__device__ __forceinline__ void loop_dll(gnsscorr_loop_t *L, GcTrkState &st, int prm, double dt)
{
    GC_FP_STRICT
    const double IE = L->sumI[L->ne], IL = L->sumI[L->nl], QE = L->sumQ[L->ne], QL = L->sumQ[L->nl];
    const double codeErr = (sqrt(IE * IE + QE * QE) - sqrt(IL * IL + QL * QL)) /
                           (sqrt(IE * IE + QE * QE) + sqrt(IL * IL + QL * QL));
    L->codeNco += L->dllaw[prm] * (codeErr - L->codeErr) + L->dllw2[prm] * dt * codeErr;
    st.codefreq = L->crate - L->codeNco + (st.carrfreq - L->f_if - L->foffset) / (L->f_cf / L->crate);
    L->codeErr = codeErr;
}

#define GC_NAVSYNCTH 50         // ref src/sdr.h:157

// checksync(), ref src/sdrnav.c:198-233.  nav->sdreph.prn is the channel's PRN (ref src/sdrinit.c:506), so every
// PRN above 5 takes the first branch (written for BeiDou's NH20 overlay): a shift register of the last `rate` prompt
// signs, correlated with the overlay code -- all ones for L1CA / SBAS / G1 (ref src/sdrinit.c:520-521,542-543,557-558)
// -- i.e. synchronised once `rate` consecutive prompts have one sign.  PRN 1-5: votes for the position of sign
// changes, synchronised once a position has more than NAVSYNCTH votes.
__device__ __forceinline__ int nav_checksync(gnsscorr_loop_t *L, double IP, double IPold)
{
    GC_FP_STRICT
    const int rate = L->rate;
    if (L->prn > 5) {
        for (int i = 0; i + 1 < rate; i++) L->bitsync[i] = L->bitsync[i + 1];      // shiftdata(&bitsync[0], &bitsync[1], ., rate-1)
        L->bitsync[rate - 1] = IP < 0 ? -1 : 1;
        int corr = 0;
        for (int i = 0; i < rate; i++) corr += L->bitsync[i];                      // ocode[i] = 1
        if ((corr < 0 ? -corr : corr) == rate) {
            L->synci = L->biti;
            return 1;
        }
    } else {
        if (IPold * IP < 0) {
            L->bitsync[L->biti] += 1;
            int maxi = L->bitsync[0], ind = 0;                                      // maxvi(bitsync, rate, -1, -1, &synci)
            for (int i = 1; i < rate; i++)
                if (maxi < L->bitsync[i]) { maxi = L->bitsync[i]; ind = i; }
            L->synci = ind;
            if (maxi > GC_NAVSYNCTH) {
                L->synci--;
                if (L->synci < 0) L->synci = rate - 1;
                return 1;
            }
        }
    }
    return 0;
}

// checkbit(), ref src/sdrnav.c:241-282 (the frame bit buffer fbits[] is the nav decoder's: the decided bits leave
// through the log rows instead).  Returns the reference's syncflag.
__device__ __forceinline__ int nav_checkbit(gnsscorr_loop_t *L, double IP)
{
    GC_FP_STRICT
    const int diffi = L->biti - L->synci;
    int syncflag = 1;
    L->swreset = 0;
    L->swsync = 0;
    if (diffi == 1 || diffi == -L->rate + 1) {
        L->bitIP = IP;
        L->swreset = 1;
        L->navcnt = 1;
    } else {
        L->bitIP += IP;
        if (L->bitIP * IP < 0) syncflag = 0;
    }
    L->swloop = (L->navcnt % L->loopms == 0) ? 1 : 0;
    if (diffi == 0) {
        const int polarity = L->flagpol ? -1 : 1;
        L->bit = (L->bitIP < 0) ? -polarity : polarity;
        L->swsync = 1;
    }
    L->navcnt++;
    return syncflag;
}

// the part of sdrnavigation() in front of the frame decoder, ref src/sdrnav.c:18-36
// cnt % rate (ref src/sdrnav.c:18) without the 64-bit division while cnt fits 32 bits
__device__ __forceinline__ int nav_biti(uint64_t cnt, int rate)
{
    if ((cnt >> 32) == 0) return (int)((unsigned)cnt % (unsigned)rate);
    return (int)(cnt % (uint64_t)rate);
}

// late_after = 2000 / (ctime * 1000), the threshold of ref src/sdrnav.c:26,30 (the same for every period of a launch);
// II0 / oldI0: sdr->trk.II[0] and sdr->trk.oldI[0] as sdrtracking() has left them when it calls sdrnavigation()
__device__ __forceinline__ void nav_step_io(gnsscorr_loop_t *L, double late_after, double II0, double oldI0)
{
    GC_FP_STRICT
    const uint64_t cnt = L->cnt;
    L->biti = nav_biti(cnt, L->rate);
    const bool late = (double)cnt > late_after;
    if (L->rate == 1 && late) {
        L->synci = 0;
        L->flagsync = 1;
    }
    if (!L->flagsync && late) L->flagsync = nav_checksync(L, II0, oldI0);
    if (L->flagsync) nav_checkbit(L, II0);
}

// emitters that fill LDS tables (lane-uniform calls from one wavefront).  The table pointers are LDS-typed (address
// space 3), so every access is a DS instruction, which one wavefront executes in order.  Through generic pointers the
// stores become FLAT instructions; those reach the LDS by way of the texture path and can be overtaken by a DS read
// issued after them -- the round-2 closed-loop kernel stalled on exactly that.
// Both emitters keep what they need of the previous piece in registers (no LDS read on the chain's path) and leave
// what can be done for all pieces at once -- the fixed-point form of the carrier pieces, the reciprocal steps of the
// code pieces -- to a lane-parallel pass afterwards (lds_car_finish / lds_code_finish).
typedef __attribute__((address_space(3))) int *gc_lds_int;
typedef __attribute__((address_space(3))) GcCarSeg *gc_lds_car;
typedef __attribute__((address_space(3))) GcCodeSeg *gc_lds_code;
typedef __attribute__((address_space(3))) double *gc_lds_f64;
struct LdsCarTable {        // GcCarTable (gnsscorr_nco.h): pieces as (x, d) doubles in the slots, converted by lds_car_finish
    gc_lds_int k0;
    gc_lds_car seg;
    int n, overflow;
    bool lastzero;
    __device__ void reset() { n = 0; overflow = 0; lastzero = false; }
    __device__ void operator()(int k, double x, double d, int)
    {
        const int e = gc_expo(x) - 1023;
        const bool zero = e < 0 || e >= 31;             // gc_carseg_make gives the all-zero piece exactly then
        if (n > 0 && zero && lastzero) return;
        if (n >= GC_NCAR) { overflow = 1; return; }
        k0[n] = k;
        gc_lds_f64 raw = (gc_lds_f64)(seg + n);
        raw[0] = x;
        raw[1] = d;
        lastzero = zero;
        n++;
    }
};
__device__ __forceinline__ void lds_car_finish(gc_lds_car seg, int n, int lane)
{
    if (lane < n) {
        gc_lds_f64 raw = (gc_lds_f64)(seg + lane);
        const GcCarSeg s = gc_carseg_make(raw[0], raw[1]);
        seg[lane].fx = s.fx;
        seg[lane].dfx = s.dfx;
    }
}
struct LdsCodeTable {       // GcCodeTable (gnsscorr_nco.h); inv is filled in by lds_code_finish
    gc_lds_code seg;
    int cap, n, overflow;
    int lw, lcnt;           // the last piece: wrap count, positions
    double ly0, lyl;        //                 first and last value
    __device__ void reset() { n = 0; overflow = 0; }
    __device__ void operator()(int j, double y, double d, int count, int w)
    {
        GC_FP_STRICT
        const double yl = fma((double)(count - 1), d, y);
        if (n > 0 && lw == w && ly0 > -1.0 && lyl < 1.0 && y > -1.0 && yl < 1.0) {
            lcnt += count;
            lyl = yl;
            seg[n - 1].cnt = lcnt;
            seg[n - 1].ylast = yl;
            seg[n - 1].d = 0.0;                  // d = 0 with y0 in (-1, 1): every position is chip 0
            return;
        }
        if (n >= cap) { overflow = 1; return; }
        seg[n].y0 = y;
        seg[n].d = count > 1 ? d : 0.0;
        seg[n].inv = 0.0;
        seg[n].ylast = yl;
        seg[n].j0 = j;
        seg[n].cnt = count;
        seg[n].w = w;
        seg[n].pad = 0;
        lw = w; lcnt = count; ly0 = y; lyl = yl;
        n++;
    }
};
__device__ __forceinline__ void lds_code_finish(gc_lds_code seg, int n, int lane)
{
    if (lane < n) {
        const double d = seg[lane].d;
        seg[lane].inv = (seg[lane].cnt > 1 && d != 0.0) ? __ddiv_rn(1.0, d) : 0.0;
    }
}

// chip under replica position j from an LDS-typed code table (gc_code_chip_at of gnsscorr_nco.h)
__device__ __forceinline__ int lds_code_chip_at(gc_lds_code seg, int nseg, int j, int *w, int *piece)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].j0 <= j) lo = mid; else hi = mid - 1;
    }
    if (w) *w = seg[lo].w;
    if (piece) *piece = lo;
    int i = j - seg[lo].j0;
    if (i < 0) i = 0;
    if (i >= seg[lo].cnt) i = seg[lo].cnt - 1;
    const double d = seg[lo].d, y0 = seg[lo].y0;
    if (d == 0.0) return (int)y0;
    return (int)__fma_rn((double)i, d, y0);
}

// periods up to and including the next one after which the filters run, for a synchronised channel: checkbit()'s
// counter (ref src/sdrnav.c:249-262) run ahead.  At most kmax.
__device__ __forceinline__ int nav_interval(const gnsscorr_loop_t *L, int kmax)
{
    if (!L->flagsync) return 1;                     // prm1 after every period (ref src/sdrmain.c:272-276)
    int navcnt = L->navcnt;
    for (int j = 1; j <= kmax; j++) {
        const int biti = nav_biti(L->cnt + (uint64_t)(j - 1), L->rate);
        const int diffi = biti - L->synci;
        if (diffi == 1 || diffi == -L->rate + 1) navcnt = 1;
        if (navcnt % L->loopms == 0) return j;
        navcnt++;
    }
    return kmax;
}

// gc_fast_init (gnsscorr_nco.h) with one lane per binade: the table entries of an addend, written straight into
// an LDS-resident table (DS stores, by name).  Every lane of the calling wavefront takes part.
__device__ __forceinline__ void fast_init_lanes(GcNcoFast &f, double s, bool with_inv, int lane)
{
    GC_FP_STRICT
    const uint64_t us = gc_d2u(s);
    const int es = gc_expo(s);
    const bool ok = gc_fast_has_table(s);
    double d = 0.0, inv = 0.0;
    bool tie = false;
    if (ok && lane < GC_NB) {
        const int ex = es + 2 + lane;
        const int et = es + 1075 - ex;
        double b = 0.0;
        if (et >= 1023 - 1) {
            const double t = gc_u2d((us & 0x800FFFFFFFFFFFFFull) | ((uint64_t)et << 52));
            b = rint(t);
            tie = fabs(t - b) == 0.5;
        }
        d = ldexp(b, ex - 1075);
        if (b != 0.0 && with_inv) inv = __ddiv_rn(1.0, fabs(d));
    }
    const unsigned long long tm = __ballot(tie);
    if (lane < GC_NB) {
        f.d[lane] = d;
        f.inv[lane] = inv;
    }
    if (lane == 0) {
        f.s = s;
        f.inv_s = __ddiv_rn(1.0, fabs(s));
        f.tie = (unsigned)tm & ((1u << GC_NB) - 1u);
        f.ex0 = ok ? es + 2 : GC_NO_TABLE;
    }
}
// what one lane of a wavefront wrote to LDS, every lane of it reads afterwards
__device__ __forceinline__ void tail_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// gc_code_plan_init(P, ci, len, smax) around fast_init_lanes
__device__ __forceinline__ void code_plan_init_lanes(GcCodePlan &P, double ci, int len, int smax, int lane)
{
    GC_FP_STRICT
    fast_init_lanes(P.f, ci, true, lane);
    tail_wave_sync();
    if (lane == 0) gc_code_plan_shape(P, ci, len, smax);
}
// Progress words (LDS): lane 0 publishes how many periods its wavefront has finished, with all it stored for them, and
// TAIL_DONE once it stops.  prog_wait_past: until period e is finished; TAIL_DONE seen with e >= S.k: e never comes.
constexpr int TAIL_DONE = 0x7fffffff;
__device__ __forceinline__ void prog_publish(int *word, int count) { __hip_atomic_store(word, count, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void prog_publish_done(int *word) { prog_publish(word, TAIL_DONE); }
__device__ __forceinline__ int prog_wait_past(const int *word, int e)
{
    int pg;
    while ((pg = __hip_atomic_load(word, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) <= e) __builtin_amdgcn_s_sleep(1);
    return pg;
}
// bracket discovery, lanes e and 32 + e: the value at the bracket's other end, and whether the two ends agree on one
template <class T> __device__ __forceinline__ T pair_other(T v, int lane) { return __shfl(v, lane ^ 32, 64); }
__device__ __forceinline__ bool pair_same(int v, int lane) { return v == pair_other(v, lane); }
// the general walkers for a period the shaped steps decline (a tie in the top binade, a phase next to zero, ...):
// out of line, with tables of their own (the workgroup's shared tables stay read-only)
template <class Emit>
__device__ __attribute__((noinline)) double tail_carrier_slow(double ps, double remcarr, int n, Emit &emit)
{
    GcNcoFast f, fp;
    gc_fast_init(f, ps);
    gc_fast_init(fp, -GC_NCO_DPI);
    const double xn = gc_fast_carrier_walk(f, gc_carrier_phis(remcarr), n, emit);
    return gc_fast_prem(fp, xn);
}
template <class Emit>
__device__ __attribute__((noinline)) double tail_code_slow(double ci, double remcode, int clen, int smax, int nt, Emit &emit)
{
    GcNcoFast f;
    gc_fast_init(f, ci);
    const double cend = gc_fast_code_walk(f, gc_code_start(remcode, smax, ci, clen), clen, nt, emit);
    return gc_code_rem(cend, smax, ci);
}
// whether an attempt ran out of table room (the chains' GcNoEmit holds no table)
__device__ __forceinline__ bool tail_emit_over(const GcNoEmit &) { return false; }
template <class Emit> __device__ __forceinline__ bool tail_emit_over(const Emit &emit) { return emit.overflow != 0; }
// The ladder's lower rungs, for the chains (GcNoEmit) and the table tasks (Lds*Table): the certified period step, else
// the emitter forgets the attempt and the walkers above take the period.  A step whose pieces did not fit the table is
// such an attempt too: the code step spells out every replica position behind the second wrap as a piece of its own
// (gc_code_period_body's tail, about 13 + smax - samples per chip pieces), the walker merges them by binade and stays at
// at most 20 pieces for every span set_channels accepts.  The carrier step has no such rule: its pieces are the walker's,
// one per binade visited (counted on the host, tests/test_tap_spans_host.py), so a table it overflows the walker
// overflows too.  (gc_*_period_any of gnsscorr_nco.h walk inline on the plan's
// tables: the kernel sits at its register cap, and S.PK.f has no reciprocals for the carrier walker.)
template <class Emit>
__device__ __forceinline__ double tail_code_period(const GcCodePlan &PC, const GcChan &c, double ci, double remcode, int nt, int lane, Emit &emit)
{
    GcFillLanes fill{lane};
    double r;
    if (gc_code_period(PC, remcode, nt, fill, &r, emit) && !tail_emit_over(emit)) return r;
    emit.reset();
    return tail_code_slow(ci, remcode, c.clen, c.smax, nt, emit);
}
template <class Emit>
__device__ __forceinline__ double tail_carrier_period(const GcCarPlan &PK, double ps, double remcarr, int n, int lane, Emit &emit)
{
    GcFillLanes fill{lane};
    double r;
    if (gc_carrier_period(PK, remcarr, n, fill, &r, emit)) return r;
    emit.reset();
    return tail_carrier_slow(ps, remcarr, n, emit);
}
// gc_code_claims_step of the channel's tail class tcls (gc_tail_class: how many positions the tail's instance holds)
template <int IT, bool PERLANE>
__device__ __forceinline__ bool tail_code_claims_step(int tcls, const GcCodePlan &PC, const GcCodeStepC<IT> &SC, double remcode, int nt,
                                                      GcCodeClaims &cl, double *out)
{
    if (tcls == 0) return gc_code_claims_step<IT, gc_tail_max(0), false, PERLANE>(PC, SC, remcode, nt, cl, out);
    if (tcls == 1) return gc_code_claims_step<IT, gc_tail_max(1), false, PERLANE>(PC, SC, remcode, nt, cl, out);
    return gc_code_claims_step<IT, gc_tail_max(2), false, PERLANE>(PC, SC, remcode, nt, cl, out);
}
// the step WITH its checks, for a period whose start lies outside the bracket its claims were proved for (rare): out
// of line, so that the chains' loops carry the value form only.  PC / PK / cl: the workgroup's tables and rows (LDS).
template <int IT>
__device__ __attribute__((noinline)) bool tail_code_checked(const GcCodePlan *PC, double remcode, int nt, int tcls, const GcCodeClaims *cl, double *out)
{
    GcCodeStepC<IT> SC;
    gc_code_stepc_init(SC, *PC);
    GcCodeClaims c2 = *cl;
    double r;
    const bool ok = tail_code_claims_step<IT, true>(tcls, *PC, SC, remcode, nt, c2, &r);
    if (ok) *out = r;
    return ok;
}
__device__ __attribute__((noinline)) bool tail_carrier_checked(const GcCarPlan *PK, int nsamp, double remcarr, int n, const GcCarClaims *cl, double *out)
{
    GcCarStepC CK;
    gc_car_stepc_init(CK, *PK, nsamp + 16);
    GcCarClaims c2 = *cl;
    double r;
    const bool ok = gc_carrier_claims_step<false, true>(*PK, CK, remcarr, n, c2, &r);
    if (ok) *out = r;
    return ok;
}
#define GC_TAIL_NW 8            // wavefronts of the tail workgroup
struct TailShared {
    gnsscorr_loop_t lp;
    GcTrkState st;                                  // the channel's state while the kernel runs (frequencies: wavefront 0)
    GcCodePlan PC;
    GcCarPlan PK;
    // the interval's periods: start values of the chain (entry k = the state the interval leaves behind), ...
    double remcode[GC_STEP_KMAX + 1], remcarr[GC_STEP_KMAX + 1];
    uint64_t buffloc[GC_STEP_KMAX + 1];
    int n[GC_STEP_KMAX], valid[GC_STEP_KMAX], ncar[GC_STEP_KMAX], ncode[GC_STEP_KMAX], bad[GC_STEP_KMAX];
    int want, k, prog, progc, nexttask, starved, navdone;
    int nflagsync[GC_STEP_KMAX], nswloop[GC_STEP_KMAX], nbit[GC_STEP_KMAX];     // sdrnavigation()'s verdict per closing period
    int psum[GC_STEP_KMAX][2 * GNSSCORR_MAXTAPS];   // the closing interval's correlator sums: [period][tap | ntap + tap]
    GcCodeClaims ccl[GC_STEP_KMAX];                 // the periods' claims (gnsscorr_nco.h: period steps on claims), discovered
    GcCarClaims kcl[GC_STEP_KMAX];                  // side by side, one lane per period, then evaluated and checked by the chain
    // ... and their NCO tables
    int k0[GC_STEP_KMAX][GC_NCAR + 4];
    GcCarSeg car[GC_STEP_KMAX][GC_NCAR];
    GcCodeSeg code[GC_STEP_KMAX][GC_NCODE];
};
// ---- the tail's phases, in the kernel's order.  A: the kernel's arguments and who this lane is; S: the LDS block ----
struct TailArgs {
    const GcChan *chan; GcTrkState *state; gnsscorr_loop_t *loop; GcStepMeta *meta; const uint64_t *wrpos; const int *partial;
    GcTrkUnit *unit; GcUnitSegs *segs; GcRound *rounds; double *corrI, *corrQ; int *nsamp_out; gnsscorr_trklog_t *log;
    int *ndone, *nco_overflow, *lapped; unsigned *hostflags;
    int nper, nseg, ntap_stride, max_n, kcap, plan;
    int ch, tid, lane, wave;        // who this lane is
};
struct TailSteps { double ci, ps, spc, dlen; bool shape_ok; };    // q, the next interval's NCO steps (shape_ok: the reference's one-subtraction code wrap is defined)
__device__ __forceinline__ void tail_copy_loop(gnsscorr_loop_t *to, const gnsscorr_loop_t *from, int tid)
{
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(from);
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(to);
    for (int i = tid; i < (int)(sizeof(gnsscorr_loop_t) / 8); i += 64 * GC_TAIL_NW) dst[i] = src[i];
}
// state in -- all wavefronts.  Writes S.lp, S.st, S.navdone; returns the channel's meta.  A barrier follows.
__device__ __forceinline__ GcStepMeta tail_state_in(const TailArgs &A, TailShared &S)
{
    tail_copy_loop(&S.lp, A.loop + A.ch, A.tid);
    const GcStepMeta m = A.meta[A.ch];
    if (A.tid == 0) { S.st = A.state[A.ch]; S.navdone = 0; }
    return m;
}
// sums -- all wavefronts.  The closing interval's (period, tap, rail) sums: partial -> S.psum; a barrier hands them on.
__device__ __forceinline__ void tail_sums(const TailArgs &A, TailShared &S, const GcStepMeta &m, int ntap)
{
    for (int x = A.tid; x < m.k * 2 * ntap; x += 64 * GC_TAIL_NW) {
        const int e = x / (2 * ntap), r = x - e * 2 * ntap;            // r: tap (I rail), ntap + tap (Q rail)
        const int col = r < ntap ? r : A.ntap_stride + (r - ntap);
        const int *pp = A.partial + ((size_t)A.ch * m.kcap + e) * A.nseg * 2 * A.ntap_stride + col;
        int sum = 0;
        for (int sg = 0; sg < A.nseg; sg++) sum += pp[(size_t)sg * 2 * A.ntap_stride];
        S.psum[e][r] = sum;
    }
}
// nav -- wavefront 1, lane 0, beside close.  sdrnavigation()'s bit sync / bit decision per closing period (ref
// src/sdrnav.c:18-36): it only looks at the prompt sums (S.psum; II0_before: trk.II[0] of the period before, which close
// overwrites) and its own fields of S.lp.  Writes S.nflagsync / nswloop / nbit; S.navdone tells close how far it is.
__device__ __forceinline__ void tail_nav(const TailArgs &A, TailShared &S, int k, int ntap, double II0_before)
{
    gnsscorr_loop_t *lp = &S.lp;
    if (A.lane == 0 && k > 0) {
        const double late_after = __ddiv_rn(2000.0, __dmul_rn(lp->ctime, 1000.0));
        double prevII0 = II0_before;                    // (what memcpy leaves in oldI[0]: ntap >= 3)
        for (int e = 0; e < k; e++) {
            const double II0 = (double)S.psum[e][ntap] * (1.0 / 32.0);      // trk.II[0] = the correlator's QQ[0] (ref src/sdrtrk.c:42)
            nav_step_io(lp, late_after, II0, prevII0);
            S.nflagsync[e] = lp->flagsync; S.nswloop[e] = lp->swloop;
            S.nbit[e] = (lp->flagsync && lp->swsync) ? lp->bit : 0;
            lp->cnt = lp->cnt + 1;
            prevII0 = II0;
            prog_publish(&S.navdone, e + 1);
        }
    }
}
// close -- wavefront 0.  Per closing period: II/QQ out, cumsumcorr (lane = tap), the filters where nav's flags (behind
// S.navdone) say so, the log row, m.early; then S.want, the chains' start values (entry 0), the frequencies in S.st and
// the progress words at zero.  Reads S.psum.  A barrier hands all of that to the planning phases.
__device__ __forceinline__ void tail_close(const TailArgs &A, TailShared &S, GcStepMeta &m, int ntap)
{
    gnsscorr_loop_t *lp = &S.lp;
    const int ch = A.ch, lane = A.lane;
    GcTrkState st = S.st;
    for (int e = 0; e < m.k; e++) {
        const int p = m.pbase + e;
        if (lane < ntap) {
            const int sI = S.psum[e][lane], sQ = S.psum[e][ntap + lane];
            const double cI = (double)sI * (1.0 / 32.0), cQ = (double)sQ * (1.0 / 32.0);     // correlator's II, QQ (ref src/sdrcmn.c:716-719)
            A.corrI[((size_t)ch * A.nper + p) * ntap + lane] = cI;
            A.corrQ[((size_t)ch * A.nper + p) * ntap + lane] = cQ;
            // memcpy(oldI, II, 1 + 2*corrn*sizeof(double)): the last tap only gets its lowest byte (ref src/sdrtrk.c:35-36)
            const double pII = lp->II[lane], pQQ = lp->QQ[lane];
            double oI = pII, oQ = pQQ;
            if (lane == ntap - 1) {
                oI = gc_u2d((gc_d2u(lp->oldI[lane]) & ~0xFFull) | (gc_d2u(pII) & 0xFFull));
                oQ = gc_u2d((gc_d2u(lp->oldQ[lane]) & ~0xFFull) | (gc_d2u(pQQ) & 0xFFull));
            }
            lp->oldI[lane] = oI; lp->oldQ[lane] = oQ;
            // correlator(..., trk.QQ, trk.II, ...): trk.II <- sum dataQ*code, trk.QQ <- sum dataI*code (ref src/sdrtrk.c:42)
            lp->II[lane] = cQ; lp->QQ[lane] = cI;
            // cumsumcorr, polarity +1: the overlay code is all ones (ref src/sdrtrk.c:64-76, src/sdrmain.c:269)
            lp->oldsumI[lane] = __dadd_rn(lp->oldsumI[lane], oI);
            lp->oldsumQ[lane] = __dadd_rn(lp->oldsumQ[lane], oQ);
            lp->sumI[lane] = __dadd_rn(lp->sumI[lane], cQ);
            lp->sumQ[lane] = __dadd_rn(lp->sumQ[lane], cI);
        }
        tail_wave_sync();
        (void)prog_wait_past(&S.navdone, e);            // (this period's nav flags: wavefront 1 is usually ahead)
        int flag = 0;
        if (lane == 0) {
            if (!S.nflagsync[e]) {
                loop_pll(lp, st, 0, lp->ctime);
                loop_dll(lp, st, 0, lp->ctime);
                flag = 1;
            } else if (S.nswloop[e]) {
                loop_pll(lp, st, 1, (double)lp->loopms / 1000);
                loop_dll(lp, st, 1, (double)lp->loopms / 1000);
                flag = 2;
            }
            gnsscorr_trklog_t *lg = A.log + (size_t)ch * A.nper + p;
            lg->carrfreq = st.carrfreq; lg->codefreq = st.codefreq;
            lg->carrErr = lp->carrErr; lg->codeErr = lp->codeErr; lg->freqErr = lp->freqErr;
            lg->carrNco = lp->carrNco; lg->codeNco = lp->codeNco;
            lg->flagloopfilter = flag; lg->flagsync = S.nflagsync[e]; lg->navbit = S.nbit[e];
            if (flag && e + 1 < m.k) m.early = 1;   // the plan held the frequencies beyond a filter update: must not happen
        }
        flag = __builtin_amdgcn_readfirstlane(flag);
        st.carrfreq = gc_u2d(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(gc_d2u(st.carrfreq) >> 32)) << 32) |
                             (unsigned)__builtin_amdgcn_readfirstlane((int)gc_d2u(st.carrfreq)));
        st.codefreq = gc_u2d(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(gc_d2u(st.codefreq) >> 32)) << 32) |
                             (unsigned)__builtin_amdgcn_readfirstlane((int)gc_d2u(st.codefreq)));
        m.early = __builtin_amdgcn_readfirstlane(m.early);
        if (flag && lane < ntap) {      // clearcumsumcorr (ref src/sdrtrk.c:77-86)
            lp->oldsumI[lane] = lp->oldsumQ[lane] = lp->sumI[lane] = lp->sumQ[lane] = 0.0;
        }
        tail_wave_sync();
        GC_TSTAMP(2);   // nav + filters + log
    }
    // the next interval: up to the next filter update, the end of the run, the step's capacity
    int want = 0;
    if (A.plan && m.done < A.nper) want = min(nav_interval(lp, A.kcap), A.nper - m.done);
    if (lane == 0) {
        S.st.carrfreq = st.carrfreq; S.st.codefreq = st.codefreq;
        S.want = want;
        S.k = S.prog = S.progc = S.nexttask = S.starved = 0;
        S.remcode[0] = st.remcode; S.remcarr[0] = st.remcarr; S.buffloc[0] = st.buffloc;
    }
}
// q from the frequencies close left in S.st (every lane, after the barrier)
__device__ __forceinline__ TailSteps tail_steps(const TailShared &S, const GcChan &c)
{
    const double codefreq = S.st.codefreq, dlen = (double)c.clen, ci = __dmul_rn(c.ti, codefreq);
    return TailSteps{ci, gc_carrier_ps(S.st.carrfreq, c.ti), __ddiv_rn(codefreq, c.f_sf), dlen, ci > 0.0 && ci < dlen};
}
// step tables -- wavefronts 0, 1, 2, one lane per binade: S.PK.f, S.PC (shaped), S.PK.fprem.  Read-only after the barrier.
__device__ __forceinline__ void tail_step_tables(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q)
{
    if (A.wave == 0) {
        fast_init_lanes(S.PK.f, q.ps, false, A.lane);
        if (A.lane == 0) S.PK.ydpi = __ddiv_rn(1.0, GC_NCO_DPI);
    } else if (A.wave == 1) {
        code_plan_init_lanes(S.PC, q.ci, c.clen, c.smax, A.lane);
    } else if (A.wave == 2) {
        fast_init_lanes(S.PK.fprem, -GC_NCO_DPI, true, A.lane);
    }
}
// discover (in the kernel's body, see there) -- code brackets on wavefront 2 (-> S.ccl), carrier brackets on wavefront 3
// (-> S.kcl); a barrier hands the rows to the chains.  Each period's structure from its closed-form start (gc_spec_start
// from entry 0), proved for a bracket around it as the batch planner's discovery does (gnsscorr_plan.hip): lane e discovers
// period e's claims from the lower end, lane 32 + e from the upper end; where both pass their checks with the same claims
// and sample count, every start in between does (every operation of the step is monotone in the start), and the chain
// evaluates the period unchecked.  +-2^-25 holds what the closed form's missing rounding adds up to over GC_STEP_KMAX periods.
constexpr double TAIL_BRACKET_W = 2.98023223876953125e-8;       // 2^-25
// One period of a chain, the ladder from the top: the exact start inside the bracket the claims were proved for -> the
// values alone (the verdict is unused, the compiler drops the checks); claims but no bracket around this start -> the step
// with its checks, out of line; else, or where that declines, the lower rungs.  inst: SC holds the channel's instance.
// (remcode by reference: returned by value, the code chain spills vector registers.)
template <int IT>
__device__ __forceinline__ void tail_code_step(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, const GcCodeStepC<IT> &SC,
                                                 bool inst, int tcls, int e, double &remcode, int n)
{
    double r = remcode;
    GcCodeClaims cl = S.ccl[e];
    const int nt = n + 2 * c.smax;
    const bool inside = __builtin_amdgcn_readfirstlane((inst && cl.tag == 1 && remcode >= cl.lo && remcode <= cl.hi && n == cl.n) ? 1 : 0) != 0;
    bool ok = inside;
    if (inside) {
        (void)tail_code_claims_step<IT, false>(tcls, S.PC, SC, remcode, nt, cl, &r);
    } else if (inst && cl.tag == 1) {
        double r2;
        ok = tail_code_checked<IT>(&S.PC, remcode, nt, tcls, &S.ccl[e], &r2);
        if (ok) r = r2;
    }
    GcNoEmit ne;
    if (ok) remcode = r;
    else remcode = tail_code_period(S.PC, c, q.ci, remcode, nt, A.lane, ne);
}
__device__ __forceinline__ double tail_carrier_step(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, const GcCarStepC &CK,
                                                    int e, double remcarr, int n)
{
    double r = remcarr;
    GcCarClaims cl = S.kcl[e];
    const int tagu = __builtin_amdgcn_readfirstlane(cl.tag);
    const bool inside = __builtin_amdgcn_readfirstlane((tagu == 1 && remcarr >= cl.lo && remcarr <= cl.hi && n == cl.nl) ? 1 : 0) != 0;
    bool ok = inside;
    if (inside) {
        (void)gc_carrier_claims_step<false, false, 1>(S.PK, CK, remcarr, n, cl, &r);      // the values alone: the bracket is the proof
    } else if (tagu == 2) {
        double r2 = remcarr;
        ok = gc_carrier_claims_step<false, false, 2>(S.PK, CK, remcarr, n, cl, &r2);       // (its own conditions, checked)
        if (ok) r = r2;
    } else if (tagu == 1) {
        double r2;
        ok = tail_carrier_checked(&S.PK, c.nsamp, remcarr, n, &S.kcl[e], &r2);
        if (ok) r = r2;
    }
    if (ok) return r;
    GcNoEmit ne;
    return tail_carrier_period(S.PK, q.ps, remcarr, n, A.lane, ne);
}
// code chain -- wavefront 1, every interval.  Per period: is it there yet (ref src/sdrtrk.c:26-30; else S.starved), its
// length (:31-32) and, in an interval of several periods, the code step.  Reads S.ccl, S.PC; writes S.n / valid / remcode /
// buffloc [e], publishes e on S.prog (the carrier chain and the table tasks wait there), steps to entry e + 1; at the end
// S.k and done.  One instance per shape of the step (ITOP: the table binade that holds the code length; 0: none, the
// certified step serves), so that its constants stay in registers over the interval.
template <int ITOP>
__device__ __forceinline__ void tail_code_chain(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, int want)
{
    constexpr int IT = ITOP ? ITOP : 7;
    const int lane = A.lane;
    const uint64_t wp = A.wrpos[A.ch];
    const bool have_data = wp >= (uint64_t)c.nsamp;
    const uint64_t bufflocnow = wp - (uint64_t)c.nsamp;
    GcCodeStepC<IT> SC;
    const bool inst = ITOP != 0 && S.PC.ok;
    if (inst) gc_code_stepc_init(SC, S.PC);
    const int tcls = gc_tail_class(c.smax);
    double remcode = S.remcode[0];
    uint64_t buffloc = S.buffloc[0];
    int k = 0;
    const double yspc = __ddiv_rn(1.0, q.spc);
    const bool fastdiv = q.spc > 1e-300 && q.spc < 1e300 && yspc < 1e300;
    for (int e = 0; e < want; e++) {
        if (!(have_data && bufflocnow > buffloc)) { if (lane == 0) S.starved = 1; break; }
        // first samples overwritten since (more than a ring behind the writer): run as sdrtracking() runs it, and counted
        if (lane == 0 && wp > c.ringlen && buffloc < wp - c.ringlen) atomicAdd(A.lapped, 1);
        // (dlen - remcode) / (codefreq / f_sf), ref src/sdrtrk.c:31-32: through the reciprocal (gc_div_y) where that is safe
        const double num = __dsub_rn(q.dlen, remcode);
        const double qq = fastdiv ? gc_div_y(num, q.spc, yspc) : __ddiv_rn(num, q.spc);
        const int n = (qq > -2147483648.0 && qq < 2147483648.0) ? (int)qq : 0;
        const bool valid = n > 0 && n <= A.max_n && q.shape_ok;
        if (lane == 0) { S.n[e] = n; S.valid[e] = valid ? 1 : 0; S.remcode[e] = remcode; S.buffloc[e] = buffloc; }
        k = e + 1;
        if (want > 1) {
            tail_wave_sync();
            if (lane == 0) prog_publish(&S.prog, k);
            if (valid) tail_code_step<IT>(A, S, c, q, SC, inst, tcls, e, remcode, n);
        }
        buffloc += (uint64_t)(int64_t)n;
        if (lane == 0) { S.remcode[e + 1] = remcode; S.buffloc[e + 1] = buffloc; }
    }
    tail_wave_sync();
    if (lane == 0) { S.k = k; prog_publish_done(&S.prog); }
}
__device__ __forceinline__ void tail_code_chain_any(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, int want)
{
    switch ((want > 1 && S.PC.ok) ? S.PC.itop : 0) {
    case 7:  tail_code_chain<7>(A, S, c, q, want); break;
    case 8:  tail_code_chain<8>(A, S, c, q, want); break;
    case 9:  tail_code_chain<9>(A, S, c, q, want); break;
    case 10: tail_code_chain<10>(A, S, c, q, want); break;
    case 11: tail_code_chain<11>(A, S, c, q, want); break;
    case 12: tail_code_chain<12>(A, S, c, q, want); break;
    default: tail_code_chain<0>(A, S, c, q, want); break;
    }
}
// carrier chain -- wavefront 0, intervals of several periods, one step behind the code chain: waits on S.prog for period
// e's length, steps (S.kcl, S.PK), stores S.remcarr[e + 1], publishes on S.progc for the carrier table tasks; done at the end.
__device__ __forceinline__ void tail_carrier_chain(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, int want)
{
    double remcarr = S.remcarr[0];
    GcCarStepC CK;
    gc_car_stepc_init(CK, S.PK, c.nsamp + 16);
    for (int e = 0; e < want; e++) {
        if (prog_wait_past(&S.prog, e) == TAIL_DONE && e >= S.k) break;
        if (S.valid[e]) remcarr = tail_carrier_step(A, S, c, q, CK, e, remcarr, S.n[e]);
        if (A.lane == 0) S.remcarr[e + 1] = remcarr;
        tail_wave_sync();
        if (A.lane == 0) prog_publish(&S.progc, e + 1);
    }
    if (A.lane == 0) prog_publish_done(&S.progc);
}
// table tasks -- all wavefronts.  Task x = (period x/2, carrier | code), from a queue (S.nexttask) in order: the period
// step again from its known start, its piece table emitted into LDS (S.k0 / S.car / S.code [e]) and finished by the lanes;
// S.ncar / S.ncode [e].  A wavefront without a chain starts as soon as the period is published (S.prog; carrier tasks also
// S.progc), the chains' wavefronts join when done.  A one-period interval has no chain: these steps are it and store
// entry 1.  A barrier hands the tables to out.
__device__ __forceinline__ void tail_table_tasks(const TailArgs &A, TailShared &S, const GcChan &c, const TailSteps &q, int want)
{
    const int lane = A.lane;
    for (;;) {
        int x = 0;
        if (lane == 0) x = __hip_atomic_fetch_add(&S.nexttask, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        x = __builtin_amdgcn_readfirstlane(x);
        if (x >= 2 * want) break;
        const int e = x >> 1;
        if (prog_wait_past(&S.prog, e) == TAIL_DONE && e >= S.k) break;     // the ring holds fewer periods than wanted
        if (!(x & 1) && want > 1) (void)prog_wait_past(&S.progc, e - 1);
        if (!S.valid[e]) {
            if (lane == 0) { if (x & 1) S.ncode[e] = 0; else S.ncar[e] = 0; S.bad[e] = 0; }
            if (want == 1 && lane == 0) { if (x & 1) S.remcode[1] = S.remcode[0]; else S.remcarr[1] = S.remcarr[0]; }
            continue;
        }
        const int n = S.n[e];
        if (x & 1) {
            LdsCodeTable dt{(gc_lds_code)S.code[e], GC_NCODE, 0, 0, 0, 0, 0.0, 0.0};
            const double r = tail_code_period(S.PC, c, q.ci, S.remcode[e], n + 2 * c.smax, lane, dt);
            tail_wave_sync();
            lds_code_finish((gc_lds_code)S.code[e], dt.n, lane);
            if (lane == 0) { S.ncode[e] = dt.overflow ? -1 : dt.n; if (want == 1) S.remcode[1] = r; }
        } else {
            LdsCarTable ct{(gc_lds_int)S.k0[e], (gc_lds_car)S.car[e], 0, 0, false};
            const double r = tail_carrier_period(S.PK, q.ps, S.remcarr[e], n, lane, ct);
            tail_wave_sync();
            lds_car_finish((gc_lds_car)S.car[e], ct.n, lane);
            if (lane == 0) { S.ncar[e] = ct.overflow ? -1 : ct.n; if (want == 1) S.remcarr[1] = r; }
        }
    }
}
// out -- period e on wavefront e mod GC_TAIL_NW.  Reads the chains' entries and the tables; checks what the correlator's
// scans rely on (else nco_overflow, nothing correlated), copies the tables to segs, builds the rounds, writes unit and log.
__device__ __forceinline__ void tail_out(const TailArgs &A, TailShared &S, const GcChan &c, int done, int k)
{
    const int ch = A.ch, lane = A.lane, dtype = c.dtype, nseg = A.nseg;
    const int nit = trk_ps_nit(dtype, 2), rgrp = GC_PS_WLANES * nit, rsamp = rgrp * (16 / dtype);     // a round: one wavefront's share (gnsscorr_ps.h)
    for (int e = A.wave; e < k; e += GC_TAIL_NW) {
        const int n = S.n[e];
        const int p = done + e;
        const size_t ui = (size_t)ch * A.kcap + e;
        const uint64_t buffloc = S.buffloc[e];
        gc_lds_int sk0 = (gc_lds_int)S.k0[e];
        gc_lds_car scar = (gc_lds_car)S.car[e];
        gc_lds_code scode = (gc_lds_code)S.code[e];
        GcTrkUnit u;
        gc_unit_geometry(u, c, buffloc, n);
        u.n = S.valid[e] ? n : 0;
        u.ncar = S.ncar[e];
        u.ncode = S.ncode[e];
        u.eq0 = u.eq1 = -1;                             // no edge table: the correlator finds the edges' start samples itself
        if (u.n > 0) {
            // carrier pieces start at sample 0 and at increasing samples; code pieces are non-empty, contiguous, cover nt
            bool bad = u.ncar < 1 || u.ncode < 1;
            if (!bad) {
                if (lane == 0) bad = sk0[0] != 0;
                if (lane + 1 < u.ncar) bad = bad || !(sk0[lane] < sk0[lane + 1]);
                if (lane < u.ncode) {
                    const int je = scode[lane].j0 + scode[lane].cnt;
                    bad = bad || scode[lane].cnt <= 0 || je != (lane + 1 < u.ncode ? scode[lane + 1].j0 : u.nt);
                }
            }
            if (__any(bad)) {
                if (lane == 0) atomicAdd(A.nco_overflow, 1);
                u.n = u.ncar = u.ncode = 0;
            }
        } else {
            u.ncar = u.ncode = 0;
        }
        if (u.n > 0) {
            GcUnitSegs *gs = A.segs + ui;
            if (lane < u.ncar) {
                gs->carK0[lane] = sk0[lane];
                GcCarSeg cs;
                cs.fx = scar[lane].fx; cs.dfx = scar[lane].dfx;
                gs->car[lane] = cs;
            }
            if (lane < u.ncode) {
                GcCodeSeg sg;
                sg.y0 = scode[lane].y0; sg.d = scode[lane].d; sg.inv = scode[lane].inv; sg.ylast = scode[lane].ylast;
                sg.j0 = scode[lane].j0; sg.cnt = scode[lane].cnt; sg.w = scode[lane].w; sg.pad = 0;
                gs->code[lane] = sg;
            }
            // rounds: four per correlator workgroup, one per wavefront; a lane takes every 64th round (periods of more
            // than 64 rounds, 65536 samples, have more rounds than the wavefront has lanes)
            for (int r = lane; r < 4 * nseg && r * rgrp < u.G; r += 64) {
                const int g0 = r * rgrp;
                int jfirst, jlast, wa = 0, wb = 0, hint = 0;
                gc_round_span((g0 * 16 - u.head) / dtype, rsamp, n, c.smax, &jfirst, &jlast);
                const int ma = lds_code_chip_at(scode, u.ncode, jfirst, &wa, &hint);
                const int mb = lds_code_chip_at(scode, u.ncode, jlast, &wb, nullptr);
                A.rounds[ui * nseg * 4 + r] = gc_round_make(c.code, c.nedge, ma, wa, mb, wb, hint);
            }
        }
        if (lane == 0) {
            A.unit[ui] = u;
            gnsscorr_trklog_t *lg = A.log + (size_t)ch * A.nper + p;
            lg->buffloc = buffloc; lg->currnsamp = n;
            lg->remcode = S.remcode[e + 1]; lg->remcarr = S.remcarr[e + 1];
            A.nsamp_out[(size_t)ch * A.nper + p] = n;
        }
    }
}
// state out -- thread 0: the state behind the k planned periods, meta, ndone, the host's flags; all wavefronts: S.lp back.
__device__ __forceinline__ void tail_state_out(const TailArgs &A, TailShared &S, const GcStepMeta &m, int k, bool was_finished)
{
    const int ch = A.ch;
    if (A.tid == 0) {
        GcTrkState st = S.st;
        st.remcode = S.remcode[k]; st.remcarr = S.remcarr[k]; st.buffloc = S.buffloc[k];
        A.state[ch] = st;
        A.meta[ch] = m;
        A.ndone[ch] = m.consumed;
        if (A.hostflags) {
            if (m.finished && !was_finished) __hip_atomic_fetch_add(&A.hostflags[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (S.lp.flagsync) __hip_atomic_store(&A.hostflags[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    tail_copy_loop(A.loop + ch, &S.lp, A.tid);
}
// One workgroup (GC_TAIL_NW wavefronts) per channel: the phases above.  Up to close they end the interval the previous
// correlator launch produced; from the step tables on they plan the next one.
__global__ __launch_bounds__(64 * GC_TAIL_NW) void trk_step_tail_kernel(
    const GcChan *__restrict__ chan, GcTrkState *__restrict__ state, gnsscorr_loop_t *__restrict__ loop,
    GcStepMeta *__restrict__ meta, const uint64_t *__restrict__ wrpos, const int *__restrict__ partial,
    GcTrkUnit *__restrict__ unit, GcUnitSegs *__restrict__ segs, GcRound *__restrict__ rounds, double *__restrict__ corrI,
    double *__restrict__ corrQ, int *__restrict__ nsamp_out, gnsscorr_trklog_t *__restrict__ log, int *__restrict__ ndone,
    int *__restrict__ nco_overflow, int *__restrict__ lapped, unsigned *__restrict__ hostflags, int nch, int nper, int nseg,
    int ntap_stride, int max_n, int kcap, int plan)
{
    __shared__ __attribute__((aligned(16))) TailShared S;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nch) return;
    GC_TSTART();
    const TailArgs A{chan, state, loop, meta, wrpos, partial, unit, segs, rounds, corrI, corrQ, nsamp_out, log, ndone, nco_overflow,
                     lapped, hostflags, nper, nseg, ntap_stride, max_n, kcap, plan, (int)blockIdx.x, tid, tid & 63, tid >> 6};
    const GcChan &c = chan[A.ch];
    const int ntap = c.ntap;
    GcStepMeta m = tail_state_in(A, S);
    __syncthreads();
    const double II0_before = S.lp.II[0];
    const bool was_finished = m.finished != 0;
    GC_TSTAMP(0);       // state in
    tail_sums(A, S, m, ntap);
    __syncthreads();
    GC_TSTAMP(1);       // sums
    if (A.wave == 1) tail_nav(A, S, m.k, ntap, II0_before);
    if (A.wave == 0) tail_close(A, S, m, ntap);      // (GC_TSTAMP(2) after each period)
    __syncthreads();
    m.consumed += m.k; m.k = 0;
    const int want = S.want;
    const TailSteps q = tail_steps(S, c);
    if (want > 0) tail_step_tables(A, S, c, q);
    __syncthreads();
    GC_TSTAMP(3);       // step tables
    if (want > 1) {
        // discover, left inline: as a function (one per wavefront, one for both, or out of line) the same statements cost a
        // ten-period interval 2 000 to 3 500 clocks more, and loop-10 0.28 us per period in the bench
        if (A.wave == 2) {       // code brackets -> S.ccl
            const int lane = A.lane, pe = lane & 31;
            const bool hiend = lane >= 32;
            if (pe < want) {
                GcCodeClaims cc;
                cc.tag = cc.n = cc.pad = 0;
                cc.lo = cc.hi = 0.0;
                double end = 0.0;       // this lane's end of the bracket; the samples, wrap branch and verdict there
                int n = 0, side = 0;
                bool ok = false;
                if (q.shape_ok && q.spc > 1e-300 && q.spc < 1e300) {
                    double rc, rk, dummy;
                    int nhat;
                    gc_spec_start(S.remcode[0], S.remcarr[0], q.ci, q.spc, q.ps, q.dlen, pe, &rc, &rk, &nhat);
                    end = hiend ? rc + TAIL_BRACKET_W : rc - TAIL_BRACKET_W;
                    n = gc_period_nsamp(q.dlen, end, q.spc);
                    side = end - S.PC.smaxci < 0.0 ? 1 : 0;                          // (ref src/sdrcmn.c:614: one branch for the whole bracket)
                    if (n > 0 && n <= (1 << 24)) ok = gc_code_claims<true>(S.PC, end, n + 2 * c.smax, cc, &dummy);
                }
                bool same = ok && pair_other(ok ? 1 : 0, lane) != 0 && pair_same(n, lane) && pair_same(side, lane);
                same = same && pair_same(cc.i0, lane) && pair_same(cc.q, lane) && pair_same(cc.nl, lane) && pair_same(cc.jsum, lane);
#pragma unroll
                for (int i = 0; i < 13; i++) same = same && pair_same(cc.dm[i], lane);
                const double other = pair_other(end, lane);
                if (!hiend) {
                    // (the discovering step allows the widest tail; the chain's instance may be narrower)
                    cc.tag = (same && n + 2 * c.smax - cc.jsum <= gc_tail_max(gc_tail_class(c.smax))) ? 1 : 0;
                    cc.n = n; cc.lo = end; cc.hi = other;
                    S.ccl[pe] = cc;
                }
            }
        }
        if (A.wave == 3) {       // carrier brackets -> S.kcl
            const int lane = A.lane, pe = lane & 31;
            const bool hiend = lane >= 32;
            if (pe < want) {
                GcCarClaims ck{};
                double end = 0.0;
                int n = 0;
                bool ok = false;
                if (q.shape_ok && q.spc > 1e-300 && q.spc < 1e300) {
                    double rc, rk, dummy;
                    gc_spec_start(S.remcode[0], S.remcarr[0], q.ci, q.spc, q.ps, q.dlen, pe, &rc, &rk, &n);
                    end = hiend ? rk + TAIL_BRACKET_W : rk - TAIL_BRACKET_W;
                    if (n > 0 && n <= (1 << 24)) {
                        GcCarStepC CK;
                        gc_car_stepc_init(CK, S.PK, c.nsamp + 16);
                        ok = gc_carrier_claims_step<true>(S.PK, CK, end, n, ck, &dummy);
                    }
                }
                bool same = ok && pair_other(ok ? 1 : 0, lane) != 0 && pair_same(ck.tag, lane) && pair_same(ck.nl, lane);
                same = same && pair_same(ck.i0, lane) && pair_same(ck.nseg, lane) && pair_same(ck.kprem, lane);
#pragma unroll
                for (int i = 0; i < GC_CLAIM_CSEG; i++) same = same && pair_same(ck.dm[i], lane);
                const double other = pair_other(end, lane);
                if (!hiend) {
                    // (tag 2, a period inside one binade, carries its own conditions and is judged by them: it needs no bracket)
                    ck.tag = same ? ck.tag : (ok && ck.tag == 2 ? 2 : 0);
                    ck.nl = n; ck.lo = end; ck.hi = other;
                    S.kcl[pe] = ck;
                }
            }
        }
        __syncthreads();
    }
    GC_TSTAMP(8);       // claims
    if (want > 0) {
        if (A.wave == 1) tail_code_chain_any(A, S, c, q, want);
        else if (A.wave == 0 && want > 1) tail_carrier_chain(A, S, c, q, want);
    }
    GC_TSTAMP(4);       // chain
    tail_table_tasks(A, S, c, q, want);
    __syncthreads();
    GC_TSTAMP(5);       // tables
    const int k = S.k;
    tail_out(A, S, c, m.done, k);
    GC_TSTAMP(6);       // checks, tables out, rounds
    if (want > 0) { m.k = k; m.kcap = kcap; m.pbase = m.done; m.done += k; }
    // the run is over for this channel once nothing is planned and nothing waits to be closed
    if (m.k == 0 && (m.done >= nper || S.starved || !plan)) m.finished = 1;
    tail_state_out(A, S, m, k, was_finished);
    GC_TSTAMP(7);       // state out
}

// (channel, period of its interval, quarter) -> one workgroup: ps_unit on four rounds of the period, one per wavefront
template <int DTYPE, int NTAP, int NIT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(trk_tap_waves_per_eu(NTAP), 8)))
void trk_step_corr_kernel(const GcChan *__restrict__ chan, const GcStepMeta *__restrict__ meta, const GcTrkUnit *__restrict__ unit,
                          const GcUnitSegs *__restrict__ segs, const GcRound *__restrict__ rounds, int *__restrict__ partial,
                          int nch, int kcap, int nseg, int ntap_stride, int max_n)
{
    using L = PsLayout<DTYPE, NIT>;
    __shared__ __attribute__((aligned(16))) char smem[L::bytes(NTAP)];
    // block -> (period, round, channel), channel fastest: the channels of one period read the same IF window
    const int tid = threadIdx.x;
    const int b = blockIdx.x;
    const int ch = b % nch, seg = (b / nch) % nseg, e = b / (nch * nseg);
    if (e >= kcap) return;
    const GcChan &c = chan[ch];
    if (c.dtype != DTYPE || c.ntap > NTAP) return;
    if (e >= meta[ch].k) return;
    const size_t ui = (size_t)ch * kcap + e;
    const GcTrkUnit u = unit[ui];
    ps_unit<DTYPE, NTAP, NIT>(c, u, segs + ui, rounds + (ui * nseg + seg) * 4, partial + (ui * nseg + seg) * 2 * ntap_stride,
                              ntap_stride, max_n, 4, seg, 0, smem, tid, nullptr);
}

// one launch per dtype present among the channels
template <int DTYPE>
int launch_step_corr(gnsscorr_ctx *ctx, int kcap)
{
    if (ctx->smax_max > 64) return gc_fail(GNSSCORR_EINVAL, "trk_step: tap offset %d samples (<= 64 supported)", ctx->smax_max);
    constexpr int NIT = DTYPE == 1 ? 1 : 2;
    const GcLoop &lp = ctx->loop;
    const unsigned grid = (unsigned)(ctx->nch * lp.step_nseg * kcap);
    // (the channels of a set share their tap count, so an instance needs no lower bound)
    return trk_with_tap_bucket(ctx->ntap, [&](auto N, int) {
        hipLaunchKernelGGL((trk_step_corr_kernel<DTYPE, decltype(N)::value, NIT>), dim3(grid), dim3(256), 0, ctx->stream,
                           ctx->dchan.p, lp.dstep_meta.p, lp.step.unit.p, lp.step.segs.p, lp.step.rounds.p, lp.step.partial.p, ctx->nch,
                           kcap, lp.step_nseg, ctx->ntap, ctx->max_n);
        GC_HIP(hipGetLastError());
        return 0;
    });
}

// workgroups per period in step mode: four rounds (one per wavefront) each
int step_nseg(int dtype, int max_n)
{
    const int nit = trk_ps_nit(dtype, 2);
    const int groups = (15 + max_n * dtype + 15) / 16 + 1;
    return (groups + 256 * nit - 1) / (256 * nit);
}

// closes the intervals the previous correlator launch produced and plans the next ones (plan = 0: closes only)
int launch_step_tail(gnsscorr_ctx *ctx, int kcap, int plan)
{
    if (kcap < 1 || kcap > GC_STEP_KMAX) return gc_fail(GNSSCORR_EINVAL, "trk_step: %d periods per step (1..%d)", kcap, GC_STEP_KMAX);
    GcLoop &lp = ctx->loop;
    hipLaunchKernelGGL(trk_step_tail_kernel, dim3(ctx->nch), dim3(64 * GC_TAIL_NW), 0, ctx->stream, ctx->dchan.p,
                       ctx->state.cur(), lp.dloop.p, lp.dstep_meta.p, lp.dwrpos.p, lp.step.partial.p, lp.step.unit.p,
                       lp.step.segs.p, lp.step.rounds.p, ctx->out.dcorrI.p, ctx->out.dcorrQ.p, ctx->out.nsamp.p, lp.dlog.p, lp.ddone.p,
                       ctx->out.dnco_overflow.p, lp.dlapped.p, lp.hostflags.dev, ctx->nch, lp.run_nper, lp.step_nseg, ctx->ntap, ctx->max_n,
                       kcap, plan);
    GC_HIP(hipGetLastError());
    return 0;
}

// One step of the run of loop.run_nper periods: the tail, then the correlator.  plan = 0: the tail that closes the run,
// alone and untimed.
int loop_step(gnsscorr_ctx *ctx, int kcap, int plan)
{
    if (!plan) return launch_step_tail(ctx, kcap, 0);
    {
        GcTimed t(ctx, "trk_step_tail");
        GC_TRY(launch_step_tail(ctx, kcap, 1));
    }
    for (int dtype = 1; dtype <= 2; dtype++) {
        if (!ctx->have_dtype[dtype]) continue;
        GcTimed t(ctx, "trk_step_corr");
        GC_TRY(dtype == 2 ? launch_step_corr<2>(ctx, kcap) : launch_step_corr<1>(ctx, kcap));
    }
    return GNSSCORR_OK;
}

}  // namespace

// ---- the host driver --------------------------------------------------------------------------------------
extern "C" int gnsscorr_loop_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_loop_t *lp)
{
    GC_TRY(gc_chan_range("loop_set", ctx, ch0, nch, lp));
    for (int i = 0; i < nch; i++) {
        const gnsscorr_loop_t &l = lp[i];
        const int ntap = ctx->hchan[ch0 + i].ntap;
        if (l.ne < 0 || l.ne >= ntap || l.nl < 0 || l.nl >= ntap)
            return gc_fail(GNSSCORR_EINVAL, "loop_set: channel %d: early/late tap index %d/%d of %d taps", ch0 + i, l.ne, l.nl, ntap);
        if (l.loopms < 1 || l.rate < 1 || l.rate > 20)
            return gc_fail(GNSSCORR_EINVAL, "loop_set: channel %d: loopms %d, rate %d (rate 1..20)", ch0 + i, l.loopms, l.rate);
    }
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_quiesce(ctx));
    GcLoop &L = ctx->loop;
    GC_HIP(hipMemcpyAsync(L.dloop + ch0, lp, sizeof(gnsscorr_loop_t) * nch, hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nch; i++) {
        L.isset[ch0 + i] = 1;
        if (lp[i].loopms > L.kmax) L.kmax = lp[i].loopms < GC_STEP_KMAX ? lp[i].loopms : GC_STEP_KMAX;
        if (lp[i].flagsync) L.sync_hint = true;
    }
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_loop_get(gnsscorr_ctx *ctx, int ch0, int nch, gnsscorr_loop_t *lp)
{
    GC_TRY(gc_chan_range("loop_get", ctx, ch0, nch, lp));
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_quiesce(ctx));
    GC_HIP(hipMemcpyAsync(lp, ctx->loop.dloop + ch0, sizeof(gnsscorr_loop_t) * nch, hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

// the step buffers: one filter interval (GC_STEP_KMAX periods at most) per channel
static int ensure_step_buffers(gnsscorr_ctx *ctx)
{
    GcLoop &L = ctx->loop;
    if (L.step_nseg) return GNSSCORR_OK;           // set once every buffer below has its size
    int nseg = 1;
    for (int i = 0; i < ctx->nch; i++) {
        const int s = step_nseg(ctx->hchan[i].dtype, ctx->max_n);
        if (s > nseg) nseg = s;
    }
    // (gnsscorr_set_channels accepts periods of up to 262144 samples: 65 workgroups of four rounds for either sample type)
    const int most = step_nseg(2, 262144 + 100);
    if (nseg > most)
        return gc_fail(GNSSCORR_EINVAL, "trk_run_loop: period of %d samples too long (%d workgroups of four rounds, %d at most)",
                       ctx->max_n, nseg, most);
    GC_TRY(L.step.reserve(ctx, (size_t)ctx->nch * GC_STEP_KMAX, nseg, 4, ctx->ntap));   // four rounds (one per wavefront) per workgroup
    GC_RESERVE(ctx, L.dlapped, 1);
    GC_TRY(L.hostflags.reserve(16, hipHostMallocMapped));
    GC_RESERVE(ctx, L.dstep_meta, ctx->nch);
    L.step_nseg = nseg;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_trk_run_loop(gnsscorr_ctx *ctx, int nperiod) { return gc_trk_run_loop(ctx, nperiod, nullptr); }

// wp_ch: nullptr, or the write position each channel is tracked up to ([nch]; 0 starves the channel at once: it plans
// no period and keeps its state), which the caller read under the context's lock
int gc_trk_run_loop(gnsscorr_ctx *ctx, int nperiod, const uint64_t *wp_ch)
{
    if (!ctx || nperiod <= 0) return gc_fail(GNSSCORR_EINVAL, "trk_run_loop: nperiod %d", nperiod);
    if (!ctx->nch) return gc_fail(GNSSCORR_ESTATE, "trk_run_loop: no channels set");
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_ensure_trk_outputs(ctx, nperiod));
    GC_TRY(ensure_step_buffers(ctx));
    GC_TRY(gc_loop_take_state(ctx));
    GcLoop &L = ctx->loop;
    L.run_nper = nperiod;
    const size_t units = (size_t)ctx->nch * nperiod;
    GC_RESERVE(ctx, L.dlog, units);
    GC_HIP(hipMemsetAsync(L.dlog, 0, sizeof(gnsscorr_trklog_t) * units, ctx->stream));
    GC_HIP(hipMemsetAsync(ctx->out.dcorrI, 0, sizeof(double) * units * ctx->ntap, ctx->stream));
    GC_HIP(hipMemsetAsync(ctx->out.dcorrQ, 0, sizeof(double) * units * ctx->ntap, ctx->stream));
    GC_HIP(hipMemsetAsync(ctx->out.nsamp, 0, sizeof(int) * units, ctx->stream));
    GC_HIP(hipMemsetAsync(L.dstep_meta, 0, sizeof(GcStepMeta) * ctx->nch, ctx->stream));
    GC_HIP(hipMemsetAsync(L.dlapped, 0, sizeof(int), ctx->stream));
    // write position of each channel's ring (ref src/sdrtrk.c:26-28: fendbuffsize*buffcnt)
    uint64_t wpr[2];
    GC_TRY(gc_ring_positions(ctx, wpr));
    std::vector<uint64_t> wp(ctx->nch);
    for (int i = 0; i < ctx->nch; i++) wp[i] = wp_ch ? wp_ch[i] : wpr[ctx->hdesc[i].ftype - 1];
    GC_HIP(hipMemcpyAsync(L.dwrpos, wp.data(), sizeof(uint64_t) * ctx->nch, hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));          // (wp is a local; the flags below are host memory)
    L.hostflags[0] = 0;
    L.hostflags[1] = L.sync_hint ? 1u : 0u;     // (some channel is known to be synchronised: steps of loopms periods from the start)
    // Every step advances every channel that still has work by at least one period, so nperiod steps always suffice;
    // channels whose nav bit is synchronised advance by up to loopms periods per step.  The host keeps a bounded number
    // of steps ahead of the device and stops as soon as the device says every channel is done (a pinned word the tail
    // kernel updates).
    const int kmax = L.kmax < 1 ? 1 : L.kmax;
    const int BURST = 4, AHEAD = GC_LOOP_AHEAD;
    int steps = 0, burst = 0;
    while (steps <= nperiod) {
        if (burst >= AHEAD) {                           // at most AHEAD bursts in flight
            GC_HIP(hipEventSynchronize(ctx->ev_burst[burst % AHEAD]));
            if (L.hostflags[0] >= (unsigned)ctx->nch) break;
        }
        for (int b = 0; b < BURST && steps <= nperiod; b++, steps++) {
            // periods per step: 1 while no channel is synchronised (a performance hint only: the tail never plans more
            // than kcap periods, and any kcap >= 1 is correct)
            GC_TRY(loop_step(ctx, L.hostflags[1] ? kmax : 1, 1));
        }
        GC_HIP(hipEventRecord(ctx->ev_burst[burst % AHEAD], ctx->stream));
        burst++;
    }
    // close whatever the last correlator launch produced
    GC_TRY(loop_step(ctx, 1, 0));
    if (L.hostflags[1]) L.sync_hint = true;
    ctx->out.fin_pending = false;           // the outputs are the main stream's own work
    ctx->out.last_nepoch = nperiod;
    L.last_nper = nperiod;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_trk_fetch_log(gnsscorr_ctx *ctx, gnsscorr_trklog_t *log, int *ndone)
{
    if (!ctx || !ctx->loop.last_nper) return gc_fail(GNSSCORR_ESTATE, "trk_fetch_log: no completed trk_run_loop");
    GC_HIP(hipSetDevice(ctx->device));
    const size_t units = (size_t)ctx->nch * ctx->loop.last_nper;
    if (log) GC_HIP(hipMemcpyAsync(log, ctx->loop.dlog, sizeof(gnsscorr_trklog_t) * units, hipMemcpyDeviceToHost, ctx->stream));
    if (ndone) GC_HIP(hipMemcpyAsync(ndone, ctx->loop.ddone, sizeof(int) * ctx->nch, hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return gc_nco_check(ctx);
}

extern "C" int gnsscorr_trk_loop_lapped(gnsscorr_ctx *ctx, int *nlapped)
{
    if (!ctx || !nlapped) return gc_fail(GNSSCORR_EINVAL, "trk_loop_lapped: null argument");
    if (!ctx->loop.last_nper) return gc_fail(GNSSCORR_ESTATE, "trk_loop_lapped: no completed trk_run_loop");
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(hipMemcpyAsync(nlapped, ctx->loop.dlapped, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}
