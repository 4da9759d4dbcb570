// gnsscorr_ctx.h -- host-side context object behind the opaque gnsscorr_ctx, and the move-only types it owns its
// resources by: GcDevBuf / GcPinBuf (memory), GcEvent / GcStream (handles).  Deleting the context releases all of them.
// Also the correlator launches' buffer set (GcUnitBufs), the tracking launchers' argument block (GcTrkLaunch), the record
// of a schedule stage (GcStage), gc_chan_range.
#pragma once

#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <cstring>
#include "gnsscorr_internal.h"

struct gnsscorr_ctx;
int gc_dev_alloc(gnsscorr_ctx *ctx, void **p, size_t bytes);   // hipMalloc + the context's poison fill, if on

// Owning device buffer (hipMalloc / hipFree), move-only.  reserve() only grows: a larger request frees the old buffer
// (hipFree synchronises the device, so no launch still reads it) and allocates through gc_dev_alloc.
template <class T>
struct GcDevBuf {
    T *p = nullptr;
    size_t n = 0;               // elements
    GcDevBuf() = default;
    GcDevBuf(GcDevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    GcDevBuf &operator=(GcDevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~GcDevBuf() { reset(); }
    void reset()
    {
        if (p) hipFree(p);
        p = nullptr;
        n = 0;
    }
    int reserve(gnsscorr_ctx *ctx, size_t elems)
    {
        if (elems <= n) return 0;
        reset();
        int rc = gc_dev_alloc(ctx, (void **)&p, sizeof(T) * elems);
        if (!rc) n = elems;
        return rc;
    }
    operator T *() const { return p; }
};

// Owning pinned host buffer (hipHostMalloc / hipHostFree), move-only and grow-only like GcDevBuf; dev is the device
// pointer of a mapped one.
template <class T>
struct GcPinBuf {
    T *p = nullptr, *dev = nullptr;
    size_t n = 0;
    GcPinBuf() = default;
    GcPinBuf(GcPinBuf &&o) noexcept : p(o.p), dev(o.dev), n(o.n) { o.p = o.dev = nullptr; o.n = 0; }
    GcPinBuf &operator=(GcPinBuf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; dev = o.dev; n = o.n; o.p = o.dev = nullptr; o.n = 0; }
        return *this;
    }
    ~GcPinBuf() { reset(); }
    void reset()
    {
        if (p) hipHostFree(p);
        p = dev = nullptr;
        n = 0;
    }
    int reserve(size_t elems, unsigned flags = hipHostMallocDefault)
    {
        if (elems <= n) return 0;
        reset();
        GC_HIP(hipHostMalloc((void **)&p, sizeof(T) * elems, flags));
        if (flags & hipHostMallocMapped) GC_HIP(hipHostGetDevicePointer((void **)&dev, p, 0));
        n = elems;
        return 0;
    }
    operator T *() const { return p; }
};

// returns the call's error code from the calling function, if it gives one
#define GC_TRY(call)                                                            \
    do {                                                                        \
        int rc_ = (call);                                                       \
        if (rc_) return rc_;                                                    \
    } while (0)
#define GC_RESERVE(ctx, buf, elems) GC_TRY((buf).reserve((ctx), (elems)))

// Owning event (hipEventCreateWithFlags / hipEventDestroy), move-only.  make() keeps an event it already has.
struct GcEvent {
    hipEvent_t e = nullptr;
    GcEvent() = default;
    GcEvent(GcEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    GcEvent &operator=(GcEvent &&o) noexcept
    {
        if (this != &o) { reset(); e = o.e; o.e = nullptr; }
        return *this;
    }
    ~GcEvent() { reset(); }
    void reset()
    {
        if (e) hipEventDestroy(e);
        e = nullptr;
    }
    int make(unsigned flags = hipEventDisableTiming)
    {
        if (!e) GC_HIP(hipEventCreateWithFlags(&e, flags));
        return 0;
    }
    operator hipEvent_t() const { return e; }
};

// A stream, move-only: its own non-blocking one (make(), destroyed with it; keeps a stream it already has) or the
// caller's (borrow(), never destroyed).
struct GcStream {
    hipStream_t s = nullptr;
    bool own = false;
    GcStream() = default;
    GcStream(GcStream &&o) noexcept : s(o.s), own(o.own) { o.s = nullptr; o.own = false; }
    GcStream &operator=(GcStream &&o) noexcept
    {
        if (this != &o) { reset(); s = o.s; own = o.own; o.s = nullptr; o.own = false; }
        return *this;
    }
    ~GcStream() { reset(); }
    void reset()
    {
        if (own) hipStreamDestroy(s);
        s = nullptr;
        own = false;
    }
    int make()
    {
        if (s) return 0;
        GC_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        own = true;
        return 0;
    }
    void borrow(hipStream_t callers)
    {
        reset();
        s = callers;
    }
    operator hipStream_t() const { return s; }
};

static_assert(!std::is_copy_constructible<GcEvent>::value && !std::is_copy_assignable<GcEvent>::value, "GcEvent owns its event");
static_assert(!std::is_copy_constructible<GcStream>::value && !std::is_copy_assignable<GcStream>::value, "GcStream owns its stream");

struct GcRing {
    int8_t  *mem = nullptr;   // own, or the caller's buffer
    GcDevBuf<int8_t> own;
    int      dtype = 0;
    uint64_t ringlen = 0;     // samples
    uint64_t wrpos = 0;       // samples written so far (fendbuffsize*buffcnt)
};

struct GcTimer {
    std::vector<std::pair<GcEvent, GcEvent>> pending;   // launches whose times are still to be read
    double total_ms = 0.0;
    int launches = 0;
};

// Ingest (gnsscorr_ring_push*, gnsscorr_api.hip): the copy stream, two pinned staging buffers (and device staging for
// the packed formats).  Made on the first push, for the context's lifetime.
struct GcIngest {
    GcStream stream;
    GcPinBuf<int8_t> pin[2];
    GcDevBuf<uint8_t> dstage[2];
    GcEvent ev_pin[2];                             // the transfer that last used the staging slot
    bool pin_busy[2] = {false, false};
    int pin_next = 0;
    GcEvent ev_in;                                 // the last transfer: the compute stream waits on it before it reads the ring
    bool in_pending = false;
    bool ready = false;                            // everything above is made (a failed init is completed by the next call)
};

// The committed tracking state, ping-pong: a batch's planner chains cur() into next() and the batch commits it once every
// launch is issued; the closed loop, both hand-overs and trk_set/get_state work on cur() in place
struct GcTrkStateBuf {
    GcDevBuf<GcTrkState> buf[2];   // [nch] each
    int icur = 0;
    bool touched = true;           // written outside gnsscorr_trk_run since its last batch: that batch does not look ahead
    GcTrkState *cur() const { return buf[icur]; }
    GcTrkState *next() const { return buf[icur ^ 1]; }
    void commit() { icur ^= 1; }
};

// What a tracking run of either kind (gnsscorr_trk_run, gc_trk_run_loop) leaves for the fetch calls, per channel set
// (gc_ensure_trk_outputs, gnsscorr_trk.hip).  nsamp and the two counters are written by the batched tracker's table
// kernels on the tables stream (the closed loop's are on the main stream); their readers are on the main stream behind
// the last batch's correlator, which stands behind every table kernel queued so far.
struct GcTrkOut {
    GcDevBuf<double> dcorrI, dcorrQ;               // [unit][ntap]
    GcDevBuf<double> dsumI, dsumQ;                 // [nch][ntap] batch sums
    GcDevBuf<int> nsamp;                           // [unit]
    GcDevBuf<double> dprompt;                      // [2][unit] tap 0 of dcorrQ, dcorrI (gnsscorr_trk_fetch_prompt; made on first use)
    GcDevBuf<int> dnco_overflow;                  // units whose NCO tables overflowed since the last fetch
    GcDevBuf<int> dring_viol;                      // planned periods outside what the ring holds, since the last fetch
    size_t units = 0;                              // (channel, period) units the per-unit buffers are sized for
    int last_nepoch = 0;                           // periods per channel of the last completed run (0: none yet)
    bool fin_pending = false;                      // a batched run was issued and the streams have not been drained since
};

// What a correlator launch reads its (channel, period) units from and writes its sums to.  The batch's plan slots, the
// closed loop's step buffers and the two scratch sets of the drop-in symbols (gnsscorr_compat.hip) each own one.
struct GcUnitBufs {
    GcDevBuf<GcTrkUnit> unit;      // [unit] per-unit constants
    GcDevBuf<GcUnitSegs> segs;     // [unit]: the unit's carrier / code NCO piece tables
    GcDevBuf<GcRound> rounds;      // [unit][nseg][rounds per workgroup]: GC_MAXR; 4 in the closed loop, one per wavefront
    GcDevBuf<int> partial;         // [unit][nseg][2*ntap] int32 partial sums
    int reserve(gnsscorr_ctx *ctx, size_t units, int nseg, int rounds_per_workgroup, int ntap)
    {
        GC_RESERVE(ctx, unit, units);
        GC_RESERVE(ctx, segs, units);
        GC_RESERVE(ctx, rounds, units * nseg * rounds_per_workgroup);
        GC_RESERVE(ctx, partial, units * nseg * 2 * ntap);
        return 0;
    }
};

// One plan slot: the planner stream expands batch k+1 into one slot while batch k is correlated from the other
struct GcPlanSlot {
    GcDevBuf<GcTrkPlan> plan;      // [unit]
    GcUnitBufs bufs;               // rounds: GC_MAXR per workgroup
    GcDevBuf<unsigned short> etab; // [unit][GC_EDGTAB] start samples of the batch's chip edges (trk_edges -> trk_corr)
};

// The argument block of the tracking launchers (gnsscorr_trk.hip): a plain host struct, never a kernel argument
struct GcTrkLaunch {
    hipStream_t st;
    const GcChan *chan;            // device channel table, [nch]
    const GcTrkPlan *plan;         // [nch][nepoch]
    const GcUnitBufs *bufs;
    int nch, nepoch, nseg, max_n, smax_max;
    int ntap;                      // taps per channel, and the stride of the partial sums
    unsigned short *etab = nullptr;    // edge table (GcPlanSlot::etab), or null: the correlator finds the edges itself
    int *nsamp_out = nullptr;      // [nch][nepoch] samples per period, or null
    int *nco_overflow;             // device counter of units whose NCO tables did not fit (their outputs are zero)
    double *corrI, *corrQ, *sumI, *sumQ;   // trk_finish: [unit][ntap] correlator outputs, [nch][ntap] batch sums
    unsigned long long *scratch;   // GC_FINISH_SCRATCH words per channel, zero before the first launch and after every one
};
int gc_launch_trk_expand(const GcTrkLaunch &a);
// one launch serves every channel of that dtype; callers invoke it once per dtype present in the channel set
int gc_launch_trk_corr(const GcTrkLaunch &a, int dtype);
int gc_launch_trk_finish(const GcTrkLaunch &a);
// the three back to back on a.st, for a channel set of one dtype (the drop-in symbols)
static inline int gc_launch_trk_chain(const GcTrkLaunch &a, int dtype)
{
    GC_TRY(gc_launch_trk_expand(a));
    GC_TRY(gc_launch_trk_corr(a, dtype));
    return gc_launch_trk_finish(a);
}

// The batched tracker (gnsscorr_trk.hip): what gnsscorr_trk_run owns, per channel set.  The planner (a short sequential
// NCO chain per channel) runs one batch ahead on its own stream: plan entries and the chained state are double buffered,
// so batch k+1 is planned while batch k is correlated.  A look-ahead plan is dropped when the caller changes the state
// or the batch length.
struct GcBatch {
    GcPlanSlot slot[2];
    size_t units = 0;                              // (channel, period) units every buffer here is sized for
    int nseg = 1;
    // claims of the batch being planned (discovery pass -> chain), two buffers: while the chain of one batch reads
    // its claims the discovery pass of the NEXT batch fills the other one from the same input state, on its own stream
    GcDevBuf<int> dspec2[2];
    GcDevBuf<unsigned long long> dfinish;          // batch-sum scratch of trk_finish
    bool spec_pending = false;                     // the discovery stream has work whose end ev_spec marks
    bool spec_ahead_valid = false;                 // dspec2[spec_ahead_buf] holds claims for the batch that starts at spec_ahead_state
    int spec_ahead_buf = 0, spec_ahead_nepoch = 0;
    int spec_last_buf = 0, spec_last_units = 0;    // (tools/debug) the claims the last planned batch used
    const void *spec_ahead_state = nullptr;
    int plan_slot = 0;                             // slot the next trk_run consumes
    bool ahead_valid = false;                      // slot[plan_slot] already planned (look-ahead)
    int ahead_nepoch = 0;
};

#define GC_LOOP_AHEAD 3         // launch bursts gc_trk_run_loop keeps in flight
// The closed loop (gnsscorr_loop.hip): what gnsscorr_trk_run_loop owns, per channel set.  The step buffers hold one filter
// interval per channel (GC_STEP_KMAX periods at most): unit constants, NCO tables, rounds, partial sums
struct GcLoop {
    GcDevBuf<gnsscorr_loop_t> dloop;               // [nch] the channels' loop states
    std::vector<char> isset;                       // [nch] the channel's loop constants have been set (gnsscorr_loop_set)
    GcDevBuf<GcStepMeta> dstep_meta;               // [nch]
    GcUnitBufs step;                               // [nch][GC_STEP_KMAX] units, step_nseg workgroups of four rounds each
    int step_nseg = 0;
    GcPinBuf<unsigned> hostflags;                  // mapped: [0] channels whose run is over, [1] some channel has its nav bit synchronised
    int kmax = 1;                                  // largest loopms among the channels' loop states (gnsscorr_loop_set)
    bool sync_hint = false;                        // some channel had its nav bit synchronised when last seen
    GcDevBuf<gnsscorr_trklog_t> dlog;              // [nch][nperiod] one row per period
    GcDevBuf<int> dlapped;                         // periods of the last run read after the writer lapped them
    GcDevBuf<int> ddone;                           // [nch] periods the last run finished
    GcDevBuf<uint64_t> dwrpos;                     // [nch] the write position each channel is tracked up to
    int run_nper = 0;                              // periods of the run being issued (the tail's bound)
    int last_nper = 0;                             // > 0: the last run was a closed-loop one of that many periods
};

// One per-channel stage behind the closed loop of the schedule, off until its gnsscorr_rx_*_set; the operations are in
// gnsscorr_stage.h
template <class Prm, class St>
struct GcStage {
    std::vector<Prm> prm;                          // [nch]; all zero: the channel's stage is off
    int on = 0;                                    // channels whose stage is on
    GcDevBuf<Prm> dprm;                            // [nch]
    GcDevBuf<St> dst;                              // [nch] the stage's state
    GcPinBuf<int> list;                            // mapped: [nch] the channels of a launch (host writes, kernel reads)
    template <class Check> int set(gnsscorr_ctx *ctx, const char *who, int ch0, int nch, const Prm &p, Check check);
    int status(gnsscorr_ctx *ctx, St *out) const;
    int start(gnsscorr_ctx *ctx);
    int fill(const std::vector<gnsscorr_rxstat_t> &rxst);
};

// The receiver schedule (gnsscorr_rx.hip): sdrthread()'s per-channel state, kept by the host
struct GcRx {
    bool on = false;
    int retry_ms = 0;                              // the reference's ACQSLEEP, counted on each channel's sample clock
    std::vector<gnsscorr_rxstat_t> st;             // [nch] (cnt is filled in by gnsscorr_rx_status)
    GcStage<gnsscorr_lockprm_t, gnsscorr_lock_t> lock;      // the lock monitor (gnsscorr_lock.hip)
    std::vector<int> losses;                       // [nch] times the channel was sent back to SEARCH
    std::vector<int> lock_listed;                  // the channels of the launch whose words are still to be read
    GcPinBuf<unsigned> lock_lost;                  // mapped: [nch] 1: the launch declared the channel lost (kernel writes)
    GcStage<gnsscorr_bsyncprm_t, gnsscorr_bsync_t> bsync;   // bit synchronisation by symbol energy (gnsscorr_bsync.hip)
    GcDevBuf<int> dbsync_applied;                  // [nch] times the kernel preset the channel's loop state
    GcStage<gnsscorr_cfmprm_t, gnsscorr_cfm_t> cfm;         // the correlation monitor (gnsscorr_cfm.hip)
};

// Frames, observables and epochs behind every step (gnsscorr_rx_nav_*, gnsscorr_rx.hip): the core object of
// csrc/sdr_rxnav.c, owned, and the host arrays a step's fetches land in.  off() is what gnsscorr_set_channels,
// gnsscorr_rx_start and a gnsscorr_ring_create under the channels do to it.
struct GcNav {
    gnsscorr_rxnav_t *nv = nullptr;                // nullptr: the driver is off
    std::vector<gnsscorr_trklog_t> log;            // [nch][max_periods]
    std::vector<double> ii0;                       // [nch][max_periods]
    std::vector<int> ndone, tracking;              // [nch]
    std::vector<uint64_t> cnt;                     // [nch]
    std::vector<gnsscorr_rxstat_t> st;             // [nch] (schedule on)
    GcNav() = default;
    GcNav(const GcNav &) = delete;
    GcNav &operator=(const GcNav &) = delete;
    ~GcNav() { off(); }
    void off()
    {
        if (nv) gnsscorr_rxnav_destroy(nv);
        nv = nullptr;
    }
};

// The FFT twiddle tables (gc_acq_twiddles, gnsscorr_acq.hip), made once per context on first use: they depend on nothing
// the caller configures.  Acquisition, gnsscorr_fft16k, gnsscorr_pspec and the IF monitor read them.
struct GcFftTables {
    GcDevBuf<float2> tw16k;     // exp(-2 pi i t/16384), t < 16384
    GcDevBuf<float2> tw32k;     // exp(-2 pi i t/32768), t < 16384
    GcDevBuf<float2> tw32p;     // the same twiddles in pass order: exp(-2 pi i freq_of(p)/32768), p < 16384
    GcDevBuf<float2> tw64p1;    // exp(-2 pi i freq_of(p)/65536) and
    GcDevBuf<float2> tw64p3;    // exp(-2 pi i 3 freq_of(p)/65536), pass order (the 65536-point path)
    bool ready = false;         // the tables' init kernels are queued on the main stream, the kernels' LDS sizes are set
};

// Carrier NCO of one Doppler bin over the (ncoh + 1)*nsamp samples of a group (ncoh = 1: the 2*nsamp acquisition
// window), phase 0 at its first sample (ref src/sdrcmn.c:761): the reference's running sum as a piece table
// (gnsscorr_nco.h)
struct GcAcqCar {
    int n, pad;
    int k0[GC_NCAR];
    GcCarSeg seg[GC_NCAR];
};

// The dimensions of a prepared search and the layout of its arrays, handed to the kernels by value (acq_fwd, acq_corr and
// acq_corr64 build theirs from scalar arguments).  iter: an iteration of the search, a group of ncoh code periods; slot =
// iter * H + hypothesis index, H the grid's bit-edge hypotheses (1 without).
struct GcAcqDims {
    int maxfreq;                // the largest bin count of a channel
    int maxintg;                // the largest iteration count, intg / ncoh
    int maxslot;                // the largest iterations x H of a grid (not the product of the two maxima)
    int L;                      // transform length of the channel set: 32768, or 65536 when a period exceeds 16384 samples
    // rows[ch][iter][bin]: one bin's record (bin 0: the bins of the iteration)
    template <class T> GC_HDM T *row(T *rows, int ch, int it, int bin = 0) const
    {
        return rows + (((size_t)ch * maxintg + it) * maxfreq + bin);
    }
    // arrivals[ch][iter]: the workgroups of the channel that are done with the iteration
    GC_HDM int *arrival(int *arrivals, int ch, int it) const { return arrivals + (ch * maxintg + it); }
    // X[grid][slot][bin][L]: X[f + 16384 q] at [q][pass position of f].  A 65536-point channel set has no hypotheses
    // (gnsscorr_acq_set_bitedge refuses it; acq_prepare checks): there slot = iter and maxslot == maxintg.
    template <class T> GC_HDM T *x(T *X, int grid, size_t slot, int bin) const
    {
        return X + (((size_t)grid * maxslot + slot) * maxfreq + bin) * (size_t)L;
    }
    GC_HDM size_t x_slot_stride() const { return (size_t)maxfreq * L; }     // from a slot to the next, same grid and bin
    // C[ch][L]: the channel's code spectrum, laid out as a slot of X
    template <class T> GC_HDM T *code(T *C, int ch) const { return C + (size_t)ch * L; }
    // prompt[ch][GNSSCORR_MAXCOH][2]: the prompt sum (I, Q) of period m of the channel's refine span
    template <class T> GC_HDM static T *prompt(T *prompt, int ch, int m) { return prompt + ((size_t)ch * GNSSCORR_MAXCOH + m) * 2; }
    static size_t prompt_ints(int nch) { return (size_t)nch * GNSSCORR_MAXCOH * 2; }
};

// Acquisition (gnsscorr_acq.hip): what depends on the channel set and its coherent setting
struct GcAcq {
    bool prepared = false;      // acq_prepare has sized the buffers below and queued the carrier tables and code spectra
    int nch = 0, ngrid = 0;     // channels and frequency grids the buffers are sized for
    GcAcqDims dims = {0, 0, 0, 32768};
    GcDevBuf<GcAcqCar> car;     // [grid][bin]
    GcDevBuf<int> car_overflow;
    GcDevBuf<float2> X;         // forward spectra (GcAcqDims::x)
    GcDevBuf<float2> C;         // code spectra (GcAcqDims::code)
    GcDevBuf<GcAcqRow> rows;    // row statistics (GcAcqDims::row)
    GcDevBuf<int> arrive;       // one buffer, one clear per search: arrivals(), then done()
    int *arrivals() const { return arrive; }                                // [ch][iter] workgroups done with the iteration
    int *done() const { return arrive + (size_t)nch * dims.maxintg; }       // [ch] "acquired" flags
    size_t arrive_ints() const { return (size_t)nch * dims.maxintg + nch; }
    GcDevBuf<int> iters;        // [ch] iteration limit for acq_corr
    GcDevBuf<gnsscorr_acqres_t> res;    // [ch]
    GcDevBuf<int> edge;         // [ch] bit edge of the deciding group's best row (gnsscorr_acq_fetch_edge), -1: none
    // code-Doppler compensation (gnsscorr_acq_set_codedoppler): acq_prepare builds the tables on the host
    bool cdop = false;                  // some channel compensates: acq_fwd runs its CDOP instances, d_shifts is made
    std::vector<int32_t> shifts;        // [grid][bin][iter] (stride maxfreq, maxintg): s(b, g), zero for a grid without
    std::vector<int> back;              // [grid] the grid's look-back beyond (intg + 1)*nsamp: max(0, max s)
    GcDevBuf<int32_t> d_shifts;         // device copy of shifts (cdop only)
    GcDevBuf<double> P;         // one channel's power array (on demand)
    // carrier refinement (gnsscorr_acq_set_refine; made by the first search that lists a channel with nref > 0)
    GcDevBuf<GcAcqCar> fcar;    // [ch] carrier table of the refine span: res[ch].acqfreq over nref*nsamp samples (n 0: none)
    GcDevBuf<int> fcar_overflow;
    GcDevBuf<int> prompt;       // prompt sums of the span's periods (GcAcqDims::prompt), zero beyond nref
    GcDevBuf<gnsscorr_acqfine_t> fine;  // [ch]
    bool refined = false;       // the last search queued the refinement: fine and prompt hold its results
    std::vector<int> grid_chan;         // a representative channel per grid
    GcDevBuf<int> d_grid_chan;          // device copy of grid_chan
    GcDevBuf<uint64_t> d_grid_wrpos;    // ring write position seen by each grid
    GcDevBuf<int> d_list;               // the last run's lists, one buffer:
    int *d_chans() const { return d_list; }                 // [nch] its channels, as listed
    int *d_grids() const { return d_list + nch; }           // [ngrid] the grids that have one of them
    int *d_parts() const { return d_list + nch + ngrid; }   // [nch] its channels again, those without hypotheses first
    size_t list_ints() const { return (size_t)2 * nch + ngrid; }
    int nplain = 0;                     // how many of the last run's channels have no hypotheses
    std::vector<int> list, glist;       // host copies of d_chans() and d_grids()
    std::vector<char> listed;           // [nch] channel was part of the last run
    bool ran = false;                   // a search has been queued: there are results to fetch
};

// IF monitor (gnsscorr_spec.hip): scratch and the shape of the last run
struct GcSpec {
    GcDevBuf<float> psd;        // [nsnap][nloop][2*nfft] fp32 power per segment
    GcDevBuf<double> sum;       // [nsnap][2*nfft]
    GcDevBuf<unsigned> hist;    // [nsnap][2][GC_SPEC_HIST]
    GcDevBuf<int> maxd;         // [nsnap]
    GcDevBuf<float> win;        // Hann window of the last nfft (hanning(nfft/2), computed on the host)
    int win_n = 0;
    GcDevBuf<uint64_t> loc;     // [nsnap] first sample of each snapshot
    GcDevBuf<int> off;          // [nsnap][nloop] segment offsets
    GcDevBuf<int8_t> stage;     // the drop-in's copy of the caller's samples
    std::vector<uint64_t> hloc;
    std::vector<int> hoff;
    // the last run, for fetch
    bool ran = false, has_hist = false;
    int nsnap = 0, nfft = 0, nloop = 0, dtype = 0;
    double f_sf = 0.0;
};

struct gnsscorr_ctx {
    int device = 0;
    GcStream stream;                               // the caller's, or the context's own
    std::mutex mtx;

    GcRing ring[2];
    GcIngest in;

    // channels
    int nch = 0;
    std::vector<GcChan> hchan;
    std::vector<gnsscorr_chan_t> hdesc;         // host copies (code/freq/corrp pointers re-targeted)
    std::vector<double> hfcf;                   // [nch] gnsscorr_acq_set_codedoppler's f_cf, 0: no compensation
    std::vector<std::vector<short>> hcode;
    std::vector<std::vector<double>> hfreq;
    std::vector<std::vector<int>> hcorrp;
    GcDevBuf<GcChan> dchan;
    GcDevBuf<int8_t> dcodes;
    GcDevBuf<double> dfreqs;
    int ntap = 0, smax_max = 0, max_n = 0;
    bool have_dtype[3] = {false, false, false};    // [dtype] some channel reads a ring of that dtype

    // tracking: the committed state, the batched tracker, the closed loop, the outputs of both.  The helper streams
    // and their events are made by gnsscorr_create and live as long as the context; the structs hold no handle and are
    // replaced whole per channel set.
    GcStream stream_plan;                          // planner: the sequential chain (and the direct discovery)
    GcStream stream_tables;                        // a batch's table kernels (expand, ring check, edges), beside the previous correlator
    GcStream stream_discover;                      // discovery of the next batch's claims, beside the chain
    GcEvent ev_plan[2];                            // per plan slot: plan finished (planner stream)
    GcEvent ev_tab[2];                             // the slot's tables are built (tables stream): the correlator may read them
    GcEvent ev_used[2];                            // the main stream is done with what the slot held before: the planner may write it
    GcEvent ev_corr[2];                            // correlator finished (main stream): the slot's tables are consumed
    GcEvent ev_spec;                               // the claims made ahead are ready, and the tables that read the plan entries their chain rewrites are done (discovery stream)
    GcTrkStateBuf state;
    GcBatch batch;
    GcTrkOut out;
    GcLoop loop;
    GcEvent ev_burst[GC_LOOP_AHEAD];               // gc_trk_run_loop: the ends of the launch bursts in flight
    GcRx rx;
    GcEvent ev_lock;                               // end of the last lock monitor launch (made on first use)
    bool lock_pending = false;                     // ev_lock is recorded and rx.lock_lost not read yet
    GcNav nav;

    // FFT tables (context lifetime); acquisition and the IF monitor (replaced whole per channel set, acquisition also
    // per coherent setting)
    GcFftTables fft;
    GcAcq acq;
    GcSpec spec;

    // FEC (gnsscorr_fec.hip): staging of gnsscorr_fec_run's symbol streams and packed rows
    GcDevBuf<signed char> dfec_sym;                // [nch][nsym]
    GcDevBuf<unsigned char> dfec_out;              // [nch][npos][rowbytes]
    int fec_parts = 3;                             // (tools) 3: the decoder; 1 / 2: forward pass / chainback alone

    // staging of gnsscorr_{lock,bsync,cfm}_run's host arrays (gc_stage_run, gnsscorr_stage.h)
    GcDevBuf<unsigned char> dstage;

    // timing
    int timing = 0;                                // 0: off, 1: every kernel, 2: only the two correlator kernels (trk_corr, acq_corr)
    std::map<std::string, GcTimer> timers;

    // gnsscorr_debug_poison: byte (0..255) every lazily allocated device buffer is filled with before first use, -1 off
    int poison = -1;
};

// RAII helper: brackets one kernel launch with HIP events when timing is on.
struct GcTimed {
    gnsscorr_ctx *ctx;
    GcEvent a, b;
    const char *name;
    hipStream_t st;
    GcTimed(gnsscorr_ctx *c, const char *n, hipStream_t s = nullptr) : ctx(c), name(n), st(s ? s : c->stream)
    {
        if (!ctx->timing) return;
        if (ctx->timing == 2 && strcmp(n, "trk_corr") != 0 && strcmp(n, "acq_corr") != 0) return;
        if (a.make(hipEventDefault) || b.make(hipEventDefault)) { a.reset(); return; }     // (timing-enabled events)
        hipEventRecord(a, st);
    }
    ~GcTimed()
    {
        if (!a) return;
        hipEventRecord(b, st);
        ctx->timers[name].pending.emplace_back(std::move(a), std::move(b));
    }
};

// The per-channel setters and getters take a channel range [ch0, ch0 + nch) and an array of nch values: EINVAL unless
// both are there and the range lies inside the channel set (compared without forming ch0 + nch, which can overflow)
static inline int gc_chan_range(const char *fn, const gnsscorr_ctx *ctx, int ch0, int nch, const void *values)
{
    if (!ctx || !values || ch0 < 0 || nch <= 0 || ch0 > ctx->nch - nch)
        return gc_fail(GNSSCORR_EINVAL, "%s: channel range [%d,%d) of %d", fn, ch0, (int)((unsigned)ch0 + nch), ctx ? ctx->nch : 0);
    return GNSSCORR_OK;
}

// gnsscorr_trk.hip.  gc_drain: the planner, tables, discovery and main streams are idle afterwards.  gc_quiesce: that
// (and the ingest stream when `ingest`), then drops the look-ahead plan and marks the state touched
int gc_drain(gnsscorr_ctx *ctx);
int gc_quiesce(gnsscorr_ctx *ctx, bool ingest = false);
// the outputs of a run of nperiod periods per channel; a fetch's counters
int gc_ensure_trk_outputs(gnsscorr_ctx *ctx, int nperiod);
int gc_nco_check(gnsscorr_ctx *ctx);
// gnsscorr_acq.hip: makes ctx->fft on first use (tables, and the dynamic LDS sizes of the kernels that read them)
int gc_acq_twiddles(gnsscorr_ctx *ctx);
int gc_ingest_fence(gnsscorr_ctx *ctx);      // orders the compute stream behind the last ring transfer
// both rings' write positions and the ingest fence together, under the lock (a grabber thread may be pushing): the
// positions cover only samples whose transfer the compute stream is ordered behind
int gc_ring_positions(gnsscorr_ctx *ctx, uint64_t wp_ring[2]);
// the closed loop takes the tracking state: quiesces if the batched interface has a look-ahead plan or a batch in flight;
// either way no plan is valid afterwards and the state is marked touched (the batched tracker plans afresh)
int gc_loop_take_state(gnsscorr_ctx *ctx);
// gnsscorr_acq.hip: one search over a channel list; the device hand-over of its acquired channels into the closed loop
int gc_acq_run_list(gnsscorr_ctx *ctx, const uint64_t wp_ring[2], const int *chlist, int n);
int gc_acq_handover(gnsscorr_ctx *ctx, bool quiesce);
// the code-Doppler shifts s(b, g) of a channel ([bin][iter], stride groups) and its look-back `back`; EINVAL for a shift
// beyond a code period.  A channel without compensation has zeros
int gc_acq_shifts(const gnsscorr_ctx *ctx, int ch, std::vector<int32_t> &s, int *back);
// gnsscorr_loop.hip: gnsscorr_trk_run_loop with per-channel write positions
int gc_trk_run_loop(gnsscorr_ctx *ctx, int nperiod, const uint64_t *wp_ch);
// gnsscorr_lock.hip: the lock monitor over the periods the last gc_trk_run_loop tracked, for the TRACK channels that have
// it on; queues the launch and its event on the context's stream and does not wait
int gc_rx_lock_launch(gnsscorr_ctx *ctx, int nperiod);
// gnsscorr_bsync.hip: the bit-synchronisation detector over the same periods, for the TRACK channels that have it on;
// queues the launch on the context's stream and does not wait
int gc_rx_bsync_launch(gnsscorr_ctx *ctx, int nperiod);
// gnsscorr_cfm.hip: the correlation monitor over the same periods, for the TRACK channels that have it on; queues the
// launch on the context's stream, waits for nothing and records no event
int gc_rx_cfm_launch(gnsscorr_ctx *ctx, int nperiod);
