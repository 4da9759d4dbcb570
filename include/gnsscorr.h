/*
 * gnsscorr.h -- C ABI of libgnsscorr.so, the MI355X (gfx950) correlation
 * engine behind GNSS-SDRLIB's acquisition / tracking entry points.
 *
 * Two layers are exported:
 *
 *  1. The reference's own symbols (sdracquisition, sdrtracking, correlator,
 *     pcorrelator, checkacquisition, ... : see sdr_compat.h).  They keep the
 *     reference signatures and operate on the reference's sdrch_t, one channel
 *     and one code period per call, exactly like src/sdracq.c / src/sdrtrk.c.
 *
 *  2. The batched, device-resident interface below.  It is what the per-call
 *     symbols are built on and what a scheduler that wants throughput calls:
 *     the IF sample ring lives in HBM, every channel of an epoch batch runs in
 *     one launch, and results stay on the device until fetched.
 *
 * Plain C types only: no HIP or torch types appear in any signature; device
 * pointers and streams cross as void*.
 *
 * Each entry point cites the reference interface it replaces as
 * "ref <file>:<line>" (paths relative to the reference root).
 *
 * All functions return 0 on success and a negative GNSSCORR_E* code on
 * failure; gnsscorr_last_error() gives the message.  Like the reference
 * (src/sdrcmn.c:697-702) a failing call leaves its outputs untouched.
 */
#ifndef GNSSCORR_H
#define GNSSCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNSSCORR_OK         0
#define GNSSCORR_EINVAL    -1   /* bad argument / unsupported shape          */
#define GNSSCORR_EHIP      -2   /* HIP runtime error (no device, OOM, ...)   */
#define GNSSCORR_ESTATE    -3   /* call order (no ring, no channels, ...)    */
#define GNSSCORR_ENOMEM    -4   /* host memory (gnsscorr_sync_* only)        */

#define GNSSCORR_MAXTAPS   33   /* 1 + 2*corrn, corrn <= 16                  */
#define GNSSCORR_MAXFREQ   1024 /* Doppler bins per channel                  */
#define GNSSCORR_MAXCOH    20   /* code periods summed coherently per group  */

typedef struct gnsscorr_ctx gnsscorr_ctx;

const char *gnsscorr_last_error(void);
int  gnsscorr_device_count(void);

/* One context = one GPU + one HIP stream.  stream == NULL creates a private
 * stream; otherwise `stream` is a hipStream_t owned by the caller. */
int  gnsscorr_create(gnsscorr_ctx **ctx, int device, void *stream);
void gnsscorr_destroy(gnsscorr_ctx *ctx);
void *gnsscorr_stream(gnsscorr_ctx *ctx);
int  gnsscorr_sync(gnsscorr_ctx *ctx);

/* ---- IF sample ring in HBM -------------------------------------------------
 * Replaces sdrstat.buff / buff2 and file_getbuff() (ref src/sdrrcv.c:505-532,
 * ring size ref src/sdr.h:134,137).  Sample index s of front end `ftype`
 * lives at byte dtype*(s % ringlen); the write position is the reference's
 * sdrstat.fendbuffsize*sdrstat.buffcnt.
 * devmem == NULL allocates dtype*ringlen bytes with hipMalloc; otherwise the
 * caller's device buffer is used (e.g. the tensor an RCCL broadcast lands
 * in).  dtype*ringlen must be a multiple of 16.
 * On a context that has channels (a front end switched under a live receiver)
 * the call re-creates the ring under them.  The channels of that ring keep
 * their device rows, which index the ring by the channel's own dtype and
 * nsamp, so the new ring must be one gnsscorr_set_channels would accept for
 * them: GNSSCORR_EINVAL naming the channel, with nothing touched -- the old
 * ring, its write position and its contents (gnsscorr_ring_read) stay -- when
 * a channel with this ftype has another dtype, or ringlen < nsamp + 100 +
 * 32/dtype for it.  To change the dtype, call gnsscorr_set_channels with
 * channels of another ring (or destroy the context) first.  Otherwise the call
 * waits until nothing of the context is in flight (every stream, the ingest
 * included; a look-ahead tracking plan is dropped), the write position becomes
 * 0, an owned ring is zero filled, and the channels read the new ring from the
 * next call on.  Everything else stays: the channel set and its acquisition
 * settings, the prepared acquisition work and the last search's results, the
 * tracking and loop states (their buffloc are positions of the old stream:
 * gnsscorr_trk_set_state or a hand-over from a new search comes next), the
 * IF monitor's last run.  A search needs (intg + 1) * nsamp new samples first
 * (GNSSCORR_ESTATE until then).
 * A running schedule (gnsscorr_rx_start done) holds positions of the old
 * stream in next_try, acq_wrpos and the TRACK channels' buffloc: re-creating a
 * ring that a channel reads switches the schedule off, and gnsscorr_rx_step,
 * gnsscorr_rx_set, gnsscorr_rx_status, gnsscorr_rx_lock_set,
 * gnsscorr_rx_lock_status, gnsscorr_rx_bsync_set, gnsscorr_rx_bsync_status,
 * gnsscorr_rx_cfm_set and gnsscorr_rx_cfm_status
 * return GNSSCORR_ESTATE until the next
 * gnsscorr_rx_start.  A ring no channel reads leaves the schedule alone. */
int  gnsscorr_ring_create(gnsscorr_ctx *ctx, int ftype, int dtype,
                          uint64_t ringlen, void *devmem);
/* append nsamp samples from host memory (what file_pushtomembuf's fread
 * delivers, ref src/sdrrcv.c:469-495) and advance the write position.  A chunk
 * may not exceed the ring; chunks of any size are staged piecewise. */
int  gnsscorr_ring_push(gnsscorr_ctx *ctx, int ftype, const void *host,
                        uint64_t nsamp);
/* The same for a front end's packed byte stream, expanded on the device on its way into the ring(s):
 *   GNSSCORR_FMT_STEREO  NSL Stereo: one byte per sample instant, bits 7-6 = front end 1 (real, {-3,-1,+1,+3}),
 *                        bits 5-3 / 2-0 = front end 2 I / Q ({+1,+3,+5,+7,-7,-5,-3,-1}) -- ref
 *                        src/rcv/stereo/stereo.c:160-205.  Feeds ring 1 (dtype 1) and ring 2 (dtype 2), whichever
 *                        exist, nsamp samples each.
 *   GNSSCORR_FMT_RTLSDR  RTL-SDR: unsigned 8-bit I, Q pairs, (char)(value - 127.5) -- ref
 *                        src/rcv/rtlsdr/rtlsdr.c:136-143.  Feeds ring 1 (dtype 2) from 2*nsamp bytes.
 * Both push calls return as soon as the host buffer may be reused; the transfer runs on a copy stream of
 * the context's own behind pinned staging buffers and never waits for (or stalls) the compute stream --
 * tracking / acquisition calls issued afterwards are ordered behind it. */
#define GNSSCORR_FMT_STEREO 1
#define GNSSCORR_FMT_RTLSDR 2
int  gnsscorr_ring_push_packed(gnsscorr_ctx *ctx, int format, const void *host,
                               uint64_t nsamp);
/* rcvgetbuff() on the HBM ring (ref src/sdrrcv.c:406-463,505-532): n samples from sample index buffloc,
 * wrapped like file_getbuff(); synchronises */
int  gnsscorr_ring_read(gnsscorr_ctx *ctx, int ftype, uint64_t buffloc, int n,
                        void *host);
/* the ring memory was filled by someone else (RCCL, a kernel): advance only */
int  gnsscorr_ring_commit(gnsscorr_ctx *ctx, int ftype, uint64_t nsamp);
uint64_t gnsscorr_ring_wrpos(gnsscorr_ctx *ctx, int ftype);
void *gnsscorr_ring_devptr(gnsscorr_ctx *ctx, int ftype);

/* ---- channels ---------------------------------------------------------------
 * The constants initsdrch() derives (ref src/sdrinit.c:583-657). */
typedef struct {
    int    prn, ctype;
    int    dtype, ftype;        /* ref sdrch_t.dtype / .ftype                */
    int    clen, nsamp, nsampchip;
    double f_sf, f_if, foffset; /* Hz                                        */
    double crate, ctime, ti;
    const short *code;          /* clen chips, +-1 (ref sdrch_t.code)        */
    int    intg;                /* ref sdracq_t.intg                         */
    int    nfreq;               /* ref sdracq_t.nfreq (<= GNSSCORR_MAXFREQ)  */
    const double *freq;         /* ref sdracq_t.freq                         */
    int    nfft;                /* ref sdracq_t.nfft (= 2*nsamp)             */
    int    corrn;               /* ref sdrtrk_t.corrn                        */
    const int *corrp;           /* ref sdrtrk_t.corrp                        */
} gnsscorr_chan_t;

/* Replaces the context's channel set; may be called again on a live context
 * (the satellite list changed).  Validates first (GNSSCORR_EINVAL /
 * GNSSCORR_ESTATE naming the channel, nothing touched), waits until nothing of
 * the context is in flight, and then starts the new set from nothing: tracking
 * and loop states zero, no loop constants (gnsscorr_loop_set), the acquisition
 * settings back at ncoh 1 / estep 0 / nref 0, no search results, the schedule
 * the lock monitor, the bit-synchronisation detector and the correlation
 * monitor off (GNSSCORR_ESTATE until gnsscorr_rx_start, and then off for every
 * channel until gnsscorr_rx_lock_set / _bsync_set / _cfm_set), and the
 * IF monitor's last run gone: gnsscorr_spec_fetch returns GNSSCORR_ESTATE
 * until the next gnsscorr_spec_run.  The rings, their contents and write
 * positions stay.  A new set computes bit for bit what it computes on a fresh
 * context over the same ring contents. */
int  gnsscorr_set_channels(gnsscorr_ctx *ctx, int nch,
                           const gnsscorr_chan_t *ch);
int  gnsscorr_num_channels(gnsscorr_ctx *ctx);

/* ---- tracking: E/P/L correlators + carrier wipe-off ------------------------
 * One (channel, epoch) unit is one call of the reference's correlator()
 * (ref src/sdrcmn.c:687-722) as driven by sdrtracking() (ref
 * src/sdrtrk.c:31-43): currnsamp from remcode/codefreq, carrier phase and
 * code phase continued from the previous epoch. */
typedef struct {
    double   carrfreq, codefreq;    /* ref sdrtrk_t.carrfreq / .codefreq     */
    double   remcode, remcarr;      /* ref sdrtrk_t.remcode / .remcarr       */
    uint64_t buffloc;               /* sample index of the next code period  */
} gnsscorr_trkstate_t;

int  gnsscorr_trk_set_state(gnsscorr_ctx *ctx, int ch0, int nch,
                            const gnsscorr_trkstate_t *st);
int  gnsscorr_trk_get_state(gnsscorr_ctx *ctx, int ch0, int nch,
                            gnsscorr_trkstate_t *st);
/* Correlate `nepoch` consecutive code periods of every channel with the
 * frequencies held (as between two loop-filter updates, ref
 * src/sdrmain.c:272-302).  Asynchronous; advances the device-resident state.
 * The correlator launches go to the context's stream back to back; the
 * planner (next batch) and the conversion of the partial sums into the
 * result arrays run on streams of the context's own.  gnsscorr_sync,
 * gnsscorr_trk_fetch*, gnsscorr_trk_get_state and gnsscorr_trk_devptrs order
 * the caller behind them. */
int  gnsscorr_trk_run(gnsscorr_ctx *ctx, int nepoch);
/* Results of the last gnsscorr_trk_run, [nch][nepoch][1+2*corrn] each, in the
 * reference's tap order {P,E1,L1,E2,L2,...}.  trkII / trkQQ are what
 * sdrtracking() leaves in sdr->trk.II / sdr->trk.QQ (II = sum dataQ*code/32,
 * QQ = sum dataI*code/32: the reference's swapped hand-over, ref
 * src/sdrtrk.c:42).  nsamp_out[nch][nepoch] = currnsamp of each period.
 * Any pointer may be NULL.  Synchronises the stream. */
int  gnsscorr_trk_fetch(gnsscorr_ctx *ctx, double *trkII, double *trkQQ,
                        int *nsamp_out);
/* cumsumcorr() over the epochs of the last run (ref src/sdrtrk.c:64-76):
 * sumI/sumQ [nch][1+2*corrn] */
int  gnsscorr_trk_fetch_sums(gnsscorr_ctx *ctx, double *sumI, double *sumQ);
/* device pointers to the result arrays of the last run (layout as fetch);
 * work queued on the context's stream after this call sees the results of
 * every gnsscorr_trk_run issued before it */
int  gnsscorr_trk_devptrs(gnsscorr_ctx *ctx, void **trkII, void **trkQQ);

/* ---- tracking, closed loop: cumsumcorr() + pll() + dll() on the device -------
 * What sdrthread() does around sdrtracking() every code period (ref
 * src/sdrmain.c:264-312): accumulate the correlator outputs (ref
 * src/sdrtrk.c:64-76), run the loop filters -- every period with prm1 until the
 * nav bit is synchronised, then whenever checkbit() raises swloop (every loopms
 * periods counted from the bit edge, ref src/sdrnav.c:241-262) with prm2 -- and
 * clear the sums after each filter update.  Bit synchronisation (checksync(),
 * ref src/sdrnav.c:198-233) and the bit decisions of checkbit() run on the
 * device too, so a channel goes acquisition -> loop every period -> flagsync ->
 * loop every loopms periods without the host.  The loop state lives on the
 * device next to the NCO state; a run of N periods needs no host round trip:
 * it is a chain of launches -- per filter interval one that closes the interval
 * (sums, nav bit, filters) and plans the next, and one that correlates it. */
typedef struct {
    double acqfreq;                         /* ref sdracq_t.acqfreq                   */
    double f_if, foffset, f_cf, crate, ctime;   /* ref sdrch_t                        */
    double pllaw[2], pllw2[2], fllw[2];     /* ref sdrtrkprm_t of prm1 [0], prm2 [1]  */
    double dllaw[2], dllw2[2];
    int    ne, nl;                          /* ref sdrtrk_t.ne / .nl                  */
    int    loopms;                          /* ref sdrtrk_t.loopms                    */
    int    rate;                            /* ref sdrnav_t.rate                      */
    int    flagsync, synci;                 /* ref sdrnav_t.flagsync / .synci         */
    int    navcnt, swloop;                  /* ref sdrnav_t.cnt / .swloop (checkbit)  */
    uint64_t cnt;                           /* ref sdrthread's cnt: periods tracked   */
    double carrNco, codeNco, carrErr, codeErr, freqErr;     /* ref sdrtrk_t           */
    double II[GNSSCORR_MAXTAPS], QQ[GNSSCORR_MAXTAPS];      /* ref sdrtrk_t (all 8)   */
    double oldI[GNSSCORR_MAXTAPS], oldQ[GNSSCORR_MAXTAPS];
    double sumI[GNSSCORR_MAXTAPS], sumQ[GNSSCORR_MAXTAPS];
    double oldsumI[GNSSCORR_MAXTAPS], oldsumQ[GNSSCORR_MAXTAPS];
    /* navigation bit synchronisation: the part of sdrnavigation() that schedules the loops (ref
     * src/sdrnav.c:18-36: biti, checksync() :198-233, checkbit() :241-282), run on the device after
     * every period's correlator like the reference does from sdrtracking() (ref src/sdrtrk.c:46) */
    int    prn;                             /* ref sdrnav_t.sdreph.prn (= the channel's PRN, src/sdrinit.c:506):
                                               checksync() takes its sign shift-register branch for prn > 5 (:203) */
    int    biti;                            /* ref sdrnav_t.biti                      */
    int    bit;                             /* ref sdrnav_t.bit: last decided bit, +-1 */
    int    swsync, swreset;                 /* ref sdrnav_t.swsync / .swreset         */
    int    flagpol;                         /* ref sdrnav_t.flagpol (the frame decoder's; 0 unless the caller sets it) */
    double bitIP;                           /* ref sdrnav_t.bitIP                     */
    int    bitsync[20];                     /* ref sdrnav_t.bitsync[rate], rate <= 20 */
} gnsscorr_loop_t;

int  gnsscorr_loop_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_loop_t *lp);
int  gnsscorr_loop_get(gnsscorr_ctx *ctx, int ch0, int nch, gnsscorr_loop_t *lp);

/* One row per code period, the columns writelog() prints (ref src/sdrout.c:412-437) */
typedef struct {
    double carrfreq, codefreq;              /* after this period's filter update      */
    double carrErr, codeErr, carrNco, codeNco, freqErr;
    double remcode, remcarr;                /* after this period                      */
    uint64_t buffloc;                       /* first sample of this period            */
    int    currnsamp;
    int    flagloopfilter;                  /* 0 none, 1 prm1, 2 prm2                 */
    int    flagsync;                        /* ref sdrnav_t.flagsync after this period */
    int    navbit;                          /* +-1: checkbit() decided a bit in this period (swsync), else 0 */
} gnsscorr_trklog_t;

/* Observables on the batched outputs: setobsdata() (ref src/sdrtrk.c:160-209) replayed over the log of a closed-loop
 * run.  The reference calls it from sdrthread() after every prm2 filter update (ref src/sdrmain.c:279-288) with
 * snrflag every SNSMOOTHMS = 100 ms; everything it reads is in the log row of that period, the row before it
 * (oldremcode) and the prompt sums of the interval (sumI[0] before clearcumsumcorr).  Plain host code, no device.
 * State carried from call to call (a channel's log may be replayed in pieces): */
typedef struct {
    /* constants of the channel: ref sdrch_t.f_sf / .f_if / .foffset / .ctime, sdrtrk_t.loopms */
    double f_sf, f_if, foffset, ctime;
    int    loopms;
    /* from the frame decoder (ref sdrnav_t.flagsyncf / .polarity / .firstsftow / .firstsfcnt); zero until it sets them */
    int    flagsyncf, polarity;
    double firstsftow;
    uint64_t firstsfcnt;
    /* running state: ref sdrtrk_t.L[0] / .Isum / .flagremcarradd / .flagpolarityadd, sdrthread's loopcnt, the
     * interval's sumI[0] so far, the remcode of the period before the next one (sdrtrk_t.oldremcode) */
    double L, Isum, sumI0, oldremcode;
    int    flagremcarradd, flagpolarityadd;
    uint64_t loopcnt;
} gnsscorr_obs_t;
/* one row per call of setobsdata(): element [0] of sdrtrk_t.tow / codei / cntout / remcout / L / D after it,
 * and S / codeisum when the call computed them (snr != 0) */
typedef struct {
    double tow, remcout, L, D, S;
    uint64_t codei, cntout;
    int    snr, pad;
} gnsscorr_obsrow_t;
/* log[nper]: rows of one channel (gnsscorr_trk_fetch_log); II0[nper]: that channel's sdrtrk_t.II[0] per period
 * (gnsscorr_trk_fetch's II, tap 0); cnt0: sdrthread's cnt at log[0].  Writes at most max_out rows, returns their
 * number (or GNSSCORR_EINVAL). */
int  gnsscorr_obs_replay(gnsscorr_obs_t *st, const gnsscorr_trklog_t *log, const double *II0, int nper, uint64_t cnt0,
                         gnsscorr_obsrow_t *out, int max_out);

/* Frame synchronisation on the batched nav bits (GPS / QZSS L1 C/A): what sdrnavigation() does behind checkbit()
 * (ref src/sdrnav.c:41-82) -- the last 302 decided bits, the preamble search with its parity check over the ten words
 * (ref :373-411, :325-346, src/sdrnav_gps.c:141-164), and of the subframe decoder the subframe number and the time of
 * week in the hand-over word (ref src/sdrnav_gps.c:123-135,170-190) -- replayed over the `navbit` column of a
 * closed-loop log.  It yields what setobsdata() needs from the frame decoder: flagsyncf, polarity, firstsfcnt,
 * firstsftow.  Ephemeris decoding is not part of this library.  Plain host code. */
typedef struct {
    int    fbits[302];                      /* ref sdrnav_t.fbits (flen 300 + addflen 2), newest last     */
    int    polarity, flagsyncf, flagtow, flagdec;   /* ref sdrnav_t                                        */
    int    sfid;                            /* subframe number decoded last (1..5; other: not a subframe) */
    int    pad;
    uint64_t firstsf, firstsfcnt;           /* ref sdrnav_t: sample / period counter of the frame's end   */
    double firstsftow, tow_gpst;            /* ref sdrnav_t.firstsftow, sdreph_t.tow_gpst                 */
} gnsscorr_frame_t;
/* log[nper]: one channel's rows; cnt0: sdrthread's cnt at log[0].  Returns 0, or GNSSCORR_EINVAL.  This is the L1 C/A
 * path: the state carries no code type, and the symbols of a GLONASS G1 channel belong to gnsscorr_g1frame_replay. */
int  gnsscorr_frame_replay(gnsscorr_frame_t *st, const gnsscorr_trklog_t *log, int nper, uint64_t cnt0);

/* Frame synchronisation of GLONASS G1 on the batched symbols: what sdrnavigation() does behind checkbit() for CTYPE_G1
 * (ref src/sdrnav.c:40-82) -- the last 200 decided symbols (ref src/sdrinit.c:546-558), no FEC (ref src/sdrnav.c:296-299),
 * the search for the 30-symbol time mark that ends a string (ref :391-408, src/sdrinit.c:494-496; the parity check
 * passes every string, ref src/sdrnav.c:361-364), and every 2000 periods from the mark on decode_g1() (ref
 * src/sdrnav_glo.c:199-224: meander and relative code removed, 85 bits packed) with the fields of strings 1, 2, 4 and 5
 * that give the time (ref :26-37, :44-59, :82-107) and merge_g1()'s week and time of week (ref :118-165) -- replayed
 * over the `navbit` column of a closed-loop log.  It yields what setobsdata() needs from the frame decoder: flagsyncf,
 * polarity, firstsfcnt, firstsftow.  DESIGN.md section 3.6 states the semantics and the reference's quirks that are
 * kept.  The Hamming check bits are not read (nor does the reference); ephemeris and almanac contents are not part of
 * this library: `str` is there for a caller's decoder.  Plain host code without the device: csrc/sdr_g1.c links alone.
 * The time is merged whenever ephcnt is exactly 5 after a string (ref src/sdrnav_glo.c:190); the reference's syncthread
 * sets the counter back to 0 once it has taken the ephemeris (ref src/sdrsync.c:138-141).  Here that is the caller's
 * job: set ephcnt = 0 between two calls to let the next five strings merge again.
 * `slot` is what the reference copies into sdr->prn at flagdec (ref src/sdrnav.c:78-79); it is never written to the
 * device. */
typedef struct {
    int    fbits[200];                      /* ref sdrnav_t.fbits (flen 200, addflen 0), newest last; 0: not filled */
    int    polarity, flagsyncf, flagtow, flagdec;   /* ref sdrnav_t                                               */
    int    id;                              /* string number decoded last (bits 1..4 of the string)                */
    int    ephcnt, s1cnt;                   /* ref sdreph_t.cnt / .s1cnt                                           */
    int    tk[3];                           /* string 1: hours - 3, minutes, seconds (ref sdreph_t.tk)             */
    int    nt, slot, n4;                    /* string 4: day number, slot number; string 5: 4-year interval        */
    int    iode, update;                    /* string 2: ref geph_t.iode, sdreph_t.update (ref src/sdrnav_glo.c:46-55) */
    int    week;                            /* ref sdreph_t.week_gpst                                              */
    unsigned char str[11];                  /* the 85 bits of the string decoded last, as decode_g1() packs them   */
    unsigned char pad[5];
    uint64_t firstsf, firstsfcnt;           /* ref sdrnav_t: sample / period counter of the time mark's last symbol */
    double firstsftow, tow_gpst;            /* ref sdrnav_t.firstsftow, sdreph_t.tow_gpst: GPS time of the string's end */
} gnsscorr_g1frame_t;
/* log[nper]: one channel's rows; cnt0: sdrthread's cnt at log[0].  The caller zero-initialises st; a log may be replayed
 * in pieces of any length.  Returns 0, or GNSSCORR_EINVAL (a NULL pointer, nper < 0) with nothing touched. */
int  gnsscorr_g1frame_replay(gnsscorr_g1frame_t *st, const gnsscorr_trklog_t *log, int nper, uint64_t cnt0);

/* ---- observation epochs: pseudorange, carrier phase and Doppler across channels ----
 * The body of syncthread()'s loop (ref src/sdrsync.c:49-121, with interp1() and uint64todouble(), ref
 * src/sdrcmn.c:505-565) replayed over the rows gnsscorr_obs_replay gives each channel: one pseudorange per satellite at
 * a common epoch, carrier phase and Doppler interpolated to that epoch.  The RINEX / RTCM writers behind it are not part
 * of this library.  Plain host code without the device: csrc/sdr_sync.c links alone.  DESIGN.md section 3.8 states the
 * semantics in full, the reference's quirks that are kept (lettered (a)..(e) there) and the one conversion C leaves
 * undefined.
 *
 * History.  Per channel tow, codei, cntout, remcout, L, D hold GNSSCORR_OBSHIST elements, zero at creation, and S0 = 0.
 * Consuming a row shifts them by one and puts the row at [0], as setobsdata() does (ref src/sdrtrk.c:163-173); a row with
 * snr != 0 also sets S0 = S.
 *
 * Order of consumption.  The reference polls while the channel threads append rows in real time; here pushed rows wait
 * in a queue per channel, and the waiting row with the smallest codei (the lower channel on ties) is consumed as soon as
 * every attached channel has a row waiting.  gnsscorr_sync_channel attaches a channel; gnsscorr_sync_detach drops its
 * queue, zeroes its history and its eligibility and stops it from holding the others back; it attaches again with its
 * next push.  Detach a channel that leaves TRACK or that will deliver nothing for a while.  So what is consumed, and
 * every epoch, depends neither on how a channel's rows are cut into pushes nor on the order of pushes between channels.
 * The frame fields given with a push belong to every row of that push.  codei values are sample indices of one stream
 * origin and rate, as in the reference, whose two Stereo rings run at one rate.
 *
 * Poll.  After every consumed row one pass of ref src/sdrsync.c:53-121 runs over the histories.  Eligible are the
 * channels whose last consumed row had flagdec && week != 0 && cntout >= firstsfcnt, in channel order.  reftow is the
 * smallest tow[0] among them, starting from 3600*24*7.  No epoch when none is eligible, when reftow equals the pass
 * before's, when (int)(reftow*1000) % outms != 0, or when reftow*1000 lies below the range of int.  Otherwise ind (per
 * position in the eligible list, kept from pass to pass, set where a history element lies within 1e-4 of reftow), the
 * nearest channel refi (smallest codei[ind]), diffcnt = cntout[ind] - firstsfcnt of refi, sampref = firstsf +
 * nsamp*(-PTIMING/(1000*ctime) + diffcnt) -- the product converted to int64 towards zero (0x8000000000000000 where it
 * does not fit) and added modulo 2^64 --, sampbase = codei[79] - 10*nsamp of refi, samprefd = (double)(sampref -
 * sampbase); and per eligible channel
 *     P = CLIGHT * ti * ((double)(codei[ind] - sampref) - remcout[ind])        metres, CLIGHT = 299792458
 *     L, D = interp1 over (double)(codei[k] - sampbase), k = 0..79, at samprefd
 *     S = S0, week = the channel's, tow = reftow + PTIMING/1000.
 * All differences of sample counts are uint64 and wrap. */
#define GNSSCORR_OBSHIST   80           /* ref OBSINTERPN, src/sdr.h:197 */
#define GNSSCORR_PTIMING   68.802       /* ref PTIMING, ms, src/sdr.h:196 */
#define GNSSCORR_SYNCQCAP  4096         /* rows that may wait per channel */
typedef struct gnsscorr_sync gnsscorr_sync_t;
/* what the frame decoder found (gnsscorr_frame_t / gnsscorr_sbasframe_t / gnsscorr_g1frame_t: flagdec, firstsf,
 * firstsfcnt) and the week: from the caller's ephemeris decoder for L1 C/A, from the state for G1 and SBAS */
typedef struct {
    int    flagdec, week;
    uint64_t firstsf, firstsfcnt;
} gnsscorr_syncframe_t;
typedef struct {
    int    ch, week;
    double tow, P, L, D, S;
    uint64_t sampref;                   /* the sample the epoch's pseudoranges count from */
} gnsscorr_epochobs_t;

/* outms: ref sdrini.outms, the epoch grid in ms.  GNSSCORR_EINVAL: NULL, nch <= 0, outms <= 0.  Any of the calls may
 * answer GNSSCORR_ENOMEM; rows that wait then stay where they are.  One thread at a time per gnsscorr_sync_t. */
int  gnsscorr_sync_create(gnsscorr_sync_t **st, int nch, int outms);
void gnsscorr_sync_destroy(gnsscorr_sync_t *st);
/* The constants of channel ch (ref sdrch_t.nsamp / .ctime / .ti); empties and attaches it.  GNSSCORR_EINVAL, nothing
 * touched: NULL, ch out of range, a value that is not positive and finite, a ti that differs from another channel's. */
int  gnsscorr_sync_channel(gnsscorr_sync_t *st, int ch, int nsamp, double ctime, double ti);
/* rows[n] of channel ch, in order, with the frame fields that hold for them; consumes what can be consumed.
 * GNSSCORR_EINVAL, nothing touched: NULL, ch out of range, a push before gnsscorr_sync_channel, a row whose codei is
 * not above the channel's last (since it was last emptied).  GNSSCORR_ESTATE, nothing touched: more than
 * GNSSCORR_SYNCQCAP rows would wait; the message names the channel that holds the others back. */
int  gnsscorr_sync_push(gnsscorr_sync_t *st, int ch, const gnsscorr_syncframe_t *fr, const gnsscorr_obsrow_t *rows, int n);
int  gnsscorr_sync_detach(gnsscorr_sync_t *st, int ch);
/* consumes every row that waits, in the same order, whether or not every attached channel has one */
int  gnsscorr_sync_flush(gnsscorr_sync_t *st);
/* Takes up to max_out rows of the epochs made so far, oldest first, and returns their number: an epoch is nsat
 * consecutive rows with one tow, in channel order. */
int  gnsscorr_sync_fetch(gnsscorr_sync_t *st, gnsscorr_epochobs_t *out, int max_out);
/* the message of the last failed gnsscorr_sync_* call of this thread (csrc/sdr_sync.c links without the rest of the
 * library, so it keeps its own) */
const char *gnsscorr_sync_last_error(void);

/* ---- FEC: sliding-window Viterbi decoder (K = 7, rate 1/2) on the device ------
 * predecodefec() for CTYPE_L1SBAS (ref src/sdrnav.c:302-318): init_viterbi27(.., 0), update_blk over win/2 symbol
 * pairs, chainback(.., ndec, end state 0), for npos windows of every channel in one launch (one wavefront per window).
 * sym[nch][nsym] holds each channel's decided symbols (+1, -1, or 0 for history not filled yet); window p of a channel
 * is the win symbols that end at symbol pos0 + p*stride, symbols in front of the stream counting as 0.  +1 is received
 * as 0, anything else as 255 (ref :305-306).  polyA, polyB: the generator masks over the register (the last seven
 * input bits, newest in bit 0), first and second symbol of a pair: libfec's V27POLYA, V27POLYB = 0x6d, 0x4f (ref
 * src/sdrinit.c:502,539).  The decoder is defined in DESIGN.md 3.5; it walks back from state 0 whatever the metrics
 * say, so the last six steps are read as a tail.
 * out[nch][npos][rowbytes]: the ndec decoded bits of each window, packed MSB first (a set bit is fbitsdec = -1, ref
 * :311-312), the rest of the row zero; rowbytes >= (ndec + 7)/8 (96 for the reference's 750 bits).
 * win even and <= 1512, ndec <= win/2 - 6, no negative count, the last window inside the stream: otherwise
 * GNSSCORR_EINVAL.  Runs on the context's stream and synchronises it; timer name "fec_viterbi27". */
int  gnsscorr_fec_run(gnsscorr_ctx *ctx, const signed char *sym, int nch, int nsym, int pos0, int npos, int stride,
                      int win, int ndec, int polyA, int polyB, unsigned char *out, int rowbytes);

/* Frame synchronisation of SBAS L1 on the batched symbols: what sdrnavigation() does behind checkbit() for
 * CTYPE_L1SBAS (ref src/sdrnav.c:40-82) -- the last 1512 decided symbols, predecodefec() on every symbol until the frame
 * is found and every 1000 periods from then on (ref src/sdrinit.c:530), the two-preamble search on the decoded bits (ref
 * src/sdrnav.c:384-389) with its CRC-24Q check (ref :351-359), and of decode_l1sbas() the CRC verdict's message, its type
 * and the time of message type 12 (ref src/sdrnav_sbs.c:69-73,100-140) -- replayed over the `navbit` column of a
 * closed-loop log.  It yields what setobsdata() needs from the frame decoder: flagsyncf, polarity, firstsfcnt,
 * firstsftow.  The Viterbi decodes run on the device (gnsscorr_fec_run, all candidate positions of the call in one
 * launch); the walk over the decoded rows is host code.
 * flagpol: a matched preamble of polarity +1 whose CRC fails sets it (ref src/sdrnav.c:404-406), and in the reference it
 * then flips every symbol checkbit() decides (ref :266-271).  The log's symbols were decided with the device's flagpol
 * as it was when the run began, so the replay keeps its own: once it is on, the log's later symbols are multiplied by
 * -1 (and the rows behind that symbol decoded again).  It is never written to the device and never goes off.
 * The NovAtel message, the TCP output and the correction / ephemeris contents are not part of this library. */
typedef struct {
    int    fbits[1512];                     /* ref sdrnav_t.fbits (flen 1500 + addflen 12), newest last; 0: not filled */
    int    polarity, flagsyncf, flagtow, flagdec, flagpol;  /* ref sdrnav_t                                        */
    int    id;                              /* ref sdrsbas_t.id: message type decoded last                         */
    int    week;                            /* ref sdrsbas_t.week (= sdreph_t.week_gpst once it is not 0)          */
    int    pad;
    uint64_t firstsf, firstsfcnt;           /* ref sdrnav_t: sample / period counter of the symbol that found it   */
    double firstsftow, tow_gpst;            /* ref sdrnav_t.firstsftow, sdreph_t.tow_gpst                          */
    double tow;                             /* ref sdrsbas_t.tow: type 12's time, else + 1.0 per message            */
    unsigned char msg[32];                  /* ref sdrsbas_t.msg: the 250 bits of the message decoded last         */
} gnsscorr_sbasframe_t;
/* log[nper]: one channel's rows; cnt0: sdrthread's cnt at log[0].  aid_tow[nper] / aid_week: the reference borrows
 * time from the last-but-one channel once that has a week (ref src/sdrnav_sbs.c:123-127): that channel's tow[0] per
 * period of this log (e.g. from gnsscorr_obs_replay) and its week; NULL / 0: no aid.  While week stays 0, tow_gpst
 * stays 0 and the frame flags reset after every decode, as ref src/sdrnav.c:69-72 does.
 * Returns 0, GNSSCORR_EINVAL, or gnsscorr_fec_run's error (there is no CPU path). */
int  gnsscorr_sbasframe_replay(gnsscorr_ctx *ctx, gnsscorr_sbasframe_t *st, const gnsscorr_trklog_t *log, int nper,
                               uint64_t cnt0, const double *aid_tow, int aid_week);

/* Track `nperiod` code periods of every channel closed loop.  A channel stops early
 * where sdrtracking() would find no data yet (ref src/sdrtrk.c:26-30: bufflocnow
 * <= buffloc).  Returns when the last launches are queued (it keeps at most a few
 * filter intervals of launches ahead of the device); results by gnsscorr_trk_fetch
 * (II/QQ per period, periods not run are zero with nsamp_out 0) and
 * gnsscorr_trk_fetch_log.  A period that starts more than ringlen samples behind
 * the write position reads samples the writer has overwritten since: it is run,
 * as sdrtracking() runs it, and counted (gnsscorr_trk_loop_lapped).  Every tap set
 * gnsscorr_set_channels accepts is served, outermost taps of 64 samples included,
 * at any sample rate: no run depends on a channel's code phase for that. */
int  gnsscorr_trk_run_loop(gnsscorr_ctx *ctx, int nperiod);
/* *nlapped = periods of the last gnsscorr_trk_run_loop that read overwritten
 * samples (0: every period read what the ring holds); synchronises */
int  gnsscorr_trk_loop_lapped(gnsscorr_ctx *ctx, int *nlapped);
/* log[nch][nperiod] of the last gnsscorr_trk_run_loop; ndone[nch] = periods run */
int  gnsscorr_trk_fetch_log(gnsscorr_ctx *ctx, gnsscorr_trklog_t *log, int *ndone);
/* Tap 0 of gnsscorr_trk_fetch's II / QQ alone, [nch][nperiod] of the last run of either kind, bit for bit; either
 * pointer may be NULL.  The prompt column is gathered on the device (kernel "trk_prompt") into a compact buffer, so the
 * call moves nch*nperiod doubles per array where gnsscorr_trk_fetch moves nch*nperiod*ntap.  Synchronises the stream
 * and reports what gnsscorr_trk_fetch reports. */
int  gnsscorr_trk_fetch_prompt(gnsscorr_ctx *ctx, double *II0, double *QQ0);

/* ---- acquisition: parallel code phase search --------------------------------
 * For every channel: up to `intg` iterations of pcorrelator() (ref
 * src/sdrcmn.c:738-773) over the channel's Doppler grid, accumulated
 * non-coherently, with checkacquisition() (ref src/sdracq.c:71-95) evaluated
 * after each iteration, as sdracquisition() does (ref src/sdracq.c:24-43). */
typedef struct {
    int      acqcodei, freqi;       /* ref sdracq_t                           */
    double   acqfreq, cn0, peakr;
    int      flagacq;               /* ref sdrch_t.flagacq                    */
    int      iters;                 /* iterations the reference would run (code periods consumed) */
    uint64_t buffloc;               /* return value of sdracquisition()       */
} gnsscorr_acqres_t;

/* wrpos == 0: use each ring's current write position.  Asynchronous. */
int  gnsscorr_acq_run(gnsscorr_ctx *ctx, uint64_t wrpos);
/* The same search for the n distinct channels chlist[0..n) only: the per-channel kernels run over that list (their
 * grids follow n), the shared forward transforms only for the frequency grids that have a listed channel.  A listed
 * channel's result is bit for bit what gnsscorr_acq_run at the same write position gives it; the other channels'
 * rows of the result array are zero (flagacq = 0, iters = 0), so gnsscorr_trk_start_from_acq touches none of them.
 * gnsscorr_acq_run is the list of all channels. */
int  gnsscorr_acq_run_subset(gnsscorr_ctx *ctx, uint64_t wrpos, const int *chlist, int n);
int  gnsscorr_acq_fetch(gnsscorr_ctx *ctx, gnsscorr_acqres_t *res);
/* Device-side hand-over of the last gnsscorr_acq_run to tracking: every acquired
 * channel gets the state sdracquisition() leaves behind (ref src/sdracq.c:51-55:
 * carrfreq = acqfreq, codefreq = crate, remcode = remcarr = 0, buffloc = the
 * returned sample index); channels not acquired keep theirs.  Asynchronous. */
int  gnsscorr_trk_start_from_acq(gnsscorr_ctx *ctx);
/* The same hand-over into the closed loop, on the device: every channel the last search listed and acquired gets that
 * tracking state and the loop state sdrthread() starts tracking with -- acqfreq from the search, every running field
 * as inittrkstruct() / initnavstruct() leave it (ref src/sdrinit.c:432-480,485-560) with cnt = 0, the constants set by
 * gnsscorr_loop_set kept (filter coefficients, ne / nl, loopms, rate, prn, f_if ... ctime).  Other channels keep
 * their tracking and loop state.  Asynchronous. */
int  gnsscorr_loop_start_from_acq(gnsscorr_ctx *ctx);
/* The reference's `power` array for one channel: nfreq*nsamp doubles,
 * accumulated over res.iters iterations (re-runs the search for that channel
 * with the iteration count of the last gnsscorr_acq_run).  A channel the last
 * search did not list: GNSSCORR_ESTATE. */
int  gnsscorr_acq_power(gnsscorr_ctx *ctx, int ch, double *power);
/* Coherent integration over several code periods (opt-in; not in the reference, whose sdracquisition() the drop-in
 * symbol keeps).  Channel ch0 + i integrates ncoh[i] code periods coherently per group and adds its intg / ncoh[i]
 * groups non-coherently: group g covers the (ncoh + 1) * nsamp samples from b0 + g * ncoh * nsamp on (b0 = wrpos -
 * (intg + 1) * nsamp, the look-back of the search is unchanged), is wiped off by one mixcarr() call per Doppler bin
 * with phase 0 at its first sample, and the ncoh windows of 2 * nsamp wiped-off samples that start nsamp apart are
 * added as integers before the forward transform -- which, the transforms being linear, is the coherent sum of their
 * ncoh correlation results.  Everything after the forward transform runs once per group as it runs once per iteration
 * without this call, checkacquisition()'s rules included; the first passing group wins.  In the result iters =
 * (g + 1) * ncoh (intg when not acquired), buffloc is what it is without this call, and cn0 = 10 log10(maxP / meanP /
 * (ncoh * ctime)), the noise bandwidth of a group being 1 / (ncoh * ctime).  ncoh = 1 is the reference's integration,
 * bit for bit.
 * Takes effect after gnsscorr_set_channels, which resets every channel to 1.  GNSSCORR_EINVAL, nothing touched: a
 * channel range outside the table, ncoh < 1, ncoh > GNSSCORR_MAXCOH, intg % ncoh != 0.  Quiesces and drops the
 * prepared acquisition work, so that the next search prepares again; channels share forward spectra only when their
 * ncoh agree as well.
 * Recommended Doppler grid: step <= 1 / (2 * ncoh * ctime) (500 / 100 / 50 Hz for 1 / 5 / 10 periods of 1 ms).  A data
 * bit edge inside a group costs correlation: gnsscorr_acq_set_bitedge (below) searches over its position; without it
 * keep ncoh * ctime <= 10 ms for L1 C/A unless the data is known, and a retry (the receiver schedule's) lands on
 * another alignment.  This call resets the bit-edge step of the channels it names to 0 (the hypotheses depend on
 * ncoh): call it first, gnsscorr_acq_set_bitedge second. */
int  gnsscorr_acq_set_coherent(gnsscorr_ctx *ctx, int ch0, int nch, const int *ncoh);
int  gnsscorr_acq_get_coherent(gnsscorr_ctx *ctx, int ch0, int nch, int *ncoh);
/* Bit-edge hypotheses for coherent groups (opt-in per channel).  Channel ch0 + i, which must have
 * ncoh >= 2, gets the edge step estep[i], 1 <= estep < ncoh; 0 switches the hypotheses off and is the default (and what
 * gnsscorr_set_channels and gnsscorr_acq_set_coherent reset to).  Its hypotheses are h = 0, estep, 2 * estep, ... < ncoh,
 * H of them.  Everything not named here is the coherent search above, unchanged:
 *   - per hypothesis h the group's windows are summed with signs, z_h[k] = sum_{j < ncoh} s(h, j) (I, Q)[j * nsamp + k],
 *     s(h, j) = -1 when h > 0 and j >= h, +1 otherwise (exact integers below 2^24; h = 0 is the sum without this call),
 *     and go through the forward transform, the product with the code spectrum, the inverse transform and
 *     pw_h[k] = |y_h[k]|^2 / L^2 as before;
 *   - per (group, Doppler bin) the hypothesis h* with the largest max_{k < nsamp} pw_h[k] is chosen, the lowest h on
 *     ties, and its whole row is added to the power, P[bin][k] += pw_{h*}[k]; the other hypotheses add nothing;
 *   - row statistics, the early stop and checkacquisition()'s rules run on P after every group as before, and iters,
 *     buffloc, acqfreq and cn0 are what they are above.  A noise row's maximum is the best of H hypotheses while its
 *     mean is that of one, so on noise peakr and cn0 read slightly high (an absent PRN: peakr 1.5 .. 1.9 with ten).
 * The edge of an acquired channel (gnsscorr_acq_fetch_edge) is h* of the deciding group's best row.  For edge > 0 the
 * satellite's data changes sign at sample buffloc + ((iters / ncoh - 1) * ncoh + edge) * nsamp.  The edge is -1 for a
 * channel that was not listed, was not acquired, or has estep = 0.
 * With estep = 0 for every listed channel, results, rows and power arrays are bit for bit those of the search without
 * this call; gnsscorr_acq_power follows the same row rule.
 * One edge per span is assumed and not enforced: exact for L1 C/A up to 20 periods; GLONASS G1 (10 ms meander) wants
 * ncoh <= 10.  The cost is H + 1 inverse transform pairs per (group, bin) instead of one and H forward transforms; the
 * forward spectra take groups * H slots.  Only the 32768-point transform is served, and the transform length is the
 * context's: GNSSCORR_EINVAL when any channel of the context has nsamp > 16384.  Also GNSSCORR_EINVAL, nothing touched
 * and the channel named: a range outside the channel table, estep < 0, estep >= 1 on a channel with ncoh < 2, estep >=
 * ncoh.  Quiesces and drops the prepared acquisition work; channels share forward spectra only when their estep agree
 * as well.  Not included: data wipe-off, a bit-synchronisation preset from the edge; the drop-in sdracquisition() is
 * untouched.  (Code-Doppler compensation: gnsscorr_acq_set_codedoppler, below.) */
int  gnsscorr_acq_set_bitedge(gnsscorr_ctx *ctx, int ch0, int nch, const int *estep);
int  gnsscorr_acq_get_bitedge(gnsscorr_ctx *ctx, int ch0, int nch, int *estep);
/* edge[nch] of the last search (above); synchronises.  GNSSCORR_ESTATE before a search. */
int  gnsscorr_acq_fetch_edge(gnsscorr_ctx *ctx, int *edge);
/* Carrier frequency refinement of acquired channels (opt-in per channel).  A search returns acqfreq as
 * the centre of the best Doppler bin; a channel with nref > 0 that the search lists and acquires also gets a refined
 * frequency, and both hand-overs and the receiver schedule then start tracking from it (carrfreq and the loop's
 * acqfreq).  nref = 0 switches it off, is the default and what gnsscorr_set_channels resets to; otherwise 2 <= nref <=
 * min(intg, GNSSCORR_MAXCOH).  gnsscorr_acqres_t is never touched: results, edges and power arrays are bit for bit what
 * they are without this call, and a channel with nref = 0 is handed over exactly as before.  With n = nsamp, K =
 * GNSSCORR_FINE_BINS and r the channel's result of this search:
 *   1. span: the nref * n ring samples from s0 = r.buffloc on (b0 + acqcodei also with ncoh > 1 and with bit-edge
 *      hypotheses; s0 + nref * n <= wrpos, the samples the search looked back over);
 *   2. carrier wipe-off: one mixcarr() call over the span at r.acqfreq, phase 0 at s0 (ref src/sdrcmn.c:633-669, the
 *      reference's sequential fp64 phase sum): integers (I, Q)[s];
 *   3. code: the replica of the search, c[k] = code[floor(k * ci) mod clen], k < n, ci = ti * crate, the same n values
 *      for every period (code Doppler ignored: at most 0.03 chip over 10 ms);
 *   4. prompt sums P_m = sum_{k < n} c[k] (I + iQ)[m n + k], m < nref: exact integers below 2^28;
 *   5. data removal S_m = P_m^2 (I^2 - Q^2, 2 I Q: exact in int64, then converted to double): the BPSK data, the G1
 *      meander and the SBAS symbols drop out, the residual frequency doubles;
 *   6. line search Z[q] = sum_m S_m exp(+2 pi i ((q m) mod K) / K), q = -K/2 .. K/2 - 1, in fp64; q* is the q with
 *      the largest |Z[q]|^2, the lowest q on ties;
 *   7. finefreq = r.acqfreq + q* / (2 K ctime) (steps of 1.953 Hz at 1 ms), quality = |Z[q*]|^2 / (sum_m |S_m|)^2 in
 *      (0, 1] (1: a clean line; 0 when every prompt sum is zero), nref = the periods used;
 *   8. a channel that was not listed, not acquired or has nref = 0: finefreq = r.acqfreq (0 for the zero row of an
 *      unlisted channel), quality = 0, q = 0, nref = 0, prompt sums zero.
 * The estimate is unambiguous for |f - acqfreq| < 1 / (4 ctime), 250 Hz at 1 ms: every Doppler grid with a step below
 * 1 / (2 ctime) qualifies (the reference's 200 Hz, every coherent_step); coarser grids alias, which is not checked.
 * gnsscorr_acq_set_refine: GNSSCORR_EINVAL, nothing touched and the channel named, for a range outside the channel
 * table, nref < 0, nref == 1, nref > min(intg, GNSSCORR_MAXCOH).  Quiesces and uploads the channel table; the prepared
 * acquisition work and the last search's results stay.  A search without a listed channel with nref > 0 queues exactly
 * the launches it queued before.  Not included: interpolation between the estimator's bins, code-Doppler
 * compensation inside the refine span (rule 3), data wipe-off; the drop-in sdracquisition() is untouched. */
#define GNSSCORR_FINE_BINS 256
typedef struct {
    double finefreq, quality;
    int    q, nref;                 /* the chosen bin q*; periods used (0: no refinement, rule 8) */
} gnsscorr_acqfine_t;
int  gnsscorr_acq_set_refine(gnsscorr_ctx *ctx, int ch0, int nch, const int *nref);
int  gnsscorr_acq_get_refine(gnsscorr_ctx *ctx, int ch0, int nch, int *nref);
/* fine[nch] of the last search; prompt may be NULL, else nch * GNSSCORR_MAXCOH * 2 int32 (I, Q of P_m, zero beyond
 * nref); synchronises.  GNSSCORR_ESTATE before a search. */
int  gnsscorr_acq_fetch_fine(gnsscorr_ctx *ctx, gnsscorr_acqfine_t *fine, int32_t *prompt);
/* Code-Doppler compensation across the groups of a search (opt-in per channel).  A satellite at Doppler
 * fd has its code compressed by fd / f_cf, so over a long span the correlation peak walks from group to group (5 kHz on
 * L1: 0.65 chip over 200 ms) and the non-coherent sum smears it.  f_cf[i] is the RF carrier of channel ch0 + i in Hz
 * (the reference's sdrch_t.f_cf); 0 switches the compensation off, is the default and what gnsscorr_set_channels resets
 * to; gnsscorr_acq_set_coherent and gnsscorr_acq_set_bitedge keep it.  A channel with G = intg / ncoh groups, n = nsamp
 * and bins freq[b] reads group g of bin b s(b, g) samples later, in fp64 and in exactly this order:
 *     dop    = (freq[b] - f_if) - foffset
 *     x      = (dop / f_cf) * (double)((int64_t)g * ncoh * n)
 *     s(b,g) = -(int32_t)rint(x)               round-half-even; s(b, 0) = 0
 *     back   = max(0, max over b, g of s(b,g))
 *     b0     = wrpos - back - (intg + 1) * n
 * Group g of bin b covers the (ncoh + 1) * n ring samples from b0 + g * ncoh * n + s(b,g) on: a positive Doppler starts
 * later groups earlier (s < 0), a negative one later, and `back` keeps the last window inside wrpos.  Everything else is
 * the coherent search's: wipe-off phase 0 at the span's first sample, the windows summed as integers, checkacquisition()'s
 * rules after every group, the first passing group wins, iters = (g + 1) * ncoh, cn0 over ncoh * ctime, buffloc = b0 +
 * acqcodei when acquired and b0 + intg * n when not.  The lag is the lag in group 0's frame: tracking starts from the
 * right samples and no hand-over changes.  The search is, in every respect, the search at write position wrpos - back:
 * the look-back checks of gnsscorr_acq_run (GNSSCORR_ESTATE / GNSSCORR_EINVAL with the sample counts) and the
 * receiver schedule's first search add `back`; gnsscorr_acq_power re-runs with the same shifts; bit-edge hypotheses,
 * the refinement and the 65536-point path combine with it.  With f_cf = 0 for every channel, results, rows and power
 * arrays are bit for bit those of a search without this call.
 * The tables are built on the host when a search prepares the channel set (at most nfreq * G int32 per grid), and that
 * search returns GNSSCORR_EINVAL when some |s(b,g)| > n: more than a code period has no meaning.  Channels share
 * forward spectra only when their shift tables agree as well.
 * gnsscorr_acq_set_codedoppler: GNSSCORR_EINVAL, nothing touched and the channel named, for a range outside the
 * channel table and an f_cf that is negative or not finite.  Quiesces and drops the prepared acquisition work.
 * gnsscorr_acq_fetch_shifts: the channel's s[nfreq][G] and back, as the last prepare built them; GNSSCORR_ESTATE before
 * the first search has prepared.
 * Not included: drift inside a group (at most 0.065 chip in 20 ms on L1), a codefreq preset at hand-over, the drop-in
 * sdracquisition(), the sharded engine. */
int  gnsscorr_acq_set_codedoppler(gnsscorr_ctx *ctx, int ch0, int nch, const double *f_cf);
int  gnsscorr_acq_get_codedoppler(gnsscorr_ctx *ctx, int ch0, int nch, double *f_cf);
int  gnsscorr_acq_fetch_shifts(gnsscorr_ctx *ctx, int ch, int32_t *s /* [nfreq][groups] */, int *back);

/* ---- receiver schedule: acquire, hand over and track each channel by state ----
 * sdrthread()'s state machine (ref src/sdrmain.c:247-316) for every channel of the context: a channel calls
 * sdracquisition() until flagacq, pausing ACQSLEEP after each failure (ref src/sdracq.c:57-60), and from then on tracks
 * one code period per call.  Opt-in: without gnsscorr_rx_start every other entry point behaves as if this section did
 * not exist.
 * The reference's pause is 2000 ms of wall time (sleepms).  Here it is restated on the sample clock: a failed search
 * at write position wp is retried once the channel's ring has reached wp + retry_ms * 1e-3 * f_sf samples, so the
 * schedule depends on the input alone, not on how fast it is fed. */
#define GNSSCORR_CH_IDLE   0   /* parked: never searched, never tracked            */
#define GNSSCORR_CH_SEARCH 1   /* sdrthread before flagacq                         */
#define GNSSCORR_CH_TRACK  2   /* sdrthread after flagacq                          */
typedef struct {
    int      state, attempts;       /* GNSSCORR_CH_*; searches run so far                          */
    uint64_t next_try;              /* SEARCH: due once the ring's write position reaches this     */
    uint64_t acq_wrpos;             /* write position the last search ended at                     */
    gnsscorr_acqres_t acq;          /* result of the last search (of the acquiring one once TRACK) */
    uint64_t cnt;                   /* ref sdrthread's cnt: periods tracked since the hand-over    */
} gnsscorr_rxstat_t;

/* Every channel -> SEARCH, first due at (intg + 1) * nsamp samples, the first moment sdracquisition()'s look-back
 * fits (ref src/sdracq.c:24-26).  retry_ms <= 0: ACQSLEEP (2000).  Needs the channels set and gnsscorr_loop_set done
 * for every one of them (the constants the hand-over keeps); otherwise GNSSCORR_ESTATE.
 * May be called again on the same channels (after gnsscorr_ring_create it must be): the schedule starts over -- states,
 * attempts, losses, the verdicts of a pending monitor launch dropped; the lock monitor, bit synchronisation and the
 * correlation monitor off for all, their device states and the bit-sync applied counts zero, so that every
 * gnsscorr_rx_*_status reads zeros -- while the device's tracking and loop states are not touched.  A channel that is acquired again is handed over like any other and from then on is bit for
 * bit a channel of a fresh context; until then its gnsscorr_rxstat_t.cnt keeps the count of its last run (the next
 * hand-over restarts it at 0), and gnsscorr_loop_get shows the loop state that run left. */
int  gnsscorr_rx_start(gnsscorr_ctx *ctx, int retry_ms);
/* Park a channel (GNSSCORR_CH_IDLE: its tracking and loop state freeze) or re-arm it (GNSSCORR_CH_SEARCH: due at its
 * ring's current write position).  GNSSCORR_CH_TRACK is reached through acquisition only: GNSSCORR_EINVAL. */
int  gnsscorr_rx_set(gnsscorr_ctx *ctx, int ch, int state);
/* One scheduling step at the rings' current write positions wp, ordered on the context's stream:
 *   1. every SEARCH channel with wp >= next_try is searched, all of them in one gnsscorr_acq_run_subset over the window
 *      that ends at wp (the reference's buffloc = fendbuffsize*buffcnt - (intg+1)*nsamp);
 *   2. acquired -> gnsscorr_loop_start_from_acq's hand-over, state TRACK; failed -> next_try = wp + the pause;
 *   3. gnsscorr_trk_run_loop(max_periods) for the TRACK channels, those acquired in 1 included (they start at the
 *      returned buffloc and catch up with wp like any other).  IDLE and SEARCH channels plan no period: ndone = 0,
 *      zero log and II/QQ rows, tracking and loop state untouched.
 * A step without a due channel synchronises no more than gnsscorr_trk_run_loop; one with due channels reads their
 * acquired flags back.  gnsscorr_trk_fetch, gnsscorr_trk_fetch_log and gnsscorr_trk_loop_lapped report part 3. */
int  gnsscorr_rx_step(gnsscorr_ctx *ctx, int max_periods);
/* st[nch]; synchronises the stream (cnt comes from the device's loop state) */
int  gnsscorr_rx_status(gnsscorr_ctx *ctx, gnsscorr_rxstat_t *st);

/* ---- lock monitor: detect loss of lock on the device, send the channel back to SEARCH ----
 * The reference never clears flagacq: a channel whose satellite sets, or that was acquired on noise, tracks noise for
 * the rest of the run.  The monitor is the missing TRACK -> SEARCH edge of the schedule above.  Opt-in per channel;
 * with it off for every channel gnsscorr_rx_step issues the launches and synchronisations it issues without it.
 * The detector (DESIGN.md 3.2b states it line by line) reads, per tracked period, the prompt sums (tap 0 of
 * gnsscorr_trk_fetch's II / QQ) and the log row's flagsync and navbit:
 *   reason 1  the nav bit is not synchronised in the period with cnt + 1 >= sync_periods (sync_periods 0: no such rule);
 *   reason 2  from bit synchronisation on, per whole nav bit (rate periods between two decided bits) the narrow-band /
 *             wide-band power ratio np = ((sum I)^2 + (sum Q)^2) / sum (I^2 + Q^2), which is rate for a clean signal
 *             and about 1 for noise; mu = the mean of kbits consecutive np; nbad consecutive windows with
 *             mu < mu_min.  The usual C/N0 estimate is (mu - 1) / ((rate - mu) * ctime); the tracker biases mu low.
 * A lost state is sticky until the hand-over of the next acquisition restarts cnt at 0, which resets the state. */
typedef struct { int sync_periods, kbits, nbad, pad; double mu_min; } gnsscorr_lockprm_t;
typedef struct { double sI, sQ, w, npsum, mu_last; uint64_t lost_cnt;
                 int open, n, k, nbad, lost, reason, windows, pad; } gnsscorr_lock_t;
/* Op-level: the monitor's kernel over host arrays.  prm[nch], rate[nch] (periods per nav bit, 2..20), st[nch] in-out,
 * I / Q [nch][nper], log[nch][nper] (only flagsync and navbit are read), ndone[nch] (rows of each channel that count,
 * 0..nper), cnt0[nch] (sdrthread's cnt of row 0).  kbits 1..4096, nbad >= 1, sync_periods >= 0, 0 < mu_min <= rate:
 * otherwise GNSSCORR_EINVAL naming the field, st untouched.  Runs on the context's stream and synchronises it; timer
 * name "rx_lock". */
int  gnsscorr_lock_run(gnsscorr_ctx *ctx, const gnsscorr_lockprm_t *prm, const int *rate, gnsscorr_lock_t *st,
                       const double *I, const double *Q, const gnsscorr_trklog_t *log, const int *ndone,
                       const uint64_t *cnt0, int nch, int nper);
/* The monitor's parameters for channels ch0 .. ch0+nch-1 of the schedule (one prm for all of them); prm == NULL or
 * kbits == 0 switches it off for them.  Their detector state is zeroed; the state of a channel no call has named reads
 * as zeros.  A range outside the channel set is GNSSCORR_EINVAL ("channels"), one whose ch0 + nch overflows an int
 * included.  gnsscorr_rx_start leaves the monitor off for all and zeroes every state.
 * Values as above, against each channel's gnsscorr_loop_t.rate; without gnsscorr_rx_start GNSSCORR_ESTATE.
 * With the monitor on, gnsscorr_rx_step
 *   0. reads the verdicts of the previous step's launch (it waits for that launch): a TRACK channel declared lost goes
 *      to SEARCH, due at this step's write position, and is searched in this very step if its look-back fits;
 *   4. behind the closed loop, queues the monitor over the periods this step tracked for the TRACK channels that have
 *      it on, without waiting for it.
 * A loss found in step k therefore takes effect at the start of step k + 1; a failed re-search pauses like any other. */
int  gnsscorr_rx_lock_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_lockprm_t *prm);
/* st[nch]: the detector states on the device, behind whatever the stream still runs; losses[nch]: how often the schedule
 * has sent each channel back to SEARCH.  Either may be NULL.  Synchronises. */
int  gnsscorr_rx_lock_status(gnsscorr_ctx *ctx, gnsscorr_lock_t *st, int *losses);

/* ---- bit synchronisation by symbol energy: preset flagsync / synci from the first tracked periods ----
 * checksync() starts only after cnt > 2000, and its shift-register branch (PRN > 5) takes the first `rate` prompts of
 * one sign for a symbol, wherever the true edge is.  The detector is the standard estimator instead: over the tracked
 * periods from start_cnt on, the prompt sums are added coherently over one symbol at each of the `rate` alignments, and
 * the alignment with the most energy wins when it beats the alignment half a symbol away by the factor `gate`.
 * Opt-in per channel; with it off for every channel gnsscorr_rx_step launches nothing new.
 * The detector (every arithmetic statement one IEEE double operation, no contraction), per channel over
 * the rows e < ndone of one closed-loop run in period order, c = cnt0 + e, (I, Q) = tap 0 of the row's II / QQ,
 * R = the channel's rate:
 *   1. c == 0: the state is zeroed (the first period behind a hand-over).
 *   2. done != 0: nothing more is read.
 *   3. the row's flagsync != 0: done = 3 (the loop synchronised by its own rule, or was preset); stop.
 *   4. c < start_cnt: the row does not count.
 *   5. the first counted row: armed = 1, a0 = c.
 *   6. for every offset o = 0 .. R-1 in ascending order: if fill[o] > 0 or c mod R == o: sI[o] += I, sQ[o] += Q,
 *      fill[o]++; when fill[o] == R: E[o] = E[o] + (sI[o]*sI[o] + sQ[o]*sQ[o]), sI[o] = sQ[o] = 0, fill[o] = 0.
 *      Offsets are in biti units: offset o means a symbol begins on the periods with cnt mod R == o.
 *   7. with L = c - a0 + 1: when (L + 1) mod R == 0 every offset has completed exactly n = (L + 1)/R - 1 whole symbols.
 *      If n >= 1 and n mod nsym == 0, a test: o* = the offset with the largest E (lowest index on ties),
 *      h = (o* + R/2) mod R (integer division), tests++, ratio_last = E[o*]/E[h] when E[h] > 0, else 0.  Pass when
 *      E[o*] > 0 and E[o*] >= gate*E[h] (the product, not the quotient): done = 1, best = o*,
 *      synci = (o* + R - 1) mod R (the biti of a symbol's last period, what checkbit() expects), decided_cnt = c.
 *      Otherwise, if n >= nsym_max: done = 2, the channel is given up and the reference's rule stays in charge.
 * The state does not depend on how the stream is cut into runs. */
typedef struct { int start_cnt, nsym, nsym_max, pad; double gate; } gnsscorr_bsyncprm_t;
typedef struct { double E[20], sI[20], sQ[20]; double ratio_last; uint64_t a0, decided_cnt;
                 int fill[20]; int armed, n, tests, done, best, synci; } gnsscorr_bsync_t;
/* Op-level: the detector's kernel over host arrays, the twin of gnsscorr_lock_run.  prm[nch] (nsym 0: the channel's
 * detector is off and its state stays), rate[nch] (2..20), st[nch] in-out, I / Q [nch][nper], log[nch][nper] (only
 * flagsync is read), ndone[nch] (0..nper), cnt0[nch].  start_cnt >= 0, 1 <= nsym <= nsym_max <= 4096, gate >= 1:
 * otherwise GNSSCORR_EINVAL naming the field, st untouched.  Writes no loop state.  Runs on the context's stream and
 * synchronises it; timer name "rx_bsync". */
int  gnsscorr_bsync_run(gnsscorr_ctx *ctx, const gnsscorr_bsyncprm_t *prm, const int *rate, gnsscorr_bsync_t *st,
                        const double *I, const double *Q, const gnsscorr_trklog_t *log, const int *ndone,
                        const uint64_t *cnt0, int nch, int nper);
/* The detector's parameters for channels ch0 .. ch0+nch-1 of the schedule (one prm for all of them); prm == NULL or
 * nsym == 0 switches it off for them.  Their detector state is zeroed.  gnsscorr_rx_start and gnsscorr_set_channels
 * leave it off for all; without gnsscorr_rx_start GNSSCORR_ESTATE.  With the detector on, gnsscorr_rx_step
 *   3b. behind the closed loop (and in front of the lock monitor) queues the kernel over the periods this step tracked
 *       for the TRACK channels that have it on, without waiting for it.  A channel whose done became 1 in that launch
 *       and whose device loop state (the state behind the step's last period) still has flagsync == 0 gets
 *       flagsync = 1 and synci written into its gnsscorr_loop_t by the same kernel, and its applied count goes up;
 *       navcnt, bitIP, biti and bitsync[] stay, as checksync()'s own success leaves them.
 * A decision therefore takes effect with the first period of the next step: the moment depends on how the stream is
 * cut into steps, as the lock monitor's verdicts do; the detector's state does not. */
int  gnsscorr_rx_bsync_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_bsyncprm_t *prm);
/* st[nch]: the detector states on the device, behind whatever the stream still runs; applied[nch]: how often the
 * schedule preset each channel.  Either may be NULL.  Synchronises. */
int  gnsscorr_rx_bsync_status(gnsscorr_ctx *ctx, gnsscorr_bsync_t *st, int *applied);

/* ---- correlation monitor: data-wiped tap sums and signal quality tests on every tap ----
 * The engine computes up to GNSSCORR_MAXTAPS correlator taps per channel and period, and the loops read the prompt and
 * one early / late pair.  The monitor sums every tap over whole nav bits, wipes the data bit off, adds kbits bits up
 * to a window -- the shape of the correlation function, which the tap sums of gnsscorr_trk_fetch_sums cannot give
 * because the data flips cancel there -- and tests each window's early-minus-late (delta) and early-plus-late (ratio)
 * metrics per tap pair against nominal values: multipath and spoofing detection (signal quality monitoring).  Opt-in
 * per channel; it reports and never acts: it writes no loop, tracking or schedule state.
 * The monitor (every arithmetic statement one IEEE double operation, no contraction, sums in period
 * order, window sums in bit order), per channel with R = gnsscorr_loop_t.rate (2..20), T = 1 + 2*corrn taps in the
 * order {P, E1, L1, E2, L2, ...}, I_t[e] / Q_t[e] = tap t of row e of gnsscorr_trk_fetch's II / QQ (II is the in-phase
 * arm, the one pll() and checkbit() read), flagsync[e] / navbit[e] of the log row, c = cnt0 + e:
 *   for e in 0 .. ndone-1:
 *     if c == 0: st = all zero                          (first period behind a hand-over)
 *     if flagsync[e] == 0: continue
 *     if st.open: for t < T: sI[t] += I_t[e], sQ[t] += Q_t[e];  n += 1
 *     if navbit[e] != 0:                                (checkbit() closed a bit in this period)
 *       if st.open and n == R:                          (a whole bit; any other length is dropped)
 *         bits += 1
 *         if bits > skip_bits:
 *           d = +1.0 if navbit[e] > 0 else -1.0
 *           for t < T: aI[t] += d*sI[t], aQ[t] += d*sQ[t], aP[t] += (sI[t]*sI[t] + sQ[t]*sQ[t])
 *           k += 1
 *           if k == kbits:                              (a window closes)
 *             cfI, cfQ, cfP = aI, aQ, aP;  win_cnt = c;  windows += 1;  P = cfI[0]
 *             for j in 1 .. 16: if j <= corrn and P > 0: delta[j-1] = (cfI[2j-1] - cfI[2j]) / P,
 *                                                        ratio[j-1] = (cfI[2j-1] + cfI[2j]) / P;  else both 0.0
 *             bad = not (P > 0);  worst = 0
 *             for j in 1 .. npair (ascending): if |delta[j-1] - dref[j-1]| > dtol or |ratio[j-1] - rref[j-1]| > rtol:
 *               bad = true, and worst = j if worst == 0
 *             worst_pair = worst;  nbad = nbad + 1 if bad else 0;  alarm = 1 if nbad >= prm.nbad else 0
 *             alarms += alarm;  aI = aQ = aP = 0.0 for all t;  k = 0
 *       open = 1;  n = 0;  sI[t] = sQ[t] = 0.0 for all t
 * The state does not depend on how the stream is cut into runs.  The bits just behind bit synchronisation belong to
 * skip_bits: the switch of the loop filters throws the code loop off for about 3.5 s. */
typedef struct { int kbits, skip_bits, nbad, npair; double dtol, rtol, dref[16], rref[16]; } gnsscorr_cfmprm_t;
typedef struct { double sI[33], sQ[33], aI[33], aQ[33], aP[33], cfI[33], cfQ[33], cfP[33], delta[16], ratio[16];
                 uint64_t win_cnt; int open, n, k, bits, nbad, alarm, alarms, windows, worst_pair, pad; } gnsscorr_cfm_t;
/* Op-level: the monitor's kernel over host arrays, the twin of gnsscorr_bsync_run.  prm[nch] (kbits 0: the channel's
 * monitor is off and its state stays), rate[nch] (2..20), corrn (1..16, one for all channels), st[nch] in-out, II / QQ
 * [nch][nper][1+2*corrn], log[nch][nper] (only flagsync and navbit are read), ndone[nch] (0..nper), cnt0[nch].
 * kbits 1..4096, skip_bits >= 0, nbad >= 1, 1 <= npair <= corrn, dtol > 0, rtol > 0, dref / rref finite: otherwise
 * GNSSCORR_EINVAL naming the channel and the field, st untouched.  One staged transfer, the kernel on the context's
 * stream, one synchronisation; timer name "rx_cfm". */
int  gnsscorr_cfm_run(gnsscorr_ctx *ctx, const gnsscorr_cfmprm_t *prm, const int *rate, int corrn, gnsscorr_cfm_t *st,
                      const double *II, const double *QQ, const gnsscorr_trklog_t *log, const int *ndone,
                      const uint64_t *cnt0, int nch, int nper);
/* The monitor's parameters for channels ch0 .. ch0+nch-1 of the schedule (one prm for all of them); prm == NULL or
 * kbits == 0 switches it off for them.  Their monitor state is zeroed.  gnsscorr_rx_start and gnsscorr_set_channels
 * leave it off for all; without gnsscorr_rx_start GNSSCORR_ESTATE.  With the monitor on, gnsscorr_rx_step
 *   5. behind the closed loop, the bit-synchronisation detector and the lock monitor's launch queues the kernel over
 *      the periods this step tracked for the TRACK channels that have it on.  It reads the device's correlator outputs,
 *      log, period counts and the loop states' rate / cnt in place, waits for nothing and records no event.
 * With the monitor off for every channel a step issues exactly the launches and synchronisations it issues without it.
 * A channel that is re-acquired restarts cnt at 0, which zeroes its monitor state. */
int  gnsscorr_rx_cfm_set(gnsscorr_ctx *ctx, int ch0, int nch, const gnsscorr_cfmprm_t *prm);
/* st[nch]: the monitor states on the device, behind whatever the stream still runs (zeros when the monitor has never
 * been on).  Synchronises. */
int  gnsscorr_rx_cfm_status(gnsscorr_ctx *ctx, gnsscorr_cfm_t *st);

/* ---- frames, observables and epochs behind every step ------------------------
 * The loop a caller writes around a step's rows, as a library object: one nav state per
 * channel -- the frame state of its code type and the observables' state -- plus one gnsscorr_sync_t.  Plain host code
 * (csrc/sdr_rxnav.c): the only device work is what gnsscorr_sbasframe_replay does for an SBAS channel.  DESIGN.md
 * section 3.9 states the rules of a feed; in short, after validation, per channel in ascending order:
 *   1. reset: the frame state, the running part of the observables' state (constants kept, oldremcode 0) and nrows are
 *      zeroed and the channel is detached from the epochs when tracking[k] == 0, or when ndone[k] > 0, cnt0 == 0 and the
 *      channel was fed rows since its last reset (a hand-over restarted cnt); resets counts those that zeroed something;
 *   2. with ndone[k] > 0 and tracking[k], the rows go through the frame replay of the code type (gnsscorr_frame_replay,
 *      gnsscorr_g1frame_replay, gnsscorr_sbasframe_replay without time aid) with cnt0 = cnt_after[k] - ndone[k];
 *   3. if the frame state has flagdec: flagsyncf, polarity, firstsftow and firstsfcnt go into the observables' state;
 *   4. gnsscorr_obs_replay over the same rows, II0 and cnt0;
 *   5. gnsscorr_sync_push of those rows with {flagdec, week, firstsf, firstsfcnt}: the state's week for G1 and SBAS, what
 *      gnsscorr_rxnav_week last set for L1 C/A (the caller's ephemeris decoder; 0: none yet).  No rows, no push;
 *   6. a channel that is attached, has tracking[k], and had ndone[k] == 0 in hold_steps consecutive feeds in each of
 *      which some other channel had rows, is detached; its nav state stays.  hold_steps 0: never.
 * Nothing is flushed.  The one dependence on how a channel's rows are cut into feeds is the documented loop's: the row
 * in which the observables learn of the frame is the first row of the piece that raised flagdec, not the row that
 * decided the frame's last symbol (an inverted frame's half cycle enters the carrier phase there).  Everything else is
 * independent of the cut.
 * Errors.  GNSSCORR_EINVAL, nothing touched: a NULL pointer, ndone[k] < 0, stride < ndone[k], cnt_after[k] < ndone[k],
 * an SBAS channel with ctx == NULL.  GNSSCORR_ESTATE, nothing touched, the channel named: ndone[k] > 0, the channel was
 * fed before, and cnt0 is neither 0 nor the cnt_after[k] of the feed before (a step's rows were skipped).  An error of a
 * replay or of the push (GNSSCORR_ESTATE for a full queue) is returned with the channel named; the channels before it
 * have been fed.  One thread at a time per object. */
typedef struct {                    /* constants of one channel */
    int    ctype, nsamp, loopms, pad;               /* CTYPE_L1CA (1) / CTYPE_L1SBAS (27) / CTYPE_G1 (20) */
    double f_sf, f_if, foffset, ctime, ti;
    double oldremcode;              /* gnsscorr_obs_t.oldremcode for the channel's very first row; 0 after every reset */
} gnsscorr_rxnavch_t;
typedef struct {
    int      ctype, attached;       /* attached: has pushed rows to the epochs since it was last detached */
    int      flagsyncf, flagdec, polarity, week, id;   /* id: sfid / string number / message type decoded last */
    int      resets;                /* how often a non-empty state of this channel was zeroed */
    uint64_t cnt;                   /* sdrthread's cnt behind the last feed */
    uint64_t firstsf, firstsfcnt, nrows;            /* nrows: rows of observables since the last reset */
    double   firstsftow, tow;       /* tow of the last row of observables, 0: none yet */
} gnsscorr_rxnavstat_t;
typedef struct gnsscorr_rxnav gnsscorr_rxnav_t;

/* GNSSCORR_EINVAL: NULL, nch <= 0, hold_steps < 0, a code type outside the three.  What gnsscorr_sync_create and
 * gnsscorr_sync_channel refuse is passed through with their message (outms <= 0, a ti that differs between channels).
 * Every channel starts declared and detached. */
int  gnsscorr_rxnav_create(gnsscorr_rxnav_t **nv, int nch, const gnsscorr_rxnavch_t *ch, int outms, int hold_steps);
void gnsscorr_rxnav_destroy(gnsscorr_rxnav_t *nv);
int  gnsscorr_rxnav_week(gnsscorr_rxnav_t *nv, int ch, int week);       /* L1 C/A: the caller's decoder; 0: none yet */
/* log[nch][stride] and II0[nch][stride]: a step's gnsscorr_trk_fetch_log rows and tap 0 of II (gnsscorr_trk_fetch_prompt);
 * ndone[k]: the rows of channel k that count; cnt_after[k]: sdrthread's cnt of channel k behind the step; tracking[k]:
 * channel k is in TRACK behind the step.  ctx may be NULL when no channel is CTYPE_L1SBAS. */
int  gnsscorr_rxnav_feed(gnsscorr_rxnav_t *nv, gnsscorr_ctx *ctx, const gnsscorr_trklog_t *log, const double *II0,
                         int stride, const int *ndone, const uint64_t *cnt_after, const int *tracking);
int  gnsscorr_rxnav_flush(gnsscorr_rxnav_t *nv);                                        /* gnsscorr_sync_flush */
int  gnsscorr_rxnav_fetch(gnsscorr_rxnav_t *nv, gnsscorr_epochobs_t *out, int max_out); /* gnsscorr_sync_fetch */
int  gnsscorr_rxnav_status(gnsscorr_rxnav_t *nv, gnsscorr_rxnavstat_t *st);             /* st[nch] */
int  gnsscorr_rxnav_frame(gnsscorr_rxnav_t *nv, int ch, void *state, size_t size);      /* copy of the channel's
                                    gnsscorr_frame_t / _sbasframe_t / _g1frame_t; size must be that struct's */
int  gnsscorr_rxnav_rows(gnsscorr_rxnav_t *nv, int ch, gnsscorr_obsrow_t *rows, int max_rows);  /* rows the last feed made;
                                    returns their number, at most max_rows */
/* the message of the last failed gnsscorr_rxnav_* call of this thread (csrc/sdr_rxnav.c links without the device code,
 * so it keeps its own; the context's calls below copy it into gnsscorr_last_error) */
const char *gnsscorr_rxnav_last_error(void);

/* The context's driver: a step of the receiver and the feed of its rows in one call.
 * gnsscorr_rx_nav_start needs the channels and gnsscorr_loop_set for every one of them (GNSSCORR_ESTATE otherwise).  It
 * fills gnsscorr_rxnavch_t from the channel table and the loop constants and takes oldremcode from the tracking state.
 * With the schedule on (gnsscorr_rx_start done) it must come before the first step: GNSSCORR_ESTATE if any channel has
 * attempts > 0.  Without the schedule every channel counts as tracking.  Calling it again starts over.
 * gnsscorr_rx_nav_step runs gnsscorr_rx_step(max_periods) with the schedule on, gnsscorr_trk_run_loop(max_periods)
 * without (their error comes first), fetches the log, ndone, the prompt column and the counters (gnsscorr_rxstat_t.cnt
 * and state == GNSSCORR_CH_TRACK, or gnsscorr_loop_t.cnt) and feeds the core.  The plain fetches stay valid behind it.
 * gnsscorr_set_channels, a later gnsscorr_rx_start and a gnsscorr_ring_create of a ring that a channel reads switch the
 * driver off: its calls return GNSSCORR_ESTATE (gnsscorr_rx_nav: NULL) until the next start.  gnsscorr_destroy frees it. */
int  gnsscorr_rx_nav_start(gnsscorr_ctx *ctx, int outms, int hold_steps);
int  gnsscorr_rx_nav_step(gnsscorr_ctx *ctx, int max_periods);
gnsscorr_rxnav_t *gnsscorr_rx_nav(gnsscorr_ctx *ctx);   /* the context's core object, NULL when off: week, fetch, flush,
                                                           status, frame, rows go through it */
int  gnsscorr_rx_nav_stop(gnsscorr_ctx *ctx);

/* ---- op-level device entry points (used by the per-call symbols and tests) --
 * 16384-point complex FFT batches on device memory, unnormalised, sign -1
 * forward / +1 backward; in/out are device pointers to float2[batch][16384] */
int  gnsscorr_fft16k(gnsscorr_ctx *ctx, const void *in, void *out, int sign,
                     int batch);
/* cpxpspec (ref src/sdrcmn.c:261-276) for n = 16384 or 32768 on host data */
int  gnsscorr_pspec(gnsscorr_ctx *ctx, const float *cpx, int n, int flagsum,
                    double *pspec);

/* ---- IF monitor: sample histogram and averaged power spectrum on the ring --
 * What specthread() computes every SPEC_MS (ref src/sdrspec.c:64-102) --
 * rcvgetbuff() + calchistgram() (ref src/sdrspec.c:170-206) +
 * spectrumanalyzer() (ref src/sdrspec.c:232-296) -- read straight from the
 * HBM ring, for nsnap snapshots in one launch chain on the context's stream. */
typedef struct {
    int    ftype;   /* ring 1 or 2; dtype comes from the ring                         */
    int    nfft;    /* 8192 or 16384 (2*nfft-point transform); ref SPEC_NFFT          */
    int    nloop;   /* segments averaged per snapshot, >= 1; ref SPEC_NLOOP           */
    int    n;       /* samples per snapshot, nfft/2 <= n <= ringlen; ref SPEC_LEN*nsamp */
    double f_sf;    /* Hz, for the frequency axis                                     */
} gnsscorr_spec_t;
/* Snapshot s covers samples [buffloc[s], buffloc[s] + n), which the ring must
 * hold at call time (wrpos - ringlen <= buffloc[s], buffloc[s] + n <= wrpos);
 * segment k of it starts offsets[s*nloop + k] samples in, 0 <= offset <=
 * n - nfft/2 (the reference's zuz).  Anything else: GNSSCORR_EINVAL naming the
 * snapshot, and nothing is launched.  Asynchronous. */
int  gnsscorr_spec_run(gnsscorr_ctx *ctx, const gnsscorr_spec_t *sp, int nsnap,
                       const uint64_t *buffloc, const int *offsets);
/* Results of the last gnsscorr_spec_run.  Any pointer may be NULL; caps are
 * element counts, and a cap below what the run needs is GNSSCORR_EINVAL with
 * nothing written.
 *   s[nsnap][2*nfft]       linear segment sums in FFT order (the reference's s)
 *   pspec[nsnap][dtype*nfft] dB, and freq[dtype*nfft] MHz, laid out as the
 *                          reference's (ref src/sdrspec.c:280-294)
 *   hist[nsnap][2][9]      I and Q counts of the bins {-7,-5,...,+7}; the 9th
 *                          counts d == maxd > 7, which the reference writes one
 *                          element past yI / yQ; the Q row is zero for dtype 1
 * Synchronises. */
int  gnsscorr_spec_fetch(gnsscorr_ctx *ctx, double *s, size_t s_cap,
                         double *pspec, size_t pspec_cap, double *freq,
                         size_t freq_cap, int64_t *hist, size_t hist_cap);

/* per-kernel launch timing: enable, run, then read the accumulated HIP-event
 * time of the named kernel ("trk_corr", "trk_plan", "trk_spec", "trk_expand",
 * "trk_finish", "acq_fwd", "acq_corr", "acq_code", "acq_final", "spec_psd",
 * "spec_sum", "spec_hist", "fec_viterbi27", "rx_lock", "rx_bsync", "rx_cfm",
 * "trk_prompt").
 * on = 1: every kernel; on = 2: only the two correlator kernels ("trk_corr",
 * "acq_corr"), leaving the planner and tables streams free of events; 0: off */
int  gnsscorr_timing_enable(gnsscorr_ctx *ctx, int on);
int  gnsscorr_timing_read(gnsscorr_ctx *ctx, const char *kernel,
                          double *total_ms, int *launches);
int  gnsscorr_timing_reset(gnsscorr_ctx *ctx);

/* the process-wide context the per-call reference symbols use (device 0 or
 * $GNSSCORR_DEVICE); created on first use */
gnsscorr_ctx *gnsscorr_default_ctx(void);

#ifdef __cplusplus
}
#endif
#endif
