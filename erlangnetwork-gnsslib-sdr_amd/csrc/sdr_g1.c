/*
 * sdr_g1.c -- frame synchronisation of GLONASS G1 on the decided symbols: what sdrnavigation() does behind checkbit()
 * for CTYPE_G1 (ref src/sdrnav.c:40-82), replayed over the `navbit` column of a closed-loop log.  One symbol per 10 ms
 * and channel: scalar host work (DESIGN.md sections 3.6 and 7).  Plain C with no device and no dependence on the rest
 * of the library: a stand-alone program can compile and link this file alone (tests/host/g1frame_host.c does).
 * Each function cites the reference routine whose behaviour it reproduces ("ref <file>:<line>").
 */
#include <stdint.h>
#include <string.h>

#include "../../include/gnsscorr.h"

#define G1_FLEN    200                  /* NAVFLEN_G1, NAVADDFLEN_G1 = 0 (ref src/sdr.h:172-173) */
#define G1_PRELEN  30                   /* NAVPRELEN_G1 (ref src/sdr.h:174) */
#define G1_NDATA   170                  /* meander symbols of a string: 85 bits x 2 */
#define G1_NBITS   85
#define G1_UPDATE  2000                 /* flen * rate periods (ref src/sdrinit.c:552) */
#define G1_EPHCNT  5                    /* NAVEPHCNT_G1 (ref src/sdr.h:175) */

/* ---- time: RTKLIB's epoch2time / utc2gpst / time2gpst on whole seconds (ref lib/RTKLIB/src/rtkcmn.c) ---- */

/* seconds since 1970-01-01 of a calendar date; 0 outside 1970..2099 or months 1..12 (ref rtkcmn.c:1201-1215).  The day
 * enters linearly: day 0 is the last day of the month before. */
static int64_t g1_epoch(int year, int mon, int day, int h, int m, int s)
{
    static const int doy[12] = {1, 32, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335};
    if (year < 1970 || year > 2099 || mon < 1 || mon > 12) return 0;
    const int days = (year - 1970) * 365 + (year - 1969) / 4 + doy[mon - 1] + day - 2 + (year % 4 == 0 && mon >= 3 ? 1 : 0);
    return (int64_t)days * 86400 + h * 3600 + m * 60 + s;
}

/* UTC to GPS time: the newest leap second at or before t (ref rtkcmn.c:136-156, :1442-1450) */
static int64_t g1_utc2gpst(int64_t t)
{
    static const short leaps[18][3] = {
        {2017, 1, 18}, {2015, 7, 17}, {2012, 7, 16}, {2009, 1, 15}, {2006, 1, 14}, {1999, 1, 13}, {1997, 7, 12},
        {1996, 1, 11}, {1994, 7, 10}, {1993, 7, 9}, {1992, 7, 8}, {1991, 1, 7}, {1990, 1, 6}, {1988, 1, 5},
        {1985, 7, 4}, {1983, 7, 3}, {1982, 7, 2}, {1981, 7, 1}};
    for (int i = 0; i < 18; i++)
        if (t >= g1_epoch(leaps[i][0], leaps[i][1], 1, 0, 0, 0)) return t + leaps[i][2];
    return t;
}

/* glot2time(): ref src/sdrnav_glo.c:118-151 with its quirks: in the first year of the interval
 * doy = nt where the other years use nt - ... + 1, so against the 1-based tables the date is the day before; the month
 * loop stops at 11, so a December date ends as month 12, day 0; nt > 1461 leaves j = 0, doy = 0. */
static int64_t g1_glot2time(int nt, int n4, const int *tk)
{
    static const int doys[12] = {1, 32, 60, 91, 121, 152, 182, 213, 244, 274, 305, 335};
    static const int doysl[12] = {1, 32, 61, 92, 122, 153, 183, 214, 245, 275, 306, 336};
    int j = 0, doy = 0, day = 0, mon;
    if (nt <= 366) { j = 1; doy = nt; }
    else if (nt <= 731) { j = 2; doy = nt - 366 + 1; }
    else if (nt <= 1096) { j = 3; doy = nt - 731 + 1; }
    else if (nt <= 1461) { j = 4; doy = nt - 1096 + 1; }
    const int year = 1996 + 4 * (n4 - 1) + (j - 1);
    const int *tab = j == 1 ? doysl : doys;
    for (mon = 1; mon < 12; mon++)
        if (doy < tab[mon]) {
            day = doy - tab[mon - 1];
            break;
        }
    return g1_utc2gpst(g1_epoch(year, mon, day, tk[0], tk[1], tk[2]));
}

/* merge_g1() without the ephemeris (ref src/sdrnav_glo.c:157-165): week and seconds since 1980-01-06 (ref
 * rtkcmn.c:1261-1269; the quotient truncates towards zero as C's does, here in 64 bits), plus 2 s per string since
 * string 1 began */
static void g1_merge(gnsscorr_g1frame_t *st)
{
    const int64_t sec = g1_glot2time(st->nt, st->n4, st->tk) - g1_epoch(1980, 1, 6, 0, 0, 0);
    const int64_t w = sec / (86400 * 7);
    st->week = (int)w;
    st->tow_gpst = (double)(sec - w * 86400 * 7) + st->s1cnt * 2.0;
}

/* getbitu() of RTKLIB: bit 0 is the MSB of buff[0] */
static int g1_getbitu(const unsigned char *buff, int pos, int len)
{
    unsigned v = 0;
    for (int i = pos; i < pos + len; i++) v = (v << 1) | ((buff[i >> 3] >> (7 - (i & 7))) & 1u);
    return (int)v;
}

/* decode_g1() and decode_flame_g1() (ref src/sdrnav_glo.c:177-224): meander off, relative code off, the 85 bits packed
 * with -1 as one, then the fields this library keeps of strings 1, 2, 4 and 5 */
static void g1_decode(gnsscorr_g1frame_t *st)
{
    int b1[G1_NDATA], b2[G1_NBITS];
    for (int i = 0; i < G1_NDATA; i++) b1[i] = (i % 2 == 0 ? st->polarity : -st->polarity) * st->fbits[i];
    b2[0] = -1;
    for (int i = 0; i < G1_NBITS - 1; i++) b2[i + 1] = b1[2 * i] * b1[2 * (i + 1)];
    memset(st->str, 0, sizeof(st->str));
    for (int i = 0; i < G1_NBITS; i++)
        if (b2[i] < 0) st->str[i >> 3] |= (unsigned char)(0x80u >> (i & 7));
    st->id = g1_getbitu(st->str, 1, 4);
    switch (st->id) {
    case 1:
        st->tk[0] = g1_getbitu(st->str, 9, 5) - 3;      /* Moscow time to UTC */
        st->tk[1] = g1_getbitu(st->str, 14, 6);
        st->tk[2] = g1_getbitu(st->str, 20, 1) * 30;
        break;
    case 2: {
        const int iode = g1_getbitu(st->str, 9, 7);
        if (iode != st->iode) st->update = 1;
        st->iode = iode;
        break;
    }
    case 4:
        st->nt = g1_getbitu(st->str, 59, 11);
        st->slot = g1_getbitu(st->str, 70, 5);
        break;
    case 5:
        st->n4 = g1_getbitu(st->str, 49, 5);
        break;
    default:
        break;
    }
    if (st->id >= 1 && st->id <= 5) st->ephcnt++;
    if (st->id == 1) st->s1cnt = 1;
    else st->s1cnt++;
    if (st->ephcnt == G1_EPHCNT) g1_merge(st);
}

int gnsscorr_g1frame_replay(gnsscorr_g1frame_t *st, const gnsscorr_trklog_t *log, int nper, uint64_t cnt0)
{
    /* the ICD's time mark 111110001101110101000010010110 with a one as -1 (ref src/sdrinit.c:494-496) */
    static const signed char mark[G1_PRELEN] = {-1, -1, -1, -1, -1, 1, 1, 1, -1, -1, 1, -1, -1, -1, 1,
                                                -1, 1, -1, 1, 1, 1, 1, -1, 1, 1, -1, 1, -1, -1, 1};
    if (!st || !log || nper < 0) return GNSSCORR_EINVAL;
    for (int p = 0; p < nper; p++) {
        const int bit = log[p].navbit;
        if (!bit) continue;                     /* checkbit() decided no symbol in this period: swsync is off */
        const uint64_t cnt = cnt0 + (uint64_t)p;
        memmove(st->fbits, st->fbits + 1, sizeof(int) * (G1_FLEN - 1));
        st->fbits[G1_FLEN - 1] = bit;
        if (!st->flagtow) {                     /* findpreamble(): the time mark ends the string (ref src/sdrnav.c:392-408) */
            int corr = 0;
            for (int i = 0; i < G1_PRELEN; i++) corr += st->fbits[G1_FLEN - G1_PRELEN + i] * mark[i];
            st->flagsyncf = corr == G1_PRELEN || corr == -G1_PRELEN;    /* (paritycheck() passes every G1 string, ref :362-364) */
            if (st->flagsyncf) {
                st->polarity = corr > 0 ? 1 : -1;
                st->firstsf = log[p].buffloc;
                st->firstsfcnt = cnt;
                st->flagtow = 1;
            }
        }
        if (st->flagtow && (int)(cnt - st->firstsfcnt) % G1_UPDATE == 0) {     /* a whole string: 200 symbols x 10 periods */
            g1_decode(st);
            if (st->tow_gpst == 0) {            /* no time yet: start over (ref src/sdrnav.c:69-72) */
                st->flagsyncf = 0;
                st->flagtow = 0;
            } else if (cnt == st->firstsfcnt) {
                st->flagdec = 1;
                st->firstsftow = st->tow_gpst;
            }
        }
    }
    return GNSSCORR_OK;
}
