// Host harness for tests/test_nco_carrier_rec.py: one period of the batch planner's carrier chain as
// gnsscorr_plan.hip runs it on a staged record (csrc/gnsscorr_nco.h: gc_car_rec_make, gc_carrier_rec_step_one),
// with the bracket discovered as trk_spec_kernel discovers it.
#include "../../erlangnetwork-gnsslib-sdr_amd/csrc/gnsscorr_nco.h"

extern "C" {

// Period of n samples from remcarr with addend ps (nmax: the channel's longest period).  The discovery sees the
// estimate est and brackets it by +-w (w = 0: claims of the estimate itself, no bracket); nrow is the sample count
// it settled on.  Returns what served the period: 1 the window value step, 2 the record's one-binade step,
// 3 the reference one-binade step, 4 the step with its checks on the row's claims, 5 the certified step / walkers.
// info: row tag, record ctl, record key, 1 when the record's one-binade step and the reference form both stepped.
// *same: 0 when they both stepped and differ.
int ncr_period(double ps, int nmax, double remcarr, int n, double est, double w, int nrow, double *out, int *info, int *same)
{
    GC_FP_STRICT
    GcCarPlan P;
    gc_car_plan_init(P, ps);
    GcCarStepC C;
    gc_car_stepc_init(C, P, nmax);
    // the row, as trk_spec_kernel writes it
    GcCarClaims ck;
    double dummy;
    const double klo = est - w, khi = est + w;
    bool kbr = false;
    if (w > 0.0) {
        bool ok = gc_carrier_claims_step<true>(P, C, klo, nrow, ck, &dummy);
        const int tag = ck.tag;
        ok = ok && gc_carrier_claims_step<false, true>(P, C, khi, nrow, ck, &dummy);
        if (ok) {
            kbr = true;
            ck.tag = tag;
            ck.lo = klo;
            ck.hi = khi;
        }
    }
    if (!kbr) {
        const bool ok = gc_carrier_claims_step<true>(P, C, est, nrow, ck, &dummy);
        ck.tag = ok ? (ck.tag == 2 ? 2 : 3) : 0;
        ck.lo = ck.hi = est;
    }
    ck.nl = nrow;
    // the record and the chain's period (plan4_car_period)
    GcCarRec R;
    gc_car_rec_make(R, ck, n, C.ilo, C.ex0, C.s, P.ydpi);
    info[0] = ck.tag;
    info[1] = R.ctl;
    info[2] = R.key;
    info[3] = 0;
    *same = 1;
    const int ctl = R.ctl, tag = GC_REC_TAG(ctl);
    if (!(ctl & GC_REC_WALK)) { *out = remcarr; return 0; }
    const bool inside = remcarr >= R.lo && remcarr <= R.hi && (ctl & (3 | GC_REC_NMATCH)) == (1 | GC_REC_NMATCH);
    if (inside) {
        *out = gc_carrier_value_step(P, C, remcarr, GC_REC_P0(ctl), GC_REC_PLAST(ctl), GC_REC_KPREM(ctl), R.dmd);
        return 1;
    }
    if (tag == 2) {
        double r1 = 0.0, r2 = 0.0;
        const bool ref = gc_carrier_value_step_one(P, C, remcarr, n, GC_REC_KPREM(ctl), &r1);
        const bool rec = (ctl & GC_REC_ONE) &&
                         gc_carrier_rec_step_one(P.ydpi, remcarr, R.key, (ctl & GC_REC_TIE) != 0, R.dmd[0], R.dmd[1], R.dmd[2], GC_REC_KPREM(ctl), &r2);
        if (rec && !ref) *same = 0;
        if (rec && ref) {
            info[3] = 1;
            *same = gc_d2u(r1) == gc_d2u(r2);
        }
        if (rec) { *out = r2; return 2; }
        if (ref) { *out = r1; return 3; }
    }
    if (ck.tag != 0) {
        GcCarClaims c2 = ck;
        c2.tag = ck.tag == 2 ? 2 : 1;
        double rp;
        if (gc_carrier_claims_step<false, true>(P, C, remcarr, n, c2, &rp)) { *out = rp; return 4; }
    }
    GcFillLoop fill;
    GcNoEmit ne;
    int tier;
    *out = gc_carrier_period_any(P, remcarr, n, fill, ne, &tier);
    return 5;
}

// gc_one_binade_consts against gc_one_binade_walk at one phase: 1 when the walk's verdict and value are what the
// constants of x's binade give (the comparison gc_carrier_rec_step_one relies on)
int ncr_consts(double x, double s, int n)
{
    GC_FP_STRICT
    double y = 0.0, dref = 0.0;
    bool tieref = false;
    const bool ref = gc_one_binade_walk(x, s, n, &y, &dref, &tieref);
    double d = 0.0, top = 0.0;
    bool tie = false;
    bool got = gc_one_binade_consts(gc_expo(x), s, &d, &tie, &top) && (gc_d2u(x) >> 63) == (gc_d2u(s) >> 63);
    double y2 = 0.0;
    if (got && tie && (gc_d2u(x) & 1)) got = false;
    if (got) {
        y2 = fma((double)n, d, x);
        if (!(fabs(y2) <= top)) got = false;
    }
    if (got != ref) return 0;
    if (ref && (gc_d2u(y) != gc_d2u(y2) || gc_d2u(d) != gc_d2u(dref) || tie != tieref)) return 0;
    return 1;
}

}
