// Host harness for tests/test_nco_value_step.py: the value-only period steps of csrc/gnsscorr_nco.h next to the
// claims steps they stand in for, on claims discovered at the same start.
#include "../../erlangnetwork-gnsslib-sdr_amd/csrc/gnsscorr_nco.h"

template <int ITOP, int TMAX>
static int code_eval(const GcCodePlan &P, double remcode, int nt, const GcCodeClaims &cl, double *val, int *ok)
{
    GcCodeStepC<ITOP> C;
    gc_code_stepc_init(C, P);
    GcCodeClaims c2 = cl;
    double dmd[ITOP + 1];
    for (int i = 0; i <= ITOP; i++) dmd[i] = (double)cl.dm[i];
    ok[0] = gc_code_claims_step<ITOP, TMAX, false, true>(P, C, remcode, nt, c2, &val[0]);
    ok[1] = gc_code_claims_step<ITOP, TMAX, false>(P, C, remcode, nt, c2, &val[1], dmd);
    val[2] = gc_code_value_step<ITOP, TMAX>(C, remcode, nt, cl.q, cl.nl, cl.i0, cl.jsum, dmd);
    ok[2] = 1;
    return 1;
}

template <int ITOP>
static int code_tmax(int tmax, const GcCodePlan &P, double remcode, int nt, const GcCodeClaims &cl, double *val, int *ok)
{
    switch (tmax) {
    case 8:  return code_eval<ITOP, 8>(P, remcode, nt, cl, val, ok);
    case GC_CLAIM_TAIL:  return code_eval<ITOP, GC_CLAIM_TAIL>(P, remcode, nt, cl, val, ok);
    case GC_CLAIM_TAIL2: return code_eval<ITOP, GC_CLAIM_TAIL2>(P, remcode, nt, cl, val, ok);
    default: return 0;
    }
}

extern "C" {

// Carrier period of n samples from remcarr with addend ps (nmax: the channel's longest period).  Discovers the
// claims at the start, then evaluates them three ways: val[0] the claims step on its row (SHAPE 0), val[1] the
// claims step in the shape the chain calls it with (dm as doubles for the window), val[2] the value step.
// ok[0..2]: what each returned (the window value step returns nothing: 1).  info: tag, p0, nseg, kprem, ptie.
// Returns the tag (0: no claims, nothing evaluated).
int nvs_carrier(double ps, int nmax, double remcarr, int n, double *val, int *ok, int *info)
{
    GC_FP_STRICT
    GcCarPlan P;
    gc_car_plan_init(P, ps);
    GcCarStepC C;
    gc_car_stepc_init(C, P, nmax);
    GcCarClaims cl;
    double dummy;
    gc_carrier_claims_step<true>(P, C, remcarr, n, cl, &dummy);
    info[0] = cl.tag;
    info[1] = cl.i0 - C.ilo;
    info[2] = cl.nseg;
    info[3] = cl.kprem;
    info[4] = C.ptie;
    if (cl.tag == 0) return 0;
    double dmd[GC_CLAIM_CWIN];
    for (int p = 0; p < GC_CLAIM_CWIN; p++) dmd[p] = (double)cl.dm[p];
    val[0] = val[1] = val[2] = 0.0;
    ok[0] = gc_carrier_claims_step<false>(P, C, remcarr, n, cl, &val[0]);
    if (cl.tag == 1) {
        ok[1] = gc_carrier_claims_step<false, false, 1>(P, C, remcarr, n, cl, &val[1], dmd);
        const int p0 = cl.i0 - C.ilo;
        val[2] = gc_carrier_value_step(P, C, remcarr, p0, p0 + cl.nseg - 1, cl.kprem, dmd);
        ok[2] = 1;
    } else {
        ok[1] = gc_carrier_claims_step<false, false, 2>(P, C, remcarr, n, cl, &val[1]);
        ok[2] = gc_carrier_value_step_one(P, C, remcarr, n, cl.kprem, &val[2]);
    }
    return cl.tag;
}

// Code period of nt replica positions from remcode (addend ci, code length len, smax): claims discovered at the
// start, evaluated by the claims step as a discovering lane (val[0]), as the chain calls it (val[1]) and by the value
// step (val[2]), in the instance with tail length tmax (8, GC_CLAIM_TAIL or GC_CLAIM_TAIL2).  info: itop, q, nl, i0,
// t (tail additions), it (tie binade or -1).  Returns 1 when the claims exist and fit the instance, else 0.
int nvs_code(double ci, int len, int smax, double remcode, int nt, int tmax, double *val, int *ok, int *info)
{
    GC_FP_STRICT
    GcCodePlan P;
    gc_code_plan_init(P, ci, len, smax);
    info[0] = P.ok ? P.itop : -1;
    info[5] = P.it;
    if (!P.ok) return 0;
    GcCodeClaims cl;
    double dummy;
    if (!gc_code_claims<true>(P, remcode, nt, cl, &dummy)) return 0;
    info[1] = cl.q;
    info[2] = cl.nl;
    info[3] = cl.i0;
    info[4] = nt - cl.jsum;
    if (nt - cl.jsum > tmax) return 0;
    switch (P.itop) {
    case 7:  return code_tmax<7>(tmax, P, remcode, nt, cl, val, ok);
    case 8:  return code_tmax<8>(tmax, P, remcode, nt, cl, val, ok);
    case 9:  return code_tmax<9>(tmax, P, remcode, nt, cl, val, ok);
    case 10: return code_tmax<10>(tmax, P, remcode, nt, cl, val, ok);
    case 11: return code_tmax<11>(tmax, P, remcode, nt, cl, val, ok);
    case 12: return code_tmax<12>(tmax, P, remcode, nt, cl, val, ok);
    default: return 0;
    }
}

}
