// Host harness for tests/test_nco_code_scan.py: the code chain taken the way the batch planner's code wavefront takes
// it (csrc/gnsscorr_nco.h: gc_code_scan_row, gc_code_scan_next) -- brackets and claims discovered as trk_spec_kernel
// discovers them, a scan row per bracketed period, the running Y carried from served period to served period.
#include "../../erlangnetwork-gnsslib-sdr_amd/csrc/gnsscorr_nco.h"

extern "C" {

// nper periods from remcode0; off[e]: how far the discovery's estimate of period e's start lies from the exact one
// (half-width of the bracket: 2^-30).  Out: rem[nper + 1] period starts, ns[nper] samples, how[nper]: 1 served by the
// scan, 2 by the step functions; info[0]: periods with a valid scan row, info[1]: served periods whose carried Y is
// not the head's own, info[2]: 1 when the channel has a code plan at all (P.ok).
int ncs_chain(double ci, int len, int smax, double spc, double remcode0, int nper, const double *off, double *rem, int *ns,
              int *how, int *info)
{
    GC_FP_STRICT
    GcCodePlan P;
    gc_code_plan_init(P, ci, len, smax);
    const double dlen = (double)len, w = 9.313225746154785e-10;
    const double u = gc_code_scan_u(dlen), invu = gc_code_scan_invu(dlen);
    const int tmax = gc_tail_max(gc_tail_class(smax));
    info[0] = info[1] = 0;
    info[2] = P.ok ? 1 : 0;
    double r = remcode0;
    bool haveY = false;
    long long Y = 0;
    for (int e = 0; e < nper; e++) {
        rem[e] = r;
        const int n = gc_period_nsamp(dlen, r, spc);
        ns[e] = n;
        if (!(n > 0 && n <= (1 << 24))) return -1;
        // discovery (trk_spec_kernel, first attempt)
        const double est = r + off[e], lo = est - w, hi = est + w;
        GcCodeClaims cc;
        GcCodeScanRow row;
        row.valid = 0;
        bool bracketed = false;
        const int nlo = gc_period_nsamp(dlen, lo, spc), nhi = gc_period_nsamp(dlen, hi, spc);
        if (nlo == nhi && nlo > 0 && nlo <= (1 << 24)) {
            double flo = 0.0, fhi = 0.0;
            const bool side = (lo - P.smaxci < 0.0) == (hi - P.smaxci < 0.0);
            const bool oklo = gc_code_claims<true>(P, lo, nlo + 2 * smax, cc, &flo);
            const bool okhi = oklo && gc_code_claims<false>(P, hi, nlo + 2 * smax, cc, &fhi);
            if (side && oklo && okhi && nlo + 2 * smax - cc.jsum <= tmax) {
                bracketed = true;
                gc_code_scan_row(row, P, lo, hi, flo, fhi);
            }
        }
        info[0] += row.valid;
        // the chain
        if (bracketed && row.valid && r >= lo && r <= hi && n == nlo) {
            bool neg;
            int ecs;
            const long long Yown = (long long)(gc_code_scan_head(r, P.smaxci, dlen, &neg, &ecs) * invu);
            if (!haveY) Y = Yown;
            if (Y != Yown || !neg) info[1]++;
            r = gc_code_scan_next(row.r1, row.Yhat, Y, u);
            Y += row.K;
            haveY = true;
            how[e] = 1;
        } else {
            GcFillLoop fill;
            GcNoEmit ne;
            int tier;
            r = gc_code_period_any<GcFillLoop, GcNoEmit, false>(P, r, n + 2 * smax, fill, ne, &tier);
            haveY = false;
            how[e] = 2;
        }
    }
    rem[nper] = r;
    return 0;
}

}
