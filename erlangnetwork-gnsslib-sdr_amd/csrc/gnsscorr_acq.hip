// gnsscorr_acq.hip -- parallel code phase acquisition for gfx950 (MI355X).
//
// Replaces sdracquisition()'s loop (ref src/sdracq.c:29-43): per iteration
// pcorrelator() (ref src/sdrcmn.c:738-773) = mixcarr + cpxcpx + cpxconv per
// Doppler bin, accumulated into P, then checkacquisition() (ref
// src/sdracq.c:71-95).
//
// The reference's FFT length m = 2*nsamp (32736) is replaced by L = 32768:
// the replica has only nsamp non-zero samples and the data window 2*nsamp, so
// lags 0..nsamp-1 never wrap for any L >= 2*nsamp-1 and the correlation values
// are the same numbers (hard part 3).  A length-32768 transform is
// done as two LDS-resident 16384-point transforms (gnsscorr_fft.h) plus one
// radix-2 stage; spectra stay in the FFT's pass order (no reordering anywhere):
//
//   acq_fwd  (per Doppler bin, iteration; shared by all SVs of a grid):
//            carrier wipe-off of the 2*nsamp window straight from the HBM
//            ring, FFT of the even and of the odd samples, radix-2 combine,
//            spectrum stored split by parity of the frequency index.
//   acq_code (per channel, once): same for the zero-padded +-1 replica.
//   acq_corr (per channel x Doppler bin): for every iteration, X*conj(C) on
//            load, inverse FFT of the even-index and odd-index halves,
//            y[k] = E[k] + w^-k O[k], |y|^2/L^2 added to fp64 accumulators that
//            live in registers across the iterations; after each iteration
//            the row statistics checkacquisition() needs are reduced in the
//            workgroup.  P only leaves the chip when the caller asks for it.
//   acq_final (per channel): the decision of checkacquisition() after each
//            iteration, first success wins (ref src/sdracq.c:39-42).
//
// Coherent integration (gnsscorr_acq_set_coherent): a channel with ncoh > 1 has intg / ncoh groups
// where the text above and below says iterations.  acq_fwd wipes the group's (ncoh + 1)*nsamp samples off with one
// carrier walk and adds its ncoh windows of 2*nsamp samples, nsamp apart, as integers before the transform -- the
// transforms are linear, so that is the coherent sum of the ncoh correlation results; acq_code, acq_corr and the row
// statistics do not know, acq_final scales iters and cn0.  ncoh = 1 is the reference's integration bit for bit.
//
// Bit-edge hypotheses (gnsscorr_acq_set_bitedge): a channel with estep > 0 has H = ceil(ncoh / estep)
// sums per group, hypothesis h = 0, estep, ... negating the windows j >= h.  acq_fwd transforms all of them (X's slot =
// group * H + hypothesis index).  acq_corr's EDGE instance runs a group's inverse transforms once per hypothesis into a
// sink that keeps only the row's maximum, then once more for the hypothesis with the largest one (lowest h on ties)
// into the power accumulators: that row alone is added.  Channels without hypotheses run the instances they always ran,
// in a launch of their own.
//
// Carrier refinement (gnsscorr_acq_set_refine): a listed channel with nref > 0 that acq_final acquired
// gets, behind it, the nref prompt correlations from its buffloc on at the bin centre (acq_fine_nco, acq_prompt) and a
// line search over their squares (acq_fine); both hand-overs then start from that frequency.  No result row is
// written, and a search without such a channel queues none of the three.
//
// Code-Doppler compensation (gnsscorr_acq_set_codedoppler): a channel with a carrier f_cf reads group g
// of bin b s(b, g) samples later (gc_acq_shifts: a host table per grid), so that every group of a bin sees the code at
// the lag it had in group 0; the search is the search at write position wrpos - back, which is what the kernels are
// handed.  acq_fwd's CDOP instances add the table entry to the window origin; nothing behind them knows.  Not included:
// drift inside a group, a codefreq preset at hand-over, the drop-in sdracquisition(), the sharded engine.
//
// Every run works on a channel list (gnsscorr_acq_run_subset; gnsscorr_acq_run is the list 0..nch-1): the
// per-channel kernels take their channel from a compacted device list, acq_fwd its frequency grid from the
// list of grids that have a listed channel, so grid sizes follow the list.  Everything a channel owns (code
// spectrum, rows, arrival counters, result) stays indexed by the channel itself: what a listed channel computes
// does not depend on who else is listed.
//
// Stated once: the carrier LUT, a span's ring positions and a sample's wipe-off (gc_span_pos, gc_wipeoff: gnsscorr_lut.h);
// a span's carrier table, that table into LDS, the replica sample (acq_span_table, acq_table_to_lds, acq_replica); where a
// row, an X slot, a code spectrum, a prompt pair and the sections of d_list and arrive are (GcAcqDims, GcAcq:
// gnsscorr_ctx.h).  A search is gc_acq_run_list: its plan, the upload, the search's queue and the refinement's.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "gnsscorr_ctx.h"
#include "gnsscorr_fft.h"
#include "gnsscorr_lut.h"

#define GC_L       32768
#define GC_LH       16384

using gcfft::cadd;
using gcfft::cmul;
using gcfft::cmulc;
using gcfft::csub;

#define GC_ACQ_CARLDS (((GC_NCAR * 4 + 15) & ~15) + GC_NCAR * (int)sizeof(GcCarSeg))

namespace {

// iterations of a channel's search: groups of ncoh code periods
__host__ __device__ __forceinline__ int acq_groups(const GcChan &c) { return c.ncoh > 1 ? c.intg / c.ncoh : c.intg; }
// bit-edge hypotheses of a group: h = 0, estep, 2 estep, ... < ncoh (one, h = 0, without them)
__host__ __device__ __forceinline__ int acq_hyps(const GcChan &c) { return c.estep > 0 ? (c.ncoh + c.estep - 1) / c.estep : 1; }

__global__ void tw64_init_kernel(float2 *tw64p1, float2 *tw64p3)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= GC_LH) return;
    double s, c;
    sincospi(-2.0 * (double)gcfft::freq_of(t) / 65536.0, &s, &c);
    tw64p1[t] = make_float2((float)c, (float)s);
    sincospi(-2.0 * 3.0 * (double)gcfft::freq_of(t) / 65536.0, &s, &c);
    tw64p3[t] = make_float2((float)c, (float)s);
}

__global__ void tw_init_kernel(float2 *tw16k, float2 *tw32k, float2 *tw32p)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= GC_LH) return;
    double s, c;
    sincospi(-2.0 * (double)t / 16384.0, &s, &c);
    tw16k[t] = make_float2((float)c, (float)s);
    sincospi(-2.0 * (double)t / 32768.0, &s, &c);
    tw32k[t] = make_float2((float)c, (float)s);
    sincospi(-2.0 * (double)gcfft::freq_of(t) / 32768.0, &s, &c);
    tw32p[t] = make_float2((float)c, (float)s);
}

// four adjacent float2 (a butterfly's pass-order positions p..p+3) as two 16-byte accesses
__device__ __forceinline__ void st4(float2 *dst, float2 x0, float2 x1, float2 x2, float2 x3)
{
    float4 *d = reinterpret_cast<float4 *>(dst);
    d[0] = make_float4(x0.x, x0.y, x1.x, x1.y);
    d[1] = make_float4(x2.x, x2.y, x3.x, x3.y);
}
__device__ __forceinline__ void ld4(const float2 *src, float2 (&v)[4])
{
    const float4 *d = reinterpret_cast<const float4 *>(src);
    const float4 a = d[0], b = d[1];
    v[0] = make_float2(a.x, a.y); v[1] = make_float2(a.z, a.w);
    v[2] = make_float2(b.x, b.y); v[3] = make_float2(b.z, b.w);
}

// Forward 32768-point transform of a sequence given by a per-sample functor, decimated in time:
// Ee = FFT16k(x[2j]), Oo = FFT16k(x[2j+1]), X[f] = Ee[f] + w^f Oo[f], X[f + 16384] = Ee[f] - w^f Oo[f]
// (w = exp(-2 pi i/32768), f < 16384).  out[0][p] / out[1][p] = X[f(p)] / X[f(p) + 16384], p in pass
// order: exactly the pairs the inverse transform of the correlation wants side by side (acq_corr).
// Ee waits in out[0] while Oo is computed (each lane reads back what it wrote itself).
template <class F>
__device__ __forceinline__ void fwd32k_store(F sample, float2 *lds, const float2 *__restrict__ tw16k,
                                             const float2 *__restrict__ tw32p, float2 *__restrict__ out,
                                             int tid)
{
    gcfft::dif<-1>([&](int j) { return sample(2 * j); },
                   [out](int p, float2 x0, float2 x1, float2 x2, float2 x3) { st4(out + p, x0, x1, x2, x3); },
                   lds, tw16k, tid);
    __syncthreads();
    gcfft::dif<-1>([&](int j) { return sample(2 * j + 1); },
                   [out, tw32p](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
                       float2 e[4], t[4];
                       ld4(out + p, e);
                       ld4(tw32p + p, t);
                       const float2 o[4] = {cmul(x0, t[0]), cmul(x1, t[1]), cmul(x2, t[2]), cmul(x3, t[3])};
                       st4(out + p, cadd(e[0], o[0]), cadd(e[1], o[1]), cadd(e[2], o[2]), cadd(e[3], o[3]));
                       st4(out + GC_LH + p, csub(e[0], o[0]), csub(e[1], o[1]), csub(e[2], o[2]), csub(e[3], o[3]));
                   },
                   lds, tw16k, tid);
}

// Forward 65536-point transform (code periods of 16385..32768 samples: 20 / 26 Msps front ends, ref
// frontend/stereo_L1G1.ini), decimated in time by four: E_r = FFT16k(x[4j + r]),
//     X[f + 16384 q] = sum_r (-i)^(r q) w^(r f) E_r[f],   w = exp(-2 pi i/65536), f < 16384,
// stored as out[q][p] (p = pass position of f): the four values the inverse transform wants side by side.
// With a_r = w^(r f) E_r:  P+- = E_0 +- a_2, Q+- = a_1 +- a_3,
//     X_0 = P+ + Q+,  X_2 = P+ - Q+,  X_1 = P- - i Q-,  X_3 = P- + i Q-.
// The partial results wait in `out` between the four sub-transforms (each lane reads back what it wrote).
template <class F>
__device__ __forceinline__ void fwd64k_store(F sample, float2 *lds, const float2 *__restrict__ tw16k,
                                             const float2 *__restrict__ tw32p, const float2 *__restrict__ tw64p1,
                                             const float2 *__restrict__ tw64p3, float2 *__restrict__ out, int tid)
{
    // r = 0: E_0 -> out[0]
    gcfft::dif<-1>([&](int j) { return sample(4 * j); },
                   [&](int p, float2 x0, float2 x1, float2 x2, float2 x3) { st4(out + p, x0, x1, x2, x3); },
                   lds, tw16k, tid);
    __syncthreads();
    // r = 2: P+ -> out[0], P- -> out[1]
    gcfft::dif<-1>([&](int j) { return sample(4 * j + 2); },
                   [&](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
                       float2 e[4], t[4];
                       ld4(out + p, e);
                       ld4(tw32p + p, t);
                       const float2 a[4] = {cmul(x0, t[0]), cmul(x1, t[1]), cmul(x2, t[2]), cmul(x3, t[3])};
                       st4(out + p, cadd(e[0], a[0]), cadd(e[1], a[1]), cadd(e[2], a[2]), cadd(e[3], a[3]));
                       st4(out + GC_LH + p, csub(e[0], a[0]), csub(e[1], a[1]), csub(e[2], a[2]), csub(e[3], a[3]));
                   },
                   lds, tw16k, tid);
    __syncthreads();
    // r = 1: a_1 -> out[2]
    gcfft::dif<-1>([&](int j) { return sample(4 * j + 1); },
                   [&](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
                       float2 t[4];
                       ld4(tw64p1 + p, t);
                       st4(out + 2 * GC_LH + p, cmul(x0, t[0]), cmul(x1, t[1]), cmul(x2, t[2]), cmul(x3, t[3]));
                   },
                   lds, tw16k, tid);
    __syncthreads();
    // r = 3: the four outputs
    gcfft::dif<-1>([&](int j) { return sample(4 * j + 3); },
                   [&](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
                       float2 t[4], a1[4], pp[4], pm[4];
                       ld4(tw64p3 + p, t);
                       ld4(out + 2 * GC_LH + p, a1);
                       ld4(out + p, pp);
                       ld4(out + GC_LH + p, pm);
                       const float2 a3[4] = {cmul(x0, t[0]), cmul(x1, t[1]), cmul(x2, t[2]), cmul(x3, t[3])};
                       float2 X0[4], X1[4], X2[4], X3[4];
#pragma unroll
                       for (int i = 0; i < 4; i++) {
                           const float2 qp = cadd(a1[i], a3[i]), qm = csub(a1[i], a3[i]);
                           const float2 iqm = make_float2(-qm.y, qm.x);            // i Q-
                           X0[i] = cadd(pp[i], qp);
                           X2[i] = csub(pp[i], qp);
                           X1[i] = csub(pm[i], iqm);
                           X3[i] = cadd(pm[i], iqm);
                       }
                       st4(out + p, X0[0], X0[1], X0[2], X0[3]);
                       st4(out + GC_LH + p, X1[0], X1[1], X1[2], X1[3]);
                       st4(out + 2 * GC_LH + p, X2[0], X2[1], X2[2], X2[3]);
                       st4(out + 3 * GC_LH + p, X3[0], X3[1], X3[2], X3[3]);
                   },
                   lds, tw16k, tid);
}

// ---- what the kernels below share: a span's carrier table, its samples in the ring, the replica ----------------------
// The carrier piece table of a span of `samples` samples at `freq`, phase 0 at its first sample (ref src/sdrcmn.c:761),
// by one lane.  A span that needs more pieces than the table holds has none (n = 0) and is counted in *overflow.
__device__ __forceinline__ void acq_span_table(GcAcqCar *t, double freq, double ti, int samples, int *overflow)
{
    GcCarTable ct{t->k0, t->seg, GC_NCAR, 0, 0};
    gc_carrier_walk(gc_carrier_phis(0.0), gc_carrier_ps(freq, ti), samples, ct);
    t->n = ct.overflow ? 0 : ct.n;
    if (ct.overflow) atomicAdd(overflow, 1);
}
// that table into the workgroup's LDS, a piece per lane; returns the number of pieces (a barrier follows)
__device__ __forceinline__ int acq_table_to_lds(const GcAcqCar *gt, int *lk0, GcCarSeg *lseg, int tid)
{
    const int ncar = gt->n;
    if (tid < ncar) { lk0[tid] = gt->k0[tid]; lseg[tid] = gt->seg[tid]; }
    return ncar;
}
// Sample s of the replica rescode(code, clen, 0, 0, ci, nsamp) (ref src/sdrinit.c:650-651), ci = __dmul_rn(ti, crate)
// (sdr->ci, ref src/sdrinit.c:605): acq_code transforms it, acq_prompt correlates with it
__device__ __forceinline__ int acq_replica(gc_gptr_i8 code, int clen, double ci, int s)
{
    long long t = (long long)__dmul_rn((double)s, ci);
    while (t >= clen) t -= clen;
    return code[(int)t];
}

// one lane per (grid, bin): the carrier table of the bin's wipe-off span
__global__ void acq_nco_kernel(const GcChan *__restrict__ chan, const int *__restrict__ grid_chan,
                               const double *__restrict__ freqs, GcAcqCar *__restrict__ car, int ngrid, int maxfreq,
                               int *__restrict__ overflow)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ngrid * maxfreq) return;
    const GcChan &c = chan[grid_chan[i / maxfreq]];
    const int bin = i % maxfreq;
    if (bin >= c.nfreq) { car[i].n = 0; return; }
    acq_span_table(car + i, freqs[c.freq_off + bin], c.ti, (c.ncoh + 1) * c.nsamp, overflow);
}

// acq_fwd: grid (bin, slot, entry of the list of frequency grids in use); slot = iteration without hypotheses.  COH:
// some listed grid integrates coherently, and the sample functor adds the group's ncoh windows (for a grid with ncoh = 1
// that is the same integer, so the same float); the instance without COH is free of the loop.  EDGE (with COH): some
// listed grid has bit-edge hypotheses; slot = iteration * H + hypothesis index, and the functor subtracts the windows
// j >= h of hypothesis h > 0 (a grid without hypotheses has H = 1, h = 0: the same integers again).  CDOP (with COH;
// DESIGN.md 3.2f): some channel compensates code Doppler; the window of (bin, iteration) starts shifts[grid][bin][iteration]
// samples later, one scalar load (a grid without compensation has a row of zeros: the same samples again).
template <bool COH, bool EDGE = false, bool CDOP = false>
__global__ __launch_bounds__(GC_FFT_THREADS) void acq_fwd_kernel(
    const GcChan *__restrict__ chan, const int *__restrict__ grid_chan, const int *__restrict__ glist,
    const GcAcqCar *__restrict__ car,
    const uint64_t *__restrict__ grid_wrpos, const float2 *__restrict__ tw16k,
    const float2 *__restrict__ tw32p, const float2 *__restrict__ tw64p1, const float2 *__restrict__ tw64p3,
    float2 *__restrict__ X, int maxfreq, int maxslot, int L, const int32_t *__restrict__ shifts, int maxintg)
{
    static_assert(COH || !EDGE, "hypotheses belong to coherent groups");
    static_assert(COH || !CDOP, "compensated grids run the coherent instances");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    const GcAcqDims d = {maxfreq, 0, maxslot, L};       // (scalar arguments, as acq_corr; no rows here)
    const int bin = blockIdx.x, slot = blockIdx.y, g = glist[blockIdx.z], tid = threadIdx.x;
    const GcChan &c = chan[grid_chan[g]];
    const int ncoh = COH ? c.ncoh : 1;
    int it = slot, hneg = ncoh;         // hneg: the first window that is subtracted (ncoh: none)
    if constexpr (EDGE) {
        const int H = acq_hyps(c);
        it = slot / H;
        const int h = (slot - it * H) * c.estep;
        if (h > 0) hneg = h;
    }
    if (bin >= c.nfreq || it >= (COH ? acq_groups(c) : c.intg)) return;
    const int n = c.nsamp, n2 = 2 * n, dtype = c.dtype;
    // window of iteration `it`: ref src/sdracq.c:24-32; a group starts ncoh windows after the one before
    uint64_t buffloc = grid_wrpos[g] - (uint64_t)(c.intg + 1) * n + (uint64_t)it * ((uint64_t)ncoh * n);
    // (grid_wrpos is `back` short of the write position, and s(b, 0) = 0: the sum stays inside what the ring holds)
    if constexpr (CDOP) buffloc += (uint64_t)(int64_t)shifts[((size_t)g * maxfreq + bin) * maxintg + it];
    const uint64_t base = buffloc % c.ringlen;
    const gc_gptr_i8 ring = (gc_gptr_i8)c.ring;
    const uint64_t ringlen = c.ringlen;
    // the bin's carrier table (phase starts at 0 for every bin and iteration, :761) behind the FFT image: acq_table_to_lds
    // and, below, gc_wipeoff's look-up and arithmetic spelled out, which this kernel's register budget needs
    int *lk0 = reinterpret_cast<int *>(smem + GC_FFT_LDS + 256);
    GcCarSeg *lseg = reinterpret_cast<GcCarSeg *>(smem + GC_FFT_LDS + 256 + ((GC_NCAR * 4 + 15) & ~15));
    const GcAcqCar *gt = car + (size_t)g * d.maxfreq + bin;
    const int ncar = gt->n;
    if (tid < ncar) { lk0[tid] = gt->k0[tid]; lseg[tid] = gt->seg[tid]; }
    __syncthreads();
    const float sc = (float)((1.0 / 32.0) / (double)c.nfft);     // CSCALE/m, ref src/sdrcmn.c:764

    // wiped-off sample s of the group's span, loaded byte by byte
    auto mixed = [&](int s, int &I, int &Q) {
        const uint64_t pos = gc_span_pos(base, s, ringlen);
        const int idx = gc_carrier_idx_at(lk0, lseg, ncar, s);
        const int cs_ = gcCos32[idx], sn_ = gcSin32[idx];
        if (dtype == 2) {
            const int d0 = ring[2 * pos], d1 = ring[2 * pos + 1];
            I = cs_ * d0 - sn_ * d1;
            Q = sn_ * d0 + cs_ * d1;
        } else {
            const int d0 = ring[pos];
            I = cs_ * d0;
            Q = sn_ * d0;
        }
    };
    auto sample = [&](int s) -> float2 {
        if (s >= n2) return make_float2(0.f, 0.f);
        int I, Q;
        mixed(s, I, Q);
        if constexpr (COH) {
            // z[s] = sum over the windows j < ncoh of (I, Q)[j n + s]: |z| <= 20 * 2 * 32 * 128 < 2^24, exact as a float
            for (int j = 1; j < ncoh; j++) {
                int Ij, Qj;
                mixed(j * n + s, Ij, Qj);
                if (EDGE && j >= hneg) { Ij = -Ij; Qj = -Qj; }       // s(h, j)
                I += Ij;
                Q += Qj;
            }
        }
        return make_float2((float)I * sc, (float)Q * sc);
    };
    float2 *out = d.x(X, g, slot, bin);
    if (d.L == 2 * GC_L) fwd64k_store(sample, lds, tw16k, tw32p, tw64p1, tw64p3, out, tid);
    else fwd32k_store(sample, lds, tw16k, tw32p, out, tid);
}

// acq_code: grid (channel)
__global__ __launch_bounds__(GC_FFT_THREADS) void acq_code_kernel(
    const GcChan *__restrict__ chan, const float2 *__restrict__ tw16k, const float2 *__restrict__ tw32p,
    const float2 *__restrict__ tw64p1, const float2 *__restrict__ tw64p3, float2 *__restrict__ C, GcAcqDims d)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    const int ch = blockIdx.x, tid = threadIdx.x;
    const GcChan &c = chan[ch];
    const int n = c.nsamp, clen = c.clen;
    const double ci = __dmul_rn(c.ti, c.crate);
    const gc_gptr_i8 code = (gc_gptr_i8)c.code;
    // the replica, zero-padded
    auto sample = [&](int s) -> float2 {
        if (s >= n) return make_float2(0.f, 0.f);
        return make_float2((float)acq_replica(code, clen, ci, s), 0.f);
    };
    if (d.L == 2 * GC_L) fwd64k_store(sample, lds, tw16k, tw32p, tw64p1, tw64p3, d.code(C, ch), tid);
    else fwd32k_store(sample, lds, tw16k, tw32p, d.code(C, ch), tid);
}

// ---- workgroup reductions used by acq_corr --------------------------------
struct MaxIdx { double v; int k; };

__device__ __forceinline__ MaxIdx better(MaxIdx a, MaxIdx b)
{   // larger value wins, first index on ties (maxvd's strict '<', ref src/sdrcmn.c:461-476)
    return (b.v > a.v || (b.v == a.v && b.k < a.k)) ? b : a;
}

template <int NT>
__device__ __forceinline__ MaxIdx wg_argmax(MaxIdx m, double *sd, int *si, int tid)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MaxIdx t;
        t.v = __shfl_xor(m.v, o, 64);
        t.k = __shfl_xor(m.k, o, 64);
        m = better(m, t);
    }
    __syncthreads();
    if ((tid & 63) == 0) { sd[tid >> 6] = m.v; si[tid >> 6] = m.k; }
    __syncthreads();
    MaxIdx r; r.v = sd[0]; r.k = si[0];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) { MaxIdx t; t.v = sd[w]; t.k = si[w]; r = better(r, t); }
    return r;
}

template <int NT>
__device__ __forceinline__ void wg_sum_max(double &s, double &m, double *sd, int tid)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        m = fmax(m, __shfl_xor(m, o, 64));
    }
    __syncthreads();
    if ((tid & 63) == 0) { sd[tid >> 6] = s; sd[16 + (tid >> 6)] = m; }
    __syncthreads();
    s = sd[0]; m = sd[16];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) { s += sd[w]; m = fmax(m, sd[16 + w]); }
}

// Row statistics for checkacquisition() (ref src/sdracq.c:71-95) of the power row a workgroup of NT lanes holds in
// registers, lane `tid` owning lag lag_of(tid, s) in P[s] (lags >= n are not part of the row): the maximum and its
// lag (first index on ties), and, outside the window of +-nsc2 samples (2 chips, wrapping) around it, the sum and
// the maximum -- for which element 0 always is a candidate: it seeds maxvd().  Two workgroup reductions (wg_argmax,
// then wg_sum_max); every lane returns the row.
template <int NT, int NP, class LagOf>
__device__ __forceinline__ GcAcqRow acq_row_stats(const double (&P)[NP], LagOf lag_of, int n, int nsc2, double *sd,
                                                  int *si, int tid)
{
    MaxIdx m; m.v = -1.0; m.k = 0x7fffffff;
#pragma unroll
    for (int s = 0; s < NP; s++) {
        const int k = lag_of(tid, s);
        if (k < n) { MaxIdx t; t.v = P[s]; t.k = k; m = better(m, t); }
    }
    m = wg_argmax<NT>(m, sd, si, tid);
    int exs = m.k - nsc2; if (exs < 0) exs += n;
    int exe = m.k + nsc2; if (exe >= n) exe -= n;
    double so = 0.0, mo = -1.0;
#pragma unroll
    for (int s = 0; s < NP; s++) {
        const int k = lag_of(tid, s);
        if (k < n) {
            const bool outside = (exs <= exe) ? (k < exs || k > exe) : (k < exs && k > exe);
            if (outside) so += P[s];
            if (outside || k == 0) mo = fmax(mo, P[s]);    // element 0 seeds maxvd()
        }
    }
    wg_sum_max<NT>(so, mo, sd, tid);
    GcAcqRow r;
    r.rowmax = m.v; r.sum_out = so; r.max_out = mo; r.argmax = m.k; r.edge = 0;
    return r;
}

// The decision of one iteration, taken by a wavefront from the rows of the channel's nfreq bins: the best row is the
// one with the largest rowmax, lowest bin on ties (every lane returns it); the channel is acquired when that row's
// peak ratio passes ACQTH (ref src/sdr.h:148, src/sdracq.c:39-42).
__device__ __forceinline__ int acq_best_row(const GcAcqRow *row, int nfreq, int lane)
{
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int b = lane; b < nfreq; b += 64) {
        const double v = row[b].rowmax;
        if (v > bv) { bv = v; bi = b; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(bv, d);
        const int oi = __shfl_xor(bi, d);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi;
}

__device__ __forceinline__ bool acq_passes(const GcAcqRow &w) { return w.rowmax / w.max_out > 3.0; }

// X[f + 16384 q], C[f + 16384 q] (q < Q) at the four pass-order positions of a butterfly, as loaded; with the
// positions' twiddles behind them
template <int Q> struct RawXC { float4 x[Q][2], c[Q][2]; };
template <int Q> struct RawXCT { RawXC<Q> r; float4 ta, tb; };
template <int Q> __device__ __forceinline__ const RawXC<Q> &acq_raw(const RawXC<Q> &r) { return r; }
template <int Q> __device__ __forceinline__ const RawXC<Q> &acq_raw(const RawXCT<Q> &t) { return t.r; }

template <int Q>
__device__ __forceinline__ RawXC<Q> acq_load(const float2 *Xb, const float2 *Cc, int p)
{
    RawXC<Q> r;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        r.x[q][0] = *reinterpret_cast<const float4 *>(Xb + q * GC_LH + p);
        r.x[q][1] = *reinterpret_cast<const float4 *>(Xb + q * GC_LH + p + 2);
        r.c[q][0] = *reinterpret_cast<const float4 *>(Cc + q * GC_LH + p);
        r.c[q][1] = *reinterpret_cast<const float4 *>(Cc + q * GC_LH + p + 2);
    }
    return r;
}
template <int Q>
__device__ __forceinline__ RawXCT<Q> acq_load_tw(const float2 *Xb, const float2 *Cc, const float2 *twp, int p)
{
    RawXCT<Q> t;
    t.r = acq_load<Q>(Xb, Cc, p);
    t.ta = *reinterpret_cast<const float4 *>(twp + p);
    t.tb = *reinterpret_cast<const float4 *>(twp + p + 2);
    return t;
}
// Y[f + 16384 q] = X conj(C) at position k (0..3) of the butterfly, and that position's twiddle
template <int Q>
__device__ __forceinline__ float2 acq_y(const RawXC<Q> &r, int q, int k)
{
    const float4 xv = r.x[q][k >> 1], cv = r.c[q][k >> 1];
    return (k & 1) ? cmulc(make_float2(xv.z, xv.w), make_float2(cv.z, cv.w))
                   : cmulc(make_float2(xv.x, xv.y), make_float2(cv.x, cv.y));
}
template <int Q>
__device__ __forceinline__ float2 acq_w(const RawXCT<Q> &t, int k)
{
    const float4 v = k < 2 ? t.ta : t.tb;
    return (k & 1) ? make_float2(v.z, v.w) : make_float2(v.x, v.y);
}

// dit() sink: |y|^2/L^2 of the lags a transform ends in (of a lane's outputs o + 1024 q those with q < 8: lags below
// nsamp) onto the fp64 accumulators P[OFF + 8 h + q] (ref src/sdrcmn.c:244-246 with the m-point scaling folded)
template <int OFF, int NP>
__device__ __forceinline__ auto acq_add_power(double (&P)[NP], float invL2)
{
    return [&P, invL2](int h, int, float2 (&a)[16]) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float pw = fmaf(a[q].x, a[q].x, a[q].y * a[q].y) * invL2;
            P[OFF + 8 * h + q] += (double)pw;
        }
    };
}

// dit() sink of a hypothesis's first pass: the same |y|^2/L^2 values, of which only the lane's maximum over the lags
// 2 (o + 1024 q) + PAR < n is kept
template <int PAR>
__device__ __forceinline__ auto acq_max_power(float &mx, float invL2, int n)
{
    return [&mx, invL2, n](int, int o, float2 (&a)[16]) {
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float pw = fmaf(a[q].x, a[q].x, a[q].y * a[q].y) * invL2;
            if (2 * (o + 1024 * q) + PAR < n) mx = fmaxf(mx, pw);
        }
    };
}

// the workgroup's maximum of a float (sf: one slot per wavefront; every lane returns it)
template <int NT>
__device__ __forceinline__ float wg_maxf(float m, float *sf, int tid)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) sf[tid >> 6] = m;
    __syncthreads();
    float r = sf[0];
#pragma unroll
    for (int w = 1; w < NT / 64; w++) r = fmaxf(r, sf[w]);
    return r;
}

// the bin's power row, from the registers to Pout[bin][lag]
template <int NP, class LagOf>
__device__ __forceinline__ void acq_write_power(double *__restrict__ Pout, const double (&P)[NP], LagOf lag_of,
                                                int tid, int bin, int n)
{
#pragma unroll
    for (int s = 0; s < NP; s++) {
        const int k = lag_of(tid, s);
        if (k < n) Pout[(size_t)bin * n + k] = P[s];
    }
}

// dynamic LDS of the correlation kernels: the FFT image, then the reductions' scratch (32 doubles sd, 16 ints si),
// in the 256-byte units of the other FFT kernels' sizes
#define GC_ACQ_SD       GC_FFT_LDS
#define GC_ACQ_SI       (GC_ACQ_SD + 32 * (int)sizeof(double))
#define GC_ACQ_CORR_LDS ((GC_ACQ_SI + 16 * (int)sizeof(int) + 255) & ~255)

#define GC_ACQ_G 4              // channels that share an XCD's forward spectra (acq_corr_kernel)

// Block order of acq_corr_kernel.  Blocks b and b + 8 tend to share an XCD (speed only).  Search: XCD `slot` takes
// the bins slot, slot + 8, ... of GC_ACQ_G channels at a time: the ~9 spectra X[iteration][bin] it needs per
// iteration (2.3 MB) and the G code spectra (1 MB) fit its 4 MB L2, so a spectrum leaves the Infinity Cache (which
// holds all of them, 186 MB) once per G channels (and both lag parities) instead of once per channel and parity;
// chip-wide the G channels' bins all run side by side and reach the end of each iteration together, which is what
// lets a channel stop at the iteration that acquires it.  Pout (one channel's power array): block = bin.
// A block whose bin or list entry does not exist (bin >= nbins, li >= nlist) has nothing to do.
struct AcqBlock { int bin, li; };       // Doppler bin, entry of the channel list

__device__ __forceinline__ AcqBlock acq_corr_block(int b, int nbins, bool pout)
{
    constexpr int G = GC_ACQ_G;
    const int slot = b & 7, qq = b >> 3;
    const int bpx = (nbins + 7) >> 3;                   // bins per XCD slot
    const int grp = qq / (bpx * G), rem = qq - grp * (bpx * G);
    AcqBlock r;
    r.bin = pout ? qq * 8 + slot : (rem / G) * 8 + slot;
    r.li = grp * G + rem % G;
    return r;
}
// its grid: 8 slots x bins per slot (x the listed channels in whole groups of G)
unsigned acq_corr_blocks(int nbins, int nlist, bool pout)
{
    const unsigned per_channel = 8u * (unsigned)((nbins + 7) / 8);
    return pout ? per_channel : per_channel * (unsigned)(GC_ACQ_G * ((nlist + GC_ACQ_G - 1) / GC_ACQ_G));
}

// Block order of acq_corr64_kernel.  Search: slot = list entry within a round of 8, the rounds' bins consecutive.
// Pout: block = bin.
__device__ __forceinline__ AcqBlock acq_corr64_block(int b, int nbins, bool pout)
{
    const int slot = b & 7, qq = b >> 3;
    AcqBlock r;
    r.bin = pout ? qq * 8 + slot : qq % nbins;
    r.li = (qq / nbins) * 8 + slot;
    return r;
}
// its grid: (rounds of 8 list entries) x bins x 8 slots
unsigned acq_corr64_blocks(int nbins, int nlist, bool pout)
{
    return pout ? 8u * (unsigned)((nbins + 7) / 8) : 8u * (unsigned)((nlist + 7) / 8) * (unsigned)nbins;
}

// acq_corr: one workgroup of NT lanes per (bin, channel).
// y = IFFT_L(Y), Y = X conj(C) (ref src/sdrcmn.c:236-246; the reference's extra minus sign vanishes
// under |.|^2), split by lag parity so that each 16384-point transform ends in final values:
//   y[2j]   = IFFT_16k( Y[f] + Y[f + L/2] )[j]
//   y[2j+1] = IFFT_16k( (Y[f] - Y[f + L/2]) exp(+2 pi i f/L) )[j],   f < L/2.
// Lags k < nsamp <= 16384 are wanted, i.e. j < 8192: of a lane's outputs j = o + 1024 q those with
// q < 8.  Nothing has to wait for the other transform, so the only long-lived registers are the
// power accumulators.
// EDGE: every channel of the launch has bit-edge hypotheses, H >= 2 spectra per (iteration, bin) in
// X's slots iteration * H + i.  Two passes per iteration: the transform pair of every hypothesis into acq_max_power
// and a workgroup maximum, then the pair of the hypothesis with the largest row maximum (lowest on ties) into the
// accumulators -- H + 1 pairs, a few floats of state, no second row in registers.  The row record carries the choice.
template <int NT, bool EDGE = false>
__global__ __launch_bounds__(NT) void acq_corr_kernel(
    const GcChan *__restrict__ chan, const float2 *__restrict__ tw16k, const float2 *__restrict__ tw32p,
    const float2 *__restrict__ X, const float2 *__restrict__ C, const int *__restrict__ iters,
    GcAcqRow *rows, double *__restrict__ Pout, int pout_ch, int maxfreq, int maxintg, int maxslot,
    const int *__restrict__ list, int nlist, int *arrive, int *done)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    double *sd = reinterpret_cast<double *>(smem + GC_ACQ_SD);
    int *si = reinterpret_cast<int *>(smem + GC_ACQ_SI);
    const int tid0 = threadIdx.x;
    // (scalar arguments: the argument block this kernel's register budget was tuned with; L is the kernel's own constant)
    const GcAcqDims d = {maxfreq, maxintg, maxslot, GC_L};
    const AcqBlock blk = acq_corr_block(blockIdx.x, d.maxfreq, Pout != nullptr);
    const int bin = blk.bin;
    if (bin >= d.maxfreq || (!Pout && blk.li >= nlist)) return;
    const int ch = Pout ? pout_ch : list[blk.li];
    const GcChan &c = chan[ch];
    if (bin >= c.nfreq) return;
    const int n = c.nsamp, nit = iters[ch], nsc2 = 2 * c.nsampchip;
    const float2 *Cc = d.code(C, ch);
    const float invL2 = 1.0f / ((float)GC_L * (float)GC_L);

    // lane `tid` owns lags k = 2 (tid + NT*h + 1024*q) + par (par < 2, h < 1024/NT, q < 8):
    // register index s = NPH*par + 8*h + q
    constexpr int NPH = 8 * (1024 / NT), NP = 2 * NPH;
    constexpr int CHUNK = 2;                       // butterflies whose operands are in flight together
    double P[NP];
#pragma unroll
    for (int s = 0; s < NP; s++) P[s] = 0.0;
    auto lag_of = [](int tid, int s) { return 2 * (tid + NT * ((s % NPH) >> 3) + 1024 * (s & 7)) + s / NPH; };

    // the two inverse transforms of the spectrum at Xb, their results to the sinks of the even and of the odd lags
    auto inverse = [&](const float2 *Xb, int &tid, auto sink_even, auto sink_odd) {
        // even lags
        gcfft::dit<+1, NT, CHUNK>([Xb, Cc](int p) { return acq_load<2>(Xb, Cc, p); },
                       [](const RawXC<2> &r, float2 &x0, float2 &x1, float2 &x2, float2 &x3) {
                           x0 = cadd(acq_y(r, 0, 0), acq_y(r, 1, 0));
                           x1 = cadd(acq_y(r, 0, 1), acq_y(r, 1, 1));
                           x2 = cadd(acq_y(r, 0, 2), acq_y(r, 1, 2));
                           x3 = cadd(acq_y(r, 0, 3), acq_y(r, 1, 3));
                       },
                       sink_even, lds, tw16k, tid);
        __syncthreads();
        asm volatile("" : "+v"(tid));            // (as below: the second transform recomputes its addresses)
        // odd lags; exp(+2 pi i f/L) = conj of the forward twiddle
        gcfft::dit<+1, NT, CHUNK>([Xb, Cc, tw32p](int p) { return acq_load_tw<2>(Xb, Cc, tw32p, p); },
                       [](const RawXCT<2> &t, float2 &x0, float2 &x1, float2 &x2, float2 &x3) {
                           x0 = cmulc(csub(acq_y(t.r, 0, 0), acq_y(t.r, 1, 0)), acq_w(t, 0));
                           x1 = cmulc(csub(acq_y(t.r, 0, 1), acq_y(t.r, 1, 1)), acq_w(t, 1));
                           x2 = cmulc(csub(acq_y(t.r, 0, 2), acq_y(t.r, 1, 2)), acq_w(t, 2));
                           x3 = cmulc(csub(acq_y(t.r, 0, 3), acq_y(t.r, 1, 3)), acq_w(t, 3));
                       },
                       sink_odd, lds, tw16k, tid);
    };
    const int H = EDGE ? acq_hyps(c) : 1;

    for (int it = 0; it < nit; it++) {
        // Opaque copy of the lane id: keeps the address computations of one iteration from being
        // hoisted out of the loop (they would be spilled to scratch, not kept in VGPRs).
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const float2 *Xb = d.x(X, c.grid, (size_t)it * H, bin);    // the iteration's first slot
        int hsel = 0;                            // index of the hypothesis whose row is added
        if constexpr (EDGE) {
            const size_t hstride = d.x_slot_stride();       // hypothesis hi is slot hi of the iteration
            float best = -1.0f;
            for (int hi = 0; hi < H; hi++) {
                float mx = -1.0f;
                inverse(Xb + hi * hstride, tid, acq_max_power<0>(mx, invL2, n), acq_max_power<1>(mx, invL2, n));
                mx = wg_maxf<NT>(mx, reinterpret_cast<float *>(sd), tid);       // (its barriers free the LDS image)
                if (mx > best) { best = mx; hsel = hi; }
                asm volatile("" : "+v"(tid));
            }
            Xb += hsel * hstride;
        }
        inverse(Xb, tid, acq_add_power<0>(P, invL2), acq_add_power<NPH>(P, invL2));

        GcAcqRow r = acq_row_stats<NT>(P, lag_of, n, nsc2, sd, si, tid);
        if constexpr (EDGE) r.edge = hsel * c.estep;
        if (tid == 0) *d.row(rows, ch, it, bin) = r;
        // The reference stops a channel at the first iteration whose peak ratio passes the threshold
        // (ref src/sdracq.c:39-42); so does this: the workgroup that finishes an iteration of its channel
        // last takes acq_final's decision from the same rows (acq_best_row, acq_passes), and the channel's
        // workgroups leave at the next iteration boundary they reach after it.  (Iterations past the
        // acquiring one are never looked at: what they would have written is not missed.)
        if (arrive && tid < 64) {
            int last = 0;
            if (tid == 0) {
                __threadfence();
                last = atomicAdd(d.arrival(arrive, ch, it), 1) == c.nfreq - 1;
            }
            last = __shfl(last, 0);
            if (last) {
                __threadfence();
                const GcAcqRow *row = d.row(rows, ch, it);
                const GcAcqRow w = row[acq_best_row(row, c.nfreq, tid)];
                if (tid == 0 && acq_passes(w))
                    __hip_atomic_store(&done[ch], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid == 0) si[15] = __hip_atomic_load(&done[ch], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();      // LDS image and reduction scratch are reused next iteration
        if (arrive && si[15]) break;
    }
    if (Pout) acq_write_power(Pout, P, lag_of, tid0, bin, n);
}

// acq_corr for the 65536-point transform: one workgroup of 512 lanes per (bin, channel).  The inverse
// transform split by lag mod 4 -- with F = f + 16384 q and k = 4 j + s,
//     y[4j + s] = IFFT_16k( w^(-f s) sum_q i^(q s) Y[f + 16384 q] )[j],   Y = X conj(C), w = exp(-2 pi i/65536)
// -- so that, as in the 32768-point kernel, every 16384-point transform ends in final lags and the
// only long-lived registers are the power accumulators: lane `tid` owns lags 4 (tid + 512 h + 1024 q) + s,
// h < 2, q < 8, s < 4 (lags below nsamp <= 32768), register index 16 s + 8 h + q.
__global__ __launch_bounds__(512) void acq_corr64_kernel(
    const GcChan *__restrict__ chan, const float2 *__restrict__ tw16k, const float2 *__restrict__ tw32p,
    const float2 *__restrict__ tw64p1, const float2 *__restrict__ tw64p3,
    const float2 *__restrict__ X, const float2 *__restrict__ C, const int *__restrict__ iters,
    GcAcqRow *__restrict__ rows, double *__restrict__ Pout, int pout_ch, int maxfreq, int maxintg,
    const int *__restrict__ list, int nlist)
{
    constexpr int NT = 512, L = 2 * GC_L, NP = 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    double *sd = reinterpret_cast<double *>(smem + GC_ACQ_SD);
    int *si = reinterpret_cast<int *>(smem + GC_ACQ_SI);
    const int tid0 = threadIdx.x;
    const GcAcqDims d = {maxfreq, maxintg, maxintg, L};     // (scalar arguments, as acq_corr; no hypotheses: GcAcqDims::x)
    const AcqBlock blk = acq_corr64_block(blockIdx.x, d.maxfreq, Pout != nullptr);
    const int bin = blk.bin;
    if (bin >= d.maxfreq || (!Pout && blk.li >= nlist)) return;
    const int ch = Pout ? pout_ch : list[blk.li];
    const GcChan &c = chan[ch];
    if (bin >= c.nfreq) return;
    const int n = c.nsamp, nit = iters[ch], nsc2 = 2 * c.nsampchip;
    const float2 *Cc = d.code(C, ch);
    const float invL2 = 1.0f / ((float)L * (float)L);
    double P[NP];
#pragma unroll
    for (int s = 0; s < NP; s++) P[s] = 0.0;
    auto lag_of = [](int tid, int s) { return 4 * (tid + 512 * ((s >> 3) & 1) + 1024 * (s & 7)) + (s >> 4); };
    for (int it = 0; it < nit; it++) {
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const float2 *Xb = d.x(X, c.grid, it, bin);         // (slot = iteration: no hypotheses at this length)
        // Lags 4 j + S.  The twiddle w^(-f S) = conj(twp[p]) (S > 0) has to be applied per input: dit() hands `make`
        // only the raw operands, so the twiddled residues fetch their factors with the operands.
        auto residue = [&](auto s_tag, const float2 *__restrict__ twp) {
            constexpr int S = decltype(s_tag)::value;
            auto make = [](const auto &t, float2 &x0, float2 &x1, float2 &x2, float2 &x3) {
                float2 z[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const RawXC<4> &r = acq_raw(t);
                    const float2 y0 = acq_y(r, 0, k), y1 = acq_y(r, 1, k), y2 = acq_y(r, 2, k), y3 = acq_y(r, 3, k);
                    if constexpr (S == 0) {
                        z[k] = cadd(cadd(y0, y2), cadd(y1, y3));
                    } else {
                        float2 v;
                        if (S == 2) v = csub(cadd(y0, y2), cadd(y1, y3));
                        else {
                            const float2 d = csub(y1, y3), id = make_float2(-d.y, d.x);      // i (y1 - y3)
                            v = S == 1 ? cadd(csub(y0, y2), id) : csub(csub(y0, y2), id);
                        }
                        z[k] = cmulc(v, acq_w(t, k));      // exp(+2 pi i f S/65536) = conj of the forward twiddle
                    }
                }
                x0 = z[0]; x1 = z[1]; x2 = z[2]; x3 = z[3];
            };
            if constexpr (S == 0)
                gcfft::dit<+1, NT, 1>([Xb, Cc](int p) { return acq_load<4>(Xb, Cc, p); }, make,
                                      acq_add_power<0>(P, invL2), lds, tw16k, tid);
            else
                gcfft::dit<+1, NT, 1>([Xb, Cc, twp](int p) { return acq_load_tw<4>(Xb, Cc, twp, p); }, make,
                                      acq_add_power<16 * S>(P, invL2), lds, tw16k, tid);
        };
        residue(std::integral_constant<int, 0>{}, nullptr);
        __syncthreads();
        asm volatile("" : "+v"(tid));
        residue(std::integral_constant<int, 1>{}, tw64p1);
        __syncthreads();
        asm volatile("" : "+v"(tid));
        residue(std::integral_constant<int, 2>{}, tw32p);
        __syncthreads();
        asm volatile("" : "+v"(tid));
        residue(std::integral_constant<int, 3>{}, tw64p3);

        const GcAcqRow r = acq_row_stats<NT>(P, lag_of, n, nsc2, sd, si, tid);
        if (tid == 0) *d.row(rows, ch, it, bin) = r;
        __syncthreads();
    }
    if (Pout) acq_write_power(Pout, P, lag_of, tid0, bin, n);
}

// The tracking state an acquired channel starts with, where sdracquisition() leaves it (ref src/sdracq.c:51-55:
// trk.carrfreq = acq.acqfreq, trk.codefreq = crate, code and carrier remainders zero, tracking from the returned
// buffloc).  carrfreq: r.acqfreq, or the refined frequency of a channel that has one (acq_start_freq)
__device__ __forceinline__ GcTrkState acq_start_state(const gnsscorr_acqres_t &r, const GcChan &c, double carrfreq)
{
    GcTrkState s;
    s.carrfreq = carrfreq;
    s.codefreq = c.crate;
    s.remcode = 0.0;
    s.remcarr = 0.0;
    s.buffloc = r.buffloc;
    return s;
}

// acq_final: one wavefront per listed channel; the lanes share the bins of an iteration.  edge_out[ch]: the hypothesis
// of the deciding iteration's best row for an acquired channel that has hypotheses, -1 otherwise.
__global__ __launch_bounds__(64) void acq_final_kernel(
    const GcChan *__restrict__ chan, const double *__restrict__ freqs, const GcAcqRow *__restrict__ rows,
    const uint64_t *__restrict__ grid_wrpos, gnsscorr_acqres_t *__restrict__ res, int *__restrict__ iters_out,
    int *__restrict__ edge_out, const int *__restrict__ list, int nlist, GcAcqDims d)
{
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= nlist) return;
    const int ch = list[blockIdx.x];
    const GcChan &c = chan[ch];
    const int n = c.nsamp, ngroup = acq_groups(c);
    const double tcoh = (double)c.ncoh * c.ctime;               // a group's coherent time: 1 / its noise bandwidth
    gnsscorr_acqres_t r;
    r.acqcodei = 0; r.freqi = 0; r.acqfreq = 0; r.cn0 = 0; r.peakr = 0; r.flagacq = 0; r.iters = c.intg;
    const uint64_t b0 = grid_wrpos[c.grid] - (uint64_t)(c.intg + 1) * n;
    int it = 0, edge = -1;
    for (; it < ngroup; it++) {
        const GcAcqRow *row = d.row(rows, ch, it);
        const int fi = acq_best_row(row, c.nfreq, lane);
        const GcAcqRow w = row[fi];
        edge = w.edge;
        const int ne = 4 * c.nsampchip + 1;                     // samples inside the excluded window
        const double meanP = w.sum_out / (double)(n - ne);
        r.cn0 = 10.0 * log10(w.rowmax / meanP / tcoh);
        r.peakr = w.rowmax / w.max_out;
        r.acqcodei = w.argmax;
        r.freqi = fi;
        r.acqfreq = freqs[c.freq_off + fi];
        if (acq_passes(w)) { r.flagacq = 1; break; }
    }
    // code periods consumed; acq_power re-runs the groups
    r.iters = r.flagacq ? (it + 1) * c.ncoh : c.intg;
    // ref src/sdracq.c:51-53 / :62
    r.buffloc = r.flagacq ? b0 + (uint64_t)r.acqcodei : b0 + (uint64_t)c.intg * n;
    if (lane == 0) {
        res[ch] = r;
        edge_out[ch] = r.flagacq && c.estep > 0 ? edge : -1;
        iters_out[ch] = r.flagacq ? it + 1 : ngroup;
    }
}

// ---- carrier refinement of the acquired channels (gnsscorr_acq_set_refine) ---------------------------
// Behind acq_final, for the listed channels with nref > 0 that it acquired: the nref*nsamp samples from the returned
// buffloc on are wiped off at the bin centre by one carrier walk (acq_fine_nco), correlated period by period with the
// search's replica (acq_prompt: the hot path, one read of the span), and the squared prompt sums are searched for
// their line on K = GNSSCORR_FINE_BINS frequencies (acq_fine).  Nothing here writes a gnsscorr_acqres_t.

// the frequency a hand-over starts tracking from: the refined one where the last search refined the channel
__device__ __forceinline__ double acq_start_freq(const gnsscorr_acqres_t &r, const gnsscorr_acqfine_t *__restrict__ fine,
                                                 int ch)
{
    return fine && fine[ch].nref > 0 ? fine[ch].finefreq : r.acqfreq;
}

// one lane per list entry: the carrier table of the channel's refine span.  n = 0: the channel is not refined (nref = 0,
// not acquired, or a span without a table -- the fetch reports the run)
__global__ void acq_fine_nco_kernel(const GcChan *__restrict__ chan, const gnsscorr_acqres_t *__restrict__ res,
                                    const int *__restrict__ list, int nlist, GcAcqCar *__restrict__ fcar,
                                    int *__restrict__ overflow)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nlist) return;
    const int ch = list[i];
    const GcChan &c = chan[ch];
    if (c.nref <= 0 || !res[ch].flagacq) { fcar[ch].n = 0; return; }
    acq_span_table(fcar + ch, res[ch].acqfreq, c.ti, c.nref * c.nsamp, overflow);
}

typedef const __attribute__((address_space(1))) short *gc_gptr_i16;
#define GC_PROMPT_NT 512

// acq_prompt: grid (period m, list entry).  P_m = sum_k c[k] (I + iQ)[m n + k] over the wiped-off samples of period m of
// the span, c the replica acq_code transforms; consecutive lanes read consecutive ring samples (an IQ pair as one
// 16-bit load), int32 partial sums per lane (|I|, |Q| <= 2*32*128, n <= 32768: |P| < 2^28).
__global__ __launch_bounds__(GC_PROMPT_NT) void acq_prompt_kernel(
    const GcChan *__restrict__ chan, const gnsscorr_acqres_t *__restrict__ res, const GcAcqCar *__restrict__ fcar,
    const int *__restrict__ list, int nlist, int *__restrict__ prompt)
{
    __shared__ int lk0[GC_NCAR];
    __shared__ GcCarSeg lseg[GC_NCAR];
    __shared__ int red[2][GC_PROMPT_NT / 64];
    const int m = blockIdx.x, tid = threadIdx.x;
    if ((int)blockIdx.y >= nlist) return;
    const int ch = list[blockIdx.y];
    const GcChan &c = chan[ch];
    if (m >= c.nref || !res[ch].flagacq) return;
    const int ncar = acq_table_to_lds(fcar + ch, lk0, lseg, tid);
    if (ncar <= 0) return;
    __syncthreads();
    const int n = c.nsamp, clen = c.clen, dtype = c.dtype;
    const uint64_t ringlen = c.ringlen, base = res[ch].buffloc % ringlen;
    const gc_gptr_i8 ring = (gc_gptr_i8)c.ring, code = (gc_gptr_i8)c.code;
    const gc_gptr_i16 ring2 = (gc_gptr_i16)c.ring;
    const double ci = __dmul_rn(c.ti, c.crate);
    int sI = 0, sQ = 0;
    for (int k = tid; k < n; k += GC_PROMPT_NT) {
        const int s = m * n + k;        // sample k of period m: sample s of the span
        const uint64_t pos = gc_span_pos(base, s, ringlen);
        int I, Q;
        gc_wipeoff(gc_carrier_idx_at(lk0, lseg, ncar, s), dtype,
                   [&] { const int v = ring2[pos]; return make_int2((signed char)(v & 0xff), v >> 8); },
                   [&] { return (int)ring[pos]; }, I, Q);
        const int cv = acq_replica(code, clen, ci, k);
        sI += cv * I;
        sQ += cv * Q;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sI += __shfl_xor(sI, o, 64);
        sQ += __shfl_xor(sQ, o, 64);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = sI; red[1][tid >> 6] = sQ; }
    __syncthreads();
    if (tid == 0) {
        int pI = 0, pQ = 0;
#pragma unroll
        for (int w = 0; w < GC_PROMPT_NT / 64; w++) { pI += red[0][w]; pQ += red[1][w]; }
        *reinterpret_cast<int2 *>(GcAcqDims::prompt(prompt, ch, m)) = make_int2(pI, pQ);
    }
}

// acq_fine: one wavefront per list entry.  S_m = P_m^2 (exact in int64, then fp64), Z[q] = sum_m S_m exp(+2 pi i
// ((q m) mod K)/K) with the lanes over q = -K/2 .. K/2-1, the largest |Z|^2 (lowest q on ties) over the wavefront, one
// gnsscorr_acqfine_t; a listed channel without refinement gets finefreq = acqfreq and zeros (its prompt row was cleared
// with the others' tails before acq_prompt).
__global__ __launch_bounds__(64) void acq_fine_kernel(
    const GcChan *__restrict__ chan, const gnsscorr_acqres_t *__restrict__ res, const GcAcqCar *__restrict__ fcar,
    const int *__restrict__ list, int nlist, const int *__restrict__ prompt, gnsscorr_acqfine_t *__restrict__ fine)
{
    constexpr int K = GNSSCORR_FINE_BINS;
    __shared__ double sr[GNSSCORR_MAXCOH], si[GNSSCORR_MAXCOH], sa[GNSSCORR_MAXCOH];
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= nlist) return;
    const int ch = list[blockIdx.x];
    const GcChan &c = chan[ch];
    const gnsscorr_acqres_t r = res[ch];
    gnsscorr_acqfine_t f;
    f.finefreq = r.acqfreq; f.quality = 0.0; f.q = 0; f.nref = 0;
    const int nref = c.nref;
    if (nref > 0 && r.flagacq && fcar[ch].n > 0) {
        if (lane < nref) {
            const int *pm = GcAcqDims::prompt(prompt, ch, lane);
            const long long I = pm[0], Q = pm[1];
            sr[lane] = (double)(I * I - Q * Q);
            si[lane] = (double)(2 * I * Q);
            sa[lane] = (double)(I * I + Q * Q);      // |S_m| = |P_m|^2
        }
        __syncthreads();
        double den = 0.0;
        for (int m = 0; m < nref; m++) den += sa[m];
        MaxIdx best; best.v = -1.0; best.k = 0x7fffffff;
        for (int q = lane - K / 2; q < K / 2; q += 64) {
            double zr = 0.0, zi = 0.0;
            for (int m = 0; m < nref; m++) {
                double sn, cs;
                sincospi(2.0 * (double)((q * m) & (K - 1)) / (double)K, &sn, &cs);
                zr += sr[m] * cs - si[m] * sn;
                zi += sr[m] * sn + si[m] * cs;
            }
            MaxIdx t; t.v = zr * zr + zi * zi; t.k = q;
            best = better(best, t);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            MaxIdx t;
            t.v = __shfl_xor(best.v, o, 64);
            t.k = __shfl_xor(best.k, o, 64);
            best = better(best, t);
        }
        f.q = best.k;
        f.nref = nref;
        f.finefreq = __dadd_rn(r.acqfreq, __ddiv_rn((double)best.k, 2.0 * (double)K * c.ctime));
        f.quality = den > 0.0 ? best.v / (den * den) : 0.0;
    }
    if (lane == 0) fine[ch] = f;
}

// acq_corr's iteration limit of the listed channels: all of their groups
__global__ void acq_iters_kernel(int *iters, const GcChan *__restrict__ chan, const int *__restrict__ list, int nlist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nlist) iters[list[i]] = acq_groups(chan[list[i]]);
}

// stand-alone batch FFT (op-level entry point and tests): grid (batch); natural order in and out
// (the pass-order result is scattered to its frequency on the way out)
template <int S>
__global__ __launch_bounds__(GC_FFT_THREADS) void fft16k_kernel(const float2 *__restrict__ in,
                                                                float2 *__restrict__ out,
                                                                const float2 *__restrict__ tw16k)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const float2 *x = in + (size_t)blockIdx.x * GC_LH;
    float2 *y = out + (size_t)blockIdx.x * GC_LH;
    gcfft::dif<S>([&](int j) { return x[j]; },
                  [&](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
                      y[gcfft::freq_of(p)] = x0; y[gcfft::freq_of(p + 1)] = x1;
                      y[gcfft::freq_of(p + 2)] = x2; y[gcfft::freq_of(p + 3)] = x3;
                  },
                  lds, tw16k, tid);
}

// power spectrum of a 16384- or 32768-point sequence (cpxpspec, ref src/sdrcmn.c:261-276)
__global__ __launch_bounds__(GC_FFT_THREADS) void pspec_kernel(const float2 *__restrict__ in, int n,
                                                               const float2 *__restrict__ tw16k,
                                                               const float2 *__restrict__ tw32k,
                                                               double *__restrict__ pspec, int flagsum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    auto power_to = [&](int mul, int add) {
        return [=](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
            const float2 xs[4] = {x0, x1, x2, x3};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int f = mul * gcfft::freq_of(p + i) + add;
                const double pw = (double)fmaf(xs[i].x, xs[i].x, xs[i].y * xs[i].y);
                pspec[f] = flagsum ? pspec[f] + pw : pw;
            }
        };
    };
    if (n == GC_LH) {
        gcfft::dif<-1>([&](int j) { return in[j]; }, power_to(1, 0), lds, tw16k, tid);
    } else {
        gcfft::dif<-1>([&](int j) { return cadd(in[j], in[j + GC_LH]); }, power_to(2, 0), lds, tw16k, tid);
        __syncthreads();
        gcfft::dif<-1>([&](int j) { return cmul(csub(in[j], in[j + GC_LH]), tw32k[j]); }, power_to(2, 1), lds,
                       tw16k, tid);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The FFT tables and the dynamic LDS sizes of the kernels that read them: once per context, whoever asks first
int gc_acq_twiddles(gnsscorr_ctx *ctx)
{
    GcFftTables &f = ctx->fft;
    if (f.ready) return GNSSCORR_OK;
    GC_RESERVE(ctx, f.tw16k, GC_LH);
    GC_RESERVE(ctx, f.tw32k, GC_LH);
    GC_RESERVE(ctx, f.tw32p, GC_LH);
    GC_RESERVE(ctx, f.tw64p1, GC_LH);
    GC_RESERVE(ctx, f.tw64p3, GC_LH);
    hipLaunchKernelGGL(tw_init_kernel, dim3(GC_LH / 256), dim3(256), 0, ctx->stream, f.tw16k, f.tw32k, f.tw32p);
    hipLaunchKernelGGL(tw64_init_kernel, dim3(GC_LH / 256), dim3(256), 0, ctx->stream, f.tw64p1, f.tw64p3);
    GC_HIP(hipGetLastError());
    const int lds = GC_FFT_LDS + 256, fwd = lds + GC_ACQ_CARLDS, corr = GC_ACQ_CORR_LDS;
    const struct { const void *kernel; int lds; } dyn[] = {
        {(const void *)acq_fwd_kernel<false>, fwd}, {(const void *)acq_fwd_kernel<true>, fwd},
        {(const void *)acq_fwd_kernel<true, true>, fwd}, {(const void *)acq_fwd_kernel<true, false, true>, fwd},
        {(const void *)acq_fwd_kernel<true, true, true>, fwd}, {(const void *)acq_code_kernel, lds},
        {(const void *)acq_corr_kernel<512>, corr}, {(const void *)acq_corr_kernel<1024>, corr},
        {(const void *)acq_corr_kernel<512, true>, corr}, {(const void *)acq_corr64_kernel, corr},
        {(const void *)fft16k_kernel<-1>, lds}, {(const void *)fft16k_kernel<+1>, lds}, {(const void *)pspec_kernel, lds}};
    for (const auto &k : dyn) GC_HIP(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    f.ready = true;
    return GNSSCORR_OK;
}

// Code-Doppler compensation (include/gnsscorr.h): group g of bin b starts s(b, g) samples later, in fp64
// and in this order:  dop = (freq[b] - f_if) - foffset;  x = (dop / f_cf) * (double)(g * ncoh * n);  s = -rint(x).
int gc_acq_shifts(const gnsscorr_ctx *ctx, int ch, std::vector<int32_t> &s, int *back)
{
    const GcChan &c = ctx->hchan[ch];
    const gnsscorr_chan_t &d = ctx->hdesc[ch];
    const int G = acq_groups(c);
    const double f_cf = ctx->hfcf[ch];
    s.assign((size_t)c.nfreq * G, 0);
    *back = 0;
    if (f_cf == 0.0) return GNSSCORR_OK;
    for (int b = 0; b < c.nfreq; b++)
        for (int g = 0; g < G; g++) {
            const double dop = (d.freq[b] - d.f_if) - d.foffset;
            const double x = (dop / f_cf) * (double)((int64_t)g * c.ncoh * c.nsamp);
            const double r = rint(x);           // round-half-even
            if (!(fabs(r) <= (double)c.nsamp))
                return gc_fail(GNSSCORR_EINVAL, "acquisition: channel %d: code-Doppler shift of %.0f samples in group %d of bin %d "
                               "(more than a code period of %d)", ch, -r, g, b, c.nsamp);
            const int32_t v = -(int32_t)r;
            s[(size_t)b * G + g] = v;
            if (v > *back) *back = v;
        }
    return GNSSCORR_OK;
}

static int acq_prepare(gnsscorr_ctx *ctx)
{
    GC_TRY(gc_acq_twiddles(ctx));
    const GcFftTables &f = ctx->fft;
    GcAcq *w = &ctx->acq;
    if (w->prepared) return GNSSCORR_OK;
    const int nch = ctx->nch;
    GcAcqDims d = {0, 0, 0, GC_L};
    w->nch = nch;
    w->ngrid = 0;
    w->grid_chan.clear();
    for (int i = 0; i < nch; i++) {
        const GcChan &c = ctx->hchan[i];
        // the window of 2*nsamp samples must fit the transform: 32768 points up to 16384 samples per code
        // period, 65536 (20 / 26 Msps front ends) up to 32768
        if (c.nsamp > GC_L)
            return gc_fail(GNSSCORR_EINVAL, "acquisition: nsamp %d needs an FFT longer than 65536", c.nsamp);
        if (c.nsamp > GC_LH) d.L = 2 * GC_L;
        if (c.grid >= w->ngrid) { w->ngrid = c.grid + 1; w->grid_chan.push_back(i); }
        if (c.nfreq > d.maxfreq) d.maxfreq = c.nfreq;
        if (acq_groups(c) > d.maxintg) d.maxintg = acq_groups(c);
        if (acq_groups(c) * acq_hyps(c) > d.maxslot) d.maxslot = acq_groups(c) * acq_hyps(c);
    }
    // acq_corr64 reads X by iteration (GcAcqDims::x)
    if (d.L == 2 * GC_L && d.maxslot != d.maxintg)
        return gc_fail(GNSSCORR_ESTATE, "acquisition: bit-edge hypotheses on the 65536-point transform");
    w->dims = d;
    // the grids' shift tables, from each grid's first channel (the channels of a grid agree on them: assign_acq_grids)
    w->cdop = false;
    w->shifts.assign((size_t)w->ngrid * d.maxfreq * d.maxintg, 0);
    w->back.assign(w->ngrid, 0);
    for (int g = 0; g < w->ngrid; g++) {
        const int ch = w->grid_chan[g], G = acq_groups(ctx->hchan[ch]);
        std::vector<int32_t> s;
        GC_TRY(gc_acq_shifts(ctx, ch, s, &w->back[g]));
        for (int b = 0; b < ctx->hchan[ch].nfreq; b++)
            std::copy(s.begin() + (size_t)b * G, s.begin() + (size_t)(b + 1) * G,
                      w->shifts.begin() + ((size_t)g * d.maxfreq + b) * d.maxintg);
        w->cdop = w->cdop || ctx->hfcf[ch] != 0.0;
    }
    if (w->cdop) {
        GC_RESERVE(ctx, w->d_shifts, w->shifts.size());
        GC_HIP(hipMemcpyAsync(w->d_shifts, w->shifts.data(), sizeof(int32_t) * w->shifts.size(), hipMemcpyHostToDevice,
                              ctx->stream));
    }
    GC_RESERVE(ctx, w->X, (size_t)w->ngrid * d.maxslot * d.maxfreq * d.L);
    GC_RESERVE(ctx, w->rows, (size_t)nch * d.maxintg * d.maxfreq);
    GC_RESERVE(ctx, w->arrive, w->arrive_ints());
    GC_RESERVE(ctx, w->iters, nch);
    GC_RESERVE(ctx, w->res, nch);
    GC_RESERVE(ctx, w->edge, nch);
    GC_RESERVE(ctx, w->d_grid_chan, w->ngrid);
    GC_RESERVE(ctx, w->d_grid_wrpos, w->ngrid);
    GC_RESERVE(ctx, w->d_list, w->list_ints());
    w->list.clear();
    w->glist.clear();
    GC_HIP(hipMemcpyAsync(w->d_grid_chan, w->grid_chan.data(), sizeof(int) * w->ngrid, hipMemcpyHostToDevice,
                          ctx->stream));
    GC_RESERVE(ctx, w->car, (size_t)w->ngrid * d.maxfreq);
    GC_RESERVE(ctx, w->car_overflow, 1);
    GC_RESERVE(ctx, w->C, (size_t)nch * d.L);
    GC_HIP(hipMemsetAsync(w->car_overflow, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(acq_nco_kernel, dim3((w->ngrid * d.maxfreq + 63) / 64), dim3(64), 0, ctx->stream, ctx->dchan,
                       w->d_grid_chan, ctx->dfreqs, w->car, w->ngrid, d.maxfreq, w->car_overflow);
    GC_HIP(hipGetLastError());
    {
        GcTimed t(ctx, "acq_code");
        hipLaunchKernelGGL(acq_code_kernel, dim3(nch), dim3(GC_FFT_THREADS), GC_FFT_LDS + 256, ctx->stream,
                           ctx->dchan, f.tw16k, f.tw32p, f.tw64p1, f.tw64p3, w->C, d);
    }
    GC_HIP(hipGetLastError());
    int over = 0;
    GC_HIP(hipMemcpyAsync(&over, w->car_overflow, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    if (over)       // (not prepared)
        return gc_fail(GNSSCORR_EINVAL, "acquisition: %d Doppler bins need more carrier NCO pieces than the tables hold", over);
    w->prepared = true;
    return GNSSCORR_OK;
}

// acq_corr over the list dlist[0..n) with early stop (Pout null), or the power array of channel pout_ch into Pout
// (no early stop; always the 512-lane kernel).  GNSSCORR_ACQ_NT=1024: the 1024-lane variant of the 32768-point search.
// edge: the list's channels (or pout_ch) have bit-edge hypotheses -- the EDGE instance, 512 lanes.
static void launch_acq_corr(gnsscorr_ctx *ctx, double *Pout, int pout_ch, const int *dlist, int n, bool edge)
{
    const GcFftTables &f = ctx->fft;
    GcAcq *w = &ctx->acq;
    static const int nt = getenv("GNSSCORR_ACQ_NT") ? atoi(getenv("GNSSCORR_ACQ_NT")) : 512;
    const bool pout = Pout != nullptr;
    const int nbins = pout ? ctx->hchan[pout_ch].nfreq : w->dims.maxfreq;
    int *arrive = pout ? nullptr : w->arrivals(), *done = pout ? nullptr : w->done();
    auto corr32 = [&](auto kernel, int lanes) {
        hipLaunchKernelGGL(kernel, dim3(acq_corr_blocks(nbins, n, pout)), dim3(lanes), GC_ACQ_CORR_LDS, ctx->stream,
                           ctx->dchan, f.tw16k, f.tw32p, w->X, w->C, w->iters, w->rows, Pout, pout_ch, w->dims.maxfreq,
                           w->dims.maxintg, w->dims.maxslot, dlist, n, arrive, done);
    };
    if (edge)       // (gnsscorr_acq_set_bitedge refuses the 65536-point path)
        corr32(acq_corr_kernel<512, true>, 512);
    else if (w->dims.L == 2 * GC_L)
        hipLaunchKernelGGL(acq_corr64_kernel, dim3(acq_corr64_blocks(nbins, n, pout)), dim3(512), GC_ACQ_CORR_LDS,
                           ctx->stream, ctx->dchan, f.tw16k, f.tw32p, f.tw64p1, f.tw64p3, w->X, w->C, w->iters,
                           w->rows, Pout, pout_ch, w->dims.maxfreq, w->dims.maxintg, dlist, n);
    else if (nt == 1024 && !pout)
        corr32(acq_corr_kernel<1024>, 1024);
    else
        corr32(acq_corr_kernel<512>, 512);
}

// One search over the channels chlist[0..n) (distinct; nullptr: all of them).  wp_ring[r]: write position of ring
// r + 1 the search ends at, 0: the ring's current one.  The steps are local functions over the search's host-side plan;
// the function's last lines are their order.
int gc_acq_run_list(gnsscorr_ctx *ctx, const uint64_t wp_ring[2], const int *chlist, int n)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    if (!ctx->nch) return gc_fail(GNSSCORR_ESTATE, "acq_run: no channels set");
    const int nch = ctx->nch;
    const GcFftTables &f = ctx->fft;
    GcAcq *w = &ctx->acq;
    if (!chlist) n = nch;
    std::vector<int> list, glist;   // the listed channels in the caller's order; the grids that have one, in grid order
    std::vector<char> listed(nch, 0);       // the channel is listed
    std::vector<uint64_t> gw;       // [ngrid] the ring write position a listed grid's search ends at
    std::vector<int> part;          // acq_corr's order of the list: the nplain channels without bit-edge hypotheses,
    int nplain = 0;                 // then those with (a launch each)
    bool coh = false, edge = false; // a listed grid integrates coherently / has bit-edge hypotheses
    bool cdop = false;              // a listed grid compensates code Doppler
    int maxref = 0;                 // the longest refine span of a listed channel, 0: no refinement
    // The caller's list and wp_ring into the plan above.  A valid list prepares the channel set and fences the rings'
    // transfers: the grids are acq_prepare's, a ring's write position the fence's.
    auto plan = [&]() -> int {
        if (n < 1 || n > nch) return gc_fail(GNSSCORR_EINVAL, "acq_run: list of %d channels (1..%d)", n, nch);
        for (int i = 0; i < n; i++) {
            const int ch = chlist ? chlist[i] : i;
            if (ch < 0 || ch >= nch || listed[ch])
                return gc_fail(GNSSCORR_EINVAL, "acq_run: list entry %d: channel %d (0..%d, each once)", i, ch, nch - 1);
            list.push_back(ch);
            listed[ch] = 1;
        }
        GC_HIP(hipSetDevice(ctx->device));
        GC_TRY(acq_prepare(ctx));
        GC_TRY(gc_ingest_fence(ctx));
        for (int ch : list) maxref = std::max(maxref, (int)ctx->hchan[ch].nref);
        if (maxref) {               // the refinement's buffers are made by the first search that asks for it
            GC_RESERVE(ctx, w->fcar, nch);
            GC_RESERVE(ctx, w->fcar_overflow, 1);
            GC_RESERVE(ctx, w->prompt, GcAcqDims::prompt_ints(nch));
            GC_RESERVE(ctx, w->fine, nch);
        }
        for (int g = 0; g < w->ngrid; g++)
            if (std::any_of(list.begin(), list.end(), [&](int ch) { return ctx->hchan[ch].grid == g; })) glist.push_back(g);
        gw.assign(w->ngrid, 0);
        for (int g : glist) {
            const GcChan &c = ctx->hchan[w->grid_chan[g]];
            const int ft = ctx->hdesc[w->grid_chan[g]].ftype;
            const uint64_t wp = wp_ring[ft - 1] ? wp_ring[ft - 1] : ctx->ring[ft - 1].wrpos;
            // a compensated grid's search is the search at wp - back
            const uint64_t look = (uint64_t)(c.intg + 1) * c.nsamp + (uint64_t)w->back[g];
            if (wp < look)
                return gc_fail(GNSSCORR_ESTATE, "acq_run: ring %d holds %llu samples, %llu needed", ft,
                               (unsigned long long)wp, (unsigned long long)look);
            if (c.ringlen < look)
                return gc_fail(GNSSCORR_EINVAL, "acq_run: ring %d (%llu samples) is shorter than the %d code periods%s the search looks back",
                               ft, (unsigned long long)c.ringlen, c.intg + 1, w->back[g] ? " and the code-Doppler shift" : "");
            gw[g] = wp - (uint64_t)w->back[g];
            coh = coh || c.ncoh > 1;
            edge = edge || c.estep > 0;
            cdop = cdop || ctx->hfcf[w->grid_chan[g]] != 0.0;
        }
        part = list;
        nplain = (int)(std::stable_partition(part.begin(), part.end(), [&](int ch) { return ctx->hchan[ch].estep <= 0; }) -
                       part.begin());
        return GNSSCORR_OK;
    };
    // What changed since the last search goes up: the three lists when they differ, the write positions always; returns
    // when the copies are staged (pageable sources)
    auto upload = [&]() -> int {
        w->nplain = nplain;
        if (list != w->list || glist != w->glist) {
            GC_HIP(hipMemcpyAsync(w->d_chans(), list.data(), sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
            GC_HIP(hipMemcpyAsync(w->d_grids(), glist.data(), sizeof(int) * glist.size(), hipMemcpyHostToDevice,
                                  ctx->stream));
            GC_HIP(hipMemcpyAsync(w->d_parts(), part.data(), sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
            w->list.clear();            // (until the copies are staged)
        }
        GC_HIP(hipMemcpyAsync(w->d_grid_wrpos, gw.data(), sizeof(uint64_t) * w->ngrid, hipMemcpyHostToDevice,
                              ctx->stream));
        GC_HIP(hipStreamSynchronize(ctx->stream));
        w->list = list;
        w->glist = glist;
        return GNSSCORR_OK;
    };
    // acq_fwd over the listed grids, the clears, acq_corr over each part of the list, acq_final
    auto queue_search = [&]() -> int {
        const GcAcqDims &d = w->dims;
        {
            GcTimed t(ctx, "acq_fwd");
            auto fwd = cdop ? (edge ? acq_fwd_kernel<true, true, true> : acq_fwd_kernel<true, false, true>)
                     : edge ? acq_fwd_kernel<true, true> : coh ? acq_fwd_kernel<true> : acq_fwd_kernel<false>;
            hipLaunchKernelGGL(fwd, dim3(d.maxfreq, d.maxslot, glist.size()), dim3(GC_FFT_THREADS),
                               GC_FFT_LDS + 256 + GC_ACQ_CARLDS, ctx->stream, ctx->dchan, w->d_grid_chan, w->d_grids(),
                               w->car, w->d_grid_wrpos, f.tw16k, f.tw32p, f.tw64p1, f.tw64p3, w->X, d.maxfreq, d.maxslot,
                               d.L, (const int32_t *)w->d_shifts.p, d.maxintg);
        }
        GC_HIP(hipGetLastError());
        // channels that are not listed: no iterations, a zero result row
        if (n < nch) {
            GC_HIP(hipMemsetAsync(w->iters, 0, sizeof(int) * nch, ctx->stream));
            GC_HIP(hipMemsetAsync(w->res, 0, sizeof(gnsscorr_acqres_t) * nch, ctx->stream));
            GC_HIP(hipMemsetAsync(w->edge, 0xff, sizeof(int) * nch, ctx->stream));      // -1
        }
        hipLaunchKernelGGL(acq_iters_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, w->iters, ctx->dchan,
                           w->d_chans(), n);
        GC_HIP(hipMemsetAsync(w->arrive, 0, sizeof(int) * w->arrive_ints(), ctx->stream));
        {
            GcTimed t(ctx, "acq_corr");
            if (nplain) launch_acq_corr(ctx, nullptr, 0, w->d_parts(), nplain, false);
            if (n > nplain) launch_acq_corr(ctx, nullptr, 0, w->d_parts() + nplain, n - nplain, true);
        }
        GC_HIP(hipGetLastError());
        {
            GcTimed t(ctx, "acq_final");
            hipLaunchKernelGGL(acq_final_kernel, dim3(n), dim3(64), 0, ctx->stream, ctx->dchan, ctx->dfreqs, w->rows,
                               w->d_grid_wrpos, w->res, w->iters, w->edge, w->d_chans(), n, d);
        }
        GC_HIP(hipGetLastError());
        return GNSSCORR_OK;
    };

    // behind acq_final: the clears, acq_fine_nco, acq_prompt, acq_fine over the list
    auto queue_refine = [&]() -> int {
        const int *dlist = w->d_chans();
        // unlisted channels: a zero row, as in res; every prompt row starts from zero (rows without refinement and
        // the periods beyond a channel's nref stay so)
        if (n < nch) GC_HIP(hipMemsetAsync(w->fine, 0, sizeof(gnsscorr_acqfine_t) * nch, ctx->stream));
        GC_HIP(hipMemsetAsync(w->prompt, 0, sizeof(int) * GcAcqDims::prompt_ints(nch), ctx->stream));
        GC_HIP(hipMemsetAsync(w->fcar_overflow, 0, sizeof(int), ctx->stream));
        {
            GcTimed t(ctx, "acq_fine_nco");
            hipLaunchKernelGGL(acq_fine_nco_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, ctx->dchan, w->res,
                               dlist, n, w->fcar, w->fcar_overflow);
        }
        {
            GcTimed t(ctx, "acq_prompt");
            hipLaunchKernelGGL(acq_prompt_kernel, dim3(maxref, n), dim3(GC_PROMPT_NT), 0, ctx->stream, ctx->dchan,
                               w->res, w->fcar, dlist, n, w->prompt);
        }
        {
            GcTimed t(ctx, "acq_fine");
            hipLaunchKernelGGL(acq_fine_kernel, dim3(n), dim3(64), 0, ctx->stream, ctx->dchan, w->res, w->fcar, dlist,
                               n, w->prompt, w->fine);
        }
        GC_HIP(hipGetLastError());
        w->refined = true;
        return GNSSCORR_OK;
    };
    GC_TRY(plan());
    GC_TRY(upload());
    w->ran = false;                 // until every launch below is queued
    GC_TRY(queue_search());
    w->refined = false;
    if (maxref) GC_TRY(queue_refine());
    w->listed = listed;
    w->ran = true;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_run(gnsscorr_ctx *ctx, uint64_t wrpos)
{
    const uint64_t wp[2] = {wrpos, wrpos};
    return gc_acq_run_list(ctx, wp, nullptr, 0);
}

extern "C" int gnsscorr_acq_run_subset(gnsscorr_ctx *ctx, uint64_t wrpos, const int *chlist, int n)
{
    if (!chlist) return gc_fail(GNSSCORR_EINVAL, "acq_run_subset: null channel list");
    const uint64_t wp[2] = {wrpos, wrpos};
    return gc_acq_run_list(ctx, wp, chlist, n);
}

// a fetch call's device array to the host (a null destination is skipped) and, behind a call's last one, the wait
static int acq_copy_out(gnsscorr_ctx *ctx, void *dst, const void *src, size_t bytes, bool last = true)
{
    GC_HIP(hipSetDevice(ctx->device));
    if (dst) GC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (last) GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_acq_fetch(gnsscorr_ctx *ctx, gnsscorr_acqres_t *res)
{
    if (!ctx || !ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "acq_fetch: no acq_run yet");
    if (!res) return gc_fail(GNSSCORR_EINVAL, "acq_fetch: null result array");
    return acq_copy_out(ctx, res, ctx->acq.res, sizeof(gnsscorr_acqres_t) * ctx->nch);
}

extern "C" int gnsscorr_acq_fetch_edge(gnsscorr_ctx *ctx, int *edge)
{
    if (!ctx || !edge) return gc_fail(GNSSCORR_EINVAL, "acq_fetch_edge: null context or result array");
    if (!ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "acq_fetch_edge: no acq_run yet");
    return acq_copy_out(ctx, edge, ctx->acq.edge, sizeof(int) * ctx->nch);
}

// The channel's copy of its grid's shift table as the last prepare built it, [nfreq][groups], and the grid's look-back
extern "C" int gnsscorr_acq_fetch_shifts(gnsscorr_ctx *ctx, int ch, int32_t *s, int *back)
{
    if (!ctx || !s || !back) return gc_fail(GNSSCORR_EINVAL, "acq_fetch_shifts: null context or result");
    if (ch < 0 || ch >= ctx->nch) return gc_fail(GNSSCORR_EINVAL, "acq_fetch_shifts: channel %d of %d", ch, ctx->nch);
    const GcAcq &w = ctx->acq;
    if (!w.prepared) return gc_fail(GNSSCORR_ESTATE, "acq_fetch_shifts: no search has prepared the channel set yet");
    const GcChan &c = ctx->hchan[ch];
    const int G = acq_groups(c);
    for (int b = 0; b < c.nfreq; b++)
        for (int g = 0; g < G; g++) s[(size_t)b * G + g] = w.shifts[((size_t)c.grid * w.dims.maxfreq + b) * w.dims.maxintg + g];
    *back = w.back[c.grid];
    return GNSSCORR_OK;
}

// The refinement of the last search (include/gnsscorr.h).  A search that queued none (no listed channel with nref > 0)
// left rule 8 for every channel: finefreq = acqfreq of its result row, zeros.
extern "C" int gnsscorr_acq_fetch_fine(gnsscorr_ctx *ctx, gnsscorr_acqfine_t *fine, int32_t *prompt)
{
    if (!ctx || !ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "acq_fetch_fine: no acq_run yet");
    if (!fine) return gc_fail(GNSSCORR_EINVAL, "acq_fetch_fine: null result array");
    GcAcq *w = &ctx->acq;
    const int nch = ctx->nch;
    const size_t np = GcAcqDims::prompt_ints(nch);
    if (!w->refined) {
        std::vector<gnsscorr_acqres_t> res(nch);
        GC_TRY(gnsscorr_acq_fetch(ctx, res.data()));
        memset(fine, 0, sizeof(gnsscorr_acqfine_t) * nch);
        for (int i = 0; i < nch; i++) fine[i].finefreq = res[i].acqfreq;
        if (prompt) memset(prompt, 0, sizeof(int32_t) * np);
        return GNSSCORR_OK;
    }
    int over = 0;
    GC_TRY(acq_copy_out(ctx, fine, w->fine, sizeof(gnsscorr_acqfine_t) * nch, false));
    GC_TRY(acq_copy_out(ctx, prompt, w->prompt, sizeof(int32_t) * np, false));
    GC_TRY(acq_copy_out(ctx, &over, w->fcar_overflow, sizeof(int)));
    if (over)
        return gc_fail(GNSSCORR_EINVAL, "acquisition: %d refine spans need more carrier NCO pieces than the tables hold", over);
    return GNSSCORR_OK;
}

// Acquired channels start tracking from acq_start_state(); channels that were not acquired keep their state.
// fine: the last search's refinement, null when it queued none.
__global__ void acq_to_trk_kernel(const GcChan *__restrict__ chan, const gnsscorr_acqres_t *__restrict__ res,
                                  const gnsscorr_acqfine_t *__restrict__ fine, GcTrkState *__restrict__ state, int nch)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nch || !res[ch].flagacq) return;
    state[ch] = acq_start_state(res[ch], chan[ch], acq_start_freq(res[ch], fine, ch));
}

extern "C" int gnsscorr_trk_start_from_acq(gnsscorr_ctx *ctx)
{
    if (!ctx || !ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "trk_start_from_acq: no acq_run yet");
    GC_HIP(hipSetDevice(ctx->device));
    int rc = gc_quiesce(ctx);
    if (rc) return rc;
    hipLaunchKernelGGL(acq_to_trk_kernel, dim3((ctx->nch + 63) / 64), dim3(64), 0, ctx->stream, ctx->dchan,
                       ctx->acq.res, ctx->acq.refined ? ctx->acq.fine.p : nullptr, ctx->state.cur(), ctx->nch);
    GC_HIP(hipGetLastError());
    return GNSSCORR_OK;
}

// The same hand-over into the closed loop: one workgroup per listed channel; an acquired one gets the tracking state
// above and the loop state sdrthread() starts tracking with -- the channel's constants kept (filter coefficients,
// ne / nl, loopms, rate, prn, the sdrch_t constants), acqfreq from the search, every running field as inittrkstruct()
// / initnavstruct() leave it (ref src/sdrinit.c:432-480,485-560: zero) and cnt = 0.  That is gnsscorr_loop_t from
// flagsync up to prn and from biti to the end.
__global__ __launch_bounds__(64) void acq_to_loop_kernel(const GcChan *__restrict__ chan, const gnsscorr_acqres_t *__restrict__ res,
                                                         const gnsscorr_acqfine_t *__restrict__ fine,
                                                         GcTrkState *__restrict__ state, gnsscorr_loop_t *__restrict__ loop,
                                                         const int *__restrict__ list, int nlist)
{
    if ((int)blockIdx.x >= nlist) return;
    const int ch = list[blockIdx.x], tid = threadIdx.x;
    const gnsscorr_acqres_t r = res[ch];
    if (!r.flagacq) return;
    static_assert(offsetof(gnsscorr_loop_t, flagsync) % 4 == 0 && offsetof(gnsscorr_loop_t, prn) % 4 == 0 &&
                  offsetof(gnsscorr_loop_t, biti) == offsetof(gnsscorr_loop_t, prn) + 4 && sizeof(gnsscorr_loop_t) % 4 == 0,
                  "loop state layout");
    constexpr int a0 = offsetof(gnsscorr_loop_t, flagsync) / 4, a1 = offsetof(gnsscorr_loop_t, prn) / 4;
    constexpr int b0 = offsetof(gnsscorr_loop_t, biti) / 4, b1 = sizeof(gnsscorr_loop_t) / 4;
    int *w = reinterpret_cast<int *>(loop + ch);
    for (int k = a0 + tid; k < a1; k += 64) w[k] = 0;
    for (int k = b0 + tid; k < b1; k += 64) w[k] = 0;
    if (tid == 0) {
        const double freq = acq_start_freq(r, fine, ch);
        loop[ch].acqfreq = freq;
        state[ch] = acq_start_state(r, chan[ch], freq);
    }
}

int gc_acq_handover(gnsscorr_ctx *ctx, bool quiesce)
{
    if (!ctx || !ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "loop_start_from_acq: no acq_run yet");
    GC_HIP(hipSetDevice(ctx->device));
    if (quiesce) { int rc = gc_quiesce(ctx); if (rc) return rc; }
    const int n = (int)ctx->acq.list.size();
    hipLaunchKernelGGL(acq_to_loop_kernel, dim3(n), dim3(64), 0, ctx->stream, ctx->dchan, ctx->acq.res,
                       ctx->acq.refined ? ctx->acq.fine.p : nullptr, ctx->state.cur(), ctx->loop.dloop, ctx->acq.d_chans(), n);
    GC_HIP(hipGetLastError());
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_loop_start_from_acq(gnsscorr_ctx *ctx) { return gc_acq_handover(ctx, true); }

extern "C" int gnsscorr_acq_power(gnsscorr_ctx *ctx, int ch, double *power)
{
    if (!ctx || !ctx->acq.ran) return gc_fail(GNSSCORR_ESTATE, "acq_power: no acq_run yet");
    if (ch < 0 || ch >= ctx->nch || !power) return gc_fail(GNSSCORR_EINVAL, "acq_power: channel %d", ch);
    if (!ctx->acq.listed[ch]) return gc_fail(GNSSCORR_ESTATE, "acq_power: channel %d was not part of the last search", ch);
    GC_HIP(hipSetDevice(ctx->device));
    GcAcq *w = &ctx->acq;
    const GcChan &c = ctx->hchan[ch];
    const size_t elems = (size_t)c.nfreq * c.nsamp;
    GC_RESERVE(ctx, w->P, elems);
    // iteration count of the last run is still in w->iters[ch]; rows of this channel are rewritten
    // with identical values
    launch_acq_corr(ctx, w->P, ch, nullptr, 0, c.estep > 0);
    GC_HIP(hipGetLastError());
    GC_HIP(hipMemcpyAsync(power, w->P, sizeof(double) * elems, hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_fft16k(gnsscorr_ctx *ctx, const void *in, void *out, int sign, int batch)
{
    if (!ctx || !in || !out || batch <= 0) return gc_fail(GNSSCORR_EINVAL, "fft16k: bad arguments");
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_acq_twiddles(ctx));
    const GcFftTables &f = ctx->fft;
    GcTimed t(ctx, "fft16k");
    if (sign < 0)
        hipLaunchKernelGGL(fft16k_kernel<-1>, dim3(batch), dim3(GC_FFT_THREADS), GC_FFT_LDS + 256, ctx->stream,
                           (const float2 *)in, (float2 *)out, f.tw16k);
    else
        hipLaunchKernelGGL(fft16k_kernel<+1>, dim3(batch), dim3(GC_FFT_THREADS), GC_FFT_LDS + 256, ctx->stream,
                           (const float2 *)in, (float2 *)out, f.tw16k);
    GC_HIP(hipGetLastError());
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_pspec(gnsscorr_ctx *ctx, const float *cpx, int n, int flagsum, double *pspec)
{
    if (!ctx || !cpx || !pspec) return gc_fail(GNSSCORR_EINVAL, "pspec: bad arguments");
    if (n != GC_LH && n != GC_L) return gc_fail(GNSSCORR_EINVAL, "pspec: n %d (16384 or 32768 supported)", n);
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_acq_twiddles(ctx));
    const GcFftTables &f = ctx->fft;
    GcDevBuf<float2> din;
    GcDevBuf<double> dps;
    GC_RESERVE(ctx, din, n);
    GC_RESERVE(ctx, dps, n);
    hipMemcpyAsync(din, cpx, sizeof(float2) * n, hipMemcpyHostToDevice, ctx->stream);
    if (flagsum) hipMemcpyAsync(dps, pspec, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream);
    hipLaunchKernelGGL(pspec_kernel, dim3(1), dim3(GC_FFT_THREADS), GC_FFT_LDS + 256, ctx->stream, din, n,
                       f.tw16k, f.tw32k, dps, flagsum);
    hipError_t e = hipGetLastError();
    hipMemcpyAsync(pspec, dps, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream);
    hipError_t e2 = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return gc_fail_hip(e, "pspec_kernel", __FILE__, __LINE__);
    if (e2 != hipSuccess) return gc_fail_hip(e2, "pspec sync", __FILE__, __LINE__);
    return GNSSCORR_OK;
}
