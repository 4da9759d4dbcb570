// gnsscorr_spec.hip -- IF monitor for gfx950 (MI355X): the front-end sample histogram and the Hann-windowed,
// segment-averaged power spectrum of specthread() (ref src/sdrspec.c:64-102), computed on the HBM ring.
//
// Replaces calchistgram() (ref src/sdrspec.c:170-206) and spectrumanalyzer() (ref src/sdrspec.c:232-296):
//
//   spec_psd  (per snapshot x segment): nfft/2 samples straight from the ring at buffloc + offset, the
//             reference's float inputs (scaled sample, times the Hann window), zero padded to 2*nfft points,
//             forward transform on the LDS-resident FFT (gnsscorr_fft.h; 32768 points as two 16384-point
//             halves of a decimation-in-frequency split, like pspec_kernel in gnsscorr_acq.hip), fp32 power of
//             every bin in natural order into a scratch slab [nsnap][nloop][2*nfft].
//   spec_sum  (per snapshot x bin): the fp64 sum over the segments in segment order -- cpxpspec()'s flagsum
//             accumulation into spectrumanalyzer()'s zeroed s (ref src/sdrcmn.c:268-274, src/sdrspec.c:277).
//             One thread owns one bin, so the order is fixed: bit-identical from run to run.
//   spec_hist (per snapshot): max |byte|, then the 8 (+1) bin counts under calchistgram()'s rules, in integers
//             (LDS atomics, one global atomic per bin and workgroup): exact in any order.
//
// The post-processing (10*log10, the frequency axis) is host code in gnsscorr_spec_fetch, with the reference's
// double expressions.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnsscorr_ctx.h"
#include "gnsscorr_fft.h"
#include "../../include/sdr_compat.h"

#define GC_SPEC_HIST 9          // bins per row: the reference's 8 and the one it writes past yI/yQ (d == maxd > 7)
#define GC_SPEC_HT   256        // threads of the histogram kernels

namespace {

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// grid (nloop, nsnap), GC_FFT_THREADS lanes.  ring: dtype*ringlen bytes (rb), sample s at byte (dtype*s) % rb.
__global__ __launch_bounds__(GC_FFT_THREADS) void spec_psd_kernel(
    const int8_t *__restrict__ ring, uint64_t rb, int dtype, const uint64_t *__restrict__ loc,
    const int *__restrict__ off, int nloop, int nfft, const float *__restrict__ win, double scale,
    const float2 *__restrict__ tw16k, const float2 *__restrict__ tw32k, float *__restrict__ psd)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *lds = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const int k = blockIdx.x, snap = blockIdx.y;
    const int nwin = nfft >> 1;
    const int L = 2 * nfft;
    // byte of the segment's first sample; the validation keeps dtype*nwin <= rb, so one subtraction wraps
    const uint64_t s0 = loc[snap] + (uint64_t)off[(size_t)snap * nloop + k];
    const uint64_t b0 = ((uint64_t)dtype * s0) % rb;
    // xxI[j] = win[j] * x[zuz + j] (ref src/sdrspec.c:262-275), x = (float)(data * scale) (:254-255); zero above nwin
    auto sample = [&](int j) -> float2 {
        if (j >= nwin) return make_float2(0.0f, 0.0f);
        uint64_t b = b0 + (uint64_t)dtype * (uint64_t)j;
        if (b >= rb) b -= rb;
        const float w = win[j];
        const float xr = w * (float)((double)ring[b] * scale);
        const float xi = dtype == 2 ? w * (float)((double)ring[b + 1] * scale) : 0.0f;
        return make_float2(xr, xi);
    };
    float *out = psd + ((size_t)snap * nloop + k) * (size_t)L;
    auto power_to = [&](int mul, int add) {
        return [=](int p, float2 x0, float2 x1, float2 x2, float2 x3) {
            const float2 xs[4] = {x0, x1, x2, x3};
#pragma unroll
            for (int i = 0; i < 4; i++)
                out[mul * gcfft::freq_of(p + i) + add] = fmaf(xs[i].x, xs[i].x, xs[i].y * xs[i].y);
        };
    };
    if (L == GC_FFT_N) {
        gcfft::dif<-1>(sample, power_to(1, 0), lds, tw16k, tid);
    } else {
        // X[2f] = FFT16k(x[j] + x[j + 16384]), X[2f + 1] = FFT16k((x[j] - x[j + 16384]) w^j); the upper half is zero
        gcfft::dif<-1>(sample, power_to(2, 0), lds, tw16k, tid);
        __syncthreads();
        gcfft::dif<-1>([&](int j) { return gcfft::cmul(sample(j), tw32k[j]); }, power_to(2, 1), lds, tw16k, tid);
    }
}

// grid (ceil(L / 256), nsnap): s[f] = sum over segments k = 0.. in order of (double)p[k][f]
__global__ __launch_bounds__(256) void spec_sum_kernel(const float *__restrict__ psd, int nloop, int L,
                                                       double *__restrict__ sum)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= L) return;
    const int snap = blockIdx.y;
    const float *p = psd + (size_t)snap * nloop * L + f;
    double s = 0.0;
    for (int k = 0; k < nloop; k++) s += (double)p[(size_t)k * L];
    sum[(size_t)snap * L + f] = s;
}

// grid (hb, nsnap): maxd[snap] = max |byte| over the snapshot's n*dtype bytes (ref src/sdrspec.c:183)
__global__ __launch_bounds__(GC_SPEC_HT) void spec_hist_max_kernel(const int8_t *__restrict__ ring, uint64_t rb,
                                                                   int dtype, const uint64_t *__restrict__ loc,
                                                                   int n, int *__restrict__ maxd)
{
    __shared__ int m;
    if (threadIdx.x == 0) m = 0;
    __syncthreads();
    const uint64_t b0 = ((uint64_t)dtype * loc[blockIdx.y]) % rb;
    const int nb = n * dtype;
    int mx = 0;
    for (int i = blockIdx.x * GC_SPEC_HT + threadIdx.x; i < nb; i += gridDim.x * GC_SPEC_HT) {
        uint64_t b = b0 + (uint64_t)i;
        if (b >= rb) b -= rb;
        const int d = ring[b];
        mx = max(mx, d < 0 ? -d : d);
    }
    atomicMax(&m, mx);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&maxd[blockIdx.y], m);
}

// calchistgram()'s bin of sample value d (ref src/sdrspec.c:186-205); 8 only for d == maxd > 7
__device__ __forceinline__ int spec_bin(int d, int maxd)
{
    const int b = maxd > 7 ? (int)((double)d / (double)maxd * 4.0 + 4.0) : (d + 7) / 2;
    return min(max(b, 0), GC_SPEC_HIST - 1);
}

// grid (hb, nsnap): the counts.  maxd > 7 and dtype 2: I from byte 2i, Q from byte 2i+1.  Otherwise byte i, i < n,
// into the I row and, for dtype 2, into the Q row too -- the reference indexes the interleaved bytes there (:198, :204)
__global__ __launch_bounds__(GC_SPEC_HT) void spec_hist_count_kernel(const int8_t *__restrict__ ring, uint64_t rb,
                                                                     int dtype, const uint64_t *__restrict__ loc,
                                                                     int n, const int *__restrict__ maxd,
                                                                     unsigned *__restrict__ hist)
{
    __shared__ unsigned c[2 * GC_SPEC_HIST];
    if (threadIdx.x < 2 * GC_SPEC_HIST) c[threadIdx.x] = 0;
    __syncthreads();
    const int snap = blockIdx.y;
    const int md = maxd[snap];
    const uint64_t b0 = ((uint64_t)dtype * loc[snap]) % rb;
    auto byte = [&](uint64_t i) {
        uint64_t b = b0 + i;
        if (b >= rb) b -= rb;
        return (int)ring[b];
    };
    for (int i = blockIdx.x * GC_SPEC_HT + threadIdx.x; i < n; i += gridDim.x * GC_SPEC_HT) {
        if (md > 7 && dtype == 2) {
            atomicAdd(&c[spec_bin(byte(2 * (uint64_t)i), md)], 1u);
            atomicAdd(&c[GC_SPEC_HIST + spec_bin(byte(2 * (uint64_t)i + 1), md)], 1u);
        } else {
            const int b = spec_bin(byte((uint64_t)i), md);
            atomicAdd(&c[b], 1u);
            if (dtype == 2) atomicAdd(&c[GC_SPEC_HIST + b], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * GC_SPEC_HIST && c[threadIdx.x])
        atomicAdd(&hist[(size_t)snap * 2 * GC_SPEC_HIST + threadIdx.x], c[threadIdx.x]);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// everything spec_enqueue needs that does not depend on the samples
int spec_prepare(gnsscorr_ctx *ctx, int nsnap, int nfft, int nloop)
{
    GcSpec *w = &ctx->spec;
    const size_t L = 2 * (size_t)nfft;
    GC_RESERVE(ctx, w->psd, (size_t)nsnap * nloop * L);
    GC_RESERVE(ctx, w->sum, (size_t)nsnap * L);
    GC_RESERVE(ctx, w->loc, (size_t)nsnap);
    GC_RESERVE(ctx, w->off, (size_t)nsnap * nloop);
    GC_RESERVE(ctx, w->hist, (size_t)2 * GC_SPEC_HIST * nsnap);
    GC_RESERVE(ctx, w->maxd, (size_t)nsnap);
    const int nwin = nfft / 2;
    if (w->win_n != nwin) {
        w->win_n = 0;
        GC_RESERVE(ctx, w->win, nwin);
        std::vector<float> hw(nwin);
        hanning(nwin, hw.data());       // the reference's double formula (ref src/sdrspec.c:214-219)
        // in stream order behind any spec_psd still reading the window, and done before hw goes
        GC_HIP(hipMemcpyAsync(w->win, hw.data(), sizeof(float) * nwin, hipMemcpyHostToDevice, ctx->stream));
        GC_HIP(hipStreamSynchronize(ctx->stream));
        w->win_n = nwin;
    }
    GC_HIP(hipFuncSetAttribute((const void *)spec_psd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               GC_FFT_LDS + 256));
    return GNSSCORR_OK;
}

// The launch chain on ctx->stream over `ring` (rb bytes); w->hloc / w->hoff hold the snapshots and offsets.
int spec_enqueue(gnsscorr_ctx *ctx, const int8_t *ring, uint64_t rb, int dtype, int n, int nsnap, int nfft,
                 int nloop, double f_sf, bool hist)
{
    GcSpec *w = &ctx->spec;
    GC_TRY(gc_acq_twiddles(ctx));
    w->ran = false;
    // pageable sources: the copies are staged before the calls return
    GC_HIP(hipMemcpyAsync(w->loc, w->hloc.data(), sizeof(uint64_t) * nsnap, hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipMemcpyAsync(w->off, w->hoff.data(), sizeof(int) * (size_t)nsnap * nloop, hipMemcpyHostToDevice,
                          ctx->stream));
    // ref src/sdrspec.c:255: data*(17.127/(nfft*2)/sqrt((float)SPEC_NLOOP)), the segment count as a float
    const double scale = 17.127 / (nfft * 2) / sqrt((double)(float)nloop);
    const int L = 2 * nfft;
    {
        GcTimed t(ctx, "spec_psd");
        hipLaunchKernelGGL(spec_psd_kernel, dim3(nloop, nsnap), dim3(GC_FFT_THREADS), GC_FFT_LDS + 256, ctx->stream,
                           ring, rb, dtype, w->loc, w->off, nloop, nfft, w->win, scale, ctx->fft.tw16k, ctx->fft.tw32k, w->psd);
    }
    GC_HIP(hipGetLastError());
    {
        GcTimed t(ctx, "spec_sum");
        hipLaunchKernelGGL(spec_sum_kernel, dim3((L + 255) / 256, nsnap), dim3(256), 0, ctx->stream, w->psd, nloop,
                           L, w->sum);
    }
    GC_HIP(hipGetLastError());
    if (hist) {
        GC_HIP(hipMemsetAsync(w->maxd, 0, sizeof(int) * nsnap, ctx->stream));
        GC_HIP(hipMemsetAsync(w->hist, 0, sizeof(unsigned) * 2 * GC_SPEC_HIST * nsnap, ctx->stream));
        const int hb = std::min(128, std::max(1, (n * dtype + 16 * GC_SPEC_HT - 1) / (16 * GC_SPEC_HT)));
        GcTimed t(ctx, "spec_hist");
        hipLaunchKernelGGL(spec_hist_max_kernel, dim3(hb, nsnap), dim3(GC_SPEC_HT), 0, ctx->stream, ring, rb, dtype,
                           w->loc, n, w->maxd);
        hipLaunchKernelGGL(spec_hist_count_kernel, dim3(hb, nsnap), dim3(GC_SPEC_HT), 0, ctx->stream, ring, rb,
                           dtype, w->loc, n, w->maxd, w->hist);
    }
    GC_HIP(hipGetLastError());
    w->ran = true;
    w->has_hist = hist;
    w->nsnap = nsnap; w->nfft = nfft; w->nloop = nloop; w->dtype = dtype; w->f_sf = f_sf;
    return GNSSCORR_OK;
}

// dB and frequency axis of one snapshot in the reference's layout and expressions (ref src/sdrspec.c:280-294)
void spec_post(int dtype, int nfft, double f_sf, const double *s, double *pspec, double *freq)
{
#pragma clang fp contract(off)
    if (dtype == DTYPEI) {
        for (int i = 0; i < nfft; i++) {
            if (pspec) pspec[i] = 10 * log10(s[i]);
            if (freq) freq[i] = (i * (f_sf / 2) / (nfft)) / 1e6;
        }
    } else {
        for (int i = 0; i < dtype * nfft; i++) {
            if (pspec) pspec[i] = i < nfft ? 10 * log10(s[nfft + i]) : 10 * log10(s[-nfft + i]);
            if (freq) freq[i] = (-f_sf / 2 + i * f_sf / nfft / 2) / 1e6;
        }
    }
}

bool spec_nfft_ok(int nfft) { return nfft == 8192 || nfft == 16384; }

}  // namespace

extern "C" int gnsscorr_spec_run(gnsscorr_ctx *ctx, const gnsscorr_spec_t *sp, int nsnap, const uint64_t *buffloc,
                                 const int *offsets)
{
    if (!ctx || !sp || !buffloc || !offsets) return gc_fail(GNSSCORR_EINVAL, "spec_run: null argument");
    if (sp->ftype != 1 && sp->ftype != 2) return gc_fail(GNSSCORR_EINVAL, "spec_run: ftype %d", sp->ftype);
    const GcRing &r = ctx->ring[sp->ftype - 1];
    if (!r.mem) return gc_fail(GNSSCORR_ESTATE, "spec_run: ring %d not created", sp->ftype);
    if (!spec_nfft_ok(sp->nfft))
        return gc_fail(GNSSCORR_EINVAL, "spec_run: nfft %d (8192 or 16384 supported)", sp->nfft);
    if (nsnap < 1 || nsnap > 65535) return gc_fail(GNSSCORR_EINVAL, "spec_run: nsnap %d (1..65535)", nsnap);
    if (sp->nloop < 1 || sp->nloop > 65535) return gc_fail(GNSSCORR_EINVAL, "spec_run: nloop %d (1..65535)", sp->nloop);
    const int nwin = sp->nfft / 2;
    if (sp->n < nwin || (uint64_t)sp->n > r.ringlen)
        return gc_fail(GNSSCORR_EINVAL, "spec_run: n %d outside [nfft/2 = %d, ringlen = %llu]", sp->n, nwin,
                       (unsigned long long)r.ringlen);
    const uint64_t wr = r.wrpos;
    const uint64_t oldest = wr > r.ringlen ? wr - r.ringlen : 0;
    for (int s = 0; s < nsnap; s++) {
        if (buffloc[s] < oldest || buffloc[s] + (uint64_t)sp->n > wr)
            return gc_fail(GNSSCORR_EINVAL,
                           "spec_run: snapshot %d [%llu, %llu) is not in ring %d (holds [%llu, %llu))", s,
                           (unsigned long long)buffloc[s], (unsigned long long)(buffloc[s] + sp->n), sp->ftype,
                           (unsigned long long)oldest, (unsigned long long)wr);
        for (int k = 0; k < sp->nloop; k++) {
            const int o = offsets[(size_t)s * sp->nloop + k];
            if (o < 0 || o > sp->n - nwin)
                return gc_fail(GNSSCORR_EINVAL, "spec_run: snapshot %d offset %d = %d outside [0, %d]", s, k, o,
                               sp->n - nwin);
        }
    }
    GC_HIP(hipSetDevice(ctx->device));
    int rc = spec_prepare(ctx, nsnap, sp->nfft, sp->nloop);
    if (rc) return rc;
    rc = gc_ingest_fence(ctx);
    if (rc) return rc;
    GcSpec *w = &ctx->spec;
    w->hloc.assign(buffloc, buffloc + nsnap);
    w->hoff.assign(offsets, offsets + (size_t)nsnap * sp->nloop);
    return spec_enqueue(ctx, r.mem, (uint64_t)r.dtype * r.ringlen, r.dtype, sp->n, nsnap, sp->nfft, sp->nloop,
                        sp->f_sf, true);
}

extern "C" int gnsscorr_spec_fetch(gnsscorr_ctx *ctx, double *s, size_t s_cap, double *pspec, size_t pspec_cap,
                                   double *freq, size_t freq_cap, int64_t *hist, size_t hist_cap)
{
    if (!ctx || !ctx->spec.ran) return gc_fail(GNSSCORR_ESTATE, "spec_fetch: no spec_run yet");
    const GcSpec *w = &ctx->spec;
    const size_t L = 2 * (size_t)w->nfft, np = (size_t)w->dtype * w->nfft;
    const size_t need_s = (size_t)w->nsnap * L, need_p = (size_t)w->nsnap * np;
    const size_t need_h = (size_t)w->nsnap * 2 * GC_SPEC_HIST;
    if (s && s_cap < need_s) return gc_fail(GNSSCORR_EINVAL, "spec_fetch: s holds %zu, %zu needed", s_cap, need_s);
    if (pspec && pspec_cap < need_p)
        return gc_fail(GNSSCORR_EINVAL, "spec_fetch: pspec holds %zu, %zu needed", pspec_cap, need_p);
    if (freq && freq_cap < np) return gc_fail(GNSSCORR_EINVAL, "spec_fetch: freq holds %zu, %zu needed", freq_cap, np);
    if (hist && !w->has_hist) return gc_fail(GNSSCORR_ESTATE, "spec_fetch: the last run made no histogram");
    if (hist && hist_cap < need_h)
        return gc_fail(GNSSCORR_EINVAL, "spec_fetch: hist holds %zu, %zu needed", hist_cap, need_h);
    GC_HIP(hipSetDevice(ctx->device));
    std::vector<double> hs;
    std::vector<unsigned> hh;
    if (s || pspec) {
        hs.resize(need_s);
        GC_HIP(hipMemcpyAsync(hs.data(), w->sum, sizeof(double) * need_s, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (hist) {
        hh.resize(need_h);
        GC_HIP(hipMemcpyAsync(hh.data(), w->hist, sizeof(unsigned) * need_h, hipMemcpyDeviceToHost, ctx->stream));
    }
    GC_HIP(hipStreamSynchronize(ctx->stream));
    if (s) std::copy(hs.begin(), hs.end(), s);
    if (pspec)
        for (int k = 0; k < w->nsnap; k++) spec_post(w->dtype, w->nfft, w->f_sf, hs.data() + k * L, pspec + k * np, nullptr);
    if (freq) spec_post(w->dtype, w->nfft, w->f_sf, nullptr, nullptr, freq);
    if (hist)
        for (size_t i = 0; i < need_h; i++) hist[i] = (int64_t)hh[i];
    return GNSSCORR_OK;
}

// ---------------------------------------------------------------------------
// reference drop-in (ref src/sdrspec.c:232-296); hanning() and calchistgram() are host C in sdr_host.c
// ---------------------------------------------------------------------------
extern "C" int spectrumanalyzer(const char *data, int dtype, int n, double f_sf, int nfft, double *freq, double *pspec)
{
    if (!data || !freq || !pspec || (dtype != DTYPEI && dtype != DTYPEIQ) || nfft < 2)
        return gc_fail(-1, "spectrumanalyzer: bad arguments (dtype %d, nfft %d)", dtype, nfft);
    const int nwin = nfft / 2, maxshift = n - nwin;
    if (maxshift < 0)
        return gc_fail(-1, "spectrumanalyzer: n %d shorter than the window nfft/2 = %d", n, nwin);
    // the reference's segment offsets, drawn in its order with the process's rand() (ref src/sdrspec.c:257), before
    // anything touches the device
    std::vector<int> zuz(SPEC_NLOOP);
    for (int i = 0; i < SPEC_NLOOP; i++) zuz[i] = (int)floor((double)rand() / RAND_MAX * maxshift);
    gnsscorr_ctx *ctx = gnsscorr_default_ctx();
    if (!ctx) {
        char why[512];
        snprintf(why, sizeof(why), "%s", gnsscorr_last_error());
        return gc_fail(-1, "spectrumanalyzer: no GPU device (%s); there is no CPU fallback", why);
    }
    const int L = 2 * nfft;
    std::vector<double> s(L, 0.0);
    if (!spec_nfft_ok(nfft)) {
        // other lengths: the reference's own loop over the any-length cpxpspec (gnsscorr_ops.hip)
        std::vector<float> win(nwin), xxx(2 * (size_t)L);
        hanning(nwin, win.data());
        const double scale = 17.127 / (nfft * 2) / sqrt((float)SPEC_NLOOP);
        for (int i = 0; i < SPEC_NLOOP; i++) {
            std::fill(xxx.begin(), xxx.end(), 0.0f);
            for (int k = 0; k < nwin; k++) {
                const size_t j = (size_t)zuz[i] + k;
                xxx[2 * k] = win[k] * (float)(data[dtype * j] * scale);
                if (dtype == DTYPEIQ) xxx[2 * k + 1] = win[k] * (float)(data[2 * j + 1] * scale);
            }
            cpxpspec(nullptr, (cpx_t *)xxx.data(), L, 1, s.data());
        }
        spec_post(dtype, nfft, f_sf, s.data(), pspec, freq);
        return 0;
    }
    std::lock_guard<std::mutex> lk(ctx->mtx);
    int rc = hipSetDevice(ctx->device) == hipSuccess ? GNSSCORR_OK : gc_fail(GNSSCORR_EHIP, "spectrumanalyzer: hipSetDevice");
    if (!rc) rc = spec_prepare(ctx, 1, nfft, SPEC_NLOOP);
    GcSpec *w = &ctx->spec;
    const size_t bytes = (size_t)dtype * n;
    if (!rc) rc = w->stage.reserve(ctx, (bytes + 15) & ~(size_t)15);
    if (!rc) {
        w->hloc.assign(1, 0);
        w->hoff = zuz;
        if (hipMemcpyAsync(w->stage, data, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            rc = gc_fail(GNSSCORR_EHIP, "spectrumanalyzer: copy of the samples");
    }
    if (!rc) rc = spec_enqueue(ctx, w->stage, bytes, dtype, n, 1, nfft, SPEC_NLOOP, f_sf, false);
    if (!rc) rc = gnsscorr_spec_fetch(ctx, nullptr, 0, pspec, (size_t)dtype * nfft, freq, (size_t)dtype * nfft,
                                      nullptr, 0);
    return rc ? -1 : 0;
}
