// gnsscorr_fec.hip -- sliding-window Viterbi decoder (K = 7, rate 1/2) for gfx950 (MI355X): the FEC step of
// predecodefec() for CTYPE_L1SBAS (ref src/sdrnav.c:302-318), which the reference runs on every decided symbol until a
// frame is found.  On a batched symbol log the decodes of all symbol positions are independent, and the 64-state
// trellis is one wavefront wide.
//
// The decoder (libfec's portable viterbi27 as the reference drives it, restated -- libfec itself is on no
// machine of this project):
//   symbols   +1 -> 0, anything else (-1, and the 0 of unfilled history) -> 255
//   state     the last six input bits, newest in bit 0; input bit b takes state i to ((i << 1) | b) & 63, with the
//             register r = (i << 1) | b
//   expected  255 * parity(r & polyA), 255 * parity(r & polyB); branch metric = sum of expected ^ received
//   start     metric 0 for state 0, 63 for the others; uint32, never renormalised
//   survivor  the smaller sum; on equal sums the predecessor i < 32
//   chainback from state 0 whatever the metrics say; decoded bit n = the input bit of step n on that path
//
//   fec_viterbi27  one wavefront per window, lane = state.  A workgroup of GC_FEC_WAVES wavefronts decodes that many
//             windows; each has its own LDS slice: the step's received pair as a 2-bit code (one byte per step) and the
//             step's 64 survivor decisions as one 64-bit word (the ballot of the compare).
//             forward: per step two ds_bpermute reads of the old metrics (states s >> 1 and (s >> 1) + 32), the
//             add-compare-select, the ballot; lane 0 stores the word.
//             chainback: lane 0 walks the words backwards (their addresses do not depend on the path, so the loads
//             pipeline; the dependent chain is a 64-bit shift and three integer operations per step) and packs the
//             bits MSB first; the wavefront then stores the row, zero padded to rowbytes.
//             Integer arithmetic only, no atomics, no scratch, win/2 steps for every window.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gnsscorr_ctx.h"

#define GC_FEC_WAVES   4                        // windows per workgroup
#define GC_FEC_MAXWIN  1512                     // NAVFLEN_SBAS + NAVADDFLEN_SBAS (ref src/sdr.h:166-167)
#define GC_FEC_MAXSTEP (GC_FEC_MAXWIN / 2)
#define GC_FEC_CODEB   ((GC_FEC_MAXSTEP + 15) & ~15)    // bytes of a window's pair codes (later: of its packed row)

namespace {

struct GcFecLds {
    unsigned long long dec[GC_FEC_MAXSTEP];     // survivor decisions of step t, bit s = state s took predecessor (s >> 1) + 32
    unsigned char code[GC_FEC_CODEB];           // received pair of step t: bit 0 / 1 = first / second symbol is not +1
};

__device__ __forceinline__ unsigned fec_bm(unsigned c, unsigned e) { return 255u * (unsigned)__popc((c ^ e) & 3u); }

// PARTS: bit 0 = forward pass, bit 1 = chainback (3: the decoder; 1, 2: ablated builds for tools/fec_time.py, whose
// rows are not decodes).  grid (ceil(npos / GC_FEC_WAVES), nch), GC_FEC_WAVES * 64 lanes.
template <int PARTS>
__global__ __launch_bounds__(GC_FEC_WAVES * 64) void fec_viterbi27_kernel(
    const signed char *__restrict__ sym, int nsym, int pos0, int npos, int stride, int win, int ndec, unsigned polyA,
    unsigned polyB, unsigned char *__restrict__ out, int rowbytes)
{
    __shared__ GcFecLds lds[GC_FEC_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    GcFecLds &w = lds[wave];
    const int nstep = win >> 1;
    // a wavefront past the last window decodes the last one again and stores nothing: every wavefront reaches every barrier
    const int pw = blockIdx.x * GC_FEC_WAVES + wave;
    const int p = min(pw, npos - 1);
    const signed char *s = sym + (size_t)blockIdx.y * (size_t)nsym;
    // the window's first symbol; symbols in front of the stream are 0 (the reference's empty fbits).  The host keeps
    // the window's last symbol pos0 + p * stride below nsym.
    const long long first = (long long)pos0 + (long long)p * stride - (win - 1);
    for (int t = lane; t < nstep; t += 64) {
        const long long i0 = first + 2 * t, i1 = i0 + 1;
        const int s0 = i0 >= 0 ? s[i0] : 0, s1 = i1 >= 0 ? s[i1] : 0;
        w.code[t] = (unsigned char)((s0 != 1) | ((s1 != 1) << 1));
    }
    __syncthreads();

    if (PARTS & 1) {
        // lane = new state s: predecessors s >> 1 (register r = s) and (s >> 1) + 32 (r = s | 64)
        const unsigned e0 = (__popc(lane & polyA) & 1) | ((__popc(lane & polyB) & 1) << 1);
        const unsigned e1 = (__popc((lane | 64) & polyA) & 1) | ((__popc((lane | 64) & polyB) & 1) << 1);
        const int a0 = (lane >> 1) << 2, a1 = ((lane >> 1) + 32) << 2;      // ds_bpermute byte addresses
        unsigned m = lane == 0 ? 0u : 63u;
        auto step = [&](int t, unsigned c) {
            const unsigned m0 = (unsigned)__builtin_amdgcn_ds_bpermute(a0, (int)m) + fec_bm(c, e0);
            const unsigned m1 = (unsigned)__builtin_amdgcn_ds_bpermute(a1, (int)m) + fec_bm(c, e1);
            const bool d = (int)(m0 - m1) > 0;                              // libfec's (m0 - m1) > 0: a tie keeps i < 32
            m = d ? m1 : m0;
            const unsigned long long word = __ballot(d);
            if (lane == 0) w.dec[t] = word;
        };
        // four steps' codes in one LDS read, off the metrics' dependent chain
        const unsigned *code4 = reinterpret_cast<const unsigned *>(w.code);
        int t = 0;
        for (; t + 4 <= nstep; t += 4) {
            const unsigned c4 = code4[t >> 2];
            step(t, c4 & 3u);
            step(t + 1, (c4 >> 8) & 3u);
            step(t + 2, (c4 >> 16) & 3u);
            step(t + 3, (c4 >> 24) & 3u);
        }
        for (; t < nstep; t++) step(t, w.code[t]);
        if (!(PARTS & 2) && lane == 0) w.code[0] = (unsigned char)(m ^ (unsigned)w.dec[nstep - 1]);
    }
    __syncthreads();

    const int nb = (ndec + 7) >> 3;
    if ((PARTS & 2) && lane == 0) {
        unsigned st = 0, cur = 0;
        for (int t = nstep - 1; t >= 0; t--) {
            const unsigned b = st & 1u;                                     // the input bit of step t
            const unsigned d = (unsigned)(w.dec[t] >> st) & 1u;
            st = (st >> 1) | (d << 5);
            if (t < ndec) {
                cur |= b << (7 - (t & 7));
                if ((t & 7) == 0) {
                    w.code[t >> 3] = (unsigned char)cur;
                    cur = 0;
                }
            }
        }
    }
    __syncthreads();
    if (pw < npos) {
        unsigned char *row = out + ((size_t)blockIdx.y * (size_t)npos + (size_t)pw) * (size_t)rowbytes;
        for (int i = lane; i < rowbytes; i += 64)
            row[i] = i < nb ? ((PARTS & 2) ? w.code[i] : (unsigned char)(i == 0 ? w.code[0] : 0)) : (unsigned char)0;
    }
}

}  // namespace

extern "C" int gnsscorr_fec_run(gnsscorr_ctx *ctx, const signed char *sym, int nch, int nsym, int pos0, int npos,
                                int stride, int win, int ndec, int polyA, int polyB, unsigned char *out, int rowbytes)
{
    if (!ctx || !sym || !out) return gc_fail(GNSSCORR_EINVAL, "fec_run: null argument");
    if (nch < 0 || nsym < 0 || pos0 < 0 || npos < 0 || stride < 0 || ndec < 0 || rowbytes < 0)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: negative count (nch %d nsym %d pos0 %d npos %d stride %d ndec %d rowbytes %d)",
                       nch, nsym, pos0, npos, stride, ndec, rowbytes);
    if (win < 2 || (win & 1) || win > GC_FEC_MAXWIN)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: win %d (even, 2..%d)", win, GC_FEC_MAXWIN);
    if (ndec > win / 2 - 6)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: ndec %d above win/2 - 6 = %d", ndec, win / 2 - 6);
    if (rowbytes < (ndec + 7) / 8)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: rowbytes %d below the %d bytes of %d bits", rowbytes, (ndec + 7) / 8, ndec);
    if (polyA < 0 || polyA > 127 || polyB < 0 || polyB > 127)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: polynomials %#x %#x (7-bit masks)", polyA, polyB);
    if (nch > 65535) return gc_fail(GNSSCORR_EINVAL, "fec_run: nch %d (at most 65535)", nch);
    if (nch == 0 || npos == 0) return GNSSCORR_OK;
    if (npos > 1 && stride < 1) return gc_fail(GNSSCORR_EINVAL, "fec_run: stride %d with %d windows", stride, npos);
    if ((long long)pos0 + (long long)(npos - 1) * stride >= (long long)nsym)
        return gc_fail(GNSSCORR_EINVAL, "fec_run: the last window ends at symbol %lld, the stream has %d",
                       (long long)pos0 + (long long)(npos - 1) * stride, nsym);
    std::lock_guard<std::mutex> lk(ctx->mtx);
    GC_HIP(hipSetDevice(ctx->device));
    const size_t nin = (size_t)nch * nsym, nout = (size_t)nch * npos * rowbytes;
    GC_RESERVE(ctx, ctx->dfec_sym, nin);
    GC_RESERVE(ctx, ctx->dfec_out, std::max(nout, (size_t)1));
    GC_HIP(hipMemcpyAsync(ctx->dfec_sym, sym, nin, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((npos + GC_FEC_WAVES - 1) / GC_FEC_WAVES, nch), block(GC_FEC_WAVES * 64);
    {
        GcTimed t(ctx, "fec_viterbi27");
        const signed char *dsym = ctx->dfec_sym;
        unsigned char *dout = ctx->dfec_out;
#define GC_FEC_LAUNCH(PARTS)                                                                                          \
    hipLaunchKernelGGL(fec_viterbi27_kernel<PARTS>, grid, block, 0, ctx->stream, dsym, nsym, pos0, npos, stride, win, \
                       ndec, (unsigned)polyA, (unsigned)polyB, dout, rowbytes)
        if (ctx->fec_parts == 1) GC_FEC_LAUNCH(1);
        else if (ctx->fec_parts == 2) GC_FEC_LAUNCH(2);
        else GC_FEC_LAUNCH(3);
#undef GC_FEC_LAUNCH
    }
    GC_HIP(hipGetLastError());
    if (nout) GC_HIP(hipMemcpyAsync(out, ctx->dfec_out, nout, hipMemcpyDeviceToHost, ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

// (tools/fec_time.py) 3: the decoder (the default); 1: forward pass only; 2: chainback only.  The rows of an ablated
// run are not decodes.
extern "C" int gnsscorr_debug_fec_parts(gnsscorr_ctx *ctx, int parts)
{
    if (!ctx || parts < 1 || parts > 3) return gc_fail(GNSSCORR_EINVAL, "debug_fec_parts: %d (1, 2 or 3)", parts);
    ctx->fec_parts = parts;
    return GNSSCORR_OK;
}
