// gnsscorr_lut.h -- the reference's carrier look-up table and the wipe-off of one sample with it (mixcarr(), ref
// src/sdrcmn.c:633-669), and where a span's sample is in a ring.  Device code, for the .hip units that wipe a carrier off: the arrays are static, so each of them
// has its own constant-memory copy of the table.
#pragma once

#include <hip/hip_runtime.h>

// cost[i] = floor(32 cos(2 pi i/32) + 0.5), sint[i] likewise (ref src/sdrcmn.c:643-648)
static __constant__ signed char gcCos32[32] = {32, 31, 30, 27, 23, 18, 12, 6, 0, -6, -12, -18, -23, -27, -30, -31,
                                               -32, -31, -30, -27, -23, -18, -12, -6, 0, 6, 12, 18, 23, 27, 30, 31};
static __constant__ signed char gcSin32[32] = {0, 6, 12, 18, 23, 27, 30, 31, 32, 31, 30, 27, 23, 18, 12, 6,
                                               0, -6, -12, -18, -23, -27, -30, -31, -32, -31, -30, -27, -23, -18, -12, -6};

// Ring position of sample s of a span that starts at `base` (< ringlen) and is no longer than the ring, so that it wraps
// at most once.  Acquisition's spans: (ncoh + 1)*nsamp (acq_fwd) and nref*nsamp (acq_prompt) samples, neither above the
// (intg + 1)*nsamp its driver checks the ring against.
static __device__ __forceinline__ uint64_t gc_span_pos(uint64_t base, int s, uint64_t ringlen)
{
    uint64_t pos = base + (uint64_t)s;
    if (pos >= ringlen) pos -= ringlen;
    return pos;
}

// One sample wiped off at LUT index idx (ref src/sdrcmn.c:652-664): (I, Q) = (cos, sin) * d for a real sample d
// (dtype 1), (cos + i sin) * (d.x + i d.y) for an IQ pair (dtype 2).  The caller loads the sample its own way:
// load_iq() returns the pair as an int2, load_re() the real sample; only the one the dtype asks for is called.
template <class LoadIQ, class LoadRe>
static __device__ __forceinline__ void gc_wipeoff(int idx, int dtype, LoadIQ load_iq, LoadRe load_re, int &I, int &Q)
{
    const int cs_ = gcCos32[idx], sn_ = gcSin32[idx];
    if (dtype == 2) {
        const int2 d = load_iq();
        I = cs_ * d.x - sn_ * d.y;
        Q = sn_ * d.x + cs_ * d.y;
    } else {
        const int d0 = load_re();
        I = cs_ * d0;
        Q = sn_ * d0;
    }
}
