// gnsscorr_api.hip -- C-ABI layer of libgnsscorr.so: context, IF ring in HBM and
// its ingest, channel tables, per-kernel timing, the default context.  The context
// owns every buffer, stream and event by type (gnsscorr_ctx.h): creating it makes
// the handles the trackers need, destroying it is `delete`.
// (The batched tracker's entry points live in gnsscorr_trk.hip, acquisition's in
// gnsscorr_acq.hip, the closed loop's in gnsscorr_loop.hip, the reference-named
// per-call symbols in gnsscorr_compat.hip.)
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gnsscorr_ctx.h"

static thread_local char g_err[512] = "";

int gc_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int gc_fail_hip(hipError_t e, const char *what, const char *file, int line)
{
    snprintf(g_err, sizeof(g_err), "HIP error %d (%s) in %s at %s:%d", (int)e, hipGetErrorString(e), what,
             file, line);
    return GNSSCORR_EHIP;
}

extern "C" const char *gnsscorr_last_error(void) { return g_err; }

extern "C" int gnsscorr_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the streams and events every context has from the start (the ingest's and the lock monitor's are made on first use)
static int create_handles(gnsscorr_ctx *ctx, hipStream_t stream)
{
    if (stream) ctx->stream.borrow(stream);
    else GC_TRY(ctx->stream.make());
    for (GcStream *s : {&ctx->stream_plan, &ctx->stream_tables, &ctx->stream_discover}) GC_TRY(s->make());
    GC_TRY(ctx->ev_spec.make());
    for (GcEvent *ev : {ctx->ev_plan, ctx->ev_tab, ctx->ev_used, ctx->ev_corr})
        for (int i = 0; i < 2; i++) GC_TRY(ev[i].make());
    for (GcEvent &ev : ctx->ev_burst) GC_TRY(ev.make());
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_create(gnsscorr_ctx **out, int device, void *stream)
{
    if (!out) return gc_fail(GNSSCORR_EINVAL, "gnsscorr_create: null out pointer");
    int ndev = 0;
    GC_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return gc_fail(GNSSCORR_EHIP, "gnsscorr_create: device %d not present (%d visible)", device, ndev);
    GC_HIP(hipSetDevice(device));
    gnsscorr_ctx *ctx = new gnsscorr_ctx();
    ctx->device = device;
    int rc = create_handles(ctx, (hipStream_t)stream);
    if (rc) {
        delete ctx;                        // with the handles made so far
        return rc;
    }
    *out = ctx;
    return GNSSCORR_OK;
}

// the channel set's device buffers; the next set starts from nothing
static void drop_channel_buffers(gnsscorr_ctx *ctx)
{
    ctx->acq = GcAcq();
    ctx->spec = GcSpec();
    ctx->dchan.reset(); ctx->dcodes.reset(); ctx->dfreqs.reset();
    ctx->state = GcTrkStateBuf();
    ctx->batch = GcBatch();
    ctx->out = GcTrkOut();
    ctx->loop = GcLoop();
    ctx->rx = GcRx();
    ctx->nav.off();
    ctx->lock_pending = false;
}

extern "C" void gnsscorr_destroy(gnsscorr_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    gc_quiesce(ctx, true);
    delete ctx;                        // the buffers, streams and events it owns go with it
}

extern "C" void *gnsscorr_stream(gnsscorr_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int gnsscorr_sync(gnsscorr_ctx *ctx)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    GC_HIP(hipSetDevice(ctx->device));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

// ---------------------------------------------------------------------------
// IF ring
// ---------------------------------------------------------------------------
static GcRing *ring_of(gnsscorr_ctx *ctx, int ftype)
{
    if (!ctx || ftype < 1 || ftype > 2) return nullptr;
    return &ctx->ring[ftype - 1];
}

static void retarget_rings(gnsscorr_ctx *ctx);

extern "C" int gnsscorr_ring_create(gnsscorr_ctx *ctx, int ftype, int dtype, uint64_t ringlen,
                                    void *devmem)
{
    GcRing *r = ring_of(ctx, ftype);
    if (!r) return gc_fail(GNSSCORR_EINVAL, "ring_create: bad context or ftype %d", ftype);
    if (dtype != 1 && dtype != 2) return gc_fail(GNSSCORR_EINVAL, "ring_create: dtype %d not 1 or 2", dtype);
    if (ringlen == 0 || ((uint64_t)dtype * ringlen) % 16 != 0)
        return gc_fail(GNSSCORR_EINVAL, "ring_create: dtype*ringlen must be a positive multiple of 16");
    if (devmem && ((uintptr_t)devmem & 15))
        return gc_fail(GNSSCORR_EINVAL, "ring_create: device buffer must be 16-byte aligned");
    // The channels that read this ring keep their rows, which index it by their own dtype and nsamp: the new ring must
    // be one gnsscorr_set_channels would have accepted for them (validated first: nothing is touched on failure)
    bool referenced = false;
    for (int i = 0; i < ctx->nch; i++) {
        const gnsscorr_chan_t &c = ctx->hdesc[i];
        if (c.ftype != ftype) continue;
        referenced = true;
        if (c.dtype != dtype)
            return gc_fail(GNSSCORR_EINVAL, "ring_create: channel %d: dtype %d but ring %d would hold dtype %d "
                           "(gnsscorr_set_channels comes first)", i, c.dtype, ftype, dtype);
        if (ringlen < (uint64_t)c.nsamp + 100 + 32 / c.dtype)
            return gc_fail(GNSSCORR_EINVAL, "ring_create: channel %d: ring %d (%llu samples) would be shorter than a code period (%d + 100 + %d)",
                           i, ftype, (unsigned long long)ringlen, c.nsamp, 32 / c.dtype);
    }
    GC_HIP(hipSetDevice(ctx->device));
    {
        std::lock_guard<std::mutex> lk(ctx->mtx);
        // Transfers into the old ring (ingest stream) and kernels reading it (compute stream) are over before it goes.
        // Only the compute stream reads samples, but with channels the call also rewrites their device rows, which the
        // planner, discovery and tables streams read (a look-ahead plan may still be running), and that plan was made
        // for positions of the old stream: quiesce like gnsscorr_set_channels does, which drops it.
        GC_TRY(gc_quiesce(ctx, true));
        // a running schedule holds sample positions of the old stream (next_try, acq_wrpos, the TRACK channels'
        // buffloc): it is off until the next gnsscorr_rx_start
        if (referenced) {
            ctx->rx.on = false;
            ctx->nav.off();             // its counters and frame positions are the old stream's, too
        }
        r->own.reset();
        r->mem = nullptr;
        if (devmem) {
            r->mem = (int8_t *)devmem;
        } else {
            GC_RESERVE(ctx, r->own, (size_t)dtype * ringlen);
            r->mem = r->own;
            // the zero fill is over before the first push: pushes run on the ingest stream, which nothing orders
            // behind the compute stream
            GC_HIP(hipMemsetAsync(r->mem, 0, (size_t)dtype * ringlen, ctx->stream));
            GC_HIP(hipStreamSynchronize(ctx->stream));
        }
        r->dtype = dtype;
        r->ringlen = ringlen;
        r->wrpos = 0;
    }
    retarget_rings(ctx);
    return GNSSCORR_OK;
}

// ---- ingest ----------------------------------------------------------------------------------------------
#define GC_PIN_BYTES (8u << 20)         // per staging buffer

// every step keeps what an earlier call made: a failed init is completed by the next call
static int ingest_init(gnsscorr_ctx *ctx)
{
    GcIngest &in = ctx->in;
    if (in.ready) return GNSSCORR_OK;
    GC_TRY(in.stream.make());
    for (int i = 0; i < 2; i++) {
        GC_TRY(in.pin[i].reserve(GC_PIN_BYTES));
        GC_RESERVE(ctx, in.dstage[i], GC_PIN_BYTES);
        GC_TRY(in.ev_pin[i].make());
    }
    GC_TRY(in.ev_in.make());
    in.ready = true;
    return GNSSCORR_OK;
}

// a free staging slot (waits for the transfer that last used it, never for the compute stream)
static int ingest_slot(gnsscorr_ctx *ctx, int *slot)
{
    GcIngest &in = ctx->in;
    const int s = in.pin_next;
    in.pin_next ^= 1;
    if (in.pin_busy[s]) GC_HIP(hipEventSynchronize(in.ev_pin[s]));
    in.pin_busy[s] = false;
    *slot = s;
    return GNSSCORR_OK;
}

// the compute stream reads the ring: order it behind the last transfer
int gc_ingest_fence(gnsscorr_ctx *ctx)
{
    if (ctx->in.in_pending) GC_HIP(hipStreamWaitEvent(ctx->stream, ctx->in.ev_in, 0));
    return GNSSCORR_OK;
}

int gc_ring_positions(gnsscorr_ctx *ctx, uint64_t wp_ring[2])
{
    std::lock_guard<std::mutex> lk(ctx->mtx);
    wp_ring[0] = ctx->ring[0].wrpos;
    wp_ring[1] = ctx->ring[1].wrpos;
    return gc_ingest_fence(ctx);
}

// ring bytes [pos, pos + bytes) <- device or pinned source, split at the end of the ring
static int ring_write(gnsscorr_ctx *ctx, GcRing *r, uint64_t bytepos, const void *src, uint64_t bytes, hipMemcpyKind kind)
{
    const uint64_t rb = (uint64_t)r->dtype * r->ringlen;
    const uint64_t pos = bytepos % rb;
    const uint64_t first = pos + bytes <= rb ? bytes : rb - pos;
    GC_HIP(hipMemcpyAsync(r->mem + pos, src, first, kind, ctx->in.stream));
    if (first < bytes) GC_HIP(hipMemcpyAsync(r->mem, (const int8_t *)src + first, bytes - first, kind, ctx->in.stream));
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_ring_push(gnsscorr_ctx *ctx, int ftype, const void *host, uint64_t nsamp)
{
    GcRing *r = ring_of(ctx, ftype);
    if (!r || !r->mem) return gc_fail(GNSSCORR_ESTATE, "ring_push: ring %d not created", ftype);
    if (nsamp > r->ringlen) return gc_fail(GNSSCORR_EINVAL, "ring_push: chunk larger than the ring");
    if (!host && nsamp) return gc_fail(GNSSCORR_EINVAL, "ring_push: null host buffer");
    GC_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->mtx);
    int rc = ingest_init(ctx);
    if (rc) return rc;
    const uint64_t d = (uint64_t)r->dtype;
    const int8_t *h = (const int8_t *)host;
    uint64_t done = 0, total = d * nsamp;
    while (done < total) {
        const uint64_t piece = total - done < GC_PIN_BYTES ? total - done : GC_PIN_BYTES;
        int s;
        rc = ingest_slot(ctx, &s);
        if (rc) return rc;
        memcpy(ctx->in.pin[s], h + done, piece);        // the caller's buffer is free again after this
        rc = ring_write(ctx, r, d * r->wrpos + done, ctx->in.pin[s], piece, hipMemcpyHostToDevice);
        if (rc) return rc;
        GC_HIP(hipEventRecord(ctx->in.ev_pin[s], ctx->in.stream));
        ctx->in.pin_busy[s] = true;
        done += piece;
    }
    GC_HIP(hipEventRecord(ctx->in.ev_in, ctx->in.stream));
    ctx->in.in_pending = true;
    r->wrpos += nsamp;
    return GNSSCORR_OK;
}

// ref src/rcv/stereo/stereo.c:160-205 (lut1 / lut2) and src/rcv/rtlsdr/rtlsdr.c:136-143
__global__ void unpack_stereo_kernel(const uint8_t *__restrict__ src, uint64_t n, int8_t *__restrict__ r1, uint64_t len1,
                                     uint64_t pos1, int8_t *__restrict__ r2, uint64_t len2, uint64_t pos2)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned b = src[i];
    // BASELUT1 = {-3,-1,+1,+3}; BASELUT2 = {+1,+3,+5,+7,-7,-5,-3,-1}
    if (r1) r1[(pos1 + i) % len1] = (int8_t)(2 * (int)((b >> 6) & 3) - 3);
    if (r2) {
        const int vi = (b >> 3) & 7, vq = b & 7;
        const uint64_t k = (pos2 + i) % len2;
        r2[2 * k] = (int8_t)(vi < 4 ? 2 * vi + 1 : 2 * vi - 15);
        r2[2 * k + 1] = (int8_t)(vq < 4 ? 2 * vq + 1 : 2 * vq - 15);
    }
}

__global__ void unpack_rtlsdr_kernel(const uint8_t *__restrict__ src, uint64_t nbytes, int8_t *__restrict__ ring,
                                     uint64_t ringbytes, uint64_t bytepos)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nbytes) return;
    // (char)(buf[i] - 127.5): the double is truncated toward zero
    const int v = (int)src[i];
    ring[(bytepos + i) % ringbytes] = (int8_t)(v >= 128 ? v - 128 : v - 127);
}

extern "C" int gnsscorr_ring_push_packed(gnsscorr_ctx *ctx, int format, const void *host, uint64_t nsamp)
{
    if (!ctx || (!host && nsamp)) return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: bad arguments");
    if (format != GNSSCORR_FMT_STEREO && format != GNSSCORR_FMT_RTLSDR)
        return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: format %d", format);
    GcRing *r1 = &ctx->ring[0], *r2 = &ctx->ring[1];
    if (format == GNSSCORR_FMT_STEREO) {
        if (!r1->mem && !r2->mem) return gc_fail(GNSSCORR_ESTATE, "ring_push_packed: no ring created");
        if (r1->mem && r1->dtype != 1) return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: Stereo front end 1 is real (ring 1 must be dtype 1)");
        if (r2->mem && r2->dtype != 2) return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: Stereo front end 2 is IQ (ring 2 must be dtype 2)");
        if ((r1->mem && nsamp > r1->ringlen) || (r2->mem && nsamp > r2->ringlen))
            return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: chunk larger than the ring");
    } else {
        if (!r1->mem || r1->dtype != 2) return gc_fail(GNSSCORR_ESTATE, "ring_push_packed: RTL-SDR feeds ring 1 as IQ (dtype 2)");
        if (nsamp > r1->ringlen) return gc_fail(GNSSCORR_EINVAL, "ring_push_packed: chunk larger than the ring");
    }
    GC_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->mtx);
    int rc = ingest_init(ctx);
    if (rc) return rc;
    const uint8_t *h = (const uint8_t *)host;
    const uint64_t total = format == GNSSCORR_FMT_STEREO ? nsamp : 2 * nsamp;       // packed bytes
    uint64_t done = 0;
    while (done < total) {
        const uint64_t piece = total - done < GC_PIN_BYTES ? total - done : GC_PIN_BYTES;
        int s;
        rc = ingest_slot(ctx, &s);
        if (rc) return rc;
        memcpy(ctx->in.pin[s], h + done, piece);
        GC_HIP(hipMemcpyAsync(ctx->in.dstage[s], ctx->in.pin[s], piece, hipMemcpyHostToDevice, ctx->in.stream));
        const unsigned blocks = (unsigned)((piece + 255) / 256);
        if (format == GNSSCORR_FMT_STEREO)
            hipLaunchKernelGGL(unpack_stereo_kernel, dim3(blocks), dim3(256), 0, ctx->in.stream, ctx->in.dstage[s], piece,
                               r1->mem, r1->mem ? r1->ringlen : 1, r1->wrpos + done, r2->mem, r2->mem ? r2->ringlen : 1,
                               r2->wrpos + done);
        else
            hipLaunchKernelGGL(unpack_rtlsdr_kernel, dim3(blocks), dim3(256), 0, ctx->in.stream, ctx->in.dstage[s], piece,
                               r1->mem, 2 * r1->ringlen, 2 * r1->wrpos + done);
        GC_HIP(hipGetLastError());
        GC_HIP(hipEventRecord(ctx->in.ev_pin[s], ctx->in.stream));
        ctx->in.pin_busy[s] = true;
        done += piece;
    }
    GC_HIP(hipEventRecord(ctx->in.ev_in, ctx->in.stream));
    ctx->in.in_pending = true;
    if (format == GNSSCORR_FMT_STEREO) {
        if (r1->mem) r1->wrpos += nsamp;
        if (r2->mem) r2->wrpos += nsamp;
    } else {
        r1->wrpos += nsamp;
    }
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_ring_read(gnsscorr_ctx *ctx, int ftype, uint64_t buffloc, int n, void *host)
{
    GcRing *r = ring_of(ctx, ftype);
    if (!r || !r->mem) return gc_fail(GNSSCORR_ESTATE, "ring_read: ring %d not created", ftype);
    if (n <= 0 || (uint64_t)n > r->ringlen || !host) return gc_fail(GNSSCORR_EINVAL, "ring_read: n %d", n);
    GC_HIP(hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lk(ctx->mtx);
    if (ctx->in.in_pending) GC_HIP(hipEventSynchronize(ctx->in.ev_in));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    // ref src/sdrrcv.c:508-521
    const uint64_t d = (uint64_t)r->dtype, rb = d * r->ringlen, pos = (d * buffloc) % rb, nb = d * (uint64_t)n;
    const uint64_t first = pos + nb <= rb ? nb : rb - pos;
    GC_HIP(hipMemcpy(host, r->mem + pos, first, hipMemcpyDeviceToHost));
    if (first < nb) GC_HIP(hipMemcpy((int8_t *)host + first, r->mem, nb - first, hipMemcpyDeviceToHost));
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_ring_commit(gnsscorr_ctx *ctx, int ftype, uint64_t nsamp)
{
    GcRing *r = ring_of(ctx, ftype);
    if (!r || !r->mem) return gc_fail(GNSSCORR_ESTATE, "ring_commit: ring %d not created", ftype);
    std::lock_guard<std::mutex> lk(ctx->mtx);
    r->wrpos += nsamp;
    return GNSSCORR_OK;
}

extern "C" uint64_t gnsscorr_ring_wrpos(gnsscorr_ctx *ctx, int ftype)
{
    GcRing *r = ring_of(ctx, ftype);
    if (!r) return 0;
    std::lock_guard<std::mutex> lk(ctx->mtx);
    return r->wrpos;
}

extern "C" void *gnsscorr_ring_devptr(gnsscorr_ctx *ctx, int ftype)
{
    GcRing *r = ring_of(ctx, ftype);
    return r ? (void *)r->mem : nullptr;
}

// ---------------------------------------------------------------------------
// channels
// ---------------------------------------------------------------------------
static int upload_channels(gnsscorr_ctx *ctx)
{
    GC_HIP(hipMemcpyAsync(ctx->dchan, ctx->hchan.data(), sizeof(GcChan) * ctx->nch, hipMemcpyHostToDevice,
                          ctx->stream));
    GC_HIP(hipStreamSynchronize(ctx->stream));
    return GNSSCORR_OK;
}

static void retarget_rings(gnsscorr_ctx *ctx)
{
    if (!ctx->nch || !ctx->dchan) return;
    for (int i = 0; i < ctx->nch; i++) {
        const GcRing &r = ctx->ring[ctx->hdesc[i].ftype - 1];
        ctx->hchan[i].ring = r.mem;
        ctx->hchan[i].ringlen = r.ringlen;
    }
    upload_channels(ctx);
}

// acquisition grid = channels that share ring, sample grid, Doppler bins, coherent integration, bit-edge step and
// code-Doppler shifts (the same f_cf, and where it is not 0 the same f_if and foffset: with the rest of the key their
// shift tables agree, gc_acq_shifts): they share the forward spectra.  Grids are numbered in the order of their first
// channel.
static void assign_acq_grids(gnsscorr_ctx *ctx)
{
    int ngrid = 0;
    for (int i = 0; i < ctx->nch; i++) {
        const gnsscorr_chan_t &d = ctx->hdesc[i];
        GcChan &g = ctx->hchan[i];
        g.grid = -1;
        for (int j = 0; j < i && g.grid < 0; j++) {
            const gnsscorr_chan_t &o = ctx->hdesc[j];
            if (o.ftype == d.ftype && o.dtype == d.dtype && o.nsamp == d.nsamp && o.nfreq == d.nfreq &&
                o.intg == d.intg && o.ti == d.ti && o.nfft == d.nfft && ctx->hchan[j].ncoh == g.ncoh &&
                ctx->hchan[j].estep == g.estep && ctx->hfcf[j] == ctx->hfcf[i] &&
                (ctx->hfcf[i] == 0.0 || (o.f_if == d.f_if && o.foffset == d.foffset)) &&
                !memcmp(o.freq, d.freq, sizeof(double) * d.nfreq))
                g.grid = ctx->hchan[j].grid;
        }
        if (g.grid < 0) g.grid = ngrid++;
    }
}

extern "C" int gnsscorr_set_channels(gnsscorr_ctx *ctx, int nch, const gnsscorr_chan_t *ch)
{
    if (!ctx || nch <= 0 || !ch) return gc_fail(GNSSCORR_EINVAL, "set_channels: bad arguments");
    GC_HIP(hipSetDevice(ctx->device));
    // validate first: nothing is touched on failure
    for (int i = 0; i < nch; i++) {
        const gnsscorr_chan_t &c = ch[i];
        if (c.dtype != 1 && c.dtype != 2) return gc_fail(GNSSCORR_EINVAL, "channel %d: dtype %d", i, c.dtype);
        if (c.ftype != 1 && c.ftype != 2) return gc_fail(GNSSCORR_EINVAL, "channel %d: ftype %d", i, c.ftype);
        if (c.clen <= 0 || c.clen > 1023 || !c.code)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: code length %d (1..1023 supported)", i, c.clen);
        if (c.corrn < 1 || 1 + 2 * c.corrn > GNSSCORR_MAXTAPS || !c.corrp)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: corrn %d (1..16 supported)", i, c.corrn);
        if (c.corrn != ch[0].corrn)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: corrn differs (one [TRACK] CORRN per receiver)", i);
        if (c.nfreq < 1 || c.nfreq > GNSSCORR_MAXFREQ || !c.freq)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: nfreq %d", i, c.nfreq);
        // tracking takes any period length the int32 accumulators hold; acquisition (gnsscorr_acq_run)
        // additionally needs nsamp <= 16384 for its 32768-point transform and says so itself
        if (c.nsamp <= 0 || c.nsamp > 262144)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: nsamp %d (1..262144 supported)", i, c.nsamp);
        for (int k = 0; k < c.corrn; k++)
            if (c.corrp[k] <= 0 || (k && c.corrp[k] <= c.corrp[k - 1]))
                return gc_fail(GNSSCORR_EINVAL, "channel %d: corrp must be positive and increasing", i);
        if (c.corrp[c.corrn - 1] > 64)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: outermost tap at %d samples (<= 64 supported)", i, c.corrp[c.corrn - 1]);
        const GcRing &r = ctx->ring[c.ftype - 1];
        if (!r.mem) return gc_fail(GNSSCORR_ESTATE, "channel %d: ring %d not created", i, c.ftype);
        if (r.dtype != c.dtype)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: dtype %d but ring %d holds dtype %d", i, c.dtype, c.ftype, r.dtype);
        // a code period (the reference's scratch is nsamp + 100 samples, ref src/sdrtrk.c:23) plus the 16-byte
        // groups around it must fit the ring once; acquisition looks (intg + 1) periods back
        if (r.ringlen < (uint64_t)c.nsamp + 100 + 32 / c.dtype)
            return gc_fail(GNSSCORR_EINVAL, "channel %d: ring %d (%llu samples) is shorter than a code period (%d + 100 + %d)",
                           i, c.ftype, (unsigned long long)r.ringlen, c.nsamp, 32 / c.dtype);
    }
    GC_TRY(gc_quiesce(ctx));
    drop_channel_buffers(ctx);

    ctx->nch = nch;
    ctx->loop.isset.assign(nch, 0);
    ctx->hdesc.assign(ch, ch + nch);
    ctx->hcode.resize(nch);
    ctx->hfreq.resize(nch);
    ctx->hcorrp.resize(nch);
    ctx->hchan.assign(nch, GcChan());
    ctx->hfcf.assign(nch, 0.0);
    std::vector<int8_t> codes((size_t)nch * GC_CODEBLOCK, 0);
    std::vector<double> freqs;
    ctx->ntap = 1 + 2 * ch[0].corrn;
    ctx->smax_max = 0;
    ctx->max_n = 0;
    for (bool &h : ctx->have_dtype) h = false;
    for (int i = 0; i < nch; i++) {
        gnsscorr_chan_t &d = ctx->hdesc[i];
        ctx->hcode[i].assign(d.code, d.code + d.clen);
        ctx->hfreq[i].assign(d.freq, d.freq + d.nfreq);
        ctx->hcorrp[i].assign(d.corrp, d.corrp + d.corrn);
        d.code = ctx->hcode[i].data();
        d.freq = ctx->hfreq[i].data();
        d.corrp = ctx->hcorrp[i].data();
        GcChan &g = ctx->hchan[i];
        gc_build_codeblock(d.code, d.clen, codes.data() + (size_t)i * GC_CODEBLOCK, &g.nedge, &g.pm1);
        ctx->have_dtype[d.dtype] = true;
        g.dtype = d.dtype; g.clen = d.clen; g.nsamp = d.nsamp; g.nsampchip = d.nsampchip;
        gc_chan_set_taps(g, d.corrp, d.corrn);
        g.ti = d.ti; g.f_sf = d.f_sf; g.crate = d.crate; g.ctime = d.ctime;
        g.nfreq = d.nfreq; g.intg = d.intg; g.nfft = d.nfft;
        g.freq_off = (int)freqs.size();
        freqs.insert(freqs.end(), d.freq, d.freq + d.nfreq);
        g.ncoh = 1;
        g.estep = 0;
        g.nref = 0;
        if (g.smax > ctx->smax_max) ctx->smax_max = g.smax;
        if (d.nsamp + 100 > ctx->max_n) ctx->max_n = d.nsamp + 100;   // ref src/sdrtrk.c:23
    }
    GC_RESERVE(ctx, ctx->dchan, nch);
    GC_RESERVE(ctx, ctx->dcodes, codes.size());
    GC_RESERVE(ctx, ctx->dfreqs, freqs.size());
    for (int i = 0; i < 2; i++) {
        GC_RESERVE(ctx, ctx->state.buf[i], nch);
        GC_HIP(hipMemsetAsync(ctx->state.buf[i], 0, sizeof(GcTrkState) * nch, ctx->stream));
    }
    GC_RESERVE(ctx, ctx->loop.dloop, nch);
    GC_HIP(hipMemsetAsync(ctx->loop.dloop, 0, sizeof(gnsscorr_loop_t) * nch, ctx->stream));
    GC_RESERVE(ctx, ctx->loop.ddone, nch);
    GC_HIP(hipMemsetAsync(ctx->loop.ddone, 0, sizeof(int) * nch, ctx->stream));
    GC_RESERVE(ctx, ctx->loop.dwrpos, nch);                      // (uploaded by every run before its first tail)
    GC_HIP(hipMemcpyAsync(ctx->dcodes, codes.data(), codes.size(), hipMemcpyHostToDevice, ctx->stream));
    GC_HIP(hipMemcpyAsync(ctx->dfreqs, freqs.data(), sizeof(double) * freqs.size(), hipMemcpyHostToDevice,
                          ctx->stream));
    for (int i = 0; i < nch; i++) {
        const GcRing &r = ctx->ring[ctx->hdesc[i].ftype - 1];
        ctx->hchan[i].ring = r.mem;
        ctx->hchan[i].ringlen = r.ringlen;
        ctx->hchan[i].code = ctx->dcodes + (size_t)i * GC_CODEBLOCK;
    }
    assign_acq_grids(ctx);
    return upload_channels(ctx);
}

// The per-channel acquisition settings below take a channel range and its values (gc_chan_range, gnsscorr_ctx.h)

// A setting the forward spectra depend on: once nothing is in flight, write() changes the host channel table, the grids
// are numbered again, the table goes up, and what acquisition had prepared for the old setting (code spectra, carrier
// tables, forward spectra, cached lists, the last results) is dropped: the next search prepares again.
template <class Write>
static int acq_change_grids(gnsscorr_ctx *ctx, Write write)
{
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_quiesce(ctx));
    write();
    assign_acq_grids(ctx);
    ctx->acq = GcAcq();
    return upload_channels(ctx);
}

// Coherent integration per channel (include/gnsscorr.h)
extern "C" int gnsscorr_acq_set_coherent(gnsscorr_ctx *ctx, int ch0, int nch, const int *ncoh)
{
    GC_TRY(gc_chan_range("acq_set_coherent", ctx, ch0, nch, ncoh));
    for (int i = 0; i < nch; i++) {
        const int intg = ctx->hchan[ch0 + i].intg;
        if (ncoh[i] < 1 || ncoh[i] > GNSSCORR_MAXCOH || intg % ncoh[i] != 0)
            return gc_fail(GNSSCORR_EINVAL, "acq_set_coherent: channel %d: ncoh %d (1..%d, a divisor of intg %d)", ch0 + i,
                           ncoh[i], GNSSCORR_MAXCOH, intg);
    }
    return acq_change_grids(ctx, [&] {
        for (int i = 0; i < nch; i++) {
            ctx->hchan[ch0 + i].ncoh = ncoh[i];
            ctx->hchan[ch0 + i].estep = 0;      // the hypotheses depend on ncoh: gnsscorr_acq_set_bitedge comes after
        }
    });
}

extern "C" int gnsscorr_acq_get_coherent(gnsscorr_ctx *ctx, int ch0, int nch, int *ncoh)
{
    GC_TRY(gc_chan_range("acq_get_coherent", ctx, ch0, nch, ncoh));
    for (int i = 0; i < nch; i++) ncoh[i] = ctx->hchan[ch0 + i].ncoh;
    return GNSSCORR_OK;
}

// Bit-edge hypotheses per channel (include/gnsscorr.h)
extern "C" int gnsscorr_acq_set_bitedge(gnsscorr_ctx *ctx, int ch0, int nch, const int *estep)
{
    GC_TRY(gc_chan_range("acq_set_bitedge", ctx, ch0, nch, estep));
    // the hypotheses are served by the 32768-point transform only, and the transform length is the context's
    for (int i = 0; i < ctx->nch; i++)
        if (ctx->hchan[i].nsamp > 16384)
            return gc_fail(GNSSCORR_EINVAL, "acq_set_bitedge: channel %d: nsamp %d puts the context on the 65536-point "
                           "transform, which has no bit-edge hypotheses", i, ctx->hchan[i].nsamp);
    for (int i = 0; i < nch; i++) {
        const int ncoh = ctx->hchan[ch0 + i].ncoh;
        if (estep[i] < 0 || (estep[i] >= 1 && (ncoh < 2 || estep[i] >= ncoh)))
            return gc_fail(GNSSCORR_EINVAL, "acq_set_bitedge: channel %d: estep %d (0, or 1..ncoh-1 with ncoh %d >= 2)",
                           ch0 + i, estep[i], ncoh);
    }
    return acq_change_grids(ctx, [&] {
        for (int i = 0; i < nch; i++) ctx->hchan[ch0 + i].estep = estep[i];
    });
}

extern "C" int gnsscorr_acq_get_bitedge(gnsscorr_ctx *ctx, int ch0, int nch, int *estep)
{
    GC_TRY(gc_chan_range("acq_get_bitedge", ctx, ch0, nch, estep));
    for (int i = 0; i < nch; i++) estep[i] = ctx->hchan[ch0 + i].estep;
    return GNSSCORR_OK;
}

// Code-Doppler compensation per channel (include/gnsscorr.h); the shift tables are acq_prepare's
extern "C" int gnsscorr_acq_set_codedoppler(gnsscorr_ctx *ctx, int ch0, int nch, const double *f_cf)
{
    GC_TRY(gc_chan_range("acq_set_codedoppler", ctx, ch0, nch, f_cf));
    for (int i = 0; i < nch; i++)
        if (!std::isfinite(f_cf[i]) || f_cf[i] < 0.0)
            return gc_fail(GNSSCORR_EINVAL, "acq_set_codedoppler: channel %d: f_cf %g (0 for off, or a finite carrier in Hz)",
                           ch0 + i, f_cf[i]);
    return acq_change_grids(ctx, [&] {
        for (int i = 0; i < nch; i++) ctx->hfcf[ch0 + i] = f_cf[i];
    });
}

extern "C" int gnsscorr_acq_get_codedoppler(gnsscorr_ctx *ctx, int ch0, int nch, double *f_cf)
{
    GC_TRY(gc_chan_range("acq_get_codedoppler", ctx, ch0, nch, f_cf));
    for (int i = 0; i < nch; i++) f_cf[i] = ctx->hfcf[ch0 + i];
    return GNSSCORR_OK;
}

// Carrier refinement per channel (include/gnsscorr.h).  The forward spectra do not depend on it: the grids keep their
// numbers, and what acquisition has prepared and the last search's results stay.
extern "C" int gnsscorr_acq_set_refine(gnsscorr_ctx *ctx, int ch0, int nch, const int *nref)
{
    GC_TRY(gc_chan_range("acq_set_refine", ctx, ch0, nch, nref));
    for (int i = 0; i < nch; i++) {
        const int intg = ctx->hchan[ch0 + i].intg, top = intg < GNSSCORR_MAXCOH ? intg : GNSSCORR_MAXCOH;
        if (nref[i] < 0 || nref[i] == 1 || nref[i] > top)
            return gc_fail(GNSSCORR_EINVAL, "acq_set_refine: channel %d: nref %d (0, or 2..%d = min(intg %d, %d))", ch0 + i,
                           nref[i], top, intg, GNSSCORR_MAXCOH);
    }
    GC_HIP(hipSetDevice(ctx->device));
    GC_TRY(gc_quiesce(ctx));
    for (int i = 0; i < nch; i++) ctx->hchan[ch0 + i].nref = nref[i];
    return upload_channels(ctx);
}

extern "C" int gnsscorr_acq_get_refine(gnsscorr_ctx *ctx, int ch0, int nch, int *nref)
{
    GC_TRY(gc_chan_range("acq_get_refine", ctx, ch0, nch, nref));
    for (int i = 0; i < nch; i++) nref[i] = ctx->hchan[ch0 + i].nref;
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_num_channels(gnsscorr_ctx *ctx) { return ctx ? ctx->nch : 0; }

// hipMalloc; with gnsscorr_debug_poison on, the new buffer is then filled with the poison byte (and the fill is over
// before this returns, so that it cannot race any later write on another stream)
int gc_dev_alloc(gnsscorr_ctx *ctx, void **p, size_t bytes)
{
    GC_HIP(hipMalloc(p, bytes));
    if (ctx->poison >= 0) {
        GC_HIP(hipMemsetAsync(*p, ctx->poison, bytes, ctx->stream));
        GC_HIP(hipStreamSynchronize(ctx->stream));
    }
    return GNSSCORR_OK;
}

// (tests) byte 0..255: every device buffer the context allocates from now on (tracking, closed-loop, acquisition
// scratch, channel tables) starts out filled with it instead of whatever memory held; -1: off (the default).
// Owned rings keep their zero fill.
extern "C" int gnsscorr_debug_poison(gnsscorr_ctx *ctx, int byte)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "debug_poison: null context");
    if (byte < -1 || byte > 255) return gc_fail(GNSSCORR_EINVAL, "debug_poison: byte %d (0..255, or -1 for off)", byte);
    ctx->poison = byte;
    return GNSSCORR_OK;
}

// ---------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------
static void drain_timers(gnsscorr_ctx *ctx)
{
    for (auto &kv : ctx->timers) {
        for (auto &p : kv.second.pending) {
            float ms = 0.f;
            if (hipEventSynchronize(p.second) == hipSuccess &&
                hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
                kv.second.total_ms += ms;
                kv.second.launches++;
            }
        }
        kv.second.pending.clear();
    }
}

extern "C" int gnsscorr_timing_enable(gnsscorr_ctx *ctx, int on)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    ctx->timing = on == 2 ? 2 : (on != 0);
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_timing_reset(gnsscorr_ctx *ctx)
{
    if (!ctx) return gc_fail(GNSSCORR_EINVAL, "null context");
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    drain_timers(ctx);
    ctx->timers.clear();
    return GNSSCORR_OK;
}

extern "C" int gnsscorr_timing_read(gnsscorr_ctx *ctx, const char *kernel, double *total_ms, int *launches)
{
    if (!ctx || !kernel) return gc_fail(GNSSCORR_EINVAL, "timing_read: bad arguments");
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    drain_timers(ctx);
    auto it = ctx->timers.find(kernel);
    if (total_ms) *total_ms = it == ctx->timers.end() ? 0.0 : it->second.total_ms;
    if (launches) *launches = it == ctx->timers.end() ? 0 : it->second.launches;
    return GNSSCORR_OK;
}

// ---------------------------------------------------------------------------
// process-wide context for the reference-named per-call symbols
// ---------------------------------------------------------------------------
extern "C" gnsscorr_ctx *gnsscorr_default_ctx(void)
{
    static std::mutex m;
    static gnsscorr_ctx *g = nullptr;
    std::lock_guard<std::mutex> lk(m);
    if (!g) {
        const char *e = getenv("GNSSCORR_DEVICE");
        int dev = e ? atoi(e) : 0;
        if (gnsscorr_create(&g, dev, nullptr) != GNSSCORR_OK) {
            fprintf(stderr, "error: gnsscorr: %s\n", gnsscorr_last_error());
            g = nullptr;
        }
    }
    return g;
}
