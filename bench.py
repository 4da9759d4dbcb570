#!/usr/bin/env python3
"""bench.py -- throughput of the GNSS correlation hot path on MI355X.

Contract (one JSON line on rank 0):
  metric  "correlations/sec (1 ms coh) + x real-time, 32-SV L1CA @16.368 Msps"  (BASELINE.json)
  step    one pass of the tracking hot path over one batch: 32 GPS L1CA channels x
          `--inner` launches of `--epochs` code periods (1 ms coherent each), 5-tap E/P/L correlators
          with carrier wipe-off, int8 IQ at 16.368 Msps (BASELINE configs[2]); planner + correlator +
          cumsumcorr kernels, IF samples already resident in the HBM ring.  Frequencies are held over a
          launch (OPEN LOOP: the correlator's throughput); the NCO chain is the reference's, bit for bit.
  value   tap-correlations per second, whole job (all ranks), of that open-loop pass; x_realtime =
          signal-ms processed per wall-ms for the whole 32-SV set; ms_per_step = wall ms of one timed step.

A plain run sets up, warms up, times `--steps` steps and prints the line.  `--dump-outputs DIR` then also writes
what the last timed step computed (dump_outputs()).  Everything below runs only with `--full`:
  also    "kernels_ms_per_launch": HIP events around every kernel of two more steps; "integrity": the timed
          launches' ring and NCO-table checks, channel 0 of one more launch against the CPU oracle; "gpu_clocks".
  also    "host_fed", "host_fed_sharded": the IF stream from host memory.
  also    "closed_loop": the same 32 channels with cumsumcorr + pll + dll on the device
          (gnsscorr_trk_run_loop), x real time with a filter update every period (before nav bit sync,
          ref src/sdrmain.c:272-276) and every 10 periods (after, :277-302).
  also    "acquisition": BASELINE configs[1] (32-SV cold search, 71 Doppler bins x 10 x 1 ms) timed
          the same way in the same run; "roofline" for the dominant kernel (trk_corr) and
          "rooflines" for the others; "cpu_baseline": the CPU oracle on the host cores.

N > 1 (launched by torch.distributed.run, one rank per GPU): weak scaling in channels -- every
rank tracks its own 32 channels on the same IF stream; rank 0 owns the stream and every chunk is
broadcast once over RCCL/xGMI into every rank's HBM ring, two chunks ahead of the batch that is being
correlated (ShardedEngine, erlangnetwork-gnsslib-sdr_amd/multigpu.py).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

F_SF = 16.368e6
NSAMP = 16368
NCH = 32
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
METRIC = "correlations/sec (1 ms coh) + x real-time, 32-SV L1CA @16.368 Msps"


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)


def pmc_traffic(kernel_prefix):
    """HBM-side bytes per launch of a kernel, from the committed rocprofv3 PMC passes of this same
    workload (separate --pmc FETCH_SIZE / WRITE_SIZE runs, tools/prof.sh; profiles/README.md).
    gfx950 correction per MI355X_MICROARCH.md: FETCH_SIZE tallies wide reads at half their bytes."""
    import glob
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r*", "*_pmc_fetch_write.json")))
    if not files:
        return None, None
    try:
        d = json.load(open(files[-1]))
        f = [v for k, v in d["FETCH_SIZE_KB_per_dispatch"].items() if k.startswith(kernel_prefix)]
        w = [v for k, v in d["WRITE_SIZE_KB_per_dispatch"].items() if k.startswith(kernel_prefix)]
        if not f or not w:
            return None, None
        return (2.0 * f[0] + w[0]) * 1024.0, os.path.relpath(files[-1], os.path.dirname(os.path.abspath(__file__)))
    except Exception:
        return None, None


def make_signal(gc, synth, nms, seed):
    """nms milliseconds of int8 IQ with ~10 of PRN 1..32 present; cached in /tmp."""
    cache = f"/tmp/gnsscorr_if_{nms}ms_{seed}.npy"
    if os.path.exists(cache):
        try:
            data = np.load(cache)
            if data.shape == (nms * NSAMP, 2) and data.dtype == np.int8:
                return data, synth.default_sats(list(range(1, 33)), seed=seed)
        except Exception:
            pass
    codes = {p: gc.gencode(p, gc.CTYPE_L1CA) for p in range(1, 33)}
    sats = synth.default_sats(list(range(1, 33)), seed=seed)
    t0 = time.time()
    data = synth.make_if(codes, nms * NSAMP, f_sf=F_SF, f_if=0.0, dtype=2, sats=sats, seed=seed)
    log(f"synthetic IF: {nms} ms generated in {time.time() - t0:.1f} s")
    try:                                            # (whole or not at all: another run may be reading it)
        tmp = f"{cache}.{os.getpid()}.tmp"
        with open(tmp, "wb") as f:
            np.save(f, data)
        os.replace(tmp, cache)
    except Exception:
        pass
    return data, sats


def dump_outputs(out_dir, eng, cap_bytes=64 << 20, seed=0):
    """What the last timed step computed, as a caller of the tracking path receives it, in float64: the E/P/L sums of
    its last launch (trk_II, trk_QQ: channel x period x tap, gnsscorr_trk_fetch), the samples of every period
    (trk_nsamp: channel x period) and the channels' NCO state after it (state_<field>: one value per channel).  Over
    cap_bytes the periods are a fixed, seeded sample, listed in trk_periods."""
    II, QQ, ns = eng.trk_fetch()
    st = eng.trk_get_state()
    nch, ne, nt = II.shape
    periods = np.arange(ne)
    per_period = nch * (2 * nt + 1) * 8
    if ne * per_period > cap_bytes - (1 << 20):
        keep = (cap_bytes - (1 << 20)) // per_period
        periods = np.sort(np.random.default_rng(seed).choice(ne, size=keep, replace=False))
    arrays = {"trk_II": II[:, periods], "trk_QQ": QQ[:, periods], "trk_nsamp": ns[:, periods],
              "trk_periods": periods}
    for k in ("carrfreq", "codefreq", "remcode", "remcarr", "buffloc"):
        arrays["state_" + k] = np.array([s[k] for s in st])
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))
    return sorted(arrays)


def channel_set(gc, rank):
    """32 channels per rank: PRN 1..32 on rank 0 (bin/gnss-sdrcli.ini:5-9), the next C/A PRNs of the
    210-entry table on the other ranks (weak scaling in channels)."""
    prns = [((32 * rank + i) % 210) + 1 for i in range(NCH)]
    corrn = int(os.environ.get("BENCH_CORRN", "2"))      # (side experiments: 6 = the shipped 13-tap front-end files)
    return [gc.Channel(p, dtype=2, f_if=0.0, corrn=corrn, corrd=3, corrp=3) for p in prns]


def gpu_clocks():
    """Clock state of the card as rocm-smi reports it (None when it cannot be read here)."""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
        d = json.loads(r.stdout)
        k = sorted(d)[0]
        return {a: b for a, b in d[k].items() if "sclk" in a.lower() or "mclk" in a.lower()}
    except Exception:
        return None


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_tracking(orc, data, ringlen, chans, states, seconds_budget=12.0):
    """The oracle's literal sdrtracking()/correlator() (one thread per channel like the reference's
    sdrthread, ref src/sdrmain.c:144-149) on the host cores, bounded sample."""
    from concurrent.futures import ThreadPoolExecutor
    ncores = min(len(chans), os.cpu_count() or 1)
    L = orc.lib()
    ring = orc.make_ring(data, ringlen, ringlen)

    def run(i, nepoch):
        c, st = chans[i], states[i]
        o = orc.make_chan(c.prn, dtype=2, f_if=0.0, corrn=2, corrd=3, corrp=3)
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = st["carrfreq"], st["codefreq"], st["remcode"], st["remcarr"]
        b = st["buffloc"]
        for _ in range(nepoch):
            L.orc_sdrtracking(C.byref(o), C.byref(ring), b)
            b += o.currnsamp
        return nepoch

    t0 = time.time()
    run(0, 20)
    per_call = (time.time() - t0) / 20
    nepoch = int(max(20, min(2000, seconds_budget / (per_call * len(chans) / ncores))))
    t0 = time.time()
    with ThreadPoolExecutor(ncores) as ex:
        list(ex.map(lambda i: run(i, nepoch), range(len(chans))))
    dt = time.time() - t0
    ntap = chans[0].ntap
    n1 = int(max(50, min(4000, 3.0 / per_call)))         # one core, one channel
    t1 = time.time()
    run(0, n1)
    dt1 = time.time() - t1
    return dict(value=len(chans) * nepoch * ntap / dt, unit="correlations/s", cores=ncores, cpu=cpu_model(), kind="port",
                sample=f"{len(chans)} channels x {nepoch} epochs x {ntap} taps, oracle sdrtracking()/correlator() with the "
                       f"reference's loops (literal NCOs, dot_23/dot_22 shape; one thread per channel), {dt:.1f} s wall",
                x_realtime=nepoch / dt / 1000.0,
                one_core={"value": n1 * ntap / dt1, "unit": "correlations/s", "us_per_correlator_call": dt1 / n1 * 1e6,
                          "sample": f"1 channel x {n1} epochs on one core, {dt1:.1f} s"})


def cpu_baseline_acq(orc, data, ringlen, wrpos, chans, seconds_budget=12.0):
    from concurrent.futures import ThreadPoolExecutor
    ncores = min(len(chans), os.cpu_count() or 1)
    L = orc.lib()
    o0 = orc.make_chan(chans[0].prn, dtype=2, f_if=0.0)
    n, nf = o0.nsamp, o0.nfreq
    ring = orc.make_ring(data, ringlen, wrpos)
    buf = np.zeros(2 * n * 2, np.int8)
    L.orc_getbuff(C.byref(ring), wrpos - 11 * n, 2 * n, 2, buf.ctypes.data)

    def run(i):
        o = orc.make_chan(chans[i].prn, dtype=2, f_if=0.0)
        xc = orc.codespectrum(o)
        P = np.zeros(nf * n)
        freq = np.ctypeslib.as_array(o.freq)[:nf].copy()
        t = time.time()
        L.orc_pcorrelator(buf.ctypes.data, 2, o.ti, n, freq.ctypes.data, nf, o.crate, o.nfft, xc.ctypes.data,
                          P.ctypes.data)
        return time.time() - t

    nsv = ncores            # one pcorrelator() call (71 bins, 1 iteration) per core
    t0 = time.time()
    with ThreadPoolExecutor(ncores) as ex:
        list(ex.map(run, range(nsv)))
    dt = time.time() - t0
    return dict(value=nsv * nf / dt, unit="correlations/s", cores=ncores, cpu=cpu_model(), kind="port",
                sample=f"{nsv} SV x 1 iteration x {nf} bins, oracle pcorrelator (mixed-radix DFT length 32736 "
                       f"standing in for FFTW3f, which is not installed), {dt:.1f} s wall")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=1000, help="code periods per channel per launch")
    ap.add_argument("--inner", type=int, default=32, help="launches per step (so that 20 steps time >= 0.5 s)")
    ap.add_argument("--loop-periods", type=int, default=2000, help="periods of the closed-loop legs (2 s of signal: a synchronised channel's first interval is partial)")
    ap.add_argument("--acq-steps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU baseline leg")
    ap.add_argument("--no-acq", action="store_true", help="skip the acquisition leg")
    ap.add_argument("--seed", type=int, default=20240601)
    ap.add_argument("--full", action="store_true",
                    help="also the legs beside the headline: per-kernel times and rooflines, integrity and oracle checks, "
                         "host-fed, closed-loop, acquisition and CPU baseline legs, GPU clocks")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    import gnsscorr_loader
    gc = gnsscorr_loader.load()
    import importlib
    synth = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.synth")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        log(f"warning: --gpus {args.gpus} but WORLD_SIZE {world}")
    dist = None
    ndev = max(torch.cuda.device_count(), 1)
    dev_index = local_rank % ndev               # one rank per GPU; wraps only in single-GPU rehearsals
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    backend = os.environ.get("BENCH_BACKEND", "nccl")    # "nccl" is RCCL on ROCm; "gloo" for rehearsals
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    E = args.epochs
    mg = importlib.import_module("erlangnetwork_gnsslib_sdr_amd.multigpu")
    # HBM ring = four chunks of E code periods (ShardedEngine: while a batch is correlated in two of them the
    # chunk after next lands in another, the fourth absorbs code-rate drift).  Rank 0 owns the IF stream (one
    # synthetic chunk, repeated).
    chunk = E * NSAMP                               # samples; 2*chunk bytes is a multiple of 16
    ringlen = 4 * chunk
    if rank == 0:
        data, sats = make_signal(gc, synth, E, args.seed)
        host = np.concatenate([data, data, data, data], axis=0)
    else:
        host, sats = None, None

    stream = torch.cuda.current_stream()
    # (BENCH_OWN_STREAM: the engine on a stream of its own -- ShardedEngine orders it against torch's with events)
    eng = gc.Engine(dev_index) if os.environ.get("BENCH_OWN_STREAM") else gc.Engine(dev_index, stream=stream.cuda_stream)
    ring_t = torch.zeros(ringlen * 2, dtype=torch.int8, device=dev)         # the HBM ring of this rank
    chans = channel_set(gc, rank)
    se = mg.ShardedEngine(eng, ring_t, chans, chunk, 2, dist=dist, rank=rank, world=world, strong=False)
    chunk_dev = None
    if rank == 0:
        chunk_dev = torch.from_numpy(data.reshape(-1)).to(dev)      # the stream's (repeating) chunk, resident in HBM
        ring_t.copy_(torch.from_numpy(host.reshape(-1)).to(dev))
    # two chunks in every ring before the first batch
    se.feed(chunk_dev, resident=True)
    se.feed(chunk_dev, resident=True)
    se.wait()
    torch.cuda.synchronize()

    rng = np.random.default_rng(args.seed + 17 * rank)
    acq_hist = 11 * NSAMP
    states0 = [dict(carrfreq=float(rng.uniform(-5000, 5000)), codefreq=c.crate + float(rng.uniform(-2, 2)),
                    remcode=float(rng.uniform(0.01, 0.99)), remcarr=float(rng.uniform(0, 6.2)),
                    buffloc=int(rng.integers(0, NSAMP))) for c in chans]
    eng.trk_set_state(states0)
    ntap = chans[0].ntap

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- tracking leg (primary) -------------------------------------------
    def step(i):
        # The channels walk through the ring (state stays on the device).  Per launch: the chunk after next
        # starts travelling from rank 0 into every rank's ring (one RCCL broadcast per epoch batch, ref SURVEY
        # 8e; on one GPU the repeating chunk is already in place and only the write position moves), then
        # the batch over the chunks already received is launched.
        for _ in range(args.inner):
            se.step(E, chunk_dev, resident=True)

    log("tracking leg: warm-up")
    for i in range(args.warmup):
        step(i)
    se.wait()
    barrier()
    # (--full) HIP events around the correlator launches only (roofline.launch_ms); the other kernels of the step
    # are timed in a short pass after the timed region
    eng.timing(0 if os.environ.get("BENCH_NOTIMING") or not args.full else 2)
    eng.timing_reset()
    log(f"tracking leg: {args.steps} steps x {args.inner} launches x {E} periods")
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    se.wait()
    barrier()
    dt = time.perf_counter() - t0
    eng.timing(False)
    if os.environ.get("GNSSCORR_TRACE_OUT"):          # debug library only (-DGC_TRK_TRACE, tools/trk_trace.sh)
        import ctypes
        tb = np.zeros(4096 * 12, dtype=np.uint64)
        gc.lib().gnsscorr_debug_trk_trace(ctypes.c_void_p(tb.ctypes.data))
        np.save(os.environ["GNSSCORR_TRACE_OUT"], tb.reshape(4096, 12))
    if os.environ.get("BENCH_PLAN_STATS"):            # (debug) which planner path served the periods
        import ctypes
        ps = np.zeros(8, dtype=np.uint64)
        gc.lib().gnsscorr_debug_plan_stats(ctypes.c_void_p(ps.ctypes.data), 1)
        log("planner paths [code claims, cert, walk | carrier claims, cert, walk | failed checks (verify mode), starts outside their bracket]:", ps.tolist())
        if hasattr(gc.lib(), "gnsscorr_debug_plan_prof"):          # (library built with -DGC_PLAN_PROF)
            pp = np.zeros(64 * 16, dtype=np.uint64)
            gc.lib().gnsscorr_debug_plan_prof(ctypes.c_void_p(pp.ctypes.data))
            pp = pp.reshape(64, 2, 8)[:NCH].astype(np.float64)
            nl = args.inner * (args.steps + args.warmup) + 1
            for name, w in (("code", 0), ("carrier", 1)):
                tot = pp[:, w, 0] / nl
                log("planner %s chain, clocks per launch: min %.0f median %.0f max %.0f (channel %d)" % (name, tot.min(), np.median(tot), tot.max(), int(tot.argmax())))
                for chx in sorted({int(tot.argmin()), int(np.argsort(tot)[len(tot) // 2]), int(tot.argmax())}):
                    v = pp[chx, w] / nl
                    log("  channel %d (carrfreq %.1f): loop %.0f  slow path %.0f (%.1f periods)  waiting for rows %.0f  waiting for n %.0f" % (
                        chx, states0[chx]["carrfreq"], v[0], v[1], v[4], v[2], v[3]))
    if args.dump_outputs and rank == 0:
        names = dump_outputs(args.dump_outputs, eng)
        log(f"outputs of the last timed step: {', '.join(names)} in {args.dump_outputs}")
    dt_max = dt
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt_max = float(t.item())

    units = NCH * E * args.inner * args.steps * world     # channel-epochs, whole job
    value = units * ntap / dt_max
    x_rt = (E * args.inner * args.steps / dt_max) / 1000.0    # epochs/s of the SV set / 1000 (per rank set)
    out = {
        "metric": METRIC, "value": value, "unit": "correlations/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt_max / args.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "int8 samples x int8 carrier LUT -> int32 accumulators (exact); NCOs: the reference's fp64 running sums, bit for bit",
        "data": "synthetic", "x_realtime": x_rt,
        "config": {"workload": "BASELINE configs[2]: 32-SV GPS L1CA tracking, 5-tap E/P/L correlators "
                               "(CORRN=2, CORRD=3), 1 ms coherent, 16.368 Msps int8 IQ, per GPU",
                   "channels_per_gpu": NCH, "epochs_per_launch": E, "launches_per_step": args.inner,
                   "epochs_per_step": E * args.inner, "taps": ntap, "loop": "open (frequencies held per launch); see closed_loop (--full)",
                   "if_broadcast": "RCCL broadcast of each step's IF chunk" if world > 1 else "none (1 GPU)"},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        eng.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    k_ms, k_n = eng.timing_read("trk_corr")
    # per-kernel times of the whole step: two more steps, every kernel bracketed by events (not part of `value`)
    eng.timing_reset()
    eng.timing(1)
    for i in range(2):
        step(i)
    se.wait()
    barrier()
    eng.timing(False)
    p_ms, p_n = eng.timing_read("trk_plan")
    s_ms, s_n = eng.timing_read("trk_finish")
    # ---- what the timed launches computed (outside the timed region): the fetch raises if any planned period lay
    # outside what the ring held or an NCO table overflowed; then one more launch, channel 0 of which is held to the
    # CPU oracle period by period (II/QQ and samples per period, bit for bit)
    integrity = None
    if world == 1:
        eng.trk_fetch()
        integrity = {"ring_and_nco_tables": "no violation over the timed launches (gnsscorr_trk_fetch)"}
    if world == 1 and not args.no_cpu:              # (the oracle as checker: part of the CPU leg)
        s0 = eng.trk_get_state()[0]
        se.step(E, chunk_dev, resident=True)
        se.wait()
        II, QQ, ns_ = eng.trk_fetch()
        import oracle as orc_chk
        o = orc_chk.make_chan(chans[0].prn, dtype=2, f_if=0.0, corrn=(ntap - 1) // 2, corrd=3, corrp=3)
        o.carrfreq, o.codefreq, o.remcode, o.remcarr = s0["carrfreq"], s0["codefreq"], s0["remcode"], s0["remcarr"]
        oring = orc_chk.make_ring(host, ringlen, 1 << 62)
        b, bad = s0["buffloc"], 0
        ncheck = min(E, 200)
        for e in range(ncheck):
            orc_chk.lib().orc_sdrtracking(C.byref(o), C.byref(oring), b)
            if not (np.array_equal(II[0, e], np.ctypeslib.as_array(o.II)[:ntap]) and
                    np.array_equal(QQ[0, e], np.ctypeslib.as_array(o.QQ)[:ntap]) and ns_[0, e] == o.currnsamp):
                bad += 1
            b += o.currnsamp
        assert bad == 0, f"bench: {bad} of {ncheck} periods of channel 0 differ from the oracle"
        integrity["oracle_check"] = f"channel 0, {ncheck} periods of the launch after the timed region: II/QQ/currnsamp bit for bit"
    bytes_unit = 32840                                    # algorithmic bytes per channel-epoch (int8 IQ, 5 taps)
    k_avg_ms = k_ms / max(k_n, 1)
    ach = NCH * E * bytes_unit / (k_avg_ms * 1e-3) / 1e9 if k_n else 0.0
    t_bytes, t_src = pmc_traffic("trk_corr")
    roof = dict(kernel="trk_corr", bound="hbm", achieved=ach, peak=HBM_PEAK_GBS, unit="GB/s",
                frac=ach / HBM_PEAK_GBS, traffic=t_bytes, traffic_source=t_src, launch_ms=k_avg_ms, launches=k_n,
                algorithmic_bytes_per_launch=NCH * E * bytes_unit)
    out.update({
        "gpu_clocks": gpu_clocks() if rank == 0 else None,
        "roofline": roof,
        "integrity": integrity,
        "kernels_ms_per_launch": {"trk_spec": (lambda a: a[0] / max(a[1], 1))(eng.timing_read("trk_spec")),
                                  "trk_plan": p_ms / max(p_n, 1),
                                  "trk_expand": (lambda a: a[0] / max(a[1], 1))(eng.timing_read("trk_expand")),
                                  "trk_edges": (lambda a: a[0] / max(a[1], 1))(eng.timing_read("trk_edges")),
                                  "trk_corr": k_ms / max(k_n, 1), "trk_finish": s_ms / max(s_n, 1)},
    })

    # the same accounting over everything that produces the E/P/L sums of a launch on the main stream (the roofline
    # line above is the dominant kernel alone; trk_edges and trk_expand prepare its look-ups and tables)
    km = out["kernels_ms_per_launch"]
    for name, ks in (("with_trk_edges", ("trk_edges", "trk_corr")), ("main_stream", ("trk_expand", "trk_edges", "trk_corr", "trk_finish"))):
        ms = sum(km[k] for k in ks)
        if ms > 0:
            roof[name] = {"kernels": list(ks), "launch_ms": ms, "frac": NCH * E * bytes_unit / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}

    # ---- host-fed leg through the sharded driver (any N): rank 0 owns the IF stream in pinned HOST memory; every
    # batch's chunk is copied into rank 0's ring slot and broadcast from there into every rank's ring (RCCL), two chunks
    # ahead of the batch that reads it.  The PCIe- and xGMI-inclusive rate of the multi-GPU data path; never `value`.
    # (at N > 1 only on request, BENCH_HOSTFED_SHARDED=1: it could not be rehearsed on RCCL with the one GPU at hand,
    # and a leg that has never run must not stand between a scaling run and its JSON line)
    if not os.environ.get("BENCH_NO_HOSTFED") and (world == 1 or os.environ.get("BENCH_HOSTFED_SHARDED")):
        log("host-fed leg through the sharded driver")
        chunk_host = torch.from_numpy(np.ascontiguousarray(data.reshape(-1))).pin_memory() if rank == 0 else None
        nl = 12
        for _ in range(3):                  # warm-up (the first feeds overwrite the resident chunks with the same samples)
            se.step(E, chunk_host, resident=False)
        se.wait()
        barrier()
        t0 = time.perf_counter()
        for _ in range(nl):
            se.step(E, chunk_host, resident=False)
        se.wait()
        barrier()
        sdt = time.perf_counter() - t0
        if dist is not None:
            tt_ = torch.tensor([sdt], dtype=torch.float64, device=dev)
            dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
            sdt = float(tt_.item())
        eng.trk_fetch()                     # (raises on a ring violation: every batch found its chunk in the ring)
        out["host_fed_sharded"] = {"x_realtime": nl * E / sdt / 1000.0, "correlations_per_s": world * NCH * E * nl * ntap / sdt,
                                   "host_to_ring_GBps": nl * chunk * 2 / sdt / 1e9, "n_gpus": world,
                                   "note": "ShardedEngine.step(..., resident=False): rank 0 copies every launch's IF chunk "
                                           "(32.7 MB) from pinned host memory into its ring slot, broadcasts it into every rank's "
                                           "ring two chunks ahead, each rank tracks its own channels"}

    # ---- closed loop (pll/dll on the device), same channels ----------------
    if world == 1 and args.loop_periods > 0:
        NP = args.loop_periods
        cl = {"periods": NP, "channels": NCH, "note": "gnsscorr_trk_run_loop: a chain of launch pairs per filter interval "
              "(1 period before nav bit sync, 10 after) -- trk_step_tail closes the interval (sums, sdrnavigation's bit sync, "
              "cumsumcorr, pll/dll) and plans the next, trk_step_corr correlates it (one workgroup per round); no host round "
              "trip inside a run"}
        # (loop1: cnt = 0, so that checksync() -- which starts at cnt > 2000, ref src/sdrnav.c:30 -- cannot synchronise a
        # channel inside the leg; loop10: synchronised from the start)
        for name, flagsync, cnt0 in (("loop1_before_bit_sync", 0, 0), ("loop10_after_bit_sync", 1, 2001)):
            log(f"closed loop leg: {name}, {NP} periods")
            lstates = [eng.loop_state(i, 200.0 * round(states0[i]["carrfreq"] / 200.0), flagsync=flagsync,
                                      synci=(7 * i) % 20, cnt=cnt0) for i in range(NCH)]
            eng.trk_set_state([dict(s, buffloc=s["buffloc"] % NSAMP) for s in states0])
            eng.loop_set(lstates)
            eng.trk_run_loop(NP)            # warm-up
            eng.sync()
            eng.trk_set_state([dict(s, buffloc=s["buffloc"] % NSAMP) for s in states0])
            eng.loop_set(lstates)
            barrier()
            t0 = time.perf_counter()
            eng.trk_run_loop(NP)
            eng.sync()
            cdt = time.perf_counter() - t0
            lg, ndone = eng.trk_fetch_log()
            assert int(ndone.min()) == NP, ndone
            nupd = int((lg["flagloopfilter"] != 0).sum())
            # kernel times of the same leg (events around every launch: not part of the figure above)
            eng.trk_set_state([dict(s, buffloc=s["buffloc"] % NSAMP) for s in states0])
            eng.loop_set(lstates)
            eng.timing_reset()
            eng.timing(1)
            eng.trk_run_loop(min(NP, 100))
            eng.sync()
            eng.timing(False)
            tt, tn = eng.timing_read("trk_step_tail")
            tc, tcn = eng.timing_read("trk_step_corr")
            cl[name] = {"x_realtime": NP / cdt / 1000.0, "us_per_period": cdt / NP * 1e6,
                        "correlations_per_s": NCH * NP * ntap / cdt, "filter_updates": nupd,
                        "kernels_us_per_launch": {"trk_step_tail": tt / max(tn, 1) * 1e3, "trk_step_corr": tc / max(tcn, 1) * 1e3,
                                                  "launch_pairs": tcn}}
        out["closed_loop"] = cl

    # ---- host-fed leg: the IF stream comes from host memory (gnsscorr_ring_push: pinned double buffer and
    # copy stream; the PCIe-inclusive rate, never `value`) ------------------
    if world == 1 and rank == 0 and not os.environ.get("BENCH_NO_HOSTFED"):
        log("host-fed leg")
        eng2 = gc.Engine(dev_index)
        eng2.ring_create(1, 2, ringlen)
        eng2.set_channels(chans)
        hostbytes = np.ascontiguousarray(data.reshape(-1))
        eng2.ring_push_raw(1, hostbytes, chunk)
        eng2.ring_push_raw(1, hostbytes, chunk)
        eng2.trk_set_state(states0)
        nl = 12
        for _ in range(2):                  # warm-up
            eng2.ring_push_raw(1, hostbytes, chunk)
            eng2.trk_run(E)
        eng2.sync()
        t0 = time.perf_counter()
        for _ in range(nl):
            eng2.ring_push_raw(1, hostbytes, chunk)
            eng2.trk_run(E)
        eng2.sync()
        hdt = time.perf_counter() - t0
        out["host_fed"] = {"x_realtime": nl * E / hdt / 1000.0, "correlations_per_s": NCH * E * nl * ntap / hdt,
                           "host_to_ring_GBps": nl * chunk * 2 / hdt / 1e9,
                           "note": "every launch's IF chunk (32.7 MB) pushed from pageable host memory through the pinned "
                                   "double buffer and the copy stream, overlapped with the previous launch's kernels"}
        eng2.close()

    # ---- acquisition leg (configs[1]) --------------------------------------
    if not args.no_acq:
        log("acquisition leg")
        wrpos = acq_hist + NSAMP // 3 + 100 * NSAMP if E > 120 else acq_hist + NSAMP // 3
        for _ in range(2):
            eng.acq_run(wrpos)
        barrier()
        eng.timing(True)
        eng.timing_reset()
        t0 = time.perf_counter()
        for _ in range(args.acq_steps):
            eng.acq_run(wrpos)
        barrier()
        adt = time.perf_counter() - t0
        eng.timing(False)
        if dist is not None:
            t = torch.tensor([adt], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            adt = float(t.item())
        res = eng.acq_fetch()
        nf, intg = chans[0].nfreq, chans[0].intg
        useful = sum(r["iters"] for r in res) * nf
        computed = NCH * nf * intg
        c_ms, c_n = eng.timing_read("acq_corr")
        f_ms, f_n = eng.timing_read("acq_fwd")
        L = 32768
        abytes = 8 * L + 8 * L + 16 * NSAMP           # SURVEY 8d per correlation
        c_avg = c_ms / max(c_n, 1)
        # (the kernel stops a channel soon after the iteration that acquires it, as the reference does at it:
        # the rate is quoted on the reference's own iteration count, the lower bound of what was computed)
        a_ach = useful * abytes / (c_avg * 1e-3) / 1e9 if c_n else 0.0
        acquired = sorted(c.prn for c, r in zip(chans, res) if r["flagacq"])
        if rank == 0 and sats is not None:
            # the stream holds ~10 PRNs at 38-50 dB-Hz.  The reference's search (10 x 1 ms
            # non-coherent, peak ratio > 3) finds every one at >= 41 dB-Hz and none that is absent; the ones
            # below may or may not cross its threshold (tests/test_gpu_configs.py holds the decisions of the
            # whole 32-SV set to the oracle's, this is the bench's own sanity check)
            present = sorted(s_["prn"] for s_ in sats)
            strong = sorted(s_["prn"] for s_ in sats if s_["cn0"] >= 41.0)
            assert set(acquired) <= set(present), f"false acquisition: found {acquired}, stream holds {present}"
            assert set(strong) <= set(acquired), f"missed a strong satellite: found {acquired}, >= 41 dB-Hz: {strong}"
        out["acquisition"] = {
            "workload": "BASELINE configs[1]: 32-SV GPS L1CA cold acquisition, 71 Doppler bins x 10 x 1 ms, "
                        "16.368 Msps int8 IQ, per GPU",
            "value": useful * args.acq_steps * world / adt, "unit": "correlations/s (1 ms FFT correlations the reference's search performs: "
                                                                     "iterations up to the acquiring one)",
            "full_grid_correlations_per_s": computed * args.acq_steps * world / adt,
            "ms_per_32sv_search": adt / args.acq_steps * 1e3,
            "acquired": acquired, "present": sorted(s_["prn"] for s_ in sats) if sats is not None else None,
            "kernels_ms_per_search": {"acq_fwd": f_ms / max(f_n, 1), "acq_corr": c_avg},
            "roofline": dict(kernel="acq_corr", bound="hbm", achieved=a_ach, peak=HBM_PEAK_GBS, unit="GB/s",
                             frac=a_ach / HBM_PEAK_GBS, traffic=pmc_traffic("acq_corr")[0], launch_ms=c_avg, launches=c_n,
                             algorithmic_bytes_per_launch=useful * abytes),
        }

    # ---- CPU baseline (rank 0, N = 1 only) ---------------------------------
    if rank == 0 and world == 1 and not args.no_cpu:
        log("CPU baseline leg")
        import oracle as orc
        flat = host
        out["cpu_baseline"] = cpu_baseline_tracking(orc, flat, ringlen, chans, states0)
        if not args.no_acq:
            out["acquisition"]["cpu_baseline"] = cpu_baseline_acq(orc, flat, ringlen, acq_hist + NSAMP // 3, chans)

    if rank == 0:
        print(json.dumps(out), flush=True)
    eng.close()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
