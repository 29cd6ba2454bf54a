#!/usr/bin/env python3
"""bench.py -- IQ->bits throughput of the MI355X-native path (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A "step" is one full pass of the hot path over one synthetic capture that is already resident in HBM:
IQ (complex64) -> demodulated signal (Signal.qad, materialised, stays in HBM) -> pulse table -> bits / pauses /
(bit_sample_pos: see config.outputs) -> the compact outputs in pinned host memory (SURVEY.md §8(d)'s timing window).  At N=1 the steps
run through urhgpu_stream_* (urh_amd.pipeline.CaptureStream): the hot kernel of step i + 1 overlaps the tail of step i -- STAGED passes
since round 6: the tail's kernels store the pulse-table rows into a staging blob in HBM, the runtime's copy ships them to the pinned host
blob while the bits are expanded, the last kernel stores the small head (header, pauses, offsets, packed bits) into the host blob itself
(kernel stores into pinned memory beside the next hot kernel cost it 10 us per pass) --, and `value` counts K steps
INCLUDING the delivery of all K (the timed region ends when the last step's results are on the host);
the device-only figure of the same steps is config.device_only_ms_per_step (--full).  Workload at N=1: BASELINE.json configs[1]
("1 GiB synthetic complex64 2-FSK @ 100 samples/symbol, single MI355X") on the bytes SURVEY.md §8(d) config 2
specifies (128 segments of 2^20 samples: numpy-seeded bits through modulate_c + numpy-seeded AWGN, see
urh_amd/synth.py:spec_fsk_capture); for N>1 every rank holds a 1 GiB sample-contiguous shard of one N-GiB capture
(segments 128*rank ..., weak scaling, configs[3] at N=8).

`python bench.py --gpus N` with N > 1 starts its own ranks (it re-executes itself under torch.distributed.run,
one process per GPU over RCCL) unless it already runs inside such a launch (WORLD_SIZE set).

A plain run sets up, warms up, times the K steps and prints the line: metric / value / unit / ms_per_step, the workload in `config`
and the headline's own fraction of HBM peak in `roofline`.  --dump-outputs DIR writes the last timed step's outputs (pulse table,
bits, pauses, offsets, bit_sample_pos, a seeded sample of qad) as DIR/<name>.npy; the capture is seeded, so two builds can be compared
output for output.  Everything else is measured and checked with --full only, which adds to the line:
  roofline      the dominant kernel (k_demod_runs_bp: demodulation + run segmentation) against HBM peak;
                achieved = algorithmic bytes (12 B/sample) / mean kernel time measured with HIP events
                attached to the kernel's dispatch on its launch stream, in K pipelined device-only steps right behind the timed
                region (the timed loop itself carries no events); traffic = HBM bytes per launch from two rocprofv3 --pmc children
                of this run (FETCH_SIZE, WRITE_SIZE in a pass of their own each, gfx950 corrections)
  config        also: one capture start to finish in the stream's latency setting, the H2D-inclusive time of a capture that starts on
                the host (urhgpu_stream_push_upload) against the bare pinned copy, the step with bit_sample_pos shipped, and -- N > 1 --
                the sharded result's self-check and the FIR-halo variant (sharded_parity, fir_halo)
  parity        the LAST timed step's outputs (qad as uint32, pulse table, bits, pauses, offsets, bit_sample_pos) of the full
                2^27-sample capture compared element for element with the CPU reference on the same bytes
  cpu_baseline  the reference's own path on this box's host cores (oracle/_ref = the reference's Cython modules compiled
                from /root/reference, plus its pure-Python tail when the staged sources are present), else the C port
  extra         the other single-GPU BASELINE configurations at full size with their own parity records (--no-extra skips them):
                configs[2] OOK + 64-tap FIR + auto noise + estimate, configs[4] 4-PSK Costas + auto center
"""
import argparse
import json
import os
import socket
import sys
import time

_FLAG_DEV = None          # where the ranks' scalar reductions live: the GPU under nccl, the host under a gloo group (main())

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEG = 1 << 20
HBM_PEAK_GBS = 8000.0            # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
ALGO_BYTES_PER_SAMPLE = 12       # 8 B complex64 read + 4 B float32 qad write


def pmc_traffic(kernel_substr):
    """HBM bytes per launch of the dominant kernel from the newest committed PMC summary under profiles/
    (rocprofv3 FETCH_SIZE / WRITE_SIZE passes, corrected as tools/prof_collect.py documents); the counters
    cannot be collected inside this process, so this is the figure of the profiled run of the SAME command -- the record names the
    file (profiles/rNN...: the round it was collected in) so that a stale figure is recognisable as such."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_fsk_1gib_pmc.json")))
    for f in reversed(files):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        for name, rec in d.items():
            if kernel_substr in name and "hbm_traffic_bytes_per_launch" in rec:
                return int(rec["hbm_traffic_bytes_per_launch"]["total"]), "profiles/" + os.path.basename(f) + " (a separate rocprofv3 --pmc run of this command)"
    return None, None


def pmc_traffic_live(segments, kernel_substr, passes=3):
    """HBM bytes per launch of the dominant kernel from PMC passes launched BY THIS RUN: two short rocprofv3 children of this file
    (--pmc-child: the same capture, `passes` un-pipelined IQ->bits passes), FETCH_SIZE and WRITE_SIZE in a pass of their own each with
    --kernel-trace only, corrected as /opt/skills/guides/MI355X_MICROARCH.md prescribes for gfx950 (both in KiB; FETCH_SIZE reports half
    the bytes of wide coalesced streaming reads).  None when rocprofv3 is not there or a child fails (the caller then quotes the
    committed profile and says so)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    mean = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="urh_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--kernel-trace", "--pmc", ctr, "--kernel-include-regex", "k_demod_runs_bp", "--output-format", "csv", "-d", d, "-o", "b", "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", "--segments", str(segments), "--steps", str(passes)]
            subprocess.run(cmd, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"}, timeout=90, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
            vals = []
            for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r.get("Counter_Name") == ctr and kernel_substr in r.get("Kernel_Name", ""):
                        vals.append(float(r["Counter_Value"]))
            if not vals:
                return None, f"the {ctr} pass returned no rows for the kernel"
            mean[ctr] = sum(vals) / len(vals)
        except Exception as exc:                               # noqa: BLE001
            return None, repr(exc)[:160]
        finally:
            shutil.rmtree(d, ignore_errors=True)
    total = mean["FETCH_SIZE"] * 1024 * 2 + mean["WRITE_SIZE"] * 1024
    return int(total), (f"rocprofv3 --kernel-trace --pmc passes launched by this run (FETCH_SIZE {mean['FETCH_SIZE']:.0f} KiB x 2 [gfx950 wide-read correction] + "
                        f"WRITE_SIZE {mean['WRITE_SIZE']:.0f} KiB, mean over {passes} un-pipelined passes of the same capture)")


def pmc_child(args):
    """what the PMC passes profile: the same capture, a few un-pipelined IQ->bits passes (qad materialised), nothing else"""
    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.synth import spec_fsk_capture
    dev = torch.device("cuda", 0)
    iq, _ = spec_fsk_capture(args.segments, dev)
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, 5, 100, 0.1, 8, True)
    pipe = DevicePipeline(0, pipelined=False)
    pipe.reserve(iq.shape[0], p)
    for _ in range(max(1, args.steps)):
        pipe.iq_to_bits(iq, p, want_qad=True)
    torch.cuda.synchronize()


def copy_ceiling(torch, pipe, iq, n):
    """What a pure copy gets out of the HBM on THIS box, measured now (urhgpu_bench_copy_ceiling_dev): the hot kernel's access shape
    without its arithmetic (8 B in + 4 B out per sample) and the guide's plain float4 copy."""
    import ctypes as C
    from urh_amd import _lib
    out = torch.empty(n, dtype=torch.float32, device=iq.device)
    rec = {}
    lib, h = _lib.load(), pipe.ctx.handle
    pipe.ctx.set_stream(torch.cuda.current_stream(iq.device).cuda_stream)
    for shape, name, bytes_per in ((0, "hot_kernel_shape", 12), (1, "plain_float4", 8), (2, "hot_kernel_shape_on_the_hot_kernels_cus", 12)):
        ms = C.c_float(0.0)
        best = None
        for _ in range(3):                           # each call: 3 warm-up + 40 timed launches
            st = lib.urhgpu_bench_copy_ceiling_dev(h, C.c_void_p(iq.data_ptr()), C.c_void_p(out.data_ptr()), n, shape, 40, C.byref(ms))
            if st == _lib.ERR_UNSUPPORTED:           # no CU-masked hot stream on this context
                break
            _lib.check(st)
            best = ms.value if best is None else min(best, ms.value)
        if best is None:
            continue
        rec[name + "_ms"] = round(best, 4)
        rec[name + "_gbs"] = round(n * bytes_per / (best * 1e-3) / 1e9, 1)
    del out
    return rec


def tuning_from_env():
    """Developer A/B knobs (tools/ab.sh): the environment is read HERE, the library itself reads none (urhgpu_ctx_set_tuning).
    URH_TUNE_<KEY>=value for every key of urhgpu_ctx_set_tuning (include/urhgpu.h), e.g. URH_TUNE_STREAM_POLICY=0.
    Returns (tuning dict for DevicePipeline, torch priority of the tail's stream)."""
    t = {}
    e = os.environ
    for key in ("hot_lds_kb", "hot_lds_kb_sharded", "hot_cus_removed_per_xcd", "profile_bracket", "stream_policy", "stream_latency",
                "stream_segments", "stream_pos_direct", "upload_pieces"):
        env = "URH_TUNE_" + key.upper()
        if env in e:
            t[key] = int(e[env])
    prio = int(e.get("URH_TAIL_STREAM_PRIORITY", "0"))
    return t, prio


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _set_omp_threads(n):
    """omp_set_num_threads on the OpenMP runtime the reference's prange uses (libgomp, already loaded with the module)."""
    import ctypes
    try:
        ctypes.CDLL("libgomp.so.1").omp_set_num_threads(int(n))
        return True
    except OSError:
        return False


def cpu_reference(iq_host, p, want_outputs=True):
    """The CPU side on the whole capture: (qad, ppseq, flat bits) for the parity check and the cpu_baseline record.

    With oracle/_ref (the reference's own Cython modules, compiled from /root/reference): afp_demod (OpenMP prange over all host
    cores) + grab_pulse_lens, timed per stage with OMP_NUM_THREADS unset and = 1; with the staged Python sources also the
    reference's end-to-end ProtocolAnalyzer.get_protocol_from_signal() (incl. its pure-Python _ppseq_to_bits), median of 3 after
    a warm-up on one segment.  Without oracle/_ref: the C restatement (kind "port", 1 thread)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import build_ref
    import ref_python
    import urh_oracle as oracle
    n = len(iq_host)
    order = 2 ** p.bits_per_symbol
    mod, sps, tol = p.modulation_type, p.samples_per_symbol, p.tolerance
    rec = {"unit": "Msamples/s", "cpu_model": cpu_model(), "host_cores": os.cpu_count() or 1}
    if not build_ref.built():
        t0 = time.perf_counter()
        qad = oracle.afp_demod(iq_host, p.noise_threshold, mod, order)
        t1 = time.perf_counter()
        pp = oracle.grab_pulse_lens(qad, p.center, tol, mod, sps, p.bits_per_symbol, p.center_spacing)
        t2 = time.perf_counter()
        flat = oracle.ppseq_to_bits_flat(pp, sps, p.bits_per_symbol, True, p.pause_threshold)
        t3 = time.perf_counter()
        rec.update({"value": round(n / (t3 - t0) / 1e6, 2), "cores": 1, "kind": "port",
                    "sample": f"all {n} samples of the same capture through the C restatement (oracle/urh_oracle.c): afp_demod {t1 - t0:.2f}s, "
                              f"grab_pulse_lens {t2 - t1:.2f}s, _ppseq_to_bits {t3 - t2:.2f}s"})
        return rec, (qad, pp, flat)
    sf, _, _ = build_ref.import_ref()
    cores = os.cpu_count() or 1
    afp = lambda a: np.asarray(sf.afp_demod(a, p.noise_threshold, mod, order, p.costas_loop_bandwidth))          # noqa: E731
    grab = lambda q: np.asarray(sf.grab_pulse_lens(q, p.center, tol, mod, sps, p.bits_per_symbol, p.center_spacing))   # noqa: E731
    grab(afp(iq_host[:SEG]))                        # warm-up
    t0 = time.perf_counter()
    qad = afp(iq_host)
    t1 = time.perf_counter()
    pp = grab(qad)
    t2 = time.perf_counter()
    flat = oracle.ppseq_to_bits_flat(pp, sps, p.bits_per_symbol, True, p.pause_threshold)       # for the parity check
    t3 = time.perf_counter()
    stages = {"afp_demod_s": round(t1 - t0, 3), "grab_pulse_lens_s": round(t2 - t1, 3), "ppseq_to_bits_c_port_s": round(t3 - t2, 3)}
    # the same two Cython stages on ONE thread (afp_demod is the only threaded stage)
    if _set_omp_threads(1):
        ta = time.perf_counter()
        q1 = afp(iq_host)
        tb = time.perf_counter()
        stages["afp_demod_1thread_s"] = round(tb - ta, 3)
        del q1
        _set_omp_threads(cores)
    value_s = t3 - t0
    kind_note = "Cython stages of the real reference + C port of its pure-Python tail"
    if ref_python.available():
        try:
            ref_python.setup()
            from urh.signalprocessing.IQArray import IQArray
            from urh.signalprocessing.ProtocolAnalyzer import ProtocolAnalyzer
            from urh.signalprocessing.Signal import Signal

            def e2e(arr):
                s = Signal("")
                s.iq_array = IQArray(arr)
                s.modulation_type = mod
                s.bits_per_symbol = p.bits_per_symbol
                s.noise_threshold = p.noise_threshold
                s.center, s.center_spacing, s.tolerance = p.center, p.center_spacing, tol
                s.samples_per_symbol, s.pause_threshold = sps, p.pause_threshold
                pa = ProtocolAnalyzer(s)
                ts = time.perf_counter()
                pa.get_protocol_from_signal()              # qad (afp_demod) -> grab_pulse_lens -> _ppseq_to_bits (pure Python) -> Messages
                return time.perf_counter() - ts, pa

            e2e(iq_host[:SEG])
            runs = sorted(e2e(iq_host)[0] for _ in range(3))
            stages["get_protocol_from_signal_s_runs"] = [round(x, 3) for x in runs]
            value_s = runs[1]
            _set_omp_threads(1)
            t1t, pa = e2e(iq_host)
            _set_omp_threads(cores)
            stages["get_protocol_from_signal_1thread_s"] = round(t1t, 3)
            rec["value_1thread"] = round(n / t1t / 1e6, 2)
            if want_outputs:           # the reference's own Python tail agrees with the C port used for the parity check
                ref_bits = "".join(m.plain_bits_str for m in pa.messages)
                stages["python_tail_equals_c_port"] = bool(ref_bits == "".join(map(str, flat[0].tolist()))) if len(flat[0]) < 50_000_000 else None
            kind_note = "the reference's own ProtocolAnalyzer.get_protocol_from_signal() end to end (Cython afp_demod + grab_pulse_lens, pure-Python _ppseq_to_bits), median of 3"
        except Exception as e:           # noqa: BLE001  (the baseline must not take the benchmark down)
            stages["python_path_error"] = repr(e)[:200]
    rec.update({"value": round(n / value_s / 1e6, 2), "cores": cores, "kind": "reference",
                "sample": f"all {n} samples of the same capture; {kind_note}; OMP_NUM_THREADS unset ({cores} threads) and = 1 (value_1thread)",
                "stages": stages})
    return rec, (qad, pp, flat)


def parity_record(res, ref_out, tx_bits, kind, got_qad=None):
    """Element-for-element comparison of the last timed step's outputs with the CPU reference's on the same bytes.  res: the step's
    HostBits (what arrived in pinned host memory through the compact blob) or a device-resident BitsResult; got_qad: the step's
    demodulated signal (host copy)."""
    import numpy as np
    qad, pp, flat = ref_out
    if got_qad is None and getattr(res, "qad", None) is not None:
        got_qad = res.qad.cpu().numpy()
    rows = res.ppseq()
    got = res.flat()
    names = ("bits", "msg_off", "pauses", "bit_sample_pos", "pos_off")
    rec = {"against": "oracle/_ref (the reference's Cython afp_demod + grab_pulse_lens; tail: C port pinned on the reference's Python)"
           if kind == "reference" else "oracle/ C restatement", "samples": int(len(qad)),
           "outputs_compared": "the LAST timed step's: host copies that arrived through the compact blob (pulse table, bits, pauses, offsets, "
                               "bit_sample_pos) + its qad read back from HBM"}
    if got_qad is not None:
        rec["qad_mismatches"] = int((got_qad.view(np.uint32) != qad.view(np.uint32)).sum())
    rec["rows"] = int(len(pp))
    rec["rows_equal"] = bool(np.array_equal(rows, pp))
    for k, name in enumerate(names):
        rec[name + "_equal"] = bool(np.array_equal(got[k], flat[k]))
    rec["n_bits"] = int(len(flat[0]))
    rec["n_messages"] = int(len(flat[2]))
    # sanity against the transmitter (not the parity criterion): bit k of a message starts at sample pos[k]
    bits, off, pauses, pos, poff = got
    errors = total = 0
    for m in range(len(pauses)):
        bp = pos[poff[m]:poff[m] + (off[m + 1] - off[m])]
        seg_of, sym_of = bp // SEG, (bp % SEG + 50) // 100
        ok = (sym_of < tx_bits.shape[1]) & (seg_of < tx_bits.shape[0])
        errors += int((bits[off[m]:off[m + 1]][ok] != tx_bits[seg_of[ok], sym_of[ok]]).sum())
        total += int(ok.sum())
    rec["bit_errors_vs_transmitted"] = errors
    rec["bits_compared_vs_transmitted"] = total
    rec["bit_exact"] = bool(rec.get("qad_mismatches", 0) == 0 and rec["rows_equal"] and all(rec[nm + "_equal"] for nm in names))
    return rec


def variant_steps(torch, pipe, iq, p, n, args, ramp, headline_copy):
    """What SURVEY 8(d) asks for beside the headline, in the driver's line: the fused bits-only mode against 8 B per
    sample, and the integer sample types real captures have (signal_functions.pyx:343-354) against THEIR bytes -- complex int16 4 + 4,
    complex int8 2 + 4 B per sample --, each K pipelined steps through the capture stream like the headline, each checked: bits-only
    against the headline's last outputs (themselves compared with the reference in `parity`), the integer captures against the
    reference (oracle/_ref, else the C restatement) run on the same integer bytes, qad included."""
    import numpy as np
    from dataclasses import replace
    import ctypes as C
    from urh_amd import _lib as _ulib
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import urh_oracle as oracle
    rec = {}
    p_np = replace(p, write_bit_sample_pos=False)

    def run(st, x, k):
        out = []
        for _ in range(k):
            r = st.push(x)
            if r is not None:
                out.append(r)
        return out + st.flush()

    def timed(st, x):
        ramp(lambda: run(st, x, 10))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run(st, x, args.steps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3, res[-1].check()

    def frac(ms, bytes_per_sample):
        return round(n * bytes_per_sample / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
    # ---- bits-only: qad is not materialised (8 B per sample) ----
    st = pipe.stream(n, p_np, want_qad=False, want_pos=False)
    ms, last = timed(st, iq)
    same = bool(np.array_equal(last.ppseq(), headline_copy["ppseq"]) and all(np.array_equal(a, b) for a, b in zip(last.flat()[:3], headline_copy["flat"][:3])))
    rec["bits_only"] = {"ms_per_step": round(ms, 4), "bytes_per_sample": 8, "frac_of_8TBs": frac(ms, 8), "Msamples_per_s": round(n / ms / 1e3, 1),
                        "equals_headline_outputs": same}
    st.close()
    # ---- integer captures: the same signal quantised (amplitude 1 -> 8192 / 64 LSB), demodulated from their own 4 / 2 bytes per sample ----
    ref = _ref_modules()
    for name, tdt, ndt, scale, bps in (("int16", torch.int16, np.int16, 8192.0, 8), ("int8", torch.int8, np.int8, 64.0, 6), ("int8_wide", torch.int8, np.int8, 64.0, 6)):
        src = iq
        if name == "int8_wide":
            # the same generator at a deviation of +-100 kHz (0.63 rad per sample: every batch leaves the hot kernel's fast loop): the stream probes
            # its captures and takes the integer instantiation with the wide loop (k_wide_probe; urh_amd/csrc/stream.hip)
            from urh_amd.synth import spec_fsk_capture as _gen
            src, _ = _gen(n >> 20, iq.device, first_segment=0, sps=p.samples_per_symbol, deviation_hz=100e3)
        x = (src * scale).round().clamp(-32767 if ndt is np.int16 else -127, 32767 if ndt is np.int16 else 127).to(tdt).contiguous()
        del src
        st = pipe.stream(n, p_np, want_qad=True, want_pos=False, dtype=ndt)
        ms, last = timed(st, x)
        r = {"ms_per_step": round(ms, 4), "bytes_per_sample": bps, "frac_of_8TBs": frac(ms, bps), "Msamples_per_s": round(n / ms / 1e3, 1),
             "capture": (f"the headline capture x {scale:g}, rounded to {name}" if name != "int8_wide" else
                         "the configs[1] generator at a deviation of +-100 kHz (0.63 rad per sample) x 64, rounded to int8")}
        if not args.no_cpu_baseline:
            host = x.cpu().numpy()
            if ref is not None:
                sf = ref[0]
                q = np.asarray(sf.afp_demod(host, p.noise_threshold, "FSK", 2, p.costas_loop_bandwidth))
                pp = np.asarray(sf.grab_pulse_lens(q, p.center, p.tolerance, "FSK", p.samples_per_symbol, 1, p.center_spacing))
                r["against"] = "oracle/_ref (the reference's Cython afp_demod + grab_pulse_lens on the integer bytes)"
            else:
                q = oracle.afp_demod(host, p.noise_threshold, "FSK", 2)
                pp = oracle.grab_pulse_lens(q, p.center, p.tolerance, "FSK", p.samples_per_symbol, 1, p.center_spacing)
                r["against"] = "oracle/ C restatement"
            flat = oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, 1, True, p.pause_threshold)
            got_q = np.empty(n, np.float32)
            _ulib.check(_ulib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(last.d_qad_ptr), got_q.ctypes.data_as(C.c_void_p), n * 4))
            r["qad_mismatches"] = int((got_q.view(np.uint32) != q.view(np.uint32)).sum())
            r["rows"] = int(len(pp))
            r["bit_exact"] = bool(r["qad_mismatches"] == 0 and np.array_equal(last.ppseq(), pp) and
                                  all(np.array_equal(a, b) for a, b in zip(last.flat()[:3], flat[:3])) and
                                  np.array_equal(last.bit_sample_pos(), flat[3]) and np.array_equal(last.pos_offsets(), flat[4]))
            del host, q, pp, flat, got_q
        rec[name] = r
        st.close()
        del x
    # ---- row density: every timing above is at 100 samples per symbol -- 671 k pulse-table rows per GiB.  The tail's work
    # is proportional to the rows; the reference's own test uses 8 samples per symbol (tests/test_demodulations.py:55-72).  Two more captures
    # of the same generator, K pipelined steps each, checked against the reference on their bytes:
    #   sps10   10 samples per symbol, tolerance 1: ~ 13 M rows, 13 M bits per GiB
    #   bursty  SURVEY 8(d) variant 2b: 10 465 symbols + a 2 076-sample gap per segment, noise_threshold 0.2: 128 messages
    from urh_amd.synth import spec_fsk_capture
    dev = iq.device
    for name, gen, pv, what in (
            ("sps10", dict(sps=10), replace(p_np, samples_per_symbol=10, tolerance=1),
             "the configs[1] generator at 10 samples per symbol (modulate_c segments + AWGN 0.05), tolerance 1"),
            ("bursty", dict(sps=100, n_symbols=10465), replace(p_np, noise_threshold=0.2),
             "SURVEY 8(d) variant 2b: 10 465 symbols + a 2 076-sample gap per 2^20-sample segment, noise_threshold 0.2")):
        try:
            x, _ = spec_fsk_capture(n >> 20, dev, first_segment=0, **gen)
            st = pipe.stream(n, pv, want_qad=True, want_pos=False)
            ms, last = timed(st, x)
            r = {"ms_per_step": round(ms, 4), "bytes_per_sample": 12, "frac_of_8TBs": frac(ms, 12), "Msamples_per_s": round(n / ms / 1e3, 1),
                 "capture": what, "rows": int(len(last.ppseq())), "messages": int(len(last.flat()[2])), "d2h_bytes": int(last.blob_bytes),
                 "d2h_gbs": round(int(last.blob_bytes) / (ms * 1e-3) / 1e9, 1),
                 "row_format": ("one uint16 per row: state and length (URHGPU_BLOB_ROW16, dense pulse tables: 2 B per row)" if getattr(last, "_row16", None) is not None
                                else "int8 state + uint16 length per row (URHGPU_BLOB_LEN16: 3 B)" if getattr(last, "_len16", None) is not None
                                else "int8 state + int32 length per row (5 B)"),
                 "bound": ("what a step ships per pulse-table row over PCIe: d2h_gbs is the link's rate" if int(last.blob_bytes) / (ms * 1e-3) > 30e9
                           else "the hot kernel's run phase and the tail over this many rows (DESIGN 7.1), not the link" if len(last.ppseq()) > n // 64
                           else "as the headline: the hot kernel (HBM) with the tail of the pass before beside it"),
                 "stream_stats": st.stats()}
            if not args.no_cpu_baseline:
                host = x.cpu().numpy()
                if ref is not None:
                    sf = ref[0]
                    q = np.asarray(sf.afp_demod(host, pv.noise_threshold, "FSK", 2, pv.costas_loop_bandwidth))
                    pp = np.asarray(sf.grab_pulse_lens(q, pv.center, pv.tolerance, "FSK", pv.samples_per_symbol, 1, pv.center_spacing))
                    r["against"] = "oracle/_ref (the reference's Cython afp_demod + grab_pulse_lens)"
                else:
                    q = oracle.afp_demod(host, pv.noise_threshold, "FSK", 2)
                    pp = oracle.grab_pulse_lens(q, pv.center, pv.tolerance, "FSK", pv.samples_per_symbol, 1, pv.center_spacing)
                    r["against"] = "oracle/ C restatement"
                flat = oracle.ppseq_to_bits_flat(pp, pv.samples_per_symbol, 1, True, pv.pause_threshold)
                got_q = np.empty(n, np.float32)
                _ulib.check(_ulib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(last.d_qad_ptr), got_q.ctypes.data_as(C.c_void_p), n * 4))
                r["qad_mismatches"] = int((got_q.view(np.uint32) != q.view(np.uint32)).sum())
                r["bit_exact"] = bool(r["qad_mismatches"] == 0 and np.array_equal(last.ppseq(), pp) and
                                      all(np.array_equal(a, b) for a, b in zip(last.flat()[:3], flat[:3])) and
                                      np.array_equal(last.bit_sample_pos(), flat[3]) and np.array_equal(last.pos_offsets(), flat[4]))
                del host, q, pp, flat, got_q
            rec[name] = r
            st.close()
            del x
        except Exception as exc:          # noqa: BLE001  (a variant must not take the headline with it)
            rec[name] = {"error": repr(exc)[:300]}
        torch.cuda.empty_cache()
    return rec


def _timed(torch, fn, reps=5, ramp_ms=30.0):
    """(result, MEDIAN wall time in ms over `reps`) of fn() with the GPU drained before and after.  The part needs about 30 ms of
    sustained load to reach its clocks (tools/ramp_probe.py) and falls back within half a second of idling -- the
    host-side parity checks between the stages are much longer than that --, so fn() is first repeated for ramp_ms, as the headline
    loop does."""
    times, out = [], None
    t_ramp = time.perf_counter()
    while ramp_ms > 0 and (time.perf_counter() - t_ramp) * 1e3 < ramp_ms:
        out = fn()
        torch.cuda.synchronize()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return out, times[len(times) // 2]


def _ref_modules():
    """(signal_functions, util, auto_interpretation Cython modules, AutoInterpretation python module or None) of the real reference"""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import build_ref
    import ref_python
    if not build_ref.built():
        return None
    sf, util, ai = build_ref.import_ref()
    AI = IQArray = None
    if ref_python.available():
        try:
            ref_python.setup()
            from urh.ainterpretation import AutoInterpretation as AI
            from urh.signalprocessing.IQArray import IQArray
        except Exception:           # noqa: BLE001
            AI = IQArray = None
    return sf, util, ai, AI, IQArray


def extra_config3(pipe, dev, args):
    """BASELINE.json configs[2] at full size: 1 GiB OOK capture -> 64-tap complex FIR (Signal.filter_range
    semantics) -> get_magnitudes + detect_noise_level -> AutoInterpretation.estimate(noise, "OOK") -> afp_demod("ASK") -> pulse
    table -> bits, every stage compared with the real reference on the same bytes."""
    import ctypes as C
    import numpy as np
    import torch
    from urh_amd import _lib, estimators
    from urh_amd.pipeline import DemodParams
    from urh_amd.synth import spec_fir_taps, spec_ook_capture
    iq, chips = spec_ook_capture(args.segments, dev)
    n = iq.shape[0]
    taps = spec_fir_taps()
    d_taps = torch.from_numpy(taps.view(np.float32).copy()).to(dev)
    lib, h = _lib.load(), pipe.ctx.handle
    filt_u = torch.empty_like(iq)

    def fir():                                  # the filter alone (its own roofline figure)
        pipe.ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(lib.urhgpu_fir_filter_dev(h, C.c_void_p(iq.data_ptr()), n, C.c_void_p(d_taps.data_ptr()), len(taps), None,
                                             C.c_void_p(filt_u.data_ptr())))
    _, t_fir = _timed(torch, fir)
    noise_u, t_noise = _timed(torch, lambda: estimators.detect_noise_level_dev(pipe, filt_u))
    # what the pipeline runs: filter with the magnitude chunk statistics fused into its epilogue
    (filt, noise), t_fir_noise = _timed(torch, lambda: estimators.fir_filter_detect_noise_dev(pipe, iq, d_taps))
    fused_equal = bool(torch.equal(filt, filt_u) and float(noise) == float(noise_u))
    del filt_u
    keep = {}
    est, t_est = _timed(torch, lambda: estimators.estimate_dev(pipe, filt, noise=noise, modulation="OOK", keep=keep))
    est_stages = {}
    estimators.estimate_dev(pipe, filt, noise=noise, modulation="OOK", timings=est_stages)
    center = float(est["center"]) if est else 0.0
    p = DemodParams("ASK", 1, float(noise), center, 1.0, 5, 100, 0.1, 8, True)
    # estimate has demodulated the capture with the parameters the Signal now has (afp_demod(iq, noise, "ASK", 2)): that IS Signal.qad
    # (Signal.py:421-431 caches it; urh_amd.signal.Signal.auto_detect keeps it) -- the bits are sliced from it, 4 B per sample
    qad_kept = keep["qad"]
    res, t_bits = _timed(torch, lambda: pipe.qad_to_bits(qad_kept, p))
    res_fused, t_bits_fused = _timed(torch, lambda: pipe.iq_to_bits_checked(filt, p, want_qad=True))     # for comparison: demodulating again
    # SURVEY 8(d)'s window ends with the compact outputs ON THE HOST: the slicing pass + pack kernel + one pinned copy of the blob
    pool = {}
    hb, t_bits_host = _timed(torch, lambda: pipe.qad_to_bits(qad_kept, p).host(pool=pool).check())
    host_counts = (hb.n_rows, hb.n_msg, hb.n_bits)
    total_ms = t_fir_noise + t_est + t_bits
    total_host_ms = t_fir_noise + t_est + t_bits_host
    rec = {"workload": "configs[2]: 1 GiB OOK (Manchester, 124 messages) + 64-tap complex FIR + auto noise threshold + estimate + bits",
           "samples": n, "ms": round(total_ms, 3), "ms_incl_d2h": round(total_host_ms, 3),
           "ms_meaning": "ms: the stages with the outputs left in HBM; ms_incl_d2h: SURVEY 8(d)'s window -- the last stage ends with pulse table, bits, pauses, "
                         "offsets and bit_sample_pos in pinned host memory (compact blob: pack kernel + one copy)",
           "timing": "every stage: median of 5 wall times (GPU drained before and after) following 30 ms of repeats of the same stage (clock ramp)",
           "stages_ms": {"fir_filter_with_fused_noise_statistics": round(t_fir_noise, 3), "estimate": round(t_est, 3),
                         "bits_from_the_qad_estimate_left": round(t_bits, 3), "bits_from_the_qad_estimate_left_plus_d2h": round(t_bits_host, 3),
                         "d2h_bytes": hb.blob_bytes, "host_counts_equal_device": bool(tuple(res.host_counts()[:3]) == host_counts)},
           "for_comparison_ms": {"iq_to_bits_ask_demodulating_again": round(t_bits_fused, 3),
                                 "same_outputs": bool(res_fused.host_counts()[:4] == res.host_counts()[:4])},
           "unfused_ms": {"fir_filter": round(t_fir, 3), "detect_noise_level": round(t_noise, 3), "fused_result_equal": fused_equal},
           "estimate_stages_ms": est_stages,
           "estimated": {k: (float(v) if not isinstance(v, str) else v) for k, v in (est or {}).items()},
           "roofline": {"algorithmic_bytes_per_sample": 28,
                        "hbm_frac": round(28 * n / (total_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "fir_valu_frac": round(512.0 * n / (t_fir_noise * 1e-3) / 78.6e12, 4),
                        "fir_valu_frac_unfused_filter_alone": round(512.0 * n / (t_fir * 1e-3) / 78.6e12, 4),
                        "note": "28 B/sample = FIR 8 + 8, demodulation 8 + 4 (SURVEY 8(d) config 3); the FIR is bound by un-fused fp32 VALU "
                                "(512 flop per sample against 78.6 TFLOP/s of non-FMA packed fp32), not by HBM.  fir_valu_frac follows the "
                                "stage that is TIMED in `ms` (the filter with the noise statistics fused into its epilogue); the filter "
                                "kernel alone is the second figure"},
           "messages": res.host_counts()[1], "bits": res.host_counts()[2]}
    mods = None if args.no_cpu_baseline else _ref_modules()
    if mods:
        sf, util, ai, AI, IQArray = mods
        host = iq.cpu().numpy()
        x = host.view(np.complex64).reshape(-1)
        t0 = time.perf_counter()
        ref_f = np.asarray(sf.fir_filter(x, taps))
        t1 = time.perf_counter()
        ref_f2 = np.ascontiguousarray(ref_f).view(np.float32).reshape(-1, 2)
        got_f = filt.cpu().numpy()
        par = {"fir_mismatches": int((got_f.view(np.uint32) != ref_f2.view(np.uint32)).sum())}
        del got_f
        mags = np.asarray(util.get_magnitudes(ref_f2))
        cpu = {"fir_filter_s": round(t1 - t0, 2)}
        if AI is not None:
            t2 = time.perf_counter()
            ref_noise = AI.detect_noise_level(mags)
            t3 = time.perf_counter()
            ref_est = AI.estimate(IQArray(ref_f2), noise=ref_noise, modulation="OOK")
            t4 = time.perf_counter()
            cpu.update({"detect_noise_level_s": round(t3 - t2, 2), "estimate_s": round(t4 - t3, 2)})
            par["noise_equal"] = bool(float(ref_noise) == float(noise))
            par["estimate_equal"] = bool(ref_est is not None and est is not None and all(
                (ref_est[k] == est[k]) if isinstance(ref_est[k], str) else (float(ref_est[k]) == float(est[k])) for k in ref_est))
            par["reference_estimate"] = {k: (float(v) if not isinstance(v, str) else v) for k, v in (ref_est or {}).items()}
        del mags
        t5 = time.perf_counter()
        ref_qad = np.asarray(sf.afp_demod(ref_f2, p.noise_threshold, "ASK", 2))
        ref_pp = np.asarray(sf.grab_pulse_lens(ref_qad, p.center, 5, "ASK", 100, 1, 1.0))
        t6 = time.perf_counter()
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import urh_oracle as oracle
        ref_flat = oracle.ppseq_to_bits_flat(ref_pp, 100, 1, True, 8)
        cpu["afp_demod_plus_grab_pulse_lens_s"] = round(t6 - t5, 2)
        par["qad_mismatches"] = int((res.qad.cpu().numpy().view(np.uint32) != ref_qad.view(np.uint32)).sum())
        par["rows_equal"] = bool(np.array_equal(res.ppseq(), ref_pp))
        par["bits_pauses_positions_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(res.flat(), ref_flat)))
        # against the transmitter (sanity, not the parity criterion): message m carries the chips of segment 4 + m from its first
        # "1" chip on (leading and trailing "0" chips of an OOK message are indistinguishable from the pause around it)
        bits, off = res.flat()[0], res.flat()[1]
        ok_msgs = 0
        if len(off) - 1 <= chips.shape[0] - 4:
            for m in range(len(off) - 1):
                c = chips[4 + m]
                lead = int(np.argmax(c))
                got = bits[off[m]:off[m + 1]]
                L = min(len(got), len(c) - lead)
                ok_msgs += int(L >= 9900 and np.array_equal(got[:L], c[lead:lead + L]))
        par["messages_equal_transmitted_chips"] = int(ok_msgs)
        par["bit_exact"] = bool(par["fir_mismatches"] == 0 and par["qad_mismatches"] == 0 and par["rows_equal"] and
                                par["bits_pauses_positions_equal"] and par.get("noise_equal", True) and par.get("estimate_equal", True))
        rec["parity"] = par
        cpu_total = sum(v for v in cpu.values())
        rec["cpu_baseline"] = {"kind": "reference", "stages": cpu, "value": round(n / cpu_total / 1e6, 2), "unit": "Msamples/s",
                               "cores": os.cpu_count() or 1,
                               "sample": f"all {n} samples: the reference's Cython fir_filter / afp_demod / grab_pulse_lens and its Python "
                                         "detect_noise_level / estimate"}
    rec["value"] = round(n / (total_ms * 1e-3) / 1e6, 1)
    rec["unit"] = "Msamples/s"
    return rec


def extra_config5(pipe, dev, args):
    """BASELINE.json configs[4] at full size: 1 GiB 4-PSK, Costas loop (order 4) + auto center detection.
    Run (i) as named: center = detect_center(qad); run (ii) center = 0, center_spacing = 1.5 as the reference's own 4-PSK test."""
    import numpy as np
    import torch
    from urh_amd import estimators
    from urh_amd.signal import Signal
    from urh_amd.synth import spec_psk_capture
    iq, tx = spec_psk_capture(args.segments, dev)
    n = iq.shape[0]
    sig = Signal(iq, modulation="PSK", pipe=pipe)
    del iq
    sig.bits_per_symbol = 2
    sig.noise_threshold = 0.2
    sig.center_spacing = 1.5
    sig.costas_loop_bandwidth = 0.1

    def costas():
        sig._drop_cache()
        return sig.qad
    qad, t_costas = _timed(torch, costas)
    stats = pipe.ctx.costas_stats()
    center, t_center = _timed(torch, lambda: estimators.detect_center_dev(pipe, qad))
    out = {}
    for tag, c in (("i_auto_center", center), ("ii_center_0", 0.0)):
        sig.center = float(c) if c is not None else 0.0

        def slice_bits():                          # outputs left in HBM, as in the headline step
            return sig._digitize_dev(sig.qad, sig.params())
        _, t_dev = _timed(torch, slice_bits)

        def slice_bits_host():                     # ... and with the pulse table / bits / positions copied to the host
            sig._bits = None
            return sig._digitize()
        dig, t_dig = _timed(torch, slice_bits_host)
        out[tag] = (dig, t_dev, sig.center, t_dig)
    total_i = t_costas + t_center + out["i_auto_center"][1]
    total_ii = t_costas + out["ii_center_0"][1]
    rec = {"workload": "configs[4]: 1 GiB 4-PSK, Costas loop (order 4, bandwidth 0.1) + detect_center + bits",
           "samples": n, "ms": round(total_i, 3), "ms_center_0": round(total_ii, 3),
           "ms_incl_d2h": round(t_costas + t_center + out["i_auto_center"][3], 3), "ms_center_0_incl_d2h": round(t_costas + out["ii_center_0"][3], 3),
           "ms_meaning": "ms: the stages with the outputs left in HBM; ms_incl_d2h: SURVEY 8(d)'s window -- the slicing stage ends with pulse table, bits, pauses, "
                         "offsets and bit_sample_pos in pinned host memory (urh_amd.signal.Signal._digitize: compact blob, pack kernel + one copy)",
           "timing": "every stage: median of 5 wall times (GPU drained before and after) following 30 ms of repeats of the same stage (clock ramp)",
           "stages_ms": {"costas_demod": round(t_costas, 3), "detect_center": round(t_center, 3),
                         "grab_pulse_lens_plus_bits_auto_center": round(out["i_auto_center"][1], 3),
                         "grab_pulse_lens_plus_bits_center_0": round(out["ii_center_0"][1], 3),
                         "grab_pulse_lens_plus_bits_plus_d2h_auto_center": round(out["i_auto_center"][3], 3),
                         "grab_pulse_lens_plus_bits_plus_d2h_center_0": round(out["ii_center_0"][3], 3)},
           "center_detected": None if center is None else float(center),
           "detect_center_roofline": {"passes_today": "5 reads + 1 write of the demodulated signal (count, compaction read + write, two leaf passes, histogram)",
                                      "gbs_at_6_passes": round(6 * 4 * n / (t_center * 1e-3) / 1e9, 1),
                                      "gbs_at_the_3_reads_a_fused_compaction_would_need": round(3 * 4 * n / (t_center * 1e-3) / 1e9, 1),
                                      "hbm_frac_at_6_passes": round(6 * 4 * n / (t_center * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                      "note": "two strictly sequential float32 sums over 16 384 chunk sums (numpy's order) take 0.2 ms of it whatever the passes cost"},
           "costas_chunks": {"matched_by_a_candidate": stats[0], "met_at_a_checkpoint": stats[1], "evaluated_serially": stats[2],
                             "respeculation_rounds": stats[3],
                             "speculative_hit_rate": round(stats[0] / max(1, stats[0] + stats[1] + stats[2]), 5)},
           "roofline": {"algorithmic_bytes_per_sample": 24, "hbm_frac": round(24 * n / (total_i * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                        "note": "bound by the dependent arithmetic of the loop recurrence (SURVEY 8(d) config 5), not by a roofline"},
           "rows_auto_center": int(len(out["i_auto_center"][0][0])), "rows_center_0": int(len(out["ii_center_0"][0][0]))}
    mods = None if args.no_cpu_baseline else _ref_modules()
    if mods:
        sf, util, ai, AI, IQArray = mods
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import urh_oracle as oracle
        host = sig.iq.cpu().numpy()
        t0 = time.perf_counter()
        ref_qad = np.asarray(sf.afp_demod(host, 0.2, "PSK", 4, 0.1)).copy()
        t1 = time.perf_counter()
        got_qad = qad.cpu().numpy()
        par = {"qad_mismatches_from_index_1": int((got_qad[1:].view(np.uint32) != ref_qad[1:].view(np.uint32)).sum())}
        ref_qad[0] = got_qad[0]          # the reference leaves element 0 uninitialised (np.empty): give both slicers the same value
        cpu = {"costas_afp_demod_s": round(t1 - t0, 2)}
        ref_center = None
        if AI is not None:
            t2 = time.perf_counter()
            ref_center = AI.detect_center(ref_qad)
            cpu["detect_center_s"] = round(time.perf_counter() - t2, 2)
            par["center_equal"] = bool((ref_center is None and center is None) or (ref_center is not None and center is not None and
                                                                                   float(ref_center) == float(center)))
            par["reference_center"] = None if ref_center is None else float(ref_center)
        t3 = time.perf_counter()
        for tag in ("i_auto_center", "ii_center_0"):
            dig, _, c, _ = out[tag]
            ref_pp = np.asarray(sf.grab_pulse_lens(ref_qad, c, 5, "PSK", 100, 2, 1.5))
            ref_flat = oracle.ppseq_to_bits_flat(ref_pp, 100, 2, True, 8)
            par[tag + "_rows_equal"] = bool(np.array_equal(dig[0], ref_pp))
            par[tag + "_bits_pauses_positions_equal"] = bool(all(np.array_equal(a, b) for a, b in zip(dig[1:], ref_flat)))
        cpu["grab_pulse_lens_x2_s"] = round(time.perf_counter() - t3, 2)
        par["bit_exact"] = bool(par["qad_mismatches_from_index_1"] == 0 and par.get("center_equal", True) and
                                all(v for k, v in par.items() if k.endswith("_equal")))
        rec["parity"] = par
        rec["cpu_baseline"] = {"kind": "reference", "stages": cpu, "value": round(n / (cpu["costas_afp_demod_s"] + cpu.get("detect_center_s", 0) +
                                                                                     cpu["grab_pulse_lens_x2_s"] / 2) / 1e6, 2),
                               "unit": "Msamples/s", "cores": os.cpu_count() or 1,
                               "sample": f"all {n} samples: the reference's Cython costa_demod (serial) / grab_pulse_lens and Python detect_center"}
    rec["value"] = round(n / (total_i * 1e-3) / 1e6, 1)
    rec["unit"] = "Msamples/s"
    return rec


def run_extras(pipe, dev, args):
    out = []
    for fn in (extra_config3, extra_config5):
        try:
            import torch
            torch.cuda.empty_cache()
            out.append(fn(pipe, dev, args))
        except Exception as e:           # noqa: BLE001  (an extra must not take the headline line down)
            import traceback
            out.append({"workload": fn.__name__, "error": repr(e)[:300], "trace": traceback.format_exc()[-600:]})
    return out


def sharded_self_check(torch, dist, pipe, iq, p, rank, world, local_rank, fir_taps, halo_given, left_halo, with_oracle, steps=0, left_raw=None):
    """N > 1: the sharded result proves itself in the same run (every rank calls this; rank 0 returns the record).  One more pass with
    bit_sample_pos on; rank 0 gathers every rank's piece (pulse-table rows that end in the shard, their bits, pauses, offsets, positions)
    and every rank's SHARD, and compares
      (ii) the stitched pieces with ONE single-GPU pass over the whole world x n capture on rank 0 (the path the -m gpu suite and the
           N = 1 line check against the reference at 2^27) -- rows, bits, message offsets, pauses, positions, element for element --
           and rank 0's demodulated shard with the first n samples of that pass's;
      (i)  (with_oracle) rank 0's shard with the real reference (oracle/_ref: Cython afp_demod + grab_pulse_lens on the shard's 2^27
           samples, C port of the Python tail): the demodulated signal (uint32 view), every row but the reference's last one (cut
           short by the shard's end), and the bits those rows expand to.
    fir_taps: the FIR-halo variant (BASELINE.json configs[3]: signal_functions.pyx:513-525 in front, 63-sample halo exchange); the
    single-GPU side then filters the whole capture in one launch.  steps > 0: also time that many passes (per rank, max over ranks)."""
    import numpy as np
    from dataclasses import replace
    from urh_amd.shard_engine import GpuShardEngine
    from urh_amd.sharding import stitch
    n = int(iq.shape[0])
    dev = iq.device
    p_pos = replace(p, write_bit_sample_pos=True)
    hg = halo_given and fir_taps is None
    was_host = pipe.engine.host_results
    pipe.engine.host_results = False

    raw_given = fir_taps is not None and (rank == 0 or left_raw is not None)     # the FIR-halo variant with the raw halo handed over: no exchange for it

    def one():
        if fir_taps is not None and raw_given:
            x, fh = pipe.fir_filter(iq, fir_taps, left_raw=left_raw, want_halo=True)
            return pipe.iq_to_bits(x, p_pos, want_qad=True, halo_given=True, left_halo=fh)
        x = pipe.fir_filter(iq, fir_taps) if fir_taps is not None else iq
        return pipe.iq_to_bits(x, p_pos, want_qad=True, halo_given=hg, left_halo=left_halo if hg else None)
    rec = {}
    if steps > 0:
        for _ in range(max(10, steps)):                       # clocks
            one()
        pipe.ctx.join(); torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        pipe.ctx.join(); torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=_FLAG_DEV)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rec["ms_per_step"] = round(float(t.item()) / steps * 1e3, 4)
        rec["steps"] = steps
    res = one()
    pipe.ctx.join()
    torch.cuda.synchronize()
    pc = res.piece()
    pieces = [None] * world if rank == 0 else None
    dist.gather_object(pc, pieces, dst=0)
    whole = torch.empty((world * n, 2), dtype=iq.dtype, device=dev) if rank == 0 else None
    if _FLAG_DEV.type == "cpu":                              # (a gloo group: through the host)
        parts = [torch.empty((n, 2), dtype=iq.dtype) for _ in range(world)] if rank == 0 else None
        dist.gather(iq.cpu(), parts, dst=0)
        if rank == 0:
            for r in range(world):
                whole[r * n:(r + 1) * n].copy_(parts[r])
    else:
        dist.gather(iq, [whole[r * n:(r + 1) * n] for r in range(world)] if rank == 0 else None, dst=0)
    torch.cuda.synchronize()
    pipe.engine.host_results = was_host
    if rank != 0:
        return None
    names = ("rows", "bits", "msg_off", "pauses", "bit_sample_pos", "pos_off")
    got = stitch(pieces)
    single = GpuShardEngine(local_rank)
    xs = single.fir(whole, fir_taps, None) if fir_taps is not None else whole
    r1 = single.iq_to_bits_checked(xs, p_pos, want_qad=True)
    want = (r1.ppseq(),) + tuple(r1.flat())
    rec.update({"against": f"one single-GPU pass over the whole {world} x {n}-sample capture on rank 0" +
                           (" (64-tap FIR over the whole capture in one launch first)" if fir_taps is not None else ""),
                "rows": int(len(want[0])), "n_bits": int(len(want[1])), "n_messages": int(len(want[3]))})
    for nm, a, b in zip(names, got, want):
        rec[nm + "_equal"] = bool(np.array_equal(a, b))
    rec["qad_rank0_shard_mismatches"] = int((res.qad.view(torch.int32) != r1.qad[:n].view(torch.int32)).sum().item())
    ok = all(rec[nm + "_equal"] for nm in names) and rec["qad_rank0_shard_mismatches"] == 0
    if fir_taps is not None:
        m_t = int(fir_taps.shape[0])
        rec["halo_bytes_per_rank"] = (m_t + 1) * 8 if raw_given else (m_t - 1) * 8
        rec["halo"] = ("the m + 1 raw samples before the shard come WITH the shard (their last m - 1 are the filter's history, filtering them gives the two "
                       "filtered samples the demodulation needs): no exchange") if raw_given else "exchanged: one all-gather for the filter, one for the demodulation"
        rec["all_gathers_per_pass"] = 2 if raw_given else 4
        if rec.get("ms_per_step"):
            t_s = rec["ms_per_step"] * 1e-3
            rec["roofline"] = {"bytes_per_sample": 28, "what": "8 read + 8 written (the filtered IQ is materialised: it replaces the capture, Signal.filter_range) + 8 read + 4 written (qad)",
                               "hbm_frac_of_8TBs": round(n * 28 / t_s / 8e12, 4),
                               "valu_flop_per_sample": 8 * m_t, "valu_frac_of_78.6_TFLOPs_non_fma": round(n * 8 * m_t / t_s / 78.6e12, 4),
                               "bound": "fp32 VALU (the reference's strict accumulation order: no FMA, no MFMA)"}
    if with_oracle and fir_taps is None:
        try:
            sys.path.insert(0, os.path.join(ROOT, "oracle"))
            import build_ref
            import urh_oracle as oracle
            host = iq.cpu().numpy()
            order = 2 ** p.bits_per_symbol
            if build_ref.built():
                sf = build_ref.import_ref()[0]
                qad = np.asarray(sf.afp_demod(host, p.noise_threshold, p.modulation_type, order, p.costas_loop_bandwidth))
                pp = np.asarray(sf.grab_pulse_lens(qad, p.center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing))
                kind = "oracle/_ref (the reference's Cython afp_demod + grab_pulse_lens) on rank 0's shard"
            else:
                qad = oracle.afp_demod(host, p.noise_threshold, p.modulation_type, order)
                pp = oracle.grab_pulse_lens(qad, p.center, p.tolerance, p.modulation_type, p.samples_per_symbol, p.bits_per_symbol, p.center_spacing)
                kind = "oracle/ C restatement on rank 0's shard"
            flat = oracle.ppseq_to_bits_flat(pp, p.samples_per_symbol, p.bits_per_symbol, True, p.pause_threshold)
            k = max(len(pp) - 1, 0)                           # the reference's last row is cut short by the shard's end
            m = max(0, len(flat[0]) - (int(pp[-1][1]) // p.samples_per_symbol + 2) * p.bits_per_symbol) if len(pp) else 0
            orc = {"against": kind, "samples": n,
                   "qad_mismatches": int((res.qad.cpu().numpy().view(np.uint32) != qad.view(np.uint32)).sum()),
                   "rows_compared": k, "rows_prefix_equal": bool(np.array_equal(got[0][:k], pp[:k])),
                   "bits_compared": m, "bits_prefix_equal": bool(np.array_equal(got[1][:m], flat[0][:m]))}
            orc["bit_exact"] = orc["qad_mismatches"] == 0 and orc["rows_prefix_equal"] and orc["bits_prefix_equal"]
            rec["oracle_shard0"] = orc
            ok = ok and orc["bit_exact"]
        except Exception as exc:                               # noqa: BLE001 (the check must not take the benchmark down: it says so instead)
            rec["oracle_shard0"] = {"error": repr(exc)[:200]}
            ok = False
    rec["bit_exact"] = bool(ok)
    del whole, xs, r1, single
    torch.cuda.empty_cache()
    return rec



DUMP_LIMIT_BYTES = 56 << 20      # --dump-outputs: all files together (under 64 MB with room for headers and block starts)
DUMP_BLOCK = 1 << 15             # a sampled array keeps whole blocks of this many rows (neighbours stay comparable)
DUMP_QAD_BLOCKS = 64             # qad (4 B per sample, 512 MiB per GiB of capture): 64 blocks = 2^21 samples, 8 MiB
DUMP_SEED = 20260
FLAT_NAMES = ("bits", "msg_off", "pauses", "bit_sample_pos", "pos_off")      # BitsResult.flat() / HostBits.flat()


def dump_block_starts(n, blocks, seed=DUMP_SEED):
    """Fixed, seeded choice of `blocks` whole blocks of DUMP_BLOCK rows out of n (sorted start rows); None: keep all n rows."""
    import numpy as np
    if n <= blocks * DUMP_BLOCK:
        return None
    return np.sort(np.random.default_rng(seed).choice(n // DUMP_BLOCK, blocks, replace=False)).astype(np.int64) * DUMP_BLOCK


def write_dump(dirname, arrays, prefix=""):
    """--dump-outputs: every array as <dirname>/<prefix><name>.npy, float32 where that holds its values exactly (float32, 8/16-bit
    integers), else float64.  Arrays too large for DUMP_LIMIT_BYTES in all are replaced by a seeded sample of whole blocks of rows
    (<name>_starts.npy: the first row of each block)."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        out[name] = a.astype(np.float32 if a.dtype == np.float32 or (a.dtype.kind in "iub" and a.dtype.itemsize <= 2) else np.float64)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT_BYTES:
        for name in sorted(out, key=lambda k: -out[k].nbytes):
            a = out[name]
            if total <= DUMP_LIMIT_BYTES:
                break
            room = DUMP_LIMIT_BYTES - (total - a.nbytes)
            starts = dump_block_starts(len(a), max(1, room // max(1, a[:1].nbytes * DUMP_BLOCK)))
            if starts is None:
                continue
            out[name] = np.concatenate([a[s:s + DUMP_BLOCK] for s in starts])
            out[name + "_starts"] = starts.astype(np.float64)
            total += out[name].nbytes + out[name + "_starts"].nbytes - a.nbytes
    os.makedirs(dirname, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(dirname, prefix + name + ".npy"), a)


def qad_sample(n, read):
    """The demodulated signal of a step, sampled: read(start, count) -> float32 numpy.  Returns (sample, block starts)."""
    import numpy as np
    starts = dump_block_starts(n, DUMP_QAD_BLOCKS)
    if starts is None:
        return read(0, n), np.zeros(1)
    return np.concatenate([read(int(s), DUMP_BLOCK) for s in starts]), starts.astype(np.float64)


def self_launch(args):
    """`python bench.py --gpus N` (N > 1) from a bare interpreter: become `python -m torch.distributed.run ... bench.py ...`."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    sys.stdout.flush()
    os.execve(sys.executable, cmd, env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--segments", type=int, default=128, help="2^20-sample segments per GPU (128 = 1 GiB complex64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU reference (then no parity record either)")
    ap.add_argument("--bits-only", action="store_true", help="do not materialise qad (8 B/sample variant)")
    ap.add_argument("--torch-capture", action="store_true", help="round-1 capture (torch RNG, clean fp64 phase ramp) instead of the §8(d) bytes")
    ap.add_argument("--no-reference-loop", action="store_true", help="skip the un-pipelined reference steps after the timed region (profiling runs)")
    ap.add_argument("--no-d2h", action="store_true", help="skip the D2H-inclusive measurements (profiling runs: their passes overlap copies)")
    ap.add_argument("--no-device-loop", action="store_true", help="profiling runs: only the capture-stream loop (no run without positions, no device-only loop)")
    ap.add_argument("--no-variants", action="store_true", help="skip the bits-only / int16 / int8 steps (profiling runs)")
    ap.add_argument("--no-extra", action="store_true", help="skip configs[2] and configs[4] at full size (they add about a minute)")
    ap.add_argument("--no-sharded-check", action="store_true", help="N > 1: skip the self-check (stitched pieces against a single-GPU pass over the whole "
                                                                     "capture and the reference on rank 0's shard) and the FIR-halo variant")
    ap.add_argument("--no-upload", action="store_true", help="skip the H2D-inclusive measurement (1 GiB of pinned host memory)")
    ap.add_argument("--fir-halo", action="store_true", help="N > 1: prepend the 64-tap FIR with halo exchange (configs[3] 'FIR-halo' variant)")
    ap.add_argument("--pipeline", action="store_true",
                    help="(default) software-pipeline consecutive steps: the hot kernel of step i+1 on the main stream while the tail of "
                         "step i runs on a second stream")
    ap.add_argument("--no-pipeline", action="store_true", help="run the passes one after the other (profiling: the dominant kernel alone)")
    ap.add_argument("--selftest-only", action="store_true",
                    help="N > 1 (or URH_BENCH_FORCE_SHARDED=1): ONE sharded pass and its self-check against a single-GPU pass over the whole "
                         "capture (+ the reference on rank 0's shard), then a short line -- under a minute, for a first lease that may be short")
    ap.add_argument("--no-pmc", action="store_true", help="do not launch the two rocprofv3 --pmc children for roofline.traffic (quote the committed profile)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: latencies, the upload, variants, the device-only and un-pipelined loops, roofline "
                         "(live PMC), the CPU baseline with the parity record, the other configurations, the sharded self-check")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32 / float64; qad as a seeded sample of blocks)")
    args = ap.parse_args()
    full = args.full
    if args.pmc_child:
        return pmc_child(args)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)

    # Exactly ONE line on stdout: libraries write there too (RCCL prints a five-line version banner through C stdio, which lands
    # behind the JSON line when the process exits), so file descriptor 1 is pointed at stderr for the rest of the run and the line
    # goes to the saved descriptor.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    from urh_amd.pipeline import DemodParams, DevicePipeline
    from urh_amd.synth import fsk_capture, spec_fsk_capture

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    # URH_BENCH_SHARE_GPU=1 + URH_BENCH_DIST_BACKEND=gloo (tools/two_ranks_one_gpu.sh): every rank on device 0 and the group over gloo --
    # RCCL refuses two ranks on one device -- so that a 1-GPU box executes the N > 1 line with real processes (rank > 0 branches,
    # exchanges, the self-check); its timings mean nothing
    if os.environ.get("URH_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    backend = os.environ.get("URH_BENCH_DIST_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    global _FLAG_DEV
    _FLAG_DEV = dev if backend == "nccl" else torch.device("cpu")
    dist = None
    # URH_BENCH_FORCE_SHARDED=1 (with torch.distributed.run --nproc-per-node 1) drives the sharded code path -- RCCL process
    # group, all-gathers, urhgpu_shard_* phases -- on a single GPU: a smoke test of the N > 1 plumbing on a 1-GPU box.
    force_sharded = os.environ.get("URH_BENCH_FORCE_SHARDED") == "1"
    sharded = world > 1 or force_sharded
    if sharded:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    sps, tol = 100, 5
    p = DemodParams("FSK", 1, 0.0, 0.0, 1.0, tol, sps, 0.1, 8, True)
    # rank r holds segments [r*segments, (r+1)*segments) of the world*segments-segment capture
    # Consecutive passes are software-pipelined (the hot kernel of pass i + 1 beside the latency-bound tail of pass i, three scratch
    # arenas in rotation) unless --no-pipeline: that is how a stream of captures is processed, on one GPU and on many.
    if not args.no_pipeline:
        args.pipeline = True
    if args.torch_capture:
        iq, tx_bits = fsk_capture(args.segments, dev, seed=1234, sps=sps, first_segment=rank * args.segments)
        tx_bits = tx_bits.cpu().numpy()
        capture = "torch RNG (round-1 generator)"
    else:
        iq, tx_bits = spec_fsk_capture(args.segments, dev, first_segment=rank * args.segments, sps=sps)
        capture = "SURVEY 8(d) config 2 bytes: modulate_c segments (default_rng(1234+k) bits) + default_rng(5678+k) AWGN 0.05"
    n = iq.shape[0]
    fir_taps = None
    tuning, tail_prio = tuning_from_env()
    if sharded:
        from urh_amd.shard_engine import GpuShardEngine
        from urh_amd.sharding import RcclComm, ShardedPipeline, TorchDistComm
        # the exchanges go straight through RCCL (a communicator of the library's own, a few us of host time each);
        # URH_BENCH_TORCH_COLLECTIVES=1: torch.distributed's all_gather_into_tensor instead (55-80 us of host time each)
        comm = TorchDistComm() if os.environ.get("URH_BENCH_TORCH_COLLECTIVES") == "1" else RcclComm.create()
        comm_fallback_reason = ("URH_BENCH_TORCH_COLLECTIVES=1" if os.environ.get("URH_BENCH_TORCH_COLLECTIVES") == "1" else RcclComm.last_fallback_reason)
        pipe = ShardedPipeline(GpuShardEngine(local_rank, pipelined=args.pipeline, tuning=tuning, tail_stream_priority=tail_prio), comm)
        pipe.engine.host_results = False                     # switched on for the headline loop below
        if args.fir_halo:
            from urh_amd.synth import spec_fir_taps
            fir_taps = torch.from_numpy(spec_fir_taps().view("float32").reshape(-1, 2).copy()).to(dev)     # (64, 2): 64 complex taps
    else:
        pipe = DevicePipeline(local_rank, pipelined=args.pipeline, tuning=tuning, tail_stream_priority=tail_prio)
    pipe.reserve(n, p)
    want_qad = not args.bits_only

    # Sharded runs: every rank but the first holds the two samples before its shard as well (the end of the previous rank's last segment,
    # 16 bytes a loader reads with the shard), so a pass needs two all-gathers -- summaries, flags -- and no halo exchange;
    # URH_BENCH_HALO_EXCHANGE=1 exchanges the halos instead (three all-gathers).  The FIR variant filters first: its halo is exchanged.
    halo_given = sharded and fir_taps is None and os.environ.get("URH_BENCH_HALO_EXCHANGE") != "1"
    left_halo = left_raw65 = None
    if sharded and rank > 0:
        prev, _ = (fsk_capture if args.torch_capture else spec_fsk_capture)(1, dev, **(dict(seed=1234, sps=sps, first_segment=rank * args.segments - 1)
                                                                                   if args.torch_capture else
                                                                                   dict(first_segment=rank * args.segments - 1, sps=sps)))
        if halo_given:
            left_halo = prev[-2:].clone()
        left_raw65 = prev[-65:].clone()                      # the FIR-halo variant: 64 taps + 1 raw samples before the shard, handed over with it
        del prev

    if args.selftest_only:
        if not sharded:
            raise SystemExit("--selftest-only checks the sharded path: --gpus N > 1, or URH_BENCH_FORCE_SHARDED=1 under torch.distributed.run")
        t_s = time.perf_counter()
        rec = sharded_self_check(torch, dist, pipe, iq, p, rank, world, local_rank, None, halo_given, left_halo, with_oracle=not args.no_cpu_baseline)
        if rank == 0:
            out = {"metric": "sharded self-test (no timing)", "value": None, "unit": None, "n_gpus": world, "steps": 1, "warmup": 0,
                   "config": {"workload": f"{world} GiB complex64 2-FSK sharded over {world} GPUs: one pass, stitched pieces against a single-GPU pass over the "
                                          "whole capture on rank 0" + ("" if args.no_cpu_baseline else " and rank 0's shard against the reference"),
                              "collectives": type(pipe.comm).__name__, "collectives_fallback_reason": comm_fallback_reason,
                              "sharded_parity": rec, "parity_bit_exact": (rec or {}).get("bit_exact"), "seconds": round(time.perf_counter() - t_s, 1)}}
            os.write(real_stdout, (json.dumps(out) + "\n").encode())
        pipe.ctx.join()
        torch.cuda.synchronize()
        if hasattr(pipe.comm, "close"):
            pipe.comm.close()
        dist.destroy_process_group()
        return

    def step():
        if sharded:
            x = pipe.fir_filter(iq, fir_taps) if fir_taps is not None else iq
            return pipe.iq_to_bits(x, p, want_qad=want_qad, halo_given=halo_given, left_halo=left_halo)
        return pipe.iq_to_bits(iq, p, want_qad=want_qad)

    for _ in range(args.warmup):
        res = step()
    pipe.ctx.join()
    torch.cuda.synchronize()
    # --full: latency of ONE step with nothing overlapped (device only), and the same plus the D2H copy of the WIDE outputs (int64 pulse
    # table, one byte per bit, int64 bit_sample_pos -- the round-2 format, kept for comparison; qad stays in HBM)
    lat, lat_d2h = [], []
    for _ in range(5 if full else 0):
        torch.cuda.synchronize()
        t_l = time.perf_counter()
        res = step()
        pipe.ctx.join()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t_l)
    d2h_bytes_wide = None
    use_stream = not sharded and args.pipeline and not args.no_d2h
    # A full collection of Python's cyclic garbage collector takes 30-40 ms in a process that has torch and numpy loaded (a hundred
    # steps' worth: a round-3 probe caught one inside a timed region): the timed regions run with the collector off.
    import gc
    gc.collect()
    gc.disable()
    if full and not sharded and not args.no_d2h:
        pinned = {}
        for _ in range(6):
            torch.cuda.synchronize()
            t_l = time.perf_counter()
            res = step()
            host_out = res.to_host_pinned(pinned)           # pulse table, bits, offsets, pauses, bit_sample_pos in pinned host memory
            lat_d2h.append(time.perf_counter() - t_l)
        lat_d2h = lat_d2h[1:]                               # the first call allocates the pinned buffers
        d2h_bytes_wide = int(sum(x.nbytes for x in host_out))
        del pinned, host_out
    latency_ms = min(lat) * 1e3 if lat else None

    # Anything slow between the clock ramp and a timed region lets the part's clocks fall again (round 3, profiles/HISTORY.md: 1 ms of idling
    # before K = 20 passes costs 3 %, 5 ms 13 %): the profile records' events (a hipEventCreate each) and the process group's first
    # barrier are paid for here, not there.
    pipe.ctx.profile_begin(args.steps)
    pipe.ctx.profile_end()
    if dist:
        dist.barrier()

    def ramp(run10):
        """The part takes some 30 ms of sustained load to reach its clocks (tools/ramp_probe.py: 0.34 -> 0.30 ms per pipelined pass over
        the first ~100 passes, and again after half a second of idling): untimed passes until the step time has settled.  (Sharded runs:
        a fixed count, every rank takes part in every pass's exchanges.)"""
        passes, best = 0, None
        if os.environ.get("URH_BENCH_NO_RAMP"):
            return 0
        for g in range(20):
            torch.cuda.synchronize()
            t_r = time.perf_counter()
            run10()
            torch.cuda.synchronize()
            cur = time.perf_counter() - t_r
            passes += 10
            if not sharded and g >= 11 and best is not None and cur > 0.99 * best:
                break
            if sharded and g >= 9:
                break
            best = cur if best is None else min(best, cur)
        return passes

    def device_steps(k):
        r = None
        for _ in range(k):
            r = step()
        pipe.ctx.join()                      # the stream waits for the last step's tail
        return r

    # ---- the headline (N = 1): K steps through the capture stream, D2H of every step's compact outputs included ---------------------
    stream_rec = {}
    last_host = None
    dump = None                                              # --dump-outputs: name -> the last timed step's array
    headline_dt = None
    kernel_ms = []
    ramp_passes = 0
    if use_stream:
        from dataclasses import replace
        # The blob of the headline steps carries the pulse table, the bits, the pauses and the message offsets: 3.5 MB per GiB.
        # bit_sample_pos is a function of the pulse table (the reference computes it from ppseq on the host, ProtocolAnalyzer.py:346-401, and
        # makes it optional: write_bit_sample_pos): HostBits.bit_sample_pos() derives it from the shipped rows when asked -- the parity
        # record below compares exactly that with the reference's positions.  The variant that computes the positions on the device
        # and ships them (uint32, +5.4 MB) is timed right after it (ms_per_step_with_device_positions).
        st = pipe.stream(n, replace(p, write_bit_sample_pos=False), want_qad=want_qad, want_pos=False)

        def stream_steps(k):
            out = []
            for _ in range(k):
                r = st.push(iq)
                if r is not None:
                    out.append(r)
            return out + st.flush()
        one, one_tp = [], []
        for mode, acc in ((1, one), (0, one_tp)) if full else ():    # ONE capture start to finish, nothing to overlap with: the stream in its
            pipe.ctx.set_tuning("stream_latency", mode)      # latency setting (an idle pipeline: the tail in segments beside the hot kernel) and
            for _ in range(6):                               # in the throughput setting the K-step loop below runs in (staged passes)
                torch.cuda.synchronize()
                t_l = time.perf_counter()
                stream_steps(1)
                acc.append(time.perf_counter() - t_l)
        pipe.ctx.set_tuning("stream_latency", 0)
        ramp_passes = ramp(lambda: stream_steps(10))
        torch.cuda.synchronize()
        # (no timing events in this loop: the dispatch-attached pair costs 5-7 us per pass while a profile record is open; the hot kernel's
        # duration is measured in the device-only loop below, whose event timing agrees with rocprofv3 -- URH_BENCH_HEADLINE_EVENTS=1: here)
        pipe.ctx.profile_begin(args.steps if os.environ.get("URH_BENCH_HEADLINE_EVENTS") else 0)
        t0 = time.perf_counter()
        results = stream_steps(args.steps)                   # K pushes, then the copies still in flight: ends with the last byte on the host
        torch.cuda.synchronize()
        headline_dt = time.perf_counter() - t0
        kernel_ms = pipe.ctx.profile_end()
        assert len(results) == args.steps and [r.seq for r in results[-3:]] == sorted(r.seq for r in results[-3:])
        last_host = results[-1].check()
        import numpy as np
        from urh_amd import _lib as _ulib
        import ctypes as C
        if args.dump_outputs:                                # the last timed step's outputs, before a later pass can reuse their buffers
            dump = {"ppseq": last_host.ppseq(), **dict(zip(FLAT_NAMES, last_host.flat()))}
            if want_qad and last_host.d_qad_ptr:
                def read_qad(s, k):
                    a = np.empty(k, np.float32)
                    _ulib.check(_ulib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(last_host.d_qad_ptr + 4 * s),
                                                                   a.ctypes.data_as(C.c_void_p), k * 4))
                    return a
                dump["qad_sample"], dump["qad_sample_starts"] = qad_sample(n, read_qad)
        stream_rec = {"d2h_bytes_per_step": last_host.blob_bytes + 40, "stream_stats": st.stats(),
                      "d2h_format": "compact blob: uint16 length (rows of 65535 samples and more through an escape list) + int8 state per pulse-table row, packed bits, int64 pauses / message offsets "
                                    "(include/urhgpu.h); bit_sample_pos derived on the host from the shipped pulse table when asked for"}
        host_copy = {"counts": (last_host.n_rows, last_host.n_msg, last_host.n_bits, last_host.n_pos)}
        qad_host = None
        if full:
            # where the host's time goes in such a loop (a second, untimed run of the same K steps): inside push() -- which blocks until the
            # tail of the pass before last has finished -- and between two pushes (Python: wrapping the result)
            t_in, t_out, t_prev = [], [], None
            for _ in range(args.steps):
                ta = time.perf_counter()
                if t_prev is not None:
                    t_out.append(ta - t_prev)
                st.push(iq)
                t_prev = time.perf_counter()
                t_in.append(t_prev - ta)
            st.flush()
            torch.cuda.synchronize()
            t_in.sort(); t_out.sort()
            host_rec = {"push_us_median": round(t_in[len(t_in) // 2] * 1e6, 1), "push_us_min": round(t_in[0] * 1e6, 1),
                        "between_pushes_us_median": round(t_out[len(t_out) // 2] * 1e6, 1)}
            stream_rec.update({"single_capture_incl_compact_d2h_ms": round(min(one) * 1e3, 4),
                               "single_capture_setting": "CaptureStream(latency=True) / tuning stream_latency=1: a pass that finds the pipeline idle runs its tail in 7 rows "
                                                         "segments + 1 bits segment beside the hot kernel; the K-step loop runs in the throughput setting (staged passes), in "
                                                         "which one capture alone takes single_capture_throughput_setting_ms",
                               "single_capture_throughput_setting_ms": round(min(one_tp) * 1e3, 4),
                               "host_loop": host_rec, "stream_stats": st.stats()})
            # the last timed step's outputs for the parity record: host copies of the blob's sections + its qad read back from HBM
            host_copy.update({"ppseq": last_host.ppseq(), "flat": last_host.flat()})
            if want_qad and last_host.d_qad_ptr:
                qad_host = np.empty(n, np.float32)
                _ulib.check(_ulib.load().urhgpu_memcpy_to_host(pipe.ctx.handle, C.c_void_p(last_host.d_qad_ptr), qad_host.ctypes.data_as(C.c_void_p), n * 4))
        # ---- one capture that starts ON THE HOST (pinned memory): bare H2D copy of the capture against upload + demodulation + results on
        # the host, the pieces demodulated as they land (urhgpu_stream_push_upload) -- SURVEY 8(d): "report H2D-inclusive time separately"
        if full and not args.no_upload:
            try:
                pinned = torch.empty(iq.shape, dtype=iq.dtype, pin_memory=True)
                pinned.copy_(iq)
                dst = torch.empty_like(iq)
                torch.cuda.synchronize()
                bare, incl = [], []
                for _ in range(4):
                    torch.cuda.synchronize()
                    t_l = time.perf_counter()
                    dst.copy_(pinned, non_blocking=True)
                    torch.cuda.synchronize()
                    bare.append(time.perf_counter() - t_l)
                for _ in range(4):
                    dst.zero_()
                    torch.cuda.synchronize()
                    t_l = time.perf_counter()
                    st.push_upload(pinned, dst)
                    up = st.flush()
                    incl.append(time.perf_counter() - t_l)
                up_host = up[-1].check()
                same = (up_host.n_rows, up_host.n_msg, up_host.n_bits) == (last_host.n_rows, last_host.n_msg, last_host.n_bits) and \
                    bool(np.array_equal(up_host.ppseq(), host_copy["ppseq"]) and np.array_equal(up_host.bits(), host_copy["flat"][0]))
                stream_rec.update({"bare_pinned_h2d_ms": round(min(bare) * 1e3, 3), "h2d_inclusive_ms": round(min(incl) * 1e3, 3),
                                   "h2d_inclusive_over_bare": round(min(incl) / min(bare), 4),
                                   "h2d_gbs": round(n * 8 / min(bare) / 1e9, 1),
                                   "h2d_inclusive_equals_resident_result": same,
                                   "h2d_inclusive_what": "pinned host capture -> urhgpu_stream_push_upload (pieces copied and demodulated as they land) -> "
                                                         "compact outputs in pinned host memory; min of 4, against the bare copy of the same 1 GiB"})
                del pinned, dst, up, up_host
            except Exception as exc:                          # (a box without 1 GiB of pinnable memory: the line says so)
                stream_rec["h2d_inclusive_error"] = repr(exc)[:200]
        st.close()
        # the same with bit_sample_pos computed on the device and shipped (uint32 per bit: 8.9 MB per GiB instead of 3.5)
        if full and not args.no_device_loop:
            st = pipe.stream(n, p, want_qad=want_qad, want_pos=True)
            ramp(lambda: stream_steps(10))
            torch.cuda.synchronize()
            t_np = time.perf_counter()
            r_np = stream_steps(args.steps)
            torch.cuda.synchronize()
            stream_rec["ms_per_step_with_device_positions"] = round((time.perf_counter() - t_np) / args.steps * 1e3, 4)
            stream_rec["with_device_positions_stream_stats"] = st.stats()
            stream_rec["d2h_bytes_per_step_with_device_positions"] = r_np[-1].blob_bytes + 40
            import numpy as np
            stream_rec["device_positions_equal_derived"] = bool(np.array_equal(r_np[-1].bit_sample_pos(), host_copy["flat"][3]) and
                                                                 np.array_equal(r_np[-1].pos_offsets(), host_copy["flat"][4]))
            st.close()
            del r_np
            stream_rec["value_with_positions"] = round(n / stream_rec["ms_per_step_with_device_positions"] / 1e3, 1)
        del st, results
        if full and not args.no_device_loop and not args.no_variants:
            try:
                stream_rec["variants"] = variant_steps(torch, pipe, iq, p, n, args, ramp, host_copy)
            except Exception as exc:                          # noqa: BLE001 (the headline stands; the line says what went wrong)
                stream_rec["variants"] = {"error": repr(exc)[:300]}

    # ---- the headline of sharded runs (N > 1): the same window per rank -- every pass's compact blob (this rank's piece: pulse table,
    # bits, pauses, offsets; bit_sample_pos derived on the host when asked for) copied to pinned host memory by a third stream while
    # the following passes run (GpuShardEngine(host_results=True)); the region ends when every rank has its last blob ------------------
    sharded_host = sharded and args.pipeline and not args.no_d2h and fir_taps is None
    host_piece = None
    if sharded_host:
        from dataclasses import replace
        p_host = replace(p, write_bit_sample_pos=False)

        def host_steps(k):
            pend, last = [], None
            for _ in range(k):
                pend.append(pipe.iq_to_bits(iq, p_host, want_qad=want_qad, halo_given=halo_given, left_halo=left_halo))
                if len(pend) > 2:                             # two passes behind the one just issued: its copy has had a pass to finish
                    last = pend.pop(0).host()
            for r in pend:
                last = r.host()
            return last
        pipe.engine.host_results = True
        ramp_passes = ramp(lambda: host_steps(10))
        dist.barrier()
        torch.cuda.synchronize()
        pipe.ctx.profile_begin(args.steps if os.environ.get("URH_BENCH_HEADLINE_EVENTS") else 0)
        t0 = time.perf_counter()
        host_piece = host_steps(args.steps).check()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        headline_dt = time.perf_counter() - t0
        kernel_ms = pipe.ctx.profile_end()
        t = torch.tensor([headline_dt], dtype=torch.float64, device=_FLAG_DEV)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        headline_dt = float(t.item())
        stream_rec = {"d2h_bytes_per_step": host_piece.blob_bytes,
                      "d2h_format": "compact blob of this rank's piece: int32 length + int8 state per pulse-table row, packed bits, int64 pauses / "
                                    "message offsets (include/urhgpu.h); bit_sample_pos derived on the host from the shipped pulse table when asked for"}
        host_copy = {"rows": host_piece.ppseq().copy(), "bits": host_piece.bits().copy(), "pauses": host_piece.pauses.copy()}
        if args.dump_outputs:                                # this rank's piece of the last timed step, as it arrived on the host
            dump = {"ppseq": host_copy["rows"], "bits": host_copy["bits"], "msg_off": host_piece.msg_off.copy(), "pauses": host_copy["pauses"]}
        pipe.engine.host_results = False
        pipe.ctx.join()
        torch.cuda.synchronize()

    # ---- device only (outputs left in HBM): what round 2 reported as the headline -- with --full, or when it is the timed path
    # (--no-d2h, --no-pipeline) ------------------------------------------------------------------------------------------------------
    device_only_ms = host_equals_device = None
    if full or headline_dt is None:
        if use_stream and args.no_device_loop:
            args_steps_dev = 1
        else:
            args_steps_dev = args.steps
            rp_dev = ramp(lambda: device_steps(10))
            if not use_stream and not sharded_host:
                ramp_passes = rp_dev
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        kernel_from_device_loop = not kernel_ms and not os.environ.get("URH_BENCH_NO_PROFILE") and args_steps_dev == args.steps
        pipe.ctx.profile_begin(args.steps if kernel_from_device_loop else 0)
        t0 = time.perf_counter()
        res = device_steps(args_steps_dev)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if kernel_from_device_loop:
            kernel_ms = pipe.ctx.profile_end()
        else:
            pipe.ctx.profile_end()
        if dist:
            t = torch.tensor([dt], dtype=torch.float64, device=_FLAG_DEV)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        device_only_ms = dt / args_steps_dev * 1e3
        if headline_dt is None:
            headline_dt = dt

        counts = res.host_counts()
        res.check_capacity()
        if sharded_host:                                         # what arrived on the host is what the device-resident pass holds
            import numpy as np
            pc = res.piece()
            host_equals_device = bool(np.array_equal(host_copy["rows"], pc["rows"]) and np.array_equal(host_copy["bits"], pc["bits"]) and
                                      np.array_equal(host_copy["pauses"], pc["pauses"]))
            assert host_equals_device, "host blob differs from the device-resident outputs"
        if use_stream:
            assert tuple(host_copy["counts"][:3]) == tuple(counts[:3]), (host_copy["counts"], counts)     # (the stream's blob ships no positions)
    elif use_stream:
        counts = host_copy["counts"]
    else:
        counts = (host_piece.n_rows, host_piece.n_msg, host_piece.n_bits, host_piece.n_pos)
    if args.dump_outputs and dump is None:                   # the device-resident loop was the timed one: its last step's outputs
        if sharded:
            pc = res.piece()
            dump = {"ppseq": pc["rows"], "bits": pc["bits"], "msg_end": pc["msg_end"], "pauses": pc["pauses"], "bit_sample_pos": pc["pos"],
                    "pos_end": pc["pos_end"]}
        else:
            dump = {"ppseq": res.ppseq(), **dict(zip(FLAT_NAMES, res.flat()))}
            if res.qad is not None:
                dump["qad_sample"], dump["qad_sample_starts"] = qad_sample(n, lambda s, k: res.qad[s:s + k].cpu().numpy())

    # For reference the N = 1 line also carries the same K steps run one after the other, nothing overlapped: step time
    # and the hot kernel's duration when it has the machine to itself.
    alone_ms, alone_kernel_ms = None, None
    ceiling = None
    if full and not sharded and n % 8192 == 0:           # (while the context is still pipelined: its CU-masked hot stream exists)
        ceiling = copy_ceiling(torch, pipe, iq, n)
    if full and not sharded and args.pipeline and not args.no_reference_loop:
        pipe.ctx.join()
        torch.cuda.synchronize()
        pipe.ctx.set_pipelined(False)                    # the same context and buffers, passes one after the other from here on
        for _ in range(max(args.warmup, 1)):
            step()
        torch.cuda.synchronize()
        pipe.ctx.profile_begin(0 if os.environ.get("URH_BENCH_NO_PROFILE") else args.steps)
        tp = time.perf_counter()
        for _ in range(args.steps):
            rp = step()
        torch.cuda.synchronize()
        alone_ms = (time.perf_counter() - tp) / args.steps * 1e3
        ka = pipe.ctx.profile_end()
        alone_kernel_ms = sum(ka) / len(ka) if ka else None
        assert rp.host_counts() == counts
        res = rp

    shard_parity = fir_halo_rec = None               # (filled in below, after everything else of the line has been put together)

    ranks_info = None
    if dist:
        info = [None] * world
        dist.all_gather_object(info, {"rank": rank, "device": torch.cuda.get_device_name(dev), "index": local_rank,
                                      "rows": counts[0], "bits": counts[2]})
        ranks_info = info

    if rank == 0:
        total_samples = n * world
        ms_per_step = headline_dt / args.steps * 1e3
        value = total_samples * args.steps / headline_dt / 1e6
        bytes_per_sample = ALGO_BYTES_PER_SAMPLE if want_qad else 8

        def frac_of(ms):
            return round(n * bytes_per_sample / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms else None
        out = {
            "metric": "Msamples/s IQ->bits (1 GiB complex64 2-FSK per GPU, qad materialised"
                      + (", compact outputs copied to the host)" if (use_stream or sharded_host) else ")"),
            "value": round(value, 1), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[1]: 1 GiB synthetic complex64 2-FSK @ 100 samples/symbol per GPU"
                       if world == 1 else f"configs[3]-style: {world} GiB complex64 2-FSK sharded sample-contiguously over {world} GPUs"
                       + (" with the 64-tap FIR (63-sample halo exchange) in front" if fir_taps is not None else ""),
                       "capture": capture,
                       "timed_region": ("K steps through urhgpu_stream_*: IQ resident in HBM -> qad (HBM) + pulse table + bits + pauses -> "
                                        "compact blob -> pinned host memory; hot kernel of step i, tail of step i - 1 and D2H copy of step i - 2 overlap; "
                                        "the region ends when the last step's copy has arrived (SURVEY 8(d) window)") if use_stream else
                                       ("K sharded steps per rank: IQ shard resident in HBM -> qad (HBM) + this rank's piece of pulse table / bits / pauses "
                                        "-> compact blob -> pinned host memory (copy stream, three slots); two all-gathers of a few bytes per step; the "
                                        "region ends when every rank holds its last blob (SURVEY 8(d) window per rank)") if sharded_host else
                                       "K device-resident steps (outputs left in HBM)",
                       "samples_per_gpu": n, "samples_per_symbol": sps, "tolerance": tol, "noise_sigma": 0.05,
                       "outputs": (("qad (HBM) + " if want_qad else "") + "pulse table + bits + pauses + message offsets on the host; bit_sample_pos NOT shipped in the "
                                   "headline steps (derived on the host from the shipped pulse table when asked for: HostBits.bit_sample_pos, compared with the "
                                   "reference's in `parity`); shipped as uint32 in ms_per_step_with_device_positions") if (use_stream or sharded_host) else
                                  (("qad+" if want_qad else "") + "ppseq+bits+pauses+bit_sample_pos, left in HBM"),
                       "rows": counts[0], "messages": counts[1], "bits": counts[2],
                       "steps_pipelined": args.pipeline, "clock_ramp_passes_before_timing": ramp_passes,
                       **stream_rec,
                       "rccl_world_size": world if dist else None,
                       "all_gathers_per_pass": (None if not sharded else (2 if halo_given else 3) + (1 if fir_taps is not None else 0)),
                       "collectives": (None if not sharded else type(pipe.comm).__name__),
                       "collectives_fallback_reason": (comm_fallback_reason if sharded else None),
                       "ranks": ranks_info,
                       "full": full},
            # the headline's own fraction of HBM peak; the kernel's figures (device-only loop, live PMC passes) come with --full
            "roofline": {"bound": "hbm", "kernel": "k_demod_runs_bp", "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "algorithmic_bytes": n * bytes_per_sample, "algorithmic_bytes_per_sample": bytes_per_sample,
                         "end_to_end_frac": frac_of(ms_per_step)},
        }
        if full:
            k_ms = sum(kernel_ms) / max(len(kernel_ms), 1)
            achieved = (n * bytes_per_sample) / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
            traffic = traffic_src = None
            if want_qad and n == 128 * SEG:
                if world == 1 and not force_sharded and not args.no_pmc and not args.no_extra:
                    traffic, traffic_src = pmc_traffic_live(args.segments, "k_demod_runs_bp<0, 4, 1, true")
                if traffic is None:
                    why = traffic_src
                    traffic, traffic_src = pmc_traffic("k_demod_runs_bp<0, 4, 1, true")
                    if traffic is not None and why:
                        traffic_src += f" [no live PMC pass: {why}]"
            out["config"].update({
                "host_libm": __import__("urh_amd._lib", fromlist=["_lib"]).host_libm_verdict(warn=False),
                "device_only_ms_per_step": round(device_only_ms, 4),
                "single_step_latency_ms": round(latency_ms, 4) if latency_ms is not None else None,
                "single_step_plus_wide_d2h_ms": round(min(lat_d2h) * 1e3, 4) if lat_d2h else None, "wide_d2h_bytes": d2h_bytes_wide,
                "unpipelined_ms_per_step": round(alone_ms, 4) if alone_ms is not None else None,
                "host_blob_equals_device_outputs": host_equals_device,
                "sharded_parity": shard_parity, "parity_bit_exact": (shard_parity or {}).get("bit_exact") if sharded else None,
                "fir_halo": fir_halo_rec})
            out["roofline"].update({
                "achieved": round(achieved, 1), "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_unit": "bytes/launch",
                "traffic_source": traffic_src, "kernel_ms": round(k_ms, 4),
                "kernel_timing": ("HIP events attached to the kernel's dispatch (hipExtLaunchKernelGGL: the kernel's own begin / end timestamps), K pipelined "
                                  "device-only steps right after the timed region -- beside the previous step's tail, as in the timed region, whose loop carries "
                                  "no events (they cost 5-7 us per pass)") if (use_stream or sharded_host) and not os.environ.get("URH_BENCH_HEADLINE_EVENTS") else
                                 "HIP events attached to the kernel's dispatch, inside the timed region",
                "kernel_ms_unshared": round(alone_kernel_ms, 4) if alone_kernel_ms else None,
                "frac_unshared": frac_of(alone_kernel_ms),
                "copy_ceiling": ceiling,
                "copy_ceiling_gbs": max(v for k, v in ceiling.items() if k.startswith("hot_kernel_shape") and k.endswith("_gbs")) if ceiling else None,
                "frac_of_copy_ceiling": round(achieved / max(v for k, v in ceiling.items() if k.startswith("hot_kernel_shape") and k.endswith("_gbs")), 4)
                if ceiling else None,
                "end_to_end_device_only_frac": frac_of(device_only_ms),
                "end_to_end_single_capture_frac": frac_of(stream_rec.get("single_capture_incl_compact_d2h_ms"))})
        if full and not args.no_cpu_baseline and world == 1 and not force_sharded:
            host = iq.cpu().numpy()
            rec, ref_out = cpu_reference(host, p)
            out["cpu_baseline"] = rec
            if use_stream:
                class _Last:                                 # the host copies taken right after the timed region
                    qad = None
                    ppseq = staticmethod(lambda: host_copy["ppseq"])
                    flat = staticmethod(lambda: host_copy["flat"])
                out["parity"] = parity_record(_Last, ref_out, tx_bits, rec["kind"], got_qad=qad_host)
            else:
                out["parity"] = parity_record(res, ref_out, tx_bits, rec["kind"])
            out["config"]["parity_bit_exact"] = out["parity"]["bit_exact"]
            bo = (out["config"].get("variants") or {}).get("bits_only")
            if bo is not None:                               # the bits-only steps gave the headline's outputs, which equal the reference's
                bo["bit_exact"] = bool(bo.get("equals_headline_outputs") and out["parity"]["rows_equal"] and out["parity"]["bits_equal"]
                                       and out["parity"]["msg_off_equal"] and out["parity"]["pauses_equal"])
            del host, ref_out
        if full and not args.no_extra and world == 1 and not force_sharded:
            del iq
            pipe.ctx.join()
            torch.cuda.synchronize()
            out["extra"] = run_extras(DevicePipeline(local_rank, pipelined=False), dev, args)     # stage by stage: nothing overlapped
            # the driver keeps `config` and `roofline`: the other configurations' verdicts and times in short form there
            for key, ex in zip(("configs2_ook_fir", "configs4_psk_costas"), out["extra"]):
                out["config"][key] = {"ms": ex.get("ms"), "ms_incl_d2h": ex.get("ms_incl_d2h"), "Msamples_per_s": ex.get("value"),
                                      "bit_exact": (ex.get("parity") or {}).get("bit_exact"), "error": ex.get("error")}
    if dump is not None:
        write_dump(args.dump_outputs, dump, prefix=f"rank{rank}_" if world > 1 else "")
    # ---- N > 1 (--full): the line proves itself -- stitched pieces against a single-GPU pass over the whole capture on rank 0 and against the
    # reference on rank 0's shard; then the FIR-halo variant BASELINE.json configs[3] names (timed, checked the same way).  It comes LAST
    # and under a watchdog: the checks add collectives (gathers of the pieces and of the shards) that the timed region never needed, and a
    # rank that hangs or dies in them must not cost the run its line -- after URH_BENCH_CHECK_TIMEOUT seconds (default 240) rank 0 prints
    # the line it has, marked as unchecked, and every rank exits.
    if full and sharded and not args.no_sharded_check:
        import threading
        line = {"out": out if rank == 0 else None}

        def bail():
            if rank == 0 and line["out"] is not None:
                line["out"]["config"]["sharded_parity"] = {"error": "the self-check did not finish within the watchdog's time: this line is UNCHECKED"}
                line["out"]["config"]["parity_bit_exact"] = None
                os.write(real_stdout, (json.dumps(line["out"]) + "\n").encode())
            os._exit(0 if rank == 0 else 3)
        dog = threading.Timer(float(os.environ.get("URH_BENCH_CHECK_TIMEOUT", "240")), bail)
        dog.daemon = True
        dog.start()
        try:
            pipe.ctx.join()
            torch.cuda.synchronize()
            shard_parity = sharded_self_check(torch, dist, pipe, iq, p, rank, world, local_rank, fir_taps, halo_given, left_halo,
                                              with_oracle=not args.no_cpu_baseline)
            if fir_taps is None:
                from urh_amd.synth import spec_fir_taps
                taps64 = torch.from_numpy(spec_fir_taps().view("float32").reshape(-1, 2).copy()).to(dev)
                fir_halo_rec = sharded_self_check(torch, dist, pipe, iq, p, rank, world, local_rank, taps64, False, None, with_oracle=False,
                                                  steps=min(args.steps, 10), left_raw=left_raw65)
                if fir_halo_rec is not None:
                    fir_halo_rec["what"] = ("configs[3] FIR-halo variant: every rank filters its shard with the 64-tap complex FIR, the 63 samples before the shard "
                                            "as history, then the sharded IQ->bits pass on the filtered shard (two all-gathers: summaries, flags); the halo -- 65 raw "
                                            "samples, 520 bytes -- comes with the shard; device-resident steps, max over ranks")
                    fir_halo_rec["Msamples_per_s"] = round(n * world / (fir_halo_rec["ms_per_step"] * 1e-3) / 1e6, 1)
        except Exception as exc:                                 # noqa: BLE001 (said in the line; the timed numbers stand)
            shard_parity = {"error": repr(exc)[:300]}
        dog.cancel()
        if rank == 0:
            out["config"]["sharded_parity"] = shard_parity
            out["config"]["parity_bit_exact"] = (shard_parity or {}).get("bit_exact")
            out["config"]["fir_halo"] = fir_halo_rec
    if rank == 0:
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if dist:
        import threading
        end = threading.Timer(60.0, lambda: os._exit(0))           # the line is out: a rank that hangs in the tear-down must not hold the launcher
        end.daemon = True
        end.start()
        pipe.ctx.join()
        torch.cuda.synchronize()
        if hasattr(pipe.comm, "close"):
            pipe.comm.close()                                # the library's own RCCL communicator, before torch's
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
