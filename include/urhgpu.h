/*
 * urhgpu.h -- C ABI of the MI355X-native IQ->bits path (liburhgpu.so).
 *
 * This is the drop-in boundary for the reference's native layer: every entry point replaces one
 * Python-visible function of the reference's Cython modules (urh.cythonext.signal_functions /
 * util / auto_interpretation) or the one pure-Python tail function that sits on the hot path
 * (ProtocolAnalyzer._ppseq_to_bits).  Reference citations are relative to /root/reference.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns an int status
 *     (URHGPU_OK == 0, negative == error, see urhgpu_strerror); nothing throws across the ABI.
 *   - "host" entry points take host pointers (numpy buffers): they upload, run the kernels and
 *     download, synchronously.  They mirror the reference functions 1:1 (same argument meaning,
 *     same edge cases) and are what the ctypes shim urh_amd/signal_functions.py calls.
 *   - "_dev" entry points take DEVICE pointers (hipMalloc / torch tensors' data_ptr()) and are
 *     asynchronous on the context's stream; nothing is copied to the host unless stated.  They
 *     are what a device-resident pipeline (urh_amd/pipeline.py, bench.py) calls.
 *   - Inputs are borrowed and never written; outputs are caller-allocated; device scratch is
 *     owned by the context and grows on demand (never inside a steady-state call).
 *   - dtype codes follow the reference's fused `iq` type (src/urh/cythonext/util.pxd:1-8).
 *   - Not thread-safe per context; use one context per host thread (fork/spawn safe: HIP is
 *     initialised lazily by urhgpu_ctx_create in the calling process).
 */
#ifndef URHGPU_H
#define URHGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define URHGPU_VERSION 100 /* 0.1.0 */

/* status codes */
#define URHGPU_OK 0
#define URHGPU_ERR_HIP (-1)          /* a HIP runtime call failed (urhgpu_last_hip_error) */
#define URHGPU_ERR_DTYPE (-2)        /* reference: ValueError("Unsupported dtype") signal_functions.pyx:283,354 */
#define URHGPU_ERR_ARG (-3)          /* bad argument (null pointer, negative size, misaligned device pointer) */
#define URHGPU_ERR_CAPACITY (-4)     /* caller-provided output capacity too small; *n_* holds the needed size */
#define URHGPU_ERR_UNSUPPORTED (-5)  /* parameter outside the supported range (e.g. bits_per_symbol > 7) */
#define URHGPU_ERR_NO_DEVICE (-6)    /* no usable GPU: the product path never falls back to the CPU */

/* dtype codes: element type of the interleaved (N,2) IQ array (util.pxd:1-8) */
#define URHGPU_DT_I8 0
#define URHGPU_DT_U8 1
#define URHGPU_DT_I16 2
#define URHGPU_DT_U16 3
#define URHGPU_DT_F32 4

/* modulation codes (Signal.modulation_type strings; signal_functions.pyx:31-44) */
#define URHGPU_MOD_ASK 0
#define URHGPU_MOD_FSK 1
#define URHGPU_MOD_PSK 2
#define URHGPU_MOD_OTHER 3 /* "OQPSK"/"QAM"/...: no demod branch in afp_demod (result stays 0) */
#define URHGPU_MOD_OQPSK 4 /* urhgpu_modulate* only: get_oqpsk_bits + PSK + half-symbol blanking (signal_functions.pyx:118-121, 165-169) */

typedef struct urhgpu_ctx urhgpu_ctx;

/* ---- context ---------------------------------------------------------------------------------- */
int urhgpu_version(void);
const char *urhgpu_strerror(int status);
const char *urhgpu_last_hip_error(void);
int urhgpu_device_count(int *count);
/* device = HIP ordinal.  Creates a private stream and an (initially empty) scratch arena. */
int urhgpu_ctx_create(int device, urhgpu_ctx **out);
int urhgpu_ctx_destroy(urhgpu_ctx *ctx);
/* Run on the caller's stream (hipStream_t passed as void*).  NULL is the HIP null stream -- what
 * torch calls the default stream -- NOT the private stream: work is then ordered with everything
 * else the caller enqueues there. */
int urhgpu_ctx_set_stream(urhgpu_ctx *ctx, void *hip_stream);
/* Go back to the context's private (non-blocking) stream. */
int urhgpu_ctx_use_private_stream(urhgpu_ctx *ctx);
int urhgpu_ctx_sync(urhgpu_ctx *ctx);
/* Pipelined mode for back-to-back passes (streaming one capture after the other): urhgpu_iq_to_bits_dev then runs its
 * hot kernel on the context's stream and everything after it (pulse table, bits: latency-bound kernels that leave the GPU
 * nearly empty) on a second stream with three scratch arenas in rotation, so that the NEXT pass's hot kernel overlaps this pass's tail.
 * tail_stream: a hipStream_t of the caller (e.g. a torch stream) or NULL for a private one.  In this mode the outputs of a
 * pass are complete only after urhgpu_ctx_join (the context's stream waits for the tail; the host does not block) or
 * urhgpu_ctx_sync; every other entry point joins first.  enable = 0 switches back (synchronises).
 * Measured on MI355X: 0.30 ms per 1 GiB pass against 0.34 ms one after the other; bench.py times this mode.
 * The hot kernel itself is launched on a private stream of the context (CU-masked, see "hot_cus_removed_per_xcd" below), ordered
 * behind what the caller has queued on the context's stream; it is a stream with default flags, i.e. it synchronises with the NULL
 * stream as every such stream does: callers that queue unrelated work on the NULL stream meanwhile serialise with the hot kernels.
 * A caller that runs more than two passes ahead of the GPU is held back on the HOST at the start of the next pass until the tail
 * that last used the pass's scratch arena has finished (bounded run-ahead).
 * The library reads no environment variable; tuning values of this mode are set with urhgpu_ctx_set_tuning. */
int urhgpu_ctx_set_pipelined(urhgpu_ctx *ctx, int enable, void *tail_stream);
/* Tuning values of the pipelined mode (the defaults are what is measured and shipped; tools/ab.sh sets others).  Nine keys; the knobs
 * earlier rounds measured as useless are gone (their records: profiles/HISTORY.md).
 *   "hot_lds_kb"               dynamic LDS per hot workgroup in KiB (fewer of them per CU); default 0
 *   "hot_lds_kb_sharded"       the same for the urhgpu_shard_* passes that keep the generic tail (ASK); default 33
 *   "hot_cus_removed_per_xcd"  0 .. 16, default 4; set before urhgpu_ctx_set_pipelined: the hot kernel of a pipelined pass runs on a private
 *                              stream whose CU mask leaves that many CUs of every XCD out -- on 224 of the MI355X's 256 CUs the kernel is 5 %
 *                              faster than on all of them, and the CUs left alone serve the previous pass's tail; 0: no mask
 *   "profile_bracket"          1: urhgpu_ctx_profile_* report the stream-level bracket, which reads 3-5 % longer than the kernel runs
 *   "stream_policy"            which tail a pass of urhgpu_stream_* takes.  5 (default): 6 (4 with "stream_latency") for passes that ship no
 *                              positions or ship them directly, 0 otherwise; 0: segments beside the hot kernel when nothing of an earlier pass is still running (one
 *                              capture, where the tail's latency counts), else the blob is packed at the end and copied by the copy engine;
 *                              1: every qualifying pass in segments; 2: never; 3: every qualifying pass DIRECT -- the ordinary tail behind the
 *                              hot kernel, whose kernels store rows and packed results into the pinned host blob themselves; 4: segments when
 *                              idle, direct otherwise; 6 (what 5 resolves to for back-to-back passes since round 6): STAGED -- the direct pass's
 *                              kernels store into a staging blob in HBM, one small kernel tightens it and the copy engine ships it with one
 *                              copy of the predicted size (kernel stores into pinned host memory beside the next hot kernel cost that kernel
 *                              10 us per GiB pass: profiles/r06b_skips.txt)
 *   "stream_latency"           1: under the default policy a pass that finds the pipeline idle -- ONE capture -- runs its tail in segments
 *                              (lowest latency); 0, default: direct passes throughout (highest throughput for back-to-back passes)
 *   "stream_segments"          rows segments of a segmented pass, 1 .. 16, default 7
 *   "stream_pos_direct"        1, default: direct passes ship bit_sample_pos themselves (uint32 stores of the kernels that compute them)
 *   "spin_wait"                1, default: the estimator calls poll their stream instead of blocking in the runtime (a blocking wait wakes
 *                              the host tens of microseconds late: 0.09 ms of config 3's estimate)
 *   "upload_pieces"            2 .. 16, default 4: pieces of urhgpu_stream_push_upload, the last one short
 *   "wide_int"                 1: one-shot and sharded passes over SIGNED INTEGER FSK captures take the hot kernel's instantiation with the
 *                              wide loop (phase steps beyond the fast loop's window, e.g. +-100 kHz at 1 MS/s: a quarter faster there, 5 %
 *                              slower on narrow captures); capture streams decide by themselves from a probe of their captures.  default 0
 *   "costas_dev_rounds"        who drives the re-speculation rounds of the parallel Costas loop (PSK, more than 8192 samples).  -1, default: the
 *                              host for one-shot passes on a context that is not pipelined (one stream synchronisation per round), the device in
 *                              capture streams and on pipelined contexts, with a number of rounds queued that follows from the capture's length.
 *                              0 .. 24: the device everywhere, with exactly that many re-speculation rounds queued behind the first; a chain still
 *                              open after them is finished serially.  The demodulated signal is the same bit for bit whatever the value.
 *   "auto_center_max_bins"     1 .. 2^20, default 4096: bins the histogram pool of the automatic center holds for its one range
 *                              (urhgpu_detect_center_dev, urhgpu_iq_to_bits_auto_center_dev; also the room a capture stream leaves for a tied
 *                              histogram, so set it before urhgpu_stream_set_auto_center).  A histogram with more bins comes back as flag 2
 *   "shard_summary_generic"    1: the local pass of urhgpu_shard_runs_dev as the three generic resolve launches instead of the one-launch
 *                              summary kernel (A/B and test use: the summaries are byte-equal).  default 0
 * Unknown key: URHGPU_ERR_ARG. */
int urhgpu_ctx_set_tuning(urhgpu_ctx *ctx, const char *key, int value);
int urhgpu_ctx_join(urhgpu_ctx *ctx);
/* Pre-size the scratch arena for captures of up to n samples with the given tolerance so that no
 * allocation happens inside later calls (bench / steady state). */
int urhgpu_ctx_reserve(urhgpu_ctx *ctx, int64_t n_samples, int tolerance);
/* Device properties the host side needs to size launches / report rooflines. */
int urhgpu_ctx_info(urhgpu_ctx *ctx, int *compute_units, int *wavefront, int64_t *hbm_bytes, char *name, int name_cap);

/* Run-time guard for the libm the reference would use on THIS host: the reference's Costas loop and FSK demodulation call the host's
 * sinf / cosf / atan2f (signal_functions.pyx:252-330, :375), which are not correctly rounded -- x86-64 glibc picks an FMA or a non-FMA
 * build of sinf / cosf by CPU, differing on about one float in 10^9 -- and the device code restates the FMA build.  out4 = {sinf / cosf
 * results compared with the host's (including every argument below 120 on which the two builds differ), mismatches, atan2f results
 * compared, mismatches}.  Mismatches != 0: the reference on this host is not the function the GPU path is bit-exact with.  Host
 * arithmetic; works without a GPU. */
int urhgpu_host_libm_check(int64_t *out4);

/* After a PSK demodulation (Costas loop) of more than 8192 samples: how the chunk chain of the exact parallel evaluation was
 * resolved -- out4 = {chunks whose true start state matched a speculative candidate, chunks evaluated serially until they
 * met a candidate's checkpoint, chunks evaluated serially to the end (or fully gated), re-speculation rounds}.
 * Synchronises the stream.  Diagnostics only: the output is exact in every case.
 * (A one-shot PSK pass on a context that is not pipelined synchronises the stream itself, once per round: the host learns whether the
 * chunk chain closed before it launches the next round or the final pass.  On a pipelined context, in a capture stream and with the
 * tuning key "costas_dev_rounds" >= 0 the rounds are driven from the device and the host waits for nothing: the stats are then copied
 * behind the pass's Costas kernels, asynchronously, and are valid once the pass has been synchronised by whoever consumes its result --
 * which these two calls do.)
 * urhgpu_ctx_costas_stats5: the five counters as the kernels keep them -- out5 = {by candidate, by checkpoint, serial, chunk the last
 * stitch stopped in front of (the chunk count: finished), re-speculation rounds}; synchronises every stream of the context. */
int urhgpu_ctx_costas_stats(urhgpu_ctx *ctx, int32_t *out4);
int urhgpu_ctx_costas_stats5(urhgpu_ctx *ctx, int32_t *out5);

/* Time the dominant kernel (demod + run segmentation) of subsequent fused / grab_pulse_lens calls with
 * HIP events on the context's stream: begin(max_records) arms up to max_records records (one per call); end()
 * synchronises the stream and returns the per-call durations in ms.  The bit-plane kernel's dispatch carries the start /
 * stop events itself (hipExtLaunchKernelGGL: the kernel's own begin / end timestamps, the duration rocprofv3 reports);
 * hot launches made of several kernels are bracketed by events recorded before and after them (urhgpu_ctx_set_tuning("profile_bracket",
 * 1): always report the bracket, which reads 3-5 % longer than the kernel runs). */
int urhgpu_ctx_profile_begin(urhgpu_ctx *ctx, int max_records);
int urhgpu_ctx_profile_end(urhgpu_ctx *ctx, float *ms_out, int cap, int *n_records);

/* ---- host-buffer entry points: 1:1 replacements of the reference's Cython functions ------------- */

/* util.get_magnitudes (src/urh/cythonext/util.pyx:128-136): out[i] = sqrt(I*I+Q*Q), float64[n]. */
int urhgpu_get_magnitudes(urhgpu_ctx *ctx, const void *iq, int dtype, int64_t n, double *out);

/* signal_functions.afp_demod (src/urh/cythonext/signal_functions.pyx:333-378).
 * n <= 2 -> zeros.  mod PSK runs the Costas loop (costa_demod, :252-330; out[0] is written as
 * NOISE(-4) here whereas the reference leaves it uninitialised).  noise_other is the NOISE sentinel
 * used when mod == URHGPU_MOD_OTHER (get_noise_for_mod_type, :31-44). */
int urhgpu_afp_demod(urhgpu_ctx *ctx, const void *iq, int dtype, int64_t n, float noise_mag, int mod,
                     int mod_order, float costas_loop_bandwidth, float noise_other, float *qad_out);

/* signal_functions.get_center_thresholds (:380-390): out has modulation_order-1 floats.  Host only. */
int urhgpu_get_center_thresholds(float center, float spacing, int modulation_order, float *out);

/* signal_functions.grab_pulse_lens (:392-495): qad float32[n] -> rows int64[n_rows][2] = [state, length]
 * (state -1 = pause).  rows_out has room for cap_rows rows; *n_rows receives the row count (also on
 * URHGPU_ERR_CAPACITY, so the caller can retry). */
int urhgpu_grab_pulse_lens(urhgpu_ctx *ctx, const float *qad, int64_t n, float center, uint16_t tolerance,
                           int mod, uint32_t samples_per_symbol, uint8_t bits_per_symbol, float center_spacing,
                           float noise_other, int64_t *rows_out, int64_t cap_rows, int64_t *n_rows);

/* ProtocolAnalyzer._ppseq_to_bits (src/urh/signalprocessing/ProtocolAnalyzer.py:323-414), flat outputs:
 *   bits[0..n_bits)      one byte per bit, all messages back to back
 *   msg_off[0..n_msg]    offsets of each message in bits[]
 *   pauses[0..n_msg)     pause after each message, in samples
 *   pos[0..n_pos)        bit_sample_pos arrays back to back (only when write_pos != 0)
 *   pos_off[0..n_msg]    offsets of each message in pos[]
 * counts[3] receives {n_msg, n_bits, n_pos}. */
int urhgpu_ppseq_to_bits(urhgpu_ctx *ctx, const int64_t *rows, int64_t n_rows, int64_t samples_per_symbol,
                         int bits_per_symbol, int write_pos, int64_t pause_threshold,
                         uint8_t *bits, int64_t cap_bits, int64_t *msg_off, int64_t *pauses, int64_t cap_msg,
                         int64_t *pos, int64_t cap_pos, int64_t *pos_off, int64_t *counts);

/* signal_functions.fir_filter (:513-525): complex64 x[n] (*) complex64 taps[m], causal, zero history,
 * accumulation order of the reference's scatter loop.  out always holds n samples; with m = 0 they are n zeros.  (The reference
 * itself returns n - 1 zeros for empty taps and raises ValueError for n = m = 0 -- np.zeros(n + m - 1)[:n]; the Python callers
 * signal_functions.fir_filter and Filter.work shape that from this result, the device routes keep the capture's length.) */
int urhgpu_fir_filter(urhgpu_ctx *ctx, const float *x, int64_t n, const float *taps, int64_t m, float *out);

/* The same on device memory (asynchronous).  d_left_halo: NULL = zero history (the reference), or DEVICE pointer
 * to the m - 1 samples that precede d_x[0] (sharded captures: the left neighbour's tail).
 * Limits (URHGPU_ERR_UNSUPPORTED beyond them, nothing is computed): the taps and one tile of input are staged in LDS, which
 * holds at most 7 950 taps; bits_per_symbol <= 7 (modulation order <= 128) in every entry point that slices. */
int urhgpu_fir_filter_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const float *d_taps, int64_t m,
                          const float *d_left_halo, float *d_out);
/* The same with the magnitude chunk statistics of the OUTPUT fused into the filter's epilogue (Signal.filter_range followed by
 * detect_noise_level, AutoInterpretation.py:60-91, in one pass over the samples): d_sum[k] / d_max[k] (device, float64) for chunk k
 * counted from the end, as urhgpu_magnitude_chunk_stats_dev computes them on a float32 capture. */
int urhgpu_fir_filter_stats_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const float *d_taps, int64_t m, const float *d_left_halo,
                                float *d_out, int64_t chunk, int64_t n_chunks, double *d_sum, double *d_max);

/* Filter.apply_bandpass_filter (src/urh/signalprocessing/Filter.py:84-101; np.convolve(data, h, "same") at :98 and
 * Filter.fft_convolve_1d at :70-82 are the same centred linear convolution): complex64 x[n] (*) complex128 taps[m],
 *   out[i] = sum_{k=0}^{m-1} taps[k] * X(i + shift - k),  i in [0, n_out),  X = x extended by zeros,
 * accumulated in complex128 (fp64 FMAs, taps ascending) -- the reference's summation order is numpy's (BLAS / FFT) and
 * undefined, so this entry point is floating point with a tolerance, not bit-exact.  The caller designs the taps
 * (Filter.py:103-131, O(m) on the host) and passes shift = (min(n, m) - 1) / 2, n_out = max(n, m) for "same".
 * out: n_out complex128 values. */
int urhgpu_bandpass(urhgpu_ctx *ctx, const float *x, int64_t n, const double *taps, int64_t m, int64_t shift,
                    int64_t n_out, double *out);

/* The same on device memory (asynchronous).  d_left / d_right: NULL or DEVICE pointers to n_left samples preceding d_x[0] /
 * n_right samples following d_x[n-1] (sharded captures: the neighbours' edges) instead of zeros.  out_c64 != 0 writes
 * complex64 (the cast of SignalFrame.py:1578-1580 fused into the store), else complex128. */
int urhgpu_bandpass_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const double *d_taps, int64_t m, int64_t shift,
                        int64_t n_out, const float *d_left, int64_t n_left, const float *d_right, int64_t n_right,
                        void *d_out, int out_c64);

/* signal_functions.iir_filter (:527-542). */
int urhgpu_iir_filter(urhgpu_ctx *ctx, const double *a, int64_t na, const double *b, int64_t nb,
                      const float *x, int64_t n, float *out);

/* ---- device-resident entry points ------------------------------------------------------------------ */

/* Demodulation + digitization parameters (Signal.py:42-109 defaults in comments). */
typedef struct urhgpu_params {
    int dtype;                  /* URHGPU_DT_* of the IQ buffer */
    int mod;                    /* URHGPU_MOD_* */
    int bits_per_symbol;        /* 1 */
    float noise_threshold;      /* Signal.noise_threshold (magnitude, not squared) */
    float center;               /* 0.02 */
    float center_spacing;       /* 1.0 */
    int tolerance;              /* 5 */
    uint32_t samples_per_symbol; /* 100 */
    float costas_loop_bandwidth; /* 0.1 */
    int64_t pause_threshold;    /* 8 */
    int write_bit_sample_pos;   /* 1 in the reference (get_protocol_from_signal) */
    float noise_other;          /* NOISE sentinel for URHGPU_MOD_OTHER */
    int mod_order;              /* 0 = 2^bits_per_symbol; afp_demod's mod_order argument (Costas loop order) */
} urhgpu_params;

/* Output descriptor of the fused path.  All pointers are DEVICE pointers owned by the caller; any
 * of qad / pos may be NULL (not materialised).  counts (device int64[5]) receives
 * {n_rows, n_msg, n_bits, n_pos, n_rows_needed}; the caller reads it back (40 bytes) when it needs the sizes.
 * n_rows is clamped to cap_rows; a table that did not fit shows as n_rows == cap_rows. */
typedef struct urhgpu_outputs {
    float *qad;            /* float32[n]  demodulated signal (Signal.qad) or NULL */
    int64_t *rows;         /* int64[cap_rows][2] pulse table (grab_pulse_lens result) */
    int64_t cap_rows;
    uint8_t *bits;         /* uint8[cap_bits] */
    int64_t cap_bits;
    int64_t *msg_off;      /* int64[cap_msg+1] */
    int64_t *pauses;       /* int64[cap_msg] */
    int64_t cap_msg;
    int64_t *pos;          /* int64[cap_pos] or NULL */
    int64_t cap_pos;
    int64_t *pos_off;      /* int64[cap_msg+1] */
    int64_t *counts;       /* int64[5]: {n_rows, n_msg, n_bits, n_pos, rows the table needed (> cap_rows: it was truncated)} */
    /* Optional compact mirror of the results for the trip over PCIe (NULL: not produced): one contiguous blob written by one more
     * kernel at the end of the pass -- see "compact result blob" below.  cap_blob >= urhgpu_blob_capacity(...). */
    void *blob;            /* device, 16-byte aligned */
    int64_t cap_blob;
    /* Optional: pinned HOST memory (hipHostMalloc / torch pin_memory; device-accessible) that receives the five counts as well, stored
     * by the kernel that finalises them -- valid once the pass has completed (an event recorded behind it).  Saves the 40-byte D2H copy
     * a streaming consumer would otherwise queue behind every pass (a copy packet costs the tail chain about 13 us). */
    int64_t *h_counts;
} urhgpu_outputs;

/* ---- compact result blob ---------------------------------------------------------------------------------------------------
 * The wide outputs above mirror the reference's Python objects (grab_pulse_lens' int64 [state, length] rows, one byte per bit,
 * int64 bit_sample_pos): 22.8 MB per GiB of 2-FSK capture at 100 samples per symbol -- 0.5 ms of PCIe, more than the device pass.
 * The blob holds the same information in 8.9 MB (3.5 MB without positions); every section starts 16-byte aligned:
 *   int64 header[16] = {URHGPU_BLOB_MAGIC, n_rows, n_msg, n_bits, n_pos, rows_needed, total_bytes (negative: the blob was too small),
 *                       has_pos, off_pauses, off_msg_off, off_pos_off, off_row_state, off_bits, off_row_len, off_pos32, truncated}
 *   int64 pauses[n_msg]; int64 msg_off[n_msg + 1] (bit offsets); int64 pos_off[n_msg + 1];
 *   int8  row_state[n_rows]   (-1 = pause; grab_pulse_lens' column 0)
 *   uint8 bits[(n_bits + 7) / 8]   eight bits per byte, most significant first (numpy.packbits / unpackbits order)
 *   int32 row_len[n_rows]     (grab_pulse_lens' column 1; captures of up to 2^31 - 1 samples)
 *   (row_state -128: URHGPU_ROW_ABSORBED -- the first row of a rank's piece of a sharded ASK capture that was merged into the previous rank's last row)
 *   uint32 pos32[n_pos]       (bit_sample_pos; absent when the pass wrote no positions)
 * header[7] holds flags: bit 0 has_pos; bit 1 (URHGPU_BLOB_LEN16; staged passes of urhgpu_stream_*, round 6): the row_len section holds
 *   uint16 row_len16[n_rows] instead -- 3 bytes per pulse-table row over PCIe instead of 5 --, a length that does not fit (65535 and more,
 *   or negative) is stored as 0xFFFF and listed behind the packed bits, at the next 16-byte boundary: int64 n_esc, then n_esc pairs
 *   {uint32 row, int32 length} (a capture of n samples has at most n / 65535 + 2 of them)
 *   bit 2 (URHGPU_BLOB_ROW16; the same passes when the pulse table is dense -- more than one row per 64 samples in the pass before): there is
 *   no row_state section; the row_len section holds uint16 row16[n_rows] = (row_state + 1) << 13 | length -- 2 bytes per row --, a length
 *   of 8191 samples and more (or negative) is stored as 0x1FFF and listed at offset header[11] of the blob (the slot names the row_state
 *   section otherwise): int64 n_esc, then n_esc pairs {uint32 row, int32 length} (at most n / 8191 + 2)
 * truncated != 0: bit 0: a capacity was exceeded (rows_needed > cap_rows, or more messages / bits / positions than fit): the sections
 * hold what fitted, the caller repeats the pass with larger capacities; bit 2: a row length did not fit int32, a position uint32 or a
 * state int8 (captures of 2^31 samples and more; sharded captures whose positions are absolute): use the wide outputs; bit 1: a
 * streamed pass's segment gave up waiting for the hot kernel (urhgpu_stream_* reports that as an error).  The counts come first (40 bytes from `counts`), then ONE copy of
 * total_bytes moves everything; urhgpu_stream_* below does that overlapped with the following passes. */
#define URHGPU_BLOB_MAGIC INT64_C(0x55524842424C4F42) /* "URHBBLOB" */
#define URHGPU_BLOB_HEADER_BYTES 128
#define URHGPU_BLOB_LEN16 2      /* header[7] bit 1: 16-bit row lengths + escape list (see above) */
#define URHGPU_BLOB_ROW16 4      /* header[7] bit 2: state and length of a row in one uint16 + escape list (see above) */
int64_t urhgpu_blob_capacity(int64_t cap_rows, int64_t cap_bits, int64_t cap_msg, int64_t cap_pos, int has_pos);

/* The results of a pass that is over, on the host through the compact blob: out = the descriptor the pass was given with out->blob /
 * cap_blob naming a device blob (the pass itself need not have packed it); pack kernel, header, ONE copy of header.total_bytes into
 * host_dst (pinned memory: at PCIe speed).  *total_bytes = the blob's size (also on URHGPU_ERR_CAPACITY: cap_dst too small).
 * Synchronous.  What the boundary objects fetch (urh_amd.pipeline.BitsResult.host(), urh_amd.signal.Signal.bits()) instead of the
 * wide int64 tables; reference shape: ProtocolAnalyzer.py:227-287, :323-414. */
int urhgpu_outputs_to_host(urhgpu_ctx *ctx, const urhgpu_outputs *out, int write_pos, void *host_dst, int64_t cap_dst, int64_t *total_bytes);

/* afp_demod on device memory (ASK/FSK/OTHER: one streaming kernel; PSK: Costas loop). */
int urhgpu_afp_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad);

/* grab_pulse_lens on device memory: d_qad float32[n] -> d_rows; d_n_rows is a device int64. */
int urhgpu_grab_pulse_lens_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t n, const urhgpu_params *p,
                               int64_t *d_rows, int64_t cap_rows, int64_t *d_n_rows);

/* _ppseq_to_bits on device memory (rows -> bits/pauses/positions); uses out->{bits..counts}. */
int urhgpu_ppseq_to_bits_dev(urhgpu_ctx *ctx, const int64_t *d_rows, const int64_t *d_n_rows, int64_t cap_rows_hint,
                             const urhgpu_params *p, const urhgpu_outputs *out);

/* THE fused hot path: IQ (device) -> [qad] -> pulse table -> bits, everything device resident.
 * ASK/FSK run demodulation and run segmentation in ONE pass over the IQ stream (8 B read +
 * 4 B qad write per sample); PSK runs the Costas kernel and then the qad-input segmentation.
 * msg_off[m] .. msg_off[m + 1] delimit message m in bits[] (msg_off[0] = 0); pos_off likewise.
 * Sharded captures use the urhgpu_shard_* phases below instead. */
int urhgpu_iq_to_bits_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p,
                          const urhgpu_outputs *out);

/* ---- automatic center inside a pass, decided on the device --------------------------------------------------------------------
 * The reference's live mode detects the center again for every buffer it demodulates (ProtocolSniffer.py:246-249:
 * detect_center(qad, max_size=150 * samples_per_symbol)); for ASK the center follows the received amplitude, so captures that differ
 * cannot share one.  These entry points run AutoInterpretation.detect_center (AutoInterpretation.py:226-277) for the ONE range [0, n) of
 * a demodulated signal as a chain of kernels that is queued and never waited for: noise removal (x > -4), the 5 % trim, max_size
 * (max_size < 0: none; the trimmed range keeps its first max_size samples, :233-234; 0 leaves nothing: no center), min / max, float32 np.var,
 * the np.arange edges, the histogram, the peak picking.  The chain's scratch is the context's own (not the pass arenas'), and every chain of
 * a context runs on one stream in order: the tail stream of a pipelined context, the context's stream otherwise.
 *   flag 1  center = detect_center's value
 *   flag 0  detect_center returns None (nothing left after the trim, zero or NaN variance, fewer than two edges, no strict peak)
 *   flag 2  the histogram has more bins than the pool holds (tuning key "auto_center_max_bins"): the caller decides (host path)
 *   flag 3  the second and third most populated peaks hold the same count: the reference's result then follows np.argsort's order of
 *           equal keys, which only numpy can tell -- the histogram is handed out (n_counts counts behind the header, when n_bins fits
 *           hist_cap) and the caller settles it with numpy.  Not rare on noisy captures (5 - 13 % of synthetic FSK captures).
 * A result block is a urhgpu_center_result followed by room for hist_cap uint32 counts (hist_cap may be 0). */
typedef struct urhgpu_center_result {
    double center;               /* flag 1: the center; else 0 */
    int64_t flag;
    int64_t n_bins;              /* bins of the histogram (0: there is none) */
    double e0, delta;            /* its edges: e0 + i * delta, i = 0 .. n_bins (np.arange's fill) */
    int64_t kept, trimmed;       /* samples > -4; samples histogrammed (after the trim and max_size) */
    int64_t n_counts;            /* uint32 counts that follow this header: n_bins when flag == 3 and n_bins <= hist_cap, else 0 */
} urhgpu_center_result;
/* The chain alone on d_qad (device, float32[n]); d_result: device memory, sizeof(urhgpu_center_result) + 4 * hist_cap bytes, complete when
 * the work queued so far on the context's stream is.  Asynchronous: no read-back, no wait. */
int urhgpu_detect_center_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t n, int64_t max_size, void *d_result, int64_t hist_cap);
/* IQ -> bits with the center detected inside the pass: demodulate into out->qad (required: URHGPU_ERR_ARG without; k_afp_demod for ASK /
 * FSK / OTHER, the Costas loop for PSK), run the chain on it, derive the slicing thresholds on the device -- urhgpu_get_center_thresholds'
 * arithmetic on (float)center --, segment the demodulated signal with them, bits, pack.  On a pipelined context everything behind the
 * demodulation runs on the tail stream.  The pass never waits for the device and reads nothing back (PSK on a context that is not
 * pipelined keeps the host-driven Costas rounds unless "costas_dev_rounds" says otherwise).
 * WITH FLAG 0, 2 OR 3 THE QUEUED SLICING USED p->center: the outputs are then those of urhgpu_iq_to_bits_dev with the configured center,
 * and a caller that wants the reference's result for flag 2 / 3 settles the center on the host and slices out->qad again
 * (urhgpu_grab_pulse_lens_dev + urhgpu_ppseq_to_bits_dev).
 * d_result: as above.  h_result: optional pinned host mirror of the same block, written by a kernel of the pass and valid once the pass
 * is over, as out->h_counts is. */
int urhgpu_iq_to_bits_auto_center_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, int64_t max_size,
                                      const urhgpu_outputs *out, void *d_result, void *h_result, int64_t hist_cap);
/* bins the context's histogram pool holds ("auto_center_max_bins"): the hist_cap that never loses a tied histogram */
int64_t urhgpu_center_hist_cap(urhgpu_ctx *ctx);

/* ---- a stream of captures, results on the host -------------------------------------------------------------------------------
 * SURVEY.md §8(d)'s window for this path ends with the compact outputs ON THE HOST.  For capture after capture (the reference's live
 * mode is such a consumer: ProtocolSniffer.py:161-202) three things overlap: the hot kernel of pass i, the tail of pass i - 1 (second
 * stream, urhgpu_ctx_set_pipelined: the stream switches the context to that mode) and the pack kernel + D2H copy of pass i - 2's blob
 * (third stream / copy engine, pinned memory owned by the stream).  Three output slots rotate.
 *   urhgpu_stream_create   n_max: largest capture (samples, < 2^31); p: demodulation + slicing parameters of every pass (ASK / FSK /
 *                          OTHER / PSK -- a PSK pass runs its Costas kernels on the context's stream with the re-speculation rounds driven
 *                          from the device, and the segmentation of the demodulated signal, bits and pack behind them on the tail stream;
 *                          the Costas scratch for n_max is reserved here); want_qad: the
 *                          demodulated signal is materialised (stays in HBM: urhgpu_host_result::d_qad); want_pos: bit_sample_pos
 *                          is produced and shipped; cap_rows: 0 = the default (urhgpu_stream_capacities), else the pulse-table capacity.
 *   urhgpu_stream_push     queue pass i on d_iq (device; must stay valid until the pass has run), its pack kernel and its D2H copy and
 *                          return WITHOUT waiting for any of it (the copy's size is predicted from the pass before; what a prediction
 *                          misses is fetched when the result is handed out); *ready receives the result of pass i - 3 (seq = -1: none
 *                          yet), valid until three pushes later.
 *   urhgpu_stream_flush    wait for every outstanding pass; out3 receives up to three results, oldest first.
 * The pointers of a result are pinned host memory owned by the stream. */
typedef struct urhgpu_stream urhgpu_stream;
typedef struct urhgpu_host_result {
    int64_t seq;                 /* index of the push this result belongs to */
    int64_t n_samples;
    int64_t n_rows, n_msg, n_bits, n_pos, rows_needed;
    int64_t blob_bytes;          /* bytes that crossed PCIe for this pass (+ 40 for the counts) */
    int truncated;               /* see "compact result blob" */
    const int32_t *row_len;      /* pulse table: grab_pulse_lens' [state, length] columns; NULL when the blob carries 16-bit lengths: */
    const uint16_t *row_len16;   /* ... then these (URHGPU_BLOB_LEN16), 0xFFFF = look the row up in esc */
    const void *esc;             /* n_esc pairs {uint32 row, int32 length} */
    int64_t n_esc;
    const int8_t *row_state;
    const uint8_t *bits_packed;  /* numpy.unpackbits(bits_packed)[msg_off[m] : msg_off[m + 1]] = message m */
    const int64_t *msg_off, *pauses, *pos_off;
    const uint32_t *pos32;       /* bit_sample_pos or NULL */
    const void *blob;            /* the whole blob (header first) */
    const float *d_qad;          /* DEVICE: the pass's demodulated signal (overwritten three pushes later) or NULL */
    const uint16_t *row16;       /* URHGPU_BLOB_ROW16: (row_state + 1) << 13 | length per row, 0x1FFF = look the row up in esc; row_len, row_len16 and
                                    row_state are NULL then */
} urhgpu_host_result;
int urhgpu_stream_capacities(int64_t n_max, const urhgpu_params *p, int64_t *cap_rows, int64_t *cap_bits, int64_t *cap_msg, int64_t *cap_pos);
int urhgpu_stream_create(urhgpu_ctx *ctx, int64_t n_max, const urhgpu_params *p, int want_qad, int want_pos, int64_t cap_rows, urhgpu_stream **out);
int urhgpu_stream_destroy(urhgpu_stream *st);
int urhgpu_stream_push(urhgpu_stream *st, const void *d_iq, int64_t n, urhgpu_host_result *ready);
/* The same for a capture that is still ON THE HOST (the reference: IQArray.from_file, IQArray.py:206-227 -> Signal.py:111-112, then
 * ProtocolAnalyzer.get_protocol_from_signal): h_iq (host; pinned memory for PCIe speed) is copied into d_iq (device, n samples of the
 * stream's dtype, the caller's: the capture stays resident there) in PIECES, and every piece is demodulated as it lands -- hot kernel
 * on the piece, the piece's share of the tail, its share of the compact blob stored into pinned host memory.  1 GiB takes some 20 ms
 * over PCIe and 0.3 ms to demodulate: "file in host memory -> bits on the host" costs the upload plus the last piece's kernels.
 * Captures the segmented path does not take (ASK, a partial tile at the end, too short) are uploaded in one copy in front of an
 * ordinary pass.  The copies are ordered behind what the caller has queued on the context's stream; h_iq must stay valid and unchanged, and d_iq
 * untouched, until the pass's result has been handed out (a later push's `ready`, or urhgpu_stream_flush). */
int urhgpu_stream_push_upload(urhgpu_stream *st, const void *h_iq, void *d_iq, int64_t n, urhgpu_host_result *ready);
int urhgpu_stream_flush(urhgpu_stream *st, urhgpu_host_result *out3, int *n_out);
/* Every pass of the stream detects its own center (urhgpu_iq_to_bits_auto_center_dev with this max_size; < 0: none).  Before the first push:
 * the chain's scratch for n_max is reserved here.  The stream must have been created with want_qad.  Such passes take the ordinary route
 * (tail behind the demodulation, pack + copy behind the tail), urhgpu_stream_push_upload one copy in front of the pass. */
int urhgpu_stream_set_auto_center(urhgpu_stream *st, int enable, int64_t max_size);
/* The center of a pass whose result has been handed out (by a push's `ready` or by urhgpu_stream_flush), valid as long as that result:
 * center and flag as above; for flag 3 *hist = the n_bins counts of the histogram (pinned host memory; NULL otherwise, or when the
 * histogram did not fit) with its edges e0 + i * delta.  With flag 0, 2 or 3 the result's rows and bits are those of the configured
 * center: the caller settles flag 2 / 3 and slices d_qad again. */
int urhgpu_stream_center(urhgpu_stream *st, int64_t seq, double *center, int64_t *flag, const uint32_t **hist, int64_t *n_bins, double *e0,
                         double *delta);
/* Diagnostics: out4 = {passes pushed, passes whose predicted copy size fell short (their rest was fetched when the result was handed
 * out), bytes the next copy is sized for, blob capacity}. */
int urhgpu_stream_stats(urhgpu_stream *st, int64_t *out4);
/* PSK streams: the Costas stats (urhgpu_ctx_costas_stats5's five counters) summed over the passes whose results have been handed out. */
int urhgpu_stream_costas_stats(urhgpu_stream *st, int64_t *out5);
/* passes of the stream whose hot kernel was the instantiation with the wide loop for integer captures (signed integer FSK streams probe their
 * captures -- the share of phase steps beyond atan(7/16) per sample -- and pick it from 1 % on; 0 for every other stream) */
int urhgpu_stream_wide_passes(urhgpu_stream *st, int64_t *n_passes);

/* ---- sharded captures: one long capture split sample-contiguously over the GPUs of a node ------------------
 * (there is no reference counterpart: the reference processes a capture in one process.)
 * Each rank calls the four phases below in order on its own context; between the phases the CALLER
 * all-gathers a few bytes per rank (urh_amd/sharding.py does it with torch.distributed = RCCL over xGMI):
 *
 *   halo    : the last 2 IQ samples of every shard                          -> d_left_halo of the next rank
 *             (not exchanged at all when whoever distributed the capture gave every rank the two samples before its shard:
 *             urhgpu_shard_launch_dev; a pass then needs two all-gathers, ASK three)
 *   runs    : hot kernel on the shard + its 72-byte summary (d_summary out) -> all-gather -> d_summaries
 *   rows    : this rank's pulse-table rows; ASK: d_merge (5 x int64) out    -> all-gather -> d_merge_all
 *   prepare : cross-shard ASK merge, per-row scan; d_flags (3 x int64) out  -> all-gather -> d_flags_all
 *   finish  : bits / pauses / bit_sample_pos of this rank's rows
 *
 * The result stays sharded: `out` (given to urhgpu_shard_runs_dev, filled by the later phases) holds the rows
 * that END in this shard and what they expand to; concatenating the ranks' pieces in rank order gives exactly
 * the single-GPU result.  Differences to urhgpu_iq_to_bits_dev's outputs:
 *   - rows[0] may carry state URHGPU_ROW_ABSORBED (ASK: the row merged into the previous rank's last row;
 *     skip it when concatenating);
 *   - msg_off[m + 1] / pos_off[m + 1] are the LOCAL end offsets of the m-th message that closes on this rank;
 *     bits / pos may continue past the last one (the message closes on a later rank);
 *   - counts = {local rows, messages closed here, local bits, local positions}.
 * out->blob (FSK / other, not ASK: URHGPU_ERR_UNSUPPORTED): the finish phase also packs this rank's piece into the compact blob.
 * PSK (Costas loop, orders 2 and 4): two more phases come first, urhgpu_shard_costas_spec_dev and urhgpu_shard_costas_resolve_dev
 * below; the halo is then the previous shard's last demodulated value (one float, exchanged after the resolve phase) and the runs
 * phase segments the shard's Costas output.  urhgpu_shard_prelaunch_dev / urhgpu_shard_launch_dev: URHGPU_ERR_UNSUPPORTED for PSK,
 * as every PSK phase on a pipelined context. */
#define URHGPU_ROW_ABSORBED (-(INT64_C(1) << 62))
#define URHGPU_SHARD_SUMMARY_BYTES 72 /* one shard summary (d_summary; d_summaries = world of them, back to back) */
int urhgpu_shard_runs_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                          int rank, int world, const void *d_left_halo, const urhgpu_params *p,
                          const urhgpu_outputs *out, void *d_summary);
/* Optional: start the hot kernel BEFORE the halo has arrived -- every chunk but the first, which alone reads it -- so that
 * the halo all-gather overlaps the kernel; urhgpu_shard_runs_dev (same arguments + the halo) then only adds the first chunk.
 * On a pipelined context (urhgpu_ctx_set_pipelined) that first chunk and every later phase run on the TAIL stream: d_left_halo
 * must be ready in tail-stream order (make the tail stream, not the context's stream, wait for the halo exchange), and the
 * context's stream never waits for a collective. */
int urhgpu_shard_prelaunch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                               int rank, int world, const urhgpu_params *p, const urhgpu_outputs *out);
/* The halo is known up front (d_left_halo: the two samples before the shard, NULL on rank 0): the whole hot launch, on the context's
 * stream (pipelined contexts: their hot stream); urhgpu_shard_runs_dev (same arguments) then only adds the summary. */
int urhgpu_shard_launch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total,
                            int rank, int world, const void *d_left_halo, const urhgpu_params *p, const urhgpu_outputs *out);
int urhgpu_shard_rows_dev(urhgpu_ctx *ctx, const void *d_summaries, int64_t *d_merge);
int urhgpu_shard_bits_prepare_dev(urhgpu_ctx *ctx, const int64_t *d_merge_all, int64_t *d_flags);
int urhgpu_shard_bits_finish_dev(urhgpu_ctx *ctx, const int64_t *d_flags_all);

/* PSK across shards: the Costas loop carries its state {freq, phase} over the whole capture.  Each rank speculates its shard
 * (candidate trajectories per 4096-sample chunk, as on one GPU) and reduces it to a fixed-size summary; the caller all-gathers the
 * summaries and composes them -- a pure function of the gathered bytes that every rank evaluates alike (urh_amd/sharding.py
 * costas_compose): rank 0 starts in {0.0f, 1.5f}; a shard without an un-gated sample passes the state on; otherwise the state is
 * looked up BITWISE among the shard's first-chunk candidates and the composed chunk maps give its end state.  Where that chain
 * breaks (no candidate starts in the state, or the map is broken) the rank whose start state is known resolves and contributes its
 * true end state in one more all-gather (d_end_state); every rank takes the same number of rounds (<= world).  Exact by construction:
 * states are compared on their bits and never assumed to have converged.
 *   urhgpu_costas_halo_samples: raw samples before its shard that a rank > 0 must be handed (fewer where the capture starts
 *       closer: min(this, pos_base - 1)); host arithmetic.
 *   urhgpu_shard_costas_spec_dev: d_halo = the n_halo raw samples (capture dtype) immediately before the shard, NULL / 0 on rank 0;
 *       out->qad (required) receives the shard's demodulated signal in the next phase (index 0 of rank 0: -4.0, as on one GPU);
 *       d_summary: URHGPU_COSTAS_SUMMARY_BYTES out (layout: costas.hip, k_costas_shard_summary).
 *   urhgpu_shard_costas_resolve_dev: start_state = HOST pointer to the shard's true start state {freq, phase} as float32 bits;
 *       stitches from it (host-driven re-speculation rounds where the chain breaks inside the shard; synchronises the stream),
 *       writes out->qad, and the true state after the shard's last sample to d_end_state (device, 2 x uint32; may be NULL).
 *       urhgpu_ctx_costas_stats then reports the rank's chunks (by map / checkpoint / serial) and re-speculation rounds.
 * Then urhgpu_shard_runs_dev (d_left_halo: the previous rank's last qad value, NULL on rank 0) and the later phases as above. */
#define URHGPU_COSTAS_SUMMARY_BYTES 160
int64_t urhgpu_costas_halo_samples(const urhgpu_params *p);
int urhgpu_shard_costas_spec_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, int rank, int world,
                                 const void *d_halo, int64_t n_halo, const urhgpu_params *p, const urhgpu_outputs *out, void *d_summary);
int urhgpu_shard_costas_resolve_dev(urhgpu_ctx *ctx, const uint32_t *start_state, uint32_t *d_end_state);

/* ASK / FSK with the demodulated signal first: the shard's demodulation as a phase of its own, for passes that need the whole capture's
 * demodulated signal before they can slice it -- an automatic center, which the ranks detect across their shards between this phase and the
 * runs phase (urh_amd/sharding.py, iq_to_bits_auto).  The shard is demodulated ONCE; the runs phase then segments out->qad.
 *   urhgpu_shard_demod_dev: arguments as urhgpu_shard_launch_dev (d_left_halo: the two raw samples before the shard, NULL on rank 0), and
 *       out->qad is required, n_total > 2, pos_base >= 1 on ranks > 0.  URHGPU_ERR_UNSUPPORTED for every modulation but ASK and FSK (PSK has
 *       its Costas phases) and on a pipelined context (the caller reads gathered values on the host between the phases).  Writes rows
 *       [pos_base, pos_base + n_local) of afp_demod(whole capture) into out->qad on the context's stream: global sample 0 gets the
 *       modulation's NOISE constant (on rank 0 only), a rank > 0 computes its first FSK value from the halo's last sample, the gate is
 *       p->noise_threshold.  On ranks > 0 it also computes the SEAM VALUE, afp_demod's value of global sample pos_base - 1 -- demod_one(halo[0],
 *       halo[1]) with the gate on halo[1]; the NOISE constant where pos_base == 1 -- into a device float the context's shard session owns:
 *       this is why the halo has two samples, and it is the left halo of the segmentation, so that the ranks do not exchange their last
 *       demodulated values.  The session records that the shard's qad is resolved, and for which d_iq, n_local, out->qad, modulation, sample
 *       type and noise threshold.
 *   urhgpu_shard_runs_dev, called next with exactly these (p->center may differ: the detected one; d_left_halo as given here, it is not
 *       read): segments out->qad -- the qad-input kernels of a PSK pass, the session's seam value as the left halo -- instead of running
 *       the fused hot kernel; ASK keeps its generic tail and the merge exchange, FSK the tile tail; the later phases are unchanged.  The
 *       record is taken by that call and dropped by urhgpu_shard_prelaunch_dev, urhgpu_shard_launch_dev and urhgpu_shard_costas_spec_dev;
 *       without it, or with other buffers or another gate, urhgpu_shard_runs_dev behaves as it always did.
 *   urhgpu_shard_seam_value: the seam value of the context's last urhgpu_shard_demod_dev on a rank > 0, read back to *seam (HOST); waits
 *       for the context's stream.  For tests and diagnostics: no pass needs it on the host. */
int urhgpu_shard_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, int rank, int world,
                           const void *d_left_halo, const urhgpu_params *p, const urhgpu_outputs *out);
int urhgpu_shard_seam_value(urhgpu_ctx *ctx, float *seam);

/* Magnitude chunk statistics for AutoInterpretation.detect_noise_level
 * (src/urh/ainterpretation/AutoInterpretation.py:60-91): chunks of `chunk` samples taken from the END
 * of the capture backwards; d_sum[k] (float64) / d_max[k] (float64) for chunk k counted from the end. */
int urhgpu_magnitude_chunk_stats_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, int64_t chunk,
                                     int64_t n_chunks, double *d_sum, double *d_max);

/* ---- estimator passes: the O(N) parts of AutoInterpretation.estimate (src/urh/ainterpretation/AutoInterpretation.py:373-470);
 * the decisions on the few hundred resulting values stay on the host (urh_amd/estimators.py). ------------------------- */

/* auto_interpretation.segment_messages_from_magnitudes (src/urh/cythonext/auto_interpretation.pyx:55-111) as a pulse table:
 * state 1 = |sample| > noise_threshold, 0 = below, switched after 10 consecutive samples (tolerance 9), row layout and
 * length conventions of urhgpu_grab_pulse_lens_dev; the state machine starts in the state of sample 0.  The host turns
 * the rows into (start, end) tuples.  Integer captures: magnitudes as util.get_magnitudes computes them (C int sum, double sqrt). */
int urhgpu_segment_runs_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold,
                            int64_t *d_rows, int64_t cap_rows, int64_t *d_n_rows);
/* segment_messages_from_magnitudes (auto_interpretation.pyx:55-111) and -- when n_merged_out is not NULL --
 * merge_message_segments_for_ook (AutoInterpretation.py:107-148) entirely on the device: state table (urhgpu_segment_runs_dev),
 * prefix sum -> (start, end) of every segment, outlier-free minimum pulse length, cuts at pauses >= 8 x that.  Only ranges cross
 * PCIe: seg_out = HOST int64[cap_seg_out][2] receives the first min(*n_seg_out, cap_seg_out) segments (AutoInterpretation.estimate
 * looks at the first 100 to tell the modulation), merged_out likewise the merged messages.  *merge_ambiguous = 1: a pulse length
 * lies within 1e-9 of the outlier bound mean +- std, where the order of the floating-point sum of squares decides -- the caller
 * then fetches every segment and takes that decision in numpy's order.  Synchronous. */
int urhgpu_message_ranges_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold, int64_t *seg_out, int64_t cap_seg_out,
                              int64_t *n_seg_out, int64_t *merged_out, int64_t cap_merged_out, int64_t *n_merged_out, int *merge_ambiguous);
/* The same pass that also leaves afp_demod(iq, noise_threshold, "ASK") (signal_functions.pyx:343-378) in d_qad_ask (DEVICE float[n]):
 * AutoInterpretation.estimate segments by the noise threshold and then demodulates with it (AutoInterpretation.py:386-404) -- for
 * an OOK / ASK capture both read the same samples, so one pass over them serves both (8 B read + 4 B written per sample instead of
 * 8 + 8 + 4).  float32 / complex64 captures only (URHGPU_ERR_UNSUPPORTED otherwise, and for a NaN threshold). */
int urhgpu_message_ranges_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, float noise_threshold, int64_t *seg_out,
                                    int64_t cap_seg_out, int64_t *n_seg_out, int64_t *merged_out, int64_t cap_merged_out,
                                    int64_t *n_merged_out, int *merge_ambiguous, float *d_qad_ask);
/* rect[rect > thr] (AutoInterpretation.py:227), order preserved; *d_count (device) = number kept. */
int urhgpu_compact_gt_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float thr, float *d_out, int64_t *d_count);
/* positions i >= 1 where (x[i] <= center) != (x[i-1] <= center), ascending (get_plateau_lengths,
 * auto_interpretation.pyx:179-208); at most cap are stored, *d_count (device) = number found. */
int urhgpu_edges_le_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float center, int64_t *d_idx, int64_t cap, int64_t *d_count);
/* util.minmax (util.pyx:20-36) of a float32 array: d_out2 = {min, max}. */
int urhgpu_minmax_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, float *d_out2);
/* numpy's pairwise float32 sum (what np.mean / np.var reduce with): mode 0 sum x[i], mode 1 sum (x[i] - mean)^2.
 * Synchronous; *sum_out is a HOST float. */
int urhgpu_pairwise_sum_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int mode, float mean, float *sum_out);
/* np.histogram(x, bins=edges) for ascending float64 edges: d_counts[n_edges - 1]. */
int urhgpu_histogram_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, const double *d_edges, int64_t n_edges, int64_t *d_counts);

/* AutoInterpretation.estimate's per-message statistics for ALL messages of a capture in one go (AutoInterpretation.py:392-446 walks
 * them one by one: detect_center :226-277 and get_plateau_lengths, auto_interpretation.pyx:179-208).  d_x: the demodulated signal
 * (device, float32[n]); ranges: HOST int64[n_msgs][2] = (start, end) of every message.  Synchronous; host outputs.
 *
 * urhgpu_msg_center_stats: per message rect = x[start:end][x > -4] trimmed to [int(0.05 k), int(0.95 k)), then
 * out_stats[m] = {kept k, trimmed length, min, max, float32 mean, float32 np.var (the bin width), n_edges, first edge} and
 * out_hist[m][0 .. n_edges - 2] = np.histogram(rect, bins = np.arange(min, max + var, var)); n_edges == 0: no histogram (empty
 * message, zero or NaN variance, fewer than two edges -> detect_center returns None); n_edges - 1 > max_bins: the histogram does not
 * fit the pool (the caller takes that message through urhgpu_histogram_f32_dev).  out_stats: double[n_msgs][8], out_hist:
 * int64[n_msgs][max_bins] or NULL (the histograms stay on the device).
 * The peak picking (AutoInterpretation.py:250-277) happens on the device too: out_flag[m] = 1: out_center[m] is detect_center's
 * result; 0: None; 2: too many bins (see above); 3: the second and third most populated peaks hold the same count, so the result
 * depends on how np.argsort orders equal keys -- the caller asks again with out_hist, for THOSE messages only, and lets numpy decide.
 * Both may be NULL.  ranges must be ascending and disjoint (start[m] >= end[m - 1]; URHGPU_ERR_ARG otherwise): per-message scratch
 * lives at [start, end) of capture-sized arrays.  The histogram pool is bounded: messages are processed in batches of at most
 * 64 MiB / (4 max_bins) (16 384 at max_bins = 4096), whatever n_msgs is. */
int urhgpu_msg_center_stats(urhgpu_ctx *ctx, const float *d_x, int64_t n, const int64_t *ranges, int n_msgs, int64_t max_bins,
                            double *out_stats, int64_t *out_hist, double *out_center, int32_t *out_flag);
/* urhgpu_msg_plateaus: get_plateau_lengths(x[start:end], centers[m], percentage) for every message with a center (NaN: none,
 * no plateaus): out_len[out_off[m] .. |out_off[m + 1]|) (uint64, back to back; out_off[0] = 0).  Boundaries are searched in the
 * first percentage % + extra_window samples of a message; when that window holds no boundary at or beyond the percentage mark the
 * message's end offset comes back as -(end + 1) and the caller repeats it with a larger window.  More than cap_total lengths:
 * URHGPU_ERR_CAPACITY with the needed total in out_off[n_msgs].  Messages longer than 2^31 - 1 samples: URHGPU_ERR_UNSUPPORTED. */
int urhgpu_msg_plateaus(urhgpu_ctx *ctx, const float *d_x, int64_t n, const int64_t *ranges, const double *centers, int n_msgs,
                        int percentage, int64_t extra_window, int64_t *out_off, uint64_t *out_len, int64_t cap_total);

/* auto_interpretation.merge_plateaus (auto_interpretation.pyx:145-176): host arrays, host arithmetic (sequential, a few thousand
 * values); out needs room for n values, *n_out = number of merged plateaus. */
int urhgpu_merge_plateaus(const uint64_t *plateaus, int64_t n, uint64_t tolerance, uint64_t max_count, uint64_t *out, int64_t *n_out);

/* AutoInterpretation.detect_modulation (AutoInterpretation.py:150-205; Wavelet.cwt_haar, Wavelet.py:15-43; median_filter,
 * auto_interpretation.pyx:213-240) for n_msgs messages of a complex64 capture on the device (d_iq: float32 pairs; ranges: HOST
 * int64[n_msgs][2]): labels_out[m] = 0 none, 1 OOK, 2 ASK, 3 FSK, 4 PSK; vars_out (or NULL): double[n_msgs][4] = the variances of
 * |CWT|, |CWT of the unit-magnitude samples| and of both after the median filter (NaN when the decision fell before them).
 * Floating-point classifier (double-precision radix-2 FFTs here, single-precision pocketfft forward transforms in the
 * reference): the label is the parity criterion.  wavelet_scale 4 and median_filter_order 11 are the reference's defaults.
 * Synchronous. */
int urhgpu_detect_modulation_dev(urhgpu_ctx *ctx, const float *d_iq, int64_t n, const int64_t *ranges, int n_msgs, int wavelet_scale,
                                 int median_filter_order, int *labels_out, double *vars_out);

/* The per-message decisions of AutoInterpretation.estimate after get_plateau_lengths (AutoInterpretation.py:416-433; tolerance :280-298,
 * merge_plateaus, round_plateau_lengths :313-326, divisor histogram, bit length :344-370) for every message in one call, host
 * arithmetic on the lengths urhgpu_msg_plateaus returned (same `off` convention).  tol_out[m]: tolerance or -1 (None);
 * bitlen_out[m]: bit length, -1 (fewer than two merged plateaus: no vote) or -2 (the reference's result depends on numpy's order of
 * equal counts: decide that message with numpy). */
int urhgpu_msg_bit_lengths(const uint64_t *lens, const int64_t *off, int n_msgs, int64_t *tol_out, int64_t *bitlen_out);
/* urhgpu_msg_plateaus and urhgpu_msg_bit_lengths in one call: the plateau lengths stay on the GPU, which counts every message's
 * distinct lengths (a few dozen per message against thousands of plateaus); the decisions that depend on the multiset only -- all of
 * them for a message without glitches (tolerance 0) -- are taken from those (value, count) pairs, and only messages with a positive
 * tolerance (merge_plateaus walks the sequence, auto_interpretation.pyx:145-176) have their sequences fetched.  Arguments as
 * urhgpu_msg_plateaus, results as urhgpu_msg_bit_lengths; tol_out[m] = bitlen_out[m] = -3: the search window of message m did not reach
 * the percentage mark (repeat that message through urhgpu_msg_plateaus with a larger window).  Synchronous. */
int urhgpu_msg_plateau_decisions(urhgpu_ctx *ctx, const float *d_x, int64_t n, const int64_t *ranges, const double *centers, int n_msgs,
                                 int percentage, int64_t extra_window, int64_t *tol_out, int64_t *bitlen_out);
/* urhgpu_msg_center_stats followed by urhgpu_msg_plateau_decisions with the centers it picked, in ONE call: the centers never leave the
 * device, the scratch of both stages is one reservation, one synchronisation ends the call (AutoInterpretation.py:397-433 per message).
 * out_stats[8 * n_msgs], out_center, out_flag as urhgpu_msg_center_stats gives them; tol_out / bitlen_out as urhgpu_msg_plateau_decisions,
 * -4 for a message whose center needs the host first (out_flag 2 or 3: settle it, then urhgpu_msg_plateau_decisions for that message).
 * URHGPU_ERR_UNSUPPORTED: n_msgs * max_bins counters do not fit one batch of the histogram pool (take the two calls). */
int urhgpu_msg_estimate(urhgpu_ctx *ctx, const float *d_x, int64_t n, const int64_t *ranges, int n_msgs, int64_t max_bins, int percentage,
                        int64_t extra_window, double *out_stats, double *out_center, int32_t *out_flag, int64_t *tol_out, int64_t *bitlen_out);
/* Test hook (host arithmetic): the multiset form of one message's decision; -3 in both where the sequence would be asked for. */
int urhgpu_test_bit_length_from_counts(const uint64_t *lens, int64_t n, int64_t *tol_out, int64_t *bitlen_out);
/* The two halves around np.argsort for a message urhgpu_msg_bit_lengths reported as -2 (equal counts in the divisor histogram: the
 * reference's result is whatever order np.argsort gives equal keys).  urhgpu_msg_divisor_histogram: tolerance, merged and rounded
 * plateaus (AutoInterpretation.py:280-326), then the dense uint64 histogram the reference sorts (auto_interpretation.pyx:113-143):
 * *hist_len = max value + 1 (cap = 0 only asks for it), -1 = fewer than two merged plateaus.  urhgpu_bit_length_from_order: the
 * selection loop of get_bit_length_from_plateau_lengths (AutoInterpretation.py:358-370) over order_desc = np.argsort(hist)[::-1]. */
int urhgpu_msg_divisor_histogram(const uint64_t *lens, int64_t n, uint64_t *hist_out, int64_t cap, int64_t *hist_len, int64_t *tol_out);
int urhgpu_bit_length_from_order(const uint64_t *hist, const int64_t *order_desc, int64_t len, int64_t *bitlen_out);

/* ---- host-array forms of the reference's remaining `util` / `auto_interpretation` functions on the path (the signatures
 * AutoInterpretation.py:8-10 imports by name; urh_amd/util.py and urh_amd/auto_interpretation.py bind them) --------------------- */
/* util.minmax (src/urh/cythonext/util.pyx:20-36): arr = n values of dtype (the fused `iq` element types); out2 = {min, max} in the
 * same type; n == 0: {0, 0}.  The reference's comparisons (a NaN never replaces min / max unless it is element 0). */
int urhgpu_minmax(urhgpu_ctx *ctx, const void *arr, int dtype, int64_t n, void *out2);
/* auto_interpretation.segment_messages_from_magnitudes (src/urh/cythonext/auto_interpretation.pyx:55-111) on caller-supplied
 * magnitudes (float32, or float64 as util.get_magnitudes returns them: is_f64): seg_out = int64[cap_seg][2] (start, end) tuples,
 * *n_seg their number (also on URHGPU_ERR_CAPACITY).  At most n / 20 + 3 segments exist. */
int urhgpu_segment_messages(urhgpu_ctx *ctx, const void *magnitudes, int is_f64, int64_t n, float noise_threshold, int64_t *seg_out,
                            int64_t cap_seg, int64_t *n_seg);
/* auto_interpretation.get_plateau_lengths (auto_interpretation.pyx:179-208): rect_data float32[n] (host) -> out uint64[cap], *n_out
 * lengths (also on URHGPU_ERR_CAPACITY). */
int urhgpu_get_plateau_lengths(urhgpu_ctx *ctx, const float *rect_data, int64_t n, float center, int percentage, uint64_t *out, int64_t cap,
                               int64_t *n_out);
/* auto_interpretation.get_threshold_divisor_histogram (auto_interpretation.pyx:113-143): dense uint64[max(lens) + 1]; cap = 0 only
 * asks for *hist_len.  Host arithmetic (sorting the multiset of values instead of the reference's P^2 / 2 pair loop). */
int urhgpu_threshold_divisor_histogram(const uint64_t *lens, int64_t n, float threshold, uint64_t *hist_out, int64_t cap, int64_t *hist_len);
/* auto_interpretation.median_filter (auto_interpretation.pyx:227-240): out[i] = sorted(float(data[i : min(i + k, n)]))[k' / 2];
 * k <= 64 (URHGPU_ERR_UNSUPPORTED beyond; the reference's callers use 3 .. 11). */
int urhgpu_median_filter(urhgpu_ctx *ctx, const double *data, int64_t n, unsigned int k, float *out);

/* Test hook: the hot kernel's fast-path division (Newton + residual chain without scaling) against the IEEE
 * division on 2^20 * reps pseudo-random operand pairs from the range the fast path accepts; *n_mismatch must be 0. */
int urhgpu_test_fast_division_dev(urhgpu_ctx *ctx, uint64_t seed, int reps, uint64_t *n_mismatch);
/* Test hook: the branch-free sinf / cosf pair of the Costas loop (glibc_sincosf.h: urh_sincosf_fast) against the branchy restatement
 * of glibc's sinf and cosf for EVERY float with |y| < 120; *n_mismatch = arguments where either result differs in a bit. */
int urhgpu_test_sincosf_fast_dev(urhgpu_ctx *ctx, uint64_t *n_mismatch);
/* Test hook: urhgpu_message_ranges_dev reports every OOK merge as borderline (*merge_ambiguous = 1), so that the caller's numpy
 * route for that case can be exercised; returns the previous setting. */
int urhgpu_test_force_merge_ambiguous(int on);

/* signal_functions.modulate_c (signal_functions.pyx:56-177) for ASK / FSK / PSK / OQPSK (URHGPU_MOD_OQPSK: bits_per_symbol must be 2; GFSK: urhgpu_modulate_gfsk*),
 * n_msgs messages rendered back to back by one launch (URH modulates message by message, Modulator.py:215-255):
 * message m has bits[bit_off[m] .. bit_off[m+1]), is followed by pause[m] zero samples and starts at sample index start[m]
 * (the time origin of its carrier).  parameters: 2^bits_per_symbol amplitudes / frequencies / phases as the reference takes
 * them.  dtype: URHGPU_DT_F32 / _I8 / _I16 (get_numpy_dtype, :46-54; anything else URHGPU_ERR_DTYPE).  All pointers are HOST
 * pointers except d_out (device, (cap_samples, 2) of dtype); *total_samples = sum over m of
 * (n_bits_m / bits_per_symbol) * samples_per_symbol + pause[m]; more than cap_samples: URHGPU_ERR_CAPACITY, nothing written.
 * Asynchronous on the context's stream. */
int urhgpu_modulate_dev(urhgpu_ctx *ctx, const uint8_t *bits, const int64_t *bit_off, const uint32_t *pause, const uint32_t *start,
                        int n_msgs, uint32_t samples_per_symbol, int mod, const float *parameters, int bits_per_symbol,
                        float carrier_amplitude, float carrier_frequency, float carrier_phase, float sample_rate, int dtype,
                        void *d_out, int64_t cap_samples, int64_t *total_samples);
/* One message, host output: exactly modulate_c's signature; out holds ((num_bits / bits_per_symbol) * samples_per_symbol + pause, 2). */
int urhgpu_modulate(urhgpu_ctx *ctx, const uint8_t *bits, int64_t num_bits, uint32_t samples_per_symbol, int mod,
                    const float *parameters, int bits_per_symbol, float carrier_amplitude, float carrier_frequency,
                    float carrier_phase, float sample_rate, uint32_t pause, uint32_t start, int dtype, void *out);

/* modulate_c(..., "GFSK", ...) (signal_functions.pyx:118-125, 156-163, 196-228).  gauss_fir: the n_taps Gaussian taps of
 * gauss_fir (:230-243), which the reference computes with numpy (host; urh_amd.signal_functions.gauss_fir restates it).
 * The per-sample symbol frequencies are convolved with the taps ("same" mode), every output an exactly accumulated dot product
 * rounded once to float32; the reference takes this value from numpy's float32 BLAS dot product, whose summation order (and last
 * bit) depends on the host CPU.  frequencies (HOST, optional): the filtered frequencies, one float per data sample of every
 * message back to back (e.g. numpy's convolution, for the reference's bits on this host) -- used instead of the device
 * convolution.  The phase recurrence (:219-226, numpy's float32 arange restated) and the carrier are evaluated exactly as
 * the reference does.  A message with fewer bits than one symbol: URHGPU_ERR_ARG (ZeroDivisionError in the reference, :201). */
int urhgpu_modulate_gfsk_dev(urhgpu_ctx *ctx, const uint8_t *bits, const int64_t *bit_off, const uint32_t *pause, const uint32_t *start,
                             int n_msgs, uint32_t samples_per_symbol, const float *parameters, int bits_per_symbol,
                             float carrier_amplitude, float carrier_phase, float sample_rate, int dtype, const float *gauss_fir,
                             int n_taps, const float *frequencies, void *d_out, int64_t cap_samples, int64_t *total_samples);
int urhgpu_modulate_gfsk(urhgpu_ctx *ctx, const uint8_t *bits, int64_t num_bits, uint32_t samples_per_symbol, const float *parameters,
                         int bits_per_symbol, float carrier_amplitude, float carrier_phase, float sample_rate, uint32_t pause,
                         uint32_t start, int dtype, const float *gauss_fir, int n_taps, const float *frequencies, void *out);

/* IQArray.convert_to (IQArray.py:127-203) on device memory: n VALUES (two per IQ sample) of src_dtype -> dst_dtype, any
 * pair of different URHGPU_DT_* codes, with the reference's wrapping / truncating numpy semantics.  Asynchronous. */
int urhgpu_convert_dev(urhgpu_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, int64_t n);
/* Signal.__load_wav_file (Signal.py:114-173) on device memory: the PCM frames of a WAV file (d_raw: n_frames * channels * sample_width
 * bytes as wave.readframes returns them; sample_width 1: unsigned bytes, 2 / 3 / 4: signed little endian) -> float32 IQ d_out[n_frames][2]:
 * (sample - center) * (1 / max) in float64, rounded once to float32, as numpy evaluates the reference's expression; one channel: the
 * imaginary part is 0 (an already demodulated capture, :155-156), two: left -> real, right -> imag.  Also what a Flipper .sub capture goes
 * through once its run lengths are expanded to bytes 255 / 0 (:175-205).  Other channel counts / widths: URHGPU_ERR_ARG (the reference
 * raises ValueError, :133, :164).  Asynchronous. */
int urhgpu_pcm_to_iq_dev(urhgpu_ctx *ctx, const void *d_raw, int64_t n_frames, int channels, int sample_width, float *d_out);
/* The run lengths IQArray.export_to_sub writes (IQArray.py:275-304) from the uint8 conversion of a capture: values[i * stride] is sample
 * i's first component (HOST memory; stride 2 for an (N, 2) array).  runs_out[k] > 0: that many samples above 127, < 0: at or below; the
 * reference's walk is restated exactly (a run of ONE sample never ends: the samples that differ from it are dropped until its value
 * comes back).  *n_runs is set also on URHGPU_ERR_CAPACITY.  Host arithmetic; works without a GPU. */
/* Signal.estimate_frequency's core (Signal.py:578-601): the bin k of the largest |FFT| of n = 2^m complex64 samples (d_x: float32[n][2] on the
 * device), the smallest such k -- what np.argmax(np.abs(np.fft.fft(data))) returns whenever the peak stands out by more than float32 rounding
 * (single-precision butterflies like numpy's complex64 transform, twiddles rounded from float64).  n up to 2^26 (URHGPU_ERR_UNSUPPORTED
 * beyond; n not a power of two: URHGPU_ERR_ARG).  Synchronous: *peak_index is a host value. */
int urhgpu_fft_peak_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int64_t *peak_index);
int urhgpu_sub_encode_runs(const uint8_t *values, int64_t n, int64_t stride, int64_t *runs_out, int64_t cap, int64_t *n_runs);
/* The plain numpy cast between float32 and one of the four integer sample types (no IQArray scaling): what Filter.apply_fir_filter
 * does to an integer capture before filtering (`tmp.real = input_signal[0::2]`, Filter.py:37-41: the raw values as float32) and what
 * IQArray.__setitem__ does with the filtered complex64 range (`self.real[key] = value.real`, IQArray.py:31-33: truncation toward zero
 * through int32, low bits kept).  Exactly one of the two dtypes is URHGPU_DT_F32.  Asynchronous. */
int urhgpu_astype_dev(urhgpu_ctx *ctx, const void *d_src, int src_dtype, void *d_dst, int dst_dtype, int64_t n);

/* path_creator.create_path's pass over the samples (path_creator.pyx:46-66): 1-D samples of dtype (the five IQ sample
 * types), stretches of samples_per_pixel samples from `start` (the last one ends at `end`); values[2k] / values[2k+1] =
 * minimum / maximum of stretch k exactly as the reference's sequential scan finds them (NaN and signed-zero behaviour
 * included).  values holds 2 * ceil((end - start) / samples_per_pixel) elements of dtype.  _dev: device pointers,
 * asynchronous; the host form takes the whole array (n samples) and returns when values is filled. */
int urhgpu_path_minmax_dev(urhgpu_ctx *ctx, const void *d_samples, int dtype, int64_t start, int64_t end,
                           int64_t samples_per_pixel, void *d_values);
int urhgpu_path_minmax(urhgpu_ctx *ctx, const void *samples, int dtype, int64_t n, int64_t start, int64_t end,
                       int64_t samples_per_pixel, void *values);

/* Spectrogram.stft + __calculate_spectrogram (Spectrogram.py:94-116, :158-164; util.arr2decibel, util.pyx:38-48) on device
 * memory: d_x complex64[n]; frames = max(1, (n - window_size) / hop + 1) frames of window_size samples (a power of two,
 * 8 .. 4096; samples at or beyond n read as zero: the reference's zero padding of captures shorter than one window),
 * d_window float64[window_size] (np.hanning by default), d_twiddles complex128[window_size / 2] = exp(-2 pi i m / window_size).
 * Exactly one output: d_stft complex128[frames * window_size] (the stft, divided by window_size) or d_db float32[frames *
 * window_size] (fftshift along frequency, complex64, 10 log10 |.|^2, fliplr).  Double-precision FFT like numpy's; floating
 * point, not bit-exact.  Asynchronous. */
int urhgpu_spectrogram_dev(urhgpu_ctx *ctx, const float *d_x, int64_t n, int window_size, int64_t hop, int64_t frames,
                           const double *d_window, const double *d_twiddles, double *d_stft, float *d_db);
/* Spectrogram.apply_bgra_lookup (Spectrogram.py:196-210, normalize=True): d_db float32 (frames, window_size) ->
 * d_image uint32 BGRA (window_size, frames) through d_colormap[n_colors]. */
int urhgpu_bgra_lookup_dev(urhgpu_ctx *ctx, const float *d_db, int64_t frames, int window_size, const uint32_t *d_colormap,
                           int n_colors, float data_min, float data_max, uint32_t *d_image);

/* Measurement hook (bench.py, SURVEY.md 8(d) "also measure an on-box copy-kernel ceiling and report both denominators"): a PURE COPY
 * on this GPU, timed with events over `reps` launches.  shape 0: the hot kernel's access structure without its arithmetic (one
 * workgroup of four wavefronts per 8192 samples, 16-byte non-temporal loads two rows ahead, 8-byte non-temporal stores: 8 B in + 4 B
 * out per sample, d_in float32[2 n], d_out float32[n]); shape 1: a plain grid-stride float4 copy of n float32 values (4 B in + 4 B
 * out per value); shape 2: shape 0 on the CU-masked stream the hot kernel of pipelined passes runs on (URHGPU_ERR_UNSUPPORTED on a context
 * without one).  n_samples a multiple of 8192.  Synchronous. */
int urhgpu_bench_copy_ceiling_dev(urhgpu_ctx *ctx, const float *d_in, float *d_out, int64_t n_samples, int shape, int reps, float *ms_per_copy);
/* Measurement hook (tools/boundary_probe.py -> profiles/r05_boundary_anatomy.txt): `launches` back-to-back launches of the hot kernel alone
 * (complex64 2-FSK, n a multiple of 2048, qad written, no tail) on the context's stream (stream_kind 0) or its CU-masked hot stream (1; a
 * pipelined context).  event_mode 0: plain launches; 1: a completion event attached to every dispatch as pipelined passes do; 2: the same
 * with hipEventDisableSystemFence | hipEventReleaseToDevice; 3: timing events on every dispatch (dur_ms[launches], gap_ms[launches - 1]:
 * the dispatches' own durations and the time from one's end to the next one's begin).  graded: that many of the launch's last chunks are
 * cut into four short ones each.  Wavefront 0 of every workgroup leaves three s_memrealtime stamps (10 ns units, low 32 bits: entry,
 * streaming phase over, ChunkInfo written) and its hardware ids in the ChunkInfo's first_acc / pend_stable / pad / pend_acc fields; the
 * tables of the last `keep` launches are copied to d_chunks_out (keep * *n_chunks_out * URHGPU_SHARD_SUMMARY_BYTES bytes).  Synchronous. */
int urhgpu_test_hot_probe(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, float *d_qad, int stream_kind, int event_mode,
                          int graded, int launches, int keep, void *d_chunks_out, int64_t *n_chunks_out, float *dur_ms, float *gap_ms, int bubble_us,
                          int load_kind);
/* ... bubble_us > 0: a one-wavefront kernel that idles for that long between two hot kernels; load_kind != 0 (event_mode 1 or 2): synthetic
 * company on a second stream beside every hot kernel (probes.hip: arithmetic / random loads on the CUs the hot mask leaves out, thousands of
 * short high-priority workgroups, six empty kernels).  The same stamps inside the PRODUCT's passes
 * (tools/inrun_anatomy.py): urhgpu_test_hot_stamps(1) makes every complex64 2-FSK pass run the stamped instantiation (process-wide; the
 * stamps sit in ChunkInfo fields the tile tail does not read), urhgpu_test_fetch_chunk_tables copies the chunk tables of the context's three
 * most recent pipelined passes (newest first, n_chunks x URHGPU_SHARD_SUMMARY_BYTES bytes each) to host_dst.  Synchronous. */
int urhgpu_test_hot_stamps(int on);
/* Measurement hook: leave kernels of the tile tail out (bit 0 k_resolve_one, 1 k_emit_rows_tiles, 2 k_tile_scan, 3 group scan, 4
 * k_expand_tiles, 5 k_pack_seg) to see what each costs the hot kernel it runs beside; outputs are only meaningful while every pass
 * processes the same capture (the buffers then hold the previous pass's identical results).  Round 6: bit 6 the row kernel without its stores
 * into the (host or staging) blob, 7 without the int64 table, 9 a staged pass without its copies, 11 the expansion without its byte stores.
 * Process-wide; 0 restores the product. */
int urhgpu_test_tail_skip(int mask);
int urhgpu_test_fetch_chunk_tables(urhgpu_ctx *ctx, void *host_dst, int64_t n_chunks);
/* Synchronous device -> host copy after urhgpu_ctx_sync (for callers that hold raw device pointers, e.g. urhgpu_host_result::d_qad). */
int urhgpu_memcpy_to_host(urhgpu_ctx *ctx, const void *d_src, void *host_dst, int64_t bytes);
/* ... and device -> device (a result's d_qad into memory the caller owns, before the stream's qad ring moves on). */
int urhgpu_memcpy_dtod(urhgpu_ctx *ctx, void *d_dst, const void *d_src, int64_t bytes);

/* Test hook: modulation order 2 (2-FSK, OOK, message segmentation) normally runs the bit-plane kernel
 * (k_demod_runs_bp) and every other order the state-byte kernel (k_demod_runs); on != 0 routes order 2 through the
 * state-byte kernel as well, so that tests can compare the two on the same input.  Process-wide. */
int urhgpu_test_force_state_bytes(int on);

/* Test hook: captures of every modulation but ASK (on one GPU and sharded) go from chunk records to bits through the five-launch "tile"
 * tail; on != 0 routes them through the generic tail (the one ASK captures use) so that tests can compare the two
 * on the same input.  Process-wide. */
int urhgpu_test_force_generic_tail(int on);

/* Test hook: the chunk plan normally depends on the capture size (1 tile = 16 rows of 128 samples per chunk below
 * about 8 M samples, 4 tiles = 64 rows -- every lane of the run phase populated, four wavefronts exchanging bit planes
 * through LDS -- above about 25 M).  tiles = 1..4 forces that many tiles per chunk for every size, so that small
 * captures the oracle finishes in seconds exercise the plan the 1 GiB benchmark runs; 0 restores the default.  Process-wide. */
int urhgpu_test_force_tiles_per_chunk(int tiles);

/* Test hook: hot launches of this process that took the signed-integer instantiation WITH the wide loop (capture streams by their probe,
 * one-shot and sharded passes by the tuning key "wide_int"): what a test of that instantiation checks it has exercised. */
int64_t urhgpu_test_wide_int_launches(void);

/* Test hooks of the Costas loop.  urhgpu_test_costas_host_syncs: stream synchronisations of this process made by the Costas launchers (the
 * host-driven rounds of one-shot and sharded passes; the device-driven loop makes none).  urhgpu_test_costas_scratch: out3 = {scratch bytes
 * reserved for a capture of n samples, one past the device-driven loop's control block as the buffers are carved for loop order 2 / 4, the
 * block's size}.  Host arithmetic; works without a GPU. */
int64_t urhgpu_test_costas_host_syncs(void);
/* how often code reached from the automatic-center entry points (urhgpu_detect_center_dev, urhgpu_iq_to_bits_auto_center_dev,
 * urhgpu_stream_set_auto_center, and through them the passes of such a stream) made the host wait for the device: counted in the library
 * beside every wait below those entry points -- stream, event and device synchronisations (the bounded run-ahead of pipelined passes,
 * host-driven Costas rounds), scratch that grows (hipFree waits for the device).  A pass whose scratch is in place does not move it.
 * Handing a result out and settling flag 2 / 3 on the host are not the pass: their waits belong to the calls that make them. */
int64_t urhgpu_test_center_host_syncs(void);
int urhgpu_test_costas_scratch(int64_t n, int loop_order, int64_t *out3);

/* Test hook: elementwise bit-faithful atan2f (the device port of glibc 2.35 atan2f), device pointers. */
int urhgpu_test_atan2f_dev(urhgpu_ctx *ctx, const float *d_y, const float *d_x, int64_t n, float *d_out);

/* ---- the live mode's pass over an incoming chunk (ProtocolSniffer.__demodulate_data, ProtocolSniffer.py:204-281) --------------------
 * d_src: n_rows rows of two samples of `dtype` (URHGPU_DT_*), device memory, any row offset into a larger buffer.  In one read of the chunk
 *   - its first n_store rows (n_store <= n_rows: the reference trims an append that does not fit its buffer) are stored to d_dst (device;
 *     NULL or == d_src: nothing is stored -- the chunk was uploaded to its place already; otherwise the two ranges must not overlap), and
 *   - *sum_out = np.sum(data ** 2.0) and *max_out = np.max(data ** 2.0) over the 2 * n_rows components are formed in the reference's
 *     arithmetic: float32 chunks in float32 (squares not fused into the adds, numpy's pairwise order, NaN as np.max propagates it) and
 *     widened exactly; integer chunks as exact integers, which is numpy's float64 result as long as the total stays below 2^53
 *     (beyond: URHGPU_ERR_UNSUPPORTED).  np.mean is *sum_out divided by 2 * n_rows in the chunk's float type.
 * Two launches whatever n_rows is; the results land in pinned host memory by ordinary stores; synchronous (one stream synchronisation). */
int urhgpu_chunk_power_stats_dev(urhgpu_ctx *ctx, const void *d_src, int dtype, int64_t n_rows, void *d_dst, int64_t n_store, double *sum_out,
                                 double *max_out);
/* Diagnostics: kernel launches urhgpu_chunk_power_stats_dev has issued on this context. */
int urhgpu_chunk_stats_launches(urhgpu_ctx *ctx, int64_t *n_launches);

/* ---- the estimators on one rank of a sharded capture (urh_amd/sharding.py: ShardedPipeline.detect_noise_level / detect_center) -------
 * detect_noise_level (AutoInterpretation.py:60-91): d_iq holds the samples [pos_base, pos_base + n_local) of a capture of n_total; chunk k
 * (counted from the END of the capture, as in urhgpu_magnitude_chunk_stats_dev) covers [n_total - (k + 1) chunk, n_total - k chunk).
 * d_sum[k] / d_max[k] (DEVICE double[n_chunks]) = fp64 sum / max of the magnitudes of the samples of chunk k that lie in the shard;
 * 0.0 and 0.0 where there is none; a NaN magnitude makes the chunk's max NaN.  The caller adds the ranks' sums and folds their maxima. */
int urhgpu_magnitude_chunk_partials_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n_local, int64_t pos_base, int64_t n_total,
                                        int64_t chunk, int64_t n_chunks, double *d_sum, double *d_max);
/* The part of numpy's pairwise float32 sum (urhgpu_pairwise_sum_f32_dev; csrc/pairwise.hpp has the order) that one rank can evaluate:
 * d_x holds the elements [g_off, g_off + m_local) of a float32 sequence of m_total; mode 0 sums x[i], mode 1 (x[i] - mean)^2.  d_out
 * (DEVICE float[cap], 8-byte aligned) receives the record below, *n_out (HOST, may be NULL) its length in words, which depends on (m_local,
 * g_off, m_total) alone: URHGPU_PW_REC_PIECES + the number of full pieces of 8192 elements wholly inside the range
 * (URHGPU_ERR_CAPACITY when cap is smaller).  Asynchronous on the context's stream.
 *   words [0:2) g_off, [2:4) m_local (int64); [4] min, [5] max of the rank's elements by util.minmax's comparisons (+inf / -inf when
 *         no element compares); [6] the rank's first element; [7] the number of words (int32)
 *   HEAD  the elements, mapped through `mode`, of the leaf that the START of the range cuts (also a range inside one leaf that begins
 *         before it): fewer than 128
 *   FIRST / LAST  the first / last piece the range touches without holding all of it: the sums of its leaves that lie wholly inside,
 *         the leaf whose first multiple of 64 (relative to the piece) is 64 s in slot s (leaves of a piece are 64 .. 128 elements long)
 *   TAIL  the mapped elements of the leaf that only the END of the range cuts
 *   PIECES  one sum per full piece wholly inside the range, ascending
 * Words nobody wrote are zero.  sharding.pairwise_combine finishes the sum from the ranks' records. */
#define URHGPU_PW_REC_HEAD 8
#define URHGPU_PW_REC_FIRST 136
#define URHGPU_PW_REC_LAST 264
#define URHGPU_PW_REC_TAIL 392
#define URHGPU_PW_REC_PIECES 520
int urhgpu_pairwise_partial_f32_dev(urhgpu_ctx *ctx, const float *d_x, int64_t m_local, int64_t g_off, int64_t m_total, int mode, float mean,
                                    float *d_out, int64_t cap, int64_t *n_out);

/* ---- automatic noise threshold inside a pass, decided on the device -------------------------------------------------------------
 * The reference opens a capture with default_noise_threshold = "automatic" (Signal.py:97-103): noise_threshold =
 * AutoInterpretation.detect_noise_level(magnitudes), and demodulates with it.  These entry points run detect_noise_level
 * (AutoInterpretation.py:60-91) as a chain that is queued and never waited for: the per-chunk (sum, max) of the magnitudes
 * (urhgpu_magnitude_chunk_stats_dev's kernels; chunks of max(1, n / 100) samples counted from the END of the capture, at most 199 of
 * them) and ONE workgroup that decides (k_noise_decide) in the reference's scalar types: float32 means of fp64 sums, minimum / maximum
 * as doubles (util.minmax hands Python floats back), the float32 product 1.1f * min for the candidates, the fp64 maximum of the
 * candidates' maxima, ceil(result * 10000) / 10000 in fp64.  The chain's scratch is a fixed part of the context from its creation: it
 * never grows.  The kernels that gate by magnitude load noise_sqrd from the result block (a uniform load per workgroup).
 *   flag 1  noise = detect_noise_level's value (this includes the 0 it returns for n <= 3, for means that lie close together and for an
 *           all-zero capture)
 *   flag 2  noise is the value, but it is not below Signal.max_magnitude of the sample type (urhgpu_noise_max_magnitude; a comparison of
 *           doubles, Signal.py:404-406): the reference then does not demodulate at all (Signal.py:474-484: np.zeros(2))
 *   flag 0  the reference raises: math.ceil of a NaN (ValueError) or of an infinity (OverflowError); noise holds that NaN / infinity
 * WITH FLAG 0 OR 2 A QUEUED PASS GATED WITH p->noise_threshold: its outputs are those of the pass without auto_noise. */
typedef struct urhgpu_noise_result {
    double noise;                /* flag 1, 2: detect_noise_level's value; flag 0: the NaN / infinity math.ceil would have been given */
    float noise_f32;             /* the threshold the pass gated with as afp_demod's `float noise_mag` argument: (float)noise for flag 1 (and for
                                  * every flag of urhgpu_detect_noise_level_dev, which has no pass), p->noise_threshold for flag 0 / 2 */
    float noise_sqrd;            /* noise_f32 * noise_f32, an fp32 multiply: what the kernels compare |sample|^2 with */
    int64_t flag;
    int64_t chunk, n_chunks;     /* the chunk geometry: samples per chunk, chunks (0 for n <= 3) */
    int64_t n_candidates;        /* chunks with mean <= 1.1f * min */
    double min_mean, max_mean;   /* of the float32 chunk means, as doubles */
} urhgpu_noise_result;
/* Signal.max_magnitude of a sample type (Signal.py:404-406): (2 * max(min^2, max^2)) ** 0.5 with IQArray.min_max_for_dtype's bounds
 * (-1, 1 for float32).  Host arithmetic; 0 for an unknown dtype. */
double urhgpu_noise_max_magnitude(int dtype);
/* The chain alone on d_iq (device, n samples of dtype): d_result (device, sizeof(urhgpu_noise_result), 8-byte aligned) is complete when the
 * work queued so far on the context's stream is.  Asynchronous: no read-back, no wait. */
int urhgpu_detect_noise_level_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t n, void *d_result);
/* IQ -> bits with the noise threshold (auto_noise) and / or the center (auto_center) detected inside the pass.
 *   auto_noise alone   the chain, then the FUSED pass of urhgpu_iq_to_bits_dev with the hot kernel reading the threshold from
 *                      d_noise_result, then the ordinary tail; out->qad is optional.  PSK: the Costas kernels read it.
 *   with auto_center   the shape of urhgpu_iq_to_bits_auto_center_dev (out->qad required: URHGPU_ERR_ARG without), k_afp_demod or the
 *                      Costas loop reading the device threshold; the center chain and the slicing are that entry point's.
 *   auto_noise = 0     exactly urhgpu_iq_to_bits_auto_center_dev (auto_center != 0) or urhgpu_iq_to_bits_dev (both 0).
 * d_noise_result (auto_noise: required, device, 8-byte aligned) / d_center_result + hist_cap (auto_center: as urhgpu_iq_to_bits_auto_center_dev).
 * h_noise_result / h_center_result: optional pinned host mirrors, written by kernels of the pass and valid once the pass is over, as
 * out->h_counts is.  The pass never waits for the device and reads nothing back (PSK on a context that is not pipelined keeps the
 * host-driven Costas rounds unless "costas_dev_rounds" says otherwise). */
int urhgpu_iq_to_bits_auto_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, int auto_noise, int auto_center,
                               int64_t center_max_size, const urhgpu_outputs *out, void *d_noise_result, void *h_noise_result,
                               void *d_center_result, void *h_center_result, int64_t hist_cap);
/* Every pass of the stream detects its own noise threshold (urhgpu_iq_to_bits_auto_dev).  Before the first push (URHGPU_ERR_ARG after).
 * Such passes take the ordinary route (tail behind the hot kernel, pack + copy behind the tail); urhgpu_stream_push_upload makes ONE copy
 * in front of the pass: the chunks count from the END of the capture, so nothing can be gated before all of it has landed.  May be
 * combined with urhgpu_stream_set_auto_center. */
int urhgpu_stream_set_auto_noise(urhgpu_stream *st, int enable);
/* The threshold of a pass whose result has been handed out (by a push's `ready` or by urhgpu_stream_flush), valid as long as that result. */
int urhgpu_stream_noise(urhgpu_stream *st, int64_t seq, double *noise, int64_t *flag);
/* how often code reached from the automatic-noise entry points (urhgpu_detect_noise_level_dev, urhgpu_iq_to_bits_auto_dev with auto_noise,
 * and through it the passes of such a stream) made the host wait for the device: the counter of urhgpu_test_center_host_syncs, kept
 * separately for these entry points. */
int64_t urhgpu_test_noise_host_syncs(void);

/* ---- message records inside a pass: RSSI, first position and ASK padding ----------------------------------------------------------
 * ProtocolAnalyzer.get_protocol_from_signal (ProtocolAnalyzer.py:227-321) ends with a step per message: ASK messages borrow zero bits
 * from the pause that follows them until their length is a multiple of message_length_divisor (:256-263, :303-321), the RSSI is the mean
 * of magnitudes_normalized over one symbol at the middle bit (:267-269), the timestamp comes from the first bit's position (:270-272).
 * These entry points queue that step behind a pass, while the capture is still in device memory: one record per message.
 *   padding   only for URHGPU_MOD_ASK and message_length_divisor > 1.  L = bits of the message, missing = (divisor - L % divisor) % divisor;
 *             applied iff missing > 0 and pause >= samples_per_symbol * missing.  The padded message has L + missing bits, the pause
 *             pause - missing * samples_per_symbol; of its np positions the last one is replaced and missing more follow: entries
 *             0 .. np - 2 stay, then A + sps, .., A + missing * sps, then A + missing * sps + the new pause, with A the entry np - 2 -- the
 *             start S of the closing pause (np = L + 2), or the last bit's position of a TRAILING message (np = L + 1), whose pause is
 *             the capture's last pulse-table row when that is a pause too short to close it: such a message is padded as well.  The
 *             record holds n_pad = missing; the caller applies it to bits, pauses and positions.
 *   mid_pos   entry k = int((L + n_pad) / 2) of those positions: the pass's own entry for k <= np - 2, else A + (k - (np - 2)) * sps
 *   rssi      np.mean over the samples [mid_pos, mid_pos + sps) as Python slices them (clipped at the capture's end): every magnitude as
 *             util.get_magnitudes gives it for the sample type (float32: fp32 multiply, add, sqrtf, widened; integer types: C int sum with
 *             its wrap-around, double sqrt, NaN for a negative sum), divided in fp64 by sqrt(min^2 + max^2) of IQArray.min_max_for_dtype,
 *             summed in the order of numpy's float64 np.add.reduce -- pieces of 8192 terms one after the other, each piece pairwise
 *             (eight accumulators per leaf of up to 128 terms, halves split at multiples of 8), as for float32; a contiguous float64
 *             reduction IS cut into buffer-sized pieces --, divided by the count.  NaN for an empty window.  Bit-equal
 *             with the reference for every window length (samples_per_symbol is a uint32).
 *   flag      1 valid; 0: the pass's outputs did not hold the positions the record needs (a capacity was exceeded: repeat the pass);
 *             -1: the summation gave up (its tree went deeper than the kernel's stack: no 64-bit window length does that)
 * The timestamp (signal.timestamp + first_pos / sample_rate) is the caller's: one float expression on values the pass does not know. */
typedef struct urhgpu_msg_record {
    double rssi;
    int64_t first_pos;           /* bit_sample_pos[m][0] */
    int64_t mid_pos;             /* bit_sample_pos[m][int(len(bits) / 2)], after the padding */
    int32_t n_pad;               /* zero bits borrowed from the pause (0: none) */
    int32_t flag;
} urhgpu_msg_record;
/* Queued behind the pass that filled `out` (urhgpu_iq_to_bits_dev, _auto_center_dev, _auto_dev, urhgpu_ppseq_to_bits_dev), on the stream
 * that pass's tail ran on: the tail stream of a pipelined context while its tail is pending (urhgpu_ctx_join then covers the records
 * too), the context's stream otherwise.  No host wait, nothing read back: the kernel reads out->counts[1] on the device, its grid is
 * bounded and workgroups without a message retire.  out->pos is required (the pass ran with write_bit_sample_pos; whether the positions
 * are SHIPPED is another decision: leave them out of the pack).  d_iq: the capture the pass demodulated; IT IS READ BY THIS KERNEL,
 * later than by anything else of the pass: it must stay valid and unchanged until the records are complete.
 * d_rec: device, 16-byte aligned, cap_msg records; record m belongs to message m, for m < min(n_msg, cap_msg, out->cap_msg).
 * h_rec: optional pinned host mirror (16-byte aligned, cap_msg records), stored by one wavefront in one contiguous sweep behind the
 * records kernel; valid once the pass is over, as out->h_counts is.  1 <= message_length_divisor <= 2^30. */
int urhgpu_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n, const urhgpu_params *p, const urhgpu_outputs *out,
                           int64_t message_length_divisor, void *d_rec, int64_t cap_msg, void *h_rec);
/* Every pass of the stream ends with its records.  Before the first push (URHGPU_ERR_ARG after): the record blocks for n_max -- and, for
 * a stream created without want_pos, device room for the positions the kernel reads, which are then computed but not shipped -- are
 * allocated here, so that no push waits.  Such passes take the ordinary route (tail behind the hot kernel, records behind the tail,
 * pack + copy behind the records); urhgpu_stream_push_upload makes ONE copy into d_iq in front of the pass.  May be combined with
 * urhgpu_stream_set_auto_center / _auto_noise.
 * LIFETIME OF d_iq IN SUCH A STREAM: the records kernel reads d_iq behind the pass's tail.  The event the pass's copy waits for is recorded
 * behind that kernel, so a result is never handed out before its records kernel has finished: d_iq (urhgpu_stream_push and
 * urhgpu_stream_push_upload alike) must stay valid and unchanged until the pass's result has been handed out -- a later push's `ready`,
 * or urhgpu_stream_flush -- and may be overwritten from then on. */
int urhgpu_stream_set_msg_records(urhgpu_stream *st, int enable, int64_t message_length_divisor);
/* The records of a pass whose result has been handed out, valid as long as that result: *rec = n_msg records in pinned host memory. */
int urhgpu_stream_msg_records(urhgpu_stream *st, int64_t seq, const urhgpu_msg_record **rec, int64_t *n_msg);
/* how often code reached from the message-record entry points (urhgpu_msg_records_dev, the pushes of a stream with records) made the
 * host wait for the device: the counter of urhgpu_test_center_host_syncs, kept separately for these entry points. */
int64_t urhgpu_test_records_host_syncs(void);

/* ---- DC correction: out = x - mean(x, axis 0), the reference's Filter type dc_correction and its receive path's per-chunk correction ----
 * (Filter.py:31-35, Device.py:822-823).  Bit-equal with numpy's expression for every input:
 *   float32   the mean of a column is numpy's strictly sequential float32 sum from +0.0 (s = fl32(s + x[i]), i = 0 .. n-1), divided in
 *             float64 by n and rounded to float32; the subtraction is float32.  The sum is evaluated in chunks of 4096 samples that are
 *             speculated from a float64 guess and stitched exactly (translated where the proof allows it, re-evaluated serially where not);
 *             captures of at most 8192 samples are summed directly by one wavefront.
 *   integers  the mean is double(exact int64 sum) / double(n); out = (T)(int32) trunc(double(x) - mean): truncated toward zero, low bits kept.
 * Asynchronous on the context's stream, no host wait (but the first call, and a call with a larger n than any before, allocates scratch).
 * d_in, d_out: device, aligned to one sample (2 x the component size); d_out == d_in is allowed, any other overlap is not.  The mean is
 * complete before the subtraction starts.  d_mean: optional, device, 8-byte aligned: the two means, float32 pair for URHGPU_DT_F32, float64
 * pair otherwise.  n == 0: nothing is done.  The calls of one context share one scratch area: they are ordered among themselves. */
int urhgpu_dc_correct_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, void *d_out, void *d_mean);
/* The same on host buffers (h_mean: optional, two float32 or two float64 as above); returns when h_out is complete. */
int urhgpu_dc_correct(urhgpu_ctx *ctx, const void *h_in, int64_t n, int dtype, void *h_out, void *h_mean);
/* how often urhgpu_dc_correct_dev made the host wait for the device (a scratch area that had to grow: freeing the old one waits) */
int64_t urhgpu_test_dc_host_syncs(void);
/* The last float32 call of the context, read back after waiting for the context's stream.  stats[0]: chunks per column (0: the capture
 * was summed directly); stats[1]: chunks (both columns) whose exit followed from the speculated one -- entered exactly as guessed, or
 * translated by the difference of the entries, or entered with a NaN sum --; stats[2]: chunks re-evaluated serially from their true entry;
 * stats[3]: the part of stats[1] that was entered exactly as guessed. */
int urhgpu_test_dc_stats(urhgpu_ctx *ctx, int64_t *stats);

/* ---- DC correction of a sharded capture (urh_amd/sharding.py, "DC correction") ----
 * Rank r holds n samples of one capture; the mean is the whole capture's.  All four calls are asynchronous on the context's stream, share the
 * scratch area of urhgpu_dc_correct_dev (the calls of one context are ordered among themselves) and take a shard aligned to one sample, n >= 0
 * (d_in may be NULL where n == 0).
 *
 * sums: d_words (device, 3 x 8 bytes) = {n, sum of column I, sum of column Q}: exact int64 sums for the integer types; for URHGPU_DT_F32 the bits
 * of two float64 sums (the sums of the shard's 4096-sample chunks, added in order) -- guesses of what the shard adds to the float32 recurrence. */
int urhgpu_shard_dc_sums_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, void *d_words);
/* float32 only.  Speculates the shard's chunks from fl32(base[col] + the float64 sum of the chunks in front) and from that value's neighbour
 * one ulp further from zero, as urhgpu_dc_correct_dev does, and stitches the shard from two entries per column: fl32(base[col]) and its
 * neighbour.  base: host, two doubles (the float64 sums of the ranks in front).  d_records (device, 16-byte aligned, URHGPU_DC_RECORD_BYTES):
 * [column][path] x four uint32 {entry bits, exit bits, room, flags}: the shard entered with `entry` leaves with `exit`; entered D ulps from it,
 * D even, same sign, |D| <= room, it leaves D ulps from `exit`.  room is the minimum over the chunks of m - 1 - |d| (a chunk derived from a
 * record whose path stays m ulps inside its binade, entered d ulps from that record's entry), 0 where a chunk was re-evaluated serially, was
 * taken by exact hit from a record that cannot be translated, or was entered with a NaN sum.  flags bit 0: n == 0, the exit is the entry.  The
 * chunk records stay in the scratch area for urhgpu_shard_dc_resolve_dev. */
#define URHGPU_DC_RECORD_BYTES 64
int urhgpu_shard_dc_spec_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, const double *base, void *d_records);
/* float32 only.  The shard last given to urhgpu_shard_dc_spec_dev on this context (the same d_in and n; anything else, or another DC call that
 * used the chunk area in between, is URHGPU_ERR_ARG) stitched from its true entry: entry (host) = the bits of the two column sums in front of
 * the shard; d_exit (device, 2 x uint32) = the bits of the two sums behind it.  One wavefront over the chunk records; chunks they do not give
 * are re-evaluated serially. */
int urhgpu_shard_dc_resolve_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, const uint32_t *entry, void *d_exit);
/* d_out = d_in - mean in the sample type, the subtraction of urhgpu_dc_correct_dev with a mean given by the caller: mean (host) = two float32 for
 * URHGPU_DT_F32, two float64 otherwise.  d_out == d_in is allowed, any other overlap is not. */
int urhgpu_shard_dc_apply_dev(urhgpu_ctx *ctx, const void *d_in, int64_t n, int dtype, const void *mean, void *d_out);
/* The last urhgpu_shard_dc_spec_dev of the context and the urhgpu_shard_dc_resolve_dev that followed it (zeros: none), read back after waiting for
 * the context's stream.  stats[0..3]: chunks per column, chunks derived from their records and chunks re-evaluated serially over all stitched
 * paths, paths per column; stats[4..7]: the same for the resolve. */
int urhgpu_shard_dc_stats(urhgpu_ctx *ctx, int64_t *stats);

/* ---- message records of a sharded capture (urh_amd/sharding.py, "message records") ----
 * One urhgpu_msg_record per message that CLOSES on this rank, behind the sharded pass that filled `out` (urhgpu_shard_bits_finish_dev; out->pos
 * required): concatenated in rank order they are the records urhgpu_msg_records_dev gives for the whole capture, bit for bit.  A rank's second and
 * later messages start behind a pause row that ends in its shard and are closed by a pause of more than pause_threshold symbols that ends in it
 * too: their bits, positions and middle window lie in the shard.  The FIRST message a rank closes may have begun on earlier ranks, and its
 * window [mid_pos, min(mid_pos + samples_per_symbol, n_total)) may lie anywhere up to the end of the closing pause.  What it needs crosses the
 * ranks in two all-gathers, and a third where a first window is not wholly inside its closing rank's shard (the caller gathers; every
 * decision is a pure function of gathered words).  All three calls are asynchronous, on the stream urhgpu_msg_records_dev would take.
 *
 * 1. summary: d_words (device, 8-byte aligned) = URHGPU_SHARD_REC_SUMMARY_WORDS int64, from the pass's device counts and offsets:
 *      [0] pos_base   [1] n_local   [2] messages closed here
 *      [3] bits before the first close (all the rank's bits when none closes)   [4] position entries before the first close (likewise)
 *      [5] bits behind the last close (0 when none closes)                      [6] position entries behind the last close (likewise)
 *      [7] the pause of the first message closed here (0: none)
 *      [8] 1: the pass's outputs stayed inside their capacities on this rank (rows, messages, bits, positions), 0: not
 *      [9] the rank's position entries
 *    From the gathered words every rank derives, for the first message of every closing rank: L and np (summed over the ranks since the
 *    previous close), n_pad, the middle index k, and which rank holds, at which local index, position entry 0 and entry rel (np - 2 where
 *    the middle lies in the padded part, k otherwise).
 * 2. look-up: d_index (device, n int64): the LOCAL index into out->pos of every entry asked of this rank, -1 where another rank holds it;
 *    d_values (device, n int64) = out->pos[d_index[i]], 0 for -1 or an index the rank does not hold.  Gathered, the values give first_pos and
 *    mid_pos of every first message, and so its window.
 * 3. windows (only where a first window leaves its closing rank's shard): the ranks contribute the raw samples of those windows that their
 *    shards hold; the closing rank assembles its window contiguously (d_window, window_len samples of the capture's sample type).
 * finish: urhgpu_shard_msg_records_dev.  d_iq: the shard the pass demodulated, samples [pos_base, pos_base + n_local) of the n_total; it is read
 *    here, later than by anything else of the pass.  first (HOST, URHGPU_SHARD_REC_FIRST_WORDS int64): the first message closed here, from the
 *    gathered data: {1: this rank closes a message, L, np, n_pad, first_pos, mid_pos, 1: every rank that contributes to it held its capacities
 *    and its entries exist, 1: its window is d_window[0 .. w)} (0: its window lies in the shard).  Every other message is computed as
 *    urhgpu_msg_records_dev computes it, from out's own msg_off / pos_off / pos / pauses, with its samples read at mid_pos - pos_base.
 *    flag: 1 valid; 0: a capacity was exceeded on a rank that contributes to the message (on this rank: every record it writes); -1 as for
 *    urhgpu_msg_records_dev; -2: the window is not inside the shard and no assembled window was given -- nothing outside the shard is read,
 *    rssi is NaN.  For a message that is not the first one closed here this does not occur (DESIGN.md 5 has the argument).
 *    d_rec / cap_msg / h_rec, the bounded grid, n_msg read on the device and the mirror sweep: as urhgpu_msg_records_dev. */
#define URHGPU_SHARD_REC_SUMMARY_WORDS 10
#define URHGPU_SHARD_REC_FIRST_WORDS 8
int urhgpu_shard_records_summary_dev(urhgpu_ctx *ctx, int64_t n_local, int64_t pos_base, const urhgpu_outputs *out, void *d_words);
int urhgpu_shard_records_lookup_dev(urhgpu_ctx *ctx, const urhgpu_outputs *out, const void *d_index, int64_t n, void *d_values);
int urhgpu_shard_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t n_local, int64_t pos_base, int64_t n_total, const urhgpu_params *p,
                                 const urhgpu_outputs *out, int64_t message_length_divisor, const int64_t *first, const void *d_window,
                                 int64_t window_len, void *d_rec, int64_t cap_msg, void *h_rec);

/* ---- a batch of captures in one pass: a wavefront per capture -------------------------------------------------------------------
 * Every entry point above takes ONE capture per pass, and below a few hundred thousand samples a pass is all fixed cost (a dozen
 * launches whose kernels run for microseconds).  A recording session is hundreds or thousands of short captures: here K of them lie
 * back to back in one device buffer and are demodulated and digitised by THREE launches whatever K and the lengths are -- one
 * wavefront walks one capture (afp_demod, grab_pulse_lens and _ppseq_to_bits followed almost literally: signal_functions.pyx:333-378,
 * :392-495, ProtocolAnalyzer.py:323-414), one workgroup takes the prefix of the result sizes, one wavefront per capture packs its
 * results.  Every capture's results are those of urhgpu_iq_to_bits_dev for that capture alone, bit for bit.  The counterpart of
 * urhgpu_modulate_dev's batch of messages.  Long captures still belong to passes and streams: a wavefront walks its capture serially.
 * These three calls gate every capture with p->noise_threshold and slice it with p->center; the estimators that give every capture its own
 * are the two sections below: a noise threshold per capture (urhgpu_iq_to_bits_batch_auto_dev), a center per capture
 * (urhgpu_iq_to_bits_batch_center_dev).
 *   Input    d_iq: (total, 2) interleaved samples of p->dtype (any of the five), 16-byte aligned; d_start: device int64[k + 1], the first
 *            sample of each capture (a capture may start at any sample; lengths 0 .. 2^31 - 1); one urhgpu_params for all.  ASK and FSK;
 *            PSK and URHGPU_MOD_OTHER: URHGPU_ERR_UNSUPPORTED.  Any tolerance (uint16), bits_per_symbol 1 .. 7.
 *   Plan     urhgpu_batch_plan (host arithmetic, works without a GPU): from the k lengths, the parameters and a row-capacity policy --
 *            0: urhgpu_stream_capacities' formula with a floor of 64 rows instead of 4096, min(n / (tolerance + 1) + 2, max(64, 4 * (n /
 *            samples_per_symbol) + 64)); 1: the hard bound n / (tolerance + 1) + 2, which cannot truncate; 2: cap_rows_fixed for every
 *            capture -- plan[0 .. k) = the byte offset of each capture's region of the work buffer (disjoint, in order, 16-byte
 *            aligned), plan[k .. 2k) = its row capacity, plan[2k .. 3k) = the launch order (a permutation, longest capture first, so
 *            that the long ones do not trail), *work_bytes, and *blob_capacity = what the blobs of all captures can need at most.  The
 *            caller uploads the plan as it is (device int64[3 k]) and allocates the two buffers.  A region's bit and message
 *            capacities follow from its row capacity and cannot overflow while the rows fit.
 *   Pass     urhgpu_iq_to_bits_batch_dev: asynchronous on the context's stream, the caller owns all memory, nothing is copied.
 *            d_qad: NULL or float32[total], the demodulated signal of every capture at its samples' indices.  d_counts: int64[8 k],
 *            per capture {rows stored, messages, bits, rows_needed, truncated, 0, 0, 0}.  d_dir: int64[k + 1], the byte offset of each
 *            capture's blob in d_blob; d_dir[k] = the used part.  At d_dir[i] lies capture i's STANDARD compact result blob (above):
 *            header flags 0, int8 row_state, int32 row_len, bits packed most significant first, no position section (positions are
 *            a function of the rows: the host derives them).  A capture that outgrows its region stops storing and keeps counting:
 *            truncated bit 0 is set, rows_needed is exact, the blob holds what fitted -- the FIRST row-capacity rows of the table, and
 *            the bits, msg_off and pauses that _ppseq_to_bits gives for exactly those rows as if the table ended there (the last stored
 *            row closes the last message): the result of a shorter table, not a prefix of the full result's bits.  The demodulated
 *            signal does not depend on the capacity.  A wavefront never writes outside its region.
 *            truncated bit 3, a capture the pass refuses, in two forms.  Its start or end does not lie inside the buffer (a negative
 *            start, start[i] > start[i + 1], start[i + 1] > total, more than 2^31 - 1 samples): nothing of it is read or stored,
 *            rows_needed is 0 and truncated is 8.  Its plan entry alone is bad (a negative region offset or one that is no multiple of
 *            16, a region that ends beyond work_bytes, a negative row capacity): its samples are valid, so it IS demodulated and
 *            walked -- its slice of d_qad is written and rows_needed is exact -- but nothing is stored in the work buffer, and bit 0 is
 *            set beside bit 3 when it needed any row.  In both forms rows, messages and bits are 0 and the blob is a well-formed empty
 *            one (header, msg_off[0] = 0); the other captures are not affected.  k = 0 and captures of length 0 are accepted.
 *   Fetch    urhgpu_batch_fetch: the directory (one read of 8 (k + 1) bytes into h_dir), then ONE copy of d_dir[k] bytes into h_blob
 *            (pinned memory: at PCIe speed); synchronous.  *total_bytes = d_dir[k] (also on URHGPU_ERR_CAPACITY: cap_host too small).
 *   urhgpu_batch_step: samples a wavefront takes per step.  urhgpu_batch_launches: out2 = {kernel launches, copies} the two calls
 *   above have issued on this context -- 3 per pass and 2 per fetch, whatever k and the lengths are. */
int urhgpu_batch_step(void);
int urhgpu_batch_plan(const int64_t *lengths, int64_t k, const urhgpu_params *p, int policy, int64_t cap_rows_fixed, int64_t *plan,
                      int64_t *work_bytes, int64_t *blob_capacity);
int urhgpu_iq_to_bits_batch_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                const urhgpu_params *p, float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir,
                                void *d_blob, int64_t cap_blob);
int urhgpu_batch_fetch(urhgpu_ctx *ctx, const int64_t *d_dir, int64_t k, const void *d_blob, int64_t *h_dir, void *h_blob, int64_t cap_host,
                       int64_t *total_bytes);
int urhgpu_batch_launches(urhgpu_ctx *ctx, int64_t *out2);

/* ---- a batch of captures: automatic noise threshold per capture, on the device ----------------------------------------------------
 * The reference opens every file of a recording session with noise_threshold = detect_noise_level(magnitudes) of THAT capture
 * (Signal.py:97-103, AutoInterpretation.py:60-91), and the captures of a session differ in gain by tens of dB: no single threshold
 * decodes them.  Here the K noise floors of a batch are decided by ONE launch and the batch's walk gates each capture with its own.
 *   urhgpu_batch_noise_dev            d_iq, total, d_start, d_plan, k, p as for urhgpu_iq_to_bits_batch_dev (of the plan only the launch
 *            order is followed; no work buffer is needed).  One launch, asynchronous on the context's stream, the caller owns all memory:
 *            a workgroup per capture takes the per-chunk (sum, max) of the magnitudes -- chunks of max(1, n / 100) samples counted from
 *            the END of that capture, at most 199; the sum in numpy's float64 pairwise order, so that sum / chunk IS np.mean(chunk) bit
 *            for bit; no load leaves [start[c], start[c + 1]) -- and decides with the body of the single-capture chain (k_noise_decide).
 *            d_noise: device urhgpu_noise_result[k], 8-byte aligned, block c = capture c's.  Flags per capture:
 *              flag 1  noise = detect_noise_level's value, also the 0 it returns for n <= 3, close means, a NaN mean, an all-zero capture;
 *                      and a capture whose start or end the batch refuses (truncated bit 3 above): nothing is read, noise = 0
 *              flag 2  noise is the value, but it is not below Signal.max_magnitude of the sample type: the reference demodulates nothing
 *                      and slices zeros(2) (Signal.py:474-484)
 *              flag 0  the reference raises (math.ceil of a NaN: ValueError, of an infinity: OverflowError); noise holds that value
 *            With flag 0 or 2 the block's noise_f32 / noise_sqrd are those of p->noise_threshold (as in a pass: "use_cfg").
 *   urhgpu_iq_to_bits_batch_auto_dev  urhgpu_iq_to_bits_batch_dev's arguments plus d_noise: FOUR launches whatever k and the lengths are,
 *            k = 0 included -- noise, bits, scan, pack.  The wavefront of capture c loads noise_sqrd and flag from d_noise[c] (uniform
 *            loads).  Flag 1: every result is that of urhgpu_iq_to_bits_batch_dev with noise_threshold = (float)noise.  Flag 2: the
 *            capture is walked as TWO samples, settled on the device -- two zeros are demodulated (only the first two entries of its slice
 *            of d_qad are written) and sliced; the caller reports n_samples = 2.  Flag 0: walked with p->noise_threshold, so that the
 *            pass stays well defined; the caller raises instead of handing the result out.
 *   urhgpu_batch_noise_fetch          one copy of 64 k bytes into h_noise (pinned host memory), synchronous.  With urhgpu_batch_fetch: the
 *            directory, the blob and the K result blocks in THREE copies whatever k >= 1 is.
 * urhgpu_batch_launches counts these launches and copies too: 4 per automatic pass, 1 per urhgpu_batch_noise_dev, 1 per noise fetch. */
int urhgpu_batch_noise_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                           const urhgpu_params *p, urhgpu_noise_result *d_noise);
int urhgpu_iq_to_bits_batch_auto_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                     const urhgpu_params *p, float *d_qad, void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir,
                                     void *d_blob, int64_t cap_blob, urhgpu_noise_result *d_noise);
int urhgpu_batch_noise_fetch(urhgpu_ctx *ctx, const urhgpu_noise_result *d_noise, int64_t k, urhgpu_noise_result *h_noise);

/* ---- a batch of captures: automatic center per capture, on the device ------------------------------------------------------------
 * The reference detects the center of every signal it demodulates (AutoInterpretation.detect_center, AutoInterpretation.py:226-277), and
 * for ASK the center follows the received amplitude: captures that differ in gain cannot share p->center.  Here the K captures of a batch
 * are demodulated into one buffer, ONE chain of kernels runs detect_center on the K ranges (the chain of "automatic center inside a pass"
 * above, over many ranges: urh_amd/csrc/msg_estimators.hip), and the batch's walk slices each capture with the thresholds of its own
 * center.  Capture c's results are those of urhgpu_iq_to_bits_auto_center_dev (with automatic noise: urhgpu_iq_to_bits_auto_dev) on that
 * capture alone, bit for bit, the flag protocol included: WITH FLAG 0, 2 OR 3 THE CAPTURE WAS SLICED WITH p->center, and a caller that wants
 * the reference's result for flag 2 / 3 settles the center on the host and slices those captures again (urhgpu_qad_to_bits_batch_dev with
 * thresholds of its own: one call for all of them).  The caller owns all memory; nothing is waited for but the fetch.
 *   urhgpu_batch_center_plan   host arithmetic, works without a GPU: *scratch_bytes the chain needs for k captures in a buffer of `total`
 *            samples (total < 0: the sum of lengths[k]; lengths may be NULL when total is given) with a pool of max_bins bins per capture
 *            (urhgpu_center_hist_cap), *group = captures per group -- the captures are taken in groups whose histogram pool stays within
 *            64 MiB, as urhgpu_msg_center_stats takes its messages: max(1, 64 MiB / (4 max_bins)) --, *n_groups = ceil(k / group).
 *   urhgpu_batch_center_dev    the chain and the publish step alone on d_qad (device float32[total]; capture c = [d_start[c], d_start[c + 1])
 *            by the batch's rules: a refused start or end is an empty range).  max_size as for urhgpu_detect_center_dev.  d_noise: NULL, or
 *            the batch's urhgpu_noise_result[k] -- a capture with flag 2 has the range of its two zeros.  14 launches and one fill per
 *            GROUP, whatever k and the lengths are: the launch count is a function of ceil(k / group) alone.  Outputs:
 *              d_thr     NULL or float32[k][order - 1], cap_thr floats: capture c's slicing thresholds -- urhgpu_get_center_thresholds'
 *                        arithmetic on (float)center for flag 1, on p->center otherwise
 *              d_result  urhgpu_batch_center_result[k + 1], cap_result blocks: block c = capture c's urhgpu_center_result and the offset of
 *                        its counts in the tie pool; the trailing block's counts_off = counts reserved in the pool (its cursor)
 *              d_tie     NULL or uint32[cap_tie], the tie pool: for flag 3 alone the histogram's n_bins counts, appended in no particular
 *                        order.  A capture whose counts do not fit gets n_counts = 0; nothing is stored beyond cap_tie.
 *            d_scratch: 256-byte aligned, scratch_bytes >= the plan's.  A capacity that is too small: URHGPU_ERR_CAPACITY, nothing is
 *            launched.  Starts that overlap can ask for more tiles than the scratch holds (total / 4096 + group + 1): the captures that
 *            do not fit get no center (flag 0).
 *   urhgpu_qad_to_bits_batch_dev   urhgpu_iq_to_bits_batch_dev on captures that are ALREADY demodulated: the walk reads d_qad (4-byte
 *            aligned) as it lies there, then scan and pack: three launches.  d_thr: NULL -- every capture is sliced with p->center -- or
 *            float32[k][order - 1] in device memory.  d_noise: NULL or the batch's result blocks (flag 2: two samples are walked).
 *   urhgpu_iq_to_bits_batch_center_dev   the whole pass: urhgpu_batch_noise_dev's launch when auto_noise is not 0, the demodulation of all
 *            captures into d_qad (required; a workgroup per capture), the chain and the publish step per group, the qad-input walk, scan,
 *            pack: 4 (auto_noise: 5) + 14 n_groups launches.  Arguments as for urhgpu_iq_to_bits_batch_auto_dev and urhgpu_batch_center_dev.
 *   urhgpu_batch_center_fetch  the k + 1 result blocks into h_result, then the used part of the tie pool -- min(cursor, cap_tie) counts,
 *            *used -- into h_tie (cap_host counts): two copies at most, one when no capture tied; synchronous.
 * urhgpu_batch_launches counts these launches and copies too. */
typedef struct urhgpu_batch_center_result {
    urhgpu_center_result r;      /* n_counts: n_bins when flag == 3 and the counts fitted the tie pool, else 0 */
    int64_t counts_off;          /* first of the n_counts counts in the tie pool; trailing block: counts reserved in the pool */
} urhgpu_batch_center_result;
int urhgpu_batch_center_plan(const int64_t *lengths, int64_t k, int64_t total, int64_t max_bins, int64_t *scratch_bytes, int64_t *n_groups,
                             int64_t *group);
int urhgpu_batch_center_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, int64_t k, const urhgpu_params *p,
                            int64_t max_size, const urhgpu_noise_result *d_noise, void *d_scratch, int64_t scratch_bytes, float *d_thr,
                            int64_t cap_thr, void *d_result, int64_t cap_result, uint32_t *d_tie, int64_t cap_tie);
int urhgpu_qad_to_bits_batch_dev(urhgpu_ctx *ctx, const float *d_qad, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                 const urhgpu_params *p, const float *d_thr, int64_t cap_thr, const urhgpu_noise_result *d_noise, void *d_work,
                                 int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob);
int urhgpu_iq_to_bits_batch_center_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                       const urhgpu_params *p, int auto_noise, int64_t max_size, float *d_qad, void *d_work, int64_t work_bytes,
                                       int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob, urhgpu_noise_result *d_noise,
                                       void *d_scratch, int64_t scratch_bytes, float *d_thr, int64_t cap_thr, void *d_result, int64_t cap_result,
                                       uint32_t *d_tie, int64_t cap_tie);
int urhgpu_batch_center_fetch(urhgpu_ctx *ctx, const void *d_result, int64_t k, const uint32_t *d_tie, int64_t cap_tie, void *h_result,
                              uint32_t *h_tie, int64_t cap_host, int64_t *used);

/* ---- a batch of captures: message records per capture, on the device --------------------------------------------------------------
 * What a user wants from a recording session is its messages: ProtocolAnalyzer.get_protocol_from_signal gives every Message of every file an
 * RSSI, a timestamp and, for ASK, the padding to message_length_divisor ("message records inside a pass" above has the arithmetic and the
 * record).  Here that step is queued behind the walk of a batch -- urhgpu_iq_to_bits_batch_dev, _batch_auto_dev, _batch_center_dev or
 * urhgpu_qad_to_bits_batch_dev -- for all K captures at once.  Capture c's records are those of urhgpu_msg_records_dev behind
 * urhgpu_iq_to_bits_dev on that capture alone, bit for bit, the RSSI included.
 *   urhgpu_batch_msg_records_dev   asynchronous on the context's stream, the caller owns all memory, nothing is copied or waited for.
 *            Queued behind the batch pass that filled d_work and d_counts, before anything rewrites them.  d_iq, total, d_plan, k, p, d_work,
 *            work_bytes, d_counts: that pass's (of the qad-input walk: the samples the captures were demodulated from).  THREE launches
 *            whatever k, the lengths and the number of messages are:
 *              directory   d_rec_dir: int64[k + 1], the exclusive prefix of the captures' stored messages (d_counts[8 c + 1]): capture c's
 *                          records are d_rec[d_rec_dir[c] .. d_rec_dir[c + 1]), d_rec_dir[k] = M, the messages of the whole batch.  The host
 *                          knows M without reading it: the sum of the blob headers' n_msg.
 *              positions   a batch ships no positions (they are a function of the pulse table); a wavefront per capture derives the three
 *                          entries a record needs -- the first bit's, the entry np - 2 and the middle bit's -- from the capture's stored rows
 *                          in d_work, with _ppseq_to_bits' control flow and arithmetic (ProtocolAnalyzer.py:346-411)
 *              RSSI        a workgroup per message over a bounded grid; the window [mid_pos, mid_pos + samples_per_symbol) is Python's slice
 *                          of THE CAPTURE: clipped at its length n_c = d_start[c + 1] - d_start[c], whatever its noise flag -- the next
 *                          capture lies directly behind it.  No load leaves [d_start[c], d_start[c + 1]).
 *            d_start: int64[k_all + 1], the captures' first samples in d_iq.  d_map: NULL (then k_all == k, capture j's samples are capture
 *            j's), or int64[k]: capture j of this call -- its plan entry, region and counts -- takes its samples from capture d_map[j] of
 *            d_start, whose length is the length its region was planned for.  That serves captures sliced a second time from a gathered
 *            demodulated buffer (urhgpu_qad_to_bits_batch_dev after a center the host settled): their rows lie in the second call's regions,
 *            their samples where they were.  An index outside [0, k_all) is a refused capture.  d_noise: NULL, or the batch's
 *            urhgpu_noise_result[k]; a capture's region is laid out from its true length also where its flag is 2 and two samples were
 *            walked, and its window is clipped at the true length, so the blocks are accepted and not read.
 *            d_rec: urhgpu_msg_record[cap_rec], 16-byte aligned; d_rec_capture: int32[cap_rec], for record i the capture of d_start its
 *            samples lie in.  A message beyond cap_rec is not stored; the sum of the plan's row capacities / 2 + 1 holds every batch.
 *            Flags as for urhgpu_msg_record; every stored message of a capture whose results were truncated or refused (bits 0 and 3 of
 *            `truncated`) gets flag 0 and a NaN RSSI: repeat that capture with the rows it needs.
 *            Rejected before anything is launched (and without a GPU, in this order): parameters a batch refuses -- PSK and
 *            URHGPU_MOD_OTHER: URHGPU_ERR_UNSUPPORTED; a sample type: URHGPU_ERR_DTYPE --, a message_length_divisor outside 1 .. 2^30,
 *            cap_rec < 0, a misaligned pointer, a missing context or buffer: URHGPU_ERR_ARG.
 *   urhgpu_batch_records_fetch     ONE copy of the first n_rec records into h_rec (pinned host memory, 16-byte aligned); synchronous.  None
 *            for n_rec = 0.  n_rec > cap_rec: URHGPU_ERR_CAPACITY.
 * urhgpu_batch_launches counts these too: 3 launches per urhgpu_batch_msg_records_dev and 1 copy per urhgpu_batch_records_fetch of at least
 * one record, whatever k, the lengths and M are. */
int urhgpu_batch_msg_records_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, int64_t k_all, const int64_t *d_map,
                                 const int64_t *d_plan, int64_t k, const urhgpu_params *p, const urhgpu_noise_result *d_noise,
                                 int64_t message_length_divisor, const void *d_work, int64_t work_bytes, const int64_t *d_counts,
                                 int64_t *d_rec_dir, void *d_rec, int64_t cap_rec, int32_t *d_rec_capture);
int urhgpu_batch_records_fetch(urhgpu_ctx *ctx, const void *d_rec, int64_t n_rec, int64_t cap_rec, void *h_rec);

/* ---- a batch of captures: message ranges per capture ------------------------------------------------------------------------------
 * Every batch entry point above takes finished parameters.  The reference learns modulation, samples per symbol and tolerance when it opens
 * a file (AutoInterpretation.estimate, AutoInterpretation.py:373-470), and that starts with the capture's message ranges:
 * auto_interpretation.segment_messages_from_magnitudes (auto_interpretation.pyx:55-111).  Here the ranges of all K captures of a batch come
 * out of three launches; capture c's pairs are those of urhgpu_message_ranges_dev (merge off) on that capture alone with ITS threshold.
 *   urhgpu_batch_segments_dev      asynchronous on the context's stream, the caller owns all memory, nothing is copied or waited for.
 *            d_iq, total, d_start, d_plan, k: as for urhgpu_iq_to_bits_batch_dev (of the plan only the launch order is read).  dtype: the
 *            sample type.  d_thr: float[k], capture c's noise threshold; a sample is above the noise where double(magnitude) > double(thr)
 *            -- the magnitude as util.get_magnitudes gives it for the sample type --, so a NaN threshold yields no segment.
 *            THREE launches whatever k and the lengths are:
 *              segments    a wavefront per capture, a step of urhgpu_batch_step() samples; the state of sample 0, conseq_above and
 *                          conseq_below with outlier_tolerance = 10, a segment opened at i - conseq_above and closed at i - conseq_below,
 *                          the trailing rule state == 1 and start < N - conseq_below -- followed over the runs of the step's above-noise
 *                          mask.  Capture c's (start, end) int64 pairs, relative to its first sample, go to ITS region
 *                          d_seg[2 d_region[c] ..) of urhgpu_batch_segments_capacity(n_c) = n_c / 20 + 1 pairs (a segment needs ten samples
 *                          to open and ten to close: the capacity cannot truncate); d_counts[c] = the exact number of its segments.  Every
 *                          store is bounded by the capacity; a region that does not lie inside [0, cap_seg) pairs stores nothing.  No load
 *                          leaves [d_start[c], d_start[c + 1]); a refused start or end (outside [0, total], descending) is an empty capture.
 *              directory   d_dir: int64[k + 1], the exclusive prefix of the captures' stored segments; d_dir[k] = M
 *              compaction  d_out: the stored pairs of all captures in capture order, capture c's at d_out[2 d_dir[c] ..); pairs beyond cap_out
 *                          are not written
 *            d_seg, d_out: 16-byte aligned.  Rejected before anything is launched (and without a GPU): a sample type: URHGPU_ERR_DTYPE; a
 *            negative size, a misaligned pointer, a missing context or buffer: URHGPU_ERR_ARG.
 *   urhgpu_batch_segments_fetch    synchronous: ONE copy of the directory into h_dir, then ONE copy of the M pairs into h_out (none for
 *            M = 0).  *n_segments = M.  M > cap_host (pairs): URHGPU_ERR_CAPACITY, the directory has been read.
 *   urhgpu_batch_demod_dev         the demodulation launch of urhgpu_iq_to_bits_batch_center_dev alone: afp_demod of every capture into
 *            d_qad[total] (the rules of sample 0 and of n <= 2 per capture; a sample's predecessor is never the neighbouring capture's).
 *            d_noise: NULL -- every capture gated with p->noise_threshold --, or urhgpu_noise_result[k]: capture c gated with block c's
 *            noise_sqrd; a block with flag 2 writes two zeros and nothing else, as in that pass.  ONE launch.
 * urhgpu_batch_launches counts these too: 3 launches per urhgpu_batch_segments_dev, 1 per urhgpu_batch_demod_dev, and 2 copies per
 * urhgpu_batch_segments_fetch (1 when M = 0), whatever k, the lengths and M are. */
int64_t urhgpu_batch_segments_capacity(int64_t n);
int urhgpu_batch_segments_dev(urhgpu_ctx *ctx, const void *d_iq, int dtype, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                              const float *d_thr, const int64_t *d_region, int64_t *d_seg, int64_t cap_seg, int64_t *d_counts, int64_t *d_dir,
                              int64_t *d_out, int64_t cap_out);
int urhgpu_batch_segments_fetch(urhgpu_ctx *ctx, const int64_t *d_dir, int64_t k, const int64_t *d_out, int64_t *h_dir, int64_t *h_out,
                                int64_t cap_host, int64_t *n_segments);
int urhgpu_batch_demod_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                           const urhgpu_params *p, const urhgpu_noise_result *d_noise, float *d_qad);

/* ---- a batch of captures: PSK, a Costas loop per capture in one launch ------------------------------------------------------------
 * The Costas loop (costa_demod, signal_functions.pyx:252-330) is a serial recurrence: its cost is the latency of about 94 dependent
 * instructions per sample.  A pass over one capture hides it by cutting a long capture into chunks and speculating on their start states; a
 * short capture runs on one wavefront of the whole chip.  In a batch the parallelism is ACROSS captures: every capture starts in the known
 * state {freq 0, phase 1.5}, nothing is speculated, and K loops run side by side -- a LANE per capture, a wavefront per 64 captures taken in
 * the plan's launch order (urh_amd/csrc/batch_psk.hip).  The device time follows the LONGEST capture, not the number of captures.  Capture
 * c's results are those of urhgpu_iq_to_bits_dev (with auto_noise / auto_center: urhgpu_iq_to_bits_auto_dev / _auto_center_dev) on that
 * capture alone with PSK parameters, bit for bit.  The other batch entry points keep refusing PSK.
 *   urhgpu_batch_costas_dev    the demodulation launch alone, asynchronous on the context's stream: afp_demod with PSK of every capture
 *            into d_qad[total].  d_iq, total, d_start, d_plan, k: as for urhgpu_iq_to_bits_batch_dev (of the plan only the launch order
 *            is read; a plan made for the same lengths, tolerance, samples per symbol and bits per symbol with the parameters recoded as
 *            FSK serves).  Per capture: n <= 2 gives zeros(n); otherwise d_qad[s0] = -4 (the reference leaves that element unwritten) and the
 *            loop runs from sample 1 in {freq 0, phase 1.5}; a sample with re * re + im * im <= noise_sqrd on its raw values gives -4 and
 *            freezes the state; the state never crosses a capture boundary; a refused start or end reads and writes nothing.  d_noise: NULL
 *            -- every capture gated with p->noise_threshold --, or urhgpu_noise_result[k]: capture c gated with block c's noise_sqrd; a
 *            block with flag 2 writes two zeros and nothing else.  Loop order min(2 ^ bits_per_symbol, 4) (p->mod_order where > 0).  ONE
 *            launch of ceil(k / 64) workgroups whatever the lengths are.  Rejected before anything is launched (and without a GPU):
 *            anything but PSK and a loop order other than 2 / 4: URHGPU_ERR_UNSUPPORTED; a sample type: URHGPU_ERR_DTYPE; a negative
 *            size, a misaligned pointer, a missing context or buffer: URHGPU_ERR_ARG.
 *   urhgpu_iq_to_bits_batch_psk_dev   the whole pass: urhgpu_batch_noise_dev's launch when auto_noise is not 0, the Costas launch into
 *            d_qad (required), -- when auto_center is not 0 -- the center chain and the publish step per group, the qad-input walk (its
 *            FSK instantiation: the noise value is the same -4 and there is no ASK rule; without auto_center every capture is sliced with
 *            p->center and d_scratch, d_thr, d_result, d_tie are not read), scan, pack.  4 launches (auto_noise: 5) without auto_center,
 *            4 (5) + 14 n_groups with it: neither depends on k or the lengths.  Arguments and the flag protocol as for
 *            urhgpu_iq_to_bits_batch_center_dev; fetched with urhgpu_batch_fetch, urhgpu_batch_noise_fetch and urhgpu_batch_center_fetch.
 *            Records: urhgpu_batch_msg_records_dev behind it with the parameters recoded as FSK -- the record arithmetic reads the
 *            modulation for the ASK padding alone.
 * urhgpu_batch_launches counts these too: 1 launch per urhgpu_batch_costas_dev, the launches above per urhgpu_iq_to_bits_batch_psk_dev. */
int urhgpu_batch_costas_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                            const urhgpu_params *p, const urhgpu_noise_result *d_noise, float *d_qad);
int urhgpu_iq_to_bits_batch_psk_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                    const urhgpu_params *p, int auto_noise, int auto_center, int64_t max_size, float *d_qad, void *d_work,
                                    int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob,
                                    urhgpu_noise_result *d_noise, void *d_scratch, int64_t scratch_bytes, float *d_thr, int64_t cap_thr,
                                    void *d_result, int64_t cap_result, uint32_t *d_tie, int64_t cap_tie);

/* ---- a batch of captures: DC correction per capture ---------------------------------------------------------------------------------
 * out_c = x_c - mean(x_c, axis 0) for every capture c of a batch (Filter.py:31-35, Device.py:822-823: the default of the reference's receive
 * path), bit for bit what urhgpu_dc_correct_dev gives for that capture alone and what numpy's expression gives -- for float32 captures that
 * includes the strictly sequential float32 column sum.  urhgpu_dc_correct_dev takes one capture per call, up to five launches and a work area
 * of the context; a batch evaluates the serial sums side by side instead (urh_amd/csrc/batch_dc.hip): nothing is speculated.
 *   urhgpu_batch_dc_correct_dev   TWO launches on the context's stream whatever k and the lengths are, asynchronous: the two column means of
 *            every capture (float32: a lane per capture and column, a wavefront per 32 captures taken in the plan's launch order, so the
 *            device time follows the LONGEST capture; integers: exact int64 sums, a workgroup per capture), then the subtraction of all
 *            captures (float32 subtracts in float32; integers give (T)(int32) trunc(double(x) - mean)).  d_iq, total, d_start, d_plan, k:
 *            as for urhgpu_iq_to_bits_batch_dev (of the plan only the launch order is read); dtype: URHGPU_DT_*.  d_out: d_iq itself (in
 *            place) or a buffer of total samples that does not overlap it; capture c lies at the same samples of it, so the same d_start
 *            and d_plan serve every later batch call on d_out.  Samples that belong to no capture are neither read nor written; a capture
 *            whose start or end is refused is an empty capture.  d_mean: NULL, or k pairs of means -- float[2 k] for float32 captures,
 *            double[2 k] otherwise; an empty capture writes nothing but its pair, NaN (numpy's 0 / 0).  Without d_mean the pairs live in a
 *            buffer of the context between the two launches (calls on one stream share it in order; it only grows).  k == 0 launches nothing.
 *            Rejected before anything is launched (and without a GPU): a sample type: URHGPU_ERR_DTYPE; a negative size, a missing context
 *            or buffer, d_iq or d_out not aligned to 16 bytes, d_start, d_plan or d_mean not aligned to 8, d_out overlapping d_iq without
 *            being it: URHGPU_ERR_ARG.
 * urhgpu_batch_launches counts the two launches. */
int urhgpu_batch_dc_correct_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan,
                                int64_t k, void *d_out, void *d_mean);

/* ---- a batch of captures: parameters per capture ------------------------------------------------------------------------------------
 * Every batch entry point above takes ONE urhgpu_params for all captures.  A recording session's transmitters are not alike, and the
 * reference opens each file with its own Signal parameters (ProtocolAnalyzer.get_protocol_from_signal per file): estimated centers and noise
 * floors are floats that differ in every capture, so grouping by equal parameters is a batch per capture.  Here capture c is demodulated,
 * sliced and turned into bits -- and, on request, message records -- with table[c], and the launch count depends neither on k nor on the
 * number of different parameter sets.  Capture c's results are those of urhgpu_iq_to_bits_dev (records: urhgpu_msg_records_dev behind it) on
 * that capture alone with its parameters, bit for bit, the demodulated signal and the RSSI included (urh_amd/csrc/batch_each.hip).
 *   Table    urhgpu_batch_each[k] in device memory, 16-byte aligned, 32 bytes per capture: the modulation (URHGPU_MOD_ASK or _FSK),
 *            bits_per_symbol (1 .. 7), samples_per_symbol (>= 1), tolerance (0 .. 65535), pause_threshold, noise_val (0 for ASK, -4 for
 *            FSK: get_noise_for_mod_type) and thr_first, the index of the capture's first slicing threshold in ONE shared table
 *            d_thr = float[n_thr], n_thr = the sum of (1 << bits_per_symbol) - 1 over the captures, which the host fills with
 *            urhgpu_get_center_thresholds(center_c, center_spacing_c, 1 << bits_per_symbol_c, d_thr + thr_first_c).  The wavefront of
 *            capture c loads its record and its thresholds through uniform addresses and reads no other capture's.  A record the device
 *            does not accept -- a value outside these ranges, thresholds that do not lie inside [0, n_thr), a noise_val that is not its
 *            modulation's, a modulation other than that of the launch its plan position falls in -- makes capture c a refused capture
 *            (truncated bit 3: nothing of it is read or stored, a well-formed empty blob); the other captures are not affected.
 *   Noise    d_noise: urhgpu_noise_result[k], 8-byte aligned, always read: capture c is gated with block c's noise_sqrd.  auto_noise 0:
 *            the CALLER has written the blocks -- flag 1, noise_f32 = (float)noise_threshold_c, noise_sqrd its fp32 square; flag 2 where the
 *            threshold is not below the sample type's max_magnitude (walked as two zeros).  auto_noise not 0: urhgpu_batch_noise_dev's
 *            launch runs in front and writes them; the flag protocol of urhgpu_iq_to_bits_batch_auto_dev.
 *   Plan     urhgpu_batch_plan_each (host arithmetic, works without a GPU): urhgpu_batch_plan with tolerance, samples_per_symbol and
 *            bits_per_symbol of each capture's own record (a host copy of the table): region c has the size of that capture's own values.
 *            The launch order holds the ASK captures first, then the FSK captures, each group longest first -- a permutation; a uniform
 *            table gives exactly urhgpu_batch_plan's output.
 *   Pass     urhgpu_iq_to_bits_batch_each_dev: asynchronous on the context's stream, the caller owns all memory, nothing is copied.  n_ask:
 *            the number of ASK records (the first n_ask positions of the launch order).  Launches whatever k, the lengths and the parameter
 *            sets are: ONE walk per modulation present (at most two; modulation is a template parameter of the walk, captures of every
 *            order share a launch), scan, pack -- and one more in front with auto_noise.  The other arguments, the counts, the directory,
 *            the blobs and the truncation protocol are those of urhgpu_iq_to_bits_batch_dev; fetched with urhgpu_batch_fetch (and
 *            urhgpu_batch_noise_fetch).  No load leaves [d_start[c], d_start[c + 1]), no store leaves capture c's region.
 *   Records  urhgpu_batch_msg_records_each_dev: urhgpu_batch_msg_records_dev (no map) behind that pass, three launches: positions from
 *            capture c's samples_per_symbol, bits_per_symbol, pause_threshold and int(samples_per_symbol / bits_per_symbol), the padding to
 *            message_length_divisor only where record c is ASK, the RSSI window [mid_pos, mid_pos + samples_per_symbol_c) clipped at the end
 *            of its OWN capture.  Fetched with urhgpu_batch_records_fetch.
 *   Rejected before anything is launched: a sample type: URHGPU_ERR_DTYPE; a negative size, n_ask outside [0, k], a misaligned pointer, a
 *   missing context or buffer: URHGPU_ERR_ARG.  urhgpu_batch_plan_each: a record outside the ranges above: URHGPU_ERR_ARG, bits_per_symbol
 *   above 7 or a modulation other than ASK / FSK: URHGPU_ERR_UNSUPPORTED.
 * urhgpu_batch_launches counts these launches too. */
typedef struct urhgpu_batch_each {
    int32_t mod;                 /* URHGPU_MOD_ASK or URHGPU_MOD_FSK */
    int32_t bits_per_symbol;     /* 1 .. 7 */
    uint32_t samples_per_symbol; /* >= 1 */
    int32_t tolerance;           /* 0 .. 65535 */
    int64_t pause_threshold;
    float noise_val;             /* 0 for ASK, -4 for FSK */
    int32_t thr_first;           /* the capture's (1 << bits_per_symbol) - 1 thresholds are d_thr[thr_first ..] */
} urhgpu_batch_each;
int urhgpu_batch_plan_each(const int64_t *lengths, int64_t k, const urhgpu_batch_each *each, int policy, int64_t cap_rows_fixed, int64_t *plan,
                           int64_t *work_bytes, int64_t *blob_capacity);
int urhgpu_iq_to_bits_batch_each_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                     const urhgpu_batch_each *d_each, const float *d_thr, int64_t n_thr, int64_t n_ask, int auto_noise, float *d_qad,
                                     void *d_work, int64_t work_bytes, int64_t *d_counts, int64_t *d_dir, void *d_blob, int64_t cap_blob,
                                     urhgpu_noise_result *d_noise);
int urhgpu_batch_msg_records_each_dev(urhgpu_ctx *ctx, const void *d_iq, int64_t total, int dtype, const int64_t *d_start, const int64_t *d_plan, int64_t k,
                                      const urhgpu_batch_each *d_each, int64_t message_length_divisor, const void *d_work, int64_t work_bytes,
                                      const int64_t *d_counts, int64_t *d_rec_dir, void *d_rec, int64_t cap_rec, int32_t *d_rec_capture);

#ifdef __cplusplus
}
#endif
#endif /* URHGPU_H */
