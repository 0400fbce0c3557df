/*
 * fmrx.h -- C ABI of libfmrx.so: the MI355X (gfx950) implementation of the
 * FM-receiver DSP hot path of mnigm2001/Software-Defined-Radio.
 *
 * This header is the drop-in boundary.  The reference has no FFI layer; its
 * operator API for this path is the set of C++ free functions declared in
 * include/filter.h:18-43 and include/iofunc.h:36 (std::vector<float>&
 * arguments), plus the stdin/stdout process contract of src/project.cpp and
 * src/threadMonoOnly.cpp.  Each entry point below names the reference
 * interface it replaces (file:line under /root/reference).  A header-only C++
 * shim (include/fmrx_filter.hpp) re-exposes the exact filter.h signatures on
 * top of this ABI; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - plain pointers + explicit lengths, no C++ or torch types;
 *  - every function returns an fmrx_status (0 = ok); nothing calls exit();
 *    fmrx_last_error() gives the message for the calling thread;
 *  - caller owns every buffer; outputs are caller-allocated to the sizes the
 *    reference's functions resize() to (stated per function);
 *  - "state" buffers are in/out and have exactly the reference's layout;
 *  - the reference's unchecked preconditions (n >= taps-1, n % decim == 0 for
 *    cross-block continuity, taps <= 65535) are validated: FMRX_EINVAL;
 *  - all compute runs on the GPU (HIP kernels).  There is NO CPU fallback:
 *    with no usable device the compute entry points return FMRX_ENODEV.
 *    Only the filter-coefficient design (a3/a4), which is host code in the
 *    reference too and runs once per run, executes on the host;
 *  - functions with a `_dev` suffix take DEVICE pointers and a HIP stream
 *    (passed as void* so this header needs no HIP include) and are
 *    asynchronous on that stream; all others take HOST pointers and are
 *    synchronous (internally H2D -> kernels -> D2H on the current device);
 *  - re-entrant; a pipeline handle is single-owner (not thread-safe), handles
 *    on different devices (= channels) are independent.
 */
#ifndef FMRX_H
#define FMRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define FMRX_API __attribute__((visibility("default")))
#else
#define FMRX_API
#endif

typedef enum fmrx_status {
    FMRX_OK = 0,
    FMRX_EINVAL = 1, /* bad argument / violated precondition */
    FMRX_ENODEV = 2, /* no usable HIP device (never falls back to the CPU) */
    FMRX_EHIP = 3,   /* HIP runtime error */
    FMRX_ENOMEM = 4
} fmrx_status;

/* ------------------------------------------------------------------ */
/* library                                                              */
/* ------------------------------------------------------------------ */
FMRX_API const char *fmrx_version(void);
FMRX_API const char *fmrx_last_error(void);
/* number of HIP devices visible to the process (0 when there is none) */
FMRX_API int fmrx_device_count(void);
/* select the device used by the host-pointer stage functions of this thread */
FMRX_API int fmrx_set_device(int device);

/* Run-time options (reference variants and A/B knobs; none is needed in normal use; any other name is rejected
 * with FMRX_EINVAL).  The process-wide defaults are
 * the built-in values, overridden ONCE, when the library first needs them, by the environment variable
 * FMRX_<NAME IN CAPITALS>; fmrx_set_option changes the defaults afterwards.  A pipeline handle copies the
 * defaults when it is created and keeps its own set (fmrx_pipeline_set_option); the stage functions use the
 * defaults.  Nothing on a per-block path reads the environment.
 * A value outside an option's range is FMRX_EINVAL and changes nothing: the ranges are given below; where none is given, any int
 * (for "fused_min_audio", any long).  An environment value is one of the option's names (=mfma, ...) or a whole base-10 integer
 * and passes the same check; one that does not is ignored with one line on stderr, and the built-in value stays.
 *   "fe_variant"       0 = matrix-core front-end kernels (default; FMRX_FE_VARIANT=mfma), 1 = vector-ALU kernels (=valu)
 *   "fused_min_audio"  audio samples per call from which the fused mono kernel is used (default 65536; 0 = always)
 *   "resample_l2"      1 = the L2-table resampler kernel also for large calls
 *   "resample_exact"   1 = the pipeline's resampler (modes 2/3) keeps the reference's rounding sequence (bit-exact kernels) instead
 *                      of the matrix-core kernel (float32-rounding-equal); the primitive fmrx_resample_fir is always bit-exact
 *   "resample_chains"  workgroups per XCD and tile group of the matrix-core resampler (0 = as many as are resident; A/B)
 *   "overlap_calls"    stereo, modes 0/1: 1 (or 2) = the caller vouches that the INPUT of a fmrx_pipeline_process_dev call is
 *                      complete when the call is made; the stages of consecutive calls then run on internal streams, a call
 *                      apart (1: the next call's front end under this call's PLL and output stage; 2: three lanes).  Outputs
 *                      stay complete in the order of the stream passed to the call; results are bit-identical.  Default 0
 *   "tuner_variant"    wideband tuner: 0 = matrix-core kernel (default; FMRX_TUNER_VARIANT=mfma), 1 = generic kernel (=generic)
 *   "pll_warmup", "pll_segment"               lane shape of the parallel-in-time PLL (-1 = built-in)
 *   "deemph_warmup", "deemph_segment"         lane shape of the parallel-in-time de-emphasis filter (-1 = built-in 256 / 256;
 *                      warm-up 0 .. 2^20, segment 1 .. 2^20): any shape gives the same bits, only the misses change
 *   "deemph_mode"      de-emphasis: 0 = parallel in time (default), 1 = one lane per row, serially (same bits; measurements)
 *   "pll_start"        where the parallel PLL's lanes start: 1 (default) = the locked loop solved as a linear system of the
 *                      input's signs + 64 true steps, 0 = the block's initial state plus drift + 512 true steps
 *   "pll_mode"         stereo PLL of the specialised pipeline: 0 = parallel in time, fast math (default),
 *                      1 = serial, fast math, 2 = serial, glibc's functions (cause-by-cause variants)
 *   "demod"            0 (default; FMRX_DEMOD=discriminator) = the C++ reference's discriminator fmDemod (src/filter.cpp:248-266);
 *                      1 (=arctan) = the Python model's arctangent demodulator fmDemodArctan
 *                      (model/fmSupportLib.py:502-531, float64 atan2 + unwrap): the pipeline
 *                      then runs its unfused kernels (front end -> IF stream -> arctan -> audio / stereo stages) */
FMRX_API int fmrx_set_option(const char *name, long value);
FMRX_API int fmrx_get_option(const char *name, long *value);

/* page-locked host buffers for the block-streaming callers (faster, truly
 * asynchronous H2D/D2H); free with fmrx_host_free.  Plain malloc memory works
 * everywhere too. */
FMRX_API int fmrx_host_alloc(void **out, size_t bytes);
FMRX_API int fmrx_host_free(void *p);

/* ------------------------------------------------------------------ */
/* filter-coefficient API (host, float32 bit-compatible)                */
/* ------------------------------------------------------------------ */
/* replaces impulseResponseLPF  include/filter.h:24, src/filter.cpp:103-114.
 * h[num_taps]. */
FMRX_API int fmrx_impulse_response_lpf(float Fs, float Fc, unsigned short num_taps, float *h);
/* replaces bandPass  include/filter.h:20, src/filter.cpp:83-99.  h[num_taps]. */
FMRX_API int fmrx_band_pass(float Fs, float Fb, float Fe, unsigned short num_taps, float *h);

/* ------------------------------------------------------------------ */
/* stage API on host buffers: one call per reference primitive          */
/* ------------------------------------------------------------------ */
/* replaces readStdinBlockData's conversion  include/iofunc.h:36,
 * src/iofunc.cpp:128-135: out[k] = (raw[k]-128)/128.  out[n]. */
FMRX_API int fmrx_u8_to_f32(const uint8_t *raw, size_t n, float *out);
/* replaces the I/Q split  src/project.cpp:98-105.  I[n_pairs], Q[n_pairs]. */
FMRX_API int fmrx_deinterleave(const float *iq, size_t n_pairs, float *I, float *Q);
/* replaces convolveFIR  include/filter.h:26, src/filter.cpp:118-130.
 * y[n + taps - 1]. */
FMRX_API int fmrx_convolve_fir(float *y, const float *x, size_t n, const float *h, size_t taps);
/* replaces convolveBlockFIR  include/filter.h:28-29, src/filter.cpp:133-154.
 * y[n]; state[taps-1] in/out.  Requires n >= taps-1. */
FMRX_API int fmrx_convolve_block_fir(float *y, const float *x, size_t n, const float *h, size_t taps, float *state);
/* replaces convolveBlockFastFIR  include/filter.h:31-32,
 * src/filter.cpp:158-188.  y[n / decim]; state[taps-1] in/out.
 * Requires n >= taps-1, decim >= 1. */
FMRX_API int fmrx_convolve_block_fast_fir(float *y, const float *x, size_t n, const float *h, size_t taps,
                                          float *state, unsigned decim);
/* replaces convolveBlockResampleFIR  include/filter.h:34-35,
 * src/filter.cpp:191-223.  y[(n*upsamp)/decim]; state[taps-1] in/out in the
 * reference's upsampled index space (slots == upsamp-1 mod upsamp are live).
 * Output gain is (1+upsamp), as in the reference (:213).
 * Requires n*upsamp >= taps-1. */
FMRX_API int fmrx_convolve_block_resample_fir(float *y, const float *x, size_t n, const float *h, size_t taps,
                                              float *state, unsigned decim, unsigned upsamp);
/* replaces upsample / downsample  include/filter.h:37-39,
 * src/filter.cpp:227-245.  xu[n*up];  out[ceil(n/ds)] (count via *n_out). */
FMRX_API int fmrx_upsample(const float *x, size_t n, float *xu, int up);
FMRX_API int fmrx_downsample(float *out, size_t *n_out, const float *in, size_t n, unsigned short ds);
/* replaces fmDemod  include/filter.h:41, src/filter.cpp:248-266.  out[n];
 * *prev_i / *prev_q in/out. */
FMRX_API int fmrx_fm_demod(float *out, const float *I, const float *Q, size_t n, float *prev_i, float *prev_q);
/* the arctangent demodulator of the reference's Python MODEL, fmDemodArctan  model/fmSupportLib.py:502-531 (the C++ receiver
 * uses fmDemod above; BASELINE.json names "arctan/PLL demod"): out[k] = the phase step atan2(Q[k], I[k]) - previous phase,
 * unwrapped into (-pi, pi] by np.unwrap's rule; float64 like the model.  *prev_phase in/out: the model's running (unwrapped)
 * phase.  Within 1e-9 of the model (the model's own rounding of its growing phase is 1e-12; tests/golden/arctan.npz).
 * In a pipeline: option "demod" = 1 (FMRX_DEMOD=arctan) replaces the discriminator by this one. */
FMRX_API int fmrx_fm_demod_arctan(double *out, const double *I, const double *Q, size_t n, double *prev_phase);
/* replaces allPass  include/filter.h:18, src/filter.cpp:14-29 (note the
 * reference's argument order: in, state, out).  out[n]; state[nstate] in/out;
 * requires n >= nstate. */
FMRX_API int fmrx_all_pass(const float *in, size_t n, float *state, size_t nstate, float *out);
/* replaces fmPLL  include/filter.h:22, src/filter.cpp:32-80.  nco_out[n+1];
 * state[6] = {integrator, phaseEst, feedbackI, feedbackQ, lastOut, trigOffset}.
 * Serial recurrence with the reference's float32 operations in its order and the
 * sinf / cosf / atan2f of its C library (glibc 2.35, restated in
 * csrc/glibc_libm.hpp and pinned against it): bit-identical to the reference. */
FMRX_API int fmrx_fm_pll(const float *in, size_t n, float *nco_out, float *state, float freq, float Fs,
                         float ncoScale, float phaseAdjust, float normBandwidth);
/* The pilot PLL as the specialised stereo pipeline runs it (pll_mode 0): parallel in time, fast math -- one lane per segment
 * of L samples started W samples early, seams judged against the merge tolerances, unmerged segments walked again serially
 * (csrc/kernels_pll.hip).  Runs exactly what a warm pipeline's PLL stage runs, with the process-wide options "pll_start",
 * "pll_warmup" and "pll_segment", the serial fast kernel below 4 L samples included; off_hint = IF samples of the stream in
 * front of this call (< 0: unknown), as the pipeline counts them.  nco_out[n+1]; state[6] in/out as fmrx_fm_pll.  The entry
 * owns the kernels' input contract (aligned device input, readable zero floats behind it) and starts from a zeroed work area:
 * no drift record of an earlier call (pll_start 0), diagnostics of this call alone.
 * Optional outputs, for tests and diagnostics (NULL = not wanted), sized for fmrx_pll_parallel_max_segments(n) segments:
 *   records[nseg][FMRX_PLL_RECORD_FLOATS]  per segment: its end state {integrator, phaseEst, feedbackI, feedbackQ, lastOut,
 *                trigOffset}, the (integrator, phaseEst) its outputs were computed from -- the lane's state after its warm-up,
 *                or the predecessor's end state the repair walked it from --, and how many times the repair walked it
 *   mask[nseg / 64 + 1]                    the final mismatch mask, bit s % 64 of word s / 64 = segment s (all zero after a call)
 * info->nseg == 0: the block was shorter than 4 L, the serial kernel ran, records and mask are untouched. */
typedef struct fmrx_pll_parallel_info {
    int L, W;                      /* samples per lane; warm-up samples per lane */
    int lti;                       /* 1 = the lanes started from the linear system's state (pll_start 1, trigArg below 2^22 rad) */
    size_t nseg;                   /* segments */
    unsigned repaired;             /* segment walks of the repair */
    float max_dphase, max_dinteg;  /* largest differences accepted as merged at a seam */
    float tol_phase, tol_integ;    /* the merge tolerances of this call */
} fmrx_pll_parallel_info;
#define FMRX_PLL_RECORD_FLOATS 9
#define fmrx_pll_parallel_max_segments(n) ((size_t)(n) / 32 + 2)
FMRX_API int fmrx_fm_pll_parallel(const float *in, size_t n, float *nco_out, float *state, float freq, float Fs,
                                  float ncoScale, float phaseAdjust, float normBandwidth, double off_hint,
                                  fmrx_pll_parallel_info *info, float *records, uint64_t *mask);
/* replaces the mixer and L/R combine loops  src/project.cpp:246-248, 277-280 */
FMRX_API int fmrx_stereo_mix(const float *stereo_filt, const float *pll, size_t n, float *mixer);
FMRX_API int fmrx_stereo_combine(const float *stereo_final, const float *mono, size_t n, float *left, float *right);
/* replaces the PCM writer's conversion  src/threadMonoOnly.cpp:185-191:
 * NaN -> 0 else (short)(a*16384).  wrap != 0 reproduces the compiled
 * reference on overflow (int32 truncation, low 16 bits); wrap == 0 saturates. */
FMRX_API int fmrx_pcm16(const float *audio, size_t n, int16_t *out, int wrap);

/* ------------------------------------------------------------------ */
/* de-emphasis                                                          */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference (it has no de-emphasis stage).  Coefficients of the one-pole de-emphasis filter for the
 * sample rate fs (Hz) and the time constant tau_us (microseconds: 50 in Europe and Asia, 75 in the Americas and Korea; any
 * value is allowed): the bilinear transform of 1 / (1 + s tau), pre-warped at the corner, in float64, rounded to float32:
 *   k = -tan(1 / (2 fs tau)),  p = (1 + k) / (1 - k),  b0 = (1 - p) / 2        (DC gain 1)
 * Host only: works without a GPU.  FMRX_EINVAL unless fs, tau_us > 0 and 1 / (2 fs tau) < pi / 4 (so that 0 < p < 1). */
FMRX_API int fmrx_deemph_design(double fs, double tau_us, float *p, float *b0);
/* No counterpart in the reference.  The filter on host buffers, rows [rows][pitch] of n samples each (pitch >= n), out of place:
 *   u = x[n] + x_prev;  v = b0 * u;  y = fmaf(p, y_prev, v);  if |y| < 2^-126: y = +0       (float32, per row)
 * state [rows][2] = {x_prev, y_prev}, zeros at the start of a stream, updated.  The device walks it parallel in time -- lanes
 * own segments of `deemph_segment` samples and start `deemph_warmup` samples early from y = 0 (process-wide options; -1 = the
 * built-in 256 / 256), a verify step compares every segment's start with its predecessor's true end and walks the misses
 * again -- with the serial walk's bits whatever the shape; option deemph_mode = 1: one lane per row, serially.  *missed (may
 * be NULL): the segments that were walked again. */
FMRX_API int fmrx_deemph(float *y, const float *x, size_t rows, size_t n, size_t pitch, float p, float b0, float *state,
                         unsigned *missed);
/* No counterpart in the reference.  The same on DEVICE buffers, asynchronous on `stream` (a hipStream_t): d_state [rows][2] is read
 * and left updated, *d_missed (device memory, the caller zeroes it) is incremented by the segments walked again.  The entry point
 * the kernels are measured on (tools/deemph_bench.py). */
FMRX_API int fmrx_deemph_dev(float *d_y, const float *d_x, size_t rows, size_t n, size_t pitch, float p, float b0, float *d_state,
                             unsigned long long *d_missed, void *stream);

/* ------------------------------------------------------------------ */
/* diagnostics                                                          */
/* ------------------------------------------------------------------ */
/* out[i] = sinf(a[i]) (fn 0), cosf(a[i]) (fn 1) or atan2f(a[i], b[i]) (fn 2) as the DEVICE evaluates the
 * restatement of glibc 2.35's functions that fmPLL uses (csrc/glibc_libm.hpp): lets a test compare the
 * device build with the C library of the host, bit for bit.  b may be NULL for fn 0, 1.  fn 3, 4, 5: the same three
 * through the branch-free forms the receiver banks' PLL lanes run (general function where those are not defined).
 * fn 6: out[i] = the hardware reciprocal (v_rcp_f32) of a[i], the one operation of the fast discriminator that a host
 * cannot restate; test hook. */
FMRX_API int fmrx_diag_libm(int fn, const float *a, const float *b, size_t n, float *out);
/* Test hook: the FAST discriminator of the specialised paths (csrc/device_math.hpp) on the caller's own IF.  iq: n interleaved
 * (I, Q) pairs; out[k] from pair k and pair k - 1, out[0] from (prev_i, prev_q).  bounded 0: demod_fast; 1: demod_fast_bounded,
 * whose precondition (every operand 0 or >= 2^-50 in magnitude) is the caller's to keep.  No pipeline calls this. */
FMRX_API int fmrx_diag_demod_fast(float *out, const float *iq, size_t n, float prev_i, float prev_q, int bounded);
/* Measurement aid for bench.py: ONE pure streaming read of a device buffer (>= 3 MiB, 16-byte aligned) by
 * one of the access methods the front-end kernels use -- method 0: non-temporal global loads into
 * registers, 1: LDS-DMA ring, one contiguous run per wave (the fused kernel's pattern), m >= 2: LDS-DMA ring, chunks of
 * m - 1 steps of 3 KiB dealt round-robin over the waves; m | 0x10000 (m >= 1): the same LDS-DMA method with the
 * non-temporal cache policy -- asynchronous on `stream`; the caller times it (what the
 * memory system gives a read-only kernel, next to the nominal 8 TB/s). */
FMRX_API int fmrx_diag_stream_read_dev(const void *d_buf, size_t bytes, int method, void *stream);
/* replaces estimatePSD  include/fourier.h, src/fourier.cpp:44-128 (with its DFT,
 * :15-23): Bartlett average, in dB, of Hann-windowed nfft-point spectra of
 * `samples`; the reference fixes nfft = NFFT = 512 (include/dy4.h:27).
 * freq[nfft/2] (Hz), psd[nfft/2] (dB).  Requires n >= nfft, nfft even. */
FMRX_API int fmrx_estimate_psd(float *freq, float *psd, const float *samples, size_t n, float Fs, int nfft);

/* ------------------------------------------------------------------ */
/* mode table and pipeline handle                                       */
/* ------------------------------------------------------------------ */
/* replaces struct PARAMS + the mode table  src/project.cpp:17-27, 424-427
 * and the block-size rule :55-57 */
typedef struct fmrx_params {
    int mode;         /* 0..3 */
    int rf_Fs, if_Fs; /* Hz */
    float audio_Fs;
    int rf_decim, audio_decim, audio_upsamp; /* upsamp 0 = integer decimation */
    int rf_taps;
    int audio_taps;   /* already multiplied by audio_upsamp for modes 2, 3 */
    int stereo_taps;
    int block_bytes;  /* the reference's per-mode stdin block size */
} fmrx_params;

/* base_audio_taps: 101 (src/threadMonoOnly.cpp:229-232) or 13
 * (src/project.cpp:424-427); rf_taps: 101 / 151 / 13. */
FMRX_API int fmrx_mode_params(int mode, int rf_taps, int base_audio_taps, int stereo_taps, fmrx_params *p);

typedef struct fmrx_pipeline fmrx_pipeline;

/* PCM overflow policy for s16 outputs */
#define FMRX_PCM_WRAP 1     /* what the compiled reference does */
#define FMRX_PCM_SATURATE 0

/* replaces main()'s setup + the RF_FrontEnd / RF_MONO / RF_STEREO thread
 * bodies  src/project.cpp:40-152, 154-309, 311-382, 385-500.
 * channels: 1 mono, 2 stereo.  max_block_bytes: the largest block that will
 * be passed to process (device buffers are sized once, here).  device: HIP
 * device ordinal.  The handle owns all device memory and the carried state
 * (I/Q FIR history, prev I/Q, audio FIR histories, all-pass delay, PLL). */
/* Parameters: any tap counts in 2..65535 and any decimations (the parameter-generic kernels run where no specialised one
 * exists); with a resampler (audio_upsamp > 0) audio_taps must be a multiple of audio_upsamp, FMRX_EINVAL otherwise (and from
 * fmrx_channels_create_ex): the reference writes its resampler state in slots upsamp-1 :: upsamp (src/filter.cpp:218-222) and
 * reads slots taps-1 - d*upsamp (:207), the same slots only when upsamp divides taps -- otherwise its output depends on where
 * the blocks are cut and no stream equals it. */
FMRX_API int fmrx_pipeline_create(fmrx_pipeline **out, const fmrx_params *p, int channels, size_t max_block_bytes,
                                  int device);
FMRX_API int fmrx_pipeline_destroy(fmrx_pipeline *pl);
/* restore the all-zero initial state of src/project.cpp:61-65, 446-458 */
FMRX_API int fmrx_pipeline_reset(fmrx_pipeline *pl);
FMRX_API size_t fmrx_pipeline_n_if(const fmrx_pipeline *pl, size_t n_bytes);
FMRX_API size_t fmrx_pipeline_n_audio(const fmrx_pipeline *pl, size_t n_bytes);

/* One block, host buffers: iq[n_bytes] interleaved u8 I,Q (the stdin format,
 * src/iofunc.cpp:128-135) -> audio.  Any of the outputs may be NULL.
 *   audio_f32 : mono [n_audio], or stereo left then right planar [2*n_audio]
 *   pcm16     : mono [n_audio], or stereo interleaved L,R [2*n_audio]
 *               (the layout of the writer at src/project.cpp:292-302)
 * n_bytes must satisfy the reference's divisibility rules for the mode
 * (n_bytes/2 % rf_decim == 0, n_if % audio_decim == 0 or
 * n_if*upsamp % decim == 0) and n_bytes/2 >= rf_taps-1. */
FMRX_API int fmrx_pipeline_process(fmrx_pipeline *pl, const uint8_t *iq, size_t n_bytes, float *audio_f32,
                                   int16_t *pcm16, int pcm_policy);
/* The same call in two halves, for block-streaming callers that want the PCIe copies of one block under the kernels of its
 * neighbours: submit enqueues one block (copy in, kernels, copy out) and returns; wait blocks until the OLDEST submitted block's
 * outputs are complete in the host buffers passed to its submit.  At most two blocks are in flight (a third submit waits
 * for the oldest first).  Buffers must stay valid until their block has been waited for; page-locked buffers (fmrx_host_alloc)
 * make the copies truly asynchronous.  fmrx_pipeline_process = submit + wait.  Results are identical to the synchronous calls'. */
FMRX_API int fmrx_pipeline_submit(fmrx_pipeline *pl, const uint8_t *iq, size_t n_bytes, float *audio_f32, int16_t *pcm16,
                                  int pcm_policy);
FMRX_API int fmrx_pipeline_wait(fmrx_pipeline *pl);
/* Same, device-resident: d_iq is DEVICE memory (16-byte aligned), outputs are
 * DEVICE memory or NULL; asynchronous on `stream` (a hipStream_t).  This is
 * the entry point the throughput figures are measured on.  (With option
 * "overlap_calls" the input must be complete at the call, not merely ordered
 * in front of it on `stream`: see the options above.) */
FMRX_API int fmrx_pipeline_process_dev(fmrx_pipeline *pl, const uint8_t *d_iq, size_t n_bytes, float *d_audio_f32,
                                       int16_t *d_pcm16, int pcm_policy, void *stream);
/* Copies of the last block's device intermediates to host, for parity tests
 * and diagnostics.  which: see FMRX_TAP_*.  out may be NULL to query *n. */
#define FMRX_TAP_IF_I 0
#define FMRX_TAP_IF_Q 1
#define FMRX_TAP_DEMOD 2
#define FMRX_TAP_MONO 3
#define FMRX_TAP_CARRIER 4
#define FMRX_TAP_STEREO_BPF 5
#define FMRX_TAP_PLL 6
#define FMRX_TAP_MIXER 7
#define FMRX_TAP_STEREO_FINAL 8
/* fast stereo banks, modes 0 and 1 only: the raw trigArg of every PLL step of the last call (n_if values; the output stage
 * takes the NCO's cosine of it on chip).  Pipelines and every other bank refuse it (FMRX_EINVAL). */
#define FMRX_TAP_TRIG_ARG 9
FMRX_API int fmrx_pipeline_read_tap(fmrx_pipeline *pl, int which, float *out, size_t *n);
/* carried state, serialised: floats in the order
 *   I_state[rf_taps-1], Q_state[rf_taps-1], prev_i, prev_q, state_mono[Ha]
 *   (+ stereo: state_stereo[St-1], state_carrier[St-1], state_stereofilt[Ha],
 *    state_allpass[(St-1)/2], state_PLL[6])
 * where Ha = audio history in INPUT samples (audio_taps-1, or
 * (audio_taps-1)/upsamp for modes 2,3: the live slots upsamp-1 :: upsamp of the reference's upsampled-space vectors).
 * n = number of floats.  The handle keeps ONE discriminator history, of which state_stereo, state_carrier (the same samples),
 * state_allpass (their last (St-1)/2) and state_mono (the Ha samples in front of those) are windows; get_state writes them all.
 * set_state returns FMRX_EINVAL and leaves the handle unchanged for a wrong n, an I_state / Q_state value that is not
 * (u8-128)/128, or windows that disagree where they overlap (a state no stream produces).  A handle resumed from get_state
 * continues bit for bit, whatever it had processed before, wherever the receiver is deterministic: mono, and stereo with the
 * serial PLL (set_force_generic, pll_mode 1 or 2); the default parallel PLL re-acquires (within its usual bounds). */
FMRX_API size_t fmrx_pipeline_state_size(const fmrx_pipeline *pl);
FMRX_API int fmrx_pipeline_get_state(fmrx_pipeline *pl, float *state, size_t n);
FMRX_API int fmrx_pipeline_set_state(fmrx_pipeline *pl, const float *state, size_t n);
/* wall-clock free: device time of the kernels of the last process call, ms,
 * per stage (HIP events on the pipeline's stream).  t[4] = {front_end, audio,
 * stereo_extra, total}. */
FMRX_API int fmrx_pipeline_last_timing(fmrx_pipeline *pl, float *t);
/* sums of the same four figures over the most recent profiled calls (at most
 * max_calls, at most the 128 the handle keeps); *count = calls summed */
FMRX_API int fmrx_pipeline_timing_sum(fmrx_pipeline *pl, float *t, int *count, int max_calls);
/* per-stage HIP events behind last_timing / timing_sum: 0 = off, 1 = around every process call,
 * k > 1 = around every k-th call (an event record costs a few microseconds of stream time) */
FMRX_API int fmrx_pipeline_set_profiling(fmrx_pipeline *pl, int on);
/* The front-end kernels consume the IF I/Q samples in registers, and the fused
 * mono kernel (modes 0/1, one channel, large blocks) the discriminator output
 * too: neither is written to memory.  on = 1 selects the kernels that store
 * them, so that FMRX_TAP_IF_I / FMRX_TAP_IF_Q / FMRX_TAP_DEMOD can be read
 * after a process call (diagnostics and tests; default 0; read_tap returns
 * FMRX_EINVAL for a tap that was not stored). */
FMRX_API int fmrx_pipeline_set_keep_intermediates(fmrx_pipeline *pl, int on);
/* Stereo only.  In the specialised pipeline the pilot PLL (fmPLL, src/filter.cpp:32-80) runs parallel
 * in time (segments with warm-up, checked against the neighbouring segment within a tolerance, serial
 * repair where the loop was not locked); it agrees with the serial recurrence to within the float32
 * grid of its phase argument, not bit for bit (see set_force_generic for the bit-exact mode).  Cumulative since creation: segment walks
 * of the serial repair (a repaired segment whose predecessor is repaired again with another result is walked again
 * and counts each time), and the largest phase / integrator difference
 * accepted as "merged" at a segment boundary, by the lanes' first judging or after a repair. */
FMRX_API int fmrx_pipeline_pll_diagnostics(fmrx_pipeline *pl, unsigned *repaired_segments, float *max_dphase,
                                           float *max_dinteg);
/* force the parameter-generic kernels (1) or allow the specialised ones (0).  on = 1 is the BIT-EXACT
 * mode: every stage keeps the reference's float32 evaluation order and fmPLL runs as the serial
 * recurrence with glibc's functions, so mono AND stereo audio equal the reference's bit for bit for
 * any stream length (the specialised kernels reorder sums, i.e. differ by ulps, which the stereo
 * recurrence amplifies to its float32 phase grid: DESIGN.md section 2). */
FMRX_API int fmrx_pipeline_set_force_generic(fmrx_pipeline *pl, int on);
/* per-handle run-time option, names as for fmrx_set_option */
FMRX_API int fmrx_pipeline_set_option(fmrx_pipeline *pl, const char *name, long value);
/* No counterpart in the reference.  De-emphasis of the audio outputs (fmrx_deemph at the handle's audio_Fs): tau_us = 0 turns it
 * off, which is the default -- the call then launches exactly the kernels it launches without this entry point.  With it on,
 * the producing stage writes float32 rows of the handle's own (channels * the largest call's n_audio floats, allocated when it is
 * first turned on, and as many again for callers that take PCM only) and one more pass writes audio_f32 and / or pcm16; every tap
 * (FMRX_TAP_MONO among them) keeps showing the signal in front of it.  Turning it on or changing tau zeroes the filter's state,
 * and so does fmrx_pipeline_reset.  While it is on, fmrx_pipeline_state_size / get_state / set_state carry {x_prev, y_prev} per
 * audio channel, appended at the end. */
FMRX_API int fmrx_pipeline_set_deemphasis(fmrx_pipeline *pl, double tau_us);
/* No counterpart in the reference.  Cumulative since creation: segments the verify step has checked (every segment of a call but
 * each row's first, which is exact) and how many of them were walked again (either may be NULL). */
FMRX_API int fmrx_pipeline_deemph_diagnostics(fmrx_pipeline *pl, unsigned long long *segments, unsigned long long *missed);

/* ------------------------------------------------------------------ */
/* many mono channels per device call                                   */
/* ------------------------------------------------------------------ */
/* The reference runs one receiver per process (one PARAMS / STATES set, src/project.cpp:460-468); a bank of N
 * receivers is N processes.  fmrx_channels processes the current block of N independent channels in one call
 * (fmrx_channels_create: mono, modes 0 and 1, ONE kernel launch; fmrx_channels_create_ex below: mono or stereo, exact or fast): what a live multi-channel receiver needs, where one 51 200-sample block per
 * channel and launch would leave the chip idle.  A channel's whole carried state is its last ~1 200 input
 * samples, kept as raw bytes in front of its block (csrc/bank.hip); results equal fmrx_pipeline's for the
 * same stream (audio to within float32 summation order, <= 2e-6; PCM +-1 LSB).
 *   block_bytes: bytes per channel and call (a multiple of 16 and of 2*rf_decim*audio_decim; the reference's
 *   p->block_bytes qualifies).  Input: either host memory, channel-major [n_channels][block_bytes]
 *   (fmrx_channels_process), or written by the caller straight into device memory: channel c's block goes to
 *   d_first_block + c*pitch_bytes (fmrx_channels_input_layout), then fmrx_channels_process_dev.
 *   Output: [n_channels][n_audio] float and/or s16, n_audio = fmrx_channels_n_audio(). */
typedef struct fmrx_channels fmrx_channels;
FMRX_API int fmrx_channels_create(fmrx_channels **out, const fmrx_params *p, int n_channels, size_t block_bytes, int device);
/* The same bank with the two choices the reference's command line has (src/project.cpp:390-419: <mode> <channels>) and the
 * numerics mode spelled out:
 *   audio_channels  1 = mono (RF_MONO, src/project.cpp:311-382), 2 = stereo (RF_STEREO, :154-309)
 *   exact           1 = every stage in the reference's float32 evaluation order and fmPLL (src/filter.cpp:32-80) as the
 *                   serial recurrence with glibc's sinf / cosf / atan2f, ONE LANE PER CHANNEL (64 receivers per wave):
 *                   audio is the compiled reference's bit for bit, per channel, for any stream length.  This is the way
 *                   to run stereo within the 1e-4 bound at speed: the recurrence cannot be cut in time without leaving
 *                   the reference's trajectory, but receivers are independent (one STATES set
 *                   each, src/project.cpp:455-468).
 *                   0 = the specialised kernels: mono, fmrx_channels_create's bank (modes 0, 1: one fused kernel); stereo, the matrix-core front end, one fused
 *                   multiply-add per tap in the band-pass pair and the audio FIRs, and the PLL's fast recurrence (closed-form phase
 *                   detector, hardware sine / cosine) walked by one lane per channel -- the error bound of the default
 *                   single-stream stereo path (1e-4 for a stream's first 0.13 s, 0.06 ulp(trigArg(t)) after; mono sum 2e-6)
 *                   at several times the exact bank's rate.
 * Modes: exact banks cover all four modes (0, 1 integer decimation; 2, 3 the rational resampler convolveBlockResampleFIR,
 * src/filter.cpp:191-223, in its own evaluation order; a block must then end on an output boundary: n_if * upsamp % decim == 0,
 * as the reference's own block sizes do), and so do the fast banks: in modes 2 and 3 they run the matrix-core front end (stereo: the fast
 * band-pass pair and PLL) in front of the same batched resampler (mono, exact = 0, modes 2 / 3: audio within 2e-6 of the reference).
 * Outputs: audio_f32 [n_channels][audio_channels][n_audio] (stereo: left, then right), pcm16
 * [n_channels][n_audio][audio_channels] (stereo: interleaved L,R as the writer at src/project.cpp:292-302). */
FMRX_API int fmrx_channels_create_ex(fmrx_channels **out, const fmrx_params *p, int n_channels, int audio_channels, int exact,
                                     size_t block_bytes, int device);
/* one channel's intermediates of the last call, kept by every bank but the fused mono bank of modes 0/1 (fmrx_channels_create's;
 * FMRX_EINVAL): FMRX_TAP_DEMOD; stereo banks also FMRX_TAP_STEREO_BPF, _PLL [n_if + 1] and _CARRIER (exact banks: the pilot
 * band-pass output; fast banks: its sign as the PLL reads it, -1 / 0 / +1), fast banks of modes 0/1 also _TRIG_ARG */
FMRX_API int fmrx_channels_read_tap(fmrx_channels *c, int channel, int which, float *out, size_t *n);
FMRX_API int fmrx_channels_destroy(fmrx_channels *c);
FMRX_API size_t fmrx_channels_n_audio(const fmrx_channels *c);
FMRX_API int fmrx_channels_input_layout(const fmrx_channels *c, uint8_t **d_first_block, size_t *pitch_bytes);
/* back to the start-of-stream state: one channel, or all of them (channel < 0) */
FMRX_API int fmrx_channels_reset(fmrx_channels *c, int channel);
/* device-resident channel-major blocks [n_channels][block_bytes] -> the slots (one strided device copy, async on `stream`) */
FMRX_API int fmrx_channels_load_dev(fmrx_channels *c, const uint8_t *d_iq, void *stream);
FMRX_API int fmrx_channels_process(fmrx_channels *c, const uint8_t *iq, float *audio_f32, int16_t *pcm16, int pcm_policy);
FMRX_API int fmrx_channels_process_dev(fmrx_channels *c, float *d_audio_f32, int16_t *d_pcm16, int pcm_policy, void *stream);
/* No counterpart in the reference.  De-emphasis for every bank flavour (fused mono, exact and fast, mono and stereo, all modes), as
 * fmrx_pipeline_set_deemphasis: tau_us = 0 = off (default).  With it on, the bank's output stage writes a float32 buffer of the
 * handle's own, [n_channels][audio_channels][n_audio] -- 4 * n_channels * audio_channels * n_audio bytes, allocated when it is first
 * turned on, and as many again for callers that take PCM only -- and one pass over its n_channels * audio_channels rows, after
 * the bank's streams have joined, writes the caller's arrays.  fmrx_channels_reset(c, ch) zeroes that channel's rows only. */
FMRX_API int fmrx_channels_set_deemphasis(fmrx_channels *c, double tau_us);
FMRX_API int fmrx_channels_deemph_diagnostics(fmrx_channels *c, unsigned long long *segments, unsigned long long *missed);

/* ------------------------------------------------------------------ */
/* RDS path                                          */
/* ------------------------------------------------------------------ */
/* The reference has this path only as a float64 Python / NumPy model: model/fmMonoBlock.py:238-296 on top of
 * model/fmSupportLib.py (it never reached its C++).  Here: float64 HIP kernels for the signal chain -- 54-60 kHz channel
 * band-pass, squarer + 114 kHz band-pass, PLL (ncoScale 0.5, phaseAdjust 3pi/8, bandwidth 0.002), I/Q mixers, rational
 * resampler to sps x 2375 Hz, root-raised-cosine matched filter -- and host C++ for the bit recovery the model does in
 * Python (CDR, Manchester, differential decoding, frame synchronisation).  Input: the discriminator output (fm_demod) of
 * the front end, one block per call, state carried by the handle. */
typedef struct fmrx_rds_params {
    int if_Fs;    /* rate of fm_demod, Hz */
    int taps;     /* band-pass filters: 151 (model/fmMonoBlock.py:114) */
    int upsamp, decim; /* resampler: 247/960 (mode 0), 817/1920 (mode 2) (:74-75, :83-84) */
    int sps;      /* samples per symbol at the resampler output: 26 / 43 */
    int rrc_taps; /* 101 */
} fmrx_rds_params;
typedef struct fmrx_rds fmrx_rds;
FMRX_API int fmrx_rds_mode_params(int mode, fmrx_rds_params *p);   /* the model defines RDS rates for modes 0 and 2 */
FMRX_API int fmrx_rds_create(fmrx_rds **out, const fmrx_rds_params *p, size_t max_block, int device);
FMRX_API int fmrx_rds_destroy(fmrx_rds *r);
FMRX_API int fmrx_rds_reset(fmrx_rds *r);
FMRX_API size_t fmrx_rds_n_out(const fmrx_rds *r, size_t n);   /* n*upsamp/decim */
/* One block of fm_demod (host, n samples; n*upsamp % decim == 0) -> rrc_i / rrc_q [n_out] (matched-filter output, in-phase
 * and quadrature; either may be NULL), bits [<= n_out/sps + 2] = the differentially decoded bits of this block, *n_bits,
 * offset_type [8] = the last offset word the frame synchroniser recognised over the bits kept so far ("A", "B", "C",
 * "C_apos", "D" or " "), exactly as model/fmMonoBlock.py:276-297 reports them per block. */
FMRX_API int fmrx_rds_process(fmrx_rds *r, const float *fm_demod, size_t n, double *rrc_i, double *rrc_q, uint8_t *bits,
                              size_t *n_bits, char *offset_type);
/* the signal chain only, on a device-resident fm_demod (e.g. the pipeline's FMRX_TAP_DEMOD buffer); async on `stream` */
FMRX_API int fmrx_rds_process_dev(fmrx_rds *r, const float *d_demod, size_t n, void *stream);
#define FMRX_RDS_TAP_CHANNEL 0
#define FMRX_RDS_TAP_CARRIER 1
#define FMRX_RDS_TAP_PLL_I 2
#define FMRX_RDS_TAP_PLL_Q 3
#define FMRX_RDS_TAP_RESAMPLED_I 4
#define FMRX_RDS_TAP_RRC_I 5
#define FMRX_RDS_TAP_RRC_Q 6
#define FMRX_RDS_TAP_PLL_STATE 7
FMRX_API int fmrx_rds_read_tap(fmrx_rds *r, int which, double *out, size_t *n);
/* the model's primitives on host buffers (float64): bandPass / impResponse (fmSupportLib.py:358, 376; Python argument
 * order taps, Fs, ...), impulseResponseRootRaisedCosine (:251), CDR incl. Manchester decoding (:103-219; state4 =
 * {pair[0], pair[1], start, prev_size} in/out), diff_decoding (:241), framesync (:30-100) */
FMRX_API int fmrx_rds_band_pass(int taps, double Fs, double Fb, double Fe, double *h);
FMRX_API int fmrx_rds_imp_response(int taps, double Fs, double Fc, double *h);
FMRX_API int fmrx_rds_rrc(double Fs, int taps, double *h);
FMRX_API int fmrx_rds_cdr(const double *x, size_t n, int sps, int block_count, double *state4, uint8_t *bits, size_t *n_bits);
FMRX_API int fmrx_rds_diff_decode(const uint8_t *in, size_t n, uint8_t *out);
FMRX_API int fmrx_rds_frame_sync(const uint8_t *bits, size_t n, char *offset_type, size_t *next_index);

/* ------------------------------------------------------------------ */
/* RDS station decoder: PI, PTY, PS name, RadioText                     */
/* ------------------------------------------------------------------ */
/* Next to the model-faithful bit recovery above (which restarts every block and so never carries an RDS group across calls):
 * a decoder whose chip timing, Manchester pairing, differential decoding and block sync carry across calls, on the in-phase
 * matched-filter row that fmrx_rds_process returns (rrc_i), then groups (IEC 62106: 0A/0B PS name, TA, MS; 2A/2B RadioText;
 * PI, PTY, TP from every group) into a station record.  Algorithm and constants: rds_station.hpp.  The host decoder below and
 * the RDS bank's stations (fmrx_rds_bank_set_stations) compute the same records byte for byte.  The host decoder is host code
 * (one station's ~2 400 samples per 40 ms call). */
typedef struct fmrx_rds_station {
    uint16_t pi;          /* programme identification (block A, or C' of version-B groups) */
    uint8_t pty, tp;      /* programme type, traffic programme (block B) */
    uint8_t ta, ms;       /* traffic announcement, music / speech (group 0) */
    uint8_t synced;       /* block sync held at the end of the last call */
    uint8_t seen;         /* bit 0: PI decoded, bit 1: PTY / TP decoded */
    uint8_t ps_mask;      /* PS segments (2 characters each) received */
    uint8_t rt_ab;        /* RadioText A/B flag of the text held; 2 = no group 2 yet */
    uint16_t rt_mask;     /* RadioText segments received (2A: 4 characters each, 2B: 2) */
    uint32_t blocks;      /* blocks checked while synced */
    uint32_t good_blocks; /* of which passed their syndrome */
    uint32_t groups;      /* groups assembled */
    char ps[8];           /* programme service name, spaces where not yet received (not NUL-terminated) */
    char rt[64];          /* RadioText, spaces where not yet received; cleared when the A/B flag changes */
} fmrx_rds_station;
typedef struct fmrx_rds_group {
    uint16_t block[4];    /* information words of slots A, B, C/C', D (0 where the slot failed) */
    uint8_t ok_mask;      /* bit s: slot s passed its syndrome; bit 4: slot 2 carried offset C' */
    uint8_t reserved[3];  /* [0]: corrected mask, bit s: slot s passed after burst error correction (0 with correction off);
                             [1], [2]: 0 */
    uint32_t bit_index;   /* index of the group's first bit in the decoder's bit stream (mod 2^32) */
} fmrx_rds_group;
/* The extension record: what burst error correction did, and the station data beyond PS and RadioText (IEC 62106 groups 0A
 * alternative frequencies, 0A/0B decoder identification, 1A country code / language / programme item number, 4A clock time,
 * 10A programme type name).  Rules: rds_station.hpp.  A fresh record is all zeros but ptyn (spaces), ptyn_ab (2) and
 * max_burst (the option). */
typedef struct fmrx_rds_station_ext {
    uint32_t corrected_blocks; /* blocks accepted after correction (a subset of fmrx_rds_station.good_blocks) */
    uint32_t burst_hist[5];    /* of which with a burst of length 1..5 */
    uint32_t sync_losses;      /* times block sync was lost */
    uint32_t group_types;      /* bit 2*type + version (A 0, B 1): a group of that type arrived with block B passed */
    uint32_t af_bits[8];       /* alternative frequencies (0A): bit c of the 256-bit set = code c = 87.5 + 0.1 c MHz, c in 1..204 */
    uint32_t ct_mjd;           /* clock time (4A), the last valid one: modified Julian day (17 bits) */
    uint32_t ct_bit_index;     /* bit_index of the group that carried it: the minute's edge in the bit stream */
    uint32_t ct_count;         /* 4A groups accepted (B, C and D passed, hour < 24, minute < 60) */
    char ptyn[8];              /* programme type name (10A), spaces where not yet received; cleared when its A/B flag changes */
    uint16_t pin;              /* programme item number (1A block D), raw */
    uint16_t lang;             /* language code (1A variant 3), 12 bits */
    uint8_t ecc;               /* extended country code (1A variant 0) */
    uint8_t ext_seen;          /* bit 0: ecc valid, bit 1: lang valid, bit 2: pin valid */
    uint8_t max_burst;         /* the correction option the decoder runs with, 0..5 */
    uint8_t di;                /* decoder identification (0A/0B): bit 3 = d3 ... bit 0 = d0 */
    uint8_t di_mask;           /* which of its bits have been received */
    uint8_t af_announced;      /* number of alternative frequencies the station announces (code 224 + n), 0..25 */
    uint8_t ct_hour;           /* UTC hour 0..23 */
    uint8_t ct_minute;         /* 0..59 */
    uint8_t ct_offset;         /* local time offset, raw: bit 5 = sign (1: negative), bits 4..0 = half hours */
    uint8_t ptyn_mask;         /* PTYN segments (4 characters each) received */
    uint8_t ptyn_ab;           /* A/B flag of the name held; 2 = no group 10A yet */
    uint8_t reserved[29];      /* 0 */
} fmrx_rds_station_ext;
#ifdef __cplusplus
static_assert(sizeof(fmrx_rds_station) == 96, "fmrx_rds_station layout");
static_assert(sizeof(fmrx_rds_group) == 16, "fmrx_rds_group layout");
static_assert(sizeof(fmrx_rds_station_ext) == 128, "fmrx_rds_station_ext layout");
#else
_Static_assert(sizeof(fmrx_rds_station) == 96, "fmrx_rds_station layout");
_Static_assert(sizeof(fmrx_rds_group) == 16, "fmrx_rds_group layout");
_Static_assert(sizeof(fmrx_rds_station_ext) == 128, "fmrx_rds_station_ext layout");
#endif
typedef struct fmrx_rds_station_decoder fmrx_rds_station_decoder;
/* sps: matched-filter samples per chip, 2..64 (fmrx_rds_params.sps: 26 in mode 0, 43 in mode 2) */
FMRX_API int fmrx_rds_station_create(fmrx_rds_station_decoder **out, int sps);
FMRX_API int fmrx_rds_station_destroy(fmrx_rds_station_decoder *d);
FMRX_API int fmrx_rds_station_reset(fmrx_rds_station_decoder *d);
/* Upper bound of the groups one feed_rrc of n_samples can produce (feed_bits of n bits: 2*(n/26 + 1)). */
FMRX_API size_t fmrx_rds_station_max_groups(const fmrx_rds_station_decoder *d, size_t n_samples);
/* One call's rrc_i [n] -> the groups completed in it (g [max_g]; groups beyond max_g are counted in st->groups but not
 * stored), *n_g, and the station record after it (st).  g / n_g may be NULL together. */
FMRX_API int fmrx_rds_station_feed_rrc(fmrx_rds_station_decoder *d, const double *rrc_i, size_t n, fmrx_rds_group *g, size_t max_g,
                                       size_t *n_g, fmrx_rds_station *st);
/* The same from differentially decoded bits (0 / 1): block sync and groups alone. */
FMRX_API int fmrx_rds_station_feed_bits(fmrx_rds_station_decoder *d, const uint8_t *bits, size_t n, fmrx_rds_group *g, size_t max_g,
                                        size_t *n_g, fmrx_rds_station *st);
/* Burst error correction (IEC 62106 annex B: the (26,16) code repairs any one burst of up to 5 bits): max_burst 0..5 = the
 * longest burst a block that failed its syndrome while sync is held may be repaired from; 0 (the default) = none.  One wrong
 * chip pair on the air is a 2-bit burst after differential decoding; 2 is the recommended setting.  A word of 26 random bits
 * is taken for a block with probability (correctable syndromes + 1) / 1024: 0.1 % at 0, 2.6 % at 1, 5.1 % at 2, 9.8 % at 3,
 * 18.8 % at 4, 35.9 % at 5.  Only on a decoder that has been fed nothing since create or reset: FMRX_EINVAL otherwise.  The
 * option outlives fmrx_rds_station_reset. */
FMRX_API int fmrx_rds_station_set_correction(fmrx_rds_station_decoder *d, int max_burst);
/* The extension record as of the last feed. */
FMRX_API int fmrx_rds_station_ext_get(const fmrx_rds_station_decoder *d, fmrx_rds_station_ext *ext);
/* One block on its own: word26 = 26 bits, first received in bit 25; offset 0 A, 1 B, 2 C, 3 C', 4 D.  -> 0 clean, 1 corrected
 * (a burst of *burst_len <= max_burst bits), 2 uncorrectable, -1 bad argument.  *info: the information word (of the repaired
 * block where corrected; of the word as received where uncorrectable).  info / burst_len may be NULL. */
FMRX_API int fmrx_rds_block_correct(uint32_t word26, int offset, int max_burst, uint16_t *info, int *burst_len);

/* ------------------------------------------------------------------ */
/* RDS banks: the RDS chain of N channels per device call               */
/* ------------------------------------------------------------------ */
/* fmrx_rds for N independent stations at once, in a fixed number of kernel launches per call whatever N: the float64 chain
 * with one lane per channel for its PLL, clock and data recovery on the device (one lane per channel), frame synchronisation on
 * the host.  Per channel every result equals, bit for bit, what an fmrx_rds handle reports for the same discriminator stream.
 * Rows are channel-major.
 *   block: IF samples per channel and call; block*upsamp % decim == 0 and block >= every history (as fmrx_rds_process_dev).
 *   9 600 IF samples (block_bytes 192 000 of a receiver bank) serve both RDS modes and the banks of modes 0 and 2.
 * Every frame-sync report depends on the bits of every earlier call: a second process_dev (or a reset) before the previous
 * call's collect returns FMRX_EINVAL; bits are never dropped. */
typedef struct fmrx_rds_bank fmrx_rds_bank;
FMRX_API int fmrx_rds_bank_create(fmrx_rds_bank **out, const fmrx_rds_params *p, int n_channels, size_t block, int device);
FMRX_API int fmrx_rds_bank_destroy(fmrx_rds_bank *b);
FMRX_API int fmrx_rds_bank_reset(fmrx_rds_bank *b, int channel);            /* channel < 0: all */
FMRX_API size_t fmrx_rds_bank_n_out(const fmrx_rds_bank *b);               /* block*upsamp/decim */
FMRX_API size_t fmrx_rds_bank_max_bits(const fmrx_rds_bank *b);            /* per channel and call */
/* device rows: channel c's block at d_demod + c*pitch (floats); async on `stream` */
FMRX_API int fmrx_rds_bank_process_dev(fmrx_rds_bank *b, const float *d_demod, size_t pitch, void *stream);
/* waits for the last process_dev; rrc_i / rrc_q [n_channels][n_out] (either may be NULL), bits [n_channels][max_bits],
 * n_bits [n_channels], offset_type [n_channels][8]: per channel exactly what fmrx_rds_process reports */
FMRX_API int fmrx_rds_bank_collect(fmrx_rds_bank *b, double *rrc_i, double *rrc_q, uint8_t *bits, size_t *n_bits,
                                   char *offset_type);
/* host rows [n_channels][block]: H2D + process_dev + collect */
FMRX_API int fmrx_rds_bank_process(fmrx_rds_bank *b, const float *demod, double *rrc_i, double *rrc_q, uint8_t *bits,
                                   size_t *n_bits, char *offset_type);
FMRX_API int fmrx_rds_bank_read_tap(fmrx_rds_bank *b, int channel, int which, double *out, size_t *n);  /* FMRX_RDS_TAP_* */
/* Stations: one station decoder per channel (rds_station.hpp) as a kernel of process_dev, one lane per channel on the
 * matched-filter row; records stay on the device until fmrx_rds_bank_stations.  Off by default (a bank then runs exactly the
 * kernels it runs without this); on / off only before the first call or right after fmrx_rds_bank_reset(b, -1).  With stations
 * on, either fmrx_rds_bank_stations or fmrx_rds_bank_collect takes the last call off the "not collected" rule, and collect's
 * frame-sync report covers the bits of the calls it saw.  fmrx_rds_bank_reset(b, c) clears channel c's decoder too. */
FMRX_API int fmrx_rds_bank_set_stations(fmrx_rds_bank *b, int on);
/* groups per channel one call can produce: the row length of g below */
FMRX_API size_t fmrx_rds_bank_max_groups(const fmrx_rds_bank *b);
/* waits for the last process_dev; st [n_channels] (required), g [n_channels][max_groups] and n_g [n_channels] (both or neither):
 * every channel's station record and the groups its last call completed, exactly what an fmrx_rds_station_decoder fed the
 * channel's rrc_i rows produces */
FMRX_API int fmrx_rds_bank_stations(fmrx_rds_bank *b, fmrx_rds_station *st, fmrx_rds_group *g, size_t *n_g);
/* Options of the bank's station decoders: max_burst as fmrx_rds_station_set_correction; ext != 0 keeps an extension record
 * per channel on the device.  Only with stations on and under the rule of fmrx_rds_bank_set_stations (before the first call
 * or right after fmrx_rds_bank_reset(b, -1)).  A bank on which this was never called runs what it ran before it existed. */
FMRX_API int fmrx_rds_bank_set_station_options(fmrx_rds_bank *b, int max_burst, int ext);
/* waits for the last process_dev as fmrx_rds_bank_stations does (and takes it off the "not collected" rule likewise);
 * ext [n_channels]: exactly what fmrx_rds_station_ext_get reports for a host decoder with the same option fed the channel's
 * rrc_i rows.  FMRX_EINVAL when the extension records are off.  fmrx_rds_bank_reset(b, c) clears channel c's record too. */
FMRX_API int fmrx_rds_bank_stations_ext(fmrx_rds_bank *b, fmrx_rds_station_ext *ext);
/* Receiver banks that keep discriminator rows (stereo banks, exact banks, the resampling modes' banks): where the last
 * call's rows are, for fmrx_rds_bank_process_dev on the same stream.  FMRX_EINVAL for the fused mono bank of modes 0/1.
 * A call leaves its rows intact (only the history in front of each row is rewritten) until the next fmrx_channels_process*;
 * the bank forks from and joins back into the caller's stream, so work enqueued on that stream after
 * fmrx_channels_process_dev sees finished rows.  n_if = block_bytes / (2*rf_decim): the RDS bank's block. */
FMRX_API int fmrx_channels_demod_layout(const fmrx_channels *c, const float **d_row0, size_t *pitch, size_t *n_if);

/* ------------------------------------------------------------------ */
/* fused front end (the hot kernel) as a stage of its own               */
/* ------------------------------------------------------------------ */
/* Fused: u8 I/Q -> (u8-128)/128 -> rf low-pass FIR -> decimate, I and Q
 * together.  Replaces readStdinBlockData's conversion (src/iofunc.cpp:133),
 * the I/Q split (src/project.cpp:98-105) and the two convolveBlockFastFIR
 * calls of RF_FrontEnd (src/project.cpp:111,121; src/filter.cpp:158-188).
 *
 * Host buffers, synchronous:
 *   iq[2*n_samples]   interleaved u8 I,Q
 *   hist              in/out, 2*(taps-1) bytes: the taps-1 complex samples that
 *                     precede the block (the reference's I_state/Q_state, kept
 *                     as raw u8); NULL = start of stream (silence), no carry
 *   if_i, if_q        out, n_samples/decim floats each (either may be NULL)
 * force_generic != 0 runs the parameter-generic kernel (reference evaluation
 * order, bit-compatible) instead of the specialised one. */
FMRX_API int fmrx_fe_fir_decim_u8(const uint8_t *iq, size_t n_samples, const float *h, size_t taps, unsigned decim,
                                  uint8_t *hist, float *if_i, float *if_q, int force_generic);

/* Device buffers, asynchronous on a HIP stream: a reusable plan holds the tap
 * tables on the device. */
typedef struct fmrx_fe_plan fmrx_fe_plan;
FMRX_API int fmrx_fe_plan_create(fmrx_fe_plan **out, const float *h, size_t taps, unsigned decim);
FMRX_API int fmrx_fe_plan_destroy(fmrx_fe_plan *plan);
/* 1 when the vector-ALU kernel (register window, packed FMA; fe_variant "valu")
 * exists for the plan's (taps, decim), which needs h[0] == 0.  It says nothing
 * about the matrix-core kernel (the default variant): that one runs for any taps
 * fe_mfma_scale accepts (finite, max|h| in [1e-30, 1e30]) at its nine shapes,
 * whatever this returns.  Otherwise the generic kernel runs. */
FMRX_API int fmrx_fe_plan_is_specialised(const fmrx_fe_plan *plan);
/* bytes of history kept in front of a block: 2*(taps-1) rounded up to a multiple
 * of 16, plus 16*decim (so the fused kernel can recompute the previous block's
 * last IF samples); the LAST 2*(taps-1) bytes are the reference's I_state/Q_state */
FMRX_API size_t fmrx_fe_plan_history_bytes(const fmrx_fe_plan *plan);
/* d_iq: DEVICE, 16-byte aligned, 2*n_samples bytes.  d_hist: DEVICE,
 * history_bytes bytes, or NULL for silence.  d_if: DEVICE, interleaved float
 * I,Q, n_samples/decim pairs.  stream: hipStream_t (NULL = default stream). */
FMRX_API int fmrx_fe_run_dev(const fmrx_fe_plan *plan, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist,
                             float *d_if, int force_generic, void *stream);

/* ------------------------------------------------------------------ */
/* Wideband tuner: N channels of a receiver bank from one wide capture   */
/* ------------------------------------------------------------------ */
/* The stage in front of a bank: ONE wide capture (interleaved I,Q at Fs_w = R * rf_Fs, R = 2 .. 32; u8, or s8 / s16 through
 * fmrx_tuner_create_ex) in, N channels'
 * u8 I,Q streams at rf_Fs out, each centred on its own offset f_c -- a frequency-translating decimating FIR per channel, one
 * int8 matrix-core GEMM for all of them (csrc/kernels_tuner.hip), written straight into the bank's input slots.
 *   y_c[m] = Q( g_c * sum_{k<T} h[k] * x[mR - k] * e^{-j 2 pi f_c (mR - k) / Fs_w} ),   x = (u8 - 128) as complex
 * in exact integer arithmetic (defined by tests/_tuner_model.py):
 *   w = round(f_c / Fs_w * 2^32) mod 2^32; taps g_c h[k] e^{+j 2 pi (w k mod 2^32) / 2^32} scaled by 2^s (s the largest
 *   integer with both parts <= 127 * 256 in magnitude, -14 <= s <= 47) and rounded half away from zero to int16 pairs;
 *   acc = sum_k taps[k] x[mR - k] in int32; rotation by (cos - j sin)(2 pi i / 4096) as round(32767 .), i = top 12 bits
 *   of w * n mod 2^32, n = mR counted in wide samples since create / reset; out = clamp(128 + ((y + 2^(s+14)) >> (s+15)), 0, 255).
 * Outputs do not depend on how the stream is cut into calls.
 *
 * Input formats (fmrx_tuner_create_ex; defined by tests/_tuner_formats_model.py).  The arithmetic above with
 *   FMRX_TUNER_U8   x = u8 - 128                      B = 0   what an RTL dongle delivers
 *   FMRX_TUNER_S8   x = the int8                      B = 0   HackRF, USRP sc8, bladeRF's 8-bit mode
 *   FMRX_TUNER_S16  x = the little-endian int16       B = 8   Airspy, SDRplay, USRP sc16, bladeRF SC16_Q11, LimeSDR
 * acc exact in 64 bits, and out = clamp(128 + ((y + 2^(s+14+B)) >> (s+15+B)), 0, 255): at gain 1 full scale in maps to full
 * scale out.  A device that puts 12 or 14 bits into the low end of the short (SC16_Q11: +-2048; SDRplay: 14 bits) is
 * brought to full scale by a `gain` of 16 or 4.  The shift stays in 1 .. 62, so an S16 tuner accepts -14 <= s <= 39:
 * fmrx_tuner_set_channel returns FMRX_EINVAL beyond that (gain x taps below 1e-7).  The output, the u8 I,Q slots of a bank,
 * is the same for every format; samples in front of a stream and past a call are zero samples (x = 0).
 *
 * Rational rates (fmrx_tuner_create_rational; defined by tests/_tuner_rational_model.py): a capture
 * at Fs_w whose rate is no integer multiple of rf_Fs -- 10, 12.5, 20 or 25 MS/s from an Airspy, an SDRplay, a HackRF or a
 * USRP -- is tuned at rf_Fs = Fs_w * U / D, gcd(U, D) = 1, 1 <= U <= 32, 2 U <= D <= 512 (6/25: 10 -> 2.4 MS/s).  h is the
 * prototype low-pass at U * Fs_w; with Tp = ceil(taps / U), n_m = floor(m D / U) and p_m = m D mod U,
 *   y_c[m] = Q( e^{-j phi_c(n_m)} * sum_{j<Tp} ( g_c h[p_m + j U] e^{+j phi_c(j)} ) * x[n_m - j] ),  phi_c(n) = 2 pi (w n mod 2^32) / 2^32
 * = zero-stuffing by U, filtering with h, keeping every D-th sample of the mixed capture.  Same w, same table, same rounding
 * and shift; ONE s per channel over all U phases; the int16 pairs are phase-major, re[p * Tp + j]; the accumulator's worst
 * case 128 * sum(|re| + |im|) is taken per phase.  A call takes n_wide % D == 0 samples and yields n_wide * U / D outputs per
 * channel; the state is the last Tp - 1 wide samples and the counter.  With U = 1 this is the integer tuner with R = D.
 *
 * fmrx_tuner_design / fmrx_tuner_table are host code (no device needed): the integers a channel uses.  design rejects
 * (FMRX_EINVAL) non-finite or all-zero gain x taps, |f_c| >= Fs_w / 2, s outside its range, and tap sets whose worst case
 * 128 * sum(|re| + |im|) does not fit int32.  table: cos_q15 / sin_q15 [4096] (either NULL: only *n is set). */
typedef struct fmrx_tuner fmrx_tuner;
FMRX_API int fmrx_tuner_design(const float *h, int taps, double Fs_w, double f_c, double gain, uint32_t *w, int *s, int16_t *re,
                               int16_t *im);
FMRX_API int fmrx_tuner_table(int16_t *cos_q15, int16_t *sin_q15, size_t *n);
/* host code: the integers of a channel of a rational tuner.  re, im: [U * ceil(taps / U)], phase-major.  Rejections as
 * fmrx_tuner_design, the accumulator's worst case per phase; U outside 1 .. 32: FMRX_EINVAL. */
FMRX_API int fmrx_tuner_design_rational(const float *h, int taps, int U, double Fs_w, double f_c, double gain, uint32_t *w, int *s,
                                        int16_t *re, int16_t *im);
/* h [taps]: the prototype low-pass at Fs_w (2 .. 4096 taps; more than 256 run the generic kernel).  max_wide_samples: the
 * largest call, a multiple of R.  Every channel starts at f_c = 0, gain 1.  The option "tuner_variant" is read here. */
FMRX_API int fmrx_tuner_create(fmrx_tuner **out, int R, const float *h, int taps, int n_channels, size_t max_wide_samples, int device);
/* the same for a capture of the given format; fmrx_tuner_create is the FMRX_TUNER_U8 case.  An unknown format: FMRX_EINVAL. */
#define FMRX_TUNER_U8 0
#define FMRX_TUNER_S8 1
#define FMRX_TUNER_S16 2
FMRX_API int fmrx_tuner_create_ex(fmrx_tuner **out, int R, const float *h, int taps, int n_channels, size_t max_wide_samples, int format,
                                  int device);
/* the tuner at rf_Fs = Fs_w * U / D.  h [taps]: the prototype low-pass at U * Fs_w (2 .. 4096 taps).  max_wide_samples: the
 * largest call, a multiple of D.  FMRX_EINVAL (the message names the argument) for gcd(U, D) != 1, U or D out of range,
 * D < 2 U, an unknown format.  Every other call works on the handle as on an integer one; calls take n_wide % D == 0.
 * The matrix kernels run for U <= 24, D <= 125, ceil(taps / U) <= 256, the generic kernel otherwise and under
 * "tuner_variant" = 1.  U = 1, D = R <= 32 is the handle of fmrx_tuner_create_ex(R): one host path builds every rate. */
FMRX_API int fmrx_tuner_create_rational(fmrx_tuner **out, int U, int D, const float *h, int taps, int n_channels,
                                        size_t max_wide_samples, int format, int device);
FMRX_API int fmrx_tuner_ratio(const fmrx_tuner *t, int *U, int *D);   /* (1, R) for a handle of fmrx_tuner_create / _create_ex */
FMRX_API int fmrx_tuner_format(const fmrx_tuner *t);            /* FMRX_TUNER_*; -1 for a null handle */
/* What a call of n_wide wide samples on this handle launches; there for tests and diagnostics.  Host arithmetic only (the same
 * function create and the launch read, csrc/tuner_host.hpp: tuner_plan_info): no device call, nothing changes.  matrix: 1 a
 * matrix-core kernel runs, 0 the generic kernel (then tiles, via_lds, lds_bytes, n_steps and steps_per_wg are 0 and the grid is
 * the generic kernel's: channels x 256 outputs).  tiles: 4, 2 or 1 tiles of 16 columns per wave and step.  via_lds: 1 a step's
 * outputs go through the per-wave LDS buffer to whole-row stores, 0 every 16-byte piece is stored directly (always 0 at an
 * integer rate).  lds_bytes: dynamic LDS of a workgroup (at most 65 536 where two share a CU, else at most 163 840).  The grid is
 * grid_x workgroups of steps_per_wg consecutive steps (n_steps in all) times grid_y rows of 16 channels.  FMRX_EINVAL for a null
 * argument or an n_wide fmrx_tuner_process_dev would refuse (0, no multiple of D, more than max_wide_samples). */
typedef struct fmrx_tuner_plan_info {
    int matrix, tiles, via_lds;
    size_t lds_bytes;
    int n_steps, steps_per_wg, grid_x, grid_y;
} fmrx_tuner_plan_info;
FMRX_API int fmrx_tuner_plan(const fmrx_tuner *t, size_t n_wide, fmrx_tuner_plan_info *out);
FMRX_API size_t fmrx_tuner_sample_bytes(const fmrx_tuner *t);   /* bytes per complex wide sample: 2, 2 or 4 */
FMRX_API int fmrx_tuner_destroy(fmrx_tuner *t);
FMRX_API int fmrx_tuner_reset(fmrx_tuner *t);     /* start of stream: silence in front, sample counter 0; channels keep their settings */
/* any time between calls; takes effect at the next call (which then waits once for its stream while it uploads) */
FMRX_API int fmrx_tuner_set_channel(fmrx_tuner *t, int channel, double f_c_hz, double Fs_w, double gain);
FMRX_API size_t fmrx_tuner_n_out_bytes(const fmrx_tuner *t, size_t n_wide);   /* 2 * n_wide * U / D (U / D = 1 / R); 0 unless n_wide % D == 0 */
/* d_wide: DEVICE, 16-byte aligned, n_wide complex samples in the tuner's format (fmrx_tuner_sample_bytes * n_wide bytes),
 * n_wide % R == 0.  Channel c's bytes go to d_out_first + c * pitch_bytes
 * (both multiples of 16): exactly what fmrx_channels_input_layout returns, so tuner -> bank -> RDS bank chain on one stream;
 * several tuners fill disjoint channel ranges of one bank by offsetting d_out_first.  Async on `stream`. */
FMRX_API int fmrx_tuner_process_dev(fmrx_tuner *t, const uint8_t *d_wide, size_t n_wide, uint8_t *d_out_first, size_t pitch_bytes,
                                    void *stream);
/* host in (n_wide complex samples in the tuner's format), host out [n_channels][n_out_bytes] */
FMRX_API int fmrx_tuner_process(fmrx_tuner *t, const uint8_t *wide, size_t n_wide, uint8_t *out);
/* waits for the last call; per channel, over that call: output bytes that clamped, and sum (I-128)^2 + (Q-128)^2 */
FMRX_API int fmrx_tuner_levels(fmrx_tuner *t, uint64_t *clipped, uint64_t *power);

/* ------------------------------------------------------------------ */
/* Signal meters: level, CNR, pilot, RDS, deviation of every channel    */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  One cheap pass over what a bank call leaves on the device -- the block region of every
 * input slot (fmrx_channels_input_layout) and, where the bank keeps them, the discriminator rows (fmrx_channels_demod_layout)
 * -- that says which channels hold a station, how good it is, whether it carries a pilot and RDS, how far off tune it is and
 * how far it deviates.  A stage with a handle of its own, fed from the layout functions as the RDS bank is; it keeps no state
 * between calls.  Defined by tests/_meters_model.py.
 *
 * Raw results, per channel and call (fmrx_meter):
 *   RF group, from the n_iq = n_iq_bytes / 2 complex samples i = I - 128, q = Q - 128 of the u8 row; exact integers:
 *     sum_i, sum_q   sum i, sum q                    m2        sum p, p = i^2 + q^2
 *     m4             sum p^2 (room for 2^33 samples)  clipped   bytes equal to 0 or 255
 *   MPX group, from the float32 discriminator row x[0 .. n_if) (radians per IF sample), accumulated in float64 in a fixed order
 *   (the same input gives the same bytes):
 *     sum_x, sum_x2, max_abs   over the n_if samples
 *     probe[p], p < 5          sum over the segments = n_if / 1024 whole segments s of |sum_k x[1024 s + k] t_p[k]|^2 with
 *                              t_p[k] = w[k] (cos, -sin)(2 pi f_p k / if_Fs), w[k] = 0.5 - 0.5 cos(2 pi (k + 0.5) / 1024) (Hann;
 *                              sum w = 512); the phase restarts in every segment, only powers are used; probe[5 .. 8) = 0
 *     f_p (fmrx_meters_probes) 17 000 and 21 000 Hz: noise, in the guard bands beside the pilot; 19 000 Hz: the pilot;
 *                              55 812.5 and 58 187.5 Hz: RDS, the biphase spectrum's maxima at 57 kHz -+ 1 187.5 Hz
 *   The samples past the last whole segment take part in sum_x, sum_x2 and max_abs only.
 * The raw sums of successive calls add and max_abs takes the maximum: integration over longer periods is the caller's, by
 * adding records field by field before fmrx_meters_derive.
 * The order of the float64 additions is part of the contract (tests/_meters_order_model.py restates it; the device is compared
 * with it bit for bit).  Thread t of 256 owns samples 4t .. 4t+3 of every 1024-sample segment.  Per segment and table row (5
 * real, 5 imaginary) it runs a = fma(x[4t+j], tab[4t+j], a) for j = 0 .. 3 from 0.0; the 256 values are added within each wave
 * of 64 lanes by halving (lanes l and l + 32, then l and l + 16, ... l and l + 1), the four waves as ((w0 + w1) + w2) + w3; the
 * power re * re + im * im (two rounded products, one add) is added to probe[p] in rising segment order.  sum_x and sum_x2: per
 * thread sx += x and sx2 = fma(x, x, sx2) over its samples, segment by segment, then over samples 1024 M + t, + 256, ... of the
 * tail; then the same halving and the same ((w0 + w1) + w2) + w3.  max_abs is an fmax chain from 0.0.
 * A row that is not finite: NaN or infinity goes into sum_x, sum_x2 and the probes -- all five, when it lies in a whole segment;
 * none, when it lies in the tail -- as IEEE arithmetic takes it in that order (the fields read NaN or infinity).  max_abs is the
 * largest |x| among the samples that are not NaN (infinity for an infinity; fmax skips NaN), 0 if there is none.  The
 * library's discriminators write 0 where I^2 + Q^2 = 0 (a noise-only channel can get there), so the rows of a bank are finite.
 *
 * Levels (fmrx_meter_levels; fmrx_meters_derive, host arithmetic in double).  Every dB value is clamped to [-99, 99]: -99
 * where the numerator is not positive (0 / 0 included), 99 where only the denominator is not; the other fields read 0 where
 * their sample count is 0.  With M2 = m2 / n_iq, M4 = m4 / n_iq, hz = if_Fs / 2 pi, M = segments:
 *   level_dbfs      10 log10(M2 / 16384)
 *   cnr_db          10 log10(S / (M2 - S)), S = sqrt(max(0, 2 M2^2 - M4)): the M2M4 estimator (a constant-envelope carrier in
 *                   complex Gaussian noise has M2 = S + N, M4 = S^2 + 4 S N + 2 N^2)
 *   clip_fraction   clipped / (2 n_iq)           dc_i, dc_q   sum_i / n_iq, sum_q / n_iq
 *   freq_offset_hz  sum_x / n_if * hz            peak_dev_hz  max_abs * hz         mpx_rms_hz  sqrt(sum_x2 / n_if) * hz
 *   pilot_dev_hz    4 sqrt(probe[19k] / M) / 1024 * hz  (a tone A cos gives a windowed sum of magnitude A * 1024 / 4)
 *   pilot_db        10 log10(probe[19k] / noise), noise = (probe[17k] + probe[21k]) / 2
 *   rds_db          10 log10(((probe[lo] + probe[hi]) / 2) / (9 noise)); 9 = (57 / 19)^2: discriminator noise rises with f^2
 * Thresholds for a stereo or an RDS lamp are the caller's.  Two limits of the definition: cnr_db is over the slot's whole
 * bandwidth (rf_Fs), not over a channel's 200 kHz; the noise probes sit about 8.5 bins from the pilot, so the window's leakage
 * caps pilot_db somewhere above 60 dB. */
#define FMRX_METERS_SEGMENT 1024
#define FMRX_METERS_PROBES 5
typedef struct fmrx_meter {
    uint64_t n_iq;
    int64_t sum_i, sum_q;
    uint64_t m2, m4, clipped, n_if, segments;
    double sum_x, sum_x2, max_abs, probe[8];
} fmrx_meter;
typedef struct fmrx_meter_levels {
    double level_dbfs, cnr_db, clip_fraction, dc_i, dc_q, freq_offset_hz, peak_dev_hz, mpx_rms_hz, pilot_dev_hz, pilot_db, rds_db;
} fmrx_meter_levels;
#ifdef __cplusplus
static_assert(sizeof(fmrx_meter) == 152, "fmrx_meter layout");
static_assert(sizeof(fmrx_meter_levels) == 88, "fmrx_meter_levels layout");
#else
_Static_assert(sizeof(fmrx_meter) == 152, "fmrx_meter layout");
_Static_assert(sizeof(fmrx_meter_levels) == 88, "fmrx_meter_levels layout");
#endif
typedef struct fmrx_meters fmrx_meters;
/* host code, no device needed: the probe frequencies (hz[0 .. 5), the rest 0; *n = 5), the tone table re, im [5][1024] as
 * the kernel uses it (built in double), and the levels of a record */
FMRX_API int fmrx_meters_probes(double hz[8], int *n);
FMRX_API int fmrx_meters_table(double if_Fs, double *re, double *im);
FMRX_API int fmrx_meters_derive(double if_Fs, const fmrx_meter *m, fmrx_meter_levels *out);
/* if_Fs: the discriminator rows' sample rate; below 120 000 the top probe would not stay under Nyquist: FMRX_EINVAL */
FMRX_API int fmrx_meters_create(fmrx_meters **out, double if_Fs, int n_channels, int device);
FMRX_API int fmrx_meters_destroy(fmrx_meters *m);
/* The arguments are what fmrx_channels_input_layout (d_iq_first, iq_pitch_bytes; n_iq_bytes = the bank's block_bytes, any
 * even count) and fmrx_channels_demod_layout (d_demod_row0, demod_pitch in floats, n_if) return: channel c's bytes at
 * d_iq_first + c * iq_pitch_bytes, its row at d_demod_row0 + c * demod_pitch.  Any byte alignment and pitch work; 16-byte
 * aligned rows, as a bank's, take the wide loads.  Either input may be NULL: that group reads zero with n_iq / n_if = 0 (the
 * fused mono bank of modes 0/1 keeps no rows).  With a demod input, n_if < 1024 is FMRX_EINVAL.  Asynchronous on `stream`,
 * after fmrx_channels_process_dev on the same stream; a second call before fmrx_meters_collect replaces the results. */
FMRX_API int fmrx_meters_process_dev(fmrx_meters *m, const uint8_t *d_iq_first, size_t iq_pitch_bytes, size_t n_iq_bytes,
                                     const float *d_demod_row0, size_t demod_pitch, size_t n_if, void *stream);
/* out [n_channels]; waits for the last call (an event it recorded), not for the device */
FMRX_API int fmrx_meters_collect(fmrx_meters *m, fmrx_meter *out);
/* host rows (either may be NULL), synchronous: the single-stream use is n_channels = 1 with the bytes given to
 * fmrx_pipeline_process and the row fmrx_pipeline_read_tap(FMRX_TAP_DEMOD) returns */
FMRX_API int fmrx_meters_process(fmrx_meters *m, const uint8_t *iq, size_t iq_pitch_bytes, size_t n_iq_bytes, const float *demod,
                                 size_t demod_pitch, size_t n_if, fmrx_meter *out);

/* ------------------------------------------------------------------ */
/* Stereo blend and soft mute, driven by the meters                     */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  The last stage behind a bank: from the pilot and guard-band noise powers the meters leave
 * on the device it decides, per channel and call, a stereo lamp, how far to blend left and right towards mono, and how far
 * to mute -- and applies both, ramped across the call, to the audio the bank wrote.  capture -> tuner -> bank -> meters ->
 * blend on one stream, no host round trip.  A stage with a handle of its own; it changes nothing in front of it.
 * Defined by tests/_blend_model.py; host and device equal that model bit for bit.
 *
 * Control (float64, per channel and call; every step one IEEE operation, no fused multiply-add, no sqrt, no log).  From
 * the MPX group of the channel's meter record:
 *   noise = (probe[17k] + probe[21k]) * 0.5       pilot ratio r_p = probe[19k] / noise       quieting r_q = ref / noise,
 *   ref = ((2 pi 7500 / if_Fs) * 256)^2 * segments: the windowed power a nominal pilot of 7.5 kHz deviation reads.
 *   drive d = plog2(r) = e + (m - 1) with r = m 2^e, m in [1, 2) (Mitchell's pseudo-logarithm through frexp: exact pieces,
 *   one rounded addition; within 0.0861 of log2 r, which is 0.26 dB).  Edge rule, as the meters' dB values: a numerator that
 *   is not > 0 (NaN included) gives d = -infinity; otherwise a denominator that is not > 0 gives d = +infinity; a quotient
 *   that underflows to 0 (or is not a number) reads -infinity, one that overflows +infinity.
 *   Thresholds are given in dB and divided by the literal 3.010299956639812 on the host; ramp(d; lo, hi) =
 *   clamp((d - lo) * (1 / (hi - lo)), 0, 1).
 *   lamp      hysteresis on d_p: on at d_p >= pilot_on, off at d_p < pilot_off, otherwise kept (off at the start)
 *   targets   separation t_b = lamp ? ramp(d_p; blend_lo, blend_hi) : 0;  gain t_m = floor + (1 - floor) * ramp(d_q; mute_lo, mute_hi)
 *   smoothing first call after create / reset: s = t.  Afterwards s = s + c * (t - s), c = attack where t < s and release
 *             otherwise; then s = t where |t - s| <= 2^-10 (a station that recovers reaches exactly 1).
 *   end points (float32): mono1 = (float)(1 - s_b), gain1 = (float)s_m; mono0, gain0 = the previous call's (the first call: equal)
 * Apply (float32, sample k of the call's n = n_audio; inv_n = (float)(1.0 / n)):
 *   a[k] = clamp(fmaf((float)(k + 1), (mono1 - mono0) * inv_n, mono0), 0, 1), m[k] likewise from gain0, gain1;
 *   D = 0.5f * (L - R);  l = a[k] == 0 ? L : fmaf(-a[k], D, L);  r = a[k] == 0 ? R : fmaf(a[k], D, R);  L' = m[k] * l, R' = m[k] * r.
 *   Full separation and full gain return the input bit for bit (-0 included); mono rows (audio_channels = 1) take the gain only.
 *   PCM: the library's pack of L', R' (pcm_policy), interleaved [n_channels][n_audio][audio_channels] as the banks write it.
 *
 * Defaults (fmrx_blend_defaults) -- design choices, not measurements of any receiver: lamp on / off at 20 / 14 dB of pilot
 * ratio; blend from mono at 20 dB to full separation at 32 dB; mute from the floor at 10 dB of quieting to full gain at
 * 24 dB; mute_floor 0 (silence between stations); attack 1 (a call that reads worse takes effect at once, ramped across
 * that call), release 0.25 per call.  fmrx_blend_create / fmrx_blend_control return FMRX_EINVAL unless blend_hi > blend_lo,
 * mute_hi > mute_lo, pilot_on >= pilot_off, 0 <= mute_floor <= 1, 0 < attack, release <= 1 and everything is finite. */
typedef struct fmrx_blend_params {
    double pilot_on, pilot_off, blend_lo, blend_hi, mute_lo, mute_hi;   /* dB */
    double mute_floor, attack, release;
} fmrx_blend_params;
/* Per channel: what the last call decided, and the state the next one starts from.  pilot_db / quiet_db: the drives times
 * 3.010299956639812 (pseudo-dB; -+infinity by the edge rule). */
typedef struct fmrx_blend_status {
    double pilot_db, quiet_db;
    double sep_target, gain_target;   /* t_b, t_m */
    double sep, gain;                 /* s_b, s_m */
    float mono0, gain0, mono1, gain1; /* the last call's ramps: from (mono0, gain0) to (mono1, gain1) */
    uint32_t lamp, reserved;
    uint64_t calls;                   /* since create / reset; 0 = the next call is a first call */
} fmrx_blend_status;
#ifdef __cplusplus
static_assert(sizeof(fmrx_blend_params) == 72, "fmrx_blend_params layout");
static_assert(sizeof(fmrx_blend_status) == 80, "fmrx_blend_status layout");
#else
_Static_assert(sizeof(fmrx_blend_params) == 72, "fmrx_blend_params layout");
_Static_assert(sizeof(fmrx_blend_status) == 80, "fmrx_blend_status layout");
#endif
typedef struct fmrx_blend fmrx_blend;
FMRX_API int fmrx_blend_defaults(fmrx_blend_params *p);
/* Host code, no device needed: one channel's control step on one record (only probe[0 .. 5) and segments are read); *state
 * is read and replaced.  A zeroed status is a fresh channel.  The function the control kernel runs (blend_control.hpp). */
FMRX_API int fmrx_blend_control(const fmrx_blend_params *p, double if_Fs, const fmrx_meter *rec, fmrx_blend_status *state_in_out);
/* n_audio: samples per row and call (fmrx_channels_n_audio); audio_channels 1 or 2 */
FMRX_API int fmrx_blend_create(fmrx_blend **out, const fmrx_blend_params *p, double if_Fs, int n_channels, int audio_channels,
                               size_t n_audio, int device);
FMRX_API int fmrx_blend_destroy(fmrx_blend *b);
/* channel < 0: all.  Waits for the handle's last call; the rows are clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_blend_reset(fmrx_blend *b, int channel);
/* Asynchronous on `stream`, after fmrx_meters_process_dev on the same stream: reads the MPX results of m's last call where
 * they lie on the device.  FMRX_EINVAL where that call had no discriminator rows (n_if = 0: the fused mono bank of modes 0/1
 * keeps none) or m has another channel count or device.  d_in [n_channels][audio_channels][n_audio] as
 * fmrx_channels_process_dev writes it; d_out the same shape, d_out == d_in allowed (no other overlap); d_pcm16
 * [n_channels][n_audio][audio_channels]; d_out or d_pcm16 may be NULL, not both.  Stereo rows that are 16-byte aligned
 * (d_in, d_out and d_pcm16 are, and n_audio is a multiple of 4) move in 16-byte pieces; all others 4 bytes at a time, the
 * same arithmetic. */
FMRX_API int fmrx_blend_process_dev(fmrx_blend *b, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16,
                                    int pcm_policy, void *stream);
/* Host rows and host records [n_channels], synchronous (it first waits for the handle's last call, whatever stream that was
 * on): the records' MPX groups are uploaded in the meters' layout and the
 * same two kernels run (the single-stream use: n_channels = 1 with fmrx_meters_process's record).  out == in allowed (the
 * device pass then runs in place); the device copies keep each host pointer's address modulo 16, so a host row that is not
 * 16-byte aligned takes the 4-byte path. */
FMRX_API int fmrx_blend_process(fmrx_blend *b, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy);
/* out [n_channels]; waits for the handle's last call (an event it recorded), not for the device */
FMRX_API int fmrx_blend_status_get(fmrx_blend *b, fmrx_blend_status *out);

/* ------------------------------------------------------------------ */
/* Variable high-cut, driven by the meters                              */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  The third thing a receiver does with a weak signal, behind the blend (or directly behind a
 * bank): a one-pole low-pass per audio row whose corner moves with the channel's quieting, from above Nyquist (transparent)
 * down to fc_min.  capture -> tuner -> bank -> meters -> blend -> high-cut on one stream, no host round trip.  A stage with a
 * handle of its own; it changes nothing in front of it.  Defined by tests/_highcut_model.py; host and
 * device equal that model bit for bit.
 *
 * Design (host, float64): p_max_d = exp(-2 pi fc_min / audio_Fs), p_max = (float)p_max_d; FMRX_EINVAL unless fc_min and
 * audio_Fs are finite and > 0 and p_max <= 0.875 (beyond that pole the built-in lanes of the parallel walk start to miss on
 * ordinary audio; at 48 kHz that is fc_min >= 1 020.1 Hz).  The pole moves linearly with the cut: 0 is transparent, p_max
 * has its -3 dB corner at fc_min.  No transcendental function runs on the device.
 * Control (float64, per channel and call; the blend's arithmetic and edge rules, one IEEE operation per step):
 *   noise and the quieting drive d_q exactly as the blend forms them (ref * segments / noise through plog2);
 *   openness target t_o = (1 - cut_max) + cut_max * ramp(d_q; hc_lo, hc_hi);
 *   smoothing as the blend's: a first call takes s_o = t_o; attack where t_o < s_o, release otherwise; the 2^-10 snap;
 *   end points (float32): p1 = (float)((1 - s_o) * p_max_d); p0 = the previous call's p1 (a first call: equal).
 * Apply (float32, per row; both rows of a stereo channel use the channel's poles; y_prev = +0 at the start of a stream, carried
 * across calls; sample k of the call's n = n_audio, inv_n = (float)(1.0 / n)):
 *   p[k] = clamp(fmaf((float)(k + 1), (p1 - p0) * inv_n, p0), 0, p_max)
 *   q = 1 - p[k];  v = q * x[k];  y = fmaf(p[k], y_prev, v);  if |y| < 2^-126: y = +0
 *   y[k] = p[k] == 0 ? x[k] : y;  y_prev = y[k]
 *   A channel at cut 0 returns its input bit for bit (-0, subnormals and NaN included: two NaNs are the same value).
 *   PCM: the library's pack of y (pcm_policy), interleaved [n_channels][n_audio][audio_channels] as the banks write it.
 * The device walks the recurrence parallel in time (lanes of `segment` samples that start `warmup` samples early, a verify
 * step, a serial repair of the misses) and returns the serial walk's bits whatever the lane shape.
 *
 * Defaults (fmrx_highcut_defaults) -- design choices, not measurements of any receiver: fc_min 2 500 Hz; no cut from 36 dB of
 * quieting (hc_hi), full cut at 16 dB (hc_lo); cut_max 1; attack 1 (a call that reads worse takes effect at once, ramped
 * across that call), release 0.25 per call; warmup and segment -1 (the built-in lane shape, 256 and 256).
 * fmrx_highcut_create / fmrx_highcut_control return FMRX_EINVAL unless hc_hi > hc_lo, 0 <= cut_max <= 1, 0 < attack,
 * release <= 1, warmup in -1 .. 2^20, segment -1 or 1 .. 2^20, the design's conditions hold and everything is finite. */
typedef struct fmrx_highcut_params {
    double fc_min;          /* Hz: the corner at full cut */
    double hc_lo, hc_hi;    /* dB of quieting: full cut at and below hc_lo, none from hc_hi */
    double cut_max, attack, release;
    int32_t warmup, segment;   /* the parallel walk's lane shape; -1 = built-in */
} fmrx_highcut_params;
/* Per channel: what the last call decided, and the state the next one starts from.  quiet_db as fmrx_blend_status's. */
typedef struct fmrx_highcut_status {
    double quiet_db;
    double open_target, open;   /* t_o, s_o: 1 = no cut */
    float p0, p1;               /* the last call's pole ramp */
    uint64_t calls;             /* since create / reset; 0 = the next call is a first call */
} fmrx_highcut_status;
#ifdef __cplusplus
static_assert(sizeof(fmrx_highcut_params) == 56, "fmrx_highcut_params layout");
static_assert(sizeof(fmrx_highcut_status) == 40, "fmrx_highcut_status layout");
#else
_Static_assert(sizeof(fmrx_highcut_params) == 56, "fmrx_highcut_params layout");
_Static_assert(sizeof(fmrx_highcut_status) == 40, "fmrx_highcut_status layout");
#endif
typedef struct fmrx_highcut fmrx_highcut;
FMRX_API int fmrx_highcut_defaults(fmrx_highcut_params *p);
/* Host code, no device needed: one channel's control step on one record (only probe[0 .. 5) and segments are read); *state
 * is read and replaced.  A zeroed status is a fresh channel.  The function the control kernel runs (highcut_control.hpp). */
FMRX_API int fmrx_highcut_control(const fmrx_highcut_params *p, double if_Fs, double audio_Fs, const fmrx_meter *rec,
                                  fmrx_highcut_status *state_in_out);
/* Host code: the design alone, *p_max = the float32 pole at full cut; FMRX_EINVAL as stated above */
FMRX_API int fmrx_highcut_design(double fc_min, double audio_Fs, float *p_max);
/* n_audio: samples per row and call (fmrx_channels_n_audio); audio_channels 1 or 2 */
FMRX_API int fmrx_highcut_create(fmrx_highcut **out, const fmrx_highcut_params *p, double if_Fs, double audio_Fs, int n_channels,
                                 int audio_channels, size_t n_audio, int device);
FMRX_API int fmrx_highcut_destroy(fmrx_highcut *h);
/* channel < 0: all.  Clears the status row and the filter state of the channel's rows.  Waits for the handle's last call; the
 * rows are clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_highcut_reset(fmrx_highcut *h, int channel);
/* on != 0: every later call walks its rows serially, one lane per row (the kernel the parallel walk is measured against); the
 * bits are the same, fmrx_highcut_diagnostics counts nothing for such calls.  Waits for the handle's last call. */
FMRX_API int fmrx_highcut_set_force(fmrx_highcut *h, int on);
/* Asynchronous on `stream`, after fmrx_meters_process_dev on the same stream (and after the blend, where there is one): reads
 * the MPX results of m's last call where they lie on the device.  FMRX_EINVAL where that call had no discriminator rows
 * (n_if = 0: the fused mono bank of modes 0/1 keeps none) or m has another channel count or device.  Shapes and alignment as
 * fmrx_blend_process_dev: d_in [n_channels][audio_channels][n_audio], d_out the same shape, d_out == d_in allowed (no other
 * overlap; the call then filters a copy of the rows it keeps in the handle); d_pcm16 [n_channels][n_audio][audio_channels];
 * d_out or d_pcm16 may be NULL, not both; float rows 4-byte aligned, PCM 2-byte. */
FMRX_API int fmrx_highcut_process_dev(fmrx_highcut *h, const fmrx_meters *m, const float *d_in, float *d_out, int16_t *d_pcm16,
                                      int pcm_policy, void *stream);
/* Host rows and host records [n_channels], synchronous (it first waits for the handle's last call): the single-stream use is
 * n_channels = 1 with fmrx_meters_process's record.  out == in allowed; the device copies keep each host pointer's address
 * modulo 16. */
FMRX_API int fmrx_highcut_process(fmrx_highcut *h, const fmrx_meter *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy);
/* out [n_channels]; waits for the handle's last call (an event it recorded), not for the device */
FMRX_API int fmrx_highcut_status_get(fmrx_highcut *h, fmrx_highcut_status *out);
/* Since create: the segment boundaries the verify step checked and the segments it walked again (as
 * fmrx_channels_deemph_diagnostics); waits for the handle's last call.  Either pointer may be NULL. */
FMRX_API int fmrx_highcut_diagnostics(fmrx_highcut *h, unsigned long long *segments, unsigned long long *missed);

/* ------------------------------------------------------------------ */
/* Audio meters: peak, RMS, BS.1770 loudness, stereo image, gating      */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  What the signal meters are for the RF and the multiplex side, for the audio that comes out
 * the other end: per channel of a receiver bank and call, is there programme or dead air, how loud is it by ITU-R BS.1770 /
 * EBU R 128, does the PCM clip, is the stereo signal really stereo.  capture -> tuner -> bank -> meters -> blend -> high-cut ->
 * audio meters on one stream; a few dozen bytes per channel come back instead of the audio.  A stage with a handle of its own
 * that only reads the rows; it needs no discriminator rows and no fmrx_meters, so it also serves the fused mono bank of modes
 * 0 / 1.  Defined by tests/_audio_meters_model.py; host and device equal that model bit for bit (a
 * NaN's sign and payload are the machine's).
 *
 * K-weighting: two biquads in float64, designed for audio_Fs by the usual closed form of the BS.1770 pre-filter, K = tan(pi f0
 * / Fs), KQ = K / Q, K2 = K K, a0 = (1 + KQ) + K2:
 *   shelf      f0 = 1681.974450955533, Q = 0.7071752369554196, Vh = 10^(3.999843853973347 / 20) and Vb = Vh^0.4996667741545416
 *              as literals;  b = [((Vh + Vb KQ) + K2) / a0, (2 (K2 - Vh)) / a0, ((Vh - Vb KQ) + K2) / a0],
 *              a = [(2 (K2 - 1)) / a0, ((1 - KQ) + K2) / a0]
 *   high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], not normalised, as in the standard's table; a as
 *              the shelf's.  At 48 000 Hz the design equals the table of BS.1770-4 to 9e-16.
 * Walk, per row and sample x, v = (double)x, for the shelf and then the high-pass (transposed direct form II; every step one
 * IEEE double operation, no fused multiply-add; float64 denormals are kept):
 *   o = b0 v + z1;   z1 = (b1 v - a1 o) + z2;   z2 = b2 v - a2 o
 * Raw results per channel and call (fmrx_audio_meter; arrays of 2 for the rows L and R, mono fills index 0 only; every sum is
 * float64, serial in sample order):
 *   n            the call's samples per row
 *   over[r]      samples with !(fabsf(x) < 2.0f): at or beyond what the PCM pack (short)(x * 16384) overflows on; NaN counts
 *   peak[r]      max |x|; skips NaN, reads infinity for an infinity
 *   sum_x[r], sum_x2[r]          sum_k2[r]   sum y^2, y the K-weighted sample          sum_lr   sum L R; 0 for mono
 *   bins_done    the 100 ms bins this call closed
 * Records of successive calls add field by field and peak takes the maximum, as the signal meters' records do.
 * 100 ms bins: bin_len = (size_t)(audio_Fs / 10 + 0.5) samples.  After each sample the row's y^2 is added to bin_acc[r]; when
 * bin_fill reaches bin_len, bin_acc[r] goes to bins[r][bins_done] and is cleared.  A call of n samples closes at most n / bin_len
 * + 1 bins; bins straddle calls.  The state per channel -- the eight filter values, bin_acc[2] and bin_fill
 * (fmrx_audio_meter_state; all zero is a fresh channel) -- is carried across calls.  A NaN or an infinity in a row poisons that
 * row's filter state: sum_k2 and the bins read NaN from then on, until fmrx_audio_meters_reset.
 *
 * Levels (fmrx_audio_levels; fmrx_audio_meters_derive, host arithmetic in double; full_scale is the float value of 0 dBFS, 2.0
 * for the library's PCM pack, which maps it to 32 768; fs2 = full_scale^2).  Every dB value follows the signal meters' edge
 * rule: clamped to [-99, 99], -99 where the numerator is not positive (0 / 0 and NaN included), 99 where only the denominator is
 * not; the other fields read 0 where they are undefined (n = 0; correlation and balance_db of a mono channel; correlation where
 * a row is silent).
 *   peak_dbfs[r]   10 log10(peak^2 / fs2)            rms_dbfs[r]   10 log10(sum_x2 / n / fs2)          dc[r]   sum_x / n
 *   loudness_lkfs  -0.691 + 10 log10((sum_k2[0] + sum_k2[1]) / n / fs2): ungated, over the record (add records for longer spans)
 *   correlation    sum_lr / sqrt(sum_x2[0] sum_x2[1])      balance_db   10 log10(sum_x2[0] / sum_x2[1])
 *   over_fraction  (over[0] + over[1]) / (n audio_channels)
 * Thresholds for silence, overload or a mono alarm are the caller's.
 *
 * The device pass: parallel over channels only -- the high-pass has its poles at 0.995, so no warm-up of practical length
 * seeds a later start to the serial walk's bits -- one lane per channel, 64 channels per wave.  A bank fills the card from
 * about 16 384 channels; a single stream (n_channels = 1) is one lane walking serially: correct, not fast. */
typedef struct fmrx_audio_meter {
    uint64_t n, over[2];
    double peak[2], sum_x[2], sum_x2[2], sum_k2[2], sum_lr;
    uint64_t bins_done;
} fmrx_audio_meter;
typedef struct fmrx_audio_meter_state {
    double z[2][4];      /* per row: shelf z1, z2, high-pass z1, z2 */
    double bin_acc[2];
    uint64_t bin_fill;
} fmrx_audio_meter_state;
typedef struct fmrx_audio_levels {
    double peak_dbfs[2], rms_dbfs[2], dc[2], loudness_lkfs, correlation, balance_db, over_fraction;
} fmrx_audio_levels;
/* Gated loudness of one channel (fmrx_loudness_read): every value by the dB edge rule, -99 where there is nothing to read yet */
typedef struct fmrx_loudness_levels {
    double momentary, short_term, integrated;
    uint64_t blocks;           /* gating blocks stored */
    uint32_t full, reserved;   /* full: max_blocks reached; later blocks are not stored (integrated stands still) */
} fmrx_loudness_levels;
#ifdef __cplusplus
static_assert(sizeof(fmrx_audio_meter) == 104, "fmrx_audio_meter layout");
static_assert(sizeof(fmrx_audio_meter_state) == 88, "fmrx_audio_meter_state layout");
static_assert(sizeof(fmrx_audio_levels) == 80, "fmrx_audio_levels layout");
static_assert(sizeof(fmrx_loudness_levels) == 40, "fmrx_loudness_levels layout");
#else
_Static_assert(sizeof(fmrx_audio_meter) == 104, "fmrx_audio_meter layout");
_Static_assert(sizeof(fmrx_audio_meter_state) == 88, "fmrx_audio_meter_state layout");
_Static_assert(sizeof(fmrx_audio_levels) == 80, "fmrx_audio_levels layout");
_Static_assert(sizeof(fmrx_loudness_levels) == 40, "fmrx_loudness_levels layout");
#endif
typedef struct fmrx_audio_meters fmrx_audio_meters;
typedef struct fmrx_loudness fmrx_loudness;
/* Host code, no device needed.  design: coef [2][5] = (b0, b1, b2, a1, a2) of the shelf, then of the high-pass; audio_Fs finite,
 * 8 000 .. 768 000, else FMRX_EINVAL (as every function here that takes audio_Fs).  bin_len / max_bins: the bin length in samples
 * and n_audio / bin_len + 1; 0 for an audio_Fs that design refuses. */
FMRX_API int fmrx_audio_meters_design(double audio_Fs, double *coef);
FMRX_API size_t fmrx_audio_meters_bin_len(double audio_Fs);
FMRX_API size_t fmrx_audio_meters_max_bins(double audio_Fs, size_t n_audio);
/* The host reference of one channel: rows [audio_channels][row_pitch] floats of which n are walked; *state is read and replaced;
 * *rec is written; bins [2][max_bins] doubles is written (entries past bins_done, and a mono channel's second row, 0);
 * max_bins >= n / bin_len + 1, else FMRX_EINVAL.  The body the kernel runs (audio_meters_core.hpp). */
FMRX_API int fmrx_audio_meters_walk(double audio_Fs, int audio_channels, const float *rows, size_t row_pitch, size_t n,
                                    fmrx_audio_meter_state *state_in_out, fmrx_audio_meter *rec, double *bins, size_t max_bins);
FMRX_API int fmrx_audio_meters_derive(const fmrx_audio_meter *rec, int audio_channels, double full_scale, fmrx_audio_levels *out);
/* n_audio: the most samples per row and call (fmrx_channels_n_audio), 1 .. 2^26; audio_channels 1 or 2 */
FMRX_API int fmrx_audio_meters_create(fmrx_audio_meters **out, double audio_Fs, int n_channels, int audio_channels, size_t n_audio,
                                      int device);
FMRX_API int fmrx_audio_meters_destroy(fmrx_audio_meters *m);
/* channel < 0: all.  Clears the channel's filter state, bin_acc and bin_fill.  Waits for the handle's last call; the state is
 * clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_audio_meters_reset(fmrx_audio_meters *m, int channel);
/* out [n_channels]: every channel's carried state; waits for the handle's last call */
FMRX_API int fmrx_audio_meters_state_get(fmrx_audio_meters *m, fmrx_audio_meter_state *out);
/* Asynchronous on `stream`, behind whatever wrote the rows on the same stream: d_audio [n_channels][audio_channels][row_pitch]
 * floats, as the banks, the blend and the high-cut write them (row_pitch = n_audio there), of which the first n <= n_audio of
 * every row are walked; 4-byte aligned.  Rows that are 16-byte aligned (d_audio is, and row_pitch is a multiple of 4) are
 * fetched in 16-byte pieces, all others 4 bytes at a time, the same arithmetic.  The rows are only read.  One kernel launch; a
 * second call before fmrx_audio_meters_collect replaces the results (the state has then advanced by both). */
FMRX_API int fmrx_audio_meters_process_dev(fmrx_audio_meters *m, const float *d_audio, size_t row_pitch, size_t n, void *stream);
/* records [n_channels], bins [n_channels][2][max_bins] doubles (may be NULL); waits for the last call (an event it recorded),
 * not for the device */
FMRX_API int fmrx_audio_meters_collect(fmrx_audio_meters *m, fmrx_audio_meter *records, double *bins);
/* host rows [n_channels][audio_channels][row_pitch], synchronous: the single-stream use is n_channels = 1 with the audio
 * fmrx_pipeline_process returns */
FMRX_API int fmrx_audio_meters_process(fmrx_audio_meters *m, const float *audio, size_t row_pitch, size_t n, fmrx_audio_meter *records,
                                       double *bins);
/* Gated loudness by BS.1770-4, host only, no device needed: an integrator over what fmrx_audio_meters_collect returns.  Gating
 * blocks are 4 consecutive bins with a hop of one bin, rows summed (400 ms, 75 % overlap); a block's loudness is -0.691 + 10
 * log10(its energy / (4 bin_len) / full_scale^2).  momentary: the last block; short_term: the last 30 bins; integrated: over the
 * stored blocks above the absolute gate of -70 LKFS that are also above the relative gate, 10 LU under the loudness of the mean
 * of the absolutely gated blocks.  Per channel up to max_blocks block energies are stored (8 bytes each; one hour is 36 000);
 * at max_blocks `full` is set and nothing is overwritten: momentary and short_term go on, integrated stands still. */
FMRX_API int fmrx_loudness_create(fmrx_loudness **out, int n_channels, size_t bin_len, size_t max_blocks, double full_scale);
FMRX_API int fmrx_loudness_destroy(fmrx_loudness *l);
FMRX_API int fmrx_loudness_reset(fmrx_loudness *l, int channel);   /* channel < 0: all */
/* records [n_channels] and bins [n_channels][2][max_bins] as fmrx_audio_meters_collect returned them (only bins_done is read
 * of a record) */
FMRX_API int fmrx_loudness_push(fmrx_loudness *l, const fmrx_audio_meter *records, const double *bins, size_t max_bins);
FMRX_API int fmrx_loudness_read(const fmrx_loudness *l, int channel, fmrx_loudness_levels *out);

/* ------------------------------------------------------------------ */
/* Loudness leveller and look-ahead peak limiter, driven by the audio meters */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  The stage that acts on what the audio meters measure: per channel of a receiver bank it
 * brings the programme to one loudness target and bounds the output below full scale, so that the PCM it packs cannot wrap.
 * capture -> tuner -> bank -> meters -> blend -> high-cut -> audio meters -> leveller on one stream, no host round trip.  A
 * stage with a handle of its own; it changes nothing in front of it.  Defined by tests/_leveller_model.py (DESIGN.md section
 * 4.15); host and device equal that model bit for bit.
 *
 * Parameters, linear values made once on the host with libm's pow: fs2 = full_scale^2; target_ms = 10^((target_lkfs + 0.691) /
 * 10), gate_ms likewise; g_max = 10^(max_boost_db / 20), g_min = 10^(-max_cut_db / 20); the ceiling c = (float)(full_scale
 * 10^(ceiling_dbfs / 20)).
 * Control (float64, per channel and call, from the audio meters' record; every step one IEEE operation, no fused multiply-add,
 * no sqrt, log or pow):
 *   ms = ((sum_k2[0] + (stereo ? sum_k2[1] : 0)) / n) / fs2          the call's K-weighted mean square against full scale
 *   gated = !(ms >= gate_ms && ms < infinity): dead air, a muted channel, n = 0, NaN -- the estimate loud_ms stands.
 *   Otherwise the first such call sets loud_ms = ms, later ones loud_ms += k (ms - loud_ms), k = attack where ms > loud_ms,
 *   else release.  Without an estimate the gain is 1.  With one, r = target_ms / loud_ms and gain = heron2(r) clamped to
 *   [g_min, g_max] (g_min where r is not > 0, g_max where it is infinite).  heron2 is a square root in basic operations:
 *   the seed pexp2(0.5 plog2(r)) -- plog2 the blend's pseudo-logarithm, pexp2(x) = ldexp(1 + (x - floor x), floor x) -- and two
 *   steps y = 0.5 (y + r / y); within 1e-5 of sqrt r (DESIGN.md has the measured figure).
 *   End points (float32): gain1 = (float)gain; gain0 = the previous call's gain1 (the first call: equal).
 * Gain and limiter (float32 and integers; W the look-ahead, ONE = 2^24 = FMRX_LEVELLER_ONE; sample k of the call's n = n_audio,
 * inv_n = (float)(1.0 / n)):
 *   g[k] = fmaf((float)(k + 1), (gain1 - gain0) * inv_n, gain0);   u_r[k] = x_r[k] * g[k] for each row r
 *   code(a) = a <= c ? ONE : (a < infinity ? (uint32)((c / a) * 16777216.0f) : 0)          NaN and infinity: 0
 *   q[k] = min over the rows of code(|u_r[k]|)                      stereo is linked: one gain for both rows
 *   m[k] = min(q[k-W+1 .. k]);   s[k] = (sum of m[k-W+1 .. k]) >> log2 W;   y_r[k] = u_r[k-(W-1)] * ((float)s[k] * 2^-24)
 *   The output is the input delayed by W - 1 samples.  Every m that enters s[k] has q[k-W+1] in its window, so s[k] <=
 *   q[k-W+1] and |y| <= c (1 + 2^-24)^2 < c (1 + 2^-22): no finite output exceeds the ceiling by more than two roundings.  With
 *   gain 1 and nothing beyond c the output is the input delayed, bit for bit.  A NaN comes out as NaN, an infinity as NaN (the
 *   product of infinity and the gain 0), and both fade their 2W - 1 neighbours to zero; neither stays in the state.
 *   The state per channel, carried across calls: the last 2W - 2 codes and the last W - 1 values of u per row; fresh: ONE and 0.
 *   Codes are integers and the float work is per sample, so any split of a row over lanes, workgroups or calls gives the
 *   same bits; only the gain ramp is defined per call.
 *   min_code: the smallest s of the call; limited: the number of k with s[k] < ONE.
 *   PCM: the library's pack of y (pcm_policy), interleaved [n_channels][n_audio][audio_channels] as the banks write it.
 *
 * Defaults (fmrx_leveller_defaults) -- design choices: target -23 LKFS (EBU R 128); at most 12 dB up and 20 dB down; gate at
 * -50 LKFS; attack 0.2 and release 0.02 per call; ceiling -1 dBFS; full_scale 2.0 (what the PCM pack maps to 32 768).
 * max_boost_db = max_cut_db = 0 is a limiter alone.  fmrx_leveller_create / fmrx_leveller_control return FMRX_EINVAL unless
 * everything is finite, max_boost_db >= 0, max_cut_db >= 0, gate_lkfs < target_lkfs, 0 < attack, release <= 1, ceiling_dbfs <
 * 0, full_scale > 0, every linear value above is finite and > 0 and c is a normal float. */
#define FMRX_LEVELLER_ONE 16777216u
typedef struct fmrx_leveller_params {
    double target_lkfs, max_boost_db, max_cut_db, gate_lkfs;
    double attack, release;
    double ceiling_dbfs, full_scale;
} fmrx_leveller_params;
/* Per channel: what the last call decided and did, and the state the next control step starts from. */
typedef struct fmrx_leveller_status {
    double loud_ms;             /* the loudness estimate as a mean square against full scale; 0: none yet */
    double gain;
    float gain0, gain1;         /* the last call's ramp */
    uint32_t gated;
    uint32_t min_code, limited; /* written by the pass over the audio */
    uint32_t reserved;
    uint64_t calls;             /* since create / reset; 0 = the next call is a first call */
} fmrx_leveller_status;
typedef struct fmrx_leveller_levels {
    double loudness_lkfs;       /* -0.691 + 10 log10(loud_ms); -99 without an estimate */
    double gain_db;             /* 20 log10(gain) */
    double reduction_db;        /* 20 log10(min_code / 2^24) <= 0: the limiter's deepest reduction of the call; -99 for code 0 */
} fmrx_leveller_levels;
#ifdef __cplusplus
static_assert(sizeof(fmrx_leveller_params) == 64, "fmrx_leveller_params layout");
static_assert(sizeof(fmrx_leveller_status) == 48, "fmrx_leveller_status layout");
static_assert(sizeof(fmrx_leveller_levels) == 24, "fmrx_leveller_levels layout");
#else
_Static_assert(sizeof(fmrx_leveller_params) == 64, "fmrx_leveller_params layout");
_Static_assert(sizeof(fmrx_leveller_status) == 48, "fmrx_leveller_status layout");
_Static_assert(sizeof(fmrx_leveller_levels) == 24, "fmrx_leveller_levels layout");
#endif
typedef struct fmrx_leveller fmrx_leveller;
FMRX_API int fmrx_leveller_defaults(fmrx_leveller_params *p);
/* Host code, no device needed.  control: one channel's control step on one record (n and sum_k2 are read); *state is read and
 * replaced; a zeroed status is a fresh channel.  The function the control kernel runs (leveller_control.hpp).  ceiling: c.
 * derive: a status in dB, with log10.  tile: the samples of a row one workgroup writes, 2048 - 2 lookahead (0 for a lookahead
 * that is no power of two in 8 .. 128). */
FMRX_API int fmrx_leveller_control(const fmrx_leveller_params *p, int audio_channels, const fmrx_audio_meter *rec,
                                   fmrx_leveller_status *state_in_out);
FMRX_API int fmrx_leveller_ceiling(const fmrx_leveller_params *p, float *ceiling);
FMRX_API int fmrx_leveller_derive(const fmrx_leveller_status *st, fmrx_leveller_levels *out);
FMRX_API size_t fmrx_leveller_tile(int lookahead);
/* The host reference of one channel's gain and limiter, serial: rows [audio_channels][row_pitch] of which n >= 1 are walked
 * with the ramp gain0 -> gain1 across them, out [audio_channels][out_pitch]; codes [2 lookahead - 2] and u
 * [audio_channels][lookahead - 1] are the state, read and replaced (fresh: FMRX_LEVELLER_ONE and 0); *min_code and *limited
 * (either may be NULL) as the status row's. */
FMRX_API int fmrx_leveller_walk(int audio_channels, int lookahead, float ceiling, float gain0, float gain1, const float *rows,
                                size_t row_pitch, size_t n, uint32_t *codes, float *u, float *out, size_t out_pitch, uint32_t *min_code,
                                uint32_t *limited);
/* n_audio: samples per row and call (fmrx_channels_n_audio); audio_channels 1 or 2; audio_Fs as the audio meters' (finite, 8 000
 * .. 768 000; only the latency in seconds depends on it); lookahead: a power of two in 8 .. 128, 0 = 64 */
FMRX_API int fmrx_leveller_create(fmrx_leveller **out, const fmrx_leveller_params *p, double audio_Fs, int n_channels, int audio_channels,
                                  size_t n_audio, int lookahead, int device);
FMRX_API int fmrx_leveller_destroy(fmrx_leveller *h);
/* channel < 0: all.  Clears the status row and the limiter's state of the channel.  Waits for the handle's last call; the rows
 * are clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_leveller_reset(fmrx_leveller *h, int channel);
/* the delay of the stage in samples, lookahead - 1; 0 for a NULL handle */
FMRX_API size_t fmrx_leveller_latency(const fmrx_leveller *h);
/* Asynchronous on `stream`, after fmrx_audio_meters_process_dev on the same stream: reads the sums of am's last call where
 * they lie on the device.  FMRX_EINVAL where am has made no call, where that call walked another n than this handle's n_audio,
 * or where am has another channel count, audio_channels or device.  d_in [n_channels][audio_channels][n_audio]; d_out the same
 * shape; d_pcm16 [n_channels][n_audio][audio_channels]; d_out or d_pcm16 may be NULL, not both.  d_out must not overlap d_in
 * (FMRX_EINVAL): a workgroup reads 2 lookahead samples in front of the ones it writes.  Float rows 4-byte aligned, PCM 2-byte;
 * stereo rows that are 16-byte aligned (every pointer given, n_audio a multiple of 4) move in 16-byte pieces, all others 4
 * bytes at a time, the same arithmetic. */
FMRX_API int fmrx_leveller_process_dev(fmrx_leveller *h, const fmrx_audio_meters *am, const float *d_in, float *d_out, int16_t *d_pcm16,
                                       int pcm_policy, void *stream);
/* Host rows and host records [n_channels] (fmrx_audio_meters_collect's), synchronous (it first waits for the handle's last
 * call): the same kernels.  out must not overlap in; the device copies keep each host pointer's address modulo 16. */
FMRX_API int fmrx_leveller_process(fmrx_leveller *h, const fmrx_audio_meter *recs, const float *in, float *out, int16_t *pcm16,
                                   int pcm_policy);
/* out [n_channels]; waits for the handle's last call (an event it recorded), not for the device */
FMRX_API int fmrx_leveller_status_get(fmrx_leveller *h, fmrx_leveller_status *out);

/* ------------------------------------------------------------------ */
/* True-peak meter: the 4x oversampled peak (dBTP) of every audio row   */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  What EBU R 128 asks of programme that is monitored, recorded or restreamed: the maximum
 * true-peak level, the peak of the reconstructed waveform between the samples, which a DAC, a resampler or a codec downstream
 * overloads on and which a sample-peak reading (the audio meters' peak, the leveller's ceiling) misses by up to 3 dB at fs/4.
 * ... -> audio meters -> leveller -> true peak on one stream; it serves any rows of the banks' shape, the limiter's output
 * first.  A handle of the audio meters' kind that only reads the rows.  Defined by tests/_true_peak_model.py (DESIGN.md section
 * 4.16); host and device equal that model bit for bit (a NaN's sign and payload are the machine's).
 *
 * Interpolator: 4x oversampling, as ITU-R BS.1770-4 Annex 2 prescribes at 44.1 / 48 kHz, at whatever rate the row has.  Four
 * phases p of 12 taps over the samples x[k-5 .. k+6] give the waveform at k + p/4.  Phase 0 is the sample itself and no filter,
 * so a true peak is never below the sample peak of the same positions, exactly.  Phases 1 .. 3 are a Kaiser-windowed sinc
 * (beta = 5): H[p][j] = sinc(t) I0(5 sqrt(1 - (t/6)^2)) / I0(5), t = (j - 5) - p/4, computed in float64 and rounded once to
 * float32.  The float32 table (fmrx_true_peak_taps; literals in true_peak_core.hpp) is the definition; H[3] is H[1] reversed,
 * H[2] is symmetric.  Phase gain error 0.03 dB up to 0.36 fs; the only systematic under-read is the 4x grid's own, -0.44 dB at
 * 0.4 fs.
 * Groups: the row is a stream across calls with zeros in front of it.  When sample i arrives, group k = i - 6 is evaluated:
 *   v0 = |x[k]|;   for p = 1, 2, 3:  acc = +0;  for j = 0 .. 11 ascending: acc = fmaf(H[p][j], x[k-5+j], acc);  v_p = |acc|
 * every step rounded once, float32 denormals kept.  A call of n samples evaluates exactly n groups, negative k on a fresh stream
 * included; there is no special case at a stream's start.  The carried state per row is the last 11 samples (fresh: zeros); a
 * call with n < 11 shifts it.  The reading lags the audio by fmrx_true_peak_latency() = 6 samples.
 * Record per channel and call (fmrx_true_peak_record; arrays of 2 for the rows L and R, mono fills index 0 only):
 *   n             the call's samples per row
 *   over[r]       groups in which any of the four values v has !(v <= limit); NaN counts
 *   true_peak[r]  the maximum over all v of all groups, taken with v > m: it skips NaN and reads infinity for an infinity
 *   peak[r]       the maximum of v0 alone
 * limit is a finite positive float fixed at create, in the row's units (the library calls no pow; -1 dBTP at full scale 2.0 is
 * (float)(2.0 * 10^(-1/20))).  Records of successive calls add n and over and take the maximum of the peaks.  Nothing depends on
 * the order of evaluation: any split of a row over lanes, workgroups and calls gives the same merged record.
 * Levels (fmrx_true_peak_levels; fmrx_true_peak_derive, host arithmetic in double; full_scale as the audio meters'), every dB
 * value by the signal meters' edge rule:
 *   true_peak_dbtp[r]  10 log10(true_peak^2 / fs2)      peak_dbfs[r]  10 log10(peak^2 / fs2)      (-99 for a row a mono channel lacks)
 *   max_dbtp           the larger of the rows' true_peak_dbtp      over_fraction  (over[0] + over[1]) / (n audio_channels)
 *
 * The device pass: parallel in time -- the channel in the grid's x, a tile of fmrx_true_peak_tile() = 2048 samples in y -- so a
 * single long stream is as fast as a bank.  About 36 fused multiply-adds and 4 bytes per sample. */
typedef struct fmrx_true_peak_record {
    uint64_t n, over[2];
    double true_peak[2], peak[2];
} fmrx_true_peak_record;
typedef struct fmrx_true_peak_levels {
    double true_peak_dbtp[2], peak_dbfs[2], max_dbtp, over_fraction;
} fmrx_true_peak_levels;
#ifdef __cplusplus
static_assert(sizeof(fmrx_true_peak_record) == 56, "fmrx_true_peak_record layout");
static_assert(sizeof(fmrx_true_peak_levels) == 48, "fmrx_true_peak_levels layout");
#else
_Static_assert(sizeof(fmrx_true_peak_record) == 56, "fmrx_true_peak_record layout");
_Static_assert(sizeof(fmrx_true_peak_levels) == 48, "fmrx_true_peak_levels layout");
#endif
typedef struct fmrx_true_peak fmrx_true_peak;
/* Host code, no device needed.  taps: h36 [3][12] = H[1], H[2], H[3].  latency: 6 samples.  tile: the samples of a row one
 * workgroup walks. */
FMRX_API int fmrx_true_peak_taps(float *h36);
FMRX_API size_t fmrx_true_peak_latency(void);
FMRX_API size_t fmrx_true_peak_tile(void);
/* The host reference of one channel: rows [audio_channels][row_pitch] floats of which n (1 .. 2^26) are walked; state_in_out
 * [2][11] floats, the rows' last 11 samples, is read and replaced (a mono channel's second row is left alone); *rec is written.
 * limit finite and > 0, else FMRX_EINVAL.  The body the kernel runs (true_peak_core.hpp). */
FMRX_API int fmrx_true_peak_walk(int audio_channels, const float *rows, size_t row_pitch, size_t n, float limit, float *state_in_out,
                                 fmrx_true_peak_record *rec);
FMRX_API int fmrx_true_peak_derive(const fmrx_true_peak_record *rec, int audio_channels, double full_scale, fmrx_true_peak_levels *out);
/* n_audio: the most samples per row and call (fmrx_channels_n_audio), 1 .. 2^26; audio_channels 1 or 2; limit finite and > 0 */
FMRX_API int fmrx_true_peak_create(fmrx_true_peak **out, int n_channels, int audio_channels, size_t n_audio, float limit, int device);
FMRX_API int fmrx_true_peak_destroy(fmrx_true_peak *m);
/* channel < 0: all.  Clears the channel's carried samples.  Waits for the handle's last call; the state is clear when it returns,
 * for a later call on any stream. */
FMRX_API int fmrx_true_peak_reset(fmrx_true_peak *m, int channel);
/* out [n_channels][2][11] floats: every channel's carried samples (a mono channel's second row 0); waits for the handle's last
 * call */
FMRX_API int fmrx_true_peak_state_get(fmrx_true_peak *m, float *out);
/* Asynchronous on `stream`, behind whatever wrote the rows on the same stream: d_audio [n_channels][audio_channels][row_pitch]
 * floats, as the banks and every later stage write them (row_pitch = n_audio there), of which the first n <= n_audio of every
 * row are walked; 4-byte aligned.  Rows that are 16-byte aligned (d_audio is, and row_pitch is a multiple of 4) are fetched in
 * 16-byte pieces, all others 4 bytes at a time, the same arithmetic.  The rows are only read.  A clear of the results and one
 * kernel launch; a second call before fmrx_true_peak_collect replaces the results (the state has then advanced by both). */
FMRX_API int fmrx_true_peak_process_dev(fmrx_true_peak *m, const float *d_audio, size_t row_pitch, size_t n, void *stream);
/* records [n_channels]; waits for the last call (an event it recorded), not for the device */
FMRX_API int fmrx_true_peak_collect(fmrx_true_peak *m, fmrx_true_peak_record *records);
/* host rows [n_channels][audio_channels][row_pitch], synchronous (it first waits for the handle's last call): the single-stream
 * use is n_channels = 1 with the audio fmrx_pipeline_process returns */
FMRX_API int fmrx_true_peak_process(fmrx_true_peak *m, const float *audio, size_t row_pitch, size_t n, fmrx_true_peak_record *records);

/* ------------------------------------------------------------------ */
/* Audio spectrum meter: band powers of every audio row of a bank       */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  What the audio consists of: the power in up to 32 frequency bands of each audio row, from
 * which a monitor reads a band-limited relay, mains hum, pilot leakage, speech against music, or the flat hiss of an empty
 * channel.  ... -> audio meters -> leveller -> true peak / audio spectrum on one stream; a handle of the audio meters' kind that
 * only reads the rows.  Defined by tests/_audio_spectrum_model.py; host and device equal that model bit
 * for bit (a NaN's sign and payload are the machine's).
 *
 * Frames: a row is a stream across calls.  Frame f covers stream samples 256 f .. 256 f + 255; no overlap, nothing in front of a
 * fresh stream.  The carried state per channel (fmrx_audio_spectrum_state) is fill (0 .. 255, one value for both rows) and the
 * fill samples of the open frame per row.  A call of n samples completes F = (fill + n) div 256 frames and leaves (fill + n) mod
 * 256 samples; a call may complete no frame (frames = 0, every band +0).
 * Tables (float32, fmrx_audio_spectrum_tables; literals in audio_spectrum_core.hpp; they are the definition):
 *   w[j] = (float)(0.5 - 0.5 cos(2 pi j / 256)), the periodic Hann window, w[0] = +0
 *   C[m] = (float)cos(2 pi m / 256), m = 0 .. 255, built from the quarter m = 0 .. 64 by symmetry, C[64] = C[192] = +0 exactly
 * Per frame and row: xw[j] = x[j] w[j], one float32 multiply; for bins k = 0 .. 127
 *   re_k = acc = +0;  for j = 0 .. 255 ascending: acc = fmaf(C[(k j) mod 256], xw[j], acc)
 *   im_k = the same chain with C[(k j - 64) mod 256]
 *   p_k  = fmaf(im_k, im_k, fl(re_k re_k))
 * every step rounded once, float32 denormals kept; NaN and infinity propagate as the arithmetic has them: a NaN sample
 * makes every bin of its frame NaN, an infinite one NaN or infinity (NaN where it meets one of the zeros w[0], C[64], C[192]).
 * Bands: edges[0 .. B] strictly ascending within 1 .. 128, 1 <= B <= 32; band b covers bins edges[b] .. edges[b+1] - 1; bin 0 is
 * computed and belongs to no band.  A frame's band power is the float32 sum of its p_k, ascending from +0.  The default
 * (fmrx_audio_spectrum_default_edges) has 23 bands, edges 1 2 3 4 5 6 7 8 10 12 14 16 20 24 28 32 40 48 56 64 80 96 112 128: at
 * 48 kHz a bin is 187.5 Hz and the 19 kHz pilot falls in band 21.
 * Record per channel and call (fmrx_audio_spectrum_record; mono fills row 0; bands >= B are +0): n, frames, and
 *   band[r][b]  a two-level float64 sum: the call's completed frames q = 0 .. F - 1 form tiles of fmrx_audio_spectrum_tile() = 16
 *               consecutive frames; a tile's sum runs over its frames ascending from +0.0, the call's over its tiles ascending
 *               from +0.0
 * The per-frame band powers do not depend on how the stream is cut into calls.  The sums DO, through this grouping: the same
 * stream cut into other calls groups other frames into tiles, and the records' sum over the calls can differ in its last bits.
 * Records of successive calls add.
 * Levels (fmrx_audio_spectrum_levels; fmrx_audio_spectrum_derive, host arithmetic in double), every dB value by the signal
 * meters' edge rule, clamped to +-99:
 *   band_dbfs[r][b]  10 log10((band / frames) / (6144 full_scale^2)); 6144 = 256 sum(w^2) / 4, so that a full-scale sine whose
 *                    main lobe lies inside a band reads 0 dBFS there
 *   total_dbfs[r]    the same over the sum of the bands
 *   centroid_hz[r]   sum_b fc_b band_b / sum_b band_b, fc_b = (edges[b] + edges[b+1] - 1) / 2 audio_Fs / 256; 0 where the total is
 *                    not positive
 * With frames = 0, for the row a mono channel lacks and for bands >= B every level reads -99 and the centroid 0.
 *
 * The device pass: a frame's 2 x 128 chains are a matrix product on the f32 matrix cores (v_mfma_f32_16x16x4_f32: 16 outputs x 4
 * window positions x 16 frames), which rounds as the chain above does.  Rows of at most 2 048 samples -- every bank row -- take
 * one workgroup per two rows and one launch; longer rows one workgroup per 16 frames and a second small launch for the tiles'
 * sum. */
typedef struct fmrx_audio_spectrum_record {
    uint64_t n, frames;
    double band[2][32];
} fmrx_audio_spectrum_record;
typedef struct fmrx_audio_spectrum_state {
    uint32_t fill;
    float carry[2][255];    /* entries at and beyond fill read 0, and so does a mono channel's second row */
} fmrx_audio_spectrum_state;
typedef struct fmrx_audio_spectrum_levels {
    double band_dbfs[2][32], total_dbfs[2], centroid_hz[2];
} fmrx_audio_spectrum_levels;
#ifdef __cplusplus
static_assert(sizeof(fmrx_audio_spectrum_record) == 528, "fmrx_audio_spectrum_record layout");
static_assert(sizeof(fmrx_audio_spectrum_state) == 2044, "fmrx_audio_spectrum_state layout");
static_assert(sizeof(fmrx_audio_spectrum_levels) == 544, "fmrx_audio_spectrum_levels layout");
#else
_Static_assert(sizeof(fmrx_audio_spectrum_record) == 528, "fmrx_audio_spectrum_record layout");
_Static_assert(sizeof(fmrx_audio_spectrum_state) == 2044, "fmrx_audio_spectrum_state layout");
_Static_assert(sizeof(fmrx_audio_spectrum_levels) == 544, "fmrx_audio_spectrum_levels layout");
#endif
typedef struct fmrx_audio_spectrum fmrx_audio_spectrum;
/* Host code, no device needed.  tables: window256 [256] = w, cos256 [256] = C.  frame 256, bins 128, tile 16, max_bands 32.
 * default_edges: edges [24], *n_bands = 23. */
FMRX_API int fmrx_audio_spectrum_tables(float *window256, float *cos256);
FMRX_API size_t fmrx_audio_spectrum_frame(void);
FMRX_API size_t fmrx_audio_spectrum_bins(void);
FMRX_API size_t fmrx_audio_spectrum_tile(void);
FMRX_API size_t fmrx_audio_spectrum_max_bands(void);
FMRX_API int fmrx_audio_spectrum_default_edges(int *edges, int *n_bands);
/* The host reference of one channel: rows [audio_channels][row_pitch] floats of which n (1 .. 2^26) are walked; edges [n_bands + 1]
 * (NULL: the default, n_bands ignored); *state_in_out is read and replaced (a mono channel's second row is left alone); *rec is
 * written.  Edges that do not ascend strictly within 1 .. 128, n_bands outside 1 .. 32 or a fill beyond 255: FMRX_EINVAL.  The body
 * the kernel's arithmetic is checked against (audio_spectrum_core.hpp). */
FMRX_API int fmrx_audio_spectrum_walk(int audio_channels, const float *rows, size_t row_pitch, size_t n, const int *edges, int n_bands,
                                      fmrx_audio_spectrum_state *state_in_out, fmrx_audio_spectrum_record *rec);
/* edges, n_bands: those the record was made with (NULL: the default); audio_Fs finite and > 0, for the centroid */
FMRX_API int fmrx_audio_spectrum_derive(const fmrx_audio_spectrum_record *rec, int audio_channels, const int *edges, int n_bands, double audio_Fs,
                                        double full_scale, fmrx_audio_spectrum_levels *out);
/* n_audio: the most samples per row and call (fmrx_channels_n_audio), 1 .. 2^26; audio_channels 1 or 2; edges [n_bands + 1], NULL:
 * the default */
FMRX_API int fmrx_audio_spectrum_create(fmrx_audio_spectrum **out, int n_channels, int audio_channels, size_t n_audio, const int *edges, int n_bands,
                                        int device);
FMRX_API int fmrx_audio_spectrum_destroy(fmrx_audio_spectrum *m);
/* channel < 0: all.  Clears the channel's open frame (fill = 0).  Waits for the handle's last call; the state is clear when it
 * returns, for a later call on any stream. */
FMRX_API int fmrx_audio_spectrum_reset(fmrx_audio_spectrum *m, int channel);
/* out [n_channels]: every channel's carried state; waits for the handle's last call */
FMRX_API int fmrx_audio_spectrum_state_get(fmrx_audio_spectrum *m, fmrx_audio_spectrum_state *out);
/* Asynchronous on `stream`, behind whatever wrote the rows on the same stream: d_audio [n_channels][audio_channels][row_pitch]
 * floats, as the banks and every later stage write them (row_pitch = n_audio there), of which the first n <= n_audio of every
 * row are walked; 4-byte aligned, at any pitch.  A frame starts wherever the open frame's fill puts it, so the rows are fetched
 * 4 bytes per lane, consecutive lanes consecutive samples, whatever their alignment; the pass is bound by the matrix cores.  The
 * rows are only read.  One kernel launch (two for n > 2048); a second call before fmrx_audio_spectrum_collect replaces the results
 * (the state has then advanced by both). */
FMRX_API int fmrx_audio_spectrum_process_dev(fmrx_audio_spectrum *m, const float *d_audio, size_t row_pitch, size_t n, void *stream);
/* records [n_channels]; waits for the last call (an event it recorded), not for the device */
FMRX_API int fmrx_audio_spectrum_collect(fmrx_audio_spectrum *m, fmrx_audio_spectrum_record *records);
/* host rows [n_channels][audio_channels][row_pitch], synchronous (it first waits for the handle's last call): the single-stream
 * use is n_channels = 1 with the audio fmrx_pipeline_process returns */
FMRX_API int fmrx_audio_spectrum_process(fmrx_audio_spectrum *m, const float *audio, size_t row_pitch, size_t n, fmrx_audio_spectrum_record *records);

/* ------------------------------------------------------------------ */
/* Audio feature frames: a mel-band spectrogram of every channel        */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference.  Every stage above reduces a channel and call to one record; what a monitor does next --
 * speech against music, speech-to-text, jingle and advert detection, programme fingerprinting -- starts from a time series: a
 * mel-band spectrogram at a 10 ms hop.  This stage leaves it on the device as a tensor [n_channels][frames][n_mels] that a
 * model reads by pointer, without the samples leaving the card.  ... -> leveller -> true peak / audio spectrum / audio features
 * on one stream; a handle of the audio meters' kind that only reads the rows.  Defined by tests/_audio_features_model.py
 * (DESIGN.md section 4.18); the host walk and the device equal that model bit for bit (a NaN's sign and payload are the machine's).
 *
 * Geometry (fmrx_audio_features_params, set at create): win, the frame length in samples, a multiple of 4 within 16 .. 1280; hop
 * 1 .. win; n_bins 1 .. min(256, win / 2), bins 0 .. n_bins - 1 of a DFT of period win; n_mels 1 .. 128; 0 <= f_lo < f_hi <=
 * audio_Fs / 2, all finite.  Anything else: FMRX_EINVAL.  fmrx_audio_features_preset fills in the speech-model geometry:
 *   audio_Fs 48 000: win 1200 (25 ms), hop 480 (10 ms), 201 bins, 80 mels, 0 .. 8 kHz: bin k sits at 40 k Hz, the bins of a 400-point
 *                    DFT of the signal at 16 kHz, with no resampler and no aliasing
 *   audio_Fs 44 100: win 1104, hop 441, 201 bins (39.95 Hz apart), 80 mels, 0 .. 8 kHz
 * and refuses any other rate.
 * Tables (float32, made on the host in double and rounded once; what fmrx_audio_features_tables returns is the definition):
 *   w[j] = 0.5 - 0.5 cos(2 pi j / win), the periodic Hann window, w[0] = +0, w[win - j] = w[j]
 *   C[m] = cos(2 pi m / win), m = 0 .. win - 1, unfolded from the quarter m = 0 .. win / 4 by symmetry (C[win/2 - m] = -C[m],
 *          C[win - m] = C[m]); C[win/4] = C[3 win/4] = +0 exactly
 *   mel filters on the Slaney scale (linear at 200/3 Hz per mel below 1 kHz, logarithmic with step ln(6.4)/27 above): n_mels + 2
 *          points f[i] equally spaced in mel from f_lo to f_hi; mel_w[b][k] = the triangle over f[b], f[b+1], f[b+2] at k audio_Fs /
 *          win, times the Slaney norm 2 / (f[b+2] - f[b]); mel_lo[b] .. mel_hi[b] - 1 are the contiguous bins whose weight is
 *          positive, lo = hi = 0 where there are none (that feature reads +0)
 * Per frame: samples m[j], j < win, of the mono mix: m = 0.5f (L + R) for a stereo channel (one float32 add, then an exact
 * halving), row 0 for a mono one.  xw[j] = m[j] w[j]; for bins k = 0 .. n_bins - 1
 *   re_k = acc = +0;  for j = 0 .. win - 1 ascending: acc = fmaf(C[(k j) mod win], xw[j], acc)
 *   im_k = the same chain with C[(k j - win/4) mod win]
 *   p_k  = fmaf(im_k, im_k, fl(re_k re_k))
 *   feat[b] = acc = +0;  for k = mel_lo[b] .. mel_hi[b] - 1 ascending: acc = fmaf(mel_w[b][k], p_k, acc)
 * every step rounded once, float32 denormals kept; NaN and infinity propagate as the arithmetic has them.  The output is linear
 * mel power; the logarithm is the caller's.
 * Frames: a row is a stream across calls.  Frame f covers stream samples f hop .. f hop + win - 1; nothing stands in front of a
 * fresh stream (no centre padding).  The carried state per channel (fmrx_audio_features_state) is fill (0 .. win - 1) and the fill
 * samples of the mono mix.  A call of n samples has T = fill + n; it completes F = 0 frames if T < win, else (T - win) div hop + 1,
 * and carries T - F hop samples.  At most F_max = (n_audio - 1) div hop + 1 frames complete per call
 * (fmrx_audio_features_max_frames; 4 for a bank row of 1 920 at the preset).  The frames do not depend on how a stream is cut
 * into calls: the same stream cut differently gives the same frames, byte for byte.
 * Results per call: feat [n_channels][F_max][n_mels] float32, frames >= F of a channel +0, and frames [n_channels] uint32, on
 * the device (fmrx_audio_features_result_dev) and, on request, on the host (fmrx_audio_features_collect).
 *
 * The device pass: a frame's 2 n_bins chains are a matrix product on the f32 matrix cores (v_mfma_f32_16x16x4_f32: 16 outputs x 4
 * window positions x 16 frames), which rounds as the chains above do.  The 16 columns of a workgroup are consecutive entries of
 * the flattened (channel, frame < F_max) list, so a tile spans several channels and a long row many tiles; one launch. */
typedef struct fmrx_audio_features_params {
    uint32_t win, hop, n_bins, n_mels;
    double f_lo, f_hi, audio_Fs;
} fmrx_audio_features_params;
typedef struct fmrx_audio_features_state {
    uint32_t fill;
    float carry[1279];      /* the mono mix; entries at and beyond fill read 0 */
} fmrx_audio_features_state;
#ifdef __cplusplus
static_assert(sizeof(fmrx_audio_features_params) == 40, "fmrx_audio_features_params layout");
static_assert(sizeof(fmrx_audio_features_state) == 5120, "fmrx_audio_features_state layout");
#else
_Static_assert(sizeof(fmrx_audio_features_params) == 40, "fmrx_audio_features_params layout");
_Static_assert(sizeof(fmrx_audio_features_state) == 5120, "fmrx_audio_features_state layout");
#endif
typedef struct fmrx_audio_features fmrx_audio_features;
/* Host code, no device needed.  preset: audio_Fs 48000 or 44100.  tables: window [win], cosine [win], mel_lo [n_mels], mel_hi
 * [n_mels], mel_w [n_mels][n_bins].  max_frames: F_max of a call of n_audio samples; 0 for a refused geometry or n_audio = 0. */
FMRX_API int fmrx_audio_features_preset(double audio_Fs, fmrx_audio_features_params *params);
FMRX_API int fmrx_audio_features_tables(const fmrx_audio_features_params *params, float *window, float *cosine, int32_t *mel_lo, int32_t *mel_hi,
                                        float *mel_w);
FMRX_API size_t fmrx_audio_features_max_frames(const fmrx_audio_features_params *params, size_t n_audio);
/* The host reference of one channel: rows [audio_channels][row_pitch] floats of which n (1 .. 2^26) are walked; *state_in_out is
 * read and replaced (a fill of win or more: FMRX_EINVAL); feat [max_frames(params, n)][n_mels] is written whole, frames the call
 * did not complete +0; *frames is the count F.  The body the kernel's arithmetic is checked against (audio_features_core.hpp). */
FMRX_API int fmrx_audio_features_walk(const fmrx_audio_features_params *params, int audio_channels, const float *rows, size_t row_pitch, size_t n,
                                      fmrx_audio_features_state *state_in_out, float *feat, uint32_t *frames);
/* n_audio: the most samples per row and call (fmrx_channels_n_audio), 1 .. 2^26; audio_channels 1 or 2 */
FMRX_API int fmrx_audio_features_create(fmrx_audio_features **out, const fmrx_audio_features_params *params, int n_channels, int audio_channels,
                                        size_t n_audio, int device);
FMRX_API int fmrx_audio_features_destroy(fmrx_audio_features *m);
/* channel < 0: all.  Clears the channel's carried samples (fill = 0): its stream starts anew.  Waits for the handle's last call;
 * the state is clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_audio_features_reset(fmrx_audio_features *m, int channel);
/* out [n_channels]: every channel's carried state; waits for the handle's last call */
FMRX_API int fmrx_audio_features_state_get(fmrx_audio_features *m, fmrx_audio_features_state *out);
/* Asynchronous on `stream`, behind whatever wrote the rows on the same stream: d_audio [n_channels][audio_channels][row_pitch]
 * floats, as the banks and every later stage write them (row_pitch = n_audio there), of which the first n <= n_audio of every
 * row are walked; 4-byte aligned, at any pitch.  The rows are only read.  One kernel launch and no copy; a second call before
 * fmrx_audio_features_collect replaces the results (the state has then advanced by both). */
FMRX_API int fmrx_audio_features_process_dev(fmrx_audio_features *m, const float *d_audio, size_t row_pitch, size_t n, void *stream);
/* The last call's results where the kernel left them: *d_feat [n_channels][F_max][n_mels] floats, *d_frames [n_channels].  The
 * pointers are the handle's and hold until it is destroyed; their contents are the last call's, ordered behind it on its stream,
 * until the handle's next call.  This is the tensor a torch consumer wraps. */
FMRX_API int fmrx_audio_features_result_dev(fmrx_audio_features *m, const float **d_feat, const uint32_t **d_frames);
/* feat [n_channels][F_max][n_mels], frames [n_channels], to the host; waits for the last call (an event it recorded), not for
 * the device */
FMRX_API int fmrx_audio_features_collect(fmrx_audio_features *m, float *feat, uint32_t *frames);
/* host rows [n_channels][audio_channels][row_pitch], synchronous (it first waits for the handle's last call), then as collect */
FMRX_API int fmrx_audio_features_process(fmrx_audio_features *m, const float *audio, size_t row_pitch, size_t n, float *feat, uint32_t *frames);

/* ------------------------------------------------------------------ */
/* Audio rate converter: a bank's audio at 16 kHz mono or any rate U/D  */
/* ------------------------------------------------------------------ */
/* No counterpart in the reference (its resampler is the IF-to-audio stage inside the pipeline).  A bank writes 48 or 44.1 kHz;
 * speech models, voice-activity detectors and loggers take 16 kHz mono, fingerprinters 8 .. 11 kHz, a restream 32 or 44.1 kHz.
 * This stage converts every channel's audio, the mono mix or each row, by a polyphase FIR at a rational rate up / down, carries
 * its history and phase from call to call and leaves the samples on the device as [n_channels][R][M_max] float32 and / or s16
 * that a model reads by pointer.  ... -> leveller -> true peak / audio spectrum / audio features / audio resample on one stream; a
 * handle of the audio meters' kind that only reads the rows.  Defined by tests/_audio_resample_model.py;
 * the host walk and the device equal that model bit for bit (a NaN's sign and payload are the machine's).
 *
 * Geometry (fmrx_audio_resample_params, set at create): up 1 .. 160, down 1 .. 1024, gcd(up, down) = 1; taps T, the input samples
 * an output reads, a multiple of 4 within 8 .. 256 with up taps <= 16 384; mix 0 or 1; 0 < cutoff <= 1; 0 <= beta <= 20.  Anything
 * else, or a double that is not finite: FMRX_EINVAL.  fmrx_audio_resample_preset(audio_Fs, out_Fs, mix) fills it in for two integer
 * rates within 8 000 .. 48 000: up / down = out_Fs / audio_Fs reduced, taps = 4 ceil(24 / min(1, up / down) / 4) (twelve zero
 * crossings a side), cutoff 0.9, beta 8; it refuses other rates and ratios beyond the limits.
 *   48 000 -> 16 000: 1/3, T 72     -> 8 000: 1/6, T 144      -> 24 000: 1/2, T 48     -> 32 000: 2/3, T 36     -> 44 100: 147/160, T 28
 *   44 100 -> 16 000: 160/441, T 68      -> 22 050: 1/2, T 48      -> 48 000: 160/147, T 24
 * Taps (float32, made on the host in double and rounded once; what fmrx_audio_resample_taps returns, [up][taps] phase-major, is
 * the definition): with L = up T, c = (L - 1) / 2, w = cutoff min(1, up / down), for k < L
 *   g[k] = w sinc(w (k - c) / up) I0(beta sqrt(1 - ((k - c) / (L / 2))^2)) / I0(beta),   h[p][j] = g[j up + p]
 * Input: with mix = 1 one row per channel is converted: 0.5f (L + R) for a stereo channel (one float32 add, then an exact
 * halving), row 0 for a mono one.  With mix = 0 every row is converted by itself.  R is 1 with mix, else audio_channels.
 * An output: a row is a stream across calls, x[s], s >= 0, with x[s < 0] = +0.  Output m reads the newest input i = (m down) div up
 * at phase p = (m down) mod up:
 *   y[m] = acc = +0;  for j = 0 .. T - 1 ascending: acc = fmaf(h[p][j], x[i - j], acc)
 * every step rounded once, float32 denormals kept; NaN and infinity propagate as this arithmetic has them and no further: a
 * sample that is not finite reaches the outputs whose T-sample window holds it.  The group delay is
 * fmrx_audio_resample_latency() = (L - 1) / (2 up) input samples.
 * Calls and state: a call brings n inputs.  pos (0 .. down - 1) is the carried position of the next output in units of 1 / up input
 * sample from the call's first sample; output q of the call has t = pos + q down, i = t div up, p = t mod up.  The call completes
 * M = ceil((n up - pos) / down) outputs if n up > pos, else 0, and leaves pos' = pos + M down - n up; at most M_max = ceil(n_audio
 * up / down) complete (fmrx_audio_resample_max_out).  All of this is 64-bit arithmetic.  The state (fmrx_audio_resample_state) is
 * pos and, per converted row, the last T - 1 samples (the mixed ones with mix), oldest first, zeros in front of a fresh stream;
 * entries from T - 1 on and the rows a channel does not convert read 0.  A call shorter than T - 1 shifts it.  The same stream cut
 * differently into calls gives the same samples, byte for byte.
 * Results per call: out_f32 and / or out_pcm [n_channels][R][M_max], entries at and beyond a channel's count +0 / 0, and counts
 * [n_channels] uint32.  The PCM is the pipeline's pack of the float value (FMRX_PCM_WRAP / FMRX_PCM_SATURATE), the policy given
 * per call.  Which of the two a handle keeps is chosen at create (want_f32, want_pcm; at least one).
 *
 * The device pass: parallel in time, the channel in the grid's x and a tile of up to 1 024 outputs in y; a workgroup stages the
 * tile's input window and the tap table in LDS and every lane runs two outputs' chains in the halves of packed fmas. */
typedef struct fmrx_audio_resample_params {
    uint32_t up, down, taps, mix;
    double cutoff, beta;
} fmrx_audio_resample_params;
typedef struct fmrx_audio_resample_state {
    uint32_t pos, reserved;
    float carry[2][255];    /* per converted row the last taps - 1 samples, oldest first; the rest reads 0 */
} fmrx_audio_resample_state;
#ifdef __cplusplus
static_assert(sizeof(fmrx_audio_resample_params) == 32, "fmrx_audio_resample_params layout");
static_assert(sizeof(fmrx_audio_resample_state) == 2048, "fmrx_audio_resample_state layout");
#else
_Static_assert(sizeof(fmrx_audio_resample_params) == 32, "fmrx_audio_resample_params layout");
_Static_assert(sizeof(fmrx_audio_resample_state) == 2048, "fmrx_audio_resample_state layout");
#endif
typedef struct fmrx_audio_resample fmrx_audio_resample;
/* Host code, no device needed.  preset: see above.  taps: h [up][taps].  max_out: M_max of a call of n_audio samples; 0 for a refused
 * geometry or n_audio = 0.  latency: (up taps - 1) / (2 up) input samples; a NaN for a refused geometry. */
FMRX_API int fmrx_audio_resample_preset(double audio_Fs, double out_Fs, int mix, fmrx_audio_resample_params *params);
FMRX_API int fmrx_audio_resample_taps(const fmrx_audio_resample_params *params, float *h);
FMRX_API size_t fmrx_audio_resample_max_out(const fmrx_audio_resample_params *params, size_t n_audio);
FMRX_API double fmrx_audio_resample_latency(const fmrx_audio_resample_params *params);
/* The host reference of one channel: rows [audio_channels][row_pitch] floats of which n (1 .. 2^26) are walked; *state_in_out is
 * read and replaced (a pos of down or more: FMRX_EINVAL); out [R][max_out(params, n)] is written whole, entries the call did not
 * complete +0; *count is M.  The bodies the kernel runs (audio_resample_core.hpp). */
FMRX_API int fmrx_audio_resample_walk(const fmrx_audio_resample_params *params, int audio_channels, const float *rows, size_t row_pitch, size_t n,
                                      fmrx_audio_resample_state *state_in_out, float *out, uint32_t *count);
/* n_audio: the most samples per row and call (fmrx_channels_n_audio), 1 .. 2^26; audio_channels 1 or 2; want_f32, want_pcm: the
 * results the handle keeps, at least one.  A geometry and n_audio whose M_max needs more than 65 535 tiles per row: FMRX_EINVAL. */
FMRX_API int fmrx_audio_resample_create(fmrx_audio_resample **out, const fmrx_audio_resample_params *params, int n_channels, int audio_channels,
                                        size_t n_audio, int want_f32, int want_pcm, int device);
FMRX_API int fmrx_audio_resample_destroy(fmrx_audio_resample *m);
/* channel < 0: all.  Clears the channel's carried samples and position: its stream starts anew.  Waits for the handle's last call;
 * the state is clear when it returns, for a later call on any stream. */
FMRX_API int fmrx_audio_resample_reset(fmrx_audio_resample *m, int channel);
/* out [n_channels]: every channel's carried state; waits for the handle's last call */
FMRX_API int fmrx_audio_resample_state_get(fmrx_audio_resample *m, fmrx_audio_resample_state *out);
/* Asynchronous on `stream`, behind whatever wrote the rows on the same stream: d_audio [n_channels][audio_channels][row_pitch]
 * floats, as the banks and every later stage write them (row_pitch = n_audio there), of which the first n <= n_audio of every
 * row are walked; 4-byte aligned, at any pitch.  Rows that are 16-byte aligned (d_audio is, and row_pitch is a multiple of 4) are
 * fetched in 16-byte pieces, all others 4 bytes per lane, the same arithmetic.  The rows are only read.  One kernel launch and no
 * copy; a second call before fmrx_audio_resample_collect replaces the results (the state has then advanced by both). */
FMRX_API int fmrx_audio_resample_process_dev(fmrx_audio_resample *m, const float *d_audio, size_t row_pitch, size_t n, int pcm_policy, void *stream);
/* The last call's results where the kernel left them: *d_f32 and *d_pcm [n_channels][R][M_max] (NULL for the one the handle does
 * not keep), *d_counts [n_channels].  The pointers are the handle's and hold until it is destroyed; their contents are the last
 * call's, ordered behind it on its stream, until the handle's next call.  These are the tensors a torch consumer wraps. */
FMRX_API int fmrx_audio_resample_result_dev(fmrx_audio_resample *m, const float **d_f32, const int16_t **d_pcm, const uint32_t **d_counts);
/* out_f32 and out_pcm [n_channels][R][M_max] (either may be NULL; one the handle does not keep must be), counts [n_channels], to the
 * host; waits for the last call (an event it recorded), not for the device */
FMRX_API int fmrx_audio_resample_collect(fmrx_audio_resample *m, float *out_f32, int16_t *out_pcm, uint32_t *counts);
/* host rows [n_channels][audio_channels][row_pitch], synchronous (it first waits for the handle's last call), then as collect */
FMRX_API int fmrx_audio_resample_process(fmrx_audio_resample *m, const float *audio, size_t row_pitch, size_t n, int pcm_policy, float *out_f32,
                                         int16_t *out_pcm, uint32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* FMRX_H */
