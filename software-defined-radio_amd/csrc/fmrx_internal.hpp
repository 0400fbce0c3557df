// fmrx_internal.hpp -- shared declarations for libfmrx.so (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fmrx.h"

namespace fmrx {

// ---- error plumbing -------------------------------------------------------
int fail(int code, const char *fmt, ...);

#define FMRX_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::fmrx::fail(FMRX_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                           \
    } while (0)

#define FMRX_TRY(expr)              \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != FMRX_OK) return rc_; \
    } while (0)

// after every kernel launch: FMRX_LAUNCH_CHECK("kernel<%d,%d>", T, D) (a literal and its arguments) makes the enclosing function
// return FMRX_EHIP, "launch kernel<101,10>: <HIP's words>", if the launch was refused
#define FMRX_LAUNCH_CHECK(name, ...)                                                                                              \
    do {                                                                                                                          \
        hipError_t e_ = hipGetLastError();                                                                                        \
        if (e_ != hipSuccess) return ::fmrx::fail(FMRX_EHIP, "launch " name ": %s", ##__VA_ARGS__, hipGetErrorString(e_));        \
    } while (0)

// true when at least one HIP device is usable; otherwise sets the error and
// the caller returns FMRX_ENODEV.  There is deliberately no CPU path.
int require_device();

// ---- run-time options (options.cpp) ------------------------------------------------
// Process-wide defaults: the built-in values below, overridden ONCE (first use) by the environment variable FMRX_<NAME IN
// CAPITALS> of each, changed afterwards only through fmrx_set_option().  A pipeline handle copies the defaults when it is
// created and keeps its own set (fmrx_pipeline_set_option); nothing on a per-block launch path reads the environment.
// Names, ranges, named values and what each option means: the table in options.cpp (one row per member).
struct Options {
    int fe_variant = 0, tuner_variant = 0, demod = 0, overlap_calls = 0;
    long fused_min_audio = 65536;
    int resample_l2 = 0, resample_exact = 0, resample_chains = 0;
    int pll_warmup = -1, pll_segment = -1, pll_start = 1, pll_mode = 0;
    int deemph_warmup = -1, deemph_segment = -1, deemph_mode = 0;
};
Options &default_options();      // callers hold options_mutex()
std::mutex &options_mutex();     // guards writes to the process-wide defaults and the copy a new handle takes
Options options_snapshot();      // the defaults, copied under the mutex: what handle constructors and stage functions use
// by name, through the table; FMRX_EINVAL for an unknown name or a value outside the option's range
int set_option_in(Options &o, const char *name, long value);
int get_option_in(const Options &o, const char *name, long *value);

// ---- small RAII device buffer ----------------------------------------------
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int alloc(size_t count)
    {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), count * sizeof(T));
        if (e != hipSuccess) return fail(FMRX_ENOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
        n = count;
        return FMRX_OK;
    }
    int ensure(size_t count) { return count <= n ? FMRX_OK : alloc(count); }
    size_t bytes() const { return n * sizeof(T); }
};

// ---- and its pinned host counterpart: where a call's asynchronous copies land ----------
template <typename T>
struct HostBuf {
    T *p = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    int alloc(size_t count)   // once per buffer
    {
        FMRX_HIP(hipHostMalloc(reinterpret_cast<void **>(&p), count * sizeof(T), hipHostMallocDefault));
        n = count;
        return FMRX_OK;
    }
    size_t bytes() const { return n * sizeof(T); }
};

// ---- front-end fast path (kernels_fe.hip) -----------------------------------
// Device-side tap table for the register-window FIR: phase-major, padded,
// pre-scaled.  See kernels_fe.hip for the layout.
struct AudioPlan;
struct FePlan {
    int taps = 0, decim = 0;
    bool fast = false;         // a specialised kernel exists for (taps, decim)
    int hist_bytes = 0;        // bytes of u8 history the kernel reads before the block (multiple of 16)
    DevBuf<float> table;       // fast-path table
    DevBuf<float> h;           // plain taps (generic path)
    // matrix-core kernel (kernels_fe_mfma.hip): taps as int8 digit fragments + the scale that undoes them
    bool mfma = false;
    DevBuf<int32_t> a_img;
    float scale_lo = 0.0f;
    DevBuf<uint8_t> silence;   // hist_bytes bytes of 128: the history of a stream that starts here
};
constexpr int kFeMfmaDigits = 3;   // base-256 digits per tap: 24-bit fixed point
int fe_plan_init(FePlan &pl, const float *h, int taps, int decim);
// Matrix-core front end + discriminator: same contract as fe_demod_launch; d_demod may be NULL when
// only the IF stream is wanted (d_if != NULL).
int fe_mfma_plan_init(FePlan &pl, const float *h, int taps, int decim);
bool fe_mfma_available(const FePlan &pl, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist);
int fe_mfma_launch(const FePlan &pl, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist, const float *d_prev,
                   float *d_demod, float *d_if, float *d_prev_out, uint8_t *d_hist_next, const Options &o, hipStream_t stream,
                   const float *d_dhist_src = nullptr, float *d_dhist_dst = nullptr, int dhist_n = 0);
// (d_dhist_src -> d_dhist_dst, dhist_n floats: the discriminator history copied in front of this block's output by the kernel itself)
// the same kernel over a bank of receivers' slots (bank.hip): see kernels_fe_mfma.hip
int fe_mfma_bank_lead(const FePlan &pl);   // bytes of the stream a row needs in front of its block
int fe_mfma_bank_launch(const FePlan &pl, const uint8_t *d_slots, long total_bytes, long in_pitch, long block_off, int n_channels,
                        long k_lo, long k_hi, float *d_demod, long out_pitch, long out_off, hipStream_t stream);
// d_hist: hist_bytes bytes whose LAST 2*(taps-1) hold the previous samples.
// Writes n_samples/decim float2 (I,Q) to d_if.
int fe_launch(const FePlan &pl, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist, float *d_if,
              const Options &o, hipStream_t stream, bool force_generic);
int fe_hist_bytes(int taps, int decim);
// Fused front end + discriminator (the pipeline's kernel).  d_demod[n/decim] is
// written; d_if (interleaved I,Q) and d_prev_out (float2 = IF[n/decim-1]) are
// optional; d_prev_override (float2) replaces the recomputed IF[-1] when given.
bool fe_fused_available(const FePlan &pl, const uint8_t *d_iq, size_t n_samples);
// d_hist_next (optional, hist_bytes bytes, requires 2*n_samples >= hist_bytes): the kernel also leaves
// the block's last bytes there for the next block.
int fe_demod_launch(const FePlan &pl, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist,
                    const float *d_prev_override, float *d_demod, float *d_if, float *d_prev_out,
                    uint8_t *d_hist_next, const Options &o, hipStream_t stream);

// ---- audio fast path (kernels_audio.hip) --------------------------------------
struct AudioPlan {
    int taps = 0, decim = 0;
    bool fast = false;
    DevBuf<float> table;
    DevBuf<float> h;
    DevBuf<float> mfma_table;  // Toeplitz image for the fused mono kernel (kernels_fe_mfma.hip)
};
// Fused mono chain (modes 0/1): u8 I/Q -> audio / PCM in one kernel; the discriminator output stays
// on chip except its last tail_keep samples, written to d_demod_tail[n_if - tail_keep .. n_if) for the
// next block.  d_dhist_end: one past the previous block's last discriminator sample; d_prev: its
// last IF sample (float2).
int audio_mfma_table_init(AudioPlan &pl, const float *h, int taps, int decim);
bool mono_fused_available(const FePlan &fe, const AudioPlan &au, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist);
int mono_fused_launch(const FePlan &fe, const AudioPlan &au, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist,
                      const float *d_prev, const float *d_dhist_end, float *d_demod_tail, int tail_keep, float *d_prev_out,
                      float *d_audio, int16_t *d_pcm, int wrap, uint8_t *d_hist_next, const Options &o, hipStream_t stream);
int audio_plan_init(AudioPlan &pl, const float *h, int taps, int decim);
// y[k] = sum_n h[n] * x[decim*k - n - delay]; x points at the block start and
// x[-(taps-1+delay+3) .. -1] must be readable history (the specialised kernel
// loads 16-byte chunks).
// Optionally also writes s16 PCM (d_pcm != nullptr).  d_hist_end (optional, specialised kernel only):
// one past the last sample of the previous block; when given, samples before d_x[0] are read from
// d_hist_end[-1], d_hist_end[-2], ... instead of d_x[-1], d_x[-2], ...
bool audio_fast_available(const AudioPlan &pl, const float *d_x);
int audio_fir_launch(const AudioPlan &pl, const float *d_x, const float *d_hist_end, size_t n_in, int delay, float *d_y,
                     int16_t *d_pcm, int wrap, hipStream_t stream, bool force_generic);

// ---- rational resampler (kernels_resample.hip) ------------------------------------
struct ResamplePlan {
    int taps = 0, decim = 0, upsamp = 0;
    int J = 0, JP = 0;         // taps per polyphase row, padded row length
    int span = 0;              // input samples one 256-output tile stages in LDS
    bool fast = false;
    // LDS-resident table kernel: the taps are applied in npass passes of W taps (all phases x W taps
    // fit LDS); tiles of 1024 outputs stage span_l inputs
    int npass = 0, W = 0, span_l = 0;
    DevBuf<float> table;       // polyphase-major taps [upsamp][JP]
    DevBuf<float> h;           // plain taps (generic path)
    // matrix-core kernel (pipeline path): tap image [tile][lane][K-step], K index 0 of every tile, tile groups
    bool mfma = false;
    int mfma_ks4 = 0, mfma_ngroups = 0, mfma_pieces = 0;
    bool mfma_reach_ok = false;   // piece staging stays within kResampleFront / kResampleBack of the block (else: element staging)
    mutable int mfma_wgs_per_cu[2] = {0, 0};   // resident workgroups per CU of the kernel instance in use (piece / element staging), asked once
    DevBuf<float> mfma_img;
    DevBuf<int> mfma_top, mfma_groups;   // per tile: K index 0's input offset; per group: m0, m1, lo, pieces
};
int resample_plan_init(ResamplePlan &pl, const float *h, int taps, int decim, int upsamp);
// exact: only the kernels that keep the reference's rounding sequence (the primitive's contract)
// d_pcm: also pack s16 PCM (d_y may then be null where resample_mfma_available(): that kernel writes either or both)
// margins: the caller vouches for finite, readable samples kResampleFront floats in front of d_x - delay and kResampleBack
// behind its n_in samples (the matrix-core kernel then stages every block alike; only taps that are zero meet those samples)
constexpr int kResampleFront = 256, kResampleBack = 1024;
int resample_launch(const ResamplePlan &pl, const float *d_x, size_t n_in, int delay, float *d_y, const Options &o,
                    hipStream_t stream, bool force_generic, bool exact = false, int16_t *d_pcm = nullptr, int wrap = 0,
                    bool margins = false);
bool resample_mfma_available(const ResamplePlan &pl, const float *d_x, size_t n_in, int delay, const Options &o);

// ---- stereo band-pass pair (kernels_stereo.hip) ------------------------------------
struct BpfPairPlan {
    int taps = 0;
    bool fast = false;
    DevBuf<float> table;        // interleaved reversed tap pairs (h_stereo, h_carrier)
    DevBuf<float> h_st, h_car;  // plain taps (generic path)
};
int bpf_pair_plan_init(BpfPairPlan &pl, const float *h_stereo, const float *h_carrier, int taps);
int bpf_pair_launch(const BpfPairPlan &pl, const float *d_x, size_t n, float *d_st, float *d_car, hipStream_t stream,
                    bool force_generic);

// everything behind the PLL of modes 0/1 in one kernel: mixer, both audio FIRs (mono branch on the all-passed
// discriminator output, stereo branch on the mixer output), L/R combine, PCM (kernels_stereo.hip)
bool stereo_out_available(int taps, int decim);
int stereo_out_launch(const float *d_demod, const float *d_bpf, const float *d_nco, const float *d_mix_tail_in,
                      float *d_mix_tail_out, int hm, size_t n_if, int delay, const float *d_h, int taps, int decim, float *d_mono,
                      float *d_st, float *d_left, float *d_right, int16_t *d_pcm, int wrap, float *d_mixer, hipStream_t stream);

// ---- generic kernels (kernels_generic.hip) ----------------------------------
// y[k] = sum_{n<taps} h[n]*x[decim*k - n], sequential mul+add in n (bit-compatible
// with the reference's evaluation order).  x[-(taps-1)..-1] must be readable.
int k_fir_generic(const float *d_x, size_t n_out, const float *d_h, int taps, int decim, float *d_y, hipStream_t s);
// same on interleaved u8 I/Q with (u-128)/128 fused; writes float2 (I,Q)
int k_fe_generic(const uint8_t *d_iq, const uint8_t *d_hist, int hist_bytes, size_t n_samples, const float *d_h,
                 int taps, int decim, float *d_if, hipStream_t s);
// polyphase resampler in stream form; d_x[-(hist)..-1] readable, hist=(taps-1)/upsamp
int k_resample_generic(const float *d_x, size_t n_in, const float *d_h, int taps, int decim, int upsamp, float *d_y,
                       hipStream_t s);
// demod[k] from interleaved IF (I,Q); IF[-1] = *d_prev (float2). Also stores IF[n-1] to d_prev_out when non-null.
// fast 1: the arithmetic of the fused audio kernel (demod_fast) instead of the reference order; 2: demod_fast_bounded
int k_fm_demod_if(const float *d_if, size_t n, const float *d_prev, float *d_prev_out, float *d_demod, int fast,
                  hipStream_t s);
int k_fm_demod_planar(const float *d_i, const float *d_q, size_t n, float prev_i, float prev_q, float *d_demod,
                      hipStream_t s);
// the model's arctangent demodulator (fmSupportLib.py:502-531), float64: out[k] = unwrap(atan2(Q[k], I[k]) - phase of the sample in
// front); planar double in / double out with the running phase `prev_phase` in front of sample 0 (stage API), and interleaved
// float IF in / float out with IF[-1] = *d_prev (pipeline option "demod" = 1)
int k_fm_demod_arctan_planar(const double *d_i, const double *d_q, size_t n, double prev_phase, double *d_out, hipStream_t s);
int k_fm_demod_arctan_if(const float *d_if, size_t n, const float *d_prev, float *d_demod, hipStream_t s);
int k_u8_to_f32(const uint8_t *d_raw, size_t n, float *d_out, hipStream_t s);
int k_deinterleave(const float *d_iq, size_t n_pairs, float *d_i, float *d_q, hipStream_t s);
int k_split_if(const float *d_if, size_t n, float *d_i, float *d_q, hipStream_t s);
int k_pcm16(const float *d_a, size_t n, int16_t *d_out, int wrap, hipStream_t s);
int k_pcm16_stereo(const float *d_l, const float *d_r, size_t n, int16_t *d_out, int wrap, hipStream_t s);
int k_all_pass(const float *d_in, size_t n, const float *d_state, size_t nstate, float *d_out, hipStream_t s);
// ---- pilot PLL (kernels_pll.hip) ----
// serial form.  fast == 0: the reference's recurrence with glibc's sinf/cosf/atan2f (glibc_libm.hpp) -- bit-identical
// to the reference given bit-identical input; fast != 0: shared double-precision argument reduction + hardware sin/cos
int k_fm_pll(const float *d_in, size_t n, float *d_out, float *d_state, float freq, float Fs, float ncoScale,
             float phaseAdjust, float normBandwidth, int fast, hipStream_t s);
// parallel-in-time form (fast math): segments with warm-up, each checked against its predecessor's end state
// within the merge tolerance below, serial repair where the loop was not locked.  Agrees with the serial
// trajectory to within the float32 grid of trigArg, not bit for bit (kernels_pll.hip).  d_scratch:
// pll_parallel_scratch_floats(n) floats; d_scratch[2] (as u32) counts segments that needed a repair (diagnostic).
// lane shape: L samples per lane, started at the last multiple of the loop's period that is >= W samples early
constexpr int kPllSegment = 64, kPllWarmup = 512, kPllSegmentMin = 32;
constexpr int kPllWarmupLti = 64;
// merge tolerance on the integrator in that mode, in Ki * ulp(trigArg): lanes 64 true steps from a noise-free start still differ
// from their neighbours by the loop's response to the float32 grid (2-3 Ki ulp), which the envelope of DESIGN section 2 contains
constexpr float kPllIntegTolUlpsLti = 6.0f;   // true steps a lane runs in front of its segment when it starts from the linear system's state (pll_start = 1)
constexpr int kPllHead = 1024;   // samples of a stream's first call walked serially (acquisition) before the lanes take over
// merge tolerance between a lane's warmed-up state and the true state (see kernels_pll.hip)
constexpr float kPllTolPhase = 1e-2f, kPllTolInteg = 1e-4f;
size_t pll_parallel_scratch_floats(size_t n);
// what a call of k_fm_pll_parallel ran: samples and warm-up samples per lane, whether the lanes started from the linear
// system, and its segments (0: the block was shorter than 4 L and the serial fast kernel ran)
struct PllParallelShape {
    int L, W;
    bool lti;
    long nseg;
};
int k_fm_pll_parallel(const float *d_in, size_t n, float *d_out, float *d_state, float freq, float Fs, float ncoScale,
                      float phaseAdjust, float normBandwidth, float *d_scratch, const Options &o, hipStream_t s,
                      double off_hint = -1.0,    // off_hint: IF samples of the stream in front of this call (the state's trigOffset), < 0 = unknown
                      int phases = 3, float *d_lti = nullptr, PllParallelShape *shape = nullptr);
// phases: 1 = only what depends on the input alone (the linear system's chunk records), 2 = the lanes and the repair, 3 = both;
// d_lti: where the chunk records live (pll_parallel_lti_floats(n) floats, 8-byte aligned) if not inside d_scratch -- a caller
// that runs phase 1 of its next call on another stream while phase 2 of this one reads them keeps two
size_t pll_parallel_lti_floats(size_t n);
// the merge tolerances pll_segments_kernel / pll_repair_kernel compute for a block of n samples whose state carries trig_offset
void pll_parallel_tolerances(float trig_offset, size_t n, float freq, float Fs, float normBandwidth, bool lti, float *tol_phase,
                             float *tol_integ);
// many channels, lane = channel, the exact serial recurrence (kernels_pll.hip); rows [channel][pitch], state 8 floats per channel
int k_fm_pll_channels(const float *d_in, long pitch_in, size_t n, int n_ch, float *d_trig, long pitch_trig, float *d_state,
                      float *d_nco0, float freq, float Fs, float ncoScale, float phaseAdjust, float normBandwidth, hipStream_t s,
                      bool flat = true,    // flat: the branch-free forms of glibc's functions (same values; false = A/B)
                      bool exact = true,   // false: the fast recurrence (closed-form phase detector, hardware sine / cosine) of the specialised path
                      bool in8 = false);   // fast only: d_in holds signed bytes (the input's sign; pitch_in in bytes)
int k_mix(const float *d_bpf, const float *d_pll, size_t n, float *d_mix, hipStream_t s);
int k_combine(const float *d_st, const float *d_mono, size_t n, float *d_l, float *d_r, hipStream_t s);
int k_upsample(const float *d_x, size_t n, float *d_xu, int up, hipStream_t s);
int k_downsample(const float *d_in, size_t n_out, float *d_out, int ds, hipStream_t s);
int k_fill_u8(uint8_t *d, size_t n, uint8_t v, hipStream_t s);
// diagnostics: out[i] = sinf / cosf / atan2f (fn 0 / 1 / 2) of a[i] (, b[i]) as the device evaluates glibc_libm.hpp
int k_libm_eval(int fn, const float *d_a, const float *d_b, size_t n, float *d_out, hipStream_t s);

// ---- de-emphasis (kernels_deemph.hip): y = one-pole IIR of x per row, parallel in time, bit-identical to the serial walk ----
constexpr int kDeemphSegment = 256, kDeemphWarmup = 256;   // built-in lane shape: samples per lane, warm-up samples in front
struct DeemphShape {
    int L = 0, W = 0;
    long nseg = 0;
};
DeemphShape deemph_shape(const Options &o, size_t n);
size_t deemph_scratch_floats(size_t rows, size_t n, const Options &o);
struct DeemphArgs {
    const float *x = nullptr;            // [rows][pitch_x], n samples per row
    long pitch_x = 0;
    float *y = nullptr;                  // [rows][pitch_y]; never x: the repair reads x again
    long pitch_y = 0;
    int16_t *pcm = nullptr;              // optional: [rows / ac][n][ac]
    int ac = 1, wrap = 0;
    size_t rows = 0, n = 0;
    float p = 0.0f, b0 = 0.0f;
    float *state = nullptr;              // [rows][2] = x_prev, y_prev: read, then left for the next call
    float *seg = nullptr;                // deemph_scratch_floats(): the segments' start and end y
    unsigned long long *missed = nullptr;   // += segments that were walked again
};
// serial: the one-lane-per-row kernel (also under option deemph_mode = 1); *segments += the segments the verify step checked
int deemph_launch(const DeemphArgs &a, const Options &o, bool serial, hipStream_t s, unsigned long long *segments);
// what a handle with de-emphasis owns: rows [rows][n] the producing stage writes (n = the call's samples per row), rows of y
// for callers that take PCM only (allocated by the first such call), the carried state, scratch, counters.  Nothing is allocated
// until it is first turned on.
struct Deemph {
    bool on = false, counted = false;
    float p = 0.0f, b0 = 0.0f;
    double tau_us = 0.0;                 // what is on (0 while off)
    size_t rows = 0, n_max = 0;
    DevBuf<float> in, out, state, seg;
    DevBuf<unsigned long long> counter;
    unsigned long long segments = 0;
    // (the handle's device is current)  tau_us 0 = off; the tau that is on: nothing happens; else waits for the device, state zeroed
    int set(double fs, double tau_us, size_t rows, size_t n_max, const Options &o);
    int reset(long first_row, long n_rows, hipStream_t s);   // asynchronous on s
    int run(size_t n, float *d_f32, int16_t *d_pcm, int ac, int wrap, const Options &o, bool serial, hipStream_t s);
    int diagnostics(unsigned long long *segments, unsigned long long *missed);
};

// ---- measurement aid (kernels_diag.hip): one pure streaming read of the buffer; method 0 registers (non-temporal), 1 LDS-DMA ring
int k_stream_read(const void *d_buf, size_t bytes, int method, unsigned *d_sink, hipStream_t s);

// ---- diagnostics (kernels_psd.hip) ---------------------------------------------------
// d_seg_db: (n/nfft)*(nfft/2) floats of scratch; d_freq, d_psd: nfft/2 floats
int k_estimate_psd(const float *d_x, size_t n, float Fs, int nfft, float *d_seg_db, float *d_freq, float *d_psd, hipStream_t s);

// ---- banks of receivers, every kind (bank.hip, kernels_bank.hip; struct Bank: bank_kernels.hpp) ----
struct Bank;
int bank_create(std::unique_ptr<Bank> &out, const fmrx_params &p, int n_channels, int audio_channels, int exact, size_t block_bytes,
                const Options &opt);
size_t bank_n_audio(const Bank *b);
void bank_input_layout(const Bank *b, uint8_t **d_first_block, size_t *pitch_bytes);
int bank_demod_layout(const Bank *b, const float **d_row0, size_t *pitch, size_t *n_if);   // FMRX_EINVAL: the bank keeps no rows
int bank_reset(Bank *b, int channel);
int bank_process_dev(Bank *b, float *d_audio, int16_t *d_pcm, int wrap, hipStream_t s);
int bank_read_tap(Bank *b, int channel, int which, float *out, size_t *n);

// ---- host-side coefficient design (coeff.cpp) --------------------------------
void design_lpf(float Fs, float Fc, int taps, float *h);
void design_bpf(float Fs, float Fb, float Fe, int taps, float *h);
// the reference's filters of one receiver: rf and audio low-pass; with `stereo`, the pilot and stereo band-pass
struct Filters {
    std::vector<float> rf, audio, pilot, stereo;
};
Filters design_filters(const fmrx_params &p, bool stereo);

// ---- wideband tuner (kernels_tuner.hip, kernels_tuner_rational.hip; handle and C ABI in tuner.hip) -----------------
// One call's launch at the rate U / D: the FIR + rotation kernel (matrix-core or generic) and the kernel that carries the
// history.  The integer tuner is U = 1, D <= 32 (tuner_integer_rate, tuner_host.hpp).
struct TunerLaunch {
    bool mfma = true;                    // the handle runs the matrix kernels (tuner_plan_info's `matrix` at create)
    int format = 0;                      // kTunerU8 / kTunerS8 / kTunerS16 (tuner_host.hpp): a value is 1, 1 or 2 raw bytes
    const uint8_t *x = nullptr;          // this call's wide samples, raw (matrix kernel: 16-byte aligned)
    long n_bytes = 0;                    // 2 * n_wide: the call's I and Q values (the raw bytes of the 8-bit formats); n_wide a multiple of D
    const uint8_t *hist = nullptr;       // `front` values in front of the call, raw, 16-byte aligned
    uint8_t *hist_next = nullptr;        // receives the history the next call starts from
    const int8_t *a_img = nullptr;       // matrix kernel: operand image [group][image q < 8 U][ksp][64 lanes][16]
    const int16_t *taps_re = nullptr, *taps_im = nullptr;   // generic kernel: [n_channels][U * Tp], phase-major
    const uint2 *chan = nullptr;         // per channel {frequency word, output shift s + 15 + B}
    const int2 *kconst = nullptr;        // 16-bit matrix kernel: [n_channels][U], per phase 128 * {sum(re - im), sum(im + re)}, what the
                                         //   low plane's offset of 128 adds to acc
    const unsigned *table = nullptr;     // rotation table, cos | sin << 16
    uint8_t *out = nullptr;
    long pitch = 0;
    int n_channels = 0, U = 1, D = 2, Tp = 0, front = 0, ks = 0, ksp = 0;
    unsigned n0 = 0;                     // wide-sample index of the call's first sample, mod 2^32
    unsigned long long *levels = nullptr;   // [n_channels][2] = {clipped, power}, zeroed by the caller
};
// what a call launches: kernel set, tiles per wave and step, output path, LDS and grid (tuner_plan_info, tuner_host.hpp)
struct TunerPlanInfo;
int tuner_launch(const TunerLaunch &a, hipStream_t stream);
// tuner_launch's matrix-kernel launch outside the integer rates (kernels_tuner_rational.hip)
int tuner_rat_mfma_launch(const TunerLaunch &a, long n_out, const TunerPlanInfo &plan, hipStream_t stream);

// ---- what the meters report in decibels (host only): offset + 10 log10(num / den) clamped to [-99, 99]; -99 where num is not
// positive (0 / 0 and NaN included), 99 where only den is not
inline double db(double num, double den, double offset = 0.0)
{
    if (!(num > 0.0)) return -99.0;
    if (!(den > 0.0)) return 99.0;
    const double v = offset + 10.0 * std::log10(num / den);
    return v < -99.0 ? -99.0 : (v > 99.0 ? 99.0 : v);
}

// ---- signal meters (kernels_meters.hip; handle, host arithmetic and C ABI in meters.hip) -----------------
constexpr int kMetersSegment = FMRX_METERS_SEGMENT, kMetersProbes = FMRX_METERS_PROBES;
constexpr int kMetersRfFields = 5;    // per channel: sum_i, sum_q, m2, m4, clipped (64-bit integers)
constexpr int kMetersMpxFields = 8;   // per channel: sum_x, sum_x2, max_abs, probe[5] (doubles)
// RF pass: rows iq + c * pitch of n_bytes (even) u8 I,Q bytes, any alignment -> acc[c][kMetersRfFields] += (zeroed by the caller)
int meters_rf_launch(const uint8_t *d_iq, size_t pitch, size_t n_bytes, int n_channels, unsigned long long *d_acc, hipStream_t s);
// MPX pass: rows x + c * pitch of n_if >= kMetersSegment floats -> out[c][kMetersMpxFields] (written, not added);
// d_table: re [5][1024] then im [5][1024]; at most max_blocks workgroups walk the channels
int meters_mpx_launch(const float *d_x, size_t pitch, size_t n_if, int n_channels, const double *d_table, double *d_out, int max_blocks,
                      hipStream_t s);
// what a meters handle's last call left on the device, for a stage behind it on the same stream (meter_stage.hpp's MpxStage): the MPX
// results [n_channels][kMetersMpxFields], and that call's n_if (0: no discriminator rows were given; ran false: no call yet)
struct MetersMpx {
    const double *d_mpx;
    size_t n_if;
    int n_channels, device;
    bool ran;
};
MetersMpx meters_mpx(const fmrx_meters *m);

// ---- stereo blend and soft mute (kernels_blend.hip; control step in blend_control.hpp; handle and C ABI in blend.hip) -----------------
namespace blend {
struct Control;
}
// one lane per channel: d_status[c] <- control_step on d_mpx[c]'s probes; segments from d_seg_each[c], or seg_all where that is NULL
int blend_control_launch(const blend::Control &c, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all,
                         fmrx_blend_status *d_status, int n_channels, hipStream_t s);
// d_in [n_channels][audio_channels][n_audio] -> d_out (the same shape; may be d_in or NULL) and d_pcm [n_channels][n_audio][audio_channels]
// (may be NULL), ramped between the end points in d_status; float rows 4-byte aligned, n_audio <= 2^26
int blend_apply_launch(const float *d_in, float *d_out, int16_t *d_pcm, const fmrx_blend_status *d_status, int n_channels, int audio_channels,
                       size_t n_audio, float inv_n, int wrap, hipStream_t s);

// ---- variable high-cut (kernels_highcut.hip; control step in highcut_control.hpp; handle and C ABI in highcut.hip) -----------------
namespace highcut {
struct Control;
}
constexpr int kHighcutSegment = 256, kHighcutWarmup = 256;   // built-in lane shape: samples per lane, warm-up samples in front
// one lane per channel: d_status[c] <- control_step on d_mpx[c]'s probes; segments from d_seg_each[c], or seg_all where that is NULL
int highcut_control_launch(const highcut::Control &c, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all,
                           fmrx_highcut_status *d_status, int n_channels, hipStream_t s);
long highcut_segments(size_t n, int L);   // segments of L samples in a row of n
struct HighcutArgs {
    const float *x = nullptr;            // [rows][n], row = channel * ac + audio channel
    float *y = nullptr;                  // [rows][n]; not x
    int16_t *pcm = nullptr;              // [rows / ac][n][ac], or NULL
    const fmrx_highcut_status *status = nullptr;   // [rows / ac]: the poles' end points
    int ac = 1, wrap = 1;
    size_t rows = 0, n = 0;
    float inv_n = 0.0f, p_max = 0.0f;
    int L = kHighcutSegment, W = kHighcutWarmup;
    float *state = nullptr;              // [rows]: y_prev, read and replaced
    float *seg = nullptr;                // 2 * rows * highcut_segments(n, L): the segments' start and end y (not for the serial walk)
    unsigned long long *missed = nullptr;   // += the segments walked again
};
// serial: the one-lane-per-row kernel; otherwise segments + verify, and *segments += the boundaries the verify step checked
int highcut_apply_launch(const HighcutArgs &a, bool serial, hipStream_t s, unsigned long long *segments);

// ---- audio meters (kernels_audio_meters.hip; one channel's walk in audio_meters_core.hpp; handle and C ABI in audio_meters.hip) -----------------
constexpr int kAudioMetersStateFields = 10;   // per channel: z[2][4], bin_acc[2] (doubles); bin_fill lies in an array of its own
constexpr int kAudioMetersSumFields = 9;      // per channel: peak[2], sum_x[2], sum_x2[2], sum_k2[2], sum_lr (doubles)
constexpr int kAudioMetersCountFields = 3;    // per channel: over[2], bins_done (32-bit)
struct AudioMetersArgs {
    const float *x = nullptr;            // [n_channels][ac][pitch]; only read
    size_t pitch = 0, n = 0;             // floats per row; samples of every row to walk
    int n_channels = 0, ac = 1;
    double coef[2][5] = {};              // fmrx_audio_meters_design
    unsigned bin_len = 0;
    size_t max_bins = 0;
    // field-major [field][n_channels], so that the lanes of a wave touch consecutive addresses
    double *state = nullptr;             // [kAudioMetersStateFields][n_channels], read and replaced
    unsigned *fill = nullptr;            // [n_channels]: bin_fill, read and replaced
    double *sums = nullptr;              // [kAudioMetersSumFields][n_channels], written
    unsigned *counts = nullptr;          // [kAudioMetersCountFields][n_channels], written
    double *bins = nullptr;              // [n_channels][2][max_bins], written
};
int audio_meters_launch(const AudioMetersArgs &a, hipStream_t s);
// what an audio meters handle's last call left on the device, for a stage behind it on the same stream (leveller.hip): the sums
// [kAudioMetersSumFields][n_channels] and that call's n (ran false: no call yet)
struct AudioMetersSums {
    const double *d_sums;
    size_t n;
    int n_channels, ac, device;
    bool ran;
};
AudioMetersSums audio_meters_sums(const fmrx_audio_meters *m);

// ---- loudness leveller and peak limiter (kernels_leveller.hip; control step in leveller_control.hpp; handle and C ABI in leveller.hip) -----------------
namespace leveller {
struct Control;
}
// one lane per channel: d_status[c] <- control_step on the channel's K-weighted sums d_k2a[c], d_k2b[c] (d_k2b is not read for
// mono) and its n from d_n_each[c], or n_all where that is NULL
int leveller_control_launch(const leveller::Control &c, int audio_channels, const double *d_k2a, const double *d_k2b,
                            const unsigned long long *d_n_each, unsigned long long n_all, fmrx_leveller_status *d_status, int n_channels,
                            hipStream_t s);
// words of one channel's limiter state: 2W - 2 code deficits (2^24 - code) and W - 1 values of u per row; all zero is fresh
inline size_t leveller_state_words(int audio_channels, int W) { return static_cast<size_t>(W - 1) * (2 + audio_channels); }
struct LevellerArgs {
    const float *x = nullptr;            // [n_channels][ac][n]
    float *y = nullptr;                  // the same shape, or NULL; no overlap with x
    int16_t *pcm = nullptr;              // [n_channels][n][ac], or NULL
    fmrx_leveller_status *status = nullptr;   // [n_channels]: gain0, gain1 read; min_code lowered, limited added to
    const uint32_t *state_in = nullptr;  // [n_channels][leveller_state_words]: read
    uint32_t *state_out = nullptr;       // another buffer of that shape: written whole
    int n_channels = 0, ac = 1, W = 64, wrap = 1;
    size_t n = 0;
    float inv_n = 0.0f, ceiling = 0.0f;
};
int leveller_apply_launch(const LevellerArgs &a, hipStream_t s);

// ---- true-peak meter (kernels_true_peak.hip; the interpolator in true_peak_core.hpp; handle and C ABI in true_peak.hip) -----------------
constexpr int kTruePeakStateFields = 22;   // per channel: the last 11 samples of row L, then of row R (floats)
constexpr int kTruePeakFields = 6;         // per channel: true_peak[2], peak[2] (the bits of floats >= +0), over[2] (32-bit)
struct TruePeakArgs {
    const float *x = nullptr;            // [n_channels][ac][pitch]; only read
    size_t pitch = 0, n = 0;             // floats per row; samples of every row to walk
    int n_channels = 0, ac = 1;
    float limit = 0.0f;
    // field-major [field][n_channels]
    const float *state_in = nullptr;     // [kTruePeakStateFields][n_channels]: read
    float *state_out = nullptr;          // another buffer of that shape: the rows' fields written whole
    unsigned *res = nullptr;             // [kTruePeakFields][n_channels]: cleared on the stream, then raised by the kernel's atomics
};
int true_peak_launch(const TruePeakArgs &a, hipStream_t s);

// ---- audio spectrum meter (kernels_audio_spectrum.hip; tables and frame arithmetic in audio_spectrum_core.hpp; handle and C ABI in
// audio_spectrum.hip) --------------------------------------------------------------------------------------------------------------
constexpr size_t kAudioSpectrumPairMax = 2048;   // a row of at most this many samples completes at most 8 frames: two rows share a tile
struct AudioSpectrumArgs {
    const float *x = nullptr;            // [n_channels][ac][pitch]; only read
    size_t pitch = 0, n = 0;             // floats per row; samples of every row to walk
    int n_channels = 0, ac = 1;
    int n_bands = 0;
    const int *edges = nullptr;          // device, [n_bands + 1]
    // the carried state, channel-major: fill [n_channels], carry [n_channels][ac][256] floats of which the first fill count
    const unsigned *fill_in = nullptr;
    const float *carry_in = nullptr;
    unsigned *fill_out = nullptr;        // another pair of buffers of those shapes
    float *carry_out = nullptr;
    unsigned *frames = nullptr;          // [n_channels]: the frames the call completed
    double *res = nullptr;               // field-major [ac * n_bands][n_channels]: field r * n_bands + b
    double *tiles = nullptr;             // rows longer than 2048 samples only: [audio_spectrum_tiles(n)][n_channels * ac][n_bands]
};
size_t audio_spectrum_tiles(size_t n);   // the tiles of 16 frames a row of n samples can complete, whatever its fill
int audio_spectrum_launch(const AudioSpectrumArgs &a, hipStream_t s);

// ---- audio feature frames (kernels_audio_features.hip; tables and frame arithmetic in audio_features_core.hpp; handle and C ABI in
// audio_features.hip) --------------------------------------------------------------------------------------------------------------
struct AudioFeaturesArgs {
    const float *x = nullptr;            // [n_channels][ac][pitch]; only read
    size_t pitch = 0, n = 0;             // floats per row; samples of every row to walk
    int n_channels = 0, ac = 1;
    int win = 0, hop = 0, n_bins = 0, n_mels = 0;
    size_t f_max = 0;                    // frames per channel in feat
    // device tables: w [win], c [win], mel_lo / mel_hi [n_mels], mel_w [n_mels][n_bins]
    const float *w = nullptr, *c = nullptr, *mel_w = nullptr;
    const int *mel_lo = nullptr, *mel_hi = nullptr;
    // the carried state, channel-major: fill [n_channels], carry [n_channels][win] floats of the mono mix of which the first fill count
    const unsigned *fill_in = nullptr;
    const float *carry_in = nullptr;
    unsigned *fill_out = nullptr;        // another pair of buffers of those shapes
    float *carry_out = nullptr;
    unsigned *frames = nullptr;          // [n_channels]: the frames the call completed
    float *feat = nullptr;               // [n_channels][f_max][n_mels]; frames the call did not complete read +0
};
size_t audio_features_tiles(size_t n_channels, size_t f_max);   // the workgroups of a call: 16 columns of the (channel, frame) list each
int audio_features_launch(const AudioFeaturesArgs &a, hipStream_t s);

// ---- audio rate converter (kernels_audio_resample.hip; taps, positions and chains in audio_resample_core.hpp; handle and C ABI in
// audio_resample.hip) ---------------------------------------------------------------------------------------------------------------
struct AudioResampleArgs {
    const float *x = nullptr;            // [n_channels][ac][pitch]; only read
    size_t pitch = 0, n = 0;             // floats per row; samples of every row to walk
    int n_channels = 0, ac = 1, rows = 1;    // rows: the rows a channel converts, 1 (the mono mix of ac) or ac
    unsigned up = 1, down = 1, taps = 8;
    const float *h = nullptr;            // device, [up][taps]
    // the carried state, channel-major: pos [n_channels], carry [n_channels][rows][taps - 1]
    const unsigned *pos_in = nullptr;
    const float *carry_in = nullptr;
    unsigned *pos_out = nullptr;         // another pair of buffers of those shapes
    float *carry_out = nullptr;
    size_t m_max = 0;                    // outputs per row in out_f32 / out_pcm
    unsigned tile_out = 0;               // outputs per workgroup, from audio_resample_tile_out
    float *out_f32 = nullptr;            // [n_channels][rows][m_max], or NULL; entries the call did not complete read +0
    int16_t *out_pcm = nullptr;          // the same shape, or NULL
    int wrap = 1;
    unsigned *counts = nullptr;          // [n_channels]: the outputs the call completed
};
unsigned audio_resample_tile_out(unsigned up, unsigned down, unsigned taps);   // the outputs of a workgroup's tile, 1 .. 1024
int audio_resample_launch(const AudioResampleArgs &a, hipStream_t s);

}  // namespace fmrx
