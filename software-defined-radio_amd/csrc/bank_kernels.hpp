// bank_kernels.hpp -- what bank.hip (the receiver bank's host side) and kernels_bank.hip (its kernels, table builders and
// launchers) share: the handle, and the launch functions its shapes resolve to.
#pragma once
#include "fmrx_internal.hpp"

namespace fmrx {

struct Bank;

constexpr int kR = 8;   // consecutive outputs per thread of the exact FIR kernels (= table entries per step)

// fmPLL(carrier_filt, 19 kHz, if_Fs, ncoScale 2, phaseAdjust 0, normBandwidth 0.01): src/project.cpp:237
constexpr float kPilotHz = 19e3f, kNcoScale = 2.0f, kPhaseAdjust = 0.0f, kPllBandwidth = 0.01f;

// The kernels of one bank: its shapes, exact / fast and mono / stereo resolved to template instances once, when the bank is
// created.  A table builder fills the bank's device table of that stage; a launcher covers a range of every channel's block.
struct BankKernels {
    // the fast mono bank of modes 0/1: the slots of all channels, back to back, are ONE pseudo-stream through the fused mono kernel
    // (kernels_fe_mfma.hip: mono_fused_launch), which keeps nothing but the audio in memory: no rows, and none of the stages below
    bool fused = false;
    size_t hist_bytes = 0;   // bytes of history the exact front end reads in front of a block
    int (*fe_table)(Bank &b, const float *h) = nullptr;
    int (*fe)(const Bank &b, long k_lo, long k_hi, hipStream_t s) = nullptr;                      // IF outputs [k_lo, k_hi)
    int (*bpf_table)(Bank &b, const float *h_st, const float *h_car) = nullptr;                   // stereo banks only
    int (*bpf)(const Bank &b, long k_lo, long k_hi, hipStream_t s) = nullptr;
    int (*out_table)(Bank &b, const float *h) = nullptr;
    // audio outputs [a_lo, a_hi), from the IF samples [.., g_hi)
    int (*out)(Bank &b, float *d_audio, int16_t *d_pcm, int wrap, long a_lo, long a_hi, long g_hi, hipStream_t s) = nullptr;
};
// false: no kernels for these shapes (k is then left partly filled)
bool bank_resolve(const fmrx_params &p, int audio_channels, int exact, BankKernels &k);

// chs_nco_kernel over [k_lo, k_hi) of n_rows rows of raw trigArg, in place; mixer != nullptr: the mixer rows too
int bank_launch_nco(bool exact, float *trig, long ypitch, int n_rows, long k_lo, long k_hi, const float *bpf, const float *nco0,
                    float *mixer, long mpitch, int hm, hipStream_t s);
// carried state: every slot's and row's tail -> its history; the fused kind: and its audio / PCM -> the caller's arrays
int bank_launch_finish(const Bank &b, float *d_audio, int16_t *d_pcm, hipStream_t s);
int bank_launch_fill_state(float *pll, long n, hipStream_t s);      // state_PLL of n / 8 channels at the start of a stream

struct Bank {
    fmrx_params p{};
    int n_channels = 0, audio_channels = 2, exact = 1;
    size_t hist_bytes = 0, slot_bytes = 0;
    long n_if = 0, n_audio = 0;
    int Ha = 0, delay = 0, Hd = 0, Hm = 0;
    long dpitch = 0, ypitch = 0, cpitch = 0, mpitch = 0;   // floats between rows: demod; bpf, carrier, trig; (bytes) carrier8; mixer
    BankKernels k;
    DevBuf<uint8_t> slots;
    DevBuf<float> fe_table, bpf_table, out_table;
    FePlan fe;                      // fast banks: the matrix-core front end's tap image
    // the fused kind: the audio taps' image, the options its launch takes, the audio samples per slot that the history region yields
    // (computed and discarded), zeros for the discriminator history of the pseudo-stream, and the audio / PCM of whole slots
    AudioPlan audio;
    Options opt;
    size_t junk_audio = 0;
    DevBuf<float> zeros, audio_all;
    DevBuf<int16_t> pcm_all;
    DevBuf<float> demod, carrier, bpf, trig, pll, nco0, mixtail[2];
    DevBuf<int8_t> carrier8;        // fast banks: the sign of the pilot band-pass output, one byte per IF sample
    // resampling modes (2, 3): the plain audio taps and, stereo, the mixer rows [Hm | n_if]
    bool resample = false;
    DevBuf<float> h_res, mixer;
    // ... and, when U is a multiple of 7 (both of the reference's), the step-major tap table of chs_resample_lanes_kernel
    DevBuf<float> res_table;
    DevBuf<int> res_top;
    int res_groups = 0, res_iters = 0, res_hist = 0;   // res_hist: samples of history its windows reach (>= Ha, by the rounding to whole iterations)
    int mix_cur = 0;
    // A stereo call walks the block in chunks on two internal streams: `wide` carries the front end, the band-pass pair and the
    // output stage of every chunk, `lanes` the PLL -- the PLL's few waves (one per 64 channels, a dependent chain each) leave
    // the chip almost idle, and chunk c+1's wide kernels fill it meanwhile.  Events: chunk c's band-pass output is ready
    // (wide -> lanes), its PLL is through (lanes -> wide); fork / join with the caller's stream around the call.
    static constexpr int kMaxChunks = 8;
    // the chunk plan, fixed at create (bank.hip: plan_chunks)
    long per = 0, fe_tile = 0;
    int K = 1, lag = 1;
    bool split = false;             // the front end on a stream of its own
    bool nco_pass = false;          // the NCO output is finished by a pass of its own (else: inside the output stage)
    hipStream_t wide = nullptr, lanes = nullptr;
    hipStream_t front = nullptr;    // fast banks: the HBM-bound front end runs on its own stream, next to the vector-ALU-bound kernels
    hipEvent_t ev_bpf[kMaxChunks] = {}, ev_pll[kMaxChunks] = {}, ev_fe[kMaxChunks] = {}, ev_fork = nullptr, ev_join = nullptr;
    ~Bank();
};

}  // namespace fmrx
