// audio_features_core.hpp -- the tables and the frame arithmetic of the audio feature frames (include/fmrx.h:
// fmrx_audio_features_*; defined by tests/_audio_features_model.py).  The host function
// fmrx_audio_features_walk (audio_features.hip) and the kernel (kernels_audio_features.hip) share the geometry's checks, the
// frame count, the table construction, the mono mix, the bin power and the mel chain; the 2 x n_bins chains of a frame are fmaf
// on the host and v_mfma_f32_16x16x4_f32 on the device, which is the same chain (tests/_fir_model.py from MFMA_K_ORDER on).
//
// A frame is win samples of the mono mix m.  xw[j] = m[j] w[j]; for bins k = 0 .. n_bins - 1, re_k = the fmaf chain over j
// ascending from +0 of C[(k j) mod win] xw[j], im_k the same with C[(k j - win/4) mod win]; p_k = fmaf(im_k, im_k, fl(re_k re_k));
// feature b is the fmaf chain over k = mel_lo[b] .. mel_hi[b] - 1 ascending from +0 of mel_w[b][k] p_k.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "fmrx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_AF_HD __host__ __device__ __forceinline__
#else
#define FMRX_AF_HD inline
#endif

namespace fmrx {
namespace audio_features {

constexpr int kMaxWin = 1280;    // samples of a frame, at most
constexpr int kMaxBins = 256;
constexpr int kMaxMels = 128;
constexpr int kTile = 16;        // frames that share a matrix instruction: its columns

// the geometry fmrx_audio_features_params may hold
inline bool good_params(const fmrx_audio_features_params *p)
{
    if (!p) return false;
    if (p->win < 16 || p->win > static_cast<uint32_t>(kMaxWin) || p->win % 4 != 0) return false;
    if (p->hop < 1 || p->hop > p->win) return false;
    if (p->n_bins < 1 || p->n_bins > static_cast<uint32_t>(kMaxBins) || p->n_bins > p->win / 2) return false;
    if (p->n_mels < 1 || p->n_mels > static_cast<uint32_t>(kMaxMels)) return false;
    if (!std::isfinite(p->f_lo) || !std::isfinite(p->f_hi) || !std::isfinite(p->audio_Fs)) return false;
    return 0.0 <= p->f_lo && p->f_lo < p->f_hi && p->f_hi <= p->audio_Fs / 2.0;
}

// the frames a stream of T = fill + n samples completes
FMRX_AF_HD unsigned frames_of(unsigned T, unsigned win, unsigned hop) { return T < win ? 0u : (T - win) / hop + 1u; }

// the most frames a call of n_audio samples completes, whatever the fill (< win)
inline size_t max_frames(size_t n_audio, unsigned hop) { return (n_audio - 1) / hop + 1; }

// the mono mix of a stereo channel: one float32 add, then an exact halving
FMRX_AF_HD float mono_mix(float l, float r) { return 0.5f * (l + r); }

// p_k of one bin: the product re re is rounded on its own
FMRX_AF_HD float bin_power(float re, float im)
{
    const float rr = re * re;
    return fmaf(im, im, rr);
}

// one feature of one frame: w[k] p[k] chained over k = lo .. hi - 1 ascending from +0
FMRX_AF_HD float mel_chain(const float *w, const float *p, int lo, int hi)
{
    float acc = 0.0f;
    for (int k = lo; k < hi; k++) acc = fmaf(w[k], p[k], acc);
    return acc;
}

// the Slaney mel scale: linear at 200/3 Hz per mel below 1 kHz, logarithmic with step ln(6.4)/27 above
inline double hz_to_mel(double f) { return f < 1000.0 ? f / (200.0 / 3.0) : 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0); }
inline double mel_to_hz(double m) { return m < 15.0 ? m * (200.0 / 3.0) : 1000.0 * std::exp((m - 15.0) * (std::log(6.4) / 27.0)); }

// float32 tables, made in double and rounded once: w[win], c[win], mel_w[n_mels][n_bins], lo / hi [n_mels]
struct Tables {
    std::vector<float> w, c, mel_w;
    std::vector<int32_t> lo, hi;
};

inline Tables make_tables(const fmrx_audio_features_params &p)
{
    const int win = static_cast<int>(p.win), n_bins = static_cast<int>(p.n_bins), n_mels = static_cast<int>(p.n_mels);
    const double two_pi = 6.283185307179586476925286766559;
    Tables t;
    t.w.assign(win, 0.0f);
    t.c.assign(win, 0.0f);
    t.mel_w.assign(static_cast<size_t>(n_mels) * n_bins, 0.0f);
    t.lo.assign(n_mels, 0);
    t.hi.assign(n_mels, 0);
    // the cosine's first quarter, unfolded: C[win/2 - m] = -C[m], C[win - m] = C[m], C[win/4] = C[3 win/4] = +0
    const int q = win / 4, h = win / 2;
    for (int m = 0; m <= q; m++) {
        const float v = m == q ? 0.0f : static_cast<float>(std::cos(two_pi * m / win));
        t.c[m] = v;
        t.c[h - m] = -v;
    }
    t.c[q] = 0.0f;
    for (int m = 1; m < h; m++) t.c[win - m] = t.c[m];
    // the periodic Hann window's first half and its middle, unfolded: w[win - j] = w[j]
    for (int j = 0; j <= h; j++) t.w[j] = static_cast<float>(0.5 - 0.5 * std::cos(two_pi * j / win));
    t.w[0] = 0.0f;
    for (int j = 1; j < h; j++) t.w[win - j] = t.w[j];
    // the filters: n_mels + 2 points equally spaced in mel, triangles between them times the Slaney norm
    const double m_lo = hz_to_mel(p.f_lo), m_hi = hz_to_mel(p.f_hi);
    std::vector<double> f(n_mels + 2);
    for (int i = 0; i < n_mels + 2; i++) f[i] = mel_to_hz(m_lo + (m_hi - m_lo) * i / (n_mels + 1));
    for (int b = 0; b < n_mels; b++) {
        const double norm = 2.0 / (f[b + 2] - f[b]);
        int first = -1, last = -1;
        for (int k = 0; k < n_bins; k++) {
            const double fk = k * p.audio_Fs / win;
            const double lower = (fk - f[b]) / (f[b + 1] - f[b]), upper = (f[b + 2] - fk) / (f[b + 2] - f[b + 1]);
            const double tri = lower < upper ? lower : upper;
            const float v = tri > 0.0 ? static_cast<float>(tri * norm) : 0.0f;
            t.mel_w[static_cast<size_t>(b) * n_bins + k] = v;
            if (v > 0.0f) {
                if (first < 0) first = k;
                last = k;
            }
        }
        if (first >= 0) {
            t.lo[b] = first;
            t.hi[b] = last + 1;
        }
    }
    return t;
}

}  // namespace audio_features
}  // namespace fmrx
