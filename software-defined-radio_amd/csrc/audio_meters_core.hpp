// audio_meters_core.hpp -- the walk of one channel of the audio meters (include/fmrx.h: fmrx_audio_meters_*; DESIGN.md section
// 4.14; defined by tests/_audio_meters_model.py): the K-weighting design, the step of one sample and the 100 ms bins.  The host
// function fmrx_audio_meters_walk (audio_meters.hip) and the kernel (kernels_audio_meters.hip) compile this one body, so the
// two cannot drift apart.  Every step is one IEEE double operation in the model's order; the Makefile's -ffp-contract=off keeps
// the compiler from fusing any of them, on the host and on the device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_AM_HD __host__ __device__ __forceinline__
#else
#define FMRX_AM_HD inline
#endif

namespace fmrx {
namespace audio_meters {

constexpr double kVh = 1.5848647011308556;   // 10^(3.999843853973347 / 20)
constexpr double kVb = 1.2587209302325617;   // kVh^0.4996667741545416
constexpr double kShelfF0 = 1681.974450955533, kShelfQ = 0.7071752369554196;
constexpr double kHpF0 = 38.13547087602444, kHpQ = 0.5003270373238773;
constexpr double kPi = 3.141592653589793;
constexpr double kMinFs = 8000.0, kMaxFs = 768000.0;   // what fmrx_audio_meters_design accepts

// (b0, b1, b2, a1, a2) of the shelf, then of the high-pass
struct Coefs {
    double q[2][5];
};

// host only: tan() is the C library's
inline void design(double Fs, Coefs *c)
{
    double K = std::tan(kPi * kShelfF0 / Fs);
    double KQ = K / kShelfQ, K2 = K * K;
    double a0 = (1.0 + KQ) + K2;
    c->q[0][0] = ((kVh + kVb * KQ) + K2) / a0;
    c->q[0][1] = (2.0 * (K2 - kVh)) / a0;
    c->q[0][2] = ((kVh - kVb * KQ) + K2) / a0;
    c->q[0][3] = (2.0 * (K2 - 1.0)) / a0;
    c->q[0][4] = ((1.0 - KQ) + K2) / a0;
    K = std::tan(kPi * kHpF0 / Fs);
    KQ = K / kHpQ;
    K2 = K * K;
    a0 = (1.0 + KQ) + K2;
    c->q[1][0] = 1.0;
    c->q[1][1] = -2.0;
    c->q[1][2] = 1.0;
    c->q[1][3] = (2.0 * (K2 - 1.0)) / a0;
    c->q[1][4] = ((1.0 - KQ) + K2) / a0;
}

inline size_t bin_len(double Fs) { return static_cast<size_t>(Fs / 10.0 + 0.5); }

// One channel during a call: the carried state (z, bin_acc, bin_fill) and the call's sums.  AC = 1: index 0 only.
template <int AC>
struct Walk {
    double z[AC][4], bin_acc[AC];
    double sum_x[AC], sum_x2[AC], sum_k2[AC], sum_lr;
    float peak[AC];
    unsigned over[AC], bin_fill, bins_done;

    FMRX_AM_HD void begin()
    {
#pragma unroll
        for (int r = 0; r < AC; r++) {
            sum_x[r] = sum_x2[r] = sum_k2[r] = 0.0;
            peak[r] = 0.0f;
            over[r] = 0;
        }
        sum_lr = 0.0;
        bins_done = 0;
    }

    // one biquad, transposed direct form II
    static FMRX_AM_HD double biquad(const double *q, double v, double *z)
    {
        const double o = q[0] * v + z[0];
        z[0] = (q[1] * v - q[3] * o) + z[1];
        z[1] = q[2] * v - q[4] * o;
        return o;
    }

    // the same with b0 = b2 = 1, the high-pass: those two products are exact (1 v = v, -0 and NaN included), so they are not formed
    static FMRX_AM_HD double biquad_unit(const double *q, double v, double *z)
    {
        const double o = v + z[0];
        z[0] = (q[1] * v - q[3] * o) + z[1];
        z[1] = v - q[4] * o;
        return o;
    }

    FMRX_AM_HD void row(const Coefs &c, int r, float x)
    {
        const float a = __builtin_fabsf(x);
        over[r] += !(a < 2.0f);
        peak[r] = a > peak[r] ? a : peak[r];
        const double v = static_cast<double>(x);
        sum_x[r] = sum_x[r] + v;
        sum_x2[r] = sum_x2[r] + v * v;
        const double y = biquad_unit(c.q[1], biquad(c.q[0], v, z[r]), z[r] + 2);
        const double y2 = y * y;
        sum_k2[r] = sum_k2[r] + y2;
        bin_acc[r] = bin_acc[r] + y2;
    }

    // one sample of every row into the sums and bin_acc, without the bin's bookkeeping: for a caller that knows that no bin
    // closes within the samples it walks (bin_fill + their count < bin_len) and advances bin_fill itself
    FMRX_AM_HD void accumulate(const Coefs &c, const float *x)
    {
#pragma unroll
        for (int r = 0; r < AC; r++) row(c, r, x[r]);
        if (AC == 2) sum_lr = sum_lr + static_cast<double>(x[0]) * static_cast<double>(x[AC - 1]);
    }

    // x[r]: the sample of row r; bins: this channel's [2][max_bins].  The caller guarantees room: a call of n samples closes at
    // most n / len + 1 bins.
    FMRX_AM_HD void sample(const Coefs &c, const float *x, unsigned len, double *bins, size_t max_bins)
    {
        accumulate(c, x);
        if (++bin_fill == len) {
#pragma unroll
            for (int r = 0; r < AC; r++) {
                if (bins_done < max_bins) bins[r * max_bins + bins_done] = bin_acc[r];
                bin_acc[r] = 0.0;
            }
            bin_fill = 0;
            bins_done++;
        }
    }

    // entries past bins_done (and a mono channel's second row) read 0
    FMRX_AM_HD void finish(double *bins, size_t max_bins) const
    {
        for (int r = 0; r < 2; r++)
            for (size_t b = r < AC ? bins_done : 0; b < max_bins; b++) bins[r * max_bins + b] = 0.0;
    }
};

}  // namespace audio_meters
}  // namespace fmrx
