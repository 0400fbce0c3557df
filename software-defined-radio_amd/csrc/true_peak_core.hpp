// true_peak_core.hpp -- the interpolator of the true-peak meter (include/fmrx.h: fmrx_true_peak_*; DESIGN.md section 4.16;
// defined by tests/_true_peak_model.py): the float32 tap table, the evaluation of a run of consecutive groups and what a group
// adds to a row's readings.  The host function fmrx_true_peak_walk (true_peak.hip) and the kernel (kernels_true_peak.hip)
// compile this one body, so the two cannot drift apart.
//
// A group is the four values of the 4x oversampled waveform at k, k + 1/4, k + 2/4, k + 3/4: phase 0 is |x[k]| itself, phases
// 1 .. 3 are 12-tap fma chains over x[k-5 .. k+6], acc = +0, taps in ascending order, one rounding per step.  The chains of
// different groups and phases do not depend on each other, so two of them ride in the halves of one packed fma
// (v_pk_fma_f32 on the device) with every chain's own order and bits.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_TP_HD __host__ __device__ __forceinline__
#else
#define FMRX_TP_HD inline
#endif

namespace fmrx {
namespace true_peak {

constexpr int kTaps = 12;      // per phase, over x[k-5 .. k+6]
constexpr int kCarry = 11;     // samples of a row carried from call to call
constexpr int kLatency = 6;    // sample i of a call evaluates group i - 6
constexpr int kTile = 2048;    // samples of a row per workgroup
constexpr int kRun = 8;        // consecutive groups a lane evaluates from registers

// float32 of sinc(t) I0(5 sqrt(1 - (t/6)^2)) / I0(5), t = (j - 5) - p/4, made in float64 and rounded once: these literals are the
// definition.  Phase 3 is phase 1 reversed, phase 2 is symmetric: 18 distinct values.
#define FMRX_TP_H1                                                                                                                 \
    -0.00487442082f, 0.0147040663f, -0.0342647396f, 0.0723257735f, -0.163275108f, 0.896830738f, 0.289778441f, -0.105972648f,      \
        0.0499966145f, -0.022908682f, 0.00887645595f, -0.0022687749f
#define FMRX_TP_H2                                                                                                                 \
    -0.00483739981f, 0.0163076762f, -0.0397830643f, 0.0850367323f, -0.184198961f, 0.626807153f, 0.626807153f, -0.184198961f,      \
        0.0850367323f, -0.0397830643f, 0.0163076762f, -0.00483739981f
#define FMRX_TP_H3                                                                                                                 \
    -0.0022687749f, 0.00887645595f, -0.022908682f, 0.0499966145f, -0.105972648f, 0.289778441f, 0.896830738f, -0.163275108f,       \
        0.0723257735f, -0.0342647396f, 0.0147040663f, -0.00487442082f

// phase p = 1 .. 3, tap j; a function of constants, so that the device sees literals and no table in memory
FMRX_TP_HD constexpr float tap(int p, int j)
{
    constexpr float h1[kTaps] = {FMRX_TP_H1}, h2[kTaps] = {FMRX_TP_H2}, h3[kTaps] = {FMRX_TP_H3};
    return p == 1 ? h1[j] : (p == 2 ? h2[j] : h3[j]);
}

using f2 = float __attribute__((ext_vector_type(2)));

// what a row has read so far in a call (or in a lane's part of it)
struct Row {
    float tp = 0.0f, pk = 0.0f;   // maxima taken with v > m: a NaN never enters, an infinity does
    unsigned over = 0;
};

// one group's four values into the row's readings.  m = fmaxf(v, m) is m = v > m ? v : m here: every v is an absolute value and
// m starts at +0, so no -0 is about, and fmaxf returns m where v is a NaN
FMRX_TP_HD void note(Row &r, const float (&v)[4], float limit)
{
    r.pk = fmaxf(v[0], r.pk);
    r.tp = fmaxf(fmaxf(v[0], v[1]), fmaxf(fmaxf(v[2], v[3]), r.tp));
    const bool within = (v[0] <= limit) & (v[1] <= limit) & (v[2] <= limit) & (v[3] <= limit);   // false for a NaN: it counts
    r.over += within ? 0u : 1u;
}

// G (even) consecutive groups, of which the first `live` count: group g reads e[g .. g + 11], its sample is e[g + 5].  Two
// neighbouring groups go to the halves of a packed fma.
template <int G>
FMRX_TP_HD void run(const float (&e)[G + kCarry], int live, float limit, Row &r)
{
    static_assert(G % 2 == 0, "groups are evaluated in pairs");
    float v[G][4];
#pragma unroll
    for (int g = 0; g < G; g += 2) {
#pragma unroll
        for (int p = 1; p < 4; p++) {
            f2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < kTaps; j++) {
                const float h = tap(p, j);
                acc = __builtin_elementwise_fma(f2{h, h}, f2{e[g + j], e[g + 1 + j]}, acc);
            }
            v[g][p] = fabsf(acc[0]);
            v[g + 1][p] = fabsf(acc[1]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; g++) v[g][0] = fabsf(e[g + 5]);
    if (live >= G) {   // the usual run, straight through
#pragma unroll
        for (int g = 0; g < G; g++) note(r, v[g], limit);
    } else {
#pragma unroll
        for (int g = 0; g < G; g++)
            if (g < live) note(r, v[g], limit);
    }
}

}  // namespace true_peak
}  // namespace fmrx
