// kernels_deemph.hip -- the 50 / 75 us de-emphasis filter (no counterpart in the reference, which has no such stage).
//
// The definition (tests/_deemph_model.py).  Per row, state (x_prev, y_prev), both +0 at the start of a stream:
//     u = x[n] + x_prev;  v = b0 * u;  y = fmaf(p, y_prev, v);  if |y| < 2^-126: y = +0
// with p, b0 from fmrx_deemph_design.  The flush is part of the definition: without it the state of a row in digital silence
// sticks at the smallest subnormal (RN(p * 2^-149) = 2^-149) and a lane that starts from zero never meets it again.
// v = b0 * (x + x_prev) does not depend on y: only the fused multiply-add and the flush are on the dependent chain.
//
// One kernel family on rows [rows][n] with a row pitch -- a pipeline has 1 or 2 rows, a bank n_channels * audio_channels --,
// the three bodies of onepole_walk.hpp (which describes the scheme, the staging and the repair) with DeemphFilter:
//   deemph_segments_kernel  parallel in time, one lane per (row, segment)
//   deemph_verify_kernel    one workgroup per row checks the segments' joints and walks a miss again
//   deemph_serial_kernel    one lane per row walks the whole row (option deemph_mode = 1, set_force_generic; what the segment
//                           kernels are measured against).
// The stage is out of place: the repair reads x again.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): segments 57 VGPRs, 8 448 bytes of LDS; verify 15 VGPRs, 8 bytes; serial
// 28 VGPRs, none; no kernel uses scratch.
#include "onepole_walk.hpp"

namespace fmrx {
namespace {

using walk::kLanes;

// state [rows][2] = x_prev, y_prev; the same p, b0 for every row
struct DeemphFilter {
    float p, b0;
    struct State {
        float x_prev, y;
    };
    __device__ __forceinline__ State load(const float *state, long row) const { return State{state[2 * row], state[2 * row + 1]}; }
    __device__ __forceinline__ void store(float *state, long row, State s) const
    {
        state[2 * row] = s.x_prev;
        state[2 * row + 1] = s.y;
    }
    __device__ __forceinline__ DeemphFilter at(long) const { return *this; }
    __device__ __forceinline__ State enter(float y, const float *x) const { return State{x[-1], y}; }
    __device__ __forceinline__ State step(float x, int, State s) const
    {
        const float v = b0 * (x + s.x_prev);
        const float y = __builtin_fmaf(p, s.y, v);
        return State{x, __builtin_fabsf(y) < 1.17549435e-38f ? 0.0f : y};
    }
};

__global__ __launch_bounds__(kLanes) void deemph_segments_kernel(const float *__restrict__ x, long pitch_x, float *__restrict__ y,
                                                                 long pitch_y, int16_t *__restrict__ pcm, int ac, int wrap, long rows,
                                                                 int n, int nseg, int L, int W, float p, float b0,
                                                                 const float *__restrict__ state, float *__restrict__ seg)
{
    walk::walk_segments(DeemphFilter{p, b0}, x, pitch_x, y, pitch_y, pcm, ac, wrap, rows, n, nseg, L, W, state, seg);
}

__global__ __launch_bounds__(walk::kVerifyMax) void deemph_verify_kernel(const float *__restrict__ x, long pitch_x, float *y, long pitch_y,
                                                                     int16_t *pcm, int ac, int wrap, long rows, int n, int nseg, int L,
                                                                     float p, float b0, float *__restrict__ state, float *seg,
                                                                     unsigned long long *missed)
{
    walk::walk_verify(DeemphFilter{p, b0}, x, pitch_x, y, pitch_y, pcm, ac, wrap, rows, n, nseg, L, state, seg, missed);
}

__global__ __launch_bounds__(kLanes) void deemph_serial_kernel(const float *__restrict__ x, long pitch_x, float *__restrict__ y,
                                                               long pitch_y, int16_t *__restrict__ pcm, int ac, int wrap, long rows,
                                                               int n, float p, float b0, float *__restrict__ state)
{
    walk::walk_serial(DeemphFilter{p, b0}, x, pitch_x, y, pitch_y, pcm, ac, wrap, rows, n, state);
}

}  // namespace

DeemphShape deemph_shape(const Options &o, size_t n)
{
    DeemphShape s;
    s.L = o.deemph_segment < 0 ? kDeemphSegment : o.deemph_segment;
    s.W = o.deemph_warmup < 0 ? kDeemphWarmup : o.deemph_warmup;
    s.nseg = walk::segments(n, s.L);
    return s;
}

size_t deemph_scratch_floats(size_t rows, size_t n, const Options &o) { return 2 * rows * static_cast<size_t>(deemph_shape(o, n).nseg) + 2; }

int deemph_launch(const DeemphArgs &a, const Options &o, bool serial, hipStream_t s, unsigned long long *segments)
{
    if (a.rows == 0 || a.n == 0) return FMRX_OK;
    if (!a.x || !a.y || !a.state) return fail(FMRX_EINVAL, "deemph: null buffer");
    if (a.x == a.y) return fail(FMRX_EINVAL, "deemph: the stage is out of place (the repair reads x again)");
    if (a.n > (static_cast<size_t>(1) << 30) || a.rows > (static_cast<size_t>(1) << 30))
        return fail(FMRX_EINVAL, "deemph: at most 2^30 samples per row and 2^30 rows");
    if (a.pitch_x < static_cast<long>(a.n) || a.pitch_y < static_cast<long>(a.n)) return fail(FMRX_EINVAL, "deemph: pitch smaller than n");
    if (a.ac < 1 || a.rows % a.ac) return fail(FMRX_EINVAL, "deemph: rows %zu are not whole groups of %d PCM channels", a.rows, a.ac);
    const long rows = static_cast<long>(a.rows);
    const int n = static_cast<int>(a.n);
    if (serial || o.deemph_mode == 1) {
        hipLaunchKernelGGL(deemph_serial_kernel, dim3(walk::serial_blocks(rows)), dim3(kLanes), 0, s, a.x, a.pitch_x, a.y, a.pitch_y, a.pcm, a.ac,
                           a.wrap, rows, n, a.p, a.b0, a.state);
        FMRX_LAUNCH_CHECK("deemph_serial_kernel");
        return FMRX_OK;
    }
    const DeemphShape sh = deemph_shape(o, a.n);
    if (!a.seg || !a.missed) return fail(FMRX_EINVAL, "deemph: null scratch");
    walk::Grid g;
    FMRX_TRY(walk::grid("deemph", rows, a.n, sh.L, &g));
    hipLaunchKernelGGL(deemph_segments_kernel, dim3(g.blocks), dim3(kLanes), 0, s, a.x, a.pitch_x, a.y, a.pitch_y, a.pcm, a.ac, a.wrap, rows, n,
                       static_cast<int>(g.nseg), sh.L, sh.W, a.p, a.b0, a.state, a.seg);
    FMRX_LAUNCH_CHECK("deemph_segments_kernel");
    hipLaunchKernelGGL(deemph_verify_kernel, dim3(static_cast<unsigned>(rows)), dim3(g.verify_lanes), 0, s, a.x, a.pitch_x, a.y, a.pitch_y, a.pcm,
                       a.ac, a.wrap, rows, n, static_cast<int>(g.nseg), sh.L, a.p, a.b0, a.state, a.seg, a.missed);
    FMRX_LAUNCH_CHECK("deemph_verify_kernel");
    if (segments) *segments += g.checked;
    return FMRX_OK;
}

// ---- a handle's de-emphasis: coefficients, carried state, scratch, counters ----
int Deemph::set(double fs, double tau_us_, size_t rows_, size_t n_max_, const Options &o)
{
    if (!(tau_us_ >= 0.0)) return fail(FMRX_EINVAL, "set_deemphasis: tau must be positive, or 0 for off");
    if (on && tau_us_ == tau_us) return FMRX_OK;
    FMRX_HIP(hipDeviceSynchronize());   // nothing in flight sees the change under it
    if (tau_us_ == 0.0) {
        on = false;
        tau_us = 0.0;
        return FMRX_OK;
    }
    float p_, b0_;
    FMRX_TRY(fmrx_deemph_design(fs, tau_us_, &p_, &b0_));
    rows = rows_;
    n_max = n_max_;
    FMRX_TRY(in.ensure(rows * n_max));
    FMRX_TRY(state.ensure(2 * rows));
    FMRX_TRY(seg.ensure(deemph_scratch_floats(rows, n_max, o)));
    FMRX_TRY(counter.ensure(1));
    if (!counted) FMRX_HIP(hipMemset(counter.p, 0, sizeof(unsigned long long)));
    counted = true;
    FMRX_HIP(hipMemset(state.p, 0, 2 * rows * sizeof(float)));
    FMRX_HIP(hipDeviceSynchronize());
    p = p_;
    b0 = b0_;
    tau_us = tau_us_;
    on = true;
    return FMRX_OK;
}

int Deemph::reset(long first_row, long n_rows, hipStream_t s)
{
    if (!state.p) return FMRX_OK;
    FMRX_HIP(hipMemsetAsync(state.p + 2 * first_row, 0, 2 * n_rows * sizeof(float), s));
    return FMRX_OK;
}

int Deemph::run(size_t n, float *d_f32, int16_t *d_pcm, int ac, int wrap, const Options &o, bool serial, hipStream_t s)
{
    if (n > n_max) return fail(FMRX_EINVAL, "deemph: %zu samples per row exceed the %zu the handle was sized for", n, n_max);
    FMRX_TRY(seg.ensure(deemph_scratch_floats(rows, n, o)));   // (grows only when the options' shape changes: a wait, not per call)
    if (!d_f32) FMRX_TRY(out.ensure(rows * n_max));            // (the first call that takes PCM only)
    DeemphArgs a;
    a.x = in.p;
    a.pitch_x = a.pitch_y = static_cast<long>(n);
    a.y = d_f32 ? d_f32 : out.p;
    a.pcm = d_pcm;
    a.ac = ac;
    a.wrap = wrap;
    a.rows = rows;
    a.n = n;
    a.p = p;
    a.b0 = b0;
    a.state = state.p;
    a.seg = seg.p;
    a.missed = counter.p;
    return deemph_launch(a, o, serial, s, &segments);
}

int Deemph::diagnostics(unsigned long long *segments_, unsigned long long *missed_)
{
    FMRX_HIP(hipDeviceSynchronize());
    if (segments_) *segments_ = segments;
    if (missed_) {
        *missed_ = 0;
        if (counter.p) FMRX_HIP(hipMemcpy(missed_, counter.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return FMRX_OK;
}

}  // namespace fmrx
