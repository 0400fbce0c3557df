// kernels_highcut.hip -- the kernels of the variable high-cut stage (include/fmrx.h: fmrx_highcut_*; DESIGN.md section 4.13;
// defined by tests/_highcut_model.py).
//
// The definition.  Per row, state y_prev, +0 at the start of a stream; sample k of the call's n:
//     p[k] = clamp(fmaf((float)(k + 1), (p1 - p0) * inv_n, p0), 0, p_max);  q = 1 - p[k];  v = q * x[k]
//     y = fmaf(p[k], y_prev, v);  if |y| < 2^-126: y = +0;  y[k] = p[k] == 0 ? x[k] : y
// with (p0, p1) from the status row of the row's channel.  The flush is there for the reason kernels_deemph.hip gives; the
// select makes a channel at cut 0 return its input's bits.
//
//   highcut_control_kernel   meter_stage.hpp's control kernel with control_step of highcut_control.hpp.
//   highcut_segments_kernel, highcut_verify_kernel, highcut_serial_kernel
//                            the three bodies of onepole_walk.hpp (which describes the scheme, the staging and the repair) with
//                            HighcutFilter: a pole that moves inside the call.  Every lane computes p[k] from k itself, so a
//                            lane's pole is the serial walk's at every sample; p[k] <= p_max < 1 keeps the recurrence a
//                            contraction.  p[k], q and v do not depend on y: only the fused multiply-add, the flush and the
//                            select are on the dependent chain.  The serial kernel is the yardstick, and
//                            fmrx_highcut_set_force's path.
// Rows are f32 [rows][n] and PCM [row / ac][k][row % ac].  The walk is out of place: highcut.hip gives it a copy where the
// caller's d_out is d_in.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4.13; no kernel uses scratch.
#include "highcut_control.hpp"
#include "meter_stage.hpp"
#include "onepole_walk.hpp"

namespace fmrx {
namespace {

using walk::kLanes;

__global__ __launch_bounds__(meter_stage::kControlThreads) void highcut_control_kernel(highcut::Control c, const double *__restrict__ mpx,
                                                                                       const unsigned long long *__restrict__ seg_each,
                                                                                       unsigned long long seg_all,
                                                                                       fmrx_highcut_status *__restrict__ st, unsigned n_channels)
{
    meter_stage::control_body(c, mpx, seg_each, seg_all, st, n_channels);
}

// a row's pole ramp: p[k] = clamp(fmaf(k + 1, step, p0), 0, p_max)
struct Pole {
    float p0, ramp, p_max;
    struct State {
        float y;
    };
    __device__ __forceinline__ State enter(float y, const float *) const { return State{y}; }
    __device__ __forceinline__ State step(float x, int k, State s) const
    {
        const float r = fmaf(static_cast<float>(k + 1), ramp, p0);
        const float p = r < 0.0f ? 0.0f : (r > p_max ? p_max : r);
        const float q = 1.0f - p;
        const float v = q * x;
        const float y = __builtin_fmaf(p, s.y, v);
        const float f = __builtin_fabsf(y) < 1.17549435e-38f ? 0.0f : y;
        return State{p == 0.0f ? x : f};
    }
};

// state [rows] = y_prev; the pole's end points from the status row of the row's channel
struct HighcutFilter {
    const fmrx_highcut_status *__restrict__ st;
    int ac;
    float inv_n, p_max;
    using State = Pole::State;
    __device__ __forceinline__ State load(const float *state, long row) const { return State{state[row]}; }
    __device__ __forceinline__ void store(float *state, long row, State s) const { state[row] = s.y; }
    __device__ __forceinline__ Pole at(long row) const
    {
        const fmrx_highcut_status *s = st + row / ac;
        const float p0 = s->p0, p1 = s->p1;
        return Pole{p0, (p1 - p0) * inv_n, p_max};
    }
};

__global__ __launch_bounds__(kLanes) void highcut_segments_kernel(const float *__restrict__ x, float *__restrict__ y, int16_t *__restrict__ pcm,
                                                                  int ac, int wrap, long rows, int n, int nseg, int L, int W,
                                                                  const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                  const float *__restrict__ state, float *__restrict__ seg)
{
    walk::walk_segments(HighcutFilter{st, ac, inv_n, p_max}, x, n, y, n, pcm, ac, wrap, rows, n, nseg, L, W, state, seg);
}

__global__ __launch_bounds__(walk::kVerifyMax) void highcut_verify_kernel(const float *__restrict__ x, float *y, int16_t *pcm, int ac, int wrap,
                                                                         long rows, int n, int nseg, int L,
                                                                         const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                         float *__restrict__ state, float *seg, unsigned long long *missed)
{
    walk::walk_verify(HighcutFilter{st, ac, inv_n, p_max}, x, n, y, n, pcm, ac, wrap, rows, n, nseg, L, state, seg, missed);
}

__global__ __launch_bounds__(kLanes) void highcut_serial_kernel(const float *__restrict__ x, float *__restrict__ y, int16_t *__restrict__ pcm,
                                                                int ac, int wrap, long rows, int n,
                                                                const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                float *__restrict__ state)
{
    walk::walk_serial(HighcutFilter{st, ac, inv_n, p_max}, x, n, y, n, pcm, ac, wrap, rows, n, state);
}

}  // namespace

int highcut_control_launch(const highcut::Control &c, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all,
                           fmrx_highcut_status *d_status, int n_channels, hipStream_t s)
{
    return meter_stage::control_launch("highcut_control_kernel", highcut_control_kernel, n_channels, s, c, d_mpx, d_seg_each, seg_all, d_status);
}

long highcut_segments(size_t n, int L) { return walk::segments(n, L); }

int highcut_apply_launch(const HighcutArgs &a, bool serial, hipStream_t s, unsigned long long *segments)
{
    if (!a.x || !a.y || !a.status || !a.state) return fail(FMRX_EINVAL, "highcut: null buffer");
    if (a.x == a.y) return fail(FMRX_EINVAL, "highcut: the walk is out of place (warm-up and repair read x again)");
    if (a.rows < 1 || a.n < 1 || a.n > (size_t{1} << 26) || a.rows > (size_t{1} << 30)) return fail(FMRX_EINVAL, "highcut: 1 .. 2^26 samples per row, 1 .. 2^30 rows");
    if (a.ac < 1 || a.rows % a.ac) return fail(FMRX_EINVAL, "highcut: rows %zu are not whole groups of %d audio channels", a.rows, a.ac);
    const long rows = static_cast<long>(a.rows);
    const int n = static_cast<int>(a.n);
    if (serial) {
        highcut_serial_kernel<<<walk::serial_blocks(rows), kLanes, 0, s>>>(a.x, a.y, a.pcm, a.ac, a.wrap, rows, n, a.status, a.inv_n, a.p_max, a.state);
        FMRX_LAUNCH_CHECK("highcut_serial_kernel");
        return FMRX_OK;
    }
    if (!a.seg || !a.missed || a.L < 1 || a.W < 0) return fail(FMRX_EINVAL, "highcut: null scratch or no lane shape");
    walk::Grid g;
    FMRX_TRY(walk::grid("highcut", rows, a.n, a.L, &g));
    highcut_segments_kernel<<<g.blocks, kLanes, 0, s>>>(a.x, a.y, a.pcm, a.ac, a.wrap, rows, n, static_cast<int>(g.nseg), a.L, a.W, a.status, a.inv_n,
                                                        a.p_max, a.state, a.seg);
    FMRX_LAUNCH_CHECK("highcut_segments_kernel");
    highcut_verify_kernel<<<static_cast<unsigned>(rows), g.verify_lanes, 0, s>>>(a.x, a.y, a.pcm, a.ac, a.wrap, rows, n, static_cast<int>(g.nseg), a.L,
                                                                                  a.status, a.inv_n, a.p_max, a.state, a.seg, a.missed);
    FMRX_LAUNCH_CHECK("highcut_verify_kernel");
    if (segments) *segments += g.checked;
    return FMRX_OK;
}

}  // namespace fmrx
