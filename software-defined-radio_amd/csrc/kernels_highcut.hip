// kernels_highcut.hip -- the kernels of the variable high-cut stage (include/fmrx.h: fmrx_highcut_*; DESIGN.md section 4.13;
// defined by tests/_highcut_model.py).
//
// The definition.  Per row, state y_prev, +0 at the start of a stream; sample k of the call's n:
//     p[k] = clamp(fmaf((float)(k + 1), (p1 - p0) * inv_n, p0), 0, p_max);  q = 1 - p[k];  v = q * x[k]
//     y = fmaf(p[k], y_prev, v);  if |y| < 2^-126: y = +0;  y[k] = p[k] == 0 ? x[k] : y
// with (p0, p1) from the status row of the row's channel.  The flush is there for the reason kernels_deemph.hip gives; the
// select makes a channel at cut 0 return its input's bits.
//
//   highcut_control_kernel   one lane per channel runs control_step (highcut_control.hpp) on the channel's probe powers, where
//                            the meters' MPX pass left them, and its status row -- state and result at once.
//   highcut_segments_kernel  parallel in time, the scheme of deemph_segments_kernel with a pole that moves inside the call.  A
//                            lane owns one (row, segment of L samples): it starts W samples early with y = +0, or at sample 0 from
//                            the carried state where its warm-up would begin in front of the call; it remembers the y it has
//                            reached at its segment's start, writes its L outputs and leaves its end y.  Every lane computes
//                            p[k] from k itself, so a lane's pole is the serial walk's at every sample; p[k] <= p_max < 1 keeps
//                            the recurrence a contraction.  64 lanes per workgroup, batches of 32 steps staged through LDS
//                            exactly as the de-emphasis does (row stride 33 words).  p[k], q and v do not depend on y: only the
//                            fused multiply-add, the flush and the select are on the dependent chain.
//   highcut_verify_kernel    one workgroup per row.  Segment c is right iff the bits of its start y equal segment c-1's true end
//                            (two NaNs count as equal); a miss is walked again by one lane from the true state until a
//                            recomputed y has the stored one's bits.  Leaves the row's carried state and counts the misses.
//   highcut_serial_kernel    one lane per row walks the whole row: the yardstick, and fmrx_highcut_set_force's path.
// All three write through highcut_write: f32 [rows][n] and PCM [row / ac][k][row % ac].  The walk is out of place (the lanes'
// warm-up and the repair read x again): highcut.hip gives it a copy where the caller's d_out is d_in.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4.13; no kernel uses scratch.
#include "device_math.hpp"
#include "fmrx_internal.hpp"
#include "highcut_control.hpp"

namespace fmrx {
namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 64, kBatch = 32, kStride = kBatch + 1;

__global__ __launch_bounds__(kThreads) void highcut_control_kernel(highcut::Control c, const double *__restrict__ mpx,
                                                                   const unsigned long long *__restrict__ seg_each,
                                                                   unsigned long long seg_all, fmrx_highcut_status *__restrict__ st,
                                                                   unsigned n_channels)
{
    const unsigned i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_channels) return;
    const double *probe = mpx + static_cast<size_t>(i) * kMetersMpxFields + 3;   // behind sum_x, sum_x2, max_abs
    fmrx_highcut_status s = st[i];
    highcut::control_step(c, probe, seg_each ? seg_each[i] : seg_all, s);
    st[i] = s;
}

// a row's pole ramp: p[k] = clamp(fmaf(k + 1, step, p0), 0, p_max)
struct Pole {
    float p0, step, p_max;
    __device__ __forceinline__ float at(int k) const
    {
        const float x = fmaf(static_cast<float>(k + 1), step, p0);
        return x < 0.0f ? 0.0f : (x > p_max ? p_max : x);
    }
};

__device__ __forceinline__ Pole highcut_pole(const fmrx_highcut_status *__restrict__ st, long row, int ac, float inv_n, float p_max)
{
    const fmrx_highcut_status *s = st + row / ac;
    const float p0 = s->p0, p1 = s->p1;
    return Pole{p0, (p1 - p0) * inv_n, p_max};
}

__device__ __forceinline__ float highcut_step(float x, float p, float y_prev)
{
    const float q = 1.0f - p;
    const float v = q * x;
    const float y = __builtin_fmaf(p, y_prev, v);
    const float f = __builtin_fabsf(y) < 1.17549435e-38f ? 0.0f : y;
    return p == 0.0f ? x : f;
}

__device__ __forceinline__ bool highcut_same(float a, float b)
{
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

// PCM of row r: [row / ac][k][row % ac]; sample k of a row sits k * ac behind the row's first
__device__ __forceinline__ long highcut_pcm_row(long row, int n, int ac) { return (row / ac) * n * ac + row % ac; }

// the one writer: sample k of a row, f32 and PCM
__device__ __forceinline__ void highcut_write(float *y_row, int16_t *pcm_row, int k, int ac, float v, int wrap)
{
    y_row[k] = v;
    if (pcm_row) pcm_row[static_cast<long>(k) * ac] = pcm_pack(v, wrap);
}

// lane (2 it + half)'s value of v: two scalar reads and a select
__device__ __forceinline__ int highcut_pick(int v, int it, int half)
{
    const int a = __builtin_amdgcn_readlane(v, 2 * it), b = __builtin_amdgcn_readlane(v, 2 * it + 1);
    return half ? b : a;
}

__global__ __launch_bounds__(kLanes) void highcut_segments_kernel(const float *__restrict__ x, float *__restrict__ y, int16_t *__restrict__ pcm,
                                                                  int ac, int wrap, long rows, int n, int nseg, int L, int W,
                                                                  const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                  const float *__restrict__ state, float *__restrict__ seg)
{
    __shared__ float buf[kLanes * kStride];
    const int tid = threadIdx.x;
    const long total = rows * nseg;
    const long t = static_cast<long>(blockIdx.x) * kLanes + tid;
    const bool ok = t < total;
    const long row = ok ? t / nseg : 0;
    const int c = ok ? static_cast<int>(t - row * nseg) : 0;
    const int g0 = c * L - W;                      // where the warm-up would begin; <= 0: the lane starts at sample 0, exact
    // what the staging loops need of every lane: its row, where it starts (a lane past the end: so early that it never meets
    // sample 0), and its row's place in the PCM
    const int lane_row = static_cast<int>(row), lane_g0 = ok ? g0 : -(1 << 30);
    const long pcm_row = highcut_pcm_row(row, n, ac);
    const int pcm_lo = static_cast<int>(pcm_row), pcm_hi = static_cast<int>(pcm_row >> 32);
    const int steps = W + L;
    const Pole pole = highcut_pole(st, row, ac, inv_n, p_max);
    float yp = (ok && g0 <= 0) ? state[row] : 0.0f, ystart = 0.0f;
    const int e = tid & (kBatch - 1), half = tid >> 5;
    for (int j0 = 0; j0 < steps; j0 += kBatch) {
        float in[kLanes / 2];   // all of the batch's loads in flight at once, then LDS
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = highcut_pick(lane_row, it, half);
            const int j = j0 + e, g = highcut_pick(lane_g0, it, half) + j;
            in[it] = 0.0f;
            if (j < steps && g >= 0 && g < n) in[it] = x[r * n + g];
        }
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) buf[(2 * it + half) * kStride + e] = in[it];
        __syncthreads();
        float xs[kBatch];   // the lane's row in registers: the LDS latency stays off the dependent chain
#pragma unroll
        for (int i = 0; i < kBatch; i++) xs[i] = buf[tid * kStride + i];
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const int j = j0 + i, g = g0 + j;
            const bool act = ok && j < steps && g >= 0 && g < n;
            ystart = j == W ? yp : ystart;
            const float yv = highcut_step(xs[i], pole.at(g), yp);
            yp = act ? yv : yp;
            xs[i] = yp;
        }
#pragma unroll
        for (int i = 0; i < kBatch; i++) buf[tid * kStride + i] = xs[i];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = highcut_pick(lane_row, it, half);
            const int j = j0 + e, g = highcut_pick(lane_g0, it, half) + j;
            const long po = (static_cast<long>(highcut_pick(pcm_hi, it, half)) << 32) | static_cast<unsigned>(highcut_pick(pcm_lo, it, half));
            const float v = buf[(2 * it + half) * kStride + e];
            if (j >= W && j < steps && g >= 0 && g < n) highcut_write(y + r * n, pcm ? pcm + po : nullptr, g, ac, v, wrap);
        }
        __syncthreads();
    }
    if (ok) {
        seg[t] = ystart;
        seg[total + t] = yp;
    }
}

constexpr int kScan = 8;           // segments every lane checks per pass
constexpr int kVerifyMax = 1024;   // lanes per row at most

// (seg is read and written here: no __restrict__, no const)
__global__ __launch_bounds__(kVerifyMax) void highcut_verify_kernel(const float *__restrict__ x, float *y, int16_t *pcm, int ac, int wrap,
                                                                   long rows, int n, int nseg, int L,
                                                                   const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                   float *__restrict__ state, float *seg, unsigned long long *missed)
{
    __shared__ int first, resume;
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const float *xr = x + row * n;
    float *yr = y + row * n;
    float *start = seg + row * nseg, *end = seg + rows * nseg + row * nseg;
    int16_t *pcm_row = pcm ? pcm + highcut_pcm_row(row, n, ac) : nullptr;
    const Pole pole = highcut_pole(st, row, ac, inv_n, p_max);
    unsigned miss = 0;
    int from = 1;
    while (from < nseg) {
        const int nt = blockDim.x;
        const int hi = from + kScan * nt < nseg ? from + kScan * nt : nseg;
        if (tid == 0) first = nseg;
        __syncthreads();
        int found = nseg;
#pragma unroll
        for (int u = kScan - 1; u >= 0; u--) {   // (no early exit: the loads of a pass are independent)
            const int c = from + u * nt + tid;
            if (c < hi && !highcut_same(start[c], end[c - 1])) found = c;
        }
        if (found < nseg) atomicMin(&first, found);
        __syncthreads();
        const int f = first;
        __syncthreads();   // (everybody has read it before lane 0 writes it again)
        if (f >= nseg) {
            from = hi;
            continue;
        }
        if (tid == 0) {
            // everything in front of segment f is true: walk f again from its predecessor's end, and on through the segments
            // behind it for as long as the walk does not meet the stored values
            int c = f;
            float yv = end[c - 1];
            for (;;) {
                miss++;
                const int g_lo = c * L, g_hi = g_lo + L < n ? g_lo + L : n;
                bool met = false;
                for (int g = g_lo; g < g_hi && !met; g += 8) {
                    float xs[8], ys[8];   // eight samples' loads in flight at once: the walk itself is a dependent chain
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        xs[i] = g + i < g_hi ? xr[g + i] : 0.0f;
                        ys[i] = g + i < g_hi ? yr[g + i] : 0.0f;
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        if (met || g + i >= g_hi) break;
                        yv = highcut_step(xs[i], pole.at(g + i), yv);
                        if (highcut_same(yv, ys[i])) met = true;
                        else highcut_write(yr, pcm_row, g + i, ac, yv, wrap);
                    }
                }
                c++;
                if (met || c >= nseg) {
                    if (!met) end[c - 1] = yv;
                    break;
                }
                end[c - 1] = yv;
                if (highcut_same(start[c], yv)) {   // the next segment started from exactly this: it and its end are true
                    c++;
                    break;
                }
            }
            resume = c;
        }
        __syncthreads();
        from = resume;
    }
    if (tid == 0) {
        state[row] = end[nseg - 1];
        if (miss) atomicAdd(missed, static_cast<unsigned long long>(miss));
    }
}

__global__ __launch_bounds__(kLanes) void highcut_serial_kernel(const float *__restrict__ x, float *__restrict__ y, int16_t *__restrict__ pcm,
                                                                int ac, int wrap, long rows, int n,
                                                                const fmrx_highcut_status *__restrict__ st, float inv_n, float p_max,
                                                                float *__restrict__ state)
{
    const long row = static_cast<long>(blockIdx.x) * kLanes + threadIdx.x;
    if (row >= rows) return;
    const float *xr = x + row * n;
    float *yr = y + row * n;
    int16_t *pcm_row = pcm ? pcm + highcut_pcm_row(row, n, ac) : nullptr;
    const Pole pole = highcut_pole(st, row, ac, inv_n, p_max);
    float yp = state[row];
    for (int g = 0; g < n; g += 8) {
        float xs[8];
#pragma unroll
        for (int i = 0; i < 8; i++) xs[i] = g + i < n ? xr[g + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (g + i >= n) break;
            yp = highcut_step(xs[i], pole.at(g + i), yp);
            highcut_write(yr, pcm_row, g + i, ac, yp, wrap);
        }
    }
    state[row] = yp;
}

}  // namespace

int highcut_control_launch(const highcut::Control &c, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all,
                           fmrx_highcut_status *d_status, int n_channels, hipStream_t s)
{
    const unsigned grid = (static_cast<unsigned>(n_channels) + kThreads - 1) / kThreads;
    highcut_control_kernel<<<grid, kThreads, 0, s>>>(c, d_mpx, d_seg_each, seg_all, d_status, static_cast<unsigned>(n_channels));
    FMRX_LAUNCH_CHECK("highcut_control_kernel");
    return FMRX_OK;
}

long highcut_segments(size_t n, int L) { return static_cast<long>((n + static_cast<size_t>(L) - 1) / static_cast<size_t>(L)); }

int highcut_apply_launch(const HighcutArgs &a, bool serial, hipStream_t s, unsigned long long *segments)
{
    if (!a.x || !a.y || !a.status || !a.state) return fail(FMRX_EINVAL, "highcut: null buffer");
    if (a.x == a.y) return fail(FMRX_EINVAL, "highcut: the walk is out of place (warm-up and repair read x again)");
    if (a.rows < 1 || a.n < 1 || a.n > (size_t{1} << 26) || a.rows > (size_t{1} << 30)) return fail(FMRX_EINVAL, "highcut: 1 .. 2^26 samples per row, 1 .. 2^30 rows");
    if (a.ac < 1 || a.rows % a.ac) return fail(FMRX_EINVAL, "highcut: rows %zu are not whole groups of %d audio channels", a.rows, a.ac);
    const long rows = static_cast<long>(a.rows);
    const int n = static_cast<int>(a.n);
    if (serial) {
        highcut_serial_kernel<<<static_cast<unsigned>((rows + kLanes - 1) / kLanes), kLanes, 0, s>>>(a.x, a.y, a.pcm, a.ac, a.wrap, rows, n, a.status,
                                                                                                     a.inv_n, a.p_max, a.state);
        FMRX_LAUNCH_CHECK("highcut_serial_kernel");
        return FMRX_OK;
    }
    if (!a.seg || !a.missed || a.L < 1 || a.W < 0) return fail(FMRX_EINVAL, "highcut: null scratch or no lane shape");
    const long nseg = highcut_segments(a.n, a.L);
    const long total = rows * nseg;
    if ((total + kLanes - 1) / kLanes > 0x7fffffffL || rows > 0x7fffffffL) return fail(FMRX_EINVAL, "highcut: too many segments");
    highcut_segments_kernel<<<static_cast<unsigned>((total + kLanes - 1) / kLanes), kLanes, 0, s>>>(a.x, a.y, a.pcm, a.ac, a.wrap, rows, n,
                                                                                                    static_cast<int>(nseg), a.L, a.W, a.status,
                                                                                                    a.inv_n, a.p_max, a.state, a.seg);
    FMRX_LAUNCH_CHECK("highcut_segments_kernel");
    const long vt = (nseg + kLanes - 1) / kLanes * kLanes;   // lanes per row: whole waves, enough to check a row's segments in few passes
    highcut_verify_kernel<<<static_cast<unsigned>(rows), static_cast<unsigned>(vt < kVerifyMax ? vt : kVerifyMax), 0, s>>>(
        a.x, a.y, a.pcm, a.ac, a.wrap, rows, n, static_cast<int>(nseg), a.L, a.status, a.inv_n, a.p_max, a.state, a.seg, a.missed);
    FMRX_LAUNCH_CHECK("highcut_verify_kernel");
    if (segments) *segments += static_cast<unsigned long long>(rows) * static_cast<unsigned long long>(nseg - 1);
    return FMRX_OK;
}

}  // namespace fmrx
